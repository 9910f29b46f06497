"""CPU: the float action granules of the host env pool (include/a2c_hostpool.h, "CONTINUOUS actions") without a GPU --
the layout (and that an int pool's is untouched), the bit-exact round trip GPU-process side -> worker side, that a torn
delivery is never handed out, a ProcessEnvPool(action_dim=n) against the same envs stepped in this process, and the
protocol under the sanitizers as a stand-alone C program (tests/c/hostpool_f32_stress.c)."""
import ctypes
import mmap
import os
import shutil
import subprocess

import numpy as np
import pytest

import cont_cases as CC
from cases import hashf
from a2c_amd.hostpool import FRAME_BITS, FRAME_F32, FRAME_U8, ROLLOUT, PoolHeader, ProcessEnvPool, pool_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xffffffffffffffff


def _up(x, a):
    return (x + a - 1) // a * a


class _Mem:
    """a page-aligned, zero-filled region of this process with numpy views of its granules"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mm = mmap.mmap(-1, nbytes)
        self._buf = (ctypes.c_char * nbytes).from_buffer(self.mm)
        self.base = ctypes.addressof(self._buf)
        self.h = PoolHeader.from_buffer(self.mm)
        self.bytes = np.frombuffer(self.mm, dtype=np.uint8)

    def u64(self, off, count):
        return self.bytes[off:off + 8 * count].view(np.uint64)

    @property
    def cmd(self):
        return self.u64(self.h.off_cmd, self.h.n_envs)

    @property
    def act(self):
        return self.u64(self.h.off_act, self.h.n_envs * self.h.act_stride).reshape(self.h.n_envs, self.h.act_stride)


def _f32_pool(n_envs, act_dim, frame_bytes=20):
    lib = pool_lib()
    m = _Mem(lib.a2c_pool_bytes_f32(n_envs, frame_bytes, act_dim))
    assert lib.a2c_pool_init(m.base, m.nbytes, n_envs, frame_bytes, FRAME_F32, 1, -1.0) == 0
    assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, act_dim) == 0
    lib.a2c_pool_set_phase(m.base, ROLLOUT)
    return m


# ------------------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("n_envs,frame_bytes", [(1, 20), (3, 7056), (256, 882)])
def test_int_pool_layout_is_unchanged_and_the_block_sits_behind_it(n_envs, frame_bytes):
    lib = pool_lib()
    # the formula of the header comment: header | cmd | rec | frames, every block page aligned, slots 16 B apart at least
    granules = _up(8 * n_envs, 4096)
    want_total = _up(4096 + 2 * granules + n_envs * _up(frame_bytes, 16), 4096)
    assert lib.a2c_pool_bytes(n_envs, frame_bytes) == want_total
    m = _Mem(want_total)
    assert lib.a2c_pool_init(m.base, m.nbytes, n_envs, frame_bytes, FRAME_U8, 1, -1.0) == 0
    h = m.h
    assert (h.total_bytes, h.off_cmd, h.off_rec, h.off_frames) == (want_total, 4096, 4096 + granules, 4096 + 2 * granules)
    assert h.off_act == 0 and h.act_dim == 0 and h.act_stride == 0 and h.off_tagged == 0 and h.version == 3
    assert ctypes.sizeof(PoolHeader) <= 4096 and PoolHeader.off_act.offset % 8 == 0
    # an int pool has no room for the block: enabling it is refused and changes nothing
    before = bytes(m.bytes[:4096])
    assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, 6) == -1
    assert bytes(m.bytes[:4096]) == before
    for act_dim in (1, 6, 64):
        total = lib.a2c_pool_bytes_f32(n_envs, frame_bytes, act_dim)
        assert total > want_total and total % 4096 == 0
        m = _Mem(total)
        assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, act_dim) == -1           # not formatted yet
        assert lib.a2c_pool_init(m.base, m.nbytes, n_envs, frame_bytes, FRAME_U8, 1, -1.0) == 0
        for bad in (0, 65, -1):
            assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, bad) == -1
        assert lib.a2c_pool_enable_actions_f32(m.base, want_total, act_dim) == -1         # region too small
        assert m.h.off_act == 0 and m.h.total_bytes == want_total
        assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, act_dim) == 0
        h = m.h
        assert (h.off_cmd, h.off_rec, h.off_frames) == (4096, 4096 + granules, 4096 + 2 * granules)
        assert h.off_act % 8 == 0 and h.off_act >= h.off_frames + n_envs * h.frame_stride
        assert h.act_dim == act_dim and h.act_stride >= act_dim
        assert h.total_bytes == total and h.off_act + 8 * n_envs * h.act_stride <= total
        assert (m.act == ONES).all() and (m.cmd == ONES).all()
        assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, act_dim) == -1           # a second time
    assert lib.a2c_pool_bytes_f32(n_envs, frame_bytes, 0) == 0 and lib.a2c_pool_bytes_f32(n_envs, frame_bytes, 65) == 0


def test_block_sits_behind_the_tagged_mirror():
    lib = pool_lib()
    n_envs, elems, act_dim = 3, 7056, 6
    fb = (elems + 7) // 8
    tagged_total = lib.a2c_pool_bytes_tagged(n_envs, fb, elems)
    total = tagged_total + lib.a2c_pool_bytes_f32(n_envs, fb, act_dim) - lib.a2c_pool_bytes(n_envs, fb)
    m = _Mem(total)
    assert lib.a2c_pool_init(m.base, m.nbytes, n_envs, fb, FRAME_BITS, 1, -1.0) == 0
    lib.a2c_pool_set_frame_elems(m.base, elems)
    assert lib.a2c_pool_enable_tagged(m.base, m.nbytes) == 0
    assert m.h.total_bytes == tagged_total
    assert lib.a2c_pool_enable_actions_f32(m.base, tagged_total, act_dim) == -1
    assert lib.a2c_pool_enable_actions_f32(m.base, m.nbytes, act_dim) == 0
    h = m.h
    assert h.off_act % 8 == 0 and h.off_act >= h.off_tagged + n_envs * h.tagged_stride and h.total_bytes == total
    assert (m.act == ONES).all()


# --------------------------------------------------------------------------------------------- 2. bit-exact round trip
PATTERNS = np.array([0x00000000, 0x80000000, 0x00000001, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001],
                    dtype=np.uint32)     # +0, -0, smallest subnormal, FLT_MAX, +inf, -inf, quiet NaNs with payloads


def _take(lib, m, next_seq, spin_ns=20_000_000):
    out = np.full(m.h.act_dim, 7.25, dtype=np.float32)
    i = lib.a2c_pool_take_f32(m.base, 0, len(next_seq), next_seq.ctypes.data, spin_ns, out.ctypes.data)
    return i, out


@pytest.mark.parametrize("n_envs", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 6, 64])
def test_round_trip_is_bit_exact(n, n_envs):
    lib = pool_lib()
    m = _f32_pool(n_envs, n)
    stride = n + 3                                           # a non-dense row stride
    pool_bits = np.concatenate([PATTERNS, hashf(64, 300 + n, -3, 3).view(np.uint32)])
    for step, seq in enumerate((0xfffffffe, 0xffffffff, 0, 1)):          # the step counter wraps
        rows = np.full((n_envs, stride), 0xdeadbeef, dtype=np.uint32)
        for j in range(n_envs):
            rows[j, :n] = pool_bits[(np.arange(n) + 5 * j + 11 * step) % len(pool_bits)]
        lib.a2c_pool_post_actions_f32(m.base, 0, n_envs, rows.view(np.float32).ctypes.data, stride, seq)
        assert (m.cmd == ((seq << 32) | n)).all()
        assert (m.act[:, :n] == ((np.uint64(seq) << np.uint64(32)) | rows[:, :n].astype(np.uint64))).all()
        assert (m.act[:, n:] == ONES).all()                  # the padding granules of a row are never written
        next_seq = np.full(n_envs, seq, dtype=np.uint32)
        seen = set()
        for _ in range(n_envs):
            i, out = _take(lib, m, next_seq)
            assert 0 <= i < n_envs and i not in seen
            seen.add(i)
            assert np.array_equal(out.view(np.uint32), rows[i, :n]), (seq, i)
            next_seq[i] = (seq + 1) & 0xffffffff
        i, out = _take(lib, m, next_seq, spin_ns=1_000_000)  # nothing further was posted
        assert i == -1 and (out == 7.25).all()
    # a part of the pool: envs 1.. only
    if n_envs == 3:
        rows = hashf(2 * n, 77, -1, 1).reshape(2, n)
        lib.a2c_pool_post_actions_f32(m.base, 1, 2, rows.ctypes.data, n, 2)
        assert m.cmd[0] == ((1 << 32) | n) and (m.cmd[1:] == ((2 << 32) | n)).all()
        ns = np.full(2, 2, dtype=np.uint32)
        out = np.zeros(n, dtype=np.float32)
        assert lib.a2c_pool_take_f32(m.base, 1, 2, ns.ctypes.data, 20_000_000, out.ctypes.data) == 0
        assert np.array_equal(out.view(np.uint32), rows[0].view(np.uint32))


def test_take_f32_sees_shutdown_and_refuses_an_int_pool():
    lib = pool_lib()
    m = _f32_pool(2, 3)
    lib.a2c_pool_set_phase(m.base, 2)
    ns = np.zeros(2, dtype=np.uint32)
    out = np.zeros(3, dtype=np.float32)
    assert lib.a2c_pool_take_f32(m.base, 0, 2, ns.ctypes.data, 5_000_000, out.ctypes.data) == -2
    # the doorbell is there, one granule is missing, and the pool shuts down: -2, nothing handed out
    m = _f32_pool(1, 2)
    m.cmd[0] = (0 << 32) | 2
    m.act[0, 0] = 0x3f800000
    lib.a2c_pool_set_phase(m.base, 2)
    assert lib.a2c_pool_take_f32(m.base, 0, 1, ns.ctypes.data, 5_000_000, out.ctypes.data) == -2 and (out == 0).all()
    im = _Mem(lib.a2c_pool_bytes(2, 20))
    assert lib.a2c_pool_init(im.base, im.nbytes, 2, 20, FRAME_F32, 1, -1.0) == 0
    lib.a2c_pool_set_phase(im.base, ROLLOUT)
    assert lib.a2c_pool_take_f32(im.base, 0, 2, ns.ctypes.data, 1_000_000, out.ctypes.data) == -1


# ----------------------------------------------------------------------------------------------- 3. torn delivery
@pytest.mark.parametrize("stale", ["previous step", "never written"])
def test_torn_delivery_is_never_handed_out(stale):
    lib = pool_lib()
    n, s = 6, 41
    m = _f32_pool(2, n)
    want = hashf(n, 900, -2, 2)
    bits = want.view(np.uint32).astype(np.uint64)
    if stale == "previous step":      # the whole vector of step s - 1 is still there
        old = hashf(n, 901, -2, 2).view(np.uint32).astype(np.uint64)
        m.act[1, :n] = (np.uint64(s - 1) << np.uint64(32)) | old
    # the doorbell of step s and only n - 1 granules of it: the last one has not arrived
    m.act[1, :n - 1] = (np.uint64(s) << np.uint64(32)) | bits[:n - 1]
    m.cmd[1] = (s << 32) | n
    assert m.act[1, n - 1] >> np.uint64(32) == (s - 1 if stale == "previous step" else 0xffffffff)
    next_seq = np.array([s, s], dtype=np.uint32)
    i, out = _take(lib, m, next_seq, spin_ns=3_000_000)
    assert i == -1 and (out == 7.25).all()
    i, out = _take(lib, m, next_seq, spin_ns=3_000_000)      # polling again changes nothing
    assert i == -1 and (out == 7.25).all()
    m.act[1, n - 1] = (np.uint64(s) << np.uint64(32)) | bits[n - 1]
    i, out = _take(lib, m, next_seq)
    assert i == 1 and np.array_equal(out.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------ 4. process pool against in-process envs
class FailingContEnv(CC.ContEnv):
    def step(self, a):
        if self.t >= 2 and self.env_id == 1:
            raise RuntimeError("env crashed (test)")
        return super().step(a)


@pytest.mark.parametrize("n", [1, 2])
def test_process_pool_matches_in_process_envs(n):
    B, K = 3, 12
    kws = [dict(n=n, env_id=j, done_period=4 + j, prepped=True) for j in range(B)]
    pool = ProcessEnvPool(CC.ContEnv, B, env_kwargs=kws, n_workers=2, register=False, action_dim=n)
    try:
        pool.start()
        h = pool.header
        assert pool.act_dim == n and h.act_dim == n and h.off_act and pool.dev_act == 0
        assert h.total_bytes == pool_lib().a2c_pool_bytes_f32(B, h.frame_bytes, n)
        assert pool.frame_dtype == np.float32 and pool.frame_shape == (1, 1, CC.D_OBS)
        pool.set_phase(ROLLOUT)
        refs = [CC.ContEnv(**kw) for kw in kws]
        fr = pool.frames_view()
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.float32)
        pool.wait_frames(0)
        pool.unpack(rew, done)
        assert (done == 1).all() and (rew == 0).all()
        for j in range(B):
            assert np.array_equal(fr[j], refs[j].reset())
        n_done = 0
        for k in range(K):
            acts = hashf(B * n, 700 + k, -2, 2).reshape(B, n)
            pool.post_actions(acts, seq=k)
            pool.wait_frames(k + 1)
            pool.unpack(rew, done)
            for j in range(B):
                obs, r, d, _ = refs[j].step(acts[j] + np.float32(0))
                if d:
                    obs = refs[j].reset()
                assert np.array_equal(fr[j], obs), (k, j)
                # the reward depends on every component of the action: the worker received exactly these floats
                assert rew[j] == np.float32(r) and done[j] == float(d), (k, j, rew[j], r)
                n_done += int(d)
        assert pool.header.episodes == n_done and n_done > 0
    finally:
        pool.close()
    assert not os.path.exists("/dev/shm/" + pool.name)


def test_int_pool_is_what_it_was_and_refuses_nothing_new():
    """action_dim unset: no block, int64 actions in post_actions; action_dim out of range is refused"""
    with pytest.raises(ValueError):
        ProcessEnvPool(CC.ContEnv, 1, env_kwargs=[dict(n=1, prepped=True)], n_workers=1, register=False, action_dim=65)
    with pytest.raises(ValueError):
        ProcessEnvPool(CC.ContEnv, 1, env_kwargs=[dict(n=1, prepped=True)], n_workers=1, register=False, action_dim=0)
    pool = ProcessEnvPool(CC.ContEnv, 1, env_kwargs=[dict(n=1, prepped=True)], n_workers=1, register=False)
    assert pool.act_dim == 0


def test_worker_exception_reaches_the_gpu_process():
    B, n = 3, 2
    kws = [dict(n=n, env_id=j, prepped=True) for j in range(B)]
    pool = ProcessEnvPool(FailingContEnv, B, env_kwargs=kws, n_workers=2, register=False, action_dim=n)
    try:
        pool.start()
        pool.set_phase(ROLLOUT)
        acts = np.zeros((B, n), np.float32)
        with pytest.raises(RuntimeError, match="env worker"):
            for k in range(5):
                pool.post_actions(acts, seq=k)
                pool.wait_frames(k + 1, timeout=20.0)
        assert pool.header.worker_error
    finally:
        pool.close()


# ------------------------------------------------------------------------------------- 5. sanitizers, stand-alone
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_protocol_under_sanitizers_stand_alone(tmp_path, sanitizer):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    base = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, "-pthread"]
    # the runtimes linked statically where the compiler can (a program then does not depend on the order in which shared
    # libraries were loaded into it), else as the compiler links them by default
    static = ["-static-lib" + {"address": "asan", "undefined": "ubsan", "thread": "tsan"}[s] for s in sanitizer.split(",")]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for flags in (base + static, base):
        if subprocess.run([cc, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the compiler cannot link the runtime of -fsanitize=" + sanitizer)
    # can the runtime start a program here at all?  (ThreadSanitizer refuses address-space layouts it does not know:
    # "unexpected memory mapping" on kernels with a large mmap_rnd_bits)
    if subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("an empty program built with -fsanitize=%s does not start on this machine" % sanitizer)
    exe = tmp_path / "stress"
    build = subprocess.run([cc, *flags, os.path.join(ROOT, "tests", "c", "hostpool_f32_stress.c"),
                            os.path.join(ROOT, "pytorch-a2c_amd", "csrc", "hostpool.c"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ")
