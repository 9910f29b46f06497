"""-m gpu: the per-step rollout kernels of csrc/rollout_ops.hip -- a2c_rollout_record, a2c_rollout_post / _u8 / _rec,
a2c_rollout_post_frames, a2c_rollout_bootstrap, a2c_frame_stack_push[_u8], a2c_frames_to_states, a2c_frame_store_begin,
a2c_frame_prep_u8 and a2c_copy_rows / a2c_mask_rows / a2c_permute_rows -- called through the C ABI (a2c_amd.ops, or _lib
where a wrapper hides a stride or a crop), in every branch their launch geometry has.

Criterion: np.array_equal with a NumPy float32 twin of the env step (tests/test_rollout_ops_twin.py), for EVERY buffer a
call is handed, in full.  These kernels are documented as exact -- copies, uint8 -> fp32 expansions, integer counters and
one fixed chain of rounded float32 operations -- so there is no tolerance in this file.  The twin itself is held to
oracle.a2c_oracle.SlotRunner on the CPU, bit for bit, in that file.  Every rollout buffer is allocated for more slots than
a call covers (below slot0 and above slot0 + B) and filled with a sentinel of its own beforehand, carries and padded rows
too: an element written that the env step does not own (the previous slot's last delta at t == 0, the next slot's first
valid-plane count at t == T - 1, a row outside [slot0, slot0 + B), the padding of a strided row) fails the comparison like
a wrong value does.  The forms of an env step are compared with the twin, never with each other.

Shapes are the smallest at which each branch exists: B around the 256 envs of a bookkeeping block, hdim around the 256
lanes of the hidden-row loop, HW = 8204 (2051 float4, past the 8 x 256 x-cap of the frame-stack grids, ragged tail),
16389 columns and 32769 rows for a2c_copy_rows' caps, 2048 * 256 + 7 elements for a2c_permute_rows', 600 slots x 128
steps for the second launch of a2c_frames_to_states.

Not covered here, on purpose: the samplers, a2c_eval_scan, a2c_unpack_bits, the scans and the pool ingest kernels (files
of their own); valid-plane counts past 4 (a2c_rollout_post_frames saturates at 4 and Runner._frame_store refuses any
other n_frame_stack, asserted in test_rollout_ops_twin.py); what the kernels do with NaN inputs.

Wall time of the file on an MI355X: 1.1 s of test calls inside a run of the whole suite (test_gpu_small_kernels.py: 4.8 s
in the same run, 5.1 s by its docstring); 4.0 s on its own, start-up included.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_rollout_ops_twin import (NV_CAP, new_carry, new_rollout, rndf, twin_begin, twin_bootstrap,  # noqa: E402
                                   twin_frames_to_states, twin_step, twin_store_begin)

DEV = "cuda"
ERR_ARG = -1
SENT = 12345.6787109375            # sentinel value (an exact float32); every buffer gets SENT + k of its own
FILL = dict(rewards=SENT, dones=SENT + 1, deltas=SENT + 2, states=SENT + 3, h_states=SENT + 4, nvalid=-77)
CFILL = dict(done_eff=SENT + 5, state=SENT + 6, h=SENT + 7, val_prev=SENT + 8, nv=-55)
PADV = SENT + 9                    # padding of strided rows
PAD = 8                            # floats (or bytes) of padding behind a strided row
GAMMA = 0.99
DONE_VALUES = np.array([0, 0, 0, 0, 1, 2, -1, 0.5], np.float32)      # any nonzero is a done


def _ops():
    from a2c_amd import ops
    return ops


def _raw():
    from a2c_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _eq(tag, got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{tag}: {len(bad)} of {got.size} elements differ, first at {i}: got {got[i]!r} want {want[i]!r}")


# ================================================================================== one env step: buffers, inputs, forms
STATE_FORMS = ("push", "push_u8", "post", "post_u8", "post_rec", "post_rec_u8", "record+push")
U8_FORMS = ("push_u8", "post_u8", "post_rec_u8")
BOOK = ("rewards", "dones", "deltas", "val_prev")
PRODUCES = {"record": BOOK + ("done_eff",), "record_h": BOOK + ("done_eff", "h"), "push": ("states", "state"),
            "push_u8": ("states", "state"), "post": BOOK + ("states", "state"), "post_u8": BOOK + ("states", "state"),
            "post_rec": BOOK + ("states", "state", "done_eff", "h", "h_states"),
            "post_rec_u8": BOOK + ("states", "state", "done_eff", "h", "h_states"),
            "frames": BOOK + ("done_eff", "nvalid", "nv"), "frames_h": BOOK + ("done_eff", "nvalid", "nv", "h", "h_states"),
            "record+push": BOOK + ("done_eff", "states", "state")}
RECURRENT = ("record_h", "post_rec", "post_rec_u8", "frames_h")


def _setup(B, T, t, slot0, C, HW, hdim, seed):
    """twin buffers at their sentinels, with what step t reads from before it filled in: the state of step t, the rewards /
    dones rows of step t - 1, the carried values and counts"""
    n_slots = slot0 + B + 2
    D = new_rollout(n_slots, T, C, HW, hdim, FILL)
    car = new_carry(B, C, HW, hdim, CFILL)
    e = (slot0 + np.arange(B)) * T + t
    car["val_prev"][:] = rndf(B, seed + 100, -3, 3)
    car["nv"][:] = 1 + (np.arange(B) + seed) % NV_CAP
    if C:
        D["states"][e] = rndf((B, C, HW), seed + 101, 0, 1)
    if t > 0:
        D["rewards"][e - 1] = rndf(B, seed + 102, -2, 2)
        D["dones"][e - 1] = rndf(B, seed + 103, 0, 1) < 0.4
    if hdim:
        car["h"][:] = rndf((B, hdim), seed + 104)
    return D, car


def _inputs(B, HW, hdim, seed):
    X = {}
    rew = rndf(B, seed + 200, -2, 2)
    rew[rndf(B, seed + 201, 0, 1) < 0.5] = 0
    done = DONE_VALUES[np.random.default_rng(seed + 202).integers(0, len(DONE_VALUES), B)]
    if B >= 5:      # no end; ends by the Pong override only; ends by done; both; a done that is not 1
        rew[:5] = [0, 1.5, 0, -0.25, 0]
        done[:5] = [0, 0, 1, -1, 0.5]
    X["rew"], X["done"] = rew, done
    X["heads"] = rndf((B, 4), seed + 203, -3, 3)             # the value is column 3 of a wider heads buffer (val_stride 4)
    X["val1"] = X["heads"][:, 3].copy()                      # or a column of its own (val_stride 1)
    X["mask_zeros"] = np.zeros(B, np.float32)
    X["mask_ones"] = np.ones(B, np.float32)
    X["mask_mixed"] = np.where(np.arange(B) % 2 == 1, np.float32(2.5), np.float32(0)).astype(np.float32)
    if HW:
        X["frame32"] = rndf((B, HW), seed + 204, 0, 1)
        f8 = np.random.default_rng(seed + 205).integers(0, 256, (B, HW + PAD), dtype=np.uint8)
        f8[:, :4] = 255                                    # 255 in every byte lane of a word
        f8[:, HW:] = 77
        if HW >= 8:
            f8[:, 4:8] = [0, 128, 127, 255]
        X["frame8"] = f8
    if hdim:
        X["h_new"] = rndf((B, hdim), seed + 206)
    return X


def _to_dev(D, car, S):
    G = {k: _dev(v) for k, v in D.items()}
    for k, v in car.items():
        if k == "state":                                   # the carried state rows are strided: S + PAD floats apart
            g = torch.full((v.shape[0], S + PAD), PADV, device=DEV)
            g[:, :S] = _dev(v.reshape(v.shape[0], S))
            G[k] = g
        else:
            G[k] = _dev(v)
    return G


def _launch(form, G, Xd, B, T, t, slot0, C, HW, pong, de=True, h_src="null", h_rows=True, reset="done", prev_null=False,
            out_off=0, vs=4, gamma=GAMMA):
    """the launches of env step t in the given form.  prev = the states row of step t, out = the row of step t + 1 or, at the
    end of the slot, the carried state (rows S + PAD floats apart)"""
    ops = _ops()
    S = C * HW
    last = t + 1 == T
    val_ptr = Xd["heads"].data_ptr() + 12 if vs == 4 else Xd["val1"].data_ptr()
    book = (Xd["rew"], Xd["done"], val_ptr, vs, G["val_prev"], G["rewards"], G["dones"], G["deltas"])
    if form in STATE_FORMS:
        rowp = lambda k: G["states"].data_ptr() + 4 * (slot0 * T + k) * S
        prev_ptr, prev_stride = (0 if prev_null else rowp(t)), T * S
        out_ptr, out_stride = (G["state"].data_ptr() + 4 * out_off, G["state"].stride(0)) if last else (rowp(t + 1), T * S)
        mask = None if reset == "null" else Xd["done" if reset == "done" else "mask_" + reset]
        f8p, f8s = Xd["frame8"].data_ptr(), Xd["frame8"].stride(0)
    de_t = G["done_eff"] if de else None
    if form in RECURRENT:
        hd = G["h"].shape[1]
        if h_src != "else":
            G["h"].copy_(Xd["h_new"])                      # the cell wrote its new hidden rows in place
        h_src_ptr = {"null": 0, "same": G["h"].data_ptr(), "else": Xd["h_new"].data_ptr()}[h_src]
        h_rows_ptr = G["h_states"].data_ptr() + 4 * (slot0 * T + t + 1) * hd if h_rows and not last else 0
    if form == "record":
        ops.rollout_record(*book, de_t, None, B, T, t, slot0, gamma, pong)
    elif form == "record_h":
        ops.rollout_record(*book, de_t, G["h"], B, T, t, slot0, gamma, pong)
    elif form == "push":
        ops.frame_stack_push(Xd["frame32"], mask, prev_ptr, prev_stride, out_ptr, out_stride, B, C, HW)
    elif form == "push_u8":
        ops.frame_stack_push_u8(f8p, f8s, mask, prev_ptr, prev_stride, out_ptr, out_stride, B, C, HW)
    elif form == "record+push":
        ops.rollout_record(*book, de_t, None, B, T, t, slot0, gamma, pong)
        ops.frame_stack_push(Xd["frame32"], mask, prev_ptr, prev_stride, out_ptr, out_stride, B, C, HW)
    elif form == "post":
        ops.rollout_post(*book, T, t, slot0, gamma, pong, Xd["frame32"], mask, prev_ptr, prev_stride, out_ptr, out_stride,
                         B, C, HW)
    elif form == "post_u8":
        ops.rollout_post_u8(*book, T, t, slot0, gamma, pong, f8p, f8s, mask, prev_ptr, prev_stride, out_ptr, out_stride,
                            B, C, HW)
    elif form in ("post_rec", "post_rec_u8"):
        u8 = form == "post_rec_u8"
        ops.rollout_post_rec(*book, T, t, slot0, gamma, pong, 0 if u8 else Xd["frame32"].data_ptr(), f8p if u8 else 0,
                             f8s if u8 else 0, mask, prev_ptr, prev_stride, out_ptr, out_stride, B, C, HW, de_t, G["h"],
                             h_rows_ptr, T * hd, h_src_ptr=h_src_ptr)
    elif form == "frames":
        ops.rollout_post_frames(*book, T, t, slot0, gamma, pong, B, de_t, None, 0, 0, 0, G["nvalid"], G["nv"].data_ptr())
    elif form == "frames_h":
        ops.rollout_post_frames(*book, T, t, slot0, gamma, pong, B, de_t, G["h"], h_rows_ptr, T * hd, h_src_ptr,
                                G["nvalid"], G["nv"].data_ptr())
    else:
        raise KeyError(form)


def _twin(form, D, car, X, T, t, slot0, HW, pong, de=True, h_rows=True, reset="done", gamma=GAMMA):
    """the twin's env step, keeping of it what the form is documented to produce"""
    keepD, keepC = {k: v.copy() for k, v in D.items()}, {k: v.copy() for k, v in car.items()}
    frame = None
    if "states" in D:
        frame = X["frame8"][:, :HW].astype(np.float32) if form in U8_FORMS else X["frame32"]
    mask = None if reset == "done" else X["mask_zeros" if reset == "null" else "mask_" + reset]
    twin_step(D, car, X["rew"], X["done"], X["heads"][:, 3], frame, T, t, slot0, gamma, pong,
              h_new=X["h_new"] if form in RECURRENT else None, reset=mask)
    made = set(PRODUCES[form])
    if not de:
        made.discard("done_eff")
    if not h_rows:
        made.discard("h_states")
    for k in D:
        if k not in made:
            D[k][...] = keepD[k]
    for k in car:
        if k not in made:
            car[k][...] = keepC[k]


def _same(tag, G, D, car, Xd, X, S, out_off=0):
    """every buffer the call was handed, in full: outputs, what must not have changed, padding, inputs"""
    for k, v in D.items():
        _eq(f"{tag} {k}", G[k], v)
    for k, v in car.items():
        if k == "state":
            want = np.full((v.shape[0], S + PAD), PADV, np.float32)
            flat = v.reshape(v.shape[0], S)
            if not (flat == CFILL["state"]).all():          # written: at the offset the call was given
                want[:, :S] = CFILL["state"]
                want[:, out_off:out_off + S] = flat
            else:
                want[:, :S] = flat
            _eq(f"{tag} carried state", G[k], want)
        else:
            _eq(f"{tag} carried {k}", G[k], v)
    for k, v in X.items():
        _eq(f"{tag} input {k}", Xd[k], v)


def _one_step(form, B, T, t, slot0, pong, C, HW, hdim, seed, **opts):
    has_states = form in STATE_FORMS
    D, car = _setup(B, T, t, slot0, C if has_states else 0, HW if has_states else 0, hdim, seed)
    X = _inputs(B, HW if has_states else 0, hdim, seed)
    G, Xd = _to_dev(D, car, C * HW), {k: _dev(v) for k, v in X.items()}
    _launch(form, G, Xd, B, T, t, slot0, C, HW, pong, **opts)
    _twin(form, D, car, X, T, t, slot0, HW, pong, **{k: v for k, v in opts.items() if k in ("de", "h_rows", "reset")})
    tag = f"{form} B={B} T={T} t={t} slot0={slot0} pong={pong} C={C} HW={HW} hdim={hdim} {opts}"
    _same(tag, G, D, car, Xd, X, C * HW, out_off=opts.get("out_off", 0))
    return D, car


# ======================================================================================================= 1. bookkeeping
TT = [(1, 0), (5, 0), (5, 2), (5, 4)]


@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("form", ["record", "record_h", "post", "post_u8", "post_rec", "post_rec_u8", "frames", "frames_h"])
def test_bookkeeping_of_one_env_step_equals_the_twin(form, B):
    """rewards / dones rows, the TD residual of the step before (none at t == 0: deltas[(slot0 + b) * T - 1] is the previous
    slot's), val_prev, done_eff (given and NULL), the valid-plane counts (none past the slot at t == T - 1) -- in blocks
    of 256 envs, whichever grid the entry point launches.  a2c_rollout_post_frames runs both of its grids (frames /
    frames_h)."""
    n = 0
    for T, t in TT:
        for slot0 in (0, 2):
            for pong in (0, 1):
                de = True if form == "record_h" else n % 2 == 0
                _one_step(form, B, T, t, slot0, pong, 4, 16, 8 if form in RECURRENT else 0, 1000 * n + B, de=de,
                          vs=4 if slot0 == 0 else 1)
                n += 1


# ======================================================================================================= 2. frame stack
@pytest.mark.parametrize("HW", [4, 16, 7056, 8204])
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("form", ["push", "push_u8", "post", "post_u8", "post_rec", "post_rec_u8"])
def test_frame_stack_planes_equal_the_twin(form, C, HW):
    """out = reset ? [0, .., 0, frame] : [prev[1:], frame], prev and out rows inside one rollout-major buffer (stride
    T * C * HW) or, at the end of the slot, in the strided carry; uint8 pixels over 0..255 from rows frame_stride > HW
    apart; HW = 8204 runs the strided iteration of the x-capped grid and its ragged tail"""
    B, T, slot0 = 3, 3, 1
    for i, reset in enumerate(["null", "zeros", "mixed", "ones", "done"]):
        _one_step(form, B, T, 1 if i % 2 == 0 else 2, slot0, i % 2, C, HW, 8 if form in RECURRENT else 0, 50 * i + C + HW,
                  reset=reset)
    if C == 1:
        _one_step(form, B, T, 2, slot0, 1, C, HW, 8 if form in RECURRENT else 0, 7, reset="mixed", prev_null=True)


@pytest.mark.parametrize("C,HW,out_off", [(3, 7, 0), (1, 7, 0), (2, 8, 1), (4, 8, 1), (2, 1, 0), (2, 1030, 1), (2, 2051, 0)])
def test_frame_stack_push_scalar_path(C, HW, out_off):
    """a2c_frame_stack_push alone has a path for HW % 4 != 0 and for rows that are not 16-byte aligned (out offset by 4
    bytes); 1030 floats are past one 256-lane block, 2051 past the 8 x 256 x-cap"""
    for i, reset in enumerate(["null", "mixed", "ones"]):
        _one_step("push", 3, 2, 1, 1, 0, C, HW, 0, 300 + i, reset=reset, out_off=out_off)
        if out_off == 0:
            _one_step("push", 3, 3, 1, 0, 0, C, HW, 0, 310 + i, reset=reset)


def _refused(fn, *a, **kw):
    from a2c_amd import _lib
    with pytest.raises(_lib.A2CKernelError) as ei:
        fn(*a, **kw)
    assert f"(code {ERR_ARG})" in str(ei.value), str(ei.value)


def test_frame_stack_refusals_leave_every_buffer_alone():
    """A2C_ERR_ARG, and every buffer still at its sentinel afterwards: misaligned pointers, HW % 4 != 0, frame_stride <
    HW, frame_stride % 4, a2c_rollout_post_rec with both or neither frame pointer or without h"""
    ops = _ops()
    B, T, t, slot0, C, HW, hd = 3, 3, 1, 1, 2, 8, 8
    S = C * HW
    D, car = _setup(B, T, t, slot0, C, HW, hd, 1)
    X = _inputs(B, HW, hd, 1)
    G, Xd = _to_dev(D, car, S), {k: _dev(v) for k, v in X.items()}
    val_ptr = Xd["heads"].data_ptr() + 12
    book = (Xd["rew"], Xd["done"], val_ptr, 4, G["val_prev"], G["rewards"], G["dones"], G["deltas"])
    prev, out, rs = G["states"].data_ptr() + 4 * (slot0 * T + t) * S, G["states"].data_ptr() + 4 * (slot0 * T + t + 1) * S, T * S
    f8, f8s, f32 = Xd["frame8"].data_ptr(), Xd["frame8"].stride(0), Xd["frame32"]
    tail = (B, C, HW)
    head = (T, t, slot0, GAMMA, 1)
    # misaligned pointers
    _refused(ops.rollout_post, *book, *head, f32, None, prev + 4, rs, out, rs, *tail)
    _refused(ops.rollout_post, *book, *head, f32, None, prev, rs, out + 4, rs, *tail)
    _refused(ops.rollout_post, *book, *head, f32, None, prev, rs + 1, out, rs, *tail)
    _refused(ops.rollout_post_u8, *book, *head, f8 + 1, f8s, None, prev, rs, out, rs, *tail)
    _refused(ops.rollout_post_u8, *book, *head, f8, f8s, None, prev, rs, out + 8, rs, *tail)
    _refused(ops.frame_stack_push_u8, f8 + 2, f8s, None, prev, rs, out, rs, *tail)
    _refused(ops.frame_stack_push_u8, f8, f8s, None, prev + 4, rs, out, rs, *tail)
    _refused(ops.frame_stack_push_u8, f8, f8s, None, prev, rs, out + 4, rs, *tail)
    rec_tail = (G["done_eff"], G["h"], 0, 0)
    _refused(ops.rollout_post_rec, *book, *head, f32.data_ptr() + 4, 0, 0, None, prev, rs, out, rs, *tail, *rec_tail)
    _refused(ops.rollout_post_rec, *book, *head, 0, f8 + 1, f8s, None, prev, rs, out, rs, *tail, *rec_tail)
    # HW % 4 != 0 (HW = 7: every stride still a multiple of 4 floats)
    _refused(ops.rollout_post, *book, *head, f32, None, prev, rs, out, rs, B, C, 7)
    _refused(ops.rollout_post_u8, *book, *head, f8, f8s, None, prev, rs, out, rs, B, C, 7)
    _refused(ops.rollout_post_rec, *book, *head, 0, f8, f8s, None, prev, rs, out, rs, B, C, 7, *rec_tail)
    _refused(ops.frame_stack_push_u8, f8, f8s, None, prev, rs, out, rs, B, C, 7)
    # frame_stride < HW, frame_stride % 4
    for bad in (HW - 4, HW + 2):
        _refused(ops.rollout_post_u8, *book, *head, f8, bad, None, prev, rs, out, rs, *tail)
        _refused(ops.frame_stack_push_u8, f8, bad, None, prev, rs, out, rs, *tail)
        _refused(ops.rollout_post_rec, *book, *head, 0, f8, bad, None, prev, rs, out, rs, *tail, *rec_tail)
    # a2c_rollout_post_rec: both frame pointers, neither, no h
    _refused(ops.rollout_post_rec, *book, *head, f32.data_ptr(), f8, f8s, None, prev, rs, out, rs, *tail, *rec_tail)
    _refused(ops.rollout_post_rec, *book, *head, 0, 0, 0, None, prev, rs, out, rs, *tail, *rec_tail)
    rc = _raw().a2c_rollout_post_rec(Xd["rew"].data_ptr(), Xd["done"].data_ptr(), val_ptr, 4, G["val_prev"].data_ptr(),
                                     G["rewards"].data_ptr(), G["dones"].data_ptr(), G["deltas"].data_ptr(), T, t, slot0, GAMMA,
                                     1, f32.data_ptr(), 0, 0, 0, prev, rs, out, rs, B, C, HW, G["done_eff"].data_ptr(), 0, hd, 0,
                                     0, 0, _st())
    assert rc == ERR_ARG
    torch.cuda.synchronize()
    _same("refusals", G, D, car, Xd, X, S)


# ======================================================================================================= 3. hidden rows
@pytest.mark.parametrize("hdim", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("form", ["post_rec", "frames_h"])
def test_hidden_rows_equal_the_twin(form, hdim):
    """h = 0 where the step ended an episode (by done, or by the Pong override alone), else what the cell left (h_src NULL =
    h, h_src == h, h_src elsewhere and then untouched); the h_states row of the step that follows (NULL, or rows T * hdim
    apart); 256 lanes striding hdim"""
    n = 0
    for h_src in ("null", "same", "else"):
        for h_rows in (True, False):
            for pong in (1, 0):
                _one_step(form, 5, 3, 1, 1, pong, 1, 4, hdim, 40 * n + hdim, h_src=h_src, h_rows=h_rows, de=n % 3 != 0)
                n += 1
    _one_step(form, 5, 3, 2, 0, 1, 1, 4, hdim, hdim, h_src="else")         # end of the slot: no h_states row to write


# ========================================================================================================= 4. bootstrap
@pytest.mark.parametrize("B", [1, 256, 257])
@pytest.mark.parametrize("T", [1, 5])
def test_bootstrap_equals_the_twin(B, T):
    ops = _ops()
    for slot0 in (0, 2):
        D, car = _setup(B, T, T - 1, slot0, 0, 0, 0, 7 * B + T + slot0)
        e = (slot0 + np.arange(B)) * T + T - 1
        D["rewards"][e] = rndf(B, B + 1, -2, 2)
        D["dones"][e] = np.arange(B) % 3 == 1 if B > 1 else slot0 == 0       # last-step dones mixed
        D["deltas"][e[:B // 2]] = rndf(B // 2, B + 2)                       # overwritten either way
        heads = rndf((B, 4), B + 3, -3, 3)                                  # val_boot: a column of a wider buffer, or
        vs, col = (4, 2) if slot0 == 0 else (1, 0)                          # B values in a row
        G, hd = _to_dev(D, car, 0), _dev(heads)
        ops.rollout_bootstrap(hd.data_ptr() + 4 * col, vs, G["val_prev"], G["rewards"], G["dones"], G["deltas"], B, T, slot0,
                              GAMMA)
        twin_bootstrap(D, car, heads[:, 2] if vs == 4 else heads.ravel()[:B], T, slot0, GAMMA)
        _same(f"bootstrap B={B} T={T} slot0={slot0}", G, D, car, {"heads": hd}, {"heads": heads}, 0)


# ======================================================================================================= 5. whole slots
def _play(form, script, B, T, slot0, C, HW, hdim, n_roll=2):
    """two consecutive rollouts of T steps through the kernels alone -> the twin's buffers, all compared on the way"""
    ops = _ops()
    S = C * HW
    n_slots = slot0 + B + 2
    rec, frames_form = form in RECURRENT, form == "frames"
    D = new_rollout(n_slots, T, C, HW, hdim if rec else 0, FILL)
    car = new_carry(B, C, HW, hdim if rec else 0, CFILL)
    car["state"][:] = 0
    car["state"][:, C - 1] = script["frame0"]
    car["nv"][:] = 1
    if rec:
        car["h"][:] = 0
    G = _to_dev(D, car, S)
    Fst = (T + C) * HW + PAD
    F = np.full((n_slots, Fst), 201, np.uint8)                             # the single-frame store, rows padded
    Fv = lambda: F[slot0:slot0 + B, :(T + C) * HW].reshape(B, T + C, HW)
    if frames_form:
        Fv()[:, T + C - 1] = script["frame0"]
        Fd = _dev(F)
        Dst = _dev(np.full((n_slots * T, C, HW), FILL["states"], np.float32))
    rowp = lambda k: G["states"].data_ptr() + 4 * (slot0 * T + k) * S
    for r in range(n_roll):
        if frames_form:
            ops.frame_store_begin(Fd.data_ptr() + slot0 * Fst, Fst, T, C, HW, G["nvalid"].data_ptr() + 4 * slot0 * T,
                                  G["nv"].data_ptr(), B)
            v = Fv()
            twin_store_begin(v, T, C)
            F[slot0:slot0 + B, :(T + C) * HW] = v.reshape(B, -1)
        else:
            ops.copy_rows(G["state"].data_ptr(), G["state"].stride(0), rowp(0), T * S, B, S)
            if rec:
                ops.copy_rows(G["h"].data_ptr(), hdim, G["h_states"].data_ptr() + 4 * slot0 * T * hdim, T * hdim, B, hdim)
        keep_nv = D["nvalid"].copy()
        twin_begin(D, car, T, slot0)
        if not frames_form:
            D["nvalid"][:] = keep_nv
        for t in range(T):
            X = script["steps"][r * T + t]
            Xd = {k: _dev(v) for k, v in X.items()}
            if frames_form:                                                # what the ingest does: the new frame into its slot
                Fd[slot0:slot0 + B, (t + C) * HW:(t + C + 1) * HW] = Xd["frame8"][:, :HW]
                F[slot0:slot0 + B, (t + C) * HW:(t + C + 1) * HW] = X["frame8"][:, :HW]
            _launch(form, G, Xd, B, T, t, slot0, C, HW, 1)
            _twin(form, D, car, X, T, t, slot0, HW, 1)
            if frames_form:                                                # the twin keeps the states the store stands for
                D2 = {"states": D["states"], "rewards": D["rewards"].copy(), "dones": D["dones"].copy(),
                      "deltas": D["deltas"].copy(), "nvalid": D["nvalid"].copy()}
                c2 = {k: v.copy() for k, v in car.items()}
                c2["state"] = car["state"]
                twin_step(D2, c2, X["rew"], X["done"], X["heads"][:, 3], X["frame8"][:, :HW].astype(np.float32), T, t, slot0,
                          GAMMA, 1)
        boot = script["boot"][r]
        bd = _dev(boot)
        ops.rollout_bootstrap(bd.data_ptr() + 4, 2, G["val_prev"], G["rewards"], G["dones"], G["deltas"], B, T, slot0, GAMMA)
        twin_bootstrap(D, car, boot[:, 1], T, slot0, GAMMA)
        tag = f"{form} rollout {r}"
        if frames_form:
            ops.frames_to_states(Fd.data_ptr() + slot0 * Fst, Fst, G["nvalid"].data_ptr() + 4 * slot0 * T, T,
                                 Dst.data_ptr() + 4 * slot0 * T * S, T * S, B, T, C, HW)
            _eq(f"{tag} frame store", Fd, F)
            want = D["states"].copy()
            G2 = dict(G, states=Dst)
            _same(tag, G2, dict(D, states=want), {k: v for k, v in car.items() if k != "state"}, {}, {}, S)
        else:
            _same(tag, G, D, car, {}, {}, S)
    return D


def _whole_slot_script(B, T, HW, hdim, n_roll=2):
    steps = []
    for k in range(n_roll * T):
        X = _inputs(B, HW, hdim, 5000 + 31 * k)
        X["frame32"] = X["frame8"][:, :HW].astype(np.float32)              # every form sees the same pixels
        steps.append(X)
    return dict(frame0=np.random.default_rng(9).integers(0, 256, (B, HW), dtype=np.uint8), steps=steps,
                boot=[rndf((B, 2), 6000 + r, -3, 3) for r in range(n_roll)])


def test_whole_slots_in_every_form_equal_the_twin():
    """two consecutive rollouts of T = 5 steps for B = 257 envs, C = 4, HW = 16, played by the kernels alone: record + push,
    post, post_u8, post_rec (hdim 8) and frame_store_begin + post_frames + frames_to_states, bootstrap at the end of each
    rollout.  A wrong val_prev carry, valid-plane count across a slot boundary or window origin shows here and in no
    single-step case.  The frame-store form's expanded states are compared with the same twin states as the others'."""
    B, T, slot0, C, HW, hdim = 257, 5, 2, 4, 16, 8
    script = _whole_slot_script(B, T, HW, hdim)
    ref = None
    for form in ("record+push", "post", "post_u8", "post_rec", "frames"):
        D = _play(form, script, B, T, slot0, C, HW, hdim)
        if ref is None:
            ref = D
        for k in ("states", "rewards", "dones", "deltas"):
            _eq(f"{form} twin {k}", D[k], ref[k])      # one twin result for every form (each already compared with the device)


# ======================================================================================================= 6. frame store
def _store(R, T, C, HW, seed, pad=0):
    rng = np.random.default_rng(seed)
    F = rng.integers(0, 256, (R, (T + C) * HW + pad), dtype=np.uint8)
    F[:, :4] = 255
    if pad:
        F[:, (T + C) * HW:] = 201
    return F


@pytest.mark.parametrize("C", [1, 2, 4])
def test_frames_to_states_equals_the_twin(C):
    ops = _ops()
    R, T, HW = 5, 6, 1028                                                   # 257 float4: a ragged second block
    F = _store(R, T, C, HW, C)
    Fv = F.reshape(R, T + C, HW)
    nv = (1 + (np.arange(R * T) * 7 + 3) % C).astype(np.int32).reshape(R, T)     # every value in 1..C
    assert set(nv.ravel()) == set(range(1, C + 1))
    Fd, nvd = _dev(F), _dev(nv)
    for nvalid in (None, nv):
        out = torch.full((R + 2, T + 1, C, HW), SENT, device=DEV)          # slot rows (T + 1) * C * HW apart, slots around
        ops.frames_to_states(Fd.data_ptr(), Fd.stride(0), 0 if nvalid is None else nvd.data_ptr(), T,
                             out.data_ptr() + 4 * out.stride(0), out.stride(0), R, T, C, HW)
        want = np.full((R + 2, T + 1, C, HW), SENT, np.float32)
        want[1:R + 1, :T] = twin_frames_to_states(Fv, nvalid, T, C)
        _eq(f"frames_to_states C={C} nvalid={'NULL' if nvalid is None else 'given'}", out, want)
        # one time step of every slot, by pointer offsets: state k = 3
        row = torch.full((R, C * HW + PAD), SENT, device=DEV)
        ops.frames_to_states(Fd.data_ptr() + 3 * HW, Fd.stride(0), 0 if nvalid is None else nvd.data_ptr() + 4 * 3, T,
                             row.data_ptr(), row.stride(0), R, 1, C, HW)
        want = np.full((R, C * HW + PAD), SENT, np.float32)
        want[:, :C * HW] = twin_frames_to_states(Fv[:, 3:], None if nvalid is None else nv[:, 3:4], 1, C).reshape(R, -1)
        _eq(f"frames_to_states one step C={C}", row, want)
    _eq("store", Fd, F)
    _eq("nvalid", nvd, nv)


def test_frames_to_states_in_two_launches():
    """R * nt = 600 * 128 rows: 65535 / 128 = 511 slots in the first launch, 89 in the second, which starts at pointer
    offsets of 511 slots into the store, the counts and the states"""
    ops = _ops()
    R, T, C, HW = 600, 128, 4, 4
    F = _store(R, T, C, HW, 11)
    nv = np.random.default_rng(12).integers(1, C + 1, (R, T)).astype(np.int32)
    Fd, nvd = _dev(F), _dev(nv)
    out = torch.full((R + 1, T, C, HW), SENT, device=DEV)
    ops.frames_to_states(Fd.data_ptr(), Fd.stride(0), nvd.data_ptr(), T, out.data_ptr(), out.stride(0), R, T, C, HW)
    want = np.full((R + 1, T, C, HW), SENT, np.float32)
    want[:R] = twin_frames_to_states(F.reshape(R, T + C, HW), nv, T, C)
    _eq("frames_to_states 600 x 128", out, want)
    # past 65535 * 8 rows: refused, nothing written
    out2 = torch.full((16,), SENT, device=DEV)
    _refused(ops.frames_to_states, Fd.data_ptr(), 0, 0, 0, out2.data_ptr(), 0, 65535 * 8 // 128 + 1, 128, C, HW)
    _refused(ops.frames_to_states, Fd.data_ptr(), 0, 0, 0, out2.data_ptr(), 0, 1, 65536, C, HW)
    assert bool((out2 == SENT).all())


@pytest.mark.parametrize("T,C,HW", [(4, 4, 16), (6, 4, 16), (2, 2, 516), (5, 1, 1028), (7, 4, 260), (4, 4, 4), (1, 1, 4)])
def test_frame_store_begin_equals_the_twin(T, C, HW):
    """frames[r][0 .. C-1] = frames[r][T .. T+C-1], nvalid_rows[r * T] = nvalid_carry[r]; T == C and T > C; C * HW / 4 =
    16, 64 (below one block), 258, 257, 260 (a ragged last block); slot rows padded, the padding left alone"""
    ops = _ops()
    R = 5
    F = _store(R + 2, T, C, HW, T + C + HW, pad=PAD)
    rows = np.full(((R + 2) * T,), -77, np.int32)
    carry = (1 + np.arange(R) % NV_CAP).astype(np.int32)
    Fd, rd, cd = _dev(F), _dev(rows), _dev(carry)
    ops.frame_store_begin(Fd.data_ptr() + Fd.stride(0), Fd.stride(0), T, C, HW, rd.data_ptr() + 4 * T, cd.data_ptr(), R)
    v = F[1:R + 1, :(T + C) * HW].reshape(R, T + C, HW).copy()
    twin_store_begin(v, T, C)
    F[1:R + 1, :(T + C) * HW] = v.reshape(R, -1)
    rows[(1 + np.arange(R)) * T] = carry
    _eq("store", Fd, F)
    _eq("nvalid_rows", rd, rows)
    _eq("nvalid_carry", cd, carry)


def test_frame_store_begin_refuses_a_slot_shorter_than_the_window():
    ops = _ops()
    F = _store(3, 4, 4, 16, 1)
    Fd, rd, cd = _dev(F), _dev(np.full((12,), -77, np.int32)), _dev(np.ones(3, np.int32))
    _refused(ops.frame_store_begin, Fd.data_ptr(), Fd.stride(0), 3, 4, 16, rd.data_ptr(), cd.data_ptr(), 3)       # T < C
    _refused(ops.frame_store_begin, Fd.data_ptr(), (4 + 4) * 16 - 4, 4, 4, 16, rd.data_ptr(), cd.data_ptr(), 3)   # stride
    _eq("store", Fd, F)
    assert bool((rd == -77).all())


# ======================================================================================================== 7. row movers
@pytest.mark.parametrize("B,n", [(1, 1), (5, 257), (3, 16389), (32769, 3)])
def test_copy_rows(B, n):
    """16389 columns are past the 64 x 256 x-cap, 32769 rows past the y-cap; both strides larger than n, padding checked"""
    ops = _ops()
    src = rndf((B + 1, n + 3), B + n)
    dst = np.full((B + 1, n + 5), SENT, np.float32)
    sd, dd = _dev(src), _dev(dst)
    ops.copy_rows(sd.data_ptr() + 4, n + 3, dd.data_ptr() + 8, n + 5, B, n)
    dst[:B, 2:2 + n] = src[:B, 1:1 + n]
    _eq("dst", dd, dst)
    _eq("src", sd, src)


@pytest.mark.parametrize("B,n", [(1, 1), (5, 7), (3, 100), (257, 3), (2, 255)])
def test_mask_rows(B, n):
    """x[b, :n] *= 1 - dones[b * done_stride]: ld > n, done_stride > 1, B * n across a block boundary"""
    x = rndf((B, n + 3), B + n)
    d = (rndf((B, 3), B + n + 1, 0, 1) < 0.5).astype(np.float32)
    xd, dd = _dev(x), _dev(d)
    rc = _raw().a2c_mask_rows(xd.data_ptr(), n + 3, dd.data_ptr() + 4, 3, B, n, _st())
    assert rc == 0
    x[:, :n] = x[:, :n] * (np.float32(1) - d[:, 1:2])
    _eq("x", xd, x)
    _eq("dones", dd, d)


@pytest.mark.parametrize("R,T,n", [(0, 3, 4), (5, 0, 4), (5, 7, 0), (5, 7, 12), (257, 3, 5), (7, 74899, 1), (1, 524295, 1)])
def test_permute_rows(R, T, n):
    """dst[t, r] = src[r, t]; 7 * 74899 = 1 * 524295 = 2048 * 256 + 5 / + 7 elements: past the 2048-block cap, so the
    grid-stride loop runs a second, ragged iteration"""
    ops = _ops()
    src = rndf((R, T, n), R + T + n)
    sd = _dev(src)
    dd = torch.full((T * R * n + 4,), SENT, device=DEV)
    ops.permute_rows(sd, dd, R, T, n)
    want = np.full((T * R * n + 4,), SENT, np.float32)
    want[:T * R * n] = np.ascontiguousarray(src.transpose(1, 0, 2)).ravel()
    _eq("dst", dd, want)
    _eq("src", sd, src)


# ================================================================================================= 8. a2c_frame_prep_u8
def _prep(raw, y0, y1, x0, x1, step, binarise):
    v = raw[:, y0:y1:step, x0:x1:step, 0]
    if binarise:
        v = np.where((v == 144) | (v == 109) | (v == 0), 0, 1).astype(np.uint8)
    return v.reshape(raw.shape[0], -1)


def _prep_call(rawd, raw_stride, H, W, C, crop, step, binarise, outd, out_stride, n):
    y0, y1, x0, x1 = crop
    return _raw().a2c_frame_prep_u8(rawd.data_ptr(), raw_stride, H, W, C, y0, y1, x0, x1, step, binarise, outd.data_ptr(),
                                    out_stride, n, _st())


PREP_CASES = [  # H, W, C, (y0, y1, x0, x1), step      -- OW % 4 == 0 in every one; OH, OW are ceilings
    (210, 160, 3, (35, 195, 0, 160, 2)), (210, 160, 3, (35, 195, 8, 152, 2)), (210, 160, 3, (34, 195, 1, 160, 2)),
    (210, 160, 3, (0, 210, 3, 159, 3)), (210, 160, 3, (7, 8, 5, 9, 1)),
    (64, 48, 1, (0, 64, 0, 48, 1)), (64, 48, 1, (1, 64, 1, 48, 2)), (64, 48, 1, (3, 62, 5, 40, 3)),
    (33, 40, 4, (0, 33, 0, 40, 1)), (33, 40, 4, (2, 33, 3, 38, 3)), (33, 40, 4, (1, 32, 7, 39, 2)),
]


@pytest.mark.parametrize("binarise", [0, 1])
@pytest.mark.parametrize("H,W,C,spec", PREP_CASES)
def test_frame_prep_u8_equals_numpy_slicing(H, W, C, spec, binarise):
    """out[oy][ox] = raw[y0 + oy * step][x0 + ox * step][0] over explicit crops (odd x0, crops that are no multiple of the
    step), raw rows and out rows padded; binarise: 144, 109 and 0 -> 0, everything else -> 1"""
    y0, y1, x0, x1, step = spec
    n = 3
    rng = np.random.default_rng(H + W + y0 + x0 + step)
    raw = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
    pick = rng.integers(0, 8, (n, H, W))
    for i, v in enumerate((0, 109, 144, 255)):                             # about half of channel 0: the four special values
        raw[..., 0][pick == i] = v
    OH, OW = -(-(y1 - y0) // step), -(-(x1 - x0) // step)
    assert OW % 4 == 0
    rawp = np.full((n, H * W * C + 5), 99, np.uint8)
    rawp[:, :H * W * C] = raw.reshape(n, -1)
    out = np.full((n + 1, OH * OW + PAD), 201, np.uint8)
    rd, od = _dev(rawp), _dev(out)
    assert _prep_call(rd, rawp.shape[1], H, W, C, (y0, y1, x0, x1), step, binarise, od, out.shape[1], n) == 0
    want = _prep(raw, y0, y1, x0, x1, step, binarise)
    assert want.shape == (n, OH * OW)
    out[:n, :OH * OW] = want
    _eq("out", od, out)
    _eq("raw", rd, rawp)


def test_frame_prep_u8_refusals():
    H, W, C, n = 33, 40, 4, 2
    rd = _dev(np.zeros((n, H * W * C), np.uint8))
    od = _dev(np.full((n, 40 * 40), 201, np.uint8))
    ok = ((0, 33, 0, 40), 1)
    call = lambda crop, step, ostride=40 * 40, rstride=H * W * C: _prep_call(rd, rstride, H, W, C, crop, step, 1, od, ostride, n)
    assert call(*ok) == 0
    od.fill_(201)
    assert call((0, 33, 0, 39), 1) == ERR_ARG          # OW = 39
    assert call((0, 33, 1, 40), 2) == 0                # OW = 20 is fine, ...
    od.fill_(201)
    assert call((0, 33, 0, 37), 2) == ERR_ARG          # ... OW = 19 is not
    assert call((0, 34, 0, 40), 1) == ERR_ARG          # a crop outside the frame
    assert call((0, 33, 0, 44), 1) == ERR_ARG
    assert call((-1, 33, 0, 40), 1) == ERR_ARG
    assert call((5, 5, 0, 40), 1) == ERR_ARG
    assert call((0, 33, 0, 40), 1, ostride=33 * 40 - 4) == ERR_ARG          # out_stride < OH * OW
    assert call((0, 33, 0, 40), 1, rstride=H * W * C - 1) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((od == 201).all())
