"""The shape-specialised 3x3 kernels of csrc/conv3.hip (c3_kernel, c3s_kernel, c3b_kernel, c3bs_kernel, c3w_kernel) over
whole batches, called through the C ABI (a2c_amd.ops) and compared with float64 F.conv2d / F.conv_transpose2d / a float64
weight gradient on the CPU.

All of these kernels are persistent: a launch has total = B * NBAND bands and grid = min(total, CUs * per_cu) workgroups,
and a workgroup walks its bands through a ring of D staged chunk images.  TABLE below has one row per kernel instance of
the dispatch (c3_fwd, c3_bwd_data, C3W_CASES, C3W_OLD_CASES) with its NBAND, its ring depth D and the static upper bound
per_cu_max of its launcher; a CPU test reads conv3.hip and fails when an instance is missing from it.  Every row runs at
three batch sizes worked out from that geometry and the device's CU count (`_sizes`):
  B = 1                                                    fewer bands than workgroups,
  the smallest B with B * NBAND > CUs * per_cu_max         some workgroups take a second band, ragged last round,
  the smallest B with B * NBAND >= (D + 2) * CUs * per_cu_max, plus one
                                                           every ring slot reused at least once, ragged last round,
clamped to the batch window in which the dispatch picks that instance: the forward switches kernels between B = 64 and
B = 65, so a `B <= 64` row runs at (1, .., 64) and a `B > 64` row at (65, ..): exactly the two sides of the switch.  (A
row whose second-round size lies beyond its window -- the short-band forward instances that only serve B <= 64 -- cannot
turn its ring through the library's entry points at all; it runs at 1 and 64.)

Inputs: x in [0, 1), w / sqrt(Cin * 9), dout in [-1, 1), a mask with half its entries <= 0.  The LAST sample of a batch
(B >= 2), whose bands are the ragged last round, is all zeros (forward, weight gradient) or has a mask that is <= 0
everywhere, exact zeros among them (backward-data); backward-data's all-zero dout sample is the one before it (B >= 3).
At the second-round size only the last sample reaches a second round (that is what makes the size the smallest one), so
there the one-before-last sample is still a first-round sample; at the ring-wrap size both lie in late rounds.

Criterion: `_crit` of test_gpu_small_kernels, e_k = max|kernel - fp64| <= 2 e_t + ulp(scale).  e_t is the error of a
plain fp32 evaluation of the same sums in index order on the CPU against the same fp64 reference -- forward and
backward-data: the first samples of the pool (`_npool`: the same number of elements for every layer), one rounded product
and one rounded addition per (c, ky, kx) in index order; weight gradient: per sample a running sum over the output
positions in raster order, then a running sum over the samples, on the batch of the middle size of the layer's default
instance (B = 1 takes the first sample's own running sum, which is stricter; beyond the middle size: `_crit_wgrad`).
scale = the largest single term: max|x| max|w| (or max|bias|), max|dout| max|w|, max|dout| max|x|, max|dout|.  Sign words, the sentinels around every output and the documented bit-identities are exact.

Worst e_k / e_t per array measured on an MI355X over all cases of this file (`pytest -s` prints them at the end):
forward out 1.40; backward-data din 1.62 (float mask), 1.62 (sign words), 1.80 (no mask), 1.43 (float mask on the odd
images, generic kernel); weight gradient dW 1.63, db 1.63, old instances 1.20 and 1.52 -- beyond the middle batch these are
against e_t scaled by B / mid; against the middle batch's e_t itself the ring-wrap sizes measure dW 4.40 (old 3.00) and
db 3.78 (old 4.32), see `_crit_wgrad` --; from frames dW 1.62, db 0.95; fall-backs: weight gradient 1.11 in all four
cases, backward-data 1.34 (dout, din or mask off by 4 bytes), 0.97 / 1.10 (A2C_NO_ODD_BS=1 with / without mask); the
workspace edge's gradient 0.68.  Wall time of the file: 28 s of test calls on its own (242 GPU cases, the slowest 1.8 s).
"""
import math
import os
import re
import time
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_small_kernels as SK
from test_gpu_small_kernels import _crit, _running_sum, _u

DEV = "cuda"
ERR_ARG, ERR_WORKSPACE = -1, -3
SENT = SK.SENT
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-a2c_amd", "csrc", "conv3.hip")

# layer specs (Cin, H, W, Cout, ks, stride, pad): ConvModel conv1..4, GRUModel conv2..5 (conv1 is shared)
L1 = (4, 84, 84, 16, 3, 1, 1)
C2 = (16, 84, 84, 24, 3, 1, 1)
C3 = (24, 84, 84, 32, 3, 2, 1)
C4 = (32, 42, 42, 64, 3, 2, 1)
G2 = (16, 84, 84, 24, 3, 2, 1)
G3 = (24, 42, 42, 32, 3, 2, 1)
G4 = (32, 21, 21, 48, 3, 2, 1)
G5 = (48, 11, 11, 64, 3, 2, 1)
LAYERS = [L1, C2, C3, C4, G2, G3, G4, G5]
NAMES = dict(zip(LAYERS, ["conv1", "C.conv2", "C.conv3", "C.conv4", "G.conv2", "G.conv3", "G.conv4", "G.conv5"]))

# kind: fwd / bwd / wgrad / wgrad_old.  launcher<targs> as written in conv3.hip.  mode: how the entry points reach it.
# per_cu: static upper bound of workgroups per CU of the launcher -- c3_launch / c3b_launch: floor(160 KB / LDS bytes of
# the instance) (they ask the occupancy calculator, which cannot answer more than LDS allows; the LDS bytes from C3Geo /
# C3BGeo are in the comment of each row), c3s_launch / c3bs_launch: 1 (grid = min(total, CUs)), c3w_launch: 3 (`n > 3 ? 3
# : n`).  bmin / bmax: the batch window of the row in the dispatch.
Row = namedtuple("Row", "kind spec launcher targs mode nband D per_cu bmin bmax")
BIG = 1 << 30


def _r(kind, spec, launcher, targs, mode, nband, D, per_cu, bmin=1, bmax=BIG):
    return Row(kind, spec, launcher, targs.replace(" ", ""), mode, nband, D, per_cu, bmin, bmax)


TABLE = [
    # ---- c3_fwd, `signs != nullptr && B > 64`: direct-store kernels with the sign-word writer wave (c3_kernel<.., SG>, D = 2)
    _r("fwd", C2, "c3_launch", "16, 24, 84, 84, 1, 12, false, 0, true", "signs", 7, 2, 1, bmin=65),   # LDS 101,760 B
    _r("fwd", C3, "c3_launch", "24, 32, 84, 84, 2, 6, false, 0, true", "signs", 7, 2, 1, bmin=65),    # 93,696
    _r("fwd", G2, "c3_launch", "16, 24, 84, 84, 2, 6, false, 0, true", "signs", 7, 2, 1, bmin=65),    # 93,312
    _r("fwd", C4, "c3_launch", "32, 64, 42, 42, 2, 11, false, 0, true", "signs", 2, 2, 1, bmin=65),   # 103,168
    _r("fwd", G3, "c3_launch", "24, 32, 42, 42, 2, 11, false, 0, true", "signs", 2, 2, 1, bmin=65),   # 83,328
    # ---- c3_fwd, `signs != nullptr`: the staged kernels (c3s_kernel: two chunk buffers, D = 2); B <= 64 where the block above took B > 64
    _r("fwd", L1, "c3s_launch", "4, 16, 84, 84, 1, 12, false", "signs", 7, 2, 1),
    _r("fwd", C2, "c3s_launch", "16, 24, 84, 84, 1, 6, false", "signs", 14, 2, 1, bmax=64),
    _r("fwd", C3, "c3s_launch", "24, 32, 84, 84, 2, 6, false", "signs", 7, 2, 1, bmax=64),
    _r("fwd", G2, "c3s_launch", "16, 24, 84, 84, 2, 6, false", "signs", 7, 2, 1, bmax=64),
    _r("fwd", C4, "c3s_launch", "32, 64, 42, 42, 2, 11, false", "signs", 2, 2, 1, bmax=64),
    _r("fwd", G3, "c3s_launch", "24, 32, 42, 42, 2, 11, false", "signs", 2, 2, 1, bmax=64),
    _r("fwd", G4, "c3s_launch", "32, 48, 21, 21, 2, 11, false", "signs", 1, 2, 1),
    # ---- c3_fwd, no sign words, `small = B <= 64`: short bands
    _r("fwd", L1, "c3_launch", "4, 16, 84, 84, 1, 6, false", "plain", 14, 2, 5, bmax=64),             # 28,672
    _r("fwd", C2, "c3_launch", "16, 24, 84, 84, 1, 6, false", "plain", 14, 2, 2, bmax=64),            # 65,536
    _r("fwd", C3, "c3_launch", "24, 32, 84, 84, 2, 3, false", "plain", 14, 2, 2, bmax=64),            # 59,392
    _r("fwd", G2, "c3_launch", "16, 24, 84, 84, 2, 3, false", "plain", 14, 2, 2, bmax=64),            # 59,392
    _r("fwd", C4, "c3_launch", "32, 64, 42, 42, 2, 3, false", "plain", 7, 2, 2, bmax=64),             # 57,344
    # ---- c3_fwd, no sign words, B > 64
    _r("fwd", L1, "c3s_launch", "4, 16, 84, 84, 1, 12, false", "plain", 7, 2, 1, bmin=65),
    _r("fwd", C2, "c3_launch", "16, 24, 84, 84, 1, 12, false", "plain", 7, 2, 1, bmin=65),            # 98,304
    _r("fwd", C3, "c3_launch", "24, 32, 84, 84, 2, 6, false", "plain", 7, 2, 1, bmin=65),             # 92,160
    _r("fwd", G2, "c3_launch", "16, 24, 84, 84, 2, 6, false", "plain", 7, 2, 1, bmin=65),             # 92,160
    _r("fwd", C4, "c3_launch", "32, 64, 42, 42, 2, 11, false", "plain", 2, 2, 1, bmin=65),            # 100,352
    # ---- c3_fwd, no sign words, any B
    _r("fwd", G3, "c3_launch", "24, 32, 42, 42, 2, 11, false", "plain", 2, 2, 2),                     # 81,920
    _r("fwd", G4, "c3_launch", "32, 48, 21, 21, 2, 11, false", "plain", 1, 2, 2),                     # 61,440
    _r("fwd", G5, "c3_launch", "48, 64, 11, 11, 2, 6, false, 24", "plain", 1, 2, 1),                  # 141,312
    # ---- c3_bwd_data, `mask != nullptr`: the float mask band staged in LDS (c3_kernel<.., BWD>, c3b_kernel: D = 2)
    _r("bwd", C2, "c3_launch", "24, 16, 84, 84, 1, 12, true", "mask", 7, 2, 1),                       # 154,624
    _r("bwd", C3, "c3b_launch", "32, 24, 42, 42, 6, 8", "mask", 7, 2, 1),                             # 135,680
    _r("bwd", G2, "c3b_launch", "24, 16, 42, 42, 6, 8", "mask", 7, 2, 1),                             # 93,184
    _r("bwd", C4, "c3b_launch", "64, 32, 21, 21, 11, 8", "mask", 2, 2, 1),                            # 155,136
    _r("bwd", G3, "c3b_launch", "32, 24, 21, 21, 11, 8", "mask", 2, 2, 1),                            # 125,568
    # ---- c3_bwd_data, sign words or no mask: the staged kernels (c3bs_kernel: D is its seventh template argument)
    _r("bwd", C2, "c3s_launch", "24, 16, 84, 84, 1, 6, true", "signs", 14, 2, 1),
    _r("bwd", C3, "c3bs_launch", "32, 24, 42, 42, 6, 8, 3, false", "signs", 7, 3, 1),
    _r("bwd", G2, "c3bs_launch", "24, 16, 42, 42, 6, 8, 4, true", "signs", 7, 4, 1),
    _r("bwd", C4, "c3bs_launch", "64, 32, 21, 21, 11, 8, 2, false", "signs", 2, 2, 1),
    _r("bwd", G3, "c3bs_launch", "32, 24, 21, 21, 11, 8, 3, true", "signs", 2, 3, 1),
    _r("bwd", G4, "c3bs_launch", "48, 32, 11, 11, 11, 16, 3, false, true", "signs", 1, 3, 1),         # odd image
    _r("bwd", G5, "c3bs_launch", "64, 48, 6, 6, 6, 16, 3, true, true, 3", "signs", 1, 3, 1),          # odd image
    # ---- C3W_CASES (CS, CD, H, W, S, R, KC, NCG, D)
    _r("wgrad", L1, "c3w_launch", "4, 16, 84, 84, 1, 6, 4, 1, 3", "wgrad", 14, 3, 3),
    _r("wgrad", C2, "c3w_launch", "16, 24, 84, 84, 1, 3, 16, 1, 3", "wgrad", 28, 3, 3),
    _r("wgrad", C3, "c3w_launch", "24, 32, 84, 84, 2, 6, 8, 2, 2", "wgrad", 7, 2, 3),
    _r("wgrad", C4, "c3w_launch", "32, 64, 42, 42, 2, 7, 8, 4, 3", "wgrad", 3, 3, 3),
    _r("wgrad", G2, "c3w_launch", "16, 24, 84, 84, 2, 6, 8, 1, 2", "wgrad", 7, 2, 3),
    _r("wgrad", G3, "c3w_launch", "24, 32, 42, 42, 2, 7, 12, 2, 3", "wgrad", 3, 3, 3),
    _r("wgrad", G4, "c3w_launch", "32, 48, 21, 21, 2, 11, 16, 4, 2", "wgrad", 1, 2, 3),
    # ---- C3W_OLD_CASES (A2C_C3W_D2=1)
    _r("wgrad_old", L1, "c3w_launch", "4, 16, 84, 84, 1, 8, 4, 1, 2", "wgrad", 11, 2, 3),
    _r("wgrad_old", C2, "c3w_launch", "16, 24, 84, 84, 1, 4, 16, 1, 2", "wgrad", 21, 2, 3),
    _r("wgrad_old", C4, "c3w_launch", "32, 64, 42, 42, 2, 7, 8, 4, 2", "wgrad", 3, 2, 3),
]
ORDER = {s: i for i, s in enumerate(LAYERS)}
REGIMES = ["one_round", "second_round", "ring_wrapped"]


def _rows(*kinds):
    return sorted((r for r in TABLE if r.kind in kinds), key=lambda r: ORDER[r.spec])


def _rid(r):
    return f"{NAMES[r.spec]}-{r.launcher}<{r.targs}>-{r.mode}"


def _cases(*kinds):
    return [pytest.param(r, k, id=f"{_rid(r)}-{REGIMES[k]}") for r in _rows(*kinds) for k in range(3)]


def _sizes(row, cus):
    """the three batch sizes of a row (module docstring), clamped to the row's window in the dispatch"""
    cap = cus * row.per_cu
    b2 = cap // row.nband + 1                               # smallest B with B * NBAND > cap
    b3 = -(-(row.D + 2) * cap // row.nband) + 1             # smallest B with B * NBAND >= (D + 2) * cap, plus one
    assert b2 * row.nband > cap >= (b2 - 1) * row.nband and (b3 - 1) * row.nband >= (row.D + 2) * cap > (b3 - 2) * row.nband
    return [min(max(b, row.bmin), row.bmax) for b in (1, b2, b3)]


def _nband_from_targs(row):
    a = [int(t) for t in row.targs.split(",")[:6]]
    if row.launcher in ("c3b_launch", "c3bs_launch"):       # (CO, CI, HO, WO, RQ, ..): bands of RQ class rows
        return -(-a[2] // a[4])
    cs, cd, h, w, s, r = a                                   # (CS, CD, H, W, S, R, ..): bands of R output rows
    return -(-((h - 1) // s + 1) // r)


def _ops():
    from a2c_amd import ops
    return ops


def _desc(spec):
    return _ops().conv_desc(*spec)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sign_words(t):
    """(B, C, H, W) bool -> (B, C*H*ceil(W/32)) int32: bit x & 31 of word [c][y][x >> 5] (a2c_conv2d_fwd_signs' layout)"""
    B, C, H, W = t.shape
    RW = (W + 31) // 32
    pad = np.zeros((B, C, H, RW * 32), dtype=np.uint8)
    pad[..., :W] = t.numpy()
    by = np.packbits(pad, axis=-1, bitorder="little")                      # (B, C, H, RW * 4) bytes, little endian words
    return torch.from_numpy(np.ascontiguousarray(by).view("<i4").reshape(B, -1).copy())


def _pad_is_sent(buf, n, sent=SENT):
    """rows of `buf` are n payload elements followed by padding: the padding still holds the sentinel"""
    return bool((buf[:, n:] == sent).all())


# ----------------------------------------------------------------------------------- fp32 evaluations in index order (e_t)
def _run32_fwd(x, w, b, s):
    """relu(conv(x, w) + b), 3x3 / pad 1 / stride s, as a plain fp32 running sum over (c, ky, kx) in index order: one
    rounded product and one rounded addition per term, the bias last (as the kernels add it)"""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    xp = F.pad(x, (1, 1, 1, 1))
    acc = torch.zeros(B, Cout, OH, OW)
    for c in range(Cin):
        for ky in range(3):
            for kx in range(3):
                xs = xp[:, c, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s]
                acc += xs[:, None] * w[None, :, c, ky, kx, None, None]
    acc += b[None, :, None, None]
    return torch.relu(acc)


def _run32_bwd(dout, w, s, H, W):
    """conv_transpose(dout, w) as a plain fp32 running sum over (co, ky, kx) in index order (no mask)"""
    B, Cout, OH, OW = dout.shape
    Cin = w.shape[1]
    acc = torch.zeros(B, Cin, H + 3, W + 3)                  # padded by one in front: y + 1 = s * oy + ky
    for co in range(Cout):
        for ky in range(3):
            for kx in range(3):
                acc[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] += \
                    dout[:, co, None] * w[co, :, ky, kx][None, :, None, None]
    return acc[:, :, 1:H + 1, 1:W + 1].contiguous()


def _ref64_fwd(x, w, b, s):
    return torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=1))


def _ref64_bwd(dout, w, s, H):
    return F.conv_transpose2d(dout.double(), w.double(), stride=s, padding=1, output_padding=(H + 2 - 3) % s)


def _wgrad64(x, dout, s, cuts):
    """fp64 (dW, db) summed over the samples [0, c) for every c in cuts: {c: (dW (Cout, Cin*9), db (Cout))}"""
    Cout = dout.shape[1]
    K = x.shape[1] * 9
    dW, db, out, a = torch.zeros(Cout, K, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64), {}, 0
    for c in sorted(set(cuts)):
        while a < c:
            b = min(a + 32, c)
            xu = F.unfold(x[a:b].double(), 3, padding=1, stride=s)                         # (n, K, L)
            do = dout[a:b].double().reshape(b - a, Cout, -1)
            dW += torch.einsum("ncl,nkl->ck", do, xu)
            db += do.sum((0, 2))
            a = b
        out[c] = (dW.clone(), db.clone())
    return out


def _run32_wgrad(x, dout, s):
    """per sample a running fp32 sum over the output positions in raster order, then a running sum over the samples
    -> (dW of the batch, db of the batch, dW of sample 0 alone, db of sample 0 alone)"""
    n, Cout = dout.shape[:2]
    xu = F.unfold(x, 3, padding=1, stride=s).permute(2, 0, 1).contiguous()                 # (L, n, K)
    do = dout.reshape(n, Cout, -1).permute(2, 0, 1).contiguous()                           # (L, n, Cout)
    sW, sb = torch.zeros(n, Cout, xu.shape[2]), torch.zeros(n, Cout)
    tmp = torch.empty_like(sW)
    for pos in range(xu.shape[0]):
        torch.mul(do[pos][:, :, None], xu[pos][:, None, :], out=tmp)
        sW += tmp
        sb += do[pos]
    return _running_sum(sW), _running_sum(sb), sW[0].clone(), sb[0].clone()


# ----------------------------------------------------------------------------------- pools: data and references, once per layer
_POOLS = {}
# samples of the fp32 evaluation: the largest of N rounding errors grows with N, so every layer's evaluation covers as many
# elements as 4 samples of the largest activation of the table (C.conv2's output, C.conv3's input: 24 x 84 x 84) -- 4
# samples there, 294 of G.conv5's 64 x 6 x 6 output.  A batch is compared with the evaluation of the samples it contains.
POOL_ELEMS = 4 * 24 * 84 * 84


def _npool(per_sample):
    return max(4, -(-POOL_ELEMS // per_sample))


def _pool(kind, spec, make):
    """one pool per kind at a time (the tests run layer by layer): inputs, the fp64 reference and the fp32 evaluation"""
    if kind not in _POOLS or _POOLS[kind][0] != spec:
        _POOLS.pop(kind, None)
        _POOLS[kind] = (spec, make())
    return _POOLS[kind][1]


def _weights(spec, seed):
    Cin, H, W, Cout, ks, s, p = spec
    w = _u((Cout, Cin, 3, 3), seed) / math.sqrt(Cin * 9)
    b = _u((Cout,), seed + 1) * 0.1
    return w, b


def _prep(spec, w):
    ops, d = _ops(), _desc(spec)
    wd = w.to(DEV)
    wf = torch.empty(ops.conv_prep_floats(d, 0), device=DEV)
    wb = torch.empty(ops.conv_prep_floats(d, 1), device=DEV)
    ops.conv_prep(d, 0, wd, wf)
    ops.conv_prep(d, 1, wd, wb)
    return wf, wb


def _batch_idx(B, last=None, before_last=None):
    """samples 0 .. B-1 of a pool with the special samples in the last places"""
    idx = list(range(B))
    if last is not None and B >= 2:
        idx[B - 1] = last
    if before_last is not None and B >= 3:
        idx[B - 2] = before_last
    return idx


def _fwd_pool(spec, n):
    def make():
        Cin, H, W, Cout, ks, s, p = spec
        x = _u((n + 1, Cin, H, W), 1000 + ORDER[spec], 0, 1)
        x[n] = 0                                                       # the all-zero sample
        w, b = _weights(spec, 1100 + 2 * ORDER[spec])
        ref = _ref64_fwd(x, w, b, s)
        npool = _npool(ref[0].numel())
        assert npool <= n
        wf, _ = _prep(spec, w)
        return dict(n=n, Z=n, x=x, w=w, b=b, ref=ref, t32=_run32_fwd(x[:npool], w, b, s), wf=wf, bd=b.to(DEV),
                    scale=max(float(x.abs().max()) * float(w.abs().max()), float(b.abs().max())))
    return _pool("fwd", spec, make)


def _bwd_pool(spec, n):
    def make():
        Cin, H, W, Cout, ks, s, p = spec
        OH = (H - 1) // s + 1
        dout = _u((n + 2, Cout, OH, OH), 1200 + ORDER[spec])
        mask = _u((n + 2, Cin, H, W), 1300 + ORDER[spec])
        dout[n] = 0                                                    # the all-zero sample
        mask[n + 1] = -mask[n + 1].abs()                               # a mask that is <= 0 everywhere,
        mask[n + 1, :, ::3] = 0.0                                      # exact zeros (and -0.0) among them
        w, _ = _weights(spec, 1400 + 2 * ORDER[spec])
        ref = _ref64_bwd(dout, w, s, H)
        npool = _npool(ref[0].numel())
        assert npool <= n
        _, wb = _prep(spec, w)
        return dict(n=n, Z=n, M=n + 1, dout=dout, mask=mask, w=w, ref=ref, t32=_run32_bwd(dout[:npool], w, s, H, W), wb=wb,
                    scale=float(dout.abs().max()) * float(w.abs().max()))
    return _pool("bwd", spec, make)


def _with_pool_rows(ref_b, idx, t32_pool, fix=None):
    """the fp32 evaluation laid out like the batch: the pool's samples where the batch has them, the fp64 value (no
    error) everywhere else, so that e_t is the pool's error and e_k covers the whole batch"""
    t32 = ref_b.clone()
    for j, i in enumerate(idx):
        if i < t32_pool.shape[0]:
            t32[j] = t32_pool[i].double() if fix is None else fix(j, t32_pool[i].double())
    return t32


def _batch(row, regime):
    """the batch size of the case, or None when clamping made it the size of the regime before it (that case has run)"""
    sizes = _sizes(row, _cus())
    return None if regime > 0 and sizes[regime] == sizes[regime - 1] else sizes[regime]


def _max_b(kinds, spec):
    return max(_sizes(r, _cus())[2] for r in TABLE if r.kind in kinds and r.spec == spec)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    _POOLS.clear()
    print(f"\ntest_gpu_conv3: {time.time() - t0:.1f} s; worst e_k / e_t per array over this run:")
    for k in sorted(SK._RATIOS):
        if k.startswith("c3."):
            print(f"  RATIO {k} {SK._RATIOS[k]:.3f}")


# =================================================================================== the table against the source (CPU)
def _source_instances():
    src = open(HIP).read()

    def between(a, b):
        i = src.index(a)
        return src[i:src.index(b, i)]

    launch = re.compile(r"\b(c3s?_launch|c3bs?_launch)<([^>]*)>\(p, st\)")
    norm = lambda s: s.replace(" ", "")
    fwd = {(m.group(1), norm(m.group(2))) for m in launch.finditer(between("\nint c3_fwd(", "\nbool c3_chain_supported("))}
    bwd = {(m.group(1), norm(m.group(2))) for m in launch.finditer(between("\nint c3_bwd_data(", "\nbool c3_bwd_data_w1_frames_supported("))}
    case = re.compile(r"\bX\((\d[\d, ]*)\)")
    new = {("c3w_launch", norm(m.group(1))) for m in case.finditer(between("#define C3W_CASES(X)", "#define C3W_OLD_CASES(X)"))}
    old = {("c3w_launch", norm(m.group(1))) for m in case.finditer(between("#define C3W_OLD_CASES(X)", "\nbool c3w_supported("))}
    return fwd, bwd, new, old


def test_table_has_every_instance_of_the_dispatch():
    fwd, bwd, new, old = _source_instances()
    assert len(fwd) == 24 and len(bwd) == 12 and len(new) == 7 and len(old) == 3, (len(fwd), len(bwd), len(new), len(old))
    for kind, want in (("fwd", fwd), ("bwd", bwd), ("wgrad", new), ("wgrad_old", old)):
        have = {(r.launcher, r.targs) for r in TABLE if r.kind == kind}
        assert have == want, (kind, sorted(want - have), sorted(have - want))
    for r in TABLE:
        assert r.nband == _nband_from_targs(r), r
        if r.launcher == "c3w_launch":
            assert r.D == int(r.targs.split(",")[8]) and r.per_cu == 3, r
        elif r.launcher == "c3bs_launch":
            assert r.D == int(r.targs.split(",")[6]) and r.per_cu == 1, r
        else:
            assert r.D == 2 and (r.per_cu == 1 or r.launcher in ("c3_launch", "c3b_launch")), r
    # c3s_launch<4, 16, 84, 84, 1, 12, false> serves two branches of c3_fwd: every (instance, mode) of the forward is a row
    assert len(_rows("fwd")) == 25 and len(_rows("bwd")) == 12


def test_table_agrees_with_the_public_predicates():
    """(the predicates are host code: no device needed)"""
    ops = _ops()
    sign_capable = {r.spec for r in TABLE if r.kind == "fwd" and r.mode == "signs"}
    bwd_specs = {r.spec for r in TABLE if r.kind == "bwd"}
    assert sign_capable == set(LAYERS) - {G5} and bwd_specs == set(LAYERS) - {L1}
    for spec in LAYERS:
        d = _desc(spec)
        Cin, H, W, Cout, ks, s, p = spec
        nsw = ops.conv_sign_words(d)
        assert (nsw != 0) == (spec in sign_capable), spec
        if nsw:
            assert nsw == Cout * d.OH * ((d.OW + 31) // 32)
        assert ops.conv_bwd_data_signs_supported(d) == (spec in bwd_specs), spec
        assert ops.conv_prep_floats(d, 0) > 0 and ops.conv_prep_floats(d, 1) > 0
    # every layer outside the table: no sign words, no sign-word backward-data
    for spec in [(4, 84, 84, 16, 8, 4, 0), (16, 20, 20, 32, 4, 2, 0), (4, 20, 20, 16, 3, 1, 1), (8, 13, 17, 12, 3, 2, 1)]:
        d = _desc(spec)
        assert ops.conv_sign_words(d) == 0 and not ops.conv_bwd_data_signs_supported(d)


def test_batch_sizes_follow_the_geometry():
    """256 CUs: the sizes the issue names, and the forward's 64 / 65 switch on both sides"""
    by = {(r.kind, r.spec, r.targs, r.mode): _sizes(r, 256) for r in TABLE}
    assert by[("fwd", L1, "4,16,84,84,1,12,false", "signs")] == [1, 37, 148]
    assert by[("fwd", G4, "32,48,21,21,2,11,false", "plain")] == [1, 513, 2049]
    assert by[("bwd", G2, "24,16,42,42,6,8,4,true", "signs")] == [1, 37, 221]
    assert by[("bwd", G5, "64,48,6,6,6,16,3,true,true,3", "signs")] == [1, 257, 1281]
    assert by[("wgrad", L1, "4,16,84,84,1,6,4,1,3", "wgrad")] == [1, 55, 276]
    assert by[("wgrad", G4, "32,48,21,21,2,11,16,4,2", "wgrad")] == [1, 769, 3073]
    for r in TABLE:
        s = _sizes(r, 256)
        assert s == sorted(s) and s[0] == r.bmin
        if r.bmax == 64:
            assert s[2] == 64, r                  # the last size of a B <= 64 row is the switch itself
        if r.bmin == 65:
            assert s[0] == 65 and s[2] > 65, r
    for spec in (L1, C2, C3, C4, G2):             # the layers whose plain forward switches: both sides are rows
        assert {r.bmax for r in TABLE if r.kind == "fwd" and r.spec == spec and r.mode == "plain"} == {64, BIG}


def test_the_checker_can_fail():
    """the criterion rejects two adjacent bands of a late-round sample swapped and one band off by 1e-4 relative; the
    sentinel check rejects a one-element overrun"""
    Cin, H, W, Cout, ks, s, p = G3
    B, R = 6, 11                                              # c3_launch<24, 32, 42, 42, 2, 11>: bands of rows 0..10, 11..20
    x = _u((B, Cin, H, W), 7, 0, 1)
    w, b = _weights(G3, 8)
    ref = _ref64_fwd(x, w, b, s)
    t32 = _with_pool_rows(ref, list(range(B)), _run32_fwd(x[:4], w, b, s))
    scale = max(float(x.abs().max()) * float(w.abs().max()), float(b.abs().max()))
    good = ref.float()
    _crit("selftest.good", good, t32, ref, scale)
    swapped = good.clone()
    swapped[B - 1, :, 0:R - 1], swapped[B - 1, :, R:2 * R - 1] = good[B - 1, :, R:2 * R - 1], good[B - 1, :, 0:R - 1]
    with pytest.raises(AssertionError):
        _crit("selftest.swapped", swapped, t32, ref, scale)
    off = good.clone()
    off[B - 1, :, R:] *= 1 + 1e-4
    with pytest.raises(AssertionError):
        _crit("selftest.off", off, t32, ref, scale)
    for k in [k for k in SK._RATIOS if k.startswith("selftest")]:
        del SK._RATIOS[k]
    n = Cout * 21 * 21
    buf = torch.full((B, n + 8), SENT)
    buf[:, :n] = good.reshape(B, -1)
    assert _pad_is_sent(buf, n)
    buf[B - 1, n] = good.reshape(B, -1)[B - 1, 0]              # one element past the last band of the last sample
    assert not _pad_is_sent(buf, n)
    sg = torch.full((B, 10), -7, dtype=torch.int32)
    sg[2, 5] = 0
    assert _pad_is_sent(sg, 6, -7) and not _pad_is_sent(sg, 5, -7) and _pad_is_sent(sg[:2], 5, -7)


# =================================================================================== forward
@pytest.mark.gpu
@pytest.mark.parametrize("row,regime", _cases("fwd"))
def test_forward(row, regime):
    ops, d = _ops(), _desc(row.spec)
    Cin, H, W, Cout, ks, s, p = row.spec
    B = _batch(row, regime)
    if B is None:
        return
    P = _fwd_pool(row.spec, _max_b(("fwd",), row.spec))
    idx = _batch_idx(B, last=P["Z"])
    xd = P["x"][idx].to(DEV)
    n, nin = Cout * d.OH * d.OW, Cin * H * W
    ob = n + 8                                                # rows of a wider buffer: out_bstride > Cout * OH * OW
    out = torch.full((B, ob), SENT, device=DEV)
    if row.mode == "signs":
        nsw = ops.conv_sign_words(d)
        sg = torch.full((B, nsw + 5), -7, dtype=torch.int32, device=DEV)
        ops.conv_fwd_signs(d, xd.data_ptr(), nin, P["wf"], P["bd"], True, out.data_ptr(), sg.data_ptr(), nsw + 5, B, out_bstride=ob)
        plain = torch.full((B, ob), SENT, device=DEV)
        ops.conv_fwd(d, xd.data_ptr(), nin, P["wf"], P["bd"], True, plain.data_ptr(), B, out_bstride=ob)
        assert torch.equal(out, plain), "a2c_conv2d_fwd_signs' output is not the plain forward's"
        sgc = sg.cpu()
        assert torch.equal(sgc[:, :nsw], _sign_words(out[:, :n].cpu().view(B, Cout, d.OH, d.OW) > 0)), "sign words != (out > 0)"
        assert _pad_is_sent(sgc, nsw, -7), "sign-word rows overrun"
    else:
        ops.conv_fwd(d, xd.data_ptr(), nin, P["wf"], P["bd"], True, out.data_ptr(), B, out_bstride=ob)
    oc = out.cpu()
    assert _pad_is_sent(oc, n), "output rows overrun"
    got = oc[:, :n]
    assert bool(torch.isfinite(got).all())
    ref = P["ref"][idx].reshape(B, n)
    t32 = _with_pool_rows(ref, idx, P["t32"].reshape(-1, n))
    # scale: the largest single term of an output element, max|x| max|w| (or max|bias|)
    _crit(f"c3.fwd.out {_rid(row)} B={B}", got, t32, ref, scale=P["scale"])


# =================================================================================== backward-data
def _bwd_cases():
    out = []
    for r in _rows("bwd"):
        odd = r.spec[1] % 2 == 1
        modes = ["mask"] if r.mode == "mask" else (["signs", "none", "mask_generic"] if odd else ["signs", "none"])
        out += [pytest.param(r, m, k, id=f"{_rid(r)}-{m}-{REGIMES[k]}") for m in modes for k in range(3)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("row,mode,regime", _bwd_cases())
def test_backward_data(row, mode, regime, monkeypatch):
    """mask: a2c_conv2d_bwd_data with the float activation; signs: a2c_conv2d_bwd_data_signs with its sign words (rows of a
    wider buffer); none: both entry points without a mask (the staged kernels); mask_generic: the float mask on the two
    odd images, which have no float-mask instance in the table: conv.hip's band kernel (A2C_NO_TUNE=1: no timed search)"""
    ops, d = _ops(), _desc(row.spec)
    Cin, H, W, Cout, ks, s, p = row.spec
    B = _batch(row, regime)
    if B is None:
        return
    P = _bwd_pool(row.spec, _max_b(("bwd",), row.spec))
    idx = _batch_idx(B, last=P["M"], before_last=P["Z"])
    dout, mask = P["dout"][idx].to(DEV), P["mask"][idx]
    n = Cin * H * W
    buf = torch.full((B * n + 16,), SENT, device=DEV)         # din is dense: the guard is behind the last sample
    din = buf[:B * n].view(B, Cin, H, W)
    if mode == "mask_generic":
        monkeypatch.setenv("A2C_NO_TUNE", "1")
    if mode in ("mask", "mask_generic"):
        ops.conv_bwd_data(d, dout, P["wb"], mask.to(DEV), din, B)
    elif mode == "signs":
        nw = Cin * H * ((W + 31) // 32)
        words = torch.full((B, nw + 3), -1, dtype=torch.int32)
        words[:, :nw] = _sign_words(mask > 0)
        ops.conv_bwd_data_signs(d, dout, P["wb"], words.to(DEV)[:, :nw], din, B)
        if H % 2 == 0:       # even images: the float-mask kernel is the same streaming family, same order of the sums
            din_f = torch.full((B, Cin, H, W), SENT, device=DEV)
            ops.conv_bwd_data(d, dout, P["wb"], mask.to(DEV), din_f, B)
            assert torch.equal(din, din_f), "sign-word and float-mask backward-data differ"
    else:
        ops.conv_bwd_data_signs(d, dout, P["wb"], None, din, B)
        din_f = torch.full((B, Cin, H, W), SENT, device=DEV)
        ops.conv_bwd_data(d, dout, P["wb"], None, din_f, B)
        assert torch.equal(din, din_f), "the two entry points without a mask differ"
    bc = buf.cpu()
    assert bool((bc[B * n:] == SENT).all()), "din overrun"
    got = bc[:B * n].view(B, n)
    assert bool(torch.isfinite(got).all())
    keep = (mask > 0).reshape(B, n) if mode != "none" else torch.ones(B, n, dtype=torch.bool)
    ref = P["ref"][idx].reshape(B, n) * keep
    t32 = _with_pool_rows(ref, idx, P["t32"].reshape(-1, n), fix=lambda j, t: t * keep[j])
    if mode != "none" and B >= 2:
        assert bool((got[B - 1] == 0).all()), "a mask that is <= 0 everywhere lets something through"
    # scale: the largest single term of an input-gradient element, max|dout| max|w|
    _crit(f"c3.bwd.din.{mode} {_rid(row)} B={B}", got, t32, ref, scale=P["scale"])


# =================================================================================== weight gradient
def _wgrad_pool(spec, frames=False):
    """x, dout of the largest batch of the layer's rows (+ the all-zero sample), the fp64 gradient of every prefix the rows
    need, and the fp32 running sums on the middle batch of the layer's default instance"""
    def make():
        Cin, H, W, Cout, ks, s, p = spec
        cus = _cus()
        rows = [r for r in TABLE if r.kind in ("wgrad", "wgrad_old") and r.spec == spec and not (frames and r.kind == "wgrad_old")]
        n = max(_sizes(r, cus)[2] for r in rows)
        mid = _sizes([r for r in rows if r.kind == "wgrad"][0], cus)[1]
        OH = (H - 1) // s + 1
        extra = {}
        if frames:               # a single-frame uint8 store (R slots of T + 4 frames) and the states it stands for
            T = 5
            R = (n + T - 1) // T
            rng = np.random.default_rng(77)
            Fs = rng.integers(0, 256, size=(R, T + 4, H * W), dtype=np.uint8)
            nv = rng.integers(1, 5, size=(R * T,), dtype=np.int32)
            win = np.lib.stride_tricks.sliding_window_view(Fs, 4, axis=1)[:, :T]            # [r][t][px][c] = Fs[r][t + c][px]
            st = np.ascontiguousarray(win.transpose(0, 1, 3, 2)).reshape(R * T, 4, H * W).astype(np.float32)
            st *= (np.arange(4)[None, :] >= 4 - nv[:, None])[:, :, None]                    # planes from before the reset read as zero
            x = torch.cat([torch.from_numpy(st[:n]).reshape(n, 4, H, W), torch.zeros(1, 4, H, W)])
            extra = dict(Fs=torch.from_numpy(Fs).to(DEV), nv=torch.from_numpy(nv).to(DEV), T=T)
        else:
            x = _u((n + 1, Cin, H, W), 1500 + ORDER[spec], 0, 1)
            x[n] = 0                                                   # the all-zero sample
        dout = _u((n + 1, Cout, OH, OH), 1600 + ORDER[spec])
        cuts = {1, mid, mid - 1}
        for r in rows:
            for b in _sizes(r, cus):
                cuts |= {b, b - 1} if frames else {b - 1}
        cuts.discard(0)
        pre = _wgrad64(x[:n], dout[:n], s, cuts)
        zb = dout[n].double().sum((1, 2))                              # the all-zero sample adds nothing to dW, this to db
        if frames:
            midx = list(range(mid))
            mW, mb = pre[mid]
        else:
            midx = _batch_idx(mid, last=n)
            mW, mb = pre[mid - 1][0], pre[mid - 1][1] + zb
        rW, rb, rW0, rb0 = _run32_wgrad(x[midx], dout[midx], s)
        eW, eb = float((rW.double() - mW).abs().max()), float((rb.double() - mb).abs().max())
        eW0, eb0 = float((rW0.double() - pre[1][0]).abs().max()), float((rb0.double() - pre[1][1]).abs().max())
        return dict(n=n, Z=n, x=x, dout=dout, pre=pre, zb=zb, mid=mid, e=(eW, eb), e0=(eW0, eb0),
                    scale=(float(dout.abs().max()) * float(x.abs().max()), float(dout.abs().max())), **extra)
    return _pool("frames" if frames else "wgrad", spec, make)


def _crit_wgrad(tag, P, B, dW, db, wantW, wantb, grow=False):
    """_crit with e_t given as a number: the fp32 evaluation is the fp64 reference with one element moved by e_t.
    grow (a2c_conv2d_bwd_weight's dW and db only): e_t comes from the middle batch of `mid` samples and is reused for the
    ring-wrap batch of (D + 2) times as many.  Measured on the MI355X, dW there is at 2.0 - 4.4 e_t(mid) and db at up to
    4.3 e_t(mid), for reasons of order alone: c3w_reduce_kernel adds the slabs of up to 768 workgroups x 8 pixel groups as one
    running fp32 sum, and the error of a running sum grows with the number of its terms -- between sqrt(B / mid) (measured
    for e_t itself on conv1: 1.03e-3, 1.55e-3, 2.41e-3 at 55, 138, 276 samples) and B / mid (the growth of the bound n u
    sum|t|).  For B > mid the factor of both arrays is therefore 2 B / mid, and never more than what test_conv2d_fwd_bwd
    allows, 1e-5 max|grad|."""
    eW, eb = P["e0"] if B == 1 else P["e"]
    if grow and B > P["mid"]:
        for name, got, want, e in (("dW", dW, wantW, eW), ("db", db, wantb, eb)):
            e_k = float((got.double().reshape(-1) - want.reshape(-1)).abs().max())
            cap = 1e-5 * float(want.abs().max())
            print(f"    {tag}.{name} B={B}: e_k / e_t(mid = {P['mid']}) {e_k / e:.3f}; 1e-5 max|{name}| = {cap:.3e}")
            k = f"{tag.split(' ')[0]}.{name}/e_t(mid)"
            SK._RATIOS[k] = max(SK._RATIOS.get(k, 0.0), e_k / e)
            assert e_k <= cap, f"{tag}.{name}: e_k {e_k:.3e} > 1e-5 max|{name}| = {cap:.3e}"
        eW, eb = eW * B / P["mid"], eb * B / P["mid"]
    for name, got, want, e, scale in (("dW", dW, wantW, eW, P["scale"][0]), ("db", db, wantb, eb, P["scale"][1])):
        want = want.reshape(-1)
        t32 = want.clone()
        t32[0] += e
        # scale: the largest single term of a gradient element, max|dout| max|x| (dW) / max|dout| (db)
        _crit(f"{tag}.{name} B={B}", got.reshape(-1), t32, want, scale=scale)


@pytest.mark.gpu
@pytest.mark.parametrize("row,regime", _cases("wgrad", "wgrad_old"))
def test_weight_gradient(row, regime, monkeypatch):
    ops, d = _ops(), _desc(row.spec)
    Cin, H, W, Cout, ks, s, p = row.spec
    old = row.kind == "wgrad_old"
    if old:
        assert ("c3w_launch", row.targs) in _source_instances()[3]           # the switch below reaches this very instance
        monkeypatch.setenv("A2C_C3W_D2", "1")
    else:
        monkeypatch.delenv("A2C_C3W_D2", raising=False)
    B = _sizes(row, _cus())[regime]
    P = _wgrad_pool(row.spec)
    idx = _batch_idx(B, last=P["Z"])
    xd, dout = P["x"][idx].to(DEV), P["dout"][idx].to(DEV)
    need = ops.conv_bwd_weight_ws_bytes(d, B)
    ws = torch.full((need // 4 + 4,), SENT, device=DEV)
    bufW = torch.full((Cout * Cin * 9 + 4,), SENT, device=DEV)
    bufb = torch.full((Cout + 4,), SENT, device=DEV)
    dW, db = bufW[:Cout * Cin * 9].view(Cout, Cin, 3, 3), bufb[:Cout]
    ops.conv_bwd_weight(d, xd.data_ptr(), Cin * H * W, dout, dW, db, B, ws[:need // 4])
    assert bool((bufW[Cout * Cin * 9:] == SENT).all()) and bool((bufb[Cout:] == SENT).all()) and bool((ws[need // 4:] == SENT).all())
    if B == 1:
        wantW, wantb = P["pre"][1]
    else:
        wantW, wantb = P["pre"][B - 1][0], P["pre"][B - 1][1] + P["zb"]
    _crit_wgrad(f"c3.{row.kind}", P, B, dW.cpu(), db.cpu(), wantW, wantb, grow=True)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", range(3), ids=REGIMES)
def test_weight_gradient_from_frames(regime):
    """a2c_conv2d_bwd_weight_frames: the first layer's gradient from a uint8 single-frame store with 1..4 valid planes per
    sample, against fp64 of the states the store stands for (pixels 0..255: scale = 255 max|dout|)"""
    ops, d = _ops(), _desc(L1)
    row = [r for r in TABLE if r.kind == "wgrad" and r.spec == L1][0]
    B = _sizes(row, _cus())[regime]
    P = _wgrad_pool(L1, frames=True)
    dout = P["dout"][:B].to(DEV)
    need = ops.conv_bwd_weight_ws_bytes(d, B)
    ws = torch.empty(need // 4, device=DEV)
    dW, db = torch.full((16, 4, 3, 3), SENT, device=DEV), torch.full((16,), SENT, device=DEV)
    ops.conv_bwd_weight_frames(d, P["Fs"], P["Fs"].stride(0), P["T"], P["nv"], dout, dW, db, B, ws)
    _crit_wgrad("c3.frames", P, B, dW.cpu(), db.cpu(), *P["pre"][B])


# =================================================================================== fall-backs at the table shapes, B = 3
_SMALL = {}


def _small(spec):
    """B = 3 of everything, its fp64 references and fp32 evaluations"""
    if spec not in _SMALL:
        Cin, H, W, Cout, ks, s, p = spec
        OH = (H - 1) // s + 1
        x, dout, mask = _u((3, Cin, H, W), 2000, 0, 1), _u((3, Cout, OH, OH), 2001), _u((3, Cin, H, W), 2002)
        w, _ = _weights(spec, 2003)
        pre = _wgrad64(x, dout, s, {1, 3})
        rW, rb, _, _ = _run32_wgrad(x, dout, s)
        _, wb = _prep(spec, w)
        _SMALL[spec] = dict(x=x, dout=dout, mask=mask, w=w, wb=wb, din=_ref64_bwd(dout, w, s, H), din32=_run32_bwd(dout, w, s, H, W),
                            pre=pre, e=(float((rW.double() - pre[3][0]).abs().max()), float((rb.double() - pre[3][1]).abs().max())),
                            e0=None, mid=3, scale=(float(dout.abs().max()) * float(x.abs().max()), float(dout.abs().max())))
    return _SMALL[spec]


def _offset(t, floats=1):
    """a copy of t on the device that starts `floats` * 4 bytes behind a 16-byte boundary"""
    buf = torch.full((t.numel() + 8,), SENT, device=DEV, dtype=t.dtype)
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * floats
    return v


WGRAD_FALLBACKS = ["in_bstride", "dout", "dW", "ws"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGRAD_FALLBACKS)
@pytest.mark.parametrize("spec", [r.spec for r in _rows("wgrad")], ids=lambda s: NAMES[s])
def test_weight_gradient_fallback(spec, case, monkeypatch):
    """a sample stride that is no multiple of 4 floats, or dout / dW / the workspace 4 bytes off a 16-byte boundary: the
    call leaves conv3.hip for conv.hip's generic kernels and must meet the same criterion"""
    monkeypatch.setenv("A2C_NO_TUNE", "1")
    ops, d = _ops(), _desc(spec)
    Cin, H, W, Cout, ks, s, p = spec
    S = _small(spec)
    B, nin = 3, Cin * H * W
    bs = nin + (3 if case == "in_bstride" else 0)
    xbuf = torch.full((B, bs), SENT, device=DEV)
    xbuf[:, :nin] = S["x"].reshape(B, -1).to(DEV)
    dout = _offset(S["dout"]) if case == "dout" else S["dout"].to(DEV)
    dW = _offset(torch.full((Cout, Cin, 3, 3), SENT)) if case == "dW" else torch.full((Cout, Cin, 3, 3), SENT, device=DEV)
    db = torch.full((Cout,), SENT, device=DEV)
    need = ops.conv_bwd_weight_ws_bytes(d, B)
    ws = torch.empty(need // 4 + 8, device=DEV)
    ws = ws[1:1 + need // 4] if case == "ws" else ws[:need // 4]
    assert ws.data_ptr() % 16 == (4 if case == "ws" else 0)
    ops.conv_bwd_weight(d, xbuf.data_ptr(), bs, dout, dW, db, B, ws)
    _crit_wgrad(f"c3.fallback.wgrad.{case} {NAMES[spec]}", S, B, dW.cpu(), db.cpu(), *S["pre"][3])


BWD_FALLBACKS = ["dout", "din", "mask", "no_odd_bs", "no_odd_bs_none"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_FALLBACKS)
@pytest.mark.parametrize("spec", [s for s in LAYERS if s != L1], ids=lambda s: NAMES[s])
def test_backward_data_fallback(spec, case, monkeypatch):
    """dout, din or the mask 4 bytes off a 16-byte boundary (every layer of c3_bwd_data), A2C_NO_ODD_BS=1 (the two odd images,
    with the float mask and without a mask): conv.hip's generic band kernel, same criterion"""
    Cin, H, W, Cout, ks, s, p = spec
    odd = H % 2 == 1
    if case.startswith("no_odd_bs"):
        if not odd:
            return                                             # (the switch only exists for the odd images)
        monkeypatch.setenv("A2C_NO_ODD_BS", "1")
    monkeypatch.setenv("A2C_NO_TUNE", "1")
    ops, d = _ops(), _desc(spec)
    if case.startswith("no_odd_bs"):
        assert not ops.conv_bwd_data_signs_supported(d)
    S = _small(spec)
    B, n = 3, Cin * H * W
    dout = _offset(S["dout"]) if case == "dout" else S["dout"].to(DEV)
    with_mask = case != "no_odd_bs_none"
    mask = None if not with_mask else (_offset(S["mask"]) if case == "mask" else S["mask"].to(DEV))
    din = _offset(torch.full((B, Cin, H, W), SENT)) if case == "din" else torch.full((B, Cin, H, W), SENT, device=DEV)
    ops.conv_bwd_data(d, dout, S["wb"], mask, din, B)
    keep = (S["mask"] > 0) if with_mask else torch.ones_like(S["mask"], dtype=torch.bool)
    # scale: the largest single term, max|dout| max|w|
    _crit(f"c3.fallback.bwd.{case} {NAMES[spec]}", din.cpu(), S["din32"].double() * keep, S["din"] * keep,
          scale=float(S["dout"].abs().max()) * float(S["w"].abs().max()))


# =================================================================================== argument edges
@pytest.mark.gpu
@pytest.mark.parametrize("spec", LAYERS, ids=lambda s: NAMES[s])
def test_argument_edges(spec):
    ops, d = _ops(), _desc(spec)
    Cin, H, W, Cout, ks, s, p = spec
    S = _small(spec)
    w, b = _weights(spec, 2003)
    wf, wb = _prep(spec, w)
    xd, dout, bd = S["x"].to(DEV), S["dout"].to(DEV), b.to(DEV)
    out, din = torch.full_like(dout, SENT), torch.full_like(xd, SENT)
    # B = 0: OK, nothing written
    ops.conv_fwd(d, xd.data_ptr(), Cin * H * W, wf, bd, True, out, 0)
    ops.conv_bwd_data(d, dout, wb, xd, din, 0)
    nsw = ops.conv_sign_words(d)
    if nsw:
        sg = torch.full((3, nsw), -7, dtype=torch.int32, device=DEV)
        ops.conv_fwd_signs(d, xd.data_ptr(), Cin * H * W, wf, bd, True, out, sg.data_ptr(), nsw, 0)
        assert bool((sg == -7).all())
    if ops.conv_bwd_data_signs_supported(d):
        ops.conv_bwd_data_signs(d, dout, wb, None, din, 0)
    assert bool((out == SENT).all()) and bool((din == SENT).all())
    # weight gradient: B = 0 is an argument error, a workspace one byte short a workspace error; nothing written
    dW, db = torch.full((Cout, Cin, 3, 3), SENT, device=DEV), torch.full((Cout,), SENT, device=DEV)
    need = ops.conv_bwd_weight_ws_bytes(d, 3)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    SK._raises(ERR_ARG, ops.conv_bwd_weight, d, xd.data_ptr(), Cin * H * W, dout, dW, db, 0, ws)
    SK._raises(ERR_WORKSPACE, ops.conv_bwd_weight, d, xd.data_ptr(), Cin * H * W, dout, dW, db, 3, ws[:need - 1])
    assert bool((dW == SENT).all()) and bool((db == SENT).all()) and bool((ws == 0x5A).all())
    ops.conv_bwd_weight(d, xd.data_ptr(), Cin * H * W, dout, dW, db, 3, ws)             # exactly `need` bytes are enough
    _crit_wgrad(f"c3.edges.wgrad {NAMES[spec]}", S, 3, dW.cpu(), db.cpu(), *S["pre"][3])
