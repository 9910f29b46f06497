"""CPU: a twin of the dispatcher of csrc/gemm.hip -- a2c_gemm_f32 and a2c_gemm_f32_partial pick one of about thirty kernel
instantiations from (transA, transB, M, N, K, ld*, pointer alignment, epilogue flags, splitk, workspace size, three
environment switches) and the caller cannot see which one ran.  `route` repeats that choice and names it; `CASES` is the
case list of tests/test_gpu_gemm_routes.py, as data, with the route each case is MEANT to take.  The tests here hold the
two together without a GPU:

  * every kernel instantiation launched from the dispatching functions of gemm.hip has an entry in ROUTES / AUX, and the
    text of every condition and derived quantity in those functions equals the copy in CONDITIONS (whitespace
    normalised): editing a launch or a condition in gemm.hip breaks a test here until the twin is revisited;
  * every route family and auxiliary kernel is reached by CASES, every case lands where it says, both sides of every
    threshold in THRESHOLDS are present and land on different routes, the ring kernels run at 1, 2, LOOK, LOOK + 1 and
    about ten K tiles per split and with last splits of 4, 28 and 32 columns, small_gemm_kernel sees every kind of wave,
    and no case needs more than 256 MB of workspace or M N K >= 3e8 (the fp32 running-sum reference of 65 x 130 x 32772
    takes 0.7 s);
  * the shape lists of the older GEMM tests are pushed through `route` and printed (`pytest -s`): which kernel serves
    which of their cases today.

What the twin shows cannot be a case: gemm_nt<Big> at M = 256 and the M = 256 / 257 edge (N K >= 2^22 puts M N K at 1.07e9
or more, over the 3e8 a case is held to; test_gemm_rollout_batch_forward_...[256] of test_gpu_kernels.py runs M = 256 at 73
tiles per split), and for the same reason the t32 = 512 / 513 edge of `deep` (K >= 1024 and 512 full tiles are 5.4e8).
`t32 <= 4096` of the small-product condition is never the deciding term: t128 < 64 already holds t32 to 1008.  (33, 95) of
the older tests is no small product (t32 = 6 and M > 32); (33, 225) takes its place, and (33, 95) stays as a fall-through.

A route name is `family attr ... +aux ...`: the family is the kernel instantiation as gemm.hip writes it (blanks removed),
the attributes are what matters inside it (vA / vB / vec_epi of gemm_kernel; nch, bands, Kc of the small-N weight
gradient; splits, K tiles of the shortest and longest split and columns of the last one for gemm_nt / skinny_stream; s6
of the x 6 path), and `+reduce`, `+wreduce`, `+splitA<..>`, `+splitB<..>` are the further launches of the call (AUX).
"""
import os
import re

import pytest

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-a2c_amd", "csrc", "gemm.hip")

# ------------------------------------------------------------------------------------------------ constants of gemm.hip
BK, SN_MAX, SN_BANDS = 16, 8, 512
NT_BKT = 32
NT_TM = {"nt::Skinny": 32, "nt::Big": 256}
NT_LOOK = {"nt::Skinny": 3, "nt::Big": 2}          # DEPTH - 1 tiles in flight ahead of the one computed

ROUTES = {
    "small_n_fwd_kernel": "N <= 8 heads forward, a wave per row",
    "small_n_bwd_data_kernel": "K <= 8 heads backward-data, float4 columns",
    "small_n_bwd_weight_kernel": "M <= 8 heads weight gradient, row bands + column chunks",
    "small_k_tn_kernel<4>": "rank-K outer-product sum, float4 columns",
    "small_k_tn_kernel<1>": "rank-K outer-product sum, scalar columns",
    "small_gemm_kernel<true,8>": "one-launch small product, B k-contiguous, eight waves share K",
    "small_gemm_kernel<true,4>": "one-launch small product, B k-contiguous, four waves",
    "small_gemm_kernel<false,8>": "one-launch small product, B n-contiguous, eight waves",
    "small_gemm_kernel<false,4>": "one-launch small product, B n-contiguous, four waves",
    "gemm_kernel<true,true,true>": "block-tiled NT, M <= 96 (32-row blocks of padding skipped)",
    "gemm_kernel<true,true,false>": "block-tiled NT",
    "gemm_kernel<true,false,true>": "block-tiled NN, M <= 96",
    "gemm_kernel<true,false,false>": "block-tiled NN",
    "gemm_kernel<false,true,true>": "block-tiled TT, M <= 96",
    "gemm_kernel<false,true,false>": "block-tiled TT",
    "gemm_kernel<false,false,true>": "block-tiled TN, M <= 96",
    "gemm_kernel<false,false,false>": "block-tiled TN",
    "gemm_nt_kernel<nt::Skinny>": "LDS-DMA ring, 32 x 256 tile, DEPTH 4 (M <= 32)",
    "gemm_nt_kernel<nt::Big>": "LDS-DMA ring, 256 x 128 tile, DEPTH 3 (64 < M <= 256)",
    "skinny_stream_kernel<1,4>": "LDS-free stream, one 32-row block (M <= 32, only with A2C_NO_GEMM_NT=1)",
    "skinny_stream_kernel<2,4>": "LDS-free stream, two 32-row blocks (32 < M <= 64)",
    "gemm_x6_kernel": "six bf16 piece products from panel images",
}
AUX = {
    "+reduce": "splitk_reduce_kernel",
    "+wreduce": "small_n_bwd_weight_reduce",
    "+splitA<false>": "x6_split_kernel<false>", "+splitA<true>": "x6_split_kernel<true>",
    "+splitB<false>": "x6_split_kernel<false>", "+splitB<true>": "x6_split_kernel<true>",
}
REFUSALS = {"ERR_ARG", "ERR_WORKSPACE", "nothing"}

# the functions of gemm.hip the twin repeats, and for each the text of its conditions (if / else if / while) and of the
# derived quantities the choice hangs on, in source order, whitespace normalised
DISPATCH_FUNCTIONS = ["launch_skinny_stream", "launch_gemm_nt_shape", "launch_gemm_nt", "launch_gemm", "x6_split", "x6_run",
                      "a2c_gemm_ws_bytes", "x9_eligible", "a2c_gemm_x9_ws_bytes", "a2c_gemm_f32", "gemm_kps", "a2c_gemm_splits",
                      "a2c_gemm_f32_partial"]
DERIVED = ["vec_epi", "Rp", "Mp", "Np", "Kp", "nmb", "nnb", "nkb", "want", "sps", "s6", "need", "sn", "e", "al16", "nch", "Kc",
           "bcap", "bands", "v4", "t128", "t32", "vA", "vB", "deep", "kps", "splitk", "slab", "vecA", "vecB", "a_kc", "b_kc",
           "base", "need9", "off9", "splits"]
CONDITIONS = {
    "launch_skinny_stream": [
        'if (M > 64 || splits < 2 || !vecA || !vecB || K % 8 || kps % 8 || N * K < (1L << 22) || a2c_env_on("A2C_NO_SKINNY_STREAM"))',
        "if (M <= 32)",
    ],
    "launch_gemm_nt_shape": [
        "if (hipMalloc(&zero, 256) != hipSuccess || hipMemset(zero, 0, 256) != hipSuccess)",
        "if (hipFuncSetAttribute((const void*)gemm_nt_kernel<S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES) != hipSuccess)",
        "if (!ready)",
    ],
    "launch_gemm_nt": [
        'if (M > nt::Big::TM || splits < 2 || !vecA || !vecB || K % 4 || kps % 4 || N * K < (1L << 22) || a2c_env_on("A2C_NO_GEMM_NT"))',
        "if (M <= nt::Skinny::TM)",
        "if (M <= 64)",
    ],
    "launch_gemm": [
        "const int vec_epi = slab == nullptr && N % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)C % 16 == 0) && (!mask || (ldmask % 4 == 0 && (uintptr_t)mask % 16 == 0)) && (!bias || (uintptr_t)bias % 16 == 0);",
        "if (false)",
        "if (M <= 96)",
    ],
    "x6_split": [
        "const long Rp = (R + 255) / 256 * 256, Kp = (K + 15) / 16 * 16, ngb = (Kp / 8 + 3) / 4;",
        "if (k_contiguous)",
    ],
    "x6_run": [
        "const long Mp = (M + 255) / 256 * 256, Np = (N + 255) / 256 * 256, Kp = (K + 15) / 16 * 16;",
        "const int nmb = (int)(Mp / 256), nnb = (int)(Np / 256), nkb = (int)(Kp / 16);",
        "int want = 1;",
        "if ((long)nmb * nnb < 192)",
        "want = (int)std::min<long>(256 / ((long)nmb * nnb), nkb / 32);",
        "if (want > splitk || !slab)",
        "want = slab ? splitk : 1;",
        "if (want < 1)",
        "want = 1;",
        "const int sps = (nkb + want - 1) / want, s6 = (nkb + sps - 1) / sps;",
        "if (s6 > 1)",
    ],
    "a2c_gemm_ws_bytes": [
        "size_t need = splitk > 1 ? (size_t)splitk * (size_t)M * (size_t)N * sizeof(float) : 0;",
        "if (M <= SN_MAX)",
        "const size_t sn = (size_t)SN_BANDS * (size_t)M * (size_t)N * sizeof(float);",
        "if (sn > need)",
        "need = sn;",
    ],
    "x9_eligible": [
        'const int e = a2c_env_int("A2C_GEMM_X9", -1);',
        "if (e == 0 || e == 1)",
        "if (e == 2)",
    ],
    "a2c_gemm_x9_ws_bytes": [
        "if (M < 1 || N < 1 || K < 1 || !x9_eligible(M, N, K))",
        "const size_t Mp = (size_t)(M + 255) / 256 * 256, Np = (size_t)(N + 255) / 256 * 256, Kp = (size_t)(K + 31) / 32 * 32;",
    ],
    "a2c_gemm_f32": [
        "if (M < 0 || N < 0 || K < 0)",
        "if (M == 0 || N == 0)",
        "if (!A || !B || !C || K == 0)",
        "const bool al16 = ((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0) && ((uintptr_t)C % 16 == 0);",
        "if (transA == 0 && transB == 1 && N <= SN_MAX && K % 4 == 0 && lda % 4 == 0 && ldb == K && !relu && !mask && !accumulate && ((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0))",
        "if (transA == 0 && transB == 0 && K <= SN_MAX && N % 4 == 0 && ldb == N && ldc % 4 == 0 && !relu && !bias && (!mask || ldmask % 4 == 0) && ((uintptr_t)B % 16 == 0) && ((uintptr_t)C % 16 == 0) && (!mask || (uintptr_t)mask % 16 == 0))",
        "if (transA == 1 && transB == 0 && M <= SN_MAX && N % 4 == 0 && N <= 8192 && ldb % 4 == 0 && ldc == N && !relu && !bias && !mask && !accumulate && ((uintptr_t)B % 16 == 0) && ((uintptr_t)C % 16 == 0) && ws && ws_bytes >= (size_t)SN_BANDS * M * N * sizeof(float))",
        "int nch = (int)((N + 1023) / 1024);",
        "while (nch <= N && !(N % nch == 0 && (N / nch) % 4 == 0 && N / nch <= 1024))",
        "if (nch <= N)",
        "const int Kc = (int)(N / nch);",
        "const int bcap = nch > 1 ? SN_BANDS / 2 : SN_BANDS;",
        "const int bands = (int)(K < bcap ? K : bcap);",
        "if (transA == 1 && transB == 0 && K <= SN_MAX && !relu && !bias && !mask)",
        "const bool v4 = N % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)B % 16 == 0) && ((uintptr_t)C % 16 == 0);",
        "if (v4)",
        "const long t128 = ((M + 127) / 128) * ((N + 127) / 128), t32 = ((M + 31) / 32) * ((N + 31) / 32);",
        "const bool vA = (lda % 4 == 0) && ((uintptr_t)A % 16 == 0), vB = (ldb % 4 == 0) && ((uintptr_t)B % 16 == 0);",
        "if (transA == 0 && K % 8 == 0 && K >= 32 && K <= 4096 && t128 < 64 && (t32 >= (K > 1024 ? 128 : 16) || (M <= 32 && t32 >= 4 && K <= 1024)) && t32 <= 4096 && vA && (transB == 0 || vB))",
        "const bool deep = K >= 1024 && t32 <= 512;",
        "if (transB && deep)",
        "if (transB)",
        "if (deep)",
        "if (splitk < 1)",
        "splitk = 1;",
        "long kps = ((K + splitk - 1) / splitk + BK - 1) / BK * BK;",
        "splitk = (int)((K + kps - 1) / kps);",
        "float* slab = nullptr;",
        "if (splitk > 1)",
        "if (!ws || ws_bytes < a2c_gemm_ws_bytes(M, N, splitk))",
        "slab = (float*)ws;",
        "const int vecA = (lda % 4 == 0) && ((uintptr_t)A % 16 == 0);",
        "const int vecB = (ldb % 4 == 0) && ((uintptr_t)B % 16 == 0);",
        "const bool a_kc = (transA == 0), b_kc = (transB != 0);",
        "const size_t base = a2c_gemm_ws_bytes(M, N, splitk), need9 = a2c_gemm_x9_ws_bytes(M, N, K);",
        "const size_t off9 = (base + 255) / 256 * 256;",
        "if (need9 && ws && ws_bytes >= off9 + need9 && x6_ready())",
        "const long Mp = (M + 255) / 256 * 256, Kp = (K + 15) / 16 * 16;",
        "if (a_kc && b_kc && launch_gemm_nt(M, N, K, A, lda, B, ldb, kps, splitk, slab, vecA, vecB, st))",
        "if (a_kc && b_kc && launch_skinny_stream(M, N, K, A, lda, B, ldb, kps, splitk, slab, vecA, vecB, st))",
        "if (a_kc && b_kc)",
        "if (a_kc && !b_kc)",
        "if (!a_kc && b_kc)",
        "if (splitk > 1)",
    ],
    "gemm_kps": [
        "if (splitk < 1)",
        "splitk = 1;",
    ],
    "a2c_gemm_splits": [
        "if (K <= 0)",
        "const long kps = gemm_kps(K, splitk);",
    ],
    "a2c_gemm_f32_partial": [
        "if (M <= 0 || N <= 0 || K <= 0 || !A || !B || !ws)",
        "const long kps = gemm_kps(K, splitk);",
        "const int splits = a2c_gemm_splits(K, splitk);",
        "if (ws_bytes < (size_t)splits * M * N * sizeof(float))",
        "const int vecA = (lda % 4 == 0) && ((uintptr_t)A % 16 == 0);",
        "const int vecB = (ldb % 4 == 0) && ((uintptr_t)B % 16 == 0);",
        "float* slab = (float*)ws;",
        "const bool a_kc = (transA == 0), b_kc = (transB != 0);",
        "if (a_kc && b_kc && launch_gemm_nt(M, N, K, A, lda, B, ldb, kps, splits, slab, vecA, vecB, st))",
        "if (a_kc && b_kc && launch_skinny_stream(M, N, K, A, lda, B, ldb, kps, splits, slab, vecA, vecB, st))",
        "if (a_kc && b_kc)",
        "if (a_kc && !b_kc)",
        "if (!a_kc && b_kc)",
    ],
}
# statements of the functions above that are neither a condition nor a declaration of a DERIVED name but that the twin repeats
RETURNS = {
    "gemm_kps": ["return ((K + splitk - 1) / splitk + BK - 1) / BK * BK;"],
    "a2c_gemm_splits": ["return (int)((K + kps - 1) / kps);"],
    "a2c_gemm_x9_ws_bytes": ["return 3 * 2 * (Mp + Np) * Kp + 256;"],
    "x9_eligible": ["if (e == 2) return M >= 256 && N >= 256 && K >= 256 && (double)M * (double)N * (double)K >= 2.5e8;",
                    "return M >= 1024 && N >= 1024 && K >= 1024 && (double)M * (double)N * (double)K >= 2e10;"],
}


# ------------------------------------------------------------------------------------------------------------ the twin
def _env_on(env, name):
    v = (env or {}).get(name)
    return v is not None and v[:1] == "1"


def _env_int(env, name, dflt):
    v = (env or {}).get(name)
    if v is None or v == "":
        return dflt
    m = re.match(r"\s*[+-]?\d+", v)          # atoi
    return int(m.group(0)) if m else 0


def ws_bytes(M, N, splitk):
    """a2c_gemm_ws_bytes"""
    need = splitk * M * N * 4 if splitk > 1 else 0
    if M <= SN_MAX:
        need = max(need, SN_BANDS * M * N * 4)
    return need


def x9_eligible(M, N, K, env=None):
    e = _env_int(env, "A2C_GEMM_X9", -1)
    if e in (0, 1):
        return False
    if e == 2:
        return M >= 256 and N >= 256 and K >= 256 and float(M) * float(N) * float(K) >= 2.5e8
    return M >= 1024 and N >= 1024 and K >= 1024 and float(M) * float(N) * float(K) >= 2e10


def x9_ws_bytes(M, N, K, env=None):
    """a2c_gemm_x9_ws_bytes"""
    if M < 1 or N < 1 or K < 1 or not x9_eligible(M, N, K, env):
        return 0
    Mp, Np, Kp = (M + 255) // 256 * 256, (N + 255) // 256 * 256, (K + 31) // 32 * 32
    return 3 * 2 * (Mp + Np) * Kp + 256


def full_ws_bytes(M, N, K, splitk, env=None):
    """what a2c_amd.ops.gemm_ws_bytes(M, N, splitk, K) returns: the slabs, then (256-aligned) the images of the x 6 path"""
    base, x9 = ws_bytes(M, N, splitk), x9_ws_bytes(M, N, K, env)
    return base if not x9 else (base + 255) // 256 * 256 + x9


def gemm_kps(K, splitk):
    splitk = max(1, splitk)
    return ((K + splitk - 1) // splitk + BK - 1) // BK * BK


def gemm_splits(K, splitk):
    """a2c_gemm_splits"""
    if K <= 0:
        return 0
    kps = gemm_kps(K, splitk)
    return (K + kps - 1) // kps


def split_tiles(K, kps, splits, tile):
    """-> (tiles of the shortest split, of the longest, columns of the last split)"""
    last = K - (splits - 1) * kps
    lens = [kps] * (splits - 1) + [last]
    t = [(n + tile - 1) // tile for n in lens]
    return min(t), max(t), last


def _x6_run(M, N, K, splitk, slab):
    Mp, Np, Kp = (M + 255) // 256 * 256, (N + 255) // 256 * 256, (K + 15) // 16 * 16
    nmb, nnb, nkb = Mp // 256, Np // 256, Kp // 16
    want = 1
    if nmb * nnb < 192:
        want = min(256 // (nmb * nnb), nkb // 32)
    if want > splitk or not slab:
        want = splitk if slab else 1
    if want < 1:
        want = 1
    sps = (nkb + want - 1) // want
    s6 = (nkb + sps - 1) // sps
    return f"gemm_x6_kernel s6={s6}" + (" +reduce" if s6 > 1 else "")


def _streams(M, N, K, kps, splits, vecA, vecB, env):
    """launch_gemm_nt, then launch_skinny_stream -> route or None"""
    big = N * K >= (1 << 22)
    if not (M > NT_TM["nt::Big"] or splits < 2 or not vecA or not vecB or K % 4 or kps % 4 or not big or _env_on(env, "A2C_NO_GEMM_NT")):
        shape = "nt::Skinny" if M <= NT_TM["nt::Skinny"] else None if M <= 64 else "nt::Big"
        if shape:
            lo, hi, last = split_tiles(K, kps, splits, NT_BKT)
            return f"gemm_nt_kernel<{shape}> splits={splits} tiles={lo}..{hi} last={last}"
    if not (M > 64 or splits < 2 or not vecA or not vecB or K % 8 or kps % 8 or not big or _env_on(env, "A2C_NO_SKINNY_STREAM")):
        lo, hi, last = split_tiles(K, kps, splits, 32)          # 8 * SK_U columns per trip of the main loop
        return f"skinny_stream_kernel<{1 if M <= 32 else 2},4> splits={splits} tiles={lo}..{hi} last={last}"
    return None


def _gemm_kernel(tA, tB, M, N, ldc, alC, bias, al_bias, mask, ldmask, al_mask, slab, vecA, vecB):
    vec_epi = (not slab and N % 4 == 0 and ldc % 4 == 0 and alC and (not mask or (ldmask % 4 == 0 and al_mask))
               and (not bias or al_bias))
    b = lambda x: "true" if x else "false"
    r = f"gemm_kernel<{b(tA == 0)},{b(tB != 0)},{b(M <= 96)}>"
    return r + (" vA" if vecA else "") + (" vB" if vecB else "") + (" vec_epi" if vec_epi else "")


def route(tA, tB, M, N, K, lda, ldb, ldc=0, *, alA=True, alB=True, alC=True, bias=False, al_bias=True, relu=False, mask=False,
          ldmask=0, al_mask=True, acc=False, splitk=1, ws=True, ws_nbytes=0, env=None, partial=False):
    """the route of a2c_gemm_f32 (partial: a2c_gemm_f32_partial).  al*: the pointer is 16-byte aligned; ws: a workspace pointer
    is passed, ws_nbytes its size"""
    if partial:
        if M <= 0 or N <= 0 or K <= 0 or not ws:
            return "ERR_ARG"
        kps, splits = gemm_kps(K, splitk), gemm_splits(K, splitk)
        if ws_nbytes < splits * M * N * 4:
            return "ERR_WORKSPACE"
        vecA, vecB = lda % 4 == 0 and alA, ldb % 4 == 0 and alB
        if tA == 0 and tB != 0:
            r = _streams(M, N, K, kps, splits, vecA, vecB, env)
            if r:
                return r
        lo, hi, last = split_tiles(K, kps, splits, BK)
        return _gemm_kernel(tA, tB, M, N, 0, True, False, True, False, 0, True, True, vecA, vecB) + f" splits={splits} last={last}"
    if M < 0 or N < 0 or K < 0:
        return "ERR_ARG"
    if M == 0 or N == 0:
        return "nothing"
    if K == 0:
        return "ERR_ARG"
    if (tA == 0 and tB == 1 and N <= SN_MAX and K % 4 == 0 and lda % 4 == 0 and ldb == K and not relu and not mask and not acc
            and alA and alB):
        return "small_n_fwd_kernel"
    if (tA == 0 and tB == 0 and K <= SN_MAX and N % 4 == 0 and ldb == N and ldc % 4 == 0 and not relu and not bias
            and (not mask or ldmask % 4 == 0) and alB and alC and (not mask or al_mask)):
        return "small_n_bwd_data_kernel"
    if (tA == 1 and tB == 0 and M <= SN_MAX and N % 4 == 0 and N <= 8192 and ldb % 4 == 0 and ldc == N and not relu and not bias
            and not mask and not acc and alB and alC and ws and ws_nbytes >= SN_BANDS * M * N * 4):
        nch = (N + 1023) // 1024
        while nch <= N and not (N % nch == 0 and (N // nch) % 4 == 0 and N // nch <= 1024):
            nch += 1
        if nch <= N:
            Kc = N // nch
            bcap = SN_BANDS // 2 if nch > 1 else SN_BANDS
            bands = K if K < bcap else bcap
            return f"small_n_bwd_weight_kernel nch={nch} bands={bands} Kc={Kc} +wreduce"
    if tA == 1 and tB == 0 and K <= SN_MAX and not relu and not bias and not mask:
        v4 = N % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and alB and alC
        return "small_k_tn_kernel<4>" if v4 else "small_k_tn_kernel<1>"
    t128, t32 = ((M + 127) // 128) * ((N + 127) // 128), ((M + 31) // 32) * ((N + 31) // 32)
    vA, vB = lda % 4 == 0 and alA, ldb % 4 == 0 and alB
    if (tA == 0 and K % 8 == 0 and K >= 32 and K <= 4096 and t128 < 64
            and (t32 >= (128 if K > 1024 else 16) or (M <= 32 and t32 >= 4 and K <= 1024)) and t32 <= 4096 and vA
            and (tB == 0 or vB)):
        deep = K >= 1024 and t32 <= 512
        return f"small_gemm_kernel<{'true' if tB else 'false'},{8 if deep else 4}>"
    splitk = max(1, splitk)
    kps = ((K + splitk - 1) // splitk + BK - 1) // BK * BK
    splitk = (K + kps - 1) // kps
    slab = False
    if splitk > 1:
        if not ws or ws_nbytes < ws_bytes(M, N, splitk):
            return "ERR_WORKSPACE"
        slab = True
    vecA, vecB = vA, vB
    base, need9 = ws_bytes(M, N, splitk), x9_ws_bytes(M, N, K, env)
    off9 = (base + 255) // 256 * 256
    if need9 and ws and ws_nbytes >= off9 + need9:
        b = lambda x: "true" if x else "false"
        return _x6_run(M, N, K, splitk, slab) + f" +splitA<{b(tA != 0)}> +splitB<{b(tB == 0)}>"
    r = _streams(M, N, K, kps, splitk, vecA, vecB, env) if (tA == 0 and tB != 0) else None
    if r is None:
        r = _gemm_kernel(tA, tB, M, N, ldc, alC, bias, al_bias, mask, ldmask, al_mask, slab, vecA, vecB)
        if slab:
            r += f" splits={splitk} last={K - (splitk - 1) * kps}"
    return r + (" +reduce" if splitk > 1 else "")


def route_x6_images(M, N, K, splitk, ws_nbytes):
    """a2c_gemm_x6_images"""
    if M < 1 or N < 1 or K < 1:
        return "ERR_ARG"
    splitk = max(1, splitk)
    if splitk > 1 and ws_nbytes < splitk * M * N * 4:
        return "ERR_WORKSPACE"
    return _x6_run(M, N, K, splitk, splitk > 1)


def family(r):
    return r.split(" ")[0]


def aux(r):
    return [t for t in r.split(" ") if t.startswith("+")]


def sg_wave_kinds(K, NW, b_kc):
    """what each wave of small_gemm_kernel<b_kc, NW> does with its K range (kq = ceil(K / 8 / NW) * 8): 'empty', 'head' (8-column
    groups one at a time only), 'head+loop', 'loop' (b_kc: trips of 32 columns, the head brings the rest to a multiple of 32;
    else trips of 16 after at most one 8-row group: wave_kinds of test_gpu_small_kernels)"""
    kq = ((K // 8 + NW - 1) // NW) * 8
    kinds = []
    for w in range(NW):
        kbeg = min(K, w * kq)
        n = min(K, kbeg + kq) - kbeg
        unit = 32 if b_kc else 16
        head, loops = (n % unit) // 8, n // unit
        kinds.append("empty" if n == 0 else "head" if not loops else "head+loop" if head else "loop")
    return kinds


# ------------------------------------------------------------------------------------------------------------ the cases
def case(id, kind, tA, tB, M, N, K, expect, *, pa=4, pb=4, pc=3, pm=4, oa=0, ob=0, oc=0, om=0, obias=0, bias=False, relu=False,
         mask=False, acc=False, splitk=1, ws="exact", env=None, also=()):
    """kind: 'gemm' (a2c_gemm_f32), 'partial' (a2c_gemm_f32_partial), 'x6img' (a2c_gemm_x6_split + a2c_gemm_x6_images).
    pa / pb / pc / pm: floats by which lda / ldb / ldc / ldmask exceed the row; o*: floats by which the pointer is off a
    16-byte boundary.  ws: 'exact' = a2c_amd.ops.gemm_ws_bytes(M, N, splitk, K) (slabs, head bands, images), 'slabs' = without
    the images, 'none', or bytes relative to 'exact' (-4: one float short).  expect: the family, or a refusal.  also:
    substrings the route name must hold."""
    return dict(id=id, kind=kind, tA=tA, tB=tB, M=M, N=N, K=K, expect=expect, pa=pa, pb=pb, pc=pc, pm=pm, oa=oa, ob=ob, oc=oc,
                om=om, obias=obias, bias=bias, relu=relu, mask=mask, acc=acc, splitk=splitk, ws=ws, env=dict(env or {}),
                also=tuple(also))


def lds(c):
    """-> lda, ldb, ldc, ldmask of a case"""
    return ((c["M"] if c["tA"] else c["K"]) + c["pa"], (c["K"] if c["tB"] else c["N"]) + c["pb"], c["N"] + c["pc"],
            c["N"] + c["pm"])


def case_ws_bytes(c):
    """bytes of workspace a case passes (0: no workspace)"""
    if c["kind"] == "partial":
        exact = gemm_splits(c["K"], c["splitk"]) * c["M"] * c["N"] * 4
    elif c["kind"] == "x6img":
        exact = c["splitk"] * c["M"] * c["N"] * 4 if c["splitk"] > 1 else 0
    else:
        exact = full_ws_bytes(c["M"], c["N"], c["K"], c["splitk"], c["env"])
    if c["ws"] == "exact":
        return exact
    if c["ws"] == "slabs":
        return ws_bytes(c["M"], c["N"], c["splitk"])
    if c["ws"] == "none":
        return 0
    return max(0, exact + int(c["ws"]))


def case_route(c):
    if c["kind"] == "x6img":
        return route_x6_images(c["M"], c["N"], c["K"], c["splitk"], case_ws_bytes(c))
    lda, ldb, ldc, ldm = lds(c)
    nb = case_ws_bytes(c)
    return route(c["tA"], c["tB"], c["M"], c["N"], c["K"], lda, ldb, ldc, alA=c["oa"] % 4 == 0, alB=c["ob"] % 4 == 0,
                 alC=c["oc"] % 4 == 0, bias=c["bias"], al_bias=c["obias"] % 4 == 0, relu=c["relu"], mask=c["mask"], ldmask=ldm,
                 al_mask=c["om"] % 4 == 0, acc=c["acc"], splitk=c["splitk"], ws=nb > 0, ws_nbytes=nb, env=c["env"],
                 partial=c["kind"] == "partial")


FULL = dict(bias=True, relu=True, mask=True, acc=True)
X6 = {"A2C_GEMM_X9": "2"}
NO_NT = {"A2C_NO_GEMM_NT": "1"}
NO_NT_NO_STREAM = {"A2C_NO_GEMM_NT": "1", "A2C_NO_SKINNY_STREAM": "1"}


def _cases():
    cs = []
    add = lambda *a, **kw: cs.append(case(*a, **kw))
    G = lambda a, b, s: f"gemm_kernel<{'true' if a == 0 else 'false'},{'true' if b else 'false'},{'true' if s else 'false'}>"

    # ---- small_n_fwd: a wave per row; K / 256 passes of a wave; the grid cap of 4096 x 4 rows forces the stride loop at 16389
    i = 0
    for M in (1, 5, 16389):
        for N in (1, 8):
            for K in (4, 252, 260, 1028):
                add(f"snf-{M}-{N}-{K}", "gemm", 0, 1, M, N, K, "small_n_fwd_kernel", pa=4, pb=0, pc=3, bias=i % 2 == 0)
                i += 1
    add("snf-K254", "gemm", 0, 1, 5, 8, 254, G(0, 1, 1), pa=2, pb=0, bias=True)                 # K % 4
    add("snf-lda", "gemm", 0, 1, 5, 8, 252, G(0, 1, 1), pa=1, pb=0, bias=True)                  # lda % 4
    add("snf-offA", "gemm", 0, 1, 5, 8, 252, G(0, 1, 1), pa=4, pb=0, oa=1, bias=True)           # A off by 4 bytes
    add("snf-ldb", "gemm", 0, 1, 5, 8, 252, G(0, 1, 1), pa=4, pb=4, bias=True)                  # ldb != K
    add("snf-relu", "gemm", 0, 1, 5, 8, 252, G(0, 1, 1), pa=4, pb=0, bias=True, relu=True)
    add("snf-N9", "gemm", 0, 1, 5, 9, 252, G(0, 1, 1), pa=4, pb=0, bias=True)

    # ---- small_n_bwd_data: dx[m, :N] = dy[m, :K] W[:K, :N]
    i = 0
    for K in (1, 3, 8):
        for N in (4, 260):
            for M in (1, 300):
                add(f"snd-{M}-{N}-{K}", "gemm", 0, 0, M, N, K, "small_n_bwd_data_kernel", pa=1, pb=0, pc=4, mask=i % 2 == 0,
                    acc=i % 4 < 2)
                i += 1
    add("snd-N258", "gemm", 0, 0, 300, 258, 3, G(0, 0, 0), pa=1, pb=0, pc=2, mask=True, acc=True)
    add("snd-offmask", "gemm", 0, 0, 300, 260, 3, G(0, 0, 0), pa=1, pb=0, pc=4, mask=True, om=1)
    add("snd-ldc", "gemm", 0, 0, 300, 260, 3, G(0, 0, 0), pa=1, pb=0, pc=3, mask=True)
    add("snd-K9", "gemm", 0, 0, 300, 260, 9, G(0, 0, 0), pa=1, pb=0, pc=4, mask=True)

    # ---- small_n_bwd_weight: dW[heads M][N] = dy[rows K][M]^T x[rows K][N]; Kc / 4 = 1, 3, 100, 200, 256; nch = 1, 2, 1031, 8
    i = 0
    for N in (4, 12, 400, 800, 1024, 2000, 4124, 8192):
        for K in (1, 7, 9, 511, 513, 1000, 4099):
            add(f"snw-{(1, 3, 8)[i % 3]}-{N}-{K}", "gemm", 1, 0, (1, 3, 8)[i % 3], N, K, "small_n_bwd_weight_kernel", pa=1, pb=4,
                pc=0)
            i += 1
    for M in (1, 3, 8):          # every head count at the wave-uniform readlane branch with partly live waves (Kc / 4 = 200)
        add(f"snw-heads-{M}", "gemm", 1, 0, M, 800, 1000, "small_n_bwd_weight_kernel", pa=1, pb=4, pc=0, also=["Kc=800"])
    add("snw-ws-short", "gemm", 1, 0, 3, 800, 1000, G(1, 0, 1), pa=1, pb=4, pc=0, ws=-4)
    add("snw-N8192", "gemm", 1, 0, 3, 8192, 513, "small_n_bwd_weight_kernel", pa=1, pb=4, pc=0)
    add("snw-N8196", "gemm", 1, 0, 3, 8196, 513, G(1, 0, 1), pa=1, pb=4, pc=0)
    add("snw-ldc", "gemm", 1, 0, 3, 800, 1000, G(1, 0, 1), pa=1, pb=4, pc=4)
    add("snw-M9", "gemm", 1, 0, 9, 800, 1000, G(1, 0, 1), pa=1, pb=4, pc=0)

    # ---- small_k_tn<4> / <1>: rank-K outer-product sum
    i = 0
    for K in (1, 8):
        for N in (8, 10):
            for M in (70, 9):           # (M <= 8 with N % 4 == 0 and a workspace is the weight gradient above; M = 1 below)
                add(f"sktn-{M}-{N}-{K}", "gemm", 1, 0, M, N, K, f"small_k_tn_kernel<{4 if N % 4 == 0 else 1}>", pa=1, pb=4,
                    pc=2 if N % 4 else 4, acc=i % 2 == 0, ws="none")
                i += 1
    add("sktn-1-8-8", "gemm", 1, 0, 1, 8, 8, "small_k_tn_kernel<4>", pa=1, pb=4, pc=4, ws="none")
    add("sktn-1-10-1", "gemm", 1, 0, 1, 10, 1, "small_k_tn_kernel<1>", pa=1, pb=4, pc=2, acc=True, ws="none")
    add("sktn-offC", "gemm", 1, 0, 70, 8, 8, "small_k_tn_kernel<1>", pa=1, pb=4, pc=4, oc=1, acc=True, ws="none")
    add("sktn-K9", "gemm", 1, 0, 70, 8, 9, G(1, 0, 1), pa=1, pb=4, pc=4, acc=True, ws="none")

    # ---- small_gemm_kernel: four instantiations x K of every kind of wave x (M, N) x plain / full epilogue
    i = 0
    for tB in (1, 0):
        for K in (32, 40, 72, 264, 1016, 1024, 1032, 4096):
            if K <= 1024:
                mns = [(33, 225), (32, 97), (128, 1024), (100, 1300)]
            else:       # K > 1024 wants t32 >= 128
                mns = [(128, 1024), (100, 1300)] if K == 1032 else [(5, 4096), (33, 2040)]
            for M, N in mns:
                nw = 8 if K >= 1024 else 4
                add(f"sg-{tB}-{M}-{N}-{K}", "gemm", 0, tB, M, N, K, f"small_gemm_kernel<{'true' if tB else 'false'},{nw}>",
                    **(FULL if i % 2 == 0 else {}), pc=(3, 4, 0)[i % 3])
                i += 1
    add("sg-K4104", "gemm", 0, 1, 33, 2040, 4104, G(0, 1, 1), **FULL)
    add("sg-K24", "gemm", 0, 1, 128, 1024, 24, G(0, 1, 0), **FULL)
    add("sg-K36", "gemm", 0, 1, 128, 1024, 36, G(0, 1, 0), **FULL)                              # K % 8
    add("sg-33-95", "gemm", 0, 1, 33, 95, 72, G(0, 1, 1), **FULL)                                  # t32 = 6 and M > 32
    add("sg-lda", "gemm", 0, 1, 32, 97, 72, G(0, 1, 1), pa=1, **FULL)
    add("sg-offA", "gemm", 0, 0, 32, 97, 72, G(0, 0, 1), oa=1, **FULL)
    add("sg-ldb-nt", "gemm", 0, 1, 32, 97, 72, G(0, 1, 1), pb=2, **FULL)
    add("sg-ldb-nn", "gemm", 0, 0, 32, 97, 72, "small_gemm_kernel<false,4>", pb=1, ob=1, **FULL)   # (B n-contiguous: scalar loads)
    add("sg-tA", "gemm", 1, 1, 32, 97, 72, G(1, 1, 1), **FULL)
    # thresholds: t32 15 / 16, 3 / 4 (M <= 32), 127 / 128 (K > 1024), t128 63 / 64, M 32 / 33 of the (M <= 32, t32 >= 4) clause
    add("sg-t32-15", "gemm", 0, 1, 96, 160, 72, G(0, 1, 1), **FULL)
    add("sg-t32-16", "gemm", 0, 1, 97, 128, 72, "small_gemm_kernel<true,4>", **FULL)
    add("sg-t32-3", "gemm", 0, 1, 32, 96, 72, G(0, 1, 1), **FULL)
    add("sg-t32-4", "gemm", 0, 1, 32, 97, 72, "small_gemm_kernel<true,4>", **FULL)
    add("sg-M33-t32-8", "gemm", 0, 1, 33, 97, 72, G(0, 1, 1), **FULL)
    add("sg-t32-127", "gemm", 0, 1, 32, 4064, 1032, G(0, 1, 1), **FULL)
    add("sg-t32-128", "gemm", 0, 1, 32, 4065, 1032, "small_gemm_kernel<true,8>", **FULL)
    add("sg-t128-63", "gemm", 0, 0, 100, 8064, 32, "small_gemm_kernel<false,4>", **FULL)
    add("sg-t128-64", "gemm", 0, 0, 100, 8065, 32, G(0, 0, 0), **FULL)
    add("sg-K1024-t32-4", "gemm", 0, 0, 32, 97, 1024, "small_gemm_kernel<false,8>")
    add("sg-K1032-t32-4", "gemm", 0, 0, 32, 97, 1032, G(0, 0, 1))

    # ---- gemm_kernel: four orientations x M 33 / 96 / 97 x N 127 / 128 / 129 x K 1 / 15 / 16 / 17 / 100, vA / vB / vec_epi
    # on and off by leading dimension and by a 4-byte pointer offset, the epilogue in the kernel and in splitk_reduce_kernel
    i = 0
    for tA, tB in ((0, 1), (0, 0), (1, 0), (1, 1)):
        for M in (33, 96, 97):
            for N in (127, 128, 129):
                for K in (1, 15, 16, 17, 100):
                    v = i % 6
                    kw = dict(pa=(4, 1, 4, 4, 3, 4)[v], pb=(4, 4, 2, 4, 4, 1)[v], pc=(4, 4, 3, 4, 4, 4)[v],
                              oa=(0, 0, 0, 1, 0, 0)[v], ob=(0, 0, 1, 0, 0, 0)[v], oc=(0, 0, 0, 0, 1, 0)[v],
                              om=(0, 0, 0, 0, 0, 1)[v], obias=(0, 1, 0, 0, 0, 0)[v], pm=(4, 4, 4, 1, 4, 4)[v])
                    sk = (1, 1, 2, 1, 7)[(i // 6 + i) % 5] if K > 16 else 1
                    add(f"gk-{tA}{tB}-{M}-{N}-{K}-v{v}-s{sk}", "gemm", tA, tB, M, N, K, G(tA, tB, M <= 96),
                        **(FULL if i % 3 or K == 1 else dict(bias=i % 2 == 0)), splitk=sk, **kw)      # (K = 1 without an epilogue: small_k_tn)
                    i += 1
    for tA, tB in ((0, 1), (0, 0), (1, 0), (1, 1)):              # the last split one column long: K = 6 * 16 + 1
        add(f"gk-{tA}{tB}-last1", "gemm", tA, tB, 97, 129, 97, G(tA, tB, 0), splitk=7, **FULL, also=["splits=7", "last=1"])
        add(f"gkp-{tA}{tB}-last1", "partial", tA, tB, 33, 129, 97, G(tA, tB, 1), splitk=7, also=["splits=7", "last=1"])
    for tA, tB in ((0, 1), (0, 0), (1, 0), (1, 1)):              # float4 epilogue, full and plain, both SKINNY settings
        for M in (33, 97):
            add(f"gk-{tA}{tB}-{M}-vec", "gemm", tA, tB, M, 128, 100, G(tA, tB, M <= 96), pa=3 if tA else 4, pc=4, **FULL,
                also=["vA", "vB", "vec_epi"])
            add(f"gk-{tA}{tB}-{M}-vec-plain", "gemm", tA, tB, M, 132, 17, G(tA, tB, M <= 96), pc=0, also=["vec_epi"])
    add("gk-M96", "gemm", 0, 1, 96, 128, 100, G(0, 1, 1), **FULL)
    add("gk-M97", "gemm", 0, 1, 97, 128, 100, G(0, 1, 0), **FULL)
    add("gk-ws-short", "gemm", 0, 1, 97, 129, 100, "ERR_WORKSPACE", splitk=3, ws=-4, **FULL)
    add("gk-ws-none", "gemm", 0, 1, 97, 129, 100, "ERR_WORKSPACE", splitk=3, ws="none", **FULL)
    add("gk-K0", "gemm", 0, 1, 5, 7, 0, "ERR_ARG")
    add("gk-M0", "gemm", 0, 1, 0, 7, 16, "nothing")
    add("gk-N0", "gemm", 0, 1, 5, 0, 16, "nothing")

    # ---- gemm_nt<Skinny> (M <= 32, DEPTH 4: LOOK = 3) and gemm_nt<Big> (64 < M <= 256, DEPTH 3: LOOK = 2): N * K just at or above
    # 2^22; splits of 1, 2, LOOK, LOOK + 1 and about ten 32-column tiles; last splits of 4, 28 and 32 columns
    def ring(tag, M, N, K, sks, fam, env=None, kinds=("gemm", "partial")):
        for j, sk in enumerate(sks):
            kind = kinds[j % len(kinds)]
            add(f"{tag}-{M}-{N}-{K}-s{sk}" + ("-p" if kind == "partial" else ""), kind, 0, 1, M, N, K, fam, pa=4, pb=(0, 4)[j % 2],
                splitk=sk, env=env, **({} if kind == "partial" else FULL if j % 2 == 0 else dict(bias=True, relu=True)))
    ring("nts", 32, 128, 32768, (1024, 512, 342, 256, 103), "gemm_nt_kernel<nt::Skinny>")       # 1, 2, 3, 4, 10 tiles, last 32
    ring("nts", 7, 300, 16388, (257, 513, 129), "gemm_nt_kernel<nt::Skinny>")                   # last split 4 columns
    ring("nts", 1, 130, 32796, (1025, 64), "gemm_nt_kernel<nt::Skinny>")                        # last split 28 columns
    ring("ntb", 65, 130, 32772, (64, 1025, 513, 342, 257), "gemm_nt_kernel<nt::Big>")           # last 4 columns; 1, 2, 3, 4 tiles
    ring("ntb", 71, 128, 32768, (1024, 512, 342, 103), "gemm_nt_kernel<nt::Big>")               # 1, 2, 3, 10 tiles, last 32
    ring("ntb", 66, 300, 14012, (438, 40), "gemm_nt_kernel<nt::Big>")                           # last split 28 columns
    add("nt-NK-below", "gemm", 0, 1, 32, 128, 32764, G(0, 1, 1), pa=4, pb=0, splitk=64, **FULL)  # N K = 2^22 - 4 N
    add("nt-splitk1", "gemm", 0, 1, 32, 128, 32768, G(0, 1, 1), splitk=1, **FULL)
    add("nt-K%4", "gemm", 0, 1, 32, 128, 32770, G(0, 1, 1), pa=2, pb=2, splitk=64, **FULL)
    add("nt-lda", "gemm", 0, 1, 32, 128, 32768, G(0, 1, 1), pa=1, splitk=64, **FULL)
    add("nt-offB", "gemm", 0, 1, 65, 130, 32772, G(0, 1, 1), ob=1, splitk=64, **FULL)

    # ---- skinny_stream<2> (32 < M <= 64) and skinny_stream<1> (M <= 32, only with A2C_NO_GEMM_NT=1): the same ladder, K % 8 == 0
    ring("ss2", 64, 128, 32768, (1024, 512, 342, 256, 103), "skinny_stream_kernel<2,4>")
    ring("ss2", 33, 300, 13992, (438, 219, 40), "skinny_stream_kernel<2,4>")                    # last split 8 / 40 / 8 columns
    ring("ss1", 32, 128, 32768, (1024, 512, 342, 103), "skinny_stream_kernel<1,4>", env=NO_NT)
    ring("ss1", 7, 300, 13992, (438, 40), "skinny_stream_kernel<1,4>", env=NO_NT)
    add("ss-K%8", "gemm", 0, 1, 40, 300, 13996, G(0, 1, 1), splitk=40, **FULL)                  # K % 8 = 4
    add("ss-off", "gemm", 0, 1, 64, 128, 32768, G(0, 1, 1), splitk=64, env={"A2C_NO_SKINNY_STREAM": "1"}, **FULL)
    add("ss1-off", "gemm", 0, 1, 32, 128, 32768, G(0, 1, 1), splitk=64, env=NO_NT_NO_STREAM, **FULL)
    add("M64", "gemm", 0, 1, 64, 130, 32772, G(0, 1, 1), splitk=64, **FULL)                     # K % 8 = 4 at M = 64: neither
    add("M33", "gemm", 0, 1, 33, 128, 32768, "skinny_stream_kernel<2,4>", splitk=64, **FULL)
    add("M65", "gemm", 0, 1, 65, 128, 32768, "gemm_nt_kernel<nt::Big>", splitk=64, **FULL)
    add("M33-nt-off", "gemm", 0, 1, 33, 128, 32768, "skinny_stream_kernel<2,4>", splitk=64, env=NO_NT, **FULL)

    # ---- x 6 through a2c_gemm_f32 with A2C_GEMM_X9=2, and from prebuilt images
    for j, (tA, tB) in enumerate(((0, 1), (0, 0), (1, 0), (1, 1))):
        add(f"x6-{tA}{tB}-256", "gemm", tA, tB, 256, 1024, 1028, "gemm_x6_kernel", splitk=(1, 4)[j % 2], env=X6, **FULL)
        add(f"x6-{tA}{tB}-257", "gemm", tA, tB, 257, 300, 3303 if j % 2 else 3300, "gemm_x6_kernel", splitk=(4, 1)[j % 2],
            pa=(4, 1)[j % 2], pb=(3, 4)[j % 2], env=X6, **FULL)
    add("x6-noimg", "gemm", 0, 1, 257, 300, 3300, G(0, 1, 0), splitk=4, ws="slabs", env=X6, **FULL)
    add("x6-noimg-short", "gemm", 0, 1, 257, 300, 3300, G(0, 1, 0), splitk=4, ws=-4, env=X6, **FULL)
    add("x6-below", "gemm", 0, 1, 256, 300, 3255, G(0, 1, 0), env=X6, **FULL)                   # M N K = 2.49984e8
    add("x6-above", "gemm", 0, 1, 256, 300, 3256, "gemm_x6_kernel", env=X6, **FULL)             # 2.50061e8
    add("x6-M255", "gemm", 0, 1, 255, 1024, 1028, G(0, 1, 0), env=X6, **FULL)
    add("x6-small-first", "gemm", 0, 1, 256, 1024, 1024, "small_gemm_kernel<true,8>", env=X6, **FULL)   # K % 8 == 0: the small product wins
    add("x6-10-1024", "gemm", 1, 0, 256, 1024, 1024, "gemm_x6_kernel", splitk=4, env=X6, **FULL)
    add("x6-default", "gemm", 0, 1, 257, 300, 3300, G(0, 1, 0), **FULL)                         # without the switch: fp32
    add("x6-img-1", "x6img", 0, 1, 257, 300, 3303, "gemm_x6_kernel", splitk=1, bias=True, relu=True)
    add("x6-img-4", "x6img", 1, 0, 256, 520, 1100, "gemm_x6_kernel", splitk=4, **FULL)
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}

# both sides of a threshold: (what, the case below / on one side, the case on the other)
THRESHOLDS = [
    ("M 96 / 97 (SKINNY)", "gk-M96", "gk-M97"),
    ("M 32 / 33 (nt<Skinny> / stream<2>)", "nts-32-128-32768-s1024", "M33"),
    ("M 32 / 33 (small_gemm, t32 >= 4)", "sg-t32-4", "sg-M33-t32-8"),
    ("M 64 / 65 (stream<2> / nt<Big>)", "ss2-64-128-32768-s1024", "M65"),
    ("K 1016 / 1024 (deep)", "sg-1-128-1024-1016", "sg-1-128-1024-1024"),
    ("K 1024 / 1032 (t32 floor 4 -> 128)", "sg-K1024-t32-4", "sg-K1032-t32-4"),
    ("K 4096 / 4104", "sg-1-33-2040-4096", "sg-K4104"),
    ("t32 15 / 16", "sg-t32-15", "sg-t32-16"),
    ("t32 3 / 4", "sg-t32-3", "sg-t32-4"),
    ("t32 127 / 128", "sg-t32-127", "sg-t32-128"),
    ("t128 63 / 64", "sg-t128-63", "sg-t128-64"),
    ("N K against 2^22", "nt-NK-below", "nts-32-128-32768-s103"),
    ("N 8192 / 8196 (weight gradient)", "snw-N8192", "snw-N8196"),
    ("K 8 / 9 (small_k_tn)", "sktn-70-8-8", "sktn-K9"),
    ("K 8 / 9 (small_n_bwd_data)", "snd-300-260-8", "snd-K9"),
    ("N 8 / 9 (small_n_fwd)", "snf-5-8-252", "snf-N9"),
    ("M 8 / 9 (weight gradient)", "snw-heads-8", "snw-M9"),
    ("workspace one float short (weight gradient)", "snw-heads-3", "snw-ws-short"),
    ("workspace one float short (split-K)", "gk-01-last1", "gk-ws-short"),
    ("workspace without the images (x 6)", "x6-01-257", "x6-noimg"),
    ("M N K against 2.5e8 (x 6)", "x6-below", "x6-above"),
    ("M 255 / 256 (x 6)", "x6-M255", "x6-01-256"),
]


# ------------------------------------------------------------------------------------------------------------ the tests
def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _function_body(src, name):
    """text between the braces of the definition of `name` (the first `name(...) {` at file or namespace level)"""
    for m in re.finditer(r"\b%s\s*\(" % re.escape(name), src):
        i = _close(src, m.end() - 1, "(", ")")
        j = i
        while j < len(src) and src[j] in " \t\r\n":
            j += 1
        if j < len(src) and src[j] == "{":
            return src[j + 1:_close(src, j, "{", "}") - 1]
    raise AssertionError(f"{name}: no definition in gemm.hip")


def _close(s, i, op, cl):
    """s[i] == op -> index just behind the matching cl"""
    assert s[i] == op
    d = 0
    for j in range(i, len(s)):
        d += s[j] == op
        d -= s[j] == cl
        if d == 0:
            return j + 1
    raise AssertionError("unbalanced")


def _norm(t):
    return re.sub(r"\s+", " ", t).strip()


def _conditions(body):
    """the `if (...)` / `while (...)` heads and the statements that declare or assign a DERIVED name, in source order"""
    found = []
    for m in re.finditer(r"\b(if|while)\s*\(", body):
        e = _close(body, m.end() - 1, "(", ")")
        found.append((m.start(), _norm(m.group(1) + " " + body[m.end() - 1:e])))
    names = "|".join(DERIVED)
    stmt = re.compile(r"(?:(?<=[;{})])|^)\s*((?:(?:const|static)\s+)*(?:(?:bool|int|long|size_t|float\*)\s+)?(?:%s)\s*=[^;]*;)" % names, re.M)
    for m in stmt.finditer(body):
        found.append((m.start(1), _norm(m.group(1))))
    found.sort()
    return [t for _, t in found]


def _launched(src):
    """kernel instantiations launched from the dispatching functions, template parameters of the launchers expanded"""
    inst = set()
    calls = {"launch_gemm": set(re.findall(r"\blaunch_gemm<([^>]*)>\(", src)),
             "launch_gemm_nt_shape": set(re.findall(r"\blaunch_gemm_nt_shape<([^>]*)>\(", src))}
    for fn in DISPATCH_FUNCTIONS:
        body = _function_body(src, fn)
        for m in re.finditer(r"hipLaunchKernelGGL\(\s*(\(?[A-Za-z_0-9:]+(?:<[^>]*>)?\)?)\s*,", body):
            k = m.group(1).strip("()").replace(" ", "")
            if fn == "launch_gemm":
                for targs in calls["launch_gemm"]:
                    a, b = [t.strip() for t in targs.split(",")]
                    inst.add(k.replace("A_KC", a).replace("B_KC", b))
            elif fn == "launch_gemm_nt_shape":
                for targs in calls["launch_gemm_nt_shape"]:
                    inst.add(k.replace("<S>", f"<{targs.strip()}>"))
            else:
                inst.add(k)
    return inst


def test_every_launch_and_condition_of_the_dispatcher_has_its_twin():
    """gemm.hip, read as text: the kernels its dispatching functions launch are exactly ROUTES and AUX, and the conditions and
    derived quantities of those functions are, word for word, CONDITIONS"""
    src = _strip_comments(open(HIP).read())
    launched = _launched(src)
    known = set(ROUTES) | set(AUX.values())
    assert launched - known == set(), f"launched from the dispatcher without a route: {sorted(launched - known)}"
    assert known - launched == set(), f"routes no launch of the dispatcher reaches: {sorted(known - launched)}"
    assert set(CONDITIONS) == set(DISPATCH_FUNCTIONS)
    for fn in DISPATCH_FUNCTIONS:
        body = _function_body(src, fn)
        got = _conditions(body)
        assert got == CONDITIONS[fn], (fn, [(a, b) for a, b in zip(got, CONDITIONS[fn]) if a != b][:1] or (len(got), len(CONDITIONS[fn])),
                                       got)
        for text in RETURNS.get(fn, []):
            assert text in _norm(body), (fn, text)
    consts = dict(re.findall(r"constexpr int (SN_MAX|SN_BANDS) = (\d+);", src))
    assert consts == {"SN_MAX": str(SN_MAX), "SN_BANDS": str(SN_BANDS)}
    assert re.search(r"constexpr int BM = 128, BN = 128, BK = %d;" % BK, src)
    assert re.search(r"constexpr int BKT = %d, NW = 8, NL = 4;" % NT_BKT, src)
    assert re.search(r"using Big = Shape<%d, 128, 4, %d>;" % (NT_TM["nt::Big"], NT_LOOK["nt::Big"] + 1), src)
    assert re.search(r"using Skinny = Shape<%d, 256, 1, %d>;" % (NT_TM["nt::Skinny"], NT_LOOK["nt::Skinny"] + 1), src)
    assert re.search(r"skinny_stream_kernel<1, 4>", src) and re.search(r"for \(; k \+ 8 \* SK_U <= kend; k \+= 8 \* SK_U\)", src)


def test_every_case_lands_on_the_route_it_names_and_every_route_is_reached():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))
    reached, reached_aux = set(), set()
    for c in CASES:
        r = case_route(c)
        assert family(r) == c["expect"], (c["id"], r, c["expect"])
        for s in c["also"]:
            assert s in r.split(" "), (c["id"], r, s)
        assert family(r) in ROUTES or family(r) in REFUSALS, r
        reached.add(family(r))
        reached_aux.update(aux(r))
    assert set(ROUTES) - reached == set(), sorted(set(ROUTES) - reached)
    assert set(AUX) - reached_aux == set(), sorted(set(AUX) - reached_aux)
    assert REFUSALS <= reached
    # epilogue through gemm_kernel itself (scalar and float4) and through splitk_reduce_kernel, in all four orientations
    for fam in (f for f in ROUTES if f.startswith("gemm_kernel<")):
        rs = [case_route(c) for c in CASES if c["expect"] == fam and c["kind"] == "gemm"]
        assert any("+reduce" in r for r in rs) and any("vec_epi" in r for r in rs), fam
        assert any("+reduce" not in r and "vec_epi" not in r for r in rs), fam
        for flag in ("vA", "vB"):
            assert any(flag in r.split(" ") for r in rs) and any(flag not in r.split(" ") for r in rs), (fam, flag)


def test_both_sides_of_every_threshold_are_cases_on_different_routes():
    for what, lo, hi in THRESHOLDS:
        assert lo in BY_ID and hi in BY_ID, (what, lo, hi)
        a, b = case_route(BY_ID[lo]), case_route(BY_ID[hi])
        assert family(a) != family(b), (what, a, b)


def _ring_attrs(r):
    d = dict(t.split("=") for t in r.split(" ") if "=" in t)
    lo, hi = d["tiles"].split("..")
    return int(d["splits"]), int(lo), int(hi), int(d["last"])


def test_ring_kernels_run_at_every_short_ring_and_every_kind_of_last_split():
    """gemm_nt's prologue issues min(LOOK, tiles) DMA tiles and wait_for counts what stays in flight: 1, 2, LOOK and LOOK + 1
    tiles per split take different paths through both, ten is the steady state; the last split is 4, 28 and 32 columns long
    (a tile with one valid 16-byte piece, with seven, a full one)"""
    for shape in ("nt::Skinny", "nt::Big"):
        look = NT_LOOK[shape]
        longest, shortest, lasts = set(), set(), set()
        for c in CASES:
            r = case_route(c)
            if family(r) == f"gemm_nt_kernel<{shape}>":
                _, lo, hi, last = _ring_attrs(r)
                longest.add(hi), shortest.add(lo), lasts.add(last % NT_BKT or NT_BKT)
        assert {1, 2, look, look + 1} <= longest and any(9 <= t <= 11 for t in longest), (shape, sorted(longest))
        assert 1 in shortest, (shape, sorted(shortest))
        assert {4, 28, 32} <= lasts, (shape, sorted(lasts))
    for mb in (1, 2):
        longest, lasts = set(), set()
        for c in CASES:
            r = case_route(c)
            if family(r) == f"skinny_stream_kernel<{mb},4>":
                _, lo, hi, last = _ring_attrs(r)
                longest.add(hi), lasts.add(last % 32 or 32)
        assert {1, 2} <= longest and any(9 <= t <= 11 for t in longest), (mb, sorted(longest))
        assert {8, 32} <= lasts, (mb, sorted(lasts))          # (the tail loop of 8 columns alone, and none of it)


def test_small_gemm_cases_reach_every_kind_of_wave_and_the_weight_gradient_every_thread_map():
    from test_gpu_small_kernels import wave_kinds
    for tB in (1, 0):
        for NW in (4, 8):
            fam = f"small_gemm_kernel<{'true' if tB else 'false'},{NW}>"
            seen = set()
            for c in CASES:
                if c["expect"] == fam:
                    seen.update(sg_wave_kinds(c["K"], NW, bool(tB)))
            # eight waves run at K >= 1024 only: 16 groups of 8 columns per wave at least, so no wave is empty or head-only
            assert seen == ({"empty", "head", "head+loop", "loop"} if NW == 4 else {"head+loop", "loop"}), (fam, seen)
    for K in (32, 40, 72, 264, 1016, 1024, 1032, 4096):          # the n-contiguous form is the GRU cell's loop
        for NW in (4, 8):
            assert sg_wave_kinds(K, NW, False) == wave_kinds(K, NW, True), (K, NW)
    assert sg_wave_kinds(32, 4, True) == ["head"] * 4 and sg_wave_kinds(40, 4, True) == ["head"] * 2 + ["head", "empty"]
    assert sg_wave_kinds(1032, 8, True) == ["head+loop"] * 7 + ["head+loop"] and sg_wave_kinds(4096, 8, True) == ["loop"] * 8
    # small_n_bwd_weight: Kc / 4 (thread map), nch (column chunks), rows against RU = 8 and against the bands
    got = set()
    for c in CASES:
        r = case_route(c)
        if family(r) == "small_n_bwd_weight_kernel":
            d = dict(t.split("=") for t in r.split(" ") if "=" in t)
            got.add((int(d["Kc"]) // 4, int(d["nch"])))
            assert int(d["bands"]) == min(c["K"], 256 if int(d["nch"]) > 1 else 512)
    assert {(1, 1), (3, 1), (100, 1), (200, 1), (256, 1), (250, 2), (1, 1031), (256, 8)} <= got, sorted(got)


def test_cases_stay_small():
    for c in CASES:
        assert c["M"] * c["N"] * c["K"] < 3e8, c["id"]
        assert case_ws_bytes(c) < 256e6, (c["id"], case_ws_bytes(c))
    print(f"\n{len(CASES)} cases, sum of M N K = {sum(c['M'] * c['N'] * c['K'] for c in CASES):.3g}")


def test_twin_of_the_workspace_sizes():
    assert ws_bytes(3, 800, 1) == 512 * 3 * 800 * 4 and ws_bytes(9, 800, 1) == 0 and ws_bytes(9, 800, 3) == 3 * 9 * 800 * 4
    assert ws_bytes(8, 100, 1000) == 1000 * 8 * 100 * 4
    assert x9_ws_bytes(257, 300, 3300) == 0 and x9_ws_bytes(257, 300, 3300, X6) == 6 * (512 + 512) * 3328 + 256
    assert x9_ws_bytes(257, 300, 3300, {"A2C_GEMM_X9": "1"}) == 0 and x9_ws_bytes(1024, 1024, 19074) == 6 * 2048 * 19104 + 256
    assert x9_ws_bytes(1024, 1024, 19073) == 0
    assert gemm_splits(97, 7) == 7 and gemm_kps(97, 7) == 16 and gemm_splits(100, 32) == 7 and gemm_splits(0, 3) == 0


# the shape lists of the older GEMM tests (tests/test_gpu_kernels.py, tests/test_gpu_small_kernels.py), as they call a2c_gemm_f32
def _older_tests():
    rows = []
    shapes = [(1, 1, 1), (5, 3, 7), (128, 128, 16), (130, 257, 100), (256, 256, 2592), (300, 4, 256), (3, 256, 1000), (200, 300, 256),
              (33, 95, 64), (256, 768, 288), (32, 512, 2000), (70, 130, 40)]
    for tA, tB in ((0, 1), (0, 0), (1, 0), (1, 1)):
        for M, N, K in shapes:
            lda, ldb = (M if tA else K), (K if tB else N)
            rows.append((f"test_gemm_f32[{tA}{tB}-{M}-{N}-{K}] plain", route(tA, tB, M, N, K, lda, ldb, N, ws=False)))
            for sk in (1, 3):
                nb = ws_bytes(M, N, sk)
                rows.append((f"test_gemm_f32[{tA}{tB}-{M}-{N}-{K}] epilogue sk={sk}",
                             route(tA, tB, M, N, K, lda, ldb, N, bias=True, relu=True, mask=True, ldmask=N, acc=True, splitk=sk,
                                   ws=True, ws_nbytes=max(4, nb))))
    for M, N, K, sk in [(32, 2000, 28224, 32), (8, 1030, 4104, 5), (33, 1500, 4096, 7), (64, 2048, 2048, 2)]:
        for env in (None, {"A2C_NO_SKINNY_STREAM": "1"}):
            rows.append((f"test_gemm_skinny_stream[{M}-{N}-{K}-{sk}]" + (" A2C_NO_SKINNY_STREAM=1" if env else ""),
                         route(0, 1, M, N, K, K, K, N, bias=True, relu=True, splitk=sk, ws=True, ws_nbytes=max(4, ws_bytes(M, N, sk)),
                               env=env)))
    for M in (7, 32, 65, 100, 256):
        for env in (None, NO_NT):
            rows.append((f"test_gemm_rollout_batch_forward[{M}]" + (" A2C_NO_GEMM_NT=1" if env else ""),
                         route(0, 1, M, 300, 14008, 14012, 14008, 300, bias=True, relu=True, splitk=6, ws=True,
                               ws_nbytes=ws_bytes(M, 300, 6), env=env)))
    rows.append(("test_gemm_skinny_head_paths fwd", route(0, 1, 1000, 4, 256, 256, 256, 4, bias=True, ws=False)))
    rows.append(("test_gemm_skinny_head_paths bwd_data", route(0, 0, 1000, 256, 3, 4, 256, 256, mask=True, ldmask=256, ws=False)))
    rows.append(("test_gemm_skinny_head_paths bwd_weight", route(1, 0, 4, 256, 1000, 4, 256, 256, splitk=2, ws=True,
                                                                 ws_nbytes=ws_bytes(4, 256, 2))))
    rows.append(("test_gemm_strided_views_and_colsum", route(0, 1, 70, 5, 33, 36, 33, 7, alC=False, ws=False)))
    for tA, tB, M, N, K in [(0, 1, 1280, 1100, 2000), (0, 0, 1152, 900, 1000), (1, 0, 520, 1030, 777)]:
        lda, ldb = (M if tA else K), (K if tB else N)
        rows.append((f"test_gemm_bf16_x9_path[{tA}{tB}-{M}-{N}-{K}]",
                     route(tA, tB, M, N, K, lda, ldb, N, bias=True, relu=True, mask=True, ldmask=N, ws=True,
                           ws_nbytes=full_ws_bytes(M, N, K, 1, X6), env=X6)))
    for tA, tB in ((0, 1), (0, 0), (1, 0), (1, 1)):
        for M, N, K in [(5, 3, 7), (130, 257, 100), (8, 1030, 4104)]:
            for sk in (1, 4, 32):
                lda, ldb = (M if tA else K), (K if tB else N)
                rows.append((f"test_gemm_partial[{tA}{tB}-{M}-{N}-{K}-{sk}]",
                             route(tA, tB, M, N, K, lda, ldb, splitk=sk, ws=True, ws_nbytes=(gemm_splits(K, sk) * M * N + 64) * 4,
                                   partial=True)))
    return rows


def test_routes_of_the_older_gemm_tests():
    """which kernel serves which case of the older tests today (printed with -s), and what they leave out: the reason for
    tests/test_gpu_gemm_routes.py"""
    rows = _older_tests()
    print()
    for name, r in rows:
        print(f"  {name:64s} {r}")
    fam = lambda prefix: {family(r) for n, r in rows if n.startswith(prefix)}
    f32 = fam("test_gemm_f32")
    for never in ("small_gemm_kernel<true,8>", "small_gemm_kernel<false,8>", "small_k_tn_kernel<4>", "small_n_bwd_data_kernel",
                  "small_n_bwd_weight_kernel", "gemm_nt_kernel<nt::Skinny>", "gemm_nt_kernel<nt::Big>", "skinny_stream_kernel<1,4>",
                  "skinny_stream_kernel<2,4>", "gemm_x6_kernel"):
        assert never not in f32, never
    by = dict(rows)
    assert family(by["test_gemm_skinny_stream[64-2048-2048-2]"]) == "small_gemm_kernel<true,8>"
    assert family(by["test_gemm_skinny_stream[32-2000-28224-32]"]) == "gemm_nt_kernel<nt::Skinny>"
    assert family(by["test_gemm_skinny_stream[8-1030-4104-5]"]) == "gemm_nt_kernel<nt::Skinny>"
    assert family(by["test_gemm_skinny_stream[33-1500-4096-7]"]) == "skinny_stream_kernel<2,4>"
    assert family(by["test_gemm_rollout_batch_forward[7]"]) == family(by["test_gemm_rollout_batch_forward[32]"]) == "gemm_nt_kernel<nt::Skinny>"
    assert family(by["test_gemm_rollout_batch_forward[7] A2C_NO_GEMM_NT=1"]) == "skinny_stream_kernel<1,4>"
    assert "tiles=73..73" in by["test_gemm_rollout_batch_forward[256]"]
    everything = {family(r) for _, r in rows}
    assert "small_gemm_kernel<false,8>" not in everything          # reached nowhere in the older tests
    assert {family(r) for n, r in rows if "skinny_stream" in family(r)} == {"skinny_stream_kernel<1,4>", "skinny_stream_kernel<2,4>"}
