"""CPU: a twin of the route-deciding integer predicates of csrc/conv.hip -- a2c_conv2d_fwd, a2c_conv2d_bwd_data and
a2c_conv2d_bwd_weight pick one of about forty kernel instantiations from the layer descriptor and the alignment of their
pointers, and the caller cannot see which one ran.  The suite's convolution cases are the layer shapes of the 84 x 84
models, which conv3.hip and the `run` kernels serve; the device worlds feed 80 x 80, 80 x 72 and 60 x 60 frames, where the
same models run the generic family of conv.hip.  `fwd_route`, `bwd_data_route` and `wgrad_route` repeat the choice and
name it as conv.hip writes the instantiation; `CASES` is the case list of tests/test_gpu_conv_worlds.py, as data, with
the route each case is MEANT to take.  The tests here hold the two together without a GPU:

  * the whitespace-normalised text of every restated condition is found in conv.hip / conv3.hip, and every instantiation
    of the route families that conv.hip launches has an entry in ROUTES: editing a gate or a launch breaks a test here
    until the twin is revisited;
  * every case lands where it says; the cases reach every ROUTES entry that a valid descriptor can reach (UNREACHABLE names
    the rest, with the reason), bwd_band2_kernel at vec 1, 2 and 4 and bwd_band_kernel with flat = 0 and flat = 1;
  * no case needs a fp64 CPU reference of more than 2e9 multiply-adds (computed from the spec);
  * the routes of CONV_SPECS of tests/test_gpu_kernels.py are printed (`pytest -s`): which kernel serves which of the older
    cases today.

What the twin does NOT model: tile heights, LDS budgets other than the defaults, grids and the tile tuners.  Two things
of that kind decide a route all the same and are restated at their defaults: the band height of band_setup under the
64 KB budget (the gate of bwd_band2_kernel needs the dOut rows of a band) and, of the row-run and prefetching kernels,
whether a band of ONE pixel row fits (`tph >= 1`).  The prefetch depth `pfb` of bwd_band2_kernel hangs on the band height
the tuner picks: its place in the name is a `?`.  The streaming kernels (conv_stream_kernel, conv2_stream_kernel,
wgrad_stream_kernel, wgrad_x6_kernel) need B >= 8 workgroups per CU-grid and exact A3CModel 84 x 84 shapes; no case here
has either, `bwd_data_route(..., B_streaming=True)` alone names the backward-data ones.

A route name is `instantiation attr ...`: `run-order` = the generic forward kernel on a layer whose fragments are laid
out for a row-run kernel, `per-class` = one igemm_kernel launch per stride class, `flat=0|1` = StageP::flat of
bwd_band_kernel, `+wgrad_reduce_kernel` = the slab reduction every weight gradient ends with.
"""
import ast
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-a2c_amd", "csrc")
HIP, HIP3 = os.path.join(CSRC, "conv.hip"), os.path.join(CSRC, "conv3.hip")
GPU_KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_kernels.py")

# ------------------------------------------------------------------------------------------------ constants of conv.hip
MAX_TAPS, CH, MAX_STEPS, MAX_CLS = 64, 8, 128, 4
PF_N, PF3, PF_B, PFB2_MAX, PF_D = 10, 16, 3, 16, 12
IGEMM_LDS_BUDGET, WGRAD_LDS_BUDGET, LDS_HARD_MAX = 64 * 1024, 48 * 1024, 160 * 1024
BS_NT, BS_PD, BS_PM = 512, 6, 4
CONSTANTS = [
    "constexpr int MAX_TAPS = 64;", "constexpr int CH = 8;", "constexpr int MAX_STEPS = 128;", "constexpr int MAX_CLS = 4;",
    "constexpr int PF_N = 10;", "constexpr int PF3 = 16;", "constexpr int PF_B = 3;", "constexpr int PFB2_MAX = 16;",
    "constexpr int PF_D = 12;", '#define IGEMM_LDS_BUDGET env_kb("A2C_IGEMM_LDS_KB", 64)',
    "constexpr int WGRAD_LDS_BUDGET = 48 * 1024;", "constexpr int LDS_HARD_MAX = 160 * 1024;",
    "constexpr int BS_NT = 512, BS_PD = 6, BS_PM = 4;",
]

WG_ARMS = {         # WGRAD_VARIANTS, arm by arm: template arguments as conv.hip writes them (defaults left out)
    "1,3,true,4,16,true": "WGRAD_PF_A: row split, three k-tiles, prefetching (4 -> 16 3x3, 16-B rows, even dOut rows)",
    "2,4,false,12,8,true": "WGRAD_PF_C: two channel tiles, prefetching (also what a prefetching nkt = 9 layer gets)",
    "2,4,false,14,8,true,2,1": "WGRAD_PF_D: 8-B input slots, 4-B dOut slots (W % 4 == 2)",
    "1,3,true,0,0,true": "row split, three k-tiles (4 -> 16 3x3)",
    "2,9,true,0,0,true": "row split, nine k-tiles (16 -> 17..32 3x3)",
    "1,1,false,0,0,true": "one channel tile, K <= 64",
    "1,4": "one channel tile, K <= 256",
    "2,4,false,0,0,true": "two channel tiles, 13..16 k-tiles",
    "2,4": "two channel tiles, fewer k-tiles",
    "4,5,false,0,0,true": "17..20 k-tiles (32 input channels, 3x3)",
    "4,7,false,0,0,true": "25..28 k-tiles (48 input channels, 3x3)",
    "4,7": "21..24 k-tiles, or 3..4 channel tiles with few k-tiles",
}
ROUTES = {
    **{f"igemm_kernel<{m}>": "generic forward / per-class backward-data, output tile through LDS" for m in (1, 2, 3, 4)},
    "igemm_run_kernel<1,8,4>": "row-run forward, 8x8 / 4, Cout <= 16", "igemm_run_kernel<2,8,4>": "row-run forward, 8x8 / 4, Cout <= 32",
    "igemm_run_kernel<1,4,2>": "row-run forward, 4x4 / 2, Cout <= 16", "igemm_run_kernel<2,4,2>": "row-run forward, 4x4 / 2, Cout <= 32",
    "igemm_run3_kernel<1,1>": "3x3 pad 1 stride 1, Cout <= 16", "igemm_run3_kernel<2,1>": "3x3 pad 1 stride 1, Cout <= 32",
    "igemm_run3_kernel<1,2>": "3x3 pad 1 stride 2, Cout <= 16", "igemm_run3_kernel<2,2>": "3x3 pad 1 stride 2, Cout <= 32",
    "bwd_fused_kernel<1>": "all classes of an unpadded ks = 2S layer, Cin <= 16", "bwd_fused_kernel<2>": "... Cin <= 32",
    **{f"bwd_band_kernel<{m},2>": "band of dX rows in LDS, fragments from L2" for m in (1, 2, 3, 4)},
    **{f"bwd_band2_kernel<1,{v},{p}>": "pipelined band kernel, fragments in LDS" for v in (1, 2, 4) for p in (8, 12, 16)},
    **{f"wgrad_kernel<{a}>": why for a, why in WG_ARMS.items()},
    "wgrad_run_kernel<1,4,1,5>": "row-run weight gradient, 8x8 / 4, 4 -> <= 16, 17..20 dOut columns",
    "wgrad_run_kernel<2,2,2,3>": "row-run weight gradient, 4x4 / 2, 16 -> 17..32, 9..12 dOut columns",
    "wgrad_reduce_kernel": "fixed-order sum of the per-workgroup slabs",
}
ROUTE_FAMILIES = {r.split("<")[0] for r in ROUTES}
# kernels conv.hip launches that the three entry points reach only at streaming batch, through another entry point or behind
# an opt-in switch; they have their own tests (test_gpu_kernels.py, test_gpu_conv3.py)
OTHER_KERNELS = {"conv_stream_kernel", "conv2_stream_kernel", "bwd_stream2_kernel", "bwd_x6_kernel", "lanemask_kernel", "wgrad_x6_kernel",
                 "wgrad_stream_kernel", "wgrad_stream_bf16_kernel", "prep_fwd_kernel", "prep_bwd_kernel"}
W1_FUSED = {f"bwd_band2_kernel<1,{v},{p},true>" for v in (1, 2, 4) for p in (8, 12, 16)}      # A2C_FUSE_W1=1 only
REFUSALS = {"ERR_ARG"}
# every ROUTES entry is reached by some desc_ok descriptor (CASES shows one each); were one not, it would be listed here by name
# with the reason, and test_cases_reach_every_route would hold the list to exactly the entries CASES misses
UNREACHABLE = {}

# the text of every restated condition, whitespace normalised, as it stands in conv.hip (comments stripped)
CONDITIONS = [
    # desc_ok
    "if (d->Cin < 4 || d->Cin % 4 || d->Cout < 4 || d->Cout % 4 || d->Cout > 64 || d->Cin > 64) return false;",
    "if (d->ks < 1 || d->stride < 1 || d->stride > 4 || (d->stride & (d->stride - 1)) || d->pad < 0 || d->pad >= d->ks) return false;",
    "if (d->ks * d->ks > MAX_TAPS) return false;",
    "if (pad_steps(d->ks * d->ks * (d->Cin / 4)) > MAX_STEPS) return false;",
    "if (pad_steps(ntaps_1d(d->ks, d->stride, 0) * ntaps_1d(d->ks, d->stride, 0) * (d->Cout / 4)) > MAX_STEPS) return false;",
    "if (d->OH != (d->H - d->ks + 2 * d->pad) / d->stride + 1 || d->OW != (d->W - d->ks + 2 * d->pad) / d->stride + 1) return false;",
    "return d->OH >= 1 && d->OW >= 1;",
    "static inline int ntaps_1d(int ks, int S, int r) { return r < ks ? (ks - r + S - 1) / S : 0; }",
    "static inline int pad_steps(int nsteps) { return ceil_div(nsteps > 0 ? nsteps : 1, CH) * CH; }",
    "off += (size_t)pad_steps(ntaps_1d(d->ks, S, ry) * ntaps_1d(d->ks, S, rx) * (d->Cout / 4)) * MTb * 64;",
    # run_layout, run3_layout
    "return d->pad == 0 && d->W % 4 == 0 && d->Cout <= 32 && ((d->ks == 8 && d->stride == 4) || (d->ks == 4 && d->stride == 2));",
    "return d->ks == 3 && d->pad == 1 && d->W % 4 == 0 && d->Cout <= 32 && (d->stride == 1 || d->stride == 2) && "
    "(size_t)9 * (d->Cin / 4) * ((d->Cout + 15) / 16) * 64 * 4 <= 48 * 1024;",
    # stage_vec
    "if (IW % 4 == 0 && bstride % 4 == 0 && ((long)IH * IW) % 4 == 0 && (uintptr_t)src % 16 == 0) return 4;",
    "if (IW % 2 == 0 && bstride % 2 == 0 && ((long)IH * IW) % 2 == 0 && (uintptr_t)src % 8 == 0) return 2;",
    # plan_src, first three lines
    "const int ncols = (t.PW - 1) * t.SX + t.span_x;",
    "t.WP = (t.sx0 == 0 && ncols <= t.IW) ? t.IW : ncols;",
    "if (t.WP < t.IW - t.sx0) t.WP = t.IW - t.sx0;",
    # a2c_conv2d_fwd, conv_fwd_impl
    "if (c3_supported(d, 0) && in_bstride % 4 == 0 && out_bstride % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0)",
    "const int nfrag = p.nchunks * CH * MT * 64;",
    "if (run && in_bstride % 4 == 0 && ((uintptr_t)in % 16 == 0) && nfrag * 4 <= 32 * 1024)",
    "if ((long)d->Cin * ((c - 1) * d->stride + d->ks) * d->W > 256L * PF_N * 4) break;",
    "if (d->ks == 8) k = MT == 1 ? (const void*)igemm_run_kernel<1, 8, 4> : (const void*)igemm_run_kernel<2, 8, 4>;",
    "else k = MT == 1 ? (const void*)igemm_run_kernel<1, 4, 2> : (const void*)igemm_run_kernel<2, 4, 2>;",
    "if (run3 && in_bstride % 4 == 0 && ((uintptr_t)in % 16 == 0))",
    'const long budget = fwd_kb > 0 ? fwd_kb * 1024L : (long)env_kb("A2C_RUN3_LDS_KB", 80);',
    "if ((long)d->Cin * tih * d->W > 256L * PF3 * 4) break;",
    "const int plane = ((tih * wp + 31) / 32) * 32 + (S == 1 ? 16 : 1);",
    "const long bytes = 4L * ((long)nfrag + (long)d->Cin * plane + 64 + (long)d->Cout * c * d->OW);",
    "if (run || run3)",
    # a2c_conv2d_bwd_data, conv_bwd_data_generic
    "if (c3_supported(d, 1) && (!mask || c3_bwd_mask_supported(d)) && ((uintptr_t)dout % 16) == 0 && ((uintptr_t)din % 16) == 0 && "
    "(!mask || ((uintptr_t)mask % 16) == 0))",
    "if (run_layout(d) && S * S <= MAX_CLS && MTb <= 2 && nel <= 256 * 4 * PF_B && (4 * c4n) % CH == 0 && nfrag * 4 <= 48 * 1024 && "
    "((uintptr_t)dout % 16 == 0) && ((uintptr_t)din % 16 == 0) && (!mask || (uintptr_t)mask % 16 == 0) && (d->H * d->W) % 4 == 0)",
    "if (S == 2 && d->ks == 4 && MTb == 1 && c4n == 8 && nel % 4 == 0 && nel <= BS_PD * BS_NT * 4 && "
    'd->Cin * d->H * d->W <= BS_PM * BS_NT * 4 && B >= 8 * stream_grid() && !a2c_env_on("A2C_NO_STREAM"))',
    "if (d->Cout == 32 && d->Cin == 16 && d->OH == 9 && d->OW == 9 && d->H == 20 && d->W == 20 && P == 0 && "
    'a2c_env_int("A2C_BWD_X6", 1) != 0)',
    "const void* k = MTb == 1 ? (const void*)bwd_fused_kernel<1> : (const void*)bwd_fused_kernel<2>;",
    "if (S * S <= MAX_CLS && ((uintptr_t)din % 16 == 0) && (!mask || (uintptr_t)mask % 16 == 0))",
    "const int rc = launch_igemm(p, ceil_div(d->Cin, 16), a2c_s(stream));",
    # band_setup, launch_bwd_band
    "const int ox_lo = (P - (d->ks - 1)) >= 0 ? (P - (d->ks - 1)) / S : -((-(P - (d->ks - 1)) + S - 1) / S);",
    "const int ox_hi = (d->W - 1 + P) / S;",
    "for (int ty = S; ty <= ((d->H + S - 1) / S) * S; ty += S)",
    "const int tih = (ty - 1 + d->ks - 1) / S + 2;",
    "const int plane = ((tih * WPo + 31) / 32) * 32 + 16;",
    "const long bytes = 4L * ((long)d->Cin * ty * d->W + (long)d->Cout * plane + 64);",
    "if (ty_force > 0 ? ty == ty_force : (bytes <= IGEMM_LDS_BUDGET || TY == 0)) { TY = ty; TIH = tih; PLANEo = plane; }",
    "if (ty_force > 0 ? ty >= ty_force : bytes > IGEMM_LDS_BUDGET) break;",
    "if (TY > d->H) TY = d->H;",
    "q.st.vec = stage_vec(dout, q.st.bstride, d->OH, d->OW); q.st.flat = (TY == d->H && q.st.vec != 4 && "
    "((long)d->Cout * d->OH * d->OW) % 4 == 0 && ((long)d->Cin * d->H * d->W) % 4 == 0 && ((uintptr_t)dout % 16 == 0)) ? 1 : 0;",
    "const int MTb = ceil_div(d->Cin, 16), c4n = d->Cout / 4;",
    "const long tot_v = (long)d->Cout * TIH * (d->OW / vecs);",
    "const size_t lds2 = 4 * (nfrag + (size_t)q.out_floats + (size_t)d->Cout * PLANEo + 64);",
    "if (nfrag * 4 <= 64 * 1024 && d->OW % vecs == 0 && tot_v <= 256L * PFB2_MAX && MTb == 1 && c4n % 2 == 0 && lds2 <= LDS_HARD_MAX)",
    "const int pfb = tot_v <= 256L * 8 ? 8 : tot_v <= 256L * 12 ? 12 : 16;",
    "BAND2_CASE(1, 8) BAND2_CASE(1, 12) BAND2_CASE(1, 16) BAND2_CASE(2, 8) BAND2_CASE(2, 12) BAND2_CASE(2, 16) "
    "BAND2_CASE(4, 8) BAND2_CASE(4, 12) BAND2_CASE(4, 16)",
    "size_t lds = 4 * ((size_t)q.out_floats + (size_t)d->Cout * PLANEo + 64);",
    "if (q.st.flat && q.bands == 1 && MTb >= 2 && MTb <= 4 && lds > 80 * 1024 && d->Cin % 16 == 0 && (16 * d->H * d->W) % 4 == 0 && "
    '!a2c_env_on("A2C_NO_BAND_GROUPS"))',
    "const size_t lds1 = 4 * ((size_t)16 * TY * d->W + (size_t)d->Cout * PLANEo + 64);",
    "if (lds1 <= 80 * 1024)",
    "if (lds <= LDS_HARD_MAX && MTb <= 4)",
    "if (MTk == 1) BAND_RUN(1, 2) else if (MTk == 2) BAND_RUN(2, 2) else if (MTk == 3) BAND_RUN(3, 2) else BAND_RUN(4, 2)",
    # a2c_conv2d_bwd_weight, wgrad_run_variant, plan_wgrad
    "const bool aligned = (in_bstride % 4 == 0) && ((uintptr_t)in % 16 == 0) && ((uintptr_t)dout % 8 == 0);",
    "if (!plan_wgrad(d, B, pl, aligned)) return A2C_ERR_ARG;",
    "if (c3w_supported(d) && aligned && ((uintptr_t)dout % 16 == 0) && ((uintptr_t)dW % 16 == 0) && ((uintptr_t)ws % 16 == 0))",
    "if (!run_layout(d)) return 0;",
    "const int mt = ceil_div(d->Cout, 16), c4n = ceil_div(d->OW, 4), rgs = d->Cin * d->ks * 2 / 16;",
    "if (d->stride == 4 && mt == 1 && rgs == 4 && c4n == 5) return 1;",
    "if (d->stride == 2 && mt == 2 && rgs == 8 && c4n == 3) return 2;",
    "pl.run = allow_run ? wgrad_run_variant(d) : 0;",
    "const int plane = ((tih * d->W + 63) / 64) * 64;",
    "const int planeo = ((c * pl.OWp + 31) / 32) * 32 + 2;",
    "const long bytes = 4L * ((long)d->Cin * plane + (long)pl.MT * 16 * planeo + 64);",
    "if ((long)d->Cin * tih * d->W <= 256L * PF_N * 4 && (long)d->Cout * c * d->OW <= 256L * PF_D && bytes <= WGRAD_LDS_BUDGET) tph = c; else break;",
    "const int nkt = ceil_div(d->Cin * d->ks * d->ks, 16);",
    "const int ktw = ceil_div(nkt, 4);",
    "if (mt == 1 && nkt == 3) { pl.MT = 1; pl.KTW = 3; pl.rs = 1; }",
    "else if (mt == 2 && nkt == 9) { pl.MT = 2; pl.KTW = 9; pl.rs = 1; }",
    "else if (mt == 1 && ktw <= 1) { pl.MT = 1; pl.KTW = 1; }",
    "else if (mt == 1 && ktw <= 4) { pl.MT = 1; pl.KTW = 4; }",
    "else if (mt <= 2 && ktw <= 4) { pl.MT = 2; pl.KTW = 4; }",
    "else if (mt <= 4 && ktw == 5) { pl.MT = 4; pl.KTW = 5; }",
    "else if (mt <= 4 && ktw <= 7) { pl.MT = 4; pl.KTW = 7; }",
    "else return false;",
    "pl.ex = (ktw == pl.KTW) ? 1 : 0;",
    "if (allow_run && d->W % 4 == 0 && d->OW % 2 == 0)",
    "const int ni = (pl.rs && pl.KTW == 3) ? 4 : (pl.rs && pl.KTW == 9) ? 8 : (!pl.rs && pl.MT == 2 && pl.KTW == 4 && pl.ex) ? 12 : 0;",
    "const int nd = (pl.rs && pl.KTW == 3) ? 16 : 8;",
    "for (int c = 1; c <= d->OH && ni; ++c)",
    "const long plane = ((tih * t.WP + 31) / 32) * 32 + 16, planeo = ((c * pl.OWp + 31) / 32) * 32 + 2;",
    "if ((long)d->Cin * tih * (d->W / 4) <= 256L * ni && (long)d->Cout * c * (d->OW / 2) <= 256L * nd && tih < 256 && "
    "4 * (d->Cin * plane + pl.MT * 16 * planeo + 64) <= budget) tph = c; else break;",
    "if (!pl.pf && allow_run && d->W % 4 && d->W % 2 == 0 && pl.ex && !pl.rs && pl.MT == 2 && pl.KTW == 4)",
    "if ((long)d->Cin * tih * (d->W / 2) <= 256L * 14 && (long)d->Cout * c * d->OW <= 256L * 8 && tih < 256 && "
    "4 * (d->Cin * plane + pl.MT * 16 * planeo + 64) <= budget) tph = c; else break;",
    # WGRAD_VARIANTS
    "#define WGRAD_PF_A 1, 3, true, 4, 16, true", "#define WGRAD_PF_C 2, 4, false, 12, 8, true", "#define WGRAD_PF_D 2, 4, false, 14, 8, true, 2, 1",
    "if (pl.pf == 2) { X(WGRAD_PF_D); } \\ else if (pl.pf && pl.KTW == 3) { X(WGRAD_PF_A); } \\ else if (pl.pf) { X(WGRAD_PF_C); } \\ "
    "else if (pl.rs && pl.KTW == 3) { X(1, 3, true, 0, 0, true); } \\ else if (pl.rs) { X(2, 9, true, 0, 0, true); } \\ "
    "else if (pl.MT == 1 && pl.KTW == 1) { X(1, 1, false, 0, 0, true); } \\ else if (pl.MT == 1 && pl.KTW == 4) { X(1, 4); } \\ "
    "else if (pl.MT == 2 && pl.KTW == 4 && pl.ex) { X(2, 4, false, 0, 0, true); } \\ else if (pl.MT == 2 && pl.KTW == 4) { X(2, 4); } \\ "
    "else if (pl.KTW == 5) { X(4, 5, false, 0, 0, true); } \\ else if (pl.ex) { X(4, 7, false, 0, 0, true); } \\ else { X(4, 7); }",
    "if (pl.run == 1) hipLaunchKernelGGL((wgrad_run_kernel<1, 4, 1, 5>), dim3(pl.grid), dim3(256), pl.lds, st, q);",
    "else hipLaunchKernelGGL((wgrad_run_kernel<2, 2, 2, 3>), dim3(pl.grid), dim3(256), pl.lds, st, q);",
]
CONDITIONS3 = [     # conv3.hip: the shape lists
    "if (d->ks != 3 || d->pad != 1 || d->stride != 2 || d->H != d->W) return false; "
    "return (d->H == 21 && d->Cin == 32 && d->Cout == 48) || (d->H == 11 && d->Cin == 48 && d->Cout == 64);",
    "bool c3_bwd_mask_supported(const a2c_conv_desc* d) { return c3_supported(d, 1) && !c3bs_odd_shape(d); }",
    "if (kind == 1 && d->stride == 2) return c3b_shape(d) || c3bs_odd_shape(d); if (d->ks != 3 || d->pad != 1) return false; "
    "if (kind == 0 && d->stride == 2 && d->H == 42 && d->W == 42) return (d->Cin == 32 && d->Cout == 64) || (d->Cin == 24 && d->Cout == 32); "
    "if (kind == 0 && d->stride == 2 && d->H == 21 && d->W == 21) return d->Cin == 32 && d->Cout == 48; "
    "if (kind == 0 && d->stride == 2 && d->H == 11 && d->W == 11) return d->Cin == 48 && d->Cout == 64; "
    "if (d->H != 84 || d->W != 84) return false; if (kind == 0) { "
    "if (d->stride == 1) return (d->Cin == 4 && d->Cout == 16) || (d->Cin == 16 && d->Cout == 24); "
    "if (d->stride == 2) return (d->Cin == 24 && d->Cout == 32) || (d->Cin == 16 && d->Cout == 24); return false; } "
    "if (d->stride == 1) return d->Cin == 16 && d->Cout == 24; return d->stride == 2; }",
    "if (d->ks != 3 || d->pad != 1 || d->stride != 2) return false; "
    "return (d->H == 84 && d->W == 84 && ((d->Cin == 24 && d->Cout == 32) || (d->Cin == 16 && d->Cout == 24))) || "
    "(d->H == 42 && d->W == 42 && ((d->Cin == 32 && d->Cout == 64) || (d->Cin == 24 && d->Cout == 32)));",
    "#define C3W_CASES(X) \\ X(4, 16, 84, 84, 1, 6, 4, 1, 3) \\ X(16, 24, 84, 84, 1, 3, 16, 1, 3) \\ X(24, 32, 84, 84, 2, 6, 8, 2, 2) \\ "
    "X(32, 64, 42, 42, 2, 7, 8, 4, 3) \\ X(16, 24, 84, 84, 2, 6, 8, 1, 2) \\ X(24, 32, 42, 42, 2, 7, 12, 2, 3) \\ X(32, 48, 21, 21, 2, 11, 16, 4, 2)",
    "if (d->Cin == cs && d->Cout == cd && d->H == h && d->W == w_ && d->stride == s_) return true;",
]
C3W_CASES = [(4, 16, 84, 84, 1), (16, 24, 84, 84, 1), (24, 32, 84, 84, 2), (32, 64, 42, 42, 2), (16, 24, 84, 84, 2), (24, 32, 42, 42, 2),
             (32, 48, 21, 21, 2)]


# ------------------------------------------------------------------------------------------------------------ the twin
class Desc:
    def __init__(self, spec):
        self.Cin, self.H, self.W, self.Cout, self.ks, self.stride, self.pad = spec
        self.OH = (self.H - self.ks + 2 * self.pad) // self.stride + 1        # a2c_amd.ops.conv_desc
        self.OW = (self.W - self.ks + 2 * self.pad) // self.stride + 1


def ceil_div(a, b):
    return (a + b - 1) // b


def ntaps_1d(ks, S, r):
    return (ks - r + S - 1) // S if r < ks else 0


def pad_steps(n):
    return ceil_div(n if n > 0 else 1, CH) * CH


def desc_ok(d):
    if d.Cin < 4 or d.Cin % 4 or d.Cout < 4 or d.Cout % 4 or d.Cout > 64 or d.Cin > 64:
        return False
    if d.ks < 1 or d.stride < 1 or d.stride > 4 or (d.stride & (d.stride - 1)) or d.pad < 0 or d.pad >= d.ks:
        return False
    if d.ks * d.ks > MAX_TAPS:
        return False
    if pad_steps(d.ks * d.ks * (d.Cin // 4)) > MAX_STEPS:
        return False
    if pad_steps(ntaps_1d(d.ks, d.stride, 0) ** 2 * (d.Cout // 4)) > MAX_STEPS:
        return False
    return d.OH >= 1 and d.OW >= 1


def run_layout(d):
    return d.pad == 0 and d.W % 4 == 0 and d.Cout <= 32 and ((d.ks == 8 and d.stride == 4) or (d.ks == 4 and d.stride == 2))


def run3_layout(d):
    return (d.ks == 3 and d.pad == 1 and d.W % 4 == 0 and d.Cout <= 32 and d.stride in (1, 2)
            and 9 * (d.Cin // 4) * ((d.Cout + 15) // 16) * 64 * 4 <= 48 * 1024)


def c3b_shape(d):
    if d.ks != 3 or d.pad != 1 or d.stride != 2:
        return False
    return ((d.H == 84 and d.W == 84 and (d.Cin, d.Cout) in ((24, 32), (16, 24)))
            or (d.H == 42 and d.W == 42 and (d.Cin, d.Cout) in ((32, 64), (24, 32))))


def c3bs_odd_shape(d):
    if d.ks != 3 or d.pad != 1 or d.stride != 2 or d.H != d.W:
        return False
    return (d.H == 21 and d.Cin == 32 and d.Cout == 48) or (d.H == 11 and d.Cin == 48 and d.Cout == 64)


def c3_supported(d, kind):
    if kind == 1 and d.stride == 2:
        return c3b_shape(d) or c3bs_odd_shape(d)
    if d.ks != 3 or d.pad != 1:
        return False
    if kind == 0 and d.stride == 2 and d.H == 42 and d.W == 42:
        return (d.Cin, d.Cout) in ((32, 64), (24, 32))
    if kind == 0 and d.stride == 2 and d.H == 21 and d.W == 21:
        return d.Cin == 32 and d.Cout == 48
    if kind == 0 and d.stride == 2 and d.H == 11 and d.W == 11:
        return d.Cin == 48 and d.Cout == 64
    if d.H != 84 or d.W != 84:
        return False
    if kind == 0:
        if d.stride == 1:
            return (d.Cin, d.Cout) in ((4, 16), (16, 24))
        if d.stride == 2:
            return (d.Cin, d.Cout) in ((24, 32), (16, 24))
        return False
    if d.stride == 1:
        return d.Cin == 16 and d.Cout == 24
    return d.stride == 2


def c3_bwd_mask_supported(d):
    return c3_supported(d, 1) and not c3bs_odd_shape(d)


def c3w_supported(d):
    if d.ks != 3 or d.pad != 1:
        return False
    return (d.Cin, d.Cout, d.H, d.W, d.stride) in C3W_CASES


def stage_vec(src_al, bstride, IH, IW):
    """src_al: the largest power of two (bytes, up to 16) the source pointer is a multiple of"""
    if IW % 4 == 0 and bstride % 4 == 0 and (IH * IW) % 4 == 0 and src_al % 16 == 0:
        return 4
    if IW % 2 == 0 and bstride % 2 == 0 and (IH * IW) % 2 == 0 and src_al % 8 == 0:
        return 2
    return 1


def bwd_class_offset(d, cls):
    S, MTb = d.stride, ceil_div(d.Cin, 16)
    return sum(pad_steps(ntaps_1d(d.ks, S, c // S) * ntaps_1d(d.ks, S, c % S) * (d.Cout // 4)) * MTb * 64 for c in range(cls))


def fwd_route(spec, aligned=True):
    """a2c_conv2d_fwd below streaming batch.  aligned: in_bstride % 4 == 0 (the pointers of a test are always 16-B aligned)"""
    d = Desc(spec)
    if not desc_ok(d):
        return "ERR_ARG"
    if c3_supported(d, 0) and aligned:
        return "c3_fwd"
    MT, c4n = ceil_div(d.Cout, 16), d.Cin // 4
    nfrag = pad_steps(d.ks * d.ks * c4n) * MT * 64
    run, run3 = run_layout(d), run3_layout(d)
    if run and aligned and nfrag * 4 <= 32 * 1024:
        if d.Cin * d.ks * d.W <= 256 * PF_N * 4:                                    # a band of one output row fits the registers
            return f"igemm_run_kernel<{MT},{d.ks},{d.stride}>"
    if run3 and aligned:
        S = d.stride
        plane = ((3 * (d.W + 2) + 31) // 32) * 32 + (16 if S == 1 else 1)
        nbytes = 4 * (nfrag + d.Cin * plane + 64 + d.Cout * d.OW)
        if d.Cin * 3 * d.W <= 256 * PF3 * 4 and nbytes <= 80 * 1024:
            return f"igemm_run3_kernel<{MT},{S}>"
    return f"igemm_kernel<{MT}>" + (" run-order" if run or run3 else "")


def band_plan(d, dout_al=16):
    """band_setup at ty_force = 0 and the default budget -> TY, TIH, PLANEo, vec, flat"""
    S, P = d.stride, d.pad
    e = P - (d.ks - 1)
    ox_lo = e // S if e >= 0 else -((-e + S - 1) // S)
    ox_hi = (d.W - 1 + P) // S
    WPo = ox_hi - ox_lo + 1
    TY = TIH = PLANEo = 0
    for ty in range(S, ((d.H + S - 1) // S) * S + 1, S):
        tih = (ty - 1 + d.ks - 1) // S + 2
        plane = ((tih * WPo + 31) // 32) * 32 + 16
        nbytes = 4 * (d.Cin * ty * d.W + d.Cout * plane + 64)
        if nbytes <= IGEMM_LDS_BUDGET or TY == 0:
            TY, TIH, PLANEo = ty, tih, plane
        if nbytes > IGEMM_LDS_BUDGET:
            break
    TY = min(TY, d.H)
    vec = stage_vec(dout_al, d.Cout * d.OH * d.OW, d.OH, d.OW)
    flat = int(TY == d.H and vec != 4 and (d.Cout * d.OH * d.OW) % 4 == 0 and (d.Cin * d.H * d.W) % 4 == 0 and dout_al % 16 == 0)
    return TY, TIH, PLANEo, vec, flat


def bwd_data_route(spec, aligned=True, B_streaming=False, mask=True):
    """a2c_conv2d_bwd_data.  aligned: dout is 16-B aligned (False: offset by one float; din and the mask always are).
    B_streaming: B >= 8 * stream_grid()"""
    d = Desc(spec)
    if not desc_ok(d):
        return "ERR_ARG"
    dout_al = 16 if aligned else 4
    if c3_supported(d, 1) and (not mask or c3_bwd_mask_supported(d)) and aligned:
        return "c3_bwd_data"
    S, MTb, c4n = d.stride, ceil_div(d.Cin, 16), d.Cout // 4
    nfrag = bwd_class_offset(d, S * S)
    nel = d.Cout * d.OH * d.OW
    if (run_layout(d) and S * S <= MAX_CLS and MTb <= 2 and nel <= 256 * 4 * PF_B and (4 * c4n) % CH == 0 and nfrag * 4 <= 48 * 1024
            and aligned and (d.H * d.W) % 4 == 0):
        if (S == 2 and d.ks == 4 and MTb == 1 and c4n == 8 and nel % 4 == 0 and nel <= BS_PD * BS_NT * 4
                and d.Cin * d.H * d.W <= BS_PM * BS_NT * 4 and B_streaming):
            if (d.Cout, d.Cin, d.OH, d.OW, d.H, d.W, d.pad) == (32, 16, 9, 9, 20, 20, 0):
                return f"bwd_x6_kernel<{1 if mask else 0}>"
            return f"bwd_stream2_kernel<{1 if mask else 0}>"
        if 4 * (nfrag + d.Cout * ((((d.OH + 2) * (d.OW + 2) + 31) // 32) * 32 + 16) + 64 + d.Cin * d.H * d.W) > LDS_HARD_MAX:
            return "ERR_ARG"
        return f"bwd_fused_kernel<{MTb}>"
    if S * S <= MAX_CLS:
        TY, TIH, PLANEo, vec, flat = band_plan(d, dout_al)
        unsure = "?" if c3_supported(d, 1) else ""          # (conv3.hip's fragments, not modelled, count towards nfrag)
        out_floats = d.Cin * TY * d.W
        tot_v = d.Cout * TIH * (d.OW // vec)
        lds2 = 4 * (nfrag + out_floats + d.Cout * PLANEo + 64)
        if nfrag * 4 <= 64 * 1024 and d.OW % vec == 0 and tot_v <= 256 * PFB2_MAX and MTb == 1 and c4n % 2 == 0 and lds2 <= LDS_HARD_MAX:
            return f"bwd_band2_kernel<1,{vec},?>" + unsure
        lds = 4 * (out_floats + d.Cout * PLANEo + 64)
        MTk = MTb
        if flat and ceil_div(d.H, TY) == 1 and 2 <= MTb <= 4 and lds > 80 * 1024 and d.Cin % 16 == 0 and (16 * d.H * d.W) % 4 == 0:
            lds1 = 4 * (16 * TY * d.W + d.Cout * PLANEo + 64)
            if lds1 <= 80 * 1024:
                MTk, lds = 1, lds1
        if lds <= LDS_HARD_MAX and MTb <= 4:
            return f"bwd_band_kernel<{MTk},2> flat={flat}" + (f" mgroups={MTb}" if MTk != MTb else "")
    return f"igemm_kernel<{MTb}> per-class"


def wgrad_plan(d, allow_run):
    """plan_wgrad -> (run, MT, KTW, rs, ex, pf), or None (the ladder has no rung: A2C_ERR_ARG)"""
    OWp = ceil_div(d.OW, 4) * 4
    mt = ceil_div(d.Cout, 16)
    run = 0
    if allow_run and run_layout(d):
        c4n, rgs = ceil_div(d.OW, 4), d.Cin * d.ks * 2 // 16
        if d.stride == 4 and mt == 1 and rgs == 4 and c4n == 5:
            run = 1
        if d.stride == 2 and mt == 2 and rgs == 8 and c4n == 3:
            run = 2
    if run:
        plane, planeo = ((d.ks * d.W + 63) // 64) * 64, ((OWp + 31) // 32) * 32 + 2          # c = 1
        if (d.Cin * d.ks * d.W <= 256 * PF_N * 4 and d.Cout * d.OW <= 256 * PF_D
                and 4 * (d.Cin * plane + mt * 16 * planeo + 64) <= WGRAD_LDS_BUDGET):
            return run, mt, 0, 0, 0, 0
    nkt = ceil_div(d.Cin * d.ks * d.ks, 16)
    ktw = ceil_div(nkt, 4)
    rs = 0
    if mt == 1 and nkt == 3:
        MT, KTW, rs = 1, 3, 1
    elif mt == 2 and nkt == 9:
        MT, KTW, rs = 2, 9, 1
    elif mt == 1 and ktw <= 1:
        MT, KTW = 1, 1
    elif mt == 1 and ktw <= 4:
        MT, KTW = 1, 4
    elif mt <= 2 and ktw <= 4:
        MT, KTW = 2, 4
    elif mt <= 4 and ktw == 5:
        MT, KTW = 4, 5
    elif mt <= 4 and ktw <= 7:
        MT, KTW = 4, 7
    else:
        return None
    ex = int(ktw == KTW)
    # plan_src's first three lines: the width of the staged rows
    sx0 = -d.pad
    ncols = (d.OW - 1) * d.stride + d.ks
    WP = d.W if (sx0 == 0 and ncols <= d.W) else ncols
    if WP < d.W - sx0:
        WP = d.W - sx0
    plane, planeo = ((d.ks * WP + 31) // 32) * 32 + 16, ((OWp + 31) // 32) * 32 + 2              # c = 1
    fits = d.ks < 256 and 4 * (d.Cin * plane + MT * 16 * planeo + 64) <= 64 * 1024
    pf = 0
    if allow_run and d.W % 4 == 0 and d.OW % 2 == 0:
        ni = 4 if (rs and KTW == 3) else 8 if (rs and KTW == 9) else 12 if (not rs and MT == 2 and KTW == 4 and ex) else 0
        nd = 16 if (rs and KTW == 3) else 8
        if ni and d.Cin * d.ks * (d.W // 4) <= 256 * ni and d.Cout * (d.OW // 2) <= 256 * nd and fits:
            pf = 1
    if not pf and allow_run and d.W % 4 and d.W % 2 == 0 and ex and not rs and MT == 2 and KTW == 4:
        if d.Cin * d.ks * (d.W // 2) <= 256 * 14 and d.Cout * d.OW <= 256 * 8 and fits:
            pf = 2
    return 0, MT, KTW, rs, ex, pf


def wgrad_arm(MT, KTW, rs, ex, pf):
    """WGRAD_VARIANTS"""
    if pf == 2:
        return "2,4,false,14,8,true,2,1"
    if pf and KTW == 3:
        return "1,3,true,4,16,true"
    if pf:
        return "2,4,false,12,8,true"
    if rs and KTW == 3:
        return "1,3,true,0,0,true"
    if rs:
        return "2,9,true,0,0,true"
    if MT == 1 and KTW == 1:
        return "1,1,false,0,0,true"
    if MT == 1 and KTW == 4:
        return "1,4"
    if MT == 2 and KTW == 4 and ex:
        return "2,4,false,0,0,true"
    if MT == 2 and KTW == 4:
        return "2,4"
    if KTW == 5:
        return "4,5,false,0,0,true"
    if ex:
        return "4,7,false,0,0,true"
    return "4,7"


def wgrad_route(spec, aligned=True, dout_al=16):
    """a2c_conv2d_bwd_weight below streaming batch.  aligned: in_bstride % 4 == 0; dout_al: alignment of dout in bytes (dW and
    the workspace of a test are always 16-B aligned)"""
    d = Desc(spec)
    if not desc_ok(d):
        return "ERR_ARG"
    al = aligned and dout_al % 8 == 0
    pl = wgrad_plan(d, al)
    if pl is None:
        return "ERR_ARG"
    if c3w_supported(d) and al and dout_al % 16 == 0:
        return "c3w_bwd_weight"
    run, MT, KTW, rs, ex, pf = pl
    if run:
        return ("wgrad_run_kernel<1,4,1,5>" if run == 1 else "wgrad_run_kernel<2,2,2,3>") + " +wgrad_reduce_kernel"
    return f"wgrad_kernel<{wgrad_arm(MT, KTW, rs, ex, pf)}> +wgrad_reduce_kernel"


def family(r):
    return r.split()[0].rstrip("?")


def ref_macs(spec, B):
    """multiply-adds of the fp64 reference of one case: forward, backward-data (with and without mask share one) and weight gradient"""
    d = Desc(spec)
    return 3 * B * d.Cout * d.OH * d.OW * d.Cin * d.ks * d.ks


# ----------------------------------------------------------------------------------------------------------- the cases
FRAMES = [(80, 80), (80, 72), (60, 60)]          # Pong-device, Breakout-device (H x W), Snake-device
STACKS = {          # (Cout, ks, stride, pad) per layer, from 4 input planes
    "A3CModel": [(16, 8, 4, 0), (32, 4, 2, 0)],
    "ConvModel": [(16, 3, 1, 1), (24, 3, 1, 1), (32, 3, 2, 1), (64, 3, 2, 1)],
    "GRUModel": [(16, 3, 1, 1), (24, 3, 2, 1), (32, 3, 2, 1), (48, 3, 2, 1), (64, 3, 2, 1)],
}


def stack_specs(model, H, W):
    out, cin = [], 4
    for cout, ks, s, p in STACKS[model]:
        out.append((cin, H, W, cout, ks, s, p))
        H, W, cin = (H - ks + 2 * p) // s + 1, (W - ks + 2 * p) // s + 1, cout
    return out


def model_specs():
    seen = []
    for model in STACKS:
        for H, W in FRAMES:
            for s in stack_specs(model, H, W):
                if s not in seen:
                    seen.append(s)
    return seen


# spec -> (forward, backward-data, weight gradient) as the aligned call of the GPU file is meant to run it
def _w(arm):
    return f"wgrad_kernel<{arm}> +wgrad_reduce_kernel"


_PER_CLASS, _B2 = "igemm_kernel<1> per-class", "bwd_band2_kernel<1,%d,?>"
_PF_A, _PF_C, _PF_D = _w("1,3,true,4,16,true"), _w("2,4,false,12,8,true"), _w("2,4,false,14,8,true,2,1")
_K5, _K7 = _w("4,5,false,0,0,true"), _w("4,7,false,0,0,true")
MODEL_ROUTES = {
    # A3CModel
    (4, 80, 80, 16, 8, 4, 0): ("igemm_run_kernel<1,8,4>", _PER_CLASS, "wgrad_run_kernel<1,4,1,5> +wgrad_reduce_kernel"),
    (16, 19, 19, 32, 4, 2, 0): ("igemm_kernel<2>", _B2 % 4, _w("2,4,false,0,0,true")),
    (4, 80, 72, 16, 8, 4, 0): ("igemm_run_kernel<1,8,4>", _PER_CLASS, "wgrad_run_kernel<1,4,1,5> +wgrad_reduce_kernel"),
    (16, 19, 17, 32, 4, 2, 0): ("igemm_kernel<2>", _B2 % 1, _w("2,4,false,0,0,true")),
    (4, 60, 60, 16, 8, 4, 0): ("igemm_run_kernel<1,8,4>", _PER_CLASS, _w("1,4")),
    (16, 14, 14, 32, 4, 2, 0): ("igemm_kernel<2>", _B2 % 2, _PF_D),
    # ConvModel
    (4, 80, 80, 16, 3, 1, 1): ("igemm_run3_kernel<1,1>", _B2 % 4, _PF_A),
    (16, 80, 80, 24, 3, 1, 1): ("igemm_run3_kernel<2,1>", _B2 % 4, _PF_C),
    (24, 80, 80, 32, 3, 2, 1): ("igemm_run3_kernel<2,2>", "bwd_band_kernel<2,2> flat=0", _PF_C),
    (32, 40, 40, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<2,2> flat=0", _K5),
    (4, 80, 72, 16, 3, 1, 1): ("igemm_run3_kernel<1,1>", _B2 % 4, _PF_A),
    (16, 80, 72, 24, 3, 1, 1): ("igemm_run3_kernel<2,1>", _B2 % 4, _PF_C),
    (24, 80, 72, 32, 3, 2, 1): ("igemm_run3_kernel<2,2>", "bwd_band_kernel<2,2> flat=0", _PF_C),
    (32, 40, 36, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<2,2> flat=0", _K5),
    (4, 60, 60, 16, 3, 1, 1): ("igemm_run3_kernel<1,1>", _B2 % 4, _PF_A),
    (16, 60, 60, 24, 3, 1, 1): ("igemm_run3_kernel<2,1>", _B2 % 4, _PF_C),
    (24, 60, 60, 32, 3, 2, 1): ("igemm_run3_kernel<2,2>", "bwd_band_kernel<2,2> flat=0", _PF_C),
    (32, 30, 30, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<2,2> flat=0", _K5),
    # GRUModel
    (16, 80, 80, 24, 3, 2, 1): ("igemm_run3_kernel<2,2>", _B2 % 4, _PF_C),
    (24, 40, 40, 32, 3, 2, 1): ("igemm_run3_kernel<2,2>", "bwd_band_kernel<2,2> flat=0", _PF_C),
    (32, 20, 20, 48, 3, 2, 1): ("igemm_kernel<3>", "bwd_band_kernel<2,2> flat=0", _K5),
    (48, 10, 10, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<3,2> flat=1", _K7),          # whole sample, 5-wide dOut rows
    (16, 80, 72, 24, 3, 2, 1): ("igemm_run3_kernel<2,2>", _B2 % 4, _PF_C),
    (24, 40, 36, 32, 3, 2, 1): ("igemm_run3_kernel<2,2>", "bwd_band_kernel<2,2> flat=0", _PF_C),
    (32, 20, 18, 48, 3, 2, 1): ("igemm_kernel<3>", "bwd_band_kernel<2,2> flat=0", _K5),
    (48, 10, 9, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<3,2> flat=1", _K7),
    (16, 60, 60, 24, 3, 2, 1): ("igemm_run3_kernel<2,2>", _B2 % 2, _PF_C),
    (24, 30, 30, 32, 3, 2, 1): ("igemm_kernel<2>", "bwd_band_kernel<2,2> flat=0", _PF_D),
    (32, 15, 15, 48, 3, 2, 1): ("igemm_kernel<3>", "bwd_band_kernel<2,2> flat=0", _K5),          # whole sample, vec == 4
    (48, 8, 8, 64, 3, 2, 1): ("igemm_kernel<4>", "bwd_band_kernel<3,2> flat=0", _K7),            # whole sample, vec == 4
}
# small desc_ok shapes (non-square and odd where the route allows) for what no model layer at a world frame reaches
SYNTHETIC = {
    (4, 36, 36, 32, 8, 4, 0): ("igemm_run_kernel<2,8,4>", _PER_CLASS, _PF_C),      # 32 KB of fragments: the edge of the gate
    (8, 20, 20, 16, 4, 2, 0): ("igemm_run_kernel<1,4,2>", "bwd_fused_kernel<1>", _w("1,4")),
    # K = 512 is 32 k-tiles: plan_wgrad's ladder ends at 28 and the weight gradient of this layer is refused
    (32, 12, 12, 16, 4, 2, 0): ("igemm_run_kernel<1,4,2>", "bwd_fused_kernel<2>", "ERR_ARG"),
    (16, 6, 24, 20, 4, 2, 0): ("igemm_run_kernel<2,4,2>", "bwd_band_kernel<1,2> flat=1", "wgrad_run_kernel<2,2,2,3> +wgrad_reduce_kernel"),
    (4, 10, 8, 12, 3, 2, 1): ("igemm_run3_kernel<1,2>", "bwd_band_kernel<1,2> flat=0", _PF_A),
    (64, 7, 6, 8, 2, 1, 1): ("igemm_kernel<1>", "bwd_band_kernel<4,2> flat=1", _w("1,4")),
    (4, 9, 7, 8, 4, 2, 0): ("igemm_kernel<1>", _B2 % 2, _w("1,1,false,0,0,true")),
    (8, 9, 7, 20, 3, 2, 1): ("igemm_kernel<2>", "bwd_band_kernel<1,2> flat=0", _w("2,4")),
    (8, 7, 9, 36, 3, 2, 1): ("igemm_kernel<3>", "bwd_band_kernel<1,2> flat=1", _w("4,7")),
}
# spec, what is unaligned ("bstride": in_bstride % 4 == 1; "dout": dout offset by one float) -> routes (None: not called)
UNALIGNED = {
    ((4, 80, 80, 16, 3, 1, 1), "bstride"): ("igemm_kernel<1> run-order", None, _w("1,3,true,0,0,true")),
    ((4, 80, 80, 16, 3, 1, 1), "dout"): (None, "bwd_band_kernel<1,2> flat=0", _w("1,3,true,0,0,true")),
    ((4, 80, 72, 16, 8, 4, 0), "bstride"): ("igemm_kernel<1> run-order", None, _w("1,4")),
    ((4, 80, 72, 16, 8, 4, 0), "dout"): (None, _PER_CLASS, _w("1,4")),
    ((16, 80, 80, 24, 3, 2, 1), "bstride"): ("igemm_kernel<2> run-order", None, _w("2,9,true,0,0,true")),
    ((16, 80, 80, 24, 3, 2, 1), "dout"): (None, "bwd_band_kernel<1,2> flat=0", _w("2,9,true,0,0,true")),
}
# more tiles than workgroups (B = 320): spec -> the family the case stands for (all three passes run on each)
PERSISTENT = {
    (32, 40, 40, 64, 3, 2, 1): "igemm_kernel<4>",
    (24, 80, 80, 32, 3, 2, 1): "bwd_band_kernel<2,2>",
    (16, 80, 80, 24, 3, 2, 1): "bwd_band2_kernel<1,4,?>",
    (16, 80, 72, 24, 3, 1, 1): "wgrad_kernel<2,4,false,12,8,true>",
}
PERSISTENT_B = 320
BATCHES = (1, 5)
MAX_REF_MACS = 2e9


def _cases():
    cases = []
    for spec in model_specs():
        cases.append(dict(spec=spec, kind="model", expect=MODEL_ROUTES.get(spec)))
    for spec, exp in SYNTHETIC.items():
        cases.append(dict(spec=spec, kind="synthetic", expect=exp))
    return cases


CASES = _cases()


def case_routes(spec, unaligned=None):
    if unaligned == "bstride":
        return fwd_route(spec, False), None, wgrad_route(spec, False)
    if unaligned == "dout":
        return None, bwd_data_route(spec, False), wgrad_route(spec, True, dout_al=4)
    return fwd_route(spec), bwd_data_route(spec), wgrad_route(spec)


# ------------------------------------------------------------------------------------------------------------ the tests
def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _norm(t):
    return re.sub(r"\s+", " ", t).strip()


def _launched(src):
    """kernel instantiations conv.hip launches, the launcher templates and macros of the route families expanded"""
    inst = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_0-9]+)\s*(<[^;]*?>)?\s*\)?\s*,\s*dim3", src):
        inst.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    out = set()
    for k in inst:
        if k == "igemm_kernel<MT>":
            out |= {f"igemm_kernel<{a}>" for a in re.findall(r"launch_igemm_t<(\d)>\(", src)}
        elif k == "bwd_band2_kernel<1,V_,P_>":
            out |= {f"bwd_band2_kernel<1,{v},{p}>" for v, p in re.findall(r"BAND2_CASE\((\d+), (\d+)\)", src)}
        elif k == "bwd_band2_kernel<1,V_,P_,true>":
            cases = re.search(r"#define BAND_W1_CASES\(X\)([^\n]*)", src).group(1)
            out |= {f"bwd_band2_kernel<1,{v},{p},true>" for v, p in re.findall(r"X\((\d+), (\d+)\)", cases)}
        elif k == "bwd_band_kernel<M_,N_>":
            out |= {f"bwd_band_kernel<{a},{b}>" for a, b in re.findall(r"BAND_RUN\((\d+), (\d+)\)", src)}
        elif k == "wgrad_kernel<MT,KTW,RS,NI,ND,EX,VI,VD>":
            body = re.search(r"#define WGRAD_VARIANTS\(X\)(.*?)\n\n", src, flags=re.S).group(1)
            defs = dict(re.findall(r"#define (WGRAD_PF_\w) ([^\n]*)", src))
            for a in re.findall(r"X\(([^)]*)\)", body):
                out.add("wgrad_kernel<" + defs.get(a.strip(), a).replace(" ", "") + ">")
        else:
            out.add(k)
    return out


def test_every_restated_condition_and_every_launch_is_in_the_source():
    """conv.hip and conv3.hip, read as text: the conditions the twin repeats stand there word for word, and the route
    families' instantiations that conv.hip launches are exactly ROUTES"""
    src, src3 = _strip_comments(open(HIP).read()), _strip_comments(open(HIP3).read())
    flat, flat3 = _norm(src), _norm(src3)
    for text in CONSTANTS + CONDITIONS:
        assert _norm(text) in flat, f"conv.hip no longer says: {text}"
    for text in CONDITIONS3:
        assert _norm(text) in flat3, f"conv3.hip no longer says: {text}"
    launched = _launched(src)
    fam = {k for k in launched if k.split("<")[0] in ROUTE_FAMILIES} - W1_FUSED
    assert fam - set(ROUTES) == set(), f"launched without a route: {sorted(fam - set(ROUTES))}"
    assert set(ROUTES) - fam == set(), f"routes that nothing launches: {sorted(set(ROUTES) - fam)}"
    rest = {k.split("<")[0] for k in launched - fam - W1_FUSED}
    assert rest == OTHER_KERNELS, sorted(rest ^ OTHER_KERNELS)
    assert W1_FUSED <= launched
    # the twelve arms of WGRAD_VARIANTS, and band_setup decides `flat` from a `vec` that is already assigned
    assert len({k for k in fam if k.startswith("wgrad_kernel<")}) == len(WG_ARMS) == 12
    assert flat.index("q.st.vec = stage_vec(dout") < flat.index("q.st.flat = (TY == d->H")


def test_every_case_lands_on_the_route_it_names():
    specs = [c["spec"] for c in CASES]
    assert len(specs) == len(set(specs))
    assert set(MODEL_ROUTES) == set(model_specs()), sorted(set(MODEL_ROUTES) ^ set(model_specs()))
    for c in CASES:
        assert desc_ok(Desc(c["spec"])), c["spec"]
        assert case_routes(c["spec"]) == c["expect"], (c["spec"], case_routes(c["spec"]), c["expect"])
        assert bwd_data_route(c["spec"], mask=False) == c["expect"][1], c["spec"]        # (mask or not: the same kernel)
    for (spec, what), exp in UNALIGNED.items():
        assert spec in specs
        assert case_routes(spec, what) == exp, (spec, what, case_routes(spec, what), exp)
    for spec in PERSISTENT:
        assert spec in specs


def _reached():
    got = set()
    for c in CASES:
        got |= {r for r in case_routes(c["spec"]) if r}
    for spec, what in UNALIGNED:
        got |= {r for r in case_routes(spec, what) if r}
    return got


def test_cases_reach_every_route():
    got = _reached()
    fams = {family(r) for r in got} - REFUSALS
    if any("+wgrad_reduce_kernel" in r for r in got):
        fams.add("wgrad_reduce_kernel")
    # bwd_band2_kernel: the prefetch depth is the tuner's; the vector width is the route
    band2 = {f for f in fams if f.startswith("bwd_band2_kernel")}
    assert band2 == {f"bwd_band2_kernel<1,{v},?>" for v in (1, 2, 4)}, sorted(band2)
    want = {r for r in ROUTES if not r.startswith("bwd_band2_kernel")}
    missing = want - fams
    assert missing == set(UNREACHABLE), f"reached by no case: {sorted(missing - set(UNREACHABLE))}; listed but reached: {sorted(set(UNREACHABLE) - missing)}"
    assert fams - band2 - want <= set(), sorted(fams - band2 - want)
    # the per-class fallback (stride 4: sixteen classes are more than the band kernels take), and both values of `flat`
    assert any(r.endswith("per-class") and Desc(c["spec"]).stride == 4 for c in CASES for r in [case_routes(c["spec"])[1]])
    flats = {r.split("flat=")[1][:1] for r in got if "flat=" in r}
    assert flats == {"0", "1"}, flats
    whole_vec4 = [c["spec"] for c in CASES if "flat=0" in case_routes(c["spec"])[1]
                  and band_plan(Desc(c["spec"]))[0] == c["spec"][1] and band_plan(Desc(c["spec"]))[3] == 4]
    assert whole_vec4, "no whole-sample band with vec == 4 (the case band_setup's ordering decides)"
    # the unaligned entries leave the row-run and prefetching kernels: generic forward, scalar staging, no `run`, no `pf`
    for (spec, what), (f, b, w) in UNALIGNED.items():
        if what == "bstride":
            assert family(f).startswith("igemm_kernel<") and wgrad_plan(Desc(spec), False)[0] == 0 and wgrad_plan(Desc(spec), False)[5] == 0
        else:
            assert band_plan(Desc(spec), 4)[3] == 1 and not family(b).startswith(("bwd_fused", "c3_"))
            assert wgrad_plan(Desc(spec), False)[5] == 0
    for spec, fam in PERSISTENT.items():
        assert fam in {family(r) for r in case_routes(spec)}, (spec, fam, case_routes(spec))
    assert {f.split("<")[0] for f in PERSISTENT.values()} == {"igemm_kernel", "bwd_band_kernel", "bwd_band2_kernel", "wgrad_kernel"}


def test_cases_stay_small():
    worst = max((ref_macs(c["spec"], max(BATCHES)), c["spec"]) for c in CASES)
    for c in CASES:
        assert ref_macs(c["spec"], max(BATCHES)) <= MAX_REF_MACS, c["spec"]
    print(f"\n{len(CASES)} specs, largest fp64 reference {worst[0]:.3g} multiply-adds at {worst[1]}, "
          f"sum {sum(ref_macs(c['spec'], b) for c in CASES for b in BATCHES):.3g}")


def test_routes_of_the_world_frames_and_of_the_older_conv_tests():
    """printed with -s: which kernels serve the layer stacks at the world frames, and which the CONV_SPECS of
    tests/test_gpu_kernels.py; at 84 x 84 the stacks never see the generic family the world frames run"""
    m = re.search(r"^CONV_SPECS = (\[.*?^\])", open(GPU_KERNELS).read(), flags=re.S | re.M)
    older = ast.literal_eval(re.sub(r"#[^\n]*", "", m.group(1)))
    assert len(older) == 14
    print()
    for title, specs in (("CONV_SPECS of test_gpu_kernels.py", older), ("world frames", [c["spec"] for c in CASES if c["kind"] == "model"]),
                         ("synthetic", [c["spec"] for c in CASES if c["kind"] == "synthetic"])):
        print(f"  {title}")
        for s in specs:
            f, b, w = case_routes(s)
            print(f"    {str(s):30s} {f:28s} {b:36s} {w}")
    print("  unaligned")
    for (s, what) in UNALIGNED:
        print(f"    {str(s):30s} {what:8s} " + "  ".join(r for r in case_routes(s, what) if r))
    old = set()
    for s in older:
        old |= {family(r) for r in case_routes(s)}
    for never in ("igemm_run_kernel<2,8,4>", "igemm_run_kernel<1,4,2>", "bwd_fused_kernel<2>", "igemm_kernel<3>", "bwd_band_kernel<4,2>",
                  "wgrad_kernel<2,4,false,14,8,true,2,1>", "wgrad_kernel<4,7>", "wgrad_kernel<2,4>"):
        assert never not in old, never
    # the 84 x 84 stacks: conv3.hip and the row-run kernels; no layer of theirs is generic in all three passes
    for model in STACKS:
        for s in stack_specs(model, 84, 84):
            f, b, w = case_routes(s)
            assert f.startswith(("c3_", "igemm_run")) or w.startswith(("c3w", "wgrad_run")), (s, f, b, w)


@pytest.mark.parametrize("spec, want", [((4, 84, 84, 16, 8, 4, 0), ("igemm_run_kernel<1,8,4>", "igemm_kernel<1>", "wgrad_run_kernel<1,4,1,5>")),
                                        ((16, 20, 20, 32, 4, 2, 0), ("igemm_run_kernel<2,4,2>", "bwd_fused_kernel<1>", "wgrad_run_kernel<2,2,2,3>")),
                                        ((16, 19, 19, 32, 4, 2, 0), ("igemm_kernel<2>", "bwd_band2_kernel<1,4,?>", "wgrad_kernel<2,4,false,0,0,true>")),
                                        ((16, 14, 14, 32, 4, 2, 0), ("igemm_kernel<2>", "bwd_band2_kernel<1,2,?>", "wgrad_kernel<2,4,false,14,8,true,2,1>")),
                                        ((32, 21, 21, 48, 3, 2, 1), ("c3_fwd", "bwd_band_kernel<2,2>", "c3w_bwd_weight"))], ids=str)
def test_twin_on_the_layers_the_sources_name(spec, want):
    """what conv.hip's own comments and the older tests say of A3CModel's layers at 84, 80 and 60 wide, and of GRUModel's conv4
    (float mask: conv3.hip's odd-image kernel reads sign words only, so the band kernel)"""
    got = case_routes(spec)
    assert tuple(family(r) for r in got) == want, got
    assert fwd_route((4, 84, 84, 16, 3, 1, 0)) == "igemm_kernel<1>" and fwd_route((4, 84, 84, 68, 3, 1, 1)) == "ERR_ARG"
    assert bwd_data_route((16, 20, 20, 32, 4, 2, 0), B_streaming=True) == "bwd_x6_kernel<1>"
