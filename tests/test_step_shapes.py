"""CPU: the frame-shape family of the one-launch A3C step / rollout kernels (csrc/step.hip: step_shapes + the step_lds
bound behind a2c_a3c_step_supported).  A plain-Python transcription of that predicate is held against the library on every
(H, W) below 130 x 130, and the eight shapes tests/test_gpu_step_shapes.py runs are pinned to the kernel paths they are
there for (ragged conv1 tile, conv2 loop split, stash / lane-mask / uint8 capability): if the predicate or a derived
quantity moves, this file fails instead of the GPU tests quietly running something else."""
import pytest

NT, HN, NF1, NF2 = 512, 8, 64 * 64, 64 * 2 * 64        # csrc/step.hip: threads, max heads, conv1 / conv2 fragment floats
STAGE = (6, 5, 5)                                      # float4 staging registers per thread and row chunk (SL0, SL1, SL2)
LDS_MAX = 160 * 1024

# id -> (H, W); the table of the GPU file.  DERIVED: what each row must reach, recomputed below by the transcription
SHAPES = {"S1": (84, 84), "S2": (68, 68), "S3": (76, 76), "S4": (64, 100), "S5": (32, 124), "S6": (48, 92),
          "S7": (85, 84), "S8": (108, 68)}
DERIVED = {  # (OH1, OW1), NP1, (OH2, OW2), ntile2, F, stash-able, lane-mask-able, uint8-able
    "S1": ((20, 20), 400, (9, 9), 6, 2592, True, True, True),
    "S2": ((16, 16), 256, (7, 7), 4, 1568, True, True, True),
    "S3": ((18, 18), 324, (8, 8), 4, 2048, True, False, True),
    "S4": ((15, 24), 360, (6, 11), 5, 2112, True, False, True),
    "S5": ((7, 30), 210, (2, 14), 2, 896, False, False, True),
    "S6": ((11, 22), 242, (4, 10), 3, 1280, False, False, True),
    "S7": ((20, 20), 400, (9, 9), 6, 2592, True, True, False),
    "S8": ((26, 16), 416, (12, 7), 6, 2688, True, True, True),
}


def plane_pad(n, mod64):
    """smallest p >= n with p % 64 == mod64"""
    p = ((n + 63) // 64) * 64 + mod64
    return p - 64 if p - 64 >= n else p


def step_shapes(C, H, W, A):
    """step_shapes() of csrc/step.hip, line by line: the derived sizes, or None where the kernels do not apply"""
    if C != 4 or H < 8 or W < 8 or W % 4 or A < 1 or A + 1 > HN:
        return None
    OH1, OW1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
    if OH1 < 4 or OW1 < 4 or OW1 % 2:
        return None
    OH2, OW2 = (OH1 - 4) // 2 + 1, (OW1 - 4) // 2 + 1
    PLANE1, PLANE2 = plane_pad(H * W, 0), plane_pad(OH1 * OW1, 32)
    F = 32 * OH2 * OW2
    F4 = ((F + 3) // 4) * 4
    if F % 4 or F > 2 * NT * 4:
        return None
    ntile2 = (OH2 * OW2 + 15) // 16
    if 4 * PLANE1 < NF2 + F4 + ntile2 * 1024 + HN * NT:
        return None
    or0, or1 = (OH1 * 7 + 19) // 20, (OH1 * 14 + 19) // 20
    row_end = (4 * (or0 - 1) + 8, 4 * (or1 - 1) + 8, H)
    if not (0 < row_end[0] < row_end[1] < H):
        return None
    ntile1 = (OH1 * OW1 + 15) // 16
    tile_end = (or0 * OW1 // 16, or1 * OW1 // 16, ntile1)
    for k in range(3):
        rows = row_end[k] - (row_end[k - 1] if k else 0)
        if rows * W > STAGE[k] * NT:
            return None
    return dict(OH1=OH1, OW1=OW1, OH2=OH2, OW2=OW2, PLANE1=PLANE1, PLANE2=PLANE2, F=F, F4=F4, ntile1=ntile1, ntile2=ntile2,
                row_end=row_end, tile_end=tile_end, NP1=OH1 * OW1, NP2=OH2 * OW2,
                lds=4 * (NF1 + 4 * PLANE1 + 16 * PLANE2 + 8 * HN + 16 + 32))


def supported(C, H, W, A):
    p = step_shapes(C, H, W, A)
    return int(p is not None and p["lds"] <= LDS_MAX)


def derived(H, W, A=3):
    """the columns of DERIVED for one shape"""
    p = step_shapes(4, H, W, A)
    return ((p["OH1"], p["OW1"]), p["NP1"], (p["OH2"], p["OW2"]), p["ntile2"], p["F"], p["NP1"] % 4 == 0,
            (16 * p["NP1"]) % 256 == 0, (H * W) % 16 == 0 and H * W <= 16 * NT)


@pytest.fixture(scope="module")
def lib():
    from a2c_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_table_rows_are_in_the_family(lib, sid):
    H, W = SHAPES[sid]
    for A in (1, 3, 7):
        assert lib.a2c_a3c_step_supported(4, H, W, A) == 1, (sid, A)
    assert lib.a2c_a3c_step_supported(4, H, W, 8) == 0
    assert lib.a2c_a3c_step_supported(3, H, W, 3) == 0


def test_shapes_outside_the_family_are_refused(lib):
    for H, W in ((80, 80), (80, 72), (72, 72), (64, 64)):      # odd conv1 output width
        assert lib.a2c_a3c_step_supported(4, H, W, 3) == 0, (H, W)
        assert supported(4, H, W, 3) == 0


def test_transcription_agrees_with_the_library_below_130(lib):
    n = 0
    for H in range(8, 130):
        for W in range(8, 129, 4):
            got, want = supported(4, H, W, 3), lib.a2c_a3c_step_supported(4, H, W, 3)
            assert got == want, (H, W, got, want)
            n += want
    assert n == 454          # (W % 4 != 0 is refused outright: these are all the pairs with H, W < 130)
    for H in range(8, 130):
        for W in (9, 30, 85, 127):
            assert lib.a2c_a3c_step_supported(4, H, W, 3) == 0 == supported(4, H, W, 3)


@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_table_rows_reach_the_paths_they_are_there_for(sid):
    H, W = SHAPES[sid]
    assert derived(H, W) == DERIVED[sid]


def test_what_the_rows_are_there_for():
    p = {s: step_shapes(4, *SHAPES[s], 3) for s in SHAPES}
    # ragged last conv1 tile: only S1, S2, S7, S8 end on a full 16-pixel tile
    assert {s for s in p if p[s]["NP1"] % 16 == 0} == {"S1", "S2", "S7", "S8"}
    assert p["S3"]["NP1"] % 16 == 4 and p["S4"]["NP1"] % 16 == 8
    # conv2's weight fragments come tap-major where conv1's output width is no multiple of 4 (conv.hip keeps the (c4, ky, kx)
    # order for layers its row-run kernel takes): the kernels must permute them on S3, S5, S6
    assert {s for s in p if p[s]["OW1"] % 4} == {"S3", "S5", "S6"}
    # ring conv2: waves w = 0..7 take units w, w+8, w+16 at once while unit + 16 < 4 * ntile2, the tail loop the rest
    unrolled = lambda s: any(w + 16 < 4 * p[s]["ntile2"] for w in range(8))
    tail = lambda s: any((w if not w + 16 < 4 * p[s]["ntile2"] else w + 24) < 4 * p[s]["ntile2"] for w in range(8))
    assert not unrolled("S2") and tail("S2") and not unrolled("S3")
    assert unrolled("S4") and tail("S4")
    assert unrolled("S1") and not tail("S1")
    # S4: chunk boundaries fall inside conv1 output rows
    assert any((e * 16) % p["S4"]["OW1"] for e in p["S4"]["tile_end"][:2])
    # S5: row chunks of 16 / 8 / 8 input rows; S7: one trailing row no conv window reads; S8: the LDS and staging edges
    assert p["S5"]["row_end"] == (16, 24, 32)
    assert 4 * (p["S7"]["OH1"] - 1) + 8 == 84 < 85
    assert 0 <= LDS_MAX - p["S8"]["lds"] < 3 * 1024
    assert p["S8"]["row_end"][0] * 68 == 2992 <= STAGE[0] * NT == 3072
    assert max(q["F"] for q in p.values()) == p["S8"]["F"]
