"""gsdr_ddc_plan (csrc/ddc_plan.h through host_logic.cpp): the rules by which a DIRECT handle takes its engine, its
product loop and, call by call, its kernel and the row tiles per workgroup.  No GPU: the exported function asks the
functions the handle asks.  Each rule is pinned on both sides of its edge, so that a threshold or a comparison in
ddc_plan.h altered by one fails here; tests/test_gpu_ddc_plan.py holds a handle's describe() to the same answers.

Windows are stated in 32-sample blocks: with M = 8 T samples per block and F = 4 tap phases a window is exactly T of
them (as in the threshold tests of test_gpu_mfma3.py, test_gpu_fold.py, test_gpu_span128.py).  256 compute units (1024
SIMDs) unless a test says otherwise.
"""
import pytest

import _ddc_plan
from _product_loops import COMMON, LOOPS

FOUR = (4, 1, 0, 0, 32, 64)                 # describe() of a handle without a product loop of its own
PREC = {"GSDR_MFMA_PREC": "1"}              # images whatever the launch size
NO_FEW = {"GSDR_DDC_FEW": "0"}              # also where ddc_few_kernel would take the shape (up to 32 tones, M >= 512)


def window(lib, T, N=64, rows=34, env=None, **kw):
    """The plan of a handle with a window of T blocks (M = 8 T, F = 4), `rows` rows per buffer"""
    return _ddc_plan.plan(lib, N, 8 * T, 4, 8 * T * rows, env=env, **kw)


def test_window_blocks_select_the_loop(gsdr_lib):
    """Three products, the pair rotation and the fold from 94 blocks (kMac3MinBlocks, kRot2MinBlocks, kFoldMinBlocks);
    on the wide tile 128-sample spans from 125 (kSpan128MinBlocks).  4096 tones in 34 rows: 256 workgroups, half a
    round of the overlapped entries, so the handle has images by its own rule from windows of 32 blocks."""
    assert window(gsdr_lib, 93, N=4096)["describe"] == FOUR
    assert window(gsdr_lib, 93, N=4096)["images"] == 1
    assert window(gsdr_lib, 94, N=4096)["describe"] == (3, 2, 1, 4, 64, 64)
    assert window(gsdr_lib, 124, N=4096)["describe"] == (3, 2, 1, 4, 64, 64)
    assert window(gsdr_lib, 125, N=4096)["describe"] == (3, 2, 1, 4, 64, 128)
    # a narrow-tile shape keeps the 64-sample spans at every length
    assert window(gsdr_lib, 125, env=PREC)["describe"] == (3, 2, 1, 4, 32, 64)
    p = window(gsdr_lib, 94, N=4096)
    assert (p["complex_mac_min_blocks"], p["rotation_min_blocks"], p["fold_min_blocks"], p["span128_min_blocks"]) == (94, 94, 94, 125)


def test_each_rule_is_asked_only_of_a_handle_the_one_before_took(gsdr_lib):
    """The thresholds one by one: the rules in front forced on at 93 blocks, the rule itself left to the window."""
    on3 = dict(PREC, GSDR_MFMA_3M="1")
    on_rot = dict(on3, GSDR_MFMA_3M_ROT="2")
    assert window(gsdr_lib, 93, env=on3)["describe"] == (3, 1, 0, 0, 32, 64)          # rotation: 94
    assert window(gsdr_lib, 93, env=on_rot)["describe"] == (3, 2, 0, 0, 32, 64)       # fold: 94
    assert window(gsdr_lib, 94, env=dict(on3, GSDR_MFMA_3M_ROT="1"))["describe"] == (3, 1, 0, 0, 32, 64)
    assert window(gsdr_lib, 94, env=dict(PREC, GSDR_MFMA_3M="0", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="1"))["describe"] == FOUR


def test_images_by_launch_size(gsdr_lib):
    """prec_pays for the handle's largest launch in an overlapped entry: half a round of workgroups (256 of 1024 / 4
    SIMDs' worth) with windows of 32 blocks or more, or four rounds (2048) whatever the window."""
    assert window(gsdr_lib, 32, N=4096)["images"] == 1                   # 8 * 32 = 256 workgroups
    assert window(gsdr_lib, 32, N=4095 - 127)["images"] == 0             # 8 * 31 = 248
    assert window(gsdr_lib, 31, N=4096)["images"] == 0                   # 31 blocks
    assert window(gsdr_lib, 1, N=128 * 256)["images"] == 1               # 8 * 256 = 2048 workgroups
    assert window(gsdr_lib, 1, N=128 * 255)["images"] == 0
    assert window(gsdr_lib, 1, N=128 * 256, env={"GSDR_MFMA_PREC": "0"})["images"] == 0
    assert window(gsdr_lib, 1, env=PREC)["images"] == 1
    # per launch: the in-order entries ask for four rounds, whatever the window
    p = window(gsdr_lib, 32, N=4096)
    assert (p["preconverted"], window(gsdr_lib, 32, N=4096, overlapped=True)["preconverted"]) == (0, 1)
    assert window(gsdr_lib, 1, N=128 * 256)["preconverted"] == 1


def wide_pays(rows, tones):
    ntg = (tones + 31) // 32
    return -(-rows // 16) * -(-ntg // 8) <= -(-rows // 32) * -(-ntg // 4)


def test_wide_tile(gsdr_lib):
    """16 rows x 64 tones where that launches no more waves: ceil(rows/16) ceil(ntg/8) <= ceil(rows/32) ceil(ntg/4)"""
    assert window(gsdr_lib, 94, N=128, env=PREC)["describe"] == (3, 2, 1, 4, 32, 64)
    assert window(gsdr_lib, 94, N=129, env=PREC)["describe"] == (3, 2, 1, 4, 64, 64)
    for rows in (3, 16, 17, 32, 33, 34, 48, 49, 64, 65, 70):
        for tones in (1, 32, 33, 64, 65, 128, 129, 256, 257, 288, 1024):
            got = window(gsdr_lib, 94, N=tones, rows=rows, env=dict(PREC, **NO_FEW))["describe"]
            assert got == (3, 2, 1, 4, 64 if wide_pays(rows, tones) else 32, 64), (rows, tones, got)


FORCED = [
    # (environment on top of GSDR_MFMA_PREC=1, blocks, tones) -> the six values
    ({"GSDR_MFMA_3M": "1"}, 1, 64, (3, 1, 0, 0, 32, 64)),
    ({"GSDR_MFMA_3M": "0"}, 200, 64, FOUR),
    ({"GSDR_MFMA_3M": "2"}, 200, 64, FOUR),
    ({"GSDR_MFMA_3M_ROT": "2"}, 93, 64, FOUR),                                        # nothing to rotate without 3M
    ({"GSDR_MFMA_3M": "1", "GSDR_MFMA_3M_ROT": "2"}, 1, 64, (3, 2, 0, 0, 32, 64)),
    ({"GSDR_MFMA_3M_ROT": "1"}, 200, 64, (3, 1, 0, 0, 32, 64)),
    ({"GSDR_MFMA_3M_ROT": "0"}, 200, 64, (3, 1, 0, 0, 32, 64)),
    ({"GSDR_MFMA_3M": "1", "GSDR_MFMA_3M_ROT": "2", "GSDR_MFMA_FOLD": "1"}, 1, 64, (3, 2, 1, 4, 32, 64)),
    ({"GSDR_MFMA_FOLD": "0"}, 200, 64, (3, 2, 0, 0, 32, 64)),
    ({"GSDR_MFMA_FOLD": "2"}, 200, 64, (3, 2, 0, 0, 32, 64)),
    ({"GSDR_MFMA_FOLD_PRODUCTS": "3"}, 94, 64, (3, 2, 1, 3, 32, 64)),
    ({"GSDR_MFMA_FOLD_PRODUCTS": "3"}, 94, 4096, (3, 2, 1, 3, 32, 64)),              # the Gauss fold has no wide tile
    ({"GSDR_MFMA_FOLD_PRODUCTS": "4"}, 94, 64, (3, 2, 1, 4, 32, 64)),
    ({"GSDR_MFMA_FOLD_PRODUCTS": "5"}, 94, 64, (3, 2, 1, 4, 32, 64)),
    ({"GSDR_MFMA_WAVE_TONES": "64"}, 94, 64, (3, 2, 1, 4, 64, 64)),
    ({"GSDR_MFMA_WAVE_TONES": "32"}, 94, 4096, (3, 2, 1, 4, 32, 64)),
    ({"GSDR_MFMA_WAVE_TONES": "48"}, 94, 4096, (3, 2, 1, 4, 64, 64)),                # neither 32 nor 64: by the rule
    ({"GSDR_MFMA_WAVE_TONES": "64"}, 125, 4096, (3, 2, 1, 4, 64, 64)),               # a forced wave tile keeps 64-sample spans
    ({"GSDR_MFMA_WAVE_TONES": "64", "GSDR_MFMA_SPAN": "128"}, 94, 64, (3, 2, 1, 4, 64, 128)),
    ({"GSDR_MFMA_SPAN": "128"}, 94, 4096, (3, 2, 1, 4, 64, 128)),
    ({"GSDR_MFMA_SPAN": "128"}, 200, 64, (3, 2, 1, 4, 32, 64)),                      # only on the wide tile
    ({"GSDR_MFMA_SPAN": "64"}, 200, 4096, (3, 2, 1, 4, 64, 64)),
    ({"GSDR_MFMA_SPAN": "0"}, 200, 4096, (3, 2, 1, 4, 64, 64)),
]


@pytest.mark.parametrize("env,T,N,want", FORCED, ids=lambda v: "_".join(f"{k[10:]}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_forcing_values(gsdr_lib, env, T, N, want):
    p = window(gsdr_lib, T, N=N, env=dict(PREC, **env))
    assert p["engine"] == "mfma" and p["describe"] == want, p
    assert p["row_tiles_per_workgroup"] == 1 and p["preconverted"] == 1 and p["eight_waves"] == 0, p


def test_loops_rows_give_their_own_values(gsdr_lib):
    """The rows of tests/_product_loops.py::LOOPS at a window of ONE block (nothing selects but the switches), the
    four-product loop chosen per launch and the 128-sample spans: the seven loops of the pre-converted family"""
    for name, (env, five) in LOOPS.items():
        for T in (1, 200):
            p = window(gsdr_lib, T, N=4096, env=env)
            assert p["describe"] == five + (64,), (name, T, p)
            assert (p["preconverted"], p["row_tiles_per_workgroup"], p["images"]) == (1, 1, 1), (name, p)
    assert window(gsdr_lib, 1, env=dict(COMMON, GSDR_MFMA_3M="0"))["describe"] == FOUR
    assert window(gsdr_lib, 1, env=dict(COMMON, GSDR_MFMA_3M="0"))["preconverted"] == 1
    assert window(gsdr_lib, 1, env=dict(LOOPS["p4fw"][0], GSDR_MFMA_SPAN="128"))["describe"] == (3, 2, 1, 4, 64, 128)


def test_kernel_forms(gsdr_lib):
    """GSDR_MFMA_ASM and the shape of the C++ kernel: only the ring16 loop at its one shape has images"""
    big = dict(N=128 * 256)
    for env, images in [({"GSDR_MFMA_ASM": "4"}, 1), ({"GSDR_MFMA_ASM": "5"}, 0), ({"GSDR_MFMA_ASM": "2"}, 0), ({"GSDR_MFMA_ASM": "0"}, 0),
                        ({"GSDR_MFMA_ASM": "4", "GSDR_MFMA_TT": "2"}, 0), ({"GSDR_MFMA_ASM": "4", "GSDR_MFMA_PK": "16"}, 0),
                        ({"GSDR_MFMA_ASM": "4", "GSDR_MFMA_W": "2"}, 0)]:
        p = window(gsdr_lib, 200, env=env, **big)
        assert p["engine"] == "mfma" and p["images"] == images, (env, p)
        assert p["describe"] == ((3, 2, 1, 4, 64, 128) if images else FOUR), (env, p)
        assert p["eight_waves"] == (env["GSDR_MFMA_ASM"] == "5" and len(env) == 1), (env, p)


def tiles(lib, ngt, N=64, T=1, **kw):
    """a launch of ngt row tiles; 64 tones: one workgroup per row tile"""
    return window(lib, T, N=N, rows=32 * ngt, **kw)


def test_two_row_tiles_per_workgroup(gsdr_lib):
    """rt = 2 exactly for overlapped calls of 512 <= workgroups < 1024 with windows of at most 32 blocks"""
    for ngt, rt in [(511, 1), (512, 2), (1023, 2), (1024, 1)]:
        assert tiles(gsdr_lib, ngt, overlapped=True)["row_tiles_per_workgroup"] == rt, ngt
        assert tiles(gsdr_lib, ngt)["row_tiles_per_workgroup"] == 1, ngt
        assert tiles(gsdr_lib, ngt, N=128, overlapped=True)["row_tiles_per_workgroup"] == rt, ngt      # still one workgroup per tile
    assert tiles(gsdr_lib, 256, N=129, overlapped=True)["row_tiles_per_workgroup"] == 2                  # two per tile: 512
    assert tiles(gsdr_lib, 255, N=129, overlapped=True)["row_tiles_per_workgroup"] == 1
    no_prec = {"GSDR_MFMA_PREC": "0"}
    assert tiles(gsdr_lib, 512, T=32, overlapped=True, env=no_prec)["row_tiles_per_workgroup"] == 2
    assert tiles(gsdr_lib, 512, T=33, overlapped=True, env=no_prec)["row_tiles_per_workgroup"] == 1
    # forced; a handle with a product loop of its own keeps one row tile per workgroup
    for rt in (1, 2):
        assert tiles(gsdr_lib, 3, env={"GSDR_MFMA_RT": str(rt)})["row_tiles_per_workgroup"] == rt
    assert tiles(gsdr_lib, 3, env={"GSDR_MFMA_RT": "3"})["row_tiles_per_workgroup"] == 1
    assert tiles(gsdr_lib, 512, T=94, overlapped=True, env=dict(PREC, GSDR_MFMA_RT="2"))["row_tiles_per_workgroup"] == 1
    # two row tiles per workgroup keep the launch off the pre-converted loop
    assert tiles(gsdr_lib, 512, overlapped=True, env=PREC)["preconverted"] == 0
    assert tiles(gsdr_lib, 511, overlapped=True, env=PREC)["preconverted"] == 1


def test_eight_wave_window(gsdr_lib):
    """In-order launches of more than simds / 4 and at most simds / 2 four-wave workgroups (row tiles counted in
    eights) that fit simds / 4 eight-wave workgroups; 1024 SIMDs: 256 < wgs4 <= 512, wgs8 <= 256"""
    for ngt, w8 in [(8 * 8, 0), (8 * 8 + 1, 1), (8 * 16, 1), (8 * 16 + 1, 0)]:        # 512 tones: wgs4 = 256, 288, 512, 544; wgs8 half
        p = tiles(gsdr_lib, ngt, N=512)
        assert (p["eight_waves"], p["row_tiles_per_workgroup"]) == (w8, 1), (ngt, p)
        assert tiles(gsdr_lib, ngt, N=512, overlapped=True)["eight_waves"] == 0, ngt
        assert tiles(gsdr_lib, ngt, N=512, env={"GSDR_MFMA_W8": "0"})["eight_waves"] == 0, ngt
    # 64 tones: an eight-wave workgroup per row tile as well, which never fits where four waves do not
    assert tiles(gsdr_lib, 8 * 32 + 1)["eight_waves"] == 0               # 264, 264
    # 1024 tones: 8 four-wave or 4 eight-wave workgroups per row tile; 1056: 9 and 5
    assert tiles(gsdr_lib, 8 * 8, N=1024)["eight_waves"] == 1            # 512, 256
    assert tiles(gsdr_lib, 8 * 7, N=1056)["eight_waves"] == 0            # 504, 280
    assert tiles(gsdr_lib, 8 * 6, N=1056)["eight_waves"] == 1            # 432, 240
    # the window scales with the device: 128 compute units
    assert [tiles(gsdr_lib, ngt, N=512, cus=128)["eight_waves"] for ngt in (8 * 4, 8 * 4 + 1, 8 * 8, 8 * 8 + 1)] == [0, 1, 1, 0]
    assert tiles(gsdr_lib, 8 * 10, N=512, env={"GSDR_MFMA_RT": "2"})["eight_waves"] == 0
    assert tiles(gsdr_lib, 8 * 10, N=512)["eight_waves"] == 1


def engine(lib, N, M, F, L, env=None):
    p = _ddc_plan.plan(lib, N, M, F, L, env=env)
    return p and p["engine"]


def test_matrix_core_shape_condition(gsdr_lib):
    """A buffer holds the carry (rows >= F - 1) and the zero padding behind a window fits the next block.  The other two
    clauses of the condition cannot decide for a handle that gsdr_demod_create accepts, which is stated here: F <= 33
    (pf_average is at most 8), and L >= 4 (with L <= 4 no M and F leave rows and padding in range)."""
    assert engine(gsdr_lib, 5, 50, 4, 100) == "generic"          # rows = F - 2
    assert engine(gsdr_lib, 5, 50, 4, 150) == "mfma"             # rows = F - 1
    assert engine(gsdr_lib, 5, 16, 1, 160) == "mfma"             # padding 16 = M
    assert engine(gsdr_lib, 5, 15, 1, 150) == "generic"          # padding 17 = M + 2
    assert engine(gsdr_lib, 5, 21, 2, 210) == "generic"          # window 42, padding 22 = M + 1
    assert engine(gsdr_lib, 5, 22, 2, 220) == "mfma"             # window 44, padding 20
    for L in (1, 2, 3, 4):
        for M in range(1, L + 1):
            for F in range(1, 9):
                if L % M == 0:
                    assert engine(gsdr_lib, 5, M, F, L) == "generic", (L, M, F)
    assert engine(gsdr_lib, 5, 50, 8, 350) == "mfma" and engine(gsdr_lib, 5, 50, 9, 400) is None
    # without the matrix cores: the flat kernel up to four tap phases, the generic one beyond or on request
    off = {"GSDR_DDC_MFMA": "0"}
    assert engine(gsdr_lib, 5, 50, 4, 150, env=off) == "flat" and engine(gsdr_lib, 5, 50, 5, 250, env=off) == "generic"
    assert engine(gsdr_lib, 5, 50, 4, 150, env=dict(off, GSDR_DDC_PIPE="0")) == "generic"
    assert engine(gsdr_lib, 5, 0, 4, 150) == "mix" and engine(gsdr_lib, 5, -1, 40, 150) == "mix"


def test_few_tones_at_a_long_decimation(gsdr_lib):
    assert engine(gsdr_lib, 32, 512, 4, 4096) == "few"
    assert engine(gsdr_lib, 32, 511, 4, 4088) == "mfma"
    assert engine(gsdr_lib, 33, 512, 4, 4096) == "mfma"
    assert engine(gsdr_lib, 1, 4096, 4, 8192) == "few"           # also where the matrix cores refuse (rows < F - 1)
    assert engine(gsdr_lib, 32, 512, 4, 4096, env=NO_FEW) == "mfma"
    assert engine(gsdr_lib, 32, 512, 4, 4096, env={"GSDR_DDC_MFMA": "0"}) == "flat"
    assert engine(gsdr_lib, 32, 512, 5, 4096, env={"GSDR_DDC_MFMA": "0"}) == "generic"


def test_refusals(gsdr_lib):
    """What gsdr_demod_create refuses of these fields"""
    ok = dict(N=5, M=50, F=4, L=150)
    assert _ddc_plan.plan(gsdr_lib, **ok) is not None
    for bad in (dict(N=0), dict(L=0), dict(L=149), dict(F=0), dict(F=9), dict(rate=0), dict(cus=0), dict(rows=-1), dict(rows=4),
                dict(M=1 << 29, L=1 << 29)):
        assert _ddc_plan.plan(gsdr_lib, **dict(ok, **bad)) is None, bad
    assert _ddc_plan.plan(gsdr_lib, 5, 1 << 28, 7, 1 << 28) is not None       # decim * pf_average = 2^31 - 2^28
    assert _ddc_plan.plan(gsdr_lib, 5, 0, 99, 149) is not None                # undecimated: pf_average is not read


FLAT = {"GSDR_DDC_MFMA": "0", "GSDR_DDC_AUTOTUNE": "0"}


def test_flat_sub_block(gsdr_lib):
    """K of {40, 20, 16, 12} with the least nsub * (K + 3.3); pad and R follow"""
    def cost(M, k):
        return -(-M // k) * (k + 3.3)
    for M in (12, 13, 37, 50, 64, 90, 100, 127, 250, 1000, 4096):
        p = _ddc_plan.plan(gsdr_lib, 8, M, 4, 40 * M, env=FLAT)
        K = min((40, 20, 16, 12), key=lambda k: cost(M, k))
        nsub = -(-M // K)
        assert (p["engine"], p["K"], p["pad"], p["R"]) == ("flat", K, nsub * K - M, M - (nsub - 1) * K), (M, p)
    assert [_ddc_plan.plan(gsdr_lib, 8, M, 4, 40 * M, env=FLAT)["K"] for M in (100, 1000, 37, 48, 24)] == [20, 40, 40, 16, 12]
    for k in (12, 16, 20, 40):
        p = _ddc_plan.plan(gsdr_lib, 8, 100, 4, 4000, env=dict(FLAT, GSDR_DDC_K=str(k)))
        assert (p["K"], p["pad"]) == (k, -(-100 // k) * k - 100), p
    assert _ddc_plan.plan(gsdr_lib, 8, 100, 4, 4000, env=dict(FLAT, GSDR_DDC_K="32"))["K"] == 20      # not a flat length
    # the generic kernel: a table of 16, or of 32 on request
    gen = dict(FLAT, GSDR_DDC_PIPE="0")
    assert [_ddc_plan.plan(gsdr_lib, 8, 100, 4, 4000, env=dict(gen, GSDR_DDC_K=k))[f] for k in ("", "32", "40") for f in ("K", "R", "pad")] == \
        [16, 4, 0, 32, 4, 0, 16, 4, 0]


def test_chunks(gsdr_lib):
    """Every chunk holds F - 1 blocks or more, no launch takes more chunks than the tails buffer has slots, a forced
    count is honoured up to both caps, and the balanced count lies within 20 % of the count it started from"""
    for F in (1, 2, 4):
        for N in (8, 64, 65, 300):
            for rows in (3, 7, 100, 1000, 5003, 100_000):
                if rows < F - 1:
                    continue
                TW = -(-N // 64)
                full = _ddc_plan.plan(gsdr_lib, N, 100, F, 100 * rows, env=FLAT)
                assert full["target_waves"] == 1024 * 6 and full["chunks_want"] == int(1.3 * 1024 * 6) // TW
                cap = rows // (F - 1) if F > 1 else rows
                assert full["tails_nch"] == max(1, min(cap, int(1.7 * 1.2 * 1024 * 6) // TW + 2)), (F, N, rows, full)
                for r in {rows, max(rows // 3, 1), 1}:
                    p = _ddc_plan.plan(gsdr_lib, N, 100, F, 100 * rows, rows=r, env=FLAT)
                    c, want = p["chunks"], p["chunks_want"]
                    assert 1 <= c <= p["tails_nch"] and (c == 1 or r // c >= F - 1), (F, N, rows, r, p)
                    rcap = max(1, min(r // (F - 1) if F > 1 else r, p["tails_nch"]))
                    if want <= rcap:
                        assert want - want // 5 <= c <= want + want // 5, (F, N, rows, r, p)
                    else:
                        assert rcap - rcap // 5 <= c <= rcap, (F, N, rows, r, p)
                    for nch in (1, 5, 777, 10 ** 6):
                        q = _ddc_plan.plan(gsdr_lib, N, 100, F, 100 * rows, rows=r, env=dict(FLAT, GSDR_DDC_NCH=str(nch)))
                        rc = max(1, r // (F - 1) if F > 1 else r)
                        assert q["chunks"] == max(1, min(nch, rc, q["tails_nch"])), (F, N, rows, r, nch, q)
    # the most even split near the wanted count: 100 000 blocks in 7987 chunks leave some of 12 blocks beside those of
    # 13 (balance 0.963); 7693 chunks are of 13 blocks but for the last (0.9999), 294 chunks off (score -0.0018)
    p = _ddc_plan.plan(gsdr_lib, 8, 100, 4, 100 * 100_000, env=FLAT)
    assert (p["chunks_want"], p["chunks"]) == (7987, 7693)
    # the generic kernel and GSDR_DDC_WAVES_PER_SIMD
    assert _ddc_plan.plan(gsdr_lib, 8, 100, 5, 100 * 1000, env=FLAT)["target_waves"] == 1024 * 4
    assert _ddc_plan.plan(gsdr_lib, 8, 100, 4, 100 * 1000, env=dict(FLAT, GSDR_DDC_WAVES_PER_SIMD="3"))["target_waves"] == 1024 * 3
    assert _ddc_plan.plan(gsdr_lib, 8, 100, 4, 100 * 1000, env=dict(FLAT, GSDR_DDC_WAVES_PER_SIMD="-1"))["target_waves"] == 1024 * 4
    assert _ddc_plan.plan(gsdr_lib, 8, 100, 4, 100 * 1000, cus=64, env=FLAT)["target_waves"] == 256 * 6
