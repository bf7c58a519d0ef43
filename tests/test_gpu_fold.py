"""The folded three-product matrix-core DDC (ddc_convert3f_kernel + ddc_mfma_ring16p3f_kernel, DESIGN.md section
4.1f; switch GSDR_MFMA_FOLD): the even and odd sums of each 64-sample span over 32 partner pairs.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  The
cases every product loop runs are in tests/test_gpu_product_loops.py; the comb and the helpers are those of
tests/test_gpu_parity.py, test_gpu_extents.py and tests/_product_loops.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from _product_loops import (_c3_handle, COMMON, direct_parity, every_entry_is_bit_identical,
                            extreme_and_nonfinite_samples, EXTREME_KINDS, EXTREME_SHAPES, force, _hdr_errors,
                            _HDR_REFS, KERNEL, shape_id)
from test_gpu_extents import clean_env
from test_gpu_parity import DIRECT_CASES, make_direct, TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", DIRECT_CASES, ids=shape_id)
def test_direct_parity_fold(cuda_device, gsdr_lib, oracle_mod, monkeypatch, case):
    """The parity sweep every product loop runs (direct_parity of tests/_product_loops.py), ddc_mfma_ring16p3f_kernel
    forced."""
    force(monkeypatch, "p3f")
    direct_parity(cuda_device, oracle_mod, "p3f", case)


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("shape", list(EXTREME_SHAPES))
def test_extreme_and_nonfinite_samples_fold(cuda_device, gsdr_lib, oracle_mod, monkeypatch, kind, shape):
    """The extreme and non-finite samples every product loop runs (tests/_product_loops.py), ddc_mfma_ring16p3f_kernel
    forced."""
    force(monkeypatch, "p3f")
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, "p3f", kind, shape)


def _c3_default(monkeypatch):
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD"):
        monkeypatch.delenv(k, raising=False)
    d, _ = _c3_handle()
    info = d.describe()
    d.close()
    return info["fold"], info["fold_min_blocks"]


@pytest.mark.parametrize("fold_env", [None, "1"], ids=["default", "fold"])
def test_c3_is_bit_identical_through_every_entry_fold(cuda_device, gsdr_lib, monkeypatch, fold_env):
    """C3 by default (the loop its handle chose, reported and recorded) and with the fold forced: process_device on
    two caller streams, submit_device in between, the synchronous host entry -- bit-equal to one in-order stream."""
    fold, T = _c3_default(monkeypatch)
    assert fold == (1 if T <= 125 else 0), (fold, T)
    record_info(fold, "C3 by default: fold")
    if fold_env:
        force(monkeypatch, "p3f")
        fold = int(fold_env)

    def same(d):
        i = d.describe()
        return d.kernel_name == KERNEL and (i["complex_mac"], i["rotation_blocks"], i["fold"]) == (3, 2, fold)

    every_entry_is_bit_identical(cuda_device, same)


def test_switch_and_threshold_fold(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_FOLD: 0 never, 1 wherever the handle is three-product and rotates per pair, unset from
    fold_min_blocks on; a handle that rotates per block (GSDR_MFMA_3M_ROT=1) and four-product handles are not touched;
    complex_mac and rotation_blocks are what they were."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def fold(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["fold"], i["fold_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    T = fold(1000)[3]
    assert T in (94, 125, 250), T
    above, below = T * 8, (T - 1) * 8                     # windows of exactly T and of T - 1 blocks
    assert fold(above)[:3] == (3, 2, 1)
    assert fold(2000)[:3] == (3, 2, 1)
    assert fold(above, GSDR_MFMA_FOLD="0")[:3] == (3, 2, 0)
    assert fold(above, GSDR_MFMA_FOLD="1")[:3] == (3, 2, 1)
    assert fold(above, GSDR_MFMA_3M_ROT="1")[:3] == (3, 1, 0)
    assert fold(above, GSDR_MFMA_3M_ROT="1", GSDR_MFMA_FOLD="1")[:3] == (3, 1, 0)
    assert fold(above, GSDR_MFMA_3M="0", GSDR_MFMA_FOLD="1")[:3] == (4, 1, 0)
    # below the threshold: never by itself, forced where the handle rotates per pair
    assert fold(below)[2] == 0
    assert fold(below, GSDR_MFMA_FOLD="0")[2] == 0
    assert fold(256, GSDR_MFMA_3M="1")[:3] == (3, 1, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_FOLD="1")[:3] == (3, 1, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2")[:3] == (3, 2, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="1")[:3] == (3, 2, 1)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="0")[:3] == (3, 2, 0)


HDR_FOLD_DECIMS = [750, 1000, 2000]        # windows of 94, 125, 250 blocks


def _fold_of(M):
    """describe()["fold"], ["fold_min_blocks"] of the handle _hdr_errors makes for decimation M under the environment as it is."""
    freq, _ = _HDR_REFS[(60, M)]
    dem = make_direct(freq, 200_000_000, M, 4, 200 * M)
    d = dem.describe()
    dem.close()
    return d["fold"], d["fold_min_blocks"]


def test_hdr_comb_fold_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """The measurement behind kFoldMinBlocks (csrc/ddc_plan.h): the 60 dB comb of test_gpu_mfma3.py (64 tones at
    200 Msps, F = 4, L = 200 * M, pre-converted operands forced), windows of 94, 125, 250 blocks, three buffers.
    Rule, per tone: err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) against the fp64 oracle on the same buffers.  Asserted for GSDR_MFMA_FOLD unset
    at every length; the figures of both loops forced (FOLD = 0, = 1) are recorded."""
    span_db = 60
    failures = []
    for M in HDR_FOLD_DECIMS:
        res = {}
        for mode in ("0", "1", None):
            if mode is None:
                clean_env(monkeypatch, COMMON)
            else:
                force(monkeypatch, {"0": "p3r2", "1": "p3f"}[mode])
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
            assert res[mode][2] == 3, (M, mode)
            fold, T = _fold_of(M)            # the switch was heard
            assert fold == {"0": 0, "1": 1, None: int((4 * M + 31) // 32 >= T)}[mode], (M, mode, fold, T)
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio = res["1"][0] / np.maximum(res["0"][0], 1e-12)
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound plain {worst['0']:.3f} folded {worst['1']:.3f} "
              f"default {worst[None]:.3f}; worst err plain {res['0'][0].max():.3e} folded {res['1'][0].max():.3e} "
              f"fp32 order {err32.max():.3e}; per-tone ratio folded/plain median {np.median(ratio):.2f} max {ratio.max():.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default")
        for m, name in (("0", "pair rotation, not folded"), ("1", "folded"), (None, "default")):
            record_info(float(res[m][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, {name}")
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(float(np.median(ratio)), f"{span_db} dB, M {M} ({nblk} blocks): median per-tone ratio folded / plain")
        record_info(float(ratio.max()), f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio folded / plain")
        if worst[None] > 1.0:
            failures.append((M, worst[None]))
    assert not failures, failures
