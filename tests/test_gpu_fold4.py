"""The direct folded matrix-core DDC (ddc_convert4f_kernel + ddc_mfma_ring16p4f_kernel, DESIGN.md section 4.1g;
switch GSDR_MFMA_FOLD_PRODUCTS): the plain four products of each 64-sample span folded over 32 partner pairs and
summed straight into Re and Im.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  The
cases every product loop runs are in tests/test_gpu_product_loops.py; the comb and the helpers are those of
tests/test_gpu_parity.py, test_gpu_extents.py and tests/_product_loops.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from _product_loops import COMMON, extreme_and_nonfinite_samples, force, _hdr_errors, _HDR_REFS
from test_gpu_extents import clean_env
from test_gpu_parity import TOL, make_direct

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", ["M100", "M90pad"])
def test_extreme_and_nonfinite_samples_fold4(cuda_device, gsdr_lib, oracle_mod, monkeypatch, kind, shape):
    """The extreme and non-finite samples every product loop runs (tests/_product_loops.py), ddc_mfma_ring16p4f_kernel
    forced."""
    force(monkeypatch, "p4f")
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, "p4f", kind, shape)


def test_switch_fold_products(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_FOLD_PRODUCTS: 3 the Gauss fold, 4 the direct fold, on every folded handle; a handle that is not
    folded (GSDR_MFMA_FOLD=0, a rotation per block, four products per block, a window below fold_min_blocks) reports
    0, and complex_mac, rotation_blocks and fold are what they were."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD", "GSDR_MFMA_FOLD_PRODUCTS"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def info(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["fold"], i["fold_products"], i["fold_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    T = info(1000)[4]
    assert T == 94
    above, below = T * 8, (T - 1) * 8                     # windows of exactly T and of T - 1 blocks
    default = info(above)
    assert default[:3] == (3, 2, 1) and default[3] in (3, 4)
    record_info(default[3], "fold_products of a folded handle by default")
    assert info(above, GSDR_MFMA_FOLD_PRODUCTS="3")[:4] == (3, 2, 1, 3)
    assert info(above, GSDR_MFMA_FOLD_PRODUCTS="4")[:4] == (3, 2, 1, 4)
    for p in ("3", "4"):
        assert info(above, GSDR_MFMA_FOLD="0", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (3, 2, 0, 0)
        assert info(above, GSDR_MFMA_3M_ROT="1", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (3, 1, 0, 0)
        assert info(above, GSDR_MFMA_3M="0", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (4, 1, 0, 0)
        assert info(below, GSDR_MFMA_FOLD_PRODUCTS=p)[2:4] == (0, 0)
    assert info(below)[2:4] == (0, 0)
    # forced below the threshold: the switch is heard there too
    forced = dict(GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="1")
    assert info(256, **forced, GSDR_MFMA_FOLD_PRODUCTS="4")[:4] == (3, 2, 1, 4)
    assert info(256, **forced, GSDR_MFMA_FOLD_PRODUCTS="3")[:4] == (3, 2, 1, 3)


HDR_ASSERTED = [750, 1000, 2000]           # windows of 94, 125, 250 blocks: the rule is asserted
HDR_RECORDED = [256, 375, 500]             # 32, 47, 63 blocks, the fold forced: recorded only


def _products_of(M):
    freq, _ = _HDR_REFS[(60, M)]
    dem = make_direct(freq, 200_000_000, M, 4, 200 * M)
    d = dem.describe()
    dem.close()
    return d["fold"], d["fold_products"]


@pytest.mark.parametrize("M", HDR_ASSERTED + HDR_RECORDED)
def test_hdr_comb_fold4_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch, M):
    """The 60 dB comb of test_gpu_mfma3.py (64 tones at 200 Msps, F = 4, L = 200 * M, pre-converted operands forced),
    three buffers.  Rule of DESIGN.md section 4.1d, per tone: err <= max(1e-5, 3 x err32), err32 the error of the
    reference's own fp32 order of operations against the fp64 oracle on the same buffers.  Asserted at 94, 125 and 250
    blocks for GSDR_MFMA_FOLD_PRODUCTS unset and = 4; the Gauss fold's figures (= 3) and the per-tone ratio 4 / 3 are
    recorded, and so are 32, 47 and 63 blocks with the fold forced (what a later change of the thresholds would rest
    on; nothing is asserted of them)."""
    span_db = 60
    asserted = M in HDR_ASSERTED
    nblk = (4 * M + 31) // 32
    res = {}
    for mode in (("3", "4", None) if asserted else ("3", "4")):
        if mode is None:
            clean_env(monkeypatch, COMMON)
        else:
            force(monkeypatch, {"3": "p3f", "4": "p4f"}[mode])
        res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
        assert res[mode][2] == 3, (M, mode)
        fold, products = _products_of(M)           # the switch was heard
        assert fold == 1 and (products == int(mode) if mode else products in (3, 4)), (M, mode, fold, products)
    err32 = res["4"][1]
    bound = np.maximum(TOL, 3.0 * err32)
    worst = {m: float((res[m][0] / bound).max()) for m in res}
    ratio = res["4"][0] / np.maximum(res["3"][0], 1e-12)
    _HDR_REFS.pop((span_db, M), None)
    print(f"hdr {span_db} dB M {M} ({nblk} blocks, {'asserted' if asserted else 'recorded'}): err/bound "
          + " ".join(f"{m or 'default'} {worst[m]:.3f}" for m in res)
          + f"; worst err 3: {res['3'][0].max():.3e} 4: {res['4'][0].max():.3e} fp32 order {err32.max():.3e}; "
          f"per-tone ratio 4/3 median {np.median(ratio):.2f} max {ratio.max():.2f}")
    if asserted:
        record_margin(float(res["4"][0][:, :32].max()), "strong half, direct fold")
    for m in res:
        name = {"3": "Gauss fold", "4": "direct fold", None: "default"}[m]
        record_info(float(res[m][0].max()), f"{nblk} blocks: worst per-tone error, {name}")
        record_info(worst[m], f"{nblk} blocks: worst err / bound, {name}")
    record_info(float(np.median(ratio)), f"{nblk} blocks: median per-tone ratio direct / Gauss")
    record_info(float(ratio.max()), f"{nblk} blocks: largest per-tone ratio direct / Gauss")
    if asserted:
        failures = [(M, m, worst[m]) for m in ("4", None) if worst[m] > 1.0]
        assert not failures, failures
