"""Three real products per complex multiply on the pre-converted matrix-core DDC
(ddc_convert3_kernel + ddc_mfma_ring16p3_kernel; switch GSDR_MFMA_3M).

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the
margin file.  The cases every product loop runs are in tests/test_gpu_product_loops.py; the comb and the helpers are
those of tests/test_gpu_parity.py and tests/_product_loops.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from _product_loops import (C3, _c3_handle, COMMON, direct_parity, every_entry_is_bit_identical,
                            extreme_and_nonfinite_samples, EXTREME_KINDS, EXTREME_SHAPES, force, _hdr_errors,
                            _HDR_REFS, KERNEL, shape_id)
from test_gpu_extents import clean_env
from test_gpu_parity import crandn, DIRECT_CASES, make_direct, TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", DIRECT_CASES, ids=shape_id)
def test_direct_parity_three_products(cuda_device, gsdr_lib, oracle_mod, monkeypatch, case):
    """The parity sweep every product loop runs (direct_parity of tests/_product_loops.py), ddc_mfma_ring16p3_kernel
    forced."""
    force(monkeypatch, "p3")
    direct_parity(cuda_device, oracle_mod, "p3", case)


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("shape", list(EXTREME_SHAPES))
def test_extreme_and_nonfinite_samples_three_products(cuda_device, gsdr_lib, oracle_mod, monkeypatch, kind, shape):
    """The extreme and non-finite samples every product loop runs (tests/_product_loops.py), ddc_mfma_ring16p3_kernel
    forced."""
    force(monkeypatch, "p3")
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, "p3", kind, shape)


def test_one_handle_is_bit_identical_through_every_entry(cuda_device, gsdr_lib, monkeypatch):
    """(c) A shape that is three-product by default (C3 itself): process_device on two caller streams,
    submit_device in between, the synchronous host entry -- bit-equal to one in-order stream."""
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    monkeypatch.delenv("GSDR_MFMA_PREC", raising=False)
    every_entry_is_bit_identical(cuda_device, lambda d: d.describe()["complex_mac"] == 3 and d.kernel_name == KERNEL)


def test_switch_and_threshold(cuda_device, gsdr_lib, monkeypatch):
    """(d) GSDR_MFMA_3M=0 gives the four-product kernels of before (ring16w8 in order, ring16p overlapped on
    C3); a window one block shorter than the threshold stays on four products by default."""
    import torch
    monkeypatch.delenv("GSDR_MFMA_PREC", raising=False)
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    N, rate, M, F, L = C3
    d, _ = _c3_handle()
    T = d.describe()["complex_mac_min_blocks"]
    d.close()
    monkeypatch.setenv("GSDR_MFMA_3M", "0")
    d, _ = _c3_handle()
    assert d.describe()["complex_mac"] == 4
    x = torch.from_numpy(crandn(np.random.default_rng(5), L)).to(cuda_device)
    out = torch.empty(d.out_capacity, dtype=torch.complex64, device=cuda_device)
    d.process_device(x, out)
    torch.cuda.synchronize()
    assert d.kernel_name == "ddc_mfma_ring16w8_kernel", d.kernel_name
    d.submit_device(x, out)
    d.wait()
    torch.cuda.synchronize()
    assert d.kernel_name == "ddc_mfma_ring16p_kernel" and d.describe()["complex_mac"] == 4
    d.close()
    monkeypatch.delenv("GSDR_MFMA_3M")
    if T * 32 % F == 0 and T > 1:
        M1 = (T - 1) * 32 // F               # a window of T-1 whole blocks
        d, _ = _c3_handle(M=M1)
        assert d.describe()["complex_mac"] == 4, (T, M1)
        d.close()
        d, _ = _c3_handle(M=T * 32 // F)
        assert d.describe()["complex_mac"] == 3, T
        d.close()


HDR_DECIMS = [256, 375, 500, 750, 1000, 2000]       # windows of 32, 47, 63, 94, 125, 250 blocks


@pytest.mark.parametrize("span_db", [60, 40])
def test_hdr_comb_sets_threshold(cuda_device, gsdr_lib, oracle_mod, monkeypatch, span_db):
    """(e) The measurement behind kMac3MinBlocks (csrc/ddc_plan.h).  64 tones spanning 40 / 60 dB at
    200 Msps, F = 4, L = 200 * M, windows of 32 ... 250 blocks, pre-converted operands forced.  Rule, per tone:
    err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) on the same buffers -- the rule of test_direct_high_dynamic_range_comb.
    Asserted for GSDR_MFMA_3M unset at every length; the forced figures (3M = 1, = 0) are recorded.
    A length at which the FOUR-product arithmetic itself misses the rule is recorded and left out (one at most)."""
    failures, left_out, T = [], [], None
    for M in HDR_DECIMS:
        res = {}
        for mode in ("1", "0", None):
            if mode == "1":
                force(monkeypatch, "p3")            # this file's loop at every length
            else:
                clean_env(monkeypatch, dict(COMMON, GSDR_MFMA_3M="0") if mode else COMMON)
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
        assert res["1"][2] == 3 and res["0"][2] == 4
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio34 = float((res["1"][0] / np.maximum(res["0"][0], 1e-12)).max())
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound three {worst['1']:.3f} four {worst['0']:.3f} "
              f"default {worst[None]:.3f} (complex_mac {res[None][2]}); worst err three {res['1'][0].max():.3e} "
              f"four {res['0'][0].max():.3e} fp32 order {err32.max():.3e}; per-tone ratio three/four up to {ratio34:.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default arithmetic")
        record_info(float(res["1"][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, three products")
        record_info(float(res["0"][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, four products")
        record_info(float(res[None][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, default (complex_mac {res[None][2]})")
        record_info(float(err32.max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error of the reference's fp32 order")
        for m, name in (("1", "three products"), ("0", "four products"), (None, "default")):
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(ratio34, f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio three / four products")
        if worst["0"] > 1.0:
            left_out.append((M, worst["0"]))
            continue
        if worst[None] > 1.0:
            failures.append((M, res[None][2], worst[None]))
        if M in (1000, 2000):
            T = T if T is not None else _threshold(monkeypatch)
            if T <= 125:
                assert res[None][2] == 3, (M, T)
    assert len(left_out) <= 1, left_out
    assert not failures, failures


def _threshold(monkeypatch):
    from gpu_sdr_amd.source import tone_comb
    freq, _, _ = tone_comb(64, 200_000_000, seed=1)
    d = make_direct(freq, 200_000_000, 1000, 4, 200_000)
    T = d.describe()["complex_mac_min_blocks"]
    d.close()
    return T


def test_c3_full_size_margin(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """C3 against the oracle through the default arithmetic of its handle (three products when the threshold
    allows): the margin to record beside the 3.3e-7 of the four-product loop."""
    from test_gpu_parity import _full_size_direct, DIRECT_CASES
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    _full_size_direct(cuda_device, oracle_mod, N=2048, M=1000, nbuf=3, subset=12)
