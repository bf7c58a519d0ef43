"""The three-product matrix-core DDC with one rotation per PAIR of blocks (ddc_convert3_kernel +
ddc_mfma_ring16p3r2_kernel; switch GSDR_MFMA_3M_ROT).

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin
file.  The cases every product loop runs are in tests/test_gpu_product_loops.py; the comb and the helpers are those of
tests/test_gpu_parity.py and tests/_product_loops.py."""
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
def test_direct_parity_pair_rotation(cuda_device, gsdr_lib, oracle_mod, monkeypatch, case):
    """The parity sweep every product loop runs (direct_parity of tests/_product_loops.py), ddc_mfma_ring16p3r2_kernel
    forced."""
    force(monkeypatch, "p3r2")
    direct_parity(cuda_device, oracle_mod, "p3r2", case)


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("shape", list(EXTREME_SHAPES))
def test_extreme_and_nonfinite_samples_pair_rotation(cuda_device, gsdr_lib, oracle_mod, monkeypatch, kind, shape):
    """The extreme and non-finite samples every product loop runs (tests/_product_loops.py), ddc_mfma_ring16p3r2_kernel
    forced."""
    force(monkeypatch, "p3r2")
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, "p3r2", kind, shape)


def _c3_default_rotation(monkeypatch):
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    d, _ = _c3_handle()
    info = d.describe()
    d.close()
    return info["rotation_blocks"], info["rotation_min_blocks"]


@pytest.mark.parametrize("rot_env", [None, "2"], ids=["default", "pair"])
def test_c3_is_bit_identical_through_every_entry(cuda_device, gsdr_lib, monkeypatch, rot_env):
    """C3 by default (the loop its handle chose, reported and recorded) and with the pair rotation forced:
    process_device on two caller streams, submit_device in between, the synchronous host entry -- bit-equal to one
    in-order stream."""
    rot, T = _c3_default_rotation(monkeypatch)
    assert rot == (2 if T <= 125 else 1), (rot, T)
    record_info(rot, "C3 by default: blocks per rotation")
    if rot_env:
        force(monkeypatch, "p3r2")
        rot = int(rot_env)

    def same(d):
        i = d.describe()
        return d.kernel_name == KERNEL and i["complex_mac"] == 3 and i["rotation_blocks"] == rot

    every_entry_is_bit_identical(cuda_device, same)


def test_switch_and_threshold(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_3M_ROT: 1 never, 2 wherever the handle is three-product, unset from rotation_min_blocks on; a handle
    forced to three products on a short window keeps the 32-sample loop; four-product handles are not touched."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def rot(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["rotation_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    _, _, T = rot(1000)
    assert T in (94, 125, 250), T
    assert rot(1000, GSDR_MFMA_3M_ROT="1")[:2] == (3, 1)
    assert rot(1000, GSDR_MFMA_3M_ROT="2")[:2] == (3, 2)
    assert rot(2000)[:2] == (3, 2)
    assert rot(T * 8)[:2] == (3, 2)                       # a window of exactly T blocks
    assert rot(256, GSDR_MFMA_3M="1")[:2] == (3, 1)       # forced three products on 32 blocks: today's loop
    assert rot(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2")[:2] == (3, 2)
    assert rot(1000, GSDR_MFMA_3M="0", GSDR_MFMA_3M_ROT="2")[:2] == (4, 1)
    if T > 94:
        assert rot(750)[:2] == (3, 1)


HDR_R2_DECIMS = [750, 1000, 2000]        # windows of 94, 125, 250 blocks


def test_hdr_comb_default_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """The measurement behind kRot2MinBlocks (csrc/ddc_plan.h): the 60 dB comb of test_gpu_mfma3.py
    (64 tones at 200 Msps, F = 4, L = 200 * M, pre-converted operands forced), windows of 94, 125, 250 blocks.
    Rule, per tone: err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) against the fp64 oracle on the same buffers.  Asserted for GSDR_MFMA_3M_ROT unset
    at every length; the figures of both loops forced (ROT = 1, = 2) are recorded."""
    span_db = 60
    failures = []
    for M in HDR_R2_DECIMS:
        res = {}
        for mode in ("1", "2", None):
            if mode is None:
                clean_env(monkeypatch, COMMON)
            else:
                force(monkeypatch, {"1": "p3", "2": "p3r2"}[mode])
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
            assert res[mode][2] == 3, (M, mode)
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio = res["2"][0] / np.maximum(res["1"][0], 1e-12)
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound per block {worst['1']:.3f} per pair {worst['2']:.3f} "
              f"default {worst[None]:.3f}; worst err per block {res['1'][0].max():.3e} per pair {res['2'][0].max():.3e} "
              f"fp32 order {err32.max():.3e}; per-tone ratio pair/block median {np.median(ratio):.2f} max {ratio.max():.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default rotation")
        for m, name in (("1", "rotation per block"), ("2", "rotation per pair"), (None, "default")):
            record_info(float(res[m][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, {name}")
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(float(np.median(ratio)), f"{span_db} dB, M {M} ({nblk} blocks): median per-tone ratio pair / block")
        record_info(float(ratio.max()), f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio pair / block")
        if worst[None] > 1.0:
            failures.append((M, worst[None]))
    assert not failures, failures


def test_c3_full_size_margin(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """C3 against the oracle through the default loop of its handle: the margin to record beside the 4.0e-7 of the
    32-sample loop."""
    from test_gpu_parity import _full_size_direct, DIRECT_CASES
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    _full_size_direct(cuda_device, oracle_mod, N=2048, M=1000, nbuf=3, subset=12)
