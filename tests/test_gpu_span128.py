"""The direct folded matrix-core DDC on wave tiles of 16 rows x 64 tones over spans of 128 samples
(ddc_convert4f2_kernel + ddc_mfma_ring16p4fw2_kernel; switch GSDR_MFMA_SPAN): the products of
128 samples, folded about the centre of the span over 64 partner pairs, are rotated into the accumulators at once.

The loop is forced with the environment of the wide tile (every selecting switch set) and GSDR_MFMA_SPAN=128, and the
handle's span_samples is asserted before the first call and after the last.  Every case compares against the fp64
oracle, bar 1e-5 per tone, over three consecutive buffers (the head and the tail are carried across calls).  The
helpers and the forced loops are those of test_gpu_parity.py, test_gpu_extents.py and tests/_product_loops.py."""
import json
import os

import numpy as np
import pytest

from _margins import record_info, record_margin
from _product_loops import (DESCRIBE, EXTREME_KINDS, EXTREME_SHAPES, KERNEL, LOOPS, _HDR_REFS, _hdr_errors,
                            dynamic_range_and_scale_carry, extreme_and_nonfinite_samples, pipelined_fuzz)
import _product_loops
from test_gpu_extents import S_C3, S_N65, S_ODD, TONES_SHAPE, clean_env, direct_inputs, run_case, run_tones
from test_gpu_parity import TOL, crandn, make_direct, rel_err_per_tone, run_device, run_host

pytestmark = pytest.mark.gpu

WIDE_ENV = LOOPS["p4fw"][0]
SPAN128_ENV = dict(WIDE_ENV, GSDR_MFMA_SPAN="128")
SPAN64_ENV = dict(WIDE_ENV, GSDR_MFMA_SPAN="64")


def is_span(dem, span=128):
    """`dem` is a handle of the wide tile (kernel name and the five-tuple) with spans of `span` samples."""
    d = dem.describe()
    assert (dem.kernel_name, tuple(d[k] for k in DESCRIBE), d["span_samples"]) == (KERNEL, LOOPS["p4fw"][1], span), d
    return True


def _check(dem, ran):
    return is_span(dem)


@pytest.fixture
def span128(monkeypatch):
    clean_env(monkeypatch, SPAN128_ENV)


def _three_buffers(cuda_device, oracle_mod, N, rate, M, F, L, seed, host_too=False):
    rng = np.random.default_rng(seed)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    is_span(dem)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    worst = 0.0
    for c in range(3):
        x = crandn(rng, L)
        y = run_host(dem, x) if host_too and c % 2 else run_device(dem, x, cuda_device)
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M), (c, y.size, yr.size)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        worst = max(worst, float(err.max()))
        assert err.max() <= TOL, (c, float(err.max()))
    is_span(dem)
    dem.close()
    record_margin(worst)
    return worst


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5, 7, 8, 9, 13, 17])
def test_windows(cuda_device, gsdr_lib, oracle_mod, span128, blocks):
    """Every nblk mod 4, windows shorter than one span (1, 2, 3), the three-slot prologue longer (1 .. 9 blocks: up to
    three spans) and shorter (13, 17) than the window, both exits of the trip (1, 3 and 5 spans against 2 and 4), a last
    span of one block (1, 5, 9, 13, 17).  65 tones, 40 rows."""
    M, F = 8 * blocks, 4
    worst = _three_buffers(cuda_device, oracle_mod, 65, 1_000_000, M, F, 40 * M, 1300 + blocks)
    print(f"{blocks} blocks: worst per-tone error {worst:.3e}")


def test_window_no_multiple_of_32(cuda_device, gsdr_lib, oracle_mod, span128):
    """M = 90, F = 4: 360 samples, 12 blocks of which the last holds 8 samples."""
    worst = _three_buffers(cuda_device, oracle_mod, 65, 9_000_000, 90, 4, 40 * 90, 1390, host_too=True)
    print(f"M 90: worst per-tone error {worst:.3e}")


@pytest.mark.parametrize("N", [1, 33, 65, 257, 288])
def test_tones(cuda_device, gsdr_lib, oracle_mod, span128, N):
    """A second tile that is absent (1, 65) or partly filled (33, 257), a second workgroup with one live wave and three
    idle ones (257, 288); windows of 3 blocks, 40 rows."""
    M, F = 24, 4
    worst = _three_buffers(cuda_device, oracle_mod, N, 1_000_000, M, F, 40 * M, 1400 + N)
    print(f"{N} tones: worst per-tone error {worst:.3e}")


@pytest.mark.parametrize("nout", [1, 8, 17, 40, 130])
def test_rows(cuda_device, gsdr_lib, oracle_mod, span128, nout):
    """A lone half tile (1, 8), short last tiles in either half (17, 40, 130), nine 16-row tiles (130).  65 tones,
    windows of 3 blocks (M = 48, F = 2: a buffer of one row still holds the carry)."""
    M, F = 48, 2
    worst = _three_buffers(cuda_device, oracle_mod, 65, 1_000_000, M, F, nout * M, 1500 + nout)
    print(f"{nout} rows: worst per-tone error {worst:.3e}")


def test_one_handle_every_entry(cuda_device, gsdr_lib, oracle_mod, span128):
    """One handle, one loop: process_device, submit_device / wait and the host entry give the same bits for the same
    buffers (288 tones, M 1000, F 4, L 200 000: 125 blocks, 200 rows), within TOL of the oracle."""
    import torch
    from gpu_sdr_amd.source import tone_comb
    N, rate, M, F, L = 288, 200_000_000, 1000, 4, 200_000
    freq, _, _ = tone_comb(N, rate, seed=44)
    rng = np.random.default_rng(444)
    xs = [crandn(rng, L) for _ in range(3)]
    got = {}
    for entry in ("process", "submit", "host"):
        dem = make_direct(freq, rate, M, F, L)
        is_span(dem)
        ys = []
        for x in xs:
            if entry == "host":
                ys.append(run_host(dem, x))
                continue
            xin = torch.from_numpy(x).to(cuda_device)
            out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
            if entry == "submit":
                dem.submit_device(xin, out)
                n = dem.wait()
            else:
                n = dem.process_device(xin, out)
            torch.cuda.synchronize()
            ys.append(out[:n].cpu().numpy())
        is_span(dem)
        dem.close()
        got[entry] = ys
    for entry in ("submit", "host"):
        for k, (y, w) in enumerate(zip(got[entry], got["process"])):
            assert y.size == w.size == N * (L // M), (entry, k)
            np.testing.assert_array_equal(y.view(np.int32), w.view(np.int32), err_msg=f"buffer {k} via {entry}")
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for k, x in enumerate(xs):
        err = rel_err_per_tone(got["process"][k].reshape(-1, N), ref.process(x))
        record_margin(float(err.max()), f"buffer {k}")
        assert err.max() <= TOL, (k, float(err.max()))


@pytest.fixture
def as_p4fw(monkeypatch):
    """The shared bodies assert is_loop(dem, name): under this fixture the row "p4fw" also asks for 128-sample spans."""
    def is_loop(dem, name):
        assert name == "p4fw"
        return is_span(dem)
    monkeypatch.setattr(_product_loops, "is_loop", is_loop)


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("shape", list(EXTREME_SHAPES))
def test_extreme_and_nonfinite_samples(cuda_device, gsdr_lib, oracle_mod, span128, as_p4fw, kind, shape):
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, "p4fw", kind, shape)


def test_dynamic_range_and_scale_carry(cuda_device, gsdr_lib, oracle_mod, span128):
    dynamic_range_and_scale_carry(cuda_device, oracle_mod, _check)


def test_pipelined_fuzz(cuda_device, gsdr_lib, span128):
    pipelined_fuzz(cuda_device, _check, "span128")


@pytest.mark.parametrize("shape", [S_N65, S_ODD, S_C3], ids=_product_loops.shape_id)
def test_direct_extents(cuda_device, gsdr_lib, oracle_mod, span128, shape):
    """The guard zones of tests/_extents.py around input and output, through process_device and submit_device: 12.5
    blocks (a last span of one block), 185 samples (two spans, the second of two blocks), the C3 block (125 blocks)."""
    N, rate, M, F, L = shape
    freq, xs, yrs = direct_inputs(shape, oracle_mod)
    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), _check, xs, yrs, N)


def test_tones_extents_on_the_ddc_kernels(cuda_device, gsdr_lib, oracle_mod, span128):
    run_tones(cuda_device, _check, *TONES_SHAPE, oracle_mod)


HDR_ASSERTED = [750, 1000, 2000]           # windows of 94, 125, 250 blocks: the rule is asserted
HDR_RECORDED = [256, 375, 500]             # 32, 47, 63 blocks: recorded only
_HDR_FIGURES = {}
HDR_RECORD = os.environ.get("SPAN128_MARGINS")     # where the figures of the comb are written beside the margin file; unset: nowhere


@pytest.mark.parametrize("M", HDR_ASSERTED + HDR_RECORDED)
def test_hdr_comb_span128_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch, M):
    """The 60 dB comb of test_hdr_comb_fold4_keeps_the_rule (64 tones at 200 Msps, F = 4, L = 200 * M, the wide tile
    forced), three buffers.  Rule of DESIGN.md section 4.1d, per tone: err <= max(1e-5, 3 x err32), err32 the error of
    the reference's own fp32 order against the fp64 oracle on the same buffers.  Asserted at 94, 125 and 250 blocks for
    128-sample spans; the 64-sample loop's figures on the same buffers are recorded beside them, and so are 32, 47
    and 63 blocks (nothing is asserted of them)."""
    span_db, asserted, nblk = 60, M in HDR_ASSERTED, (4 * M + 31) // 32
    res = {}
    for span, env in ((64, SPAN64_ENV), (128, SPAN128_ENV)):
        clean_env(monkeypatch, env)
        freq, _ = _product_loops._hdr_refs(oracle_mod, span_db, M)
        dem = make_direct(freq, 200_000_000, M, 4, 200 * M)
        is_span(dem, span)
        dem.close()
        res[span] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
    _HDR_REFS.pop((span_db, M), None)
    err32 = res[128][1]
    bound = np.maximum(TOL, 3.0 * err32)
    worst = {s: float((res[s][0] / bound).max()) for s in res}
    ratio = res[128][0] / np.maximum(res[64][0], 1e-12)
    print(f"hdr {span_db} dB M {M} ({nblk} blocks, {'asserted' if asserted else 'recorded'}): err/bound 64: {worst[64]:.3f} "
          f"128: {worst[128]:.3f}; worst err 64: {res[64][0].max():.3e} 128: {res[128][0].max():.3e} fp32 order "
          f"{err32.max():.3e}; per-tone ratio 128/64 median {np.median(ratio):.2f} max {ratio.max():.2f}")
    for s in res:
        record_info(float(res[s][0].max()), f"{nblk} blocks: worst per-tone error, {s}-sample spans")
        record_info(worst[s], f"{nblk} blocks: worst err / bound, {s}-sample spans")
    _HDR_FIGURES[str(nblk)] = {"asserted": asserted, "fp32_order_worst_err": float(err32.max()),
                               **{f"span{s}": {"worst_err": float(res[s][0].max()), "worst_err_over_bound": worst[s]} for s in res},
                               "ratio_128_over_64_median": float(np.median(ratio)), "ratio_128_over_64_max": float(ratio.max())}
    if HDR_RECORD:          # SPAN128_MARGINS=<file>: the table of profiles/span128_parity_margins.json
        try:
            with open(HDR_RECORD, "w") as fh:
                json.dump({"comb_dB": span_db, "rule": "per tone err <= max(1e-5, 3 x err32)", "blocks": _HDR_FIGURES}, fh, indent=1)
        except OSError:
            pass
    if asserted:
        record_margin(float(res[128][0][:, :32].max()), "strong half, 128-sample spans")
        assert worst[128] <= 1.0, (M, worst[128])


def test_span_64_gives_the_bytes_of_the_wide_tile(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_SPAN=64 beside the p4fw environment: the same handle, the same bytes (one window, one tone and one
    row case: 5 blocks, 65 tones, 40 rows)."""
    N, rate, M, F = 65, 1_000_000, 40, 4
    L = 40 * M
    rng = np.random.default_rng(6464)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    xs = [crandn(rng, L) for _ in range(3)]
    got = []
    for env in (WIDE_ENV, SPAN64_ENV):
        clean_env(monkeypatch, env)
        dem = make_direct(freq, rate, M, F, L)
        is_span(dem, 64)
        got.append([run_device(dem, x, cuda_device) for x in xs])
        is_span(dem, 64)
        dem.close()
    for k, (a, b) in enumerate(zip(*got)):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=f"buffer {k}")


def test_switch_span(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_SPAN: 128 on every handle the wide tile takes and on no other; 64 never; unset, a handle whose wave
    tile was forced keeps the 64-sample spans, and one that took the wide tile by its own rule has 128-sample spans from
    span128_min_blocks blocks on (0: never)."""
    from gpu_sdr_amd.source import tone_comb
    rate, M, F, L = 200_000_000, 1000, 4, 40_000
    free = {k: v for k, v in WIDE_ENV.items() if k != "GSDR_MFMA_WAVE_TONES"}

    def span_of(N, env, M=M):
        clean_env(monkeypatch, env)
        freq, _, _ = tone_comb(N, rate, seed=1)
        d = make_direct(freq, rate, M, F, 40 * M)
        i = d.describe()
        d.close()
        return i["wave_tones"], i["span_samples"], i["span128_min_blocks"]

    T = span_of(288, WIDE_ENV)[2]
    assert span_of(288, WIDE_ENV)[:2] == (64, 64)                      # a forced tile keeps its bits
    assert span_of(288, SPAN128_ENV)[:2] == (64, 128)
    assert span_of(288, SPAN64_ENV)[:2] == (64, 64)
    assert span_of(288, dict(free, GSDR_MFMA_SPAN="128"))[:2] == (64, 128)
    assert span_of(64, dict(free, GSDR_MFMA_SPAN="128"))[:2] == (32, 64)          # the 32 x 32 tile by the wave rule
    assert span_of(288, dict(LOOPS["p4f"][0], GSDR_MFMA_SPAN="128"))[:2] == (32, 64)
    assert span_of(288, dict(LOOPS["p3f"][0], GSDR_MFMA_SPAN="128"))[:2] == (32, 64)
    assert span_of(288, dict(free, GSDR_MFMA_SPAN="64"))[:2] == (64, 64)
    assert span_of(288, free)[:2] == (64, 128 if 0 < T <= 125 else 64)
    if T > 1:
        assert span_of(288, free, M=8 * (T - 1))[:2] == (64, 64)
        assert span_of(288, free, M=8 * T)[:2] == (64, 128)
    record_info(T, "span128_min_blocks")
