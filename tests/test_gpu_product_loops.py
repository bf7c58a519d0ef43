"""The cases every product loop of the pre-converted matrix-core DDC runs (DESIGN.md sections 4.1d - 4.1h): each stated
once, over all five loops of tests/_product_loops.py, each loop forced with every selecting switch set and asserted --
kernel name and the whole describe() tuple -- before the first call and after the last.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  What
is particular to one loop (switches and thresholds, the HDR combs, C3, wide against narrow bits) is in that loop's own
file."""
import numpy as np
import pytest

from _product_loops import (EXTREME_KINDS, EXTREME_SHAPES, LOOPS, VALU_CASES, direct_parity, extreme_and_nonfinite_samples, force,
                            is_loop, shape_id)
from test_gpu_parity import DIRECT_CASES, TOL, crandn, make_direct, make_pfb, rel_err_per_tone, run_device, run_host
from test_gpu_extents import S_C3, S_N65, S_ODD, TONES_SHAPE, direct_inputs, run_case, run_tones

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(LOOPS))
def loop(request, monkeypatch):
    force(monkeypatch, request.param)
    return request.param


def test_valu_cases_are_a_few():
    assert VALU_CASES <= set(DIRECT_CASES) and len(VALU_CASES) <= 3


@pytest.mark.parametrize("case", DIRECT_CASES, ids=shape_id)
def test_direct_parity(cuda_device, gsdr_lib, oracle_mod, loop, case):
    direct_parity(cuda_device, oracle_mod, loop, case)


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5])
def test_shortest_windows(cuda_device, gsdr_lib, oracle_mod, loop, blocks):
    """Windows of one to five blocks: a half-empty last span (1, 3, 5) or a whole one, with no, one and two whole
    spans in front; both exits of the trip."""
    N, rate, F = 40, 1_000_000, 4
    M = 8 * blocks                      # M * F = 32 * blocks
    L = 64 * M
    rng = np.random.default_rng(31 + blocks)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    is_loop(dem, loop)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"{loop} {blocks} blocks buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    is_loop(dem, loop)
    dem.close()


def test_window_no_multiple_of_32_or_64(cuda_device, gsdr_lib, oracle_mod, loop):
    """M = 90, F = 4: M * F = 360 is a multiple of neither 32 nor 64 (12 blocks, the last one 8 samples long)."""
    N, rate, M, F, L = 12, 9_000_000, 90, 4, 90_000
    rng = np.random.default_rng(90)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    is_loop(dem, loop)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        err = rel_err_per_tone(y.reshape(-1, N), ref.process(x))
        print(f"{loop} M 90 buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    is_loop(dem, loop)
    dem.close()


def test_tones_on_the_ddc_kernels(cuda_device, gsdr_lib, oracle_mod, loop):
    """TONES through the DDC kernels (the FFT path off), buffer length no multiple of nfft (short last batches)."""
    N, rate, nfft, avg, L, nbuf = 5, 200_000_000, 1000, 4, 50_123, 4
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    is_loop(dem, loop)
    ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
    emitted = 0
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        emitted += len(yr)
        if len(yr):
            err = rel_err_per_tone(y.reshape(-1, N), yr)
            print(f"{loop} tones buffer {c}: worst per-tone error {err.max():.3e}")
            assert err.max() <= TOL, (c, err.max())
    assert emitted > 0
    is_loop(dem, loop)
    dem.close()


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("shape", list(EXTREME_SHAPES))


def test_extreme_and_nonfinite_samples(cuda_device, gsdr_lib, oracle_mod, loop, kind, shape):
    extreme_and_nonfinite_samples(cuda_device, oracle_mod, loop, kind, shape)


@pytest.mark.parametrize("shape", [S_N65, S_ODD, S_C3], ids=shape_id)
def test_direct_extents(cuda_device, gsdr_lib, oracle_mod, loop, shape):
    """The guard zones of tests/_extents.py around input and output (both patterns, both offsets of each), through
    process_device and submit_device: 65 tones and a last row tile of 4 rows over 12.5 blocks (a half-empty last span);
    an odd row stride with F = 5 (185 samples: three spans, the last one short); the C3 block (125 blocks)."""
    N, rate, M, F, L = shape
    freq, xs, yrs = direct_inputs(shape, oracle_mod)
    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), lambda dem, ran: is_loop(dem, loop), xs, yrs, N)


def test_tones_extents_on_the_ddc_kernels(cuda_device, gsdr_lib, oracle_mod, loop):
    """The same guard zones around a TONES handle's buffers, every selected bin a DDC tone: the rows read the handle's
    raw window, the staging pass reads the caller's buffer (windows of 125 blocks)."""
    run_tones(cuda_device, lambda dem, ran: is_loop(dem, loop), *TONES_SHAPE, oracle_mod)


@pytest.mark.parametrize("N", [32, 288])
def test_one_handle_every_entry(cuda_device, gsdr_lib, loop, N):
    """One handle, one loop: process_device, submit_device / wait and the host entry give the same bits for the same
    buffers (M 1000, F 4, L 200 000: 125 blocks, 200 rows; one workgroup of tones and, with 288, a second one)."""
    import torch
    from gpu_sdr_amd.source import tone_comb
    rate, M, F, L = 200_000_000, 1000, 4, 200_000
    freq, _, _ = tone_comb(N, rate, seed=44)
    rng = np.random.default_rng(444)
    xs = [crandn(rng, L) for _ in range(3)]
    got = {}
    for entry in ("process", "submit", "host"):
        dem = make_direct(freq, rate, M, F, L)
        is_loop(dem, loop)
        ys = []
        for x in xs:
            if entry == "host":
                ys.append(run_host(dem, x))
                continue
            xin = torch.from_numpy(x).to(cuda_device)
            out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
            if entry == "process":
                n = dem.process_device(xin, out)
            else:
                dem.submit_device(xin, out)
                n = dem.wait()
            torch.cuda.synchronize()
            ys.append(out[:n].cpu().numpy())
        is_loop(dem, loop)
        dem.close()
        got[entry] = ys
    for entry in ("submit", "host"):
        for k, (y, w) in enumerate(zip(got[entry], got["process"])):
            assert y.size == w.size == N * (L // M), (entry, k)
            np.testing.assert_array_equal(y.view(np.int32), w.view(np.int32), err_msg=f"buffer {k} via {entry}")
