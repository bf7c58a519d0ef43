"""The cases every product loop of the pre-converted matrix-core DDC runs (DESIGN.md sections 4.1d - 4.1h): each stated
once, over all five loops of tests/_product_loops.py, each loop forced with every selecting switch set and asserted --
kernel name and the whole describe() tuple -- before the first call and after the last.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  What
is particular to one loop (switches and thresholds, the HDR combs, C3, wide against narrow bits) is in that loop's own
file.

The second half of the file brings the engine-wide behavioural tests of tests/test_gpu_parity.py (whose engine fixtures
stop at the four-product build) to the loops: the bodies are those tests' own, shared through tests/_product_loops.py,
at small shapes.  No test sets an engine switch by hand: force() is the only source, GSDR_PIPE_OVERLAP and
GSDR_PIPE_STREAMS (which select no loop) excepted."""
import numpy as np
import pytest

from _margins import record_info
from _product_loops import (EXTREME_KINDS, EXTREME_SHAPES, LOOPS, STREAMING_SHAPE, VALU_CASES, direct_parity,
                            dynamic_range_and_scale_carry, extreme_and_nonfinite_samples, force, fuzz_random_shapes, is_loop,
                            more_tap_phases, pipelined_fuzz, pipelined_overlapping_buffers, pipelined_tones,
                            pure_tones_demodulate_to_their_phasors, shape_id, streaming_runs, two_handles_interleaved)
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


# ---------------------------------------------------------------------------
# the engine-wide behavioural tests, on each loop
# ---------------------------------------------------------------------------
def _on(loop):
    return lambda dem, ran: is_loop(dem, loop)


def test_fuzz_random_shapes(cuda_device, gsdr_lib, oracle_mod, loop):
    """36 seeded shapes nobody picked by hand (loop_fuzz_shapes; tests/test_product_loops_host.py states what they
    cover: windows of one and two blocks, odd block counts, partial row tiles, rows == F - 1, F up to 8, 65 and 257
    tones, M >= rate, the NCO sample index passing `rate` inside a buffer); every shape runs the loop."""
    fuzz_random_shapes(cuda_device, oracle_mod, _on(loop), loop)


def test_pipelined_fuzz(cuda_device, gsdr_lib, loop):
    """The first 12 of those shapes through submit_device with up to four buffers in flight, the loudness changing by
    up to five orders between consecutive buffers: each call's convert pass reads its own scale table and writes its
    own image set, or the bits differ from the in-order entry's."""
    pipelined_fuzz(cuda_device, _on(loop), loop)


def test_dynamic_range_and_scale_carry(cuda_device, gsdr_lib, oracle_mod, loop):
    """Loudness 1, 1e-6, 1e-6, 3e4, 1, 0, 1e-3, 0 in consecutive buffers: finite everywhere, exact zeros where the
    oracle's are, every tone within TOL otherwise."""
    dynamic_range_and_scale_carry(cuda_device, oracle_mod, _on(loop))


@pytest.mark.parametrize("F", [5, 6, 7, 8])
def test_more_tap_phases(cuda_device, gsdr_lib, oracle_mod, loop, F):
    """pf_average 5 .. 8 at M = 40: windows of 200, 240, 280 and 320 samples -- 7, 8, 9 and 10 blocks (both parities of
    the span count) with 24, 16, 8 and 0 samples of padding; the device and the host entry in turn."""
    more_tap_phases(cuda_device, oracle_mod, _on(loop), F, M=40, alternate=True)


def test_two_handles_interleaved(cuda_device, gsdr_lib, oracle_mod, loop):
    """Two handles of one loop fed alternately, loudness 10 ** (c - 2k): image sets, d_bfrag3 / d_ptab3 and the scale
    tables are per handle."""
    two_handles_interleaved(cuda_device, oracle_mod, lambda k, *shape: make_direct(*shape),
                            lambda k, dem, ran: is_loop(dem, loop))


def test_two_handles_on_different_loops_interleaved(cuda_device, gsdr_lib, oracle_mod, monkeypatch, loop):
    """The same with the second handle on the next loop of LOOPS (cyclically): the switches are read once per handle,
    at creation, so the environment is forced anew between the two creations."""
    names = list(LOOPS)
    pair = (loop, names[(names.index(loop) + 1) % len(names)])

    def make(k, *shape):
        force(monkeypatch, pair[k])
        return make_direct(*shape)
    two_handles_interleaved(cuda_device, oracle_mod, make, lambda k, dem, ran: is_loop(dem, pair[k]))


def test_streaming_equals_one_long_buffer(cuda_device, gsdr_lib, oracle_mod, loop):
    """One stream as one buffer of 60 000 samples and as three of 20 000: both within TOL of the oracle of the whole
    stream.  The difference between the two runs is recorded, not bounded (two runs inside TOL of a third need not be
    within 2e-6 of each other, the figure test_direct_streaming_equals_one_long_buffer holds four-product engines to)."""
    N, rate, M, F, L = STREAMING_SHAPE
    freq, x, ya, yb = streaming_runs(cuda_device, _on(loop))
    yr = oracle_mod.Direct(freq, rate, M, F, L).process(x)
    assert ya.shape == yb.shape == yr.shape == (L // M, N)
    ea = rel_err_per_tone(ya, yr, "one buffer")
    eb = rel_err_per_tone(yb, yr, "three buffers")
    den = np.linalg.norm(ya.astype(np.complex128), axis=0)
    diff = float((np.linalg.norm(yb.astype(np.complex128) - ya, axis=0) / den).max())
    record_info(diff, "three buffers against one buffer, worst per-tone difference")
    print(f"{loop}: one buffer {ea.max():.3e}, three buffers {eb.max():.3e}, three against one {diff:.3e}")
    assert ea.max() <= TOL and eb.max() <= TOL, (float(ea.max()), float(eb.max()))


def test_pure_tones_demodulate_to_their_phasors(cuda_device, gsdr_lib, loop):
    """Closed form, no oracle: |y - a e^{i phi}| < 5e-4 (the filter's stop band) behind the first F rows."""
    pure_tones_demodulate_to_their_phasors(cuda_device, _on(loop))


@pytest.mark.parametrize("overlap,streams", [("1", "2"), ("1", "3"), ("0", "2")])
def test_pipelined_overlapping_buffers(cuda_device, gsdr_lib, oracle_mod, monkeypatch, loop, overlap, streams):
    """Eleven buffers of loudness 1e-4 .. 100 with up to four in flight, 160 tones x 1000 rows (more than one workgroup
    of tones on every loop): bit-equal to the in-order handle, the first four within TOL of the oracle, and
    process_device works after the drain."""
    monkeypatch.setenv("GSDR_PIPE_OVERLAP", overlap)
    monkeypatch.setenv("GSDR_PIPE_STREAMS", streams)
    pipelined_overlapping_buffers(cuda_device, oracle_mod, _on(loop), N=160, L=100_000)


@pytest.mark.parametrize("streams", ["2", "3"])
def test_pipelined_tones_on_the_ddc_kernels(cuda_device, gsdr_lib, oracle_mod, monkeypatch, loop, streams):
    """TONES (nfft 250, 96 tones, L = 100 003) through submit_device, nine buffers of changing loudness and batch
    count: bit-equal to the in-order handle, the first four within TOL of the oracle."""
    monkeypatch.setenv("GSDR_PIPE_STREAMS", streams)
    pipelined_tones(cuda_device, oracle_mod, _on(loop))
