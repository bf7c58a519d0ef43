"""The TX tone comb on the device against its float64 model (tests/_tx_comb.py; the model itself is held to exact
integers and to the fp64 oracle in test_tx_comb_host.py): tones_synth_kernel behind gsdr_txgen_tones_fill and
TX_buffer_generator.get, and source_tones_kernel behind gsdr_source_tones.

What is pinned: the `phase` argument of gsdr_txgen_tones_create (value, sign, which tone), the tone slots (tables
B[k][64] / C[k][16], the hand-round by v_readlane, the clamps of the last chunk) one slot at a time, `start` as a
caller passes it (negative, past `rate`, the wrap inside the first workgroup, rates up to 2^31 - 1 through the device's
mod_rate), short lengths, no tones at all, and the running index of the generator over two wraps of its period.

Bars: max |x - model| <= 2e-6 sum|a| for the comb (the bar of test_tx_tone_generator_against_oracle), 3e-6 sum|a|
for gsdr_source_tones (the bar of test_device_sources_match_their_formulas)."""
import ctypes as C

import numpy as np
import pytest

import _extents as E
import _tx_comb as T
from _margins import record_margin

pytestmark = pytest.mark.gpu

TAIL = 64                    # samples behind the n of a fill that must stay as they were
LABEL = "max abs error / sum of amplitudes"


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def make_handle(lib, rate, freq, ampl, phase):
    freq = np.ascontiguousarray(freq, dtype=np.int32)
    ampl = np.ascontiguousarray(ampl, dtype=np.float32)
    phase = None if phase is None else np.ascontiguousarray(phase, dtype=np.float32)
    h = lib.gsdr_txgen_tones_create(rate, freq.ctypes.data_as(C.POINTER(C.c_int)), _fp(ampl), _fp(phase), len(freq), 0)
    assert h, lib.gsdr_last_error(None)
    return h


def fill(lib, h, n, start, dev):
    """n samples from `start` as the caller gives it; the TAIL samples behind them must keep their NaN."""
    import torch
    out = torch.full((n + TAIL,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    assert lib.gsdr_txgen_tones_fill(h, out.data_ptr(), n, start, None) == 0, lib.gsdr_last_error(None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[n:].view(np.float32)).all(), (n, start, "written behind n")
    return got[:n]


def worst_error(got, want):
    assert got.shape == want.shape and np.isfinite(got.view(np.float32)).all()
    return float(np.max(np.abs(got.astype(np.complex128) - want)))


# ---------------------------------------------------------------------------
# a. gsdr_txgen_tones_fill over the case table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_tones", T.CASES)
def test_tones_fill_against_the_model(cuda_device, gsdr_lib, rate, n_tones):
    """Every start at n = 1025 and every length at start = rate - 5, phases passed.  start = -5 is the model at
    rate - 5, 3 rate + 17 the model at 17.  (One model per start: the lengths at rate - 5 are its beginning.)"""
    freq, ampl, phase = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    h = make_handle(gsdr_lib, rate, freq, ampl, phase)
    models, bad = {}, []
    for n, start in T.fills(rate):
        s = T.reduced(start, rate)
        if s not in models:
            models[s] = T.model(max(T.LENGTHS) if s == rate - 5 else 1025, s, rate, freq, ampl, phase)
        err = worst_error(fill(gsdr_lib, h, n, start, cuda_device), models[s][:n])
        print(f"rate {rate} tones {n_tones} n {n} start {start}: {err / sa:.3e}")
        record_margin(err / sa, LABEL)
        if not err <= T.BAR * sa:
            bad.append((n, start, err / sa))
    gsdr_lib.gsdr_txgen_close(h)
    assert T.reduced(-5, rate) == rate - 5 and T.reduced(3 * rate + 17, rate) == 17 % rate
    assert not bad, bad


# ---------------------------------------------------------------------------
# b. one tone at a time inside a large comb
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_tones", [(1_000_003, 320), (2_147_483_647, 2048)])
def test_one_slot_at_a_time(cuda_device, gsdr_lib, rate, n_tones):
    """Every amplitude 0 except slot k (a = 1, its own phase): the exact zeros of the other slots add nothing, so the
    output is that single tone, within 2e-6 -- its table rows, its lane in the hand-round, its chunk's clamp, with
    nothing hidden under the sum of the others."""
    freq, _, phase = T.comb(rate, n_tones)
    bad = []
    for k in (0, 1, 63, 64, 65, 255, 256, 257, n_tones - 1):
        ampl = np.zeros(n_tones, dtype=np.float32)
        ampl[k] = 1.0
        h = make_handle(gsdr_lib, rate, freq, ampl, phase)
        for n, start in ((1025, rate - 5), (4099, 12345)):
            want = T.model(n, start, rate, freq[k:k + 1], ampl[k:k + 1], phase[k:k + 1])
            err = worst_error(fill(gsdr_lib, h, n, start, cuda_device), want)
            print(f"rate {rate} tones {n_tones} slot {k} n {n} start {start}: {err:.3e}")
            record_margin(err, LABEL)
            if not err <= T.BAR:
                bad.append((k, n, start, err))
        gsdr_lib.gsdr_txgen_close(h)
    assert not bad, bad


# ---------------------------------------------------------------------------
# c., d. phases: none given, and their sign
# ---------------------------------------------------------------------------
def test_null_phases_are_zero_phases(cuda_device, gsdr_lib):
    rate, n_tones = 1_000_003, 257
    freq, ampl, _ = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    h = make_handle(gsdr_lib, rate, freq, ampl, None)
    for n, start in ((1025, rate - 5), (4099, 0)):
        err = worst_error(fill(gsdr_lib, h, n, start, cuda_device), T.model(n, start, rate, freq, ampl, None))
        record_margin(err / sa, LABEL)
        assert err <= T.BAR * sa, (n, start, err / sa)
    gsdr_lib.gsdr_txgen_close(h)


def test_phase_sign(cuda_device, gsdr_lib):
    """The handle made with -phi gives the model of -phi, and that is more than 100 bars away from the handle made
    with phi: neither can pass with the phases ignored or their sign flipped."""
    rate, n_tones, n, start = 1_000_003, 257, 1025, 1_000_003 - 5
    freq, ampl, phase = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    got = {}
    for sign in (1.0, -1.0):
        ph = (sign * phase).astype(np.float32)
        h = make_handle(gsdr_lib, rate, freq, ampl, ph)
        got[sign] = fill(gsdr_lib, h, n, start, cuda_device)
        gsdr_lib.gsdr_txgen_close(h)
        err = worst_error(got[sign], T.model(n, start, rate, freq, ampl, ph))
        record_margin(err / sa, LABEL)
        assert err <= T.BAR * sa, (sign, err / sa)
    apart = float(np.max(np.abs(got[1.0] - got[-1.0])))
    assert apart > 100 * T.BAR * sa, apart / sa


# ---------------------------------------------------------------------------
# e. no tones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_no_tones_is_exact_zeros(cuda_device, gsdr_lib, off):
    import torch
    rate, n = 1_000_003, 1025
    h = gsdr_lib.gsdr_txgen_tones_create(rate, None, None, None, 0, 0)
    assert h, gsdr_lib.gsdr_last_error(None)
    whole, view = E.guarded_output(n, off, cuda_device)
    assert gsdr_lib.gsdr_txgen_tones_fill(h, view.data_ptr(), n, rate - 5, None) == 0
    torch.cuda.synchronize()
    gsdr_lib.gsdr_txgen_close(h)
    E.check_output(whole, view, n)
    assert (view.cpu().numpy().view(np.uint32) << 1 == 0).all()          # +0 or -0, nothing else


# ---------------------------------------------------------------------------
# f. TX_buffer_generator(TONES) on its running index
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate,L", [(65_536, 100_003), (1_000_003, 99_999)])
def test_generator_running_index_over_two_wraps(cuda_device, gsdr_lib, rate, L):
    """257 tones, whole buffers, get() to the device and to the host in turn, until the period (2 rate for the first
    case: a buffer longer than `rate`) has wrapped twice; against one period of the model (by inverse DFT, held to the
    model in test_tx_comb_host.py) at start = (c L) mod period."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.generator import tone_bins
    freq, ampl, _ = T.comb(rate, 257)
    f2, a2 = tone_bins(freq, ampl, rate)
    np.testing.assert_array_equal(f2, freq)                  # no duplicate, no 0 Hz: the comb is generated as given
    np.testing.assert_array_equal(a2, ampl)
    sa = float(np.sum(ampl, dtype=np.float64))
    one = T.period_model(rate, freq, ampl)
    period = rate * -(-L // rate)
    nbuf = -(-2 * period // L) + 1
    tx = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=[int(f) for f in freq],
                                       ampl=[float(a) for a in ampl], wave_type=[g.w_type.TONES] * len(freq)))
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    xh = np.empty(L, dtype=np.complex64)
    start, wraps, bad = 0, 0, []
    for c in range(nbuf):
        if c % 2:
            tx.get(xh)
            got = xh
        else:
            tx.get(x)
            torch.cuda.synchronize()
            got = x.cpu().numpy()
        err = worst_error(got, T.wrapped(one, start % rate, L))
        record_margin(err / sa, LABEL)
        if not err <= T.BAR * sa:
            bad.append((c, start, err / sa))
        wraps += (start + L) // period
        start = (start + L) % period
    tx.close()
    assert wraps >= 2
    assert not bad, bad


# ---------------------------------------------------------------------------
# g. gsdr_source_tones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [1000, 200_000_000, 2_147_483_647])
@pytest.mark.parametrize("n_tones", [1, 5, 64, 300])
def test_source_tones_against_the_model(cuda_device, gsdr_lib, rate, n_tones):
    """The per-sample synthesis (bench.py's input and the reference of the at-scale test) with phases in
    (-3 pi, 3 pi), n = 20 000 from rate - 7000 (start + j passes `rate`) and from 0, sigma = 0."""
    import torch
    from gpu_sdr_amd.source import device_tones
    n = 20_000
    freq, ampl, phase = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    x = torch.empty(n, dtype=torch.complex64, device=cuda_device)
    for start in (max(rate - 7000, 0), 0):
        device_tones(x, start, rate, freq, ampl, phase, sigma=0.0)
        err = worst_error(x.cpu().numpy(), T.model(n, start, rate, freq, ampl, phase))
        print(f"rate {rate} tones {n_tones} start {start}: {err / sa:.3e}")
        record_margin(err / sa, LABEL)
        assert err <= T.SOURCE_BAR * sa, (start, err / sa)


def test_source_tones_noise_is_a_function_of_seed_and_start(cuda_device, gsdr_lib):
    """sigma > 0: the statistics of test_device_sources_match_their_formulas on top of this comb, and the noise is
    reproducible: the same seed and start give the same bits, another seed does not."""
    import torch
    from gpu_sdr_amd.source import device_tones
    rate, n, sigma = 200_000_000, 20_000, 0.1
    freq, ampl, phase = T.comb(rate, 5)
    start = rate - 7000
    a, b, c = (torch.empty(n, dtype=torch.complex64, device=cuda_device) for _ in range(3))
    device_tones(a, start, rate, freq, ampl, phase, sigma=sigma, seed=5)
    device_tones(b, start, rate, freq, ampl, phase, sigma=sigma, seed=5)
    device_tones(c, start, rate, freq, ampl, phase, sigma=sigma, seed=6)
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a != c).mean() > 0.99
    for y in (a, c):
        noise = y - T.model(n, start, rate, freq, ampl, phase)
        assert abs(noise.real.std() - sigma) < 0.005 and abs(noise.imag.std() - sigma) < 0.005
        assert abs(noise.mean()) < 0.005
