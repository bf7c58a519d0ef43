"""The float64 model of the TX tone comb (tests/_tx_comb.py) is what test_gpu_tx_comb.py holds the device to; here the
model is held to something plainer, on the CPU: Python integers with math.fsum, the fp64 oracle, and -- the other way
round -- a float32 emulation of tones_synth_kernel's factorisation shows that the combs of the case table leave a
correct kernel a factor 10 inside the device tests' bar."""
import numpy as np
import pytest

import _tx_comb as T
from _margins import record_margin


@pytest.mark.parametrize("rate,n_tones", T.CASES)
def test_model_against_python_integers(rate, n_tones):
    """A handful of samples per case and start, the first and the last of a fill and those on both sides of the wrap
    at `rate`: |model - exact| <= 1e-12 sum|a|.  (The complex64 form of host_tones differs from `exact` by
    6e-10 .. 9e-9 sum|a|: its final rounding, which the complex128 form does not have.)"""
    freq, ampl, phase = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    worst = 0.0
    for start in sorted({T.reduced(s, rate) for s in (0, rate - 5, rate - 1, 12345, 3 * rate + 17)}):
        x = T.model(1025, start, rate, freq, ampl, phase)
        assert x.dtype == np.complex128
        wrap = (rate - start) % rate                     # the sample of this fill whose index is 0 again
        for j in sorted({0, 1, 511, 1024, (wrap - 1) % 1025, wrap % 1025}):
            worst = max(worst, abs(x[j] - T.exact(start + j, rate, freq, ampl, phase)))
    print(f"rate {rate} tones {n_tones}: |model - exact| / sum|a| = {worst / sa:.3e}")
    assert worst <= 1e-12 * sa


def test_complex64_form_differs_by_its_rounding_only():
    """host_tones as the other tests use it (complex64) is the complex128 form rounded once."""
    from gpu_sdr_amd.source import host_tones
    rate, n_tones = 2_147_483_647, 257
    freq, ampl, phase = T.comb(rate, n_tones)
    x = T.model(1025, rate - 5, rate, freq, ampl, phase)
    np.testing.assert_array_equal(host_tones(1025, rate - 5, rate, freq, ampl, phase), x.astype(np.complex64))


@pytest.mark.parametrize("rate,n_tones", [(1_000_003, 257), (65_536, 320), (1000, 65)])
def test_model_against_the_fp64_oracle(gsdr_lib, oracle_mod, rate, n_tones):
    """Phase 0, a tone set gsdr_tx_tone_bins leaves as it is: the oracle's tone_gen sums in double and returns
    float32, so it differs from the model by that rounding alone: each component by at most 2^-24 of itself, the
    sample by at most 2^-24 |x| <= 2^-24 sum|a| = 6.0e-8 sum|a| (measured: 1.0e-8 .. 2.1e-8)."""
    from gpu_sdr_amd.generator import tone_bins
    freq, ampl, _ = T.comb(rate, n_tones)
    f2, a2 = tone_bins(freq, ampl, rate)
    np.testing.assert_array_equal(f2, freq)
    np.testing.assert_array_equal(a2, ampl)
    sa = float(np.sum(ampl, dtype=np.float64))
    worst = 0.0
    for n, start in ((4099, 0), (1025, rate - 5), (1025, 12345 % rate)):
        want = oracle_mod.tone_gen(freq, ampl, rate, start, n)
        worst = max(worst, float(np.max(np.abs(want - T.model(n, start, rate, freq, ampl)))))
    print(f"rate {rate} tones {n_tones}: |oracle - model| / sum|a| = {worst / sa:.3e}")
    record_margin(worst / sa, "oracle.tone_gen (float32 out) against the model / sum of amplitudes")
    assert worst <= (2.0 ** -24 + 1e-12) * sa


@pytest.mark.parametrize("rate,n_tones", [(65_536, 257), (1_000_003, 257), (1000, 65)])
def test_period_model_against_the_model(rate, n_tones):
    """The inverse-DFT period (the reference for buffers of 100 000 samples) against the model on windows at both
    ends of the period and across its wrap: 1e-10 sum|a|, four orders under the device tests' bar."""
    for phase_given in (False, True):
        freq, ampl, phase = T.comb(rate, n_tones)
        if not phase_given:
            phase = None
        p = T.period_model(rate, freq, ampl, phase)
        sa = float(np.sum(ampl, dtype=np.float64))
        worst = 0.0
        for start in (0, rate - 5, rate // 3):
            n = min(4099, 3 * rate)
            worst = max(worst, float(np.max(np.abs(T.wrapped(p, start, n) - T.model(n, start, rate, freq, ampl, phase)))))
        print(f"rate {rate} tones {n_tones} phases {phase_given}: |period - model| / sum|a| = {worst / sa:.3e}")
        assert worst <= 1e-10 * sa


@pytest.mark.parametrize("rate,n_tones", T.CASES)
def test_float32_emulation_of_the_kernel_is_a_factor_10_inside_the_bar(rate, n_tones):
    """tones_synth_kernel's arithmetic in numpy float32 (_tx_comb.emulate_synth) against the model, for the combs of
    the case table at starts 0, rate - 5 and 12345: the inputs chosen leave a correct kernel inside the bar of the
    device tests with a factor 10 to spare.  A numpy emulation, not a measurement of the device: 6.9e-8 .. 1.74e-7
    here; the device, over all sixteen fills of a case, measured 7.5e-8 .. 2.45e-7 (profiles/txcomb_margins.json).
    The factor belongs to these combs: see _tx_comb.comb on how other draws of 63 .. 65 tones fare."""
    freq, ampl, phase = T.comb(rate, n_tones)
    sa = float(np.sum(ampl, dtype=np.float64))
    worst = 0.0
    for start in (0, rate - 5, 12345 % rate):
        got = T.emulate_synth(1025, start, rate, freq, ampl, phase)
        worst = max(worst, float(np.max(np.abs(got - T.model(1025, start, rate, freq, ampl, phase)))))
    print(f"rate {rate} tones {n_tones}: |float32 emulation - model| / sum|a| = {worst / sa:.3e}")
    record_margin(worst / sa, "float32 emulation against the model / sum of amplitudes")
    assert 10.0 * worst <= T.BAR * sa


def test_device_mod_rate_is_short_by_one_at_most():
    """The device's mod_rate (csrc/ddc_device.h) in Python integers: q = (x magic) >> 64 with
    magic = (2^64 - 1) // rate, r = x - q rate, then corrections.  With d = 2^64 / rate - magic <= 1 the estimate is
    floor(x / rate - x d / 2^64), and x d / 2^64 < 1/2 for x < 2^63: q is short by one at most, so ONE correction
    gives x mod rate for everything the kernels pass (a start below rate plus a sample offset, a product of two values
    below rate <= 2^31 - 1); the second `if (r >= rate) r -= rate` never fires there and no output can depend on it.
    Checked at the values that come closest: just under multiples of `rate` at the top of the range."""
    rng = np.random.default_rng(3)
    rates = list(T.RATES) + [1, 2, 3, 2 ** 16, 2 ** 30, 2 ** 31 - 2, 2 ** 31]
    for rate in rates:
        magic = (2 ** 64 - 1) // rate
        top = 2 ** 63 - 1
        xs = {0, 1, rate - 1, rate, (rate - 1) ** 2, (rate - 1) * (rate - 2), top, top - 1}
        for k in (top // rate, top // rate - 1, (rate - 1) ** 2 // rate, 2 ** 62 // rate, 2 ** 61 // rate):
            xs.update(k * rate + d for d in (-2, -1, 0, 1, rate - 1) if 0 <= k * rate + d <= top)
        xs.update(int(v) for v in rng.integers(0, top, size=2000, dtype=np.int64))
        xs.update(int(a) * int(b) for a, b in rng.integers(0, rate, size=(2000, 2), dtype=np.int64))
        worst = 0
        for x in xs:
            q = (x * magic) >> 64
            r = x - q * rate
            worst = max(worst, r // rate - (x % rate) // rate)
            assert r - rate * (r >= rate) == x % rate, (rate, x)
        assert worst <= 1


def test_the_case_table_is_what_it_says():
    assert {r for r, _ in T.CASES} == set(T.RATES) and {t for _, t in T.CASES} == set(T.TONE_COUNTS)
    assert len(set(T.CASES)) == len(T.CASES)
    for rate, n_tones in T.CASES:
        freq, ampl, phase = T.comb(rate, n_tones)
        assert len(set(freq.tolist())) == n_tones and 0 not in freq and (2 * np.abs(freq.astype(np.int64)) < rate).all()
        assert freq.tolist()[:4] == [rate // 2 - 1, -rate // 2 + 1, 1, -1][:n_tones]
        assert ampl.dtype == phase.dtype == np.float32 and (ampl >= 0.01).all() and (ampl <= 1.0).all()
        assert (np.abs(phase) < 3 * np.pi + 1e-6).all()
        if n_tones >= 64:
            assert phase.min() < -2 * np.pi and phase.max() > 2 * np.pi and ampl.max() / ampl.min() > 30
        assert {n for n, _ in T.fills(rate)} == set(T.LENGTHS)
        assert {s for n, s in T.fills(rate) if n == 1025} == set(T.starts(rate))
        assert len(set(T.fills(rate))) == len(T.fills(rate)) == 16
    assert T.reduced(-5, 1000) == 995 and T.reduced(3017, 1000) == 17
