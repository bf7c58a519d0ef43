"""The float64 model of TONES / NOISE (tests/_pfb.py) against the oracle, on the CPU.

The GPU run tests compare the device with the model, because the oracle's O(nfft^2) DFT is too slow for hundreds of
frames of a thousand points; here the model is held to oracle.Noise / oracle.Pfb on a dozen small shapes: the lengths
of every call exactly, the values to 1e-12.

The oracle sums in double and hands back complex64, so a component of its output is the float nearest to its double
sum: 6e-8 relative, four orders above the bar.  The comparison therefore asks how far the model's double is from the
interval of doubles that round to the oracle's float (half a float spacing each way): that distance is what a
disagreement of the two double sums leaves over, and it is held to 1e-12 of the call's norm.  A model value that
differs from the oracle's sum by more than 1e-12 relative lands outside the interval for all but a vanishing share of
the components.
"""
import numpy as np
import pytest

import _pfb

RATE = 1_000_000

# nfft, avg, L, calls, TONES frequencies (None: NOISE)
SHAPES = [
    (16, 1, 100, 5, None),                 # one tap, L not a multiple of nfft
    (16, 4, 50, 6, None),                  # buffers shorter than a window (64): calls without a frame
    (10, 2, 1003, 3, None),
    (64, 3, 1000, 4, None),
    (100, 4, 5_000, 3, None),
    (128, 5, 4_001, 3, None),
    (256, 6, 10_000, 3, None),
    (243, 4, 3_000, 3, None),              # 3^5
    (101, 2, 2_000, 4, None),              # prime
    (64, 4, 777, 5, [100_000, -100_000, 100_000, 0, -484_375, 15_625, 15_625]),      # repeated and negative-frequency bins
    (200, 3, 2_345, 4, [-250_000, 250_000, -5_000, 5_000, 499_999, -500_000, 250_000]),
    (256, 6, 1_500, 5, [123_456, -123_456, 123_456]),                                  # L shorter than the window (1536)
    (32, 1, 31, 5, [0, 31_250]),                                                       # a buffer shorter than one frame
]


def outside_rounding(model, got32):
    """per component: how far the model's double lies outside the doubles that round to the oracle's float"""
    out = np.zeros(model.shape)
    for part in (np.real, np.imag):
        m, g = part(model), part(got32).astype(np.float32)
        half = np.spacing(np.abs(g)).astype(np.float64) / 2
        out = np.hypot(out, np.maximum(np.abs(m - g.astype(np.float64)) - half, 0.0))
    return out


@pytest.mark.parametrize("nfft,avg,L,calls,freq", SHAPES, ids=lambda v: str(v) if not isinstance(v, list) else "tones%d" % len(v))
def test_model_is_the_oracle(oracle_mod, nfft, avg, L, calls, freq):
    rng = np.random.default_rng(77 + nfft + avg)
    if freq is None:
        ref, bins = oracle_mod.Noise(nfft, avg, L), None
    else:
        ref = oracle_mod.Pfb(freq, RATE, nfft, avg, L)
        bins = ref.bins()
        assert len(set(bins.tolist())) < len(bins) or nfft == 32      # the TONES shapes repeat a bin
    model = _pfb.Model(oracle_mod, nfft, avg, bins)
    emitted = 0
    for c in range(calls):
        x = _pfb.tones_on_bins(rng, L, nfft, [1, nfft // 3, nfft - 2], model.w)
        want = model.frames_of(L)
        y, yr = model.process(x), ref.process(x)
        assert y.shape == yr.shape and y.shape[0] == want, (c, y.shape, yr.shape, want)
        if y.size:
            emitted += 1
            assert np.linalg.norm(outside_rounding(y, yr)) <= 1e-12 * np.linalg.norm(y), c
            # and the plain distance is the oracle's rounding to float, no more
            assert np.linalg.norm(y - yr) <= 2.0 ** -24 * np.sqrt(2) * np.linalg.norm(y) + 1e-12 * np.linalg.norm(y)
    assert emitted >= 2
    ref.close()


def test_fp32_emulation_is_a_float32_evaluation(oracle_mod):
    """the emulation sits a few float32 roundings from the model, well inside the parity bar, and is not the model"""
    rng = np.random.default_rng(5)
    for nfft, avg in ((128, 4), (200, 3), (1024, 4), (101, 2), (4096, 4)):
        nfr = 20
        model = _pfb.Model(oracle_mod, nfft, avg)
        x = _pfb.tones_on_bins(rng, (nfr + avg) * nfft, nfft, [1, nfft // 3, nfft - 2], model.w)
        y = model.process(x)[:nfr]
        w32 = oracle_mod.make_sinc_window(nfft * avg, np.float32(1.0 / (2 * nfft)))
        e = _pfb.fp32_emulation(x, nfft, avg, w32, nfr)
        err = np.linalg.norm(e - y, axis=0) / np.linalg.norm(y, axis=0)
        assert 1e-9 < err.max() <= 2e-6, (nfft, err.max())
