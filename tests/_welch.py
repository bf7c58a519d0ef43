"""A numpy-only float64 oracle of the Welch estimator of include/gsdr.h ("Welch spectra on the device") and the cases
the Welch tests share.  The oracle states the estimator without the float32 roundings of its steps 1 - 3 (the device
rounds the detrended sample, the windowed sample and the transform to float32; the host twin, like this oracle, does
not): closed-form detrend, np.fft.fft, the spectra of the real and of the imaginary part of g z, the density scaling.
tests/test_welch_host.py checks it against scipy.signal.welch; the GPU tests use only this module.

Plain module: no GPU work, no library call at import time.
"""
import numpy as np

MODES = ("raw", "rotate", "dbc", "gain")
PARITY_BAR = 1e-5          # the project's parity bar: per bin, relative, device against this oracle
HOST_BAR = 1e-9            # host twin and scipy against this oracle


def hann32(nperseg):
    """The default window of the contract: the periodic Hann window, evaluated in double, rounded to float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nperseg) / nperseg)).astype(np.float32)


def n_segments(total, nperseg, step):
    return 0 if total < nperseg else (total - nperseg) // step + 1


def mean_of(rows, nperseg, step):
    """S / (n_seg step) with S summed as the contract says: the first `step` rows of a segment one after the other, the
    segment sums in segment order (np.cumsum adds sequentially), real and imaginary part on their own."""
    x = np.asarray(rows).astype(np.complex128)
    n_seg = n_segments(x.shape[0], nperseg, step)
    if n_seg == 0:
        return np.zeros(x.shape[1], dtype=np.complex128)
    seg_sums = np.cumsum(x[:n_seg * step].reshape(n_seg, step, -1), axis=1)[:, -1, :]
    s = np.cumsum(seg_sums, axis=0)[-1]
    return s.real / float(n_seg * step) + 1j * (s.imag / float(n_seg * step))


def gain_of(mode, mean, gain=None):
    m = np.asarray(mean, dtype=np.complex128)
    ok = np.isfinite(m) & (m != 0)
    safe = np.where(ok, m, 1.0)
    if mode == "raw":
        return np.ones_like(m)
    if mode == "rotate":
        return np.where(ok, np.abs(safe) / safe, 1.0)
    if mode == "dbc":
        return np.where(ok, 1.0 / safe, 1.0)
    if mode == "gain":
        return np.asarray(gain).astype(np.complex128)
    raise ValueError(mode)


def accumulators(rows, nperseg, step, detrend="linear", window=None):
    """(A0, A1, A2) of the contract, [n_ch][nperseg // 2 + 1] float64 each, and n_seg."""
    x = np.asarray(rows).astype(np.complex128)
    N, K1 = nperseg, nperseg // 2 + 1
    n_seg = n_segments(x.shape[0], N, step)
    w = (hann32(N) if window is None else np.asarray(window, dtype=np.float32)).astype(np.float64)
    A = np.zeros((3, x.shape[1], K1))
    t = np.arange(N) - (N - 1) / 2.0
    for s in range(n_seg):                                  # one segment at a time: the 8192-point cases stay small
        seg = x[s * step:s * step + N]                      # [N][n_ch]
        if detrend in ("linear", "constant"):
            m = seg.mean(axis=0)
            b = (seg * t[:, None]).sum(axis=0) / (t * t).sum() if detrend == "linear" else 0.0
            seg = seg - (m + b * t[:, None])
        elif detrend not in ("none", None, False):
            raise ValueError(detrend)
        Z = np.fft.fft(seg * w[:, None], axis=0)
        Zm = np.conj(Z[(N - np.arange(K1)) % N])
        X, Y = (Z[:K1] + Zm) / 2.0, (Z[:K1] - Zm) / 2.0j
        A[0] += (np.abs(X) ** 2).T
        A[1] += (np.abs(Y) ** 2).T
        A[2] += (X * np.conj(Y)).real.T
    return A, n_seg, float((w * w).sum())


def psd_from(A, n_seg, sum_w2, g, nperseg, fs=1.0):
    K1 = nperseg // 2 + 1
    gr, gi = g.real[:, None], g.imag[:, None]
    f = np.full(K1, 2.0)
    f[0] = f[-1] = 1.0
    scale = f / (fs * sum_w2 * n_seg)
    out = np.empty((A.shape[1], 2, K1))
    out[:, 0] = (gr * gr * A[0] + gi * gi * A[1] - 2 * gr * gi * A[2]) * scale
    out[:, 1] = (gi * gi * A[0] + gr * gr * A[1] + 2 * gr * gi * A[2]) * scale
    return out


class Oracle:
    """The accumulators and the mean of one stream, computed once; psd(mode) is cheap."""

    def __init__(self, rows, nperseg, step, detrend="linear", window=None):
        self.nperseg, self.step = nperseg, step
        self.A, self.n_seg, self.sum_w2 = accumulators(rows, nperseg, step, detrend, window)
        self.mean = mean_of(rows, nperseg, step)

    def psd(self, mode, fs=1.0, gain=None):
        return psd_from(self.A, self.n_seg, self.sum_w2, gain_of(mode, self.mean, gain), self.nperseg, fs)


def noise_rows(n_rows, n_ch, seed, carrier=1.0, sigma=1e-3, slope=0.0):
    """White complex noise of `sigma` per component on a carrier (channel c: the carrier turned by 0.7 c rad and scaled
    by 1 + 0.1 (c mod 7), so that the modes differ per channel), plus `slope` per row; complex64."""
    rng = np.random.default_rng(seed)
    c = np.arange(n_ch)
    car = carrier * np.exp(0.7j * c) * (1.0 + 0.1 * (c % 7))
    x = car[None, :] + sigma * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))
    x = x + slope * np.arange(n_rows)[:, None] * (1.0 + 0.5j)
    return x.astype(np.complex64)


def some_gain(n_ch, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n_ch) + 1j * rng.standard_normal(n_ch)).astype(np.complex64)


def cuttings(total, nperseg, step):
    """name -> feed lengths that sum to `total`: whole; sevens; with empty feeds; feeds shorter than a step; a feed that
    holds several segments."""
    def rest(parts):
        left = total - sum(parts)
        assert left >= 0
        return parts + ([left] if left else [])

    short = max(1, step - 1)
    several = min(total, nperseg + 3 * step)
    a = min(total, 3)
    return {
        "whole": [total],
        "sevens": rest([7] * (total // 7)),
        "empties": rest([0, a, 0, 0, min(total - a, nperseg + 1), 0]),
        "short": rest([short] * (total // short)),
        "several": rest([several]),
    }


def rel_err(got, want):
    """Worst per-bin relative error; every bin counts."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.abs(want)))


def floor_ratio(want):
    """The smallest bin of each spectrum over that spectrum's mean, the worst over channels and parts."""
    return float(np.min(want.min(axis=-1) / want.mean(axis=-1)))
