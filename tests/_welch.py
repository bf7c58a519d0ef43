"""A numpy-only float64 oracle of the Welch estimator of include/gsdr.h ("Welch spectra on the device") and the cases
the Welch tests share.  The oracle states the estimator without the float32 roundings of its steps 1 - 3 (the device
rounds the detrended sample, the windowed sample and the transform to float32; the host twin, like this oracle, does
not): closed-form detrend, np.fft.fft, the spectra of the real and of the imaginary part of g z, the density scaling.
tests/test_welch_host.py checks it against scipy.signal.welch; the GPU tests use only this module.
Beside it: a float32 MODEL of the contract (accumulators32), which says whether an input is one a float32 pipeline can
resolve to the bar at all, and the GRID of cases (every segment kernel x detrend x window) with their preconditions.

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


def _fft_c64(e):
    """The forward transform of complex64 columns IN complex64 (numpy.fft before 2.0 works in double)."""
    try:
        from scipy.fft import fft
    except ImportError:
        fft = np.fft.fft
    Z = fft(e, axis=0)
    assert Z.dtype == np.complex64, Z.dtype
    return Z


def accumulators32(rows, nperseg, step, detrend="linear", window=None):
    """`accumulators` with the roundings the contract names: d_n rounded once to float32 after the double subtraction
    (no detrend: the sample itself), e_n = d_n w_n in float32, a complex64 transform, the three products of a segment
    (formed in double from the float32 transform) rounded to float32 before the double accumulation.  A MODEL of the
    device, not its twin -- the transform is another one: what it cannot resolve of an input, the device is not asked to."""
    x = np.asarray(rows).astype(np.complex128)
    N, K1 = nperseg, nperseg // 2 + 1
    n_seg = n_segments(x.shape[0], N, step)
    w = hann32(N) if window is None else np.asarray(window, dtype=np.float32)
    A = np.zeros((3, x.shape[1], K1))
    t = np.arange(N) - (N - 1) / 2.0
    for s in range(n_seg):
        seg = x[s * step:s * step + N]
        if detrend in ("linear", "constant"):
            m = seg.mean(axis=0)
            b = (seg * t[:, None]).sum(axis=0) / (t * t).sum() if detrend == "linear" else 0.0
            seg = seg - (m + b * t[:, None])
        elif detrend not in ("none", None, False):
            raise ValueError(detrend)
        dr, di = seg.real.astype(np.float32), seg.imag.astype(np.float32)
        e = np.empty(seg.shape, dtype=np.complex64)
        e.real, e.imag = dr * w[:, None], di * w[:, None]          # float32 products
        assert (dr * w[:, None]).dtype == np.float32
        Z = _fft_c64(e).astype(np.complex128)
        Zm = np.conj(Z[(N - np.arange(K1)) % N])
        X, Y = (Z[:K1] + Zm) / 2.0, (Z[:K1] - Zm) / 2.0j
        A[0] += (np.abs(X) ** 2).T.astype(np.float32)
        A[1] += (np.abs(Y) ** 2).T.astype(np.float32)
        A[2] += (X * np.conj(Y)).real.T.astype(np.float32)
    w64 = w.astype(np.float64)
    return A, n_seg, float((w64 * w64).sum())


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
    estimator = staticmethod(accumulators)

    def __init__(self, rows, nperseg, step, detrend="linear", window=None):
        self.nperseg, self.step = nperseg, step
        self.A, self.n_seg, self.sum_w2 = self.estimator(rows, nperseg, step, detrend, window)
        self.mean = mean_of(rows, nperseg, step)

    def psd(self, mode, fs=1.0, gain=None):
        return psd_from(self.A, self.n_seg, self.sum_w2, gain_of(mode, self.mean, gain), self.nperseg, fs)


class Model(Oracle):
    """The float32 model of the contract (accumulators32) behind the oracle's face."""
    estimator = staticmethod(accumulators32)


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


# ---- the grid: every segment kernel x every detrend x the default and a caller's window -------------------------------
# nperseg: (n_ch, step).  The ten nperseg are the ten instantiations of welch_segment_kernel; the steps include N/8, N
# and values that are no power of two; the odd channel counts put different channels into the slots of one workgroup
# (below 1024 points a workgroup takes 1024 / nperseg segments) and leave the last workgroup partly empty.
GRID_SHAPES = {16: (3, 2), 32: (3, 4), 64: (5, 40), 128: (5, 100), 256: (3, 256), 512: (3, 64), 1024: (2, 1024),
               2048: (2, 1000), 4096: (2, 512), 8192: (2, 4096)}
DETRENDS = ("linear", "constant", "none")
WINDOWS = ("hann", "own")
GRID = [(N, d, w) for N in GRID_SHAPES for d in DETRENDS for w in WINDOWS]
GRID_SEED, GRID_SIGMA = 11, 1e-3
MODEL_BAR = PARITY_BAR / 3       # the float32 model against the oracle: an input the model resolves worse is not a fair one
DISTINCT = 100 * PARITY_BAR      # two variants of one case differ by more than this on some bin


def grid_total(nperseg):
    return nperseg + 9 * GRID_SHAPES[nperseg][1] + 3


def own_window(nperseg):
    """A caller's window that a reversed or shifted tap index, a lost sign or |w| would change: asymmetric, with
    negative taps and a zero tap.  float32."""
    n = np.arange(nperseg)
    w = hann32(nperseg).astype(np.float64) * (0.5 + n / nperseg) * np.where(n % 5 == 2, -1.0, 1.0)
    w[3] = 0.0
    return w.astype(np.float32)


def grid_window(nperseg, window):
    return {"hann": None, "own": own_window(nperseg)}[window]


_grid_memo = {}


def _memo(key, make):
    if key not in _grid_memo:
        _grid_memo[key] = make()
    return _grid_memo[key]


def grid_rows(nperseg, detrend):
    """The rows of a grid case, made once; nobody writes to them.  linear and constant share theirs: a carrier of 1 and a ramp of
    four sigma per segment, which the constant detrend leaves in and the linear one removes.  Without a detrend a
    carrier stays in bins 0 and 1 and the ROTATE / DBC read subtracts two large numbers in the quadrature: the float32
    MODEL misses the bar there with a carrier of 0.2 sigma (1.5e-5 at 4096 points), so that input has no carrier and no
    slope (the model: 5e-7)."""
    bare = detrend == "none"

    def make():
        return noise_rows(grid_total(nperseg), GRID_SHAPES[nperseg][0], GRID_SEED, carrier=0.0 if bare else 1.0, sigma=GRID_SIGMA,
                          slope=0.0 if bare else 4.0 * GRID_SIGMA / nperseg)
    return _memo(("rows", nperseg, bare), make)


def _grid_oracle(kind, nperseg, rows_of, detrend, window):
    """Oracle or Model of (detrend, window) on the rows of the grid's `rows_of` cases."""
    return _memo((kind.__name__, nperseg, rows_of == "none", detrend, window),
                 lambda: kind(grid_rows(nperseg, rows_of), nperseg, GRID_SHAPES[nperseg][1], detrend, grid_window(nperseg, window)))


def grid_case(nperseg, detrend, window):
    """(rows, oracle) of a grid case."""
    return grid_rows(nperseg, detrend), _grid_oracle(Oracle, nperseg, detrend, detrend, window)


def rel_diff(a, b):
    """Worst per-bin difference of two spectra over the smaller of the two."""
    return float(np.max(np.abs(a - b) / np.minimum(np.abs(a), np.abs(b))))


def grid_precondition(nperseg, detrend, window, fs=1.0):
    """What must hold of a grid case before the device is asked to meet the bar on it; looks at the oracle and the model
    only.  {"floor": the smallest floor_ratio over the modes (> 0.01: every bin carries noise), "model": the float32
    model against the oracle, worst bin over the modes (<= MODEL_BAR), "distinct": the smallest of the worst-bin
    differences between this case's raw spectrum and that of the same rows under each other detrend and under the other
    window (> DISTINCT: a kernel that ignores the flag or the window cannot pass), "ok"}."""
    def make():
        o = _grid_oracle(Oracle, nperseg, detrend, detrend, window)
        m = _grid_oracle(Model, nperseg, detrend, detrend, window)
        gain = some_gain(GRID_SHAPES[nperseg][0])
        want = {mode: o.psd(mode, fs=fs, gain=gain) for mode in MODES}
        floor = min(floor_ratio(want[mode]) for mode in MODES)
        model = max(rel_err(m.psd(mode, fs=fs, gain=gain), want[mode]) for mode in MODES)
        others = [(d, window) for d in DETRENDS if d != detrend] + [(detrend, w) for w in WINDOWS if w != window]
        distinct = min(rel_diff(_grid_oracle(Oracle, nperseg, detrend, d, w).psd("raw", fs=fs), want["raw"]) for d, w in others)
        return {"floor": floor, "model": model, "distinct": distinct,
                "ok": bool(floor > 0.01 and model <= MODEL_BAR and distinct > DISTINCT)}
    return _memo(("pre", nperseg, detrend, window, fs), make)
