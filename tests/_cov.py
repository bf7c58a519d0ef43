"""A bit model of the channel covariance's contract (include/gsdr.h, "channel covariance on the device"), the stream
makers and the helpers the CPU and GPU tests share.

The projection is plain float32 numpy (numpy fuses nothing); d = float64(v) - pivot is one numpy operation; a chain's S
is a strictly ordered sum; every fma of the law -- one per row and cell, and the one of the covariance -- is exact in
rationals (fractions.Fraction) and rounded once to double, as tests/_resmap.py does it; the tree and the rest of the
read laws are single numpy operations.

Ordinary noise around a pivot at the carrier sums almost exactly in double, so it cannot see a wrong order of the
additions.  ``stream`` therefore can make WIDE variables: N(0, 1) 2^e with e uniform in [-20, 20], whose sums round at
almost every step and differ from one order to the next.
"""
import numpy as np

from _resmap import _fma
from _stats import cuttings, feed_cut, same_doubles  # noqa: F401  (the cuttings are the stats object's)

AXIS_DTYPE = np.dtype([("channel", "<i4"), ("bx", "<f4"), ("by", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("reserved", "<i4"), ("pivot", "<f8")])
f32, f64 = np.float32, np.float64
KINDS = ("sums", "cov", "corr")


def project(rows, axes):
    """v, float32 [n][n_var]: the five float32 operations of the trigger's q on the channel of each variable."""
    x = np.ascontiguousarray(rows, dtype=np.complex64)[:, axes["channel"]]
    with np.errstate(all="ignore"):
        t0 = x.real.astype(f32) - axes["bx"]
        t1 = x.imag.astype(f32) - axes["by"]
        p0 = t0 * axes["dx"]
        p1 = t1 * axes["dy"]
        return (p0 + p1).astype(f32)


def _tree(X):
    """the halving tree over axis 0 (a power of two long)"""
    h = X.shape[0] // 2
    with np.errstate(all="ignore"):
        while h >= 1:
            X = X[:h] + X[h:2 * h]
            h //= 2
    return X[0]


class Model:
    """The whole stream at once (no result depends on the cutting): the joined sums and the three reads."""

    def __init__(self, rows, axes, lanes):
        rows = np.ascontiguousarray(rows, dtype=np.complex64)
        self.n, self.n_var, self.lanes, self.axes = rows.shape[0], axes.shape[0], lanes, axes
        with np.errstate(all="ignore"):
            d = project(rows, axes).astype(f64) - axes["pivot"]
        nv = self.n_var
        S = np.zeros((lanes, nv), dtype=f64)
        G = np.zeros((lanes, nv, nv), dtype=f64)                  # the cells j <= i
        for r in range(self.n):
            k = r % lanes
            with np.errstate(all="ignore"):
                S[k] = S[k] + d[r]
            for i in range(nv):
                for j in range(i + 1):
                    G[k, i, j] = _fma(float(d[r, i]), float(d[r, j]), float(G[k, i, j]))
        self.S, self.G = _tree(S), _tree(G)

    def read(self, kind):
        """(out [n_var][n_var], mean [n_var]) of kind "sums", "cov" or "corr"."""
        nv, n, S, G = self.n_var, self.n, self.S, self.G
        out = np.full((nv, nv), np.nan, dtype=f64)
        if kind == "sums":
            for i in range(nv):
                for j in range(i + 1):
                    out[i, j] = out[j, i] = G[i, j]
            return out, S.copy()
        with np.errstate(all="ignore"):
            mean = self.axes["pivot"] + S / f64(n) if n >= 1 else np.full(nv, np.nan)
            C = np.full((nv, nv), np.nan, dtype=f64)
            if n >= 2:
                m = S / f64(n)
                for i in range(nv):
                    for j in range(i + 1):
                        c = f64(_fma(-float(S[i]), float(m[j]), float(G[i, j]))) / (f64(n) - f64(1.0))
                        if i == j and c < 0.0:
                            c = f64(0.0)
                        C[i, j] = c
            if kind == "cov":
                for i in range(nv):
                    for j in range(i + 1):
                        out[i, j] = out[j, i] = C[i, j]
                return out, mean
            s = np.sqrt(np.diagonal(C))
            for i in range(nv):
                for j in range(i + 1):
                    if i == j:
                        v = f64(1.0) if np.isfinite(C[i, i]) and C[i, i] > 0 else f64(np.nan)
                    else:
                        p = s[i] * s[j]
                        v = C[i, j] / p
                    out[i, j] = out[j, i] = v
        return out, mean


def read_all(obj, **kw):
    """{kind: (out, mean)} of a host_cov or a device_cov"""
    return {k: obj.read(k, **kw) for k in KINDS}


def same_reads(got, want):
    """"" or the first kind and array that differs, bit for bit, a NaN matching any NaN"""
    for k in KINDS:
        for name, a, b in (("out", got[k][0], want[k][0]), ("mean", got[k][1], want[k][1])):
            if not same_doubles(a, b):
                a, b = np.asarray(a), np.asarray(b)
                at = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).reshape(-1))
                return f"{k}.{name}[{at[0] if at.size else '?'}]: {a.reshape(-1)[at[0]]!r} != {b.reshape(-1)[at[0]]!r}" if at.size else f"{k}.{name}: signs of zero"
    return ""


def stream(n, n_ch, seed=1, wide=(), share=0.5):
    """(rows complex64 [n][n_ch], carriers complex128 [n_ch]): per channel a carrier with real and imaginary part in
    0.2 - 0.5 and Gaussian noise at 1e-3 of the carrier, `share` of whose variance is common to all channels (per
    quadrature), so that the correlations between channels lie around `share`.  Channels in `wide` carry N(0, 1) 2^e
    instead, e uniform in [-20, 20], around 0: their sums round at every step."""
    rng = np.random.default_rng(seed)
    carriers = rng.uniform(0.2, 0.5, size=n_ch) + 1j * rng.uniform(0.2, 0.5, size=n_ch)
    common = rng.normal(size=(n, 1)) + 1j * rng.normal(size=(n, 1))
    own = rng.normal(size=(n, n_ch)) + 1j * rng.normal(size=(n, n_ch))
    noise = np.sqrt(share) * common + np.sqrt(1.0 - share) * own
    rows = carriers + 1e-3 * (noise.real * carriers.real + 1j * noise.imag * carriers.imag)
    rows = rows.astype(np.complex64)
    for c in wide:
        e = rng.integers(-20, 21, size=n)
        rows[:, c] = (rng.normal(size=n) * 2.0 ** e).astype(f32) + 1j * (rng.normal(size=n) * 2.0 ** e).astype(f32)
        carriers[c] = 0.0
    return np.ascontiguousarray(rows), carriers


def axes_of(channels, quadrature="re", carriers=None):
    """AXIS_DTYPE axes: the real part, the imaginary part or both (re of every channel first) of `channels`, the pivots
    at the float32 of the carriers (None: 0)."""
    ch = np.asarray(channels, dtype=np.int32).reshape(-1)
    parts = {"re": [(1.0, 0.0)], "im": [(0.0, 1.0)], "both": [(1.0, 0.0), (0.0, 1.0)]}[quadrature]
    ax = np.zeros(len(parts) * ch.shape[0], dtype=AXIS_DTYPE)
    for k, (dx, dy) in enumerate(parts):
        part = ax[k * ch.shape[0]:(k + 1) * ch.shape[0]]
        part["channel"], part["dx"], part["dy"] = ch, dx, dy
        if carriers is not None:
            c = np.asarray(carriers)[ch]
            part["pivot"] = (c.real if dx else c.imag).astype(f32).astype(f64)
    return ax


def distances(rows, axes, cov, corr, keep):
    """The distances to numpy of a COV and a CORR read on the variables `keep`:
    max |C - numpy.cov| / sqrt(C_ii C_jj) and max |rho - numpy.corrcoef| (of the float64 of the float32 projections)."""
    v = project(rows, axes).astype(f64)[:, keep]
    ref, rho = np.atleast_2d(np.cov(v, rowvar=False)), np.atleast_2d(np.corrcoef(v, rowvar=False))
    C, R = cov[np.ix_(keep, keep)], corr[np.ix_(keep, keep)]
    scale = np.sqrt(np.outer(np.diagonal(ref), np.diagonal(ref)))
    return float((np.abs(C - ref) / scale).max()), float(np.abs(R - rho).max())
