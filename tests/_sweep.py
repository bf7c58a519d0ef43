"""A numpy / float64 model of the sweep accumulator's contract (include/gsdr.h, "VNA sweep accumulator on the device"),
the cuttings of a stream into feeds, and the run helpers for the host twin and the device.  Plain module: no GPU work
and no library call at import time.

The model follows the contract operation for operation -- sequential double sums per accumulator, one division and one
rounding for a mean, the fused multiply-add of the variance exactly (fractions.Fraction, rounded once to double), the
slope's terms and block order -- so device and twin are compared with it bit for bit."""
from fractions import Fraction

import numpy as np

SLOPE_BLOCK = 256

# (n_ch, n_points, group): the shapes of tests/test_sweep_host.py, and what tests/test_gpu_sweep.py adds
SHAPES = [(1, 5, 1), (3, 67, 1), (16, 1000, 1), (2, 250, 40), (1, 7, 3)]
GPU_SHAPES = SHAPES + [(1030, 3, 1), (4, 200, 64)]
FIRST_ROWS = (0, 3, (1 << 40) + 17)


def total_for(n_points, group):
    """Rows of a test stream: two passes and an uneven part of a third, so that the counts are unequal."""
    W = n_points * group
    return 2 * W + (W * 3) // 7 + 1


def rows_of(total, n_ch, seed=5):
    """A carrier per channel (different levels and signs) and noise at 1e-2 of it, complex64 [total][n_ch]."""
    rng = np.random.default_rng(seed)
    level = (0.3 + 0.05 * np.arange(n_ch)) * np.exp(2j * np.pi * np.arange(n_ch) / 7.0)
    x = level[None, :] + 3e-3 * (rng.standard_normal((total, n_ch)) + 1j * rng.standard_normal((total, n_ch)))
    return x.astype(np.complex64)


def point_of_rows(first_row, total, n_points, group):
    """p(r) for r in [first_row, first_row + total), by enumeration in Python integers."""
    return np.array([((first_row + i) // group) % n_points for i in range(total)], dtype=np.int64)


def counts_by_enumeration(first_row, total, n_points, group):
    return np.bincount(point_of_rows(first_row, total, n_points, group), minlength=n_points).astype(np.int64)


def counts_closed(first_row, total, n_points, group):
    """The contract's closed form, in Python integers."""
    W = n_points * group

    def below(x, p):
        return (x // W) * group + min(max(x % W - p * group, 0), group)
    return np.array([below(first_row + total, p) - below(first_row, p) for p in range(n_points)], dtype=np.int64)


def accumulate(x, n_points, group, first_row):
    """(S, Q): complex128 [n_points][n_ch] each (re and im are separate doubles), every accumulator summed in stream
    order from +0, one addition per row.  Rows of equal rank within their point go in one vector step: they belong to
    different accumulators."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    total, n_ch = x.shape
    p = point_of_rows(first_row, total, n_points, group)
    order = np.argsort(p, kind="stable")
    ps = p[order]
    starts = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]]) if total else np.zeros(0, dtype=np.int64)
    rank = np.empty(total, dtype=np.int64)
    rank[order] = np.arange(total) - np.repeat(starts, np.diff(np.r_[starts, total]))
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    S, Q = np.zeros((2, n_points, n_ch)), np.zeros((2, n_points, n_ch))      # [re, im][point][channel]
    with np.errstate(all="ignore"):
        for j in range(int(rank.max()) + 1 if total else 0):
            at = np.flatnonzero(rank == j)
            S[0][p[at]] += xr[at]
            S[1][p[at]] += xi[at]
            Q[0][p[at]] += xr[at] * xr[at]
            Q[1][p[at]] += xi[at] * xi[at]
    return S, Q


def fma64(a, b, c):
    """round(a b + c) to double, once; non-finite operands take the plain expression (the same Inf / NaN)."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        return 0.0 if not (a * b == 0 and np.signbit(a * b) and np.signbit(c)) else -0.0
    return float(exact)


def read_model(S, Q, n):
    """(mean, var) complex64 [n_points][n_ch] from the sums and the counts n [n_points]."""
    mean = np.zeros(S[0].shape, dtype=np.complex64)
    var = np.zeros(S[0].shape, dtype=np.complex64)
    with np.errstate(all="ignore"):
        for k, part in enumerate(("real", "imag")):
            m = np.zeros(S[k].shape, dtype=np.float32)
            v = np.zeros(S[k].shape, dtype=np.float32)
            for p in range(S[k].shape[0]):
                if n[p] == 0:
                    continue
                nn = np.float64(n[p])
                m[p] = (S[k][p] / nn).astype(np.float32)
                if n[p] > 1:
                    for c in range(S[k].shape[1]):
                        s, q = S[k][p, c], Q[k][p, c]
                        w = np.float64(fma64(-s, s / nn, q)) / (nn - 1.0)
                        v[p, c] = np.float32(w if not (w < 0) else 0.0)
            getattr(mean, part)[...] = m
            getattr(var, part)[...] = v
    return mean, var


def sequential_sum(t):
    """t[0] + t[1] + ... from +0, one double addition after another"""
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in t:
            s = s + v
    return s


def slope_model(mean):
    """D[c], complex128 [n_ch], from the float32 means: terms in ascending p from +0 inside blocks of 256, block sums in
    ascending order from block 0's."""
    m = np.asarray(mean, dtype=np.complex64)
    n_points, n_ch = m.shape
    a, b = m.real[1:].astype(np.float64), m.imag[1:].astype(np.float64)
    c, d = m.real[:-1].astype(np.float64), m.imag[:-1].astype(np.float64)
    with np.errstate(all="ignore"):
        tx, ty = a * c + b * d, b * c - a * d
    out = np.zeros(n_ch, dtype=np.complex128)
    for ch in range(n_ch):
        sums = []
        for first in range(0, max(n_points - 1, 1), SLOPE_BLOCK):
            sums.append((sequential_sum(tx[first:first + SLOPE_BLOCK, ch]), sequential_sum(ty[first:first + SLOPE_BLOCK, ch])))
        sx, sy = sums[0]
        with np.errstate(all="ignore"):
            for bx, by in sums[1:]:
                sx, sy = sx + bx, sy + by
        out[ch] = complex(sx, sy)
    return out


def model(x, n_points, group, first_row):
    """(mean, var, D, n) of the whole stream x."""
    n = counts_closed(first_row, x.shape[0], n_points, group)
    S, Q = accumulate(x, n_points, group, first_row)
    mean, var = read_model(S, Q, n)
    return mean, var, slope_model(mean), n


def cuttings(total, pass_rows, ones_cap=4000):
    """name -> feed lengths that add up to `total`: one feed, single rows, sevens, feeds with empty ones between, and one
    feed longer than two passes.  Streams longer than ones_cap rows are fed row by row for their first ones_cap rows."""
    assert total > 2 * pass_rows + 1
    ones = [1] * min(total, ones_cap) + ([total - ones_cap] if total > ones_cap else [])
    sevens = [min(7, total - at) for at in range(0, total, 7)]
    a = min(3, total)
    b = min(pass_rows + 1, total - a)
    gaps = [0, a, 0, 0, b, 0, total - a - b, 0]
    return {"whole": [total], "ones": ones, "sevens": sevens, "gaps": gaps, "long": [1, 2 * pass_rows + 1, total - 2 * pass_rows - 2]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(got, want):
    """(mean, var, D) against (mean, var, D), bit for bit"""
    return all(same_bits(g, w) for g, w in zip(got[:3], want[:3]))


def run_host(sweep, x, n_points, group, first_row=0, cut=None):
    """(mean, var, D, n, sweeps) of the host twin fed x cut as `cut` (None: one feed)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    s = sweep.host_sweep(x.shape[1], n_points, group, first_row)
    at = 0
    for n in ([x.shape[0]] if cut is None else cut):
        s.feed(x[at:at + n])
        at += n
    assert at == x.shape[0] == s.rows_seen
    mean, var = s.read(variance=True)
    out = (mean, var, s.slope(), s.counts(), s.sweeps)
    assert same_bits(s.read(), mean)                       # without the variance: the same means
    s.close()
    return out


def run_device(sweep, x, n_points, group, dev, first_row=0, cut=None, stream=None):
    """The same from a device_sweep: the stream is uploaded once, the feeds are views of it."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.complex64)
    xd = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()
    s = sweep.device_sweep(x.shape[1], n_points, group, first_row, device_index=0)
    at = 0
    for n in ([x.shape[0]] if cut is None else cut):
        s.feed_device(xd[at:at + n], stream=stream)
        at += n
    assert at == x.shape[0] == s.rows_seen
    mean, var = s.read(variance=True, stream=stream)
    out = (mean, var, s.slope(stream=stream), s.counts(), s.sweeps)
    s.close()
    return out
