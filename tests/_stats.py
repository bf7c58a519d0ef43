"""A numpy bit model of the row statistics' contract (include/gsdr.h, "row statistics on the device"), the stream makers
and the cuttings the CPU and GPU tests share.

Every operation of the model is one plain float32 / float64 numpy operation on arrays (numpy fuses nothing), in the
order the header states: the law has no fused operation, so no rational arithmetic is needed.  A chain's sums are
``numpy.cumsum`` along the rows of the chain: cumsum adds strictly in order (unlike ``numpy.sum``, which adds in pairs).

Ordinary noise sums EXACTLY in double -- a few thousand float32 of one magnitude never round -- so it cannot see a wrong
order of the additions.  ``stream`` therefore has a WIDE kind: N(0, 1) 2^e with e uniform in [-20, 20], whose sums round
at almost every step and differ from one order to the next (``lanes`` 64, 16 and 1 give different means).
"""
import numpy as np

LEVEL_DTYPE = np.dtype([("bx", "<f4"), ("by", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("lo", "<f4"), ("hi", "<f4")])
f32, f64 = np.float32, np.float64


def project(rows, axes):
    """q, float32 [n][n_ch]: five float32 operations, as the trigger's."""
    x = np.ascontiguousarray(rows, dtype=np.complex64)
    with np.errstate(all="ignore"):
        t0 = x.real.astype(f32) - axes["bx"]
        t1 = x.imag.astype(f32) - axes["by"]
        p0 = t0 * axes["dx"]
        p1 = t1 * axes["dy"]
        return (p0 + p1).astype(f32)


def constants(axes, n_bins):
    """p, inv_w, w in double, as the host derives them once."""
    lo, hi = axes["lo"].astype(f64), axes["hi"].astype(f64)
    return f64(0.5) * (lo + hi), f64(n_bins) / (hi - lo), (hi - lo) / f64(n_bins)


def _earlier_min(a, b):
    return np.where(b < a, b, a)


def _earlier_max(a, b):
    return np.where(b > a, b, a)


class Model:
    """The whole stream at once (no result depends on the cutting): counts, summaries and quantiles of the contract."""

    def __init__(self, rows, axes, n_bins, lanes):
        rows = np.ascontiguousarray(rows, dtype=np.complex64)
        n, n_ch = rows.shape
        self.n_ch, self.n_bins, self.lanes, self.axes = n_ch, n_bins, lanes, axes
        self.p, self.inv_w, self.w = constants(axes, n_bins)
        q = self.q = project(rows, axes)
        ok = self.ok = np.isfinite(q)
        # bins
        lo64 = axes["lo"].astype(f64)
        with np.errstate(all="ignore"):
            k = np.floor((np.where(ok, q, axes["lo"]).astype(f64) - lo64) * self.inv_w)
        slot = np.where(k >= n_bins, n_bins + 1, 1 + np.minimum(k, n_bins).astype(np.int64))
        slot = np.where(q < axes["lo"], 0, slot)
        slot = np.where(ok, slot, n_bins + 2)
        self.counts = np.zeros((n_ch, n_bins + 3), dtype=np.uint64)
        for c in range(n_ch):
            self.counts[c] = np.bincount(slot[:, c], minlength=n_bins + 3).astype(np.uint64)
        # chains: row r -> chain r mod lanes; a sample that is not finite adds +0 (which changes no sum) and is no extreme
        steps = -(-n // lanes) if n else 0
        d = np.zeros((steps * lanes, n_ch), dtype=f64)
        d[:n] = np.where(ok, q.astype(f64) - self.p, 0.0)
        dd = d * d
        d, dd = d.reshape(steps, lanes, n_ch), dd.reshape(steps, lanes, n_ch)
        S = np.cumsum(d, axis=0)[-1] if steps else np.zeros((lanes, n_ch))
        Q = np.cumsum(dd, axis=0)[-1] if steps else np.zeros((lanes, n_ch))
        qm = np.full((steps * lanes, n_ch), np.nan, dtype=f32)
        qm[:n] = np.where(ok, q, f32(np.nan))
        qm = qm.reshape(steps, lanes, n_ch)
        mn, mx = np.full((lanes, n_ch), np.inf, dtype=f32), np.full((lanes, n_ch), -np.inf, dtype=f32)
        for s in range(steps):                                    # a NaN is neither < nor >: it leaves both
            mn, mx = _earlier_min(mn, qm[s]), _earlier_max(mx, qm[s])
        # the halving tree
        h = lanes // 2
        while h >= 1:
            S, Q = S[:h] + S[h:2 * h], Q[:h] + Q[h:2 * h]
            mn, mx = _earlier_min(mn[:h], mn[h:2 * h]), _earlier_max(mx[:h], mx[h:2 * h])
            h //= 2
        self.S, self.Q, self.mn, self.mx = S[0], Q[0], mn[0], mx[0]

    def summary(self):
        """dict of arrays [n_ch]: n, bad, under, over, mean, var, min, max."""
        cnt = self.counts
        under, over, bad = cnt[:, 0], cnt[:, self.n_bins + 1], cnt[:, self.n_bins + 2]
        n = under + cnt[:, 1:self.n_bins + 1].sum(axis=1, dtype=np.uint64) + over
        nd = n.astype(f64)
        with np.errstate(all="ignore"):
            m = self.S / nd
            mean = np.where(n >= 1, self.p + m, np.nan)
            v = (self.Q - self.S * m) / (nd - 1.0)
            var = np.where(n >= 2, np.where(v < 0.0, 0.0, v), np.nan)
        return dict(n=n, bad=bad, under=under, over=over, mean=mean, var=var, min=self.mn, max=self.mx)

    def quantiles(self, pr):
        pr = np.atleast_1d(np.asarray(pr, dtype=f64))
        out = np.zeros((self.n_ch, pr.shape[0]), dtype=f64)
        lo64 = self.axes["lo"].astype(f64)
        for c in range(self.n_ch):
            cnt = self.counts[c].astype(np.int64)
            under, bins = int(cnt[0]), cnt[1:self.n_bins + 1]
            n = under + int(bins.sum()) + int(cnt[self.n_bins + 1])
            cum = under + np.cumsum(bins)
            for i, p in enumerate(pr):
                if n == 0:
                    out[c, i] = np.nan
                    continue
                t = max(1, int(np.ceil(p * f64(n))))
                if under >= t:
                    out[c, i] = -np.inf
                    continue
                k = int(np.searchsorted(cum, t, side="left"))     # the first bin whose cumulative count reaches t
                if k >= self.n_bins:
                    out[c, i] = np.inf
                    continue
                C, h = int(cum[k] - bins[k]), int(bins[k])
                frac = (f64(t - C) - f64(0.5)) / f64(h)
                out[c, i] = lo64[c] + (f64(k) + frac) * self.w[c]
        return out

    def levels(self, nsigma, centre="median", on=None):
        s = self.summary()
        mid = self.quantiles([0.5])[:, 0] if centre == "median" else s["mean"]
        with np.errstate(all="ignore"):
            sigma = np.sqrt(s["var"])
            span = f64(nsigma) * sigma
            lo, hi = (mid - span).astype(f32), (mid + span).astype(f32)
        live = (s["n"] >= 2) & np.isfinite(mid) & np.isfinite(sigma)
        if on is not None:
            live &= np.asarray(on) != 0
        lv = np.zeros(self.n_ch, dtype=LEVEL_DTYPE)
        for f in ("bx", "by", "dx", "dy"):
            lv[f] = self.axes[f]
        lv["lo"], lv["hi"] = np.where(live, lo, f32(-np.inf)), np.where(live, hi, f32(np.inf))
        return lv


SUMMARY_FIELDS = ("n", "bad", "under", "over", "mean", "var", "min", "max")


def same_summary(got, want):
    """got: the library's structured array; want: Model.summary().  Bit for bit, field by field; "" or what differs."""
    for f in SUMMARY_FIELDS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f]).astype(got[f].dtype)
        if a.dtype.kind == "f":
            nan = np.isnan(a) & np.isnan(b)
            a, b = np.where(nan, 0, a).view(f"u{a.itemsize}"), np.where(nan, 0, b).view(f"u{a.itemsize}")
        if not np.array_equal(a, b):
            c = int(np.flatnonzero(a != b)[0])
            return f"{f}[{c}]: {got[f][c]!r} != {want[f][c]!r}"
    if "reserved" in got.dtype.names and got["reserved"].any():
        return "reserved bytes are not zero"
    return ""


def same_doubles(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.asarray(a, dtype=f64), np.asarray(b, dtype=f64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0, a).view(np.uint64), np.where(nan, 0, b).view(np.uint64))


def stream(n, n_ch, seed=1, wide=()):
    """(rows complex64 [n][n_ch], axes): Gaussian noise of per-channel centre and sigma around a baseline, a projection of
    its own per channel, and a range of centre -/+ 8 sigma of q.  Channels in `wide` carry N(0, 1) 2^e instead, e uniform
    in [-20, 20], in a range of -/+ 2^23: their double sums round at every step."""
    rng = np.random.default_rng(seed)
    base = (rng.normal(size=n_ch) + 1j * rng.normal(size=n_ch)).astype(np.complex64)
    sigma = (10.0 ** rng.uniform(-3, 0, size=n_ch)).astype(f32)
    ang = rng.uniform(0, 2 * np.pi, size=n_ch)
    axes = np.zeros(n_ch, dtype=LEVEL_DTYPE)
    axes["bx"], axes["by"] = base.real, base.imag
    axes["dx"], axes["dy"] = np.cos(ang), np.sin(ang)
    noise = rng.normal(size=(n, n_ch)) + 1j * rng.normal(size=(n, n_ch))
    rows = (base + noise * sigma + (0.3 + 0.1j) * sigma).astype(np.complex64)
    for c in wide:
        e = rng.integers(-20, 21, size=n)
        rows[:, c] = (rng.normal(size=n) * 2.0 ** e).astype(f32) + 1j * rng.normal(size=n).astype(f32)
        axes[c] = (0, 0, 1, 0, 0, 0)
    q = project(rows, axes).astype(f64)
    mid, sd = (q.mean(axis=0), q.std(axis=0)) if n else (np.zeros(n_ch), np.ones(n_ch))
    sd = np.where(sd > 0, sd, 1.0)
    axes["lo"], axes["hi"] = (mid - 8 * sd).astype(f32), (mid + 8 * sd).astype(f32)
    for c in wide:
        axes["lo"][c], axes["hi"][c] = -2.0 ** 23, 2.0 ** 23
    return np.ascontiguousarray(rows), axes


PIVOT_AXIS = (0, 0, 1, 0, -2.0 ** 23, 2.0 ** 23)       # q = Re x, the pivot is 0


def after_a_prefix_of_pivot_rows(T0, tail, axes, n_bins, lanes):
    """The Model of a stream no model can take: T0 rows whose q EQUALS the pivot (0 + 0j on PIVOT_AXIS), then `tail`.

    Such a row adds exactly +0 to S and Q of its chain, which leaves them +0, makes min = max = +0 and counts in one known
    bin: the chains after the prefix are those after ANY number >= 1 of such rows.  So the stream is modelled by
    z = T0 mod lanes pivot rows (z = lanes where that is 0), which put the tail's rows into the chains they have behind T0
    rows, and the T0 - z rows left out are added to the pivot's counter before anything is derived from the counts.
    (The extremes of chains that got a pivot row in the real stream only are +-Inf here; the tree joins them with a chain
    that has one, so min and max of the channel are the same -- as long as z >= 1, and no tail value is a zero of the
    other sign.)"""
    tail = np.ascontiguousarray(tail, dtype=np.complex64)
    n_ch = tail.shape[1]
    assert T0 >= 1 and np.array_equal(axes, np.array([PIVOT_AXIS] * n_ch, dtype=LEVEL_DTYPE)) and not (project(tail, axes) == 0).any()
    z = T0 % lanes or lanes
    assert z <= T0
    m = Model(np.concatenate([np.zeros((z, n_ch), dtype=np.complex64), tail]), axes, n_bins, lanes)
    slot = np.argmax(Model(np.zeros((1, n_ch), dtype=np.complex64), axes, n_bins, 1).counts, axis=1)
    assert (slot >= 1).all() and (slot <= n_bins).all()
    m.counts[np.arange(n_ch), slot] += np.uint64(T0 - z)
    m.pivot_slot = slot
    return m


def cuttings(n, max_rows):
    """name -> feed lengths that add up to n, each <= max_rows."""
    def pieces(total, m):
        return [m] * (total // m) + ([total % m] if total % m else [])
    head = min(3, n)
    cuts = {"whole": pieces(n, max_rows), "37": pieces(n, min(37, max_rows)),
            "gaps": [0, head, 0, 0] + pieces(n - head, max_rows) + [0]}
    if n <= 600:
        cuts["ones"] = [1] * n
    return cuts


def feed_cut(obj, rows, cut, to_feed=lambda r: r):
    at = 0
    for m in cut:
        obj.feed(to_feed(rows[at:at + m]))
        at += m
    assert at == rows.shape[0]
