"""Shared by the trigger tests: a numpy float32 model of the contract in include/gsdr.h ("trigger on the device") that
keeps the whole stream and evaluates the definitions literally, and the seeded cases every suite runs.

A case: background 0.1 * (N(0,1) + i N(0,1)), levels {0, 0, 1, 0, -1, 1} (q = the real part, thresholds -1 / +1), pulses
planted by (row, channel, amplitude).  The builder asserts max |q| of the background < 0.9, so that only planted samples
hit: a case can neither pass by producing no events nor fail because of a noise hit."""
import numpy as np

EVENT_DTYPE = np.dtype([("row", "<i8"), ("channel", "<i4"), ("side", "<i4"), ("q", "<f4"), ("n_hit", "<i4")])
LEVEL_DTYPE = np.dtype([("bx", "<f4"), ("by", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("lo", "<f4"), ("hi", "<f4")])


def default_levels(n_ch, off=()):
    lv = np.zeros(n_ch, dtype=LEVEL_DTYPE)
    lv["dx"], lv["lo"], lv["hi"] = 1.0, -1.0, 1.0
    for c in off:
        lv["lo"][c], lv["hi"][c] = -np.inf, np.inf
    return lv


def quantity(rows, lv):
    """q [n][n_ch] in float32, one rounding per operation (numpy float32 arithmetic does not fuse)."""
    f = np.ascontiguousarray(rows, dtype=np.complex64).view(np.float32).reshape(rows.shape[0], rows.shape[1], 2)
    with np.errstate(all="ignore"):
        t0 = f[:, :, 0] - lv["bx"][None, :]
        t1 = f[:, :, 1] - lv["by"][None, :]
        p0 = t0 * lv["dx"][None, :]
        p1 = t1 * lv["dy"][None, :]
        q = p0 + p1
    assert q.dtype == np.float32
    return q


class Model:
    """The definitions, literally, on the whole stream kept in memory."""

    def __init__(self, n_ch, pre, post, holdoff, max_events, levels):
        self.n_ch, self.pre, self.post, self.holdoff, self.max_events = n_ch, pre, post, holdoff, max_events
        self.levels = np.array(levels, dtype=LEVEL_DTYPE)
        self.reset()

    def reset(self):
        self.rows = np.zeros((0, self.n_ch), dtype=np.complex64)
        self.rec = np.zeros(0, dtype=EVENT_DTYPE)        # per row; n_hit == 0: the row does not hit
        self.would_emit = 0                              # triggers a feed would have emitted, written or not

    def set_levels(self, levels):
        self.levels = np.array(levels, dtype=LEVEL_DTYPE)

    def _records(self, rows, R0):
        q = quantity(rows, self.levels)
        with np.errstate(all="ignore"):
            up = q > self.levels["hi"][None, :]
            dn = ~up & (q < self.levels["lo"][None, :])
        hit = up | dn
        rec = np.zeros(rows.shape[0], dtype=EVENT_DTYPE)
        for i in range(rows.shape[0]):
            rec["row"][i] = R0 + i
            cs = np.flatnonzero(hit[i])
            if len(cs):
                c = cs[0]
                rec[i] = (R0 + i, c, 1 if up[i, c] else -1, q[i, c], len(cs))
        return rec

    def feed(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        R0 = self.rows.shape[0]
        self.rows = np.concatenate([self.rows, rows])
        self.rec = np.concatenate([self.rec, self._records(rows, R0)])   # made once, with the levels of this feed
        R1 = self.rows.shape[0]
        hit = self.rec["n_hit"] > 0
        S = self.pre + self.post
        events, snippets, dropped = [], [], 0
        for r in range(max(R0 - self.post + 1, 0), R1 - self.post + 1):       # R0 <= r + post - 1 < R1
            if not hit[r] or hit[max(0, r - self.holdoff):r].any():
                continue
            if r < self.pre:
                continue
            self.would_emit += 1
            if len(events) >= self.max_events:
                dropped += 1
                continue
            events.append(self.rec[r])
            snippets.append(self.rows[r - self.pre:r + self.post])
        ev = np.array(events, dtype=EVENT_DTYPE) if events else np.zeros(0, dtype=EVENT_DTYPE)
        sn = np.stack(snippets) if snippets else np.zeros((0, S, self.n_ch), dtype=np.complex64)
        return ev, sn, dropped


def same_bits(a, b):
    """Equality of two arrays as the integers of their bytes (NaN payloads and -0 included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Case:
    def __init__(self, name, n_ch, pre, post, holdoff, max_events, n_rows, pulses, cuts, off=(), seed=0, special=None):
        self.name, self.n_ch, self.pre, self.post, self.holdoff, self.max_events = name, n_ch, pre, post, holdoff, max_events
        self.cuts = [list(c) for c in cuts]
        assert all(sum(c) == n_rows for c in self.cuts), name
        self.max_rows = max(max(c) for c in self.cuts)
        self.levels = default_levels(n_ch, off)
        rng = np.random.default_rng(seed)
        bg = (0.1 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))).astype(np.complex64)
        assert np.abs(quantity(bg, self.levels)).max() < 0.9, name
        self.rows = bg.copy()
        for (r, c, a) in pulses:
            self.rows[r, c] += np.float32(a)
        if special:
            special(self.rows)
        self.pulses = list(pulses)

    def model(self):
        return Model(self.n_ch, self.pre, self.post, self.holdoff, self.max_events, self.levels)

    def feeds(self, cut):
        at = 0
        for n in cut:
            yield self.rows[at:at + n]
            at += n

    def expected(self, cut):
        """[(events, snippets, dropped)] per feed, by the model."""
        m = self.model()
        return [m.feed(x) for x in self.feeds(cut)]


PLANTED = [(1, 0, 2), (9, 2, 2), (11, 1, 2), (15, 3, 3), (31, 0, 2), (32, 1, 2), (40, 4, 5), (47, 3, -2), (47, 1, -2), (63, 2, 2)]
PLANTED_CUTS = [[64], [32, 32], [1] * 64, [7] * 9 + [1], [3, 0, 29, 32], [31, 1, 1, 31]]


def _special(rows):
    """NaN, +-Inf, -0 and denormal samples inside the snippets of the planted pulses and under the thresholds."""
    f = rows.view(np.float32).reshape(rows.shape[0], rows.shape[1], 2)
    nan_payload = np.array([0x7fc12345], dtype=np.uint32).view(np.float32)[0]
    f[8, 0, 0] = nan_payload               # q is NaN: never a hit
    f[8, 1, 1] = np.nan                    # NaN * dy (0): q NaN
    f[10, 3, 1] = np.inf                   # Inf * 0 = NaN in q: no hit
    f[14, 4, 0] = np.inf                   # a switched-off channel: q = +Inf is not > +Inf
    f[14, 0, 0] = -0.0
    f[16, 2, 0] = np.float32(1e-45)
    f[16, 2, 1] = np.float32(-1e-39)
    f[30, 1, 1] = -np.inf
    f[46, 0, 0] = -0.0
    f[46, 0, 1] = -0.0
    f[52, 2, 0] = np.inf                   # a hit with q = +Inf
    f[58, 0, 0] = -np.inf                  # a hit with q = -Inf, side -1


def _grid_pulses(n_ch, n_rows, seed):
    rng = np.random.default_rng(1000 + seed)
    rows = sorted(set(int(r) for r in rng.integers(0, n_rows, 14)) | {0, 3, n_rows - 1, n_rows // 2, n_rows // 2 + 1})
    pulses = []
    for k, r in enumerate(rows):
        c = int(rng.integers(0, n_ch))
        pulses.append((r, c, 2 if k % 3 else -2))
        if k % 4 == 0 and n_ch > 1:
            pulses.append((r, (c + 1 + int(rng.integers(0, n_ch - 1))) % n_ch, 3))
    return pulses


def build_cases():
    cases = [
        Case("planted", 5, 2, 4, 3, 8, 64, PLANTED, PLANTED_CUTS, off=(4,)),
        Case("planted_overflow", 5, 2, 4, 3, 2, 64, PLANTED, [[64]], off=(4,)),
        Case("special", 5, 2, 4, 3, 8, 64, PLANTED, [[64], [32, 32], [7] * 9 + [1]], off=(4,), special=_special),
    ]
    k = 0
    for n_ch in (1, 5, 64, 65, 200):
        for (pre, post, holdoff) in ((0, 1, 0), (2, 4, 3), (5, 1, 0), (0, 70, 100)):
            k += 1
            n = 150
            cuts = [[n], [7] * 21 + [3], [64, 64, 22], [1] * 9 + [0] + [141]]
            cases.append(Case(f"grid_{n_ch}_{pre}_{post}_{holdoff}", n_ch, pre, post, holdoff, 32, n, _grid_pulses(n_ch, n, k), cuts,
                              off=(n_ch - 1,) if n_ch > 1 else (), seed=k))
    # more than 256 channels: trigger_hits_wide_kernel takes a row in two steps; hits in the second step, and in both
    cases.append(Case("wide_300", 300, 2, 4, 3, 16, 40, [(5, 299, 2), (12, 7, -2), (12, 280, 3), (20, 256, 2), (20, 255, 2),
                                                          (30, 63, 2), (30, 64, 2), (30, 290, -2)], [[40], [13, 27]], seed=91))
    cases.append(Case("thousand", 5, 3, 5, 10, 64, 2000, [(r, r % 5, 2) for r in range(5, 2000, 61)],
                      [[1000, 1000], [1000, 0, 1, 7, 64, 928]], seed=77))
    every7 = [(r, r % 3, 2) for r in range(3, 5000, 7)]
    for holdoff in (6, 7):
        cases.append(Case(f"every7_holdoff{holdoff}", 3, 1, 2, holdoff, 1024, 5000, every7,
                          [[5000], [1000] * 5, [999, 1001, 3000]], seed=5))
    return cases


CASES = build_cases()
CASE_IDS = [c.name for c in CASES]
