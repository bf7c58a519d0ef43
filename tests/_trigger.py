"""Shared by the trigger tests: a numpy float32 model of the contract in include/gsdr.h ("trigger on the device") that
keeps the whole stream and evaluates the definitions literally, and the seeded cases every suite runs.

A case: background 0.1 * (N(0,1) + i N(0,1)), levels {0, 0, 1, 0, -1, 1} (q = the real part, thresholds -1 / +1), pulses
planted by (row, channel, amplitude).  The builder asserts max |q| of the background < 0.9, so that only planted samples
hit: a case can neither pass by producing no events nor fail because of a noise hit.

CASES are small (Model walks rows in Python) and run through every suite.  LARGE_CASES are the feeds of 65 536 to 2^20 rows
at which trigger_select_kernel's chunks take several steps and the row passes reach their grid caps; they are built when
first asked for and have stream_expected, the same contract evaluated on the whole stream at once, as their model."""
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


def stream_expected(rows, levels, pre, post, holdoff, max_events, cut):
    """The contract once more, on the whole stream at once (no row loop, so 10^6 rows take a moment): the
    [(events, snippets, dropped)] per feed of `cut` that Model gives, for levels that do not change.
    Hits by quantity(); triggers are the hitting rows more than `holdoff` behind the hitting row before them (the first
    one always); a trigger with r >= pre is emitted by the feed whose rows contain r + post - 1; a feed writes its first
    max_events and counts the rest."""
    rows = np.ascontiguousarray(rows, dtype=np.complex64)
    S = pre + post
    q = quantity(rows, levels)
    with np.errstate(all="ignore"):
        up = q > levels["hi"][None, :]
        dn = ~up & (q < levels["lo"][None, :])
    hit = up | dn
    hr = np.flatnonzero(hit.any(axis=1))
    first = np.ones(len(hr), dtype=bool)
    first[1:] = np.diff(hr) > holdoff
    tr = hr[first]
    tr = tr[tr >= pre]
    ends = np.cumsum(np.asarray(cut, dtype=np.int64))
    feed_of = np.searchsorted(ends, tr + post - 1, side="right")     # len(cut): its last row is not delivered yet
    ch = hit[tr].argmax(axis=1)
    ev = np.zeros(len(tr), dtype=EVENT_DTYPE)
    ev["row"], ev["channel"] = tr, ch
    ev["side"] = np.where(up[tr, ch], 1, -1)
    ev["q"] = q[tr, ch]
    ev["n_hit"] = hit[tr].sum(axis=1)
    out = []
    for k in range(len(cut)):
        a, b = (int(v) for v in np.searchsorted(feed_of, [k, k + 1]))
        w = min(b - a, max_events)
        idx = tr[a:a + w, None] - pre + np.arange(S)[None, :]
        out.append((ev[a:a + w].copy(), rows[idx].reshape(w, S, rows.shape[1]), b - a - w))
    return out


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

    def expected_vec(self, cut):
        """The same by stream_expected: the whole stream at once."""
        return stream_expected(self.rows, self.levels, self.pre, self.post, self.holdoff, self.max_events, cut)


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


def lane_width(n_ch):
    """lw of trigger_hits_kernel (n_ch <= 64): a row takes 1 << lw >= n_ch lanes, a wave 64 >> lw rows."""
    lw = 0
    while (1 << lw) < n_ch:
        lw += 1
    return lw


def _lane_pulses(n_ch):
    """Three rows in a row, the first of them the first row of a wave (where a wave holds four rows or more): the last
    channel alone, channel 0 alone, both.  A record shifted by one row inside the wave, or a segment mask one bit short,
    changes which of them hits and what their records say.  Two up / down pairs elsewhere."""
    rpw = 64 >> lane_width(n_ch)
    g0 = -(-70 // rpw) * rpw                  # rpw divides 64: the head of a row group in the cuts [150] and [64, 64, 22]
    return [(g0, n_ch - 1, 2), (g0 + 1, 0, 2), (g0 + 2, 0, -2), (g0 + 2, n_ch - 1, 3),
            (10, n_ch // 2, 2), (20, n_ch // 2, -2), (120, 0, -2), (132, n_ch - 1, 2)]


def _wide_pulses(n_ch):
    """trigger_hits_wide_kernel: wave w takes channels base + 64 w + lane of the step at `base` (256 per step).  The last
    channel alone; a higher-numbered wave's hit in step 0 against wave 0's hit in step 1 (70 / 200 against 261, or 256
    where there is no 261); both sides of the step boundary; at 513 the third step alone and with the second."""
    second = 261 if n_ch > 261 else (256 if n_ch > 256 else 255)
    p = [(5, n_ch - 1, 2), (15, 70, 2), (15, second, 3), (25, 200, -2), (25, second, 2),
         (65, 0, 2), (65, n_ch - 1, 2), (100, n_ch - 1, -2)]
    p += [(35, 255, 2), (35, 256, 2)] if n_ch > 256 else [(35, 254, 2), (35, 255, -2)]
    if n_ch > 512:
        p += [(45, 512, -2), (55, 300, 2), (55, 512, 2)]
    return p


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
    grid_cuts = [[150], [7] * 21 + [3], [64, 64, 22], [1] * 9 + [0] + [141]]
    # every lane width of trigger_hits_kernel, both sides of each power of two; holdoff 0 makes each of the three rows an
    # event, so that the record of every one of them is seen
    for k, n_ch in enumerate((2, 4, 8, 9, 16, 17, 32, 33, 63)):
        for holdoff in (3, 0):
            cases.append(Case(f"lanes_{n_ch}" + ("" if holdoff else "_h0"), n_ch, 2, 4, holdoff, 32, 150, _lane_pulses(n_ch),
                              grid_cuts, seed=200 + k))
    # the wide row pass at one step exactly, one channel into the second step, one channel into the third
    for k, n_ch in enumerate((256, 257, 513)):
        cases.append(Case(f"wide_{n_ch}", n_ch, 2, 4, 3, 32, 150, _wide_pulses(n_ch), grid_cuts, seed=300 + k))
    # both grid caps of trigger_capture_kernel: (S - 1) n_ch = 526 336 > 2^19 carried elements, max_events S n_ch =
    # 2 113 536 > 2^21 snippet elements.  Six triggers; row r is emitted by the feed that holds r + 157, so [600] drops two,
    # the second feed of [257, 257, 86] drops one, and the other cuts drop none; the 86-row feed is shorter than the carry.
    # Six snippets of 258 rows in 600 rows overlap: each is a full copy.  A name ending in "overflow" keeps the case out of
    # test_cut_invariance, which needs feeds that drop nothing.
    cases.append(Case("caps_2048_overflow", 2048, 100, 158, 3, 4, 600,
                      [(100, 2047, 2), (130, 0, -2), (190, 1024, 2), (190, 5, 2), (260, 2047, -2), (330, 255, 2), (441, 256, 2),
                       (50, 7, 2)], [[600], [300, 300], [257, 257, 86], [100] * 6], seed=400))
    return cases


CASES = build_cases()
CASE_IDS = [c.name for c in CASES]


# ---- long feeds: only stream_expected, the host twin and the device see these (Model walks rows in Python) -------------
def select_chunk(E):
    """L(E) of trigger_select_kernel: thread t of 1024 owns the window entries [t L, (t + 1) L) of the E = post - 1 + n_rows
    a feed has; a chunk is whole 64-byte steps."""
    return ((E + 1023) // 1024 + 63) & ~63


def chunk_edge_rows(cut, post):
    """Stream rows at the edges the selection has in each feed of `cut`: the window entries k L - 1, k L, k L + 1 for the
    chunks k = 1, 2, a middle one and the last non-empty one (feed row = entry - (post - 1)), and the feed's first and last
    row."""
    rows, at, P = set(), 0, post - 1
    for n in cut:
        if n == 0:
            continue
        E = P + n
        L = select_chunk(E)
        last = (E - 1) // L
        for k in {1, 2, last // 2, last} - {0}:
            rows |= {at + j - P for j in (k * L - 1, k * L, k * L + 1) if P <= j < E}
        rows |= {at, at + n - 1}
        at += n
    return rows


def _spread(rows, n_ch, step=1):
    """One pulse per row, the channels cycling over all of them."""
    return [(r, (i * step) % n_ch, 2 if i % 5 else -2) for i, r in enumerate(sorted(rows))]


def _edge(n_rows):
    # 1 channel, post 4: E = 3 + n_rows.  About 1 080 triggers for max_events 1024: the long feed drops.  What hits in its
    # last three rows (the last window entry is its last row: at E = 65 537 the only entry of chunk 512) can only be emitted
    # by a next feed, so eight more rows follow: their feed emits it from the trigger bit and the record the long feed left, and a hit three rows
    # behind the long feed's last row is chained to it through the last hitting row that feed left
    return Case(f"edge_{n_rows + 3}", 1, 2, 4, 3, 1024, n_rows + 8,
                _spread(set(range(7, n_rows - 3, 61)) | chunk_edge_rows([n_rows], 4) | {n_rows + 2}, 1), [[n_rows, 8]], seed=500)


def _million():
    n = 1 << 20
    cuts = [[n], [n - 4, 4], [70_000, 1, 65_535, n - 135_536]]          # E = 2^20 + 4, 2^20, 913 044: L = 1088, 1024, 896
    rows = set(range(11, n, 997))
    for cut in cuts:
        rows |= chunk_edge_rows(cut, 5)
    # a trigger that is the first entry of a chunk, and one that is the last, with nothing beside them (L = 1088, P = 4)
    rows |= {5 * 1088 - 4, 7 * 1088 - 1 - 4}
    return Case("million_4ch", 4, 3, 5, 10, 4096, n, _spread(rows, 4), cuts, seed=501)


CHAIN_BREAKS = (257 * 40, 257 * 100, 257 * 260)          # the last one behind window entry 65 536


def _chain(broken):
    # 40 channels take a wave per row: 70 001 row groups > 65 536, the 2048-workgroup cap of trigger_hits_kernel.  E = 70 005,
    # L = 128; a hit every 257 rows or closer and holdoff 300: row 0 is the only trigger.  Broken: three hits taken out, each
    # leaving a gap of 514 rows, so the hit behind each gap is a trigger whose verdict rests on a last hit four chunks back
    n = 70_001
    rows = set(range(0, n, 257)) | chunk_edge_rows([n], 5)
    if broken:
        rows -= set(CHAIN_BREAKS)
        srt = sorted(rows)
        assert sum(b - a > 300 for a, b in zip(srt, srt[1:])) == 3
    return Case("chain_40ch_broken" if broken else "chain_40ch", 40, 0, 5, 300, 16, n, _spread(rows, 40, step=7), [[n]], seed=502)


def _wide_long():
    # 65 channels: a workgroup per row, 66 000 (65 537) rows > the 65 536-workgroup cap of trigger_hits_wide_kernel
    n = 66_000
    cuts = [[65_537, 463], [n]]
    rows = set(range(5, n, 511))
    for cut in cuts:
        rows |= chunk_edge_rows(cut, 70)
    return Case("wide_65ch_long", 65, 0, 70, 100, 256, n, _spread(rows, 65, step=9), cuts, seed=503)


def _every7(holdoff):
    # E = 200 001, L = 256: 36 or 37 hits in every chunk.  Holdoff 6: every one of them a trigger; 7: row 0 alone
    n = 200_000
    cuts = [[n], [131_072, 68_928]]
    rows = set(range(3, n, 7))
    for cut in cuts:
        rows |= chunk_edge_rows(cut, 2)
    return Case(f"every7_200k_holdoff{holdoff}", 3, 0, 2, holdoff, 1 << 15, n, _spread(rows, 3), cuts, seed=504)


class LargeCase:
    """A long case, built when first asked for and kept."""

    def __init__(self, name, build):
        self.name, self._build, self._case = name, build, None

    def case(self):
        if self._case is None:
            self._case = self._build()
            assert self._case.name == self.name
        return self._case


LARGE_CASES = [LargeCase("edge_65536", lambda: _edge(65_533)), LargeCase("edge_65537", lambda: _edge(65_534)),
               LargeCase("million_4ch", _million), LargeCase("chain_40ch", lambda: _chain(False)),
               LargeCase("chain_40ch_broken", lambda: _chain(True)), LargeCase("wide_65ch_long", _wide_long),
               LargeCase("every7_200k_holdoff6", lambda: _every7(6)), LargeCase("every7_200k_holdoff7", lambda: _every7(7))]
LARGE_IDS = [c.name for c in LARGE_CASES]


# ---- stream rows beyond 2^31: a quiet buffer fed 2 049 times, then a tail with pulses -----------------------------------
PAST_N, PAST_FEEDS, PAST_TAIL = 1 << 20, 2049, 5000
PAST_PARAMS = (1, PAST_N, 3, 5, 10, 64)                 # n_ch, max_rows, pre, post, holdoff, max_events
PAST_PULSES = (0, 2, 3, 700, 4990, 4999)                # 2 and 3 chain onto 0; 4999 has no post rows yet


def past_2g_stream():
    """(quiet [2^20][1], tail [5000][1], levels): nothing hits in `quiet`, so behind any number of quiet feeds only the row
    numbers and the carried rows depend on the prefix, and the carried rows are the same quiet rows."""
    lv = default_levels(1)
    rng = np.random.default_rng(600)
    bg = (0.1 * (rng.standard_normal((PAST_N + PAST_TAIL, 1)) + 1j * rng.standard_normal((PAST_N + PAST_TAIL, 1)))).astype(np.complex64)
    assert np.abs(quantity(bg, lv)).max() < 0.9
    quiet, tail = bg[:PAST_N].copy(), bg[PAST_N:].copy()
    for r in PAST_PULSES:
        tail[r, 0] += np.float32(2)
    return quiet, tail, lv
