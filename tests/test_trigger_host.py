"""The trigger's host twin (gsdr_trigger_* over GSDR_TRIGGER_HOST, trigger_host.cpp) against the literal model of
tests/_trigger.py, bit for bit; the refusals, the struct layouts and the Python mirror.  The vectorised model is pinned to
the literal one on every small case, and the host twin to the vectorised one on the long feeds and past row 2^31.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from _trigger import (CASE_IDS, CASES, EVENT_DTYPE, LARGE_CASES, LARGE_IDS, LEVEL_DTYPE, PAST_FEEDS, PAST_N, PAST_PARAMS, PAST_TAIL,
                      Model, default_levels, lane_width, past_2g_stream, same_bits, select_chunk)


@pytest.fixture(scope="module")
def trig(gsdr_lib):
    import gpu_sdr_amd.trigger as t
    return t


def run_host(trig, case, cut, max_events=None):
    h = trig.host_trigger(case.n_ch, case.max_rows, case.pre, case.post, case.holdoff, max_events or case.max_events, case.levels)
    out = [h.feed(x) for x in case.feeds(cut)]
    assert h.rows_seen == case.rows.shape[0]
    h.close()
    return out


def assert_feeds_equal(got, want, what):
    assert len(got) == len(want)
    for k, ((ge, gs, gd), (we, ws, wd)) in enumerate(zip(got, want)):
        assert gd == wd, (what, k, gd, wd)
        assert same_bits(ge, we), (what, k, ge, we)
        assert same_bits(gs, ws), (what, k)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_twin_matches_the_model(trig, case):
    emitted = 0
    for cut in case.cuts:
        want = case.expected(cut)
        assert_feeds_equal(run_host(trig, case, cut), want, (case.name, cut))
        emitted += sum(len(e) for e, _, _ in want)
    assert emitted > 0, "a case that emits nothing checks nothing"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_vectorised_model_equals_the_literal_model(case):
    """stream_expected, the only model the long cases have, against Model on every case and cut, bit for bit."""
    for cut in case.cuts:
        assert_feeds_equal(case.expected_vec(cut), case.expected(cut), (case.name, cut))


def test_select_chunk_is_what_the_kernel_computes():
    assert [select_chunk(E) for E in (1, 65_536, 65_537, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 4)] == \
        [64, 64, 128, 1024, 1024, 1088, 1088]
    for E in (150, 65_536, 65_537, 200_001, 913_044, (1 << 20) + 4):
        L = select_chunk(E)
        assert L % 64 == 0 and 1024 * L >= E and (L == 64 or 1024 * (L - 64) < E)


LARGE_EVENTS = {"edge_65536": None, "edge_65537": None, "million_4ch": None, "chain_40ch": 1, "chain_40ch_broken": 4,
                "wide_65ch_long": None, "every7_200k_holdoff6": None, "every7_200k_holdoff7": 1}


@pytest.mark.parametrize("large", LARGE_CASES, ids=LARGE_IDS)
def test_host_twin_matches_the_vectorised_model_on_long_feeds(trig, large):
    case = large.case()
    for cut in case.cuts:
        want = case.expected_vec(cut)
        assert_feeds_equal(run_host(trig, case, cut), want, (case.name, cut))
        n = sum(len(e) for e, _, _ in want)
        assert n > 0, "a cut that emits nothing checks nothing"
        if LARGE_EVENTS[case.name] is not None:
            assert n == LARGE_EVENTS[case.name], (case.name, cut, n)
    dropped = sum(d for _, _, d in case.expected_vec(case.cuts[0]))
    if case.name.startswith("edge_"):
        assert dropped > 0 and case.max_events == 1024          # the cut at max_events, behind all 1024 (513) chunks
    else:
        assert dropped == 0
    if case.name == "every7_200k_holdoff6":
        assert n > 28_000


def test_long_cases_reach_what_they_are_for():
    """The chunk lengths and grid caps each long case names, restated from launch_trigger_feed."""
    seen = {}
    for large in LARGE_CASES:
        case = large.case()
        for cut in case.cuts:
            for n in cut:
                E = case.post - 1 + n
                seen.setdefault(case.name, set()).add(select_chunk(E))
                if case.n_ch <= 64:
                    rpw = 64 >> lane_width(case.n_ch)
                    if -(-n // rpw) > 65_536:
                        seen[case.name].add("hits cap")
                elif n > 65_536:
                    seen[case.name].add("wide cap")
    assert seen["edge_65536"] == {64} and seen["edge_65537"] == {128, 64}      # 64: the eight rows behind the long feed
    assert {1088, 1024, 896} <= seen["million_4ch"]
    assert seen["chain_40ch"] == seen["chain_40ch_broken"] == {128, "hits cap"}
    assert {128, "wide cap"} <= seen["wide_65ch_long"]
    assert 256 in seen["every7_200k_holdoff6"] and 256 in seen["every7_200k_holdoff7"]
    caps = next(c for c in CASES if c.name == "caps_2048_overflow")
    S = caps.pre + caps.post
    assert (S - 1) * caps.n_ch > 1 << 19 and caps.max_events * S * caps.n_ch > 1 << 21
    assert any(0 < n < S - 1 for cut in caps.cuts for n in cut)
    drops = [sum(d for _, _, d in caps.expected(cut)) for cut in caps.cuts]
    assert any(d > 0 for d in drops) and any(d == 0 for d in drops)


def test_rows_past_2_to_the_31_on_the_host_twin(trig):
    """2 049 quiet feeds of 2^20 rows, then a tail with pulses: the events are those of a twin that saw ONE quiet feed, 2048 *
    2^20 rows later, with the same snippets -- every row number along the way is 64 bits wide."""
    quiet, tail, lv = past_2g_stream()
    full, short = trig.host_trigger(*PAST_PARAMS, lv), trig.host_trigger(*PAST_PARAMS, lv)
    for _ in range(PAST_FEEDS):
        ev, _, dropped = full.feed(quiet)
        assert len(ev) == 0 and dropped == 0
    ev, _, _ = short.feed(quiet)
    assert len(ev) == 0
    (ge, gs, gd), (we, ws, wd) = full.feed(tail), short.feed(tail)
    assert full.rows_seen == PAST_FEEDS * PAST_N + PAST_TAIL == (1 << 31) + (1 << 20) + 5000
    assert list(ge["row"]) == [(1 << 31) + (1 << 20) + r for r in (0, 700, 4990)]
    we = we.copy()
    we["row"] += (PAST_FEEDS - 1) * PAST_N
    assert same_bits(ge, we) and same_bits(gs, ws) and gd == wd == 0
    assert same_bits(gs[0], np.concatenate([quiet[-3:], tail[:5]]))
    full.reset()
    ev, sn, _ = full.feed(tail)
    assert list(ev["row"]) == [700, 4990] and same_bits(sn[0], tail[697:705])      # row 0 < pre: a trigger, not emitted
    full.close(), short.close()


def test_planted_case_is_what_the_issue_states(trig):
    case = CASES[0]
    assert case.name == "planted"
    for cut in case.cuts:
        out = run_host(trig, case, cut)
        ev = np.concatenate([e for e, _, _ in out])
        assert list(ev["row"]) == [9, 15, 31, 47], cut
        assert list(ev["channel"]) == [2, 3, 0, 1] and list(ev["side"]) == [1, 1, 1, -1] and list(ev["n_hit"]) == [1, 1, 1, 2]
        assert sum(d for _, _, d in out) == 0
    first, second = run_host(trig, case, [32, 32])
    assert list(first[0]["row"]) == [9, 15] and list(second[0]["row"]) == [31, 47]      # 31 is deferred
    # the snippet is rows [r - pre, r + post) of the input
    sn = np.concatenate([s for _, s, _ in run_host(trig, case, [64])])
    for k, r in enumerate([9, 15, 31, 47]):
        assert same_bits(sn[k], case.rows[r - 2:r + 4])


def test_cut_invariance(trig):
    for case in CASES:
        if case.name.endswith("overflow"):
            continue
        outs = []
        for cut in case.cuts:
            out = run_host(trig, case, cut)
            assert sum(d for _, _, d in out) == 0
            outs.append((np.concatenate([e for e, _, _ in out]), np.concatenate([s for _, s, _ in out])))
        for ev, sn in outs[1:]:
            assert same_bits(ev, outs[0][0]) and same_bits(sn, outs[0][1]), case.name


def test_capacity_rule(trig):
    case = next(c for c in CASES if c.name == "planted_overflow")
    (ev, sn, dropped), = run_host(trig, case, [64])
    assert list(ev["row"]) == [9, 15] and dropped == 2 and sn.shape == (2, 6, 5)
    # the cut-dependent rule: two feeds of 32 rows have room for all four
    out = run_host(trig, case, [32, 32])
    assert [list(e["row"]) for e, _, _ in out] == [[9, 15], [31, 47]] and all(d == 0 for _, _, d in out)


def test_set_levels_between_feeds_keeps_earlier_records(trig):
    """Rows 0..31 are fed with thresholds of +-1, then the thresholds drop to +-1e-6, where every sample hits: row 31's
    record (a hit, its event deferred to the second feed) and those of the quiet rows before it stay as they were made."""
    case = CASES[0]
    wide = default_levels(5, off=(4,))
    tight = default_levels(5, off=(4,))
    tight["lo"][:4], tight["hi"][:4] = -1e-6, 1e-6            # every sample of the background hits
    h = trig.host_trigger(5, 32, 2, 4, 3, 8, wide)
    m = Model(5, 2, 4, 3, 8, wide)
    a, b = h.feed(case.rows[:32]), m.feed(case.rows[:32])
    assert_feeds_equal([a], [b], "first")
    h.set_levels(tight)
    m.set_levels(tight)
    a, b = h.feed(case.rows[32:]), m.feed(case.rows[32:])
    assert_feeds_equal([a], [b], "second")
    # row 31 was quiet-before under the OLD levels, so it is a trigger; re-evaluating rows 28..30 with the new levels
    # would have chained it to them.  Row 32 hits under both and is chained to 31; nothing else can trigger behind it.
    assert list(a[0]["row"]) == [31]
    h.close()


def test_reset(trig):
    case = CASES[0]
    h = trig.host_trigger(5, 64, 2, 4, 3, 8, case.levels)
    h.feed(case.rows[:40])
    assert h.rows_seen == 40
    h.reset()
    assert h.rows_seen == 0
    ev, sn, dropped = h.feed(case.rows)
    want = case.expected([64])[0]
    assert same_bits(ev, want[0]) and same_bits(sn, want[1]) and dropped == 0
    h.close()


def test_struct_sizes(gsdr_lib):
    from gpu_sdr_amd import _lib
    assert C.sizeof(_lib.TriggerLevelC) == 24 and C.sizeof(_lib.TriggerEventC) == 24
    assert EVENT_DTYPE.itemsize == 24 and LEVEL_DTYPE.itemsize == 24
    import gpu_sdr_amd.trigger as t
    assert t.EVENT_DTYPE == EVENT_DTYPE and t.LEVEL_DTYPE == LEVEL_DTYPE
    assert [n for n, _ in _lib.TriggerEventC._fields_] == list(EVENT_DTYPE.names)
    assert [getattr(_lib.TriggerEventC, n).offset for n in EVENT_DTYPE.names] == [EVENT_DTYPE.fields[n][1] for n in EVENT_DTYPE.names]


REFUSALS = [
    (dict(n_ch=0), "n_ch"), (dict(n_ch=(1 << 20) + 1), "n_ch"), (dict(max_rows=0), "max_rows"),
    (dict(max_rows=(1 << 20) + 1), "max_rows"), (dict(pre=-1), "pre"), (dict(post=0), "post"),
    (dict(pre=65535, post=2), "pre + post"), (dict(holdoff=-1), "holdoff"), (dict(holdoff=(1 << 30) + 1), "holdoff"),
    (dict(max_events=0), "max_events"), (dict(max_events=(1 << 20) + 1), "max_events"), (dict(levels=None), "levels"),
    (dict(device_index=-3), "device_index"),
]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(REFUSALS)])
@pytest.mark.parametrize("device_index", [-2, 0])
def test_create_refusals_touch_no_device(gsdr_lib, change, word, device_index):
    """Refused before the device is touched: the same refusal for a device object, on a machine without a GPU."""
    lv = default_levels(4)
    args = dict(n_ch=4, max_rows=16, pre=1, post=2, holdoff=0, max_events=4, levels=lv.ctypes.data, device_index=device_index)
    args.update(change)
    h = gsdr_lib.gsdr_trigger_create(*[args[k] for k in ("n_ch", "max_rows", "pre", "post", "holdoff", "max_events", "levels", "device_index")])
    assert not h
    msg = gsdr_lib.gsdr_last_error(None).decode()
    assert msg.startswith("gsdr_trigger_create: ") and word in msg, msg


def test_feed_refusals(gsdr_lib, trig):
    lv = default_levels(4)
    h = trig.host_trigger(4, 16, 1, 2, 0, 4, lv)
    rows = np.zeros((17, 4), dtype=np.complex64)
    ev = np.zeros(4, dtype=EVENT_DTYPE)
    sn = np.zeros((4, 3, 4), dtype=np.complex64)
    h.feed(rows[:5])
    for n in (17, -1):
        assert gsdr_lib.gsdr_trigger_feed_host(h._h, rows.ctypes.data, n, ev.ctypes.data, sn.ctypes.data, None) == -1
        assert gsdr_lib.gsdr_last_error(None).decode().startswith("gsdr_trigger_feed_host: n_rows")
        assert h.rows_seen == 5                                   # state unchanged
    # n_rows == 0 touches no row pointer
    assert gsdr_lib.gsdr_trigger_feed_host(h._h, None, 0, None, None, None) == 0 and h.rows_seen == 5
    # the device feeds are refused on a host object, with a message
    cnt = (C.c_int * 2)()
    assert gsdr_lib.gsdr_trigger_feed_device(h._h, rows.ctypes.data, 1, ev.ctypes.data, sn.ctypes.data, cnt, None) == -1
    assert "host object" in gsdr_lib.gsdr_last_error(None).decode()
    assert gsdr_lib.gsdr_trigger_feed(h._h, rows.ctypes.data, 1, ev.ctypes.data, sn.ctypes.data, None, None) == -1
    assert gsdr_lib.gsdr_last_error(None).decode().startswith("gsdr_trigger_feed: ")
    assert h.rows_seen == 5
    h.close()
    with pytest.raises(trig.GsdrError, match="gsdr_trigger_create: post"):
        trig.host_trigger(4, 16, 1, 0, 0, 4, lv)


def test_levels_from_rows(trig):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((501, 6)) + 1j * rng.standard_normal((501, 6))).astype(np.complex64)
    lv = trig.levels_from_rows(x, 5.0, direction=(0.6, 0.8), channels=[0, 2, 5])
    assert lv.dtype == LEVEL_DTYPE and lv.shape == (6,)
    for c in range(6):
        proj = x[:, c].real.astype(np.float32) * np.float32(0.6) + x[:, c].imag.astype(np.float32) * np.float32(0.8)
        proj = proj.astype(np.float64)
        med, std = np.sort(proj)[250], np.sqrt(np.mean((proj - proj.mean()) ** 2))
        assert lv["bx"][c] == 0 and lv["by"][c] == 0 and lv["dx"][c] == np.float32(0.6) and lv["dy"][c] == np.float32(0.8)
        if c in (0, 2, 5):
            assert abs(lv["lo"][c] - (med - 5 * std)) < 1e-6 and abs(lv["hi"][c] - (med + 5 * std)) < 1e-6   # one float32 rounding of a value below 8
        else:
            assert lv["lo"][c] == -np.inf and lv["hi"][c] == np.inf
    # a quiet stretch gives levels that a 5 sigma trigger does not fire on
    h = trig.host_trigger(6, 501, 0, 1, 0, 4, trig.levels_from_rows(x, 6.0))
    ev, _, _ = h.feed(x)
    assert len(ev) == 0
    h.close()


def test_reference_shaped_trigger_surface(trig):
    """trigger(data, metadata) as pyUSRP's client calls it: flat packets in ch0_t0, ch1_t0, ... order in, the flat
    snippets and metadata['length'] out."""
    case = CASES[0]
    h = trig.host_trigger(5, 16, 2, 4, 3, 8, case.levels)          # packets of 32 rows: fed in pieces of max_rows
    assert h.trigger_control == "AUTO"
    want = case.expected([32, 32])
    for k in range(2):
        data, meta = h.trigger(case.rows[32 * k:32 * k + 32].reshape(-1), {"channels": 5, "length": 160, "packet_number": k})
        assert meta["packet_number"] == k and meta["length"] == len(data) == want[k][1].size
        assert same_bits(data, want[k][1].reshape(-1))
    data, meta = h.trigger(np.zeros(0, dtype=np.complex64), {"channels": 5, "length": 0})
    assert meta["length"] == 0 and len(data) == 0
    h.close()


def test_case_list_holds_every_class_the_suite_relies_on():
    seen = set()
    for case in CASES:
        K = case.pre + case.post - 1
        hit_rows = sorted({r for (r, c, a) in case.pulses if np.isfinite(case.levels["hi"][c])})
        if any(not np.isfinite(case.levels["hi"][c]) for (_, c, _) in case.pulses):
            seen.add("switched-off channel")
        if hit_rows and hit_rows[0] < case.pre:
            seen.add("trigger before pre")
        for cut in case.cuts:
            bounds = np.cumsum([0] + cut)
            want = case.expected(cut)
            if any(d > 0 for _, _, d in want):
                seen.add("overflowing feed")
            if any(0 < n < K for n in cut):
                seen.add("feed shorter than the carry")
            for k, (ev, _, _) in enumerate(want):
                if any(r < bounds[k] for r in ev["row"]):
                    seen.add("deferred event")
                if any(n > 1 for n in ev["n_hit"]):
                    seen.add("row with n_hit > 1")
            for a, b in zip(hit_rows, hit_rows[1:]):
                if 0 < b - a <= case.holdoff and any(a < e <= b for e in bounds[1:-1]):
                    seen.add("hit chained across a feed boundary")
    assert seen == {"deferred event", "trigger before pre", "hit chained across a feed boundary", "switched-off channel",
                    "row with n_hit > 1", "overflowing feed", "feed shorter than the carry"}, seen
    # every lane width of trigger_hits_kernel, and both sides of each power of two up to the wide kernel's first channel
    n_chs = {case.n_ch for case in CASES}
    assert {lane_width(n) for n in n_chs if n <= 64} == set(range(7))
    assert all((1 << k) in n_chs and (1 << k) + 1 in n_chs for k in range(7)), sorted(n_chs)
    # the wide kernel: one step exactly, one channel into the second and the third, and more than two steps
    assert {256, 257, 513} <= n_chs
    # a row with two hits whose lowest channel is 0 and whose other one is the last channel, as an event of its own
    for case in CASES:
        if case.name.startswith("lanes_") and case.name.endswith("_h0"):
            ev = np.concatenate([e for e, _, _ in case.expected(case.cuts[0])])
            both = ev[ev["n_hit"] == 2]
            assert len(both) == 1 and both["channel"][0] == 0 and both["side"][0] == -1, case.name
            assert case.n_ch - 1 in ev["channel"] and {1, -1} <= set(ev["side"]), case.name
