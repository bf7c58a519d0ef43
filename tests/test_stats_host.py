"""The row statistics without a GPU (include/gsdr.h, "row statistics on the device"): the library's host twin
(GSDR_STATS_HOST) against the numpy bit model of tests/_stats.py, bit for bit, the wide-range column included; every
cutting of the stream; the edge laws of the bins, the chains and the quantiles; the results against numpy on the
Gaussian stream with the bounds the arithmetic gives; the levels against levels_from_rows; every refusal.

Bounds.  mean: any order of n double additions of terms |d| <= D is within n 2^-52 D of the exact sum, the division
and the pivot add two roundings.  Variance: 1e-9 relative with the pivot within 10 sigma of the mean
(n 2^-52 (1 + 100) at n <= 2^17).  Quantile: within one bin width w of sorted(q)[t - 1], by construction."""
import ctypes as C

import numpy as np
import pytest

from _stats import LEVEL_DTYPE, Model, cuttings, feed_cut, project, same_doubles, same_summary, stream


@pytest.fixture(scope="module")
def stats(gsdr_lib):
    from gpu_sdr_amd import stats
    return stats


_memo = {}


def case(n, n_ch, seed, wide=()):
    key = (n, n_ch, seed, tuple(wide))
    if key not in _memo:
        _memo[key] = stream(n, n_ch, seed=seed, wide=wide)
    return _memo[key]


PR = [0.01, 0.25, 0.5, 0.999, 1.0]
PR16 = [k / 16 for k in range(1, 17)]


def run_twin(stats, rows, axes, n_bins, lanes, cut, max_rows):
    h = stats.host_stats(rows.shape[1], max_rows, n_bins, axes, lanes=lanes)
    feed_cut(h, rows, cut)
    assert h.rows_seen == rows.shape[0]
    out = (h.read(), h.counts(), h.quantiles(PR), h.levels(5.0, "median"), h.levels(3.0, "mean"), h.lanes)
    h.close()
    return out


@pytest.mark.parametrize("n,n_ch,n_bins,lanes", [(1, 1, 1, 1), (257, 3, 7, 4), (5000, 5, 256, 64), (5000, 5, 256, 16), (5000, 5, 256, 1),
                                                  (700, 6, 33, 1024), (10, 1, 4, 32768)])
def test_twin_equals_the_model_bit_for_bit(stats, n, n_ch, n_bins, lanes):
    rows, axes = case(n, n_ch, 5, wide=(n_ch - 1,))
    summary, counts, quant, lv_med, lv_mean, got_lanes = run_twin(stats, rows, axes, n_bins, lanes, [n], n)
    m = Model(rows, axes, n_bins, lanes)
    assert got_lanes == lanes
    assert np.array_equal(counts, m.counts)
    assert same_summary(summary, m.summary()) == ""
    assert same_doubles(quant, m.quantiles(PR))
    assert lv_med.tobytes() == m.levels(5.0, "median").tobytes()
    assert lv_mean.tobytes() == m.levels(3.0, "mean").tobytes()


def test_the_wide_column_sees_the_order_of_the_additions(stats):
    """What makes the bit tests mean something: on the wide column lanes 64, 16 and 1 give different means; on the
    Gaussian columns they need not."""
    rows, axes = case(5000, 5, 5, wide=(4,))
    means = [Model(rows, axes, 256, lanes).summary()["mean"][4] for lanes in (64, 16, 1)]
    assert len({float(v).hex() for v in means}) == 3


@pytest.mark.parametrize("n,n_ch,n_bins,lanes,max_rows", [(257, 3, 7, 4, 257), (500, 5, 64, 64, 100), (5000, 2, 256, 16, 1200)])
def test_every_cutting_gives_the_same_bits(stats, n, n_ch, n_bins, lanes, max_rows):
    rows, axes = case(n, n_ch, 9, wide=(0,))
    want = None
    for name, cut in cuttings(n, max_rows).items():
        got = run_twin(stats, rows, axes, n_bins, lanes, cut, max_rows)
        blob = tuple(np.asarray(g).tobytes() for g in got[:5])
        want = want or blob
        assert blob == want, name
    m = Model(rows, axes, n_bins, lanes)
    assert same_summary(got[0], m.summary()) == ""


def test_edge_laws_of_the_bins_and_the_chains(stats):
    """q == lo -> bin 0; q == hi -> over; the largest float below hi where the model says; -0.0 and denormals; 1e38 dx
    overflowing -> bad; NaN and Inf -> bad and nothing else."""
    lo, hi = np.float32(-1.0), np.float32(3.0)
    axes = np.zeros(2, dtype=LEVEL_DTYPE)
    axes[0] = (0, 0, 1, 0, lo, hi)
    axes[1] = (0, 0, 1e3, 0, lo, hi)
    below_hi, below_lo = np.nextafter(hi, np.float32(-np.inf)), np.nextafter(lo, np.float32(-np.inf))
    vals = np.array([lo, hi, below_hi, below_lo, -0.0, 0.0, 1e-45, -1e-40, 1e38, np.nan, np.inf, -np.inf, 2.9999, 0.5], dtype=np.float32)
    rows = np.zeros((len(vals), 2), dtype=np.complex64)
    rows[:, 0] = vals
    rows[:, 1] = vals                                      # channel 1: q = 1e3 x, 1e38 overflows to +Inf -> bad
    for n_bins in (1, 4, 7, 4096):
        h = stats.host_stats(2, 64, n_bins, axes, lanes=2)
        h.feed(rows)
        counts, summary = h.counts(), h.read()
        h.close()
        m = Model(rows, axes, n_bins, 2)
        assert np.array_equal(counts, m.counts) and same_summary(summary, m.summary()) == ""
        c0 = counts[0]
        assert c0[0] == 1 and c0[n_bins + 1] == 2 and c0[n_bins + 2] == 3          # below_lo | hi, 1e38 | nan, +-inf
        assert c0[n_bins] >= 1                                                       # below_hi lies in the last bin
        assert c0[1] >= 1 and (n_bins == 1 or c0[1] == 1)                            # lo itself opens bin 0
        assert counts[1][n_bins + 2] == 4                                            # 1e38 x 1e3 overflowed
        assert summary["min"][0] == below_lo and summary["max"][0] == np.float32(1e38)
        assert summary["n"][0] == len(vals) - 3 and summary["bad"][0] == 3
    # -0.0 against +0.0: the earlier one stays (q = -0 needs both terms -0: x = y = -0 with dy = +0)
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        h = stats.host_stats(1, 4, 4, axes[:1], lanes=1)
        h.feed(np.array([first, first, second, second], dtype=np.float32).view(np.complex64).reshape(2, 1))
        s = h.read()
        h.close()
        assert np.signbit(s["min"][0]) == np.signbit(np.float32(first)) and np.signbit(s["max"][0]) == np.signbit(np.float32(first))


def test_n_0_n_1_and_ranks_outside_the_range(stats):
    axes = np.zeros(1, dtype=LEVEL_DTYPE)
    axes[0] = (0, 0, 1, 0, 0.0, 1.0)
    h = stats.host_stats(1, 16, 8, axes, lanes=4)
    s = h.read()
    assert s["n"][0] == 0 and np.isnan(s["mean"][0]) and np.isnan(s["var"][0]) and s["min"][0] == np.inf and s["max"][0] == -np.inf
    assert np.isnan(h.quantiles([0.5])[0, 0])
    lv = h.levels(3.0)
    assert lv["lo"][0] == -np.inf and lv["hi"][0] == np.inf and lv["dx"][0] == 1
    h.feed(np.array([[0.30]], dtype=np.complex64))
    s = h.read()
    assert s["n"][0] == 1 and s["mean"][0] == 0.5 + (np.float64(np.float32(0.30)) - 0.5) and np.isnan(s["var"][0])
    assert s["min"][0] == s["max"][0] == np.float32(0.30)
    assert h.levels(3.0)["lo"][0] == -np.inf                                         # n < 2: switched off
    q = h.quantiles([0.5, 1.0])[0]
    assert q[0] == q[1] == 0.0 + (2.0 + (1.0 - 0.5) / 1.0) * 0.125                    # bin 2, the middle of it
    h.reset()
    assert h.rows_seen == 0 and h.read()["n"][0] == 0 and not h.counts().any()
    # three below, one inside, four above: ranks 1-3 -> -inf, 4 -> the bin, 5-8 -> +inf
    h.feed(np.array([[-1], [-2], [-3], [0.55], [2], [3], [4], [1.0]], dtype=np.complex64))
    q = h.quantiles([1 / 8, 3 / 8, 4 / 8, 5 / 8, 1.0])[0]
    assert list(q[:2]) == [-np.inf, -np.inf] and 0.5 <= q[2] < 0.625 and list(q[3:]) == [np.inf, np.inf]
    s = h.read()
    assert (s["under"][0], s["over"][0], s["n"][0]) == (3, 4, 8)
    h.close()


def test_against_numpy_on_the_gaussian_stream(stats):
    n, n_ch, n_bins = 5000, 5, 256
    rows, axes = case(n, n_ch, 21)
    for lanes in (1, 64):
        summary, counts, quant, _, _, _ = run_twin(stats, rows, axes, n_bins, lanes, [n], n)
        q = project(rows, axes).astype(np.float64)
        p = 0.5 * (axes["lo"].astype(np.float64) + axes["hi"].astype(np.float64))
        w = (axes["hi"].astype(np.float64) - axes["lo"].astype(np.float64)) / n_bins
        assert not counts[:, 0].any() and not counts[:, -2].any() and not counts[:, -1].any()
        bound = n * 2.0 ** -52 * np.abs(q - p).max(axis=0)
        assert np.all(np.abs(summary["mean"] - q.mean(axis=0)) <= bound)
        var = q.var(axis=0, ddof=1)
        assert np.all(np.abs(q.mean(axis=0) - p) <= 10 * np.sqrt(var))
        assert np.all(np.abs(summary["var"] - var) <= 1e-9 * var)
        assert np.array_equal(summary["min"], q.min(axis=0).astype(np.float32)) and np.array_equal(summary["max"], q.max(axis=0).astype(np.float32))
        srt = np.sort(q, axis=0)
        for i, pr in enumerate(PR):
            t = max(1, int(np.ceil(pr * n)))
            assert np.all(np.abs(quant[:, i] - srt[t - 1]) < w), pr


def test_levels_against_levels_from_rows(stats):
    """The same rows through the numpy recipe of trigger.py (projection from 0: bx = by = 0): the centre within one bin,
    the half-width within nsigma sigma / n (n - 1 against n) + 1e-6 sigma."""
    from gpu_sdr_amd.trigger import levels_from_rows
    n, n_ch, n_bins, nsigma = 4000, 4, 512, 5.0
    rows, axes = case(n, n_ch, 33)
    axes = axes.copy()
    axes["bx"], axes["by"] = 0, 0
    q = project(rows, axes).astype(np.float64)
    axes["lo"], axes["hi"] = (q.mean(axis=0) - 8 * q.std(axis=0)).astype(np.float32), (q.mean(axis=0) + 8 * q.std(axis=0)).astype(np.float32)
    direction = np.stack([axes["dx"], axes["dy"]], axis=1)
    ref = levels_from_rows(rows, nsigma, direction=direction, channels=[0, 1, 3])
    h = stats.host_stats(n_ch, n, n_bins, axes)
    h.feed(rows)
    lv = h.levels(nsigma, "median", on=[1, 1, 0, 1])
    h.close()
    w = (axes["hi"].astype(np.float64) - axes["lo"].astype(np.float64)) / n_bins
    sigma = q.std(axis=0)
    for f in ("bx", "by", "dx", "dy"):
        assert np.array_equal(lv[f], ref[f])
    assert lv["lo"][2] == ref["lo"][2] == -np.inf and lv["hi"][2] == ref["hi"][2] == np.inf
    for c in (0, 1, 3):
        mid, half = 0.5 * (float(lv["lo"][c]) + float(lv["hi"][c])), 0.5 * (float(lv["hi"][c]) - float(lv["lo"][c]))
        rmid, rhalf = 0.5 * (float(ref["lo"][c]) + float(ref["hi"][c])), 0.5 * (float(ref["hi"][c]) - float(ref["lo"][c]))
        assert abs(mid - rmid) < w[c] + 1e-6 * sigma[c]
        assert abs(half - rhalf) <= nsigma * sigma[c] / n + 1e-6 * sigma[c]


def test_reset_with_new_axes_is_the_two_pass_use(stats):
    from gpu_sdr_amd.stats import axes_around
    n, n_ch = 3000, 3
    rows, axes = case(n, n_ch, 41)
    coarse = axes.copy()
    coarse["lo"], coarse["hi"] = -100, 100
    h = stats.host_stats(n_ch, n, 64, coarse, lanes=8)
    h.feed(rows)
    fine = axes_around(h.levels(8.0, "mean"))
    h.reset(fine)
    assert h.rows_seen == 0 and np.array_equal(h.axes, fine)
    h.feed(rows)
    got = h.read(), h.counts(), h.quantiles(PR)
    h.close()
    m = Model(rows, fine, 64, 8)
    assert same_summary(got[0], m.summary()) == "" and np.array_equal(got[1], m.counts) and same_doubles(got[2], m.quantiles(PR))


def test_the_lanes_rule(stats):
    axes = np.zeros(1, dtype=LEVEL_DTYPE)
    axes["hi"] = 1
    for n_ch, max_rows, want in ((2048, 1000, 32), (256, 10000, 256), (4, 1 << 20, 16384), (1, 1 << 20, 32768), (1, 1, 1), (1, 100, 64),
                                 (1 << 20, 1000, 1), (3, 1 << 20, 32768)):
        h = stats.host_stats(n_ch, max_rows, 1, np.tile(axes, n_ch))
        assert h.lanes == want, (n_ch, max_rows)
        h.close()


def test_the_feed_plan_at_its_edges(stats, gsdr_lib):
    """gsdr_stats_plan (stats_plan_of in csrc/stats_state.h, the function the feed's launcher asks): the tile is the
    largest power of two that is at most n_ch, at most 32, and whose table tile (n_bins + 3) 4 fits into 65 536 bytes --
    pinned on both sides of the four n_bins at which the table of a tile is EXACTLY 65 536 bytes, and over every n_bins."""
    plan = stats.feed_plan
    for n_bins, tile in ((509, 32), (1021, 16), (2045, 8), (4093, 4)):
        for n_ch in (tile, tile + 1, 2 * tile - 1, 2 * tile, 100, 1 << 20):
            a, b = plan(n_ch, n_bins, 8), plan(n_ch, n_bins + 1, 8)
            assert (a["tile"], a["lds_bytes"]) == (tile, 65536), (n_ch, n_bins)
            assert (b["tile"], b["lds_bytes"]) == (tile // 2, (tile // 2) * (n_bins + 4) * 4), (n_ch, n_bins)
            assert plan(tile - 1, n_bins, 8)["tile"] == tile // 2                    # fewer channels than the table has room for
    channels = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 2048, (1 << 20) - 1, 1 << 20)
    out = (C.c_int * 4)()
    for n_bins in range(1, 4097):
        per = (n_bins + 3) * 4
        for n_ch in channels:
            assert gsdr_lib.gsdr_stats_plan(n_ch, n_bins, 64, out) == 0
            tile, tiles, splits, lds = out
            assert tile in (1, 2, 4, 8, 16, 32) and tile <= n_ch and lds == tile * per <= 65536, (n_ch, n_bins)
            assert tile == 32 or 2 * tile > n_ch or 2 * tile * per > 65536, (n_ch, n_bins)      # and no smaller than it has to be
            assert tiles == -(-n_ch // tile) and splits == -(-64 // (256 // tile)), (n_ch, n_bins)
    # the grid's y over every lanes creation accepts
    for n_bins in (1, 256, 509, 510, 1021, 1022, 2045, 2046, 4093, 4094, 4096):
        for n_ch in channels:
            for lanes in (1 << e for e in range(16)):
                p = plan(n_ch, n_bins, lanes)
                assert p["splits"] == -(-lanes // (256 // p["tile"])) and 1 <= p["splits"] <= 65535, (n_ch, n_bins, lanes)
    assert plan(1 << 20, 1, 32768) == dict(tile=32, tiles=32768, splits=4096, lds_bytes=512)
    assert plan(1, 4096, 1) == dict(tile=1, tiles=1, splits=1, lds_bytes=16396)
    # it refuses what creation refuses (a lanes of 0 is the rule, which needs max_rows: the object reports its lanes)
    for args in ((0, 8, 1), ((1 << 20) + 1, 8, 1), (2, 0, 1), (2, 4097, 1), (2, 8, 0), (2, 8, -1), (2, 8, 3), (2, 8, 65536)):
        assert gsdr_lib.gsdr_stats_plan(*args, out) == -1, args
        with pytest.raises(ValueError):
            plan(*args)
    assert gsdr_lib.gsdr_stats_plan(2, 8, 1, None) == -1


def test_the_model_behind_a_prefix_of_pivot_rows_is_the_twin(stats):
    """tests/_stats.py, after_a_prefix_of_pivot_rows -- the expected result of the GPU test that feeds more than 2^32
    rows -- against the twin at a T0 the twin can take: 41 feeds of 997 rows of 0 + 0j, then 3 001 wide rows in pieces
    that begin at stream positions which are no multiple of lanes."""
    from _stats import PIVOT_AXIS, after_a_prefix_of_pivot_rows
    n_ch, n_bins, lanes, per, K = 2, 256, 64, 997, 41
    tail, axes = case(3001, n_ch, 17, wide=(0, 1))
    assert np.array_equal(axes, np.array([PIVOT_AXIS] * n_ch, dtype=LEVEL_DTYPE))
    T0 = K * per
    assert T0 % lanes == 45
    h = stats.host_stats(n_ch, per, n_bins, axes, lanes=lanes)
    zeros = np.zeros((per, n_ch), dtype=np.complex64)
    for _ in range(K):
        h.feed(zeros)
    feed_cut(h, tail, [7, 401, 997, 997, 599])
    assert h.rows_seen == T0 + 3001
    got = h.read(), h.counts(), h.quantiles(PR16), h.levels(5.0, "median"), h.levels(3.0, "mean")
    h.close()
    m = after_a_prefix_of_pivot_rows(T0, tail, axes, n_bins, lanes)
    assert (got[1][np.arange(n_ch), m.pivot_slot] >= T0).all() and np.array_equal(got[1], m.counts)
    assert same_summary(got[0], m.summary()) == "" and same_doubles(got[2], m.quantiles(PR16))
    assert got[3].tobytes() == m.levels(5.0, "median").tobytes() and got[4].tobytes() == m.levels(3.0, "mean").tobytes()
    # What this cannot see, by design: the tree joins chains j and j + h, so moving EVERY row by the same number of chains
    # gives the same sums (the tail alone, in one piece, has the twin's S and Q).  Only the phase of one feed against
    # another shows -- hence the pieces above, and a tail piece moved by one chain against the others has other sums.
    whole = Model(tail, axes, n_bins, lanes)
    assert np.array_equal(whole.S, m.S) and np.array_equal(whole.Q, m.Q)
    moved = Model(np.concatenate([np.zeros((T0 % lanes, n_ch), np.complex64), tail[:7], np.zeros((1, n_ch), np.complex64), tail[7:]]), axes, n_bins, lanes)
    assert not np.array_equal(moved.S, m.S)


def test_every_refusal(stats, gsdr_lib):
    from gpu_sdr_amd import GsdrError
    L = gsdr_lib
    ax = np.zeros(2, dtype=LEVEL_DTYPE)
    ax["dx"], ax["hi"] = 1, 1
    p = ax.ctypes.data

    def err():
        return L.gsdr_last_error(None).decode()
    for args, word in (((0, 8, 4, 1, p, -2), "n_ch"), (((1 << 20) + 1, 8, 4, 1, p, -2), "n_ch"), ((2, 0, 4, 1, p, -2), "max_rows"),
                       ((2, (1 << 20) + 1, 4, 1, p, -2), "max_rows"), ((2, 8, 0, 1, p, -2), "n_bins"), ((2, 8, 4097, 1, p, -2), "n_bins"),
                       ((2, 8, 4, -1, p, -2), "lanes"), ((2, 8, 4, 3, p, -2), "lanes"), ((2, 8, 4, 65536, p, -2), "lanes"),
                       ((2, 8, 4, 1, None, -2), "axes"), ((2, 8, 4, 1, p, -3), "device_index")):
        assert not L.gsdr_stats_create(*args) and err().startswith("gsdr_stats_create: ") and word in err(), args
    for lo, hi in ((1, 1), (2, 1), (np.nan, 1), (0, np.inf), (-np.inf, 0), (0, np.nan)):
        bad = ax.copy()
        bad["lo"][1], bad["hi"][1] = lo, hi
        assert not L.gsdr_stats_create(2, 8, 4, 1, bad.ctypes.data, -2) and "axes" in err() and "channel 1" in err()
    h = stats.host_stats(2, 8, 4, ax, lanes=2)
    rows = np.zeros((9, 2), dtype=np.complex64)
    with pytest.raises(GsdrError, match="gsdr_stats_feed_host: .*n_rows"):
        h.feed(rows)
    assert L.gsdr_stats_feed_host(h._h, rows.ctypes.data, -1) == -1 and L.gsdr_stats_feed_host(h._h, None, 1) == -1 and "rows" in err()
    assert L.gsdr_stats_feed_host(h._h, None, 0) == 0
    assert L.gsdr_stats_feed_device(h._h, rows.ctypes.data, 1, None) == -1 and "host object" in err()
    assert L.gsdr_stats_read(h._h, rows.ctypes.data, None) == -1 and L.gsdr_stats_read_device(h._h, rows.ctypes.data, None) == -1
    assert L.gsdr_stats_read_host(h._h, None) == -1 and L.gsdr_stats_counts(h._h, None, None) == -1
    out = np.zeros(64)
    pr = (C.c_double * 17)(*([0.5] * 17))
    assert L.gsdr_stats_quantiles(h._h, pr, 0, out.ctypes.data, None) == -1 and L.gsdr_stats_quantiles(h._h, pr, 17, out.ctypes.data, None) == -1
    assert L.gsdr_stats_quantiles(h._h, None, 1, out.ctypes.data, None) == -1 and L.gsdr_stats_quantiles(h._h, pr, 1, None, None) == -1
    for v in (0.0, -0.1, 1.0000001, np.nan):
        with pytest.raises(GsdrError, match=r"gsdr_stats_quantiles: pr"):
            h.quantiles([0.5, v])
    for centre, nsigma in ((2, 1.0), (-1, 1.0), (0, np.nan), (0, np.inf), (1, -1.0)):
        assert L.gsdr_stats_levels(h._h, centre, nsigma, None, out.ctypes.data, None) == -1 and err().startswith("gsdr_stats_levels: ")
    assert L.gsdr_stats_levels(h._h, 0, 1.0, None, None, None) == -1
    bad = ax.copy()
    bad["hi"][0] = 0
    with pytest.raises(GsdrError, match="gsdr_stats_reset: axes"):
        h.reset(bad)
    assert np.array_equal(h.axes, ax) and h.rows_seen == 0
    h.feed(rows[:8])
    assert h.rows_seen == 8                                                          # no refusal moved the stream
    h.close()
    # a NULL object
    assert L.gsdr_stats_rows(None) == 0 and L.gsdr_stats_lanes(None) == 0 and L.gsdr_stats_n_bins(None) == 0
    assert L.gsdr_stats_feed_host(None, None, 0) == -1 and L.gsdr_stats_reset(None, None) == -1 and L.gsdr_stats_read_host(None, out.ctypes.data) == -1
    assert L.gsdr_stats_feed_device(None, None, 0, None) == -1 and L.gsdr_stats_counts(None, out.ctypes.data, None) == -1
    assert L.gsdr_stats_quantiles(None, pr, 1, out.ctypes.data, None) == -1 and L.gsdr_stats_levels(None, 0, 1.0, None, out.ctypes.data, None) == -1
    L.gsdr_stats_close(None)
    with pytest.raises(ValueError):
        stats.device_stats(2, 8, 4, ax, device_index=-2)
