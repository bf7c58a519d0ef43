"""The row statistics on the GPU (include/gsdr.h, "row statistics on the device"): the device against the host twin, bit
for bit -- summaries, counters, quantiles and levels -- for every shape at which stats_feed_kernel and stats_read_kernel
(stats_kernels.hip) take another path: one thread in use, a half-empty channel tile, many channel tiles, more lanes than
a feed has rows, more lanes than rows at all, the tree's levels above 256 chains, 4 096 bins in a two-channel tile, and
the lanes rule.  Every cutting, two runs, reads in mid-stream, reset with new axes, poison, guard zones and offset
pointers, a stream of the caller's, and the chain DIRECT handle -> resmap -> stats -> levels -> trigger.

Below those, the device against the numpy Model of tests/_stats.py directly (and the twin wherever it can run the case):
the tile edges of the launch rule with the plan gsdr_stats_plan reports, the four 65 536-byte LDS tables among them; the
edge laws of the bins, the chains and the quantiles; every rank of a small channel; degenerate and masked channels; one
column through one thread and through full tiles; and a stream of more than 2^32 rows against a closed form.

The measured distances to numpy (the bounds are asserted in tests/test_stats_host.py on the same law) are written to
the file that GSDR_STATS_MARGINS names, when it is set; profiles/stats_margins.json is the committed copy."""
import json
import os

import numpy as np
import pytest

from _extents import OUT_SENTINEL_BITS, check_input_untouched, guarded_input, guarded_output
from _stats import (LEVEL_DTYPE, PIVOT_AXIS, Model, after_a_prefix_of_pivot_rows, cuttings, feed_cut, project, same_doubles, same_summary,
                    stream)

pytestmark = pytest.mark.gpu

STATS_MARGINS = {}
PR = [0.01, 0.25, 0.5, 0.999, 1.0]
PR16 = [k / 16 for k in range(1, 17)]                      # GSDR_STATS_MAX_QUANTILES of them


@pytest.fixture(scope="module")
def stats(gsdr_lib):
    from gpu_sdr_amd import stats
    yield stats
    path = os.environ.get("GSDR_STATS_MARGINS")
    if STATS_MARGINS and path:
        doc = {"metrics": {"mean": "max over channels of |mean - numpy.mean(q)| / (n 2^-52 max|q - p|), the any-order bound: <= 1",
                           "var": "max over channels of |var - numpy.var(q, ddof=1)| / var: bar 1e-9",
                           "quantile": "max over channels and pr of |quantile - sorted(q)[t - 1]| / w: < 1 by construction"},
               "per_case": dict(sorted(STATS_MARGINS.items()))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


# name: (n_ch, rows, n_bins, lanes, rows per feed)
SHAPES = {
    "1x1": (1, 1, 1, 1, 1),
    "3x257": (3, 257, 7, 4, 257),
    "5x5000": (5, 5000, 256, 64, 5000),
    "130x700": (130, 700, 256, 16, 700),           # 4 full channel tiles and one of 2 channels
    "2048x130": (2048, 130, 64, 2, 130),
    "2x40000": (2, 40000, 1024, 4096, 100),        # most chains get no row in a feed
    "1x10": (1, 10, 4, 32768, 10),                 # more lanes than rows
    "4x3000": (4, 3000, 4096, 64, 3000),           # a tile of two channels
    "rule 7x900": (7, 900, 100, 0, 900),
    "rule 300x64": (300, 64, 33, 0, 64),
}

_memo = {}


def case_of(name):
    """(rows, axes) of a shape, made once and left unchanged; the last channel carries the wide-range column."""
    if name not in _memo:
        n_ch, n, _, _, _ = SHAPES[name]
        _memo[name] = stream(n, n_ch, seed=7, wide=(n_ch - 1,))
    return _memo[name]


def results_of(obj, pr=PR):
    return obj.read(), obj.counts(), obj.quantiles(pr), obj.levels(5.0, "median"), obj.levels(3.0, "mean")


def twin_of(stats, name):
    key = ("twin", name)
    if key not in _memo:
        n_ch, n, n_bins, lanes, per = SHAPES[name]
        rows, axes = case_of(name)
        h = stats.host_stats(n_ch, per, n_bins, axes, lanes=lanes)
        feed_cut(h, rows, cuttings(n, per)["whole"])
        _memo[key] = results_of(h) + (h.lanes,)
        h.close()
    return _memo[key]


def same_results(got, want):
    """"" or the first of summary, counts, quantiles, levels that differs (a NaN matching any NaN in the doubles)."""
    s, w = got[0], want[0]
    for f in ("n", "bad", "under", "over", "min", "max", "reserved"):
        if s[f].tobytes() != w[f].tobytes():
            return f"summary.{f}"
    for f in ("mean", "var"):
        if not same_doubles(s[f], w[f]):
            c = int(np.flatnonzero(~((s[f] == w[f]) | (np.isnan(s[f]) & np.isnan(w[f]))))[0])
            return f"summary.{f}[{c}]: {s[f][c]!r} != {w[f][c]!r}"
    if not np.array_equal(got[1], want[1]):
        return "counts"
    if not same_doubles(got[2], want[2]):
        return "quantiles"
    return "" if got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() else "levels"


def to_dev(rows, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows)).to(dev)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_host_twin(stats, cuda_device, name):
    n_ch, n, n_bins, lanes, per = SHAPES[name]
    rows, axes = case_of(name)
    want = twin_of(stats, name)
    xd = to_dev(rows, cuda_device)
    d = stats.device_stats(n_ch, per, n_bins, axes, lanes=lanes, device_index=0)
    assert d.lanes == want[5] and (lanes == 0 or d.lanes == lanes)
    feed_cut(d, xd, cuttings(n, per)["whole"])
    got = results_of(d)
    assert d.rows_seen == n
    d.close()
    assert same_results(got, want) == ""
    # the distances to numpy, on the Gaussian channels
    if n >= 100 and n_ch > 1:
        g = slice(0, n_ch - 1)
        q = project(rows, axes).astype(np.float64)[:, g]
        p = 0.5 * (axes["lo"].astype(np.float64) + axes["hi"].astype(np.float64))[g]
        w = ((axes["hi"].astype(np.float64) - axes["lo"].astype(np.float64)) / n_bins)[g]
        s = got[0][g]
        srt = np.sort(q, axis=0)
        ranks = [max(1, int(np.ceil(pr * n))) - 1 for pr in PR]
        STATS_MARGINS[name] = {
            "mean": float((np.abs(s["mean"] - q.mean(axis=0)) / (n * 2.0 ** -52 * np.abs(q - p).max(axis=0))).max()),
            "var": float((np.abs(s["var"] - q.var(axis=0, ddof=1)) / q.var(axis=0, ddof=1)).max()),
            "quantile": float((np.abs(got[2][g] - srt[ranks].T) / w[:, None]).max())}
        assert STATS_MARGINS[name]["mean"] <= 1.0 and STATS_MARGINS[name]["var"] <= 1e-9 and STATS_MARGINS[name]["quantile"] < 1.0


@pytest.mark.parametrize("name", ["3x257", "1x10", "130x700"])
def test_every_cutting_and_two_runs_give_the_same_bits(stats, cuda_device, name):
    n_ch, n, n_bins, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    want = twin_of(stats, name)
    xd = to_dev(rows, cuda_device)
    for max_rows in (n, 100):
        for cut_name, cut in cuttings(n, max_rows).items():
            for _ in range(2 if cut_name == "37" else 1):
                d = stats.device_stats(n_ch, max_rows, n_bins, axes, lanes=lanes, device_index=0)
                feed_cut(d, xd, cut)
                got = results_of(d)
                d.close()
                assert same_results(got, want) == "", (max_rows, cut_name)


def test_reads_in_mid_stream_and_reset_with_new_axes(stats, cuda_device):
    import torch
    name = "5x5000"
    n_ch, n, n_bins, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    xd = to_dev(rows, cuda_device)
    d = stats.device_stats(n_ch, n, n_bins, axes, lanes=lanes, device_index=0)
    h = stats.host_stats(n_ch, n, n_bins, axes, lanes=lanes)
    on_dev = torch.zeros(n_ch * 8, dtype=torch.float64, device=cuda_device)
    for a, b in ((0, 1234), (1234, 1235), (1235, 4000), (4000, 5000)):
        d.feed(xd[a:b]), h.feed(rows[a:b])
        assert same_results(results_of(d), results_of(h)) == "", b          # any number of reads, the accumulation goes on
        d.read_device(on_dev)
        torch.cuda.synchronize()
        assert on_dev.cpu().numpy().tobytes() == h.read().tobytes()
    assert same_results(results_of(d), twin_of(stats, name)) == ""
    # the two-pass use: the ranges of the second pass from the levels of the first
    fine = stats.axes_around(d.levels(8.0, "mean"))
    assert fine.tobytes() == stats.axes_around(h.levels(8.0, "mean")).tobytes()
    d.reset(fine), h.reset(fine)
    assert d.rows_seen == 0 and not d.counts().any() and d.read()["n"].sum() == 0
    d.feed(xd[:3000]), h.feed(rows[:3000])
    got, want = results_of(d), results_of(h)
    assert same_results(got, want) == "" and got[0].tobytes() != twin_of(stats, name)[0].tobytes()
    d.reset(), h.reset()
    d.feed(xd[:3000]), h.feed(rows[:3000])
    assert same_results(results_of(d), want) == ""
    d.close(), h.close()


def test_poison_in_one_channel_leaves_every_other_channel_alone(stats, cuda_device):
    name = "130x700"
    n_ch, n, n_bins, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    clean = twin_of(stats, name)
    c = 37
    bad = rows.copy()
    at = np.array([0, 5, 16, 17, 300, 699])
    bad[at, c] = np.array([np.nan, np.inf, -np.inf, complex(np.nan, 1), complex(0, np.inf), complex(1e38, 1e38)], dtype=np.complex64)
    ax = axes.copy()
    ax["dx"][c], ax["dy"][c] = 1e3, 1e3                   # 1e38 x 1e3 overflows: bad as well
    h = stats.host_stats(n_ch, n, n_bins, ax, lanes=lanes)
    h.feed(bad)
    want = results_of(h)
    h.close()
    d = stats.device_stats(n_ch, n, n_bins, ax, lanes=lanes, device_index=0)
    d.feed(to_dev(bad, cuda_device))
    got = results_of(d)
    d.close()
    assert same_results(got, want) == ""
    assert got[0]["bad"][c] == len(at) and got[0]["bad"].sum() == len(at) and got[0]["n"][c] == n - len(at)
    others = np.arange(n_ch) != c
    for g, w in zip(got, clean[:5]):
        assert g[others].tobytes() == w[others].tobytes()


@pytest.mark.parametrize("name", ["3x257", "130x700", "2048x130"])
def test_guard_zones_and_offset_pointers(stats, gsdr_lib, cuda_device, name):
    """The rows and the summaries in the middle of larger allocations, on a 16-byte boundary and 8 bytes past one: a feed
    reads rows_dev[0, n_rows n_ch) only and leaves it as it was, a read writes summary_dev[0, n_ch) only."""
    import torch
    n_ch, n, n_bins, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    want = twin_of(stats, name)
    sentinel = np.uint32(OUT_SENTINEL_BITS)
    for off, pattern in ((0, "nan"), (1, "huge")):
        d = stats.device_stats(n_ch, n, n_bins, axes, lanes=lanes, device_index=0)
        whole_in, view_in = guarded_input(rows.reshape(-1), off, pattern, cuda_device)
        assert gsdr_lib.gsdr_stats_feed_device(d._h, view_in.data_ptr(), n, None) == 0
        whole_out, view_out = guarded_output(n_ch * 8, off, cuda_device)
        assert gsdr_lib.gsdr_stats_read_device(d._h, view_out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        check_input_untouched(whole_in, rows.reshape(-1), off, pattern)
        bits = whole_out.cpu().numpy().view(np.uint32)
        first = (view_out.data_ptr() - whole_out.data_ptr()) // 8
        assert (bits[:2 * first] == sentinel).all() and (bits[2 * (first + n_ch * 8):] == sentinel).all()
        assert view_out.cpu().numpy().tobytes() == want[0].tobytes()
        assert same_results(results_of(d), want) == ""
        # a pointer 4 bytes past a sample is refused, and so is a feed that is too long
        assert gsdr_lib.gsdr_stats_feed_device(d._h, view_in.data_ptr() + 4, 1, None) == -1
        assert gsdr_lib.gsdr_stats_read_device(d._h, view_out.data_ptr() + 4, None) == -1
        assert gsdr_lib.gsdr_stats_feed_device(d._h, view_in.data_ptr(), n + 1, None) == -1
        assert gsdr_lib.gsdr_stats_feed_device(d._h, None, 1, None) == -1 and gsdr_lib.gsdr_stats_feed_device(d._h, None, 0, None) == 0
        assert gsdr_lib.gsdr_stats_feed_host(d._h, rows.ctypes.data, 1) == -1 and gsdr_lib.gsdr_stats_read_host(d._h, rows.ctypes.data) == -1
        assert d.rows_seen == n and same_results(results_of(d), want) == ""
        d.close()


def test_a_stream_of_the_callers(stats, cuda_device):
    """Feeds, a read on the device, more feeds, all on one side stream with no wait in between; then the entries that
    return to the host, which wait for that stream."""
    import torch
    name = "2x40000"
    n_ch, n, n_bins, lanes, per = SHAPES[name]
    rows, axes = case_of(name)
    want = twin_of(stats, name)
    xd = to_dev(rows, cuda_device)
    half = torch.zeros(n_ch * 8, dtype=torch.float64, device=cuda_device)
    d = stats.device_stats(n_ch, per, n_bins, axes, lanes=lanes, device_index=0)
    torch.cuda.synchronize()
    stream_ = torch.cuda.Stream()
    for at in range(0, n, per):
        d.feed_device(xd[at:at + per], stream=stream_)
        if at + per == n // 2:
            d.read_device(half, stream=stream_)
    got = (d.read(stream=stream_), d.counts(stream=stream_), d.quantiles(PR, stream=stream_), d.levels(5.0, "median", stream=stream_),
           d.levels(3.0, "mean", stream=stream_))
    d.close()
    assert same_results(got, want) == ""
    h = stats.host_stats(n_ch, n, n_bins, axes, lanes=lanes)
    h.feed(rows[:n // 2])
    assert half.cpu().numpy().tobytes() == h.read().tobytes()
    h.close()


def test_handle_resmap_stats_levels_trigger_chain(stats, cuda_device):
    """DIRECT, 8 tones, decim 50, buffer 50 000: 1000 rows per buffer.  The handle's output goes through a resmap object
    (5 tones, calibrated S21) into a stats object, all on one stream; a coarse first pass over two buffers gives the
    ranges of a second pass over two more; its levels go into a trigger, and a step injected into one channel of a fifth
    buffer is found at the row where it was put."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd import resmap
    from gpu_sdr_amd.source import host_tones
    from _resmap import fit_of
    rate, L, n_ch = 1_000_000, 50_000, 8
    freq = [-400_000, -300_000, -200_000, -100_000, 100_000, 200_000, 300_000, 400_000]
    channels = [1, 2, 4, 6, 7]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=L, decim=50, pf_average=4, freq=freq,
                                          wave_type=[g.w_type.DIRECT] * n_ch), device_index=0)
    max_rows = dem.out_capacity // n_ch
    rng = np.random.default_rng(37)
    fits, tones = zip(*[fit_of(rng) for _ in channels])
    m = resmap.device_resmap(n_ch, max_rows, resmap.resmap_constants(fits, tones), channels=channels, kind="cal", device_index=0)
    coarse = np.zeros(len(channels), dtype=LEVEL_DTYPE)
    coarse["dx"], coarse["lo"], coarse["hi"] = 1, -1000, 1000
    st = stats.device_stats(len(channels), max_rows, 256, coarse, device_index=0)
    twin = stats.host_stats(len(channels), max_rows, 256, coarse)
    assert st.lanes == twin.lanes
    ampl, phase = np.full(n_ch, 0.1, dtype=np.float32), np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream_ = torch.cuda.Stream()

    def mapped(b):
        xin = torch.from_numpy(host_tones(L, b * L, rate, freq, ampl, phase, sigma=2e-2, seed=40 + b)).to(cuda_device)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        y = torch.empty((max_rows, len(channels)), dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        n = dem.process_device(xin, out, stream=stream_)
        assert n > 0 and n % n_ch == 0 and m.feed_device(out[:n], y, stream=stream_) == n // n_ch
        return y[:n // n_ch], out

    kept = []
    for b in (0, 1):
        y, out = mapped(b)
        st.feed_device(y, stream=stream_)
        kept.append((y, out))
    first = st.levels(8.0, "mean", stream=stream_)                 # waits for the stream
    for y, _ in kept:
        twin.feed(y.cpu().numpy())
    assert first.tobytes() == twin.levels(8.0, "mean").tobytes() and np.isfinite(first["lo"]).all()
    fine = stats.axes_around(first)
    st.reset(fine), twin.reset(fine)
    kept = []
    for b in (2, 3):
        y, out = mapped(b)
        st.feed_device(y, stream=stream_)
        kept.append((y, out))
    levels = st.levels(6.0, "median", stream=stream_)
    summary = st.read(stream=stream_)
    for y, _ in kept:
        twin.feed(y.cpu().numpy())
    assert levels.tobytes() == twin.levels(6.0, "median").tobytes() and summary.tobytes() == twin.read().tobytes()
    assert summary["n"].min() == 2000 and not summary["bad"].any() and not summary["under"].any() and not summary["over"].any()
    # the trigger takes the table as it is
    trig = g.device_trigger(len(channels), max_rows, 2, 2, 10_000, 8, np.zeros((len(channels), 6), dtype=np.float32), device_index=0)
    trig.set_levels(levels, stream=stream_)
    y, out = mapped(4)
    row, ch = 613, 3
    sigma = float(np.sqrt(summary["var"][ch]))
    with torch.cuda.stream(stream_):
        quiet = y.clone()
        y[row:, ch] += 20.0 * sigma
    ev, sn, dropped = trig.feed(y, stream=stream_)
    assert dropped == 0 and len(ev) == 1 and ev["row"][0] == row and ev["channel"][0] == ch and ev["side"][0] == 1
    assert np.array_equal(sn[0, :2], quiet[row - 2:row].cpu().numpy())
    trig.close(), st.close(), twin.close(), m.close(), dem.close()


# ---- against the numpy model directly, at the shapes the ten above leave out ------------------------------------------------

def same_as_model(got, m, pr=PR):
    """"" or the first of summary, counts, quantiles, levels that is not the Model's, bit for bit."""
    d = same_summary(got[0], m.summary())
    if d:
        return "summary." + d
    if not np.array_equal(got[1], m.counts):
        return "counts"
    if not same_doubles(got[2], m.quantiles(pr)):
        return "quantiles"
    return "" if got[3].tobytes() == m.levels(5.0, "median").tobytes() and got[4].tobytes() == m.levels(3.0, "mean").tobytes() else "levels"


def device_twin_model(stats, dev, rows, axes, n_bins, lanes, pr=PR, cut=None):
    """The device's results and the Model of rows fed as `cut`, after device == twin == Model has been asserted."""
    n, n_ch = rows.shape
    cut = cut or [n]
    d = stats.device_stats(n_ch, max(cut), n_bins, axes, lanes=lanes, device_index=0)
    h = stats.host_stats(n_ch, max(cut), n_bins, axes, lanes=lanes)
    feed_cut(d, to_dev(rows, dev), cut), feed_cut(h, rows, cut)
    got, twin = results_of(d, pr), results_of(h, pr)
    assert d.rows_seen == n
    d.close(), h.close()
    m = Model(rows, axes, n_bins, lanes)
    assert same_results(got, twin) == "" and same_as_model(got, m, pr) == ""
    return got, m


# The four n_bins at which a tile's table is EXACTLY the 65 536 bytes of LDS the rule allows, and the next, where the tile
# halves; one channel more than the larger tile.  name: (n_ch, n_bins, tile, lds_bytes)
EDGES = {
    "33x509": (33, 509, 32, 65536), "33x510": (33, 510, 16, 16 * 513 * 4),
    "17x1021": (17, 1021, 16, 65536), "17x1022": (17, 1022, 8, 8 * 1025 * 4),
    "9x2045": (9, 2045, 8, 65536), "9x2046": (9, 2046, 4, 4 * 2049 * 4),
    "5x4093": (5, 4093, 4, 65536), "5x4094": (5, 4094, 2, 2 * 4097 * 4),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_the_tile_edges_of_the_feed(stats, cuda_device, name):
    """601 rows, lanes 8, the wide column in the last channel (the tile of one channel).  Every channel also has one sample
    below lo, one above hi and one NaN, so that the LAST counters of every channel -- the end of the run of counters a
    tile flushes -- are not zero."""
    n_ch, n_bins, tile, lds = EDGES[name]
    n, lanes = 601, 8
    assert stats.feed_plan(n_ch, n_bins, lanes) == dict(tile=tile, tiles=-(-n_ch // tile), splits=-(-lanes // (256 // tile)), lds_bytes=lds)
    rows, axes = stream(n, n_ch, seed=7, wide=(n_ch - 1,))
    c = np.arange(n_ch)
    span = axes["hi"].astype(np.float64) - axes["lo"].astype(np.float64)
    along = axes["dx"].astype(np.float64) + 1j * axes["dy"].astype(np.float64)            # |along| = 1: q moves by what it is scaled by
    base = axes["bx"].astype(np.float64) + 1j * axes["by"].astype(np.float64)
    rows[3 + c % 7, c] = np.nan
    rows[100 + c % 5, c] = (base + (axes["hi"] + span) * along).astype(np.complex64)
    rows[590 + c % 11, c] = (base + (axes["lo"] - span) * along).astype(np.complex64)
    got, _ = device_twin_model(stats, cuda_device, rows, axes, n_bins, lanes)
    s = got[0]
    assert (s["bad"] == 1).all() and (s["over"] == 1).all() and (s["under"] == 1).all() and (s["n"] == n - 1).all()
    assert (got[1][:, -1] == 1).all() and (got[1][:, -2] == 1).all() and (got[1][:, 0] == 1).all()


def test_edge_laws_of_the_bins_and_the_chains_on_the_device(stats, cuda_device):
    """tests/test_stats_host.py, test_edge_laws_of_the_bins_and_the_chains, with the device in the twin's place: the same
    header compiled by another compiler for another target, where float32 denormals and contraction could differ."""
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
        got, _ = device_twin_model(stats, cuda_device, rows, axes, n_bins, 2)
        summary, counts = got[0], got[1]
        c0 = counts[0]
        assert c0[0] == 1 and c0[n_bins + 1] == 2 and c0[n_bins + 2] == 3          # below_lo | hi, 1e38 | nan, +-inf
        assert c0[n_bins] >= 1                                                       # below_hi lies in the last bin
        assert c0[1] >= 1 and (n_bins == 1 or c0[1] == 1)                            # lo itself opens bin 0
        assert counts[1][n_bins + 2] == 4                                            # 1e38 x 1e3 overflowed
        assert summary["min"][0] == below_lo and summary["max"][0] == np.float32(1e38)
        assert summary["n"][0] == len(vals) - 3 and summary["bad"][0] == 3
    # -0.0 against +0.0: the earlier one stays (q = -0 needs both terms -0: x = y = -0 with dy = +0)
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        pair = np.array([first, first, second, second], dtype=np.float32).view(np.complex64).reshape(2, 1)
        got, _ = device_twin_model(stats, cuda_device, pair, axes[:1], 4, 1)
        s = got[0]
        assert np.signbit(s["min"][0]) == np.signbit(np.float32(first)) and np.signbit(s["max"][0]) == np.signbit(np.float32(first))


def test_denormals_next_to_the_range_edge_on_the_device(stats, cuda_device):
    """lo = 0: -1e-45 is below the range (under), +1e-45, +0 and -0 open bin 0.  A device that flushed float32 denormals
    would count -1e-45 in bin 0 and report a minimum of -0."""
    axes = np.zeros(1, dtype=LEVEL_DTYPE)
    axes[0] = (0, 0, 1, 0, 0.0, 1.0)
    tiny = np.float32(1e-45)
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    below_1 = np.nextafter(np.float32(1), np.float32(0))
    x = np.array([tiny, -tiny, 0.0, -0.0, 1.0, below_1], dtype=np.float32)
    rows = np.zeros((len(x), 1), dtype=np.complex64)
    rows[:, 0] = x
    rows[3, 0] = complex(-0.0, -0.0)                       # q = -0 needs both terms -0
    for n_bins in (1, 8, 4096):
        for lanes in (1, 4):
            got, m = device_twin_model(stats, cuda_device, rows, axes, n_bins, lanes, pr=PR16)
            assert np.signbit(m.q[3, 0]) and m.q[3, 0] == 0
            s, cnt = got[0], got[1][0]
            assert (cnt[0], cnt[1], cnt[n_bins], cnt[n_bins + 1], cnt[n_bins + 2]) == (1, 3 + (n_bins == 1), 1 + 3 * (n_bins == 1), 1, 0)
            assert s["min"][0] == -tiny and s["max"][0] == 1.0 and s["n"][0] == 6 and s["under"][0] == 1 and s["over"][0] == 1


def test_n_0_n_1_and_ranks_outside_the_range_on_the_device(stats, cuda_device):
    """tests/test_stats_host.py, test_n_0_n_1_and_ranks_outside_the_range, on the device and against the Model."""
    axes = np.zeros(1, dtype=LEVEL_DTYPE)
    axes[0] = (0, 0, 1, 0, 0.0, 1.0)
    d = stats.device_stats(1, 16, 8, axes, lanes=4, device_index=0)
    s = d.read()
    assert s["n"][0] == 0 and np.isnan(s["mean"][0]) and np.isnan(s["var"][0]) and s["min"][0] == np.inf and s["max"][0] == -np.inf
    assert np.isnan(d.quantiles([0.5])[0, 0]) and np.isnan(d.quantiles(PR16)).all()
    lv = d.levels(3.0)
    assert lv["lo"][0] == -np.inf and lv["hi"][0] == np.inf and lv["dx"][0] == 1
    assert same_as_model(results_of(d, PR16), Model(np.zeros((0, 1), dtype=np.complex64), axes, 8, 4), PR16) == ""
    one = np.array([[0.30]], dtype=np.complex64)
    d.feed(to_dev(one, cuda_device))
    s = d.read()
    assert s["n"][0] == 1 and s["mean"][0] == 0.5 + (np.float64(np.float32(0.30)) - 0.5) and np.isnan(s["var"][0])
    assert s["min"][0] == s["max"][0] == np.float32(0.30)
    assert d.levels(3.0)["lo"][0] == -np.inf                                         # n < 2: switched off
    q = d.quantiles([0.5, 1.0])[0]
    assert q[0] == q[1] == 0.0 + (2.0 + (1.0 - 0.5) / 1.0) * 0.125                    # bin 2, the middle of it
    assert same_as_model(results_of(d, PR16), Model(one, axes, 8, 4), PR16) == ""
    d.reset()
    assert d.rows_seen == 0 and d.read()["n"][0] == 0 and not d.counts().any()
    # three below, one inside, four above: ranks 1-3 -> -inf, 4 -> the bin, 5-8 -> +inf
    eight = np.array([[-1], [-2], [-3], [0.55], [2], [3], [4], [1.0]], dtype=np.complex64)
    d.feed(to_dev(eight, cuda_device))
    pr = [1 / 8, 3 / 8, 4 / 8, 5 / 8, 1.0]
    q = d.quantiles(pr)[0]
    assert list(q[:2]) == [-np.inf, -np.inf] and 0.5 <= q[2] < 0.625 and list(q[3:]) == [np.inf, np.inf]
    s = d.read()
    assert (s["under"][0], s["over"][0], s["n"][0]) == (3, 4, 8)
    m = Model(eight, axes, 8, 4)
    assert same_as_model(results_of(d, pr), m, pr) == "" and same_as_model(results_of(d, PR16), m, PR16) == ""
    d.close()


def test_every_rank_of_a_small_channel_on_the_device(stats, cuda_device):
    """16 samples in 300 bins of width 1 (a thread of stats_read_kernel sums two bins: bins 1 | 2 and 255 | 256 lie in
    different threads): three below lo, two above hi, the rest in bins 0, 1, 2, 255, 256 and 299.  pr = k / 16 is rank k:
    -Inf for 1 .. 3, +Inf for 15 and 16, the Model's value between -- all 16 in one call (the kernel picks pr[k] through a
    compare chain of GSDR_STATS_MAX_QUANTILES = 16) and each alone."""
    axes = np.zeros(1, dtype=LEVEL_DTYPE)
    axes[0] = (0, 0, 1, 0, 0.0, 300.0)
    x = np.array([299.5, -1, 0.5, 255.5, 301, 1.5, 2.5, -2, 256.5, 0.25, 299.9, 2.75, 400, 255.1, -3, 299.0], dtype=np.float32)
    rows = np.zeros((16, 1), dtype=np.complex64)
    rows[:, 0] = x
    for lanes in (4, 1):
        got, m = device_twin_model(stats, cuda_device, rows, axes, 300, lanes, pr=PR16)
        cnt = got[1][0]
        assert cnt[0] == 3 and cnt[301] == 2 and [int(cnt[1 + b]) for b in (0, 1, 2, 255, 256, 299)] == [2, 1, 2, 2, 1, 3] and cnt.sum() == 16
        q = got[2][0]
        assert list(q[:3]) == [-np.inf] * 3 and list(q[14:]) == [np.inf] * 2 and np.isfinite(q[3:14]).all()
        assert [int(v) for v in q[3:14]] == [0, 0, 1, 2, 2, 255, 255, 256, 299, 299, 299]      # the bin of each rank
        assert (np.diff(q[3:14]) > 0).all()
    d = stats.device_stats(1, 16, 300, axes, lanes=4, device_index=0)
    d.feed(to_dev(rows, cuda_device))
    for k, pr in enumerate(PR16):
        assert same_doubles(d.quantiles([pr]), m.quantiles([pr])) and same_doubles(d.quantiles([pr])[0, 0], got[2][0, k]), k + 1
    d.close()


def test_degenerate_and_masked_channels_on_the_device(stats, cuda_device):
    """In one read: 5 000 equal samples (one bin, variance 0), a channel without a finite sample (n = 0: NaN quantiles, levels
    off), a channel with one (n = 1: levels off), an ordinary one; and levels with a mask."""
    n, n_ch, n_bins, lanes = 5000, 4, 64, 8
    rows, axes = stream(n, n_ch, seed=13)
    rows[:, 0] = rows[17, 0]
    rows[:, 1] = np.nan
    keep = rows[4321, 2]
    rows[:, 2] = complex(np.inf, 0)
    rows[4321, 2] = keep
    got, m = device_twin_model(stats, cuda_device, rows, axes, n_bins, lanes, pr=PR16, cut=[1200, 1200, 1200, 1200, 200])
    s, q = got[0], got[2]
    assert list(s["n"]) == [n, 0, 1, n] and list(s["bad"]) == [0, n, n - 1, 0]
    assert s["var"][0] == 0 and s["min"][0] == s["max"][0] and (got[1][0] == n).sum() == 1
    assert (np.diff(q[0]) > 0).all() and q[0][15] - q[0][0] < m.w[0]                  # 16 ranks inside one bin
    assert np.isnan(q[1]).all() and np.isnan(s["mean"][1]) and s["min"][1] == np.inf and s["max"][1] == -np.inf
    assert (q[2] == q[2][0]).all() and np.isfinite(q[2]).all() and np.isnan(s["var"][2])
    for lv in got[3], got[4]:
        assert list(np.isinf(lv["lo"])) == [False, True, True, False] and list(np.isinf(lv["hi"])) == [False, True, True, False]
    assert got[4]["lo"][0] == got[4]["hi"][0]                                         # sigma = 0: the level is the mean
    d = stats.device_stats(n_ch, n, n_bins, axes, lanes=lanes, device_index=0)
    h = stats.host_stats(n_ch, n, n_bins, axes, lanes=lanes)
    d.feed(to_dev(rows, cuda_device)), h.feed(rows)
    for on in ([1, 1, 1, 0], [0, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]):
        for centre, nsigma in (("median", 5.0), ("mean", 3.0)):
            lv = d.levels(nsigma, centre, on=on)
            assert lv.tobytes() == h.levels(nsigma, centre, on=on).tobytes() == m.levels(nsigma, centre, on=on).tobytes(), (on, centre)
            assert list(np.isfinite(lv["lo"])) == [bool(on[0]), False, False, bool(on[3])]
    d.close(), h.close()


def test_the_same_column_through_one_thread_and_through_full_tiles(stats, cuda_device):
    """The wide column alone with lanes 1 (tile 1: one thread of one workgroup does everything), and in each of 64
    channels with lanes 4 (two tiles of 32): every channel gives channel 0's bits, and those are the Model's."""
    n, n_bins = 1003, 100
    rows, axes = stream(n, 1, seed=19, wide=(0,))
    assert stats.feed_plan(1, n_bins, 1) == dict(tile=1, tiles=1, splits=1, lds_bytes=412)
    device_twin_model(stats, cuda_device, rows, axes, n_bins, 1, pr=PR16, cut=[500, 3, 500])
    assert stats.feed_plan(64, n_bins, 4) == dict(tile=32, tiles=2, splits=1, lds_bytes=32 * 412)
    many, many_axes = np.ascontiguousarray(np.repeat(rows, 64, axis=1)), np.repeat(axes, 64)
    got, m = device_twin_model(stats, cuda_device, many, many_axes, n_bins, 4, pr=PR16, cut=[500, 3, 500])
    for g in got:
        assert all(g[c].tobytes() == g[0].tobytes() for c in range(64))
    one = Model(rows, axes, n_bins, 4)
    assert same_summary(got[0][:1], one.summary()) == "" and same_doubles(got[2][:1], one.quantiles(PR16))


# ---- more rows than 2^32 -------------------------------------------------------------------------------------------------------
# Two channels on PIVOT_AXIS (q = Re x, range -/+ 2^23, the pivot 0), 256 bins, lanes 32 768.  A prefix of T0 = 4100 (2^20 - 1)
# rows of 0 + 0j -- each adds exactly +0 to its chain and counts in one bin --, then 70 001 wide rows in three pieces that
# begin at stream positions which are no multiple of lanes.  Neither the twin nor the Model can take 4.3 10^9 rows: the
# expected result is after_a_prefix_of_pivot_rows (tests/_stats.py; held against the twin at a small T0 in
# tests/test_stats_host.py).
BIG_K, BIG_PER, BIG_LANES, BIG_BINS = 4100, (1 << 20) - 1, 32768, 256
BIG_T0 = BIG_K * BIG_PER
BIG_TAIL = (7, 40001, 29993)


def big_case():
    if "big" not in _memo:
        tail, axes = stream(sum(BIG_TAIL), 2, seed=11, wide=(0, 1))
        assert np.array_equal(axes, np.array([PIVOT_AXIS] * 2, dtype=LEVEL_DTYPE))
        _memo["big"] = tail, axes, after_a_prefix_of_pivot_rows(BIG_T0, tail, axes, BIG_BINS, BIG_LANES)
    return _memo["big"]


def big_run(stats, dev, per):
    """The results of the stream above with the prefix in feeds of `per` rows (and a shorter last one), asserted along the
    way; made once per `per`.  The feeds are chained: the first that is refused raises and ends the test."""
    import torch
    if ("big", per) in _memo:
        return _memo[("big", per)]
    tail, axes, m = big_case()
    assert BIG_T0 > 1 << 32 and BIG_T0 % BIG_LANES == 28668
    zeros = torch.zeros((per, 2), dtype=torch.complex64, device=dev)
    d = stats.device_stats(2, per, BIG_BINS, axes, lanes=BIG_LANES, device_index=0)
    fed, feeds = 0, 0
    while fed < BIG_T0:
        k = min(per, BIG_T0 - fed)
        d.feed(zeros if k == per else zeros[:k])
        fed, feeds = fed + k, feeds + 1
        if feeds == 2049:                                         # past 2^31 rows, and 2^31 in one counter
            assert d.rows_seen == fed > 1 << 31
            assert (d.read()["n"] == fed).all() and (d.counts()[np.arange(2), m.pivot_slot] == fed).all()
    assert d.rows_seen == BIG_T0 and feeds == -(-BIG_T0 // per)
    feed_cut(d, to_dev(tail, dev), BIG_TAIL)
    got = results_of(d, PR16)
    assert d.rows_seen == BIG_T0 + tail.shape[0] > 1 << 32
    d.close()
    assert (got[0]["n"] == BIG_T0 + tail.shape[0]).all() and (got[1][np.arange(2), m.pivot_slot] > 1 << 32).all()
    _memo[("big", per)] = got
    return got


def test_more_than_2_32_rows_against_the_closed_form(stats, cuda_device):
    """4100 feeds of 2^20 - 1 rows, then the tail: rows_seen, n and one counter pass 2^31 (asserted after 2049 feeds) and
    2^32; counts, summaries, 16 quantiles and both kinds of levels are the construction's, bit for bit.  Measured on the
    MI355X (--durations, one run): 0.06 s for this test, 0.04 s for the next."""
    _, _, m = big_case()
    assert same_as_model(big_run(stats, cuda_device, BIG_PER), m, PR16) == ""


def test_more_than_2_32_rows_in_feeds_of_2_20_rows(stats, cuda_device):
    """The same stream with the prefix in feeds of 2^20 rows = the largest max_rows, every row of a feed in one bin (the
    32-bit counters of the LDS table reach the bound the kernel states for them), and one shorter feed up to the same T0:
    the same bits as with feeds of 2^20 - 1 rows, whose feeds begin at other phases, and the construction's."""
    _, _, m = big_case()
    got = big_run(stats, cuda_device, 1 << 20)
    assert same_as_model(got, m, PR16) == ""
    assert same_results(got, big_run(stats, cuda_device, BIG_PER)) == ""
