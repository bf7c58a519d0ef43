"""The row statistics on the GPU (include/gsdr.h, "row statistics on the device"): the device against the host twin, bit
for bit -- summaries, counters, quantiles and levels -- for every shape at which stats_feed_kernel and stats_read_kernel
(stats_kernels.hip) take another path: one thread in use, a half-empty channel tile, many channel tiles, more lanes than
a feed has rows, more lanes than rows at all, the tree's levels above 256 chains, 4 096 bins in a two-channel tile, and
the lanes rule.  Every cutting, two runs, reads in mid-stream, reset with new axes, poison, guard zones and offset
pointers, a stream of the caller's, and the chain DIRECT handle -> resmap -> stats -> levels -> trigger.

The measured distances to numpy (the bounds are asserted in tests/test_stats_host.py on the same law) are written to
the file that GSDR_STATS_MARGINS names, when it is set; profiles/stats_margins.json is the committed copy."""
import json
import os

import numpy as np
import pytest

from _extents import OUT_SENTINEL_BITS, check_input_untouched, guarded_input, guarded_output
from _stats import LEVEL_DTYPE, cuttings, feed_cut, project, same_doubles, stream

pytestmark = pytest.mark.gpu

STATS_MARGINS = {}
PR = [0.01, 0.25, 0.5, 0.999, 1.0]


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


def results_of(obj):
    return obj.read(), obj.counts(), obj.quantiles(PR), obj.levels(5.0, "median"), obj.levels(3.0, "mean")


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
