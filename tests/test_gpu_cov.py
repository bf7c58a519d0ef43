"""The channel covariance on the GPU (include/gsdr.h, "channel covariance on the device"): the device against the host
twin, bit for bit (a NaN matching any NaN), for all three reads, at every shape at which cov_project_kernel,
cov_accumulate_kernel and cov_read_kernel (cov_kernels.hip) take another path: one variable and one row; a partial tile, a
full tile and the first off-diagonal pair with a one-variable edge at the largest tile T the plan reports; six tile
pairs with one chain; chains that get no row in a feed; more chains than rows; the lanes rule; each smaller tile.  On
the smaller shapes every cutting, two objects in one process, reads in mid-stream, reset, poison, guard zones and
offset pointers, a stream of the caller's, read_device into a tensor, and the chain DIRECT handle -> resmap -> cov.  One
stream of more than 2^32 rows against a closed form.

The bars against numpy are those of tests/test_cov_host.py, asserted on the device's results; the measured distances
are written to the file that GSDR_COV_MARGINS names, when it is set (profiles/cov_margins.json is the committed copy)."""
import json
import os

import numpy as np
import pytest

from _cov import AXIS_DTYPE, KINDS, Model, axes_of, cuttings, distances, feed_cut, read_all, same_doubles, same_reads, stream
from _extents import OUT_SENTINEL_BITS, check_input_untouched, guarded_input, guarded_output

pytestmark = pytest.mark.gpu

COV_MARGINS = {}
BAR = 1e-12


@pytest.fixture(scope="module")
def cov(gsdr_lib):
    from gpu_sdr_amd import covariance
    yield covariance
    path = os.environ.get("GSDR_COV_MARGINS")
    if COV_MARGINS and path:
        doc = {"metrics": {"cov": "max over cells of |C - numpy.cov| / sqrt(C_ii C_jj): bar 1e-12 with the pivots at the carriers",
                           "corr": "max over cells of |rho - numpy.corrcoef|: bar 1e-12 with the pivots at the carriers"},
               "per_case": dict(sorted(COV_MARGINS.items()))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


T = 128                                                    # the largest tile: asserted against the plan below

# name: (n_ch, n_var, rows, lanes, rows per feed)
SHAPES = {
    "1x1": (1, 1, 1, 1, 1),
    "3x257": (3, 3, 257, 4, 257),
    "T-1 x130": (40, T - 1, 130, 2, 130),                  # a partial tile
    "T x130": (40, T, 130, 2, 130),                        # a full tile
    "T+1 x130": (40, T + 1, 130, 2, 130),                  # the first off-diagonal pair, one variable wide
    "2T+1 x70": (40, 2 * T + 1, 70, 1, 70),                # six pairs, one chain
    "8x40000": (4, 8, 40000, 1024, 100),                   # most chains get no row in a feed
    "2x10": (2, 2, 10, 4096, 10),                          # more chains than rows
    "rule 7x900": (7, 7, 900, 0, 900),
    "rule 300x64": (30, 300, 64, 0, 64),
    "16x130": (16, 16, 130, 2, 130),                       # the tile of 16
    "20x130": (13, 20, 130, 2, 130),                       # the tile of 32
    "40x130": (40, 40, 130, 2, 130),                       # the tile of 64
}
TILES = {"1x1": 16, "3x257": 16, "T-1 x130": T, "T x130": T, "T+1 x130": T, "2T+1 x70": T, "8x40000": 16, "2x10": 16, "rule 7x900": 16,
         "rule 300x64": T, "16x130": 16, "20x130": 32, "40x130": 64}

_memo = {}


def case_of(name):
    """(rows, axes) of a shape, made once and left unchanged: variable i is a quadrature (alternating) of channel
    (11 i + 1) mod n_ch -- no identity list --, the pivots at the carriers; the last channel is the wide-range one."""
    if name not in _memo:
        n_ch, n_var, n, _, _ = SHAPES[name]
        rows, carriers = stream(n, n_ch, seed=7, wide=(n_ch - 1,) if n_ch > 1 else ())
        i = np.arange(n_var)
        ch = (11 * i + 1) % n_ch
        axes = np.zeros(n_var, dtype=AXIS_DTYPE)
        axes["channel"], axes["dx"], axes["dy"] = ch, i % 2 == 0, i % 2 == 1
        axes["pivot"] = np.where(i % 2 == 0, carriers[ch].real, carriers[ch].imag).astype(np.float32)
        _memo[name] = rows, axes
    return _memo[name]


def twin_of(cov, name):
    key = ("twin", name)
    if key not in _memo:
        n_ch, n_var, n, lanes, per = SHAPES[name]
        rows, axes = case_of(name)
        h = cov.host_cov(n_ch, axes, per, lanes=lanes)
        feed_cut(h, rows, cuttings(n, per)["whole"])
        _memo[key] = read_all(h), h.lanes
        h.close()
    return _memo[key]


def to_dev(rows, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows)).to(dev)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_host_twin(cov, cuda_device, name):
    n_ch, n_var, n, lanes, per = SHAPES[name]
    rows, axes = case_of(name)
    want, want_lanes = twin_of(cov, name)
    d = cov.device_cov(n_ch, axes, per, lanes=lanes, device_index=0)
    assert d.lanes == want_lanes and (lanes == 0 or d.lanes == lanes)
    assert cov.feed_plan(n_ch, n_var, d.lanes)["tile"] == TILES[name]
    feed_cut(d, to_dev(rows, cuda_device), cuttings(n, per)["whole"])
    got = read_all(d)
    assert d.rows_seen == n
    d.close()
    assert same_reads(got, want) == ""
    for k in KINDS:
        assert np.array_equal(got[k][0], got[k][0].T, equal_nan=True)
    if n >= 100 and n_ch > 1:
        keep = np.flatnonzero(axes["channel"] != n_ch - 1)        # the Gaussian variables
        c, r = distances(rows, axes, got["cov"][0], got["corr"][0], keep)
        COV_MARGINS[name] = {"cov": c, "corr": r}
        print(name, COV_MARGINS[name])
        assert c <= BAR and r <= BAR


@pytest.mark.parametrize("name", ["3x257", "T+1 x130", "2x10", "20x130"])
def test_every_cutting_and_two_objects_give_the_same_bits(cov, cuda_device, name):
    n_ch, n_var, n, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    want, _ = twin_of(cov, name)
    xd = to_dev(rows, cuda_device)
    for max_rows in (n, 100):
        for cut_name, cut in cuttings(n, max_rows).items():
            a = cov.device_cov(n_ch, axes, max_rows, lanes=lanes, device_index=0)
            b = cov.device_cov(n_ch, axes, max_rows, lanes=lanes, device_index=0) if cut_name == "37" else None
            feed_cut(a, xd, cut)
            if b is not None:
                feed_cut(b, xd, cut)
                assert same_reads(read_all(b), want) == "", (max_rows, cut_name)
                b.close()
            assert same_reads(read_all(a), want) == "", (max_rows, cut_name)
            a.close()


def test_reads_in_mid_stream_reset_and_read_device(cov, cuda_device):
    import torch
    name = "T+1 x130"
    n_ch, n_var, n, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    xd = to_dev(rows, cuda_device)
    d = cov.device_cov(n_ch, axes, n, lanes=lanes, device_index=0)
    h = cov.host_cov(n_ch, axes, n, lanes=lanes)
    out = torch.zeros(n_var * n_var, dtype=torch.float64, device=cuda_device)
    mean = torch.zeros(n_var, dtype=torch.float64, device=cuda_device)
    for a, b in ((0, 33), (33, 34), (34, 100), (100, 130)):
        d.feed(xd[a:b]), h.feed(rows[a:b])
        want = read_all(h)
        assert same_reads(read_all(d), want) == "", b             # any number of reads, the accumulation goes on
        for k in KINDS:
            d.read_device(out, mean, kind=k)
            torch.cuda.synchronize()
            assert same_doubles(out.cpu().numpy().reshape(n_var, n_var), want[k][0]) and same_doubles(mean.cpu().numpy(), want[k][1])
        d.read_device(out, None, kind="cov")                       # the mean is optional
    assert same_reads(read_all(d), twin_of(cov, name)[0]) == ""
    d.reset(), h.reset()
    assert d.rows_seen == 0 and not d.read("sums")[0].any() and np.isnan(d.read("cov")[0]).all()
    d.feed(xd[:77]), h.feed(rows[:77])
    assert same_reads(read_all(d), read_all(h)) == ""
    other = axes.copy()
    other["dx"], other["dy"], other["pivot"] = axes["dy"], axes["dx"], 0.0
    d.reset(other), h.reset(other)
    d.feed(xd), h.feed(rows)
    got = read_all(d)
    assert same_reads(got, read_all(h)) == "" and not same_doubles(got["cov"][0], twin_of(cov, name)[0]["cov"][0])
    d.close(), h.close()


def test_poison_in_one_variable_leaves_every_other_cell_alone(cov, cuda_device):
    name = "T+1 x130"
    n_ch, n_var, n, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    clean, _ = twin_of(cov, name)
    c = 17                                                         # a Gaussian channel: variables 16, 56 and 96 carry it
    hit = np.flatnonzero(axes["channel"] == c)
    assert hit.size >= 2
    bad = rows.copy()
    bad[[0, 5, 64, 129], c] = np.array([np.nan, np.inf, complex(0, -np.inf), complex(3e38, 3e38)], dtype=np.complex64)
    h = cov.host_cov(n_ch, axes, n, lanes=lanes)
    h.feed(bad)
    want = read_all(h)
    h.close()
    d = cov.device_cov(n_ch, axes, n, lanes=lanes, device_index=0)
    d.feed(to_dev(bad, cuda_device))
    got = read_all(d)
    d.close()
    assert same_reads(got, want) == ""
    others = np.setdiff1d(np.arange(n_var), hit)
    for k in KINDS:
        assert got[k][0][np.ix_(others, others)].tobytes() == clean[k][0][np.ix_(others, others)].tobytes()
        assert got[k][1][others].tobytes() == clean[k][1][others].tobytes()
    assert not np.isfinite(got["sums"][1][hit]).any()


@pytest.mark.parametrize("name", ["3x257", "T+1 x130", "40x130"])
def test_guard_zones_and_offset_pointers(cov, gsdr_lib, cuda_device, name):
    """The rows, the matrix and the means in the middle of larger allocations, on a 16-byte boundary and 8 bytes past
    one: a feed reads rows_dev[0, n_rows n_ch) only and leaves it as it was, a read writes out_dev[0, n_var^2) and
    mean_dev[0, n_var) only."""
    import torch
    n_ch, n_var, n, lanes, _ = SHAPES[name]
    rows, axes = case_of(name)
    want, _ = twin_of(cov, name)
    sentinel = np.uint32(OUT_SENTINEL_BITS)
    for off, pattern in ((0, "nan"), (1, "huge")):
        d = cov.device_cov(n_ch, axes, n, lanes=lanes, device_index=0)
        whole_in, view_in = guarded_input(rows.reshape(-1), off, pattern, cuda_device)
        assert gsdr_lib.gsdr_cov_feed_device(d._h, view_in.data_ptr(), n, None) == 0
        whole_out, view_out = guarded_output(n_var * n_var, off, cuda_device)
        whole_mean, view_mean = guarded_output(n_var, off, cuda_device)
        assert gsdr_lib.gsdr_cov_read_device(d._h, 1, view_out.data_ptr(), view_mean.data_ptr(), None) == 0
        torch.cuda.synchronize()
        check_input_untouched(whole_in, rows.reshape(-1), off, pattern)
        for whole, view, count, expect in ((whole_out, view_out, n_var * n_var, want["cov"][0]), (whole_mean, view_mean, n_var, want["cov"][1])):
            bits = whole.cpu().numpy().view(np.uint32)
            first = (view.data_ptr() - whole.data_ptr()) // 8
            assert (bits[:2 * first] == sentinel).all() and (bits[2 * (first + count):] == sentinel).all()
            assert same_doubles(view.cpu().numpy().view(np.float64).reshape(expect.shape), expect)
        # a pointer 4 bytes past a sample is refused, and so is a feed that is too long
        assert gsdr_lib.gsdr_cov_feed_device(d._h, view_in.data_ptr() + 4, 1, None) == -1
        assert gsdr_lib.gsdr_cov_read_device(d._h, 1, view_out.data_ptr() + 4, None, None) == -1
        assert gsdr_lib.gsdr_cov_read_device(d._h, 1, view_out.data_ptr(), view_mean.data_ptr() + 4, None) == -1
        assert gsdr_lib.gsdr_cov_read_device(d._h, 3, view_out.data_ptr(), None, None) == -1
        assert gsdr_lib.gsdr_cov_feed_device(d._h, view_in.data_ptr(), n + 1, None) == -1
        assert gsdr_lib.gsdr_cov_feed_device(d._h, None, 1, None) == -1 and gsdr_lib.gsdr_cov_feed_device(d._h, None, 0, None) == 0
        assert gsdr_lib.gsdr_cov_feed_host(d._h, rows.ctypes.data, 1) == -1 and gsdr_lib.gsdr_cov_read_host(d._h, 1, rows.ctypes.data, None) == -1
        assert d.rows_seen == n and same_reads(read_all(d), want) == ""
        d.close()


def test_a_stream_of_the_callers(cov, cuda_device):
    """Feeds, a read on the device, more feeds, all on one side stream with no wait in between; then the reads that return
    to the host, which wait for that stream."""
    import torch
    name = "8x40000"
    n_ch, n_var, n, lanes, per = SHAPES[name]
    rows, axes = case_of(name)
    want, _ = twin_of(cov, name)
    xd = to_dev(rows, cuda_device)
    half = torch.zeros(n_var * n_var, dtype=torch.float64, device=cuda_device)
    d = cov.device_cov(n_ch, axes, per, lanes=lanes, device_index=0)
    torch.cuda.synchronize()
    stream_ = torch.cuda.Stream()
    for at in range(0, n, per):
        d.feed_device(xd[at:at + per], stream=stream_)
        if at + per == n // 2:
            d.read_device(half, kind="corr", stream=stream_)
    got = read_all(d, stream=stream_)
    d.close()
    assert same_reads(got, want) == ""
    h = cov.host_cov(n_ch, axes, n, lanes=lanes)
    h.feed(rows[:n // 2])
    assert same_doubles(half.cpu().numpy().reshape(n_var, n_var), h.read("corr")[0])
    h.close()


def test_handle_resmap_cov_chain(cov, cuda_device):
    """DIRECT, 8 tones, decim 50, buffer 50 000: 1000 rows per buffer.  The handle's output goes through a resmap object
    (5 tones, X_DQR) into a cov object over both quadratures of the five mapped channels, all on one stream, three buffers;
    the twin fed the same mapped rows gives the same bits."""
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
    m = resmap.device_resmap(n_ch, max_rows, resmap.resmap_constants(fits, tones), channels=channels, kind="x_dqr", device_index=0)
    axes = g.cov_axes(range(len(channels)), "both")
    d = g.device_cov(len(channels), axes, max_rows, device_index=0)
    twin = g.host_cov(len(channels), axes, max_rows)
    assert d.lanes == twin.lanes and d.n_var == 10
    ampl, phase = np.full(n_ch, 0.1, dtype=np.float32), np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream_ = torch.cuda.Stream()
    kept = []
    for b in range(3):
        xin = torch.from_numpy(host_tones(L, b * L, rate, freq, ampl, phase, sigma=2e-2, seed=40 + b)).to(cuda_device)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        y = torch.empty((max_rows, len(channels)), dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        n = dem.process_device(xin, out, stream=stream_)
        assert n > 0 and n % n_ch == 0 and m.feed_device(out[:n], y, stream=stream_) == n // n_ch
        d.feed_device(y[:n // n_ch], stream=stream_)
        kept.append((y[:n // n_ch], out))
    got = read_all(d, stream=stream_)                              # waits for the stream
    for y, _ in kept:
        twin.feed(y.cpu().numpy())
    assert d.rows_seen == twin.rows_seen == 3000
    assert same_reads(got, read_all(twin)) == ""
    assert np.isfinite(got["cov"][0]).all() and (np.diagonal(got["corr"][0]) == 1.0).all()
    d.close(), twin.close(), m.close(), dem.close()


# ---- more rows than 2^32 -------------------------------------------------------------------------------------------------------
# Two variables on pivot-0 axes (the real parts of two channels), lanes 1024.  A prefix of T0 = 4100 (2^20 - 1) rows of
# 0 + 0j -- each adds exactly +0 by fma(0, 0, G) and S + 0 --, then 3 001 wide rows in three pieces that begin at stream
# positions which are no multiple of lanes.  Neither the twin nor the Model can take 4.3 10^9 rows: the expected result is
# the Model of T0 mod lanes such rows plus the tail, read with the n of the whole stream.
BIG_K, BIG_PER, BIG_LANES = 4100, (1 << 20) - 1, 1024
BIG_T0 = BIG_K * BIG_PER
BIG_TAIL = (7, 2001, 993)


def test_more_than_2_32_rows_against_the_closed_form(cov, cuda_device):
    import torch
    tail, _ = stream(sum(BIG_TAIL), 2, seed=11, wide=(0, 1))
    axes = axes_of([0, 1], "re")
    z = BIG_T0 % BIG_LANES
    assert BIG_T0 > 1 << 32 and z == 1020
    m = Model(np.concatenate([np.zeros((z, 2), dtype=np.complex64), tail]), axes, BIG_LANES)
    m.n = BIG_T0 + tail.shape[0]                                   # the n of the reads
    zeros = torch.zeros((BIG_PER, 2), dtype=torch.complex64, device=cuda_device)
    d = cov.device_cov(2, axes, BIG_PER, lanes=BIG_LANES, device_index=0)
    for feeds in range(1, BIG_K + 1):
        d.feed(zeros)
        if feeds == 2049:                                          # past 2^31 rows
            assert d.rows_seen == feeds * BIG_PER > 1 << 31
            assert not d.read("sums")[0].any() and not d.read("cov")[0].any()
    assert d.rows_seen == BIG_T0
    feed_cut(d, to_dev(tail, cuda_device), BIG_TAIL)
    got = read_all(d)
    assert d.rows_seen == BIG_T0 + tail.shape[0] > 1 << 32
    d.close()
    assert same_reads(got, {k: m.read(k) for k in KINDS}) == ""
