"""The channel covariance without a GPU (include/gsdr.h, "channel covariance on the device"): the library's host twin
(GSDR_COV_HOST) against the bit model of tests/_cov.py, bit for bit, for all three reads, a wide-range variable
included; every cutting of the stream; poison; n = 0 and n = 1, a constant variable, reset; every refusal with its words;
the launch rule and the lanes rule; and the twin against numpy.cov and numpy.corrcoef.

The bar against numpy.  With the pivots at the carriers, |C - numpy.cov| <= 1e-12 sqrt(C_ii C_jj) and
|rho - numpy.corrcoef| <= 1e-12 (the same quantity: rho is C over that root).  A numpy emulation of the law with separate
multiply and add gives 1.7e-16 - 7.6e-16 on such streams (4 000 x 6 with lanes 4, 257 x 5 with lanes 8, 100 000 x 8 with
lanes 64): the bar leaves three decades.  With the pivots at 0 the sum form loses n 2^-53 |mean|^2 / var -- the
emulation gives 2e-10 - 7e-9 --: that case is recorded, not barred.  The measured distances are written to the file
that GSDR_COV_MARGINS names, when it is set; profiles/cov_margins.json is the committed copy."""
import json
import os

import numpy as np
import pytest

from _cov import AXIS_DTYPE, KINDS, Model, axes_of, cuttings, distances, feed_cut, read_all, same_doubles, same_reads, stream

COV_MARGINS = {}
BAR = 1e-12


@pytest.fixture(scope="module")
def cov(gsdr_lib):
    from gpu_sdr_amd import covariance
    yield covariance
    path = os.environ.get("GSDR_COV_MARGINS")
    if COV_MARGINS and path:
        doc = {"metrics": {"cov": "max over cells of |C - numpy.cov| / sqrt(C_ii C_jj): bar 1e-12 with the pivots at the carriers",
                           "corr": "max over cells of |rho - numpy.corrcoef|: bar 1e-12 with the pivots at the carriers",
                           "*_pivot0": "the same with the pivots at 0: recorded, not barred"},
               "per_case": dict(sorted(COV_MARGINS.items()))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


_memo = {}


def case(n, n_ch, seed, wide=()):
    key = (n, n_ch, seed, tuple(wide))
    if key not in _memo:
        _memo[key] = stream(n, n_ch, seed=seed, wide=wide)
    return _memo[key]


def run_twin(cov, rows, axes, lanes, cut, max_rows):
    h = cov.host_cov(rows.shape[1], axes, max_rows, lanes=lanes)
    feed_cut(h, rows, cut)
    assert h.rows_seen == rows.shape[0]
    got, got_lanes = read_all(h), h.lanes
    h.close()
    return got, got_lanes


def model_reads(rows, axes, lanes):
    m = Model(rows, axes, lanes)
    return {k: m.read(k) for k in KINDS}


# name: (n_ch, rows, lanes, the axes from (carriers, n_ch))
TWIN_SHAPES = {
    "1x1": (1, 1, 1, lambda c, n: axes_of([0], "re", c)),
    "3x257": (3, 257, 4, lambda c, n: axes_of(range(n), "re", c)),
    "5x300": (5, 300, 8, lambda c, n: axes_of(range(n), "im", c)),
    "repeated channel, both quadratures": (4, 120, 2, lambda c, n: axes_of([2, 0, 2, 3], "both", c)),
    "lanes larger than the rows": (2, 10, 64, lambda c, n: axes_of([1, 0], "both", c)),
}


@pytest.mark.parametrize("name", list(TWIN_SHAPES))
def test_twin_equals_the_model_bit_for_bit(cov, name):
    n_ch, n, lanes, make = TWIN_SHAPES[name]
    rows, carriers = case(n, n_ch, 5, wide=(n_ch - 1,))
    axes = make(carriers, n_ch)
    got, got_lanes = run_twin(cov, rows, axes, lanes, [n], n)
    assert got_lanes == lanes
    assert same_reads(got, model_reads(rows, axes, lanes)) == ""
    for k in KINDS:
        assert np.array_equal(got[k][0], got[k][0].T, equal_nan=True)


def test_the_wide_variable_sees_the_order_of_the_additions(cov):
    """What makes the bit tests mean something: on the wide variable lanes 8, 4 and 1 give different sums, in the model
    and, bit for bit the same ones, in the twin."""
    rows, carriers = case(300, 3, 5, wide=(2,))
    axes = axes_of([2], "re", carriers)
    cells = [Model(rows, axes, lanes).read("sums") for lanes in (8, 4, 1)]
    for lanes, want in zip((8, 4, 1), cells):
        got, _ = run_twin(cov, rows, axes, lanes, [300], 300)
        assert same_doubles(got["sums"][0], want[0]) and same_doubles(got["sums"][1], want[1])
    assert len({float(c[0][0, 0]).hex() for c in cells}) == 3 and len({float(c[1][0]).hex() for c in cells}) >= 2


@pytest.mark.parametrize("n,n_ch,lanes,max_rows", [(257, 3, 4, 257), (500, 5, 64, 100), (2000, 2, 16, 1200)])
def test_every_cutting_gives_the_same_bits(cov, n, n_ch, lanes, max_rows):
    rows, carriers = case(n, n_ch, 9, wide=(0,))
    axes = axes_of(range(n_ch), "both", carriers)
    want = None
    for name, cut in cuttings(n, max_rows).items():
        got, _ = run_twin(cov, rows, axes, lanes, cut, max_rows)
        blob = tuple(np.asarray(a).tobytes() for k in KINDS for a in got[k])
        want = want or blob
        assert blob == want, name


def test_poison_in_one_variable_changes_only_its_row_column_and_sum(cov):
    n_ch, n, lanes = 4, 257, 4
    rows, carriers = case(n, n_ch, 11)
    axes = axes_of([0, 1, 2, 3, 1], "re", carriers)                # variables 1 and 4 are both channel 1
    clean, _ = run_twin(cov, rows, axes, lanes, [n], n)
    bad = rows.copy()
    bad[[0, 100, 256], 2] = np.array([np.inf, complex(np.nan, 0), 3e38], dtype=np.complex64)
    got, _ = run_twin(cov, bad, axes, lanes, [n], n)
    assert same_reads(got, model_reads(bad, axes, lanes)) == ""
    others = np.array([0, 1, 3, 4])
    for k in KINDS:
        assert got[k][0][np.ix_(others, others)].tobytes() == clean[k][0][np.ix_(others, others)].tobytes()
        assert got[k][1][others].tobytes() == clean[k][1][others].tobytes()
        assert not np.isfinite(got[k][0][2, 2]) or k == "corr"
    assert np.isnan(got["sums"][0][2]).all() and np.isnan(got["sums"][1][2]) and np.isnan(got["corr"][0][2]).all()


def test_n_0_n_1_a_constant_variable_and_reset(cov):
    rows, carriers = case(50, 2, 13)
    rows = rows.copy()
    rows[:, 1] = 0.75                                              # a constant variable: d = 0.5, every sum exact
    axes = axes_of([0, 1], "re", carriers)
    axes["pivot"][1] = 0.25
    h = cov.host_cov(2, axes, 64, lanes=4)
    got = read_all(h)
    assert not got["sums"][0].any() and not got["sums"][1].any()
    for k in ("cov", "corr"):
        assert np.isnan(got[k][0]).all() and np.isnan(got[k][1]).all()
    h.feed(rows[:1])
    got = read_all(h)
    assert np.isnan(got["cov"][0]).all() and np.isnan(got["corr"][0]).all()
    assert same_doubles(got["cov"][1], axes["pivot"] + (rows[0].real.astype(np.float64) - axes["pivot"]))
    assert same_reads(got, model_reads(rows[:1], axes, 4)) == ""
    h.feed(rows[1:])
    got = read_all(h)
    assert same_reads(got, model_reads(rows, axes, 4)) == ""
    assert got["cov"][0][1, 1] == 0.0 and got["cov"][0][0, 0] > 0
    assert got["corr"][0][0, 0] == 1.0 and np.isnan(got["corr"][0][1, 1]) and not np.isfinite(got["corr"][0][0, 1])
    h.reset()
    assert h.rows_seen == 0 and not read_all(h)["sums"][0].any()
    h.feed(rows)
    assert same_reads(read_all(h), got) == ""
    other = axes_of([1, 0], "im", carriers)
    h.reset(other)
    assert h.rows_seen == 0 and np.array_equal(h.axes, other)
    h.feed(rows)
    assert same_reads(read_all(h), model_reads(rows, other, 4)) == ""
    h.close()


def test_every_refusal(cov, gsdr_lib):
    from gpu_sdr_amd import GsdrError
    L = gsdr_lib
    ax = axes_of([0, 1], "re")
    p = ax.ctypes.data

    def err():
        return L.gsdr_last_error(None).decode()
    for args, words in (((0, 2, 8, 1, p, -2), "n_ch must be in [1, 1048576]"), (((1 << 20) + 1, 2, 8, 1, p, -2), "n_ch must be in [1, 1048576]"),
                        ((2, 0, 8, 1, p, -2), "n_var must be in [1, 4096]"), ((2, 4097, 8, 1, p, -2), "n_var must be in [1, 4096]"),
                        ((2, 2, 0, 1, p, -2), "max_rows must be in [1, 1048576]"), ((2, 2, (1 << 20) + 1, 1, p, -2), "max_rows must be in [1, 1048576]"),
                        ((2, 2, 8, 3, p, -2), "lanes must be 0 or a power of two in [1, 4096]"),
                        ((2, 2, 8, 8192, p, -2), "lanes must be 0 or a power of two in [1, 4096]"),
                        ((2, 2, 8, -1, p, -2), "lanes must be 0 or a power of two in [1, 4096]"),
                        ((2, 4096, 8, 64, p, -2), "lanes and n_var: lanes x n_var (n_var + 1) / 2 must be at most 268435456 cells"),
                        ((2, 2, 8, 1, None, -2), "axes must not be NULL"), ((2, 2, 8, 1, p, -3), "device_index must be >= -1 or GSDR_COV_HOST")):
        assert not L.gsdr_cov_create(*args), args
        assert err() == "gsdr_cov_create: " + words, (args, err())
    for field, value, words in (("channel", 2, "axes: channel must be in [0, n_ch) (variable 1)"), ("channel", -1, "axes: channel must be in [0, n_ch) (variable 1)"),
                                ("reserved", 1, "axes: reserved must be 0 (variable 1)"), ("bx", np.nan, "axes: every field must be finite (variable 1)"),
                                ("by", np.inf, "axes: every field must be finite (variable 1)"), ("dx", -np.inf, "axes: every field must be finite (variable 1)"),
                                ("dy", np.nan, "axes: every field must be finite (variable 1)"), ("pivot", np.nan, "axes: every field must be finite (variable 1)")):
        bad = ax.copy()
        bad[field][1] = value
        assert not L.gsdr_cov_create(2, 2, 8, 1, bad.ctypes.data, -2) and err() == "gsdr_cov_create: " + words, (field, err())
    with pytest.raises(ValueError, match="host_cov"):
        cov.device_cov(2, ax, 8, device_index=-2)
    h = cov.host_cov(2, ax, 8, lanes=2)
    rows = np.ones((9, 2), dtype=np.complex64)
    h.feed(rows[:5])
    before = read_all(h)
    with pytest.raises(GsdrError, match=r"gsdr_cov_feed_host: n_rows must be in \[0, max_rows\]"):
        h.feed(rows)
    assert L.gsdr_cov_feed_host(h._h, rows.ctypes.data, -1) == -1 and err() == "gsdr_cov_feed_host: n_rows must be in [0, max_rows]"
    assert L.gsdr_cov_feed_host(h._h, None, 1) == -1 and err() == "gsdr_cov_feed_host: null buffer: rows"
    assert L.gsdr_cov_feed_host(h._h, None, 0) == 0
    out = np.zeros(4)
    for kind in (-1, 3):
        assert L.gsdr_cov_read_host(h._h, kind, out.ctypes.data, None) == -1
        assert err() == "gsdr_cov_read_host: kind must be GSDR_COV_SUMS, GSDR_COV_COV or GSDR_COV_CORR"
    assert L.gsdr_cov_read_host(h._h, 1, None, None) == -1 and err() == "gsdr_cov_read_host: null buffer: out"
    assert L.gsdr_cov_read_host(h._h, 1, out.ctypes.data, None) == 0                  # the mean is optional
    assert L.gsdr_cov_feed_device(h._h, rows.ctypes.data, 1, None) == -1 and "GSDR_COV_HOST" in err()
    assert L.gsdr_cov_read(h._h, 1, out.ctypes.data, None, None) == -1 and L.gsdr_cov_read_device(h._h, 1, out.ctypes.data, None, None) == -1
    bad = ax.copy()
    bad["channel"][0] = 5
    with pytest.raises(GsdrError, match=r"gsdr_cov_reset: axes: channel must be in \[0, n_ch\) \(variable 0\)"):
        h.reset(bad)
    with pytest.raises(ValueError):
        h.reset(ax[:1])
    assert np.array_equal(h.axes, ax) and h.rows_seen == 5 and same_reads(read_all(h), before) == ""
    h.close()
    assert L.gsdr_cov_reset(None, None) == -1 and err() == "gsdr_cov_reset: null object"
    assert L.gsdr_cov_feed_host(None, None, 0) == -1 and L.gsdr_cov_read_host(None, 1, out.ctypes.data, None) == -1
    assert L.gsdr_cov_rows(None) == 0 and L.gsdr_cov_lanes(None) == 0 and L.gsdr_cov_n_var(None) == 0
    L.gsdr_cov_close(None)


def test_plan_at_the_launch_rules_edges(cov):
    def plan(n_var, lanes=1):
        return cov.feed_plan(4, n_var, lanes)
    for n_var, tile, tiles in ((1, 16, 1), (16, 16, 1), (17, 32, 1), (32, 32, 1), (33, 64, 1), (64, 64, 1), (65, 128, 1), (128, 128, 1),
                               (129, 128, 2), (256, 128, 2), (257, 128, 3), (2048, 128, 16), (4096, 128, 32)):
        p = plan(n_var)
        assert (p["tile"], p["tiles"], p["pairs"], p["lds_bytes"]) == (tile, tiles, tiles * (tiles + 1) // 2, 256 * tile), n_var
        assert p["project_x"] == min(256, 1 << max(0, (n_var - 1).bit_length()))
    assert plan(2048, 4)["lanes"] == 4 and plan(8, 4096)["lanes"] == 4096
    for args in ((0, 8, 1), (4, 0, 1), (4, 4097, 1), (4, 8, 0), (4, 8, 3), (4, 8, 8192), (4, 4096, 32), ((1 << 20) + 1, 8, 1)):
        with pytest.raises(ValueError):
            cov.feed_plan(*args)
    assert cov.feed_plan(1 << 20, 4096, 16)["pairs"] == 528       # 32 x 4096 x 4097 / 2 cells are 65 536 too many


def test_the_lanes_rule(cov):
    """The smallest power of two with pairs x lanes >= 512 x 128 / tile, at most the largest power of two <= max_rows, at
    most 4096, and within 2^28 cells."""
    for n_var, max_rows, lanes in ((2048, 1000, 4), (8, 1 << 20, 4096), (256, 10000, 256), (4096, 1 << 20, 1), (8, 100, 64), (8, 1, 1),
                                   (3, 257, 256), (129, 1 << 20, 256), (1, 1 << 20, 4096), (3000, 1 << 20, 2), (20, 1 << 20, 2048),
                                   (64, 1 << 20, 1024), (40, 600, 512), (128, 1 << 20, 512)):
        ax = axes_of(np.zeros(n_var, dtype=np.int32), "re")
        h = cov.host_cov(1, ax, max_rows)
        assert h.lanes == lanes, (n_var, max_rows, h.lanes)
        h.close()


NUMPY_SHAPES = {"4000x6 lanes 4": (4000, 6, 4), "257x5 lanes 8": (257, 5, 8), "100000x8 lanes 64": (100000, 8, 64)}


@pytest.mark.parametrize("name", list(NUMPY_SHAPES))
def test_twin_against_numpy(cov, name):
    n, n_ch, lanes = NUMPY_SHAPES[name]
    rows, carriers = case(n, n_ch, 21)
    margins = {}
    for tag, c in (("", carriers), ("_pivot0", None)):
        axes = axes_of(range(n_ch), "re", c)
        h = cov.host_cov(n_ch, axes, n, lanes=lanes)
        h.feed(rows)
        (C, mean), (R, _) = h.read("cov"), h.read("corr")
        h.close()
        margins["cov" + tag], margins["corr" + tag] = distances(rows, axes, C, R, np.arange(n_ch))
        off = R[~np.eye(n_ch, dtype=bool)]
        assert (np.diagonal(R) == 1.0).all() and (off > 0.3).all() and (off < 0.7).all()
        assert np.abs(mean - rows.real.astype(np.float64).mean(axis=0)).max() <= 1e-12
    COV_MARGINS["twin " + name] = margins
    print(name, margins)
    assert margins["cov"] <= BAR and margins["corr"] <= BAR, margins
