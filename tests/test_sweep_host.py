"""The sweep accumulator's host twin (gsdr_sweep_* with GSDR_SWEEP_HOST, sweep_host.cpp) against the model of
tests/_sweep.py, bit for bit: means, variances and the phase slope for every shape under every cutting and first_row;
partial sweeps; the counts against enumeration; poison; every refusal; sweep_shape against gsdr_chirp_derive; vna_axis
against numpy.linspace; the line delay of a noiseless cable and the variance against numpy.var.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from _sweep import (FIRST_ROWS, SHAPES, counts_by_enumeration, counts_closed, cuttings, model, rows_of, run_host, same_bits, same_result,
                    total_for)


@pytest.fixture(scope="module")
def sweep(gsdr_lib):
    from gpu_sdr_amd import sweep
    return sweep


@pytest.mark.parametrize("first_row", FIRST_ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_twin_equals_model_under_every_cutting(sweep, shape, first_row):
    n_ch, n_points, group = shape
    total = total_for(n_points, group)
    x = rows_of(total, n_ch)
    want = model(x, n_points, group, first_row)
    assert np.array_equal(want[3], counts_by_enumeration(first_row, total, n_points, group))
    assert want[3].min() >= 2 * group and (want[3].max() > want[3].min() or n_points == 1)
    for name, cut in cuttings(total, n_points * group).items():
        got = run_host(sweep, x, n_points, group, first_row, cut)
        assert same_result(got, want), (name, [same_bits(g, w) for g, w in zip(got[:3], want[:3])])
        assert np.array_equal(got[3], want[3]) and got[4] == want[3].min() // group == 2, name
    assert np.all(np.isfinite(want[0].view(np.float32))) and np.all(want[1].view(np.float32) > 0)


@pytest.mark.parametrize("first_row", FIRST_ROWS)
@pytest.mark.parametrize("shape,total", [((3, 67, 1), 40), ((1, 7, 3), 10), ((2, 250, 40), 40 * 3 + 1), ((16, 1000, 1), 1001), ((1, 5, 1), 0)])
def test_partial_sweeps(sweep, shape, total, first_row):
    """Less than one pass, or just over one: points with no row ((+0, +0) in mean and variance), with one row (the row
    itself, variance +0) and with unequal counts."""
    n_ch, n_points, group = shape
    x = rows_of(max(total, 1), n_ch, seed=9)[:total]
    want = model(x, n_points, group, first_row)
    n = want[3]
    assert np.array_equal(n, counts_by_enumeration(first_row, total, n_points, group))
    assert (n == 0).any() or (n == 1).any()
    got = run_host(sweep, x, n_points, group, first_row, None if total else [0, 0])
    assert same_result(got, want) and np.array_equal(got[3], n) and got[4] == n.min() // group
    zero = np.zeros(n_ch, dtype=np.complex64)
    for p in np.flatnonzero(n == 0):
        assert same_bits(got[0][p], zero) and same_bits(got[1][p], zero)
    p_of = [((first_row + i) // group) % n_points for i in range(total)]
    for p in np.flatnonzero(n == 1):
        assert same_bits(got[0][p], x[p_of.index(p)]) and same_bits(got[1][p], zero)


@pytest.mark.parametrize("n_points,group", [(1, 1), (1, 5), (5, 1), (7, 3), (67, 1), (4, 64), (250, 40)])
def test_counts_and_sweeps_against_enumeration(sweep, gsdr_lib, n_points, group):
    W = n_points * group
    for first_row in (0, 1, group - 1, group, W - 1, W + 2, 3 * W + group + 1, (1 << 40) + 17, 1 << 62):
        s = sweep.host_sweep(1, n_points, group, first_row)
        total = 0
        for n in (0, 1, group, 1, W - group - 2 if W > group + 2 else 0, 3, W, 2 * W + 5):
            s.feed(np.zeros((n, 1), dtype=np.complex64))
            total += n
            want = counts_by_enumeration(first_row, total, n_points, group)
            assert np.array_equal(s.counts(), want), (first_row, total)
            assert np.array_equal(counts_closed(first_row, total, n_points, group), want)
            assert [s.point_rows(p) for p in range(n_points)] == want.tolist()
            assert s.sweeps == want.min() // group and s.rows_seen == total
        assert s.point_rows(-1) == 0 and s.point_rows(n_points) == 0
        again = (first_row + 5) % (1 << 62)
        s.reset(again)
        assert s.rows_seen == 0 and s.sweeps == 0 and not s.counts().any()
        s.feed(np.zeros((W + 1, 1), dtype=np.complex64))
        assert np.array_equal(s.counts(), counts_by_enumeration(again, W + 1, n_points, group))
        s.close()


def test_reset_and_reads_do_not_disturb(sweep):
    n_ch, n_points, group = 3, 67, 1
    x = rows_of(total_for(n_points, group), n_ch, seed=12)
    want = model(x, n_points, group, 3)
    s = sweep.host_sweep(n_ch, n_points, group, 99)
    s.feed(rows_of(50, n_ch, seed=13))
    s.reset(3)
    for at in range(0, x.shape[0], 30):
        s.feed(x[at:at + 30])
        s.read(variance=True), s.slope()                 # any number of reads
    got = s.read(variance=True) + (s.slope(),)
    s.close()
    assert same_result(got, want)


def test_poison_reaches_exactly_its_accumulators(sweep):
    for n_ch, n_points, group in ((3, 67, 1), (2, 25, 4)):
        total = total_for(n_points, group)
        x = rows_of(total, n_ch, seed=21)
        clean = run_host(sweep, x, n_points, group, 3)
        bad = x.copy()
        r_inf, r_nan = total // 3, total // 2
        bad[r_inf, 1] = np.complex64(complex(np.inf, 0.0))
        bad[r_nan, 0] = np.complex64(complex(0.0, np.nan))
        p_inf, p_nan = ((3 + r_inf) // group) % n_points, ((3 + r_nan) // group) % n_points
        assert p_inf != p_nan
        for cut in (None, cuttings(total, n_points * group)["sevens"]):
            got = run_host(sweep, bad, n_points, group, 3, cut)
            assert same_result(got, model(bad, n_points, group, 3))
            hit = np.zeros((n_points, n_ch), dtype=bool)
            hit[p_inf, 1] = hit[p_nan, 0] = True
            for k in (0, 1):
                assert same_bits(got[k][~hit], clean[k][~hit])
            assert not np.isfinite(got[0][p_inf, 1].real) and np.isfinite(got[0][p_inf, 1].imag)
            assert np.isnan(got[0][p_nan, 0].imag) and np.isfinite(got[0][p_nan, 0].real)
            assert np.isnan(got[1][p_inf, 1].real) and np.isnan(got[1][p_nan, 0].imag)          # NaN stays NaN
            # the slope: the poisoned channels are not finite, the others keep their bits
            assert not np.isfinite(got[2][0]) and not np.isfinite(got[2][1])
            assert all(same_bits(got[2][c], clean[2][c]) for c in range(2, n_ch))


def test_create_refusals(sweep, gsdr_lib):
    from gpu_sdr_amd import GsdrError
    bad = [((0, 5, 1, 0), "n_ch"), (((1 << 20) + 1, 5, 1, 0), "n_ch"), ((1, 0, 1, 0), "n_points"), ((1, (1 << 24) + 1, 1, 0), "n_points"),
           ((3, 1 << 24, 1, 0), r"n_points \* n_ch"), ((1, 5, 0, 0), "group"), ((1, 5, (1 << 30) + 1, 0), "group"),
           ((1, 5, 1, -1), "first_row"), ((1, 5, 1, (1 << 62) + 1), "first_row")]
    for args, word in bad:
        for device in (-2, 0):                           # refused before the device is touched: the same on a machine with no GPU
            assert not gsdr_lib.gsdr_sweep_create(*args, device)
            msg = gsdr_lib.gsdr_last_error(None).decode()
            assert msg.startswith("gsdr_sweep_create: ") and word.replace("\\", "") in msg, (args, msg)
        with pytest.raises(GsdrError, match="gsdr_sweep_create: .*" + word):
            sweep.host_sweep(*args)
    assert not gsdr_lib.gsdr_sweep_create(1, 5, 1, 0, -3)
    assert "device_index" in gsdr_lib.gsdr_last_error(None).decode()
    with pytest.raises(ValueError):
        sweep.device_sweep(1, 5, 1, 0, device_index=-2)
    s = sweep.host_sweep(1 << 20, 1, 1 << 30, 1 << 62)    # the bounds themselves are accepted
    assert s.sweeps == 0
    s.close()


def test_feed_and_null_object_refusals(sweep, gsdr_lib):
    s = sweep.host_sweep(2, 5, 1, 0)
    x = rows_of(8, 2)
    s.feed(x[:3])
    err = lambda: gsdr_lib.gsdr_last_error(None).decode()
    for n in (-1, (1 << 24) + 1):
        assert gsdr_lib.gsdr_sweep_feed_host(s._h, x.ctypes.data, n) == -1 and "gsdr_sweep_feed_host: n_rows" in err()
    assert gsdr_lib.gsdr_sweep_feed_host(s._h, None, 2) == -1 and "null buffer: rows" in err()
    assert gsdr_lib.gsdr_sweep_feed_host(s._h, None, 0) == 0
    assert gsdr_lib.gsdr_sweep_read_host(s._h, None, None) == -1 and "null buffer: mean" in err()
    assert gsdr_lib.gsdr_sweep_slope(s._h, None, None) == -1 and "null buffer: d_host" in err()
    assert gsdr_lib.gsdr_sweep_reset(s._h, -1) == -1 and "first_row" in err()
    # the device entries are refused on a host object
    m = np.zeros((5, 2), dtype=np.complex64)
    assert gsdr_lib.gsdr_sweep_feed_device(s._h, x.ctypes.data, 1, None) == -1 and "host object" in err()
    assert gsdr_lib.gsdr_sweep_read_device(s._h, m.ctypes.data, None, None) == -1 and "host object" in err()
    assert gsdr_lib.gsdr_sweep_read(s._h, m.ctypes.data, None, None) == -1 and "host object" in err()
    assert s.rows_seen == 3                               # state unchanged
    s.feed(x[3:])
    assert same_result(s.read(variance=True) + (s.slope(),), model(x, 5, 1, 0))
    s.close()
    gsdr_lib.gsdr_sweep_close(None)
    assert gsdr_lib.gsdr_sweep_rows(None) == 0 and gsdr_lib.gsdr_sweep_sweeps(None) == 0 and gsdr_lib.gsdr_sweep_point_rows(None, 0) == 0
    d = np.zeros(2)
    for call, name in ((lambda: gsdr_lib.gsdr_sweep_feed_host(None, None, 0), "feed_host"), (lambda: gsdr_lib.gsdr_sweep_feed_device(None, None, 0, None), "feed_device"),
                       (lambda: gsdr_lib.gsdr_sweep_read_host(None, m.ctypes.data, None), "read_host"), (lambda: gsdr_lib.gsdr_sweep_read(None, m.ctypes.data, None, None), "read"),
                       (lambda: gsdr_lib.gsdr_sweep_read_device(None, m.ctypes.data, None, None), "read_device"),
                       (lambda: gsdr_lib.gsdr_sweep_slope(None, d.ctypes.data, None), "slope"), (lambda: gsdr_lib.gsdr_sweep_reset(None, 0), "reset")):
        assert call() == -1 and err() == f"gsdr_sweep_{name}: null object", name


def test_sweep_shape_against_chirp_derive(sweep, gsdr_lib):
    import gpu_sdr_amd as g
    from gpu_sdr_amd import GsdrError
    rate = 200_000_000
    for chirp_t, swipe_s, length in ((1.0, 1_000_000, 200), (1.5, 1_000_000, 300), (3.5e-5, 1000, 7), (3e-3, 1000, 600)):      # the first is C4
        cp = g.chirp_derive(rate, -rate // 2, rate // 2, swipe_s, chirp_t)
        assert (cp.num_steps, cp.length) == (swipe_s, length)
        period = cp.num_steps * cp.length
        assert sweep.sweep_shape(rate, -rate // 2, rate // 2, swipe_s, chirp_t, 0) == (swipe_s, length)
        for decim in (1, 4, 3, 7):
            ppt = length * decim
            if period % ppt == 0:
                assert sweep.sweep_shape(rate, -rate // 2, rate // 2, swipe_s, chirp_t, decim) == (period // ppt, 1)
            else:
                with pytest.raises(GsdrError, match="gsdr_sweep_shape_for_chirp: decim.*does not divide"):
                    sweep.sweep_shape(rate, -rate // 2, rate // 2, swipe_s, chirp_t, decim)
    # decim 1 and 4 divide both 10^6-step periods; 3 does not divide C4's and 7 neither
    assert sweep.sweep_shape(rate, 0, 1000, 1_000_000, 1.0, 4) == (250_000, 1) and sweep.sweep_shape(rate, 0, 1000, 1_000_000, 1.5, 4) == (250_000, 1)
    for decim in (3, 7):
        with pytest.raises(GsdrError):
            sweep.sweep_shape(rate, 0, 1000, 1_000_000, 1.0, decim)
    with pytest.raises(GsdrError, match="decim"):
        sweep.sweep_shape(rate, 0, 1000, 1000, 3.5e-5, -1)
    n, grp = C.c_longlong(0), C.c_longlong(0)
    assert gsdr_lib.gsdr_sweep_shape_for_chirp(None, 1, C.byref(n), C.byref(grp)) == -1


def numpy_axis(rate, freq0, chirp_f, swipe_s, n_points, rf):
    """VNA_analysis, pyUSRP/USRP_VNA.py:738-759"""
    df = int((2.0**32 - 1) * (chirp_f - freq0) / (swipe_s - 1.) / float(rate))
    df = df * (swipe_s - 1.) * float(rate) / (2.0**32 - 1)
    stop = df + freq0
    return np.linspace(freq0, stop, n_points, dtype=np.float64) + rf, stop


@pytest.mark.parametrize("rate,freq0,chirp_f,swipe_s,n_points,rf", [
    (200_000_000, -90_000_000, 90_000_000, 1_000_000, 1_000_000, 300e6), (200_000_000, 50_000_000, -50_000_000, 1000, 250, 1.2e9),
    (100_000_000, -1_234_567, 7_654_321, 10_000, 2500, 0.0), (10_000_000, 4_000_000, -3_999_999, 50, 25, 75e6), (1_000_000, 10, 499_999, 7, 7, 1e9),
    (200_000_000, 0, 1000, 1000, 1, 5.0)])
def test_vna_axis_against_numpy(sweep, rate, freq0, chirp_f, swipe_s, n_points, rf):
    want, stop = numpy_axis(rate, freq0, chirp_f, swipe_s, n_points, rf)
    assert stop != chirp_f and abs(stop - chirp_f) < abs(chirp_f - freq0) * 1e-3 + rate / 2.0**32 * swipe_s
    assert (stop < freq0) == (chirp_f < freq0)
    f = sweep.vna_axis(rate, freq0, chirp_f, swipe_s, n_points, rf)
    assert f.shape == (n_points,) and f[0] == rf + freq0 and (n_points == 1 or f[-1] == rf + stop)      # the ends are exact
    assert np.all(np.abs(f - want) <= np.spacing(np.abs(want)))                                      # within one ulp of numpy's
    assert np.all(np.diff(f) > 0) if chirp_f > freq0 else np.all(np.diff(f) < 0)


def test_vna_axis_refusals(sweep):
    from gpu_sdr_amd import GsdrError
    for args, word in (((1e6, 0, 1000, 1, 5), "swipe_s"), ((1e6, 0, 1000, 100, 0), "n_points"), ((0.0, 0, 1000, 100, 5), "rate"), ((-1.0, 0, 1000, 100, 5), "rate")):
        with pytest.raises(GsdrError, match="gsdr_vna_axis: " + word):
            sweep.vna_axis(*args)


@pytest.mark.parametrize("n_points,f_step,tau", [(1000, 200.0, 250e-6), (67, 10e3, 3e-6)])
def test_line_delay_of_a_noiseless_cable(sweep, n_points, f_step, tau):
    """Rows 0.7 e^{-2 pi i f tau} on the axis, three sweeps.  The bar of 1e-6 relative: a float32 mean carries half an ulp,
    6e-8, of phase error, over a step phase of at least 0.1 rad (measured in numpy: 6e-11 and 4e-10)."""
    f = 1e6 + f_step * np.arange(n_points)
    assert 2 * np.pi * f_step * tau >= 0.1 and tau < 1 / (2 * f_step)
    one = (0.7 * np.exp(-2j * np.pi * f * tau)).astype(np.complex64)
    x = np.tile(np.stack([one, one.conj()], axis=1), (3, 1))
    s = sweep.host_sweep(2, n_points, 1, 0)
    s.feed(x)
    got = s.line_delay(f_step)
    assert s.sweeps == 3
    s.close()
    rel = np.abs(got - np.array([tau, -tau])) / tau
    print(f"line delay {n_points} points: relative error {rel.max():.3e}")
    assert rel.max() <= 1e-6, rel


@pytest.mark.parametrize("n", [2, 5, 64])
def test_variance_against_numpy(sweep, n):
    """Noise at 1e-3 of the carrier, n rows per point: against numpy.var(ddof=1) in float64 to 1e-6 (the sum formula's
    own error there is about n 2^-53 1e6 = 1e-8, the rounding to float32 6e-8)."""
    n_ch, n_points = 4, 50
    rng = np.random.default_rng(77)
    carrier = (0.5 + 0.1 * np.arange(n_ch)) * np.exp(1j * np.arange(n_ch))
    z = carrier[None, None, :] * (1 + 1e-3 * (rng.standard_normal((n, n_points, n_ch)) + 1j * rng.standard_normal((n, n_points, n_ch))))
    x = z.astype(np.complex64)
    s = sweep.host_sweep(n_ch, n_points, 1, 0)
    s.feed(x.reshape(-1, n_ch))
    mean, var = s.read(variance=True)
    s.close()
    x64 = x.astype(np.complex128)
    for got, part in ((var.real, x64.real), (var.imag, x64.imag)):
        want = np.var(part, axis=0, ddof=1)
        rel = np.abs(got - want) / want
        print(f"variance n = {n}: relative error {rel.max():.3e}")
        assert rel.max() <= 1e-6, rel.max()
    assert np.all(np.abs(mean - x64.mean(axis=0)) <= np.spacing(np.float32(np.abs(mean))))
