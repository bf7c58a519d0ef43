"""The Welch estimator on the host (include/gsdr.h, "Welch spectra on the device"): the numpy oracle of tests/_welch.py
against scipy.signal.welch, the library's host twin (GSDR_WELCH_HOST) against the oracle, the refusals of every entry
and the poison rule; and the preconditions of the grid of cases the GPU tests run (tests/_welch.py, GRID), which look at
the oracle and at the float32 model only.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from _welch import (DETRENDS, DISTINCT, GRID, GRID_SHAPES, HOST_BAR, MODEL_BAR, MODES, WINDOWS, Oracle, cuttings, grid_case,
                    grid_precondition, grid_total, hann32, n_segments, noise_rows, own_window, rel_err, some_gain)

SHAPES = [(16, 16), (16, 2), (64, 32), (256, 100), (256, 256), (1024, 512), (8192, 4096)]


def total_rows(nperseg, step):
    return 4 * nperseg + 3 * step + 5


@pytest.fixture(scope="module")
def spectrum(gsdr_lib):
    from gpu_sdr_amd import spectrum
    return spectrum


@pytest.fixture(scope="module")
def streams():
    """(rows, oracle) per (nperseg, step, n_ch), made once."""
    memo = {}

    def get(nperseg, step, n_ch, detrend="linear"):
        key = (nperseg, step, n_ch, detrend)
        if key not in memo:
            x = noise_rows(total_rows(nperseg, step), n_ch, seed=nperseg + step + n_ch)
            x.setflags(write=False)
            memo[key] = (x, Oracle(x, nperseg, step, detrend))
        return memo[key]
    return get


@pytest.mark.parametrize("window", ["default", "array"])
@pytest.mark.parametrize("detrend", ["linear", "constant", False])
@pytest.mark.parametrize("nperseg,step", [(64, 32), (256, 100), (256, 64), (1024, 1024)])
def test_oracle_equals_scipy(nperseg, step, detrend, window):
    """The real and the imaginary part of the rotated stream through scipy.signal.welch, noverlap = nperseg - step.
    The contract's default window is scipy's default ('hann', periodic) ROUNDED TO FLOAT32: the rounding alone moves a
    density by a few 1e-8, so scipy is given the rounded taps, and the taps are checked against scipy's own.
    Without a detrend the carrier stays in bins 0 and 1 of A0, A1 and A2, and the rotation at read time takes the
    quadrature's noise out of them by cancellation: its error there is eps (|m| / sigma)^2 N, 1e-16 x 1e6 x 64 for a
    carrier of 1 over a noise of 1e-3 -- at the bar in double, whatever the code.  That case runs with |m| / sigma = 10
    (1e-16 x 100 x 1024 = 1e-11); the detrended cases keep the carrier of 1."""
    signal = pytest.importorskip("scipy.signal")
    x = noise_rows(total_rows(nperseg, step), 3, seed=7, slope=1e-5, carrier=0.01 if detrend is False else 1.0)
    if window == "default":
        win, taps = None, hann32(nperseg)
        assert np.max(np.abs(taps.astype(np.float64) - signal.get_window("hann", nperseg))) <= 2.0 ** -24
    else:
        taps = (np.blackman(nperseg) + 0.1).astype(np.float32)
        win = taps
    o = Oracle(x, nperseg, step, "none" if detrend is False else detrend, win)
    want_segments = n_segments(x.shape[0], nperseg, step)
    assert o.n_seg == want_segments >= 4
    fs = 2.5e5
    got = o.psd("rotate", fs=fs)
    g = np.abs(o.mean) / o.mean
    z = x.astype(np.complex128) * g[None, :]
    for part, y in enumerate((z.real, z.imag)):
        f, p = signal.welch(y, fs=fs, window=taps.astype(np.float64), nperseg=nperseg, noverlap=nperseg - step, detrend=detrend,
                            scaling="density", return_onesided=True, axis=0)
        assert p.shape[0] == nperseg // 2 + 1
        # scipy drops nothing here: every segment of the contract is one of its segments
        assert rel_err(got[:, part], p.T) <= HOST_BAR, (part, rel_err(got[:, part], p.T))
    assert np.allclose(f, np.arange(nperseg // 2 + 1) * fs / nperseg, rtol=1e-14, atol=0)


def run_host(spectrum, x, nperseg, step, cut, detrend="linear", window=None, gain=None, fs=1.0):
    w = spectrum.host_welch(x.shape[1], max(max(cut), 1), nperseg, step, detrend=detrend, window=window)
    at = 0
    for n in cut:
        w.feed(x[at:at + n])
        at += n
    assert at == x.shape[0]
    modes = [m for m in MODES if m != "gain" or gain is not None]
    out = {m: w.read(m, fs=fs, gain=gain if m == "gain" else None) for m in modes}
    res = {m: out[m][1] for m in modes}, w.mean(), w.segments, w.rows_seen, [out[m][2] for m in modes]
    w.close()
    return res


@pytest.mark.parametrize("n_ch", [1, 3])
@pytest.mark.parametrize("nperseg,step", SHAPES)
def test_host_twin_equals_the_oracle(spectrum, streams, nperseg, step, n_ch):
    x, o = streams(nperseg, step, n_ch)
    gain = some_gain(n_ch)
    first = None
    for name, cut in cuttings(x.shape[0], nperseg, step).items():
        psd, mean, segs, rows, returned = run_host(spectrum, x, nperseg, step, cut, gain=gain, fs=3.0)
        assert segs == o.n_seg == n_segments(x.shape[0], nperseg, step) and rows == x.shape[0], name
        assert returned == [o.n_seg] * 4
        assert np.array_equal(mean, o.mean), name                       # the same additions in the same order
        for m in MODES:
            err = rel_err(psd[m], o.psd(m, fs=3.0, gain=gain))
            assert err <= HOST_BAR, (name, m, err)
        if first is None:
            first = psd
        for m in MODES:                                                 # and the twin itself does not see the cutting
            assert np.array_equal(psd[m], first[m]), (name, m)


@pytest.mark.parametrize("detrend", ["constant", "none"])
def test_host_twin_detrend_and_window(spectrum, detrend):
    nperseg, step = 64, 24
    # (no detrend: a carrier of 10 sigma, see test_oracle_equals_scipy)
    x = noise_rows(total_rows(nperseg, step), 2, seed=3, slope=1e-4 if detrend == "constant" else 0.0,
                   carrier=0.01 if detrend == "none" else 1.0)
    taps = (np.hamming(nperseg) * 0.7).astype(np.float32)
    o = Oracle(x, nperseg, step, detrend, taps)
    psd, mean, segs, _, _ = run_host(spectrum, x, nperseg, step, [50, 0, x.shape[0] - 50], detrend=detrend, window=taps)
    assert segs == o.n_seg
    for m in ("raw", "rotate", "dbc"):
        assert rel_err(psd[m], o.psd(m)) <= HOST_BAR, m


def test_read_before_the_first_segment_and_reset(spectrum, gsdr_lib):
    nperseg, step, n_ch = 64, 32, 3
    x = noise_rows(total_rows(nperseg, step), n_ch, seed=11)
    w = spectrum.host_welch(n_ch, 512, nperseg, step)
    w.feed(x[:nperseg - 1])
    psd = np.full((n_ch, 2, nperseg // 2 + 1), 7.0)
    mean = np.full((n_ch, 2), 7.0)
    assert gsdr_lib.gsdr_welch_read_host(w._h, 1, None, 1.0, psd.ctypes.data, mean.ctypes.data) == 0
    assert (psd == 7.0).all() and (mean == 7.0).all() and w.segments == 0 and w.rows_seen == nperseg - 1
    w.feed(x[nperseg - 1:])
    one = w.read("rotate")[1], w.mean()
    w.reset()
    assert w.rows_seen == 0 and w.segments == 0
    w.feed(x[:100])
    w.feed(x[100:])
    two = w.read("rotate")[1], w.mean()
    w.close()
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


def test_zero_mean_gives_unit_gain(spectrum):
    x = np.zeros((64, 1), dtype=np.complex64)
    x[::2], x[1::2] = 1 + 1j, -1 - 1j                         # mean exactly 0
    w = spectrum.host_welch(1, 64, 16, 16, detrend="none")
    w.feed(x)
    assert w.mean()[0] == 0
    assert np.array_equal(w.read("rotate")[1], w.read("raw")[1]) and np.array_equal(w.read("dbc")[1], w.read("raw")[1])
    w.close()


CREATE_REFUSALS = [
    ((0, 64, 64, 32, 2, -2), "n_ch"), (((1 << 20) + 1, 64, 64, 32, 2, -2), "n_ch"),
    ((2, 0, 64, 32, 2, -2), "max_rows"), ((2, (1 << 20) + 1, 64, 32, 2, -2), "max_rows"),
    ((2, 64, 8, 8, 2, -2), "nperseg"), ((2, 64, 96, 48, 2, -2), "nperseg"), ((2, 64, 16384, 8192, 2, -2), "nperseg"),
    ((2, 64, 64, 7, 2, -2), "step"), ((2, 64, 64, 65, 2, -2), "step"), ((2, 64, 64, 0, 2, -2), "step"),
    ((2, 64, 64, 32, 3, -2), "detrend"), ((2, 64, 64, 32, -1, -2), "detrend"),
    ((2, 64, 64, 32, 2, -3), "device_index"),
]


@pytest.mark.parametrize("args,names", CREATE_REFUSALS)
def test_create_refusals_name_the_argument(gsdr_lib, args, names):
    n_ch, max_rows, nperseg, step, detrend, dev = args
    assert not gsdr_lib.gsdr_welch_create(n_ch, max_rows, nperseg, step, detrend, None, dev)
    msg = gsdr_lib.gsdr_last_error(None).decode()
    assert msg.startswith("gsdr_welch_create: ") and names in msg, msg


def test_feed_and_read_refusals(spectrum, gsdr_lib):
    L = gsdr_lib
    w = spectrum.host_welch(2, 32, 16, 8)
    x = noise_rows(40, 2, seed=1)
    w.feed(x[:20])
    before = w.read("raw")[1]

    def refused(rc, entry, *names):
        msg = L.gsdr_last_error(None).decode()
        assert rc == -1 and msg.startswith(entry + ": ") and all(n in msg for n in names), (rc, msg)

    refused(L.gsdr_welch_feed_host(w._h, x.ctypes.data, -1), "gsdr_welch_feed_host", "n_rows")
    refused(L.gsdr_welch_feed_host(w._h, x.ctypes.data, 33), "gsdr_welch_feed_host", "n_rows")
    refused(L.gsdr_welch_feed_host(w._h, None, 4), "gsdr_welch_feed_host", "rows")
    refused(L.gsdr_welch_feed_host(None, x.ctypes.data, 4), "gsdr_welch_feed_host", "null object")
    assert w.rows_seen == 20 and np.array_equal(w.read("raw")[1], before)           # state unchanged
    assert L.gsdr_welch_feed_host(w._h, None, 0) == 0 and w.rows_seen == 20        # an empty feed touches no pointer
    psd = np.zeros((2, 2, 9))
    gain = some_gain(2)
    for fs in (0.0, -1.0, float("inf"), float("nan")):
        refused(L.gsdr_welch_read_host(w._h, 0, None, fs, psd.ctypes.data, None), "gsdr_welch_read_host", "fs")
    for mode in (-1, 4):
        refused(L.gsdr_welch_read_host(w._h, mode, gain.ctypes.data, 1.0, psd.ctypes.data, None), "gsdr_welch_read_host", "mode")
    refused(L.gsdr_welch_read_host(w._h, 3, None, 1.0, psd.ctypes.data, None), "gsdr_welch_read_host", "gain")
    refused(L.gsdr_welch_read_host(w._h, 0, None, 1.0, None, None), "gsdr_welch_read_host", "psd")
    refused(L.gsdr_welch_reset(None), "gsdr_welch_reset", "null object")
    # the device entries on a host object
    stream = C.c_void_p(0)
    refused(L.gsdr_welch_feed_device(w._h, x.ctypes.data, 4, stream), "gsdr_welch_feed_device", "host object")
    refused(L.gsdr_welch_read_device(w._h, 0, None, 1.0, psd.ctypes.data, stream), "gsdr_welch_read_device", "host object")
    refused(L.gsdr_welch_read(w._h, 0, None, 1.0, psd.ctypes.data, None, stream), "gsdr_welch_read", "host object")
    refused(L.gsdr_welch_mean_device(w._h, psd.ctypes.data, stream), "gsdr_welch_mean_device", "host object")
    assert L.gsdr_welch_rows(None) == 0 and L.gsdr_welch_segments(None) == 0
    L.gsdr_welch_close(None)
    w.close()


def test_python_face_checks_its_arguments(spectrum):
    with pytest.raises(ValueError):
        spectrum.host_welch(2, 32, 16, 8, detrend="quadratic")
    with pytest.raises(ValueError):
        spectrum.host_welch(2, 32, 16, 8, window=np.ones(15))
    with pytest.raises(spectrum.GsdrError):
        spectrum.host_welch(2, 32, 48)
    w = spectrum.host_welch(2, 32, 16)
    assert w.step == 8 and w.bins == 9
    with pytest.raises(ValueError):
        w.read("gain")
    with pytest.raises(ValueError):
        w.read("raw", gain=np.ones(2))
    with pytest.raises(ValueError):
        w.read("sideways")
    f, psd, n = w.read()
    assert n == 0 and (psd == 0).all() and np.array_equal(f, np.arange(9) / 16.0)
    w.close()


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_poison_stays_in_its_channel(spectrum, poison):
    nperseg, step, n_ch = 64, 32, 5
    x = noise_rows(total_rows(nperseg, step), n_ch, seed=2)
    bad = x.copy()
    at = 3 * step + 5                                           # in segments 2 and 3, in the mean from segment 3 on
    bad[at, 2] = poison
    clean, mean_c, _, _, _ = run_host(spectrum, x, nperseg, step, [x.shape[0]])
    got, mean_b, _, _, _ = run_host(spectrum, bad, nperseg, step, [100, x.shape[0] - 100])
    others = [0, 1, 3, 4]
    for m in ("raw", "rotate", "dbc"):
        assert np.array_equal(got[m][others], clean[m][others]), m
        assert not np.isfinite(got[m][2]).any(), m
    assert np.array_equal(mean_b[others], mean_c[others]) and not np.isfinite(mean_b[2])
    # the poisoned row has been fed, but the first segment that holds it (rows 64 .. 127) is not complete yet
    early, _, segs, _, _ = run_host(spectrum, bad[:127], nperseg, step, [127])
    assert segs == 2 and np.isfinite(early["raw"]).all()


def test_the_grid_covers_every_kernel_detrend_and_window():
    assert sorted(GRID_SHAPES) == [16 << k for k in range(10)] and len(GRID) == len(set(GRID)) == 60
    assert {d for _, d, _ in GRID} == {"linear", "constant", "none"} and {w for _, _, w in GRID} == {"hann", "own"}
    steps = {N: GRID_SHAPES[N][1] for N in GRID_SHAPES}
    assert any(s == N for N, s in steps.items()) and any(8 * s == N for N, s in steps.items()) and any(s & (s - 1) for s in steps.values())
    for N, (n_ch, step) in GRID_SHAPES.items():
        assert n_segments(grid_total(N), N, step) >= 9 and 1 <= step <= N
    assert sum(n_ch % 2 for n_ch, _ in GRID_SHAPES.values()) >= 6


@pytest.mark.parametrize("nperseg", list(GRID_SHAPES))
def test_own_window_is_asymmetric_signed_and_has_a_zero_tap(nperseg):
    w = own_window(nperseg)
    assert w.dtype == np.float32 and w.shape == (nperseg,)
    assert w[3] == 0 and (w < 0).sum() >= nperseg // 5 - 1 and (w > 0).sum() > nperseg // 2
    # neither reversed, nor mirrored about N/2 as the Hann window is, nor shifted by one tap, nor without its signs
    for other in (w[::-1], np.roll(w[::-1], 1), np.roll(w, 1), np.roll(w, -1), np.abs(w)):
        assert np.max(np.abs(other - w)) > 0.1


@pytest.mark.parametrize("nperseg", list(GRID_SHAPES))
def test_grid_preconditions(nperseg):
    """For the six cases of one nperseg, at the fs the GPU test reads with: every bin carries noise in every mode; the
    float32 model of the contract meets a third of the bar against the oracle (measured: 1.2e-7 .. 1.5e-6, the worst at
    8192 points, constant, Hann) -- so the input is one a float32 pipeline can resolve, and the device has two thirds of
    the bar for its own transform; and the case tells its variants apart (measured: the raw spectra of two detrends or
    two windows on the same rows differ by 0.4 .. 270 of the smaller on some bin)."""
    for detrend in DETRENDS:
        for window in WINDOWS:
            x, o = grid_case(nperseg, detrend, window)
            assert x.shape == (grid_total(nperseg), GRID_SHAPES[nperseg][0]) and x.dtype == np.complex64 and o.n_seg >= 9
            pre = grid_precondition(nperseg, detrend, window, fs=2.0e5)
            print(f"welch grid {nperseg} {detrend} {window}: floor {pre['floor']:.3f} model {pre['model']:.3e} distinct {pre['distinct']:.3g}")
            assert pre["floor"] > 0.01, (detrend, window, pre)
            assert pre["model"] <= MODEL_BAR, (detrend, window, pre)
            assert pre["distinct"] > DISTINCT, (detrend, window, pre)
            assert pre["ok"]
