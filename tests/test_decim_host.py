"""The FIR decimator without a GPU (include/gsdr.h, "FIR decimation on the device"): the default taps against
scipy.signal.firwin, the host twin (GSDR_DECIM_HOST) against scipy.signal.decimate and against the float64 oracle of
tests/_decim.py over a grid of factors, tap counts and offsets, the count law, the cuttings, poison, every refusal and
the entries on a NULL object.

Measured here (bar 1e-5): host twin against scipy.signal.decimate 0.8e-7 .. 2.0e-7; against the oracle over the grid
2.7e-8 .. 7.2e-6, the largest at q = 4096 (signed random taps, chains of 4096 fused multiply-adds: 7.2e-6 with 2 q + 3
taps, 6.8e-6 with 64 q); the device gives the same bits (tests/test_gpu_decim.py)."""
import ctypes as C

import numpy as np
import pytest

from _decim import (INPUTS, PARITY_BAR, caller_taps, carrier, cuttings, n_out, noise, oracle, rel_err, run_host, same_bits)


@pytest.fixture(scope="module")
def decimate(gsdr_lib):
    from gpu_sdr_amd import decimate
    return decimate


def last_error(lib):
    return lib.gsdr_last_error(None).decode()


@pytest.mark.parametrize("q", [2, 3, 7, 100, 4096])
def test_default_taps_are_scipys_fir_design(decimate, q):
    from scipy.signal import firwin
    t = decimate.fir_taps(q)
    ref = firwin(20 * q + 1, 1.0 / q, window="hamming").astype(np.float32)
    assert t.dtype == np.float32 and t.shape == ref.shape
    ulp = float(np.spacing(np.float32(ref.max())))
    assert np.abs(t.astype(np.float64) - ref.astype(np.float64)).max() <= ulp
    assert np.array_equal(t.view(np.uint32), t[::-1].view(np.uint32))
    assert abs(t.astype(np.float64).sum() - 1.0) <= 1e-6
    d = decimate.host_decimator(2, 16, q)
    assert d.n_taps == 20 * q + 1 and d.offset == 10 * q and np.array_equal(d.taps.view(np.uint32), t.view(np.uint32))
    d.close()


def test_default_taps_refusals(gsdr_lib):
    w = (C.c_float * 64)()
    assert gsdr_lib.gsdr_decim_default_taps(1, w) == -1
    assert gsdr_lib.gsdr_decim_default_taps(4097, w) == -1
    assert gsdr_lib.gsdr_decim_default_taps(2, None) == -1
    assert gsdr_lib.gsdr_decim_default_taps(2, w) == 41


@pytest.mark.parametrize("kind", ["carrier", "noise"])
@pytest.mark.parametrize("q", [2, 7, 100])
def test_host_twin_against_scipy_decimate(decimate, q, kind):
    from scipy.signal import decimate as sp_decimate
    T = 20 * q + 1
    rows = T + 40 * q + 5
    x = INPUTS[kind](rows, 2, seed=11 + q)
    y = run_host(decimate, x, q, None, None)
    ref = sp_decimate(x.astype(np.complex128), q, ftype="fir", axis=0)
    m = n_out(rows, (T - 1) // 2, q)
    assert y.shape[0] == m >= 30 and ref.shape[0] >= m
    err = rel_err(y, ref[:m])
    print(f"scipy.signal.decimate q={q} {kind}: {err:.3e}")
    assert err <= PARITY_BAR, err


def _tap_counts(q):
    named = {"1": 1, "q-1": q - 1, "q": q, "q+1": q + 1, "2q+3": 2 * q + 3, "20q+1": 20 * q + 1, "64q": 64 * q}
    return {k: T for k, T in named.items() if 1 <= T <= 64 * q}


GRID = [(q, name) for q in (1, 2, 7, 100, 4096) for name in _tap_counts(q)]


@pytest.mark.parametrize("q,name", GRID)
def test_host_twin_against_the_oracle(decimate, q, name):
    T = _tap_counts(q)[name]
    h = caller_taps(T)
    if T >= 6:
        assert np.count_nonzero(h == 0) == 1 and not np.array_equal(h, h[::-1]) and h.min() < 0 < h.max()
    worst = 0.0
    for k, offset in enumerate(sorted({0, q - 1, (T - 1) // 2, T + 5})):
        for n_ch in (1, 3):
            rows = offset + 8 * q + 3
            x = (carrier, noise)[(k + n_ch) % 2](rows, n_ch, seed=5 + k)
            y = run_host(decimate, x, q, h, offset)
            ref = oracle(x, q, h, offset)
            assert y.shape == ref.shape and y.shape[0] >= 8
            worst = max(worst, rel_err(y, ref))
    print(f"host twin q={q} T={T}: {worst:.3e}")
    assert worst <= PARITY_BAR, worst


def test_count_law_exhaustively(gsdr_lib):
    one = (C.c_float * 1)(1.0)
    for q in range(1, 6):
        for p in range(0, 13):
            zeros = np.zeros(48, dtype=np.complex64)
            out = np.zeros(48, dtype=np.complex64)
            for total in range(0, 41):
                d = gsdr_lib.gsdr_decim_create(1, 48, q, 1, one, p, -2)
                assert d
                assert gsdr_lib.gsdr_decim_feed_host(d, zeros.ctypes.data, total, out.ctypes.data) == n_out(total, p, q)
                assert gsdr_lib.gsdr_decim_rows(d) == total and gsdr_lib.gsdr_decim_rows_out(d) == n_out(total, p, q)
                for n in (0, 1, 2, q - 1, q, q + 1, 7, 48):
                    assert gsdr_lib.gsdr_decim_next_rows(d, n) == n_out(total + n, p, q) - n_out(total, p, q), (q, p, total, n)
                assert gsdr_lib.gsdr_decim_next_rows(d, 49) == -1 and gsdr_lib.gsdr_decim_next_rows(d, -1) == -1
                assert gsdr_lib.gsdr_decim_out_capacity(d) == 47 // q + 1
                gsdr_lib.gsdr_decim_close(d)


CUT_CASES = {"3x2x41": (3, 2, 41, 20, 300), "3x7x6": (3, 7, 6, 6, 300), "2x7x141": (2, 7, 141, 70, 500), "1x5x17_late": (1, 5, 17, 22, 200)}


@pytest.mark.parametrize("name", list(CUT_CASES))
def test_same_bits_under_every_cutting(decimate, name):
    n_ch, q, T, offset, rows = CUT_CASES[name]
    x, h = noise(rows, n_ch, seed=21), caller_taps(T)
    cuts = cuttings(rows, q)
    want = run_host(decimate, x, q, h, offset, cuts["one"])
    assert want.shape[0] == n_out(rows, offset, q) > 8
    for cname, cut in cuts.items():
        assert same_bits(run_host(decimate, x, q, h, offset, cut), want), cname


def test_poison_reaches_exactly_its_windows(decimate):
    n_ch, q, T, offset, rows = 3, 7, 17, 8, 200
    h = caller_taps(T)
    assert h[5] == 0.0
    x = carrier(rows, n_ch, seed=31)
    clean = run_host(decimate, x, q, h, offset)
    bad = x.copy()
    r_inf, r_nan = 67, 130                     # row 67 sits on the zero tap of output 10: 67 - (7 * 10 + 8 - 16) == 5
    bad[r_inf, 1] = np.complex64(complex(np.inf, 0.0))
    bad[r_nan, 1] = np.complex64(complex(0.0, np.nan))
    for cut in (None, cuttings(rows, q)["sevens"]):
        got = run_host(decimate, bad, q, h, offset, cut)
        hit = np.array([any(o * q + offset - (T - 1) <= r <= o * q + offset for r in (r_inf, r_nan)) for o in range(got.shape[0])])
        assert hit[10] and hit.sum() == 4          # outputs 9, 10 and 18, 19
        assert np.array_equal(~np.isfinite(got[:, 1]), hit)
        assert same_bits(got[~hit], clean[~hit]) and same_bits(got[:, [0, 2]], clean[:, [0, 2]])


REFUSALS = [
    (dict(n_ch=0), "n_ch"), (dict(n_ch=(1 << 20) + 1), "n_ch"), (dict(max_rows=0), "max_rows"), (dict(max_rows=(1 << 20) + 1), "max_rows"),
    (dict(q=0), "q must"), (dict(q=4097), "q must"), (dict(n_taps=0), "n_taps"), (dict(q=2, n_taps=129), "n_taps"),
    (dict(n_taps=-1), "n_taps"), (dict(poison=np.inf), "taps"), (dict(poison=np.nan), "taps"), (dict(offset=-1), "offset"),
    (dict(offset=(1 << 30) + 1), "offset"), (dict(device_index=-3), "device_index"), (dict(null_taps=True, n_taps=5), "taps"),
    (dict(null_taps=True, n_taps=0, q=1), "q must"),
]


@pytest.mark.parametrize("change,named", REFUSALS)
def test_every_refusal_names_its_argument(gsdr_lib, change, named):
    a = dict(n_ch=2, max_rows=16, q=4, n_taps=9, offset=3, device_index=-2)
    a.update({k: v for k, v in change.items() if k in a})
    taps = np.linspace(-1.0, 1.0, 200).astype(np.float32)
    if "poison" in change:
        taps[4] = change["poison"]
    d = gsdr_lib.gsdr_decim_create(a["n_ch"], a["max_rows"], a["q"], a["n_taps"], None if change.get("null_taps") else taps.ctypes.data,
                                   a["offset"], a["device_index"])
    assert not d
    msg = last_error(gsdr_lib)
    assert msg.startswith("gsdr_decim_create: ") and named in msg, msg


def test_bounds_are_accepted_at_their_ends(gsdr_lib):
    taps = np.full(64 * 4096, 1e-3, dtype=np.float32)
    for n_ch, max_rows, q, n_taps, offset in ((1, 1, 1, 1, 0), (1, 1, 4096, 64 * 4096, 1 << 30), (1, 1 << 20, 4096, 1, 0), (1 << 20, 1, 1, 1, 0)):
        d = gsdr_lib.gsdr_decim_create(n_ch, max_rows, q, n_taps, taps.ctypes.data, offset, -2)
        assert d, last_error(gsdr_lib)
        gsdr_lib.gsdr_decim_close(d)
    d = gsdr_lib.gsdr_decim_create(1, 8, 2, 0, None, 20, -2)
    assert d and gsdr_lib.gsdr_decim_get_taps(d, None, 0) == 41
    gsdr_lib.gsdr_decim_close(d)


def test_feed_refusals_leave_the_state(decimate, gsdr_lib):
    d = decimate.host_decimator(2, 16, 4, taps=caller_taps(9), offset=3)
    x = noise(40, 2, seed=41)
    a = d.feed(x[:10])
    for n in (17, -1):
        assert gsdr_lib.gsdr_decim_feed_host(d._h, x.ctypes.data, n, x.ctypes.data) == -1
        assert last_error(gsdr_lib).startswith("gsdr_decim_feed_host: ") and "n_rows" in last_error(gsdr_lib)
    assert gsdr_lib.gsdr_decim_feed_host(d._h, None, 3, x.ctypes.data) == -1 and "rows" in last_error(gsdr_lib)
    assert gsdr_lib.gsdr_decim_feed_host(d._h, None, 0, None) == 0                       # touches no pointer
    # the device feeds are refused on a host object, before any device is touched
    assert gsdr_lib.gsdr_decim_feed_device(d._h, x.ctypes.data, 4, x.ctypes.data, None) == -1
    assert last_error(gsdr_lib).startswith("gsdr_decim_feed_device: ") and "GSDR_DECIM_HOST" in last_error(gsdr_lib)
    assert gsdr_lib.gsdr_decim_feed(d._h, x.ctypes.data, 4, x.ctypes.data, None) == -1
    assert last_error(gsdr_lib).startswith("gsdr_decim_feed: ")
    assert d.rows_seen == 10
    b = d.feed(x[10:26])
    d.close()
    assert same_bits(np.concatenate([a, b]), run_host(decimate, x[:26], 4, caller_taps(9), 3))


def test_reset_restarts_the_stream(decimate):
    h, x = caller_taps(30), noise(120, 3, seed=51)
    want = run_host(decimate, x, 7, h, 11)
    d = decimate.host_decimator(3, 64, 7, taps=h, offset=11)
    d.feed(carrier(45, 3, seed=52))               # leaves an open block and carried sums behind
    d.reset()
    assert d.rows_seen == 0 and d.rows_out == 0
    got = np.concatenate([d.feed(x[:64]), d.feed(x[64:])])
    d.close()
    assert same_bits(got, want)


def test_entries_on_a_null_object(gsdr_lib):
    buf = np.zeros(8, dtype=np.complex64)
    gsdr_lib.gsdr_decim_close(None)
    assert gsdr_lib.gsdr_decim_next_rows(None, 5) == 0 and gsdr_lib.gsdr_decim_out_capacity(None) == 0
    assert gsdr_lib.gsdr_decim_get_taps(None, None, 0) == 0
    assert gsdr_lib.gsdr_decim_rows(None) == 0 and gsdr_lib.gsdr_decim_rows_out(None) == 0
    for name, call in (("gsdr_decim_feed_host", lambda: gsdr_lib.gsdr_decim_feed_host(None, buf.ctypes.data, 1, buf.ctypes.data)),
                       ("gsdr_decim_feed_device", lambda: gsdr_lib.gsdr_decim_feed_device(None, buf.ctypes.data, 1, buf.ctypes.data, None)),
                       ("gsdr_decim_feed", lambda: gsdr_lib.gsdr_decim_feed(None, buf.ctypes.data, 1, buf.ctypes.data, None)),
                       ("gsdr_decim_reset", lambda: gsdr_lib.gsdr_decim_reset(None))):
        assert call() == -1
        assert last_error(gsdr_lib).startswith(name + ": ") and "null" in last_error(gsdr_lib), name
