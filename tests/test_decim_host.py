"""The FIR decimator without a GPU (include/gsdr.h, "FIR decimation on the device"): the default taps against
scipy.signal.firwin, the host twin (GSDR_DECIM_HOST) against scipy.signal.decimate and against the float64 oracle of
tests/_decim.py over a grid of factors, tap counts and offsets, the count law, the cuttings, poison, every refusal and
the entries on a NULL object.  fma32 and contract_bits of tests/_decim.py -- the paragraph "Arithmetic" written out
from the header, with no ring -- against a rational reference and against the twin, bit for bit, over the run shapes
of the kernels; two deliberately wrong models that the twin must differ from; the counts across stream row 2^31.

Measured here (bar 1e-5): host twin against scipy.signal.decimate 0.8e-7 .. 2.0e-7; against the oracle over the grid
2.7e-8 .. 7.2e-6, the largest at q = 4096 (signed random taps, chains of 4096 fused multiply-adds: 7.2e-6 with 2 q + 3
taps, 6.8e-6 with 64 q); the device gives the same bits (tests/test_gpu_decim.py)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from _decim import (INPUTS, PARITY_BAR, RUN_F, RUN_Q, VALUE_KINDS, caller_taps, carrier, check_values_model, contract_bits, cuttings, fma32,
                    n_out, noise, oracle, rel_err, run_host, run_modelled, run_tap_counts, same_bits, same_values, values_case)


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


# ---- the bit model of the contract (tests/_decim.py: fma32, contract_bits) ----------------------------------------

def _f32(v):
    return np.float32(v)


def _round_once(a, b, c):
    """float32(a b + c) from the exact rational value, rounded once, ties to even: the reference of fma32."""
    a, b, c = _f32(a), _f32(b), _f32(c)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        p_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        if a != 0 and b != 0:                      # the product is not zero: it cancels c exactly, +0
            return _f32(0.0)
        return _f32(-0.0) if p_neg and np.signbit(c) else _f32(0.0)          # (+-0) + (+-0)
    mag = abs(exact)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()           # 2^(e-1) < mag < 2^(e+1)
    if Fraction(2) ** e > mag:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n, rest = divmod(mag, ulp)
    if rest * 2 > ulp or (rest * 2 == ulp and n % 2 == 1):
        n += 1
    val = n * ulp
    out = np.inf if val >= Fraction(2) ** 128 else float(val)
    return _f32(-out if exact < 0 else out)


def _fma_triples():
    """(a, b, c) float32 triples: the issue's counter-example and its family (a b just above or just below half an ulp
    of c, c of both signs and both last-bit parities), subnormal results, results that round up into the next binade,
    exact cancellations, signed zeros, and a few thousand random ones over many exponents."""
    rng = np.random.default_rng(77)
    u = 2.0 ** -23
    t = [(2.0 ** -24 * (1 + u), 1 - u, 1 + u)]
    for k in range(1, 400):
        for sign in (1.0, -1.0):
            c = sign * (1 + k * u)                                   # ulp(c) = 2^-23: half an ulp is 2^-24
            for above in (1 + k * u, 1 - (k % 7 + 1) * u / 2):       # a b = 2^-24 (1 +- few 2^-23): beside the tie
                t.append((2.0 ** -24 * (1 + u), above, c))
                t.append((-(2.0 ** -24) * (1 + u), above, c))
    for k in range(300):                                             # subnormal results, ties among them
        t.append(((1 + k * u) * 2.0 ** -70, (1.5 + k * u) * 2.0 ** -70, (k % 5) * 2.0 ** -149))
        t.append(((3 + 2 * k) * 2.0 ** -100, 2.0 ** -50, -(k % 3) * 2.0 ** -148))     # odd multiples of 2^-150: ties
    for k in range(300):                                             # round up into the next binade
        t.append((2.0 ** -24, 1 + k * u, 2 - u))
        t.append((-(1 + u * k), 2.0 ** -25, -(1 - u / 2)))
    for k in range(200):                                             # exact cancellation: +0
        a, b = 1 + k * u, 2.0 ** (k % 20 - 10)
        t.append((a, b, -(a * b)))
        t.append((-a, b, a * b))
    t += [(0.0, 1.0, 0.0), (-0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, -0.0), (0.0, 0.0, -0.0), (3e38, 3.0, -3e38), (3e38, 2.0, 3e38)]
    m = rng.standard_normal((3000, 3)) * 2.0 ** rng.integers(-40, 40, size=(3000, 3))
    m[:1000, 2] = -(m[:1000, 0].astype(np.float32).astype(np.float64) * m[:1000, 1].astype(np.float32)) * (1 + rng.integers(-3, 4, 1000) * u)
    arr = np.concatenate([np.array(t, dtype=np.float64), m]).astype(np.float32)
    assert np.all(np.isfinite(arr))
    return arr


def test_fma32_rounds_once():
    tr = _fma_triples()
    a, b, c = tr[:, 0], tr[:, 1], tr[:, 2]
    assert tr.shape[0] >= 5000
    got = fma32(a, b, c)
    want = np.array([_round_once(*row) for row in tr], dtype=np.float32)
    assert got.dtype == np.float32
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(tr[i].tolist(), float(got[i]), float(want[i])) for i in bad[:5]]
    # what the triples hold: the issue's counter-example gives 1 + 2^-23, subnormal results, a binade crossed, +0
    u = np.float32(2.0 ** -23)
    assert got[0] == np.float32(1) + u
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert np.count_nonzero((got != 0) & (np.abs(got) < tiny)) >= 100
    assert np.count_nonzero((np.abs(c) < 2) & (np.abs(got) == 2)) >= 1 and np.count_nonzero((np.abs(c) < 1) & (np.abs(got) == 1)) >= 1
    cancelled = (a != 0) & (c != 0) & (a.astype(np.float64) * b.astype(np.float64) == -c.astype(np.float64))
    assert np.count_nonzero(cancelled) >= 100 and not np.any(np.signbit(got[cancelled]))
    # ... and they discriminate: the expression that rounds to float64 first and to float32 second is wrong on some
    with np.errstate(over="ignore"):
        twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    differ = np.flatnonzero(twice.view(np.uint32) != got.view(np.uint32))
    assert 0 in differ and twice[0] == np.float32(1) + 2 * u
    up, down = twice[differ].astype(np.float64) > got[differ], twice[differ].astype(np.float64) < got[differ]
    assert up.any() and down.any() and differ.size >= 20, differ.size


MODEL_GRID = [(q, F) for q in RUN_Q for F in RUN_F if run_modelled(F, q)]      # q in {1, 3}: every F; q in {8, 9, 17}: F <= 22


@pytest.mark.parametrize("q,F", MODEL_GRID)
def test_host_twin_has_the_bits_of_the_contract(decimate, q, F):
    """The twin against contract_bits, bit for bit: every T of the run shapes, the offsets {0, q-1, q, (T-1)//2, T+5},
    3 channels, F + 5 outputs or more (those whose windows begin before the stream and the steady state), as one feed
    and as feeds of 7 rows.  The model takes about 15 us per output and tap, so F in {63, 64} is modelled for q in
    {1, 3} only."""
    for T in run_tap_counts(F, q):
        h = caller_taps(T)
        for k, offset in enumerate(sorted({0, q - 1, q, (T - 1) // 2, T + 5})):
            rows = offset + (F + 4) * q + 3
            x = noise(rows, 3, seed=90 + k)
            want = contract_bits(x, q, h, offset)
            assert want.shape[0] == n_out(rows, offset, q) >= F + 4
            for cname in ("one", "sevens"):
                got = run_host(decimate, x, q, h, offset, cuttings(rows, q)[cname])
                assert same_bits(got, want), (q, F, T, offset, cname, int(np.flatnonzero((got != want).any(axis=1))[0]))


def _wrong_variant(x, q, taps, offset, newest_first=False, cut_from_start=False):
    """contract_bits with one law broken on purpose: the chunk sums added newest first, or the chunks cut from the
    START of the taps (chunk F-1 is t < q, chunk 0 the short one at the end)."""
    xf = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    h = np.asarray(taps, dtype=np.float32)
    T, n2 = h.shape[0], xf.shape[1]
    F = (T + q - 1) // q
    m = n_out(x.shape[0], offset, q)
    y = np.zeros((m, n2), dtype=np.float32)
    for o in range(m):
        first = o * q + offset - (T - 1)
        P = []
        for j in range(F):
            span = range((F - 1 - j) * q, min(T, (F - j) * q)) if cut_from_start else range(max(0, T - (j + 1) * q), T - j * q)
            acc = np.zeros(n2, dtype=np.float32)
            for t in span:
                if first + t >= 0:
                    acc = fma32(h[t], xf[first + t], acc)
            P.append(acc)
        order = P if newest_first else P[::-1]
        s = order[0]
        for p in order[1:]:
            s = (s + p).astype(np.float32)
        y[o] = s
    return y.view(np.complex64)


def test_the_model_has_teeth(decimate):
    """F = 21, q = 2, noise.  The unbroken variant is contract_bits (so the helper is the same law); each broken one
    differs from the twin, and so does an ordinary float32 dot product in tap order."""
    q, T, offset, rows = 2, 41, 20, 120
    x, h = noise(rows, 3, seed=95), caller_taps(T)
    twin = run_host(decimate, x, q, h, offset)
    assert twin.shape[0] == 50
    assert same_bits(_wrong_variant(x, q, h, offset), contract_bits(x, q, h, offset)) and same_bits(twin, contract_bits(x, q, h, offset))
    for broken in (dict(newest_first=True), dict(cut_from_start=True)):
        bad = _wrong_variant(x, q, h, offset, **broken)
        differ = (bad.view(np.uint32) != twin.view(np.uint32))
        assert differ.any(), broken
        assert rel_err(bad, oracle(x, q, h, offset)) <= PARITY_BAR        # and the float64 bar does not see it
        print(f"{broken}: {differ.any(axis=1).sum()} of {twin.shape[0]} output rows differ")
    xp = np.concatenate([np.zeros((T - 1, 3), dtype=np.complex64), x]).view(np.float32)
    plain = np.zeros((50, 6), dtype=np.float32)
    for o in range(50):
        for t in range(T):
            plain[o] = fma32(h[t], xp[o * q + offset + t], plain[o])
    assert (plain.view(np.uint32) != twin.view(np.float32).view(np.uint32)).any(axis=1).all()


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_values_twin_against_the_model(decimate, kind):
    """Subnormal products and sums, rows of -0, and chunk sums that overflow: the twin against the model, and the model
    against what the case is there for (tests/test_gpu_decim.py runs the same cases on the device)."""
    x, h, q, offset = values_case(kind)
    want = contract_bits(x, q, h, offset)
    check_values_model(kind, want)
    for cname in ("one", "sevens"):
        got = run_host(decimate, x, q, h, offset, cuttings(x.shape[0], q)[cname])
        assert same_values(got, want), (kind, cname)


def test_host_twin_counts_past_2_to_the_31_rows(decimate):
    """2 049 feeds of 2^20 zero rows through the cheapest shape (q = 4096, one tap, one channel): the counts of every
    feed against n_out in Python integers, across stream row 2^31.  (About 12 s: measured before it was added; the
    device crosses 2^31 and 2^32 with data in tests/test_gpu_decim.py.)"""
    q, offset, n = 4096, 4101, 1 << 20
    d = decimate.host_decimator(1, n, q, taps=np.ones(1, dtype=np.float32), offset=offset)
    x = np.zeros((n, 1), dtype=np.complex64)
    total = 0
    for k in range(2049):
        want = n_out(total + n, offset, q) - n_out(total, offset, q)
        assert d.next_rows(n) == want
        y = d.feed(x)
        total += n
        assert y.shape == (want, 1) and not y.view(np.uint32).any(), k
        assert d.rows_seen == total and d.rows_out == n_out(total, offset, q), k
    d.close()
    assert total == (1 << 31) + n and want == 256


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
