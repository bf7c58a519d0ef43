"""The FIR decimator on the GPU (include/gsdr.h, "FIR decimation on the device"): the device output against the host
twin (the same bits) and against the float64 oracle of tests/_decim.py, the cuttings, the extents of what a feed reads
and writes, poison, empty feeds, the refusals of a feed, a stream of the caller's, gsdr_decim_feed, and a chain of a
DIRECT handle, a decimator and a Welch object.  Every run shape of the two kernels (tests/_decim.py, RUN_F x RUN_Q)
against the twin and against the bit model of the contract's arithmetic (contract_bits); reset on a device object;
subnormals, signed zeros and overflowing chunk sums; streams of more than 2^31 and 2^32 rows and the offset at its
bound of 2^30 (measured on an MI355X: 0.09 s, 0.18 s and 0.02 s for the 2 049, 4 097 and 1 026 feeds).

Measured worst per-channel relative errors (bar 1e-5) are written to the file that GSDR_DECIM_MARGINS names, when it is
set; profiles/decim_margins.json is the committed copy."""
import json
import os

import numpy as np
import pytest

from _decim import (PARITY_BAR, RUN_F, RUN_Q, VALUE_KINDS, caller_taps, carrier, check_values_model, contract_bits, cuttings, n_out, noise,
                    oracle, rel_err, run_device, run_host, run_modelled, run_shapes, same_bits, same_values, values_case)
from _extents import check_input_untouched, check_output, guarded_input, guarded_output
from _margins import record_info, record_margin

pytestmark = pytest.mark.gpu

DECIM_MARGINS = {}


@pytest.fixture(scope="module")
def decimate(gsdr_lib):
    from gpu_sdr_amd import decimate
    yield decimate
    path = os.environ.get("GSDR_DECIM_MARGINS")
    if DECIM_MARGINS and path:
        doc = {"bar": PARITY_BAR, "metric": "max over channels of ||y - y_oracle||_2 / ||y_oracle||_2 (oracle: float64 on the float32 rows and taps)",
               "worst": max(DECIM_MARGINS.values()), "per_case": dict(sorted(DECIM_MARGINS.items(), key=lambda t: -t[1]))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


def margin(label, value):
    DECIM_MARGINS[label] = max(DECIM_MARGINS.get(label, 0.0), float(value))
    record_margin(value, label)


# name: (n_ch, q, T, offset, rows, rows per feed or None for one feed, input).  T == 20 q + 1 runs on the default taps.
CASES = {
    "1x1x5": (1, 1, 5, 0, 300, None, "noise"),
    "3x2x41": (3, 2, 41, 20, 500, None, "carrier"),
    "3x7x6": (3, 7, 6, 6, 400, None, "noise"),
    "65x7x141": (65, 7, 141, 70, 1500, None, "carrier"),
    "1030x3x10": (1030, 3, 10, 2, 200, None, "noise"),
    "2048x100x2001": (2048, 100, 2001, 1000, 4000, None, "carrier"),
    "4x100x2001": (4, 100, 2001, 99, 60000, 20000, "noise"),
    "2x4096x81921": (2, 4096, 81921, 40960, 4096 * 30, None, "carrier"),
    "5x64x4096": (5, 64, 4096, 63, 64 * 80, None, "noise"),
}
CUTTING = ["65x7x141", "3x2x41", "3x7x6"]        # many channels, few channels, T < q

_memo = {}


def case_of(name):
    """(x, taps or None for the default taps) of a case, made once and left unchanged."""
    if name not in _memo:
        n_ch, q, T, offset, rows, _, kind = CASES[name]
        x = (carrier if kind == "carrier" else noise)(rows, n_ch, seed=7)
        taps = None if T == 20 * q + 1 and q >= 2 else caller_taps(T)
        _memo[name] = (x, taps)
    return _memo[name]


def feeds_of(name):
    rows, per = CASES[name][4], CASES[name][5]
    return None if per is None else [min(per, rows - at) for at in range(0, rows, per)]


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_twin_and_oracle(decimate, cuda_device, name):
    n_ch, q, T, offset, rows, _, _ = CASES[name]
    x, taps = case_of(name)
    got = run_device(decimate, x, q, taps, offset, cuda_device, feeds_of(name))
    twin = run_host(decimate, x, q, taps, offset, feeds_of(name))
    assert got.shape == (n_out(rows, offset, q), n_ch) and got.shape[0] >= 8
    assert same_bits(got, twin)
    err = rel_err(got, oracle(x, q, decimate.fir_taps(q) if taps is None else taps, offset))
    print(f"decim {name}: {err:.3e}")
    margin(name, err)
    assert err <= PARITY_BAR, err


@pytest.mark.parametrize("name", CUTTING)
def test_same_bits_under_every_cutting(decimate, cuda_device, name):
    n_ch, q, T, offset, rows, _, _ = CASES[name]
    x, taps = case_of(name)
    want = run_host(decimate, x, q, taps, offset)
    for cname, cut in cuttings(rows, q).items():
        assert same_bits(run_device(decimate, x, q, taps, offset, cuda_device, cut), want), cname


@pytest.mark.parametrize("pattern,off", [("nan", 1), ("huge", 0)])
@pytest.mark.parametrize("name", ["65x7x141", "3x2x41", "3x7x6", "1030x3x10"])
def test_extents_and_alignment(decimate, gsdr_lib, cuda_device, name, pattern, off):
    """Input and output in the middle of larger allocations, 8 bytes past a 16-byte boundary or on it: the feed reads
    rows_dev[0, n_rows n_ch) only (a guard that reached an output would show), writes out_dev[0, emitted n_ch) only, and
    leaves the input as it was.  Two feeds, so that the second goes on from carried sums."""
    import torch
    n_ch, q, T, offset, rows, _, _ = CASES[name]
    x, taps = case_of(name)
    want = run_host(decimate, x, q, taps, offset)
    d = decimate.device_decimator(n_ch, rows, q, taps=taps, offset=offset, device_index=0)
    cut, at, seen = [rows // 3 + 1, rows - rows // 3 - 1], 0, 0
    for n in cut:
        part = x[at:at + n]
        m = d.next_rows(n)
        whole_in, view_in = guarded_input(part.reshape(-1), off, pattern, cuda_device)
        whole_out, view_out = guarded_output(m * n_ch, 1 - off, cuda_device)
        assert gsdr_lib.gsdr_decim_feed_device(d._h, view_in.data_ptr(), n, view_out.data_ptr(), None) == m
        torch.cuda.synchronize()
        check_output(whole_out, view_out, m * n_ch)
        check_input_untouched(whole_in, part.reshape(-1), off, pattern)
        assert same_bits(view_out.cpu().numpy().reshape(m, n_ch), want[seen:seen + m])
        at += n
        seen += m
    assert seen == want.shape[0] > 0
    d.close()


def test_poison_reaches_exactly_its_windows(decimate, cuda_device):
    for n_ch, q, T, offset, rows, r_inf, r_nan, on_zero in ((3, 7, 17, 8, 200, 67, 130, 10), (70, 5, 33, 16, 300, 100, 207, None)):
        h = caller_taps(T)
        x = carrier(rows, n_ch, seed=31)
        clean = run_device(decimate, x, q, h, offset, cuda_device)
        bad = x.copy()
        bad[r_inf, 1] = np.complex64(complex(np.inf, 0.0))
        bad[r_nan, 1] = np.complex64(complex(0.0, np.nan))
        for cut in (None, cuttings(rows, q)["sevens"]):
            got = run_device(decimate, bad, q, h, offset, cuda_device, cut)
            hit = np.array([any(o * q + offset - (T - 1) <= r <= o * q + offset for r in (r_inf, r_nan)) for o in range(got.shape[0])])
            assert hit.sum() >= 4
            if on_zero is not None:                # row 67 sits on the zero tap h[5] of output 10
                assert h[5] == 0.0 and r_inf - (on_zero * q + offset - (T - 1)) == 5 and hit[on_zero]
            assert np.array_equal(~np.isfinite(got[:, 1]), hit)
            others = [c for c in range(n_ch) if c != 1]
            assert same_bits(got[~hit], clean[~hit]) and same_bits(got[:, others], clean[:, others])


def test_empty_feeds_and_feeds_that_emit_nothing(decimate, gsdr_lib, cuda_device):
    import torch
    n_ch, q, T, offset = 3, 50, 120, 70
    h, x = caller_taps(T), noise(400, n_ch, seed=61)
    want = run_host(decimate, x, q, h, offset)
    d = decimate.device_decimator(n_ch, 256, q, taps=h, offset=offset, device_index=0)
    xd = torch.from_numpy(x).to(cuda_device)
    out = torch.zeros((16, n_ch), dtype=torch.complex64, device=cuda_device)
    assert gsdr_lib.gsdr_decim_feed_device(d._h, None, 0, None, None) == 0          # touches no pointer
    assert d.next_rows(60) == 0 and gsdr_lib.gsdr_decim_feed_device(d._h, xd.data_ptr(), 60, None, None) == 0   # rows 0 .. 59: none complete
    assert d.rows_seen == 60 and d.rows_out == 0
    seen = 0
    for a, b in ((60, 70), (70, 71), (71, 71), (71, 121), (121, 377), (377, 400)):
        seen += d.feed_device(xd[a:b], out[seen:], stream=None)
    torch.cuda.synchronize()
    assert seen == want.shape[0] == n_out(400, offset, q) and same_bits(out[:seen].cpu().numpy(), want)
    d.close()


def test_a_feed_that_is_too_long_is_refused(decimate, gsdr_lib, cuda_device):
    import torch
    from gpu_sdr_amd import GsdrError
    h, x = caller_taps(9), noise(64, 2, seed=71)
    d = decimate.device_decimator(2, 16, 4, taps=h, offset=3, device_index=0)
    xd = torch.from_numpy(x).to(cuda_device)
    out = torch.zeros((32, 2), dtype=torch.complex64, device=cuda_device)
    a = d.feed_device(xd[:10], out)
    with pytest.raises(GsdrError, match=r"gsdr_decim_feed_device: .*n_rows"):
        d.feed_device(xd[:17], out[a:])
    assert gsdr_lib.gsdr_decim_feed(d._h, xd.data_ptr(), -1, x.ctypes.data, None) == -1
    assert d.rows_seen == 10 and d.rows_out == a
    b = d.feed_device(xd[10:26], out[a:])
    torch.cuda.synchronize()
    assert same_bits(out[:a + b].cpu().numpy(), run_host(decimate, x[:26], 4, h, 3))
    d.close()


def test_on_a_stream_of_the_callers(decimate, cuda_device):
    import torch
    n_ch, q, T, offset, rows, _, _ = CASES["65x7x141"]
    x, taps = case_of("65x7x141")
    got = run_device(decimate, x, q, taps, offset, cuda_device, cuttings(rows, q)["max_rows"], stream=torch.cuda.Stream())
    assert same_bits(got, run_host(decimate, x, q, taps, offset))


def test_feed_to_the_host(decimate, cuda_device):
    import torch
    n_ch, q, T, offset, rows, _, _ = CASES["3x2x41"]
    x, taps = case_of("3x2x41")
    d = decimate.device_decimator(n_ch, 200, q, taps=taps, offset=offset, device_index=0)
    xd = torch.from_numpy(x).to(cuda_device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    parts = [d.feed(xd[at:at + 200], stream=stream).copy() for at in range(0, rows, 200)] + [d.feed(xd[:0], stream=stream)]
    d.close()
    assert same_bits(np.concatenate(parts), run_host(decimate, x, q, taps, offset))


@pytest.mark.parametrize("q", RUN_Q)
def test_every_run_shape(decimate, cuda_device, q):
    """The grid of tests/_decim.py (RUN_F x RUN_Q x pad 0, q - 1 and in between): every chunks-per-thread of
    decim_partial_kernel with full and clamped last groups, every count of turns and tail of decim_combine_kernel, and
    factors on both sides of the 8 rows a thread has in flight.  Each case as one feed and cut unevenly with max_rows the
    largest feed, so that the ring wraps inside the case; the same bits as the host twin, and as the model of the
    contract where it is affordable (run_modelled)."""
    shapes = run_shapes(q)
    assert len(shapes) >= (3 if q > 1 else 1) * len(RUN_F)
    for name, n_ch, _, T, offset, rows in shapes:
        F = (T + q - 1) // q
        x, h = noise(rows, n_ch, seed=13), caller_taps(T)
        twin = run_host(decimate, x, q, h, offset)
        assert twin.shape == (n_out(rows, offset, q), n_ch) and twin.shape[0] >= F + 13
        one = run_device(decimate, x, q, h, offset, cuda_device)
        assert same_bits(one, twin), (name, "one feed")
        cut = cuttings(rows, q)["uneven"]
        assert (max(cut) - 1) // q + 2 + F < F + 13               # fewer ring blocks than the case has blocks: it wraps
        assert same_bits(run_device(decimate, x, q, h, offset, cuda_device, cut, max_rows=max(cut)), twin), (name, "uneven")
        if run_modelled(F, q):
            assert same_bits(one, contract_bits(x, q, h, offset)), (name, "contract")
        err = rel_err(one, oracle(x, q, h, offset))
        margin(name, err)
        assert err <= PARITY_BAR, (name, err)


@pytest.mark.parametrize("T", [3, 141])
@pytest.mark.parametrize("offset", [2, 6, 70])
def test_reset_on_the_device(decimate, cuda_device, T, offset):
    """q = 7, F = 1 and F = 21.  Stream A ends in the middle of a block and leaves open chunk sums in the ring; after
    reset() stream B, in two feeds, gives what a fresh object and the twin give: the first block of B starts from +0
    where it begins before row 0 (offsets 2 and 70: r0 < 0) and where it begins on row 0 (offset q - 1 = 6)."""
    import torch
    n_ch, q = 3, 7
    h = caller_taps(T)
    a, b = carrier(45 + offset % 5, n_ch, seed=52), noise(offset + 30 * q + 4, n_ch, seed=53)
    r0 = offset % q + 1 - q
    assert (r0 < 0) == (offset % q != q - 1) and (a.shape[0] - r0) % q != 0          # A ends inside a block
    want = run_host(decimate, b, q, h, offset)
    fresh = run_device(decimate, b, q, h, offset, cuda_device, [64, b.shape[0] - 64], max_rows=64 + 30 * q)
    d = decimate.device_decimator(n_ch, 64 + 30 * q, q, taps=h, offset=offset, device_index=0)
    ad, bd = torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device)
    out = torch.zeros((want.shape[0] + 8, n_ch), dtype=torch.complex64, device=cuda_device)
    m = d.feed_device(ad, out)
    assert d.rows_seen == a.shape[0] and d.rows_out == m == n_out(a.shape[0], offset, q)
    torch.cuda.synchronize()                                      # the contract leaves the ordering to the caller
    d.reset()
    assert d.rows_seen == 0 and d.rows_out == 0 and d.next_rows(offset + 1) == 1
    m = d.feed_device(bd[:64], out)
    m += d.feed_device(bd[64:], out[m:])
    torch.cuda.synchronize()
    assert d.rows_seen == b.shape[0] and d.rows_out == m == want.shape[0] == n_out(b.shape[0], offset, q) >= 30
    got = out[:m].cpu().numpy()
    d.close()
    assert same_bits(got, want) and same_bits(fresh, want)


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_values_device_twin_and_model(decimate, cuda_device, kind):
    """Subnormal products and sums (the device keeps them, as std::fmaf does), rows of -0 (every output +0: a chunk sum
    starts at +0), and chunk sums that overflow to +Inf and -Inf, which the combine adds to NaN.  Device, twin and model
    agree bit for bit, except that a NaN matches any NaN: x86 and the GPU give the NaN of an Inf - Inf different signs and
    the contract fixes neither (same_values)."""
    x, h, q, offset = values_case(kind)
    model = contract_bits(x, q, h, offset)
    check_values_model(kind, model)
    twin = run_host(decimate, x, q, h, offset)
    for cname in ("one", "sevens"):
        got = run_device(decimate, x, q, h, offset, cuda_device, cuttings(x.shape[0], q)[cname])
        assert same_values(got, twin) and same_values(got, model), (kind, cname)
        check_values_model(kind, got)


# ---- streams of more than 2^31 and 2^32 rows: one device buffer of 2^20 rows of period LONG_R, fed again and again ----
LONG_N, LONG_R = 1 << 20, 1024


def long_pattern():
    return noise(LONG_R, 1, seed=19)


def short_reference(decimate, q, h, offset):
    """(rows, offset') of the host twin on a short stream of the same period: offset' = offset mod R q, enough rows for
    R + F outputs whose windows lie inside the stream.
    Why it may stand for the long stream: an output is a function of the T rows of its window alone (the chunks are cut
    relative to the window's end and each chunk sum depends on its block's rows alone), provided the window does not
    begin before the stream.  The stream has period R, so two windows that end a multiple of R rows apart hold the same
    rows.  Output o ends on row o q + offset; with offset' = offset (mod R q) and o' = o (mod R) the ends differ by a
    multiple of R (and for odd q, which is a unit mod R, by nothing else: all R phases are distinct)."""
    T = h.shape[0]
    F = (T + q - 1) // q
    p = offset % (LONG_R * q)
    rows = p + T + (LONG_R + F) * q
    x = np.tile(long_pattern(), (rows // LONG_R + 1, 1))[:rows]
    y = run_host(decimate, x, q, h, p)
    lo = max(0, -(-(T - 1 - p) // q))                            # first output whose window lies inside the stream
    assert y.shape[0] >= LONG_R + F + 1 and lo <= F and same_bits(y[lo:F + 1], y[lo + LONG_R:F + 1 + LONG_R])
    return y, p


def expected_rows(short, p, q, T, offset, o_first, count):
    """Outputs o_first .. o_first + count - 1 of the long stream, out of the short reference."""
    assert o_first * q + offset - (T - 1) >= 0                   # no window begins before the stream
    o = np.arange(o_first, o_first + count, dtype=np.int64) % LONG_R
    o = np.where(o * q + p < T - 1, o + LONG_R, o)
    return short[o]


def run_long(decimate, dev, q, h, offset, feeds, keep):
    """`feeds` feeds of the one device buffer, nothing uploaded or read in the loop; the count of every feed against
    n_out in Python integers.  feed index -> (first output, rows) for the feeds in `keep`; the seconds it took."""
    import time
    import torch
    d = decimate.device_decimator(1, LONG_N, q, taps=h, offset=offset, device_index=0)
    xd = torch.from_numpy(np.tile(long_pattern(), (LONG_N // LONG_R, 1))).to(dev)
    scratch = torch.zeros((d.out_capacity, 1), dtype=torch.complex64, device=dev)
    kept = {k: torch.zeros((d.out_capacity, 1), dtype=torch.complex64, device=dev) for k in keep}
    torch.cuda.synchronize()
    t0, total, first = time.perf_counter(), 0, {}
    for k in range(feeds):
        want = n_out(total + LONG_N, offset, q) - n_out(total, offset, q)
        assert d.next_rows(LONG_N) == want, k
        first[k] = (n_out(total, offset, q), want)
        assert d.feed_device(xd, kept.get(k, scratch)) == want, k
        total += LONG_N
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert d.rows_seen == total == feeds * LONG_N and d.rows_out == n_out(total, offset, q)
    got = {k: (first[k][0], kept[k][:first[k][1]].cpu().numpy()) for k in keep}
    d.close()
    return got, seconds


def test_rows_past_2_to_the_31(decimate, cuda_device):
    """q = 7, T = 141 (F = 21), offset 70, 2 049 feeds: the first feed against the twin fed the same rows, the feed that
    begins at stream row 2^31 (the last) against the short reference."""
    q, offset, h = 7, 70, caller_taps(141)
    got, seconds = run_long(decimate, cuda_device, q, h, offset, 2049, (0, 2048))
    record_info(seconds, "seconds")
    print(f"decim past 2^31: {seconds:.2f} s")
    x = np.tile(long_pattern(), (LONG_N // LONG_R, 1))
    o0, y0 = got[0]
    assert o0 == 0 and same_bits(y0, run_host(decimate, x, q, h, offset))
    short, p = short_reference(decimate, q, h, offset)
    o1, y1 = got[2048]
    assert o1 == n_out(1 << 31, offset, q) and y1.shape[0] >= LONG_N // q
    assert same_bits(y1, expected_rows(short, p, q, 141, offset, o1, y1.shape[0]))


def test_rows_and_outputs_past_2_to_the_32(decimate, cuda_device):
    """q = 1, T = 5, offset 0, 4 097 feeds: blocks, outputs and rows are the same numbers and all pass 2^32 with the
    last feed, which begins at stream row 2^32."""
    q, offset, h = 1, 0, caller_taps(5)
    got, seconds = run_long(decimate, cuda_device, q, h, offset, 4097, (0, 4096))
    record_info(seconds, "seconds")
    print(f"decim past 2^32: {seconds:.2f} s")
    x = np.tile(long_pattern(), (LONG_N // LONG_R, 1))
    assert got[0][0] == 0 and same_bits(got[0][1], run_host(decimate, x, q, h, offset))
    short, p = short_reference(decimate, q, h, offset)
    o1, y1 = got[4096]
    assert o1 == 1 << 32 and y1.shape[0] == LONG_N
    assert same_bits(y1, expected_rows(short, p, q, 5, offset, o1, LONG_N))


def test_offset_at_its_bound(decimate, cuda_device):
    """offset = 2^30, the accepted bound (2^30 + 1 is refused): 1 024 feeds emit nothing, the next reaches row
    offset + 1 and emits the first outputs; it and the feed after it against the short reference."""
    from gpu_sdr_amd import GsdrError
    q, offset, h = 7, 1 << 30, caller_taps(141)
    with pytest.raises(GsdrError, match=r"gsdr_decim_create: .*offset"):
        decimate.device_decimator(1, LONG_N, q, taps=h, offset=offset + 1, device_index=0)
    assert all(n_out(k * LONG_N, offset, q) == 0 for k in range(1025)) and n_out(1025 * LONG_N, offset, q) == (LONG_N - 1) // q + 1
    got, seconds = run_long(decimate, cuda_device, q, h, offset, 1026, (1023, 1024, 1025))
    record_info(seconds, "seconds")
    print(f"decim offset 2^30: {seconds:.2f} s")
    short, p = short_reference(decimate, q, h, offset)
    assert p == offset % (LONG_R * q) == 4096 and got[1023][1].shape[0] == 0
    (oa, ya), (ob, yb) = got[1024], got[1025]
    assert oa == 0 and ob == ya.shape[0] == (LONG_N - 1) // q + 1 and yb.shape[0] >= LONG_N // q
    assert same_bits(ya, expected_rows(short, p, q, 141, offset, oa, ya.shape[0]))
    assert same_bits(yb, expected_rows(short, p, q, 141, offset, ob, yb.shape[0]))


def test_handle_decimator_welch_chain(decimate, cuda_device):
    """DIRECT, 8 tones, decim 50, buffer 50 000: 1000 rows per buffer, four buffers.  The handle's output buffer goes
    straight into a decimator (q = 10, default taps) and its output into a Welch object (nperseg 64), all on one stream
    with no wait in between."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import host_tones
    rate, L, n_ch, q = 1_000_000, 50_000, 8, 10
    freq = [-400_000, -300_000, -200_000, -100_000, 100_000, 200_000, 300_000, 400_000]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=L, decim=50, pf_average=4, freq=freq,
                                          wave_type=[g.w_type.DIRECT] * n_ch), device_index=0)
    max_rows = dem.out_capacity // n_ch
    dec = decimate.device_decimator(n_ch, max_rows, q, device_index=0)
    w = g.device_welch(n_ch, dec.out_capacity, 64, device_index=0)
    ampl, phase = np.full(n_ch, 0.1, dtype=np.float32), np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream = torch.cuda.Stream()
    outs, kept, dec_outs, dec_kept = [], [], [], []
    for k in range(4):
        xin = torch.from_numpy(host_tones(L, k * L, rate, freq, ampl, phase, sigma=2e-2, seed=20 + k)).to(cuda_device)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        y = torch.empty((dec.out_capacity, n_ch), dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        n = dem.process_device(xin, out, stream=stream)
        assert n % n_ch == 0 and n > 0
        m = dec.feed_device(out[:n], y, stream=stream)
        w.feed_device(y[:m], stream=stream)
        outs.append(out), kept.append(n), dec_outs.append(y), dec_kept.append(m)
    _, psd, n_seg = w.read("raw", fs=1.0, stream=stream)
    rows = np.concatenate([o[:n].cpu().numpy().reshape(-1, n_ch) for o, n in zip(outs, kept)])
    got = np.concatenate([y[:m].cpu().numpy() for y, m in zip(dec_outs, dec_kept)])
    dec.close(), w.close(), dem.close()
    twin = run_host(decimate, rows, q, None, None, [n // n_ch for n in kept])
    assert rows.shape[0] == 4000 and got.shape[0] == n_out(4000, 100, q) == 390
    assert same_bits(got, twin)
    assert n_seg == (390 - 64) // 32 + 1 and np.all(np.isfinite(psd)) and np.all(psd >= 0) and psd.max() > 0
