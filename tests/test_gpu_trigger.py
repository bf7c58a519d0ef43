"""The trigger on the device (gsdr_trigger_feed_device / gsdr_trigger_feed; trigger_kernels.hip) against the library's
host twin fed the same rows: events, snippets and counts bit for bit, on every case and cutting of tests/_trigger.py;
long feeds (several steps per selection chunk, capped grids) and stream rows beyond 2^31; extents, streams, set_levels /
reset in stream order, and behind real DIRECT and TONES handles."""
import ctypes as C

import numpy as np
import pytest

from _extents import OUT_SENTINEL_BITS, check_input_untouched, guarded_input, guarded_output
from _trigger import (CASE_IDS, CASES, EVENT_DTYPE, LARGE_CASES, LARGE_IDS, LEVEL_DTYPE, PAST_FEEDS, PAST_N, PAST_PARAMS, PAST_TAIL,
                      default_levels, past_2g_stream, same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trig(gsdr_lib, cuda_device):
    import gpu_sdr_amd.trigger as t
    return t


def host_feeds(trig, p, levels, feeds):
    """p = (n_ch, max_rows, pre, post, holdoff, max_events); the host twin's (events, snippets, dropped) per feed."""
    h = trig.host_trigger(*p, levels)
    out = [h.feed(x) for x in feeds]
    h.close()
    return out


class DeviceRun:
    """A device trigger with plain output tensors of its own; feed() enqueues and reads the result back."""

    def __init__(self, trig, p, levels, dev, stream=None):
        import torch
        self.t = trig.device_trigger(*p, levels, device_index=0)
        n_ch, _, pre, post, _, max_events = p
        self.stream = stream
        self.ev = torch.zeros(max_events * 24, dtype=torch.uint8, device=dev)
        self.sn = torch.zeros((max_events, pre + post, n_ch), dtype=torch.complex64, device=dev)
        self.cnt = torch.full((2,), -7, dtype=torch.int32, device=dev)
        self.dev = dev

    def enqueue(self, rows):
        import torch
        x = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows)).to(self.dev)
        self.t.feed_device(x, self.ev, self.sn, self.cnt, stream=self.stream)
        return x

    def result(self):
        import torch
        (self.stream or torch.cuda.current_stream()).synchronize()
        n, dropped = (int(v) for v in self.cnt.cpu().numpy())
        assert 0 <= n <= self.t.max_events and dropped >= 0
        ev = self.ev.cpu().numpy().view(EVENT_DTYPE)[:n].copy()
        return ev, self.sn[:n].cpu().numpy(), dropped

    def feed(self, rows):
        keep = self.enqueue(rows)      # noqa: F841  (alive until the result is read)
        return self.result()

    def close(self):
        self.t.close()


def params(case):
    return (case.n_ch, case.max_rows, case.pre, case.post, case.holdoff, case.max_events)


def assert_feeds_equal(got, want, what):
    assert len(got) == len(want)
    for k, ((ge, gs, gd), (we, ws, wd)) in enumerate(zip(got, want)):
        assert gd == wd and len(ge) == len(we), (what, k, gd, wd, ge, we)
        assert same_bits(ge, we), (what, k, ge, we)
        assert same_bits(gs, ws), (what, k)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_feed_device_equals_the_host_twin(trig, cuda_device, case):
    for cut in case.cuts:
        want = host_feeds(trig, params(case), case.levels, case.feeds(cut))
        d = DeviceRun(trig, params(case), case.levels, cuda_device)
        got = [d.feed(x) for x in case.feeds(cut)]
        assert d.t.rows_seen == case.rows.shape[0]
        d.close()
        assert_feeds_equal(got, want, (case.name, cut))
        assert sum(len(e) for e, _, _ in want) > 0


@pytest.mark.parametrize("large", LARGE_CASES, ids=LARGE_IDS)
def test_long_feeds_equal_the_host_twin(trig, cuda_device, large):
    """Chunks of several 64-byte steps in trigger_select_kernel (L = 128 ... 1088), its block scans with every slot in use,
    and the row passes beyond their grid caps: what each case reaches is stated beside it in tests/_trigger.py."""
    import torch
    case = large.case()
    whole = torch.from_numpy(case.rows).to(cuda_device)            # one upload; the feeds are views of it
    for cut in case.cuts:
        want = host_feeds(trig, params(case), case.levels, case.feeds(cut))
        d = DeviceRun(trig, params(case), case.levels, cuda_device)
        got, at = [], 0
        for n in cut:
            got.append(d.feed(whole[at:at + n]))
            at += n
        assert d.t.rows_seen == case.rows.shape[0]
        d.close()
        assert_feeds_equal(got, want, (case.name, cut))
        assert sum(len(e) for e, _, _ in want) > 0


def test_rows_past_2_to_the_31(trig, cuda_device):
    """2 049 quiet feeds of 2^20 rows from one tensor, enqueued back to back with nothing read, then a tail with pulses: the
    events are those of a host twin that saw ONE quiet feed, with 2048 * 2^20 added to the rows, and the same snippets.
    (Nothing hits in the quiet rows, so only the row numbers and the carried rows depend on the prefix, and the carried
    rows are the same quiet rows; tests/test_trigger_host.py checks that shift on the host twin over all 2 049 feeds.)"""
    import torch
    quiet, tail, lv = past_2g_stream()
    h = trig.host_trigger(*PAST_PARAMS, lv)
    ev, _, _ = h.feed(quiet)
    assert len(ev) == 0
    we, ws, wd = h.feed(tail)
    we["row"] += (PAST_FEEDS - 1) * PAST_N
    assert list(we["row"]) == [(1 << 31) + (1 << 20) + r for r in (0, 700, 4990)] and wd == 0

    d = DeviceRun(trig, PAST_PARAMS, lv, cuda_device)
    xq, xt = torch.from_numpy(quiet).to(cuda_device), torch.from_numpy(tail).to(cuda_device)
    seen = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    for _ in range(PAST_FEEDS):
        d.enqueue(xq)
        seen += d.cnt                                              # on the stream of the feeds: no read-back
    assert seen.cpu().tolist() == [0, 0]
    assert d.t.rows_seen == PAST_FEEDS * PAST_N
    ge, gs, gd = d.feed(xt)
    assert d.t.rows_seen == PAST_FEEDS * PAST_N + PAST_TAIL == (1 << 31) + (1 << 20) + 5000
    assert_feeds_equal([(ge, gs, gd)], [(we, ws, wd)], "past 2^31")
    # reset: the numbering restarts at 0, where the pulse in row 0 has r < pre and is not emitted
    d.t.reset()
    assert d.t.rows_seen == 0
    h.reset()
    want = h.feed(tail)
    assert list(want[0]["row"]) == [700, 4990]
    assert_feeds_equal([d.feed(xt)], [want], "behind reset")
    d.close(), h.close()


@pytest.mark.parametrize("name,cut", [("planted", [32, 32]), ("planted_overflow", [64]), ("special", [7] * 9 + [1]),
                                      ("grid_65_0_70_100", [64, 64, 22])])
def test_feed_copies_only_what_was_emitted(trig, gsdr_lib, cuda_device, name, cut):
    """gsdr_trigger_feed returns what gsdr_trigger_feed_device leaves on the device and does not touch the host arrays
    behind n_events."""
    import torch
    case = next(c for c in CASES if c.name == name)
    want = host_feeds(trig, params(case), case.levels, case.feeds(cut))
    t = trig.device_trigger(*params(case), case.levels, device_index=0)
    S = case.pre + case.post
    for k, x in enumerate(case.feeds(cut)):
        ev = np.full(case.max_events * 6, 0x5A5A5A5A, dtype=np.uint32)
        sn = np.full(case.max_events * S * case.n_ch * 2, 0x7FD5C3C3, dtype=np.uint32)
        dropped = C.c_int(-1)
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device)
        n = gsdr_lib.gsdr_trigger_feed(t._h, xd.data_ptr(), x.shape[0], ev.ctypes.data, sn.ctypes.data, C.byref(dropped),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        we, ws, wd = want[k]
        assert n == len(we) and dropped.value == wd, (k, n, dropped.value)
        assert same_bits(ev[:6 * n].view(EVENT_DTYPE), we) and same_bits(sn[:2 * n * S * case.n_ch].view(np.complex64).reshape(ws.shape), ws)
        assert (ev[6 * n:] == 0x5A5A5A5A).all() and (sn[2 * n * S * case.n_ch:] == 0x7FD5C3C3).all()
    # the Python mirror
    t.reset()
    got = [t.feed(torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device)) for x in case.feeds(cut)]
    assert_feeds_equal(got, want, name)
    t.close()


def _int_guarded(n_words, lead_words, dev, fill=0x7FD5C3C3):
    """(whole, view): n_words int32 inside a larger int32 allocation, the view lead_words past its 512-byte-aligned start
    plus 4096 words of guard; everything filled with `fill`."""
    import torch
    whole = torch.from_numpy(np.full(8192 + n_words + 4, fill, dtype=np.uint32).view(np.int32)).to(dev)
    at = 4096 + lead_words
    return whole, whole[at:at + n_words]


@pytest.mark.parametrize("pattern,off", [("nan", 1), ("huge", 0), ("huge", 1)])
@pytest.mark.parametrize("name,cut", [("planted", [32, 32]), ("grid_65_2_4_3", [7] * 21 + [3]), ("grid_200_0_70_100", [64, 64, 22]),
                                      ("planted_overflow", [64])])
def test_extents_and_alignment(trig, gsdr_lib, cuda_device, name, cut, pattern, off):
    """Rows, events, snippets and counts as views into larger allocations between guard zones, 8-byte-only alignment (4
    for the counts): the zones stay intact and the output is that of plain tensors."""
    import torch
    case = next(c for c in CASES if c.name == name)
    want = host_feeds(trig, params(case), case.levels, case.feeds(cut))
    t = trig.device_trigger(*params(case), case.levels, device_index=0)
    S, cap = case.pre + case.post, case.max_events
    fill = np.array(OUT_SENTINEL_BITS, dtype=np.uint32).view(np.int32)
    for k, x in enumerate(case.feeds(cut)):
        if x.shape[0] == 0:
            continue
        rows_whole, rows = guarded_input(x.reshape(-1), off, pattern, cuda_device)
        sn_whole, sn = guarded_output(cap * S * case.n_ch, off, cuda_device)
        ev_whole, ev = _int_guarded(cap * 6, 2, cuda_device)              # 8 bytes past 16
        cnt_whole, cnt = _int_guarded(2, 1, cuda_device)                  # 4 bytes past 8
        assert ev.data_ptr() % 16 == 8 and cnt.data_ptr() % 8 == 4
        assert gsdr_lib.gsdr_trigger_feed_device(t._h, rows.data_ptr(), x.shape[0], ev.data_ptr(), sn.data_ptr(), cnt.data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        n, dropped = (int(v) for v in cnt.cpu().numpy())
        we, ws, wd = want[k]
        assert (n, dropped) == (len(we), wd)
        assert same_bits(ev.cpu().numpy().view(EVENT_DTYPE)[:n], we)
        assert same_bits(sn.cpu().numpy()[:n * S * case.n_ch].reshape(ws.shape), ws)
        check_input_untouched(rows_whole, x.reshape(-1), off, pattern)
        for whole, view, words in ((ev_whole, ev, cap * 6), (cnt_whole, cnt, 2)):
            w = whole.cpu().numpy()
            first = (view.data_ptr() - whole.data_ptr()) // 4
            assert (w[:first] == fill).all() and (w[first + words:] == fill).all()
        w = sn_whole.cpu().numpy().view(np.int32)
        first = (sn.data_ptr() - sn_whole.data_ptr()) // 4
        assert (w[:first] == fill).all() and (w[first + 2 * cap * S * case.n_ch:] == fill).all()
    t.close()


def test_feeds_on_a_non_default_stream(trig, cuda_device):
    import torch
    case = next(c for c in CASES if c.name == "thousand")
    s = torch.cuda.Stream()
    for cut in case.cuts:
        want = host_feeds(trig, params(case), case.levels, case.feeds(cut))
        d = DeviceRun(trig, params(case), case.levels, cuda_device, stream=s)
        xs = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device) for x in case.feeds(cut)]
        torch.cuda.synchronize()
        got = [d.feed(x) for x in xs]
        d.close()
        assert_feeds_equal(got, want, cut)


def test_set_levels_and_reset_in_stream_order(trig, cuda_device):
    import torch
    case = CASES[0]
    wide, tight = default_levels(5, off=(4,)), default_levels(5, off=(4,))
    tight["lo"][:4], tight["hi"][:4] = -1e-6, 1e-6
    p = (5, 32, 2, 4, 3, 8)
    h = trig.host_trigger(*p, wide)
    s = torch.cuda.Stream()
    d = DeviceRun(trig, p, wide, cuda_device, stream=s)
    a, b = case.rows[:32], case.rows[32:]
    got, want = [d.feed(a)], [h.feed(a)]
    d.t.set_levels(tight, stream=s)
    h.set_levels(tight)
    got.append(d.feed(b)), want.append(h.feed(b))
    assert list(want[1][0]["row"]) == [31]            # row 31 keeps the record the first feed made
    d.t.reset()
    h.reset()
    assert d.t.rows_seen == 0
    d.t.set_levels(wide, stream=s)
    h.set_levels(wide)
    for x in (a, b):
        got.append(d.feed(x)), want.append(h.feed(x))
    assert [list(e["row"]) for e, _, _ in want[2:]] == [[9, 15], [31, 47]]
    assert_feeds_equal(got, want, "levels / reset")
    d.close(), h.close()


def test_refusals_on_a_device_object(trig, gsdr_lib, cuda_device):
    import torch
    case = CASES[0]
    t = trig.device_trigger(*params(case), case.levels, device_index=0)
    x = torch.from_numpy(case.rows).to(cuda_device)
    d = DeviceRun(trig, params(case), case.levels, cuda_device)
    ev = np.zeros(case.max_events, dtype=EVENT_DTYPE)
    sn = np.zeros((case.max_events, case.pre + case.post, case.n_ch), dtype=np.complex64)
    # the host feed is refused on a device object
    assert gsdr_lib.gsdr_trigger_feed_host(t._h, case.rows.ctypes.data, 8, ev.ctypes.data, sn.ctypes.data, None) == -1
    assert "device object" in gsdr_lib.gsdr_last_error(None).decode()
    # n_rows outside [0, max_rows]: -1 and the state unchanged
    t.feed_device(x[:10], d.ev, d.sn, d.cnt)
    for n in (case.max_rows + 1, -1):
        assert gsdr_lib.gsdr_trigger_feed_device(t._h, x.data_ptr(), n, d.ev.data_ptr(), d.sn.data_ptr(), d.cnt.data_ptr(), None) == -1
        assert gsdr_lib.gsdr_last_error(None).decode().startswith("gsdr_trigger_feed_device: n_rows")
        assert t.rows_seen == 10
    # n_rows == 0: a valid feed that emits nothing and touches no row pointer
    assert gsdr_lib.gsdr_trigger_feed_device(t._h, None, 0, d.ev.data_ptr(), d.sn.data_ptr(), d.cnt.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert d.cnt.cpu().tolist() == [0, 0] and t.rows_seen == 10
    # the stream goes on as if nothing had happened
    t.feed_device(x[10:], d.ev, d.sn, d.cnt)
    torch.cuda.synchronize()
    want = host_feeds(trig, params(case), case.levels, [case.rows[:10], case.rows[10:]])[1]
    n = int(d.cnt.cpu()[0])
    assert same_bits(d.ev.cpu().numpy().view(EVENT_DTYPE)[:n], want[0]) and same_bits(d.sn[:n].cpu().numpy(), want[1])
    t.close(), d.close()


def _levels_from_baseline(base, frac=0.5):
    """Project on the direction of each channel's steady value `base`, thresholds at -/+ frac * |base| around it."""
    lv = np.zeros(len(base), dtype=LEVEL_DTYPE)
    mag = np.abs(base).astype(np.float32)
    lv["bx"], lv["by"] = base.real, base.imag
    lv["dx"], lv["dy"] = base.real / mag, base.imag / mag
    lv["lo"], lv["hi"] = -frac * mag, frac * mag
    return lv


def _behind_a_handle(trig, dev, dem, rate, freq, step_tone, step_at, n_buffers, rows_per_sample):
    """Runs n_buffers + 1 buffers of a comb through `dem` (the first one settles the filter and gives the baseline), the
    amplitude of tone `step_tone` tripled from sample `step_at` of the fed stream on; a device trigger behind
    process_device on one stream, the host twin fed the rows the device produced."""
    import torch
    from gpu_sdr_amd.source import host_tones
    L, n_ch = dem.parameters.buffer_len, len(freq)
    ampl = np.full(n_ch, 0.1, dtype=np.float32)
    high = ampl.copy()
    high[step_tone] = 0.3
    phase = np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream = torch.cuda.current_stream()
    outs = []
    t = h = None
    got, want = [], []
    for k in range(n_buffers + 1):
        x = host_tones(L, k * L, rate, freq, ampl, phase, sigma=0.0, seed=1)
        xh = host_tones(L, k * L, rate, freq, high, phase, sigma=0.0, seed=1)
        lo = min(max(step_at - (k - 1) * L, 0), L) if k >= 1 else L
        x[lo:] = xh[lo:]
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=dev)
        n = dem.process_device(torch.from_numpy(x).to(dev), out, stream=stream)
        assert n % n_ch == 0 and n > 0
        rows = out[:n].reshape(-1, n_ch)
        if k == 0:
            torch.cuda.synchronize()
            base = rows[-1].cpu().numpy()
            p = (n_ch, dem.out_capacity // n_ch, 4, 8, 8, 4)
            lv = _levels_from_baseline(base)
            t, h = DeviceRun(trig, p, lv, dev), trig.host_trigger(*p, lv)
            continue
        got.append(t.feed(rows.contiguous()))
        want.append(h.feed(rows.cpu().numpy()))
        outs.append(n // n_ch)
    t.close(), h.close()
    assert_feeds_equal(got, want, "behind a handle")
    ev = np.concatenate([e for e, _, _ in got])
    assert len(ev) == 1 and ev["channel"][0] == step_tone and ev["side"][0] == 1, ev
    expect = step_at * rows_per_sample
    return ev["row"][0], expect


def test_behind_a_direct_handle(trig, cuda_device):
    """DIRECT, 4 tones, decim 10, buffer_len 640: 64 rows per buffer, four buffers behind the one that settles the filter."""
    import gpu_sdr_amd as g
    rate, freq = 1_000_000, [100_000, -200_000, 300_000, -400_000]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=640, decim=10, pf_average=4, freq=freq,
                                          wave_type=[g.w_type.DIRECT] * 4), device_index=0)
    row, expect = _behind_a_handle(trig, cuda_device, dem, rate, freq, step_tone=2, step_at=640 + 300, n_buffers=4, rows_per_sample=0.1)
    dem.close()
    assert expect - 5 <= row <= expect + 5, (row, expect)      # within the 40-tap filter (4 rows) of the planted sample


def test_behind_a_tones_handle(trig, cuda_device):
    """TONES at frame length 64 (tones on bin centres)."""
    import gpu_sdr_amd as g
    rate, freq = 1_000_000, [0, 125_000, -250_000]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=20_001, decim=0, pf_average=4, fft_tones=64, freq=freq,
                                          wave_type=[g.w_type.TONES] * 3), device_index=0)
    row, expect = _behind_a_handle(trig, cuda_device, dem, rate, freq, step_tone=1, step_at=20_001 + 5000, n_buffers=3,
                                   rows_per_sample=1 / 64)
    dem.close()
    assert expect - 12 <= row <= expect + 12, (row, expect)    # frames are numbered from the handle's own carry; 4 frames of filter


def test_two_triggers_on_two_streams(trig, cuda_device):
    """Two objects fed concurrently on two streams give what each gives alone."""
    import torch
    ca, cb = (next(c for c in CASES if c.name == n) for n in ("every7_holdoff6", "thousand"))
    cut_a, cut_b = [1000] * 5, [1000, 0, 1, 7, 64, 928]
    want_a = host_feeds(trig, params(ca), ca.levels, ca.feeds(cut_a))
    want_b = host_feeds(trig, params(cb), cb.levels, cb.feeds(cut_b))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da = [DeviceRun(trig, params(ca), ca.levels, cuda_device, stream=sa) for _ in cut_a]     # one set of outputs per feed
    db = [DeviceRun(trig, params(cb), cb.levels, cuda_device, stream=sb) for _ in cut_b]
    xa = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device) for x in ca.feeds(cut_a)]
    xb = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda_device) for x in cb.feeds(cut_b)]
    torch.cuda.synchronize()
    # everything enqueued before anything is read: object a on stream sa, object b on stream sb, interleaved
    for k in range(max(len(xa), len(xb))):
        if k < len(xa):
            da[0].t.feed_device(xa[k], da[k].ev, da[k].sn, da[k].cnt, stream=sa)
        if k < len(xb):
            db[0].t.feed_device(xb[k], db[k].ev, db[k].sn, db[k].cnt, stream=sb)
    got_a, got_b = [d.result() for d in da], [d.result() for d in db]
    for d in da + db:
        d.close()
    assert_feeds_equal(got_a, want_a, "a")
    assert_feeds_equal(got_b, want_b, "b")
