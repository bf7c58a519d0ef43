"""The resonator map on the GPU (include/gsdr.h, "resonator map on the device"): the device output against the host twin
(the same bits, a NaN matching any NaN) for every kind, shape and alignment of the two pointers -- which between them
take every form of the kernel's lanes (resmap_kernels.hip: 8 bytes a sample, 16-byte stores, 16-byte loads and stores) --
with the extents of what a feed reads and writes; every value kind of tests/_resmap.py; feeds cut anywhere, empty, too
long, in place and overlapping; offsets set between feeds on one stream; a stream of the caller's; gsdr_resmap_feed; rows
of 2^20 channels whose sample index passes 2^31; and the chain of a DIRECT handle, the map and a Welch object."""
import numpy as np
import pytest

from _extents import check_input_untouched, check_output, guarded_input, guarded_output
from _resmap import KINDS, VALUE_KINDS, exact_n_constants, first_difference, fit_of, noisy_stream, same_values, value_samples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def resmap(gsdr_lib):
    from gpu_sdr_amd import resmap
    return resmap


# name: (rows, n_ch, n_out, channels or None for the identity)
SHAPES = {
    "1x1": (1, 1, 1, None),
    "3x1": (3, 1, 1, None),
    "7x3": (7, 3, 3, None),
    "5x3to2": (5, 3, 2, [2, 0]),
    "257x64to5": (257, 64, 5, [63, 0, 7, 7, 31]),
    "65x7": (65, 7, 7, None),
    "1030x3": (1030, 3, 3, None),
    "2x2048": (2, 2048, 2048, None),
    "262144x4": (262144, 4, 4, None),
}

_memo = {}


def case_of(resmap, name):
    """(rows complex64 [n][n_ch], constants [n_out][7]) of a shape, made once and left unchanged.  The resonators repeat
    with period 16 across the columns: a case takes the time of 16 streams, whatever its width."""
    if name not in _memo:
        n, n_ch, n_out, channels = SHAPES[name]
        rng = np.random.default_rng(3)
        fits, tones = zip(*[fit_of(rng) for _ in range(min(n_ch, 16))])
        streams = np.stack([noisy_stream(rng, f, t, n)[0] for f, t in zip(fits, tones)], axis=1)
        rows = np.ascontiguousarray(np.tile(streams, (1, -(-n_ch // 16)))[:, :n_ch])
        k_in = np.tile(resmap.resmap_constants(fits, tones), (-(-n_ch // 16), 1))[:n_ch]
        _memo[name] = (rows, np.ascontiguousarray(k_in if channels is None else k_in[channels]))
    return _memo[name]


def twin_of(resmap, name, kind, offsets=None):
    key = (name, kind, None if offsets is None else offsets.tobytes())
    if key not in _memo:
        n, n_ch, n_out, channels = SHAPES[name]
        rows, k = case_of(resmap, name)
        h = resmap.host_resmap(n_ch, n, k, channels=channels, kind=kind)
        if offsets is not None:
            h.set_offsets(offsets)
        _memo[key] = h.feed(rows)
        h.close()
    return _memo[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_host_twin_in_guarded_buffers(resmap, gsdr_lib, cuda_device, name, kind):
    """Input and output in the middle of larger allocations, each on a 16-byte boundary or 8 bytes past one: the feed
    reads rows_dev[0, n_rows n_ch) only, writes out_dev[0, n_rows n_out) only and leaves the input as it was."""
    import torch
    n, n_ch, n_out, channels = SHAPES[name]
    rows, k = case_of(resmap, name)
    want = twin_of(resmap, name, kind)
    assert want.shape == (n, n_out) and np.all(np.isfinite(want.view(np.float32)))
    d = resmap.device_resmap(n_ch, n, k, channels=channels, kind=kind, device_index=0)
    for in_off, out_off, pattern in ((0, 0, "nan"), (1, 0, "huge"), (0, 1, "huge"), (1, 1, "nan")):
        whole_in, view_in = guarded_input(rows.reshape(-1), in_off, pattern, cuda_device)
        whole_out, view_out = guarded_output(n * n_out, out_off, cuda_device)
        assert gsdr_lib.gsdr_resmap_feed_device(d._h, view_in.data_ptr(), n, view_out.data_ptr(), None) == n
        torch.cuda.synchronize()
        check_output(whole_out, view_out, n * n_out)
        check_input_untouched(whole_in, rows.reshape(-1), in_off, pattern)
        got = view_out.cpu().numpy().reshape(n, n_out)
        assert same_values(got, want), (in_off, out_off, first_difference(got, want))
    d.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_value_kind(resmap, cuda_device, kind):
    """Ordinary samples, float32 denormals, 1e38, Inf, NaN and samples equal to the cable term, in one feed of 6 columns x
    240 rows and in one of 240 columns' worth of the same rows laid out 4 wide (the 16-byte lanes)."""
    import torch
    n = 240
    rng = np.random.default_rng(17)
    fits, tones = zip(*[fit_of(rng) for _ in VALUE_KINDS])
    k = resmap.resmap_constants(fits, tones)
    rows = np.zeros((n, len(VALUE_KINDS)), dtype=np.complex64)
    for c, vk in enumerate(VALUE_KINDS):
        if vk == "equal_n":
            k[c], n32 = exact_n_constants(k[c], fits[c], tones[c])
            rows[:, c] = n32
            rows[1::2, c] = np.nextafter(np.float32(n32.real), np.float32(np.inf)) + 1j * np.float32(n32.imag)
        else:
            rows[:, c] = value_samples(vk, fits[c], tones[c], n, seed=200 + c)
    h = resmap.host_resmap(6, n, k, kind=kind)
    want = h.feed(rows)
    h.close()
    assert np.isnan(want.view(np.float32)).any() or kind == "cal"
    d = resmap.device_resmap(6, n, k, kind=kind, device_index=0)
    got = d.feed(torch.from_numpy(rows).to(cuda_device))
    d.close()
    assert same_values(got, want), first_difference(got, want)
    # the same samples through the paired lanes: 4 columns that all carry column c's constants, n / 4 rows
    for c in range(len(VALUE_KINDS)):
        k4 = np.tile(k[c], (4, 1))
        d = resmap.device_resmap(4, n // 4, k4, kind=kind, device_index=0)
        got = d.feed(torch.from_numpy(np.ascontiguousarray(rows[:, c])).to(cuda_device))
        d.close()
        assert same_values(got.reshape(-1), want[:, c]), (VALUE_KINDS[c], first_difference(got.reshape(-1), want[:, c]))


@pytest.mark.parametrize("name", ["65x7", "1030x3", "257x64to5"])
def test_a_feed_cut_anywhere_gives_the_same_rows(resmap, cuda_device, name):
    import torch
    n, n_ch, n_out, channels = SHAPES[name]
    rows, k = case_of(resmap, name)
    want = twin_of(resmap, name, "x_dqr")
    xd = torch.from_numpy(rows).to(cuda_device)
    d = resmap.device_resmap(n_ch, n, k, channels=channels, kind="x_dqr", device_index=0)
    for cut in ([1] * 9 + [n - 9], [0, n // 2, 0, n - n // 2], [n - 1, 1], [7] * (n // 7) + [n % 7]):
        out = torch.zeros((n, n_out), dtype=torch.complex64, device=cuda_device)
        at = 0
        for m in cut:
            assert d.feed_device(xd[at:at + m], out[at:at + m]) == m
            at += m
        torch.cuda.synchronize()
        assert at == n and same_values(out.cpu().numpy(), want), cut[:3]
    d.close()


def test_empty_feeds_long_feeds_in_place_and_overlap(resmap, gsdr_lib, cuda_device):
    import torch
    from gpu_sdr_amd import GsdrError
    n, n_ch, n_out, _ = SHAPES["65x7"]
    rows, k = case_of(resmap, "65x7")
    want = twin_of(resmap, "65x7", "x_qr")
    L = gsdr_lib
    d = resmap.device_resmap(n_ch, n, k, kind="x_qr", device_index=0)
    xd = torch.from_numpy(rows).to(cuda_device)
    out = torch.zeros((n + 1, n_out), dtype=torch.complex64, device=cuda_device)
    assert L.gsdr_resmap_feed_device(d._h, None, 0, None, None) == 0                # touches no pointer
    assert d.feed_device(xd[:0], out) == 0
    with pytest.raises(GsdrError, match=r"gsdr_resmap_feed_device: .*n_rows"):
        d.feed_device(torch.cat([xd, xd[:1]]), out)
    assert L.gsdr_resmap_feed_device(d._h, xd.data_ptr(), -1, out.data_ptr(), None) == -1
    assert L.gsdr_resmap_feed(d._h, xd.data_ptr(), n + 1, rows.ctypes.data, None) == -1
    assert L.gsdr_resmap_feed_device(d._h, None, 1, out.data_ptr(), None) == -1 and "rows_dev" in L.gsdr_last_error(None).decode()
    assert L.gsdr_resmap_feed_device(d._h, xd.data_ptr(), 1, None, None) == -1 and "out_dev" in L.gsdr_last_error(None).decode()
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                              # no refusal wrote anything
    assert d.feed_device(xd, out) == n                                              # and the object works as before
    torch.cuda.synchronize()
    assert same_values(out[:n].cpu().numpy(), want)
    # in place with the identity list, at both alignments (7 columns: row 1 starts 8 bytes past a 16-byte boundary)
    for first in (0, 1):
        io = xd.clone()
        assert d.feed_device(io[first:], io[first:]) == n - first
        torch.cuda.synchronize()
        assert same_values(io[first:].cpu().numpy(), want[first:]) and same_values(io[:first].cpu().numpy(), rows[:first])
    # (and through the 16-byte lanes: an even row length on aligned pointers)
    n2, n_ch2, _, _ = SHAPES["2x2048"]
    rows2, k2 = case_of(resmap, "2x2048")
    d2 = resmap.device_resmap(n_ch2, n2, k2, kind="x_qr", device_index=0)
    io = torch.from_numpy(rows2).to(cuda_device)
    assert io.data_ptr() % 16 == 0 and d2.feed_device(io, io) == n2
    torch.cuda.synchronize()
    d2.close()
    assert same_values(io.cpu().numpy(), twin_of(resmap, "2x2048", "x_qr"))
    # any other overlap of the two extents is refused and nothing is written
    io = torch.cat([xd, xd])
    before = io.cpu().numpy()
    for a, b in ((0, 1), (1, 0), (0, n - 1), (n - 1, 0)):
        assert L.gsdr_resmap_feed_device(d._h, io[a:].data_ptr(), n, io[b:].data_ptr(), None) == -1
        assert "overlaps" in L.gsdr_last_error(None).decode()
    assert L.gsdr_resmap_feed_device(d._h, io.data_ptr(), n, io[n:].data_ptr(), None) == n      # adjacent extents do not overlap
    torch.cuda.synchronize()
    after = io.cpu().numpy()
    assert same_values(after[:n], before[:n]) and same_values(after[n:], want)
    d.close()
    # a list that is not the identity: out == rows is refused too, also where the list is a permutation
    for channels in ([6, 5, 4, 3, 2, 1, 0], [0, 1, 2]):
        g = resmap.device_resmap(n_ch, n, k[channels], channels=channels, kind="cal", device_index=0)
        io = xd.clone()
        assert L.gsdr_resmap_feed_device(g._h, io.data_ptr(), n, io.data_ptr(), None) == -1 and "overlaps" in L.gsdr_last_error(None).decode()
        assert L.gsdr_resmap_feed_device(g._h, io.data_ptr(), n, io[1:].data_ptr(), None) == -1
        torch.cuda.synchronize()
        assert same_values(io.cpu().numpy(), rows)
        g.close()
    # the identity written out is the identity
    g = resmap.device_resmap(n_ch, n, k, channels=list(range(n_ch)), kind="x_qr", device_index=0)
    io = xd.clone()
    assert g.feed_device(io, io) == n
    torch.cuda.synchronize()
    assert same_values(io.cpu().numpy(), want)
    g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_offsets_between_feeds_on_a_stream_of_the_callers(resmap, cuda_device, kind):
    """feed, set_offsets, feed, set_offsets, feed, set_offsets(None), feed on one stream with no wait in between: each
    feed sees the offsets set before it.  Then gsdr_resmap_feed, which copies to the host."""
    import torch
    name = "1030x3"
    n, n_ch, n_out, _ = SHAPES[name]
    rows, k = case_of(resmap, name)
    plain = twin_of(resmap, name, kind).astype(np.complex128)
    off_a = np.stack([plain.real.mean(axis=0), plain.imag.mean(axis=0)], axis=1)
    off_b = off_a * (1 + 2.0 ** -20) + 1e-3
    d = resmap.device_resmap(n_ch, n, k, kind=kind, device_index=0)
    xd = torch.from_numpy(rows).to(cuda_device)
    outs = [torch.zeros((n, n_out), dtype=torch.complex64, device=cuda_device) for _ in range(4)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    d.feed_device(xd, outs[0], stream=stream)
    d.set_offsets(off_a, stream=stream)
    d.feed_device(xd, outs[1], stream=stream)
    d.set_offsets(off_b, stream=stream)
    d.feed_device(xd, outs[2], stream=stream)
    d.set_offsets(None, stream=stream)
    d.feed_device(xd, outs[3], stream=stream)
    assert np.array_equal(d.offsets, np.zeros((n_out, 2)))
    stream.synchronize()
    for out, off in zip(outs, (None, off_a, off_b, None)):
        want = twin_of(resmap, name, kind, off)
        assert same_values(out.cpu().numpy(), want), first_difference(out.cpu().numpy(), want)
    assert not same_values(twin_of(resmap, name, kind, off_a), twin_of(resmap, name, kind, off_b))
    d.set_offsets(off_b, stream=stream)
    parts = [d.feed(xd[:500], stream=stream).copy(), d.feed(xd[500:], stream=stream).copy(), d.feed(xd[:0], stream=stream)]
    d.close()
    assert same_values(np.concatenate(parts), twin_of(resmap, name, kind, off_b))


def test_rows_of_2_to_the_20_channels(resmap, gsdr_lib, cuda_device):
    """n_ch = 2^20, 2 049 rows, three picked columns: the sample index of the last row passes 2^31.  The input is
    torch.empty (about 17 GB), only the picked columns are written; the twin maps the same three streams laid side by
    side."""
    import torch
    n_ch, n, channels = 1 << 20, 2049, [0, 524287, (1 << 20) - 1]
    rng = np.random.default_rng(29)
    fits, tones = zip(*[fit_of(rng) for _ in channels])
    k = resmap.resmap_constants(fits, tones)
    cols = np.stack([noisy_stream(rng, f, t, n)[0] for f, t in zip(fits, tones)], axis=1)
    try:
        xd = torch.empty((n, n_ch), dtype=torch.complex64, device=cuda_device)
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:      # the allocation itself was refused
        if "out of memory" not in str(e).lower():
            raise
        pytest.skip(f"no room for {n * n_ch * 8 / 2 ** 30:.0f} GiB of rows on this device")
    cd = torch.from_numpy(cols).to(cuda_device)
    for j, c in enumerate(channels):
        xd[:, c] = cd[:, j]
    assert (n - 1) * n_ch + channels[-1] > 1 << 31
    for kind in KINDS:
        h = resmap.host_resmap(3, n, k, kind=kind)
        want = h.feed(cols)
        h.close()
        d = resmap.device_resmap(n_ch, n, k, channels=channels, kind=kind, device_index=0)
        out = torch.zeros((n, 3), dtype=torch.complex64, device=cuda_device)
        assert d.feed_device(xd, out) == n
        torch.cuda.synchronize()
        d.close()
        assert same_values(out.cpu().numpy(), want), (kind, first_difference(out.cpu().numpy(), want))
    del xd
    torch.cuda.empty_cache()


def test_handle_resmap_welch_chain(resmap, cuda_device):
    """DIRECT, 8 tones, decim 50, buffer 50 000: 1000 rows per buffer, four buffers.  The handle's output buffer goes
    straight into the map (5 of the 8 tones, x_dqr, offsets from a first estimate) and its output into a Welch object in
    'raw' mode, all on one stream with no wait in between.  The spectra are those of a Welch object fed the twin's rows."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import host_tones
    rate, L, n_ch = 1_000_000, 50_000, 8
    freq = [-400_000, -300_000, -200_000, -100_000, 100_000, 200_000, 300_000, 400_000]
    channels = [1, 2, 4, 6, 7]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=L, decim=50, pf_average=4, freq=freq,
                                          wave_type=[g.w_type.DIRECT] * n_ch), device_index=0)
    max_rows = dem.out_capacity // n_ch
    rng = np.random.default_rng(37)
    fits, tones = zip(*[fit_of(rng) for _ in channels])
    k = resmap.resmap_constants(fits, tones)
    offsets = np.stack([np.linspace(10.0, 50.0, 5), 1.0 / np.array([f[5] for f in fits])], axis=1)
    m = resmap.device_resmap(n_ch, max_rows, k, channels=channels, kind="x_dqr", device_index=0)
    w = g.device_welch(len(channels), max_rows, 64, device_index=0)
    ampl, phase = np.full(n_ch, 0.1, dtype=np.float32), np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream = torch.cuda.Stream()
    m.set_offsets(offsets, stream=stream)
    outs, kept, mapped = [], [], []
    for b in range(4):
        xin = torch.from_numpy(host_tones(L, b * L, rate, freq, ampl, phase, sigma=2e-2, seed=40 + b)).to(cuda_device)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        y = torch.empty((max_rows, len(channels)), dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        n = dem.process_device(xin, out, stream=stream)
        assert n % n_ch == 0 and n > 0
        assert m.feed_device(out[:n], y, stream=stream) == n // n_ch
        w.feed_device(y[:n // n_ch], stream=stream)
        outs.append(out), kept.append(n), mapped.append(y)
    _, psd, n_seg = w.read("raw", fs=rate / 50 / 4, stream=stream)
    rows = [o[:n].cpu().numpy().reshape(-1, n_ch) for o, n in zip(outs, kept)]
    got = np.concatenate([y[:n // n_ch].cpu().numpy() for y, n in zip(mapped, kept)])
    m.close(), w.close(), dem.close()
    h = resmap.host_resmap(n_ch, max_rows, k, channels=channels, kind="x_dqr")
    h.set_offsets(offsets)
    twin = [h.feed(r) for r in rows]
    h.close()
    assert got.shape == (4000, 5) and same_values(got, np.concatenate(twin)) and np.all(np.isfinite(got.view(np.float32)))
    w2 = g.device_welch(len(channels), max_rows, 64, device_index=0)
    for t in twin:
        w2.feed_device(torch.from_numpy(t).to(cuda_device))
    _, psd2, n_seg2 = w2.read("raw", fs=rate / 50 / 4)
    w2.close()
    assert n_seg == n_seg2 == (4000 - 64) // 32 + 1 and np.all(np.isfinite(psd)) and psd.max() > 0
    assert np.array_equal(psd.view(np.int32), psd2.view(np.int32))
