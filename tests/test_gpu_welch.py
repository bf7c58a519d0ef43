"""The Welch accumulator on the device (include/gsdr.h, "Welch spectra on the device"): parity
with the float64 oracle of tests/_welch.py on the same float32 rows -- a handful of shapes up to 1030 channels, and the
grid of every segment kernel x every detrend x the default and a caller's window --, bit-identical output whatever the
cutting, extents, poison, a mean of exactly zero, real handles in front and the gsdr_welch_read entry.

Measured worst per-bin relative errors (bar 1e-5) are written to the file that GSDR_WELCH_MARGINS names, when it
is set; the committed copy is profiles/welch_margins.json.  They also go into the suite's parity margins (_margins.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from _extents import OUT_SENTINEL_BITS, check_input_untouched, guarded_input
from _margins import record_margin
from _welch import (GRID, GRID_SHAPES, MODES, PARITY_BAR, Oracle, cuttings, floor_ratio, grid_case, grid_precondition, grid_total,
                    grid_window, n_segments, noise_rows, rel_err, some_gain)

pytestmark = pytest.mark.gpu

WELCH_MARGINS = {}


@pytest.fixture(scope="module")
def spectrum(gsdr_lib):
    from gpu_sdr_amd import spectrum
    yield spectrum
    path = os.environ.get("GSDR_WELCH_MARGINS")
    if WELCH_MARGINS and path:
        doc = {"bar": PARITY_BAR, "metric": "max over channels, parts and bins of |psd - psd_oracle| / psd_oracle (oracle: float64)",
               "worst": max(WELCH_MARGINS.values()), "per_case": dict(sorted(WELCH_MARGINS.items(), key=lambda t: -t[1]))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


def margin(label, value):
    WELCH_MARGINS[label] = max(WELCH_MARGINS.get(label, 0.0), float(value))
    record_margin(value, label)


# name: (n_ch, nperseg, step, rows, one feed?, noise_rows arguments).  The seeds are fixed.  That of the 1030-channel
# case is chosen for the test's PRECONDITION, which looks at the input alone: with 8 segments and 2060 spectra the DC bin
# of some channel (a real chi-square of about 6 degrees of freedom around 0.17 of the mean) falls to 0.006 .. 0.012 of its
# mean for most seeds, 0.015 for this one; the others give 0.04 .. 0.18 whatever the seed.
PARITY = {
    "3x16_step16": (3, 16, 16, 16 * 12, False, {"seed": 1}),
    "3x16_step2": (3, 16, 2, 16 * 12, False, {"seed": 1}),
    "5x64": (5, 64, 32, 64 * 9, False, {"seed": 1}),
    "65x256_step100": (65, 256, 100, 256 * 10, False, {"seed": 1}),
    "1030x64": (1030, 64, 32, 300, False, {"seed": 53}),
    "2x8192": (2, 8192, 4096, 8192 * 5, False, {"seed": 1}),
    "2x8192_small_noise": (2, 8192, 4096, 8192 * 5, False, {"seed": 1, "carrier": 0.3 + 0.4j, "sigma": 1e-5, "slope": 1e-6}),
    "1x64_step8_one_feed": (1, 64, 8, 4000, True, {"seed": 1}),
}

_memo = {}


def stream_of(name):
    """(rows, oracle) of a parity case, made once and left unchanged."""
    if name not in _memo:
        n_ch, nperseg, step, rows, _, kw = PARITY[name]
        x = noise_rows(rows, n_ch, **kw)
        _memo[name] = (x, Oracle(x, nperseg, step))
    return _memo[name]


def case_of(name):
    """(n_ch, nperseg, step, rows, x, detrend, window) of a PARITY case (linear, the default window) or of the grid case
    "grid<nperseg>" (linear, Hann) / "grid<nperseg>_<detrend>_<window>" of tests/_welch.py."""
    if name in PARITY:
        n_ch, nperseg, step, rows, _, _ = PARITY[name]
        return n_ch, nperseg, step, rows, stream_of(name)[0], "linear", None
    nperseg, detrend, window = (name[4:].split("_") + ["linear", "hann"])[:3]
    nperseg = int(nperseg)
    n_ch, step = GRID_SHAPES[nperseg]
    return n_ch, nperseg, step, grid_total(nperseg), grid_case(nperseg, detrend, window)[0], detrend, grid_window(nperseg, window)


def feed_all(w, x, cut, dev, stream=None):
    import torch
    at = 0
    for n in cut:
        w.feed(torch.from_numpy(np.ascontiguousarray(x[at:at + n])).to(dev), stream=stream)
        at += n
    assert at == x.shape[0]


def read_all(w, gain, fs=1.0, stream=None):
    """psd of the four modes and the mean, as bits on the host."""
    out = {m: w.read(m, fs=fs, gain=gain if m == "gain" else None, stream=stream)[1] for m in MODES}
    out["mean"] = w.mean(stream=stream)
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_float64_oracle(spectrum, cuda_device, name):
    n_ch, nperseg, step, rows, one_feed, _ = PARITY[name]
    x, o = stream_of(name)
    assert o.n_seg == n_segments(rows, nperseg, step) >= 8
    gain = some_gain(n_ch)
    cut = [rows] if one_feed else cuttings(rows, nperseg, step)["sevens" if rows < 5000 else "several"]
    w = spectrum.device_welch(n_ch, max(cut), nperseg, step, device_index=0)
    feed_all(w, x, cut, cuda_device)
    fs = 2.0e5
    worst = 0.0
    for m in MODES:
        want = o.psd(m, fs=fs, gain=gain)
        ratio = floor_ratio(want)
        assert ratio > 0.01, (m, ratio)                  # every bin carries noise: the relative error means something on each
        f, got, n = w.read(m, fs=fs, gain=gain if m == "gain" else None)
        assert n == o.n_seg == w.segments and w.rows_seen == rows and got.dtype == np.float32
        err = rel_err(got, want)
        print(f"welch parity {name} {m}: {err:.3e} (floor ratio {ratio:.3f})")
        margin(f"{name} {m}", err)
        worst = max(worst, err)
    mean = w.mean()
    w.close()
    assert np.allclose(f, np.fft.rfftfreq(nperseg, 1 / fs))
    assert np.max(np.abs(mean - o.mean) / np.abs(o.mean)) <= 2.0 ** -23      # a double mean, each part rounded once to float32
    assert worst <= PARITY_BAR, worst


@pytest.mark.parametrize("window", ["hann", "own"])
@pytest.mark.parametrize("detrend", ["linear", "constant", "none"])
@pytest.mark.parametrize("nperseg", list(GRID_SHAPES))
def test_parity_over_the_grid(spectrum, cuda_device, nperseg, detrend, window):
    """Every instantiation of welch_segment_kernel (16 .. 8192 points: every radix plan, either result buffer, one- and
    two-level detrend sums, 1 .. 64 segments per workgroup, the LDS request above 64 KiB) x every detrend x the default
    and a caller's window (asymmetric, signed, one zero tap), against the float64 oracle at the project's bar.  What the
    case must fulfil itself -- noise in every bin, the float32 model of the contract within a third of the bar, spectra
    that differ between the variants -- is asserted without a GPU in tests/test_welch_host.py::test_grid_preconditions."""
    assert (nperseg, detrend, window) in GRID
    n_ch, step = GRID_SHAPES[nperseg]
    rows = grid_total(nperseg)
    fs = 2.0e5
    pre = grid_precondition(nperseg, detrend, window, fs=fs)
    if not pre["ok"]:
        pytest.skip(f"not a fair case (tests/test_welch_host.py::test_grid_preconditions fails on it): {pre}")
    x, o = grid_case(nperseg, detrend, window)
    assert o.n_seg == n_segments(rows, nperseg, step) >= 9
    gain = some_gain(n_ch)
    cut = cuttings(rows, nperseg, step)["sevens" if nperseg <= 1024 else "several"]
    w = spectrum.device_welch(n_ch, max(cut), nperseg, step, detrend=detrend, window=grid_window(nperseg, window), device_index=0)
    feed_all(w, x, cut, cuda_device)
    worst = 0.0
    for m in MODES:
        want = o.psd(m, fs=fs, gain=gain)
        f, got, n = w.read(m, fs=fs, gain=gain if m == "gain" else None)
        assert n == o.n_seg == w.segments and w.rows_seen == rows and got.dtype == np.float32
        err = rel_err(got, want)
        print(f"welch grid {nperseg} {detrend} {window} {m}: {err:.3e} (model {pre['model']:.3e}, floor ratio {pre['floor']:.3f})")
        margin(f"grid {nperseg} {detrend} {window} {m}", err)
        worst = max(worst, err)
    mean = w.mean()
    w.close()
    assert np.allclose(f, np.fft.rfftfreq(nperseg, 1 / fs))
    there = o.mean != 0
    assert there.all() or detrend == "none"
    assert np.max(np.abs(mean - o.mean)[there] / np.abs(o.mean)[there], initial=0.0) <= 2.0 ** -23
    assert worst <= PARITY_BAR, worst


CUTTING = ["3x16_step16", "3x16_step2", "5x64", "65x256_step100", "1030x64", "2x8192"]
# the other six kernels at the grid's channel counts and steps (linear, Hann), and 512 points -- the one size where a
# segment's slot in its workgroup changes with the cutting AND the detrend sums go through the LDS -- once more with the
# constant detrend and a caller's window
CUTTING += ["grid32", "grid128", "grid512", "grid1024", "grid2048", "grid4096", "grid512_constant_own"]


@pytest.mark.parametrize("name", CUTTING)
def test_output_does_not_depend_on_the_cutting(spectrum, cuda_device, name):
    """Device against device, bit for bit: psd of every mode and the mean."""
    import torch
    n_ch, nperseg, step, rows, x, detrend, window = case_of(name)
    gain = some_gain(n_ch)
    cuts = cuttings(rows, nperseg, step)
    if rows > 5000 if name in PARITY else nperseg >= 2048:
        cuts.pop("short"), cuts.pop("sevens")            # thousands of feeds: the other cuttings cover the long segments
        cuts["thirds"] = [rows // 3, rows // 3 + 1, rows - 2 * (rows // 3) - 1]
    ref = None
    for cname, cut in cuts.items():
        w = spectrum.device_welch(n_ch, max(max(cut), 1), nperseg, step, detrend=detrend, window=window, device_index=0)
        stream = torch.cuda.Stream() if cname in ("empties", "several") else None
        torch.cuda.synchronize()
        feed_all(w, x, cut, cuda_device, stream=stream)
        got = read_all(w, gain, stream=stream)
        w.close()
        if ref is None:
            ref = got
        assert same_bits(got, ref), cname


def test_two_objects_on_two_streams(spectrum, cuda_device):
    """Two objects fed concurrently on two streams give what each gives alone."""
    import torch
    (xa, _), (xb, _) = stream_of("5x64"), stream_of("65x256_step100")
    pa, pb = PARITY["5x64"], PARITY["65x256_step100"]
    ga, gb = some_gain(5), some_gain(65)
    alone = []
    for x, p, g in ((xa, pa, ga), (xb, pb, gb)):
        w = spectrum.device_welch(p[0], p[3], p[1], p[2], device_index=0)
        feed_all(w, x, [p[3]], cuda_device)
        alone.append(read_all(w, g))
        w.close()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    wa = spectrum.device_welch(pa[0], 128, pa[1], pa[2], device_index=0)
    wb = spectrum.device_welch(pb[0], 512, pb[1], pb[2], device_index=0)
    ta = [torch.from_numpy(np.ascontiguousarray(xa[i:i + 128])).to(cuda_device) for i in range(0, xa.shape[0], 128)]
    tb = [torch.from_numpy(np.ascontiguousarray(xb[i:i + 512])).to(cuda_device) for i in range(0, xb.shape[0], 512)]
    torch.cuda.synchronize()
    for k in range(max(len(ta), len(tb))):               # everything enqueued before anything is read, interleaved
        if k < len(ta):
            wa.feed_device(ta[k], stream=sa)
        if k < len(tb):
            wb.feed_device(tb[k], stream=sb)
    got_a, got_b = read_all(wa, ga, stream=sa), read_all(wb, gb, stream=sb)
    wa.close(), wb.close()
    assert same_bits(got_a, alone[0]) and same_bits(got_b, alone[1])


def _float_guarded(n, off_floats, dev, guard=4096):
    """(whole, view): n float32 inside one allocation of sentinel floats, `off_floats` floats past 16 bytes."""
    import torch
    whole = torch.from_numpy(np.full(2 * guard + n + 4, OUT_SENTINEL_BITS, dtype=np.uint32).view(np.float32).copy()).to(dev)
    view = whole[guard + off_floats:guard + off_floats + n]
    assert view.data_ptr() % 16 == 4 * off_floats
    return whole, view


def _guards_intact(whole, view, n):
    bits = whole.cpu().numpy().view(np.uint32)
    first = (view.data_ptr() - whole.data_ptr()) // 4
    return (bits[:first] == OUT_SENTINEL_BITS).all() and (bits[first + n:] == OUT_SENTINEL_BITS).all()


@pytest.mark.parametrize("pattern,off", [("nan", 1), ("huge", 0), ("huge", 1)])
@pytest.mark.parametrize("name", ["3x16_step2", "65x256_step100", "grid512_none_own"])
def test_extents_and_alignment(spectrum, gsdr_lib, cuda_device, name, pattern, off):
    """Rows, psd, mean and gain as views into larger allocations between guard zones, natural alignment only: the rows
    are read and not written, the zones around every output stay intact, the output is that of plain tensors.  (The
    third case: a caller's window, no detrend, the 512-point kernel.)"""
    import torch
    n_ch, nperseg, step, rows, x, detrend, window = case_of(name)
    K1 = nperseg // 2 + 1
    gain = some_gain(n_ch)
    cut = cuttings(rows, nperseg, step)["empties"]
    plain = spectrum.device_welch(n_ch, max(cut), nperseg, step, detrend=detrend, window=window, device_index=0)
    feed_all(plain, x, cut, cuda_device)
    want = read_all(plain, gain)
    plain.close()
    w = spectrum.device_welch(n_ch, max(cut), nperseg, step, detrend=detrend, window=window, device_index=0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    at = 0
    for n in cut:
        if n == 0:
            assert gsdr_lib.gsdr_welch_feed_device(w._h, None, 0, st) == 0
            continue
        part = x[at:at + n].reshape(-1)
        whole, view = guarded_input(part, off, pattern, cuda_device)
        assert gsdr_lib.gsdr_welch_feed_device(w._h, view.data_ptr(), n, st) == 0
        torch.cuda.synchronize()
        check_input_untouched(whole, part, off, pattern)
        at += n
    gain_whole, gain_view = guarded_input(gain, off, pattern, cuda_device)
    for k, m in enumerate(MODES):
        psd_whole, psd = _float_guarded(n_ch * 2 * K1, 1 + (k & 1) * 2, cuda_device)      # 4 or 12 bytes past 16
        n_seg = gsdr_lib.gsdr_welch_read_device(w._h, k, gain_view.data_ptr() if m == "gain" else None, 1.0, psd.data_ptr(), st)
        torch.cuda.synchronize()
        assert n_seg == n_segments(rows, nperseg, step)
        assert _guards_intact(psd_whole, psd, n_ch * 2 * K1), m
        assert np.array_equal(psd.cpu().numpy().view(np.uint32), want[m].reshape(-1).view(np.uint32)), m
    check_input_untouched(gain_whole, gain, off, pattern)
    mean_whole, mean = _float_guarded(2 * n_ch, 2, cuda_device)                             # 8 bytes past 16
    assert gsdr_lib.gsdr_welch_mean_device(w._h, mean.data_ptr(), st) == n_segments(rows, nperseg, step)
    torch.cuda.synchronize()
    assert _guards_intact(mean_whole, mean, 2 * n_ch)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), want["mean"].view(np.uint32))
    w.close()


def test_poison_stays_in_its_channel(spectrum, cuda_device):
    """An Inf and a NaN in channel 2 of 5: that channel is non-finite from the segment that holds them on, the other four
    keep the bits of a clean run."""
    n_ch, nperseg, step, rows, _, _ = PARITY["5x64"]
    x, _ = stream_of("5x64")
    bad = x.copy()
    bad[3 * step + 5, 2] = np.inf                         # segments 2 and 3; the mean from segment 3 on
    bad[7 * step + 1, 2] = np.nan
    gain = some_gain(n_ch)
    runs = []
    for data, cut in ((x, [rows]), (bad, [100, 27, rows - 127])):
        w = spectrum.device_welch(n_ch, rows, nperseg, step, device_index=0)
        import torch
        t = torch.from_numpy(data).to(cuda_device)
        w.feed(t[:cut[0]])
        early = read_all(w, gain) if len(cut) > 1 else None
        at = cut[0]
        for n in cut[1:]:
            w.feed(t[at:at + n])
            if at + n == 127:
                early = read_all(w, gain)                 # 127 rows: the poisoned row is in, its first segment is not complete
            at += n
        runs.append((read_all(w, gain), early))
        w.close()
    (clean, _), (got, early) = runs
    others = [0, 1, 3, 4]
    for k in list(MODES) + ["mean"]:
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k
        assert not np.isfinite(got[k][2]).any(), k
        assert np.isfinite(early[k]).all(), k


@pytest.mark.parametrize("nperseg", [512, 2048])
def test_poison_stays_in_its_channel_through_the_lds_sums(spectrum, cuda_device, nperseg):
    """The scheme of test_poison_stays_in_its_channel where the detrend sums of a segment go through the LDS (more than
    one wave per segment).  512 points, three channels: two segments share a workgroup, and a feed that completes an odd
    number of segments puts the last segment of one channel beside the first of the next -- the poisoned channel 1 sits
    beside channel 0 and beside channel 2.  2048 points, two channels: sixteen waves, two samples per thread."""
    import torch
    n_ch, step = GRID_SHAPES[nperseg]
    rows = grid_total(nperseg)
    x, _ = grid_case(nperseg, "linear", "hann")
    bad = x.copy()
    at = nperseg + 5                                      # not in segment 0, in every later segment that reaches it
    bad[at, 1] = np.inf
    bad[nperseg + 5 * step + 1, 1] = np.nan
    early_rows = at + 1                                   # the poisoned row is in, segment 1 is not complete
    assert n_segments(early_rows, nperseg, step) == 1 and n_segments(early_rows + 27, nperseg, step) == 1
    assert (n_segments(rows, nperseg, step) - 1) % 2 == 1 and at // step < n_segments(rows, nperseg, step)      # 9 segments in the last feed; the mean reaches the row
    gain = some_gain(n_ch)
    runs = []
    for data, cut in ((x, [rows]), (bad, [early_rows, 27, rows - early_rows - 27])):
        w = spectrum.device_welch(n_ch, rows, nperseg, step, device_index=0)
        t = torch.from_numpy(data).to(cuda_device)
        early, fed = None, 0
        for n in cut:
            w.feed(t[fed:fed + n])
            fed += n
            if fed == early_rows and len(cut) > 1:
                early = read_all(w, gain)
        runs.append((read_all(w, gain), early))
        w.close()
    (clean, _), (got, early) = runs
    others = [c for c in range(n_ch) if c != 1]
    for k in list(MODES) + ["mean"]:
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k
        assert not np.isfinite(got[k][1]).any(), k
        assert np.isfinite(early[k]).all(), k


def test_a_mean_of_exactly_zero_reads_with_unit_gain(spectrum, cuda_device):
    """The contract: for ROTATE and DBC a mean of exactly 0 gives g = 1.  Channel 0 of three holds multiples of 1/1024
    with rows 2i and 2i + 1 the negatives of each other, so the first `step` (even) rows of every segment sum to zero
    exactly, in double, in any order; channels 1 and 2 are noise on a carrier.  Channel 0 then reads the bits of RAW in
    both modes, and channels 1 and 2 do not: the fallback is per channel."""
    n_ch, nperseg, step = 3, 64, 32
    rows = nperseg + 9 * step + 3
    x = noise_rows(rows, n_ch, seed=4)
    rng = np.random.default_rng(8)
    k = rng.integers(-512, 513, size=(rows // 2 + 1, 2))
    pairs = (k[:, 0] + 1j * k[:, 1]) / 1024.0
    x[:, 0] = np.stack([pairs, -pairs], axis=1).reshape(-1)[:rows].astype(np.complex64)
    assert (x[0:2 * (rows // 2):2, 0] == -x[1:rows:2, 0]).all() and np.abs(x[:, 0]).max() > 0.25 and step % 2 == 0
    w = spectrum.device_welch(n_ch, rows, nperseg, step, detrend="constant", device_index=0)
    feed_all(w, x, [100, rows - 100], cuda_device)
    got = read_all(w, some_gain(n_ch))
    assert w.segments == n_segments(rows, nperseg, step) == 10
    w.close()
    assert got["mean"][0].real == 0 and got["mean"][0].imag == 0
    assert (got["mean"][1:] != 0).all()
    assert np.isfinite(got["raw"]).all() and (got["raw"] > 0).all()
    for m in ("rotate", "dbc"):
        assert np.array_equal(got[m][0].view(np.uint32), got["raw"][0].view(np.uint32)), m
    for c in (1, 2):
        assert not np.array_equal(got["rotate"][c].view(np.uint32), got["raw"][c].view(np.uint32)), c


def _behind_a_handle(spectrum, dev, dem, rate, freq, n_buffers, nperseg):
    """n_buffers buffers of a noisy comb through `dem`; a device accumulator fed straight from out_dev on the handle's
    stream, the oracle run on the same rows copied to the host.  The noise (sigma 0.02 on tones of 0.1) stands above
    what the handle's filter leaves of the other tones, so that -- as in the parity cases, and asserted in the same way
    -- every bin carries noise: a float32 transform resolves a bin 70 dB under a neighbouring line to 1e-4, not 1e-5."""
    import torch
    from gpu_sdr_amd.source import host_tones
    L, n_ch = dem.parameters.buffer_len, len(freq)
    ampl = np.full(n_ch, 0.1, dtype=np.float32)
    phase = np.linspace(0.1, 1.0, n_ch).astype(np.float32)
    stream = torch.cuda.Stream()
    w = spectrum.device_welch(n_ch, dem.out_capacity // n_ch, nperseg, device_index=0)
    outs, kept = [], []
    for k in range(n_buffers):
        x = host_tones(L, k * L, rate, freq, ampl, phase, sigma=2e-2, seed=20 + k)
        xin = torch.from_numpy(x).to(dev)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        n = dem.process_device(xin, out, stream=stream)
        assert n % n_ch == 0 and n > 0
        w.feed_device(out[:n], stream=stream)             # no wait in between: stream order
        outs.append(out), kept.append(n)
    f, got, n_seg = w.read("rotate", fs=1.0, stream=stream)
    raw = w.read("raw", fs=1.0, stream=stream)[1]
    w.close()
    rows = np.concatenate([o[:n].cpu().numpy().reshape(-1, n_ch) for o, n in zip(outs, kept)])
    o = Oracle(rows, nperseg, nperseg // 2)
    assert n_seg == o.n_seg >= 8
    for m in ("rotate", "raw"):
        assert floor_ratio(o.psd(m)) > 0.01, (m, floor_ratio(o.psd(m)))
    return max(rel_err(got, o.psd("rotate")), rel_err(raw, o.psd("raw")))


def test_behind_a_direct_handle(spectrum, cuda_device):
    """DIRECT, 8 tones, rate 1e6, buffer 50 000, decim 50: 1000 rows per buffer, four buffers, nperseg 256."""
    import gpu_sdr_amd as g
    rate = 1_000_000
    freq = [-400_000, -300_000, -200_000, -100_000, 100_000, 200_000, 300_000, 400_000]      # five output bands apart
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=50_000, decim=50, pf_average=4, freq=freq,
                                          wave_type=[g.w_type.DIRECT] * 8), device_index=0)
    err = _behind_a_handle(spectrum, cuda_device, dem, rate, freq, 4, 256)
    dem.close()
    margin("behind DIRECT", err)
    assert err <= PARITY_BAR, err


def test_behind_a_tones_handle(spectrum, cuda_device):
    """TONES at a 64-point frame (tones on bin centres), nperseg 256."""
    import gpu_sdr_amd as g
    rate, freq = 1_000_000, [0, 125_000, -250_000]
    dem = g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=40_000, decim=0, pf_average=4, fft_tones=64, freq=freq,
                                          wave_type=[g.w_type.TONES] * 3), device_index=0)
    err = _behind_a_handle(spectrum, cuda_device, dem, rate, freq, 4, 256)
    dem.close()
    margin("behind TONES", err)
    assert err <= PARITY_BAR, err


def test_read_entry_and_refusals_on_a_device_object(spectrum, gsdr_lib, cuda_device):
    """gsdr_welch_read returns what read_device left on the device; reading twice gives the same bits; a read does not
    change what later feeds accumulate; the host entries and bad arguments are refused with the state unchanged."""
    import torch
    L = gsdr_lib
    n_ch, nperseg, step, rows, _, _ = PARITY["5x64"]
    x, _ = stream_of("5x64")
    gain = some_gain(n_ch)
    K1 = nperseg // 2 + 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = torch.from_numpy(x).to(cuda_device)
    w = spectrum.device_welch(n_ch, rows, nperseg, step, device_index=0)
    psd_t = torch.full((n_ch, 2, K1), 7.0, dtype=torch.float32, device=cuda_device)
    assert w.read_device(psd_t) == 0 and w.read()[2] == 0          # before the first segment: 0, nothing written
    torch.cuda.synchronize()
    assert (psd_t == 7.0).all()
    w.feed(t[:300])
    first = read_all(w, gain)
    again = read_all(w, gain)
    assert same_bits(first, again)
    gain_t = torch.from_numpy(gain).to(cuda_device)
    for k, m in enumerate(MODES):
        assert w.read_device(psd_t, mode=m, fs=1.0, gain_t=gain_t if m == "gain" else None) == n_segments(300, nperseg, step)
        torch.cuda.synchronize()
        assert np.array_equal(psd_t.cpu().numpy().view(np.uint32), first[m].view(np.uint32)), m

    def refused(rc, entry, *names):
        msg = L.gsdr_last_error(None).decode()
        assert rc == -1 and msg.startswith(entry + ": ") and all(n in msg for n in names), (rc, msg)

    refused(L.gsdr_welch_feed_device(w._h, t.data_ptr(), -1, st), "gsdr_welch_feed_device", "n_rows")
    refused(L.gsdr_welch_feed_device(w._h, t.data_ptr(), rows + 1, st), "gsdr_welch_feed_device", "n_rows")
    refused(L.gsdr_welch_feed_device(w._h, None, 4, st), "gsdr_welch_feed_device", "rows_dev")
    refused(L.gsdr_welch_feed_host(w._h, x.ctypes.data, 4), "gsdr_welch_feed_host", "device object")
    host_psd = np.zeros((n_ch, 2, K1))
    refused(L.gsdr_welch_read_host(w._h, 0, None, 1.0, host_psd.ctypes.data, None), "gsdr_welch_read_host", "device object")
    refused(L.gsdr_welch_read_device(w._h, 0, None, 0.0, psd_t.data_ptr(), st), "gsdr_welch_read_device", "fs")
    refused(L.gsdr_welch_read_device(w._h, 9, None, 1.0, psd_t.data_ptr(), st), "gsdr_welch_read_device", "mode")
    refused(L.gsdr_welch_read_device(w._h, 3, None, 1.0, psd_t.data_ptr(), st), "gsdr_welch_read_device", "gain")
    refused(L.gsdr_welch_read_device(w._h, 0, None, 1.0, None, st), "gsdr_welch_read_device", "psd_dev")
    refused(L.gsdr_welch_mean_device(w._h, None, st), "gsdr_welch_mean_device", "mean_dev")
    assert w.rows_seen == 300
    w.feed(t[300:])
    with_reads = read_all(w, gain)
    w.reset()
    assert w.rows_seen == 0 and w.segments == 0
    w.feed(t)
    after_reset = read_all(w, gain)
    w.close()
    assert same_bits(with_reads, after_reset)
    # more (channel, segment) pairs per feed than a launch can index: refused with the size, before anything is allocated
    with pytest.raises(spectrum.GsdrError, match="gsdr_welch_create: .*MiB"):
        spectrum.device_welch(1 << 20, 1 << 20, 16, 2, device_index=0)
