"""Timing of the device FIR decimator (gsdr_decim_feed_device) beside the demodulation it
follows and the Welch feed at the same shape, in one process on one GPU: python tools/decim_timing.py [LOG]
(profiles/decim_timing.log is its output).  DECIM_TIMING_FEEDS=n takes n feeds instead of 200, DECIM_TIMING_DEMOD=0
leaves the demodulators and the Welch feeds out."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402

FEEDS = int(os.environ.get("DECIM_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("DECIM_TIMING_DEMOD", "1") != "0"
Q = 100
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device FIR decimator beside the demodulation it follows;", torch.cuda.get_device_name(0), "; q", Q, "default taps (", 20 * Q + 1,
    "taps, 21 chunks per output) ; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (2 launches), median / p90 of", FEEDS, "; amortised: one event pair around all of them;")
say("# every timed run is enqueued behind some tens of ms of other work, so that the device, not the host, sets the pace")
say("# bytes: the rows a feed must read plus the rows it must write, once each; GB/s: those bytes over the median")

RATE = 200_000_000


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def noise_rows(n_rows, n_ch):
    rng = np.random.default_rng(1)
    return (1.0 + 1e-3 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))).astype(np.complex64)


_busy = torch.randn(8192, 8192, device=dev)


def hold_the_queue():
    """Work of some tens of milliseconds in front of a timed run: the host enqueues all its feeds meanwhile, so the
    events see the device run them back to back and not the host's pace (some 50 us of Python and launches per feed,
    which is what the events measured on an empty queue, whatever the shape)."""
    for _ in range(6):
        torch.mm(_busy, _busy)


def timed(feed):
    for _ in range(WARM):
        feed()
    torch.cuda.synchronize()
    a, b = events(FEEDS), events(FEEDS)
    hold_the_queue()
    for k in range(FEEDS):
        a[k].record()
        feed()
        b[k].record()
    torch.cuda.synchronize()
    per = np.array([a[k].elapsed_time(b[k]) for k in range(FEEDS)]) * 1e3
    s, e = events(2)
    hold_the_queue()
    s.record()
    for k in range(FEEDS):
        feed()
    e.record()
    torch.cuda.synchronize()
    return per, s.elapsed_time(e) * 1e3 / FEEDS


def time_decim(n_ch, n_rows):
    rows = noise_rows(n_rows, n_ch)
    x = torch.from_numpy(rows).to(dev)
    d = g.device_decimator(n_ch, n_rows, Q, device_index=0)
    out = torch.zeros((d.out_capacity, n_ch), dtype=torch.complex64, device=dev)
    emitted = []
    per, amort = timed(lambda: emitted.append(d.feed_device(x, out)))
    torch.cuda.synchronize()
    mean = complex(out[:emitted[-1]].mean().cpu())
    moved = rows.nbytes + emitted[-1] * n_ch * 8
    d.close()
    med = float(np.median(per))
    say(f"decim   {n_ch:5d} ch x {n_rows:8d} rows  median {med:8.1f} us  p90 {np.percentile(per, 90):8.1f} us  amortised {amort:8.1f} us"
        f"  ({amort / n_rows / n_ch * 1e3:6.3f} ns per sample, {emitted[-1]} rows out per feed)  bytes {moved / 1e6:.1f} MB  {moved / med / 1e3:7.1f} GB/s"
        f"  mean of the last output {mean.real:.4f}{mean.imag:+.4f}j")
    return med, amort


def time_welch(n_ch, n_rows):
    x = torch.from_numpy(noise_rows(n_rows, n_ch)).to(dev)
    w = g.device_welch(n_ch, n_rows, 1024, 512, device_index=0)
    per, amort = timed(lambda: w.feed_device(x))
    w.close()
    say(f"welch   {n_ch:5d} ch x {n_rows:8d} rows  median {np.median(per):8.1f} us  p90 {np.percentile(per, 90):8.1f} us  amortised {amort:8.1f} us"
        f"  (nperseg 1024 step 512, the same box and process)")


def time_demod(n_ch, decim, L, label):
    freq, ampl, phase = tone_comb(n_ch, RATE, seed=1)
    p = g.param(mode="RX", rate=RATE, buffer_len=L, decim=decim, pf_average=4, freq=[int(f) for f in freq],
                wave_type=[g.w_type.DIRECT] * n_ch)
    dem = g.RX_buffer_demodulator(p, device_index=0)
    x = torch.randn(L, dtype=torch.complex64, device=dev) * 0.1
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=dev)
    for _ in range(5):
        n = dem.process(x, out)
    torch.cuda.synchronize()
    dem.profile_enable(True)
    for _ in range(30):
        n = dem.process(x, out)
    torch.cuda.synchronize()
    k, ms = dem.profile_read()
    name = dem.kernel_name
    dem.close()
    say(f"demod   {label}: {name}  {ms / max(k, 1) * 1e3:8.1f} us per buffer ({k} timed launches), {n // n_ch} rows x {n_ch} ch per buffer")
    return ms / max(k, 1) * 1e3


SHAPES = [(2048, 1000, 1000, 1_000_000, "DIRECT 2048 tones decim 1000 L 1e6"),
          (256, 10000, 100, 1_000_000, "DIRECT 256 tones decim 100 L 1e6"),
          (4, 1 << 20, 0, 1 << 20, "DIRECT 4 tones undecimated L 2^20")]
res = {}
for n_ch, n_rows, decim, L, label in SHAPES:
    res[label] = time_decim(n_ch, n_rows)
if DEMOD:
    for n_ch, n_rows, decim, L, label in SHAPES:
        try:
            time_welch(n_ch, n_rows)
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   decimator feed / demodulation kernel: {res[label][1] / d:.3f} (amortised)")
log.close()
