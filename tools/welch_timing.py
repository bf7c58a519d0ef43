"""Timing of the device Welch accumulator (gsdr_welch_feed_device / _read_device) beside the
demodulation it follows, in one process on one GPU: python tools/welch_timing.py [LOG]  (profiles/welch_timing.log is
its output).  WELCH_TIMING_FEEDS=n takes n feeds instead of 200, WELCH_TIMING_DEMOD=0 leaves the demodulators out."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402

FEEDS = int(os.environ.get("WELCH_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("WELCH_TIMING_DEMOD", "1") != "0"
NPERSEG, STEP = 1024, 512
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device Welch accumulator beside the demodulation it follows;", torch.cuda.get_device_name(0), "; nperseg", NPERSEG, "step", STEP,
    "; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (3 launches), median / p90 of", FEEDS, "; amortised: one event pair around all of them")

RATE = 200_000_000


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def time_welch(n_ch, n_rows):
    rng = np.random.default_rng(1)
    rows = (1.0 + 1e-3 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))).astype(np.complex64)
    x = torch.from_numpy(rows).to(dev)
    w = g.device_welch(n_ch, n_rows, NPERSEG, STEP, device_index=0)
    psd = torch.zeros((n_ch, 2, NPERSEG // 2 + 1), dtype=torch.float32, device=dev)
    for _ in range(WARM):
        w.feed_device(x)
    torch.cuda.synchronize()
    a, b = events(FEEDS), events(FEEDS)
    for k in range(FEEDS):
        a[k].record()
        w.feed_device(x)
        b[k].record()
    torch.cuda.synchronize()
    per = np.array([a[k].elapsed_time(b[k]) for k in range(FEEDS)]) * 1e3
    s, e = events(2)
    s.record()
    for k in range(FEEDS):
        w.feed_device(x)
    e.record()
    torch.cuda.synchronize()
    amort = s.elapsed_time(e) * 1e3 / FEEDS
    reads = 50
    a, b = events(reads), events(reads)
    for k in range(reads):
        a[k].record()
        n_seg = w.read_device(psd, mode="rotate", fs=1.0)
        b[k].record()
    torch.cuda.synchronize()
    rd = np.array([a[k].elapsed_time(b[k]) for k in range(reads)]) * 1e3
    # the spectrum of unit-variance-scaled white noise: the mean density over the inner bins is 2 sigma^2 / fs
    flat = float(psd[:, :, 8:-8].mean().cpu()) / (2 * 1e-6)
    segs_per_feed = n_rows / STEP
    w.close()
    say(f"welch   {n_ch:5d} ch x {n_rows:8d} rows  median {np.median(per):8.1f} us  p90 {np.percentile(per, 90):8.1f} us  amortised {amort:8.1f} us"
        f"  ({amort / n_rows / n_ch * 1e3:6.3f} ns per sample, {segs_per_feed:7.1f} segments per channel and feed)  read_device median {np.median(rd):6.1f} us"
        f"  segments {n_seg}  density / (2 sigma^2) {flat:.4f}  bytes in {rows.nbytes / 1e6:.1f} MB")
    return float(np.median(per)), amort


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
    reps = 30
    for _ in range(reps):
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
    res[label] = time_welch(n_ch, n_rows)
if DEMOD:
    for n_ch, n_rows, decim, L, label in SHAPES:
        try:
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   welch feed / demodulation kernel: {res[label][1] / d:.3f} (amortised)")
log.close()
