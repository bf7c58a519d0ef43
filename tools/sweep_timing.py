"""Timing of the device sweep accumulator (gsdr_sweep_feed_device) beside the chirp kernels it
follows, in one process on one GPU: python tools/sweep_timing.py [LOG] (profiles/sweep_timing.log is its output).
SWEEP_TIMING_FEEDS=n takes n feeds instead of 200, SWEEP_TIMING_DEMOD=0 leaves the demodulators out."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402

FEEDS = int(os.environ.get("SWEEP_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("SWEEP_TIMING_DEMOD", "1") != "0"
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device sweep accumulator beside the chirp kernel it follows;", torch.cuda.get_device_name(0), "; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (1 launch), median / p90 of", FEEDS, "; amortised: one event pair around all of them;")
say("# every timed run is enqueued behind some tens of ms of other work, so that the device, not the host, sets the pace")
say("# bytes: the rows a feed must read, once, plus the 32-byte accumulators it touches, read and written; GB/s: those bytes over the median")

RATE, STEPS, CHIRP_T, L = 200_000_000, 1_000_000, 1.0, 1_000_000          # C4: 200 samples per point, 5 000 points per buffer


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


_busy = torch.randn(8192, 8192, device=dev)


def hold_the_queue():
    """Work of some tens of milliseconds in front of a timed run: the host enqueues all its feeds meanwhile, so the
    events see the device run them back to back and not the host's pace."""
    for _ in range(6):
        torch.mm(_busy, _busy)


def timed(call, count=FEEDS):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    a, b = events(count), events(count)
    hold_the_queue()
    for k in range(count):
        a[k].record()
        call()
        b[k].record()
    torch.cuda.synchronize()
    per = np.array([a[k].elapsed_time(b[k]) for k in range(count)]) * 1e3
    s, e = events(2)
    hold_the_queue()
    s.record()
    for k in range(count):
        call()
    e.record()
    torch.cuda.synchronize()
    return per, s.elapsed_time(e) * 1e3 / count


def time_sweep(n_ch, n_rows, n_points, group, label):
    rng = np.random.default_rng(1)
    rows = (1.0 + 1e-3 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))).astype(np.complex64)
    x = torch.from_numpy(rows).to(dev)
    s = g.device_sweep(n_ch, n_points, group, 0, device_index=0)
    per, amort = timed(lambda: s.feed_device(x))
    touched = min(-(-n_rows // group), n_points)
    moved = rows.nbytes + touched * n_ch * 64
    med = float(np.median(per))
    say(f"sweep   {n_ch:3d} ch x {n_rows:8d} rows  n_points {n_points} group {group:4d}  median {med:8.1f} us  p90 {np.percentile(per, 90):8.1f} us"
        f"  amortised {amort:8.1f} us  bytes {moved / 1e6:.2f} MB  {moved / med / 1e3:7.1f} GB/s  ({label}; {s.rows_seen} rows fed, {s.sweeps} sweeps)")
    mean = torch.zeros((n_points, n_ch), dtype=torch.complex64, device=dev)
    var = torch.zeros((n_points, n_ch), dtype=torch.complex64, device=dev)
    per_r, amort_r = timed(lambda: s.read_device(mean, var), 50)
    moved_r = n_points * n_ch * (32 + 16)
    say(f"read    {n_ch:3d} ch x {n_points} points, mean and variance  median {np.median(per_r):8.1f} us  amortised {amort_r:8.1f} us"
        f"  bytes {moved_r / 1e6:.1f} MB  {moved_r / np.median(per_r) / 1e3:7.1f} GB/s")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        d = s.slope()
    dt = (time.perf_counter() - t0) / 20 * 1e6
    say(f"slope   {n_ch:3d} ch x {n_points} points  {dt:8.1f} us per call (host clock: two launches, the wait and the copy of {n_ch} complex128);"
        f" arg D[0] {np.angle(d[0]):+.3e}")
    s.close()
    return med, amort


def time_demod(n_ch, decim, label):
    bands = [(-90_000_000 + 1_000_000 * c, 90_000_000 - 1_000_000 * c) for c in range(n_ch)]
    p = g.param(mode="RX", rate=RATE, buffer_len=L, decim=decim, freq=[b[0] for b in bands], chirp_f=[b[1] for b in bands],
                swipe_s=[STEPS], chirp_t=[CHIRP_T], wave_type=[g.w_type.CHIRP] * n_ch)
    dem = g.RX_buffer_demodulator(p, device_index=0, multi_chirp=n_ch > 1)
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


# rows x channels per feed, n_points, group, the handle's decim, note
SHAPES = [(1, 5_000, 1_000_000, 1, 1, "C4: lock-in rows, one chirp"),
          (16, 5_000, 1_000_000, 1, 1, "lock-in rows, 16 chirps"),
          (1, 1_000_000, 1_000_000, 200, 0, "undecimated, one chirp"),
          (4, 1_000_000, 1_000_000, 200, 0, "undecimated, 4 chirps")]
res = {}
for n_ch, n_rows, n_points, group, decim, label in SHAPES:
    res[label] = time_sweep(n_ch, n_rows, n_points, group, label)
if DEMOD:
    for n_ch, n_rows, n_points, group, decim, label in SHAPES:
        try:
            d = time_demod(n_ch, decim, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   sweep feed / chirp kernel: {res[label][1] / d:.3f} (amortised)")
log.close()
