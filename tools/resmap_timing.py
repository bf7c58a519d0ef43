"""Timing of the device resonator map (gsdr_resmap_feed_device) beside the demodulation it
follows, in one process on one GPU: python tools/resmap_timing.py [LOG]  (profiles/resmap_timing.log is its output).
RESMAP_TIMING_FEEDS=n takes n feeds instead of 200, RESMAP_TIMING_DEMOD=0 leaves the demodulators out."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402

FEEDS = int(os.environ.get("RESMAP_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("RESMAP_TIMING_DEMOD", "1") != "0"
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device resonator map beside the demodulation it follows;", torch.cuda.get_device_name(0), "; identity channel list, 16-byte aligned buffers;",
    "feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (1 launch), median / p90 of", FEEDS, "; back to back: one event pair around all of them;")
say("# every timed run is enqueued behind some tens of ms of other work, so that the device, not the host, sets the pace")
say("# bytes: 8 read and 8 written per mapped sample; GB/s: those bytes over the median and over the back-to-back time")

RATE = 200_000_000


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def resonator_rows(n_rows, n_ch, constants):
    """samples around half the cable term of each column, 1e-3 of noise: what a resonator's tone looks like"""
    rng = np.random.default_rng(1)
    n = (constants[:, 0] + 1j * constants[:, 1])[None, :]
    return (n * (0.5 + 1e-3 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch))))).astype(np.complex64)


_busy = torch.randn(8192, 8192, device=dev)


def hold_the_queue():
    """Work of some tens of milliseconds in front of a timed run: the host enqueues all its feeds meanwhile, so the
    events see the device run them back to back and not the host's pace."""
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


def time_resmap(n_ch, n_rows, kind):
    fits = [(400.0 + 0.1 * c, 0.5, 0.1, 30.0, 2e4, 1e4, 2e4, 1e3, 0.0) for c in range(n_ch)]
    constants = g.resmap_constants(fits, [(400.0 + 0.1 * c) * 1e6 for c in range(n_ch)])
    x = torch.from_numpy(resonator_rows(n_rows, n_ch, constants)).to(dev)
    m = g.device_resmap(n_ch, n_rows, constants, kind=kind, device_index=0)
    out = torch.zeros((n_rows, n_ch), dtype=torch.complex64, device=dev)
    per, back = timed(lambda: m.feed_device(x, out))
    torch.cuda.synchronize()
    mean = complex(out.mean().cpu())
    m.close()
    moved = 16 * n_rows * n_ch
    med = float(np.median(per))
    say(f"resmap  {kind:5s} {n_ch:5d} ch x {n_rows:8d} rows  median {med:8.1f} us  p90 {np.percentile(per, 90):8.1f} us  back to back {back:8.1f} us"
        f"  ({back / n_rows / n_ch * 1e3:6.3f} ns per sample)  bytes {moved / 1e6:.1f} MB  {moved / med / 1e3:7.1f} GB/s median, {moved / back / 1e3:7.1f} GB/s back to back"
        f"  mean of the last output {mean.real:.6g}{mean.imag:+.6g}j")
    return med, back


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
    for kind in ("cal", "x_dqr", "x_qr"):
        res[label, kind] = time_resmap(n_ch, n_rows, kind)
if DEMOD:
    for n_ch, n_rows, decim, L, label in SHAPES:
        try:
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   resmap feed (x_dqr) / demodulation kernel: {res[label, 'x_dqr'][1] / d:.3f} (back to back)")
log.close()
