"""Timing of the device row statistics (gsdr_stats_feed_device) beside the demodulation they
follow and the Welch and resmap feeds of the same shape, in one process on one GPU:
python tools/stats_timing.py [LOG]  (profiles/stats_timing.log is its output).
STATS_TIMING_FEEDS=n takes n feeds instead of 200, STATS_TIMING_DEMOD=0 leaves the demodulators out."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402
from gpu_sdr_amd.trigger import LEVEL_DTYPE  # noqa: E402

FEEDS = int(os.environ.get("STATS_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("STATS_TIMING_DEMOD", "1") != "0"
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device row statistics beside the demodulation they follow and the Welch and resmap feeds of the same shape;", torch.cuda.get_device_name(0),
    "; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (1 launch), median / p90 of", FEEDS, "; back to back: one event pair around all of them;")
say("# every timed run is enqueued behind some tens of ms of other work, so that the device, not the host, sets the pace;")
say("# the stats, Welch and resmap runs of a shape alternate (stats, welch, resmap, stats, ...): the figure is the median over the runs of a kind")
say("# bytes: 8 read per sample (the rows of a feed); GB/s: those bytes over the back-to-back time")

RATE = 200_000_000
ROUNDS = 3


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


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
    return float(np.median(per)), float(np.percentile(per, 90)), s.elapsed_time(e) * 1e3 / FEEDS


def noise_rows(n_rows, n_ch):
    """unit Gaussian noise on a per-channel baseline: the range of the axes is -/+ 8 sigma around it"""
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.linspace(-1.0, 1.0, n_ch, device=dev)
    x = torch.randn((n_rows, n_ch, 2), generator=gen, device=dev) * 0.05
    x[..., 0] += base
    axes = np.zeros(n_ch, dtype=LEVEL_DTYPE)
    axes["dx"] = 1
    axes["lo"], axes["hi"] = base.cpu().numpy() - 0.4, base.cpu().numpy() + 0.4
    return torch.view_as_complex(x).contiguous(), axes


def time_shape(n_ch, n_rows, label):
    x, axes = noise_rows(n_rows, n_ch)
    moved = 8 * n_rows * n_ch
    objs = {}
    for n_bins in (256, 1024):
        objs[f"stats {n_bins:4d} bins"] = g.device_stats(n_ch, n_rows, n_bins, axes, device_index=0)
    seg = 256 if n_rows >= 512 else 64
    objs["welch"] = g.device_welch(n_ch, n_rows, seg, device_index=0)
    fits = [(400.0 + 0.1 * c, 0.5, 0.1, 30.0, 2e4, 1e4, 2e4, 1e3, 0.0) for c in range(n_ch)]
    objs["resmap x_dqr"] = g.device_resmap(n_ch, n_rows, g.resmap_constants(fits, [(400.0 + 0.1 * c) * 1e6 for c in range(n_ch)]), kind="x_dqr",
                                           device_index=0)
    out = torch.zeros((n_rows, n_ch), dtype=torch.complex64, device=dev)
    feeds = {k: ((lambda o=o: o.feed_device(x, out)) if k.startswith("resmap") else (lambda o=o: o.feed_device(x))) for k, o in objs.items()}
    runs = {k: [] for k in objs}
    for _ in range(ROUNDS):
        for k in objs:
            runs[k].append(timed(feeds[k]))
    res = {}
    for k in objs:
        med, p90, back = (float(np.median([r[i] for r in runs[k]])) for i in range(3))
        lanes = f"lanes {objs[k].lanes:5d}" if k.startswith("stats") else ("segment %d" % seg if k == "welch" else "")
        say(f"{k:16s} {n_ch:5d} ch x {n_rows:8d} rows  median {med:8.1f} us  p90 {p90:8.1f} us  back to back {back:8.1f} us"
            f"  rows {moved / 1e6:.1f} MB  {moved / back / 1e3:7.1f} GB/s back to back  {lanes}")
        res[k] = back
    # the reads of a stats object: the summary read (one launch, n_ch x 64 bytes to the host, a wait) and the levels
    st = objs["stats  256 bins"]
    for name, call in (("read", st.read), ("levels median", lambda: st.levels(5.0, "median")), ("quantiles x5", lambda: st.quantiles([0.01, 0.25, 0.5, 0.75, 0.99]))):
        call()
        torch.cuda.synchronize()
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        say(f"stats {name:14s} {n_ch:5d} ch, 256 bins, lanes {st.lanes}: host wall time of the call, median of 20: {np.median(t):8.1f} us")
    s = st.read()
    say(f"check  n {int(s['n'][0])}  under+over {int(s['under'].sum() + s['over'].sum())}  bad {int(s['bad'].sum())}  sigma[0] {np.sqrt(s['var'][0]):.5f}")
    for o in objs.values():
        o.close()
    say(f"ratio   stats feed (256 bins) / welch feed: {res['stats  256 bins'] / res['welch']:.3f};  / resmap feed: {res['stats  256 bins'] / res['resmap x_dqr']:.3f}"
        f"  (back to back; {label})")
    return res


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
    res[label] = time_shape(n_ch, n_rows, label)
if DEMOD:
    for n_ch, n_rows, decim, L, label in SHAPES:
        try:
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   stats feed (256 bins) / demodulation kernel: {res[label]['stats  256 bins'] / d:.3f} (back to back)")
log.close()
