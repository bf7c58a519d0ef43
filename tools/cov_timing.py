"""Timing of the device channel covariance (gsdr_cov_feed_device) beside the stats feed of the
same rows and the demodulation they follow, in one process on one GPU:
python tools/cov_timing.py [LOG]  (profiles/cov_timing.log is its output).
COV_TIMING_FEEDS=n takes n feeds instead of 200, COV_TIMING_DEMOD=0 leaves the demodulators out, COV_TIMING_LANES=n
asks for n chains instead of the rule's, COV_TIMING_SHAPES=0,2 takes those of the three shapes only."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd import covariance  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402
from gpu_sdr_amd.trigger import LEVEL_DTYPE  # noqa: E402

FEEDS = int(os.environ.get("COV_TIMING_FEEDS", "200"))
WARM = 10
DEMOD = os.environ.get("COV_TIMING_DEMOD", "1") != "0"
LANES = int(os.environ.get("COV_TIMING_LANES", "0"))
ONLY = [int(v) for v in os.environ.get("COV_TIMING_SHAPES", "0,1,2").split(",")]
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device channel covariance beside the stats feed of the same rows and the demodulation they follow;", torch.cuda.get_device_name(0),
    "; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (2 launches), median / p90 of", FEEDS, "; back to back: one event pair around all of them;")
say("# every timed run is enqueued behind some tens of ms of other work, so that the device, not the host, sets the pace;")
say("# the cov and stats runs of a shape alternate: the figure is the median over the runs of a kind")
say("# FMAs: rows x n_var (n_var + 1) / 2, the cells the contract names; TFLOP/s: 2 x those over the back-to-back time;")
say("# the kernel does rows x pairs x tile^2 of them (whole squares of the diagonal pairs and the padding of the last tile)")
say("# data-sheet FP64 vector peak: 78.6 TFLOP/s")

RATE = 200_000_000
ROUNDS = 3
PEAK = 78.6e12


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
    """Gaussian noise at 1e-3 of a per-channel carrier, half of its variance common to all channels"""
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.linspace(0.2, 0.5, n_ch, device=dev)
    own = torch.randn((n_rows, n_ch, 2), generator=gen, device=dev)
    common = torch.randn((n_rows, 1, 2), generator=gen, device=dev)
    x = (own + common) * (0.5 ** 0.5) * 1e-3 * base[None, :, None] + base[None, :, None]
    return torch.view_as_complex(x.contiguous()).contiguous(), base.cpu().numpy().astype(np.float64)


def time_shape(n_ch, n_rows, quadrature, label):
    x, base = noise_rows(n_rows, n_ch)
    n_quad = 2 if quadrature == "both" else 1
    axes = g.cov_axes(range(n_ch), quadrature, pivots=np.tile(base, n_quad))
    n_var = axes.shape[0]
    cv = g.device_cov(n_ch, axes, n_rows, lanes=LANES, device_index=0)
    plan = covariance.feed_plan(n_ch, n_var, cv.lanes)
    lv = np.zeros(n_ch, dtype=LEVEL_DTYPE)
    lv["dx"], lv["lo"], lv["hi"] = 1, base - 0.01, base + 0.01
    st = g.device_stats(n_ch, n_rows, 256, lv, device_index=0)
    feeds = {"cov": lambda: cv.feed_device(x), "stats 256 bins": lambda: st.feed_device(x)}
    runs = {k: [] for k in feeds}
    for _ in range(ROUNDS):
        for k in feeds:
            runs[k].append(timed(feeds[k]))
    res = {}
    for k in feeds:
        med, p90, back = (float(np.median([r[i] for r in runs[k]])) for i in range(3))
        res[k] = back
        extra = ""
        if k == "cov":
            fmas = n_rows * n_var * (n_var + 1) // 2
            done = n_rows * plan["pairs"] * plan["tile"] ** 2
            extra = (f"  n_var {n_var}  lanes {cv.lanes}  tile {plan['tile']}  pairs {plan['pairs']}  {fmas / 1e9:.3f} GFMA named, {done / 1e9:.3f} done"
                     f"  {2 * fmas / back / 1e6:6.2f} TFLOP/s named, {2 * done / back / 1e6:6.2f} done  at peak {2 * fmas / PEAK * 1e6:6.1f} us")
        say(f"{k:16s} {n_ch:5d} ch x {n_rows:8d} rows  median {med:8.1f} us  p90 {p90:8.1f} us  back to back {back:8.1f} us{extra}")
    for kind in ("sums", "cov", "corr"):
        cv.read(kind)
        torch.cuda.synchronize()
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            cv.read(kind)
            t.append((time.perf_counter() - t0) * 1e6)
        say(f"cov read {kind:5s} {n_var:5d} variables, lanes {cv.lanes}: host wall time of the call (launch, wait, {8 * n_var * (n_var + 1) / 1e6:.2f} MB to the host),"
            f" median of 20: {np.median(t):9.1f} us")
    c, _ = cv.read("corr")
    off = c[~np.eye(n_var, dtype=bool)] if n_var > 1 else np.zeros(1)
    say(f"check  rows {cv.rows_seen}  corr diagonal {float(np.diagonal(c).min()):.3f}..{float(np.diagonal(c).max()):.3f}  off-diagonal {float(off.min()):.3f}..{float(off.max()):.3f}")
    say(f"ratio   cov feed / stats feed: {res['cov'] / res['stats 256 bins']:.2f}  (back to back; {label})")
    cv.close(), st.close()
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


# n_ch, rows per buffer, quadratures, decim, L, label
SHAPES = [(2048, 1000, "re", 1000, 1_000_000, "DIRECT 2048 tones decim 1000 L 1e6"),
          (256, 10000, "re", 100, 1_000_000, "DIRECT 256 tones decim 100 L 1e6"),
          (4, 1 << 20, "both", 0, 1 << 20, "DIRECT 4 tones undecimated L 2^20, both quadratures")]
SHAPES = [s for k, s in enumerate(SHAPES) if k in ONLY]
res = {}
for n_ch, n_rows, quad, decim, L, label in SHAPES:
    res[label] = time_shape(n_ch, n_rows, quad, label)
    say(f"period  {label}: a buffer of {L} samples lasts {L / RATE * 1e6:.0f} us at 200 Msps; cov feed / period: {res[label]['cov'] / (L / RATE * 1e6):.4f}")
if DEMOD:
    for n_ch, n_rows, quad, decim, L, label in SHAPES:
        try:
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   cov feed / demodulation kernel: {res[label]['cov'] / d:.3f} (back to back)")
log.close()
