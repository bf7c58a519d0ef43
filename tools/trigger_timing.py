"""Timing of the device trigger (gsdr_trigger_feed_device) beside the demodulation it follows, in
one process on one GPU: python tools/trigger_timing.py [LOG]  (profiles/trigger_ab.log is its output).
TRIGGER_AB_FEEDS=n takes n feeds instead of 200, TRIGGER_AB_DEMOD=0 leaves the demodulators out (a pass under
rocprofv3 --kernel-trace for the per-kernel split)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
import gpu_sdr_amd.trigger as T  # noqa: E402
from gpu_sdr_amd.source import tone_comb  # noqa: E402

FEEDS = int(os.environ.get("TRIGGER_AB_FEEDS", "200"))
WARM = 20
DEMOD = os.environ.get("TRIGGER_AB_DEMOD", "1") != "0"
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


dev = torch.device("cuda:0")
say("# device trigger beside the demodulation it follows;", torch.cuda.get_device_name(0), "; feeds", FEEDS, "after", WARM, "warm-up")
say("# per-feed time: hipEvents around each feed (3 launches), median / p90 of", FEEDS, "; amortised: one event pair around all of them")

RATE = 200_000_000


def time_trigger(n_ch, n_rows, hits):
    rng = np.random.default_rng(1)
    rows = (0.1 * (rng.standard_normal((n_rows, n_ch)) + 1j * rng.standard_normal((n_rows, n_ch)))).astype(np.complex64)
    lv = np.zeros(n_ch, dtype=T.LEVEL_DTYPE)
    lv["dx"] = 1.0
    pre, post, holdoff, max_events = 16, 48, 16, 64
    if hits:
        lv["lo"], lv["hi"] = -1.0, 1.0
        for k in range(10):
            rows[100 + k * (n_rows - 200) // 10, (k * 7) % n_ch] += 3.0
    else:
        lv["lo"], lv["hi"] = -1e9, 1e9
    want = None
    if hits:
        h = T.host_trigger(n_ch, n_rows, pre, post, holdoff, max_events, lv)
        h.feed(rows)
        want = h.feed(rows)          # the second feed of the stream: what every later feed gives
        h.close()
    x = torch.from_numpy(rows).to(dev)
    t = T.device_trigger(n_ch, n_rows, pre, post, holdoff, max_events, lv, device_index=0)
    ev = torch.zeros(max_events * 24, dtype=torch.uint8, device=dev)
    sn = torch.zeros((max_events, pre + post, n_ch), dtype=torch.complex64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    for _ in range(WARM):
        t.feed_device(x, ev, sn, cnt)
    torch.cuda.synchronize()
    a = [torch.cuda.Event(enable_timing=True) for _ in range(FEEDS)]
    b = [torch.cuda.Event(enable_timing=True) for _ in range(FEEDS)]
    for k in range(FEEDS):
        a[k].record()
        t.feed_device(x, ev, sn, cnt)
        b[k].record()
    torch.cuda.synchronize()
    per = np.array([a[k].elapsed_time(b[k]) for k in range(FEEDS)]) * 1e3
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(FEEDS):
        t.feed_device(x, ev, sn, cnt)
    e.record()
    torch.cuda.synchronize()
    amort = s.elapsed_time(e) * 1e3 / FEEDS
    n_ev, dropped = (int(v) for v in cnt.cpu().numpy())
    ok = ""
    if want is not None:
        got_ev = ev.cpu().numpy().view(T.EVENT_DTYPE)[:n_ev]
        got_sn = sn[:n_ev].cpu().numpy()
        same = (n_ev == len(want[0]) and (got_ev["row"] - got_ev["row"][0] == want[0]["row"] - want[0]["row"][0]).all()
                and all(got_ev[f].tobytes() == want[0][f].tobytes() for f in ("channel", "side", "q", "n_hit"))
                and got_sn.tobytes() == want[1].tobytes())
        ok = "equals host twin" if same else "DIFFERS FROM HOST TWIN"
    t.close()
    say(f"trigger {n_ch:5d} ch x {n_rows:8d} rows  {'~10 events' if hits else 'no hits  '}  median {np.median(per):8.1f} us  p90 {np.percentile(per, 90):8.1f} us"
        f"  amortised {amort:8.1f} us  events {n_ev} dropped {dropped}  bytes {rows.nbytes / 1e6:.1f} MB  {ok}")
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
trig = {}
for n_ch, n_rows, decim, L, label in SHAPES:
    trig[label] = (time_trigger(n_ch, n_rows, False), time_trigger(n_ch, n_rows, True))
if DEMOD:
    for n_ch, n_rows, decim, L, label in SHAPES:
        a, b = trig[label]
        try:
            d = time_demod(n_ch, decim, L, label)
        except Exception as ex:
            say(f"demod   {label}: not measured ({type(ex).__name__}: {ex})")
            log.close()
            sys.exit(3)              # nothing more on the GPU after an error
        say(f"ratio   trigger / demodulation kernel: no hits {a[1] / d:.3f}, ~10 events {b[1] / d:.3f} (amortised)")
log.close()
