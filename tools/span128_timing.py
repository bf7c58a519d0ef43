"""A/B of the 64- and the 128-sample spans of the wide-tile folded DDC over the window length,
in one process on one GPU: python tools/span128_timing.py [LOG]  (profiles/span128_ab_windows.log is its output).

2048 tones at 200 Msps, F = 4, 1000 rows per buffer, windows of 32, 63, 94 and 125 blocks (decimation 256, 500, 750,
1000); the wide tile and the fold forced at every length, GSDR_MFMA_SPAN = 64 and = 128 on two handles that take
turns: six rounds of STEPS buffers through gsdr_demod_submit_device with three outstanding, behind a warm-up."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sdr_amd as g  # noqa: E402
from gpu_sdr_amd.source import device_tones, tone_comb  # noqa: E402

STEPS = int(os.environ.get("SPAN128_AB_STEPS", "500"))
ROUNDS, DEPTH, RATE, N, F, ROWS = 6, 3, 200_000_000, 2048, 4, 1000
FORCED = {"GSDR_DDC_MFMA": "1", "GSDR_DDC_FEW": "0", "GSDR_MFMA_ASM": "4", "GSDR_MFMA_PREC": "1", "GSDR_MFMA_3M": "1",
          "GSDR_MFMA_3M_ROT": "2", "GSDR_MFMA_FOLD": "1", "GSDR_MFMA_FOLD_PRODUCTS": "4", "GSDR_MFMA_WAVE_TONES": "64"}
log = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
dev = torch.device("cuda:0")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


def handle(M, span, freq):
    os.environ.update(FORCED, GSDR_MFMA_SPAN=str(span))       # read when a demodulator is created
    p = g.param(mode="RX", rate=RATE, buffer_len=ROWS * M, decim=M, pf_average=F, freq=[int(v) for v in freq],
                wave_type=[g.w_type.DIRECT] * N)
    d = g.RX_buffer_demodulator(p, device_index=0)
    assert d.describe()["span_samples"] == span and d.describe()["wave_tones"] == 64, d.describe()
    return d


def run(d, bufs, outs, steps):
    pending = 0
    for k in range(steps):
        if pending == DEPTH:
            d.wait()
            pending -= 1
        d.submit_device(bufs[k % len(bufs)], outs[k % DEPTH])
        pending += 1
    while pending:
        d.wait()
        pending -= 1
    torch.cuda.synchronize()


say("# spans of 64 and of 128 samples, wide tile forced;", torch.cuda.get_device_name(0), f"; {N} tones, {ROWS} rows, F {F};",
    ROUNDS, "alternating rounds of", STEPS, "buffers, submit_device with", DEPTH, "outstanding")
freq, ampl, phase = tone_comb(N, RATE, seed=20251004)
for M in (256, 500, 750, 1000):
    L = ROWS * M
    bufs = [torch.empty(L, dtype=torch.complex64, device=dev) for _ in range(4)]
    for k, x in enumerate(bufs):
        device_tones(x, k * L, RATE, freq, ampl, phase, sigma=1e-3, seed=300 + k)
    hs = {s: handle(M, s, freq) for s in (64, 128)}
    outs = {s: [torch.empty(hs[s].out_capacity, dtype=torch.complex64, device=dev) for _ in range(DEPTH)] for s in hs}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:
        for s in hs:
            run(hs[s], bufs, outs[s], 50)
    ms = {s: [] for s in hs}
    for r in range(ROUNDS):
        for s in hs:
            run(hs[s], bufs, outs[s], 50)
            t0 = time.perf_counter()
            run(hs[s], bufs, outs[s], STEPS)
            ms[s].append((time.perf_counter() - t0) * 1e3 / STEPS)
    for s in hs:
        hs[s].close()
    nblk = (M * F + 31) // 32
    a, b = np.array(ms[64]), np.array(ms[128])
    gap = "128 wholly below 64" if b.max() < a.min() else "64 wholly below 128" if a.max() < b.min() else "ranges overlap"
    say(f"{nblk:4d} blocks (M {M:4d}): span 64 median {np.median(a):.5f} range {a.min():.5f} - {a.max():.5f} ms | "
        f"span 128 median {np.median(b):.5f} range {b.min():.5f} - {b.max():.5f} ms | 128/64 x{np.median(b) / np.median(a):.4f} | {gap}")
