#!/usr/bin/env python3
"""Timings behind DESIGN.md section 5b.2 (sc16 output of the TX generators); the log is profiles/txgen_sc16.log.

One process measures one library (GSDR_LIB names another build, e.g. the parent commit's, with GSDR_LIB_OLD_ABI=1 when
it lacks the sc16 entries) and prints one JSON line:
  fill_c64_us / fill_sc16_us   gsdr_txgen_tones_fill / _fill_sc16, 2048 tones, 1 Mi samples: hipEvents round `--iters`
                               launches, blocks of the two alternating, `--pairs` blocks each; per-launch time of every block
  narrow_us                    gsdr_narrow_sc16_device at 1 Mi samples, the same way
  get_c64_ms / get_sc16_ms     gsdr_txgen_get / _get_sc16 of a 1 000 000-sample TONES buffer (16 tones) into pageable host
                               memory, host clock round the synchronous call, alternating
A/B between two builds: run this script alternately with the two libraries on the same box and compare the ranges.
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--tones", type=int, default=2048)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd import _lib
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    has_sc16 = hasattr(L, "gsdr_txgen_tones_fill_sc16") and L.gsdr_txgen_tones_fill_sc16.argtypes is not None
    rate, n = 200_000_000, 1 << 20
    rng = np.random.default_rng(1)
    freq = rng.choice(np.arange(1, rate // 2), size=a.tones, replace=False).astype(np.int32)
    freq[::2] *= -1
    ampl = np.full(a.tones, 0.5 / a.tones, dtype=np.float32)
    h = L.gsdr_txgen_tones_create(rate, freq.ctypes.data_as(C.POINTER(C.c_int)), ampl.ctypes.data_as(C.POINTER(C.c_float)),
                                  None, a.tones, 0)
    assert h, L.gsdr_last_error(None)
    out64 = torch.empty(n, dtype=torch.complex64, device=dev)
    out16 = torch.empty((n, 2), dtype=torch.int16, device=dev)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters):
            assert fn() == 0
        e1.record(st)
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1000.0 / a.iters, 3)

    def fill64():
        return L.gsdr_txgen_tones_fill(h, out64.data_ptr(), n, 12345, sp)

    def fill16():
        return L.gsdr_txgen_tones_fill_sc16(h, out16.data_ptr(), n, 12345, sp)

    def narrow():
        return L.gsdr_narrow_sc16_device(out64.data_ptr(), out16.data_ptr(), n, C.c_float(32767.0), None, sp)

    res = {"label": a.label, "lib": _lib.LIB_PATH, "tones": a.tones, "samples": n, "iters": a.iters}
    for fn in (fill64,) + ((fill16, narrow) if has_sc16 else ()):
        for _ in range(10):
            assert fn() == 0
    torch.cuda.synchronize()
    res["fill_c64_us"], res["fill_sc16_us"], res["narrow_us"] = [], [], []
    for _ in range(a.pairs):
        res["fill_c64_us"].append(timed(fill64))
        if has_sc16:
            res["fill_sc16_us"].append(timed(fill16))
    if has_sc16:
        for _ in range(a.pairs):
            res["narrow_us"].append(timed(narrow))
        # the sc16 fill is the narrowed complex64 fill (the comparison the tests make at small sizes, here at the timed size)
        fill64(), fill16()
        torch.cuda.synchronize()
        want = g.narrow_sc16(out64.cpu().numpy(), gain=32767.0)
        res["fill_sc16_equals_narrowed_fill_c64"] = bool(np.array_equal(out16.cpu().numpy(), want))
        res["clipped"] = int(L.gsdr_txgen_sc16_clipped(h))
    L.gsdr_txgen_close(h)
    # host copy: a 1 000 000-sample buffer to pageable host memory
    Lb = 1_000_000
    p = g.param(mode="TX", rate=100_000_000, buffer_len=Lb, freq=[1_000_000 * (k + 1) + 137 for k in range(16)],
                ampl=[1.0 / 16] * 16, wave_type=[g.w_type.TONES] * 16)
    tx = g.TX_buffer_generator(p)
    h64, h16 = np.empty(Lb, dtype=np.complex64), np.empty((Lb, 2), dtype=np.int16)
    res["get_c64_ms"], res["get_sc16_ms"] = [], []
    for k in range(3 + 20):
        t0 = time.perf_counter()
        tx.get(h64)
        t1 = time.perf_counter()
        if has_sc16:
            tx.get_sc16(h16)
        t2 = time.perf_counter()
        if k >= 3:
            res["get_c64_ms"].append(round((t1 - t0) * 1e3, 3))
            if has_sc16:
                res["get_sc16_ms"].append(round((t2 - t1) * 1e3, 3))
    tx.close()
    for k in ("get_c64_ms", "get_sc16_ms"):
        v = res.pop(k)
        if v:
            res[k] = {"min": min(v), "median": float(np.median(v)), "max": max(v), "n": len(v)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
