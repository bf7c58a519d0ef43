#!/usr/bin/env python3
"""CPU rehearsal of the matrix-core DDC arithmetic with four and with three real products per
complex multiply, on the high-dynamic-range combs of
tests/test_gpu_parity.py::test_direct_high_dynamic_range_comb (first buffer).

Emulated, in numpy: one power-of-two scale per output row (row_scale_exp of csrc/ddc_mfma.hip), the
tap product rounded to fp32, every MFMA operand split into fp16 hi + lo (three of the four
cross products kept), exact products, one fp32 rounding per 32-sample block sum, the block phasor
applied with fp32 FMAs, the row phasor in fp32.  Against oracle.Direct (fp64), with the reference's
own fp32 order (oracle/recipe_b.py, complex64) beside it; bound = max(1e-5, 3 x err32) per tone.

--rot-span 64: the three-product arithmetic with the block sum taken over 64 samples (phasor images of 64 samples,
one rotation per pair of blocks; the window padded with zero taps to whole pairs) beside the
32-sample one, on the 60 dB comb at the three longest windows.

--fold: the 64-sample arithmetic beside its folded form (phase from the centre of the span,
P1 = sum (a_j + a_j')*c_j, P2 = sum (b_j - b_j')*d_j, P3 = sum (a_j+b_j)*(c_j+d_j) + (a_j'+b_j')*(c_j-d_j) over j < 32,
j' = 63 - j; every operand one fp32 add, one rounding per sum), 60 dB comb at the three longest windows and the 40 dB
comb at M 1000.

--fold4: the folded three-product arithmetic beside the folded plain four products (DESIGN.md section 4.1g:
Re = sum (a_j + a_j')*c_j + (b_j' - b_j)*d_j, Im = sum (a_j - a_j')*d_j + (b_j + b_j')*c_j over j < 32, two units summed
into one fp32 result, acc += P*(Re + i*Im)), 60 dB comb at 250, 125, 94, 63 and 32 blocks and the 40 dB comb at M 1000.

--fold4 --span 128: the direct fold over 64-sample spans beside the same fold over 128-sample spans (DESIGN.md section
4.1i: t = j - 63.5, partner 127 - j, 64 partner pairs per unit, one rotation per 128 samples), same combs.

Reads nothing but oracle/ and gpu_sdr_amd/source.py.

    python3 tools/mac3_rehearsal.py > profiles/mac3_rehearsal.log
    python3 tools/mac3_rehearsal.py --rot-span 64 > profiles/mac3r2_rehearsal.log
    python3 tools/mac3_rehearsal.py --fold > profiles/fold_rehearsal.log
    python3 tools/mac3_rehearsal.py --fold4 > profiles/fold4_rehearsal.log
    python3 tools/mac3_rehearsal.py --fold4 --span 128 > profiles/span128_rehearsal.log
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle                                  # noqa: E402
from oracle import recipe_b                    # noqa: E402
from gpu_sdr_amd.source import host_tones      # noqa: E402

f32, f64 = np.float32, np.float64


def split(v):
    """fp32 -> fp16 hi + fp16 lo (v_cvt_f16_f32 round to nearest even; residual formed in fp32)"""
    v = v.astype(f32)
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(f32)).astype(np.float16)
    return hi.astype(f64), lo.astype(f64)


def gemm3(a, b):
    """sum over the block of hi*hi + hi*lo + lo*hi, products exact, one rounding to fp32"""
    ah, al = split(a)
    bh, bl = split(b)
    return (ah @ bh + ah @ bl + al @ bh).astype(f32)


def split_sum(a, b):
    """gemm3 without its rounding (a sum that goes on in the same accumulator)"""
    ah, al = split(a)
    bh, bl = split(b)
    return ah @ bh + ah @ bl + al @ bh


def fma(acc, p, k):
    return (acc.astype(f64) + p.astype(f64) * k.astype(f64)).astype(f32)


def phasor(ph, rate):
    ang = 2.0 * np.pi * (np.asarray(ph, dtype=f64) / rate)
    return np.cos(ang), -np.sin(ang)


def emulate(x, taps, freq, rate, M, F, products, span=32, fold=False):
    """rows F-1 .. nout-1 of the first buffer (windows that lie inside it); returns [rows][tones] complex128.
    span: samples per block sum and rotation (64: the pair rotation of section 4.1e, three products only);
    fold: the 64-sample span folded about its centre (section 4.1f; products 4: the direct fold of section 4.1g,
    which also folds a 128-sample span about its centre: 64 partner pairs, section 4.1i)"""
    assert span == 32 or products == 3 or fold
    assert not fold or span == 64 or (span == 128 and products == 4)
    N, MF = len(freq), M * F
    nout = len(x) // M
    rows = np.arange(F - 1, nout)
    nhi = (MF + span - 1) // span
    fm = np.mod(np.asarray(freq, dtype=np.int64), rate)
    eh = int(np.frexp(np.abs(taps).max())[1])
    hp = np.zeros(nhi * span, dtype=f32)
    hp[:MF] = np.ldexp(taps.astype(f32), -eh)
    xp = np.concatenate([x, np.zeros(span, dtype=np.complex64)])
    start = (rows - F + 1) * M
    win = xp[start[:, None] + np.arange(nhi * span)[None, :]]
    inside = np.arange(nhi * span) < MF
    mx = np.maximum(np.abs(win.real), np.abs(win.imag))[:, inside].max(axis=1).astype(f32)
    e = (mx.view(np.uint32) >> 23) & 0xff
    se = np.clip(140 - e.astype(np.int64), -100, 100)
    S = np.ldexp(f32(1), se).astype(f32)
    hs = hp[None, :] * S[:, None]
    a = np.where(inside[None, :], (win.real.astype(f32) * hs).astype(f32), f32(0))
    b = np.where(inside[None, :], (win.imag.astype(f32) * hs).astype(f32), f32(0))
    accr = np.zeros((len(rows), N), dtype=f32)
    acci = np.zeros((len(rows), N), dtype=f32)
    lo = np.arange(span, dtype=np.int64)
    wr, wi = phasor((fm[None, :] * lo[:, None]) % rate, rate)            # [span][N]
    c, d = wr.astype(f32), wi.astype(f32)
    if fold:
        H = span // 2                                                     # partner pairs of a span
        j = np.arange(H, dtype=np.int64)
        ph2 = (fm[None, :] * (span - 1 - 2 * j)[:, None]) % (2 * rate)    # w^(j - (span-1)/2) = conj(w^((span-1)/2 - j)), half samples
        cc, dd = np.cos(np.pi * ph2 / rate), np.sin(np.pi * ph2 / rate)
    for blk in range(nhi):
        ab, bb = a[:, span * blk: span * blk + span], b[:, span * blk: span * blk + span]
        pr, pi = phasor((fm * ((blk * span) % rate)) % rate, rate)
        if fold and products == 4:
            aj, bj, ap, bp = ab[:, :H], bb[:, :H], ab[:, :H - 1:-1], bb[:, :H - 1:-1]
            re = (split_sum((aj + ap).astype(f32), cc.astype(f32)) + split_sum((bp - bj).astype(f32), dd.astype(f32))).astype(f32)
            im = (split_sum((aj - ap).astype(f32), dd.astype(f32)) + split_sum((bj + bp).astype(f32), cc.astype(f32))).astype(f32)
            ps2 = (fm * ((2 * span * blk + span - 1) % (2 * rate))) % (2 * rate)
            pr, pi = np.cos(np.pi * ps2 / rate), -np.sin(np.pi * ps2 / rate)
            prf, pif = pr.astype(f32)[None, :], pi.astype(f32)[None, :]
            accr = fma(fma(accr, prf, re), -pif, im)
            acci = fma(fma(acci, pif, re), prf, im)
        elif fold:
            aj, bj, ap, bp = ab[:, :32], bb[:, :32], ab[:, :31:-1], bb[:, :31:-1]
            p1 = gemm3((aj + ap).astype(f32), cc.astype(f32))
            p2 = gemm3((bj - bp).astype(f32), dd.astype(f32))
            p3 = (split_sum((aj + bj).astype(f32), (cc + dd).astype(f32)) +
                  split_sum((ap + bp).astype(f32), (cc - dd).astype(f32))).astype(f32)
            ps2 = (fm * ((128 * blk + 63) % (2 * rate))) % (2 * rate)
            pr, pi = np.cos(np.pi * ps2 / rate), -np.sin(np.pi * ps2 / rate)
            prf, pif = pr.astype(f32)[None, :], pi.astype(f32)[None, :]
            pm, pp = (pi - pr).astype(f32)[None, :], (pr + pi).astype(f32)[None, :]
            accr = fma(fma(fma(accr, pp, p1), pm, p2), -pif, p3)
            acci = fma(fma(fma(acci, pm, p1), -pp, p2), prf, p3)
        elif products == 4:
            re = (gemm3(np.concatenate([ab, bb], axis=1), np.concatenate([c, -d], axis=0)))
            im = (gemm3(np.concatenate([ab, bb], axis=1), np.concatenate([d, c], axis=0)))
            prf, pif = pr.astype(f32)[None, :], pi.astype(f32)[None, :]
            accr = fma(fma(accr, prf, re), -pif, im)
            acci = fma(fma(acci, prf, im), pif, re)
        else:
            k1 = gemm3((ab + bb).astype(f32), c)
            k2 = gemm3(ab, (wi - wr).astype(f32))
            k3 = gemm3(bb, (wr + wi).astype(f32))
            prf, pif = pr.astype(f32)[None, :], pi.astype(f32)[None, :]
            pm, pp = (pr - pi).astype(f32)[None, :], (pr + pi).astype(f32)[None, :]
            accr = fma(fma(fma(accr, pm, k1), -pif, k2), -prf, k3)
            acci = fma(fma(fma(acci, pp, k1), prf, k2), -pif, k3)
    # row phasor w^(start of the window) / S * 2^eh, in fp32: tile phasor x row-in-tile phasor
    gt, r = rows // 32, rows % 32
    back = ((F - 1) * M) % rate
    tile_ph = (fm[None, :] * ((gt * 32 * M + rate - back) % rate)[:, None]) % rate
    br, bi = phasor(tile_ph, rate)
    dr, di = phasor((fm[None, :] * ((r * M) % rate)[:, None]) % rate, rate)
    inv = (np.ldexp(f32(1), -se) * f32(np.ldexp(1.0, eh))).astype(f32)[:, None]
    br, bi, dr, di = br.astype(f32), bi.astype(f32), (dr.astype(f32) * inv).astype(f32), (di.astype(f32) * inv).astype(f32)
    rr = (br * dr - bi * di).astype(f32)
    ri = (br * di + bi * dr).astype(f32)
    yr = (accr * rr - acci * ri).astype(f32)
    yi = (accr * ri + acci * rr).astype(f32)
    return yr.astype(f64) + 1j * yi.astype(f64)


def comb(N, rate, L, span_db, rng):
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    ampl = (10.0 ** (-np.linspace(0.0, span_db, N) / 20.0)).astype(np.float32)
    phase = rng.uniform(0, 2 * np.pi, N).astype(np.float32)
    return freq, host_tones(L, 0, rate, freq, ampl, phase, sigma=1e-5, seed=50)


def main_span(span):
    N, rate, F, span_db = 64, 200_000_000, 4, 60
    print(f"span_dB  M  blocks | err32 (reference fp32 order) | 3 products, rotation per 32: worst err, worst err/bound | "
          f"rotation per {span}: worst err, worst err/bound | median, max per-tone ratio {span}/32")
    for M in (2000, 1000, 750):
        L = 200 * M
        freq, x = comb(N, rate, L, span_db, np.random.default_rng(4242 + span_db))
        ref = oracle.Direct(freq, rate, M, F, L)
        taps = ref.taps()
        yr = ref.process(x).astype(np.complex128)[F:]
        y32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64).process(x).astype(np.complex128)[F:]
        den = np.linalg.norm(yr, axis=0)
        err32 = np.linalg.norm(y32 - yr, axis=0) / den
        bound = np.maximum(1e-5, 3.0 * err32)
        errs = {}
        for sp in (32, span):
            y = emulate(x, taps, freq, rate, M, F, 3, span=sp)[1:]
            errs[sp] = np.linalg.norm(y - yr, axis=0) / den
        ratio = errs[span] / errs[32]
        print(f"{span_db:3d} {M:5d} {(M * F + 31) // 32:4d} | {err32.max():.3e} | {errs[32].max():.3e} {(errs[32] / bound).max():.3f} | "
              f"{errs[span].max():.3e} {(errs[span] / bound).max():.3f} | {np.median(ratio):.2f} {ratio.max():.2f}", flush=True)


def main_fold():
    N, rate, F = 64, 200_000_000, 4
    print("span_dB  M  blocks | err32 (reference fp32 order) | 3 products, rotation per 64: worst err, worst err/bound | "
          "folded: worst err, worst err/bound | median, max per-tone ratio folded/64")
    for span_db, decims in ((60, (2000, 1000, 750)), (40, (1000,))):
        for M in decims:
            L = 200 * M
            freq, x = comb(N, rate, L, span_db, np.random.default_rng(4242 + span_db))
            ref = oracle.Direct(freq, rate, M, F, L)
            taps = ref.taps()
            yr = ref.process(x).astype(np.complex128)[F:]
            y32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64).process(x).astype(np.complex128)[F:]
            den = np.linalg.norm(yr, axis=0)
            err32 = np.linalg.norm(y32 - yr, axis=0) / den
            bound = np.maximum(1e-5, 3.0 * err32)
            errs = {}
            for fold in (False, True):
                y = emulate(x, taps, freq, rate, M, F, 3, span=64, fold=fold)[1:]
                errs[fold] = np.linalg.norm(y - yr, axis=0) / den
            ratio = errs[True] / errs[False]
            print(f"{span_db:3d} {M:5d} {(M * F + 31) // 32:4d} | {err32.max():.3e} | {errs[False].max():.3e} {(errs[False] / bound).max():.3f} | "
                  f"{errs[True].max():.3e} {(errs[True] / bound).max():.3f} | {np.median(ratio):.2f} {ratio.max():.2f}", flush=True)


def main_fold4():
    N, rate, F = 64, 200_000_000, 4
    print("span_dB  M  blocks | err32 (reference fp32 order) | Gauss fold: worst err, worst err/bound | "
          "direct fold: worst err, worst err/bound | median, max per-tone ratio direct/Gauss")
    for span_db, decims in ((60, (2000, 1000, 750, 500, 256)), (40, (1000,))):
        for M in decims:
            L = 200 * M
            freq, x = comb(N, rate, L, span_db, np.random.default_rng(4242 + span_db))
            ref = oracle.Direct(freq, rate, M, F, L)
            taps = ref.taps()
            yr = ref.process(x).astype(np.complex128)[F:]
            y32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64).process(x).astype(np.complex128)[F:]
            den = np.linalg.norm(yr, axis=0)
            err32 = np.linalg.norm(y32 - yr, axis=0) / den
            bound = np.maximum(1e-5, 3.0 * err32)
            errs = {}
            for products in (3, 4):
                y = emulate(x, taps, freq, rate, M, F, products, span=64, fold=True)[1:]
                errs[products] = np.linalg.norm(y - yr, axis=0) / den
            ratio = errs[4] / errs[3]
            print(f"{span_db:3d} {M:5d} {(M * F + 31) // 32:4d} | {err32.max():.3e} | {errs[3].max():.3e} {(errs[3] / bound).max():.3f} | "
                  f"{errs[4].max():.3e} {(errs[4] / bound).max():.3f} | {np.median(ratio):.2f} {ratio.max():.2f}", flush=True)


def main_span128():
    N, rate, F = 64, 200_000_000, 4
    print("span_dB  M  blocks | err32 (reference fp32 order) | direct fold, 64-sample spans: worst err, worst err/bound | "
          "128-sample spans: worst err, worst err/bound | median, max per-tone ratio 128/64")
    for span_db, decims in ((60, (2000, 1000, 750, 500, 375, 256)), (40, (1000,))):
        for M in decims:
            L = 200 * M
            freq, x = comb(N, rate, L, span_db, np.random.default_rng(4242 + span_db))
            ref = oracle.Direct(freq, rate, M, F, L)
            taps = ref.taps()
            yr = ref.process(x).astype(np.complex128)[F:]
            y32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64).process(x).astype(np.complex128)[F:]
            den = np.linalg.norm(yr, axis=0)
            err32 = np.linalg.norm(y32 - yr, axis=0) / den
            bound = np.maximum(1e-5, 3.0 * err32)
            errs = {}
            for sp in (64, 128):
                y = emulate(x, taps, freq, rate, M, F, 4, span=sp, fold=True)[1:]
                errs[sp] = np.linalg.norm(y - yr, axis=0) / den
            ratio = errs[128] / errs[64]
            print(f"{span_db:3d} {M:5d} {(M * F + 31) // 32:4d} | {err32.max():.3e} | {errs[64].max():.3e} {(errs[64] / bound).max():.3f} | "
                  f"{errs[128].max():.3e} {(errs[128] / bound).max():.3f} | {np.median(ratio):.2f} {ratio.max():.2f}", flush=True)


def main():
    if "--fold4" in sys.argv and "--span" in sys.argv:
        assert sys.argv[sys.argv.index("--span") + 1] == "128"
        return main_span128()
    if "--fold4" in sys.argv:
        return main_fold4()
    if "--fold" in sys.argv:
        return main_fold()
    if "--rot-span" in sys.argv:
        return main_span(int(sys.argv[sys.argv.index("--rot-span") + 1]))
    N, rate, F = 64, 200_000_000, 4
    print("span_dB  M  blocks | err32 (reference fp32 order) | 4 products: worst err, worst err/bound | 3 products: worst err, worst err/bound | median, max per-tone ratio 3/4")
    for span_db, decims in ((60, (2000, 1000, 750, 500, 375, 256, 100)), (40, (1000,))):
        for M in decims:
            n, rt = (32, 10_000_000) if M == 100 else (N, rate)
            L = 1000 * M if M == 100 else 200 * M
            freq, x = comb(n, rt, L, span_db, np.random.default_rng(4242 + span_db))
            ref = oracle.Direct(freq, rt, M, F, L)
            taps = ref.taps()
            yr = ref.process(x).astype(np.complex128)[F:]
            y32 = recipe_b.Direct(freq, rt, M, F, L, acc=np.complex64).process(x).astype(np.complex128)[F:]
            den = np.linalg.norm(yr, axis=0)
            err32 = np.linalg.norm(y32 - yr, axis=0) / den
            bound = np.maximum(1e-5, 3.0 * err32)
            errs = {}
            for products in (4, 3):
                y = emulate(x, taps, freq, rt, M, F, products)[1:]      # rows F .. as the test
                errs[products] = np.linalg.norm(y - yr, axis=0) / den
            ratio = errs[3] / errs[4]
            print(f"{span_db:3d} {M:5d} {(M * F + 31) // 32:4d} | {err32.max():.3e} | {errs[4].max():.3e} {(errs[4] / bound).max():.3f} | "
                  f"{errs[3].max():.3e} {(errs[3] / bound).max():.3f} | {np.median(ratio):.2f} {ratio.max():.2f}", flush=True)


if __name__ == "__main__":
    main()
