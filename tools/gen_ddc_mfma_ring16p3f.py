#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p3f_gen.h: main loop of ddc_mfma_ring16p3f_kernel
(gfx950) -- the three-product loop with the even and odd sums of each 64-sample span FOLDED
(DESIGN.md section 4.1f).

The phase of a span is taken from its centre, t = j - 31.5 with partner j' = 63 - j, so that the
phasor w^t = c + i*d has c(j') = c(j) and d(j') = -d(j).  With a + i*b = S*h'*x, Gauss's three
products over the 64 samples become

    P1 = sum a*c        = sum_{j<32} (a_j + a_j')*c_j                              U1 x c
    P2 = sum b*d        = sum_{j<32} (b_j - b_j')*d_j                              U2 x d
    P3 = sum (a+b)(c+d) = sum_{j<32} (a_j+b_j)*(c_j+d_j) + (a_j'+b_j')*(c_j-d_j)   U3 x (c+d) + U4 x (c-d)
    Re = P1 - P2        Im = P3 - P1 - P2

four real GEMMs of K = 32 per span: 4 units x 4 tiles x 3 (lo*hi, hi*lo, hi*hi) = 48
v_mfma_f32_16x16x32_f16 where the loop of section 4.1e takes 72.  The rotation acc += P*(Re + i*Im)
with the span phasor P = w^(64*s + 31.5), (Pr, Pi, Pi-Pr, Pr+Pi) from the host table:

    P1: acc_r += (Pr+Pi)*P1   acc_i += (Pi-Pr)*P1
    P2: acc_r += (Pi-Pr)*P2   acc_i += -(Pr+Pi)*P2
    P3: acc_r += -Pi*P3       acc_i += Pr*P3

96 v_fma_f32 per span.

Ring slot (16 KiB, written by ddc_convert3f_kernel): piece p = 4*unit + 2*sp + rh of 1 KiB, lane
linear: lane l holds row 16*rh + (l & 15), j = 8*(l >> 4) .. +7; unit 0..3 = U1..U4; sp 0 = fp16 hi,
1 = lo.  Wave w copies pieces 4w .. 4w+3 of every image.  The phasor images c, d, c+d, c-d of j < 32
live in a0..a63.

One trip of the generated loop is two spans (parity A, parity B: one set of ring addresses, scalar
bases and span phasors each, rule R2), with an exit between them.  Schedule of a span (48 gaps, one
behind each MFMA), unit u at gaps 12u .. 12u+11, P3 summed over units 2 and 3:
  * rotation, two FMAs per gap over gaps 2..47: P3 of the span BEFORE (final after its gap 47,
    rewritten from gap 24 on) in gaps 2..17 with that span's P, P1 (final after gap 11) in 17..32,
    P2 (final after gap 23, rewritten from gap 12 of the next span) in 32..47;
  * an operand fragment is read again for its next use 23 or more MFMAs after its last one (R1) and
    8 or more ahead of its first: the lo fragments 10 and 8 gaps ahead of their unit, the hi
    fragments 4 and 2 -- units 1, 2, 3 of this span in gaps 2..34, unit 0 of the next span (from the
    next slot) in gaps 38..46;
  * the image of span s+3 is copied in four pieces at gaps 2, 10, 18, 26; P of span s+1 is loaded at
    gap 28 into the other parity's registers (last read in gap 16) and first used in gap 17 of s+1.

    python3 tools/gen_ddc_mfma_ring16p3f.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p3f_gen.h
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddc_mfma_pframe import Loop, print_loop   # noqa: E402

NU = 4                     # operand units U1..U4
NG = 12 * NU               # MFMAs per span

# ---- register map ------------------------------------------------------------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48, VB + 64)   # products P1, P2, P3
F0 = VB + 80               # operand fragment (unit, rh, sp) at v[F0 + 16*unit + 8*sp + 4*rh : +3]
P = {"A": VB + 144, "B": VB + 152}   # (Pr, Pi, Pi-Pr, Pr+Pi) of tone half 0, of tone half 1
ADDR = {"A": (VB + 160, VB + 161), "B": (VB + 162, VB + 163)}
V_LAST = VB + 163
NAGPR = 16 * NU
BF = [56, 66, 68, 70]      # scalar bases of the 16 phasor images, 4 KiB apart (prologue)
ROT0, ROT1 = 2, 47         # the FMAs of a span lie in gaps ROT0..ROT1
G_PLOAD = 28


def rotation(p_cur, p_prev):
    """[(gap, kind, v_fma_f32)]: P3 of the span before, then P1 and P2 of this one."""
    ops = [("rot", op) for op in LOOP.rotate_ops(2, p_prev)] + \
          [("rotp", op) for prod in (0, 1) for op in LOOP.rotate_ops(prod, p_cur)]
    n = len(ops)
    placed = [(ROT0 + (k * (ROT1 - ROT0 + 1)) // n, kind, op) for k, (kind, op) in enumerate(ops)]
    for k, (g, _, _) in enumerate(placed):
        # a product is final three MFMAs ago and not rewritten for two more
        lo, hi = ((NG - 1 + 3 - NG, 24 - 2), (11 + 3, NG - 2), (23 + 3, NG + 12 - 2))[k // 32]
        assert lo <= g <= hi, (k, g)
    # the registers of p_prev are loaded anew at G_PLOAD
    assert max(g for g, kind, _ in placed if kind == "rot") < G_PLOAD - 2
    return placed


LOOP = Loop(noun="span", units=NU, prod=(0, 1, 2, 2), image=(0, 1, 2, 3),
            split=((1, 0), (0, 1), (0, 0)),                  # lo*hi, hi*lo, hi*hi: small terms first
            # the lo fragments (used by the first four MFMAs only) first, the hi fragments in the one gap that is
            # 23 MFMAs behind their last use (R1) and 8 ahead of their first
            read_at={(0, 1): -10, (1, 1): -8, (0, 0): -4, (1, 0): -2},
            coef=(("p", "m"), ("m", "-p"), ("-i", "r")),     # P1, P2, P3; m = Pi-Pr, p = Pr+Pi
            late=2, g_pload=G_PLOAD,
            rotation=rotation, vb=VB, acc=ACC, kb=KB, f0=F0, p=P, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P3F", __file__,
               "Main loop of ddc_mfma_ring16p3f_kernel (three real products per complex multiply over 64-sample spans folded about their centre: four K=32 operand units per span)")


if __name__ == "__main__":
    main()
