#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p3_gen.h: main loop of ddc_mfma_ring16p3_kernel
(gfx950) -- the pre-converted ring loop of tools/gen_ddc_mfma_ring16p.py with the complex
multiply-accumulate done in THREE real products instead of four.

With x*h' = a + i*b (the tone-independent A operand) and the phasor w = c + i*d (the B table):

    K1 = sum (a+b)*c      K2 = sum a*(d-c)      K3 = sum b*(c+d)
    Re = K1 - K3          Im = K1 + K2

Each of the three is a real GEMM whose K = 32 spans the 32 samples of a block, so a block takes
3 components x 4 tiles x 3 (hi*hi, hi*lo, lo*hi) = 36 v_mfma_f32_16x16x32_f16 instead of 48.
The rotation acc += P*(Re + i*Im) becomes, per component and accumulator element, two plain FMAs

    K1: acc_r += (Pr-Pi)*K1   acc_i += (Pr+Pi)*K1
    K2: acc_r += -Pi*K2       acc_i +=  Pr*K2
    K3: acc_r += -Pr*K3       acc_i += -Pi*K3

(Pr-Pi and Pr+Pi come from the host table: four floats per block and tone), 96 per block.

Ring slot (12 KiB, written by ddc_convert3_kernel): piece p = 4*comp + 2*sp + rh of 1 KiB, lane
linear: lane l holds row 16*rh + (l & 15), samples 8*(l >> 4) .. +7 of the block; comp 0 = a+b,
1 = a, 2 = b; sp 0 = fp16 hi, 1 = lo.  Wave w copies pieces 3w .. 3w+2 of every image.

Schedule of block b (36 gaps, one behind each MFMA), component c at gaps 12c .. 12c+11:
  * the products of a component are rotated into the accumulators from two MFMAs behind its last
    one on: component 0 in gaps 14..25, 1 in 26..35, 2 in gaps 2..13 of block b+1 -- one buffer of
    16 registers per component is enough (it is rewritten 24 MFMAs after its last FMA read it);
  * an operand fragment is read again for block b+1 24 MFMAs after its last use (R1), eight or more
    ahead of its first: component 1 and 2 of block b in gaps 4..10 / 16..22, component 0 of b+1 in
    gaps 28..34;
  * the image of block b+3 is copied in three pieces at gaps 2, 10, 18; P of block b+1 is loaded at
    gap 20 (its registers were last read in gap 13) and first used in gap 14 of block b+1.

    python3 tools/gen_ddc_mfma_ring16p3.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p3_gen.h
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddc_mfma_pframe import Loop, print_loop   # noqa: E402

NC = 3                     # components: a+b, a, b
NG = 12 * NC               # MFMAs per block

# ---- register map ------------------------------------------------------------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48, VB + 64)   # products K1, K2, K3
F0 = VB + 80               # operand fragment (comp, rh, sp) at v[F0 + 16*comp + 8*sp + 4*rh : +3]
P = {"A": VB + 128, "B": VB + 136}   # (Pr, Pi, Pr-Pi, Pr+Pi) of tone half 0, of tone half 1
# ring addresses, one set per iteration parity (R2): this block's slot, the next block's
ADDR = {"A": (VB + 144, VB + 145), "B": (VB + 146, VB + 147)}
V_LAST = VB + 147
NAGPR = 16 * NC
BF = [56, 66, 68]          # scalar bases of the 12 phasor images, 4 KiB apart (prologue)


def rotation(p_cur, p_prev):
    """[(gap, kind, v_fma_f32)]: component 2 of the previous block (gaps 2..13), 0 (14..25) and 1
    (26..35) of this one"""
    return [(g0 + (k * span) // 32, kind, op)
            for comp, kind, p, g0, span in ((2, "rot", p_prev, 2, 12), (0, "rotp", p_cur, 14, 12), (1, "rotp", p_cur, 26, 10))
            for k, op in enumerate(LOOP.rotate_ops(comp, p))]


LOOP = Loop(noun="block", units=NC, prod=(0, 1, 2), image=(0, 1, 2),
            split=((0, 0), (0, 1), (1, 0)),                  # hi*hi, hi*lo, lo*hi
            read_at={(0, 0): -8, (1, 0): -6, (0, 1): -4, (1, 1): -2},
            coef=(("m", "p"), ("-i", "r"), ("-r", "-i")),    # K1, K2, K3; m = Pr-Pi, p = Pr+Pi
            late=2, g_pload=20,                              # P's registers were last read in gap 13
            rotation=rotation, vb=VB, acc=ACC, kb=KB, f0=F0, p=P, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P3", __file__,
               "Main loop of ddc_mfma_ring16p3_kernel (pre-converted operands by LDS-DMA, three real products per complex multiply, v_mfma_f32_16x16x32_f16)")


if __name__ == "__main__":
    main()
