#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p4f_gen.h: main loop of ddc_mfma_ring16p4f_kernel
(gfx950) -- the folded loop of tools/gen_ddc_mfma_ring16p3f.py with the plain four real products
per complex multiply instead of Gauss's three.

With t = j - 31.5, partner j' = 63 - j, w^t = c + i*d, c(j') = c(j), d(j') = -d(j) and
a + i*b = S*h'*x, both parts of the complex sum over a 64-sample span fold completely:

    Re = sum a*c - sum b*d = sum_{j<32} (a_j + a_j')*c_j + (b_j' - b_j)*d_j        V1 x c + V2 x d
    Im = sum a*d + sum b*c = sum_{j<32} (a_j - a_j')*d_j + (b_j + b_j')*c_j        V3 x d + V4 x c

four real GEMMs of K = 32 per span as in the Gauss fold (whose third sum stays at K = 64):
4 units x 4 tiles x 3 (lo*hi, hi*lo, hi*hi) = 48 v_mfma_f32_16x16x32_f16, summed straight into two
product tile sets (Re: units 0 and 1, Im: units 2 and 3).  The rotation with the span phasor
P = w^(64*s + 31.5) is the plain complex multiply

    acc_r += Pr*Re - Pi*Im        acc_i += Pi*Re + Pr*Im

64 v_fma_f32 per span where the Gauss fold takes 96.  Only the images of c and d are needed (-d is
in the sign of V2): a0..a31.

Ring, slot image (16 KiB: piece 4*unit + 2*sp + rh, written by ddc_convert4f_kernel), LDS-DMA
pieces, fragment reads, scalar registers, the P rows (float4 per tone, of which Pr and Pi are
read) and the epilogue are those of the Gauss fold: the frame of tools/ddc_mfma_pframe.py.

Schedule of a span (48 gaps, one behind each MFMA), unit u at gaps 12u .. 12u+11:
  * Re is final three MFMAs after gap 23 and rewritten from gap 0 of the next span: its 32 FMAs lie
    in gaps 26..46.  Im is final three MFMAs after gap 47 and rewritten from gap 24 of the next
    span: the 32 FMAs of the span BEFORE, with that span's P, lie in gaps 2..22;
  * each group of 32 sweeps acc_r, then acc_i: an accumulator is read again 32 FMAs after it was
    written;
  * fragment reads, image copies (gaps 2, 10, 18, 26), the P load (gap 28, into the other
    parity's registers, last read in gap 22 and first used in gap 26 of the next span) and the ring
    rotation are placed as in the Gauss fold.

    python3 tools/gen_ddc_mfma_ring16p4f.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p4f_gen.h
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddc_mfma_pframe import Loop, print_loop   # noqa: E402

NU = 4                     # operand units V1..V4
NG = 12 * NU               # MFMAs per span

# ---- register map ------------------------------------------------------------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48)    # products Re, Im
F0 = VB + 64               # operand fragment (unit, rh, sp) at v[F0 + 16*unit + 8*sp + 4*rh : +3]
P = {"A": VB + 128, "B": VB + 136}   # (Pr, Pi, -, -) of tone half 0, of tone half 1
ADDR = {"A": (VB + 144, VB + 145), "B": (VB + 146, VB + 147)}
V_LAST = VB + 147
NAGPR = 32
BF = [56, 66]              # scalar bases of the 8 phasor images, 4 KiB apart (prologue)
ROT_RE = (26, 46)          # gaps of the FMAs of this span's Re
ROT_IM = (2, 22)           # gaps of the FMAs of the Im of the span before
G_PLOAD = 28


def rotation(p_cur, p_prev):
    """[(gap, kind, v_fma_f32)]: Im of the span before, then Re of this one."""
    placed = []
    for kind, prod, p, (g0, g1) in (("rot", 1, p_prev, ROT_IM), ("rotp", 0, p_cur, ROT_RE)):
        ops = LOOP.rotate_ops(prod, p)
        placed += [(g0 + (k * (g1 - g0 + 1)) // len(ops), kind, op) for k, op in enumerate(ops)]
    for k, (g, _, _) in enumerate(placed):
        # a product is final three MFMAs ago and not rewritten for two more
        lo, hi = ((NG - 1 + 3 - NG, 24 - 2), (23 + 3, NG - 2))[k // 32]
        assert lo <= g <= hi, (k, g)
    # the registers of p_prev are loaded anew at G_PLOAD
    assert max(g for g, kind, _ in placed if kind == "rot") < G_PLOAD - 2
    return placed


LOOP = Loop(noun="span", units=NU,
            prod=(0, 0, 1, 1),                               # the product a unit sums into: Re, Re, Im, Im
            image=(0, 1, 1, 0),                              # the phasor image a unit multiplies by: c, d, d, c
            split=((1, 0), (0, 1), (0, 0)),                  # lo*hi, hi*lo, hi*hi: small terms first
            read_at={(0, 1): -10, (1, 1): -8, (0, 0): -4, (1, 0): -2},     # as in the Gauss fold
            coef=(("r", "i"), ("-i", "r")),                  # Re, Im
            late=1, g_pload=G_PLOAD,
            rotation=rotation, vb=VB, acc=ACC, kb=KB, f0=F0, p=P, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P4F", __file__,
               "Main loop of ddc_mfma_ring16p4f_kernel (four real products per complex multiply over 64-sample spans folded about their centre: four K=32 operand units per span, two product tile sets)")


if __name__ == "__main__":
    main()
