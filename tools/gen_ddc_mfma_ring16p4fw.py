#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p4fw_gen.h: main loop of ddc_mfma_ring16p4fw_kernel
(gfx950) -- the direct folded loop of tools/gen_ddc_mfma_ring16p4f.py on a wave tile of 16 rows x 64
tones instead of 32 x 32.

The arithmetic is that loop's: the same four operand units V1..V4 of K = 32 per 64-sample span, the
same images c and d, per output element the same MFMAs in the same (unit, split) order and the same
rotation.  What changes is which elements a wave holds: tile q = tone quarter 0..3 of ONE row half,
so an operand fragment (two ds_read_b128, hi and lo) feeds twelve MFMAs instead of six, and a
workgroup of four waves (16 rows x 256 tones) needs only the eight 1-KiB pieces of its row half:

  * ring: four slots of 8 KiB, piece 2*unit + sp inside a slot; a wave copies two pieces per span
    (unit = wave: hi, lo).  The slot image in memory is the unchanged 16 KiB of
    ddc_convert4f_kernel, piece 4*unit + 2*sp + rh: the kernel's DMA offsets select rh;
  * phasor images: a[((tile32*2 + image)*2 + th)*2 + sp], 64 AGPRs, tile32 = q >> 1, th = q & 1:
    the 8 + 8 KiB of two 32-tone tiles, the second through its own offset operand (a wave whose
    second tile does not exist is given a copy of the last one);
  * P: Pr, Pi of four tone quarters per parity, four global_load_dwordx2 from the float4 rows;
  * eight fragment reads per span; 48 MFMAs, 64 rotation FMAs, one barrier as before.

Schedule of a span: that of the 32 x 32 loop (Re rotated in gaps 26..46, the Im of the span before
in gaps 2..22, P loaded at gap 28), image copies at gaps 2 and 10, fragment (unit, lo) read 10 gaps
ahead of its unit and (unit, hi) 4 gaps ahead: 8 or more gaps before the first use, 33 or more
MFMAs behind the last.

    python3 tools/gen_ddc_mfma_ring16p4fw.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p4fw_gen.h
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
F0 = VB + 64               # operand fragment (unit, sp) at v[F0 + 8*unit + 4*sp : +3]
P = {"A": VB + 96, "B": VB + 104}    # (Pr, Pi) of tone quarters 0..3
ADDR = {"A": (VB + 112, VB + 113), "B": (VB + 114, VB + 115)}
V_LAST = VB + 115
NAGPR = 64
BF = [56, 66]              # scalar bases of the 8 phasor images of a 32-tone tile, 4 KiB apart (prologue)
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


LOOP = Loop(noun="span", units=NU, rows=1, tq=4,             # 16 rows x 64 tones per wave
            prod=(0, 0, 1, 1),                               # the product a unit sums into: Re, Re, Im, Im
            image=(0, 1, 1, 0),                              # the phasor image a unit multiplies by: c, d, d, c
            split=((1, 0), (0, 1), (0, 0)),                  # lo*hi, hi*lo, hi*hi: small terms first
            read_at={(0, 1): -10, (0, 0): -4},               # lo, hi
            coef=(("r", "i"), ("-i", "r")),                  # Re, Im
            late=1, g_pload=G_PLOAD,
            rotation=rotation, vb=VB, acc=ACC, kb=KB, f0=F0, p=P, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P4FW", __file__,
               "Main loop of ddc_mfma_ring16p4fw_kernel (the direct folded loop on a wave tile of 16 rows x 64 tones: four K=32 operand units per span, two product tile sets, half the operand traffic)")


if __name__ == "__main__":
    main()
