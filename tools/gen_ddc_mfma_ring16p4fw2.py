#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p4fw2_gen.h: main loop of ddc_mfma_ring16p4fw2_kernel
(gfx950) -- the direct folded loop on wave tiles of 16 rows x 64 tones of
tools/gen_ddc_mfma_ring16p4fw.py over spans of 128 samples instead of 64.

A span folds about its own centre: t = j - 63.5, partner j' = 127 - j, w^t = c + i*d, c(j') = c(j),
d(j') = -d(j), 64 partner pairs per operand:

    Re = sum_{j<64} (a_j + a_j')*c_j + (b_j' - b_j)*d_j        V1 x c + V2 x d
    Im = sum_{j<64} (a_j - a_j')*d_j + (b_j + b_j')*c_j        V3 x d + V4 x c

Each V is two operand units of K = 32 (K-half 0: j = 0..31, K-half 1: j = 32..63): unit u = 2*V + K-half,
eight units and 96 MFMAs per span -- per sample what the 64-sample loop issues -- summed into the same two
product tile sets (Re: units 0..3, Im: units 4..7) and rotated by the span phasor P = w^(128*s + 63.5)
once per 128 samples: 64 v_fma_f32, four P loads, one barrier, one ring rotation and one image pointer
per 128 samples, half of what two 64-sample spans take.

  * ring: four slots of 16 KiB, piece 2*u + sp inside a slot; a wave copies four pieces per span
    (units 2*wave and 2*wave + 1: hi, lo).  The slot image in memory is the 32 KiB of
    ddc_convert4f2_kernel, piece 4*u + 2*sp + rh: the kernel's DMA offsets select rh;
  * phasor images: a[((tile32*4 + image)*2 + th)*2 + sp], image = 2*K-half + (0: c, 1: d), 128 AGPRs:
    the 16 + 16 KiB of two 32-tone tiles;
  * fragments: the 32 registers of four units; unit u takes those of unit u - 4, read 27 MFMAs after
    that unit's last MFMA;
  * P: Pr, Pi of four tone quarters per parity, as in the 64-sample loop.

Schedule of a span (96 gaps), unit u at gaps 12u .. 12u+11:
  * Re is final three MFMAs after gap 47 and rewritten from gap 0 of the next span: its 32 FMAs lie in
    gaps 50..94.  Im is final three MFMAs after gap 95 and rewritten from gap 48 of the next span: the
    32 FMAs of the span BEFORE, with that span's P, lie in gaps 2..46;
  * the P of the next span is loaded at gap 52 into the other parity's registers (last read in gap 46,
    first used in gap 50 of the next span);
  * image copies at gaps 2, 10, 18, 26; fragment (u, lo) read 10 gaps ahead of its unit, (u, hi) 4.

    python3 tools/gen_ddc_mfma_ring16p4fw2.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p4fw2_gen.h
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddc_mfma_pframe import Loop, print_loop   # noqa: E402

NU = 8                     # operand units: V1..V4 x K-half
NG = 12 * NU               # MFMAs per span

# ---- register map ------------------------------------------------------------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48)    # products Re, Im
F0 = VB + 64               # operand fragment (unit, sp) at v[F0 + 8*(unit % 4) + 4*sp : +3]
P = {"A": VB + 96, "B": VB + 104}    # (Pr, Pi) of tone quarters 0..3
ADDR = {"A": (VB + 112, VB + 113), "B": (VB + 114, VB + 115)}
V_LAST = VB + 115
NAGPR = 128
BF = [56, 66, 68, 70]      # scalar bases of the 16 phasor images of a 32-tone tile, 4 KiB apart (prologue)
ROT_RE = (50, 94)          # gaps of the FMAs of this span's Re
ROT_IM = (2, 46)           # gaps of the FMAs of the Im of the span before
G_PLOAD = 52


def rotation(p_cur, p_prev):
    """[(gap, kind, v_fma_f32)]: Im of the span before, then Re of this one."""
    placed = []
    for kind, prod, p, (g0, g1) in (("rot", 1, p_prev, ROT_IM), ("rotp", 0, p_cur, ROT_RE)):
        ops = LOOP.rotate_ops(prod, p)
        placed += [(g0 + (k * (g1 - g0 + 1)) // len(ops), kind, op) for k, op in enumerate(ops)]
    for k, (g, _, _) in enumerate(placed):
        # a product is final three MFMAs ago and not rewritten for two more
        lo, hi = ((NG - 1 + 3 - NG, NG // 2 - 2), (NG // 2 - 1 + 3, NG - 2))[k // 32]
        assert lo <= g <= hi, (k, g)
    # the registers of p_prev are loaded anew at G_PLOAD
    assert max(g for g, kind, _ in placed if kind == "rot") < G_PLOAD - 2
    return placed


LOOP = Loop(noun="span", units=NU, frag_units=4, rows=1, tq=4,     # 16 rows x 64 tones per wave
            prod=(0, 0, 0, 0, 1, 1, 1, 1),                   # the product a unit sums into: Re (V1, V2), Im (V3, V4)
            image=(0, 2, 1, 3, 1, 3, 0, 2),                  # 2*K-half + (c, d, d, c)[V]
            split=((1, 0), (0, 1), (0, 0)),                  # lo*hi, hi*lo, hi*hi: small terms first
            read_at={(0, 1): -10, (0, 0): -4},               # lo, hi
            coef=(("r", "i"), ("-i", "r")),                  # Re, Im
            late=1, g_pload=G_PLOAD,
            rotation=rotation, vb=VB, acc=ACC, kb=KB, f0=F0, p=P, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P4FW2", __file__,
               "Main loop of ddc_mfma_ring16p4fw2_kernel (the direct folded loop on a wave tile of 16 rows x 64 tones over 128-sample spans: eight K=32 operand units per span, two product tile sets, one rotation per 128 samples)")


if __name__ == "__main__":
    main()
