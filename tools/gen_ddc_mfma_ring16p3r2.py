#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p3r2_gen.h: main loop of ddc_mfma_ring16p3r2_kernel
(gfx950) -- the three-product ring loop of tools/gen_ddc_mfma_ring16p3.py with the rotation
acc += P*K done once per PAIR of blocks (64 samples) instead of once per block (DESIGN.md
section 4.1e).

The B operand (phasor images c, d-c, c+d) covers 64 samples: a0..a47 the samples 0..31 of a pair,
a48..a95 the samples 32..63.  The MFMAs of the first block of a pair start from 0, those of the
second block accumulate onto the same K registers, and the pair's phasor P = w^(64*p) turns the
sums once: 96 v_fma_f32 per pair instead of 192.  Ring, slot images, LDS-DMA pieces and the
epilogue are those of the 32-sample loop (the frame of tools/ddc_mfma_pframe.py); so is the
register map, stated again below.

One trip = one pair = 72 gaps (one behind each MFMA), first block X in gaps 0..35, second block Y
in gaps 36..71; component c of a block at its gaps 12c..12c+11:
  * K of component c is final after gap 47 + 12c and rewritten from gap 72 + 12c (gap 12c of the
    next trip) on.  The 96 FMAs -- components 0, 1, 2 in that order, acc_r then acc_i of each, so
    that an accumulator is read again 32 instructions after it was written -- are laid evenly over
    gaps 50..93: component 0 in 50..64, 1 in 64..78, 2 in 79..93.  Gaps 72..93 are gaps 0..21 of
    the NEXT trip's X block (the first trip finds K = 0 there);
  * P of pair p+1 is loaded into a staging set (PN) at gap 28 and moved to P at gaps 24..25 of
    the next trip, behind the last FMA that read pair p's (gap 21) and 24 MFMAs ahead of the first
    that reads pair p+1's (gap 50): the load has 68 MFMAs to land;
  * image copies (three pieces per block at gaps 2, 10, 18), the ring rotation and the per-parity
    address / scalar-base sets (R2) are those of the 32-sample loop: X is its parity A, Y its
    parity B.  The three splits of a component run lo*hi, hi*lo, hi*hi (small terms first: fewer
    fp32 roundings at the size of K), and the fragment reads are placed for that order;
  * odd block counts leave the trip after X (label 2): all 96 FMAs follow with that pair's P (the
    B images of samples 0..31 were used, the sums are those of a 32-sample block).  An even count
    leaves after Y: the FMAs of gaps 72..93 follow.

    python3 tools/gen_ddc_mfma_ring16p3r2.py > gpu_sdr_amd/csrc/ddc_mfma_ring16p3r2_gen.h
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddc_mfma_pframe import SB, S_PSTRIDE, Loop, p_loads, print_loop   # noqa: E402
from ddc_mfma_gen import vr   # noqa: E402

NC = 3                     # components: a+b, a, b
NG = 12 * NC               # MFMAs per block
NT = 2 * NG                # gaps per trip

# ---- register map: that of the 32-sample loop, with its two parity sets of P as P and PN -------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48, VB + 64)   # products K1, K2, K3
F0 = VB + 80               # operand fragment (comp, rh, sp) at v[F0 + 16*comp + 8*sp + 4*rh : +3]
P = VB + 128               # (Pr, Pi, Pr-Pi, Pr+Pi) of tone half 0, of tone half 1: the pair being rotated
PN = VB + 136              # the next pair's, as loaded
ADDR = {"A": (VB + 144, VB + 145), "B": (VB + 146, VB + 147)}
V_LAST = VB + 147
NAGPR = 2 * 16 * NC        # B images of 64 samples
S_P = SB["A"]["p"]         # s[40:41]: P row of the next pair
BF = [56, 66, 68, 70, 38, 48]      # scalar bases of the 24 phasor images, 4 KiB apart (prologue)
ROT0, ROT1 = 50, 93        # the FMAs of a pair lie in gaps ROT0..ROT1
G_PMOVE, G_PLOAD, G_PNEXT = 24, 28, 44

assert F0 + 48 == P and ADDR["B"][1] == V_LAST


class PairLoop(Loop):
    """X is parity A, Y parity B; one P pointer, P loaded into PN and moved"""
    s_p0 = S_P

    def acc_base(self, label):
        return 48 * (label == "B")

    def from_zero(self, label):
        return label == "A"

    def pair_rotation(self):
        """[(gap 50..93, v_fma_f32)]: 96 FMAs, two per accumulator element and component."""
        ops = [op for comp in range(NC) for op in self.rotate_ops(comp, P)]
        n = len(ops)
        placed = [(ROT0 + (k * (ROT1 - ROT0 + 1)) // n, op) for k, op in enumerate(ops)]
        for k, (g, _) in enumerate(placed):
            comp = k // 32
            # K final three MFMAs ago, not rewritten for two more; P moved before, not again until after
            assert NG + 12 * comp + 11 + 3 <= g <= NT + 12 * comp - 2 and G_PMOVE + 1 < g < NT + G_PMOVE - 2
        return placed

    def p_prologue(self):
        # P of pair 0 into the staging set (the first trip moves it), then the pointer goes on to pair 1;
        # the first trip rotates "the pair before": K = 0, P = 0
        return (["s_nop 4"] + p_loads(PN, S_P),
                [f"s_add_u32 s{S_P}, s{S_P}, s{S_PSTRIDE}", f"s_addc_u32 s{S_P + 1}, s{S_P + 1}, 0"], list(KB), P)

    def p_schedule(self, label):
        half = "AB".index(label)
        if half == 0:
            # this pair's P out of the staging set (loaded one trip ago), then the next pair's into it
            items = [(G_PMOVE + j // 4, "pmove", f"v_mov_b32 {vr(P + j)}, {vr(PN + j)}", "pn") for j in range(8)] + \
                    [(G_PLOAD, "vm", tx, "pn") for tx in p_loads(PN, S_P)]
        else:
            items = [(G_PNEXT - NG, "salu", f"s_add_u32 s{S_P}, s{S_P}, s{S_PSTRIDE}", None),
                     (G_PNEXT - NG, "salu", f"s_addc_u32 s{S_P + 1}, s{S_P + 1}, 0", None)]
        return items + [(g % NG, "rot", op, None) for g, op in self.pair_rotation() if g // NG % 2 == half]

    def tail(self, label):
        # an even count leaves after Y: what the next trip's X block would have rotated.  An odd count: the
        # last pair is its X block alone, nothing of it has been rotated
        return [op for g, op in self.pair_rotation() if g >= NT or label == "A"]


LOOP = PairLoop(noun="block", units=NC, prod=(0, 1, 2), image=(0, 1, 2),
                # the two small cross terms (2^-11 of the main one) are summed first, so that a block adds onto a
                # large K with fp32 rounding once where the order hi*hi, hi*lo, lo*hi of the 32-sample loop does
                # it three times
                split=((1, 0), (0, 1), (0, 0)),              # lo*hi, hi*lo, hi*hi
                # the lo fragments (used by the first four MFMAs only) first, the hi fragments in the one gap that
                # is 23 MFMAs behind their last use (R1) and 8 ahead of their first
                read_at={(0, 1): -10, (1, 1): -8, (0, 0): -4, (1, 0): -2},
                coef=(("m", "p"), ("-i", "r"), ("-r", "-i")),    # K1, K2, K3; m = Pr-Pi, p = Pr+Pi
                vb=VB, acc=ACC, kb=KB, f0=F0, addr=ADDR, v_last=V_LAST, nagpr=NAGPR, bf=BF)


def main():
    print_loop(LOOP, "GSDR_MFMA_RING16P3R2", __file__,
               "Main loop of ddc_mfma_ring16p3r2_kernel (the three-product loop of ddc_mfma_ring16p3_gen.h with phasor images of 64 samples: one rotation per pair of blocks)")


if __name__ == "__main__":
    main()
