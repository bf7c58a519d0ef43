#!/usr/bin/env python3
"""Generates gpu_sdr_amd/csrc/ddc_mfma_ring16p3r2_gen.h: main loop of ddc_mfma_ring16p3r2_kernel
(gfx950) -- the three-product ring loop of tools/gen_ddc_mfma_ring16p3.py with the rotation
acc += P*K done once per PAIR of blocks (64 samples) instead of once per block (DESIGN.md
section 4.1e).

The B operand (phasor images c, d-c, c+d) covers 64 samples: a0..a47 the samples 0..31 of a pair,
a48..a95 the samples 32..63.  The MFMAs of the first block of a pair start from 0, those of the
second block accumulate onto the same K registers, and the pair's phasor P = w^(64*p) turns the
sums once: 96 v_fma_f32 per pair instead of 192.  Ring, slot images, LDS-DMA pieces, register
map and the epilogue are those of the 32-sample loop (imported from its generator).

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
from ddc_mfma_gen import Counters, ar, print_header, vr   # noqa: E402
from gen_ddc_mfma_ring16p3 import (ABLATE, ACC, ADDR, F0, KB, NC, NG, NSLOT, S_BF, S_K, S_M0, S_NHI1, S_NLEFT,   # noqa: E402
                                   S_PSTRIDE, S_RD, S_RD2, S_RDN, S_T0, S_WR, S_WRS, S_XB, SB, SGPR_CLOBBER, SLOT, VB,
                                   dma_ops, frag, image_pointer, piece)

# ---- register map: that of the 32-sample loop, with its two parity sets of P as P and PN -------
P = VB + 128               # (Pr, Pi, Pr-Pi, Pr+Pi) of tone half 0, of tone half 1: the pair being rotated
PN = VB + 136              # the next pair's, as loaded
V_LAST = VB + 147
NVGPR_CLOBBER = list(range(VB, V_LAST + 1))
NAGPR = 2 * 16 * NC        # B images of 64 samples
S_P = SB["A"]["p"]         # s[40:41]: P row of the next pair
BF = [S_BF, 66, 68, 70, 38, 48]    # scalar bases of the 24 phasor images, 4 KiB apart (prologue)
NT = 2 * NG                # gaps per trip
ROT0, ROT1 = 50, 93        # the FMAs of a pair lie in gaps ROT0..ROT1
G_PMOVE, G_PLOAD, G_PNEXT = 24, 28, 44

assert F0 + 48 == P and ADDR["B"][1] == V_LAST and not (set(BF) | {b + 1 for b in BF}) - set(SGPR_CLOBBER)


# MFMA m of a component: split m // 4, tile m % 4 = 2*rh + th.  The splits run lo*hi, hi*lo, hi*hi: the two small
# cross terms (2^-11 of the main one) are summed first, so that a block adds onto a large K with fp32 rounding once
# where the order hi*hi, hi*lo, lo*hi of the 32-sample loop does it three times.
def mfma_of(m):
    s, t = divmod(m, 4)
    return (t >> 1, t & 1) + ((1, 0), (0, 1), (0, 0))[s]    # rh, th, sp_a, sp_b


def first_use(comp, rh, sp):
    return min(12 * comp + m for m in range(12) if mfma_of(m)[0] == rh and mfma_of(m)[2] == sp)


def last_use(comp, rh, sp):
    return max(12 * comp + m for m in range(12) if mfma_of(m)[0] == rh and mfma_of(m)[2] == sp)


# gap of the ds_read of fragment (rh, sp) relative to the first gap of its component: the lo fragments (used by the
# first four MFMAs only) first, the hi fragments in the one gap that is 23 MFMAs behind their last use (R1) and 8
# ahead of their first
READ_AT = {(0, 1): -10, (1, 1): -8, (0, 0): -4, (1, 0): -2}


def bfrag(half, comp, th, sp):
    return ar(48 * half + ((comp * 2 + th) * 2 + sp) * 4)


def rotation():
    """[(gap 50..93, v_fma_f32)]: 96 FMAs, two per accumulator element and component."""
    ops = []
    for comp in range(NC):
        for part in range(2):                # 0: acc_r, 1: acc_i
            for i in range(16):
                th = (i >> 2) & 1            # register i belongs to tile (rh, th) = (i >> 3, (i >> 2) & 1)
                pr, pi, pm, pp = (vr(P + 4 * th + j) for j in range(4))
                acc = vr(ACC[part] + i)
                k = vr(KB[comp] + i)
                coef = ((pm, pp), ("-" + pi, pr), ("-" + pr, "-" + pi))[comp][part]
                ops.append(f"v_fma_f32 {acc}, {coef}, {k}, {acc}")
    n = len(ops)
    placed = [(ROT0 + (k * (ROT1 - ROT0 + 1)) // n, op) for k, op in enumerate(ops)]
    for k, (g, _) in enumerate(placed):
        comp = k // 32
        # K final three MFMAs ago, not rewritten for two more; P moved before, not again until after
        assert NG + 12 * comp + 11 + 3 <= g <= NT + 12 * comp - 2 and G_PMOVE + 1 < g < NT + G_PMOVE - 2
    return placed


def p_loads(dst):
    return [f"global_load_dwordx4 {vr(dst, 4)}, %[po], s[{S_P}:{S_P + 1}]",
            f"global_load_dwordx4 {vr(dst + 4, 4)}, %[po], s[{S_P}:{S_P + 1}] offset:256"]


def block(cnt, out, half):
    """One block of 32 samples, 36 MFMAs: half 0 = X (first of its pair, parity set A), 1 = Y (B).
    Block b computes from ring slot RD, prefetches block b+1's first fragments from RDN and starts
    the copy of block b+3's image into slot WR (free since the barrier that ended b-1)."""
    label, other = ("A", "B") if half == 0 else ("B", "A")
    out.append(f"; ---- block {'XY'[half]} of the pair, parity {label}")
    gaps = {g: [] for g in range(NG)}
    V_RD, V_RDN = ADDR[label]
    N_RD, N_RDN = ADDR[other]

    last_rd = None
    for comp, slot_reg in ((1, V_RD), (2, V_RD), (0, V_RDN)):
        for (rh, sp), rel in READ_AT.items():
            g = (12 * comp if comp else NG) + rel
            lu, fu = last_use(comp, rh, sp), first_use(comp, rh, sp)
            if comp == 0:
                assert g - lu >= 23 and NG + fu - g >= 8, (comp, rh, sp)
            else:
                assert NG + g - lu >= 23 and fu - g >= 8, (comp, rh, sp)
                last_rd = f"f{comp}{rh}{sp}"
            gaps[g].append(("lds", f"ds_read_b128 {vr(frag(comp, rh, sp), 4)}, {vr(slot_reg)} offset:{piece(comp, rh, sp)}",
                            f"f{comp}{rh}{sp}"))
    for i, sx in enumerate(image_pointer(label)):
        gaps[i // 3].append(("salu", sx, None))
    for which in range(3):
        for tx in dma_ops(label, S_WR, which):
            gaps[2 + 8 * which].append(("dma" if tx.startswith("global") else "salu", tx, f"d{which}{label}"))
    if half == 0:
        # this pair's P out of the staging set, then the next pair's into it
        for j in range(8):
            gaps[G_PMOVE + j // 4].append(("pmove", f"v_mov_b32 {vr(P + j)}, {vr(PN + j)}", None))
        for tx in p_loads(PN):
            gaps[G_PLOAD].append(("vm", tx, "pn"))
    else:
        gaps[G_PNEXT - NG].append(("salu", f"s_add_u32 s{S_P}, s{S_P}, s{S_PSTRIDE}", None))
        gaps[G_PNEXT - NG].append(("salu", f"s_addc_u32 s{S_P + 1}, s{S_P + 1}, 0", None))
    for g, op in rotation():
        if g // NG % 2 == half:
            gaps[g % NG].append(("rot", op, None))
    # ring slot rotation (four slots) and the read addresses of the next block, once every ring
    # access of this one has been issued (gap 34)
    gaps[34].append(("salu", f"s_mov_b32 s{S_T0}, s{S_RD}", None))
    gaps[34].append(("salu", f"s_mov_b32 s{S_RD}, s{S_RDN}", None))
    gaps[34].append(("salu", f"s_mov_b32 s{S_RDN}, s{S_RD2}", None))
    gaps[35].append(("salu", f"s_mov_b32 s{S_RD2}, s{S_WR}", None))
    gaps[35].append(("salu", f"s_mov_b32 s{S_WR}, s{S_T0}", None))
    gaps[35].append(("addr", f"v_add_u32 {vr(N_RD)}, s{S_RD}, %[lane16]", None))
    gaps[35].append(("addr", f"v_add_u32 {vr(N_RDN)}, s{S_RDN}, %[lane16]", None))

    waited_p = False
    for g in range(NG):
        comp, m = divmod(g, 12)
        rh, th, sp_a, sp_b = mfma_of(m)
        if first_use(comp, rh, sp_a) == g:
            cnt.need_lgkm(f"f{comp}{rh}{sp_a}")
        dst = KB[comp] + 4 * (2 * rh + th)
        src_c = "0" if half == 0 and m < 4 else vr(dst, 4)
        if "mfma" not in ABLATE:
            out.append(f"v_mfma_f32_16x16x32_f16 {vr(dst, 4)}, {vr(frag(comp, rh, sp_a), 4)}, "
                       f"{bfrag(half, comp, th, sp_b)}, {src_c}")
        for kind, text, tag in gaps[g]:
            if kind == "lds":
                if "lds" not in ABLATE:
                    out.append(text)
                    cnt.issue_lgkm(tag)
            elif kind == "vm":
                out.append(text)
                cnt.issue_vm(tag)
            elif kind == "dma":
                if "gload" not in ABLATE:
                    out.append(text)
                    cnt.issue_vm(tag)
            elif kind == "pmove":
                if not waited_p:
                    cnt.need_vm("pn")             # loaded one trip ago
                    waited_p = True
                out.append(text)
            elif kind == "rot":
                if "rot" not in ABLATE:
                    out.append(text)
            else:
                out.append(text)
    # the image this wave started one block ago (block b+2's) must have landed before the barrier
    # publishes it: block b+1 prefetches from it
    cnt.need_vm("d2" + other)
    # every read of THIS block's slot has returned (the barrier frees it for the copy of block b+4); the
    # prefetch of block b+1's first fragments (gaps 26..34, from the next slot) stays in flight across it
    cnt.need_lgkm(last_rd)
    if "bar" not in ABLATE:
        out.append("s_barrier")


def generate():
    out = []
    cnt = Counters(out)
    o = out.append
    o("; ===== prologue =====")
    o(f"s_mov_b32 s{S_M0}, m0")
    o(f"s_mov_b32 s{S_XB}, %[ib_lo]")          # image base of this row tile, block 0
    o(f"s_mov_b32 s{S_XB + 1}, %[ib_hi]")
    o(f"s_mov_b32 s{S_WRS}, %[wrs]")
    o(f"s_mov_b32 s{S_P}, %[pp_lo]")
    o(f"s_mov_b32 s{S_P + 1}, %[pp_hi]")
    o(f"s_mov_b32 s{S_BF}, %[bf_lo]")
    o(f"s_mov_b32 s{S_BF + 1}, %[bf_hi]")
    o(f"s_mov_b32 s{S_PSTRIDE}, %[pstride]")
    o(f"s_mov_b32 s{S_NLEFT}, %[nhi]")
    o(f"s_add_u32 s{S_NHI1}, %[nhi], -1")
    o(f"s_mov_b32 s{S_K}, 0")
    o(f"s_mov_b32 s{S_RD}, 0")
    o(f"s_mov_b32 s{S_RDN}, {SLOT}")
    o(f"s_mov_b32 s{S_RD2}, {2 * SLOT}")
    o(f"s_mov_b32 s{S_WR}, {3 * SLOT}")
    o("s_nop 4")
    for j in range(1, len(BF)):
        o(f"s_add_u32 s{BF[j]}, s{S_BF}, {4096 * j}")
        o(f"s_addc_u32 s{BF[j] + 1}, s{S_BF + 1}, 0")
    o("s_nop 4")
    # P of pair 0 into the staging set (the first trip moves it); the pointer goes on to pair 1
    out.extend(p_loads(PN))
    for f in range(2 * 4 * NC):
        b = BF[f // 4]
        if "bimg" not in ABLATE:
            o(f"global_load_dwordx4 {ar(4 * f)}, %[bo], s[{b}:{b + 1}] offset:{(f % 4) * 1024}")
    # the first trip rotates "the pair before": K = 0, P = 0
    for base in (KB[0], KB[1], KB[2], ACC[0], ACC[1]):
        for i in range(16):
            o(f"v_mov_b32 {vr(base + i)}, 0")
    for i in range(8):
        o(f"v_mov_b32 {vr(P + i)}, 0")
    # images of blocks 0, 1, 2 into slots 0, 1, 2 (pointer sets A, B, C: one per image)
    for par, slot in (("A", S_RD), ("B", S_RDN), ("C", S_RD2)):
        out.extend(image_pointer(par))
        for which in range(3):
            o("s_nop 4")
            out.extend(dma_ops(par, slot, which))
        o("s_nop 4")
    V_RD, V_RDN = ADDR["A"]
    o(f"v_add_u32 {vr(V_RD)}, s{S_RD}, %[lane16]")
    o(f"v_add_u32 {vr(V_RDN)}, s{S_RDN}, %[lane16]")
    o("s_waitcnt vmcnt(0)")          # P of pair 0, the phasor images and the three slot images
    o(f"s_add_u32 s{S_P}, s{S_P}, s{S_PSTRIDE}")
    o(f"s_addc_u32 s{S_P + 1}, s{S_P + 1}, 0")
    o("s_barrier")
    for rh, sp in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o(f"ds_read_b128 {vr(frag(0, rh, sp), 4)}, {vr(V_RD)} offset:{piece(0, rh, sp)}")
    o("s_waitcnt lgkmcnt(0)")
    cnt.lgkm = []

    def trip(out_, cnt_):
        block(cnt_, out_, 0)
        out_.append(f"s_sub_u32 s{S_NLEFT}, s{S_NLEFT}, 1")
        out_.append(f"s_cmp_eq_u32 s{S_NLEFT}, 0")
        out_.append("s_cbranch_scc1 2f")
        block(cnt_, out_, 1)
        out_.append(f"s_sub_u32 s{S_NLEFT}, s{S_NLEFT}, 1")
        out_.append(f"s_cmp_lg_u32 s{S_NLEFT}, 0")
        out_.append("s_cbranch_scc1 1b")

    # outstanding operations at the top of the loop in the steady state (on entry there are none:
    # the waits derived from the steady state are then met at once)
    state = ([], [])
    for _ in range(4):
        probe = Counters([])
        probe.vm, probe.lgkm = list(state[0]), list(state[1])
        trip(probe.out, probe)
        if (probe.vm, probe.lgkm) == state:
            break
        state = (list(probe.vm), list(probe.lgkm))
    else:
        raise AssertionError("no steady state")
    cnt.vm, cnt.lgkm = list(state[0]), list(state[1])
    o(f"; ===== main loop, one pair of blocks per trip; vm, lgkm at the top: {state}")
    o("1:")
    trip(out, cnt)
    assert (cnt.vm, cnt.lgkm) == state, (cnt.lgkm, cnt.vm, state)
    rot = rotation()
    # an even count: what the next trip's X block would have rotated
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(op for g, op in rot if g >= NT)
    o("s_branch 3f")
    # an odd count: the last pair is its X block alone, nothing of it has been rotated
    o("2:")
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(op for g, op in rot)
    o("3:")
    # every image copy has landed (vmcnt(0) above) and every wave is past the last barrier: the
    # ring is idle, the accumulators go to the C++ epilogue through it
    o("s_barrier")
    for q in range(8):
        base = (ACC[0] if q < 4 else ACC[1]) + 4 * (q & 3)
        o(f"ds_write_b128 %[accaddr], {vr(base, 4)} offset:{q * 1024}")
    o("s_waitcnt lgkmcnt(0)")
    o(f"s_mov_b32 m0, s{S_M0}")
    return out


def main():
    print_header("GSDR_MFMA_RING16P3R2", __file__,
                 "Main loop of ddc_mfma_ring16p3r2_kernel (the three-product loop of ddc_mfma_ring16p3_gen.h with phasor images of 64 samples: one rotation per pair of blocks)",
                 generate(), vb=VB, v_last=V_LAST, nagpr=NAGPR, sgprs=SGPR_CLOBBER, nbytes=NSLOT * SLOT, slot=SLOT)


if __name__ == "__main__":
    main()
