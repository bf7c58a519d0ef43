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
read) and the epilogue are those of the Gauss fold, imported from its generator and from the ones
it builds on.

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
from ddc_mfma_gen import Counters, ar, print_header, vr   # noqa: E402
from gen_ddc_mfma_ring16p3 import (ABLATE, S_BF, S_K, S_M0, S_NHI1, S_NLEFT, S_PSTRIDE, S_RD, S_RD2, S_RDN,   # noqa: E402
                                   S_T0, S_WR, S_WRS, S_XB, SB, SGPR_CLOBBER, dma_ops, p_loads)
from gen_ddc_mfma_ring16p3r2 import READ_AT, first_use, last_use, mfma_of   # noqa: E402
from gen_ddc_mfma_ring16p3f import NG, NSLOT, NU, SLOT, image_pointer, piece   # noqa: E402

PROD = (0, 0, 1, 1)        # the product a unit sums into: Re, Re, Im, Im
IMAGE = (0, 1, 1, 0)       # the phasor image a unit multiplies by: c, d, d, c

# ---- register map ------------------------------------------------------------
VB = 12                    # v0..v11 stay with the compiler
ACC = (VB + 0, VB + 16)    # accumulators re, im
KB = (VB + 32, VB + 48)    # products Re, Im
F0 = VB + 64               # operand fragment (unit, rh, sp) at v[F0 + 16*unit + 8*sp + 4*rh : +3]
P = {"A": VB + 128, "B": VB + 136}   # (Pr, Pi, -, -) of tone half 0, of tone half 1
ADDR = {"A": (VB + 144, VB + 145), "B": (VB + 146, VB + 147)}
V_LAST = VB + 147
NAGPR = 32
BF = [S_BF, 66]            # scalar bases of the 8 phasor images, 4 KiB apart (prologue)
ROT_RE = (26, 46)          # gaps of the FMAs of this span's Re
ROT_IM = (2, 22)           # gaps of the FMAs of the Im of the span before
G_PLOAD = 28

assert V_LAST + 1 + NAGPR <= 256 and not (set(BF) | {b + 1 for b in BF}) - set(SGPR_CLOBBER)


def frag(unit, rh, sp):
    return F0 + 16 * unit + 8 * sp + 4 * rh


def bfrag(unit, th, sp):
    return ar(((IMAGE[unit] * 2 + th) * 2 + sp) * 4)


def rotate_ops(prod, p):
    """The two FMAs per accumulator element that product `prod` (0: Re, 1: Im) feeds: 32 v_fma_f32
    in two sweeps (an accumulator is read again 32 instructions after it was written)."""
    ops = []
    for part in range(2):                # 0: acc_r, 1: acc_i
        for i in range(16):
            th = (i >> 2) & 1            # register i belongs to tile (rh, th) = (i >> 3, (i >> 2) & 1)
            pr, pi = vr(p + 4 * th), vr(p + 4 * th + 1)
            acc = vr(ACC[part] + i)
            k = vr(KB[prod] + i)
            coef = ((pr, pi), ("-" + pi, pr))[prod][part]
            ops.append(f"v_fma_f32 {acc}, {coef}, {k}, {acc}")
    return ops


def rotation(p_cur, p_prev):
    """[(gap, kind, v_fma_f32)]: Im of the span before, then Re of this one."""
    placed = []
    for kind, prod, p, (g0, g1) in (("rot", 1, p_prev, ROT_IM), ("rotp", 0, p_cur, ROT_RE)):
        ops = rotate_ops(prod, p)
        placed += [(g0 + (k * (g1 - g0 + 1)) // len(ops), kind, op) for k, op in enumerate(ops)]
    for k, (g, _, _) in enumerate(placed):
        # a product is final three MFMAs ago and not rewritten for two more
        lo, hi = ((NG - 1 + 3 - NG, 24 - 2), (23 + 3, NG - 2))[k // 32]
        assert lo <= g <= hi, (k, g)
    # the registers of p_prev are loaded anew at G_PLOAD
    assert max(g for g, kind, _ in placed if kind == "rot") < G_PLOAD - 2
    return placed


def span(cnt, out, label):
    """One span of 64 samples: 48 MFMAs.  Span s computes from ring slot RD, prefetches span s+1's
    first fragments from RDN and starts the copy of span s+3's image into slot WR (free since the
    barrier that ended s-1)."""
    out.append(f"; ---- span, parity {label}")
    other = "B" if label == "A" else "A"
    p_cur, p_prev = P[label], P[other]
    S_P, N_P = SB[label]["p"], SB[other]["p"]
    gaps = {g: [] for g in range(NG)}
    V_RD, V_RDN = ADDR[label]
    N_RD, N_RDN = ADDR[other]

    last_rd = None
    for unit in (1, 2, 3, 0):
        for (rh, sp), rel in READ_AT.items():
            g = (12 * unit if unit else NG) + rel
            lu, fu = last_use(unit, rh, sp), first_use(unit, rh, sp)
            if unit == 0:
                assert g - lu >= 23 and NG + fu - g >= 8, (unit, rh, sp)
            else:
                assert NG + g - lu >= 23 and fu - g >= 8, (unit, rh, sp)
                last_rd = f"f{unit}{rh}{sp}"
            gaps[g].append(("lds", f"ds_read_b128 {vr(frag(unit, rh, sp), 4)}, {vr(V_RD if unit else V_RDN)} "
                            f"offset:{piece(unit, rh, sp)}", f"f{unit}{rh}{sp}"))
    # image of span s+3 -> slot WR: pointer (this parity's set) in gaps 0..1, the four pieces at
    # gaps 2, 10, 18, 26
    for i, sx in enumerate(image_pointer(label)):
        gaps[i // 3].append(("salu", sx, None))
    for which in range(4):
        for tx in dma_ops(label, S_WR, which):
            gaps[2 + 8 * which].append(("dma" if tx.startswith("global") else "salu", tx, f"d{which}{label}"))
    # P of span s+1 into the other parity's registers
    for tx in p_loads(p_prev, S_P):
        gaps[G_PLOAD].append(("vm", tx, "p" + other))
    gaps[G_PLOAD + 1].append(("salu", f"s_add_u32 s{N_P}, s{S_P}, s{S_PSTRIDE}", None))
    gaps[G_PLOAD + 1].append(("salu", f"s_addc_u32 s{N_P + 1}, s{S_P + 1}, 0", None))
    for g, kind, op in rotation(p_cur, p_prev):
        gaps[g].append((kind, op, None))
    # ring slot rotation (four slots) and the read addresses of the next span, once every ring
    # access of this one has been issued (gap 46)
    gaps[46].append(("salu", f"s_mov_b32 s{S_T0}, s{S_RD}", None))
    gaps[46].append(("salu", f"s_mov_b32 s{S_RD}, s{S_RDN}", None))
    gaps[46].append(("salu", f"s_mov_b32 s{S_RDN}, s{S_RD2}", None))
    gaps[47].append(("salu", f"s_mov_b32 s{S_RD2}, s{S_WR}", None))
    gaps[47].append(("salu", f"s_mov_b32 s{S_WR}, s{S_T0}", None))
    gaps[47].append(("addr", f"v_add_u32 {vr(N_RD)}, s{S_RD}, %[lane16]", None))
    gaps[47].append(("addr", f"v_add_u32 {vr(N_RDN)}, s{S_RDN}, %[lane16]", None))

    waited_p = False
    for g in range(NG):
        unit, m = divmod(g, 12)
        rh, th, sp_a, sp_b = mfma_of(m)
        if first_use(unit, rh, sp_a) == g:
            cnt.need_lgkm(f"f{unit}{rh}{sp_a}")
        dst = KB[PROD[unit]] + 4 * (2 * rh + th)
        src_c = "0" if unit in (0, 2) and m < 4 else vr(dst, 4)
        if "mfma" not in ABLATE:
            out.append(f"v_mfma_f32_16x16x32_f16 {vr(dst, 4)}, {vr(frag(unit, rh, sp_a), 4)}, "
                       f"{bfrag(unit, th, sp_b)}, {src_c}")
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
            elif kind in ("rot", "rotp"):
                if kind == "rotp" and not waited_p:
                    cnt.need_vm("p" + label)      # loaded one span ago
                    waited_p = True
                if "rot" not in ABLATE:
                    out.append(text)
            else:
                out.append(text)
    # the image this wave started one span ago (span s+2's) must have landed before the barrier
    # publishes it: span s+1 prefetches from it (the wait for P has covered it already)
    cnt.need_vm("d3" + other)
    # every read of THIS span's slot has returned (the barrier frees it for the copy of span s+4); the
    # prefetch of span s+1's first fragments (gaps 38..46, from the next slot) stays in flight across it
    cnt.need_lgkm(last_rd)
    if "bar" not in ABLATE:
        out.append("s_barrier")


def generate():
    out = []
    cnt = Counters(out)
    o = out.append
    o("; ===== prologue =====")
    o(f"s_mov_b32 s{S_M0}, m0")
    o(f"s_mov_b32 s{S_XB}, %[ib_lo]")          # image base of this row tile, span 0
    o(f"s_mov_b32 s{S_XB + 1}, %[ib_hi]")
    o(f"s_mov_b32 s{S_WRS}, %[wrs]")
    o(f"s_mov_b32 s{SB['B']['p']}, %[pp_lo]")
    o(f"s_mov_b32 s{SB['B']['p'] + 1}, %[pp_hi]")
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
    # P of span 0 (parity A) through parity B's pointer; parity A's pointer is span 1's
    o(f"s_add_u32 s{SB['A']['p']}, s{SB['B']['p']}, s{S_PSTRIDE}")
    o(f"s_addc_u32 s{SB['A']['p'] + 1}, s{SB['B']['p'] + 1}, 0")
    o("s_nop 4")
    out.extend(p_loads(P["A"], SB["B"]["p"]))
    for f in range(NAGPR // 4):
        b = BF[f // 4]
        if "bimg" not in ABLATE:
            o(f"global_load_dwordx4 {ar(4 * f)}, %[bo], s[{b}:{b + 1}] offset:{(f % 4) * 1024}")
    # the first span rotates "Im of the span before": 0, with P = 0
    for base in (KB[1], ACC[0], ACC[1]):
        for i in range(16):
            o(f"v_mov_b32 {vr(base + i)}, 0")
    for i in range(8):
        o(f"v_mov_b32 {vr(P['B'] + i)}, 0")
    # images of spans 0, 1, 2 into slots 0, 1, 2 (pointer sets A, B, C: one per image)
    for par, slot in (("A", S_RD), ("B", S_RDN), ("C", S_RD2)):
        out.extend(image_pointer(par))
        for which in range(4):
            o("s_nop 4")
            out.extend(dma_ops(par, slot, which))
        o("s_nop 4")
    V_RD, V_RDN = ADDR["A"]
    o(f"v_add_u32 {vr(V_RD)}, s{S_RD}, %[lane16]")
    o(f"v_add_u32 {vr(V_RDN)}, s{S_RDN}, %[lane16]")
    o("s_waitcnt vmcnt(0)")          # P of span 0, the phasor images and the three slot images
    o("s_barrier")
    for rh, sp in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o(f"ds_read_b128 {vr(frag(0, rh, sp), 4)}, {vr(V_RD)} offset:{piece(0, rh, sp)}")
    o("s_waitcnt lgkmcnt(0)")
    cnt.lgkm = []

    def trip(out_, cnt_):
        span(cnt_, out_, "A")
        out_.append(f"s_sub_u32 s{S_NLEFT}, s{S_NLEFT}, 1")
        out_.append(f"s_cmp_eq_u32 s{S_NLEFT}, 0")
        out_.append("s_cbranch_scc1 2f")
        span(cnt_, out_, "B")
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
    o(f"; ===== main loop, two spans per trip; vm, lgkm at the top: {state}")
    o("1:")
    trip(out, cnt)
    assert (cnt.vm, cnt.lgkm) == state, (cnt.lgkm, cnt.vm, state)
    # Im of the last span is still to be rotated, with that span's P
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(rotate_ops(1, P["B"]))
    o("s_branch 3f")
    o("2:")
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(rotate_ops(1, P["A"]))
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
    print_header("GSDR_MFMA_RING16P4F", __file__,
                 "Main loop of ddc_mfma_ring16p4f_kernel (four real products per complex multiply over 64-sample spans folded about their centre: four K=32 operand units per span, two product tile sets)",
                 generate(), vb=VB, v_last=V_LAST, nagpr=NAGPR, sgprs=SGPR_CLOBBER, nbytes=NSLOT * SLOT, slot=SLOT)


if __name__ == "__main__":
    main()
