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
from ddc_mfma_gen import Counters, ar, print_header, vr   # noqa: E402

# timing-only builds (WRONG results): GEN_ABLATE=rot,lds,gload,bar,bimg,mfma as in gen_ddc_mfma_ring16p.py
ABLATE = set(filter(None, os.environ.get("GEN_ABLATE", "").split(",")))
NC = 3                     # components: a+b, a, b
SLOT = NC * 4 * 1024       # bytes of one ring slot
NSLOT = 4                  # ring slots: images arrive three blocks ahead
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
NVGPR_CLOBBER = list(range(VB, V_LAST + 1))
NAGPR = 16 * NC

# private SGPRs: scalar bases of the global loads, one set per iteration parity (never rewrite what
# a queued memory instruction reads); C: prologue only
SB = {"A": dict(x=36, p=40), "B": dict(x=60, p=64), "C": dict(x=76, p=0)}
S_NLEFT, S_K, S_NHI1 = 42, 43, 44
S_RD, S_RDN, S_WR = 45, 46, 47
S_RD2 = 72     # slot of block b+2 (between RDN and WR)
S_M0 = 73      # M0 on entry
S_WRS = 74     # wave-uniform LDS base of this wave's three image pieces
S_T0, S_T1 = 50, 51
S_XB = 52      # s[52:53] image base, block 0
S_BF = 56      # s[56:57] phasor-table images
S_PSTRIDE = 58
SGPR_CLOBBER = list(range(36, 80))


def frag(comp, rh, sp):
    return F0 + 16 * comp + 8 * sp + 4 * rh


def piece(comp, rh, sp):
    return 1024 * (4 * comp + 2 * sp + rh)


def bfrag(comp, th, sp):
    return ar(((comp * 2 + th) * 2 + sp) * 4)


def rotate_ops(comp, p):
    """The two FMAs per accumulator element that component `comp` feeds: 32 v_fma_f32 in two sweeps
    (an accumulator is read again 16 instructions after it was written)."""
    ops = []
    for part in range(2):                # 0: acc_r, 1: acc_i
        for i in range(16):
            th = (i >> 2) & 1            # register i belongs to tile (rh, th) = (i >> 3, (i >> 2) & 1)
            pr, pi, pm, pp = (vr(p + 4 * th + j) for j in range(4))
            acc = vr(ACC[part] + i)
            k = vr(KB[comp] + i)
            coef = ((pm, pp), ("-" + pi, pr), ("-" + pr, "-" + pi))[comp][part]
            ops.append(f"v_fma_f32 {acc}, {coef}, {k}, {acc}")
    return ops


# MFMA m of a component: split m // 4 (hi*hi, hi*lo, lo*hi), tile m % 4 = 2*rh + th
def mfma_of(m):
    s, t = divmod(m, 4)
    return t >> 1, t & 1, (1 if s == 2 else 0), (1 if s == 1 else 0)    # rh, th, sp_a, sp_b


def first_use(comp, rh, sp):
    return min(12 * comp + m for m in range(12) if mfma_of(m)[0] == rh and mfma_of(m)[2] == sp)


def last_use(comp, rh, sp):
    return max(12 * comp + m for m in range(12) if mfma_of(m)[0] == rh and mfma_of(m)[2] == sp)


def image_pointer(par):
    """SALU: s[SB[par].x] = image base + SLOT * min(S_K, nhi-1), then S_K += 1"""
    S_X = SB[par]["x"]
    return [
        f"s_min_u32 s{S_T0}, s{S_K}, s{S_NHI1}",
        f"s_mul_i32 s{S_T1}, s{S_T0}, {SLOT}",
        f"s_add_u32 s{S_X}, s{S_XB}, s{S_T1}",
        f"s_addc_u32 s{S_X + 1}, s{S_XB + 1}, 0",
        f"s_add_u32 s{S_K}, s{S_K}, 1",
    ]


def dma_ops(par, slot_sreg, which):
    """LDS-DMA piece `which` (0..2) of this wave of the image s[SB[par].x] into ring slot `slot_sreg`.
    M0 carries the wave-uniform LDS address; it is written right in front of its only reader and
    not again for eight MFMAs."""
    S_X = SB[par]["x"]
    return [
        f"s_add_u32 m0, s{slot_sreg}, s{S_WRS}" if which == 0 else "s_add_u32 m0, m0, 1024",
        "s_nop 0",
        f"global_load_lds_dwordx4 %[io{which}], s[{S_X}:{S_X + 1}]",
    ]


def p_loads(dst, sp_):
    return [f"global_load_dwordx4 {vr(dst, 4)}, %[po], s[{sp_}:{sp_ + 1}]",
            f"global_load_dwordx4 {vr(dst + 4, 4)}, %[po], s[{sp_}:{sp_ + 1}] offset:256"]


def iteration(cnt, out, label):
    """One block of 32 samples: 36 MFMAs.  Block b computes from ring slot RD, prefetches block
    b+1's first fragments from RDN and starts the copy of block b+3's image into slot WR (free
    since the barrier that ended b-1)."""
    out.append(f"; ---- block iteration, parity {label}")
    other = "B" if label == "A" else "A"
    p_cur, p_prev = P[label], P[other]
    S_P, N_P = SB[label]["p"], SB[other]["p"]
    gaps = {g: [] for g in range(NG)}
    V_RD, V_RDN = ADDR[label]
    N_RD, N_RDN = ADDR[other]

    def read_frag(g, slot_reg, comp, rh, sp):
        gaps[g].append(("lds", f"ds_read_b128 {vr(frag(comp, rh, sp), 4)}, {vr(slot_reg)} offset:{piece(comp, rh, sp)}",
                        f"f{comp}{rh}{sp}"))

    for comp, g0, slot_reg in ((1, 4, V_RD), (2, 16, V_RD), (0, 28, V_RDN)):
        for k, (rh, sp) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            g = g0 + 2 * k
            lu, fu = last_use(comp, rh, sp), first_use(comp, rh, sp)
            if comp == 0:
                assert g - lu >= 23 and NG + fu - g >= 8, (comp, rh, sp)
            else:
                assert NG + g - lu >= 23 and fu - g >= 8, (comp, rh, sp)
            read_frag(g, slot_reg, comp, rh, sp)
    # image of block b+3 -> slot WR: pointer (this parity's set) in gaps 0..1, the three pieces at
    # gaps 2, 10, 18
    for i, sx in enumerate(image_pointer(label)):
        gaps[i // 3].append(("salu", sx, None))
    for which in range(3):
        for tx in dma_ops(label, S_WR, which):
            gaps[2 + 8 * which].append(("dma" if tx.startswith("global") else "salu", tx, f"d{which}{label}"))
    # P of block b+1 into the other parity's registers (last read in gap 13)
    for k, tx in enumerate(p_loads(p_prev, S_P)):
        gaps[20].append(("vm", tx, "p" + other))
    gaps[21].append(("salu", f"s_add_u32 s{N_P}, s{S_P}, s{S_PSTRIDE}", None))
    gaps[21].append(("salu", f"s_addc_u32 s{N_P + 1}, s{S_P + 1}, 0", None))
    # rotation: component 2 of the previous block (gaps 2..13), 0 (14..25) and 1 (26..35) of this one
    for comp, p, g0, span in ((2, p_prev, 2, 12), (0, p_cur, 14, 12), (1, p_cur, 26, 10)):
        for k, op in enumerate(rotate_ops(comp, p)):
            gaps[g0 + (k * span) // 32].append(("rot" if comp == 2 else "rotp", op, None))
    # ring slot rotation (four slots) and the read addresses of the next iteration, once every
    # ring access of this iteration has been issued (gap 34)
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
        src_c = "0" if m < 4 else vr(dst, 4)
        if "mfma" not in ABLATE:
            out.append(f"v_mfma_f32_16x16x32_f16 {vr(dst, 4)}, {vr(frag(comp, rh, sp_a), 4)}, "
                       f"{bfrag(comp, th, sp_b)}, {src_c}")
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
                    cnt.need_vm("p" + label)      # loaded one block ago
                    waited_p = True
                if "rot" not in ABLATE:
                    out.append(text)
            else:
                out.append(text)
    # the image this wave started one iteration ago (block b+2's) must have landed before the
    # barrier publishes it: block b+1 prefetches from it (the wait for P has covered it already)
    cnt.need_vm("d2" + other)
    # every read of THIS block's slot has returned (the barrier frees it for the copy of block b+4); the
    # prefetch of block b+1's first fragments (gaps 28..34, from the next slot) stays in flight across it
    cnt.need_lgkm("f211")
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
    BF = [S_BF, 66, 68]
    for j in range(1, 3):
        o(f"s_add_u32 s{BF[j]}, s{S_BF}, {4096 * j}")
        o(f"s_addc_u32 s{BF[j] + 1}, s{S_BF + 1}, 0")
    # P of block 0 (parity A) through parity B's pointer; parity A's pointer is block 1's
    o(f"s_add_u32 s{SB['A']['p']}, s{SB['B']['p']}, s{S_PSTRIDE}")
    o(f"s_addc_u32 s{SB['A']['p'] + 1}, s{SB['B']['p'] + 1}, 0")
    o("s_nop 4")
    out.extend(p_loads(P["A"], SB["B"]["p"]))
    for f in range(4 * NC):
        b = BF[f // 4]
        if "bimg" not in ABLATE:
            o(f"global_load_dwordx4 {ar(4 * f)}, %[bo], s[{b}:{b + 1}] offset:{(f % 4) * 1024}")
    for base in (KB[2], ACC[0], ACC[1]):
        for i in range(16):
            o(f"v_mov_b32 {vr(base + i)}, 0")
    for i in range(8):
        o(f"v_mov_b32 {vr(P['B'] + i)}, 0")
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
    o("s_waitcnt vmcnt(0)")          # P of block 0, the phasor images and the three slot images
    o("s_barrier")
    for rh, sp in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o(f"ds_read_b128 {vr(frag(0, rh, sp), 4)}, {vr(V_RD)} offset:{piece(0, rh, sp)}")
    o("s_waitcnt lgkmcnt(0)")
    cnt.lgkm = []

    def trip(out_, cnt_):
        iteration(cnt_, out_, "A")
        out_.append(f"s_sub_u32 s{S_NLEFT}, s{S_NLEFT}, 1")
        out_.append(f"s_cmp_eq_u32 s{S_NLEFT}, 0")
        out_.append("s_cbranch_scc1 2f")
        iteration(cnt_, out_, "B")
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
    o(f"; ===== main loop, two blocks per trip; vm, lgkm at the top: {state}")
    o("1:")
    trip(out, cnt)
    assert (cnt.vm, cnt.lgkm) == state, (cnt.lgkm, cnt.vm, state)
    # component 2 of the last block is still to be rotated, with that block's P
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(rotate_ops(2, P["B"]))
    o("s_branch 3f")
    o("2:")
    o("s_waitcnt vmcnt(0)")
    o("s_nop 15")
    o("s_nop 15")
    out.extend(rotate_ops(2, P["A"]))
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
    print_header("GSDR_MFMA_RING16P3", __file__,
                 "Main loop of ddc_mfma_ring16p3_kernel (pre-converted operands by LDS-DMA, three real products per complex multiply, v_mfma_f32_16x16x32_f16)",
                 generate(), vb=VB, v_last=V_LAST, nagpr=NAGPR, sgprs=SGPR_CLOBBER, nbytes=NSLOT * SLOT, slot=SLOT)


if __name__ == "__main__":
    main()
