"""The frame of a pre-converted product loop of the matrix-core DDC (ring16p3, ring16p3r2, ring16p3f,
ring16p4f): a ring of four slot images filled by LDS-DMA three spans ahead, `units` operand units of
twelve v_mfma_f32_16x16x32_f16 per span, products turned into the accumulators by plain FMAs, two
spans (parity A, parity B: rule R2) per trip with an exit between them.  A library: it generates
nothing itself and imports nothing from a generator.  The scalar registers of the family are here;
a generator states its vector register map, its tables and where its rotation goes as a Loop."""
import os

from ddc_mfma_gen import Counters, ar, print_header, vr

# timing-only builds (WRONG results): GEN_ABLATE=rot,lds,gload,bar,bimg,mfma drops the rotation FMAs /
# the operand reads of the ring / the image copies / the barrier / the phasor-image loads of the
# prologue / the MFMAs
ABLATE = set(filter(None, os.environ.get("GEN_ABLATE", "").split(",")))
NSLOT = 4                  # ring slots: images arrive three spans ahead

# private SGPRs: scalar bases of the global loads, one set per parity (never rewrite what a queued
# memory instruction reads); C: prologue only
SB = {"A": dict(x=36, p=40), "B": dict(x=60, p=64), "C": dict(x=76, p=0)}
S_NLEFT, S_K, S_NHI1 = 42, 43, 44
S_RD, S_RDN, S_WR = 45, 46, 47
S_RD2 = 72     # slot of span s+2 (between RDN and WR)
S_M0 = 73      # M0 on entry
S_WRS = 74     # wave-uniform LDS base of this wave's image pieces
S_T0, S_T1 = 50, 51
S_XB = 52      # s[52:53] image base, span 0
S_BF = 56      # s[56:57] phasor-table images
S_PSTRIDE = 58
SGPR_CLOBBER = list(range(36, 80))


def dma_ops(par, slot_sreg, which):
    """LDS-DMA piece `which` of this wave of the image s[SB[par].x] into ring slot `slot_sreg`.
    M0 carries the wave-uniform LDS address; it is written right in front of its only reader and
    not again for eight MFMAs."""
    S_X = SB[par]["x"]
    return [
        f"s_add_u32 m0, s{slot_sreg}, s{S_WRS}" if which == 0 else "s_add_u32 m0, m0, 1024",
        "s_nop 0",
        f"global_load_lds_dwordx4 %[io{which}], s[{S_X}:{S_X + 1}]",
    ]


def p_loads(dst, sp_):
    """The float4 rows (Pr, Pi, -, -) of the two tone quarters of a 32-tone tile."""
    return [f"global_load_dwordx4 {vr(dst, 4)}, %[po], s[{sp_}:{sp_ + 1}]",
            f"global_load_dwordx4 {vr(dst + 4, 4)}, %[po], s[{sp_}:{sp_ + 1}] offset:256"]


class Loop:
    """What a variant states (keyword arguments):
      noun            what it calls 32 or 64 samples ("block", "span"), for the comments
      units           operand units per span; unit u at gaps 12u .. 12u+11, piece 4u + 2*sp + rh of a slot
      prod, image     per unit: the product it sums into (index of kb), the phasor image it multiplies by
      split           (sp_a, sp_b) of the three MFMAs of a tile, in issue order
      read_at         {(rh, sp): gap of the fragment's ds_read relative to the first gap of its unit}
      coef            per product (acc_r, acc_i): the element of a P row, "r" "i" "m" "p" = 0..3, "-" negates
      late            the product whose rotation falls into the span after its own
      g_pload         gap of the load of the next span's P
      rotation        (p_cur, p_prev) -> [(gap, "rot" | "rotp", v_fma_f32)]: rotp reads this span's P
      vb, acc, kb, f0, p, addr, v_last, nagpr, bf    the register map
      frag_units      the units whose fragments have registers of their own (all of them unless stated): unit u takes
                      those of unit u % frag_units, free 23 MFMAs after unit u - frag_units read them last
      rows, tq        the wave tile: row halves (of 16 rows) and tone quarters (of 16 tones) per wave, 2 x 2 unless
                      stated; 1 x 4 takes the pieces of one row half (chosen by the kernel through %[io..]) and the
                      phasor images and P of two 32-tone tiles (the second through %[bo1], %[po1])
    What follows from the wave tile: the pieces a wave copies per span (npiece), the ring slot (slot; an image in
    memory stays units * 4 KiB, image_bytes), piece, frag, mfma_of, b_image, rotate_ops, p_loads.
    late, g_pload, rotation and p belong to the loops that keep P by parity; one that handles P differently
    (ring16p3r2) overrides the methods of the last section instead."""

    def __init__(self, **desc):
        self.rows, self.tq, self.frag_units = 2, 2, None
        self.__dict__.update(desc)
        self.frag_units = self.frag_units or self.units
        assert self.units % self.frag_units == 0
        assert (self.rows, self.tq) in ((2, 2), (1, 4))
        self.image_bytes = self.units * 4 * 1024           # a slot image in memory: both row halves
        self.slot = self.units * 2 * self.rows * 1024      # bytes of one ring slot
        self.npiece = self.units * self.rows // 2          # 1-KiB pieces of a slot that each of the four waves copies
        self.ng = 12 * self.units              # MFMAs per span
        assert self.v_last + 1 + self.nagpr <= 256 and 16 * len(self.bf) * (self.tq // 2) == self.nagpr
        assert not (set(self.bf) | {b + 1 for b in self.bf}) - set(SGPR_CLOBBER)

    def piece(self, unit, rh, sp):
        """byte offset of operand piece (unit, rh, sp) inside a ring slot"""
        return 1024 * ((2 * unit + sp) * self.rows + rh)

    def frag(self, unit, rh, sp):
        return self.f0 + 4 * ((2 * (unit % self.frag_units) + sp) * self.rows + rh)

    # MFMA m of a unit: split m // 4, tile m % 4 = tq*rh + th
    def mfma_of(self, m):
        s, t = divmod(m, 4)
        return divmod(t, self.tq) + self.split[s]    # rh, th, sp_a, sp_b

    def b_image(self, image, th, sp):
        """AGPR (relative to acc_base) of phasor image `image`, tone quarter th, split sp: per 32-tone tile the
        images lie in the order of the table, (image, tone half, split)"""
        return ((((th >> 1) * (self.nagpr // 16 // (self.tq // 2)) + image) * 2 + (th & 1)) * 2 + sp) * 4

    def p_loads(self, dst, sp_):
        """Loads of the P of one span into v[dst : dst + 8]"""
        if self.tq == 2:
            return p_loads(dst, sp_)
        # (Pr, Pi) of four tone quarters: the first two floats of the float4 rows of two 32-tone tiles
        return [f"global_load_dwordx2 {vr(dst + 2 * q, 2)}, %[{'po1' if q >> 1 else 'po'}], s[{sp_}:{sp_ + 1}]" +
                (" offset:256" if q & 1 else "") for q in range(4)]

    def _uses(self, unit, rh, sp):
        return [12 * unit + m for m in range(12) if self.mfma_of(m)[0] == rh and self.mfma_of(m)[2] == sp]

    def first_use(self, unit, rh, sp):
        return min(self._uses(unit, rh, sp))

    def last_use(self, unit, rh, sp):
        return max(self._uses(unit, rh, sp))

    def image_pointer(self, par):
        """SALU: s[SB[par].x] = image base + slot * min(S_K, spans-1), then S_K += 1"""
        S_X = SB[par]["x"]
        return [
            f"s_min_u32 s{S_T0}, s{S_K}, s{S_NHI1}",
            f"s_mul_i32 s{S_T1}, s{S_T0}, {self.image_bytes}",
            f"s_add_u32 s{S_X}, s{S_XB}, s{S_T1}",
            f"s_addc_u32 s{S_X + 1}, s{S_XB + 1}, 0",
            f"s_add_u32 s{S_K}, s{S_K}, 1",
        ]

    def rotate_ops(self, prod, p):
        """The two FMAs per accumulator element that product `prod` feeds: 32 v_fma_f32 in two sweeps
        (an accumulator is read again 16 or more instructions after it was written)."""
        ops = []
        for part in range(2):                # 0: acc_r, 1: acc_i
            for i in range(16):
                th = (i >> 2) % self.tq      # register i belongs to tile (rh, th) = divmod(i >> 2, tq)
                c = self.coef[prod][part]
                assert "rimp".index(c[-1]) < 8 // self.tq
                coef = c[:-1] + vr(p + 8 // self.tq * th + "rimp".index(c[-1]))
                acc, k = vr(self.acc[part] + i), vr(self.kb[prod] + i)
                ops.append(f"v_fma_f32 {acc}, {coef}, {k}, {acc}")
        return ops

    # ---- P by parity: the next span's row is loaded into the other parity's registers ----
    s_p0 = SB["B"]["p"]        # takes %[pp]: span 0 (parity A) is loaded through parity B's pointer

    def acc_base(self, label):
        """first AGPR of the phasor images of a span of parity `label`"""
        return 0

    def from_zero(self, label):
        """whether a product's first unit starts it from 0 in a span of parity `label`"""
        return True

    def p_prologue(self):
        """-> (lines that load P of span 0, lines behind the wait for it, product bases and the P
        registers to clear: the first span rotates the late product "of the span before")"""
        A, B = SB["A"]["p"], SB["B"]["p"]
        return ([f"s_add_u32 s{A}, s{B}, s{S_PSTRIDE}", f"s_addc_u32 s{A + 1}, s{B + 1}, 0", "s_nop 4"] +
                self.p_loads(self.p["A"], B), [], [self.kb[self.late]], self.p["B"])

    def p_schedule(self, label):
        """[(gap, kind, text, tag)] of P and the rotation in a span of parity `label`"""
        other = "B" if label == "A" else "A"
        S_P, N_P = SB[label]["p"], SB[other]["p"]
        return [(self.g_pload, "vm", tx, "p" + other) for tx in self.p_loads(self.p[other], S_P)] + \
               [(self.g_pload + 1, "salu", f"s_add_u32 s{N_P}, s{S_P}, s{S_PSTRIDE}", None),
                (self.g_pload + 1, "salu", f"s_addc_u32 s{N_P + 1}, s{S_P + 1}, 0", None)] + \
               [(g, "rot", op, "p" + label if kind == "rotp" else None)      # loaded one span ago
                for g, kind, op in self.rotation(self.p[label], self.p[other])]

    def tail(self, label):
        """what is still to be rotated when the loop leaves behind a span of parity `label`"""
        return self.rotate_ops(self.late, self.p[label])


def span(v, cnt, out, label):
    """One span: v.ng MFMAs.  Span s computes from ring slot RD, prefetches span s+1's first
    fragments from RDN and starts the copy of span s+3's image into slot WR (free since the
    barrier that ended s-1)."""
    NG = v.ng
    out.append(f"; ---- {v.noun}, parity {label}")
    other = "B" if label == "A" else "A"
    gaps = {g: [] for g in range(NG)}
    V_RD, V_RDN = v.addr[label]
    N_RD, N_RDN = v.addr[other]

    # an operand fragment is read again 23 or more MFMAs after its last use (R1) and 8 or more ahead
    # of its first: units 1.. of this span, then unit 0 of the next one from the next slot
    last_rd = None
    for unit in list(range(1, v.units)) + [0]:
        for (rh, sp), rel in v.read_at.items():
            g = (12 * unit if unit else NG) + rel
            # the registers were last read by unit - frag_units, of this span or of the one before
            lu, fu = v.last_use((unit - v.frag_units) % v.units, rh, sp), v.first_use(unit, rh, sp)
            lu -= NG if lu >= g else 0
            if unit == 0:
                assert g - lu >= 23 and NG + fu - g >= 8, (unit, rh, sp)
            else:
                assert g - lu >= 23 and fu - g >= 8, (unit, rh, sp)
                last_rd = f"f{unit}{rh}{sp}"
            gaps[g].append(("lds", f"ds_read_b128 {vr(v.frag(unit, rh, sp), 4)}, {vr(V_RD if unit else V_RDN)} "
                            f"offset:{v.piece(unit, rh, sp)}", f"f{unit}{rh}{sp}"))
    # image of span s+3 -> slot WR: pointer (this parity's set) in gaps 0..1, this wave's pieces at
    # gaps 2, 10, 18, ..
    for i, sx in enumerate(v.image_pointer(label)):
        gaps[i // 3].append(("salu", sx, None))
    for which in range(v.npiece):
        for tx in dma_ops(label, S_WR, which):
            gaps[2 + 8 * which].append(("dma" if tx.startswith("global") else "salu", tx, f"d{which}{label}"))
    for g, kind, text, tag in v.p_schedule(label):
        gaps[g].append((kind, text, tag))
    # ring slot rotation (four slots) and the read addresses of the next span, once every ring
    # access of this one has been issued (gap NG - 2)
    gaps[NG - 2].append(("salu", f"s_mov_b32 s{S_T0}, s{S_RD}", None))
    gaps[NG - 2].append(("salu", f"s_mov_b32 s{S_RD}, s{S_RDN}", None))
    gaps[NG - 2].append(("salu", f"s_mov_b32 s{S_RDN}, s{S_RD2}", None))
    gaps[NG - 1].append(("salu", f"s_mov_b32 s{S_RD2}, s{S_WR}", None))
    gaps[NG - 1].append(("salu", f"s_mov_b32 s{S_WR}, s{S_T0}", None))
    gaps[NG - 1].append(("addr", f"v_add_u32 {vr(N_RD)}, s{S_RD}, %[lane16]", None))
    gaps[NG - 1].append(("addr", f"v_add_u32 {vr(N_RDN)}, s{S_RDN}, %[lane16]", None))

    waited_p = False
    for g in range(NG):
        unit, m = divmod(g, 12)
        rh, th, sp_a, sp_b = v.mfma_of(m)
        if v.first_use(unit, rh, sp_a) == g:
            cnt.need_lgkm(f"f{unit}{rh}{sp_a}")
        dst = v.kb[v.prod[unit]] + 4 * (v.tq * rh + th)
        first = v.prod.index(v.prod[unit]) == unit and m < 4 and v.from_zero(label)
        if "mfma" not in ABLATE:
            out.append(f"v_mfma_f32_16x16x32_f16 {vr(dst, 4)}, {vr(v.frag(unit, rh, sp_a), 4)}, "
                       f"{ar(v.acc_base(label) + v.b_image(v.image[unit], th, sp_b))}, {'0' if first else vr(dst, 4)}")
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
            elif kind in ("rot", "pmove"):      # tag: the load of the P they read, waited for once
                if tag and not waited_p:
                    cnt.need_vm(tag)
                    waited_p = True
                if kind == "pmove" or "rot" not in ABLATE:
                    out.append(text)
            else:
                out.append(text)
    # the image this wave started one span ago (span s+2's) must have landed before the barrier
    # publishes it: span s+1 prefetches from it
    cnt.need_vm(f"d{v.npiece - 1}{other}")
    # every read of THIS span's slot has returned (the barrier frees it for the copy of span s+4); the
    # prefetch of span s+1's first fragments (from the next slot) stays in flight across it
    cnt.need_lgkm(last_rd)
    if "bar" not in ABLATE:
        out.append("s_barrier")


def generate(v):
    out = []
    cnt = Counters(out)
    o = out.append
    p_load, p_landed, zero_k, zero_p = v.p_prologue()
    o("; ===== prologue =====")
    o(f"s_mov_b32 s{S_M0}, m0")
    o(f"s_mov_b32 s{S_XB}, %[ib_lo]")          # image base of this row tile, span 0
    o(f"s_mov_b32 s{S_XB + 1}, %[ib_hi]")
    o(f"s_mov_b32 s{S_WRS}, %[wrs]")
    o(f"s_mov_b32 s{v.s_p0}, %[pp_lo]")
    o(f"s_mov_b32 s{v.s_p0 + 1}, %[pp_hi]")
    o(f"s_mov_b32 s{S_BF}, %[bf_lo]")
    o(f"s_mov_b32 s{S_BF + 1}, %[bf_hi]")
    o(f"s_mov_b32 s{S_PSTRIDE}, %[pstride]")
    o(f"s_mov_b32 s{S_NLEFT}, %[nhi]")
    o(f"s_add_u32 s{S_NHI1}, %[nhi], -1")
    o(f"s_mov_b32 s{S_K}, 0")
    o(f"s_mov_b32 s{S_RD}, 0")
    o(f"s_mov_b32 s{S_RDN}, {v.slot}")
    o(f"s_mov_b32 s{S_RD2}, {2 * v.slot}")
    o(f"s_mov_b32 s{S_WR}, {3 * v.slot}")
    o("s_nop 4")
    # scalar bases of the phasor images, 4 KiB (four images) apart
    for j in range(1, len(v.bf)):
        o(f"s_add_u32 s{v.bf[j]}, s{S_BF}, {4096 * j}")
        o(f"s_addc_u32 s{v.bf[j] + 1}, s{S_BF + 1}, 0")
    out.extend(p_load)
    per_tile = 4 * len(v.bf)                # 1-KiB images of a 32-tone tile
    for f in range(v.nagpr // 4):
        b = v.bf[f % per_tile // 4]
        if "bimg" not in ABLATE:
            o(f"global_load_dwordx4 {ar(4 * f)}, %[{'bo1' if f // per_tile else 'bo'}], s[{b}:{b + 1}] offset:{(f % 4) * 1024}")
    for base in zero_k + list(v.acc):
        for i in range(16):
            o(f"v_mov_b32 {vr(base + i)}, 0")
    for i in range(8):
        o(f"v_mov_b32 {vr(zero_p + i)}, 0")
    # images of spans 0, 1, 2 into slots 0, 1, 2 (pointer sets A, B, C: one per image)
    for par, slot in (("A", S_RD), ("B", S_RDN), ("C", S_RD2)):
        out.extend(v.image_pointer(par))
        for which in range(v.npiece):
            o("s_nop 4")
            out.extend(dma_ops(par, slot, which))
        o("s_nop 4")
    V_RD, V_RDN = v.addr["A"]
    o(f"v_add_u32 {vr(V_RD)}, s{S_RD}, %[lane16]")
    o(f"v_add_u32 {vr(V_RDN)}, s{S_RDN}, %[lane16]")
    o("s_waitcnt vmcnt(0)")          # P of span 0, the phasor images and the three slot images
    out.extend(p_landed)
    o("s_barrier")
    for rh, sp in ((rh, sp) for sp in range(2) for rh in range(v.rows)):
        o(f"ds_read_b128 {vr(v.frag(0, rh, sp), 4)}, {vr(V_RD)} offset:{v.piece(0, rh, sp)}")
    o("s_waitcnt lgkmcnt(0)")
    cnt.lgkm = []

    def trip(out_, cnt_):
        span(v, cnt_, out_, "A")
        out_.append(f"s_sub_u32 s{S_NLEFT}, s{S_NLEFT}, 1")
        out_.append(f"s_cmp_eq_u32 s{S_NLEFT}, 0")
        out_.append("s_cbranch_scc1 2f")
        span(v, cnt_, out_, "B")
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
    o(f"; ===== main loop, two {v.noun}s per trip; vm, lgkm at the top: {state}")
    o("1:")
    trip(out, cnt)
    assert (cnt.vm, cnt.lgkm) == state, (cnt.lgkm, cnt.vm, state)
    # left after a span of parity B (label 2: of parity A): what the next span would have rotated
    for label, then in (("B", ["s_branch 3f", "2:"]), ("A", ["3:"])):
        o("s_waitcnt vmcnt(0)")
        o("s_nop 15")
        o("s_nop 15")
        out.extend(v.tail(label) + then)
    # every image copy has landed (vmcnt(0) above) and every wave is past the last barrier: the
    # ring is idle, the accumulators go to the C++ epilogue through it
    o("s_barrier")
    for q in range(8):
        base = (v.acc[0] if q < 4 else v.acc[1]) + 4 * (q & 3)
        o(f"ds_write_b128 %[accaddr], {vr(base, 4)} offset:{q * 1024}")
    o("s_waitcnt lgkmcnt(0)")
    o(f"s_mov_b32 m0, s{S_M0}")
    return out


def print_loop(v, pfx, gen_file, what):
    print_header(pfx, gen_file, what, generate(v), vb=v.vb, v_last=v.v_last, nagpr=v.nagpr, sgprs=SGPR_CLOBBER,
                 nbytes=NSLOT * v.slot, slot=v.slot)
