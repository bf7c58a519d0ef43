"""Host-side checks of the direct folded loop over 128-sample spans (tools/gen_ddc_mfma_ring16p4fw2.py,
csrc/ddc_mfma_ring16p4fw2_gen.h, ddc_mfma_ring16p4fw2_kernel, mfma_build_tables4f2): no GPU
needed."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu_sdr_amd", "csrc")
HEADER = os.path.join(CSRC, "ddc_mfma_ring16p4fw2_gen.h")
KERNEL = "ddc_mfma_ring16p4fw2_kernel"
OLDER = ["ring16p3", "ring16p3r2", "ring16p3f", "ring16p4f", "ring16p4fw"]
MFMA = re.compile(r"v_mfma_f32_16x16x32_f16 v\[(\d+):\d+\], v\[(\d+):\d+\], a\[(\d+):\d+\], (\S+)")
NG = 96


def _lines():
    return re.findall(r'"(.*?)\\n\\t"', open(HEADER).read())


def _spans():
    """The two spans (parity A, parity B) of one trip of the loop."""
    lines = _lines()
    top, mid, back = lines.index("1:"), lines.index("s_cbranch_scc1 2f"), lines.index("s_cbranch_scc1 1b")
    return lines[top:mid], lines[mid:back]


def _generate(name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GEN_")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", f"gen_ddc_mfma_{name}.py")], capture_output=True,
                          text=True, check=True, env=env).stdout


def test_header_is_what_the_generator_emits():
    assert _generate("ring16p4fw2") == open(HEADER).read()


@pytest.mark.parametrize("name", OLDER)
def test_older_generators_still_emit_their_headers(name):
    """The frame (tools/ddc_mfma_pframe.py) learnt to share fragment registers between units: nothing changes for the
    loops that do not."""
    assert _generate(name) == open(os.path.join(CSRC, f"ddc_mfma_{name}_gen.h")).read()


def test_loop_obeys_the_hazard_rules():
    spec = importlib.util.spec_from_file_location("check_asm_rules", os.path.join(ROOT, "tools", "check_asm_rules.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert chk.check(HEADER) == []


def test_span_has_96_mfmas_64_fmas_four_copies_four_p_loads_and_sixteen_reads():
    for body in _spans():
        assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in body) == NG
        assert sum(ln.startswith("v_fma_f32") for ln in body) == 64
        assert sum(ln.startswith("global_load_lds_dwordx4") for ln in body) == 4
        assert sum(ln.startswith("global_load_dwordx2") for ln in body) == 4
        assert sum(ln.startswith("ds_read_b128") for ln in body) == 16
        assert sum(ln == "s_barrier" for ln in body) == 1
    assert not any(ln.startswith("v_pk_") for ln in _lines())


def test_units_take_their_images_in_the_order_of_the_fold():
    """Unit u = 2*V + K-half at MFMAs 12u .. 12u+11: Re from units 0..3, Im from 4..7, started from 0 in the first four
    MFMAs of units 0 and 4 only; image 2*K-half + (c, d, d, c)[V] of the tone quarter's 32-tone tile; splits lo*hi,
    hi*lo, hi*hi; fragment registers of unit u % 4."""
    for body in _spans():
        mfmas = [MFMA.fullmatch(ln) for ln in body if ln.startswith("v_mfma")]
        assert all(mfmas) and len(mfmas) == NG
        frag0 = min(int(m.group(2)) for m in mfmas)
        ks = sorted({int(m.group(1)) for m in mfmas})
        assert ks == list(range(ks[0], ks[0] + 32, 4))
        seen = set()
        for i, m in enumerate(mfmas):
            d, a, b, c = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            u, k = divmod(i, 12)
            assert not any(kk <= a < kk + 4 for kk in ks), "product registers are C/D only"
            assert (d - ks[0]) // 16 == u // 4                   # Re, Im
            q = (d - ks[0]) // 4 % 4                             # tile q of a product holds tone quarter q
            assert q == k % 4
            blk = b // 4                                         # ((tile32*4 + image)*2 + th)*2 + sp
            assert b + 3 < 128 and blk >> 4 == q >> 1 and (blk >> 1) & 1 == q & 1
            assert (blk >> 2) & 3 == 2 * (u & 1) + (0, 1, 1, 0)[u >> 1], (i, b)
            rel = (a - frag0) // 4                               # fragment 2*(u % 4) + sp
            assert rel // 2 == u % 4
            assert (rel % 2, blk & 1) == ((1, 0), (0, 1), (0, 0))[k // 4]
            if d in seen:
                assert c.startswith(f"v[{d}:")
            else:
                assert c == "0" and u in (0, 4) and k < 4
                seen.add(d)
        assert len(seen) == 8


def _stream():
    a, b = _spans()
    return [ln for ln in a + b if not ln.endswith(":")]


def test_fragments_are_read_8_gaps_ahead_and_rewritten_23_mfmas_behind():
    """Over three trips: a ds_read_b128 into a fragment register lies 23 or more MFMAs behind the last MFMA that read
    the register (rule R1) and 8 or more ahead of the next one that does."""
    stream = _stream() * 3
    uses, n = {}, 0
    for ln in stream:
        m = MFMA.fullmatch(ln)
        if m:
            for r in range(int(m.group(2)), int(m.group(2)) + 4):
                uses.setdefault(r, []).append(n)
            n += 1
    n = checked = 0
    for ln in stream:
        if ln.startswith("v_mfma"):
            n += 1
        elif ln.startswith("ds_read_b128") and 2 * NG <= n < 4 * NG:
            r = int(re.match(r"ds_read_b128 v\[(\d+):", ln).group(1))
            before = max(u for u in uses[r] if u < n)
            after = min(u for u in uses[r] if u >= n)
            assert n - 1 - before >= 23 and after - (n - 1) >= 8, (ln, n, before, after)
            checked += 1
    assert checked == 32


def test_products_are_read_three_mfmas_after_their_last_one_and_before_their_next():
    """A rotation FMA reads a product tile no sooner than three MFMAs behind the last MFMA that summed into it, and with
    two or more MFMAs to go before the one that starts the tile anew (walked over three trips)."""
    stream = _stream() * 3
    writes, n = {}, 0
    for ln in stream:
        if ln.startswith("v_mfma"):
            d = int(re.match(r"v_mfma\S+ v\[(\d+):", ln).group(1))
            for r in range(d, d + 4):
                writes.setdefault(r, []).append(n)
            n += 1
    n = checked = 0
    for ln in stream:
        if ln.startswith("v_mfma"):
            n += 1
        elif ln.startswith("v_fma_f32") and 2 * NG <= n < 4 * NG:       # the middle trip
            k = int(ln.split(",")[2].strip().lstrip("v"))
            before = max(w for w in writes[k] if w < n)
            after = min(w for w in writes[k] if w >= n)
            assert n - 1 - before >= 3 and after - n >= 1, (ln, n, before, after)
            checked += 1
    assert checked == 128


def test_accumulators_are_reread_no_sooner_than_16_instructions_later():
    body, last = _stream(), {}
    for i, ln in enumerate(body + body):
        if ln.startswith("v_fma_f32"):
            acc = ln.split()[1].rstrip(",")
            assert i - last.get(acc, -100) >= 16, ln
            last[acc] = i


def test_p_is_loaded_after_its_registers_were_last_read():
    """The four P loads of a span write the other parity's registers: behind the last FMA that reads them (the Im of
    the span before) and ahead of the first of the next span."""
    for body in _spans():
        loads = [i for i, ln in enumerate(body) if ln.startswith("global_load_dwordx2")]
        regs = set()
        for i in loads:
            lo, hi = map(int, re.match(r"global_load_dwordx2 v\[(\d+):(\d+)\]", body[i]).groups())
            regs |= set(range(lo, hi + 1))
        assert len(regs) == 8
        readers = [i for i, ln in enumerate(body) if ln.startswith("v_fma_f32")
                   and int(ln.split(",")[1].strip().lstrip("-v")) in regs]
        assert len(readers) == 32 and max(readers) < min(loads)


def test_m0_is_rewritten_eight_mfmas_behind_its_reader():
    n, read_at = 0, None
    for ln in _stream() * 2:
        if ln.startswith("v_mfma"):
            n += 1
        elif ln.startswith("global_load_lds"):
            read_at = n
        elif re.match(r"s_\w+ m0,", ln) and read_at is not None:
            assert n - read_at >= 8, (ln, n, read_at)


def test_both_exits_rotate_the_last_im():
    lines = _lines()
    back, odd, end = lines.index("s_cbranch_scc1 1b"), lines.index("2:"), lines.index("3:")
    for tail in (lines[back:odd], lines[odd:end]):
        fmas = [ln for ln in tail if ln.startswith("v_fma_f32")]
        assert len(fmas) == 32 and len(set(fmas)) == 32


def test_kernel_takes_128_and_128_registers_and_64_kib(gsdr_lib, tmp_path):
    """From the code object of the library as built: the kernel once, 128 VGPRs + 128 AGPRs (two waves per SIMD), no
    spills, no scratch, 64 KiB of LDS (two workgroups per compute unit out of 160 KiB)."""
    from gpu_sdr_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm llvm tools")
    so = tmp_path / "libgsdr.so"
    shutil.copy(_lib.LIB_PATH, so)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    found = 0
    for f in tmp_path.iterdir():
        if "amdgcn" not in f.name:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or KERNEL not in name.group(1):
                continue
            found += 1
            agprs = int(blk.split()[0])
            regs = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))        # VGPRs + AGPRs on gfx90a and later
            lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
            print(f"{KERNEL}: {regs} VGPRs + AGPRs ({agprs} AGPRs), {lds} bytes of LDS")
            assert (regs, agprs, lds) == (256, 128, 64 * 1024)
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0
    assert found == 1


@pytest.mark.parametrize("fm", [0, 1, 2, 37, 4096, 99999, 100000, 100001, 199999])
def test_folded_sums_over_64_pairs_equal_the_complex_sum(fm):
    """Re = V1 x c + V2 x d and Im = V3 x d + V4 x c over the 64 partner pairs of a 128-sample span, the phase taken
    from the centre of the span in half samples, turned by the span phasor, give sum (a + i*b) * w^t over the whole
    window.  Three spans, the last holding one block (its other samples and partners zero), in double."""
    rate, nspan, nblk = 200000, 3, 9
    rng = np.random.default_rng(fm)
    a, b = rng.standard_normal(128 * nspan), rng.standard_normal(128 * nspan)
    a[32 * nblk:] = 0
    b[32 * nblk:] = 0
    t = np.arange(128 * nspan)
    w = np.exp(-2j * np.pi * ((fm * t) % rate) / rate)              # host_phasor's sign
    want = np.sum((a + 1j * b) * w)
    j = np.arange(64)
    ph2 = (fm * (127 - 2 * j)) % (2 * rate)                          # half samples, exact integers
    c, d = np.cos(np.pi * ph2 / rate), np.sin(np.pi * ph2 / rate)    # w^(j - 63.5) = conj(w^(63.5 - j))
    acc = 0j
    for s in range(nspan):
        aj, bj = a[128 * s:128 * s + 64], b[128 * s:128 * s + 64]
        ap, bp = a[128 * s + 127 - j], b[128 * s + 127 - j]
        re_ = np.sum((aj + ap) * c) + np.sum((bp - bj) * d)
        im_ = np.sum((aj - ap) * d) + np.sum((bj + bp) * c)
        ps2 = (fm * ((256 * s + 127) % (2 * rate))) % (2 * rate)
        pr, pi = np.cos(np.pi * ps2 / rate), -np.sin(np.pi * ps2 / rate)
        acc += (pr * re_ - pi * im_) + 1j * (pi * re_ + pr * im_)
    assert abs(acc - want) <= 1e-11


def test_table_builder_against_the_double_precision_formula(gsdr_lib):
    """mfma_build_tables4f2 for two 32-tone tiles at 200 Msps that hold tones 0, +-1, +-(rate/2 - 1) and a few others:
    every c and d is the double-precision value rounded once to fp32 and split hi = fp16(v), lo = fp16(v - hi); image
    2*K-half + (c, d), tone half, split; lane l = tone 16*th + (l & 15), element jj <-> j = 32*K-half + 8*(l >> 4) + jj;
    P rows (Pr, Pi, Pi-Pr, Pr+Pi) of w^(128*span + 63.5) and a zero row behind the last span."""
    from gpu_sdr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rate, nblk, tiles = 200_000_000, 9, 2
    tones = [0, 1, -1, rate // 2 - 1, -(rate // 2 - 1), 12345, -7654321, 50_000_000]
    rng = np.random.default_rng(5)
    fm = np.mod(np.concatenate([tones, rng.integers(-rate // 2 + 1, rate // 2, size=32 * tiles - len(tones))]), rate).astype(np.uint32)
    nspan = (nblk + 3) // 4
    images = np.zeros((tiles, 16, 64, 8), dtype=np.float16)
    p = np.zeros((nspan + 1, 32 * tiles, 4), dtype=np.float32)
    fn = lib.gsdr_mfma_tables4f2_host_
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(rate, fm.ctypes.data, tiles, nblk, images.ctypes.data, p.ctypes.data) == nspan + 1
    f = fm.astype(np.int64)
    for T in range(tiles):
        for kh in range(2):
            for cd in range(2):
                for th in range(2):
                    lane = np.arange(64)
                    tone = f[32 * T + 16 * th + (lane & 15)]
                    j = 32 * kh + 8 * (lane >> 4)[:, None] + np.arange(8)[None, :]
                    ph2 = (tone[:, None] * (127 - 2 * j)) % (2 * rate)
                    ang = np.pi * (ph2.astype(np.float64) / rate)
                    v = (np.sin(ang) if cd else np.cos(ang)).astype(np.float32)
                    hi = v.astype(np.float16)
                    lo = (v - hi.astype(np.float32)).astype(np.float16)
                    img = 2 * kh + cd
                    np.testing.assert_array_equal(images[T, (img * 2 + th) * 2 + 0].view(np.uint16), hi.view(np.uint16))
                    np.testing.assert_array_equal(images[T, (img * 2 + th) * 2 + 1].view(np.uint16), lo.view(np.uint16))
    for s in range(nspan):
        ph2 = (f * ((256 * s + 127) % (2 * rate))) % (2 * rate)
        ang = np.pi * (ph2.astype(np.float64) / rate)
        re, im = np.cos(ang), -np.sin(ang)
        want = np.stack([re, im, im - re, re + im], axis=1).astype(np.float32)
        np.testing.assert_array_equal(p[s].view(np.uint32), want.view(np.uint32))
    assert not p[nspan].any()
    # tone 0: c = 1, d = 0 exactly; P = 1
    assert (images[0, 0, ::16].astype(np.float32) == 1).all() and (p[:nspan, 0, 0] == 1).all() and (p[:nspan, 0, 1] == 0).all()
