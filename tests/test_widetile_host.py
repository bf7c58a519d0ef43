"""Host-side checks of the direct folded loop on wave tiles of 16 rows x 64 tones (tools/gen_ddc_mfma_ring16p4fw.py,
csrc/ddc_mfma_ring16p4fw_gen.h, ddc_mfma_ring16p4fw_kernel): no GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu_sdr_amd", "csrc")
HEADER = os.path.join(CSRC, "ddc_mfma_ring16p4fw_gen.h")
NARROW = os.path.join(CSRC, "ddc_mfma_ring16p4f_gen.h")
KERNEL = "ddc_mfma_ring16p4fw_kernel"
MFMA = re.compile(r"v_mfma_f32_16x16x32_f16 v\[(\d+):\d+\], v\[(\d+):\d+\], a\[(\d+):\d+\], (\S+)")


def _lines(path=HEADER):
    return re.findall(r'"(.*?)\\n\\t"', open(path).read())


def _spans(path=HEADER):
    """The two spans (parity A, parity B) of one trip of the loop."""
    lines = _lines(path)
    top = lines.index("1:")
    mid = lines.index("s_cbranch_scc1 2f")
    back = lines.index("s_cbranch_scc1 1b")
    return lines[top:mid], lines[mid:back]


def test_header_is_what_the_generator_emits():
    env = {k: v for k, v in os.environ.items() if not k.startswith("GEN_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ddc_mfma_ring16p4fw.py")], capture_output=True,
                         text=True, check=True, env=env).stdout
    assert out == open(HEADER).read()


def test_loop_obeys_the_hazard_rules():
    spec = importlib.util.spec_from_file_location("check_asm_rules", os.path.join(ROOT, "tools", "check_asm_rules.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert chk.check(HEADER) == []


def test_span_has_48_mfmas_64_fmas_two_copies_and_eight_reads():
    for body in _spans():
        assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in body) == 48
        assert sum(ln.startswith("v_fma_f32") for ln in body) == 64
        assert sum(ln.startswith("global_load_lds_dwordx4") for ln in body) == 2
        assert sum(ln.startswith("ds_read_b128") for ln in body) == 8
        assert sum(ln == "s_barrier" for ln in body) == 1
    assert not any(ln.startswith("v_pk_") for ln in _lines())


def _tile_sequences(path, wide):
    """Per span: {tile position: [(unit, (fragment split, image split), image)]} in issue order.  A tile position is the
    product register block counted from the first block of its product (Re, Im); unit = MFMA ordinal // 12; the
    fragment split from the operand register, the image and its split from the AGPR block."""
    res = []
    for body in _spans(path):
        mfmas = [MFMA.fullmatch(ln) for ln in body if ln.startswith("v_mfma")]
        assert all(mfmas)
        frag0 = min(int(m.group(2)) for m in mfmas)
        dsts = sorted({int(m.group(1)) for m in mfmas})
        assert len(dsts) == 8 and dsts == list(range(dsts[0], dsts[0] + 32, 4))
        seqs = {}
        for i, m in enumerate(mfmas):
            d, a, b = int(m.group(1)), int(m.group(2)), int(m.group(3)) // 4
            unit = i // 12
            rel = (a - frag0) // 4
            if wide:        # fragment (2*unit + sp); AGPR block ((tile32*2 + image)*2 + th)*2 + sp
                assert rel // 2 == unit
                sp_a, image, sp_b = rel % 2, (b >> 2) & 1, b & 1
            else:           # fragment 4*unit + 2*sp + rh; AGPR block (image*2 + th)*2 + sp
                assert rel // 4 == unit
                sp_a, image, sp_b = (rel >> 1) & 1, b >> 2, b & 1
            seqs.setdefault((d - dsts[0]) // 4, []).append((unit, (sp_a, sp_b), image))
        res.append(seqs)
    return res


def test_every_tile_sums_its_products_in_the_order_of_the_32x32_loop():
    """For every product tile the sequence of (unit, split, image) of its MFMAs is that of the same tile position in
    ddc_mfma_ring16p4f_gen.h: an output element receives its products in the same order."""
    wide, narrow = _tile_sequences(HEADER, True), _tile_sequences(NARROW, False)
    for w, n in zip(wide, narrow):
        assert sorted(w) == sorted(n) == list(range(8))
        for t in range(8):
            assert len(w[t]) == 6 and w[t] == n[t], (t, w[t], n[t])


def test_tiles_start_from_zero_in_units_0_and_2_only_and_take_the_images_of_their_tones():
    for body in _spans():
        mfmas = [MFMA.fullmatch(ln) for ln in body if ln.startswith("v_mfma")]
        ks = sorted({int(m.group(1)) for m in mfmas})
        seen = set()
        for i, m in enumerate(mfmas):
            d, a, b, c = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            assert not any(k <= a < k + 4 for k in ks), "product registers are C/D only"
            assert b + 3 < 64
            # tile q of a product holds tone quarter q: 32-tone tile q >> 1, tone half q & 1
            q = (d - ks[0]) // 4 % 4
            assert b // 4 // 8 == q >> 1 and (b // 4 >> 1) & 1 == q & 1, (i, d, b)
            if d in seen:
                assert c.startswith(f"v[{d}:")
            else:
                assert c == "0" and i // 12 in (0, 2) and i % 12 < 4
                seen.add(d)
        assert len(seen) == 8


def test_fragments_are_read_8_gaps_ahead_and_rewritten_23_mfmas_behind():
    """Over three trips: a ds_read_b128 into a fragment register lies 23 or more MFMAs behind the last MFMA that read
    the register and 8 or more ahead of the next one that does."""
    a, b = _spans()
    body = [ln for ln in a + b if not ln.endswith(":")]
    stream = body * 3
    uses = {}
    n = 0
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
        elif ln.startswith("ds_read_b128") and 96 <= n < 192:
            r = int(re.match(r"ds_read_b128 v\[(\d+):", ln).group(1))
            before = max(u for u in uses[r] if u < n)
            after = min(u for u in uses[r] if u >= n)
            assert n - 1 - before >= 23 and after - (n - 1) >= 8, (ln, n, before, after)
            checked += 1
    assert checked == 16


def test_m0_is_rewritten_eight_mfmas_behind_its_reader():
    a, b = _spans()
    body = [ln for ln in a + b if not ln.endswith(":")]
    n, read_at = 0, None
    for ln in body * 2:
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


def test_kernel_keeps_two_workgroups_per_compute_unit(gsdr_lib, tmp_path):
    """From the code object of the library as built: the kernel once, at most 256 VGPRs + AGPRs, no spills, no
    scratch, 32 KiB of LDS or more (the accumulators of four waves) and two workgroups to a compute unit (registers
    of two waves per SIMD out of 512, LDS of two workgroups out of 160 KiB).  The figures are printed."""
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
            regs = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))        # VGPRs + AGPRs on gfx90a and later
            lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
            print(f"{KERNEL}: {regs} VGPRs + AGPRs, {lds} bytes of LDS")
            assert regs <= 256
            assert 2 * regs <= 512
            assert 32 * 1024 <= lds <= 80 * 1024
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0
    assert found == 1
