"""Host-side checks of the pair-rotating three-product matrix-core loop (tools/gen_ddc_mfma_ring16p3r2.py,
csrc/ddc_mfma_ring16p3r2_gen.h, ddc_mfma_ring16p3r2_kernel): no GPU needed."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gpu_sdr_amd", "csrc", "ddc_mfma_ring16p3r2_gen.h")
KERNEL = "ddc_mfma_ring16p3r2_kernel"


def _lines():
    return re.findall(r'"(.*?)\\n\\t"', open(HEADER).read())


def test_generated_header_is_current():
    env = {k: v for k, v in os.environ.items() if not k.startswith("GEN_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ddc_mfma_ring16p3r2.py")], capture_output=True,
                         text=True, check=True, env=env).stdout
    assert out == open(HEADER).read()


def test_loop_obeys_the_hazard_rules():
    spec = importlib.util.spec_from_file_location("check_asm_rules", os.path.join(ROOT, "tools", "check_asm_rules.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert chk.check(HEADER) == []


def test_trip_has_72_mfmas_and_96_rotation_fmas():
    lines = _lines()
    top = lines.index("1:")
    back = next(i for i, ln in enumerate(lines) if ln == "s_cbranch_scc1 1b")
    body = lines[top:back]                    # one pair of blocks per trip
    assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in body) == 72
    assert sum(ln.startswith("v_fma_f32") for ln in body) == 96
    assert sum(ln.startswith("global_load_lds_dwordx4") for ln in body) == 6
    assert not any(ln.startswith("v_pk_") for ln in lines)


def test_second_block_accumulates_onto_the_first():
    """The first block of a pair multiplies by the images of samples 0..31 (a0..a47) and starts every product tile
    from 0; the second by those of samples 32..63 (a48..a95) and always accumulates.  K registers are C/D only."""
    lines = _lines()
    top = lines.index("1:")
    back = next(i for i, ln in enumerate(lines) if ln == "s_cbranch_scc1 1b")
    mfmas = [re.fullmatch(r"v_mfma_f32_16x16x32_f16 v\[(\d+):\d+\], v\[(\d+):\d+\], a\[(\d+):\d+\], (\S+)", ln)
             for ln in lines[top:back] if ln.startswith("v_mfma")]
    assert all(mfmas)
    ks = {int(m.group(1)) for m in mfmas}
    for i, m in enumerate(mfmas):
        d, a, b, c = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
        assert (b < 48) == (i < 36)
        assert not any(k <= a < k + 4 for k in ks)
        if c == "0":
            assert i < 36 and i % 12 < 4
        else:
            assert c.startswith(f"v[{d}:") and not (i < 36 and i % 12 < 4)


def test_accumulators_are_reread_no_sooner_than_16_instructions_later():
    lines = _lines()
    top = lines.index("1:")
    back = next(i for i, ln in enumerate(lines) if ln == "s_cbranch_scc1 1b")
    body = [ln for ln in lines[top:back] if not ln.endswith(":")]
    last = {}
    for i, ln in enumerate(body + body):
        if ln.startswith("v_fma_f32"):
            acc = ln.split()[1].rstrip(",")
            assert i - last.get(acc, -100) >= 16, ln
            last[acc] = i


def test_both_exits_finish_the_rotation():
    """Behind the loop, an even block count still owes what the next trip's first block would have rotated;
    an odd count (left after a first block) owes all 96 FMAs.  Loop + even tail = 96 + the carried part once more."""
    lines = _lines()
    back = next(i for i, ln in enumerate(lines) if ln == "s_cbranch_scc1 1b")
    odd = lines.index("2:")
    end = lines.index("3:")
    even_tail = [ln for ln in lines[back:odd] if ln.startswith("v_fma_f32")]
    odd_tail = [ln for ln in lines[odd:end] if ln.startswith("v_fma_f32")]
    top = lines.index("1:")
    mid = lines.index("s_cbranch_scc1 2f")
    carried = [ln for ln in lines[top:mid] if ln.startswith("v_fma_f32")]
    assert len(odd_tail) == 96 and len(set(odd_tail)) == 96
    assert even_tail == carried and 0 < len(carried) < 96
    in_second = [ln for ln in lines[mid:back] if ln.startswith("v_fma_f32")]
    assert in_second + carried == odd_tail


def test_kernel_keeps_two_waves_per_simd(gsdr_lib, tmp_path):
    """From the code object of the library as built: the kernel once, at most 256 VGPRs + AGPRs, at most 80 KiB of
    LDS (two workgroups per compute unit), no spills."""
    import shutil
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
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 256        # VGPRs + AGPRs on gfx90a and later
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 80 * 1024
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0
    assert found == 1
