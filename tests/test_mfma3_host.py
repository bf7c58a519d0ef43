"""Host-side checks of the three-product matrix-core loop (tools/gen_ddc_mfma_ring16p3.py,
csrc/ddc_mfma_ring16p3_gen.h, ddc_mfma_ring16p3_kernel) and of the code objects of both three-product kernels: no GPU
needed.  That the headers are current and obey the hazard rules is checked in tests/test_host_logic.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gpu_sdr_amd", "csrc", "ddc_mfma_ring16p3_gen.h")


def test_loop_has_36_mfmas_and_96_rotation_fmas_per_block():
    lines = re.findall(r'"(.*?)\\n\\t"', open(HEADER).read())
    top = lines.index("1:")
    back = next(i for i, ln in enumerate(lines) if ln == "s_cbranch_scc1 1b")
    body = lines[top:back]                    # two blocks per trip
    assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in body) == 2 * 36
    assert sum(ln.startswith("v_fma_f32") for ln in body) == 2 * 96
    assert sum(ln.startswith("global_load_lds_dwordx4") for ln in body) == 2 * 3
    assert not any(ln.startswith("v_pk_") for ln in lines)


@pytest.mark.parametrize("kernel", ["ddc_mfma_ring16p3_kernel", "ddc_mfma_ring16p3r2_kernel"])
def test_kernel_keeps_two_waves_per_simd(gsdr_lib, tmp_path, kernel):
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
            if not name or kernel not in name.group(1):
                continue
            found += 1
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 256        # VGPRs + AGPRs on gfx90a and later
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 80 * 1024
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0
    assert found == 1
