"""Host-side checks of the direct folded matrix-core loop (tools/gen_ddc_mfma_ring16p4f.py,
csrc/ddc_mfma_ring16p4f_gen.h, ddc_mfma_ring16p4f_kernel): no GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gpu_sdr_amd", "csrc", "ddc_mfma_ring16p4f_gen.h")
KERNEL = "ddc_mfma_ring16p4f_kernel"
IMAGE = (0, 1, 1, 0)        # the phasor image of unit u: c, d, d, c (a0..a15 hold c, a16..a31 hold d)


def _lines():
    return re.findall(r'"(.*?)\\n\\t"', open(HEADER).read())


def _spans():
    """The two spans (parity A, parity B) of one trip of the loop."""
    lines = _lines()
    top = lines.index("1:")
    mid = lines.index("s_cbranch_scc1 2f")
    back = lines.index("s_cbranch_scc1 1b")
    return lines[top:mid], lines[mid:back]


def test_header_is_what_the_generator_emits():
    env = {k: v for k, v in os.environ.items() if not k.startswith("GEN_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ddc_mfma_ring16p4f.py")], capture_output=True,
                         text=True, check=True, env=env).stdout
    assert out == open(HEADER).read()


def test_loop_obeys_the_hazard_rules():
    spec = importlib.util.spec_from_file_location("check_asm_rules", os.path.join(ROOT, "tools", "check_asm_rules.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert chk.check(HEADER) == []


def test_span_has_48_mfmas_64_rotation_fmas_and_four_copies():
    for body in _spans():
        assert sum(ln.startswith("v_mfma_f32_16x16x32_f16") for ln in body) == 48
        assert sum(ln.startswith("v_fma_f32") for ln in body) == 64
        assert sum(ln.startswith("global_load_lds_dwordx4") for ln in body) == 4
        assert sum(ln == "s_barrier" for ln in body) == 1
    assert not any(ln.startswith("v_pk_") for ln in _lines())


def test_mfmas_sum_straight_into_re_and_im():
    """Re is the sum of units 0 and 1, Im of units 2 and 3 (24 MFMAs a tile set): the first MFMA into each of the
    eight product tiles of a span has C = 0, every other one accumulates onto its own destination; product registers
    are C/D only, and unit u multiplies by the images of (c, d, d, c) alone."""
    for body in _spans():
        mfmas = [re.fullmatch(r"v_mfma_f32_16x16x32_f16 v\[(\d+):\d+\], v\[(\d+):\d+\], a\[(\d+):\d+\], (\S+)", ln)
                 for ln in body if ln.startswith("v_mfma")]
        assert all(mfmas)
        seen = set()
        ks = {int(m.group(1)) for m in mfmas}
        assert len(ks) == 8
        for i, m in enumerate(mfmas):
            d, a, b, c = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            assert not any(k <= a < k + 4 for k in ks)
            assert b // 16 == IMAGE[i // 12] and b + 3 < 32
            if d in seen:
                assert c.startswith(f"v[{d}:")
            else:
                assert c == "0"
                seen.add(d)
        assert len(seen) == 8
        # the tiles of units 0, 1 and of units 2, 3 are two disjoint sets of four
        re_tiles = {int(m.group(1)) for m in mfmas[:24]}
        im_tiles = {int(m.group(1)) for m in mfmas[24:]}
        assert len(re_tiles) == len(im_tiles) == 4 and not re_tiles & im_tiles


def test_accumulators_are_reread_no_sooner_than_16_instructions_later():
    a, b = _spans()
    body = [ln for ln in a + b if not ln.endswith(":")]
    last = {}
    for i, ln in enumerate(body + body):
        if ln.startswith("v_fma_f32"):
            acc = ln.split()[1].rstrip(",")
            assert i - last.get(acc, -100) >= 16, ln
            last[acc] = i


def test_products_are_read_three_mfmas_after_their_last_one_and_before_their_next():
    """A rotation FMA reads a product tile no sooner than three MFMAs behind the last MFMA that summed into it, and
    with at least one other MFMA between it and the one that starts the tile anew (walked over two trips)."""
    a, b = _spans()
    body = [ln for ln in a + b if not ln.endswith(":")]
    stream = body + body + body
    writes = {}              # product register -> MFMA ordinals that write it
    n = 0
    for ln in stream:
        if ln.startswith("v_mfma"):
            d = int(re.match(r"v_mfma\S+ v\[(\d+):", ln).group(1))
            for r in range(d, d + 4):
                writes.setdefault(r, []).append(n)
            n += 1
    n = 0
    checked = 0
    for ln in stream:
        if ln.startswith("v_mfma"):
            n += 1
        elif ln.startswith("v_fma_f32") and 96 <= n < 192:       # the middle trip
            k = int(ln.split(",")[2].strip().lstrip("v"))
            before = max(w for w in writes[k] if w < n)
            after = min(w for w in writes[k] if w >= n)
            assert n - 1 - before >= 3 and after - n >= 1, (ln, n, before, after)
            checked += 1
    assert checked == 128


def test_both_exits_rotate_the_last_im():
    lines = _lines()
    back, odd, end = lines.index("s_cbranch_scc1 1b"), lines.index("2:"), lines.index("3:")
    for tail in (lines[back:odd], lines[odd:end]):
        fmas = [ln for ln in tail if ln.startswith("v_fma_f32")]
        assert len(fmas) == 32 and len(set(fmas)) == 32


def test_kernel_keeps_two_waves_per_simd(gsdr_lib, tmp_path):
    """From the code object of the library as built: the kernel once, at most 256 VGPRs + AGPRs, at most 80 KiB of
    LDS (two workgroups per compute unit), no spills, no scratch.  The register count is printed."""
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
            assert lds <= 80 * 1024
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0
    assert found == 1


@pytest.mark.parametrize("fm", [1, 2, 37, 4096, 99999, 100000, 199999])
def test_four_folded_sums_equal_the_complex_sum_and_the_gauss_fold(fm):
    """Re = V1 x c + V2 x d and Im = V3 x d + V4 x c over 32 partner pairs, the phase taken from the centre of the span
    in half samples, turned by the span phasor, give sum (a + i*b) * w^t over the whole window; per span they equal the
    Gauss fold's (P1 - P2, P3 - P1 - P2).  Odd and even tone frequencies, three spans, in double."""
    rate, nspan = 200000, 3
    rng = np.random.default_rng(fm)
    a = rng.standard_normal(64 * nspan)
    b = rng.standard_normal(64 * nspan)
    t = np.arange(64 * nspan)
    w = np.exp(-2j * np.pi * ((fm * t) % rate) / rate)              # host_phasor's sign
    want = np.sum((a + 1j * b) * w)
    j = np.arange(32)
    ph2 = (fm * (63 - 2 * j)) % (2 * rate)                           # half samples, exact integers
    c, d = np.cos(np.pi * ph2 / rate), np.sin(np.pi * ph2 / rate)    # w^(j - 31.5) = conj(w^(31.5 - j))
    acc = 0j
    for s in range(nspan):
        aj, bj = a[64 * s:64 * s + 32], b[64 * s:64 * s + 32]
        ap, bp = a[64 * s + 63 - j], b[64 * s + 63 - j]
        re_ = np.sum((aj + ap) * c) + np.sum((bp - bj) * d)
        im_ = np.sum((aj - ap) * d) + np.sum((bj + bp) * c)
        p1 = np.sum((aj + ap) * c)
        p2 = np.sum((bj - bp) * d)
        p3 = np.sum((aj + bj) * (c + d) + (ap + bp) * (c - d))
        assert abs(re_ - (p1 - p2)) <= 1e-12 and abs(im_ - (p3 - p1 - p2)) <= 1e-12
        ps2 = (fm * ((128 * s + 63) % (2 * rate))) % (2 * rate)
        pr, pi = np.cos(np.pi * ps2 / rate), -np.sin(np.pi * ps2 / rate)
        acc += (pr * re_ - pi * im_) + 1j * (pi * re_ + pr * im_)
    assert abs(acc - want) <= 1e-12
