"""Host-side checks of the pair-rotating three-product matrix-core loop (tools/gen_ddc_mfma_ring16p3r2.py,
csrc/ddc_mfma_ring16p3r2_gen.h, ddc_mfma_ring16p3r2_kernel): no GPU needed.  That the header is current and obeys the
hazard rules is checked in tests/test_host_logic.py, the kernel's code object in tests/test_mfma3_host.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gpu_sdr_amd", "csrc", "ddc_mfma_ring16p3r2_gen.h")


def _lines():
    return re.findall(r'"(.*?)\\n\\t"', open(HEADER).read())


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
