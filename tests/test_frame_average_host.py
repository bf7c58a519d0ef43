"""Mean of k consecutive PFB frames, the part that needs no GPU: gsdr_frame_average_host against a numpy float32 model
of the arithmetic in include/gsdr.h (bit for bit), its independence of where the stream is cut, its error against
float64, the same translation unit under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program, and
the method of the C++ drop-in class."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from _frame_average import CASES, KINDS, bits, case_input, model, nonfinite_groups
from _margins import record_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_frames,n_ch,k,count", CASES)
def test_host_matches_numpy_model_bit_for_bit(gsdr_lib, n_frames, n_ch, k, count, kind):
    import gpu_sdr_amd as g
    frames, acc, nan_f, inf_f = case_input(n_frames, n_ch, k, count)
    keep_frames, keep_acc = frames.copy(), None if acc is None else acc.copy()
    out, acc_out, c = g.frame_average(frames, k, kind, count, acc)
    m_out, m_acc, m_c = model(frames, k, kind, count, acc)
    assert out.shape == m_out.shape == ((count + n_frames) // k, n_ch) and c == m_c == (count + n_frames) % k
    np.testing.assert_array_equal(bits(out), bits(m_out))
    np.testing.assert_array_equal(bits(acc_out), bits(m_acc))
    np.testing.assert_array_equal(bits(frames), bits(keep_frames))          # inputs are not modified
    if acc is not None:
        np.testing.assert_array_equal(bits(acc), bits(keep_acc))
    # an Inf or NaN reaches exactly the groups that hold it (slot `rows` is the open group: the accumulator)
    rows = out.shape[0]
    slots = np.concatenate([out, acc_out[None, :]]) if c else out
    bad = nonfinite_groups(n_frames, k, count, (nan_f, inf_f))
    for s in range(slots.shape[0]):
        if s in bad:
            assert not np.isfinite(slots[s].real).any(), (s, bad, rows)
            assert not np.isfinite(slots[s].imag).any() if kind == "complex" else not slots[s].imag.any()
        else:
            assert np.isfinite(slots[s].real).all() and np.isfinite(slots[s].imag).all(), (s, bad, rows)
    if c == 0:
        assert not bits(acc_out).any()                                       # +0, +0 when no group is open


def test_minus_zero_survives_a_group_of_one_and_the_first_frame(gsdr_lib):
    import gpu_sdr_amd as g
    x = np.array([[complex(-0.0, -0.0), complex(0.0, -0.0)]], dtype=np.complex64)
    out, acc_out, c = g.frame_average(x, 1, "complex")
    np.testing.assert_array_equal(bits(out), bits(x))                        # acc = t_0, times 1.0f
    out, acc_out, c = g.frame_average(x, 2, "complex")
    assert c == 1 and out.shape == (0, 2)
    np.testing.assert_array_equal(bits(acc_out), bits(x[0]))
    out, _, _ = g.frame_average(x, 1, "power")
    assert not bits(out).any()                                               # (-0)^2 + (-0)^2 = +0, imaginary part +0


@pytest.mark.parametrize("k", [2, 3, 7, 64])
def test_result_does_not_depend_on_the_cuts(gsdr_lib, k):
    import gpu_sdr_amd as g
    n_frames, n_ch = 300, 37
    for seed in range(20):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((n_frames, n_ch)) + 1j * rng.standard_normal((n_frames, n_ch))).astype(np.complex64)
        for kind in KINDS:
            whole, whole_acc, whole_c = g.frame_average(x, k, kind)
            cuts = np.sort(rng.integers(0, n_frames + 1, size=int(rng.integers(1, 12))))
            cuts = np.concatenate([[0], cuts, cuts[-1:], [n_frames]])        # a zero-length piece in every run
            parts, acc, c = [], None, 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                out, acc, c = g.frame_average(np.ascontiguousarray(x[a:b]), k, kind, c, acc if c else None)
                parts.append(out)
            np.testing.assert_array_equal(bits(np.concatenate(parts)), bits(whole))
            np.testing.assert_array_equal(bits(acc), bits(whole_acc))
            assert c == whole_c


def test_error_against_float64_on_unit_noise(gsdr_lib):
    """Per-channel relative error of the float32 chain against the float64 mean: k - 1 additions and one product, each
    within 2^-24 relative, on sums that grow like sqrt(k) (complex) or k (power).  The model gives <= 2.0e-7 (complex)
    and <= 1.5e-7 (power) for k <= 64; the bar is 1e-6."""
    import gpu_sdr_amd as g
    rng = np.random.default_rng(5)
    n_ch = 256
    for k in (2, 3, 7, 16, 64):
        n_frames = 32 * k
        x = (rng.standard_normal((n_frames, n_ch)) + 1j * rng.standard_normal((n_frames, n_ch))).astype(np.complex64)
        x64 = x.astype(np.complex128).reshape(32, k, n_ch)
        for kind, ref in (("complex", x64.mean(axis=1)), ("power", (np.abs(x64) ** 2).mean(axis=1))):
            out, _, c = g.frame_average(x, k, kind)
            assert c == 0 and out.shape == (32, n_ch)
            err = np.linalg.norm(out - ref, axis=0) / np.linalg.norm(ref, axis=0)
            record_margin(err.max(), f"{kind} k={k}")
            print(f"frame average vs fp64: {kind} k={k}: worst per-channel relative error {err.max():.3e}")
            assert err.max() <= 1e-6, (kind, k, err.max())
            if kind == "power":
                assert not out.imag.any()


def test_bad_arguments_are_refused_with_a_message(gsdr_lib):
    x = np.zeros((4, 3), dtype=np.complex64)
    acc, out = np.zeros(3, dtype=np.complex64), np.zeros((4, 3), dtype=np.complex64)
    def call(n_frames=4, n_ch=3, k=2, kind=0, count=0, frames=x, acc_in=acc, acc_out=acc.copy(), o=out):
        p = lambda a: None if a is None else a.ctypes.data
        return gsdr_lib.gsdr_frame_average_host(p(frames), n_frames, n_ch, k, kind, count, p(acc_in), p(acc_out), p(o))
    assert call() == 2
    for kw in (dict(k=0), dict(k=(1 << 20) + 1), dict(kind=2), dict(kind=-1), dict(count=2), dict(count=-1), dict(n_ch=0),
               dict(n_frames=-1), dict(acc_out=None), dict(frames=None), dict(count=1, acc_in=None), dict(o=None)):
        assert call(**kw) == -1, kw
        assert b"gsdr_frame_average" in gsdr_lib.gsdr_last_error(None), kw
    assert call(n_frames=0, frames=None, o=None) == 0                        # nothing to read, no row to write
    assert call(n_frames=1, o=None) == 0                                     # no group completes: out is not needed


SAN_DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

// the six cases of tests/_frame_average.py, both kinds, on buffers of exactly the documented sizes
int main() {
    const int cases[6][4] = {{1, 1, 1, 0}, {7, 3, 2, 1}, {40, 64, 5, 3}, {3, 1000, 8, 6}, {2, 130, 16, 0}, {257, 1230, 16, 15}};
    unsigned seed = 1u;
    long long rows_total = 0;
    for (const auto &c : cases)
        for (int kind = 0; kind < 2; ++kind) {
            const int n_frames = c[0], n_ch = c[1], k = c[2], count = c[3];
            std::vector<gsdr_c64> frames((size_t)n_frames * n_ch), acc_in((size_t)(count > 0 ? n_ch : 0)), acc_out((size_t)n_ch);
            const int rows = (count + n_frames) / k;
            std::vector<gsdr_c64> out((size_t)rows * n_ch);
            for (auto &v : frames) {
                seed = seed * 1664525u + 1013904223u;
                v.x = (float)(int)(seed >> 8) * 1e-6f;
                seed = seed * 1664525u + 1013904223u;
                v.y = (seed & 64u) ? -0.0f : (float)(int)(seed >> 8) * -1e-6f;
            }
            if (n_frames > 4)
                for (int ch = 0; ch < n_ch; ++ch) frames[(size_t)2 * n_ch + ch] = gsdr_c64{std::numeric_limits<float>::quiet_NaN(), 0.f};
            if (n_frames > 30)
                for (int ch = 0; ch < n_ch; ++ch) frames[(size_t)(n_frames - 2) * n_ch + ch] = gsdr_c64{std::numeric_limits<float>::infinity(), 1.f};
            for (auto &v : acc_in) v = gsdr_c64{1.f, -1.f};
            const int r = gsdr_frame_average_host(n_frames ? frames.data() : nullptr, n_frames, n_ch, k, kind, count,
                                                  count ? acc_in.data() : nullptr, acc_out.data(), rows ? out.data() : nullptr);
            if (r != rows) return 3;
            rows_total += r;
        }
    if (gsdr_frame_average_host(nullptr, 0, 1, 0, 0, 0, nullptr, nullptr, nullptr) != -1) return 4;
    std::printf("rows %lld\n", rows_total);
    return 0;
}
'''


def test_host_function_under_asan_and_ubsan(tmp_path):
    """A stand-alone program (its own main) with the translation unit that holds gsdr_frame_average_host; nothing is
    loaded into Python under a sanitizer."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "driver.cpp").write_text(SAN_DRIVER)
    exe = tmp_path / "driver"
    build = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"),
                            os.path.join(ROOT, "gpu_sdr_amd", "csrc", "host_logic.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    expect = 2 * sum((c + n) // k for n, _, k, c in CASES)
    assert run.stdout.split() == ["rows", str(expect)], run.stdout


def test_cpp_shim_method_compiles_with_gxx(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "USRP_demodulator.hpp"\n'
                   "bool f(RX_buffer_demodulator *d) { return d->set_frame_average(16) && d->set_frame_average(4, GSDR_AVERAGE_POWER)\n"
                   "  && d->frame_average() == 4; }\n"
                   "int main(){ return sizeof(&f) > 0 && GSDR_AVERAGE_COMPLEX == 0 && GSDR_AVERAGE_POWER == 1 ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_wrapper_checks_its_arguments(gsdr_lib):
    import gpu_sdr_amd as g
    x = np.zeros((4, 3), dtype=np.complex64)
    with pytest.raises(ValueError):
        g.frame_average(x, 0)
    with pytest.raises(ValueError):
        g.frame_average(x, 2, count=2, acc=np.zeros(3, dtype=np.complex64))
    with pytest.raises(ValueError):
        g.frame_average(x, 2, count=1)                                       # an open group without its sums
    with pytest.raises(ValueError):
        g.frame_average(x, 2, kind="amplitude")
    with pytest.raises(ValueError):
        g.frame_average(np.zeros(12, dtype=np.complex64), 2)
    with pytest.raises(TypeError):
        g.frame_average(x.astype(np.complex128), 2)
    with pytest.raises(TypeError):
        g.frame_average(x, 2, count=1, acc=np.zeros(4, dtype=np.complex64))
