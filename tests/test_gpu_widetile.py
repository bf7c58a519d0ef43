"""The direct folded matrix-core DDC on wave tiles of 16 rows x 64 tones (ddc_mfma_ring16p4fw_kernel, DESIGN.md section
4.1h; switch GSDR_MFMA_WAVE_TONES): the images, tables and arithmetic of ddc_mfma_ring16p4f_kernel, so its bits.

Every case builds two handles from the same parameters, GSDR_MFMA_WAVE_TONES = 64 and = 32, feeds both three
consecutive buffers (the head and the tail are carried across calls) and asks for equal bytes; the 64 handle is also
held to the bar of 1e-5 per tone against the fp64 oracle.  The cases every product loop runs are in
tests/test_gpu_product_loops.py; the helpers and the forced loops are those of test_gpu_parity.py, test_gpu_extents.py
and tests/_product_loops.py."""
import numpy as np
import pytest

from _product_loops import LOOPS, force, is_loop
from test_gpu_extents import clean_env
from test_gpu_parity import TOL, crandn, make_direct, rel_err_per_tone, run_device, run_host

pytestmark = pytest.mark.gpu

WIDE_ENV, NARROW_ENV = LOOPS["p4fw"][0], LOOPS["p4f"][0]
FOLD4_ENV = {k: v for k, v in WIDE_ENV.items() if k != "GSDR_MFMA_WAVE_TONES"}      # the tile left to the handle


def _is_wide(dem, tones=64):
    return is_loop(dem, {64: "p4fw", 32: "p4f"}[tones])


def _pair(monkeypatch, cuda_device, oracle_mod, N, rate, M, F, L, seed):
    """Three buffers through a 64 handle and a 32 handle: equal bytes, and the 64 handle within TOL of the oracle."""
    rng = np.random.default_rng(seed)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    force(monkeypatch, "p4fw")
    wide = make_direct(freq, rate, M, F, L)
    assert _is_wide(wide, 64), (wide.kernel_name, wide.describe())
    force(monkeypatch, "p4f")
    narrow = make_direct(freq, rate, M, F, L)
    assert _is_wide(narrow, 32), (narrow.kernel_name, narrow.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    worst = 0.0
    for c in range(3):
        x = crandn(rng, L)
        y = run_device(wide, x, cuda_device)
        w = run_device(narrow, x, cuda_device)
        assert y.size == w.size == N * (L // M), (c, y.size, w.size)
        np.testing.assert_array_equal(y.view(np.int32), w.view(np.int32), err_msg=f"buffer {c}: 64 against 32")
        err = rel_err_per_tone(y.reshape(-1, N), ref.process(x))
        worst = max(worst, float(err.max()))
        assert err.max() <= TOL, (c, err.max())
    assert _is_wide(wide, 64) and _is_wide(narrow, 32)
    wide.close()
    narrow.close()
    return worst


# rows of the tone cases: 8 (half a 16-row tile) ... 40 (two and a half)
TONE_ROWS = {1: 8, 32: 24, 33: 40, 64: 16, 65: 40, 96: 33, 224: 40, 256: 17, 257: 40, 288: 40}


@pytest.mark.parametrize("N", sorted(TONE_ROWS))
def test_tones_bit_identical(cuda_device, gsdr_lib, oracle_mod, monkeypatch, N):
    """A second tile that is absent (1, 32, 65 .. 96: odd tile counts) or partly filled (33, 257), a full workgroup
    (256), a second workgroup with one live wave and three idle ones (257, 288), two tone groups; windows of 3 blocks."""
    rows, M, F = TONE_ROWS[N], 24, 4
    worst = _pair(monkeypatch, cuda_device, oracle_mod, N, 1_000_000, M, F, rows * M, 100 + N)
    print(f"{N} tones, {rows} rows: worst per-tone error {worst:.3e}")


@pytest.mark.parametrize("nout", [1, 8, 16, 17, 24, 32, 33, 40, 130])
def test_rows_bit_identical(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nout):
    """A lone half tile (1, 8, 16), an empty rh = 1 workgroup (1 .. 16, 33, 40), short last tiles in either half (17,
    24, 33, 40, 130) and nine 16-row tiles (130: the XCD round wraps).  65 tones, windows of 3 blocks (M = 48, F = 2:
    a buffer of one row still holds the carry)."""
    M, F = 48, 2
    worst = _pair(monkeypatch, cuda_device, oracle_mod, 65, 1_000_000, M, F, nout * M, 200 + nout)
    print(f"{nout} rows: worst per-tone error {worst:.3e}")


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5, 6, 7, 9])
def test_window_bit_identical(cuda_device, gsdr_lib, oracle_mod, monkeypatch, blocks):
    """One to five spans, a half-empty last span (odd counts), the three-slot prologue longer (1 .. 4 blocks) and
    shorter (7, 9) than the window, both exits of the trip.  65 tones, 40 rows."""
    M, F = 8 * blocks, 4
    worst = _pair(monkeypatch, cuda_device, oracle_mod, 65, 1_000_000, M, F, 40 * M, 300 + blocks)
    print(f"{blocks} blocks: worst per-tone error {worst:.3e}")


def test_window_no_multiple_of_32_or_64_bit_identical(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """M = 90, F = 4: 360 samples, 12 blocks of which the last holds 8 samples."""
    worst = _pair(monkeypatch, cuda_device, oracle_mod, 65, 9_000_000, 90, 4, 40 * 90, 390)
    print(f"M 90: worst per-tone error {worst:.3e}")


def test_one_handle_every_entry_widetile(cuda_device, gsdr_lib, monkeypatch):
    """One handle, one loop: process_device, submit_device / wait and the host entry give the same bits for the same
    buffers (288 tones, M 1000, F 4, L 200 000: 125 blocks, 200 rows), and they are the bits of the 32-tone tile."""
    import torch
    from gpu_sdr_amd.source import tone_comb
    N, rate, M, F, L = 288, 200_000_000, 1000, 4, 200_000
    freq, _, _ = tone_comb(N, rate, seed=44)
    rng = np.random.default_rng(444)
    xs = [crandn(rng, L) for _ in range(3)]
    got = {}
    for entry in ("process", "submit", "host", "narrow"):
        force(monkeypatch, "p4f" if entry == "narrow" else "p4fw")
        dem = make_direct(freq, rate, M, F, L)
        assert _is_wide(dem, 32 if entry == "narrow" else 64), (dem.kernel_name, dem.describe())
        ys = []
        for x in xs:
            if entry == "host":
                ys.append(run_host(dem, x))
                continue
            xin = torch.from_numpy(x).to(cuda_device)
            out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
            if entry == "submit":
                dem.submit_device(xin, out)
                n = dem.wait()
            else:
                n = dem.process_device(xin, out)
            torch.cuda.synchronize()
            ys.append(out[:n].cpu().numpy())
        assert _is_wide(dem, 32 if entry == "narrow" else 64), entry
        dem.close()
        got[entry] = ys
    for entry in ("submit", "host", "narrow"):
        for k, (y, w) in enumerate(zip(got[entry], got["process"])):
            assert y.size == w.size == N * (L // M), (entry, k)
            np.testing.assert_array_equal(y.view(np.int32), w.view(np.int32), err_msg=f"buffer {k} via {entry}")


def test_switch_wave_tones(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_WAVE_TONES: unset, a handle of four products takes the 64-tone tile where that launches no more waves
    (288 tones x 125 blocks x 40 rows: 3 x 2 workgroups against 2 x 3) and keeps the 32-tone tile where it would not (64
    tones: 3 x 1 against 2 x 1); 32 and 64 pick what they name; a handle that does not sum the four products reports
    32 whatever is set."""
    from gpu_sdr_amd.source import tone_comb
    rate, M, F, L = 200_000_000, 1000, 4, 40_000

    def tones_of(N, env):
        clean_env(monkeypatch, env)
        freq, _, _ = tone_comb(N, rate, seed=1)
        d = make_direct(freq, rate, M, F, L)
        i = d.describe()
        d.close()
        return i["fold_products"], i["wave_tones"]

    assert tones_of(288, FOLD4_ENV) == (4, 64)
    assert tones_of(64, FOLD4_ENV) == (4, 32)
    for N in (64, 288):
        assert tones_of(N, NARROW_ENV) == (4, 32)
        assert tones_of(N, WIDE_ENV) == (4, 64)
        for w in ("32", "64"):
            assert tones_of(N, dict(FOLD4_ENV, GSDR_MFMA_FOLD_PRODUCTS="3", GSDR_MFMA_WAVE_TONES=w)) == (3, 32)
            assert tones_of(N, dict(FOLD4_ENV, GSDR_MFMA_FOLD="0", GSDR_MFMA_WAVE_TONES=w)) == (0, 32)
