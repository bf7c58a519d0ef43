"""The three-product matrix-core DDC with one rotation per PAIR of blocks (ddc_convert3_kernel +
ddc_mfma_ring16p3r2_kernel; switch GSDR_MFMA_3M_ROT).

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin
file.  The cases, the comb and the helpers are those of tests/test_gpu_parity.py and tests/test_gpu_mfma3.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from test_gpu_parity import (DIRECT_CASES, TOL, crandn, make_direct, make_pfb, rel_err_per_tone, run_device, run_host)
from test_gpu_mfma3 import C3, VALU_CASES, _c3_handle, _hdr_errors, _HDR_REFS

pytestmark = pytest.mark.gpu

KERNEL = "ddc_mfma_ring16p_kernel"          # the name every pre-converted loop reports


@pytest.fixture
def forced_r2(monkeypatch):
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_MFMA_3M", "1")
    monkeypatch.setenv("GSDR_MFMA_3M_ROT", "2")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    monkeypatch.setenv("GSDR_TONES_FFT", "0")


def _is_r2(dem):
    d = dem.describe()
    return dem.kernel_name == KERNEL and d["complex_mac"] == 3 and d["rotation_blocks"] == 2


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_direct_parity_pair_rotation(cuda_device, gsdr_lib, oracle_mod, forced_r2, case):
    """One row tile, a partial last tile, N no multiple of 32, windows of one block, odd and even block counts,
    M*F no multiple of 32, F from 1 to 8, consecutive buffers through both entries."""
    N, rate, M, F, L, nbuf = case
    rng = np.random.default_rng(1000 + N + M)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    if N >= 3:
        freq[0], freq[1], freq[2] = 0, rate // 2 - 1, -(rate // 2) + 1
    dem = make_direct(freq, rate, M, F, L)
    if case in VALU_CASES:
        assert not dem.kernel_name.startswith("ddc_mfma"), dem.kernel_name
        assert dem.describe()["rotation_blocks"] == 1
    else:
        assert _is_r2(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"case {case} ({(M * F + 31) // 32} blocks) buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    if case not in VALU_CASES:
        assert _is_r2(dem)
    dem.close()


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5])
def test_shortest_windows(cuda_device, gsdr_lib, oracle_mod, forced_r2, blocks):
    """Windows of one to five blocks: both exits of the trip with no, one and two whole trips in front."""
    N, rate, F = 40, 1_000_000, 4
    M = 8 * blocks                      # M * F = 32 * blocks
    L = 64 * M
    rng = np.random.default_rng(31 + blocks)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_r2(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"{blocks} blocks buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    dem.close()


def test_tones_on_the_ddc_kernels_pair_rotation(cuda_device, gsdr_lib, oracle_mod, forced_r2):
    """TONES through the DDC kernels, buffer length no multiple of nfft (short last batches)."""
    N, rate, nfft, avg, L, nbuf = 5, 200_000_000, 1000, 4, 50_123, 4
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    assert _is_r2(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
    emitted = 0
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        emitted += len(yr)
        if len(yr):
            err = rel_err_per_tone(y.reshape(-1, N), yr)
            print(f"tones buffer {c}: worst per-tone error {err.max():.3e}")
            assert err.max() <= TOL, (c, err.max())
    assert emitted > 0
    assert _is_r2(dem)
    dem.close()


@pytest.mark.parametrize("kind", ["1e8", "1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (32, 200_000_000, 1000, 4, 200_000),
                                   (12, 9_000_000, 90, 4, 90_000)], ids=["M100", "M1000", "M90pad"])
def test_extreme_and_nonfinite_samples_pair_rotation(cuda_device, gsdr_lib, oracle_mod, forced_r2, kind, shape):
    """test_direct_extreme_and_nonfinite_samples of tests/test_gpu_parity.py, same three assertions."""
    N, rate, M, F, L = shape
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_r2(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    at = (L // M // 2) * M + 3
    rows = np.arange(L // M)
    hit = (rows >= at // M) & (rows <= at // M + F - 1)
    far = near = 0.0
    for c in range(4):
        x = host_tones(L, c * L, rate, freq, ampl, phase, sigma=1e-3, seed=700 + c)
        if c == 1:
            rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
            x[at] = {"1e8": np.complex64(1e8 * rms * (0.6 + 0.8j)), "1e10": np.complex64(1e10 * rms * (0.6 - 0.8j)),
                     "inf": np.complex64(complex(np.inf, 0.5)), "nan": np.complex64(complex(0.25, np.nan))}[kind]
        y = run_device(dem, x, cuda_device).reshape(-1, N)
        with np.errstate(invalid="ignore", over="ignore"):
            yr = ref.process(x)
        assert y.shape == yr.shape
        fin_y = np.isfinite(y.real) & np.isfinite(y.imag)
        fin_r = np.isfinite(yr.real) & np.isfinite(yr.imag)
        if c == 1:
            if kind in ("inf", "nan"):
                assert not fin_r[hit].any(), "the oracle's rows that hold the sample are non-finite"
                np.testing.assert_array_equal(fin_y, fin_r, err_msg=f"{kind}: non-finite outputs elsewhere than the oracle's")
            else:
                assert fin_y.all()
                near = max(near, float(rel_err_per_tone(y[hit], yr[hit], "rows whose window holds the spike").max()))
            keep = ~hit
            keep[:F] = False
            e = rel_err_per_tone(y[keep], yr[keep], "rows of the bad sample's buffer that do not hold it")
        else:
            assert fin_y.all(), (kind, c)
            e = rel_err_per_tone(y[F:] if c == 0 else y, yr[F:] if c == 0 else yr, "the other buffers")
        far = max(far, float(e.max()))
    dem.close()
    print(f"{kind} {shape}: far {far:.3e} near {near:.3e}")
    assert far <= TOL, (kind, far)
    assert near <= TOL, (kind, near)


def _c3_default_rotation(monkeypatch):
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    d, _ = _c3_handle()
    info = d.describe()
    d.close()
    return info["rotation_blocks"], info["rotation_min_blocks"]


@pytest.mark.parametrize("rot_env", [None, "2"], ids=["default", "pair"])
def test_c3_is_bit_identical_through_every_entry(cuda_device, gsdr_lib, monkeypatch, rot_env):
    """C3 by default (the loop its handle chose, reported and recorded) and with the pair rotation forced:
    process_device on two caller streams, submit_device in between, the synchronous host entry -- bit-equal to one
    in-order stream."""
    import torch
    from gpu_sdr_amd.source import device_tones
    rot, T = _c3_default_rotation(monkeypatch)
    assert rot == (2 if T <= 125 else 1), (rot, T)
    record_info(rot, "C3 by default: blocks per rotation")
    if rot_env:
        monkeypatch.setenv("GSDR_MFMA_3M_ROT", rot_env)
        rot = int(rot_env)
    N, rate, M, F, L = C3
    a, (freq, ampl, phase) = _c3_handle()
    b, _ = _c3_handle()

    def same(d):
        i = d.describe()
        return d.kernel_name == KERNEL and i["complex_mac"] == 3 and i["rotation_blocks"] == rot

    assert same(a) and same(b)
    pattern = ["s1", "sub", "s2", "host", "sub", "sub", "s1", "host", "sub"]
    xs = []
    for k in range(len(pattern)):
        x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
        device_tones(x, k * L, rate, freq, ampl, phase, sigma=1e-3, seed=300 + k)
        xs.append(x)
    torch.cuda.synchronize()
    want = []
    for x in xs:
        out = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
        n = a.process_device(x, out)
        torch.cuda.synchronize()
        assert same(a)
        want.append(out[:n].cpu().numpy())
    s1, s2 = torch.cuda.Stream(cuda_device), torch.cuda.Stream(cuda_device)
    outs = [torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in pattern]
    got, pending = [None] * len(pattern), []

    def drain():
        while pending:
            j = pending.pop(0)
            n = b.wait()
            torch.cuda.synchronize()
            got[j] = outs[j][:n].cpu().numpy()

    for k, how in enumerate(pattern):
        if how == "sub":
            if len(pending) == 3:
                j = pending.pop(0)
                n = b.wait()
                got[j] = (j, n)
            b.submit_device(xs[k], outs[k])
            pending.append(k)
        elif how == "host":
            drain()
            got[k] = run_host(b, xs[k].cpu().numpy())
        else:
            st = s1 if how == "s1" else s2
            n = b.process_device(xs[k], outs[k], st)
            got[k] = (k, n)
        assert same(b), (k, how)
    drain()
    torch.cuda.synchronize()
    for k, how in enumerate(pattern):
        y = got[k]
        if isinstance(y, tuple):
            y = outs[y[0]][:y[1]].cpu().numpy()
        assert y.size == want[k].size, (k, how)
        np.testing.assert_array_equal(y, want[k], err_msg=f"buffer {k} via {how}")
    a.close()
    b.close()


def test_switch_and_threshold(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_3M_ROT: 1 never, 2 wherever the handle is three-product, unset from rotation_min_blocks on; a handle
    forced to three products on a short window keeps the 32-sample loop; four-product handles are not touched."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def rot(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["rotation_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    _, _, T = rot(1000)
    assert T in (94, 125, 250), T
    assert rot(1000, GSDR_MFMA_3M_ROT="1")[:2] == (3, 1)
    assert rot(1000, GSDR_MFMA_3M_ROT="2")[:2] == (3, 2)
    assert rot(2000)[:2] == (3, 2)
    assert rot(T * 8)[:2] == (3, 2)                       # a window of exactly T blocks
    assert rot(256, GSDR_MFMA_3M="1")[:2] == (3, 1)       # forced three products on 32 blocks: today's loop
    assert rot(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2")[:2] == (3, 2)
    assert rot(1000, GSDR_MFMA_3M="0", GSDR_MFMA_3M_ROT="2")[:2] == (4, 1)
    if T > 94:
        assert rot(750)[:2] == (3, 1)


HDR_R2_DECIMS = [750, 1000, 2000]        # windows of 94, 125, 250 blocks


def test_hdr_comb_default_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """The measurement behind kRot2MinBlocks (csrc/demod.cpp): the 60 dB comb of test_gpu_mfma3.py
    (64 tones at 200 Msps, F = 4, L = 200 * M, pre-converted operands forced), windows of 94, 125, 250 blocks.
    Rule, per tone: err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) against the fp64 oracle on the same buffers.  Asserted for GSDR_MFMA_3M_ROT unset
    at every length; the figures of both loops forced (ROT = 1, = 2) are recorded."""
    span_db = 60
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    failures = []
    for M in HDR_R2_DECIMS:
        res = {}
        for mode in ("1", "2", None):
            if mode is None:
                monkeypatch.delenv("GSDR_MFMA_3M_ROT", raising=False)
            else:
                monkeypatch.setenv("GSDR_MFMA_3M_ROT", mode)
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
            assert res[mode][2] == 3, (M, mode)
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio = res["2"][0] / np.maximum(res["1"][0], 1e-12)
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound per block {worst['1']:.3f} per pair {worst['2']:.3f} "
              f"default {worst[None]:.3f}; worst err per block {res['1'][0].max():.3e} per pair {res['2'][0].max():.3e} "
              f"fp32 order {err32.max():.3e}; per-tone ratio pair/block median {np.median(ratio):.2f} max {ratio.max():.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default rotation")
        for m, name in (("1", "rotation per block"), ("2", "rotation per pair"), (None, "default")):
            record_info(float(res[m][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, {name}")
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(float(np.median(ratio)), f"{span_db} dB, M {M} ({nblk} blocks): median per-tone ratio pair / block")
        record_info(float(ratio.max()), f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio pair / block")
        if worst[None] > 1.0:
            failures.append((M, worst[None]))
    assert not failures, failures


def test_c3_full_size_margin(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """C3 against the oracle through the default loop of its handle: the margin to record beside the 4.0e-7 of the
    32-sample loop."""
    from test_gpu_parity import _full_size_direct
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC"):
        monkeypatch.delenv(k, raising=False)
    _full_size_direct(cuda_device, oracle_mod, N=2048, M=1000, nbuf=3, subset=12)
