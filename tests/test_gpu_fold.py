"""The folded three-product matrix-core DDC (ddc_convert3f_kernel + ddc_mfma_ring16p3f_kernel, DESIGN.md section
4.1f; switch GSDR_MFMA_FOLD): the even and odd sums of each 64-sample span over 32 partner pairs.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  The
cases, the comb and the helpers are those of tests/test_gpu_parity.py, test_gpu_mfma3.py, test_gpu_mfma3r2.py and
test_gpu_extents.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from test_gpu_parity import (DIRECT_CASES, TOL, crandn, make_direct, make_pfb, rel_err_per_tone, run_device, run_host)
from test_gpu_mfma3 import C3, VALU_CASES, _c3_handle, _hdr_errors, _HDR_REFS
from test_gpu_extents import (DIRECT_ENGINES, S_C3, S_N65, S_ODD, clean_env, direct_inputs, expect_kernel, run_case)

pytestmark = pytest.mark.gpu

KERNEL = "ddc_mfma_ring16p_kernel"          # the name every pre-converted loop reports
FOLD_ENV = dict(DIRECT_ENGINES["mac3r2"][0], GSDR_MFMA_FOLD="1")      # forced_r2 of test_gpu_mfma3r2.py + the fold


@pytest.fixture
def forced_fold(monkeypatch):
    for k, v in FOLD_ENV.items():
        monkeypatch.setenv(k, v)


def _is_fold(dem):
    d = dem.describe()
    return dem.kernel_name == KERNEL and (d["complex_mac"], d["rotation_blocks"], d["fold"]) == (3, 2, 1)


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_direct_parity_fold(cuda_device, gsdr_lib, oracle_mod, forced_fold, case):
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
        assert dem.describe()["fold"] == 0
    else:
        assert _is_fold(dem), (dem.kernel_name, dem.describe())
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
        assert _is_fold(dem)
    dem.close()


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5])
def test_shortest_windows_fold(cuda_device, gsdr_lib, oracle_mod, forced_fold, blocks):
    """Windows of one to five blocks: a half-empty last span (1, 3, 5) or a whole one, with no, one and two whole
    spans in front; both exits of the trip."""
    N, rate, F = 40, 1_000_000, 4
    M = 8 * blocks                      # M * F = 32 * blocks
    L = 64 * M
    rng = np.random.default_rng(31 + blocks)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"{blocks} blocks buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    dem.close()


def test_window_no_multiple_of_32_or_64_fold(cuda_device, gsdr_lib, oracle_mod, forced_fold):
    """M = 90, F = 4: M * F = 360 is a multiple of neither 32 nor 64 (12 blocks, the last one 8 samples long)."""
    N, rate, M, F, L = 12, 9_000_000, 90, 4, 90_000
    rng = np.random.default_rng(90)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        err = rel_err_per_tone(y.reshape(-1, N), ref.process(x))
        print(f"M 90 buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    dem.close()


def test_tones_on_the_ddc_kernels_fold(cuda_device, gsdr_lib, oracle_mod, forced_fold):
    """TONES through the DDC kernels, buffer length no multiple of nfft (short last batches)."""
    N, rate, nfft, avg, L, nbuf = 5, 200_000_000, 1000, 4, 50_123, 4
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    assert _is_fold(dem), (dem.kernel_name, dem.describe())
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
    assert _is_fold(dem)
    dem.close()


@pytest.mark.parametrize("kind", ["1e8", "1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (32, 200_000_000, 1000, 4, 200_000),
                                   (12, 9_000_000, 90, 4, 90_000)], ids=["M100", "M1000", "M90pad"])
def test_extreme_and_nonfinite_samples_fold(cuda_device, gsdr_lib, oracle_mod, forced_fold, kind, shape):
    """test_direct_extreme_and_nonfinite_samples of tests/test_gpu_parity.py, same three assertions."""
    N, rate, M, F, L = shape
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold(dem), (dem.kernel_name, dem.describe())
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


@pytest.mark.parametrize("shape", [S_N65, S_ODD, S_C3], ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_direct_extents_fold(cuda_device, gsdr_lib, oracle_mod, monkeypatch, shape):
    """The guard zones of tests/_extents.py around input and output (both patterns, both offsets of each), through
    process_device and submit_device: 65 tones and a last row tile of 4 rows over 12.5 blocks (a half-empty last span);
    an odd row stride with F = 5 (185 samples: three spans, the last one short); the C3 block (125 blocks)."""
    N, rate, M, F, L = shape
    clean_env(monkeypatch, FOLD_ENV)
    freq, xs, yrs = direct_inputs(shape, oracle_mod)

    def expect(dem, ran):
        expect_kernel(KERNEL, 3, 2)(dem, ran)
        assert dem.describe()["fold"] == 1

    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), expect, xs, yrs, N)


def _c3_default(monkeypatch):
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD"):
        monkeypatch.delenv(k, raising=False)
    d, _ = _c3_handle()
    info = d.describe()
    d.close()
    return info["fold"], info["fold_min_blocks"]


@pytest.mark.parametrize("fold_env", [None, "1"], ids=["default", "fold"])
def test_c3_is_bit_identical_through_every_entry_fold(cuda_device, gsdr_lib, monkeypatch, fold_env):
    """C3 by default (the loop its handle chose, reported and recorded) and with the fold forced: process_device on
    two caller streams, submit_device in between, the synchronous host entry -- bit-equal to one in-order stream."""
    import torch
    from gpu_sdr_amd.source import device_tones
    fold, T = _c3_default(monkeypatch)
    assert fold == (1 if T <= 125 else 0), (fold, T)
    record_info(fold, "C3 by default: fold")
    if fold_env:
        monkeypatch.setenv("GSDR_MFMA_FOLD", fold_env)
        fold = int(fold_env)
    N, rate, M, F, L = C3
    a, (freq, ampl, phase) = _c3_handle()
    b, _ = _c3_handle()

    def same(d):
        i = d.describe()
        return d.kernel_name == KERNEL and (i["complex_mac"], i["rotation_blocks"], i["fold"]) == (3, 2, fold)

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


def test_switch_and_threshold_fold(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_FOLD: 0 never, 1 wherever the handle is three-product and rotates per pair, unset from
    fold_min_blocks on; a handle that rotates per block (GSDR_MFMA_3M_ROT=1) and four-product handles are not touched;
    complex_mac and rotation_blocks are what they were."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def fold(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["fold"], i["fold_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    T = fold(1000)[3]
    assert T in (94, 125, 250), T
    above, below = T * 8, (T - 1) * 8                     # windows of exactly T and of T - 1 blocks
    assert fold(above)[:3] == (3, 2, 1)
    assert fold(2000)[:3] == (3, 2, 1)
    assert fold(above, GSDR_MFMA_FOLD="0")[:3] == (3, 2, 0)
    assert fold(above, GSDR_MFMA_FOLD="1")[:3] == (3, 2, 1)
    assert fold(above, GSDR_MFMA_3M_ROT="1")[:3] == (3, 1, 0)
    assert fold(above, GSDR_MFMA_3M_ROT="1", GSDR_MFMA_FOLD="1")[:3] == (3, 1, 0)
    assert fold(above, GSDR_MFMA_3M="0", GSDR_MFMA_FOLD="1")[:3] == (4, 1, 0)
    # below the threshold: never by itself, forced where the handle rotates per pair
    assert fold(below)[2] == 0
    assert fold(below, GSDR_MFMA_FOLD="0")[2] == 0
    assert fold(256, GSDR_MFMA_3M="1")[:3] == (3, 1, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_FOLD="1")[:3] == (3, 1, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2")[:3] == (3, 2, 0)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="1")[:3] == (3, 2, 1)
    assert fold(256, GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="0")[:3] == (3, 2, 0)


HDR_FOLD_DECIMS = [750, 1000, 2000]        # windows of 94, 125, 250 blocks


def _fold_of(M):
    """describe()["fold"], ["fold_min_blocks"] of the handle _hdr_errors makes for decimation M under the environment as it is."""
    freq, _ = _HDR_REFS[(60, M)]
    dem = make_direct(freq, 200_000_000, M, 4, 200 * M)
    d = dem.describe()
    dem.close()
    return d["fold"], d["fold_min_blocks"]


def test_hdr_comb_fold_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """The measurement behind kFoldMinBlocks (csrc/demod.cpp): the 60 dB comb of test_gpu_mfma3.py (64 tones at
    200 Msps, F = 4, L = 200 * M, pre-converted operands forced), windows of 94, 125, 250 blocks, three buffers.
    Rule, per tone: err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) against the fp64 oracle on the same buffers.  Asserted for GSDR_MFMA_FOLD unset
    at every length; the figures of both loops forced (FOLD = 0, = 1) are recorded."""
    span_db = 60
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    monkeypatch.setenv("GSDR_MFMA_3M_ROT", "2")
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    failures = []
    for M in HDR_FOLD_DECIMS:
        res = {}
        for mode in ("0", "1", None):
            if mode is None:
                monkeypatch.delenv("GSDR_MFMA_FOLD", raising=False)
                monkeypatch.delenv("GSDR_MFMA_3M_ROT", raising=False)
            else:
                monkeypatch.setenv("GSDR_MFMA_FOLD", mode)
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
            assert res[mode][2] == 3, (M, mode)
            fold, T = _fold_of(M)            # the switch was heard
            assert fold == {"0": 0, "1": 1, None: int((4 * M + 31) // 32 >= T)}[mode], (M, mode, fold, T)
        monkeypatch.setenv("GSDR_MFMA_3M_ROT", "2")
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio = res["1"][0] / np.maximum(res["0"][0], 1e-12)
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound plain {worst['0']:.3f} folded {worst['1']:.3f} "
              f"default {worst[None]:.3f}; worst err plain {res['0'][0].max():.3e} folded {res['1'][0].max():.3e} "
              f"fp32 order {err32.max():.3e}; per-tone ratio folded/plain median {np.median(ratio):.2f} max {ratio.max():.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default")
        for m, name in (("0", "pair rotation, not folded"), ("1", "folded"), (None, "default")):
            record_info(float(res[m][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, {name}")
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(float(np.median(ratio)), f"{span_db} dB, M {M} ({nblk} blocks): median per-tone ratio folded / plain")
        record_info(float(ratio.max()), f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio folded / plain")
        if worst[None] > 1.0:
            failures.append((M, worst[None]))
    assert not failures, failures
