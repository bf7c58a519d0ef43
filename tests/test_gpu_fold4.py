"""The direct folded matrix-core DDC (ddc_convert4f_kernel + ddc_mfma_ring16p4f_kernel, DESIGN.md section 4.1g;
switch GSDR_MFMA_FOLD_PRODUCTS): the plain four products of each 64-sample span folded over 32 partner pairs and
summed straight into Re and Im.

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the margin file.  The
cases, the comb and the helpers are those of tests/test_gpu_parity.py, test_gpu_mfma3.py, test_gpu_fold.py and
test_gpu_extents.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from test_gpu_parity import TOL, crandn, make_direct, make_pfb, rel_err_per_tone, run_device, run_host
from test_gpu_mfma3 import _hdr_errors, _HDR_REFS
from test_gpu_extents import S_N65, S_ODD, clean_env, direct_inputs, expect_kernel, run_case
from test_gpu_fold import FOLD_ENV, KERNEL

pytestmark = pytest.mark.gpu

FOLD4_ENV = dict(FOLD_ENV, GSDR_MFMA_FOLD_PRODUCTS="4")


@pytest.fixture
def forced_fold4(monkeypatch):
    for k, v in FOLD4_ENV.items():
        monkeypatch.setenv(k, v)


def _is_fold4(dem):
    d = dem.describe()
    return (dem.kernel_name == KERNEL and (d["complex_mac"], d["rotation_blocks"], d["fold"]) == (3, 2, 1)
            and d["fold_products"] == 4)


@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5])
def test_shortest_windows_fold4(cuda_device, gsdr_lib, oracle_mod, forced_fold4, blocks):
    """Windows of one to five blocks: a half-empty last span (1, 3, 5) or a whole one, with no, one and two whole
    spans in front; both exits of the trip."""
    N, rate, F = 40, 1_000_000, 4
    M = 8 * blocks                      # M * F = 32 * blocks
    L = 64 * M
    rng = np.random.default_rng(31 + blocks)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold4(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"{blocks} blocks buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    assert _is_fold4(dem)
    dem.close()


def test_window_no_multiple_of_32_or_64_fold4(cuda_device, gsdr_lib, oracle_mod, forced_fold4):
    """M = 90, F = 4: M * F = 360 is a multiple of neither 32 nor 64 (12 blocks, the last one 8 samples long)."""
    N, rate, M, F, L = 12, 9_000_000, 90, 4, 90_000
    rng = np.random.default_rng(90)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold4(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(3):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        err = rel_err_per_tone(y.reshape(-1, N), ref.process(x))
        print(f"M 90 buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    dem.close()


@pytest.mark.parametrize("shape", [S_N65, S_ODD], ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_direct_extents_fold4(cuda_device, gsdr_lib, oracle_mod, monkeypatch, shape):
    """The guard zones of tests/_extents.py around input and output (both patterns, both offsets of each), through
    process_device and submit_device: 65 tones and a last row tile of 4 rows over 12.5 blocks (a half-empty last span);
    an odd row stride with F = 5 (185 samples: three spans, the last one short)."""
    N, rate, M, F, L = shape
    clean_env(monkeypatch, FOLD4_ENV)
    freq, xs, yrs = direct_inputs(shape, oracle_mod)

    def expect(dem, ran):
        expect_kernel(KERNEL, 3, 2)(dem, ran)
        d = dem.describe()
        assert (d["fold"], d["fold_products"]) == (1, 4)

    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), expect, xs, yrs, N)


def test_one_handle_every_entry_fold4(cuda_device, gsdr_lib, forced_fold4):
    """One handle, one loop: process_device, submit_device / wait and the host entry give the same bits for the same
    buffers (32 tones, M 1000, F 4, L 200 000: 125 blocks, 200 rows)."""
    import torch
    from gpu_sdr_amd.source import tone_comb
    N, rate, M, F, L = 32, 200_000_000, 1000, 4, 200_000
    freq, _, _ = tone_comb(N, rate, seed=44)
    rng = np.random.default_rng(444)
    xs = [crandn(rng, L) for _ in range(3)]
    got = {}
    for entry in ("process", "submit", "host"):
        dem = make_direct(freq, rate, M, F, L)
        assert _is_fold4(dem), (dem.kernel_name, dem.describe())
        ys = []
        for x in xs:
            if entry == "host":
                ys.append(run_host(dem, x))
                continue
            xin = torch.from_numpy(x).to(cuda_device)
            out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
            if entry == "process":
                n = dem.process_device(xin, out)
            else:
                dem.submit_device(xin, out)
                n = dem.wait()
            torch.cuda.synchronize()
            ys.append(out[:n].cpu().numpy())
        assert _is_fold4(dem), entry
        dem.close()
        got[entry] = ys
    for entry in ("submit", "host"):
        for k, (y, w) in enumerate(zip(got[entry], got["process"])):
            assert y.size == w.size == N * (L // M), (entry, k)
            np.testing.assert_array_equal(y.view(np.int32), w.view(np.int32), err_msg=f"buffer {k} via {entry}")


@pytest.mark.parametrize("kind", ["1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (12, 9_000_000, 90, 4, 90_000)], ids=["M100", "M90pad"])
def test_extreme_and_nonfinite_samples_fold4(cuda_device, gsdr_lib, oracle_mod, forced_fold4, kind, shape):
    """test_extreme_and_nonfinite_samples_fold of tests/test_gpu_fold.py, same three assertions."""
    N, rate, M, F, L = shape
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    assert _is_fold4(dem), (dem.kernel_name, dem.describe())
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    at = (L // M // 2) * M + 3
    rows = np.arange(L // M)
    hit = (rows >= at // M) & (rows <= at // M + F - 1)
    far = near = 0.0
    for c in range(4):
        x = host_tones(L, c * L, rate, freq, ampl, phase, sigma=1e-3, seed=700 + c)
        if c == 1:
            rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
            x[at] = {"1e10": np.complex64(1e10 * rms * (0.6 - 0.8j)), "inf": np.complex64(complex(np.inf, 0.5)),
                     "nan": np.complex64(complex(0.25, np.nan))}[kind]
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


def test_tones_on_the_ddc_kernels_fold4(cuda_device, gsdr_lib, oracle_mod, forced_fold4):
    """TONES through the DDC kernels, buffer length no multiple of nfft (short last batches)."""
    N, rate, nfft, avg, L, nbuf = 5, 200_000_000, 1000, 4, 50_123, 4
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    assert _is_fold4(dem), (dem.kernel_name, dem.describe())
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
    assert _is_fold4(dem)
    dem.close()


def test_switch_fold_products(cuda_device, gsdr_lib, monkeypatch):
    """GSDR_MFMA_FOLD_PRODUCTS: 3 the Gauss fold, 4 the direct fold, on every folded handle; a handle that is not
    folded (GSDR_MFMA_FOLD=0, a rotation per block, four products per block, a window below fold_min_blocks) reports
    0, and complex_mac, rotation_blocks and fold are what they were."""
    from gpu_sdr_amd.source import tone_comb
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_PREC", "GSDR_MFMA_FOLD", "GSDR_MFMA_FOLD_PRODUCTS"):
        monkeypatch.delenv(k, raising=False)
    rate, F = 200_000_000, 4
    freq, _, _ = tone_comb(64, rate, seed=1)

    def info(M, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = make_direct(freq, rate, M, F, 200 * M)
        i = d.describe()
        d.close()
        for k in env:
            monkeypatch.delenv(k)
        return i["complex_mac"], i["rotation_blocks"], i["fold"], i["fold_products"], i["fold_min_blocks"]

    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    T = info(1000)[4]
    assert T == 94
    above, below = T * 8, (T - 1) * 8                     # windows of exactly T and of T - 1 blocks
    default = info(above)
    assert default[:3] == (3, 2, 1) and default[3] in (3, 4)
    record_info(default[3], "fold_products of a folded handle by default")
    assert info(above, GSDR_MFMA_FOLD_PRODUCTS="3")[:4] == (3, 2, 1, 3)
    assert info(above, GSDR_MFMA_FOLD_PRODUCTS="4")[:4] == (3, 2, 1, 4)
    for p in ("3", "4"):
        assert info(above, GSDR_MFMA_FOLD="0", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (3, 2, 0, 0)
        assert info(above, GSDR_MFMA_3M_ROT="1", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (3, 1, 0, 0)
        assert info(above, GSDR_MFMA_3M="0", GSDR_MFMA_FOLD_PRODUCTS=p)[:4] == (4, 1, 0, 0)
        assert info(below, GSDR_MFMA_FOLD_PRODUCTS=p)[2:4] == (0, 0)
    assert info(below)[2:4] == (0, 0)
    # forced below the threshold: the switch is heard there too
    forced = dict(GSDR_MFMA_3M="1", GSDR_MFMA_3M_ROT="2", GSDR_MFMA_FOLD="1")
    assert info(256, **forced, GSDR_MFMA_FOLD_PRODUCTS="4")[:4] == (3, 2, 1, 4)
    assert info(256, **forced, GSDR_MFMA_FOLD_PRODUCTS="3")[:4] == (3, 2, 1, 3)


HDR_ASSERTED = [750, 1000, 2000]           # windows of 94, 125, 250 blocks: the rule is asserted
HDR_RECORDED = [256, 375, 500]             # 32, 47, 63 blocks, the fold forced: recorded only


def _products_of(M):
    freq, _ = _HDR_REFS[(60, M)]
    dem = make_direct(freq, 200_000_000, M, 4, 200 * M)
    d = dem.describe()
    dem.close()
    return d["fold"], d["fold_products"]


@pytest.mark.parametrize("M", HDR_ASSERTED + HDR_RECORDED)
def test_hdr_comb_fold4_keeps_the_rule(cuda_device, gsdr_lib, oracle_mod, monkeypatch, M):
    """The 60 dB comb of test_gpu_mfma3.py (64 tones at 200 Msps, F = 4, L = 200 * M, pre-converted operands forced),
    three buffers.  Rule of DESIGN.md section 4.1d, per tone: err <= max(1e-5, 3 x err32), err32 the error of the
    reference's own fp32 order of operations against the fp64 oracle on the same buffers.  Asserted at 94, 125 and 250
    blocks for GSDR_MFMA_FOLD_PRODUCTS unset and = 4; the Gauss fold's figures (= 3) and the per-tone ratio 4 / 3 are
    recorded, and so are 32, 47 and 63 blocks with the fold forced (what a later change of the thresholds would rest
    on; nothing is asserted of them)."""
    span_db = 60
    asserted = M in HDR_ASSERTED
    nblk = (4 * M + 31) // 32
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    for k in ("GSDR_MFMA_3M", "GSDR_MFMA_3M_ROT", "GSDR_MFMA_FOLD", "GSDR_MFMA_FOLD_PRODUCTS"):
        monkeypatch.delenv(k, raising=False)
    if not asserted:
        monkeypatch.setenv("GSDR_MFMA_3M", "1")
        monkeypatch.setenv("GSDR_MFMA_3M_ROT", "2")
        monkeypatch.setenv("GSDR_MFMA_FOLD", "1")
    res = {}
    for mode in (("3", "4", None) if asserted else ("3", "4")):
        if mode is None:
            monkeypatch.delenv("GSDR_MFMA_FOLD_PRODUCTS", raising=False)
        else:
            monkeypatch.setenv("GSDR_MFMA_FOLD_PRODUCTS", mode)
        res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
        assert res[mode][2] == 3, (M, mode)
        fold, products = _products_of(M)           # the switch was heard
        assert fold == 1 and (products == int(mode) if mode else products in (3, 4)), (M, mode, fold, products)
    err32 = res["4"][1]
    bound = np.maximum(TOL, 3.0 * err32)
    worst = {m: float((res[m][0] / bound).max()) for m in res}
    ratio = res["4"][0] / np.maximum(res["3"][0], 1e-12)
    _HDR_REFS.pop((span_db, M), None)
    print(f"hdr {span_db} dB M {M} ({nblk} blocks, {'asserted' if asserted else 'recorded'}): err/bound "
          + " ".join(f"{m or 'default'} {worst[m]:.3f}" for m in res)
          + f"; worst err 3: {res['3'][0].max():.3e} 4: {res['4'][0].max():.3e} fp32 order {err32.max():.3e}; "
          f"per-tone ratio 4/3 median {np.median(ratio):.2f} max {ratio.max():.2f}")
    if asserted:
        record_margin(float(res["4"][0][:, :32].max()), "strong half, direct fold")
    for m in res:
        name = {"3": "Gauss fold", "4": "direct fold", None: "default"}[m]
        record_info(float(res[m][0].max()), f"{nblk} blocks: worst per-tone error, {name}")
        record_info(worst[m], f"{nblk} blocks: worst err / bound, {name}")
    record_info(float(np.median(ratio)), f"{nblk} blocks: median per-tone ratio direct / Gauss")
    record_info(float(ratio.max()), f"{nblk} blocks: largest per-tone ratio direct / Gauss")
    if asserted:
        failures = [(M, m, worst[m]) for m in ("4", None) if worst[m] > 1.0]
        assert not failures, failures
