"""Three real products per complex multiply on the pre-converted matrix-core DDC
(ddc_convert3_kernel + ddc_mfma_ring16p3_kernel; switch GSDR_MFMA_3M).

Per-tone relative error against the fp64 oracle, bar 1e-5 as everywhere; every figure goes to the
margin file.  The cases, the comb and the helpers are those of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from _margins import record_info, record_margin
from test_gpu_parity import (DIRECT_CASES, TOL, crandn, hdr_comb, make_direct, make_pfb, rel_err_per_tone, run_device,
                             run_host)

pytestmark = pytest.mark.gpu

# DIRECT_CASES the matrix-core engine does not take (setup rules of csrc/demod.cpp: the zero padding
# behind a window must fit the next block, a buffer holds at least F-1 blocks): they run the generic
# VALU kernel under every GSDR_MFMA_* setting, today's mfma16p engine included
VALU_CASES = {(1, 1000, 10, 8, 1000, 5), (5, 1000, 50, 4, 100, 7), (4, 1_000_000, 7, 3, 7000, 3)}


@pytest.fixture
def forced3(monkeypatch):
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_MFMA_3M", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    monkeypatch.setenv("GSDR_TONES_FFT", "0")


def test_valu_cases_are_a_few():
    assert VALU_CASES <= set(DIRECT_CASES) and len(VALU_CASES) <= 3


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_direct_parity_three_products(cuda_device, gsdr_lib, oracle_mod, forced3, case):
    """(a) one row tile, a partial last tile, N no multiple of 32, windows of one block, M*F no
    multiple of 32, F from 1 to 8, consecutive buffers through both entries."""
    N, rate, M, F, L, nbuf = case
    rng = np.random.default_rng(1000 + N + M)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    if N >= 3:
        freq[0], freq[1], freq[2] = 0, rate // 2 - 1, -(rate // 2) + 1
    dem = make_direct(freq, rate, M, F, L)
    if case in VALU_CASES:
        assert not dem.kernel_name.startswith("ddc_mfma"), dem.kernel_name
        assert dem.describe()["complex_mac"] == 4
    else:
        assert dem.kernel_name == "ddc_mfma_ring16p_kernel", dem.kernel_name
        assert dem.describe()["complex_mac"] == 3
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"case {case} buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    if case not in VALU_CASES:
        assert dem.kernel_name == "ddc_mfma_ring16p_kernel" and dem.describe()["complex_mac"] == 3
    dem.close()


def test_tones_on_the_ddc_kernels_three_products(cuda_device, gsdr_lib, oracle_mod, forced3):
    """(a) TONES through the DDC kernels, buffer length no multiple of nfft (short last batches)."""
    N, rate, nfft, avg, L, nbuf = 5, 200_000_000, 1000, 4, 50_123, 4
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    assert dem.kernel_name == "ddc_mfma_ring16p_kernel", dem.kernel_name
    assert dem.describe()["complex_mac"] == 3
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
    assert dem.kernel_name == "ddc_mfma_ring16p_kernel"
    dem.close()


@pytest.mark.parametrize("kind", ["1e8", "1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (32, 200_000_000, 1000, 4, 200_000),
                                   (12, 9_000_000, 90, 4, 90_000)], ids=["M100", "M1000", "M90pad"])
def test_extreme_and_nonfinite_samples_three_products(cuda_device, gsdr_lib, oracle_mod, forced3, kind, shape):
    """(b) test_direct_extreme_and_nonfinite_samples of tests/test_gpu_parity.py, same three assertions:
    a NaN in b makes a+b NaN, so the rows that hold it are non-finite for every tone, as the oracle's."""
    N, rate, M, F, L = shape
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    assert dem.describe()["complex_mac"] == 3
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


C3 = (2048, 200_000_000, 1000, 4, 1_000_000)


def _c3_handle(M=1000):
    from gpu_sdr_amd.source import tone_comb
    N, rate, _, F, _ = C3
    freq, ampl, phase = tone_comb(N, rate, seed=20251004)
    return make_direct(freq, rate, M, F, M * 1000), (freq, ampl, phase)


def test_one_handle_is_bit_identical_through_every_entry(cuda_device, gsdr_lib, monkeypatch):
    """(c) A shape that is three-product by default (C3 itself): process_device on two caller streams,
    submit_device in between, the synchronous host entry -- bit-equal to one in-order stream."""
    import torch
    from gpu_sdr_amd.source import device_tones
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    monkeypatch.delenv("GSDR_MFMA_PREC", raising=False)
    N, rate, M, F, L = C3
    a, (freq, ampl, phase) = _c3_handle()
    b, _ = _c3_handle()
    for d in (a, b):
        assert d.describe()["complex_mac"] == 3 and d.kernel_name == "ddc_mfma_ring16p_kernel"
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
        assert a.kernel_name == "ddc_mfma_ring16p_kernel" and a.describe()["complex_mac"] == 3
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
        assert b.kernel_name == "ddc_mfma_ring16p_kernel" and b.describe()["complex_mac"] == 3, (k, how)
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
    """(d) GSDR_MFMA_3M=0 gives the four-product kernels of before (ring16w8 in order, ring16p overlapped on
    C3); a window one block shorter than the threshold stays on four products by default."""
    import torch
    monkeypatch.delenv("GSDR_MFMA_PREC", raising=False)
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    N, rate, M, F, L = C3
    d, _ = _c3_handle()
    T = d.describe()["complex_mac_min_blocks"]
    d.close()
    monkeypatch.setenv("GSDR_MFMA_3M", "0")
    d, _ = _c3_handle()
    assert d.describe()["complex_mac"] == 4
    x = torch.from_numpy(crandn(np.random.default_rng(5), L)).to(cuda_device)
    out = torch.empty(d.out_capacity, dtype=torch.complex64, device=cuda_device)
    d.process_device(x, out)
    torch.cuda.synchronize()
    assert d.kernel_name == "ddc_mfma_ring16w8_kernel", d.kernel_name
    d.submit_device(x, out)
    d.wait()
    torch.cuda.synchronize()
    assert d.kernel_name == "ddc_mfma_ring16p_kernel" and d.describe()["complex_mac"] == 4
    d.close()
    monkeypatch.delenv("GSDR_MFMA_3M")
    if T * 32 % F == 0 and T > 1:
        M1 = (T - 1) * 32 // F               # a window of T-1 whole blocks
        d, _ = _c3_handle(M=M1)
        assert d.describe()["complex_mac"] == 4, (T, M1)
        d.close()
        d, _ = _c3_handle(M=T * 32 // F)
        assert d.describe()["complex_mac"] == 3, T
        d.close()


HDR_DECIMS = [256, 375, 500, 750, 1000, 2000]       # windows of 32, 47, 63, 94, 125, 250 blocks


_HDR_REFS = {}


def _hdr_refs(oracle_mod, span_db, M):
    """The comb, its three buffers, the fp64 oracle's outputs and those of the reference's fp32 order
    (computed once per comb and length: they do not depend on the library's switches)."""
    from oracle import recipe_b
    key = (span_db, M)
    if key not in _HDR_REFS:
        N, rate, F = 64, 200_000_000, 4
        L = 200 * M
        rng = np.random.default_rng(4242 + span_db)
        freq, ampl, phase, make = hdr_comb(N, rate, L, span_db, rng, 0)
        ref = oracle_mod.Direct(freq, rate, M, F, L)
        ref32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64)     # the reference's fp32 order
        bufs = []
        for c in range(3):
            x = make(c, 50 + c)
            bufs.append((x, ref.process(x), ref32.process(x)))
        _HDR_REFS[key] = (freq, bufs)
    return _HDR_REFS[key]


def _hdr_errors(cuda_device, oracle_mod, span_db, M):
    """Per-tone errors of the library (under the environment as it is) and of the reference's fp32 order,
    three buffers; returns (err[3][N], err32[3][N], complex_mac)."""
    N, rate, F = 64, 200_000_000, 4
    freq, bufs = _hdr_refs(oracle_mod, span_db, M)
    dem = make_direct(freq, rate, M, F, 200 * M)
    mac = dem.describe()["complex_mac"]
    errs, errs32 = [], []
    for x, yr, y32 in bufs:
        y = run_device(dem, x, cuda_device).reshape(-1, N)
        assert y.shape == yr.shape == y32.shape
        den = np.linalg.norm(yr[F:].astype(np.complex128), axis=0)
        errs.append(np.linalg.norm(y[F:].astype(np.complex128) - yr[F:], axis=0) / den)
        errs32.append(np.linalg.norm(y32[F:].astype(np.complex128) - yr[F:], axis=0) / den)
    dem.close()
    return np.array(errs), np.array(errs32), mac


@pytest.mark.parametrize("span_db", [60, 40])
def test_hdr_comb_sets_threshold(cuda_device, gsdr_lib, oracle_mod, monkeypatch, span_db):
    """(e) The measurement behind kMac3MinBlocks (csrc/demod.cpp).  64 tones spanning 40 / 60 dB at
    200 Msps, F = 4, L = 200 * M, windows of 32 ... 250 blocks, pre-converted operands forced.  Rule, per tone:
    err <= max(1e-5, 3 x err32), err32 the error of the reference's own fp32 order of operations
    (oracle/recipe_b.py, complex64) on the same buffers -- the rule of test_direct_high_dynamic_range_comb.
    Asserted for GSDR_MFMA_3M unset at every length; the forced figures (3M = 1, = 0) are recorded.
    A length at which the FOUR-product arithmetic itself misses the rule is recorded and left out (one at most)."""
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", "4")
    monkeypatch.setenv("GSDR_MFMA_PREC", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    failures, left_out, T = [], [], None
    for M in HDR_DECIMS:
        res = {}
        for mode in ("1", "0", None):
            if mode is None:
                monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
            else:
                monkeypatch.setenv("GSDR_MFMA_3M", mode)
            res[mode] = _hdr_errors(cuda_device, oracle_mod, span_db, M)
        assert res["1"][2] == 3 and res["0"][2] == 4
        err32 = res[None][1]
        bound = np.maximum(TOL, 3.0 * err32)
        nblk = (4 * M + 31) // 32
        worst = {m: float((res[m][0] / bound).max()) for m in res}
        ratio34 = float((res["1"][0] / np.maximum(res["0"][0], 1e-12)).max())
        _HDR_REFS.pop((span_db, M), None)
        print(f"hdr {span_db} dB M {M} ({nblk} blocks): err/bound three {worst['1']:.3f} four {worst['0']:.3f} "
              f"default {worst[None]:.3f} (complex_mac {res[None][2]}); worst err three {res['1'][0].max():.3e} "
              f"four {res['0'][0].max():.3e} fp32 order {err32.max():.3e}; per-tone ratio three/four up to {ratio34:.2f}")
        record_margin(float(res[None][0][:, :32].max()), f"{span_db} dB, M {M}: strong half, default arithmetic")
        record_info(float(res["1"][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, three products")
        record_info(float(res["0"][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, four products")
        record_info(float(res[None][0].max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error, default (complex_mac {res[None][2]})")
        record_info(float(err32.max()), f"{span_db} dB, M {M} ({nblk} blocks): worst per-tone error of the reference's fp32 order")
        for m, name in (("1", "three products"), ("0", "four products"), (None, "default")):
            record_info(worst[m], f"{span_db} dB, M {M} ({nblk} blocks): worst err / bound, {name}")
        record_info(ratio34, f"{span_db} dB, M {M} ({nblk} blocks): largest per-tone ratio three / four products")
        if worst["0"] > 1.0:
            left_out.append((M, worst["0"]))
            continue
        if worst[None] > 1.0:
            failures.append((M, res[None][2], worst[None]))
        if M in (1000, 2000):
            T = T if T is not None else _threshold(monkeypatch)
            if T <= 125:
                assert res[None][2] == 3, (M, T)
    assert len(left_out) <= 1, left_out
    assert not failures, failures


def _threshold(monkeypatch):
    from gpu_sdr_amd.source import tone_comb
    freq, _, _ = tone_comb(64, 200_000_000, seed=1)
    d = make_direct(freq, 200_000_000, 1000, 4, 200_000)
    T = d.describe()["complex_mac_min_blocks"]
    d.close()
    return T


def test_c3_full_size_margin(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """C3 against the oracle through the default arithmetic of its handle (three products when the threshold
    allows): the margin to record beside the 3.3e-7 of the four-product loop."""
    from test_gpu_parity import _full_size_direct
    monkeypatch.delenv("GSDR_MFMA_3M", raising=False)
    _full_size_direct(cuda_device, oracle_mod, N=2048, M=1000, nbuf=3, subset=12)
