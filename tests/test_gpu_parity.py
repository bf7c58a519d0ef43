"""GPU parity tests: the HIP path, called through the C ABI (libgsdr.so), against
the CPU oracle on the same seeded inputs, against the frozen fixtures in
tests/golden/, and -- at BASELINE.json's full sizes -- against the oracle on a
subset of tones plus size-independent properties.

Bar (north_star): per tone ||y - y_ref||_2 / ||y_ref||_2 <= 1e-5 (float32), and
exact equality of every returned length.
"""
import json
import os

import numpy as np
import pytest

import _pfb
from _margins import record_info, record_margin

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def rel_err_per_tone(y, yr, label=None):
    """Per-tone relative l2 error.  Every call also feeds the margin record (tests/conftest.py
    writes it at the end of the session): worst value per (test id incl. engine)."""
    y = np.asarray(y, dtype=np.complex128)
    yr = np.asarray(yr, dtype=np.complex128)
    num = np.linalg.norm(y - yr, axis=0)
    den = np.linalg.norm(yr, axis=0)
    err = num / np.where(den == 0, 1.0, den)
    record_margin(float(np.max(err)) if np.size(err) else 0.0, label)
    return err


def run_host(dem, x):
    """host-pointer entry (gsdr_demod_process), synchronous like the reference"""
    out = np.empty(dem.out_capacity, dtype=np.complex64)
    n = dem.process(np.ascontiguousarray(x), out)
    return out[:n].copy()


def run_device(dem, x, dev):
    """device-pointer entry (gsdr_demod_process_device) on the current torch stream"""
    import torch
    xin = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=dev)
    n = dem.process(xin, out)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy()


def make_direct(freq, rate, decim, f, L):
    import gpu_sdr_amd as g
    p = g.param(mode="RX", rate=rate, buffer_len=L, decim=decim, pf_average=f,
                freq=[int(v) for v in freq], wave_type=[g.w_type.DIRECT] * len(freq))
    return g.RX_buffer_demodulator(p, device_index=0)


def make_pfb(freq, rate, nfft, avg, L):
    import gpu_sdr_amd as g
    p = g.param(mode="RX", rate=rate, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                freq=[int(v) for v in freq], wave_type=[g.w_type.TONES] * len(freq))
    return g.RX_buffer_demodulator(p, device_index=0)


def make_chirp(rate, f0, f1, steps, t, decim, L):
    import gpu_sdr_amd as g
    p = g.param(mode="RX", rate=rate, buffer_len=L, decim=decim, freq=[f0], chirp_f=[f1],
                swipe_s=[steps], chirp_t=[t], wave_type=[g.w_type.CHIRP])
    return g.RX_buffer_demodulator(p, device_index=0)


@pytest.fixture(params=["default", "flat", "mfma", "mfma_rt2", "mfma16", "mfma16w8", "mfma16p"])
def engine(request, monkeypatch):
    """Runs a test once per engine: "default" = the library as shipped, no variable set (per-launch
    kernel choice for the DDC; TONES through the filter + in-LDS FFT kernel); then the DDC engines,
    forced, with TONES on the DDC kernels too (every selected bin as a tone, GSDR_TONES_FFT=0):
    packed-FP32 VALU kernel; round 1's matrix-core kernel (32x32x16 MFMA; one / two row tiles per
    workgroup); the 16x16x32 ring loop, its eight-wave build and its pre-converted-operand build."""
    if request.param == "default":
        for k in [k for k in os.environ if k.startswith("GSDR_")]:
            monkeypatch.delenv(k)
        return request.param
    monkeypatch.setenv("GSDR_TONES_FFT", "0")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")          # (the forced engine, also where ddc_few_kernel would take the shape)
    monkeypatch.setenv("GSDR_DDC_MFMA", "0" if request.param == "flat" else "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", {"mfma16": "4", "mfma16w8": "5", "mfma16p": "4"}.get(request.param, "2"))
    monkeypatch.setenv("GSDR_MFMA_PREC", "1" if request.param == "mfma16p" else "0")
    monkeypatch.setenv("GSDR_MFMA_RT", "2" if request.param == "mfma_rt2" else "0")
    return request.param


@pytest.fixture(params=["staged", "x16", "x16w8", "x16p"])
def mfma_engine(request, monkeypatch):
    """Matrix-core DDC: round 1's loop on the 32x32x16 MFMA / the ring loop on the 16x16x32 shape /
    its eight-wave build / its pre-converted-operand build."""
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_DDC_FEW", "0")
    monkeypatch.setenv("GSDR_TONES_FFT", "0")
    monkeypatch.setenv("GSDR_MFMA_ASM", {"x16": "4", "x16w8": "5", "x16p": "4"}.get(request.param, "2"))
    monkeypatch.setenv("GSDR_MFMA_PREC", "1" if request.param == "x16p" else "0")
    return request.param


# ---------------------------------------------------------------------------
# frozen fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["direct", "pfb", "chirp", "noise"])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_golden_fixture(cuda_device, gsdr_lib, name, entry, engine):
    g = np.load(os.path.join(HERE, "golden", f"{name}.npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    L = cfg["buffer_len"]
    if name == "direct":
        dem = make_direct(cfg["freq"], cfg["rate"], cfg["decim"], cfg["pf_average"], L)
        nch = len(cfg["freq"])
    elif name == "pfb":
        dem = make_pfb(cfg["freq"], cfg["rate"], cfg["fft_tones"], cfg["pf_average"], L)
        nch = len(cfg["freq"])
    elif name == "noise":
        import gpu_sdr_amd as g_
        dem = g_.RX_buffer_demodulator(g_.param(mode="RX", rate=1200, buffer_len=L, decim=0, pf_average=cfg["pf_average"],
                                                fft_tones=cfg["fft_tones"], freq=[0], wave_type=[g_.w_type.NOISE]),
                                       device_index=0)
        nch = cfg["fft_tones"]
    else:
        dem = make_chirp(cfg["rate"], cfg["freq"], cfg["chirp_f"], cfg["swipe_s"], cfg["chirp_t"], cfg["decim"], L)
        nch = 1
    x = g["x"]
    outs = []
    for c in range(len(x) // L):
        xb = x[c * L:(c + 1) * L]
        outs.append(run_host(dem, xb) if entry == "host" else run_device(dem, xb, cuda_device))
    dem.close()
    assert [len(o) for o in outs] == list(g["lengths"])
    y = np.concatenate(outs).reshape(-1, nch)
    yr = g["y"].reshape(-1, nch)
    assert rel_err_per_tone(y, yr).max() <= TOL


# ---------------------------------------------------------------------------
# DIRECT (DDC)
# ---------------------------------------------------------------------------
DIRECT_CASES = [
    # N, rate, M, F, L, buffers
    (3, 1_000_000, 50, 4, 50_000, 4),        # survey probe shape, MIN_USEFULL_BUFFER
    (8, 1_000_000, 100, 1, 50_000, 3),       # single tap phase: no carry
    (1, 1000, 10, 8, 1000, 5),               # NCO index wraps every buffer, F = 8
    (65, 10_000_000, 100, 4, 10_000, 3),     # 2 tone waves, one almost empty; M % 16 = 4
    (5, 1000, 50, 4, 100, 7),                # fewer blocks (2) than F-1: carry outlives a buffer
    (7, 200_000_000, 1000, 4, 50_000, 3),    # C3 block shape
    (16, 100_000_000, 100, 4, 100_000, 3),   # C1 shape (16 tones @ 100 Msps, decim 100)
    (4, 1_000_000, 16, 2, 4096, 3),          # M == K, no remainder
    (4, 1_000_000, 7, 3, 7000, 3),           # M < K: remainder path only
    (6, 1_000_000, 37, 5, 37_000, 2),        # odd everything
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
@pytest.mark.parametrize("impl", ["flat", "flat12", "flat16", "flat20", "flat40", "simple16", "simple32",
                                  "mfma", "mfma_rt2", "mfma16", "mfma16_rt2", "mfma16w8", "mfma16p", "mfma_c", "mfma_t2",
                                  "mfma_w2", "mfma_pk16"])
def test_direct_parity(cuda_device, gsdr_lib, oracle_mod, monkeypatch, case, impl):
    """flat* = ddc_flat_kernel (packed FP32; sub-block length auto / forced),
    simple* = ddc_kernel (generic fallback, phasor table 16 / 32),
    mfma = ddc_mfma_ring_kernel (split-fp16 matrix cores, assembly main loop, operand
    shared through an LDS ring: the production kernel),
    mfma_rt2 = the same kernel with two row tiles per workgroup (GSDR_MFMA_RT=2: the second tile
    keeps the phasor images),
    mfma16 = ddc_mfma_ring16_kernel (the same ring loop on v_mfma_f32_16x16x32_f16: 2 x 2 tiles of
    16 x 16 per wave, 48 MFMAs per block; _rt2: two row tiles per workgroup),
    mfma16w8 = ddc_mfma_ring16w8_kernel (that loop for workgroups of eight waves: 32 rows x 256 tones, the
    waves of a SIMD barrier-coupled partners, conversion shared by eight waves),
    mfma16p = ddc_convert_kernel + ddc_mfma_ring16p_kernel (the operand converted once per buffer, the loop
    copies 8-KiB images into its ring by LDS-DMA: the path of launches of many rounds, forced here),
    mfma_c* = ddc_mfma_kernel (same algorithm, compiler-scheduled; tone tiles per wave 1/2,
    waves per workgroup 4/2, phasor block 32/16)."""
    N, rate, M, F, L, nbuf = case
    if impl.startswith("mfma"):
        monkeypatch.setenv("GSDR_DDC_MFMA", "1")
        if impl == "mfma":
            monkeypatch.setenv("GSDR_MFMA_ASM", "2")
        if impl == "mfma_rt2":
            monkeypatch.setenv("GSDR_MFMA_ASM", "2")
            monkeypatch.setenv("GSDR_MFMA_RT", "2")
        if impl.startswith("mfma16"):
            monkeypatch.setenv("GSDR_MFMA_ASM", "5" if impl == "mfma16w8" else "4")
            monkeypatch.setenv("GSDR_MFMA_PREC", "1" if impl == "mfma16p" else "0")
            if impl == "mfma16_rt2":
                monkeypatch.setenv("GSDR_MFMA_RT", "2")
        if impl in ("mfma_c", "mfma_t2", "mfma_w2", "mfma_pk16"):
            monkeypatch.setenv("GSDR_MFMA_ASM", "0")
        if "_t" in impl:
            monkeypatch.setenv("GSDR_MFMA_TT", impl[-1])
        if "_w" in impl:
            monkeypatch.setenv("GSDR_MFMA_W", impl[-1])
        if "_pk" in impl:
            monkeypatch.setenv("GSDR_MFMA_PK", impl[-2:])
    else:
        monkeypatch.setenv("GSDR_DDC_MFMA", "0")
        monkeypatch.setenv("GSDR_DDC_PIPE", "1" if impl.startswith("flat") else "0")
        monkeypatch.setenv("GSDR_DDC_K", impl.lstrip("flatsimple") or "0")
    rng = np.random.default_rng(1000 + N + M)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    if N >= 3:
        freq[0], freq[1], freq[2] = 0, rate // 2 - 1, -(rate // 2) + 1
    dem = make_direct(freq, rate, M, F, L)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    np.testing.assert_array_equal(dem.window(), ref.taps())
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        assert err.max() <= TOL, (c, err.max())
    dem.close()


def test_direct_fuzz_random_shapes(cuda_device, gsdr_lib, oracle_mod, engine):
    """Seeded fuzz over (tones, decim, pf_average, buffer_len, rate): shapes nobody
    picked by hand -- prime decimations, single tones, 1-block buffers, F = 5..8
    (generic kernel), tone counts around the 64-lane boundaries."""
    rng = np.random.default_rng(777)
    for it in range(40):
        F = int(rng.integers(1, 9))
        M = int(rng.choice([1, 2, 3, 5, 7, 11, 16, 20, 25, 33, 64, 100, 127, 250]))
        nb = int(rng.integers(1, 40))
        L = M * nb
        rate = int(rng.choice([1000, 65536, 1_000_000, 200_000_000]))
        N = int(rng.choice([1, 2, 5, 63, 64, 65, 130]))
        freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        dem = make_direct(freq, rate, M, F, L)
        ref = oracle_mod.Direct(freq, rate, M, F, L)
        for c in range(3):
            x = crandn(rng, L)
            y = run_device(dem, x, cuda_device)
            yr = ref.process(x)
            assert y.size == yr.size, (it, N, M, F, L)
            err = rel_err_per_tone(y.reshape(-1, N), yr)
            assert err.max() <= TOL, (it, N, M, F, L, rate, c, err.max())
        dem.close()


def test_pfb_and_chirp_fuzz_random_shapes(cuda_device, gsdr_lib, oracle_mod, engine):
    rng = np.random.default_rng(778)
    for it in range(25):
        nfft = int(rng.choice([2, 3, 8, 10, 17, 50, 64, 100, 333, 1000]))
        avg = int(rng.integers(1, 9))
        L = int(rng.integers(max(4, nfft), 6 * nfft * avg + 200))
        rate = int(rng.choice([1000, 1_000_000, 200_000_000]))
        N = int(rng.choice([1, 3, 64, 65]))
        freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        dem = make_pfb(freq, rate, nfft, avg, L)
        ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
        np.testing.assert_array_equal(dem.bins(), ref.bins())
        for c in range(4):
            x = crandn(rng, L)
            y = run_device(dem, x, cuda_device)
            yr = ref.process(x)
            assert y.size == yr.size, (it, N, nfft, avg, L, c)
            if yr.size:
                bins = ref.bins()
                ok = bins >= 0          # unmatched tones read bin 0 here, garbage in the reference
                err = rel_err_per_tone(y.reshape(-1, N)[:, ok], yr[:, ok])
                assert err.size == 0 or err.max() <= TOL, (it, N, nfft, avg, L, c, err.max())
        dem.close()
    for it in range(25):
        rate = int(rng.choice([1_000_000, 200_000_000]))
        steps = int(rng.choice([1, 2, 3, 10, 100, 1000]))
        length = int(rng.choice([1, 2, 7, 64, 65, 300]))
        decim = int(rng.choice([0, 1, 2, 5]))
        L = int(rng.integers(max(1, length * max(decim, 1)), 20 * length * max(decim, 1) + 500))
        f0, f1 = (int(v) for v in rng.integers(-rate // 2 + 1, rate // 2, size=2))
        t = float(np.float32(steps * length / rate))
        ocp = oracle_mod.chirp_params(rate, f0, f1, steps, t)
        if ocp.length * max(decim, 1) > L or ocp.length < 1:
            continue
        dem = make_chirp(rate, f0, f1, steps, t, decim, L)
        ref = oracle_mod.Chirp(rate, f0, f1, steps, t, decim, L)
        for c in range(4):
            x = crandn(rng, L)
            y = run_device(dem, x, cuda_device)
            yr = ref.process(x)
            assert y.size == yr.size, (it, steps, length, decim, L, c)
            if yr.size:
                assert rel_err_per_tone(y[:, None], yr[:, None]).max() <= TOL, (it, steps, length, decim, L, c)
        dem.close()


def _is_mfma(dem, ran):
    assert ran or dem.kernel_name.startswith("ddc_mfma"), dem.kernel_name


def _any_engine(dem, ran):
    pass


def test_mfma_dynamic_range_and_scale_carry(cuda_device, gsdr_lib, oracle_mod, mfma_engine):
    """The matrix-core DDC scales every buffer into fp16 range from its own maximum (and
    the previous buffer's, whose tail it still reads).  Same tolerance for inputs of
    1e-6, 1 and 3e4, for a loud buffer followed by a quiet one and vice versa, and an
    all-zero buffer gives exact zeros.  (The body, as those of the tests below that name _product_loops, is shared
    with tests/test_gpu_product_loops.py, which runs it on every product loop.)"""
    from _product_loops import dynamic_range_and_scale_carry
    dynamic_range_and_scale_carry(cuda_device, oracle_mod, _is_mfma)


@pytest.mark.parametrize("F", [5, 6, 7, 8])
def test_mfma_more_tap_phases(cuda_device, gsdr_lib, oracle_mod, mfma_engine, F):
    """pf_average 5..8: the packed-FP32 production kernel stops at 4, the matrix-core DDC
    takes any window that is made of whole blocks behind its last sample."""
    from _product_loops import more_tap_phases
    more_tap_phases(cuda_device, oracle_mod, _is_mfma, F, M=64, alternate=False)


def test_mfma_two_handles_interleaved(cuda_device, gsdr_lib, oracle_mod, mfma_engine):
    """Two matrix-core demodulators fed alternately on one stream (the server's two RX front
    ends): carry, scale slots and head/tail copies are per handle."""
    from _product_loops import two_handles_interleaved
    two_handles_interleaved(cuda_device, oracle_mod, lambda k, *shape: make_direct(*shape), lambda k, dem, ran: None)


def hdr_comb(N, rate, L, span_db, rng, start):
    """N tones whose amplitudes fall by span_db from the first to the last, plus noise at
    -100 dB of the strongest."""
    from gpu_sdr_amd.source import host_tones
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    ampl = (10.0 ** (-np.linspace(0.0, span_db, N) / 20.0)).astype(np.float32)
    phase = rng.uniform(0, 2 * np.pi, N).astype(np.float32)
    return freq, ampl, phase, lambda c, seed: host_tones(L, start + c * L, rate, freq, ampl, phase, sigma=1e-5, seed=seed)


@pytest.mark.parametrize("impl", ["flat", "mfma"])
@pytest.mark.parametrize("span_db", [40, 60])
@pytest.mark.parametrize("shape", [(32, 10_000_000, 100, 4, 100_000), (64, 200_000_000, 1000, 4, 200_000)],
                         ids=["M100", "M1000"])
def test_direct_high_dynamic_range_comb(cuda_device, gsdr_lib, oracle_mod, monkeypatch, impl, span_db, shape):
    """A comb whose tones span 40 / 60 dB, against the fp64 oracle.  The matrix-core engine
    carries ~22 bits relative to the largest sample of each output row's window (one power-of-two
    scale per row, fp16 hi/lo split), the fp32 engines 24 relative to each product: the weakest
    tones are where they could differ most.

    The bar is 1e-5 per tone.  A tone 60 dB under the strongest sits at the noise floor of any
    fp32 evaluation of this sum, so the test also evaluates the REFERENCE'S OWN ARITHMETIC on the
    same buffers -- oracle/recipe_b.py with complex64 accumulation: double sincos mix stored as
    float (ref: cpp/kernels.cu:72-83), then the fp32 Cgemm + Caxpy order (ref: cpp/fir.cu:44-62) --
    and measures it against the same fp64 oracle.  Per tone the HIP path must stay within the larger
    of 1e-5 and 3 x the restatement's own error, and below 1.5e-5 outright (round 2 asserted a flat 3e-5
    at 60 dB).  Both errors and their largest per-tone ratio go to the margin file.  What the evidence says
    (profiles/r03_parity_margins.json, "other_figures" for the restatement): at 40 dB everything is below 1.6e-6.
    At 60 dB, weakest tones:
        M100  (400 taps):  fp32 restatement 0.99e-5,  HIP 1.26e-5 (matrix cores) / 1.27e-5 (packed-FP32 VALU)
        M1000 (4000 taps): fp32 restatement 2.78e-5,  HIP 1.03e-5 / 1.06e-5
    So a tone 60 dB under the strongest sits at the 1e-5 bar for every fp32 evaluation of this sum: the reference's
    own order of operations misses it by a factor 2.8 on the long window (its Cgemm accumulates a thousand
    products per output in sequence), where the HIP engines -- which sum 32-sample blocks first -- stay at the
    bar; on the short window the engines are the noisier by a quarter (they mix in fp32: a table phasor times a
    block phasor, where the reference mixes in double and rounds once)."""
    N, rate, M, F, L = shape
    monkeypatch.setenv("GSDR_DDC_MFMA", "0" if impl == "flat" else "1")
    rng = np.random.default_rng(4242 + span_db)
    freq, ampl, phase, make = hdr_comb(N, rate, L, span_db, rng, 0)
    dem = make_direct(freq, rate, M, F, L)
    assert dem.kernel_name.startswith("ddc_mfma") == (impl == "mfma")
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    from oracle import recipe_b
    ref32 = recipe_b.Direct(freq, rate, M, F, L, acc=np.complex64)     # the reference's fp32 order
    worst_strong = worst_weak = worst_all = worst_weak32 = worst_ratio = 0.0
    for c in range(3):
        x = make(c, 50 + c)
        y = run_device(dem, x, cuda_device).reshape(-1, N)
        yr = ref.process(x)
        y32 = ref32.process(x)
        assert y.shape == yr.shape == y32.shape
        den = np.linalg.norm(yr[F:].astype(np.complex128), axis=0)
        d = y[F:].astype(np.complex128) - yr[F:]
        err = np.linalg.norm(d, axis=0) / den
        err32 = np.linalg.norm(y32[F:].astype(np.complex128) - yr[F:], axis=0) / den
        bound = np.maximum(TOL, 3.0 * err32)
        k = int(np.argmax(err / bound))
        assert (err <= bound).all(), (impl, span_db, c, k, float(err[k]), float(err32[k]), err[-4:].tolist(), err32[-4:].tolist())
        assert err.max() <= 1.5e-5, (impl, span_db, c, float(err.max()))
        worst_strong = max(worst_strong, float(err[: N // 2].max()))
        worst_weak = max(worst_weak, float(err[N // 2:].max()))
        worst_weak32 = max(worst_weak32, float(err32[N // 2:].max()))
        worst_ratio = max(worst_ratio, float((err / np.maximum(err32, 1e-12)).max()))
        worst_all = max(worst_all, float(np.linalg.norm(d) / np.linalg.norm(yr[F:].astype(np.complex128))))
    dem.close()
    record_margin(worst_strong, "strong half of the comb")
    record_margin(worst_weak, f"weak half of the comb (down to -{span_db} dB)")
    record_info(worst_weak32, "weak half of the comb: error of the reference's fp32 order evaluated on the CPU (oracle/recipe_b.py, complex64)")
    record_info(worst_ratio, "largest per-tone ratio HIP error / fp32-restatement error (both against the fp64 oracle)")
    record_margin(worst_all, "all tones together (error against the comb's total power)")
    assert worst_strong <= TOL, worst_strong
    assert worst_all <= 1e-6, worst_all


@pytest.mark.parametrize("path", ["fft", "ddc"])
@pytest.mark.parametrize("span_db", [40, 60])
def test_tones_high_dynamic_range_comb(cuda_device, gsdr_lib, oracle_mod, monkeypatch, path, span_db):
    """TONES on a comb of 32 tones at bin centres whose amplitudes span 40 / 60 dB, against the fp64
    oracle: "fft" = polyphase filter + fp32 FFT inside the LDS (its rounding error is relative to the
    frame's total power, so a weak bin beside strong ones is where it shows), "ddc" = every selected bin
    as a DDC tone on the matrix cores.  Recorded per path in the margin file.  Measured: the weakest
    bins at -60 dB come out at 3.3e-6 through the FFT and 4.7e-6 as DDC tones (a frame sums 4096 products
    where DIRECT's M1000 window sums 4000 of 64 tones at full scale): inside the bar on both paths."""
    from gpu_sdr_amd.source import host_tones
    nfft, F, L, N = 1024, 4, 200_000, 32
    rate = nfft * 10_000
    if path == "ddc":
        monkeypatch.setenv("GSDR_TONES_FFT", "0")
        monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    rng = np.random.default_rng(777 + span_db)
    bins = rng.choice(np.arange(1, nfft), size=N, replace=False)
    freq = (bins - nfft // 2) * (rate // nfft)
    ampl = (10.0 ** (-np.linspace(0.0, span_db, N) / 20.0)).astype(np.float32)
    phase = rng.uniform(0, 2 * np.pi, N).astype(np.float32)
    dem = make_pfb(freq, rate, nfft, F, L)
    assert (dem.kernel_name in PFB_LDS_KERNELS if path == "fft" else True) and \
        (path == "fft" or dem.kernel_name.startswith("ddc_mfma"))
    ref = oracle_mod.Pfb(freq, rate, nfft, F, L)
    np.testing.assert_array_equal(dem.bins(), ref.bins())
    from oracle import recipe_b
    ref32 = recipe_b.Pfb(freq, rate, nfft, F, L)       # the reference's mechanics in complex64 (numpy.fft for cuFFT)
    worst_strong = worst_weak = worst_all = worst_weak32 = 0.0
    for c in range(3):
        x = host_tones(L, c * L, rate, freq, ampl, phase, sigma=1e-5, seed=900 + c)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        y32 = np.asarray(ref32.process(x))
        assert y.size == yr.size == y32.size and yr.size
        y, yr = y.reshape(-1, N).astype(np.complex128), yr.reshape(-1, N).astype(np.complex128)
        d = y - yr
        den = np.linalg.norm(yr, axis=0)
        err = np.linalg.norm(d, axis=0) / den
        err32 = np.linalg.norm(y32.reshape(-1, N).astype(np.complex128) - yr, axis=0) / den
        assert (err <= np.maximum(TOL, 3.0 * err32)).all(), (path, span_db, c, float(err.max()), float(err32.max()))
        worst_strong = max(worst_strong, float(err[: N // 2].max()))
        worst_weak = max(worst_weak, float(err[N // 2:].max()))
        worst_weak32 = max(worst_weak32, float(err32[N // 2:].max()))
        worst_all = max(worst_all, float(np.linalg.norm(d) / np.linalg.norm(yr)))
    dem.close()
    record_margin(worst_strong, "strong half of the comb")
    record_margin(worst_weak, f"weak half of the comb (down to -{span_db} dB)")
    record_info(worst_weak32, "weak half of the comb: error of the reference's mechanics in complex64 on the CPU (oracle/recipe_b.py)")
    record_margin(worst_all, "all tones together (error against the comb's total power)")
    assert worst_strong <= TOL, worst_strong
    assert worst_all <= 1e-6, worst_all
    assert worst_weak <= TOL, (path, span_db, worst_weak)


@pytest.mark.parametrize("impl", ["flat", "mfma"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (32, 200_000_000, 1000, 4, 200_000)],
                         ids=["M100", "M1000"])
def test_direct_isolated_spike(cuda_device, gsdr_lib, oracle_mod, monkeypatch, impl, shape):
    """One sample at 1e6 x the signal's rms in the middle buffer of three.  The matrix-core
    engine scales by the maximum of this and the previous buffer, so while the spike is in
    reach the lo halves of ordinary samples fall into fp16 subnormals; the reference's fp32
    path has no such mode.  Rows whose window holds the spike and rows far from it are
    compared separately; both stay within the bar (recorded in the margin file)."""
    N, rate, M, F, L = shape
    monkeypatch.setenv("GSDR_DDC_MFMA", "0" if impl == "flat" else "1")
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=99)
    dem = make_direct(freq, rate, M, F, L)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    spike_at = L // 2 + 3
    far = near = 0.0
    for c in range(4):
        x = host_tones(L, c * L, rate, freq, ampl, phase, sigma=1e-3, seed=300 + c)
        if c == 1:
            rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
            x[spike_at] = np.complex64(1e6 * rms * (0.6 + 0.8j))
        y = run_device(dem, x, cuda_device).reshape(-1, N)
        yr = ref.process(x)
        rows = np.arange(L // M)
        if c == 1:
            # output row G covers samples (G-F+1)*M .. (G+1)*M
            hit = (rows >= spike_at // M) & (rows <= spike_at // M + F - 1)
            near = max(near, float(rel_err_per_tone(y[hit], yr[hit], "rows whose window holds the spike").max()))
            e = rel_err_per_tone(y[~hit][F:], yr[~hit][F:], "rows of the spike's buffer far from it")
        else:
            e = rel_err_per_tone(y[F:] if c == 0 else y, yr[F:] if c == 0 else yr,
                                 "buffer %d (the spike is in buffer 1; buffer 2 still shares its scale)" % c)
        far = max(far, float(e.max()))
    dem.close()
    assert near <= TOL, (impl, near)
    assert far <= TOL, (impl, far)


EXTREME_ENGINES = {
    # name: (GSDR_DDC_MFMA, GSDR_DDC_PIPE, GSDR_MFMA_ASM, GSDR_MFMA_PREC, GSDR_DDC_FEW)
    "flat": ("0", "1", "4", "0", "0"),        # packed-FP32 VALU kernel (north_star's arithmetic)
    "generic": ("0", "0", "4", "0", "0"),     # compiler-scheduled FP32 VALU kernel
    "mfma16": ("1", "1", "4", "0", "0"),      # the default matrix-core loop
    "mfma16w8": ("1", "1", "5", "0", "0"),
    "mfma16p": ("1", "1", "4", "1", "0"),
    "mfma32": ("1", "1", "2", "0", "0"),
    "mfmacxx": ("1", "1", "0", "0", "0"),
    "few": ("1", "1", "4", "0", "1"),         # the library as shipped: ddc_few_kernel where it takes the shape (M1000), else mfma16
}


@pytest.mark.parametrize("impl", list(EXTREME_ENGINES))
@pytest.mark.parametrize("kind", ["1e8", "1e10", "inf", "nan"])
@pytest.mark.parametrize("shape", [(16, 10_000_000, 100, 4, 100_000), (32, 200_000_000, 1000, 4, 200_000),
                                   (12, 9_000_000, 90, 4, 90_000)], ids=["M100", "M1000", "M90pad"])
def test_direct_extreme_and_nonfinite_samples(cuda_device, gsdr_lib, oracle_mod, monkeypatch, impl, kind, shape):
    """One sample at 1e8 x / 1e10 x the signal's rms, one Inf, one NaN, in the second buffer of four.
    In the reference a bad sample reaches only the outputs whose window holds it: the mix is elementwise
    (ref: cpp/kernels.cu:82-83) and the FIR sums one window (ref: cpp/fir.cu:48-61).  The same must
    hold here on every engine -- the matrix-core engines scale every output row from the finite maximum of
    its own window (row_scale_exp, csrc/ddc_mfma.hip), so a spike costs the other rows nothing:
      * rows whose window does not hold the sample: <= 1e-5 per tone in EVERY buffer;
      * rows that hold a finite spike: <= 1e-5 per tone as well (the spike term dominates them);
      * rows that hold the Inf / NaN: non-finite exactly where the oracle's outputs are.
    The sample sits 3 samples behind a block boundary: for the "M90pad" shape that is inside the zero-padded
    tail of the previous rows' windows (M*F = 360 is not a whole number of 32-sample blocks), which must not
    let it through either (0 * Inf)."""
    N, rate, M, F, L = shape
    mf, pipe, asm, prec, few = EXTREME_ENGINES[impl]
    monkeypatch.setenv("GSDR_DDC_MFMA", mf)
    monkeypatch.setenv("GSDR_DDC_PIPE", pipe)
    monkeypatch.setenv("GSDR_MFMA_ASM", asm)
    monkeypatch.setenv("GSDR_MFMA_PREC", prec)
    monkeypatch.setenv("GSDR_DDC_FEW", few)
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    if few == "1" and M >= 512 and N <= 32:
        assert dem.kernel_name == "ddc_few_kernel"
    else:
        assert dem.kernel_name.startswith("ddc_mfma") == (mf == "1"), dem.kernel_name
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    at = (L // M // 2) * M + 3
    rows = np.arange(L // M)
    hit = (rows >= at // M) & (rows <= at // M + F - 1)      # output row G covers samples (G-F+1)*M .. (G+1)*M
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
                np.testing.assert_array_equal(fin_y, fin_r, err_msg=f"{impl} {kind}: non-finite outputs elsewhere than the oracle's")
            else:
                assert fin_y.all()
                near = max(near, float(rel_err_per_tone(y[hit], yr[hit], "rows whose window holds the spike").max()))
            keep = ~hit
            keep[:F] = False
            e = rel_err_per_tone(y[keep], yr[keep], "rows of the bad sample's buffer that do not hold it")
        else:
            assert fin_y.all(), (impl, kind, c)
            e = rel_err_per_tone(y[F:] if c == 0 else y, yr[F:] if c == 0 else yr, "the other buffers")
        far = max(far, float(e.max()))
    dem.close()
    assert far <= TOL, (impl, kind, far)
    assert near <= TOL, (impl, kind, near)


def test_direct_streaming_equals_one_long_buffer(cuda_device, gsdr_lib, engine):
    """Concatenated per-buffer outputs == one call on the concatenated input."""
    from _product_loops import streaming_runs
    _, _, ya, yb = streaming_runs(cuda_device, _any_engine)
    assert rel_err_per_tone(yb, ya).max() <= 2e-6


@pytest.mark.parametrize("few", ["default", "older_kernels"])
def test_direct_undecimated(cuda_device, gsdr_lib, oracle_mod, monkeypatch, few):
    rng = np.random.default_rng(6)
    # (at most 32 tones: mix_few_kernel, a lane per (sample, tone) with its own phasor; more: a lane per tone.
    #  GSDR_MIX_FEW=0: round 2's kernels -- at most 32 tones mix_small_kernel, several sample phases per wave)
    if few == "older_kernels":
        monkeypatch.setenv("GSDR_MIX_FEW", "0")
    few_max = 32 if few == "default" else 0
    for N, rate, L in [(3, 1000, 1000), (70, 1_000_000, 5000), (5, 200_000_000, 4099), (1, 1000, 777), (2, 10_000, 2048),
                       (8, 200_000_000, 100_003), (17, 1_000_000, 9000), (32, 1_000_000, 4096), (33, 1_000_000, 4096),
                       (1, 200_000_000, 1_000_000), (4, 200_000_000, 999_983), (7, 123_456_789, 300_001), (9, 1_000_000, 5000)]:
        freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        dem = make_direct(freq, rate, 0, 4, L)
        assert dem.kernel_name == ("mix_few_kernel" if N <= few_max else "mix_small_kernel" if N <= 32 else "mix_kernel")
        ref = oracle_mod.Direct(freq, rate, 0, 4, L)
        for c in range(3):
            x = crandn(rng, L)
            y = run_device(dem, x, cuda_device) if c != 1 else run_host(dem, x)
            yr = ref.process(x)
            assert y.size == N * L
            assert rel_err_per_tone(y.reshape(-1, N), yr).max() <= 2e-6
        dem.close()


@pytest.mark.parametrize("N,M,F,L,nbuf", [(1, 1000, 4, 100_000, 4), (5, 512, 3, 102_400, 3), (16, 1000, 4, 1_000_000, 3),
                                          (32, 2000, 2, 200_000, 3), (3, 777, 8, 77_700, 4), (2, 4096, 4, 8192, 6),
                                          (7, 1000, 1, 50_000, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("few", ["few", "GSDR_DDC_FEW=0"])
def test_direct_few_tones_long_decimation(cuda_device, gsdr_lib, oracle_mod, monkeypatch, N, M, F, L, nbuf, few):
    """A handful of tones at a decimation of 512 and more: ddc_few_kernel (a wave per (chunk, tone), the lanes split
    the samples of a block) against the oracle, and the engine the library would take otherwise on the same buffers.
    The last shape but one has blocks longer than half a buffer (two blocks per call, F - 1 = 3 of carry)."""
    if few != "few":
        monkeypatch.setenv("GSDR_DDC_FEW", "0")
    rate = 200_000_000
    rng = np.random.default_rng(7000 + N * M)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_direct(freq, rate, M, F, L)
    assert (dem.kernel_name == "ddc_few_kernel") == (few == "few"), dem.kernel_name
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(nbuf):
        x = crandn(rng, L) * (1.0, 30.0, 0.01, 1.0, 5.0, 1.0)[c % 6]
        y = run_device(dem, x, cuda_device) if c != 1 else run_host(dem, x)
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M)
        e = rel_err_per_tone(y.reshape(-1, N), yr).max()
        record_margin(float(e), "worst tone")
        assert e <= TOL
    dem.close()


def test_direct_pure_tones_demodulate_to_their_phasors(cuda_device, gsdr_lib, engine):
    """Closed form, no oracle: a comb demodulates to a_k e^{i phi_k} (DC gain of h is 1)."""
    from _product_loops import pure_tones_demodulate_to_their_phasors
    pure_tones_demodulate_to_their_phasors(cuda_device, _any_engine)


# ---------------------------------------------------------------------------
# TONES (PFB)
# ---------------------------------------------------------------------------
PFB_CASES = [
    # N, rate, nfft, avg, L, buffers
    (3, 1000, 10, 4, 103, 6),                # survey probe shape
    (3, 1_000_000, 10, 4, 50_000, 3),
    (6, 1_000_000, 100, 1, 50_000, 3),
    (8, 1_000_000, 100, 4, 50_000, 4),
    (5, 200_000_000, 1000, 4, 50_123, 4),    # nfft does not divide L
    (4, 200_000_000, 1230, 4, 100_000, 3),   # the client's typical odd nfft
    (2, 1000, 64, 8, 300, 6),                # buffer shorter than the window: empty outputs
    (70, 10_000_000, 128, 2, 20_000, 3),
]


@pytest.mark.parametrize("case", PFB_CASES, ids=lambda c: "N%d_nfft%d_avg%d_L%d" % (c[0], c[2], c[3], c[4]))
def test_pfb_parity(cuda_device, gsdr_lib, oracle_mod, case, engine):
    N, rate, nfft, avg, L, nbuf = case
    rng = np.random.default_rng(2000 + nfft + avg)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    freq[0] = 0
    dem = make_pfb(freq, rate, nfft, avg, L)
    ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
    np.testing.assert_array_equal(dem.bins(), ref.bins())
    np.testing.assert_array_equal(dem.window(),
                                  oracle_mod.make_sinc_window(nfft * avg, np.float32(1. / (2 * nfft))))
    assert dem.out_capacity == N * ref.batching
    emitted = 0
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        emitted += len(yr)
        if len(yr):
            err = rel_err_per_tone(y.reshape(-1, N), yr)
            assert err.max() <= TOL, (c, err.max())
    assert emitted > 0
    dem.close()


@pytest.mark.parametrize("nfft,avg,L,nbuf", [(16, 3, 200, 4), (100, 4, 50_000, 3), (1000, 4, 50_123, 3),
                                            (64, 1, 4096, 2)])
def test_noise_full_spectrum_parity(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nfft, avg, L, nbuf, engine):
    """NOISE, decim == 0 (ref: process_pfb_spec): every FFT bin, [frame][bin].  This is round 1's
    evaluation of every bin as a DDC tone (GSDR_NOISE_FFT=0), once per DDC engine; the FFT stage
    that NOISE uses by default has its own cases below."""
    import gpu_sdr_amd as g
    monkeypatch.setenv("GSDR_NOISE_FFT", "0")
    rng = np.random.default_rng(4000 + nfft)
    p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                freq=[0], wave_type=[g.w_type.NOISE])
    dem = g.RX_buffer_demodulator(p, device_index=0)
    ref = oracle_mod.Noise(nfft, avg, L)
    assert dem.channels == 1                       # rx_single_link reports wave_type.size() channels
    assert dem.out_capacity == nfft * ref.batching
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size
        if yr.size:
            assert rel_err_per_tone(y.reshape(-1, nfft), yr).max() <= TOL
    dem.close()


@pytest.mark.parametrize("nfft", [2 * 509, 4 * 251, 1021], ids=lambda v: "nfft%d" % v)
def test_tones_frames_with_a_large_prime_factor_take_the_fft_path(cuda_device, gsdr_lib, oracle_mod, nfft):
    """The reference takes ANY fft_tones through one cufftPlanMany (ref: cpp/USRP_demodulator.cpp:150-153).  Frames of
    up to 8192 points with a prime factor above 127 ran as one DDC per selected bin until round 2; now they take
    filter + FFT + selection like every other length -- Bluestein's identity inside the LDS, one launch per buffer.
    1 M-sample buffers at 200 Msps, 64 tones, four buffers against the oracle (lengths exact, <= 1e-5 per tone),
    and the launch duration by hipEvents on its stream: at most 60 us per buffer."""
    rate, N, F, L, nbuf = 200_000_000, 64, 4, 1_000_000, 4
    rng = np.random.default_rng(nfft)
    bins = rng.choice(np.arange(nfft), size=N, replace=False)
    freq = [int((b if b < nfft // 2 else b - nfft) * (rate / nfft)) for b in bins]
    dem = make_pfb(freq, rate, nfft, F, L)
    assert dem.kernel_name == "pfb_cu_kernel", dem.kernel_name
    ref = oracle_mod.Pfb(freq, rate, nfft, F, L)
    np.testing.assert_array_equal(dem.bins(), ref.bins())
    dem.profile_enable(1)
    for c in range(nbuf):
        x = crandn(rng, L)
        y = run_device(dem, x, cuda_device)
        yr = ref.process(x)
        assert y.size == yr.size and yr.size
        assert rel_err_per_tone(y.reshape(-1, N), yr.reshape(-1, N)).max() <= TOL
    kn, kms = dem.profile_read()
    dem.close()
    us = kms / kn * 1e3
    record_info(us, "launch duration per 1 M-sample buffer in us (hipEvents)")
    assert kn == nbuf and us <= 60.0, us


NOISE_FFT_CASES = [
    # nfft, avg, L, buffers                      stages
    (16, 3, 200, 4),                           # 4 4
    (64, 1, 4096, 2),                          # 4 4 4, no averaging
    (100, 4, 50_000, 3),                       # 4 5 5
    (1000, 4, 50_123, 3),                      # 4 2 5 5 5, L not a multiple of nfft
    (1230, 4, 100_000, 3),                     # 2 3 5 41: prime factor 41 -> Bluestein through 4096
    (2 * 3 * 5 * 7 * 11 * 13, 2, 200_000, 2),  # 30030: every generic butterfly
    (1, 2, 100, 2),                            # degenerate: the "FFT" of one point
    (2, 4, 50_000, 2),
    (4099, 3, 60_000, 3),                      # prime: Bluestein through 16384
    (8192, 4, 100_000, 2),                     # 4^6 * 2
    (127 * 8, 2, 40_000, 3),                   # 1016: the largest first-stage prime of the in-LDS kernel
    (17 * 19 * 4, 3, 30_000, 3),               # 1292: two primes above 13 (19 first, 17 through the generic stage)
    (48, 8, 300, 6),                           # frames longer than a buffer: calls without a frame; 22 frames per workgroup
    (131 * 4, 2, 20_000, 2),                   # 524: prime factor 131 > 127 -> not for the in-LDS kernel
    (101, 2, 5_000, 3),                        # a prime frame: one stage; the run kernel, ten thread groups of 101 threads
    (2 * 17, 3, 3_000, 3),                     # 34: the run kernel, 30 thread groups, prime-first stage with two columns
    (2 * 509, 4, 60_000, 3),                   # 1018: prime factor 509 -> Bluestein through 2048 inside the LDS (round 3)
    (4 * 251, 3, 50_000, 3),                   # 1004: the same through 2048
    (1021, 2, 30_000, 3),                      # a prime frame through 2048
    (3 * 1009, 2, 40_000, 3),                  # 3027 -> 8192: the longest Bluestein length the LDS takes
    (2048, 4, 100_000, 2),                     # 49 frames per call: too few to fill the run kernel's units, a frame per workgroup
    (4096, 4, 100_000, 2),                     # no room for a run's raw samples in the LDS: four taps filter straight out of memory
    (4096, 3, 100_000, 2),                     # ... and so do three: the direct filter with a zero tap
    (3001, 4, 40_000, 3),                      # a prime frame through 8192 with the direct filter (two buffers of 8192 fill the LDS)
    (3072, 4, 200_000, 2),                     # 16 16 4 3, 65 frames per call: too few to fill the run kernel's units
    (250, 4, 20_000, 3),                       # 10 5 5: the radix-10 butterfly (a 2 joined with a 5)
    (70, 3, 5_000, 3),                         # 7 10
    (600, 4, 30_000, 3),                       # 8 3 5 5; 512 threads, two columns per thread in the direct filter
    (1536, 4, 60_000, 2),                      # 8 8 8 3
    (1230, 3, 60_000, 3),                      # 41 6 5 with three taps: the direct filter, two columns per thread
    (1000, 5, 50_000, 3),                      # five taps, 50 frames per call: two frames per workgroup of pfb_lds_kernel
]
# what the comments above say of the shape a case's last call runs in, asserted from describe()["pfb_last"] (path "lds",
# 256 compute units; tests/test_gpu_pfb_runs.py has the shapes that only many frames per call reach)
NOISE_FFT_BRANCH = {
    (48, 8): {"kernel": "pfb_lds_kernel", "G": 22},
    (101, 2): {"kernel": "pfb_cu_kernel", "direct": 4, "dir_s": 10},
    (34, 3): {"kernel": "pfb_cu_kernel", "direct": 4, "dir_s": 30},
    (2048, 4): {"kernel": "pfb_lds_kernel", "G": 1},
    (4096, 4): {"kernel": "pfb_cu_kernel", "direct": 3, "G": 1},
    (4096, 3): {"kernel": "pfb_cu_kernel", "direct": 3, "G": 1},
    (3001, 4): {"kernel": "pfb_cu_kernel", "direct": 5},
    (3072, 4): {"kernel": "pfb_lds_kernel", "frames": 65},
    (600, 4): {"kernel": "pfb_cu_kernel", "threads": 512, "direct": 2},
    (1230, 3): {"kernel": "pfb_cu_kernel", "direct": 2},
    (1000, 5): {"kernel": "pfb_lds_kernel", "G": 2},
}


def cuda_device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def pfb_last_is_the_plan(dem, lib, nfft, avg, frames, env=None):
    """describe()["pfb_last"] of the call that just ran is what gsdr_pfb_plan says of its frame count on this device"""
    d = dem.describe()
    if "pfb_last" not in d:
        return None
    cus = cuda_device_cus()
    sw = _pfb.switches_of_env(env or {})
    plan = _pfb.plan(lib, nfft, avg, frames, cus, sw=sw)
    assert plan is not None
    _pfb.describe_matches_plan(d["pfb_last"], plan, frames)
    return d["pfb_last"]


@pytest.mark.parametrize("path", ["fft", "ddc"])
@pytest.mark.parametrize("nfft,avg,L,nbuf", [(16384, 4, 300_000, 3), (12_000, 2, 100_000, 4)], ids=lambda v: str(v))
def test_tones_long_frames(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nfft, avg, L, nbuf, path):
    """TONES with frames above 8192 points (the in-LDS kernel's limit): the polyphase filter, the
    FFT stages through memory and a bin selection ("fft", the library's choice) against one DDC per
    bin on the matrix cores (GSDR_TONES_FFT=0), both against the oracle."""
    if path == "ddc":
        monkeypatch.setenv("GSDR_TONES_FFT", "0")
    rate, N = 200_000_000, 24
    rng = np.random.default_rng(nfft)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    dem = make_pfb(freq, rate, nfft, avg, L)
    assert dem.kernel_name == "fft_pass_kernel" if path == "fft" else dem.kernel_name.startswith("ddc_")
    ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
    np.testing.assert_array_equal(dem.bins(), ref.bins())
    assert dem.out_capacity == N * ref.batching
    emitted = 0
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        if yr.size:
            emitted += 1
            e = float(np.linalg.norm(y.reshape(-1, N) - yr.reshape(-1, N)) / np.linalg.norm(yr))
            record_margin(e, "all tones together")
            assert e <= TOL
    assert emitted >= 2
    dem.close()


PFB_LDS_KERNELS = ("pfb_cu_kernel", "pfb_lds_kernel")     # a run of frames per compute unit / a frame per workgroup


def pfb_lds_fits(nfft, avg=4):
    """Lengths TONES / NOISE run inside the LDS in one launch: up to 8192 points without a prime factor above 127
    (radix stages over the frame length), or -- round 3 -- any length whose Bluestein length m = 2^ceil(log2(2n-1))
    is at most 8192 and fits the run kernel's LDS layout (a buffer of m points plus one of max(m, avg*n); with four
    taps plus one of m: the direct filter keeps no raw samples there)."""
    m, q, largest = nfft, 2, 1
    while m > 1:
        while m % q == 0:
            m //= q
            largest = q
        q += 1
    if nfft <= 8192 and largest <= 127:
        return True
    mm = 1
    while mm < 2 * nfft - 1:
        mm *= 2
    even = lambda v: (v + 1) & ~1
    if mm > 8192:
        return False
    if (even(mm) + even(max(mm, avg * nfft)) + 128 + (nfft + 1) // 2) * 8 <= 156 * 1024:
        return True
    # up to four taps, 128 points and more: the filter runs straight out of global memory and the second buffer holds no raw samples
    return avg <= 4 and 128 <= nfft <= 4096 and (2 * even(mm) + 128 + (nfft + 1) // 2) * 8 <= 156 * 1024


@pytest.mark.parametrize("path", ["lds", "global"])
@pytest.mark.parametrize("nfft,avg,L,nbuf", NOISE_FFT_CASES, ids=lambda v: str(v))
def test_noise_fft_stage_parity(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nfft, avg, L, nbuf, path):
    """NOISE through the hand-written FFT (csrc/fft_kernels.hip) against the oracle's fp64 DFT of every
    bin.  "lds": the library's choice -- polyphase filter, transform and output of a frame in one
    workgroup, inside the LDS (up to 8192 points, prime factors up to 127: a large prime is the first
    stage); other lengths fall to the second path.  "global" (GSDR_PFB_LDS=0): polyphase filter kernel,
    then one launch per Stockham stage through memory, Bluestein for lengths with a prime factor above 13.
    Frame counts per call and the carry of unconsumed samples are exact."""
    import gpu_sdr_amd as g
    if path == "global":
        monkeypatch.setenv("GSDR_PFB_LDS", "0")
    rng = np.random.default_rng(4100 + nfft)
    p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                freq=[0], wave_type=[g.w_type.NOISE])
    dem = g.RX_buffer_demodulator(p, device_index=0)
    if path == "lds" and pfb_lds_fits(nfft, avg):
        assert dem.kernel_name in PFB_LDS_KERNELS
    else:
        assert dem.kernel_name == "fft_pass_kernel"
    ref = oracle_mod.Noise(nfft, avg, L)
    assert dem.out_capacity == nfft * ref.batching
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        if yr.size:
            # per bin over the frames of the call, and over everything together (few frames per
            # call at large nfft make a single bin's norm small)
            e_all = float(np.linalg.norm(y.reshape(-1, nfft) - yr) / np.linalg.norm(yr))
            record_margin(e_all, "all bins together")
            assert e_all <= TOL
            if yr.shape[0] >= 8:
                assert rel_err_per_tone(y.reshape(-1, nfft), yr).max() <= TOL
    if path == "lds":
        last = pfb_last_is_the_plan(dem, gsdr_lib, nfft, avg, yr.shape[0])
        for k, v in NOISE_FFT_BRANCH.get((nfft, avg), {}).items():
            assert last is not None and last[k] == v, (k, last, v)
    dem.close()


PFB_VARIANTS = [
    # environment                      kernel the library must then run (None: its own choice stands), what the variant is
    ({},                               None,             "the library's choice"),
    ({"GSDR_PFB_CU": "0"},             "pfb_lds_kernel", "a frame (or a set of short frames) per workgroup"),
    ({"GSDR_PFB_CU": "1"},             "pfb_cu_kernel",  "the run kernel, forced"),
    ({"GSDR_PFB_DIRECT": "0"},         None,             "the run kernel's filter staged through the LDS, column-wise"),
    ({"GSDR_PFB_DIRECT": "0", "GSDR_PFB_COL": "0"}, None, "... staged, point-wise"),
    ({"GSDR_PFB_CU": "1", "GSDR_PFB_CU_NT": "1024"}, "pfb_cu_kernel", "one workgroup of 1024 threads per unit"),
    ({"GSDR_PFB_CU": "1", "GSDR_PFB_CU_NT": "512"},  "pfb_cu_kernel", "two workgroups of 512 threads per unit where the direct filter takes them"),
    ({"GSDR_PFB_RADIX8": "0"},         None,             "radix 4 / 2 stages only"),
    ({"GSDR_PFB_TEAMS": "0"},          None,             "all waves of the run kernel in step through the stages (no teams)"),
]
PFB_VARIANT_SHAPES = [
    # nfft, avg, L, buffers
    (64, 4, 9_000, 3),        # short frames: thread groups in the direct filter
    (200, 4, 30_011, 3),      # 8 5 5, groups that do not divide the workgroup, L not a multiple of the frame
    (512, 4, 700, 8),         # calls without a frame (the carry alone moves), then one
    (1024, 4, 60_000, 3),     # one column per thread where the run kernel is forced; 58 frames per call fill too few units: by default a frame per workgroup
    (1230, 4, 60_000, 3),     # two columns per thread, matrix-core first stage (41)
    (1536, 4, 60_000, 2),     # two columns, 8 8 8 3
    (2600, 4, 80_000, 2),     # three columns per thread
    (4096, 4, 100_000, 2),    # four columns, a frame per unit
    (1018, 4, 40_000, 2),     # 2 * 509: Bluestein through 2048 (the run kernel under every switch but GSDR_PFB_CU=0)
    (1024, 1, 30_000, 3),     # one tap: the direct filter with three zero taps
    (1230, 2, 60_000, 3),     # two taps
    (200, 3, 30_011, 3),      # three taps, thread groups
    (1000, 6, 60_000, 3),     # six taps: staged through the LDS, point-wise
    (128, 4, 75_264, 3),      # 588 frames per call: runs of two frames in four thread groups, teams
    (1024, 4, 524_288, 2),    # 512 frames per call: runs of two frames, teams of eight waves
]
# The comments above name the shape of the run kernel: that of GSDR_PFB_CU=1 (with no switch set, calls of a few dozen
# long frames fill too few units and go to pfb_lds_kernel).  Asserted from describe()["pfb_last"] in that row.
PFB_VARIANT_FORCED_SHAPE = {
    (64, 4, 9_000): {"direct": 4, "dir_s": 8},
    (200, 4, 30_011): {"direct": 4, "dir_s": 2},
    (512, 4, 700): {"direct": 1},
    (1024, 4, 60_000): {"direct": 1, "threads": 1024},
    (1230, 4, 60_000): {"direct": 2, "threads": 1024},
    (1536, 4, 60_000): {"direct": 2},
    (2600, 4, 80_000): {"direct": 5},
    (4096, 4, 100_000): {"direct": 3, "G": 1},
    (1018, 4, 40_000): {"direct": 1},
    (1024, 1, 30_000): {"direct": 1},
    (1230, 2, 60_000): {"direct": 2},
    (200, 3, 30_011): {"direct": 4, "dir_s": 2},
    (1000, 6, 60_000): {"direct": 0, "col": 0},
    (128, 4, 75_264): {"direct": 4, "dir_s": 4, "G": 2, "teams": 1},
    (1024, 4, 524_288): {"direct": 1, "G": 2, "teams": 1},
}


@pytest.mark.parametrize("env,kernel,what", PFB_VARIANTS,
                         ids=["+".join(f"{k[9:]}={x}" for k, x in v[0].items()) or "default" for v in PFB_VARIANTS])
@pytest.mark.parametrize("nfft,avg,L,nbuf", PFB_VARIANT_SHAPES, ids=lambda v: str(v))
def test_noise_every_kernel_variant(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nfft, avg, L, nbuf, env, kernel, what):
    """Every variant of the in-LDS TONES / NOISE kernels on the same inputs against the oracle:
    the switches are the A/B switches of the library (GSDR_PFB_*), read when the handle is created.  The default
    suite only sees the variant the library picks for a shape."""
    import gpu_sdr_amd as g
    for k in ("GSDR_PFB_CU", "GSDR_PFB_DIRECT", "GSDR_PFB_COL", "GSDR_PFB_CU_NT", "GSDR_PFB_RADIX8", "GSDR_PFB_TEAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        rng = np.random.default_rng(5200 + nfft)
        p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                    freq=[0], wave_type=[g.w_type.NOISE])
        dem = g.RX_buffer_demodulator(p, device_index=0)
        blue = nfft == 1018
        if blue and env.get("GSDR_PFB_CU") == "0":
            dem.close()
            pytest.skip("Bluestein inside the LDS is the run kernel's")
        if kernel is not None and not blue and not (kernel == "pfb_cu_kernel" and nfft > 4096):
            assert dem.kernel_name == kernel, what
        assert dem.kernel_name in PFB_LDS_KERNELS
        ref = oracle_mod.Noise(nfft, avg, L)
        emitted = 0
        for c in range(nbuf):
            x = crandn(rng, L)
            y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
            yr = ref.process(x)
            assert y.size == yr.size, (c, y.size, yr.size)
            if yr.size:
                emitted += 1
                e_all = float(np.linalg.norm(y.reshape(-1, nfft) - yr) / np.linalg.norm(yr))
                record_margin(e_all, "all bins together")
                assert e_all <= TOL, what
        assert emitted >= 1
        last = pfb_last_is_the_plan(dem, gsdr_lib, nfft, avg, yr.shape[0], env)
        if env == {"GSDR_PFB_CU": "1"}:
            assert last["kernel"] == "pfb_cu_kernel"
            for k, v in PFB_VARIANT_FORCED_SHAPE[(nfft, avg, L)].items():
                assert last[k] == v, (k, last, v)
        if L in (75_264, 524_288):
            # the two shapes with runs: the switch rows compare something
            assert last["G"] >= 2 or last["kernel"] == "pfb_lds_kernel" or env.get("GSDR_PFB_CU_NT") == "512"
            if env == {"GSDR_PFB_TEAMS": "0"}:
                assert last["teams"] == 0 and _pfb.plan(gsdr_lib, nfft, avg, yr.shape[0], cuda_device_cus())["teams"] == 1
        dem.close()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def test_noise_beyond_16384_bins(cuda_device, gsdr_lib):
    """fft_tones > 16384 (refused in round 1, where every bin was a DDC tone): 20000 = 4^2 2 5^4
    and 65536 bins, 1 M-sample buffers, against numpy's double-precision FFT of the same
    polyphase-filtered frames (the oracle's O(nfft^2) DFT would take minutes here)."""
    import gpu_sdr_amd as g
    for nfft, avg in ((20_000, 4), (65_536, 2), (17_389, 2)):   # 17389 is prime: Bluestein through 65536
        L = 1_000_000
        rng = np.random.default_rng(nfft)
        p = g.param(mode="RX", rate=200_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                    freq=[0], wave_type=[g.w_type.NOISE])
        dem = g.RX_buffer_demodulator(p, device_index=0)
        w = dem.window().astype(np.float64)
        stream = np.zeros(0, dtype=np.complex64)
        for c in range(2):
            x = crandn(rng, L)
            y = run_device(dem, x, cuda_device).reshape(-1, nfft)
            stream = np.concatenate([stream, x])
            # frames r with (r + avg) * nfft < len(stream), as buffer_helper counts them
            nfr = len([r for r in range(len(stream) // nfft + 1) if r * nfft + avg * nfft < len(stream)])
            assert y.shape[0] == nfr, (nfft, c, y.shape, nfr)
            fr = np.zeros((nfr, nfft), dtype=np.complex128)
            for i in range(avg):
                fr += stream[i * nfft:(i + nfr) * nfft].astype(np.complex128).reshape(nfr, nfft) * w[i * nfft:(i + 1) * nfft]
            yr = np.fft.fft(fr, axis=1)
            e = float(np.linalg.norm(y - yr) / np.linalg.norm(yr))
            record_margin(e, f"nfft {nfft}")
            assert e <= TOL, (nfft, c, e)
            stream = stream[nfr * nfft:]          # the unconsumed samples carry over
        dem.close()


# ---------------------------------------------------------------------------
# CHIRP (VNA)
# ---------------------------------------------------------------------------
CHIRP_CASES = [
    # rate, f0, f1, steps, chirp_t, decim, L, buffers
    (200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5, 0, 5000, 3),   # survey probe, undecimated
    (200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5, 1, 5000, 4),   # ppt 7, remainder 2
    (1_000_000, -100_000, 100_000, 50, 0.00035, 2, 500, 5),             # ppt 14
    (200_000_000, -100_000_000, 100_000_000, 1_000_000, 1.0, 1, 50_000, 3),   # C4: ppt 200
    (200_000_000, -100_000_000, 100_000_000, 1_000_000, 1.5, 1, 50_000, 4),   # C4 variant: ppt 300, carry
    (200_000_000, 50_000_000, -50_000_000, 300, 3e-4, 0, 60_000, 2),    # downward sweep (wrapping chirpness)
    (200_000_000, -100_000_000, 100_000_000, 1_000_000, 30.0, 0, 20_000, 2),  # period > 2^32: 64-bit path
    (200_000_000, -100_000_000, 100_000_000, 1_000_000, 30.0, 1, 20_000, 3),  # same with lock-in, ppt 6000
    (1_000_000, -400_000, 400_000, 10, 1e-5, 3, 1000, 3),               # length 1, ppt 3 < 64 lanes
    (200_000_000, -80_000_000, 80_000_000, 1000, 3e-3, 3, 50_000, 4),   # length 600, ppt 1800: three 256-sample
                                                                        # stretches per step, three steps per point
    # many samples per point, few points per buffer (a VNA scan): chirp_lockin_split_kernel deals a point's
    # stretches to several waves and chirp_lockin_sum_kernel adds their partial sums
    (200_000_000, -100_000_000, 100_000_000, 2000, 1.0, 1, 250_000, 4),      # ppt 100 000: 2.5 points per buffer
    (200_000_000, -80_000_000, 80_000_000, 100, 0.02, 3, 200_000, 4),        # length 40 000, three steps per point
    (10_000_000, -4_000_000, 4_000_000, 50, 0.05, 2, 30_000, 5),             # ppt 20 000, 1.5 points per buffer
    (20_000_000, -8_000_000, 8_000_000, 100, 1.0, 1, 200_000, 4),            # ppt 200 000 = the buffer: one point per call, 782 stretches
]


@pytest.mark.parametrize("case", CHIRP_CASES,
                         ids=lambda c: "steps%d_t%g_dec%d_L%d" % (c[3], c[4], c[5], c[6]))
def test_chirp_parity(cuda_device, gsdr_lib, oracle_mod, case):
    rate, f0, f1, steps, t, decim, L, nbuf = case
    rng = np.random.default_rng(3000 + steps + decim)
    dem = make_chirp(rate, f0, f1, steps, t, decim, L)
    ref = oracle_mod.Chirp(rate, f0, f1, steps, t, decim, L)
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size, (c, y.size, yr.size)
        assert rel_err_per_tone(y[:, None], yr[:, None]).max() <= TOL
    dem.close()


def test_chirp_loopback_constant_phasor(cuda_device, gsdr_lib):
    """TX law -> RX law gives a constant phasor (no oracle)."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import device_chirp
    rate, L = 200_000_000, 1_000_000
    cp = g.chirp_derive(rate, -100_000_000, 100_000_000, 1_000_000, 1.0)
    dem = make_chirp(rate, -100_000_000, 100_000_000, 1_000_000, 1.0, 1, L)
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    last = 0
    for c in range(3):
        device_chirp(x, last, cp, scale=0.5)
        n = dem.process(x, out)
        torch.cuda.synchronize()
        assert n == 5000
        y = out[:n].cpu().numpy()
        # flat window drops the first ppt/10 samples and averages the rest: gain 1
        np.testing.assert_allclose(y, 0.5 + 0j, rtol=0, atol=2e-6)
        last += L
    dem.close()


# ---------------------------------------------------------------------------
# full BASELINE.json sizes
# ---------------------------------------------------------------------------
def _full_size_direct(cuda_device, oracle_mod, N, M, nbuf, subset):
    import torch
    from gpu_sdr_amd.source import device_tones, tone_comb
    rate, L, F = 200_000_000, 1_000_000, 4
    freq, ampl, phase = tone_comb(N, rate, seed=20251004)
    dem = make_direct(freq, rate, M, F, L)
    rng = np.random.default_rng(9)
    pick = np.unique(np.concatenate([[0, 63, 64, N - 1], rng.integers(0, N, size=subset)]))
    ref = oracle_mod.Direct(freq[pick], rate, M, F, L)
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    for c in range(nbuf):
        # start near the end of a second so that the NCO index wraps inside the run
        start = rate - L - 12345 + c * L
        device_tones(x, start, rate, freq, ampl, phase, sigma=1e-3, seed=77 + c)
        if c == 0:
            # the demodulator's index starts at 0: feed it the same phase origin
            pass
        n = dem.process(x, out)
        torch.cuda.synchronize()
        assert n == N * (L // M)
        y = out[:n].cpu().numpy().reshape(-1, N)
        assert np.isfinite(y.view(np.float32)).all()
        yr = ref.process(x.cpu().numpy())
        err = rel_err_per_tone(y[:, pick], yr)
        assert err.max() <= TOL, (c, err.max())
    dem.close()


def test_c2_256_tones_decim100_full_size(cuda_device, gsdr_lib, oracle_mod, engine):
    _full_size_direct(cuda_device, oracle_mod, N=256, M=100, nbuf=3, subset=12)


def test_c3_2048_tones_decim1000_full_size(cuda_device, gsdr_lib, oracle_mod, engine):
    _full_size_direct(cuda_device, oracle_mod, N=2048, M=1000, nbuf=3, subset=12)


def test_many_tones_16384_decim1000_full_size(cuda_device, gsdr_lib, oracle_mod):
    """The regime of the max-real-time-tones figure: 16384 tones (512 tone tiles), oracle on
    a subset, two buffers."""
    _full_size_direct(cuda_device, oracle_mod, N=16384, M=1000, nbuf=2, subset=10)


def test_pfb_full_size_1024_tones(cuda_device, gsdr_lib, oracle_mod, engine):
    """TONES at full buffer size: 1024 tones, the client's typical odd nfft (1230 does
    not divide 1e6: buffer_helper carry every call), oracle on a subset of tones."""
    import torch
    from gpu_sdr_amd.source import device_tones, tone_comb
    rate, L, nfft, avg, N = 200_000_000, 1_000_000, 1230, 4, 1024
    freq, ampl, phase = tone_comb(N, rate, seed=5)
    dem = make_pfb(freq, rate, nfft, avg, L)
    rng = np.random.default_rng(12)
    pick = np.unique(np.concatenate([[0, 63, 64, N - 1], rng.integers(0, N, size=8)]))
    ref = oracle_mod.Pfb(freq[pick], rate, nfft, avg, L)
    np.testing.assert_array_equal(dem.bins()[pick], ref.bins())
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    frames = 0
    for c in range(3):
        device_tones(x, c * L, rate, freq, ampl, phase, sigma=1e-2, seed=31 + c)
        n = dem.process(x, out)
        torch.cuda.synchronize()
        yr = ref.process(x.cpu().numpy())
        assert n == N * len(yr)
        frames += len(yr)
        y = out[:n].cpu().numpy().reshape(-1, N)
        err = rel_err_per_tone(y[:, pick], yr)
        assert err.max() <= TOL, (c, err.max())
    assert frames == (3 * L - avg * nfft - 1) // nfft + 1
    dem.close()


def test_c3_linearity_all_tones(cuda_device, gsdr_lib, engine):
    """Size-independent property over ALL 2048 tones at full size:
    demod(a + b) == demod(a) + demod(b)."""
    import torch
    from gpu_sdr_amd.source import tone_comb
    rate, L, M, F, N = 200_000_000, 1_000_000, 1000, 4, 2048
    freq, _, _ = tone_comb(N, rate, seed=3)
    gen = torch.Generator(device=cuda_device).manual_seed(11)
    a = torch.view_as_complex(torch.randn(L, 2, device=cuda_device, generator=gen))
    b = torch.view_as_complex(torch.randn(L, 2, device=cuda_device, generator=gen))
    ys = []
    for x in (a, b, a + b):
        dem = make_direct(freq, rate, M, F, L)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        n = dem.process(x.contiguous(), out)
        torch.cuda.synchronize()
        ys.append(out[:n].clone().reshape(-1, N))
        dem.close()
    num = torch.linalg.vector_norm(ys[2] - (ys[0] + ys[1]), dim=0)
    den = torch.linalg.vector_norm(ys[2], dim=0)
    assert float((num / den).max()) <= 5e-6


def test_c4_chirp_vna_full_size(cuda_device, gsdr_lib, oracle_mod):
    """1e6-point sweep over 200 MHz, 1 M-sample buffers, lock-in ppt = 200."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import device_chirp
    rate, L = 200_000_000, 1_000_000
    args = (rate, -100_000_000, 100_000_000, 1_000_000, 1.0)
    cp = g.chirp_derive(*args)
    dem = make_chirp(*args, 1, L)
    ref = oracle_mod.Chirp(*args, 1, L)
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    gen = torch.Generator(device=cuda_device).manual_seed(4)
    for c in range(3):
        device_chirp(x, c * L, cp, scale=0.3)
        x += 1e-3 * torch.view_as_complex(torch.randn(L, 2, device=cuda_device, generator=gen))
        n = dem.process(x, out)
        torch.cuda.synchronize()
        yr = ref.process(x.cpu().numpy())
        assert n == len(yr) == 5000
        y = out[:n].cpu().numpy()
        assert rel_err_per_tone(y[:, None], yr[:, None]).max() <= TOL
    dem.close()


# ---------------------------------------------------------------------------
# sources, passthrough, error paths
# ---------------------------------------------------------------------------
def test_device_sources_match_their_formulas(cuda_device, gsdr_lib, oracle_mod):
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import device_chirp, device_tones, host_tones, tone_comb
    rate, n = 1_000_000, 20_000
    freq, ampl, phase = tone_comb(5, rate, seed=2)
    x = torch.empty(n, dtype=torch.complex64, device=cuda_device)
    device_tones(x, rate - 7000, rate, freq, ampl, phase, sigma=0.0)
    np.testing.assert_allclose(x.cpu().numpy(), host_tones(n, rate - 7000, rate, freq, ampl, phase),
                               rtol=0, atol=3e-6)
    device_tones(x, 0, rate, freq, ampl, phase, sigma=0.1, seed=5)
    noise = x.cpu().numpy() - host_tones(n, 0, rate, freq, ampl, phase)
    assert abs(noise.real.std() - 0.1) < 0.005 and abs(noise.imag.std() - 0.1) < 0.005
    assert abs(noise.mean()) < 0.005
    cp = g.chirp_derive(200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5)
    ocp = oracle_mod.chirp_params(200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5)
    device_chirp(x, 6500, cp, scale=0.5)
    np.testing.assert_allclose(x.cpu().numpy(), oracle_mod.chirp_gen(ocp, 6500, n, 0.5), rtol=0, atol=3e-7)


def test_pipelined_submit_wait_equals_process(cuda_device, gsdr_lib, engine):
    """gsdr_demod_submit/_wait (overlapped H2D / kernels / D2H) must give exactly
    what the synchronous process() gives, in order, for every mode."""
    import torch
    import gpu_sdr_amd as g
    rng = np.random.default_rng(21)
    makers = [lambda: make_direct([1000, -2500, 77777], 1_000_000, 100, 4, 20_000),
              lambda: make_pfb([0, 125_000, -250_000], 1_000_000, 64, 4, 20_001),
              lambda: make_chirp(1_000_000, -100_000, 100_000, 50, 0.00035, 2, 5000),
              lambda: g.RX_buffer_demodulator(g.param(mode="RX", rate=1_000_000, buffer_len=50_123, decim=0,
                                                      pf_average=4, fft_tones=100, freq=[0],
                                                      wave_type=[g.w_type.NOISE]), device_index=0),
              lambda: g.RX_buffer_demodulator(g.param(rate=1000, buffer_len=3000, wave_type=[]), device_index=0)]
    for mk in makers:
        a, b = mk(), mk()
        L = a.parameters.buffer_len
        xs = [torch.from_numpy(crandn(rng, L)).pin_memory().numpy() for _ in range(9)]
        outs = [torch.empty(a.out_capacity, dtype=torch.complex64).pin_memory().numpy() for _ in range(9)]
        want = [run_host(a, x) for x in xs]
        got, pending = [], []
        for k, x in enumerate(xs):
            if len(pending) == 4:
                j = pending.pop(0)
                got.append(outs[j][:b.wait()].copy())
            b.submit(x, outs[k])
            pending.append(k)
        while pending:
            j = pending.pop(0)
            got.append(outs[j][:b.wait()].copy())
        with pytest.raises(g.GsdrError):
            b.wait()
        assert len(got) == len(want)
        for y, yr in zip(got, want):
            np.testing.assert_array_equal(y, yr)
        a.close()
        b.close()


@pytest.mark.parametrize("asm", ["2", "4"], ids=["ring", "ring16"])
@pytest.mark.parametrize("mode", ["direct", "tones"])
def test_mixed_entries_and_streams_keep_the_stream_state_in_order(cuda_device, gsdr_lib, monkeypatch, mode, asm):
    """The FIR carry, the scale slots, the raw windows and the head/tail copies pass from call
    to call ON THE DEVICE.  Calls that arrive on different streams -- process_device on two
    user streams, submit_device in between, with buffers outstanding -- must still see their
    predecessor's state: every call first joins the streams the earlier ones used (one event,
    nothing on the usual path).  A busy neighbour keeps the 'old' stream late, so a missing
    wait shows as wrong first rows.  Bit-equal to the same buffers through one in-order stream."""
    import torch
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", asm)
    rng = np.random.default_rng(2718)
    if mode == "direct":
        N, rate, M, F, L = 96, 10_000_000, 100, 4, 100_000
        freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
        a, b = make_direct(freq, rate, M, F, L), make_direct(freq, rate, M, F, L)
    else:
        N, rate, nfft, F, L = 40, 1_000_000, 100, 4, 100_037
        freq = [int(k * (rate // nfft)) for k in range(-20, 20)]
        a, b = make_pfb(freq, rate, nfft, F, L), make_pfb(freq, rate, nfft, F, L)
    nbuf = 14
    xs = [torch.from_numpy(crandn(rng, L) * np.float32(10.0 ** rng.uniform(-2, 2))).to(cuda_device) for _ in range(nbuf)]
    want = []
    for x in xs:
        out = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
        n = a.process_device(x, out)
        torch.cuda.synchronize()
        want.append(out[:n].cpu().numpy())
    s1, s2 = torch.cuda.Stream(cuda_device), torch.cuda.Stream(cuda_device)
    ballast = torch.randn(4096, 4096, device=cuda_device)
    outs = [torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in range(nbuf)]
    lens, pending = [None] * nbuf, []
    pattern = ["s1", "s2", "sub", "sub", "s1", "sub", "s2", "s2", "sub", "sub", "sub", "s1", "sub", "s2"]
    torch.cuda.synchronize()
    for k, how in enumerate(pattern):
        if how == "sub":
            if len(pending) == 3:
                j = pending.pop(0)
                lens[j] = b.wait()
            b.submit_device(xs[k], outs[k])
            pending.append(k)
        else:
            st = s1 if how == "s1" else s2
            with torch.cuda.stream(st):
                for _ in range(3):
                    ballast = ballast @ ballast * 1e-4      # keeps this stream busy for a while
            lens[k] = b.process_device(xs[k], outs[k], st)
    while pending:
        j = pending.pop(0)
        lens[j] = b.wait()
    torch.cuda.synchronize()
    for k in range(nbuf):
        assert lens[k] == want[k].size, (k, pattern[k])
        np.testing.assert_array_equal(outs[k][:lens[k]].cpu().numpy(), want[k], err_msg=f"buffer {k} via {pattern[k]}")
    a.close()
    b.close()


def test_caller_streams_may_be_destroyed_between_calls(cuda_device, gsdr_lib):
    """Every call arrives on a stream of its own, created for it and destroyed by the caller as soon as
    include/gsdr.h allows: once the NEXT call on the handle has been made -- while work on it may still be
    executing (a busy stream in front).  The handle must not touch a stream after that (it forgets a stream
    when the next call has joined it) and must not lose the order of the carry: bit-equal to the same buffers
    through one stream.  (Destroying a stream BEFORE the next call is outside the contract and cannot be made
    safe: HIP itself faults when an event is recorded on a destroyed stream -- tried, a segmentation fault inside
    hipEventRecord -- and an event of the handle's own behind every call costs 3 - 4 us of stream time per call.)"""
    import ctypes as C
    import torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    rng = np.random.default_rng(31337)
    N, rate, M, F, L = 64, 10_000_000, 100, 4, 100_000
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    a, b = make_direct(freq, rate, M, F, L), make_direct(freq, rate, M, F, L)
    nbuf = 8
    xs = [torch.from_numpy(crandn(rng, L) * np.float32(10.0 ** rng.uniform(-2, 2))).to(cuda_device) for _ in range(nbuf)]
    want = []
    for x in xs:
        out = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
        n = a.process_device(x, out)
        torch.cuda.synchronize()
        want.append(out[:n].cpu().numpy())
    ballast = torch.randn(4096, 4096, device=cuda_device)
    outs = [torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in range(nbuf)]
    lens = []
    torch.cuda.synchronize()
    prev = None
    for k in range(nbuf):
        raw = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0          # hipStreamNonBlocking
        st = torch.cuda.ExternalStream(raw.value, device=cuda_device)
        with torch.cuda.stream(st):
            for _ in range(3):
                ballast = ballast @ ballast * 1e-4                          # the call's work starts late
        lens.append(b.process_device(xs[k], outs[k], st))
        del st
        if prev is not None:
            assert hip.hipStreamDestroy(prev) == 0                          # the next call has been made: allowed
        prev = raw
    torch.cuda.synchronize()
    for k in range(nbuf):
        assert lens[k] == want[k].size
        np.testing.assert_array_equal(outs[k][:lens[k]].cpu().numpy(), want[k], err_msg=f"buffer {k}")
    assert hip.hipStreamDestroy(prev) == 0         # nothing follows on this handle but close()
    a.close()
    b.close()


@pytest.mark.parametrize("asm", ["2", "4"], ids=["ring", "ring16"])
@pytest.mark.parametrize("overlap,streams", [("1", "2"), ("1", "3"), ("0", "2")])
def test_pipelined_submit_device_overlapping_buffers(cuda_device, gsdr_lib, oracle_mod, monkeypatch, overlap,
                                                     streams, asm):
    """gsdr_demod_submit_device: the main kernels of consecutive DIRECT buffers run on two
    streams and overlap (the staging passes stay in order).  Buffers of very different
    loudness follow each other, so a kernel that picked up its neighbour's scale slot, head
    or tail copy would be far off.  Bit-equal to the in-order entry, and within tolerance
    of the oracle."""
    from _product_loops import pipelined_overlapping_buffers
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_ASM", asm)
    monkeypatch.setenv("GSDR_PIPE_OVERLAP", overlap)
    monkeypatch.setenv("GSDR_PIPE_STREAMS", streams)

    def check(dem, ran):
        assert ran or dem.kernel_name == ("ddc_mfma_ring_kernel" if asm == "2" else "ddc_mfma_ring16_kernel"), dem.kernel_name
    pipelined_overlapping_buffers(cuda_device, oracle_mod, check, N=256, L=200_000)


@pytest.mark.parametrize("streams", ["2", "3", "fft"])
def test_pipelined_submit_device_tones(cuda_device, gsdr_lib, oracle_mod, monkeypatch, streams):
    """TONES through gsdr_demod_submit_device.  On the DDC kernels (GSDR_TONES_FFT=0; 2 / 3 compute
    streams) the raw windows of consecutive buffers are separate (the staging pass of a call copies
    the unconsumed end of the previous window), so their kernels overlap too; "fft": the library's
    own choice, the frame-per-workgroup kernel with its two carry buffers.  L is no multiple of nfft:
    the carried length changes from buffer to buffer.  Bit-equal to the in-order entry, within
    tolerance of the oracle."""
    from _product_loops import pipelined_tones
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    if streams != "fft":
        monkeypatch.setenv("GSDR_TONES_FFT", "0")
        monkeypatch.setenv("GSDR_PIPE_STREAMS", streams)

    def check(dem, ran):
        assert ran or (dem.kernel_name in PFB_LDS_KERNELS if streams == "fft" else dem.kernel_name.startswith("ddc_mfma")), dem.kernel_name
    pipelined_tones(cuda_device, oracle_mod, check)


def test_pipelined_soak_full_size(cuda_device, gsdr_lib, monkeypatch):
    """400 buffers of the C2 shape (256 tones, decim 100, 1 M samples) through the overlapped
    entry while a second handle runs the same stream in order on another stream: every buffer
    bit-equal (scratch/soak.py runs the long version over C2, C3 and TONES)."""
    import torch
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    N, rate, M, F, L = 256, 200_000_000, 100, 4, 1_000_000
    rng = np.random.default_rng(8)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    a, b = make_direct(freq, rate, M, F, L), make_direct(freq, rate, M, F, L)
    gen = torch.Generator(device=cuda_device).manual_seed(5)
    bufs = [torch.view_as_complex(torch.randn(L, 2, device=cuda_device, generator=gen)) * sc
            for sc in (1e-3, 1.0, 40.0, 1.0, 1e-2, 5.0)]
    out_a = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
    outs = [torch.empty_like(out_a) for _ in range(3)]

    def fingerprint(t):
        return torch.view_as_real(t).view(torch.int32).sum(dtype=torch.int64)

    torch.cuda.synchronize()
    pend, bad = [], []
    for k in range(400):
        n = a.process_device(bufs[k % 6], out_a)
        fp = fingerprint(out_a[:n])
        if len(pend) == 3:
            kk, want = pend.pop(0)
            m = b.wait()
            if fingerprint(outs[kk % 3][:m]).item() != want.item():
                bad.append(kk)
        b.submit_device(bufs[k % 6], outs[k % 3])
        pend.append((k, fp))
    while pend:
        kk, want = pend.pop(0)
        m = b.wait()
        if fingerprint(outs[kk % 3][:m]).item() != want.item():
            bad.append(kk)
    assert not bad, bad
    a.close()
    b.close()


def test_pipelined_entry_limits(cuda_device, gsdr_lib):
    """At most GSDR_PIPELINE_DEPTH (4) buffers outstanding; wait() without one is an error;
    after draining, the synchronous entry works on the same handle."""
    import torch
    import gpu_sdr_amd as g
    dem = make_direct([1000, -2500, 77777], 1_000_000, 100, 4, 20_000)
    x = torch.zeros(20_000, dtype=torch.complex64, device=cuda_device)
    outs = [torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in range(5)]
    torch.cuda.synchronize()
    with pytest.raises(g.GsdrError):
        dem.wait()
    for k in range(4):
        dem.submit_device(x, outs[k])
    with pytest.raises(g.GsdrError, match="pipeline full"):
        dem.submit_device(x, outs[4])
    assert [dem.wait() for _ in range(4)] == [3 * 200] * 4
    with pytest.raises(g.GsdrError):
        dem.wait()
    y = run_host(dem, np.zeros(20_000, np.complex64))
    assert y.size == 600 and np.abs(y).max() == 0
    dem.close()


@pytest.mark.parametrize("rt,tones", [("0", "ddc"), ("2", "ddc"), ("0", "fft")])
def test_pipelined_fuzz_random_shapes(cuda_device, gsdr_lib, monkeypatch, rt, tones):
    """Seeded fuzz of the overlapped device entry against the in-order entry, bit for bit:
    DIRECT and TONES shapes nobody picked by hand (one row tile, partial last tiles, windows of
    one block, buffers barely longer than the carry, batch counts that change from buffer to
    buffer), seven buffers each with up to four outstanding.  TONES on the DDC kernels
    (GSDR_TONES_FFT=0) or through the frame-per-workgroup kernel (the library's choice)."""
    import torch
    from _product_loops import submit_equals_process
    monkeypatch.setenv("GSDR_DDC_MFMA", "1")
    monkeypatch.setenv("GSDR_MFMA_RT", rt)
    if tones == "ddc":
        monkeypatch.setenv("GSDR_TONES_FFT", "0")
    rng = np.random.default_rng(4242)
    ran_mfma = 0
    for it in range(36):
        rate = int(rng.choice([1_000_000, 10_000_000, 200_000_000]))
        N = int(rng.choice([1, 7, 33, 64, 129, 300]))
        F = int(rng.integers(1, 9))
        freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        if it % 3 == 2:
            nfft = int(rng.choice([16, 50, 250, 1000]))
            L = int(nfft * rng.integers(F + 2, 60) + rng.integers(0, nfft))
            mk = lambda: make_pfb(freq, rate, nfft, F, L)
        else:
            M = int(rng.choice([4, 10, 32, 100, 250, 1000]))
            L = int(M * rng.integers(max(F, 4), 400))
            mk = lambda: make_direct(freq, rate, M, F, L)
        a, b = mk(), mk()
        ran_mfma += b.kernel_name.startswith("ddc_mfma") or b.kernel_name in PFB_LDS_KERNELS
        if it % 3 == 2 and tones == "fft":
            assert b.kernel_name in PFB_LDS_KERNELS
        xs = [torch.from_numpy((crandn(rng, L) * np.float32(10.0 ** rng.integers(-3, 3))).astype(np.complex64))
              .to(cuda_device) for _ in range(7)]
        submit_equals_process(cuda_device, a, b, xs, "shape %d (%s N=%d F=%d L=%d) " % (it, b.kernel_name, N, F, L))
        a.close()
        b.close()
    assert ran_mfma >= 18


def test_profile_sampling(cuda_device, gsdr_lib):
    """gsdr_demod_profile_enable(n): hipEvents around every n-th launch of the dominant kernel."""
    import torch
    dem = make_direct([1000, -2500, 77777], 1_000_000, 100, 4, 20_000)
    x = torch.zeros(20_000, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    for every, want in ((1, 16), (True, 16), (4, 4), (8, 2)):
        dem.profile_enable(every)
        for _ in range(16):
            dem.process_device(x, out)
        torch.cuda.synchronize()
        n, ms = dem.profile_read()
        assert n == want and ms > 0
    dem.close()


def test_sw_loop_tx_tones_into_rx_direct(cuda_device, gsdr_lib):
    """The reference's --sw_loop chain: TX_buffer_generator(TONES) buffers fed
    straight to RX_buffer_demodulator(DIRECT).  TX is the unnormalised IFFT comb
    (amplitude a_k per tone), so every demodulated channel settles on a_k + 0j
    and stays there across the buffer wrap of the length-`rate` TX table."""
    import torch
    import gpu_sdr_amd as g
    rate, L, M, F = 1_000_000, 100_000, 100, 4
    freq = [-400_000 + 50_000 * k + 137 for k in range(16)]
    ampl = [1.0 / 16] * 16                       # pyUSRP/USRP_noise.py:477
    tx = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=freq, ampl=ampl,
                                       wave_type=[g.w_type.TONES] * 16))
    rx = make_direct(freq, rate, M, F, L)
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(rx.out_capacity, dtype=torch.complex64, device=cuda_device)
    for c in range(12):                          # 1.2 s of stream: wraps the TX table once
        tx.get(x)
        n = rx.process(x, out)
        torch.cuda.synchronize()
        y = out[:n].cpu().numpy().reshape(-1, 16)
        if c > 0:
            assert np.abs(y - 1.0 / 16).max() < 2e-4
    rx.close()
    tx.close()
    with pytest.raises(g.GsdrError, match="Mixed TX"):
        g.TX_buffer_generator(g.param(rate=rate, buffer_len=L, freq=[1, 2], ampl=[1, 1],
                                      wave_type=[g.w_type.TONES, g.w_type.CHIRP]))
    with pytest.raises(g.GsdrError, match="NOT IMPLEMENTED"):
        g.TX_buffer_generator(g.param(rate=rate, buffer_len=L, wave_type=[g.w_type.DIRECT]))


def test_tx_tone_generator_against_oracle(cuda_device, gsdr_lib, oracle_mod):
    """TX_buffer_generator(TONES) buffer by buffer against the oracle's tone_gen
    (cpp/kernels.cu:589-684: unnormalised inverse DFT of a bin vector filled by ASSIGNMENT):
    a 0 Hz tone and f = +rate are not generated, f = -rate is the DC term, of tones on one bin
    the last wins; buffers wrap the length-`rate` table (cpp/USRP_buffer_generator.cpp:226-229),
    and a buffer longer than `rate` replicates it (:78-90)."""
    import torch
    import gpu_sdr_amd as g
    for rate, L, nbuf in [(1_000_000, 300_007, 8), (100_000, 250_000, 3)]:
        freq = [1000, -250_000, 0, 77_777 % (rate // 2), 1000, -rate, rate, rate // 2, -250_000 % -(rate // 2) or -5, -1]
        ampl = [0.1, 0.2, 0.3, 0.05, 0.4, 0.07, 0.9, 0.11, 0.6, 0.02]
        tx = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=freq, ampl=ampl,
                                           wave_type=[g.w_type.TONES] * len(freq)))
        x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
        period = rate * max(1, -(-L // rate))
        start = 0
        for c in range(nbuf):
            tx.get(x)
            torch.cuda.synchronize()
            want = oracle_mod.tone_gen(freq, ampl, rate, start, L)
            err = float(np.max(np.abs(x.cpu().numpy() - want)))
            record_margin(err / float(np.sum(ampl)), "max abs error / sum of amplitudes")
            assert err <= 2e-6 * float(np.sum(ampl)), (rate, c, err)
            start = (start + L) % period
        tx.close()


def test_tx_tone_generator_at_scale(cuda_device, gsdr_lib):
    """TX_buffer_generator(TONES) with 2048 tones at 200 Msps and 300 tones at 1 Msps (gsdr_txgen_*: exact
    phase once per tone and 1024 samples, two table factors for the rest) against the per-sample synthesis of
    the input source (one float sincos of an exact integer phase per tone and sample), buffer by buffer --
    the second case across the wrap of the sample index at `rate`, with a buffer length that is no multiple
    of 1024, and into host memory on alternate buffers (gsdr_txgen_get).  That reference is a float32 device kernel
    itself: the first 4099 samples of every buffer are held to the float64 model (host_tones, complex128) too."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.generator import tone_bins
    from gpu_sdr_amd.source import device_tones, host_tones, tone_comb
    for N, rate, L, nbuf in [(2048, 200_000_000, 150_000, 3), (300, 1_000_000, 99_999, 13)]:
        freq, ampl, phase = tone_comb(N, rate, 17)
        tx = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=[int(f) for f in freq],
                                           ampl=[float(a) for a in ampl], wave_type=[g.w_type.TONES] * N))
        f2, a2 = tone_bins(freq, ampl, rate)
        x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
        xh = np.empty(L, dtype=np.complex64)
        want = torch.empty(L, dtype=torch.complex64, device=cuda_device)
        period = rate * max(1, -(-L // rate))
        start = 0
        for c in range(nbuf):
            if c % 2:
                tx.get(xh)
                got = torch.from_numpy(xh).to(cuda_device)
            else:
                tx.get(x)
                got = x
            device_tones(want, start, rate, f2, a2, np.zeros(len(f2), dtype=np.float32), sigma=0.0)
            torch.cuda.synchronize()
            err = float((got - want).abs().max())
            record_margin(err / float(np.sum(a2)), "max abs error / sum of amplitudes")
            assert err <= 2e-6 * float(np.sum(a2)), (N, c, err)
            # the per-sample synthesis is float32 too: the beginning of every buffer against the float64 model as well
            model = host_tones(4099, start % rate, rate, f2, a2, np.zeros(len(f2), dtype=np.float32), dtype=np.complex128)
            err = float(np.max(np.abs(got[:4099].cpu().numpy() - model)))
            record_margin(err / float(np.sum(a2)), "max abs error / sum of amplitudes")
            assert err <= 2e-6 * float(np.sum(a2)), (N, c, err, "model")
            start = (start + L) % period
        tx.close()


def test_sw_loop_tx_chirp_into_rx_chirp(cuda_device, gsdr_lib):
    """TX chirp generator -> RX chirp demodulator with lock-in: a flat S21 = ampl."""
    import torch
    import gpu_sdr_amd as g
    rate, L = 200_000_000, 1_000_000
    p = dict(rate=rate, buffer_len=L, freq=[-80_000_000], chirp_f=[80_000_000], swipe_s=[10_000],
             chirp_t=[0.0075], wave_type=[g.w_type.CHIRP])          # length 150, sweep = 1.5 buffers
    tx = g.TX_buffer_generator(g.param(mode="TX", ampl=[0.25], **p))
    rx = g.RX_buffer_demodulator(g.param(mode="RX", decim=1, **p), device_index=0)
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(rx.out_capacity, dtype=torch.complex64, device=cuda_device)
    total = 0
    for c in range(4):
        tx.get(x)
        n = rx.process(x, out)
        torch.cuda.synchronize()
        total += n
        np.testing.assert_allclose(out[:n].cpu().numpy(), 0.25 + 0j, rtol=0, atol=2e-6)
    assert total == (4 * L) // 150
    rx.close()


def test_nodsp_passthrough(cuda_device, gsdr_lib):
    import gpu_sdr_amd as g
    rng = np.random.default_rng(8)
    p = g.param(rate=1000, buffer_len=500, wave_type=[])
    dem = g.RX_buffer_demodulator(p, device_index=0)
    assert dem.mode == g.w_type.NODSP
    x = crandn(rng, 500)
    np.testing.assert_array_equal(run_host(dem, x), x)
    np.testing.assert_array_equal(run_device(dem, x, cuda_device), x)
    dem.close()


def test_unsupported_requests_fail_loudly(cuda_device, gsdr_lib, monkeypatch):
    import gpu_sdr_amd as g
    base = dict(rate=1_000_000, buffer_len=1000, freq=[1, 2])
    with pytest.raises(g.GsdrError, match="not supported"):
        g.RX_buffer_demodulator(g.param(decim=2, fft_tones=10, wave_type=[g.w_type.TONES] * 2, **base), device_index=0)
    with pytest.raises(g.GsdrError, match="multiple of decim"):
        g.RX_buffer_demodulator(g.param(decim=7, wave_type=[g.w_type.DIRECT] * 2, **base), device_index=0)
    with pytest.raises(g.GsdrError, match="pf_average"):
        g.RX_buffer_demodulator(g.param(decim=10, pf_average=9, wave_type=[g.w_type.DIRECT] * 2, **base), device_index=0)
    # NOISE takes any fft_tones through the FFT stage; only round 1's bin-by-bin evaluation is bounded
    g.RX_buffer_demodulator(g.param(fft_tones=20000, wave_type=[g.w_type.NOISE], **dict(base, buffer_len=100_000)),
                            device_index=0).close()
    monkeypatch.setenv("GSDR_NOISE_FFT", "0")
    with pytest.raises(g.GsdrError, match="fft_tones <= 16384"):
        g.RX_buffer_demodulator(g.param(fft_tones=20000, wave_type=[g.w_type.NOISE], **base), device_index=0)
    monkeypatch.delenv("GSDR_NOISE_FFT")
    with pytest.raises(g.GsdrError, match="not supported"):
        g.RX_buffer_demodulator(g.param(decim=2, fft_tones=10, wave_type=[g.w_type.NOISE], **base), device_index=0)
    with pytest.raises(g.GsdrError, match="Void demodulation"):
        g.RX_buffer_demodulator(g.param(wave_type=[g.w_type.RAMP], **base), device_index=0)


def test_native_library_is_the_one_loaded(cuda_device, gsdr_lib):
    """Guards against a silent fallback: the in-tree libgsdr.so must be mapped."""
    maps = open("/proc/self/maps").read()
    assert "gpu_sdr_amd/libgsdr.so" in maps


def test_describe_reports_the_engine_that_ran(cuda_device, gsdr_lib, monkeypatch):
    """gsdr_demod_describe: the kernel of the last launch, the pipeline streams, the build, and every
    GSDR_* variable of the process (bench.py prints it into its line)."""
    import torch
    monkeypatch.setenv("GSDR_MFMA_PREC", "0")
    rng = np.random.default_rng(5)
    dem = make_direct([1000, -2000, 3000], 1_000_000, 100, 4, 50_000)
    d0 = dem.describe()
    assert d0["mode"] == "DIRECT" and d0["timing_build"] == 0 and d0["channels"] == 3
    assert d0["env"].get("GSDR_MFMA_PREC") == "0"
    x = torch.from_numpy(crandn(rng, 50_000)).to(cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    dem.process_device(x, out)
    torch.cuda.synchronize()
    d1 = dem.describe()
    assert d1["kernel"] == dem.kernel_name == "ddc_mfma_ring16_kernel" and d1["row_tiles_per_workgroup"] == 1
    assert "timing_build 0" in gsdr_lib.gsdr_build_info().decode()
    dem.close()


def test_two_front_ends_on_one_gpu_do_not_disturb_each_other(cuda_device, gsdr_lib):
    """The reference runs one demodulator per RX front-end, each on its own thread (A_RX2 and B_RX2 of one
    board share the GPU).  A heavy matrix-core DIRECT handle streams on one thread while TONES (in-LDS FFT),
    the undecimated mix, the chirp lock-in, a second DIRECT handle and the TX tone comb generator run on threads and
    streams of their own; every result of the
    small handles must be bit-identical to what the same handle produces on an idle GPU.  Round 3 adds the
    TX chirp generator and the synthetic IQ source (source_chirp_kernel, source_tones_kernel): they run beside
    another handle's loop in the TX + RX use (ref: cpp/USRP_server_link_threads.cpp:121,136) and are built
    without packed FP32 since.

    What this guards: rule R3 of DESIGN.md section 4.1 holds ACROSS kernels -- a kernel in which the compiler
    used v_pk_*_f32 returns wrong values now and then while a wave of the matrix-core loop shares its SIMD
    (scratch/pk_hazard_ab.sh: 300+ wrong TONES buffers and 600+ wrong mix buffers in 15 s with packed FP32
    allowed in those kernels, none with the shipped library, which compiles every product kernel that can
    meet the loop with no-packed-fp32-ops) -- and that create() leaves no asynchronous initialisation
    behind.  Each thread keeps allocations, comparisons and launches on ONE stream of its own (torch's
    caching allocator reuses a freed block on the stream it was allocated on)."""
    import threading
    import time
    import torch
    import gpu_sdr_amd as g
    rate, L, NB = 200_000_000, 200_000, 8
    rng = np.random.default_rng(99)

    def mk_chirp():
        return make_chirp(rate, -rate // 2, rate // 2, 1_000_000, 1.0, 1, L)

    tone_freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=256, replace=False)

    def mk_tones():
        return make_pfb(tone_freq, rate, 1230, 4, L)

    def mk_mix():
        return make_direct([1_000_000 * (k + 1) for k in range(8)], rate, 0, 1, L)

    direct_freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=256, replace=False)

    def mk_direct():                                   # a second matrix-core front-end
        return make_direct(direct_freq, rate, 100, 4, L)

    class TxAsDem:
        """the TX tone comb generator behind the demodulators' calling convention: TX and RX of a
        front-end run at the same time"""
        def __init__(self):
            self.gen = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=[int(f) for f in tone_freq],
                                                     ampl=[0.01] * len(tone_freq), wave_type=[g.w_type.TONES] * len(tone_freq)))
            self.out_capacity = L

        def process_device(self, x, out, stream=None):
            self.gen.get(out, stream)
            return L

        def close(self):
            self.gen.close()

    class TxChirpAsDem(TxAsDem):
        """the TX chirp generator (source_chirp_kernel) the same way"""
        def __init__(self):
            self.gen = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=[-rate // 2], chirp_f=[rate // 2],
                                                     swipe_s=[1_000_000], chirp_t=[1.0], ampl=[0.5], wave_type=[g.w_type.CHIRP]))
            self.out_capacity = L

    class SourceAsDem:
        """the synthetic in-memory IQ source (source_tones_kernel): what stands in for the receiver beside the
        demodulators of the other front-end"""
        out_capacity = L

        def __init__(self):
            from gpu_sdr_amd.source import tone_comb
            self.comb = tone_comb(12, rate, seed=3)
            self.k = 0

        def process_device(self, x, out, stream=None):
            from gpu_sdr_amd.source import device_tones
            f, a, ph = self.comb
            device_tones(out, self.k * L, rate, f, a, ph, sigma=1e-3, seed=self.k, stream=stream)
            self.k += 1
            return L

        def close(self):
            pass

    cases = {"chirp": mk_chirp, "tones": mk_tones, "mix": mk_mix, "direct": mk_direct, "tx": TxAsDem,
             "tx_chirp": TxChirpAsDem, "source": SourceAsDem}
    xs = [torch.from_numpy(crandn(rng, L)).to(cuda_device) for _ in range(4)]
    refs = {}
    for name, mk in cases.items():
        dem = mk()
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        refs[name] = []
        for k in range(NB):
            n = dem.process_device(xs[k % 4], out)
            torch.cuda.synchronize()
            refs[name].append(out[:n].clone())
        dem.close()
    torch.cuda.synchronize()
    stop, lock = threading.Event(), threading.Lock()
    bad = {k: 0 for k in cases}
    rounds = {k: 0 for k in cases}
    heavy_n = [0]
    errors = []

    def heavy():
        try:
            freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=2048, replace=False)
            with lock:
                dem = make_direct(freq, rate, 1000, 4, 1_000_000)
            st = torch.cuda.Stream(cuda_device)
            with torch.cuda.stream(st):
                x = torch.from_numpy(crandn(np.random.default_rng(1), 1_000_000)).to(cuda_device)
                outs = [torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in range(3)]
                st.synchronize()
                pend = 0
                while not stop.is_set():
                    if pend == 3:
                        dem.wait()
                        pend -= 1
                    dem.submit_device(x, outs[heavy_n[0] % 3])
                    pend += 1
                    heavy_n[0] += 1
                while pend:
                    dem.wait()
                    pend -= 1
            dem.close()
        except Exception as e:                      # pragma: no cover
            errors.append(repr(e))

    def small(name):
        try:
            st = torch.cuda.Stream(cuda_device)
            with torch.cuda.stream(st):
                while not stop.is_set():
                    with lock:
                        dem = cases[name]()
                    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
                    for k in range(NB):
                        n = dem.process_device(xs[k % 4], out, st)
                        st.synchronize()
                        if not torch.equal(out[:n], refs[name][k]):
                            bad[name] += 1
                    dem.close()
                    rounds[name] += 1
        except Exception as e:                      # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=heavy)] + [threading.Thread(target=small, args=(n,)) for n in cases]
    for t in threads:
        t.start()
    time.sleep(5.0)
    stop.set()
    for t in threads:
        t.join()
    assert not errors, errors
    assert heavy_n[0] > 1000 and all(r >= 3 for r in rounds.values()), (heavy_n, rounds)
    assert bad == {k: 0 for k in cases}, (bad, rounds)


@pytest.mark.parametrize("key", ["c1", "pfb", "c4"])
def test_bench_dump_is_the_last_timed_step(key, cuda_device, gsdr_lib, tmp_path):
    """bench.py --dump-outputs: the same arguments give the same arrays, and they are what the hot path returns for
    the last timed step (the warm-up and timed steps of the stream, replayed through gsdr_demod_process_device)."""
    import torch
    import bench
    args = ["--workload", key, "--steps", "3", "--warmup", "2"]
    lines = [bench.main(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    a, b = (np.load(tmp_path / d / "iq_out.npy") for d in ("a", "b"))
    np.testing.assert_array_equal(a, b)
    assert a.dtype == np.float32 and [ln["steps"] for ln in lines] == [3, 3]
    dem, bufs, outs, N = bench.HipEngine().build(bench.WORKLOADS[key], cuda_device, bench.stream_seed(0))
    for k in range(5):
        n = dem.process_device(bufs[k % len(bufs)], outs[0])
    torch.cuda.synchronize()
    want = outs[0][:n].cpu().numpy().reshape(-1, N)
    dem.close()
    y = a[..., 0] + 1j * a[..., 1]
    assert y.shape == want.shape and n > 0
    err = np.linalg.norm(y - want, axis=0) / np.linalg.norm(want, axis=0)
    assert err.max() <= TOL, err.max()
