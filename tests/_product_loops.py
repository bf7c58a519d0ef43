"""The product loops of the pre-converted matrix-core DDC (DESIGN.md sections 4.1d - 4.1h), one row each: the
environment that selects a loop -- EVERY selecting switch set, so that a switch added later cannot reroute the handle
-- and the five describe() values a handle on that loop reports.  Shared by tests/test_gpu_product_loops.py (the cases
every loop runs) and the loops' own files (test_gpu_mfma3.py, test_gpu_mfma3r2.py, test_gpu_fold.py, test_gpu_fold4.py,
test_gpu_widetile.py), with the helpers those files have in common.  Not collected."""
import numpy as np

from test_gpu_parity import TOL, crandn, hdr_comb, make_direct, rel_err_per_tone, run_device, run_host

KERNEL = "ddc_mfma_ring16p_kernel"          # the name every pre-converted loop reports
DESCRIBE = ("complex_mac", "rotation_blocks", "fold", "fold_products", "wave_tones")
FOUR_PRODUCTS = (4, 1, 0, 0, 32)            # what every handle off these loops reports

# pre-converted operands forced on the ring16 loop; GSDR_DDC_FEW=0: also where ddc_few_kernel would take the shape
# (the C3 block); GSDR_TONES_FFT=0: TONES handles run the DDC kernels
COMMON = {"GSDR_DDC_MFMA": "1", "GSDR_DDC_FEW": "0", "GSDR_MFMA_ASM": "4", "GSDR_MFMA_PREC": "1", "GSDR_TONES_FFT": "0"}


def _row(m3, rot, fold, products, tones, describe):
    return (dict(COMMON, GSDR_MFMA_3M=m3, GSDR_MFMA_3M_ROT=rot, GSDR_MFMA_FOLD=fold, GSDR_MFMA_FOLD_PRODUCTS=products,
                 GSDR_MFMA_WAVE_TONES=tones), describe)


LOOPS = {
    # name: (environment, (complex_mac, rotation_blocks, fold, fold_products, wave_tones))
    "p3":   _row("1", "1", "0", "4", "32", (3, 1, 0, 0, 32)),      # ddc_mfma_ring16p3_kernel
    "p3r2": _row("1", "2", "0", "4", "32", (3, 2, 0, 0, 32)),      # ddc_mfma_ring16p3r2_kernel
    "p3f":  _row("1", "2", "1", "3", "32", (3, 2, 1, 3, 32)),      # ddc_mfma_ring16p3f_kernel
    "p4f":  _row("1", "2", "1", "4", "32", (3, 2, 1, 4, 32)),      # ddc_mfma_ring16p4f_kernel
    "p4fw": _row("1", "2", "1", "4", "64", (3, 2, 1, 4, 64)),      # ddc_mfma_ring16p4fw_kernel
}


def force(monkeypatch, name):
    """Only the row's environment of the engine switches is set."""
    from test_gpu_extents import clean_env
    clean_env(monkeypatch, LOOPS[name][0])


def describe_tuple(dem):
    d = dem.describe()
    return tuple(d[k] for k in DESCRIBE)


def is_loop(dem, name):
    """Asserts that `dem` is a handle of loop `name`: the kernel name and the whole five-tuple (before the first call
    and after the last)."""
    assert (dem.kernel_name, describe_tuple(dem)) == (KERNEL, LOOPS[name][1]), (name, dem.kernel_name, dem.describe())
    return True


# DIRECT_CASES the matrix-core engine does not take (setup rules of csrc/demod.cpp: the zero padding
# behind a window must fit the next block, a buffer holds at least F-1 blocks): they run the generic
# VALU kernel under every GSDR_MFMA_* setting, today's mfma16p engine included
VALU_CASES = {(1, 1000, 10, 8, 1000, 5), (5, 1000, 50, 4, 100, 7), (4, 1_000_000, 7, 3, 7000, 3)}

shape_id = lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4])


def direct_parity(cuda_device, oracle_mod, loop, case):
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
        assert describe_tuple(dem) == FOUR_PRODUCTS, dem.describe()
    else:
        is_loop(dem, loop)
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    for c in range(nbuf):
        x = crandn(rng, L)
        y = (run_host if c % 2 else run_device)(dem, x, *(() if c % 2 else (cuda_device,)))
        yr = ref.process(x)
        assert y.size == yr.size == N * (L // M)
        err = rel_err_per_tone(y.reshape(-1, N), yr)
        print(f"{loop} case {case} ({(M * F + 31) // 32} blocks) buffer {c}: worst per-tone error {err.max():.3e}")
        assert err.max() <= TOL, (c, err.max())
    if case not in VALU_CASES:
        is_loop(dem, loop)
    dem.close()


EXTREME_KINDS = ["1e8", "1e10", "inf", "nan"]
EXTREME_SHAPES = {"M100": (16, 10_000_000, 100, 4, 100_000), "M1000": (32, 200_000_000, 1000, 4, 200_000),
                  "M90pad": (12, 9_000_000, 90, 4, 90_000)}


def extreme_and_nonfinite_samples(cuda_device, oracle_mod, loop, kind, shape):
    """test_direct_extreme_and_nonfinite_samples of tests/test_gpu_parity.py, same three assertions:
    a NaN in b makes a+b NaN, so the rows that hold it are non-finite for every tone, as the oracle's."""
    N, rate, M, F, L = EXTREME_SHAPES[shape]
    from gpu_sdr_amd.source import host_tones, tone_comb
    freq, ampl, phase = tone_comb(N, rate, seed=77)
    dem = make_direct(freq, rate, M, F, L)
    is_loop(dem, loop)
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
    is_loop(dem, loop)
    dem.close()
    print(f"{loop} {kind} {shape}: far {far:.3e} near {near:.3e}")
    assert far <= TOL, (kind, far)
    assert near <= TOL, (kind, near)


C3 = (2048, 200_000_000, 1000, 4, 1_000_000)


def _c3_handle(M=1000):
    from gpu_sdr_amd.source import tone_comb
    N, rate, _, F, _ = C3
    freq, ampl, phase = tone_comb(N, rate, seed=20251004)
    return make_direct(freq, rate, M, F, M * 1000), (freq, ampl, phase)


def every_entry_is_bit_identical(cuda_device, same):
    """Two C3 handles under the environment as it is, `same(handle)` asserted of both throughout: process_device on two
    caller streams, submit_device in between, the synchronous host entry -- bit-equal to one in-order stream."""
    import torch
    from gpu_sdr_amd.source import device_tones
    N, rate, M, F, L = C3
    a, (freq, ampl, phase) = _c3_handle()
    b, _ = _c3_handle()
    assert same(a) and same(b), (a.kernel_name, a.describe())
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
