"""The product loops of the pre-converted matrix-core DDC (DESIGN.md sections 4.1d - 4.1h), one row each: the
environment that selects a loop -- EVERY selecting switch set, so that a switch added later cannot reroute the handle
-- and the five describe() values a handle on that loop reports.  Shared by tests/test_gpu_product_loops.py (the cases
every loop runs) and the loops' own files (test_gpu_mfma3.py, test_gpu_mfma3r2.py, test_gpu_fold.py, test_gpu_fold4.py,
test_gpu_widetile.py), with the helpers those files have in common; the second half holds the seeded shape draw and the
bodies of the engine-wide behavioural tests, which tests/test_gpu_parity.py runs on the engines up to the four-product
build and tests/test_gpu_product_loops.py on each loop.  Not collected."""
import numpy as np

from _margins import record_info, record_margin
from test_gpu_parity import TOL, crandn, hdr_comb, make_direct, make_pfb, rel_err_per_tone, run_device, run_host

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


# DIRECT_CASES the matrix-core engine does not take (setup rules of csrc/ddc_plan.h: the zero padding
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


# ---------------------------------------------------------------------------
# the engine-wide behavioural tests of tests/test_gpu_parity.py, their bodies stated once: called from there (every
# engine up to the four-product build) and from tests/test_gpu_product_loops.py (each loop).  `check(dem, ran)`
# asserts the engine of a handle, before its first call (ran false) and after its last.
# ---------------------------------------------------------------------------
FUZZ_SEED = 0
FUZZ_F = (1, 8)
FUZZ_M = (8, 13, 16, 20, 25, 33, 37, 40, 64, 72, 90, 100, 127, 250, 1000)
FUZZ_ROWS = 70
FUZZ_RATE = (1000, 65_536, 1_000_000, 200_000_000)
FUZZ_N = (1, 2, 5, 31, 32, 33, 63, 64, 65, 130, 257)


def matrix_cores_take(M, F, L):
    """The setup rule of csrc/ddc_plan.h (ddc_mfma_takes_direct), asked of the library under the switches of COMMON: a
    buffer holds the carry, and the zero padding behind a window fits the next block."""
    import _ddc_plan
    from gpu_sdr_amd import _lib
    return _ddc_plan.plan(_lib.lib(), 1, M, F, L, env=COMMON)["engine"] == "mfma"


def loop_fuzz_shapes():
    """36 DIRECT shapes (N, rate, M, F, L) nobody picked by hand, every one taken by the matrix cores (rejection
    sampling against matrix_cores_take); tests/test_product_loops_host.py holds what the list must contain."""
    rng = np.random.default_rng(FUZZ_SEED)
    shapes = []
    while len(shapes) < 36:
        F = int(rng.integers(FUZZ_F[0], FUZZ_F[1] + 1))
        M = int(rng.choice(FUZZ_M))
        rows = int(rng.integers(max(F - 1, 1), FUZZ_ROWS + 1))
        rate = int(rng.choice(FUZZ_RATE))
        N = int(rng.choice(FUZZ_N))
        if matrix_cores_take(M, F, M * rows):
            shapes.append((N, rate, M, F, M * rows))
    return shapes


_REFS = {}


def _once(key, build):
    """What build() returns (a tuple of arrays and lists of arrays), computed once per session, shared by the engines
    and never modified."""
    if key not in _REFS:
        got = build()
        for part in got:
            for a in (part if isinstance(part, list) else [part]):
                a.flags.writeable = False
        _REFS[key] = got
    return _REFS[key]


def _scaled(rng, L, scale):
    return (crandn(rng, L) * np.float32(scale)).astype(np.complex64)


def direct_stream(oracle_mod, shape, seed, scales, distinct=False, nref=None):
    """-> (freq, xs, yrs): the tones, one white-noise buffer per entry of `scales` and the oracle's outputs for the
    first `nref` of them (all by default), drawn in this order from default_rng(seed)."""
    N, rate, M, F, L = shape
    nref = len(scales) if nref is None else nref

    def build():
        rng = np.random.default_rng(seed)
        if distinct:
            freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
        else:
            freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        xs = [_scaled(rng, L, sc) for sc in scales]
        ref = oracle_mod.Direct(freq, rate, M, F, L)
        return freq, xs, [np.array(ref.process(x)) for x in xs[:nref]]
    return _once(("direct", shape, seed, tuple(scales), distinct, nref), build)


def fuzz_random_shapes(cuda_device, oracle_mod, check, name):
    """The shapes of loop_fuzz_shapes(), three buffers each through the device entry: exact lengths, every tone within
    TOL of the oracle."""
    for it, shape in enumerate(loop_fuzz_shapes()):
        N, rate, M, F, L = shape
        freq, xs, yrs = direct_stream(oracle_mod, shape, 7770 + it, [1.0] * 3)
        dem = make_direct(freq, rate, M, F, L)
        check(dem, False)
        worst = 0.0
        for c, (x, yr) in enumerate(zip(xs, yrs)):
            y = run_device(dem, x, cuda_device)
            assert y.size == yr.size == N * (L // M), (it, shape, c, y.size, yr.size)
            err = rel_err_per_tone(y.reshape(-1, N), yr)
            worst = max(worst, float(err.max()))
            assert err.max() <= TOL, (it, shape, c, float(err.max()))
        check(dem, True)
        dem.close()
        print(f"{name} shape {it} {shape} ({(M * F + 31) // 32} blocks, {L // M} rows): worst per-tone error {worst:.3e}")


def submit_equals_process(cuda_device, a, b, xs, what=""):
    """The device buffers `xs` through process_device of `a`, one at a time, and through submit_device of `b` with up
    to four outstanding: the same lengths and the same bits.  Returns b's outputs (host copies)."""
    import torch
    out_a = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
    want = []
    for x in xs:
        n = a.process_device(x, out_a)
        torch.cuda.synchronize()
        want.append(out_a[:n].cpu().numpy())
    outs = [torch.zeros(b.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in xs]
    torch.cuda.synchronize()
    got, pending = [], []
    for k, x in enumerate(xs):
        if len(pending) == 4:
            j = pending.pop(0)
            got.append(outs[j][:b.wait()].cpu().numpy())
        b.submit_device(x, outs[k])
        pending.append(k)
    while pending:
        j = pending.pop(0)
        got.append(outs[j][:b.wait()].cpu().numpy())
    assert [len(y) for y in got] == [len(y) for y in want], what
    for k, (y, yr) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(y, yr, err_msg=f"{what}buffer {k}")
    return got


def pipelined_fuzz(cuda_device, check, name):
    """The first 12 shapes of loop_fuzz_shapes(), seven buffers each whose loudness changes by up to five orders from
    one to the next: the overlapped entry with up to four outstanding against the in-order entry, bit for bit."""
    import torch
    for it, shape in enumerate(loop_fuzz_shapes()[:12]):
        N, rate, M, F, L = shape
        rng = np.random.default_rng(4200 + it)
        freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
        a, b = make_direct(freq, rate, M, F, L), make_direct(freq, rate, M, F, L)
        check(a, False)
        check(b, False)
        xs = [torch.from_numpy(_scaled(rng, L, 10.0 ** rng.integers(-3, 3))).to(cuda_device) for _ in range(7)]
        got = submit_equals_process(cuda_device, a, b, xs, f"{name} shape {it} {shape} ")
        assert [len(y) for y in got] == [N * (L // M)] * 7, (it, shape)
        check(a, True)
        check(b, True)
        a.close()
        b.close()


DYNAMIC_RANGE_SHAPE = (40, 10_000_000, 100, 4, 20_000)
DYNAMIC_RANGE_SCALES = (1.0, 1e-6, 1e-6, 3e4, 1.0, 0.0, 1e-3, 0.0)


def dynamic_range_and_scale_carry(cuda_device, oracle_mod, check):
    """The matrix-core DDC scales every buffer into fp16 range from its own maximum (and
    the previous buffer's, whose tail it still reads).  Same tolerance for inputs of
    1e-6, 1 and 3e4, for a loud buffer followed by a quiet one and vice versa, and an
    all-zero buffer gives exact zeros."""
    N, rate, M, F, L = DYNAMIC_RANGE_SHAPE
    freq, xs, yrs = direct_stream(oracle_mod, DYNAMIC_RANGE_SHAPE, 99, DYNAMIC_RANGE_SCALES)
    dem = make_direct(freq, rate, M, F, L)
    check(dem, False)
    for c, (scale, x, yr) in enumerate(zip(DYNAMIC_RANGE_SCALES, xs, yrs)):
        y = run_device(dem, x, cuda_device).reshape(-1, N)
        assert y.shape == yr.shape, (c, scale)
        assert np.isfinite(y.view(np.float32)).all(), (c, scale)
        den = np.linalg.norm(yr, axis=0)
        if den.max() == 0:
            assert np.abs(y).max() == 0
            continue
        # rows fed by the previous (louder) buffer's tail dominate the norm of a quiet
        # buffer: compare where the reference itself is not ~0
        err = np.linalg.norm(y - yr, axis=0) / np.where(den == 0, 1, den)
        record_margin(float(err.max()), f"buffer {c}, loudness {scale:g}")
        assert err.max() <= TOL, (c, scale, err.max())
    check(dem, True)
    dem.close()


def more_tap_phases(cuda_device, oracle_mod, check, F, M, alternate):
    """pf_average 5..8: the packed-FP32 production kernel stops at 4, the matrix-core DDC
    takes any window that is made of whole blocks behind its last sample.  Three buffers through the device entry, or
    (`alternate`) through the device and the host entry in turn."""
    N, rate, L = 70, 1_000_000, M * 300
    freq, xs, yrs = direct_stream(oracle_mod, (N, rate, M, F, L), F, [1.0] * 3)
    dem = make_direct(freq, rate, M, F, L)
    check(dem, False)
    for c, (x, yr) in enumerate(zip(xs, yrs)):
        y = (run_host(dem, x) if alternate and c % 2 else run_device(dem, x, cuda_device)).reshape(-1, N)
        assert y.shape == yr.shape, (F, c)
        assert rel_err_per_tone(y, yr).max() <= TOL, (F, c)
    check(dem, True)
    dem.close()


TWO_HANDLES = [(33, 10_000_000, 100, 4, 30_000), (70, 1_000_000, 40, 2, 16_000)]


def two_handles_interleaved(cuda_device, oracle_mod, make, check):
    """Two matrix-core demodulators fed alternately on one stream (the server's two RX front
    ends): carry, scale slots and head/tail copies are per handle.  make(k, freq, rate, M, F, L) creates handle k (the
    first before the second), check(k, dem, ran) asserts its engine."""
    def build():
        rng = np.random.default_rng(123)
        freqs = [rng.integers(-rate // 2 + 1, rate // 2, size=N) for N, rate, M, F, L in TWO_HANDLES]
        refs = [oracle_mod.Direct(freqs[k], rate, M, F, L) for k, (N, rate, M, F, L) in enumerate(TWO_HANDLES)]
        xs, yrs = [], []
        for c in range(4):
            for k, (N, rate, M, F, L) in enumerate(TWO_HANDLES):
                xs.append(_scaled(rng, L, 10.0 ** (c - 2 * k)))
                yrs.append(np.array(refs[k].process(xs[-1])))
        return freqs, xs, yrs
    freqs, xs, yrs = _once("two handles", build)
    dems = [make(k, freqs[k], *TWO_HANDLES[k][1:]) for k in range(2)]
    for k, d in enumerate(dems):
        check(k, d, False)
    for c in range(4):
        for k, (N, rate, M, F, L) in enumerate(TWO_HANDLES):
            y = run_device(dems[k], xs[2 * c + k], cuda_device).reshape(-1, N)
            assert y.shape == yrs[2 * c + k].shape, (c, k)
            assert rel_err_per_tone(y, yrs[2 * c + k], f"handle {k}").max() <= TOL, (c, k)
    for k, d in enumerate(dems):
        check(k, d, True)
        d.close()


STREAMING_SHAPE = (9, 1_000_000, 100, 4, 60_000)


def streaming_runs(cuda_device, check):
    """One stream of 60 000 samples as one buffer and as three of 20 000 -> (freq, x, ya, yb), [rows][N] each."""
    N, rate, M, F, L = STREAMING_SHAPE
    rng = np.random.default_rng(5)
    freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
    x = crandn(rng, L)
    a = make_direct(freq, rate, M, F, L)
    check(a, False)
    ya = run_device(a, x, cuda_device).reshape(-1, N)
    check(a, True)
    a.close()
    b = make_direct(freq, rate, M, F, L // 3)
    check(b, False)
    yb = np.concatenate([run_device(b, x[c * (L // 3):(c + 1) * (L // 3)], cuda_device) for c in range(3)]).reshape(-1, N)
    check(b, True)
    b.close()
    return freq, x, ya, yb


def pure_tones_demodulate_to_their_phasors(cuda_device, check):
    """Closed form, no oracle: a comb demodulates to a_k e^{i phi_k} (DC gain of h is 1)."""
    from gpu_sdr_amd.source import host_tones
    rate, L, M, F, N = 10_000_000, 100_000, 100, 4, 12
    freq = (np.arange(N) - N // 2) * 400_000 + 12_345  # >= 4 output bandwidths apart
    ampl = np.linspace(0.02, 0.08, N).astype(np.float32)
    phase = np.linspace(0, 6, N).astype(np.float32)
    dem = make_direct(freq, rate, M, F, L)
    check(dem, False)
    ys = []
    for c in range(2):
        ys.append(run_device(dem, host_tones(L, c * L, rate, freq, ampl, phase), cuda_device).reshape(-1, N))
    check(dem, True)
    dem.close()
    y = np.concatenate(ys)[F:]
    want = ampl * np.exp(1j * phase.astype(np.float64))
    worst = float(np.abs(y - want).max())
    record_info(worst, "largest |y - a e^{i phi}| behind the first F rows (bar 5e-4)")
    assert worst < 5e-4  # stop-band leakage of the other tones


OVERLAP_SCALES = (1.0, 1e-4, 30.0, 1.0, 1e-3, 1e-3, 100.0, 1.0, 1.0, 1e-2, 5.0)


def pipelined_overlapping_buffers(cuda_device, oracle_mod, check, N, L):
    """gsdr_demod_submit_device: the main kernels of consecutive DIRECT buffers run on two
    streams and overlap (the staging passes stay in order).  Buffers of very different
    loudness follow each other, so a kernel that picked up its neighbour's scale slot, head
    or tail copy would be far off.  Bit-equal to the in-order entry, and within tolerance
    of the oracle."""
    import torch
    rate, M, F = 10_000_000, 100, 4
    freq, xs_host, yrs = direct_stream(oracle_mod, (N, rate, M, F, L), 314, OVERLAP_SCALES, distinct=True, nref=4)
    a, b = make_direct(freq, rate, M, F, L), make_direct(freq, rate, M, F, L)
    check(a, False)
    check(b, False)
    xs = [torch.from_numpy(x.copy()).to(cuda_device) for x in xs_host]
    got = submit_equals_process(cuda_device, a, b, xs)
    for k, yo in enumerate(yrs):
        assert got[k].size == yo.size, k
        den = np.linalg.norm(yo, axis=0)
        err = np.linalg.norm(got[k].reshape(-1, N) - yo, axis=0) / den
        record_margin(float(err.max()), f"buffer {k}, loudness {OVERLAP_SCALES[k]:g}")
        assert err.max() <= TOL, (k, err.max())
    # the in-order entry keeps working on the same handle once the pipeline is drained
    out = torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device)
    n = b.process_device(xs[0], out)
    torch.cuda.synchronize()
    assert n == N * (L // M)
    check(a, True)
    check(b, True)
    a.close()
    b.close()


PIPELINED_TONES_SCALES = (1.0, 1e-3, 50.0, 1.0, 1e-2, 1.0, 7.0, 1.0, 1.0)


def pipelined_tones(cuda_device, oracle_mod, check):
    """TONES through gsdr_demod_submit_device, L no multiple of nfft: the carried length and the batch count change
    from buffer to buffer.  Bit-equal to the in-order entry, within tolerance of the oracle."""
    import torch
    rate, nfft, F, L, N = 10_000_000, 250, 4, 100_003, 96

    def build():
        rng = np.random.default_rng(2718)
        freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
        xs = [_scaled(rng, L, sc) for sc in PIPELINED_TONES_SCALES]
        ref = oracle_mod.Pfb(freq, rate, nfft, F, L)
        return freq, xs, [np.array(ref.process(x)) for x in xs[:4]]
    freq, xs_host, yrs = _once("pipelined tones", build)
    a, b = make_pfb(freq, rate, nfft, F, L), make_pfb(freq, rate, nfft, F, L)
    check(a, False)
    check(b, False)
    xs = [torch.from_numpy(x.copy()).to(cuda_device) for x in xs_host]
    got = submit_equals_process(cuda_device, a, b, xs)
    assert len({len(y) for y in got}) > 1          # the batch count does change
    for k, yo in enumerate(yrs):
        assert yo.size == got[k].size
        yo = yo.reshape(-1, N)
        den = np.linalg.norm(yo, axis=0)
        err = np.linalg.norm(got[k].reshape(-1, N) - yo, axis=0) / den
        record_margin(float(err.max()), f"buffer {k}, loudness {PIPELINED_TONES_SCALES[k]:g}")
        assert err.max() <= TOL, (k, err.max())
    check(a, True)
    check(b, True)
    a.close()
    b.close()
