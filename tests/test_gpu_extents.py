"""Extents and alignment of every device entry (include/gsdr.h, "Extents and alignment of device pointers").

Every other GPU test hands the library tensors of their own: aligned to 512 bytes, rounded up in size, a finite
neighbour behind them.  Here every buffer is a view into the middle of a larger allocation of the test's own
(tests/_extents.py): 65 536 samples of guard on each side, the view 0 or 1 sample past a 16-byte boundary, the input
guards NaN or +-1e30, the output allocation a sentinel NaN throughout.

For every case, three consecutive buffers (zero carry, a real carry, the state handed on) through process_device
and, on a handle of its own, through submit_device with two buffers outstanding; all four (in_off, out_off) and both
guard patterns.  Asserted:
  1. lengths equal the oracle's, per-tone error within TOL (1e-5);
  2. after every buffer: the output's guards untouched, 0 <= n <= capacity, out[0, n) written; the input allocation
     bit for bit what it was;
  3. outputs bit-equal to those of a twin handle fed the same samples from plain tensors of their own through the same
     entry: what lies outside the buffer, and where the buffer starts, must not matter;
  4. the engine meant to run did run (kernel_name; complex_mac and rotation_blocks for the pre-converted family), at
     creation and after the last buffer.
The shapes are the smallest with a partial row tile, an odd row stride or a window that ends short of its last
32-sample block; none is a workload size.
"""
import os

import numpy as np
import pytest

import _ddc_plan
from _extents import PATTERNS, check_input_untouched, check_output, guarded_input, guarded_output
from _product_loops import LOOPS
from test_gpu_parity import (CHIRP_CASES, PFB_LDS_KERNELS, PFB_VARIANTS, TOL, crandn, make_chirp, make_direct, make_pfb,
                             rel_err_per_tone)

pytestmark = pytest.mark.gpu

NBUF = 3
OFFSETS = [(i, o) for i in (0, 1) for o in (0, 1)]
P16 = "ddc_mfma_ring16p_kernel"          # the name every pre-converted loop reports


# ---------------------------------------------------------------------------
# the run pattern
# ---------------------------------------------------------------------------
def _feed(dem, entry, xs, dev, place_in, place_out, after):
    """The buffers `xs` through `entry` of `dem`; place_in(x) / place_out(cap) -> (whole, view); after(k, whole_in,
    whole_out, view_out, n) runs once buffer k is complete.  Returns the outputs (host copies)."""
    import torch
    cap = dem.out_capacity
    ys = [None] * len(xs)

    def done(k, bufs, n):
        (win, _), (wout, vout) = bufs
        after(k, win, wout, vout, n)
        ys[k] = vout[:n].cpu().numpy().copy()

    if entry == "process":
        for k, x in enumerate(xs):
            bufs = (place_in(x), place_out(cap))
            n = dem.process_device(bufs[0][1], bufs[1][1])
            torch.cuda.synchronize()
            done(k, bufs, n)
    else:
        bufs = [(place_in(x), place_out(cap)) for x in xs]
        torch.cuda.synchronize()                  # submit_device: the input must be complete
        pending = []
        for k in range(len(xs)):
            if len(pending) == 2:                 # two buffers outstanding
                j = pending.pop(0)
                done(j, bufs[j], dem.wait())
            dem.submit_device(bufs[k][0][1], bufs[k][1][1])
            pending.append(k)
        while pending:
            j = pending.pop(0)
            done(j, bufs[j], dem.wait())
    return ys


def _plain(dev):
    import torch
    return (lambda x: (None, torch.from_numpy(np.ascontiguousarray(x)).to(dev)),
            lambda cap: (None, torch.empty(cap, dtype=torch.complex64, device=dev)),
            lambda k, win, wout, vout, n: None)


def _guarded(xs, in_off, out_off, pattern, dev):
    def after(k, win, wout, vout, n):
        check_output(wout, vout, n)
        check_input_untouched(win, xs[k], in_off, pattern)
    return (lambda x: guarded_input(x, in_off, pattern, dev), lambda cap: guarded_output(cap, out_off, dev), after)


def run_case(dev, make, expect, xs, yrs, ncol):
    """make() -> a new handle; expect(dem) asserts the engine; xs: the buffers; yrs: the oracle's outputs
    ([rows][ncol] each; CHIRP and NODSP: one column)."""
    for entry in ("process", "submit"):
        # the guarded runs first: a stray write is seen in a guard zone before any plain tensor is handed in
        runs = []
        for pattern in PATTERNS:
            for in_off, out_off in OFFSETS:
                dem = make()
                expect(dem, False)
                got = _feed(dem, entry, xs, dev, *_guarded(xs, in_off, out_off, pattern, dev))      # (2)
                expect(dem, True)                                                                 # (4)
                dem.close()
                runs.append(((entry, pattern, in_off, out_off), got))
        twin = make()
        expect(twin, False)
        want = _feed(twin, entry, xs, dev, *_plain(dev))
        expect(twin, True)
        twin.close()
        for k, (y, yr) in enumerate(zip(want, yrs)):            # (1), once: every guarded run is bit-equal to this one
            assert y.size == np.size(yr), (entry, k, y.size, np.size(yr))
            if y.size:
                err = rel_err_per_tone(y.reshape(-1, ncol), np.asarray(yr).reshape(-1, ncol))
                assert err.max() <= TOL, (entry, k, float(err.max()))
        for tag, got in runs:
            for k, (y, w) in enumerate(zip(got, want)):
                assert y.size == w.size, (tag, k, y.size, w.size)
                same = y.view(np.int32) == w.view(np.int32)                                       # (3)
                if not same.all():
                    bad = np.flatnonzero(~same.reshape(-1, 2).all(axis=1))
                    raise AssertionError(f"{tag} buffer {k}: {bad.size} of {y.size} output samples differ from the "
                                         f"twin's (plain tensors), first at sample {bad[0]} (row {bad[0] // ncol}, "
                                         f"column {bad[0] % ncol}): {y[bad[0]]} against {w[bad[0]]}")


def clean_env(monkeypatch, env):
    """Only `env` of the engine switches is set (GSDR_LIB*, which pick the library itself, stay as they are)."""
    for k in [k for k in os.environ if k.startswith("GSDR_") and not k.startswith("GSDR_LIB")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


LDS_FFT = "Stockham FFT inside the LDS"          # describe()["family"] of the in-LDS TONES / NOISE kernels ...
BLUESTEIN = "Bluestein"                           # ... through Bluestein's identity


def expect_kernel(name, mac=None, rot=None, new=(), family=None, not_family=None):
    """-> expect(dem, ran): asserts the engine of a handle before its first call and after its last.  `name`: a kernel
    name or a tuple of admissible ones; `new`: names a handle may also report before its first launch (a handle names
    the kernel of its last launch, and the four-product pre-converted loop is chosen per launch); `family` /
    `not_family`: text describe()["family"] must / must not hold."""
    names = (name,) if isinstance(name, str) else tuple(name)

    def expect(dem, ran):
        d = dem.describe()
        assert dem.kernel_name in (names if ran else names + tuple(new)), (dem.kernel_name, names, ran, d)
        if mac is not None:
            assert (d["complex_mac"], d["rotation_blocks"]) == (mac, rot), (d, mac, rot)
        if family is not None:
            assert family in d["family"], (d["family"], family)
        if not_family is not None:
            assert not_family not in d["family"], (d["family"], not_family)
    return expect


_REFS = {}


def cached(key, build):
    """(xs, yrs) of a case, computed once per session and shared by the engines; never modified."""
    if key not in _REFS:
        xs, yrs = build()
        for a in list(xs) + list(yrs):
            a.flags.writeable = False
        _REFS[key] = (xs, yrs)
    return _REFS[key]


# ---------------------------------------------------------------------------
# DIRECT
# ---------------------------------------------------------------------------
_MF = {"GSDR_DDC_MFMA": "1", "GSDR_DDC_FEW": "0"}      # (GSDR_DDC_FEW=0: the forced engine, also where ddc_few_kernel
#                                                         would take the shape -- the C3 block)
_PRE = dict(_MF, GSDR_MFMA_ASM="4", GSDR_MFMA_PREC="1")
DIRECT_ENGINES = {
    # key: (environment, kernel, (complex_mac, rotation_blocks) or None)
    "default":  ({}, None, None),
    "flat":     ({"GSDR_DDC_MFMA": "0", "GSDR_DDC_PIPE": "1", "GSDR_DDC_K": "0"}, "ddc_flat_kernel", None),
    "simple16": ({"GSDR_DDC_MFMA": "0", "GSDR_DDC_PIPE": "0", "GSDR_DDC_K": "16"}, "ddc_kernel", None),
    "mfma":     (dict(_MF, GSDR_MFMA_ASM="2"), "ddc_mfma_ring_kernel", None),
    "mfma16":   (dict(_MF, GSDR_MFMA_ASM="4", GSDR_MFMA_PREC="0"), "ddc_mfma_ring16_kernel", None),
    "mfma16w8": (dict(_MF, GSDR_MFMA_ASM="5", GSDR_MFMA_PREC="0"), "ddc_mfma_ring16w8_kernel", None),
    "mfma16p":  (_PRE, P16, "by window"),
    "mfma_c":   (dict(_MF, GSDR_MFMA_ASM="0"), "ddc_mfma_kernel", None),
    "mac3":     (LOOPS["p3"][0], P16, (3, 1)),
    "mac3r2":   (LOOPS["p3r2"][0], P16, (3, 2)),
}
MATRIX_ENGINES = ("mfma", "mfma16", "mfma16w8", "mfma16p", "mfma_c", "mac3", "mac3r2")

# N, rate, M, F, L
S_LAST_ROW = (40, 1_000_000, 9, 4, 585)         # 65 rows: two full row tiles and a last tile of ONE row of 9 samples;
#                                                 the window of 36 samples ends 28 short of its second 32-sample block
S_N65 = (65, 10_000_000, 100, 4, 10_000)        # 100 rows (a last tile of 4), 65 tones, M * F = 400 = 12.5 blocks
S_ODD = (6, 1_000_000, 37, 5, 37_000)           # odd stride: every row but each fourth starts 8 bytes past 16; F = 5
S_C3 = (7, 200_000_000, 1000, 4, 50_000)        # the C3 block, 50 rows
S_TWO_ROWS = (5, 1000, 50, 4, 100)              # two rows, the carry (150 samples) longer than a buffer
DIRECT_SHAPES = [S_LAST_ROW, S_N65, S_ODD, S_C3, S_TWO_ROWS]

# Shapes an engine's chooser refuses (csrc/ddc_plan.h, gsdr_demod_create) run on the smallest shape it takes that
# keeps what the shape is there for:
#   matrix cores   the zero padding behind a window must fit one row stride, (M*F + 31)/32*32 - M*F <= M (middle rows
#                  read the caller's buffer in whole blocks), and a buffer holds the carry, L/M >= F - 1.
#                  S_LAST_ROW: with F = 4, M = 9 .. 12 leave 28 .. 16 > M; M = 13 is the shortest stride whose window
#                  (52 samples) still spills into a second block; 65 rows as before.
#                  S_TWO_ROWS: three rows, the carry exactly as long as a buffer.
#   ddc_flat       F <= 4: the odd stride with four tap phases.
REPLACED = {
    ("matrix", S_LAST_ROW): (40, 1_000_000, 13, 4, 845),
    ("matrix", S_TWO_ROWS): (5, 1000, 50, 4, 150),
    ("flat", S_ODD): (6, 1_000_000, 37, 4, 37_000),
}
# the library's own choice: the generic kernel where the matrix cores refuse, ddc_few_kernel for <= 32 tones at M >= 512
DEFAULT_KERNEL = {S_LAST_ROW: "ddc_kernel", S_N65: "ddc_mfma_ring16_kernel", S_ODD: "ddc_mfma_ring16_kernel",
                  S_C3: "ddc_few_kernel", S_TWO_ROWS: "ddc_kernel"}
# kMac3MinBlocks = kRot2MinBlocks (csrc/ddc_plan.h, read from gsdr_ddc_plan): a pre-converted handle left to itself takes
# three products and the pair rotation from windows of that many blocks


def direct_inputs(shape, oracle_mod):
    N, rate, M, F, L = shape

    def build():
        rng = np.random.default_rng(1000 + N + M + F + L)
        freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
        if N >= 3:
            freq[0], freq[1], freq[2] = 0, rate // 2 - 1, -(rate // 2) + 1
        ref = oracle_mod.Direct(freq, rate, M, F, L)
        xs = [crandn(rng, L) for _ in range(NBUF)]
        return xs + [freq], [ref.process(x) for x in xs]
    xs, yrs = cached(("direct", shape), build)
    return xs[-1], xs[:-1], yrs


@pytest.mark.parametrize("shape", DIRECT_SHAPES, ids=lambda c: "N%d_M%d_F%d_L%d" % (c[0], c[2], c[3], c[4]))
@pytest.mark.parametrize("engine", list(DIRECT_ENGINES))
def test_direct_extents(cuda_device, gsdr_lib, oracle_mod, monkeypatch, engine, shape):
    """Every DIRECT engine with decimation on every shape (or its replacement, REPLACED above)."""
    env, kernel, mac = DIRECT_ENGINES[engine]
    family = "matrix" if engine in MATRIX_ENGINES else engine
    if engine == "default":
        kernel = DEFAULT_KERNEL[shape]
    shape = REPLACED.get((family, shape), shape)
    N, rate, M, F, L = shape
    new = ()
    if mac == "by window":
        mac = (3, 2) if (M * F + 31) // 32 >= _ddc_plan.plan(gsdr_lib, N, M, F, L, env=env)["complex_mac_min_blocks"] else (4, 1)
        new = ("ddc_mfma_ring16_kernel",) if mac == (4, 1) else ()
    clean_env(monkeypatch, env)
    freq, xs, yrs = direct_inputs(shape, oracle_mod)
    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), expect_kernel(kernel, *(mac or ()), new=new), xs, yrs, N)


def test_direct_few_tones_extents(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """ddc_few_kernel on the smallest shape of test_direct_few_tones_long_decimation: two tones, blocks of 4096
    samples, two blocks per buffer behind three blocks of carry."""
    shape = (2, 200_000_000, 4096, 4, 8192)
    N, rate, M, F, L = shape
    clean_env(monkeypatch, {})
    freq, xs, yrs = direct_inputs(shape, oracle_mod)
    run_case(cuda_device, lambda: make_direct(freq, rate, M, F, L), expect_kernel("ddc_few_kernel"), xs, yrs, N)


@pytest.mark.parametrize("N,env,kernel", [(4, {}, "mix_few_kernel"), (20, {"GSDR_MIX_FEW": "0"}, "mix_small_kernel"),
                                          (40, {}, "mix_kernel")], ids=["few", "small", "wide"])
def test_direct_undecimated_extents(cuda_device, gsdr_lib, oracle_mod, monkeypatch, N, env, kernel):
    """decim == 0: N * L outputs, L = 4099 (a prime: no multiple of any tile); a lane per (sample, tone), several
    sample phases per wave (the older kernel for up to 32 tones, GSDR_MIX_FEW=0), a lane per tone."""
    shape = (N, 200_000_000, 0, 4, 4099)
    rate, L = shape[1], shape[4]
    clean_env(monkeypatch, env)
    freq, xs, yrs = direct_inputs(shape, oracle_mod)
    run_case(cuda_device, lambda: make_direct(freq, rate, 0, 4, L), expect_kernel(kernel), xs, yrs, N)


# ---------------------------------------------------------------------------
# TONES, NOISE
# ---------------------------------------------------------------------------
def tones_inputs(N, rate, nfft, avg, L, oracle_mod, on_bins):
    def build():
        rng = np.random.default_rng(2000 + nfft + avg)
        if on_bins:         # bin centres: every tone has a bin
            bins = rng.choice(np.arange(nfft), size=N, replace=False)
            freq = np.array([int((b if b < nfft // 2 else b - nfft) * (rate / nfft)) for b in bins])
        else:               # the tones of test_pfb_parity
            freq = rng.integers(-rate // 2 + 1, rate // 2, size=N)
            freq[0] = 0
        ref = oracle_mod.Pfb(freq, rate, nfft, avg, L)
        bins = ref.bins()
        assert (bins >= 0).all()
        xs = [crandn(rng, L) for _ in range(NBUF)]
        yrs = [np.array(ref.process(x)) for x in xs]
        assert sum(len(y) for y in yrs) > 0
        return xs + [freq, bins], yrs
    xs, yrs = cached(("tones", N, rate, nfft, avg, L), build)
    return xs[-2], xs[-1], xs[:-2], yrs


def run_tones(dev, expect, N, rate, nfft, avg, L, oracle_mod, on_bins=False):
    freq, bins, xs, yrs = tones_inputs(N, rate, nfft, avg, L, oracle_mod, on_bins)

    def make():
        dem = make_pfb(freq, rate, nfft, avg, L)
        np.testing.assert_array_equal(dem.bins(), bins)
        return dem
    run_case(dev, make, expect, xs, yrs, N)


TONES_SHAPE = (5, 200_000_000, 1000, 4, 50_123)     # nfft does not divide L: a carry of another length every call


@pytest.mark.parametrize("env,kernel,what", PFB_VARIANTS,
                         ids=["+".join(f"{k[9:]}={x}" for k, x in v[0].items()) or "default" for v in PFB_VARIANTS])
def test_tones_extents_every_pfb_variant(cuda_device, gsdr_lib, oracle_mod, monkeypatch, env, kernel, what):
    """TONES through filter + in-LDS FFT + bin selection, every variant of the kernels (PFB_VARIANTS of
    tests/test_gpu_parity.py).  Asserted: the kernel a switch forces, or one of the two in-LDS kernels where the
    library's choice stands, and the family text of describe() (in the LDS, not Bluestein).  How the filter is staged,
    the radix of the stages and the teams are variants INSIDE those two kernels: neither kernel_name nor describe()
    tells them apart, so for them only the family is asserted and the switch is trusted."""
    clean_env(monkeypatch, env)
    run_tones(cuda_device, expect_kernel(kernel or PFB_LDS_KERNELS, family=LDS_FFT, not_family=BLUESTEIN), *TONES_SHAPE,
              oracle_mod)


def test_tones_extents_bluestein(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """A prime frame: Bluestein's identity inside the LDS.  It runs under the run kernel's name; describe()["family"]
    says "Bluestein", and that is asserted."""
    clean_env(monkeypatch, {})
    run_tones(cuda_device, expect_kernel("pfb_cu_kernel", family=BLUESTEIN), 5, 200_000_000, 1021, 4, 50_123, oracle_mod, on_bins=True)


def test_tones_extents_long_frames(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """Frames above 8192 points: polyphase filter, FFT stages through memory, bin selection."""
    clean_env(monkeypatch, {})
    run_tones(cuda_device, expect_kernel("fft_pass_kernel", family="FFT behind the polyphase filter"), 5, 200_000_000, 12_000, 2, 100_000, oracle_mod, on_bins=True)


@pytest.mark.parametrize("engine", ["mfma16", "mac3r2"])
def test_tones_extents_on_the_ddc_kernels(cuda_device, gsdr_lib, oracle_mod, monkeypatch, engine):
    """Every selected bin as a DDC tone (GSDR_TONES_FFT=0): the rows read the handle's raw window, the staging pass
    reads the caller's buffer."""
    env, kernel, mac = DIRECT_ENGINES[engine]
    clean_env(monkeypatch, dict(env, GSDR_TONES_FFT="0"))
    run_tones(cuda_device, expect_kernel(kernel, *(mac or ())), *TONES_SHAPE, oracle_mod)


@pytest.mark.parametrize("nfft,avg,L", [(16, 3, 200), (1000, 4, 50_123)])
def test_noise_extents(cuda_device, gsdr_lib, oracle_mod, monkeypatch, nfft, avg, L):
    """NOISE: every bin of every frame, [frame][bin]."""
    import gpu_sdr_amd as g
    clean_env(monkeypatch, {})

    def build():
        rng = np.random.default_rng(4000 + nfft)
        ref = oracle_mod.Noise(nfft, avg, L)
        xs = [crandn(rng, L) for _ in range(NBUF)]
        return xs, [np.array(ref.process(x)) for x in xs]
    xs, yrs = cached(("noise", nfft, avg, L), build)
    p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft, freq=[0],
                wave_type=[g.w_type.NOISE])
    run_case(cuda_device, lambda: g.RX_buffer_demodulator(p, device_index=0), expect_kernel(PFB_LDS_KERNELS, family=LDS_FFT, not_family=BLUESTEIN),
             xs, yrs, nfft)


# ---------------------------------------------------------------------------
# CHIRP, NODSP
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row,kernel,form,parts", [(0, "chirp_demod_kernel", "plain", 1), (1, "chirp_lockin_kernel", "plain", 1),
                                                   (12, "chirp_lockin_kernel", "split", 20)],
                         ids=["undecimated_L5000", "ppt7_remainder2", "ppt20000_split"])
def test_chirp_extents(cuda_device, gsdr_lib, oracle_mod, monkeypatch, row, kernel, form, parts):
    """CHIRP_CASES of tests/test_gpu_parity.py: undecimated; 7 samples per point with 2 left over per buffer; 20 000
    samples per point, 1.5 points per buffer (chirp_lockin_split_kernel deals a point to several waves and
    chirp_lockin_sum_kernel adds their sums).  A handle reports all three lock-in kernels as chirp_lockin_kernel; which
    of them ran is in describe()["chirp_calls"]: every call of a handle took `form`, the third row's the split pair
    with 20 waves per point (80 stretches, four per wave)."""
    rate, f0, f1, steps, t, decim, L, _ = CHIRP_CASES[row]
    clean_env(monkeypatch, {})

    def build():
        rng = np.random.default_rng(3000 + steps + decim)
        ref = oracle_mod.Chirp(rate, f0, f1, steps, t, decim, L)
        xs = [crandn(rng, L) for _ in range(NBUF)]
        return xs, [np.array(ref.process(x)) for x in xs]
    xs, yrs = cached(("chirp", row), build)
    name = expect_kernel(kernel)

    def expect(dem, ran):
        name(dem, ran)
        d = dem.describe()
        want = dict({"plain": 0, "split": 0, "generic": 0}, **({form: len(xs)} if ran else {}))
        assert d["chirp_calls"] == want, (d["chirp_calls"], want)
        if ran:
            assert d["chirp_parts"] == parts and d["chirp_calls"][form] > 0, d
    run_case(cuda_device, lambda: make_chirp(rate, f0, f1, steps, t, decim, L), expect, xs, yrs, 1)


def test_nodsp_extents(cuda_device, gsdr_lib, monkeypatch):
    """NODSP: the buffer itself, bit for bit."""
    import gpu_sdr_amd as g
    L = 501
    clean_env(monkeypatch, {})
    rng = np.random.default_rng(501)
    xs = [crandn(rng, L) for _ in range(NBUF)]
    p = g.param(rate=1000, buffer_len=L, wave_type=[])
    run_case(cuda_device, lambda: g.RX_buffer_demodulator(p, device_index=0), expect_kernel("memcpy"), xs, xs, 1)
    dem = g.RX_buffer_demodulator(p, device_index=0)
    want = _feed(dem, "process", xs, cuda_device, *_plain(cuda_device))
    dem.close()
    for y, x in zip(want, xs):
        np.testing.assert_array_equal(y.view(np.int32), x.view(np.int32))


# ---------------------------------------------------------------------------
# writers: output guards only
# ---------------------------------------------------------------------------
WRITER_N = 5_003            # no multiple of 4, 64, 256 or 1024


def _check_writer(dev, fill_pairs):
    """fill_pairs: (out_off, fill) with fill(out, guarded) writing WRITER_N samples; called on a guarded view -- whose
    guards are checked before anything else is written -- and on a plain tensor: the two must agree bit for bit."""
    import torch
    for out_off, fill in fill_pairs:
        whole, view = guarded_output(WRITER_N, out_off, dev)
        fill(view, True)
        torch.cuda.synchronize()
        check_output(whole, view, WRITER_N)
        plain = torch.empty(WRITER_N, dtype=torch.complex64, device=dev)
        fill(plain, False)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(view.cpu().numpy().view(np.int32), plain.cpu().numpy().view(np.int32),
                                      err_msg=f"out_off {out_off}")


def test_tx_generator_tones_extents(cuda_device, gsdr_lib):
    """TX_buffer_generator TONES, 70 tones at 1 Msps: two generators in step, one writes plain tensors, one guarded
    views; consecutive buffers."""
    import gpu_sdr_amd as g
    rate = 1_000_000
    rng = np.random.default_rng(70)
    freq = [int(f) for f in rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=70, replace=False)]
    p = g.param(mode="TX", rate=rate, buffer_len=WRITER_N, freq=freq, ampl=[1.0 / 70] * 70, wave_type=[g.w_type.TONES] * 70)
    a, b = g.TX_buffer_generator(p), g.TX_buffer_generator(p)
    fill = lambda out, guarded: (b if guarded else a).get(out)
    _check_writer(cuda_device, [(0, fill), (1, fill), (1, fill), (0, fill)])
    a.close()
    b.close()


def test_tx_generator_chirp_extents(cuda_device, gsdr_lib):
    import gpu_sdr_amd as g
    p = g.param(mode="TX", rate=200_000_000, buffer_len=WRITER_N, freq=[-80_000_000], chirp_f=[80_000_000],
                swipe_s=[1000], chirp_t=[3.5e-5], ampl=[0.25], wave_type=[g.w_type.CHIRP])
    a, b = g.TX_buffer_generator(p), g.TX_buffer_generator(p)
    fill = lambda out, guarded: (b if guarded else a).get(out)
    _check_writer(cuda_device, [(0, fill), (1, fill), (1, fill), (0, fill)])
    a.close()
    b.close()


def test_device_tones_extents(cuda_device, gsdr_lib):
    from gpu_sdr_amd.source import device_tones, tone_comb
    rate = 1_000_000
    freq, ampl, phase = tone_comb(70, rate, seed=3)
    for sigma in (0.0, 1e-3):
        fill = lambda out, guarded: device_tones(out, rate - 2000, rate, freq, ampl, phase, sigma=sigma, seed=5)
        _check_writer(cuda_device, [(0, fill), (1, fill)])


def test_device_chirp_extents(cuda_device, gsdr_lib):
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import device_chirp
    cp = g.chirp_derive(200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5)
    fill = lambda out, guarded: device_chirp(out, 6500, cp, scale=0.5)
    _check_writer(cuda_device, [(0, fill), (1, fill)])
