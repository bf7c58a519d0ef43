"""Several chirps demodulated in one pass (GSDR_CREATE_MULTI_CHIRP, RX side) on the GPU: every column against the
CPU oracle of its chirp, against a single-CHIRP handle, and the properties of the entries (streaming, pipeline, sc16,
rehearsal, extents).  Shapes are CHIRP_CASES of tests/test_gpu_parity.py, one per kernel form and edge.

Bar: per column ||y - y_ref||_2 / ||y_ref||_2 <= TOL of tests/test_gpu_parity.py, and exact equality of every length.
"""
import json
import os

import numpy as np
import pytest

import _extents as ex
from _margins import record_info
from test_gpu_parity import TOL, crandn, rel_err_per_tone, run_device, run_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = 4                      # kChirpGroup of csrc/ddc_kernels.h: the lock-in kernels are instantiated for whole groups
LOCKIN, DEMOD = "chirp_multi_lockin_kernel", "chirp_multi_demod_kernel"

SHAPES = {
    # name: (rate, steps, chirp_t, decim, L)
    "undecimated": (200_000_000, 1000, 3.5e-5, 0, 5000),
    "ppt7_remainder2": (200_000_000, 1000, 3.5e-5, 1, 5000),
    "ppt3_length1": (1_000_000, 10, 1e-5, 3, 1000),
    "ppt300_carry": (200_000_000, 1_000_000, 1.5, 1, 50_000),
    "length600_ppt1800": (200_000_000, 1000, 3e-3, 3, 50_000),
    "generic_lockin": (200_000_000, 1_000_000, 30.0, 1, 20_000),
    "generic_undecimated": (200_000_000, 1_000_000, 30.0, 0, 20_000),
    "split_1p5_points": (10_000_000, 50, 0.05, 2, 30_000),
    "split_one_point": (20_000_000, 100, 1.0, 1, 200_000),
}
NBUF = 3
# describe()["chirp_calls"] / ["chirp_parts"]: the lock-in form every call of a shape takes (csrc/chirp_plan.h), and the
# waves per point of the split shapes -- 80 stretches in parts of four; 782 stretches, 195 waves wanted, in parts of five
# -- for every number of chirps up to 16 (the partial sums of one or two points fit the buffer 512 times over)
SPLIT_PARTS = {"split_1p5_points": 20, "split_one_point": 157}


def form_of(shape):
    return "split" if shape.startswith("split_") else "generic" if shape.startswith("generic_") else "plain"


def assert_forms(dem, shape, calls):
    d = dem.describe()
    want = dict({"plain": 0, "split": 0, "generic": 0}, **{form_of(shape): calls})
    assert d["chirp_calls"] == want, (shape, d["chirp_calls"], want)
    assert d["chirp_calls"][form_of(shape)] > 0
    assert d["chirp_parts"] == SPLIT_PARTS.get(shape, 1), (shape, d["chirp_parts"])


def spans(rate, n=16):
    """(freq, chirp_f) of up to 16 chirps: an upward sweep, a downward one (wrapping chirpness), a zero-span chirp, a
    copy of chirp 0, then distinct random spans.  Every set of C chirps is the first C of these."""
    rng = np.random.default_rng(rate % 9973)
    s = [(-(rate * 9) // 20, (rate * 9) // 20), (rate // 4, -(rate // 4)), (rate // 10, rate // 10), (-(rate * 9) // 20, (rate * 9) // 20)]
    while len(s) < 16:
        f0, f1 = (int(v) for v in rng.integers(-rate // 2 + 1, rate // 2, size=2))
        if (f0, f1) not in s:
            s.append((f0, f1))
    return s[:n]


def make_multi(shape, sp, L=None, multi=True):
    import gpu_sdr_amd as g
    rate, steps, t, decim, L0 = SHAPES[shape]
    p = g.param(mode="RX", rate=rate, buffer_len=L or L0, decim=decim, freq=[s[0] for s in sp], chirp_f=[s[1] for s in sp],
                swipe_s=[steps], chirp_t=[t], wave_type=[g.w_type.CHIRP] * len(sp))
    return g.RX_buffer_demodulator(p, device_index=0, multi_chirp=multi)


_REFERENCE = {}


def reference(oracle_mod, shape):
    """The buffers of a shape and, per chirp of spans() and per buffer, what the oracle returns: made once."""
    if shape not in _REFERENCE:
        rate, steps, t, decim, L = SHAPES[shape]
        rng = np.random.default_rng(5000 + steps + decim)
        xs = [crandn(rng, L) for _ in range(NBUF)]
        cols = []
        for f0, f1 in spans(rate):
            ref = oracle_mod.Chirp(rate, f0, f1, steps, t, decim, L)
            cols.append([np.array(ref.process(x)) for x in xs])
            ref.close()
        _REFERENCE[shape] = (xs, cols)
    return _REFERENCE[shape]


@pytest.mark.parametrize("C", [2, GROUP - 1, GROUP, GROUP + 1, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_multichirp_parity(cuda_device, gsdr_lib, oracle_mod, shape, C):
    rate, steps, t, decim, L = SHAPES[shape]
    xs, cols = reference(oracle_mod, shape)
    dem = make_multi(shape, spans(rate, C))
    assert dem.channels == C and dem.describe()["chirps"] == C
    assert dem.kernel_name == (LOCKIN if decim else DEMOD)
    for b, x in enumerate(xs):
        y = (run_host if b % 2 else run_device)(dem, x, *(() if b % 2 else (cuda_device,)))
        rows = len(cols[0][b])
        assert y.size == rows * C and y.size <= dem.out_capacity, (b, y.size, rows)
        assert all(len(cols[c][b]) == rows for c in range(C))
        assert dem.kernel_name == (LOCKIN if decim else DEMOD)
        y = y.reshape(rows, C)
        yr = np.stack([cols[c][b] for c in range(C)], axis=1)
        err = rel_err_per_tone(y, yr)
        assert err.max() <= TOL, (shape, C, b, err.tolist())
        if C >= 4:          # chirp 3 is chirp 0 again
            assert np.array_equal(y[:, 0].copy().view(np.int32), y[:, 3].copy().view(np.int32))
    assert dem.out_capacity == ((L // (dem.window().size) + 1) * C if decim else L * C)
    assert_forms(dem, shape, len(xs))
    dem.close()


def _margin_file(update):
    """Keeps profiles/multichirp_margins.json at what this run measured; a run that measures what is recorded there
    leaves the file alone."""
    path = os.path.join(ROOT, "profiles", "multichirp_margins.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        doc = dict(old)
        doc.update(update)
        if doc != old:
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


@pytest.mark.parametrize("shape", ["ppt300_carry", "split_1p5_points"])
def test_multichirp_equals_single_chirp_handles(cuda_device, gsdr_lib, shape):
    """Column c of a five-chirp handle against a single-CHIRP handle for chirp c on the same buffers: the same lengths,
    call by call, and the same values BIT FOR BIT.  (The arithmetic of a column is that of the single-chirp kernels;
    whether the compiler contracts it alike in both kernels is its own decision, so this was first measured within TOL:
    the largest deviation, recorded in profiles/multichirp_margins.json, is 0 on both shapes.)"""
    rate, steps, t, decim, L = SHAPES[shape]
    C = 5
    sp = spans(rate, C)
    rng = np.random.default_rng(77)
    multi = make_multi(shape, sp)
    singles = [make_multi(shape, [s], multi=False) for s in sp]
    assert all(s.kernel_name == "chirp_lockin_kernel" for s in singles) and multi.kernel_name == LOCKIN
    worst, same_bits = 0.0, True
    for b in range(4):
        x = crandn(rng, L)
        y = run_device(multi, x, cuda_device)
        ys = [run_device(s, x, cuda_device) for s in singles]
        assert all(len(v) * C == y.size for v in ys), (b, y.size, [len(v) for v in ys])
        if y.size:
            y = y.reshape(-1, C)
            yr = np.stack(ys, axis=1)
            worst = max(worst, float(rel_err_per_tone(y, yr).max()))
            same_bits = same_bits and np.array_equal(y.view(np.int32), yr.view(np.int32))
    for h in [multi] + singles:
        assert_forms(h, shape, 4)
    multi.close()
    for s in singles:
        s.close()
    print(f"multichirp vs single-chirp handles, {shape}: largest deviation {worst:.3e}, same bits {same_bits}")
    record_info(worst, "largest deviation from the single-chirp handles")
    _margin_file({shape: {"chirps": C, "buffers": 4, "largest_relative_deviation_from_single_chirp_handles": worst,
                          "same_bits": bool(same_bits)}})
    assert worst <= TOL, (shape, worst)
    assert same_bits, (shape, worst)


def test_multichirp_streaming_equals_one_long_buffer(cuda_device, gsdr_lib):
    """L = 5000 at 7 samples per point leaves 2 samples over per call: four calls give the points of one call on the
    concatenation (lengths sum exactly; the values within TOL -- the windows are the same, the kernels too)."""
    rate = SHAPES["ppt7_remainder2"][0]
    sp = spans(rate, 3)
    rng = np.random.default_rng(11)
    x = crandn(rng, 20_000)
    short, long_ = make_multi("ppt7_remainder2", sp), make_multi("ppt7_remainder2", sp, L=20_000)
    parts = [run_device(short, x[k * 5000:(k + 1) * 5000], cuda_device) for k in range(4)]
    whole = run_device(long_, x, cuda_device)
    assert sum(len(p) for p in parts) == len(whole) == (20_000 // 7) * 3
    assert [len(p) for p in parts] == [714 * 3, 714 * 3, 714 * 3, 715 * 3]
    assert rel_err_per_tone(np.concatenate(parts).reshape(-1, 3), whole.reshape(-1, 3)).max() <= TOL
    short.close()
    long_.close()


@pytest.mark.parametrize("shape", ["ppt7_remainder2", "split_1p5_points", "undecimated"])
def test_multichirp_entries_give_the_same_bits(cuda_device, gsdr_lib, shape):
    """submit / wait, submit_device and the sc16 forms against process_device on a twin handle, bit for bit; sc16 input
    is widen-then-complex64; a rehearsed handle (prepare with REHEARSE | PIPELINE) starts from the same state as an
    unprepared twin."""
    import torch
    from gpu_sdr_amd import widen_sc16
    rate, steps, t, decim, L = SHAPES[shape]
    sp = spans(rate, 3)
    rng = np.random.default_rng(31)
    x16 = [rng.integers(-20_000, 20_000, size=(L, 2)).astype(np.int16) for _ in range(4)]
    xs = [widen_sc16(v) for v in x16]
    twin = make_multi(shape, sp)
    want = [run_device(twin, x, cuda_device) for x in xs]
    twin.close()

    def bits(a):
        return np.ascontiguousarray(a).view(np.int32)

    # host pipeline
    a = make_multi(shape, sp)
    a.prepare(host=False, pipeline=True, pipeline_host=False, rehearse=True)     # REHEARSE | PIPELINE
    pinned_in = [torch.from_numpy(x).pin_memory().numpy() for x in xs]
    outs = [torch.empty(a.out_capacity, dtype=torch.complex64).pin_memory().numpy() for _ in xs]
    for k, o in enumerate(outs):
        a.submit(x16[k] if k % 2 else pinned_in[k], o)       # gsdr_demod_submit_sc16 and gsdr_demod_submit in turn
    got = [o[:a.wait()].copy() for o in outs]
    assert [len(v) for v in got] == [len(v) for v in want]
    assert all(np.array_equal(bits(v), bits(w)) for v, w in zip(got, want))
    a.close()
    # device pipeline, complex64 and sc16 in turn
    b = make_multi(shape, sp)
    d_out = [torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in xs]
    d_in = [torch.from_numpy(x16[k] if k % 2 else xs[k]).to(cuda_device) for k in range(4)]
    torch.cuda.synchronize()
    for x, o in zip(d_in, d_out):
        b.submit_device(x, o)
    got = [o[:b.wait()].cpu().numpy() for o in d_out]
    assert all(np.array_equal(bits(v), bits(w)) for v, w in zip(got, want))
    b.close()
    # the in-order sc16 entries, host and device
    c = make_multi(shape, sp)
    for k in range(4):
        out = np.empty(c.out_capacity, dtype=np.complex64)
        if k % 2:
            n = c.process(x16[k], out)
            y = out[:n]
        else:
            o = torch.empty(c.out_capacity, dtype=torch.complex64, device=cuda_device)
            n = c.process(torch.from_numpy(x16[k]).to(cuda_device), o)
            torch.cuda.synchronize()
            y = o[:n].cpu().numpy()
        assert np.array_equal(bits(y), bits(want[k])), (shape, k)
    c.close()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("pattern", ex.PATTERNS)
@pytest.mark.parametrize("shape", ["ppt7_remainder2", "split_1p5_points", "undecimated"])
def test_multichirp_extents(cuda_device, gsdr_lib, shape, pattern, off):
    """Buffers in the middle of larger allocations, 0 or 1 sample past 16 bytes: exactly buffer_len samples are read,
    only out_dev[0, capacity) is written, and the output is bit for bit that of a call on buffers of their own."""
    import torch
    rate, steps, t, decim, L = SHAPES[shape]
    sp = spans(rate, 3)
    rng = np.random.default_rng(41)
    plain, guarded = make_multi(shape, sp), make_multi(shape, sp)
    cap = guarded.out_capacity
    for b in range(2):
        x = crandn(rng, L)
        want = run_device(plain, x, cuda_device)
        win, vin = ex.guarded_input(x, off, pattern, cuda_device)
        wout, vout = ex.guarded_output(cap, off, cuda_device)
        n = guarded.process_device(vin, vout)
        torch.cuda.synchronize()
        ex.check_output(wout, vout, n)
        ex.check_input_untouched(win, x, off, pattern)
        assert n == want.size
        assert np.array_equal(vout[:n].cpu().numpy().view(np.int32), want.view(np.int32)), (shape, pattern, off, b)
    plain.close()
    guarded.close()


@pytest.mark.parametrize("shape", ["ppt300_carry", "undecimated", "split_1p5_points"])
def test_one_chirp_with_the_flag_is_the_single_chirp_handle(cuda_device, gsdr_lib, shape):
    rate, steps, t, decim, L = SHAPES[shape]
    sp = spans(rate, 1)
    flagged, plain = make_multi(shape, sp, multi=True), make_multi(shape, sp, multi=False)
    assert flagged.kernel_name == plain.kernel_name == ("chirp_lockin_kernel" if decim else "chirp_demod_kernel")
    assert flagged.out_capacity == plain.out_capacity and flagged.channels == 1
    rng = np.random.default_rng(51)
    for b in range(3):
        x = crandn(rng, L)
        ya, yb = run_device(flagged, x, cuda_device), run_device(plain, x, cuda_device)
        assert np.array_equal(ya.view(np.int32), yb.view(np.int32))
    assert_forms(flagged, shape, 3)
    assert_forms(plain, shape, 3)
    flagged.close()
    plain.close()


def test_frame_average_stays_refused(cuda_device, gsdr_lib):
    import gpu_sdr_amd as g
    dem = make_multi("ppt7_remainder2", spans(200_000_000, 3))
    with pytest.raises(g.GsdrError):
        dem.set_frame_average(2)
    dem.close()
