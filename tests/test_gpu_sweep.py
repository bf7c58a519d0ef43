"""The sweep accumulator on the GPU (include/gsdr.h, "VNA sweep accumulator on the device"): the device against the host
twin (the same bits for means, variances and the phase slope) on every shape, under every cutting, with a first_row past
2^40; feeds longer than two passes and much shorter than one; reads in the middle of a stream; reset; the extents of what
a feed reads and a read writes; poison; empty feeds; a refused feed; a stream of the caller's; and a CHIRP handle's rows
fed buffer by buffer, for one chirp and for three in one handle, decimated and undecimated.

Measured figures (line delay, variance and mean against numpy in float64) are written to the file that
GSDR_SWEEP_MARGINS names, when it is set; profiles/sweep_margins.json is the committed copy."""
import json
import os

import numpy as np
import pytest

from _extents import check_input_untouched, check_output, guarded_input, guarded_output
from _margins import record_margin
from _sweep import GPU_SHAPES, cuttings, model, rows_of, run_device, run_host, same_bits, same_result, total_for

pytestmark = pytest.mark.gpu

SWEEP_MARGINS = {}


@pytest.fixture(scope="module")
def sweep(gsdr_lib):
    from gpu_sdr_amd import sweep
    yield sweep
    path = os.environ.get("GSDR_SWEEP_MARGINS")
    if SWEEP_MARGINS and path:
        doc = {"bars": {"line_delay": 1e-6, "variance": 1e-6, "mean_ulp": 1.0},
               "metric": "line_delay, variance: worst relative error against float64; mean_ulp: worst distance in float32 ulps from numpy.mean in float64",
               "per_case": dict(sorted(SWEEP_MARGINS.items()))}
        try:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1)
        except OSError:
            pass


def margin(label, value):
    SWEEP_MARGINS[label] = max(SWEEP_MARGINS.get(label, 0.0), float(value))
    record_margin(value, label)


_memo = {}


def case_of(shape):
    """The stream of a shape, made once and left unchanged."""
    if shape not in _memo:
        n_ch, n_points, group = shape
        _memo[shape] = rows_of(total_for(n_points, group), n_ch)
    return _memo[shape]


def ident(shape):
    return "x".join(map(str, shape))


@pytest.mark.parametrize("first_row", [0, (1 << 40) + 17])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=ident)
def test_device_equals_host_twin(sweep, cuda_device, shape, first_row):
    n_ch, n_points, group = shape
    x = case_of(shape)
    want = run_host(sweep, x, n_points, group, first_row)
    got = run_device(sweep, x, n_points, group, cuda_device, first_row)
    assert same_result(got, want), [same_bits(g, w) for g, w in zip(got[:3], want[:3])]
    assert np.array_equal(got[3], want[3]) and got[4] == want[4] == 2
    assert np.all(want[1].view(np.float32) >= 0) and np.count_nonzero(want[1].view(np.float32)) > want[1].size


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=ident)
def test_same_bits_under_every_cutting(sweep, cuda_device, shape):
    """Among them one feed longer than two passes ("long") and single rows."""
    n_ch, n_points, group = shape
    x = case_of(shape)
    want = run_host(sweep, x, n_points, group, 3)
    for name, cut in cuttings(x.shape[0], n_points * group).items():
        got = run_device(sweep, x, n_points, group, cuda_device, 3, cut)
        assert same_result(got, want), (name, [same_bits(g, w) for g, w in zip(got[:3], want[:3])])


def test_feeds_much_shorter_than_a_sweep(sweep, cuda_device):
    n_ch, n_points, group = 16, 1000, 1
    x = case_of((n_ch, n_points, group))
    cut = [min(37, x.shape[0] - at) for at in range(0, x.shape[0], 37)]
    assert same_result(run_device(sweep, x, n_points, group, cuda_device, (1 << 40) + 17, cut), run_host(sweep, x, n_points, group, (1 << 40) + 17))


def test_reads_in_the_middle_and_reset(sweep, cuda_device):
    """Reads and slopes between the feeds leave the later bits alone; after reset() the object gives what a fresh one
    gives, with the new first_row."""
    import torch
    n_ch, n_points, group = 3, 67, 1
    x = case_of((n_ch, n_points, group))
    xd = torch.from_numpy(x).to(cuda_device)
    mean_d = torch.zeros((n_points, n_ch), dtype=torch.complex64, device=cuda_device)
    s = sweep.device_sweep(n_ch, n_points, group, 0, device_index=0)
    s.feed_device(xd[:50])
    torch.cuda.synchronize()
    s.reset(3)
    assert s.rows_seen == 0 and s.sweeps == 0
    for at in range(0, x.shape[0], 30):
        s.feed_device(xd[at:at + 30])
        if at % 90 == 0:
            part = s.read(variance=True) + (s.slope(),)
            assert same_result(part, run_host(sweep, x[:at + 30], n_points, group, 3)), at
        s.read_device(mean_d)
    got = s.read(variance=True) + (s.slope(),)
    torch.cuda.synchronize()
    want = run_host(sweep, x, n_points, group, 3)
    assert same_result(got, want) and same_bits(mean_d.cpu().numpy(), want[0])
    assert np.array_equal(s.counts(), want[3]) and s.sweeps == want[4]
    s.close()


@pytest.mark.parametrize("pattern,off", [("nan", 1), ("huge", 0)])
@pytest.mark.parametrize("shape", [(3, 67, 1), (1030, 3, 1), (2, 250, 40), (1, 7, 3)], ids=ident)
def test_extents_and_alignment(sweep, gsdr_lib, cuda_device, shape, pattern, off):
    """Input in the middle of a larger allocation, 8 bytes past a 16-byte boundary or on it: the feed reads
    rows_dev[0, n_rows n_ch) only (a guard that reached a sum would show) and leaves the input as it was; a read writes
    mean_dev and var_dev to exactly their extents.  Two feeds, so that the second goes on from carried sums."""
    import torch
    n_ch, n_points, group = shape
    x = case_of(shape)
    rows = x.shape[0]
    want = run_host(sweep, x, n_points, group, 3)
    s = sweep.device_sweep(n_ch, n_points, group, 3, device_index=0)
    at = 0
    for n in (rows // 3 + 1, rows - rows // 3 - 1):
        part = x[at:at + n]
        whole_in, view_in = guarded_input(part.reshape(-1), off, pattern, cuda_device)
        assert gsdr_lib.gsdr_sweep_feed_device(s._h, view_in.data_ptr(), n, None) == 0
        torch.cuda.synchronize()
        check_input_untouched(whole_in, part.reshape(-1), off, pattern)
        at += n
    cells = n_points * n_ch
    whole_m, view_m = guarded_output(cells, 1 - off, cuda_device)
    whole_v, view_v = guarded_output(cells, off, cuda_device)
    assert gsdr_lib.gsdr_sweep_read_device(s._h, view_m.data_ptr(), view_v.data_ptr(), None) == 0
    torch.cuda.synchronize()
    check_output(whole_m, view_m, cells), check_output(whole_v, view_v, cells)
    assert same_bits(view_m.cpu().numpy().reshape(n_points, n_ch), want[0]) and same_bits(view_v.cpu().numpy().reshape(n_points, n_ch), want[1])
    whole_m, view_m = guarded_output(cells, off, cuda_device)
    assert gsdr_lib.gsdr_sweep_read_device(s._h, view_m.data_ptr(), None, None) == 0          # without the variance
    torch.cuda.synchronize()
    check_output(whole_m, view_m, cells)
    assert same_bits(view_m.cpu().numpy().reshape(n_points, n_ch), want[0]) and same_bits(s.slope(), want[2])
    s.close()


def test_poison_reaches_exactly_its_accumulators(sweep, cuda_device):
    for shape in ((3, 67, 1), (70, 25, 4)):
        n_ch, n_points, group = shape
        total = total_for(n_points, group)
        x = rows_of(total, n_ch, seed=21)
        clean = run_device(sweep, x, n_points, group, cuda_device, 3)
        bad = x.copy()
        r_inf, r_nan = total // 3, total // 2
        bad[r_inf, 1] = np.complex64(complex(np.inf, 0.0))
        bad[r_nan, 0] = np.complex64(complex(0.0, np.nan))
        p_inf, p_nan = ((3 + r_inf) // group) % n_points, ((3 + r_nan) // group) % n_points
        hit = np.zeros((n_points, n_ch), dtype=bool)
        hit[p_inf, 1] = hit[p_nan, 0] = True
        for cut in (None, cuttings(total, n_points * group)["sevens"]):
            got = run_device(sweep, bad, n_points, group, cuda_device, 3, cut)
            for k in (0, 1):
                assert same_bits(got[k][~hit], clean[k][~hit])
                assert np.array_equal(~np.isfinite(got[k].real) | ~np.isfinite(got[k].imag), hit)
            assert np.isnan(got[1][p_inf, 1].real) and np.isnan(got[1][p_nan, 0].imag)          # NaN stays NaN
            assert not np.isfinite(got[2][0]) and not np.isfinite(got[2][1])
            assert all(same_bits(got[2][c], clean[2][c]) for c in range(2, n_ch))
            twin = run_host(sweep, bad, n_points, group, 3)
            assert same_bits(got[0][~hit], twin[0][~hit]) and same_bits(got[1][~hit], twin[1][~hit])


def test_empty_feeds_and_a_refused_feed(sweep, gsdr_lib, cuda_device):
    import torch
    from gpu_sdr_amd import GsdrError
    n_ch, n_points, group = 3, 67, 1
    x = case_of((n_ch, n_points, group))
    xd = torch.from_numpy(x).to(cuda_device)
    s = sweep.device_sweep(n_ch, n_points, group, 0, device_index=0)
    assert gsdr_lib.gsdr_sweep_feed_device(s._h, None, 0, None) == 0                 # touches no pointer
    s.feed_device(xd[:40])
    s.feed_device(xd[:0])
    assert s.rows_seen == 40
    for n in (-1, (1 << 24) + 1):
        assert gsdr_lib.gsdr_sweep_feed_device(s._h, xd.data_ptr(), n, None) == -1
        assert "gsdr_sweep_feed_device: n_rows" in gsdr_lib.gsdr_last_error(None).decode()
    assert gsdr_lib.gsdr_sweep_feed_device(s._h, None, 5, None) == -1 and "null buffer: rows_dev" in gsdr_lib.gsdr_last_error(None).decode()
    assert gsdr_lib.gsdr_sweep_read_device(s._h, None, None, None) == -1 and "null buffer: mean_dev" in gsdr_lib.gsdr_last_error(None).decode()
    with pytest.raises(GsdrError, match="a device object takes gsdr_sweep_feed_device"):
        if gsdr_lib.gsdr_sweep_feed_host(s._h, x.ctypes.data, 1) != 0:
            s._fail()
    m = np.zeros((n_points, n_ch), dtype=np.complex64)
    assert gsdr_lib.gsdr_sweep_read_host(s._h, m.ctypes.data, None) == -1
    assert s.rows_seen == 40                              # the state is as it was
    s.feed_device(xd[40:])
    got = s.read(variance=True) + (s.slope(),)
    s.close()
    assert same_result(got, run_host(sweep, x, n_points, group, 0))


def test_on_a_stream_of_the_callers(sweep, cuda_device):
    import torch
    shape = (4, 200, 64)
    x = case_of(shape)
    got = run_device(sweep, x, shape[1], shape[2], cuda_device, 3, cuttings(x.shape[0], shape[1] * shape[2])["gaps"], stream=torch.cuda.Stream())
    assert same_result(got, run_host(sweep, x, shape[1], shape[2], 3))


@pytest.mark.parametrize("n_points,f_step,tau", [(1000, 200.0, 250e-6), (67, 10e3, 3e-6)])
def test_line_delay_on_the_device(sweep, cuda_device, n_points, f_step, tau):
    f = 1e6 + f_step * np.arange(n_points)
    one = (0.7 * np.exp(-2j * np.pi * f * tau)).astype(np.complex64)
    x = np.tile(np.stack([one, one.conj()], axis=1), (3, 1))
    import torch
    s = sweep.device_sweep(2, n_points, 1, 0, device_index=0)
    s.feed_device(torch.from_numpy(x).to(cuda_device))
    got = s.line_delay(f_step)
    s.close()
    rel = np.abs(got - np.array([tau, -tau])) / tau
    margin(f"line_delay {n_points} points", rel.max())
    assert rel.max() <= 1e-6, rel


def test_variance_against_numpy_on_the_device(sweep, cuda_device):
    import torch
    n_ch, n_points, n = 4, 50, 64
    rng = np.random.default_rng(77)
    carrier = (0.5 + 0.1 * np.arange(n_ch)) * np.exp(1j * np.arange(n_ch))
    z = carrier[None, None, :] * (1 + 1e-3 * (rng.standard_normal((n, n_points, n_ch)) + 1j * rng.standard_normal((n, n_points, n_ch))))
    x = z.astype(np.complex64)
    s = sweep.device_sweep(n_ch, n_points, 1, 0, device_index=0)
    s.feed_device(torch.from_numpy(x.reshape(-1, n_ch)).to(cuda_device))
    mean, var = s.read(variance=True)
    s.close()
    x64 = x.astype(np.complex128)
    for got, part in ((var.real, x64.real), (var.imag, x64.imag)):
        want = np.var(part, axis=0, ddof=1)
        rel = np.abs(got - want) / want
        margin("variance n = 64", rel.max())
        assert rel.max() <= 1e-6, rel.max()


# ---- end to end: a CHIRP handle's rows, buffer by buffer --------------------------------------------------------------
RATE, STEPS, LENGTH, CHIRP_T, BUF, NBUF, SWEEPS = 1_000_000, 250, 40, 0.01, 12_500, 8, 10
BANDS = [(-450_000, -250_000), (100_000, -100_000), (250_000, 450_000)]        # the middle one sweeps downwards
DIP_AT = [61, 140, 203]                                                        # point next to which each band's dip sits


def ulps_apart(a, b):
    """distance of two float32 arrays in units of the spacing at the larger magnitude"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


@pytest.mark.parametrize("C", [1, 3])
def test_chirp_handle_into_a_device_sweep(sweep, cuda_device, C):
    """250 points x 40 samples, period 10 000, buffers of 12 500: 40 does not divide 12 500, so the buffers cut points and
    sweeps; 8 buffers are 10 sweeps.  The input: each band's own TX chirp times an S21 with a Lorentzian dip, summed, plus
    noise at 1e-3.  The lock-in's rows (decim 1) go into a device_sweep of group 1, the samples of a decim 0 handle into
    one of group 40, buffer by buffer on one stream."""
    import torch
    import gpu_sdr_amd as g
    bands = BANDS[:C]
    cp = g.chirp_derive(RATE, bands[0][0], bands[0][1], STEPS, CHIRP_T)
    assert (cp.num_steps, cp.length) == (STEPS, LENGTH) and (BUF % LENGTH, NBUF * BUF) == (20, SWEEPS * STEPS * LENGTH)
    assert sweep.sweep_shape(RATE, bands[0][0], bands[0][1], STEPS, CHIRP_T, 1) == (STEPS, 1)
    assert sweep.sweep_shape(RATE, bands[0][0], bands[0][1], STEPS, CHIRP_T, 0) == (STEPS, LENGTH)
    # S21 per band on its axis: a dip of depth 0.9 and half width 1.5 points, 0.3 points off the grid
    axes = [sweep.vna_axis(RATE, f0, f1, STEPS, STEPS) for f0, f1 in bands]
    s21 = []
    for c, ax in enumerate(axes):
        step = ax[1] - ax[0]
        fr = ax[DIP_AT[c]] + 0.3 * step
        s21.append(torch.from_numpy((1.0 - 0.9 / (1.0 + 1j * (ax - fr) / (1.5 * abs(step)))).astype(np.complex64)).to(cuda_device))
    gens = [g.TX_buffer_generator(g.param(mode="TX", rate=RATE, buffer_len=BUF, freq=[f0], chirp_f=[f1], swipe_s=[STEPS], chirp_t=[CHIRP_T],
                                          ampl=[0.25], wave_type=[g.w_type.CHIRP]), device_index=0) for f0, f1 in bands]

    def handle(decim):
        return g.RX_buffer_demodulator(g.param(mode="RX", rate=RATE, buffer_len=BUF, decim=decim, freq=[b[0] for b in bands],
                                               chirp_f=[b[1] for b in bands], swipe_s=[STEPS], chirp_t=[CHIRP_T],
                                               wave_type=[g.w_type.CHIRP] * C), device_index=0, multi_chirp=C > 1)
    dem1, dem0 = handle(1), handle(0)
    sw1 = sweep.device_sweep(C, STEPS, 1, 0, device_index=0)
    sw0 = sweep.device_sweep(C, STEPS, LENGTH, 0, device_index=0)
    rng = np.random.default_rng(100 + C)
    stream = torch.cuda.Stream()
    tmp = torch.empty(BUF, dtype=torch.complex64, device=cuda_device)
    outs1, outs0 = [], []
    for b in range(NBUF):
        point = torch.from_numpy(((b * BUF + np.arange(BUF)) % (STEPS * LENGTH)) // LENGTH).to(cuda_device)
        noise = 1e-3 * (rng.standard_normal(BUF) + 1j * rng.standard_normal(BUF))
        x = torch.from_numpy(noise.astype(np.complex64)).to(cuda_device)
        for c in range(C):
            gens[c].get(tmp)
            x += tmp * s21[c][point]
        out1 = torch.empty(dem1.out_capacity, dtype=torch.complex64, device=cuda_device)
        out0 = torch.empty(dem0.out_capacity, dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        n1 = dem1.process_device(x, out1, stream=stream)
        sw1.feed_device(out1[:n1], stream=stream)
        n0 = dem0.process_device(x, out0, stream=stream)
        sw0.feed_device(out0[:n0], stream=stream)
        assert n1 % C == 0 and n1 // C in (BUF // LENGTH, BUF // LENGTH + 1) and n0 == BUF * C
        outs1.append(out1[:n1]), outs0.append(out0[:n0])
    mean1, var1 = sw1.read(variance=True, stream=stream)
    mean0 = sw0.read(stream=stream)
    d1 = sw1.slope(stream=stream)
    z1 = np.concatenate([o.cpu().numpy() for o in outs1]).reshape(-1, C)
    z0 = np.concatenate([o.cpu().numpy() for o in outs0]).reshape(-1, C)
    assert z1.shape == (SWEEPS * STEPS, C) and z0.shape == (SWEEPS * STEPS * LENGTH, C)
    assert sw1.sweeps == SWEEPS and np.array_equal(sw1.counts(), np.full(STEPS, SWEEPS))
    assert sw0.sweeps == SWEEPS and np.array_equal(sw0.counts(), np.full(STEPS, SWEEPS * LENGTH))
    for h in gens + [dem1, dem0, sw1, sw0]:
        h.close()
    # the model on the handle's own rows, bit for bit
    want1, want0 = model(z1, STEPS, 1, 0), model(z0, STEPS, LENGTH, 0)
    assert same_bits(mean1, want1[0]) and same_bits(var1, want1[1]) and same_bits(d1, want1[2])
    assert same_bits(mean0, want0[0])
    # what VNA_analysis computes: numpy.mean over the sweeps in float64
    ref = np.mean(np.split(z1.astype(np.complex128), SWEEPS), axis=0)
    apart = max(ulps_apart(mean1.real, ref.real.astype(np.float32)).max(), ulps_apart(mean1.imag, ref.imag.astype(np.float32)).max())
    margin(f"mean_ulp C = {C}", apart)
    assert apart <= 1.0, apart
    ref0 = np.mean(np.mean(np.split(z0.astype(np.complex128), SWEEPS), axis=0).reshape(STEPS, LENGTH, C), axis=1)
    assert max(ulps_apart(mean0.real, ref0.real.astype(np.float32)).max(), ulps_apart(mean0.imag, ref0.imag.astype(np.float32)).max()) <= 1.0
    # each band shows its dip within one point of its place on the axis
    for c, ax in enumerate(axes):
        at = int(np.argmin(np.abs(mean1[:, c])))
        assert abs(at - DIP_AT[c]) <= 1 and abs(ax[at] - ax[DIP_AT[c]]) <= abs(ax[1] - ax[0]), (c, at)
        assert np.abs(mean1[at, c]) < 0.1 and np.median(np.abs(mean1[:, c])) > 0.2
