"""sc16 output on the GPU (include/gsdr.h, "sc16 output"): every sc16 entry of the TX side writes exactly the bits that
narrowing the output of its complex64 entry gives -- the narrowing kernel against gsdr_narrow_sc16_host, the tone comb
and the chirp generator against the narrowed output of their complex64 kernels, TX_buffer_generator against a twin that
only uses get(), with the clipped counters against numpy's counts -- and the loop TX sc16 -> RX sc16 against the oracle.
Destinations are views 0 .. 3 samples into an allocation filled with a canary: what lies in front of the n samples and
64 samples behind them must survive."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import CHIRP_CASES, TOL, make_direct, rel_err_per_tone
from test_sc16_tx_host import all_values, narrow_model

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A


def canary_dst(n, d_off, dev):
    """(allocation, view of n samples that starts d_off samples in): int16 (.., 2), everything set to the canary"""
    import torch
    dst = torch.full((d_off + n + 64, 2), CANARY, dtype=torch.int16, device=dev)
    assert dst.data_ptr() % 16 == 0
    return dst, dst[d_off:d_off + n]


def check_canary(dst, n, d_off, want, msg):
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[d_off:d_off + n], want, err_msg=str(msg))
    assert (got[:d_off] == CANARY).all() and (got[d_off + n:] == CANARY).all(), msg


# ---------------------------------------------------------------------------
# 1. the narrowing kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 4099, "all"])
def test_narrow_kernel_bit_exact(cuda_device, gsdr_lib, n):
    """gsdr_narrow_sc16_device against gsdr_narrow_sc16_host for lengths around the group of four and the wave, the
    destination 0 .. 3 samples into its allocation (4-byte aligned only), the source 0 / 1 sample in (8-byte aligned
    only); the counter tensor starts at a non-zero value and gets the host's count added by every call."""
    import torch
    import gpu_sdr_amd as g
    vals = all_values()
    x = vals if n == "all" else np.random.default_rng(n).choice(vals, size=n)
    x = np.ascontiguousarray(x)
    n = x.size
    if n >= 63:
        # a random draw of a few thousand of the 459 000 values seldom holds one that clips: plant the special values
        # (+-Inf, NaN, +-1e10, both saturation edges) where the head, the body and the tail of the kernel take them
        special = vals[-17:]
        x[:3], x[n // 2:n // 2 + 17], x[-3:] = special[8:11], special, special[11:14]
    want, count = g.narrow_sc16(x, gain=1.0, return_clipped=True)
    np.testing.assert_array_equal(want, narrow_model(x, 1.0)[0])
    counter = torch.full((1,), 1000, dtype=torch.int64, device=cuda_device)
    calls = 0
    for s_off in (0, 1):
        src = torch.zeros(n + 2, dtype=torch.complex64, device=cuda_device)
        src[s_off:s_off + n] = torch.from_numpy(x).to(cuda_device)
        for d_off in range(4):
            dst, view = canary_dst(n, d_off, cuda_device)
            assert view.data_ptr() % 16 == 4 * d_off and src[s_off:].data_ptr() % 16 == 8 * s_off
            ret = g.narrow_sc16(src[s_off:s_off + n], out=view, gain=1.0, clipped=counter)
            assert ret is view
            calls += 1
            check_canary(dst, n, d_off, want, (s_off, d_off))
    assert int(counter.item()) == 1000 + calls * count
    if n > 100:
        assert count > 0
    # without `out` and without a counter: a new tensor of the input's shape + (2,)
    y = g.narrow_sc16(torch.from_numpy(x).to(cuda_device), gain=1.0)
    assert tuple(y.shape) == (n, 2) and y.dtype == torch.int16
    np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_narrow_kernel_gains_and_another_stream(cuda_device, gsdr_lib):
    import torch
    import gpu_sdr_amd as g
    rng = np.random.default_rng(9)
    n = 4099
    x = (rng.standard_normal(n) * 0.5 + 1j * rng.standard_normal(n) * 0.5).astype(np.complex64)
    src = torch.from_numpy(x).to(cuda_device)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda_device)
    counter = torch.full((1,), 7, dtype=torch.int64, device=cuda_device)
    total = 7
    for gain in (32767.0, 32768.0, 1.0 / 3.0):
        want, count = narrow_model(x, gain)
        dst = torch.zeros((n, 2), dtype=torch.int16, device=cuda_device)
        torch.cuda.synchronize()
        g.narrow_sc16(src, out=dst, gain=gain, stream=st, clipped=counter)
        st.synchronize()
        np.testing.assert_array_equal(dst.cpu().numpy(), want)
        total += count
    assert int(counter.item()) == total and total > 7
    with torch.cuda.stream(st):                              # the current torch stream when none is passed
        y = g.narrow_sc16(src, gain=32767.0)
    st.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), narrow_model(x, 32767.0)[0])
    # n == 0 touches nothing, not even the pointers; a bad gain is refused
    assert gsdr_lib.gsdr_narrow_sc16_device(None, None, 0, C.c_float(1.0), None, None) == 0
    assert gsdr_lib.gsdr_narrow_sc16_device(src.data_ptr(), y.data_ptr(), 4, C.c_float(0.0), None, None) == -1
    assert b"gain" in gsdr_lib.gsdr_last_error(None)
    with pytest.raises(ValueError):
        g.narrow_sc16(src, gain=float("nan"))


# ---------------------------------------------------------------------------
# 2. the tone comb
# ---------------------------------------------------------------------------
def make_comb(lib, rate, n_tones, seed):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(-(rate // 2) + 1, 0), np.arange(1, rate // 2)])
    freq = rng.choice(pool, size=n_tones, replace=False).astype(np.int32)
    ampl = rng.uniform(0.05, 1.0, n_tones).astype(np.float32)
    phase = rng.uniform(-3.0, 3.0, n_tones).astype(np.float32)
    h = lib.gsdr_txgen_tones_create(rate, freq.ctypes.data_as(C.POINTER(C.c_int)), ampl.ctypes.data_as(C.POINTER(C.c_float)),
                                    phase.ctypes.data_as(C.POINTER(C.c_float)), n_tones, 0)
    assert h, lib.gsdr_last_error(None)
    return h


def fill_c64(lib, h, n, start, dev):
    import torch
    out = torch.empty(n, dtype=torch.complex64, device=dev)
    assert lib.gsdr_txgen_tones_fill(h, out.data_ptr(), n, start, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("rate", [1_000_003, 1000])
@pytest.mark.parametrize("n_tones", [1, 3, 64, 65, 257])
def test_tones_fill_sc16_is_the_narrowed_complex64_fill(cuda_device, gsdr_lib, rate, n_tones):
    """gsdr_txgen_tones_fill_sc16 against the narrowed gsdr_txgen_tones_fill, bit for bit: one lane, a partial chunk, a
    full chunk, two chunks, four waves plus a remainder; lengths around the 1024-sample workgroup; start 0 and across
    the wrap of the period.  The gain of a case is 32767 / (0.99 quantile of |component| of its complex64 output), so
    that about one component in a hundred clips whatever the tones are."""
    import torch
    lib = gsdr_lib
    h = make_comb(lib, rate, n_tones, 100 * n_tones + rate % 7)
    assert lib.gsdr_txgen_sc16_gain(h) == 32767.0 and lib.gsdr_txgen_sc16_clipped(h) == 0
    expected_clipped = 0
    for n in (1, 1023, 1024, 1025, 4099):
        for start in (0, rate - 5):
            ref = fill_c64(lib, h, n, start, cuda_device)
            q = float(np.quantile(np.abs(ref.view(np.float32)), 0.99))
            assert q > 0
            gain = float(np.float32(32767.0 / q))
            assert lib.gsdr_txgen_set_sc16_gain(h, C.c_float(gain)) == 0 and lib.gsdr_txgen_sc16_gain(h) == gain
            want, count = narrow_model(ref, gain)
            if 2 * n >= 200:
                assert count > 0, (n, start)
            for d_off in range(4):
                dst, view = canary_dst(n, d_off, cuda_device)
                assert lib.gsdr_txgen_tones_fill_sc16(h, view.data_ptr(), n, start, None) == 0
                torch.cuda.synchronize()
                check_canary(dst, n, d_off, want, (n, start, d_off))
                expected_clipped += count
                assert lib.gsdr_txgen_sc16_clipped(h) == expected_clipped, (n, start, d_off)
    lib.gsdr_txgen_close(h)


def test_tones_fill_sc16_small_gain_no_tones_and_refusals(cuda_device, gsdr_lib):
    import torch
    lib = gsdr_lib
    h = make_comb(lib, 1000, 3, 1)
    # a gain so small that everything rounds to 0: zeros, nothing clipped
    assert lib.gsdr_txgen_set_sc16_gain(h, C.c_float(1e-6)) == 0
    dst, view = canary_dst(1025, 1, cuda_device)
    assert lib.gsdr_txgen_tones_fill_sc16(h, view.data_ptr(), 1025, 0, None) == 0
    check_canary(dst, 1025, 1, np.zeros((1025, 2), dtype=np.int16), "small gain")
    assert lib.gsdr_txgen_sc16_clipped(h) == 0
    # bad gains are refused and the old one stays
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.gsdr_txgen_set_sc16_gain(h, C.c_float(bad)) == -1
        assert b"gain" in lib.gsdr_last_error(None)
    assert lib.gsdr_txgen_sc16_gain(h) == float(np.float32(1e-6))
    # n == 0 touches nothing, not even the pointer
    assert lib.gsdr_txgen_tones_fill_sc16(h, None, 0, 0, None) == 0
    lib.gsdr_txgen_close(h)
    # no tones at all: zeros
    h = lib.gsdr_txgen_tones_create(1000, None, None, None, 0, 0)
    assert h
    dst, view = canary_dst(1500, 3, cuda_device)
    assert lib.gsdr_txgen_tones_fill_sc16(h, view.data_ptr(), 1500, 998, None) == 0
    check_canary(dst, 1500, 3, np.zeros((1500, 2), dtype=np.int16), "no tones")
    assert lib.gsdr_txgen_sc16_clipped(h) == 0
    lib.gsdr_txgen_close(h)


# ---------------------------------------------------------------------------
# 3. the chirp generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4099])
def test_source_chirp_sc16_is_the_narrowed_complex64_chirp(cuda_device, gsdr_lib, n):
    import torch
    from gpu_sdr_amd.demodulator import chirp_derive_tx
    lib = gsdr_lib
    scale = 0.7
    counter = torch.full((1,), 5, dtype=torch.int64, device=cuda_device)
    total = 5
    # a short period that wraps inside the buffer, and one beyond 2^32 samples (the 64-bit index path)
    for rate, f0, f1, steps, t in ((1_000_000, -100_000, 100_000, 50, 0.00035), (200_000_000, -100_000_000, 100_000_000, 1_000_000, 30.0)):
        cp = chirp_derive_tx(rate, f0, f1, steps, t)
        period = cp.num_steps * cp.length
        for last in (0, period - 3):
            ref = torch.empty(n, dtype=torch.complex64, device=cuda_device)
            assert lib.gsdr_source_chirp(ref.data_ptr(), n, C.c_ulonglong(last), C.byref(cp), C.c_float(scale), None) == 0
            torch.cuda.synchronize()
            ref = ref.cpu().numpy()
            for gain in (32767.0, 50000.0):              # 0.7 * 50000 > 32767: the crests clip
                want, count = narrow_model(ref, gain)
                for d_off in (0, 1, 3):
                    dst, view = canary_dst(n, d_off, cuda_device)
                    assert lib.gsdr_source_chirp_sc16(view.data_ptr(), n, C.c_ulonglong(last), C.byref(cp), C.c_float(scale),
                                                      C.c_float(gain), counter.data_ptr(), None) == 0
                    torch.cuda.synchronize()
                    check_canary(dst, n, d_off, want, (rate, last, gain, d_off))
                    total += count
    assert int(counter.item()) == total
    if n > 100:
        assert total > 5
    # no counter, n == 0
    assert lib.gsdr_source_chirp_sc16(None, 0, C.c_ulonglong(0), None, C.c_float(scale), C.c_float(1.0), None, None) == 0


# ---------------------------------------------------------------------------
# 4. TX_buffer_generator
# ---------------------------------------------------------------------------
def tx_params(kind):
    import gpu_sdr_amd as g
    if kind == "chirp":
        rate, f0, f1, steps, t, _, L, _ = CHIRP_CASES[2]                     # period 350 < buffer_len 500
        return g.param(mode="TX", rate=rate, buffer_len=L, freq=[f0], chirp_f=[f1], swipe_s=[steps], chirp_t=[t], ampl=[0.7],
                       wave_type=[g.w_type.CHIRP])
    wt = g.w_type.NOISE if kind == "noise" else g.w_type.TONES
    return g.param(mode="TX", rate=1000, buffer_len=300, freq=[100, -200, 37], ampl=[0.3, 0.2, 0.4], wave_type=[wt] * 3)


@pytest.mark.parametrize("kind", ["tones", "chirp", "noise"])
def test_tx_buffer_generator_sc16(cuda_device, gsdr_lib, kind):
    """get_sc16 (device), get_sc16 (numpy) and get (complex64) mixed on one generator advance one running index and equal
    the narrowed outputs of a twin that only uses get(); get_view_sc16() equals the narrowed get_view(); the gain is
    refused once the sc16 period buffer exists; sc16_clipped() is the sum of numpy's counts."""
    import torch
    import gpu_sdr_amd as g
    p = tx_params(kind)
    L = p.buffer_len
    p_twin = tx_params("tones") if kind == "noise" else p            # a NOISE request behaves as TONES
    gen, twin = g.TX_buffer_generator(p), g.TX_buffer_generator(p_twin)
    assert gen.mode == (g.w_type.CHIRP if kind == "chirp" else g.w_type.TONES)       # a NOISE request is TONES
    assert gen.sc16_gain == 32767.0 and gen.sc16_clipped() == 0
    gain = 50000.0                                       # crests above 32767 / 50000 = 0.655 clip
    gen.sc16_gain = gain
    assert gen.sc16_gain == gain
    for bad in (0.0, float("nan")):
        with pytest.raises(g.GsdrError, match="gain"):
            gen.sc16_gain = bad
    assert gen.sc16_gain == gain
    expected = 0
    ref = np.empty(L, dtype=np.complex64)
    for c in range(5):
        twin.get(ref)
        want, count = narrow_model(ref, gain)
        if c % 3 == 0:
            dst, view = canary_dst(L, 1 + c % 2, cuda_device)
            gen.get_sc16(view)
            torch.cuda.synchronize()
            check_canary(dst, L, 1 + c % 2, want, c)
            expected += count
        elif c % 3 == 1:
            out = np.full((L + 2, 2), CANARY, dtype=np.int16)
            gen.get_sc16(out[1:L + 1])
            np.testing.assert_array_equal(out[1:L + 1], want)
            assert (out[0] == CANARY).all() and (out[L + 1] == CANARY).all()
            expected += count
        else:
            got = np.empty(L, dtype=np.complex64)
            gen.get(got)
            np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert expected > 0 and gen.sc16_clipped() == expected
    if kind == "chirp":
        with pytest.raises(g.GsdrError, match="TONES"):
            gen.get_view_sc16()
        gen.sc16_gain = 1000.0                           # no period buffer: the gain stays free
    else:
        gen.sc16_gain = 45000.0                          # accepted: the period buffer does not exist yet
        gain = 45000.0
        views = []
        for c in range(5):
            v = gen.get_view_sc16()
            assert v.shape == (L, 2) and v.dtype == np.int16 and not v.flags.writeable
            views.append(v)
            np.testing.assert_array_equal(v, narrow_model(twin.get_view(), gain)[0], err_msg=str(c))
        with pytest.raises(g.GsdrError, match="period buffer"):
            gen.sc16_gain = 32767.0
        assert gen.sc16_gain == 45000.0
        # the period buffer is counted once: period + buffer_len samples, whatever number of views is handed out
        fresh = g.TX_buffer_generator(p_twin)
        ptr = gsdr_lib.gsdr_txgen_get_ptr(fresh._h)
        assert ptr
        total = 1000 + L                                 # rate * ceil(L / rate) + L
        whole = np.frombuffer((C.c_float * (2 * total)).from_address(ptr), dtype=np.complex64, count=total).copy()
        fresh.close()
        expected += narrow_model(whole, gain)[1]
        assert gen.sc16_clipped() == expected
        # mixing goes on: a device buffer behind the views continues the index, and the first view still holds its data
        twin.get(ref)
        want, count = narrow_model(ref, gain)
        dev = torch.empty((L, 2), dtype=torch.int16, device=cuda_device)
        gen.get_sc16(dev)
        np.testing.assert_array_equal(dev.cpu().numpy(), want)
        assert gen.sc16_clipped() == expected + count
        first = narrow_model(whole[(5 * L) % 1000:(5 * L) % 1000 + L], gain)[0]
        np.testing.assert_array_equal(views[0], first)
    with pytest.raises(TypeError):
        gen.get_sc16(np.zeros((L - 1, 2), dtype=np.int16))
    with pytest.raises(TypeError):
        gen.get_sc16(np.zeros(2 * L, dtype=np.int16))
    gen.close()
    twin.close()


# ---------------------------------------------------------------------------
# 5. the loop: TX generator -> sc16 -> RX sc16 entry
# ---------------------------------------------------------------------------
def test_loop_tx_sc16_into_rx_sc16(cuda_device, gsdr_lib, oracle_mod):
    """TONES generator -> get_sc16 (device) -> process_device_sc16 of a DIRECT demodulator whose sc16 scale is 1 / gain:
    within the project's bar of the oracle fed the widened int16 stream, lengths exact, and the recovered amplitudes
    within 1 % of the transmitted ones (a silently zeroed stream cannot pass)."""
    import torch
    import gpu_sdr_amd as g
    rate, L, M, F, N = 100_000, 10_000, 100, 4, 8
    freq = [-40_000 + 10_000 * k + 137 for k in range(N)]
    ampl = [0.04 + 0.01 * k for k in range(N)]           # sum 0.6: nothing clips at gain 32767
    tx = g.TX_buffer_generator(g.param(mode="TX", rate=rate, buffer_len=L, freq=freq, ampl=ampl, wave_type=[g.w_type.TONES] * N))
    assert tx.sc16_gain == 32767.0
    rx = make_direct(freq, rate, M, F, L)
    rx.sc16_scale = 1.0 / 32767.0
    ref = oracle_mod.Direct(freq, rate, M, F, L)
    x16 = torch.empty((L, 2), dtype=torch.int16, device=cuda_device)
    out = torch.empty(rx.out_capacity, dtype=torch.complex64, device=cuda_device)
    rows = []
    for c in range(3):
        tx.get_sc16(x16)
        n = rx.process(x16, out)
        torch.cuda.synchronize()
        y = out[:n].cpu().numpy().reshape(-1, N)
        x = g.widen_sc16(x16.cpu().numpy(), scale=1.0 / 32767.0)
        assert np.abs(x).max() > 0.3
        yr = ref.process(x)
        assert y.shape == yr.shape == (L // M, N), (c, y.shape, yr.shape)
        assert rel_err_per_tone(y, yr).max() <= TOL
        rows.append(y)
    assert tx.sc16_clipped() == 0
    settled = np.concatenate(rows[1:])                   # the FIR has filled after the first buffer
    got = np.abs(settled.mean(axis=0))
    assert (np.abs(got - np.array(ampl)) <= 0.01 * np.array(ampl)).all(), (got, ampl)
    rx.close()
    tx.close()
