"""Several chirps added into one TX buffer (GSDR_CREATE_MULTI_CHIRP, TX side) on the GPU: gsdr_source_multichirp against
the in-order float32 sum of gsdr_source_chirp outputs (bit for bit) and against the oracle, its sc16 form against the
narrowed complex64 output (bit for bit, clipped components counted alike), the generator handle, and the loop TX -> RX.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import TOL, rel_err_per_tone

pytestmark = pytest.mark.gpu

RATE = 200_000_000
SHORT = (1000, 3.5e-5)          # steps, chirp_t: length 7, period 7000
LONG = (1_000_000, 30.0)        # period 6e9 > 2^32: the 64-bit index
SPANS = [(-90_000_000, 90_000_000), (50_000_000, -50_000_000), (20_000_000, 20_000_000), (-90_000_000, 90_000_000),
         (-1_000_000, 77_777_777)] + [(-99_000_000 + 12_345_678 * k, 95_000_000 - 9_876_543 * k) for k in range(11)]


def derive(steps, t, n, tx=False):
    import gpu_sdr_amd as g
    from gpu_sdr_amd.demodulator import chirp_derive_tx
    return [(chirp_derive_tx if tx else g.chirp_derive)(RATE, f0, f1, steps, t) for f0, f1 in SPANS[:n]]


def scales_for(n, value=None):
    return [np.float32(value if value is not None else 0.5 / (1 + c % 3)) for c in range(n)]


def cp_array(cps):
    from gpu_sdr_amd._lib import ChirpParamC
    arr = (ChirpParamC * len(cps))()
    for c, cp in enumerate(cps):
        arr[c].num_steps, arr[c].length, arr[c].chirpness, arr[c].f0 = cp.num_steps, cp.length, cp.chirpness, cp.f0
    return arr


def in_order_sum(terms):
    """acc = t0; acc = acc + t1; ... on float32 views (real and imaginary parts apart)."""
    acc = terms[0].view(np.float32).copy()
    for t in terms[1:]:
        acc = acc + t.view(np.float32)
    return acc


@pytest.mark.parametrize("law", [SHORT, LONG], ids=["period7000", "period6e9"])
@pytest.mark.parametrize("n_chirps", [1, 2, 5, 16])
def test_source_multichirp_is_the_in_order_sum(cuda_device, gsdr_lib, oracle_mod, law, n_chirps):
    import torch
    from gpu_sdr_amd.source import device_chirp, device_chirps
    steps, t = law
    cps, scales = derive(steps, t, n_chirps), scales_for(n_chirps)
    period = cps[0].num_steps * cps[0].length
    ocps = [oracle_mod.chirp_params(RATE, f0, f1, steps, t) for f0, f1 in SPANS[:n_chirps]]
    for n in (1, 63, 64, 65, 4097):
        last = period - 30                 # the index wraps inside every call longer than 30 samples
        out = torch.empty(n, dtype=torch.complex64, device=cuda_device)
        one = torch.empty(n, dtype=torch.complex64, device=cuda_device)
        device_chirps(out, last, cps, scales)
        terms = []
        for cp, s in zip(cps, scales):
            device_chirp(one, last, cp, scale=float(s))
            terms.append(one.cpu().numpy())
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.int32), in_order_sum(terms).view(np.int32)), (n_chirps, n)
        # the oracle's sum; a term is within 3e-7 of its formula (test_device_sources_match_their_formulas), C terms add
        want = sum(oracle_mod.chirp_gen(ocp, last, n, float(s)).astype(np.complex128) for ocp, s in zip(ocps, scales))
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-7 * n_chirps)


def test_source_multichirp_sc16_is_the_narrowed_sum(cuda_device, gsdr_lib):
    """Scales of 0.6 per chirp: the sum of five chirps exceeds full scale now and then.  The buffer sits 4 bytes past
    a 16-byte boundary in the middle of an allocation of sentinels."""
    import torch
    from gpu_sdr_amd import narrow_sc16
    from gpu_sdr_amd.source import device_chirps
    lib = gsdr_lib
    n_chirps, guard = 5, 4096
    cps, scales = derive(*SHORT, n_chirps), scales_for(n_chirps, 0.6)
    arr, sc = cp_array(cps), (C.c_float * n_chirps)(*[float(s) for s in scales])
    stream = C.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)
    for n in (1, 63, 65, 4097):
        last = 7000 - 30
        ref = torch.empty(n, dtype=torch.complex64, device=cuda_device)
        device_chirps(ref, last, cps, scales)
        want, want_clipped = narrow_sc16(ref.cpu().numpy(), return_clipped=True)
        whole = torch.full((2 * guard + n + 1, 2), 0x5A5A, dtype=torch.int16, device=cuda_device)
        view = whole[guard + 1:guard + 1 + n]
        assert view.data_ptr() % 16 == 4
        clipped = torch.zeros(1, dtype=torch.int64, device=cuda_device)
        assert lib.gsdr_source_multichirp_sc16(view.data_ptr(), n, last, arr, sc, n_chirps, 32767.0, clipped.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        host = whole.cpu().numpy()
        assert np.array_equal(host[guard + 1:guard + 1 + n], want), n
        assert (host[:guard + 1] == 0x5A5A).all() and (host[guard + 1 + n:] == 0x5A5A).all(), n
        assert int(clipped.item()) == want_clipped
        if n == 4097:
            assert want_clipped > 0, "the scales were chosen to clip"
    # n == 0 touches nothing
    assert lib.gsdr_source_multichirp_sc16(None, 0, 0, None, None, 0, 0.0, None, None) == 0
    assert lib.gsdr_source_multichirp(None, 0, 0, None, None, 0, None) == 0


def make_tx(n_chirps, L, steps, t, ampl):
    import gpu_sdr_amd as g
    p = g.param(mode="TX", rate=RATE, buffer_len=L, freq=[s[0] for s in SPANS[:n_chirps]], chirp_f=[s[1] for s in SPANS[:n_chirps]],
                swipe_s=[steps], chirp_t=[t], ampl=[float(a) for a in ampl], wave_type=[g.w_type.CHIRP] * n_chirps)
    return g.TX_buffer_generator(p, device_index=0, multi_chirp=True)


def test_generator_handle_follows_the_running_index(cuda_device, gsdr_lib):
    """Successive buffers of a three-chirp generator are gsdr_source_multichirp at the running index, across the wrap at
    num_steps * length = 7000 (L = 3000: the third buffer wraps); complex64 and sc16 entries advance one index."""
    import torch
    import gpu_sdr_amd as g
    from gpu_sdr_amd.source import device_chirps
    L, n_chirps = 3000, 3
    scales = scales_for(n_chirps)
    gen = make_tx(n_chirps, L, *SHORT, scales)
    assert gen.mode == g.w_type.CHIRP
    cps = derive(*SHORT, n_chirps, tx=True)
    want = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    last = 0
    for k in range(6):
        device_chirps(want, last, cps, scales)
        w = want.cpu().numpy()
        if k % 3 == 0:
            out = torch.empty(L, dtype=torch.complex64, device=cuda_device)
            gen.get(out)
            assert np.array_equal(out.cpu().numpy().view(np.int32), w.view(np.int32)), k
        elif k % 3 == 1:
            host = np.empty(L, dtype=np.complex64)
            gen.get(host)
            assert np.array_equal(host.view(np.int32), w.view(np.int32)), k
        else:
            out16 = torch.empty((L, 2), dtype=torch.int16, device=cuda_device)
            gen.get_sc16(out16)
            assert np.array_equal(out16.cpu().numpy(), g.narrow_sc16(w)), k
        last = (last + L) % 7000
    with pytest.raises(g.GsdrError):
        gen.get_view()                      # gsdr_txgen_get_ptr stays TONES only
    gen.close()


def test_multichirp_loopback(cuda_device, gsdr_lib, oracle_mod):
    """A two-chirp generator (-100 ... 0 MHz and 0 ... +100 MHz) into a two-chirp demodulator: each column against the
    oracle of its chirp run on the generated buffer -- the other chirp's crosstalk is part of the expected value."""
    import torch
    import gpu_sdr_amd as g
    L, steps, t = 1_000_000, 1_000_000, 1.0
    sp = [(-100_000_000, 0), (0, 100_000_000)]
    ptx = g.param(mode="TX", rate=RATE, buffer_len=L, freq=[s[0] for s in sp], chirp_f=[s[1] for s in sp], swipe_s=[steps],
                  chirp_t=[t], ampl=[0.5, 0.25], wave_type=[g.w_type.CHIRP] * 2)
    gen = g.TX_buffer_generator(ptx, device_index=0, multi_chirp=True)
    prx = g.param(mode="RX", rate=RATE, buffer_len=L, decim=1, freq=[s[0] for s in sp], chirp_f=[s[1] for s in sp],
                  swipe_s=[steps], chirp_t=[t], wave_type=[g.w_type.CHIRP] * 2)
    dem = g.RX_buffer_demodulator(prx, device_index=0, multi_chirp=True)
    refs = [oracle_mod.Chirp(RATE, f0, f1, steps, t, 1, L) for f0, f1 in sp]
    x = torch.empty(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    for b in range(3):
        gen.get(x)
        n = dem.process(x, out)
        torch.cuda.synchronize()
        assert n == 5000 * 2
        y = out[:n].cpu().numpy().reshape(-1, 2)
        xh = x.cpu().numpy()
        yr = np.stack([np.array(r.process(xh)) for r in refs], axis=1)
        assert yr.shape == y.shape
        assert rel_err_per_tone(y, yr).max() <= TOL, b
        # and what a loop should show: each column sees its own chirp as a constant phasor of its amplitude
        assert abs(abs(y[:, 0].mean()) - 0.5) < 1e-2 and abs(abs(y[:, 1].mean()) - 0.25) < 1e-2
    gen.close()
    dem.close()
