"""Create, prepare, use and close a handle of every setup path, three times in one process: what the handle owns is
released by its owners (gpu_sdr_amd/csrc/dev_owner.h), and a handle made after two others were closed computes, bit
for bit, what the first one did.  Also the refusals of gsdr_demod_create that come behind the creation of the stream
(the half-made handle is released, a good creation follows), gsdr_demod_set_frame_average around the staging it drops,
and the TX generator.  No test here measures free device memory: on a shared machine that number belongs to everyone's
processes.  Leaks of the owners themselves are counted by tests/test_dev_owner_host.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE = 1_000_000
AVERAGE_TOO_LATE = "frame average: must be set before the first buffer goes through the handle"


def direct(decim, L, f=4):
    return dict(rate=RATE, buffer_len=L, decim=decim, pf_average=f, freq=[100_000, -200_000, 37_000], wave="DIRECT", n=3)


def pfb(wave="TONES", nfft=64):
    return dict(rate=RATE, buffer_len=1024, decim=0, pf_average=2, fft_tones=nfft, freq=[100_000, -200_000, 37_000],
                wave=wave, n=3)


def chirp(decim, L=500):
    # 350 samples in 50 steps: length 7, with decim 2 a point is 14 samples (tests/test_gpu_parity.py, CHIRP_CASES[2])
    return dict(rate=RATE, buffer_len=L, decim=decim, freq=[-100_000], chirp_f=[100_000], swipe_s=[50], chirp_t=[0.00035],
                wave="CHIRP", n=1)


# id: (environment of the creation, parameters, frame average, what describe() must say)
PATHS = {
    # decim 10 x pf_average 4: the 24 samples that pad the 40-sample window to whole 32-sample blocks are more than a
    # block of 10, which fails the padding condition of ddc_mfma_takes_direct (csrc/ddc_plan.h): this shape runs the generic
    # ddc_kernel; the two shapes below it do run the matrix cores
    "direct": ({}, direct(10, 1000), 1, dict(family="fp32 VALU")),
    "direct_mfma": ({}, direct(32, 3200), 1, dict(family="f16 MFMA, hi/lo split", complex_mac=4)),
    "direct_mfma_images": (dict(GSDR_MFMA_PREC="1", GSDR_MFMA_3M="1"), direct(32, 3200), 1,
                           dict(family="f16 MFMA, hi/lo split", complex_mac=3)),
    "direct_flat_autotuned": (dict(GSDR_DDC_MFMA="0"), direct(10, 1000), 1, dict(family="packed fp32 VALU")),
    "direct_undecimated": ({}, direct(0, 1000), 1, dict(family="fp32 VALU")),
    "tones_lds": ({}, pfb(), 1, dict(family="polyphase filter + fp32 Stockham FFT inside the LDS + bin selection, one launch")),
    "tones_fft_stages": (dict(GSDR_PFB_LDS="0"), pfb(), 1, dict(family="fp32 Stockham FFT behind the polyphase filter")),
    "tones_ddc": (dict(GSDR_PFB_LDS="0", GSDR_TONES_FFT="0"), pfb(), 1, dict(family="f16 MFMA, hi/lo split")),
    "noise_fft_stages": (dict(GSDR_PFB_LDS="0"), pfb("NOISE"), 1, dict(family="fp32 Stockham FFT behind the polyphase filter", channels=64)),
    # 34 = 2 * 17 points: in the LDS either way, through Bluestein's identity (at 128 points) only because of the switch.
    # (The switch needs a length that fft_plan_build plans through Bluestein, a prime factor above 13: at 64 points it
    # makes the creation fail with "PFB allocation failed".)
    "tones_lds_bluestein": (dict(GSDR_PFB_BLUESTEIN="1"), pfb(nfft=34), 1,
                            dict(family="polyphase filter + Bluestein (two fp32 Stockham FFTs) inside the LDS + bin selection, one launch")),
    "tones_lds_averaged": ({}, pfb(), 2, dict(frame_average=2)),
    "chirp_lockin": ({}, chirp(2), 1, dict(mode="CHIRP")),
    "chirp_undecimated": ({}, chirp(0), 1, dict(mode="CHIRP")),
    "nodsp": ({}, dict(rate=RATE, buffer_len=1000, decim=0, wave="NODSP", n=1), 1, dict(mode="NODSP")),
}


def make(monkeypatch, env, kw):
    """A handle created under exactly `env` (the switches are read at creation)."""
    import gpu_sdr_amd as g
    for k in [k for k in os.environ if k.startswith("GSDR_") and not k.startswith("GSDR_LIB")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw)
    wave, n = getattr(g.w_type, kw.pop("wave")), kw.pop("n")
    return g.RX_buffer_demodulator(g.param(mode="RX", wave_type=[wave] * n, **kw), device_index=0)


def buffers(L, count=2):
    rng = np.random.default_rng(L)
    return [(0.5 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64) for _ in range(count)]


def feed(dem, x):
    out = np.zeros(max(dem.out_capacity, 1), dtype=np.complex64)
    n = dem.process(x, out)
    return out[:n].copy()


def lifetime(monkeypatch, name):
    """create -> prepare with every flag -> two buffers through process -> close; the two outputs"""
    env, kw, avg, says = PATHS[name]
    dem = make(monkeypatch, env, kw)
    try:
        if avg > 1:
            dem.set_frame_average(avg)
        d = dem.describe()
        assert {k: d[k] for k in says} == says, d
        dem.prepare(host=True, pipeline=True, pipeline_host=True, rehearse=True, sc16=True)
        return [feed(dem, x) for x in buffers(kw["buffer_len"])]
    finally:
        dem.close()


FIRST = {}      # path -> the outputs of its first handle: computed once, shared, never changed


def first_outputs(monkeypatch, name):
    if name not in FIRST:
        FIRST[name] = lifetime(monkeypatch, name)
    return FIRST[name]


@pytest.mark.parametrize("name", list(PATHS))
def test_third_handle_equals_the_first(cuda_device, monkeypatch, name):
    first = first_outputs(monkeypatch, name)
    assert sum(y.size for y in first) > 0 and all(np.isfinite(y.view(np.float32)).all() for y in first)
    assert any(y.size and np.abs(y).max() > 0 for y in first)
    lifetime(monkeypatch, name)
    third = lifetime(monkeypatch, name)
    assert len(third) == len(first)
    for a, b in zip(first, third):
        assert a.size == b.size and a.tobytes() == b.tobytes()


def test_frame_average_switched_off_again_and_set_too_late(cuda_device, monkeypatch):
    """set_frame_average(4) behind prepare, then (1): the staging that prepare made is dropped and made anew by the
    entry, and the handle returns the frames themselves.  Behind the first buffer the call is refused, and the handle
    goes on as if it had not been made."""
    plain = first_outputs(monkeypatch, "tones_lds")
    env, kw, _, _ = PATHS["tones_lds"]
    dem = make(monkeypatch, env, kw)
    try:
        cap = dem.out_capacity
        dem.prepare(host=True, pipeline=True, pipeline_host=True, rehearse=True, sc16=True)
        dem.set_frame_average(4)
        assert dem.out_capacity < cap
        dem.set_frame_average(1)
        assert dem.out_capacity == cap and dem.frame_average == 1
        xs = buffers(kw["buffer_len"])
        assert feed(dem, xs[0]).tobytes() == plain[0].tobytes()
        from gpu_sdr_amd.demodulator import GsdrError
        with pytest.raises(GsdrError) as e:
            dem.set_frame_average(2)
        assert str(e.value) == AVERAGE_TOO_LATE
        assert dem.frame_average == 1 and dem.out_capacity == cap
        assert feed(dem, xs[1]).tobytes() == plain[1].tobytes()
    finally:
        dem.close()


@pytest.mark.parametrize("bad,good,msg", [
    (direct(10, 1005), direct(10, 1000), "buffer_len must be a multiple of decim (ref: fir.cu:20)"),
    (chirp(2, L=10), chirp(2), "chirp lock-in needs length*decim <= buffer_len"),
], ids=["direct_length_not_a_multiple", "chirp_point_longer_than_buffer"])
def test_refusal_behind_the_stream_then_a_good_creation(cuda_device, gsdr_lib, monkeypatch, bad, good, msg):
    from gpu_sdr_amd.demodulator import GsdrError
    for _ in range(3):
        with pytest.raises(GsdrError) as e:
            make(monkeypatch, {}, bad)
        assert str(e.value) == msg and gsdr_lib.gsdr_last_error(None) == msg.encode()
        dem = make(monkeypatch, {}, good)
        try:
            assert feed(dem, buffers(good["buffer_len"], 1)[0]).size > 0
        finally:
            dem.close()


@pytest.mark.parametrize("kind", ["tones", "chirp"])
def test_tx_generator_three_times(cuda_device, kind):
    """One generator of each kind, read once per wire format (to host memory, through the staging buffer it owns; TONES
    also through its period buffers), closed; the third reads what the first did."""
    import gpu_sdr_amd as g
    from test_gpu_sc16_tx import tx_params
    p = tx_params(kind)
    reads = []
    for _ in range(3):
        gen = g.TX_buffer_generator(p)
        try:
            c64, sc16 = np.zeros(p.buffer_len, dtype=np.complex64), np.zeros((p.buffer_len, 2), dtype=np.int16)
            gen.get(c64)
            gen.get_sc16(sc16)
            got = [c64, sc16]
            if kind == "tones":
                got += [gen.get_view().copy(), gen.get_view_sc16().copy()]
            assert gen.sc16_clipped() == 0
            reads.append(got)
        finally:
            gen.close()
    assert np.abs(reads[0][0]).max() > 0 and np.abs(reads[0][1]).max() > 0
    for a, b in zip(reads[0], reads[2]):
        assert a.tobytes() == b.tobytes()
