"""sc16 input on the GPU: the widening kernel bit for bit against numpy, and every mode through the four sc16
entries (gsdr_demod_process_sc16 / _process_device_sc16 / _submit_sc16 / _submit_device_sc16) against the CPU
oracle fed the widened floats -- the project's bar: per tone <= 1e-5, every returned length exact.

Inputs: x16 = clip(rint(crandn * 8000), -32768, 32767) with the samples (32767, -32768) and (-32768, 32767)
planted in the first buffer.  The expected complex64 of a sample is float32(v) * float32(scale), exactly."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity import DIRECT_CASES, TOL, crandn, make_chirp, make_direct, make_pfb, rel_err_per_tone
from test_sc16_host import SCALES, bits, every_int16_pair, widened

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RX_LINK = os.path.join(ROOT, "gpu_sdr_amd", "rx_link")
DEFAULT_SCALE = 2.0 ** -15
ENTRIES = ["host", "device", "submit", "submit_device"]


def quantised(rng, L, first):
    z = crandn(rng, L) * 8000
    x = np.empty((L, 2), dtype=np.int16)
    x[:, 0] = np.clip(np.rint(z.real), -32768, 32767)
    x[:, 1] = np.clip(np.rint(z.imag), -32768, 32767)
    if first:
        x[L // 3] = (32767, -32768)
        x[L - 1] = (-32768, 32767)
    return x


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 4099, 65536])
def test_widen_kernel_bit_exact(cuda_device, gsdr_lib, n):
    """gsdr_widen_sc16_device for lengths around the group of four and the wave, every start alignment a view can
    have (source 0 .. 3 samples into its allocation: 4-byte aligned only; destination 0 / 1 sample in: 8-byte
    aligned only), three scales.  The sample in front of the destination and 64 behind it stay untouched."""
    import torch
    import gpu_sdr_amd as g
    x = every_int16_pair() if n == 65536 else quantised(np.random.default_rng(n), n, True)
    canary = np.complex64(-7.5 + 3.25j)
    for scale in SCALES:
        want = bits(widened(x, scale))
        for s_off in range(4):
            src = torch.zeros((n + 8, 2), dtype=torch.int16, device=cuda_device)
            src[s_off:s_off + n] = torch.from_numpy(x).to(cuda_device)
            for d_off in (0, 1):
                dst = torch.full((n + 66,), complex(canary), dtype=torch.complex64, device=cuda_device)
                view = dst[1 + d_off:1 + d_off + n]
                assert src[s_off:].data_ptr() % 16 == 4 * s_off and view.data_ptr() % 16 == 8 * (1 - d_off)
                ret = g.widen_sc16(src[s_off:s_off + n], out=view, scale=scale)
                assert ret is view
                got = dst.cpu().numpy()
                np.testing.assert_array_equal(bits(got[1 + d_off:1 + d_off + n]), want, err_msg=f"{scale} {s_off} {d_off}")
                assert (got[:1 + d_off] == canary).all() and (got[1 + d_off + n:] == canary).all(), (scale, s_off, d_off)
    # without `out`: a new tensor of the input's shape
    y = g.widen_sc16(torch.from_numpy(x).to(cuda_device))
    assert y.shape == (n,) and y.dtype == torch.complex64
    np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(widened(x, DEFAULT_SCALE)))


def test_widen_kernel_on_another_stream(cuda_device, gsdr_lib):
    import torch
    import gpu_sdr_amd as g
    n = 4099
    x = quantised(np.random.default_rng(77), n, True)
    src = torch.from_numpy(x).to(cuda_device)
    dst = torch.zeros(n, dtype=torch.complex64, device=cuda_device)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(cuda_device)
    g.widen_sc16(src, out=dst, scale=1.0 / 32767.0, stream=st)
    st.synchronize()
    np.testing.assert_array_equal(bits(dst.cpu().numpy()), bits(widened(x, 1.0 / 32767.0)))
    with torch.cuda.stream(st):                              # the current torch stream when none is passed
        y = g.widen_sc16(src)
    st.synchronize()
    np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(widened(x, DEFAULT_SCALE)))


# ---------------------------------------------------------------------------
# 2. every mode through every entry
# ---------------------------------------------------------------------------
def golden_config(name):
    return json.loads(str(np.load(os.path.join(HERE, "golden", f"{name}.npz"), allow_pickle=False)["config"]))


def direct_case(N, rate, M, F, L, nbuf):
    rng = np.random.default_rng(1600 + N + M)
    freq = rng.choice(np.arange(-rate // 2 + 1, rate // 2), size=N, replace=False)
    freq[0], freq[1], freq[2] = 0, rate // 2 - 1, -(rate // 2) + 1
    return dict(make=lambda: make_direct(freq, rate, M, F, L), oracle=lambda o: o.Direct(freq, rate, M, F, L),
                nch=N, L=L, nbuf=nbuf, seed=N + M)


def tones_case(nbuf=5):
    c = golden_config("pfb")
    return dict(make=lambda: make_pfb(c["freq"], c["rate"], c["fft_tones"], c["pf_average"], c["buffer_len"]),
                oracle=lambda o: o.Pfb(c["freq"], c["rate"], c["fft_tones"], c["pf_average"], c["buffer_len"]),
                nch=len(c["freq"]), L=c["buffer_len"], nbuf=nbuf, seed=2)


def noise_case():
    import gpu_sdr_amd as g
    c = golden_config("noise")
    p = g.param(mode="RX", rate=1200, buffer_len=c["buffer_len"], decim=0, pf_average=c["pf_average"],
                fft_tones=c["fft_tones"], freq=[0], wave_type=[g.w_type.NOISE])
    return dict(make=lambda: g.RX_buffer_demodulator(p, device_index=0),
                oracle=lambda o: o.Noise(c["fft_tones"], c["pf_average"], c["buffer_len"]),
                nch=c["fft_tones"], L=c["buffer_len"], nbuf=5, seed=3)


def chirp_case(nbuf=4):
    c = golden_config("chirp")
    args = (c["rate"], c["freq"], c["chirp_f"], c["swipe_s"], c["chirp_t"], c["decim"], c["buffer_len"])
    return dict(make=lambda: make_chirp(*args), oracle=lambda o: o.Chirp(*args), nch=1, L=c["buffer_len"], nbuf=nbuf, seed=4)


C3_BLOCK = (7, 200_000_000, 1000, 4, 50_000, 3)
DIRECT_SC16 = {"c3_block": C3_BLOCK, "carry_outlives_buffer": (5, 1000, 50, 4, 100, 7), "odd": (6, 1_000_000, 37, 5, 37_000, 2),
               "undecimated": (4, 1_000_000, 0, 4, 4096, 2)}
CASES = {**{k: (lambda v=v: direct_case(*v)) for k, v in DIRECT_SC16.items()},
         "tones": tones_case, "noise": noise_case, "chirp": chirp_case}
_STREAMS = {}


def test_direct_shapes_are_those_of_the_parity_suite():
    for k, v in DIRECT_SC16.items():
        assert k == "undecimated" or v in DIRECT_CASES, k


def stream_of(name, case, oracle_mod, scale=DEFAULT_SCALE):
    """The quantised input buffers of a case and what the oracle makes of the widened floats; computed once."""
    key = (name, scale)
    if key not in _STREAMS:
        rng = np.random.default_rng(160 + case["seed"])
        xs = [quantised(rng, case["L"], c == 0) for c in range(case["nbuf"])]
        ref = case["oracle"](oracle_mod)
        want = [np.array(ref.process(widened(x, scale)), copy=True) for x in xs]
        ref.close()
        _STREAMS[key] = (xs, want)
    return _STREAMS[key]


def pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def run_entry(dem, entry, xs, dev):
    """Buffers xs (int16 (L, 2) = sc16, or complex64) through one entry of `dem`, in order; the outputs as numpy."""
    import torch
    cap = dem.out_capacity
    if entry == "host":
        outs = []
        for x in xs:
            out = np.empty(cap, dtype=np.complex64)
            outs.append(out[:dem.process(x, out)].copy())
        return outs
    if entry == "device":
        outs = []
        for x in xs:
            out = torch.empty(cap, dtype=torch.complex64, device=dev)
            n = dem.process(torch.from_numpy(x).to(dev), out)
            torch.cuda.synchronize()
            outs.append(out[:n].cpu().numpy())
        return outs
    depth = 4                                          # GSDR_PIPELINE_DEPTH (include/gsdr.h)
    if entry == "submit":
        ins = [pinned(x) for x in xs]
        bufs = [pinned(np.zeros(max(cap, 1), dtype=np.complex64)) for _ in xs]
    else:
        ins = [torch.from_numpy(x).to(dev) for x in xs]
        bufs = [torch.empty(max(cap, 1), dtype=torch.complex64, device=dev) for _ in xs]
        torch.cuda.synchronize()
    lens, pending = [None] * len(xs), []
    for k in range(len(xs)):
        if len(pending) == depth:                      # as many outstanding as the pipeline takes
            j = pending.pop(0)
            lens[j] = dem.wait()
        (dem.submit if entry == "submit" else dem.submit_device)(ins[k], bufs[k])
        pending.append(k)
    while pending:
        j = pending.pop(0)
        lens[j] = dem.wait()
    if entry == "submit":
        return [b[:n].copy() for b, n in zip(bufs, lens)]
    torch.cuda.synchronize()
    return [b[:n].cpu().numpy() for b, n in zip(bufs, lens)]


def check_against_oracle(outs, want, nch):
    assert [o.size for o in outs] == [w.size for w in want]
    y = np.concatenate(outs).reshape(-1, nch)
    yr = np.concatenate([w.reshape(-1) for w in want]).reshape(-1, nch)
    err = rel_err_per_tone(y, yr)
    assert err.max() <= TOL, err.max()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_mode_through_every_sc16_entry(cuda_device, gsdr_lib, oracle_mod, monkeypatch, name, entry):
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    case = CASES[name]()
    xs, want = stream_of(name, case, oracle_mod)
    dem = case["make"]()
    assert dem.sc16_scale == DEFAULT_SCALE
    outs = run_entry(dem, entry, xs, cuda_device)
    dem.close()
    check_against_oracle(outs, want, case["nch"])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(DIRECT_SC16))
@pytest.mark.parametrize("engine", ["mfma_ring16", "valu"])
def test_direct_sc16_on_forced_engines(cuda_device, gsdr_lib, oracle_mod, monkeypatch, engine, name, entry):
    """DIRECT once more on the matrix cores (GSDR_DDC_MFMA=1 GSDR_MFMA_ASM=4; GSDR_DDC_FEW=0 as well, or the few-tone
    kernel would take the long decimation) and on the VALU kernels (GSDR_DDC_MFMA=0)."""
    monkeypatch.setenv("GSDR_DDC_MFMA", "1" if engine == "mfma_ring16" else "0")
    if engine == "mfma_ring16":
        monkeypatch.setenv("GSDR_MFMA_ASM", "4")
        monkeypatch.setenv("GSDR_DDC_FEW", "0")
    case = CASES[name]()
    xs, want = stream_of(name, case, oracle_mod)
    dem = case["make"]()
    outs = run_entry(dem, entry, xs, cuda_device)
    dem.close()
    check_against_oracle(outs, want, case["nch"])


@pytest.mark.parametrize("entry", ENTRIES)
def test_nodsp_sc16_is_the_widening(cuda_device, gsdr_lib, entry):
    import gpu_sdr_amd as g
    L = 501
    dem = g.RX_buffer_demodulator(g.param(rate=1000, buffer_len=L, wave_type=[]), device_index=0)
    assert dem.mode == g.w_type.NODSP
    rng = np.random.default_rng(5)
    xs = [quantised(rng, L, c == 0) for c in range(6)]
    outs = run_entry(dem, entry, xs, cuda_device)
    dem.sc16_scale = 1.0
    outs1 = run_entry(dem, entry, xs[:1], cuda_device)
    dem.close()
    for x, y in zip(xs, outs):
        np.testing.assert_array_equal(bits(y), bits(widened(x, DEFAULT_SCALE)))
    np.testing.assert_array_equal(bits(outs1[0]), bits(widened(xs[0], 1.0)))


# ---------------------------------------------------------------------------
# 3. twin identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tones", "chirp", "c3_block"])
def test_sc16_twin_is_bit_identical_to_the_complex64_twin(cuda_device, gsdr_lib, monkeypatch, name):
    """Two handles with the same parameters, one fed sc16, one the numpy-widened complex64: the same bits out, on every
    entry -- the sc16 entries add the widening and nothing else.  Two complex64 twins are compared first: were those
    to differ, the engine itself would not be repeatable and the sc16 comparison would say nothing."""
    if name == "c3_block":
        monkeypatch.setenv("GSDR_DDC_MFMA", "1")
        monkeypatch.setenv("GSDR_MFMA_ASM", "4")
        monkeypatch.setenv("GSDR_DDC_FEW", "0")
    case = CASES[name]()
    rng = np.random.default_rng(33)
    xs = [quantised(rng, case["L"], c == 0) for c in range(case["nbuf"])]
    ws = [widened(x, DEFAULT_SCALE) for x in xs]
    for entry in ENTRIES:
        a, b, c = case["make"](), case["make"](), case["make"]()
        if name == "c3_block":
            assert a.kernel_name.startswith("ddc_mfma"), a.kernel_name
        ya, yb, yc = run_entry(a, entry, ws, cuda_device), run_entry(b, entry, ws, cuda_device), run_entry(c, entry, xs, cuda_device)
        for h in (a, b, c):
            h.close()
        assert sum(y.size for y in ya) > 0
        for k in range(len(xs)):
            np.testing.assert_array_equal(bits(ya[k]), bits(yb[k]), err_msg=f"complex64 twins differ: {entry} buffer {k}")
            np.testing.assert_array_equal(bits(yc[k]), bits(ya[k]), err_msg=f"sc16 twin differs: {entry} buffer {k}")


# ---------------------------------------------------------------------------
# 4. pipeline
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prepared", [True, False], ids=["prepared", "unprepared"])
def test_sc16_pipeline_nine_buffers(cuda_device, gsdr_lib, oracle_mod, monkeypatch, prepared):
    """submit() with GSDR_PIPELINE_DEPTH sc16 buffers outstanding, nine different buffers, the whole stream against the
    oracle; once after prepare(sc16=True, rehearse=True) -- whose twin must leave the handle's own state alone -- and
    once with everything created on first use."""
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    case = direct_case(*C3_BLOCK[:5], 9)
    xs, want = stream_of("c3_block_x9", case, oracle_mod)
    assert len({x.tobytes() for x in xs}) == 9
    dem = case["make"]()
    if prepared:
        dem.prepare(sc16=True, rehearse=True)
    outs = run_entry(dem, "submit", xs, cuda_device)
    dem.close()
    check_against_oracle(outs, want, case["nch"])


# ---------------------------------------------------------------------------
# 5. two streams
# ---------------------------------------------------------------------------
def test_sc16_process_device_alternating_streams(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """process_device with int16 tensors on two torch streams in turn, six different buffers, nothing synchronised in
    between.  The handle widens into a buffer of its own: the widening of call j+1 must sit behind the join with
    call j's stream, or it overwrites what call j still reads (a busy neighbour keeps the older stream late)."""
    import torch
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    case = direct_case(*C3_BLOCK[:5], 6)
    xs, want = stream_of("c3_block_x6", case, oracle_mod)
    dem = case["make"]()
    ins = [torch.from_numpy(x).to(cuda_device) for x in xs]
    outs = [torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device) for _ in xs]
    ballast = torch.randn(2048, 2048, device=cuda_device)
    streams = [torch.cuda.Stream(cuda_device), torch.cuda.Stream(cuda_device)]
    torch.cuda.synchronize()
    lens = []
    for k in range(len(xs)):
        st = streams[k % 2]
        with torch.cuda.stream(st):
            for _ in range(3):
                ballast = ballast @ ballast * 1e-4        # keeps this stream busy for a while
        lens.append(dem.process_device(ins[k], outs[k], st))
    torch.cuda.synchronize()
    got = [o[:n].cpu().numpy() for o, n in zip(outs, lens)]
    dem.close()
    check_against_oracle(got, want, case["nch"])


# ---------------------------------------------------------------------------
# 6. mixed entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_block", "tones"])
def test_sc16_and_complex64_calls_mixed_on_one_handle(cuda_device, gsdr_lib, oracle_mod, monkeypatch, name):
    """Buffers 0 and 2 go in as sc16, 1 and 3 as the widened complex64, through host and device entries in turn: the
    stream state (FIR carry, NCO index, raw windows) does not know the difference."""
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    case = direct_case(*C3_BLOCK[:5], 4) if name == "c3_block" else tones_case(4)
    xs, want = stream_of(name + "_x4", case, oracle_mod)
    dem = case["make"]()
    outs = []
    for k, (x, entry) in enumerate(zip(xs, ["host", "device", "device", "host"])):
        outs += run_entry(dem, entry, [x if k % 2 == 0 else widened(x, DEFAULT_SCALE)], cuda_device)
    dem.close()
    check_against_oracle(outs, want, case["nch"])


# ---------------------------------------------------------------------------
# 7. scale and errors
# ---------------------------------------------------------------------------
def test_sc16_scale_and_errors(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    import torch
    import gpu_sdr_amd as g
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    scale = 1.0 / 32767.0
    case = direct_case(*C3_BLOCK)
    xs, want = stream_of("c3_block", case, oracle_mod, scale)
    dem = case["make"]()
    dem.sc16_scale = scale
    assert dem.sc16_scale == float(np.float32(scale))
    for bad in (0.0, -1.0, -2.0 ** -15, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(g.GsdrError, match="finite and > 0"):
            dem.sc16_scale = bad
        assert gsdr_lib.gsdr_demod_set_sc16_scale(dem._h, C.c_float(bad)) == -1
        assert dem.sc16_scale == float(np.float32(scale))                  # the old scale is kept
    outs = run_entry(dem, "host", xs[:1], cuda_device) + run_entry(dem, "device", xs[1:], cuda_device)
    check_against_oracle(outs, want, case["nch"])
    # null pointers: -1 and "null buffer", on each of the four entries
    L = case["L"]
    buf = np.zeros(max(dem.out_capacity, 2 * L), dtype=np.complex64)
    dbuf = torch.zeros(max(dem.out_capacity, L), dtype=torch.complex64, device=cuda_device)
    for fn, good, extra in ((gsdr_lib.gsdr_demod_process_sc16, buf.ctypes.data, ()),
                            (gsdr_lib.gsdr_demod_submit_sc16, buf.ctypes.data, ()),
                            (gsdr_lib.gsdr_demod_process_device_sc16, dbuf.data_ptr(), (None,)),
                            (gsdr_lib.gsdr_demod_submit_device_sc16, dbuf.data_ptr(), ())):
        for args in ((None, good), (good, None)):
            gsdr_lib.gsdr_demod_set_sc16_scale(dem._h, C.c_float(-1.0))     # leaves another message behind
            assert fn(dem._h, *args, *extra) == -1
            assert gsdr_lib.gsdr_last_error(dem._h) == b"null buffer"
    with pytest.raises(g.GsdrError):
        dem.wait()                                                       # nothing was submitted
    # other dtypes are still refused
    out = np.empty(dem.out_capacity, dtype=np.complex64)
    for wrong in (np.zeros((L, 2), dtype=np.float32), np.zeros(2 * L, dtype=np.int16), np.zeros((L, 2), dtype=np.int32)):
        with pytest.raises(TypeError):
            dem.process(wrong, out)
        with pytest.raises(TypeError):
            dem.submit(wrong, out)
    dout = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
    for wrong in (torch.zeros((L, 2), dtype=torch.float32, device=cuda_device), torch.zeros(2 * L, dtype=torch.int16, device=cuda_device)):
        with pytest.raises(TypeError):
            dem.process_device(wrong, dout)
        with pytest.raises(TypeError):
            dem.submit_device(wrong, dout)
    with pytest.raises(ValueError):
        dem.process(np.zeros((L - 1, 2), dtype=np.int16), out)
    dem.close()


# ---------------------------------------------------------------------------
# 8. the C++ class
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", [False, True], ids=["process", "submit_wait"])
def test_rx_link_sc16_direct_against_oracle(cuda_device, gsdr_lib, oracle_mod, tmp_path, pipe):
    """`rx_link file ... sc16`: the sc16 overloads of include/USRP_demodulator.hpp in the reference's per-buffer loop,
    over a recorded int16 stream at the DIRECT golden configuration (more buffers than the pipeline is deep)."""
    assert os.path.exists(RX_LINK), "gpu_sdr_amd/rx_link is built by __graft_entry__.build() / make -C gpu_sdr_amd/csrc"
    c = golden_config("direct")
    L, N, nbuf = c["buffer_len"], len(c["freq"]), 7
    rng = np.random.default_rng(88)
    xs = [quantised(rng, L, k == 0) for k in range(nbuf)]
    cfg, fin, fout = tmp_path / "cfg.txt", tmp_path / "in.sc16", tmp_path / "out.c64"
    cfg.write_text("\n".join(["mode DIRECT", f"rate {c['rate']}", f"buffer_len {L}", f"decim {c['decim']}",
                              f"pf_average {c['pf_average']}", "freq " + " ".join(str(int(f)) for f in c["freq"])]) + "\n")
    np.concatenate(xs).tofile(fin)
    p = subprocess.run([RX_LINK, "file", str(cfg), str(fin), str(fout)] + (["pipe"] if pipe else []) + ["sc16"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert "sc16" in info["harness"] and info["buffers"] == nbuf
    ref = oracle_mod.Direct(c["freq"], c["rate"], c["decim"], c["pf_average"], L)
    want = [ref.process(widened(x, DEFAULT_SCALE)) for x in xs]
    assert info["channels"] == N and info["lengths"] == [w.size for w in want]
    y = np.fromfile(fout, dtype=np.complex64)
    check_against_oracle([y], [np.concatenate(want)], N)
