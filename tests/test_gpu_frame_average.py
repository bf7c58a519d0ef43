"""Mean of k consecutive PFB frames on the device (gsdr_demod_set_frame_average, gsdr_frame_average_device):
the kernel alone against the host function, bit for bit, with guard zones; a handle on every PFB path against
(a) the host function applied to the frames of a twin handle that does not average, bit for bit, and (b) the
oracle's frames averaged in float64; every RX entry; the surface; rx_link and gsdr_server."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import _extents as ext
from _frame_average import CASES, KINDS, bits, case_input, nonfinite_groups
from _margins import record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
KIND_C = {"complex": 0, "power": 1}


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_frames,n_ch,k,count", CASES)
def test_kernel_matches_host_bit_for_bit(cuda_device, gsdr_lib, n_frames, n_ch, k, count, kind):
    """Null stream and a second stream; -0, denormal squares, a NaN frame and an Inf frame in the input."""
    import torch
    import gpu_sdr_amd as g
    frames, acc, nan_f, inf_f = case_input(n_frames, n_ch, k, count)
    want, want_acc, want_c = g.frame_average(frames, k, kind, count, acc)
    d_frames = torch.from_numpy(frames).to(cuda_device)
    d_acc = None if acc is None else torch.from_numpy(acc).to(cuda_device)
    second = torch.cuda.Stream(device=cuda_device)
    torch.cuda.synchronize()
    for stream in (torch.cuda.default_stream(cuda_device), second):
        out, acc_out, c = g.frame_average(d_frames, k, kind, count, d_acc, stream=stream)
        stream.synchronize()
        assert c == want_c and tuple(out.shape) == want.shape
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(want))
        np.testing.assert_array_equal(bits(acc_out.cpu().numpy()), bits(want_acc))
    np.testing.assert_array_equal(bits(d_frames.cpu().numpy()), bits(frames))
    bad = nonfinite_groups(n_frames, k, count, (nan_f, inf_f))
    for s in range(want.shape[0]):
        assert np.isfinite(want[s].real).all() == (s not in bad), (s, bad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_frames,n_ch,k,count", CASES)
def test_kernel_extents_offset_pointers_and_guards(cuda_device, gsdr_lib, n_frames, n_ch, k, count, kind):
    """Every pointer one sample past a 16-byte boundary inside a larger allocation, guards of NaN and of +-1e30 around
    the inputs: frames and acc_in stay untouched, out[rows * n_ch, ...) and the guards of both outputs keep their
    sentinel, acc_out is exactly n_ch samples, and the bits do not depend on any of it."""
    import torch
    import gpu_sdr_amd as g
    rng = np.random.default_rng(n_frames + n_ch)
    frames = crandn(rng, n_frames * n_ch).reshape(n_frames, n_ch)
    acc = crandn(rng, n_ch) if count else None
    want, want_acc, _ = g.frame_average(frames, k, kind, count, acc)
    rows, slack = want.shape[0], 64
    st = torch.cuda.current_stream(cuda_device)
    for pattern in ext.PATTERNS:
        f_whole, f_view = ext.guarded_input(frames.reshape(-1), 1, pattern, cuda_device)
        a_whole, a_view = ext.guarded_input(acc, 1, pattern, cuda_device) if count else (None, None)
        o_whole, o_view = ext.guarded_output(rows * n_ch + slack, 1, cuda_device)
        c_whole, c_view = ext.guarded_output(n_ch, 1, cuda_device)
        r = gsdr_lib.gsdr_frame_average_device(f_view.data_ptr(), n_frames, n_ch, k, KIND_C[kind], count,
                                               a_view.data_ptr() if count else None, c_view.data_ptr(), o_view.data_ptr(),
                                               C.c_void_p(st.cuda_stream))
        torch.cuda.synchronize()
        assert r == rows, gsdr_lib.gsdr_last_error(None)
        ext.check_input_untouched(f_whole, frames.reshape(-1), 1, pattern)
        if count:
            ext.check_input_untouched(a_whole, acc, 1, pattern)
        ext.check_output(o_whole, o_view, rows * n_ch)
        ext.check_output(c_whole, c_view, n_ch)
        tail = o_view[rows * n_ch:].cpu().numpy().view(np.uint32)
        assert (tail == ext.OUT_SENTINEL_BITS).all(), "out was written behind the rows that completed"
        np.testing.assert_array_equal(bits(o_view[:rows * n_ch].cpu().numpy()), bits(want.reshape(-1)))
        np.testing.assert_array_equal(bits(c_view.cpu().numpy()), bits(want_acc))


def test_kernel_bad_arguments(cuda_device, gsdr_lib):
    import torch
    x = torch.zeros(64, dtype=torch.complex64, device=cuda_device)       # frames [0, 12), out [16, 22), acc_out [32, 35)
    ok = lambda **kw: gsdr_lib.gsdr_frame_average_device(
        kw.get("frames", x.data_ptr()), 4, 3, kw.get("k", 2), kw.get("kind", 0), kw.get("count", 0), None,
        kw.get("acc_out", x.data_ptr() + 256), kw.get("out", x.data_ptr() + 128), None)
    for kw in (dict(k=0), dict(kind=2), dict(count=2), dict(count=1), dict(acc_out=None), dict(out=None), dict(frames=x.data_ptr() + 4)):
        assert ok(**kw) == -1, kw
        assert b"gsdr_frame_average_device" in gsdr_lib.gsdr_last_error(None)
    torch.cuda.synchronize()


# ---- 2. a handle, every PFB path ------------------------------------------------------------------------------------

def tone_freqs(nfft, rate):
    """5 tones, two of them in one bin"""
    tone_bins = [1, 3 % nfft, 3 % nfft, nfft // 2, nfft - 1]
    return [int((b if b < nfft // 2 else b - nfft) * (rate // nfft)) for b in tone_bins]


def make(mode, nfft, avg, L, freq=None, rate=None):
    import gpu_sdr_amd as g
    rate = rate or nfft * 1000
    if mode == "NOISE":
        p = g.param(mode="RX", rate=rate, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft, freq=[0],
                    wave_type=[g.w_type.NOISE])
    else:
        p = g.param(mode="RX", rate=rate, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft,
                    freq=[int(f) for f in freq], wave_type=[g.w_type.TONES] * len(freq))
    return g.RX_buffer_demodulator(p, device_index=0)


def expected_from_twin(twin_frames, n_ch, k, kind):
    """gsdr_frame_average_host over the per-call outputs of the twin, with the carried count and accumulator"""
    import gpu_sdr_amd as g
    outs, acc, c = [], None, 0
    for fr in twin_frames:
        out, acc, c = g.frame_average(np.ascontiguousarray(fr.reshape(-1, n_ch)), k, kind, c, acc if c else None)
        outs.append(out.reshape(-1))
    return outs


def group_means64(frames64, k, kind):
    n = (frames64.shape[0] // k) * k
    t = frames64[:n] if kind == "complex" else np.abs(frames64[:n]) ** 2
    return t.reshape(-1, k, frames64.shape[1]).mean(axis=1)


SHAPES = [  # nfft, avg, L, buffers, ks
    (16, 3, 200, 4, (2, 3, 7)),
    (64, 4, 9_000, 3, (2, 7)),
    (200, 4, 30_011, 3, (2, 7)),
    (512, 4, 700, 16, (2, 3)),              # calls without a frame
    (1230, 4, 60_000, 3, (2, 7)),           # matrix-core first stage
    (1018, 4, 40_000, 3, (2, 7)),           # Bluestein
    (4096, 4, 100_000, 3, (2, 7)),
]
POWER_TOO = {(16, 3), (200, 7), (1230, 2)}  # (nfft, k): these also run kind = power
PATHS = {"default": {}, "pfb_cu0": {"GSDR_PFB_CU": "0"}, "pfb_lds0": {"GSDR_PFB_LDS": "0"},
         "tones_fft0": {"GSDR_TONES_FFT": "0"}, "noise_fft0": {"GSDR_NOISE_FFT": "0"}}
_STREAMS = {}


def stream_and_oracle(oracle_mod, mode, nfft, avg, L, nbuf):
    """the input buffers of a shape and the oracle's frames of the whole stream in float64, computed once"""
    key = (mode, nfft, avg, L, nbuf)
    if key not in _STREAMS:
        rng = np.random.default_rng(nfft * 7 + L)
        xs = [crandn(rng, L) for _ in range(nbuf)]
        freq = tone_freqs(nfft, nfft * 1000) if mode == "TONES" else None
        ref = oracle_mod.Noise(nfft, avg, L) if mode == "NOISE" else oracle_mod.Pfb(freq, nfft * 1000, nfft, avg, L)
        frames = np.concatenate([ref.process(x).reshape(-1, ref.n_tones) for x in xs]).astype(np.complex128)
        ref.close()
        for a in xs + [frames]:
            a.setflags(write=False)
        _STREAMS[key] = (xs, freq, frames)
    return _STREAMS[key]


def path_cases():
    for nfft, avg, L, nbuf, ks in SHAPES:
        for mode in ("NOISE", "TONES"):
            for path in PATHS:
                if path == "tones_fft0" and mode != "TONES":
                    continue
                if path == "noise_fft0" and (mode != "NOISE" or nfft > 200):
                    continue
                yield pytest.param(mode, nfft, avg, L, nbuf, ks, path, id=f"{mode}-{nfft}-{path}")


@pytest.mark.parametrize("mode,nfft,avg,L,nbuf,ks,path", list(path_cases()))
def test_handle_every_pfb_path(cuda_device, gsdr_lib, oracle_mod, monkeypatch, mode, nfft, avg, L, nbuf, ks, path):
    import torch
    n_ch = nfft if mode == "NOISE" else 5
    # non-vacuous: at least 4 groups complete in all, and at least one call starts with an open group
    bh = oracle_mod.BufferHelper(nfft, L, avg, n_ch)
    batches = []
    for _ in range(nbuf):
        batches.append(bh.current_batch)
        bh.update()
    for k in ks:
        assert sum(batches) // k >= 4, (k, batches)
        assert any(c % k for c in np.cumsum(batches)[:-1]), (k, batches)
    for name, value in PATHS[path].items():
        monkeypatch.setenv(name, value)
    xs, freq, oracle_frames = stream_and_oracle(oracle_mod, mode, nfft, avg, L, nbuf)
    assert oracle_frames.shape[0] == sum(batches)
    twin = make(mode, nfft, avg, L, freq)
    runs = [(k, kind) for k in ks for kind in KINDS if kind == "complex" or ((nfft, k) in POWER_TOO and path == "default")]
    handles = []
    for k, kind in runs:
        h = make(mode, nfft, avg, L, freq)
        h.set_frame_average(k, kind)
        assert h.out_capacity == n_ch * math.ceil(twin.out_capacity // n_ch / k)
        assert h.kernel_name == twin.kernel_name
        handles.append(h)
    t_out = torch.empty(twin.out_capacity, dtype=torch.complex64, device=cuda_device)
    h_outs = [torch.empty(h.out_capacity, dtype=torch.complex64, device=cuda_device) for h in handles]
    twin_frames, got = [], [[] for _ in handles]
    for x in xs:
        xd = torch.tensor(x, device=cuda_device)               # (x is shared between the cases and read-only)
        n = twin.process_device(xd, t_out)
        ns = [h.process_device(xd, o) for h, o in zip(handles, h_outs)]
        torch.cuda.synchronize()
        twin_frames.append(t_out[:n].cpu().numpy())
        for i, (o, m) in enumerate(zip(h_outs, ns)):
            got[i].append(o[:m].cpu().numpy())
    assert [f.size // n_ch for f in twin_frames] == batches
    assert handles[0].kernel_name == twin.kernel_name          # the PFB kernel, not the averaging one
    for (k, kind), h, outs in zip(runs, handles, got):
        want = expected_from_twin(twin_frames, n_ch, k, kind)
        assert [o.size for o in outs] == [w.size for w in want], (k, kind)          # lengths, call by call
        for c, (o, w) in enumerate(zip(outs, want)):
            np.testing.assert_array_equal(bits(o), bits(w), err_msg=f"k={k} {kind} call {c}")   # (a)
        y = np.concatenate(outs).reshape(-1, n_ch).astype(np.complex128)
        ref = group_means64(oracle_frames, k, kind)
        assert y.shape == ref.shape
        err = np.linalg.norm(y - ref, axis=0) / np.linalg.norm(ref, axis=0)                         # (b)
        record_margin(float(err.max()), f"k={k} {kind}")
        print(f"frame average {mode} nfft {nfft} {path} k={k} {kind}: worst per-channel relative error {err.max():.3e}")
        assert err.max() <= TOL, (k, kind, float(err.max()))
        h.close()
    twin.close()


# ---- 3. every entry -------------------------------------------------------------------------------------------------

ENTRIES = ["process", "process_device", "submit", "submit_device"]


class EntryRunner:
    """feeds buffers to a handle through one entry at a time; `flush()` waits for what is outstanding"""

    def __init__(self, h, dev):
        import torch
        self.h, self.dev, self.torch = h, dev, torch
        self.streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        self.pending, self.results, self.calls, self.keep = [], [], 0, []

    def flush(self, down_to=0):
        while len(self.pending) > down_to:
            out = self.pending.pop(0)
            n = self.h.wait()
            self.results.append((out[:n].cpu().numpy() if self.torch.is_tensor(out) else out[:n]).copy())

    def collect(self):
        """per call, in order; the process_device calls are read only now: nothing synchronised between them"""
        self.flush()
        self.torch.cuda.synchronize()
        return [r[0][:r[1]].cpu().numpy() if isinstance(r, tuple) else r for r in self.results]

    def feed(self, entry, x):
        torch, h = self.torch, self.h
        pipelined = entry.startswith("submit")
        if not pipelined:
            self.flush()
        elif len(self.pending) == 4:                       # GSDR_PIPELINE_DEPTH outstanding
            self.flush(3)
        if entry.endswith("device"):
            xd = torch.from_numpy(x).to(self.dev)
            out = torch.empty(h.out_capacity, dtype=torch.complex64, device=self.dev)
            if pipelined:
                torch.cuda.current_stream(self.dev).synchronize()        # submit_device: the input must be complete
            else:
                for st in self.streams:
                    st.wait_stream(torch.cuda.current_stream(self.dev))  # the upload only
            self.keep += [xd, out]
        else:
            out = np.empty(h.out_capacity, dtype=np.complex64)
            self.keep += [x, out]
        if entry == "process":
            self.results.append(out[:h.process(x, out)].copy())
        elif entry == "process_device":
            st = self.streams[self.calls % 2]
            n = h.process_device(xd, out, stream=st)     # ordered behind the call before by the handle alone
            self.results.append((out, n))
        elif entry == "submit":
            h.submit(x, out)
            self.pending.append(out)
        else:
            h.submit_device(xd, out)
            self.pending.append(out)
        self.calls += 1


ENTRY_SHAPES = {
    "NOISE": dict(mode="NOISE", nfft=200, avg=4, L=30_011, rate=200_000, env={}),
    # TONES bin by bin on the matrix cores: the path whose pipelined entries rotate over three compute streams
    "TONES_ddc": dict(mode="TONES", nfft=250, avg=4, L=100_003, rate=10_000_000,
                      env={"GSDR_TONES_FFT": "0", "GSDR_DDC_MFMA": "1"}),
}


@pytest.mark.parametrize("shape", list(ENTRY_SHAPES))
def test_every_entry_same_bits_and_lengths(cuda_device, gsdr_lib, monkeypatch, shape):
    """k = 7, nine buffers of sc16-representable samples: process / process_device on two alternating streams / submit
    with GSDR_PIPELINE_DEPTH outstanding / submit_device, each in its complex64 and its sc16 form (the complex64 form
    and the twin are fed the widened samples), and one handle that changes entry with every buffer."""
    import torch
    import gpu_sdr_amd as g
    s = ENTRY_SHAPES[shape]
    for name, value in s["env"].items():
        monkeypatch.setenv(name, value)
    k, nbuf, L = 7, 9, s["L"]
    rng = np.random.default_rng(99)
    x16 = [rng.integers(-20000, 20000, size=(L, 2), dtype=np.int16) for _ in range(nbuf)]
    xw = [g.widen_sc16(a) for a in x16]
    freq = None
    if s["mode"] == "TONES":
        freq = rng.choice(np.arange(-s["rate"] // 2 + 1, s["rate"] // 2), size=96, replace=False)
    n_ch = s["nfft"] if s["mode"] == "NOISE" else 96
    twin = make(s["mode"], s["nfft"], s["avg"], L, freq, s["rate"])
    if shape == "TONES_ddc":
        assert twin.kernel_name.startswith("ddc_mfma"), twin.kernel_name
    t_out = torch.empty(twin.out_capacity, dtype=torch.complex64, device=cuda_device)
    twin_frames = []
    for x in xw:
        n = twin.process_device(torch.from_numpy(x).to(cuda_device), t_out)
        torch.cuda.synchronize()
        twin_frames.append(t_out[:n].cpu().numpy())
    twin.close()
    want = expected_from_twin(twin_frames, n_ch, k, "complex")
    assert sum(w.size for w in want) // n_ch >= 4 and len({w.size for w in want}) > 1

    def run(plan):
        h = make(s["mode"], s["nfft"], s["avg"], L, freq, s["rate"])
        h.set_frame_average(k)
        r = EntryRunner(h, cuda_device)
        for c, (entry, sc16) in enumerate(plan):
            r.feed(entry, x16[c] if sc16 else xw[c])
        res = r.collect()
        h.close()
        return res

    plans = {f"{e}{'_sc16' if sc else ''}": [(e, sc)] * nbuf for e in ENTRIES for sc in (False, True)}
    mixed = [(ENTRIES[(c // 2) % 4], bool(c % 2)) for c in range(nbuf)]
    plans["mixed"] = mixed
    plans["mixed_pipelined_first"] = [(ENTRIES[(2 + c) % 4], bool((c // 3) % 2)) for c in range(nbuf)]
    for name, plan in plans.items():
        got = run(plan)
        assert [o.size for o in got] == [w.size for w in want], name
        for c, (o, w) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(bits(o), bits(w), err_msg=f"{name}, call {c}")


# ---- 4. the surface -------------------------------------------------------------------------------------------------

def test_k1_is_the_parents_path(cuda_device, gsdr_lib):
    import torch
    nfft, avg, L = 200, 4, 30_011
    rng = np.random.default_rng(3)
    a, b = make("NOISE", nfft, avg, L), make("NOISE", nfft, avg, L)
    assert b.frame_average == 1 and b.frame_average_kind == "complex"
    b.set_frame_average(5, "power")
    assert (b.frame_average, b.frame_average_kind) == (5, "power")
    b.set_frame_average(1)                                   # off again, before the first buffer
    assert b.frame_average == 1 and b.out_capacity == a.out_capacity and b.kernel_name == a.kernel_name
    d = b.describe()
    assert d["frame_average"] == 1 and d["frame_average_kind"] == "complex"
    oa = torch.empty(a.out_capacity, dtype=torch.complex64, device=cuda_device)
    ob = torch.empty(b.out_capacity, dtype=torch.complex64, device=cuda_device)
    for _ in range(3):
        x = torch.from_numpy(crandn(rng, L)).to(cuda_device)
        na, nb = a.process_device(x, oa), b.process_device(x, ob)
        torch.cuda.synchronize()
        assert na == nb and a.kernel_name == b.kernel_name
        np.testing.assert_array_equal(bits(oa[:na].cpu().numpy()), bits(ob[:nb].cpu().numpy()))
    a.close()
    b.close()


def test_setter_refusals_keep_the_old_setting(cuda_device, gsdr_lib):
    import torch
    import gpu_sdr_amd as g
    nfft, avg, L = 64, 4, 9_000
    h = make("TONES", nfft, avg, L, tone_freqs(nfft, nfft * 1000))
    batching = h.out_capacity // 5
    h.set_frame_average(3, "power")
    assert h.out_capacity == 5 * math.ceil(batching / 3)
    d = h.describe()
    assert d["frame_average"] == 3 and d["frame_average_kind"] == "power"
    for k, kind in ((0, 0), (-1, 0), ((1 << 20) + 1, 0), (2, 2), (2, -1)):
        with pytest.raises(g.GsdrError, match="frame average"):
            h.set_frame_average(k, kind)
        assert (h.frame_average, h.frame_average_kind) == (3, "power") and h.out_capacity == 5 * math.ceil(batching / 3)
    h.prepare(rehearse=True, sc16=True)                      # covers the averaging kernel; the stream state is untouched
    x = torch.zeros(L, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(h.out_capacity, dtype=torch.complex64, device=cuda_device)
    n = h.process_device(x, out)
    torch.cuda.synchronize()
    assert n % 5 == 0 and 0 < n <= h.out_capacity
    with pytest.raises(g.GsdrError, match="before the first buffer"):
        h.set_frame_average(2)
    assert (h.frame_average, h.frame_average_kind) == (3, "power")
    h.close()
    # handles without frames
    rate = 1_000_000
    others = [g.param(mode="RX", rate=rate, buffer_len=50_000, decim=50, pf_average=4, freq=[1000, 2000], wave_type=[g.w_type.DIRECT] * 2),
              g.param(mode="RX", rate=rate, buffer_len=50_000, decim=0, freq=[-400_000], chirp_f=[400_000], swipe_s=[1000],
                      chirp_t=[0.01], wave_type=[g.w_type.CHIRP]),
              g.param(mode="RX", rate=rate, buffer_len=50_000, decim=0, freq=[0], wave_type=[g.w_type.NODSP])]
    for p in others:
        dem = g.RX_buffer_demodulator(p, device_index=0)
        cap = dem.out_capacity
        with pytest.raises(g.GsdrError, match="TONES and NOISE"):
            dem.set_frame_average(2)
        assert dem.frame_average == 1 and dem.out_capacity == cap
        dem.close()
    # param::decim keeps meaning the reference's path
    for wt, freq in ((g.w_type.NOISE, [0]), (g.w_type.TONES, [1000])):
        with pytest.raises(g.GsdrError, match="not supported"):
            g.RX_buffer_demodulator(g.param(mode="RX", rate=rate, buffer_len=50_000, decim=2, pf_average=4, fft_tones=100,
                                            freq=freq, wave_type=[wt]), device_index=0)


def test_setter_refused_with_a_buffer_outstanding(cuda_device, gsdr_lib):
    import torch
    import gpu_sdr_amd as g
    h = make("NOISE", 64, 4, 9_000)
    x = torch.zeros(9_000, dtype=torch.complex64, device=cuda_device)
    out = torch.empty(h.out_capacity, dtype=torch.complex64, device=cuda_device)
    h.submit_device(x, out)
    with pytest.raises(g.GsdrError, match="before the first buffer"):
        h.set_frame_average(2)
    h.wait()
    assert h.frame_average == 1
    h.close()


# ---- 5. rx_link and the server --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipe", [False, True], ids=["process", "submit_wait"])
def test_rx_link_frame_average(cuda_device, gsdr_lib, tmp_path, pipe):
    """`frame_average 7` in the config of rx_link's file mode (RX_buffer_demodulator::set_frame_average) against the
    host function applied to the frames of the same run without that line."""
    from test_gpu_rxlink import run_rx_link
    rate, nfft, avg, L, nbuf, k = 1_000_000, 100, 4, 100_037, 6, 7
    bins_ = [0, 3, 17, 50, 77, 99]
    freq = [int((b if b < nfft // 2 else b - nfft) * (rate // nfft)) for b in bins_]
    rng = np.random.default_rng(8)
    x = crandn(rng, L * nbuf)
    cfg = ["mode TONES", f"rate {rate}", f"buffer_len {L}", "decim 0", f"pf_average {avg}", f"fft_tones {nfft}",
           "freq " + " ".join(map(str, freq))]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    info0, y0 = run_rx_link(tmp_path / "a", cfg, x, pipe)
    info, y = run_rx_link(tmp_path / "b", cfg + [f"frame_average {k}"], x, pipe)
    frames = np.split(y0, np.cumsum(info0["lengths"])[:-1])
    want = expected_from_twin(frames, len(freq), k, "complex")
    assert info["lengths"] == [w.size for w in want] and sum(info["lengths"]) >= 4 * len(freq)
    np.testing.assert_array_equal(bits(y), bits(np.concatenate(want)))


from test_gpu_server import server  # noqa: E402,F401  (the fixture that starts gsdr_server)


def test_server_maps_decim_of_a_noise_command_to_the_frame_average(server, oracle_mod):
    """tests/golden/cmd_noise_decim.json: a NOISE command with decim = 4 (pyUSRP's Get_full_spec(decimation=4)) on the
    software loop-back, one TX tone in every bin.  The packets carry the oracle's frames averaged in fours; calls that
    complete no group send nothing, `length` follows the rows, and the lengths sum to the expected count."""
    from test_gpu_server import HEADER, recv_all, recv_async, send_command
    asyn, data = server
    cmd = json.load(open(os.path.join(ROOT, "tests", "golden", "cmd_noise_decim.json")))
    rx, tx = cmd["A_RX2"], cmd["A_TXRX"]
    assert rx["wave_type"] == ["NOISE"] and rx["decim"] == 4
    rate, L, nfft, avg, k = int(rx["rate"]), int(rx["buffer_len"]), int(rx["fft_tones"]), int(rx["pf_average"]), int(rx["decim"])
    nbuf = -(-int(rx["samples"]) // L)
    ref = oracle_mod.Noise(nfft, avg, L)
    frames = np.concatenate([ref.process(oracle_mod.tone_gen(tx["freq"], tx["ampl"], rate, c * L, L)).reshape(-1, nfft)
                             for c in range(nbuf)]).astype(np.complex128)
    want = group_means64(frames, k, "complex")
    assert want.shape[0] >= 4
    send_command(asyn, cmd)
    assert recv_async(asyn) == {"type": "ack", "payload": "Message received"}
    got, total, packet = [], 0, 0
    while total < want.size:
        h = np.frombuffer(recv_all(data, 21), dtype=HEADER)[0]
        assert (h["front_end_code"], h["packet_number"], h["errors"], h["channels"]) == (b"B", packet, 0, 1)
        assert h["length"] > 0 and h["length"] % nfft == 0
        got.append(np.frombuffer(recv_all(data, int(h["length"]) * 8), dtype=np.complex64))
        total += int(h["length"])
        packet += 1
    reply = recv_async(asyn)
    assert reply["type"] == "ack" and "EOM" in reply["payload"]
    assert total == want.size
    y = np.concatenate(got).reshape(-1, nfft).astype(np.complex128)
    err = np.linalg.norm(y - want, axis=0) / np.linalg.norm(want, axis=0)
    record_margin(float(err.max()))
    assert err.max() <= TOL, float(err.max())
