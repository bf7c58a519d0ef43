"""Host-side mirror of the reference's demodulator interface over the C ABI.

Same names and argument meaning as the C++ the server uses:
  * ``w_type`` / ``string_to_w_type``  -- headers/USRP_server_settings.hpp:114,
    cpp/USRP_server_settings.cpp:38-54
  * ``param``                          -- headers/USRP_server_settings.hpp:130-167
  * ``RX_wrapper``                     -- headers/USRP_server_settings.hpp:216-224
  * ``RX_buffer_demodulator``          -- headers/USRP_demodulator.hpp:13-33
(citations relative to /root/reference).

All arithmetic happens in libgsdr.so (HIP); this module only marshals
parameters and pointers.  torch is used for device memory and stream handles.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib


class GsdrError(RuntimeError):
    """Raised where the reference would print_error() and exit(-1), and on
    device errors (the reference ignores CUDA return codes)."""


class w_type(enum.IntEnum):
    """enum w_type, headers/USRP_server_settings.hpp:114"""
    TONES = 0
    CHIRP = 1
    NOISE = 2
    RAMP = 3
    NODSP = 4
    SWONLY = 5
    DIRECT = 6


def string_to_w_type(s: str) -> w_type:
    """cpp/USRP_server_settings.cpp:38-54: unknown strings (and "RAMP") map to NODSP."""
    return {"NODSP": w_type.NODSP, "CHIRP": w_type.CHIRP, "NOISE": w_type.NOISE,
            "TONES": w_type.TONES, "SWONLY": w_type.SWONLY, "DIRECT": w_type.DIRECT}.get(
                s, w_type.NODSP)


def w_type_to_str(w: w_type) -> str:
    """cpp/USRP_server_settings.cpp:9-36"""
    try:
        return w_type(w).name
    except ValueError:
        return "UNINIT"


@dataclass
class param:
    """struct param, headers/USRP_server_settings.hpp:130-167 (RX-relevant defaults
    follow the client's, pyUSRP/USRP_files.py:449-478)."""
    mode: str = "OFF"
    rate: int = 0
    gain: int = 0
    bw: int = 0
    tone: int = 0
    samples: int = 0
    delay: float = 1.0
    burst_on: float = 0.0
    burst_off: float = 0.0
    buffer_len: int = 1000000
    tuning_mode: bool = True
    freq: List[int] = field(default_factory=list)
    wave_type: List[w_type] = field(default_factory=list)
    ampl: List[float] = field(default_factory=list)
    decim: int = 0
    chirp_t: List[float] = field(default_factory=list)
    chirp_f: List[int] = field(default_factory=list)
    swipe_s: List[int] = field(default_factory=list)
    data_mem_mult: int = 1
    fft_tones: int = 0
    pf_average: int = 4


@dataclass
class RX_wrapper:
    """struct RX_wrapper, headers/USRP_server_settings.hpp:216-224"""
    buffer: object = None
    usrp_number: int = 0
    front_end_code: str = "A"
    packet_number: int = 0
    length: int = 0
    errors: int = 0
    channels: int = 0


def _carr(values, ctype):
    arr = (ctype * max(len(values), 1))(*values)
    return arr, C.cast(arr, C.POINTER(ctype))


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


SC16_DEFAULT_SCALE = 2.0 ** -15
AVERAGE_KINDS = ("complex", "power")       # GSDR_AVERAGE_COMPLEX, GSDR_AVERAGE_POWER


def _average_kind(kind) -> int:
    if kind in AVERAGE_KINDS:
        return AVERAGE_KINDS.index(kind)
    if isinstance(kind, int) and not isinstance(kind, bool):
        return kind                        # the library checks the value
    raise ValueError('kind must be "complex" or "power"')


def _is_sc16(x) -> bool:
    """An sc16 buffer: contiguous int16 array or tensor of shape (..., 2), I first (struct gsdr_sc16)."""
    if _is_torch(x):
        import torch
        return x.dtype == torch.int16 and x.dim() >= 2 and x.shape[-1] == 2 and x.is_contiguous()
    return (isinstance(x, np.ndarray) and x.dtype == np.int16 and x.ndim >= 2 and x.shape[-1] == 2
            and x.flags.c_contiguous)


def _sc16_rows(x) -> int:
    return int(x.numel() if _is_torch(x) else x.size) // 2


class RX_buffer_demodulator:
    """class RX_buffer_demodulator, headers/USRP_demodulator.hpp:13-33.

    ``process(in, out)`` returns the number of valid complex samples written to
    ``out`` (all channels interleaved [sample][channel]); ``close()`` releases
    the device state.  ``in``/``out`` are numpy complex64 arrays (host path,
    synchronous like the reference) or torch complex64 CUDA tensors (device
    path, enqueued on the current torch stream, not synchronised).

    sc16 input: ``process``, ``process_device``, ``submit`` and ``submit_device`` also take ``in`` as a contiguous
    int16 array / CUDA tensor of shape (..., 2) (I, Q) with at least buffer_len rows; it is widened to
    ``float(v) * sc16_scale`` on the way in (gsdr_demod_*_sc16) and demodulated as the complex64 it stands for.
    """

    def __init__(self, init_parameters: param, init_diagnostic: bool = False,
                 device_index: int = -1, multi_chirp: bool = False):
        self.parameters = init_parameters
        self.diagnostic = bool(init_diagnostic)
        L = _lib.lib()
        p = init_parameters
        keep = []
        pc = _lib.ParamC()
        pc.rate = int(p.rate)
        pc.decim = int(p.decim)
        pc.fft_tones = int(p.fft_tones)
        pc.pf_average = int(p.pf_average)
        pc.buffer_len = int(p.buffer_len)
        a, pc.wave_type = _carr([int(w) for w in p.wave_type], C.c_int); keep.append(a)
        pc.n_wave_type = len(p.wave_type)
        a, pc.freq = _carr([int(f) for f in p.freq], C.c_int); keep.append(a)
        pc.n_freq = len(p.freq)
        a, pc.chirp_t = _carr([float(f) for f in p.chirp_t], C.c_float); keep.append(a)
        pc.n_chirp_t = len(p.chirp_t)
        a, pc.chirp_f = _carr([int(f) for f in p.chirp_f], C.c_int); keep.append(a)
        pc.n_chirp_f = len(p.chirp_f)
        a, pc.swipe_s = _carr([int(f) for f in p.swipe_s], C.c_int); keep.append(a)
        pc.n_swipe_s = len(p.swipe_s)
        pc.device_index = int(device_index)
        self._L = L
        # multi_chirp: wave_type = CHIRP x C demodulates C chirps in one pass (GSDR_CREATE_MULTI_CHIRP), rows
        # [point][chirp]; without it the request is refused as the reference refuses it
        if multi_chirp:
            self._h = L.gsdr_demod_create_ex(C.byref(pc), _lib.CREATE_MULTI_CHIRP)
        else:
            self._h = L.gsdr_demod_create(C.byref(pc))
        if not self._h:
            raise GsdrError(L.gsdr_last_error(None).decode())
        self.fcut = float(L.gsdr_demod_fcut(self._h))
        if self.diagnostic and self.mode in (w_type.TONES, w_type.NOISE):
            # ref: make_sinc_window(..., diagnostic, ...) dumps the window,
            # cpp/kernels.cu:290-296 (float2 records, imag = 0)
            w = self.window()
            rec = np.zeros((len(w), 2), dtype=np.float32)
            rec[:, 0] = w
            rec.tofile("USRP_polyphase_filter_window.dat")

    # -- introspection ------------------------------------------------------
    @property
    def mode(self) -> w_type:
        return w_type(self._L.gsdr_demod_mode(self._h))

    @property
    def channels(self) -> int:
        return self._L.gsdr_demod_channels(self._h)

    @property
    def out_capacity(self) -> int:
        return int(self._L.gsdr_demod_out_capacity(self._h))

    @property
    def kernel_name(self) -> str:
        return self._L.gsdr_demod_kernel_name(self._h).decode()

    @property
    def sc16_scale(self) -> float:
        """Factor of the sc16 widening (gsdr_demod_sc16_scale); 2^-15 unless set.  Must be finite and > 0."""
        return float(self._L.gsdr_demod_sc16_scale(self._h))

    @sc16_scale.setter
    def sc16_scale(self, scale: float) -> None:
        if self._L.gsdr_demod_set_sc16_scale(self._h, C.c_float(scale)) != 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())

    @property
    def frame_average(self) -> int:
        """k of the frame averaging (gsdr_demod_frame_average): frames per returned row; 1 is off."""
        return int(self._L.gsdr_demod_frame_average(self._h, None))

    @property
    def frame_average_kind(self) -> str:
        """"complex" or "power" (set_frame_average)."""
        kind = C.c_int(0)
        self._L.gsdr_demod_frame_average(self._h, C.byref(kind))
        return AVERAGE_KINDS[kind.value]

    def set_frame_average(self, k: int, kind="complex") -> None:
        """TONES / NOISE: return the mean of every k consecutive frames per channel instead of the frames
        (gsdr_demod_set_frame_average; rows [group][channel], ``out_capacity`` shrinks to channels * ceil(batching / k),
        a call returns the groups that complete in it, possibly none).  kind "complex": mean of the complex frames;
        "power": mean of |X|^2 in the real part.  Only before the first buffer; k = 1 switches it off."""
        if self._L.gsdr_demod_set_frame_average(self._h, int(k), _average_kind(kind)) != 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())

    def prepare(self, host: bool = True, pipeline: bool = True, pipeline_host: bool = True, rehearse: bool = True,
                sc16: bool = False) -> None:
        """gsdr_demod_prepare: create now what the entries would create on first use; `rehearse` also runs a
        throw-away twin through a few buffers of zeros (the process-wide first-use costs of kernels, pinned
        copies and streams: 5 - 7 ms each, otherwise paid by the first packets); `sc16`: the same for the sc16
        forms of the entries named (GSDR_PREPARE_SC16)."""
        what = (1 if host else 0) | (2 if pipeline else 0) | (4 if pipeline_host else 0) | (8 if rehearse else 0)
        what |= 16 if sc16 else 0
        if self._L.gsdr_demod_prepare(self._h, what) != 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())

    def describe(self) -> dict:
        """The engine this handle resolved to (gsdr_demod_describe): dominant kernel, family,
        row tiles per workgroup, pipeline streams, every GSDR_* variable set in the process.  TONES / NOISE
        handles inside the LDS add "pfb_last" (the shape of the last call, as gsdr_pfb_plan gives it) and
        "pfb_calls" (the calls so far by kernel, filter variant, teams, runs and short last runs)."""
        import json
        buf = C.create_string_buffer(4096)
        self._L.gsdr_demod_describe(self._h, buf, len(buf))
        return json.loads(buf.value.decode())

    def window(self) -> np.ndarray:
        n = self._L.gsdr_demod_get_window(self._h, None, 0)
        w = np.empty(n, dtype=np.float32)
        self._L.gsdr_demod_get_window(self._h, w.ctypes.data_as(C.POINTER(C.c_float)), n)
        return w

    def bins(self) -> np.ndarray:
        n = self._L.gsdr_demod_get_bins(self._h, None, 0)
        b = np.empty(n, dtype=np.int32)
        self._L.gsdr_demod_get_bins(self._h, b.ctypes.data_as(C.POINTER(C.c_int)), n)
        return b

    # -- the hot path ---------------------------------------------------------
    def process(self, in_buffer, out_buffer) -> int:
        if not self._h:
            raise GsdrError("demodulator is closed")
        if _is_torch(in_buffer) or _is_torch(out_buffer):
            return self.process_device(in_buffer, out_buffer)
        sc16 = _is_sc16(in_buffer)
        if not (sc16 or in_buffer.dtype == np.complex64) or out_buffer.dtype != np.complex64:
            raise TypeError("buffers must be complex64 (float2); the input may be contiguous int16 of shape (..., 2)")
        if (_sc16_rows(in_buffer) if sc16 else in_buffer.size) < self.parameters.buffer_len:
            raise ValueError("input buffer shorter than parameters.buffer_len")
        if out_buffer.size < self.out_capacity:
            raise ValueError(f"output buffer needs room for {self.out_capacity} samples")
        if not (in_buffer.flags.c_contiguous and out_buffer.flags.c_contiguous):
            raise ValueError("buffers must be contiguous")
        entry = self._L.gsdr_demod_process_sc16 if sc16 else self._L.gsdr_demod_process
        n = entry(self._h, in_buffer.ctypes.data, out_buffer.ctypes.data)
        if n < 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())
        return n

    def process_device(self, in_tensor, out_tensor, stream=None) -> int:
        """Device-pointer entry (gsdr_demod_process_device); asynchronous."""
        import torch
        if not self._h:
            raise GsdrError("demodulator is closed")
        sc16 = self._check_tensors(in_tensor, out_tensor)
        if (_sc16_rows(in_tensor) if sc16 else in_tensor.numel()) < self.parameters.buffer_len:
            raise ValueError("input tensor shorter than parameters.buffer_len")
        if out_tensor.numel() < self.out_capacity:
            raise ValueError(f"output tensor needs room for {self.out_capacity} samples")
        if stream is None:
            stream = torch.cuda.current_stream(in_tensor.device)
        entry = self._L.gsdr_demod_process_device_sc16 if sc16 else self._L.gsdr_demod_process_device
        n = entry(self._h, in_tensor.data_ptr(), out_tensor.data_ptr(), C.c_void_p(stream.cuda_stream))
        if n < 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())
        return n

    @staticmethod
    def _check_tensors(in_tensor, out_tensor) -> bool:
        """TypeError unless both are contiguous CUDA tensors, complex64 -- or, the input only, sc16: True then."""
        import torch
        sc16 = _is_sc16(in_tensor)
        for t, ok in ((in_tensor, sc16 or in_tensor.dtype == torch.complex64), (out_tensor, out_tensor.dtype == torch.complex64)):
            if not (t.is_cuda and ok and t.is_contiguous()):
                raise TypeError("need contiguous complex64 CUDA tensors (the input may be contiguous int16 of shape (..., 2))")
        return sc16

    def submit(self, in_buffer: np.ndarray, out_buffer: np.ndarray) -> None:
        """Pipelined host-pointer entry (gsdr_demod_submit): returns at once; the
        buffers (ideally pinned) must stay alive until the matching wait()."""
        sc16 = _is_sc16(in_buffer)
        if not (sc16 or in_buffer.dtype == np.complex64) or out_buffer.dtype != np.complex64:
            raise TypeError("buffers must be complex64 (float2); the input may be contiguous int16 of shape (..., 2)")
        rows = _sc16_rows(in_buffer) if sc16 else in_buffer.size
        if rows < self.parameters.buffer_len or out_buffer.size < self.out_capacity:
            raise ValueError("buffer too small")
        entry = self._L.gsdr_demod_submit_sc16 if sc16 else self._L.gsdr_demod_submit
        if entry(self._h, in_buffer.ctypes.data, out_buffer.ctypes.data) != 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())

    def submit_device(self, in_tensor, out_tensor) -> None:
        """Pipelined device-pointer entry (gsdr_demod_submit_device): in_tensor must be
        complete (synchronise its producer first), out_tensor distinct per outstanding call."""
        if not self._h:
            raise GsdrError("demodulator is closed")
        sc16 = self._check_tensors(in_tensor, out_tensor)
        rows = _sc16_rows(in_tensor) if sc16 else in_tensor.numel()
        if rows < self.parameters.buffer_len or out_tensor.numel() < self.out_capacity:
            raise ValueError("tensor too small")
        entry = self._L.gsdr_demod_submit_device_sc16 if sc16 else self._L.gsdr_demod_submit_device
        if entry(self._h, in_tensor.data_ptr(), out_tensor.data_ptr()) != 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())

    def wait(self) -> int:
        """Valid length of the oldest submitted buffer (gsdr_demod_wait)."""
        n = self._L.gsdr_demod_wait(self._h)
        if n == -2:
            raise GsdrError("nothing outstanding")
        if n < 0:
            raise GsdrError(self._L.gsdr_last_error(self._h).decode())
        return n

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.gsdr_demod_close(self._h)
            self._h = None

    # -- kernel timing (hipEvents on the launch stream) ----------------------
    def profile_enable(self, on=True) -> None:
        """on = True / 1: time every launch; an integer n > 1: every n-th launch."""
        self._L.gsdr_demod_profile_enable(self._h, int(on))

    def profile_read(self):
        ms = C.c_double(0.0)
        n = self._L.gsdr_demod_profile_read(self._h, C.byref(ms))
        return n, ms.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def widen_sc16(in_buffer, out=None, scale: float = SC16_DEFAULT_SCALE, stream=None):
    """sc16 -> complex64 on its own: ``out[k] = (float(in[k, 0]) * scale, float(in[k, 1]) * scale)``, an exact
    conversion and one float32 multiply.  ``in_buffer``: contiguous int16 of shape (..., 2); a CUDA tensor is
    widened on the device (gsdr_widen_sc16_device, enqueued on `stream` / the current torch stream, not
    synchronised), a numpy array on the host (gsdr_widen_sc16_host, needs no GPU) -- bit-identical results.
    ``out``: contiguous complex64 of at least as many samples (created when None).  Returns ``out``."""
    if not _is_sc16(in_buffer):
        raise TypeError("need a contiguous int16 array or tensor of shape (..., 2)")
    n = _sc16_rows(in_buffer)
    L = _lib.lib()
    if _is_torch(in_buffer):
        import torch
        if not in_buffer.is_cuda:
            raise TypeError("a tensor must live on the GPU (pass a numpy array for the host path)")
        if out is None:
            out = torch.empty(in_buffer.shape[:-1], dtype=torch.complex64, device=in_buffer.device)
        if not (_is_torch(out) and out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous()):
            raise TypeError("out must be a contiguous complex64 CUDA tensor")
        if out.numel() < n:
            raise ValueError("out is shorter than the input")
        if stream is None:
            stream = torch.cuda.current_stream(in_buffer.device)
        if L.gsdr_widen_sc16_device(in_buffer.data_ptr(), out.data_ptr(), n, C.c_float(scale),
                                    C.c_void_p(stream.cuda_stream)) != 0:
            raise GsdrError(L.gsdr_last_error(None).decode())
        return out
    if out is None:
        out = np.empty(in_buffer.shape[:-1], dtype=np.complex64)
    if not (isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.flags.c_contiguous):
        raise TypeError("out must be a contiguous complex64 array")
    if out.size < n:
        raise ValueError("out is shorter than the input")
    L.gsdr_widen_sc16_host(in_buffer.ctypes.data, out.ctypes.data, n, C.c_float(scale))
    return out


SC16_DEFAULT_GAIN = 32767.0


def _check_sc16_gain(gain) -> float:
    gain = float(np.float32(gain))
    if not (np.isfinite(gain) and gain > 0):
        raise ValueError("the sc16 gain must be finite and > 0")
    return gain


def narrow_sc16(in_buffer, out=None, gain: float = SC16_DEFAULT_GAIN, stream=None, clipped=None, return_clipped: bool = False):
    """complex64 -> sc16 on its own (include/gsdr.h, "sc16 output"): per component ``v = float32(c * gain)``, rounded to
    the nearest integer (ties to even), saturated to [-32768, 32767], NaN -> 0.  ``in_buffer``: contiguous complex64; a
    CUDA tensor is narrowed on the device (gsdr_narrow_sc16_device, enqueued on `stream` / the current torch stream,
    not synchronised), a numpy array on the host (gsdr_narrow_sc16_host, needs no GPU) -- bit-identical results.
    ``out``: contiguous int16 of shape (..., 2) with at least as many samples (created when None).
    ``clipped`` (device path): a one-element int64 CUDA tensor the kernel ADDS the number of clipped components to.
    Returns ``out``; the host path returns ``(out, count)`` with ``return_clipped=True``."""
    gain = _check_sc16_gain(gain)
    L = _lib.lib()
    if _is_torch(in_buffer):
        import torch
        if not (in_buffer.is_cuda and in_buffer.dtype == torch.complex64 and in_buffer.is_contiguous()):
            raise TypeError("need a contiguous complex64 CUDA tensor (pass a numpy array for the host path)")
        if return_clipped:
            raise ValueError("return_clipped is for the host path: pass a `clipped` tensor on the device path")
        n = int(in_buffer.numel())
        if out is None:
            out = torch.empty(tuple(in_buffer.shape) + (2,), dtype=torch.int16, device=in_buffer.device)
        if not (_is_sc16(out) and _is_torch(out) and out.is_cuda):
            raise TypeError("out must be a contiguous int16 CUDA tensor of shape (..., 2)")
        if _sc16_rows(out) < n:
            raise ValueError("out is shorter than the input")
        cptr = None
        if clipped is not None:
            if not (_is_torch(clipped) and clipped.is_cuda and clipped.dtype == torch.int64 and clipped.numel() == 1):
                raise TypeError("clipped must be a one-element int64 CUDA tensor")
            cptr = clipped.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(in_buffer.device)
        if L.gsdr_narrow_sc16_device(in_buffer.data_ptr(), out.data_ptr(), n, C.c_float(gain), cptr,
                                     C.c_void_p(stream.cuda_stream)) != 0:
            raise GsdrError(L.gsdr_last_error(None).decode())
        return out
    if not (isinstance(in_buffer, np.ndarray) and in_buffer.dtype == np.complex64 and in_buffer.flags.c_contiguous):
        raise TypeError("need a contiguous complex64 array or tensor")
    if clipped is not None:
        raise ValueError("clipped is for the device path: use return_clipped=True on the host path")
    n = int(in_buffer.size)
    if out is None:
        out = np.empty(in_buffer.shape + (2,), dtype=np.int16)
    if not (_is_sc16(out) and isinstance(out, np.ndarray)):
        raise TypeError("out must be a contiguous int16 array of shape (..., 2)")
    if _sc16_rows(out) < n:
        raise ValueError("out is shorter than the input")
    count = int(L.gsdr_narrow_sc16_host(in_buffer.ctypes.data, out.ctypes.data, n, C.c_float(gain)))
    return (out, count) if return_clipped else out


def frame_average(frames, k: int, kind="complex", count: int = 0, acc=None, stream=None):
    """The frame averaging on its own (gsdr_frame_average_device / _host, bit-identical): ``frames`` is complex64 of
    shape (n_frames, n_ch) -- a CUDA tensor (one kernel on `stream` / the current torch stream, not synchronised) or a
    numpy array (host, needs no GPU) --, ``count`` < k frames of the open group are already summed in ``acc`` (n_ch).
    Returns ``(out, acc_out, count_out)``: the groups that completed, (rows, n_ch); the sums of the group left open
    (zeros when none is); and its frame count, to be passed to the next call."""
    kind_c = _average_kind(kind)
    if len(frames.shape) != 2 or frames.shape[1] < 1:
        raise ValueError("frames must have shape (n_frames, n_ch) with n_ch >= 1")
    n_frames, n_ch = int(frames.shape[0]), int(frames.shape[1])
    k, count = int(k), int(count)
    if k < 1 or not 0 <= count < k:
        raise ValueError("need k >= 1 and 0 <= count < k")
    if count > 0 and acc is None:
        raise ValueError("count > 0 needs the accumulator of the call before")
    rows = (count + n_frames) // k
    L = _lib.lib()
    if _is_torch(frames):
        import torch
        def ok(t, n):
            return _is_torch(t) and t.is_cuda and t.dtype == torch.complex64 and t.is_contiguous() and t.numel() == n
        if not ok(frames, n_frames * n_ch) or (acc is not None and not ok(acc, n_ch)):
            raise TypeError("need contiguous complex64 CUDA tensors; acc holds n_ch samples")
        out = torch.empty((rows, n_ch), dtype=torch.complex64, device=frames.device)
        acc_out = torch.empty(n_ch, dtype=torch.complex64, device=frames.device)
        if stream is None:
            stream = torch.cuda.current_stream(frames.device)
        r = L.gsdr_frame_average_device(frames.data_ptr(), n_frames, n_ch, k, kind_c, count,
                                        acc.data_ptr() if acc is not None else None, acc_out.data_ptr(), out.data_ptr(),
                                        C.c_void_p(stream.cuda_stream))
    else:
        def ok(a, n):
            return isinstance(a, np.ndarray) and a.dtype == np.complex64 and a.flags.c_contiguous and a.size == n
        if not ok(frames, n_frames * n_ch) or (acc is not None and not ok(acc, n_ch)):
            raise TypeError("need contiguous complex64 arrays; acc holds n_ch samples")
        out = np.empty((rows, n_ch), dtype=np.complex64)
        acc_out = np.empty(n_ch, dtype=np.complex64)
        r = L.gsdr_frame_average_host(frames.ctypes.data, n_frames, n_ch, k, kind_c, count,
                                      acc.ctypes.data if acc is not None else None, acc_out.ctypes.data, out.ctypes.data)
    if r != rows:
        raise GsdrError(L.gsdr_last_error(None).decode())
    return out, acc_out, (count + n_frames) % k


# ---- host-side helpers of the path, straight from the library --------------

def make_sinc_window(length: int, fc: float) -> np.ndarray:
    w = np.empty(length, dtype=np.float32)
    _lib.lib().gsdr_make_sinc_window(length, C.c_float(fc), w.ctypes.data_as(C.POINTER(C.c_float)))
    return w


def make_flat_window(length: int, side: int) -> np.ndarray:
    w = np.empty(length, dtype=np.float32)
    _lib.lib().gsdr_make_flat_window(length, side, w.ctypes.data_as(C.POINTER(C.c_float)))
    return w


class buffer_helper:
    """class buffer_helper, headers/USRP_server_memory_management.hpp:77-101"""
    FIELDS = [n for n, _ in _lib.BufferHelperC._fields_]

    def __init__(self, n_tones, buffer_len, average, n_eff_tones):
        self._s = _lib.BufferHelperC()
        _lib.lib().gsdr_buffer_helper_init(C.byref(self._s), n_tones, buffer_len, average, n_eff_tones)

    def update(self):
        _lib.lib().gsdr_buffer_helper_update(C.byref(self._s))

    def __getattr__(self, k):
        if k in buffer_helper.FIELDS:
            return getattr(self._s, k)
        raise AttributeError(k)

    def state(self):
        return {k: getattr(self._s, k) for k in self.FIELDS}


class VNA_decimator_helper:
    """class VNA_decimator_helper, headers/USRP_server_memory_management.hpp:24-40"""
    FIELDS = ["valid_size", "new0", "total_len", "spare_begin"]

    def __init__(self, init_ppt, init_buffer_len):
        self._s = _lib.VnaHelperC()
        _lib.lib().gsdr_vna_helper_init(C.byref(self._s), init_ppt, init_buffer_len)

    def update(self):
        _lib.lib().gsdr_vna_helper_update(C.byref(self._s))

    def __getattr__(self, k):
        if k in VNA_decimator_helper.FIELDS:
            return getattr(self._s, k)
        raise AttributeError(k)

    def state(self):
        return {k: getattr(self._s, k) for k in self.FIELDS}


def pfb_tone_bins(rate, fft_tones, freq) -> np.ndarray:
    f = np.ascontiguousarray(np.asarray(freq, dtype=np.int32))
    bins = np.empty(len(f), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    _lib.lib().gsdr_pfb_tone_bins(rate, fft_tones, f.ctypes.data_as(ip), len(f), bins.ctypes.data_as(ip))
    return bins


def pfb_batching(buffer_len, fft_tones, pf_average) -> int:
    return _lib.lib().gsdr_pfb_batching(buffer_len, fft_tones, pf_average)


def chirp_derive(rate, freq0, chirp_f, swipe_s, chirp_t) -> _lib.ChirpParamC:
    cp = _lib.ChirpParamC()
    _lib.lib().gsdr_chirp_derive(rate, freq0, chirp_f, swipe_s, C.c_float(chirp_t), C.byref(cp))
    return cp


def chirp_derive_tx(rate, freq0, chirp_f, swipe_s, chirp_t) -> _lib.ChirpParamC:
    """The TX generator's own derivation (ref: cpp/USRP_buffer_generator.cpp:107-129)."""
    cp = _lib.ChirpParamC()
    _lib.lib().gsdr_chirp_derive_tx(rate, freq0, chirp_f, swipe_s, C.c_float(chirp_t), C.byref(cp))
    return cp
