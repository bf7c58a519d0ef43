"""ctypes binding over oracle/_ref/libgsdr_ref.so: the reference's own RX path, compiled for
the host by oracle/build_ref.py -- TEST INFRASTRUCTURE ONLY, like the rest of oracle/.

Mirrors oracle/__init__.py: Direct / Pfb / Noise / Chirp / Nodsp take the same arguments as
the oracle's classes and return the same shapes, but every number comes from the reference's
RX_buffer_demodulator, its kernels (run serially) and its FIR class; only cuBLAS and cuFFT are
stand-ins (double-accumulating, oracle/ref/include/).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libgsdr_ref.so")
SKIP_REASON = "oracle/_ref not built"

TONES, CHIRP, NOISE, NODSP, DIRECT = 0, 1, 2, 4, 6   # the reference's w_type values
BUFFER_HELPER_FIELDS = ["n_tones", "eff_length", "buffer_len", "average", "n_eff_tones",
                        "new_0", "copy_size", "current_batch", "spare_samples", "spare_begin"]
VNA_HELPER_FIELDS = ["valid_size", "new0", "total_len", "spare_begin"]

_lib = None


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(LIB_PATH)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.ref_demod_create.argtypes = [C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_long, ip, C.c_int,
                                   C.c_float, C.c_int, C.c_int]
    L.ref_demod_create.restype = vp
    L.ref_demod_process.argtypes = [vp, vp, vp]
    L.ref_demod_process.restype = C.c_int
    L.ref_demod_out_capacity.argtypes = [vp]
    L.ref_demod_out_capacity.restype = C.c_long
    L.ref_demod_close.argtypes = [vp]
    L.ref_demod_chirp_params.argtypes = [vp, C.POINTER(C.c_ulong), C.POINTER(C.c_ulong), C.POINTER(C.c_uint), ip]
    L.ref_make_sinc_window.argtypes = [C.c_int, C.c_float, fp]
    L.ref_make_flat_window.argtypes = [C.c_int, C.c_int, fp]
    L.ref_buffer_helper_seq.argtypes = [C.c_int] * 5 + [ip]
    L.ref_vna_helper_seq.argtypes = [C.c_int] * 3 + [ip]
    L.ref_chirp_gen.argtypes = [C.c_ulong, C.c_ulong, C.c_uint, C.c_int, C.c_ulong, C.c_uint, C.c_float, vp]
    L.ref_tone_gen.argtypes = [ip, fp, C.c_int, C.c_int, C.c_float, vp]
    L.ref_tone_gen.restype = C.c_int
    _lib = L
    return L


def _iarr(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def make_sinc_window(length: int, fc: float) -> np.ndarray:
    w = np.empty(length, dtype=np.float32)
    lib().ref_make_sinc_window(length, C.c_float(fc), w.ctypes.data_as(C.POINTER(C.c_float)))
    return w


def make_flat_window(length: int, side: int) -> np.ndarray:
    w = np.empty(length, dtype=np.float32)
    lib().ref_make_flat_window(length, side, w.ctypes.data_as(C.POINTER(C.c_float)))
    return w


def buffer_helper_seq(n_tones, buffer_len, average, n_eff_tones, steps) -> list:
    """buffer_helper's fields after construction and after each update, one dict per step."""
    o = np.zeros((steps, 10), dtype=np.int32)
    lib().ref_buffer_helper_seq(n_tones, buffer_len, average, n_eff_tones, steps, o.ctypes.data_as(C.POINTER(C.c_int)))
    return [dict(zip(BUFFER_HELPER_FIELDS, map(int, r))) for r in o]


def vna_helper_seq(ppt, buffer_len, steps) -> list:
    o = np.zeros((steps, 4), dtype=np.int32)
    lib().ref_vna_helper_seq(ppt, buffer_len, steps, o.ctypes.data_as(C.POINTER(C.c_int)))
    return [dict(zip(VNA_HELPER_FIELDS, map(int, r))) for r in o]


def chirp_gen(num_steps, length, chirpness, f0, last_index, n, scale=1.0) -> np.ndarray:
    out = np.empty(n, dtype=np.complex64)
    lib().ref_chirp_gen(num_steps, length, chirpness, f0, last_index, n, C.c_float(scale), out.ctypes.data_as(C.c_void_p))
    return out


def tone_gen(freq, ampl, rate, scale=1.0) -> np.ndarray:
    """One period (rate samples) of the reference's TX tone comb."""
    f, fptr = _iarr(freq)
    a = np.ascontiguousarray(np.asarray(ampl, dtype=np.float32))
    out = np.empty(rate, dtype=np.complex64)
    rc = lib().ref_tone_gen(fptr, a.ctypes.data_as(C.POINTER(C.c_float)), len(f), rate, C.c_float(scale),
                            out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError("a tone's bin falls outside the vector (0 Hz or |f| >= rate)")
    return out


class _Demod:
    """RX_buffer_demodulator of the reference; process() returns [rows, channels]."""

    def __init__(self, wave_type, channels, rate=1, buffer_len=1, decim=0, fft_tones=0, pf_average=0, freq=(0,),
                 chirp_t=0.0, chirp_f=0, swipe_s=0):
        self.L, self.channels = int(buffer_len), int(channels)
        f, fptr = _iarr(freq)
        self._f = f
        self._h = lib().ref_demod_create(wave_type, int(rate), self.L, int(decim), int(fft_tones), int(pf_average),
                                         fptr, len(f), C.c_float(chirp_t), int(chirp_f), int(swipe_s))
        if not self._h:
            raise ValueError("the reference refuses these parameters")
        self._out = np.zeros(lib().ref_demod_out_capacity(self._h), dtype=np.complex64)

    def process(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.complex64)
        assert len(x) == self.L
        n = lib().ref_demod_process(self._h, x.ctypes.data_as(C.c_void_p), self._out.ctypes.data_as(C.c_void_p))
        assert 0 <= n <= len(self._out) and n % self.channels == 0, n
        return self._out[:n].reshape(-1, self.channels).copy()

    def chirp_params(self):
        ns, ln, ch, f0 = C.c_ulong(), C.c_ulong(), C.c_uint(), C.c_int()
        lib().ref_demod_chirp_params(self._h, C.byref(ns), C.byref(ln), C.byref(ch), C.byref(f0))
        return {"num_steps": ns.value, "length": ln.value, "chirpness": ch.value, "f0": f0.value}

    def close(self):
        if getattr(self, "_h", None):
            lib().ref_demod_close(self._h)
            self._h = None

    __del__ = close


class Direct(_Demod):
    def __init__(self, freq, rate, decim, pf_average, buffer_len):
        super().__init__(DIRECT, len(freq), rate, buffer_len, decim, 0, pf_average, freq)


class Pfb(_Demod):
    def __init__(self, freq, rate, fft_tones, pf_average, buffer_len):
        super().__init__(TONES, len(freq), rate, buffer_len, 0, fft_tones, pf_average, freq)


class Noise(_Demod):
    def __init__(self, fft_tones, pf_average, buffer_len, rate=1_000_000):
        super().__init__(NOISE, fft_tones, rate, buffer_len, 0, fft_tones, pf_average, (0,))


class Chirp(_Demod):
    def __init__(self, rate, freq0, chirp_f, swipe_s, chirp_t, decim, buffer_len):
        super().__init__(CHIRP, 1, rate, buffer_len, decim, 0, 0, (freq0,), chirp_t, chirp_f, swipe_s)


class Nodsp(_Demod):
    def __init__(self, buffer_len, rate=1_000_000):
        super().__init__(NODSP, 1, rate, buffer_len)
