"""Demodulated rows to resonance-frequency shift and quality factor: the Python face of gsdr_resmap_* (include/gsdr.h,
"resonator map on the device").

The reference's client does this on the host, per channel (``calculate_frequency_timestream`` in pyUSRP/USRP_noise.py)
-- after every timestream has crossed PCIe and TCP.  ``device_resmap`` maps the rows an RX entry has just left in device
memory and leaves rows of the same ``[row][channel]`` layout there, for a ``device_welch`` (a frequency-noise spectrum in
Hz^2/Hz), a ``device_trigger`` (a trigger on the frequency shift) or a ``device_decimator``.  ``host_resmap`` is the
library's host twin (GSDR_RESMAP_HOST), the same bits from numpy rows, no GPU.

Kinds: ``"cal"`` the calibrated S21, ``"x_dqr"`` (frequency shift in Hz, 1/Qr), ``"x_qr"`` (frequency shift in Hz, Qr).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RESMAP_HOST
from ._stage import DeviceStage, Stage
from .demodulator import GsdrError

KINDS = {"cal": 0, "x_dqr": 1, "x_qr": 2}      # GSDR_RESMAP_CAL, GSDR_RESMAP_X_DQR, GSDR_RESMAP_X_QR
NCONST = _lib.RESMAP_NCONST


def resmap_constants(fits, tones) -> np.ndarray:
    """The per-column constants, float64 [n][7] = (nr, ni, gr, gi, kr, ki, hf0), of gsdr_resmap_constants.

    fits: one tuple per column as the reference's fit returns it, ``(f0 [MHz], A, phi, D, Qi, Qr, Qe_re, Qe_im, a)``
    (entries behind the ninth are ignored; Qi, Qr and a are not used: the map is the linear one).  tones: the tone of
    each column in Hz."""
    L = _lib.lib()
    fits = [tuple(f) for f in fits]
    tones = np.asarray(tones, dtype=np.float64).reshape(-1)
    if len(fits) != tones.shape[0]:
        raise ValueError(f"{len(fits)} fits for {tones.shape[0]} tones")
    out = np.zeros((len(fits), NCONST), dtype=np.float64)
    for k, (fit, tone) in enumerate(zip(fits, tones)):
        if len(fit) < 9:
            raise ValueError("a fit is (f0, A, phi, D, Qi, Qr, Qe_re, Qe_im, a)")
        f0, A, phi, D, _, _, qe_re, qe_im = (float(v) for v in fit[:8])
        if L.gsdr_resmap_constants(float(tone), f0, A, phi, D, qe_re, qe_im, out[k].ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise GsdrError(L.gsdr_last_error(None).decode())
    return out


class _resmap(Stage):
    """What device_resmap and host_resmap share: the object, its tables and its offsets."""

    _NAME = "resmap"

    def __init__(self, n_ch, max_rows, constants, channels, kind, device_index):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        self.n_ch, self.max_rows, self.kind = int(n_ch), int(max_rows), kind
        k = np.ascontiguousarray(constants, dtype=np.float64)
        if k.ndim != 2 or k.shape[1] != NCONST:
            raise ValueError(f"constants must be [n_out][{NCONST}] (resmap_constants)")
        ch = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
        if ch is not None and ch.shape[0] != k.shape[0]:
            raise ValueError(f"{k.shape[0]} columns of constants for {ch.shape[0]} channels")
        self._create(self.n_ch, self.max_rows, int(k.shape[0]), ch.ctypes.data if ch is not None else None, k.ctypes.data,
                     KINDS[kind], int(device_index))
        self.n_out = int(self._L.gsdr_resmap_n_out(self._h))

    @property
    def constants(self) -> np.ndarray:
        k = np.zeros((self.n_out, NCONST), dtype=np.float64)
        self._L.gsdr_resmap_get_constants(self._h, k.ctypes.data_as(C.POINTER(C.c_double)), self.n_out)
        return k

    @property
    def channels(self) -> np.ndarray:
        ch = np.zeros(self.n_out, dtype=np.int32)
        self._L.gsdr_resmap_get_channels(self._h, ch.ctypes.data_as(C.POINTER(C.c_int)), self.n_out)
        return ch

    @property
    def offsets(self) -> np.ndarray:
        """What set_offsets was given last, float64 [n_out][2]."""
        xy = np.zeros((self.n_out, 2), dtype=np.float64)
        self._L.gsdr_resmap_get_offsets(self._h, xy.ctypes.data_as(C.POINTER(C.c_double)), self.n_out)
        return xy

    def _set_offsets(self, xy, stream):
        a = None
        if xy is not None:
            a = np.ascontiguousarray(xy, dtype=np.float64)
            if a.size != 2 * self.n_out:
                raise ValueError(f"offsets must be [n_out = {self.n_out}][2]")
        if self._L.gsdr_resmap_set_offsets(self._h, a.ctypes.data if a is not None else None, stream) != 0:
            self._fail()


class host_resmap(_resmap):
    """The library's host twin (GSDR_RESMAP_HOST): numpy complex64 rows in, complex64 rows out, the device's bits."""

    def __init__(self, n_ch, max_rows, constants, channels=None, kind="x_dqr"):
        super().__init__(n_ch, max_rows, constants, channels, kind, RESMAP_HOST)

    def set_offsets(self, xy=None):
        """xy: float64 [n_out][2] = (x0, y0) per column, subtracted in double before the rounding; None: zeros."""
        self._set_offsets(xy, None)

    def feed(self, rows) -> np.ndarray:
        """rows: complex64 [n][n_ch], n <= max_rows.  Returns complex64 [n][n_out]."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        out = np.zeros((x.shape[0], self.n_out), dtype=np.complex64)
        m = self._L.gsdr_resmap_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0],
                                          out.ctypes.data if x.shape[0] else None)
        if m < 0:
            self._fail()
        return out[:m]


class device_resmap(DeviceStage, _resmap):
    """The map on the GPU, behind rows that are already in device memory (what gsdr_demod_process_device /
    _submit_device wrote).  ``feed_device`` is asynchronous and leaves its rows on the device; ``feed`` waits for the
    stream and returns a host array."""

    def __init__(self, n_ch, max_rows, constants, channels=None, kind="x_dqr", device_index: int = 0):
        super().__init__(n_ch, max_rows, constants, channels, kind, self._device_index(device_index, "host_resmap"))

    def set_offsets(self, xy=None, stream=None):
        """xy: float64 [n_out][2] = (x0, y0) per column, or None for zeros; copied before the call returns.  Ordered on
        the stream: feeds enqueued on it afterwards see the new offsets."""
        self._set_offsets(xy, self._stream(stream))

    def feed_device(self, rows, out, stream=None) -> int:
        """rows: contiguous CUDA complex64 [n][n_ch], n <= max_rows; out: contiguous CUDA complex64 with room for
        n x n_out samples (``rows`` itself is allowed where the channel list is the identity).  One launch on the
        stream; nothing is read back.  Returns n."""
        import torch
        n_rows = self._rows(rows)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous()):
            raise TypeError("out must be a contiguous CUDA complex64 tensor")
        if 0 <= n_rows <= self.max_rows and out.numel() < n_rows * self.n_out:
            raise ValueError(f"out holds {out.numel()} samples, this feed writes {n_rows * self.n_out}")
        m = self._L.gsdr_resmap_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows,
                                            out.data_ptr() if n_rows else None, self._stream(stream))
        if m < 0:
            self._fail()
        return m

    def feed(self, rows, stream=None) -> np.ndarray:
        """Waits for the stream.  Returns the mapped rows as a host array [n][n_out]."""
        n_rows = self._rows(rows)
        out = np.zeros((max(n_rows, 1), self.n_out), dtype=np.complex64)
        m = self._L.gsdr_resmap_feed(self._h, rows.data_ptr() if n_rows else None, n_rows, out.ctypes.data, self._stream(stream))
        if m < 0:
            self._fail()
        return out[:m]
