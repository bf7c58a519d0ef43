"""A second decimation stage behind demodulated rows: the Python face of gsdr_decim_* (include/gsdr.h, "FIR decimation
on the device").

The reference's client decimates on the host, per channel (``scipy.signal.decimate(..., ftype='fir')`` in
pyUSRP/USRP_noise.py) -- after every timestream has crossed PCIe and TCP.  ``device_decimator`` filters and decimates
the rows an RX entry has just left in device memory and leaves rows of the same ``[row][channel]`` layout there, for the
host, a ``device_trigger`` or a ``device_welch``.  ``host_decimator`` is the library's host twin (GSDR_DECIM_HOST), the
same bits from numpy rows, no GPU.

With the default taps and the default ``offset = (T - 1) // 2`` the output is what
``scipy.signal.decimate(x, q, ftype='fir', zero_phase=True)`` gives, up to the rows at the end whose window the stream
has not filled yet.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DECIM_HOST
from ._stage import DeviceStage, Stage
from .demodulator import GsdrError  # noqa: F401  (raised by Stage; kept importable from here)


def fir_taps(q: int) -> np.ndarray:
    """The default taps: float32(scipy.signal.firwin(20 q + 1, 1 / q, window='hamming')), 2 <= q <= 4096."""
    q = int(q)
    w = np.zeros(20 * max(q, 0) + 1, dtype=np.float32)
    if _lib.lib().gsdr_decim_default_taps(q, w.ctypes.data_as(C.POINTER(C.c_float))) != w.shape[0]:
        raise ValueError(f"q must be in [2, 4096] (got {q})")
    return w


class _decimator(Stage):
    """What device_decimator and host_decimator share: the object and its bookkeeping."""

    _NAME = "decim"

    def __init__(self, n_ch, max_rows, q, taps, offset, device_index):
        self.n_ch, self.max_rows, self.q = int(n_ch), int(max_rows), int(q)
        t = None
        if taps is not None:
            t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        n_taps = 0 if t is None else int(t.shape[0])
        T = n_taps if t is not None else 20 * self.q + 1
        self.offset = (T - 1) // 2 if offset is None else int(offset)
        self._create(self.n_ch, self.max_rows, self.q, n_taps, t.ctypes.data if t is not None else None, self.offset, int(device_index))
        self.n_taps = int(self._L.gsdr_decim_get_taps(self._h, None, 0))

    @property
    def taps(self) -> np.ndarray:
        w = np.zeros(self.n_taps, dtype=np.float32)
        self._L.gsdr_decim_get_taps(self._h, w.ctypes.data_as(C.POINTER(C.c_float)), self.n_taps)
        return w

    @property
    def out_capacity(self) -> int:
        """The most rows one feed can emit."""
        return int(self._L.gsdr_decim_out_capacity(self._h))

    def next_rows(self, n_rows: int) -> int:
        """The rows a feed of n_rows would emit now."""
        n = self._L.gsdr_decim_next_rows(self._h, int(n_rows))
        if n < 0:
            self._fail()
        return n

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_decim_rows(self._h))

    @property
    def rows_out(self) -> int:
        return int(self._L.gsdr_decim_rows_out(self._h))

    def reset(self):
        """Restarts the row numbering.  Order it behind the feeds in flight."""
        if self._L.gsdr_decim_reset(self._h) != 0:
            self._fail()


class host_decimator(_decimator):
    """The library's host twin (GSDR_DECIM_HOST): numpy complex64 rows in, complex64 rows out, the device's bits."""

    def __init__(self, n_ch, max_rows, q, taps=None, offset=None):
        super().__init__(n_ch, max_rows, q, taps, offset, DECIM_HOST)

    def feed(self, rows, stream=None) -> np.ndarray:
        """rows: complex64 [n][n_ch], n <= max_rows.  Returns the rows this feed completes, [m][n_ch] (m may be 0)."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        out = np.zeros((max(self.out_capacity, 1), self.n_ch), dtype=np.complex64)
        m = self._L.gsdr_decim_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0], out.ctypes.data)
        if m < 0:
            self._fail()
        return out[:m]


class device_decimator(DeviceStage, _decimator):
    """The decimator on the GPU, behind rows that are already in device memory (what gsdr_demod_process_device /
    _submit_device wrote).  ``feed_device`` is asynchronous and leaves its rows on the device; ``feed`` waits for the
    stream and returns a host array."""

    def __init__(self, n_ch, max_rows, q, taps=None, offset=None, device_index: int = 0):
        super().__init__(n_ch, max_rows, q, taps, offset, self._device_index(device_index, "host_decimator"))

    def feed_device(self, rows, out, stream=None) -> int:
        """rows: contiguous CUDA complex64 [n][n_ch], n <= max_rows; out: contiguous CUDA complex64 with room for
        ``next_rows(n)`` rows.  Asynchronous on the stream; nothing is read back.  Returns the rows written to out."""
        import torch
        n_rows = self._rows(rows)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous()):
            raise TypeError("out must be a contiguous CUDA complex64 tensor")
        if 0 <= n_rows <= self.max_rows and out.numel() < self.next_rows(n_rows) * self.n_ch:
            raise ValueError(f"out holds {out.numel()} samples, this feed writes {self.next_rows(n_rows) * self.n_ch}")
        m = self._L.gsdr_decim_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows,
                                           out.data_ptr() if out.numel() else None, self._stream(stream))
        if m < 0:
            self._fail()
        return m

    def feed(self, rows, stream=None) -> np.ndarray:
        """Waits for the stream.  Returns the rows this feed completes as a host array [m][n_ch] (m may be 0)."""
        n_rows = self._rows(rows)
        out = np.zeros((max(self.out_capacity, 1), self.n_ch), dtype=np.complex64)
        m = self._L.gsdr_decim_feed(self._h, rows.data_ptr() if n_rows else None, n_rows, out.ctypes.data, self._stream(stream))
        if m < 0:
            self._fail()
        return out[:m]
