"""The step every VNA measurement ends with, behind demodulated CHIRP rows: the Python face of gsdr_sweep_*
(include/gsdr.h, "VNA sweep accumulator on the device").

The reference's client reads the whole stream back, splits it into sweeps and takes ``np.mean(..., axis=0)`` per
frequency point (``VNA_analysis`` in pyUSRP/USRP_VNA.py) -- after every row has crossed PCIe and TCP.  ``device_sweep``
folds the rows a CHIRP handle has just left in device memory onto the points of one sweep and keeps double sums there;
only ``n_points x n_ch`` means (and, when asked, as many variances and one complex number per channel for the line
delay) leave the device.  ``host_sweep`` is the library's host twin (GSDR_SWEEP_HOST), the same bits from numpy rows,
no GPU.

``sweep_shape`` gives ``(n_points, group)`` for a chirp's command numbers, ``vna_axis`` the frequency axis of
``VNA_analysis``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SWEEP_HOST
from ._stage import DeviceStage, Stage
from .demodulator import GsdrError, chirp_derive


def sweep_shape(rate, freq0, chirp_f, swipe_s, chirp_t, decim):
    """(n_points, group) of the rows a CHIRP handle with these command numbers writes: one row per point
    (``decim >= 1``: group 1, ``n_points = num_steps length / (length decim)``) or one row per sample (``decim == 0``:
    ``n_points = num_steps``, ``group = length``).  Raises GsdrError where ``length * decim`` does not divide the
    period: the points then do not repeat from sweep to sweep."""
    cp = chirp_derive(int(rate), int(freq0), int(chirp_f), int(swipe_s), float(chirp_t))
    n_points, group = C.c_longlong(0), C.c_longlong(0)
    L = _lib.lib()
    if L.gsdr_sweep_shape_for_chirp(C.byref(cp), int(decim), C.byref(n_points), C.byref(group)) != 0:
        raise GsdrError(L.gsdr_last_error(None).decode())
    return int(n_points.value), int(group.value)


def vna_axis(rate, freq0, chirp_f, swipe_s, n_points, rf=0.0) -> np.ndarray:
    """The frequency axis of ``VNA_analysis``, float64 [n_points]: ``rf + numpy.linspace(freq0, stop, n_points)`` with
    ``stop`` the last frequency the kernel's integer slope reaches, not ``chirp_f``."""
    f = np.zeros(max(int(n_points), 1), dtype=np.float64)
    L = _lib.lib()
    if L.gsdr_vna_axis(float(rate), float(freq0), float(chirp_f), float(swipe_s), int(n_points), float(rf),
                       f.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise GsdrError(L.gsdr_last_error(None).decode())
    return f


class _sweep(Stage):
    """What device_sweep and host_sweep share: the object and its bookkeeping."""

    _NAME = "sweep"

    def __init__(self, n_ch, n_points, group, first_row, device_index):
        self.n_ch, self.n_points, self.group, self.first_row = int(n_ch), int(n_points), int(group), int(first_row)
        self._create(self.n_ch, self.n_points, self.group, int(first_row), int(device_index))

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_sweep_rows(self._h))

    @property
    def sweeps(self) -> int:
        """Complete passes over every point since creation / reset."""
        return int(self._L.gsdr_sweep_sweeps(self._h))

    def point_rows(self, p: int) -> int:
        return int(self._L.gsdr_sweep_point_rows(self._h, int(p)))

    def counts(self) -> np.ndarray:
        """n[p], int64 [n_points]: the rows each point has taken.  A closed form on the host, nothing is read back."""
        W, g = self.n_points * self.group, self.group
        pg = np.arange(self.n_points, dtype=np.int64) * g

        def below(x):
            return (x // W) * g + np.clip(x % W - pg, 0, g)
        return below(self.first_row + self.rows_seen) - below(self.first_row)

    def _slope(self, stream_ptr) -> np.ndarray:
        d = np.zeros(self.n_ch, dtype=np.complex128)
        if self._L.gsdr_sweep_slope(self._h, d.ctypes.data, stream_ptr) != 0:
            self._fail()
        return d

    def slope(self, stream=None) -> np.ndarray:
        """D[c] = sum over p of mean[p+1][c] conj(mean[p][c]), complex128 [n_ch]."""
        return self._slope(None)

    def line_delay(self, f_step, stream=None) -> np.ndarray:
        """tau[c] = -arg D[c] / (2 pi f_step) in seconds, float64 [n_ch], for points f_step Hz apart (negative for a
        downward sweep).  Unambiguous for |tau| < 1 / (2 |f_step|)."""
        return -np.angle(self.slope(stream=stream)) / (2.0 * np.pi * float(f_step))

    def reset(self, first_row: int = 0):
        """Zeroes the sums and restarts the row numbering at first_row.  Order it behind the feeds and reads in flight."""
        if self._L.gsdr_sweep_reset(self._h, int(first_row)) != 0:
            self._fail()
        self.first_row = int(first_row)


class host_sweep(_sweep):
    """The library's host twin (GSDR_SWEEP_HOST): numpy complex64 rows in, the device's bits out."""

    def __init__(self, n_ch, n_points, group=1, first_row=0):
        super().__init__(n_ch, n_points, group, first_row, SWEEP_HOST)

    def feed(self, rows):
        """rows: complex64 [n][n_ch]."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        if self._L.gsdr_sweep_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0]) != 0:
            self._fail()

    def read(self, variance=False):
        """mean, complex64 [n_points][n_ch]; with variance=True (mean, var), var a complex64 that holds the variance of
        the real and of the imaginary part."""
        mean = np.zeros((self.n_points, self.n_ch), dtype=np.complex64)
        var = np.zeros((self.n_points, self.n_ch), dtype=np.complex64) if variance else None
        if self._L.gsdr_sweep_read_host(self._h, mean.ctypes.data, var.ctypes.data if variance else None) != 0:
            self._fail()
        return (mean, var) if variance else mean


class device_sweep(DeviceStage, _sweep):
    """The accumulator on the GPU, behind rows that are already in device memory (what gsdr_demod_process_device /
    _submit_device wrote).  ``feed_device`` is one asynchronous launch; ``read_device`` leaves the means on the device;
    ``read``, ``slope`` and ``line_delay`` wait for the stream and return host arrays."""

    def __init__(self, n_ch, n_points, group=1, first_row=0, device_index: int = 0):
        super().__init__(n_ch, n_points, group, first_row, self._device_index(device_index, "host_sweep"))

    def _out(self, t, name):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.complex64 and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous CUDA complex64 tensor")
        if t.numel() < self.n_points * self.n_ch:
            raise ValueError(f"{name} holds {t.numel()} samples, a read writes {self.n_points * self.n_ch}")
        return t.data_ptr()

    def feed_device(self, rows, stream=None):
        """rows: contiguous CUDA complex64 [n][n_ch].  Asynchronous on the stream; nothing is read back."""
        n_rows = self._rows(rows)
        if self._L.gsdr_sweep_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows, self._stream(stream)) != 0:
            self._fail()

    feed = feed_device

    def read_device(self, mean, var=None, stream=None):
        """mean (and var, unless None): contiguous CUDA complex64 with room for n_points x n_ch.  Asynchronous."""
        m = self._out(mean, "mean")
        v = self._out(var, "var") if var is not None else None
        if self._L.gsdr_sweep_read_device(self._h, m, v, self._stream(stream)) != 0:
            self._fail()

    def read(self, variance=False, stream=None):
        """Waits for the stream.  mean, complex64 [n_points][n_ch], or (mean, var) with variance=True."""
        mean = np.zeros((self.n_points, self.n_ch), dtype=np.complex64)
        var = np.zeros((self.n_points, self.n_ch), dtype=np.complex64) if variance else None
        if self._L.gsdr_sweep_read(self._h, mean.ctypes.data, var.ctypes.data if variance else None, self._stream(stream)) != 0:
            self._fail()
        return (mean, var) if variance else mean

    def slope(self, stream=None) -> np.ndarray:
        """Waits for the stream.  D[c], complex128 [n_ch]."""
        return self._slope(self._stream(stream))
