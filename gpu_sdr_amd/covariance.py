"""Covariance across the channels of demodulated rows: the Python face of gsdr_cov_* (include/gsdr.h, "channel covariance
on the device").

Amplifier noise, TLS noise, pickup and temperature drift show up as correlation between the tones of a resonator array;
an off-resonance tone that tracks the on-resonance ones is the standard handle for cleaning them.  ``numpy.cov`` needs
every timestream on the host.  ``device_cov`` keeps, behind the rows an RX entry or a ``device_resmap`` has just left in
device memory, double sums of products of ``n_var`` real projections; a read returns ``n_var x n_var`` doubles -- the
sums, the covariance or the correlation -- and the means.  ``host_cov`` is the library's host twin (GSDR_COV_HOST):
numpy rows in, the device's bits out, no GPU.

Put the pivots near the carriers (a first read's means will do): the sums hold v - pivot.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import COV_CORR, COV_COV, COV_HOST, COV_MAX_LANES, COV_MAX_VARS, COV_SUMS
from ._stage import DeviceStage, Stage

#: numpy layout of struct gsdr_cov_axis (32 bytes)
AXIS_DTYPE = np.dtype([("channel", "<i4"), ("bx", "<f4"), ("by", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("reserved", "<i4"), ("pivot", "<f8")])

_KINDS = {"sums": COV_SUMS, "cov": COV_COV, "corr": COV_CORR}


def as_axes(axes, n_var) -> np.ndarray:
    """axes as a contiguous AXIS_DTYPE array of n_var entries (a copy); ValueError for another length."""
    ax = np.array(axes, dtype=AXIS_DTYPE, copy=True).reshape(-1)
    if ax.shape[0] != n_var:
        raise ValueError(f"axes: {ax.shape[0]} entries for {n_var} variables")
    return np.ascontiguousarray(ax)


def cov_axes(channels, quadrature="re", pivots=None) -> np.ndarray:
    """The axes of the usual variables: per channel of ``channels`` its real part ("re"), its imaginary part ("im"), or
    both ("both": re of every channel first, then im).  ``pivots``: None (0), or one per variable."""
    ch = np.asarray(channels, dtype=np.int32).reshape(-1)
    if quadrature not in ("re", "im", "both"):
        raise ValueError('quadrature must be "re", "im" or "both"')
    parts = {"re": [(1.0, 0.0)], "im": [(0.0, 1.0)], "both": [(1.0, 0.0), (0.0, 1.0)]}[quadrature]
    ax = np.zeros(len(parts) * ch.shape[0], dtype=AXIS_DTYPE)
    for k, (dx, dy) in enumerate(parts):
        part = ax[k * ch.shape[0]:(k + 1) * ch.shape[0]]
        part["channel"], part["dx"], part["dy"] = ch, dx, dy
    if pivots is not None:
        p = np.asarray(pivots, dtype=np.float64).reshape(-1)
        if p.shape[0] != ax.shape[0]:
            raise ValueError(f"pivots: {p.shape[0]} values for {ax.shape[0]} variables")
        ax["pivot"] = p
    return ax


def _kind(kind) -> int:
    return _KINDS[kind] if kind in _KINDS else int(kind)


class _cov(Stage):
    """What device_cov and host_cov share: the object and its bookkeeping."""

    _NAME = "cov"

    def __init__(self, n_ch, axes, max_rows, lanes, device_index):
        self.n_ch, self.max_rows = int(n_ch), int(max_rows)
        ax = np.ascontiguousarray(np.array(axes, dtype=AXIS_DTYPE, copy=True).reshape(-1)) if axes is not None else None
        self.n_var = int(ax.shape[0]) if ax is not None else 0
        self._create(self.n_ch, self.n_var, self.max_rows, int(lanes), ax.ctypes.data if ax is not None and self.n_var else None, int(device_index))
        self.axes = ax

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_cov_rows(self._h))

    rows = rows_seen

    @property
    def lanes(self) -> int:
        """Chains per cell: what the sums' bits depend on, and nothing else about the launch."""
        return int(self._L.gsdr_cov_lanes(self._h))

    def reset(self, axes=None):
        """Zeroes the sums and restarts the row numbering; with ``axes`` the object takes new variables (as many as it
        has).  Order it behind the feeds and reads in flight."""
        ax = as_axes(axes, self.n_var) if axes is not None else None
        if self._L.gsdr_cov_reset(self._h, ax.ctypes.data if ax is not None else None) != 0:
            self._fail()
        if ax is not None:
            self.axes = ax


class host_cov(_cov):
    """The library's host twin (GSDR_COV_HOST): numpy complex64 rows in, the device's bits out."""

    def __init__(self, n_ch, axes, max_rows, lanes=0):
        super().__init__(n_ch, axes, max_rows, lanes, COV_HOST)

    def feed(self, rows):
        """rows: complex64 [n][n_ch]."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        if self._L.gsdr_cov_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0]) != 0:
            self._fail()

    def read(self, kind="cov"):
        """(float64 [n_var][n_var], float64 [n_var]): the matrix of ``kind`` ("sums", "cov", "corr") and the means
        (the sums of d for "sums")."""
        out, mean = np.zeros((self.n_var, self.n_var), dtype=np.float64), np.zeros(self.n_var, dtype=np.float64)
        if self._L.gsdr_cov_read_host(self._h, _kind(kind), out.ctypes.data, mean.ctypes.data) != 0:
            self._fail()
        return out, mean


class device_cov(DeviceStage, _cov):
    """The covariance on the GPU, behind rows that are already in device memory.  ``feed_device`` is two asynchronous
    launches; ``read_device`` leaves the matrix on the device; ``read`` waits for the stream and returns host arrays."""

    def __init__(self, n_ch, axes, max_rows, lanes=0, device_index: int = 0):
        super().__init__(n_ch, axes, max_rows, lanes, self._device_index(device_index, "host_cov"))

    def feed_device(self, rows, stream=None):
        """rows: contiguous CUDA complex64 [n][n_ch].  Asynchronous on the stream; nothing is read back."""
        n_rows = self._rows(rows)
        if self._L.gsdr_cov_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows, self._stream(stream)) != 0:
            self._fail()

    feed = feed_device

    def read_device(self, out, mean=None, kind="cov", stream=None):
        """out: a contiguous CUDA float64 tensor of at least n_var^2 elements; mean: None or one of at least n_var.
        Asynchronous."""
        import torch
        for name, t, need in (("out", out, self.n_var * self.n_var), ("mean", mean, self.n_var)):
            if t is None and name == "mean":
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= need):
                raise ValueError(f"{name} must be a contiguous CUDA float64 tensor of at least {need} elements")
        if self._L.gsdr_cov_read_device(self._h, _kind(kind), out.data_ptr(), mean.data_ptr() if mean is not None else None,
                                        self._stream(stream)) != 0:
            self._fail()

    def read(self, kind="cov", stream=None):
        """Waits for the stream.  (float64 [n_var][n_var], float64 [n_var])."""
        out, mean = np.zeros((self.n_var, self.n_var), dtype=np.float64), np.zeros(self.n_var, dtype=np.float64)
        if self._L.gsdr_cov_read(self._h, _kind(kind), out.ctypes.data, mean.ctypes.data, self._stream(stream)) != 0:
            self._fail()
        return out, mean


def feed_plan(n_ch, n_var, lanes) -> dict:
    """The launches of one feed (gsdr_cov_plan; no GPU needed): ``tile`` variables a side, ``tiles``, ``pairs`` x
    ``lanes`` accumulate workgroups with ``lds_bytes`` of LDS each, ``project_x`` variables per project workgroup.
    ``lanes``: what the object reports.  No result depends on any of them.  ValueError for what gsdr_cov_create refuses
    of the three."""
    out = (C.c_int * 6)()
    if _lib.lib().gsdr_cov_plan(int(n_ch), int(n_var), int(lanes), out) != 0:
        raise ValueError(f"gsdr_cov_plan refuses n_ch {n_ch}, n_var {n_var}, lanes {lanes}")
    return dict(zip(("tile", "tiles", "pairs", "lanes", "lds_bytes", "project_x"), (int(v) for v in out)))


__all__ = ["device_cov", "host_cov", "cov_axes", "feed_plan", "AXIS_DTYPE", "COV_MAX_VARS", "COV_MAX_LANES"]
