"""Per-channel statistics of demodulated rows: the Python face of gsdr_stats_* (include/gsdr.h, "row statistics on the
device").

The reference's trigger in use takes, per packet and channel, the median and the standard deviation of the frequency
timestream on the host (``amplitude_trigger``, pyUSRP/USRP_triggers.py) -- after every row has crossed PCIe and TCP.
``device_stats`` keeps, behind the rows an RX entry or a ``device_resmap`` has just left in device memory, double sums,
the extremes and a histogram of the trigger's own projection per channel; a read returns 64 bytes per channel, and
``levels()`` the table ``device_trigger.set_levels`` takes.  ``host_stats`` is the library's host twin
(GSDR_STATS_HOST): numpy rows in, the device's bits out, no GPU.

The two-pass use: a coarse range first, then ``reset(axes_around(levels(8.0)))`` for bins of sigma / 16.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import STATS_CENTRE_MEAN, STATS_CENTRE_MEDIAN, STATS_HOST, STATS_MAX_QUANTILES
from ._stage import DeviceStage, Stage
from .trigger import LEVEL_DTYPE, as_levels

#: numpy layout of struct gsdr_stats_summary (64 bytes)
SUMMARY_DTYPE = np.dtype([("n", "<u8"), ("bad", "<u8"), ("under", "<u8"), ("over", "<u8"), ("mean", "<f8"), ("var", "<f8"),
                          ("min", "<f4"), ("max", "<f4"), ("reserved", "u1", (8,))])

_CENTRES = {"mean": STATS_CENTRE_MEAN, "median": STATS_CENTRE_MEDIAN}


class _stats(Stage):
    """What device_stats and host_stats share: the object, its bookkeeping and the entries that take either kind."""

    _NAME = "stats"

    def __init__(self, n_ch, max_rows, n_bins, axes, lanes, device_index):
        self.n_ch, self.max_rows, self.n_bins = int(n_ch), int(max_rows), int(n_bins)
        ax = as_levels(axes, self.n_ch) if self.n_ch >= 1 and axes is not None else None
        self._create(self.n_ch, self.max_rows, self.n_bins, int(lanes), ax.ctypes.data if ax is not None else None, int(device_index))
        self.axes = ax.copy()

    def _stream(self, stream):
        return None

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_stats_rows(self._h))

    @property
    def lanes(self) -> int:
        """Chains per channel: what the sums' bits depend on, and nothing else about the launch."""
        return int(self._L.gsdr_stats_lanes(self._h))

    def counts(self, stream=None) -> np.ndarray:
        """uint64 [n_ch][n_bins + 3]: under, the bins, over, bad."""
        out = np.zeros((self.n_ch, self.n_bins + 3), dtype=np.uint64)
        if self._L.gsdr_stats_counts(self._h, out.ctypes.data, self._stream(stream)) != 0:
            self._fail()
        return out

    def quantiles(self, pr, stream=None) -> np.ndarray:
        """float64 [n_ch][len(pr)], every pr in (0, 1]: within one bin of the order statistic of rank ceil(pr n)."""
        p = np.ascontiguousarray(np.atleast_1d(pr), dtype=np.float64)
        out = np.zeros((self.n_ch, max(p.shape[0], 1)), dtype=np.float64)
        if self._L.gsdr_stats_quantiles(self._h, p.ctypes.data_as(C.POINTER(C.c_double)), int(p.shape[0]), out.ctypes.data,
                                        self._stream(stream)) != 0:
            self._fail()
        return out

    def levels(self, nsigma, centre="median", on=None, stream=None) -> np.ndarray:
        """A LEVEL_DTYPE table for ``set_levels`` of a trigger: centre -/+ nsigma sigma of q, the projection copied from the
        axes.  ``on``: None, or n_ch flags (0 switches a channel off)."""
        out = np.zeros(self.n_ch, dtype=LEVEL_DTYPE)
        flags = None
        if on is not None:
            flags = np.ascontiguousarray(np.asarray(on) != 0, dtype=np.uint8).reshape(-1)
            if flags.shape[0] != self.n_ch:
                raise ValueError(f"on: {flags.shape[0]} flags for {self.n_ch} channels")
        code = _CENTRES[centre] if centre in _CENTRES else int(centre)
        if self._L.gsdr_stats_levels(self._h, code, float(nsigma), flags.ctypes.data if flags is not None else None, out.ctypes.data,
                                     self._stream(stream)) != 0:
            self._fail()
        return out

    def reset(self, axes=None):
        """Empties the sums and the counters and restarts the row numbering; with ``axes`` the object takes new ranges
        (and projections).  Order it behind the feeds and reads in flight."""
        ax = as_levels(axes, self.n_ch) if axes is not None else None
        if self._L.gsdr_stats_reset(self._h, ax.ctypes.data if ax is not None else None) != 0:
            self._fail()
        if ax is not None:
            self.axes = ax.copy()


class host_stats(_stats):
    """The library's host twin (GSDR_STATS_HOST): numpy complex64 rows in, the device's bits out."""

    def __init__(self, n_ch, max_rows, n_bins, axes, lanes=0):
        super().__init__(n_ch, max_rows, n_bins, axes, lanes, STATS_HOST)

    def feed(self, rows):
        """rows: complex64 [n][n_ch]."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        if self._L.gsdr_stats_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0]) != 0:
            self._fail()

    def read(self) -> np.ndarray:
        """SUMMARY_DTYPE [n_ch]."""
        out = np.zeros(self.n_ch, dtype=SUMMARY_DTYPE)
        if self._L.gsdr_stats_read_host(self._h, out.ctypes.data) != 0:
            self._fail()
        return out


class device_stats(DeviceStage, _stats):
    """The statistics on the GPU, behind rows that are already in device memory.  ``feed_device`` is one asynchronous
    launch; ``read_device`` leaves the summaries on the device; ``read``, ``counts``, ``quantiles`` and ``levels`` wait
    for the stream and return host arrays."""

    def __init__(self, n_ch, max_rows, n_bins, axes, lanes=0, device_index: int = 0):
        super().__init__(n_ch, max_rows, n_bins, axes, lanes, self._device_index(device_index, "host_stats"))

    def feed_device(self, rows, stream=None):
        """rows: contiguous CUDA complex64 [n][n_ch].  Asynchronous on the stream; nothing is read back."""
        n_rows = self._rows(rows)
        if self._L.gsdr_stats_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows, self._stream(stream)) != 0:
            self._fail()

    feed = feed_device

    def read_device(self, summary, stream=None):
        """summary: a contiguous CUDA tensor of at least n_ch x 64 bytes (8-byte aligned).  Asynchronous."""
        if not (summary.is_cuda and summary.is_contiguous()) or summary.numel() * summary.element_size() < self.n_ch * SUMMARY_DTYPE.itemsize:
            raise ValueError(f"summary must be a contiguous CUDA tensor of at least {self.n_ch * SUMMARY_DTYPE.itemsize} bytes")
        if self._L.gsdr_stats_read_device(self._h, summary.data_ptr(), self._stream(stream)) != 0:
            self._fail()

    def read(self, stream=None) -> np.ndarray:
        """Waits for the stream.  SUMMARY_DTYPE [n_ch]."""
        out = np.zeros(self.n_ch, dtype=SUMMARY_DTYPE)
        if self._L.gsdr_stats_read(self._h, out.ctypes.data, self._stream(stream)) != 0:
            self._fail()
        return out


def feed_plan(n_ch, n_bins, lanes) -> dict:
    """The launch of one feed (gsdr_stats_plan; no GPU needed): ``tile`` channels by 256 / tile chains per workgroup, a
    grid of ``tiles`` x ``splits``, ``lds_bytes`` = tile (n_bins + 3) 4 of counters.  ``lanes``: what the object reports.
    No result depends on any of them.  ValueError for what gsdr_stats_create refuses of the three."""
    out = (C.c_int * 4)()
    if _lib.lib().gsdr_stats_plan(int(n_ch), int(n_bins), int(lanes), out) != 0:
        raise ValueError(f"gsdr_stats_plan refuses n_ch {n_ch}, n_bins {n_bins}, lanes {lanes}")
    return dict(zip(("tile", "tiles", "splits", "lds_bytes"), (int(v) for v in out)))


def axes_around(levels) -> np.ndarray:
    """The axes of a second pass from the levels of a first: the same projection, [lo, hi] as the histogram range.
    Channels that are switched off (an infinite level) cannot serve as a range: ValueError."""
    lv = np.array(levels, dtype=LEVEL_DTYPE, copy=True).reshape(-1)
    if not (np.isfinite(lv["lo"]).all() and np.isfinite(lv["hi"]).all() and (lv["lo"] < lv["hi"]).all()):
        raise ValueError("levels with lo < hi, both finite, are needed as a histogram range")
    return lv


__all__ = ["device_stats", "host_stats", "axes_around", "feed_plan", "SUMMARY_DTYPE", "STATS_MAX_QUANTILES"]
