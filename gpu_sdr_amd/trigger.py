"""Trigger on demodulated rows: the Python face of gsdr_trigger_* (include/gsdr.h, "trigger on the device").

The reference's triggers run in its Python 2 client on every packet that crossed the network
(pyUSRP/USRP_triggers.py; ``amplitude_trigger`` is the one in use).  ``device_trigger`` puts that trigger behind the
rows an RX entry has just left in device memory -- a threshold on a per-channel projection, hits closer than ``holdoff``
rows one glitch, a window of ``pre + post`` rows of ALL channels around each glitch -- so that only events and their
snippets reach the host.  ``host_trigger`` is the same object over the library's host twin (GSDR_TRIGGER_HOST): numpy in,
numpy out, no GPU.  Both give the same bits.

Both also have the surface the reference's client expects of a trigger object (trigger_template,
pyUSRP/USRP_triggers.py:14-63): ``trigger_control = "AUTO"`` and ``trigger(data, metadata)``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import TRIGGER_HOST
from ._stage import DeviceStage, Stage
from .demodulator import GsdrError  # noqa: F401  (raised by Stage; kept importable from here)

#: numpy layouts of struct gsdr_trigger_level and struct gsdr_trigger_event (24 bytes each)
LEVEL_DTYPE = np.dtype([("bx", "<f4"), ("by", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("lo", "<f4"), ("hi", "<f4")])
EVENT_DTYPE = np.dtype([("row", "<i8"), ("channel", "<i4"), ("side", "<i4"), ("q", "<f4"), ("n_hit", "<i4")])


def as_levels(levels, n_ch: int) -> np.ndarray:
    """``levels`` as a contiguous LEVEL_DTYPE array of n_ch entries: a structured array, or anything of shape (n_ch, 6)
    in the order bx, by, dx, dy, lo, hi."""
    a = np.asarray(levels)
    if a.dtype != LEVEL_DTYPE:
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 6).view(LEVEL_DTYPE).reshape(-1)
    a = np.ascontiguousarray(a).reshape(-1)
    if a.shape[0] != n_ch:
        raise ValueError(f"levels: {a.shape[0]} entries for {n_ch} channels")
    return a


def levels_from_rows(rows, nsigma: float, direction=(1, 0), channels=None) -> np.ndarray:
    """Levels from a stretch of quiet data, what the reference's amplitude_trigger derives per packet: per channel the
    median and the standard deviation of the projection ``re * direction[0] + im * direction[1]`` (a baseline of 0, so
    that q IS the projection), ``lo / hi = median -/+ nsigma * std``.  Channels not in ``channels`` (None: all) are
    switched off (lo = -inf, hi = +inf).  ``direction`` is one pair for all channels or one per channel.  Plain numpy."""
    x = np.asarray(rows)
    if x.ndim != 2:
        raise ValueError("rows must be [row][channel]")
    n_ch = x.shape[1]
    d = np.broadcast_to(np.asarray(direction, dtype=np.float32).reshape(-1, 2), (n_ch, 2))
    proj = x.real.astype(np.float32) * d[:, 0] + x.imag.astype(np.float32) * d[:, 1]
    med = np.median(proj.astype(np.float64), axis=0)         # the projection in float32, as q is; its statistics in double
    std = np.std(proj.astype(np.float64), axis=0)
    lv = np.zeros(n_ch, dtype=LEVEL_DTYPE)
    lv["dx"], lv["dy"] = d[:, 0], d[:, 1]
    lv["lo"], lv["hi"] = -np.inf, np.inf
    on = np.arange(n_ch) if channels is None else np.asarray(channels, dtype=np.int64)
    lv["lo"][on] = (med - nsigma * std)[on]
    lv["hi"][on] = (med + nsigma * std)[on]
    return lv


class _trigger(Stage):
    """What device_trigger and host_trigger share: the object, its bookkeeping and the reference's trigger surface."""

    _NAME = "trigger"
    trigger_control = "AUTO"

    def __init__(self, n_ch, max_rows, pre, post, holdoff, max_events, levels, device_index):
        self.n_ch, self.max_rows, self.pre, self.post = int(n_ch), int(max_rows), int(pre), int(post)
        self.holdoff, self.max_events = int(holdoff), int(max_events)
        lv = as_levels(levels, self.n_ch) if self.n_ch >= 1 else np.zeros(1, dtype=LEVEL_DTYPE)
        self._create(self.n_ch, self.max_rows, self.pre, self.post, self.holdoff, self.max_events, lv.ctypes.data, int(device_index))
        self.dropped = 0          # triggers counted but not written since creation, by feed() / trigger()

    @property
    def snippet_rows(self) -> int:
        return self.pre + self.post

    def set_levels(self, levels, stream=None):
        """Levels for the rows of later feeds; rows already fed keep their records."""
        lv = as_levels(levels, self.n_ch)
        if self._L.gsdr_trigger_set_levels(self._h, lv.ctypes.data, self._stream(stream)) != 0:
            self._fail()

    def _stream(self, stream):
        return None

    def reset(self):
        """Row numbering restarts at 0; carried rows and records are dropped.  Order it behind the feeds in flight."""
        if self._L.gsdr_trigger_reset(self._h) != 0:
            self._fail()

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_trigger_rows(self._h))

    def _out(self):
        ev = np.zeros(self.max_events, dtype=EVENT_DTYPE)
        sn = np.zeros((self.max_events, self.snippet_rows, self.n_ch), dtype=np.complex64)
        return ev, sn

    def trigger(self, data, metadata):
        """The reference's trigger surface (pyUSRP/USRP_triggers.py:50-63): ``data`` is a packet in the client's order
        ch0_t0, ch1_t0, ... (``metadata['channels']`` channels); returns the snippets of the events the packet
        completes, flat in the same order, and the metadata with 'length' set to their length (0: nothing to write)."""
        if int(metadata.get("channels", self.n_ch)) != self.n_ch:
            raise ValueError(f"packet of {metadata['channels']} channels for a trigger of {self.n_ch}")
        rows = self._packet_rows(data)
        parts = []
        for at in range(0, rows.shape[0], self.max_rows):
            _, sn, _ = self.feed(rows[at:at + self.max_rows])
            if len(sn):
                parts.append(sn.reshape(-1))
        out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex64)
        metadata["length"] = int(out.shape[0])
        return out, metadata


class host_trigger(_trigger):
    """The trigger over the library's host twin (GSDR_TRIGGER_HOST): numpy complex64 rows in, no GPU touched."""

    def __init__(self, n_ch, max_rows, pre, post, holdoff, max_events, levels):
        super().__init__(n_ch, max_rows, pre, post, holdoff, max_events, levels, TRIGGER_HOST)

    def _packet_rows(self, data):
        return np.ascontiguousarray(data, dtype=np.complex64).reshape(-1, self.n_ch)

    def feed(self, rows):
        """rows: complex64 [n][n_ch].  Returns (events, snippets [n_events][pre+post][n_ch], dropped)."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        ev, sn = self._out()
        dropped = C.c_int(0)
        n = self._L.gsdr_trigger_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0], ev.ctypes.data,
                                           sn.ctypes.data, C.byref(dropped))
        if n < 0:
            self._fail()
        self.dropped += dropped.value
        return ev[:n].copy(), sn[:n].copy(), dropped.value


class device_trigger(DeviceStage, _trigger):
    """The trigger on the GPU, behind rows that are already in device memory (what gsdr_demod_process_device /
    _submit_device wrote).  ``feed`` returns host arrays and copies only the emitted events and snippets;
    ``feed_device`` leaves everything on the device and does not synchronise."""

    def __init__(self, n_ch, max_rows, pre, post, holdoff, max_events, levels, device_index: int = 0):
        super().__init__(n_ch, max_rows, pre, post, holdoff, max_events, levels, self._device_index(device_index, "host_trigger"))

    def _packet_rows(self, data):
        import torch
        if isinstance(data, torch.Tensor):
            return data.reshape(-1, self.n_ch)
        return torch.from_numpy(np.ascontiguousarray(data, dtype=np.complex64).reshape(-1, self.n_ch)).cuda()

    def feed(self, rows, stream=None):
        """rows: CUDA complex64 [n][n_ch].  Waits for the stream; returns (events, snippets, dropped) on the host."""
        n_rows = self._rows(rows)
        ev, sn = self._out()
        dropped = C.c_int(0)
        n = self._L.gsdr_trigger_feed(self._h, rows.data_ptr() if n_rows else None, n_rows, ev.ctypes.data, sn.ctypes.data,
                                      C.byref(dropped), self._stream(stream))
        if n < 0:
            self._fail()
        self.dropped += dropped.value
        return ev[:n].copy(), sn[:n].copy(), dropped.value

    def feed_device(self, rows, events_t, snippets_t, counts_t, stream=None):
        """Asynchronous: events_t (uint8 or int32 storage of max_events x 24 bytes), snippets_t (complex64, max_events x
        (pre+post) x n_ch) and counts_t (int32 [2]: n_events, n_dropped) are CUDA tensors the caller owns."""
        n_rows = self._rows(rows)
        for t, need in ((events_t, self.max_events * EVENT_DTYPE.itemsize),
                        (snippets_t, self.max_events * self.snippet_rows * self.n_ch * 8), (counts_t, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < need:
                raise ValueError(f"output tensor too small or not a contiguous CUDA tensor: needs {need} bytes")
        if self._L.gsdr_trigger_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows, events_t.data_ptr(),
                                            snippets_t.data_ptr(), counts_t.data_ptr(), self._stream(stream)) != 0:
            self._fail()
