"""Welch noise spectra from demodulated rows: the Python face of gsdr_welch_* (include/gsdr.h, "Welch spectra on the
device").

The reference's client computes its noise spectra on the host, per channel, in a pool of Python processes
(pyUSRP/USRP_noise.py, ``spec_from_samples``: rotate each channel by the phase of its mean or divide by the mean,
``scipy.signal.welch(detrend='linear', scaling='density')`` on the real and on the imaginary part) -- after every
timestream has crossed PCIe and TCP.  ``device_welch`` keeps running spectra behind the rows an RX entry has just left
in device memory, so that only ``n_ch x 2 x (nperseg/2 + 1)`` floats reach the host, when the caller asks for them.
``host_welch`` is the same estimator over the library's host twin (GSDR_WELCH_HOST): numpy in, float64 out, no GPU.
"""
from __future__ import annotations

import numpy as np

from ._lib import WELCH_HOST
from ._stage import DeviceStage, Stage
from .demodulator import GsdrError  # noqa: F401  (raised by Stage; kept importable from here)

DETREND = {"none": 0, "constant": 1, "linear": 2, None: 0, False: 0}      # GSDR_WELCH_DETREND_*
MODES = {"raw": 0, "rotate": 1, "dbc": 2, "gain": 3}                      # GSDR_WELCH_*


class _welch(Stage):
    """What device_welch and host_welch share: the object and its bookkeeping."""

    _NAME = "welch"

    def __init__(self, n_ch, max_rows, nperseg, step, detrend, window, device_index):
        self.n_ch, self.max_rows, self.nperseg = int(n_ch), int(max_rows), int(nperseg)
        self.step = self.nperseg // 2 if step is None else int(step)
        if detrend not in DETREND:
            raise ValueError(f"detrend must be one of 'linear', 'constant', 'none' (got {detrend!r})")
        win = None
        if window is not None:
            win = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
            if win.shape[0] != self.nperseg:
                raise ValueError(f"window: {win.shape[0]} taps for nperseg {self.nperseg}")
        self._create(self.n_ch, self.max_rows, self.nperseg, self.step, DETREND[detrend],
                     win.ctypes.data if win is not None else None, int(device_index))

    @property
    def bins(self) -> int:
        return self.nperseg // 2 + 1

    def freqs(self, fs: float = 1.0) -> np.ndarray:
        """The bin frequencies, as numpy.fft.rfftfreq(nperseg, 1 / fs)."""
        return np.arange(self.bins, dtype=np.float64) * (float(fs) / self.nperseg)

    def _mode(self, mode, gain):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
        if (mode == "gain") != (gain is not None):
            raise ValueError("gain goes with mode='gain', and only with it")
        return MODES[mode]

    @property
    def rows_seen(self) -> int:
        return int(self._L.gsdr_welch_rows(self._h))

    @property
    def segments(self) -> int:
        return int(self._L.gsdr_welch_segments(self._h))

    def reset(self):
        """Zeroes the accumulators and restarts the row numbering.  Order it behind the feeds in flight."""
        if self._L.gsdr_welch_reset(self._h) != 0:
            self._fail()


class host_welch(_welch):
    """The estimator over the library's host twin (GSDR_WELCH_HOST): numpy complex64 rows in, float64 spectra out."""

    def __init__(self, n_ch, max_rows, nperseg, step=None, detrend="linear", window=None):
        super().__init__(n_ch, max_rows, nperseg, step, detrend, window, WELCH_HOST)

    def feed(self, rows, stream=None):
        """rows: complex64 [n][n_ch]."""
        x = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, self.n_ch)
        if self._L.gsdr_welch_feed_host(self._h, x.ctypes.data if x.shape[0] else None, x.shape[0]) != 0:
            self._fail()

    def _read(self, mode, fs, gain):
        m = self._mode(mode, gain)
        g = None if gain is None else np.ascontiguousarray(gain, dtype=np.complex64).reshape(self.n_ch)
        psd = np.zeros((self.n_ch, 2, self.bins), dtype=np.float64)
        mean = np.zeros((self.n_ch, 2), dtype=np.float64)
        n = self._L.gsdr_welch_read_host(self._h, m, g.ctypes.data if g is not None else None, float(fs), psd.ctypes.data,
                                         mean.ctypes.data)
        if n < 0:
            self._fail()
        return psd, mean[:, 0] + 1j * mean[:, 1], n

    def read(self, mode="rotate", fs=1.0, gain=None, stream=None):
        """(freqs, psd[n_ch, 2, nperseg//2+1] float64, n_segments); psd is all zero before the first segment."""
        psd, _, n = self._read(mode, fs, gain)
        return self.freqs(fs), psd, n

    def mean(self):
        """The mean of the rows [0, n_segments * step) per channel, complex128 (zeros before the first segment)."""
        return self._read("raw", 1.0, None)[1]


class device_welch(DeviceStage, _welch):
    """The accumulator on the GPU, behind rows that are already in device memory (what gsdr_demod_process_device /
    _submit_device wrote).  ``feed`` and ``feed_device`` are the same asynchronous call; ``read`` waits for the stream and
    returns host arrays, ``read_device`` leaves the spectra on the device."""

    def __init__(self, n_ch, max_rows, nperseg, step=None, detrend="linear", window=None, device_index: int = 0):
        super().__init__(n_ch, max_rows, nperseg, step, detrend, window, self._device_index(device_index, "host_welch"))

    def feed_device(self, rows, stream=None):
        """rows: contiguous CUDA complex64 [n][n_ch], n <= max_rows.  Asynchronous on the stream; nothing is read back."""
        n_rows = self._rows(rows)
        if self._L.gsdr_welch_feed_device(self._h, rows.data_ptr() if n_rows else None, n_rows, self._stream(stream)) != 0:
            self._fail()

    feed = feed_device

    def read_device(self, psd_t, mode="rotate", fs=1.0, gain_t=None, stream=None) -> int:
        """Asynchronous: psd_t is a contiguous CUDA float32 tensor of n_ch x 2 x (nperseg//2+1), gain_t (mode 'gain') a
        CUDA complex64 tensor of n_ch.  Returns the number of segments; 0: nothing was written."""
        m = self._mode(mode, gain_t)
        need = self.n_ch * 2 * self.bins
        if not (psd_t.is_cuda and psd_t.is_contiguous() and psd_t.element_size() == 4 and psd_t.numel() >= need):
            raise ValueError(f"psd_t must be a contiguous CUDA float32 tensor of at least {need} elements")
        if gain_t is not None and not (gain_t.is_cuda and gain_t.is_contiguous() and gain_t.element_size() == 8 and gain_t.numel() >= self.n_ch):
            raise ValueError(f"gain_t must be a contiguous CUDA complex64 tensor of at least {self.n_ch} elements")
        n = self._L.gsdr_welch_read_device(self._h, m, gain_t.data_ptr() if gain_t is not None else None, float(fs),
                                           psd_t.data_ptr(), self._stream(stream))
        if n < 0:
            self._fail()
        return n

    def mean_device(self, mean_t, stream=None) -> int:
        """Asynchronous: mean_t (CUDA complex64, n_ch) receives the mean of the rows [0, n_segments * step)."""
        if not (mean_t.is_cuda and mean_t.is_contiguous() and mean_t.element_size() == 8 and mean_t.numel() >= self.n_ch):
            raise ValueError(f"mean_t must be a contiguous CUDA complex64 tensor of at least {self.n_ch} elements")
        n = self._L.gsdr_welch_mean_device(self._h, mean_t.data_ptr(), self._stream(stream))
        if n < 0:
            self._fail()
        return n

    def _read(self, mode, fs, gain, stream):
        m = self._mode(mode, gain)
        g = None if gain is None else np.ascontiguousarray(gain, dtype=np.complex64).reshape(self.n_ch)
        psd = np.zeros((self.n_ch, 2, self.bins), dtype=np.float32)
        mean = np.zeros(self.n_ch, dtype=np.complex64)
        n = self._L.gsdr_welch_read(self._h, m, g.ctypes.data if g is not None else None, float(fs), psd.ctypes.data,
                                    mean.ctypes.data, self._stream(stream))
        if n < 0:
            self._fail()
        return psd, mean, n

    def read(self, mode="rotate", fs=1.0, gain=None, stream=None):
        """Waits for the stream.  (freqs, psd[n_ch, 2, nperseg//2+1] float32, n_segments); ``gain`` is a host array."""
        psd, _, n = self._read(mode, fs, gain, stream)
        return self.freqs(fs), psd, n

    def mean(self, stream=None):
        """Waits for the stream.  The mean of the rows [0, n_segments * step) per channel, complex64."""
        return self._read("raw", 1.0, None, stream)[1]
