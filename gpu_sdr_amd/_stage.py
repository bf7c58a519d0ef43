"""What the Python faces of the seven objects behind demodulated rows share (trigger.py, spectrum.py, decimate.py,
sweep.py, resmap.py, stats.py, covariance.py): the handle with its creation-or-raise and its release, and, for the device classes, the stream,
the check of the rows and the check of device_index."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .demodulator import GsdrError


class Stage:
    """Base of _trigger, _welch, _decimator, _sweep, _resmap, _stats and _cov: the library ``_L`` and the object ``_h`` of
    gsdr_<_NAME>_create, released by gsdr_<_NAME>_close."""

    _NAME = ""
    _h = None

    def _create(self, *args):
        """The object gsdr_<_NAME>_create(*args) makes; GsdrError with the library's words where it refuses."""
        self._L = _lib.lib()
        h = getattr(self._L, f"gsdr_{self._NAME}_create")(*args)
        if not h:
            self._fail()
        self._h = h

    def _fail(self):
        raise GsdrError(self._L.gsdr_last_error(None).decode())

    def close(self):
        if self._h:
            getattr(self._L, f"gsdr_{self._NAME}_close")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceStage:
    """Mixed into the device_* classes, in front of their Stage: what an object on the GPU asks of its arguments."""

    @staticmethod
    def _device_index(device_index, host_class: str) -> int:
        """device_index as an int; the host twin has a class of its own, named in the refusal."""
        if int(device_index) < -1:
            raise ValueError(f"device_index must be >= -1 ({host_class} is the host-only object)")
        return int(device_index)

    def _stream(self, stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def _rows(self, rows) -> int:
        """n_rows of a contiguous CUDA complex64 tensor [n][n_ch]."""
        import torch
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.complex64 and rows.is_contiguous()):
            raise TypeError("rows must be a contiguous CUDA complex64 tensor [n][n_ch]")
        if rows.numel() % self.n_ch:
            raise ValueError("rows is not a whole number of rows")
        return rows.numel() // self.n_ch
