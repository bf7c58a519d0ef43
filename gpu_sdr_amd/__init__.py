"""gpu_sdr_amd -- MI355X-native RX demodulation engine for the GPU_SDR readout.

Only what the hot path needs: csrc/ (HIP kernels + the C ABI of libgsdr.so),
the host-side mirror of the reference's demodulator interface, and the
synthetic IQ source used for benchmarking.
"""
from .demodulator import (GsdrError, RX_buffer_demodulator, RX_wrapper,  # noqa: F401
                          VNA_decimator_helper, buffer_helper, chirp_derive, frame_average,
                          make_flat_window, make_sinc_window, narrow_sc16, param, pfb_batching,
                          pfb_tone_bins, string_to_w_type, w_type, w_type_to_str, widen_sc16)

from .generator import TX_buffer_generator  # noqa: E402,F401
from .trigger import device_trigger, host_trigger, levels_from_rows  # noqa: E402,F401
from .spectrum import device_welch, host_welch  # noqa: E402,F401
from .decimate import device_decimator, fir_taps, host_decimator  # noqa: E402,F401
from .sweep import device_sweep, host_sweep, sweep_shape, vna_axis  # noqa: E402,F401
from .resmap import device_resmap, host_resmap, resmap_constants  # noqa: E402,F401
from .stats import device_stats, host_stats  # noqa: E402,F401
from .covariance import cov_axes, device_cov, host_cov  # noqa: E402,F401

__all__ = [
    "TX_buffer_generator", "device_trigger", "host_trigger", "levels_from_rows", "device_welch", "host_welch",
    "device_decimator", "host_decimator", "fir_taps", "device_sweep", "host_sweep", "sweep_shape", "vna_axis",
    "device_resmap", "host_resmap", "resmap_constants", "device_stats", "host_stats", "device_cov", "host_cov", "cov_axes",
    "GsdrError", "RX_buffer_demodulator", "RX_wrapper", "VNA_decimator_helper",
    "buffer_helper", "chirp_derive", "frame_average", "make_flat_window", "make_sinc_window", "narrow_sc16", "param",
    "pfb_batching", "pfb_tone_bins", "string_to_w_type", "w_type", "w_type_to_str", "widen_sc16",
]
