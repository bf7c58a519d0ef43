"""ctypes binding of libgsdr.so (include/gsdr.h).

The product path has NO CPU fallback: if the HIP library is missing this module
raises at import of the symbols, and every compute call needs a GPU.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSDR_LIB: load a differently built copy (timing-only ablation builds in scratch/)
LIB_PATH = os.environ.get("GSDR_LIB") or os.path.join(_HERE, "libgsdr.so")


class GsdrLibraryError(RuntimeError):
    pass


class ParamC(C.Structure):
    """struct gsdr_param_c (include/gsdr.h)"""
    _fields_ = [
        ("rate", C.c_int),
        ("decim", C.c_longlong),
        ("fft_tones", C.c_int),
        ("pf_average", C.c_longlong),
        ("buffer_len", C.c_longlong),
        ("wave_type", C.POINTER(C.c_int)),
        ("n_wave_type", C.c_int),
        ("freq", C.POINTER(C.c_int)),
        ("n_freq", C.c_int),
        ("chirp_t", C.POINTER(C.c_float)),
        ("n_chirp_t", C.c_int),
        ("chirp_f", C.POINTER(C.c_int)),
        ("n_chirp_f", C.c_int),
        ("swipe_s", C.POINTER(C.c_int)),
        ("n_swipe_s", C.c_int),
        ("device_index", C.c_int),
    ]


class BufferHelperC(C.Structure):
    """struct gsdr_buffer_helper"""
    _fields_ = [(n, C.c_int) for n in (
        "n_tones", "eff_length", "buffer_len", "average", "n_eff_tones",
        "new_0", "copy_size", "current_batch", "spare_samples", "spare_begin")]


class VnaHelperC(C.Structure):
    """struct gsdr_vna_helper"""
    _fields_ = [(n, C.c_int) for n in (
        "valid_size", "new0", "total_len", "spare_begin", "ppt", "buffer_len")]


class AntennaInfoC(C.Structure):
    """struct gsdr_antenna_info"""
    _fields_ = [("mode", C.c_int), ("rf", C.c_double), ("gain", C.c_int), ("bw", C.c_int),
                ("tuning_mode", C.c_int), ("samples", C.c_longlong), ("delay", C.c_double),
                ("burst_on", C.c_float), ("burst_off", C.c_float), ("data_mem_mult", C.c_longlong),
                ("ampl", C.POINTER(C.c_float)), ("n_ampl", C.c_int)]


class RxHeaderC(C.Structure):
    """struct gsdr_rx_header"""
    _fields_ = [("usrp_number", C.c_int), ("front_end_code", C.c_char), ("packet_number", C.c_int),
                ("length", C.c_int), ("errors", C.c_int), ("channels", C.c_int)]


class ChirpParamC(C.Structure):
    """struct gsdr_chirp_param"""
    _fields_ = [("num_steps", C.c_ulonglong), ("length", C.c_ulonglong),
                ("chirpness", C.c_uint), ("f0", C.c_int)]


class PfbPlanInC(C.Structure):
    """struct gsdr_pfb_plan_in"""
    _fields_ = [(n, C.c_int) for n in (
        "nfft", "avg", "blue_m", "frames", "n_out", "cus",
        "pfb_cu", "pfb_direct", "pfb_col", "pfb_cu_nt", "pfb_teams", "pfb_radix8", "pfb_fr", "pfb_wide")]


class PfbPlanOutC(C.Structure):
    """struct gsdr_pfb_plan_out"""
    _fields_ = [(n, C.c_int) for n in (
        "cu", "threads", "G", "twl", "lds", "b_off", "b_len", "col", "direct", "dir_s", "dir_gs", "teams",
        "len", "n_radices")] + [("radices", C.c_int * 16)]


class DdcPlanInC(C.Structure):
    """struct gsdr_ddc_plan_in"""
    _fields_ = [(n, C.c_longlong) for n in ("decim", "pf_average", "buffer_len")] + [(n, C.c_int) for n in (
        "tones", "rate", "rows", "overlapped", "cus",
        "ddc_mfma", "ddc_few", "ddc_pipe", "ddc_k", "ddc_waves", "ddc_nch",
        "mfma_asm", "mfma_tt", "mfma_pk", "mfma_w", "mfma_rt", "mfma_w8", "mfma_prec",
        "mfma_3m", "mfma_3m_rot", "mfma_fold", "mfma_fold_products", "mfma_wave_tones", "mfma_span")]


class DdcPlanOutC(C.Structure):
    """struct gsdr_ddc_plan_out"""
    _fields_ = [(n, C.c_int) for n in (
        "engine", "K", "pad", "R", "target_waves", "tails_nch", "chunks", "chunks_want",
        "complex_mac", "rotation_blocks", "fold", "fold_products", "wave_tones", "span_samples",
        "images", "preconverted", "row_tiles_per_workgroup", "eight_waves",
        "complex_mac_min_blocks", "rotation_min_blocks", "fold_min_blocks", "span128_min_blocks")]


# every symbol include/gsdr.h declares: (name, restype, argtypes)
_vp, _ip, _fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
SIGNATURES = [
    ("gsdr_demod_create", _vp, [C.POINTER(ParamC)]),
    ("gsdr_demod_process", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_demod_process_device", C.c_int, [_vp, _vp, _vp, _vp]),
    ("gsdr_demod_submit", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_demod_submit_device", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_demod_wait", C.c_int, [_vp]),
    ("gsdr_demod_prepare", C.c_int, [_vp, C.c_int]),
    ("gsdr_demod_set_sc16_scale", C.c_int, [_vp, C.c_float]),
    ("gsdr_demod_sc16_scale", C.c_float, [_vp]),
    ("gsdr_demod_process_sc16", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_demod_process_device_sc16", C.c_int, [_vp, _vp, _vp, _vp]),
    ("gsdr_demod_submit_sc16", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_demod_submit_device_sc16", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_widen_sc16_device", C.c_int, [_vp, _vp, C.c_longlong, C.c_float, _vp]),
    ("gsdr_widen_sc16_host", None, [_vp, _vp, C.c_longlong, C.c_float]),
    ("gsdr_narrow_sc16_device", C.c_int, [_vp, _vp, C.c_longlong, C.c_float, _vp, _vp]),
    ("gsdr_narrow_sc16_host", C.c_longlong, [_vp, _vp, C.c_longlong, C.c_float]),
    ("gsdr_demod_set_frame_average", C.c_int, [_vp, C.c_int, C.c_int]),
    ("gsdr_demod_frame_average", C.c_int, [_vp, _ip]),
    ("gsdr_frame_average_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    ("gsdr_frame_average_host", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("gsdr_demod_close", None, [_vp]),
    ("gsdr_last_error", C.c_char_p, [_vp]),
    ("gsdr_abi_version", C.c_int, []),
    ("gsdr_build_info", C.c_char_p, []),
    ("gsdr_reload_env", None, []),
    ("gsdr_demod_describe", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("gsdr_demod_mode", C.c_int, [_vp]),
    ("gsdr_demod_channels", C.c_int, [_vp]),
    ("gsdr_demod_out_capacity", C.c_longlong, [_vp]),
    ("gsdr_demod_fcut", C.c_float, [_vp]),
    ("gsdr_demod_get_window", C.c_int, [_vp, _fp, C.c_int]),
    ("gsdr_demod_get_bins", C.c_int, [_vp, _ip, C.c_int]),
    ("gsdr_demod_profile_enable", None, [_vp, C.c_int]),
    ("gsdr_demod_profile_read", C.c_int, [_vp, C.POINTER(C.c_double)]),
    ("gsdr_demod_kernel_name", C.c_char_p, [_vp]),
    ("gsdr_make_sinc_window", None, [C.c_int, C.c_float, _fp]),
    ("gsdr_make_flat_window", None, [C.c_int, C.c_int, _fp]),
    ("gsdr_buffer_helper_init", None, [C.POINTER(BufferHelperC)] + [C.c_int] * 4),
    ("gsdr_buffer_helper_update", None, [C.POINTER(BufferHelperC)]),
    ("gsdr_vna_helper_init", None, [C.POINTER(VnaHelperC), C.c_int, C.c_int]),
    ("gsdr_vna_helper_update", None, [C.POINTER(VnaHelperC)]),
    ("gsdr_pfb_tone_bins", None, [C.c_int, C.c_int, _ip, C.c_int, _ip]),
    ("gsdr_pfb_batching", C.c_int, [C.c_longlong, C.c_int, C.c_longlong]),
    ("gsdr_pfb_lds_stages", C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    ("gsdr_chirp_lockin_plan", C.c_int, [C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_ulonglong, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("gsdr_pfb_plan", C.c_int, [C.POINTER(PfbPlanInC), C.POINTER(PfbPlanOutC)]),
    ("gsdr_pfb_plan_many", C.c_int, [_vp, C.c_int, _vp]),
    ("gsdr_pfb_blue_length", C.c_int, [C.c_int] * 5),
    ("gsdr_ddc_plan", C.c_int, [C.POINTER(DdcPlanInC), C.POINTER(DdcPlanOutC)]),
    ("gsdr_txgen_tones_create", C.c_void_p, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int]),
    ("gsdr_txgen_tones_fill", C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]),
    ("gsdr_txgen_close", None, [C.c_void_p]),
    ("gsdr_txgen_create", C.c_void_p, [C.POINTER(ParamC), C.POINTER(C.c_float), C.c_int]),
    ("gsdr_txgen_get", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gsdr_txgen_get_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("gsdr_txgen_buffer_len", C.c_longlong, [C.c_void_p]),
    ("gsdr_txgen_get_ptr", C.c_void_p, [C.c_void_p]),
    ("gsdr_txgen_prepare_host", C.c_int, [C.c_void_p]),
    ("gsdr_txgen_mode", C.c_int, [C.c_void_p]),
    ("gsdr_txgen_set_sc16_gain", C.c_int, [C.c_void_p, C.c_float]),
    ("gsdr_txgen_sc16_gain", C.c_float, [C.c_void_p]),
    ("gsdr_txgen_tones_fill_sc16", C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p]),
    ("gsdr_txgen_get_device_sc16", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("gsdr_txgen_get_sc16", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gsdr_txgen_prepare_host_sc16", C.c_int, [C.c_void_p]),
    ("gsdr_txgen_get_ptr_sc16", C.c_void_p, [C.c_void_p]),
    ("gsdr_txgen_sc16_clipped", C.c_longlong, [C.c_void_p]),
    ("gsdr_source_chirp_sc16", C.c_int, [_vp, C.c_longlong, C.c_ulonglong, C.POINTER(ChirpParamC), C.c_float,
                                         C.c_float, _vp, _vp]),
    ("gsdr_chirp_derive", None, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                 C.POINTER(ChirpParamC)]),
    ("gsdr_chirp_derive_tx", None, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.POINTER(ChirpParamC)]),
    ("gsdr_command_parse", _vp, [C.c_char_p, C.c_int]),
    ("gsdr_command_free", None, [_vp]),
    ("gsdr_command_error", C.c_char_p, []),
    ("gsdr_command_device", C.c_int, [_vp]),
    ("gsdr_command_antenna", C.c_int, [_vp, C.c_int, C.POINTER(ParamC), C.POINTER(AntennaInfoC)]),
    ("gsdr_server_reply", C.c_int, [C.c_int, C.c_char_p, C.c_char_p, C.c_int]),
    ("gsdr_format_async_header", None, [C.c_int, C.POINTER(C.c_ubyte)]),
    ("gsdr_format_rx_header", None, [C.POINTER(RxHeaderC), C.POINTER(C.c_ubyte)]),
    ("gsdr_source_tones", C.c_int, [_vp, C.c_longlong, C.c_longlong, C.c_int, _ip, _fp, _fp,
                                    C.c_int, C.c_float, C.c_ulonglong, _vp]),
    ("gsdr_tx_tone_bins", C.c_int, [C.c_int, _ip, _fp, C.c_int, _ip, _fp]),
    ("gsdr_source_chirp", C.c_int, [_vp, C.c_longlong, C.c_ulonglong,
                                    C.POINTER(ChirpParamC), C.c_float, _vp]),
    ("gsdr_demod_create_ex", _vp, [C.POINTER(ParamC), C.c_uint]),
    ("gsdr_txgen_create_ex", C.c_void_p, [C.POINTER(ParamC), C.POINTER(C.c_float), C.c_int, C.c_uint]),
    ("gsdr_source_multichirp", C.c_int, [_vp, C.c_longlong, C.c_ulonglong, C.POINTER(ChirpParamC), _fp, C.c_int, _vp]),
    ("gsdr_source_multichirp_sc16", C.c_int, [_vp, C.c_longlong, C.c_ulonglong, C.POINTER(ChirpParamC), _fp, C.c_int,
                                              C.c_float, _vp, _vp]),
    ("gsdr_trigger_create", _vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    ("gsdr_trigger_set_levels", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_trigger_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    ("gsdr_trigger_feed", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _ip, _vp]),
    ("gsdr_trigger_feed_host", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _ip]),
    ("gsdr_trigger_reset", C.c_int, [_vp]),
    ("gsdr_trigger_rows", C.c_longlong, [_vp]),
    ("gsdr_trigger_close", None, [_vp]),
    ("gsdr_welch_create", _vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    ("gsdr_welch_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_welch_read_device", C.c_int, [_vp, C.c_int, _vp, C.c_double, _vp, _vp]),
    ("gsdr_welch_read", C.c_int, [_vp, C.c_int, _vp, C.c_double, _vp, _vp, _vp]),
    ("gsdr_welch_mean_device", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_welch_feed_host", C.c_int, [_vp, _vp, C.c_int]),
    ("gsdr_welch_read_host", C.c_int, [_vp, C.c_int, _vp, C.c_double, _vp, _vp]),
    ("gsdr_welch_reset", C.c_int, [_vp]),
    ("gsdr_welch_rows", C.c_longlong, [_vp]),
    ("gsdr_welch_segments", C.c_longlong, [_vp]),
    ("gsdr_welch_close", None, [_vp]),
    ("gsdr_decim_create", _vp, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_longlong, C.c_int]),
    ("gsdr_decim_next_rows", C.c_int, [_vp, C.c_int]),
    ("gsdr_decim_out_capacity", C.c_longlong, [_vp]),
    ("gsdr_decim_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    ("gsdr_decim_feed", C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    ("gsdr_decim_feed_host", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_decim_get_taps", C.c_int, [_vp, _fp, C.c_int]),
    ("gsdr_decim_reset", C.c_int, [_vp]),
    ("gsdr_decim_rows", C.c_longlong, [_vp]),
    ("gsdr_decim_rows_out", C.c_longlong, [_vp]),
    ("gsdr_decim_close", None, [_vp]),
    ("gsdr_decim_default_taps", C.c_int, [C.c_int, _fp]),
    ("gsdr_sweep_create", _vp, [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int]),
    ("gsdr_sweep_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_sweep_feed_host", C.c_int, [_vp, _vp, C.c_int]),
    ("gsdr_sweep_read_device", C.c_int, [_vp, _vp, _vp, _vp]),
    ("gsdr_sweep_read", C.c_int, [_vp, _vp, _vp, _vp]),
    ("gsdr_sweep_read_host", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_sweep_slope", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_sweep_reset", C.c_int, [_vp, C.c_longlong]),
    ("gsdr_sweep_rows", C.c_longlong, [_vp]),
    ("gsdr_sweep_sweeps", C.c_longlong, [_vp]),
    ("gsdr_sweep_point_rows", C.c_longlong, [_vp, C.c_longlong]),
    ("gsdr_sweep_close", None, [_vp]),
    ("gsdr_sweep_shape_for_chirp", C.c_int, [C.POINTER(ChirpParamC), C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    ("gsdr_vna_axis", C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_longlong, C.c_double, C.POINTER(C.c_double)]),
    ("gsdr_resmap_constants", C.c_int, [C.c_double] * 7 + [C.POINTER(C.c_double)]),
    ("gsdr_resmap_create", _vp, [C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int]),
    ("gsdr_resmap_set_offsets", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_resmap_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    ("gsdr_resmap_feed", C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    ("gsdr_resmap_feed_host", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_resmap_n_out", C.c_int, [_vp]),
    ("gsdr_resmap_kind", C.c_int, [_vp]),
    ("gsdr_resmap_get_constants", C.c_int, [_vp, C.POINTER(C.c_double), C.c_int]),
    ("gsdr_resmap_get_offsets", C.c_int, [_vp, C.POINTER(C.c_double), C.c_int]),
    ("gsdr_resmap_get_channels", C.c_int, [_vp, C.POINTER(C.c_int), C.c_int]),
    ("gsdr_resmap_close", None, [_vp]),
    ("gsdr_stats_create", _vp, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    ("gsdr_stats_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_stats_feed_host", C.c_int, [_vp, _vp, C.c_int]),
    ("gsdr_stats_read_device", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_stats_read", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_stats_read_host", C.c_int, [_vp, _vp]),
    ("gsdr_stats_counts", C.c_int, [_vp, _vp, _vp]),
    ("gsdr_stats_quantiles", C.c_int, [_vp, C.POINTER(C.c_double), C.c_int, _vp, _vp]),
    ("gsdr_stats_levels", C.c_int, [_vp, C.c_int, C.c_double, _vp, _vp, _vp]),
    ("gsdr_stats_reset", C.c_int, [_vp, _vp]),
    ("gsdr_stats_rows", C.c_longlong, [_vp]),
    ("gsdr_stats_lanes", C.c_int, [_vp]),
    ("gsdr_stats_n_bins", C.c_int, [_vp]),
    ("gsdr_stats_plan", C.c_int, [C.c_int, C.c_int, C.c_int, _ip]),
    ("gsdr_stats_close", None, [_vp]),
    ("gsdr_cov_create", _vp, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    ("gsdr_cov_feed_device", C.c_int, [_vp, _vp, C.c_int, _vp]),
    ("gsdr_cov_feed_host", C.c_int, [_vp, _vp, C.c_int]),
    ("gsdr_cov_read_device", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("gsdr_cov_read", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("gsdr_cov_read_host", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("gsdr_cov_reset", C.c_int, [_vp, _vp]),
    ("gsdr_cov_rows", C.c_longlong, [_vp]),
    ("gsdr_cov_lanes", C.c_int, [_vp]),
    ("gsdr_cov_n_var", C.c_int, [_vp]),
    ("gsdr_cov_plan", C.c_int, [C.c_int, C.c_int, C.c_int, _ip]),
    ("gsdr_cov_close", None, [_vp]),
]

CREATE_MULTI_CHIRP = 1      # GSDR_CREATE_MULTI_CHIRP
MULTI_CHIRP_MAX = 16        # GSDR_MULTI_CHIRP_MAX
TRIGGER_HOST = -2           # GSDR_TRIGGER_HOST
WELCH_HOST = -2             # GSDR_WELCH_HOST
DECIM_HOST = -2             # GSDR_DECIM_HOST
SWEEP_HOST = -2             # GSDR_SWEEP_HOST
SWEEP_MAX_FEED = 1 << 24    # GSDR_SWEEP_MAX_FEED
RESMAP_HOST = -2            # GSDR_RESMAP_HOST
RESMAP_NCONST = 7           # GSDR_RESMAP_NCONST
STATS_HOST = -2             # GSDR_STATS_HOST
STATS_MAX_BINS = 4096       # GSDR_STATS_MAX_BINS
STATS_MAX_LANES = 32768     # GSDR_STATS_MAX_LANES
STATS_MAX_QUANTILES = 16    # GSDR_STATS_MAX_QUANTILES
STATS_CENTRE_MEAN = 0       # GSDR_STATS_CENTRE_MEAN
STATS_CENTRE_MEDIAN = 1     # GSDR_STATS_CENTRE_MEDIAN
COV_HOST = -2               # GSDR_COV_HOST
COV_MAX_VARS = 4096         # GSDR_COV_MAX_VARS
COV_MAX_LANES = 4096        # GSDR_COV_MAX_LANES
COV_SUMS, COV_COV, COV_CORR = 0, 1, 2       # GSDR_COV_SUMS, GSDR_COV_COV, GSDR_COV_CORR


class TriggerLevelC(C.Structure):
    """struct gsdr_trigger_level"""
    _fields_ = [(n, C.c_float) for n in ("bx", "by", "dx", "dy", "lo", "hi")]


class TriggerEventC(C.Structure):
    """struct gsdr_trigger_event"""
    _fields_ = [("row", C.c_longlong), ("channel", C.c_int), ("side", C.c_int), ("q", C.c_float), ("n_hit", C.c_int)]

_lib = None


def lib() -> C.CDLL:
    """Load libgsdr.so (built in-tree by gpu_sdr_amd/csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as
    # the system one libgsdr.so is linked against).  Whichever copy is mapped
    # first serves both, and torch only works with its own: load torch first so
    # that device pointers, streams and this library share ONE runtime.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise GsdrLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C gpu_sdr_amd/csrc`. There is no CPU fallback.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise GsdrLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, restype, argtypes in SIGNATURES:
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            if os.environ.get("GSDR_LIB") and os.environ.get("GSDR_LIB_OLD_ABI"):
                continue      # scratch/ A/B runs against a library of an earlier round (bench.py marks such lines INVALID)
            raise GsdrLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L
