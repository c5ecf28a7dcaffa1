"""gnsscorr -- ctypes binding of libgnsscorr.so (include/gnsscorr.h).

The product is the C-ABI HIP library; this module only marshals numpy arrays
and raw device pointers (e.g. ``torch.Tensor.data_ptr()``) into it for tests
and the benchmark.  There is no CPU fallback: every compute entry point needs
the HIP library and a GPU, and raises ``GnsscorrError`` otherwise.

Class and method names follow the reference
(``Cpu_Multicorrelator_Real_Codes`` -> :class:`HipMulticorrelatorRealCodes`,
``pcps_acquisition`` -> :class:`PcpsAcquisition`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNSSCORR_LIB", os.path.join(os.path.dirname(_HERE), "libgnsscorr.so"))

GC_OK, GC_ERR_INVALID, GC_ERR_NO_DEVICE, GC_ERR_HIP, GC_ERR_STATE = range(5)
GC_MAX_TAPS = 8
GC_IQ_F32, GC_IQ_I16, GC_IQ_I8 = range(3)
# gc_raw_real_format: real raw samples, for Conditioner only (float32 / int16 / int8 one per sample; 2 bits, four samples per byte)
GC_RAW_REAL_F32, GC_RAW_REAL_I16, GC_RAW_REAL_I8, GC_RAW_REAL_2BIT = range(16, 20)
GC_RESAMP_DIRECT, GC_RESAMP_POLYPHASE = range(2)
GC_NOTCH_FULL, GC_NOTCH_LITE = range(2)
GC_NOTCH_FLOOR_REFERENCE, GC_NOTCH_FLOOR_LINEAR = range(2)
GC_SIGGEN_TABLES_AUTO, GC_SIGGEN_TABLES_HBM, GC_SIGGEN_TABLES_LDS = range(3)
GC_SIGGEN_MAX_SATS, GC_SIGGEN_MAX_TABLE, GC_SIGGEN_MAX_SECONDARY = 32, 49104, 100


class GnsscorrError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("gnsscorr status %d: %s" % (status, msg))
        self.status = status


class EpochParams(C.Structure):
    """gc_epoch_params (include/gnsscorr.h)."""
    _fields_ = [
        ("sample_offset", C.c_uint64),
        ("phase0_re", C.c_float), ("phase0_im", C.c_float),
        ("phase_inc_re", C.c_float), ("phase_inc_im", C.c_float),
        ("phase_rate_re", C.c_float), ("phase_rate_im", C.c_float),
        ("rem_code_phase_chips", C.c_float),
        ("code_phase_step_chips", C.c_float),
        ("code_phase_rate_step_chips", C.c_float),
        ("n_samples", C.c_int32),
    ]


EPOCH_DTYPE = np.dtype([
    ("sample_offset", np.uint64),
    ("phase0_re", np.float32), ("phase0_im", np.float32),
    ("phase_inc_re", np.float32), ("phase_inc_im", np.float32),
    ("phase_rate_re", np.float32), ("phase_rate_im", np.float32),
    ("rem_code_phase_chips", np.float32),
    ("code_phase_step_chips", np.float32),
    ("code_phase_rate_step_chips", np.float32),
    ("n_samples", np.int32),
], align=True)
assert EPOCH_DTYPE.itemsize == C.sizeof(EpochParams) == 48


class AcqConf(C.Structure):
    """gc_acq_conf: the Acq_Conf fields pcps_acquisition reads."""
    _fields_ = [
        ("fs_in", C.c_int64),
        ("sampled_ms", C.c_uint32),
        ("ms_per_code", C.c_uint32),
        ("samples_per_ms", C.c_float),
        ("samples_per_code", C.c_float),
        ("samples_per_chip", C.c_uint32),
        ("doppler_max", C.c_uint32),
        ("doppler_step", C.c_uint32),
        ("max_dwells", C.c_uint32),
        ("bit_transition_flag", C.c_int32),
        ("use_CFAR_algorithm_flag", C.c_int32),
        ("num_doppler_bins_override", C.c_uint32),
        ("make_2_steps", C.c_int32),
        ("num_doppler_bins_step2", C.c_uint32),
        ("doppler_step2", C.c_float),
    ]


class AcqResult(C.Structure):
    """gc_acq_result."""
    _fields_ = [
        ("indext", C.c_uint32),
        ("doppler_hz", C.c_int32),
        ("doppler_index", C.c_uint32),
        ("test_statistics", C.c_float),
        ("mag", C.c_float),
        ("input_power", C.c_float),
        ("second_peak", C.c_float),
        ("second_peak_full_row", C.c_float),
        ("acq_delay_samples", C.c_double),
        ("acq_doppler_hz", C.c_double),
    ]


class LoopConf(C.Structure):
    """gc_loop_conf."""
    _fields_ = [
        ("fs_in", C.c_double), ("signal_carrier_freq_hz", C.c_double), ("code_chip_rate_hz", C.c_double),
        ("code_period_s", C.c_double), ("carrier_lock_th", C.c_double), ("acq_delay_samples", C.c_double),
        ("acq_doppler_hz", C.c_double), ("acq_samplestamp_samples", C.c_uint64), ("sample_counter", C.c_uint64),
        ("code_length_chips", C.c_uint32), ("code_samples_per_chip", C.c_uint32), ("vector_length", C.c_uint32),
        ("pull_in_time_s", C.c_uint32), ("veml", C.c_int32), ("pll_filter_order", C.c_int32), ("dll_filter_order", C.c_int32),
        ("enable_fll_pull_in", C.c_int32), ("enable_fll_steady_state", C.c_int32), ("cn0_samples", C.c_int32),
        ("cn0_min", C.c_int32), ("max_lock_fail", C.c_int32), ("pll_bw_hz", C.c_float), ("dll_bw_hz", C.c_float),
        ("fll_bw_hz", C.c_float), ("early_late_space_chips", C.c_float), ("very_early_late_space_chips", C.c_float),
        ("high_dyn_smoother_length", C.c_uint32),
    ]


class GlonassLoopConf(C.Structure):
    """gc_glonass_loop_conf: what the GLONASS L1 / L2 C/A tracking block knows at start_tracking()."""
    _fields_ = [
        ("fs_in", C.c_double), ("band_carrier_freq_hz", C.c_double), ("channel_offset_hz", C.c_double), ("carrier_lock_th", C.c_double),
        ("acq_delay_samples", C.c_double), ("acq_doppler_hz", C.c_double), ("acq_samplestamp_samples", C.c_uint64),
        ("sample_counter", C.c_uint64), ("vector_length", C.c_uint32), ("cn0_samples", C.c_int32), ("cn0_min", C.c_int32),
        ("max_lock_fail", C.c_int32), ("pll_bw_hz", C.c_float), ("dll_bw_hz", C.c_float), ("early_late_space_chips", C.c_float),
        ("reserved", C.c_uint32),
    ]


LOOP_RECORD_DTYPE = np.dtype([
    ("corr", np.float32, (10,)), ("carrier_doppler_hz", np.float32), ("code_freq_chips", np.float32),
    ("carr_phase_error_hz", np.float32), ("carr_error_filt_hz", np.float32), ("code_error_chips", np.float32),
    ("code_error_filt_chips", np.float32), ("cn0_db_hz", np.float32), ("carrier_lock_test", np.float32),
    ("sample_counter", np.uint64), ("acc_carrier_phase_rad", np.float64), ("rem_code_phase_samples", np.float64),
    ("state", np.int32), ("valid", np.int32), ("current_prn_length_samples", np.int32), ("extend_count", np.int32),
    ("accu", np.float32, (10,)), ("prompt_data", np.float32, (2,)), ("integrating", np.int32), ("reserved", np.int32),
], align=True)


class LoopSyncConf(C.Structure):
    """gc_loop_sync_conf: symbol synchronisation, extended integration and pilot tracking of one channel."""
    _fields_ = [
        ("extend_correlation_symbols", C.c_int32), ("track_pilot", C.c_int32), ("symbols_per_bit", C.c_int32),
        ("secondary_code_length", C.c_int32), ("preamble_length_symbols", C.c_int32), ("bit_sync_min_time_s", C.c_float),
        ("pll_bw_narrow_hz", C.c_float), ("dll_bw_narrow_hz", C.c_float), ("early_late_space_narrow_chips", C.c_float),
        ("very_early_late_space_narrow_chips", C.c_float), ("secondary_code", C.c_char * 128), ("preamble_symbols", C.c_int8 * 192),
    ]

    @classmethod
    def make(cls, extend_correlation_symbols=1, track_pilot=False, symbols_per_bit=1, secondary_code="", preamble_symbols=(),
            bit_sync_min_time_s=10.0, pll_bw_narrow_hz=0.0, dll_bw_narrow_hz=0.0, early_late_space_narrow_chips=0.0,
            very_early_late_space_narrow_chips=0.0):
        y = cls()
        y.extend_correlation_symbols, y.track_pilot, y.symbols_per_bit = int(extend_correlation_symbols), int(bool(track_pilot)), int(symbols_per_bit)
        y.secondary_code_length, y.preamble_length_symbols = len(secondary_code), len(preamble_symbols)
        y.bit_sync_min_time_s = bit_sync_min_time_s
        y.pll_bw_narrow_hz, y.dll_bw_narrow_hz = pll_bw_narrow_hz, dll_bw_narrow_hz
        y.early_late_space_narrow_chips, y.very_early_late_space_narrow_chips = early_late_space_narrow_chips, very_early_late_space_narrow_chips
        if len(secondary_code) > 128 or len(preamble_symbols) > 192:
            raise ValueError("secondary code / preamble too long")
        y.secondary_code = secondary_code.encode()
        for i, v in enumerate(preamble_symbols):
            y.preamble_symbols[i] = int(v)
        return y


assert LOOP_RECORD_DTYPE.itemsize == 168 and C.sizeof(LoopConf) == 144 and C.sizeof(LoopSyncConf) == 360


class ConditionerConf(C.Structure):
    """gc_conditioner_conf: the frequency-translating FIR decimator in front of a ring."""
    _fields_ = [
        ("fs_in", C.c_double), ("translate_hz", C.c_double), ("decimation", C.c_uint32), ("n_taps", C.c_uint32),
        ("in_format", C.c_int32), ("reserved", C.c_int32),
    ]


assert C.sizeof(ConditionerConf) == 32


class BlankingConf(C.Structure):
    """gc_blanking_conf: pulse blanking on the conditioner's raw samples (the reference's Pulse_Blanking_Filter)."""
    _fields_ = [
        ("pfa", C.c_float), ("threshold", C.c_float), ("length", C.c_uint32), ("segments_est", C.c_uint32),
        ("segments_reset", C.c_uint32), ("reserved", C.c_uint32),
    ]


assert C.sizeof(BlankingConf) == 24


class ResamplerConf(C.Structure):
    """gc_resampler_conf: the ring resampler's rates, mode and (polyphase mode) tap bank."""
    _fields_ = [
        ("fs_in", C.c_double), ("fs_out", C.c_double), ("mode", C.c_int32), ("phases", C.c_uint32), ("taps_per_phase", C.c_uint32),
        ("reserved", C.c_uint32), ("bank", C.POINTER(C.c_float)),
    ]


assert C.sizeof(ResamplerConf) == 40


class NotchConf(C.Structure):
    """gc_notch_conf: the notch filter ring stage (the reference's Notch_Filter / Notch_Filter_Lite)."""
    _fields_ = [
        ("pfa", C.c_float), ("threshold", C.c_float), ("p_c_factor", C.c_float), ("length", C.c_uint32), ("segments_est", C.c_uint32),
        ("segments_reset", C.c_uint32), ("segments_coeff", C.c_uint32), ("mode", C.c_int32), ("noise_floor", C.c_int32),
        ("reserved", C.c_uint32 * 3),
    ]


assert C.sizeof(NotchConf) == 48


class SiggenComponent(C.Structure):
    """gc_siggen_component: one component of a generated satellite (table, secondary code, data, axis, gain)."""
    _fields_ = [
        ("table", C.POINTER(C.c_float)), ("secondary", C.POINTER(C.c_int8)), ("secondary_len", C.c_uint32), ("periods_per_symbol", C.c_uint32),
        ("period_offset", C.c_uint32), ("axis", C.c_int32), ("gain", C.c_float), ("reserved", C.c_uint32),
    ]


class SiggenSat(C.Structure):
    """gc_siggen_sat: one satellite of a SignalGenerator."""
    _fields_ = [
        ("doppler_hz", C.c_double), ("carrier_phase0_turns", C.c_double), ("code_phase0_periods", C.c_double), ("code_periods_per_sample", C.c_double),
        ("amplitude", C.c_double), ("table_len", C.c_uint32), ("n_components", C.c_uint32), ("comp", SiggenComponent * 2),
    ]


class SiggenConf(C.Structure):
    """gc_siggen_conf: the scene of a SignalGenerator."""
    _fields_ = [
        ("fs_hz", C.c_double), ("noise_sigma", C.c_double), ("seed", C.c_uint64), ("t0", C.c_uint64), ("n_sats", C.c_uint32),
        ("table_placement", C.c_uint32), ("sats", C.POINTER(SiggenSat)),
    ]


assert C.sizeof(SiggenComponent) == 40 and C.sizeof(SiggenSat) == 128 and C.sizeof(SiggenConf) == 48


# every symbol include/gnsscorr.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
_fp = C.POINTER(C.c_float)
_i16p = C.POINTER(C.c_int16)
API = {
    "gc_last_error": (C.c_char_p, []),
    "gc_version": (C.c_char_p, []),
    "gc_abi_check": (C.c_int, [C.c_size_t] * 6),
    "gc_device_count": (C.c_int, []),
    "gc_build_has_experiments": (C.c_int, []),
    "gc_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "gc_ctx_destroy": (C.c_int, [_vp]),
    "gc_ctx_synchronize": (C.c_int, [_vp]),
    "gc_correlator_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "gc_correlator_destroy": (C.c_int, [_vp]),
    "gc_correlator_set_high_dynamics_resampler": (C.c_int, [_vp, C.c_int]),
    "gc_correlator_init": (C.c_int, [_vp, C.c_int, C.c_int]),
    "gc_correlator_set_local_code_and_taps": (C.c_int, [_vp, C.c_int, _fp, _fp]),
    "gc_correlator_set_input_output_vectors": (C.c_int, [_vp, _fp, _fp]),
    "gc_correlator_carrier_wipeoff_multicorrelator_resampler": (C.c_int, [_vp] + [C.c_float] * 6 + [C.c_int]),
    "gc_correlator_carrier_wipeoff_multicorrelator_resampler_6": (C.c_int, [_vp] + [C.c_float] * 5 + [C.c_int]),
    "gc_correlator_free": (C.c_int, [_vp]),
    "gc_correlator_batch_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "gc_ctx_register_host_buffer": (C.c_int, [_vp, _vp, C.c_size_t]),
    "gc_ctx_unregister_host_buffer": (C.c_int, [_vp, _vp]),
    "gc_correlator_set_local_code_and_taps_complex": (C.c_int, [_vp, C.c_int, _fp, _fp]),
    "gc_correlator_carrier_wipeoff_multicorrelator_resampler_5": (C.c_int, [_vp] + [C.c_float] * 4 + [C.c_int]),
    "gc_correlator_set_local_code_and_taps_16sc": (C.c_int, [_vp, C.c_int, _i16p, _fp]),
    "gc_correlator_set_input_output_vectors_16sc": (C.c_int, [_vp, _i16p, _i16p]),
    "gc_epoch_params_fill": (None, [C.POINTER(EpochParams), C.c_uint64] + [C.c_float] * 6 + [C.c_int]),
    "gc_stream_create": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "gc_stream_destroy": (C.c_int, [_vp]),
    "gc_stream_push": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gc_stream_push_pinned": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gc_stream_broadcast_pinned": (C.c_int, [C.POINTER(_vp), C.c_int, _vp, C.c_uint64]),
    "gc_stream_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_stream_synchronize": (C.c_int, [_vp]),
    "gc_stream_read": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "gc_stream_debug_read_storage": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "gc_stream_debug_guards": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gc_stream_debug_set_origin": (C.c_int, [_vp, C.c_uint64]),
    "gc_stream_accept_quantised_output": (C.c_int, [_vp]),
    "gc_conditioner_conf_size": (C.c_size_t, []),
    "gc_conditioner_create": (C.c_int, [_vp, C.POINTER(ConditionerConf), _fp, _vp, C.POINTER(_vp)]),
    "gc_conditioner_destroy": (C.c_int, [_vp]),
    "gc_conditioner_push": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_conditioner_push_pinned": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_conditioner_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_conditioner_set_output_scale": (C.c_int, [_vp, C.c_float]),
    "gc_conditioner_output_info": (C.c_int, [_vp, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_uint64)]),
    "gc_fir_low_pass": (C.c_int, [C.c_double] * 4 + [_fp, C.c_int, C.POINTER(C.c_int)]),
    "gc_blanking_conf_size": (C.c_size_t, []),
    "gc_conditioner_set_pulse_blanking": (C.c_int, [_vp, C.POINTER(BlankingConf)]),
    "gc_conditioner_blanking_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _fp, C.POINTER(C.c_uint32), _fp]),
    "gc_chi2_upper_quantile": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "gc_trk_loop_set_input_format": (C.c_int, [_vp, C.c_int]),
    "gc_trk_loop_set_input_stream": (C.c_int, [_vp, C.c_int, _vp]),
    "gc_trk_batch_set_input_stream": (C.c_int, [_vp, C.c_int, _vp]),
    "gc_trk_batch_set_read_floor": (C.c_int, [_vp, C.c_uint64]),
    "gc_acq_set_frequency_offset": (C.c_int, [_vp, C.c_int64]),
    "gc_acq_dwell_stream": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "gc_trk_batch_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "gc_trk_batch_destroy": (C.c_int, [_vp]),
    "gc_trk_batch_set_code": (C.c_int, [_vp, C.c_int, _fp, C.c_int, _fp]),
    "gc_trk_batch_set_shifts": (C.c_int, [_vp, C.c_int, _fp]),
    "gc_trk_batch_set_complex_codes": (C.c_int, [_vp, C.c_int]),
    "gc_trk_batch_set_code_complex": (C.c_int, [_vp, C.c_int, _fp, C.c_int, _fp]),
    "gc_trk_batch_set_16sc": (C.c_int, [_vp, C.c_int]),
    "gc_trk_batch_set_code_16sc": (C.c_int, [_vp, C.c_int, _i16p, C.c_int, _fp]),
    "gc_trk_batch_set_input_format": (C.c_int, [_vp, C.c_int]),
    "gc_trk_batch_set_input_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_uint64]),
    "gc_trk_batch_run_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "gc_trk_batch_run": (C.c_int, [_vp, C.c_int, _vp, _fp]),
    "gc_trk_batch_set_nominal_length": (C.c_int, [_vp, C.c_int]),
    "gc_trk_batch_set_slices": (C.c_int, [_vp, C.c_int]),
    "gc_trk_loop_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "gc_trk_loop_destroy": (C.c_int, [_vp]),
    "gc_trk_loop_set_input_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_uint64]),
    "gc_trk_loop_set_sync": (C.c_int, [_vp, C.c_int, C.POINTER(LoopSyncConf), _fp, C.c_int]),
    "gc_loop_sync_for_signal": (C.c_int, [C.c_char, C.c_char_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(LoopSyncConf)]),
    "gc_trk_loop_start": (C.c_int, [_vp, C.c_int, C.POINTER(LoopConf), _fp, C.c_int]),
    "gc_glonass_loop_conf_size": (C.c_size_t, []),
    "gc_trk_loop_start_glonass": (C.c_int, [_vp, C.c_int, C.POINTER(GlonassLoopConf)]),
    "gc_glonass_loop_pull_in": (C.c_int, [C.POINTER(GlonassLoopConf), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "gc_trk_loop_stop": (C.c_int, [_vp, C.c_int]),
    "gc_trk_loop_run_dev": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "gc_trk_loop_set_geometry": (C.c_int, [_vp, C.c_int, C.c_int]),
    "gc_trk_loop_set_mixed": (C.c_int, [_vp, C.c_int]),
    "gc_trk_loop_run": (C.c_int, [_vp, C.c_int, _vp]),
    "gc_gps_l1_ca_code_gen_float": (C.c_int, [_fp, C.c_int32, C.c_uint32]),
    "gc_gps_l1_ca_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_glonass_l1_ca_code_gen_float": (C.c_int, [_fp, C.c_uint32]),
    "gc_glonass_l1_ca_code_gen_complex_sampled": (C.c_int, [_fp, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_beidou_b1i_code_gen_float": (C.c_int, [_fp, C.c_int32, C.c_uint32]),
    "gc_beidou_b1i_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_galileo_e1_code_gen_sinboc11_float": (C.c_int, [_fp, C.c_char_p, C.c_uint32]),
    "gc_galileo_e1_code_gen_complex_sampled": (C.c_int, [_fp, C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_gps_l2c_m_code_gen_float": (C.c_int, [_fp, C.c_uint32]),
    "gc_gps_l2c_m_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.POINTER(C.c_int32)]),
    "gc_gps_l5i_code_gen_float": (C.c_int, [_fp, C.c_uint32]),
    "gc_gps_l5q_code_gen_float": (C.c_int, [_fp, C.c_uint32]),
    "gc_gps_l5i_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.POINTER(C.c_int32)]),
    "gc_gps_l5q_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.POINTER(C.c_int32)]),
    "gc_beidou_b3i_code_gen_float": (C.c_int, [_fp, C.c_int32, C.c_uint32]),
    "gc_beidou_b3i_code_gen_complex_sampled": (C.c_int, [_fp, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_galileo_e5_a_code_gen_complex_primary": (C.c_int, [_fp, C.c_int32, C.c_char_p]),
    "gc_galileo_e5_a_code_gen_complex_sampled": (C.c_int, [_fp, C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "gc_secondary_code": (C.c_int, [C.c_char_p, C.c_uint32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    "gc_acq_create": (C.c_int, [_vp, C.POINTER(AcqConf), C.c_int, C.POINTER(_vp)]),
    "gc_acq_destroy": (C.c_int, [_vp]),
    "gc_acq_fft_size": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gc_acq_set_local_code": (C.c_int, [_vp, C.c_int, _fp]),
    "gc_acq_reset": (C.c_int, [_vp]),
    "gc_acq_set_step_two": (C.c_int, [_vp, C.c_int, C.c_float]),
    "gc_acq_set_input_format": (C.c_int, [_vp, C.c_int]),
    "gc_acq_dwell_dev": (C.c_int, [_vp, _vp, C.POINTER(AcqResult), _vp]),
    "gc_acq_dwell": (C.c_int, [_vp, _fp, C.POINTER(AcqResult)]),
    "gc_acq_dwell_enqueue": (C.c_int, [_vp, _vp, _vp]),
    "gc_acq_fetch_results": (C.c_int, [_vp, C.POINTER(AcqResult), _vp]),
    "gc_acq_flush": (C.c_int, [_vp, _vp]),
    "gc_acq_get_grid": (C.c_int, [_vp, C.c_int, _fp]),
    "gc_acq_peek": (C.c_int, [_vp, C.c_int, C.c_int, _fp]),
    "gc_acq_create_paired": (C.c_int, [_vp, C.POINTER(AcqConf), C.c_int, C.c_int, C.POINTER(_vp)]),
    "gc_acq_set_local_code_pair": (C.c_int, [_vp, C.c_int, _fp, _fp]),
    "gc_acq_create_quicksync": (C.c_int, [_vp, C.POINTER(AcqConf), C.c_int, C.c_uint32, C.POINTER(_vp)]),
    "gc_acq_quicksync_candidates": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint32), _fp]),
    "gc_quicksync_default_folding_factor": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32)]),
    "gc_quicksync_threshold": (C.c_int, [C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "gc_acq_create_tong": (C.c_int, [_vp, C.POINTER(AcqConf), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "gc_acq_tong_set_threshold": (C.c_int, [_vp, C.c_float]),
    "gc_acq_tong_status": (C.c_int, [_vp, _vp]),
    "gc_acq_tong_search_stream": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp]),
    "gc_tong_threshold": (C.c_int, [C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "gc_acq_create_caf": (C.c_int, [_vp, C.POINTER(AcqConf), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(_vp)]),
    "gc_acq_set_local_code_iq": (C.c_int, [_vp, C.c_int, _fp, _fp]),
    "gc_acq_caf_vectors": (C.c_int, [_vp, C.c_int, _fp, _fp, _fp, C.POINTER(C.c_uint8)]),
    "gc_fine_doppler_create": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "gc_fine_doppler_destroy": (C.c_int, [_vp]),
    "gc_fine_doppler_set_code": (C.c_int, [_vp, C.c_int, _fp]),
    "gc_fine_doppler_estimate_stream": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_int, _vp]),
    "gc_fine_doppler_estimate": (C.c_int, [_vp, _fp, _vp, C.c_int, _vp]),
    "gc_fine_doppler_spectrum": (C.c_int, [_vp, C.c_int, _fp]),
    "gc_fine_doppler_window": (C.c_int, [C.c_int64, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gc_fine_doppler_conf_size": (C.c_size_t, []),
    "gc_cccwsr_replicas": (C.c_int, [_fp, _fp, C.c_uint32, _fp, _fp]),
    "gc_e1_8ms_replicas": (C.c_int, [_fp, C.c_uint32, C.c_uint32, _fp, _fp]),
    "gc_ring_decimator_create": (C.c_int, [_vp, _vp, C.c_uint32, _fp, C.c_uint32, _vp, C.POINTER(_vp)]),
    "gc_ring_decimator_destroy": (C.c_int, [_vp]),
    "gc_ring_decimator_update": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_ring_decimator_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_ring_decimator_set_output_scale": (C.c_int, [_vp, C.c_float]),
    "gc_ring_decimator_output_info": (C.c_int, [_vp, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_uint64)]),
    "gc_acq_resampler_plan": (C.c_int, [C.c_int64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), _fp, C.c_int, C.POINTER(C.c_int),
        C.POINTER(C.c_uint32)]),
    "gc_resampler_conf_size": (C.c_size_t, []),
    "gc_ring_resampler_create": (C.c_int, [_vp, _vp, C.POINTER(ResamplerConf), _vp, C.POINTER(_vp)]),
    "gc_ring_resampler_destroy": (C.c_int, [_vp]),
    "gc_ring_resampler_update": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_ring_resampler_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_resampler_design": (C.c_int, [C.c_double, C.c_double, C.c_uint32, _fp, C.c_int, C.POINTER(C.c_int)]),
    "gc_notch_conf_size": (C.c_size_t, []),
    "gc_ring_notch_create": (C.c_int, [_vp, _vp, C.POINTER(NotchConf), _vp, C.POINTER(_vp)]),
    "gc_ring_notch_destroy": (C.c_int, [_vp]),
    "gc_ring_notch_update": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_ring_notch_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gc_ring_notch_state": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _fp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), _fp, _fp]),
    "gc_siggen_component_size": (C.c_size_t, []),
    "gc_siggen_sat_size": (C.c_size_t, []),
    "gc_siggen_conf_size": (C.c_size_t, []),
    "gc_signal_generator_create": (C.c_int, [_vp, C.POINTER(SiggenConf), _vp, C.POINTER(_vp)]),
    "gc_signal_generator_destroy": (C.c_int, [_vp]),
    "gc_signal_generator_generate": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gc_signal_generator_info": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "gc_signal_generator_set_output_scale": (C.c_int, [_vp, C.c_float]),
    "gc_signal_generator_output_info": (C.c_int, [_vp, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_uint64)]),
    "gc_signal_generator_plan": (C.c_int, [C.POINTER(SiggenSat), C.c_double] + [C.POINTER(C.c_uint64)] * 4),
    "gc_siggen_reference_satellite": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double,
        C.c_int, C.c_int, C.c_double, C.POINTER(SiggenSat), _fp, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_double)]),
}

_lib = None


def load_library():
    """Loads libgnsscorr.so (built by gnss-sdr-1_amd/csrc/Makefile).  Raises
    when it is missing: the HIP library IS the product."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GnsscorrError(GC_ERR_NO_DEVICE, "%s not built (run __graft_entry__.build())" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own
        # libamdhip64.so.7.  When torch is going to share the process (device
        # buffers for tests/bench) it must be loaded first, so that this library
        # binds to the same runtime instead of /opt/rocm's copy.
        if os.environ.get("GNSSCORR_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in API.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        # the ctypes mirrors above against the library that was actually loaded
        st = lib.gc_abi_check(C.sizeof(EpochParams), C.sizeof(LoopConf), LOOP_RECORD_DTYPE.itemsize, C.sizeof(LoopSyncConf), C.sizeof(AcqConf), C.sizeof(AcqResult))
        if st != 0:
            raise GnsscorrError(st, lib.gc_last_error().decode() + " -- rebuild with __graft_entry__.build()")
        if lib.gc_conditioner_conf_size() != C.sizeof(ConditionerConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_conditioner_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_conditioner_conf_size(), C.sizeof(ConditionerConf)))
        if lib.gc_blanking_conf_size() != C.sizeof(BlankingConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_blanking_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_blanking_conf_size(), C.sizeof(BlankingConf)))
        if lib.gc_glonass_loop_conf_size() != C.sizeof(GlonassLoopConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_glonass_loop_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_glonass_loop_conf_size(), C.sizeof(GlonassLoopConf)))
        if lib.gc_resampler_conf_size() != C.sizeof(ResamplerConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_resampler_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_resampler_conf_size(), C.sizeof(ResamplerConf)))
        if lib.gc_notch_conf_size() != C.sizeof(NotchConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_notch_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_notch_conf_size(), C.sizeof(NotchConf)))
        for what, mirror in (("gc_siggen_component", SiggenComponent), ("gc_siggen_sat", SiggenSat), ("gc_siggen_conf", SiggenConf)):
            if getattr(lib, what + "_size")() != C.sizeof(mirror):
                raise GnsscorrError(GC_ERR_INVALID, "%s is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                    % (what, getattr(lib, what + "_size")(), C.sizeof(mirror)))
        if lib.gc_fine_doppler_conf_size() != C.sizeof(FineDopplerConf):
            raise GnsscorrError(GC_ERR_INVALID, "gc_fine_doppler_conf is %d bytes in the library, %d here -- rebuild with __graft_entry__.build()"
                % (lib.gc_fine_doppler_conf_size(), C.sizeof(FineDopplerConf)))
        _lib = lib
    return _lib


def _check(st):
    if st != GC_OK:
        raise GnsscorrError(st, load_library().gc_last_error().decode())


def _f32p(a):
    return a.ctypes.data_as(_fp)


def device_count():
    return load_library().gc_device_count()


def epoch_params(sample_offset, rem_carr_phase_rad, carr_phase_step_rad, rem_code_phase_chips,
        code_phase_step_chips, n_samples, carr_phase_rate_step_rad=0.0, code_phase_rate_step_chips=0.0):
    """gc_epoch_params_fill: the reference's scalar arguments -> kernel arguments
    (cpu_multicorrelator_real_codes.cc:141-149)."""
    p = EpochParams()
    load_library().gc_epoch_params_fill(C.byref(p), int(sample_offset), rem_carr_phase_rad, carr_phase_step_rad,
        carr_phase_rate_step_rad, rem_code_phase_chips, code_phase_step_chips, code_phase_rate_step_chips, int(n_samples))
    return p


def epoch_params_array(records):
    """list (or nested list [ch][epoch]) of EpochParams -> numpy structured array."""
    flat = []
    for r in records:
        if isinstance(r, (list, tuple)):
            flat.extend(r)
        else:
            flat.append(r)
    out = np.zeros(len(flat), EPOCH_DTYPE)
    for i, p in enumerate(flat):
        out[i] = np.frombuffer(bytes(p), EPOCH_DTYPE)[0]
    return out


# ---- PRN replica generators (host side; names follow the reference's free functions) ----
def gps_l1_ca_code_gen_float(prn, chip_shift=0):
    d = np.zeros(1023, np.float32)
    _check(load_library().gc_gps_l1_ca_code_gen_float(_f32p(d), prn, chip_shift))
    return d


def gps_l1_ca_code_gen_complex_sampled(prn, fs, chip_shift=0):
    d = np.zeros(int(fs // 1000) + 8, np.complex64)
    n = C.c_int32()
    _check(load_library().gc_gps_l1_ca_code_gen_complex_sampled(d.view(np.float32).ctypes.data_as(_fp), prn, fs, chip_shift, C.byref(n)))
    return d[:n.value].copy()


def glonass_l1_ca_code_gen_float(chip_shift=0):
    d = np.zeros(511, np.float32)
    _check(load_library().gc_glonass_l1_ca_code_gen_float(_f32p(d), chip_shift))
    return d


def glonass_l1_ca_code_gen_complex_sampled(fs, chip_shift=0):
    d = np.zeros(int(fs // 1000) + 8, np.complex64)
    n = C.c_int32()
    _check(load_library().gc_glonass_l1_ca_code_gen_complex_sampled(d.view(np.float32).ctypes.data_as(_fp), fs, chip_shift, C.byref(n)))
    return d[:n.value].copy()


def beidou_b1i_code_gen_float(prn, chip_shift=0):
    d = np.zeros(2046, np.float32)
    _check(load_library().gc_beidou_b1i_code_gen_float(_f32p(d), prn, chip_shift))
    return d


def beidou_b1i_code_gen_complex_sampled(prn, fs, chip_shift=0):
    d = np.zeros(int(fs // 1000) + 8, np.complex64)
    n = C.c_int32()
    _check(load_library().gc_beidou_b1i_code_gen_complex_sampled(d.view(np.float32).ctypes.data_as(_fp), prn, fs, chip_shift, C.byref(n)))
    return d[:n.value].copy()


def _chips10230(fn, *args):
    d = np.zeros(10230, np.float32)
    _check(getattr(load_library(), fn)(_f32p(d), *args))
    return d


def _sampled10230(fn, fs, code_rate_hz, *args):
    d = np.zeros(int(fs / (code_rate_hz / 10230.0)) + 8, np.complex64)
    n = C.c_int32()
    _check(getattr(load_library(), fn)(d.view(np.float32).ctypes.data_as(_fp), *args, C.byref(n)))
    return d[:n.value].copy()


def gps_l2c_m_code_gen_float(prn):
    return _chips10230("gc_gps_l2c_m_code_gen_float", prn)


def gps_l2c_m_code_gen_complex_sampled(prn, fs):
    return _sampled10230("gc_gps_l2c_m_code_gen_complex_sampled", fs, 0.5115e6, prn, fs)


def gps_l5i_code_gen_float(prn):
    return _chips10230("gc_gps_l5i_code_gen_float", prn)


def gps_l5q_code_gen_float(prn):
    return _chips10230("gc_gps_l5q_code_gen_float", prn)


def gps_l5i_code_gen_complex_sampled(prn, fs):
    return _sampled10230("gc_gps_l5i_code_gen_complex_sampled", fs, 10.23e6, prn, fs)


def gps_l5q_code_gen_complex_sampled(prn, fs):
    return _sampled10230("gc_gps_l5q_code_gen_complex_sampled", fs, 10.23e6, prn, fs)


def beidou_b3i_code_gen_float(prn, chip_shift=0):
    return _chips10230("gc_beidou_b3i_code_gen_float", prn, chip_shift)


def beidou_b3i_code_gen_complex_sampled(prn, fs, chip_shift=0):
    return _sampled10230("gc_beidou_b3i_code_gen_complex_sampled", fs, 10.23e6, prn, fs, chip_shift)


def galileo_e5_a_code_gen_complex_primary(prn, signal):
    d = np.zeros(10230, np.complex64)
    _check(load_library().gc_galileo_e5_a_code_gen_complex_primary(d.view(np.float32).ctypes.data_as(_fp), prn, signal.encode()))
    return d


def galileo_e5_a_code_gen_complex_sampled(signal, prn, fs, chip_shift=0):
    return _sampled10230("gc_galileo_e5_a_code_gen_complex_sampled", fs, 10.23e6, signal.encode(), prn, fs, chip_shift)


def loop_sync_for_signal(system, signal, prn, track_pilot=False, extend_correlation_symbols=1):
    """gc_loop_sync_for_signal: the LoopSyncConf the block's constructor would derive for this signal and satellite."""
    y = LoopSyncConf()
    _check(load_library().gc_loop_sync_for_signal(system.encode(), signal.encode(), prn, int(bool(track_pilot)), extend_correlation_symbols, C.byref(y)))
    return y


def secondary_code(signal, prn=0):
    """Secondary (overlay) code of a signal as a '0'/'1' string: "1C", "B1", "B3", "L5I", "L5Q", "5I", "5Q" (per PRN)."""
    buf = C.create_string_buffer(128)
    n = C.c_int32()
    _check(load_library().gc_secondary_code(signal.encode(), prn, buf, 128, C.byref(n)))
    return buf.value.decode()


def galileo_e1_code_gen_sinboc11_float(signal, prn):
    d = np.zeros(8184, np.float32)
    _check(load_library().gc_galileo_e1_code_gen_sinboc11_float(_f32p(d), signal.encode(), prn))
    return d


def galileo_e1_code_gen_complex_sampled(signal, cboc, prn, fs, chip_shift=0):
    d = np.zeros(int(fs * 0.004) + 8, np.complex64)
    n = C.c_int32()
    _check(load_library().gc_galileo_e1_code_gen_complex_sampled(d.view(np.float32).ctypes.data_as(_fp), signal.encode(), int(cboc), prn, fs,
        chip_shift, C.byref(n)))
    return d[:n.value].copy()


def _c64p(a):
    return a.view(np.float32).ctypes.data_as(_fp)


def cccwsr_replicas(code_data, code_pilot):
    """gc_cccwsr_replicas: (cd - j cp, cd + j cp), the two complex replicas whose correlations are the d + jp and d - jp of
    pcps_cccwsr_acquisition_cc.cc:342-351."""
    cd = np.ascontiguousarray(code_data, np.complex64)
    cp = np.ascontiguousarray(code_pilot, np.complex64)
    assert cd.shape == cp.shape and cd.ndim == 1, (cd.shape, cp.shape)
    a, b = np.zeros_like(cd), np.zeros_like(cd)
    _check(load_library().gc_cccwsr_replicas(_c64p(cd), _c64p(cp), cd.size, _c64p(a), _c64p(b)))
    return a, b


def e1_8ms_replicas(code, samples_per_code):
    """gc_e1_8ms_replicas: the block's code A and code B, the second code period negated (galileo_pcps_8ms_acquisition_cc.cc:150-165)."""
    code = np.ascontiguousarray(code, np.complex64)
    assert code.ndim == 1, code.shape
    a, b = np.zeros_like(code), np.zeros_like(code)
    _check(load_library().gc_e1_8ms_replicas(_c64p(code), code.size, int(samples_per_code), _c64p(a), _c64p(b)))
    return a, b


def quicksync_default_folding_factor(code_length):
    """gc_quicksync_default_folding_factor: ceil(sqrt(log2(code_length))), the QuickSync adapters' default."""
    out = C.c_uint32()
    _check(load_library().gc_quicksync_default_folding_factor(int(code_length), C.byref(out)))
    return out.value


def tong_threshold(pfa, vector_length, doppler_max, doppler_step):
    """gc_tong_threshold: calculate_threshold of the Tong adapters."""
    out = C.c_float()
    _check(load_library().gc_tong_threshold(float(pfa), int(vector_length), int(doppler_max), int(doppler_step), C.byref(out)))
    return out.value


class AcqTongStatus(C.Structure):
    """struct gc_acq_tong_status."""
    _fields_ = [("state", C.c_int32), ("tong_count", C.c_uint32), ("dwell_count", C.c_uint32)]


TONG_RUNNING, TONG_POSITIVE, TONG_NEGATIVE = 0, 1, 2


class FineDopplerConf(C.Structure):
    """gc_fine_doppler_conf."""
    _fields_ = [("fs_in", C.c_int64), ("samples_per_code", C.c_uint32), ("prn_replicas", C.c_uint32), ("zero_padding_factor", C.c_uint32),
        ("window_hz", C.c_float), ("alignment", C.c_int32)]


class FineDopplerRequest(C.Structure):
    """gc_fine_doppler_request."""
    _fields_ = [("slot", C.c_uint32), ("delay_samples", C.c_uint32), ("coarse_doppler_hz", C.c_double)]


class FineDopplerResult(C.Structure):
    """gc_fine_doppler_result."""
    _fields_ = [("doppler_hz", C.c_double), ("bin", C.c_uint32), ("status", C.c_int32), ("peak", C.c_float), ("mean", C.c_float),
        ("window_first_bin", C.c_uint32), ("window_bins", C.c_uint32)]


FINE_ALIGN_REFERENCE, FINE_ALIGN_EXACT = 0, 1
CAF_REFERENCE, CAF_EXACT = 0, 1
FINE_REFINED, FINE_EDGE = 1, 2


def fine_doppler_window(fs_in, next_size, coarse_hz, window_hz=1000.0):
    """gc_fine_doppler_window: (first_bin, bins), the circular run of {k : |f[k] - coarse_hz| < window_hz} of the block's float32
    frequency table of next_size entries.  Host rule, no device."""
    a, b = C.c_uint32(), C.c_uint32()
    _check(load_library().gc_fine_doppler_window(int(fs_in), int(next_size), float(coarse_hz), float(window_hz), C.byref(a), C.byref(b)))
    return a.value, b.value


def quicksync_threshold(pfa, code_length, folding_factor, doppler_max, doppler_step):
    """gc_quicksync_threshold: calculate_threshold of the QuickSync adapters."""
    out = C.c_float()
    _check(load_library().gc_quicksync_threshold(float(pfa), int(code_length), int(folding_factor), int(doppler_max), int(doppler_step), C.byref(out)))
    return out.value


class Context:
    """gc_ctx: one per GPU."""

    def __init__(self, device=0):
        self._h = _vp()
        _check(load_library().gc_ctx_create(device, C.byref(self._h)))
        self.device = device

    def synchronize(self):
        _check(load_library().gc_ctx_synchronize(self._h))

    def register_host_buffer(self, array):
        """gc_ctx_register_host_buffer on a numpy array (the caller keeps it alive until unregister_host_buffer)."""
        _check(load_library().gc_ctx_register_host_buffer(self._h, _vp(array.ctypes.data), array.nbytes))

    def unregister_host_buffer(self, array):
        _check(load_library().gc_ctx_unregister_host_buffer(self._h, _vp(array.ctypes.data)))

    def correlator_batch_stats(self):
        """(launches, calls served, calls that shared their window's upload, largest batch) of the level-1 epoch batcher."""
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _check(load_library().gc_correlator_batch_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def close(self):
        if self._h:
            load_library().gc_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IqStream:
    """HBM ring of one RF stream (gc_stream_*): push host blocks once, every channel / acquisition of the
    stream reads them by absolute sample number."""
    _DTYPES = {GC_IQ_F32: (np.complex64, 1), GC_IQ_I16: (np.int16, 2), GC_IQ_I8: (np.int8, 2)}

    def __init__(self, ctx, capacity_samples, max_window_samples, iq_format=GC_IQ_F32):
        self._ctx = ctx
        self.iq_format = iq_format
        self._h = _vp()
        _check(load_library().gc_stream_create(ctx._h, int(iq_format), int(capacity_samples), int(max_window_samples), C.byref(self._h)))

    def push(self, block):
        """block: complex64 [n] (GC_IQ_F32) or int16 / int8 [n, 2].  Returns the absolute index of its first sample."""
        dt, per = self._DTYPES[self.iq_format]
        block = np.ascontiguousarray(block, dt)
        n = block.size // per
        first = C.c_uint64(0)
        _check(load_library().gc_stream_push(self._h, block.ctypes.data_as(_vp), n, C.byref(first)))
        return int(first.value)

    def push_pinned(self, host_ptr, n_samples):
        """host_ptr: address of page-locked host memory (e.g. a pinned torch tensor's data_ptr()); no staging copy."""
        first = C.c_uint64(0)
        _check(load_library().gc_stream_push_pinned(self._h, _vp(host_ptr), int(n_samples), C.byref(first)))
        return int(first.value)

    def info(self):
        o, h, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(load_library().gc_stream_info(self._h, C.byref(o), C.byref(h), C.byref(c)))
        return int(o.value), int(h.value), int(c.value)

    def synchronize(self):
        _check(load_library().gc_stream_synchronize(self._h))

    def accept_quantised_output(self):
        """gc_stream_accept_quantised_output: opens this empty GC_IQ_I16 / GC_IQ_I8 ring as the output ring of a Conditioner or
        RingDecimator (which refuse an integer ring otherwise).  Returns self."""
        _check(load_library().gc_stream_accept_quantised_output(self._h))
        return self

    def read(self, first_index, n):
        """gc_stream_read: the resident window [first_index, first_index + n) in the ring's format -- complex64 [n] or
        int16 / int8 [n, 2].  Synchronous; GC_ERR_STATE when the window is not resident."""
        dt, per = self._DTYPES[self.iq_format]
        out = np.zeros(int(n) if per == 1 else (int(n), per), dt)
        _check(load_library().gc_stream_read(self._h, int(first_index), int(n), out.ctypes.data_as(_vp)))
        return out

    def read_storage(self, position, n):
        """gc_stream_debug_read_storage (diagnostic): the raw storage positions [position, position + n) -- the ring, then its
        mirror, then two samples of slack -- in the ring's format, with no residency check.  Synchronous."""
        dt, per = self._DTYPES[self.iq_format]
        out = np.zeros(int(n) if per == 1 else (int(n), per), dt)
        _check(load_library().gc_stream_debug_read_storage(self._h, int(position), int(n), out.ctypes.data_as(_vp)))
        return out

    def guards_intact(self):
        """gc_stream_debug_guards (diagnostic): (front, back) -- whether the guard band in front of the ring's storage and the
        one behind it still hold the byte they were filled with."""
        front, back = C.c_int32(0), C.c_int32(0)
        _check(load_library().gc_stream_debug_guards(self._h, C.byref(front), C.byref(back)))
        return bool(front.value), bool(back.value)

    def set_origin(self, origin):
        """gc_stream_debug_set_origin (diagnostic): the empty ring starts at sample number `origin` (<= 2^62) as if that many samples
        had been pushed and evicted.  Once, before the first push and before a stage claims the ring.  Returns self."""
        origin = int(origin)
        if not 0 <= origin < 1 << 64:
            raise ValueError("origin is outside 0 .. 2^64 - 1")
        _check(load_library().gc_stream_debug_set_origin(self._h, origin))
        return self

    def close(self):
        if self._h:
            load_library().gc_stream_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fir_low_pass(gain, fs, cutoff_hz, transition_hz):
    """gc_fir_low_pass: Hamming-windowed sinc of odd length (int)(53 fs / (22 transition_hz)) | 1 with sum(h) = gain; float32 taps."""
    n = C.c_int(0)
    _check(load_library().gc_fir_low_pass(gain, fs, cutoff_hz, transition_hz, None, 0, C.byref(n)))
    taps = np.zeros(n.value, np.float32)
    _check(load_library().gc_fir_low_pass(gain, fs, cutoff_hz, transition_hz, _f32p(taps), n.value, C.byref(n)))
    return taps


def pack_2bit(values):
    """GC_RAW_REAL_2BIT bytes (uint8 [n / 4]) from integers in {-2, -1, 0, 1} ([n], n a multiple of 4): sample 4b + i goes to bits
    2i .. 2i + 1 of byte b, least-significant pair first, as a two's-complement 2-bit integer (-2 -> 0b10, -1 -> 0b11)."""
    v = np.asarray(values)
    if v.ndim != 1 or v.size % 4 != 0:
        raise ValueError("pack_2bit: need a one-dimensional array whose length is a multiple of 4")
    if v.size and (v.min() < -2 or v.max() > 1 or np.any(v != np.round(v))):
        raise ValueError("pack_2bit: values must be integers in -2 .. 1")
    q = (v.astype(np.int64) & 3).astype(np.uint8).reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)


def unpack_2bit(packed):
    """The samples of GC_RAW_REAL_2BIT bytes (uint8 or int8 [n / 4]) as int8 [n] in {-2, -1, 0, 1}: the inverse of pack_2bit."""
    b = np.ascontiguousarray(packed).view(np.uint8).reshape(-1)
    q = ((b[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).astype(np.int8)
    return np.where(q >= 2, q - 4, q).astype(np.int8).reshape(-1)


def chi2_upper_quantile(dof, pfa):
    """gc_chi2_upper_quantile: x with P(chi-squared with `dof` degrees of freedom > x) = pfa (float64)."""
    out = C.c_double(0.0)
    _check(load_library().gc_chi2_upper_quantile(float(dof), float(pfa), C.byref(out)))
    return float(out.value)


class _RingStage:
    """Handle of a stage that writes a ring on the device (Conditioner, RingDecimator, RingResampler): the calls that differ between
    the stages in the C prefix alone.  A subclass names its prefix in _C and sets self._h."""
    _C = None

    def _call(self, name, *args):
        _check(getattr(load_library(), "%s_%s" % (self._C, name))(self._h, *args))

    def _pair(self, name):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._call(name, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def info(self):
        """(source head the newest update saw, output ring head)."""
        return self._pair("info")

    def _output_info(self):
        fmt, scale, n = C.c_int32(0), C.c_float(0.0), C.c_uint64(0)
        self._call("output_info", C.byref(fmt), C.byref(scale), C.byref(n))
        return int(fmt.value), float(scale.value), int(n.value)

    def close(self):
        if self._h:
            getattr(load_library(), self._C + "_destroy")(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DerivedRing(_RingStage):
    """A stage whose input is another ring: update() appends what the source's samples so far complete."""

    def update(self):
        """Returns (number of the first new output, new outputs).  Asynchronous on the output ring's copy stream."""
        return self._pair("update")


class Conditioner(_RingStage):
    """gc_conditioner: raw samples of any gc_iq_format or gc_raw_real_format at fs_in are mixed down by translate_hz, filtered with
    `taps` and decimated on the device into `out_ring` (an empty GC_IQ_F32 IqStream, or an integer one after accept_quantised_output()), which consumers then read at
    fs_in / decimation.  A GC_IQ_I16 / GC_IQ_I8 ring receives each component scaled, clamped and rounded (set_output_scale,
    output_info).  The filter's group delay, (len(taps) - 1) / 2 input samples, is the caller's to account for."""
    _C = "gc_conditioner"
    _REAL_DTYPES = {GC_RAW_REAL_F32: np.float32, GC_RAW_REAL_I16: np.int16, GC_RAW_REAL_I8: np.int8}

    def __init__(self, ctx, out_ring, fs_in, translate_hz, decimation, taps, in_format=GC_IQ_F32):
        self._ctx = ctx
        self._ring = out_ring
        self.in_format = in_format
        self.taps = np.ascontiguousarray(taps, np.float32)
        self.conf = ConditionerConf(float(fs_in), float(translate_hz), int(decimation), int(self.taps.size), int(in_format), 0)
        self._h = _vp()
        _check(load_library().gc_conditioner_create(ctx._h, C.byref(self.conf), _f32p(self.taps), out_ring._h, C.byref(self._h)))

    def push(self, block, n_samples=None):
        """block: complex64 [n] (GC_IQ_F32) or int16 / int8 [n, 2]; float32 / int16 / int8 [n] for the real formats; uint8 or int8
        [n / 4] for GC_RAW_REAL_2BIT (see pack_2bit).  n_samples: push only the first n_samples of the block.  Returns (number of
        the first new output, new outputs)."""
        if self.in_format == GC_RAW_REAL_2BIT:
            block = np.ascontiguousarray(block)
            if block.dtype not in (np.uint8, np.int8) or block.ndim != 1:
                raise ValueError("GC_RAW_REAL_2BIT takes a uint8 or int8 array of shape [n / 4]")
            n = 4 * block.size
        elif self.in_format in self._REAL_DTYPES:
            block = np.ascontiguousarray(block, self._REAL_DTYPES[self.in_format])
            if block.ndim != 1:
                raise ValueError("a real format takes an array of shape [n]")
            n = block.size
        else:
            dt, per = IqStream._DTYPES[self.in_format]
            block = np.ascontiguousarray(block, dt)
            n = block.size // per
        if n_samples is not None:
            if not 0 <= int(n_samples) <= n:
                raise ValueError("n_samples is outside the block")
            n = int(n_samples)
        first, n_out = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().gc_conditioner_push(self._h, block.ctypes.data_as(_vp), n, C.byref(first), C.byref(n_out)))
        return int(first.value), int(n_out.value)

    def push_pinned(self, host_ptr, n_in):
        """host_ptr: address of page-locked host memory; it stays untouched until the output ring is synchronised."""
        first, n_out = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().gc_conditioner_push_pinned(self._h, _vp(host_ptr), int(n_in), C.byref(first), C.byref(n_out)))
        return int(first.value), int(n_out.value)

    def info(self):
        """(raw samples pushed, output ring head)."""
        return self._pair("info")

    def set_output_scale(self, scale):
        """gc_conditioner_set_output_scale: the factor in front of the clamp of a GC_IQ_I16 / GC_IQ_I8 output ring (default 1; 127
        is the reference's translating filter with cbyte output).  Only before the first push; GC_ERR_INVALID on a GC_IQ_F32 ring."""
        _check(load_library().gc_conditioner_set_output_scale(self._h, float(scale)))

    def output_info(self):
        """gc_conditioner_output_info (synchronous): (output ring's format, scale, clipped components so far)."""
        return self._output_info()

    def set_pulse_blanking(self, pfa=0.04, length=32, segments_est=12500, segments_reset=5000000, threshold=None):
        """gc_conditioner_set_pulse_blanking (defaults: the reference adapter's): segments of `length` raw samples whose energy
        exceeds `threshold` times the estimated noise floor are zeroed before the mixer and the filter.  threshold None: the
        upper-pfa chi-squared quantile with 2 * length degrees of freedom (length for the real formats; GC_RAW_REAL_2BIT is not
        blanked: GC_ERR_INVALID).  Only before the first push."""
        self.blanking = BlankingConf(float(pfa), 0.0 if threshold is None else float(threshold), int(length), int(segments_est),
            int(segments_reset), 0)
        _check(load_library().gc_conditioner_set_pulse_blanking(self._h, C.byref(self.blanking)))

    def blanking_info(self):
        """gc_conditioner_blanking_info (synchronous): dict(segments_decided, segments_blanked, noise_power, n_segments, threshold)."""
        d, b, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        noise, thr = C.c_float(0.0), C.c_float(0.0)
        _check(load_library().gc_conditioner_blanking_info(self._h, C.byref(d), C.byref(b), C.byref(noise), C.byref(n), C.byref(thr)))
        return dict(segments_decided=int(d.value), segments_blanked=int(b.value), noise_power=float(noise.value), n_segments=int(n.value),
            threshold=float(thr.value))


class RingDecimator(_DerivedRing):
    """gc_ring_decimator: y[m] = sum_k taps[k] x[m decimation - k] from the ring `src` (any format; pushed, or fed by a Conditioner)
    into `out_ring` (an empty GC_IQ_F32 IqStream, or an integer one after accept_quantised_output(), which receives the
    conditioner's quantisation), on the device.
    update() appends what the source's samples so far complete."""
    _C = "gc_ring_decimator"

    def __init__(self, ctx, src, decimation, taps, out_ring):
        self._ctx = ctx
        self._src = src
        self._ring = out_ring
        self.decimation = int(decimation)
        self.taps = np.ascontiguousarray(taps, np.float32)
        self._h = _vp()
        _check(load_library().gc_ring_decimator_create(ctx._h, src._h, self.decimation, _f32p(self.taps), int(self.taps.size), out_ring._h,
            C.byref(self._h)))

    def set_output_scale(self, scale):
        """gc_ring_decimator_set_output_scale: as Conditioner.set_output_scale; only before the first update."""
        _check(load_library().gc_ring_decimator_set_output_scale(self._h, float(scale)))

    def output_info(self):
        """gc_ring_decimator_output_info (synchronous): (output ring's format, scale, clipped components so far)."""
        return self._output_info()


def acq_resampler_plan(fs_in, opt_acq_fs_hz):
    """gc_acq_resampler_plan: (decimation, resampled_fs, taps, latency_samples) of the acquisition resampler for a ring at fs_in and a
    signal whose optimal search rate is opt_acq_fs_hz; decimation 1 with no taps when the reference would disable the resampler."""
    lib = load_library()
    d, rfs, n, lat = C.c_uint32(0), C.c_int64(0), C.c_int(0), C.c_uint32(0)
    _check(lib.gc_acq_resampler_plan(int(fs_in), int(opt_acq_fs_hz), C.byref(d), C.byref(rfs), None, 0, C.byref(n), C.byref(lat)))
    taps = np.zeros(n.value, np.float32)
    if n.value:
        _check(lib.gc_acq_resampler_plan(int(fs_in), int(opt_acq_fs_hz), C.byref(d), C.byref(rfs), _f32p(taps), n.value, C.byref(n), C.byref(lat)))
    return int(d.value), int(rfs.value), taps, int(lat.value)


def resampler_design(fs_in, fs_out, phases):
    """gc_resampler_design: the [phases, T] float32 bank of RingResampler's polyphase mode from the library's low-pass design --
    prototype gc_fir_low_pass(phases, phases * fs_in, min(fs_in, fs_out) / 2.1, min(fs_in, fs_out) / 10), bank[p, k] = g[k * phases + p]."""
    lib = load_library()
    t = C.c_int(0)
    _check(lib.gc_resampler_design(float(fs_in), float(fs_out), int(phases), None, 0, C.byref(t)))
    bank = np.zeros((int(phases), t.value), np.float32)
    _check(lib.gc_resampler_design(float(fs_in), float(fs_out), int(phases), _f32p(bank), bank.size, C.byref(t)))
    return bank


class RingResampler(_DerivedRing):
    """gc_ring_resampler: the ring `out` derived on the device from the ring `src` (any format; pushed, or fed by a Conditioner or a
    RingDecimator) at the rate ratio fs_in / fs_out.  mode "direct": the reference's Direct_Resampler, nearest earlier sample, bits
    as they are; `out` is an empty IqStream of src's format.  mode "polyphase": y[m] = sum_k bank[p_m, k] x[n_m - k] with `bank` a
    [P, T] float32 array (resampler_design makes one); `out` is an empty GC_IQ_F32 IqStream.  update() appends what the source's
    samples so far complete."""
    _C = "gc_ring_resampler"
    _MODES = {"direct": GC_RESAMP_DIRECT, "polyphase": GC_RESAMP_POLYPHASE, GC_RESAMP_DIRECT: GC_RESAMP_DIRECT, GC_RESAMP_POLYPHASE: GC_RESAMP_POLYPHASE}

    def __init__(self, ctx, src, fs_in, fs_out, out, mode="direct", bank=None):
        if mode not in self._MODES:
            raise ValueError("mode is 'direct' or 'polyphase'")
        self._ctx = ctx
        self._src = src
        self._ring = out
        self.mode = self._MODES[mode]
        self.bank = None
        phases = taps = 0
        if bank is not None:
            self.bank = np.ascontiguousarray(bank, np.float32)
            if self.bank.ndim != 2:
                raise ValueError("bank is a [phases, taps per phase] array")
            phases, taps = self.bank.shape
        self.conf = ResamplerConf(float(fs_in), float(fs_out), self.mode, phases, taps, 0, None if self.bank is None else _f32p(self.bank))
        self._h = _vp()
        _check(load_library().gc_ring_resampler_create(ctx._h, src._h, C.byref(self.conf), out._h, C.byref(self._h)))


class RingNotch(_DerivedRing):
    """gc_ring_notch: the GC_IQ_F32 ring `out` derived on the device from the GC_IQ_F32 ring `src` (pushed, or fed by a Conditioner or
    another derived ring) at the same rate, with continuous-wave interference notched out: the reference's Notch_Filter (mode "full")
    and Notch_Filter_Lite (mode "lite", one coefficient per `segments_coeff` filtered segments).  Defaults: the reference adapter's.
    noise_floor "reference" is the block's mean of decibels (biased low: it flags most pure-noise segments), "linear" the mean of
    powers over the same bins.  threshold None: the upper-pfa chi-squared quantile with 2 * length degrees of freedom.  update()
    appends the segments the source's samples so far complete."""
    _C = "gc_ring_notch"
    _MODES = {"full": GC_NOTCH_FULL, "lite": GC_NOTCH_LITE, GC_NOTCH_FULL: GC_NOTCH_FULL, GC_NOTCH_LITE: GC_NOTCH_LITE}
    _FLOORS = {"reference": GC_NOTCH_FLOOR_REFERENCE, "linear": GC_NOTCH_FLOOR_LINEAR, GC_NOTCH_FLOOR_REFERENCE: GC_NOTCH_FLOOR_REFERENCE,
        GC_NOTCH_FLOOR_LINEAR: GC_NOTCH_FLOOR_LINEAR}

    def __init__(self, ctx, src, out, pfa=0.001, p_c_factor=0.9, length=32, segments_est=12500, segments_reset=5000000, mode="full",
            segments_coeff=1, noise_floor="reference", threshold=None):
        if mode not in self._MODES:
            raise ValueError("mode is 'full' or 'lite'")
        if noise_floor not in self._FLOORS:
            raise ValueError("noise_floor is 'reference' or 'linear'")
        self._ctx = ctx
        self._src = src
        self._ring = out
        self.conf = NotchConf(float(pfa), 0.0 if threshold is None else float(threshold), float(p_c_factor), int(length), int(segments_est),
            int(segments_reset), int(segments_coeff), self._MODES[mode], self._FLOORS[noise_floor])
        self._h = _vp()
        _check(load_library().gc_ring_notch_create(ctx._h, src._h, C.byref(self.conf), out._h, C.byref(self._h)))

    def state(self):
        """gc_ring_notch_state (synchronous): dict(segments_decided, segments_filtered, noise_power, n_segments, active, threshold, last)."""
        d, f, n, act = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
        noise, thr, last = C.c_float(0.0), C.c_float(0.0), (C.c_float * 2)(0.0, 0.0)
        _check(load_library().gc_ring_notch_state(self._h, C.byref(d), C.byref(f), C.byref(noise), C.byref(n), C.byref(act), C.byref(thr), last))
        return dict(segments_decided=int(d.value), segments_filtered=int(f.value), noise_power=float(noise.value), n_segments=int(n.value),
            active=bool(act.value), threshold=float(thr.value), last=complex(last[0], last[1]))


class SiggenSatellite:
    """One satellite of a SignalGenerator: the gc_siggen_sat and the arrays its pointers lead into.  components: one or two dicts
    with `table` (float32 [table_len], one code period) and optionally `secondary` (+-1, int8 [<= 100]), `periods_per_symbol`
    (0: no data), `period_offset`, `axis` (0 real, 1 imaginary) and `gain`."""

    def __init__(self, doppler_hz, code_periods_per_sample, components, amplitude=1.0, carrier_phase0_turns=0.0, code_phase0_periods=0.0):
        components = list(components)
        if not 1 <= len(components) <= 2:
            raise ValueError("a satellite has one or two components")
        self._keep = []
        self.c = SiggenSat()
        self.c.doppler_hz, self.c.carrier_phase0_turns = float(doppler_hz), float(carrier_phase0_turns)
        self.c.code_phase0_periods, self.c.code_periods_per_sample = float(code_phase0_periods), float(code_periods_per_sample)
        self.c.amplitude = float(amplitude)
        self.c.n_components = len(components)
        self.tables, self.secondaries = [], []
        for i, comp in enumerate(components):
            table = np.ascontiguousarray(comp["table"], np.float32)
            if i and table.size != self.tables[0].size:
                raise ValueError("both components have table_len entries")
            self.tables.append(table)
            sec = comp.get("secondary")
            sec = None if sec is None else np.ascontiguousarray(sec, np.int8)
            self.secondaries.append(sec)
            k = self.c.comp[i]
            k.table = _f32p(table)
            k.secondary = None if sec is None else sec.ctypes.data_as(C.POINTER(C.c_int8))
            k.secondary_len = 0 if sec is None else int(sec.size)
            k.periods_per_symbol = int(comp.get("periods_per_symbol", 0))
            k.period_offset = int(comp.get("period_offset", 0))
            k.axis = int(comp.get("axis", 0))
            k.gain = float(comp.get("gain", 1.0))
        self.c.table_len = int(self.tables[0].size)

    @classmethod
    def _from_c(cls, sat, tables, secondaries):
        """Wraps a gc_siggen_sat the library filled; `tables` / `secondaries` are the arrays its pointers lead into."""
        self = cls.__new__(cls)
        self.c = sat
        self._keep = [tables, secondaries]
        n = int(sat.table_len)
        self.tables = [tables[i, :n] for i in range(int(sat.n_components))]
        self.secondaries = [secondaries[i, :int(sat.comp[i].secondary_len)] if sat.comp[i].secondary_len else None for i in range(int(sat.n_components))]
        return self


def siggen_plan(sat, fs_hz):
    """gc_signal_generator_plan (host only): the Q0.64 words (code_step_q, code_phase0_q, carr_step_q, carr_phase0_q) of a
    SiggenSatellite at the stream rate fs_hz -- floor(x 2^64) of each quantity in [0, 1)."""
    w = [C.c_uint64(0) for _ in range(4)]
    _check(load_library().gc_signal_generator_plan(C.byref(sat.c), float(fs_hz), *[C.byref(x) for x in w]))
    return tuple(int(x.value) for x in w)


def siggen_reference_satellite(system, signal, prn, cn0_db, doppler_hz, delay_chips, delay_sec, fs, bw_bb=1.0, data_flag=False, noise_flag=True,
        intermediate_freq_hz=4e6):
    """gc_siggen_reference_satellite: one satellite of the reference's Signal_Generator configuration (system "G" / "R" / "E", signal
    "1C" / "1G" / "1B" / "5X").  Returns (SiggenSatellite, noise_sigma)."""
    tables = np.zeros((2, GC_SIGGEN_MAX_TABLE), np.float32)
    secondaries = np.zeros((2, GC_SIGGEN_MAX_SECONDARY), np.int8)
    sat, sigma = SiggenSat(), C.c_double(0.0)
    _check(load_library().gc_siggen_reference_satellite(system.encode(), signal.encode(), int(prn), float(cn0_db), float(doppler_hz), int(delay_chips),
        int(delay_sec), float(fs), float(bw_bb), int(bool(data_flag)), int(bool(noise_flag)), float(intermediate_freq_hz), C.byref(sat), _f32p(tables),
        GC_SIGGEN_MAX_TABLE, secondaries.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(sigma)))
    return SiggenSatellite._from_c(sat, tables, secondaries), float(sigma.value)


class SignalGenerator(_RingStage):
    """gc_signal_generator: the source stage of a ring.  A HIP kernel synthesises the scene of `sats` (SiggenSatellite, 1..32) plus
    Gaussian noise of `noise_sigma` per part straight into `out_ring` (an empty GC_IQ_F32 IqStream, or an integer one after
    accept_quantised_output()); ring sample i is scenario sample t0 + i, a closed form of that number alone.  generate(n) appends."""
    _C = "gc_signal_generator"
    _PLACEMENTS = {"auto": GC_SIGGEN_TABLES_AUTO, "hbm": GC_SIGGEN_TABLES_HBM, "lds": GC_SIGGEN_TABLES_LDS}

    def __init__(self, ctx, out_ring, fs_hz, sats, noise_sigma=0.0, seed=0, t0=0, table_placement="auto"):
        self._ctx = ctx
        self._ring = out_ring
        self.sats = list(sats)
        self._sats_c = (SiggenSat * max(1, len(self.sats)))(*[s.c for s in self.sats])
        self.conf = SiggenConf(float(fs_hz), float(noise_sigma), int(seed), int(t0), len(self.sats), self._PLACEMENTS[table_placement], self._sats_c)
        self._h = _vp()
        _check(load_library().gc_signal_generator_create(ctx._h, C.byref(self.conf), out_ring._h, C.byref(self._h)))

    def generate(self, n_samples):
        """Appends n_samples samples (asynchronous on the ring's copy stream); returns the absolute number of the first."""
        first = C.c_uint64(0)
        self._call("generate", int(n_samples), C.byref(first))
        return int(first.value)

    def info(self):
        """Samples generated so far (the ring's head)."""
        head = C.c_uint64(0)
        self._call("info", C.byref(head))
        return int(head.value)

    def set_output_scale(self, scale):
        """gc_signal_generator_set_output_scale: as Conditioner.set_output_scale; only before the first generate."""
        self._call("set_output_scale", C.c_float(float(scale)))

    def output_info(self):
        """gc_signal_generator_output_info (synchronous): (output ring's format, scale, clipped components so far)."""
        return self._output_info()


class HipMulticorrelatorRealCodes:
    """Image of Cpu_Multicorrelator_Real_Codes
    (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:45-69): same
    methods, same argument meaning, pointers retained not copied, every method
    returns True."""

    def __init__(self, ctx):
        self._ctx = ctx
        self._h = _vp()
        _check(load_library().gc_correlator_create(ctx._h, C.byref(self._h)))
        self._keep = {}

    def set_high_dynamics_resampler(self, use_high_dynamics_resampler):
        _check(load_library().gc_correlator_set_high_dynamics_resampler(self._h, int(bool(use_high_dynamics_resampler))))

    def init(self, max_signal_length_samples, n_correlators):
        _check(load_library().gc_correlator_init(self._h, max_signal_length_samples, n_correlators))
        return True

    def set_local_code_and_taps(self, code_length_chips, local_code_in, shifts_chips):
        assert local_code_in.dtype == np.float32 and shifts_chips.dtype == np.float32
        self._keep["code"] = local_code_in
        self._keep["shifts"] = shifts_chips
        _check(load_library().gc_correlator_set_local_code_and_taps(self._h, code_length_chips, _f32p(local_code_in), _f32p(shifts_chips)))
        return True

    def set_input_output_vectors(self, corr_out, sig_in):
        assert corr_out.dtype == np.complex64 and sig_in.dtype == np.complex64
        self._keep["out"] = corr_out
        self._keep["in"] = sig_in
        _check(load_library().gc_correlator_set_input_output_vectors(self._h,
            corr_out.view(np.float32).ctypes.data_as(_fp), sig_in.view(np.float32).ctypes.data_as(_fp)))
        return True

    def Carrier_wipeoff_multicorrelator_resampler(self, rem_carrier_phase_in_rad, phase_step_rad, *rest):
        """7-argument form (…, phase_rate_step_rad, rem_code_phase_chips, code_phase_step_chips,
        code_phase_rate_step_chips, signal_length_samples) or the 6-argument overload without
        phase_rate_step_rad, as in the reference (.cc:129-170)."""
        lib = load_library()
        if len(rest) == 5:
            rate, rem_code, code_step, code_rate, n = rest
            _check(lib.gc_correlator_carrier_wipeoff_multicorrelator_resampler(self._h, rem_carrier_phase_in_rad,
                phase_step_rad, rate, rem_code, code_step, code_rate, int(n)))
        elif len(rest) == 4:
            rem_code, code_step, code_rate, n = rest
            _check(lib.gc_correlator_carrier_wipeoff_multicorrelator_resampler_6(self._h, rem_carrier_phase_in_rad,
                phase_step_rad, rem_code, code_step, code_rate, int(n)))
        else:
            raise TypeError("expected 6 or 7 arguments")
        return True

    def free(self):
        _check(load_library().gc_correlator_free(self._h))
        return True

    def close(self):
        if self._h:
            load_library().gc_correlator_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipMulticorrelator(HipMulticorrelatorRealCodes):
    """Image of Cpu_Multicorrelator (complex chips;
    src/algorithms/tracking/libs/cpu_multicorrelator.h:46-64): init, set_local_code_and_taps,
    set_input_output_vectors, the 5-argument Carrier_wipeoff_multicorrelator_resampler, free."""

    def set_high_dynamics_resampler(self, use_high_dynamics_resampler):
        raise AttributeError("Cpu_Multicorrelator has no high-dynamics resampler")

    def set_local_code_and_taps(self, code_length_chips, local_code_in, shifts_chips):
        assert local_code_in.dtype == np.complex64 and shifts_chips.dtype == np.float32
        self._keep["code"] = local_code_in
        self._keep["shifts"] = shifts_chips
        _check(load_library().gc_correlator_set_local_code_and_taps_complex(self._h, code_length_chips,
            local_code_in.view(np.float32).ctypes.data_as(_fp), _f32p(shifts_chips)))
        return True

    def Carrier_wipeoff_multicorrelator_resampler(self, rem_carrier_phase_in_rad, phase_step_rad, rem_code_phase_chips,
            code_phase_step_chips, signal_length_samples):
        _check(load_library().gc_correlator_carrier_wipeoff_multicorrelator_resampler_5(self._h, rem_carrier_phase_in_rad,
            phase_step_rad, rem_code_phase_chips, code_phase_step_chips, int(signal_length_samples)))
        return True


class HipMulticorrelator16sc(HipMulticorrelatorRealCodes):
    """Image of Cpu_Multicorrelator_16sc (src/algorithms/tracking/libs/cpu_multicorrelator_16sc.h:44-67):
    lv_16sc_t chips, input and output as int16 arrays of shape (n, 2)."""

    def set_high_dynamics_resampler(self, use_high_dynamics_resampler):
        raise AttributeError("Cpu_Multicorrelator_16sc has no high-dynamics resampler")

    def set_local_code_and_taps(self, code_length_chips, local_code_in, shifts_chips):
        assert local_code_in.dtype == np.int16 and local_code_in.shape[-1] == 2 and shifts_chips.dtype == np.float32
        self._keep["code"] = local_code_in
        self._keep["shifts"] = shifts_chips
        _check(load_library().gc_correlator_set_local_code_and_taps_16sc(self._h, code_length_chips,
            local_code_in.ctypes.data_as(_i16p), _f32p(shifts_chips)))
        return True

    def set_input_output_vectors(self, corr_out, sig_in):
        assert corr_out.dtype == np.int16 and sig_in.dtype == np.int16
        self._keep["out"] = corr_out
        self._keep["in"] = sig_in
        _check(load_library().gc_correlator_set_input_output_vectors_16sc(self._h, corr_out.ctypes.data_as(_i16p), sig_in.ctypes.data_as(_i16p)))
        return True

    def Carrier_wipeoff_multicorrelator_resampler(self, rem_carrier_phase_in_rad, phase_step_rad, rem_code_phase_chips,
            code_phase_step_chips, signal_length_samples):
        _check(load_library().gc_correlator_carrier_wipeoff_multicorrelator_resampler_5(self._h, rem_carrier_phase_in_rad,
            phase_step_rad, rem_code_phase_chips, code_phase_step_chips, int(signal_length_samples)))
        return True


def stream_broadcast_pinned(streams, host_ptr, n_samples):
    """gc_stream_broadcast_pinned: one page-locked block into the ring of every GPU."""
    arr = (_vp * len(streams))(*[s._h for s in streams])
    _check(load_library().gc_stream_broadcast_pinned(arr, len(streams), _vp(host_ptr), int(n_samples)))


def glonass_loop_pull_in(conf):
    """gc_glonass_loop_pull_in: the pull-in alignment a GLONASS start with `conf` (GlonassLoopConf) performs before its first
    period, computed on the host: (samples skipped, sample counter behind them, accumulated carrier phase in rad)."""
    off, counter, phase = C.c_int32(0), C.c_uint64(0), C.c_double(0.0)
    _check(load_library().gc_glonass_loop_pull_in(C.byref(conf), C.byref(off), C.byref(counter), C.byref(phase)))
    return int(off.value), int(counter.value), float(phase.value)


class TrackingBatch:
    """gc_trk_batch: all channels of one GPU, many epochs per launch."""

    def __init__(self, ctx, n_channels, n_taps, max_code_length, high_dyn=False):
        self._ctx = ctx
        self.n_channels, self.n_taps = n_channels, n_taps
        self._sc16 = False
        self._h = _vp()
        _check(load_library().gc_trk_batch_create(ctx._h, n_channels, n_taps, max_code_length, int(high_dyn), C.byref(self._h)))

    def set_code(self, ch, code, shifts_chips):
        code = np.ascontiguousarray(code, np.float32)
        shifts = np.ascontiguousarray(shifts_chips, np.float32)
        assert shifts.size == self.n_taps
        _check(load_library().gc_trk_batch_set_code(self._h, ch, _f32p(code), code.size, _f32p(shifts)))

    def set_complex_codes(self, on=True):
        _check(load_library().gc_trk_batch_set_complex_codes(self._h, int(bool(on))))

    def set_code_complex(self, ch, code, shifts_chips):
        code = np.ascontiguousarray(code, np.complex64)
        shifts = np.ascontiguousarray(shifts_chips, np.float32)
        assert shifts.size == self.n_taps
        _check(load_library().gc_trk_batch_set_code_complex(self._h, ch, code.view(np.float32).ctypes.data_as(_fp), code.size, _f32p(shifts)))

    def set_16sc(self, on=True):
        _check(load_library().gc_trk_batch_set_16sc(self._h, int(bool(on))))
        self._sc16 = bool(on)

    def set_code_16sc(self, ch, code, shifts_chips):
        code = np.ascontiguousarray(code, np.int16)
        shifts = np.ascontiguousarray(shifts_chips, np.float32)
        assert shifts.size == self.n_taps and code.ndim == 2 and code.shape[1] == 2
        _check(load_library().gc_trk_batch_set_code_16sc(self._h, ch, code.ctypes.data_as(_i16p), code.shape[0], _f32p(shifts)))

    def set_shifts(self, ch, shifts_chips):
        shifts = np.ascontiguousarray(shifts_chips, np.float32)
        assert shifts.size == self.n_taps
        _check(load_library().gc_trk_batch_set_shifts(self._h, ch, _f32p(shifts)))

    def set_input_format(self, iq_format):
        _check(load_library().gc_trk_batch_set_input_format(self._h, int(iq_format)))

    def set_input_dev(self, ch, dev_ptr, n_samples):
        _check(load_library().gc_trk_batch_set_input_dev(self._h, ch, _vp(dev_ptr), int(n_samples)))

    def set_input_stream(self, ch, stream):
        _check(load_library().gc_trk_batch_set_input_stream(self._h, ch, stream._h))
        self._streams = getattr(self, "_streams", {})
        self._streams[ch] = stream  # keep the ring alive

    def set_read_floor(self, oldest_index_read):
        _check(load_library().gc_trk_batch_set_read_floor(self._h, int(oldest_index_read)))

    def set_nominal_length(self, n):
        _check(load_library().gc_trk_batch_set_nominal_length(self._h, int(n)))

    def set_slices(self, n):
        _check(load_library().gc_trk_batch_set_slices(self._h, int(n)))

    def run_dev(self, n_epochs, dev_params_ptr, dev_out_ptr, stream=None):
        _check(load_library().gc_trk_batch_run_dev(self._h, n_epochs, _vp(dev_params_ptr), _vp(dev_out_ptr), _vp(stream or 0)))

    def run(self, n_epochs, params):
        """params: structured array (EPOCH_DTYPE) of n_channels*n_epochs records, channel-major.
        Returns complex64 [n_channels, n_epochs, n_taps] (int16 [n_channels, n_epochs, n_taps, 2] in 16-bit mode)."""
        params = np.ascontiguousarray(params, EPOCH_DTYPE)
        assert params.size == self.n_channels * n_epochs
        if self._sc16:
            out = np.zeros((self.n_channels, n_epochs, self.n_taps, 2), np.int16)
            _check(load_library().gc_trk_batch_run(self._h, n_epochs, params.ctypes.data_as(_vp), C.cast(out.ctypes.data, _fp)))
            return out
        out = np.zeros((self.n_channels, n_epochs, self.n_taps), np.complex64)
        _check(load_library().gc_trk_batch_run(self._h, n_epochs, params.ctypes.data_as(_vp), out.view(np.float32).ctypes.data_as(_fp)))
        return out

    def close(self):
        if self._h:
            load_library().gc_trk_batch_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackingLoop:
    """gc_trk_loop: closed-loop DLL/PLL tracking on the device (correlations + loop maths per epoch in one launch)."""

    def __init__(self, ctx, n_channels, max_code_length, mixed=False):
        self._ctx = ctx
        self.n_channels = n_channels
        self._h = _vp()
        _check(load_library().gc_trk_loop_create(ctx._h, n_channels, max_code_length, C.byref(self._h)))
        if mixed:
            try:
                self.set_mixed(True)
            except BaseException:
                self.close()
                raise

    def set_mixed(self, on=True):
        """Mixed mode (gc_trk_loop_set_mixed): each channel its own tap count, pilot mode, code length and period, all in
        one launch.  Only while no channel is started."""
        _check(load_library().gc_trk_loop_set_mixed(self._h, 1 if on else 0))

    def set_input_dev(self, ch, dev_ptr, n_samples):
        _check(load_library().gc_trk_loop_set_input_dev(self._h, ch, _vp(dev_ptr), int(n_samples)))

    def set_input_format(self, iq_format):
        _check(load_library().gc_trk_loop_set_input_format(self._h, int(iq_format)))

    def set_input_stream(self, ch, stream):
        _check(load_library().gc_trk_loop_set_input_stream(self._h, ch, stream._h))

    def set_sync(self, ch, sync, data_code=None):
        """Installs (or, with sync=None, removes) the LoopSyncConf of a channel; data_code is the data component's
        replica for pilot tracking.  Takes effect at the next start()."""
        if sync is None:
            _check(load_library().gc_trk_loop_set_sync(self._h, ch, None, None, 0))
            return
        if data_code is None:
            _check(load_library().gc_trk_loop_set_sync(self._h, ch, C.byref(sync), None, 0))
        else:
            data_code = np.ascontiguousarray(data_code, np.float32)
            _check(load_library().gc_trk_loop_set_sync(self._h, ch, C.byref(sync), _f32p(data_code), data_code.size))

    def start(self, ch, conf, code):
        code = np.ascontiguousarray(code, np.float32)
        _check(load_library().gc_trk_loop_start(self._h, ch, C.byref(conf), _f32p(code), code.size))

    def start_glonass(self, ch, conf):
        """gc_trk_loop_start_glonass: channel `ch` runs the GLONASS L1 / L2 C/A block's own loop (conf: GlonassLoopConf); the
        library generates the 511-chip replica.  The running channels of an engine are all of one kind."""
        _check(load_library().gc_trk_loop_start_glonass(self._h, ch, C.byref(conf)))

    def stop(self, ch):
        _check(load_library().gc_trk_loop_stop(self._h, ch))

    def set_geometry(self, threads_per_workgroup=0, slices_per_channel=0):
        """0 = automatic.  threads: 256 / 512 / 1024 (persistent kernel); slices: workgroups per channel-period (1: persistent
        one-workgroup-per-channel kernel; >= 2: one launch per code period, the last slice runs the loop maths)."""
        _check(load_library().gc_trk_loop_set_geometry(self._h, int(threads_per_workgroup), int(slices_per_channel)))

    def run(self, n_epochs):
        """Returns a structured array [n_channels, n_epochs] of LOOP_RECORD_DTYPE."""
        out = np.zeros((self.n_channels, n_epochs), LOOP_RECORD_DTYPE)
        _check(load_library().gc_trk_loop_run(self._h, n_epochs, out.ctypes.data_as(_vp)))
        return out

    def run_dev(self, n_epochs, dev_records_ptr, stream=None):
        _check(load_library().gc_trk_loop_run_dev(self._h, n_epochs, _vp(dev_records_ptr), _vp(stream or 0)))

    def close(self):
        if self._h:
            load_library().gc_trk_loop_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PcpsAcquisition:
    """gc_acq: pcps_acquisition (pcps_acquisition.cc) for n_sats satellites that
    search the same input block.  combine = "max" / "sum": a paired engine (gc_acq_create_paired) whose slots hold two
    replicas each (set_local_code_pair) and whose grid cells hold max(a, b) / a + b of the two |.|^2.
    folding_factor = f: the QuickSync engine (gc_acq_create_quicksync, pcps_quicksync_acquisition_cc.cc): fft_size is
    samples_per_code // f, a dwell consumes f * samples_per_code samples, set_local_code takes one code period, candidates(sat)
    gives the f aliased delays and their time-domain correlations.  It excludes `combine`.
    tong = (init, max, max_dwells): the Tong engine (gc_acq_create_tong, pcps_tong_acquisition_cc.cc): every dwell adds its
    power-normalised |.|^2 to the grid and is decided on the device; set_threshold, tong_search_stream and tong_status drive it.  It
    excludes `combine` and `folding_factor`.
    caf = dict(both_components=, hypotheses=, window_hz=, arithmetic="reference" | "exact"): the CAF engine (gc_acq_create_caf,
    galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc): up to four replicas per slot (set_local_code_iq), the stronger sign hypothesis
    of each component chosen per Doppler bin on the device, the CAF Doppler filter; caf_vectors(sat) reads CAF, CAF_I, CAF_Q and the
    choice bytes.  It excludes `combine`, `folding_factor` and `tong`."""

    COMBINE = {"max": 1, "sum": 2}
    CAF_ARITHMETIC = {"reference": CAF_REFERENCE, "exact": CAF_EXACT}

    def __init__(self, ctx, n_sats, fs_in, sampled_ms, ms_per_code, samples_per_ms, samples_per_code, samples_per_chip,
            doppler_max, doppler_step, max_dwells=1, bit_transition_flag=False, use_cfar=True, num_doppler_bins_override=0,
            make_2_steps=False, num_doppler_bins_step2=4, doppler_step2=125.0, combine=None, folding_factor=None, tong=None, caf=None):
        if folding_factor is not None and combine is not None:
            raise ValueError("folding_factor (the QuickSync engine) excludes combine (the paired engine)")
        if tong is not None and (combine is not None or folding_factor is not None):
            raise ValueError("tong (the Tong engine) excludes combine and folding_factor")
        if caf is not None and (combine is not None or folding_factor is not None or tong is not None):
            raise ValueError("caf (the CAF engine) excludes combine, folding_factor and tong")
        self.caf = None if caf is None else dict(caf)
        self.tong = None if tong is None else tuple(int(v) for v in tong)
        self._ctx = ctx
        self.n_sats = n_sats
        self.combine = combine
        self.folding_factor = folding_factor
        conf = AcqConf(int(fs_in), sampled_ms, ms_per_code, samples_per_ms, samples_per_code, samples_per_chip,
            doppler_max, doppler_step, max_dwells, int(bit_transition_flag), int(use_cfar), num_doppler_bins_override,
            int(make_2_steps), num_doppler_bins_step2, doppler_step2)
        self.conf = conf
        self._h = _vp()
        if self.caf is not None:
            unknown = set(self.caf) - {"both_components", "hypotheses", "window_hz", "arithmetic"}
            if unknown:
                raise ValueError("caf: unknown keys %s" % sorted(unknown))
            window = int(self.caf.get("window_hz", 0))
            if not 0 <= window < 2 ** 32:
                raise GnsscorrError(GC_ERR_INVALID, "caf window_hz %r out of range" % (window,))
            # an unknown name reaches the library as an unknown arithmetic: GC_ERR_INVALID
            _check(load_library().gc_acq_create_caf(ctx._h if ctx is not None else None, C.byref(conf), n_sats, int(self.caf.get("both_components", 0)),
                int(self.caf.get("hypotheses", 1)), window, self.CAF_ARITHMETIC.get(self.caf.get("arithmetic", "reference"), -1), C.byref(self._h)))
        elif self.tong is not None:
            if len(self.tong) != 3 or not all(0 <= v < 2 ** 32 for v in self.tong):
                raise GnsscorrError(GC_ERR_INVALID, "tong = (init, max, max_dwells), got %r" % (tong,))
            _check(load_library().gc_acq_create_tong(ctx._h, C.byref(conf), n_sats, self.tong[0], self.tong[1], self.tong[2], C.byref(self._h)))
        elif folding_factor is not None:
            if not 0 <= int(folding_factor) < 2 ** 32:
                raise GnsscorrError(GC_ERR_INVALID, "folding factor %r out of range" % (folding_factor,))
            _check(load_library().gc_acq_create_quicksync(ctx._h, C.byref(conf), n_sats, int(folding_factor), C.byref(self._h)))
        elif combine is None:
            _check(load_library().gc_acq_create(ctx._h, C.byref(conf), n_sats, C.byref(self._h)))
        else:
            # an unknown name reaches the library as an unknown combiner: GC_ERR_INVALID
            _check(load_library().gc_acq_create_paired(ctx._h, C.byref(conf), n_sats, self.COMBINE.get(combine, 0), C.byref(self._h)))
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load_library().gc_acq_fft_size(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.fft_size, self.consumed_samples, self.num_doppler_bins = a.value, b.value, c.value

    def set_local_code(self, sat, code):
        code = np.ascontiguousarray(code, np.complex64)
        need = self.fft_size // 2 if self.conf.bit_transition_flag else self.consumed_samples
        if self.folding_factor is not None:
            need = int(self.conf.samples_per_code)  # one code period, folded by the engine
        assert code.size >= need, (code.size, need)
        _check(load_library().gc_acq_set_local_code(self._h, sat, code.view(np.float32).ctypes.data_as(_fp)))

    def set_local_code_pair(self, sat, code_a, code_b):
        code_a = np.ascontiguousarray(code_a, np.complex64)
        code_b = np.ascontiguousarray(code_b, np.complex64)
        need = self.fft_size // 2 if self.conf.bit_transition_flag else self.consumed_samples
        assert code_a.size >= need and code_b.size >= need, (code_a.size, code_b.size, need)
        _check(load_library().gc_acq_set_local_code_pair(self._h, sat, _c64p(code_a), _c64p(code_b)))

    def set_local_code_iq(self, sat, code_i, code_q=None):
        """gc_acq_set_local_code_iq (CAF engine): fft_size complex samples per component; the library derives the B replicas."""
        code_i = np.ascontiguousarray(code_i, np.complex64)
        assert code_i.size >= self.fft_size, (code_i.size, self.fft_size)
        if code_q is not None:
            code_q = np.ascontiguousarray(code_q, np.complex64)
            assert code_q.size >= self.fft_size, (code_q.size, self.fft_size)
        _check(load_library().gc_acq_set_local_code_iq(self._h, sat, _c64p(code_i), None if code_q is None else _c64p(code_q)))

    def caf_vectors(self, sat):
        """gc_acq_caf_vectors: (CAF, CAF_I, CAF_Q float32[num_doppler_bins], choice uint8[num_doppler_bins]) of the last dwell."""
        n = self.num_doppler_bins
        caf, caf_i, caf_q, choice = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        _check(load_library().gc_acq_caf_vectors(self._h, sat, _f32p(caf), _f32p(caf_i), _f32p(caf_q), choice.ctypes.data_as(C.POINTER(C.c_uint8))))
        return caf, caf_i, caf_q, choice

    def reset(self):
        _check(load_library().gc_acq_reset(self._h))

    def set_step_two(self, enable, doppler_center_hz=0.0):
        _check(load_library().gc_acq_set_step_two(self._h, int(enable), float(doppler_center_hz)))
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load_library().gc_acq_fft_size(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.num_doppler_bins = c.value

    def dwell(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        assert iq.size >= self.consumed_samples
        res = (AcqResult * self.n_sats)()
        _check(load_library().gc_acq_dwell(self._h, iq.view(np.float32).ctypes.data_as(_fp), res))
        return list(res)

    def set_frequency_offset(self, offset_hz):
        _check(load_library().gc_acq_set_frequency_offset(self._h, int(offset_hz)))

    def dwell_stream(self, stream, first_index):
        res = (AcqResult * self.n_sats)()
        _check(load_library().gc_acq_dwell_stream(self._h, stream._h, int(first_index), C.cast(res, _vp)))
        return list(res)

    def set_input_format(self, iq_format):
        _check(load_library().gc_acq_set_input_format(self._h, int(iq_format)))

    def dwell_dev(self, dev_ptr, stream=None):
        res = (AcqResult * self.n_sats)()
        _check(load_library().gc_acq_dwell_dev(self._h, _vp(dev_ptr), res, _vp(stream or 0)))
        return list(res)

    def dwell_enqueue(self, dev_ptr, stream=None):
        _check(load_library().gc_acq_dwell_enqueue(self._h, _vp(dev_ptr), _vp(stream or 0)))

    def flush(self, stream=None):
        """Enqueues held-back inverse passes and the last dwell's statistics kernel; no copy, no synchronisation."""
        _check(load_library().gc_acq_flush(self._h, _vp(stream or 0)))

    def fetch_results(self, stream=None):
        res = (AcqResult * self.n_sats)()
        _check(load_library().gc_acq_fetch_results(self._h, res, _vp(stream or 0)))
        return list(res)

    def grid(self, sat):
        g = np.zeros((self.num_doppler_bins, self.fft_size), np.float32)
        _check(load_library().gc_acq_get_grid(self._h, sat, _f32p(g)))
        return g

    def set_threshold(self, threshold):
        """gc_acq_tong_set_threshold (Tong engine): used by the decisions of the dwells enqueued afterwards."""
        _check(load_library().gc_acq_tong_set_threshold(self._h, float(threshold)))

    def tong_status(self):
        """gc_acq_tong_status: a list of AcqTongStatus (state, tong_count, dwell_count), one per satellite."""
        st = (AcqTongStatus * self.n_sats)()
        _check(load_library().gc_acq_tong_status(self._h, C.cast(st, _vp)))
        return list(st)

    def tong_search_stream(self, ring, first_index, max_new_dwells=None):
        """gc_acq_tong_search_stream: up to max_new_dwells (default: all that are left of tong_max_dwells) dwells on consecutive
        blocks of the ring, back to back, one fetch.  Returns (results, status)."""
        res = (AcqResult * self.n_sats)()
        st = (AcqTongStatus * self.n_sats)()
        n = 0xFFFFFFFF if max_new_dwells is None else int(max_new_dwells)
        _check(load_library().gc_acq_tong_search_stream(self._h, ring._h, int(first_index), n, C.cast(res, _vp), C.cast(st, _vp)))
        return list(res), list(st)

    def candidates(self, sat):
        """gc_acq_quicksync_candidates: (possible_delay uint32[f], corr_output_f float32[f]) of the last dwell (QuickSync engine)."""
        f = int(self.folding_factor or 0)
        delay, val = np.zeros(max(f, 1), np.uint32), np.zeros(max(f, 1), np.float32)
        _check(load_library().gc_acq_quicksync_candidates(self._h, sat, delay.ctypes.data_as(C.POINTER(C.c_uint32)), _f32p(val)))
        return delay[:f], val[:f]

    PEEK_WIPEOFF, PEEK_SPECTRUM, PEEK_CODE, PEEK_ROW_MAX = 0, 1, 2, 3

    def peek(self, what, index):
        """gc_acq_peek: a device-resident intermediate in natural order (complex64[fft_size], or float32[num_doppler_bins, 2]
        = (row maximum, its index) for PEEK_ROW_MAX).  PEEK_CODE on a paired engine: index = 2 * sat + replica; on a CAF engine
        index = R * sat + replica."""
        if what == self.PEEK_ROW_MAX:
            out = np.zeros((self.num_doppler_bins, 2), np.float32)
        elif what == self.PEEK_WIPEOFF and self.folding_factor is not None:
            out = np.zeros(2 * self.consumed_samples, np.float32)  # the QuickSync table holds f code periods per bin
        else:
            out = np.zeros(2 * self.fft_size, np.float32)
        _check(load_library().gc_acq_peek(self._h, int(what), int(index), _f32p(out)))
        return out if what == self.PEEK_ROW_MAX else out.view(np.complex64)

    def close(self):
        if self._h:
            load_library().gc_acq_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FineDoppler:
    """gc_fine_doppler: the fine Doppler stage of pcps_acquisition_fine_doppler_cc -- the Doppler of acquired satellites to
    fs_in / (prn_replicas * zero_padding_factor * samples_per_code) from prn_replicas code periods, the code-wiped spectrum evaluated at
    the bins within window_hz of each coarse value only.  alignment: "reference" (the block's std::rotate, one element short) or
    "exact".  A request is (slot, delay_samples, coarse_doppler_hz)."""
    ALIGNMENT = {"reference": FINE_ALIGN_REFERENCE, "exact": FINE_ALIGN_EXACT}

    def __init__(self, ctx, n_slots, fs_in, samples_per_code, prn_replicas=10, zero_padding_factor=8, window_hz=1000.0, alignment="reference"):
        self._h = _vp()
        self._ctx = ctx
        self.n_slots = int(n_slots)
        # an unknown name reaches the library as an unknown alignment: GC_ERR_INVALID
        self.conf = FineDopplerConf(int(fs_in), int(samples_per_code), int(prn_replicas), int(zero_padding_factor), float(window_hz),
            self.ALIGNMENT.get(alignment, -1))
        self.block_samples = int(samples_per_code) * int(prn_replicas)
        self.next_size = self.block_samples * int(zero_padding_factor)
        _check(load_library().gc_fine_doppler_create(ctx._h if ctx is not None else None, C.byref(self.conf), self.n_slots, C.byref(self._h)))
        self._last_bins = []

    def set_code(self, slot, code):
        code = np.ascontiguousarray(code, np.complex64)
        assert code.size == self.conf.samples_per_code, (code.size, self.conf.samples_per_code)
        _check(load_library().gc_fine_doppler_set_code(self._h, int(slot), _c64p(code)))

    @staticmethod
    def _requests(requests):
        req = (FineDopplerRequest * max(len(requests), 1))()
        for i, (slot, delay, coarse) in enumerate(requests):
            req[i] = FineDopplerRequest(int(slot), int(delay), float(coarse))
        return req

    def _done(self, res, n):
        out = list(res)[:n]
        self._last_bins = [r.window_bins for r in out]
        return out

    def estimate_stream(self, ring, first_index, requests):
        """gc_fine_doppler_estimate_stream: a list of FineDopplerResult, one per request."""
        req = self._requests(requests)
        res = (FineDopplerResult * max(len(requests), 1))()
        _check(load_library().gc_fine_doppler_estimate_stream(self._h, ring._h, int(first_index), C.cast(req, _vp), len(requests), C.cast(res, _vp)))
        return self._done(res, len(requests))

    def estimate(self, iq, requests):
        """gc_fine_doppler_estimate on block_samples complex64 samples in host memory."""
        iq = np.ascontiguousarray(iq, np.complex64)
        assert iq.size >= self.block_samples, (iq.size, self.block_samples)
        req = self._requests(requests)
        res = (FineDopplerResult * max(len(requests), 1))()
        _check(load_library().gc_fine_doppler_estimate(self._h, _c64p(iq), C.cast(req, _vp), len(requests), C.cast(res, _vp)))
        return self._done(res, len(requests))

    def spectrum(self, request_index):
        """gc_fine_doppler_spectrum: p over the window of a request of the last call, window_bins float32 in run order."""
        if not 0 <= request_index < len(self._last_bins):
            raise GnsscorrError(GC_ERR_INVALID, "request %d of %d in the last call" % (request_index, len(self._last_bins)))
        out = np.zeros(self._last_bins[request_index], np.float32)
        _check(load_library().gc_fine_doppler_spectrum(self._h, int(request_index), _f32p(out)))
        return out

    def close(self):
        if self._h:
            load_library().gc_fine_doppler_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
