"""ctypes binding of libp25fe.so (the C ABI of include/p25fe.h).

The library is the product: if it is missing or no gfx950 device is present every call
fails loudly -- there is no Python/NumPy compute fallback anywhere in this package.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libp25fe.so")
MAX_TAPS = 64
ABI_VERSION = 6
FMT_CF32, FMT_U8, FMT_S16 = 0, 1, 2
S16_SCALE = 2.0 ** -15                    # P25FE_S16_SCALE: an int16 v is the sample (float)v * 2^-15, exactly
MAX_POSITION = 1 << 62                   # P25FE_MAX_POSITION: abs0 / abs_bb0 from here on are P25FE_ERR_ARG
RS_MAX_L, RS_MAX_M, RS_MAX_T, RS_MAX_TABLE = 32, 1024, 1024, 4096   # P25FE_RS_MAX_*: limits of the rational resampler
TUNE_MAX_CH, TUNE_MAX_DEN = 256, 8192    # P25FE_TUNE_MAX_*: limits of the tuner
AFC_MIN_D, AFC_MAX_D, AFC_MAX_T, AFC_MAX_CH, AFC_MAX_SHIFT = 2, 64, 512, 256, 40   # P25FE_AFC_*: limits of the frequency measure

OK, ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_FORMAT, ERR_NOMEM, ERR_JIT, ERR_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7, -8
CLOCK_FIXED, CLOCK_TRACKING, CLOCK_TRACKING_RESLICE, CLOCK_CAUSAL_OK = 0, 1, 2, 0x100
SPECIALIZE_AUTO, SPECIALIZE_OFF, SPECIALIZE_REQUIRE, SPECIALIZE_FORCE = 0, -1, 1, 2
VARIANT_BUILTIN, VARIANT_SPECIALIZED, VARIANT_GENERIC = 0, 1, 2


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_channels", C.c_int32),
                ("n_decim_taps", C.c_int32), ("n_chan_taps", C.c_int32),
                ("decim_taps", C.c_float * MAX_TAPS), ("chan_taps", C.c_float * MAX_TAPS),
                ("symbol_clock", C.c_int32), ("specialize", C.c_int32),
                ("fm_deviation_hz", C.c_uint32), ("fm_sample_rate_hz", C.c_uint32), ("fm_gain", C.c_float),
                ("u8_scale", C.c_float), ("u8_offset", C.c_float), ("u8_lut_valid", C.c_int32), ("u8_lut", C.c_float * 256),
                ("decim_phase", C.c_int32), ("n_avg_taps", C.c_int32), ("avg_taps", C.c_float * MAX_TAPS)]


class WindowsStats(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("ms_total", C.c_double), ("ms_h2d", C.c_double), ("ms_compute", C.c_double),
                ("pinned_input", C.c_int32), ("reserved", C.c_int32)]


class Anchor(C.Structure):
    _fields_ = [("s", C.c_int64), ("hi", C.c_float), ("mid", C.c_float), ("lo", C.c_float), ("valid", C.c_int32),
                ("period_d", C.c_int32), ("period_n", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("n_baseband", C.c_uint64), ("n_dibits", C.c_uint64), ("n_sync", C.c_uint64),
                ("anchor_out", Anchor), ("first_event", C.c_int64), ("n_dibits_after_first", C.c_uint64),
                ("carry_end", C.c_int64), ("first_seg_end", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


ANCHOR_DTYPE = np.dtype([("s", "<i8"), ("hi", "<f4"), ("mid", "<f4"), ("lo", "<f4"), ("valid", "<i4"),
                         ("period_d", "<i4"), ("period_n", "<i4")])
RESULT_DTYPE = np.dtype([("n_baseband", "<u8"), ("n_dibits", "<u8"), ("n_sync", "<u8"), ("anchor_out", ANCHOR_DTYPE),
                         ("first_event", "<i8"), ("n_dibits_after_first", "<u8"), ("carry_end", "<i8"),
                         ("first_seg_end", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])
NID_DTYPE = np.dtype([("raw", "<u8"), ("sync_pos", "<i8"), ("nac", "<u2"), ("duid", "u1"), ("n_errors", "u1"),
                      ("valid", "<i4")])
assert NID_DTYPE.itemsize == 24
CODE_STATS_DTYPE = np.dtype([("words", "<u8"), ("errs", "<u8"), ("fixed", "<u8"), ("size", "<u4"), ("reserved", "<u4")])
CHAN_STATS_DTYPE = np.dtype([("sig_power_dbm", "<f4"), ("locked", "<i4"), ("n_dibits", "<u8"), ("n_sync", "<u8"),
                             ("last_sync_pos", "<i8"), ("bch", CODE_STATS_DTYPE)])
assert CHAN_STATS_DTYPE.itemsize == 64
assert ANCHOR_DTYPE.itemsize == C.sizeof(Anchor) and RESULT_DTYPE.itemsize == C.sizeof(Result)
AFC_ACC_DTYPE = np.dtype([("re", "<i8"), ("im", "<i8"), ("pow", "<i8"), ("n", "<u8")])      # p25fe_afc_acc_t
assert AFC_ACC_DTYPE.itemsize == 32
TRACK_CFG_DTYPE = np.dtype([("shift", "<i4"), ("coh_min_q15", "<i4"), ("gain_q16", "<i4"), ("max_pull", "<i4"), ("max_dev", "<i4"),
                            ("reserved", "<i4"), ("min_products", "<u8")])                     # p25fe_track_cfg_t
TRACK_STATE_DTYPE = np.dtype([("step", "<i4"), ("ph0", "<u4"), ("last_theta", "<i4"), ("last_dstep", "<i4"), ("n_applied", "<u4"),
                              ("n_rejected", "<u4"), ("n_short", "<u4"), ("status", "<u4")])    # p25fe_track_state_t
assert TRACK_CFG_DTYPE.itemsize == 32 and TRACK_STATE_DTYPE.itemsize == 32
TRACK_NONE, TRACK_SHORT, TRACK_REJECT, TRACK_APPLY = 0, 1, 2, 3     # p25fe_track_state_t.status
SCAN_MAX_SHIFT = 40                                                 # P25FE_SCAN_MAX_SHIFT
SCAN_CHAN_DTYPE = np.dtype([("raster_index", "<i4"), ("reserved", "<i4"), ("centre_hz", "<f8"), ("db_over_floor", "<f8"),
                            ("offset_hz", "<f8")])                                             # p25fe_scan_chan_t
assert SCAN_CHAN_DTYPE.itemsize == 32
WATERFALL_KEY_DTYPE = np.dtype([("raster_index", "<i4"), ("reserved", "<i4"), ("first_slot", "<u8"), ("n_slots", "<u8"),
                                ("centre_hz", "<f8"), ("offset_hz", "<f8"), ("peak_db_over_floor", "<f8")])   # p25fe_waterfall_key_t
assert WATERFALL_KEY_DTYPE.itemsize == 48
CUT_DTYPE = np.dtype([("abs_first", "<u8"), ("n", "<u8"), ("step", "<i4"), ("ph0", "<u4")])   # p25fe_cut_t
assert CUT_DTYPE.itemsize == 24
CUTS_MAX = 4096
KEYS_MAX_CHANNELS = 4096                                            # P25FE_KEYS_MAX_CHANNELS

# every symbol include/p25fe.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "p25fe_default_config", "p25fe_create", "p25fe_destroy", "p25fe_strerror", "p25fe_last_hip_error", "p25fe_device",
    "p25fe_demod_u8", "p25fe_demod_cf32", "p25fe_slice", "p25fe_run_u8", "p25fe_run_cf32", "p25fe_resync",
    "p25fe_reset", "p25fe_state_size", "p25fe_state_export", "p25fe_state_import", "p25fe_demod_dev",
    "p25fe_slice_dev", "p25fe_run_dev", "p25fe_run_dev_pipelined", "p25fe_join_dev", "p25fe_shard_halo", "p25fe_shard_pass1", "p25fe_shard_pass2",
    "p25fe_shard_resolve", "p25fe_n_baseband", "p25fe_profile_enable", "p25fe_profile_read",
    "p25fe_predecim_dev", "p25fe_n_predecim", "p25fe_shard_resolve_dev", "p25fe_nid_dev",
    "p25fe_nid_batch_dev", "p25fe_chan_stats_dev", "p25fe_channelise_dev", "p25fe_nid",
    "p25fe_shard_pass1_main", "p25fe_shard_pass1_finish", "p25fe_shard_compact_dev", "p25fe_resync_at_dev",
    "p25fe_kernel_variant", "p25fe_specialize", "p25fe_specialize_log", "p25fe_run_host_windows",
    "p25fe_shard_pass1_head", "p25fe_shard_pipe_begin", "p25fe_shard_pipe_end", "p25fe_rx_stream", "p25fe_shard_head_check", "p25fe_shard_pass1_k1", "p25fe_streams_share_queue", "p25fe_shard_pass2_dev", "p25fe_shard_compact_from_dev", "p25fe_probe_variant", "p25fe_n_baseband_h",
    "p25fe_demod_s16", "p25fe_run_s16", "p25fe_format_variant", "p25fe_probe_format_variant",
    "p25fe_predecim_fmt_dev", "p25fe_channelise_fmt_dev",
    "p25fe_resampler_design", "p25fe_resampler_create", "p25fe_resampler_destroy", "p25fe_resampler_reset", "p25fe_n_resample",
    "p25fe_resample_dev", "p25fe_resample",
    "p25fe_tuner_freq", "p25fe_tuner_rotator", "p25fe_tuner_create", "p25fe_tuner_destroy", "p25fe_tuner_reset", "p25fe_tune_dev",
    "p25fe_tune",
    "p25fe_nco_step", "p25fe_nco_factor", "p25fe_nco_create",
    "p25fe_afc_set_step", "p25fe_afc_get_step", "p25fe_afc_factor", "p25fe_afc_design", "p25fe_afc_create", "p25fe_afc_destroy",
    "p25fe_afc_measure_dev", "p25fe_afc_hz",
    "p25fe_track_create", "p25fe_track_destroy", "p25fe_track_records", "p25fe_track_measure_dev", "p25fe_track_update_dev", "p25fe_track_run_dev",
    "p25fe_track_read", "p25fe_track_step", "p25fe_track_hz",
    "p25fe_scan_window", "p25fe_scan_create", "p25fe_scan_destroy", "p25fe_scan_reset", "p25fe_scan_dev", "p25fe_scan", "p25fe_scan_read",
    "p25fe_scan_channels",
    "p25fe_waterfall_slots", "p25fe_waterfall_dev", "p25fe_waterfall_open", "p25fe_waterfall", "p25fe_waterfall_read",
    "p25fe_waterfall_keys",
    "p25fe_cuts_from_keys", "p25fe_cuts_create", "p25fe_cuts_destroy", "p25fe_cuts_dev",
    "p25fe_keys_create", "p25fe_keys_destroy", "p25fe_keys_dev", "p25fe_keys_stream", "p25fe_keys_read",
    "p25fe_debug_planes_size", "p25fe_debug_planes_dev",
]


class P25feError(RuntimeError):
    def __init__(self, status, msg, hip=0):
        super().__init__("p25fe: %s (status %d%s)" % (msg, status, ", hipError %d" % hip if hip else ""))
        self.status = status
        self.hip = hip


_LIB = None


def load():
    """Load libp25fe.so.  Raises if it has not been built -- never substitutes another path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("libp25fe.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C p25rx_amd/csrc` (there is no CPU fallback)")
    # torch (plumbing: device memory, streams, RCCL) bundles its own libamdhip64.so.7.  Import it FIRST so
    # that libp25fe.so's NEEDED libamdhip64.so.7 binds to the runtime torch uses: two HIP runtimes in one
    # process do not share devices or pointers.  A host without torch binds to /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(os.environ.get("P25FE_LIB", LIB_PATH))      # P25FE_LIB: measurement builds (tools/ablate.sh) only
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    psz = C.POINTER(sz)
    L.p25fe_default_config.argtypes = [C.POINTER(Config)]
    L.p25fe_default_config.restype = None
    L.p25fe_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.p25fe_destroy.argtypes = [vp]
    L.p25fe_destroy.restype = None
    L.p25fe_strerror.argtypes = [C.c_int]
    L.p25fe_strerror.restype = C.c_char_p
    L.p25fe_last_hip_error.argtypes = [vp]
    L.p25fe_device.argtypes = [vp]
    L.p25fe_kernel_variant.argtypes = [vp]
    L.p25fe_specialize.argtypes = [C.POINTER(Config), C.c_char_p, C.c_char_p, sz]
    L.p25fe_probe_variant.argtypes = [C.POINTER(Config)]
    L.p25fe_format_variant.argtypes = [vp, C.c_int]
    L.p25fe_probe_format_variant.argtypes = [C.POINTER(Config), C.c_int]
    L.p25fe_specialize_log.argtypes = [C.c_char_p, sz]
    L.p25fe_specialize_log.restype = sz
    L.p25fe_demod_u8.argtypes = [vp, vp, sz, vp, sz, psz, vp]
    L.p25fe_demod_cf32.argtypes = [vp, vp, sz, vp, sz, psz, vp]
    L.p25fe_demod_s16.argtypes = [vp, vp, sz, vp, sz, psz, vp]
    L.p25fe_slice.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, sz, vp]
    L.p25fe_run_u8.argtypes = [vp, vp, sz, vp, sz, vp]
    L.p25fe_run_cf32.argtypes = [vp, vp, sz, vp, sz, vp]
    L.p25fe_run_s16.argtypes = [vp, vp, sz, vp, sz, vp]
    L.p25fe_run_host_windows.argtypes = [vp, vp, C.c_int, sz, sz, vp, sz, vp, C.POINTER(WindowsStats)]
    L.p25fe_resync.argtypes = [vp]
    L.p25fe_reset.argtypes = [vp]
    L.p25fe_state_size.argtypes = [vp, psz]
    L.p25fe_state_export.argtypes = [vp, vp, sz, psz]
    L.p25fe_state_import.argtypes = [vp, vp, sz]
    L.p25fe_demod_dev.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp, sz, vp, vp]
    L.p25fe_slice_dev.argtypes = [vp, vp, sz, sz, sz, u64, vp, vp, sz, vp, vp, sz, vp, vp]
    L.p25fe_run_dev.argtypes = [vp, vp, C.c_int, sz, sz, vp, sz, vp, vp]
    L.p25fe_run_dev_pipelined.argtypes = [vp, vp, C.c_int, sz, sz, vp, sz, vp, vp]
    L.p25fe_join_dev.argtypes = [vp, vp]
    L.p25fe_shard_halo.argtypes = []
    L.p25fe_shard_halo.restype = sz
    L.p25fe_shard_pass1.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp, vp]
    L.p25fe_shard_pass1_main.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp]
    L.p25fe_shard_pass1_finish.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp, vp]
    L.p25fe_shard_compact_dev.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    L.p25fe_shard_pass1_head.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp]
    L.p25fe_shard_pipe_begin.argtypes = [vp, vp, C.POINTER(C.c_void_p)]
    L.p25fe_shard_head_check.argtypes = [C.c_void_p]
    L.p25fe_rx_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.p25fe_shard_pipe_end.argtypes = [vp, vp]
    L.p25fe_debug_planes_size.argtypes = [vp, sz, psz, psz]
    L.p25fe_debug_planes_dev.argtypes = [vp, sz, vp, sz, vp, sz, vp]
    L.p25fe_shard_pass1_k1.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp]
    L.p25fe_streams_share_queue.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.p25fe_shard_pass2_dev.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.p25fe_shard_compact_from_dev.argtypes = [vp, vp, sz, vp, sz, sz, vp, sz, vp]
    L.p25fe_shard_pass2.argtypes = [vp, vp, vp, sz, vp, vp]
    L.p25fe_shard_resolve.argtypes = [vp, vp, vp, sz, C.c_int, vp, vp]
    L.p25fe_resync_at_dev.argtypes = [vp, vp, sz, sz]
    L.p25fe_shard_resolve_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp]
    L.p25fe_nid_dev.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp]
    L.p25fe_nid.argtypes = [vp, vp, sz, vp, vp, sz, vp]
    L.p25fe_nid_batch_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, vp]
    L.p25fe_chan_stats_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    L.p25fe_channelise_dev.argtypes = [vp, vp, sz, sz, u64, vp, sz, vp]
    L.p25fe_profile_enable.argtypes = [vp, C.c_int]
    L.p25fe_profile_read.argtypes = [vp, C.POINTER(C.c_double * 4), C.POINTER(u64)]
    L.p25fe_predecim_dev.argtypes = [vp, vp, sz, sz, sz, u64, vp, sz, vp]
    L.p25fe_predecim_fmt_dev.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp, sz, vp]
    L.p25fe_channelise_fmt_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, vp, sz, vp]
    pi32 = C.POINTER(C.c_int32)
    L.p25fe_resampler_design.argtypes = [C.c_uint32, pi32, pi32, pi32, vp, sz]
    L.p25fe_resampler_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.POINTER(vp)]
    L.p25fe_resampler_destroy.argtypes = [vp]
    L.p25fe_resampler_destroy.restype = None
    L.p25fe_resampler_reset.argtypes = [vp]
    L.p25fe_n_resample.argtypes = [C.c_int32, C.c_int32, u64, sz]
    L.p25fe_n_resample.restype = sz
    L.p25fe_resample_dev.argtypes = [vp, vp, C.c_int, sz, sz, sz, u64, vp, sz, vp]
    L.p25fe_resample.argtypes = [vp, vp, C.c_int, sz, vp, sz, psz]
    L.p25fe_tuner_freq.argtypes = [C.c_uint32, C.c_int64, pi32, pi32]
    L.p25fe_tuner_rotator.argtypes = [C.c_int32, vp, sz]
    L.p25fe_tuner_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, C.POINTER(vp)]
    L.p25fe_tuner_destroy.argtypes = [vp]
    L.p25fe_tuner_destroy.restype = None
    L.p25fe_tuner_reset.argtypes = [vp]
    L.p25fe_tune_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, vp, sz, vp]
    L.p25fe_tune.argtypes = [vp, vp, C.c_int, sz, vp, sz, psz]
    L.p25fe_nco_step.argtypes = [C.c_uint32, C.c_double, pi32]
    L.p25fe_nco_factor.argtypes = [C.c_int32, u64, vp]
    L.p25fe_nco_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.POINTER(vp)]
    L.p25fe_afc_set_step.argtypes = [vp, C.c_int32, C.c_int32, u64, vp]
    L.p25fe_afc_get_step.argtypes = [vp, C.c_int32, pi32, C.POINTER(C.c_uint32)]
    L.p25fe_afc_factor.argtypes = [C.c_int32, C.c_uint32, u64, vp]
    L.p25fe_afc_design.argtypes = [C.c_int32, C.c_double, C.c_int32, vp, sz]
    L.p25fe_afc_create.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, C.POINTER(vp)]
    L.p25fe_afc_destroy.argtypes = [vp]
    L.p25fe_afc_destroy.restype = None
    L.p25fe_afc_measure_dev.argtypes = [vp, vp, sz, sz, sz, u64, C.c_int32, vp, vp]
    L.p25fe_afc_hz.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.p25fe_track_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.p25fe_track_destroy.argtypes = [vp]
    L.p25fe_track_destroy.restype = None
    L.p25fe_track_records.argtypes = [vp, vp, vp]
    L.p25fe_track_measure_dev.argtypes = [vp, vp, sz, sz, sz, u64, vp]
    L.p25fe_track_update_dev.argtypes = [vp, u64, vp]
    L.p25fe_track_run_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, u64, vp, sz, sz, vp]
    L.p25fe_track_read.argtypes = [vp, vp]
    L.p25fe_track_step.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, u64, vp, vp]
    L.p25fe_track_hz.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    L.p25fe_scan_window.argtypes = [C.c_int32, vp, sz]
    L.p25fe_scan_create.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, C.POINTER(vp)]
    L.p25fe_scan_destroy.argtypes = [vp]
    L.p25fe_scan_destroy.restype = None
    L.p25fe_scan_reset.argtypes = [vp]
    L.p25fe_scan_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, vp, vp]
    L.p25fe_scan.argtypes = [vp, vp, C.c_int, sz]
    L.p25fe_scan_read.argtypes = [vp, vp, C.c_int]
    L.p25fe_scan_channels.argtypes = [vp, C.c_int32, C.c_uint32, C.c_double, C.c_double, C.c_double, vp, sz, psz]
    L.p25fe_waterfall_slots.argtypes = [C.c_int32, C.c_uint32, u64, sz, C.POINTER(u64), psz]
    L.p25fe_waterfall_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, C.c_uint32, u64, vp, sz, sz, vp]
    L.p25fe_waterfall_open.argtypes = [vp, C.c_uint32, sz]
    L.p25fe_waterfall.argtypes = [vp, vp, C.c_int, sz]
    L.p25fe_waterfall_read.argtypes = [vp, vp, sz, psz]
    L.p25fe_waterfall_keys.argtypes = [vp, sz, sz, C.c_int32, C.c_uint32, u64, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_uint32, vp, sz, psz]
    L.p25fe_cuts_from_keys.argtypes = [vp, sz, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, u64, u64, u64, vp, sz, psz]
    L.p25fe_cuts_create.argtypes = [vp, vp, sz, vp, psz, C.POINTER(vp)]
    L.p25fe_cuts_destroy.argtypes = [vp]
    L.p25fe_cuts_destroy.restype = None
    L.p25fe_cuts_dev.argtypes = [vp, vp, C.c_int, sz, sz, u64, vp, sz, vp]
    L.p25fe_keys_create.argtypes = [vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, sz, sz, C.POINTER(vp)]
    L.p25fe_keys_destroy.argtypes = [vp]
    L.p25fe_keys_destroy.restype = None
    L.p25fe_keys_dev.argtypes = [vp, vp, sz, sz, u64, vp]
    L.p25fe_keys_stream.argtypes = [vp]
    L.p25fe_keys_read.argtypes = [vp, vp, sz, psz]
    L.p25fe_n_predecim.argtypes = [u64, sz]
    L.p25fe_n_predecim.restype = sz
    L.p25fe_n_baseband.argtypes = [u64, sz]
    L.p25fe_n_baseband.restype = sz
    L.p25fe_n_baseband_h.argtypes = [vp, u64, sz]
    L.p25fe_n_baseband_h.restype = sz
    _LIB = L
    return L


def default_config():
    cfg = Config()
    load().p25fe_default_config(C.byref(cfg))
    return cfg


def specialize_log():
    buf = C.create_string_buffer(1 << 16)
    load().p25fe_specialize_log(buf, len(buf))
    return buf.value.decode(errors="replace")


def make_config(n_channels=1, device=0, decim_taps=None, chan_taps=None, symbol_clock=0, specialize=SPECIALIZE_AUTO,
                fm_deviation_hz=None, fm_sample_rate_hz=None, fm_gain=None, u8_scale=None, u8_offset=None, u8_lut=None,
                decim_phase=None, avg_taps=None):
    """p25fe_config_t from keyword arguments (None = the build's default)."""
    cfg = default_config()
    cfg.device, cfg.n_channels, cfg.symbol_clock, cfg.specialize = device, n_channels, symbol_clock, specialize
    if decim_taps is not None:
        cfg.n_decim_taps = len(decim_taps)                       # the library rejects counts above P25FE_MAX_TAPS
        for i, v in enumerate(decim_taps[:MAX_TAPS]):
            cfg.decim_taps[i] = v
    if chan_taps is not None:
        cfg.n_chan_taps = len(chan_taps)
        for i, v in enumerate(chan_taps[:MAX_TAPS]):
            cfg.chan_taps[i] = v
    if fm_deviation_hz is not None:
        cfg.fm_deviation_hz = int(fm_deviation_hz)
    if fm_sample_rate_hz is not None:
        cfg.fm_sample_rate_hz = int(fm_sample_rate_hz)
    if fm_gain is not None:
        cfg.fm_gain = float(fm_gain)
    if u8_scale is not None:
        cfg.u8_scale = float(u8_scale)
    if u8_offset is not None:
        cfg.u8_offset = float(u8_offset)
    if u8_lut is not None:
        lut = np.asarray(u8_lut, dtype=np.float32)
        assert lut.shape == (256,)
        cfg.u8_lut_valid = 1
        for i in range(256):
            cfg.u8_lut[i] = lut[i]
    if decim_phase is not None:
        cfg.decim_phase = int(decim_phase)
    if avg_taps is not None:
        cfg.n_avg_taps = len(avg_taps)                           # the library rejects counts above P25FE_MAX_TAPS
        for i, v in enumerate(list(avg_taps)[:MAX_TAPS]):
            cfg.avg_taps[i] = v
    return cfg


def specialize(cfg, directory=None):
    """p25fe_specialize: compile (no GPU needed) and store the kernels for cfg's numbers; returns the file name ('' for the
    build's own numbers)."""
    L = load()
    out = C.create_string_buffer(4096)
    rc = L.p25fe_specialize(C.byref(cfg), directory.encode() if directory else None, out, len(out))
    if rc != OK:
        raise P25feError(rc, L.p25fe_strerror(rc).decode() + ": " + specialize_log()[-2000:])
    return out.value.decode()


def probe_variant(cfg):
    """p25fe_probe_variant: the kernels a handle made from cfg would run on this host (VARIANT_*); no GPU needed"""
    L = load()
    rc = L.p25fe_probe_variant(C.byref(cfg))
    if rc < 0:
        raise P25feError(rc, L.p25fe_strerror(rc).decode() + ": " + specialize_log()[-2000:])
    return rc


def probe_format_variant(cfg, fmt):
    """p25fe_probe_format_variant: the kernels input format `fmt` would run on a handle made from cfg (VARIANT_*); no GPU needed"""
    L = load()
    rc = L.p25fe_probe_format_variant(C.byref(cfg), int(fmt))
    if rc < 0:
        raise P25feError(rc, L.p25fe_strerror(rc).decode())
    return rc


def check(L, h, rc):
    if rc != OK:
        hip = L.p25fe_last_hip_error(h) if (h and rc == ERR_HIP) else 0
        raise P25feError(rc, L.p25fe_strerror(rc).decode(), hip)
