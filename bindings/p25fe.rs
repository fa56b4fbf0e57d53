//! bindings/p25fe.rs -- Rust side of the C ABI of `include/p25fe.h` / `include/p25fe_rccl.h` (ABI version 6).
//!
//! NOT COMPILED IN THIS REPOSITORY: the build image has no Rust toolchain.  This is the file a
//! maintainer of kchmck/p25rx drops in as `src/p25fe.rs` (`mod p25fe;` in `src/main.rs:55-64`); the layouts below are the
//! `#[repr(C)]` twins of the C structs, and `p25rx_amd/_lib.py` holds the same layouts as ctypes / NumPy types whose sizes
//! the tests assert.  The tested host code of this repository is the C++ mirror (`p25rx_amd/host/p25fe_host.hpp`) and the
//! Python one (`p25rx_amd/demod.py`, `recv.py`), which have the shape of `DemodTask` / `RecvTask` below.
//!
//! What it replaces in the reference (file:line in kchmck/p25rx):
//!   * `DemodTask::new`  src/demod.rs:44-59   -> `FrontEnd::new` (tables, FM deviation / rate, the u8 table: all run-time)
//!   * `DemodTask::run`  src/demod.rs:62-119  -> `DemodTask::run` below: one `p25fe_demod_u8` per buffer
//!   * `RecvTask::run` sample loop  src/recv.rs:148-150, 204-210 -> `FrontEnd::slice` (or keep `MessageReceiver::feed`)
//!   * `MessageReceiver::resync`    src/recv.rs:136, 179         -> `FrontEnd::resync`
#![allow(dead_code, non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const ABI_VERSION: i32 = 6;
/// P25FE_MAX_POSITION: an abs0 / abs_bb0 (or a state blob's counter) from here on is P25FE_ERR_ARG
pub const MAX_POSITION: u64 = 1 << 62;
pub const MAX_TAPS: usize = 64;
pub const FMT_CF32: c_int = 0;
pub const FMT_U8: c_int = 1;
pub const FMT_S16: c_int = 2;
/// P25FE_S16_SCALE: an int16 v of an FMT_S16 stream is the sample v as f32 * 2^-15, exactly
pub const S16_SCALE: f32 = 1.0 / 32768.0;
pub const CLOCK_FIXED: i32 = 0;
pub const CLOCK_TRACKING: i32 = 1;
/// CLOCK_TRACKING, and the calls that hold a whole range (run_dev, run_dev_pipelined, slice_dev) re-slice the first frame of a lock
/// run with the period the next sync word confirms (docs/SPEC.md 3.8c).  The calls that see the stream in pieces (slice, run_u8 / run_cf32,
/// run_host_windows, the time-shard passes) cannot: on such a handle they return ERR_ARG (ABI 6) unless CLOCK_CAUSAL_OK was or-ed into
/// `symbol_clock`, which lets them run CLOCK_TRACKING's causal rule instead
pub const CLOCK_TRACKING_RESLICE: i32 = 2;
pub const CLOCK_CAUSAL_OK: i32 = 0x100;
/// a device-side wait gave up (p25fe_shard_head_check: the head segment of a time shard never arrived)
pub const ERR_TIMEOUT: c_int = -8;
pub const SPECIALIZE_AUTO: i32 = 0;
pub const SPECIALIZE_OFF: i32 = -1;
pub const SPECIALIZE_REQUIRE: i32 = 1;
pub const SPECIALIZE_FORCE: i32 = 2;
pub const VARIANT_BUILTIN: c_int = 0;
pub const VARIANT_SPECIALIZED: c_int = 1;
pub const VARIANT_GENERIC: c_int = 2;
pub const GATHER_NONE: c_int = 0;
pub const GATHER_ROOT: c_int = 1;
pub const GATHER_ALL: c_int = 2;
pub const GATHER_ROOT_EXACT: c_int = 3;

/// p25fe_config_t
#[repr(C)]
#[derive(Clone, Copy)]
pub struct Config {
    pub abi_version: i32,
    pub device: i32,
    pub n_channels: i32,
    pub n_decim_taps: i32,
    pub n_chan_taps: i32,
    pub decim_taps: [f32; MAX_TAPS],   // p25_filts::DecimFir, src/demod.rs:27: tap 0 multiplies the newest sample
    pub chan_taps: [f32; MAX_TAPS],    // p25_filts::BandpassFir, src/demod.rs:29
    pub symbol_clock: i32,
    pub specialize: i32,
    pub fm_deviation_hz: u32,          // FmDemod::new(5000, BASEBAND_SAMPLE_RATE), src/demod.rs:54
    pub fm_sample_rate_hz: u32,
    pub fm_gain: f32,                  // 0: derived from the two above
    pub u8_scale: f32,                 // rtlsdr_iq::IQ as fma(b, scale, offset), src/demod.rs:83 ...
    pub u8_offset: f32,
    pub u8_lut_valid: i32,             // ... or as the table itself
    pub u8_lut: [f32; 256],
    pub decim_phase: i32,              // Decimator::new(5), src/demod.rs:50, 87-90: output m comes from input 5 m + decim_phase (4)
    pub n_avg_taps: i32,               // MovingAverage::new(10), src/demod.rs:52, 114, as a table (ten equal taps of 0.1)
    pub avg_taps: [f32; MAX_TAPS],
}

/// p25fe_anchor_t
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct Anchor {
    pub s: i64,
    pub hi: f32,
    pub mid: f32,
    pub lo: f32,
    pub valid: i32,                    // test `!= 0`; hand on unchanged (upper bits: docs/SPEC.md 3.8b)
    pub period_d: i32,
    pub period_n: i32,
}

/// p25fe_result_t
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ResultRec {
    pub n_baseband: u64,
    pub n_dibits: u64,
    pub n_sync: u64,
    pub anchor_out: Anchor,
    pub first_event: i64,
    pub n_dibits_after_first: u64,
    pub carry_end: i64,
    pub first_seg_end: i64,
    pub flags: u32,
    pub reserved: u32,
}

/// p25fe_nid_t
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct Nid {
    pub raw: u64,
    pub sync_pos: i64,
    pub nac: u16,
    pub duid: u8,
    pub n_errors: u8,
    pub valid: i32,
}

/// p25fe_code_stats_t / p25fe_chan_stats_t
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct CodeStats {
    pub words: u64,
    pub errs: u64,
    pub fixed: u64,
    pub size: u32,
    pub reserved: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ChanStats {
    pub sig_power_dbm: f32,
    pub locked: i32,
    pub n_dibits: u64,
    pub n_sync: u64,
    pub last_sync_pos: i64,
    pub bch: CodeStats,
}

/// p25fe_windows_stats_t
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct WindowsStats {
    pub n_windows: u64,
    pub ms_total: f64,
    pub ms_h2d: f64,
    pub ms_compute: f64,
    pub pinned_input: i32,
    pub reserved: i32,
}

pub enum Handle {}
/// p25fe_resampler_t: the rational resampler of docs/SPEC.md 3.0b (made from a Handle, which must outlive it)
pub enum Resampler {}
/// P25FE_RS_MAX_L / _M / _T / _TABLE: L <= 32, L < M <= 1024, T <= 1024, L * T <= 4096, gcd(L, M) = 1
pub const RS_MAX_L: i32 = 32;
pub const RS_MAX_M: i32 = 1024;
pub const RS_MAX_T: i32 = 1024;
pub const RS_MAX_TABLE: i32 = 4096;
/// p25fe_tuner_t: the tuner of docs/SPEC.md 3.0c (rational channels) or 3.0d (NCO channels), made from a Handle, which must outlive it
pub enum Tuner {}
/// p25fe_afc_t: the frequency measure of docs/SPEC.md 3.0f (made from a Handle, which must outlive it)
pub enum Afc {}
/// p25fe_track_t: the AFC loop of docs/SPEC.md 3.0g (made from a Tuner of NCO channels and an Afc, which must outlive it)
pub enum Track {}
pub const TRACK_NONE: u32 = 0;
pub const TRACK_SHORT: u32 = 1;
pub const TRACK_REJECT: u32 = 2;
pub const TRACK_APPLY: u32 = 3;
/// p25fe_track_cfg_t: the loop's configuration, 32 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct TrackCfg {
    pub shift: i32,
    pub coh_min_q15: i32,
    pub gain_q16: i32,
    pub max_pull: i32,
    pub max_dev: i32,
    pub reserved: i32,
    pub min_products: u64,
}
/// p25fe_track_state_t: one channel's state, 32 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct TrackState {
    pub step: i32,
    pub ph0: u32,
    pub last_theta: i32,
    pub last_dstep: i32,
    pub n_applied: u32,
    pub n_rejected: u32,
    pub n_short: u32,
    pub status: u32,
}
/// p25fe_afc_acc_t: one row's sums, 32 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct AfcAcc {
    pub re: i64,
    pub im: i64,
    pub pow: i64,
    pub n: u64,
}
/// P25FE_AFC_*: 2 <= D <= 64, 1 <= T <= 512, 1 <= rows <= 256, 0 <= shift <= 40
pub const AFC_MIN_D: i32 = 2;
pub const AFC_MAX_D: i32 = 64;
pub const AFC_MAX_T: i32 = 512;
pub const AFC_MAX_CH: i32 = 256;
pub const AFC_MAX_SHIFT: i32 = 40;
/// p25fe_scan_t: the survey of docs/SPEC.md 3.0h (made for a Handle, which must outlive every use of it)
pub enum Scan {}
/// P25FE_SCAN_MAX_SHIFT: 0 <= shift <= 40; N is 1024 or 4096, hop a multiple of 8 that divides N
pub const SCAN_MAX_SHIFT: i32 = 40;
/// p25fe_scan_chan_t: one active raster channel of a survey's record (32 bytes)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ScanChan {
    pub raster_index: i32,
    pub reserved: i32,
    pub centre_hz: f64,
    pub db_over_floor: f64,
    pub offset_hz: f64,
}
/// p25fe_waterfall_key_t: one keyed interval of a survey over time, docs/SPEC.md 3.0i (48 bytes)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct WaterfallKey {
    pub raster_index: i32,
    pub reserved: i32,
    pub first_slot: u64,
    pub n_slots: u64,
    pub centre_hz: f64,
    pub offset_hz: f64,
    pub peak_db_over_floor: f64,
}
/// p25fe_cut_t: one cut of a capture, docs/SPEC.md 3.0j (24 bytes)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct Cut {
    pub abs_first: u64,
    pub n: u64,
    pub step: i32,
    pub ph0: u32,
}
pub const CUTS_MAX: usize = 4096;
pub enum Cuts {}
/// p25fe_keys_t: the keyed intervals of docs/SPEC.md 3.0k computed on the device (made from a Scan, which must outlive it)
pub enum Keys {}
/// P25FE_KEYS_MAX_CHANNELS: the eligible raster channels a Keys object admits
pub const KEYS_MAX_CHANNELS: usize = 4096;
/// P25FE_TUNE_MAX_CH / _DEN: 1 <= channels <= 256; num / den in lowest terms, 1 <= den <= 8192, 2 |num| <= den
pub const TUNE_MAX_CH: i32 = 256;
pub const TUNE_MAX_DEN: i32 = 8192;
pub enum Shard {}

#[link(name = "p25fe")]
extern "C" {
    pub fn p25fe_default_config(cfg: *mut Config);
    pub fn p25fe_create(cfg: *const Config, out: *mut *mut Handle) -> c_int;
    pub fn p25fe_destroy(h: *mut Handle);
    pub fn p25fe_strerror(status: c_int) -> *const c_char;
    pub fn p25fe_last_hip_error(h: *const Handle) -> c_int;
    pub fn p25fe_device(h: *const Handle) -> c_int;
    pub fn p25fe_kernel_variant(h: *const Handle) -> c_int;
    pub fn p25fe_specialize(cfg: *const Config, dir: *const c_char, path_out: *mut c_char, path_cap: usize) -> c_int;
    pub fn p25fe_probe_variant(cfg: *const Config) -> c_int;
    pub fn p25fe_format_variant(h: *const Handle, fmt: c_int) -> c_int;
    pub fn p25fe_probe_format_variant(cfg: *const Config, fmt: c_int) -> c_int;
    pub fn p25fe_specialize_log(buf: *mut c_char, cap: usize) -> usize;
    // streaming, host buffers: the bodies of DemodTask::run (src/demod.rs:70-117) and RecvTask::run (src/recv.rs:148-150)
    pub fn p25fe_demod_u8(h: *mut Handle, iq: *const u8, n_bytes: usize, bb: *mut f32, bb_cap: usize, n_out: *mut usize,
                          power_dbm: *mut f32) -> c_int;
    pub fn p25fe_demod_cf32(h: *mut Handle, iq: *const f32, n_samples: usize, bb: *mut f32, bb_cap: usize, n_out: *mut usize,
                            power_dbm: *mut f32) -> c_int;
    pub fn p25fe_slice(h: *mut Handle, bb: *const f32, n: usize, dibits: *mut u8, cap: usize, n_dibits: *mut usize,
                       sync_pos: *mut i64, sync_dibit: *mut u64, sync_cap: usize, n_sync: *mut usize) -> c_int;
    pub fn p25fe_run_u8(h: *mut Handle, iq: *const u8, n_bytes: usize, dibits: *mut u8, cap: usize, n_dibits: *mut usize) -> c_int;
    pub fn p25fe_run_cf32(h: *mut Handle, iq: *const f32, n_samples: usize, dibits: *mut u8, cap: usize, n_dibits: *mut usize) -> c_int;
    pub fn p25fe_run_s16(h: *mut Handle, iq: *const i16, n_samples: usize, dibits: *mut u8, cap: usize, n_dibits: *mut usize) -> c_int;
    pub fn p25fe_demod_s16(h: *mut Handle, iq: *const i16, n_samples: usize, bb: *mut f32, bb_cap: usize, n_out: *mut usize,
                           power_dbm: *mut f32) -> c_int;
    pub fn p25fe_run_host_windows(h: *mut Handle, iq: *const c_void, fmt: c_int, n: usize, window: usize, dibits: *mut u8,
                                  cap: usize, n_dibits: *mut usize, stats: *mut WindowsStats) -> c_int;
    pub fn p25fe_resync(h: *mut Handle) -> c_int;
    pub fn p25fe_resync_at_dev(h: *mut Handle, d_idx: *const i64, n_idx: usize, idx_stride: usize) -> c_int;
    pub fn p25fe_reset(h: *mut Handle) -> c_int;
    pub fn p25fe_state_size(h: *const Handle, n: *mut usize) -> c_int;
    pub fn p25fe_state_export(h: *const Handle, buf: *mut c_void, cap: usize, n: *mut usize) -> c_int;
    pub fn p25fe_state_import(h: *mut Handle, buf: *const c_void, n: usize) -> c_int;
    // device-resident ranges (all pointers device pointers; stream = hipStream_t or null)
    pub fn p25fe_demod_dev(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize, abs0: u64,
                           d_bb: *mut f32, bb_stride: usize, d_power_dbm: *mut f32, stream: *mut c_void) -> c_int;
    pub fn p25fe_predecim_dev(h: *mut Handle, d_iq: *const f32, ch_stride: usize, n_hist: usize, n: usize, abs0: u64,
                              d_out: *mut f32, out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_predecim_fmt_dev(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize, abs_first: u64,
                                  d_out: *mut f32, out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_n_predecim(abs0: u64, n: usize) -> usize;
    // rational resampler: any tuner rate -> 240 ksps (taps[j * L + p] = tap j of phase p)
    pub fn p25fe_resampler_design(fs_in_hz: u32, l: *mut i32, m: *mut i32, t: *mut i32, taps: *mut f32, cap: usize) -> c_int;
    pub fn p25fe_resampler_create(h: *mut Handle, l: i32, m: i32, t: i32, taps: *const f32, out: *mut *mut Resampler) -> c_int;
    pub fn p25fe_resampler_destroy(rs: *mut Resampler);
    pub fn p25fe_resampler_reset(rs: *mut Resampler) -> c_int;
    pub fn p25fe_n_resample(l: i32, m: i32, abs_first: u64, n: usize) -> usize;
    pub fn p25fe_resample_dev(rs: *mut Resampler, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize, abs_first: u64,
                              d_out: *mut f32, out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_resample(rs: *mut Resampler, iq: *const c_void, fmt: c_int, n: usize, out: *mut f32, cap: usize, n_out: *mut usize) -> c_int;
    // tuner: K channels at num / den cycles per input sample out of one capture (the resampler with a mixer in front)
    pub fn p25fe_tuner_freq(fs_in_hz: u32, offset_hz: i64, num: *mut i32, den: *mut i32) -> c_int;
    pub fn p25fe_tuner_rotator(den: i32, cs: *mut f32, cap: usize) -> c_int;
    pub fn p25fe_tuner_create(h: *mut Handle, l: i32, m: i32, t: i32, taps: *const f32, n_out_channels: i32, num: *const i32,
                              den: *const i32, out: *mut *mut Tuner) -> c_int;
    pub fn p25fe_tuner_destroy(tn: *mut Tuner);
    pub fn p25fe_tuner_reset(tn: *mut Tuner) -> c_int;
    pub fn p25fe_tune_dev(tn: *mut Tuner, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64, d_out: *mut f32,
                          out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_tune(tn: *mut Tuner, iq: *const c_void, fmt: c_int, n: usize, out: *mut f32, cap: usize, n_out: *mut usize) -> c_int;
    // tuner, NCO channels (docs/SPEC.md 3.0d): step / 2^32 cycles per input sample, any frequency offset; the object is a Tuner
    pub fn p25fe_nco_step(fs_in_hz: u32, offset_hz: f64, step: *mut i32) -> c_int;
    pub fn p25fe_nco_factor(step: i32, n: u64, cs: *mut f32) -> c_int;
    pub fn p25fe_nco_create(h: *mut Handle, l: i32, m: i32, t: i32, taps: *const f32, n_out_channels: i32, step: *const i32,
                                  out: *mut *mut Tuner) -> c_int;
    // AFC (docs/SPEC.md 3.0e, 3.0f): an NCO channel's step changed in a stream without a phase jump, and the frequency measure
    pub fn p25fe_afc_set_step(tn: *mut Tuner, k: i32, step: i32, abs_at: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_afc_get_step(tn: *const Tuner, k: i32, step: *mut i32, ph0: *mut u32) -> c_int;
    pub fn p25fe_afc_factor(step: i32, ph0: u32, n: u64, cs: *mut f32) -> c_int;
    pub fn p25fe_afc_design(d: i32, cutoff_hz: f64, t: i32, taps: *mut f32, cap: usize) -> c_int;
    pub fn p25fe_afc_create(h: *mut Handle, d: i32, t: i32, taps: *const f32, k: i32, out: *mut *mut Afc) -> c_int;
    pub fn p25fe_afc_destroy(afc: *mut Afc);
    pub fn p25fe_afc_measure_dev(afc: *mut Afc, d_rows: *const f32, row_stride: usize, n_hist: usize, n: usize, abs_first: u64,
                                 shift: i32, d_acc: *mut AfcAcc, stream: *mut c_void) -> c_int;
    pub fn p25fe_afc_hz(acc: *const AfcAcc, d: i32, hz: *mut f64, coherence: *mut f64) -> c_int;
    // AFC loop (docs/SPEC.md 3.0g): every channel's (step, ph0) updated on the device from its record, in stream order
    pub fn p25fe_track_create(tn: *mut Tuner, afc: *mut Afc, cfg: *const TrackCfg, out: *mut *mut Track) -> c_int;
    pub fn p25fe_track_destroy(lp: *mut Track);
    pub fn p25fe_track_records(lp: *mut Track, get: *mut AfcAcc, set: *const AfcAcc) -> c_int;
    pub fn p25fe_track_measure_dev(lp: *mut Track, d_rows: *const f32, row_stride: usize, n_hist: usize, n: usize, abs_first: u64,
                                   stream: *mut c_void) -> c_int;
    pub fn p25fe_track_update_dev(lp: *mut Track, abs_at: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_track_run_dev(lp: *mut Track, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64, window: u64,
                               d_out: *mut f32, out_stride: usize, n_hist_out: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_track_read(lp: *mut Track, state_out: *mut TrackState) -> c_int;
    pub fn p25fe_track_step(cfg: *const TrackCfg, l: i32, m: i32, d: i32, step_ref: i32, acc_in: *const AfcAcc,
                            state_in: *const TrackState, abs_at: u64, acc_out: *mut AfcAcc, state_out: *mut TrackState) -> c_int;
    pub fn p25fe_track_hz(state: *const TrackState, d: i32, hz: *mut f64) -> c_int;
    // survey (docs/SPEC.md 3.0h): per-bin power sums of one capture row (the record is N + 1 words), and its active raster channels
    pub fn p25fe_scan_window(n: i32, w: *mut f32, cap: usize) -> c_int;
    pub fn p25fe_scan_create(h: *mut Handle, n: i32, hop: i32, window: *const f32, shift: i32, out: *mut *mut Scan) -> c_int;
    pub fn p25fe_scan_destroy(sc: *mut Scan);
    pub fn p25fe_scan_reset(sc: *mut Scan) -> c_int;
    pub fn p25fe_scan_dev(sc: *mut Scan, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64, d_acc: *mut u64,
                          stream: *mut c_void) -> c_int;
    pub fn p25fe_scan(sc: *mut Scan, iq: *const c_void, fmt: c_int, n: usize) -> c_int;
    pub fn p25fe_scan_read(sc: *mut Scan, acc_out: *mut u64, clear: c_int) -> c_int;
    pub fn p25fe_scan_channels(acc: *const u64, n: i32, fs_hz: u32, raster_hz: f64, half_bw_hz: f64, thr_db: f64, out: *mut ScanChan,
                               cap: usize, n_out: *mut usize) -> c_int;
    // survey over time (docs/SPEC.md 3.0i): the frames of a range into one row of N + 1 words per slot of B frames, and keyed intervals
    pub fn p25fe_waterfall_slots(hop: i32, b: u32, abs_first: u64, n: usize, first_slot: *mut u64, n_slots: *mut usize) -> c_int;
    pub fn p25fe_waterfall_dev(sc: *mut Scan, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64, b: u32,
                               slot0: u64, d_rows: *mut u64, n_rows: usize, row_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_waterfall_open(sc: *mut Scan, b: u32, max_rows: usize) -> c_int;
    pub fn p25fe_waterfall(sc: *mut Scan, iq: *const c_void, fmt: c_int, n: usize) -> c_int;
    pub fn p25fe_waterfall_read(sc: *mut Scan, rows_out: *mut u64, cap_rows: usize, n_rows: *mut usize) -> c_int;
    pub fn p25fe_waterfall_keys(rows: *const u64, n_rows: usize, row_stride: usize, n: i32, fs_hz: u32, slot0: u64, raster_hz: f64,
                                half_bw_hz: f64, on_db: f64, off_db: f64, min_slots: u32, out: *mut WaterfallKey, cap: usize,
                                n_out: *mut usize) -> c_int;
    pub fn p25fe_cuts_from_keys(keys: *const WaterfallKey, n_keys: usize, n: i32, hop: i32, b: u32, fs_hz: u32, margin: u64,
                                range_first: u64, range_n: u64, out: *mut Cut, cap: usize, n_out: *mut usize) -> c_int;
    pub fn p25fe_cuts_create(tn: *mut Tuner, cuts: *const Cut, n_cuts: usize, counts_out: *mut usize, max_count: *mut usize,
                             out: *mut *mut Cuts) -> c_int;
    pub fn p25fe_cuts_destroy(ct: *mut Cuts);
    pub fn p25fe_cuts_dev(ct: *mut Cuts, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64,
                          d_out: *mut f32, out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_keys_create(sc: *mut Scan, fs_hz: u32, raster_hz: f64, half_bw_hz: f64, on_db: f64, off_db: f64, min_slots: u32,
                             max_rows: usize, max_keys: usize, out: *mut *mut Keys) -> c_int;
    pub fn p25fe_keys_destroy(kp: *mut Keys);
    pub fn p25fe_keys_dev(kp: *mut Keys, d_rows: *const u64, n_rows: usize, row_stride: usize, slot0: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_keys_stream(kp: *mut Keys) -> c_int;
    pub fn p25fe_keys_read(kp: *mut Keys, out: *mut WaterfallKey, cap: usize, n_out: *mut usize) -> c_int;
    pub fn p25fe_n_baseband(abs0: u64, n: usize) -> usize;
    pub fn p25fe_slice_dev(h: *mut Handle, d_bb: *const f32, bb_stride: usize, n_hist_bb: usize, n_bb: usize, abs_bb0: u64,
                           d_anchor_in: *const Anchor, d_dibits: *mut u8, dibit_stride: usize, d_sync_pos: *mut i64,
                           d_sync_dibit: *mut u64, sync_stride: usize, d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_run_dev(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n: usize, d_dibits: *mut u8,
                         dibit_stride: usize, d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_run_dev_pipelined(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n: usize, d_dibits: *mut u8,
                                   dibit_stride: usize, d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_join_dev(h: *mut Handle, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_halo() -> usize;
    pub fn p25fe_shard_pass1(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize, abs0: u64,
                             d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pass1_main(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize,
                                  abs0: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pass1_finish(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize,
                                    abs0: u64, d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pass1_head(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize,
                                  abs0: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pipe_begin(h: *mut Handle, stream: *mut c_void, rx_stream: *mut *mut c_void) -> c_int;
    pub fn p25fe_shard_pipe_end(h: *mut Handle, last_stream: *mut c_void) -> c_int;
    pub fn p25fe_rx_stream(h: *mut Handle, rx_stream: *mut *mut c_void) -> c_int;
    pub fn p25fe_shard_head_check(h: *mut Handle) -> c_int;
    /// diagnostic: the planar baseband and sign words of the handle's most recent scratch-using call (include/p25fe.h)
    pub fn p25fe_debug_planes_size(h: *const Handle, n_bb: usize, n_floats: *mut usize, n_words: *mut usize) -> c_int;
    pub fn p25fe_debug_planes_dev(h: *mut Handle, n_bb: usize, d_f: *mut f32, f_stride: usize, d_bits: *mut u32, bits_stride: usize,
                                  stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pass1_k1(h: *mut Handle, d_iq: *const c_void, fmt: c_int, ch_stride: usize, n_hist: usize, n: usize,
                                abs0: u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_streams_share_queue(h: *mut Handle, stream_a: *mut c_void, stream_b: *mut c_void, shared: *mut c_int) -> c_int;
    pub fn p25fe_shard_pass2(h: *mut Handle, d_anchor_in: *const Anchor, d_dibits: *mut u8, dibit_stride: usize,
                             d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_pass2_dev(h: *mut Handle, d_summaries: *const ResultRec, d_shard_bb0: *const u64, d_shard_bb_n: *const u64,
                                 n_shards: usize, rank: usize, d_anchor_in: *mut Anchor, d_dibit_offset: *mut u64, d_dibits: *mut u8,
                                 dibit_stride: usize, d_dibits_dup: *mut u8, d_result: *mut ResultRec, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_resolve(summaries: *const ResultRec, shard_bb0: *const u64, shard_bb_n: *const u64, n_shards: usize,
                               symbol_clock: c_int, anchor_in: *mut Anchor, dibit_offset: *mut u64) -> c_int;
    pub fn p25fe_shard_resolve_dev(h: *mut Handle, d_summaries: *const ResultRec, d_shard_bb0: *const u64, d_shard_bb_n: *const u64,
                                   n_shards: usize, d_anchor_in: *mut Anchor, d_dibit_offset: *mut u64, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_compact_dev(h: *mut Handle, d_gathered: *const u8, cap: usize, d_dibit_offset: *const u64, n_shards: usize,
                                   d_out: *mut u8, out_cap: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_compact_from_dev(h: *mut Handle, d_gathered: *const u8, cap: usize, d_dibit_offset: *const u64,
                                        first_shard: usize, n_shards: usize, d_out: *mut u8, out_cap: usize,
                                        stream: *mut c_void) -> c_int;
    pub fn p25fe_nid_dev(h: *mut Handle, d_dibits: *const u8, n_dibits: usize, d_sync_dibit: *const u64, d_sync_pos: *const i64,
                         n_sync: usize, d_out: *mut Nid, stream: *mut c_void) -> c_int;
    pub fn p25fe_nid(h: *mut Handle, dibits: *const u8, n_dibits: usize, sync_dibit: *const u64, sync_pos: *const i64, n_sync: usize,
                     out: *mut Nid) -> c_int;
    pub fn p25fe_nid_batch_dev(h: *mut Handle, d_dibits: *const u8, dibit_stride: usize, d_result: *const ResultRec,
                               d_sync_dibit: *const u64, d_sync_pos: *const i64, sync_stride: usize, d_out: *mut Nid,
                               stream: *mut c_void) -> c_int;
    pub fn p25fe_chan_stats_dev(h: *mut Handle, d_result: *const ResultRec, d_nid: *const Nid, sync_stride: usize,
                                d_power_dbm: *const f32, d_stats: *mut ChanStats, stream: *mut c_void) -> c_int;
    pub fn p25fe_channelise_dev(h: *mut Handle, d_iq: *const f32, n_hist: usize, n: usize, abs0: u64, d_out: *mut f32,
                                out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_channelise_fmt_dev(h: *mut Handle, d_iq: *const c_void, fmt: c_int, n_hist: usize, n: usize, abs_first: u64,
                                    d_out: *mut f32, out_stride: usize, stream: *mut c_void) -> c_int;
    pub fn p25fe_n_baseband_h(h: *const Handle, abs0: u64, n: usize) -> usize;
    pub fn p25fe_profile_enable(h: *mut Handle, on: c_int) -> c_int;
    pub fn p25fe_profile_read(h: *mut Handle, ms: *mut f64, n_calls: *mut u64) -> c_int;
}

#[link(name = "p25fe_rccl")]
extern "C" {
    pub fn p25fe_rccl_unique_id(id128: *mut u8) -> c_int;
    pub fn p25fe_shard_create(h: *mut Handle, rank: c_int, world: c_int, id128: *const u8, n_per_rank: usize, out: *mut *mut Shard) -> c_int;
    pub fn p25fe_shard_destroy(s: *mut Shard);
    pub fn p25fe_shard_dibit_cap(s: *const Shard) -> usize;
    pub fn p25fe_shard_step(s: *mut Shard, d_buf: *mut c_void, fmt: c_int, d_dibits: *mut u8, d_result: *mut ResultRec, gather: c_int,
                            stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_step_pipelined(s: *mut Shard, d_buf: *mut c_void, fmt: c_int, d_dibits: *mut u8, d_result: *mut ResultRec,
                                      gather: c_int, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_join(s: *mut Shard, stream: *mut c_void) -> c_int;
    pub fn p25fe_shard_offsets(s: *mut Shard, offsets: *mut u64) -> c_int;
    pub fn p25fe_shard_stream_dev(s: *const Shard) -> *const u8;
    pub fn p25fe_shard_comm_ms(s: *mut Shard, ms: *mut f64, n_steps: *mut u64) -> c_int;
    pub fn p25fe_shard_comm_timing(s: *mut Shard, every: c_int) -> c_int;
    pub fn p25fe_shard_gather_ran(s: *const Shard) -> c_int;
    pub fn p25fe_shard_info(s: *const Shard, out: *mut ShardInfo) -> c_int;
    pub fn p25fe_shard_prepare(s: *mut Shard, stream: *mut c_void) -> c_int;
}

/// `p25fe_shard_info_t`: what the shard object itself knows about the job (RCCL's own rank count, this rank's GPU, the agreed layout)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ShardInfo {
    pub rank: i32,
    pub world: i32,
    pub rccl_ranks: i32,
    pub rccl_rank: i32,
    pub device: i32,
    pub comms: i32,
    pub pipe_layout: i32,
    pub gather_ran: i32,
    pub staged: i32,
    pub head_wait: i32,
    pub broken: i32,
    pub reserved: i32,
    pub steps: u64,
    pub pci_bus_id: [c_char; 32],
}

/// Owning wrapper of one handle.  One per thread, like the tasks of the reference (src/main.rs:270-287).
pub struct FrontEnd {
    h: *mut Handle,
}
unsafe impl Send for FrontEnd {}

fn check(rc: c_int, what: &str) {
    // the reference's convention for this path: every failure aborts (`expect`, panic = "abort", Cargo.toml:50-51)
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(p25fe_strerror(rc)) };
        panic!("{}: {}", what, msg.to_string_lossy());
    }
}

impl FrontEnd {
    /// The build's own numbers (decimation 5, boxcar 10, 5 kHz at 48 kHz: src/demod.rs:50-54).
    pub fn new(device: i32) -> Self {
        let mut cfg: Config = unsafe { std::mem::zeroed() };
        unsafe { p25fe_default_config(&mut cfg) };
        cfg.device = device;
        Self::with_config(&cfg)
    }

    /// The reference's own numbers: p25_filts' tables, rtlsdr_iq's table, FmDemod's arguments.  The library compiles its
    /// kernels for them (once per set of numbers, cached on disk): no slower than the built-in ones.
    pub fn with_tables(device: i32, decim: &[f32], chan: &[f32], iq_lut: Option<&[f32; 256]>, deviation: u32, rate: u32) -> Self {
        let mut cfg: Config = unsafe { std::mem::zeroed() };
        unsafe { p25fe_default_config(&mut cfg) };
        cfg.device = device;
        cfg.n_decim_taps = decim.len() as i32;
        cfg.n_chan_taps = chan.len() as i32;
        cfg.decim_taps[..decim.len()].copy_from_slice(decim);
        cfg.chan_taps[..chan.len()].copy_from_slice(chan);
        if let Some(lut) = iq_lut {
            cfg.u8_lut_valid = 1;
            cfg.u8_lut = *lut;
        }
        cfg.fm_deviation_hz = deviation;
        cfg.fm_sample_rate_hz = rate;
        Self::with_config(&cfg)
    }

    pub fn with_config(cfg: &Config) -> Self {
        let mut h: *mut Handle = std::ptr::null_mut();
        check(unsafe { p25fe_create(cfg, &mut h) }, "unable to create the front end");
        FrontEnd { h: h }
    }

    /// One loop body of DemodTask::run (src/demod.rs:70-117); returns the number of baseband samples written.
    pub fn demod_u8(&mut self, bytes: &[u8], baseband: &mut [f32], power_dbm: Option<&mut f32>) -> usize {
        let mut n_out = 0usize;
        let p = power_dbm.map_or(std::ptr::null_mut(), |r| r as *mut f32);
        check(unsafe { p25fe_demod_u8(self.h, bytes.as_ptr(), bytes.len(), baseband.as_mut_ptr(), baseband.len(), &mut n_out, p) },
              "unable to demodulate");
        n_out
    }

    /// The sample loop of RecvTask::run (src/recv.rs:148-150) down to "a dibit exists"; returns (dibits, sync events).
    pub fn slice(&mut self, baseband: &[f32], dibits: &mut [u8], sync_pos: &mut [i64], sync_dibit: &mut [u64]) -> (usize, usize) {
        let (mut nd, mut ns) = (0usize, 0usize);
        let cap = sync_pos.len().min(sync_dibit.len());
        check(unsafe { p25fe_slice(self.h, baseband.as_ptr(), baseband.len(), dibits.as_mut_ptr(), dibits.len(), &mut nd,
                                   sync_pos.as_mut_ptr(), sync_dibit.as_mut_ptr(), cap, &mut ns) }, "unable to slice");
        (nd, ns.min(cap))
    }

    /// MessageReceiver::resync (src/recv.rs:136, 179)
    pub fn resync(&mut self) {
        check(unsafe { p25fe_resync(self.h) }, "unable to resync");
    }

    /// A long recording from host memory at bus speed (the replay path, src/replay.rs:26-37, for IQ files).
    pub fn run_host_windows_u8(&mut self, bytes: &[u8], dibits: &mut [u8]) -> (usize, WindowsStats) {
        let mut nd = 0usize;
        let mut st = WindowsStats::default();
        check(unsafe { p25fe_run_host_windows(self.h, bytes.as_ptr() as *const c_void, FMT_U8, bytes.len() / 2, 0, dibits.as_mut_ptr(),
                                              dibits.len(), &mut nd, &mut st) }, "unable to run the capture");
        (nd, st)
    }

    pub fn raw(&self) -> *mut Handle {
        self.h
    }
}

impl Drop for FrontEnd {
    fn drop(&mut self) {
        unsafe { p25fe_destroy(self.h) };
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// DemodTask with the handle in place of decim / bandpass / avg / demod (src/demod.rs:25-40): same constructor arguments, same
// channels, same messages.  Replaces the struct and impl of src/demod.rs:24-119; `power_dbm` (src/demod.rs:123-134) stays
// for other callers.  (`use` lines as in src/demod.rs:3-21 minus the six DSP crates.)
// ---------------------------------------------------------------------------------------------------------------------
/*
pub struct DemodTask {
    fe: FrontEnd,
    reader: Receiver<Checkout<Vec<u8>>>,
    hub: mio_more::channel::Sender<HubEvent>,
    chan: Sender<RecvEvent>,
}

impl DemodTask {
    pub fn new(reader: Receiver<Checkout<Vec<u8>>>, hub: mio_more::channel::Sender<HubEvent>, chan: Sender<RecvEvent>) -> Self {
        DemodTask {
            // the reference's own tables and constants, as data (src/demod.rs:27-29, 54, 83)
            fe: FrontEnd::with_tables(0, &DECIM_TAPS, &BANDPASS_TAPS, Some(&IQ_BYTE_TABLE), 5000, BASEBAND_SAMPLE_RATE),
            reader: reader, hub: hub, chan: chan,
        }
    }

    pub fn run(&mut self) {
        let mut pool = Pool::with_capacity(16, || vec![0.0; BUF_SAMPLES]);                 // src/demod.rs:63
        let mut notifier = Throttler::new(4);                                               // src/demod.rs:67
        loop {
            let bytes = self.reader.recv().expect("unable to receive sdr samples");        // src/demod.rs:70
            let mut baseband = pool.checkout().expect("unable to allocate baseband");      // src/demod.rs:103
            unsafe { baseband.set_len(BUF_SAMPLES); }
            let mut power = 0f32;
            let mut want = false;
            notifier.throttle(|| want = true);                                              // src/demod.rs:95
            let n = self.fe.demod_u8(&bytes[..], &mut baseband[..], if want { Some(&mut power) } else { None });
            unsafe { baseband.set_len(n); }                                                 // 3276 / 3277, src/demod.rs:87-90, 106
            if want {
                self.hub.send(HubEvent::UpdateSignalPower(power)).expect("unable to send signal power");   // src/demod.rs:99
            }
            self.chan.send(RecvEvent::Baseband(baseband)).expect("unable to send baseband");               // src/demod.rs:116
        }
    }
}
*/
