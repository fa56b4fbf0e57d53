/*
 * p25fe.h -- C ABI of the MI355X-native P25 front end (IQ -> 48 kHz baseband -> C4FM dibits).
 *
 * Drop-in boundary for the hot path of kchmck/p25rx.  The reference has no FFI for this path:
 * it is two Rust task types wired by channels.  Each entry point below names
 * the reference item whose work it replaces; INTEGRATION.md shows the Rust `extern "C"` block
 * and the DemodTask / RecvTask edits a maintainer would make.
 *
 *   reference item (file:line in /root/reference)                  replaced by
 *   -------------------------------------------------------------  ---------------------------
 *   DemodTask::new   src/demod.rs:44-59                             p25fe_create
 *     Decimator::new(5)                 :50, 87-90                  p25fe_config_t.decim_phase (the factor 5 is the build's)
 *     MovingAverage::new(10)            :52, 114                    p25fe_config_t.n_avg_taps / avg_taps
 *     DecimFir / BandpassFir tables     :27-29                      p25fe_config_t.decim_taps / chan_taps
 *     FmDemod::new(5000, 48000)         :54                         p25fe_config_t.fm_deviation_hz / fm_sample_rate_hz / fm_gain
 *     rtlsdr_iq::IQ                     :83                         p25fe_config_t.u8_scale / u8_offset / u8_lut
 *     (type-level FIRs = compile-time tables)                       p25fe_specialize / p25fe_kernel_variant
 *   DemodTask::run   src/demod.rs:70-117 loop body, u8 chunk        p25fe_demod_u8
 *     IQ[s] LUT                         :74-84
 *     decim.decim_in_place              :87-90
 *     bandpass.feed                     :93
 *     power_dbm                         :95-101, :123-134           (power_dbm out-parameter)
 *     demod.feed / avg.feed             :109-114
 *   RecvTask::run sample loop  src/recv.rs:148-150, 204-210         p25fe_slice
 *     msg.feed(s) down to "a dibit exists" (p25 crate, un-vendored)
 *   MessageReceiver::resync    src/recv.rs:136, 179                 p25fe_resync
 *   reader -> pool -> demodulator pipeline  src/sdr.rs:25-33,        p25fe_run_host_windows (a long host capture as a
 *     src/demod.rs:62-70, 103                                         pipeline of windows at the speed of the bus)
 *   (state hand-off for time-sharded captures; no reference item)   p25fe_state_export/import,
 *                                                                   p25fe_shard_*
 *
 * Conventions kept from the reference: streaming semantics -- any chunking of the input gives
 * the same concatenated output, state lives in the handle (src/demod.rs:25-40); the output count
 * is data dependent (src/demod.rs:87-90).  Convention NOT kept: the reference aborts on every
 * error (`expect`, panic = "abort", Cargo.toml:50-51); here every call returns 0 or a negative
 * p25fe_status, because unwinding across extern "C" is undefined.
 *
 * Threading: one handle per thread (the reference moves each task into its own thread,
 * src/main.rs:270-287).  No globals, no callbacks.  Host-pointer calls are synchronous.
 * *_dev calls take device pointers, enqueue on `stream` (a hipStream_t passed as void*) and do
 * not synchronise.  There is no CPU fallback: without a HIP device p25fe_create fails.
 */
#ifndef P25FE_H
#define P25FE_H

#ifndef __HIPCC_RTC__      /* (the library's own kernel source includes this header under hipRTC, which has no system headers) */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define P25FE_MAX_TAPS 64
#define P25FE_ABI_VERSION 6        /* 3: symbol_clock in the config, clock period in p25fe_anchor_t, carry_end / first_seg_end /
                                      flags in p25fe_result_t, p25fe_resync_at_dev, symbol_clock argument of p25fe_shard_resolve
                                      4: the run-time arguments of the reference's constructors in the config (FM deviation / rate,
                                      the u8 -> float LUT), `specialize`, p25fe_specialize / p25fe_kernel_variant,
                                      p25fe_run_host_windows
                                      5: the LAST constructor numbers: the post-discriminator filter as a table (avg_taps:
                                      MovingAverage::new(10)) and the decimator's phase (decim_phase: Decimator::new(5));
                                      p25fe_n_baseband_h; p25fe_shard_halo() is 2 560; p25fe_shard_pass1_head / _pass2_dev /
                                      _compact_from_dev; p25fe_probe_variant
                                      6: symbol_clock = 2 is refused by the calls that cannot run SPEC 3.8c unless P25FE_CLOCK_CAUSAL_OK
                                      is or-ed in; P25FE_ERR_TIMEOUT, p25fe_shard_head_check (the detection's wait for a shard's head is
                                      bounded); p25fe_rx_stream; p25fe_rccl.h: p25fe_shard_info, p25fe_shard_prepare (no step probes or
                                      synchronises streams any more), the communicator layout agreed by all ranks */

typedef enum p25fe_status {
    P25FE_OK = 0,
    P25FE_ERR_ARG = -1,        /* null pointer, bad size, bad config */
    P25FE_ERR_NO_DEVICE = -2,  /* no HIP device / wrong architecture */
    P25FE_ERR_HIP = -3,        /* a HIP runtime call failed (see p25fe_last_hip_error) */
    P25FE_ERR_CAPACITY = -4,   /* output buffer too small; nothing consumed */
    P25FE_ERR_FORMAT = -5,     /* u8 / cf32 / s16 mixed within one stream */
    P25FE_ERR_NOMEM = -6,
    P25FE_ERR_JIT = -7,        /* specialising the kernels failed (p25fe_specialize_log has the compiler's words) */
    P25FE_ERR_TIMEOUT = -8     /* a device-side wait gave up (the head segment of a time shard never arrived: p25fe_shard_head_check) */
} p25fe_status;

typedef enum p25fe_format {
    P25FE_FMT_CF32 = 0,        /* interleaved float32 I,Q (num::Complex32 layout) */
    P25FE_FMT_U8 = 1,          /* interleaved uint8 I,Q (RTL-SDR; src/demod.rs:74-76) */
    P25FE_FMT_S16 = 2          /* interleaved int16_t I,Q, native little-endian, I first, 4 bytes per complex sample (Airspy, SDRplay,
                                  USRP sc16, BladeRF, SigMF ci16_le; no reference item: the reference reads an RTL-SDR).  Value
                                  (float)v * P25FE_S16_SCALE -- exact in fp32 for every int16_t, -32768 is -1.0 -- so an s16 stream IS the
                                  cf32 stream of its converted samples, bit for bit, at every output (docs/SPEC.md 3.1).  The scale
                                  is fixed: no configuration field. */
} p25fe_format;
#define P25FE_S16_SCALE 0x1p-15f

/* Replaces the compile-time DSP parameters of DemodTask::new (src/demod.rs:49-54: every constructor argument of the four DSP
 * objects, ABI 5), the type-level tap tables of p25_filts (DecimFir / BandpassFir, src/demod.rs:27-29), the arguments of
 * FmDemod::new (src/demod.rs:54) and the rtlsdr_iq::IQ lookup table (src/demod.rs:83).  Up to P25FE_MAX_TAPS = 64 taps per filter; a table of n taps is evaluated as 31 / 41 taps (64 / 64
 * as soon as either table is longer) with zero coefficients at the old end: the same filter on finite samples; a NaN / Inf
 * sample reaches that many taps' worth of outputs (docs/SPEC.md 3.3).
 *
 * Which kernels run (p25fe_kernel_variant): the build's own numbers (p25fe_default_config) run as the immediate-coefficient
 * kernels compiled into the library.  ANY other table / constant set is compiled the same way -- the reference fixes its
 * tables at compile time too (type-level FIRs, src/demod.rs:27-29) -- by hipRTC at p25fe_create (or ahead of time by
 * p25fe_specialize) from the kernel source embedded in the library, cached on disk under a hash of the numbers; the
 * generic kernels (taps broadcast-read from LDS, the LUT in LDS) are the fallback when that is switched off or fails. */
typedef struct p25fe_config {
    int32_t abi_version;                 /* P25FE_ABI_VERSION */
    int32_t device;                      /* HIP device ordinal */
    int32_t n_channels;                  /* independent channels per call, channel-major */
    int32_t n_decim_taps;
    int32_t n_chan_taps;
    float decim_taps[P25FE_MAX_TAPS];    /* 240k -> 48k anti-alias, tap 0 multiplies the newest sample */
    float chan_taps[P25FE_MAX_TAPS];     /* 48 kHz channel-select low-pass */
    int32_t symbol_clock;                /* P25FE_CLOCK_FIXED (0, default): symbol instants at a fixed 10-sample stride from the last
                                            sync word, the receiver structure of the reference; P25FE_CLOCK_TRACKING (1): docs/SPEC.md
                                            3.8b -- the stride is the measured interval between the last two sync words over its
                                            symbol count, instants are read by 4-tap interpolation, the receiver runs 2 samples
                                            behind the baseband; P25FE_CLOCK_TRACKING_RESLICE (2): the same, and the calls that hold
                                            a whole range re-slice the first frame of a lock run (SPEC 3.8c, see the define; the calls
                                            that cannot are refused unless P25FE_CLOCK_CAUSAL_OK is or-ed in) */
    int32_t specialize;                  /* P25FE_SPECIALIZE_AUTO (0): non-default numbers get immediate-coefficient kernels (cache, then
                                            hipRTC), the generic kernels if that fails; _OFF (-1): always the generic kernels for
                                            non-default numbers; _REQUIRE (1): p25fe_create fails with P25FE_ERR_JIT instead of
                                            falling back; _FORCE (2): as _REQUIRE, and the build's own numbers are specialised too
                                            (measurement: the hipRTC product beside the library's own code object) */
    /* ---- ABI 4 ---- */
    uint32_t fm_deviation_hz;            /* FmDemod::new(5000, BASEBAND_SAMPLE_RATE), src/demod.rs:54: first argument */
    uint32_t fm_sample_rate_hz;          /* ... second argument: the rate of the discriminator's input (src/consts.rs:13: 48 000) */
    float fm_gain;                       /* 0 (default): the discriminator's output scale is (float)(fm_sample_rate_hz / (2 pi
                                            fm_deviation_hz)), evaluated in double and rounded once (docs/SPEC.md 3.4); any other
                                            finite value is used verbatim (a dump of demod_fm's own constant, tools/pin/) */
    float u8_scale, u8_offset;           /* rtlsdr_iq::IQ (src/demod.rs:83) as arithmetic: byte b -> fma((float)b, u8_scale, u8_offset)
                                            (docs/SPEC.md 3.1; defaults 2 / 255, -1) */
    int32_t u8_lut_valid;                /* non-zero: u8_lut[b] IS the value of byte b (I and Q alike) and u8_scale / u8_offset are
                                            ignored.  A table that equals fma(b, s, o) bit for bit for some (s, o) the library
                                            finds runs as arithmetic; any other table is looked up in LDS. */
    float u8_lut[256];
    /* ---- ABI 5 ---- */
    int32_t decim_phase;                 /* Decimator::new(5) / decim_in_place (src/demod.rs:50, 87-90): output m of the 5:1 decimator
                                            is produced by the input sample with absolute index 5 m + decim_phase, 0..4.  Default 4
                                            (the 5th, 10th, ... sample: 16 384-sample chunks give 3 276, 3 277, 3 277, ... outputs). */
    int32_t n_avg_taps;                  /* MovingAverage::new(10) (src/demod.rs:52, 114) as a table: the real FIR behind the
                                            discriminator, 1 .. P25FE_MAX_TAPS taps, tap 0 on the newest sample (docs/SPEC.md 3.5).
                                            A table whose taps are ALL EQUAL is a moving average and is evaluated as one: the
                                            samples summed newest first, then one multiply by the tap -- the default, ten taps of
                                            (float)0.1, gives the bits of every earlier ABI.  Any other table (e.g. the raised
                                            cosine P25FE_RC_AVG_TAPS of p25fe_spec.h) is evaluated like the other two FIRs: one
                                            accumulator from +0, fma in tap order. */
    float avg_taps[P25FE_MAX_TAPS];
} p25fe_config_t;

#define P25FE_CLOCK_FIXED 0
#define P25FE_CLOCK_TRACKING 1
/* P25FE_CLOCK_TRACKING plus docs/SPEC.md 3.8c in the calls that hold a whole range in device memory (p25fe_run_dev,
 * p25fe_run_dev_pipelined, p25fe_slice_dev): a detection without a period of its own -- the first of a lock run -- is sliced with
 * the period of the interval that STARTS at it, once the next sync word of the range confirms one, and every detection's instants
 * start from its refined position s + f / 4 instead of the whole sample s (0 symbol errors of 2.88 M at 150 ppm where
 * P25FE_CLOCK_TRACKING leaves 29 and the fixed stride 16 502).  That is not causal, so the calls that see the stream in pieces --
 * p25fe_slice, p25fe_run_u8 / _cf32, p25fe_run_host_windows, the time-shard passes (and with them p25fe_shard_step) -- cannot run it: they
 * have P25FE_CLOCK_TRACKING's rule only ("any chunking gives the same output", src/demod.rs:25-40).  ABI 6: on a handle created with
 * symbol_clock = 2 those calls return P25FE_ERR_ARG -- a request for one receiver is not answered with another's dibits -- unless the
 * handle was created with symbol_clock = P25FE_CLOCK_TRACKING_RESLICE | P25FE_CLOCK_CAUSAL_OK: 3.8c where a call holds the range, 3.8b
 * everywhere else, and a resident call and a streaming call then differ, by design (what ABI 5's mode 2 did without being asked). */
#define P25FE_CLOCK_TRACKING_RESLICE 2
#define P25FE_CLOCK_CAUSAL_OK 0x100
#define P25FE_SPECIALIZE_AUTO 0
#define P25FE_SPECIALIZE_OFF (-1)
#define P25FE_SPECIALIZE_REQUIRE 1
#define P25FE_SPECIALIZE_FORCE 2

typedef struct p25fe p25fe_t;

/* Symbol-timing anchor carried between calls / shards: the last frame-sync detection. */
typedef struct p25fe_anchor {
    int64_t s;                           /* absolute baseband index of the sync word's last symbol */
    float hi, mid, lo;                   /* slicer thresholds derived from that sync word */
    int32_t valid;                       /* 0: no lock.  Non-zero: locked -- bit 0 set; with the tracking clock bits 8..10 carry the sync
                                            position's fraction in quarter samples (3-bit two's complement, docs/SPEC.md 3.8b: it
                                            enters the NEXT detection's period; 0 from the fixed-stride receiver).  Test `valid != 0`. */
    int32_t period_d, period_n;          /* symbol period period_d / period_n samples (10 / 1 unless the clock tracks -- then quarter
                                            samples over four times the interval's symbol count; 0 / 0 reads as 10 / 1) */
} p25fe_anchor_t;

/* Per-channel summary of one processed range (device or host memory, see each call). */
typedef struct p25fe_result {
    uint64_t n_baseband;                 /* baseband samples produced */
    uint64_t n_dibits;                   /* dibits produced */
    uint64_t n_sync;                     /* frame-sync detections */
    p25fe_anchor_t anchor_out;           /* anchor after the range */
    int64_t first_event;                 /* baseband index at which the range's first own detection is decided (s + W), -1 if none */
    uint64_t n_dibits_after_first;       /* dibits governed by the range's own detections */
    /* what p25fe_shard_resolve needs beyond that when the clock tracks or lock is dropped inside ranges: */
    int64_t carry_end;                   /* index from which the carry-in anchor no longer governs (first_event + 1, or the first lock
                                            drop if that comes first; never negative); -1: it governs the whole range */
    int64_t first_seg_end;               /* end (exclusive) of the interval the first own detection governs: the next event of the range (detection or lock drop) or the range's end */
    uint32_t flags;                      /* P25FE_RES_* */
    uint32_t reserved;                   /* tracking clock: quarter-sample fraction (3-bit two's complement) of the first own detection's sync position; else 0 */
} p25fe_result_t;
#define P25FE_RES_FIRST_TRACKS_CARRY 1u  /* no lock drop between the range's start and its first detection: with a tracking clock that
                                            detection takes its period from the carry-in (n_dibits_after_first assumed 10 / 1) */
#define P25FE_RES_OUT_PERIOD_FROM_CARRY 2u /* anchor_out's period is that same interval (the range has one detection, nothing else) */

void p25fe_default_config(p25fe_config_t *cfg);
int p25fe_create(const p25fe_config_t *cfg, p25fe_t **out);
void p25fe_destroy(p25fe_t *h);
const char *p25fe_strerror(int status);
int p25fe_last_hip_error(const p25fe_t *h);      /* raw hipError_t of the last P25FE_ERR_HIP */
int p25fe_device(const p25fe_t *h);              /* HIP device ordinal the handle lives on (p25fe_config_t.device); < 0: null handle */

/* Which front-end kernels the handle launches: the library's own immediate-coefficient kernels (the config's numbers are
 * the build's), kernels specialised for the config's numbers (cache / hipRTC), or the generic LDS-tap kernels. */
#define P25FE_VARIANT_BUILTIN 0
#define P25FE_VARIANT_SPECIALIZED 1
#define P25FE_VARIANT_GENERIC 2
int p25fe_kernel_variant(const p25fe_t *h);      /* < 0: null handle */
/* The same per input format.  P25FE_FMT_U8 / _CF32: p25fe_kernel_variant.  P25FE_FMT_S16 has no specialised kernels (a code object
 * keeps exactly its six): BUILTIN with the build's numbers; with any others GENERIC -- said once per process on stderr unless
 * specialize is _OFF or P25FE_QUIET=1 -- or, on a handle created with P25FE_SPECIALIZE_REQUIRE / _FORCE, P25FE_ERR_JIT, which is
 * then also what every call given s16 input returns, before any state moves.  P25FE_ERR_ARG: null handle, unknown format. */
int p25fe_format_variant(const p25fe_t *h, int fmt);
/* Ahead-of-time form of what p25fe_create does for non-default numbers (the `make SPEC=` step; needs no GPU): compile the
 * front-end kernels for cfg's tables and constants and store the code object as <dir>/p25fe-<hash>.hsaco (dir NULL: the
 * cache directory -- $P25FE_CACHE_DIR, else $XDG_CACHE_HOME/p25fe, else $HOME/.cache/p25fe, else /tmp/p25fe-cache-<uid>;
 * p25fe_create looks in $P25FE_SPEC_DIR first, then there; what IT compiles is stored as p25fe-<hash>-rtc<version>.hsaco and
 * looked for before the plain name, so another toolchain's object is never preferred over this one's).  path_out (nullable) receives the file name.  Returns P25FE_OK
 * (also when cfg holds the build's own numbers: nothing to do, path_out = ""), P25FE_ERR_JIT or P25FE_ERR_ARG. */
int p25fe_specialize(const p25fe_config_t *cfg, const char *dir, char *path_out, size_t path_cap);
/* Which kernels a handle made from cfg would run ON THIS HOST (P25FE_VARIANT_*), by the same steps p25fe_create takes --
 * $P25FE_SPEC_DIR, the cache, hipRTC (the object is stored in the cache), else the fallback -- but without a device: a
 * deployment check.  When P25FE_SPECIALIZE_AUTO ends on the generic kernels, p25fe_create and this call say so ONCE per
 * process on stderr (P25FE_QUIET=1 silences it).  P25FE_ERR_JIT if cfg->specialize demands what cannot be had.
 * Code objects are read from / written to directories that are real directories owned by the caller (or root) and
 * writable by their owner only; every file carries a trailer that ties its content to cfg's numbers and is verified
 * before it reaches the loader; files under $P25FE_SPEC_DIR are never deleted. */
int p25fe_probe_variant(const p25fe_config_t *cfg);
/* p25fe_format_variant without a device: p25fe_probe_variant for P25FE_FMT_U8 / _CF32, the rule above for P25FE_FMT_S16. */
int p25fe_probe_format_variant(const p25fe_config_t *cfg, int fmt);
/* compiler log of the calling thread's last p25fe_specialize / p25fe_create; returns the length copied (NUL-terminated) */
size_t p25fe_specialize_log(char *buf, size_t cap);

/* ---- streaming, host buffers: the bodies of DemodTask::run and RecvTask::run ----------------
 * Multi-channel handles take channel-major buffers: channel c starts at c * (elements per
 * channel) of the call; every channel gets the same number of input samples. */

/* src/demod.rs:70-117 for one chunk of interleaved u8 I/Q.  n_bytes even.  Writes *n_out
 * baseband samples per channel to bb (channel c at bb + c * bb_cap).  power_dbm (nullable)
 * receives power_dbm() of the post-channel-filter chunk per channel (src/demod.rs:97); the
 * every-4th-chunk throttle (src/demod.rs:67, 95) is the caller's. */
int p25fe_demod_u8(p25fe_t *h, const uint8_t *iq, size_t n_bytes, float *bb, size_t bb_cap, size_t *n_out,
                   float *power_dbm);
/* Same for Complex32 input (BASELINE.json configs 2-5). */
int p25fe_demod_cf32(p25fe_t *h, const float *iq, size_t n_samples, float *bb, size_t bb_cap, size_t *n_out,
                     float *power_dbm);

/* src/recv.rs:148-150: feed n baseband samples per channel; one dibit per byte (0..3) to
 * dibits (channel c at dibits + c * cap), counts to n_dibits[c].  sync_pos / sync_dibit
 * (nullable) receive, per detection, the absolute baseband index of the sync word's last
 * symbol and the index (in the channel's dibit stream) of the first dibit it governs;
 * n_sync[c] gets the number of detections (may exceed sync_cap; extra ones are not stored).
 * Capacity: cap >= n / 10 + 1 is required (an undisturbed lock), cap = n / 6 + 2 is always enough (every re-anchor starts
 * a new symbol grid and two of them are at least 6 samples apart); a chunk that needs more than `cap` returns
 * P25FE_ERR_CAPACITY with the stream state untouched -- repeat the call with more room. */
int p25fe_slice(p25fe_t *h, const float *bb, size_t n, uint8_t *dibits, size_t cap, size_t *n_dibits,
                int64_t *sync_pos, uint64_t *sync_dibit, size_t sync_cap, size_t *n_sync);

/* Same for interleaved int16_t input (P25FE_FMT_S16): n_samples complex samples = 2 n_samples int16_t per channel. */
int p25fe_demod_s16(p25fe_t *h, const int16_t *iq, size_t n_samples, float *bb, size_t bb_cap, size_t *n_out,
                    float *power_dbm);

/* Both halves with the baseband kept in HBM (DemodTask -> RecvTask without the channel hop).  Capacity as for
 * p25fe_slice with n = the chunk's baseband samples (p25fe_n_baseband): n_samples / 30 + 4 is always enough. */
int p25fe_run_u8(p25fe_t *h, const uint8_t *iq, size_t n_bytes, uint8_t *dibits, size_t cap, size_t *n_dibits);
int p25fe_run_cf32(p25fe_t *h, const float *iq, size_t n_samples, uint8_t *dibits, size_t cap, size_t *n_dibits);
int p25fe_run_s16(p25fe_t *h, const int16_t *iq, size_t n_samples, uint8_t *dibits, size_t cap, size_t *n_dibits);

/* A LONG capture in host memory through the same path at the speed of the bus: the capture is cut into windows of `window`
 * samples per channel (0: 64 MB worth; rounded down to a multiple of 8, at least 8 192); window k + 1 travels to the GPU
 * (hipMemcpyAsync on a copy stream, two device windows) while window k is demodulated and sliced, and window k - 1's dibits
 * travel back.  Filter and receiver state cross the window boundaries exactly as they cross a time shard's: the last
 * p25fe_shard_halo() samples stay in front of the next window (device-to-device), the anchor is handed on in device
 * memory.  The reference's shape is the same pipeline with a 16-deep buffer pool between reader and demodulator
 * (src/demod.rs:62-70, 103; src/sdr.rs:25-33).  Continues the handle's stream (any chunking of p25fe_run_* and this call
 * gives the same concatenated dibits) and leaves it ready for more.
 * iq: [C][n] channel-major.  Pinned memory (hipHostMalloc / hipHostRegister) is copied from directly; pageable memory is
 * staged through two pinned windows of the library by the calling thread.  dibits: [C][cap]; capacity as for p25fe_run_*.
 * stats (nullable): where the time went.
 * On an error (P25FE_ERR_CAPACITY from a window's count, P25FE_ERR_HIP) the handle's stream state has not moved -- the call
 * can be repeated -- and nothing of the call is in flight any more, but `dibits` may already hold the dibits of earlier
 * windows and n_dibits reads 0: treat the output buffers as undefined. */
typedef struct p25fe_windows_stats {
    uint64_t n_windows;
    double ms_total;                     /* wall time of the call */
    double ms_h2d;                       /* the H2D copies' own time (events on the copy stream), summed */
    double ms_compute;                   /* the windows' kernels (events on the compute stream), summed */
    int32_t pinned_input;                /* 1: copied straight from the caller's memory, 0: staged by the calling thread */
    int32_t reserved;
} p25fe_windows_stats_t;
int p25fe_run_host_windows(p25fe_t *h, const void *iq, int fmt, size_t n, size_t window, uint8_t *dibits, size_t cap,
                           size_t *n_dibits, p25fe_windows_stats_t *stats);

/* MessageReceiver::resync (src/recv.rs:136, 179): drop symbol lock at the current position. */
int p25fe_resync(p25fe_t *h);
/* The same for device-resident ranges, where "the current position" lies INSIDE the range (RecvTask handles
 * RecvEvent::SetControlFreq between two baseband chunks, src/recv.rs:127-137; a resident capture spans many): the NEXT
 * call on this handle that runs the receiver (p25fe_slice_dev, p25fe_run_dev, p25fe_run_dev_pipelined,
 * p25fe_shard_pass1 / _finish + the p25fe_shard_pass2 that follows; also the host-buffer calls p25fe_slice,
 * p25fe_run_u8 / _cf32, whose range is the chunk) drops lock before each listed sample -- exactly as
 * if resync() had been called between feeding samples q - 1 and q.  d_idx: device array, n_idx ascending ABSOLUTE
 * baseband indices per channel, channel c at d_idx + c * idx_stride (pad a shorter list with INT64_MAX); it must stay
 * valid and unchanged until that call's kernels have run.  n_idx = 0 cancels.  The list is consumed by that call -- a host-buffer
 * call that returns P25FE_ERR_CAPACITY has consumed nothing, the list included; p25fe_reset and p25fe_state_import drop it. */
int p25fe_resync_at_dev(p25fe_t *h, const int64_t *d_idx, size_t n_idx, size_t idx_stride);
/* Forget all stream state (a new DemodTask + MessageReceiver). */
int p25fe_reset(p25fe_t *h);

/* Filter histories, decimator phase, FM/boxcar context and symbol lock as an opaque blob. */
int p25fe_state_size(const p25fe_t *h, size_t *n);
int p25fe_state_export(const p25fe_t *h, void *buf, size_t cap, size_t *n);
int p25fe_state_import(p25fe_t *h, const void *buf, size_t n);

/* ---- device-resident ranges: the measured path -------------------------------------------------
 * d_iq points at the first OWNED sample of channel 0; channel c starts ch_stride elements
 * (complex samples for CF32 and S16, byte pairs for U8) later; it is 16-byte aligned, and ch_stride a multiple of 2 (CF32),
 * 4 (S16) or 8 (U8) samples, so that every channel's first owned sample is (P25FE_ERR_ARG otherwise).  n_hist valid samples precede each
 * channel's first owned sample in memory (0 at the start of a stream: history reads as zero,
 * exactly like the zero-initialised filters of DemodTask::new); abs0 is the absolute index of
 * the first owned sample in its stream (fixes the 5:1 grid, src/demod.rs:87-90).
 * All outputs are device pointers; nothing is synchronised.
 * POSITIONS are 64-bit sample counts: a stream that runs for days passes 2^31 and 2^32 (the IQ
 * index after 4 h 58 min at 240 ksps) and nothing changes there -- a range at position P computes
 * what the same samples compute at any P' congruent to P modulo the stage's grid (5; 10 for the
 * pre-decimator; 10 and 192 for the channeliser; the receiver has none), with every index that
 * comes back shifted by the difference (docs/SPEC.md section 4).
 * The one bound is P25FE_MAX_POSITION = 2^62: the kernels keep signed 64-bit indices and add a
 * range's length on top.  What the host can see is checked and answers P25FE_ERR_ARG at 2^62 or
 * more: abs0 (p25fe_demod_dev, p25fe_predecim_dev, p25fe_channelise_dev -- abs_first in their _fmt_ forms --, the p25fe_shard_pass1
 * forms), abs_bb0 (p25fe_slice_dev), shard_bb0[r] and shard_bb0[r] + shard_bb_n[r] of
 * p25fe_shard_resolve, and in a blob given to p25fe_state_import the two counters and the `s` of
 * every valid anchor.  Positions the library only ever sees in DEVICE memory are the caller's to
 * keep below the bound and are not checked: p25fe_resync_at_dev indices (INT64_MAX is padding, no
 * position), d_anchor_in, and the d_shard_bb0 of p25fe_shard_resolve_dev / p25fe_shard_pass2_dev.
 * The count functions (p25fe_n_baseband, _h, p25fe_n_predecim) are exact for every uint64_t. */
#define P25FE_MAX_POSITION ((uint64_t)1 << 62)

/* stages 1-5: writes n_baseband(n, abs0) samples per channel to d_bb (+ c * bb_stride). */
int p25fe_demod_dev(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                    uint64_t abs0, float *d_bb, size_t bb_stride, float *d_power_dbm, void *stream);

/* Stage 0 of BASELINE.json config 3 (2.4 Msps front end; the reference is fixed at 240 ksps, src/consts.rs:11):
 * 10:1 decimating FIR, cf32 @ 2.4 Msps -> cf32 @ 240 ksps, P25FE_T0 taps of p25fe_spec.h.  Same range
 * conventions as p25fe_demod_dev; writes p25fe_n_predecim(abs0, n) complex samples per channel to d_out
 * (+ c * out_stride complex samples).  Feed d_out to p25fe_run_dev / p25fe_demod_dev. */
int p25fe_predecim_dev(p25fe_t *h, const float *d_iq, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                       float *d_out, size_t out_stride, void *stream);
size_t p25fe_n_predecim(uint64_t abs0, size_t n);
/* The same stage on the capture as the tuner delivers it (docs/SPEC.md 3.0): fmt = P25FE_FMT_U8 (byte pairs, I first; the
 * handle's u8_scale / u8_offset or u8_lut) or P25FE_FMT_S16 (little-endian int16 pairs, I first; value * 2^-15).  The output is,
 * bit for bit, p25fe_predecim_dev's on the converted samples.  d_iq is 16-byte aligned, ch_stride a multiple of 8 (u8) or 4
 * (s16) samples, as for p25fe_demod_dev; only the aligned 16-byte vectors that hold samples [-n_hist, n) of a channel are read.
 * fmt = P25FE_FMT_CF32 is p25fe_predecim_dev itself.  P25FE_ERR_ARG: unknown format, misaligned or null pointer, abs_first >= 2^62. */
int p25fe_predecim_fmt_dev(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                           uint64_t abs_first /* = p25fe_predecim_dev's abs0 */, float *d_out, size_t out_stride, void *stream);

/* ---- rational resampler: any tuner sample rate -> 240 ksps (docs/SPEC.md 3.0b) -------------------
 * A polyphase FIR resampler by L / M (= 240000 / fs_in in lowest terms) with a caller-supplied table taps[0 .. L*T): T taps per
 * phase, index j*L + p is tap j of phase p.  With x[n] = 0 for n < 0:
 *     u = m*M + (M-1);  n_m = u div L;  p_m = u mod L;  y[m] = sum_{j<T} taps[j*L + p_m] x[n_m - j]   (fp32 fma chain, j ascending)
 * L = 1, M = 10, T = 80 with p25fe_spec.h's pre-decimator taps IS p25fe_predecim_dev, bit for bit.  A range [abs_first,
 * abs_first + n) owns the outputs whose n_m lies in it; n_hist >= T - 1 gives exact continuation; the position grid is M.
 * Limits (P25FE_ERR_ARG otherwise): gcd(L, M) = 1, 1 <= L <= P25FE_RS_MAX_L, L < M <= P25FE_RS_MAX_M, 1 <= T <= P25FE_RS_MAX_T,
 * L*T <= P25FE_RS_MAX_TABLE, finite taps. */
#define P25FE_RS_MAX_L 32
#define P25FE_RS_MAX_M 1024
#define P25FE_RS_MAX_T 1024
#define P25FE_RS_MAX_TABLE 4096
#define P25FE_RS_RATE_OUT_HZ 240000u
typedef struct p25fe_resampler p25fe_resampler_t;

/* The table for a tuner rate, no device needed: L / M = 240000 / fs_in_hz reduced, T = ceil(fs_in_hz / 30000) taps per phase, a
 * Kaiser(beta = 7.0)-windowed sinc of L*T points with its cutoff at 60 kHz (at the rate L * fs_in_hz), scaled to sum L, evaluated in
 * double and rounded once (at 2.4 Msps: the design rule of the pre-decimator's own table).  *L, *M, *T are always filled when the
 * ratio is within the limits; taps (cap floats) is filled when cap >= L*T, P25FE_ERR_CAPACITY otherwise (taps may then be null).
 * P25FE_ERR_ARG: a null L / M / T, fs_in_hz = 0, or a reduced ratio outside the limits (fs_in_hz = 240000 among them). */
int p25fe_resampler_design(uint32_t fs_in_hz, int32_t *L, int32_t *M, int32_t *T, float *taps, size_t cap);

/* A resampler on h's device, for h's n_channels and u8 conversion; h must outlive every USE of it (p25fe_resampler_destroy alone
 * is safe after p25fe_destroy(h): it does not read the handle).  The arguments are checked before any
 * device is touched.  The object holds the table's device copy and the state of the host streaming form. */
int p25fe_resampler_create(p25fe_t *h, int32_t L, int32_t M, int32_t T, const float *taps, p25fe_resampler_t **out);
void p25fe_resampler_destroy(p25fe_resampler_t *rs);
int p25fe_resampler_reset(p25fe_resampler_t *rs);      /* the host streaming form restarts at position 0 with zero history */

/* outputs a range owns: floor((abs_first + n) L / M) - floor(abs_first L / M); exact for every uint64_t abs_first (0 for a ratio
 * outside the limits) */
size_t p25fe_n_resample(int32_t L, int32_t M, uint64_t abs_first, size_t n);

/* A device-resident range, conventions as p25fe_predecim_fmt_dev: d_iq points at owned sample 0 of channel 0 and is 16-byte
 * aligned, ch_stride is a multiple of 2 / 4 / 8 samples (cf32 / s16 / u8), only the aligned 16-byte vectors that hold samples
 * [-n_hist, n) of a channel are read.  Writes exactly p25fe_n_resample(L, M, abs_first, n) cf32 samples per channel to d_out +
 * c * out_stride (complex samples) and nothing beyond them; enqueues on `stream`, synchronises nothing.  u8 / s16 input gives,
 * bit for bit, the cf32 call's output on the converted samples.  P25FE_ERR_ARG: null or misaligned pointer, unknown format,
 * out_stride < the count, abs_first >= 2^62. */
int p25fe_resample_dev(p25fe_resampler_t *rs, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                       uint64_t abs_first, float *d_out, size_t out_stride, void *stream);

/* Host streaming form: iq holds n new samples per channel, channel-major ([n_channels][n] in the format's units), out is
 * [n_channels][cap] cf32; *n_out = samples written per channel.  The object keeps the last T - 1 samples and the stream position:
 * any chunking gives the same concatenated output.  P25FE_ERR_CAPACITY (cap too small; *n_out = the count needed) leaves the
 * state untouched; P25FE_ERR_FORMAT when the format differs from the stream's first call (p25fe_resampler_reset starts a new
 * stream).  Synchronous. */
int p25fe_resample(p25fe_resampler_t *rs, const void *iq, int fmt, size_t n, float *out, size_t cap, size_t *n_out);

/* ---- tuner: K channels at chosen frequency offsets out of ONE capture of any supported rate (docs/SPEC.md 3.0c) --------------
 * The resampler above with a mixer in front.  Channel k has the frequency num_k / den_k cycles per INPUT sample, in lowest terms
 * (positive: above the capture's centre; 0 / 1: the centre): with i = ((num mod den)(n mod den)) mod den and the rotator table of
 * den, c = C[i] = (float)cos(2 pi i / den), s = S[i] = (float)sin(2 pi i / den),
 *     v_k[n] = ( fma(x[n].im, s, x[n].re * c), fma(-x[n].re, s, x[n].im * c) )       (= x[n] e^{-j 2 pi num n / den}; num = 0: v = x)
 * and y_k[m] is the resampler's formula on v_k: the same table, counts (p25fe_n_resample), ownership and history rule
 * (n_hist >= T - 1) for every channel.  A channel with num = 0 IS p25fe_resample_dev, bit for bit.  The phase is a function of the
 * absolute index n, so the position grid of channel k is lcm(M, den_k).
 * Limits (P25FE_ERR_ARG otherwise): the resampler's, 1 <= n_out_channels <= P25FE_TUNE_MAX_CH, 1 <= den <= P25FE_TUNE_MAX_DEN,
 * 2 |num| <= den, gcd(|num|, den) = 1.  Every combination inside them runs. */
#define P25FE_TUNE_MAX_CH  256
#define P25FE_TUNE_MAX_DEN 8192
typedef struct p25fe_tuner p25fe_tuner_t;

/* offset_hz / fs_in_hz in lowest terms, the sign on *num; no device needed.  On the 12.5 kHz raster den is 200 at 2.5 Msps, 800 at
 * 10 Msps, 4096 at 2.048 Msps, 192 at 2.4 Msps.  P25FE_ERR_ARG: a null pointer, fs_in_hz = 0, 2 |offset_hz| > fs_in_hz, or a reduced
 * denominator above P25FE_TUNE_MAX_DEN. */
int p25fe_tuner_freq(uint32_t fs_in_hz, int64_t offset_hz, int32_t *num, int32_t *den);
/* The rotator table of den, 2 * den floats: C[0 .. den) then S[0 .. den), evaluated in double and rounded once; no device needed.
 * This function is the table's definition (C[0] = 1 and S[0] = +0 exactly).  P25FE_ERR_ARG: den outside [1, P25FE_TUNE_MAX_DEN];
 * P25FE_ERR_CAPACITY: cap < 2 * den (cs may then be null). */
int p25fe_tuner_rotator(int32_t den, float *cs, size_t cap);

/* A tuner on h's device with h's u8 conversion (h's n_channels does not matter: the input is ONE capture); h must outlive every
 * USE of it (p25fe_tuner_destroy alone is safe after p25fe_destroy(h)).  Every argument is checked before any device is touched.
 * The object holds the table, one rotator table per distinct denominator and the channels' numbers in device memory, and the
 * state of the host streaming form. */
int p25fe_tuner_create(p25fe_t *h, int32_t L, int32_t M, int32_t T, const float *taps,
                       int32_t n_out_channels, const int32_t *num, const int32_t *den, p25fe_tuner_t **out);
void p25fe_tuner_destroy(p25fe_tuner_t *tn);
int p25fe_tuner_reset(p25fe_tuner_t *tn);              /* the host streaming form restarts at position 0 with zero history */

/* A device-resident range of the capture, conventions as p25fe_resample_dev: d_iq points at owned sample 0 and is 16-byte aligned,
 * only the aligned 16-byte vectors that hold samples [-n_hist, n) are read.  Writes exactly p25fe_n_resample(L, M, abs_first, n)
 * cf32 samples to each of the rows d_out + k * out_stride (complex samples), k < n_out_channels, and nothing beyond them; enqueues
 * on `stream`, synchronises nothing.  The rows are the input of an n_out_channels-channel handle's p25fe_run_dev / p25fe_demod_dev
 * with ch_stride = out_stride; those calls want 16-byte aligned rows, so give d_out that alignment and an even out_stride.  u8 / s16
 * input gives, bit for bit, the cf32 call's output on the converted samples.  P25FE_ERR_ARG: null or misaligned pointer (d_out: 8
 * bytes), unknown format, out_stride < the count, abs_first >= 2^62. */
int p25fe_tune_dev(p25fe_tuner_t *tn, const void *d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first,
                   float *d_out, size_t out_stride, void *stream);

/* Host streaming form, p25fe_resample's semantics: iq holds the capture's next n samples, out is [n_out_channels][cap] cf32, *n_out
 * = samples written per row.  The object keeps the last T - 1 samples and the stream position: any chunking gives the same
 * concatenated output.  P25FE_ERR_CAPACITY (cap too small; *n_out = the count needed) leaves the state untouched; P25FE_ERR_FORMAT
 * when the format differs from the stream's first call (p25fe_tuner_reset starts a new stream).  Synchronous. */
int p25fe_tune(p25fe_tuner_t *tn, const void *iq, int fmt, size_t n, float *out, size_t cap, size_t *n_out);

/* ---- tuner, NCO channels: any frequency offset, for off-raster and ppm tuning (docs/SPEC.md 3.0d) --------------------------------
 * Another kind of the same object.  Channel k has the frequency step_k / 2^32 cycles per INPUT sample, step a signed 32-bit
 * integer (positive: above the capture's centre; resolution fs / 2^32).  The phase is an integer function of the absolute index,
 *     ph = ((uint32)step * (uint32)(n mod 2^32)) mod 2^32,    a = ((ph + 2^23) mod 2^32) >> 24,    r = (int32)(ph - (a << 24)),
 *     t = (float)r * (float)(2 pi / 2^32),  t2 = t * t,  cf = fma(t2, -0.5f, 1.0f),  sf = fma(t2 * t, (float)(-1 / 6), t),
 *     c = fma(-S[a], sf, C[a] * cf),  s = fma(C[a], sf, S[a] * cf)             with C, S = p25fe_tuner_rotator(256, ...),
 * and v_k[n], y_k[m] follow from (c, s) as above (step = 0: v = x).  A channel with step = 0 IS p25fe_resample_dev and a channel
 * with step = num * 2^24, num odd, |num| <= 127, IS the rational channel num / 256, both bit for bit.  The position grid of
 * channel k is lcm(M, 2^32 / gcd(step_k, 2^32)); positions congruent modulo lcm(M, 2^32) give the same bits for every step.
 * Limits: the resampler's and 1 <= n_out_channels <= P25FE_TUNE_MAX_CH; every step value is valid. */

/* step = nearbyint(offset_hz / fs_in_hz * 2^32) in double, ties to even, wrapped to 32 bits (+2^31 becomes -2^31: Nyquist either
 * way); no device needed.  P25FE_ERR_ARG: a null pointer, fs_in_hz = 0, an offset that is not finite, 2 |offset_hz| > fs_in_hz. */
int p25fe_nco_step(uint32_t fs_in_hz, double offset_hz, int32_t *step);
/* (c, s) of the formula above for a step and an absolute index, computed on the host with exactly the kernel's operations; no
 * device needed.  P25FE_ERR_ARG: a null pointer. */
int p25fe_nco_factor(int32_t step, uint64_t n, float cs[2]);
/* p25fe_tuner_create for NCO channels: the same checks in the same order and the same lifetime rules.  The object is used and
 * destroyed with p25fe_tune_dev, p25fe_tune, p25fe_tuner_reset and p25fe_tuner_destroy.  It holds the table, the ONE rotator table
 * of denominator 256 and the channels' steps in device memory. */
int p25fe_nco_create(p25fe_t *h, int32_t L, int32_t M, int32_t T, const float *taps,
                           int32_t n_out_channels, const int32_t *step, p25fe_tuner_t **out);

/* ---- AFC, part 1: an NCO channel's phase offset, and changing its step in a stream (docs/SPEC.md 3.0e) ---------------------------
 * Every NCO channel has a phase offset ph0_k besides its step: ph = (ph0_k + step_k * n) mod 2^32, everything after ph as in 3.0d.
 * p25fe_nco_create makes ph0 = 0 (3.0d, bit for bit); the product is skipped only when step == 0 && ph0 == 0. */

/* ph0_k <- ph0_k + (step_k - step) * abs_at (mod 2^32), then step_k <- step: the mixer's factor at index abs_at is the same bits
 * before and after, so a stream retuned at abs_at has no phase jump there.  Applies to the p25fe_tune_dev / p25fe_tune calls
 * issued after it on `stream`; the channel's device record is rewritten in stream order, so a launch issued before it never sees the
 * new numbers.  A null stream is the handle's, the one p25fe_tune uses, and the update is then also ordered against the default
 * stream, where p25fe_tune_dev with a null stream enqueues.  A call mixes its WHOLE window, the T - 1 history samples
 * included, with the current (step, ph0): the first T - 1 taps after a change see history mixed at a frequency that is off by the
 * change (100 Hz over 84 samples at 2.5 Msps: 0.0034 cycles).  p25fe_tuner_reset leaves steps and offsets alone.
 * P25FE_ERR_ARG: a null or rational tuner, k outside [0, n_out_channels), abs_at >= 2^62; a tuner whose steps a tracking loop
 * (part 3) has updated on the device since the last p25fe_track_read: the host's (step, ph0) are stale then, and nothing is computed
 * from stale numbers. */
int p25fe_afc_set_step(p25fe_tuner_t *tn, int32_t k, int32_t step, uint64_t abs_at, void *stream);
/* channel k's current step and phase offset, as the host holds them; no device is touched.  P25FE_ERR_ARG: a null or rational
 * tuner, k outside the range, a null pointer; a tuner whose host pair is stale (p25fe_afc_set_step). */
int p25fe_afc_get_step(const p25fe_tuner_t *tn, int32_t k, int32_t *step, uint32_t *ph0);
/* (c, s) of 3.0e for a step, a phase offset and an absolute index, with exactly the kernel's operations (ph0 = 0:
 * p25fe_nco_factor); no device needed.  P25FE_ERR_ARG: a null pointer. */
int p25fe_afc_factor(int32_t step, uint32_t ph0, uint64_t n, float cs[2]);

/* ---- AFC, part 2: frequency measure (docs/SPEC.md 3.0f) ----------------------------------------------------------------------------
 * Input: K rows of 240 ksps cf32, the tuner's output rows.  A channel-selective real FIR g[0 .. T) decimating by D (the tuner's
 * own table cuts off at 60 kHz and lets the neighbours 12.5 kHz away through), then the lag-1 product at 240000 / D sps, quantised
 * and summed as integers.  With absolute indices and x[n] = 0 for n < 0:
 *     w[m]  = the resampler's y[m] with L = 1, M = D, T, taps = g            (n_m = m D + D - 1;  w[-1] = 0)
 *     p.re  = fma( w[m].im, w[m-1].im, w[m].re * w[m-1].re)                  (= w[m] conj(w[m-1]))
 *     p.im  = fma(-w[m].re, w[m-1].im, w[m].im * w[m-1].re)
 *     e     = fma( w[m].im, w[m].im,   w[m].re * w[m].re)
 *     Q(v)  = (int32) rintf(clamp(v * 2^shift, -2147483520, 2147483520)),  NaN -> 0
 *     acc.re += Q(p.re);  acc.im += Q(p.im);  acc.pow += Q(e);  acc.n += 1    (64-bit, wrapping)
 * A range owns the m whose n_m lies in it (p25fe_n_resample(1, D, abs_first, n) of them).  Integer sums commute: any split of a
 * stream into ranges with enough history gives the same 32 bytes per channel as one range. */
#define P25FE_AFC_MIN_D 2
#define P25FE_AFC_MAX_D 64
#define P25FE_AFC_MAX_T 512
#define P25FE_AFC_MAX_CH 256
#define P25FE_AFC_MAX_SHIFT 40
typedef struct p25fe_afc p25fe_afc_t;
typedef struct p25fe_afc_acc {
    int64_t re, im;      /* sum of Q(p.re), Q(p.im) */
    int64_t pow;         /* sum of Q(e) */
    uint64_t n;          /* products summed */
} p25fe_afc_acc_t;       /* 32 bytes */

/* The recommended prefilter is D = 10, T = 240, cutoff 7000 Hz.  taps[0 .. T): a Kaiser(beta = 7.0)-windowed sinc of T points with
 * its cutoff at cutoff_hz (at 240 ksps), scaled to sum 1, evaluated in double and rounded once -- p25fe_resampler_design's rule; no
 * device needed.  P25FE_ERR_ARG: D or T outside the limits, a cutoff that is not finite or not in (0, 120000];
 * P25FE_ERR_CAPACITY: cap < T (taps may then be null). */
int p25fe_afc_design(int32_t D, double cutoff_hz, int32_t T, float *taps, size_t cap);
/* A measuring object on h's device for K rows; h must outlive every USE of it (p25fe_afc_destroy alone is safe after
 * p25fe_destroy(h)).  Every argument is checked before any device is touched: P25FE_ERR_ARG unless 2 <= D <= 64, 1 <= T <= 512,
 * 1 <= K <= 256 and the taps are finite. */
int p25fe_afc_create(p25fe_t *h, int32_t D, int32_t T, const float *taps, int32_t K, p25fe_afc_t **out);
void p25fe_afc_destroy(p25fe_afc_t *afc);
/* One range of the K rows d_rows + k * row_stride (complex samples; 8-byte aligned), conventions as p25fe_resample_dev: d_rows
 * points at owned sample 0, n_hist valid samples precede it (n_hist >= T - 1 + D: exact continuation; what is missing reads as
 * zero), abs_first matters modulo D.  ADDS into the caller's d_acc[K] (device, 8-byte aligned): zero the records to open a window.
 * Enqueues on `stream`, synchronises nothing.  P25FE_ERR_ARG: a null or misaligned pointer, shift outside [0, 40],
 * abs_first >= 2^62. */
int p25fe_afc_measure_dev(p25fe_afc_t *afc, const float *d_rows, size_t row_stride, size_t n_hist, size_t n, uint64_t abs_first,
                          int32_t shift, p25fe_afc_acc_t *d_acc, void *stream);
/* A record the caller has copied back -> hz = atan2(im, re) / (2 pi) * 240000 / D (unambiguous to +-120000 / D) and coherence =
 * hypot(re, im) / pow (1: one clean carrier; near 0: noise); both 0 when pow <= 0.  Host only.  P25FE_ERR_ARG: a null pointer, D
 * outside the limits. */
int p25fe_afc_hz(const p25fe_afc_acc_t *acc, int32_t D, double *hz, double *coherence);

/* ---- AFC, part 3: the tracking loop, closed on the device in stream order (docs/SPEC.md 3.0g) ---------------------------------------
 * One kernel launch (k_afc_loop, one thread per channel) reads every channel's record of part 2 and its (step, ph0), and by an
 * integer law writes the next (step, ph0): tune -> measure -> update -> tune is enqueued without the host reading a record.  Per
 * channel, for an update at the absolute INPUT index abs_at, the first of these that applies:
 *     SHORT   n < min_products: nothing changes, the record keeps accumulating;  n_short += 1
 *     REJECT  pow <= 0, or hypot(re, im) / pow < coh_min_q15 / 32768 (compared in integers, 3.0g): the record is zeroed, the step
 *             stays;  n_rejected += 1
 *     APPLY   theta = the angle of (re, im) in 2^-32 turns (a 32-iteration CORDIC on 64-bit integers, 3.0g; within 2^-32 turn);
 *             e = round_half_away(theta L / (M D));  d = clamp((e gain_q16 + 2^15) >> 16, +-max_pull);
 *             step' = clamp(step + d, step_ref +- max_dev), then to int32;  ph0' = ph0 + (step - step') abs_at (mod 2^32), part 1's
 *             rule;  the record is zeroed;  n_applied += 1;  last_theta = theta, last_dstep = d
 * step_ref is the channel's step when the loop was made.  A positive theta (the signal above the channel's centre) raises the step:
 * the sign of step + p25fe_nco_step(fs, hz) on part 2's estimate.  The names do not begin with p25fe_afc_: the loop is an object of
 * its own that holds a tuner and a measure. */
#define P25FE_TRACK_NONE   0      /* status: no update yet */
#define P25FE_TRACK_SHORT  1
#define P25FE_TRACK_REJECT 2
#define P25FE_TRACK_APPLY  3
typedef struct p25fe_track p25fe_track_t;
typedef struct p25fe_track_cfg {
    int32_t shift;           /* Q's shift of the loop's measure, 0 .. P25FE_AFC_MAX_SHIFT (recommended: 24) */
    int32_t coh_min_q15;     /* coherence gate, 0 .. 32768 (recommended: 24576 = 0.75) */
    int32_t gain_q16;        /* loop gain, 1 .. 65536 (recommended: 65536 = 1) */
    int32_t max_pull;        /* largest change of the step in one update, > 0 */
    int32_t max_dev;         /* largest distance of the step from step_ref, > 0 */
    int32_t reserved;        /* 0 */
    uint64_t min_products;   /* products a record needs before it is judged, >= 1 (recommended: half a window's) */
} p25fe_track_cfg_t;         /* 32 bytes */
typedef struct p25fe_track_state {
    int32_t step;            /* the channel's current step ... */
    uint32_t ph0;            /* ... and phase offset (part 1) */
    int32_t last_theta;      /* the last applied angle, 2^-32 turns per D samples at 240 ksps */
    int32_t last_dstep;      /* the last applied change of the step, before the max_dev clamp */
    uint32_t n_applied, n_rejected, n_short;   /* wrapping counts of the outcomes */
    uint32_t status;         /* the last outcome, P25FE_TRACK_* */
} p25fe_track_state_t;       /* 32 bytes */

/* A loop over the NCO tuner tn and the measure afc, which must be of the same handle and have the same channel count; both must
 * outlive every use of it, and a tuner has one loop at a time.  The loop owns zeroed records d_acc[K] and the states d_state[K],
 * made from the (step, ph0) the host holds.  Every argument is checked before any device is touched.  P25FE_ERR_ARG: a null
 * pointer, a rational tuner, a tuner whose host pair is stale (below), different handles or channel counts, a configuration
 * outside the ranges above (reserved != 0 among them). */
int p25fe_track_create(p25fe_tuner_t *tn, p25fe_afc_t *afc, const p25fe_track_cfg_t *cfg, p25fe_track_t **out);
void p25fe_track_destroy(p25fe_track_t *lp);
/* The loop's K open records, synchronously: waits for the device, copies them to `get` (nullable), then overwrites them from `set`
 * (nullable) -- for a caller that reports a window's coherence before the update closes it, or opens a window with records of its
 * own.  P25FE_ERR_ARG: a null loop. */
int p25fe_track_records(p25fe_track_t *lp, p25fe_afc_acc_t *get, const p25fe_afc_acc_t *set);
/* p25fe_afc_measure_dev into the loop's own records with the configuration's shift: same arguments, same refusals. */
int p25fe_track_measure_dev(p25fe_track_t *lp, const float *d_rows, size_t row_stride, size_t n_hist, size_t n, uint64_t abs_first,
                            void *stream);
/* The one launch of k_afc_loop: every channel's update at abs_at, ordered on `stream` behind the measure launches that fed the
 * records and in front of the next p25fe_tune_dev, as p25fe_afc_set_step is (a null stream is treated as there).  Synchronises
 * nothing.  From the first call on, the (step, ph0) the host holds for tn are STALE until p25fe_track_read: p25fe_afc_set_step and
 * p25fe_afc_get_step refuse.  P25FE_ERR_ARG: a null loop, abs_at >= 2^62. */
int p25fe_track_update_dev(p25fe_track_t *lp, uint64_t abs_at, void *stream);
/* The sequencer for a device-resident range of the capture (p25fe_tune_dev's conventions for d_iq, fmt, n_hist, n, abs_first,
 * d_out, out_stride).  The range is cut at the absolute multiples of `window` input samples; for each piece it enqueues
 * p25fe_tune_dev, then the measure of the rows just written, then, where the piece ends on a multiple of `window`, the update at
 * that index.  A trailing partial window is tuned and measured but not updated: the next call continues it.  n_hist_out is the
 * number of valid OUTPUT samples in front of d_out (the measure's T - 1 + D history; what is missing reads as zero).  The rows
 * and states a stream leaves are the same bits for any split of it into calls that keep the alignment; `window` is part of the
 * definition, like D.  Writes exactly p25fe_n_resample(L, M, abs_first, n) samples per row.  Marks the host pair stale as
 * p25fe_track_update_dev does.  P25FE_ERR_ARG: p25fe_tune_dev's refusals for the whole range; window or abs_first not a multiple
 * of the format's 16-byte vector (2 / 4 / 8 samples for cf32 / s16 / u8: multiples of 8 serve every format); window < T - 1 of the
 * tuner or window >= 2^62. */
int p25fe_track_run_dev(p25fe_track_t *lp, const void *d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint64_t window,
                        float *d_out, size_t out_stride, size_t n_hist_out, void *stream);
/* Synchronous: waits for the device, copies the K state records to state_out (nullable) and refreshes the (step, ph0) the host
 * holds for every channel of tn, after which p25fe_afc_set_step / p25fe_afc_get_step work again.  The kernel takes a channel's
 * (step, ph0) from the tuner's device record, so the next update goes on from what a p25fe_afc_set_step after the read left there
 * (step_ref stays).  P25FE_ERR_ARG: a null loop. */
int p25fe_track_read(p25fe_track_t *lp, p25fe_track_state_t *state_out);
/* One channel's update on the host with exactly the kernel's operations (the same function compiled for both); no device needed.
 * acc_out / state_out may alias the inputs.  P25FE_ERR_ARG: a null pointer, a configuration outside the ranges, a ratio L / M
 * outside the resampler's limits, D outside the measure's. */
int p25fe_track_step(const p25fe_track_cfg_t *cfg, int32_t L, int32_t M, int32_t D, int32_t step_ref, const p25fe_afc_acc_t *acc_in,
                     const p25fe_track_state_t *state_in, uint64_t abs_at, p25fe_afc_acc_t *acc_out, p25fe_track_state_t *state_out);
/* hz = last_theta / 2^32 * 240000 / D, for reports.  Host only.  P25FE_ERR_ARG: a null pointer, D outside the limits. */
int p25fe_track_hz(const p25fe_track_state_t *state, int32_t D, double *hz);

/* ---- survey: per-bin power spectrum of a capture, and the active raster channels (docs/SPEC.md 3.0h) -------------------------------
 * The stage in front of the tuner: which raster channels of a capture of any rate carry a signal, and roughly how far off the raster
 * each one is.  A Welch periodogram of ONE capture row (cf32, s16 or u8; 3.1 / 3.0's conversions): windowed length-N DFTs of frames
 * H samples apart, squared magnitudes quantised and summed as 64-bit integers per bin.  With absolute indices and x[n] = 0 for n < 0,
 * frame f ends at n_f = f H + H - 1 and covers [n_f - N + 1, n_f]:
 *     X_f[b] = sum_j w[j] x[n_f - N + 1 + j] e^{-2 pi i b j / N}          b = 0 .. N - 1   (fp32; the factoring is the implementation's)
 *     P_f[b] = fma(X.im, X.im, X.re * X.re)
 *     Q(v)   = (int64) rint(min(v * 2^shift, 2^62)),  NaN -> 0
 *     acc[b] += Q(P_f[b])  (uint64, wrapping);   acc[N] += 1 per frame
 * A range owns the frames whose n_f lies in it.  Integer sums commute: any split of a stream into ranges with N - 1 samples of
 * history gives the same 8 (N + 1) bytes as one range.  Bin b is b fs / N Hz for b < N / 2, else (b - N) fs / N. */
#define P25FE_SCAN_MAX_SHIFT 40
typedef struct p25fe_scanner p25fe_scan_t;
typedef struct p25fe_scan_chan {
    int32_t raster_index;    /* r: the channel is centred r * raster_hz from the capture's centre */
    int32_t reserved;        /* 0 */
    double centre_hz;        /* r * raster_hz */
    double db_over_floor;    /* the channel's power over the median channel's, dB (+inf over a floor of zero) */
    double offset_hz;        /* centroid of the channel's raster cell minus centre_hz */
} p25fe_scan_chan_t;         /* 32 bytes */

/* The designed window: periodic Hann, w[j] = 0.5 - 0.5 cos(2 pi j / N), evaluated in double and rounded once; no device needed.
 * P25FE_ERR_ARG: N is neither 1024 nor 4096; P25FE_ERR_CAPACITY: cap < N (w may then be null). */
int p25fe_scan_window(int32_t N, float *w, size_t cap);
/* A survey object on h's device; h must outlive every USE of it (p25fe_scan_destroy alone is safe after p25fe_destroy(h)).  window:
 * N real values, null for the designed one.  Every argument is checked before any device is touched: P25FE_ERR_ARG unless N is 1024
 * or 4096, 8 <= hop <= N with hop a multiple of 8 that divides N, the window is finite and 0 <= shift <= 40 (recommended: 16 for
 * samples of magnitude up to about 2). */
int p25fe_scan_create(p25fe_t *h, int32_t N, int32_t hop, const float *window, int32_t shift, p25fe_scan_t **out);
void p25fe_scan_destroy(p25fe_scan_t *sc);
/* The host streaming form starts over: position 0, no history, no format, the object's record zeroed.  Waits for the device. */
int p25fe_scan_reset(p25fe_scan_t *sc);
/* One device-resident range of the capture, p25fe_tune_dev's conventions: d_iq points at owned sample 0 (16-byte aligned), n_hist
 * valid samples precede it (n_hist >= N - 1: exact continuation; what is missing reads as zero), abs_first matters modulo hop.  ADDS
 * into the caller's record d_acc[N + 1] (device, 8-byte aligned): zero it to open a survey.  Enqueues on `stream`, synchronises
 * nothing.  P25FE_ERR_ARG: a null or misaligned pointer, an unknown format, abs_first or n >= 2^62. */
int p25fe_scan_dev(p25fe_scan_t *sc, const void *d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint64_t *d_acc,
                   void *stream);
/* The host streaming form, as p25fe_tune: n more samples of the object's stream, which starts at position 0; the last N - 1 samples
 * are carried on the device, the sums go into the object's own record.  Returns when the caller's buffer is free again.
 * P25FE_ERR_FORMAT: the format changed within a stream. */
int p25fe_scan(p25fe_scan_t *sc, const void *iq, int fmt, size_t n);
/* Waits for the device, copies the object's record to acc_out[N + 1] and, with clear != 0, zeroes it. */
int p25fe_scan_read(p25fe_scan_t *sc, uint64_t *acc_out, int clear);
/* A record the caller has copied back -> the active raster channels; host only, works on doubles formed from the record.  Raster
 * index r is eligible when |r raster_hz| + raster_hz / 2 <= fs / 2; pow[r] sums acc[b] over the bins with |f_b - r raster_hz| <=
 * half_bw_hz; the floor is the lower median of pow over the eligible r; r is active iff pow[r] > 0 and pow[r] >= floor *
 * 10^(thr_db / 10); offset_hz is the centroid sum acc[b] f_b / sum acc[b] over |f_b - r raster_hz| <= raster_hz / 2, minus
 * r raster_hz.  Sorted by power, descending; ties go to the smaller r.  *n_out is the number of active channels even when it exceeds
 * cap (the first cap are written); a record of zero frames has none.  Recommended: raster_hz = 12500, half_bw_hz = 4000, thr_db = 20.
 * P25FE_ERR_ARG: a null acc or n_out, a null out with cap > 0, N neither 1024 nor 4096, fs_hz = 0, raster_hz not finite or <= 0,
 * half_bw_hz not finite or < 0, thr_db not finite, a raster of more than 10^6 eligible channels a side. */
int p25fe_scan_channels(const uint64_t *acc, int32_t N, uint32_t fs_hz, double raster_hz, double half_bw_hz, double thr_db,
                        p25fe_scan_chan_t *out, size_t cap, size_t *n_out);

/* ---- survey over time: per-slot spectra in one launch, and keyed intervals (docs/SPEC.md 3.0i) --------------------------------------
 * Which raster channel was keyed from when to when.  Frames, window, X_f, P_f and Q are 3.0h's and the object is a p25fe_scan_t (its
 * N, hop, window, shift and device).  With B >= 1 frames per slot, frame f (ABSOLUTE: the one that ends at f H + H - 1) belongs to
 * slot s = f / B, and a call adds Q(P_f[b]) into row[s - slot0][b] and 1 into row[s - slot0][N] of d_rows[n_rows][row_stride]
 * (uint64, wrapping); words N + 1 .. row_stride - 1 of a row are never written.  Integer sums commute: any split of a stream into
 * calls, inside a slot included, gives the same bytes; the wrapping sum of the rows of a range is p25fe_scan_dev's record of it, and
 * with B = 1 a row is that frame's record. */
typedef struct p25fe_waterfall_key {
    int32_t raster_index;    /* r: the channel is centred r * raster_hz from the capture's centre */
    int32_t reserved;        /* 0 */
    uint64_t first_slot;     /* the interval's first slot (slot0 + its first row) */
    uint64_t n_slots;        /* ... and its length in slots */
    double centre_hz;        /* r * raster_hz */
    double offset_hz;        /* centroid of the channel's raster cell over the interval's rows minus centre_hz */
    double peak_db_over_floor;   /* the largest per-row power over that row's floor, dB (+inf over a floor of zero) */
} p25fe_waterfall_key_t;     /* 48 bytes */

/* The slots the frames of [abs_first, abs_first + n) at this hop fall into: [*first_slot, *first_slot + *n_slots); n_slots = 0 when
 * the range owns no frame.  Host only.  P25FE_ERR_ARG: a null pointer, hop not a multiple of 8 from 8 to 4096 that divides 4096,
 * B = 0 or B > 2^20, abs_first or n >= 2^62. */
int p25fe_waterfall_slots(int32_t hop, uint32_t B, uint64_t abs_first, size_t n, uint64_t *first_slot, size_t *n_slots);
/* One device-resident range, p25fe_scan_dev's conventions, except that abs_first matters in full: ADDS the range's frames into the
 * rows of their slots, row i standing for slot slot0 + i (device, 8-byte aligned; zero them to open a survey).  One launch;
 * enqueues on `stream`, synchronises nothing.  A range that owns no frame returns P25FE_OK and writes nothing.
 * P25FE_ERR_ARG (before any device is touched): p25fe_scan_dev's refusals, B = 0 or B > 2^20, row_stride < N + 1, d_rows null or
 * misaligned, n_rows = 0 while the range owns a frame.  P25FE_ERR_CAPACITY: the range owns a frame whose slot lies outside
 * [slot0, slot0 + n_rows) -- nothing is enqueued and nothing written. */
int p25fe_waterfall_dev(p25fe_scan_t *sc, const void *d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint32_t B,
                        uint64_t slot0, uint64_t *d_rows, size_t n_rows, size_t row_stride, void *stream);
/* The host streaming form.  _open allocates and zeroes [max_rows][N + 1] on the device for slots of B frames from slot 0 (a second
 * open replaces the first; P25FE_ERR_ARG: B = 0 or > 2^20, max_rows = 0 or > 2^20).  p25fe_waterfall is p25fe_scan with the call's
 * frames going into the rows: it shares the object's position, carried history and format rule, so the two may be mixed on one
 * stream, each call's frames going where that call sends them.  P25FE_ERR_CAPACITY: the call would pass the last row; nothing is
 * consumed (the arguments and the format are checked first).  _read waits for the device and copies the *n_rows =
 * min(ceil(frames so far / B), max_rows) rows touched so far (P25FE_ERR_CAPACITY with *n_rows set when cap_rows is smaller).  Frames
 * count whichever call took them and p25fe_scan has no last row: a stream may run past the rows, the count then stays at max_rows
 * and every further p25fe_waterfall that owns a frame is P25FE_ERR_CAPACITY.  p25fe_scan_reset also zeroes the open rows.  Without an open, p25fe_waterfall and
 * _read are P25FE_ERR_ARG. */
int p25fe_waterfall_open(p25fe_scan_t *sc, uint32_t B, size_t max_rows);
int p25fe_waterfall(p25fe_scan_t *sc, const void *iq, int fmt, size_t n);
int p25fe_waterfall_read(p25fe_scan_t *sc, uint64_t *rows_out, size_t cap_rows, size_t *n_rows);
/* Rows the caller has copied back -> keyed intervals; host only.  Eligible raster indices, pow[t][r] and the floor of row t are
 * p25fe_scan_channels' rules applied to every row t with row[t][N] > 0.  Channel r turns on at the first row where pow > 0 and
 * pow >= floor 10^(on_db / 10) and stays on while pow >= floor 10^(off_db / 10); a row of zero frames and the end of the rows end
 * every open interval; intervals shorter than min_slots are dropped.  offset_hz is the centroid over the raster cell of the bins
 * summed as doubles over the interval's rows; peak_db_over_floor the largest per-row ratio.  Sorted by first_slot, then
 * raster_index.  *n_out counts all intervals even beyond cap.  Recommended: on_db = 20, off_db = 14, min_slots = 2.
 * P25FE_ERR_ARG: p25fe_scan_channels' refusals, row_stride < N + 1, off_db > on_db, a number not finite, min_slots = 0. */
int p25fe_waterfall_keys(const uint64_t *rows, size_t n_rows, size_t row_stride, int32_t N, uint32_t fs_hz, uint64_t slot0,
                         double raster_hz, double half_bw_hz, double on_db, double off_db, uint32_t min_slots,
                         p25fe_waterfall_key_t *out, size_t cap, size_t *n_out);

/* ---- tuner, cuts: keyed intervals cut out of one capture in a single launch (docs/SPEC.md 3.0j) -------------------------------------
 * A cut {abs_first, n, step, ph0} owns the absolute input samples [abs_first, abs_first + n); (step, ph0) is an NCO channel's pair
 * (3.0d / 3.0e).  Its output is, bit for bit, the slice [m0, m0 + cnt) of the row p25fe_tune_dev writes for an NCO channel with that
 * (step, ph0) over the call's whole range: m0 = p25fe_n_resample(L, M, call.abs_first, cut.abs_first - call.abs_first), cnt =
 * p25fe_n_resample(L, M, cut.abs_first, cut.n).  A cut that begins inside the call's range therefore reads the real samples in front
 * of it (what lies before the call's -n_hist reads as zero), the mixer's phase is a function of the absolute index alone, and
 * splitting a cut at any sample -- within a call, or across two calls of a stream, the second with n_hist >= T - 1 -- gives the same
 * concatenated outputs.  A cut with step = 0 and ph0 = 0 is p25fe_resample_dev's slice; a cut with cnt = 0 writes nothing. */
#define P25FE_CUTS_MAX 4096
typedef struct p25fe_cut {
    uint64_t abs_first, n;   /* the samples the cut owns; both < 2^62 */
    int32_t step;            /* the NCO's step (p25fe_nco_step) ... */
    uint32_t ph0;            /* ... and phase offset (3.0e; 0 for a channel tuned from the start of the stream) */
} p25fe_cut_t;               /* 24 bytes */
typedef struct p25fe_cuts p25fe_cuts_t;

/* keys -> cuts, host only: cut j is key j (p25fe_waterfall_keys' output for a survey of N, hop, B at fs_hz).  Frame f of the survey
 * spans samples [f hop + hop - N, f hop + hop - 1], so key j owns [first_slot B hop + hop - N - margin, (first_slot + n_slots) B hop
 * + hop - 1 + margin], clipped to [range_first, range_first + range_n) (empty after clipping: n = 0, abs_first at the range's nearer
 * end); step = p25fe_nco_step(fs_hz, centre_hz + offset_hz), ph0 = 0.  *n_out = n_keys.  P25FE_ERR_ARG: a null n_out, null keys with
 * n_keys > 0, null out with cap > 0, N neither 1024 nor 4096, hop not a multiple of 8 from 8 to N that divides N, B = 0 or B > 2^20,
 * fs_hz = 0, margin, range_first or range_n >= 2^62, a key whose frequency p25fe_nco_step refuses (past Nyquist, not finite).
 * P25FE_ERR_CAPACITY: cap < n_keys (*n_out is set, nothing written). */
int p25fe_cuts_from_keys(const p25fe_waterfall_key_t *keys, size_t n_keys, int32_t N, int32_t hop, uint32_t B, uint32_t fs_hz,
                         uint64_t margin, uint64_t range_first, uint64_t range_n, p25fe_cut_t *out, size_t cap, size_t *n_out);
/* Checks, plans and uploads a list of cuts (synchronous).  tn must be an NCO tuner: its table, rotator, device and u8 conversion are
 * used, its own channels are not.  counts_out (nullable) [n_cuts] = cnt_j; *max_count (nullable) = their maximum.  tn must outlive
 * every USE of the object (p25fe_cuts_destroy alone is safe after the tuner is gone).  Every argument is checked before any device is
 * touched.  P25FE_ERR_ARG: a null out or cuts, n_cuts = 0 or > P25FE_CUTS_MAX, a cut with abs_first or n >= 2^62, a null or rational
 * tuner, more than 2^31 - 1 workgroups in total. */
int p25fe_cuts_create(p25fe_tuner_t *tn, const p25fe_cut_t *cuts, size_t n_cuts, size_t *counts_out, size_t *max_count,
                      p25fe_cuts_t **out);
void p25fe_cuts_destroy(p25fe_cuts_t *ct);
/* p25fe_tune_dev's conventions for d_iq / fmt / n_hist / n / abs_first / stream.  Writes exactly cnt_j cf32 samples to d_out + j *
 * out_stride (complex samples) and nothing else; ONE launch; synchronises nothing.  The rows have different lengths and
 * p25fe_run_dev on an n_cuts-channel handle needs rows of one length: nothing is written beyond cnt_j, so ZERO d_out first and run
 * the rows at max_count -- a zero tail demodulates to zero baseband.  Give d_out 16-byte alignment and an even out_stride for that.
 * P25FE_ERR_ARG (before any device is touched, nothing enqueued): p25fe_tune_dev's refusals, a cut not inside [abs_first, abs_first +
 * n), out_stride < max_count (or >= 2^50). */
int p25fe_cuts_dev(p25fe_cuts_t *ct, const void *d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first,
                   float *d_out, size_t out_stride, void *stream);

/* ---- survey over time, keys on the device: the keyed intervals computed where the rows are (docs/SPEC.md 3.0k) -----------------------
 * p25fe_waterfall_keys is the definition; an object of this section returns the same bytes -- the count and the whole 48-byte
 * records -- for the same rows and parameters without the rows leaving the device.  The object is the plan of one raster over a
 * p25fe_scan_t's N on its device; a run enqueues a fixed number of launches and leaves a few raw records on the device; _read
 * waits for the run, copies them back and finishes them on the host (the centroid's quotient and 10 log10 of the largest ratio).
 * The caller orders the calls on one object, as it orders the rows. */
#define P25FE_KEYS_MAX_CHANNELS 4096
typedef struct p25fe_keys p25fe_keys_t;
/* Builds the raster (p25fe_waterfall_keys' own), uploads it and allocates all scratch; synchronous.  sc must outlive every USE of
 * the object (p25fe_keys_destroy alone is safe after it is gone).  Every argument is checked before any device is touched.
 * P25FE_ERR_ARG: p25fe_waterfall_keys' refusals, a null sc or out, max_rows = 0 or > 2^20, max_keys = 0 or > 2^20.
 * P25FE_ERR_CAPACITY (limits of the device form; the host function has none): more than P25FE_KEYS_MAX_CHANNELS eligible channels,
 * max_rows * (channels + 1) > 2^28 words of scratch.  A raster with no eligible channel is a valid object whose runs find no key. */
int p25fe_keys_create(p25fe_scan_t *sc, uint32_t fs_hz, double raster_hz, double half_bw_hz, double on_db, double off_db,
                      uint32_t min_slots, size_t max_rows, size_t max_keys, p25fe_keys_t **out);
void p25fe_keys_destroy(p25fe_keys_t *kp);
/* One run over d_rows[n_rows][row_stride] (device, 8-byte aligned; p25fe_waterfall_dev's rows, row i standing for slot slot0 + i):
 * four launches on `stream`, a memset among them, whatever n_rows and the raster are; synchronises nothing, reads nothing back and
 * never writes d_rows.  The run replaces the object's previous result; n_rows = 0 is P25FE_OK and a result of no key.
 * P25FE_ERR_ARG (before any device is touched): d_rows null or misaligned, row_stride < N + 1.  P25FE_ERR_CAPACITY: n_rows >
 * max_rows. */
int p25fe_keys_dev(p25fe_keys_t *kp, const uint64_t *d_rows, size_t n_rows, size_t row_stride, uint64_t slot0, void *stream);
/* The same run over the rows of sc's open host-streaming waterfall: the rows touched so far (p25fe_waterfall_read's count), slot0 =
 * 0, on the handle's stream behind the p25fe_waterfall calls made so far.  P25FE_ERR_ARG: no open waterfall. */
int p25fe_keys_stream(p25fe_keys_t *kp);
/* Waits for the last run (an event recorded behind it) and returns its keys with p25fe_waterfall_keys' contract for out, cap and
 * n_out, sorted by first_slot, then raster_index.  One difference: a run that found more than max_keys intervals is
 * P25FE_ERR_CAPACITY with *n_out the true count and nothing written -- the device emits in no particular order, so there is no
 * sorted prefix.  Before any run: P25FE_OK and no key. */
int p25fe_keys_read(p25fe_keys_t *kp, p25fe_waterfall_key_t *out, size_t cap, size_t *n_out);

/* stages 6-7 on device baseband.  d_bb points at the first owned sample; n_hist_bb valid
 * samples precede it; abs_bb0 is its absolute index; d_anchor_in (nullable = no lock) is the
 * carry-in per channel.  d_result[c] is filled per channel.
 * dibit_stride (here and in every *_dev call) is the row stride AND the per-channel capacity of d_dibits: a receiver
 * that re-anchors on every sync word follows the transmitter's symbol clock, so a range of n baseband samples can hold
 * more than n / 10 dibits (n / 6 at most, under back-to-back detections).  d_result[c].n_dibits is always the exact
 * count; dibits past the capacity are not stored (n_dibits > dibit_stride tells the caller so). */
int p25fe_slice_dev(p25fe_t *h, const float *d_bb, size_t bb_stride, size_t n_hist_bb, size_t n_bb,
                    uint64_t abs_bb0, const p25fe_anchor_t *d_anchor_in, uint8_t *d_dibits, size_t dibit_stride,
                    int64_t *d_sync_pos, uint64_t *d_sync_dibit, size_t sync_stride, p25fe_result_t *d_result,
                    void *stream);

/* stages 1-7 from a fresh stream state over a resident capture (BASELINE.json config 2/4). */
int p25fe_run_dev(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n, uint8_t *d_dibits,
                  size_t dibit_stride, p25fe_result_t *d_result, void *stream);

/* The same pass with the two halves of the path on two streams, for a SEQUENCE of captures (or chunks of separate
 * tuners): stages 1-5 (K1, which is what loads the GPU) run on `stream`, stages 6-7 (sync detect, scan, slicer: three
 * short, latency-bound launches) on a stream of the handle, so that they overlap the NEXT call's K1 -- the way
 * DemodTask and RecvTask are two threads joined by a channel (src/demod.rs:116, src/recv.rs:140-150: the demodulator
 * is already filling the next chunk while the receiver works on the previous one).  The receiver's scratch is double
 * buffered; call i + 2 waits on the device for call i's receive kernels.
 * d_dibits / d_result of a call are complete only after p25fe_join_dev has been enqueued on a stream and that stream
 * has reached it (or after any other call on this handle that uses the receiver, which joins first).  Consecutive calls
 * may name the same output buffers (their receive kernels run in call order on one stream); d_iq must stay unchanged
 * until `stream` has passed the call (K1 is the only reader). */
int p25fe_run_dev_pipelined(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n, uint8_t *d_dibits,
                            size_t dibit_stride, p25fe_result_t *d_result, void *stream);
/* make `stream` wait for every receive kernel that p25fe_run_dev_pipelined has enqueued so far */
int p25fe_join_dev(p25fe_t *h, void *stream);

/* Time-sharded capture (BASELINE.json config 5): shard = owned range [abs0, abs0 + n) with
 * n_hist >= p25fe_shard_halo() samples of left context in memory (or n_hist == abs0 for the
 * first shard).  Pass 1 demodulates, detects frame syncs and fills d_result[c] with the
 * shard summary (first_event, n_dibits_after_first, anchor_out) assuming no carry-in.  The
 * caller exchanges summaries (all_gather of a few bytes), resolves each shard's carry-in
 * anchor with p25fe_shard_resolve on the host, then pass 2 slices.
 * ORDERING: pass 2 works on the baseband and the detections that pass 1 left in the handle's
 * scratch.  No other call that demodulates or slices (p25fe_run_*, p25fe_demod_*, p25fe_slice*,
 * another shard's pass 1) may come between a shard's pass 1 and its pass 2 on the same handle:
 * any of them invalidates the shard context and pass 2 then returns P25FE_ERR_ARG (as it does
 * after a failed pass 1) instead of slicing stale data. */
size_t p25fe_shard_halo(void);
int p25fe_shard_pass1(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                      uint64_t abs0, p25fe_result_t *d_result, void *stream);
int p25fe_shard_pass2(p25fe_t *h, const p25fe_anchor_t *d_anchor_in, uint8_t *d_dibits, size_t dibit_stride,
                      p25fe_result_t *d_result, void *stream);
/* The same pass 1 in two launches, so that the exchange of the filter-state overlap hides behind K1: _main enqueues
 * the front end for every part of the shard whose input lies inside the OWNED samples (all but the first ~900
 * baseband samples) and may run while the left neighbour's halo is still on the wire; _finish (same arguments, after
 * the halo has arrived in front of d_iq) enqueues the remaining head, the sync detection and the scan, and fills
 * d_result.  p25fe_shard_pass1 == _main + _finish. */
int p25fe_shard_pass1_main(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                           uint64_t abs0, void *stream);
int p25fe_shard_pass1_finish(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                             uint64_t abs0, p25fe_result_t *d_result, void *stream);
/* The head alone (same arguments, after the halo has arrived), so that it can run on ANOTHER stream beside the main launch
 * -- the stream the halo arrives on: the two launches share no byte of their outputs.  p25fe_shard_pass1_finish then only
 * enqueues the sync detection and the scan, and needs NO stream-level wait for the head: the head launch's last workgroup
 * publishes a flag word, and the detection workgroups whose tiles read the head's planes poll it (a cross-stream event wait
 * costs 10 - 20 us of idle GPU) -- for at most 2 s of device wall clock, after which they give up and p25fe_shard_head_check
 * reports P25FE_ERR_TIMEOUT (a stalled peer must not hang the queue).  Making _finish's stream wait for the head's with an
 * event as well is harmless.  Optional: without this call _finish launches the head itself. */
int p25fe_shard_pass1_head(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                           uint64_t abs0, void *stream);
/* After the stream(s) of a step whose head ran through p25fe_shard_pass1_head have been synchronised: P25FE_OK, or P25FE_ERR_TIMEOUT if a
 * detection workgroup gave up waiting for the head's flag (2 s of device wall clock: the stream the head was on never delivered it, e.g. a
 * halo exchange whose peer died) -- the results of that step, and of every later one on this handle, are not to be used. */
int p25fe_shard_head_check(p25fe_t *h);
/* The whole front end of pass 1 in ONE launch (main + head: the halo must be in memory), nothing else; p25fe_shard_pass1_finish
 * then only enqueues the sync detection and the scan.  p25fe_shard_pass1 == _k1 + _finish. */
int p25fe_shard_pass1_k1(p25fe_t *h, const void *d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                         void *stream);
/* Steps one behind the other (p25fe_shard_step_pipelined): between _begin and _end the shard passes work on the next of up to four
 * scratch sets (p25fe_run_dev_pipelined rotates through two of them) and do not wait for the handle's receive stream -- they are
 * its work.  _begin makes `stream` (where pass 1's front end is about to overwrite that set's planes) wait for the passes that read
 * it four steps back and returns the receive stream in *rx_stream; p25fe_shard_pass1_k1 / _main(..., stream) then makes the receive
 * stream wait for its launch; every later pass of the step (_finish, pass 2, the exchanges between them) is enqueued on the receive
 * stream or on streams that wait for it.  _end(h, last) records "this step's passes are done" on `last` (NULL: the receive stream)
 * and marks it as pending: p25fe_join_dev makes a stream wait for it, every non-pipelined entry point does so by itself. */
int p25fe_shard_pipe_begin(p25fe_t *h, void *stream, void **rx_stream);
int p25fe_shard_pipe_end(p25fe_t *h, void *last_stream);
/* the handle's receive stream (created on first use), without starting a step: for a host that wants to check its own streams against it
 * (p25fe_streams_share_queue; libp25fe_rccl.so's p25fe_shard_create / p25fe_shard_prepare do) */
int p25fe_rx_stream(p25fe_t *h, void **rx_stream);

/* DIAGNOSTIC (tests/test_gpu_planes.py; no receiver needs it, additive: the ABI version stays): the blocked polyphase baseband and its
 * sign words that the most recent scratch-using call on the handle wrote (K1 of the fused calls, the planarising kernels of
 * p25fe_slice_dev / p25fe_slice) or read (a shard's later passes), copied device to device on `stream`, channel c's floats to
 * d_f + c * f_stride and its words to d_bits + c * bits_stride.  The layout is the one described at PLPAD / planar_index in
 * p25rx_amd/csrc/p25fe_kernels.hip: sample m of the call's range sits at position p = m + 320 + look (look: 0 with the fixed clock,
 * P25FE_CLK_LOOKAHEAD with the tracking ones), plane p % 10, symbol i = p / 10; its float at (i / 32) * 320 + (p % 10) * 32 + i % 32,
 * its raw sign bit at bit i % 32 of word (i / 32) * 10 + p % 10.  n_bb is the call's baseband length per channel (0 counts as 1); _size
 * gives the floats and words per channel it stands for.  P25FE_ERR_ARG: null pointers, no such call yet, a length whose geometry is not
 * the one that call sized the scratch for, strides below _size's figures.  The copy is ordered on `stream` only: give it the stream of
 * the call (the host-pointer calls have finished when they return); which scratch set that call used is remembered by the handle. */
int p25fe_debug_planes_size(const p25fe_t *h, size_t n_bb, size_t *n_floats, size_t *n_words);
int p25fe_debug_planes_dev(p25fe_t *h, size_t n_bb, float *d_f, size_t f_stride, uint32_t *d_bits, size_t bits_stride, void *stream);

/* Host-side combine: summaries[r] for r = 0..n_shards-1 in time order (one channel) ->
 * anchor_in[r] (n_shards entries) and dibit_offset[r] (n_shards + 1 entries: shard r's dibits occupy
 * [dibit_offset[r], dibit_offset[r + 1]) of the whole stream, the last entry is the total).
 * Pure integer/struct logic, no device work.  symbol_clock: the handles' p25fe_config_t.symbol_clock. */
int p25fe_shard_resolve(const p25fe_result_t *summaries, const uint64_t *shard_bb0, const uint64_t *shard_bb_n,
                        size_t n_shards, int symbol_clock, p25fe_anchor_t *anchor_in, uint64_t *dibit_offset);

/* Same combine on the device (one tiny kernel, no host synchronisation): all arrays are device pointers, e.g. the
 * all-gathered summaries; writes n_shards anchors and n_shards + 1 offsets; pass d_anchor_in + rank to p25fe_shard_pass2. */
int p25fe_shard_resolve_dev(p25fe_t *h, const p25fe_result_t *d_summaries, const uint64_t *d_shard_bb0,
                            const uint64_t *d_shard_bb_n, size_t n_shards, p25fe_anchor_t *d_anchor_in,
                            uint64_t *d_dibit_offset, void *stream);

/* Pass 2 with the combine on the device and INSIDE the pass: d_summaries = the n_shards pass-1 summaries in time order
 * (the all-gathered records, device memory), `rank` = this handle's shard.  One-channel handles.  With the fixed-stride
 * receiver and no lock drops inside the shard this is ONE launch: no second scan and no resolve kernel -- every slicer
 * workgroup derives its carry-in from the summaries and applies it in closed form (ShardFix, p25fe_recv.hip); otherwise it
 * enqueues p25fe_shard_resolve_dev + p25fe_shard_pass2.  Also written: d_anchor_in[n_shards] and
 * d_dibit_offset[n_shards + 1] (what p25fe_shard_resolve_dev writes), *d_result = this shard's final record.
 * d_dibits_dup (nullable): a second destination of every dibit with the same row layout -- rank 0's shard starts at offset
 * 0 of the capture's ordered stream, so it can slice straight into it.
 * Same ordering rule as p25fe_shard_pass2: it follows its shard's pass 1 on this handle. */
int p25fe_shard_pass2_dev(p25fe_t *h, const p25fe_result_t *d_summaries, const uint64_t *d_shard_bb0,
                          const uint64_t *d_shard_bb_n, size_t n_shards, size_t rank, p25fe_anchor_t *d_anchor_in,
                          uint64_t *d_dibit_offset, uint8_t *d_dibits, size_t dibit_stride, uint8_t *d_dibits_dup,
                          p25fe_result_t *d_result, void *stream);

/* Dibit gather, receiving side (BASELINE.json config 5: "RCCL ... carrying ... the reduced dibit stream"): after an
 * all-gather of the shards' dibit buffers (each `cap` bytes, shard r at d_gathered + r * cap, its first
 * dibit_offset[r + 1] - dibit_offset[r] bytes valid) write the contiguous stream to d_out[0 .. dibit_offset[n_shards]).
 * d_dibit_offset: the n_shards + 1 entries of p25fe_shard_resolve_dev.  The consumer is the ordered stream that
 * RecvTask feeds into MessageReceiver (src/recv.rs:148-150). */
int p25fe_shard_compact_dev(p25fe_t *h, const uint8_t *d_gathered, size_t cap, const uint64_t *d_dibit_offset,
                            size_t n_shards, uint8_t *d_out, size_t out_cap, void *stream);
/* the same for shards first_shard .. n_shards - 1 only (first_shard = 1: rank 0 has sliced its own shard into d_out already,
 * p25fe_shard_pass2_dev's d_dibits_dup; first_shard == n_shards: nothing to do) */
int p25fe_shard_compact_from_dev(p25fe_t *h, const uint8_t *d_gathered, size_t cap, const uint64_t *d_dibit_offset,
                                 size_t first_shard, size_t n_shards, uint8_t *d_out, size_t out_cap, void *stream);

/* Do two streams of this process share a HARDWARE queue (*shared = 1) -- i.e. do their kernels run one after the other whatever the
 * streams say?  HIP multiplexes the streams of one priority level onto four queues in creation order; the pipelined calls of this
 * library only overlap what they promise when their streams sit on different queues ("Which stream to pass").
 * Synchronises both streams and runs a 1-thread probe on each (< 1 ms); p25fe_shard_create's side stream is chosen with it. */
int p25fe_streams_share_queue(p25fe_t *h, void *stream_a, void *stream_b, int *shared);

/* Network identifier that follows each frame sync (next row after the dibits, SURVEY.md section 8f: what
 * p25::MessageReceiver reports as MessageEvent::PacketNID, src/recv.rs:216-222, consumed by
 * ReceiverPolicy::handle_nid, src/policy.rs:92).  64 bits = BCH(63,16,23) code word (NAC 12 bits, DUID 4 bits)
 * + 1 extra bit, 32 dibits after the sync word with a status symbol interleaved (docs/SPEC.md 3.9). */
typedef struct p25fe_nid {
    uint64_t raw;                        /* received 64 bits, first transmitted bit in bit 63 */
    int64_t sync_pos;                    /* copied from the sync event (0 if d_sync_pos is null) */
    uint16_t nac;                        /* network access code of the nearest code word */
    uint8_t duid;                        /* data unit id */
    uint8_t n_errors;                    /* Hamming distance to that code word */
    int32_t valid;                       /* 1 decoded (<= 11 bit errors), 0 undecodable, -1 dibit stream ends inside the NID */
} p25fe_nid_t;

/* d_dibits / n_dibits: one channel's dibit stream (as written by p25fe_run_dev / p25fe_slice_dev); d_sync_dibit[k]:
 * index of the first dibit after sync word k (the sync_dibit output of p25fe_slice_dev); d_sync_pos nullable.
 * Writes n_sync records.  All device pointers; enqueued on `stream`. */
int p25fe_nid_dev(p25fe_t *h, const uint8_t *d_dibits, size_t n_dibits, const uint64_t *d_sync_dibit,
                  const int64_t *d_sync_pos, size_t n_sync, p25fe_nid_t *d_out, void *stream);

/* Host-buffer form (the file-driven harness: p25fe_replay -j): copies the stream and the events to the device, runs the
 * same kernel, copies the n_sync records back; synchronous. */
int p25fe_nid(p25fe_t *h, const uint8_t *dibits, size_t n_dibits, const uint64_t *sync_dibit, const int64_t *sync_pos,
              size_t n_sync, p25fe_nid_t *out);

/* The same for a whole channel batch without a host round trip: channel c's stream is d_dibits + c * dibit_stride
 * with d_result[c].n_dibits dibits, its events d_sync_dibit / d_sync_pos + c * sync_stride (the outputs of
 * p25fe_slice_dev), min(d_result[c].n_sync, sync_stride) of them; records go to d_out + c * sync_stride. */
int p25fe_nid_batch_dev(p25fe_t *h, const uint8_t *d_dibits, size_t dibit_stride, const p25fe_result_t *d_result,
                        const uint64_t *d_sync_dibit, const int64_t *d_sync_pos, size_t sync_stride,
                        p25fe_nid_t *d_out, void *stream);

/* Polyphase channeliser (no reference counterpart -- the reference tunes ONE channel,
 * src/sdr.rs:64-65): one cf32 capture at 2.4 Msps -> P25FE_CHZ_CHANNELS = 192 channels on the 12.5 kHz raster
 * (channel c centred c * 12.5 kHz above the capture's centre, c >= 96 below it), each at 240 ksps -- the stream
 * stage 1 (src/demod.rs:74-84) would deliver for a tuner on that channel, ready for p25fe_demod_dev / p25fe_run_dev
 * of a 192-channel handle (ch_stride = out_stride).  docs/SPEC.md 3.11; channel 0 equals p25fe_predecim_dev.
 * d_iq: owned sample 0 (16-byte aligned), n_hist valid samples before it (>= 79 for exact continuation), abs0 its
 * absolute index (fixes the decimation grid and the mixer phase, so any chunking gives the same stream);
 * d_out: [192][out_stride] cf32, n_out = p25fe_n_predecim(abs0, n) samples per channel; rows are written in whole
 * 64-sample tiles, so out_stride >= n_out rounded up to 64 (P25FE_ERR_ARG otherwise) and row samples >= n_out are
 * unspecified.  The handle only supplies the device. */
#define P25FE_CHZ_CHANNELS_ABI 192
int p25fe_channelise_dev(p25fe_t *h, const float *d_iq, size_t n_hist, size_t n, uint64_t abs0, float *d_out,
                         size_t out_stride, void *stream);
/* ... on a u8 or s16 capture (docs/SPEC.md 3.11; formats, conversion, alignment and errors as p25fe_predecim_fmt_dev): bit for
 * bit p25fe_channelise_dev's output on the converted samples; here the handle also supplies the u8 conversion.
 * fmt = P25FE_FMT_CF32 is p25fe_channelise_dev itself. */
int p25fe_channelise_fmt_dev(p25fe_t *h, const void *d_iq, int fmt, size_t n_hist, size_t n,
                             uint64_t abs_first /* = p25fe_channelise_dev's abs0 */, float *d_out, size_t out_stride, void *stream);

/* Per-channel observability record: what the reference pushes to its hub as
 * HubEvent::UpdateSignalPower (src/demod.rs:95-101, "sigPower" src/hub.rs:344) and HubEvent::UpdateStats
 * (src/recv.rs:162-165, 212-215; "updateStats" src/hub.rs:401-402), restricted to what exists on this path: the
 * "bch" row of serialize_stats (src/hub.rs:559) -- p25::stats::CodeStats as serialised by serialize_code_stats
 * (src/hub.rs:574-581: totalWords = words, errWords = errs, totalSymbols = words * size, fixedSymbols = fixed) --
 * plus the receiver's lock state.  The other code rows (Golay, Hamming, RS, Viterbi) belong to the out-of-scope
 * frame decoder. */
typedef struct p25fe_code_stats {
    uint64_t words;                      /* code words seen (NIDs complete in the dibit stream) */
    uint64_t errs;                       /* of those, undecodable (more than 11 bit errors) */
    uint64_t fixed;                      /* corrected bits over the decodable words */
    uint32_t size;                       /* symbols per word: 63 */
    uint32_t reserved;
} p25fe_code_stats_t;

typedef struct p25fe_chan_stats {
    float sig_power_dbm;                 /* copied from d_power_dbm[c]; NaN when not supplied */
    int32_t locked;                      /* an anchor is in force at the end of the range */
    uint64_t n_dibits;
    uint64_t n_sync;                     /* detections decided in the range */
    int64_t last_sync_pos;               /* s of the last detection, -1 if none */
    p25fe_code_stats_t bch;
} p25fe_chan_stats_t;

/* d_result[C] from p25fe_slice_dev / p25fe_run_dev; d_nid[C][sync_stride] from p25fe_nid_batch_dev (nullable: bch
 * stays zero); d_power_dbm[C] from p25fe_demod_dev (nullable).  Writes d_stats[C]. */
int p25fe_chan_stats_dev(p25fe_t *h, const p25fe_result_t *d_result, const p25fe_nid_t *d_nid, size_t sync_stride,
                         const float *d_power_dbm, p25fe_chan_stats_t *d_stats, void *stream);

/* Measurement hook for bench.py: when enabled, p25fe_run_dev / p25fe_shard_pass1 record HIP
 * events on the caller's stream around each kernel (K1 front end, K2 sync detect, K3 scan, K4 slice);
 * p25fe_shard_pass2 records its own slot with K3 and K4 only (ms[0], ms[1] of that slot read as 0).
 * p25fe_profile_read synchronises those events and returns the summed milliseconds per kernel over the
 * kept slots (at most the last 64) and, in *n_calls, how many of those slots ran K1 (= passes of the path).
 * on = 1: events around every kernel (five records per call); on = 2: around K1 only (two records; ms[1..3] read
 * as 0) -- the records themselves cost ~4 us each between kernels, which matters for a 0.28 ms step; on = 3: as 2, but
 * only every 8th call carries the two records (the kept slots then span the last 512 calls). */
int p25fe_profile_enable(p25fe_t *h, int on);
int p25fe_profile_read(p25fe_t *h, double ms[4], uint64_t *n_calls);

/* Number of baseband samples produced by n input samples starting at absolute index abs0 -- with the default decimator
 * phase (p25fe_config_t.decim_phase = 4), and with the handle's. */
size_t p25fe_n_baseband(uint64_t abs0, size_t n);
size_t p25fe_n_baseband_h(const p25fe_t *h, uint64_t abs0, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* P25FE_H */
