// p25fe_api.hip -- host side of the C ABI declared in include/p25fe.h.
//
// Owns device scratch and the stream state that DemodTask / MessageReceiver keep in their
// structs (src/demod.rs:25-40, src/recv.rs:47), and launches the kernels of p25fe_kernels.hip.
// No CPU compute path exists here: every entry point either runs the HIP kernels or fails.
#include "p25fe_kernels.hip"

#include <hip/hip_ext.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <new>
#include <utility>
#include <string>
#include <vector>

#include "p25fe_jit.h"

using namespace p25k;

namespace {

constexpr size_t BBPAD = 256;        // >= HIST_BB (240) + the tracking clock's lookahead, multiple of 4
constexpr size_t SHARD_HALO = 2560;                     // samples (20 KB of cf32): K1 recomputes one block (320 + 2) of baseband history in front of a
                                                       // shard and needs up to 127 decimator outputs (64-tap post-discriminator and channel filters;
                                                       // 160 when a segment recomputes its halo) and 63 samples in front of that
static_assert(SHARD_HALO >= (size_t)(DEC * (PLPAD + CLK_L + 160) + TMAX) && 160 >= TMAX + TMAX - 1 && SHARD_HALO % 8 == 0, "shard halo");
constexpr uint32_t STATE_MAGIC = 0x50323546u;          // "P25F"

// device memory, freed with its owner
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
// ... holding elements of one type: sized by count, read without a cast
template <class T> struct DevArr {
    DevBuf buf;
    hipError_t ensure(size_t count) { return buf.ensure(count * sizeof(T)); }
    T* get() const { return static_cast<T*>(buf.p); }
};

// pinned host memory that the device reads and writes in place (the streaming entry points' staging and result buffers)
struct PinBuf {
    void* p = nullptr;          // host view
    void* dp = nullptr;         // device view of the same bytes
    size_t cap = 0;
    PinBuf() = default; PinBuf(const PinBuf&) = delete; PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        // coherent (fine-grained): the chunk kernels' results and completion word must reach the polling host while the
        // kernel is still running, not at its end
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocCoherent | hipHostMallocMapped);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostMalloc(&p, want, hipHostMallocDefault); }
        if (e != hipSuccess) { p = nullptr; return e; }
        e = hipHostGetDevicePointer(&dp, p, 0);
        if (e != hipSuccess) { (void)hipHostFree(p); p = dp = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = dp = nullptr; cap = 0; }
};

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// carve `bytes` (rounded up to 64) out of a pinned arena; returns the host pointer, *dev = the device view
struct Arena {
    char* hp; char* dp; size_t off = 0;
    Arena(const PinBuf& b) : hp(static_cast<char*>(b.p)), dp(static_cast<char*>(b.dp)) {}
    template <class T> T* take(size_t count, T** dev)
    {
        T* r = reinterpret_cast<T*>(hp + off);
        *dev = reinterpret_cast<T*>(dp + off);
        off += round_up(count * sizeof(T), 64);
        return r;
    }
    template <class T> T* take(size_t count) { T* dev; return take<T>(count, &dev); }     // ... for what only the host side names
};

// Kernel launch with optional events ATTACHED TO THE DISPATCH (hipExtLaunchKernelGGL): the start / stop events are
// signalled by the kernel's own AQL packet, where hipEventRecord would put one more barrier packet (and its release) in
// front of the next kernel of the stream.
template <class... Args, class... Act>
inline void launch_ev(void (*kern)(Args...), dim3 grid, dim3 block, size_t lds, hipStream_t st, hipEvent_t e0, hipEvent_t e1,
                      Act... args)
{
    if (e0 || e1) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, st, e0, e1, 0u, Args(args)...);
    else hipLaunchKernelGGL(kern, grid, block, lds, st, Args(args)...);
}
inline bool fmt_known(int fmt) { return fmt == P25FE_FMT_CF32 || fmt == P25FE_FMT_U8 || fmt == P25FE_FMT_S16; }
inline size_t fmt_bytes(int fmt) { return (size_t)fmt_bps(fmt); }  // bytes per complex sample: 8 / 2 / 4 (p25fe_kernels.hip)
// samples a channel stride must be a multiple of, so that every channel's owned sample 0 is 16-byte aligned
inline size_t fmt_stride_unit(int fmt) { return 16 / fmt_bytes(fmt); }

static_assert(BBPAD == (size_t)TAILN && BBPAD >= (size_t)HIST_BB + CLK_L, "baseband tail kept between calls");

constexpr int MAX_LANES = 4;
// ShardCtx::flag: words 0 / 1 the head segment's flag and ticket, 2 / 3 the queue probe's pair, 4 "a detection gave up waiting for the head"
constexpr int SH_FLAG_WORDS = 8, SH_FLAG_ERR = 4;
constexpr int PROF_RING = 64, PROF_SAMPLE = 8;

// One set of the receiver's scratch: K1's planes and everything K2 .. K4 hand each other.  A receive chain writes nothing else but the caller's
// outputs and the per-handle buffers listed at struct p25fe, so chains on different sets may overlap.  Sized on first use (ensure_slice_scratch).
struct RxScratch {
    DevArr<float> pl_f; DevArr<uint32_t> pl_bits;                            // planar baseband and its sign planes (K1 or k_planarize)
    DevArr<uint16_t> evl; DevArr<float> evthr;                               // K2: the tiles' detections and their thresholds
    DevArr<TileRec> recs; DevArr<unsigned long long> tsum; DevArr<ScanOut> outs;
    DevArr<GroupAgg> gagg; DevArr<GroupPre> gpre; DevArr<unsigned> gtick;    // K3 (k_scan_tiles): group aggregates, group carry-ins, the arrival counters (zero between launches)
    DevArr<TileSumG> gsum; DevArr<ScanOutG> gouts; DevArr<uint32_t> evg;     // general receiver only (tracking clock / lock drops): allocated on first use
    DevArr<GroupSumG> gsg; DevArr<GroupPreG> gpg;
};

// A scratch set and what orders its users.  A pipelined call runs K1 (caller's stream) -> K2 .. K4 (the handle's receive stream) -> the next K1
// into the same set `depth` calls later: ev_k1 makes the receive stream wait for K1, ev_rx the set's next user for the chain.  (The pipelined
// shard step rotates through up to MAX_LANES sets: its chain holds exchanges that only find room on the chip when a K1 drains, so it spans several.)
struct Lane {
    RxScratch s;
    hipEvent_t ev_k1 = nullptr, ev_rx = nullptr;
    bool pending = false;                  // ev_rx stands for receive kernels that may still be running on this set
    hipStream_t joined = nullptr; bool joined_any = false;   // the stream that has already been made to wait for ev_rx (valid while pending && joined_any)
};

// The set a pipelined call of `depth` sets takes next, and where the one it retires goes.  With `cur` the current id and
// q[0 .. MAX_LANES-2] the others:  new_cur = q[0]; q[0 .. d-3] = q[1 .. d-2]; q[d-2] = cur; cur = new_cur  (depth 2: a plain exchange;
// a handle that only ever uses one depth d walks 0, 1, ..., d-1, 0, ...).  Entries of q at and beyond d-1 do not move.
static inline void rotate_lanes(int* cur, int* q, int depth)
{
    const int next = q[0];
    for (int k = 0; k + 2 < depth; ++k) q[k] = q[k + 1];
    q[depth - 2] = *cur;
    *cur = next;
}

// A time shard between its passes.  The planar baseband and the tile summaries stay in the current scratch set; the flags say what is there:
//   entry point                    requires               leaves
//   main   (pass1, _main, _k1)     --                     invalidate(); main_out for this range; head_done = the launch held the head's segments too
//   head   (pass1_head)            main_out, same range   unless head_done: the head goes out on the caller's stream, head_flagged = it has a workgroup; head_done
//   finish (pass1, _finish)        main_out, same range   the head goes out here unless head_done; K2 (waits for flag >= seq if head_flagged), K3; finish_pass1()
//   pass 2                         valid                  !scan_fresh (K3 rewrites the groups' carry-ins)
//   pass 2 dev                     valid                  the closed form on pass 1's scan iff !gen && scan_fresh && nbb != 0, else !scan_fresh
//   pipe_begin; pipe_end           !pipe; pipe            invalidate(), pipe; !pipe
//   any other user of the scratch  --                     invalidate(): a stale head, finish or pass 2 is refused
struct ShardCtx {
    bool valid = false;                    // pass 1 is complete: nbb, abs_bb0, gen describe what pass 2 finds in the scratch
    bool main_out = false;                 // the main K1 launch of (main_nbb, main_abs0) is out, waiting for p25fe_shard_pass1_finish
    size_t main_nbb = 0; uint64_t main_abs0 = 0;
    bool head_done = false;                // ... and its head segment has been launched too
    bool head_flagged = false;             // ... by p25fe_shard_pass1_head: the detection's first tiles wait for flag >= seq
    DevBuf flag;                           // SH_FLAG_WORDS words (above)
    unsigned seq = 0; int head_tile_max = -1;
    size_t nbb = 0; long abs_bb0 = 0;
    bool gen = false;                      // pass 1 ran the general receiver (pass 2 reads its summaries)
    bool pipe = false;                     // between p25fe_shard_pipe_begin and _end: the shard passes do not join the receive stream (they ARE its work)
    bool scan_fresh = false;               // the groups' carry-ins (`gpre`) are still pass 1's (no carry-in): p25fe_shard_pass2 rewrites them
    bool main_is(size_t n_bb, uint64_t abs0) const { return main_out && main_nbb == n_bb && main_abs0 == abs0; }
    void invalidate() { valid = false; main_out = false; head_done = false; head_flagged = false; }
    void finish_pass1(size_t n_bb, long bb0, bool general) { valid = true; nbb = n_bb; abs_bb0 = bb0; gen = general; scan_fresh = true; main_out = false; head_done = false; }
};

// state blob: header | IQ history raw | baseband tail | anchors | totals
struct StateHeader { uint32_t magic, abi; int32_t n_channels, fmt_locked; uint64_t abs_iq, abs_bb; };

// Where the stream stands (the streaming entry points; per channel, all of it host side)
struct StreamState {
    uint64_t abs_iq = 0, abs_bb = 0;       // IQ samples consumed; baseband samples consumed by the slicer
    int fmt_locked = -1;
    std::vector<char> hist_iq;             // [C][SHARD_HALO] raw samples (8 bytes reserved per sample)
    std::vector<float> tail_bb;            // [C][BBPAD]
    std::vector<p25fe_anchor_t> anchor;    // [C]
    std::vector<uint64_t> total_dibits;    // [C]
    void reset(size_t C)                   // (may throw)
    {
        abs_iq = 0; fmt_locked = -1; abs_bb = 0;
        anchor.assign(C, p25fe_anchor_t{0, 0.f, 0.f, 0.f, 0, SPS, 1}); total_dibits.assign(C, 0);
        hist_iq.assign(C * SHARD_HALO * 8, 0); tail_bb.assign(C * BBPAD, 0.f);
    }
    bool format_refused(int fmt) const { return fmt_locked >= 0 && fmt_locked != fmt && abs_iq > 0; }
    size_t n_hist() const { return abs_iq < SHARD_HALO ? (size_t)abs_iq : SHARD_HALO; }   // valid samples of the history
    void stage_hist(int fmt, char* rows, size_t row_bytes) const     // the history in front of staged input: channel c's to rows + c * row_bytes
    {
        for (size_t c = 0; c < anchor.size(); ++c) memcpy(rows + c * row_bytes, hist_iq.data() + c * SHARD_HALO * 8, SHARD_HALO * fmt_bytes(fmt));
    }
    // n new samples per channel have been consumed (channel c's at fresh + c * row_bytes): the last SHARD_HALO samples of
    // [history | new] become the history
    void commit_iq(size_t C, int fmt, size_t n, const char* fresh, size_t row_bytes)
    {
        const size_t eb = fmt_bytes(fmt);
        for (size_t c = 0; c < C; ++c) {
            char* hist = hist_iq.data() + c * SHARD_HALO * 8;
            const char* src = fresh + c * row_bytes;
            if (n >= SHARD_HALO) memcpy(hist, src + (n - SHARD_HALO) * eb, SHARD_HALO * eb);
            else { memmove(hist, hist + n * eb, (SHARD_HALO - n) * eb); memcpy(hist + (SHARD_HALO - n) * eb, src, n * eb); }
        }
        fmt_locked = fmt; abs_iq += n;
    }
    // the receiver has consumed n_bb baseband samples: channel c stands at res[c].anchor_out and gave n_dibits[c] dibits (null: res[c].n_dibits)
    void commit_recv(const p25fe_result_t* res, const uint64_t* n_dibits, size_t n_bb)
    {
        for (size_t c = 0; c < anchor.size(); ++c) { anchor[c] = res[c].anchor_out; total_dibits[c] += n_dibits ? n_dibits[c] : res[c].n_dibits; }
        abs_bb += n_bb;
    }
    // Channel c's baseband tail for a later p25fe_slice after a call that produced nb samples: the newest BBPAD.  `fresh` [TAILN] is what
    // k_tail_extract read from the planes, which hold HIST_BB + look samples in front of the call's first; what is older (a very short chunk)
    // comes from the previous tail.  (That branch has nb - BBPAD + j < -(HIST_BB + look) <= 0, hence j + nb < BBPAD: inside the tail.)
    void merge_tail(size_t c, size_t nb, long look, const float* fresh)
    {
        float* t = tail_bb.data() + c * BBPAD;
        float merged[BBPAD];
        for (size_t j = 0; j < (size_t)BBPAD; ++j) {
            const long m = (long)nb - (long)BBPAD + (long)j;        // index relative to this call's first baseband sample
            merged[j] = m >= -(long)(HIST_BB + look) ? fresh[j] : t[j + nb];
        }
        memcpy(t, merged, sizeof merged);
    }
    // the blob behind its header: these four, in this order
    struct Sec { void* p; size_t bytes; };
    void sections(Sec s[4])
    {
        s[0] = {hist_iq.data(), hist_iq.size()}; s[1] = {tail_bb.data(), tail_bb.size() * sizeof(float)};
        s[2] = {anchor.data(), anchor.size() * sizeof(p25fe_anchor_t)}; s[3] = {total_dibits.data(), total_dibits.size() * sizeof(uint64_t)};
    }
    size_t blob_size() { Sec s[4]; sections(s); return sizeof(StateHeader) + s[0].bytes + s[1].bytes + s[2].bytes + s[3].bytes; }
    void write(char* p)
    {
        StateHeader hd = {STATE_MAGIC, P25FE_ABI_VERSION, (int32_t)anchor.size(), fmt_locked, abs_iq, abs_bb};
        memcpy(p, &hd, sizeof hd); p += sizeof hd;
        Sec s[4]; sections(s);
        for (int k = 0; k < 4; ++k) { memcpy(p, s[k].p, s[k].bytes); p += s[k].bytes; }
    }
    // false, and nothing taken over, if the blob is not one of a handle with this many channels and this clock (`track`)
    bool read(const char* p, int track)
    {
        StateHeader hd;
        memcpy(&hd, p, sizeof hd); p += sizeof hd;
        if (hd.magic != STATE_MAGIC || hd.abi != P25FE_ABI_VERSION || hd.n_channels != (int32_t)anchor.size()) return false;
        if (hd.fmt_locked != -1 && !fmt_known(hd.fmt_locked)) return false;
        if (hd.abs_iq >= P25FE_MAX_POSITION || hd.abs_bb >= P25FE_MAX_POSITION) return false;
        Sec s[4]; sections(s);
        // a blob is data from outside: every anchor's clock must be a usable period before anything is taken over
        for (size_t c = 0; c < anchor.size(); ++c) {
            p25fe_anchor_t a;
            memcpy(&a, p + s[0].bytes + s[1].bytes + c * sizeof a, sizeof a);
            // (0 / 0 reads as 10 / 1: include/p25fe.h)
            if (!(a.period_d == 0 && a.period_n == 0) && !clock_plausible(a.period_d, a.period_n)) return false;
            if (!track && a.valid != 0 && !(a.period_d == 0 && a.period_n == 0) && !(a.period_d == SPS && a.period_n == 1)) return false;
            if (a.valid != 0 && (a.s >= (int64_t)P25FE_MAX_POSITION || a.s <= -(int64_t)P25FE_MAX_POSITION)) return false;
        }
        for (int k = 0; k < 4; ++k) { memcpy(s[k].p, p, s[k].bytes); p += s[k].bytes; }
        fmt_locked = hd.fmt_locked; abs_iq = hd.abs_iq; abs_bb = hd.abs_bb;
        return true;
    }
};

// Profiling ring: PROF_RING calls x 5 events (before K1, after K1, K2, K3, K4).  An entry point opens a slot with begin() and closes it
// with end(); the launchers in between mark the open slot, if there is one.
struct Prof {
    bool on = false;
    int level = 1;                         // 1: events around every kernel, 2: around K1 only (two records per call, not five), 3: that on a sample of the calls
    std::vector<hipEvent_t> ev;
    std::vector<uint8_t> mask;             // per slot: which of its five events were recorded
    uint64_t calls = 0, seq = 0;           // seq: level 3, calls seen (every PROF_SAMPLE-th is recorded)
    int slot = -1;                         // slot being recorded by the current call
    void begin()
    {
        // level 3: only every PROF_SAMPLE-th call carries events (the two records around K1 are two more packets between kernels, ~4 us each)
        if (on && level == 3 && (seq++ % PROF_SAMPLE) != 0) { slot = -1; return; }
        slot = on ? (int)(calls++ % PROF_RING) : -1;
        if (slot >= 0) mask[(size_t)slot] = 0;
    }
    void end() { slot = -1; }
    // ext_events (the handle's): K1's pair rides on its dispatch (k1_events) instead of being recorded
    void mark(int idx, hipStream_t st, bool ext_events)
    {
        if (slot < 0 || (idx > 1 && level != 1) || (idx <= 1 && ext_events)) return;      // levels 2, 3: only the two events around K1
        if (hipEventRecord(ev[(size_t)slot * 5 + idx], st) == hipSuccess) mask[(size_t)slot] |= (uint8_t)(1u << idx);
    }
    // the open slot's pair for K1's own dispatch (null when this call is not sampled): the kernel's begin / end time stamps, no extra packet
    void k1_events(bool ext_events, hipEvent_t* e0, hipEvent_t* e1)
    {
        *e0 = *e1 = nullptr;
        if (slot < 0 || !ext_events) return;
        *e0 = ev[(size_t)slot * 5 + 0]; *e1 = ev[(size_t)slot * 5 + 1];
        mask[(size_t)slot] |= 3u;
    }
};

// p25fe_run_host_windows: window k uses device window and dibit rows k % WIN_PARITY, result records and events k % WIN_RING
constexpr size_t WIN_PARITY = 2, WIN_RING = 4;
struct WinSlot {                           // what window k's events mark, each on the stream that records it
    hipEvent_t h2d_begin = nullptr, h2d_end = nullptr;     // copy stream: around the window's host-to-device copy
    hipEvent_t comp_begin = nullptr, comp_end = nullptr;   // compute stream: around its kernels
    hipEvent_t on_host = nullptr;                          // result stream: its records and dibit rows are in pinned memory
    std::array<hipEvent_t*, 5> all() { return {&h2d_begin, &h2d_end, &comp_begin, &comp_end, &on_host}; }
};
struct Windows {
    DevBuf buf[WIN_PARITY], dib[WIN_PARITY], res, anc;
    PinBuf stage[WIN_PARITY], out;
    hipStream_t cs = nullptr, os = nullptr;                // the copy stream, the result stream (compute: the handle's)
    WinSlot slot[WIN_RING];
    WinSlot& of(size_t k) { return slot[k % WIN_RING]; }
    hipError_t ensure()                    // the streams and events, once
    {
        if (cs) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&os, hipStreamNonBlocking);
        for (WinSlot& s : slot) for (hipEvent_t* x : s.all()) if (e == hipSuccess) e = hipEventCreate(x);
        return e;
    }
};

}  // namespace (the handle's parts: nothing of them is exported)

// The handle.  Every call uses the scratch set lanes[cur].s; a pipelined call first moves on to the next one (pipe_open).  A set keeps
// its id, which is its index in `lanes`.
// Device buffers that are per HANDLE on purpose, although chains on different sets use them, and what that rests on:
//  power_partial, chunk_cnt  K1's own: written and consumed inside one K1 launch (+ k_power_finish behind it).  Safe while a handle's K1s go down one
//                            stream: the pipelined calls keep K1 on the caller's, the chunk calls' is h->stream (synchronised before they return).
//  evrec, evnext, evoff      the detection list of symbol_clock = 2: only p25fe_run_dev* and p25fe_slice_dev use it, either on the one receive
//                            stream or, unpipelined, on the caller's stream behind pipe_join; ev_seq tells the calls' entries apart.
//  sh.flag                   one shard is between its passes at a time; K2 waits for flag >= seq, seq only grows, and the heads of consecutive
//                            (pipelined) steps finish in order while the caller gives them one stream (p25fe_rccl.cpp does).
struct p25fe {
    // configuration: written by p25fe_create only
    p25fe_config_t cfg;
    int C = 1, n_cu = 256;
    Taps taps;                             // resolved numbers: padded tables, the u8 table, the discriminator's scale
    int k1_p = 5;                          // FIR outputs per thread
    int variant = P25FE_VARIANT_BUILTIN;   // which front-end kernels run (p25fe_kernel_variant)
    bool dflt = true;                      // the numbers are the build's own (the built-in kernels carry them, whatever `variant` says)
    bool long_taps = false;                // more than P25FE_T1 / P25FE_T2 taps -> the 64 / 64 geometry (Geo<5, 1>)
    int phase = P25FE_DECIM_PHASE;         // p25fe_config_t.decim_phase: baseband sample m comes from input 5 m + phase
    int n_avg = BOX;                       // post-discriminator filter: taps in use (the table is taps.avg)
    bool u8_lut_mode = false;              // the u8 table is not affine: the specialised kernels look it up in LDS (the generic ones always do)
    float u8_scale = 0.0f, u8_offset = 0.0f;   // the affine u8 table as arithmetic (unused when u8_lut_mode): K0 / K6 on u8 input
    int track = 0;                         // p25fe_config_t.symbol_clock without its flag bits (docs/SPEC.md 3.8b)
    bool causal_ok = false;                // P25FE_CLOCK_CAUSAL_OK: mode 2 may run as mode 1 in the calls that see the stream in pieces
    long look = 0;                         // samples the receiver runs behind the baseband (2 with the tracking clock)
    bool ext_events = true;                // events ride on the kernel dispatches (hipExtLaunchKernelGGL) instead of separate records
    int rx_cus = 0;                        // > 0: the receive stream is confined to this many CUs (hipExtStreamCreateWithCUMask)
    int run_depth = 2;                     // sets p25fe_run_dev_pipelined rotates through (P25FE_PIPE_DEPTH)
    bool k1_pair = true;                   // cf32 planar main launches run k_frontend_pair (P25FE_K1_PAIR=0: k_frontend everywhere)
    int sh_depth = MAX_LANES;              // sets the pipelined shard step rotates through (P25FE_SHARD_PIPE_DEPTH)

    int last_hip = 0;
    DevBuf d_taps;                         // device copy (generic kernels: everything; specialised ones: the u8 table, if not affine)
    hipModule_t jit_mod = nullptr;         // specialised kernels (p25fe_jit.cpp): [format][linear, planar, chunk]
    hipFunction_t jit_fn[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    hipStream_t stream = nullptr, rx_stream = nullptr;   // for the host-pointer calls; for the receive chains of the pipelined calls
    const long* rs_idx = nullptr; size_t rs_n = 0, rs_stride = 0;    // lock drops for the next receiver-running call (p25fe_resync_at_dev); consumed by it
    Lane lanes[MAX_LANES];
    int cur = 0, lane_q[MAX_LANES - 1] = {1, 2, 3};    // the current set's id, the others' in the order they come up (rotate_lanes)
    int pl_lane = -1; size_t pl_blocks = 0;            // the set whose planes the most recent call sized, and their blocks per channel (p25fe_debug_planes_dev)
    Lane& lane() { return lanes[cur]; }
    RxScratch& rx() { return lanes[cur].s; }
    const RxScratch& rx() const { return lanes[cur].s; }
    DevBuf power_partial, chunk_cnt, evrec, evnext, evoff;
    unsigned long long ev_seq = 0;         // marks an EvNext entry as this call's
    PinBuf hin, hbb, hout;                 // streaming entry points: staged input ([history | new] IQ, [tail | new] baseband), results
    unsigned chunk_seq = 0;                // completion sequence number of the one-launch chunk calls
    Windows win; StreamState state; Prof prof; ShardCtx sh;
};

// geometry of the planar scratch for n_bb owned baseband samples (p25fe_recv.hip: Planar)
struct PlanarGeo {
    size_t n_tiles, n_blocks;
    explicit PlanarGeo(size_t n_bb)
    {
        n_tiles = (n_bb + TS - 1) / TS;
        if (n_tiles == 0) n_tiles = 1;
        n_blocks = (size_t)TWORDS * n_tiles + 6;   // K1 writes symbols < 768 n_tiles + 32; K2 reads words < 24 n_tiles + 5
    }
    size_t floats() const { return n_blocks * PL_BLK; }
    size_t words() const { return n_blocks * SPS; }
};

// Symbol indices are 32-bit in the receive kernels: a range holds < 2^31 symbols (124 h of one channel).  Checked by every
// entry point BEFORE it sizes scratch for the range, so that an absurd length is an argument error, not an allocation failure.
constexpr size_t MAX_RANGE_BB = (size_t)0x7ff00000u * 10u;
// Positions (abs0, abs_bb0, the counters of a state blob) are 64-bit sample counts kept as signed 64-bit indices inside the kernels,
// with a range's length, the lookahead and the history added on top: P25FE_MAX_POSITION (include/p25fe.h) leaves that headroom.
static inline bool position_refused(uint64_t pos) { return pos >= P25FE_MAX_POSITION; }

// --------------------------------------------------------------------------------------------
// p25fe_config_t -> the numbers the kernels run with.  No device needed (p25fe_specialize runs on a build host).
// --------------------------------------------------------------------------------------------
struct Resolved {
    Taps taps;              // tables zero-padded to the evaluation length, the u8 table, the discriminator's scale, the post-discriminator filter
    bool long_taps;         // 64 / 64 evaluation
    bool lut_affine;        // the u8 table is fma(b, u8_scale, u8_offset) for every byte
    float u8_scale, u8_offset;
    bool dflt;              // every number is the build's own (p25fe_spec.h): the built-in immediate-coefficient kernels apply
};

static inline bool finite_f(float v) { return v - v == 0.0f; }
static inline bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

static bool lut_is_affine(const float* lut, float sc, float of)
{
    for (int b = 0; b < 256; ++b)
        if (!same_bits(lut[b], fmaf((float)b, sc, of))) return false;
    return true;
}

static int resolve_config(const p25fe_config_t* cfg, Resolved* r)
{
    if (cfg->abi_version != P25FE_ABI_VERSION || cfg->n_decim_taps < 1 || cfg->n_decim_taps > P25FE_MAX_TAPS || cfg->n_chan_taps < 1 ||
        cfg->n_chan_taps > P25FE_MAX_TAPS || (cfg->symbol_clock != P25FE_CLOCK_FIXED && cfg->symbol_clock != P25FE_CLOCK_TRACKING && cfg->symbol_clock != P25FE_CLOCK_TRACKING_RESLICE &&
         cfg->symbol_clock != (P25FE_CLOCK_TRACKING_RESLICE | P25FE_CLOCK_CAUSAL_OK)) ||
        cfg->specialize < P25FE_SPECIALIZE_OFF || cfg->specialize > P25FE_SPECIALIZE_FORCE || cfg->decim_phase < 0 || cfg->decim_phase >= DEC ||
        cfg->n_avg_taps < 1 || cfg->n_avg_taps > P25FE_MAX_TAPS)
        return P25FE_ERR_ARG;
    memset(&r->taps, 0, sizeof r->taps);                             // zero padding at the old end is bit-neutral on finite samples
    // MovingAverage::new(10), src/demod.rs:52 (docs/SPEC.md 3.5): all taps equal -> a moving average, summed then scaled once
    r->taps.n_avg = cfg->n_avg_taps;
    r->taps.avg_uniform = 1;
    for (int k = 0; k < cfg->n_avg_taps; ++k) {
        if (!finite_f(cfg->avg_taps[k])) return P25FE_ERR_ARG;
        r->taps.avg[k] = cfg->avg_taps[k];
        if (!same_bits(cfg->avg_taps[k], cfg->avg_taps[0])) r->taps.avg_uniform = 0;
    }
    for (int k = 0; k < cfg->n_decim_taps; ++k) { if (!finite_f(cfg->decim_taps[k])) return P25FE_ERR_ARG; r->taps.dec[k] = cfg->decim_taps[k]; }
    for (int k = 0; k < cfg->n_chan_taps; ++k) { if (!finite_f(cfg->chan_taps[k])) return P25FE_ERR_ARG; r->taps.ch[k] = cfg->chan_taps[k]; }
    r->long_taps = cfg->n_decim_taps > P25FE_T1 || cfg->n_chan_taps > P25FE_T2;
    // FmDemod::new(deviation, sample_rate), src/demod.rs:54 -> output scale (docs/SPEC.md 3.4)
    if (cfg->fm_gain != 0.0f) {
        if (!finite_f(cfg->fm_gain)) return P25FE_ERR_ARG;
        r->taps.fm_gain = cfg->fm_gain;
    } else {
        if (cfg->fm_deviation_hz == 0 || cfg->fm_sample_rate_hz == 0) return P25FE_ERR_ARG;
        r->taps.fm_gain = (float)((double)cfg->fm_sample_rate_hz / (2.0 * M_PI * (double)cfg->fm_deviation_hz));
    }
    // rtlsdr_iq::IQ, src/demod.rs:83 (docs/SPEC.md 3.1)
    if (cfg->u8_lut_valid) {
        for (int b = 0; b < 256; ++b) { if (!finite_f(cfg->u8_lut[b])) return P25FE_ERR_ARG; r->taps.lut[b] = cfg->u8_lut[b]; }
        // a table that IS an fma of the byte runs as arithmetic: the caller's own pair first, then the two obvious fits
        const float* L = r->taps.lut;
        const float cand[3][2] = {{cfg->u8_scale, cfg->u8_offset}, {L[1] - L[0], L[0]},
                                  {(float)(((double)L[255] - (double)L[0]) / 255.0), L[0]}};
        r->lut_affine = false;
        for (int c = 0; c < 3 && !r->lut_affine; ++c)
            if (finite_f(cand[c][0]) && finite_f(cand[c][1]) && lut_is_affine(L, cand[c][0], cand[c][1])) {
                r->lut_affine = true; r->u8_scale = cand[c][0]; r->u8_offset = cand[c][1];
            }
        if (!r->lut_affine) r->u8_scale = r->u8_offset = 0.0f;
    } else {
        if (!finite_f(cfg->u8_scale) || !finite_f(cfg->u8_offset)) return P25FE_ERR_ARG;
        r->lut_affine = true; r->u8_scale = cfg->u8_scale; r->u8_offset = cfg->u8_offset;
        for (int b = 0; b < 256; ++b) r->taps.lut[b] = fmaf((float)b, cfg->u8_scale, cfg->u8_offset);
    }
    Taps def;
    memset(&def, 0, sizeof def);
    memcpy(def.dec, P25FE_DEFAULT_DECIM_TAPS, sizeof(float) * P25FE_T1);
    memcpy(def.ch, P25FE_DEFAULT_CHAN_TAPS, sizeof(float) * P25FE_T2);
    memcpy(def.avg, P25FE_DEFAULT_AVG_TAPS, sizeof(float) * BOX);
    r->dflt = !r->long_taps && memcmp(def.dec, r->taps.dec, sizeof def.dec) == 0 && memcmp(def.ch, r->taps.ch, sizeof def.ch) == 0 &&
              r->taps.n_avg == BOX && memcmp(def.avg, r->taps.avg, sizeof def.avg) == 0 &&
              same_bits(r->taps.fm_gain, P25FE_FM_GAIN) && r->lut_affine && same_bits(r->u8_scale, P25FE_U8_SCALE) &&
              same_bits(r->u8_offset, P25FE_U8_OFFSET);
    return P25FE_OK;
}

static p25jit::Spec jit_spec(const Resolved& r)
{
    p25jit::Spec s;
    memset(&s, 0, sizeof s);
    s.tx = r.long_taps ? 1 : 0;
    s.t1 = r.long_taps ? TMAX : T1;
    s.t2 = r.long_taps ? TMAX : T2;
    memcpy(s.dec, r.taps.dec, sizeof s.dec);
    memcpy(s.ch, r.taps.ch, sizeof s.ch);
    s.fm_gain = r.taps.fm_gain;
    s.u8_lut = r.lut_affine ? 0 : 1;
    s.u8_scale = r.u8_scale; s.u8_offset = r.u8_offset;
    s.n_avg = r.taps.n_avg; s.avg_uniform = r.taps.avg_uniform;
    memcpy(s.avg, r.taps.avg, sizeof s.avg);
    return s;
}

static thread_local std::string t_jit_log;          // compiler log of this thread's last p25fe_create / p25fe_specialize

// Where specialised code objects are looked for: $P25FE_SPEC_DIR (a deployment's ahead-of-time directory), then the cache.
static std::vector<std::string> jit_dirs()
{
    std::vector<std::string> d;
    const char* e = getenv("P25FE_SPEC_DIR");
    if (e && *e) d.push_back(e);
    d.push_back(p25jit::default_cache_dir());
    return d;
}

// P25FE_SPECIALIZE_AUTO fell back to the generic kernels (1.3 - 2.4 x slower): say so once per process, on stderr -- a caller
// that never polls p25fe_kernel_variant would otherwise not know.  P25FE_QUIET=1 silences it.
static void fallback_notice()
{
    static bool said = false;
    if (said) return;
    said = true;
    const char* q = getenv("P25FE_QUIET");
    if (q && atoi(q) != 0) return;
    fprintf(stderr, "p25fe: no specialised kernels for this configuration's numbers (no usable cached code object and hipRTC did not "
                    "deliver one): running the GENERIC kernels, 1.3 - 2.4 x slower.  p25fe_specialize_log() has the details; "
                    "p25fe_specialize() / $P25FE_SPEC_DIR is the ahead-of-time form.\n");
}

// Which front-end kernels a handle made from cfg gets on this host, and -- for P25FE_VARIANT_SPECIALIZED -- the code object
// (looked up in $P25FE_SPEC_DIR and the cache, else compiled and stored).  Needs no device.  Returns the variant or P25FE_ERR_JIT.
static int choose_variant(const p25fe_config_t* cfg, const Resolved& rs, std::vector<char>* code, std::string* path, bool* from_cache)
{
    // P25FE_JIT=0 in the environment switches the AUTO mode off for a whole process.
    static const bool jit_env_off = [] { const char* v = getenv("P25FE_JIT"); return v && atoi(v) == 0; }();
    const bool must = cfg->specialize >= P25FE_SPECIALIZE_REQUIRE;
    const bool want_jit = (!rs.dflt || cfg->specialize == P25FE_SPECIALIZE_FORCE) && cfg->specialize != P25FE_SPECIALIZE_OFF && !(jit_env_off && !must);
    const int plain = rs.dflt ? P25FE_VARIANT_BUILTIN : P25FE_VARIANT_GENERIC;
    if (!want_jit) return plain;
    bool ok = false;
    try {
        t_jit_log.clear();
        ok = p25jit::get_code(jit_spec(rs), jit_dirs(), true, p25jit::default_cache_dir(), false, *code, *path, t_jit_log, from_cache);
    } catch (...) {
        ok = false;
        try { t_jit_log += "exception while specialising\n"; } catch (...) { }
    }
    if (ok) return P25FE_VARIANT_SPECIALIZED;
    if (must) return P25FE_ERR_JIT;
    if (plain == P25FE_VARIANT_GENERIC) fallback_notice();
    return plain;
}

// s16 has no specialised kernels yet (a code object keeps exactly its six): a configuration whose numbers are
// not the build's runs s16 through the generic kernels -- said once per process on stderr, like the notice above -- unless it
// demands specialised ones, which cannot be had.
static void s16_generic_notice()
{
    static bool said = false;
    if (said) return;
    said = true;
    const char* q = getenv("P25FE_QUIET");
    if (q && atoi(q) != 0) return;
    fprintf(stderr, "p25fe: P25FE_FMT_S16 has no specialised kernels: with this configuration's numbers s16 input runs the GENERIC "
                    "kernels (u8 and cf32 are not affected; p25fe_format_variant() reports it per format).\n");
}
// The kernels format `fmt` runs with: `variant` (what u8 and cf32 get) for those two; for s16 BUILTIN with the build's numbers, else
// GENERIC, or P25FE_ERR_JIT where the configuration requires specialised kernels.
static int format_variant_of(int variant, bool dflt, int specialize, int fmt)
{
    if (!fmt_known(fmt)) return P25FE_ERR_ARG;
    if (fmt != P25FE_FMT_S16 || variant < 0) return variant;
    if (dflt) return P25FE_VARIANT_BUILTIN;
    if (specialize >= P25FE_SPECIALIZE_REQUIRE) return P25FE_ERR_JIT;
    if (specialize != P25FE_SPECIALIZE_OFF) s16_generic_notice();
    return P25FE_VARIANT_GENERIC;
}

#define HIPCHK(h, expr)                                                        \
    do {                                                                       \
        hipError_t e__ = (expr);                                               \
        if (e__ != hipSuccess) { (h)->last_hip = (int)e__; return P25FE_ERR_HIP; } \
    } while (0)

extern "C" {

void p25fe_default_config(p25fe_config_t* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->abi_version = P25FE_ABI_VERSION;
    cfg->device = 0;
    cfg->n_channels = 1;
    cfg->n_decim_taps = P25FE_T1;
    cfg->n_chan_taps = P25FE_T2;
    memcpy(cfg->decim_taps, P25FE_DEFAULT_DECIM_TAPS, sizeof(float) * P25FE_T1);
    memcpy(cfg->chan_taps, P25FE_DEFAULT_CHAN_TAPS, sizeof(float) * P25FE_T2);
    cfg->specialize = P25FE_SPECIALIZE_AUTO;
    cfg->fm_deviation_hz = P25FE_FM_DEVIATION_HZ;                    // FmDemod::new(5000, BASEBAND_SAMPLE_RATE), src/demod.rs:54
    cfg->fm_sample_rate_hz = P25FE_FM_SAMPLE_RATE_HZ;
    cfg->fm_gain = 0.0f;                                             // derived from the two
    cfg->u8_scale = P25FE_U8_SCALE;
    cfg->u8_offset = P25FE_U8_OFFSET;
    cfg->u8_lut_valid = 0;
    cfg->decim_phase = P25FE_DECIM_PHASE;                            // Decimator::new(5): the 5th sample of every five, src/demod.rs:50, 87-90
    cfg->n_avg_taps = P25FE_BOXCAR;                                  // MovingAverage::new(10), src/demod.rs:52
    memcpy(cfg->avg_taps, P25FE_DEFAULT_AVG_TAPS, sizeof(float) * P25FE_BOXCAR);
}

const char* p25fe_strerror(int status)
{
    switch (status) {
    case P25FE_OK: return "ok";
    case P25FE_ERR_ARG: return "invalid argument";
    case P25FE_ERR_NO_DEVICE: return "no usable HIP device (gfx950 required; there is no CPU fallback)";
    case P25FE_ERR_HIP: return "HIP runtime error";
    case P25FE_ERR_CAPACITY: return "output buffer too small";
    case P25FE_ERR_FORMAT: return "sample format changed within a stream";
    case P25FE_ERR_NOMEM: return "out of memory";
    case P25FE_ERR_JIT: return "kernel specialisation failed (p25fe_specialize_log)";
    case P25FE_ERR_TIMEOUT: return "a device-side wait gave up (time shard: the head segment never arrived)";
    default: return "unknown status";
    }
}

int p25fe_last_hip_error(const p25fe_t* h) { return h ? h->last_hip : 0; }
int p25fe_device(const p25fe_t* h) { return h ? h->cfg.device : -1; }
int p25fe_kernel_variant(const p25fe_t* h) { return h ? h->variant : -1; }
int p25fe_format_variant(const p25fe_t* h, int fmt)
{
    return h ? format_variant_of(h->variant, h->dflt, h->cfg.specialize, fmt) : P25FE_ERR_ARG;
}

size_t p25fe_specialize_log(char* buf, size_t cap)
{
    if (!buf || cap == 0) return 0;
    const size_t n = t_jit_log.size() < cap - 1 ? t_jit_log.size() : cap - 1;
    memcpy(buf, t_jit_log.data(), n);
    buf[n] = '\0';
    return n;
}

int p25fe_specialize(const p25fe_config_t* cfg, const char* dir, char* path_out, size_t path_cap)
{
    if (!cfg) return P25FE_ERR_ARG;
    if (path_out && path_cap) path_out[0] = '\0';
    Resolved r;
    const int rc = resolve_config(cfg, &r);
    if (rc) return rc;
    if (r.dflt && cfg->specialize != P25FE_SPECIALIZE_FORCE) return P25FE_OK;   // the library's own kernels carry these numbers
    try {
        t_jit_log.clear();
        const std::string d = (dir && *dir) ? std::string(dir) : p25jit::default_cache_dir();
        std::vector<char> code;
        std::string path;
        if (!p25jit::get_code(jit_spec(r), {d}, true, d, /*aot=*/true, code, path, t_jit_log) || path.empty()) return P25FE_ERR_JIT;
        if (path_out && path_cap) snprintf(path_out, path_cap, "%s", path.c_str());
    } catch (...) {
        return P25FE_ERR_NOMEM;
    }
    return P25FE_OK;
}

int p25fe_probe_variant(const p25fe_config_t* cfg)
{
    if (!cfg) return P25FE_ERR_ARG;
    Resolved r;
    const int rc = resolve_config(cfg, &r);
    if (rc) return rc;
    std::vector<char> code;
    std::string path;
    try {
        return choose_variant(cfg, r, &code, &path, nullptr);
    } catch (...) {
        return P25FE_ERR_NOMEM;
    }
}

int p25fe_probe_format_variant(const p25fe_config_t* cfg, int fmt)
{
    if (!cfg || !fmt_known(fmt)) return P25FE_ERR_ARG;
    if (fmt != P25FE_FMT_S16) return p25fe_probe_variant(cfg);
    Resolved r;
    const int rc = resolve_config(cfg, &r);
    if (rc) return rc;
    return format_variant_of(P25FE_VARIANT_GENERIC, r.dflt, cfg->specialize, fmt);
}

static inline size_t n_baseband_ph(int phase, uint64_t abs0, size_t n)
{
    const size_t o0 = (size_t)(((uint64_t)phase + 5 - abs0 % 5) % 5);       // first decimation instant inside the range
    return n > o0 ? (n - o0 - 1) / 5 + 1 : 0;
}
size_t p25fe_n_baseband(uint64_t abs0, size_t n) { return n_baseband_ph(P25FE_DECIM_PHASE, abs0, n); }
size_t p25fe_n_baseband_h(const p25fe_t* h, uint64_t abs0, size_t n) { return n_baseband_ph(h ? h->phase : P25FE_DECIM_PHASE, abs0, n); }

size_t p25fe_shard_halo(void) { return SHARD_HALO; }

int p25fe_reset(p25fe_t* h)
{
    if (!h) return P25FE_ERR_ARG;
    h->rs_idx = nullptr; h->rs_n = 0; h->rs_stride = 0;             // a pending lock-drop list belonged to the old stream
    try {                                                           // no exception crosses the C boundary
        h->state.reset((size_t)h->C);
    } catch (...) {
        return P25FE_ERR_NOMEM;
    }
    return P25FE_OK;
}

int p25fe_create(const p25fe_config_t* cfg, p25fe_t** out)
{
    if (!cfg || !out) return P25FE_ERR_ARG;
    *out = nullptr;
    if (cfg->abi_version != P25FE_ABI_VERSION || cfg->n_channels < 1 || cfg->n_channels > 65535 /* grid.y */) return P25FE_ERR_ARG;
    Resolved rs;
    if (int rrc = resolve_config(cfg, &rs)) return rrc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
        return P25FE_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return P25FE_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return P25FE_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return P25FE_ERR_NO_DEVICE;   // code object is gfx950 only

    p25fe_t* h = new (std::nothrow) p25fe;
    if (!h) return P25FE_ERR_NOMEM;
    h->cfg = *cfg;
    h->C = cfg->n_channels;
    h->track = cfg->symbol_clock & 0xff;
    h->causal_ok = (cfg->symbol_clock & P25FE_CLOCK_CAUSAL_OK) != 0;
    h->look = h->track ? CLK_L : 0;
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->taps = rs.taps;
    h->phase = cfg->decim_phase;
    h->n_avg = rs.taps.n_avg;
    h->long_taps = rs.long_taps;
    h->u8_lut_mode = !rs.lut_affine;
    h->u8_scale = rs.u8_scale; h->u8_offset = rs.u8_offset;
    h->variant = rs.dflt ? P25FE_VARIANT_BUILTIN : P25FE_VARIANT_GENERIC;
    h->dflt = rs.dflt;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { p25fe_destroy(h); return P25FE_ERR_HIP; }
    hipError_t e = hipSuccess;
    {
        const char* pv = getenv("P25FE_K1_P");            // tuning knob: FIR outputs per lane (5 default, 3)
        h->k1_p = (pv && atoi(pv) == 3) ? 3 : 5;
        // measurement knobs of the two-stream form: events attached to the dispatches (default) or
        // recorded separately; CUs the receive stream is confined to (0 = no mask)
        const char* ee = getenv("P25FE_EXT_EVENTS");
        h->ext_events = !(ee && atoi(ee) == 0);
        const char* rc_ = getenv("P25FE_RX_CUS");
        h->rx_cus = rc_ ? atoi(rc_) : 0;
        const char* pd = getenv("P25FE_SHARD_PIPE_DEPTH");            // (measurement knob: 2 .. MAX_LANES)
        if (pd && atoi(pd) >= 2 && atoi(pd) <= MAX_LANES) h->sh_depth = atoi(pd);
        // The general receiver's chain (tracking clock) is the longer one: 150 - 230 us beside a K1 of 275.  Round 5's held a 512-thread
        // k_scan_g that waited for K1's drain, and a third scratch set was worth 12 % (0.326 -> 0.286 ms per pipelined step); with the chain
        // as one-wave work it still is worth 0.6 - 0.9 % (profiles/r06_run_depth.txt).  The fixed-stride chain: two sets.
        if (cfg->symbol_clock != P25FE_CLOCK_FIXED) h->run_depth = 3;
        const char* rd = getenv("P25FE_PIPE_DEPTH");
        if (rd && atoi(rd) >= 2 && atoi(rd) <= MAX_LANES) h->run_depth = atoi(rd);
        const char* kp = getenv("P25FE_K1_PAIR");                     // (A/B knob: 0 = the one-wave kernel for every K1 launch)
        h->k1_pair = !(kp && atoi(kp) == 0);
    }
    if (e == hipSuccess) e = h->d_taps.ensure(sizeof(Taps));
    if (e == hipSuccess) e = hipMemcpy(h->d_taps.p, &h->taps, sizeof(Taps), hipMemcpyHostToDevice);
    if (e != hipSuccess) { p25fe_destroy(h); return P25FE_ERR_HIP; }
    // Numbers other than the build's own: the same kernels with THOSE numbers as immediates (cached code object, else
    // hipRTC -- seconds, once per set of numbers and library build); the generic LDS-tap kernels if that is off or fails.
    {
        std::vector<char> code;
        std::string path;
        bool from_cache = false;
        int var = choose_variant(cfg, rs, &code, &path, &from_cache);
        if (var < 0) { p25fe_destroy(h); return var; }
        if (var == P25FE_VARIANT_SPECIALIZED) {
            bool ok = false;
            try {
                hipError_t me = hipModuleLoadData(&h->jit_mod, code.data());
                if (me != hipSuccess && from_cache) {
                    // a verified file the loader still refuses (another architecture's object under this name): compile afresh;
                    // the stale entry is removed only from the cache -- never from a deployment's $P25FE_SPEC_DIR
                    (void)hipGetLastError();
                    t_jit_log += "cached code object " + path + " did not load: recompiling\n";
                    const std::string store = p25jit::default_cache_dir();
                    if (path.compare(0, store.size() + 1, store + "/") == 0) (void)remove(path.c_str());
                    h->jit_mod = nullptr;
                    if (p25jit::get_code(jit_spec(rs), {}, true, store, false, code, path, t_jit_log)) me = hipModuleLoadData(&h->jit_mod, code.data());
                }
                ok = me == hipSuccess;
                for (int f = 0; f < 2 && ok; ++f)
                    for (int k = 0; k < 3 && ok; ++k)
                        ok = hipModuleGetFunction(&h->jit_fn[f][k], h->jit_mod, p25jit::KERNEL_NAMES[f][k]) == hipSuccess;
                if (!ok) { (void)hipGetLastError(); t_jit_log += "loading the specialised code object failed\n"; }
            } catch (...) {
                ok = false;
            }
            if (!ok) {
                if (h->jit_mod) { (void)hipModuleUnload(h->jit_mod); h->jit_mod = nullptr; }
                if (cfg->specialize >= P25FE_SPECIALIZE_REQUIRE) { p25fe_destroy(h); return P25FE_ERR_JIT; }
                var = rs.dflt ? P25FE_VARIANT_BUILTIN : P25FE_VARIANT_GENERIC;
                if (var == P25FE_VARIANT_GENERIC) fallback_notice();
            }
        }
        h->variant = var;
    }
    int rc = p25fe_reset(h);
    if (rc != P25FE_OK) { p25fe_destroy(h); return rc; }
    *out = h;
    return P25FE_OK;
}

// What has an order: the streams drain and go, then the module and the events; `delete h` frees every buffer after that.
void p25fe_destroy(p25fe_t* h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    for (hipStream_t st : {h->stream, h->rx_stream, h->win.cs, h->win.os})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (h->jit_mod) (void)hipModuleUnload(h->jit_mod);
    for (WinSlot& s : h->win.slot) for (hipEvent_t* e : s.all()) if (*e) (void)hipEventDestroy(*e);
    for (Lane& l : h->lanes)
        for (hipEvent_t e : {l.ev_k1, l.ev_rx}) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->prof.ev) if (e) (void)hipEventDestroy(e);
    delete h;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------
// internal launchers
// --------------------------------------------------------------------------------------------
// One K1 launch (k_frontend, or k_chunk when `chunk` is set).  The output is the linear baseband (`bb`, from output 0 on) or --
// `planar` -- the handle's planar scratch, from the layout's own first output on (a block boundary of the layout, or 80 outputs
// in front of the receiver's 240-sample history).
// part: which segments of a time shard's range run -- every one; only those whose input window lies inside the owned samples
// (the main launch, runs while the halo is still on the wire); the others (the head, after the halo has arrived)
enum K1Part { K1_ALL = 0, K1_MAIN = 1, K1_HEAD = 2 };
// An entry point's first question about its `fmt`, asked before anything moves: P25FE_ERR_ARG for a format that does not exist,
// P25FE_ERR_JIT for s16 on a handle that may only run specialised kernels, else 0.
static int format_unusable(const p25fe_t* h, int fmt)
{
    const int v = format_variant_of(h->variant, h->dflt, h->cfg.specialize, fmt);
    return v < 0 ? v : P25FE_OK;
}
struct K1Launch {
    const void* src = nullptr;             // owned sample 0 of channel 0, n_hist valid samples in front of it
    int fmt = P25FE_FMT_CF32;
    size_t ch_stride = 0, n_hist = 0, n = 0;
    uint64_t abs0 = 0;
    float* bb = nullptr; size_t bb_stride = 0;      // linear output ...
    float* power_dbm = nullptr;            // ... and (nullable) its power per channel
    bool planar = false;
    K1Part part = K1_ALL;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;        // (nullable) attached to K1's dispatch: begin / end of the kernel
    const ChunkRecvArgs* chunk = nullptr;  // (nullable, planar only) k_chunk: K1 plus the one-tile receiver run by each channel's last workgroup
    long* head_end = nullptr;              // (nullable, K1_HEAD) receives the planar position up to which the head's segments write
    unsigned* done_flag = nullptr; unsigned done_seq = 0u;   // (nullable, planar) the launch's last workgroup publishes done_flag[0] = done_seq
    hipStream_t stream = nullptr;
};

// What a K1Launch comes to: the segment geometry and the part split (as the kernel's arguments), the kernel's form, grid and LDS.
// Arithmetic only.
struct K1Plan {
    bool empty;                            // nothing to launch: no output, or no segment on this side of the part split
    K1Args a;                              // complete but for power_partial (the launch allocates it)
    int fmt, variant; bool ct; int pk;     // which kernel: format, the variant that format runs (format_variant_of), immediate coefficients, FIR outputs per lane
    bool pair;                             // k_frontend_pair (two waves per workgroup) instead of k_frontend
    long n_seg;                            // segments of the whole range (a.seg_first, a.seg_count: this launch's)
    long head_end;                         // planar position up to which the head's segments write (part != K1_ALL)
    size_t lds;
};
static int k1_plan(const p25fe_t* h, const K1Launch& L, K1Plan* p)
{
    const int fmt = L.fmt;
    const int variant = format_variant_of(h->variant, h->dflt, h->cfg.specialize, fmt);
    if (variant < 0) return variant;                               // unknown format; s16 where only specialised kernels will do
    if ((reinterpret_cast<uintptr_t>(L.src) & 15u) != 0) return P25FE_ERR_ARG;   // owned sample 0 on a 16-byte boundary, every format
    if (h->C > 1 && (L.ch_stride % fmt_stride_unit(fmt)) != 0) return P25FE_ERR_ARG;
    if (L.chunk && (!L.planar || L.part)) return P25FE_ERR_ARG;
    bool pro = seg_prologue(fmt);                                  // p25fe_kernels.hip: segment prologue (u8, s16) or recomputed halo (cf32)
    long m_begin = !L.planar ? 0 : (pro ? -(long)PLPAD - h->look : -(long)HIST_BB - h->look);
    const size_t n_out_range = p25fe_n_baseband_h(h, L.abs0, L.n); // (the planes' strides follow the whole range, whatever part a launch computes)
    long n_out = (long)n_out_range;
    static const long subs_env = [] { const char* e = getenv("P25FE_SUBS"); return e ? atol(e) : 0L; }();
    const long o0 = (long)(((uint64_t)h->phase + 5 - L.abs0 % 5) % 5);
    // The pair kernel (k_frontend_pair: prologue segments, two waves per workgroup) takes the MAIN part of a cf32 range on the planar
    // scratch when the handle runs the build's own numbers and that part holds at least one whole segment.  The range is then laid out
    // in the prologue form; its head segments (a time shard's, whose input reaches into the halo) stay on k_frontend, which computes
    // exactly their outputs -- positions [0, head_len), a whole number of blocks -- in its own halo form: the same planes, the same bits.
    K1Part part = L.part;
    bool pair = false;
    long pair_head = -1;                                            // >= 0: this is the HEAD launch of such a range: k_frontend over [m_begin, m_begin + pair_head)
    if (h->k1_pair && fmt == P25FE_FMT_CF32 && L.planar && variant == P25FE_VARIANT_BUILTIN && !h->long_taps && !L.chunk && !L.power_dbm) {
        SegGeo gp{true, WV * 5, (int)(subs_env > 0 ? (subs_env > 32768 ? 32768 : subs_env) : 3), 0, 0, -(long)PLPAD - h->look, n_out};
        const long tot = n_out - gp.m_begin;
        const int ndp = gp.front(h->n_avg, T2);
        if (L.part) gp.set_lead(ndp, o0, T1);
        const long ns = tot > 0 ? gp.count(tot) : 0;
        const long km = L.part ? gp.head_count(ns, ndp, o0, T1) : 0;
        const long head_len = km >= ns ? tot : gp.start(km) - gp.m_begin;
        if (tot - head_len >= gp.seg_len()) {
            m_begin = gp.m_begin;
            if (L.part == K1_HEAD) {
                pair_head = head_len;
                n_out = m_begin + head_len;                         // (nothing in front of the main part: the launch is empty, below)
                part = K1_ALL;
            } else {
                pair = true; pro = true;
            }
        }
    }
    const long total = n_out - m_begin;
    K1Args& a = p->a;
    a.m_begin = m_begin; a.n_out = n_out; p->pair = pair; p->head_end = pair_head > 0 ? pair_head : 0;
    p->empty = total <= 0;
    if (p->empty) return P25FE_OK;
    // Segments are SHORT: three sub-tiles per one-wave workgroup.  Measured on config 2 (profiles/): one long
    // segment per resident wave (44 sub-tiles, no tail round) ran K1 in 0.305 ms, 2-4 sub-tiles per workgroup in
    // 0.23-0.27 ms depending on the box -- neighbouring workgroups then stream neighbouring DRAM pages and the
    // dispatcher balances the CUs, which outweighs recomputing the 50-sample filter halo once per segment (5.5 % at
    // 3 sub-tiles; A/B on one box, three rounds: 2 -> 0.275, 3 -> 0.264, 4 -> 0.269 ms).  P25FE_SUBS overrides.
    const int pk = (L.planar || h->long_taps || variant == P25FE_VARIANT_SPECIALIZED) ? 5 : h->k1_p;
    const int t1 = h->long_taps ? TMAX : T1;
    // (round 2: the instruction-bound u8 kernel prefers longer segments -- less halo recomputed: 3 -> 239, 6 -> 231 us on one
    // box; with the final build 4 -> 222 / 216, 6 -> 217 / 215, 9 -> 212 / 209, 12 -> 216 / 205 us under rocprofv3)
    // (s16: u8's length until a box says otherwise -- docs/MEASUREMENTS.md)
    long subs = subs_env > 0 ? subs_env : (fmt == P25FE_FMT_U8 ? 9 : (fmt == P25FE_FMT_S16 ? P25FE_K1_SUBS_S16 : 3));
    if (L.chunk) subs = 1;                                          // a chunk is latency: every sub-tile its own workgroup
    if (pair_head >= 0) subs = 1;                                   // the head of a pair range: one-sub-tile workgroups side by side, as lead segments are
    if (subs > 32768) subs = 32768;
    // the post-discriminator filter's length as far as the kernel's GEOMETRY goes (frontend_body's T3): the handle's own for the
    // immediate-coefficient kernels, the ABI's ceiling for the generic ones; the halo form's recomputed halo follows the
    // handle's real length either way (the generic kernels take it as an argument)
    const bool ct = variant != P25FE_VARIANT_GENERIC;
    const int t2e = h->long_taps ? TMAX : T2;
    const int t3geo = ct ? h->n_avg : TMAX;
    SegGeo g{pro, WV * pk, (int)subs, seg_halo_for(h->n_avg, t2e), 0, m_begin, n_out};      // p25fe_kernels.hip: the kernel's own geometry
    const int nd = g.front(t3geo, t2e);
    if (part && subs > 1 && !L.chunk) g.set_lead(nd, o0, t1);    // a time shard's launches (part != K1_ALL)
    const long n_seg = g.count(total);
    const long pl_shift = PLPAD + h->look;       // the general receiver sees the range h->look samples late (p25fe_recv.hip)
    // (halo form: the outputs a segment recomputes and drops may lie in front of planar position 0 -- with a 160-output halo the
    // range's first segment starts 80 positions in front of it; they are never stored, only whole bytes of the planes are)
    if (L.planar && !g.planar_ok(pl_shift)) return P25FE_ERR_ARG;
    if (L.planar && n_out_range > MAX_RANGE_BB) return P25FE_ERR_ARG;
    long seg_first = 0, seg_count = n_seg;
    if (L.part && L.power_dbm) return P25FE_ERR_ARG;
    if (part) {
        const long k_min = g.head_count(n_seg, nd, o0, t1);
        if (part == K1_MAIN) { seg_first = k_min; seg_count = n_seg - k_min; }
        else seg_count = k_min;
        p->head_end = g.start(k_min) - m_begin;
        p->empty = seg_count <= 0;
        if (p->empty) return P25FE_OK;
    }
    if (seg_count * (long)h->C > 0x7fffffffL) return P25FE_ERR_ARG;
    p->fmt = fmt; p->variant = variant; p->ct = ct; p->pk = pk; p->n_seg = n_seg;
    a.x = L.src; a.ch_stride = (long)L.ch_stride; a.n_hist = (long)L.n_hist; a.n_new = (long)L.n; a.o0 = (int)o0; a.n_ch = h->C;
    a.bb = L.bb; a.bb_stride = (long)L.bb_stride; a.power_partial = nullptr;
    a.subs_per_seg = g.subs_per_seg; a.seg_first = (int)seg_first; a.seg_count = (int)seg_count; a.lead_segs = g.lead_segs; a.seg_halo = g.segh;
    a.bbp = nullptr; a.bbp_ch_stride = 0; a.bits = nullptr; a.bits_ch_stride = 0; a.pl_shift = (int)pl_shift;
    a.done_flag = L.planar ? L.done_flag : nullptr; a.done_seq = L.done_seq;
    if (L.planar) {
        const PlanarGeo g(n_out_range);
        a.bbp = h->rx().pl_f.get(); a.bbp_ch_stride = (long)g.floats();
        a.bits = reinterpret_cast<uint8_t*>(h->rx().pl_bits.get()); a.bits_ch_stride = (long)(4 * g.words());   // (K1 stores the sign words' bytes)
    }
    // LDS per workgroup: [d carry | window] (+ taps: generic kernels) (+ the u8 table: generic u8 kernels, and specialised ones
    // whose table is not affine).  Immediate-coefficient kernels never touch the taps area at the end of the layout: not
    // allocated.  (13 376 B per wave is 11 waves per CU; a 12th would need 13 312 -- trimming to that changed nothing.)
    const bool lut = fmt == P25FE_FMT_U8 && (!ct || h->u8_lut_mode);
    p->lds = h->long_taps ? k1_lds_bytes<Geo<5, 1>>(ct, lut, t3geo) : (pk == 3 ? k1_lds_bytes<Geo<3>>(ct, lut, t3geo) : k1_lds_bytes<Geo<5>>(ct, lut, t3geo));
    // (experiments: extra dynamic LDS per workgroup = fewer resident waves per CU; the occupancy sensitivity of docs/MEASUREMENTS.md)
    static const size_t lds_pad_env = [] { const char* e = getenv("P25FE_K1_LDS_PAD"); return e ? (size_t)atol(e) : (size_t)0; }();
    p->lds += lds_pad_env;
    if (pair) p->lds = PairGeo::LDS;                                // (the pair kernel's own layout: 8 two-wave workgroups per CU)
    return P25FE_OK;
}

// The built-in kernels: one instantiation per (format, coefficient form, outputs per lane, output layout, long taps) in use.
// (Long taps are never the build's own numbers: the generic form, five outputs per lane; every planar kernel has five too.)
using K1Kernel = void (*)(K1Args, const Taps*);
using ChunkKernel = void (*)(K1Args, const Taps*, ChunkTail);
template <int FMT> static K1Kernel k1_kernel_of(bool ct, int pk, bool planar, bool long_taps)
{
    if (long_taps) return planar ? k_frontend<FMT, false, 5, OUT_PLANAR, 1> : k_frontend<FMT, false, 5, OUT_LINEAR, 1>;
    if (planar) return ct ? k_frontend<FMT, true, 5, OUT_PLANAR, 0> : k_frontend<FMT, false, 5, OUT_PLANAR, 0>;
    if (pk == 3) return ct ? k_frontend<FMT, true, 3, OUT_LINEAR, 0> : k_frontend<FMT, false, 3, OUT_LINEAR, 0>;
    return ct ? k_frontend<FMT, true, 5, OUT_LINEAR, 0> : k_frontend<FMT, false, 5, OUT_LINEAR, 0>;
}
template <int FMT> static ChunkKernel chunk_kernel_of(bool ct, bool long_taps)
{
    if (long_taps) return k_chunk<FMT, false, 1>;
    return ct ? k_chunk<FMT, true, 0> : k_chunk<FMT, false, 0>;
}
static K1Kernel k1_kernel_of(int fmt, bool ct, int pk, bool planar, bool long_taps)
{
    switch (fmt) {
    case P25FE_FMT_U8: return k1_kernel_of<P25FE_FMT_U8>(ct, pk, planar, long_taps);
    case P25FE_FMT_S16: return k1_kernel_of<P25FE_FMT_S16>(ct, pk, planar, long_taps);
    default: return k1_kernel_of<P25FE_FMT_CF32>(ct, pk, planar, long_taps);
    }
}
static ChunkKernel chunk_kernel_of(int fmt, bool ct, bool long_taps)
{
    switch (fmt) {
    case P25FE_FMT_U8: return chunk_kernel_of<P25FE_FMT_U8>(ct, long_taps);
    case P25FE_FMT_S16: return chunk_kernel_of<P25FE_FMT_S16>(ct, long_taps);
    default: return chunk_kernel_of<P25FE_FMT_CF32>(ct, long_taps);
    }
}

static int launch_k1(p25fe_t* h, const K1Launch& L)
{
    K1Plan p;
    if (int rc = k1_plan(h, L, &p)) return rc;
    if (L.head_end) *L.head_end = p.head_end;
    hipStream_t st = L.stream;
    if (p.empty) {
        // power_dbm of an empty chunk: the reference divides 0 by 0 (src/demod.rs:123-134) -> NaN (0xffffffff is a quiet NaN)
        if (L.power_dbm) HIPCHK(h, hipMemsetAsync(L.power_dbm, 0xff, sizeof(float) * (size_t)h->C, st));
        return P25FE_OK;
    }
    K1Args& a = p.a;
    if (L.power_dbm) {
        HIPCHK(h, h->power_partial.ensure(sizeof(float) * (size_t)h->C * (size_t)p.n_seg));
        a.power_partial = h->power_partial.as<float>();
    }
    ChunkTail tail;
    if (L.chunk) {
        if (!h->chunk_cnt.p) {                                      // the channels' arrival counters: zero between launches
            HIPCHK(h, h->chunk_cnt.ensure(sizeof(unsigned) * (size_t)h->C));
            HIPCHK(h, hipMemsetAsync(h->chunk_cnt.p, 0, sizeof(unsigned) * (size_t)h->C, h->stream));
        }
        tail.r = *L.chunk; tail.counter = h->chunk_cnt.as<unsigned>(); tail.wg_per_ch = a.seg_count;
    }
    const Taps* dt = h->d_taps.as<Taps>();
    const dim3 grid((unsigned)a.seg_count, (unsigned)h->C);          // one one-wave workgroup per (segment, channel)
    if (p.variant == P25FE_VARIANT_SPECIALIZED) {
        // kernels compiled for this handle's numbers (p25fe_jit.cpp): same source, same launch shape, C entry points (u8 and cf32)
        hipFunction_t f = h->jit_fn[p.fmt == P25FE_FMT_U8 ? 1 : 0][L.chunk ? 2 : (L.planar ? 1 : 0)];
        void* params[3] = {&a, &dt, &tail};
        if (L.ev0 || L.ev1)
            HIPCHK(h, hipExtModuleLaunchKernel(f, grid.x * WV, grid.y, 1, WV, 1, 1, p.lds, st, params, nullptr, L.ev0, L.ev1, 0));
        else
            HIPCHK(h, hipModuleLaunchKernel(f, grid.x, grid.y, 1, WV, 1, 1, (unsigned)p.lds, st, params, nullptr));
    } else if (L.chunk) {
        const ChunkKernel k = chunk_kernel_of(p.fmt, p.ct, h->long_taps);
        hipLaunchKernelGGL(k, grid, dim3(WV), p.lds, st, a, dt, tail);
    } else {
        const K1Kernel k = p.pair ? k_frontend_pair : k1_kernel_of(p.fmt, p.ct, p.pk, L.planar, h->long_taps);
        launch_ev(k, grid, dim3(p.pair ? 2 * WV : WV), p.lds, st, L.ev0, L.ev1, a, dt);
    }
    HIPCHK(h, hipGetLastError());
    if (L.power_dbm) {
        hipLaunchKernelGGL(k_power_finish, dim3((unsigned)h->C), dim3(256), 0, st, a.power_partial, (int)p.n_seg, a.n_out, L.power_dbm);
        HIPCHK(h, hipGetLastError());
    }
    return P25FE_OK;
}

// the current scratch set, large enough for n_bb owned baseband samples per channel
static int ensure_slice_scratch(p25fe_t* h, size_t n_bb)
{
    const size_t C = (size_t)h->C;
    const PlanarGeo g(n_bb);
    const size_t nt = C * g.n_tiles, ng = C * (size_t)n_groups_of((int)g.n_tiles);
    RxScratch& s = h->rx();
    HIPCHK(h, s.pl_f.ensure(C * g.floats())); HIPCHK(h, s.pl_bits.ensure(C * g.words()));
    HIPCHK(h, s.evl.ensure(nt * EVCAP)); HIPCHK(h, s.evthr.ensure(nt * EVTHR_N * 3));
    HIPCHK(h, s.recs.ensure(nt)); HIPCHK(h, s.tsum.ensure(nt)); HIPCHK(h, s.outs.ensure(nt));
    HIPCHK(h, s.gagg.ensure(ng)); HIPCHK(h, s.gpre.ensure(ng));
    const unsigned* before = s.gtick.get();
    HIPCHK(h, s.gtick.ensure(ng + C));
    if (s.gtick.get() != before) HIPCHK(h, hipMemset(s.gtick.get(), 0, s.gtick.buf.cap));    // a fresh buffer: the counters start at zero and return to it
    if (h->track || h->rs_n) {                                       // the general receiver's summaries and carry-ins
        HIPCHK(h, s.gsum.ensure(nt)); HIPCHK(h, s.gouts.ensure(nt)); HIPCHK(h, s.evg.ensure(nt * EVCAP));
        HIPCHK(h, s.gsg.ensure(ng)); HIPCHK(h, s.gpg.ensure(ng));
    }
    h->pl_lane = h->cur; h->pl_blocks = g.n_blocks;                  // what p25fe_debug_planes_dev reads back
    return P25FE_OK;
}

// The receive side (K2 .. K4) of the call being enqueued: the range on the planar scratch, where the results go, the receiver's
// options and which steps run.  h->rs_* (p25fe_resync_at_dev) is consumed by the call that runs the sync detection; a shard keeps
// its copy for pass 2.
struct RecvRange {
    size_t n_bb = 0;                            // owned baseband samples per channel
    long abs_bb0 = 0;                           // absolute index of the first PROCESSED sample = owned sample 0 minus h->look
    const p25fe_anchor_t* anchor_in = nullptr;  // nullable, [ch]
};
struct RecvDest {
    uint8_t* dibits = nullptr; size_t dibit_stride = 0;
    uint8_t* dibits2 = nullptr;                 // nullable: second destination of the dibits
    int64_t* sync_pos = nullptr; uint64_t* sync_dibit = nullptr;      // nullable, both or neither
    size_t sync_stride = 0;
    p25fe_result_t* result = nullptr;
};
struct RecvCall {
    bool gen = false;
    bool reslice = false;       // SPEC 3.8c: set by the entry points that hold the whole range (p25fe_run_dev*, p25fe_slice_dev)
    RecvOpt opt;
    RecvRange range;
    RecvDest dest;
    // detect: K2 runs in this call, and K3 whole behind it (k_scan_tiles / k_scan_tiles_g: group scans, then the range's).  Otherwise --
    // and for an empty range, whose record is the carry-in handed through -- the group summaries in the scratch are re-scanned
    // under range.anchor_in by the top step alone (k_range_scan / k_range_scan_g: a time shard's pass 2 under resolved anchors).
    bool detect = true;
    bool slice = true;          // K4 runs (a time shard's pass 1 stops behind K3)
    bool wait_head = false;     // K2's first tiles wait for the flag of a shard's head launch (p25fe_shard_pass1_head)
    // (nullable, fixed-stride receiver only) pass 2 of a time shard on pass 1's scan: no K3, the slicer applies the shard's carry-in in
    // closed form (ShardFix in p25fe_recv.hip) on top of the group's
    const ShardFix* fix = nullptr;
    hipEvent_t ev_done = nullptr;               // (nullable) fires when the last kernel of the chain has finished
    hipStream_t stream = nullptr;
};
static RecvCall recv_call(const p25fe_t* h)
{
    RecvCall c;
    c.opt.track = h->track;
    c.opt.n_resync = (int)h->rs_n;
    c.opt.resync = h->rs_idx;
    c.opt.resync_stride = (long)h->rs_stride;
    c.gen = h->track != 0 || h->rs_n != 0;
    return c;
}
static inline int n_tiles_of(const RecvRange& r) { return r.n_bb ? (int)PlanarGeo(r.n_bb).n_tiles : 0; }

static Planar planar_view(const p25fe_t* h, const PlanarGeo& g)
{
    Planar p;
    p.f = h->rx().pl_f.get(); p.f_ch = (long)g.floats();
    p.bits = h->rx().pl_bits.get(); p.bits_ch = (long)g.words();
    return p;
}

// The scratch buffers and the call's range / destination as the receive kernels' argument structs name them: every mapping that
// more than one struct shares is written here.
template <class A> static void view_planes(const p25fe_t* h, const RecvRange& r, A* a)       // K2, K4 (all forms), the chunk receiver
{
    a->pl = planar_view(h, PlanarGeo(r.n_bb)); a->n = (long)r.n_bb; a->abs0 = r.abs_bb0;
    a->evl = h->rx().evl.get(); a->evthr = h->rx().evthr.get();
}
template <class A> static void view_tiles(const p25fe_t* h, A* a) { a->recs = h->rx().recs.get(); a->tsum = h->rx().tsum.get(); }
template <class A> static void view_general(const p25fe_t* h, A* a) { a->gsum = h->rx().gsum.get(); a->evg = h->rx().evg.get(); }
template <class A> static void view_scan(const p25fe_t* h, const RecvCall& rc, A* a)         // K3, both receivers
{
    a->recs = h->rx().recs.get(); a->tickets = h->rx().gtick.get();
    a->n_tiles = n_tiles_of(rc.range); a->n = (long)rc.range.n_bb; a->abs0 = rc.range.abs_bb0; a->n_baseband = rc.range.n_bb;
    a->anchor_in = rc.range.anchor_in; a->result = rc.dest.result;
}
template <class A> static void view_dest(const RecvRange& r, const RecvDest& d, A* a)        // K4 (all forms), the chunk receiver
{
    a->anchor_in = r.anchor_in;
    a->dibits = d.dibits; a->dibit_stride = (long)d.dibit_stride;
    a->sync_pos = (d.sync_pos && d.sync_dibit) ? d.sync_pos : nullptr; a->sync_dibit = d.sync_dibit; a->sync_stride = (long)d.sync_stride;
}

// linear baseband (n_hist_bb valid samples before d_bb) -> the planar scratch
static int launch_planarize(p25fe_t* h, const float* d_bb, size_t bb_stride, size_t n_hist_bb, size_t n_bb, hipStream_t st)
{
    const PlanarGeo g(n_bb);
    PlanarizeArgs a;
    a.bb = d_bb; a.bb_stride = (long)bb_stride; a.n_hist = (long)n_hist_bb; a.n = (long)n_bb;
    a.f = h->rx().pl_f.get(); a.f_ch = (long)g.floats();
    a.bits = h->rx().pl_bits.get(); a.bits_ch = (long)g.words(); a.n_blocks = (long)g.n_blocks;
    a.shift = (int)h->look;
    hipLaunchKernelGGL(k_planarize, dim3((unsigned)((g.n_blocks + 1) / 2), (unsigned)h->C), dim3(WV * SPS), 0, st, a);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// K2 on the planar scratch
static int launch_detect(p25fe_t* h, const RecvCall& rc)
{
    DetArgs d;
    d.head_flag = nullptr; d.head_seq = 0u; d.head_tile_max = -1; d.head_err = nullptr;
    if (rc.wait_head) {
        d.head_flag = h->sh.flag.as<unsigned>(); d.head_seq = h->sh.seq; d.head_tile_max = h->sh.head_tile_max;
        d.head_err = h->sh.flag.as<unsigned>() + SH_FLAG_ERR;
    }
    view_planes(h, rc.range, &d); view_tiles(h, &d); view_general(h, &d);
    d.n_tiles = n_tiles_of(rc.range); d.opt = rc.opt;
    const dim3 grid((unsigned)d.n_tiles, (unsigned)h->C);
    if (rc.gen) hipLaunchKernelGGL(k_detect<true>, grid, dim3(WV), 0, rc.stream, d);
    else hipLaunchKernelGGL(k_detect<false>, grid, dim3(WV), 0, rc.stream, d);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// K3, either receiver.  SCAN_WHOLE: group scans, then the range's; SCAN_RANGE: the range's alone, on the group summaries that are
// there; SCAN_TILES_G: the general receiver's pass B, the tiles' carry-ins under their groups' (one wave per group).
enum ScanStep { SCAN_WHOLE, SCAN_RANGE, SCAN_TILES_G };
static int launch_scan(p25fe_t* h, const RecvCall& rc, ScanStep step, hipEvent_t ev_done)
{
    const dim3 grid = step == SCAN_RANGE ? dim3((unsigned)h->C) : dim3((unsigned)n_groups_of(n_tiles_of(rc.range)), (unsigned)h->C);
    if (rc.gen) {
        ScanArgsG c;
        view_scan(h, rc, &c);
        c.gsum = h->rx().gsum.get(); c.outs = h->rx().gouts.get(); c.gsg = h->rx().gsg.get(); c.gpg = h->rx().gpg.get();
        c.track = h->track;
        launch_ev(step == SCAN_WHOLE ? k_scan_tiles_g : step == SCAN_RANGE ? k_range_scan_g : k_scan_g_groups, grid, dim3(WV), 0, rc.stream,
                  nullptr, ev_done, c);
    } else {
        ScanArgs c;
        view_scan(h, rc, &c);
        c.tsum = h->rx().tsum.get(); c.outs = h->rx().outs.get(); c.gagg = h->rx().gagg.get(); c.gpre = h->rx().gpre.get();
        launch_ev(step == SCAN_WHOLE ? k_scan_tiles : k_range_scan, grid, dim3(WV), 0, rc.stream, nullptr, ev_done, c);
    }
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// K4, fixed-stride receiver
static int launch_slice(p25fe_t* h, const RecvCall& rc)
{
    SliceArgs l;
    view_planes(h, rc.range, &l); view_tiles(h, &l); view_dest(rc.range, rc.dest, &l);
    l.n_tiles = n_tiles_of(rc.range); l.outs = h->rx().outs.get(); l.gpre = h->rx().gpre.get(); l.dibits2 = rc.dest.dibits2;
    if (rc.fix) l.fix = *rc.fix; else memset(&l.fix, 0, sizeof l.fix);
    // (pass 2 of a time shard: one extra workgroup runs the combine for the record beside the slicing ones)
    launch_ev(k_slice, dim3((unsigned)l.n_tiles + (rc.fix ? 1u : 0u), (unsigned)h->C), dim3(WV), 0, rc.stream, nullptr, rc.ev_done, l);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// K4, general receiver (tracking clock / lock drops), on the carry-ins of SCAN_TILES_G
static int launch_slice_g(p25fe_t* h, const RecvCall& rc)
{
    SliceArgsG l;
    view_planes(h, rc.range, &l); view_general(h, &l); view_dest(rc.range, rc.dest, &l);
    l.n_tiles = n_tiles_of(rc.range); l.outs = h->rx().gouts.get(); l.recs = h->rx().recs.get();
    l.track = h->track; l.dibits2 = rc.dest.dibits2;
    launch_ev(k_slice_g, dim3((unsigned)l.n_tiles, (unsigned)h->C), dim3(WV), 0, rc.stream, nullptr, rc.ev_done, l);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// SPEC 3.8c: the slicer by detection (k_ev_collect / k_ev_count / k_ev_scan / k_ev_slice) on the same carry-ins
static int launch_slice_by_detection(p25fe_t* h, const RecvCall& rc)
{
    const size_t C = (size_t)h->C, n_bb = rc.range.n_bb;
    const int n_tiles = n_tiles_of(rc.range);
    hipStream_t st = rc.stream;
    size_t cap_ev = (size_t)n_tiles * EVCAP;
    const size_t bound = n_bb / (size_t)(W + 1) + (size_t)n_tiles + 8;
    if (bound < cap_ev) cap_ev = bound;
    const size_t stride = cap_ev + 2;
    HIPCHK(h, h->evrec.ensure(C * stride * sizeof(EvRec)));
    HIPCHK(h, h->evoff.ensure(C * (stride + 1) * sizeof(unsigned long long)));
    {
        const void* before = h->evnext.p;
        HIPCHK(h, h->evnext.ensure(C * stride * sizeof(EvNext)));
        if (h->evnext.p != before) HIPCHK(h, hipMemsetAsync(h->evnext.p, 0, h->evnext.cap, st));   // sequence numbers start above 0
    }
    EvArgs e;
    view_planes(h, rc.range, &e); view_general(h, &e); view_dest(rc.range, rc.dest, &e);
    e.n_tiles = n_tiles; e.outs = h->rx().gouts.get();
    e.rec = h->evrec.as<EvRec>(); e.nxt = h->evnext.as<EvNext>(); e.off = h->evoff.as<unsigned long long>();
    e.ev_stride = (long)stride; e.seq = ++h->ev_seq; e.result = rc.dest.result;
    hipLaunchKernelGGL(k_ev_collect, dim3((unsigned)n_tiles, (unsigned)h->C), dim3(WV), 0, st, e);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ev_count, dim3((unsigned)(n_tiles < 1024 ? n_tiles : 1024), (unsigned)h->C), dim3(WV), 0, st, e);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ev_scan, dim3((unsigned)h->C), dim3(WV), 0, st, e);
    HIPCHK(h, hipGetLastError());
    // (a tracked period is within 1 / 1024 of the nominal one over long intervals and at least 9 samples over the shortest)
    const size_t max_dibits = n_bb / (SPS - 1) + (size_t)n_tiles + 64;
    const size_t lim = rc.dest.dibit_stride < max_dibits ? rc.dest.dibit_stride : max_dibits;
    launch_ev(k_ev_slice, dim3((unsigned)((lim + WV * 4 - 1) / (WV * 4)), (unsigned)h->C), dim3(WV), 0, st, nullptr, rc.ev_done, e);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// The receive chain on the planar scratch: K2 (rc.detect), K3, K4 (rc.slice) in order, with the profiling marks behind each.
// rc.ev_done rides on the LAST kernel launched; if none was, it is recorded on the stream.
static int launch_recv(p25fe_t* h, const RecvCall& rc)
{
    const int n_tiles = n_tiles_of(rc.range);
    const bool detect = rc.detect && n_tiles != 0, slice = rc.slice && n_tiles != 0, scan = rc.fix == nullptr;
    hipStream_t st = rc.stream;
    int e = detect ? launch_detect(h, rc) : P25FE_OK;
    if (e) return e;
    h->prof.mark(2, st, h->ext_events);
    if (scan && (e = launch_scan(h, rc, detect ? SCAN_WHOLE : SCAN_RANGE, slice ? nullptr : rc.ev_done)) != P25FE_OK) return e;
    h->prof.mark(3, st, h->ext_events);
    if (slice) {
        if (!rc.gen) e = launch_slice(h, rc);
        else if ((e = launch_scan(h, rc, SCAN_TILES_G, nullptr)) == P25FE_OK) e = rc.reslice ? launch_slice_by_detection(h, rc) : launch_slice_g(h, rc);
        if (e) return e;
    }
    if (rc.ev_done && !scan && !slice) HIPCHK(h, hipEventRecord(rc.ev_done, st));
    h->prof.mark(4, st, h->ext_events);
    return P25FE_OK;
}

// K1 into the planar scratch (nothing if the range holds no baseband sample), under the open profiling slot's event pair.
// k1_done (nullable): fires when K1 has finished -- riding on its dispatch if h->ext_events -- and `waiter` waits for it.
static int launch_k1_planar(p25fe_t* h, K1Launch& k, hipEvent_t k1_done, hipStream_t waiter)
{
    h->prof.mark(0, k.stream, h->ext_events);
    bool attached = false;
    if (p25fe_n_baseband_h(h, k.abs0, k.n)) {
        h->prof.k1_events(h->ext_events, &k.ev0, &k.ev1);
        if (k1_done && h->ext_events) {
            if (k.ev1) k1_done = k.ev1;                             // a sampled call: the profiling stop event doubles as "K1 done"
            else k.ev1 = k1_done;
            attached = true;
        }
        k.planar = true;
        if (int rc = launch_k1(h, k)) return rc;
    }
    if (k1_done) {
        if (!attached) HIPCHK(h, hipEventRecord(k1_done, k.stream));
        HIPCHK(h, hipStreamWaitEvent(waiter, k1_done, 0));
    }
    return P25FE_OK;
}

// Planar front end, then the receive chain (on rc.stream, which may be another stream than K1's: then k1_done orders the two)
static int launch_planar_recv(p25fe_t* h, K1Launch& k, const RecvCall& rc, hipEvent_t k1_done = nullptr)
{
    if (int e = launch_k1_planar(h, k, k1_done, rc.stream)) return e;
    if (rc.range.n_bb) h->prof.mark(1, k.stream, h->ext_events);
    return launch_recv(h, rc);
}

// SPEC 3.8c needs the whole range in one call.  The calls that see the stream in pieces (host streaming chunks, host windows, the
// passes of a time shard) can only run 3.8b's causal rule; a handle that asked for 3.8c gets that ONLY if it said so
// (P25FE_CLOCK_CAUSAL_OK) -- otherwise the call is refused instead of quietly returning another receiver's dibits.
static inline bool piecewise_refused(const p25fe_t* h) { return h->track == P25FE_CLOCK_TRACKING_RESLICE && !h->causal_ok; }

// --------------------------------------------------------------------------------------------
// K0 and K6 launches: one function per stage for every wideband format (h and fmt are checked by the caller).  The conversion's
// numbers are kernel arguments; a u8 table the handle could not recognise as affine is read from its device copy.
// --------------------------------------------------------------------------------------------
static WideConv wide_conv_of(const p25fe_t* h)
{
    WideConv cv;
    cv.scale = h->u8_scale; cv.offset = h->u8_offset;
    cv.lut = h->u8_lut_mode ? h->d_taps.as<Taps>()->lut : nullptr;
    return cv;
}
static inline bool wide_fmt_known(int fmt) { return fmt == P25FE_FMT_CF32 || fmt == P25FE_FMT_S16 || fmt == P25FE_FMT_U8; }
static inline int wide_o0(uint64_t abs0) { return (int)((PD - 1 + PD - abs0 % PD) % PD); }   // first decimation instant of the range

static int launch_k0(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                     float* d_out, size_t out_stride, hipStream_t st)
{
    if (!d_iq || !d_out || position_refused(abs0)) return P25FE_ERR_ARG;
    // the kernels fetch aligned 16-byte vectors: channel rows are whole vectors (2 cf32, 4 s16, 8 u8 samples)
    if ((reinterpret_cast<uintptr_t>(d_iq) & 15u) != 0 || (h->C > 1 && ch_stride % fmt_stride_unit(fmt) != 0)) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n_out = p25fe_n_predecim(abs0, n);
    if (n_out == 0) return P25FE_OK;
    K0Args a;
    a.x = static_cast<const float*>(d_iq); a.ch_stride = (long)ch_stride; a.n_hist = (long)n_hist; a.n_new = (long)n;   // (x: addressed by the format's bytes)
    a.o0 = wide_o0(abs0);
    a.y = d_out; a.y_stride = (long)out_stride; a.n_out = (long)n_out;
    const size_t per_wg = (size_t)K0_SUB * K0_SUBS;
    const dim3 grid((unsigned)((n_out + per_wg - 1) / per_wg), (unsigned)h->C);
    const WideConv cv = wide_conv_of(h);
    if (fmt == P25FE_FMT_CF32) hipLaunchKernelGGL(k_predecim, grid, dim3(WV), 0, st, a);
    else if (fmt == P25FE_FMT_S16) hipLaunchKernelGGL((k_predecim_fmt<P25FE_FMT_S16, false>), grid, dim3(WV), 0, st, a, cv);
    else if (cv.lut) hipLaunchKernelGGL((k_predecim_fmt<P25FE_FMT_U8, true>), grid, dim3(WV), 0, st, a, cv);
    else hipLaunchKernelGGL((k_predecim_fmt<P25FE_FMT_U8, false>), grid, dim3(WV), 0, st, a, cv);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

static int launch_k6(p25fe_t* h, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs0, float* d_out,
                     size_t out_stride, hipStream_t st)
{
    static_assert(P25FE_CHZ_CHANNELS_ABI == CZ_M, "header and spec disagree");
    if (!d_iq || !d_out || position_refused(abs0)) return P25FE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 7u) != 0) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n_out = p25fe_n_predecim(abs0, n);
    if (n_out == 0) return P25FE_OK;
    if (out_stride < round_up(n_out, (size_t)WV)) return P25FE_ERR_ARG;      // rows are written in whole 64-instant tiles
    ChzArgs a;
    a.x = static_cast<const float*>(d_iq); a.n_hist = (long)n_hist; a.n_new = (long)n; a.abs0 = (long)abs0;
    a.o0 = wide_o0(abs0);
    a.y = d_out; a.y_stride = (long)out_stride; a.n_out = (long)n_out;
    const dim3 grid((unsigned)((n_out + WV - 1) / WV));
    const WideConv cv = wide_conv_of(h);
    if (fmt == P25FE_FMT_CF32) hipLaunchKernelGGL(k_channelise, grid, dim3(WV), 0, st, a);
    else if (fmt == P25FE_FMT_S16) hipLaunchKernelGGL((k_channelise_fmt<P25FE_FMT_S16, false>), grid, dim3(WV), 0, st, a, cv);
    else if (cv.lut) hipLaunchKernelGGL((k_channelise_fmt<P25FE_FMT_U8, true>), grid, dim3(WV), 0, st, a, cv);
    else hipLaunchKernelGGL((k_channelise_fmt<P25FE_FMT_U8, false>), grid, dim3(WV), 0, st, a, cv);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// --------------------------------------------------------------------------------------------
// Rational resampler (SPEC 3.0b; kernel: k_resample) and tuner (SPEC 3.0c; kernel: k_tune).  The tuner is the resampler with a mixer
// in front, on the device and here: RsCore is what both objects hold -- the ratio, the table's device copy in the kernel's layout,
// and the state of the host streaming form (position, format, the last T - 1 samples per input row as they came in).  The resampler
// is C input rows to C output rows; the tuner is ONE input row to K output rows, plus the channels' frequencies: one rotator table per
// distinct denominator and the per-channel numbers (TuneCh) in device memory.  A tuner of NCO channels (SPEC 3.0d; kernel:
// k_tune_nco) is the same object with another kind: ONE rotator table, of denominator 256, and a step and a phase offset per channel
// in TuneCh (SPEC 3.0e): the host keeps (step, ph0) per channel, and p25fe_afc_set_step rewrites a channel's record in stream order.
// --------------------------------------------------------------------------------------------
struct RsCore {
    p25fe_t* h = nullptr;
    int device = 0;                        // h's, kept here: destroying the object must not read the handle
    int L = 0, M = 0, T = 0, TP = 0;
    size_t rows_in = 0;                    // input rows: the handle's channels (resampler), 1 (tuner)
    DevBuf d_taps, d_in, d_out;
    uint64_t pos = 0;                      // samples consumed per row
    int fmt = -1;                          // format of the stream (-1: none yet)
    std::vector<unsigned char> stage;      // host image of the device rows of one streaming call
    std::vector<unsigned char> hist;       // [rows_in][T - 1] samples in the stream's format, oldest first (the valid ones are the last min(pos, T - 1))
};
struct p25fe_resampler : RsCore {};
struct p25fe_tuner : RsCore {
    int K = 0;
    int mix = MIX_RATIONAL;                // the kind, as the kernel's MIX: rational channels (k_tune) or NCO channels (k_tune_nco)
    int rot_off = 0;                       // floats of dynamic LDS in front of the rotator's copy
    size_t lds = 0;                        // dynamic LDS of a launch: the table, and the largest rotator that is copied there
    DevBuf d_rot, d_ch;
    std::vector<int32_t> step;             // NCO channels: the current step ...
    std::vector<uint32_t> ph0;             // ... and phase offset of every channel, as the launches issued from now on see them
    hipEvent_t ev = nullptr;               // orders a record's update between the handle's stream and the default stream (made on first use)
    bool stale = false;                    // a tracking loop has rewritten the device records since step / ph0 were last read back
    ~p25fe_tuner() { if (ev) (void)hipEventDestroy(ev); }
};
// The frequency measure of SPEC 3.0f (kernel: k_afc_measure): the prefilter's taps on the device and the shape
struct p25fe_afc {
    p25fe_t* h = nullptr;
    int device = 0;
    int D = 0, T = 0, K = 0;
    DevBuf d_taps;
};
// The tracking loop of SPEC 3.0g (kernel: k_afc_loop): a tuner of NCO channels, a measure, and per channel the open record, the
// state and the step the loop was made at, all on the device
struct p25fe_track {
    p25fe_t* h = nullptr;
    int device = 0;
    p25fe_tuner* tn = nullptr;
    p25fe_afc* afc = nullptr;
    p25fe_track_cfg_t cfg{};
    int K = 0;
    DevBuf d_acc, d_state, d_ref;
};
static_assert(sizeof(p25fe_track_cfg_t) == 32 && sizeof(p25fe_track_state_t) == 32 && sizeof(p25fe_afc_acc_t) == 32, "32-byte records");
static bool afc_shape_ok(int64_t D, int64_t T)
{
    return D >= P25FE_AFC_MIN_D && D <= P25FE_AFC_MAX_D && T >= 1 && T <= P25FE_AFC_MAX_T;
}

static uint64_t gcd_u64(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }
static bool rs_ratio_ok(int64_t L, int64_t M)
{
    if (L < 1 || L > P25FE_RS_MAX_L || M <= L || M > P25FE_RS_MAX_M) return false;
    return gcd_u64((uint64_t)M, (uint64_t)L) == 1;
}
static bool rs_shape_ok(int64_t L, int64_t M, int64_t T)
{
    return rs_ratio_ok(L, M) && T >= 1 && T <= P25FE_RS_MAX_T && L * T <= P25FE_RS_MAX_TABLE;
}
// floor(a L / M) without a 64-bit product that overflows (M <= 1024, L <= 32)
static inline uint64_t rs_floor(uint64_t a, uint64_t L, uint64_t M) { return (a / M) * L + ((a % M) * L) / M; }
// modified Bessel function I0 from its power series (terms fall below 1e-17 of the sum well inside 64 of them at beta = 7)
static double rs_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; ++k) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
    return s;
}
// The Kaiser-windowed sinc (beta = 7) of both design calls: N taps of cutoff fc (cycles per sample), hd[k] = g sinc w, scaled to sum s
static void rs_kaiser_sinc(size_t N, double fc, double g, double s, float* taps)
{
    const double pi = 3.14159265358979323846;
    const double mid = ((double)N - 1.0) / 2.0, den = rs_i0(7.0);
    std::vector<double> hd(N);
    double sum = 0.0;
    for (size_t k = 0; k < N; ++k) {
        const double x = (double)k - mid, arg = 2.0 * fc * x;
        const double sinc = arg == 0.0 ? 1.0 : sin(pi * arg) / (pi * arg);
        const double r = N > 1 ? x / mid : 0.0;
        const double w = rs_i0(7.0 * sqrt(r * r < 1.0 ? 1.0 - r * r : 0.0)) / den;
        hd[k] = g * sinc * w;
        sum += hd[k];
    }
    for (size_t k = 0; k < N; ++k) taps[k] = (float)(hd[k] * s / sum);
}
// num / den in lowest terms inside the tuner's limits (0 / 1 is the centre)
static bool tn_freq_ok(int64_t num, int64_t den)
{
    if (den < 1 || den > P25FE_TUNE_MAX_DEN) return false;
    const int64_t an = num < 0 ? -num : num;
    return 2 * an <= den && gcd_u64((uint64_t)an, (uint64_t)den) == 1;
}

// The end of both tuner constructors: the rotators' host image (interleaved (cos, sin) pairs) and the channels' records to the
// device, and the dynamic LDS of a launch (lds_den: the largest denominator whose rotator is copied there).  ch[k] comes with
// everything but its rotator's address, which is pair at[k] of the image.  On failure tn is gone.
static int tn_finish(p25fe_tuner* tn, const std::vector<float>& rot, std::vector<TuneCh>& ch, const std::vector<long>& at, int lds_den,
                     p25fe_tuner_t** out)
{
    tn->rot_off = (int)round_up((size_t)tn->L * tn->TP, 2);
    tn->lds = sizeof(float) * ((size_t)tn->rot_off + 2 * (size_t)lds_den);
    if (tn->d_rot.ensure(rot.size() * sizeof(float)) == hipSuccess && tn->d_ch.ensure(ch.size() * sizeof(TuneCh)) == hipSuccess) {
        for (size_t k = 0; k < ch.size(); ++k) ch[k].rot = tn->d_rot.as<float2>() + at[k];
        if (hipMemcpy(tn->d_rot.p, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(tn->d_ch.p, ch.data(), ch.size() * sizeof(TuneCh), hipMemcpyHostToDevice) == hipSuccess) {
            *out = tn;
            return P25FE_OK;
        }
    }
    tn->h->last_hip = (int)hipGetLastError();
    delete tn;
    return P25FE_ERR_HIP;
}

// A new object of either kind: the shape and the table are checked first (they need no handle, and no device is touched before
// they pass), then the table goes to the device in the kernel's layout.  *out stays null on any failure.
template <class Obj>
static int rs_create(Obj** out, p25fe_t* h, int32_t L, int32_t M, int32_t T, const float* taps, size_t rows_in)
{
    if (!rs_shape_ok(L, M, T) || !taps) return P25FE_ERR_ARG;
    for (int k = 0; k < L * T; ++k) if (!finite_f(taps[k])) return P25FE_ERR_ARG;
    if (!h) return P25FE_ERR_ARG;
    Obj* o = new (std::nothrow) Obj;
    if (!o) return P25FE_ERR_NOMEM;
    o->h = h; o->device = h->cfg.device; o->L = L; o->M = M; o->T = T; o->TP = rs_tap_pitch(T); o->rows_in = rows_in;
    // the kernel's layout: phase-major rows of pitch TP, the pad zero
    std::vector<float> tab((size_t)L * o->TP, 0.0f);
    for (int p = 0; p < L; ++p) for (int j = 0; j < T; ++j) tab[(size_t)p * o->TP + j] = taps[(size_t)j * L + p];
    o->hist.assign(rows_in * (size_t)(T - 1) * 8, 0);
    if (hipSetDevice(h->cfg.device) != hipSuccess || o->d_taps.ensure(tab.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(o->d_taps.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        h->last_hip = (int)hipGetLastError(); delete o; return P25FE_ERR_HIP;
    }
    *out = o;
    return P25FE_OK;
}

// the kernel's arguments for one range of the stream (everything but the tuner's own)
static void rs_fill_args(const RsCore* o, RsArgs& a, const void* d_iq, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs_first,
                         float* d_out, size_t out_stride, size_t n_out)
{
    const int L = o->L, M = o->M, T = o->T;
    a.x = d_iq; a.ch_stride = (long)ch_stride; a.n_hist = (long)n_hist; a.n_new = (long)n;
    a.y = d_out; a.y_stride = (long)out_stride; a.n_out = (long)n_out;
    a.taps = o->d_taps.as<float>(); a.L = L; a.M = M; a.T = T; a.TP = o->TP;
    // owned output 0 is output floor(abs_first L / M) of the stream; with abs_first = qa M + ra it is output qa L + mr, whose
    // u = (qa L + mr) M + M - 1: its input index is qa M + (mr M + M - 1) div L -- only ra matters (the position grid of the
    // resampler is M; the tuner's mixer takes the whole position)
    const int ra = (int)(abs_first % (uint64_t)M), mr = ra * L / M, ur = mr * M + M - 1;
    a.p0 = ur % L; a.d0 = ur / L - ra;
    // the sub-tile fits the window: its last output's newest sample sits at position <= (L - 1 + (tile - 1) M) / L + T - 1 < RS_NIN
    const int fit = 1 + (RS_NIN - T) * L / M;
    a.gl = WV - WV % L;
    if (fit >= a.gl) { a.R = fit / a.gl < RS_R ? fit / a.gl : RS_R; a.tile = a.gl * a.R; }
    else { a.R = 1; a.tile = fit; }
}

// what a launch refuses about its pointers: the position, the alignment of both, and, where there is more than one input row,
// the rows' distance
static bool rs_pointers_refused(const RsCore* o, const void* d_iq, int fmt, size_t ch_stride, uint64_t abs_first, const float* d_out)
{
    if (!d_iq || !d_out || position_refused(abs_first)) return true;
    return (reinterpret_cast<uintptr_t>(d_iq) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 7u) != 0 ||
           (o->rows_in > 1 && ch_stride % fmt_stride_unit(fmt) != 0);
}

// the kernel of a MIX value (the resampler takes the tuner's arguments' first part)
template <int MIX, int FMT, bool LUTM>
static void rs_launch_as(dim3 grid, size_t lds, hipStream_t st, const TuneArgs& ta, const WideConv& cv)
{
    if constexpr (MIX == MIX_NONE) hipLaunchKernelGGL((k_resample<FMT, LUTM>), grid, dim3(WV), lds, st, ta.r, cv);
    else if constexpr (MIX == MIX_RATIONAL) hipLaunchKernelGGL((k_tune<FMT, LUTM>), grid, dim3(WV), lds, st, ta, cv);
    else hipLaunchKernelGGL((k_tune_nco<FMT, LUTM>), grid, dim3(WV), lds, st, ta, cv);
}
// ... and its instance for a format: cf32, s16, u8 with the table as arithmetic or looked up
template <int MIX>
static void rs_dispatch(int fmt, dim3 grid, size_t lds, hipStream_t st, const TuneArgs& ta, const WideConv& cv)
{
    if (fmt == P25FE_FMT_CF32) rs_launch_as<MIX, P25FE_FMT_CF32, false>(grid, lds, st, ta, cv);
    else if (fmt == P25FE_FMT_S16) rs_launch_as<MIX, P25FE_FMT_S16, false>(grid, lds, st, ta, cv);
    else if (cv.lut) rs_launch_as<MIX, P25FE_FMT_U8, true>(grid, lds, st, ta, cv);
    else rs_launch_as<MIX, P25FE_FMT_U8, false>(grid, lds, st, ta, cv);
}

// One range through k_resample (tn null: o->rows_in rows in and out) or k_tune / k_tune_nco (tn is o: one row in, tn->K rows out).
static int rs_launch(RsCore* o, const p25fe_tuner* tn, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n,
                     uint64_t abs_first, float* d_out, size_t out_stride, hipStream_t st)
{
    p25fe_t* h = o->h;
    if (rs_pointers_refused(o, d_iq, fmt, ch_stride, abs_first, d_out)) return P25FE_ERR_ARG;
    const size_t n_out = p25fe_n_resample(o->L, o->M, abs_first, n);
    if (out_stride < n_out) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_out == 0) return P25FE_OK;
    TuneArgs ta;
    rs_fill_args(o, ta.r, d_iq, ch_stride, n_hist, n, abs_first, d_out, out_stride, n_out);
    const size_t per_wg = (size_t)ta.r.tile * RS_SUBS, groups = (n_out + per_wg - 1) / per_wg;
    dim3 grid((unsigned)groups, (unsigned)o->rows_in);
    if (tn) {
        ta.ch = tn->d_ch.as<TuneCh>(); ta.K = tn->K; ta.rot_off = tn->rot_off; ta.abs_first = abs_first;
        // workgroup index = sub-tile group * K + channel: the channel varies fastest.  Groups beyond grid.x's range go to grid.y
        const size_t gx = std::min(groups, (size_t)0x7fffffffu / (size_t)tn->K), gy = (groups + gx - 1) / gx;
        if (gy > 65535) return P25FE_ERR_ARG;
        grid = dim3((unsigned)(gx * (size_t)tn->K), (unsigned)gy);
    }
    const WideConv cv = wide_conv_of(h);
    (void)hipGetLastError();                                        // the check below is for THIS launch: drop what an earlier call of the thread left behind
    if (!tn) rs_dispatch<MIX_NONE>(fmt, grid, sizeof(float) * (size_t)o->L * (size_t)o->TP, st, ta, cv);
    else if (tn->mix == MIX_RATIONAL) rs_dispatch<MIX_RATIONAL>(fmt, grid, tn->lds, st, ta, cv);
    else rs_dispatch<MIX_NCO>(fmt, grid, tn->lds, st, ta, cv);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// The host streaming call of either object (tn as in rs_launch): n new samples of each input row, *n_out outputs in each output row
// (row r at out + r * cap).  The state (history, position, format) moves on whether or not the range yields an output.
static int rs_stream(RsCore* o, const p25fe_tuner* tn, const void* iq, int fmt, size_t n, float* out, size_t cap, size_t* n_out)
{
    if (!o || !o->h || !n_out || !wide_fmt_known(fmt) || (n && !iq)) return P25FE_ERR_ARG;
    if (o->fmt >= 0 && fmt != o->fmt) return P25FE_ERR_FORMAT;
    if (position_refused(o->pos) || n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    p25fe_t* h = o->h;
    const size_t C = o->rows_in, rows_out = tn ? (size_t)tn->K : C, bps = fmt_bytes(fmt), keep = (size_t)o->T - 1;
    const size_t no = p25fe_n_resample(o->L, o->M, o->pos, n);
    *n_out = no;
    if (no > cap || (no && !out)) return P25FE_ERR_CAPACITY;
    const size_t n_hist = o->pos < keep ? (size_t)o->pos : keep;
    const unsigned char* src = static_cast<const unsigned char*>(iq);
    if (no) {
        // device rows: [history, right-aligned in `lead` slots | n new samples], owned sample 0 of every row 16-byte aligned
        const size_t lead = round_up(keep, 8), stride = lead + round_up(n, 8);
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, o->d_in.ensure(C * stride * bps));
        HIPCHK(h, o->d_out.ensure(rows_out * no * sizeof(float) * 2));
        unsigned char* din = o->d_in.as<unsigned char>();
        // the rows are put together on the host and go over in ONE copy (no transfers of a few bytes to odd addresses)
        o->stage.assign(C * stride * bps, 0);
        for (size_t c = 0; c < C; ++c) {
            unsigned char* row = o->stage.data() + c * stride * bps;
            if (n_hist) memcpy(row + (lead - n_hist) * bps, o->hist.data() + (c * keep + keep - n_hist) * bps, n_hist * bps);
            memcpy(row + lead * bps, src + c * n * bps, n * bps);
        }
        HIPCHK(h, hipMemcpyAsync(din, o->stage.data(), o->stage.size(), hipMemcpyHostToDevice, h->stream));
        if (int rc = rs_launch(o, tn, din + lead * bps, fmt, stride, n_hist, n, o->pos, o->d_out.as<float>(), no, h->stream)) return rc;
        for (size_t r = 0; r < rows_out; ++r)
            HIPCHK(h, hipMemcpyAsync(out + r * cap * 2, o->d_out.as<float>() + r * no * 2, no * sizeof(float) * 2, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    // the state moves: the last T - 1 samples of [history | new]
    for (size_t c = 0; keep && c < C; ++c) {
        unsigned char* hc = o->hist.data() + c * keep * bps;
        if (n >= keep) memcpy(hc, src + (c * n + n - keep) * bps, keep * bps);
        else { memmove(hc, hc + n * bps, (keep - n) * bps); memcpy(hc + (keep - n) * bps, src + c * n * bps, n * bps); }
    }
    o->pos += n; o->fmt = fmt;
    return P25FE_OK;
}

template <class Obj>
static void rs_destroy(Obj* o)
{
    if (!o) return;
    (void)hipSetDevice(o->device);
    delete o;
}
static int rs_reset(RsCore* o)
{
    if (!o) return P25FE_ERR_ARG;
    o->pos = 0; o->fmt = -1;
    std::fill(o->hist.begin(), o->hist.end(), (unsigned char)0);
    return P25FE_OK;
}

extern "C" {

int p25fe_resampler_design(uint32_t fs_in_hz, int32_t* L, int32_t* M, int32_t* T, float* taps, size_t cap)
{
    if (!L || !M || !T || fs_in_hz == 0) return P25FE_ERR_ARG;
    const uint64_t a = gcd_u64(P25FE_RS_RATE_OUT_HZ, fs_in_hz);
    const int64_t l = (int64_t)(P25FE_RS_RATE_OUT_HZ / a), m = (int64_t)(fs_in_hz / a);
    const int64_t t = ((int64_t)fs_in_hz + 29999) / 30000;
    if (!rs_shape_ok(l, m, t)) return P25FE_ERR_ARG;
    *L = (int32_t)l; *M = (int32_t)m; *T = (int32_t)t;
    const size_t N = (size_t)(l * t);
    if (cap < N || !taps) return P25FE_ERR_CAPACITY;
    const double fc = 60000.0 / ((double)l * (double)fs_in_hz);       // cutoff in cycles per sample of the prototype's rate
    rs_kaiser_sinc(N, fc, 2.0 * fc, (double)l, taps);                 // the prototype's gain 2 fc, every phase's taps sum to 1
    return P25FE_OK;
}

size_t p25fe_n_resample(int32_t L, int32_t M, uint64_t abs_first, size_t n)
{
    if (!rs_ratio_ok(L, M)) return 0;
    // floor((abs_first + n) L / M) - floor(abs_first L / M) with abs_first + n split so that no sum wraps: the quotients and
    // the remainders add up separately
    const uint64_t l = (uint64_t)L, m = (uint64_t)M;
    const uint64_t ra = abs_first % m, qn = (uint64_t)n / m, rn = (uint64_t)n % m;
    // abs_first = qa m + ra, end = (qa + qn) m + (ra + rn): floor(end l / m) = (qa + qn) l + floor((ra + rn) l / m), and qa l cancels
    return (size_t)(qn * l + ((ra + rn) * l) / m - (ra * l) / m);
}

int p25fe_resampler_create(p25fe_t* h, int32_t L, int32_t M, int32_t T, const float* taps, p25fe_resampler_t** out)
{
    if (out) *out = nullptr;
    if (!out) return P25FE_ERR_ARG;
    return rs_create(out, h, L, M, T, taps, h ? (size_t)h->C : 0);
}

void p25fe_resampler_destroy(p25fe_resampler_t* rs) { rs_destroy(rs); }

int p25fe_resampler_reset(p25fe_resampler_t* rs) { return rs_reset(rs); }

int p25fe_resample_dev(p25fe_resampler_t* rs, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs_first,
                       float* d_out, size_t out_stride, void* stream)
{
    if (!rs || !rs->h || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    return rs_launch(rs, nullptr, d_iq, fmt, ch_stride, n_hist, n, abs_first, d_out, out_stride, (hipStream_t)stream);
}

int p25fe_resample(p25fe_resampler_t* rs, const void* iq, int fmt, size_t n, float* out, size_t cap, size_t* n_out)
{
    return rs_stream(rs, nullptr, iq, fmt, n, out, cap, n_out);
}

int p25fe_tuner_freq(uint32_t fs_in_hz, int64_t offset_hz, int32_t* num, int32_t* den)
{
    if (!num || !den || fs_in_hz == 0) return P25FE_ERR_ARG;
    const uint64_t ao = offset_hz < 0 ? 0 - (uint64_t)offset_hz : (uint64_t)offset_hz;
    if (ao > fs_in_hz || 2 * ao > fs_in_hz) return P25FE_ERR_ARG;
    const uint64_t g = gcd_u64(ao, fs_in_hz);                       // gcd(0, fs) = fs: the centre is 0 / 1
    const uint64_t d = fs_in_hz / g, nn = ao / g;
    if (d > P25FE_TUNE_MAX_DEN) return P25FE_ERR_ARG;
    *num = offset_hz < 0 ? -(int32_t)nn : (int32_t)nn; *den = (int32_t)d;
    return P25FE_OK;
}

int p25fe_tuner_rotator(int32_t den, float* cs, size_t cap)
{
    if (den < 1 || den > P25FE_TUNE_MAX_DEN) return P25FE_ERR_ARG;
    if (cap < 2 * (size_t)den || !cs) return P25FE_ERR_CAPACITY;
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int32_t i = 0; i < den; ++i) {
        const double w = two_pi * (double)i / (double)den;          // (2 pi i) / den, in this order
        cs[i] = (float)cos(w); cs[den + i] = (float)sin(w);
    }
    return P25FE_OK;
}

int p25fe_tuner_create(p25fe_t* h, int32_t L, int32_t M, int32_t T, const float* taps, int32_t n_out_channels, const int32_t* num,
                       const int32_t* den, p25fe_tuner_t** out)
{
    if (out) *out = nullptr;
    if (!out || n_out_channels < 1 || n_out_channels > P25FE_TUNE_MAX_CH || !num || !den) return P25FE_ERR_ARG;
    for (int k = 0; k < n_out_channels; ++k) if (!tn_freq_ok(num[k], den[k])) return P25FE_ERR_ARG;
    p25fe_tuner* tn = nullptr;
    if (int rc = rs_create(&tn, h, L, M, T, taps, 1)) return rc;    // (the handle is looked at last)
    const int K = tn->K = n_out_channels;
    // one rotator per distinct denominator, (cos, sin) interleaved, one after the other in one buffer
    std::vector<long> at_den(P25FE_TUNE_MAX_DEN + 1, -1), at((size_t)K);
    std::vector<float> rot, cs;
    std::vector<TuneCh> ch((size_t)K);
    int lds_den = 0;
    for (int k = 0; k < K; ++k) {
        const int D = den[k];
        if (num[k] != 0 && D <= TN_ROT_LDS_DEN && D > lds_den) lds_den = D;
        if (at_den[D] < 0) {
            at_den[D] = (long)(rot.size() / 2);
            cs.resize(2 * (size_t)D);
            (void)p25fe_tuner_rotator(D, cs.data(), cs.size());
            for (int i = 0; i < D; ++i) { rot.push_back(cs[i]); rot.push_back(cs[D + i]); }
        }
        at[(size_t)k] = at_den[D];
        ch[(size_t)k].D = D;
        ch[(size_t)k].nm = (int)(((int64_t)num[k] % D + D) % D);
    }
    return tn_finish(tn, rot, ch, at, lds_den, out);
}

int p25fe_nco_step(uint32_t fs_in_hz, double offset_hz, int32_t* step)
{
    if (!step || fs_in_hz == 0 || !(offset_hz - offset_hz == 0.0) || 2.0 * fabs(offset_hz) > (double)fs_in_hz) return P25FE_ERR_ARG;
    // |offset / fs| <= 1/2, so the product is within [-2^31, 2^31] and exact as a power-of-two scaling; ties go to even
    const double q = nearbyint(ldexp(offset_hz / (double)fs_in_hz, 32));
    *step = (int32_t)(uint32_t)(int64_t)q;                          // +2^31 wraps to -2^31: both are the Nyquist frequency
    return P25FE_OK;
}

// (c, s) of a 32-bit phase: SPEC 3.0d from `ph` on
static void nco_factor_host(uint32_t ph, float cs[2])
{
    static const std::vector<float> rot = [] {
        std::vector<float> r(2 * (size_t)TN_NCO_DEN);
        (void)p25fe_tuner_rotator(TN_NCO_DEN, r.data(), r.size());
        return r;
    }();
    // SPEC 3.0d, the operations the kernel's nco_factor does, in its order (this file is compiled without contraction)
    const uint32_t ia = (ph + (1u << 23)) >> 24;
    const int32_t r = (int32_t)(ph - (ia << 24));
    const float t = (float)r * (float)(6.283185307179586476925 / 4294967296.0);
    const float t2 = t * t;
    const float cf = fmaf(t2, -0.5f, 1.0f);
    const float sf = fmaf(t2 * t, (float)(-1.0 / 6.0), t);
    const float C = rot[ia], S = rot[TN_NCO_DEN + ia];
    cs[0] = fmaf(-S, sf, C * cf);
    cs[1] = fmaf(C, sf, S * cf);
}

int p25fe_nco_factor(int32_t step, uint64_t n, float cs[2])
{
    if (!cs) return P25FE_ERR_ARG;
    nco_factor_host((uint32_t)step * (uint32_t)n, cs);
    return P25FE_OK;
}

int p25fe_nco_create(p25fe_t* h, int32_t L, int32_t M, int32_t T, const float* taps, int32_t n_out_channels, const int32_t* step,
                           p25fe_tuner_t** out)
{
    if (out) *out = nullptr;
    if (!out || n_out_channels < 1 || n_out_channels > P25FE_TUNE_MAX_CH || !step) return P25FE_ERR_ARG;
    p25fe_tuner* tn = nullptr;
    if (int rc = rs_create(&tn, h, L, M, T, taps, 1)) return rc;    // (the handle is looked at last)
    const int K = tn->K = n_out_channels;
    tn->mix = MIX_NCO;
    tn->step.assign(step, step + K);
    tn->ph0.assign((size_t)K, 0u);
    std::vector<float> cs(2 * (size_t)TN_NCO_DEN), rot;
    (void)p25fe_tuner_rotator(TN_NCO_DEN, cs.data(), cs.size());
    for (int i = 0; i < TN_NCO_DEN; ++i) { rot.push_back(cs[i]); rot.push_back(cs[TN_NCO_DEN + i]); }
    std::vector<TuneCh> ch((size_t)K);
    for (int k = 0; k < K; ++k) { ch[(size_t)k].ph0 = 0u; ch[(size_t)k].step = step[k]; }
    return tn_finish(tn, rot, ch, std::vector<long>((size_t)K, 0), TN_NCO_DEN, out);   // every channel has the one table
}

void p25fe_tuner_destroy(p25fe_tuner_t* tn) { rs_destroy(tn); }

int p25fe_tuner_reset(p25fe_tuner_t* tn) { return rs_reset(tn); }

int p25fe_tune_dev(p25fe_tuner_t* tn, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, float* d_out,
                   size_t out_stride, void* stream)
{
    if (!tn || !tn->h || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    return rs_launch(tn, tn, d_iq, fmt, 0, n_hist, n, abs_first, d_out, out_stride, (hipStream_t)stream);
}

int p25fe_tune(p25fe_tuner_t* tn, const void* iq, int fmt, size_t n, float* out, size_t cap, size_t* n_out)
{
    return rs_stream(tn, tn, iq, fmt, n, out, cap, n_out);
}

// --------------------------------------------------------------------------------------------
// AFC (SPEC 3.0e, 3.0f): a channel's step changed in a stream, and the frequency measure
// --------------------------------------------------------------------------------------------
int p25fe_afc_factor(int32_t step, uint32_t ph0, uint64_t n, float cs[2])
{
    if (!cs) return P25FE_ERR_ARG;
    nco_factor_host(ph0 + (uint32_t)step * (uint32_t)n, cs);
    return P25FE_OK;
}

int p25fe_afc_set_step(p25fe_tuner_t* tn, int32_t k, int32_t step, uint64_t abs_at, void* stream)
{
    if (!tn || !tn->h || tn->mix != MIX_NCO || k < 0 || k >= tn->K || position_refused(abs_at)) return P25FE_ERR_ARG;
    if (tn->stale) return P25FE_ERR_ARG;                            // the device has newer numbers than the host (p25fe_track_read)
    p25fe_t* h = tn->h;
    // the phase at abs_at stays: ph0 + step_old abs_at = ph0' + step abs_at (mod 2^32)
    const uint32_t ph0 = tn->ph0[(size_t)k] + ((uint32_t)tn->step[(size_t)k] - (uint32_t)step) * (uint32_t)abs_at;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    (void)hipGetLastError();
    // A null stream is the handle's (p25fe_tune's).  p25fe_tune_dev with a null stream enqueues on the default stream, which the
    // handle's non-blocking stream is not ordered against: the update waits for what the default stream holds, and the default
    // stream's later work waits for the update.
    const hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if (!stream) {
        if (!tn->ev) HIPCHK(h, hipEventCreateWithFlags(&tn->ev, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(tn->ev, nullptr));
        HIPCHK(h, hipStreamWaitEvent(st, tn->ev, 0));
    }
    // by value through a one-thread kernel: ordered on the stream behind every launch issued before it, no host buffer to keep alive
    hipLaunchKernelGGL(k_afc_set_ch, dim3(1), dim3(1), 0, st, tn->d_ch.as<TuneCh>() + k, (int)step, (unsigned)ph0);
    HIPCHK(h, hipGetLastError());
    if (!stream) {
        HIPCHK(h, hipEventRecord(tn->ev, st));
        HIPCHK(h, hipStreamWaitEvent(nullptr, tn->ev, 0));
    }
    tn->step[(size_t)k] = step; tn->ph0[(size_t)k] = ph0;
    return P25FE_OK;
}

int p25fe_afc_get_step(const p25fe_tuner_t* tn, int32_t k, int32_t* step, uint32_t* ph0)
{
    if (!tn || tn->mix != MIX_NCO || k < 0 || k >= tn->K || !step || !ph0 || tn->stale) return P25FE_ERR_ARG;
    *step = tn->step[(size_t)k]; *ph0 = tn->ph0[(size_t)k];
    return P25FE_OK;
}

int p25fe_afc_design(int32_t D, double cutoff_hz, int32_t T, float* taps, size_t cap)
{
    if (!afc_shape_ok(D, T) || !(cutoff_hz - cutoff_hz == 0.0) || !(cutoff_hz > 0.0) || cutoff_hz > 120000.0) return P25FE_ERR_ARG;
    const size_t N = (size_t)T;
    if (cap < N || !taps) return P25FE_ERR_CAPACITY;
    // p25fe_resampler_design's rule with L = 1 at 240 ksps and the caller's cutoff (the prototype's gain cancels in the scaling to sum 1)
    rs_kaiser_sinc(N, cutoff_hz / (double)P25FE_RS_RATE_OUT_HZ, 1.0, 1.0, taps);
    return P25FE_OK;
}

int p25fe_afc_create(p25fe_t* h, int32_t D, int32_t T, const float* taps, int32_t K, p25fe_afc_t** out)
{
    if (out) *out = nullptr;
    if (!out || !afc_shape_ok(D, T) || K < 1 || K > P25FE_AFC_MAX_CH || !taps) return P25FE_ERR_ARG;
    for (int k = 0; k < T; ++k) if (!finite_f(taps[k])) return P25FE_ERR_ARG;
    if (!h) return P25FE_ERR_ARG;                                   // (the handle is looked at last)
    p25fe_afc* o = new (std::nothrow) p25fe_afc;
    if (!o) return P25FE_ERR_NOMEM;
    o->h = h; o->device = h->cfg.device; o->D = D; o->T = T; o->K = K;
    if (hipSetDevice(h->cfg.device) != hipSuccess || o->d_taps.ensure((size_t)T * sizeof(float)) != hipSuccess ||
        hipMemcpy(o->d_taps.p, taps, (size_t)T * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        h->last_hip = (int)hipGetLastError(); delete o; return P25FE_ERR_HIP;
    }
    *out = o;
    return P25FE_OK;
}

void p25fe_afc_destroy(p25fe_afc_t* afc) { rs_destroy(afc); }

int p25fe_afc_measure_dev(p25fe_afc_t* afc, const float* d_rows, size_t row_stride, size_t n_hist, size_t n, uint64_t abs_first,
                          int32_t shift, p25fe_afc_acc_t* d_acc, void* stream)
{
    if (!afc || !afc->h || !d_rows || !d_acc || position_refused(abs_first) || n >= P25FE_MAX_POSITION ||
        row_stride >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    if (shift < 0 || shift > P25FE_AFC_MAX_SHIFT) return P25FE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 7u) != 0 || (reinterpret_cast<uintptr_t>(d_acc) & 7u) != 0) return P25FE_ERR_ARG;
    p25fe_t* h = afc->h;
    const int D = afc->D, T = afc->T;
    const size_t n_out = p25fe_n_resample(1, D, abs_first, n);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_out == 0) return P25FE_OK;
    AfcArgs a;
    a.x = reinterpret_cast<const float2*>(d_rows); a.row_stride = (long)row_stride;
    a.n_hist = (long)std::min(n_hist, (size_t)(T - 1 + D));        // nothing before that is ever read
    a.n_new = (long)n; a.n_out = (long)n_out;
    a.taps = afc->d_taps.as<float>(); a.D = D; a.T = T;
    a.d0 = D - 1 - (int)(abs_first % (uint64_t)D);                  // owned w 0 is the first m with n_m = m D + D - 1 >= abs_first
    a.tw = std::min(WV * RS_R, 1 + (RS_NIN - T) / D);
    a.scale = ldexpf(1.0f, shift);
    a.acc = d_acc;
    const size_t per = (size_t)a.tw - 1, tiles = (n_out + per - 1) / per;
    if (tiles > (size_t)0x7fffffffu) return P25FE_ERR_ARG;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_afc_measure, dim3((unsigned)tiles, (unsigned)afc->K), dim3(WV), 0, (hipStream_t)stream, a);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_afc_hz(const p25fe_afc_acc_t* acc, int32_t D, double* hz, double* coherence)
{
    if (!acc || !hz || !coherence || D < P25FE_AFC_MIN_D || D > P25FE_AFC_MAX_D) return P25FE_ERR_ARG;
    *hz = 0.0; *coherence = 0.0;
    if (acc->pow <= 0) return P25FE_OK;
    const double re = (double)acc->re, im = (double)acc->im;
    *hz = atan2(im, re) / (2.0 * 3.14159265358979323846) * (double)P25FE_RS_RATE_OUT_HZ / (double)D;
    *coherence = hypot(re, im) / (double)acc->pow;
    return P25FE_OK;
}

// --------------------------------------------------------------------------------------------
// AFC loop (SPEC 3.0g): the update of every channel on the device, and the sequencer tune -> measure -> update
// --------------------------------------------------------------------------------------------
static bool track_cfg_ok(const p25fe_track_cfg_t* c)
{
    return c && c->shift >= 0 && c->shift <= P25FE_AFC_MAX_SHIFT && c->coh_min_q15 >= 0 && c->coh_min_q15 <= 32768 &&
           c->gain_q16 >= 1 && c->gain_q16 <= 65536 && c->max_pull > 0 && c->max_dev > 0 && c->reserved == 0 && c->min_products >= 1;
}

int p25fe_track_create(p25fe_tuner_t* tn, p25fe_afc_t* afc, const p25fe_track_cfg_t* cfg, p25fe_track_t** out)
{
    if (out) *out = nullptr;
    if (!out || !tn || !afc || !track_cfg_ok(cfg)) return P25FE_ERR_ARG;
    if (tn->mix != MIX_NCO || tn->stale || tn->K != afc->K || !tn->h || tn->h != afc->h) return P25FE_ERR_ARG;
    p25fe_t* h = tn->h;
    p25fe_track* o = new (std::nothrow) p25fe_track;
    if (!o) return P25FE_ERR_NOMEM;
    o->h = h; o->device = h->cfg.device; o->tn = tn; o->afc = afc; o->cfg = *cfg; o->K = tn->K;
    const size_t K = (size_t)o->K;
    std::vector<p25fe_track_state_t> st(K);
    for (size_t k = 0; k < K; ++k) { st[k] = p25fe_track_state_t{}; st[k].step = tn->step[k]; st[k].ph0 = tn->ph0[k]; }
    if (hipSetDevice(h->cfg.device) != hipSuccess || o->d_acc.ensure(K * sizeof(p25fe_afc_acc_t)) != hipSuccess ||
        o->d_state.ensure(K * sizeof(p25fe_track_state_t)) != hipSuccess || o->d_ref.ensure(K * sizeof(int32_t)) != hipSuccess ||
        hipMemset(o->d_acc.p, 0, K * sizeof(p25fe_afc_acc_t)) != hipSuccess ||
        hipMemcpy(o->d_state.p, st.data(), K * sizeof(p25fe_track_state_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(o->d_ref.p, tn->step.data(), K * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        h->last_hip = (int)hipGetLastError(); delete o; return P25FE_ERR_HIP;
    }
    *out = o;
    return P25FE_OK;
}

void p25fe_track_destroy(p25fe_track_t* lp) { rs_destroy(lp); }

int p25fe_track_records(p25fe_track_t* lp, p25fe_afc_acc_t* get, const p25fe_afc_acc_t* set)
{
    if (!lp) return P25FE_ERR_ARG;
    p25fe_t* h = lp->h;
    const size_t bytes = (size_t)lp->K * sizeof(p25fe_afc_acc_t);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    if (get) HIPCHK(h, hipMemcpy(get, lp->d_acc.p, bytes, hipMemcpyDeviceToHost));
    if (set) HIPCHK(h, hipMemcpy(lp->d_acc.p, set, bytes, hipMemcpyHostToDevice));
    return P25FE_OK;
}

int p25fe_track_measure_dev(p25fe_track_t* lp, const float* d_rows, size_t row_stride, size_t n_hist, size_t n, uint64_t abs_first,
                            void* stream)
{
    if (!lp) return P25FE_ERR_ARG;
    return p25fe_afc_measure_dev(lp->afc, d_rows, row_stride, n_hist, n, abs_first, lp->cfg.shift, lp->d_acc.as<p25fe_afc_acc_t>(), stream);
}

int p25fe_track_update_dev(p25fe_track_t* lp, uint64_t abs_at, void* stream)
{
    if (!lp || position_refused(abs_at)) return P25FE_ERR_ARG;
    p25fe_t* h = lp->h;
    p25fe_tuner* tn = lp->tn;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    (void)hipGetLastError();
    // the ordering of p25fe_afc_set_step: a null stream is the handle's, ordered against the default stream on both sides
    const hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if (!stream) {
        if (!tn->ev) HIPCHK(h, hipEventCreateWithFlags(&tn->ev, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(tn->ev, nullptr));
        HIPCHK(h, hipStreamWaitEvent(st, tn->ev, 0));
    }
    AfcLoopArgs a;
    a.cfg = lp->cfg; a.L = tn->L; a.M = tn->M; a.D = lp->afc->D; a.K = lp->K;
    a.step_ref = lp->d_ref.as<int32_t>(); a.acc = lp->d_acc.as<p25fe_afc_acc_t>(); a.state = lp->d_state.as<p25fe_track_state_t>();
    a.ch = tn->d_ch.as<TuneCh>(); a.abs_at = (unsigned long)abs_at;
    tn->stale = true;                                               // from here on the device's numbers are the newer ones
    hipLaunchKernelGGL(k_afc_loop, dim3(1), dim3((unsigned)round_up((size_t)lp->K, (size_t)WV)), 0, st, a);
    HIPCHK(h, hipGetLastError());
    if (!stream) {
        HIPCHK(h, hipEventRecord(tn->ev, st));
        HIPCHK(h, hipStreamWaitEvent(nullptr, tn->ev, 0));
    }
    return P25FE_OK;
}

int p25fe_track_run_dev(p25fe_track_t* lp, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint64_t window,
                        float* d_out, size_t out_stride, size_t n_hist_out, void* stream)
{
    if (!lp || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    p25fe_tuner* tn = lp->tn;
    if (rs_pointers_refused(tn, d_iq, fmt, 0, abs_first, d_out) || n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    // every piece starts on an aligned 16-byte vector of the input, and a window holds at least the tuner's history
    const uint64_t unit = fmt_stride_unit(fmt);
    if (window >= P25FE_MAX_POSITION || window == 0 || window % unit != 0 || abs_first % unit != 0 || window + 1 < (uint64_t)tn->T)
        return P25FE_ERR_ARG;
    const uint64_t L = (uint64_t)tn->L, M = (uint64_t)tn->M;
    if (out_stride < p25fe_n_resample(tn->L, tn->M, abs_first, n)) return P25FE_ERR_ARG;
    const uint64_t end = abs_first + n, out_first = rs_floor(abs_first, L, M);
    const unsigned char* src = static_cast<const unsigned char*>(d_iq);
    for (uint64_t a = abs_first; a < end;) {
        const uint64_t b = std::min(end, (a / window + 1) * window);
        const size_t off = (size_t)(a - abs_first), len = (size_t)(b - a);
        const size_t out_off = (size_t)(rs_floor(a, L, M) - out_first), cnt = p25fe_n_resample(tn->L, tn->M, a, len);
        float* rows = d_out + 2 * out_off;
        if (int rc = rs_launch(tn, tn, src + off * fmt_bytes(fmt), fmt, 0, n_hist + off, len, a, rows, out_stride, (hipStream_t)stream)) return rc;
        if (int rc = p25fe_track_measure_dev(lp, rows, out_stride, n_hist_out + out_off, cnt, out_first + out_off, stream)) return rc;
        if (b % window == 0) if (int rc = p25fe_track_update_dev(lp, b, stream)) return rc;
        a = b;
    }
    return P25FE_OK;
}

int p25fe_track_read(p25fe_track_t* lp, p25fe_track_state_t* state_out)
{
    if (!lp) return P25FE_ERR_ARG;
    p25fe_t* h = lp->h;
    p25fe_tuner* tn = lp->tn;
    const size_t K = (size_t)lp->K;
    std::vector<p25fe_track_state_t> st(K);
    std::vector<TuneCh> ch(K);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());                              // whatever stream the updates went to
    HIPCHK(h, hipMemcpy(st.data(), lp->d_state.p, K * sizeof(p25fe_track_state_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(ch.data(), tn->d_ch.p, K * sizeof(TuneCh), hipMemcpyDeviceToHost));
    // the tuner's record is what runs: a p25fe_afc_set_step after the last update shows there and not in the state
    for (size_t k = 0; k < K; ++k) { st[k].step = tn->step[k] = ch[k].step; st[k].ph0 = tn->ph0[k] = ch[k].ph0; }
    tn->stale = false;
    if (state_out) memcpy(state_out, st.data(), K * sizeof(p25fe_track_state_t));
    return P25FE_OK;
}

int p25fe_track_step(const p25fe_track_cfg_t* cfg, int32_t L, int32_t M, int32_t D, int32_t step_ref, const p25fe_afc_acc_t* acc_in,
                     const p25fe_track_state_t* state_in, uint64_t abs_at, p25fe_afc_acc_t* acc_out, p25fe_track_state_t* state_out)
{
    if (!track_cfg_ok(cfg) || !rs_ratio_ok(L, M) || D < P25FE_AFC_MIN_D || D > P25FE_AFC_MAX_D || !acc_in || !state_in || !acc_out ||
        !state_out) return P25FE_ERR_ARG;
    p25fe_afc_acc_t acc = *acc_in;
    p25fe_track_state_t st = *state_in;
    afc_loop_law(*cfg, L, M, D, step_ref, abs_at, acc, st);
    *acc_out = acc; *state_out = st;
    return P25FE_OK;
}

int p25fe_track_hz(const p25fe_track_state_t* state, int32_t D, double* hz)
{
    if (!state || !hz || D < P25FE_AFC_MIN_D || D > P25FE_AFC_MAX_D) return P25FE_ERR_ARG;
    *hz = ldexp((double)state->last_theta, -32) * (double)P25FE_RS_RATE_OUT_HZ / (double)D;
    return P25FE_OK;
}

// --------------------------------------------------------------------------------------------
// device-resident ranges
// --------------------------------------------------------------------------------------------
int p25fe_demod_dev(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                    float* d_bb, size_t bb_stride, float* d_power_dbm, void* stream)
{
    if (!h || !d_iq || !d_bb || position_refused(abs0)) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    K1Launch k;
    k.src = d_iq; k.fmt = fmt; k.ch_stride = ch_stride; k.n_hist = n_hist; k.n = n; k.abs0 = abs0;
    k.bb = d_bb; k.bb_stride = bb_stride; k.power_dbm = d_power_dbm; k.stream = (hipStream_t)stream;
    return launch_k1(h, k);
}

size_t p25fe_n_predecim(uint64_t abs0, size_t n)
{
    const size_t o0 = (size_t)wide_o0(abs0);
    return n > o0 ? (n - o0 - 1) / PD + 1 : 0;
}

int p25fe_predecim_dev(p25fe_t* h, const float* d_iq, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                       float* d_out, size_t out_stride, void* stream)
{
    if (!h) return P25FE_ERR_ARG;
    return launch_k0(h, d_iq, P25FE_FMT_CF32, ch_stride, n_hist, n, abs0, d_out, out_stride, (hipStream_t)stream);
}

int p25fe_channelise_dev(p25fe_t* h, const float* d_iq, size_t n_hist, size_t n, uint64_t abs0, float* d_out,
                         size_t out_stride, void* stream)
{
    if (!h) return P25FE_ERR_ARG;
    return launch_k6(h, d_iq, P25FE_FMT_CF32, n_hist, n, abs0, d_out, out_stride, (hipStream_t)stream);
}

// Wideband input as the tuner delivers it (SPEC 3.0 / 3.11): the same stages on s16 or u8 pairs, or on cf32.
int p25fe_predecim_fmt_dev(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs_first,
                           float* d_out, size_t out_stride, void* stream)
{
    if (!h || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    return launch_k0(h, d_iq, fmt, ch_stride, n_hist, n, abs_first, d_out, out_stride, (hipStream_t)stream);
}

int p25fe_channelise_fmt_dev(p25fe_t* h, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, float* d_out,
                             size_t out_stride, void* stream)
{
    if (!h || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    return launch_k6(h, d_iq, fmt, n_hist, n, abs_first, d_out, out_stride, (hipStream_t)stream);
}

// Every entry point that uses the receiver's scratch first makes its stream wait for receive kernels that
// p25fe_run_dev_pipelined left running on the handle's own stream (no-op when nothing is pending).
static int pipe_join(p25fe_t* h, hipStream_t st)
{
    // The events stay pending until the lane is reused: a later call on ANOTHER stream must wait too (the receive
    // kernels may still be running and share the scratch with whatever that call launches).
    for (Lane& l : h->lanes)
        if (l.pending && !(l.joined_any && l.joined == st)) {
            HIPCHK(h, hipStreamWaitEvent(st, l.ev_rx, 0));
            l.joined = st; l.joined_any = true;
        }
    return P25FE_OK;
}

int p25fe_slice_dev(p25fe_t* h, const float* d_bb, size_t bb_stride, size_t n_hist_bb, size_t n_bb, uint64_t abs_bb0,
                    const p25fe_anchor_t* d_anchor_in, uint8_t* d_dibits, size_t dibit_stride, int64_t* d_sync_pos,
                    uint64_t* d_sync_dibit, size_t sync_stride, p25fe_result_t* d_result, void* stream)
{
    if (!h || !d_bb || !d_dibits || !d_result || position_refused(abs_bb0)) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_bb > MAX_RANGE_BB) return P25FE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    h->sh.invalidate();
    if (int jrc = pipe_join(h, st)) return jrc;
    int rc = ensure_slice_scratch(h, n_bb ? n_bb : 1);
    if (rc) return rc;
    RecvCall rcall = recv_call(h);
    rcall.reslice = h->track == P25FE_CLOCK_TRACKING_RESLICE;      // the whole range is in memory: SPEC 3.8c applies
    h->rs_n = 0;                                         // the lock drops belong to this call
    rcall.range.n_bb = n_bb; rcall.range.anchor_in = d_anchor_in;
    rcall.range.abs_bb0 = (long)abs_bb0 - h->look;       // first processed index: the tracking clock runs h->look samples late
    rcall.dest.dibits = d_dibits; rcall.dest.dibit_stride = dibit_stride; rcall.dest.result = d_result;
    rcall.dest.sync_pos = d_sync_pos; rcall.dest.sync_dibit = d_sync_dibit; rcall.dest.sync_stride = sync_stride;
    rcall.stream = st;
    // stages 6-7 on a LINEAR device baseband: planarize, detect, scan, slice (an empty range: only the scan runs and hands the anchor through)
    if (n_bb)
        if ((rc = launch_planarize(h, d_bb, bb_stride, n_hist_bb, n_bb, st)) != P25FE_OK) return rc;
    return launch_recv(h, rcall);
}

int p25fe_join_dev(p25fe_t* h, void* stream)
{
    if (!h) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return pipe_join(h, (hipStream_t)stream);
}

int p25fe_debug_planes_size(const p25fe_t* h, size_t n_bb, size_t* n_floats, size_t* n_words)
{
    if (!h || !n_floats || !n_words || n_bb > MAX_RANGE_BB) return P25FE_ERR_ARG;
    const PlanarGeo g(n_bb);
    *n_floats = g.floats(); *n_words = g.words();
    return P25FE_OK;
}

// The planes stay where they are: a device-to-device copy per channel out of the set the last call sized (which a pipelined call has
// moved on to BEFORE it sized it; the set is remembered by id all the same, so that nothing here depends on when `cur` moves).
int p25fe_debug_planes_dev(p25fe_t* h, size_t n_bb, float* d_f, size_t f_stride, uint32_t* d_bits, size_t bits_stride, void* stream)
{
    if (!h || !d_f || !d_bits || n_bb > MAX_RANGE_BB || h->pl_lane < 0) return P25FE_ERR_ARG;
    const PlanarGeo g(n_bb);
    const size_t C = (size_t)h->C;
    const RxScratch& s = h->lanes[h->pl_lane].s;
    if (g.n_blocks != h->pl_blocks || f_stride < g.floats() || bits_stride < g.words()) return P25FE_ERR_ARG;
    if (!s.pl_f.get() || !s.pl_bits.get() || s.pl_f.buf.cap < C * g.floats() * sizeof(float) || s.pl_bits.buf.cap < C * g.words() * sizeof(uint32_t))
        return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    for (size_t c = 0; c < C; ++c) {
        HIPCHK(h, hipMemcpyAsync(d_f + c * f_stride, s.pl_f.get() + c * g.floats(), g.floats() * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(d_bits + c * bits_stride, s.pl_bits.get() + c * g.words(), g.words() * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
    return P25FE_OK;
}

static int ensure_rx_stream(p25fe_t* h)
{
    if (!h->rx_stream) {
        if (h->rx_cus > 0) {
            // The receive kernels are a few thousand short one-wave workgroups and one single-workgroup scan.  Left free they
            // take wave slots, LDS and memory-pipe time from K1 on EVERY CU (K1 measured 12 % slower under overlap in round
            // 2's driver run); confined to a few CUs they cost K1 at most that share of the chip while they run.
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int ncu = h->n_cu < 256 ? h->n_cu : 256;
            const int want = h->rx_cus < ncu ? h->rx_cus : ncu;
            // spread over the XCDs: CU c of the mask numbering sits on XCD c % 8 (workgroups are handed out the same way)
            for (int k = 0; k < want; ++k) mask[k / 32] |= 1u << (k % 32);
            if (hipExtStreamCreateWithCUMask(&h->rx_stream, (uint32_t)((ncu + 31) / 32), mask) != hipSuccess) {
                (void)hipGetLastError();
                h->rx_stream = nullptr;
            }
        }
        if (!h->rx_stream) {
            int prio_lo = 0, prio_hi = 0;
            // (highest priority; normal and lowest were measured in round 6 and change nothing: 0.2647 - 0.2656 / 0.2647 - 0.2650 / 0.2651 -
            // 0.2709 ms per step, docs/MEASUREMENTS.md)
            if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
                hipStreamCreateWithPriority(&h->rx_stream, hipStreamNonBlocking, prio_hi) != hipSuccess) {
                (void)hipGetLastError();
                h->rx_stream = nullptr;
                HIPCHK(h, hipStreamCreateWithFlags(&h->rx_stream, hipStreamNonBlocking));     // any non-blocking stream will do
            }
        }
    }
    return P25FE_OK;
}
// The preamble of a pipelined call: the receive stream and the lanes' events exist, the NEXT scratch set becomes the current one, and
// `st` (where K1 is about to overwrite that set's planes) waits for the receive kernels that last read it, `depth` calls back.
static int pipe_open(p25fe_t* h, hipStream_t st, int depth = 2)
{
    if (int rc = ensure_rx_stream(h)) return rc;
    for (Lane& l : h->lanes) {                                       // (per event: a failed creation is retried by the next call)
        if (!l.ev_k1) HIPCHK(h, hipEventCreateWithFlags(&l.ev_k1, hipEventDisableTiming));
        if (!l.ev_rx) HIPCHK(h, hipEventCreateWithFlags(&l.ev_rx, hipEventDisableTiming));
    }
    rotate_lanes(&h->cur, h->lane_q, depth);
    Lane& l = h->lane();
    if (l.pending) {
        const bool nowait = P25FE_M_PIPE_NOWAIT();                   // (false in the product: measurement hook, p25fe_kernels.hip)
        if (!nowait && !(l.joined_any && l.joined == st)) HIPCHK(h, hipStreamWaitEvent(st, l.ev_rx, 0));
        l.pending = false;
    }
    l.joined_any = false;
    return P25FE_OK;
}

// A device-resident capture from the start of a stream: K1 straight into the polyphase layout (+ sign planes; the 240 history
// positions in front of the stream come out as the zeros of a fresh DemodTask), then the receive chain -- on the caller's stream,
// or (pipelined) on the handle's receive stream in the next scratch set, beside the caller's next K1.
static int run_dev(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n, const RecvDest& dest, hipStream_t st, bool pipelined)
{
    if (!h || !d_iq || !dest.dibits || !dest.result || p25fe_n_baseband_h(h, 0, n) > MAX_RANGE_BB) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->sh.invalidate();
    if (int orc = pipelined ? pipe_open(h, st, h->run_depth) : pipe_join(h, st)) return orc;
    Lane& lane = h->lane();
    const size_t n_bb = p25fe_n_baseband_h(h, 0, n);
    int rc = ensure_slice_scratch(h, n_bb ? n_bb : 1);   // (growing a buffer frees the old one: hipFree synchronises the device)
    if (rc) return rc;
    RecvCall rcall = recv_call(h);
    rcall.reslice = h->track == P25FE_CLOCK_TRACKING_RESLICE;      // the whole range is in memory: SPEC 3.8c applies
    h->rs_n = 0;
    rcall.range.n_bb = n_bb; rcall.range.abs_bb0 = -h->look;
    rcall.dest = dest;
    rcall.stream = pipelined ? h->rx_stream : st;
    if (pipelined && h->ext_events) rcall.ev_done = lane.ev_rx;
    K1Launch k;
    k.src = d_iq; k.fmt = fmt; k.ch_stride = ch_stride; k.n = n; k.stream = st;
    if (n_bb) h->prof.begin();
    rc = launch_planar_recv(h, k, rcall, pipelined ? lane.ev_k1 : nullptr);
    h->prof.end();
    if (rc || !pipelined) return rc;
    if (!h->ext_events) HIPCHK(h, hipEventRecord(lane.ev_rx, h->rx_stream));
    lane.pending = true;
    return P25FE_OK;
}

int p25fe_run_dev_pipelined(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n, uint8_t* d_dibits,
                            size_t dibit_stride, p25fe_result_t* d_result, void* stream)
{
    RecvDest dest;
    dest.dibits = d_dibits; dest.dibit_stride = dibit_stride; dest.result = d_result;
    return run_dev(h, d_iq, fmt, ch_stride, n, dest, (hipStream_t)stream, /*pipelined=*/true);
}

int p25fe_run_dev(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n, uint8_t* d_dibits,
                  size_t dibit_stride, p25fe_result_t* d_result, void* stream)
{
    RecvDest dest;
    dest.dibits = d_dibits; dest.dibit_stride = dibit_stride; dest.result = d_result;
    return run_dev(h, d_iq, fmt, ch_stride, n, dest, (hipStream_t)stream, /*pipelined=*/false);
}

// --------------------------------------------------------------------------------------------
// time shards
// --------------------------------------------------------------------------------------------
// what: bit 0 = the main K1 launch, bit 1 = the head segment(s), bit 2 = sync detection + scan
enum { SH_MAIN = 1, SH_HEAD = 2, SH_RECV = 4 };
static int shard_pass1_part(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                            p25fe_result_t* d_result, hipStream_t st, int what)
{
    const bool do_main = (what & SH_MAIN) != 0, do_finish = (what & SH_RECV) != 0;
    bool do_head = (what & SH_HEAD) != 0;
    if (!h || !d_iq || (do_finish && !d_result) || position_refused(abs0) || p25fe_n_baseband_h(h, abs0, n) > MAX_RANGE_BB || piecewise_refused(h)) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    if (do_main) h->sh.invalidate();
    if (n_hist < SHARD_HALO && n_hist != abs0) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->sh.pipe)
        if (int jrc = pipe_join(h, st)) return jrc;
    const size_t n_bb = p25fe_n_baseband_h(h, abs0, n);
    const long abs_bb0 = (long)p25fe_n_baseband_h(h, 0, (size_t)abs0) - h->look;      // first processed baseband index of this shard
    int rc = ensure_slice_scratch(h, n_bb ? n_bb : 1);
    if (rc) return rc;
    // the receiver's 240 history samples are recomputed from the IQ halo (zeros before the start of the stream)
    K1Launch k;
    k.src = d_iq; k.fmt = fmt; k.ch_stride = ch_stride; k.n_hist = n_hist; k.n = n; k.abs0 = abs0; k.planar = true; k.stream = st;
    if (do_main) {
        h->prof.begin();
        // K1's event pair rides on THIS launch: with the split form it times the main launch alone (the head segment
        // that follows the halo wait is one workgroup), so an RCCL wait between the two is not in K1's figure.
        // Pipelined step: everything behind this launch runs on the receive stream, which waits for it here
        // (K1 on a CU-masked stream of its own, to keep a few CUs free for the exchanges that run beside it, was tried: the
        // masked launch itself ran 30 - 60 % slower -- profiles/r05_shard_pipelined.txt)
        k.part = do_head ? K1_ALL : K1_MAIN;
        rc = launch_k1_planar(h, k, h->sh.pipe ? h->lane().ev_k1 : nullptr, h->rx_stream);
        if (rc) return rc;
        h->sh.main_out = true; h->sh.main_nbb = n_bb; h->sh.main_abs0 = abs0;
        h->sh.head_done = do_head;
        do_head = false;                                            // (K1_ALL = every segment)
    } else {
        if (!h->sh.main_is(n_bb, abs0)) return P25FE_ERR_ARG;       // head / finish without its main launch
    }
    if ((do_head || do_finish) && !h->sh.head_done) {
        // the segments whose input reaches into the halo.  They share no byte of the planes with the main launch's
        // (SEG_HALO in p25fe_kernels.hip), so this launch may run BESIDE it on another stream (p25fe_shard_pass1_head).
        long head_end = 0;                                          // planar positions [0, head_end) are the head's
        const bool own_stream = !do_finish;                         // launched on its own (another stream's)
        h->sh.head_flagged = false;
        if (n_bb) {
            if (own_stream) {
                // the launch's last workgroup publishes "the head is in memory"; the detection's first tiles wait for that
                // word instead of the whole stream waiting for an event
                if (!h->sh.flag.p) {
                    HIPCHK(h, h->sh.flag.ensure(SH_FLAG_WORDS * sizeof(unsigned)));
                    HIPCHK(h, hipMemsetAsync(h->sh.flag.p, 0, SH_FLAG_WORDS * sizeof(unsigned), st));
                }
                ++h->sh.seq;
                if (h->sh.seq == 0u) ++h->sh.seq;
            }
            k.part = K1_HEAD; k.ev0 = k.ev1 = nullptr; k.head_end = &head_end;
            k.done_flag = own_stream ? h->sh.flag.as<unsigned>() : nullptr; k.done_seq = h->sh.seq;
            rc = launch_k1(h, k);
            if (rc) return rc;
            if (own_stream && head_end > 0) {                       // (no head workgroup, no flag: nothing to wait for)
                h->sh.head_flagged = true;
                h->sh.head_tile_max = (int)(head_end / TS);         // a tile reads planes up to its own end (+ one sign word): tiles past the head's never touch it
            }
        }
        h->sh.head_done = true;
    }
    if (!do_finish) return P25FE_OK;
    h->prof.mark(1, st, h->ext_events);
    RecvCall rcall = recv_call(h);
    h->rs_n = 0;
    rcall.range.n_bb = n_bb; rcall.range.abs_bb0 = abs_bb0;
    rcall.dest.result = d_result;
    rcall.slice = false; rcall.wait_head = h->sh.head_flagged; rcall.stream = st;
    rc = launch_recv(h, rcall);
    h->sh.head_flagged = false;
    h->prof.end();
    if (rc) return rc;
    h->sh.finish_pass1(n_bb, abs_bb0, rcall.gen);
    return P25FE_OK;
}

int p25fe_shard_pass1(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                      p25fe_result_t* d_result, void* stream)
{
    return shard_pass1_part(h, d_iq, fmt, ch_stride, n_hist, n, abs0, d_result, (hipStream_t)stream, SH_MAIN | SH_HEAD | SH_RECV);
}

int p25fe_shard_pass1_main(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                           void* stream)
{
    return shard_pass1_part(h, d_iq, fmt, ch_stride, n_hist, n, abs0, nullptr, (hipStream_t)stream, SH_MAIN);
}

int p25fe_shard_pass1_head(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                           void* stream)
{
    return shard_pass1_part(h, d_iq, fmt, ch_stride, n_hist, n, abs0, nullptr, (hipStream_t)stream, SH_HEAD);
}

int p25fe_shard_pass1_k1(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0, void* stream)
{
    return shard_pass1_part(h, d_iq, fmt, ch_stride, n_hist, n, abs0, nullptr, (hipStream_t)stream, SH_MAIN | SH_HEAD);
}

int p25fe_shard_pass1_finish(p25fe_t* h, const void* d_iq, int fmt, size_t ch_stride, size_t n_hist, size_t n, uint64_t abs0,
                             p25fe_result_t* d_result, void* stream)
{
    return shard_pass1_part(h, d_iq, fmt, ch_stride, n_hist, n, abs0, d_result, (hipStream_t)stream, SH_RECV);
}

// The pipelined step of p25fe_rccl.cpp (p25fe_shard_step_pipelined): between _begin and _end the shard passes use the scratch set
// p25fe_run_dev_pipelined would use next; p25fe_shard_pass1_main stays on the caller's stream and makes the receive stream wait for
// it, every later pass is given the receive stream.  _end marks that stream's work as pending (p25fe_join_dev waits for it).
int p25fe_shard_pipe_begin(p25fe_t* h, void* stream, void** rx_stream)
{
    if (!h || !rx_stream || h->sh.pipe) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->sh.invalidate();
    if (int orc = pipe_open(h, (hipStream_t)stream, h->sh_depth)) return orc;
    h->sh.pipe = true;
    *rx_stream = h->rx_stream;
    return P25FE_OK;
}

int p25fe_rx_stream(p25fe_t* h, void** rx_stream)
{
    if (!h || !rx_stream) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = ensure_rx_stream(h)) return rc;
    *rx_stream = h->rx_stream;
    return P25FE_OK;
}

int p25fe_shard_pipe_end(p25fe_t* h, void* last_stream)
{
    if (!h || !h->sh.pipe) return P25FE_ERR_ARG;
    h->sh.pipe = false;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipEventRecord(h->lane().ev_rx, last_stream ? (hipStream_t)last_stream : h->rx_stream));
    h->lane().pending = true;
    return P25FE_OK;
}

// Pass 2 of a shard: K3 / K4 on what pass 1's K2 left in the scratch (the lock drops are in its summaries), no K2
static RecvCall shard_pass2_call(const p25fe_t* h, const p25fe_anchor_t* d_anchor_in, uint8_t* d_dibits, size_t dibit_stride, p25fe_result_t* d_result,
                                 hipStream_t st)
{
    RecvCall c = recv_call(h);
    c.gen = h->sh.gen;
    c.detect = false;
    c.range.n_bb = h->sh.nbb; c.range.abs_bb0 = h->sh.abs_bb0; c.range.anchor_in = d_anchor_in;
    c.dest.dibits = d_dibits; c.dest.dibit_stride = dibit_stride; c.dest.result = d_result;
    c.stream = st;
    return c;
}

int p25fe_shard_pass2(p25fe_t* h, const p25fe_anchor_t* d_anchor_in, uint8_t* d_dibits, size_t dibit_stride,
                      p25fe_result_t* d_result, void* stream)
{
    if (!h || !d_dibits || !d_result || !h->sh.valid) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    RecvCall rcall = shard_pass2_call(h, d_anchor_in, d_dibits, dibit_stride, d_result, (hipStream_t)stream);
    h->sh.scan_fresh = false;                            // the re-scan below rewrites the groups' carry-ins with THIS carry-in
    h->prof.begin();
    const int rc = launch_recv(h, rcall);
    h->prof.end();
    return rc;
}

int p25fe_shard_pass2_dev(p25fe_t* h, const p25fe_result_t* d_summaries, const uint64_t* d_shard_bb0, const uint64_t* d_shard_bb_n,
                          size_t n_shards, size_t rank, p25fe_anchor_t* d_anchor_in, uint64_t* d_dibit_offset, uint8_t* d_dibits,
                          size_t dibit_stride, uint8_t* d_dibits_dup, p25fe_result_t* d_result, void* stream)
{
    if (!h || !d_summaries || !d_shard_bb0 || !d_shard_bb_n || !d_anchor_in || !d_dibit_offset || !d_dibits || !d_result || !h->sh.valid ||
        n_shards == 0 || n_shards > 0x7fffffffu || rank >= n_shards || h->C != 1)
        return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    RecvCall rcall = shard_pass2_call(h, d_anchor_in + rank, d_dibits, dibit_stride, d_result, st);
    rcall.dest.dibits2 = d_dibits_dup;
    ShardFix fx;
    if (rcall.gen || !h->sh.scan_fresh || h->sh.nbb == 0) {
        // tracking clock / lock drops inside the shard (or a p25fe_shard_pass2 has already rewritten pass 1's scan; or a shard without a
        // baseband sample, which has no slicer tile to run the combine in: never the hot path): the combine as its own (one-thread)
        // launch, then the re-scan of the shard's groups + slicer with that carry-in
        h->sh.scan_fresh = false;
        hipLaunchKernelGGL(k_shard_resolve, dim3(1), dim3(64), 0, st, d_summaries, d_shard_bb0, d_shard_bb_n, (int)n_shards, h->track,
                           d_anchor_in, d_dibit_offset);
        HIPCHK(h, hipGetLastError());
    } else {
        fx.summ = d_summaries; fx.bb0 = d_shard_bb0; fx.bbn = d_shard_bb_n; fx.n_shards = (int)n_shards; fx.rank = (int)rank;
        fx.anc_out = d_anchor_in; fx.off_out = d_dibit_offset; fx.result = d_result;
        rcall.range.anchor_in = nullptr; rcall.fix = &fx;
    }
    h->prof.begin();
    const int rc = launch_recv(h, rcall);
    h->prof.end();
    return rc;
}

int p25fe_shard_resolve(const p25fe_result_t* summaries, const uint64_t* shard_bb0, const uint64_t* shard_bb_n,
                        size_t n_shards, int symbol_clock, p25fe_anchor_t* anchor_in, uint64_t* dibit_offset)
{
    if (!summaries || !shard_bb0 || !shard_bb_n || !anchor_in || !dibit_offset || n_shards > 0x7fffffffu) return P25FE_ERR_ARG;
    for (size_t r = 0; r < n_shards; ++r)
        if (position_refused(shard_bb0[r]) || position_refused(shard_bb_n[r]) || position_refused(shard_bb0[r] + shard_bb_n[r])) return P25FE_ERR_ARG;
    shard_resolve_impl(summaries, shard_bb0, shard_bb_n, (int)n_shards, symbol_clock, anchor_in, dibit_offset);
    return P25FE_OK;
}

int p25fe_shard_resolve_dev(p25fe_t* h, const p25fe_result_t* d_summaries, const uint64_t* d_shard_bb0,
                            const uint64_t* d_shard_bb_n, size_t n_shards, p25fe_anchor_t* d_anchor_in,
                            uint64_t* d_dibit_offset, void* stream)
{
    if (!h || !d_summaries || !d_shard_bb0 || !d_shard_bb_n || !d_anchor_in || !d_dibit_offset || n_shards > 0x7fffffffu) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_shard_resolve, dim3(1), dim3(64), 0, (hipStream_t)stream, d_summaries, d_shard_bb0, d_shard_bb_n,
                       (int)n_shards, h->track, d_anchor_in, d_dibit_offset);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_shard_head_check(p25fe_t* h)
{
    if (!h) return P25FE_ERR_ARG;
    if (!h->sh.flag.p) return P25FE_OK;                              // no head segment has ever run on a stream of its own
    HIPCHK(h, hipSetDevice(h->cfg.device));
    unsigned err = 0u;
    HIPCHK(h, hipMemcpy(&err, h->sh.flag.as<unsigned>() + SH_FLAG_ERR, sizeof err, hipMemcpyDeviceToHost));
    return err ? P25FE_ERR_TIMEOUT : P25FE_OK;
}

int p25fe_streams_share_queue(p25fe_t* h, void* stream_a, void* stream_b, int* shared)
{
    if (!h || !shared) return P25FE_ERR_ARG;
    *shared = 0;
    if (stream_a == stream_b) { *shared = 1; return P25FE_OK; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->sh.flag.p) {
        HIPCHK(h, h->sh.flag.ensure(SH_FLAG_WORDS * sizeof(unsigned)));
        HIPCHK(h, hipMemset(h->sh.flag.p, 0, SH_FLAG_WORDS * sizeof(unsigned)));
    }
    unsigned* w = h->sh.flag.as<unsigned>() + 2;                     // (words 0 / 1 are the head segment's flag and ticket)
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream_a));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream_b));
    int votes = 0;
    for (int rep = 0; rep < 3; ++rep) {                              // (three rounds: a busy chip can delay the setter once)
        HIPCHK(h, hipMemset(w, 0, 2 * sizeof(unsigned)));
        hipLaunchKernelGGL(k_queue_probe_wait, dim3(1), dim3(1), 0, (hipStream_t)stream_a, w, 20000ull);      // 200 us at 100 MHz
        hipLaunchKernelGGL(k_queue_probe_set, dim3(1), dim3(1), 0, (hipStream_t)stream_b, w);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize((hipStream_t)stream_a));
        HIPCHK(h, hipStreamSynchronize((hipStream_t)stream_b));
        unsigned r[2] = {0u, 0u};
        HIPCHK(h, hipMemcpy(r, w, sizeof r, hipMemcpyDeviceToHost));
        if (r[1] == 2u) ++votes;
    }
    *shared = votes == 3;
    return P25FE_OK;
}

int p25fe_shard_compact_dev(p25fe_t* h, const uint8_t* d_gathered, size_t cap, const uint64_t* d_dibit_offset,
                            size_t n_shards, uint8_t* d_out, size_t out_cap, void* stream)
{
    if (!h || !d_gathered || !d_dibit_offset || !d_out || n_shards == 0 || n_shards > 65535) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const unsigned bx = (unsigned)((cap + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(k_shard_compact, dim3(bx ? bx : 1, (unsigned)n_shards), dim3(256), 0, (hipStream_t)stream, d_gathered,
                       (unsigned long long)cap, d_dibit_offset, 0, (int)n_shards, d_out, (unsigned long long)out_cap);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_shard_compact_from_dev(p25fe_t* h, const uint8_t* d_gathered, size_t cap, const uint64_t* d_dibit_offset, size_t first_shard,
                                 size_t n_shards, uint8_t* d_out, size_t out_cap, void* stream)
{
    if (!h || !d_gathered || !d_dibit_offset || !d_out || n_shards == 0 || n_shards > 65535 || first_shard > n_shards) return P25FE_ERR_ARG;
    if (first_shard == n_shards) return P25FE_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const unsigned bx = (unsigned)((cap + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(k_shard_compact, dim3(bx ? bx : 1, (unsigned)(n_shards - first_shard)), dim3(256), 0, (hipStream_t)stream, d_gathered,
                       (unsigned long long)cap, d_dibit_offset, (int)first_shard, (int)n_shards, d_out, (unsigned long long)out_cap);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// --------------------------------------------------------------------------------------------
// streaming with host buffers: the bodies of DemodTask::run / RecvTask::run, one chunk per call
//
// All stream state (IQ history, baseband tail, anchors, counters) lives in HOST memory; input is staged in pinned,
// device-visible memory as [history | new samples] and read by the kernels over PCIe (zero copy: a 32 768-byte chunk is
// one latency, not a DMA command); results are written by the kernels straight into pinned memory.  A call is
// launches + ONE synchronisation, and for a chunk of at most one tile (the reference's 16 384-sample buffer gives
// 3 276 / 3 277 baseband samples) ONE launch: k_chunk / k_recv_chunk.
// --------------------------------------------------------------------------------------------
// [history | new] per channel in h->hin: the host view of the new samples (rows row_bytes apart), K1 on them from the stream's position on
struct Staged { char* fresh; size_t row_bytes; K1Launch k1; };
static int stage_iq(p25fe_t* h, const void* iq, int fmt, size_t n, Staged* s)
{
    if (h->state.format_refused(fmt)) return P25FE_ERR_FORMAT;
    const size_t C = (size_t)h->C, eb = fmt_bytes(fmt);
    const size_t stride = SHARD_HALO + round_up(n, 8) + 8;           // samples, multiple of 8: owned sample 0 stays 16-B aligned
    HIPCHK(h, h->hin.ensure(C * stride * eb));
    s->fresh = static_cast<char*>(h->hin.p) + SHARD_HALO * eb; s->row_bytes = stride * eb;
    h->state.stage_hist(fmt, static_cast<char*>(h->hin.p), s->row_bytes);
    for (size_t c = 0; c < C && n; ++c) memcpy(s->fresh + c * s->row_bytes, static_cast<const char*>(iq) + c * n * eb, n * eb);
    K1Launch& k = s->k1;
    k.src = static_cast<const char*>(h->hin.dp) + SHARD_HALO * eb; k.fmt = fmt; k.ch_stride = stride; k.n_hist = h->state.n_hist(); k.n = n;
    k.abs0 = h->state.abs_iq; k.stream = h->stream;
    return P25FE_OK;
}

static int demod_host(p25fe_t* h, const void* iq, int fmt, size_t n, float* bb, size_t bb_cap, size_t* n_out,
                      float* power_dbm)
{
    if (!h || (!iq && n) || !bb || !n_out) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nb = p25fe_n_baseband_h(h, h->state.abs_iq, n);
    if (nb > bb_cap) return P25FE_ERR_CAPACITY;
    const size_t C = (size_t)h->C;
    Staged sg;
    if (int rc = stage_iq(h, iq, fmt, n, &sg)) return rc;
    const size_t bb_stride = round_up(nb + 4, 4);
    HIPCHK(h, h->hout.ensure(C * bb_stride * sizeof(float) + 64 * (C + 2)));
    Arena ar(h->hout);
    float *d_bb, *d_pw;
    float* h_bb = ar.take<float>(C * bb_stride, &d_bb);
    float* h_pw = ar.take<float>(C, &d_pw);
    K1Launch k = sg.k1;
    k.bb = d_bb; k.bb_stride = bb_stride; k.power_dbm = power_dbm ? d_pw : nullptr;
    if (int rc = launch_k1(h, k)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t c = 0; c < C; ++c) memcpy(bb + c * bb_cap, h_bb + c * bb_stride, nb * sizeof(float));
    if (power_dbm) memcpy(power_dbm, h_pw, sizeof(float) * C);
    h->state.commit_iq(C, fmt, n, sg.fresh, sg.row_bytes);           // the call succeeded: the stream moves on behind the staged samples
    *n_out = nb;
    return P25FE_OK;
}

int p25fe_demod_u8(p25fe_t* h, const uint8_t* iq, size_t n_bytes, float* bb, size_t bb_cap, size_t* n_out,
                   float* power_dbm)
{
    if (n_bytes & 1) return P25FE_ERR_ARG;
    return demod_host(h, iq, P25FE_FMT_U8, n_bytes / 2, bb, bb_cap, n_out, power_dbm);
}

int p25fe_demod_cf32(p25fe_t* h, const float* iq, size_t n_samples, float* bb, size_t bb_cap, size_t* n_out,
                     float* power_dbm)
{
    return demod_host(h, iq, P25FE_FMT_CF32, n_samples, bb, bb_cap, n_out, power_dbm);
}

int p25fe_demod_s16(p25fe_t* h, const int16_t* iq, size_t n_samples, float* bb, size_t bb_cap, size_t* n_out,
                    float* power_dbm)
{
    return demod_host(h, iq, P25FE_FMT_S16, n_samples, bb, bb_cap, n_out, power_dbm);
}

// hard ceiling of the dibits of n_bb baseband samples, as a row size: detections, hence re-anchors, are at least W + 1 samples apart
static inline size_t dibit_row(size_t n_bb, size_t align) { return round_up(n_bb / (W + 1) + 2, align); }
// Pinned outputs of one receiver call: per channel a result record, the carry-in anchor, a dibit row and (optionally) the
// sync event rows; plus the baseband tail the fused path hands back.
struct RecvOut {
    p25fe_result_t *res, *d_res;
    p25fe_anchor_t *anc, *d_anc;
    uint8_t *dib, *d_dib;
    int64_t *spos, *d_spos;
    uint64_t *sdib, *d_sdib;
    float *tail, *d_tail;
    unsigned *done, *d_done;             // completion words the chunk kernels write last (polled by the host)
    size_t dstride, sstride;
};
static int recv_out(p25fe_t* h, size_t n_bb, size_t sync_cap, RecvOut* o)
{
    const size_t C = (size_t)h->C;
    o->dstride = dibit_row(n_bb, 16); o->sstride = sync_cap;
    const size_t bytes = C * (sizeof(p25fe_result_t) + sizeof(p25fe_anchor_t) + o->dstride + 16 * sync_cap + TAILN * sizeof(float) + 4) + 64 * 8;
    HIPCHK(h, h->hout.ensure(bytes));
    Arena ar(h->hout);
    o->res = ar.take<p25fe_result_t>(C, &o->d_res);
    o->anc = ar.take<p25fe_anchor_t>(C, &o->d_anc);
    o->dib = ar.take<uint8_t>(C * o->dstride, &o->d_dib);
    o->spos = ar.take<int64_t>(C * sync_cap, &o->d_spos);
    o->sdib = ar.take<uint64_t>(C * sync_cap, &o->d_sdib);
    o->tail = ar.take<float>(C * TAILN, &o->d_tail);
    o->done = ar.take<unsigned>(C, &o->d_done);
    memcpy(o->anc, h->state.anchor.data(), sizeof(p25fe_anchor_t) * C);
    return ensure_slice_scratch(h, n_bb);                           // ... and the scratch set the call's kernels work in
}
// the receive side of a host-buffer call: n_bb samples behind the stream's position, the pinned outputs
static RecvCall host_recv_call(const p25fe_t* h, const RecvOut& o, size_t n_bb, bool want_sync)
{
    RecvCall c = recv_call(h);                                      // (a pending p25fe_resync_at_dev list belongs to this call: cleared once it has succeeded)
    c.range.n_bb = n_bb; c.range.abs_bb0 = (long)h->state.abs_bb - h->look; c.range.anchor_in = o.d_anc;
    c.dest.dibits = o.d_dib; c.dest.dibit_stride = o.dstride; c.dest.result = o.d_res;
    c.dest.sync_pos = want_sync ? o.d_spos : nullptr; c.dest.sync_dibit = want_sync ? o.d_sdib : nullptr; c.dest.sync_stride = o.sstride;
    c.stream = h->stream;
    return c;
}
// ... and the same for the one-tile receiver of the chunk kernels
static void chunk_recv_args(const p25fe_t* h, const RecvCall& rc, float* d_tail, ChunkRecvArgs* c)
{
    view_planes(h, rc.range, c); view_tiles(h, c); view_dest(rc.range, rc.dest, c);
    c->result = rc.dest.result; c->n_baseband = rc.range.n_bb;
    c->tail = d_tail; c->look = (int)h->look;
    c->done = nullptr; c->seq = 0u;
}

// One-launch chunk calls finish by POLLING a word the kernel writes last into pinned memory (a system-scope release in front
// of it) instead of hipStreamSynchronize: the completion signal -> interrupt -> wake-up path costs more than the kernel.
// P25FE_CHUNK_POLL=0 keeps the synchronisation.  The stream is synchronised anyway if the word does not arrive in time.
static void chunk_poll_arm(p25fe_t* h, const RecvOut& o, ChunkRecvArgs* c)
{
    static const bool poll = [] { const char* e = getenv("P25FE_CHUNK_POLL"); return !(e && atoi(e) == 0); }();
    if (!poll) return;
    ++h->chunk_seq;
    if (h->chunk_seq == 0u) ++h->chunk_seq;
    for (int ch = 0; ch < h->C; ++ch) o.done[ch] = 0u;
    c->done = o.d_done; c->seq = h->chunk_seq;
}
static int chunk_wait(p25fe_t* h, const RecvOut& o, const ChunkRecvArgs& c)
{
    if (c.done) {
        volatile unsigned* w = o.done;
        const size_t C = (size_t)h->C;
        for (long spin = 0; spin < 4000000L; ++spin) {               // ~ tens of milliseconds at worst, then fall back
            size_t k = 0;
            while (k < C && w[k] == c.seq) ++k;
            if (k == C) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return P25FE_OK; }
            __builtin_ia32_pause();
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return P25FE_OK;
}
// the end of a call whose kernels are out (`polled`: the arguments they got): wait, capacity check, copy-out, receiver state
static int recv_finish(p25fe_t* h, const RecvOut& o, const ChunkRecvArgs& polled, size_t n_bb, uint8_t* dibits, size_t cap, size_t* n_dibits,
                       int64_t* sync_pos, uint64_t* sync_dibit, size_t sync_cap, size_t* n_sync)
{
    const size_t C = (size_t)h->C;
    if (int rc = chunk_wait(h, o, polled)) return rc;
    for (size_t c = 0; c < C; ++c)
        if (o.res[c].n_dibits > cap) return P25FE_ERR_CAPACITY;      // before any state moves: the call can be repeated with more room
    for (size_t c = 0; c < C; ++c) {
        const p25fe_result_t& r = o.res[c];
        memcpy(dibits + c * cap, o.dib + c * o.dstride, (size_t)r.n_dibits);
        const size_t ns = r.n_sync < sync_cap ? (size_t)r.n_sync : sync_cap;
        if (ns && sync_pos) memcpy(sync_pos + c * sync_cap, o.spos + c * o.sstride, ns * sizeof(int64_t));
        if (sync_dibit)
            for (size_t k = 0; k < ns; ++k) sync_dibit[c * sync_cap + k] = o.sdib[c * o.sstride + k] + h->state.total_dibits[c];
        n_dibits[c] = (size_t)r.n_dibits;
        if (n_sync) n_sync[c] = (size_t)r.n_sync;
    }
    h->state.commit_recv(o.res, nullptr, n_bb);
    return P25FE_OK;
}

// p25fe_slice, p25fe_run_* and p25fe_run_host_windows each keep their own checks in front (arguments, format, device, capacity, the empty
// call) in their own order: which refusal wins is part of the interface.  Once none applies, the call takes the scratch set:
static int recv_begin(p25fe_t* h) { h->sh.invalidate(); return pipe_join(h, h->stream); }
// ... and an IQ call that succeeded consumes the lock-drop list, moves the stream behind the n samples per channel at `fresh` (rows
// row_bytes apart) and keeps the tail of its last n_bb baseband samples (`tail` [C][TAILN], from k_tail_extract)
static void run_commit(p25fe_t* h, int fmt, size_t n, const char* fresh, size_t row_bytes, size_t n_bb, const float* tail)
{
    h->rs_n = 0;
    h->state.commit_iq((size_t)h->C, fmt, n, fresh, row_bytes);
    for (size_t c = 0; c < (size_t)h->C; ++c) h->state.merge_tail(c, n_bb, h->look, tail + c * TAILN);
}

int p25fe_slice(p25fe_t* h, const float* bb, size_t n, uint8_t* dibits, size_t cap, size_t* n_dibits, int64_t* sync_pos,
                uint64_t* sync_dibit, size_t sync_cap, size_t* n_sync)
{
    if (!h || (!bb && n) || !dibits || !n_dibits || piecewise_refused(h)) return P25FE_ERR_ARG;
    if ((sync_pos || sync_dibit) && !(sync_pos && sync_dibit)) return P25FE_ERR_ARG;
    if (!sync_pos) sync_cap = 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t C = (size_t)h->C;
    if (n == 0) { for (size_t c = 0; c < C; ++c) { n_dibits[c] = 0; if (n_sync) n_sync[c] = 0; } return P25FE_OK; }
    if (cap < n / SPS + 1) return P25FE_ERR_CAPACITY;               // worst case of an undisturbed lock, checked before any state moves
    if (int jrc = recv_begin(h)) return jrc;
    // stage [tail | new] per channel
    const size_t bb_stride = round_up(BBPAD + n + 4, 4);
    HIPCHK(h, h->hbb.ensure(C * bb_stride * sizeof(float)));
    float* hb = static_cast<float*>(h->hbb.p);
    const float* db = static_cast<const float*>(h->hbb.dp);
    for (size_t c = 0; c < C; ++c) {
        memcpy(hb + c * bb_stride, h->state.tail_bb.data() + c * BBPAD, BBPAD * sizeof(float));
        memcpy(hb + c * bb_stride + BBPAD, bb + c * n, n * sizeof(float));
    }
    RecvOut o;
    if (int rc = recv_out(h, n, sync_cap, &o)) return rc;
    const size_t hist = h->state.abs_bb < BBPAD ? (size_t)h->state.abs_bb : BBPAD;
    const RecvCall rcall = host_recv_call(h, o, n, sync_cap != 0);
    RecvChunkArgs a;
    chunk_recv_args(h, rcall, nullptr, &a.r);                       // (not polled unless armed below)
    if (!rcall.gen && n <= (size_t)TS) {
        chunk_poll_arm(h, o, &a.r);
        const PlanarGeo g(n);
        a.bb = db + BBPAD; a.bb_stride = (long)bb_stride; a.n_hist = (long)hist;
        a.f = h->rx().pl_f.get(); a.bits = h->rx().pl_bits.get(); a.n_blocks = (long)g.n_blocks;
        hipLaunchKernelGGL(k_recv_chunk, dim3((unsigned)C), dim3(WV), 0, h->stream, a);
        HIPCHK(h, hipGetLastError());
    } else {
        int rc = launch_planarize(h, db + BBPAD, bb_stride, hist, n, h->stream);
        if (!rc) rc = launch_recv(h, rcall);
        if (rc) return rc;
    }
    if (int rc = recv_finish(h, o, a.r, n, dibits, cap, n_dibits, sync_pos, sync_dibit, sync_cap, n_sync)) return rc;
    h->rs_n = 0;                                                     // (after P25FE_ERR_CAPACITY nothing has moved, this list included -- repeat the call)
    for (size_t c = 0; c < C; ++c)                                   // the tail: last BBPAD samples of [tail | new]
        memcpy(h->state.tail_bb.data() + c * BBPAD, hb + c * bb_stride + n, BBPAD * sizeof(float));
    return P25FE_OK;
}

static int run_host(p25fe_t* h, const void* iq, int fmt, size_t n, uint8_t* dibits, size_t cap, size_t* n_dibits)
{
    if (!h || (!iq && n) || !dibits || !n_dibits || piecewise_refused(h)) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t C = (size_t)h->C;
    const size_t nb = p25fe_n_baseband_h(h, h->state.abs_iq, n);
    if (cap < nb / SPS + 1) return P25FE_ERR_CAPACITY;              // worst case of an undisturbed lock, checked before any state moves
    if (int jrc = recv_begin(h)) return jrc;
    Staged sg;
    if (int rc = stage_iq(h, iq, fmt, n, &sg)) return rc;
    if (nb == 0) {                                                  // fewer than five new samples: only the filters' history moves
        h->state.commit_iq(C, fmt, n, sg.fresh, sg.row_bytes);
        for (size_t c = 0; c < C; ++c) n_dibits[c] = 0;
        return P25FE_OK;
    }
    RecvOut o;
    if (int rc = recv_out(h, nb, 0, &o)) return rc;
    const RecvCall rcall = host_recv_call(h, o, nb, false);
    ChunkRecvArgs cr;
    chunk_recv_args(h, rcall, o.d_tail, &cr);
    K1Launch k = sg.k1;
    if (!rcall.gen && nb <= (size_t)TS) {
        // ONE launch: K1 (planar) + the receiver, run by each channel's last workgroup
        chunk_poll_arm(h, o, &cr);
        k.planar = true; k.chunk = &cr;
        if (int rc = launch_k1(h, k)) return rc;
    } else {
        // the baseband stays in HBM; the receiver's history is recomputed from the IQ history, like a shard's from its halo
        if (int rc = launch_planar_recv(h, k, rcall)) return rc;
        hipLaunchKernelGGL(k_tail_extract, dim3((unsigned)C), dim3(WV), 0, h->stream, cr);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = recv_finish(h, o, cr, nb, dibits, cap, n_dibits, nullptr, nullptr, 0, nullptr)) return rc;
    run_commit(h, fmt, n, sg.fresh, sg.row_bytes, nb, o.tail);
    return P25FE_OK;
}

int p25fe_run_u8(p25fe_t* h, const uint8_t* iq, size_t n_bytes, uint8_t* dibits, size_t cap, size_t* n_dibits)
{
    if (n_bytes & 1) return P25FE_ERR_ARG;
    return run_host(h, iq, P25FE_FMT_U8, n_bytes / 2, dibits, cap, n_dibits);
}

int p25fe_run_cf32(p25fe_t* h, const float* iq, size_t n_samples, uint8_t* dibits, size_t cap, size_t* n_dibits)
{
    return run_host(h, iq, P25FE_FMT_CF32, n_samples, dibits, cap, n_dibits);
}

int p25fe_run_s16(p25fe_t* h, const int16_t* iq, size_t n_samples, uint8_t* dibits, size_t cap, size_t* n_dibits)
{
    return run_host(h, iq, P25FE_FMT_S16, n_samples, dibits, cap, n_dibits);
}

// --------------------------------------------------------------------------------------------
// a long host capture as a pipeline of windows: H2D copy | K1..K4 | dibits D2H, each on its own stream
// --------------------------------------------------------------------------------------------
// The windows of one call.  A remainder of fewer than 8 samples (it may not even yield a baseband sample) rides with the window in front
// of it: every window then produces baseband, and the tail handed to a later p25fe_slice is always the last window's.  That window is
// up to window + 7 samples long: the + 8 of the row stride and of the worst cases.
struct WinPlan {
    size_t C, eb, n, window, n_win;        // channels, bytes per sample; samples of the capture and of a window (clamped); windows
    size_t stride, nb_win, dstride;        // samples per channel row of a device window, [halo | window (+ < 8)]; worst case of a window's baseband, its dibit row
    int fmt, phase; uint64_t abs_iq;       // (abs_iq: where the stream stands before the call)
    WinPlan(size_t n_, size_t win, int fmt_, size_t C_, uint64_t abs_, int ph) : C(C_), eb(fmt_bytes(fmt_)), n(n_), fmt(fmt_), phase(ph), abs_iq(abs_)
    {
        window = (win ? win : (size_t)(64u << 20) / eb) & ~(size_t)7;    // every window's first sample stays 16-byte aligned
        if (window < 8192) window = 8192;
        n_win = (n + window - 1) / window;
        if (n_win >= 2 && n - (n_win - 1) * window < 8) --n_win;
        stride = SHARD_HALO + window + 8; nb_win = (window + 8) / DEC + 2; dstride = dibit_row(nb_win, 64);
    }
    size_t first(size_t k) const { return k * window; }
    size_t len(size_t k) const { return k + 1 == n_win ? n - first(k) : window; }
    size_t n_bb(size_t k) const { return n_baseband_ph(phase, abs_iq + first(k), len(k)); }
    size_t n_bb_before(size_t k) const { return n_baseband_ph(phase, abs_iq, first(k)); }    // ... of all windows in front of k
};
// The pinned block of a call: per ring slot the result records, per parity a dibit row block, the baseband tail (the last window's
// k_tail_extract writes it in place) and what window 0 starts from -- the carry-in anchors and the IQ history.  win_alloc carves and fills it.
struct WinPin { p25fe_result_t* res[WIN_RING]; uint8_t* dib[WIN_PARITY]; float *tail, *d_tail; p25fe_anchor_t* anc; char* hist; };
static int win_alloc(p25fe_t* h, const WinPlan& p, bool staged, WinPin* o)
{
    Windows& w = h->win;
    const size_t C = p.C;
    HIPCHK(h, w.ensure());
    if (int rc = ensure_slice_scratch(h, p.nb_win)) return rc;
    for (DevBuf& d : w.buf) HIPCHK(h, d.ensure(C * p.stride * p.eb));
    for (DevBuf& d : w.dib) HIPCHK(h, d.ensure(C * p.dstride));
    HIPCHK(h, w.res.ensure(WIN_RING * C * sizeof(p25fe_result_t)));
    HIPCHK(h, w.anc.ensure(WIN_PARITY * C * sizeof(p25fe_anchor_t)));
    HIPCHK(h, w.out.ensure(WIN_RING * round_up(C * sizeof(p25fe_result_t), 64) + WIN_PARITY * round_up(C * p.dstride, 64) +
                           round_up(C * TAILN * sizeof(float), 64) + round_up(C * sizeof(p25fe_anchor_t), 64) + round_up(C * SHARD_HALO * p.eb, 64)));
    Arena ar(w.out);
    for (p25fe_result_t*& r : o->res) r = ar.take<p25fe_result_t>(C);
    for (uint8_t*& d : o->dib) d = ar.take<uint8_t>(C * p.dstride);
    o->tail = ar.take<float>(C * TAILN, &o->d_tail);
    o->anc = ar.take<p25fe_anchor_t>(C);
    o->hist = ar.take<char>(C * SHARD_HALO * p.eb);
    if (staged) for (PinBuf& s : w.stage) HIPCHK(h, s.ensure(C * p.stride * p.eb));
    memcpy(o->anc, h->state.anchor.data(), C * sizeof(p25fe_anchor_t));
    h->state.stage_hist(p.fmt, o->hist, SHARD_HALO * p.eb);
    return P25FE_OK;
}
// Window k on its three streams; a stage returns at its first error.  Copy stream: [halo | window] in ONE copy.  The halo of window
// k >= 1 is simply the SHARD_HALO samples in front of it in the caller's capture (16 KB more per window); only window 0 takes it from the
// handle's history.  (A device-to-device copy of the previous window's tail put a second operation between every two H2D copies: 7 - 9 %.)
static int win_copy_in(p25fe_t* h, const WinPlan& p, const WinPin& o, const char* iq, bool pinned, size_t k)
{
    Windows& w = h->win;
    const size_t b = k % WIN_PARITY, eb = p.eb;
    const size_t lead = k == 0 ? 0 : SHARD_HALO;                    // samples in front of the window that travel with it
    const size_t row = (lead + p.len(k)) * eb;
    char* dst = w.buf[b].as<char>() + (SHARD_HALO - lead) * eb;
    if (k >= WIN_PARITY) HIPCHK(h, hipStreamWaitEvent(w.cs, w.of(k - WIN_PARITY).comp_end, 0));       // the kernels of window k - 2 have read this device window
    if (k == 0) HIPCHK(h, hipMemcpy2DAsync(dst - SHARD_HALO * eb, p.stride * eb, o.hist, SHARD_HALO * eb, SHARD_HALO * eb, p.C, hipMemcpyHostToDevice, w.cs));
    const char* src = iq + (p.first(k) - lead) * eb;
    size_t spitch = p.n * eb;
    if (!pinned) {                                                   // pageable memory: this thread stages the rows
        if (k >= WIN_PARITY) HIPCHK(h, hipEventSynchronize(w.of(k - WIN_PARITY).h2d_end));            // the copy engine is done with this staging window
        char* sg = static_cast<char*>(w.stage[b].p);
        for (size_t c = 0; c < p.C; ++c) memcpy(sg + c * row, src + c * p.n * eb, row);
        src = sg; spitch = row;
    }
    HIPCHK(h, hipEventRecord(w.of(k).h2d_begin, w.cs));
    if (p.C == 1) HIPCHK(h, hipMemcpyAsync(dst, src, row, hipMemcpyHostToDevice, w.cs));
    else HIPCHK(h, hipMemcpy2DAsync(dst, p.stride * eb, src, spitch, row, p.C, hipMemcpyHostToDevice, w.cs));
    HIPCHK(h, hipEventRecord(w.of(k).h2d_end, w.cs));
    return P25FE_OK;
}
// Compute stream (the handle's): K1 .. K4 on the device window, the next window's carry-in anchors, behind the last window the baseband tail
static int win_compute(p25fe_t* h, const WinPlan& p, const WinPin& o, size_t k)
{
    Windows& w = h->win;
    hipStream_t st = h->stream;
    const size_t b = k % WIN_PARITY, C = p.C;
    p25fe_anchor_t* d_anc = w.anc.as<p25fe_anchor_t>();             // [WIN_PARITY][C]: window k finds its carry-in in row b and leaves window k + 1's in the other
    p25fe_result_t* d_res = w.res.as<p25fe_result_t>() + k % WIN_RING * C;
    HIPCHK(h, hipStreamWaitEvent(st, w.of(k).h2d_end, 0));
    if (k >= WIN_PARITY) HIPCHK(h, hipStreamWaitEvent(st, w.of(k - WIN_PARITY).on_host, 0));          // window k - 2's dibit rows have left this device row block
    if (k == 0) HIPCHK(h, hipMemcpyAsync(d_anc, o.anc, C * sizeof(p25fe_anchor_t), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipEventRecord(w.of(k).comp_begin, st));
    K1Launch k1;
    k1.src = w.buf[b].as<char>() + SHARD_HALO * p.eb; k1.fmt = p.fmt; k1.ch_stride = p.stride; k1.n_hist = k == 0 ? h->state.n_hist() : SHARD_HALO;
    k1.n = p.len(k); k1.abs0 = p.abs_iq + p.first(k); k1.stream = st;
    RecvCall rc = recv_call(h);                                      // (a pending lock-drop list holds absolute indices: every window sees it)
    rc.range.n_bb = p.n_bb(k); rc.range.abs_bb0 = (long)(h->state.abs_bb + p.n_bb_before(k)) - h->look; rc.range.anchor_in = d_anc + b * C;
    rc.dest.dibits = w.dib[b].as<uint8_t>(); rc.dest.dibit_stride = p.dstride; rc.dest.result = d_res; rc.stream = st;
    if (int lrc = launch_planar_recv(h, k1, rc)) return lrc;
    hipLaunchKernelGGL(k_anchors_from_results, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, d_res, d_anc + (k + 1) % WIN_PARITY * C, (int)C);
    if (k + 1 == p.n_win) {                                          // the baseband tail for a later p25fe_slice on this handle
        ChunkRecvArgs cr;
        chunk_recv_args(h, rc, o.d_tail, &cr);
        hipLaunchKernelGGL(k_tail_extract, dim3((unsigned)C), dim3(WV), 0, st, cr);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(w.of(k).comp_end, st));
    return P25FE_OK;
}
// Result stream: the window's result records and dibit rows leave for pinned memory
static int win_copy_out(p25fe_t* h, const WinPlan& p, const WinPin& o, size_t k)
{
    Windows& w = h->win;
    const size_t b = k % WIN_PARITY, q = k % WIN_RING;
    HIPCHK(h, hipStreamWaitEvent(w.os, w.of(k).comp_end, 0));
    HIPCHK(h, hipMemcpyAsync(o.res[q], w.res.as<p25fe_result_t>() + q * p.C, p.C * sizeof(p25fe_result_t), hipMemcpyDeviceToHost, w.os));
    HIPCHK(h, hipMemcpyAsync(o.dib[b], w.dib[b].as<uint8_t>(), p.C * p.dstride, hipMemcpyDeviceToHost, w.os));
    HIPCHK(h, hipEventRecord(w.of(k).on_host, w.os));
    return P25FE_OK;
}
// This thread: window j's dibits are on the host, append them to the caller's rows (total: dibits per channel so far)
static int win_drain(p25fe_t* h, const WinPlan& p, const WinPin& o, size_t j, uint8_t* dibits, size_t cap, uint64_t* total, p25fe_windows_stats_t* st)
{
    const WinSlot& s = h->win.of(j);
    HIPCHK(h, hipEventSynchronize(s.on_host));
    float t = 0.f;
    if (hipEventElapsedTime(&t, s.h2d_begin, s.h2d_end) == hipSuccess) st->ms_h2d += t; else (void)hipGetLastError();
    if (hipEventElapsedTime(&t, s.comp_begin, s.comp_end) == hipSuccess) st->ms_compute += t; else (void)hipGetLastError();
    const p25fe_result_t* r = o.res[j % WIN_RING];
    for (size_t c = 0; c < p.C; ++c) {
        const uint64_t nd = r[c].n_dibits;
        if (nd > p.dstride || total[c] + nd > cap) return P25FE_ERR_CAPACITY;
        memcpy(dibits + c * cap + total[c], o.dib[j % WIN_PARITY] + c * p.dstride, (size_t)nd);
        total[c] += nd;
    }
    return P25FE_OK;
}

int p25fe_run_host_windows(p25fe_t* h, const void* iq, int fmt, size_t n, size_t window, uint8_t* dibits, size_t cap,
                           size_t* n_dibits, p25fe_windows_stats_t* stats)
{
    // ---- guard
    if (!h || (!iq && n) || !dibits || !n_dibits || piecewise_refused(h)) return P25FE_ERR_ARG;
    if (int frc = format_unusable(h, fmt)) return frc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->state.format_refused(fmt)) return P25FE_ERR_FORMAT;
    const size_t C = (size_t)h->C;
    const WinPlan p(n, window, fmt, C, h->state.abs_iq, h->phase);
    const size_t nb_all = p25fe_n_baseband_h(h, h->state.abs_iq, n);
    if (cap < nb_all / SPS + 1) return P25FE_ERR_CAPACITY;          // worst case of an undisturbed lock, before any state moves
    if (stats) memset(stats, 0, sizeof *stats);
    for (size_t c = 0; c < C; ++c) n_dibits[c] = 0;
    if (n == 0) return P25FE_OK;
    if (n <= p.window && n <= (size_t)(1u << 20)) {                 // one small window: the streaming call does the same with less set-up
        if (stats) stats->n_windows = 1;
        return run_host(h, iq, fmt, n, dibits, cap, n_dibits);
    }
    if (int jrc = recv_begin(h)) return jrc;
    const auto t_begin = std::chrono::steady_clock::now();
    // ---- allocate.  Is the caller's memory pinned?  (then the copy engine reads it directly; otherwise this thread stages it)
    bool pinned = false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, iq) == hipSuccess) pinned = at.type == hipMemoryTypeHost; else (void)hipGetLastError();
    WinPin pin;
    if (int arc = win_alloc(h, p, !pinned, &pin)) return arc;
    std::vector<uint64_t> total(C, 0);
    p25fe_windows_stats_t st = {};
    // ---- the pipeline (an error must not return at once: copies that read the caller's capture are in flight)
    int status = P25FE_OK;
    for (size_t k = 0; k < p.n_win && status == P25FE_OK; ++k) {
        status = win_copy_in(h, p, pin, static_cast<const char*>(iq), pinned, k);
        if (status == P25FE_OK) status = win_compute(h, p, pin, k);
        if (status == P25FE_OK) status = win_copy_out(h, p, pin, k);
        if (status == P25FE_OK && k >= 1) status = win_drain(h, p, pin, k - 1, dibits, cap, total.data(), &st);
    }
    if (status == P25FE_OK) status = win_drain(h, p, pin, p.n_win - 1, dibits, cap, total.data(), &st);
    if (status != P25FE_OK) {
        // Nothing of the handle's STREAM STATE has moved (history, anchors, counters: the call can be repeated), and no copy or
        // kernel of this call is still in flight when it returns: they read the caller's capture and the handle's windows.
        // The caller's dibit buffer may already hold the dibits of earlier windows and n_dibits reads 0: treat both as undefined.
        (void)hipStreamSynchronize(h->win.cs); (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->win.os);
        return status;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // ---- commit
    for (size_t c = 0; c < C; ++c) n_dibits[c] = (size_t)total[c];
    h->state.commit_recv(pin.res[(p.n_win - 1) % WIN_RING], total.data(), nb_all);
    run_commit(h, fmt, n, static_cast<const char*>(iq), n * p.eb, p.n_bb(p.n_win - 1), pin.tail);
    st.n_windows = p.n_win; st.pinned_input = pinned ? 1 : 0;
    st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return P25FE_OK;
}

int p25fe_nid_dev(p25fe_t* h, const uint8_t* d_dibits, size_t n_dibits, const uint64_t* d_sync_dibit,
                  const int64_t* d_sync_pos, size_t n_sync, p25fe_nid_t* d_out, void* stream)
{
    if (!h) return P25FE_ERR_ARG;
    if (n_sync == 0) return P25FE_OK;
    if (!d_dibits || !d_sync_dibit || !d_out) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_nid, dim3((unsigned)n_sync), dim3(256), 0, (hipStream_t)stream, d_dibits,
                       (unsigned long long)n_dibits, reinterpret_cast<const unsigned long long*>(d_sync_dibit),
                       reinterpret_cast<const long*>(d_sync_pos), d_out, (const p25fe_result_t*)nullptr, 0ull, 0ull);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

// host-buffer form for the file-driven harness: one channel's whole dibit stream and its sync events
int p25fe_nid(p25fe_t* h, const uint8_t* dibits, size_t n_dibits, const uint64_t* sync_dibit, const int64_t* sync_pos,
              size_t n_sync, p25fe_nid_t* out)
{
    if (!h) return P25FE_ERR_ARG;
    if (n_sync == 0) return P25FE_OK;                               // a capture without a frame sync: nothing to decode (empty vectors hand over null pointers)
    if ((!dibits && n_dibits) || !sync_dibit || !out) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf d_dib, d_sd, d_sp, d_out;
    int rc = P25FE_OK;
    hipError_t e = d_dib.ensure(n_dibits + 16);
    if (e == hipSuccess) e = d_sd.ensure(n_sync * sizeof(uint64_t));
    if (e == hipSuccess) e = d_out.ensure(n_sync * sizeof(p25fe_nid_t));
    if (e == hipSuccess && sync_pos) e = d_sp.ensure(n_sync * sizeof(int64_t));
    if (e == hipSuccess && n_dibits) e = hipMemcpyAsync(d_dib.p, dibits, n_dibits, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sd.p, sync_dibit, n_sync * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && sync_pos) e = hipMemcpyAsync(d_sp.p, sync_pos, n_sync * sizeof(int64_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        rc = p25fe_nid_dev(h, d_dib.as<uint8_t>(), n_dibits, d_sd.as<uint64_t>(), sync_pos ? d_sp.as<int64_t>() : nullptr,
                           n_sync, d_out.as<p25fe_nid_t>(), h->stream);
        if (rc == P25FE_OK) e = hipMemcpyAsync(out, d_out.p, n_sync * sizeof(p25fe_nid_t), hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->last_hip = (int)e; return P25FE_ERR_HIP; }
    return rc;
}

int p25fe_nid_batch_dev(p25fe_t* h, const uint8_t* d_dibits, size_t dibit_stride, const p25fe_result_t* d_result,
                        const uint64_t* d_sync_dibit, const int64_t* d_sync_pos, size_t sync_stride,
                        p25fe_nid_t* d_out, void* stream)
{
    if (!h || !d_dibits || !d_result || !d_sync_dibit || !d_out) return P25FE_ERR_ARG;
    if (sync_stride == 0) return P25FE_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_nid, dim3((unsigned)sync_stride, (unsigned)h->C), dim3(256), 0, (hipStream_t)stream, d_dibits,
                       0ull, reinterpret_cast<const unsigned long long*>(d_sync_dibit),
                       reinterpret_cast<const long*>(d_sync_pos), d_out, d_result, (unsigned long long)dibit_stride,
                       (unsigned long long)sync_stride);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_chan_stats_dev(p25fe_t* h, const p25fe_result_t* d_result, const p25fe_nid_t* d_nid, size_t sync_stride,
                         const float* d_power_dbm, p25fe_chan_stats_t* d_stats, void* stream)
{
    if (!h || !d_result || !d_stats) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_chan_stats, dim3((unsigned)h->C), dim3(256), 0, (hipStream_t)stream, d_result, d_nid,
                       (unsigned long long)sync_stride, d_power_dbm, d_stats);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_profile_enable(p25fe_t* h, int on)
{
    if (!h) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (on && h->prof.ev.empty()) {
        try {
            h->prof.ev.assign((size_t)PROF_RING * 5, nullptr);
            h->prof.mask.assign((size_t)PROF_RING, 0);
        } catch (...) {
            h->prof.ev.clear();
            return P25FE_ERR_NOMEM;
        }
        for (auto& e : h->prof.ev) {
            const hipError_t er = hipEventCreate(&e);
            if (er != hipSuccess) {                                 // all or nothing: a half-made ring is never indexed
                for (auto& d : h->prof.ev) if (d) (void)hipEventDestroy(d);
                h->prof.ev.clear();
                h->last_hip = (int)er;
                return P25FE_ERR_HIP;
            }
        }
    }
    h->prof.on = on != 0;
    h->prof.level = on == 2 ? 2 : (on == 3 ? 3 : 1);
    h->prof.calls = 0;
    h->prof.seq = 0;
    return P25FE_OK;
}

int p25fe_profile_read(p25fe_t* h, double ms[4], uint64_t* n_calls)
{
    if (!h || !ms) return P25FE_ERR_ARG;
    for (int k = 0; k < 4; ++k) ms[k] = 0.0;
    const uint64_t calls = h->prof.calls;
    const uint64_t kept = calls < (uint64_t)PROF_RING ? calls : (uint64_t)PROF_RING;
    uint64_t n_k1 = 0;
    for (uint64_t s = 0; s < kept; ++s) {
        const unsigned m = h->prof.mask[s];                          // a slot holds the events its call recorded: all five
        if ((m & 3u) == 3u) ++n_k1;
        for (int k = 4; k >= 0; --k)                                 // (run_dev, shard pass 1) or 2..4 (shard pass 2)
            if (m & (1u << k)) { HIPCHK(h, hipEventSynchronize(h->prof.ev[s * 5 + k])); break; }
        for (int k = 0; k < 4; ++k) {
            if ((m & (3u << k)) != (3u << k)) continue;
            float t = 0.f;
            if (hipEventElapsedTime(&t, h->prof.ev[s * 5 + k], h->prof.ev[s * 5 + k + 1]) != hipSuccess) {
                (void)hipGetLastError();                             // a slot whose launch had nothing to do (empty part of a shard)
                if (k == 0 && n_k1) --n_k1;
                continue;
            }
            ms[k] += t;
        }
    }
    if (n_calls) *n_calls = n_k1;          // calls that ran K1 (a shard's pass 2 has a slot of its own without one)
    h->prof.calls = 0;
    return P25FE_OK;
}

int p25fe_resync(p25fe_t* h)
{
    if (!h) return P25FE_ERR_ARG;
    for (auto& a : h->state.anchor) a.valid = 0;      // lock and, with it, the clock estimate (the next sync word starts from 10 / 1)
    return P25FE_OK;
}

int p25fe_resync_at_dev(p25fe_t* h, const int64_t* d_idx, size_t n_idx, size_t idx_stride)
{
    if (!h || (n_idx && !d_idx) || n_idx > 0x7fffffffu || (h->C > 1 && n_idx && idx_stride < n_idx)) return P25FE_ERR_ARG;
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    h->rs_idx = reinterpret_cast<const long*>(d_idx);
    h->rs_n = n_idx; h->rs_stride = idx_stride;
    return P25FE_OK;
}

// --------------------------------------------------------------------------------------------
// state blob (StreamState::write / read)
// --------------------------------------------------------------------------------------------
int p25fe_state_size(const p25fe_t* h, size_t* n)
{
    if (!h || !n) return P25FE_ERR_ARG;
    *n = const_cast<p25fe_t*>(h)->state.blob_size();
    return P25FE_OK;
}

int p25fe_state_export(const p25fe_t* hc, void* buf, size_t cap, size_t* n)
{
    p25fe_t* h = const_cast<p25fe_t*>(hc);
    size_t need = 0;
    if (!h || !buf || p25fe_state_size(h, &need)) return P25FE_ERR_ARG;
    if (n) *n = need;
    if (cap < need) return P25FE_ERR_CAPACITY;
    h->state.write(static_cast<char*>(buf));
    return P25FE_OK;
}

int p25fe_state_import(p25fe_t* h, const void* buf, size_t n)
{
    size_t need = 0;
    if (!h || !buf || p25fe_state_size(h, &need) || n < need) return P25FE_ERR_ARG;
    if (!h->state.read(static_cast<const char*>(buf), h->track)) return P25FE_ERR_ARG;
    h->rs_idx = nullptr; h->rs_n = 0; h->rs_stride = 0;             // (absolute indices of another stream position)
    return P25FE_OK;
}

P25FE_M_API_EXTRAS
}  // extern "C"

#include "p25fe_scan.inc"       // survey (SPEC 3.0h): k_scan and its entry points
#include "p25fe_waterfall.inc"  // survey over time (SPEC 3.0i): k_waterfall and its entry points
#include "p25fe_cuts.inc"       // tuner, cuts (SPEC 3.0j): the entry points of k_tune_cuts
#include "p25fe_keys.inc"       // survey over time, keys on the device (SPEC 3.0k): k_keys_pow / _walk / _cell and their entry points
