// p25fe_replay -- file-in / file-out driver in the role of the reference's command line for this path
// (src/main.rs:95-102, 162-175, 278-283 and src/replay.rs:26-57): a deterministic harness for the hot path.
//
//   p25fe_replay [-w BB.f32le] [-j EVENTS.jsonl] [-b CHUNKS] [-r RATE_HZ [-S MS] [-f OFFSET_HZ | -F OFFSET_HZ [-a MS | -A MS]]] u8|s16|cf32|bb <in> <dibits.out>
//   p25fe_replay -W WINDOW_BYTES u8|s16|cf32 <in> <dibits.out>
//
//     u8    RTL-SDR style interleaved u8 I/Q, the reference's live input (src/consts.rs:6: 32768-byte chunks)
//     s16   interleaved little-endian int16 I/Q at 240 ksps (Airspy, SDRplay, USRP sc16, SigMF ci16_le), 16384 samples per chunk
//     cf32  Complex32 I/Q at 240 ksps
//     bb    48 kHz f32le baseband: what `p25rx -w FILE` records and `p25rx -r FILE` replays (src/main.rs:95-102)
//
//     -w FILE   write the baseband as f32le / 48 kHz / mono while receiving -- the reference's `-w`
//               (src/main.rs:99-102, 174-175): RecvTask::run hands every chunk to a callback AFTER feeding it
//               (src/recv.rs:152), and the callback appends it to the file (src/main.rs:278-283).
//               `p25fe_replay bb FILE ...` on that file reproduces the dibits of the recording run.
//     -j FILE   JSON lines in the vocabulary of the reference's hub: {"event":"sigPower"} per power report
//               (HubEvent::UpdateSignalPower, src/demod.rs:95-101, src/hub.rs:344), {"event":"nid"} per frame sync
//               (MessageEvent::PacketNID, src/recv.rs:216-222), {"event":"updateStats","periodic":true} after every 16th
//               baseband chunk (Throttler::new(16), src/recv.rs:141, 162-165), one final {"event":"updateStats"} with
//               the "bch" row of serialize_stats (src/hub.rs:401-402, 559, 574-581).
//     -b N      file chunks per library call (default 64; 1 = the reference's cadence of one 32768-byte buffer per
//               DemodTask iteration, which also fixes the every-4th-chunk power report of src/demod.rs:67, 95).
//               The dibits do not depend on N (streaming semantics); only the PCIe transfer size does.
//
//     -r HZ     the capture's sample rate when it is not 240 ksps (u8, s16, cf32): every chunk first goes through the rational
//               resampler (docs/SPEC.md 3.0b) with the table p25fe_resampler_design gives for HZ -- 2.5 or 10 Msps of an Airspy
//               R2, 2.048 Msps of an RTL-SDR, ... -- and the 240 ksps cf32 stream it returns takes the cf32 mode's path.
//
//     -f HZ     with -r: the channel's offset from the capture's centre in Hz (negative: below it).  The chunks then go through the
//               tuner (docs/SPEC.md 3.0c, p25fe_tune) with the same table: OFFSET_HZ / RATE_HZ in lowest terms must have a
//               denominator of at most 8192, which every 12.5 kHz or 6.25 kHz raster at the customary rates has.
//
//     -F HZ     with -r, instead of -f: the offset as a decimal that may be fractional, at any value up to half the rate -- a channel
//               off the raster, or on it with the crystal's ppm error taken out.  The chunks go through the tuner's NCO channel
//               (docs/SPEC.md 3.0d, p25fe_nco_create) at the step p25fe_nco_step gives: the nearest multiple of RATE_HZ / 2^32.
//
//     -a MS     with -F: automatic frequency correction.  The first MS ms of the capture are tuned at -F's offset while the GPU
//               measures the tuned row's frequency error (docs/SPEC.md 3.0f, p25fe_afc_measure_dev, the recommended prefilter);
//               then the channel's step is corrected ONCE by the estimate, without a phase jump (3.0e, p25fe_afc_set_step), and
//               the stream carries on.  The estimate is printed, and goes to the -j events as {"event":"afc", ...}.
//
//     -A MS     with -F, instead of -a: the AFC loop (docs/SPEC.md 3.0g).  The measure runs on every chunk, reads are cut at the
//               multiples of MS ms of input, and at each of them ONE kernel updates the channel's step on the device from the window's
//               record (the recommended loop: gate 0.75, gain 1, half a window of products); the state is read back and printed as
//               an {"event":"afc", ...} line per boundary, in -a's format plus "status".
//
//     -S MS     with -r: the survey (docs/SPEC.md 3.0h).  The first MS ms of the capture go through p25fe_scan (N = 4096, hop 2048, the
//               designed window, shift 16), and the active channels of the 12.5 kHz raster (p25fe_scan_channels: +-4 kHz, 20 dB over
//               the median channel) are printed as ONE line {"event":"scan","n_frames":..,"channels":[{"raster_index","centre_hz",
//               "db_over_floor","offset_hz"}, ..]}, strongest first, on stdout and in the -j events.  With neither -f nor -F the run
//               ends there with status 0 and <dibits.out> is not touched; with one of them it goes on as without -S, from the start
//               of the input: centre_hz + offset_hz of a channel is what -F takes.
//
//     -W BYTES  bulk mode for long captures (p25fe_run_host_windows): a READER THREAD fills pinned blocks of eight windows
//               from the file while the library pipelines the previous block -- window k + 1 on its way to the GPU,
//               window k in the kernels, window k - 1's dibits on their way back.  The shape of the reference's own loop (a
//               reader feeding a pool of buffers to the demodulator, src/sdr.rs:25-33, src/demod.rs:62-70) at bus speed;
//               same dibits as the chunked modes.  BYTES takes k / M suffixes (64M is the library's default).
//
// Wires DemodTask -> RecvTask exactly like src/main.rs:270-287, single-threaded through in-memory channels.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "p25fe_host.hpp"

using namespace p25rx;

template <class T> struct Chan {
    std::deque<T> q;
    void send(T v) { q.push_back(std::move(v)); }
    bool recv(T& v)
    {
        if (q.empty()) return false;
        v = std::move(q.front());
        q.pop_front();
        return true;
    }
};

// hub side of the harness: power reports become JSON lines as they arrive
struct Hub {
    FILE* js = nullptr;
    size_t n_power = 0;
    size_t n_stats = 0;
    ~Hub() { if (js) std::fclose(js); }
    void send(HubEvent e)
    {
        ++n_power;
        if (js) std::fprintf(js, "{\"event\":\"sigPower\",\"dbm\":%.4f}\n", (double)e.signal_power_dbm);
    }
    void send(StatsEvent e)                                           // every 16th receiver event, src/recv.rs:141, 162-165
    {
        ++n_stats;
        if (js) std::fprintf(js, "{\"event\":\"updateStats\",\"periodic\":true,\"dibits\":%" PRIu64 ",\"syncs\":%" PRIu64 "}\n", e.dibits, e.syncs);
    }
};

struct Sink {
    std::ofstream out;
    std::vector<uint8_t> all_dibits;            // kept for the NID pass at the end of the file (-j)
    std::vector<int64_t> sync_pos;
    std::vector<uint64_t> sync_dibit;
    bool keep = false;
    size_t n_sync = 0, n_dibits = 0;
    void send(Symbols s)
    {
        out.write(reinterpret_cast<const char*>(s.dibits.data()), (std::streamsize)s.dibits.size());
        n_dibits += s.dibits.size();
        n_sync += s.sync_pos.size();
        if (keep) {
            all_dibits.insert(all_dibits.end(), s.dibits.begin(), s.dibits.end());
            sync_pos.insert(sync_pos.end(), s.sync_pos.begin(), s.sync_pos.end());
            sync_dibit.insert(sync_dibit.end(), s.sync_dibit.begin(), s.sync_dibit.end());
        }
    }
};

static int usage(const char* argv0)
{
    std::fprintf(stderr, "usage: %s [-w BB.f32le] [-j EVENTS.jsonl] [-b CHUNKS] [-r RATE_HZ [-S MS] [-f OFFSET_HZ | -F OFFSET_HZ [-a MS | -A MS]]] u8|s16|cf32|bb <in> <dibits.out>\n"
                         "       %s -W WINDOW_BYTES u8|s16|cf32 <in> <dibits.out>\n"
                         "       %s -r RATE_HZ -T MS u8|s16|cf32 <in> <unused>\n", argv0, argv0, argv0);
    return 2;
}

// an error that ends the run with a message and status 1 (the library's own abort in `expect`): thrown, so that the owners let go
struct Exit { int status; };
[[noreturn]] __attribute__((format(printf, 1, 2))) static void fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
    throw Exit{1};
}

struct Options {
    const char *in_path = nullptr, *out_path = nullptr, *wpath = nullptr, *jpath = nullptr;
    size_t batch = 64, window_bytes = 0;                              // window_bytes != 0: bulk mode
    unsigned long rate_hz = 0;                                        // -r; 0: the capture is at 240 ksps
    struct { enum { NONE, RATIONAL, NCO } kind = NONE; long long hz = 0; double nco_hz = 0.0; } offset;   // -f: hz; -F: nco_hz
    double afc_ms = 0.0;                                              // -a: measure the first MS ms at -F's offset, correct once
    double track_ms = 0.0;                                            // -A: the loop, updated at every multiple of MS ms of input
    double scan_ms = 0.0;                                             // -S: survey the first MS ms, print the active raster channels
    double activity_ms = 0.0;                                         // -T: survey the whole input in slots of MS ms, print the keyed intervals
    bool bb = false;                                                  // the mode: 48 kHz baseband, or ...
    int fmt = 0; size_t bps = 0;                                      // ... IQ in this format (P25FE_FMT_*) of this many bytes per sample
};

// -T: frames of hop 2048 per slot of MS ms, at least one
static uint64_t activity_slot_frames(const Options& o)
{
    return (uint64_t)std::max(1.0, std::floor(o.activity_ms * (double)o.rate_hz / 1000.0 / 2048.0 + 0.5));
}

// argv -> Options; false: a usage error (all of them are decided here, before anything is opened or created)
static bool parse(int argc, char** argv, Options& o)
{
    bool f = false, F = false;                                        // -f and -F exclude each other
    bool b = false;                                                   // -b was given (-T takes no other option but -r)
    const auto number = [](const char* s, double& v) { char* end = nullptr; v = std::strtod(s, &end); return end != s && *end == '\0'; };
    int a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1] != '\0'; a += 2) {
        if (a + 1 >= argc) return false;
        const std::string opt = argv[a];
        const char* val = argv[a + 1];
        if (opt == "-w") o.wpath = val;
        else if (opt == "-j") o.jpath = val;
        else if (opt == "-b") { o.batch = (size_t)std::strtoull(val, nullptr, 10); b = true; }
        else if (opt == "-r") { if ((o.rate_hz = std::strtoul(val, nullptr, 10)) == 0 || o.rate_hz > 0xfffffffful) return false; }
        else if (opt == "-f") { o.offset.hz = std::strtoll(val, nullptr, 10); f = true; }
        else if (opt == "-F") { if (!number(val, o.offset.nco_hz)) return false; F = true; }
        else if (opt == "-a") { if (!number(val, o.afc_ms) || !(o.afc_ms > 0.0) || o.afc_ms > 60000.0) return false; }
        else if (opt == "-A") { if (!number(val, o.track_ms) || !(o.track_ms > 0.0) || o.track_ms > 60000.0) return false; }
        else if (opt == "-S") { if (!number(val, o.scan_ms) || !(o.scan_ms > 0.0) || o.scan_ms > 60000.0) return false; }
        else if (opt == "-T") { if (!number(val, o.activity_ms) || !(o.activity_ms > 0.0) || o.activity_ms > 60000.0) return false; }
        else if (opt == "-W") {
            char* end = nullptr;
            o.window_bytes = (size_t)std::strtoull(val, &end, 10);
            o.window_bytes <<= (*end == 'k' || *end == 'K') ? 10 : (*end == 'm' || *end == 'M') ? 20 : 0;
        }
        else return false;
    }
    if (argc - a != 3 || o.batch == 0 || (f && F) || ((f || F) && !o.rate_hz) || (o.afc_ms > 0.0 && !F)) return false;
    if (o.track_ms > 0.0 && (!F || o.afc_ms > 0.0)) return false;   // -A goes with -F and instead of -a
    if (o.scan_ms > 0.0 && !o.rate_hz) return false;                 // -S goes with -r
    if (o.activity_ms > 0.0 && (!o.rate_hz || o.scan_ms > 0.0 || f || F || o.afc_ms > 0.0 || o.track_ms > 0.0 || o.wpath || o.jpath || b ||
                                o.window_bytes)) return false;       // -T goes with -r and with nothing else
    if (o.activity_ms > 0.0 && activity_slot_frames(o) > ((uint64_t)1 << 20)) return false;   // more frames a slot than the library takes
    o.offset.kind = F ? o.offset.NCO : (f ? o.offset.RATIONAL : o.offset.NONE);
    const std::string mode = argv[a];
    o.in_path = argv[a + 1]; o.out_path = argv[a + 2];
    if (mode == "u8") { o.fmt = P25FE_FMT_U8; o.bps = 2; }
    else if (mode == "s16") { o.fmt = P25FE_FMT_S16; o.bps = 4; }
    else if (mode == "cf32") { o.fmt = P25FE_FMT_CF32; o.bps = 8; }
    else if (mode == "bb") o.bb = true;
    else return false;
    if (o.bb && (o.rate_hz || o.window_bytes)) return false;         // the resampler, the tuner and the bulk mode take IQ
    return !(o.window_bytes && (o.wpath || o.jpath || o.rate_hz || o.afc_ms > 0.0 || o.track_ms > 0.0 || o.scan_ms > 0.0));
}

// device memory (hipMalloc) or pinned host memory (hipHostMalloc); p is null when there was none: the caller has the message
struct HipMem {
    void* p = nullptr;
    const bool pinned;
    HipMem(size_t bytes, bool pin) : pinned(pin) { if ((pin ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) != hipSuccess) p = nullptr; }
    ~HipMem() { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
    HipMem(const HipMem&) = delete;
};

// bulk mode: reader thread -> two pinned blocks -> p25fe_run_host_windows
static int bulk(Handle& h, const Options& o, std::ifstream& in)
{
    const size_t eb = o.bps;
    const size_t window = o.window_bytes / eb / 8 * 8;
    if (window < 8192) { std::fprintf(stderr, "window too small\n"); return 2; }
    const size_t block = 8 * window;                                  // samples per pinned block: the reader fills one while the library pipelines the other
                                                                      // (measured on a 1.15 GB file from the page cache: 8 windows 78 ms, 2 windows 93 - 105 ms;
                                                                      // the single reader thread's ~15 GB/s is what bounds this mode, not the bus)
    const HipMem pinned[2] = {HipMem(block * eb, true), HipMem(block * eb, true)};
    char* const buf[2] = {static_cast<char*>(pinned[0].p), static_cast<char*>(pinned[1].p)};
    if (!buf[0] || !buf[1]) { std::fprintf(stderr, "unable to allocate pinned blocks\n"); return 1; }
    std::mutex mu;
    std::condition_variable cv;
    size_t filled[2] = {0, 0};
    bool full[2] = {false, false}, eof = false, stop = false;      // stop: the consumer gave up (an error): the reader must not block
    std::thread reader([&] {
        for (int b = 0;; b ^= 1) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !full[b] || stop; });
                if (stop) return;
            }
            in.read(buf[b], (std::streamsize)(block * eb));
            const size_t got = (size_t)in.gcount() / eb;
            std::lock_guard<std::mutex> lk(mu);
            filled[b] = got; full[b] = true; eof = got < block;
            cv.notify_all();
            if (got < block) return;
        }
    });
    std::ofstream out(o.out_path, std::ios::binary);
    std::vector<uint8_t> dib(block / 30 + 4);
    size_t total = 0, samples = 0, windows = 0;
    double ms_h2d = 0.0, ms_comp = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    int failed = 0;                                                  // an error ends the loop, never the process: the reader thread is joinable
    if (!out) { std::fprintf(stderr, "unable to open %s\n", o.out_path); failed = 1; }
    for (int b = 0; !failed; b ^= 1) {
        size_t n;
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return full[b]; }); n = filled[b]; }
        size_t nd = 0;
        p25fe_windows_stats_t st;
        const int rc = p25fe_run_host_windows(h.get(), buf[b], o.fmt, n, window, dib.data(), dib.size(), &nd, &st);
        if (rc != P25FE_OK) {
            std::fprintf(stderr, "p25fe_replay: unable to run the capture: %s (%d)\n", p25fe_strerror(rc), rc);
            failed = 1;
            break;
        }
        out.write(reinterpret_cast<const char*>(dib.data()), (std::streamsize)nd);
        if (!out.good()) { std::fprintf(stderr, "p25fe_replay: write error on %s (disk full?)\n", o.out_path); failed = 1; break; }
        total += nd; samples += n; windows += st.n_windows; ms_h2d += st.ms_h2d; ms_comp += st.ms_compute;
        bool last;
        { std::lock_guard<std::mutex> lk(mu); full[b] = false; last = eof && n < block; cv.notify_all(); }
        if (last || n < block) break;
    }
    { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); }
    reader.join();
    out.close();
    if (!failed && out.fail()) { std::fprintf(stderr, "p25fe_replay: write error on %s at close\n", o.out_path); failed = 1; }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (failed) return 1;
    std::fprintf(stderr, "p25fe_replay: %zu dibits from %zu samples in %zu windows, %.1f ms (%.1f Msamples/s, %.2f GB/s; H2D copies %.1f ms, "
                         "kernels %.1f ms)\n", total, samples, windows, ms, samples / ms / 1e3, samples * eb / ms / 1e6, ms_h2d, ms_comp);
    return 0;
}

// The read loop of every chunked mode: the next chunk -- len() elements, a final short read cut to whole units -- goes into the
// front of the chain (`push` may move it away), then `recv` runs the receiver.  An empty chunk goes through like any other.
template <class T, class Len, class Push, class Recv> static void pump(std::ifstream& in, size_t unit, Len len, Push push, Recv recv)
{
    for (std::vector<T> chunk;;) {
        chunk.resize(len());
        if (!(in.read(reinterpret_cast<char*>(chunk.data()), (std::streamsize)(chunk.size() * sizeof(T))) || in.gcount() > 0)) break;
        chunk.resize((size_t)in.gcount() / (unit * sizeof(T)) * unit);
        push(chunk);
        recv();
    }
}

// chunks of In -> `front` -> 240 ksps IQ chunks of Sample -> DemodTask -> the receiver
template <class Sample, class In, class Len, class Front, class Recv>
static void demodulate(Handle& h, std::ifstream& in, Hub& hub, Chan<Baseband>& chan, size_t unit, Len len, Front front, Recv recv)
{
    Chan<std::vector<Sample>> reader;
    DemodTask<Chan<std::vector<Sample>>, Hub, Chan<Baseband>, Sample> demod(h, reader, hub, chan);
    pump<In>(in, unit, len, [&](std::vector<In>& chunk) { reader.send(front(chunk)); demod.run(); }, recv);
}

// -a MS: the frequency measure (docs/SPEC.md 3.0f, the recommended prefilter) runs on the tuned row while the first MS ms of the
// capture go by; then the channel's step is corrected ONCE, without a phase jump (3.0e), and the stream carries on
class Afc {                                                           // (span: input samples to measure; cap240: the most tuned samples of one chunk)
    static constexpr int32_t D = 10, T = 240;
    static constexpr size_t KEEP = (size_t)(T - 1 + D);
    size_t left_;                                                     // input samples still to measure (-A: up to the next boundary)
    size_t window_ = 0;                                               // -A: input samples between two updates (0: -a)
    FreqMeasure measure_;
    Track loop_;                                                      // -A
    HipMem d_row_, d_acc_;
    std::vector<float> row_;                                          // [history | the chunk's tuned samples], as it goes to the device
    float* row() const { return static_cast<float*>(d_row_.p); }
    p25fe_afc_acc_t* acc() const { return static_cast<p25fe_afc_acc_t*>(d_acc_.p); }
public:
    Afc(Handle& h, size_t span, size_t cap240) : left_(span), d_row_((KEEP + cap240) * 2 * sizeof(float), false), d_acc_(sizeof(p25fe_afc_acc_t), false)
    {
        std::vector<float> g((size_t)T);
        expect(p25fe_afc_design(D, 7000.0, T, g.data(), g.size()), "unable to design the measure's prefilter");
        measure_ = FreqMeasure(h, D, T, g.data(), 1);
        const p25fe_afc_acc_t zero = {0, 0, 0, 0};
        if (!row() || !acc() || hipMemcpy(acc(), &zero, sizeof zero, hipMemcpyHostToDevice) != hipSuccess)
            fail("p25fe_replay: no device memory for the frequency measure\n");
    }
    // -A: the recommended loop of SPEC 3.0g over tn, updated every `span` input samples; a pull or a deviation of at most 6.25 kHz
    void track(const Tuner& tn, uint32_t rate_hz)
    {
        window_ = left_;
        int32_t half_channel = 1 << 24;
        (void)p25fe_nco_step(rate_hz, 6250.0, &half_channel);
        const uint64_t half_window = (uint64_t)((double)window_ * 240000.0 / (double)rate_hz) / (uint64_t)D / 2;
        const p25fe_track_cfg_t cfg = {24, 24576, 65536, std::max(half_channel, 1), std::max(half_channel, 1), 0, std::max<uint64_t>(half_window, 1)};
        loop_ = Track(tn, measure_, cfg);
    }
    bool tracking() const { return window_ != 0; }
    bool over() const { return left_ == 0; }
    size_t chunk(size_t n_chunk) const { return left_ ? std::min(n_chunk, left_) : n_chunk; }   // input samples of the next read
    // one chunk: its n_in input samples (short_read: the capture ended in it) gave the tuned samples x240, the first at pos240
    void feed(const std::vector<float>& x240, uint64_t pos240, size_t n_in, bool short_read)
    {
        row_.erase(row_.begin(), row_.end() - (long)(2 * std::min(KEEP, row_.size() / 2)));     // the last KEEP tuned samples (fewer at the start)
        const size_t nh = row_.size() / 2;
        row_.insert(row_.end(), x240.begin(), x240.end());
        if (hipMemcpy(row(), row_.data(), row_.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            fail("p25fe_replay: unable to copy the tuned row to the device\n");
        if (tracking()) {
            expect(p25fe_track_measure_dev(loop_.get(), row() + 2 * nh, 0, nh, x240.size() / 2, pos240, nullptr), "unable to measure the frequency");
            left_ -= n_in;                                            // (a trailing partial window is measured and not updated)
            return;
        }
        expect(p25fe_afc_measure_dev(measure_.get(), row() + 2 * nh, 0, nh, x240.size() / 2, pos240, 24, acc(), nullptr), "unable to measure the frequency");
        left_ = short_read ? 0 : left_ - n_in;                        // (a capture shorter than MS ms: what there is)
    }
    // -A, a boundary: the window's record (for the report), the update on the device at input sample `at`, and the state it left
    void update(uint64_t at, FILE* js)
    {
        static const char* const names[] = {"none", "short", "reject", "apply"};
        p25fe_afc_acc_t a;
        p25fe_track_state_t st;
        double hz = 0.0, coherence = 0.0;
        expect(p25fe_track_records(loop_.get(), &a, nullptr), "unable to read the frequency measure");
        expect(p25fe_afc_hz(&a, D, &hz, &coherence), "unable to evaluate the frequency measure");
        expect(p25fe_track_update_dev(loop_.get(), at, nullptr), "unable to update the loop");
        expect(p25fe_track_read(loop_.get(), &st), "unable to read the loop's state");
        const char* status = names[st.status & 3u];
        std::fprintf(stderr, "p25fe_replay: afc: %.1f Hz off (coherence %.3f, %" PRIu64 " products): %s; step %d at sample %" PRIu64 "\n",
                     hz, coherence, a.n, status, st.step, at);
        if (js)
            std::fprintf(js, "{\"event\":\"afc\",\"hz\":%.3f,\"coherence\":%.6f,\"products\":%" PRIu64 ",\"step\":%d,\"at\":%" PRIu64 ",\"status\":\"%s\"}\n",
                         hz, coherence, a.n, st.step, at, status);
        left_ = window_;
    }
    // the span is over: the estimate, reported on stderr and in the -j events, and the one correction from input sample `at` on
    int32_t correct(const Tuner& tn, uint32_t rate_hz, int32_t step, uint64_t at, FILE* js) const
    {
        p25fe_afc_acc_t a;
        if (hipMemcpy(&a, acc(), sizeof a, hipMemcpyDeviceToHost) != hipSuccess) fail("p25fe_replay: unable to read the frequency measure\n");
        double hz = 0.0, coherence = 0.0;
        int32_t dstep = 0;
        expect(p25fe_afc_hz(&a, D, &hz, &coherence), "unable to evaluate the frequency measure");
        expect(p25fe_nco_step(rate_hz, hz, &dstep), "unable to turn the estimate into a step");
        const int32_t new_step = (int32_t)((uint32_t)step + (uint32_t)dstep);
        expect(p25fe_afc_set_step(tn.get(), 0, new_step, at, nullptr), "unable to retune");
        std::fprintf(stderr, "p25fe_replay: afc: %.1f Hz off (coherence %.3f, %" PRIu64 " products); step %d -> %d at sample %" PRIu64 "\n",
                     hz, coherence, a.n, step, new_step, at);
        if (js)
            std::fprintf(js, "{\"event\":\"afc\",\"hz\":%.3f,\"coherence\":%.6f,\"products\":%" PRIu64 ",\"step\":%d,\"at\":%" PRIu64 "}\n",
                         hz, coherence, a.n, new_step, at);
        return new_step;
    }
};

// -r: what sits in front of the cf32 DemodTask when the capture is not at 240 ksps -- the resampler (docs/SPEC.md 3.0b), or the tuner
// with a rational (-f, 3.0c) or an NCO channel (-F, 3.0d) and the optional AFC (-a).  A raw chunk in, its 240 ksps cf32 samples out.
class ToChannelRate {
    const Options& o_;
    FILE* js_;
    Resampler rs_;                                                    // -r alone
    Tuner tn_;                                                        // -r with -f or -F
    std::optional<Afc> afc_;
    int32_t step_ = 0;                                                // the NCO channel's
    size_t n_chunk_ = 0, cap240_ = 0;                                 // input samples per chunk; the most 240 ksps samples one gives
    uint64_t consumed_ = 0, pos240_ = 0;
public:
    ToChannelRate(Handle& h, const Options& o, FILE* js) : o_(o), js_(js)
    {
        int32_t L = 0, M = 0, T = 0, num = 0, den = 0;
        const uint32_t rate = (uint32_t)o.rate_hz;
        if (p25fe_resampler_design(rate, &L, &M, &T, nullptr, 0) != P25FE_ERR_CAPACITY)
            fail("no resampler for %lu Hz (240000 / rate in lowest terms must be L / M with L <= %d, L < M <= %d)\n", o.rate_hz, P25FE_RS_MAX_L, P25FE_RS_MAX_M);
        std::vector<float> taps((size_t)L * (size_t)T);
        expect(p25fe_resampler_design(rate, &L, &M, &T, taps.data(), taps.size()), "unable to design the resampler");
        if (o.offset.kind == o.offset.NONE) rs_ = Resampler(h, L, M, T, taps.data());
        else if (o.offset.kind == o.offset.NCO) {
            if (p25fe_nco_step(rate, o.offset.nco_hz, &step_) != P25FE_OK) fail("no tuner for %g Hz at %lu Hz (beyond half the rate)\n", o.offset.nco_hz, o.rate_hz);
            tn_ = Tuner::nco(h, L, M, T, taps.data(), 1, &step_);
        } else {
            if (p25fe_tuner_freq(rate, o.offset.hz, &num, &den) != P25FE_OK)
                fail("no tuner for %lld Hz at %lu Hz (beyond half the rate, or offset / rate in lowest terms has a denominator above %d)\n",
                     o.offset.hz, o.rate_hz, P25FE_TUNE_MAX_DEN);
            tn_ = Tuner::rational(h, L, M, T, taps.data(), 1, &num, &den);
        }
        n_chunk_ = (size_t)BUF_SAMPLES * o.batch * (size_t)M / (size_t)L;       // about one cf32-mode chunk of 240 ksps samples
        cap240_ = n_chunk_ * (size_t)L / (size_t)M + 2;
        if (o.afc_ms > 0.0) afc_.emplace(h, std::max<size_t>(1, (size_t)((double)o.rate_hz * o.afc_ms / 1000.0)), cap240_);
        if (o.track_ms > 0.0) {
            afc_.emplace(h, std::max<size_t>(1, (size_t)((double)o.rate_hz * o.track_ms / 1000.0)), cap240_);
            afc_->track(tn_, rate);
        }
    }
    size_t next_bytes() const { return (afc_ ? afc_->chunk(n_chunk_) : n_chunk_) * o_.bps; }
    std::vector<float> operator()(const std::vector<char>& raw)       // tune, measure, maybe retune
    {
        const size_t n = raw.size() / o_.bps;
        const bool short_read = raw.size() < next_bytes();
        std::vector<float> x240(2 * cap240_);
        size_t n240 = 0;
        if (tn_.get()) expect(p25fe_tune(tn_.get(), raw.data(), o_.fmt, n, x240.data(), cap240_, &n240), "unable to tune");
        else expect(p25fe_resample(rs_.get(), raw.data(), o_.fmt, n, x240.data(), cap240_, &n240), "unable to resample");
        x240.resize(2 * n240);
        consumed_ += n;
        if (afc_ && afc_->tracking()) {
            afc_->feed(x240, pos240_, n, short_read);
            if (afc_->over()) afc_->update(consumed_, js_);
        } else if (afc_ && !afc_->over()) {
            afc_->feed(x240, pos240_, n, short_read);
            if (afc_->over()) step_ = afc_->correct(tn_, (uint32_t)o_.rate_hz, step_, consumed_, js_);
        }
        pos240_ += n240;
        return x240;
    }
};

// -S MS: the survey (docs/SPEC.md 3.0h) of the first MS ms of the capture with N = 4096, hop 2048, the designed window and shift 16
// -> the {"event":"scan"} line with the active channels of the 12.5 kHz raster, strongest first.  The input is back at its start.
static std::string survey(Handle& h, const Options& o, std::ifstream& in)
{
    constexpr int32_t N = 4096;
    p25fe_scan_t* made = nullptr;
    expect(p25fe_scan_create(h.get(), N, N / 2, nullptr, 16, &made), "unable to make the survey");
    const std::unique_ptr<p25fe_scan_t, void (*)(p25fe_scan_t*)> sc(made, p25fe_scan_destroy);
    size_t left = std::max<size_t>(1, (size_t)((double)o.rate_hz * o.scan_ms / 1000.0));
    for (std::vector<char> chunk; left;) {
        const size_t want = std::min(left, (size_t)1 << 22);
        chunk.resize(want * o.bps);
        in.read(chunk.data(), (std::streamsize)chunk.size());
        const size_t got = (size_t)in.gcount() / o.bps;
        if (got) expect(p25fe_scan(sc.get(), chunk.data(), o.fmt, got), "unable to survey the capture");
        left -= got;
        if (got < want) break;                                        // (a capture shorter than MS ms: what there is)
    }
    in.clear();
    in.seekg(0);
    std::vector<uint64_t> acc((size_t)N + 1);
    expect(p25fe_scan_read(sc.get(), acc.data(), 0), "unable to read the survey");
    std::vector<p25fe_scan_chan_t> ch(256);
    size_t n = 0;
    expect(p25fe_scan_channels(acc.data(), N, (uint32_t)o.rate_hz, 12500.0, 4000.0, 20.0, ch.data(), ch.size(), &n), "unable to list the channels");
    char buf[160];
    std::snprintf(buf, sizeof buf, "{\"event\":\"scan\",\"n_frames\":%" PRIu64 ",\"channels\":[", acc[(size_t)N]);
    std::string line = buf;
    for (size_t i = 0; i < std::min(n, ch.size()); ++i) {
        const double db = ch[i].db_over_floor < 999.0 ? ch[i].db_over_floor : 999.0;              // (JSON has no infinity)
        std::snprintf(buf, sizeof buf, "%s{\"raster_index\":%d,\"centre_hz\":%.1f,\"db_over_floor\":%.2f,\"offset_hz\":%.1f}", i ? "," : "",
                      ch[i].raster_index, ch[i].centre_hz, db, ch[i].offset_hz);
        line += buf;
    }
    return line + "]}";
}

// -T MS: the survey over time (docs/SPEC.md 3.0i) of the whole input in slots of about MS ms (a whole number of frames of N = 4096 at
// hop 2048, the designed window, shift 16; at most 65 536 slots, then "truncated") -> the {"event":"activity"} line with the keyed
// intervals of the 12.5 kHz raster at 20 / 14 dB, at least two slots long, by first slot
static std::string activity(Handle& h, const Options& o, std::ifstream& in)
{
    constexpr int32_t N = 4096, H = N / 2;
    constexpr size_t MAX_SLOTS = 65536;
    const uint32_t B = (uint32_t)activity_slot_frames(o);
    p25fe_scan_t* made = nullptr;
    expect(p25fe_scan_create(h.get(), N, H, nullptr, 16, &made), "unable to make the survey");
    const std::unique_ptr<p25fe_scan_t, void (*)(p25fe_scan_t*)> sc(made, p25fe_scan_destroy);
    expect(p25fe_waterfall_open(sc.get(), B, MAX_SLOTS), "unable to open the rows");
    uint64_t left = (uint64_t)MAX_SLOTS * B * (uint64_t)H;           // samples whose frames all have a row
    bool truncated = false;
    for (std::vector<char> chunk;;) {
        const size_t want = (size_t)std::min<uint64_t>(left, (uint64_t)1 << 22);
        chunk.resize(std::max<size_t>(want, 1) * o.bps);
        in.read(chunk.data(), (std::streamsize)chunk.size());
        const size_t got = (size_t)in.gcount() / o.bps;
        if (want == 0) { truncated = got != 0; break; }              // every row is in use: is there more input?
        if (got) expect(p25fe_waterfall(sc.get(), chunk.data(), o.fmt, got), "unable to survey the capture");
        left -= got;
        if (got < want) break;
    }
    size_t n_rows = 0;
    (void)p25fe_waterfall_read(sc.get(), nullptr, 0, &n_rows);       // (P25FE_ERR_CAPACITY with the count)
    std::vector<uint64_t> rows(std::max<size_t>(n_rows, 1) * ((size_t)N + 1));
    expect(p25fe_waterfall_read(sc.get(), rows.data(), n_rows, &n_rows), "unable to read the rows");
    std::vector<p25fe_waterfall_key_t> key(256);
    size_t n = 0;
    for (int pass = 0; pass < 2; ++pass) {                            // (the count is whole even beyond the capacity: once more with room for all)
        expect(p25fe_waterfall_keys(rows.data(), n_rows, (size_t)N + 1, N, (uint32_t)o.rate_hz, 0, 12500.0, 4000.0, 20.0, 14.0, 2, key.data(),
                                    key.size(), &n), "unable to list the keyed intervals");
        if (n <= key.size()) break;
        key.resize(n);
    }
    const double slot_ms = (double)B * (double)H * 1000.0 / (double)o.rate_hz;
    char buf[256];
    std::snprintf(buf, sizeof buf, "{\"event\":\"activity\",\"slot_frames\":%u,\"slot_ms\":%.4f,\"n_slots\":%zu,%s\"keys\":[", B, slot_ms, n_rows,
                  truncated ? "\"truncated\":true," : "");
    std::string line = buf;
    for (size_t i = 0; i < n; ++i) {
        const double db = key[i].peak_db_over_floor < 999.0 ? key[i].peak_db_over_floor : 999.0;   // (JSON has no infinity)
        std::snprintf(buf, sizeof buf, "%s{\"raster_index\":%d,\"centre_hz\":%.1f,\"offset_hz\":%.1f,\"first_ms\":%.3f,\"last_ms\":%.3f,\"db_over_floor\":%.2f}",
                      i ? "," : "", key[i].raster_index, key[i].centre_hz, key[i].offset_hz, (double)key[i].first_slot * slot_ms,
                      (double)(key[i].first_slot + key[i].n_slots) * slot_ms, db);
        line += buf;
    }
    return line + "]}";
}

int main(int argc, char** argv)
try {
    Options o;
    if (!parse(argc, argv, o)) return usage(argv[0]);
    std::ifstream in(o.in_path, std::ios::binary);
    if (!in) fail("unable to open %s\n", o.in_path);
    Handle h(0, 1);
    if (o.window_bytes) return bulk(h, o, in);
    if (o.activity_ms > 0.0) {                                        // the survey over time alone: no output file
        std::printf("%s\n", activity(h, o, in).c_str());
        return 0;
    }
    std::string scan_event;
    if (o.scan_ms > 0.0) {
        scan_event = survey(h, o, in);
        std::printf("%s\n", scan_event.c_str());
        std::fflush(stdout);
        if (o.offset.kind == o.offset.NONE) return 0;                 // a survey alone
    }
    Hub hub;
    Chan<Baseband> chan;
    Sink sink;
    sink.out.open(o.out_path, std::ios::binary);
    sink.keep = o.jpath != nullptr;
    if (o.jpath && !(hub.js = std::fopen(o.jpath, "w"))) fail("unable to open %s\n", o.jpath);
    if (hub.js && !scan_event.empty()) std::fprintf(hub.js, "%s\n", scan_event.c_str());
    std::ofstream bbfile;                                             // samples_file, src/main.rs:174-175
    if (o.wpath) bbfile.open(o.wpath, std::ios::binary);
    if (o.wpath && !bbfile) fail("unable to open baseband file\n");
    RecvTask<Chan<Baseband>, Sink> recv(h, chan, sink);
    const auto receive = [&] {
        recv.run([&](const std::vector<float>& s) {                   // the closure of src/main.rs:278-283
            if (o.wpath) bbfile.write(reinterpret_cast<const char*>(s.data()), (std::streamsize)(s.size() * sizeof(float)));
        }, hub);
    };
    const auto len240k = [&] { return 2 * BUF_SAMPLES * o.batch; };  // BUF_SAMPLES * batch samples per chunk, whatever the format
    const auto take = [](auto& chunk) { return std::move(chunk); };   // straight into the reader channel
    if (o.rate_hz) {
        ToChannelRate front(h, o, hub.js);
        demodulate<float, char>(h, in, hub, chan, o.bps, [&] { return front.next_bytes(); }, [&](std::vector<char>& raw) { return front(raw); }, receive);
    } else if (o.bb)                                                  // replay.rs reads 32768-byte blocks (src/replay.rs:27); only the bytes
        pump<float>(in, 1, [&] { return 8192 * o.batch; },            // actually read go on (replay.rs:36 re-feeds the stale tail)
                    [&](std::vector<float>& chunk) { chan.send(Baseband{std::move(chunk)}); }, receive);
    else if (o.fmt == P25FE_FMT_U8) demodulate<uint8_t, uint8_t>(h, in, hub, chan, 2, len240k, take, receive);
    else if (o.fmt == P25FE_FMT_S16) demodulate<int16_t, int16_t>(h, in, hub, chan, 2, len240k, take, receive);
    else demodulate<float, float>(h, in, hub, chan, 2, len240k, take, receive);

    if (hub.js) {
        // network identifiers of all frame syncs in one pass over the finished dibit stream, then the stats row
        std::vector<p25fe_nid_t> nid(sink.sync_pos.size());
        expect(p25fe_nid(h.get(), sink.all_dibits.data(), sink.all_dibits.size(), sink.sync_dibit.data(), sink.sync_pos.data(), nid.size(), nid.data()),
               "unable to decode network identifiers");
        uint64_t words = 0, errs = 0, fixed = 0;
        for (const p25fe_nid_t& r : nid) {
            std::fprintf(hub.js, "{\"event\":\"nid\",\"sync_pos\":%" PRId64 ",\"nac\":%u,\"duid\":%u,\"errors\":%u,\"valid\":%d}\n",
                         r.sync_pos, (unsigned)r.nac, (unsigned)r.duid, (unsigned)r.n_errors, (int)r.valid);
            if (r.valid >= 0) { ++words; if (r.valid == 0) ++errs; else fixed += r.n_errors; }
        }
        // serialize_code_stats (src/hub.rs:574-581): totalWords, errWords, totalSymbols = words * size, fixedSymbols
        std::fprintf(hub.js, "{\"event\":\"updateStats\",\"dibits\":%zu,\"syncs\":%zu,\"bch\":{\"totalWords\":%" PRIu64 ",\"errWords\":%" PRIu64
                             ",\"totalSymbols\":%" PRIu64 ",\"fixedSymbols\":%" PRIu64 "}}\n", sink.n_dibits, sink.n_sync, words, errs, words * 63, fixed);
    }
    std::fprintf(stderr, "p25fe_replay: %zu dibits, %zu frame syncs, %zu power reports\n", sink.n_dibits, sink.n_sync, hub.n_power);
    return 0;
} catch (const Exit& e) { return e.status; }
