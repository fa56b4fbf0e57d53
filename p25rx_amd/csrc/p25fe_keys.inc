// p25fe_keys.inc -- survey over time, keys on the device: p25fe_waterfall_keys' rule applied where the rows are (docs/SPEC.md 3.0k;
// kernels: k_keys_pow, k_keys_walk, k_keys_cell), device and host side.  Included by p25fe_api.hip behind p25fe_cuts.inc; never
// embedded for hipRTC.
//
// The host function is the definition and the three kernels return its bytes.  What makes that so: every sum is taken in the host's
// order, one rounded operation at a time (-ffp-contract=off); the floor is a selection, not arithmetic; the comparisons have the
// host's shapes, so a NaN threshold fails where it fails there; and the two things the device does not evaluate -- the centroid's
// quotient and log10 -- are left to p25fe_keys_read, which uses the host function's expressions on the device's sums.
//
//   k_keys_pow   one workgroup per row: pow[t][c] into LDS and scratch, a bitonic sort of the C bit patterns in LDS (non-negative
//                doubles order as their words do), the lower median to scratch; a row of zero frames is marked by a floor of -1
//   k_keys_walk  one lane per channel: the two-state rule over the rows, 16 rows' loads in flight; an interval that ends and is
//                long enough takes the next raw record through one counter, which counts every interval
//   k_keys_cell  one wave per interval: the cell's bins of the interval's rows, 64 at a time in the host's order, each lane forming
//                v and v * f_b, all of them added in order out of LDS
#ifndef P25FE_KEYS_INC
#define P25FE_KEYS_INC

namespace p25k {

constexpr int KY_WG = 256;                 // k_keys_pow's workgroup
constexpr int KY_MAX_C = 4096;             // P25FE_KEYS_MAX_CHANNELS: the sort's LDS, 8 bytes a channel
constexpr int KY_AHEAD = 16;               // rows k_keys_walk loads before it looks at the first of them

// a channel's bins: runs in signed-frequency order, k0 the signed index of the first (bin k + N for k < 0)
struct KeyChan { int bw0, bw_n, cell0, cell_n; };
// what the device knows of an interval: rows [first, first + n) of channel `chan`, the cell's sums and the largest p / floor
struct KeyRaw { unsigned chan, first, n, pad; double s, sf, q; };

struct KeysArgs {
    const unsigned long long* rows;        // [n_rows][stride], read only
    long stride;
    int n_rows, N, C, P;                   // P: the power of two the sort runs over, >= max(C, 2)
    const KeyChan* chan;                   // [C]
    const double* fb;                      // [N]
    double* pw;                            // scratch [n_rows][C + 1]: the powers and, in word C, the floor (-1: no frame)
    double on, off;
    unsigned min_slots, max_keys;
    KeyRaw* raw;                           // [max_keys]
    unsigned* count;                       // every interval, also those beyond max_keys
};

__device__ __forceinline__ int ky_bin(int k, int N) { return k < 0 ? k + N : k; }

__global__ __launch_bounds__(KY_WG) void k_keys_pow(KeysArgs a)
{
    __shared__ unsigned long long srt[KY_MAX_C];
    const int tid = threadIdx.x;
    const unsigned long long* row = a.rows + (long)blockIdx.x * a.stride;
    double* out = a.pw + (long)blockIdx.x * (a.C + 1);
    if (row[a.N] == 0) {                                            // uniform: no frame, nothing else of the row is looked at
        if (tid == 0) out[a.C] = -1.0;
        return;
    }
    for (int c = tid; c < a.P; c += KY_WG) {
        unsigned long long bits = ~0ull;                            // the padding sorts behind every power
        if (c < a.C) {
            const KeyChan ch = a.chan[c];
            double p = 0.0;
            for (int j = 0; j < ch.bw_n; ++j) p += (double)row[ky_bin(ch.bw0 + j, a.N)];
            out[c] = p;
            bits = (unsigned long long)__double_as_longlong(p);
        }
        srt[c] = bits;
    }
    __syncthreads();
    for (int k = 2; k <= a.P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < a.P / 2; i += KY_WG) {
                const int lo = 2 * (i & ~(j - 1)) + (i & (j - 1)), hi = lo + j;   // (j is a power of two)
                const unsigned long long x = srt[lo], y = srt[hi];
                if ((x > y) == ((lo & k) == 0)) { srt[lo] = y; srt[hi] = x; }
            }
            __syncthreads();
        }
    }
    if (tid == 0) out[a.C] = __longlong_as_double((long long)srt[(a.C - 1) / 2]);   // the lower median
}

__global__ __launch_bounds__(64) void k_keys_walk(KeysArgs a)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.C) return;
    const long W = a.C + 1;
    bool live = false;
    int first = 0;
    double q = 0.0;
    const auto close = [&](int end) {                               // the interval ends in front of row `end`
        if (live && (unsigned)(end - first) >= a.min_slots) {
            const unsigned at = atomicAdd(a.count, 1u);
            if (at < a.max_keys) {
                KeyRaw r;
                r.chan = (unsigned)c; r.first = (unsigned)first; r.n = (unsigned)(end - first); r.pad = 0u;
                r.s = 0.0; r.sf = 0.0; r.q = q;
                a.raw[at] = r;
            }
        }
        live = false;
    };
    for (int t0 = 0; t0 < a.n_rows; t0 += KY_AHEAD) {
        double p[KY_AHEAD], f[KY_AHEAD];
#pragma unroll
        for (int u = 0; u < KY_AHEAD; ++u) {                        // the loads do not depend on the state: all of them first
            const bool in = t0 + u < a.n_rows;
            const double* at = a.pw + (long)(in ? t0 + u : t0) * W;
            p[u] = at[c]; f[u] = at[a.C];
        }
#pragma unroll
        for (int u = 0; u < KY_AHEAD; ++u) {
            const int t = t0 + u;
            if (t >= a.n_rows) break;
            const double flr = f[u], pc = p[u];
            if (flr < 0.0) { close(t); continue; }                  // no frame: every open interval ends (p was never written)
            if (live && !(pc >= flr * a.off)) close(t);
            if (!live && pc > 0.0 && pc >= flr * a.on) { live = true; first = t; q = 0.0; }
            if (live) {
                const double r = flr > 0.0 ? pc / flr : HUGE_VAL;
                if (r > q) q = r;
            }
        }
    }
    close(a.n_rows);
}

__global__ __launch_bounds__(64) void k_keys_cell(KeysArgs a)
{
    __shared__ double2 buf[2][64];
    const int lane = threadIdx.x;
    const unsigned total = min(*a.count, a.max_keys);
    int turn = 0;
    for (unsigned i = blockIdx.x; i < total; i += gridDim.x) {      // (uniform: the workgroup is one wave)
        const KeyRaw r = a.raw[i];
        const KeyChan ch = a.chan[r.chan];
        const unsigned long long E = (unsigned long long)r.n * (unsigned)ch.cell_n;   // the interval's bins, row by row
        double s = 0.0, sf = 0.0;
        for (unsigned long long e0 = 0; e0 < E; e0 += 64, turn ^= 1) {
            const unsigned long long e = e0 + (unsigned)lane;
            double2 vm = make_double2(0.0, 0.0);
            if (e < E) {
                const unsigned t = r.first + (unsigned)(e / (unsigned)ch.cell_n);
                const int b = ky_bin(ch.cell0 + (int)(e % (unsigned)ch.cell_n), a.N);
                vm.x = (double)a.rows[(long)t * a.stride + b];
                vm.y = vm.x * a.fb[b];
            }
            buf[turn][lane] = vm;
            __syncthreads();                                        // the other buffer was read in front of this barrier
            const int cnt = (int)min((unsigned long long)64, E - e0);
            for (int j = 0; j < cnt; ++j) { const double2 x = buf[turn][j]; s += x.x; sf += x.y; }
        }
        if (lane == 0) { a.raw[i].s = s; a.raw[i].sf = sf; }
    }
}

}  // namespace p25k

// The plan of one raster over one survey object's N, on its device: the channels' bin runs and the bin frequencies uploaded once, all
// scratch allocated.  A run leaves the raw records and their count on the device; p25fe_keys_read finishes them.
struct p25fe_keys {
    p25fe_scanner* sc = nullptr;           // used by every run (its handle, device and open rows), never by the destructor
    int device = 0;
    int N = 0, P = 2;
    std::vector<int32_t> r;                // per channel: the raster index ...
    std::vector<double> fc;                // ... and the centre
    double on = 0.0, off = 0.0;
    uint32_t min_slots = 0;
    size_t max_rows = 0, max_keys = 0;
    DevBuf d_chan, d_fb, d_pw, d_raw, d_count;
    hipEvent_t done = nullptr;             // recorded behind the last run
    bool ran = false;
    uint64_t slot0 = 0;                    // the last run's
    ~p25fe_keys() { if (done) (void)hipEventDestroy(done); }
};

namespace {

static_assert(sizeof(KeyRaw) == 40 && sizeof(KeyChan) == 16 && KY_MAX_C == P25FE_KEYS_MAX_CHANNELS, "the records of p25fe_keys.inc");
constexpr size_t KY_MAX_KEYS = (size_t)1 << 20;
constexpr size_t KY_MAX_SCRATCH = (size_t)1 << 28;                  // words
constexpr unsigned KY_CELL_GRID = 2048;

// a channel's bins as a run: the signed index of the first and the count; false unless they are consecutive in signed order
bool ky_run(const std::vector<uint32_t>& bins, int N, int* k0, int* n)
{
    *k0 = 0; *n = (int)bins.size();
    for (size_t i = 0; i < bins.size(); ++i) {
        const int k = bins[i] < (uint32_t)(N / 2) ? (int)bins[i] : (int)bins[i] - N;
        if (i == 0) *k0 = k;
        else if (k != *k0 + (int)i) return false;
    }
    return true;
}

int ky_run_rows(p25fe_keys* kp, const uint64_t* d_rows, size_t n_rows, size_t row_stride, uint64_t slot0, hipStream_t st)
{
    p25fe_t* h = kp->sc->h;
    if (n_rows > kp->max_rows) return P25FE_ERR_CAPACITY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    KeysArgs a;
    a.rows = reinterpret_cast<const unsigned long long*>(d_rows);
    a.stride = (long)row_stride;
    a.n_rows = (int)n_rows; a.N = kp->N; a.C = (int)kp->r.size(); a.P = kp->P;
    a.chan = kp->d_chan.as<KeyChan>(); a.fb = kp->d_fb.as<double>(); a.pw = kp->d_pw.as<double>();
    a.on = kp->on; a.off = kp->off; a.min_slots = kp->min_slots; a.max_keys = (unsigned)kp->max_keys;
    a.raw = kp->d_raw.as<KeyRaw>(); a.count = kp->d_count.as<unsigned>();
    HIPCHK(h, hipMemsetAsync(kp->d_count.p, 0, sizeof(unsigned), st));
    kp->ran = true; kp->slot0 = slot0;
    if (a.C != 0 && n_rows != 0) {
        (void)hipGetLastError();                                    // the check below is for THESE launches
        hipLaunchKernelGGL(k_keys_pow, dim3((unsigned)n_rows), dim3(KY_WG), 0, st, a);
        hipLaunchKernelGGL(k_keys_walk, dim3((unsigned)((a.C + 63) / 64)), dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_keys_cell, dim3((unsigned)std::min<size_t>(kp->max_keys, KY_CELL_GRID)), dim3(64), 0, st, a);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipEventRecord(kp->done, st));
    return P25FE_OK;
}

}  // namespace

extern "C" {

int p25fe_keys_create(p25fe_scan_t* sc, uint32_t fs_hz, double raster_hz, double half_bw_hz, double on_db, double off_db,
                      uint32_t min_slots, size_t max_rows, size_t max_keys, p25fe_keys_t** out)
{
    if (out) *out = nullptr;
    if (!out || !sc || !sc->h || fs_hz == 0 || !finite_d(raster_hz) || !(raster_hz > 0.0) || !finite_d(half_bw_hz) ||
        half_bw_hz < 0.0 || !finite_d(on_db) || !finite_d(off_db) || off_db > on_db || min_slots == 0 || max_rows == 0 ||
        max_rows > WF_MAX_ROWS || max_keys == 0 || max_keys > KY_MAX_KEYS) return P25FE_ERR_ARG;
    ScRaster ra;
    if (int rc = ra.build(sc->N, (double)fs_hz, raster_hz, half_bw_hz)) return rc;
    const size_t C = ra.chan.size();
    if (C > (size_t)KY_MAX_C || max_rows * (C + 1) > KY_MAX_SCRATCH) return P25FE_ERR_CAPACITY;
    std::vector<KeyChan> chan(C);
    p25fe_keys* kp = new (std::nothrow) p25fe_keys;
    if (!kp) return P25FE_ERR_NOMEM;
    kp->sc = sc; kp->device = sc->device; kp->N = sc->N;
    kp->on = pow(10.0, on_db / 10.0); kp->off = pow(10.0, off_db / 10.0);
    kp->min_slots = min_slots; kp->max_rows = max_rows; kp->max_keys = max_keys;
    while ((size_t)kp->P < C) kp->P *= 2;
    kp->r.resize(C); kp->fc.resize(C);
    for (size_t c = 0; c < C; ++c) {
        kp->r[c] = ra.chan[c].r; kp->fc[c] = ra.chan[c].fc;
        if (!ky_run(ra.chan[c].in_bw, sc->N, &chan[c].bw0, &chan[c].bw_n) ||
            !ky_run(ra.chan[c].in_cell, sc->N, &chan[c].cell0, &chan[c].cell_n)) { delete kp; return P25FE_ERR_ARG; }
    }
    p25fe_t* h = sc->h;
    bool ok = hipSetDevice(kp->device) == hipSuccess && hipEventCreateWithFlags(&kp->done, hipEventDisableTiming) == hipSuccess &&
              kp->d_count.ensure(sizeof(unsigned)) == hipSuccess && kp->d_raw.ensure(max_keys * sizeof(KeyRaw)) == hipSuccess &&
              hipMemset(kp->d_count.p, 0, sizeof(unsigned)) == hipSuccess;
    if (ok && C != 0)
        ok = kp->d_chan.ensure(C * sizeof(KeyChan)) == hipSuccess && kp->d_fb.ensure(ra.fb.size() * sizeof(double)) == hipSuccess &&
             kp->d_pw.ensure(max_rows * (C + 1) * sizeof(double)) == hipSuccess &&
             hipMemcpy(kp->d_chan.p, chan.data(), C * sizeof(KeyChan), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(kp->d_fb.p, ra.fb.data(), ra.fb.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { h->last_hip = (int)hipGetLastError(); (void)hipSetDevice(kp->device); delete kp; return P25FE_ERR_HIP; }
    *out = kp;
    return P25FE_OK;
}

void p25fe_keys_destroy(p25fe_keys_t* kp) { rs_destroy(kp); }

int p25fe_keys_dev(p25fe_keys_t* kp, const uint64_t* d_rows, size_t n_rows, size_t row_stride, uint64_t slot0, void* stream)
{
    if (!kp || !kp->sc || !kp->sc->h || !d_rows || (reinterpret_cast<uintptr_t>(d_rows) & 7u) != 0 ||
        row_stride < (size_t)kp->N + 1 || row_stride >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    return ky_run_rows(kp, d_rows, n_rows, row_stride, slot0, (hipStream_t)stream);
}

int p25fe_keys_stream(p25fe_keys_t* kp)
{
    if (!kp || !kp->sc || !kp->sc->h || kp->sc->wf_B == 0) return P25FE_ERR_ARG;
    const p25fe_scanner* sc = kp->sc;
    // p25fe_waterfall_read's count: the rows touched so far, and never more than there are
    const size_t rows = (size_t)std::min<uint64_t>((sc->pos / (uint64_t)sc->H + sc->wf_B - 1) / sc->wf_B, sc->wf_rows);
    return ky_run_rows(kp, sc->d_rows.as<uint64_t>(), rows, (size_t)sc->N + 1, 0, sc->h->stream);
}

int p25fe_keys_read(p25fe_keys_t* kp, p25fe_waterfall_key_t* out, size_t cap, size_t* n_out)
{
    if (n_out) *n_out = 0;
    if (!kp || !kp->sc || !kp->sc->h || !n_out || (cap && !out)) return P25FE_ERR_ARG;
    if (!kp->ran) return P25FE_OK;
    p25fe_t* h = kp->sc->h;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipEventSynchronize(kp->done));
    unsigned count = 0;
    HIPCHK(h, hipMemcpy(&count, kp->d_count.p, sizeof count, hipMemcpyDeviceToHost));
    *n_out = count;
    if ((size_t)count > kp->max_keys) return P25FE_ERR_CAPACITY;    // the device emits in no order: there is no sorted prefix
    std::vector<KeyRaw> raw(count);
    if (count) HIPCHK(h, hipMemcpy(raw.data(), kp->d_raw.p, (size_t)count * sizeof(KeyRaw), hipMemcpyDeviceToHost));
    std::vector<p25fe_waterfall_key_t> keys(count);
    for (size_t i = 0; i < raw.size(); ++i) {                       // the host function's expressions on the device's sums
        const KeyRaw& w = raw[i];
        const double fc = kp->fc[w.chan];
        p25fe_waterfall_key_t& k = keys[i];
        k.raster_index = kp->r[w.chan]; k.reserved = 0;
        k.first_slot = kp->slot0 + w.first; k.n_slots = w.n;
        k.centre_hz = fc;
        k.offset_hz = w.s > 0.0 ? w.sf / w.s - fc : 0.0;
        k.peak_db_over_floor = 10.0 * log10(w.q);
    }
    std::sort(keys.begin(), keys.end(), [](const p25fe_waterfall_key_t& x, const p25fe_waterfall_key_t& y) {
        return x.first_slot != y.first_slot ? x.first_slot < y.first_slot : x.raster_index < y.raster_index;   // (the pair is unique)
    });
    for (size_t i = 0; i < keys.size() && i < cap; ++i) out[i] = keys[i];
    return P25FE_OK;
}

}  // extern "C"

#endif  /* P25FE_KEYS_INC */
