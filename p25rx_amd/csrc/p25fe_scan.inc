// p25fe_scan.inc -- survey: power spectrum of a capture (docs/SPEC.md 3.0h; kernel: k_scan), device and host side.
// Included by p25fe_api.hip at file scope, behind its last extern "C" block; never embedded for hipRTC (the Makefile's embed list
// does not name it): the kernel takes the handle's conversion numbers as arguments and is never specialised.
//
// K0d, k_scan<FMT, LUTM, N>: a Welch periodogram.  One workgroup of 256 lanes takes F consecutive frames of one capture row.  Its
// strip of (F - 1) H + N samples is read ONCE, hop by hop, with the 16-byte vector loaders of K0 / K0b (wide_sample: one body, three
// formats), converted to cf32 and kept in an LDS ring of N samples; the hop of the next frame is fetched into registers under the
// current frame's first pass.  The length-N DFT is a Stockham autosort of radix R = N / 256 (16 for N = 4096: three passes;
// 4 for N = 1024: five passes): lane j reads positions j + 256 r of the previous pass (conflict-free), multiplies by its twiddles,
// does one radix-R butterfly in registers and writes to (j / Ns) Ns R + j % Ns + r Ns; only these transposes go through LDS, with a
// pad of one entry per 16 against the power-of-two strides.  After the last pass lane j holds bins j + 256 r in natural order: it
// quantises their powers and keeps R 64-bit sums in registers across the F frames, then issues ONE 64-bit integer atomic add per bin
// (and lane 0 one for the frame count).  The window and the twiddles (from the table p25fe_scan_create made in double) do not depend
// on the frame.  Radix 4 holds them in registers.  Radix 16 cannot at two workgroups per CU (256 registers a lane): pass 1's 240
// distinct twiddle pairs sit in LDS, the last pass's 15 pairs a lane and the 16 window values are read per frame from the tables,
// which L2 serves.  A frame's arithmetic is one fixed sequence of operations on its N converted samples: the values do not depend
// on the workgroup or on the frame's place in its batch.  The body is sc_frames, which k_waterfall (p25fe_waterfall.inc, SPEC 3.0i)
// shares: there the sums go into one row per slot of B frames instead.
#ifndef P25FE_SCAN_INC
#define P25FE_SCAN_INC

namespace p25k {

constexpr int SC_WG = 256;                                          // lanes per workgroup: four waves, one per SIMD
constexpr int sc_radix(int N) { return N == 4096 ? 16 : 4; }
constexpr int sc_passes(int N) { return N == 4096 ? 3 : 5; }
__host__ __device__ constexpr int sc_pad(int i) { return i + (i >> 4); }   // LDS position of entry i of a ring / transpose buffer

struct SurveyArgs {
    const void* x;          // owned sample 0, 16-B aligned
    long n_hist, n_new;
    long e0;                // last sample of the first owned frame, relative to owned sample 0 (0 .. H - 1)
    long n_frames;          // frames the range owns
    int H, F;               // hop; frames per workgroup
    float scale;            // 2^shift
    const float* win;       // device, N floats
    const float2* tw;       // device, N pairs: e^{-2 pi i m / N}
    unsigned long long* acc;   // [N + 1]
};

__device__ __forceinline__ float2 sc_cmul(float2 a, float2 b)
{
    return make_float2(__builtin_fmaf(-a.y, b.y, a.x * b.x), __builtin_fmaf(a.y, b.x, a.x * b.y));
}
// forward 4-point DFT in place, outputs in natural order
__device__ __forceinline__ void sc_dft4(float2& a0, float2& a1, float2& a2, float2& a3)
{
    const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
    a0 = make_float2(s02.x + s13.x, s02.y + s13.y);
    a2 = make_float2(s02.x - s13.x, s02.y - s13.y);
    a1 = make_float2(d02.x + d13.y, d02.y - d13.x);                 // d02 - i d13
    a3 = make_float2(d02.x - d13.y, d02.y + d13.x);                 // d02 + i d13
}
// e^{-2 pi i k / 16} for k = 0 .. 9 (the products a c of the 4 x 4 factoring), correctly rounded
__device__ constexpr float SC_W16_C[10] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f,
                                           -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f, -1.0f, -0.92387953251128674f};
__device__ constexpr float SC_W16_S[10] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f, 1.0f,
                                           0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f, -0.38268343236508977f};
// forward R-point DFT of v in place, natural order (R = 16: input n = a + 4 b, output k = c + 4 d)
template <int R>
__device__ __forceinline__ void sc_dft(float2 (&v)[R])
{
    static_assert(R == 4 || R == 16, "radix 4 or 16");
    if constexpr (R == 4) {
        sc_dft4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) sc_dft4(v[a], v[a + 4], v[a + 8], v[a + 12]);      // v[a + 4 c] = sum_b x[a + 4 b] W4^{b c}
#pragma unroll
        for (int a = 1; a < 4; ++a)
#pragma unroll
            for (int c = 1; c < 4; ++c) v[a + 4 * c] = sc_cmul(v[a + 4 * c], make_float2(SC_W16_C[a * c], -SC_W16_S[a * c]));
        float2 t[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sc_dft4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);                // over a: v[4 c + d] = X[c + 4 d]
#pragma unroll
            for (int d = 0; d < 4; ++d) t[c + 4 * d] = v[4 * c + d];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = t[k];
    }
}
// Q of SPEC 3.0h
__device__ __forceinline__ unsigned long long sc_q(float2 X, float scale)
{
    float s = __builtin_fmaf(X.y, X.y, X.x * X.x) * scale;
    s = s != s ? 0.0f : s;
    s = s > 0x1p62f ? 0x1p62f : s;
    return (unsigned long long)(long)__builtin_rintf(s);
}

// where the frames of a launch go when they go into rows (SPEC 3.0i; p25fe_waterfall.inc): frame f0 + g of the range belongs to
// slot (f0 + g) / B, whose row is acc + (slot - slot0) stride.  All of it is uniform: the compiler keeps it in scalar registers
struct SurveyRows {
    unsigned long long f0;      // absolute index of the range's first owned frame
    unsigned long long slot0;   // the slot of row 0
    long stride;                // words from one row to the next (>= N + 1)
    unsigned B;                 // frames per slot
};

// The body of k_scan and of k_waterfall: the hop loader, the staging, the transform of every frame up to x[r] as bins in natural
// order and the sums are one text.  ROWS = false: the sums of all the workgroup's frames go into a.acc once, behind the loop
// (rw is not looked at).  ROWS = true: they go into the current slot's row whenever a slot or the batch ends, and start over.
// Inlined into its kernel, whose launch bound it runs under.  (`a` by value and the table staged behind the early return: in this
// form the eight k_scan instantiations keep the registers tests/test_isa_scan.py pins; the arithmetic does not depend on either.)
template <int FMT, bool LUTM, int N, bool ROWS>
__device__ __forceinline__ void sc_frames(const SurveyArgs a, const WideConv& cv, const SurveyRows& rw)
{
    static_assert(FMT == P25FE_FMT_U8 || !LUTM, "only u8 has a table");
    constexpr int R = sc_radix(N), P = sc_passes(N), T = N / R;
    static_assert(T == SC_WG, "a lane owns one butterfly of every pass");
    constexpr int LS = wide_log_spv(FMT), SPV = 1 << LS;
    constexpr int NVC = (N >> LS) / SC_WG + 1;                      // vectors per lane of the largest hop (H = N) at any alignment
    __shared__ float2 RING[sc_pad(N)];                              // entry (strip position mod N), cf32
    __shared__ float2 BUF[sc_pad(N)];                               // the transposes between passes
    const int tid = threadIdx.x;
    const float* lut = nullptr;
    const long g0 = (long)blockIdx.x * a.F;                         // the workgroup's first frame
    long nfl = a.n_frames - g0;
    if (nfl <= 0) return;                                           // uniform (the host launches no such workgroup)
    const int nf = (int)(nfl < (long)a.F ? nfl : (long)a.F);
    if constexpr (LUTM) {
        __shared__ float LUT[256];
        LUT[tid] = cv.lut[tid];
        lut = LUT;
    }
    const int H = a.H, HV = H >> LS, NH = N / H;
    // the strip: position p is sample s0 + p (relative to owned sample 0); hop c covers positions [c H, c H + H)
    const long s0 = a.e0 + g0 * H - (N - 1);
    const long v0 = s0 >> LS;
    const int sh = (int)(s0 - (v0 << LS));                          // 0 .. SPV - 1, the same for every hop (H is a multiple of 8)
    const long lo = (-a.n_hist) >> LS, hi = (a.n_new - 1) >> LS;    // the vectors that hold a valid sample
    const uint4* xb = reinterpret_cast<const uint4*>(a.x);

    uint4 v[NVC];
#pragma unroll
    for (int m = 0; m < NVC; ++m) v[m] = make_uint4(0u, 0u, 0u, 0u);
    auto load = [&](int c) {
        const long vb = v0 + (long)c * HV;
#pragma unroll
        for (int m = 0; m < NVC; ++m) {
            const int i = tid + m * SC_WG;
            if (i <= HV) {                                          // (vector HV holds the hop's last sh samples)
                long r = vb + i;
                r = r < lo ? lo : r;
                r = r > hi ? hi : r;
                v[m] = xb[r];
            }
        }
    };
    auto stage = [&](int c) {
        const long sb = s0 + (long)c * H;                           // sample of the hop's position 0
        const int rb = (int)(((long)c * H) & (N - 1));
        // positions [zlo, zhi) of the hop hold valid samples, the others read as zero (32-bit from here on)
        const long vl = -a.n_hist - sb, vh = a.n_new - sb;
        const int zlo = (int)(vl < 0 ? 0 : (vl > H ? H : vl)), zhi = (int)(vh < 0 ? 0 : (vh > H ? H : vh));
        int shv = sh;
        asm volatile("" : "+s"(shv));                               // per hop: the positions below are not carried across the frame loop
#pragma unroll
        for (int m = 0; m < NVC; ++m) {
            const int i = tid + m * SC_WG;
            if (i <= HV) {
#pragma unroll
                for (int e = 0; e < SPV; ++e) {
                    const int k = SPV * i + e - shv;                // position inside the hop
                    float2 s2 = wide_sample<FMT, LUTM>(v[m], e, cv, lut);
                    if (k < zlo || k >= zhi) s2 = make_float2(0.f, 0.f);
                    if ((unsigned)k < (unsigned)H) RING[sc_pad(rb + k)] = s2;
                }
            }
        }
    };

    // what does not depend on the frame: this lane's window values, twiddles and sums
    constexpr bool WREG = R == 4;                                   // radix 16 reads its 16 window values per frame (coalesced, L2)
    float wr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wr[r] = WREG ? a.win[tid + r * T] : 0.0f;
    // twiddles of pass p (Ns = R^p): e^{-2 pi i k r / (Ns R)} with k = j % Ns, entry k r N / (Ns R) of the table.  Radix 4 keeps
    // them in registers (12 pairs).  Radix 16 has two such passes of 15 pairs a lane: pass 1's (k = j % 16: 240 distinct pairs)
    // sit in LDS, the last pass's (k = j) are read from the table for every frame, which L2 serves
    constexpr int PREG = R == 16 ? 0 : P - 1;                       // passes whose twiddles stay in registers
    float2 twr[PREG > 0 ? PREG : 1][R - 1];
    __shared__ float2 TW1[R == 16 ? 16 * 15 : 1];
    if constexpr (R == 16) {
        if (tid < 16 * 15) TW1[tid] = a.tw[(tid / 15) * (tid % 15 + 1) * (N / 256)];   // [k][r - 1]
    } else {
#pragma unroll
        for (int p = 1; p <= PREG; ++p) {
            int Ns = 1;
#pragma unroll
            for (int q = 0; q < p; ++q) Ns *= R;
            const int k = tid & (Ns - 1), step = N / (Ns * R);
#pragma unroll
            for (int r = 1; r < R; ++r) twr[p - 1][r - 1] = a.tw[k * r * step];
        }
    }
    unsigned long long sum[R];
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = 0ull;
    // the slot of the workgroup's first frame (one 64-bit division), the frames it still lacks, its row and the frames summed
    unsigned long long* row = a.acc;
    unsigned left = 0u, held = 0u;
    if constexpr (ROWS) {
        const unsigned long long fa = rw.f0 + (unsigned long long)g0, slot = fa / rw.B;
        left = rw.B - (unsigned)(fa - slot * rw.B);
        row += (long)(slot - rw.slot0) * rw.stride;
    }

    if constexpr (LUTM) __syncthreads();                            // the table before the first look-up
    for (int c = 0; c < NH; ++c) { load(c); stage(c); }             // frame 0's hops
#pragma unroll 1
    for (int g = 0; g < nf; ++g) {
        __syncthreads();                                            // the ring holds frame g
        float2 x[R];
        const int rot = (int)(((long)g * H) & (N - 1));
        if constexpr (!WREG) {
            const float* wg = a.win;
            asm volatile("" : "+s"(wg));                            // (not held across the loop)
#pragma unroll
            for (int r = 0; r < R; ++r) wr[r] = wg[tid + r * T];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float2 s = RING[sc_pad((rot + tid + r * T) & (N - 1))];
            x[r] = make_float2(wr[r] * s.x, wr[r] * s.y);
        }
        const bool more = g + 1 < nf;                               // uniform
        if (more) load(g + NH);                                     // the next frame's hop, under pass 0's butterflies
        sc_dft<R>(x);                                               // pass 0: Ns = 1, no twiddles
#pragma unroll
        for (int r = 0; r < R; ++r) BUF[sc_pad(tid * R + r)] = x[r];
        __syncthreads();                                            // (every lane has read the ring, too)
        if (more) stage(g + NH);                                    // ... over hop g, which no later frame needs
#pragma unroll
        for (int p = 1; p < P; ++p) {
            int Ns = 1;
#pragma unroll
            for (int q = 0; q < p; ++q) Ns *= R;
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = BUF[sc_pad(tid + r * T)];
            if constexpr (R == 4) {
#pragma unroll
                for (int r = 1; r < R; ++r) x[r] = sc_cmul(x[r], twr[p - 1][r - 1]);
            } else if (p == 1) {
                const float2* t1 = TW1 + (tid & 15) * 15;
#pragma unroll
                for (int r = 1; r < R; ++r) x[r] = sc_cmul(x[r], t1[r - 1]);
            } else {
                const float2* twg = a.tw;
                asm volatile("" : "+s"(twg));                       // read per frame: 30 registers are not held across the loop
#pragma unroll
                for (int r = 1; r < R; ++r) x[r] = sc_cmul(x[r], twg[tid * r]);
            }
            sc_dft<R>(x);
            if (p < P - 1) {
                __syncthreads();                                    // every lane has read this pass's input
                const int j0 = (tid / Ns) * Ns * R + (tid & (Ns - 1));
#pragma unroll
                for (int r = 0; r < R; ++r) BUF[sc_pad(j0 + r * Ns)] = x[r];
                __syncthreads();
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) sum[r] += sc_q(x[r], a.scale); // x[r] is bin tid + 256 r
        if constexpr (ROWS) {
            ++held;
            if (--left == 0u || !more) {                            // uniform: the slot is complete, or the batch ends inside it
#pragma unroll
                for (int r = 0; r < R; ++r) { atomicAdd(row + tid + r * T, sum[r]); sum[r] = 0ull; }
                if (tid == 0) atomicAdd(row + N, (unsigned long long)held);
                row += rw.stride; left = rw.B; held = 0u;
            }
        }
    }
    if constexpr (!ROWS) {
#pragma unroll
        for (int r = 0; r < R; ++r) atomicAdd(a.acc + tid + r * T, sum[r]);
        if (tid == 0) atomicAdd(a.acc + N, (unsigned long long)nf);
    }
}

template <int FMT, bool LUTM, int N>
__global__ __launch_bounds__(SC_WG, 2) void k_scan(SurveyArgs a, WideConv cv)
{
    sc_frames<FMT, LUTM, N, false>(a, cv, SurveyRows{});
}

}  // namespace p25k

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
struct p25fe_scanner {
    p25fe_t* h = nullptr;
    int device = 0;                        // h's, kept here: destroying the object must not read the handle
    int N = 0, H = 0, shift = 0;
    DevBuf d_win, d_tw;
    // the host streaming form: the object's record, the last N - 1 samples (right-aligned in `lead` slots) and a call's device row
    DevBuf d_acc, d_hist, d_in;
    uint64_t pos = 0;                      // samples consumed
    int fmt = -1;                          // format of the stream (-1: none yet)
    // survey over time (3.0i, p25fe_waterfall.inc): the open rows [wf_rows][N + 1] of slots of wf_B frames from slot 0 (wf_B = 0: none)
    DevBuf d_rows;
    uint32_t wf_B = 0;
    size_t wf_rows = 0;
};

namespace {

constexpr double SC_PI = 3.14159265358979323846;
inline bool sc_n_ok(int64_t N) { return N == 1024 || N == 4096; }
inline bool finite_d(double v) { return v - v == 0.0; }
inline bool sc_hop_ok(int64_t N, int64_t H) { return H >= 8 && H <= N && H % 8 == 0 && N % H == 0; }
// frames a range owns: 3.0b's rule with L = 1, M = H
inline size_t sc_n_frames(uint64_t H, uint64_t abs_first, size_t n) { return (size_t)((uint64_t)n / H + (abs_first % H + (uint64_t)n % H) / H); }
inline size_t sc_lead(int N) { return round_up((size_t)N - 1, 8); }
// frames per workgroup: the N / H - 1 hops in front of a batch are read again by its neighbour, so a batch is at least four
// frame lengths; about a thousand workgroups fill the device twice over
inline int sc_batch(int N, int H, size_t n_frames)
{
    return (int)std::min((size_t)1 << 20, std::max({(size_t)8, (size_t)(4 * (N / H)), (n_frames + 1023) / 1024}));
}

// the raster of p25fe_scan_channels and p25fe_waterfall_keys over N bins at fs: the eligible indices, and for each the bins (in
// order of signed frequency) whose powers make pow[r] and those of its raster cell
struct ScRaster {
    struct Chan { int r; double fc; std::vector<uint32_t> in_bw, in_cell; };
    std::vector<Chan> chan;
    std::vector<double> fb;
    int build(int32_t N, double fs, double raster_hz, double half_bw_hz)
    {
        const double rm = floor((fs / 2.0 - raster_hz / 2.0) / raster_hz);
        if (rm < 0.0) return P25FE_OK;
        if (rm > 1e6) return P25FE_ERR_ARG;
        const int rmax = (int)rm;
        fb.resize((size_t)N);
        for (int b = 0; b < N; ++b) fb[(size_t)b] = (double)(b < N / 2 ? b : b - N) * fs / (double)N;
        const double df = fs / (double)N, reach = std::max(half_bw_hz, raster_hz / 2.0);
        for (int r = -rmax; r <= rmax; ++r) {
            const double fc = (double)r * raster_hz;
            if (fabs(fc) + raster_hz / 2.0 > fs / 2.0) continue;
            Chan c; c.r = r; c.fc = fc;
            const long k0 = (long)floor((fc - reach) / df) - 1, k1 = (long)ceil((fc + reach) / df) + 1;
            for (long k = std::max(k0, -(long)(N / 2)); k <= std::min(k1, (long)(N / 2) - 1); ++k) {
                const uint32_t b = (uint32_t)(k < 0 ? k + N : k);
                const double d = fabs(fb[b] - fc);
                if (d <= half_bw_hz) c.in_bw.push_back(b);
                if (d <= raster_hz / 2.0) c.in_cell.push_back(b);
            }
            chan.push_back(std::move(c));
        }
        return P25FE_OK;
    }
};

template <int FMT, bool LUTM>
void sc_launch_as(int N, dim3 grid, hipStream_t st, const SurveyArgs& a, const WideConv& cv)
{
    if (N == 4096) hipLaunchKernelGGL((k_scan<FMT, LUTM, 4096>), grid, dim3(SC_WG), 0, st, a, cv);
    else hipLaunchKernelGGL((k_scan<FMT, LUTM, 1024>), grid, dim3(SC_WG), 0, st, a, cv);
}

// The host streaming form of p25fe_scan and p25fe_waterfall: the format rule, the position, the carried history and the device
// row are the object's and one text; where the call's frames go is `enqueue`(owned sample 0 on the device, format, n_hist, n),
// which runs on the handle's stream at the object's position; `admit`() may refuse the call behind the argument and format checks,
// before anything is copied or consumed
template <class Admit, class Enqueue>
int sc_stream(p25fe_scanner* sc, const void* iq, int fmt, size_t n, Admit admit, Enqueue enqueue)
{
    if (!sc || !sc->h || !wide_fmt_known(fmt) || (n && !iq)) return P25FE_ERR_ARG;
    if (sc->fmt >= 0 && fmt != sc->fmt) return P25FE_ERR_FORMAT;
    if (position_refused(sc->pos) || n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    if (n == 0) return P25FE_OK;
    if (int rc = admit()) return rc;
    p25fe_t* h = sc->h;
    const size_t bps = fmt_bytes(fmt), keep = (size_t)sc->N - 1, lead = sc_lead(sc->N);
    const size_t n_hist = sc->pos < keep ? (size_t)sc->pos : keep;
    // the device row: [the carried history, right-aligned in `lead` slots | n new samples], owned sample 0 16-byte aligned
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sc->d_in.ensure((lead + round_up(n, 8)) * bps));
    unsigned char* din = sc->d_in.as<unsigned char>();
    HIPCHK(h, hipMemcpyAsync(din, sc->d_hist.p, lead * bps, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(din + lead * bps, iq, n * bps, hipMemcpyHostToDevice, h->stream));
    if (int rc = enqueue(din + lead * bps, fmt, n_hist, n)) return rc;
    // the carry moves: the last `lead` samples of [history | new]
    HIPCHK(h, hipMemcpyAsync(sc->d_hist.p, din + n * bps, lead * bps, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                     // the caller's buffer and the row are free again
    sc->pos += n; sc->fmt = fmt;
    return P25FE_OK;
}

}  // namespace

extern "C" {

int p25fe_scan_window(int32_t N, float* w, size_t cap)
{
    if (!sc_n_ok(N)) return P25FE_ERR_ARG;
    if (cap < (size_t)N || !w) return P25FE_ERR_CAPACITY;
    for (int32_t j = 0; j < N; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * SC_PI * (double)j / (double)N));
    return P25FE_OK;
}

int p25fe_scan_create(p25fe_t* h, int32_t N, int32_t hop, const float* window, int32_t shift, p25fe_scan_t** out)
{
    if (out) *out = nullptr;
    if (!out || !sc_n_ok(N) || !sc_hop_ok(N, hop) || shift < 0 || shift > P25FE_SCAN_MAX_SHIFT) return P25FE_ERR_ARG;
    std::vector<float> win((size_t)N);
    if (window) {
        for (int j = 0; j < N; ++j) { if (!finite_f(window[j])) return P25FE_ERR_ARG; win[(size_t)j] = window[j]; }
    } else {
        (void)p25fe_scan_window(N, win.data(), win.size());
    }
    if (!h) return P25FE_ERR_ARG;                                   // (the handle is looked at last)
    p25fe_scanner* sc = new (std::nothrow) p25fe_scanner;
    if (!sc) return P25FE_ERR_NOMEM;
    sc->h = h; sc->device = h->cfg.device; sc->N = N; sc->H = hop; sc->shift = shift;
    std::vector<float> tw(2 * (size_t)N);
    for (int m = 0; m < N; ++m) {
        const double w = 2.0 * SC_PI * (double)m / (double)N;
        tw[2 * (size_t)m] = (float)cos(w); tw[2 * (size_t)m + 1] = (float)-sin(w);
    }
    const size_t rec = ((size_t)N + 1) * sizeof(uint64_t), hist = sc_lead(N) * 8;
    if (hipSetDevice(h->cfg.device) != hipSuccess || sc->d_win.ensure(win.size() * sizeof(float)) != hipSuccess ||
        sc->d_tw.ensure(tw.size() * sizeof(float)) != hipSuccess || sc->d_acc.ensure(rec) != hipSuccess ||
        sc->d_hist.ensure(hist) != hipSuccess ||
        hipMemcpy(sc->d_win.p, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sc->d_tw.p, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(sc->d_acc.p, 0, rec) != hipSuccess || hipMemset(sc->d_hist.p, 0, hist) != hipSuccess) {
        h->last_hip = (int)hipGetLastError(); delete sc; return P25FE_ERR_HIP;
    }
    *out = sc;
    return P25FE_OK;
}

void p25fe_scan_destroy(p25fe_scan_t* sc)
{
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    delete sc;
}

int p25fe_scan_dev(p25fe_scan_t* sc, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint64_t* d_acc,
                   void* stream)
{
    if (!sc || !sc->h || !wide_fmt_known(fmt) || !d_iq || !d_acc || position_refused(abs_first) || n >= P25FE_MAX_POSITION)
        return P25FE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_acc) & 7u) != 0) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    const int N = sc->N, H = sc->H;
    const size_t n_frames = sc_n_frames((uint64_t)H, abs_first, n);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_frames == 0) return P25FE_OK;
    SurveyArgs a;
    a.x = d_iq;
    a.n_hist = (long)std::min(n_hist, (size_t)N - 1);               // nothing before that is ever read
    a.n_new = (long)n;
    a.e0 = (long)(H - 1 - (int)(abs_first % (uint64_t)H));
    a.n_frames = (long)n_frames;
    a.H = H;
    a.F = sc_batch(N, H, n_frames);
    a.scale = ldexpf(1.0f, sc->shift);
    a.win = sc->d_win.as<float>(); a.tw = sc->d_tw.as<float2>();
    a.acc = reinterpret_cast<unsigned long long*>(d_acc);
    const size_t groups = (n_frames + (size_t)a.F - 1) / (size_t)a.F;
    if (groups > (size_t)0x7fffffffu) return P25FE_ERR_ARG;
    const dim3 grid((unsigned)groups);
    const WideConv cv = wide_conv_of(h);
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();                                        // the check below is for THIS launch
    if (fmt == P25FE_FMT_CF32) sc_launch_as<P25FE_FMT_CF32, false>(N, grid, st, a, cv);
    else if (fmt == P25FE_FMT_S16) sc_launch_as<P25FE_FMT_S16, false>(N, grid, st, a, cv);
    else if (cv.lut) sc_launch_as<P25FE_FMT_U8, true>(N, grid, st, a, cv);
    else sc_launch_as<P25FE_FMT_U8, false>(N, grid, st, a, cv);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_scan(p25fe_scan_t* sc, const void* iq, int fmt, size_t n)
{
    return sc_stream(sc, iq, fmt, n, [] { return P25FE_OK; }, [sc](const void* d_iq, int f, size_t n_hist, size_t cnt) {
        return p25fe_scan_dev(sc, d_iq, f, n_hist, cnt, sc->pos, sc->d_acc.as<uint64_t>(), sc->h->stream);
    });
}

int p25fe_scan_reset(p25fe_scan_t* sc)
{
    if (!sc || !sc->h) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemset(sc->d_acc.p, 0, ((size_t)sc->N + 1) * sizeof(uint64_t)));
    if (sc->wf_B) HIPCHK(h, hipMemset(sc->d_rows.p, 0, sc->wf_rows * ((size_t)sc->N + 1) * sizeof(uint64_t)));
    sc->pos = 0; sc->fmt = -1;
    return P25FE_OK;
}

int p25fe_scan_read(p25fe_scan_t* sc, uint64_t* acc_out, int clear)
{
    if (!sc || !sc->h || !acc_out) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    const size_t rec = ((size_t)sc->N + 1) * sizeof(uint64_t);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(acc_out, sc->d_acc.p, rec, hipMemcpyDeviceToHost));
    if (clear) HIPCHK(h, hipMemset(sc->d_acc.p, 0, rec));
    return P25FE_OK;
}

int p25fe_scan_channels(const uint64_t* acc, int32_t N, uint32_t fs_hz, double raster_hz, double half_bw_hz, double thr_db,
                        p25fe_scan_chan_t* out, size_t cap, size_t* n_out)
{
    if (n_out) *n_out = 0;
    if (!acc || !n_out || (cap && !out) || !sc_n_ok(N) || fs_hz == 0 || !finite_d(raster_hz) || !(raster_hz > 0.0) ||
        !finite_d(half_bw_hz) || half_bw_hz < 0.0 || !finite_d(thr_db)) return P25FE_ERR_ARG;
    if (acc[N] == 0) return P25FE_OK;                               // no frame: no channel
    ScRaster ra;
    if (int rc = ra.build(N, (double)fs_hz, raster_hz, half_bw_hz)) return rc;   // (none eligible: the raster is wider than the capture)
    struct Cand { int r; double pow, off; };
    std::vector<Cand> cand;
    std::vector<double> pows;
    for (const ScRaster::Chan& c : ra.chan) {
        double p = 0.0, s = 0.0, sf = 0.0;
        for (uint32_t b : c.in_bw) p += (double)acc[b];
        for (uint32_t b : c.in_cell) { const double v = (double)acc[b]; s += v; sf += v * ra.fb[b]; }
        pows.push_back(p);
        cand.push_back(Cand{c.r, p, s > 0.0 ? sf / s - c.fc : 0.0});
    }
    if (cand.empty()) return P25FE_OK;
    std::vector<double> sorted(pows);
    std::sort(sorted.begin(), sorted.end());
    const double flr = sorted[(sorted.size() - 1) / 2];             // the lower median
    const double thr = flr * pow(10.0, thr_db / 10.0);
    std::vector<Cand> act;
    for (const Cand& c : cand) if (c.pow > 0.0 && c.pow >= thr) act.push_back(c);
    std::stable_sort(act.begin(), act.end(), [](const Cand& x, const Cand& y) { return x.pow > y.pow; });   // ties: the smaller r first
    *n_out = act.size();
    for (size_t i = 0; i < act.size() && i < cap; ++i) {
        out[i].raster_index = act[i].r; out[i].reserved = 0;
        out[i].centre_hz = (double)act[i].r * raster_hz;
        out[i].db_over_floor = flr > 0.0 ? 10.0 * log10(act[i].pow / flr) : HUGE_VAL;
        out[i].offset_hz = act[i].off;
    }
    return P25FE_OK;
}

}  // extern "C"

#endif  /* P25FE_SCAN_INC */
