// p25fe_measure.inc -- bodies of the measurement hooks of p25fe_kernels.hip / p25fe_recv.hip / p25fe_api.hip.
// Included ONLY by builds made with -DP25FE_MEASURE (tools/ablate.sh, tools/k1_stamps.py, tools/k6_variants.sh, `make variant`): never
// part of libp25fe.so, never embedded for hipRTC (the Makefile's embed list does not name it).  Switches, as before the hooks existed:
//   P25FE_ABLATE=N          K1 truncated after stage N (1 loads, 2 decimator, 3 channel filter, 4 discriminator, 5 no output staging,
//                           6 every window load served from one cached row); P25FE_ABLATE_CACHED: that loader with any N;
//                           P25FE_ABLATE_STORES: N = 1 keeps the output stream; P25FE_DRIFT / P25FE_DRIFT_SPREAD: s_sleep phases there
//                           (k_frontend_pair: N = 1, with or without P25FE_ABLATE_STORES, and N = 6)
//   P25FE_EXP (bit mask)    1 no sign planes, 4 channel filter without its FMAs, 8 no baseband stores
//   P25FE_K1_STAMP          shader-clock time per phase of the sub-tiles, summed into g_k1_stamp (p25fe_debug_k1_stamps)
//   P25FE_ABLATE_DET=1,2    K2 after the screen / after the exact test;   P25FE_ABLATE6=1,2   K6's store stream alone
//   P25FE_MEASURE_UNSAFE    p25fe_run_dev_pipelined without the cross-stream wait in front of K1 (P25FE_PIPE_NOWAIT=1; timing only)
#ifndef P25FE_MEASURE_INC
#define P25FE_MEASURE_INC

#ifndef P25FE_ABLATE
#define P25FE_ABLATE 99
#endif
#ifndef P25FE_EXP
#define P25FE_EXP 0
#endif

#if P25FE_ABLATE == 6 || defined(P25FE_ABLATE_CACHED)
#define P25FE_M_LOAD_OFFSET(product_, cached_row_) (cached_row_)
#else
#define P25FE_M_LOAD_OFFSET(product_, cached_row_) (product_)
#endif

#define P25FE_M_NO_BB_STORES ((P25FE_EXP & 8) != 0)
#define P25FE_M_NO_SIGN_PLANES ((P25FE_EXP & 1) != 0)
#define P25FE_M_NO_CH_FMA ((P25FE_EXP & 4) != 0)
#define P25FE_M_NO_OUT_STAGE (P25FE_ABLATE == 5)
#define P25FE_M_KEEP1(a_) asm volatile("" ::"v"(a_))
#define P25FE_M_KEEP2(a_, b_) asm volatile("" ::"v"(a_), "v"(b_))

#ifdef P25FE_K1_STAMP
// (this file is included inside namespace p25k)
constexpr int K1_STAMP_SLOTS = 8192;          // workgroup b adds into slot b % 8192: no hot address
__device__ unsigned long long g_k1_stamp[K1_STAMP_SLOTS][16];
#define K1_STAMP(i)                                                                   \
    do {                                                                              \
        unsigned long long t_;                                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");   \
        st_acc[i] += t_ - st_last;                                                    \
        st_last = t_;                                                                 \
    } while (0)
#define K1_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))
#define P25FE_M_PIN_V2(arr_, n_) _Pragma("unroll") for (int p_ = 0; p_ < (n_); ++p_) K1_PIN2((arr_)[p_].x, (arr_)[p_].y)
#define P25FE_M_PIN_F2(arr_, n_) _Pragma("unroll") for (int p_ = 0; p_ < (n_); ++p_) K1_PIN2((arr_)[p_].x, (arr_)[p_].y)
#define P25FE_M_ENTRY                                                                                                   \
    unsigned long long st_t0, st_r0;                                /* entry: shader clock / constant 100 MHz clock */   \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t0), "=s"(st_r0)::"memory")
#define P25FE_M_LOCALS unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_last = 0, st_n = 0, st_pro = 0, st_items = 0
#define P25FE_M_ITEM                                                                  \
    unsigned long long st_i0;                                                         \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_i0)::"memory");    \
    bool st_first_sub = true;                                                         \
    ++st_items
#define P25FE_M_SUBTILE                                                               \
    do {                                                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_last)::"memory"); \
        if (st_first_sub) { st_pro += st_last - st_i0; st_first_sub = false; }        \
        ++st_n;                                                                       \
    } while (0)
#define P25FE_M_EXIT                                                                                                    \
    if (tid == 0) {                                                                                                     \
        unsigned long long st_t1, st_r1;                                                                                \
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t1), "=s"(st_r1)::"memory");  \
        unsigned long long* slot = g_k1_stamp[blockIdx.x % K1_STAMP_SLOTS];                                             \
        for (int i = 0; i < 7; ++i) atomicAdd(&slot[i], st_acc[i]);                                                     \
        atomicAdd(&slot[7], st_n);                                                                                      \
        atomicAdd(&slot[8], st_pro);                                /* prologues: item start -> its first sub-tile */    \
        atomicAdd(&slot[9], st_t1 - st_t0);                         /* lifetime, shader clock */                         \
        atomicAdd(&slot[10], st_r1 - st_r0);                        /* lifetime, 100 MHz clock */                        \
        atomicAdd(&slot[11], 1ull);                                 /* workgroups */                                     \
        atomicAdd(&slot[12], st_items);                             /* work items */                                     \
    }
#else
#define K1_STAMP(i) do { } while (0)
#define K1_PIN2(a, b) do { } while (0)
#define P25FE_M_PIN_V2(arr_, n_) do { } while (0)
#define P25FE_M_PIN_F2(arr_, n_) do { } while (0)
#define P25FE_M_ENTRY do { } while (0)
#define P25FE_M_LOCALS do { } while (0)
#define P25FE_M_ITEM do { } while (0)
#define P25FE_M_SUBTILE do { } while (0)
#define P25FE_M_EXIT do { } while (0)
#endif

// truncated builds: the sub-tile lambda returns after stage N (what it has computed is kept alive)
#if P25FE_ABLATE <= 1
#if defined(P25FE_ABLATE_STORES)            // ... N = 1 keeping the OUTPUT stream: the next iteration stores this sub-tile's (zero) planes --
#define P25FE_M_CUT_STORES_ out_rel = (int)(dlo - m_seg0);          /* K1's whole HBM traffic without its arithmetic */
#else
#define P25FE_M_CUT_STORES_
#endif
#if defined(P25FE_DRIFT)                    // ... with pseudo-random idle phases (units of 64 cycles) in place of the arithmetic
#define P25FE_M_CUT_DRIFT_                                                                                   \
    {                                                                                                        \
        unsigned hsh = (unsigned)blockIdx.x * 2654435761u + (unsigned)(dlo & 0xffff) * 40503u;               \
        hsh ^= hsh >> 13;                                                                                    \
        const int units = P25FE_DRIFT + (int)(hsh % (unsigned)(P25FE_DRIFT_SPREAD + 1));                     \
        for (int u = 0; u < units; ++u) __builtin_amdgcn_s_sleep(1);                                         \
    }
#else
#define P25FE_M_CUT_DRIFT_
#endif
#define P25FE_M_CUT_LOADS do { P25FE_M_CUT_STORES_ P25FE_M_CUT_DRIFT_ return true; } while (0)
#else
#define P25FE_M_CUT_LOADS do { } while (0)
#endif
#define P25FE_M_CUT(stage_) do { if constexpr (P25FE_ABLATE <= (stage_)) return true; } while (0)
// k_frontend_pair with N = 1: the producer stops behind its window turnaround, the consumer behind B(t) -- both keep their barriers;
// P25FE_ABLATE_STORES: the consumer's next iteration stores this sub-tile's (zero) planes.  (N = 6 needs no hook: the loader's offset.)
#if P25FE_ABLATE <= 1
#define P25FE_M_PAIR_PRODUCER_CUT { pair_barrier(); continue; }
#if defined(P25FE_ABLATE_STORES)
#define P25FE_M_PAIR_CONSUMER_CUT { out_rel = t * SUB; continue; }
#else
#define P25FE_M_PAIR_CONSUMER_CUT { continue; }
#endif
#else
#define P25FE_M_PAIR_PRODUCER_CUT do { } while (0)
#define P25FE_M_PAIR_CONSUMER_CUT do { } while (0)
#endif
#define P25FE_M_CUT_KEEP_F2(stage_, arr_, n_)                                                                \
    do { if constexpr (P25FE_ABLATE <= (stage_)) {                                                           \
        _Pragma("unroll") for (int p_ = 0; p_ < (n_); ++p_) asm volatile("" ::"v"((arr_)[p_].x), "v"((arr_)[p_].y)); \
        return true; } } while (0)
#define P25FE_M_CUT_KEEP_F(stage_, arr_, n_)                                                                 \
    do { if constexpr (P25FE_ABLATE <= (stage_)) {                                                           \
        _Pragma("unroll") for (int p_ = 0; p_ < (n_); ++p_) asm volatile("" ::"v"((arr_)[p_]));              \
        return true; } } while (0)

// K6: the store stream alone (1: 8-byte stores, 2: 16-byte stores -- a lane pair writes two instants of two rows)
#if defined(P25FE_ABLATE6)
#if P25FE_ABLATE6 == 2
#define P25FE_M_K6_STORES_ONLY                                                                               \
    {                                                                                                        \
        const float2 xv = lds_read_c(X + lane);                                                              \
        float4* const y4 = reinterpret_cast<float4*>(yb - (lane & 1));                                       \
        _Pragma("unroll 1") for (int c = 0; c < CZ_M; c += 2) {                                              \
            typedef float __attribute__((ext_vector_type(4))) f32x4;                                         \
            f32x4 ov; ov.x = xv.x + (float)c; ov.y = xv.y; ov.z = xv.x; ov.w = xv.y;                          \
            __builtin_nontemporal_store(ov, reinterpret_cast<f32x4*>(reinterpret_cast<float2*>(y4) + (size_t)(c + (lane & 1)) * a.y_stride)); \
        }                                                                                                    \
        return;                                                                                              \
    }
#else
#define P25FE_M_K6_STORES_ONLY                                                                               \
    {                                                                                                        \
        const float2 xv = lds_read_c(X + lane);                                                              \
        _Pragma("unroll 1") for (int c = 0; c < CZ_M; ++c) yb[(size_t)c * a.y_stride] = make_float2(xv.x + (float)c, xv.y); \
        return;                                                                                              \
    }
#endif
#else
#define P25FE_M_K6_STORES_ONLY do { } while (0)
#endif

// K2 truncated: 1 after the sign-bit screen, 2 after the exact test (no peak test)
#ifndef P25FE_ABLATE_DET
#define P25FE_ABLATE_DET 0
#endif
#define P25FE_M_DET_CUT_SCREEN                                                                               \
    do { if constexpr (P25FE_ABLATE_DET == 1) {                                                              \
        if (lane == 0) a.tsum[(size_t)ch * a.n_tiles + tile] = (hw[0] | hw[1] | hw[2] | hw[3]) == 0x12345u ? 1ull : 0ull; \
        return; } } while (0)
#define P25FE_M_DET_NO_PEAK_TEST (P25FE_ABLATE_DET == 2)

// host side (p25fe_api.hip)
#ifdef P25FE_MEASURE_UNSAFE
// what the cross-stream wait packet in front of a pipelined K1 costs -- without it the planes can be overwritten under a receive kernel
// that is still reading them: timing only
#define P25FE_M_PIPE_NOWAIT() ([] { static const bool nowait = [] { const char* e = getenv("P25FE_PIPE_NOWAIT"); return e && atoi(e) != 0; }(); return nowait; }())
#else
#define P25FE_M_PIPE_NOWAIT() false
#endif
#ifdef P25FE_K1_STAMP
// read (and clear) K1's per-phase cycle sums; out[7] = sub-tiles counted
#define P25FE_M_API_EXTRAS                                                                                               \
    int p25fe_debug_k1_stamps(uint64_t out[16])                                                                          \
    {                                                                                                                    \
        std::vector<unsigned long long> z((size_t)p25k::K1_STAMP_SLOTS * 16, 0ull), v(z.size());                         \
        if (hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(p25k::g_k1_stamp), v.size() * 8) != hipSuccess) return P25FE_ERR_HIP; \
        if (hipMemcpyToSymbol(HIP_SYMBOL(p25k::g_k1_stamp), z.data(), z.size() * 8) != hipSuccess) return P25FE_ERR_HIP;   \
        for (int i = 0; i < 16; ++i) out[i] = 0;                                                                         \
        for (size_t k = 0; k < v.size(); ++k) out[k & 15] += v[k];                                                       \
        return P25FE_OK;                                                                                                 \
    }
#else
#define P25FE_M_API_EXTRAS
#endif

#endif  /* P25FE_MEASURE_INC */
