// p25fe_waterfall.inc -- survey over time: per-slot spectra of a capture in one launch, and keyed intervals (docs/SPEC.md 3.0i;
// kernel: k_waterfall), device and host side.  Included by p25fe_api.hip behind p25fe_scan.inc; never embedded for hipRTC.
//
// K0e, k_waterfall<FMT, LUTM, N>: k_scan's body (sc_frames: the hop loader, the staging, the Stockham passes and the sums are the
// same text) with the sums delivered per SLOT of B frames instead of once per workgroup.  Frame f of the stream belongs to slot
// f / B, row slot - slot0 of d_rows.  One 64-bit division places the workgroup's first frame; from there a counter of the frames
// the slot still lacks runs down, and when it reaches zero, or the batch ends, every lane issues its R 64-bit atomic adds into the
// current row, lane 0 adds the frames summed, the sums start over and the row pointer moves on by the stride.  All of that is
// uniform and lives in scalar registers.  A frame's Q values are k_scan's, and integer sums commute: the rows do not depend on F,
// on where a slot's boundary falls in a batch, or on how a stream is split into calls.
#ifndef P25FE_WATERFALL_INC
#define P25FE_WATERFALL_INC

namespace p25k {

template <int FMT, bool LUTM, int N>
__global__ __launch_bounds__(SC_WG, 2) void k_waterfall(SurveyArgs a, WideConv cv, SurveyRows rw)
{
    sc_frames<FMT, LUTM, N, true>(a, cv, rw);
}

}  // namespace p25k

namespace {

constexpr uint32_t WF_MAX_B = 1u << 20;
constexpr size_t WF_MAX_ROWS = (size_t)1 << 20;

template <int FMT, bool LUTM>
void wf_launch_as(int N, dim3 grid, hipStream_t st, const SurveyArgs& a, const WideConv& cv, const SurveyRows& rw)
{
    if (N == 4096) hipLaunchKernelGGL((k_waterfall<FMT, LUTM, 4096>), grid, dim3(SC_WG), 0, st, a, cv, rw);
    else hipLaunchKernelGGL((k_waterfall<FMT, LUTM, 1024>), grid, dim3(SC_WG), 0, st, a, cv, rw);
}

// the slots the frames of [abs_first, abs_first + n) fall into: [*first, *first + *count), count = 0 when the range owns no frame
inline void wf_slots(uint64_t H, uint64_t B, uint64_t abs_first, size_t n, uint64_t* first, size_t* count)
{
    const uint64_t f0 = abs_first / H, nf = sc_n_frames(H, abs_first, n);
    *first = f0 / B;
    *count = nf ? (size_t)((f0 + nf - 1) / B - f0 / B + 1) : 0;
}

}  // namespace

extern "C" {

int p25fe_waterfall_slots(int32_t hop, uint32_t B, uint64_t abs_first, size_t n, uint64_t* first_slot, size_t* n_slots)
{
    if (first_slot) *first_slot = 0;
    if (n_slots) *n_slots = 0;
    if (!first_slot || !n_slots || !sc_hop_ok(4096, hop) || B == 0 || B > WF_MAX_B || position_refused(abs_first) ||
        n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    wf_slots((uint64_t)hop, B, abs_first, n, first_slot, n_slots);
    return P25FE_OK;
}

int p25fe_waterfall_dev(p25fe_scan_t* sc, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, uint32_t B,
                        uint64_t slot0, uint64_t* d_rows, size_t n_rows, size_t row_stride, void* stream)
{
    if (!sc || !sc->h || !wide_fmt_known(fmt) || !d_iq || !d_rows || position_refused(abs_first) || n >= P25FE_MAX_POSITION)
        return P25FE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_rows) & 7u) != 0) return P25FE_ERR_ARG;
    if (B == 0 || B > WF_MAX_B || row_stride < (size_t)sc->N + 1 || row_stride >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    const int N = sc->N, H = sc->H;
    const size_t n_frames = sc_n_frames((uint64_t)H, abs_first, n);
    uint64_t first = 0; size_t count = 0;
    wf_slots((uint64_t)H, B, abs_first, n, &first, &count);
    if (n_frames != 0 && n_rows == 0) return P25FE_ERR_ARG;
    // every slot the range touches has a row: nothing is enqueued otherwise
    if (n_frames != 0 && (first < slot0 || first - slot0 >= n_rows || count > n_rows - (size_t)(first - slot0))) return P25FE_ERR_CAPACITY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_frames == 0) return P25FE_OK;
    SurveyArgs a;
    a.x = d_iq;
    a.n_hist = (long)std::min(n_hist, (size_t)N - 1);
    a.n_new = (long)n;
    a.e0 = (long)(H - 1 - (int)(abs_first % (uint64_t)H));
    a.n_frames = (long)n_frames;
    a.H = H;
    a.F = sc_batch(N, H, n_frames);                                 // p25fe_scan_dev's plan
    a.scale = ldexpf(1.0f, sc->shift);
    a.win = sc->d_win.as<float>(); a.tw = sc->d_tw.as<float2>();
    a.acc = reinterpret_cast<unsigned long long*>(d_rows);
    SurveyRows rw;
    rw.f0 = abs_first / (uint64_t)H; rw.slot0 = slot0; rw.stride = (long)row_stride; rw.B = B;
    const size_t groups = (n_frames + (size_t)a.F - 1) / (size_t)a.F;
    if (groups > (size_t)0x7fffffffu) return P25FE_ERR_ARG;
    const dim3 grid((unsigned)groups);
    const WideConv cv = wide_conv_of(h);
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();                                        // the check below is for THIS launch
    if (fmt == P25FE_FMT_CF32) wf_launch_as<P25FE_FMT_CF32, false>(N, grid, st, a, cv, rw);
    else if (fmt == P25FE_FMT_S16) wf_launch_as<P25FE_FMT_S16, false>(N, grid, st, a, cv, rw);
    else if (cv.lut) wf_launch_as<P25FE_FMT_U8, true>(N, grid, st, a, cv, rw);
    else wf_launch_as<P25FE_FMT_U8, false>(N, grid, st, a, cv, rw);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

int p25fe_waterfall_open(p25fe_scan_t* sc, uint32_t B, size_t max_rows)
{
    if (!sc || !sc->h || B == 0 || B > WF_MAX_B || max_rows == 0 || max_rows > WF_MAX_ROWS) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    const size_t bytes = max_rows * ((size_t)sc->N + 1) * sizeof(uint64_t);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sc->wf_B = 0; sc->wf_rows = 0;
    HIPCHK(h, sc->d_rows.ensure(bytes));
    HIPCHK(h, hipMemset(sc->d_rows.p, 0, bytes));
    sc->wf_B = B; sc->wf_rows = max_rows;
    return P25FE_OK;
}

int p25fe_waterfall(p25fe_scan_t* sc, const void* iq, int fmt, size_t n)
{
    if (!sc || !sc->h || sc->wf_B == 0) return P25FE_ERR_ARG;
    // behind the argument and format checks, before anything is copied: every frame the call owns has a row, or nothing is consumed
    const auto admit = [sc, n] {
        uint64_t first = 0; size_t count = 0;
        wf_slots((uint64_t)sc->H, sc->wf_B, sc->pos, n, &first, &count);
        return count != 0 && (first >= sc->wf_rows || count > sc->wf_rows - (size_t)first) ? P25FE_ERR_CAPACITY : P25FE_OK;
    };
    return sc_stream(sc, iq, fmt, n, admit, [sc](const void* d_iq, int f, size_t n_hist, size_t cnt) {
        return p25fe_waterfall_dev(sc, d_iq, f, n_hist, cnt, sc->pos, sc->wf_B, 0, sc->d_rows.as<uint64_t>(), sc->wf_rows,
                                   (size_t)sc->N + 1, sc->h->stream);
    });
}

int p25fe_waterfall_read(p25fe_scan_t* sc, uint64_t* rows_out, size_t cap_rows, size_t* n_rows)
{
    if (n_rows) *n_rows = 0;
    if (!sc || !sc->h || sc->wf_B == 0 || !n_rows || (cap_rows && !rows_out)) return P25FE_ERR_ARG;
    p25fe_t* h = sc->h;
    // the rows touched so far, and never more than there are: p25fe_scan moves the same position and has no last row
    const size_t rows = (size_t)std::min<uint64_t>((sc->pos / (uint64_t)sc->H + sc->wf_B - 1) / sc->wf_B, sc->wf_rows);
    *n_rows = rows;
    if (rows > cap_rows) return P25FE_ERR_CAPACITY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (rows) HIPCHK(h, hipMemcpy(rows_out, sc->d_rows.p, rows * ((size_t)sc->N + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return P25FE_OK;
}

int p25fe_waterfall_keys(const uint64_t* rows, size_t n_rows, size_t row_stride, int32_t N, uint32_t fs_hz, uint64_t slot0,
                         double raster_hz, double half_bw_hz, double on_db, double off_db, uint32_t min_slots,
                         p25fe_waterfall_key_t* out, size_t cap, size_t* n_out)
{
    if (n_out) *n_out = 0;
    if (!n_out || (n_rows && !rows) || (cap && !out) || !sc_n_ok(N) || row_stride < (size_t)N + 1 || fs_hz == 0 ||
        !finite_d(raster_hz) || !(raster_hz > 0.0) || !finite_d(half_bw_hz) || half_bw_hz < 0.0 || !finite_d(on_db) ||
        !finite_d(off_db) || off_db > on_db || min_slots == 0) return P25FE_ERR_ARG;
    ScRaster ra;
    if (int rc = ra.build(N, (double)fs_hz, raster_hz, half_bw_hz)) return rc;
    const size_t C = ra.chan.size();
    if (C == 0 || n_rows == 0) return P25FE_OK;
    const double on = pow(10.0, on_db / 10.0), off = pow(10.0, off_db / 10.0);
    struct Open { bool live = false; size_t first = 0; double s = 0.0, sf = 0.0, peak = 0.0; };
    std::vector<Open> open(C);
    std::vector<p25fe_waterfall_key_t> keys;
    std::vector<double> pows(C), sorted(C);
    const auto close = [&](size_t c, size_t end) {                  // the interval of channel c ends in front of row `end`
        Open& o = open[c];
        if (o.live && end - o.first >= (size_t)min_slots) {
            p25fe_waterfall_key_t k;
            k.raster_index = ra.chan[c].r; k.reserved = 0;
            k.first_slot = slot0 + o.first; k.n_slots = end - o.first;
            k.centre_hz = ra.chan[c].fc;
            k.offset_hz = o.s > 0.0 ? o.sf / o.s - ra.chan[c].fc : 0.0;
            k.peak_db_over_floor = o.peak;
            keys.push_back(k);
        }
        o = Open();
    };
    for (size_t t = 0; t < n_rows; ++t) {
        const uint64_t* row = rows + t * row_stride;
        if (row[N] == 0) {                                          // no frame: every open interval ends
            for (size_t c = 0; c < C; ++c) close(c, t);
            continue;
        }
        for (size_t c = 0; c < C; ++c) {
            double p = 0.0;
            for (uint32_t b : ra.chan[c].in_bw) p += (double)row[b];
            pows[c] = p;
        }
        sorted = pows;
        std::sort(sorted.begin(), sorted.end());
        const double flr = sorted[(C - 1) / 2];                     // the lower median
        for (size_t c = 0; c < C; ++c) {
            Open& o = open[c];
            const double p = pows[c];
            if (o.live && !(p >= flr * off)) close(c, t);
            if (!o.live && p > 0.0 && p >= flr * on) { o.live = true; o.first = t; o.peak = -HUGE_VAL; }
            if (o.live) {
                for (uint32_t b : ra.chan[c].in_cell) { const double v = (double)row[b]; o.s += v; o.sf += v * ra.fb[b]; }
                const double db = flr > 0.0 ? 10.0 * log10(p / flr) : HUGE_VAL;
                if (db > o.peak) o.peak = db;
            }
        }
    }
    for (size_t c = 0; c < C; ++c) close(c, n_rows);
    std::stable_sort(keys.begin(), keys.end(), [](const p25fe_waterfall_key_t& x, const p25fe_waterfall_key_t& y) {
        return x.first_slot != y.first_slot ? x.first_slot < y.first_slot : x.raster_index < y.raster_index;
    });
    *n_out = keys.size();
    for (size_t i = 0; i < keys.size() && i < cap; ++i) out[i] = keys[i];
    return P25FE_OK;
}

}  // extern "C"

#endif  /* P25FE_WATERFALL_INC */
