// p25fe_cuts.inc -- tuner, cuts: many pieces of one capture in a single launch, each the slice of the row p25fe_tune_dev writes for an
// NCO channel over the call's whole range (docs/SPEC.md 3.0j; kernel: k_tune_cuts in p25fe_kernels.hip), host side.  Included by
// p25fe_api.hip behind p25fe_waterfall.inc, whose keys p25fe_cuts_from_keys turns into cuts.
#ifndef P25FE_CUTS_INC
#define P25FE_CUTS_INC

// The cuts of one list on a tuner's device: the records and the exclusive prefix of the cuts' workgroup counts, uploaded once.
// Nothing here depends on a call: the kernel adds the cut's offset into the call's buffer itself.
struct p25fe_cuts {
    p25fe_tuner* tn = nullptr;             // used by every launch (its table, rotator, device and handle), never by the destructor
    int device = 0;
    size_t J = 0;
    std::vector<size_t> cnt;               // outputs per cut
    size_t max_cnt = 0;
    uint64_t lo = 0, hi = 0;               // the cuts' hull [lo, hi): a call's range must hold it
    size_t total_wg = 0;
    DevBuf d_rec, d_first;
};

namespace {

static_assert(sizeof(p25fe_cut_t) == 24 && sizeof(p25fe_waterfall_key_t) == 48, "the records of include/p25fe.h");

template <int FMT, bool LUTM>
void ct_launch_as(dim3 grid, size_t lds, hipStream_t st, const TuneArgs& ta, const CutArgs& ca, const WideConv& cv)
{
    hipLaunchKernelGGL((k_tune_cuts<FMT, LUTM>), grid, dim3(WV), lds, st, ta, ca, cv);
}

// clamp a position that may lie on either side of [lo, hi] into it
inline uint64_t ct_clamp(__int128 v, uint64_t lo, uint64_t hi) { return v < (__int128)lo ? lo : (v > (__int128)hi ? hi : (uint64_t)v); }

}  // namespace

extern "C" {

int p25fe_cuts_from_keys(const p25fe_waterfall_key_t* keys, size_t n_keys, int32_t N, int32_t hop, uint32_t B, uint32_t fs_hz,
                         uint64_t margin, uint64_t range_first, uint64_t range_n, p25fe_cut_t* out, size_t cap, size_t* n_out)
{
    if (n_out) *n_out = 0;
    if (!n_out || (n_keys && !keys) || (cap && !out) || !sc_n_ok(N) || !sc_hop_ok(N, hop) || B == 0 || B > WF_MAX_B || fs_hz == 0 ||
        margin >= P25FE_MAX_POSITION || position_refused(range_first) || range_n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    std::vector<int32_t> step(n_keys);
    for (size_t j = 0; j < n_keys; ++j)
        if (p25fe_nco_step(fs_hz, keys[j].centre_hz + keys[j].offset_hz, &step[j]) != P25FE_OK) return P25FE_ERR_ARG;
    *n_out = n_keys;
    if (cap < n_keys) return P25FE_ERR_CAPACITY;
    const uint64_t r0 = range_first, r1 = range_first + range_n;
    const __int128 slot = (__int128)B * hop;                         // samples per slot
    for (size_t j = 0; j < n_keys; ++j) {
        // frame f spans [f hop + hop - N, f hop + hop - 1]: from the first sample of the key's first frame to one hop past its last,
        // the margin on both sides (128-bit: any slot numbers)
        const __int128 first = (__int128)keys[j].first_slot * slot + hop - N - (__int128)margin;
        const __int128 end = ((__int128)keys[j].first_slot + (__int128)keys[j].n_slots) * slot + hop + (__int128)margin;   // one past the last
        const uint64_t a = ct_clamp(first, r0, r1), b = ct_clamp(end, r0, r1);
        out[j].abs_first = a; out[j].n = b > a ? b - a : 0;
        out[j].step = step[j]; out[j].ph0 = 0;
    }
    return P25FE_OK;
}

int p25fe_cuts_create(p25fe_tuner_t* tn, const p25fe_cut_t* cuts, size_t n_cuts, size_t* counts_out, size_t* max_count, p25fe_cuts_t** out)
{
    if (out) *out = nullptr;
    if (max_count) *max_count = 0;
    if (!out || !cuts || n_cuts == 0 || n_cuts > P25FE_CUTS_MAX) return P25FE_ERR_ARG;
    for (size_t j = 0; j < n_cuts; ++j)
        if (position_refused(cuts[j].abs_first) || cuts[j].n >= P25FE_MAX_POSITION) return P25FE_ERR_ARG;
    if (!tn || !tn->h || tn->mix != MIX_NCO) return P25FE_ERR_ARG;   // (the tuner is looked at last)
    p25fe_t* h = tn->h;
    const int L = tn->L, M = tn->M;
    RsArgs geo;
    rs_fill_args(tn, geo, nullptr, 0, 0, 0, 0, nullptr, 0, 0);       // the sub-tile: a function of (L, M, T) alone
    const size_t per_wg = (size_t)geo.tile * RS_SUBS;
    std::vector<CutRec> rec(n_cuts);
    std::vector<int> first(n_cuts + 1, 0);
    p25fe_cuts* ct = new (std::nothrow) p25fe_cuts;
    if (!ct) return P25FE_ERR_NOMEM;
    ct->tn = tn; ct->device = tn->device; ct->J = n_cuts; ct->cnt.resize(n_cuts);
    ct->lo = cuts[0].abs_first; ct->hi = cuts[0].abs_first + cuts[0].n;
    for (size_t j = 0; j < n_cuts; ++j) {
        const p25fe_cut_t& c = cuts[j];
        const size_t cnt = p25fe_n_resample(L, M, c.abs_first, (size_t)c.n);
        ct->cnt[j] = cnt;
        ct->max_cnt = std::max(ct->max_cnt, cnt);
        ct->lo = std::min(ct->lo, c.abs_first); ct->hi = std::max(ct->hi, c.abs_first + c.n);
        ct->total_wg += (cnt + per_wg - 1) / per_wg;                 // (each term is below 2^62: 4096 of them do not wrap)
        if (ct->total_wg > (size_t)0x7fffffffu) { delete ct; return P25FE_ERR_ARG; }
        first[j + 1] = (int)ct->total_wg;
        // rs_fill_args' (p0, d0) for the cut's own first sample
        const int ra = (int)(c.abs_first % (uint64_t)M), mr = ra * L / M, ur = mr * M + M - 1;
        rec[j].abs_first = c.abs_first; rec[j].n_out = (long)cnt;
        rec[j].p0 = ur % L; rec[j].d0 = ur / L - ra;
        rec[j].step = c.step; rec[j].ph0 = c.ph0;
    }
    if (hipSetDevice(ct->device) != hipSuccess || ct->d_rec.ensure(rec.size() * sizeof(CutRec)) != hipSuccess ||
        ct->d_first.ensure(first.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(ct->d_rec.p, rec.data(), rec.size() * sizeof(CutRec), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ct->d_first.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        h->last_hip = (int)hipGetLastError(); delete ct; return P25FE_ERR_HIP;
    }
    if (counts_out) std::copy(ct->cnt.begin(), ct->cnt.end(), counts_out);
    if (max_count) *max_count = ct->max_cnt;
    *out = ct;
    return P25FE_OK;
}

void p25fe_cuts_destroy(p25fe_cuts_t* ct) { rs_destroy(ct); }

int p25fe_cuts_dev(p25fe_cuts_t* ct, const void* d_iq, int fmt, size_t n_hist, size_t n, uint64_t abs_first, float* d_out,
                   size_t out_stride, void* stream)
{
    if (!ct || !ct->tn || !ct->tn->h || !wide_fmt_known(fmt)) return P25FE_ERR_ARG;
    p25fe_tuner* tn = ct->tn;
    p25fe_t* h = tn->h;
    if (rs_pointers_refused(tn, d_iq, fmt, 0, abs_first, d_out)) return P25FE_ERR_ARG;
    // every cut lies inside the call's range (the hull does), every row holds its cut, and row J - 1 is addressable
    if (ct->lo < abs_first || ct->hi - abs_first > (uint64_t)n) return P25FE_ERR_ARG;
    if (out_stride < ct->max_cnt || out_stride >= P25FE_MAX_POSITION / P25FE_CUTS_MAX) return P25FE_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (ct->total_wg == 0) return P25FE_OK;
    TuneArgs ta;
    rs_fill_args(tn, ta.r, d_iq, 0, n_hist, n, abs_first, d_out, out_stride, 0);   // (p0, d0, n_out: the records')
    ta.ch = nullptr; ta.K = 1; ta.rot_off = tn->rot_off; ta.abs_first = abs_first;
    CutArgs ca;
    ca.rec = ct->d_rec.as<CutRec>(); ca.first_wg = ct->d_first.as<int>(); ca.rot = tn->d_rot.as<float2>(); ca.J = (int)ct->J;
    const dim3 grid((unsigned)ct->total_wg);
    const WideConv cv = wide_conv_of(h);
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();                                        // the check below is for THIS launch
    if (fmt == P25FE_FMT_CF32) ct_launch_as<P25FE_FMT_CF32, false>(grid, tn->lds, st, ta, ca, cv);
    else if (fmt == P25FE_FMT_S16) ct_launch_as<P25FE_FMT_S16, false>(grid, tn->lds, st, ta, ca, cv);
    else if (cv.lut) ct_launch_as<P25FE_FMT_U8, true>(grid, tn->lds, st, ta, ca, cv);
    else ct_launch_as<P25FE_FMT_U8, false>(grid, tn->lds, st, ta, ca, cv);
    HIPCHK(h, hipGetLastError());
    return P25FE_OK;
}

}  // extern "C"

#endif
