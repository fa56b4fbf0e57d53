// CPU walk of K1's segment geometry (p25k::SegGeo, p25fe_kernels.hip): the one set of functions that the host's launch planner
// (k1_plan) and the kernel (frontend_body) both call.  No HIP runtime call, no GPU; built host-only, with AddressSanitizer and
// UBSan, and run by tests/test_sanitizers.py.  Exit code 0 and the last line "k1 geometry driver ok" = pass.
//
// What the project relies on, asserted for every case of the grid in main():
//   * the segments start(k) .. end(k), k in [0, count), are ascending, disjoint and cover exactly [m_begin, n_out), and subs(k)
//     sub-tiles compute exactly the outputs of segment k (halo form: after the first sub-tile's dropped halo);
//   * a time shard's HEAD and MAIN launches partition [0, count); every MAIN segment's first input sample lies inside the
//     owned samples (>= 0), the last HEAD segment's does not; head_end is where MAIN's first segment starts;
//   * with lead segments, HEAD is made of one-sub-tile segments only;
//   * planar_ok() holds exactly when the planar epilogue's stores are aligned as they assume (see planar_aligned below).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../p25rx_amd/csrc/p25fe_kernels.hip"

using p25k::SegGeo;

static long n_checked = 0;
#define EXPECT(cond) do { ++n_checked; if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d): pro %d sub %d subs %d segh %d lead %d m_begin %ld n_out %ld\n", \
    #cond, __LINE__, (int)g.pro, g.sub, g.subs_per_seg, g.segh, g.lead_segs, g.m_begin, g.n_out); return false; } } while (0)

// Length of segment k, from the two forms' definitions (not from SegGeo's formulas): its sub-tiles' outputs; the halo form's
// first sub-tile drops segh of them.
static long seg_outputs(const SegGeo& g, long k) { return (long)g.subs(k) * g.sub - (g.pro ? 0 : g.segh); }

// What the kernel's planar stores assume, in this file's own words.  Prologue form: a sub-tile is stored as ONE 320-float block
// (ten whole rows, ten sign words), so every sub-tile of every segment starts on a block boundary of the layout at or behind
// position 0.  Halo form: a sign byte (8 symbols x 10 samples = 80 outputs) is written by one workgroup only, so every segment
// boundary is a multiple of 80 at or behind position 0.  Looked at over the first segments of an unbounded range.
static bool planar_aligned(const SegGeo& g, long pl_shift)
{
    long pos = g.m_begin + pl_shift;
    if (pos < 0) return false;
    for (long k = 0; k < g.lead_segs + 3; ++k) {
        if (g.pro) {
            for (int s = 0; s < g.subs(k); ++s)
                if ((pos + (long)s * g.sub) % 320 != 0) return false;
        } else if (pos % 80 != 0) return false;
        pos += seg_outputs(g, k);
    }
    return g.pro ? true : pos % 80 == 0;
}

// The segments of one range.  `walk`: visit every segment (small ranges) or a sample of them (ranges of up to 2^31 segments).
static bool check_tiling(const SegGeo& g, bool walk, std::mt19937_64& rng)
{
    const long n = g.count(g.n_out - g.m_begin);
    EXPECT(n >= 1 && g.start(0) == g.m_begin && g.end(n - 1) == g.n_out && g.start(n - 1) < g.n_out);
    EXPECT(g.lead_len() == (g.pro ? g.sub : g.sub - g.segh) && g.seg_len() == g.lead_len() + (long)(g.subs_per_seg - 1) * g.sub);
    auto seg_ok = [&](long k, long pos) {                            // segment k starts at pos and is what its sub-tiles compute
        EXPECT(g.start(k) == pos && g.end(k) > g.start(k) && g.len(k) == seg_outputs(g, k));
        EXPECT(g.end(k) == (pos + seg_outputs(g, k) < g.n_out ? pos + seg_outputs(g, k) : g.n_out));
        EXPECT(k == n - 1 || g.start(k + 1) == g.end(k));
        EXPECT(g.subs(k) == (k < g.lead_segs ? 1 : g.subs_per_seg));
        // the kernel's sub-tile loop: first window at start - (halo form: segh), one sub-tile further each time, until end
        const long dlo = g.start(k) - (g.pro ? 0 : g.segh);
        EXPECT(dlo + (long)g.subs(k) * g.sub >= g.end(k));
        return true;
    };
    if (walk) {
        long pos = g.m_begin;
        for (long k = 0; k < n; ++k) {
            if (!seg_ok(k, pos)) return false;
            pos += seg_outputs(g, k);
        }
        EXPECT(pos >= g.n_out && pos - seg_outputs(g, n - 1) < g.n_out);
    } else {
        const long lead_out = g.lead_segs * g.lead_len();
        for (int i = 0; i < 24; ++i) {
            const long k = i < 8 ? (i < n ? i : n - 1) : (i < 16 ? (n - 1 - (i - 8) >= 0 ? n - 1 - (i - 8) : 0) : (long)(rng() % (uint64_t)n));
            const long pos = g.m_begin + (k < g.lead_segs ? k * g.lead_len() : lead_out + (k - g.lead_segs) * seg_outputs(g, g.lead_segs));
            if (!seg_ok(k, pos)) return false;
        }
    }
    for (long pl_shift : {320L, 322L}) EXPECT(g.planar_ok(pl_shift) == planar_aligned(g, pl_shift));
    return true;
}

// A time shard's two launches over the range: HEAD = (seg_first 0, seg_count k_min), MAIN = (k_min, n - k_min)  (K1Args)
static bool check_parts(const SegGeo& g, int front, long o0, int t1, bool walk, std::mt19937_64& rng)
{
    const long n = g.count(g.n_out - g.m_begin);
    const long k_min = g.head_count(n, front, o0, t1);
    const long head_first = 0, head_count = k_min, main_first = k_min, main_count = n - k_min;
    EXPECT(head_count >= 0 && main_count >= 0 && head_first + head_count == main_first && main_first + main_count == n);
    auto first_in = [&](long k) { return SegGeo::first_input(g.start(k) - front, o0, t1); };
    EXPECT(SegGeo::first_input(7, o0, t1) == o0 + 5 * 7 - (t1 - 1));
    if (walk) for (long k = main_first; k < n; ++k) EXPECT(first_in(k) >= 0);
    else if (main_count > 0) EXPECT(first_in(main_first) >= 0 && first_in(n - 1) >= 0 && first_in(main_first + (long)(rng() % (uint64_t)main_count)) >= 0);
    if (head_count > 0) EXPECT(first_in(k_min - 1) < 0);
    for (long k = 0; k < k_min; ++k) EXPECT(g.in_head(k, front, o0, t1));
    // head_end (K1Plan): the planar position, counted from the range's first output, where MAIN's first segment starts
    long head_outputs = 0;
    for (long k = 0; k < k_min; ++k) head_outputs += seg_outputs(g, k);
    EXPECT(g.start(k_min) - g.m_begin == head_outputs);
    if (g.subs_per_seg > 1 && g.lead_segs < 64) {                     // the rule: lead segments up to the first one that needs no halo
        EXPECT(k_min == g.lead_segs);
        for (long k = 0; k < k_min; ++k) EXPECT(g.subs(k) == 1);
    } else if (g.subs_per_seg == 1) EXPECT(g.lead_segs == 0);
    return true;
}

int main()
{
    std::mt19937_64 rng(25);
    const long MAX_RANGE_BB = 0x7ff00000L * 10;                      // the planar scratch's ceiling (p25fe_api.hip)
    long n_cases = 0;
    for (int pro = 0; pro < 2; ++pro)
    for (int sub : {192, 320})
    for (int subs : {1, 2, 3, 9, 12})
    for (int segh : {80, 160})
    for (long m_begin : {0L, -320L, -322L, -240L, -242L}) {         // linear; prologue form, planar (+ lookahead); halo form, planar
        SegGeo g{pro != 0, sub, subs, segh, 0, m_begin, 0};
        const long three = 4 * g.lead_len() + 3 * g.seg_len() + 7;  // a little past three segments behind the lead ones
        // (the segments of a range depend on the filters and on o0 only through lead_segs: each (lead_segs, total) is walked once)
        std::vector<char> walked((size_t)65 * (size_t)(three + 1), 0);
        auto tiling_once = [&](long total) {
            char& w = walked[(size_t)g.lead_segs * (size_t)(three + 1) + (size_t)total];
            if (w) return true;
            w = 1;
            return check_tiling(g, true, rng);
        };
        // a large range: around the planar ceiling, segment counts around 2^31 / C for C = 1, 2, 3, 16, 192, anything
        auto large_total = [&](int i) {
            static const long C[] = {1, 2, 3, 16, 192};
            const long jitter = (long)(rng() % 4001);
            const long total = i < 4 ? MAX_RANGE_BB - m_begin - i * jitter
                             : i < 9 ? ((1L << 31) / C[i - 4]) * g.seg_len() + jitter - 2000
                             : 1 + (long)(rng() % (uint64_t)((1L << 31) * g.seg_len()));
            return total < 1 ? 1 : total;
        };
        // K1_ALL, and a chunk: no lead segments, no split
        for (long total = 1; total <= three + 12; ++total, ++n_cases) {
            g.n_out = m_begin + (total <= three ? total : large_total((int)(total - three - 1)));
            if (!(total <= three ? tiling_once(total) : check_tiling(g, false, rng))) return 1;
        }
        // a time shard's HEAD and MAIN
        for (int t1 : {31, 64}) for (int t2 : {41, 64}) for (int t3 : {1, 10, 17, 64})
        for (long o0 = 0; o0 < 5; ++o0) {
            const int front = g.front(t3, t2);
            if (front != (g.pro ? t3 + t2 - 1 : g.segh)) { std::fprintf(stderr, "FAILED: front\n"); return 1; }
            if (!g.pro && (t2 != 41 || t3 != 1)) continue;              // (halo form: the same front, so the same cases, for every t2 and t3)
            for (long total = 1; total <= three + 12; ++total, ++n_cases) {
                const bool small = total <= three;
                g.n_out = m_begin + (small ? total : large_total((int)(total - three - 1)));
                g.lead_segs = 0;
                if (subs > 1) g.set_lead(front, o0, t1);            // the planner's rule (k1_plan)
                if (g.lead_segs < 0 || g.lead_segs > 64) { std::fprintf(stderr, "FAILED: lead_segs\n"); return 1; }
                if (!(small ? tiling_once(total) : check_tiling(g, false, rng)) || !check_parts(g, front, o0, t1, small, rng)) return 1;
            }
            g.lead_segs = 0;
        }
    }
    std::printf("%ld ranges, %ld assertions\nk1 geometry driver ok\n", n_cases, n_checked);
    return 0;
}
