// The host-only functions of the tuner's cuts (docs/SPEC.md 3.0j) under AddressSanitizer + UBSan: p25fe_cuts_from_keys and the
// argument checks of p25fe_cuts_create that answer before any device is touched.  Links the host-side sanitizer build of the
// library (make asan); no HIP runtime call is reached, no GPU is needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "tune cuts host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static p25fe_waterfall_key_t key(int32_t r, uint64_t first, uint64_t n, double centre, double off)
{
    p25fe_waterfall_key_t k{};
    k.raster_index = r; k.first_slot = first; k.n_slots = n; k.centre_hz = centre; k.offset_hz = off; k.peak_db_over_floor = 30.0;
    return k;
}

int main()
{
    static_assert(sizeof(p25fe_cut_t) == 24 && sizeof(p25fe_waterfall_key_t) == 48, "the records' sizes");
    const uint64_t u62 = 1ull << 62, umax = std::numeric_limits<uint64_t>::max();
    const int32_t imin = std::numeric_limits<int32_t>::min();
    // from_keys: exactly the room the cuts need (the heap's red zones sit on both sides), slot numbers at every extreme
    std::vector<p25fe_waterfall_key_t> keys = {
        key(1, 0, 2, 12500.0, 0.0), key(1, 60, 2, 12500.0, 0.0), key(1, 4, 3, 12500.0, 0.0), key(-33, 0, 51, -412500.0, 1871.3),
        key(7, umax, umax, 87500.0, 1.0), key(7, u62, 1, -87500.0, -1.0), key(0, umax, 0, 0.0, 0.0), key(100, 3, umax, 1250000.0, 0.0)};
    std::vector<p25fe_cut_t> cuts(keys.size());
    size_t n = 99;
    CHECK(p25fe_cuts_from_keys(keys.data(), keys.size(), 4096, 2048, 6, 2500000u, 0, 0, 625000, cuts.data(), cuts.size(), &n) == P25FE_OK);
    CHECK(n == keys.size());
    CHECK(cuts[0].abs_first == 0 && cuts[0].n == 2 * 12288 + 2048 && cuts[0].step == 21474836 && cuts[0].ph0 == 0);
    CHECK(cuts[1].abs_first == 625000 && cuts[1].n == 0);
    CHECK(cuts[2].abs_first == 4 * 12288 - 2048 && cuts[2].n == 3 * 12288 + 4096);
    CHECK(cuts[3].abs_first == 0 && cuts[3].n == 625000);
    CHECK(cuts[4].n == 0 && cuts[5].n == 0 && cuts[6].n == 0 && cuts[4].abs_first == 625000);
    CHECK(cuts[7].abs_first == 3 * 12288 - 2048 && cuts[7].n == 625000 - cuts[7].abs_first && cuts[7].step == imin);
    // the largest survey shape and margin, a range at the top of the positions
    CHECK(p25fe_cuts_from_keys(keys.data(), keys.size(), 4096, 4096, 1u << 20, 4294967295u, u62 - 1, u62 - 1, u62 - 1, cuts.data(),
                               cuts.size(), &n) == P25FE_OK);
    for (const p25fe_cut_t& c : cuts) CHECK(c.abs_first >= u62 - 1 && c.abs_first + c.n <= 2 * (u62 - 1));
    CHECK(p25fe_cuts_from_keys(keys.data(), keys.size(), 1024, 8, 1, 1u, 0, 5007, 0, cuts.data(), cuts.size(), &n) == P25FE_ERR_ARG);   // 12.5 kHz at 1 Hz
    // refusals: nothing is written
    std::vector<p25fe_cut_t> mark(2, p25fe_cut_t{5, 5, -7, 5});
    const auto untouched = [&] { return mark[0].step == -7 && mark[1].step == -7 && mark[0].n == 5; };
    const int32_t bad_n[] = {0, 512, 2048, 4095, 8192, -4096, imin}, bad_hop[] = {0, 4, 12, 2047, 3000, 8192, -8, imin};
    for (int32_t N : bad_n) CHECK(p25fe_cuts_from_keys(keys.data(), 2, N, 8, 6, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG && n == 0);
    for (int32_t h : bad_hop) CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, h, 6, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
    const uint32_t bad_b[] = {0u, (1u << 20) + 1u, 4294967295u};
    for (uint32_t B : bad_b) CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, B, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 0u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
    const uint64_t big[] = {u62, umax};
    for (uint64_t b : big) {
        CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, b, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
        CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, b, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
        CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, b, mark.data(), 2, &n) == P25FE_ERR_ARG);
    }
    const double bad_f[] = {1250000.001, -1250000.001, 1e300, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (double f : bad_f) {
        std::vector<p25fe_waterfall_key_t> k2 = {keys[0], key(3, 1, 1, f, 0.0)};
        CHECK(p25fe_cuts_from_keys(k2.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG && n == 0);
        k2[1] = key(3, 1, 1, 0.0, f);
        CHECK(p25fe_cuts_from_keys(k2.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG && n == 0);
    }
    CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, mark.data(), 2, nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_from_keys(nullptr, 2, 4096, 2048, 6, 2500000u, 0, 0, 100, mark.data(), 2, &n) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, nullptr, 2, &n) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, mark.data(), 1, &n) == P25FE_ERR_CAPACITY && n == 2);
    CHECK(p25fe_cuts_from_keys(keys.data(), 2, 4096, 2048, 6, 2500000u, 0, 0, 100, nullptr, 0, &n) == P25FE_ERR_CAPACITY && n == 2);
    CHECK(untouched());
    CHECK(p25fe_cuts_from_keys(nullptr, 0, 4096, 2048, 6, 2500000u, 0, 0, 100, nullptr, 0, &n) == P25FE_OK && n == 0);

    // create: every check answers with no tuner (the last one BECAUSE there is none)
    p25fe_cuts_t* ct = reinterpret_cast<p25fe_cuts_t*>(1);
    size_t mx = 77;
    std::vector<p25fe_cut_t> list(P25FE_CUTS_MAX + 1, p25fe_cut_t{100, 5000, 12345, 0});
    CHECK(p25fe_cuts_create(nullptr, list.data(), 0, nullptr, &mx, &ct) == P25FE_ERR_ARG && ct == nullptr && mx == 0);
    ct = reinterpret_cast<p25fe_cuts_t*>(1);
    CHECK(p25fe_cuts_create(nullptr, list.data(), P25FE_CUTS_MAX + 1, nullptr, nullptr, &ct) == P25FE_ERR_ARG && ct == nullptr);
    CHECK(p25fe_cuts_create(nullptr, list.data(), umax, nullptr, nullptr, &ct) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_create(nullptr, nullptr, 1, nullptr, nullptr, &ct) == P25FE_ERR_ARG);
    CHECK(p25fe_cuts_create(nullptr, list.data(), 1, nullptr, nullptr, nullptr) == P25FE_ERR_ARG);
    const p25fe_cut_t bad_cut[] = {{u62, 1, 0, 0}, {5, u62, 0, 0}, {umax, umax, 0, 0}};
    for (const p25fe_cut_t& b : bad_cut) {
        std::vector<p25fe_cut_t> l2(list.begin(), list.begin() + 3);
        l2.back() = b;                                               // the LAST cut: the check reads exactly n_cuts of them
        CHECK(p25fe_cuts_create(nullptr, l2.data(), l2.size(), nullptr, nullptr, &ct) == P25FE_ERR_ARG);
    }
    std::vector<size_t> counts(P25FE_CUTS_MAX, 5);
    list[1] = p25fe_cut_t{u62 - 1, u62 - 1, imin, 4294967295u};
    list[2] = p25fe_cut_t{0, 0, 0, 0};
    ct = reinterpret_cast<p25fe_cuts_t*>(1);
    CHECK(p25fe_cuts_create(nullptr, list.data(), P25FE_CUTS_MAX, counts.data(), &mx, &ct) == P25FE_ERR_ARG && ct == nullptr);   // all valid, no tuner
    CHECK(counts[0] == 5 && mx == 0);
    CHECK(p25fe_cuts_dev(nullptr, nullptr, P25FE_FMT_CF32, 0, 0, 0, nullptr, 0, nullptr) == P25FE_ERR_ARG);
    p25fe_cuts_destroy(nullptr);
    std::puts("tune cuts host driver ok");
    return 0;
}
