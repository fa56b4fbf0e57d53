// The host-only functions of AFC (docs/SPEC.md 3.0e, 3.0f) under AddressSanitizer + UBSan: p25fe_afc_design, p25fe_afc_hz,
// p25fe_afc_factor and the argument checks of p25fe_afc_create, p25fe_afc_measure_dev, p25fe_afc_set_step and p25fe_afc_get_step
// that answer before any device is touched.  Links the host-side sanitizer build of the library (make asan); no HIP runtime call is
// reached, no GPU is needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "afc host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // design: exactly T floats are written, at the limits of D and T
    const int32_t shapes[][2] = {{10, 240}, {2, 1}, {64, 512}, {3, 7}, {10, 2}};
    for (const auto& s : shapes) {
        std::vector<float> taps((size_t)s[1], -9.0f);                 // exactly the room the table needs
        CHECK(p25fe_afc_design(s[0], 7000.0, s[1], taps.data(), taps.size()) == P25FE_OK);
        double sum = 0.0;
        for (float v : taps) { CHECK(std::isfinite(v)); sum += v; }
        CHECK(std::fabs(sum - 1.0) < 1e-5);
        for (size_t k = 0; k < taps.size(); ++k) CHECK(taps[k] == taps[taps.size() - 1 - k]);
        if (s[1] > 1) CHECK(p25fe_afc_design(s[0], 7000.0, s[1], taps.data(), taps.size() - 1) == P25FE_ERR_CAPACITY);
        CHECK(p25fe_afc_design(s[0], 7000.0, s[1], nullptr, taps.size()) == P25FE_ERR_CAPACITY);
    }
    float one[1] = {-9.0f};
    const int32_t bad_shapes[][2] = {{1, 8}, {65, 8}, {0, 8}, {-1, 8}, {imin, 8}, {imax, 8}, {10, 0}, {10, 513}, {10, -1}, {10, imin}, {10, imax}};
    for (const auto& s : bad_shapes) CHECK(p25fe_afc_design(s[0], 7000.0, s[1], one, 1) == P25FE_ERR_ARG);
    const double bad_fc[] = {0.0, -0.0, -1.0, 120000.001, 1e300, inf, -inf, nan, std::numeric_limits<double>::max()};
    for (double fc : bad_fc) CHECK(p25fe_afc_design(10, fc, 1, one, 1) == P25FE_ERR_ARG);
    CHECK(one[0] == -9.0f);
    CHECK(p25fe_afc_design(10, std::numeric_limits<double>::denorm_min(), 1, one, 1) == P25FE_OK && one[0] == 1.0f);

    // hz: the conversions at the extremes of the record's fields
    const int64_t lmin = std::numeric_limits<int64_t>::min(), lmax = std::numeric_limits<int64_t>::max();
    const p25fe_afc_acc_t recs[] = {{1000, 0, 1000, 5}, {0, 1000, 1000, 5}, {-1000, 0, 1000, 5}, {0, -1000, 1000, 5}, {lmin, lmax, lmax, ~0ull},
                                    {lmax, lmin, 1, 0}, {lmin, lmin, lmax, 1}, {3, 4, 5, 1}};
    for (const auto& r : recs) {
        const int32_t ds[] = {2, 10, 64};
        for (int32_t D : ds) {
            double hz = nan, coh = nan;
            CHECK(p25fe_afc_hz(&r, D, &hz, &coh) == P25FE_OK);
            CHECK(std::isfinite(hz) && std::isfinite(coh) && std::fabs(hz) <= 120000.0 / D && coh >= 0.0);
        }
    }
    double hz = -1.0, coh = -1.0;
    CHECK(p25fe_afc_hz(&recs[1], 10, &hz, &coh) == P25FE_OK && std::fabs(hz - 6000.0) < 1e-9 && std::fabs(coh - 1.0) < 1e-12);
    const p25fe_afc_acc_t dead[] = {{1000, 1000, 0, 5}, {1000, 1000, -1, 5}, {1000, 1000, lmin, 5}, {0, 0, 1000, 5}, {0, 0, 0, 0}};
    for (const auto& r : dead) { hz = coh = -1.0; CHECK(p25fe_afc_hz(&r, 10, &hz, &coh) == P25FE_OK && hz == 0.0 && coh == 0.0); }
    hz = coh = -1.0;
    CHECK(p25fe_afc_hz(nullptr, 10, &hz, &coh) == P25FE_ERR_ARG && p25fe_afc_hz(&recs[0], 10, nullptr, &coh) == P25FE_ERR_ARG);
    CHECK(p25fe_afc_hz(&recs[0], 10, &hz, nullptr) == P25FE_ERR_ARG);
    const int32_t bad_d[] = {1, 0, -1, 65, imin, imax};
    for (int32_t D : bad_d) CHECK(p25fe_afc_hz(&recs[0], D, &hz, &coh) == P25FE_ERR_ARG);
    CHECK(hz == -1.0 && coh == -1.0);

    // the factor: every wrapping product and sum at the extremes of the three arguments; unit modulus to fp32
    const int32_t steps[] = {0, 1, -1, imax, imin, 1 << 24, -(1 << 24), 127 << 24, 232387521, -3527459, (1 << 23), (1 << 23) - 1, -(1 << 23)};
    const uint32_t offs[] = {0u, 1u, 0xffffffffu, 0x80000000u, 0x7fffffffu, (1u << 23), (1u << 23) - 1u, 0x12345678u};
    const uint64_t pos[] = {0, 1, 255, 12345, 0xffffffffull, 0x100000000ull, 0x100000001ull, (1ull << 56) - 1, (1ull << 62) - 1,
                            std::numeric_limits<uint64_t>::max()};
    for (int32_t s : steps)
        for (uint32_t p : offs)
            for (uint64_t n : pos) {
                float cs[2] = {-9.0f, -9.0f};                         // exactly the room the pair needs
                CHECK(p25fe_afc_factor(s, p, n, cs) == P25FE_OK);
                CHECK(std::fabs(cs[0] * cs[0] + cs[1] * cs[1] - 1.0f) < 1e-6f);
                if (p == 0) {
                    float q[2];
                    CHECK(p25fe_nco_factor(s, n, q) == P25FE_OK && q[0] == cs[0] && q[1] == cs[1]);
                }
            }
    float q[2];
    CHECK(p25fe_afc_factor(0, 1u << 30, 77, q) == P25FE_OK && q[1] == 1.0f && std::fabs(q[0]) < 1e-7f);      // a quarter turn from ph0 alone
    CHECK(p25fe_afc_factor(imin, 0x80000000u, 1, q) == P25FE_OK && q[0] == 1.0f && q[1] == 0.0f);          // two halves
    CHECK(p25fe_afc_factor(1, 0, 0, nullptr) == P25FE_ERR_ARG);

    // create: every check answers with no handle (the last one BECAUSE there is none)
    std::vector<float> taps(512, 0.01f);
    p25fe_afc_t* afc = reinterpret_cast<p25fe_afc_t*>(1);
    const int32_t bad_create[][3] = {{1, 240, 1}, {65, 240, 1}, {0, 240, 1}, {imin, 240, 1}, {imax, 240, 1}, {10, 0, 1}, {10, 513, 1}, {10, imin, 1},
                                     {10, imax, 1}, {10, 240, 0}, {10, 240, 257}, {10, 240, imin}, {10, 240, imax}};
    for (const auto& s : bad_create) {
        afc = reinterpret_cast<p25fe_afc_t*>(1);
        CHECK(p25fe_afc_create(nullptr, s[0], s[1], taps.data(), s[2], &afc) == P25FE_ERR_ARG && afc == nullptr);
    }
    std::vector<float> nan_taps(240, 0.01f);
    nan_taps.back() = std::numeric_limits<float>::quiet_NaN();        // the LAST tap: the check reads exactly T of them
    CHECK(p25fe_afc_create(nullptr, 10, 240, nan_taps.data(), 1, &afc) == P25FE_ERR_ARG);
    nan_taps.back() = std::numeric_limits<float>::infinity();
    CHECK(p25fe_afc_create(nullptr, 10, 240, nan_taps.data(), 1, &afc) == P25FE_ERR_ARG);
    CHECK(p25fe_afc_create(nullptr, 10, 240, nullptr, 1, &afc) == P25FE_ERR_ARG);
    CHECK(p25fe_afc_create(nullptr, 10, 240, taps.data(), 1, nullptr) == P25FE_ERR_ARG);
    afc = reinterpret_cast<p25fe_afc_t*>(1);
    CHECK(p25fe_afc_create(nullptr, 64, 512, taps.data(), 256, &afc) == P25FE_ERR_ARG && afc == nullptr);    // all valid, no handle
    p25fe_afc_destroy(nullptr);

    // measure, set_step, get_step: no object
    p25fe_afc_acc_t acc[2] = {};
    CHECK(p25fe_afc_measure_dev(nullptr, taps.data(), 256, 0, 256, 0, 24, acc, nullptr) == P25FE_ERR_ARG);
    CHECK(acc[0].n == 0 && acc[1].n == 0);
    int32_t step = -7;
    uint32_t ph0 = 7;
    CHECK(p25fe_afc_set_step(nullptr, 0, 5, 0, nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_afc_get_step(nullptr, 0, &step, &ph0) == P25FE_ERR_ARG && step == -7 && ph0 == 7);
    std::puts("afc host driver ok");
    return 0;
}
