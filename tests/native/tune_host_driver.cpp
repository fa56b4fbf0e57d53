// The tuner's host-only functions (docs/SPEC.md 3.0c) under AddressSanitizer + UBSan: p25fe_tuner_freq, p25fe_tuner_rotator and the
// argument checks of p25fe_tuner_create / _reset / p25fe_tune / p25fe_tune_dev that answer before any device is touched.  Links the
// host-side sanitizer build of the library (make asan); no HIP runtime call is reached, no GPU is needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "tune host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    int32_t num = -7, den = -7;
    CHECK(p25fe_tuner_freq(2500000u, 137500, &num, &den) == P25FE_OK && num == 11 && den == 200);
    CHECK(p25fe_tuner_freq(2048000u, -412500, &num, &den) == P25FE_OK && num == -825 && den == 4096);
    CHECK(p25fe_tuner_freq(10000000u, 3012500, &num, &den) == P25FE_OK && num == 241 && den == 800);
    CHECK(p25fe_tuner_freq(2500000u, 0, &num, &den) == P25FE_OK && num == 0 && den == 1);
    CHECK(p25fe_tuner_freq(2048000u, 6250, &num, &den) == P25FE_OK && den == 8192);
    CHECK(p25fe_tuner_freq(2048000u, 3125, &num, &den) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_freq(0u, 0, &num, &den) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_freq(4294967295u, 2147483647, &num, &den) == P25FE_ERR_ARG);       // in range, but the denominator is 2^32 - 1
    const int64_t extremes[] = {std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), -1250001, 1250001};
    for (int64_t off : extremes) CHECK(p25fe_tuner_freq(2500000u, off, &num, &den) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_freq(2500000u, 0, nullptr, &den) == P25FE_ERR_ARG && p25fe_tuner_freq(2500000u, 0, &num, nullptr) == P25FE_ERR_ARG);

    const int32_t dens[] = {1, 2, 3, 200, 4096, 8192};
    for (int32_t d : dens) {
        std::vector<float> cs(2 * (size_t)d, -9.0f);                 // exactly the room the table needs: a write past it is caught
        CHECK(p25fe_tuner_rotator(d, cs.data(), cs.size()) == P25FE_OK);
        CHECK(cs[0] == 1.0f && cs[(size_t)d] == 0.0f && !std::signbit(cs[(size_t)d]));
        for (int32_t i = 0; i < d; ++i) CHECK(std::fabs(cs[i] * cs[i] + cs[d + i] * cs[d + i] - 1.0f) < 1e-6f);
        CHECK(p25fe_tuner_rotator(d, cs.data(), cs.size() - 1) == P25FE_ERR_CAPACITY);
        CHECK(p25fe_tuner_rotator(d, nullptr, 0) == P25FE_ERR_CAPACITY);
    }
    float one[2];
    CHECK(p25fe_tuner_rotator(0, one, 2) == P25FE_ERR_ARG && p25fe_tuner_rotator(-5, one, 2) == P25FE_ERR_ARG &&
          p25fe_tuner_rotator(8193, one, 2) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_rotator(std::numeric_limits<int32_t>::max(), one, 2) == P25FE_ERR_ARG);

    // create: every check answers with no handle (the last one BECAUSE there is none)
    std::vector<float> taps(12 * 84, 0.01f);
    std::vector<int32_t> nums(257, 1), dd(257, 200);
    p25fe_tuner_t* tn = reinterpret_cast<p25fe_tuner_t*>(1);
    const int ks[] = {0, -1, 257, std::numeric_limits<int32_t>::max()};
    for (int k : ks) { CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), k, nums.data(), dd.data(), &tn) == P25FE_ERR_ARG); CHECK(tn == nullptr); }
    const int32_t bad[][2] = {{1, 0}, {1, 8193}, {0, -1}, {2, 4}, {0, 2}, {3, 5}, {-3, 5}, {101, 200}, {std::numeric_limits<int32_t>::min(), 8192},
                              {std::numeric_limits<int32_t>::max(), 8192}, {1, std::numeric_limits<int32_t>::max()}, {1, std::numeric_limits<int32_t>::min()}};
    for (const auto& b : bad) {
        const int32_t n2[2] = {0, b[0]}, d2[2] = {1, b[1]};           // the second channel is the bad one: every entry is looked at
        CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), 2, n2, d2, &tn) == P25FE_ERR_ARG);
    }
    const int32_t shapes[][3] = {{2, 4, 8}, {10, 10, 8}, {8, 125, 513}, {0, 10, 8}, {33, 34, 8}, {1, 1025, 8}, {1, 10, 0}, {1, 10, 1025}};
    for (const auto& s : shapes) CHECK(p25fe_tuner_create(nullptr, s[0], s[1], s[2], taps.data(), 1, nums.data(), dd.data(), &tn) == P25FE_ERR_ARG);
    std::vector<float> nan_taps(taps);
    nan_taps.back() = std::numeric_limits<float>::quiet_NaN();       // the LAST tap: the check reads exactly L * T of them
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, nan_taps.data(), 1, nums.data(), dd.data(), &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, nullptr, 1, nums.data(), dd.data(), &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), 1, nullptr, dd.data(), &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), 1, nums.data(), nullptr, &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), 1, nums.data(), dd.data(), nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_tuner_create(nullptr, 12, 125, 84, taps.data(), 256, nums.data(), dd.data(), &tn) == P25FE_ERR_ARG);    // all valid, no handle
    CHECK(p25fe_tuner_reset(nullptr) == P25FE_ERR_ARG);
    p25fe_tuner_destroy(nullptr);
    size_t n_out = 0;
    CHECK(p25fe_tune(nullptr, nullptr, P25FE_FMT_CF32, 0, nullptr, 0, &n_out) == P25FE_ERR_ARG);
    CHECK(p25fe_tune_dev(nullptr, nullptr, P25FE_FMT_CF32, 0, 0, 0, nullptr, 0, nullptr) == P25FE_ERR_ARG);
    std::puts("tune host driver ok");
    return 0;
}
