// The host-only functions of the tuner's NCO channels (docs/SPEC.md 3.0d) under AddressSanitizer + UBSan: p25fe_nco_step,
// p25fe_nco_factor and the argument checks of p25fe_nco_create that answer before any device is touched.  Links the host-side
// sanitizer build of the library (make asan); no HIP runtime call is reached, no GPU is needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "tune nco host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    int32_t step = -7;
    CHECK(p25fe_nco_step(2500000u, 137500.0, &step) == P25FE_OK && step == 236223201);
    CHECK(p25fe_nco_step(2048000u, 8000.0, &step) == P25FE_OK && step == (1 << 24));
    CHECK(p25fe_nco_step(2048000u, -8000.0, &step) == P25FE_OK && step == -(1 << 24));
    CHECK(p25fe_nco_step(2500000u, 0.0, &step) == P25FE_OK && step == 0);
    CHECK(p25fe_nco_step(2500000u, 1250000.0, &step) == P25FE_OK && step == imin);       // +2^31 wraps: the conversion is defined
    CHECK(p25fe_nco_step(2500000u, -1250000.0, &step) == P25FE_OK && step == imin);
    CHECK(p25fe_nco_step(4294967295u, 2147483647.5, &step) == P25FE_OK && step == imin);
    CHECK(p25fe_nco_step(4294967295u, 0.4, &step) == P25FE_OK && step == 0);
    CHECK(p25fe_nco_step(1u, 0.5, &step) == P25FE_OK && step == imin);
    CHECK(p25fe_nco_step(2500000u, 135289.3, &step) == P25FE_OK && step > 0);
    step = -7;
    const double bad[] = {1250000.001, -1250000.001, 1e300, -1e300, std::numeric_limits<double>::infinity(),
                          -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(),
                          std::numeric_limits<double>::max(), std::numeric_limits<double>::lowest()};
    for (double off : bad) CHECK(p25fe_nco_step(2500000u, off, &step) == P25FE_ERR_ARG && step == -7);
    CHECK(p25fe_nco_step(0u, 0.0, &step) == P25FE_ERR_ARG && p25fe_nco_step(2500000u, 0.0, nullptr) == P25FE_ERR_ARG);

    // the factor: every wrapping product and shift at the extremes of both arguments; unit modulus to fp32
    const int32_t steps[] = {0, 1, -1, imax, imin, 1 << 24, -(1 << 24), 127 << 24, 236223201, -3527459, (1 << 23), (1 << 23) - 1, -(1 << 23)};
    const uint64_t pos[] = {0, 1, 255, 256, 12345, 0xffffffffull, 0x100000000ull, 0x100000001ull, (1ull << 56) - 1, (1ull << 62) - 1,
                            std::numeric_limits<uint64_t>::max()};
    for (int32_t s : steps)
        for (uint64_t n : pos) {
            float cs[2] = {-9.0f, -9.0f};                             // exactly the room the pair needs
            CHECK(p25fe_nco_factor(s, n, cs) == P25FE_OK);
            CHECK(std::fabs(cs[0] * cs[0] + cs[1] * cs[1] - 1.0f) < 1e-6f);
            if (s == 0 || n == 0) CHECK(cs[0] == 1.0f && cs[1] == 0.0f);
        }
    float q[2];
    CHECK(p25fe_nco_factor(1 << 30, 1, q) == P25FE_OK && q[1] == 1.0f && std::fabs(q[0]) < 1e-7f);       // a quarter turn
    CHECK(p25fe_nco_factor(imin, 1, q) == P25FE_OK && q[0] == -1.0f && std::fabs(q[1]) < 1e-7f);        // half a turn
    CHECK(p25fe_nco_factor(imin, 2, q) == P25FE_OK && q[0] == 1.0f && q[1] == 0.0f);
    CHECK(p25fe_nco_factor(1, 0, nullptr) == P25FE_ERR_ARG);

    // create: every check answers with no handle (the last one BECAUSE there is none)
    std::vector<float> taps(12 * 84, 0.01f);
    std::vector<int32_t> st(257, 1);
    st[1] = imin; st[2] = imax; st[3] = 0; st[4] = -1;
    p25fe_tuner_t* tn = reinterpret_cast<p25fe_tuner_t*>(1);
    const int ks[] = {0, -1, 257, imax, imin};
    for (int k : ks) { CHECK(p25fe_nco_create(nullptr, 12, 125, 84, taps.data(), k, st.data(), &tn) == P25FE_ERR_ARG); CHECK(tn == nullptr); }
    const int32_t shapes[][3] = {{2, 4, 8}, {10, 10, 8}, {8, 125, 513}, {0, 10, 8}, {33, 34, 8}, {1, 1025, 8}, {1, 10, 0}, {1, 10, 1025}};
    for (const auto& s : shapes) CHECK(p25fe_nco_create(nullptr, s[0], s[1], s[2], taps.data(), 1, st.data(), &tn) == P25FE_ERR_ARG);
    std::vector<float> nan_taps(taps);
    nan_taps.back() = std::numeric_limits<float>::quiet_NaN();       // the LAST tap: the check reads exactly L * T of them
    CHECK(p25fe_nco_create(nullptr, 12, 125, 84, nan_taps.data(), 1, st.data(), &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_nco_create(nullptr, 12, 125, 84, nullptr, 1, st.data(), &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_nco_create(nullptr, 12, 125, 84, taps.data(), 1, nullptr, &tn) == P25FE_ERR_ARG);
    CHECK(p25fe_nco_create(nullptr, 12, 125, 84, taps.data(), 1, st.data(), nullptr) == P25FE_ERR_ARG);
    tn = reinterpret_cast<p25fe_tuner_t*>(1);
    CHECK(p25fe_nco_create(nullptr, 12, 125, 84, taps.data(), 256, st.data(), &tn) == P25FE_ERR_ARG && tn == nullptr);   // all valid, no handle
    std::puts("tune nco host driver ok");
    return 0;
}
