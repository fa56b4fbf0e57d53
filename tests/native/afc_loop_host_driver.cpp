// The host-only functions of the AFC loop (docs/SPEC.md 3.0g) under AddressSanitizer + UBSan: p25fe_track_step (the law, the same
// function the kernel k_afc_loop compiles), p25fe_track_hz and the argument checks of the loop's entry points that answer before
// any device is touched.  Links the host-side sanitizer build of the library (make asan); no HIP runtime call is reached, no GPU
// is needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "afc loop host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    const int64_t lmin = std::numeric_limits<int64_t>::min(), lmax = std::numeric_limits<int64_t>::max();
    const p25fe_track_cfg_t good = {24, 24576, 65536, 1 << 24, 1 << 24, 0, 600};

    // the law at the extremes of every field: each wrapping sum, each shift, the division and both clamps
    const int64_t vals[] = {0, 1, -1, 3, -4, 65535, 65536, -65537, (1ll << 31), -(1ll << 31) - 1, (1ll << 59), (1ll << 60) - 1, 1ll << 60,
                            -(1ll << 61), (1ll << 62), lmax, lmin, lmin + 1};
    const uint64_t ns[] = {0, 599, 600, ~0ull};
    const uint64_t ats[] = {0, 1, 0xffffffffull, 0x100000000ull, (1ull << 40) + 5, (1ull << 62) - 1, ~0ull};
    const int32_t steps[] = {0, 1, -1, imax, imin, imax - 500, imin + 500, 232387521};
    const p25fe_track_cfg_t cfgs[] = {good, {0, 0, 65536, imax, imax, 0, 1}, {40, 32768, 1, 1, 1, 0, ~0ull}, {24, 0, 32768, 100, 1000, 0, 1}};
    const int32_t ratios[][3] = {{12, 125, 10}, {24, 25, 10}, {1, 2, 2}, {32, 1023, 64}, {31, 32, 2}};
    unsigned applied = 0, rejected = 0, shorts = 0;
    size_t i = 0;
    for (int64_t re : vals)
        for (int64_t im : vals)
            for (int64_t pw : vals) {
                ++i;
                const p25fe_track_cfg_t& cfg = cfgs[i % 4];
                const int32_t* r = ratios[i % 5];
                const p25fe_afc_acc_t acc = {re, im, pw, ns[i % 4]};
                p25fe_track_state_t st = {steps[i % 8], (uint32_t)(i * 2654435761u), imin, imax, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0};
                const int32_t ref = steps[(i / 8) % 8];
                p25fe_afc_acc_t out_acc = {1, 1, 1, 1};
                p25fe_track_state_t out = st;
                CHECK(p25fe_track_step(&cfg, r[0], r[1], r[2], ref, &acc, &st, ats[i % 7], &out_acc, &out) == P25FE_OK);
                CHECK(out.status >= P25FE_TRACK_SHORT && out.status <= P25FE_TRACK_APPLY);
                if (out.status == P25FE_TRACK_SHORT) {
                    ++shorts;
                    CHECK(out_acc.re == re && out_acc.im == im && out_acc.pow == pw && out_acc.n == acc.n && out.step == st.step && out.ph0 == st.ph0);
                    CHECK(out.n_short == 0 && out.n_applied == 0xffffffffu);
                } else {
                    CHECK(out_acc.re == 0 && out_acc.im == 0 && out_acc.pow == 0 && out_acc.n == 0);
                    if (out.status == P25FE_TRACK_REJECT) { ++rejected; CHECK(out.step == st.step && out.ph0 == st.ph0 && out.n_rejected == 0); }
                    else {
                        ++applied;
                        CHECK(out.n_applied == 0 && std::llabs((long long)out.last_dstep) <= cfg.max_pull);
                        // the phase at abs_at stays: the factor is the same bits
                        float a[2], b[2];
                        CHECK(p25fe_afc_factor(st.step, st.ph0, ats[i % 7], a) == P25FE_OK && p25fe_afc_factor(out.step, out.ph0, ats[i % 7], b) == P25FE_OK);
                        CHECK(a[0] == b[0] && a[1] == b[1]);
                    }
                }
                // in place
                p25fe_afc_acc_t acc2 = acc;
                p25fe_track_state_t st2 = st;
                CHECK(p25fe_track_step(&cfg, r[0], r[1], r[2], ref, &acc2, &st2, ats[i % 7], &acc2, &st2) == P25FE_OK);
                CHECK(st2.step == out.step && st2.ph0 == out.ph0 && st2.last_theta == out.last_theta && st2.status == out.status && acc2.n == out_acc.n);
            }
    CHECK(applied > 100 && rejected > 100 && shorts > 100);
    // known angles: the axes are exact
    const struct { int64_t re, im; int32_t theta; } known[] = {{1000, 0, 0}, {0, 1000, 1 << 30}, {-1000, 0, imin}, {0, -1000, -(1 << 30)},
                                                               {lmax, 0, 0}, {0, lmin, -(1 << 30)}, {1, 1, 1 << 29}, {-(1ll << 62), -(1ll << 62), -(3 << 29)}};
    for (const auto& k : known) {
        const p25fe_track_cfg_t c = {24, 0, 65536, imax, imax, 0, 1};
        const p25fe_afc_acc_t acc = {k.re, k.im, 1, 1};
        p25fe_track_state_t st = {}, out = {};
        p25fe_afc_acc_t oa;
        CHECK(p25fe_track_step(&c, 12, 125, 10, 0, &acc, &st, 0, &oa, &out) == P25FE_OK && out.status == P25FE_TRACK_APPLY);
        CHECK(std::llabs((long long)out.last_theta - (long long)k.theta) <= 1);
    }

    // refusals of the law
    p25fe_afc_acc_t acc = {1000, 0, 1000, 700}, oa = {7, 7, 7, 7};
    p25fe_track_state_t st = {}, out = {7, 7, 7, 7, 7, 7, 7, 7};
    const p25fe_track_cfg_t bad[] = {{-1, 24576, 65536, 1, 1, 0, 600}, {41, 24576, 65536, 1, 1, 0, 600}, {imin, 24576, 65536, 1, 1, 0, 600},
                                     {24, -1, 65536, 1, 1, 0, 600}, {24, 32769, 65536, 1, 1, 0, 600}, {24, imax, 65536, 1, 1, 0, 600},
                                     {24, 24576, 0, 1, 1, 0, 600}, {24, 24576, 65537, 1, 1, 0, 600}, {24, 24576, imin, 1, 1, 0, 600},
                                     {24, 24576, 65536, 0, 1, 0, 600}, {24, 24576, 65536, imin, 1, 0, 600}, {24, 24576, 65536, 1, 0, 0, 600},
                                     {24, 24576, 65536, 1, imin, 0, 600}, {24, 24576, 65536, 1, 1, 1, 600}, {24, 24576, 65536, 1, 1, 0, 0}};
    for (const auto& c : bad) CHECK(p25fe_track_step(&c, 12, 125, 10, 0, &acc, &st, 0, &oa, &out) == P25FE_ERR_ARG);
    const int32_t bad_ratio[][3] = {{0, 125, 10}, {33, 125, 10}, {12, 12, 10}, {12, 1025, 10}, {6, 8, 10}, {imin, 5, 10}, {12, imax, 10},
                                    {12, 125, 1}, {12, 125, 65}, {12, 125, imin}, {12, 125, imax}};
    for (const auto& r : bad_ratio) CHECK(p25fe_track_step(&good, r[0], r[1], r[2], 0, &acc, &st, 0, &oa, &out) == P25FE_ERR_ARG);
    CHECK(p25fe_track_step(nullptr, 12, 125, 10, 0, &acc, &st, 0, &oa, &out) == P25FE_ERR_ARG);
    CHECK(p25fe_track_step(&good, 12, 125, 10, 0, nullptr, &st, 0, &oa, &out) == P25FE_ERR_ARG);
    CHECK(p25fe_track_step(&good, 12, 125, 10, 0, &acc, nullptr, 0, &oa, &out) == P25FE_ERR_ARG);
    CHECK(p25fe_track_step(&good, 12, 125, 10, 0, &acc, &st, 0, nullptr, &out) == P25FE_ERR_ARG);
    CHECK(p25fe_track_step(&good, 12, 125, 10, 0, &acc, &st, 0, &oa, nullptr) == P25FE_ERR_ARG);
    CHECK(oa.re == 7 && oa.n == 7 && out.step == 7 && out.status == 7);

    // hz
    double hz = -1.0;
    p25fe_track_state_t s = {};
    const int32_t thetas[] = {0, 1, -1, imax, imin, 1 << 30};
    for (int32_t t : thetas) {
        const int32_t ds[] = {2, 10, 64};
        for (int32_t D : ds) {
            s.last_theta = t;
            CHECK(p25fe_track_hz(&s, D, &hz) == P25FE_OK && std::isfinite(hz) && std::fabs(hz) <= 120000.0 / D);
        }
    }
    s.last_theta = 1 << 30;
    CHECK(p25fe_track_hz(&s, 10, &hz) == P25FE_OK && hz == 6000.0);
    hz = -1.0;
    CHECK(p25fe_track_hz(nullptr, 10, &hz) == P25FE_ERR_ARG && p25fe_track_hz(&s, 10, nullptr) == P25FE_ERR_ARG);
    const int32_t bad_d[] = {1, 0, -1, 65, imin, imax};
    for (int32_t D : bad_d) CHECK(p25fe_track_hz(&s, D, &hz) == P25FE_ERR_ARG);
    CHECK(hz == -1.0);

    // the objects' entry points with no object
    p25fe_track_t* lp = reinterpret_cast<p25fe_track_t*>(1);
    CHECK(p25fe_track_create(nullptr, nullptr, &good, &lp) == P25FE_ERR_ARG && lp == nullptr);
    CHECK(p25fe_track_create(nullptr, nullptr, &good, nullptr) == P25FE_ERR_ARG);
    lp = reinterpret_cast<p25fe_track_t*>(1);
    CHECK(p25fe_track_create(nullptr, nullptr, nullptr, &lp) == P25FE_ERR_ARG && lp == nullptr);
    p25fe_track_destroy(nullptr);
    float rows[16] = {};
    CHECK(p25fe_track_measure_dev(nullptr, rows, 8, 0, 8, 0, nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_track_update_dev(nullptr, 0, nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_track_run_dev(nullptr, rows, P25FE_FMT_CF32, 0, 8, 0, 1024, rows, 8, 0, nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_track_read(nullptr, &st) == P25FE_ERR_ARG && p25fe_track_records(nullptr, &acc, nullptr) == P25FE_ERR_ARG);
    std::puts("afc loop host driver ok");
    return 0;
}
