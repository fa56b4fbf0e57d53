// The host-only functions of the survey (docs/SPEC.md 3.0h) under AddressSanitizer + UBSan: p25fe_scan_window, p25fe_scan_channels
// and the argument checks of p25fe_scan_create, p25fe_scan_dev, p25fe_scan, p25fe_scan_read and p25fe_scan_reset that answer before
// any device is touched.  Links the host-side sanitizer build of the library (make asan); no HIP runtime call is reached, no GPU is
// needed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "p25fe.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "scan host driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // the window: exactly N floats are written
    const int32_t sizes[] = {1024, 4096};
    for (int32_t N : sizes) {
        std::vector<float> w((size_t)N, -9.0f);                       // exactly the room the window needs
        CHECK(p25fe_scan_window(N, w.data(), w.size()) == P25FE_OK);
        CHECK(w[0] == 0.0f && w[(size_t)N / 2] == 1.0f);
        for (int32_t j = 1; j < N; ++j) CHECK(w[(size_t)j] == w[(size_t)(N - j)] && w[(size_t)j] > 0.0f && w[(size_t)j] <= 1.0f);
        CHECK(p25fe_scan_window(N, w.data(), w.size() - 1) == P25FE_ERR_CAPACITY);
        CHECK(p25fe_scan_window(N, nullptr, w.size()) == P25FE_ERR_CAPACITY);
    }
    float one[1] = {-9.0f};
    const int32_t bad_n[] = {0, -1, 512, 1023, 1025, 2048, 8192, imin, imax};
    for (int32_t N : bad_n) CHECK(p25fe_scan_window(N, one, 1) == P25FE_ERR_ARG);
    CHECK(one[0] == -9.0f);

    // create: every check answers with no handle (the last one BECAUSE there is none)
    std::vector<float> win(4096, 0.5f);
    p25fe_scan_t* sc = reinterpret_cast<p25fe_scan_t*>(1);
    const int32_t bad_create[][3] = {{0, 8, 16}, {512, 8, 16}, {2048, 8, 16}, {imin, 8, 16}, {imax, 8, 16}, {1024, 0, 16}, {1024, 4, 16},
                                     {1024, 12, 16}, {1024, 24, 16}, {1024, 2048, 16}, {1024, -8, 16}, {1024, imin, 16}, {1024, imax, 16},
                                     {4096, 8192, 16}, {4096, 96, 16}, {4096, 2048, -1}, {4096, 2048, 41}, {4096, 2048, imin},
                                     {4096, 2048, imax}};
    for (const auto& s : bad_create) {
        sc = reinterpret_cast<p25fe_scan_t*>(1);
        CHECK(p25fe_scan_create(nullptr, s[0], s[1], win.data(), s[2], &sc) == P25FE_ERR_ARG && sc == nullptr);
    }
    for (int32_t N : sizes) {
        std::vector<float> bad((size_t)N, 0.5f);                      // exactly N values: the check reads no more
        bad.back() = std::numeric_limits<float>::quiet_NaN();
        CHECK(p25fe_scan_create(nullptr, N, N / 2, bad.data(), 16, &sc) == P25FE_ERR_ARG);
        bad.back() = -std::numeric_limits<float>::infinity();
        CHECK(p25fe_scan_create(nullptr, N, N / 2, bad.data(), 16, &sc) == P25FE_ERR_ARG);
    }
    CHECK(p25fe_scan_create(nullptr, 4096, 2048, win.data(), 16, nullptr) == P25FE_ERR_ARG);
    sc = reinterpret_cast<p25fe_scan_t*>(1);
    CHECK(p25fe_scan_create(nullptr, 4096, 2048, nullptr, 16, &sc) == P25FE_ERR_ARG && sc == nullptr);       // all valid, no handle
    sc = reinterpret_cast<p25fe_scan_t*>(1);
    CHECK(p25fe_scan_create(nullptr, 1024, 8, win.data(), 40, &sc) == P25FE_ERR_ARG && sc == nullptr);
    p25fe_scan_destroy(nullptr);

    // the calls on an object: no object
    std::vector<uint64_t> rec(4097, 0);
    CHECK(p25fe_scan_dev(nullptr, win.data(), P25FE_FMT_CF32, 0, 2048, 0, rec.data(), nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_scan_dev(nullptr, nullptr, P25FE_FMT_CF32, 0, 2048, 0, rec.data(), nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_scan_dev(nullptr, win.data(), P25FE_FMT_CF32, 0, 2048, (uint64_t)1 << 62, rec.data(), nullptr) == P25FE_ERR_ARG);
    CHECK(p25fe_scan(nullptr, win.data(), P25FE_FMT_CF32, 16) == P25FE_ERR_ARG);
    CHECK(p25fe_scan_read(nullptr, rec.data(), 1) == P25FE_ERR_ARG);
    CHECK(p25fe_scan_reset(nullptr) == P25FE_ERR_ARG);
    for (uint64_t v : rec) CHECK(v == 0);

    // channels: records at the extremes of the words, exactly N + 1 of them, and output arrays of exactly cap records
    for (int32_t N : sizes) {
        std::vector<uint64_t> acc((size_t)N + 1, 1);                  // exactly the record
        acc[(size_t)N] = 7;
        acc[25] = 1000000;
        acc[(size_t)N - 50] = 1000000;
        const uint32_t fs = (uint32_t)N * 1000u;                      // bins 1000 Hz apart: both spikes sit on a raster centre
        size_t n = 99;
        std::vector<p25fe_scan_chan_t> out(2);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, out.data(), out.size(), &n) == P25FE_OK && n == 2);
        CHECK(out[0].raster_index == -4 && out[1].raster_index == 2 && out[0].reserved == 0);     // the tie goes to the smaller r
        CHECK(out[0].centre_hz == -50000.0 && std::fabs(out[0].offset_hz) < 1e-6 && out[0].db_over_floor > 40.0);
        std::vector<p25fe_scan_chan_t> small(1);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, small.data(), small.size(), &n) == P25FE_OK && n == 2);
        CHECK(small[0].raster_index == -4);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, nullptr, 0, &n) == P25FE_OK && n == 2);
        // every eligible channel listed: the output holds exactly as many records
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, -400.0, nullptr, 0, &n) == P25FE_OK && n > 2);
        std::vector<p25fe_scan_chan_t> all(n);
        size_t n2 = 0;
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, -400.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == n);
        for (size_t i = 1; i < n; ++i) CHECK(all[i - 1].db_over_floor >= all[i].db_over_floor);
        // the largest words, a raster of one bin, a raster as wide as the capture, a bandwidth wider than the capture
        for (size_t b = 0; b < (size_t)N; ++b) acc[b] = ~0ull;
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == 0);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 0.0, all.data(), all.size(), &n2) == P25FE_OK && n2 > 0);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 1000.0, 0.0, -10.0, nullptr, 0, &n2) == P25FE_OK && n2 == (size_t)N - 1);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, (double)fs, 1e12, -10.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == 1);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 2.0 * fs, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == 0);
        CHECK(p25fe_scan_channels(acc.data(), N, 1u, 12500.0, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == 0);
        CHECK(p25fe_scan_channels(acc.data(), N, 0xffffffffu, 12500.0, 4000.0, 20.0, nullptr, 0, &n2) == P25FE_OK);
        acc[(size_t)N] = 0;                                           // zero frames
        n2 = 99;
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_OK && n2 == 0);
        acc[(size_t)N] = 1;
        // refusals
        CHECK(p25fe_scan_channels(nullptr, N, fs, 12500.0, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_ERR_ARG);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, all.data(), all.size(), nullptr) == P25FE_ERR_ARG);
        CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, 20.0, nullptr, 1, &n2) == P25FE_ERR_ARG);
        CHECK(p25fe_scan_channels(acc.data(), N, 0, 12500.0, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_ERR_ARG);
        const double bad_raster[] = {0.0, -0.0, -12500.0, inf, -inf, nan};
        for (double r : bad_raster) CHECK(p25fe_scan_channels(acc.data(), N, fs, r, 4000.0, 20.0, all.data(), all.size(), &n2) == P25FE_ERR_ARG);
        const double bad_bw[] = {-1.0, inf, -inf, nan};
        for (double b : bad_bw) CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, b, 20.0, all.data(), all.size(), &n2) == P25FE_ERR_ARG);
        const double bad_thr[] = {inf, -inf, nan};
        for (double t : bad_thr) CHECK(p25fe_scan_channels(acc.data(), N, fs, 12500.0, 4000.0, t, all.data(), all.size(), &n2) == P25FE_ERR_ARG);
        // a raster so fine that the list would be absurd is refused, not allocated
        CHECK(p25fe_scan_channels(acc.data(), N, 0xffffffffu, 1e-3, 4000.0, 20.0, nullptr, 0, &n2) == P25FE_ERR_ARG);
    }
    for (int32_t N : bad_n) {
        uint64_t acc1[1] = {1};
        size_t n = 0;
        CHECK(p25fe_scan_channels(acc1, N, 1000000u, 12500.0, 4000.0, 20.0, nullptr, 0, &n) == P25FE_ERR_ARG);
    }
    std::puts("scan host driver ok");
    return 0;
}
