// Stand-alone check of the HIP-free DP noise sampler (pgh_host.h / pgh_host.cpp), built by
// tests/test_native_dp.py with plain g++ under ASan + UBSan: the Philox4x32-10 known answers, plog against
// libm, the polar method's invariants, and that any window [i0, i0 + n) of the normals -- odd starts, one
// element, indices above 2^33 -- is the same slice of the one sequence, written inside its bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using namespace pgh_detail;

static int fails = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            ++fails;                            \
            std::printf("FAIL %s: ", #cond);    \
            std::printf(__VA_ARGS__);           \
            std::printf("\n");                  \
        }                                       \
    } while (0)

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

int main() {
    struct Kat { uint32_t c[4], k[2], want[4]; };
    const Kat kats[] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
         {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
         {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (const Kat& t : kats) {
        uint32_t x[4];
        philox4x32_10(t.c, t.k, x);
        CHECK(std::memcmp(x, t.want, sizeof x) == 0, "philox known answer: %08x %08x %08x %08x", x[0], x[1], x[2], x[3]);
    }

    // plog within 2 ulp of libm over (0, 1): a sweep of mantissas at many exponents, and the edges
    uint64_t st = 0x9E3779B97F4A7C15ull;
    double worst = 0;
    for (int k = 0; k < 200000; ++k) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t mant = st >> 12;
        const int e = 1022 - (int)((st >> 3) % 110);  // 2^-1 .. 2^-110
        const uint64_t b = ((uint64_t)e << 52) | mant;
        double s;
        std::memcpy(&s, &b, 8);
        const double got = dp_plog(s), want = std::log(s);
        const double ulp = std::fabs(std::nextafter(want, 0.0) - want);
        worst = std::fmax(worst, std::fabs(got - want) / ulp);
    }
    CHECK(worst <= 2.0, "plog is %.3f ulp from log", worst);
    CHECK(dp_plog(std::nextafter(1.0, 0.0)) < 0.0, "plog just below 1 must be negative");
    CHECK(std::fabs(dp_plog(0x1p-105) - std::log(0x1p-105)) < 1e-12, "plog of the smallest s");

    // one sequence, whatever the window
    const uint64_t key = 0x0000567800001234ull;
    const uint32_t round = 7;
    for (const int64_t base : {(int64_t)0, (int64_t)1 << 33, ((int64_t)1 << 62) - 600}) {
        std::vector<double> whole(1000);
        dp_normals(key, round, base, (int64_t)whole.size(), whole.data());
        for (const int64_t off : {0, 1, 2, 3, 7, 500, 999}) {
            for (const int64_t n : {0, 1, 2, 3, 8, 1000}) {
                if (off + n > (int64_t)whole.size()) continue;
                std::vector<double> part((size_t)n);  // exactly n: ASan sees a write past it
                dp_normals(key, round, base + off, n, part.data());
                for (int64_t i = 0; i < n; ++i)
                    CHECK(bits(part[(size_t)i]) == bits(whole[(size_t)(off + i)]), "window %lld+%lld differs at %lld",
                          (long long)(base + off), (long long)n, (long long)i);
            }
        }
        // a pair is a point on the circle of radius sqrt(-2 log s): finite, not both zero
        double sum = 0, sq = 0;
        for (size_t i = 0; i + 1 < whole.size(); i += 2) {
            CHECK(std::isfinite(whole[i]) && std::isfinite(whole[i + 1]), "non-finite normal at %zu", i);
            CHECK(whole[i] != 0.0 || whole[i + 1] != 0.0, "a rejected pair at %zu", i);
        }
        for (double z : whole) { sum += z; sq += z * z; }
        CHECK(std::fabs(sum / 1000) < 0.2 && std::fabs(sq / 1000 - 1.0) < 0.25, "mean %.3f, second moment %.3f", sum / 1000, sq / 1000);
    }
    // another round, another key: another sequence
    double a[4], b[4], c[4];
    dp_normals(key, round, 0, 4, a);
    dp_normals(key, round + 1, 0, 4, b);
    dp_normals(key ^ (1ull << 40), round, 0, 4, c);
    CHECK(std::memcmp(a, b, sizeof a) != 0 && std::memcmp(a, c, sizeof a) != 0, "round / key do not reach the counter");
    CHECK(dp_sigma(1.5f, 2.0f, 3) == 1.0, "sigma = z C / N");

    if (fails) return 1;
    std::printf("ok: philox, plog (%.2f ulp), windows\n", worst);
    return 0;
}
