// Stand-alone check of the trust rule's host code (pgh_host.h: trust_weights, row_dot_host), built with ASan + UBSan
// by tests/test_native_trust.py.  argv[1] names a text file written from tests/golden/trust_cases.npz and the
// oracle: the number of weight cases, then per case
//   s0 (f64 bits, hex), n, n pairs of sumsq and dot (f64 bits), the expected return code, the number included,
//   their positions, their weights (f32 bits), T (f64 bits);
// then the number of dot cases, per case p, p values of x and p of y (f32 bits), the expected sum (f64 bits).
// Prints "ok" and exits 0 when both functions reproduce every position and every bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::row_dot_host;
using pgh_detail::trust_weights;

template <class T, class U>
static T bit_cast(U u) {
    static_assert(sizeof(T) == sizeof(U), "same size");
    T x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++fails;                      \
        }                                 \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: trust_check <cases.txt>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    int cases = 0;
    if (std::fscanf(f, "%d", &cases) != 1) return 2;
    for (int c = 0; c < cases; ++c) {
        uint64_t s0b = 0, tb = 0;
        int n = 0, rc_want = 0, ni_want = 0;
        if (std::fscanf(f, "%" SCNx64 " %d", &s0b, &n) != 2) return 2;
        // exactly n entries each: the sanitizer sees any read or write past them
        std::vector<double> ss((size_t)n), dot((size_t)n);
        for (int k = 0; k < n; ++k) {
            uint64_t a = 0, b = 0;
            if (std::fscanf(f, "%" SCNx64 " %" SCNx64, &a, &b) != 2) return 2;
            ss[(size_t)k] = bit_cast<double>(a);
            dot[(size_t)k] = bit_cast<double>(b);
        }
        if (std::fscanf(f, "%d %d", &rc_want, &ni_want) != 2) return 2;
        std::vector<int32_t> pos_want((size_t)ni_want);
        std::vector<uint32_t> w_want((size_t)ni_want);
        for (int k = 0; k < ni_want; ++k)
            if (std::fscanf(f, "%" SCNd32, &pos_want[(size_t)k]) != 1) return 2;
        for (int k = 0; k < ni_want; ++k)
            if (std::fscanf(f, "%" SCNx32, &w_want[(size_t)k]) != 1) return 2;
        if (std::fscanf(f, "%" SCNx64, &tb) != 1) return 2;
        std::vector<float> w((size_t)n, -1.f);
        std::vector<int32_t> pos((size_t)n, -1);
        int64_t ni = -1, nt = -1;
        double T = -1.0;
        float mx = -1.f;
        const int rc = trust_weights(bit_cast<double>(s0b), ss.data(), dot.data(), n, w.data(), pos.data(), &ni, &T, &nt, &mx);
        CHECK(rc == rc_want, "case %d: rc %d, want %d", c, rc, rc_want);
        if (rc == -1) continue;  // a bad root: nothing else is written
        CHECK(ni == ni_want, "case %d: %lld included, want %d", c, (long long)ni, ni_want);
        CHECK(bit_cast<uint64_t>(T) == tb, "case %d: T bits %016" PRIx64 ", want %016" PRIx64, c, bit_cast<uint64_t>(T), tb);
        for (int k = 0; k < ni_want && k < ni; ++k) {
            if (rc != -2) CHECK(pos[(size_t)k] == pos_want[(size_t)k], "case %d: position %d is %d, want %d", c, k, pos[(size_t)k], pos_want[(size_t)k]);
            if (rc == 0)
                CHECK(bit_cast<uint32_t>(w[(size_t)k]) == w_want[(size_t)k], "case %d: weight %d bits %08x, want %08x", c, k,
                      bit_cast<uint32_t>(w[(size_t)k]), w_want[(size_t)k]);
        }
        if (rc == 0) {
            float m2 = 0.f;
            for (int64_t k = 0; k < ni; ++k) m2 = w[(size_t)k] > m2 ? w[(size_t)k] : m2;
            CHECK(m2 == mx && nt >= 1 && nt <= ni, "case %d: max weight or trusted count", c);
            // the nullable outputs
            std::vector<float> w2((size_t)n);
            std::vector<int32_t> p2((size_t)n);
            int64_t ni2 = 0;
            double T2 = 0.0;
            CHECK(trust_weights(bit_cast<double>(s0b), ss.data(), dot.data(), n, w2.data(), p2.data(), &ni2, &T2, nullptr, nullptr) == 0 &&
                      ni2 == ni && std::memcmp(w2.data(), w.data(), sizeof(float) * (size_t)ni) == 0,
                  "case %d: the call without the nullable outputs differs", c);
        }
    }
    int dots = 0;
    if (std::fscanf(f, "%d", &dots) != 1) return 2;
    for (int c = 0; c < dots; ++c) {
        long long p = 0;
        uint64_t want = 0;
        if (std::fscanf(f, "%lld", &p) != 1) return 2;
        std::vector<float> x((size_t)p), y((size_t)p);  // exactly p floats: no padding to hide a read past the end
        for (auto* v : {&x, &y})
            for (long long i = 0; i < p; ++i) {
                uint32_t b = 0;
                if (std::fscanf(f, "%" SCNx32, &b) != 1) return 2;
                (*v)[(size_t)i] = bit_cast<float>(b);
            }
        if (std::fscanf(f, "%" SCNx64, &want) != 1) return 2;
        const uint64_t got = bit_cast<uint64_t>(row_dot_host(x.data(), y.data(), p));
        CHECK(got == want, "dot case %d (p = %lld): bits %016" PRIx64 ", want %016" PRIx64, c, p, got, want);
    }
    std::fclose(f);
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ok: %d weight cases, %d dot cases\n", cases, dots);
    return 0;
}
