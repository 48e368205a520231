// Stand-alone check of the "gram" kind's host step (pgh_host.h: gram_distances), built with ASan + UBSan by
// tests/test_gram_logic.py.  No input: every entry against the definition in include/pgh_api.h written out once
// more, as bits, for n = 0, 1 and 9, a coinciding pair and an overflowed row among them.  Prints "ok", exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

int main() {
    int fails = 0;
    for (int n : {0, 1, 9}) {
        const size_t N = (size_t)n;
        std::vector<double> G(N * N), s(N), D(N * N, -1.0);
        uint64_t z = 16;
        for (size_t a = 0; a < N; ++a)
            for (size_t b = a; b < N; ++b) {
                z = z * 6364136223846793005ull + 1442695040888963407ull;
                G[a * N + b] = G[b * N + a] = (double)(int64_t)(z >> 40) / 65536.0 - (a == b ? 0.0 : 128.0);
                if (a == b) s[a] = G[a * N + a];
            }
        if (n == 9) {
            s[1] = s[0];
            G[1] = G[N] = std::nextafter(s[0], INFINITY);  // rows 0 and 1 coincide; the rounding went against them
            s[5] = G[5 * N + 2] = G[2 * N + 5] = INFINITY;  // row 5 overflowed, against row 2 in the product too
        }
        pgh_detail::gram_distances(G.data(), s.data(), n, D.data());
        for (size_t a = 0; a < N; ++a)
            for (size_t b = 0; b < N; ++b) {
                const volatile double sum = s[a] + s[b], twice = 2.0 * G[a * N + b];
                const volatile double d = sum - twice;
                const double want = a == b ? 0.0 : std::isnan(d) ? INFINITY : d < 0.0 ? 0.0 : d;
                fails += !same_bits(D[a * N + b], want) || !same_bits(D[a * N + b], D[b * N + a]);
            }
        if (n == 9) fails += !same_bits(D[1], 0.0) || D[5 * N + 2] != INFINITY || D[5 * N + 3] != INFINITY;
    }
    std::printf(fails ? "%d entries differ\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
