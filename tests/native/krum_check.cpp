// Stand-alone check of the Multi-Krum selection's host step (pgh_host.h: krum_select), built with ASan + UBSan
// by tests/test_native_krum.py.  argv[1] names a text file written from tests/golden/krum_cases.npz: the number
// of cases, then per case
//   n f m, n * n squared distances (f64 bits, hex), the number picked, the picked positions, n scores (f64 bits).
// Prints "ok" and exits 0 when krum_select reproduces every picked list and every bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::krum_select;

static double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}
static uint64_t bits_of(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
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
        std::printf("usage: krum_check <golden.txt>\n");
        return 2;
    }
    std::FILE* fp = std::fopen(argv[1], "r");
    if (!fp) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    int ncases = 0;
    if (std::fscanf(fp, "%d", &ncases) != 1 || ncases <= 0 || ncases > 64) return 2;
    for (int c = 0; c < ncases; ++c) {
        int n = 0, f = 0, m = 0, want_np = 0;
        if (std::fscanf(fp, "%d %d %d", &n, &f, &m) != 3 || n <= 0 || n > 1024) return 2;
        std::vector<double> D((size_t)n * (size_t)n);
        uint64_t u = 0;
        for (double& x : D) {
            if (std::fscanf(fp, "%" SCNx64, &u) != 1) return 2;
            x = from_bits(u);
        }
        if (std::fscanf(fp, "%d", &want_np) != 1 || want_np < 0 || want_np > n) return 2;
        std::vector<int32_t> want((size_t)want_np);
        for (int32_t& p : want)
            if (std::fscanf(fp, "%" SCNd32, &p) != 1) return 2;
        std::vector<uint64_t> want_sc((size_t)n);
        for (uint64_t& s : want_sc)
            if (std::fscanf(fp, "%" SCNx64, &s) != 1) return 2;

        std::vector<int32_t> picked((size_t)n, -1);
        std::vector<double> sc((size_t)n, -1.0);
        int np = -1;
        CHECK(krum_select(D.data(), n, f, m, picked.data(), &np, sc.data()) == 0, "case %d: the step failed", c);
        CHECK(np == want_np, "case %d: %d picked, want %d", c, np, want_np);
        for (int k = 0; k < want_np && k < np; ++k)
            CHECK(picked[(size_t)k] == want[(size_t)k], "case %d: picked[%d] = %d, want %d", c, k, picked[(size_t)k], want[(size_t)k]);
        for (int k = 0; k < n; ++k)
            CHECK(bits_of(sc[(size_t)k]) == want_sc[(size_t)k], "case %d: score[%d] = %a", c, k, sc[(size_t)k]);
        // scores are optional; the picked list does not depend on them being asked for
        std::vector<int32_t> again((size_t)n, -1);
        int np2 = -1;
        CHECK(krum_select(D.data(), n, f, m, again.data(), &np2, nullptr) == 0 && np2 == np && again == picked, "case %d: without scores", c);
    }
    std::fclose(fp);

    // the smallest selection: f = 0, three rows, k = 1: each row's nearest neighbour
    {
        const double D[9] = {0, 1, 4, 1, 0, 9, 4, 9, 0};
        int32_t p[3] = {-1, -1, -1};
        int np = 0;
        double sc[3];
        CHECK(krum_select(D, 3, 0, 1, p, &np, sc) == 0 && np == 1 && p[0] == 0 && sc[0] == 1 && sc[1] == 1 && sc[2] == 4, "three rows");
        CHECK(krum_select(D, 3, 0, 0, p, &np, nullptr) == 0 && np == 3 && p[0] == 0 && p[1] == 1 && p[2] == 2, "three rows, all kept");
    }
    // refusals: too few rows for f, m too large, a NaN and a negative entry; nothing is written to picked
    {
        std::vector<double> D(36, 1.0);
        for (int a = 0; a < 6; ++a) D[(size_t)a * 7] = 0.0;
        int32_t p[6] = {7, 7, 7, 7, 7, 7};
        int np = 7;
        CHECK(krum_select(D.data(), 6, 2, 0, p, &np, nullptr) == -3 && np == 7 && p[0] == 7, "n < 2f + 3");
        CHECK(krum_select(D.data(), 6, 1, 6, p, &np, nullptr) == -3 && np == 7 && p[0] == 7, "m > n - f");
        D[9] = NAN;
        CHECK(krum_select(D.data(), 6, 1, 0, p, &np, nullptr) == -1 && np == 7, "a NaN entry");
        D[9] = -1.0;
        CHECK(krum_select(D.data(), 6, 1, 0, p, &np, nullptr) == -1 && np == 7, "a negative entry");
        D[9] = INFINITY;
        CHECK(krum_select(D.data(), 6, 1, 0, p, &np, nullptr) == 0 && np == 5, "+inf is a value");
    }
    if (fails) return 1;
    std::printf("ok: the Multi-Krum host step reproduces the golden picks and bits (%d cases)\n", ncases);
    return 0;
}
