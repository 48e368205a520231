// Stand-alone check of the geometric median's host step (pgh_host.h: geomed_step), built with ASan + UBSan
// by tests/test_native_geomed.py.  argv[1] names a text file written from tests/golden/geomed_cases.npz:
//   n, the smoothing's f32 bits, n squared distances (f64 bits), n weights (f32 bits), W (f32 bits),
//   the objective (f64 bits) -- all in hex.
// Prints "ok" and exits 0 when geomed_step reproduces every bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::geomed_step;

template <class T, class U>
static T from_bits(U u) {
    static_assert(sizeof(T) == sizeof(U), "same size");
    T x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}
template <class U, class T>
static U bits_of(T x) {
    static_assert(sizeof(T) == sizeof(U), "same size");
    U u;
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
        std::printf("usage: geomed_check <golden.txt>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    long n = 0;
    uint32_t nu_bits = 0;
    if (std::fscanf(f, "%ld %" SCNx32, &n, &nu_bits) != 2 || n <= 0 || n > 4096) return 2;
    std::vector<double> D((size_t)n);
    std::vector<uint32_t> want_w((size_t)n);
    uint32_t want_W = 0;
    uint64_t want_obj = 0, u = 0;
    for (long k = 0; k < n; ++k) {
        if (std::fscanf(f, "%" SCNx64, &u) != 1) return 2;
        D[(size_t)k] = from_bits<double>(u);
    }
    for (long k = 0; k < n; ++k)
        if (std::fscanf(f, "%" SCNx32, &want_w[(size_t)k]) != 1) return 2;
    if (std::fscanf(f, "%" SCNx32 " %" SCNx64, &want_W, &want_obj) != 2) return 2;
    std::fclose(f);
    const float nu = from_bits<float>(nu_bits);

    // the golden case
    std::vector<float> w((size_t)n, -1.f);
    float W = -1.f, mx = -1.f;
    double obj = -1.0;
    CHECK(geomed_step(D.data(), n, nu, w.data(), &W, &obj, &mx), "golden: the step failed");
    float want_mx = 0.f;
    for (long k = 0; k < n; ++k) {
        CHECK(bits_of<uint32_t>(w[(size_t)k]) == want_w[(size_t)k], "golden: w[%ld] = %a", k, (double)w[(size_t)k]);
        const float x = from_bits<float>(want_w[(size_t)k]);
        want_mx = k == 0 || x > want_mx ? x : want_mx;
    }
    CHECK(bits_of<uint32_t>(W) == want_W, "golden: W = %a", (double)W);
    const double wo = from_bits<double>(want_obj);
    CHECK((std::isnan(obj) && std::isnan(wo)) || bits_of<uint64_t>(obj) == want_obj, "golden: objective = %a", obj);
    CHECK(bits_of<uint32_t>(mx) == bits_of<uint32_t>(want_mx), "golden: max weight = %a", (double)mx);

    // one row: w = W = 1 whatever the distance, the objective is the distance
    {
        const double d1[1] = {6.25};
        float w1 = 0.f, W1 = 0.f, m1 = 0.f;
        double o1 = 0.0;
        CHECK(geomed_step(d1, 1, nu, &w1, &W1, &o1, &m1) && w1 == 1.f && W1 == 1.f && o1 == 2.5 && m1 == 1.f, "one row");
        const double d0[1] = {0.0};  // at the point itself: the smoothing keeps the weight finite
        CHECK(geomed_step(d0, 1, nu, &w1, &W1, nullptr, nullptr) && w1 == 1.f && W1 == 1.f, "one row at distance 0");
    }
    // no finite distance: refused, nothing written
    {
        const double bad[3] = {INFINITY, NAN, INFINITY};
        float wb[3] = {7.f, 7.f, 7.f}, Wb = 7.f;
        CHECK(!geomed_step(bad, 3, nu, wb, &Wb, nullptr, nullptr) && wb[0] == 7.f && wb[2] == 7.f && Wb == 7.f, "no finite distance");
    }
    // equal distances: equal weights that fold to 1 within f32 rounding, in fold order
    {
        std::vector<double> eq(1000, 4.0);
        std::vector<float> we(1000);
        float We = 0.f;
        CHECK(geomed_step(eq.data(), 1000, nu, we.data(), &We, nullptr, nullptr), "equal distances");
        float t = we[0];
        for (int k = 1; k < 1000; ++k) t = t + we[(size_t)k];
        CHECK(we[0] == (float)(0.5 / (1000 * 0.5)) && we[999] == we[0] && bits_of<uint32_t>(t) == bits_of<uint32_t>(We), "equal weights");
    }
    if (fails) return 1;
    std::printf("ok: the geometric median's host step reproduces the golden bits (%ld rows)\n", n);
    return 0;
}
