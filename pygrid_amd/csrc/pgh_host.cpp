// libpygrid_hip: the host side that never touches HIP (declared in pgh_host.h).
#include "pgh_host.h"

#include <emmintrin.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

namespace pgh_detail {

void copy_stream(uint8_t* dst, const uint8_t* src, size_t n) {
    if (n < (256u << 10)) { std::memcpy(dst, src, n); return; }
    const size_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    std::memcpy(dst, src, head);
    dst += head; src += head; n -= head;
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i));
        const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 16));
        const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 32));
        const __m128i d = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i + 48));
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i), a);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i + 16), b);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i + 32), c);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i + 48), d);
    }
    std::memcpy(dst + i, src + i, n - i);
    _mm_sfence();
}

void bind_thread(const std::vector<int>& cpus) {
    if (cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus)
        if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
    (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
}

// Copy bytes [off, off + len) of the concatenation of `pieces` from `src`.
void scatter_out(const uint8_t* src, size_t off, size_t len, const std::vector<OutPiece>& pieces, CopyPool& pool) {
    std::vector<CopyPool::Seg> segs;
    size_t base = 0;
    for (auto& p : pieces) {
        const size_t a = std::max(off, base), b = std::min(off + len, base + p.n);
        if (a < b) segs.push_back({p.dst + (a - base), src + (a - off), b - a});
        base += p.n;
        if (base >= off + len) break;
    }
    pool.run(segs);
}

// Fault in the pages of a small, freshly allocated host destination with one madvise call
// (MADV_POPULATE_WRITE, Linux 5.14+) instead of one page fault per 4 KiB during the copy-out; big
// destinations are left to the copy pool, whose threads fault their own pages in parallel.  Best
// effort: an older kernel or a non-anonymous mapping just returns an error, which is ignored.
void prefault_small(uint8_t* p, size_t n) {
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
    if (!p || n == 0 || n >= (4u << 20)) return;
    static const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
    const uintptr_t a = (uintptr_t)p & ~(page - 1), b = ((uintptr_t)p + n + page - 1) & ~(page - 1);
    (void)madvise((void*)a, b - a, MADV_POPULATE_WRITE);
}

// MADV_POPULATE_WRITE over [p, p + n) whatever its size (pgh_host_prefault's per-thread piece).
void prefault_small_any(uint8_t* p, size_t n) {
    static const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
    const uintptr_t a = (uintptr_t)p & ~(page - 1), b = ((uintptr_t)p + n + page - 1) & ~(page - 1);
    (void)madvise((void*)a, b - a, MADV_POPULATE_WRITE);
}

// The same for a big fresh destination, split over the copy pool's threads: run while the fold
// and the first D2H are still in flight, so the copy-out afterwards writes to resident pages
// instead of taking a page fault per 4 KiB.
// Every page of [a, b) is already in memory (an output framed and faulted in beforehand,
// pgh_host_prefault): one mincore call, far cheaper than MADV_POPULATE_WRITE walking the same
// present pages again (≈1.6 ms for 47 MB, tools/patch_probe.py, profiles/r03l/).
bool all_resident(uintptr_t a, uintptr_t b, uintptr_t page) {
    std::vector<unsigned char> v((size_t)((b - a) / page));
    if (v.empty() || mincore((void*)a, b - a, v.data()) != 0) return false;
    for (unsigned char x : v)
        if (!(x & 1)) return false;
    return true;
}

void prefault_parallel(uint8_t* p, size_t n, CopyPool& pool) {
    if (!p || n == 0) return;
    if (n < (4u << 20)) { prefault_small(p, n); return; }
    static const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
    const uintptr_t a = (uintptr_t)p & ~(page - 1), b = ((uintptr_t)p + n + page - 1) & ~(page - 1);
    if (all_resident(a, b, page)) return;
    // (transparent huge pages for this range measured neutral, profiles/r02ad/: 4 KiB pages)
    const int k = pool.threads();
    const uintptr_t per = ((b - a) / k + page - 1) & ~(page - 1);
    pool.run_items(k, true, [&](int i) {
        const uintptr_t lo = a + per * (uintptr_t)i, hi = std::min(b, lo + per);
        if (lo < hi) (void)madvise((void*)lo, hi - lo, MADV_POPULATE_WRITE);
    });
}

// ---- the DP noise sampler (the definition: include/pgh_api.h) -----------------------------------------------

void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

double dp_plog(double s) {
    uint64_t b;
    std::memcpy(&b, &s, 8);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    uint64_t mb = b & 0xfffffffffffffull;
    if (mb >= 0x6a09e667f3bcdull) {
        e += 1;
        mb |= 0x3fe0000000000000ull;
    } else {
        mb |= 0x3ff0000000000000ull;
    }
    double m;
    std::memcpy(&m, &mb, 8);
    const double f = m - 1.0, t = f / (2.0 + f), w = t * t;
    static const double lg[7] = {6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01,
                                 2.222219843214978396e-01, 1.818357216161805012e-01, 1.531383769920937332e-01,
                                 1.479819860511658591e-01};
    double R = lg[6];
    for (int k = 5; k >= 0; --k) {
        R = R * w;
        R = R + lg[k];
    }
    R = R * w;
    const double hi = (double)e * 0x1.62e42fefa39efp-1, u = f - R, tu = t * u, lo = f - tu;
    return hi + lo;
}

namespace {
inline double dp_uniform(uint32_t lo, uint32_t hi) {
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    // an arithmetic shift by 11, written without shifting a negative value
    const int64_t q = (u >> 63) ? (int64_t)((u >> 11) | 0xffe0000000000000ull) : (int64_t)(u >> 11);
    return ((double)q + 0.5) * 0x1p-52;
}
}  // namespace

void dp_pair_normals(uint64_t key, uint32_t round, uint64_t pair, double* z0, double* z1) {
    const uint32_t kw[2] = {(uint32_t)key, (uint32_t)(key >> 32)};
    for (uint32_t a = 0; a < 32; ++a) {
        const uint32_t ctr[4] = {(uint32_t)pair, (uint32_t)(pair >> 32), round, a};
        uint32_t x[4];
        philox4x32_10(ctr, kw, x);
        const double v1 = dp_uniform(x[0], x[1]), v2 = dp_uniform(x[2], x[3]);
        const double s1 = v1 * v1, s2 = v2 * v2, s = s1 + s2;
        if (s < 1.0) {
            const double num = -2.0 * dp_plog(s), quo = num / s, f = std::sqrt(quo);
            *z0 = v1 * f;
            *z1 = v2 * f;
            return;
        }
    }
    *z0 = 0.0;
    *z1 = 0.0;
}

void dp_normals(uint64_t key, uint32_t round, int64_t i0, int64_t n, double* out) {
    for (int64_t i = i0; i < i0 + n;) {
        double z[2];
        dp_pair_normals(key, round, (uint64_t)i >> 1, &z[0], &z[1]);
        for (int64_t e = i & 1; e < 2 && i < i0 + n; ++e, ++i) out[i - i0] = z[e];
    }
}

bool geomed_step(const double* D, int64_t n, float nu, float* w, float* W, double* objective, float* max_w) {
    std::vector<double> beta((size_t)n);
    double B = 0.0, obj = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const double dist = std::sqrt(D[k]);
        beta[(size_t)k] = std::isfinite(D[k]) ? 1.0 / std::max((double)nu, dist) : 0.0;
        B = k == 0 ? beta[0] : B + beta[(size_t)k];
        obj = k == 0 ? dist : obj + dist;
    }
    if (objective) *objective = obj;
    if (!(B != 0.0)) return false;
    float tot = 0.f, mx = 0.f;
    for (int64_t k = 0; k < n; ++k) {
        w[k] = (float)(beta[(size_t)k] / B);
        tot = k == 0 ? w[0] : tot + w[k];
        mx = k == 0 || w[k] > mx ? w[k] : mx;
    }
    *W = tot;
    if (max_w) *max_w = mx;
    return true;
}

int krum_select(const double* D, int n, int f, int m, int32_t* picked, int* n_picked, double* scores) {
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b)
            if (a != b && !(D[(size_t)a * (size_t)n + (size_t)b] >= 0.0)) return -1;  // NaN or negative
    if ((int64_t)n < 2 * (int64_t)f + 3) return -3;
    const int k = n - f - 2, keep = m == 0 ? n - f : m;
    std::vector<double> sc((size_t)n), row;
    for (int a = 0; a < n; ++a) {
        row.clear();
        for (int b = 0; b < n; ++b)
            if (b != a) row.push_back(D[(size_t)a * (size_t)n + (size_t)b]);
        std::partial_sort(row.begin(), row.begin() + k, row.end());  // (no NaN: < is a strict weak order; equal values add alike)
        double s = row[0];
        for (int j = 1; j < k; ++j) s += row[(size_t)j];
        sc[(size_t)a] = s;
    }
    if (scores) std::copy(sc.begin(), sc.end(), scores);
    if (keep > n - f) return -3;
    std::vector<int32_t> order((size_t)n);
    for (int a = 0; a < n; ++a) order[(size_t)a] = a;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return sc[(size_t)x] < sc[(size_t)y]; });
    std::sort(order.begin(), order.begin() + keep);  // the picked rows in list order
    std::copy(order.begin(), order.begin() + keep, picked);
    *n_picked = keep;
    return 0;
}

double row_dot_host(const float* x, const float* y, int64_t p) {
    double row = 0.0;
    for (int64_t base = 0; base < p || base == 0; base += 4096) {
        double a[256];
        for (int l = 0; l < 256; ++l) {
            double acc = 0.0;
            for (int j = 0; j < 4; ++j)
                for (int e = 0; e < 4; ++e) {
                    const int64_t i = base + 4 * (l + 256 * j) + e;
                    // (the product of two f32 values is exact in f64: one rounded addition, as the kernels' fma)
                    acc = acc + (i < p ? (double)x[i] * (double)y[i] : 0.0);
                }
            a[l] = acc;
        }
        double w[4];
        for (int wv = 0; wv < 4; ++wv) {
            double* v = a + 64 * wv;
            for (int h = 32; h >= 1; h >>= 1)
                for (int l = 0; l < h; ++l) v[l] = v[l] + v[l + h];
            w[wv] = v[0];
        }
        row = row + (((w[0] + w[1]) + w[2]) + w[3]);
    }
    return row;
}

int trust_weights(double s0, const double* sumsq, const double* dot, int64_t n, float* w, int32_t* included,
                  int64_t* n_included, double* T, int64_t* n_trusted, float* max_w) {
    if (!(std::isfinite(s0) && s0 > 0.0)) return -1;
    const double n0 = std::sqrt(s0);
    std::vector<double> a;
    double tot = 0.0;
    int64_t ni = 0, nt = 0;
    for (int64_t k = 0; k < n; ++k) {
        const double sc = sumsq[k];
        if (!std::isfinite(sc)) continue;  // excluded
        double ts = 0.0, ac = 0.0;
        if (sc > 0.0) {
            const double nc = std::sqrt(sc);
            const double den = n0 * nc;
            const double cosc = dot[k] / den;
            ts = cosc > 0.0 ? cosc : 0.0;
            const double resc = n0 / nc;
            ac = ts * resc;
        }
        included[ni] = (int32_t)k;
        tot = ni == 0 ? ts : tot + ts;
        a.push_back(ac);
        nt += ts > 0.0 ? 1 : 0;
        ++ni;
    }
    *n_included = ni;
    if (n_trusted) *n_trusted = nt;
    if (max_w) *max_w = 0.f;
    if (ni == 0) {
        *T = 0.0;
        return -2;
    }
    *T = tot;
    if (!(tot != 0.0)) return -3;
    float mx = 0.f;
    for (int64_t k = 0; k < ni; ++k) {
        const double q = a[(size_t)k] / tot;
        w[k] = (float)std::min(q, (double)FLT_MAX);
        mx = w[k] > mx ? w[k] : mx;
    }
    if (max_w) *max_w = mx;
    return 0;
}

}  // namespace pgh_detail

namespace pgh_int {
int usable_cpus() {
    static const int n = [] {
        int cpus = 0;
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = CPU_COUNT(&set);
        if (cpus <= 0) cpus = (int)std::max(1u, std::thread::hardware_concurrency());
        double quota = 0;
        std::ifstream v2("/sys/fs/cgroup/cpu.max");
        std::string q;
        long long per = 0;
        if (v2 >> q >> per) {
            if (q != "max" && per > 0) quota = std::atof(q.c_str()) / (double)per;
        } else {
            std::ifstream qf("/sys/fs/cgroup/cpu/cpu.cfs_quota_us"), pf("/sys/fs/cgroup/cpu/cpu.cfs_period_us");
            long long qq = 0, pp = 0;
            if ((qf >> qq) && (pf >> pp) && qq > 0 && pp > 0) quota = (double)qq / (double)pp;
        }
        if (quota >= 1 && (int)quota < cpus) cpus = (int)quota;
        return std::max(1, cpus);
    }();
    return n;
}
}  // namespace pgh_int
