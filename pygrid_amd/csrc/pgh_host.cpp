// libpygrid_hip: the host side that never touches HIP (declared in pgh_host.h).
#include "pgh_host.h"

#include <emmintrin.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

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
