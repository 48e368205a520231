// Stand-alone check of the HIP-free host code (pgh_host.h): CopyPool::run / run_items and scatter_out
// against memcpy, built by tests/test_native_copy_pool.py under TSan and under ASan + UBSan.
// argv[1]: how many of the 200 run / run_items alternations copy more than the 4 MiB inline threshold
// (the rest stay below it; TSan makes the large ones slow).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::CopyPool;
using pgh_detail::OutPiece;

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

namespace {
constexpr size_t GUARD = 64;
constexpr uint8_t SENTINEL = 0xA5;

std::vector<uint8_t> pattern(size_t n, uint32_t seed) {
    std::vector<uint8_t> v(n);
    uint32_t x = seed * 2654435761u + 1;
    for (auto& b : v) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    return v;
}

// `total` bytes as segments of odd sizes (a zero-length one among them), destinations contiguous
// from dst_off past a 64-byte aligned base, sources taken from the far end of `src` backwards.
void check_run(CopyPool& pool, size_t total, size_t dst_off) {
    const size_t sizes[] = {1, 0, 4095, 300001, 7, 65537, (1u << 20) + 3, 15, 262145, 33};
    const std::vector<uint8_t> src = pattern(total, (uint32_t)(total + dst_off));
    const size_t room = GUARD + 16 + total + GUARD;
    std::unique_ptr<uint8_t, void (*)(void*)> got((uint8_t*)std::aligned_alloc(64, (room + 63) & ~(size_t)63), std::free);
    std::vector<uint8_t> want(room, SENTINEL);
    std::memset(got.get(), SENTINEL, room);
    std::vector<CopyPool::Seg> segs;
    std::vector<size_t> starts;
    size_t at = 0;
    for (size_t k = 0; at < total; ++k) {
        const size_t n = std::min(sizes[k % 10], total - at);
        const uint8_t* from = src.data() + (total - at - n);
        segs.push_back({got.get() + GUARD + dst_off + at, from, n});
        std::memcpy(want.data() + GUARD + dst_off + at, from, n);
        starts.push_back(at);
        at += n;
    }
    if (total >= (4u << 20) && pool.threads() > 1) {  // some segment straddles a thread's share boundary
        const size_t nt = (size_t)pool.threads();
        const size_t per = ((total + nt - 1) / nt + 4095) & ~(size_t)4095;  // CopyPool::share's granules
        bool straddled = false;
        for (size_t k = 0; k < segs.size(); ++k)
            for (size_t edge = per; edge < total; edge += per)
                straddled = straddled || (starts[k] < edge && edge < starts[k] + segs[k].n);
        REQUIRE(straddled);
    }
    pool.run(segs);
    REQUIRE(std::memcmp(got.get(), want.data(), room) == 0);  // the copy and both guards
}

void check_items(CopyPool& pool, int n, bool parallel) {
    std::vector<int> seen((size_t)n + 2, 0);  // plain ints: the pool's hand-over orders the accesses
    pool.run_items(n, parallel, [&](int i) {
        REQUIRE(i >= 0 && i < n);
        ++seen[(size_t)i + 1];
    });
    REQUIRE(seen.front() == 0 && seen.back() == 0);
    for (int i = 0; i < n; ++i) REQUIRE(seen[(size_t)i + 1] == 1);
}

// Windows [off, off + len) of the concatenation of pieces that lie apart in one buffer.
void check_scatter(CopyPool& pool) {
    const size_t sizes[] = {5, 0, 1000, 70000, 13}, gap = 32;
    size_t concat = 0;
    for (size_t n : sizes) concat += n;
    const size_t windows[][2] = {{0, concat}, {2, 2}, {3, 1500}, {1004, 1}, {1006, 69990}, {4, concat - 4 - 6}, {concat - 1, 1}};
    for (auto& w : windows) {
        const size_t off = w[0], len = w[1];
        std::vector<uint8_t> got(gap + concat + 5 * gap, SENTINEL), want = got;
        const std::vector<uint8_t> src = pattern(len, (uint32_t)(off * 31 + len));
        std::vector<OutPiece> pieces;
        size_t pos = gap, base = 0;
        for (size_t n : sizes) {
            pieces.push_back({got.data() + pos, n});
            for (size_t i = 0; i < n; ++i)
                if (base + i >= off && base + i < off + len) want[pos + i] = src[base + i - off];
            pos += n + gap;
            base += n;
        }
        pgh_detail::scatter_out(src.data(), off, len, pieces, pool);
        REQUIRE(got == want);
    }
}
}  // namespace

int main(int argc, char** argv) {
    const int large = argc > 1 ? std::atoi(argv[1]) : 200;
    const size_t above = (5u << 20) + 37, below = (1u << 20) + 37;
    for (int threads : {1, 2, 7}) {
        { CopyPool idle(threads); }  // made and destroyed without a job
        CopyPool pool(threads);
        for (size_t dst_off : {(size_t)1, (size_t)15}) {
            check_run(pool, below, dst_off);
            check_run(pool, above, dst_off);
        }
        for (int n : {0, 1, 2, 3, 5, 10, 16})  // n < threads, n not a multiple of threads
            for (bool parallel : {false, true}) check_items(pool, n, parallel);
        check_scatter(pool);
    }
    CopyPool pool(7);  // the generation counter and the fn_ / segs_ hand-over
    for (int k = 0; k < 200; ++k) {
        check_run(pool, k < large ? (4u << 20) + 4097 : 4097, 1);
        check_items(pool, 10, true);
    }
    std::printf("ok\n");
    return 0;
}
