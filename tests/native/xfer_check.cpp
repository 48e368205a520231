// Stand-alone check of the HIP-free pieces of the transfer side (pgh_host.h): PieceCursor, the walk over
// concatenated host pieces that fills staging slots and ingest chunks, against a memcpy of the
// concatenation; and the chunk arithmetic of ranged ingest.  Built by tests/test_native_xfer.py under
// ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::CopyPool;
using pgh_detail::INGEST_CHUNK;
using pgh_detail::Piece;
using pgh_detail::PieceCursor;

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

namespace {
uint32_t g_x = 12345;
uint32_t rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

// The pieces lie apart in `store`; `concat` is what they hold one after another.
struct Pieces {
    std::vector<std::vector<uint8_t>> store;
    std::vector<Piece> list;
    std::vector<uint8_t> concat;
    explicit Pieces(const std::vector<size_t>& sizes) {
        for (size_t n : sizes) {
            store.emplace_back(n);
            for (auto& b : store.back()) b = (uint8_t)rnd();
            concat.insert(concat.end(), store.back().begin(), store.back().end());
        }
        for (auto& s : store) list.push_back({s.data(), s.size()});
    }
};

// Walk `p` with the rooms rooms[0], rooms[1], ... (cycled) the way the staging loops do -- one destination
// per take, of exactly `room` bytes, so a segment past it is an overflow the sanitizer sees -- and copy
// through the emitted segments.
void check_walk(const Pieces& p, const std::vector<size_t>& rooms) {
    const size_t total = p.concat.size();
    std::vector<uint8_t> got;
    PieceCursor cur{p.list};
    size_t done = 0;
    for (size_t k = 0; done < total; ++k) {
        const size_t room = rooms[k % rooms.size()];
        REQUIRE(room > 0);
        std::vector<uint8_t> dst(room, 0xA5);
        std::vector<CopyPool::Seg> segs;
        const size_t took = cur.take(dst.data(), room, &segs);
        REQUIRE(took == std::min(room, total - done));  // the room filled, or what is left
        size_t at = 0;
        for (auto& sg : segs) {  // the segments tile [dst, dst + took) in order
            REQUIRE(sg.dst == dst.data() + at);
            if (sg.n) std::memcpy(sg.dst, sg.src, sg.n);  // (an empty piece may have no address)
            at += sg.n;
        }
        REQUIRE(at == took);
        got.insert(got.end(), dst.begin(), dst.begin() + (std::ptrdiff_t)took);
        done += took;
    }
    REQUIRE(done == total);
    REQUIRE(got == p.concat);
    std::vector<CopyPool::Seg> segs;  // past the end (trailing zero-length pieces aside): nothing more to take
    uint8_t one = 0;
    REQUIRE(cur.take(&one, 1, &segs) == 0);
    for (auto& sg : segs) REQUIRE(sg.n == 0);
}

void check_cursor() {
    // by hand: zero-length pieces first, in the middle and last; single bytes; pieces ending on the room edge
    const std::vector<std::vector<size_t>> lists = {
        {0, 5, 0, 1, 1, 8, 0},      {8, 8, 8},          {1},       {0, 0, 1, 0}, {16},
        {3, 5, 8, 16, 1, 7, 0, 24}, {4096, 1, 4095, 0}, {7, 9, 0}, {1, 1, 1, 1, 1, 1, 1, 1, 1},
    };
    for (auto& sizes : lists) {
        Pieces p(sizes);
        for (size_t room : {1, 2, 3, 7, 8, 16, 24, 4096, 8192, 100000}) check_walk(p, {room});
        check_walk(p, {8, 1, 16, 3});
        // rooms that end exactly where a piece does: the prefix sums of the sizes, as successive rooms
        std::vector<size_t> edges;
        for (size_t n : sizes)
            if (n) edges.push_back(n);
        check_walk(p, edges);
    }
    for (int it = 0; it < 300; ++it) {  // random lists: a third zero-length, a third single bytes
        std::vector<size_t> sizes((size_t)(1 + rnd() % 12));
        size_t total = 0;
        for (auto& n : sizes) {
            const uint32_t kind = rnd() % 3;
            n = kind == 0 ? 0 : kind == 1 ? 1 : 1 + rnd() % 5000;
            total += n;
        }
        if (total == 0) sizes.push_back(1);
        Pieces p(sizes);
        std::vector<size_t> rooms((size_t)(1 + rnd() % 4));
        for (auto& r : rooms) r = 1 + rnd() % 6000;
        check_walk(p, rooms);
        check_walk(p, {sizes[rnd() % sizes.size()] + 1});  // a room one past a piece's length
    }
}

void check_chunks() {
    for (int64_t pg : {(int64_t)1, INGEST_CHUNK - 1, INGEST_CHUNK, INGEST_CHUNK + 1, 2 * INGEST_CHUNK + 5}) {
        const int K = pgh_detail::ingest_chunks(pg);
        REQUIRE(K == (int)((pg + INGEST_CHUNK - 1) / INGEST_CHUNK) && K >= 1);
        size_t end = 0;  // the chunks tile [0, 4 pg): each starts where the one before ended
        for (int k = 0; k < K; ++k) {
            size_t a = 1, b = 0;
            pgh_detail::ingest_chunk_bytes(pg, k, &a, &b);
            REQUIRE(a == end && b > a && b - a <= (size_t)INGEST_CHUNK * 4 && a % 4 == 0 && b % 4 == 0);
            REQUIRE(a == (size_t)k * INGEST_CHUNK * 4);  // chunk k holds the params from k * INGEST_CHUNK on
            end = b;
        }
        REQUIRE(end == (size_t)pg * 4);
    }
    // a gather chunk cut at the room never crosses an INGEST_CHUNK boundary, and reaches it when not cut sooner
    std::vector<int64_t> ats = {0, 1, INGEST_CHUNK - 1, INGEST_CHUNK, INGEST_CHUNK + 1, 2 * INGEST_CHUNK - 1, 5 * INGEST_CHUNK};
    for (int it = 0; it < 1000; ++it) ats.push_back((int64_t)(((uint64_t)rnd() << 8) % (uint64_t)(4 * INGEST_CHUNK)));
    for (int64_t at : ats) {
        const int64_t room = pgh_detail::ingest_chunk_room(at);
        REQUIRE(room >= 1 && room <= INGEST_CHUNK);
        REQUIRE(at / INGEST_CHUNK == (at + room - 1) / INGEST_CHUNK);
        REQUIRE((at + room) % INGEST_CHUNK == 0);
    }
    // the cut as the gather table makes it: payloads of nf floats one after another, chunks of at most G
    for (int64_t G : {(int64_t)1000, (int64_t)1 << 16, 3 * INGEST_CHUNK}) {
        int64_t dst = 0;
        for (int64_t nf : {INGEST_CHUNK - 3, (int64_t)7, INGEST_CHUNK, (int64_t)0, 2 * INGEST_CHUNK + 5}) {
            for (int64_t k = 0; k < nf;) {
                const int64_t len = std::min(std::min(G, nf - k), pgh_detail::ingest_chunk_room(dst + k));
                REQUIRE(len >= 1);
                REQUIRE((dst + k) / INGEST_CHUNK == (dst + k + len - 1) / INGEST_CHUNK);
                k += len;
            }
            dst += nf;
        }
    }
}
}  // namespace

int main() {
    check_cursor();
    check_chunks();
    std::printf("ok\n");
    return 0;
}
