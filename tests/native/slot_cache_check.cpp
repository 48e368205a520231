// Stand-alone check of the per-slot state machine of a cached row reduction (pgh_host.h: SlotCache), built with
// ASan + UBSan by tests/test_native_slot_cache.py.  First a scripted sequence, the state and value of every slot
// checked after each step.  Then, with argv[1], operation sequences replayed from a text file against the states a
// model computed: the number of sequences, then per sequence the number of operations and per operation
//   R n | W slot n | M k s.. | Q k s.. | H v.. (one per slot) | S | F | C
// (reserved, written, missing alone, missing + mark_queued, harvest, all_stale, forget, clear), after M and Q
// the expected list (count, slots), and after every operation the expected cache: the number of slots, per slot
// its state (0, 1, 2) and value, and whether anything is queued.  Values are small integers, exact as doubles.
// Prints "ok" and exits 0 when every state, value and list agrees.
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../pygrid_amd/csrc/pgh_host.h"

using pgh_detail::SlotCache;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++fails;                      \
        }                                 \
    } while (0)

// every slot's state ('N', 'Q', 'V', one letter per slot) and value, and the queued flag
static void expect(const char* step, const SlotCache& sc, const std::string& states, const std::vector<double>& values, bool queued) {
    CHECK(sc.state.size() == states.size() && sc.value.size() == states.size(), "%s: %zu states, %zu values, want %zu", step,
          sc.state.size(), sc.value.size(), states.size());
    if (sc.state.size() != states.size() || sc.value.size() != states.size() || values.size() != states.size()) return;
    for (size_t k = 0; k < states.size(); ++k) {
        const int want = states[k] == 'N' ? SlotCache::NONE : states[k] == 'Q' ? SlotCache::QUEUED : SlotCache::VALID;
        CHECK(sc.state[k] == want, "%s: slot %zu in state %d, want %d", step, k, (int)sc.state[k], want);
        CHECK(sc.at((int)k) == values[k], "%s: slot %zu holds %g, want %g", step, k, sc.at((int)k), values[k]);
    }
    CHECK(sc.anything_queued() == queued, "%s: anything_queued() is %d, want %d", step, (int)sc.anything_queued(), (int)queued);
}

static std::vector<int32_t> missing(SlotCache& sc, std::initializer_list<int32_t> slots) {
    const std::vector<int32_t> v(slots);  // exactly the listed entries: the sanitizer sees a read past them
    return sc.missing(v.data(), (int)v.size());
}

static void scripted() {
    using L = std::vector<int32_t>;
    SlotCache sc;
    expect("made", sc, "", {}, false);
    sc.reserved(8);
    expect("reserved(8)", sc, "NNNNNNNN", {0, 0, 0, 0, 0, 0, 0, 0}, false);
    // a list with repeats: the NONE ones once each, in list order; asking changes nothing
    L todo = missing(sc, {3, 1, 3, 5, 1});
    CHECK(todo == (L{3, 1, 5}), "missing of a list with repeats: %zu entries", todo.size());
    expect("missing alone", sc, "NNNNNNNN", {0, 0, 0, 0, 0, 0, 0, 0}, false);
    sc.mark_queued(todo);
    expect("queued 3 1 5", sc, "NQNQNQNN", {0, 0, 0, 0, 0, 0, 0, 0}, true);
    // slots already QUEUED do not come back
    todo = missing(sc, {1, 2, 3, 2, 6});
    CHECK(todo == (L{2, 6}), "missing beside QUEUED slots: %zu entries", todo.size());
    sc.mark_queued(todo);
    expect("queued 2 6", sc, "NQQQNQQN", {0, 0, 0, 0, 0, 0, 0, 0}, true);
    const std::vector<double> img1{10, 11, 12, 13, 14, 15, 16, 17};
    sc.harvest(img1.data());
    expect("harvest 1", sc, "NVVVNVVN", {0, 11, 12, 13, 0, 15, 16, 0}, false);
    // nor do VALID ones
    todo = missing(sc, {0, 1, 2, 7, 7, 0});
    CHECK(todo == (L{0, 7}), "missing beside VALID slots: %zu entries", todo.size());
    sc.mark_queued(todo);
    expect("queued 0 7", sc, "QVVVNVVQ", {0, 11, 12, 13, 0, 15, 16, 0}, true);
    // written on a QUEUED slot, then the harvest: the slot stays NONE and the image's stale value is not taken
    sc.written(7, 1);
    expect("written(7) while queued", sc, "QVVVNVVN", {0, 11, 12, 13, 0, 15, 16, 0}, true);
    const std::vector<double> img2{20, 21, 22, 23, 24, 25, 26, 27};
    sc.harvest(img2.data());
    expect("harvest 2", sc, "VVVVNVVN", {20, 11, 12, 13, 0, 15, 16, 0}, false);
    // written on VALID slots: NONE, and they are missing again
    sc.written(2, 2);
    expect("written(2, 2)", sc, "VVNNNVVN", {20, 11, 12, 13, 0, 15, 16, 0}, false);
    todo = missing(sc, {2, 3});
    CHECK(todo == (L{2, 3}), "missing after a write: %zu entries", todo.size());
    // queued, written, queued again, one harvest: the value is the image's, the slot is listed twice
    sc.mark_queued(missing(sc, {4}));
    sc.written(4, 1);
    todo = missing(sc, {4});
    CHECK(todo == (L{4}), "missing of a slot written while queued: %zu entries", todo.size());
    sc.mark_queued(todo);
    CHECK(sc.queued == (L{4, 4}), "the queued list holds %zu entries, want 2", sc.queued.size());
    const std::vector<double> img3{30, 31, 32, 33, 34, 35, 36, 37};
    sc.harvest(img3.data());
    expect("harvest 3", sc, "VVNNVVVN", {20, 11, 12, 13, 34, 15, 16, 0}, false);
    // all_stale with entries queued: every slot NONE, and the harvest behind it takes nothing
    sc.mark_queued(missing(sc, {2, 3}));
    expect("queued 2 3", sc, "VVQQVVVN", {20, 11, 12, 13, 34, 15, 16, 0}, true);
    sc.all_stale();
    expect("all_stale", sc, "NNNNNNNN", {20, 11, 12, 13, 34, 15, 16, 0}, false);
    const std::vector<double> img4{40, 41, 42, 43, 44, 45, 46, 47};
    sc.harvest(img4.data());
    expect("harvest after all_stale", sc, "NNNNNNNN", {20, 11, 12, 13, 34, 15, 16, 0}, false);
    // forget, with one slot VALID and one QUEUED
    sc.mark_queued(missing(sc, {5}));
    sc.harvest(img4.data());
    sc.mark_queued(missing(sc, {6}));
    expect("before forget", sc, "NNNNNVQN", {20, 11, 12, 13, 34, 45, 16, 0}, true);
    sc.forget();
    expect("forget", sc, "NNNNNNNN", {20, 11, 12, 13, 34, 45, 16, 0}, false);
    sc.harvest(img4.data());
    expect("harvest after forget", sc, "NNNNNNNN", {20, 11, 12, 13, 34, 45, 16, 0}, false);
    // reserved to a larger length: the new slots exist, every value is 0 again
    sc.reserved(12);
    expect("reserved(12)", sc, "NNNNNNNNNNNN", std::vector<double>(12, 0.0), false);
    sc.mark_queued(missing(sc, {11, 8}));
    const std::vector<double> img5{50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61};
    sc.harvest(img5.data());
    expect("harvest 5", sc, "NNNNNNNNVNNV", {0, 0, 0, 0, 0, 0, 0, 0, 58, 0, 0, 61}, false);
    // ... and to a smaller one with slots past it queued: nothing is left to harvest from an image of 4
    sc.mark_queued(missing(sc, {10, 3}));
    sc.reserved(4);
    expect("reserved(4)", sc, "NNNN", {0, 0, 0, 0}, false);
    const std::vector<double> img6{70, 71, 72, 73};
    sc.harvest(img6.data());
    expect("harvest after reserved(4)", sc, "NNNN", {0, 0, 0, 0}, false);
    sc.mark_queued(missing(sc, {3, 0}));
    sc.harvest(img6.data());
    expect("harvest 6", sc, "VNNV", {70, 0, 0, 73}, false);
    // clear, with a slot queued: no slot at all
    sc.mark_queued(missing(sc, {1}));
    sc.clear();
    expect("clear", sc, "", {}, false);
    sc.harvest(img6.data());
    todo = sc.missing(nullptr, 0);
    CHECK(todo.empty(), "missing of an empty list");
    expect("after clear", sc, "", {}, false);
}

static bool read_list(std::FILE* f, std::vector<int32_t>* v) {
    int k = 0;
    if (std::fscanf(f, "%d", &k) != 1 || k < 0) return false;
    v->assign((size_t)k, 0);
    for (int i = 0; i < k; ++i)
        if (std::fscanf(f, "%d", &(*v)[(size_t)i]) != 1) return false;
    return true;
}

static int replay(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) {
        std::printf("cannot open %s\n", path);
        return -1;
    }
    int seqs = 0;
    if (std::fscanf(f, "%d", &seqs) != 1) return -1;
    for (int q = 0; q < seqs; ++q) {
        SlotCache sc;
        int ops = 0;
        if (std::fscanf(f, "%d", &ops) != 1) return -1;
        for (int o = 0; o < ops; ++o) {
            char op = 0;
            if (std::fscanf(f, " %c", &op) != 1) return -1;
            char step[64];
            std::snprintf(step, sizeof step, "sequence %d, operation %d (%c)", q, o, op);
            std::vector<int32_t> list, want_list;
            if (op == 'R' || op == 'W') {
                int a = 0, b = 0;
                if (std::fscanf(f, "%d", &a) != 1 || (op == 'W' && std::fscanf(f, "%d", &b) != 1)) return -1;
                op == 'R' ? sc.reserved(a) : sc.written(a, b);
            } else if (op == 'M' || op == 'Q') {
                if (!read_list(f, &list) || !read_list(f, &want_list)) return -1;
                const std::vector<int32_t> todo = sc.missing(list.data(), (int)list.size());
                CHECK(todo == want_list, "%s: missing() gave %zu slots, want %zu", step, todo.size(), want_list.size());
                if (op == 'Q') sc.mark_queued(todo);
            } else if (op == 'H') {
                std::vector<double> img(sc.state.size());  // exactly one value per slot
                for (double& v : img)
                    if (std::fscanf(f, "%lf", &v) != 1) return -1;
                sc.harvest(img.data());
            } else if (op == 'S') {
                sc.all_stale();
            } else if (op == 'F') {
                sc.forget();
            } else if (op == 'C') {
                sc.clear();
            } else {
                return -1;
            }
            int n = 0, queued = 0;
            if (std::fscanf(f, "%d", &n) != 1 || n < 0) return -1;
            std::string states((size_t)n, 'N');
            std::vector<double> values((size_t)n);
            for (int k = 0; k < n; ++k) {
                int st = 0;
                if (std::fscanf(f, "%d %lf", &st, &values[(size_t)k]) != 2) return -1;
                states[(size_t)k] = "NQV"[st];
            }
            if (std::fscanf(f, "%d", &queued) != 1) return -1;
            expect(step, sc, states, values, queued != 0);
        }
    }
    std::fclose(f);
    return seqs;
}

int main(int argc, char** argv) {
    scripted();
    int seqs = 0;
    if (argc > 1 && (seqs = replay(argv[1])) < 0) {
        std::printf("bad sequence file %s\n", argv[1]);
        return 2;
    }
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ok: the scripted sequence, %d replayed\n", seqs);
    return 0;
}
