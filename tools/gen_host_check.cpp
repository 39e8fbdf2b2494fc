// gen_host_check.cpp — the host bookkeeping of the generation path (optable_amd/csrc/gen_host.h) under the host sanitizers.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gen_host_check.cpp -o tools/bin/gen_host_check && tools/bin/gen_host_check
// No GPU, no HIP: the structs are plain C++.  Exits non-zero at the first check that fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../optable_amd/csrc/gen_host.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// size pass == carve pass; every piece 256-byte aligned, inside the allocation and written end to end (the sanitizer watches);
// unwanted pieces NULL
template <class T> static void check_scratch(int64_t n, int ns, bool reuse, size_t expected_bytes) {
    GenScratch<T> sized, s;
    const size_t bytes = sized.carve(nullptr, n, ns, reuse);
    CHECK(bytes == expected_bytes);
    CHECK(!sized.totals && !sized.code && !sized.rank && !sized.hit_t);
    std::vector<uint8_t> heap(bytes + 256);
    uint8_t* base = (uint8_t*)align_up((size_t)heap.data());
    CHECK(s.carve(base, n, ns, reuse) == bytes);
    const size_t n_waves = (size_t)((n + 63) / 64);
    size_t end = 0;
    const auto piece = [&](void* p, size_t item, size_t count, bool wanted) {
        if (!wanted) {
            CHECK(p == nullptr);
            return;
        }
        const size_t at = (size_t)((uint8_t*)p - base);
        CHECK(at == end && at % 256 == 0 && at + item * count <= bytes);  // in the order of the list, nothing between the pieces but padding
        for (size_t k = 0; k < item * count; ++k) ((uint8_t*)p)[k] = 1;
        end = at + align_up(item * count);
    };
    piece(s.totals, 8, 4, true);
    piece(s.code, 1, n, true);
    piece(s.wave_total, 8, n_waves, true);
    piece(s.wave_prefix, 8, n_waves, true);
    piece(s.probe, 4, (size_t)n * ns, ns > 0);
    piece(s.probe_ex, 4, (size_t)n * ns, ns > 0);
    piece(s.rank, 4, (size_t)n * ns, ns > 0);
    piece(s.hit_node, 4, n, reuse);
    piece(s.hit_t, sizeof(T), n, reuse);
    CHECK(end == bytes);
}

int main() {
    // Carve itself
    Carve size{nullptr};
    CHECK(size.take<int32_t>(1) == nullptr && size.used == 256);
    CHECK(size.take<double>(100, false) == nullptr && size.used == 256);  // an unwanted piece costs nothing
    CHECK(size.take<double>(33) == nullptr && size.used == 256 + 512);
    alignas(256) static uint8_t arena[1024];
    Carve cv{arena};
    CHECK((uint8_t*)cv.take<int32_t>(1) == arena);
    CHECK(cv.take<double>(100, false) == nullptr);
    CHECK((uint8_t*)cv.take<double>(33) == arena + 256 && cv.used == size.used);

    // The two-pass scratch of 1000 rays.  The sums are the layout this file was introduced to preserve, written out:
    // totals 256 | code 1024 | wave totals 256 | wave prefixes 256 = 1792, three times 12032 per count-slot array with 3 slots,
    // hit nodes 4096 and hit distances 8192 (4096 in single precision) with decision reuse.
    check_scratch<double>(1000, 0, false, 1792);
    check_scratch<double>(1000, 0, true, 14080);
    check_scratch<float>(1000, 0, true, 9984);
    check_scratch<double>(1000, 3, false, 37888);
    check_scratch<double>(1000, 3, true, 50176);
    check_scratch<float>(1000, 3, true, 46080);
    GenScratch<double> s;
    uint8_t* const base = (uint8_t*)4096;  // (offsets only: nothing is dereferenced)
    s.carve(base, 1000, 3, true);
    CHECK((uint8_t*)s.totals - base == 0 && s.code - base == 256 && (uint8_t*)s.wave_total - base == 1280 && (uint8_t*)s.wave_prefix - base == 1536);
    CHECK((uint8_t*)s.probe - base == 1792 && (uint8_t*)s.probe_ex - base == 13824 && (uint8_t*)s.rank - base == 25856);
    CHECK((uint8_t*)s.hit_node - base == 37888 && (uint8_t*)s.hit_t - base == 41984);
    s.carve(base, 1000, 0, true);
    CHECK(!s.probe && !s.probe_ex && !s.rank && (uint8_t*)s.hit_node - base == 1792 && (uint8_t*)s.hit_t - base == 5888);
    check_scratch<double>(1, 1, true, 256 * 9);  // the smallest generation: every piece one unit
    check_scratch<float>(65537, 2, false, 256 + 65792 + 2 * 8448 + 3 * 524544);

    // Where the generations go: a call starts on the caller's input (0) and writes buf_a (1); from then on the two buffers
    // take turns, whichever kernel runs and whether the step is a chain link or not.
    CHECK(other(0) == 1 && other(1) == 2 && other(2) == 1);
    const int expected[] = {1, 2, 1, 2, 1, 2, 1};  // one pass, two passes, a chain of four links, two passes
    int where = 0;
    for (int want : expected) {
        const int src = where, dst = other(where);
        CHECK(dst != src && dst != 0 && dst == want);  // never onto the generation being read, never onto the caller's input
        where = dst;
    }
    puts("gen_host_check: ok");
    return 0;
}
