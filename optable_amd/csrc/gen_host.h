// gen_host.h — host-side bookkeeping of the generation path (optable_hip.hip: trace_tree, trace_generation) that needs no
// HIP: where the generations live and how scratch is carved.  Plain C++, so tools/gen_host_check.cpp runs it under the host
// sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/optable_hip.h"

static inline size_t align_up(size_t x) { return (x + 255) / 256 * 256; }

// Bump carver over one allocation, every piece rounded up to 256 bytes.  Run the list of take() calls once over a NULL base
// for the size (`used`; the pointers it hands out are NULL) and again over the allocation for the layout: one list gives both.
struct Carve {
    uint8_t* base;
    size_t used = 0;
    template <class U> U* take(size_t count, bool wanted = true) {  // !wanted: NULL, no bytes
        if (!wanted) return nullptr;
        U* p = base ? (U*)(base + used) : nullptr;
        used += align_up(sizeof(U) * count);
        return p;
    }
};

// One holder of a generation.  ot_trace_tree_* has three, indexed by the `where` its result[2] reports: [0] the caller's
// input, [1] buf_a, [2] buf_b.  A generation is read from holder w and its children written to other(w).
struct GenBuf {
    const ot_rays* rays;
    const int32_t* tree;
    int32_t* tree_out = nullptr;  // the same array where children may be written to it: the two buffers, not the caller's input
    int32_t* rem = nullptr;       // per-ray budgets of the one-pass kernel (NULL: the call takes no one-pass generation)
    uint8_t* ahead = nullptr;     // look-ahead bytes (NULL: none kept; the caller's input never has them)
};
static inline int other(int where) { return where == 1 ? 2 : 1; }

// Scratch of a two-pass generation of n rays (k_gen_pass and what surrounds it) in a scene with `ns` count slots; `reuse`: the
// count pass keeps its decision per ray for the emit pass.  Returns the bytes.
template <class T> struct GenScratch {
    int64_t* totals;
    uint8_t* code;
    unsigned long long *wave_total, *wave_prefix;
    int32_t *probe, *probe_ex, *rank, *hit_node;
    T* hit_t;
    size_t carve(void* base, int64_t n, int ns, bool reuse) {
        Carve cv{(uint8_t*)base};
        const size_t n_waves = (size_t)((n + 63) / 64), n_slot = (size_t)n * (ns > 0 ? ns : 0);
        totals = cv.take<int64_t>(4);
        code = cv.take<uint8_t>((size_t)n);
        wave_total = cv.take<unsigned long long>(n_waves);
        wave_prefix = cv.take<unsigned long long>(n_waves);
        probe = cv.take<int32_t>(n_slot, ns > 0);
        probe_ex = cv.take<int32_t>(n_slot, ns > 0);
        rank = cv.take<int32_t>(n_slot, ns > 0);
        hit_node = cv.take<int32_t>((size_t)n, reuse);
        hit_t = cv.take<T>((size_t)n, reuse);
        return cv.used;
    }
};
