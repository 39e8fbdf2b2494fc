// optable_hip.hip — the C-ABI of liboptable_hip.so (include/optable_hip.h): context, scene validation and upload,
// kernel selection and launch.  The kernels are in kernels.h, the device math in trace_core.h.
// No CPU fallback lives here: without a GPU every entry point fails with OT_ERR_HIP.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <tuple>
#include <chrono>
#include <vector>

#include "gen_host.h"
#include "kernels.h"
#include "misc_kernels.h"
#include "tables.h"

// ------------------------------------------------------------------------------------------
// error plumbing
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(OT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

// ------------------------------------------------------------------------------------------
// context
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, need) != hipSuccess) return -1;
        bytes = need;
        return 0;
    }
};

// The uploaded scene in one precision (fill_blob): [0] single, [1] double in ot_ctx, image_of<T>() picks
struct SceneImage {
    void* blob = nullptr;
    size_t bytes = 0;
    size_t head = 0;        // node + material records at the front of the image (k_trace_trees IMG = 2 keeps these in LDS)
    int32_t runs_word = 0;  // instanced runs folded by fill_blob (trace_core.h NodeRef)
};

// Shape of a launch as ot_debug_last_launch reports it (include/optable_hip.h), in the order of info[0..7]
enum : int32_t { LL_PAIR_QUEUE = 1, LL_REC_LDS = 2, LL_APPEND = 4, LL_TILES = 8, LL_POOL = 16, LL_REFILL = 32 };  // bits of info[7]
struct LaunchShape {
    int32_t kernel, threads, per_cu, grid, lds_bytes;
    int32_t cap;    // rolling lists: list capacity per wave; refill: rays per ticket; pool: its slots; lane per tree: queue entries in LDS
    int32_t mixed;  // 1 = mixed generations; lane per tree: queue entries in the scratch ring
    int32_t flags;  // LL_*
};

// Heavy scenes (launch_rolling): what classify_rolling makes of the scene and the options, ...
struct RollingScene {
    int fr = 0;                                // preset of k_trace_rolling / k_trace_refill / k_trace_pool (tables.h): 0 FR, 1 FC, 2 FD, 3 F_ALL, 4 FRP
    bool mix = false;                          // lists mix generations
    bool img_fits = false;                     // the image goes to LDS next to the lists; else: read from L2, by the all-features preset
    bool flat_ok = false;                      // candidates through the wave-wide pair queue (flat_grid_hit) ...
    int32_t flat_cap = 0;                      // ... of at most this many pairs a round
    size_t img = 0, entry = 0, rec_bytes = 0;  // bytes: the image in whole 16, a list entry, the record of a live ray
    int32_t cap0 = 0;                          // list capacity asked for
    auto tie() const { return std::tie(fr, mix, img, img_fits, flat_ok, flat_cap, entry, rec_bytes, cap0); }
};
// ... everything plan_rolling may read (it sees no ot_ctx, so no option can move a plan without being part of this key), ...
struct RollingPlanArgs {
    RollingScene scene;
    int32_t opt_rec_lds = -1;  // OT_OPT_LDS_RECORDS
    bool sweep_room = false;   // the pair queue's room is the plan's to choose (OT_OPT_FLAT_QUEUE = 1)
    uint64_t upload = 0;       // serial of the ot_scene_upload the scene came with (0: no plan yet)
    bool operator==(const RollingPlanArgs& o) const { return scene.tie() == o.scene.tie() && opt_rec_lds == o.opt_rec_lds && sweep_room == o.sweep_room && upload == o.upload; }
};
// ... one placement of image and records with the waves per CU it allows (rolling_occupancy; waves = 0: none fits), ...
struct RollingTry { int waves = 0, wpb = 0, per_cu = 0; int32_t cap = 0, capl = 0; size_t lds = 0; bool lds_img = false; };  // capl > 0: the records of the first `capl` list positions in LDS
// ... and the launch plan (a dozen occupancy queries): kept per precision and output layout, reused while its arguments compare equal
struct RollingPlan { RollingPlanArgs args; RollingTry at; int32_t flat_cap = 0; };

struct ot_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cus = 256;
    // scene
    bool has_scene = false;
    bool has_implicit = false;  // a leaf is OT_SHAPE_IMPLICIT_CHEB (the IMG = 2 tree kernel lacks its normal: kernels.h k_trace_trees)
    SceneImage image[2];
    uint64_t uploads = 0;  // ot_scene_upload calls that replaced the images
    int32_t n_nodes = 0, n_mats = 0, n_aux = 0, n_slots = 0, max_children = 0;
    int32_t n_phys = 0, n_runs = 0;  // instanced runs folded by fill_blob (trace_core.h NodeRef)
    int32_t opt_append_chunk = 512;  // append layout: slots per claim
    int32_t opt_instancing = 1;      // fold lattice children into instanced runs at upload
    bool opt_gen_parent = false;     // ot_trace_generation_*: next_tree[] = index of the parent ray (OT_OPT_GEN_PARENT_INDEX)
    int32_t opt_gen_drop = 1;        // generation kernels: children of a tree whose budget ends with this generation are not emitted
    int32_t opt_gen_reuse = -1;      // generation kernels: emit pass rebuilds the count pass's hit instead of searching again (-1 auto)
    double unit = 1e-2;
    uint32_t features = 0;
    int32_t root_max_items = 0;  // most items in one cell of the top-level grid
    int64_t root_n_items = 0;    // entries of all its cells together
    int32_t root_pack = -1;      // aux offset of the packed cells (fill_blob), -1 when not built
    int32_t root_grid = -1;  // aux offset of the top-level grid
    int32_t cache_mat = -1;  // first Sellmeier material
    int32_t* slot_max = nullptr;  // device [n_slots]: max_interact_count per count slot
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    double total_ms = 0.0;
    int64_t launches = 0;
    // knobs
    // scene images above this stay in global memory (L2): a 100+ KB LDS image leaves one block per CU,
    // and on cfg 5 the lost occupancy cost 1.5x (tools/bench_configs.py)
    int32_t opt_lds_limit_kb = 64;
    int32_t opt_kernel = 0;  // 0 auto, 1 fused (lane per ray), 2 rolling lists (the heavy-scene kernel)
    int32_t last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ot_debug_last_launch
    RollingPlan plan[2][2];  // [precision][output layout]
    int32_t opt_refill = 0;      // mixed scenes: rays in registers, refilled in place (k_trace_refill): 0 never (the lists; default: the two tie on cfg 3
                                 // in the append layout, 2.08-2.11 ms, and the lists win into [k][ray] slots, 3.7 against 4.7 ms), 1 whenever a kernel exists
    int32_t opt_refill_ticket = 0;  // rays per ticket of k_trace_refill (0 = by batch size)
    int32_t opt_pool_jitter = 0; // k_trace_pool: one in this many state-word publications is held back ~8000 cycles (protocol test; 0 = off)
    int32_t opt_pool = -1;       // curved-surface scenes, fp32: workgroup-wide block pool (-1 auto, 0 never, 1 whenever it fits)
    int32_t opt_rec_lds = -1;    // pair-queue scenes: records of the live rays in LDS (-1 auto, 0 never, 1 whenever it fits)
    int32_t opt_list_cap = 128;  // k_trace_rolling: live rays per wave (cfg 3: 128 beats 256 and 512)
    int32_t opt_flat = 1;  // fp32 planar top-level-grid scenes: wave-wide pair queue (flat_grid_hit)
    int32_t opt_mix = -1;  // -1 auto (scenes under a top-level grid mix generations), 0 never
    int32_t opt_list_cap_pure = 0;  // generation-pure lists: 0 = the chunk rule below
    Scratch blocked;
    size_t blocked_queue_off = 0;
    int32_t opt_pair = 1;  // paired 16-byte segment stores in the lane-per-ray kernel
    int32_t opt_nt = 1, opt_minw = 4, opt_blocks_per_cu = 0;  // defaults from tools/tune.py on MI355X
    Scratch gen, scan_tmp, mon, gen_rem, gen_ahead, trees;
    Scratch psf, psf_hits;  // ot_monitor_psf_many: its tables and tickets; the hit list and the partials (sized once the hits are counted)
    int32_t opt_trees_global = 0;      // k_trace_trees: 1 = every scene through the all-features kernel that reads its image from global memory (test knob)
    int32_t opt_uniform = 1;  // the lane-per-ray kernel reads fields flagged in a call's uniform_mask once per wave (0: the mask is dropped)
    int32_t opt_resident = 1; // ... and leaves the planes of a call's resident_mask and the fields of its first_mask unwritten where the output holds them (2: planes only; 0: both masks are dropped)
    bool whole_intensity = false;  // every leaf hands a ray's intensity on unchanged or not at all (found at upload: resident_planes)
    int32_t opt_trees_flat = 1;        // k_trace_trees: planar scenes under a top-level grid of leaves search through the wave-wide pair queue
    int32_t opt_trees_refill_at = 16;  // k_trace_trees: idle lanes of a wave at which they take their next trees (64: a wave takes 64 trees at a time)
    int32_t opt_trees_lds = 0;  // k_trace_trees: queue entries per lane kept in LDS (the rest of a tree's queue lives in a global scratch); 0: by the cap
    int32_t opt_gen_ahead = 1;  // ot_trace_tree_*: the emit pass counts its children's children, the next generation skips its count pass (k_gen_pass MODE 2)
    int32_t opt_gen_onepass = -1;  // ot_trace_tree_*: one pass per generation with a decoupled look-back (k_gen_one): -1 (default) generations of up to
                                   // 65536 rays (one launch instead of six), 0 never, 1 always.  Large generations keep count + scan + emit: the
                                   // one-pass kernel moves 22 % fewer bytes but every tile waits for the slowest of its predecessors (cfg 4 with
                                   // R = 0.2: 18.4 ms against 13.6, tools/ab_onepass.py).  Scenes with count-limited surfaces: always two passes
    double probe_us[2][2] = {{0, 0}, {0, 0}};  // ot_probe_layouts: [precision][0 slot arrays, 1 tiles] microseconds per launch of the stream companion; 0 = not measured
    int64_t* gen_chain = nullptr;                // k_gen_one in chained launches: the generation sizes, on the device
    unsigned long long* gen_mismatch = nullptr;  // count / emit disagreements of k_gen_pass (expected: 0)
    int64_t* pinned_state = nullptr;             // ot_trace_tree_*: page-locked landing place of the per-generation read-back
};

// derived scene facts, one definition each
template <class T> static const SceneImage& image_of(const ot_ctx* c) { return c->image[sizeof(T) == 8 ? 1 : 0]; }
// the generation, lane-per-ray and one-pass kernels stage the whole image in LDS (OT_OPT_LDS_LIMIT_KB), else read it from L2
template <class T> static bool in_lds(const ot_ctx* c) { return image_of<T>(c).bytes <= (size_t)c->opt_lds_limit_kb * 1024; }
// heavy scenes keep the count pass's decision per ray for the emit pass (kernels.h k_gen_pass); OT_OPT_GEN_REUSE: -1 auto
static bool gen_reuse(const ot_ctx* c) { return c->opt_gen_reuse < 0 ? c->n_nodes >= 12 : c->opt_gen_reuse != 0; }
static void set_last_launch(ot_ctx* c, const LaunchShape& s) {
    const int32_t info[8] = {s.kernel, s.threads, s.per_cu, s.grid, s.lds_bytes, s.cap, s.mixed, s.flags};
    memcpy(c->last_launch, info, sizeof info);
}

static int flush_events(ot_ctx* c) {
    if (c->events_used == 0) return 0;
    HIP_TRY(hipEventSynchronize(c->events[c->events_used - 1].second));
    for (size_t k = 0; k < c->events_used; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->events[k].first, c->events[k].second));
        c->total_ms += ms;
        c->launches += 1;
    }
    c->events_used = 0;
    return 0;
}
// room for one more event pair at events[events_used]
static int next_event_pair(ot_ctx* c) {
    if (c->events_used < c->events.size()) return 0;
    if (c->events.size() >= 1024) return flush_events(c);
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    c->events.push_back({a, b});
    return 0;
}
static int timing_begin(ot_ctx* c) {
    if (!c->timing) return 0;
    const int rc = next_event_pair(c);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->events[c->events_used].first, c->stream));
    return 0;
}
// Single-kernel launches attach the event pair to the dispatch itself (hipExtLaunchKernelGGL): the
// timestamps are the kernel's own begin/end and no extra marker packets sit between launches.
static int timing_pair(ot_ctx* c, hipEvent_t* start, hipEvent_t* stop) {
    *start = *stop = nullptr;
    if (!c->timing) return 0;
    const int rc = next_event_pair(c);
    if (rc) return rc;
    *start = c->events[c->events_used].first;
    *stop = c->events[c->events_used].second;
    c->events_used += 1;
    return 0;
}

static int timing_end(ot_ctx* c) {
    if (!c->timing) return 0;
    HIP_TRY(hipEventRecord(c->events[c->events_used].second, c->stream));
    c->events_used += 1;
    return 0;
}

// host -> device node conversion
// Cells of the top-level grid in one word each (first item | count << 11) behind the caller's aux array, for the pair-queue
// walk (trace_core.h flat_grid_hit): possible when the item list has at most 1023 entries and no cell more than 42.
// Returns the number of cells to append, 0 when the grid is absent or too large for the packing.
static int64_t packable_cells(const ot_scene_desc* s) {
    if (s->root_grid < 0) return 0;
    const double* g = s->aux + s->root_grid;
    const int64_t cells = (int64_t)g[2] * (int64_t)g[3];
    if ((int64_t)g[11 + cells] > 1023) return 0;  // a queue marker is (lane << 10 | index into the item list) + 1, in 16 bits
    for (int64_t k = 0; k < cells; ++k)
        if (g[11 + k + 1] - g[11 + k] > 42) return 0;
    return cells;
}
// Aspheres whose implicit function g = x + F(r) is convex (or concave) along every line through the local box — F convex and
// non-decreasing on [0, box diagonal] (or -F) — get a device flag: a ray that starts on such a surface can skip the root
// scan in the two cases trace_core.h hit_leaf spells out.  Checked numerically on 512 samples of the reference's own F
// (component_group.py:1061-1064, 1092-1097); anything not clearly convex gets no flag and the full scan.
static double host_sag(const ot_node& h, double r) {
    const double r2 = r * r;
    if (h.shape == OT_SHAPE_ASPHERE_PARAM) {
        const double R = h.p[1], k = h.p[2], r4 = r2 * r2;
        return r2 / (R * (1.0 + std::sqrt(1.0 - (1.0 + k) * r2 / (R * R)))) + h.p[3] * r4 + h.p[4] * r4 * r2 + h.p[5] * r4 * r4;
    }
    const double EFL = h.p[1], n = h.p[2];
    return (EFL / (n + 1.0)) * (-1.0 + std::sqrt(1.0 + (n + 1.0) / (n - 1.0) * r2 / (EFL * EFL)));
}
static int32_t asphere_convexity(const ot_node& h) {
    if (h.kind != OT_NODE_LEAF || (h.shape != OT_SHAPE_ASPHERE_PARAM && h.shape != OT_SHAPE_ASPHERE_EXACT)) return 0;
    constexpr int N = 512;
    const double rmax = 1.4143 * h.p[0] * 1.001, dr = rmax / N;
    if (!(rmax > 0)) return 0;
    double f[N + 1];
    for (int j = 0; j <= N; ++j) {
        f[j] = host_sag(h, j * dr);
        if (!std::isfinite(f[j])) return 0;
    }
    double scale = 0.0;
    for (int j = 0; j <= N; ++j) scale = std::fmax(scale, std::fabs(f[j]));
    const double tol = 1e-13 * (scale + 1e-300);
    bool pos = true, neg = true;  // F (resp. -F) non-decreasing and convex
    for (int j = 1; j <= N; ++j) {
        const double d1 = f[j] - f[j - 1];
        if (d1 < -tol) pos = false;
        if (d1 > tol) neg = false;
        if (j < N) {
            const double d2 = f[j + 1] - 2.0 * f[j] + f[j - 1];
            if (d2 < -tol) pos = false;
            if (d2 > tol) neg = false;
        }
    }
    return pos ? DN_CONVEX_POS : (neg ? DN_CONVEX_NEG : 0);
}

// Instanced runs: consecutive leaf children of a gridded group that differ only in origin, lab AABB and leaf id — the caps
// of an MMA, the lenslets of an MLA, the mirrors of a DMD (component_group.py:228-304, 367).  The device image keeps one
// record per run plus 9 reals per member (trace_core.h NodeRef); everything is compared bit for bit, so a lattice with
// per-element drift (roc_drift, focal_drift) simply has no runs.  Children of gridded groups are only ever reached
// through the group's grid, never by the linear walk, which is what makes folding them safe.
struct NodeRun { int32_t first, count, pnode, geo; };
static bool same_but_pose(const ot_node& a, const ot_node& b) {
    return !memcmp(a.M, b.M, sizeof a.M) && !memcmp(a.lbox, b.lbox, sizeof a.lbox) && !memcmp(a.p, b.p, sizeof a.p) &&
           !memcmp(&a.reflectivity, &b.reflectivity, 4 * sizeof(double)) && a.kind == b.kind && a.flags == b.flags && a.shape == b.shape &&
           a.interaction == b.interaction && a.mat1 == b.mat1 && a.mat2 == b.mat2 && a.roc_kind == b.roc_kind &&
           a.max_interact_count < 0 && b.max_interact_count < 0 && a.aux < 0 && b.aux < 0 && b.leaf_id == a.leaf_id + 1;
}
static std::vector<NodeRun> find_runs(const ot_scene_desc* s) {
    std::vector<NodeRun> runs;
    constexpr int MIN_RUN = 8, MAX_RUNS = 8;
    for (int g = 0; g < s->n_nodes; ++g) {
        const ot_node& grp = s->nodes[g];
        if (grp.kind != OT_NODE_GROUP || !(grp.flags & OT_NODE_GRID)) continue;
        for (int j = g + 1; j < grp.end;) {  // (validate_scene: every child of a gridded group is a leaf)
            int e = j + 1;
            while (e < grp.end && s->nodes[e].kind == OT_NODE_LEAF && s->nodes[e - 1].kind == OT_NODE_LEAF && same_but_pose(s->nodes[e - 1], s->nodes[e])) ++e;
            if (e - j >= MIN_RUN && (int)runs.size() < MAX_RUNS) runs.push_back({j, e - j, 0, 0});
            j = e;
        }
    }
    return runs;  // ascending in `first` (groups are visited in node order, children in order)
}

template <class T> static void fill_blob(const ot_scene_desc* s, const std::vector<NodeRun>& runs_in, std::vector<uint8_t>& out, int32_t& n_phys,
                                         SceneImage& im) {
    std::vector<NodeRun> runs = runs_in;
    const int64_t pack = packable_cells(s);
    int folded = 0, geo_reals = 0;
    for (const NodeRun& r : runs) { folded += r.count - 1; geo_reals += 9 * r.count; }
    n_phys = s->n_nodes - folded;
    const size_t nb = sizeof(DNode<T>) * n_phys, mb = sizeof(DMat<T>) * s->n_materials, ab = sizeof(T) * (s->n_aux + pack + geo_reals);
    const size_t rb = sizeof(int32_t) * 4 * runs.size();
    out.assign(((nb + mb + ab + rb + 15) / 16) * 16, 0);
    DNode<T>* nodes = reinterpret_cast<DNode<T>*>(out.data());
    size_t next_run = 0;
    int phys = 0;
    for (int i = 0; i < s->n_nodes; ++i) {
        if (next_run < runs.size() && i == runs[next_run].first) runs[next_run].pnode = phys;
        if (next_run < runs.size() && i > runs[next_run].first) {  // a folded member
            if (i == runs[next_run].first + runs[next_run].count - 1) ++next_run;
            continue;
        }
        const ot_node& h = s->nodes[i];
        DNode<T>& d = nodes[phys++];
        for (int k = 0; k < 9; ++k) d.M[k] = (T)h.M[k];
        for (int k = 0; k < 3; ++k) d.org[k] = (T)h.origin[k];
        for (int k = 0; k < 6; ++k) { d.aabb[k] = (T)h.aabb[k]; d.lbox[k] = (T)h.lbox[k]; }
        for (int k = 0; k < 8; ++k) d.p[k] = (T)h.p[k];
        d.refl = (T)h.reflectivity; d.trans = (T)h.transmission; d.focal = (T)h.focal_length; d.roc = (T)h.roc;
        d.inv_focal = (T)(h.focal_length != 0.0 ? 1.0 / h.focal_length : 0.0);
        d.r2 = (T)(h.p[0] * h.p[0]);
        if (h.shape == OT_SHAPE_SPHERE) {  // cap aperture radius squared when the cap is shallower than a hemisphere, else 0
            const double R = h.p[0], ht = h.p[1];
            d.r2 = (T)(ht < R ? R * R - (R - ht) * (R - ht) : 0.0);
        }
        d.rad2 = (T)(h.p[0] * h.p[0]);  // sphere / cylinder radius squared
        if (h.shape == OT_SHAPE_ASPHERE_PARAM) {  // folded constants of the root search (trace_core.h sag_search)
            d.p[6] = (T)((1.0 + h.p[2]) / (h.p[1] * h.p[1]));
            d.p[7] = (T)(1.0 / h.p[1]);
        } else if (h.shape == OT_SHAPE_ASPHERE_EXACT) {
            d.p[6] = (T)((h.p[2] + 1.0) / ((h.p[2] - 1.0) * h.p[1] * h.p[1]));
            d.p[7] = (T)(h.p[1] / (h.p[2] + 1.0));
        }
        d.pad1 = (T)0;
        d.kind = h.kind; d.end = h.end; d.flags = h.flags | asphere_convexity(h); d.shape = h.shape; d.inter = h.interaction;
        d.mat1 = h.mat1; d.mat2 = h.mat2; d.roc_kind = h.roc_kind; d.max_count = h.max_interact_count;
        d.slot = h.count_slot; d.aux = h.aux; d.leaf_id = h.leaf_id;
    }
    DMat<T>* mats = reinterpret_cast<DMat<T>*>(out.data() + nb);
    for (int i = 0; i < s->n_materials; ++i) {
        const ot_material& h = s->materials[i];
        mats[i].n = (T)h.n;
        for (int k = 0; k < 3; ++k) { mats[i].B[k] = (T)h.B[k]; mats[i].C[k] = (T)h.C[k]; }
        mats[i].kind = h.kind;
        mats[i].pad = 0;
    }
    T* aux = reinterpret_cast<T*>(out.data() + nb + mb);
    for (int i = 0; i < s->n_aux; ++i) aux[i] = (T)s->aux[i];
    if (sizeof(T) == 4) {
        // The cell lookup of a gridded group widens the ray's footprint by the grid's margin (trace_core.h grid_children);
        // in single precision the footprint itself carries a few ulp of the coordinates, far above the 1e-7 the host
        // chose for double: widen to 64 ulp of the group's largest coordinate (a fraction of a percent of a cell).
        for (int i = 0; i < s->n_nodes; ++i) {
            const ot_node& g = s->nodes[i];
            if (g.kind != OT_NODE_GROUP || !(g.flags & OT_NODE_GRID)) continue;
            double big = 0.0;
            for (int k = 0; k < 6; ++k) big = std::fmax(big, std::fabs(g.aabb[k]));
            const double m = 64.0 * 1.1920929e-7 * big;
            if ((double)aux[g.aux + 8] < m) aux[g.aux + 8] = (T)m;
        }
    }
    for (int64_t k = 0; k < pack; ++k) {
        const double* start = s->aux + s->root_grid + 11;
        aux[s->n_aux + k] = (T)(start[k] + 2048.0 * (start[k + 1] - start[k]));
    }
    int32_t geo = (int32_t)(s->n_aux + pack);
    for (NodeRun& r : runs) {  // per member: origin[3], lab AABB[6]
        r.geo = geo;
        for (int m = 0; m < r.count; ++m) {
            const ot_node& h = s->nodes[r.first + m];
            for (int k = 0; k < 3; ++k) aux[geo++] = (T)h.origin[k];
            for (int k = 0; k < 6; ++k) aux[geo++] = (T)h.aabb[k];
        }
    }
    im.head = nb + mb;
    im.runs_word = (int32_t)((nb + mb + ab) / 4);
    int32_t* rt = reinterpret_cast<int32_t*>(out.data() + nb + mb + ab);
    for (size_t k = 0; k < runs.size(); ++k) { rt[4 * k] = runs[k].first; rt[4 * k + 1] = runs[k].count; rt[4 * k + 2] = runs[k].pnode; rt[4 * k + 3] = runs[k].geo; }
}

// which code paths the scene needs (trace_core.h feature mask)
static uint32_t scene_features(const ot_scene_desc* s) {
    uint32_t f = 0;
    for (int i = 0; i < s->n_nodes; ++i) {
        const ot_node& nd = s->nodes[i];
        if (nd.flags & OT_NODE_CHECK_AABB) f |= F_AABB;
        if (nd.flags & OT_NODE_GRID) f |= F_GRID;
        if (nd.kind != OT_NODE_LEAF) continue;
        if (nd.shape == OT_SHAPE_POLYGON2D || nd.shape == OT_SHAPE_CSG) f |= F_POLY;
        if (nd.shape != OT_SHAPE_CIRCLE && nd.shape != OT_SHAPE_RECT && nd.shape != OT_SHAPE_POLYGON2D &&
            nd.shape != OT_SHAPE_CSG)
            f |= F_CURVED;
        if (nd.shape == OT_SHAPE_ASPHERE_CHEB || nd.shape == OT_SHAPE_IMPLICIT_CHEB) f |= F_MISC;
        if (nd.shape == OT_SHAPE_POLYGON3D) f |= F_POLY | F_MISC;
        if (nd.shape == OT_SHAPE_CYLINDER) f |= F_MISC;
        if (nd.interaction == OT_INT_REFRACT) f |= F_REFRACT;
        if (nd.interaction == OT_INT_LENS) f |= F_LENS;
        if (nd.max_interact_count >= 0) f |= F_LIMIT;
    }
    for (int i = 0; i < s->n_materials; ++i)
        if (s->materials[i].kind == OT_MAT_CHEB) f |= F_MISC;  // series materials: evaluated by the all-features kernels only
    return f;
}

static int validate_root_grid(const ot_scene_desc* s) {
    if (s->root_grid < 0) return 0;
    if (s->root_grid + 11 > s->n_aux) return fail(OT_ERR_INVALID, "root grid out of range");
    const double* g = s->aux + s->root_grid;
    const int a0 = (int)g[0], a1 = (int)g[1], g0 = (int)g[2], g1 = (int)g[3];
    if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a0 == a1 || g0 < 1 || g1 < 1 || (int64_t)g0 * g1 > 1 << 20)
        return fail(OT_ERR_INVALID, "bad root grid header");
    const int64_t cells = (int64_t)g0 * g1;
    if (s->root_grid + 11 + cells + 1 > s->n_aux) return fail(OT_ERR_INVALID, "root grid starts out of range");
    const double* start = g + 11;
    const int64_t n_items = (int64_t)start[cells];
    if (start[0] != 0 || s->root_grid + 11 + cells + 1 + n_items > s->n_aux) return fail(OT_ERR_INVALID, "root grid items out of range");
    for (int64_t k = 0; k < cells; ++k)
        if (start[k + 1] < start[k]) return fail(OT_ERR_INVALID, "root grid starts not monotone");
    const double* items = start + cells + 1;
    for (int64_t k = 0; k < n_items; ++k) {
        const int ni = (int)items[k];
        if (ni < 0 || ni >= s->n_nodes) return fail(OT_ERR_INVALID, "root grid item out of range");
    }
    for (int i = 0; i < s->n_nodes; ++i)
        if (s->nodes[i].kind == OT_NODE_LEAF && s->nodes[i].max_interact_count >= 0)
            return fail(OT_ERR_INVALID, "a root grid cannot be combined with count-limited leaves");
    for (int i = 0; i < s->n_nodes; ++i)
        if (!(s->nodes[i].flags & OT_NODE_BOX_TRUSTED)) return fail(OT_ERR_INVALID, "a root grid needs OT_NODE_BOX_TRUSTED on every node (the walk stops early on the strength of the boxes)");
    return 0;
}

// polygon record: [nv, plane normal(3), v0(3), e1(3), e2(3) | nv x (x, y)]; returns its length or -1
static int64_t polygon_record_len(const ot_scene_desc* s, int64_t off) {
    if (off < 0 || off + 13 > s->n_aux) return -1;
    const double nv = s->aux[off];
    if (!(nv >= 3 && nv <= 4096) || nv != (double)(int)nv) return -1;
    const int64_t len = 13 + 2 * (int64_t)nv;
    return off + len <= s->n_aux ? len : -1;
}

// Chebyshev series record: [N, lo, hi | blocks x N coefficients] (trace_core.h cheb_eval); returns its length or -1
static int64_t series_record_len(const ot_scene_desc* s, int64_t off, int blocks) {
    if (off < 0 || off + 3 > s->n_aux) return -1;
    const double n = s->aux[off];
    if (!(n >= 1 && n <= 512) || n != (double)(int)n || !(s->aux[off + 2] > s->aux[off + 1])) return -1;
    const int64_t len = 3 + blocks * (int64_t)n;
    return off + len <= s->n_aux ? len : -1;
}

// implicit record: [OT_IMPLICIT_HEADER | 4 blocks x nx*ny*nz coefficients] (trace_core.h cheb3_eval); returns its length or -1
static int64_t implicit_record_len(const ot_scene_desc* s, int64_t off) {
    if (off < 0 || off + OT_IMPLICIT_HEADER > s->n_aux) return -1;
    const double* h = s->aux + off;
    int64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (!(h[a] >= 1 && h[a] <= 64) || h[a] != (double)(int)h[a]) return -1;
        if (!(h[6 + a] > 0) || !(h[6 + a] < 1e300)) return -1;  // 1 / half width: positive and finite
        n *= (int64_t)h[a];
    }
    const int ap = (int)h[10];
    if (h[10] != (double)ap || ap < OT_APERTURE_BOX || ap > OT_APERTURE_BALL || !(h[9] == 1.0 || h[9] == -1.0)) return -1;
    const int64_t len = OT_IMPLICIT_HEADER + 4 * n;
    return off + len <= s->n_aux ? len : -1;
}

// CSG record: [ntok | ntok x (kind, len, body[len])], postfix over a 32-deep bit stack (trace_core.h csg_inside)
static int validate_csg(const ot_scene_desc* s, int64_t off) {
    if (off < 0 || off + 1 > s->n_aux) return fail(OT_ERR_INVALID, "CSG program out of range");
    const double ntok = s->aux[off];
    if (!(ntok >= 1 && ntok <= 1024) || ntok != (double)(int)ntok) return fail(OT_ERR_INVALID, "bad CSG token count");
    int64_t t = off + 1;
    int sp = 0;
    for (int k = 0; k < (int)ntok; ++k) {
        if (t + 2 > s->n_aux) return fail(OT_ERR_INVALID, "CSG token out of range");
        const int kind = (int)s->aux[t];
        const double len = s->aux[t + 1];
        if (!(len >= 0 && len <= 16384) || len != (double)(int)len || t + 2 + (int64_t)len > s->n_aux)
            return fail(OT_ERR_INVALID, "CSG token body out of range");
        if (kind == 100 || kind == 101) {  // union / subtract
            if (sp < 2) return fail(OT_ERR_INVALID, "CSG operator without two operands");
            sp -= 1;
        } else {
            if (kind == OT_SHAPE_CIRCLE) { if (len < 1) return fail(OT_ERR_INVALID, "CSG circle needs a radius"); }
            else if (kind == OT_SHAPE_RECT) { if (len < 2) return fail(OT_ERR_INVALID, "CSG rectangle needs two half sizes"); }
            else if (kind == OT_SHAPE_POLYGON2D) { if (polygon_record_len(s, t + 2) != (int64_t)len) return fail(OT_ERR_INVALID, "bad CSG polygon record"); }
            else return fail(OT_ERR_UNSUPPORTED, "unknown CSG primitive");
            if (++sp > 32) return fail(OT_ERR_UNSUPPORTED, "CSG program deeper than 32");
        }
        t += 2 + (int64_t)len;
    }
    if (sp != 1) return fail(OT_ERR_INVALID, "CSG program does not reduce to one value");
    return 0;
}

static int validate_scene(const ot_scene_desc* s) {
    if (!s || s->n_nodes < 0 || s->n_materials < 0 || s->n_aux < 0 || s->n_count_slots < 0) return fail(OT_ERR_INVALID, "bad scene sizes");
    if (s->n_nodes && !s->nodes) return fail(OT_ERR_INVALID, "nodes is NULL");
    if (s->n_materials && !s->materials) return fail(OT_ERR_INVALID, "materials is NULL");
    if (s->n_aux && !s->aux) return fail(OT_ERR_INVALID, "aux is NULL");
    if (s->max_children < 0 || s->max_children > 2) return fail(OT_ERR_INVALID, "max_children must be 0, 1 or 2");
    if (!(s->unit > 0)) return fail(OT_ERR_INVALID, "unit must be positive");
    for (int i = 0; i < s->n_materials; ++i) {
        const ot_material& m = s->materials[i];
        if (m.kind != OT_MAT_CONST && m.kind != OT_MAT_SELLMEIER && m.kind != OT_MAT_CHEB)
            return fail(OT_ERR_UNSUPPORTED, "unknown material kind");
        if (m.kind == OT_MAT_CHEB && series_record_len(s, (int64_t)m.n, 1) < 0) return fail(OT_ERR_INVALID, "material series record out of range");
    }
    for (int i = 0; i < s->n_nodes; ++i) {
        const ot_node& nd = s->nodes[i];
        if (nd.end <= i || nd.end > s->n_nodes) return fail(OT_ERR_INVALID, "node.end out of range at " + std::to_string(i));
        if (nd.kind == OT_NODE_LEAF) {
            if (nd.end != i + 1) return fail(OT_ERR_INVALID, "leaf.end must be index+1");
            if (nd.shape < 0 || nd.shape > OT_SHAPE_IMPLICIT_CHEB) return fail(OT_ERR_UNSUPPORTED, "unknown shape kind");
            if (nd.shape == OT_SHAPE_ASPHERE_CHEB && series_record_len(s, nd.aux, 3) < 0)
                return fail(OT_ERR_INVALID, "asphere series record out of range at node " + std::to_string(i));
            if (nd.shape == OT_SHAPE_IMPLICIT_CHEB && implicit_record_len(s, nd.aux) < 0)
                return fail(OT_ERR_INVALID, "implicit series record malformed or out of range at node " + std::to_string(i));
            if (nd.interaction < 0 || nd.interaction > OT_INT_BLOCK) return fail(OT_ERR_UNSUPPORTED, "unknown interaction kind");
            if (nd.interaction == OT_INT_REFRACT &&
                (nd.mat1 < 0 || nd.mat1 >= s->n_materials || nd.mat2 < 0 || nd.mat2 >= s->n_materials))
                return fail(OT_ERR_INVALID, "material index out of range");
            if ((nd.shape == OT_SHAPE_POLYGON2D || nd.shape == OT_SHAPE_POLYGON3D) && polygon_record_len(s, nd.aux) < 0)
                return fail(OT_ERR_INVALID, "polygon record out of range at node " + std::to_string(i));
            if (nd.shape == OT_SHAPE_CSG) {
                const int rc = validate_csg(s, nd.aux);
                if (rc) return rc;
            }
            if (nd.max_interact_count >= 0 && (nd.count_slot < 0 || nd.count_slot >= s->n_count_slots))
                return fail(OT_ERR_INVALID, "count_slot out of range");
        } else if (nd.kind != OT_NODE_GROUP) {
            return fail(OT_ERR_INVALID, "unknown node kind");
        } else if (nd.flags & OT_NODE_GRID) {  // grid record: [a0 a1 g0 g1 org0 org1 inv0 inv1 margin | start[] | items]
            if (nd.aux < 0 || nd.aux + 9 > s->n_aux) return fail(OT_ERR_INVALID, "grid record out of range");
            const double* g = s->aux + nd.aux;
            const int a0 = (int)g[0], a1 = (int)g[1], g0 = (int)g[2], g1 = (int)g[3];
            if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a0 == a1 || g0 < 1 || g1 < 1 || (int64_t)g0 * g1 > 1 << 20)
                return fail(OT_ERR_INVALID, "bad grid header");
            const int64_t cells = (int64_t)g0 * g1;
            if (nd.aux + 9 + cells + 1 > s->n_aux) return fail(OT_ERR_INVALID, "grid starts out of range");
            const double* start = g + 9;
            const int64_t n_items = (int64_t)start[cells];
            if (start[0] != 0 || nd.aux + 9 + cells + 1 + n_items > s->n_aux) return fail(OT_ERR_INVALID, "grid items out of range");
            for (int64_t k = 0; k < cells; ++k)
                if (start[k + 1] < start[k]) return fail(OT_ERR_INVALID, "grid starts not monotone");
            const double* items = start + cells + 1;
            for (int64_t k = 0; k < n_items; ++k) {
                const int ci = (int)items[k];
                if (ci <= i || ci >= nd.end || s->nodes[ci].kind != OT_NODE_LEAF) return fail(OT_ERR_INVALID, "grid item is not a leaf child");
            }
            if (!(nd.flags & OT_NODE_BOX_TRUSTED)) return fail(OT_ERR_INVALID, "a gridded group needs OT_NODE_BOX_TRUSTED on itself and its children");
            for (int ci = i + 1; ci < nd.end; ++ci)
                if (!(s->nodes[ci].flags & OT_NODE_BOX_TRUSTED)) return fail(OT_ERR_INVALID, "a gridded group needs OT_NODE_BOX_TRUSTED on itself and its children");
        }
    }
    return 0;
}

extern "C" {

int ot_abi_version(void) { return OT_ABI_VERSION; }

// Which HIP runtime did the dynamic linker bind this library to?  (a process must hold ONE libamdhip64; the
// library names it by soname only, so a copy that is already loaded — PyTorch ships its own — is the one that is used.)
int ot_runtime_info(char* path, int32_t path_capacity, int32_t* runtime_version) {
    if (runtime_version) {
        int v = 0;
        if (hipRuntimeGetVersion(&v) != hipSuccess) { v = 0; (void)hipGetLastError(); }
        *runtime_version = v;
    }
    if (path && path_capacity > 0) {
        path[0] = 0;
        Dl_info info;
        if (dladdr((const void*)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::strncpy(path, info.dli_fname, (size_t)path_capacity - 1);
            path[path_capacity - 1] = 0;
        }
    }
    return 0;
}
const char* ot_last_error(void) { return g_err.c_str(); }

int ot_ctx_create(int device, void* stream, ot_ctx** out) {
    if (!out) return fail(OT_ERR_INVALID, "out is NULL");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(OT_ERR_INVALID, "no such device");
    HIP_TRY(hipSetDevice(device));
    ot_ctx* c = new ot_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;  // NULL is the device's default (null) stream, e.g. torch's default
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cus = prop.multiProcessorCount;
    *out = c;
    return 0;
}

int ot_ctx_destroy(ot_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& e : c->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (SceneImage& im : c->image)
        if (im.blob) (void)hipFree(im.blob);
    if (c->slot_max) (void)hipFree(c->slot_max);
    for (Scratch* s : {&c->gen, &c->gen_rem, &c->gen_ahead, &c->trees, &c->scan_tmp, &c->mon, &c->psf, &c->psf_hits, &c->blocked})
        if (s->p) (void)hipFree(s->p);
    if (c->gen_mismatch) (void)hipFree(c->gen_mismatch);
    if (c->gen_chain) (void)hipFree(c->gen_chain);
    if (c->pinned_state) (void)hipHostFree(c->pinned_state);
    delete c;
    return 0;
}

int ot_ctx_synchronize(ot_ctx* c) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ot_ctx_set_stream(ot_ctx* c, void* stream) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    int rc = flush_events(c);  // pending timing events belong to the old stream
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)stream;
    return 0;
}

int ot_scene_upload(ot_ctx* c, const ot_scene_desc* s) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    int rc = validate_scene(s);
    if (rc) return rc;
    rc = validate_root_grid(s);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint8_t> host[2];
    const std::vector<NodeRun> runs = c->opt_instancing ? find_runs(s) : std::vector<NodeRun>();
    fill_blob<float>(s, runs, host[0], c->n_phys, c->image[0]);
    fill_blob<double>(s, runs, host[1], c->n_phys, c->image[1]);
    c->n_runs = (int32_t)runs.size();
    HIP_TRY(hipStreamSynchronize(c->stream));  // previous launches may still read the old scene
    ++c->uploads;
    for (int p = 0; p < 2; ++p) {
        SceneImage& im = c->image[p];
        if (im.blob) { (void)hipFree(im.blob); im.blob = nullptr; }
        HIP_TRY(hipMalloc(&im.blob, host[p].size() ? host[p].size() : 16));
        if (!host[p].empty()) HIP_TRY(hipMemcpy(im.blob, host[p].data(), host[p].size(), hipMemcpyHostToDevice));
        im.bytes = host[p].size();
    }
    c->n_nodes = s->n_nodes; c->n_mats = s->n_materials; c->n_aux = s->n_aux;
    c->n_slots = s->n_count_slots; c->max_children = s->max_children; c->unit = s->unit;
    c->features = scene_features(s);
    // Does `intensity` survive every interaction bit for bit?  x * 1 keeps the bits of x, so: reflectivity and transmission of every
    // leaf exactly 0 or 1 (a zero emits nothing), and a thin lens — which emits its ray whatever `transmission` is — exactly 1.
    c->whole_intensity = true;
    for (int i = 0; i < s->n_nodes; ++i) {
        const ot_node& h = s->nodes[i];
        if (h.kind != OT_NODE_LEAF) continue;
        const bool unit_rt = (h.reflectivity == 0.0 || h.reflectivity == 1.0) && (h.transmission == 0.0 || h.transmission == 1.0);
        if (!unit_rt || (h.interaction == OT_INT_LENS && h.transmission != 1.0)) c->whole_intensity = false;
    }
    c->has_implicit = false;
    for (int i = 0; i < s->n_nodes; ++i)
        if (s->nodes[i].kind == OT_NODE_LEAF && s->nodes[i].shape == OT_SHAPE_IMPLICIT_CHEB) c->has_implicit = true;
    c->root_grid = s->root_grid;
    c->root_pack = packable_cells(s) > 0 ? s->n_aux : -1;
    c->cache_mat = -1;
    for (int i = 0; i < s->n_materials; ++i)
        if (s->materials[i].kind != OT_MAT_CONST) { c->cache_mat = i; break; }  // the first dispersive material: evaluated once per ray
    if (c->root_grid >= 0) {
        c->features |= F_ROOT | F_AABB;
        const double* g = s->aux + s->root_grid;
        const int64_t cells = (int64_t)g[2] * (int64_t)g[3];
        const double* items = g + 11 + cells + 1;
        const int64_t n_items = (int64_t)g[11 + cells];
        for (int64_t k = 0; k < n_items; ++k)
            if (s->nodes[(int)items[k]].kind != OT_NODE_LEAF) { c->features |= F_SUBTREE; break; }
        c->root_max_items = 0;
        c->root_n_items = n_items;
        for (int64_t k = 0; k < cells; ++k) {
            const int m = (int)(g[11 + k + 1] - g[11 + k]);
            if (m > c->root_max_items) c->root_max_items = m;
        }
    }
    if (c->slot_max) { (void)hipFree(c->slot_max); c->slot_max = nullptr; }
    if (s->n_count_slots > 0) {
        std::vector<int32_t> smax(s->n_count_slots, 0);
        for (int i = 0; i < s->n_nodes; ++i)
            if (s->nodes[i].kind == OT_NODE_LEAF && s->nodes[i].max_interact_count >= 0) smax[s->nodes[i].count_slot] = s->nodes[i].max_interact_count;
        HIP_TRY(hipMalloc((void**)&c->slot_max, sizeof(int32_t) * smax.size()));
        HIP_TRY(hipMemcpy(c->slot_max, smax.data(), sizeof(int32_t) * smax.size(), hipMemcpyHostToDevice));
    }
    c->has_scene = true;
    return 0;
}

}  // extern "C"

static int check_rays(const ot_rays* r, const char* what) {
    if (!r) return fail(OT_ERR_INVALID, std::string(what) + " is NULL");
    const void* f[] = {r->ox, r->oy, r->oz, r->dx, r->dy, r->dz, r->wavelength, r->q_re, r->q_im, r->intensity, r->n,
                       r->pathlength, r->id, r->flags};
    for (const void* p : f)
        if (!p) return fail(OT_ERR_INVALID, std::string(what) + " has a NULL field");
    return 0;
}
static int check_segs(const ot_segments* s) {
    if (!s) return fail(OT_ERR_INVALID, "segments is NULL");
    const void* f[] = {s->ox, s->oy, s->oz, s->dx, s->dy, s->dz, s->length, s->intensity, s->q_re, s->q_im, s->n,
                       s->pathlength, s->ray, s->surface};
    for (const void* p : f)
        if (!p) return fail(OT_ERR_INVALID, "segments has a NULL field");
    return 0;
}

// paired segment stores (kernels.h store_segment_paired), slot arrays only: slot k*n + i is even on even lanes iff n is even, and
// every segment array must be aligned to two elements.  (Tiles are written one element per lane: a tile's planes are contiguous and
// lie at constant offsets from the record, so the pair buys no wider line there and costs its exchange: trace_tiled.)
// fp64 only: measured on cfg 4 (1.6e8 pairs) 12.73 -> 12.08 ms (5230 -> 5510 GB/s, 97 % of the stream ceiling), cfg 2
// 0.108 -> 0.106 ms; in fp32 the pair is an 8-byte store and the kernel is VALU-bound: the exchange costs 7-13 %.
template <class T> static int32_t pair_ok(const ot_ctx* c, const ot_segments* s, int64_t n) {
    if (!c->opt_pair || (n & 1) || sizeof(T) != 8) return 0;
    const void* real[] = {s->ox, s->oy, s->oz, s->dx, s->dy, s->dz, s->length, s->intensity, s->q_re, s->q_im, s->n, s->pathlength};
    for (const void* p : real)
        if ((uintptr_t)p % (2 * sizeof(T))) return 0;
    if ((uintptr_t)s->ray % 8 || (uintptr_t)s->surface % 8) return 0;
    return 1;
}

template <class T> static SceneBlob make_blob(const ot_ctx* c) {
    const SceneImage& im = image_of<T>(c);
    SceneBlob blob;
    blob.words = (const uint32_t*)im.blob;
    blob.n_words = (int32_t)(im.bytes / 4);
    blob.n_nodes = c->n_nodes;
    blob.n_phys = c->n_phys;
    blob.n_mats = c->n_mats;
    blob.root = c->root_grid;
    blob.root_pack = c->root_pack;
    blob.cache_mat = c->cache_mat;
    blob.n_runs = c->n_runs;
    blob.runs_word = im.runs_word;
    return blob;
}

// One kernel launch with everything that goes with it: the ticket words of the persistent kernels and the append cursor zeroed,
// the timing pair attached to the dispatch, the error checked, the shape recorded for ot_debug_last_launch.  `ticket`, `cursor`:
// NULL where the kernel has none.  Grid, workgroup size and dynamic LDS are the shape's.
#ifdef OT_STAMP
constexpr size_t TICKET_WORDS = 24;  // the counter + the phase stamps (ot_debug_stamps)
#else
constexpr size_t TICKET_WORDS = 1;
#endif
template <class... P>
static int launch_kernel(ot_ctx* c, void (*kern)(P...), const LaunchShape& s, unsigned long long* ticket, unsigned long long* cursor,
                         typename std::common_type<P>::type... args) {
    if (s.lds_bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, s.lds_bytes));
    if (ticket) HIP_TRY(hipMemsetAsync(ticket, 0, TICKET_WORDS * sizeof(unsigned long long), c->stream));
    if (cursor) HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
    hipEvent_t ev0, ev1;
    const int rc = timing_pair(c, &ev0, &ev1);
    if (rc) return rc;
    hipExtLaunchKernelGGL(kern, dim3(s.grid), dim3(s.threads), (uint32_t)s.lds_bytes, c->stream, ev0, ev1, 0u, args...);
    HIP_TRY(hipGetLastError());
    set_last_launch(c, s);
    return 0;
}
// The ticket counter of the persistent kernels: TICKET_WORDS behind `scratch_bytes` of per-wave scratch in c->blocked (NULL: no memory)
static unsigned long long* ticket_counter(ot_ctx* c, size_t scratch_bytes) {
    if (c->blocked.ensure(scratch_bytes + 256)) return nullptr;
    c->blocked_queue_off = scratch_bytes;
    return (unsigned long long*)((uint8_t*)c->blocked.p + scratch_bytes);
}

// The planar presets of scenes under a top-level grid: 0 = FR, 1 = FRP, -1 = neither (k_trace_rolling numbers them 0 / 4, k_trace_trees 5 / 6)
static int planar_grid_preset(const ot_ctx* c) {
    using namespace preset;  // tables.h
    if (c->root_grid < 0) return -1;
    return (c->features & ~FR) == 0 ? 0 : ((c->features & ~FRP) == 0 ? 1 : -1);
}
// planar scenes under a top-level grid of leaves: candidates through a wave-wide pair queue (flat_grid_hit).  Returns the pairs a
// round of the queue can hold, 0 when the scene does not qualify.  `planar`: the caller's kernel is one of the planar presets and
// has nothing else against the queue (the callers differ there: classify_rolling, trees_flat_cap).
static int32_t pair_queue_room(const ot_ctx* c, bool planar) {
    // pairs a round of the pair queue can hold: 512, not the worst case of 64 lanes x the fullest cells (cfg 3: 1152) — a round
    // that would overflow defers lanes (flat_grid_hit), and the 1.3 KB per wave are what lets 16 waves per CU run instead of 12
    const int32_t flat_full = 64 * FLAT_CELLS * (c->root_max_items > 0 ? c->root_max_items : 1);
    const int32_t flat_room = c->opt_flat > 1 ? c->opt_flat : 512;  // (>= one lane's worst case: 2 * FLAT_CELLS * 42 items = 168)
    const int32_t flat_cap = flat_full < flat_room ? flat_full : flat_room;
    const bool ok = c->opt_flat && planar && c->root_pack >= 0 && flat_cap <= 8192 && c->n_runs == 0;  // queue entry = lane << 10 | index into the grid's item list
    return ok ? flat_cap : 0;
}

// Heavy scenes: persistent waves with their own lists of live rays (k_trace_rolling).  OUT = SegsT<T>: the [k][ray] slots of
// ot_trace_*; SegPlanes<T>: the append layout of ot_trace_append_*.  Three steps: classify_rolling (the scene and the options),
// plan_rolling (the occupancy search of the lists), and one launcher per kernel: launch_refill, launch_pool, launch_lists.
template <class T> static RollingScene classify_rolling(const ot_ctx* c) {
    using namespace preset;  // tables.h
    RollingScene s;
    const uint32_t need = c->features;
    // Scenes under a top-level grid (many separate components, rays of a wave unrelated after the first bounce)
    // mix generations in a list and top it up continuously.  Scenes whose rays all run through the same sequence
    // of surfaces (cfg 5) keep generation-pure lists: mixing costs them more than the tails do (cfg 5 fp32:
    // 36.6 vs 31.6 ms; cfg 3 fp32: 5.1 vs 5.5 ms).
    s.mix = c->opt_mix < 0 ? c->root_grid >= 0 : (c->opt_mix != 0 && c->root_grid >= 0);
    s.img = ((image_of<T>(c).bytes + 15) / 16) * 16;
    s.img_fits = c->opt_lds_limit_kb != 0 && s.img <= 140 * 1024;  // else: read from L2, by the all-features preset
    const int planar = planar_grid_preset(c);
    s.fr = !s.img_fits ? 3 : (planar == 0 ? 0 : (planar == 1 ? 4 : ((need & ~FC) == 0 ? 1 : ((need & ~FD) == 0 ? 2 : 3))));
    s.flat_cap = pair_queue_room(c, s.mix && (s.fr == 0 || s.fr == 4));  // (generation-pure lists have no pair-queue kernel)
    s.flat_ok = s.flat_cap > 0;
    s.entry = s.mix ? 8 : 4;  // list entry: (ray index | segment index << 32), or the ray index alone (kernels.h)
    s.rec_bytes = 12 * sizeof(T) + 4 * (s.fr == 3 ? 2 : 1);  // per record of a live ray (kernels.h rec_int_words: the all-features preset keeps the count class)
    // List capacity.  Mixed lists (rings, a power of two): 128 (256: +4 %, 512: +25 % on cfg 3).  Generation-pure lists: the
    // longer the better for the lanes (a list shrinks as its rays die and every round ends in a partial pass: 45 lanes per
    // pass at 128 entries, 53 at 256, 58 at 512 on cfg 5), but only the first 128 positions keep their records in LDS and a
    // pass over the global part waits for its loads behind the segment stores of the pass before (one in-order counter):
    // cfg 5 fp32, append layout, 16 waves per CU: 14.9 ms at 128, 13.5 at 256, 16+ at 384 and beyond.
    s.cap0 = s.mix ? c->opt_list_cap : (c->opt_list_cap_pure > 0 ? c->opt_list_cap_pure : 256);
    return s;
}

// Where the scene image and the records of the live rays live, and how many waves share an image.  The waves never
// synchronise after staging, so the workgroup size is only packaging: take what keeps most waves resident per CU
// (registers and LDS decide).  Preference: image + records in LDS (a pass then waits for nothing in global memory)
// when enough waves still fit; else image in LDS, records in the per-wave global scratch (L2); images beyond what
// LDS holds next to the lists are read from L2 (all-features preset only).
// most waves per CU for one placement: image in LDS or not, the first `capl` records of every list in LDS
template <class T, class OUT>
static int rolling_occupancy(const RollingScene& s, size_t flat_b, bool lds_img, int32_t CAP, int32_t CAPL, RollingTry* best) {
    *best = RollingTry();
    const void* k = (const void*)rolling_kernel<T, OUT>(s.fr, s.flat_ok, lds_img, CAPL > 0);
    if (!k) return 0;
    const size_t per_wave = (size_t)CAP * s.entry + flat_b + s.rec_bytes * CAPL;
    for (int wpb = 4; wpb * 64 <= rolling_max_threads<T>(s.fr, s.flat_ok, CAPL > 0); wpb += 4) {
        const size_t lds_b = (lds_img ? s.img : 0) + (size_t)wpb * per_wave;
        if (lds_b > 158 * 1024) continue;
        if (lds_b > 48 * 1024) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 64 * wpb, lds_b) != hipSuccess) per_cu = 0;
        if (per_cu * wpb > best->waves) *best = RollingTry{per_cu * wpb, wpb, per_cu, CAP, CAPL, lds_b, lds_img};
    }
    return 0;
}
// the placement policy for one room of the pair queue (`room` pairs; ignored without the queue)
template <class T, class OUT> static int rolling_placement(const RollingPlanArgs& a, int32_t room, RollingTry* chosen) {
    const RollingScene& s = a.scene;
    const size_t flat_b = s.flat_ok ? flat_lds_bytes<T>(room) : 0;
    *chosen = RollingTry();
    // (1) image in LDS, records in LDS: all of them (mixed lists) or the front of the list (generation-pure lists).
    //     Taken when at least 12 waves per CU still fit (OT_OPT_LDS_RECORDS = 1: whenever it fits at all).
    const int rec_lds_min_waves = a.opt_rec_lds > 0 ? 4 : 12;
    if (s.img_fits && a.opt_rec_lds != 0) {
        // (the LDS part of a list is REC_LDS_POSITIONS = 128 entries, a compile-time constant of the kernels: a mixed list
        // is then exactly that long, a generation-pure one keeps the rest of its cap0 entries in global scratch)
        const int rc = rolling_occupancy<T, OUT>(s, flat_b, true, s.mix || s.cap0 < REC_LDS_POSITIONS ? REC_LDS_POSITIONS : s.cap0, REC_LDS_POSITIONS, chosen);
        if (rc) return rc;
        if (chosen->waves < rec_lds_min_waves) *chosen = RollingTry();
    }
    // (2) image in LDS, records in global scratch
    for (int32_t CAP = s.cap0; s.img_fits && CAP >= 128 && !chosen->waves; CAP >>= 1) {
        const int rc = rolling_occupancy<T, OUT>(s, flat_b, true, CAP, 0, chosen);
        if (rc) return rc;
    }
    // (3) image read from L2
    if (!chosen->waves) return rolling_occupancy<T, OUT>(s, flat_b, false, s.cap0, 0, chosen);
    return 0;
}
template <class T, class OUT> static int plan_rolling(const RollingPlanArgs& a, RollingPlan* plan) {
    const RollingScene& s = a.scene;
    RollingTry best;
    int32_t room_sel = s.flat_cap;
    int rc = rolling_placement<T, OUT>(a, s.flat_cap, &best);
    if (rc) return rc;
    // The pair queue's room is LDS that every wave holds: 512 pairs are 1 KB, and with the records of the live rays in LDS the
    // sixteenth wave of a CU can hang on the last few hundred bytes (cfg 3's scene under grids whose fullest cell holds four or
    // five leaves instead of three: 12 waves per CU instead of 16, 2.6-3.0 ms instead of 2.15-2.25 — tools/sweep_root_grid.py).
    // A round that overflows a smaller queue defers lanes and costs little (cfg 3 with room for 192 pairs where its worst case is
    // 384: 2.165 against 2.13-2.17 ms at 256 ... 512); a lost quarter of the waves costs 25 %.
    // So the room is the largest of 512, 448, ... 192 (>= one lane's worst case of 168) that keeps the most waves resident;
    // OT_OPT_FLAT_QUEUE > 1 still sets it by hand.
    for (int32_t room = s.flat_cap - 64; a.sweep_room && room >= 192; room -= 64) {
        RollingTry t;
        rc = rolling_placement<T, OUT>(a, room, &t);
        if (rc) return rc;
        // (the policy of rolling_placement first — records in LDS when at least 12 waves fit — then the number of waves)
        const bool rec_new = t.capl > 0, rec_old = best.capl > 0;
        if ((rec_new && !rec_old) || (rec_new == rec_old && t.waves > best.waves)) { best = t; room_sel = room; }
    }
    if (!best.waves) return fail(OT_ERR_UNSUPPORTED, "no k_trace_rolling launch configuration fits this scene image");
    *plan = RollingPlan{a, best, room_sel};
    return 0;
}

// what the caller of launch_rolling passed, for the launchers
template <class T, class OUT> struct RollingCall {
    const ot_rays* rays; int64_t n; int32_t K; const OUT& out; const AppendCtl& ac; int32_t *seg_count, *counts; int32_t n_classes;
    static constexpr bool append = std::is_same<OUT, SegPlanes<T>>::value;
};
template <class T, class OUT>
static int launch_rolling_kernel(ot_ctx* c, RollingKern<T, OUT> k, const LaunchShape& shape, const RollingCall<T, OUT>& a, WaveScratch<T> ws,
                                 int32_t cap, int32_t capl, unsigned long long* queue, int32_t mix, int32_t last) {
    return launch_kernel(c, k, shape, queue, a.append ? a.ac.cursor : nullptr, make_blob<T>(c), (T)c->unit, view<T>(a.rays), a.n, a.K, a.out, a.ac,
                         a.seg_count, a.counts, a.n_classes, ws, cap, capl, queue, mix, last);
}
// Mixed scenes: the live rays in registers, refilled in place (k_trace_refill) — no list, no records, 1.5 KB of LDS per wave
// (pair queue) + 1.5 KB (the parked ride-along fields), so registers alone decide how many waves share a CU.
// *done = false: no kernel or no room for this scene, the lists take it.
template <class T, class OUT> static int launch_refill(ot_ctx* c, const RollingScene& s, const RollingCall<T, OUT>& a, bool* done) {
    const auto kf = s.mix && s.img_fits && c->opt_refill > 0 ? refill_kernel<T, OUT>(s.fr, s.flat_ok) : nullptr;
    if (!kf) return 0;
    const int threads = refill_max_threads<T>(s.fr, s.flat_ok), waves = threads / 64;
    const size_t park_bytes = s.flat_ok ? 6 * 64 * sizeof(T) : 0;
    const size_t lds_f = s.img + (size_t)waves * ((s.flat_ok ? flat_lds_bytes<T>(s.flat_cap) : 0) + park_bytes);
    if (lds_f > 158 * 1024) return 0;
    int per_cu = 0;
    if (lds_f > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kf, threads, lds_f) != hipSuccess || per_cu < 1) return 0;
    if (c->opt_blocks_per_cu > 0) per_cu = c->opt_blocks_per_cu;
    const int64_t want = (a.n + 64 * (int64_t)waves - 1) / (64 * (int64_t)waves);
    const int64_t capf = (int64_t)c->n_cus * per_cu;
    const int gridf = (int)(want < capf ? want : capf);
    // rays per ticket (one atomic on the device-wide queue each): 256, less when the batch is small enough that
    // whole tickets would leave waves without work
    const int64_t per_wave4 = a.n / ((int64_t)gridf * waves * 4);
    const int32_t ticket = c->opt_refill_ticket > 0 ? c->opt_refill_ticket : (int32_t)(per_wave4 >= 256 ? 256 : (per_wave4 < 64 ? 64 : (per_wave4 / 64) * 64));
    unsigned long long* queue = ticket_counter(c, 0);
    if (!queue) return fail(OT_ERR_HIP, "hipMalloc of the ticket counter failed");
    *done = true;
    const LaunchShape shape = {2, threads, per_cu, gridf, (int32_t)lds_f, ticket, 1, (s.flat_ok ? LL_PAIR_QUEUE : 0) | (a.append ? LL_APPEND : 0) | LL_REFILL};
    return launch_rolling_kernel<T, OUT>(c, kf, shape, a, WaveScratch<T>{nullptr, 0}, ticket, 0, queue, 1, s.flat_cap);
}
// Generation-pure scenes of the curved-surface preset, single precision, append layout: the workgroup-wide block pool
// (k_trace_pool) when at least 24 blocks of 64 records fit next to the image (cfg 5: 15 KB image, 41 blocks; 12.1 ms
// against 13.8 with the per-wave lists).  Not for the [k][ray] slots unless asked for (OT_OPT_BLOCK_POOL = 1): blocks
// that merge mix rays of many tickets, a pass then stores 64 scattered elements per plane instead of runs (20 ms
// against 14.4).
template <class T, class OUT> static int launch_pool(ot_ctx* c, const RollingScene& s, const RollingCall<T, OUT>& a, bool* done) {
    if (s.mix || sizeof(T) == 8 || !s.img_fits || !(c->opt_pool > 0 || (c->opt_pool < 0 && a.append)) || c->opt_rec_lds == 0 || a.K >= (1 << 20)) return 0;  // (a block's generation has 20 bits)
    const auto kp = pool_kernel<T, OUT>(s.fr);
    const size_t fixed = s.img + (64 + 16) * sizeof(uint32_t);
    const int64_t nb_fit = fixed < 158 * 1024 ? (int64_t)((158 * 1024 - fixed) / (POOL_BLOCK_WORDS * 4)) : 0;
    const int32_t NB = (int32_t)(nb_fit > 64 ? 64 : nb_fit);
    if (!kp || NB < (c->opt_pool > 0 ? 16 : 24)) return 0;
    const size_t lds_p = fixed + (size_t)NB * POOL_BLOCK_WORDS * 4;
    const int64_t want = (a.n + 1023) / 1024;
    const int gridp = (int)(want < c->n_cus ? want : c->n_cus);
    unsigned long long* queue = ticket_counter(c, 0);
    if (!queue) return fail(OT_ERR_HIP, "hipMalloc of the ticket counter failed");
    *done = true;
    const LaunchShape shape = {2, 1024, 1, gridp, (int32_t)lds_p, NB * 64, 0, LL_REC_LDS | LL_POOL | (a.append ? LL_APPEND : 0)};
    return launch_rolling_kernel<T, OUT>(c, kp, shape, a, WaveScratch<T>{nullptr, 0}, NB, 0, queue, 0, c->opt_pool_jitter);
}
template <class T, class OUT> static int launch_lists(ot_ctx* c, const RollingScene& s, const RollingCall<T, OUT>& a) {
    RollingPlan& plan = c->plan[sizeof(T) == 8 ? 1 : 0][a.append ? 1 : 0];
    const RollingPlanArgs args = {s, c->opt_rec_lds, s.flat_ok && c->opt_flat == 1, c->uploads};
    if (!(plan.args == args)) {
        const int rc = plan_rolling<T, OUT>(args, &plan);
        if (rc) return rc;
    }
    const RollingTry& at = plan.at;
    const int wpb = at.wpb;
    const auto kr = rolling_kernel<T, OUT>(s.fr, s.flat_ok, at.lds_img, at.capl > 0);
    if (!kr) return fail(OT_ERR_UNSUPPORTED, "no k_trace_rolling instantiation for this scene / option combination");
    const int per_cu_r = c->opt_blocks_per_cu > 0 ? c->opt_blocks_per_cu : at.per_cu;
    const int64_t want = (a.n + 64 * (int64_t)wpb - 1) / (64 * (int64_t)wpb);  // one ticket per wave at least
    const int64_t capr = (int64_t)c->n_cus * per_cu_r;
    const int gridr = (int)(want < capr ? want : capr);
    // per-wave record scratch (by list position) + the ticket counter
    const size_t wave_bytes = align_up((size_t)(at.cap - at.capl) * s.rec_bytes);  // what the lists keep outside LDS
    unsigned long long* queue = ticket_counter(c, wave_bytes * (size_t)gridr * wpb);
    if (!queue) return fail(OT_ERR_HIP, "hipMalloc of rolling-trace scratch failed");
    const LaunchShape shape = {2, 64 * wpb, per_cu_r, gridr, (int32_t)at.lds, at.cap, s.mix ? 1 : 0,
                               (s.flat_ok ? LL_PAIR_QUEUE : 0) | (at.capl > 0 ? LL_REC_LDS : 0) | (a.append ? LL_APPEND : 0)};
    return launch_rolling_kernel<T, OUT>(c, kr, shape, a, WaveScratch<T>{(uint8_t*)c->blocked.p, (int64_t)wave_bytes}, at.cap, at.capl, queue, s.mix ? 1 : 0,
                                         s.flat_ok ? plan.flat_cap : 0);
}
template <class T, class OUT>
static int launch_rolling(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const OUT& out, const AppendCtl& ac, int32_t* seg_count,
                          int32_t* counts, int32_t n_classes) {
    const RollingScene s = classify_rolling<T>(c);
    const RollingCall<T, OUT> call = {rays, n, K, out, ac, seg_count, counts, n_classes};
    bool done = false;
    int rc = launch_refill<T, OUT>(c, s, call, &done);
    if (!rc && !done) rc = launch_pool<T, OUT>(c, s, call, &done);
    if (!rc && !done) rc = launch_lists<T, OUT>(c, s, call);
    return rc;
}

static int check_trace_args(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const int32_t* seg_count, const int32_t* counts, int32_t n_classes) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    if (!c->has_scene) return fail(OT_ERR_NOSCENE, "ot_scene_upload has not been called");
    if (c->max_children > 2) return fail(OT_ERR_UNSUPPORTED, "more than two children per hit");
    int rc = check_rays(rays, "rays");
    if (rc) return rc;
    if (n < 0 || K < 1 || !seg_count) return fail(OT_ERR_INVALID, "bad n / max_segments / seg_count");
    if (n >= (int64_t)1 << 31) return fail(OT_ERR_INVALID, "n must be < 2^31 per launch (int32 ray index)");
    if (c->n_slots > 0 && (!counts || n_classes < 1)) return fail(OT_ERR_INVALID, "scene has limited surfaces: counts table required");
    return 0;
}

// does this scene take the rolling lists (heavy: many nodes per segment => VALU-bound, uneven path lengths) or one lane per
// ray with perfectly coalesced streams (light: HBM-bound)?  The all-features preset has no lane-per-ray form in double
// precision (it would need more than 256 registers): those scenes always take the lists.
static int fused_preset(uint32_t need) {  // smallest lane-per-ray preset that covers the scene (tables.h): 0 FA, 1 FB, 2 FE, 3 FM, 4 F_ALL
    using namespace preset;
    return (need & ~FA) == 0 ? 0 : ((need & ~FB) == 0 ? 1 : ((need & ~FE) == 0 ? 2 : ((need & ~FM) == 0 ? 3 : 4)));
}
template <class T> static bool wants_rolling(const ot_ctx* c, int32_t K) {
    const bool f64 = sizeof(T) == 8;
    return c->opt_kernel == 2 || (c->opt_kernel == 0 && c->n_nodes >= 24 && K > 2) || (f64 && (fused_preset(c->features) == 4 || !in_lds<T>(c)));
}

// the uniform_mask of a call (include/optable_hip.h: OT_UNIFORM_*)
static int check_uniform(uint32_t uniform) {
    if (uniform & ~(uint32_t)OT_UNIFORM_ALL) return fail(OT_ERR_INVALID, "uniform_mask has bits outside OT_UNIFORM_ALL");
    return 0;
}

// the resident_mask of a call (include/optable_hip.h: OT_RESIDENT_*)
static int check_resident(uint32_t resident) {
    if (resident & ~(uint32_t)OT_RESIDENT_ALL) return fail(OT_ERR_INVALID, "resident_mask has bits outside OT_RESIDENT_ALL");
    return 0;
}
// The planes every record of a lane-per-ray launch with this uniform_mask holds ONE known value in, whatever the rays do: `ray` is
// the ray's index.  `n`: a preset without Snell interfaces hands r.n to every child (trace_core.h interact: lens and mirror
// branches), so a uniform input field is a uniform plane; `intensity` likewise where every leaf multiplies it by exactly 1.
// This rule, not the caller, decides what a launch may leave unwritten: launch_fused masks the caller's word with it.
template <class T> static uint32_t resident_planes(const ot_ctx* c, uint32_t uniform, int32_t K) {
    if (!c->opt_resident || K > (int32_t)SegCount::SEGS_MAX) return 0;  // (the kernel keeps a ray's old and new count in one register: kernels.h SegCount)
    if (!c->opt_uniform) uniform = 0;
    uint32_t planes = OT_RESIDENT_RAY;
    const bool hands_on = fused_preset(c->features) == 0 && in_lds<T>(c);  // the preset FA: no F_REFRACT (tables.h; inst_fused.hip lookup)
    if (hands_on && (uniform & OT_UNIFORM_N)) planes |= OT_RESIDENT_N;
    if (hands_on && (uniform & OT_UNIFORM_INTENSITY) && c->whole_intensity) planes |= OT_RESIDENT_INTENSITY;
    return planes;
}

// the first_mask of a call (include/optable_hip.h: OT_FIRST_FIELDS)
static int check_first(uint32_t first) {
    if (first & ~(uint32_t)OT_FIRST_FIELDS) return fail(OT_ERR_INVALID, "first_mask has bits outside OT_FIRST_FIELDS");
    return 0;
}
// The record fields segment 0 of every ray holds ONE known bit pattern in: segment 0 is the input ray handed through (k_trace_fused
// stores what it loaded), so every uniform input field among the eleven a record shares with a ray, whatever the scene does.
// OT_OPT_RESIDENT = 2 keeps the planes and drops these.
static uint32_t first_fields(const ot_ctx* c, uint32_t uniform, int32_t K) {
    if (c->opt_resident != 1 || !c->opt_uniform || K > (int32_t)SegCount::SEGS_MAX) return 0;
    return uniform & (uint32_t)OT_FIRST_FIELDS;
}

// one lane per ray (k_trace_fused); OUT = SegsT<T> or SegTiles<T>
template <class T, class OUT>
static int launch_fused(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const OUT& out, int32_t pair, int32_t* seg_count, int32_t* counts,
                        int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    const bool f64 = sizeof(T) == 8;
    const int fi = fused_preset(c->features);
    const size_t bytes = image_of<T>(c).bytes;
    const bool lds = in_lds<T>(c);
    const int block = 256;
    const int64_t blocks_needed = (n + block - 1) / block;
    // Grid: small scenes (staging the blob costs nothing) get up to 256 blocks per CU, i.e. one ray per
    // lane up to 1.7e7 rays and a short grid-stride loop beyond: fresh blocks replace finished ones, which
    // balances better than 16 long-lived blocks per CU (cfg 4, 1.6e8 rays: 12.7 -> 11.8 ms fp64; flat from
    // 64 per CU on).  Scenes with a large LDS image run persistent, as many blocks per CU as the image allows.
    int per_cu = 256;
    if (lds && bytes > 16 * 1024) {  // beyond 64 B of staging per ray a short-lived workgroup no longer pays
        const int fit = (int)((160 * 1024) / (bytes + 512));
        per_cu = fit < 1 ? 1 : (fit > 8 ? 8 : fit);
    }
    if (c->opt_blocks_per_cu > 0) per_cu = c->opt_blocks_per_cu;
    const int64_t cap = (int64_t)c->n_cus * per_cu;
    const int grid = (int)(blocks_needed < cap ? blocks_needed : cap);
    // smallest instantiation that covers the scene's features; the 128-register cap is stated for the mirror / lens kernel
    // and the fp32 Snell kernel only (the fp64 Snell kernel stays within 128 registers uncapped: inst_fused.hip; nothing in
    // the grid rule above depends on the waves a SIMD holds)
    const bool mw = c->opt_minw == 4 && (fi == 0 || (fi == 1 && !f64));
    FusedKern<T, OUT> kern = fused_kernel<T, OUT>(fi, lds, mw, c->opt_nt != 0);
    if (!kern) return fail(OT_ERR_UNSUPPORTED, "no kernel instantiation for this scene / option combination");
    const LaunchShape shape = {1, block, 0, grid, (int32_t)(lds ? bytes : 0), 0, 0, std::is_same<OUT, SegTiles<T>>::value ? LL_TILES : 0};
    return launch_kernel(c, kern, shape, nullptr, nullptr, make_blob<T>(c), (T)c->unit, view<T>(rays), n, K, out, seg_count, counts, n_classes, pair,
                         c->opt_uniform ? uniform : 0u,
                         (resident & resident_planes<T>(c, uniform, K)) | ((first & first_fields(c, uniform, K)) << FIRST_SHIFT));
}

template <class T>
static int trace_fused(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                       int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    int rc = check_trace_args(c, rays, n, K, seg_count, counts, n_classes);
    if (rc) return rc;
    rc = check_segs(out);
    if (rc) return rc;
    rc = check_uniform(uniform);
    if (rc) return rc;
    rc = check_resident(resident);
    if (rc) return rc;
    rc = check_first(first);
    if (rc) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // (the rolling lists read the full arrays and write whole records: the masks end here)
    if (wants_rolling<T>(c, K)) return launch_rolling<T, SegsT<T>>(c, rays, n, K, view<T>(out), AppendCtl{nullptr, 0, 0}, seg_count, counts, n_classes);
    return launch_fused<T, SegsT<T>>(c, rays, n, K, view<T>(out), pair_ok<T>(c, out, n), seg_count, counts, n_classes, uniform, resident, first);
}

// Tiled layout: the lane-per-ray kernel only (light scenes; heavy ones have the append layout)
template <class T> static int check_tiles(const void* tiles, int64_t capacity, int64_t n, int32_t K) {
    if (!tiles || (uintptr_t)tiles % 16) return fail(OT_ERR_INVALID, "tiles must be a 16-byte aligned device pointer");
    if (capacity % 64 || capacity < ((n * K + 63) / 64) * 64) return fail(OT_ERR_CAPACITY, "tiled layout: capacity must be a multiple of 64 and hold max_segments * n_rays slots");
    return 0;
}
template <class T>
static int trace_tiled(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    int rc = check_trace_args(c, rays, n, K, seg_count, counts, n_classes);
    if (rc) return rc;
    rc = check_tiles<T>(tiles, capacity, n, K);
    if (rc) return rc;
    rc = check_uniform(uniform);
    if (rc) return rc;
    rc = check_resident(resident);
    if (rc) return rc;
    rc = check_first(first);
    if (rc) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    if (wants_rolling<T>(c, K))
        return fail(OT_ERR_UNSUPPORTED, "the tiled layout belongs to the lane-per-ray kernel (light scenes); heavy scenes write [k][ray] slots (ot_trace_*) or the append layout (ot_trace_append_*)");
    // pair = 0: the tiled kernels store one element per lane and do not read the argument (OT_OPT_PAIR_STORES governs the slot arrays)
    return launch_fused<T, SegTiles<T>>(c, rays, n, K, SegTiles<T>{(uint8_t*)tiles}, 0, seg_count, counts, n_classes, uniform, resident, first);
}

// the segment block of the append layout (ot_trace_append_*, ot_trace_trees_append_*)
template <class T> static int check_append_block(const ot_segment_block* out, const int64_t* n_slots) {
    if (!out || !out->base || out->capacity < 0 || !n_slots) return fail(OT_ERR_INVALID, "bad segment block / n_slots");
    if ((uintptr_t)out->base % 16 || out->capacity % 64) return fail(OT_ERR_INVALID, "segment block: base must be 16-byte aligned, capacity a multiple of 64");
    if (out->capacity >= ((int64_t)1 << 30) / (int64_t)(sizeof(T) / 4)) return fail(OT_ERR_INVALID, "segment block: capacity must stay below 2^30 slots (2^29 in double precision) per launch");
    return 0;
}
// Append layout: always the rolling lists (a light scene takes the planar preset FC).
template <class T>
static int trace_append(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segment_block* out, int64_t* n_slots,
                        int32_t* seg_count, int32_t* counts, int32_t n_classes) {
    int rc = check_trace_args(c, rays, n, K, seg_count, counts, n_classes);
    if (rc) return rc;
    rc = check_append_block<T>(out, n_slots);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(n_slots, 0, sizeof(int64_t), c->stream));
        return 0;
    }
    // slots per claim: one device-wide atomic per chunk.  512 keeps a cfg 3 trace (5e7 records) at 1e5 claims per launch;
    // the price is the unused tail of every wave's last chunk (holes, ray = -1: half a chunk per wave on average).
    const int32_t chunk = c->opt_append_chunk;
    const SegPlanes<T> planes = {(uint8_t*)out->base, out->capacity};
    const AppendCtl ac = {(unsigned long long*)n_slots, out->capacity, chunk};
    return launch_rolling<T, SegPlanes<T>>(c, rays, n, K, planes, ac, seg_count, counts, n_classes);
}

extern "C" {

int ot_trace_reuse_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                       int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    return trace_fused<double>(c, rays, n, K, out, seg_count, counts, n_classes, uniform, resident, first);
}
int ot_trace_reuse_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                       int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    return trace_fused<float>(c, rays, n, K, out, seg_count, counts, n_classes, uniform, resident, first);
}
int ot_trace_tiled_reuse_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                             int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    return trace_tiled<double>(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, resident, first);
}
int ot_trace_tiled_reuse_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                             int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident, uint32_t first) {
    return trace_tiled<float>(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, resident, first);
}
// (no first-segment fields: the same path with an empty mask)
int ot_trace_resident_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                          int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident) {
    return ot_trace_reuse_f64(c, rays, n, K, out, seg_count, counts, n_classes, uniform, resident, 0u);
}
int ot_trace_resident_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                          int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident) {
    return ot_trace_reuse_f32(c, rays, n, K, out, seg_count, counts, n_classes, uniform, resident, 0u);
}
int ot_trace_tiled_resident_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                                int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident) {
    return ot_trace_tiled_reuse_f64(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, resident, 0u);
}
int ot_trace_tiled_resident_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                                int32_t* counts, int32_t n_classes, uint32_t uniform, uint32_t resident) {
    return ot_trace_tiled_reuse_f32(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, resident, 0u);
}
// Which planes would such a call keep invariant on the uploaded scene (0: it would not land on the lane-per-ray kernel)?
int ot_trace_resident_plan(ot_ctx* c, int32_t real_bytes, uint32_t uniform, int64_t n, int32_t K, int32_t* planes) {
    if (!c || !planes || (real_bytes != 4 && real_bytes != 8) || n < 0 || K < 1) return fail(OT_ERR_INVALID, "ot_trace_resident_plan: bad argument");
    if (!c->has_scene) return fail(OT_ERR_NOSCENE, "ot_scene_upload has not been called");
    const int rc = check_uniform(uniform);
    if (rc) return rc;
    const bool f64 = real_bytes == 8;
    const bool fused = n > 0 && c->max_children <= 2 && !(f64 ? wants_rolling<double>(c, K) : wants_rolling<float>(c, K));
    *planes = !fused ? 0 : (int32_t)(f64 ? resident_planes<double>(c, uniform, K) : resident_planes<float>(c, uniform, K));
    return 0;
}
// ... and which record fields would its segment 0 hold the batch's one bit pattern in (0 likewise, and for planes only: OT_OPT_RESIDENT = 2)?
int ot_trace_reuse_plan(ot_ctx* c, int32_t real_bytes, uint32_t uniform, int64_t n, int32_t K, int32_t* planes, uint32_t* first_fields_out) {
    if (!first_fields_out) return fail(OT_ERR_INVALID, "ot_trace_reuse_plan: bad argument");
    const int rc = ot_trace_resident_plan(c, real_bytes, uniform, n, K, planes);
    if (rc) return rc;
    const bool fused = n > 0 && c->max_children <= 2 && !(real_bytes == 8 ? wants_rolling<double>(c, K) : wants_rolling<float>(c, K));
    *first_fields_out = fused ? first_fields(c, uniform, K) : 0u;
    return 0;
}
// (nothing resident: the same path with an empty mask)
int ot_trace_uniform_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                         int32_t* counts, int32_t n_classes, uint32_t uniform) {
    return ot_trace_resident_f64(c, rays, n, K, out, seg_count, counts, n_classes, uniform, 0u);
}
int ot_trace_uniform_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                         int32_t* counts, int32_t n_classes, uint32_t uniform) {
    return ot_trace_resident_f32(c, rays, n, K, out, seg_count, counts, n_classes, uniform, 0u);
}
int ot_trace_tiled_uniform_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                               int32_t* counts, int32_t n_classes, uint32_t uniform) {
    return ot_trace_tiled_resident_f64(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, 0u);
}
int ot_trace_tiled_uniform_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count,
                               int32_t* counts, int32_t n_classes, uint32_t uniform) {
    return ot_trace_tiled_resident_f32(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, uniform, 0u);
}
// (no uniform fields: the same path with an empty mask)
int ot_trace_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                 int32_t* counts, int32_t n_classes) {
    return ot_trace_uniform_f64(c, rays, n, K, out, seg_count, counts, n_classes, 0u);
}
int ot_trace_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count,
                 int32_t* counts, int32_t n_classes) {
    return ot_trace_uniform_f32(c, rays, n, K, out, seg_count, counts, n_classes, 0u);
}
int ot_trace_tiled_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes) {
    return ot_trace_tiled_uniform_f64(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, 0u);
}
int ot_trace_tiled_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes) {
    return ot_trace_tiled_uniform_f32(c, rays, n, K, tiles, capacity, seg_count, counts, n_classes, 0u);
}
int ot_trace_append_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segment_block* out, int64_t* n_slots,
                        int32_t* seg_count, int32_t* counts, int32_t n_classes) {
    return trace_append<double>(c, rays, n, K, out, n_slots, seg_count, counts, n_classes);
}
int ot_trace_append_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segment_block* out, int64_t* n_slots,
                        int32_t* seg_count, int32_t* counts, int32_t n_classes) {
    return trace_append<float>(c, rays, n, K, out, n_slots, seg_count, counts, n_classes);
}

}  // extern "C"

static int gen_preset(uint32_t need) {  // 0 FB (planar, no count gates), 1 FC (planar under grids), 2 FE, 3 FM, 4 F_ALL
    using namespace preset;
    return (need & ~FB) == 0 ? 0 : ((need & ~FC) == 0 ? 1 : ((need & ~FE) == 0 ? 2 : ((need & ~FM) == 0 ? 3 : 4)));
}

// What one ot_trace_tree_* / ot_trace_generation_* call launches its generations with, worked out once: the scene image, the
// LDS it takes (0: the kernels read it from L2), and the kernels of the scene's preset (tables.h).  emit_ahead and one_pass
// exist for some presets only: NULL otherwise.
template <class T> struct GenSetup {
    SceneBlob blob;
    size_t lds_bytes;
    ProbeKern<T> probe; GenKern<T> count, emit, emit_ahead; GenOneKern<T> one_pass;
};
template <class T> static int gen_setup(const ot_ctx* c, GenSetup<T>* g) {
    const int fg = gen_preset(c->features);  // smallest generation preset that covers the scene
    const bool lds = in_lds<T>(c);
    *g = {make_blob<T>(c), lds ? image_of<T>(c).bytes : 0, probe_kernel<T>(fg, lds), gen_kernel<T>(fg, lds, false), gen_kernel<T>(fg, lds, true),
          gen_ahead_kernel<T>(fg, lds), gen_one_kernel<T>(fg, lds)};
    if (g->lds_bytes > 48 * 1024)
        for (const void* k : {(const void*)g->probe, (const void*)g->count, (const void*)g->emit, (const void*)g->emit_ahead, (const void*)g->one_pass})
            if (k) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->lds_bytes));
    return 0;
}

// Everything about the arguments of ot_trace_tree_* / ot_trace_generation_* that does not depend on the size of a generation,
// refused before anything is enqueued.  `cursor`, `result`: state and result, or seg_cursor and n_next; `next`: the holders
// children are written to, under the names the header gives them.
struct NamedBuf { const GenBuf& buf; const char* name; };
static int check_generation_args(const ot_ctx* c, const GenBuf& in, const int32_t* budget, const ot_segments* out, const int64_t* cursor,
                                 const int64_t* result, const int32_t* counts, int32_t n_classes, std::initializer_list<NamedBuf> next) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    if (!c->has_scene) return fail(OT_ERR_NOSCENE, "ot_scene_upload has not been called");
    int rc = check_rays(in.rays, "rays");
    if (rc) return rc;
    for (const NamedBuf& b : next) {
        rc = check_rays(b.buf.rays, b.name);
        if (rc) return rc;
        if (!b.buf.tree_out) return fail(OT_ERR_INVALID, "bad generation arguments");
    }
    rc = check_segs(out);
    if (rc) return rc;
    if (!in.tree || !budget || !cursor || !result) return fail(OT_ERR_INVALID, "bad generation arguments");
    if (c->max_children > 2) return fail(OT_ERR_UNSUPPORTED, "more than two children per hit");
    if (c->n_slots > 0 && (!counts || n_classes < 1)) return fail(OT_ERR_INVALID, "scene has limited surfaces: counts table required");
    return 0;
}
// ... and what does: per generation, whichever kernel takes it
static int check_generation_size(const ot_ctx* c, int64_t n, int64_t next_capacity) {
    if (n < 1) return fail(OT_ERR_INVALID, "bad generation arguments");
    if (n >= (int64_t)1 << 30) return fail(OT_ERR_INVALID, "generation too large");
    if (next_capacity < n * (c->max_children < 1 ? 1 : c->max_children)) return fail(OT_ERR_CAPACITY, "next_capacity < n * max_children");
    return 0;
}

// One generation in two passes (kernels.h k_gen_pass): src's rays traced, the children into dst.
// ahead_in: src.ahead holds what the emit pass of the generation before left for these rays (children per ray if processed):
// no count pass over the rays, k_gen_recount instead.  dst.ahead, where there is one, receives the same for the children
// (next_capacity bytes); both live outside c->gen, which may be reallocated between generations.
// parent_index (OT_OPT_GEN_PARENT_INDEX, the single-generation entry points only): dst.tree_out[] receives the input index of
// each child's parent instead of its tree id.
template <class T>
static int trace_generation(ot_ctx* c, const GenSetup<T>& g, const GenBuf& src, int64_t n, int32_t* budget, const ot_segments* out,
                            int64_t out_capacity, int64_t* seg_cursor, const GenBuf& dst, int64_t next_capacity, int64_t* n_next,
                            int32_t* counts, int32_t n_classes, bool ahead_in, bool parent_index = false) {
    int rc = check_generation_size(c, n, next_capacity);
    if (rc) return rc;
    const int ns = c->n_slots;
    const int64_t n_waves = (n + 63) / 64;
    const bool reuse = gen_reuse(c) && !ahead_in;
    GenScratch<T> s;
    if (c->gen.ensure(s.carve(nullptr, n, ns, reuse))) return fail(OT_ERR_HIP, "hipMalloc of generation scratch failed");
    s.carve(c->gen.p, n, ns, reuse);
    uint8_t* const code = ahead_in ? src.ahead : s.code;  // (the look-ahead bytes are rewritten in place by k_gen_recount)
    const size_t tmp = ns > 0 ? scan_tmp_bytes<int32_t>(n) : 0, tmp_w = scan_tmp_bytes<unsigned long long>(n_waves);
    if (c->scan_tmp.ensure((tmp > tmp_w ? tmp : tmp_w) + 256)) return fail(OT_ERR_HIP, "hipMalloc of scan scratch failed");
    const int block = 256;
    const int g1 = (int)((n + block - 1) / block);
    rc = timing_begin(c);
    if (rc) return rc;
    if (!c->gen_mismatch) {
        HIP_TRY(hipMalloc((void**)&c->gen_mismatch, sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(c->gen_mismatch, 0, sizeof(unsigned long long), c->stream));
    }
    unsigned long long* const mismatch = c->gen_mismatch;  // lives with the ctx: accumulated over all generations (ot_debug_generation_mismatches)
    const GenKern<T> k_emit = dst.ahead ? g.emit_ahead : g.emit;
    const RaysT<T> rays = view<T>(src.rays);
    if (ns > 0) {  // FIFO-exact interact-count gating: probe -> per-slot scan -> rank within the tree
        HIP_TRY(hipMemsetAsync(s.probe, 0, sizeof(int32_t) * n * ns, c->stream));
        hipLaunchKernelGGL(g.probe, dim3(g1), dim3(block), g.lds_bytes, c->stream, g.blob, (T)c->unit, rays, src.tree, n, budget, counts, n_classes,
                           s.probe);
        for (int k = 0; k < ns; ++k)
            exclusive_scan<int32_t, int32_t>(c->scan_tmp.p, s.probe + (int64_t)k * n, s.probe_ex + (int64_t)k * n, n, c->stream);
        hipLaunchKernelGGL(k_gen_per_ray, dim3(g1), dim3(block), 0, c->stream, GEN_RANK, src.tree, n, ns, (const int32_t*)s.probe_ex, s.rank);
    }
    // count -> scan of the wave totals -> emit (kernels.h: k_gen_pass)
    if (ahead_in)
        hipLaunchKernelGGL(k_gen_recount, dim3(g1), dim3(block), 0, c->stream, src.tree, n, (const int32_t*)budget, code, s.wave_total, c->opt_gen_drop ? 1 : 0);
    else
        hipLaunchKernelGGL(g.count, dim3(g1), dim3(block), g.lds_bytes, c->stream, g.blob, (T)c->unit, rays, src.tree, n, budget,
                           (const int64_t*)seg_cursor, view<T>(out), out_capacity, view_out<T>(dst.rays), dst.tree_out, next_capacity, code, s.wave_total,
                           (const unsigned long long*)s.wave_prefix, counts, n_classes, (const int32_t*)s.rank, mismatch, s.hit_node, s.hit_t,
                           c->opt_gen_drop ? 1 : 0, (uint8_t*)nullptr);
    exclusive_scan<unsigned long long, unsigned long long>(c->scan_tmp.p, s.wave_total, s.wave_prefix, n_waves, c->stream);
    hipLaunchKernelGGL(k_gen_totals, dim3(1), dim3(64), 0, c->stream, (const unsigned long long*)s.wave_total,
                       (const unsigned long long*)s.wave_prefix, n_waves, s.totals, seg_cursor, n_next);
    hipLaunchKernelGGL(k_emit, dim3(g1), dim3(block), g.lds_bytes, c->stream, g.blob, (T)c->unit, rays, src.tree, n, budget,
                       (const int64_t*)(s.totals + 2), view<T>(out), out_capacity, view_out<T>(dst.rays), dst.tree_out, next_capacity, code, s.wave_total,
                       (const unsigned long long*)s.wave_prefix, counts, n_classes, (const int32_t*)s.rank, mismatch, s.hit_node, s.hit_t,
                       (c->opt_gen_drop ? 1 : 0) | (parent_index ? 2 : 0), dst.ahead);
    if (ns > 0)
        hipLaunchKernelGGL(k_gen_counts, dim3(g1), dim3(block), 0, c->stream, src.tree, src.rays->id, n, ns, s.rank, s.probe, c->slot_max, counts,
                           n_classes);
    HIP_TRY(hipGetLastError());
    return timing_end(c);
}

// Whole ray trees, a lane per tree (kernels.h k_trace_trees).  The plan: workgroups of 256 threads; QL entries per lane in LDS
// (OT_OPT_TREES_LDS_ENTRIES, default 3: eight waves per CU in double precision, sixteen in single) and the rest of the
// ceil(cap / 2) entries a tree can need in a per-wave global scratch, as long as the scratch of all resident waves stays
// within 1 GiB (caps up to ~170 in double precision); beyond that the queues are what fits and the launch is a speculation
// on small trees (full = 0).
struct TreesPlan { int32_t QL, QG, full, groups_per_cu, grid, chunk, preset, flat_cap, img_global; size_t lds_bytes; };
// Planar scenes under a top-level grid of leaves search through the wave-wide pair queue of the heavy non-branching kernel
// (pair_queue_room, flat_grid_hit): the tree kernel's presets 5 (FR) / 6 (FRP).  0: the scene does not qualify.
static int32_t trees_flat_cap(const ot_ctx* c, int* preset) {
    const int planar = planar_grid_preset(c);
    // (a tree is one lane's: no mixed lists to ask for, and the queue is tried whether or not the image will fit — trees_plan
    // drops it again when it does not; the presets 5 / 6 have no count gates)
    const int32_t flat_cap = pair_queue_room(c, planar >= 0 && c->n_slots == 0);
    if (flat_cap) *preset = 5 + planar;
    return flat_cap;
}
template <class T> static bool trees_plan(const ot_ctx* c, int32_t cap, int64_t n, TreesPlan* p) {
    const size_t image = image_of<T>(c).bytes;
    *p = TreesPlan{};
    if (!c->has_scene || c->max_children > 2 || cap < 1) return false;
    p->preset = gen_preset(c->features);
    p->flat_cap = c->opt_trees_flat ? trees_flat_cap(c, &p->preset) : 0;
    if (!tree_kernel<T, SegPlanes<T>>(p->preset)) return false;
    const size_t flat_bytes = p->flat_cap ? flat_lds_bytes<T>(p->flat_cap) : 0;
    const size_t room = 160 * 1024 - 1024, entry = (size_t)tree_entry_bytes<T>();
    size_t img = ((image + 15) & ~(size_t)15) + 4 * flat_bytes;
    if (img + 4 * entry > room || c->opt_trees_global) {  // (OT_OPT_TREES_GLOBAL_IMAGE: test knob, every scene takes this path)
        // an image no LDS holds (thousands of leaves): the all-features kernel reads it from global memory (L2), the LDS holds queues alone
        if (!tree_kernel<T, SegPlanes<T>>(4, 0)) return false;
        p->preset = 4; p->flat_cap = 0; p->img_global = 1;
        img = 0;
        // ... and the node and material records alone in LDS when they leave room for the queues (instanced runs fold thousands of
        // lattice members into a few records: the walk's dependent reads then come from LDS, only poses and grids from L2)
        const size_t head = (image_of<T>(c).head + 16 * (size_t)c->n_runs + 15) & ~(size_t)15;  // records + the run table
        if (head > 0 && head + 4 * 3 * entry <= room / 2 && c->opt_trees_global != 2 && !c->has_implicit && tree_kernel<T, SegPlanes<T>>(4, 2)) { p->img_global = 2; img = head; }
    }
    const int64_t need = ((int64_t)cap + 1) / 2, fit = (int64_t)((room - img) / (4 * entry));
    // entries in LDS: two under small caps (queues stay short: a third workgroup per CU is worth more than the third entry —
    // cfg 4 R = 0.2: 4.05 vs 4.2 ms, bushy trees under a cap of 12: 0.56 vs 0.62), three above (cap 48: 3.35 vs 3.99)
    // ... and ONE where the search is the pair queue (heavy planar scenes: their image and queues take the LDS, and a fourth workgroup
    // per CU is worth more than entries — cfg 3 with reflecting slabs 1.38 / 1.49 / 1.85 ms with one / two / three)
    const int64_t want = c->opt_trees_lds > 0 ? c->opt_trees_lds : (p->flat_cap ? 1 : (cap <= 16 ? 2 : 3));
    int64_t ql = want < need ? want : need;
    if (ql > fit) ql = fit;
    if (ql > 255) ql = 255;
    // (... but never a third entry that leaves a CU with ONE workgroup where two would fit with two entries: cfg 3 with reflecting
    // slabs in double precision, image + pair queues + rings: 4.1 ms with three entries, 3.3-3.7 with two)
    if (c->opt_trees_lds <= 0 && ql == 3 && (160 * 1024) / (img + 4 * 3 * entry + 256) < 2 && (160 * 1024) / (img + 4 * 2 * entry + 256) >= 2) ql = 2;
    p->QL = (int32_t)ql;
    p->lds_bytes = img + 4 * (size_t)ql * entry;
    const int by_lds = (int)((160 * 1024) / (p->lds_bytes + 256)), by_regs = tree_groups_by_registers<T>(p->preset);  // (waves per SIMD the kernel's registers allow)
    p->groups_per_cu = by_lds < by_regs ? (by_lds < 1 ? 1 : by_lds) : by_regs;
    // (the scratch is per workgroup of the LAUNCH: a batch of a few trees is a few workgroups, and gets long queues out of the same 1 GiB)
    const int64_t groups_needed = n > 0 ? (n + 255) / 256 : (int64_t)1 << 40, groups_most = (int64_t)c->n_cus * p->groups_per_cu;
    p->grid = (int32_t)(groups_needed < groups_most ? groups_needed : groups_most);
    const int64_t waves = (int64_t)p->grid * 4;
    // Append output: slots per claim.  A wave waits for its claim (one atomic on ONE device-wide cursor, ~2 us) at the occupancy of this
    // kernel: 512-slot chunks were 12 % of a cfg 4 R = 0.2 trace (4.06 -> 3.55 ms with 2048+).  As large as leaves the unused chunk tails
    // (one per wave) within a sixteenth of the output, 8192 at most, OT_OPT_APPEND_CHUNK at least.
    {
        const int64_t sixteenth = n > 0 ? (n * (int64_t)cap) / (waves * 16) / 64 * 64 : 8192;
        const int64_t most_chunk = sixteenth < 8192 ? sixteenth : 8192;
        p->chunk = (int32_t)(most_chunk > c->opt_append_chunk ? most_chunk : c->opt_append_chunk);
    }
    const int64_t scratch_entry = 64 * (sizeof(T) == 8 ? 96 : 48);  // lane-major records of 12 words (kernels.h)
    int64_t most = ((int64_t)1 << 30) / (waves * scratch_entry);
    if (most > 255) most = 255;  // (the kernel keeps ring positions in bytes)
    // (the scratch ring alone must hold a whole queue: pushes keep going there while the LDS entries in front of them drain)
    const int64_t qg = need > ql ? need : 0;
    p->QG = (int32_t)(qg < most ? qg : most);
    p->full = qg <= most;
    return true;
}
template <class T, class OUT>
static int launch_trees(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t cap, const OUT& out, const AppendCtl& ac, int32_t* seg_count, int32_t* counts,
                        int32_t n_classes) {
    TreesPlan p;
    if (!trees_plan<T>(c, cap, n, &p)) return fail(OT_ERR_UNSUPPORTED, "no tree kernel for this scene (a hit that emits more than two rays, or no room for the queues): use ot_trace_tree_*");
    HIP_TRY(hipSetDevice(c->device));
    const TreeKern<T, OUT> kern = tree_kernel<T, OUT>(p.preset, p.img_global == 0 ? 1 : (p.img_global == 2 ? 2 : 0));
    if (!kern) return fail(OT_ERR_UNSUPPORTED, "this scene's tree kernel writes the append layout only (ot_trace_trees_append_*)");
    const size_t scratch = (size_t)p.grid * 4 * (size_t)p.QG * 64 * (sizeof(T) == 8 ? 96 : 48);  // (the grid is persistent: the scratch is per workgroup)
    if (c->trees.ensure(scratch + 256)) return fail(OT_ERR_HIP, "hipMalloc of the tree queues failed");
    AppendCtl ctl = ac;
    if (ac.cursor) ctl.chunk = p.chunk;
    const LaunchShape shape = {4, 256, p.groups_per_cu, p.grid, (int32_t)p.lds_bytes, p.QL, p.QG, (std::is_same<OUT, SegPlanes<T>>::value ? LL_APPEND : 0) | (p.flat_cap ? LL_PAIR_QUEUE : 0)};
    return launch_kernel(c, kern, shape, nullptr, ac.cursor, make_blob<T>(c), (T)c->unit, view<T>(rays), n, cap, p.QL, p.QG, (uint8_t*)c->trees.p, out, ctl, seg_count, counts,
                         n_classes, c->opt_trees_refill_at, p.flat_cap);
}
template <class T>
static int trace_trees(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t cap, const ot_segments* out, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes) {
    int rc = check_trace_args(c, rays, n, cap, seg_count, counts, n_classes);
    if (rc) return rc;
    rc = check_segs(out);
    if (rc) return rc;
    if (n == 0) return 0;
    return launch_trees<T, SegsT<T>>(c, rays, n, cap, view<T>(out), AppendCtl{nullptr, 0, 0}, seg_count, counts, n_classes);
}
template <class T>
static int trace_trees_append(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t cap, const ot_segment_block* out, int64_t* n_slots, int32_t* seg_count,
                              int32_t* counts, int32_t n_classes) {
    int rc = check_trace_args(c, rays, n, cap, seg_count, counts, n_classes);
    if (rc) return rc;
    rc = check_append_block<T>(out, n_slots);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(n_slots, 0, sizeof(int64_t), c->stream));
        return 0;
    }
    const SegPlanes<T> planes = {(uint8_t*)out->base, out->capacity};
    const AppendCtl ac = {(unsigned long long*)n_slots, out->capacity, c->opt_append_chunk};
    return launch_trees<T, SegPlanes<T>>(c, rays, n, cap, planes, ac, seg_count, counts, n_classes);
}

// One generation in one pass (kernels.h k_gen_one): zero the tile descriptors and the ticket, launch.  src.rem: what is left of
// its tree's budget for every ray of the generation; dst.rem receives the children's.  n_in / n_out: chained launches (trace_tree).
template <class T>
static int trace_generation_one(ot_ctx* c, const GenSetup<T>& g, const GenBuf& src, int64_t n, int32_t* budget, const ot_segments* out,
                                int64_t out_capacity, int64_t* state, const GenBuf& dst, int64_t next_capacity, int32_t* counts, int32_t n_classes,
                                const int64_t* n_in, int64_t* n_out) {
    int rc = check_generation_size(c, n, next_capacity);
    if (rc) return rc;
    const int64_t n_tiles = (n + 63) / 64, n_groups = (n + 255) / 256;  // a tile = the 64 rays of one wave
    const size_t sz_desc = align_up(sizeof(unsigned long long) * n_tiles + 8);
    // (at least 64 KB: growing the scratch frees it, which waits for the device — not between the launches of a chain)
    if (c->gen.ensure(sz_desc < 65536 ? 65536 : sz_desc)) return fail(OT_ERR_HIP, "hipMalloc of generation scratch failed");
    unsigned long long* desc = (unsigned long long*)c->gen.p;
    uint32_t* ticket = (uint32_t*)(desc + n_tiles);
    rc = timing_begin(c);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(desc, 0, sizeof(unsigned long long) * n_tiles + 8, c->stream));
    hipLaunchKernelGGL(g.one_pass, dim3((unsigned)n_groups), dim3(256), g.lds_bytes, c->stream, g.blob, (T)c->unit, view<T>(src.rays), src.tree,
                       (const int32_t*)src.rem, n, budget, state, view<T>(out), out_capacity, view_out<T>(dst.rays), dst.tree_out, dst.rem, next_capacity, desc,
                       ticket, counts, n_classes, c->opt_gen_drop ? 1 : 0, n_in, n_out);
    HIP_TRY(hipGetLastError());
    return timing_end(c);
}

// The generation loop of a whole ray tree batch (optical_table.py:115-147): one launch sequence per generation, then the two
// counters read back (16 bytes, one stream synchronisation).  gen[where] holds the pending generation, its children go to
// gen[other(where)].  It stops when the queue is empty, when the next generation does not fit the buffers or the segment
// arrays (the caller grows them and calls again with the pending generation as input), or when the wall clock runs out.
template <class T>
static int trace_tree(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget, const ot_segments* out,
                      int64_t out_capacity, int64_t* state, const ot_rays* buf_a, int32_t* tree_a, const ot_rays* buf_b, int32_t* tree_b,
                      int64_t buf_capacity, int32_t* counts, int32_t n_classes, double max_seconds, int64_t* result) {
    GenBuf gen[3] = {{rays, tree}, {buf_a, tree_a, tree_a}, {buf_b, tree_b, tree_b}};
    int rc = check_generation_args(c, gen[0], budget, out, state, result, counts, n_classes, {{gen[1], "buf_a"}, {gen[2], "buf_b"}});
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    GenSetup<T> g;
    rc = gen_setup<T>(c, &g);
    if (rc) return rc;
    const int fan = c->max_children < 1 ? 1 : c->max_children;
    const auto t0 = std::chrono::steady_clock::now();
    if (!c->pinned_state) HIP_TRY(hipHostMalloc((void**)&c->pinned_state, 2 * sizeof(int64_t), hipHostMallocDefault));
    int64_t* const host_state = c->pinned_state;  // (page-locked: the copy is a DMA the stream waits for, not a staged memcpy)
    HIP_TRY(hipMemcpyAsync(host_state, state, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t written = host_state[0], cur_n = n, generations = 0, reason = 0;
    int where = 0;
    // What the launch that produced the CURRENT generation left with it: its per-ray budgets in gen[where].rem (a one-pass
    // generation; else they are seeded from budget[]), its look-ahead bytes in gen[where].ahead (a two-pass one with look-ahead)
    bool rem_valid = false, ahead_valid = false;
    // One pass per generation (k_gen_one) where OT_OPT_GEN_ONEPASS allows it and the scene has no count-limited leaves (their
    // gate needs the scans between a probe pass and the trace).  OT_OPT_GEN_ONEPASS: 1 every generation, 0 none, -1 (default)
    // the SMALL ones: a generation of a few thousand rays is a handful of tiles that are all resident at once — nothing to
    // wait for in the look-back — and one launch instead of six (count, three scan kernels, totals, emit) is what a tree of
    // six rays costs: 1.08 -> ms per table.ray_tracing call.
    constexpr int64_t ONE_PASS_SMALL = 1 << 16;
    const bool one_pass_ok = c->n_slots == 0 && c->opt_gen_onepass != 0 && n > 0 && g.one_pass;
    int64_t* chain_n = nullptr;  // two device words: sizes handed from one chained generation to the next
    if (one_pass_ok) {
        if (c->gen_rem.ensure(sizeof(int32_t) * (size_t)(n + 2 * buf_capacity) + 256)) return fail(OT_ERR_HIP, "hipMalloc of the per-ray budgets failed");
        gen[0].rem = (int32_t*)c->gen_rem.p;
        gen[1].rem = gen[0].rem + n;
        gen[2].rem = gen[1].rem + buf_capacity;
        if (!c->gen_chain) HIP_TRY(hipMalloc((void**)&c->gen_chain, 2 * sizeof(int64_t)));
        chain_n = c->gen_chain;
    }
    // Look-ahead (k_gen_pass MODE 2; OT_OPT_GEN_AHEAD): the emit pass of a two-pass generation leaves, per child, the number of
    // children that child will have; the next two-pass generation replaces its count pass over the rays by k_gen_recount over
    // those bytes.  Light scenes (no decision reuse: their search is a few planes) without count gates whose generation
    // buffers carry no `len`; a byte array of buf_capacity with each buffer.
    if (c->opt_gen_ahead != 0 && c->n_slots == 0 && !gen_reuse(c) && !gen[1].rays->length && !gen[2].rays->length && g.emit_ahead) {
        const size_t each = align_up((size_t)buf_capacity + 64);
        if (c->gen_ahead.ensure(2 * each)) return fail(OT_ERR_HIP, "hipMalloc of the look-ahead bytes failed");
        gen[1].ahead = (uint8_t*)c->gen_ahead.p;
        gen[2].ahead = gen[1].ahead + each;
    }
    while (cur_n > 0) {
        if (written + cur_n > out_capacity) { reason = 1; break; }        // the segment arrays are too small for this generation
        if (cur_n * fan > buf_capacity) { reason = 2; break; }           // ... the generation buffers for the next one
        int src = where, dst = other(where);
        if (one_pass_ok && (c->opt_gen_onepass > 0 || cur_n <= ONE_PASS_SMALL)) {
            if (!rem_valid) {
                hipLaunchKernelGGL(k_gen_per_ray, dim3((unsigned)((cur_n + 255) / 256)), dim3(256), 0, c->stream, GEN_SEED_REM, gen[src].tree, cur_n, 0,
                                   (const int32_t*)budget, gen[src].rem);
                HIP_TRY(hipGetLastError());
            }
            rc = trace_generation_one<T>(c, g, gen[src], cur_n, budget, out, out_capacity, state, gen[dst], buf_capacity, counts, n_classes, nullptr, chain_n);
            if (rc) return rc;
            rem_valid = true;
            ahead_valid = false;
            // Small trees: further generations are enqueued WITHOUT reading anything back — each launch sized for the most rays
            // the one before can have emitted, its real size taken on the device from where that one left it (k_gen_one's n_in /
            // n_out, the two words used in turn).  One read-back per chain instead of one per generation: a tree of a handful of
            // rays is launch and synchronisation latency, nothing else.
            if (max_seconds < 0 || max_seconds > 1.0) {  // (a chain is at most fifteen launches of a few microseconds)
                int64_t bound = cur_n * fan, written_bound = written + cur_n;
                for (int link = 0; link < 15 && bound <= 4096 && bound * fan <= buf_capacity && written_bound + bound <= out_capacity; ++link) {
                    src = dst;
                    dst = other(dst);
                    rc = trace_generation_one<T>(c, g, gen[src], bound, budget, out, out_capacity, state, gen[dst], buf_capacity, counts, n_classes,
                                                 chain_n + (link & 1), chain_n + (~link & 1));
                    if (rc) return rc;
                    written_bound += bound;
                    bound *= fan;
                    ++generations;
                }
            }
        } else {
            rc = trace_generation<T>(c, g, gen[src], cur_n, budget, out, out_capacity, state, gen[dst], buf_capacity, state + 1, counts, n_classes, ahead_valid);
            if (rc) return rc;
            rem_valid = false;
            ahead_valid = gen[dst].ahead != nullptr;
        }
        HIP_TRY(hipMemcpyAsync(host_state, state, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the one host synchronisation per generation (per chain of small generations)
        written = host_state[0];
        cur_n = host_state[1];
        ++generations;
        where = dst;
        if (max_seconds >= 0 && cur_n > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= max_seconds) { reason = 3; break; }
    }
    result[0] = written; result[1] = cur_n; result[2] = where; result[3] = generations; result[4] = reason;
    return 0;
}

// One generation for the caller (ot_trace_generation_*): the two passes, whatever OT_OPT_GEN_ONEPASS says
template <class T>
static int trace_one_generation(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget, const ot_segments* out,
                                int64_t out_capacity, int64_t* seg_cursor, const ot_rays* next, int32_t* next_tree, int64_t next_capacity,
                                int64_t* n_next, int32_t* counts, int32_t n_classes) {
    const GenBuf src = {rays, tree}, dst = {next, next_tree, next_tree};
    int rc = check_generation_args(c, src, budget, out, seg_cursor, n_next, counts, n_classes, {{dst, "next"}});
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    GenSetup<T> g;
    rc = gen_setup<T>(c, &g);
    if (rc) return rc;
    return trace_generation<T>(c, g, src, n, budget, out, out_capacity, seg_cursor, dst, next_capacity, n_next, counts, n_classes, false, c->opt_gen_parent);
}

extern "C" {

int ot_trace_trees_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t max_trace_num, const ot_segments* out, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes) {
    return trace_trees<double>(c, rays, n, max_trace_num, out, seg_count, counts, n_classes);
}
int ot_trace_trees_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t max_trace_num, const ot_segments* out, int32_t* seg_count, int32_t* counts,
                       int32_t n_classes) {
    return trace_trees<float>(c, rays, n, max_trace_num, out, seg_count, counts, n_classes);
}
int ot_trace_trees_append_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t max_trace_num, const ot_segment_block* out, int64_t* n_slots, int32_t* seg_count,
                              int32_t* counts, int32_t n_classes) {
    return trace_trees_append<double>(c, rays, n, max_trace_num, out, n_slots, seg_count, counts, n_classes);
}
int ot_trace_trees_append_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t max_trace_num, const ot_segment_block* out, int64_t* n_slots, int32_t* seg_count,
                              int32_t* counts, int32_t n_classes) {
    return trace_trees_append<float>(c, rays, n, max_trace_num, out, n_slots, seg_count, counts, n_classes);
}
int ot_trace_trees_plan(ot_ctx* c, int32_t real_bytes, int32_t max_trace_num, int64_t n_rays, int32_t* info) {
    if (!c || !info || (real_bytes != 4 && real_bytes != 8)) return fail(OT_ERR_INVALID, "bad ot_trace_trees_plan arguments");
    TreesPlan p;
    const bool ok = real_bytes == 8 ? trees_plan<double>(c, max_trace_num, n_rays, &p) : trees_plan<float>(c, max_trace_num, n_rays, &p);
    info[0] = ok ? 1 : 0; info[1] = p.QL + p.QG; info[2] = p.full; info[3] = p.QL;
    info[4] = p.chunk; info[5] = p.grid * 4; info[6] = info[7] = 0;
    if (ok && (real_bytes == 8 ? tree_kernel<double, SegsT<double>>(p.preset, p.img_global ? 0 : 1) != nullptr : tree_kernel<float, SegsT<float>>(p.preset, p.img_global ? 0 : 1) != nullptr))
        info[0] |= 2;  // ... and writes the [k][tree] slots too
    return 0;
}
int ot_trace_tree_f64(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget, const ot_segments* out,
                      int64_t out_capacity, int64_t* state, const ot_rays* buf_a, int32_t* tree_a, const ot_rays* buf_b, int32_t* tree_b,
                      int64_t buf_capacity, int32_t* counts, int32_t n_classes, double max_seconds, int64_t* result) {
    return trace_tree<double>(c, rays, tree, n, budget, out, out_capacity, state, buf_a, tree_a, buf_b, tree_b, buf_capacity, counts, n_classes,
                              max_seconds, result);
}
int ot_trace_tree_f32(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget, const ot_segments* out,
                      int64_t out_capacity, int64_t* state, const ot_rays* buf_a, int32_t* tree_a, const ot_rays* buf_b, int32_t* tree_b,
                      int64_t buf_capacity, int32_t* counts, int32_t n_classes, double max_seconds, int64_t* result) {
    return trace_tree<float>(c, rays, tree, n, budget, out, out_capacity, state, buf_a, tree_a, buf_b, tree_b, buf_capacity, counts, n_classes,
                             max_seconds, result);
}

int ot_trace_generation_f64(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget,
                            const ot_segments* out, int64_t out_capacity, int64_t* seg_cursor, const ot_rays* next,
                            int32_t* next_tree, int64_t next_capacity, int64_t* n_next, int32_t* counts,
                            int32_t n_classes) {
    return trace_one_generation<double>(c, rays, tree, n, budget, out, out_capacity, seg_cursor, next, next_tree, next_capacity, n_next, counts, n_classes);
}
int ot_trace_generation_f32(ot_ctx* c, const ot_rays* rays, const int32_t* tree, int64_t n, int32_t* budget,
                            const ot_segments* out, int64_t out_capacity, int64_t* seg_cursor, const ot_rays* next,
                            int32_t* next_tree, int64_t next_capacity, int64_t* n_next, int32_t* counts,
                            int32_t n_classes) {
    return trace_one_generation<float>(c, rays, tree, n, budget, out, out_capacity, seg_cursor, next, next_tree, next_capacity, n_next, counts, n_classes);
}

// What every call that reads an ot_segment_source refuses of it and of n_segments / seg_count / n_rays, in one place.
static int check_source(const ot_segment_source* src, int64_t n, const int32_t* seg_count, int64_t n_rays) {
    if (n < 0 || n >= (int64_t)1 << 31) return fail(OT_ERR_INVALID, "bad segment count");
    if (src->width != 4 && src->width != 8) return fail(OT_ERR_INVALID, "segment source: width must be 4 or 8");
    for (const void* p : src->base)
        if (!p) return fail(OT_ERR_INVALID, "segment source has a NULL field");
    if (!src->ray) return fail(OT_ERR_INVALID, "segment source has a NULL field");
    if (src->tile_stride < 64 * (int64_t)src->width || src->ray_stride < 256) return fail(OT_ERR_INVALID, "segment source: a tile stride shorter than 64 slots");
    if (n > src->capacity) return fail(OT_ERR_INVALID, "n_segments exceeds the capacity of the segment source");
    if (seg_count && (n_rays < 1 || n % n_rays != 0)) return fail(OT_ERR_INVALID, "n_segments must be a multiple of n_rays");
    if (!seg_count && n_rays > 0) return fail(OT_ERR_INVALID, "n_rays without seg_count: pass 0 for a list, -1 for a list with holes");
    return 0;
}
// One table of bin edges: finite and strictly increasing
static bool edges_ok(const double* e, int32_t count) {
    for (int32_t k = 0; k < count; ++k)
        if (!std::isfinite(e[k]) || (k && !(e[k] > e[k - 1]))) return false;
    return true;
}
static MonSource mon_source(const ot_segment_source* src) {
    MonSource ms;
    for (int f = 0; f < 7; ++f) ms.base[f] = (const uint8_t*)src->base[f];
    ms.ray = (const uint8_t*)src->ray;
    ms.tile_stride = src->tile_stride, ms.ray_stride = src->ray_stride, ms.width = src->width;
    return ms;
}

// The partition of n > 0 slots every kernel over the segments is launched on: `grid` workgroups of `iters` visits of MON_THREADS
// slots.  Straight to global memory: 8 visits up to 2^25 slots (2441 workgroups for cfg 2's 5e6) and more beyond, which keeps a
// launch at some 16 thousand workgroups however many slots.  through_lds: workgroups long enough to be worth an LDS image of
// their own, a thousand of them at most (two rounds of the chip at two a CU), each of which zeroes and flushes its image once.
struct SlotPartition { int32_t iters; int64_t grid; };
static SlotPartition slot_partition(int64_t n, bool through_lds) {
    const int32_t iters = (int32_t)std::max<int64_t>(8, through_lds ? (n + 1024 * MON_THREADS - 1) / (1024 * MON_THREADS) : n >> 22);
    const int64_t span = (int64_t)iters * MON_THREADS;
    return {iters, (n + span - 1) / span};
}

// The launches of a checked record call with n > 0: count, scan, emit, MON_MAX monitors at a time, both passes on one partition.
// first: n_monitors + 1 device words, or NULL when the caller has no use for them (scratch of the call's own then).
static int record_passes(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const MonSource& ms, int64_t n, const int32_t* seg_count,
                         int64_t n_rays, int64_t capacity, int64_t* first, int64_t* hit_index, double* Px, double* Py, double* Pz, double* t,
                         int64_t* n_total) {
    const SlotPartition sp = slot_partition(n, false);
    const int32_t most = std::min<int32_t>(n_monitors, MON_MAX);
    ot_monitor* table;
    int32_t* count;
    int64_t *off, *own_first;
    const auto carve = [&](void* base) {
        Carve cv{(uint8_t*)base};
        table = cv.take<ot_monitor>(n_monitors), count = cv.take<int32_t>(most * sp.grid + 1), off = cv.take<int64_t>(most * sp.grid + 1);
        own_first = cv.take<int64_t>(first ? 0 : n_monitors + 1);
        return cv.used;
    };
    if (c->mon.ensure(carve(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of monitor scratch failed");
    carve(c->mon.p);
    if (!first) first = own_first;
    if (c->scan_tmp.ensure(scan_tmp_bytes<int64_t>(most * sp.grid + 1) + 256)) return fail(OT_ERR_HIP, "hipMalloc of scan scratch failed");
    HIP_TRY(hipMemcpyAsync(table, mons, sizeof(ot_monitor) * (size_t)n_monitors, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(first, 0, sizeof(int64_t), c->stream));
    // MON_MAX monitors per launch; a launch takes the hits before it from first[m0], where the launch before it left them
    for (int32_t m0 = 0; m0 < n_monitors; m0 += MON_MAX) {
        const int32_t nm = std::min<int32_t>(MON_MAX, n_monitors - m0);
        hipLaunchKernelGGL(k_mon_count, dim3((unsigned)sp.grid), dim3(MON_THREADS), 0, c->stream, table + m0, nm, ms, n, sp.iters, seg_count, n_rays, count,
                           MonImage{}, MonField{}, MonBeam{});
        exclusive_scan<int32_t, int64_t>(c->scan_tmp.p, count, off, nm * sp.grid + 1, c->stream);
        hipLaunchKernelGGL(k_mon_emit, dim3((unsigned)sp.grid), dim3(MON_THREADS), 0, c->stream, table + m0, nm, ms, n, sp.iters, seg_count, n_rays, off,
                           capacity, first + m0, hit_index, Px, Py, Pz, t, n_total);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// One monitor over slot arrays: ot_monitor_record_many's passes with one monitor, room for every slot and *n_hits as the total.
int ot_monitor_record_f64(ot_ctx* c, const ot_monitor* mon, const ot_segments* segs, int64_t n, const int32_t* seg_count,
                          int64_t n_rays, int64_t* hit_index, void* Px, void* Py, void* Pz, void* t, int64_t* n_hits) {
    if (!c || !mon || !hit_index || !Px || !Py || !Pz || !t || !n_hits) return fail(OT_ERR_INVALID, "NULL argument");
    int rc = check_segs(segs);
    if (rc) return rc;
    // plain arrays of doubles: 64-slot "tiles" back to back, room for the n slots asked for
    const ot_segment_source src = {{segs->ox, segs->oy, segs->oz, segs->dx, segs->dy, segs->dz, segs->length}, segs->ray, 512, 256, n, 8};
    rc = check_source(&src, n, seg_count, n_rays);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(n_hits, 0, sizeof(int64_t), c->stream));
        return 0;
    }
    return record_passes(c, mon, 1, mon_source(&src), n, seg_count, n_rays, n, nullptr, hit_index, (double*)Px, (double*)Py, (double*)Pz, (double*)t,
                         n_hits);
}

int ot_monitor_record_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const ot_segment_source* src, int64_t n,
                           const int32_t* seg_count, int64_t n_rays, int64_t capacity, int64_t* first, int64_t* hit_index, void* Px, void* Py,
                           void* Pz, void* t, int64_t* n_total) {
    if (!c || !mons || !src || !first || !hit_index || !Px || !Py || !Pz || !t || !n_total) return fail(OT_ERR_INVALID, "NULL argument");
    if (n_monitors < 1) return fail(OT_ERR_INVALID, "n_monitors must be at least 1");
    if (const int rc = check_source(src, n, seg_count, n_rays)) return rc;
    if (capacity < 0) return fail(OT_ERR_INVALID, "negative output capacity");
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(first, 0, sizeof(int64_t) * ((size_t)n_monitors + 1), c->stream));
        HIP_TRY(hipMemsetAsync(n_total, 0, sizeof(int64_t), c->stream));
        return 0;
    }
    return record_passes(c, mons, n_monitors, mon_source(src), n, seg_count, n_rays, capacity, first, hit_index, (double*)Px, (double*)Py,
                         (double*)Pz, (double*)t, n_total);
}

// Fluence maps: k_seg_raster over the segments as they lie (misc_kernels.h).  Through LDS while the image fits the budget of
// ot_monitor_image_many (12 bytes a pixel) — on its partition, workgroups long enough to be worth an image of their own — else
// on ot_monitor_record_many's partition with every piece a global atomic.  optable_amd/engine.py fluence_plan says the same.
int ot_fluence_map(ot_ctx* c, const double* axes, const double* u_edges, int32_t nu, const double* v_edges, int32_t nv, double w_lo, double w_hi,
                   const ot_segment_source* src, const void* intensity, int64_t n, const int32_t* seg_count, int64_t n_rays,
                   unsigned long long* counts, double* fluence, unsigned long long* skipped, int32_t accumulate) {
    if (!c || !axes || !u_edges || !v_edges || !src || !counts || !fluence || !skipped) return fail(OT_ERR_INVALID, "NULL argument");
    if (nu < 1 || nv < 1) return fail(OT_ERR_INVALID, "nu and nv must be at least 1");
    if ((int64_t)nu * nv > SEG_RASTER_MAX_PIXELS) return fail(OT_ERR_INVALID, "nu * nv exceeds 2^24 pixels");
    if (accumulate != 0 && accumulate != 1) return fail(OT_ERR_INVALID, "accumulate must be 0 or 1");
    if (const int rc = check_source(src, n, seg_count, n_rays)) return rc;
    if (!edges_ok(u_edges, nu + 1) || !edges_ok(v_edges, nv + 1)) return fail(OT_ERR_INVALID, "edges must be finite and strictly increasing");
    if (!(w_lo <= w_hi)) return fail(OT_ERR_INVALID, "w_lo must not exceed w_hi");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(axes[k])) return fail(OT_ERR_INVALID, "axes must be finite");
    HIP_TRY(hipSetDevice(c->device));
    const size_t pixels = (size_t)nu * nv;
    if (!accumulate) {
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * pixels, c->stream));
        HIP_TRY(hipMemsetAsync(fluence, 0, sizeof(double) * pixels, c->stream));
        HIP_TRY(hipMemsetAsync(skipped, 0, sizeof(unsigned long long), c->stream));
    }
    if (n == 0) return 0;
    const bool lds = pixels <= (size_t)MON_IMG_LDS_BINS;
    const SlotPartition sp = slot_partition(n, lds);
    double* d_edges;
    const auto carve = [&](void* base) {
        Carve cv{(uint8_t*)base};
        d_edges = cv.take<double>((int64_t)nu + nv + 2);
        return cv.used;
    };
    if (c->mon.ensure(carve(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of monitor scratch failed");
    carve(c->mon.p);
    HIP_TRY(hipMemcpyAsync(d_edges, u_edges, sizeof(double) * ((size_t)nu + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_edges + nu + 1, v_edges, sizeof(double) * ((size_t)nv + 1), hipMemcpyHostToDevice, c->stream));
    SegRaster r{};
    r.counts = counts, r.fluence = fluence, r.skipped = skipped;
    r.ue = d_edges, r.ve = d_edges + nu + 1;
    r.intensity = (const uint8_t*)intensity;
    for (int k = 0; k < 9; ++k) r.axes[k] = axes[k];
    r.w_lo = w_lo, r.w_hi = w_hi;
    r.nu = nu, r.nv = nv, r.lds_pixels = lds ? (int32_t)pixels : 0;
    hipLaunchKernelGGL(k_seg_raster, dim3((unsigned)sp.grid), dim3(MON_THREADS), (size_t)r.lds_pixels * 12, c->stream, mon_source(src), n, sp.iters,
                       seg_count, n_rays, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

// What the reductions of k_mon_spots (ot_monitor_spots_many, ot_monitor_spot_groups_many, ot_monitor_wavefront_many, ot_monitor_wavefront_groups_many; misc_kernels.h) take alike, and what
// they refuse of it alike: after their own NULL, size and enum refusals (a size before any array of that size is read), before
// their own tables' and before anything is zeroed or launched.
struct ReduceCall {
    ot_ctx* c; const ot_monitor* mons; int32_t n_monitors; const double* axes;
    const ot_segment_source* src; const void* intensity; int64_t n; const int32_t* seg_count; int64_t n_rays;
    int64_t* counts; double* sums; int32_t accumulate;
};
static int check_reduce_call(const ReduceCall& a) {
    if (a.accumulate != 0 && a.accumulate != 1) return fail(OT_ERR_INVALID, "accumulate must be 0 or 1");
    if (const int rc = check_source(a.src, a.n, a.seg_count, a.n_rays)) return rc;
    for (int64_t k = 0; k < 6 * (int64_t)a.n_monitors; ++k)
        if (!std::isfinite(a.axes[k])) return fail(OT_ERR_INVALID, "axes must be finite");
    return 0;
}
// A mode, as its caller describes it to reduce_call: `cells` of the call, `cells_a_launch` of them a launch at `values` doubles each
// (optable_amd/engine.py _cell_plan: the same list), the int64 counts and double sums a call that does not accumulate zeroes,
// and the mode's host tables: `doubles` doubles each, whose device copy goes to MonSpots::*to (host NULL: none).
struct ReduceTable { const double* host; int64_t doubles; const double* MonSpots::*to; };
struct ReduceMode { int64_t cells; int32_t cells_a_launch, values; size_t n_counts, n_sums; ReduceTable tables[3]; };
// The shared half of a checked call: counts and sums zeroed unless they are kept, nothing more for n = 0; else the monitors, axes
// and tables to the device and one launch per `cells_a_launch` cells, all on the partition of the LDS image passes: at most 1024
// workgroups, four a CU, which bounds the partials (1024 rows of a launch's values: 14 MB for a full group of any mode) and the
// last workgroup's loop over them.  One ticket per launch, zeroed together.  A new mode is a new caller: its checks, its ReduceMode
// and, in `spots`, its own MonSpots fields by name.
static int reduce_call(const ReduceCall& a, const ReduceMode& mode, MonSpots spots) {
    ot_ctx* c = a.c;
    HIP_TRY(hipSetDevice(c->device));
    if (!a.accumulate) {
        HIP_TRY(hipMemsetAsync(a.counts, 0, sizeof(int64_t) * mode.n_counts, c->stream));
        HIP_TRY(hipMemsetAsync(a.sums, 0, sizeof(double) * mode.n_sums, c->stream));
    }
    if (a.n == 0) return 0;
    const SlotPartition sp = slot_partition(a.n, true);
    const int64_t launches = (mode.cells + mode.cells_a_launch - 1) / mode.cells_a_launch;
    const int64_t most = std::min<int64_t>(mode.cells, mode.cells_a_launch);
    const ReduceTable up[4] = {{a.axes, 6 * (int64_t)a.n_monitors, &MonSpots::axes}, mode.tables[0], mode.tables[1], mode.tables[2]};
    ot_monitor* table;
    double *d_up[4], *partials;
    unsigned int* tickets;
    const auto carve = [&](void* base) {
        Carve cv{(uint8_t*)base};
        table = cv.take<ot_monitor>(a.n_monitors), partials = cv.take<double>(sp.grid * most * mode.values), tickets = cv.take<unsigned int>(launches);
        for (int k = 0; k < 4; ++k) d_up[k] = cv.take<double>(up[k].doubles, up[k].host);
        return cv.used;
    };
    if (c->mon.ensure(carve(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of monitor scratch failed");
    carve(c->mon.p);
    HIP_TRY(hipMemcpyAsync(table, a.mons, sizeof(ot_monitor) * (size_t)a.n_monitors, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < 4; ++k)
        if (up[k].host) {
            HIP_TRY(hipMemcpyAsync(d_up[k], up[k].host, sizeof(double) * (size_t)up[k].doubles, hipMemcpyHostToDevice, c->stream));
            spots.*up[k].to = d_up[k];
        }
    HIP_TRY(hipMemsetAsync(tickets, 0, sizeof(unsigned int) * (size_t)launches, c->stream));
    spots.intensity = (const uint8_t*)a.intensity, spots.partials = partials, spots.ticket = tickets;
    spots.counts = (long long*)a.counts, spots.sums = a.sums, spots.accumulate = a.accumulate, spots.values = mode.values;
    // (the launches of a call share the partials: they run one after the other on the stream)
    for (int64_t cell0 = 0; cell0 < mode.cells; cell0 += mode.cells_a_launch, ++spots.ticket) {
        spots.cell0 = (int32_t)cell0, spots.n_cells = (int32_t)std::min<int64_t>(mode.cells_a_launch, mode.cells - cell0);
        const size_t lds_bytes = std::max<size_t>(sizeof(double) * MON_WAVES * mode.values * (size_t)spots.n_cells, MON_SPOT_LDS_MIN);
        spots.lds_doubles = (int32_t)(lds_bytes / sizeof(double));
        hipLaunchKernelGGL(k_mon_spots, dim3((unsigned)sp.grid), dim3(MON_THREADS), lds_bytes, c->stream, table, mon_source(a.src), a.n, sp.iters,
                           a.seg_count, a.n_rays, spots);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Spot statistics: a cell per (monitor, plane) of the list [monitor][offset], 7 doubles, MON_SPOT_CELLS cells a launch
// (optable_amd/engine.py spots_plan).
int ot_monitor_spots_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* centre, const double* offsets,
                          int32_t n_offsets, const ot_segment_source* src, const void* intensity, int64_t n, const int32_t* seg_count,
                          int64_t n_rays, int64_t* counts, double* sums, int32_t accumulate) {
    if (!c || !mons || !axes || !centre || !offsets || !src || !counts || !sums) return fail(OT_ERR_INVALID, "NULL argument");
    if (n_monitors < 1) return fail(OT_ERR_INVALID, "n_monitors must be at least 1");
    if (n_offsets < 1) return fail(OT_ERR_INVALID, "n_offsets must be at least 1");
    const int64_t cells = (int64_t)n_monitors * n_offsets;
    if (cells > (int64_t)1 << 20) return fail(OT_ERR_INVALID, "n_monitors * n_offsets exceeds 2^20 cells");
    const ReduceCall a{c, mons, n_monitors, axes, src, intensity, n, seg_count, n_rays, counts, sums, accumulate};
    if (const int rc = check_reduce_call(a)) return rc;
    for (int64_t k = 0; k < 2 * (int64_t)n_monitors; ++k)
        if (!std::isfinite(centre[k])) return fail(OT_ERR_INVALID, "centre must be finite");
    for (int32_t k = 0; k < n_offsets; ++k)
        if (!std::isfinite(offsets[k])) return fail(OT_ERR_INVALID, "offsets must be finite");
    MonSpots spots{};
    spots.n_off = n_offsets;
    return reduce_call(a, {cells, MON_SPOT_CELLS, MON_SPOT_VALUES, (size_t)cells, 6 * (size_t)cells,
                           {{centre, 2 * (int64_t)n_monitors, &MonSpots::centre}, {offsets, n_offsets, &MonSpots::offsets}}}, spots);
}

// Spot statistics per ray group: k_mon_spots in its group mode, a cell per (monitor, plane, group) of the list [monitor][offset][group],
// 7 doubles; a launch takes whole (monitor, plane) pairs, (MON_SPOT_CELLS / n_groups) * n_groups cells (optable_amd/engine.py
// spot_groups_plan).  `groups` stays where it is, on the device.
int ot_monitor_spot_groups_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* centre,
                                const double* offsets, int32_t n_offsets, const int32_t* groups, int64_t n_group_ids, int32_t n_groups,
                                const ot_segment_source* src, const void* intensity, int64_t n, const int32_t* seg_count, int64_t n_rays,
                                int64_t* counts, double* sums, int32_t accumulate) {
    static_assert(OT_SPOT_GROUPS_MAX == MON_SPOT_CELLS, "one pair of a launch: every group of it a cell in LDS");
    if (!c || !mons || !axes || !centre || !offsets || !src || !counts || !sums) return fail(OT_ERR_INVALID, "NULL argument");
    if (!groups) return fail(OT_ERR_INVALID, "NULL argument: groups");
    if (n_monitors < 1) return fail(OT_ERR_INVALID, "n_monitors must be at least 1");
    if (n_offsets < 1) return fail(OT_ERR_INVALID, "n_offsets must be at least 1");
    if (n_groups < 1 || n_groups > OT_SPOT_GROUPS_MAX) return fail(OT_ERR_INVALID, "n_groups must be 1 .. 256");
    if (n_group_ids < 1 || n_group_ids > INT32_MAX) return fail(OT_ERR_INVALID, "n_group_ids must be 1 .. 2^31 - 1");
    const int64_t pairs = (int64_t)n_monitors * n_offsets, cells = pairs * n_groups;
    if (pairs > (int64_t)1 << 20 || cells > (int64_t)1 << 20) return fail(OT_ERR_INVALID, "n_monitors * n_offsets * n_groups exceeds 2^20 cells");
    const ReduceCall a{c, mons, n_monitors, axes, src, intensity, n, seg_count, n_rays, counts, sums, accumulate};
    if (const int rc = check_reduce_call(a)) return rc;
    for (int64_t k = 0; k < 2 * (int64_t)n_monitors; ++k)
        if (!std::isfinite(centre[k])) return fail(OT_ERR_INVALID, "centre must be finite");
    for (int32_t k = 0; k < n_offsets; ++k)
        if (!std::isfinite(offsets[k])) return fail(OT_ERR_INVALID, "offsets must be finite");
    MonSpots spots{};
    spots.n_off = n_offsets;
    spots.groups = groups, spots.n_group_ids = (int32_t)n_group_ids, spots.n_groups = n_groups;
    return reduce_call(a, {cells, MON_SPOT_CELLS / n_groups * n_groups, MON_SPOT_VALUES, (size_t)cells, 6 * (size_t)cells,
                           {{centre, 2 * (int64_t)n_monitors, &MonSpots::centre}, {offsets, n_offsets, &MonSpots::offsets}}}, spots);
}

// Wavefront error: k_mon_spots in its wavefront mode, a cell per monitor of 63 doubles, MON_WAVEFRONT_CELLS monitors a launch
// (optable_amd/engine.py wavefront_plan): 28 x 63 doubles a row of the partials, what a full group of spots takes.
int ot_monitor_wavefront_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                              const double* reference, int32_t coordinates, const double* pupil, const double* piston,
                              const ot_segment_source* src, const void* intensity, const void* n_index, const void* pathlength, int64_t n,
                              const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* sums, int32_t accumulate) {
    static_assert(MON_WAVEFRONT_CELLS == OT_WAVEFRONT_MONITORS && MON_WAVEFRONT_SUMS == OT_WAVEFRONT_SUMS, "the header's constants");
    if (!c || !mons || !axes || !reference || !pupil || !piston || !src || !n_index || !pathlength || !counts || !sums)
        return fail(OT_ERR_INVALID, "NULL argument");
    if (n_monitors < 1 || n_monitors > 1 << 20) return fail(OT_ERR_INVALID, "n_monitors must be 1 .. 2^20");
    if (reference_kind != 0 && reference_kind != 1) return fail(OT_ERR_INVALID, "reference_kind must be 0 (focus) or 1 (direction)");
    if (coordinates != 0 && coordinates != 1) return fail(OT_ERR_INVALID, "coordinates must be 0 (direction) or 1 (position)");
    const ReduceCall a{c, mons, n_monitors, axes, src, intensity, n, seg_count, n_rays, counts, sums, accumulate};
    if (const int rc = check_reduce_call(a)) return rc;
    if (src->width != 8) return fail(OT_ERR_INVALID, "a wavefront needs double-precision segments: width must be 8");
    for (int64_t m = 0; m < n_monitors; ++m) {
        const double *r = reference + 3 * m, *p = pupil + 3 * m;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2])) return fail(OT_ERR_INVALID, "reference must be finite");
        if (reference_kind == 1 && r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0) return fail(OT_ERR_INVALID, "the direction of a plane wave must not be zero");
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail(OT_ERR_INVALID, "pupil must be finite");
        if (!(p[2] > 0.0)) return fail(OT_ERR_INVALID, "the pupil's radius must be positive");
        if (!std::isfinite(piston[m])) return fail(OT_ERR_INVALID, "piston must be finite");
    }
    MonSpots spots{};
    spots.n_off = 1;  // a cell is a monitor
    spots.kind = reference_kind, spots.coordinates = coordinates;
    spots.n_index = (const uint8_t*)n_index, spots.pathlength = (const uint8_t*)pathlength;
    return reduce_call(a, {n_monitors, MON_WAVEFRONT_CELLS, MON_WAVEFRONT_VALUES, 2 * (size_t)n_monitors, MON_WAVEFRONT_SUMS * (size_t)n_monitors,
                           {{reference, 3 * (int64_t)n_monitors, &MonSpots::reference}, {pupil, 3 * (int64_t)n_monitors, &MonSpots::pupil},
                            {piston, n_monitors, &MonSpots::piston}}}, spots);
}

// Wavefront error per ray group: k_mon_spots in the wavefront mode's group mode, a cell per (monitor, group) of the list
// [monitor][group], 63 doubles, MON_WAVEFRONT_CELLS consecutive cells a launch wherever they fall in a monitor
// (optable_amd/engine.py wavefront_groups_plan); reference, pupil and piston are tables by cell.  `groups` stays on the device.
int ot_monitor_wavefront_groups_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                                     const double* reference, int32_t coordinates, const double* pupil, const double* piston,
                                     const int32_t* groups, int64_t n_group_ids, int32_t n_groups, const ot_segment_source* src,
                                     const void* intensity, const void* n_index, const void* pathlength, int64_t n, const int32_t* seg_count,
                                     int64_t n_rays, int64_t* counts, double* sums, int32_t accumulate) {
    if (!c || !mons || !axes || !reference || !pupil || !piston || !src || !n_index || !pathlength || !counts || !sums)
        return fail(OT_ERR_INVALID, "NULL argument");
    if (!groups) return fail(OT_ERR_INVALID, "NULL argument: groups");
    if (n_monitors < 1 || n_monitors > 1 << 20) return fail(OT_ERR_INVALID, "n_monitors must be 1 .. 2^20");
    if (n_groups < 1 || n_groups > OT_SPOT_GROUPS_MAX) return fail(OT_ERR_INVALID, "n_groups must be 1 .. 256");
    if (n_group_ids < 1 || n_group_ids > INT32_MAX) return fail(OT_ERR_INVALID, "n_group_ids must be 1 .. 2^31 - 1");
    const int64_t cells = (int64_t)n_monitors * n_groups;
    if (cells > OT_WAVEFRONT_GROUP_CELLS_MAX) return fail(OT_ERR_INVALID, "n_monitors * n_groups exceeds 4096 cells");
    if (reference_kind != 0 && reference_kind != 1) return fail(OT_ERR_INVALID, "reference_kind must be 0 (focus) or 1 (direction)");
    if (coordinates != 0 && coordinates != 1) return fail(OT_ERR_INVALID, "coordinates must be 0 (direction) or 1 (position)");
    const ReduceCall a{c, mons, n_monitors, axes, src, intensity, n, seg_count, n_rays, counts, sums, accumulate};
    if (const int rc = check_reduce_call(a)) return rc;
    if (src->width != 8) return fail(OT_ERR_INVALID, "a wavefront needs double-precision segments: width must be 8");
    for (int64_t k = 0; k < cells; ++k) {
        const double *r = reference + 3 * k, *p = pupil + 3 * k;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2])) return fail(OT_ERR_INVALID, "reference must be finite");
        if (reference_kind == 1 && r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0) return fail(OT_ERR_INVALID, "the direction of a plane wave must not be zero");
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail(OT_ERR_INVALID, "pupil must be finite");
        if (!(p[2] > 0.0)) return fail(OT_ERR_INVALID, "the pupil's radius must be positive");
        if (!std::isfinite(piston[k])) return fail(OT_ERR_INVALID, "piston must be finite");
    }
    MonSpots spots{};
    spots.n_off = 1;
    spots.kind = reference_kind, spots.coordinates = coordinates;
    spots.n_index = (const uint8_t*)n_index, spots.pathlength = (const uint8_t*)pathlength;
    spots.groups = groups, spots.n_group_ids = (int32_t)n_group_ids, spots.n_groups = n_groups;
    return reduce_call(a, {cells, MON_WAVEFRONT_CELLS, MON_WAVEFRONT_VALUES, 2 * (size_t)cells, MON_WAVEFRONT_SUMS * (size_t)cells,
                           {{reference, 3 * cells, &MonSpots::reference}, {pupil, 3 * cells, &MonSpots::pupil}, {piston, cells, &MonSpots::piston}}}, spots);
}

// How the detector-image calls (ot_monitor_image_many / _field_many / _beam_many / _wave_many) walk n_monitors monitors of nby x nbz
// bins: `passes` launches of at most `per_pass` monitors each, as even as they come (8 monitors of 30 x 30: 4 + 4, not 6 + 2),
// through LDS when a pass's bins fit the mode's `budget` (MON_IMG_LDS_BINS; MON_FIELD_LDS_BINS: 8 monitors go 3 + 3 + 2;
// MON_BEAM_LDS_BINS: 6 go 3 + 3; MON_WAVE_LDS_BINS: 4 go 2 + 2), else (one monitor alone does not fit) MON_MAX at a time straight
// to global memory.  optable_amd/engine.py image_plan / field_plan / beam_plan / wave_plan say the same.
struct ImagePlan {
    int32_t per_pass, passes;
    bool lds;
};
static ImagePlan image_plan(int32_t n_monitors, int32_t nby, int32_t nbz, int32_t budget) {
    const int64_t bins = (int64_t)nby * nbz;
    ImagePlan p;
    p.lds = bins <= budget;
    const int32_t most = p.lds ? (int32_t)std::min<int64_t>(MON_MAX, budget / bins) : MON_MAX;
    p.passes = (n_monitors + most - 1) / most;
    p.per_pass = (n_monitors + p.passes - 1) / p.passes;
    return p;
}

// What the four calls take alike, and what they refuse of it alike (their other outputs apart), before anything is launched or
// zeroed.  counts: the [n_monitors][nby][nbz] image every mode has.
struct ImageCall {
    ot_ctx* c; const ot_monitor* mons; int32_t n_monitors; const double *axes, *edges; int32_t nby, nbz;
    const ot_segment_source* src; const void* intensity; int64_t n; const int32_t* seg_count; int64_t n_rays;
    int64_t* counts; int32_t accumulate;
};
static int check_image_call(const ImageCall& a) {
    if (!a.c || !a.mons || !a.axes || !a.edges || !a.src || !a.counts) return fail(OT_ERR_INVALID, "NULL argument");
    if (a.n_monitors < 1) return fail(OT_ERR_INVALID, "n_monitors must be at least 1");
    if (a.nby < 1 || a.nbz < 1) return fail(OT_ERR_INVALID, "nby and nbz must be at least 1");
    if ((int64_t)a.nby * a.nbz > MON_IMG_MAX_BINS) return fail(OT_ERR_INVALID, "nby * nbz exceeds 2^24 bins per monitor");
    if (a.accumulate != 0 && a.accumulate != 1) return fail(OT_ERR_INVALID, "accumulate must be 0 or 1");
    if (const int rc = check_source(a.src, a.n, a.seg_count, a.n_rays)) return rc;
    if (!a.intensity) return fail(OT_ERR_INVALID, "NULL intensity");
    const int32_t n_edges = a.nby + a.nbz + 2;
    for (int32_t m = 0; m < a.n_monitors; ++m) {
        const double* e = a.edges + (int64_t)m * n_edges;
        if (!edges_ok(e, a.nby + 1) || !edges_ok(e + a.nby + 1, a.nbz + 1)) return fail(OT_ERR_INVALID, "edges must be finite and strictly increasing");
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(a.axes[6 * (int64_t)m + k])) return fail(OT_ERR_INVALID, "axes must be finite");
    }
    return 0;
}
// ... and what the coherent and the beam modes refuse alike of their wavelengths and their amplitude
static int check_wavelength_args(const double* wavelength, int64_t n_wavelengths, double wavelength_uniform) {
    if (wavelength && (n_wavelengths < 1 || n_wavelengths >= (int64_t)1 << 31)) return fail(OT_ERR_INVALID, "n_wavelengths must be at least 1 (and below 2^31)");
    if (!wavelength && !(std::isfinite(wavelength_uniform) && wavelength_uniform > 0.0))
        return fail(OT_ERR_INVALID, "wavelength_uniform must be finite and > 0 when there is no wavelength array");
    return 0;
}
static int check_amplitude_mode(int32_t amplitude_mode) {
    return amplitude_mode != 0 && amplitude_mode != 1 ? fail(OT_ERR_INVALID, "amplitude_mode must be 0 (sqrt) or 1 (linear)") : 0;
}

// A mode of the detector images, as its caller describes it to image_call: how much LDS its kernel takes (`strips` bytes in front
// of `bytes_a_bin` for each of at most `lds_budget` bins), the outputs it has next to `counts` (`planes`: [n_monitors][nby][nbz]
// doubles; `tallies`: one int64 each; NULL where a mode has fewer) ...
struct ImageMode {
    int32_t lds_budget; size_t bytes_a_bin, strips;
    double* planes[2]; int64_t* tallies[2];
};
// ... and what its `launch` is handed for one pass: the pass's monitors, the partition and LDS bytes to launch on, `img` with the
// counts, edges and axes of the pass's first monitor, and `first_bin`, where that monitor's image starts in every plane.
struct ImagePass {
    const ot_monitor* table; int32_t nm; MonSource ms; SlotPartition sp; size_t lds_bytes, first_bin;
    MonImage img;
};

// The shared half of a checked call: the outputs zeroed unless they are kept, nothing more for n = 0; else the monitors, edges and
// axes to the device and one `launch` per pass of the plan.  A new mode is a new caller: its checks, its ImageMode, its launch.
static int image_call(const ImageCall& a, const ImageMode& mode, const std::function<void(const ImagePass&)>& launch) {
    ot_ctx* c = a.c;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bins = (size_t)a.nby * a.nbz;
    if (!a.accumulate) {
        HIP_TRY(hipMemsetAsync(a.counts, 0, sizeof(int64_t) * bins * a.n_monitors, c->stream));
        for (double* plane : mode.planes)
            if (plane) HIP_TRY(hipMemsetAsync(plane, 0, sizeof(double) * bins * a.n_monitors, c->stream));
        for (int64_t* tally : mode.tallies)
            if (tally) HIP_TRY(hipMemsetAsync(tally, 0, sizeof(int64_t), c->stream));
    }
    if (a.n == 0) return 0;
    const ImagePlan plan = image_plan(a.n_monitors, a.nby, a.nbz, mode.lds_budget);
    const int32_t n_edges = a.nby + a.nbz + 2;
    ot_monitor* table;
    double *d_edges, *d_axes;
    const auto carve = [&](void* base) {
        Carve cv{(uint8_t*)base};
        table = cv.take<ot_monitor>(a.n_monitors), d_edges = cv.take<double>((int64_t)a.n_monitors * n_edges), d_axes = cv.take<double>((int64_t)a.n_monitors * 6);
        return cv.used;
    };
    if (c->mon.ensure(carve(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of monitor scratch failed");
    carve(c->mon.p);
    HIP_TRY(hipMemcpyAsync(table, a.mons, sizeof(ot_monitor) * (size_t)a.n_monitors, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_edges, a.edges, sizeof(double) * (size_t)a.n_monitors * n_edges, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_axes, a.axes, sizeof(double) * (size_t)a.n_monitors * 6, hipMemcpyHostToDevice, c->stream));
    ImagePass pass{};
    pass.ms = mon_source(a.src);
    pass.sp = slot_partition(a.n, true);  // (the long workgroups on the global path too)
    pass.img.intensity = (const uint8_t*)a.intensity;
    pass.img.nby = a.nby, pass.img.nbz = a.nbz;
    for (int32_t m0 = 0; m0 < a.n_monitors; m0 += plan.per_pass) {
        pass.table = table + m0, pass.nm = std::min<int32_t>(plan.per_pass, a.n_monitors - m0);
        pass.first_bin = m0 * bins;
        pass.img.counts = (unsigned long long*)a.counts + pass.first_bin;
        pass.img.edges = d_edges + (int64_t)m0 * n_edges, pass.img.axes = d_axes + (int64_t)m0 * 6;
        pass.img.lds_bins = plan.lds ? (int32_t)(pass.nm * bins) : 0;
        pass.lds_bytes = mode.strips + (size_t)pass.img.lds_bins * mode.bytes_a_bin;
        launch(pass);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// k_mon_count in one of its image modes (no per-workgroup counts): fld.re and beam.power NULL for plain images
static void launch_count(const ImageCall& a, const ImagePass& p, const MonImage& img, const MonField& fld, const MonBeam& beam) {
    hipLaunchKernelGGL(k_mon_count, dim3((unsigned)p.sp.grid), dim3(MON_THREADS), p.lds_bytes, a.c->stream, p.table, p.nm, p.ms, a.n, p.sp.iters,
                       a.seg_count, a.n_rays, (int32_t*)nullptr, img, fld, beam);
}

int ot_monitor_image_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges, int32_t nby,
                          int32_t nbz, const ot_segment_source* src, const void* intensity, int64_t n, const int32_t* seg_count,
                          int64_t n_rays, int64_t* counts, double* weights, int32_t accumulate) {
    if (!weights) return fail(OT_ERR_INVALID, "NULL argument");
    const ImageCall a{c, mons, n_monitors, axes, edges, nby, nbz, src, intensity, n, seg_count, n_rays, counts, accumulate};
    if (const int rc = check_image_call(a)) return rc;
    return image_call(a, {MON_IMG_LDS_BINS, 12, 0, {weights}, {}}, [&](const ImagePass& p) {
        MonImage img = p.img;
        img.weights = weights + p.first_bin;
        launch_count(a, p, img, MonField{}, MonBeam{});
    });
}

int ot_monitor_field_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges, int32_t nby,
                          int32_t nbz, const ot_segment_source* src, const void* intensity, const void* n_index, const void* pathlength,
                          const double* wavelength, int64_t n_wavelengths, double wavelength_uniform, int32_t amplitude_mode, int64_t n,
                          const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* re, double* im, int64_t* skipped,
                          int32_t accumulate) {
    if (!re || !im || !skipped) return fail(OT_ERR_INVALID, "NULL argument");
    const ImageCall a{c, mons, n_monitors, axes, edges, nby, nbz, src, intensity, n, seg_count, n_rays, counts, accumulate};
    if (const int rc = check_image_call(a)) return rc;
    if (src->width != 8) return fail(OT_ERR_INVALID, "a field needs double-precision segments: width must be 8");
    if (!n_index || !pathlength) return fail(OT_ERR_INVALID, "NULL n_index or pathlength");
    if (const int rc = check_wavelength_args(wavelength, n_wavelengths, wavelength_uniform)) return rc;
    if (const int rc = check_amplitude_mode(amplitude_mode)) return rc;
    MonField fld{};
    fld.n_index = (const uint8_t*)n_index, fld.pathlength = (const uint8_t*)pathlength;
    fld.lam = {wavelength, (unsigned long long*)skipped, wavelength_uniform, (int32_t)n_wavelengths}, fld.amplitude_mode = amplitude_mode;
    return image_call(a, {MON_FIELD_LDS_BINS, 20, 0, {re, im}, {skipped}}, [&](const ImagePass& p) {
        fld.re = re + p.first_bin, fld.im = im + p.first_bin;
        launch_count(a, p, p.img, fld, MonBeam{});
    });
}

int ot_monitor_beam_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges, int32_t nby,
                         int32_t nbz, const ot_segment_source* src, const void* intensity, const void* q_re, const void* q_im,
                         const void* n_index, const double* wavelength, int64_t n_wavelengths, double wavelength_uniform, int64_t n,
                         const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* power, int64_t* skipped, int32_t accumulate) {
    if (!power || !skipped) return fail(OT_ERR_INVALID, "NULL argument");
    const ImageCall a{c, mons, n_monitors, axes, edges, nby, nbz, src, intensity, n, seg_count, n_rays, counts, accumulate};
    if (const int rc = check_image_call(a)) return rc;
    if (!q_re || !q_im || !n_index) return fail(OT_ERR_INVALID, "NULL q_re, q_im or n_index");
    if (const int rc = check_wavelength_args(wavelength, n_wavelengths, wavelength_uniform)) return rc;
    MonBeam beam{};
    beam.q_re = (const uint8_t*)q_re, beam.q_im = (const uint8_t*)q_im, beam.n_index = (const uint8_t*)n_index;
    beam.lam = {wavelength, (unsigned long long*)skipped, wavelength_uniform, (int32_t)n_wavelengths};
    return image_call(a, {MON_BEAM_LDS_BINS, 12, sizeof(double) * MON_WAVES * MON_BEAM_STRIP, {power}, {skipped}}, [&](const ImagePass& p) {
        beam.power = power + p.first_bin;
        launch_count(a, p, p.img, MonField{}, beam);
    });
}

int ot_monitor_wave_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges, int32_t nby,
                         int32_t nbz, const ot_segment_source* src, const void* intensity, const void* n_index, const void* pathlength,
                         const void* q_re, const void* q_im, const double* wavelength, int64_t n_wavelengths, double wavelength_uniform,
                         int32_t amplitude_mode, int32_t gouy, int64_t n, const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* re,
                         double* im, int64_t* skipped, int64_t* aliased, int32_t accumulate) {
    if (!re || !im || !skipped || !aliased) return fail(OT_ERR_INVALID, "NULL argument");
    const ImageCall a{c, mons, n_monitors, axes, edges, nby, nbz, src, intensity, n, seg_count, n_rays, counts, accumulate};
    if (const int rc = check_image_call(a)) return rc;
    if (src->width != 8) return fail(OT_ERR_INVALID, "a beam field needs double-precision segments: width must be 8");
    if (!n_index || !pathlength || !q_re || !q_im) return fail(OT_ERR_INVALID, "NULL n_index, pathlength, q_re or q_im");
    if (const int rc = check_wavelength_args(wavelength, n_wavelengths, wavelength_uniform)) return rc;
    if (const int rc = check_amplitude_mode(amplitude_mode)) return rc;
    if (gouy != 0 && gouy != 1) return fail(OT_ERR_INVALID, "gouy must be 0 or 1");
    MonWave wav{};
    wav.q_re = (const uint8_t*)q_re, wav.q_im = (const uint8_t*)q_im;
    wav.n_index = (const uint8_t*)n_index, wav.pathlength = (const uint8_t*)pathlength;
    wav.lam = {wavelength, (unsigned long long*)skipped, wavelength_uniform, (int32_t)n_wavelengths}, wav.aliased = (unsigned long long*)aliased;
    wav.amplitude_mode = amplitude_mode, wav.gouy = gouy;
    return image_call(a, {MON_WAVE_LDS_BINS, 20, sizeof(double) * MON_WAVES * MON_WAVE_STRIP, {re, im}, {skipped, aliased}}, [&](const ImagePass& p) {
        wav.re = re + p.first_bin, wav.im = im + p.first_bin;  // a kernel of its own, on the same partition
        hipLaunchKernelGGL(k_mon_wave, dim3((unsigned)p.sp.grid), dim3(MON_THREADS), p.lds_bytes, c->stream, p.table, p.nm, p.ms, n, p.sp.iters, seg_count,
                           n_rays, p.img, wav);
    });
}

// Diffraction PSF: the hit list of ot_monitor_record_many into scratch of the context's own, then k_mon_psf (misc_kernels.h) over
// (monitor, pixel tile, hit chunk).  The hit list is sized exactly: record_passes runs once with no room (its emit pass then writes
// first[] and nothing else), the n_monitors + 1 offsets come back to the host — the call's one synchronisation — and it runs
// again into a list of that size.  The offsets also give every monitor's chunk count (mon_psf_chunks), the same number the kernel
// forms on the device.  A launch takes max(1, MON_PSF_PARTIAL_ROWS / (most chunks of a monitor)) (monitor, tile) pairs, so its
// partials stay within MON_PSF_PARTIAL_ROWS rows of MON_PSF_ROW doubles; the launches of a call follow one another on the stream
// and share partials and tickets.  optable_amd/engine.py psf_plan says the same.
// With groups (ot_monitor_psf_groups_many; `grp` not NULL) the hit list is then split by group — k_mon_psf's count pass over the
// partition tiles the host cuts from first[], an exclusive_scan, its scatter pass into a second list — and the sum runs over CELLS
// (m, g) as if they were monitors: monitor, axes, reference and grid of m replicated per group, first_cell in place of first[],
// the outputs indexed by cell.  first_cell comes back to the host (the second synchronisation) for the cells' chunk counts.
// optable_amd/engine.py psf_groups_plan says the same.
struct PsfGroups { const int32_t* ids; int64_t n_ids; int32_t n; int64_t* ungrouped; };
static int psf_call(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind, const double* reference,
                    const double* grid, int32_t ny, int32_t nz, const PsfGroups* grp, const ot_segment_source* src, const void* intensity,
                    const void* n_index, const void* pathlength, const double* wavelength, int64_t n_wavelengths, double wavelength_uniform,
                    int32_t amplitude_mode, int64_t n, const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* norm, double* re, double* im,
                    int32_t accumulate) {
    static_assert(MON_PSF_MAX_SAMPLES == OT_PSF_MAX_SAMPLES && MON_PSF_PARTIAL_ROWS * (int64_t)MON_PSF_ROW * 8 == OT_PSF_SCRATCH_BYTES, "the header's constants");
    static_assert(MON_PSF_GROUPS_MAX == OT_SPOT_GROUPS_MAX, "the partition's LDS holds a counter per group and wave");
    if (!c || !mons || !axes || !reference || !grid || !src || !n_index || !pathlength || !counts || !norm || !re || !im)
        return fail(OT_ERR_INVALID, "NULL argument");
    if (n_monitors < 1 || n_monitors > 1 << 20) return fail(OT_ERR_INVALID, "n_monitors must be 1 .. 2^20");
    if (reference_kind != 0 && reference_kind != 1) return fail(OT_ERR_INVALID, "reference_kind must be 0 (focus) or 1 (direction)");
    if (ny < 1 || ny > MON_PSF_MAX_SAMPLES || nz < 1 || nz > MON_PSF_MAX_SAMPLES) return fail(OT_ERR_INVALID, "ny and nz must be 1 .. 512");
    if (amplitude_mode < 0 || amplitude_mode > 2) return fail(OT_ERR_INVALID, "amplitude_mode must be 0 (sqrt), 1 (linear) or 2 (unit)");
    if (amplitude_mode != 2 && !intensity) return fail(OT_ERR_INVALID, "NULL intensity");
    const ReduceCall a{c, mons, n_monitors, axes, src, intensity, n, seg_count, n_rays, counts, norm, accumulate};
    if (const int rc = check_reduce_call(a)) return rc;
    if (src->width != 8) return fail(OT_ERR_INVALID, "a PSF needs double-precision segments: width must be 8");
    if (const int rc = check_wavelength_args(wavelength, n_wavelengths, wavelength_uniform)) return rc;
    for (int64_t m = 0; m < n_monitors; ++m) {
        const double *r = reference + 3 * m, *g = grid + 4 * m;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2])) return fail(OT_ERR_INVALID, "reference must be finite");
        if (reference_kind == 1 && r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0) return fail(OT_ERR_INVALID, "the direction of a plane wave must not be zero");
        if (!std::isfinite(g[0]) || !std::isfinite(g[1]) || !std::isfinite(g[2]) || !std::isfinite(g[3])) return fail(OT_ERR_INVALID, "grid must be finite");
        if (!(g[1] > 0.0) || !(g[3] > 0.0)) return fail(OT_ERR_INVALID, "the steps of a grid must be positive");
    }
    const int32_t G = grp ? grp->n : 1;
    if (grp) {
        if (!grp->ids || !grp->ungrouped) return fail(OT_ERR_INVALID, "NULL argument");
        if (G < 1 || G > OT_SPOT_GROUPS_MAX) return fail(OT_ERR_INVALID, "n_groups must be 1 .. 256");
        if (grp->n_ids < 1 || grp->n_ids >= (int64_t)1 << 31) return fail(OT_ERR_INVALID, "n_group_ids must be at least 1 (and below 2^31)");
        if ((int64_t)n_monitors * G > OT_PSF_GROUP_CELLS_MAX) return fail(OT_ERR_INVALID, "n_monitors * n_groups exceeds 4096 cells");
        if ((int64_t)n_monitors * G * ny * nz > (int64_t)1 << 27) return fail(OT_ERR_INVALID, "n_monitors * n_groups * ny * nz exceeds 2^27 samples");
    }
    const int32_t n_cells = n_monitors * G;  // (a cell is a monitor where there are no groups)
    HIP_TRY(hipSetDevice(c->device));
    const size_t pixels = (size_t)n_cells * ny * nz;
    if (!accumulate) {
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)n_cells, c->stream));
        HIP_TRY(hipMemsetAsync(norm, 0, sizeof(double) * (size_t)n_cells, c->stream));
        HIP_TRY(hipMemsetAsync(re, 0, sizeof(double) * pixels, c->stream));
        HIP_TRY(hipMemsetAsync(im, 0, sizeof(double) * pixels, c->stream));
        if (grp) HIP_TRY(hipMemsetAsync(grp->ungrouped, 0, sizeof(int64_t) * (size_t)n_monitors, c->stream));
    }
    if (n == 0) return 0;
    ot_monitor* table;
    int64_t *first, *n_total, *first_cell;
    double *d_axes, *d_reference, *d_grid;
    unsigned int* tickets;
    MonPsfPartition* d_pp;
    const auto carve = [&](void* base) {
        Carve cv{(uint8_t*)base};
        table = cv.take<ot_monitor>(n_cells), first = cv.take<int64_t>((size_t)n_monitors + 1), n_total = cv.take<int64_t>(1);
        d_axes = cv.take<double>(6 * (size_t)n_cells), d_reference = cv.take<double>(3 * (size_t)n_cells), d_grid = cv.take<double>(4 * (size_t)n_cells);
        tickets = cv.take<unsigned int>(MON_PSF_PARTIAL_ROWS);
        first_cell = cv.take<int64_t>((size_t)n_cells + 1, grp != nullptr), d_pp = cv.take<MonPsfPartition>(1, grp != nullptr);
        return cv.used;
    };
    if (c->psf.ensure(carve(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of PSF scratch failed");
    carve(c->psf.p);
    const MonSource ms = mon_source(src);
    if (const int rc = record_passes(c, mons, n_monitors, ms, n, seg_count, n_rays, 0, first, nullptr, nullptr, nullptr, nullptr, nullptr, n_total)) return rc;
    std::vector<int64_t> host_first((size_t)n_monitors + 1);
    HIP_TRY(hipMemcpyAsync(host_first.data(), first, sizeof(int64_t) * host_first.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t total = host_first[n_monitors];
    if (total == 0) return 0;
    int32_t max_chunks = 1;  // (of a monitor: no cell of it has more)
    for (int32_t m = 0; m < n_monitors; ++m) max_chunks = std::max(max_chunks, mon_psf_chunks(host_first[m + 1] - host_first[m]));
    const int64_t n_pairs = (int64_t)n_cells * mon_psf_parts(ny) * mon_psf_parts(nz);
    int64_t pairs_a_launch = std::min<int64_t>(n_pairs, std::max(1, MON_PSF_PARTIAL_ROWS / max_chunks));
    // the partition tiles: MON_PSF_PART_TILE consecutive hits of one monitor each, one empty tile for a monitor without a hit
    std::vector<MonPsfTile> tiles;
    for (int32_t m = 0; grp && m < n_monitors; ++m) {
        const int64_t h0 = host_first[m], h1 = host_first[m + 1], base = (int64_t)G * (int64_t)tiles.size();
        const int32_t nt = (int32_t)std::max<int64_t>(1, (h1 - h0 + MON_PSF_PART_TILE - 1) / MON_PSF_PART_TILE);
        for (int32_t k = 0; k < nt; ++k)
            tiles.push_back({h0 + (int64_t)k * MON_PSF_PART_TILE, std::min(h1, h0 + (int64_t)(k + 1) * MON_PSF_PART_TILE), base, m, k, nt, 0});
    }
    const int64_t n_count = (int64_t)G * (int64_t)tiles.size();
    int64_t *hit_index, *to_hit_index, *tile_off;
    double *Px, *Py, *Pz, *tt, *to_Px, *to_Py, *to_Pz, *to_t, *partials;
    MonPsfTile* part;
    int32_t* tile_count;
    // the partials: a launch's rows; with groups the cells' chunk counts are not known yet, and no plan of theirs takes more rows
    // than the monitors' most chunks allow
    const size_t rows = grp ? (size_t)std::min<int64_t>(n_pairs * max_chunks, MON_PSF_PARTIAL_ROWS) : (size_t)pairs_a_launch * max_chunks;
    const auto carve_hits = [&](void* base) {
        Carve cv{(uint8_t*)base};
        hit_index = cv.take<int64_t>(total), Px = cv.take<double>(total), Py = cv.take<double>(total), Pz = cv.take<double>(total), tt = cv.take<double>(total);
        partials = cv.take<double>(rows * MON_PSF_ROW);
        const bool g = grp != nullptr;
        to_hit_index = cv.take<int64_t>(total, g), to_Px = cv.take<double>(total, g), to_Py = cv.take<double>(total, g), to_Pz = cv.take<double>(total, g);
        to_t = cv.take<double>(total, g);
        part = cv.take<MonPsfTile>(tiles.size(), g), tile_count = cv.take<int32_t>(n_count + 1, g), tile_off = cv.take<int64_t>(n_count + 1, g);
        return cv.used;
    };
    if (c->psf_hits.ensure(carve_hits(nullptr))) return fail(OT_ERR_HIP, "hipMalloc of the PSF hit list failed");
    carve_hits(c->psf_hits.p);
    if (grp && c->scan_tmp.ensure(scan_tmp_bytes<int64_t>(n_count + 1) + 256)) return fail(OT_ERR_HIP, "hipMalloc of scan scratch failed");
    if (const int rc = record_passes(c, mons, n_monitors, ms, n, seg_count, n_rays, total, first, hit_index, Px, Py, Pz, tt, n_total)) return rc;
    // the tables of the sum, a row per cell: those of monitor m for each of its groups
    std::vector<ot_monitor> cell_mons;
    std::vector<double> cell_tables;
    if (grp) {
        cell_mons.resize(n_cells), cell_tables.resize(13 * (size_t)n_cells);
        double *ca = cell_tables.data(), *cr = ca + 6 * (size_t)n_cells, *cg = cr + 3 * (size_t)n_cells;
        for (int32_t k = 0; k < n_cells; ++k) {
            const int32_t m = k / G;
            cell_mons[k] = mons[m];
            std::copy(axes + 6 * (size_t)m, axes + 6 * (size_t)m + 6, ca + 6 * (size_t)k);
            std::copy(reference + 3 * (size_t)m, reference + 3 * (size_t)m + 3, cr + 3 * (size_t)k);
            std::copy(grid + 4 * (size_t)m, grid + 4 * (size_t)m + 4, cg + 4 * (size_t)k);
        }
        mons = cell_mons.data(), axes = ca, reference = cr, grid = cg;
    }
    HIP_TRY(hipMemcpyAsync(table, mons, sizeof(ot_monitor) * (size_t)n_cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_axes, axes, sizeof(double) * 6 * (size_t)n_cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_reference, reference, sizeof(double) * 3 * (size_t)n_cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_grid, grid, sizeof(double) * 4 * (size_t)n_cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(tickets, 0, sizeof(unsigned int) * MON_PSF_PARTIAL_ROWS, c->stream));
    MonPsf ps{};
    ps.first = first, ps.hit_index = hit_index, ps.Px = Px, ps.Py = Py, ps.Pz = Pz, ps.t = tt;
    ps.axes = d_axes, ps.reference = d_reference, ps.grid = d_grid;
    ps.intensity = (const uint8_t*)intensity, ps.n_index = (const uint8_t*)n_index, ps.pathlength = (const uint8_t*)pathlength;
    ps.lam = {wavelength, nullptr, wavelength_uniform, (int32_t)n_wavelengths};
    ps.partials = partials, ps.ticket = tickets;
    ps.re = re, ps.im = im, ps.norm = norm, ps.counts = (long long*)counts;
    ps.kind = reference_kind, ps.amplitude_mode = amplitude_mode, ps.ny = ny, ps.nz = nz, ps.max_chunks = max_chunks;
    if (grp) {
        HIP_TRY(hipMemcpyAsync(part, tiles.data(), sizeof(MonPsfTile) * tiles.size(), hipMemcpyHostToDevice, c->stream));
        const MonPsfPartition pp{G, (int32_t)grp->n_ids, n_cells, 0, grp->ids, part, tile_count, tile_off, n_count, first_cell, to_hit_index,
                                 to_Px, to_Py, to_Pz, to_t, (unsigned long long*)grp->ungrouped};
        HIP_TRY(hipMemcpyAsync(d_pp, &pp, sizeof(pp), hipMemcpyHostToDevice, c->stream));
        ps.pp = d_pp;
        ps.mode = 1;
        hipLaunchKernelGGL(k_mon_psf, dim3((unsigned)tiles.size()), dim3(MON_THREADS), 0, c->stream, table, ms, ps);
        exclusive_scan<int32_t, int64_t>(c->scan_tmp.p, tile_count, tile_off, n_count + 1, c->stream);
        ps.mode = 2;
        hipLaunchKernelGGL(k_mon_psf, dim3((unsigned)tiles.size()), dim3(MON_THREADS), 0, c->stream, table, ms, ps);
        HIP_TRY(hipGetLastError());
        std::vector<int64_t> host_cell((size_t)n_cells + 1);
        HIP_TRY(hipMemcpyAsync(host_cell.data(), first_cell, sizeof(int64_t) * host_cell.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (host_cell[n_cells] == 0) return 0;
        max_chunks = 1;
        for (int32_t k = 0; k < n_cells; ++k) max_chunks = std::max(max_chunks, mon_psf_chunks(host_cell[k + 1] - host_cell[k]));
        pairs_a_launch = std::min<int64_t>(n_pairs, std::max(1, MON_PSF_PARTIAL_ROWS / max_chunks));
        ps.mode = 0, ps.max_chunks = max_chunks;
        ps.first = first_cell, ps.hit_index = to_hit_index, ps.Px = to_Px, ps.Py = to_Py, ps.Pz = to_Pz, ps.t = to_t;
    }
    for (int64_t pair0 = 0; pair0 < n_pairs; pair0 += pairs_a_launch) {
        ps.pair0 = (int32_t)pair0;
        const int64_t pairs = std::min(pairs_a_launch, n_pairs - pair0);
        hipLaunchKernelGGL(k_mon_psf, dim3((unsigned)(pairs * max_chunks)), dim3(MON_THREADS), 0, c->stream, table, ms, ps);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ot_monitor_psf_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind, const double* reference,
                        const double* grid, int32_t ny, int32_t nz, const ot_segment_source* src, const void* intensity, const void* n_index,
                        const void* pathlength, const double* wavelength, int64_t n_wavelengths, double wavelength_uniform, int32_t amplitude_mode,
                        int64_t n, const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* norm, double* re, double* im,
                        int32_t accumulate) {
    return psf_call(c, mons, n_monitors, axes, reference_kind, reference, grid, ny, nz, nullptr, src, intensity, n_index, pathlength, wavelength,
                    n_wavelengths, wavelength_uniform, amplitude_mode, n, seg_count, n_rays, counts, norm, re, im, accumulate);
}

int ot_monitor_psf_groups_many(ot_ctx* c, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                               const double* reference, const double* grid, int32_t ny, int32_t nz, const int32_t* groups, int64_t n_group_ids,
                               int32_t n_groups, const ot_segment_source* src, const void* intensity, const void* n_index, const void* pathlength,
                               const double* wavelength, int64_t n_wavelengths, double wavelength_uniform, int32_t amplitude_mode, int64_t n,
                               const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* norm, double* re, double* im, int64_t* ungrouped,
                               int32_t accumulate) {
    const PsfGroups grp{groups, n_group_ids, n_groups, ungrouped};
    return psf_call(c, mons, n_monitors, axes, reference_kind, reference, grid, ny, nz, &grp, src, intensity, n_index, pathlength, wavelength,
                    n_wavelengths, wavelength_uniform, amplitude_mode, n, seg_count, n_rays, counts, norm, re, im, accumulate);
}

int ot_debug_last_launch(ot_ctx* c, int32_t info[8]) {
    if (!c || !info) return fail(OT_ERR_INVALID, "NULL argument");
    for (int q = 0; q < 8; ++q) info[q] = c->last_launch[q];
    return 0;
}

int ot_debug_generation_mismatches(ot_ctx* c, int64_t* out) {
    if (!c || !out) return fail(OT_ERR_INVALID, "NULL argument");
    *out = 0;
    if (!c->gen_mismatch) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, c->gen_mismatch, sizeof(v), hipMemcpyDeviceToHost));
    *out = (int64_t)v;
    return 0;
}

}  // extern "C"

// Which of the two [k][ray] slot layouts do THIS device's memory channels like better?  The lane-per-ray kernel is bound by
// its streams, and the stream rate of the two layouts differs by box: on some the 64-slot tiles run 12 % faster than the 14
// arrays, on others 8 % slower (same code, same clocks; stable within a box to half a percent: tools/stream_layouts2.hip).
// So it is measured, once per context and precision: cfg 2's shape (2^20 rays, 5 segments) through k_stream_ceiling in
// both layouts, interleaved, on buffers of the library's own that are freed again (1.3 GB in double precision, ~15 ms).
template <class T> static int probe_layouts(ot_ctx* c) {
    constexpr int64_t n = 1 << 20;
    constexpr int32_t K = 5;
    const int pi = sizeof(T) == 8 ? 1 : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t in_bytes = (size_t)n * (12 * sizeof(T) + 8), slots_bytes = (size_t)n * K * (12 * sizeof(T) + 8);
    const size_t tiles_bytes = (size_t)(n * K / SegTiles<T>::LANES) * SegTiles<T>::TILE_BYTES;  // (the tile's geometry: kernels.h SegTiles, the one definition)
    uint8_t* buf = nullptr;
    if (hipMalloc((void**)&buf, in_bytes + slots_bytes + tiles_bytes + 4 * n + 4096) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OT_ERR_HIP, "ot_probe_layouts: no room for the probe buffers");
    }
    HIP_TRY(hipMemsetAsync(buf, 0, in_bytes, c->stream));
    ot_rays in;
    void** inf[12] = {&in.ox, &in.oy, &in.oz, &in.dx, &in.dy, &in.dz, &in.wavelength, &in.q_re, &in.q_im, &in.intensity, &in.n, &in.pathlength};
    uint8_t* p = buf;
    for (int f = 0; f < 12; ++f) { *inf[f] = p; p += n * sizeof(T); }
    in.id = (int32_t*)p; p += 4 * n;
    in.flags = (int32_t*)p; p += 4 * n;
    in.length = nullptr;
    ot_segments sg;
    void** of[12] = {&sg.ox, &sg.oy, &sg.oz, &sg.dx, &sg.dy, &sg.dz, &sg.length, &sg.intensity, &sg.q_re, &sg.q_im, &sg.n, &sg.pathlength};
    for (int f = 0; f < 12; ++f) { *of[f] = p; p += n * K * sizeof(T); }
    sg.ray = (int32_t*)p; p += 4 * n * K;
    sg.surface = (int32_t*)p; p += 4 * n * K;
    p = (uint8_t*)(((uintptr_t)p + 4095) & ~(uintptr_t)4095);
    uint8_t* tiles = p; p += tiles_bytes;
    int32_t* seg_count = (int32_t*)p;
    const int block = 256, grid = (int)((n + block - 1) / block);
    const int32_t pair = (c->opt_pair && sizeof(T) == 8) ? 1 : 0;  // the slot arrays' stores, as the trace pairs them; tiles: one element per lane, as the trace
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    double best[2] = {1e30, 1e30};
    auto launch = [&](int layout) {
        if (layout == 0) hipLaunchKernelGGL((k_stream_ceiling<T, true, SegsT<T>>), dim3(grid), dim3(block), 0, c->stream, view<T>(&in), n, K, view<T>(&sg), seg_count, pair, 0u);
        else hipLaunchKernelGGL((k_stream_ceiling<T, true, SegTiles<T>>), dim3(grid), dim3(block), 0, c->stream, view<T>(&in), n, K, SegTiles<T>{tiles}, seg_count, 0, 0u);
    };
    int rc = 0;
    for (int round = 0; round < 3 && !rc; ++round)
        for (int layout = 0; layout < 2 && !rc; ++layout) {
            for (int w = 0; w < (round == 0 ? 30 : 5); ++w) launch(layout);  // clocks up, code object loaded
            if (hipEventRecord(e0, c->stream) != hipSuccess) { rc = 1; break; }
            for (int w = 0; w < 10; ++w) launch(layout);
            float ms = 0.f;
            if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { rc = 1; break; }
            const double us = ms * 1e3 / 10;
            if (us < best[layout]) best[layout] = us;
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(buf);
    if (rc || hipGetLastError() != hipSuccess) return fail(OT_ERR_HIP, "ot_probe_layouts: a probe launch failed");
    c->probe_us[pi][0] = best[0];
    c->probe_us[pi][1] = best[1];
    return 0;
}

extern "C" int ot_probe_layouts(ot_ctx* c, int32_t real_bytes, double* us_slots, double* us_tiled) {
    if (!c || (real_bytes != 4 && real_bytes != 8)) return fail(OT_ERR_INVALID, "ot_probe_layouts: ctx / real_bytes (4 or 8)");
    const int pi = real_bytes == 8 ? 1 : 0;
    if (c->probe_us[pi][0] == 0) {
        const int rc = real_bytes == 8 ? probe_layouts<double>(c) : probe_layouts<float>(c);
        if (rc) return rc;
    }
    if (us_slots) *us_slots = c->probe_us[pi][0];
    if (us_tiled) *us_tiled = c->probe_us[pi][1];
    return 0;
}

// What would the library launch for this scene and batch, and which output layout do its kernels write fastest?
extern "C" int ot_trace_plan(ot_ctx* c, int32_t real_bytes, int64_t n, int32_t K, int32_t info[8]) {
    if (!c || !info || (real_bytes != 4 && real_bytes != 8) || n < 0 || K < 1) return fail(OT_ERR_INVALID, "ot_trace_plan: bad argument");
    if (!c->has_scene) return fail(OT_ERR_NOSCENE, "ot_scene_upload has not been called");
    const bool f64 = real_bytes == 8;
    const bool heavy = f64 ? wants_rolling<double>(c, K) : wants_rolling<float>(c, K);
    const int64_t limit = ((int64_t)1 << 30) / (f64 ? 2 : 1);  // append capacity: the byte offset of a slot inside a plane stays below 2^32
    for (int q = 0; q < 8; ++q) info[q] = 0;
    info[0] = heavy ? 2 : 1;
    info[1] = heavy ? 0 : 1;                      // ot_trace_tiled_* takes the scene
    info[2] = f64 ? 29 : 30;                      // log2 of the first append capacity that is refused
    int layout = 0;
    if (heavy) {
        // the dense list — unless even a tight block could not hold the worst case of this batch (the caller then falls back
        // to the slots, which have no such limit, or splits the batch)
        layout = (n * (int64_t)K + ((int64_t)1 << 23) < limit) ? 2 : 0;
    } else {
        const int pi = f64 ? 1 : 0;
        if (c->probe_us[pi][0] == 0) {
            const int rc = f64 ? probe_layouts<double>(c) : probe_layouts<float>(c);
            if (rc) return rc;
        }
        layout = c->probe_us[pi][1] < 0.985 * c->probe_us[pi][0] ? 1 : 0;  // tiles only where they win by more than the probe's noise
        info[5] = (int32_t)(c->probe_us[pi][0] * 100);  // hundredths of a microsecond per probe launch: slot arrays, tiles
        info[6] = (int32_t)(c->probe_us[pi][1] * 100);
    }
    info[3] = layout;  // 0 slot arrays (ot_trace_*), 1 tiles (ot_trace_tiled_*), 2 append (ot_trace_append_*)
    return 0;
}

extern "C" {

int ot_set_option(ot_ctx* c, int32_t option, int32_t value) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    switch (option) {
        case OT_OPT_NT_STORES: c->opt_nt = value != 0; return 0;
        case OT_OPT_PAIR_STORES: c->opt_pair = value != 0; return 0;
        case OT_OPT_MIX_GENERATIONS: c->opt_mix = value < 0 ? -1 : (value != 0); return 0;
        case OT_OPT_FLAT_QUEUE:
            if (value < 0 || (value > 1 && (value < 192 || value > 8192 || value % 64))) return fail(OT_ERR_INVALID, "OT_OPT_FLAT_QUEUE takes 0, 1, or the pairs a round may hold: a multiple of 64, 192..8192");
            c->opt_flat = value; return 0;
        case OT_OPT_MIN_WAVES: 
            if (value != 0 && value != 4) return fail(OT_ERR_INVALID, "OT_OPT_MIN_WAVES takes 0 or 4");
            c->opt_minw = value; return 0;
        case OT_OPT_KERNEL:
            if (value < 0 || value > 2) return fail(OT_ERR_INVALID, "OT_OPT_KERNEL takes 0 (auto), 1 (lane per ray) or 2 (rolling lists)");
            c->opt_kernel = value; return 0;
        case OT_OPT_LDS_LIMIT_KB:
            if (value < 0 || value > 150) return fail(OT_ERR_INVALID, "OT_OPT_LDS_LIMIT_KB takes 0..150");
            c->opt_lds_limit_kb = value; return 0;
        case OT_OPT_LIST_CAP:  // generation-pure lists never wrap: any multiple of 64; mixed lists are rings: powers of two only
            if (value < 128 || value > 1024 || value % 64) return fail(OT_ERR_INVALID, "OT_OPT_LIST_CAP takes a multiple of 64, 128..1024");
            if (!(value & (value - 1))) c->opt_list_cap = value;
            c->opt_list_cap_pure = value; return 0;
        case OT_OPT_LDS_RECORDS:
            if (value < -1 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_LDS_RECORDS takes -1 (auto), 0 or 1");
            c->opt_rec_lds = value; return 0;
        case OT_OPT_APPEND_CHUNK:
            if (value < 64 || value > (1 << 20) || value % 64) return fail(OT_ERR_INVALID, "OT_OPT_APPEND_CHUNK takes a multiple of 64, 64..1048576");
            c->opt_append_chunk = value; return 0;
        case OT_OPT_GEN_REUSE:
            if (value < -1 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_GEN_REUSE takes -1 (auto), 0 or 1");
            c->opt_gen_reuse = value; return 0;
        case OT_OPT_GEN_DROP_DOOMED: c->opt_gen_drop = value != 0; return 0;
        case OT_OPT_BLOCK_POOL:
            if (value < -1 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_BLOCK_POOL takes -1 (auto), 0 or 1");
            c->opt_pool = value; return 0;
        case OT_OPT_INSTANCING: c->opt_instancing = value != 0; return 0;  // takes effect at the next ot_scene_upload
        case OT_OPT_GEN_AHEAD: c->opt_gen_ahead = value != 0; return 0;
        case OT_OPT_TREES_FLAT: c->opt_trees_flat = value != 0; return 0;
        case OT_OPT_GEN_PARENT_INDEX: c->opt_gen_parent = value != 0; return 0;
        case OT_OPT_TREES_GLOBAL_IMAGE: c->opt_trees_global = value < 0 ? 0 : (value > 2 ? 2 : value); return 0;  // 1: records in LDS when they fit; 2: everything from global memory
        case OT_OPT_TREES_REFILL_AT:
            if (value < 1 || value > 64) return fail(OT_ERR_INVALID, "OT_OPT_TREES_REFILL_AT takes 1..64");
            c->opt_trees_refill_at = value; return 0;
        case OT_OPT_TREES_LDS_ENTRIES:
            if (value < 0 || value > 64) return fail(OT_ERR_INVALID, "OT_OPT_TREES_LDS_ENTRIES takes 0 (by the cap) or 1..64");
            c->opt_trees_lds = value; return 0;
        case OT_OPT_GEN_ONEPASS:
            if (value < -1 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_GEN_ONEPASS takes -1 (small generations), 0 or 1");
            c->opt_gen_onepass = value; return 0;
        case OT_OPT_POOL_JITTER:
            if (value < 0 || value > (1 << 20)) return fail(OT_ERR_INVALID, "OT_OPT_POOL_JITTER takes 0 (off) or a period up to 2^20");
            c->opt_pool_jitter = value; return 0;
        case OT_OPT_REFILL:
            if (value < 0 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_REFILL takes 0 or 1");
            c->opt_refill = value; return 0;
        case OT_OPT_REFILL_TICKET:
            if (value < 0 || value > 4096 || value % 64) return fail(OT_ERR_INVALID, "OT_OPT_REFILL_TICKET takes 0 (by batch size) or a multiple of 64 up to 4096");
            c->opt_refill_ticket = value; return 0;
        case OT_OPT_UNIFORM:
            if (value < 0 || value > 1) return fail(OT_ERR_INVALID, "OT_OPT_UNIFORM takes 0 or 1");
            c->opt_uniform = value; return 0;
        case OT_OPT_RESIDENT:
            if (value < 0 || value > 2) return fail(OT_ERR_INVALID, "OT_OPT_RESIDENT takes 0, 1 or 2");
            c->opt_resident = value; return 0;
        case OT_OPT_BLOCKS_PER_CU:
            if (value < 0 || value > 65536) return fail(OT_ERR_INVALID, "OT_OPT_BLOCKS_PER_CU out of range");
            c->opt_blocks_per_cu = value; return 0;
        default: return fail(OT_ERR_INVALID, "unknown option");
    }
}

}  // extern "C"

template <class T, class OUT>
static int bench_stream(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const OUT& out, int32_t pair, int32_t* seg_count, uint32_t uniform) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    int rc = check_rays(rays, "rays");
    if (rc) return rc;
    rc = check_uniform(uniform);
    if (rc) return rc;
    if (!c->opt_uniform) uniform = 0;
    if (n < 1 || K < 1 || !seg_count || n >= (int64_t)1 << 31) return fail(OT_ERR_INVALID, "bad n / K / seg_count");
    HIP_TRY(hipSetDevice(c->device));
    const int block = 256;
    const int64_t need = (n + block - 1) / block, cap = (int64_t)c->n_cus * (c->opt_blocks_per_cu > 0 ? c->opt_blocks_per_cu : 256);  // the fused kernel's grid rule
    const int grid = (int)(need < cap ? need : cap);
    rc = timing_begin(c);
    if (rc) return rc;
    if (c->opt_nt)
        hipLaunchKernelGGL((k_stream_ceiling<T, true, OUT>), dim3(grid), dim3(block), 0, c->stream, view<T>(rays), n, K, out, seg_count, pair, uniform);
    else
        hipLaunchKernelGGL((k_stream_ceiling<T, false, OUT>), dim3(grid), dim3(block), 0, c->stream, view<T>(rays), n, K, out, seg_count, pair, uniform);
    HIP_TRY(hipGetLastError());
    return timing_end(c);
}

extern "C" {

int ot_bench_stream_uniform_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count, uint32_t uniform) {
    const int rc = check_segs(out);
    return rc ? rc : bench_stream<double, SegsT<double>>(c, rays, n, K, view<double>(out), pair_ok<double>(c, out, n), seg_count, uniform);
}
int ot_bench_stream_uniform_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count, uint32_t uniform) {
    const int rc = check_segs(out);
    return rc ? rc : bench_stream<float, SegsT<float>>(c, rays, n, K, view<float>(out), pair_ok<float>(c, out, n), seg_count, uniform);
}
int ot_bench_stream_tiled_uniform_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count, uint32_t uniform) {
    const int rc = check_tiles<double>(tiles, capacity, n, K);
    return rc ? rc : bench_stream<double, SegTiles<double>>(c, rays, n, K, SegTiles<double>{(uint8_t*)tiles}, 0, seg_count, uniform);
}
int ot_bench_stream_tiled_uniform_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count, uint32_t uniform) {
    const int rc = check_tiles<float>(tiles, capacity, n, K);
    return rc ? rc : bench_stream<float, SegTiles<float>>(c, rays, n, K, SegTiles<float>{(uint8_t*)tiles}, 0, seg_count, uniform);
}
int ot_bench_stream_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count) {
    return ot_bench_stream_uniform_f64(c, rays, n, K, out, seg_count, 0u);
}
int ot_bench_stream_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, const ot_segments* out, int32_t* seg_count) {
    return ot_bench_stream_uniform_f32(c, rays, n, K, out, seg_count, 0u);
}
int ot_bench_stream_tiled_f64(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count) {
    return ot_bench_stream_tiled_uniform_f64(c, rays, n, K, tiles, capacity, seg_count, 0u);
}
int ot_bench_stream_tiled_f32(ot_ctx* c, const ot_rays* rays, int64_t n, int32_t K, void* tiles, int64_t capacity, int32_t* seg_count) {
    return ot_bench_stream_tiled_uniform_f32(c, rays, n, K, tiles, capacity, seg_count, 0u);
}

#ifdef OT_STAMP
// diagnostic builds only (make STAMP=1): wave-cycles the last k_trace_rolling launch spent per phase
int ot_debug_stamps(ot_ctx* c, unsigned long long* out5) {
    if (!c || !c->blocked.p) return fail(OT_ERR_INVALID, "no rolling launch yet");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out5, (uint8_t*)c->blocked.p + c->blocked_queue_off + 8 * sizeof(unsigned long long), 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
#endif
int ot_timing_enable(ot_ctx* c, int enabled) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    if (!enabled) {
        int rc = flush_events(c);
        if (rc) return rc;
    }
    c->timing = enabled != 0;
    return 0;
}
int ot_timing_read(ot_ctx* c, double* total_ms, int64_t* launches) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    int rc = flush_events(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->total_ms;
    if (launches) *launches = c->launches;
    return 0;
}
int ot_timing_reset(ot_ctx* c) {
    if (!c) return fail(OT_ERR_INVALID, "ctx is NULL");
    int rc = flush_events(c);
    if (rc) return rc;
    c->total_ms = 0.0;
    c->launches = 0;
    return 0;
}
}  // extern "C"
