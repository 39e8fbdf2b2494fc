// misc_kernels.h — the small non-template kernels of the library (one translation unit: optable_hip.hip) and the
// device-wide exclusive scan they share.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

// ------------------------------------------------------------------------------------------
// Exclusive prefix sum over n elements in three streaming launches: tile sums -> scan of the tile sums (one
// workgroup) -> tile-local scan + tile offset.  Every scan of the library is small next to the pass it serves (wave
// totals of a generation: n / 64 words; Monitor.record: 4 of the ~110 bytes its test reads per slot), so the second
// read of the input is in the noise, and the library carries three kernels of its own instead of a scan library's
// several hundred tuning variants.
//   In  int32 flags / counts, or packed 2 x 32-bit totals in one 64-bit word (the halves never carry into each other)
//   Out int32 / int64 / uint64
static constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

template <class V> __device__ __forceinline__ V wave_incl_scan(V v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
// exclusive scan of one value per thread over a 256-thread workgroup; `total` = the workgroup's sum (all threads)
template <class V> __device__ __forceinline__ V block_excl_scan(V v, V& total) {
    __shared__ V wsum[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const V incl = wave_incl_scan(v, lane);
    __syncthreads();  // wsum may still be read by the previous call
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    V before = V(0), all = V(0);
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    total = all;
    return before + incl - v;
}
template <class In, class Out>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_tiles(const In* __restrict__ in, int64_t n, Out* __restrict__ tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    Out s = Out(0);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += (Out)in[base + k];
    Out total;
    (void)block_excl_scan(s, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
template <class Out> __global__ __launch_bounds__(SCAN_THREADS) void k_scan_spine(Out* tile_sum, int64_t n_tiles) {
    Out carry = Out(0);
    for (int64_t b = 0; b < n_tiles; b += SCAN_THREADS) {
        const int64_t i = b + threadIdx.x;
        const Out v = i < n_tiles ? tile_sum[i] : Out(0);
        Out total;
        const Out ex = block_excl_scan(v, total);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
}
template <class In, class Out>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(const In* __restrict__ in, int64_t n, const Out* __restrict__ tile_sum,
                                                             Out* __restrict__ out) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    Out v[SCAN_ITEMS];
    Out s = Out(0);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? (Out)in[base + k] : Out(0);
        s += v[k];
    }
    Out total;
    Out run = block_excl_scan(s, total) + tile_sum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}
// bytes of temporary storage an exclusive_scan over n elements needs
template <class Out> static size_t scan_tmp_bytes(int64_t n) { return sizeof(Out) * (size_t)((n + SCAN_TILE - 1) / SCAN_TILE + 1); }
template <class In, class Out> static void exclusive_scan(void* tmp, const In* in, Out* out, int64_t n, hipStream_t stream) {
    if (n <= 0) return;
    const int64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    Out* tile_sum = (Out*)tmp;
    // the spine only adds: every 64-bit Out shares the unsigned instantiation (the same bits in two's complement), one kernel less
    using Spine = std::conditional_t<sizeof(Out) == 8, unsigned long long, Out>;
    hipLaunchKernelGGL((k_scan_tiles<In, Out>), dim3((unsigned)tiles), dim3(SCAN_THREADS), 0, stream, in, n, tile_sum);
    hipLaunchKernelGGL((k_scan_spine<Spine>), dim3(1), dim3(SCAN_THREADS), 0, stream, (Spine*)tile_sum, tiles);
    hipLaunchKernelGGL((k_scan_apply<In, Out>), dim3((unsigned)tiles), dim3(SCAN_THREADS), 0, stream, in, n, (const Out*)tile_sum, out);
}

// ------------------------------------------------------------------------------------------
// totals of a generation from the scanned wave totals: segments written and rays of the next generation.  Runs between
// the two passes: the emit pass takes its first slot from totals[2] (the cursor as it stood), so the caller's cursor
// and next-generation count can be published here and the generation needs no closing kernel.
__global__ void k_gen_totals(const unsigned long long* wave_total, const unsigned long long* wave_prefix, int64_t n_waves, int64_t* totals,
                             int64_t* cursor, int64_t* n_next) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long all = wave_prefix[n_waves - 1] + wave_total[n_waves - 1];
        totals[0] = (int64_t)(all >> 32);
        totals[1] = (int64_t)(all & 0xffffffffull);
        totals[2] = *cursor;
        *cursor += totals[0];
        *n_next = totals[1];
    }
}

// k_gen_recount: the count pass of a generation whose rays were looked ahead by the emit pass that wrote them (k_gen_pass MODE 2):
// rank within the tree, budget cut and doomed children exactly as the count pass decides them, the number of children from the
// byte the emit pass left.  Writes the code byte in place of it and the wave totals.
__global__ __launch_bounds__(256) void k_gen_recount(const int32_t* __restrict__ tree, int64_t n, const int32_t* __restrict__ budget, uint8_t* code,
                                                     unsigned long long* __restrict__ wave_total, int32_t drop_doomed) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gwave = i >> 6;
    int32_t my_tree = -1;
    int start_lane = -1;
    if (i < n) {
        my_tree = tree[i];
        if (lane == 0 || tree[i - 1] != my_tree) start_lane = lane;
    }
    const int head_lane = wave_incl_max_i32(start_lane);
    int64_t head = (i - lane) + head_lane;
    if (i < n && head_lane == 0) head = tree_head(tree, i - lane);
    const int64_t bud = i < n ? (int64_t)budget[my_tree] : 0;
    const bool active = i < n && (i - head) < bud;
    bool doomed = false;
    if (active && drop_doomed) {
        const int64_t last_needed = head + bud - 1;
        doomed = last_needed < n && tree[last_needed] == my_tree;
    }
    int32_t nk = active ? (int32_t)(code[i] & 3) : 0;
    if (doomed) nk = 0;
    if (i < n) code[i] = (uint8_t)((active ? 1 : 0) | (nk << 1) | (doomed ? 8 : 0));
    const int n_act = __popcll(__ballot(active));
    int kids;
    wave_excl_scan_i32(nk, kids);
    if (lane == 0 && (gwave << 6) < n) wave_total[gwave] = ((unsigned long long)n_act << 32) | (unsigned long long)kids;
}

// The two elementwise integer passes of the generation path over tree[], one kernel with a launch-uniform mode:
// GEN_SEED_REM: out[i] = table[tree[i]] — k_gen_one's per-ray budgets rem[], seeded from the per-tree table budget[] before the first
//   generation of a call (kernels.h); n_slots is not read.
// GEN_RANK: out[slot][i] = table[slot][i] - table[slot][head of i's tree] — rank[slot][i] = how many earlier rays of i's tree (this
//   generation) hit limited leaf `slot`, from the exclusive scans ex[] of the probe pass.
enum : int32_t { GEN_SEED_REM = 0, GEN_RANK = 1 };
__global__ void k_gen_per_ray(int32_t mode, const int32_t* __restrict__ tree, int64_t n, int32_t n_slots, const int32_t* __restrict__ table,
                              int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == GEN_SEED_REM) {
        out[i] = table[tree[i]];
        return;
    }
    const int64_t head = tree_head(tree, i);
    for (int s = 0; s < n_slots; ++s) out[(int64_t)s * n + i] = table[(int64_t)s * n + i] - table[(int64_t)s * n + head];
}
// after the trace: each tree's last ray of the generation folds the generation's hits into the table
__global__ void k_gen_counts(const int32_t* tree, const int32_t* ids, int64_t n, int32_t n_slots, const int32_t* rank,
                             const int32_t* probe, const int32_t* slot_max, int32_t* counts, int32_t n_classes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1 || tree[i + 1] != tree[i]) {
        for (int s = 0; s < n_slots; ++s) {
            if ((uint32_t)ids[i] >= (uint32_t)n_classes) break;  // id outside the table: not counted (count_gate's rule)
            int32_t* c = counts + (int64_t)s * n_classes + ids[i];
            const int32_t total = *c + rank[(int64_t)s * n + i] + probe[(int64_t)s * n + i];
            *c = total < slot_max[s] ? total : (*c > slot_max[s] ? *c : slot_max[s]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Monitor.record
// The plane and aperture test of one segment (monitor.py:183-193): the segment in the monitor's frame, direction renormalised
// (ray_to_local_coordinates), the crossing of the plane x = 0 within the segment's length and the rectangle.  One definition
// for every monitor kernel (k_mon_count / k_mon_emit, k_mon_wave, k_mon_spots): P = local hit point, t = distance.
// In two halves, which mon_hit puts together: the segment in the monitor's frame (mon_local), and the crossing of the plane
// x = 0 by a segment whose local origin has the x coordinate `ox` (mon_cross) — the monitor's own plane for ox = l.ox, the
// plane moved by d along the monitor's normal (the local x axis, column 0 of M) for ox = l.ox - d (k_mon_spots).
struct MonLocal {
    double ox, oy, oz, dx, dy, dz;
};
__device__ __forceinline__ MonLocal mon_local(const ot_monitor& mon, double sox, double soy, double soz, double sdx, double sdy, double sdz) {
    const double rx = sox - mon.origin[0], ry = soy - mon.origin[1], rz = soz - mon.origin[2];
    const double* M = mon.M;
    const double ox = M[0] * rx + M[3] * ry + M[6] * rz, oy = M[1] * rx + M[4] * ry + M[7] * rz,
                 oz = M[2] * rx + M[5] * ry + M[8] * rz;
    double dx = M[0] * sdx + M[3] * sdy + M[6] * sdz, dy = M[1] * sdx + M[4] * sdy + M[7] * sdz,
           dz = M[2] * sdx + M[5] * sdy + M[8] * sdz;
    const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);  // ray_to_local_coordinates renormalises
    dx *= inv; dy *= inv; dz *= inv;
    return {ox, oy, oz, dx, dy, dz};
}
__device__ __forceinline__ bool mon_cross(const ot_monitor& mon, const MonLocal& l, double ox, double slen, double& Px, double& Py, double& Pz,
                                          double& t) {
    if (l.dx == 0.0) return false;
    t = -ox / l.dx;
    if (fabs(t) < 1e-9 || t < 0.0 || t > slen) return false;
    Px = ox + t * l.dx; Py = l.oy + t * l.dy; Pz = l.oz + t * l.dz;
    return fabs(Py) <= mon.half_width && fabs(Pz) <= mon.half_height;
}
__device__ __forceinline__ bool mon_hit(const ot_monitor& mon, double sox, double soy, double soz, double sdx, double sdy, double sdz, double slen,
                                        double& Px, double& Py, double& Pz, double& t) {
    const MonLocal l = mon_local(mon, sox, soy, soz, sdx, sdy, sdz);
    return mon_cross(mon, l, l.ox, slen, Px, Py, Pz, t);
}

// ------------------------------------------------------------------------------------------
// Monitor.record on up to MON_MAX monitors in one pass over the segments (ot_monitor_record_many), in two kernels that share
// one partition of the slots: workgroup g owns the slots [g * span, (g + 1) * span), span = iters * MON_THREADS, and visits
// them MON_THREADS at a time.  k_mon_count leaves count[m][g]; an exclusive_scan over them in monitor-major order gives every
// workgroup its place in ONE concatenated output (monitor 0's hits, then monitor 1's, ...); k_mon_emit runs the same loads
// and tests and writes each hit there, so the hits of a monitor come out in ascending slot order.  No per-slot scratch.
// A segment is read where it lies, in either precision (fp32 widened in registers: exact): field f of slot s at
//   base[f] + (s >> 6) * tile_stride + (s & 63) * width
// — a block of 64-slot tiles with tile_stride = its tile size, plain arrays (slot arrays, planes of an append block) with
// tile_stride = 64 * width.  Layout and precision are launch arguments: uniform branches in kernels bound by their loads.
static constexpr int MON_THREADS = 256, MON_WAVES = MON_THREADS / 64, MON_MAX = 32;
struct MonSource {
    const uint8_t* base[7];  // ox oy oz dx dy dz length
    const uint8_t* ray;      // int32 per slot, read only for lists with holes
    int64_t tile_stride, ray_stride;
    int32_t width;
};
struct MonSeg {
    double ox, oy, oz, dx, dy, dz, len;
    bool valid;
};
__device__ __forceinline__ double mon_real(const uint8_t* p, int32_t width) {
    return width == 8 ? *reinterpret_cast<const double*>(p) : (double)*reinterpret_cast<const float*>(p);
}
// The partition, said once: the slots of workgroup blockIdx.x, visit by visit.  Visit `it` is the MON_THREADS slots from at(it).
struct MonSpan {
    int64_t first, n;
    int32_t iters;
    __device__ __forceinline__ int64_t at(int32_t it) const { return first + (int64_t)it * MON_THREADS; }
    __device__ __forceinline__ bool has(int32_t it) const { return it < iters && at(it) < n; }
};
__device__ __forceinline__ MonSpan mon_span(int64_t n, int32_t iters) { return {(int64_t)blockIdx.x * iters * MON_THREADS, n, iters}; }
// The addressing rule, said once: the byte offset of slot s in a plane of 64-slot tiles `stride` bytes apart, `width` bytes a slot
// (a field: src.tile_stride, src.width; the ray plane: src.ray_stride, 4) ...
__device__ __forceinline__ int64_t mon_at(int64_t s, int64_t stride, int32_t width) { return (s >> 6) * stride + (s & 63) * width; }
// ... and its scalar form for the passes that keep few registers: the 64 slots of a wave are one tile, so its place is a scalar
// (mon_tile, through v_readfirstlane) and the lane's within it one 32-bit offset for every plane
__device__ __forceinline__ int64_t mon_tile(int64_t s) { return __builtin_amdgcn_readfirstlane((int32_t)(s >> 6)); }
__device__ __forceinline__ const uint8_t* mon_in_tile(const uint8_t* plane, int64_t tile, int64_t stride, int lane, int32_t width) {
    return plane + tile * stride + (uint32_t)(lane * width);
}
// slot s and whether it holds a segment: k < |seg_count[ray]| in [k][ray] slots, ray >= 0 in lists with holes (n_rays < 0)
__device__ __forceinline__ MonSeg mon_load(const MonSource& src, int64_t s, int64_t n, const int32_t* __restrict__ seg_count, int64_t n_rays) {
    MonSeg g;
    g.ox = g.oy = g.oz = g.dx = g.dy = g.dz = g.len = 0.0;
    g.valid = s < n;
    if (!g.valid) return g;
    if (seg_count) {
        const uint32_t nr = (uint32_t)n_rays, su = (uint32_t)s;  // (n < 2^31)
        const int32_t c = seg_count[su % nr];
        g.valid = (int32_t)(su / nr) < (c < 0 ? -c : c);
    } else if (n_rays < 0) {
        g.valid = *reinterpret_cast<const int32_t*>(src.ray + mon_at(s, src.ray_stride, 4)) >= 0;
    }
    if (!g.valid) return g;
    const int64_t at = mon_at(s, src.tile_stride, src.width);
    g.ox = mon_real(src.base[0] + at, src.width); g.oy = mon_real(src.base[1] + at, src.width); g.oz = mon_real(src.base[2] + at, src.width);
    g.dx = mon_real(src.base[3] + at, src.width); g.dy = mon_real(src.base[4] + at, src.width); g.dz = mon_real(src.base[5] + at, src.width);
    g.len = mon_real(src.base[6] + at, src.width);
    return g;
}
// The image mode of k_mon_count (ot_monitor_image_many): the same partition, loads and tests, tallied by (monitor, bin) instead
// of (monitor, workgroup).  All zero for ot_monitor_record_many.  A hit at the local point P of monitor m has the coordinates
// y = P . a_y[m], z = P . a_z[m] (axes[m] = a_y, a_z) and the weight intensity[s], addressed like the fields of MonSource; it
// lands in bin (ky, kz) of the monitor's edge tables (edges[m] = nby + 1 edges of y, then nbz + 1 of z) or is dropped.
// lds_bins = n_mon * nby * nbz when the workgroup keeps a private image of the launch's monitors in dynamic LDS (lds_bins doubles,
// then lds_bins int32: 12 bytes a bin; lds_image_zero, lds_image_flush); 0 when every hit goes to global memory at once (an
// image no LDS holds).  MON_IMG_LDS_BINS: what fits 64 KB of LDS a
// workgroup — the most a launch gets without a function attribute, two workgroups per CU — next to the 128 bytes of `total`.
// Counts are integers, exact and the same every run; the weights are fp64 atomic adds, whose last bits depend on arrival order.
static constexpr int MON_IMG_LDS_BINS = (65536 - MON_MAX * 4) / 12;  // 5450: six monitors of 30 x 30
static constexpr int MON_IMG_MAX_BINS = 1 << 24;                     // nby * nbz of one monitor
struct MonImage {
    unsigned long long* counts;  // [n_mon][nby][nbz], of the launch's first monitor on; NULL: no image mode
    double* weights;             // same shape
    const double* edges;         // [n_mon][nby + 1 + nbz + 1]
    const double* axes;          // [n_mon][6]
    const uint8_t* intensity;
    int32_t nby, nbz, lds_bins;
};
// The bin of v among the edges e[0 .. nb]: k with e[k] <= v < e[k + 1], the last bin closed at e[nb] (np.histogram's rule);
// -1 for everything else, NaN included.  The guess comes from the range, the answer from the table: exact for every double.
__device__ __forceinline__ int32_t mon_bin(const double* __restrict__ e, int32_t nb, double v) {
    const double lo = e[0], hi = e[nb];
    if (!(v >= lo && v <= hi)) return -1;
    int32_t k = (int32_t)((v - lo) * (double)nb / (hi - lo));
    k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
    while (k > 0 && v < e[k]) --k;
    while (k < nb - 1 && v >= e[k + 1]) ++k;
    return k;
}
// What the image passes share (the image, field and beam modes of k_mon_count, k_mon_wave, k_seg_raster) is written once, here and
// above: the partition (MonSpan), the addressing rule (mon_at; mon_tile / mon_in_tile), the bin rule (mon_image_bin), a deposit
// (lds_image_deposit; mon_tally, mon_add), the workgroup's LDS image (lds_image_zero, lds_image_flush) and, further down, the
// wavelength of a ray (mon_wavelength) and the spot of a hit (mon_spot).  Each pass below says only what is its own.  The
// expressions are the ones the passes held in copies; against those copies k_mon_count has 124 vector registers for 126 (132
// scalar spills for 127), k_mon_wave 123 for 125, k_mon_emit 65 for 67, k_seg_raster 71 as before, and none has scratch or a
// vector spill (times: DESIGN.md 4.6).
// What stays in a copy of its own, marked where it stands:
//   - THE BEAM PASS, whole (mon_beam_deposit, mon_beam_pass), but for the wavelength arguments.  Built from the pieces above it
//     computed the same and kept its registers, and beam_all took 1.2 % (narrow spots) to 4.5 % (wide) longer: k_mon_count
//     lives on some 130 spilled scalars, and where the allocator puts them in the loop that takes the hits one at a time decides
//     its time.  Three partial forms (the deposit alone, with the tile addressing, with the wavelength and the spot written
//     out) stayed 0.8 to 1.4 % behind; written out, the pass is where it was.
//   - "the wave takes its hits one at a time" in k_mon_wave: two lines around a call whose operands are the mode's; a helper
//     taking a callable is three lines and leaves the site as long as it is;
//   - the chunked two-phase deposit of k_mon_wave (mon_wave_deposit).  One walk for it and mon_beam_deposit, taking "fill the
//     strip" and "combine" as callables, was built: one code line shorter than the two copies, k_mon_wave at 127 vector
//     registers for 123 — one short of the 128 its launch bounds and the LDS budgets stand on.  Not worth a line.
// The bin rule: the image coordinates (y0, z0) of the local hit point P on monitor m and its bin among the launch's
// [n_mon][nby][nbz], or -1 outside the image.
__device__ __forceinline__ int32_t mon_image_bin(const MonImage& img, int32_t m, double Px, double Py, double Pz, double& y0, double& z0) {
    const double* a = img.axes + 6 * m;
    const double* e = img.edges + (int64_t)m * (img.nby + img.nbz + 2);
    y0 = Px * a[0] + Py * a[1] + Pz * a[2];
    z0 = Px * a[3] + Py * a[4] + Pz * a[5];
    const int32_t ky = mon_bin(e, img.nby, y0), kz = mon_bin(e + img.nby + 1, img.nbz, z0);
    return ky < 0 || kz < 0 ? -1 : m * (img.nby * img.nbz) + ky * img.nbz + kz;
}
// A deposit that spreads (k_mon_wave): the count of the centre (mon_tally) apart from v on a plane of a footprint's bin (mon_add),
// into the workgroup's LDS image (`lds`: the launch keeps one) or straight to global memory.
__device__ __forceinline__ void mon_tally(int32_t lds, int32_t* tally, unsigned long long* counts, int32_t bin) {
    if (lds) atomicAdd(&tally[bin], 1);
    else atomicAdd(&counts[bin], 1ull);
}
__device__ __forceinline__ void mon_add(int32_t lds, double* in_lds, double* in_global, int32_t bin, double v) {
    if (lds) unsafeAtomicAdd(&in_lds[bin], v);
    else unsafeAtomicAdd(&in_global[bin], v);
}
// The workgroup's LDS image: P planes of `bins` doubles, then `bins` int32 tallies (bins = 0: none, and both loops are empty).
// Zeroed before the first visit; flushed after the last, consecutive lanes consecutive bins, non-zero values only.  The flush
// rule is the mode's: a pass that deposits where it counts (image, field, raster) adds the planes of a bin when its count is not
// zero; one that spreads a hit over a footprint (beam, wave: PER_PLANE) adds the count and each plane when itself is not zero.
template <int P> __device__ __forceinline__ int32_t* lds_image_tally(double* planes, int32_t bins) {
    return reinterpret_cast<int32_t*>(planes + P * bins);
}
template <int P> __device__ __forceinline__ void lds_image_zero(double* planes, int32_t bins) {
    int32_t* tally = lds_image_tally<P>(planes, bins);
    for (int32_t b = threadIdx.x; b < bins; b += MON_THREADS) {
#pragma unroll
        for (int p = 0; p < P; ++p) planes[p * bins + b] = 0.0;
        tally[b] = 0;
    }
    __syncthreads();
}
// One hit or piece that deposits where it counts: a count and v0 (v1 on the second plane).  The count comes LAST in the LDS arm
// and first in the other: where both arms end in the same add, the compiler merges the two into one add on a selected address
// — a flat atomic, which cost the LDS path of k_seg_raster's walk 4 %.
template <int P>
__device__ __forceinline__ void lds_image_deposit(double* planes, int32_t bins, unsigned long long* counts, double* out0, double* out1, int32_t bin,
                                                  double v0, double v1 = 0.0) {
    if (bins) {
        unsafeAtomicAdd(&planes[bin], v0);
        if (P > 1) unsafeAtomicAdd(&planes[bins + bin], v1);
        atomicAdd(&lds_image_tally<P>(planes, bins)[bin], 1);
    } else {
        atomicAdd(&counts[bin], 1ull);
        unsafeAtomicAdd(&out0[bin], v0);
        if (P > 1) unsafeAtomicAdd(&out1[bin], v1);
    }
}
template <int P, bool PER_PLANE>
__device__ __forceinline__ void lds_image_flush(double* planes, int32_t bins, unsigned long long* counts, double* out0, double* out1 = nullptr) {
    int32_t* tally = lds_image_tally<P>(planes, bins);
    __syncthreads();
    for (int32_t b = threadIdx.x; b < bins; b += MON_THREADS) {
        const int32_t c = tally[b];
        if (c) atomicAdd(&counts[b], (unsigned long long)c);
        if (!PER_PLANE && !c) continue;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const double v = planes[p * bins + b];
            if (!PER_PLANE || v != 0.0) unsafeAtomicAdd(&(p ? out1 : out0)[b], v);
        }
    }
}
// One workgroup's part of an image pass: k_mon_count's partition, loads and tests, every hit binned where the record mode counts it.
__device__ __forceinline__ void mon_image_pass(const ot_monitor* __restrict__ mons, int32_t n_mon, const MonSource& src, int64_t n, int32_t iters,
                                               const int32_t* __restrict__ seg_count, int64_t n_rays, const MonImage& img, double* weight) {
    lds_image_zero<1>(weight, img.lds_bins);
    const MonSpan span = mon_span(n, iters);
    for (int32_t it = 0; span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        double w = 0.0;
        bool have_w = false;  // the intensity of a slot is read once, at its first hit inside an image
        for (int32_t m = 0; m < n_mon; ++m) {
            double Px, Py, Pz, t, y0, z0;
            if (!(g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, Px, Py, Pz, t))) continue;
            const int32_t bin = mon_image_bin(img, m, Px, Py, Pz, y0, z0);
            if (bin < 0) continue;
            if (!have_w) {
                w = mon_real(img.intensity + mon_at(s, src.tile_stride, src.width), src.width);
                have_w = true;
            }
            lds_image_deposit<1>(weight, img.lds_bins, img.counts, img.weights, nullptr, bin, w);
        }
    }
    lds_image_flush<1, false>(weight, img.lds_bins, img.counts, img.weights);
}
// The wavelength arguments of the field, beam and wave modes, and the one rule they are read by: the wavelength of a slot is
// table[ray[s]] or, with no table, `uniform`.  mon_wavelength is false — the hit adds nothing and the caller counts it in
// *skipped — when the ray is outside [0, n) (nothing is read out of range) or the wavelength is not finite and > 0.
struct MonWavelength {
    const double* table;  // [n], or NULL: `uniform` for every ray
    unsigned long long* skipped;
    double uniform;
    int32_t n;
};
__device__ __forceinline__ bool mon_wavelength(const MonWavelength& lam, const uint8_t* ray_of_slot, double& wl) {
    wl = lam.uniform;
    bool known = true;
    if (lam.table) {
        const int32_t ray = *reinterpret_cast<const int32_t*>(ray_of_slot);
        known = ray >= 0 && ray < lam.n;
        if (known) wl = lam.table[ray];
    }
    return known && wl > 0.0 && wl < HUGE_VAL;
}
// The field mode of k_mon_count (ot_monitor_field_many): the image mode's partition, loads, tests and bin rule, with a phasor in
// place of the weight.  All zero for the two other modes.  A hit of slot s at the distance t has the optical path
// L = t * n[s] + pathlength[s] (Ray.pathlength(t)), x = L / wavelength cycles, the phase 2 pi (x - floor x) (Ray.phase(t)) and the
// amplitude sqrt(intensity[s]) (amplitude_mode 0) or intensity[s] (1); its bin gets a cos, a sin and one count.  n and pathlength are
// addressed like the fields of MonSource and read as doubles (the host refuses single precision); the wavelength is the ray's
// (MonWavelength).  A hit inside the image whose ray has no usable wavelength adds nothing and is counted in *lam.skipped.
// Through LDS: re[lds_bins], im[lds_bins] (double), tally[lds_bins] (int32) — 20 bytes a bin.
static constexpr int MON_FIELD_LDS_BINS = (65536 - MON_MAX * 4) / 20;  // 3270: three monitors of 30 x 30
struct MonField {
    double *re, *im;  // [n_mon][nby][nbz], of the launch's first monitor on; re NULL: no field mode
    const uint8_t *n_index, *pathlength;
    MonWavelength lam;
    int32_t amplitude_mode;
};
__device__ __forceinline__ void mon_field_pass(const ot_monitor* __restrict__ mons, int32_t n_mon, const MonSource& src, int64_t n, int32_t iters,
                                               const int32_t* __restrict__ seg_count, int64_t n_rays, const MonImage& img, const MonField& fld,
                                               double* re) {
    lds_image_zero<2>(re, img.lds_bins);  // (re, then im)
    const MonSpan span = mon_span(n, iters);
    int32_t skipped = 0;
    for (int32_t it = 0; span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        double a = 0.0, n_index = 0.0, pl = 0.0, wl = 0.0;
        int32_t have = 0;  // amplitude, index, path and wavelength of a slot are read once, at its first hit inside an image; -1: refused
        for (int32_t m = 0; m < n_mon; ++m) {
            double Px, Py, Pz, t, y0, z0;
            if (!(g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, Px, Py, Pz, t))) continue;
            const int32_t bin = mon_image_bin(img, m, Px, Py, Pz, y0, z0);
            if (bin < 0) continue;
            if (!have) {
                have = mon_wavelength(fld.lam, src.ray + mon_at(s, src.ray_stride, 4), wl) ? 1 : -1;
                if (have > 0) {
                    const int64_t at = mon_at(s, src.tile_stride, 8);
                    a = *reinterpret_cast<const double*>(img.intensity + at);
                    if (fld.amplitude_mode == 0) a = sqrt(a);
                    n_index = *reinterpret_cast<const double*>(fld.n_index + at);
                    pl = *reinterpret_cast<const double*>(fld.pathlength + at);
                }
            }
            if (have < 0) {
                ++skipped;
                continue;
            }
            const double L = t * n_index + pl;
            const double x = L / wl;
            const double f = x - floor(x);
            double sn, cs;
            sincospi(2.0 * f, &sn, &cs);
            lds_image_deposit<2>(re, img.lds_bins, img.counts, fld.re, fld.im, bin, a * cs, a * sn);
        }
    }
    if (skipped) atomicAdd(fld.lam.skipped, (unsigned long long)skipped);
    lds_image_flush<2, false>(re, img.lds_bins, img.counts, fld.re, fld.im);
}
// The beam mode of k_mon_count (ot_monitor_beam_many): the image mode's partition, loads, tests and bin rule for the count, with
// the hit's power spread over its Gaussian spot.  All zero for the three other modes.  A hit of slot s at the distance t and the
// image coordinates (y0, z0) carries q = q_re[s] + t + i q_im[s] (GaussianBeam.q_at_z) and the spot size
//   w^2 = wavelength (qr^2 + qi^2) / (n[s] pi qi)            (Ray.spot_size(t), written without the reciprocal)
// and bin (ky, kz) gets intensity[s] Fy(ky) Fz(kz), Fy(k) = (erf(sqrt2 (ey[k + 1] - y0) / w) - erf(sqrt2 (ey[k] - y0) / w)) / 2: the
// integral over the bin of I 2 / (pi w^2) exp(-2 r^2 / w^2), the beam taken at normal incidence.  Bins whose nearer edge lies
// more than 5 w from the centre along an axis are left out (a share below erfc(5 sqrt2) = 1.5e-23).  All in double precision;
// intensity, q_re, q_im and n are addressed like the fields of MonSource, in its precision; the wavelength as in the field mode.
// A hit without a usable wavelength (mon_wavelength) or whose n, qi or w is not finite and > 0 (mon_spot) adds nothing and is
// counted in *lam.skipped.
// One hit has a footprint of 1 to nby * nbz bins, so the deposit is the wave's work, not the lane's: every lane finds its own
// slot's hit, counts its centre and steps out its footprint (64 searches side by side), then the wave takes the hits with a
// footprint one at a time (the lowest set bit of their ballot; y0, z0, w, I and the footprint come through v_readlane, as
// scalars), its lanes evaluate erf at the footprint's edges — 63 x 63 bins at a time: 64 + 64 edges, one erf a lane or two — into
// the wave's strip of LDS, and then stride over the footprint's bins with one atomic add each.  fy + fz + 2 erfs a hit instead of
// fy * fz and no private array.  Registers: the pass reads q, n, the wavelength and the intensity at every hit instead of keeping
// them from one monitor of a slot to the next, and erf is a call (mon_beam_erf) — k_mon_count stays within 128 registers.
// Wave-synchronous throughout: the strip is the wave's own, its LDS operations retire in order, and the wavefront fences keep
// the compiler from moving a read across a write.  No barrier inside the visit loop.
// Through LDS: MON_WAVES strips of MON_BEAM_STRIP doubles, then power[lds_bins] (double), then tally[lds_bins] (int32): 12 bytes
// a bin next to 4 KB of strips (the strips are there on the global path too).
static constexpr int MON_BEAM_STRIP = 128, MON_BEAM_CHUNK = 63;  // erf at the 64 + 64 edges of 63 x 63 bins
static constexpr int MON_BEAM_LDS_BINS = (65536 - MON_MAX * 4 - MON_WAVES * MON_BEAM_STRIP * 8) / 12;  // 5109: five monitors of 30 x 30
struct MonBeam {
    double* power;  // [n_mon][nby][nbz], of the launch's first monitor on; NULL: no beam mode
    const uint8_t *q_re, *q_im, *n_index;
    MonWavelength lam;
};
// The spot of a hit (k_mon_wave; the beam pass below holds the same expressions written out): |q|^2, w^2 = wl |q|^2 / (n pi qi) and w.  false — the hit adds nothing and is counted
// in *skipped — when n, qi or w is not finite and > 0.
__device__ __forceinline__ bool mon_spot(double qr, double qi, double n_index, double wl, double& q2, double& w2, double& w) {
    q2 = qr * qr + qi * qi;
    w2 = wl * q2 / (n_index * M_PI * qi);
    w = sqrt(w2);
    return n_index > 0.0 && n_index < HUGE_VAL && qi > 0.0 && qi < HUGE_VAL && w > 0.0 && w < HUGE_VAL;
}
// lane `from`'s v in every lane (from is wave-uniform): a scalar
__device__ __forceinline__ double mon_lane_value(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}
// The footprint of [lo, hi] among the bins of e[0 .. nb]: the first bin whose upper edge is >= lo (nb: none) and the last whose
// lower edge is <= hi (-1: none).  As in mon_bin the guess comes from the range and the answer from the table.
__device__ __forceinline__ int32_t mon_beam_guess(const double* __restrict__ e, int32_t nb, double v) {
    const float g = (float)(v - e[0]) * (float)nb / (float)(e[nb] - e[0]);  // (single precision will do: the table decides)
    return (int32_t)fminf(fmaxf(g, 0.0f), (float)(nb - 1));                 // (a NaN guess starts at 0)
}
__device__ __forceinline__ int32_t mon_beam_first(const double* __restrict__ e, int32_t nb, double lo) {
    int32_t k = mon_beam_guess(e, nb, lo);
    while (k > 0 && e[k] >= lo) --k;
    while (k < nb && e[k + 1] < lo) ++k;
    return k;
}
__device__ __forceinline__ int32_t mon_beam_last(const double* __restrict__ e, int32_t nb, double hi) {
    int32_t k = mon_beam_guess(e, nb, hi);
    while (k >= 0 && e[k] > hi) --k;
    while (k < nb - 1 && e[k + 1] <= hi) ++k;
    return k;
}
// erf as a call, not inlined: inlined, the coefficients of its polynomials are hoisted out of every loop of the pass and sit in 42
// vector registers from its first instruction to its last (157 registers, or 128 and scratch)
__device__ __noinline__ double mon_beam_erf(double x) { return erf(x); }
// One hit, by its whole wave: centre (y0, z0), spot size w, power I and the footprint ky0 .. ky1 x kz0 .. kz1 are wave-uniform; the
// monitor's nby x nbz bins of power are `in_lds` or, when that is NULL, `in_global`.
// (This deposit and the pass below are WRITTEN OUT — zero, partition, tile addressing, wavelength, spot, bin, count, flush and the
// walk that mon_wave_deposit repeats: built from the shared pieces beam_all was 1.2 to 4.5 % slower, see "What stays" above.)
__device__ __forceinline__ void mon_beam_deposit(const double* __restrict__ ey, const double* __restrict__ ez, int32_t nbz, double y0, double z0, double w,
                                                 double I, int32_t ky0, int32_t ky1, int32_t kz0, int32_t kz1, double* strip, int lane, double* in_lds,
                                                 double* in_global) {
    for (int32_t by = ky0; by <= ky1; by += MON_BEAM_CHUNK) {
        const int32_t ny = min(MON_BEAM_CHUNK, ky1 - by + 1);
        for (int32_t bz = kz0; bz <= kz1; bz += MON_BEAM_CHUNK) {
            const int32_t nz = min(MON_BEAM_CHUNK, kz1 - bz + 1);
            // strip[0 .. ny] = erf at the y edges by .. by + ny, strip[ny + 1 .. ny + nz + 1] = at the z edges bz .. bz + nz
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int32_t j = lane; j < ny + nz + 2; j += 64) {
                const double d = j <= ny ? ey[by + j] - y0 : ez[bz + j - ny - 1] - z0;
                strip[j] = mon_beam_erf(M_SQRT2 * d / w);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int32_t b = lane; b < ny * nz; b += 64) {
                const int32_t iy = b / nz, iz = b - iy * nz;
                const double fy = 0.5 * (strip[iy + 1] - strip[iy]), fz = 0.5 * (strip[ny + iz + 2] - strip[ny + iz + 1]);
                const double share = I * fy * fz;
                if (share == 0.0) continue;
                if (in_lds) unsafeAtomicAdd(&in_lds[(by + iy) * nbz + bz + iz], share);
                else unsafeAtomicAdd(&in_global[(by + iy) * nbz + bz + iz], share);
            }
        }
    }
}
__device__ __forceinline__ void mon_beam_pass(const ot_monitor* __restrict__ mons, int32_t n_mon, const MonSource& src, int64_t n, int32_t iters,
                                              const int32_t* __restrict__ seg_count, int64_t n_rays, const MonImage& img, const MonBeam& beam,
                                              double* strips, double* power, int32_t* tally) {
    for (int32_t b = threadIdx.x; b < img.lds_bins; b += MON_THREADS) power[b] = 0.0, tally[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    double* strip = strips + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * MON_BEAM_STRIP;
    const int32_t per_mon = img.nby * img.nbz;
    const int64_t first = (int64_t)blockIdx.x * iters * MON_THREADS;
    int32_t skipped = 0;
    for (int32_t it = 0; it < iters && first + (int64_t)it * MON_THREADS < n; ++it) {
        const int64_t s = first + (int64_t)it * MON_THREADS + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        // the 64 slots of a wave are one tile: its place is a scalar, and the lane's within it one 32-bit offset for every plane
        const int64_t tile = __builtin_amdgcn_readfirstlane((int32_t)(s >> 6));
        const int64_t at_tile = tile * src.tile_stride;
        const uint32_t at_lane = (uint32_t)(lane * src.width);
        for (int32_t m = 0; m < n_mon; ++m) {
            double Px, Py, Pz, t;
            const bool hit = g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, Px, Py, Pz, t);
            if (!__ballot(hit)) continue;
            const double* ax = img.axes + 6 * m;
            const double* ey = img.edges + (int64_t)m * (img.nby + img.nbz + 2);
            const double* ez = ey + img.nby + 1;
            // the lane's own hit: its spot (nothing of a slot is kept from one monitor to the next: the registers are erf's), the
            // count of its centre, its footprint
            double y0 = 0.0, z0 = 0.0, w = 0.0, I = 0.0;
            int32_t ky0 = 0, ky1 = -1, kz0 = 0, kz1 = -1;
            if (hit) {
                double wl = beam.lam.uniform;
                bool usable = true;
                if (beam.lam.table) {
                    const int32_t ray = *reinterpret_cast<const int32_t*>(src.ray + tile * src.ray_stride + (uint32_t)(lane * 4));
                    usable = ray >= 0 && ray < beam.lam.n;
                    if (usable) wl = beam.lam.table[ray];
                }
                const double qr = mon_real(beam.q_re + at_tile + at_lane, src.width) + t, qi = mon_real(beam.q_im + at_tile + at_lane, src.width);
                const double n_index = mon_real(beam.n_index + at_tile + at_lane, src.width);
                w = sqrt(wl * (qr * qr + qi * qi) / (n_index * M_PI * qi));
                usable = usable && wl > 0.0 && wl < HUGE_VAL && n_index > 0.0 && n_index < HUGE_VAL && qi > 0.0 && qi < HUGE_VAL && w > 0.0 && w < HUGE_VAL;
                if (usable) {
                    I = mon_real(img.intensity + at_tile + at_lane, src.width);
                    y0 = Px * ax[0] + Py * ax[1] + Pz * ax[2];
                    z0 = Px * ax[3] + Py * ax[4] + Pz * ax[5];
                    const int32_t ky = mon_bin(ey, img.nby, y0), kz = mon_bin(ez, img.nbz, z0);
                    if (ky >= 0 && kz >= 0) {  // the centre is counted where the image mode counts the hit
                        const int32_t bin = m * per_mon + ky * img.nbz + kz;
                        if (img.lds_bins) atomicAdd(&tally[bin], 1);
                        else atomicAdd(&img.counts[bin], 1ull);
                    }
                    const double reach = 5.0 * w;
                    ky0 = mon_beam_first(ey, img.nby, y0 - reach), ky1 = mon_beam_last(ey, img.nby, y0 + reach);
                    kz0 = mon_beam_first(ez, img.nbz, z0 - reach), kz1 = mon_beam_last(ez, img.nbz, z0 + reach);
                } else {
                    ++skipped;
                }
            }
            // the wave takes its hits one at a time
            for (unsigned long long rest = __ballot(ky0 <= ky1 && kz0 <= kz1); rest; rest &= rest - 1) {
                const int from = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rest));
                mon_beam_deposit(ey, ez, img.nbz, mon_lane_value(y0, from), mon_lane_value(z0, from), mon_lane_value(w, from), mon_lane_value(I, from),
                                 __builtin_amdgcn_readlane(ky0, from), __builtin_amdgcn_readlane(ky1, from), __builtin_amdgcn_readlane(kz0, from),
                                 __builtin_amdgcn_readlane(kz1, from), strip, lane, img.lds_bins ? power + m * per_mon : nullptr,
                                 beam.power + (int64_t)m * per_mon);
            }
        }
    }
    if (skipped) atomicAdd(beam.lam.skipped, (unsigned long long)skipped);
    __syncthreads();
    for (int32_t b = threadIdx.x; b < img.lds_bins; b += MON_THREADS) {  // consecutive lanes, consecutive bins
        const int32_t c = tally[b];
        const double p = power[b];
        if (c) atomicAdd(&img.counts[b], (unsigned long long)c);
        if (p != 0.0) unsafeAtomicAdd(&beam.power[b], p);
    }
}
// count[m * gridDim.x + g] = hits of monitor m among workgroup g's slots; count[n_mon * gridDim.x] = 0, so that the scan's last
// element is the total.  In image, field and beam mode (img.counts set: one uniform branch at entry) `count` is not touched.
__global__ __launch_bounds__(MON_THREADS) void k_mon_count(const ot_monitor* __restrict__ mons, int32_t n_mon, MonSource src, int64_t n, int32_t iters,
                                                           const int32_t* __restrict__ seg_count, int64_t n_rays, int32_t* __restrict__ count,
                                                           MonImage img, MonField fld, MonBeam beam) {
    __shared__ int32_t total[MON_MAX];
    // through LDS: weights[lds_bins], then counts[lds_bins]; field mode: re, im, then counts; beam mode: the waves' strips, power, then counts
    extern __shared__ double mon_image[];
    if (img.counts) {
        if (beam.power)
            mon_beam_pass(mons, n_mon, src, n, iters, seg_count, n_rays, img, beam, mon_image, mon_image + MON_WAVES * MON_BEAM_STRIP,
                          lds_image_tally<1>(mon_image + MON_WAVES * MON_BEAM_STRIP, img.lds_bins));
        else if (fld.re)
            mon_field_pass(mons, n_mon, src, n, iters, seg_count, n_rays, img, fld, mon_image);
        else
            mon_image_pass(mons, n_mon, src, n, iters, seg_count, n_rays, img, mon_image);
        return;
    }
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < MON_MAX) total[threadIdx.x] = 0;
    __syncthreads();
    const MonSpan span = mon_span(n, iters);
    for (int32_t it = 0; span.has(it); ++it) {
        const MonSeg g = mon_load(src, span.at(it) + threadIdx.x, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        for (int32_t m = 0; m < n_mon; ++m) {  // m is wave-uniform: the monitor comes through scalar loads
            double Px, Py, Pz, t;
            const bool hit = g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, Px, Py, Pz, t);
            const unsigned long long b = __ballot(hit);
            if (lane == 0 && b) atomicAdd(&total[m], (int32_t)__popcll(b));
        }
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < n_mon) count[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = total[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) count[(int64_t)n_mon * gridDim.x] = 0;
}
// Coherent Gaussian-beam images (ot_monitor_wave_many), a kernel of its own — k_mon_count's partition, loads, tests and bin rule
// for the count, the beam pass's walk over a hit's footprint, with a complex, phase-carrying deposit SAMPLED AT THE BIN CENTRE.
// A hit of slot s at the distance t, at (y0, z0) = (P . a_y, P . a_z), of the segment direction d:
//   q = q_re[s] + t + i q_im[s],  |q|^2 = qr^2 + qi^2,  w^2 = wavelength |q|^2 / (n[s] pi qi)       (the beam pass's w)
//   ty = d . a_y, tz = d . a_z (MonitorHits.tYList / tZList),  a = sqrt(intensity[s]) (amplitude_mode 0) or intensity[s] (1)
//   cycles = (pathlength[s] + t n) / wavelength                         Ray.phase(t), as the field mode
//          + n (ty Dy + tz Dz) / wavelength                             tilt: the beam's plane-wave phase across the monitor
//          + n qr (Dy^2 + Dz^2) / (2 wavelength |q|^2)                  wavefront curvature, k r^2 / (2 R)
//   u(yc, zc) = a sqrt(2 / (pi w^2)) exp(-(Dy^2 + Dz^2) / w^2) exp(i (2 pi frac(cycles) - g)),   Dy = yc - y0, Dz = zc - z0
// with g = atan2(qr, qi) (gouy = 1: exp(-i g) = (qi - i qr) / |q|, no arc tangent is taken) or 0.  It is separable,
// u = A gy(Dy) gz(Dz): A = a sqrt(2 / (pi w^2)) exp(-i g),
// gy(D) = exp(-D^2 / w^2) exp(2 pi i frac(f + D (ry + kc D))) with f = frac(L / wavelength), ry = n ty / wavelength and
// kc = n qr / (2 wavelength |q|^2), gz likewise with f = 0 — one exp and one sincospi of a reduced cycle count per bin centre
// and axis.  All in double; the host refuses single-precision segments.
// The footprint of a hit is the bins whose CENTRE lies within 6 w of the hit's along either axis (beyond, the amplitude is below
// exp(-36) of the peak): a spot narrower than a bin that falls between the centres deposits nothing.  The envelope is taken at
// normal incidence and q is not advanced across the tilt.
// Sampling: the cycle rate along y is ry + 2 kc D, linear in D; where its largest magnitude over the footprint (at one of the two
// end centres) times the mean bin width (e[nb] - e[0]) / nb exceeds 0.5 on either axis, the hit is counted in *aliased — and is
// deposited all the same.  A hit without a usable wavelength or spot (mon_wavelength, mon_spot, as in the beam pass) adds nothing
// and is counted in *lam.skipped.
// As in the beam pass every lane finds its own slot's hit, counts its centre and steps out its footprint; the wave then takes the
// hits with a footprint one at a time (ballot, v_readlane), its lanes put A gy at the footprint's y centres and gz at its z
// centres into the wave's strip of LDS — 63 x 63 bins at a time, 63 + 63 complex values — and stride over the bins with one
// complex product and two atomic adds each: fy + fz exp / sincospi pairs a hit, not fy * fz.  Wave-synchronous, no barrier inside
// the visit loop, the beam pass's wavefront fences.
// Through LDS: MON_WAVES strips of MON_WAVE_STRIP doubles, re[lds_bins], im[lds_bins] (double), tally[lds_bins] (int32): 20 bytes a
// bin next to 8 KB of strips (and the 128 bytes the count kernel's tally takes, left free here: one rule for every budget).
static constexpr int MON_WAVE_STRIP = 256, MON_WAVE_CHUNK = 63;
static constexpr int MON_WAVE_LDS_BINS = (65536 - MON_MAX * 4 - MON_WAVES * MON_WAVE_STRIP * 8) / 20;  // 2860: three monitors of 30 x 30
struct MonWave {
    double *re, *im;  // [n_mon][nby][nbz], of the launch's first monitor on
    const uint8_t *q_re, *q_im, *n_index, *pathlength;
    MonWavelength lam;
    unsigned long long* aliased;
    int32_t amplitude_mode, gouy;
};
// exp and the phasor of a cycle count as calls, not inlined, as the beam pass's erf: inlined, their polynomials' coefficients are
// hoisted out of every loop of the kernel and held in vector registers from its first instruction to its last (223 registers)
__device__ __noinline__ double mon_wave_exp(double x) { return exp(x); }
__device__ __noinline__ double2 mon_wave_cis(double cycles) {  // (cos, sin) of 2 pi frac(cycles)
    double sn, cs;
    sincospi(2.0 * (cycles - floor(cycles)), &sn, &cs);
    return make_double2(cs, sn);
}
// exp(-D^2 / w2) exp(2 pi i frac(f + D (rate + kc D))): the factor of one axis at the distance D from the hit's centre
__device__ __forceinline__ void mon_wave_axis(double D, double w2, double f, double rate, double kc, double& re, double& im) {
    const double2 p = mon_wave_cis(f + D * (rate + kc * D));
    const double env = mon_wave_exp(-(D * D) / w2);
    re = env * p.x, im = env * p.y;
}
// One hit, by its whole wave: everything but `lane` is wave-uniform; the monitor's nby x nbz bins are re_lds / im_lds (`lds`: the
// launch keeps an image there) or re_global / im_global.
// (mon_beam_deposit's walk, written again: shared, it left this kernel 1 vector register of the 5 it has to spare.)
__device__ __forceinline__ void mon_wave_deposit(const double* __restrict__ ey, const double* __restrict__ ez, int32_t nbz, double y0, double z0, double w2,
                                                 double Are, double Aim, double f, double ry, double rz, double kc, int32_t ky0, int32_t ky1, int32_t kz0,
                                                 int32_t kz1, double* strip, int lane, int32_t lds, double* re_lds, double* im_lds, double* re_global,
                                                 double* im_global) {
    for (int32_t by = ky0; by <= ky1; by += MON_WAVE_CHUNK) {
        const int32_t ny = min(MON_WAVE_CHUNK, ky1 - by + 1);
        for (int32_t bz = kz0; bz <= kz1; bz += MON_WAVE_CHUNK) {
            const int32_t nz = min(MON_WAVE_CHUNK, kz1 - bz + 1);
            // strip[2 j], strip[2 j + 1] = A gy at the y centres by .. by + ny - 1 (j < ny), gz at the z centres bz .. (j - ny)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int32_t j = lane; j < ny + nz; j += 64) {
                const bool along_y = j < ny;
                const double* e = along_y ? ey + by + j : ez + bz + j - ny;
                const double D = 0.5 * (e[0] + e[1]) - (along_y ? y0 : z0);
                double gr, gi;
                mon_wave_axis(D, w2, along_y ? f : 0.0, along_y ? ry : rz, kc, gr, gi);
                strip[2 * j] = along_y ? Are * gr - Aim * gi : gr;
                strip[2 * j + 1] = along_y ? Are * gi + Aim * gr : gi;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int32_t b = lane; b < ny * nz; b += 64) {
                const int32_t iy = b / nz, iz = b - iy * nz;
                const double yr = strip[2 * iy], yi = strip[2 * iy + 1], zr = strip[2 * (ny + iz)], zi = strip[2 * (ny + iz) + 1];
                const double ur = yr * zr - yi * zi, ui = yr * zi + yi * zr;
                if (ur == 0.0 && ui == 0.0) continue;
                const int32_t bin = (by + iy) * nbz + bz + iz;
                mon_add(lds, re_lds, re_global, bin, ur);
                mon_add(lds, im_lds, im_global, bin, ui);
            }
        }
    }
}
// The bins of e[0 .. nb] whose centre lies in [lo, hi]: the footprint helpers of the beam pass give the bins that reach into
// the range, and the bin at either end is dropped when its centre is outside.
__device__ __forceinline__ void mon_wave_footprint(const double* __restrict__ e, int32_t nb, double lo, double hi, int32_t& k0, int32_t& k1) {
    k0 = mon_beam_first(e, nb, lo), k1 = mon_beam_last(e, nb, hi);
    if (k0 <= k1 && 0.5 * (e[k0] + e[k0 + 1]) < lo) ++k0;
    if (k0 <= k1 && 0.5 * (e[k1] + e[k1 + 1]) > hi) --k1;
}
__global__ __launch_bounds__(MON_THREADS, 4) void k_mon_wave(const ot_monitor* __restrict__ mons, int32_t n_mon, MonSource src, int64_t n, int32_t iters,
                                                          const int32_t* __restrict__ seg_count, int64_t n_rays, MonImage img, MonWave wav) {
    extern __shared__ double mon_wave_lds[];  // the waves' strips, then re, im, tally
    double* re = mon_wave_lds + MON_WAVES * MON_WAVE_STRIP;
    double* im = re + img.lds_bins;
    int32_t* tally = lds_image_tally<2>(re, img.lds_bins);
    lds_image_zero<2>(re, img.lds_bins);
    const int lane = threadIdx.x & 63;
    double* strip = mon_wave_lds + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * MON_WAVE_STRIP;
    const int32_t per_mon = img.nby * img.nbz;
    const MonSpan span = mon_span(n, iters);
    int32_t skipped = 0, aliased = 0;
    for (int32_t it = 0; span.has(it); ++it) {
        int32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // (opaque: the seven per-lane plane addresses are formed here, not held across the loop)
        const int64_t s = span.at(it) + tid;
        if (!__ballot(mon_load(src, s, n, seg_count, n_rays).valid)) continue;
        const int64_t tile = mon_tile(s);
        for (int32_t m = 0; m < n_mon; ++m) {
            // the segment again for every monitor (from the cache): held across the deposits it would cost 14 registers
            asm volatile("" : "+v"(tid));
            const MonSeg g = mon_load(src, span.at(it) + tid, n, seg_count, n_rays);
            double Px, Py, Pz, t;
            const bool hit = g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, Px, Py, Pz, t);
            if (!__ballot(hit)) continue;
            const double* ax = img.axes + 6 * m;
            const double* ey = img.edges + (int64_t)m * (img.nby + img.nbz + 2);
            const double* ez = ey + img.nby + 1;
            // the lane's own hit: A, w^2, the rates, the count of its centre, its footprint and the sampling test
            double y0 = 0.0, z0 = 0.0, w2 = 0.0, Are = 0.0, Aim = 0.0, f = 0.0, ry = 0.0, rz = 0.0, kc = 0.0;
            int32_t ky0 = 0, ky1 = -1, kz0 = 0, kz1 = -1;
            bool usable = true, alias = false;
            if (hit) {
                double wl, q2, w;
                usable = mon_wavelength(wav.lam, mon_in_tile(src.ray, tile, src.ray_stride, lane, 4), wl);
                const double qr = mon_real(mon_in_tile(wav.q_re, tile, src.tile_stride, lane, 8), 8) + t;
                const double qi = mon_real(mon_in_tile(wav.q_im, tile, src.tile_stride, lane, 8), 8);
                const double n_index = mon_real(mon_in_tile(wav.n_index, tile, src.tile_stride, lane, 8), 8);
                usable = mon_spot(qr, qi, n_index, wl, q2, w2, w) && usable;
                if (usable) {
                    const int32_t bin = mon_image_bin(img, m, Px, Py, Pz, y0, z0);
                    if (bin >= 0) mon_tally(img.lds_bins, tally, img.counts, bin);  // the centre is counted where the image mode counts the hit
                    const double reach = 6.0 * w;
                    mon_wave_footprint(ey, img.nby, y0 - reach, y0 + reach, ky0, ky1);
                    mon_wave_footprint(ez, img.nbz, z0 - reach, z0 + reach, kz0, kz1);
                    if (ky0 <= ky1 && kz0 <= kz1) {
                        double a = mon_real(mon_in_tile(img.intensity, tile, src.tile_stride, lane, 8), 8);
                        if (wav.amplitude_mode == 0) a = sqrt(a);
                        const double L = t * n_index + mon_real(mon_in_tile(wav.pathlength, tile, src.tile_stride, lane, 8), 8);
                        f = L / wl;
                        f -= floor(f);  // the cycles of the path ride along y: one phasor less a hit
                        Are = a * sqrt(2.0 / (M_PI * w2)), Aim = 0.0;
                        if (wav.gouy) {  // exp(-i g), g = atan2(qr, qi), is (qi - i qr) / |q|
                            const double inv = Are / sqrt(q2);
                            Are = qi * inv, Aim = -qr * inv;
                        }
                        ry = n_index * (g.dx * ax[0] + g.dy * ax[1] + g.dz * ax[2]) / wl;
                        rz = n_index * (g.dx * ax[3] + g.dy * ax[4] + g.dz * ax[5]) / wl;
                        kc = n_index * qr / (2.0 * wl * q2);
                        // the largest cycle rate over the footprint, at one of its end centres, in cycles a bin
                        const double by0 = 0.5 * (ey[ky0] + ey[ky0 + 1]) - y0, by1 = 0.5 * (ey[ky1] + ey[ky1 + 1]) - y0;
                        const double bz0 = 0.5 * (ez[kz0] + ez[kz0 + 1]) - z0, bz1 = 0.5 * (ez[kz1] + ez[kz1 + 1]) - z0;
                        const double turn_y = fmax(fabs(ry + 2.0 * kc * by0), fabs(ry + 2.0 * kc * by1)) * ((ey[img.nby] - ey[0]) / (double)img.nby);
                        const double turn_z = fmax(fabs(rz + 2.0 * kc * bz0), fabs(rz + 2.0 * kc * bz1)) * ((ez[img.nbz] - ez[0]) / (double)img.nbz);
                        alias = turn_y > 0.5 || turn_z > 0.5;
                    }
                }
            }
            // (wave-wide tallies: scalars)
            skipped += (int32_t)__popcll(__ballot(hit && !usable));
            aliased += (int32_t)__popcll(__ballot(alias));
            // the wave takes its hits one at a time (the beam pass's two lines again, around this mode's operands)
            for (unsigned long long rest = __ballot(ky0 <= ky1 && kz0 <= kz1); rest; rest &= rest - 1) {
                const int from = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rest));
                mon_wave_deposit(ey, ez, img.nbz, mon_lane_value(y0, from), mon_lane_value(z0, from), mon_lane_value(w2, from), mon_lane_value(Are, from),
                                 mon_lane_value(Aim, from), mon_lane_value(f, from), mon_lane_value(ry, from), mon_lane_value(rz, from), mon_lane_value(kc, from),
                                 __builtin_amdgcn_readlane(ky0, from), __builtin_amdgcn_readlane(ky1, from), __builtin_amdgcn_readlane(kz0, from),
                                 __builtin_amdgcn_readlane(kz1, from), strip, lane, img.lds_bins, re + m * per_mon, im + m * per_mon,
                                 wav.re + (int64_t)m * per_mon, wav.im + (int64_t)m * per_mon);
            }
        }
    }
    if (lane == 0 && skipped) atomicAdd(wav.lam.skipped, (unsigned long long)skipped);
    if (lane == 0 && aliased) atomicAdd(wav.aliased, (unsigned long long)aliased);
    lds_image_flush<2, true>(re, img.lds_bins, img.counts, wav.re, wav.im);
}
// off = the exclusive scan of count (n_mon * gridDim.x + 1 elements).  Position of a hit in the concatenated output: first[0]
// (the hits of the monitors of earlier launches: the host walks long lists MON_MAX monitors at a time) + off[m][g] + hits of
// monitor m in the workgroup's earlier visits + in the earlier waves of this visit + in the lower lanes (v_mbcnt).  Writes stop
// at `capacity`; first[1 .. n_mon] and *n_total are exact whatever the capacity.  A workgroup none of whose slots hit leaves
// without reading a segment, and only the monitors it has hits on are tested again.
__global__ __launch_bounds__(MON_THREADS) void k_mon_emit(const ot_monitor* __restrict__ mons, int32_t n_mon, MonSource src, int64_t n, int32_t iters,
                                                          const int32_t* __restrict__ seg_count, int64_t n_rays, const int64_t* __restrict__ off,
                                                          int64_t capacity, int64_t* first, int64_t* __restrict__ hit_index, double* __restrict__ Px,
                                                          double* __restrict__ Py, double* __restrict__ Pz, double* __restrict__ tt, int64_t* n_total) {
    __shared__ int32_t wave_hits[2][MON_MAX][MON_WAVES];  // [parity of the visit]: one barrier per visit
    __shared__ int32_t seen[MON_WAVES][MON_MAX];          // every wave's own copy of the hits of the workgroup's earlier visits
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t G = gridDim.x, before_launch = first[0];
    if (blockIdx.x == 0 && (int32_t)threadIdx.x < n_mon) first[threadIdx.x + 1] = before_launch + off[(int64_t)(threadIdx.x + 1) * G];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_total = before_launch + off[(int64_t)n_mon * G];
    bool mine = false;
    if (lane < n_mon) {
        const int64_t at = (int64_t)lane * G + blockIdx.x;
        mine = off[at + 1] != off[at];
    }
    const uint32_t live = (uint32_t)__ballot(mine);  // monitors this workgroup has hits on
    if (!live) return;
    // seen[wave][] is this wave's own: written and read by lanes of one wave only, whose LDS operations retire in order; the
    // wavefront fences keep the compiler from moving a read across the write before it
    if (lane < MON_MAX) seen[wave][lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const MonSpan span = mon_span(n, iters);
    for (int32_t it = 0; span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const int p = it & 1;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        uint32_t hits = 0;
        for (uint32_t rest = live; rest; rest &= rest - 1) {
            const int m = __builtin_ctz(rest);
            double x, y, z, t;
            const bool hit = g.valid && mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, x, y, z, t);
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wave_hits[p][m][wave] = (int32_t)__popcll(b);
            hits |= (hit ? 1u : 0u) << m;
        }
        __syncthreads();
        for (uint32_t rest = live; rest; rest &= rest - 1) {
            const int m = __builtin_ctz(rest);
            int32_t below = 0, all = 0;
#pragma unroll
            for (int w = 0; w < MON_WAVES; ++w) {
                const int32_t c = wave_hits[p][m][w];
                below += w < wave ? c : 0;
                all += c;
            }
            if (!all) continue;
            const bool hit = (hits >> m) & 1u;
            const unsigned long long b = __ballot(hit);
            const int32_t earlier = seen[wave][m];
            if (hit) {
                const int64_t d = before_launch + off[(int64_t)m * G + blockIdx.x] + earlier + below + rank_below(b);
                if (d < capacity) {
                    double x, y, z, t;
                    (void)mon_hit(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.len, x, y, z, t);
                    hit_index[d] = s; Px[d] = x; Py[d] = y; Pz[d] = z; tt[d] = t;
                }
            }
            if (lane == 0) seen[wave][m] = earlier + all;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ------------------------------------------------------------------------------------------
// Spot statistics (ot_monitor_spots_many): the moments of the hit distribution of every CELL (monitor m, plane j) — plane j of
// monitor m is the monitor moved by offsets[j] along its normal, the local x axis — from one pass over the segments on
// k_mon_count's partition and loads.  The hit test is mon_hit's with the local origin's x less offsets[j] (mon_cross).  A hit at
// the local point P has y = P . a_y - c_y, z = P . a_z - c_z (axes[m] = a_y, a_z as in the image mode; centre[m] = c_y, c_z,
// which keeps the variance of a spot far from the monitor's centre from cancelling) and the weight w = intensity[s], read once
// per slot at its first hit (intensity NULL: 1).  A cell accumulates MON_SPOT_VALUES doubles: the count (an integer below 2^31,
// exact in a double), W = sum w, Wy, Wz, Wyy, Wzz, Wyz.  All arithmetic is double.
// NO FLOATING-POINT ATOMIC, and a fixed order of every sum: a wave reduces the seven values of a cell over its lanes by a butterfly
// (wave_sum) — only where __ballot(hit) is not zero: in slot layout a wave holds one segment index of 64 rays and misses most
// cells — and lanes 0..6 add the totals to the wave's OWN row of the cell in LDS, visit after visit in the order of the span; at
// the end of the span the workgroup adds its four rows in wave order and writes partials[workgroup][cell][7]; the workgroup that
// draws the last ticket (one atomic add on an int zeroed before the launch; nobody waits) sums the rows in ascending workgroup
// order and adds the result to the outputs (accumulate) or stores it.  The result depends on (inputs, layout, grid) alone.
// The hand-over of the partials is write-through stores (agent-scope relaxed atomic stores: no release fence, so no workgroup
// writes the L2 back), every wave's wait for them, a barrier, and the ticket by one lane; the last workgroup takes ONE agent-scope
// acquire before a barrier and reads them with plain loads.
// LDS: MON_WAVES rows of 7 doubles a cell, 224 bytes; MON_SPOT_CELLS cells of one launch, 56 KB of the 64 KB a launch gets
// without a function attribute.  Longer cell lists: one launch per MON_SPOT_CELLS cells of the list [m][j].
// A launch of few cells gets MON_SPOT_LDS_MIN bytes all the same (four workgroups a CU still fit): the last workgroup reads the
// partials through them, MON_SPOT_TILE_MIN rows at a time or more.
static constexpr int MON_SPOT_CELLS = 256, MON_SPOT_VALUES = 7, MON_SPOT_LDS_MIN = 32768, MON_SPOT_TILE_MIN = 32;
struct MonSpots {
    const double* axes;        // [n_monitors][6]
    const double* centre;      // [n_monitors][2]
    const double* offsets;     // [n_off]
    const uint8_t* intensity;  // addressed like the fields of MonSource; NULL: weight 1
    double* partials;          // [gridDim.x][n_cells][values]
    unsigned int* ticket;      // 0 before the launch
    long long* counts;         // [n_monitors][n_off]; the wavefront mode: [n_monitors][2]
    double* sums;              // [n_monitors][n_off][6]; the wavefront mode: [n_monitors][61]
    int32_t n_off, cell0, n_cells, accumulate;  // the launch's cells: cell0 .. cell0 + n_cells of the list [m][j]
    int32_t lds_doubles;                        // the launch's dynamic LDS, at least MON_WAVES * n_cells * values doubles
    // the wavefront mode (below): values = MON_WAVEFRONT_VALUES, a cell is a monitor (n_off = 1; centre and offsets are not read)
    int32_t values;                      // MON_SPOT_VALUES or MON_WAVEFRONT_VALUES doubles a cell
    int32_t kind, coordinates;           // reference_kind and coordinates of ot_monitor_wavefront_many
    const double *reference, *pupil, *piston;  // [n_monitors][3] F_loc or u_loc, [n_monitors][3] (c_y, c_z, R), [n_monitors]
    const uint8_t *n_index, *pathlength;  // double, addressed like the fields of MonSource
    // the group mode (below): n_groups > 0, a cell is (monitor, plane, group) and counts / sums are [n_monitors][n_off][n_groups] (x 6)
    const int32_t* groups;               // [n_group_ids], one id per input ray
    int32_t n_group_ids, n_groups;       // n_groups = 0: the two other modes
    // the wavefront mode's group mode: values = MON_WAVEFRONT_VALUES and n_groups > 0, a cell is (monitor, group); counts / sums are
    // [n_monitors][n_groups][2] / [61], and reference, pupil and piston [n_monitors][n_groups][3], [..][3], [n_monitors][n_groups]
};
// Entry k of a host table of the call (axes, centre, offsets: uploaded before the launch, written by no kernel), read through the constant
// address space: a scalar load whatever else the kernel holds.  Without it the compiler proves "nothing in this kernel writes
// here" by a bounded search, and with the group mode in the kernel that search gave up: the spot statistics' inner loop read its
// offset, centre and axes through vector loads and took 3 to 4 % longer.
__device__ __forceinline__ double mon_table(const double* table, int32_t k) {
    typedef const __attribute__((address_space(4))) double* ConstPtr;
    return ((ConstPtr)(uintptr_t)table)[k];
}
template <class V> __device__ __forceinline__ V wave_sum(V v) {  // every lane gets the sum, formed in one order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// The wavefront mode of k_mon_spots (ot_monitor_wavefront_many): the same partition, loads, rows, partials, ticket and last
// workgroup, with a cell of MON_WAVEFRONT_VALUES = 63 doubles per monitor — the hits inside the pupil, the hits outside, and the
// 61 sums S[a, b] (a + b <= 8), T[a, b] (a + b <= 4), Q of the header, in its order.  A hit (mon_hit, unchanged) of slot s:
//   L = t n[s] + pathlength[s] (as k_mon_field),  W = L + n ((F_loc - P) . d) (kind 0)  or  L - n (P . u_loc) (kind 1),
//   (p, q) = ((u - c_y) / R, (v - c_z) / R) with (u, v) = (P . a_y, P . a_z) (coordinates 1) or (g.d . a_y, g.d . a_z) as
//   k_mon_wave forms ty, tz (0);  inside: p^2 + q^2 <= 1 and W finite;  W' = W - piston.
// n, pathlength and intensity of a slot are read once, at its first hit.  A lane that is not inside carries w = W' = p = q = 0 into
// the butterflies (a zero weight alone would leave NaN 0 = NaN in the sums).  The powers p^0..p^8, q^0..q^8 are two register tables
// indexed by the constants of a fully unrolled body; term (a, b) is (w p^a) q^b, ((w W') p^a) q^b, (w W') W'.  Every total goes
// through wave_sum, lane 2 + i keeps total i, and lanes 0..62 add their value to the wave's row: the order of every sum is that of
// the spot statistics.  Where no lane of the wave is inside the pupil the 61 butterflies are skipped (their totals are zero).
// LDS: MON_WAVES rows of 63 doubles a monitor, 2,016 bytes; MON_WAVEFRONT_CELLS = 28 monitors a launch — 56,448 bytes, and
// 28 x 63 = 1,764 values, within the 7 x MON_THREADS the last workgroup's threads own.
static constexpr int MON_WAVEFRONT_CELLS = 28, MON_WAVEFRONT_VALUES = 63, MON_WAVEFRONT_SUMS = 61;
static_assert(MON_WAVEFRONT_CELLS * MON_WAVEFRONT_VALUES <= MON_SPOT_CELLS * MON_SPOT_VALUES, "a launch's values: seven a thread of the last workgroup");
// What the wavefront mode and its group mode (below) do alike, as the one source of both: a hit's W, (p, q), inside and W', and
// the 61 butterflies.  Const: the tables' entries come through mon_table (the group mode, whose cell changes inside a loop over
// lanes), or through the pointers as they are.
template <bool Const> __device__ __forceinline__ double mon_entry(const double* table, int32_t k) {
    if constexpr (Const) return mon_table(table, k);
    else return table[k];
}
// a, f, c, piston: the axes of the monitor and the reference, pupil and piston of the cell.  Returns inside; wi, Wp, p, q are set only then.
template <bool Const> __device__ __forceinline__ bool mon_wavefront_hit(const MonSpots& sp, const MonSeg& g, const MonLocal& l, const double* a,
                                                                        const double* f, const double* c, const double* piston, double Px, double Py,
                                                                        double Pz, double t, double n_index, double pl, double w, double& wi,
                                                                        double& Wp, double& p, double& q) {
    const double L = t * n_index + pl;
    const double Wv = sp.kind == 0 ? L + n_index * ((mon_entry<Const>(f, 0) - Px) * l.dx + (mon_entry<Const>(f, 1) - Py) * l.dy + (mon_entry<Const>(f, 2) - Pz) * l.dz)
                                   : L - n_index * (Px * mon_entry<Const>(f, 0) + Py * mon_entry<Const>(f, 1) + Pz * mon_entry<Const>(f, 2));
    const double u = sp.coordinates ? Px * mon_entry<Const>(a, 0) + Py * mon_entry<Const>(a, 1) + Pz * mon_entry<Const>(a, 2)
                                    : g.dx * mon_entry<Const>(a, 0) + g.dy * mon_entry<Const>(a, 1) + g.dz * mon_entry<Const>(a, 2);
    const double v = sp.coordinates ? Px * mon_entry<Const>(a, 3) + Py * mon_entry<Const>(a, 4) + Pz * mon_entry<Const>(a, 5)
                                    : g.dx * mon_entry<Const>(a, 3) + g.dy * mon_entry<Const>(a, 4) + g.dz * mon_entry<Const>(a, 5);
    const double pp = (u - mon_entry<Const>(c, 0)) / mon_entry<Const>(c, 2), qq = (v - mon_entry<Const>(c, 1)) / mon_entry<Const>(c, 2);
    const bool inside = pp * pp + qq * qq <= 1.0 && fabs(Wv) < HUGE_VAL;  // (a NaN fails both)
    if (inside) wi = w, Wp = Wv - mon_entry<Const>(piston, 0), p = pp, q = qq;
    return inside;
}
// the 61 totals of a wave's (wi, Wp, p, q) into v: lane 2 + i keeps total i
__device__ __forceinline__ void mon_wavefront_sums(double wi, double Wp, double p, double q, int lane, double& v) {
    double pa[9], qa[9];
    pa[0] = qa[0] = 1.0;
#pragma unroll
    for (int e = 1; e <= 8; ++e) pa[e] = pa[e - 1] * p, qa[e] = qa[e - 1] * q;
    const double wW = wi * Wp;
#pragma unroll
    for (int a = 0; a <= 8; ++a) {  // (by a, so that one w p^a is alive at a time; the place of (a, b) is the header's)
        const double wa = wi * pa[a];
#pragma unroll
        for (int b = 0; a + b <= 8; ++b) {
            const double total = wave_sum(wa * qa[b]);
            if (lane == 2 + (a + b) * (a + b + 1) / 2 + b) v = total;
            asm volatile("" : "+v"(v));         // v takes the total here, not in a chain of selects behind 61 live totals,
            __builtin_amdgcn_sched_barrier(0);  // and one butterfly at a time: interleaved, their operands take hundreds of registers
        }
    }
#pragma unroll
    for (int a = 0; a <= 4; ++a) {
        const double wa = wW * pa[a];
#pragma unroll
        for (int b = 0; a + b <= 4; ++b) {
            const double total = wave_sum(wa * qa[b]);
            if (lane == 2 + 45 + (a + b) * (a + b + 1) / 2 + b) v = total;
            asm volatile("" : "+v"(v));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const double total = wave_sum(wW * Wp);
    if (lane == 2 + 45 + 15) v = total;
}
__device__ __forceinline__ void mon_wavefront_visit(const ot_monitor* __restrict__ mons, const MonSource& src, const MonSeg& g, int64_t s,
                                                    const MonSpots& sp, double* mine, int lane) {
    double w = 1.0, n_index = 0.0, pl = 0.0;
    bool have = false;
    for (int32_t k = 0; k < sp.n_cells; ++k) {
        const int32_t m = sp.cell0 + k;  // wave-uniform: monitor, axes, reference, pupil and piston come through scalar loads
        double Px, Py, Pz, t;
        const MonLocal l = mon_local(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz);
        const bool hit = g.valid && mon_cross(mons[m], l, l.ox, g.len, Px, Py, Pz, t);
        if (!__ballot(hit)) continue;
        if (hit && !have) {
            const int64_t at = mon_at(s, src.tile_stride, 8);
            if (sp.intensity) w = *reinterpret_cast<const double*>(sp.intensity + at);
            n_index = *reinterpret_cast<const double*>(sp.n_index + at);
            pl = *reinterpret_cast<const double*>(sp.pathlength + at);
            have = true;
        }
        double wi = 0.0, Wp = 0.0, p = 0.0, q = 0.0;
        bool inside = false;
        if (hit)
            inside = mon_wavefront_hit<false>(sp, g, l, sp.axes + 6 * m, sp.reference + 3 * m, sp.pupil + 3 * m, sp.piston + m, Px, Py, Pz, t, n_index, pl,
                                              w, wi, Wp, p, q);
        const unsigned long long bi = __ballot(inside), bo = __ballot(hit && !inside);
        double v = lane == 0 ? (double)__popcll(bi) : lane == 1 ? (double)__popcll(bo) : 0.0;
        if (bi) mon_wavefront_sums(wi, Wp, p, q, lane, v);
        if (lane < MON_WAVEFRONT_VALUES) mine[k * MON_WAVEFRONT_VALUES + lane] += v;
    }
}
// The group mode of the wavefront mode (ot_monitor_wavefront_groups_many; values = MON_WAVEFRONT_VALUES and n_groups > 0): a cell
// per (monitor m, GROUP g) of the list [m][g], 63 doubles as above, with reference, pupil and piston PER CELL ([m][g][3],
// [m][g][3], [m][g]: every field point has its own image point and pupil centre); axes stay [m][6].  The group of a hit is
// groups[ray[s]] as in mon_groups_visit (below): loaded once per slot at its first hit, nothing read out of range, a ray outside
// [0, n_group_ids) or an id outside [0, n_groups) in no cell and not tallied.
// A launch takes MON_WAVEFRONT_CELLS consecutive cells, cell0 .. cell0 + n_cells, which may begin and end inside a monitor: the
// visit walks the monitors cell0 / G .. (cell0 + n_cells - 1) / G with one hit test each, and where its ballot is not zero the
// DISTINCT groups among the hitting lanes in ascending order of each group's first lane.  Group g0: the cell's tables by scalar
// loads (mon_table), W, (p, q), inside and W' for the lanes with hit && id == g0 (mon_wavefront_hit, the ungrouped source),
// every other lane 0, the two popcounts, the 61 butterflies (mon_wavefront_sums, skipped where no lane is inside), lanes 0..62
// adding to the wave's row of the cell; those lanes cleared.  A group whose cell is outside the launch's window is skipped, its
// lanes cleared all the same.  With one group of id 0 the inputs of every add are the ungrouped visit's, and so is every bit.
__device__ __forceinline__ void mon_wavefront_groups_visit(const ot_monitor* __restrict__ mons, const MonSource& src, const MonSeg& g, int64_t s,
                                                           const MonSpots& sp, double* mine, int lane) {
    double w = 1.0, n_index = 0.0, pl = 0.0;
    int32_t id = -1;
    bool have = false;
    const int32_t m_last = (sp.cell0 + sp.n_cells - 1) / sp.n_groups;
    for (int32_t m = sp.cell0 / sp.n_groups; m <= m_last; ++m) {  // wave-uniform
        double Px, Py, Pz, t;
        const MonLocal l = mon_local(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz);
        const bool hit = g.valid && mon_cross(mons[m], l, l.ox, g.len, Px, Py, Pz, t);
        if (!__ballot(hit)) continue;
        if (hit && !have) {
            const int64_t at = mon_at(s, src.tile_stride, 8);
            if (sp.intensity) w = *reinterpret_cast<const double*>(sp.intensity + at);
            n_index = *reinterpret_cast<const double*>(sp.n_index + at);
            pl = *reinterpret_cast<const double*>(sp.pathlength + at);
            const int32_t ray = *reinterpret_cast<const int32_t*>(src.ray + mon_at(s, src.ray_stride, 4));
            if (ray >= 0 && ray < sp.n_group_ids) id = sp.groups[ray];
            if (id < 0 || id >= sp.n_groups) id = -1;
            have = true;
        }
        const int32_t row0 = m * sp.n_groups - sp.cell0;  // the row of (m, group 0) in the launch's window: may lie before it
        unsigned long long rest = __ballot(hit && id >= 0);
        while (rest) {
            const int32_t g0 = __builtin_amdgcn_readlane(id, __ffsll((long long)rest) - 1);
            const bool in = hit && id == g0;
            rest &= ~__ballot(in);
            const int32_t k = row0 + g0;
            if (k < 0 || k >= sp.n_cells) continue;
            const int32_t cell = sp.cell0 + k;
            double wi = 0.0, Wp = 0.0, p = 0.0, q = 0.0;
            bool inside = false;
            if (in) {
                // the hit point again, from operands the compiler cannot trace to the test above: kept from there, P, t and the
                // local direction stay alive through the 61 butterflies of every group, 22 registers more than the ungrouped visit
                // holds and past four workgroups a CU; formed again they are the same bits
                double o[6] = {g.ox, g.oy, g.oz, g.dx, g.dy, g.dz};
#pragma unroll
                for (int e = 0; e < 6; ++e) asm volatile("" : "+v"(o[e]));
                double Qx, Qy, Qz, tq;
                const MonLocal lq = mon_local(mons[m], o[0], o[1], o[2], o[3], o[4], o[5]);
                (void)mon_cross(mons[m], lq, lq.ox, g.len, Qx, Qy, Qz, tq);
                inside = mon_wavefront_hit<true>(sp, g, lq, sp.axes + 6 * m, sp.reference + 3 * cell, sp.pupil + 3 * cell, sp.piston + cell, Qx, Qy, Qz, tq,
                                                 n_index, pl, w, wi, Wp, p, q);
            }
            const unsigned long long bi = __ballot(inside), bo = __ballot(in && !inside);
            double v = lane == 0 ? (double)__popcll(bi) : lane == 1 ? (double)__popcll(bo) : 0.0;
            if (bi) mon_wavefront_sums(wi, Wp, p, q, lane, v);
            if (lane < MON_WAVEFRONT_VALUES) mine[k * MON_WAVEFRONT_VALUES + lane] += v;
        }
    }
}
// The group mode of k_mon_spots (ot_monitor_spot_groups_many): the spot statistics' partition, loads, hit test, coordinates,
// weight, rows, partials, ticket and last workgroup, with a cell per (monitor m, plane j, GROUP g) of the list [m][j][g] — the
// group of a hit of slot s is groups[ray[s]], the id of the input ray the slot's segment descends from (the ray plane read as
// mon_wavelength reads it), loaded once per slot at its first hit.  A hit whose ray is outside [0, n_group_ids) (nothing is read
// out of range) or whose id is outside [0, n_groups) belongs to no cell and is not tallied: id -1 masks a ray.
// One hit test serves all groups of a pair (m, j).  Where its ballot is not zero the wave walks the DISTINCT groups among its
// hitting lanes: the id g0 of the lowest lane left in the ballot (v_readlane), the lanes with hit && id == g0, the six butterflies
// with every other lane carrying 0, lanes 0..6 adding to the wave's own row of cell (m, j, g0), those lanes cleared — in
// ascending order of each group's first lane, a function of the inputs and their layout alone, so the order of every sum is as
// fixed as the spot statistics'.  A wave of one group (every wave of a group-major batch in slot or tile layout) does one
// butterfly set per pair: with n_groups = 1 the inputs of every add are the spot statistics', and so is every bit of the result.
// A launch takes whole pairs, (MON_SPOT_CELLS / n_groups) * n_groups cells (cell0 and n_cells are multiples of n_groups), so
// the row of (pair k, group g0) is k * n_groups + g0 < n_cells.
__device__ __forceinline__ void mon_groups_visit(const ot_monitor* __restrict__ mons, const MonSource& src, const MonSeg& g, int64_t s,
                                                 const MonSpots& sp, double* mine, int lane) {
    double w = 1.0;
    bool have_w = sp.intensity == nullptr;  // intensity and group of a slot are read once, at its first hit
    int32_t id = -1;
    bool have_id = false;
    const int32_t pair0 = sp.cell0 / sp.n_groups;
    int32_t m = pair0 / sp.n_off, j = pair0 - m * sp.n_off;  // wave-uniform, as in the spot statistics
    for (int32_t k = 0; k < sp.n_cells; ++m, j = 0) {
        const MonLocal l = mon_local(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz);
        const double* a = sp.axes + 6 * m;
        const double cy = mon_table(sp.centre, 2 * m), cz = mon_table(sp.centre, 2 * m + 1);
        for (; j < sp.n_off && k < sp.n_cells; ++j, k += sp.n_groups) {
            double Px, Py, Pz, t;
            const bool hit = g.valid && mon_cross(mons[m], l, l.ox - mon_table(sp.offsets, j), g.len, Px, Py, Pz, t);
            if (!__ballot(hit)) continue;
            if (hit && !have_w) {
                w = mon_real(sp.intensity + mon_at(s, src.tile_stride, src.width), src.width);
                have_w = true;
            }
            if (hit && !have_id) {
                const int32_t ray = *reinterpret_cast<const int32_t*>(src.ray + mon_at(s, src.ray_stride, 4));
                if (ray >= 0 && ray < sp.n_group_ids) id = sp.groups[ray];
                if (id < 0 || id >= sp.n_groups) id = -1;
                have_id = true;
            }
            double W = 0.0, Wy = 0.0, Wz = 0.0, Wyy = 0.0, Wzz = 0.0, Wyz = 0.0;
            if (hit) {
                const double y = Px * mon_table(a, 0) + Py * mon_table(a, 1) + Pz * mon_table(a, 2) - cy,
                             z = Px * mon_table(a, 3) + Py * mon_table(a, 4) + Pz * mon_table(a, 5) - cz;
                W = w, Wy = w * y, Wz = w * z;
                Wyy = Wy * y, Wzz = Wz * z, Wyz = Wy * z;
            }
            unsigned long long rest = __ballot(hit && id >= 0);
            while (rest) {
                const int32_t g0 = __builtin_amdgcn_readlane(id, __ffsll((long long)rest) - 1);
                const bool in = hit && id == g0;
                const unsigned long long b = __ballot(in);
                const double gW = wave_sum(in ? W : 0.0), gWy = wave_sum(in ? Wy : 0.0), gWz = wave_sum(in ? Wz : 0.0),
                             gWyy = wave_sum(in ? Wyy : 0.0), gWzz = wave_sum(in ? Wzz : 0.0), gWyz = wave_sum(in ? Wyz : 0.0);
                const double v = lane == 0 ? (double)__popcll(b) : lane == 1 ? gW : lane == 2 ? gWy : lane == 3 ? gWz : lane == 4 ? gWyy : lane == 5 ? gWzz : gWyz;
                if (lane < MON_SPOT_VALUES) mine[(k + g0) * MON_SPOT_VALUES + lane] += v;
                rest &= ~b;
            }
        }
    }
}
__global__ __launch_bounds__(MON_THREADS) void k_mon_spots(const ot_monitor* __restrict__ mons, MonSource src, int64_t n, int32_t iters,
                                                           const int32_t* __restrict__ seg_count, int64_t n_rays, MonSpots sp) {
    extern __shared__ double spot_rows[];  // [MON_WAVES][n_cells][values]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t nv = sp.n_cells * sp.values;
    double* mine = spot_rows + wave * nv;
    for (int32_t i = lane; i < nv; i += 64) mine[i] = 0.0;
    __syncthreads();
    const MonSpan span = mon_span(n, iters);
    // the wavefront mode walks the span in a loop of its own: one loop for both keeps the scalars of either alive through the
    // other, and the spot statistics' test of every slot against every plane pays for the spills
    const bool wavefront = sp.values == MON_WAVEFRONT_VALUES;  // (uniform for the launch)
    // ... and so do the two group modes (below the spot statistics' loop), for the same reason
    const bool grouped = sp.n_groups > 0;  // (uniform for the launch)
    for (int32_t it = 0; wavefront && !grouped && span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (__ballot(g.valid)) mon_wavefront_visit(mons, src, g, s, sp, mine, lane);
    }
    for (int32_t it = 0; !wavefront && !grouped && span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        double w = 1.0;
        bool have_w = sp.intensity == nullptr;  // the intensity of a slot is read once, at its first hit
        int32_t m = sp.cell0 / sp.n_off, j = sp.cell0 - m * sp.n_off;  // wave-uniform: monitor, axes and offsets come through scalar loads
        for (int32_t k = 0; k < sp.n_cells; ++m, j = 0) {
            const MonLocal l = mon_local(mons[m], g.ox, g.oy, g.oz, g.dx, g.dy, g.dz);
            const double* a = sp.axes + 6 * m;
            const double cy = mon_table(sp.centre, 2 * m), cz = mon_table(sp.centre, 2 * m + 1);
            for (; j < sp.n_off && k < sp.n_cells; ++j, ++k) {
                double Px, Py, Pz, t;
                const bool hit = g.valid && mon_cross(mons[m], l, l.ox - mon_table(sp.offsets, j), g.len, Px, Py, Pz, t);
                const unsigned long long b = __ballot(hit);
                if (!b) continue;
                if (hit && !have_w) {
                    w = mon_real(sp.intensity + mon_at(s, src.tile_stride, src.width), src.width);
                    have_w = true;
                }
                double W = 0.0, Wy = 0.0, Wz = 0.0, Wyy = 0.0, Wzz = 0.0, Wyz = 0.0;
                if (hit) {
                    const double y = Px * mon_table(a, 0) + Py * mon_table(a, 1) + Pz * mon_table(a, 2) - cy,
                                 z = Px * mon_table(a, 3) + Py * mon_table(a, 4) + Pz * mon_table(a, 5) - cz;
                    W = w, Wy = w * y, Wz = w * z;
                    Wyy = Wy * y, Wzz = Wz * z, Wyz = Wy * z;
                }
                W = wave_sum(W), Wy = wave_sum(Wy), Wz = wave_sum(Wz), Wyy = wave_sum(Wyy), Wzz = wave_sum(Wzz), Wyz = wave_sum(Wyz);
                const double v = lane == 0 ? (double)__popcll(b) : lane == 1 ? W : lane == 2 ? Wy : lane == 3 ? Wz : lane == 4 ? Wyy : lane == 5 ? Wzz : Wyz;
                if (lane < MON_SPOT_VALUES) mine[k * MON_SPOT_VALUES + lane] += v;
            }
        }
    }
    for (int32_t it = 0; !wavefront && grouped && span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (__ballot(g.valid)) mon_groups_visit(mons, src, g, s, sp, mine, lane);
    }
    for (int32_t it = 0; wavefront && grouped && span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (__ballot(g.valid)) mon_wavefront_groups_visit(mons, src, g, s, sp, mine, lane);
    }
    __syncthreads();
    double* row = sp.partials + (int64_t)blockIdx.x * nv;
    for (int32_t i = threadIdx.x; i < nv; i += MON_THREADS)  // (write-through stores: no workgroup pays for a write-back of the L2)
        __hip_atomic_store(&row[i], ((spot_rows[i] + spot_rows[nv + i]) + spot_rows[2 * nv + i]) + spot_rows[3 * nv + i], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the rows are read and the partials have arrived: word 0 of the rows now says whether this workgroup is the last
    int32_t* last = reinterpret_cast<int32_t*>(spot_rows);
    if (threadIdx.x == 0) {
        const unsigned int drawn = __hip_atomic_fetch_add(sp.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last = drawn == gridDim.x - 1;
        if (*last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!*last) return;
    // value i of the launch (cell i / 7, sum i % 7) belongs to thread i % MON_THREADS: at most seven a thread.  The rows are added
    // in ascending workgroup order, one add after the other.  Few cells: the workgroups' rows lie back to back, so all threads copy
    // `tile` rows at a time into LDS (every load of a tile in flight at once) and the owner adds them from there; many cells: a
    // thread's own loads of a row are enough in flight, and it adds them straight from memory.
    double sum[MON_SPOT_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int32_t tile = sp.lds_doubles / nv;
    if (tile >= MON_SPOT_TILE_MIN) {
        for (uint32_t g0 = 0; g0 < gridDim.x; g0 += tile) {
            const int32_t rows = (int32_t)min((uint32_t)tile, gridDim.x - g0);
            __syncthreads();  // `last` and the tile before are read
            for (int32_t e = threadIdx.x; e < rows * nv; e += MON_THREADS) spot_rows[e] = sp.partials[(int64_t)g0 * nv + e];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < MON_SPOT_VALUES; ++q) {
                const int32_t i = threadIdx.x + q * MON_THREADS;
                if (i < nv)
                    for (int32_t r = 0; r < rows; ++r) sum[q] += spot_rows[r * nv + i];
            }
        }
    } else {
        for (uint32_t grp = 0; grp < gridDim.x; ++grp) {
#pragma unroll
            for (int q = 0; q < MON_SPOT_VALUES; ++q) {
                const int32_t i = threadIdx.x + q * MON_THREADS;
                if (i < nv) sum[q] += sp.partials[(int64_t)grp * nv + i];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < MON_SPOT_VALUES; ++q) {
        const int32_t i = threadIdx.x + q * MON_THREADS;
        if (i >= nv) continue;
        // a cell's values: its counts (one; inside and outside in the wavefront mode), then its sums
        const int32_t nc = sp.values == MON_SPOT_VALUES ? 1 : 2, ns = sp.values - nc;
        const int64_t cell = sp.cell0 + i / sp.values;
        const int32_t f = i % sp.values;
        if (f < nc) sp.counts[cell * nc + f] = (sp.accumulate ? sp.counts[cell * nc + f] : 0) + (long long)sum[q];
        else sp.sums[cell * ns + f - nc] = sp.accumulate ? sp.sums[cell * ns + f - nc] + sum[q] : sum[q];
    }
}

// ------------------------------------------------------------------------------------------
// Diffraction PSF (ot_monitor_psf_many): U[m][k][l] = sum_j a_j exp(2 pi i (x0_j + gy_j y_k + gz_j z_l)) over the hit list of
// monitor m (k_mon_emit's: ascending slots), as the complex product [ny x hits] . [hits x nz] that the sum separates into:
// exp(2 pi i x_j(k, l)) = (a_j c_j Ey_j[k]) Ez_j[l].  One workgroup per (monitor, pixel tile, hit chunk):
//   pixel tiles: an axis of n samples is ceil(n / 16) SUBTILES of 16, split as evenly as it goes into ceil(subtiles / 4) parts
//     (mon_psf_part: 65 samples = 5 subtiles = 2 + 3, not 4 + 1), so a tile is at most 4 x 4 subtiles = 64 x 64 samples.  Subtile
//     q = (row part) * (columns of the tile) + (column part) of a tile belongs to wave q % 4 as its slot q / 4: four slots a wave,
//     each a 16 x 16 complex accumulator in registers (v_mfma_f64_16x16x4_f64: lane l holds column l & 15, rows (l >> 4) + 4 r).
//   hit chunks: mon_psf_chunks(hits of the monitor) chunks of ceil(hits / chunks) consecutive hits — a function of the hit count
//     alone, at most MON_PSF_MAX_CHUNKS.
// A workgroup walks its chunk in rounds of MON_THREADS hits.  Per round every thread forms one hit's a c = a cis(x0), gy, gz and the
// two rotations cis(gy dy), cis(gz dz) from the hit list and the segment planes (MonPsf: the arguments of k_mon_spots' wavefront
// mode and of k_mon_field, read the same way) into LDS, and tallies it; a hit that is skipped, and the places past the end of the
// chunk, carry a = 0.  Then, MON_PSF_BATCH = 16 hits at a time: every thread builds one RUN of 8 consecutive samples of one axis of
// one hit — one direct mon_wave_cis at the run's first sample, a complex rotation per sample after it (7 roundings of 2^-53: far
// inside the 2^-38 the contract leaves the recurrence) — into the tables tab[A re, A im, B re, B im][sample][hit], A = a c Ey, B = Ez
// (16 hits with 64-sample tiles: more hits a batch and the tables pass the 64 KB a launch gets without a function attribute);
// a barrier; every wave runs its slots over the batch, four hits a step in list order, four real MFMAs a step and slot
// (re += Ar Br, re += (-Ai) Bi, im += Ar Bi, im += Ai Br); a barrier.  No transcendental per pixel and no floating-point atomic.
// The workgroup's accumulators go to partials[workgroup] (write-through stores; in the layout the registers have: the workgroup
// that reads them has the same lanes on the same elements) with, from the tile 0 of a monitor only, norm = sum a and the three
// counts behind them; the hand-over, the ticket and the last workgroup's acquire are k_mon_spots'.  The workgroup that draws the
// last ticket of its (monitor, tile) adds the chunks' partials in ascending chunk order, adds the sum to re, im (and norm, counts:
// tile 0) — the host has zeroed them unless the call accumulates — and leaves the ticket at zero for the launch after it.
// The result is a function of the inputs, their layout and (ny, nz) alone.
// LDS: tables 4 x 64 x 17 doubles (the odd stride keeps the lanes of a wave on different banks, writing and reading), the hits of a
// round 8 x 256 doubles: 51,200 bytes, three workgroups a CU.
static constexpr int MON_PSF_BATCH = 16, MON_PSF_STRIDE = MON_PSF_BATCH + 1, MON_PSF_TILE = 64, MON_PSF_RUN = 8, MON_PSF_MAX_SAMPLES = 512;
static constexpr int MON_PSF_CHUNK_MIN = 512, MON_PSF_MAX_CHUNKS = 256;
static constexpr int MON_PSF_PARTIAL_ROWS = 1024;                            // partials of one launch: workgroups ...
static constexpr int MON_PSF_ROW = 2 * MON_PSF_TILE * MON_PSF_TILE + 8;      // ... of this many doubles each (67 MB in all)
struct MonPsf {
    const int64_t *first, *hit_index;     // first[n_monitors + 1] into the concatenated hit list (k_mon_emit)
    const double *Px, *Py, *Pz, *t;       // the hit list
    const double *axes, *reference, *grid;  // [n_monitors][6], [n_monitors][3] F_loc or u_loc, [n_monitors][4] y0 dy z0 dz
    const uint8_t *intensity, *n_index, *pathlength;  // double, addressed like the fields of MonSource
    MonWavelength lam;                    // (lam.skipped is not used: the tally goes through the partials)
    double* partials;                     // [gridDim.x][MON_PSF_ROW]
    unsigned int* ticket;                 // [pairs of the launch], 0 before it and after it
    double *re, *im, *norm;               // [n_monitors][ny][nz] twice, [n_monitors]
    long long* counts;                    // [n_monitors][3]: used, skipped, aliased
    int32_t kind, amplitude_mode, ny, nz;
    int32_t pair0, max_chunks;            // the launch: (monitor, tile) pairs from pair0 on, max_chunks workgroups each
    int32_t mode;                         // 0: the sum; 1, 2: the count and scatter passes of the partition by group (below)
    const struct MonPsfPartition* pp;     // ... and their arguments, in device memory: the sum's kernel arguments stay what they were
};
// Partition of the hit list by group (ot_monitor_psf_groups_many): a STABLE counting sort of every monitor's hits by the key
// g = groups[ray[hit_index[j]]] (the ray plane read as mon_groups_visit reads it), in two launches with an exclusive_scan between
// them.  A TILE is MON_PSF_PART_TILE consecutive hits of ONE monitor (the host builds `part` from first[]; a monitor without a
// hit has one empty tile), so a workgroup meets at most n_groups keys.  The count pass leaves
// tile_count[base + g * tiles + local]: the entries of cell (m, g) lie together, its tiles in their order, the cells in theirs —
// so the scan over all of them gives every tile's place in every cell, and cell (m, g) starts at tile_off[base + g * tiles].
// The scatter pass walks the same tile in rounds of MON_THREADS hits in list order; a hit goes to seen[g] (the tile's place plus the
// hits of g in its earlier rounds) + the hits of g in the round's lower waves (wcnt, LDS) + those in the wave's lower lanes
// (the ballot-and-match walk of mon_groups_visit, rank_below).  No place depends on the order in which anything lands.
// A hit whose ray is outside [0, n_group_ids) (nothing is read out of range) or whose id is outside [0, n_groups) is in no cell: it
// is not copied, and the count pass tallies it in ungrouped[m] with one integer atomic a wave.
// The first tile of a monitor writes first_cell[m * n_groups + g] for its groups, workgroup 0 first_cell[n_cells].
// LDS: wcnt [MON_WAVES][256] int32 and seen [256] int64 lie in the sum's `tab`.  The passes' arguments (MonPsfPartition) lie in device
// memory behind one pointer of MonPsf: as kernel arguments they cost the sum scalar registers it has no room for.
static constexpr int MON_PSF_PART_TILE = 2048, MON_PSF_GROUPS_MAX = 256;
static_assert(MON_PSF_PART_TILE % MON_THREADS == 0 && MON_PSF_PART_TILE <= 2048, "whole rounds, and a tile's count fits any counter");
struct MonPsfTile {
    int64_t j0, j1, base;           // its hits [j0, j1) of the list; tile_count index of (group 0, tile 0) of its monitor
    int32_t monitor, local, tiles;  // its monitor, its place among that monitor's tiles, how many those are
    int32_t pad;
};
struct MonPsfPartition {
    int32_t n_groups, n_group_ids, n_cells, pad;
    const int32_t* groups;               // [n_group_ids], one id per input ray
    const MonPsfTile* part;              // [gridDim.x]: the tile of every workgroup
    int32_t* tile_count;                 // [n_count + 1], out of the count pass
    const int64_t* tile_off;             // [n_count + 1], its exclusive scan
    int64_t n_count;
    int64_t *first_cell, *to_hit_index;  // out of the scatter pass: [n_cells + 1] and the second hit list
    double *to_Px, *to_Py, *to_Pz, *to_t;
    unsigned long long* ungrouped;       // [monitors]
};
__device__ __forceinline__ void mon_psf_partition(const MonSource& src, const MonPsf& ps, int32_t* wcnt, int64_t* seen, int tid, int lane, int wave) {
    const MonPsfPartition pp = *ps.pp;  // (read once, before any store of the pass)
    const MonPsfTile tl = pp.part[blockIdx.x];
    const int32_t G = pp.n_groups;
    const bool scatter = ps.mode == 2;  // (uniform for the launch)
    for (int32_t g = tid; g < G; g += MON_THREADS) {
        for (int w = 0; w < MON_WAVES; ++w) wcnt[w * MON_PSF_GROUPS_MAX + g] = 0;
        if (scatter) {
            seen[g] = pp.tile_off[tl.base + (int64_t)g * tl.tiles + tl.local];
            if (tl.local == 0) pp.first_cell[(int64_t)tl.monitor * G + g] = pp.tile_off[tl.base + (int64_t)g * tl.tiles];
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (scatter) pp.first_cell[pp.n_cells] = pp.tile_off[pp.n_count];
        else pp.tile_count[pp.n_count] = 0;  // (the scan reads one entry past the counts)
    }
    __syncthreads();
    int32_t none = 0;
    for (int64_t r0 = tl.j0; r0 < tl.j1; r0 += MON_THREADS) {
        const int64_t j = r0 + tid;
        const bool have = j < tl.j1;
        int32_t id = -1;
        if (have) {
            const int32_t ray = *reinterpret_cast<const int32_t*>(src.ray + mon_at(ps.hit_index[j], src.ray_stride, 4));
            if (ray >= 0 && ray < pp.n_group_ids) id = pp.groups[ray];
            if (id < 0 || id >= G) id = -1;
        }
        none += __popcll(__ballot(have && id < 0));
        unsigned long long rest = __ballot(id >= 0);
        int32_t rank = 0;
        while (rest) {  // the distinct groups of the wave, in ascending order of each one's first lane
            const int32_t g0 = __builtin_amdgcn_readlane(id, __ffsll((long long)rest) - 1);
            const bool in = id == g0;
            const unsigned long long b = __ballot(in);
            if (in) rank = rank_below(b);
            if (lane == 0) wcnt[wave * MON_PSF_GROUPS_MAX + g0] += __popcll(b);
            rest &= ~b;
        }
        if (!scatter) continue;  // the count pass keeps adding: wcnt is the wave's count of the whole tile
        __syncthreads();
        if (id >= 0) {
            int64_t d = seen[id] + rank;
            for (int w = 0; w < wave; ++w) d += wcnt[w * MON_PSF_GROUPS_MAX + id];
            pp.to_hit_index[d] = ps.hit_index[j];
            pp.to_Px[d] = ps.Px[j], pp.to_Py[d] = ps.Py[j], pp.to_Pz[d] = ps.Pz[j], pp.to_t[d] = ps.t[j];
        }
        __syncthreads();
        for (int32_t g = tid; g < G; g += MON_THREADS) {
            int32_t sum = 0;
            for (int w = 0; w < MON_WAVES; ++w) sum += wcnt[w * MON_PSF_GROUPS_MAX + g], wcnt[w * MON_PSF_GROUPS_MAX + g] = 0;
            seen[g] += sum;
        }
        __syncthreads();
    }
    if (scatter) return;
    if (lane == 0 && none) atomicAdd(pp.ungrouped + tl.monitor, (unsigned long long)none);
    __syncthreads();
    for (int32_t g = tid; g < G; g += MON_THREADS) {
        int32_t sum = 0;
        for (int w = 0; w < MON_WAVES; ++w) sum += wcnt[w * MON_PSF_GROUPS_MAX + g];
        pp.tile_count[tl.base + (int64_t)g * tl.tiles + tl.local] = sum;
    }
}
// chunks of a monitor with `hits` hits, and part `i` of the `parts` an axis of `subtiles` is split into: [first, first + count)
__host__ __device__ inline int32_t mon_psf_chunks(int64_t hits) {
    const int64_t c = (hits + MON_PSF_CHUNK_MIN - 1) / MON_PSF_CHUNK_MIN;
    return (int32_t)(c < 1 ? 1 : c > MON_PSF_MAX_CHUNKS ? MON_PSF_MAX_CHUNKS : c);
}
__host__ __device__ inline int32_t mon_psf_parts(int32_t samples) { return ((samples + 15) / 16 + 3) / 4; }
__host__ __device__ inline int32_t mon_psf_part(int32_t samples, int32_t i, int32_t& count) {
    const int32_t subtiles = (samples + 15) / 16, parts = mon_psf_parts(samples), first = i * subtiles / parts;
    count = (i + 1) * subtiles / parts - first;
    return first;
}
typedef double mon_psf_acc __attribute__((ext_vector_type(4)));
// the sum (mode 0 of k_mon_psf, which owns the LDS: tab, and par: a c (re, im), gy, gz, cis(gy dy) (re, im), cis(gz dz) (re, im))
__device__ __forceinline__ void mon_psf_sum(const ot_monitor* __restrict__ mons, const MonSource& src, const MonPsf& ps,
                                            double (&tab)[4][MON_PSF_TILE][MON_PSF_STRIDE], double (&par)[8][MON_THREADS]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t parts_z = mon_psf_parts(ps.nz), n_tiles = mon_psf_parts(ps.ny) * parts_z;
    const int32_t pair_local = blockIdx.x / ps.max_chunks, chunk = blockIdx.x % ps.max_chunks;
    const int32_t m = (ps.pair0 + pair_local) / n_tiles, tile = (ps.pair0 + pair_local) % n_tiles;
    const int64_t h0 = ps.first[m], hits = ps.first[m + 1] - h0;
    const int32_t chunks = mon_psf_chunks(hits);
    if (chunk >= chunks) return;
    const int64_t per = (hits + chunks - 1) / chunks;
    const int64_t j0 = h0 + (chunk * per < hits ? chunk * per : hits), j1 = h0 + ((chunk + 1) * per < hits ? (chunk + 1) * per : hits);
    int32_t sub_y, sub_z;  // the tile: sub_y x sub_z subtiles from sample (row0, col0)
    const int32_t row0 = 16 * mon_psf_part(ps.ny, tile / parts_z, sub_y), col0 = 16 * mon_psf_part(ps.nz, tile % parts_z, sub_z);
    const int32_t n_sub = sub_y * sub_z, n_slot = n_sub > wave ? (n_sub - wave + 3) >> 2 : 0;  // this wave's slots
    const double *ax = ps.axes + 6 * m, *ref = ps.reference + 3 * m, *grid = ps.grid + 4 * m;
    const double y0 = grid[0], dy = grid[1], z0 = grid[2], dz = grid[3];
    mon_psf_acc acc_re[4], acc_im[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc_re[q] = acc_im[q] = mon_psf_acc{0.0, 0.0, 0.0, 0.0};
    int32_t used = 0, skipped = 0, aliased = 0;
    double norm = 0.0;
    for (int64_t r0 = j0; r0 < j1; r0 += MON_THREADS) {
        {  // one hit a thread
            const int64_t j = r0 + tid;
            double cr = 0.0, ci = 0.0, gy = 0.0, gz = 0.0, ryr = 1.0, ryi = 0.0, rzr = 1.0, rzi = 0.0;
            if (j < j1) {
                const int64_t s = ps.hit_index[j];
                const double Px = ps.Px[j], Py = ps.Py[j], Pz = ps.Pz[j], t = ps.t[j];
                const int64_t at = mon_at(s, src.tile_stride, 8);
                const double n_index = *reinterpret_cast<const double*>(ps.n_index + at), pl = *reinterpret_cast<const double*>(ps.pathlength + at);
                double wl;
                bool ok = mon_wavelength(ps.lam, src.ray + mon_at(s, src.ray_stride, 4), wl);
                const double L = t * n_index + pl;
                double W;
                if (ps.kind == 0) {  // the renormalised local direction, as mon_hit formed it
                    const MonLocal l = mon_local(mons[m], 0.0, 0.0, 0.0, *reinterpret_cast<const double*>(src.base[3] + at),
                                                 *reinterpret_cast<const double*>(src.base[4] + at), *reinterpret_cast<const double*>(src.base[5] + at));
                    W = L + n_index * ((ref[0] - Px) * l.dx + (ref[1] - Py) * l.dy + (ref[2] - Pz) * l.dz);
                    gy = n_index * (l.dx * ax[0] + l.dy * ax[1] + l.dz * ax[2]);
                    gz = n_index * (l.dx * ax[3] + l.dy * ax[4] + l.dz * ax[5]);
                } else {
                    W = L - n_index * (Px * ref[0] + Py * ref[1] + Pz * ref[2]);
                    gy = -n_index * (Px * ax[0] + Py * ax[1] + Pz * ax[2]);
                    gz = -n_index * (Px * ax[3] + Py * ax[4] + Pz * ax[5]);
                }
                ok = ok && fabs(W) < HUGE_VAL;
                const double x0 = ok ? W / wl : 0.0;
                gy = ok ? gy / wl : 0.0, gz = ok ? gz / wl : 0.0;
                if (!(fabs(gy) < HUGE_VAL && fabs(gz) < HUGE_VAL)) ok = false, gy = gz = 0.0;
                if (ok) {
                    double a = 1.0;
                    if (ps.amplitude_mode != 2) {
                        const double I = *reinterpret_cast<const double*>(ps.intensity + at);
                        a = ps.amplitude_mode == 0 ? sqrt(I) : I;
                    }
                    const double2 c = mon_wave_cis(x0), ry = mon_wave_cis(gy * dy), rz = mon_wave_cis(gz * dz);
                    cr = a * c.x, ci = a * c.y, ryr = ry.x, ryi = ry.y, rzr = rz.x, rzi = rz.y;
                    norm += a;
                    ++used;
                    if (fabs(gy * dy) > 0.5 || fabs(gz * dz) > 0.5) ++aliased;
                } else {
                    ++skipped;
                }
            }
            par[0][tid] = cr, par[1][tid] = ci, par[2][tid] = gy, par[3][tid] = gz;
            par[4][tid] = ryr, par[5][tid] = ryi, par[6][tid] = rzr, par[7][tid] = rzi;
        }
        __syncthreads();
        const int32_t in_round = j1 - r0 < MON_THREADS ? (int32_t)(j1 - r0) : MON_THREADS;
        for (int32_t b0 = 0; b0 < in_round; b0 += MON_PSF_BATCH) {
            {  // one run a thread: waves 0, 1 the rows (A), waves 2, 3 the columns (B)
                const int hb = tid & (MON_PSF_BATCH - 1), run = (tid >> 4) & 7, axis = tid >> 7;
                if (run * MON_PSF_RUN < 16 * (axis ? sub_z : sub_y)) {
                    const int p = b0 + hb;
                    const double g = par[2 + axis][p], rr = par[4 + 2 * axis][p], ri = par[5 + 2 * axis][p];
                    const double k0 = (double)((axis ? col0 : row0) + run * MON_PSF_RUN);
                    const double v = axis ? z0 + k0 * dz : y0 + k0 * dy;
                    const double2 e = mon_wave_cis(g * v);
                    double er = e.x, ei = e.y;
                    if (!axis) {
                        const double cr = par[0][p], ci = par[1][p];
                        er = cr * e.x - ci * e.y, ei = cr * e.y + ci * e.x;
                    }
#pragma unroll
                    for (int i = 0; i < MON_PSF_RUN; ++i) {
                        tab[2 * axis][run * MON_PSF_RUN + i][hb] = er, tab[2 * axis + 1][run * MON_PSF_RUN + i][hb] = ei;
                        const double nr = er * rr - ei * ri, ni = er * ri + ei * rr;
                        er = nr, ei = ni;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < MON_PSF_BATCH / 4; ++ks) {
                const int hit = 4 * ks + (lane >> 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < n_slot) {
                        const int sub = 4 * q + wave, row = 16 * (sub / sub_z) + (lane & 15), col = 16 * (sub % sub_z) + (lane & 15);
                        const double ar = tab[0][row][hit], ai = tab[1][row][hit], br = tab[2][col][hit], bi = tab[3][col][hit];
                        acc_re[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc_re[q], 0, 0, 0);
                        acc_re[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, acc_re[q], 0, 0, 0);
                        acc_im[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, acc_im[q], 0, 0, 0);
                        acc_im[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, acc_im[q], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
    }
    // the partials: element (slot q, re / im, register r) of lane `lane` of wave `wave` at ((sub * 2 + re / im) * 4 + r) * 64 + lane
    double* mine = ps.partials + (int64_t)blockIdx.x * MON_PSF_ROW;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < n_slot) {
            double* at = mine + (int64_t)(4 * q + wave) * 512 + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                __hip_atomic_store(at + 64 * r, acc_re[q][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(at + 256 + 64 * r, acc_im[q][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (tile == 0) {  // (uniform for the workgroup) the tallies: a butterfly per wave, the waves in their order
        const double v[4] = {wave_sum(norm), (double)wave_sum(used), (double)wave_sum(skipped), (double)wave_sum(aliased)};
        if (lane == 0)
            for (int i = 0; i < 4; ++i) par[i][wave] = v[i];
        __syncthreads();
        if (tid < 4)
            __hip_atomic_store(mine + MON_PSF_ROW - 8 + tid, ((par[tid][0] + par[tid][1]) + par[tid][2]) + par[tid][3], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the partials have arrived: word 0 of `tab` now says whether this workgroup is the last of its (monitor, tile)
    int32_t* last = reinterpret_cast<int32_t*>(&tab[0][0][0]);
    if (tid == 0) {
        const unsigned int drawn = __hip_atomic_fetch_add(ps.ticket + pair_local, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last = drawn == (unsigned int)chunks - 1;
        if (*last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ps.ticket + pair_local, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (!*last) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc_re[q] = acc_im[q] = mon_psf_acc{0.0, 0.0, 0.0, 0.0};
    const double* rows = ps.partials + (int64_t)(blockIdx.x - chunk) * MON_PSF_ROW;  // the chunks of this pair, in their order
    for (int32_t c = 0; c < chunks; ++c) {
        const double* row = rows + (int64_t)c * MON_PSF_ROW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < n_slot) {
                const double* at = row + (int64_t)(4 * q + wave) * 512 + lane;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc_re[q][r] += at[64 * r], acc_im[q][r] += at[256 + 64 * r];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < n_slot) {
            const int sub = 4 * q + wave, col = col0 + 16 * (sub % sub_z) + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + 16 * (sub / sub_z) + (lane >> 4) + 4 * r;
                if (row < ps.ny && col < ps.nz) {
                    const int64_t o = ((int64_t)m * ps.ny + row) * ps.nz + col;
                    ps.re[o] += acc_re[q][r], ps.im[o] += acc_im[q][r];
                }
            }
        }
    }
    if (tile == 0 && tid < 4) {
        double sum = 0.0;
        for (int32_t c = 0; c < chunks; ++c) sum += rows[(int64_t)c * MON_PSF_ROW + MON_PSF_ROW - 8 + tid];
        if (tid == 0) ps.norm[m] += sum;
        else ps.counts[3 * (int64_t)m + tid - 1] += (long long)sum;
    }
}
__global__ __launch_bounds__(MON_THREADS) void k_mon_psf(const ot_monitor* __restrict__ mons, MonSource src, MonPsf ps) {
    __shared__ double tab[4][MON_PSF_TILE][MON_PSF_STRIDE];
    __shared__ double par[8][MON_THREADS];
    if (ps.mode == 0) {  // (uniform for the launch)
        mon_psf_sum(mons, src, ps, tab, par);
        return;
    }
    // the two passes of the partition by group, behind the sum: its code comes out as it did without them.  The sum's LDS serves them.
    const int tid = threadIdx.x;
    int32_t* wcnt = reinterpret_cast<int32_t*>(&tab[0][0][0]);
    mon_psf_partition(src, ps, wcnt, reinterpret_cast<int64_t*>(wcnt + MON_WAVES * MON_PSF_GROUPS_MAX), tid, tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6));
}

// ------------------------------------------------------------------------------------------
// Fluence maps (ot_fluence_map): every segment rasterised into a projected view of the table, nu x nv pixels over the edge
// tables ue[0 .. nu], ve[0 .. nv].  k_mon_count's partition and loads (mon_load: any layout, either precision, widened in
// registers); all arithmetic is double.  A segment is the points o + t dh, t in [0, length], dh = d / |d| (renormalised as
// mon_hit does), in the view's coordinates u = . a_u, v = . a_v, w = . a_w (axes[9]).  Its parameter interval is clipped to
// the box [ue[0], ue[nu]] x [ve[0], ve[nv]] x [w_lo, w_hi]; a coordinate that does not move (dh == 0 exactly) is inside under
// mon_bin's rule, lo <= x <= hi.  The grid lines cut the clipped interval [t_a, t_b] into pieces, one pixel each, and pixel
// (ku, kv) gets one count and intensity * (piece length) for every piece of positive length.
// Every crossing parameter is (e[j] - o) / dh with e[j] from the table, recomputed where it is used; none is derived from a
// step.  That expression is monotone in j, so pixels follow from parameters alone: moving up, the pixel at t is the k with
// t(e[k]) <= t < t(e[k + 1]); moving down, t(e[k]) > t >= t(e[k + 1]) — a piece that starts on a line lies on the side it moves
// to; a coordinate at rest is binned by mon_bin (a segment along a line lies in the upper pixel, the last one closed).  A
// passage through a corner steps both axes and leaves no piece.
// The walk is a counted loop: a trip deposits one piece and steps at least one axis, or is the last — nu + nv + 1 trips at most,
// and no loop of the kernel waits on a floating-point condition (the two searches of seg_first_pixel count their trips too).
// Deposits go to the workgroup's image in LDS (lds_pixels = nu * nv: fluence[lds_pixels] doubles, then tally[lds_pixels] int32:
// the image passes' lds_image_zero / lds_image_flush, a pixel flushed when its count is not zero) or, with lds_pixels = 0,
// straight to global memory.  Counts are integers, exact and the same every run; the fluence is fp64 atomic adds.
// A valid segment with a NaN in origin, direction or length, with |d| == 0, or whose clipped interval is not empty and not
// finite (an unbounded last segment inside an infinite depth range) deposits nothing and is counted in *skipped: one atomic a
// wave.  An empty interval (the segment misses the box) is neither.
static constexpr int SEG_RASTER_MAX_PIXELS = 1 << 24;  // nu * nv
struct SegRaster {
    unsigned long long* counts;  // [nu][nv]
    double* fluence;             // [nu][nv]
    unsigned long long* skipped;
    const double *ue, *ve;       // nu + 1, nv + 1 edges
    const uint8_t* intensity;    // addressed like the fields of MonSource; NULL: weight 1
    double axes[9];              // a_u, a_v, a_w
    double w_lo, w_hi;
    int32_t nu, nv, lds_pixels;
};
// the crossing parameter of edge j
__device__ __forceinline__ double seg_cross(const double* __restrict__ e, int32_t j, double o, double dh) { return (e[j] - o) / dh; }
// One axis of the clip: [t_a, t_b] cut to lo <= o + t dh <= hi.  false: the segment stays outside (dh == 0, o outside).
__device__ __forceinline__ bool seg_clip(double lo, double hi, double o, double dh, double& t_a, double& t_b) {
    if (dh == 0.0) return o >= lo && o <= hi;
    const double t_lo = (lo - o) / dh, t_hi = (hi - o) / dh;
    const double t_in = dh > 0.0 ? t_lo : t_hi, t_out = dh > 0.0 ? t_hi : t_lo;
    t_a = t_in > t_a ? t_in : t_a;
    t_b = t_out < t_b ? t_out : t_b;
    return true;
}
// The pixel along one axis of the piece that starts at t (see above); 0 .. nb - 1 whatever the numbers.  The guess comes from
// the position, the answer from the table's crossing parameters.
__device__ __forceinline__ int32_t seg_first_pixel(const double* __restrict__ e, int32_t nb, double o, double dh, double t) {
    if (dh == 0.0) {
        const int32_t k = mon_bin(e, nb, o);
        return k < 0 ? 0 : k;
    }
    const double g = (o + t * dh - e[0]) * (double)nb / (e[nb] - e[0]);
    int32_t k = g >= 0.0 ? (g < (double)(nb - 1) ? (int32_t)g : nb - 1) : 0;  // (a NaN guess starts at 0)
    if (dh > 0.0) {
        for (int32_t i = 0; i < nb && k > 0 && seg_cross(e, k, o, dh) > t; ++i) --k;
        for (int32_t i = 0; i < nb && k < nb - 1 && !(seg_cross(e, k + 1, o, dh) > t); ++i) ++k;
    } else {
        for (int32_t i = 0; i < nb && k < nb - 1 && seg_cross(e, k + 1, o, dh) > t; ++i) ++k;
        for (int32_t i = 0; i < nb && k > 0 && !(seg_cross(e, k, o, dh) > t); ++i) --k;
    }
    return k;
}
__global__ __launch_bounds__(MON_THREADS) void k_seg_raster(MonSource src, int64_t n, int32_t iters, const int32_t* __restrict__ seg_count,
                                                            int64_t n_rays, SegRaster r) {
    extern __shared__ double seg_image[];  // fluence[lds_pixels], then tally[lds_pixels]
    double* fluence = seg_image;
    lds_image_zero<1>(fluence, r.lds_pixels);
    const int lane = threadIdx.x & 63;
    const MonSpan span = mon_span(n, iters);
    int32_t skipped = 0;  // (wave-wide: a scalar)
    for (int32_t it = 0; span.has(it); ++it) {
        const int64_t s = span.at(it) + threadIdx.x;
        const MonSeg g = mon_load(src, s, n, seg_count, n_rays);
        if (!__ballot(g.valid)) continue;
        const double* a = r.axes;
        const double ou = g.ox * a[0] + g.oy * a[1] + g.oz * a[2], ov = g.ox * a[3] + g.oy * a[4] + g.oz * a[5],
                     ow = g.ox * a[6] + g.oy * a[7] + g.oz * a[8];
        double du = g.dx * a[0] + g.dy * a[1] + g.dz * a[2], dv = g.dx * a[3] + g.dy * a[4] + g.dz * a[5],
               dw = g.dx * a[6] + g.dy * a[7] + g.dz * a[8];
        const double norm = sqrt(du * du + dv * dv + dw * dw);
        const double inv = 1.0 / norm;
        du *= inv; dv *= inv; dw *= inv;
        // (x == x is false for a NaN only; norm > 0 refuses a zero direction and a NaN one)
        const bool numbers = ou == ou && ov == ov && ow == ow && du == du && dv == dv && dw == dw && g.len == g.len && norm > 0.0;
        double t_a = 0.0, t_b = g.len;
        bool inside = g.valid && numbers;
        inside = inside && seg_clip(r.ue[0], r.ue[r.nu], ou, du, t_a, t_b);
        inside = inside && seg_clip(r.ve[0], r.ve[r.nv], ov, dv, t_a, t_b);
        inside = inside && seg_clip(r.w_lo, r.w_hi, ow, dw, t_a, t_b);
        inside = inside && t_a <= t_b;
        const bool endless = inside && !(t_b < HUGE_VAL);
        skipped += (int32_t)__popcll(__ballot((g.valid && !numbers) || endless));
        if (!inside || endless) continue;
        double w = 1.0;
        if (r.intensity) w = mon_real(r.intensity + mon_at(s, src.tile_stride, src.width), src.width);
        int32_t ku = seg_first_pixel(r.ue, r.nu, ou, du, t_a), kv = seg_first_pixel(r.ve, r.nv, ov, dv, t_a);
        const int32_t su = du > 0.0 ? 1 : -1, sv = dv > 0.0 ? 1 : -1;
        double t = t_a;
        for (int32_t trip = 0; trip <= r.nu + r.nv; ++trip) {
            const bool in_grid = ku >= 0 && ku < r.nu && kv >= 0 && kv < r.nv;
            if (!in_grid) break;  // (stepped off the grid: t has reached the box's wall)
            const double t_u = du == 0.0 ? HUGE_VAL : seg_cross(r.ue, du > 0.0 ? ku + 1 : ku, ou, du);
            const double t_v = dv == 0.0 ? HUGE_VAL : seg_cross(r.ve, dv > 0.0 ? kv + 1 : kv, ov, dv);
            double t_next = t_u < t_v ? t_u : t_v;
            t_next = t_next < t_b ? t_next : t_b;
            if (t_next > t) {
                const int32_t pixel = ku * r.nv + kv;
                lds_image_deposit<1>(fluence, r.lds_pixels, r.counts, r.fluence, nullptr, pixel, w * (t_next - t));
                t = t_next;
            }
            if (!(t_next < t_b)) break;
            if (t_u <= t_next) ku += su;
            if (t_v <= t_next) kv += sv;
        }
    }
    if (lane == 0 && skipped) atomicAdd(r.skipped, (unsigned long long)skipped);
    lds_image_flush<1, false>(fluence, r.lds_pixels, r.counts, r.fluence);
}
