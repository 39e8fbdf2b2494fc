/*
 * optable_hip.h — C-ABI of liboptable_hip.so, the MI355X (gfx950) trace engine that
 * sits behind optable's OpticalTable.ray_tracing().
 *
 * The reference (tim4431/optable) is pure Python and has no FFI of its own; the boundary
 * this library replaces is the body of
 *     OpticalTable.ray_tracing / _single_ray_tracing      optable/optical_table.py:57-147
 * and everything that loop calls per (segment, surface):
 *     OpticalComponent.interact / intersect_point_local   optable/optical_component.py:151-233,337-378
 *     ComponentGroup.interact (AABB prune + first-min)    optable/component_group.py:93-122
 *     solve_ray_bboxes_intersections                      optable/solver.py:5-48
 *     BaseMirror / BaseRefraciveSurface / Lens .interact_local
 *                                                         optable/optical_component.py:536-570,617-717,930-948
 *     Surface.f / normal / within_boundary                optable/surfaces.py
 *     GaussianBeam.q_at_z, Ray.pathlength, Sellmeier n    optable/ray.py:17-19,145-147; material.py:106-120
 *     Monitor.record                                      optable/monitor.py:183-193
 *
 * Conventions
 *   - plain C, no torch types; every pointer in ot_rays / ot_segments is a DEVICE pointer
 *     (hipMalloc'd or a torch tensor's data_ptr()), every pointer in the scene structs is HOST.
 *   - every entry point returns 0 on success or a negative ot_status; the message for the last
 *     failure on the calling thread is ot_last_error().
 *   - the caller owns all ray / segment buffers; the library owns the uploaded scene and its
 *     scratch.  Calls on one ot_ctx are serialised on the ctx's hipStream_t.
 *   - there is NO CPU fallback in this library.
 */
#ifndef OPTABLE_HIP_H
#define OPTABLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OT_ABI_VERSION 14  /* 14: OT_SHAPE_IMPLICIT_CHEB and its record; 13: OT_OPT_TREES_GLOBAL_IMAGE, tree kernels for scenes beyond the LDS; 12: OT_OPT_GEN_PARENT_INDEX; 11: OT_OPT_GEN_AHEAD, ot_trace_trees_*, ot_trace_trees_append_*, OT_OPT_TREES_LDS_ENTRIES, OT_OPT_TREES_REFILL_AT, OT_OPT_TREES_FLAT; 10: ot_trace_plan, ot_probe_layouts, ot_runtime_info, OT_OPT_REFILL, OT_OPT_REFILL_TICKET, OT_OPT_POOL_JITTER, OT_OPT_GEN_ONEPASS; 9: ot_trace_tree_*, OT_OPT_BLOCK_POOL, OT_OPT_GEN_DROP_DOOMED, ot_trace_append_* holes per workgroup chunk; 8: OT_SHAPE_ASPHERE_CHEB, OT_MAT_CHEB, OT_NODE_BOX_TRUSTED, ot_trace_tiled_*, ot_bench_stream_tiled_*; 3: ot_trace_generation_f32; 4: ot_bench_stream_f32; 5: OT_OPT_LIST_CAP, ray flags bits 8..31, ot_debug_generation_mismatches; 6: ot_debug_last_launch, OT_OPT_FLAT_QUEUE, OT_OPT_LDS_RECORDS; 7: ot_trace_append_*, ot_segment_block, OT_OPT_APPEND_CHUNK, OT_OPT_INSTANCING */

/* ---- status codes ------------------------------------------------------------------- */
enum ot_status {
    OT_OK = 0,
    OT_ERR_INVALID = -1,      /* bad argument / shape mismatch                            */
    OT_ERR_HIP = -2,          /* a HIP runtime call failed (message has hipGetErrorString) */
    OT_ERR_UNSUPPORTED = -3,  /* scene needs a feature this build does not have           */
    OT_ERR_CAPACITY = -4,     /* an output buffer was too small (branching trace)         */
    OT_ERR_NOSCENE = -5       /* trace called before ot_scene_upload                      */
};

/* ---- scene description (host PODs, copied by ot_scene_upload) ------------------------- */

/* node kinds: the scene is the depth-first flattening of OpticalTable.components
 * (optical_table.py:119-123 iterates top-level components in list order; a ComponentGroup
 * iterates its children in list order, component_group.py:110-120).  With a strict '<'
 * nearest-hit update in that order the first minimum wins at every level, exactly as
 * np.argmin + the strict '<' at optical_table.py:121 do. */
enum ot_node_kind { OT_NODE_GROUP = 0, OT_NODE_LEAF = 1 };

/* surface shapes in the leaf's local frame, normal along +x (optical_component.py:43-47) */
enum ot_shape_kind {
    OT_SHAPE_CIRCLE = 0,     /* surfaces.py:139-161   p[0]=radius                                   */
    OT_SHAPE_RECT = 1,       /* surfaces.py:164-209   p[0]=width/2 p[1]=height/2                    */
    OT_SHAPE_POLYGON2D = 2,  /* surfaces.py:426-568, planar=True: aux -> polygon record             */
    OT_SHAPE_POLYGON3D = 3,  /* same, planar=False (plane not x=0): general root solve              */
    OT_SHAPE_SPHERE = 4,     /* surfaces.py:284-336   p[0]=R p[1]=height                            */
    OT_SHAPE_ASPHERE_PARAM = 5, /* component_group.py:1092-1097 p[0]=aperture radius p[1]=R p[2]=kappa p[3]=a4 p[4]=a6 p[5]=a8 */
    OT_SHAPE_ASPHERE_EXACT = 6, /* component_group.py:1061-1064 p[0]=aperture radius p[1]=EFL p[2]=n */
    OT_SHAPE_CYLINDER = 7,   /* surfaces.py:212-281   p[0]=R p[1]=height/2 p[2]=theta0 p[3]=theta1  */
    OT_SHAPE_POINT = 8,      /* surfaces.py:68-86     never hit                                     */
    OT_SHAPE_CSG = 9,        /* Plane.union/subtract  surfaces.py:100-136: aux -> postfix program   */
    OT_SHAPE_ASPHERE_CHEB = 10, /* ASphere with an arbitrary sag F(r) (component_group.py:1014-1055), given as a verified
                                Chebyshev series: p[0]=aperture radius, aux -> [N, lo, hi, c[N], c'[N], c''[N]]: F, dF/dr and
                                d2F/dr2 as series in t = (2r - lo - hi) / (hi - lo); [lo, hi] covers -2h .. radius*sqrt2 + 2h,
                                h = 1e-4 radius (the reference's finite-difference step, surfaces.py:355-369)            */
    OT_SHAPE_IMPLICIT_CHEB = 11 /* a user's implicit surface f(P) = 0 (surfaces.py:5-65), given as a verified tensor Chebyshev
                                series over its local box: aux -> implicit record (below)                                 */
};

/* Implicit record (OT_SHAPE_IMPLICIT_CHEB): a header of OT_IMPLICIT_HEADER reals, then four blocks of nx*ny*nz coefficients —
   f, df/dx, df/dy, df/dz — each indexed [(i * ny + j) * nz + k] for T_i(tx) T_j(ty) T_k(tz), t = (x - centre) * (1 / half width).
   header: [0..2] nx ny nz (terms per axis, 1..64)   [3..5] centre of the box   [6..8] 1 / half widths (formed on the host)
           [9] normal sign s (normal = s grad f / |grad f|)   [10] aperture kind (OT_APERTURE_*)   [11] aperture radius^2
           [12..17] aperture box x0 x1 y0 y1 z0 z1   [18] measured max error of f / max|f|   [19] max|f| over the box */
#define OT_IMPLICIT_HEADER 20
enum ot_implicit_aperture {
    OT_APERTURE_BOX = 0,   /* the (slightly widened) local box                          */
    OT_APERTURE_DISC = 1,  /* (y - cy)^2 + (z - cz)^2 <= R^2, the disc inscribed in the box's yz face */
    OT_APERTURE_RECT = 2,  /* the rectangle of the box's yz face                        */
    OT_APERTURE_BALL = 3   /* |P| <= R (the 3-norm form of Circle, surfaces.py:144-145)  */
};

/* interaction kinds (what interact_local does) */
enum ot_interaction_kind {
    OT_INT_MIRROR = 0,   /* BaseMirror.interact_local            optical_component.py:536-570 */
    OT_INT_REFRACT = 1,  /* BaseRefraciveSurface.interact_local  optical_component.py:617-717 */
    OT_INT_LENS = 2,     /* Lens.interact_local (thin lens)      optical_component.py:930-948 */
    OT_INT_BLOCK = 3     /* Block.interact_local (absorb)        optical_component.py:501-503 */
};

/* radius-of-curvature source for the refractive ABCD update (optical_component.py:633-639) */
enum ot_roc_kind {
    OT_ROC_INF = 0,      /* flat: ROC = +inf                                   */
    OT_ROC_CONST = 1,    /* SphereRefractive: ROC = radius (:847)              */
    OT_ROC_ASPHERE = 2   /* ASphere.roc(P) finite differences (surfaces.py:355-373) */
};

enum ot_node_flags {
    OT_NODE_CHECK_AABB = 1, /* set for groups and for children of groups (component_group.py:98-107) */
    OT_NODE_GRID = 2,       /* group: aux -> 2-D grid over the children's AABBs (acceleration only: the
                               children found through it still pass their own AABB test)             */
    OT_NODE_BOX_TRUSTED = 4 /* the node's aabb contains its geometry.  The reference caches boxes and never updates
                               them (optical_component.py:62-67): a box that went stale is still THE pass / fail gate,
                               but nothing may be skipped because of where it lies.  The kernels prune a node whose
                               box starts behind the best hit only when this flag is set; callers that are not sure
                               leave it clear (results are the same, a little slower).                  */
};

typedef struct ot_node {
    double M[9];       /* leaf: transform_matrix, local->lab rotation, row major          */
    double origin[3];  /* leaf: lab origin                                                */
    double aabb[6];    /* lab AABB (xmin,xmax,ymin,ymax,zmin,zmax) = component.bbox       */
    double lbox[6];    /* leaf, non-planar: surface.get_bbox_local()                      */
    double p[8];       /* shape parameters, see ot_shape_kind                             */
    double reflectivity;
    double transmission;
    double focal_length; /* OT_INT_LENS                                                   */
    double roc;          /* OT_ROC_CONST                                                  */
    int32_t kind;        /* ot_node_kind                                                  */
    int32_t end;         /* index one past the last descendant (leaf: own index + 1)      */
    int32_t flags;       /* ot_node_flags                                                 */
    int32_t shape;       /* ot_shape_kind                                                 */
    int32_t interaction; /* ot_interaction_kind                                           */
    int32_t mat1, mat2;  /* material table indices of _n1 (x>0 side) and _n2 (x<0 side)   */
    int32_t roc_kind;    /* ot_roc_kind                                                   */
    int32_t max_interact_count; /* <0: unlimited (optical_component.py:140-149)           */
    int32_t count_slot;  /* row in the interact-count table, -1 when unlimited            */
    int32_t aux;         /* offset (in doubles) into the aux table, -1 when unused        */
    int32_t leaf_id;     /* index among leaves (what ot_segments.surface reports)         */
} ot_node;

enum ot_material_kind {
    OT_MAT_CONST = 0,
    OT_MAT_SELLMEIER = 1,
    OT_MAT_CHEB = 2      /* n(wavelength in metres) as a verified Chebyshev series of a user function (material.py:4-21):
                            ot_material.n holds the aux offset of [N, lo, hi, c[N]]; wavelengths outside [lo, hi] are clamped
                            to the interval (callers check their rays against it: optable_amd/engine.py)                   */
};

/* material.py:48-85 (RefractiveIndex), :106-120 (Sellmeier, wavelength in metres -> microns) */
typedef struct ot_material {
    double n;        /* OT_MAT_CONST; OT_MAT_CHEB: aux offset  */
    double B[3];     /* OT_MAT_SELLMEIER                    */
    double C[3];     /* microns^2                           */
    int32_t kind;
    int32_t _pad;
} ot_material;

typedef struct ot_scene_desc {
    const ot_node* nodes;
    int32_t n_nodes;
    const ot_material* materials;
    int32_t n_materials;
    const double* aux;     /* polygon records and CSG programs, see DESIGN.md               */
    int32_t n_aux;
    int32_t n_count_slots; /* leaves with max_interact_count set                            */
    int32_t max_children;  /* most rays any interaction can emit (1 => non-branching scene) */
    double unit;           /* metres per model length unit (OpticalTable(unit=...), 1e-2)   */
    int32_t root_grid;     /* aux offset of a 2-D grid over the top-level components (walked
                              cell by cell instead of the linear pass), -1 for none.  Record:
                              [a0 a1 g0 g1 org0 org1 inv0 inv1 margin size0 size1 | start | items] */
    int32_t _pad;
} ot_scene_desc;

/* ---- ray / segment streams (device pointers, structure of arrays) -------------------- */

enum ot_ray_flags {
    OT_RAY_HAS_Q = 1,   /* qo is not None (ray.py:98-104)        */
    OT_RAY_DEAD = 2     /* alive == False on input (optical_component.py:349) */
    /* bits 8..31: zero for a caller's rays.  In the `next` buffers of ot_trace_generation_* they carry
     * (node index + 1) of the surface a ray was emitted on — a ray is never tested against the plane it
     * starts on (the reference rejects that root, t = 0, by |t| < 1e-9) — so a generation's output can be
     * handed back as the next call's input unchanged. */
};

/* One ray = one Ray object of the reference (ray.py:63-104): 12 reals + id + flags.
 * "real" is double for the _f64 entry points and float for _f32. */
typedef struct ot_rays {
    void* ox; void* oy; void* oz;   /* origin                                 */
    void* dx; void* dy; void* dz;   /* unit direction                         */
    void* wavelength;               /* model units (0 when unset)             */
    void* q_re; void* q_im;         /* Gaussian q at origin (ignored w/o HAS_Q) */
    void* intensity;
    void* n;                        /* refractive index of the medium the ray is in, _n(wavelength*unit) */
    void* pathlength;               /* _pathlength                            */
    int32_t* id;                    /* interact-count class of the ray (rays sharing a Python _id share a class) */
    int32_t* flags;                 /* ot_ray_flags                           */
    void* length;                   /* optional: finite input length, +inf = None; NULL = all None */
} ot_rays;

/* One segment = one element of the list OpticalTable.ray_tracing returns
 * (optical_table.py:125-134): the parent truncated at the hit (alive=False, length=t) or the
 * unchanged escaping ray (alive=True, length=None -> +inf here, surface = -1). */
typedef struct ot_segments {
    void* ox; void* oy; void* oz;
    void* dx; void* dy; void* dz;
    void* length;
    void* intensity;
    void* q_re; void* q_im;
    void* n;
    void* pathlength;
    int32_t* ray;       /* index of the input ray whose tree this segment belongs to */
    int32_t* surface;   /* leaf_id that terminated the segment, -1 = escaped        */
} ot_segments;

typedef struct ot_ctx ot_ctx;

/* ---- lifecycle ------------------------------------------------------------------------ */
int ot_abi_version(void);
const char* ot_last_error(void);
/* The HIP runtime this library is bound to: file name of the libamdhip64 that resolves its symbols, and hipRuntimeGetVersion.
 * A process must hold ONE HIP runtime.  The library names libamdhip64.so.7 by soname, so a copy that is already in the process
 * is used (PyTorch ships its own: load it, or `import torch`, BEFORE this library — INTEGRATION.md); loaded first and alone, the
 * library falls back to the ROCm installation's copy.  Never touches the device. */
int ot_runtime_info(char* path, int32_t path_capacity, int32_t* runtime_version);

/* stream: a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL is the device's default (null) stream — which is what torch uses unless told otherwise.
 * Every launch, and the hipEvents of ot_timing_*, go to this stream. */
int ot_ctx_create(int device, void* stream, ot_ctx** out);
int ot_ctx_destroy(ot_ctx* ctx);
int ot_ctx_synchronize(ot_ctx* ctx);
/* Re-target the ctx at another stream of the same device (synchronises the old one first). */
int ot_ctx_set_stream(ot_ctx* ctx, void* stream);

/* Copies the scene (converted to the f32 layout as well) to the device. */
int ot_scene_upload(ot_ctx* ctx, const ot_scene_desc* scene);

/* ---- the hot path ----------------------------------------------------------------------- */

/* Non-branching trace (scene.max_children <= 1): one lane per ray, all segments of a ray in
 * one launch.  Segment k of ray i is written at slot k*n_rays + i of every ot_segments array
 * (capacity max_segments*n_rays); seg_count[i] = number of slots ray i used.  max_segments is
 * the reference's perfomance_limit["max_trace_num"] (optical_table.py:87-97).
 * Scenes in which a hit CAN emit two rays (max_children == 2) may still be traced here
 * speculatively: a ray whose tree actually branches at its k-th segment gets
 * seg_count[i] = -(k+1) (its first k+1 slots are valid, the tree is incomplete) and must be
 * re-traced with ot_trace_generation_f64.
 * counts: int32 [n_count_slots][n_count_classes] interact-count table indexed by rays.id, or
 * NULL when the scene has no limited surface.  A ray whose id lies outside [0, n_count_classes)
 * is not counted (every limited surface stays open to it); nothing is indexed out of range.
 * Precondition for the reference's order (optical_table.py:66-70 finishes one input ray before the
 * next): at most ONE ray per id in a launch — callers with rays that share an id trace them in
 * successive launches over the same table (round r = the r-th ray of every id), as table.py does.
 * If the precondition is broken nothing is corrupted: the gate is an atomic increment-below-cap,
 * a counter never passes its cap; only WHICH of the sharing rays get the remaining counts is then
 * unspecified (ot_trace_generation_*: the trees of one generation all see the table as it stood
 * before the generation, and the table is closed at the cap afterwards). */
int ot_trace_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                 const ot_segments* out, int32_t* seg_count, int32_t* counts,
                 int32_t n_count_classes);
int ot_trace_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                 const ot_segments* out, int32_t* seg_count, int32_t* counts,
                 int32_t n_count_classes);

/* The same trace with the TILED layout: the max_segments * n_rays slots of ot_trace_* in tiles of 64 consecutive slots.
 * Slot s = k * n_rays + i lives in tile s / 64 at lane s % 64; a tile is OT_TILE_BYTES(real) = 64 * (12 * sizeof(real) + 8)
 * bytes: the 12 real fields of ot_segments, 64 values each, then int32 ray[64], int32 surface[64].  A wave of the kernel
 * then writes ONE contiguous 6656-byte (fp32: 3584) block per segment instead of 14 runs in 14 arrays that lie
 * max_segments * n_rays elements apart: the HBM streams of a light scene run 9 % faster (tools/stream_layouts.hip:
 * 5.68 instead of 5.22 TB/s for cfg 2's 1 record in, 5 out).  `tiles` is a device pointer (16-byte aligned) to
 * capacity / 64 tiles; capacity is a multiple of 64 and >= max_segments * n_rays rounded up to 64.  seg_count, counts:
 * as for ot_trace_*.  Light scenes only (the lane-per-ray kernel): a scene that ot_trace_* would send to the rolling
 * lists (24 nodes or more) gets OT_ERR_UNSUPPORTED here — its dense output is ot_trace_append_*. */
#define OT_TILE_BYTES(real_bytes) (64 * (12 * (real_bytes) + 8))
int ot_trace_tiled_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                       int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes);
int ot_trace_tiled_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                       int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes);

/* Uniform fields.  A batch often holds ONE value in every element of a field: one wavelength and one q per beam, the
 * reference's defaults for intensity, n and pathlength, one origin for a point source, one direction for a collimated beam
 * (cfg 2: 72 of the 104 input bytes per ray).  The ot_rays arrays stay full arrays; `uniform_mask` is the caller's word that
 * every element of a field has the bit pattern of element 0, and the lane-per-ray kernel then reads that one element per wave
 * instead of one per ray.  Bit k (OT_UNIFORM_OX .. OT_UNIFORM_PATHLENGTH) stands for the k-th real field in the order of
 * ot_rays; OT_UNIFORM_ID says id[i] == i for every ray; OT_UNIFORM_FLAGS says every flags word equals flags[0].  `length` has
 * no bit.  A bit set for a field that is NOT uniform is the caller's error: every ray is then traced with element 0 of it.
 * uniform_mask = 0 is ot_trace_* / ot_trace_tiled_* exactly (those call these with 0); bits outside OT_UNIFORM_ALL are
 * OT_ERR_INVALID.  Same records either way.  The mask is honoured by the lane-per-ray kernel only: a call that lands on another
 * kernel (heavy scenes) ignores it, as does every call after ot_set_option(OT_OPT_UNIFORM, 0). */
enum ot_uniform_bits {
    OT_UNIFORM_OX = 1 << 0, OT_UNIFORM_OY = 1 << 1, OT_UNIFORM_OZ = 1 << 2,
    OT_UNIFORM_DX = 1 << 3, OT_UNIFORM_DY = 1 << 4, OT_UNIFORM_DZ = 1 << 5,
    OT_UNIFORM_WAVELENGTH = 1 << 6, OT_UNIFORM_Q_RE = 1 << 7, OT_UNIFORM_Q_IM = 1 << 8,
    OT_UNIFORM_INTENSITY = 1 << 9, OT_UNIFORM_N = 1 << 10, OT_UNIFORM_PATHLENGTH = 1 << 11,
    OT_UNIFORM_ID = 1 << 12,     /* id[i] == i                       */
    OT_UNIFORM_FLAGS = 1 << 13,  /* flags[i] == flags[0]             */
    OT_UNIFORM_ALL = (1 << 14) - 1
};
int ot_trace_uniform_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                         const ot_segments* out, int32_t* seg_count, int32_t* counts,
                         int32_t n_count_classes, uint32_t uniform_mask);
int ot_trace_uniform_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                         const ot_segments* out, int32_t* seg_count, int32_t* counts,
                         int32_t n_count_classes, uint32_t uniform_mask);
int ot_trace_tiled_uniform_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                               int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                               uint32_t uniform_mask);
int ot_trace_tiled_uniform_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                               int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                               uint32_t uniform_mask);

/* Resident planes.  A caller that traces into the SAME output again and again (a sustained loop, a stream slot) finds part of
 * every record there already: `ray` is the ray's index whatever the rays do, and in a scene without Snell interfaces every
 * segment of a ray carries the ray's own `n` — and its `intensity`, where every mirror and lens passes all of it or nothing.
 * `resident_mask` is the caller's word that the output holds, for every ray i and every k < |seg_count[i]| AS seg_count STANDS
 * WHEN THE CALL IS MADE (the array being passed in: the counts of the launch that wrote those records), the value this launch
 * would write into that plane of slot k * n_rays + i.  The lane-per-ray kernel then reads the old count with the ray and leaves
 * a flagged plane unwritten for a segment — unless any ray of the wave is past its old count there (a ray that lives longer
 * than last time): then the whole wave writes the full record.  A ray that arrives dead always gets its full record.
 * Same records either way, 4 + 8 + 8 of 104 bytes per record fewer written (fp64) for 4 bytes per ray more read.
 * The library masks the caller's word with what the uploaded scene and the call's uniform_mask keep invariant
 * (ot_trace_resident_plan), so a mask that is wrong for the SCENE skips nothing that changes; a mask that is wrong about the
 * OUTPUT (other n_rays, another layout, other values of n / intensity, records written by something else since, a seg_count
 * that is not the one of the launch that wrote them) is the caller's error: the skipped planes keep what they held.
 * resident_mask = 0 is ot_trace_uniform_* / ot_trace_tiled_uniform_* exactly (those call these with 0); bits outside
 * OT_RESIDENT_ALL are OT_ERR_INVALID.  A call that lands on another kernel (heavy scenes) ignores the mask, as does every call
 * after ot_set_option(OT_OPT_RESIDENT, 0). */
enum ot_resident_bits {
    OT_RESIDENT_RAY = 1 << 0,        /* ray[k * n_rays + i] == i: every scene                                                  */
    OT_RESIDENT_N = 1 << 1,          /* n: needs OT_UNIFORM_N and a scene without Snell interfaces                             */
    OT_RESIDENT_INTENSITY = 1 << 2,  /* intensity: needs OT_UNIFORM_INTENSITY, such a scene, reflectivity / transmission 0 or 1 */
    OT_RESIDENT_ALL = (1 << 3) - 1
};
int ot_trace_resident_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                          const ot_segments* out, int32_t* seg_count, int32_t* counts,
                          int32_t n_count_classes, uint32_t uniform_mask, uint32_t resident_mask);
int ot_trace_resident_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                          const ot_segments* out, int32_t* seg_count, int32_t* counts,
                          int32_t n_count_classes, uint32_t uniform_mask, uint32_t resident_mask);
int ot_trace_tiled_resident_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                                int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                                uint32_t uniform_mask, uint32_t resident_mask);
int ot_trace_tiled_resident_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                                int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                                uint32_t uniform_mask, uint32_t resident_mask);
/* *planes = the OT_RESIDENT_* planes that EVERY record of such a call on the uploaded scene holds one known value in (what a
 * later call into the same output may flag); 0 when the call would not land on the lane-per-ray kernel (or n_rays is 0, or
 * after ot_set_option(OT_OPT_RESIDENT, 0)).  real_bytes: 4 or 8. */
int ot_trace_resident_plan(ot_ctx* ctx, int32_t real_bytes, uint32_t uniform_mask, int64_t n_rays, int32_t max_segments,
                           int32_t* planes);

/* First-segment fields.  Segment 0 of a ray's record is the input ray handed through, whatever the scene does: the lane-per-ray
 * kernel stores there what it loaded.  So where the batch holds ONE bit pattern in a field (uniform_mask), slot 0 * n_rays + i of
 * that plane receives the same pattern on every launch, and a caller that traces batch after batch from the same source into the
 * same output rewrites it for nothing.  `first_mask` uses the OT_UNIFORM_* bit positions of the eleven real fields a record
 * shares with a ray (OT_FIRST_FIELDS: ox .. dz, q_re, q_im, intensity, n, pathlength).  A set bit is the caller's word that, for
 * every ray i with |seg_count[i]| >= 1 AS seg_count STANDS WHEN THE CALL IS MADE, slot 0 * n_rays + i of that plane already holds
 * the bit pattern this launch would write there.  The kernel then leaves the plane unwritten at segment 0 under the rule of the
 * resident planes: for a whole wave or not at all (a wave with a ray whose old count is 0 writes whole records), and a ray that
 * arrives dead always gets its full record.  Segments k >= 1 are not concerned.  Same records either way; cfg 2 (a point source:
 * ox, oy, oz, q_re, q_im, pathlength beside the resident n and intensity) writes 48 bytes per ray fewer.
 * The library masks the caller's word with the call's uniform_mask, so a bit for a field that is not flagged uniform skips nothing;
 * a mask that is wrong about the OUTPUT is the caller's error, as for resident_mask.  Both masks are independent: resident_mask
 * is checked and honoured exactly as by ot_trace_resident_* (which call these with first_mask = 0).  Bits outside OT_FIRST_FIELDS
 * are OT_ERR_INVALID.  The mask is dropped when the call lands on another kernel, when max_segments exceeds 32767, after
 * ot_set_option(OT_OPT_UNIFORM, 0), and unless OT_OPT_RESIDENT is 1. */
enum ot_first_bits {
    OT_FIRST_FIELDS = OT_UNIFORM_OX | OT_UNIFORM_OY | OT_UNIFORM_OZ | OT_UNIFORM_DX | OT_UNIFORM_DY | OT_UNIFORM_DZ | OT_UNIFORM_Q_RE |
                      OT_UNIFORM_Q_IM | OT_UNIFORM_INTENSITY | OT_UNIFORM_N | OT_UNIFORM_PATHLENGTH
};
int ot_trace_reuse_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                       const ot_segments* out, int32_t* seg_count, int32_t* counts,
                       int32_t n_count_classes, uint32_t uniform_mask, uint32_t resident_mask, uint32_t first_mask);
int ot_trace_reuse_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                       const ot_segments* out, int32_t* seg_count, int32_t* counts,
                       int32_t n_count_classes, uint32_t uniform_mask, uint32_t resident_mask, uint32_t first_mask);
int ot_trace_tiled_reuse_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                             int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                             uint32_t uniform_mask, uint32_t resident_mask, uint32_t first_mask);
int ot_trace_tiled_reuse_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                             int64_t capacity, int32_t* seg_count, int32_t* counts, int32_t n_count_classes,
                             uint32_t uniform_mask, uint32_t resident_mask, uint32_t first_mask);
/* ot_trace_resident_plan, and beside it *first_fields = the OT_FIRST_FIELDS bits such a call would honour: the fields of
 * uniform_mask among the eleven; 0 when the call would not land on the lane-per-ray kernel, n_rays is 0, max_segments exceeds
 * 32767, OT_OPT_UNIFORM is 0 or OT_OPT_RESIDENT is not 1. */
int ot_trace_reuse_plan(ot_ctx* ctx, int32_t real_bytes, uint32_t uniform_mask, int64_t n_rays, int32_t max_segments,
                        int32_t* planes, uint32_t* first_fields);

/* The same trace with the APPEND layout: a dense list of segment records instead of max_segments * n_rays slots.
 * The reference returns a list with one entry per processed segment (optical_table.py:125-134); the [k][ray] slots of
 * ot_trace_* hold that list with a hole for every segment a ray did not live to (cfg 3: 11 GB of slots for 2.8 GB of
 * records; cfg 5: 35 GB for 17 GB), and their late planes are written a few elements per cache line.  Here the output is
 * ONE allocation of 14 planes of `capacity` slots each — the 12 real fields in the order of ot_segments, then int32
 * ray[capacity], int32 surface[capacity] — filled in append order: every wave of the kernel claims chunks of slots from
 * a device-wide cursor and writes 64 consecutive records per pass.
 *   - *n_slots (device int64) receives the number of slots claimed.  Slots [0, *n_slots) hold records, except for HOLES,
 *     marked ray = -1: the unused tail of each wave's last chunk (at most OT_OPT_APPEND_CHUNK - 1 slots per wave); with
 *     the block pool (OT_OPT_BLOCK_POOL: curved scenes in single precision) chunks of 16 * OT_OPT_APPEND_CHUNK slots belong
 *     to a workgroup: up to 63 holes at the end of every chunk and the tail of each workgroup's last one.
 *   - order: the records of one ray lie at increasing slot numbers in segment order, so a STABLE sort by `ray` yields the
 *     reference's order (input ray major, then segment order) — the contract of ot_trace_generation_*'s flat list.  The
 *     order of rays among each other is not deterministic.  seg_count[i] is written as by ot_trace_*.
 *   - capacity (a multiple of 64, below 2^30 slots in single and 2^29 in double precision; base 16-byte aligned): if *n_slots > capacity the records that did not fit are lost
 *     (nothing is written outside the block); *n_slots is still exact, so the caller can retry with enough room.
 *     (*n_slots >= 2^62: a wave of the block-pool kernel stopped at one of its internal bounds — a defect, never a capacity matter.)
 *     sum(seg_count) + chunk * (number of waves launched) always suffices (block pool: sum(seg_count) * (1 + 1/128) +
 *     (16 * chunk + 64) * (number of workgroups launched)); ot_debug_last_launch names the launch shape, and
 *     max_segments * n_rays plus that slack never fails.
 * Works for every scene ot_trace_* accepts, always on the heavy-scene kernels (rolling lists or block pool). */
typedef struct ot_segment_block {
    void* base;        /* device pointer: 12 planes of `real`[capacity], then int32 ray[capacity], int32 surface[capacity] */
    int64_t capacity;  /* slots per plane */
} ot_segment_block;
int ot_trace_append_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                        const ot_segment_block* out, int64_t* n_slots, int32_t* seg_count, int32_t* counts,
                        int32_t n_count_classes);
int ot_trace_append_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                        const ot_segment_block* out, int64_t* n_slots, int32_t* seg_count, int32_t* counts,
                        int32_t n_count_classes);

/* Branching trace, one generation of the breadth-first ray tree per call
 * (optical_table.py:115-134).  Input: the generation's alive rays with their tree index
 * (rays_tree) in BFS order.  budget[i] = how many more segments tree i may still process
 * (max_trace_num minus what it already used); rays beyond the budget are dropped as the
 * reference drops them (optical_table.py:138-144).  Output: one segment per processed ray
 * appended at *seg_cursor, and the next generation's rays (stable order: parent order, then
 * child order) in next/next_tree with *n_next.  All counters are device int64/int32 scalars.  A tree that uses up its
 * budget in this call emits no children (OT_OPT_GEN_DROP_DOOMED): the next call would drop them all. */
int ot_trace_generation_f64(ot_ctx* ctx, const ot_rays* rays, const int32_t* rays_tree,
                            int64_t n_rays, int32_t* budget, const ot_segments* out,
                            int64_t out_capacity, int64_t* seg_cursor, const ot_rays* next,
                            int32_t* next_tree, int64_t next_capacity, int64_t* n_next,
                            int32_t* counts, int32_t n_count_classes);
int ot_trace_generation_f32(ot_ctx* ctx, const ot_rays* rays, const int32_t* rays_tree,
                            int64_t n_rays, int32_t* budget, const ot_segments* out,
                            int64_t out_capacity, int64_t* seg_cursor, const ot_rays* next,
                            int32_t* next_tree, int64_t next_capacity, int64_t* n_next,
                            int32_t* counts, int32_t n_count_classes);

/* Whole ray trees in ONE launch, a lane per tree (k_trace_trees): the reference's loop — pop the oldest ray, archive it,
 * push its children, stop after max_trace_num rays (optical_table.py:115-147) — runs per lane with the queue on the chip (its
 * front in LDS, the rest in an L2-resident scratch of the library), and only segment records go to memory.  Output as
 * ot_trace_*: slot k * n_rays + i of `out` (max_trace_num * n_rays slots) is the k-th ray of tree i in the reference's FIFO
 * order, seg_count[i] the rays tree i processed (== max_trace_num: cut short by the cap, or ended exactly there).  A queue of
 * ceil(max_trace_num / 2) rays per lane always suffices; ot_trace_trees_plan says whether the scene has such a kernel
 * (info[0] bit 0: every scene — one whose image and queue fronts fit the CU's LDS through the kernel of its preset, a larger one (thousands
 * of leaves) through the all-features kernel that keeps the node records in LDS, or nothing but the queues, and reads the tables from
 * global memory: dense list only; bit 1: it also writes these [k][tree] slots — scenes
 * of the planar preset; every such kernel writes the dense list of ot_trace_trees_append_*), how many entries its queues get
 * (info[1]), whether that is enough for every tree (info[2]: always, up to caps of ~170 in double precision for a batch that
 * fills the device and of 510 for a few hundred trees — the scratch is per workgroup of the launch) how many of them are in
 * LDS (info[3]), and for ot_trace_trees_append_* the slots a wave claims at a time (info[4]) and the waves of the launch (info[5]):
 * a block of n_rays * max_trace_num + info[4] * info[5] slots holds any trace of the batch.  If not, a tree whose queue overflows reports seg_count[i] = -(rays processed so far) and the
 * caller takes ot_trace_tree_*.  OT_ERR_UNSUPPORTED when info[0] would be 0.  counts / n_count_classes as for ot_trace_*:
 * a tree meets count-limited surfaces in the reference's FIFO order; trees that share a column (rays.id) in one launch get
 * the remaining counts in unspecified order — the caller's rounds, as for ot_trace_*. */
int ot_trace_trees_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_trace_num, const ot_segments* out, int32_t* seg_count,
                       int32_t* counts, int32_t n_count_classes);
int ot_trace_trees_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_trace_num, const ot_segments* out, int32_t* seg_count,
                       int32_t* counts, int32_t n_count_classes);
/* ... into the append layout of ot_trace_append_* (a dense list; *n_slots = slots claimed, records and holes): the records of
 * a step go to consecutive slots whatever trees the lanes are on, so batches whose trees differ widely in size (lanes refill
 * from their wave's share as their trees end) still write whole lines.  A tree's records lie at increasing addresses in FIFO
 * order: a stable sort by `ray` is the reference's order.  seg_count / counts as above. */
int ot_trace_trees_append_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_trace_num, const ot_segment_block* out, int64_t* n_slots,
                              int32_t* seg_count, int32_t* counts, int32_t n_count_classes);
int ot_trace_trees_append_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_trace_num, const ot_segment_block* out, int64_t* n_slots,
                              int32_t* seg_count, int32_t* counts, int32_t n_count_classes);
int ot_trace_trees_plan(ot_ctx* ctx, int32_t real_bytes, int32_t max_trace_num, int64_t n_rays /* 0: a batch that fills the device */,
                        int32_t* info /* int32[8] */);

/* The whole breadth-first trace of a batch of ray trees: the loop over ot_trace_generation_* (optical_table.py:115-147) run
 * by the library — per generation one launch sequence and ONE 16-byte read-back.  `state` is device int64[2] = {segment
 * cursor, rays of the pending generation}: zero it before the first call.  buf_a / buf_b (+ tree_a / tree_b) are two
 * generation buffers of buf_capacity rays each.  result (host int64[5]): [0] segments written so far, [1] rays of the
 * pending generation (0: finished), [2] where they are (0: the caller's `rays`, 1: buf_a, 2: buf_b), [3] generations run by
 * this call, [4] why it stopped: 0 queue empty, 1 the segment arrays cannot take the pending generation, 2 the buffers
 * cannot take its children (max_children x rays), 3 max_seconds (>= 0) ran out.  After 1 or 2 the caller provides more
 * room and calls again with the pending generation as `rays` / `rays_tree` (and the same state and budget).  The arguments
 * are checked once, at entry, as ot_trace_generation_* checks its own, whichever kernels the generations then take. */
int ot_trace_tree_f64(ot_ctx* ctx, const ot_rays* rays, const int32_t* rays_tree, int64_t n_rays, int32_t* budget,
                      const ot_segments* out, int64_t out_capacity, int64_t* state, const ot_rays* buf_a, int32_t* tree_a,
                      const ot_rays* buf_b, int32_t* tree_b, int64_t buf_capacity, int32_t* counts, int32_t n_count_classes,
                      double max_seconds, int64_t* result);
int ot_trace_tree_f32(ot_ctx* ctx, const ot_rays* rays, const int32_t* rays_tree, int64_t n_rays, int32_t* budget,
                      const ot_segments* out, int64_t out_capacity, int64_t* state, const ot_rays* buf_a, int32_t* tree_a,
                      const ot_rays* buf_b, int32_t* tree_b, int64_t buf_capacity, int32_t* counts, int32_t n_count_classes,
                      double max_seconds, int64_t* result);

/* What the library would launch for the uploaded scene and a batch of n_rays rays of `real_bytes` (4 / 8) precision, and
 * which output layout its kernels write fastest — what a caller with no preference should ask for:
 * info[0] kernel family of ot_trace_* (1 lane per ray, 2 rolling lists / block pool); [1] 1 = ot_trace_tiled_* accepts the
 * scene; [2] log2 of the first capacity ot_trace_append_* refuses (30 / 29); [3] the recommended layout: 0 slot arrays
 * (ot_trace_*), 1 tiles (ot_trace_tiled_*), 2 append (ot_trace_append_*); [5], [6] light scenes: hundredths of a microsecond
 * per launch of the stream companion in slot arrays / tiles (ot_probe_layouts).  Heavy scenes: append, unless the worst case
 * max_segments * n_rays would not fit the capacity limit (then slots, which have none).  Light scenes: the layout this DEVICE
 * streams faster — the 64-slot tiles run up to 12 % faster than the 14 arrays on some boxes and 8 % slower on others, so
 * it is measured (once per context and precision, ~15 ms, 1.3 GB of temporary buffers in double precision). */
int ot_trace_plan(ot_ctx* ctx, int32_t real_bytes, int64_t n_rays, int32_t max_segments, int32_t info[8]);
/* The measurement behind it: microseconds per launch of cfg 2's streams (2^20 rays, 5 segments, no tracing) into the 14 slot
 * arrays and into 64-slot tiles; cached in the context. */
int ot_probe_layouts(ot_ctx* ctx, int32_t real_bytes, double* us_slots, double* us_tiled);

/* Diagnostic: how often the two passes of a generation (count, then emit: both run the same trace) disagreed about a
 * ray since the ctx was created.  Expected 0; a disagreement is contained (nothing is written outside the slots the
 * count pass reserved) and shows up as a zero-intensity dead ray in the next generation. */
int ot_debug_generation_mismatches(ot_ctx* ctx, int64_t* count);

/* Diagnostic: the shape of the last ot_trace_* launch on this ctx, for profiles and tuning notes.
 * info[0] kernel (1 lane per ray, 2 rolling lists, 3 refill, 4 lane per tree: [5] / [6] = its queue entries in LDS / in the
 * scratch ring), [1] threads per workgroup, [2] workgroups per CU the occupancy
 * query allowed, [3] workgroups launched, [4] dynamic LDS bytes per workgroup, [5] list capacity per wave (rolling),
 * [6] 1 = mixed generations, [7] bit 0 = candidate pair queue (OT_OPT_FLAT_QUEUE took effect), bit 1 = records in LDS,
 * bit 2 = append layout, bit 3 = tiled layout, bit 4 = workgroup-wide block pool (OT_OPT_BLOCK_POOL; [5] = its slots),
 * bit 5 = rays in registers, refilled in place (OT_OPT_REFILL: reported as kernel 2; [5] = rays per ticket). */
int ot_debug_last_launch(ot_ctx* ctx, int32_t info[8]);

/* Monitor.record (monitor.py:183-193): intersect finished segments with a rectangular
 * monitor plane, honouring segment length.  hit_index receives the slot indices of the segments
 * that hit (ascending), P the local hit point, t the distance; *n_hits the count.
 * seg_count/n_rays: pass ot_trace_*'s seg_count and n_rays to scan a [k][ray] slot array
 * (n_segments = max_segments*n_rays; unused slots are skipped); NULL/0 for a flat list (ot_trace_generation_*);
 * NULL/-1 for a list with holes (ot_trace_append_*: slots whose `ray` is negative are skipped). */
typedef struct ot_monitor {
    double M[9];
    double origin[3];
    double half_width, half_height;
} ot_monitor;
int ot_monitor_record_f64(ot_ctx* ctx, const ot_monitor* mon, const ot_segments* segs,
                          int64_t n_segments, const int32_t* seg_count, int64_t n_rays,
                          int64_t* hit_index, void* Px, void* Py, void* Pz, void* t, int64_t* n_hits);

/* Monitor.record on EVERY monitor of a table (optical_table.py:145-146: `for monitor in self.monitors: monitor.record(rays)`;
 * the test of monitor.py:183-193 as above) in one pass over the segments, read where they lie: no conversion, no per-slot
 * scratch.  Two kernels over one partition of the slots — count the hits per monitor and workgroup, scan, write — for up to 32
 * monitors at a time; longer lists are walked 32 at a time inside the call.
 * The segments: field f of slot s (ox, oy, oz, dx, dy, dz, length) lies at base[f] + (s >> 6) * tile_stride + (s & 63) * width
 * and its int32 `ray` at ray + (s >> 6) * ray_stride + (s & 63) * 4 — plain arrays (ot_segments, the planes of an
 * ot_segment_block): base[f] = the array, tile_stride = 64 * width, ray_stride = 256; a block of 64-slot tiles (ot_trace_tiled_*):
 * base[f] = block + 64 * f * width, ray = block + 64 * 12 * width, both strides the tile size 64 * (12 * width + 8).  width: bytes of
 * a real, 4 or 8 (single precision is widened, exactly; the test is done in double precision either way); capacity: slots the
 * source holds (n_segments may not exceed it).  seg_count / n_rays: as for ot_monitor_record_f64.
 * Output, all on the device: the hits of monitor m are entries first[m] .. first[m + 1] - 1 of hit_index (slot indices,
 * ascending), Px, Py, Pz, t (double), each of `capacity` entries; first has n_monitors + 1 entries, *n_total = first[n_monitors].
 * Like the append layout's cursor, first and *n_total are exact even when they exceed `capacity`: entries beyond it are not
 * written (nothing is written outside the buffers) and the caller repeats the call with room.  n_segments = 0: first all zero.
 * OT_ERR_INVALID, nothing launched: a NULL argument or source field, n_monitors < 1, n_segments < 0 or >= 2^31, a width other
 * than 4 or 8, a seg_count / n_rays combination ot_monitor_record_f64 refuses. */
typedef struct ot_segment_source {
    const void* base[7];
    const void* ray;
    int64_t tile_stride, ray_stride;
    int64_t capacity;
    int32_t width;
} ot_segment_source;
int ot_monitor_record_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const ot_segment_source* src,
                           int64_t n_segments, const int32_t* seg_count, int64_t n_rays, int64_t capacity, int64_t* first,
                           int64_t* hit_index, void* Px, void* Py, void* Pz, void* t, int64_t* n_total);

/* Detector images: the hits of ot_monitor_record_many binned per monitor on the device, with no hit list — a count image and
 * an intensity image of nby x nbz bins for every monitor, from ONE launch of the count kernel per group of monitors (no scan,
 * no second pass, no scratch sized by the hits).  The same segments, the same test; what np.histogram2d(y, z, bins = [y edges,
 * z edges], weights = intensity) gives for the hits' coordinates.
 * Coordinates of a hit at the local point P of monitor m: y = P . a_y, z = P . a_z with axes[m] = a_y, a_z (host, 6 doubles a
 * monitor).  (0,1,0), (0,0,1) is the monitor's own frame; the Python layer passes the monitor's LAB tangents, on which the
 * reference's yList / zList project the local point.
 * Bins are defined by the edge table and nothing else: edges[m] = nby + 1 edges of y, then nbz + 1 edges of z (host), finite and
 * strictly increasing.  Bin k of an axis takes v iff e[k] <= v < e[k + 1], the last bin also v == e[nb]; everything else, NaN
 * included, is dropped (np.histogram's rule, exact for every double: the device steps against the table, it derives no edge).
 * The weight of a hit is `intensity` (device) of its slot, addressed like src->base[f]: intensity + (s >> 6) * tile_stride +
 * (s & 63) * width, in the source's precision.
 * counts, weights: device, [n_monitors][nby][nbz] int64 / double.  accumulate = 0: the call zeroes both first; 1: it adds to
 * what is there (a detector summed over the chunks of a streamed trace).  n_segments = 0 with accumulate = 0: zero images.
 * Counts are integers, exact and the same every run.  The weights are fp64 atomic adds: their last bits depend on the order
 * in which the hits arrive and may differ from run to run.
 * Paths: while the images of a group of monitors fit 64 KB of LDS at 12 bytes a bin (5,450 bins: six monitors of 30 x 30),
 * every workgroup keeps a private image and adds its non-zero bins to global memory at the end; the call walks the monitors in
 * as few, as even groups as that allows (at most 32).  An image that does not fit alone goes to global atomics hit by hit.
 * OT_ERR_INVALID, nothing launched or zeroed: a NULL argument, source field or intensity; n_monitors < 1; nby or nbz < 1 or
 * nby * nbz > 2^24; accumulate other than 0 / 1; a width other than 4 / 8; every n_segments / seg_count / n_rays / capacity
 * combination ot_monitor_record_many refuses; edges not finite and strictly increasing; axes not finite. */
int ot_monitor_image_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges,
                          int32_t nby, int32_t nbz, const ot_segment_source* src, const void* intensity, int64_t n_segments,
                          const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* weights, int32_t accumulate);

/* Coherent detector images: ot_monitor_image_many with a phasor in place of the weight — per monitor a count image and the two
 * parts of a complex field image, re = sum a cos(phi), im = sum a sin(phi) over the hits of a bin, from the same launches of the
 * count kernel (a third mode of it), the same test and the same bin rule; mons, axes, edges, nby, nbz, src, n_segments, seg_count,
 * n_rays and accumulate as there.
 * A hit of slot s at the distance t: L = t * n[s] + pathlength[s] (Ray.pathlength(t)), x = L / wavelength cycles,
 * phi = 2 pi (x - floor x) (Ray.phase(t)), a = sqrt(intensity[s]) for amplitude_mode 0 (intensity is a power) or intensity[s] for 1
 * (scenes whose splitting ratios are amplitudes).  All in double precision; the model's phase and nothing more: no pi on
 * reflection, no Gaussian envelope.
 * intensity, n_index, pathlength: device planes of the segments, addressed like src->base[f].  The wavelength of a hit is
 * wavelength[ray[s]] (device, n_wavelengths doubles: one per input ray, ray[s] through src->ray) or, with wavelength = NULL,
 * wavelength_uniform for every hit.  A hit inside the image whose ray lies outside [0, n_wavelengths), or whose wavelength is not
 * finite and > 0, adds nothing to the images and one to *skipped (device); nothing is read out of range.
 * counts, re, im: device, [n_monitors][nby][nbz] int64 / double / double; skipped: device, one int64.  accumulate = 0 zeroes all
 * four first, 1 adds to what is there.  Counts are integers, exact and the same every run.  re and im are fp64 atomic sums:
 * their last bits depend on the order in which the hits arrive and may differ from run to run.
 * Paths: as for ot_monitor_image_many at 20 bytes of LDS a bin (3,270 bins: three monitors of 30 x 30 a group); an image that
 * does not fit alone goes to global atomics hit by hit.
 * OT_ERR_INVALID, nothing launched or zeroed: everything ot_monitor_image_many refuses; src->width other than 8 (single-precision
 * path lengths carry some 0.02 cycle of phase noise at table scale: refused, not approximated); a NULL n_index, pathlength, counts,
 * re, im or skipped; wavelength = NULL with wavelength_uniform not finite or not > 0; a wavelength array with n_wavelengths < 1;
 * an amplitude_mode other than 0 / 1. */
int ot_monitor_field_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges,
                          int32_t nby, int32_t nbz, const ot_segment_source* src, const void* intensity, const void* n_index,
                          const void* pathlength, const double* wavelength, int64_t n_wavelengths, double wavelength_uniform,
                          int32_t amplitude_mode, int64_t n_segments, const int32_t* seg_count, int64_t n_rays, int64_t* counts,
                          double* re, double* im, int64_t* skipped, int32_t accumulate);

/* Gaussian-beam detector images: ot_monitor_image_many with every hit spread over its Gaussian spot — per monitor a count image
 * and the power every bin receives, from the same launches of the count kernel (a fourth mode of it), the same test and, for the
 * count, the same bin rule; mons, axes, edges, nby, nbz, src, n_segments, seg_count, n_rays and accumulate as there.
 * A hit of slot s at the distance t, at y0 = P . a_y, z0 = P . a_z: q = q_re[s] + t + i q_im[s] (GaussianBeam.q_at_z),
 * w^2 = wavelength (qr^2 + qi^2) / (n[s] pi qi) (Ray.spot_size(t)), and bin (ky, kz) gets intensity[s] Fy(ky) Fz(kz) with
 * Fy(k) = (erf(sqrt2 (ey[k + 1] - y0) / w) - erf(sqrt2 (ey[k] - y0) / w)) / 2 and Fz likewise: the integral over the bin of
 * I 2 / (pi w^2) exp(-2 r^2 / w^2).  The beam is taken at normal incidence in the monitor's (y, z): a tilted beam's spot is not
 * stretched.  Bins whose nearer edge lies more than 5 w from the centre along an axis are left out (a share below 1.5e-23).  All
 * in double precision, whatever the segments' (spot sizes are not phase-sensitive: width 4 is accepted and widened exactly).
 * The centre is counted in counts where ot_monitor_image_many counts the hit; a centre outside the edges is counted nowhere and
 * its tails are still deposited.
 * intensity, q_re, q_im, n_index: device planes of the segments, addressed like src->base[f], in the source's precision.  The
 * wavelength of a hit as for ot_monitor_field_many.  A hit whose ray lies outside [0, n_wavelengths), or whose wavelength, n, qi
 * or w is not finite and > 0 (a ray without q has q = 0), adds nothing anywhere and one to *skipped (device); nothing is read
 * out of range.
 * counts, power: device, [n_monitors][nby][nbz] int64 / double; skipped: device, one int64.  accumulate = 0 zeroes all three first,
 * 1 adds to what is there.  Counts are exact and the same every run; power is fp64 atomic sums, whose last bits depend on the
 * order of arrival.
 * Paths: as for ot_monitor_image_many at 12 bytes of LDS a bin next to 4 KB of per-wave erf tables (5,109 bins: five monitors of
 * 30 x 30 a group); an image that does not fit alone goes to global atomics bin by bin.
 * OT_ERR_INVALID, nothing launched or zeroed: everything ot_monitor_image_many refuses; a NULL q_re, q_im, n_index, counts, power
 * or skipped; wavelength = NULL with wavelength_uniform not finite or not > 0; a wavelength array with n_wavelengths < 1. */
int ot_monitor_beam_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges,
                         int32_t nby, int32_t nbz, const ot_segment_source* src, const void* intensity, const void* q_re,
                         const void* q_im, const void* n_index, const double* wavelength, int64_t n_wavelengths,
                         double wavelength_uniform, int64_t n_segments, const int32_t* seg_count, int64_t n_rays, int64_t* counts,
                         double* power, int64_t* skipped, int32_t accumulate);

/* Coherent Gaussian-beam detector images: the complex field the hits' Gaussian beams make on every monitor, sampled at the bin
 * centres — ot_monitor_field_many with every hit a beam (envelope, wavefront curvature, tilt) instead of a point phasor, from a
 * kernel of its own (k_mon_wave) on the same partition, test and, for the count, bin rule; mons, axes, edges, nby, nbz, src,
 * n_segments, seg_count, n_rays and accumulate as for ot_monitor_image_many.
 * A hit of slot s at the distance t, at y0 = P . a_y, z0 = P . a_z, of the segment direction d (ty = d . a_y, tz = d . a_z):
 *   q = q_re[s] + t + i q_im[s],  |q|^2 = qr^2 + qi^2,  w^2 = wavelength |q|^2 / (n[s] pi qi)        (Ray.spot_size(t))
 *   cycles = (pathlength[s] + t n[s]) / wavelength + n (ty Dy + tz Dz) / wavelength + n qr (Dy^2 + Dz^2) / (2 wavelength |q|^2)
 *   u(yc, zc) = a sqrt(2 / (pi w^2)) exp(-(Dy^2 + Dz^2) / w^2) exp(i (2 pi frac(cycles) - g))
 * at the centre (yc, zc) of a bin, Dy = yc - y0, Dz = zc - z0; a = sqrt(intensity[s]) (amplitude_mode 0) or intensity[s] (1);
 * g = atan2(qr, qi) (gouy = 1) or 0 (gouy = 0) — the tracer's q accumulates no Gouy phase across lenses, so g is exact only for a
 * beam that has met no focusing element since its waist.  The sum of |u|^2 times the bin area over a finely sampled image is a^2.
 * re, im get the sum of u over the hits; counts the hit centres where ot_monitor_image_many counts them.  The envelope is taken at
 * normal incidence (a tilted beam's spot is not stretched), q is not advanced across the tilt, and bin centres more than 6 w from
 * the hit's along an axis are left out (below exp(-36) of the peak).  All in double precision: width 8 only.
 * Sampling: the cycle rate along y is n ty / wavelength + n qr Dy / (wavelength |q|^2), likewise z.  A hit whose largest rate over
 * its footprint (at one of its two end centres) times the mean bin width (last edge - first edge) / bins exceeds 0.5 on either
 * axis is still deposited and adds one to *aliased (device): the image is undersampled there.
 * intensity, n_index, pathlength, q_re, q_im: device planes of the segments, addressed like src->base[f].  The wavelength of a hit
 * as for ot_monitor_field_many.  A hit whose ray lies outside [0, n_wavelengths), or whose wavelength, n, qi or w is not finite and
 * > 0 (a ray without q has q = 0), adds nothing anywhere and one to *skipped (device); nothing is read out of range.
 * counts, re, im: device, [n_monitors][nby][nbz] int64 / double / double; skipped, aliased: device, one int64 each.  accumulate = 0
 * zeroes all five first, 1 adds to what is there (a field is linear: the chunks of a streamed trace add).  Counts are exact and the
 * same every run; re and im are fp64 atomic sums, whose last bits depend on the order of arrival.
 * Paths: as for ot_monitor_image_many at 20 bytes of LDS a bin next to 8 KB of per-wave strips (2,860 bins: three monitors of
 * 30 x 30 a group); an image that does not fit alone goes to global atomics bin by bin.
 * OT_ERR_INVALID, nothing launched or zeroed: everything ot_monitor_image_many refuses; width 4; a NULL n_index, pathlength, q_re,
 * q_im, counts, re, im, skipped or aliased; wavelength = NULL with wavelength_uniform not finite or not > 0; a wavelength array
 * with n_wavelengths < 1; amplitude_mode or gouy outside {0, 1}. */
int ot_monitor_wave_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* edges,
                         int32_t nby, int32_t nbz, const ot_segment_source* src, const void* intensity, const void* n_index,
                         const void* pathlength, const void* q_re, const void* q_im, const double* wavelength, int64_t n_wavelengths,
                         double wavelength_uniform, int32_t amplitude_mode, int32_t gouy, int64_t n_segments, const int32_t* seg_count,
                         int64_t n_rays, int64_t* counts, double* re, double* im, int64_t* skipped, int64_t* aliased,
                         int32_t accumulate);

/* Fluence maps: every segment rasterised into a projected view of the table (what OpticalTable.render(type=..., roi=...) draws
 * line by line, as numbers) — per pixel the number of segment pieces inside it and their intensity-weighted path length.
 * The view: axes = a_u, a_v, a_w (host, 9 doubles); a point x has the image coordinates u = x . a_u, v = x . a_v and the depth
 * w = x . a_w.  The pixels: u_edges (nu + 1) and v_edges (nv + 1), host, finite and strictly increasing; the box of the view is
 * [u_edges[0], u_edges[nu]] x [v_edges[0], v_edges[nv]] x [w_lo, w_hi], where a depth bound may be infinite.
 * A segment is the points o + t dh, t in [0, length], dh = d / |d|.  Its parameter interval is clipped to the box (a coordinate
 * that does not move is inside iff lo <= x <= hi), and the grid lines it crosses cut the rest into pieces, each in one pixel.
 * Every crossing parameter is (edge - o) / dh with the edge read from the table.  A piece lies in the pixel that holds its
 * midpoint: a segment along a grid line in the upper pixel (half-open bins, the last one closed), a piece that starts on a line
 * on the side it moves to; the passage of a corner is a piece of no length.  Pixel (i, j) gets one count and
 * intensity * (t_b - t_a) for every piece of positive length; nothing is counted twice on a line.
 * intensity: device plane of the segments, addressed like src->base[f], in the source's precision; NULL: weight 1 (path length).
 * src, n_segments, seg_count, n_rays as for ot_monitor_record_many.
 * A valid segment with a NaN in origin, direction or length, with |d| = 0, or whose clipped interval is not finite (an unbounded
 * last segment inside an infinite depth range) deposits nothing and adds one to *skipped.
 * counts, fluence: device, [nu][nv] uint64 / double; skipped: device, one uint64.  accumulate = 0 zeroes all three first (also
 * for n_segments = 0), 1 adds to what is there.  Counts are integers, exact and the same every run; the fluence is fp64 atomic
 * adds whose last bits depend on the order of arrival.
 * Paths: an image of up to 5,450 pixels (12 bytes of LDS a pixel) is kept per workgroup and flushed at the end; a larger one
 * takes every piece as a global atomic.  One lane walks one segment: nu + nv + 1 steps at most.
 * OT_ERR_INVALID, nothing launched or zeroed: a NULL argument (intensity apart); nu or nv < 1; nu * nv > 2^24; accumulate other
 * than 0 / 1; everything ot_monitor_record_many refuses of src, n_segments, seg_count and n_rays; edges not finite and strictly
 * increasing; w_lo > w_hi (or a NaN); axes not finite. */
int ot_fluence_map(ot_ctx* ctx, const double* axes, const double* u_edges, int32_t nu, const double* v_edges, int32_t nv,
                   double w_lo, double w_hi, const ot_segment_source* src, const void* intensity, int64_t n_segments,
                   const int32_t* seg_count, int64_t n_rays, unsigned long long* counts, double* fluence,
                   unsigned long long* skipped, int32_t accumulate);

/* Spot statistics and through-focus scans: the zeroth, first and second moments of the hit distribution of every monitor, on the
 * monitor and on a stack of n_offsets virtual planes displaced along its normal, from one pass over the segments with no hit list
 * and no image.  A CELL is a pair (monitor m, plane j): plane j of monitor m is the monitor moved by offsets[j] (host) along its
 * own normal, the local x axis (column 0 of ot_monitor.M).  One list of offsets is shared by all monitors; duplicates are allowed
 * and no order is required.
 * The hit test is ot_monitor_record_many's with one change: once the local origin (ox, oy, oz) of the segment is formed, ox becomes
 * ox - offsets[j].  The renormalised direction, dx == 0, |t| < 1e-9 || t < 0 || t > length and the rectangle test on Py, Pz are
 * unchanged.  offsets[j] = 0 is the monitor itself.
 * Coordinates of a hit at the local point P: y = P . a_y - c_y, z = P . a_z - c_z with axes[m] = a_y, a_z as for
 * ot_monitor_image_many and centre[m] = c_y, c_z (host, 2 doubles a monitor): a centre near the spot keeps the variance of a spot
 * far from the monitor's centre from cancelling in Wyy - Wy^2 / W.  The weight w of a hit is `intensity` (device) of its slot,
 * addressed like src->base[f] in the source's precision; NULL: w = 1.
 * counts: device, [n_monitors][n_offsets] int64, the hits of every cell.  sums: device, [n_monitors][n_offsets][6] double:
 * W = sum w, Wy = sum w y, Wz = sum w z, Wyy = sum w y^2, Wzz = sum w z^2, Wyz = sum w y z.  All arithmetic is double, whatever
 * the segments' precision (width 4 is widened exactly).  accumulate = 0 zeroes both first (also for n_segments = 0), 1 adds to
 * what is there (the chunks of a streamed trace).
 * Determinism: counts are exact, and the sums are BIT-IDENTICAL from run to run — no floating-point atomic takes part.  A wave
 * sums a cell over its lanes by a butterfly, adds to a row of its own, the workgroup adds its waves in order, and the last
 * workgroup to finish adds the workgroups' rows in ascending order: the result depends on the inputs, their layout and the grid
 * (a function of n_segments) alone.
 * Cell groups: a launch takes 256 cells of the list [m][j] (224 bytes of LDS a cell); longer lists are walked in groups inside the
 * call, every group one pass over the segments.
 * src, n_segments, seg_count, n_rays as for ot_monitor_record_many.
 * OT_ERR_INVALID, nothing launched or zeroed: a NULL argument (intensity apart); n_monitors < 1; n_offsets < 1 or
 * n_monitors * n_offsets > 2^20; axes, centre or offsets not finite; accumulate other than 0 / 1; everything
 * ot_monitor_record_many refuses of src, n_segments, seg_count and n_rays. */
int ot_monitor_spots_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* centre,
                          const double* offsets, int32_t n_offsets, const ot_segment_source* src, const void* intensity,
                          int64_t n_segments, const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* sums,
                          int32_t accumulate);

/* Spot statistics per ray group: ot_monitor_spots_many with a GROUP axis on the cells — the moments of every wavelength, field
 * point or port of one batch from one pass over the segments (chromatic focal shift, field curvature, the power of every port).
 * A CELL is a triple (monitor m, plane j, group g).  mons, axes, centre, offsets, src, intensity, n_segments, seg_count, n_rays
 * and accumulate are ot_monitor_spots_many's, and so are the hit test, the coordinates y, z and the weight of a hit: a hit of
 * slot s is exactly that call's hit.  It belongs to group groups[ray[s]], where ray[s] is the int32 `ray` of the slot (src->ray:
 * the index of the input ray the segment descends from, in every layout and for every node of a ray tree) and `groups` is a
 * DEVICE table of n_group_ids int32 ids, one per input ray.
 * A hit belongs to NO cell — it is counted nowhere and no tally of such hits is kept — when its ray index is outside
 * 0 .. n_group_ids - 1 (nothing is read out of range) or its id is outside 0 .. n_groups - 1.  That is how rays are masked: id -1.
 * counts: device, [n_monitors][n_offsets][n_groups] int64.  sums: device, [n_monitors][n_offsets][n_groups][6] double, W, Wy, Wz,
 * Wyy, Wzz, Wyz as for ot_monitor_spots_many.  All arithmetic is double, whatever the segments' precision.  accumulate as there.
 * Determinism: as ot_monitor_spots_many — counts exact, sums bit-identical from run to run, no floating-point atomic.  Per pair
 * (m, j) a wave walks the distinct groups among its hitting lanes, in ascending order of each group's first lane, and sums each
 * over its lanes by a butterfly in which the other lanes carry 0; rows, workgroups and the last workgroup as there.  With
 * n_groups = 1 and every id 0 the result is ot_monitor_spots_many's, bit for bit.
 * Cell groups: the list is [m][j][g] and a launch takes whole pairs (m, j): (256 / n_groups) * n_groups cells, every launch one
 * pass over the segments.
 * OT_ERR_INVALID, nothing launched or zeroed: everything ot_monitor_spots_many refuses; groups NULL; n_groups outside
 * 1 .. OT_SPOT_GROUPS_MAX; n_group_ids < 1 (or >= 2^31); n_monitors * n_offsets * n_groups > 2^20. */
#define OT_SPOT_GROUPS_MAX 256
int ot_monitor_spot_groups_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, const double* centre,
                                const double* offsets, int32_t n_offsets, const int32_t* groups, int64_t n_group_ids,
                                int32_t n_groups, const ot_segment_source* src, const void* intensity, int64_t n_segments,
                                const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* sums, int32_t accumulate);

/* Wavefront error: the hits of every monitor reduced to the moments of their optical path difference over a unit pupil, from one
 * pass over the segments with no hit list — what a least-squares fit of Zernike (or any other) polynomials up to radial order 4
 * and the rms wavefront error need.  One cell per monitor; mons, axes, src, n_segments, seg_count, n_rays and accumulate as for
 * ot_monitor_spots_many, and there are no plane offsets.
 * The hit test is ot_monitor_record_many's, unchanged.  A hit of slot s on monitor m gives the local hit point P, the distance t
 * and the renormalised local direction d.  With n = n_index[s] and L = t n + pathlength[s] (Ray.pathlength(t), as
 * ot_monitor_field_many forms it) the optical path W is taken against an ideal wave: reference_kind is one int for the call,
 * reference[m] three host doubles per monitor.
 *   reference_kind 0, a spherical wave about a focus F: reference[m] = F_loc = M^T (F - origin), the focus in the monitor's frame.
 *     W = L + n ((F_loc - P) . d): the optical path at the foot of the perpendicular from F onto the ray.  A perfect wave that
 *     converges on F, or diverges from it, has one W for every ray.  This is the reference sphere AT INFINITY: against a sphere of
 *     the finite radius R_s about F, W differs by n e^2 / (2 R_s) to leading order, e the ray's miss distance at F — the limit
 *     in which the two agree is e^2 / R_s far below the error of interest.
 *   reference_kind 1, a plane wave along the unit vector u: reference[m] = u_loc = M^T u.  W = L - n (P . u_loc).
 * Pupil coordinates: coordinates is one int for the call, pupil[m] = (c_y, c_z, R), R > 0, host.
 *   coordinates 1, position: (p, q) = ((y - c_y) / R, (z - c_z) / R) with y = P . a_y, z = P . a_z (axes[m] = a_y, a_z, the
 *     images' coordinates).
 *   coordinates 0, direction: (p, q) = ((ty - c_y) / R, (tz - c_z) / R) with ty = D . a_y, tz = D . a_z of the segment's
 *     direction D as it is stored (MonitorHits.tYList / tZList, as ot_monitor_wave_many forms them).
 * A hit is INSIDE the pupil when p^2 + q^2 <= 1 and W, p and q are finite; every other hit is tallied as outside and adds to no
 * sum.  The weight w of a hit is `intensity` (device, double, addressed like src->base[f]) of its slot; NULL: w = 1.
 * With W' = W - piston[m] (host, one double a monitor; near the mean of W it keeps Q from cancelling) monitor m accumulates 61
 * sums, sums[m][0 .. 60], in this order:
 *   S[a, b] = sum w p^a q^b,    a + b <= 8: 45 values, (a, b) at g (g + 1) / 2 + b with g = a + b
 *   T[a, b] = sum w W' p^a q^b, a + b <= 4: 15 values, (a, b) at 45 + g (g + 1) / 2 + b
 *   Q       = sum w W'^2:                     1 value, at 60
 * (a term is (w p^a) q^b, ((w W') p^a) q^b, (w W') W', the powers by repeated multiplication) and counts[m] = (inside, outside),
 * int64.  Both are device arrays; accumulate = 0 zeroes them first (also for n_segments = 0), 1 adds to what is there.  All
 * arithmetic is double, and the segments must be double (src->width 8): a path length in single precision is a hundredth of a wave
 * wrong at table scale.  n_index, pathlength: device, double, addressed like src->base[f].
 * Determinism: as ot_monitor_spots_many — counts exact, sums bit-identical from run to run, no floating-point atomic; the result
 * is a function of the inputs, their layout and the grid alone.
 * Monitor groups: a launch takes OT_WAVEFRONT_MONITORS monitors (4 waves x 63 doubles of LDS each); longer lists are walked in
 * groups inside the call, every group one pass over the segments.
 * OT_ERR_INVALID, nothing launched or zeroed: a NULL argument (intensity apart); n_monitors < 1 or > 2^20; reference_kind or
 * coordinates other than 0 / 1; axes, reference, pupil or piston not finite; R <= 0; u_loc = 0 (reference_kind 1); src->width
 * other than 8; accumulate other than 0 / 1; everything ot_monitor_record_many refuses of src, n_segments, seg_count, n_rays. */
#define OT_WAVEFRONT_MONITORS 28
#define OT_WAVEFRONT_SUMS 61
int ot_monitor_wavefront_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                              const double* reference, int32_t coordinates, const double* pupil, const double* piston,
                              const ot_segment_source* src, const void* intensity, const void* n_index, const void* pathlength,
                              int64_t n_segments, const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* sums,
                              int32_t accumulate);

/* Wavefront error per ray group: ot_monitor_wavefront_many with a GROUP axis on the cells — the 61 sums of every wavelength or
 * field point of one batch from one trace (Zernike coefficients against wavelength and against field).  A CELL is a pair
 * (monitor m, group g) of the list [m][g].  mons, axes, reference_kind, coordinates, src, intensity, n_index, pathlength,
 * n_segments, seg_count, n_rays and accumulate are ot_monitor_wavefront_many's, and so are the hit test, W, (p, q), inside,
 * the weight and the 61 sums of a hit.  The group of a hit of slot s is groups[ray[s]], exactly as for
 * ot_monitor_spot_groups_many: `groups` is a DEVICE table of n_group_ids int32 ids, one per input ray; a hit whose ray index is
 * outside 0 .. n_group_ids - 1 (nothing is read out of range) or whose id is outside 0 .. n_groups - 1 belongs to NO cell and no
 * tally of such hits is kept: id -1 masks a ray.
 * Every field point has its own image point and its own pupil centre, so reference, pupil and piston are PER CELL, host:
 * reference[m * n_groups + g] three doubles (F_loc or u_loc in monitor m's frame), pupil[m * n_groups + g] = (c_y, c_z, R),
 * piston[m * n_groups + g] one double.  axes stay [n_monitors][6].
 * counts: device, [n_monitors][n_groups][2] int64 (inside, outside).  sums: device, [n_monitors][n_groups][61] double, S, T, Q
 * in ot_monitor_wavefront_many's order.
 * Determinism: as ot_monitor_wavefront_many — no floating-point atomic.  Per monitor a wave walks the distinct groups among its
 * hitting lanes in ascending order of each group's first lane and sums each over its lanes by the same 61 butterflies, the other
 * lanes carrying 0.
 *   With n_groups = 1 and every id 0, group 0 of this call equals ot_monitor_wavefront_many with the same reference, pupil and
 *   piston, bit for bit.
 *   Group g of this call equals group 0 of the call with n_groups = 1, the ids (id == g ? 0 : -1) and cell (m, g)'s reference,
 *   pupil and piston for monitor m, bit for bit.
 * Cell groups: a launch takes OT_WAVEFRONT_MONITORS = 28 consecutive cells of [m][g], which may begin and end inside a monitor; a
 * call over C cells is ceil(C / 28) passes over the segments.
 * OT_ERR_INVALID, nothing launched or zeroed: everything ot_monitor_wavefront_many refuses (of reference, pupil and piston: per
 * cell); groups NULL; n_groups outside 1 .. OT_SPOT_GROUPS_MAX; n_group_ids < 1 (or >= 2^31); n_monitors * n_groups >
 * OT_WAVEFRONT_GROUP_CELLS_MAX. */
#define OT_WAVEFRONT_GROUP_CELLS_MAX 4096
int ot_monitor_wavefront_groups_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                                     const double* reference, int32_t coordinates, const double* pupil, const double* piston,
                                     const int32_t* groups, int64_t n_group_ids, int32_t n_groups, const ot_segment_source* src,
                                     const void* intensity, const void* n_index, const void* pathlength, int64_t n_segments,
                                     const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* sums, int32_t accumulate);

/* Diffraction PSF: the plane waves of every monitor's hits summed over a grid of image samples, on the device.
 * ot_monitor_psf_many uses the hit test of ot_monitor_record_many, unchanged.  A hit of slot s on monitor m gives the local point P,
 * the distance t and the renormalised local direction d.  Further: n = n_index[s]; L = t n + pathlength[s]; the wavelength lambda,
 * resolved exactly as ot_monitor_field_many resolves it (wavelength[ray[s]] from the per-ray array, or wavelength_uniform); the
 * amplitude a = sqrt(intensity[s]) (amplitude_mode 0), intensity[s] (1) or 1 (2: intensity is not read and may be NULL).
 * W is exactly ot_monitor_wavefront_many's: reference_kind 0: W = L + n ((F_loc - P) . d); reference_kind 1: W = L - n (P . u_loc);
 * reference[m] holds three host doubles, axes[m] = a_y, a_z as everywhere else.
 * Samples, not bins: grid[m] = (y0, dy, z0, dz), host, dy and dz finite and > 0; ny and nz are shared by the call; sample (k, l)
 * lies at y_k = y0 + k dy, z_l = z0 + l dz.  Meaning of a sample, and phase of hit j there in cycles:
 *   kind 0 (image space about a focus F): the sample is the point F + y_k a_y + z_l a_z, in the plane through F parallel to the
 *     monitor; every ray counts as the plane wave it locally is.  x = (W + n (d . a_y) y_k + n (d . a_z) z_l) / lambda.
 *   kind 1 (angle space about a plane wave u: the far field of an afocal system): the sample is the direction
 *     u + y_k a_y + z_l a_z.  x = (W - n (P . a_y) y_k - n (P . a_z) z_l) / lambda.
 * So x_j(k, l) = x0_j + gy_j y_k + gz_j z_l, and the field is U[m][k][l] = sum_j a_j exp(2 pi i frac(x_j(k, l))) over the usable
 * hits of monitor m.
 * Outputs, all on the device: re, im: [n_monitors][ny][nz] double; norm[m] = sum_j a_j, double; counts[m] = (used, skipped,
 * aliased), int64.  skipped counts the hits whose ray lies outside [0, n_wavelengths), whose lambda is not finite and > 0, or whose
 * W, gy or gz is not finite: these add nothing.  aliased counts the used hits with |gy dy| > 1/2 or |gz dz| > 1/2; they are summed
 * all the same.  accumulate = 0 zeroes everything first, also for n_segments = 0; accumulate = 1 adds this call's result to what
 * is there: the sum is linear, so the chunks of a streamed trace add.  All arithmetic is double, and src->width must be 8.
 * OT_ERR_INVALID, with nothing launched or zeroed: everything ot_monitor_wavefront_many refuses of its shared arguments (ctx, mons,
 * n_monitors, axes, reference_kind, reference, src, n_index, pathlength, n_segments, seg_count, n_rays, accumulate; a NULL
 * output); ny or nz outside 1 .. OT_PSF_MAX_SAMPLES; grid not finite, or a step of 0 or less; an amplitude_mode outside 0 .. 2; a
 * NULL intensity with amplitude_mode 0 or 1; the wavelength errors of ot_monitor_field_many.
 * Determinism: like the spot statistics, re, im and norm are bit-identical from run to run.  No floating-point atomic takes part:
 * the hits of a monitor are taken in the order of its hit list (ascending slots), in chunks whose number is a function of the
 * monitor's hit count alone, and the chunks' partial images are added in ascending order by the workgroup that finishes last.  The
 * result is a function of the inputs, their layout and the launch grid alone.  The counts are exact.
 * Accuracy: the phasor of a sample comes from one direct sincospi per 8 samples of an axis and complex rotations between them, and
 * |U_device - U_exact| <= norm (2 pi E + 2^-38), U_exact the sum above in extended precision from the segments' doubles,
 * E = 16 x 2^-53 x max_j(|L_j| + n_j |F_loc - P_j|) / min_j lambda_j (kind 1: |P_j| in place of |F_loc - P_j|): sixteen roundings
 * of a quantity the size of the path go into W / lambda, and 2^-38 is the budget of the recurrence.
 * Scratch, owned by the context and kept between calls: the hit list (40 bytes a hit, sized exactly: the call counts the hits,
 * reads the n_monitors + 1 totals back — its one synchronisation of the stream — and then writes them) and the partial images of
 * one launch, at most OT_PSF_SCRATCH_BYTES however large the call. */
#define OT_PSF_MAX_SAMPLES 512
#define OT_PSF_SCRATCH_BYTES 67174400
int ot_monitor_psf_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                        const double* reference, const double* grid, int32_t ny, int32_t nz, const ot_segment_source* src,
                        const void* intensity, const void* n_index, const void* pathlength, const double* wavelength,
                        int64_t n_wavelengths, double wavelength_uniform, int32_t amplitude_mode, int64_t n_segments,
                        const int32_t* seg_count, int64_t n_rays, int64_t* counts, double* norm, double* re, double* im,
                        int32_t accumulate);

/* Diffraction PSF per ray group: ot_monitor_psf_many with a GROUP axis on the cells — the image of every wavelength, field point
 * or port of one batch from one pass over the segments.  Fields of different groups are never added: white light adds the
 * INTENSITIES of its wavelengths, and different field points make different images (the caller sums |U_g|^2 as it needs).
 * A CELL is a pair (monitor m, group g).  Every argument ot_monitor_psf_many has means what it means there, and so do the hit
 * test, W, lambda, the amplitude, the samples and the phase of a hit: a hit of slot s is exactly that call's hit.  It belongs to
 * group groups[ray[s]], where ray[s] is the int32 `ray` of the slot (src->ray: the index of the input ray the segment descends
 * from, in every layout and for every node of a ray tree) and `groups` is a DEVICE table of n_group_ids int32 ids, one per input ray.
 * A hit belongs to NO cell when its ray index is outside 0 .. n_group_ids - 1 (nothing is read out of range) or its id is outside
 * 0 .. n_groups - 1.  That is how rays are masked: id -1.  Such a hit adds to no field, norm or count; it is tallied in
 * ungrouped[m] (device, [n_monitors] int64, zeroed or kept with the other outputs), so that for every monitor
 * sum_g (used + skipped) + ungrouped = the hits ot_monitor_record_many finds.
 * Outputs, all on the device: counts [n_monitors][n_groups][3] int64 (used, skipped, aliased), norm [n_monitors][n_groups] double,
 * re, im [n_monitors][n_groups][ny][nz] double: U[m][g] is the sum over the usable hits of cell (m, g).  accumulate as there.
 * How: the hit list of the call is split by group on the device — a stable counting sort in two passes of the PSF kernel with a
 * scan between them, over tiles of 2048 consecutive hits of one monitor — into a second list in which the hits of cell (m, g) lie
 * together in the order they had (ascending slots); the sum then runs over the cells as ot_monitor_psf_many's runs over monitors.
 * Determinism: as ot_monitor_psf_many.  The place of a hit in the second list is a function of the inputs and their layout alone
 * (no position depends on the order in which an atomic lands; the ungrouped tally is an integer atomic, whose result does not),
 * the chunks of a cell are a function of its hit count alone, and their partial images are added in ascending order.  So the
 * result of cell (m, g) is bit for bit that of ot_monitor_psf_many over the segments of group g's rays alone in the same slot
 * order, and with n_groups = 1 and every id 0, counts, norm, re and im are ot_monitor_psf_many's bit for bit.
 * Synchronisation: two.  The hit totals per monitor come back to size the lists, as there; then, after the scan, the first hit of
 * every cell (first_cell, n_monitors * n_groups + 1 words) comes back, because the chunks of a launch and the pairs a launch
 * takes follow from the cells' hit counts.
 * Scratch: the hit list twice (80 bytes a hit), 12 bytes per (group, tile) and the partial images of ot_monitor_psf_many.
 * OT_ERR_INVALID, with nothing launched or zeroed: everything ot_monitor_psf_many refuses; groups or ungrouped NULL; n_groups
 * outside 1 .. OT_SPOT_GROUPS_MAX; n_group_ids < 1 (or >= 2^31); n_monitors * n_groups > OT_PSF_GROUP_CELLS_MAX;
 * n_monitors * n_groups * ny * nz > 2^27. */
#define OT_PSF_GROUP_CELLS_MAX 4096
int ot_monitor_psf_groups_many(ot_ctx* ctx, const ot_monitor* mons, int32_t n_monitors, const double* axes, int32_t reference_kind,
                               const double* reference, const double* grid, int32_t ny, int32_t nz, const int32_t* groups,
                               int64_t n_group_ids, int32_t n_groups, const ot_segment_source* src, const void* intensity,
                               const void* n_index, const void* pathlength, const double* wavelength, int64_t n_wavelengths,
                               double wavelength_uniform, int32_t amplitude_mode, int64_t n_segments, const int32_t* seg_count,
                               int64_t n_rays, int64_t* counts, double* norm, double* re, double* im, int64_t* ungrouped,
                               int32_t accumulate);

/* ---- measurement ------------------------------------------------------------------------ */
/* When enabled every trace launch is bracketed by hipEvents on the ctx stream. */
int ot_timing_enable(ot_ctx* ctx, int enabled);
/* Sum and count of kernel durations since the last reset (synchronises the stream). */
int ot_timing_read(ot_ctx* ctx, double* total_ms, int64_t* launches);
int ot_timing_reset(ot_ctx* ctx);

/* Tuning knobs (tools/tune.py, tests); the defaults are the measured best on MI355X. */
enum ot_option {
    OT_OPT_NT_STORES = 1,      /* segment records written with non-temporal stores (0/1)        */
    OT_OPT_MIN_WAVES = 2,      /* 0: compiler's choice; 4: cap registers for 4 waves per SIMD  */
    OT_OPT_BLOCKS_PER_CU = 3,  /* persistent-grid size in 256-thread blocks per CU (0 = auto)  */
    OT_OPT_KERNEL = 4,         /* 0 auto; 1 lane-per-ray kernel; 2 rolling-list kernel (heavy scenes) */
    OT_OPT_LDS_LIMIT_KB = 5,   /* scene images above this many KB are read from global memory   */
    OT_OPT_LIST_CAP = 6,       /* heavy scenes: live rays per wave in the rolling list: a multiple of 64, 128..1024 (mixed lists use it only if it is a power of two) */
    OT_OPT_PAIR_STORES = 7,    /* lane-per-ray kernel, slot arrays (ot_trace_*) only: lane pairs write two fields per 16-byte store (0/1); tiles are written one element per lane */
    OT_OPT_MIX_GENERATIONS = 8,/* heavy scenes: -1 auto, 0 generation-pure lists even under a top-level grid */
    OT_OPT_FLAT_QUEUE = 9,     /* planar scenes under a top-level grid: wave-wide candidate queue (0 / 1; a multiple of 64 in 192..8192:
                                  on, with room for that many (ray, leaf) pairs per round instead of 512 — lanes that do not fit wait a round) */
    OT_OPT_LDS_RECORDS = 10,   /* heavy scenes, fp32: records of the live rays in LDS (the first 128 positions of every wave's list; the rest
                                  of a generation-pure list of OT_OPT_LIST_CAP entries spills to global scratch): -1 auto, 0 never, 1 whenever it fits */
    OT_OPT_APPEND_CHUNK = 11,  /* ot_trace_append_*: slots a wave claims per atomic (multiple of 64, default 512) */
    OT_OPT_INSTANCING = 12,    /* fold identical lattice children (MMA / MLA / DMD) into one record + per-member pose at upload (0/1) */
    OT_OPT_GEN_REUSE = 13,     /* ot_trace_generation_*: the emit pass rebuilds the hit the count pass found (node + distance kept per
                                  ray) instead of searching the scene again: -1 auto (scenes of 12 nodes or more), 0 never, 1 always */
    OT_OPT_BLOCK_POOL = 14,    /* heavy scenes with curved surfaces, fp32: the live rays of a workgroup in one pool of 64-ray blocks in
                                  LDS, shared by its sixteen waves (k_trace_pool), instead of a list per wave: -1 auto, 0 never, 1 whenever it fits */
    OT_OPT_REFILL = 16,        /* heavy scenes under a top-level grid (mixed generations): the live rays in registers, every lane takes its
                                  next fresh ray in place (k_trace_refill) instead of a list per wave: 0 (default: the lists; the two tie on cfg 3), 1 whenever a kernel exists */
    OT_OPT_REFILL_TICKET = 17, /* ... rays a wave draws from the device-wide queue per atomic: 0 = by batch size (64..256), or a multiple of 64 */
    OT_OPT_GEN_ONEPASS = 19,   /* ot_trace_tree_*: every generation in ONE pass — each workgroup traces a tile of rays once, keeps the children in
                                  registers and takes its output offsets from a decoupled look-back over per-tile descriptors (k_gen_one) —
                                  instead of count + scan + emit: -1 (default) for generations of up to 65536 rays (one launch instead of six: what
                                  small ray trees cost), 0 never, 1 always.  Large generations are faster in two passes (every tile of the one-pass
                                  kernel waits for the slowest of its predecessors).  Scenes with count-limited surfaces always take the two
                                  passes.  Identical output either way. */
    OT_OPT_GEN_AHEAD = 20,     /* ot_trace_tree_*, light scenes without count-limited surfaces: the emit pass of a generation also counts the
                                  children of the children it writes, and the next generation replaces its count pass over the ray records by a pass
                                  over one byte per ray (k_gen_recount): 1 (default) / 0.  Identical output either way. */
    OT_OPT_TREES_GLOBAL_IMAGE = 25, /* ot_trace_trees_*: scenes whose image no LDS holds (thousands of leaves) are traced by the all-features tree kernel
                                  that reads the image from global memory; 1 = every scene takes that kernel (test knob: results must not change), 0 default */
    OT_OPT_GEN_PARENT_INDEX = 24, /* ot_trace_generation_*: 1 = next_tree[] receives, for every emitted ray, the INDEX of its parent in this call's
                                  `rays` instead of the parent's tree id (0, default).  For a host that keeps an object per ray and needs to know whose
                                  child a ray is while `tree` groups the rays for the FIFO-exact count gates: the object API's trace through scenes
                                  with user-defined components (optical_component.py:235-240; table.py _trace_hooked).  ot_trace_tree_* ignores it. */
    OT_OPT_TREES_FLAT = 23,    /* ot_trace_trees_*: planar scenes under a top-level grid of leaves search through the wave-wide pair queue of the
                                  heavy non-branching kernel (OT_OPT_FLAT_QUEUE) instead of a grid walk per lane: 1 (default) / 0.  Identical records. */
    OT_OPT_TREES_REFILL_AT = 22, /* ot_trace_trees_*: idle lanes of a wave at which they take the next trees of the wave's share (default 16: lanes
                                  kept busy; 64: a wave takes 64 trees at a time and its lanes stay at the same depth of their trees — faster
                                  when trees differ moderately in size, slower when most are tiny).  Identical records either way. */
    OT_OPT_TREES_LDS_ENTRIES = 21, /* ot_trace_trees_*: queue entries per lane kept in LDS (the rest of a tree's queue lives in a global scratch):
                                  more entries, fewer waves per CU.  0 (default): two under caps of up to 16, three above */
    OT_OPT_POOL_JITTER = 18,   /* test knob of the block pool's cross-wave protocol: one in `value` publications of a state or control word is
                                  held back ~8000 cycles after the records it announces were written (0 = off).  Results must not change. */
    OT_OPT_GEN_DROP_DOOMED = 15,/* ot_trace_generation_*: a tree whose budget ends with this generation gets no children in `next` (they
                                  could never be processed: optical_table.py:138-144) — 1 (default) / 0: emit them, for a caller who
                                  wants to go on with a larger budget */
    OT_OPT_UNIFORM = 26,       /* ot_trace_uniform_*, ot_trace_tiled_uniform_*, ot_bench_stream_*uniform_*: 1 (default) the uniform_mask is
                                  honoured; 0 it is dropped and every field is read per ray (A/B runs with one library).  Identical records. */
    OT_OPT_RESIDENT = 27       /* ot_trace_resident_*, ot_trace_reuse_* and their tiled forms: 1 (default) the resident_mask and the first_mask
                                  are honoured; 2 the resident_mask only; 0 both are dropped and every record is written whole (A/B runs
                                  with one library).  Identical records. */
};
int ot_set_option(ot_ctx* ctx, int32_t option, int32_t value);

/* Roofline companion of ot_trace_f64: the same streams (one ray record in, max_segments segment
 * records out per ray) with no tracing in between — the ceiling of this access pattern. */
int ot_bench_stream_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                        const ot_segments* out, int32_t* seg_count);
int ot_bench_stream_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                        const ot_segments* out, int32_t* seg_count);
/* ... and of ot_trace_tiled_*: the same records into 64-slot tiles. */
int ot_bench_stream_tiled_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                              int64_t capacity, int32_t* seg_count);
int ot_bench_stream_tiled_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                              int64_t capacity, int32_t* seg_count);
/* ... and of the uniform-field entry points: "the same bytes as the trace" holds with a mask too, so the ceiling reads the
 * flagged fields the way the trace does (element 0, once per wave).  A mask of 0 is the four calls above. */
int ot_bench_stream_uniform_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                                const ot_segments* out, int32_t* seg_count, uint32_t uniform_mask);
int ot_bench_stream_uniform_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments,
                                const ot_segments* out, int32_t* seg_count, uint32_t uniform_mask);
int ot_bench_stream_tiled_uniform_f64(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                                      int64_t capacity, int32_t* seg_count, uint32_t uniform_mask);
int ot_bench_stream_tiled_uniform_f32(ot_ctx* ctx, const ot_rays* rays, int64_t n_rays, int32_t max_segments, void* tiles,
                                      int64_t capacity, int32_t* seg_count, uint32_t uniform_mask);

#ifdef __cplusplus
}
#endif
#endif /* OPTABLE_HIP_H */
