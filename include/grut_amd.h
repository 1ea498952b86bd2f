/*
 * grut_amd.h — C-ABI of the MI355X-native 3DGUT / 3DGRT renderer plugin.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * torch types.  Every entry point replaces one method of the reference's
 * pybind11 classes (citations are into /root/reference):
 *
 *   gut_create / gut_destroy   <- SplatRaster(json)            threedgut_tracer/bindings.cpp:103-109,
 *                                                              src/splatRaster.cpp:163-181
 *   gut_forward                <- SplatRaster::trace            include/3dgut/splatRaster.h:47-63,
 *                                                              src/splatRaster.cpp:184-261
 *   gut_backward               <- SplatRaster::trace_bwd        include/3dgut/splatRaster.h:65-86,
 *                                                              src/splatRaster.cpp:264-350
 *   gut_timings                <- SplatRaster::collect_times    src/splatRaster.cpp:352-382
 *   grt_create / grt_destroy   <- OptixTracer(...)              threedgrt_tracer/include/3dgrt/optixTracer.h:128-147
 *   grt_build_bvh              <- OptixTracer::build_bvh        optixTracer.h:149-155, src/optixTracer.cpp:616-890
 *   grt_forward                <- OptixTracer::trace            optixTracer.h:157-166, src/optixTracer.cpp:893-960
 *   grt_backward               <- OptixTracer::trace_bwd        optixTracer.h:168-177, src/optixTracer.cpp:962-1031
 *
 * Ownership: every I/O buffer is allocated by the caller (PyTorch) on the GPU
 * the handle was created on; a handle owns only grow-only scratch (and, for
 * 3DGRT, the BVH).  All work is enqueued on the hipStream_t passed in; the
 * backward of a frame must be enqueued on the same stream as its forward
 * (same rule as gutRenderer.cu:436-440).  Functions return 0 on success and a
 * negative GrutStatus otherwise; nothing throws across this boundary.
 */
#ifndef GRUT_AMD_H
#define GRUT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (mirrors ErrorCode, 3dgut/utils/status.h:22-29) -------- */
typedef enum GrutStatus {
    GRUT_OK              = 0,
    GRUT_ERR_BAD_INPUT   = -1,
    GRUT_ERR_RUNTIME     = -2, /* a HIP call failed; see grut_last_error() */
    GRUT_ERR_NOT_READY   = -3, /* backward without a matching forward / BVH not built */
    GRUT_ERR_UNSUPPORTED = -4
} GrutStatus;

/* ---- camera model (sensors/cameraModels.h:22-72) ------------------------- */
enum { GRUT_SHUTTER_ROLLING_TOP_TO_BOTTOM = 0,
       GRUT_SHUTTER_ROLLING_LEFT_TO_RIGHT = 1,
       GRUT_SHUTTER_ROLLING_BOTTOM_TO_TOP = 2,
       GRUT_SHUTTER_ROLLING_RIGHT_TO_LEFT = 3,
       GRUT_SHUTTER_GLOBAL                = 4 };

enum { GRUT_CAMERA_OPENCV_PINHOLE = 0,
       GRUT_CAMERA_OPENCV_FISHEYE = 1,
       GRUT_CAMERA_FTHETA         = 2 };

enum { GRUT_FTHETA_PIXELDIST_TO_ANGLE = 0,
       GRUT_FTHETA_ANGLE_TO_PIXELDIST = 1 };

typedef struct GrutCamera {
    int32_t model;              /* GRUT_CAMERA_*  */
    int32_t shutter;            /* GRUT_SHUTTER_* */
    int32_t width, height;      /* resolution of the ray image */
    float principal_point[2];
    float focal_length[2];      /* pinhole + fisheye */
    float radial[6];            /* pinhole: k1..k6; fisheye: k1..k4 */
    float tangential[2];        /* pinhole */
    float thin_prism[4];        /* pinhole */
    float max_angle;            /* fisheye + ftheta */
    int32_t ftheta_reference_poly;
    float ftheta_pixeldist_to_angle[6];
    float ftheta_angle_to_pixeldist[6];
    float ftheta_linear_cde[3];
} GrutCamera;

/* ---- 3DGUT ---------------------------------------------------------------- */
/* Mirrors the conf.render.* keys setup_3dgut.py:41-95 turns into -D macros.   */
typedef struct GutConfig {
    int32_t particle_kernel_degree;      /* 2 (default 3dgut.yaml) | 4 | 3 | 5 | 8 | 1 | 0 */
    float   particle_kernel_min_response;/* 0.0113 */
    float   particle_kernel_min_alpha;   /* 1/255  */
    float   particle_kernel_max_alpha;   /* 0.99   */
    float   min_transmittance;           /* 1e-4   */
    int32_t particle_radiance_sph_degree;/* max degree of the SH buffer: 3 -> 16 coeffs */
    int32_t enable_hitcounts;
    int32_t enable_kernel_timings;
    /* render.splat.* */
    float   ut_alpha, ut_beta, ut_kappa; /* 1, 2, 0 */
    float   ut_in_image_margin_factor;   /* 0.1 */
    int32_t ut_require_all_sigma_points_valid; /* must be 0 (threedgut.cuh:78) */
    int32_t n_rolling_shutter_iterations;/* 5 */
    int32_t k_buffer_size;               /* 0 = unsorted compositing */
    int32_t global_z_order;              /* 1 */
    int32_t rect_bounding;               /* 1 */
    int32_t tight_opacity_bounding;      /* 1 */
    int32_t tile_based_culling;          /* 1 */
    /* fp16 feature I/O (setup_3dgut.py:60-61 PARTICLE_FEATURE_HALF / FEATURE_OUTPUT_HALF; defaults 0).
     * particle_feature_half: particle_sph is [N, 3*(deg+1)^2] IEEE half (splatRaster.cpp:90-98 converts the model's tensor per call);
     *   everything is computed in fp32 from the rounded coefficients, gradients stay fp32.
     * feature_output_half: out_feat_density (and feat_density of the backward) is [H,W,4] IEEE half (rayPayload.cuh:176-186,
     *   rayPayloadBackward.cuh:50-58); GutFrame::out_features / out_opacity must then be NULL.  Hit distance / count stay fp32. */
    int32_t particle_feature_half;
    int32_t feature_output_half;
    /* Neural harmonic features (model.feature_type = nht; setup_3dgut.py:47-57, threedgrut/model/features.py:133-175; any k_buffer_size since round 6: with k_buffer_size > 0 the sorted hit buffer sits in front of the feature integration, gutKBufferRenderer.cuh:158-225).  feature_transform_type 1: `particle_sph` is the per-particle feature buffer [N, particle_feature_dim] (fp32 or
     * half), features are interpolated per hit at the canonical intersection (gutKBufferRenderer.cuh:199-225,
     * neuralHarmonicFeaturesParticle.slang:146-196) and out_feat_density is [H, W, ray_feature_dim + 1] with
     * ray_feature_dim = interp_point_feature_dim x (2 x num_frequencies for sincos | num_frequencies for siren | 1), at most 32;
     * GutFrame::out_features / out_opacity must be NULL.  Backward: gut_backward only (gutKBufferRenderer.cuh:546-641): grad_feat_density is
     * [H, W, ray_feature_dim + 1], grad_particle_sph receives the feature buffer's gradient [N, particle_feature_dim] fp32, both gradient
     * outputs are fully written; gut_backward_unpacked / _factored return GRUT_ERR_UNSUPPORTED.  All zero = SH radiance. */
    int32_t feature_transform_type;              /* 0 SH radiance (default), 1 neural harmonic features */
    int32_t particle_feature_dim;                /* K: floats per particle (nht_features.dim, 48) */
    int32_t interp_point_feature_dim;            /* K / interpolation points (12) */
    int32_t feature_interpolation_support;       /* 0 centre (1 point), 1 tetrahedra (4 points, barycentric) */
    int32_t feature_activation_type;             /* 0 none, 1 siren, 2 sincos, 3 relu */
    int32_t feature_activation_num_frequencies;  /* (1) */
} GutConfig;

/* Per-call frame description: SplatRaster::trace's non-tensor arguments. */
typedef struct GutFrame {
    uint32_t   frame_id;
    int32_t    n_active_features;  /* active SH degree (model.n_active_features) */
    uint32_t   num_particles;
    int32_t    width, height;      /* rays are [height, width, 3] */
    GrutCamera camera;
    float      pose_start[7];      /* world->sensor, [t(3), q(x,y,z,w)] (tracer.py:359-380) */
    float      pose_end[7];
    /* Optional: camera-to-world matrices (row-major 4x4 f32) in DEVICE memory.  When device_T_to_world is non-NULL the
     * library derives the sensor poses on the GPU (same math as tracer.py:359-423) and ignores pose_start / pose_end, so
     * the caller never has to read the pose back to the host (the reference's `.cpu()` there drains the stream). */
    const float* device_T_to_world;
    const float* device_T_to_world_end; /* NULL: static sensor (end = start) */
    /* Optional extra outputs of gut_forward (device pointers, may be NULL): the radiance [H,W,3] and the opacity [H,W,1] as
     * separate CONTIGUOUS tensors next to out_feat_density [H,W,4] — what the reference plugin returns as `pred_features` /
     * `pred_opacity` after `.contiguous()` (tracer.py:334-337), written by the compositing kernel itself. */
    float* out_features;
    float* out_opacity;
} GutFrame;

/* Measured work of the last forward (for the roofline byte model). */
typedef struct GutStats {
    uint32_t num_particles;      /* N  */
    uint32_t num_visible;        /* Nv: particles with >=1 tile */
    uint64_t num_intersections;  /* I  */
    uint32_t num_tiles;
    uint32_t key_bits;           /* bits of the tile part of the sort key */
    /* Work the two compositing sweeps actually did in the last frame, counted on the device when gut_profile_enable(handle, 2)
     * is in effect (0 otherwise): tile-list entries a half-tile wave EVALUATED (each one a 68-byte fetch: list entry, particle row,
     * radiance) and, of those, the entries at least one of its 128 pixels ACCEPTED (each one a 64-byte gradient slot in the
     * backward).  A sweep stops at the rays' termination, so these are far below the list length I; the roofline of the sweeps
     * is priced with them (bench.py: roofline.touched_bytes). */
    uint64_t fwd_entries_evaluated, fwd_entries_accepted;
    uint64_t bwd_entries_evaluated, bwd_entries_accepted;
} GutStats;

typedef struct GutHandle GutHandle;

int  gut_create(const GutConfig* config, GutHandle** handle);
void gut_destroy(GutHandle* handle);
int  gut_trim(GutHandle* handle);   /* release all scratch (see grut_set_allocator); the next frame allocates afresh */

/*  particle_density : [N,12] f32  {pos.xyz, density, quat.wxyz, scale.xyz, pad}
 *  particle_sph     : [N, 3*(deg+1)^2] f32, coefficient-major float3
 *  ray_origin/dir   : [H,W,3] f32, in sensor space (transformed by the inverse mid-exposure pose)
 *  out_feat_density : [H,W,4] f32  (rgb, 1-T)          fully overwritten when N > 0: rays that miss the scene box get 0
 *  out_hit_distance : [H,W,1] f32                      fully overwritten when N > 0: missing rays get 1e6 (splatRaster.cpp:213)
 *  out_hit_count    : [H,W,1] f32                      fully overwritten when N > 0 and hit counts are enabled; untouched otherwise
 *  out_visibility   : [N]     i32 (bit pattern read by the caller as float, splatRaster.cpp:215), fully overwritten
 *  With N == 0 nothing is launched and the outputs keep whatever the caller put there (the reference's zeros / 1e6). */
/*  (particle_sph / out_feat_density are void*: fp32 by default, IEEE half with GutConfig::particle_feature_half / feature_output_half) */
int gut_forward(GutHandle* handle, void* stream, const GutFrame* frame,
                const float* particle_density, const void* particle_sph,
                const float* ray_origin, const float* ray_direction,
                void* out_feat_density, float* out_hit_distance,
                float* out_hit_count, int32_t* out_visibility);

/*  grad_hit_distance     : [H,W,1] f32 or NULL when no gradient flows into the hit distance (the usual
 *                          training case: trainer.py:677-748 supervises colour/opacity only) — selects the
 *                          kernel variant without the hit-distance terms
 *  grad_particle_density : [N,12] f32 and grad_particle_sph [N, 3*(deg+1)^2] f32 are fully overwritten (no zero fill
 *                          needed): gradients are gathered per particle from per-tile-entry partials, not accumulated
 *                          with atomics, so they are bitwise reproducible from run to run */
int gut_backward(GutHandle* handle, void* stream, const GutFrame* frame,
                 const float* particle_density, const void* particle_sph,
                 const float* ray_origin, const float* ray_direction,
                 const void* feat_density, const float* grad_feat_density,
                 const float* hit_distance, const float* grad_hit_distance,
                 float* grad_particle_density, float* grad_particle_sph);

/* gut_backward with the gradient tensors in the CALLER's layout instead of the reference's packed one (new surface; the reference
 * plugin concatenates the two upstream gradients into [H,W,4] and slices the packed [N,12] result apart again,
 * threedgut_tracer/tracer.py:226-285 — two extra passes per iteration that this entry point makes unnecessary):
 *   grad_features [H,W,3], grad_opacity [H,W,1]: upstream gradients as autograd delivers them; either may be NULL (= zero);
 *   grad_positions [N,3], grad_density [N,1], grad_rotation [N,4] (16-byte aligned), grad_scale [N,3]: fully overwritten.
 * Same preconditions, errors and results (bit for bit) as gut_backward; k_buffer_size > 0 is GRUT_ERR_UNSUPPORTED here. */
typedef struct GutGradIO {
    const float* grad_features;
    const float* grad_opacity;
    float* grad_positions;
    float* grad_density;
    float* grad_rotation;
    float* grad_scale;
} GutGradIO;
int gut_backward_unpacked(GutHandle* handle, void* stream, const GutFrame* frame,
                          const float* particle_density, const void* particle_sph,
                          const float* ray_origin, const float* ray_direction,
                          const void* feat_density, const float* hit_distance, const float* grad_hit_distance,
                          const GutGradIO* io, float* grad_particle_sph);

/* ---- the model's two SH tensors read in place (new surface) ----------------------------------------------------------------------
 * Every SH configuration of the reference keeps the radiance coefficients in two Parameters, features_albedo [N,3] and
 * features_specular [N,45] (threedgrut/model/model.py:204-210), and joins them with torch.cat on every get_features() call
 * (model.py:94-96); autograd then slices grad_particle_sph [N,48] apart again and clones both slices.  The three entry points below
 * are gut_forward, gut_backward and gut_backward_unpacked with that pair in place of particle_sph and the pair of their gradients in
 * place of grad_particle_sph (they replace the get_features() call at the top of 3dgrut_amd/gut_tracer.py's Tracer.render and the
 * single g_sph tensor of its autograd Function): virtual float e of particle i's 48-float row is sph_albedo[3 i + e] for e < 3 and
 * sph_specular[45 i + e - 3] otherwise, for the coefficients and for their gradients.  The arithmetic and its order are the twins':
 * every output equals theirs bit for bit.
 *   sph_albedo [N,3] f32, sph_specular [N,45] f32: read only, and only rows of the arrays (specular rows are 180 bytes: row i begins
 *     on a 4-byte boundary only, and nothing is read beyond float 45 N);
 *   grad_sph_albedo [N,3] f32, grad_sph_specular [N,45] f32: fully overwritten - zeros for particles without tiles and for the
 *     coefficients beyond 3 (n_active_features + 1)^2 - with no atomics: two calls give equal bits.
 * Alignment: the four base pointers must be 16-byte aligned (GRUT_ERR_BAD_INPUT otherwise; any allocator's blocks are).
 * Accepted configurations: SH radiance (feature_transform_type 0) with particle_radiance_sph_degree 3, fp32 coefficients
 * (particle_feature_half 0) and k_buffer_size 0; anything else is GRUT_ERR_UNSUPPORTED with the reason in grut_last_error().  A NULL
 * among the four pointers is GRUT_ERR_BAD_INPUT.  Both errors come before any launch and leave the handle's forward context alone.
 * Forward context: as for the twins (same handle, stream, frame_id, density and ray pointers, else GRUT_ERR_NOT_READY); the SH
 * pointers are not part of it, and a forward of one kind may be followed by a backward of the other.
 * GRUT_GUT_UNFUSED_FINALIZE=1 selects the two-kernel gradient finalisation here as it does for the twins. */
int gut_forward_split(GutHandle* handle, void* stream, const GutFrame* frame,
                      const float* particle_density, const float* sph_albedo, const float* sph_specular,
                      const float* ray_origin, const float* ray_direction,
                      void* out_feat_density, float* out_hit_distance,
                      float* out_hit_count, int32_t* out_visibility);
int gut_backward_split(GutHandle* handle, void* stream, const GutFrame* frame,
                       const float* particle_density, const float* sph_albedo, const float* sph_specular,
                       const float* ray_origin, const float* ray_direction,
                       const void* feat_density, const float* grad_feat_density,
                       const float* hit_distance, const float* grad_hit_distance,
                       float* grad_particle_density, float* grad_sph_albedo, float* grad_sph_specular);
int gut_backward_unpacked_split(GutHandle* handle, void* stream, const GutFrame* frame,
                                const float* particle_density, const float* sph_albedo, const float* sph_specular,
                                const float* ray_origin, const float* ray_direction,
                                const void* feat_density, const float* hit_distance, const float* grad_hit_distance,
                                const GutGradIO* io, float* grad_sph_albedo, float* grad_sph_specular);

/* ---- frames nobody differentiates (new surface) ----------------------------------------------------------------------------------
 * gut_forward keeps, next to the image, what gut_backward restarts from: the running state of every pixel at every 64th entry of its
 * tile's list (80 B of table per tile entry against the 20 B of the lists themselves, plus a table of its own for the neural-harmonic
 * fast path), the tile each such boundary cuts and the marks of the boundaries a wave reached alive.  Validation passes, rendering,
 * viewers and visibility filters never run a backward.  gut_forward_only and gut_forward_only_split are gut_forward and
 * gut_forward_split for those frames (they replace the same SplatRaster::trace, src/splatRaster.cpp:184-261, which has no such mode:
 * the reference's GUTRenderer fills one forward context for every frame, train or not, gutRenderer.cu:252-253); same arguments, same
 * preconditions and errors, the same arithmetic in the same order, so every output - image, out_features / out_opacity, hit distance,
 * hit count, visibility, the N == 0 and no-intersection outputs, gut_stats, gut_timings, gut_debug_fetch - equals the twin's bit for
 * bit.  What differs:
 *   - the compositing sweeps run in their builds without checkpoint stores (unsorted SH half-tile and quarter-tile kernels, the
 *     neural-harmonic fast path; the sorted k-buffer and generic feature forwards never had any), the tile-range pass writes no
 *     boundary tiles, the reached marks are not cleared;
 *   - the checkpoint tables are neither allocated nor grown: a handle that only renders such frames never owns them (gut_memory);
 *   - the handle remembers that its last frame was forward-only, and every gut_backward* entry point then returns
 *     GRUT_ERR_NOT_READY before anything is launched or read, with a grut_last_error() that says so.  The next gut_forward /
 *     gut_forward_split clears the mark; it allocates the tables it finds missing or shorter than the lists and starts from cleared
 *     reached marks, so training and forward-only frames may alternate on one handle in any order, with gut_trim in between or not;
 *   - an instrumented frame (gut_profile_enable level 2) counts no forward-sweep entries: the counting build is the training sweep's. */
int gut_forward_only(GutHandle* handle, void* stream, const GutFrame* frame,
                     const float* particle_density, const void* particle_sph,
                     const float* ray_origin, const float* ray_direction,
                     void* out_feat_density, float* out_hit_distance,
                     float* out_hit_count, int32_t* out_visibility);
int gut_forward_only_split(GutHandle* handle, void* stream, const GutFrame* frame,
                           const float* particle_density, const float* sph_albedo, const float* sph_specular,
                           const float* ray_origin, const float* ray_direction,
                           void* out_feat_density, float* out_hit_distance,
                           float* out_hit_count, int32_t* out_visibility);
/* Bytes of device scratch the handle owns right now (HOST function, no device work; new surface, the reference's
 * GutRenderForwardContext, gutRenderer.cu:99-110, reports nothing of the kind): out[0] = all of it, out[1] = the five per-intersection lists (tile keys
 * and payloads with their sort ping-pong, entry -> particle), out[2] = the checkpoint tables of the backward (per-pixel state, its
 * neural-harmonic twin, reached marks, boundary tiles).  out[2] is 0 for a handle that has only rendered forward-only frames. */
int gut_memory(GutHandle* handle, uint64_t out[3]);

/* ---- view-sharded data parallelism: the radiance gradient in factored form (new surface; the reference is
 * single-GPU) ------------------------------------------------------------------------------------------------------------------
 * With one view per GPU, the gradient exchange of a step is dominated by grad_particle_sph: 3*(deg+1)^2 floats per particle
 * (192 B at degree 3 of the 236 B total) that are, per view, the outer product of two small factors — the SH basis at the
 * particle's view direction (a function of the particle and the sensor position alone) and the 3-float radiance gradient
 * behind the clamp (GUTProjector::evalBackward, gutProjector.cuh:390-431).  gut_backward_factored is gut_backward without the
 * expansion: it returns that view-specific factor,
 *   grad_radiance [N+1,3] f32, fully overwritten: rows 0..N-1 = dL/d(unclamped per-particle radiance) of this view (0 where the
 *                 radiance was clamped or the particle was not rendered), row N = the view's sensor position in world space,
 * and grad_particle_density exactly as gut_backward does (including the view-direction part of the position gradient).
 * Ranks gather the factors (12 B per particle and view over the links instead of 192 B through an all-reduce) and every rank
 * rebuilds the sum over views locally with grut_sph_grad_from_views:
 *   grad_particle_sph[p][k] = scale * sum_v basis_k(normalize(position_p - sensor_v)) * grad_radiance_v[p],  k < (n_active+1)^2
 * view_factors [num_views, N+1, 3] (the gathered grad_radiance buffers, in rank order: every rank adds the views in the same
 * order, so replicas stay bitwise identical); positions: N rows of position_stride floats whose first three are the particle
 * position (3 for a [N,3] tensor, 12 for particle_density rows); scale: 1 for a sum over views, 1/num_views for a mean.
 * With num_views = 1 and scale = 1 the result is bit for bit what gut_backward writes.  Same preconditions and errors as
 * gut_backward (forward context on the same stream); with N == 0 nothing is launched and nothing is written. */
int gut_backward_factored(GutHandle* handle, void* stream, const GutFrame* frame,
                          const float* particle_density, const void* particle_sph,
                          const float* ray_origin, const float* ray_direction,
                          const void* feat_density, const float* grad_feat_density,
                          const float* hit_distance, const float* grad_hit_distance,
                          float* grad_particle_density, float* grad_radiance);

/* gut_backward_factored with the gradient finalisation cut into `num_chunks` particle ranges (starting at multiples of 128): after the
 * launches of each chunk the library calls on_chunk(user, chunk, first_particle, num_particles) ON THE CALLING THREAD; rows [first, first +
 * num) of grad_particle_density and grad_radiance are then complete in stream order, and the caller may enqueue that chunk's collectives
 * (3dgrut_amd/dp.py: all-reduce of the packed rows, all-gather of the view factors), which run under the next chunk's kernels.  Row N of
 * grad_radiance (the sensor position) is written with the first chunk.  Results are bit for bit gut_backward_factored's. */
typedef void (*GrutChunkFn)(void* user, uint32_t chunk, uint32_t first_particle, uint32_t num_particles);
int gut_backward_factored_chunked(GutHandle* handle, void* stream, const GutFrame* frame,
                                  const float* particle_density, const void* particle_sph,
                                  const float* ray_origin, const float* ray_direction,
                                  const void* feat_density, const float* grad_feat_density,
                                  const float* hit_distance, const float* grad_hit_distance,
                                  float* grad_particle_density, float* grad_radiance,
                                  uint32_t num_chunks, GrutChunkFn on_chunk, void* user);
int grut_sph_grad_from_views(void* stream, uint32_t num_particles, uint32_t num_views, const float* view_factors,
                             const float* positions, uint32_t position_stride, int32_t n_active_features, int32_t sph_degree,
                             float scale, float* grad_particle_sph);

/* average ms of the forward / backward launches since the last call (-1 if none). Synchronises. */
int gut_timings(GutHandle* handle, float* forward_ms, float* backward_ms);
int gut_stats(GutHandle* handle, GutStats* stats);

/* Per-stage device time (hipEvents on the launch stream), for the roofline report.  While enabled, every
 * gut_forward / gut_backward brackets each stage with an event pair; gut_profile_read synchronises, returns the
 * average ms per stage since the last read (-1 where a stage did not run) and resets the accumulators. */
enum { GUT_STAGE_PROJECT = 0, GUT_STAGE_DEPTH_SORT, GUT_STAGE_SCAN, GUT_STAGE_EXPAND, GUT_STAGE_TILE_SORT,
       GUT_STAGE_TILE_RANGES, GUT_STAGE_RENDER_FWD, GUT_STAGE_RENDER_BWD, GUT_STAGE_PROJECT_BWD, GUT_NUM_STAGES };
int gut_profile_enable(GutHandle* handle, int enable);
/* Restrict the event pairs to the stages whose bit (1 << GUT_STAGE_*) is set (default: all).  Two event records between adjacent
 * stages leave ~10 us of idle stream on MI355X; timing only the kernel of interest keeps the rest of the frame back to back. */
int gut_profile_select(GutHandle* handle, uint32_t stage_mask);
int gut_profile_read(GutHandle* handle, float* stage_ms /* [GUT_NUM_STAGES] */);

/* ---- stage-level entry points (parity tests drive each stage alone) ------ */
/* Stable LSD radix sort of (key,value) pairs on key bits [begin_bit,end_bit). tmp buffers sized n.
 * keys, keys_tmp and scratch must be 16-byte aligned (the passes read the keys, and scan the histogram rows in scratch, 16 bytes at a
 * time); a misaligned pointer is GRUT_ERR_BAD_INPUT and nothing is launched. */
int grut_sort_pairs_u32(void* stream, uint32_t n, int begin_bit, int end_bit,
                        uint32_t* keys, uint32_t* values,
                        uint32_t* keys_tmp, uint32_t* values_tmp,
                        void* scratch, uint64_t scratch_bytes,
                        uint32_t** sorted_keys, uint32_t** sorted_values);
uint64_t grut_sort_scratch_bytes(uint32_t n);
/* inclusive prefix sum of n u32 (cub::DeviceScan::InclusiveSum, gutRenderer.cu:302-310); in and out must be 16-byte aligned
 * (GRUT_ERR_BAD_INPUT otherwise, nothing launched) */
int grut_inclusive_scan_u32(void* stream, uint32_t n, const uint32_t* in, uint32_t* out,
                            void* scratch, uint64_t scratch_bytes);
uint64_t grut_scan_scratch_bytes(uint32_t n);
/* The same two primitives with the arguments the renderers vary.
 * Sort: n_dev (DEVICE pointer, may be NULL) holds the live count, clamped to n - only the first min(*n_dev, n) pairs are read and
 * written, n is then the capacity of the buffers; values_iota != 0: the payload of pair i is i, generated by the first pass - `values`
 * is never read but still serves as a ping-pong buffer.  Same alignment rule.
 * Scan: gather (DEVICE pointer, may be NULL): element i of the input is in[gather[i]]; `in` may then have any alignment, out not. */
int grut_debug_sort_pairs_u32(void* stream, uint32_t n, const uint32_t* n_dev, int begin_bit, int end_bit,
                              uint32_t* keys, uint32_t* values, uint32_t* keys_tmp, uint32_t* values_tmp, int values_iota,
                              void* scratch, uint64_t scratch_bytes, uint32_t** sorted_keys, uint32_t** sorted_values);
/* grut_debug_sort_pairs_u32 with the tile geometry of the three-kernel passes forced: tile_keys = keys per workgroup, one of 2048
 * (256 threads x 8), 4096 (256 x 16), 8192 (512 x 16), 16384 (1024 x 16); 0 = the library's own choice for n.  Any other value is
 * GRUT_ERR_BAD_INPUT.  grut_sort_scratch_bytes(n) is enough for every geometry. */
int grut_debug_sort_pairs_u32_tiled(void* stream, uint32_t n, const uint32_t* n_dev, int begin_bit, int end_bit,
                                    uint32_t* keys, uint32_t* values, uint32_t* keys_tmp, uint32_t* values_tmp, int values_iota,
                                    uint32_t tile_keys, void* scratch, uint64_t scratch_bytes, uint32_t** sorted_keys, uint32_t** sorted_values);
int grut_debug_scan_gather_u32(void* stream, uint32_t n, const uint32_t* in, const uint32_t* gather, uint32_t* out,
                               void* scratch, uint64_t scratch_bytes);
/* Tile ranges of a 3DGUT frame from its sorted tile keys (16-byte aligned) alone: ranges[t] = [first, last) of the entries whose
 * key & tile_mask is t < num_tiles (tiles without entries are NOT written: clear the table first), boundary_tile[b] = the tile of entry
 * b * *segment (0xFFFFFFFF where that entry's tile is >= num_tiles) for every such entry below the live count min(*n_dev, n) (n alone
 * with n_dev NULL).  *segment (HOST) receives the library's segment length. */
int gut_debug_tile_ranges(void* stream, uint32_t n, const uint32_t* n_dev, uint32_t tile_mask, uint32_t num_tiles,
                          const uint32_t* sorted_tile_keys, uint32_t* ranges, uint32_t* boundary_tile, uint32_t* segment);

/* Copies the binning products of the last gut_forward to caller DEVICE buffers (any may be NULL):
 * tiles_count[N] u32, proj_pos[N,2], conic_opacity[N,4], extent[N,2], depth[N], rgb[N,3],
 * sorted_particle_idx[I] u32, tile_ranges[tiles,2] u32. */
/* Diagnostics of an instrumented frame (gut_profile_enable level 2): the raw counter block to a caller DEVICE buffer — words 0..3 =
 * GutStats' four entry counters, words 16 + 4 b .. 19 + 4 b = lifetime and start (100 MHz ticks), accepted << 32 | evaluated entries and
 * tile-list length of forward-sweep workgroup b. */
int gut_debug_fetch_work(GutHandle* handle, void* stream, unsigned long long* out, uint64_t count);
/* HOST function, no device work: the world->sensor pose [t(3), q(x,y,z,w)] the library derives from a camera-to-world matrix handed
 * over as GutFrame::device_T_to_world (row-major 4x4, rows 0-2 read) - the host twin of the device code, same arithmetic: float64
 * general inverse, one rounding to float32, float32 quaternion (threedgut_tracer/tracer.py:88-136, 359-380, 413-423). */
int grut_debug_pose_from_c2w(const float* c2w16, float* out7);
/* The whole per-frame pose block the kernels read (47 floats: start R[9] t[3] q[4], end t[3] q[4], mid-exposure world->sensor
 * R[9] t[3], sensor->world R[9] t[3]; sensors.h:44-73, gutRenderer.cu:266-267) from camera-to-world matrices: on_device != 0 runs the
 * device code on DEVICE matrices and synchronises the stream, on_device == 0 its host twin on HOST matrices.  T_end may be NULL. */
int grut_debug_frame_poses(void* stream, int on_device, const float* T_start, const float* T_end, float* host_out47);
int gut_debug_fetch(GutHandle* handle, void* stream,
                    uint32_t* tiles_count, float* proj_pos, float* conic_opacity, float* extent,
                    float* depth, float* rgb, uint32_t* sorted_particle_idx, uint32_t* tile_ranges);

/* ---- 3DGRT ----------------------------------------------------------------- */
typedef struct GrtConfig {
    int32_t particle_kernel_degree;        /* 4 (3dgrt.yaml) */
    float   particle_kernel_min_response;  /* 0.0113 */
    float   particle_kernel_min_alpha;     /* 1/255 */
    float   particle_kernel_max_alpha;     /* 0.99 */
    int32_t particle_kernel_density_clamping; /* 1 */
    int32_t particle_radiance_sph_degree;  /* 3 */
    int32_t enable_normals;
    int32_t enable_hitcounts;
    int32_t enable_kernel_timings;
    int32_t max_hits_per_trace;            /* 16 (pipelineParameters.h:83) */
    /* fp16 feature I/O (setup_3dgrt.py:42-43; 3dgrt/pipelineParameters.h:24-46): particle_sph as IEEE half / out_features (and the
     * `features` input of the backward) as [H,W,3] IEEE half; arithmetic and gradients stay fp32 */
    int32_t particle_feature_half;
    int32_t feature_output_half;
    /* Neural harmonic features (model.feature_type = nht with render.pipeline_type referenceSlang / referenceSlangBwd:
     * referenceSlangOptix.cu:103-186, referenceSlangBwdOptix.cu:70-185), same fields and meaning as in GutConfig: particle_sph is the
     * feature buffer [N, particle_feature_dim], out_features / features are [H, W, ray_feature_dim] (at most 32), grad_particle_sph the
     * feature buffer's gradient; enable_normals must be 0.  All zero = SH radiance (the `reference` pipeline). */
    int32_t feature_transform_type;
    int32_t particle_feature_dim;
    int32_t interp_point_feature_dim;
    int32_t feature_interpolation_support;
    int32_t feature_activation_type;
    int32_t feature_activation_num_frequencies;
    /* render.primitive_type (optixTracer.cpp:176-201): the proxy geometry a particle is traced through.  GRUT_PRIM_INSTANCES: the unit cube
     * under the particle's instance transform, hit distance = the point of maximum response (intersectInstanceParticle).  The closed convex
     * triangle meshes of particlePrimitives.cu:63-496: the ray is offered the particle at the distance at which it ENTERS the proxy (OptiX
     * triangles with back faces culled, referenceOptix.cu:62), rays that start inside are not offered it.  GRUT_PRIM_CUSTOM: custom primitives over
     * the particles' WORLD boxes (computeGaussianEnclosingAABBKernel) with the world-space intersection program intersectCustomParticle
     * (gaussianParticles.cuh:407-441): the instances' hit point, offered to the rays that cross the world box, accepted within 3 sigma.
     * The open meshes GRUT_PRIM_TRISURFEL / GRUT_PRIM_TRIHEXA and the enclosing spheres GRUT_PRIM_SPHERE: below. */
    int32_t primitive_type;
    /* render.pipeline_type (optixTracer.cpp:246-318: the forward program's file).  GRUT_PIPELINE_REFERENCE: referenceOptix.cu.
     * GRUT_PIPELINE_REFERENCE_SLANG: referenceSlangOptix.cu (SH radiance or neural harmonic features).  The Slang programs integrate the same
     * function as the hand-written ones and run on the same kernels, with ONE difference in the candidate test: for GRUT_PRIM_CUSTOM the Slang
     * intersection program (particleDensityHitCustom, gaussianParticles.slang:489-523) reports the UNSIGNED distance of the point of maximum
     * response, so a particle whose maximum lies behind the ray origin is a candidate there and not under GRUT_PIPELINE_REFERENCE (forward and
     * backward alike).  Every other primitive: bit-equal program outputs (tests/golden/grt_trace_slang_sh_prims.npz).
     * GRUT_PIPELINE_BARYCENTRIC_SURFELS: barycentricSurfelsOptix.cu - FORWARD ONLY (the reference ships
     * no backward program for it): trisurfel proxies (primitive_type must be GRUT_PRIM_TRISURFEL), ten hits per trace, the response evaluated
     * from the squared distance of the ray's crossing of the surfel's plane in the proxy frame (the hit triangle's barycentrics) with the
     * kernel-scaled minimum response, depth from the triangle hit distances, normals from the surfel's plane.  grt_backward returns
     * GRUT_ERR_UNSUPPORTED. */
    int32_t pipeline_type;
} GrtConfig;
enum { GRUT_PIPELINE_REFERENCE = 0, GRUT_PIPELINE_BARYCENTRIC_SURFELS = 1, GRUT_PIPELINE_REFERENCE_SLANG = 2 };
enum { GRUT_PRIM_INSTANCES = 0, GRUT_PRIM_ICOSAHEDRON = 1, GRUT_PRIM_OCTAHEDRON = 2, GRUT_PRIM_TETRAHEDRON = 3, GRUT_PRIM_DIAMOND = 4, GRUT_PRIM_CUSTOM = 5,
       /* trisurfel (particlePrimitives.cu:155-205): two triangles per particle = the rhombus |x| + |y| <= sqrt 2 of the proxy's z = 0 plane, traced
        * WITHOUT face culling (referenceOptix.cu:62); the hit is the ray's crossing of that plane and the per-hit math takes its
        * SurfelPrimitive branches (gaussianParticles.cuh:371-400, 512-521, 558-565, 628-659). */
       GRUT_PRIM_TRISURFEL = 6,
       /* trihexa (particlePrimitives.cu:107-153): three rhombi in the proxy's coordinate planes, six triangles, back faces culled - the windings
        * make the x = 0 / y = 0 rhombi face +x / +y and the two halves of the z = 0 rhombus face opposite ways, so a ray is offered the SAME
        * particle up to three times at three distances and the programs process every offer as a hit of the particle.  Here every rhombus is a
        * proxy of its own (3 N leaves, proxy 3 i + j = plane j of particle i). */
       GRUT_PRIM_TRIHEXA = 7,
       /* sphere (optixTracer.cpp:189-190, 765-781, 823-833; computeGaussianEnclosingSphereKernel, particlePrimitives.cu:386-403): one OptiX
        * built-in sphere per particle, centre mu, radius max(scale) * kernelScale.  The built-in intersector offers the any-hit program the
        * ray's ENTRY into the sphere and - the program ignores every offer but the one that fills its payload - its EXIT as well: the particle is
        * a candidate at both roots and is processed twice when both fall into the ray's rounds (the volumetric processHit either time).  Here
        * every root is a proxy of its own (2 N leaves, proxy 2 i = entry, 2 i + 1 = exit of particle i).  NVIDIA does not publish the
        * intersector's arithmetic: the roots are those of |po + t pd|^2 = 1 in the frame scaled by the radius, operation by operation as
        * oracle/grt_oracle.c and the emulated OptiX of oracle/ref/ref_grt_emul.inl evaluate them. */
       GRUT_PRIM_SPHERE = 8 };

typedef struct GrtFrame {
    uint32_t frame_id;
    int32_t  sph_degree;          /* active SH degree */
    float    min_transmittance;
    uint32_t num_particles;
    int32_t  width, height;
    float    ray_to_world[12];    /* row-major 3x4 */
    int32_t  keep_hits_for_backward; /* forward: record the processed hits so that grt_backward of the same frame
                                      * replays them instead of traversing again (identical results) */
    const float* device_ray_to_world; /* optional: row-major 4x4 (or 3x4) matrix in DEVICE memory, read by the kernels instead of
                                       * ray_to_world — a pose that lives on the GPU needs no host copy (the reference does
                                       * rayToWorld.cpu() per call, optixTracer.cpp:931) */
} GrtFrame;

typedef struct GrtStats {
    uint32_t num_particles;
    uint32_t num_nodes;
    uint64_t nodes_visited;     /* only in instrumented launches */
    uint64_t candidates;
    uint64_t processed_hits;
    float    scene_aabb[6];
    uint64_t list_entries;      /* last forward: entries of the packet lists (0: the tree walk served the frame — rays with different origins) */
    uint64_t packet_tests;      /* only in instrumented launches: candidate tests of whole packets (list entries / leaves tested by a wave) */
    uint64_t list_batches;      /* only in instrumented launches: 64-entry batches of packet lists fetched by the trace rounds (one 64-byte record per entry) */
    uint32_t bwd_rederived_rays;   /* last replayed backward: rays whose rounds were re-derived instead of replayed (a round met more ghosts than a log chunk holds) */
    uint32_t bwd_premise_rays;     /* last replayed backward: rays for which the ghost filter's premise failed (DESIGN.md "3DGRT backward"; expected 0) */
    uint64_t bwd_atomic_instructions; /* last replayed backward: atomic-add instructions issued (one per differentiated hit or same-slot group of hits) */
    uint64_t bwd_atomic_words;     /* ... and the non-zero float words they carried (to 16): what scripts/atomic_calib.hip's rate prices */
} GrtStats;

typedef struct GrtHandle GrtHandle;

/* ---- hybrid mesh + Gaussian path tracing (BASELINE config 5) -------------------------------------------------------------------
 * Replaces HybridOptixTracer::buildMeshBVH / traceHybrid (threedgrut_playground/include/playground/hybridTracer.h:121-141) and the
 * OptiX programs of threedgrut_playground/src/kernels/cuda/playgroundKernel.cu:39-352 with materials.cuh, trace.cuh, rng.cuh under
 * them: per ray a path loop — closest triangle, the face's primitive type (none / mirror / glass / diffuse / PBR: Cook-Torrance
 * sampling with GGX importance sampling, glTF alpha modes, diffuse / emissive / metallic-roughness / normal textures, vertex tangents),
 * then the Gaussians between the ray origin and the surface with the forward program's k = 16 rounds (3dgrtTracer.cuh:137-204),
 * transmittance and path throughput carried along the whole path; the environment map is looked up along the last ray.  Forward
 * only, like the reference.  All array pointers are DEVICE pointers owned by the caller; the GrtMaterial table itself is a HOST
 * array (the library uploads it with the launch: a few hundred bytes, as HybridOptixTracer::syncMaterials does).
 * Textures: row-major [height, width, channels] f32, sampled with normalised coordinates, clamp-to-edge, bilinear — the modes
 * playground/cutexture.h:54-60 sets (CUDA filters with 8 fractional weight bits; here the float weights themselves). */
typedef struct GrtTexture {
    const float* data;                /* NULL: no texture */
    int32_t height, width, channels;
} GrtTexture;
typedef struct GrtMaterial {          /* PBRMaterial, playground/pipelineParameters.h:26-52 */
    GrtTexture diffuse, emissive, metallic_roughness, normal;   /* 4, 4, 2, 4 channels */
    float diffuse_factor[4], emissive_factor[3];
    float metallic_factor, roughness_factor, transmission_factor, ior, alpha_cutoff;
    uint32_t alpha_mode;              /* GltfAlphaMode (pipelineDefinitions.h:42-48): 0 opaque, 1 blend, 2 mask */
} GrtMaterial;
typedef struct GrtMesh {
    uint32_t num_vertices, num_faces;
    const float*   vertices;            /* [V,3] */
    const int32_t* triangles;           /* [F,3] vertex indices */
    const float*   vertex_normals;      /* [V,3] (needed with playground_opts bit 0) */
    const float*   vertex_tangents;     /* [V,3] or NULL */
    const uint8_t* vertex_has_tangents; /* [V]   or NULL (no precomputed tangents) */
    const int32_t* prim_type;           /* [F] PlaygroundPrimitiveTypes (pipelineDefinitions.h:18-24): 0 none, 1 mirror, 2 glass, 3 diffuse, 4 PBR */
    const float*   mat_uv;              /* [F,3,2] texture coordinates per face corner, or NULL (0) */
    const int32_t* mat_id;              /* [F] row of `materials`, or NULL (0) */
    const float*   refractive_index;    /* [F] */
    uint32_t num_materials;
    const GrtMaterial* materials;       /* HOST array [num_materials] (needed when a diffuse or PBR face exists) */
    GrtTexture envmap;                  /* [EH,EW,4]; data == NULL: black */
    float envmap_offset[2];             /* rotates the environment (trace.cuh:233-257) */
} GrtMesh;
typedef struct GrtHybridOptions {
    uint32_t playground_opts;         /* PlaygroundRenderOptions: bit 0 smooth normals, bit 1 disable Gaussian tracing, bit 2 disable PBR textures */
    uint32_t max_pbr_bounces;         /* the path loop runs while pbrNumBounces < max_pbr_bounces */
    uint32_t frame_number;            /* seeds the per-pixel random streams (rng.cuh; playgroundKernel.cu:59, materials.cuh:224-228) */
} GrtHybridOptions;
/* rebuild = 0 with allow_update != 0 and an unchanged face count refits the boxes of the existing tree (OPTIX_BUILD_OPERATION_UPDATE,
 * hybridTracer.cpp buildMeshBVH); anything else builds from scratch */
int grt_build_mesh_bvh(GrtHandle* handle, void* stream, uint32_t num_vertices, const float* vertices, uint32_t num_faces,
                       const int32_t* triangles, int rebuild, int allow_update);
/* rays [H,W,3] in ray space (frame->ray_to_world applies); ray_max_t [H,W] or NULL; out_radiance [H,W,3], out_opacity [H,W,1] fully
 * written; out_last_ray [H,W,6] (world-space origin + direction of the last segment: what the reference writes back into its ray
 * buffers, trace.cuh:158-173) and out_bounces [H,W] (mirror bounces) may be NULL. */
/* (particle_sph: IEEE half with GrtConfig::particle_feature_half; the four outputs are always fp32) */
int grt_trace_hybrid(GrtHandle* handle, void* stream, const GrtFrame* frame, const float* particle_density, const void* particle_sph,
                     const float* ray_origin, const float* ray_direction, const float* ray_max_t, const GrtMesh* mesh,
                     const GrtHybridOptions* options, float* out_radiance, float* out_opacity, float* out_last_ray, uint32_t* out_bounces);

/* ---- frame denoiser of the playground (replaces HybridOptixTracer::denoise, playground/hybridTracer.h:143) -------------------------
 * The reference hands the engine's tonemapped RGB frame, and nothing else (no albedo, normal or flow layer), to OptiX's learned LDR
 * denoiser (hybridTracer.cpp:428-498); those weights are not public.  THIS PROJECT'S CHOICE of algorithm is non-local means
 * (Buades, Coll, Morel 2005), an exact formula on RGB alone; the call surface is the reference's.
 * rgb_in, rgb_out: [batch, height, width, 3] f32, DEVICE, dense.  With f = patch_radius, r = search_radius, n = 3 (2f+1)^2 and
 * X_MAX = 80, for a pixel p of image b and every OTHER pixel q of the same image with |q - p|_inf <= r that lies inside the image:
 *   d2(p,q) = sum over o in [-f,f]^2, c in {r,g,b} of (I[clamp(p+o)]_c - I[clamp(q+o)]_c)^2     (clamp: each coordinate to the image)
 *   x(p,q)  = min(d2(p,q) / (n h^2), X_MAX)
 *   w(p,q)  = exp(-x(p,q))                  (>= e^-80, a normal fp32 number: no weight is ever zero)
 *   w(p,p)  = max over those q of w(p,q), or 1 when there is no such q (a 1x1 image)
 *   out[p]  = (sum_q w(p,q) I[q] + w(p,p) I[p]) / (sum_q w(p,q) + w(p,p))
 * The min is a continuous clamp, not a cut to zero: with the max rule for the centre a cut would make an isolated pixel's result jump
 * when one far neighbour crosses the threshold.  Nothing clamps the values: the frame is nominally in [0, 1].
 * Out of place: rgb_out is written completely and rgb_in is never written (the engine keeps the input as its accumulation buffer).
 * No address depends on a pixel's value: a NaN or inf pixel makes the outputs within r + f of it unspecified and moves no load or
 * store.  No atomics; the order of every sum depends on (height, width, f, r) only, so two calls on one input are bitwise equal; the
 * images of a batch never see each other.  One launch on `stream`; no scratch, no allocation, no synchronisation.
 * GRUT_ERR_BAD_INPUT before any HIP call, with the argument named by grut_last_error: a NULL among cfg, rgb_in, rgb_out; f outside
 * 0..4; r outside 1..16; h not finite or <= 0; height or width 0; batch * height * width >= 2^31; ranges of rgb_in and rgb_out that
 * overlap.  batch == 0 is GRUT_OK without a launch. */
typedef struct GrutDenoiseConfig {
    int32_t patch_radius;             /* f: patches are (2f+1)^2 pixels; the plugin's default is 3 */
    int32_t search_radius;            /* r: candidates are the (2r+1)^2 - 1 pixels around p; default 7 */
    float   h;                        /* strength: the per-element patch distance at which a weight is 1/e; default 0.1 */
} GrutDenoiseConfig;
int grut_denoise(void* stream, const GrutDenoiseConfig* cfg, uint32_t batch, uint32_t height, uint32_t width, const float* rgb_in,
                 float* rgb_out);

int  grt_create(const GrtConfig* config, GrtHandle** handle);
int  grt_trim(GrtHandle* handle);
void grt_destroy(GrtHandle* handle);

/* positions[N,3], rotations[N,4] wxyz normalised, scales[N,3], densities[N] — activated values */
int grt_build_bvh(GrtHandle* handle, void* stream, uint32_t num_particles,
                  const float* positions, const float* rotations,
                  const float* scales, const float* densities,
                  int rebuild, int allow_update);

/*  out_features [H,W,3], out_density [H,W,1], out_hit_distance [H,W,2] (integrated depth, last hit t),
 *  out_normals [H,W,3], out_hits_count [H,W,1], out_visibility [N] i32 — all must arrive zero-filled.
 *  Replaces OptixTracer::trace (optixTracer.h:150-163, optixTracer.cpp:890-1000).  When every ray of the frame starts at the same
 *  point (decided on the device from ray_origin) the candidates of each 8x8 ray packet are binned once per frame and the k = 16 trace
 *  rounds scan sorted per-packet lists instead of walking the BVH (identical results; GrtStats::list_entries tells which path ran; the
 *  call then waits once for the list size — a 4-byte read-back — before it enqueues the trace).  Environment GRUT_GRT_NO_LISTS=1
 *  forces the tree walk. */
/*  (particle_sph / out_features are void*: fp32 by default, IEEE half with GrtConfig::particle_feature_half / feature_output_half) */
int grt_forward(GrtHandle* handle, void* stream, const GrtFrame* frame,
                const float* particle_density, const void* particle_sph,
                const float* ray_origin, const float* ray_direction,
                void* out_features, float* out_density, float* out_hit_distance,
                float* out_normals, float* out_hits_count, int32_t* out_visibility);

int grt_backward(GrtHandle* handle, void* stream, const GrtFrame* frame,
                 const float* particle_density, const void* particle_sph,
                 const float* ray_origin, const float* ray_direction,
                 const void* features, const float* density, const float* hit_distance, const float* normals,
                 const float* grad_features, const float* grad_density,
                 const float* grad_hit_distance, const float* grad_normals,
                 float* grad_particle_density, float* grad_particle_sph);

/* grt_forward that also records, per ray, the particles it processed in order (the BVH hit-order parity test):
 * hit_ids [H*W, capacity] u32, hit_counts [H*W] u32 (counts may exceed capacity; only the first `capacity` are stored) */
int grt_debug_forward_hits(GrtHandle* handle, void* stream, const GrtFrame* frame,
                           const float* particle_density, const void* particle_sph,
                           const float* ray_origin, const float* ray_direction,
                           void* out_features, float* out_density, float* out_hit_distance,
                           float* out_normals, float* out_hits_count, int32_t* out_visibility,
                           uint32_t* hit_ids, uint32_t* hit_counts, uint32_t capacity);
/* Parity aid: until called again with NULLs, every grt_backward also writes, per ray (caller DEVICE buffers of W*H entries, zero-filled
 * by the caller), how many hits it differentiated and an order-independent signature of which particles they were
 * (sum of particle * 0x9E3779B97F4A7C15 + 1, mod 2^64) — the tests compare the replayed backward with the re-derived one ray by ray. */
int grt_debug_backward_signature(GrtHandle* handle, unsigned long long* ray_signature, uint32_t* ray_hit_count);
/* proxy instance records of the last build: [N,12] f32 = rows of W = diag(1/kscl) R^T, then mu (object ray: o' = W (o - mu)) */
int grt_debug_fetch_instances(GrtHandle* handle, void* stream, float* instances);
/* GRUT_PRIM_CUSTOM: [N,8] f32 = the particle's world box (min xyz, max xyz; computeGaussianEnclosingAABBKernel, particlePrimitives.cu:498-541),
 * kernelScale^2, 0 - what the candidate test of the custom primitives reads.  GRUT_ERR_NOT_READY for another primitive type. */
int grt_debug_fetch_custom_boxes(GrtHandle* handle, void* stream, float* box8);
/* The per-packet candidate lists of the last train-mode forward (GrtStats::list_entries of them) to caller DEVICE buffers: ranges [blocks,2]
 * ([first, last) of each 8x8 ray packet, row-major), entries [list_entries] particle ids (top bit: internal flag).  GRUT_ERR_NOT_READY when
 * the tree walk served the frame or the capacity is too small.  The parity tests hand them to the CPU checker as a candidate prefilter. */
int grt_debug_fetch_lists(GrtHandle* handle, void* stream, uint32_t* ranges, uint32_t* entries, uint64_t entry_capacity);
/* Packet ranges from sorted block keys (16-byte aligned) alone: ranges[2 k], ranges[2 k + 1] = [first, last) of the entries whose key is
 * k < num_blocks (blocks without entries are not written), over the first min(*n_dev, n) entries (n alone with n_dev NULL). */
int grt_debug_list_ranges(void* stream, uint32_t n, const uint32_t* n_dev, uint32_t num_blocks, const uint32_t* sorted_keys,
                          uint32_t* ranges);

int grt_timings(GrtHandle* handle, float* forward_ms, float* backward_ms, float* build_ms);
int grt_stats(GrtHandle* handle, GrtStats* stats);
/* Diagnostics of an instrumented forward (environment GRUT_GRT_COUNT=1): the raw counter block to a caller DEVICE buffer — words 0..11
 * the totals grt_stats reports, then per launched workgroup {start, lifetime (10 ns ticks of the chip-wide counter), node visits << 32 |
 * leaf visits}.  Development aid (scripts/diag_grt_balance.py). */
int grt_debug_fetch_work(GrtHandle* handle, void* stream, unsigned long long* out, uint64_t count);

/* ---- parameter marshalling -------------------------------------------------- */
/* [N,3] positions, [N,1] density, [N,4] rotation (wxyz), [N,3] scale (all contiguous fp32, DEVICE) -> [N,12] ParticleDensity
 * rows {position, density, quaternion, scale, 0}: the torch.cat of threedgut_tracer/tracer.py:178 and
 * threedgrt_tracer/tracer.py:93-96, in one pass. */
int grut_pack_particles(void* stream, uint32_t num_particles, const float* positions, const float* density,
                        const float* rotation, const float* scale, float* particle_density);

/* The inverse for gradients: packed [N,12] -> [N,3] positions, [N,1] density, [N,4] rotation, [N,3] scale, contiguous
 * (what tracer.py:268-285 hands to autograd as strided slices). */
int grut_unpack_particle_grads(void* stream, uint32_t num_particles, const float* grad_particle_density, float* grad_positions,
                               float* grad_density, float* grad_rotation, float* grad_scale);

/* The same packing fused with the model's activations (threedgrut/model/model.py:102-118 with the defaults of
 * configs/base_gs.yaml:77-78 and model.py:241): density = sigmoid(raw), scale = exp(raw), rotation = normalize(raw).
 * Replaces three elementwise passes + the torch.cat per call. */
int grut_activate_pack(void* stream, uint32_t num_particles, const float* positions, const float* raw_density,
                       const float* raw_rotation, const float* raw_scale, float* particle_density);
/* Chain rule of the above: the renderer's packed gradient [N,12] -> gradients of the four RAW tensors (all fully written). */
int grut_activate_pack_backward(void* stream, uint32_t num_particles, const float* raw_density, const float* raw_rotation,
                                const float* raw_scale, const float* grad_particle_density, float* grad_positions,
                                float* grad_raw_density, float* grad_raw_rotation, float* grad_raw_scale);

/* ---- opacity and scale regularisers (threedgrut/trainer.py:722-736, on in configs/base_mcmc.yaml) ------------ */
/* The two means Trainer3DGRUT.get_losses takes of the ACTIVATED parameters, from the raw tensors:
 *   out[0] = 1/N  sum_i  sigmoid(raw_density[i])          torch.abs(model.get_density()).mean()
 *   out[1] = 1/3N sum_ij exp(raw_scale[i][j])             torch.abs(model.get_scale()).mean()
 * Both activations are non-negative, so the reference's abs is the identity and is not evaluated.  Each activation is evaluated in
 * double and rounded to fp32 once: the expf that grut_activate_pack renders with was measured up to 11 ulp off on gfx950, which is
 * more than the bounds of these sums and gradients allow; the value rendered is within those 11 ulp of the value regularised.
 * A NULL input skips its term and its slot of `out` is +0.0f; at least one input is needed.
 * Summation, all fp32 and in one fixed order: a lane sums its float4 as (x + y) + (z + w) and carries the trips of its grid-stride
 * loop in a compensated (Kahan) sum; 64 lanes and then the 4 waves of a block are added as balanced binary trees; a second launch
 * of one block adds the block partials in index order, again as a balanced tree, and divides.  The non-zero leaves fill a prefix of
 * every tree, so no term passes more than min(ceil(log2(count)), 22) roundings, whatever N is.  No atomics, no allocation, no
 * synchronisation, two launches on `stream`, a grid that depends on N only: two calls on the same input are bitwise equal.
 * partials: grut_reg_partials(N) floats of scratch that belong to the caller (two per block, at most 8 KiB); nothing has to be
 * zeroed.  grut_reg_partials is host arithmetic and returns 0 where the forward call would refuse N.
 *
 * Backward, one launch, grad_out [2] read on the device:
 *   grad_raw_density[i]  = grad_out[0] / N  * s (1 - s),  s = sigmoid(raw_density[i])
 *   grad_raw_scale[i][j] = grad_out[1] / 3N * exp(raw_scale[i][j])
 * s (1 - s) is evaluated as e / (1 + e)^2 with e = exp(-|x|), which keeps its leading digits where s rounds to 1; every element
 * is computed in double and rounded once.  Each output is
 * overwritten completely.  A NULL gradient pointer means that term is not wanted (its slot of grad_out is not read); a gradient
 * whose input is NULL is an error, and so are two NULL gradients.  Where an activation underflows to exactly 0 the reference's
 * abs passes sign(0) = 0 and these formulas give 0 as well: no special case.
 * Every non-NULL tensor base must be 16-byte aligned (the flat [N] and [3N] arrays move as float4; one may straddle rows of
 * raw_scale).  GRUT_ERR_BAD_INPUT, before any launch and with the argument named by grut_last_error: N == 0, 3N >= 2^32, both
 * inputs NULL, a NULL out / partials / grad_out, a misaligned base. */
uint32_t grut_reg_partials(uint32_t num_particles);
int grut_reg_forward(void* stream, uint32_t num_particles, const float* raw_density, const float* raw_scale, float* partials, float* out);
int grut_reg_backward(void* stream, uint32_t num_particles, const float* raw_density, const float* raw_scale, const float* grad_out,
                      float* grad_raw_density, float* grad_raw_scale);

/* ---- MCMC densification strategy (threedgrut/strategy/mcmc.py) ---------------------------------------------- */
/* Replaces compute_relocation_kernel (threedgrut/strategy/src/gaussian_mcmc.cu:36-66, host side :70-92), one lane per sampled
 * Gaussian: new_opacities[i] = 1 - (1 - opacities[i])^(1/n), new_scales[i] = opacities[i] / D * scales[i] with
 * D = sum_{a=1..n} sum_{k=0..a-1} binoms[(a-1) n_max + k] (-1)^k / sqrt(k+1) new_opacities[i]^(k+1), summed in that order in fp32.
 * n = ratios[i] clamped to [1, n_max] (the reference's caller clamps, mcmc.py:203-205; the clamp keeps every table read in bounds).
 * Device tensors: opacities / new_opacities [n], scales / new_scales [n,3], ratios int32 [n], binoms [n_max, n_max]. */
int grut_mcmc_relocation(void* stream, uint32_t n, const float* opacities, const float* scales, const int32_t* ratios,
                         const float* binoms, int n_max, float* new_opacities, float* new_scales);
/* Replaces MCMCStrategy.perturb_gaussians after its noise draw (threedgrut/strategy/mcmc.py:169-187, with get_covariance of
 * model.py:120-130 and quaternion_to_so3 of utils/misc.py:67-88) in one pass:
 * positions += R S S^T R^T (noise * sigmoid(-100 ((1 - density) - 0.995)) * noise_lr * lr), IN PLACE.
 * activated = 0: rotation [n,4] / scale [n,3] / density [n,1] are the model's RAW parameters and normalize / exp / sigmoid are
 * applied here (the defaults of configs/base_gs.yaml); activated = 1: they are already activated.  noise [n,3] is the caller's
 * torch.randn_like(positions) (the random generator stays the caller's).  rotation 16-byte aligned; nothing is allocated. */
int grut_mcmc_perturb(void* stream, uint32_t n, float* positions, const float* rotation, const float* scale, const float* density,
                      const float* noise, float noise_lr, float lr, int activated);

/* The strategy's two periodic events, relocate_gaussians and add_new_gaussians (mcmc.py:109-165, 189-224), as fused passes.  None of
 * the four allocates, synchronises or uses float atomics; every buffer is a contiguous DEVICE buffer of the caller; zero rows launch
 * nothing; row counts are below 2^31.  A NULL among the required pointers or a value out of range is GRUT_ERR_BAD_INPUT before any
 * HIP call, and grut_last_error() names the argument. */
/* Replaces the two torch.where of relocate_gaussians (mcmc.py:112-116) and the gather densities[alive_idxs].flatten() of
 * sample_new_gaussians (mcmc.py:198).  density [n]: the ACTIVATED densities as the caller computed them.  dead_idx int64 [n]: ascending,
 * the rows with density <= threshold; alive_idx int64 [n]: ascending, the rows with density > threshold (a NaN is in neither, as with
 * torch.where); alive_prob [n]: density[alive_idx], copied as bits (what torch.multinomial is given); counts[2] = {n_dead, n_alive} in
 * device memory.  Only the first n_dead / n_alive entries of the lists are written.  scratch: grut_mcmc_classify_scratch_bytes(n)
 * bytes, 16-byte aligned. */
int grut_mcmc_classify(void* stream, uint32_t n, const float* density, float threshold, int64_t* dead_idx, int64_t* alive_idx,
                       float* alive_prob, uint32_t* counts, void* scratch, uint64_t scratch_bytes);
uint64_t grut_mcmc_classify_scratch_bytes(uint32_t n);
/* Replaces sample_new_gaussians after its torch.multinomial draw (mcmc.py:202-222): valid_indices[sampled], bincount and its gather
 * and clamp, the gathers around compute_relocation_tensor, the relocation and the two inverse activations.
 * sampled int64 [m]: the draws; index_map (optional) int64 [n_map]: source[j] = index_map[sampled[j]], otherwise sampled[j] (draws and
 * mapped indices are clamped into their ranges, so nothing is accessed out of bounds).  density [n] ACTIVATED; scale [n,3] raw
 * (scale_activated = 0: exp is applied here) or activated (1); binoms [n_max, n_max].
 * Out: source int64 [m]; count int32 [n]: the histogram of source (cleared here); first int32 [n]: the smallest j with source[j] == i
 * (INT32_MAX where count is 0); with ratio = clamp(count[source[j]] + 1, 1, n_max) and (new_o, new_s) the relocation of
 * grut_mcmc_relocation (the same device function): new_density_act [m] = new_o and new_scale_act [m,3] = new_s (both optional),
 * new_density_raw [m] = logf(x / (1 - x)) with x = min(max(new_o, threshold), 1 - FLT_EPSILON) and an IEEE division,
 * new_scale_raw [m,3] = logf(new_s).  Draws of one source get bit-identical values. */
int grut_mcmc_sample_plan(void* stream, uint32_t n, uint32_t m, const int64_t* sampled, const int64_t* index_map, uint32_t n_map,
                          const float* density, const float* scale, int scale_activated, const float* binoms, int n_max, float threshold,
                          int64_t* source, int32_t* count, int32_t* first, float* new_density_raw, float* new_scale_raw,
                          float* new_density_act, float* new_scale_act);
enum { GRUT_MCMC_MAX_TENSORS = 32 };
enum { GRUT_MCMC_ROLE_COPY = 0,          /* a parameter whose rows are copied */
       GRUT_MCMC_ROLE_NEW_DENSITY = 1,   /* the raw density [.,1]: sources and copies take new_density */
       GRUT_MCMC_ROLE_NEW_SCALE = 2,     /* the raw scale [.,3]: sources and copies take new_scale */
       GRUT_MCMC_ROLE_STATE = 3          /* an optimizer moment */ };
typedef struct GrutMcmcTensor {
    void* data;          /* [rows, row_elems] of 4-byte elements, moved as bits */
    uint32_t row_elems;
    uint32_t role;       /* GRUT_MCMC_ROLE_* */
} GrutMcmcTensor;
/* Replaces update_param_fn / update_optimizer_fn of relocate_gaussians (mcmc.py:121-131) as applied to every parameter and moment by
 * strategy/base.py:77-107, IN PLACE and in ONE launch over all num_tensors <= 32 tensors (a host array, passed on by value).  With
 * source / first / new_density [m] / new_scale [m,3] of grut_mcmc_sample_plan and dead_idx int64 [m] (distinct rows, none of them a source):
 *   COPY     data[dead_idx[j]] = data[source[j]]
 *   NEW_*    data[source[j]] = new[j], written by the j with first[source[j]] == j, and data[dead_idx[j]] = new[j]
 *   STATE    data[source[j]] = 0 (dead rows keep their moments) */
int grut_mcmc_relocate_rows(void* stream, const GrutMcmcTensor* tensors, uint32_t num_tensors, uint32_t m, const int64_t* source,
                            const int64_t* dead_idx, const int32_t* first, const float* new_density, const float* new_scale);
/* Replaces update_param_fn / update_optimizer_fn of add_new_gaussians (mcmc.py:148-158: the indexed write, torch.cat([param,
 * param[sampled]]) and zeros + cat per moment) in ONE launch over all tensors: tensors[k].data [n, row_elems] -> outs[k] [n + m,
 * row_elems] (must not overlap any input).
 *   rows i < n    outs[i] = data[i]; NEW_*: new[first[i]] where count[i] > 0
 *   rows n + j    COPY: data[source[j]]; NEW_*: new[j]; STATE: 0 */
int grut_mcmc_append_rows(void* stream, const GrutMcmcTensor* tensors, void* const* outs, uint32_t num_tensors, uint32_t n, uint32_t m,
                          const int64_t* source, const int32_t* count, const int32_t* first, const float* new_density,
                          const float* new_scale);

/* ---- default densification strategy (threedgrut/strategy/gs.py) ------------------------------------------------ */
/* None of these allocates or synchronises; every tensor is a contiguous DEVICE tensor of the caller. */
/* Replaces GSStrategy.update_gradient_buffer (gs.py:131-139) in one pass: for every row with a non-zero (or NaN) component of
 * positions_grad [n,3]: accum[i] += || positions_grad[i] * ||positions[i] - c||_2 ||_2 / 2 and denom[i] += 1 (accum fp32 [n], denom
 * int32 [n]); all other rows of both buffers are left untouched.  c is read from DEVICE memory at sensor_position[0],
 * [sensor_stride], [2 sensor_stride] (element stride: the caller's T_to_world[0, :3, 3] view has stride 4 and is read in place). */
int grut_densify_accumulate(void* stream, uint32_t n, const float* positions_grad, const float* positions,
                            const float* sensor_position, int64_t sensor_stride, float* accum, int32_t* denom);
enum { GRUT_APPEND_COPY = 0,   /* the appended block holds copies of the selected rows */
       GRUT_APPEND_ZERO = 1    /* the appended block is zeros (the optimizer's moments of new Gaussians) */ };
/* The destinations of the boolean indexing in clone_gaussians / split_gaussians / prune_* (gs.py:154-283): keep / append are byte
 * masks [n] (torch bool storage); keep = NULL means every row, append = NULL none.  Writes the exclusive prefix sums keep_offset [n],
 * append_offset [n] and counts[2] = {n_keep, n_append} (device memory).  scratch: grut_relayout_scratch_bytes(n) bytes, 16-byte
 * aligned like the offsets. */
int grut_relayout_scan(void* stream, uint32_t n, const uint8_t* keep, const uint8_t* append, uint32_t* keep_offset,
                       uint32_t* append_offset, uint32_t* counts, void* scratch, uint64_t scratch_bytes);
uint64_t grut_relayout_scratch_bytes(uint32_t n);
/* Replaces torch.cat([v[keep], v[append].repeat(copies, 1)]) of one tensor (the update_param_fn / update_optimizer_fn closures of
 * gs.py:179-196, :218-223, :236-240, :258-262, :276-280 as applied by strategy/base.py:76-107): in [n, row_elems] of 4-byte elements
 * (copied as bits) -> out [n_keep + copies n_append, row_elems].  Kept row i lands at keep_offset[i]; copy c of appended row i at
 * n_keep + c n_append + append_offset[i] (the whole block repeated), zeros instead with GRUT_APPEND_ZERO.  Masks, offsets and counts
 * are those of grut_relayout_scan; an output of zero rows launches nothing. */
int grut_relayout_rows(void* stream, uint32_t n, uint32_t row_elems, const void* in, const uint8_t* keep, const uint8_t* append,
                       const uint32_t* keep_offset, const uint32_t* append_offset, uint32_t n_keep, uint32_t n_append,
                       uint32_t copies, int append_mode, void* out);
/* Finishes the appended block of a split (gs.py:168-186, exp scale activation) IN PLACE over its n = copies n_append rows, given the
 * tails of the new raw tensors: positions += R(q / |q|) (noise * exp(scale)) with R of quaternion_to_so3 (utils/misc.py:67-88,
 * q = (w, x, y, z) from rotation_tail [n,4]) and noise [n,3] standard normals; then scale = log(exp(scale) / (0.8 copies)): exp in
 * fp32, the quotient and its logarithm in fp64 rounded once (closer to the exact value than the reference's all-fp32 chain, not
 * bit-identical to it). */
int grut_split_tail(void* stream, uint32_t n, float* positions_tail, float* scale_tail, const float* rotation_tail,
                    const float* noise, uint32_t copies);

/* ---- fused SSIM loss (the `fused_ssim` package as called by threedgrut/model/losses.py:31-33) ------------------- */
/* Both entry points replace fused_ssim(img1, img2, padding) of the CUDA-only third-party extension the reference's loss imports
 * (threedgrut/model/losses.py:17; trainer.py:715-720 evaluates 1 - ssim on every step).  Window: separable 11-tap Gaussian, sigma 1.5,
 * zero padding per channel and image; C1 = 0.01^2, C2 = 0.03^2; valid = 0: mean of the map over all B C H W pixels ("same"), valid = 1:
 * over map[:, :, 5:-5, 5:-5] ("valid", needs H, W >= 11).
 * Strides contract: img1 / img2 / grad_img1 are [B, C, H, W] fp32 DEVICE tensors addressed through ELEMENT strides for (B, C, H, W), so a
 * contiguous NCHW tensor and an NCHW view of channels-last memory (stride_c = 1, stride_w = C, C <= 4: read as contiguous runs) are both
 * read in place; any other non-negative strides are accepted and read element-wise.  Outputs and scratch belong to the caller:
 * out_mean [1], partials [the companion below] and, when training, three planes of B C H W floats each (all three NULL: inference, no
 * plane is written).  Nothing needs to be zeroed; every element of every buffer is written before it is read.  The result is bitwise
 * reproducible (fixed-order reduction, no atomics); nothing synchronises with the host. */
int grut_ssim_forward(void* stream, int B, int C, int H, int W, const float* img1, const int64_t* stride1, const float* img2,
                      const int64_t* stride2, int valid, float* out_mean, float* partials, float* dm_dmu1, float* dm_ds1, float* dm_ds12);
/* dL/dimg1 = G*(dL dm_dmu1) + 2 img1 G*(dL dm_ds1) + img2 G*(dL dm_ds12) with dL = grad_out[0] / count inside the counted region and 0
 * outside (img2 is a constant: no gradient, as upstream).  grad_out [1] is read from DEVICE memory; grad_img1 is fully written through
 * grad_stride (pass img1's strides and autograd has nothing to re-lay out). */
int grut_ssim_backward(void* stream, int B, int C, int H, int W, const float* img1, const int64_t* stride1, const float* img2,
                       const int64_t* stride2, int valid, const float* grad_out, const float* dm_dmu1, const float* dm_ds1,
                       const float* dm_ds12, float* grad_img1, const int64_t* grad_stride);
/* How many floats of `partials` the forward call may write for this shape (one per workgroup; 0 for a bad shape). */
uint32_t grut_ssim_partials(int B, int C, int H, int W);

/* ---- fused photometric loss (threedgrut/trainer.py:687-720: mask, L1, L2 and SSIM of get_losses) ------------------- */
/* One pass over both images each way for everything Trainer3DGRUT.get_losses takes from them.  With a = mask pred and b = mask gt
 * (trainer.py:692-694; mask NULL: a = pred, b = gt):
 *   out[0] = mean |a - b|                 torch.abs(rgb_pred - rgb_gt).mean()                            trainer.py:701
 *   out[1] = mean (pred - b)^2            mse_loss(outputs["pred_features"], rgb_gt): UNMASKED pred      trainer.py:709
 *   out[2] = mean SSIM(a, b)              ssim(permute(rgb_pred), permute(rgb_gt)), see grut_ssim_forward trainer.py:717-719
 * terms selects what is computed: 1 (L1) | 2 (L2) | 4 (SSIM); out[k] of a term that is not selected is written as 0.  valid as for
 * grut_ssim_forward (it only concerns the SSIM term, as does the H, W >= 11 limit).  pred / gt / grad_pred follow the strides contract of
 * the SSIM entry points; mask is a [B, H, W] fp32 DEVICE tensor addressed through mask_stride[3] (element strides of B, H, W), broadcast
 * over the channels and read once per pixel.  partials [grut_photo_loss_partials] and the three planes (B C H W floats each; all NULL for
 * inference, and only allowed with the SSIM term selected) belong to the caller; nothing needs to be zeroed, no atomics, bitwise reproducible.
 * With mask NULL and terms = 4, out[2] and the gradient are bit for bit those of grut_ssim_forward / grut_ssim_backward. */
int grut_photo_loss_forward(void* stream, int B, int C, int H, int W, const float* pred, const int64_t* pred_stride, const float* gt,
                            const int64_t* gt_stride, const float* mask, const int64_t* mask_stride, int terms, int valid, float* out,
                            float* partials, float* dm_dmu1, float* dm_ds1, float* dm_ds12);
/* The backward of all selected terms in one launch (replaces autograd's chain for trainer.py:693-720), grad_out [3] read from DEVICE
 * memory (entries of terms that are not selected are not read), P = B C H W:
 *   dL/dpred = mask [ G*(dL dm_dmu1) + 2 a G*(dL dm_ds1) + b G*(dL dm_ds12) ]   dL = grad_out[2] / count inside the counted region
 *            + grad_out[0] mask sign(a - b) / P                                  sign(0) = 0
 *            + 2 grad_out[1] (pred - b) / P
 * grad_pred is fully written through grad_stride.  The planes are those the forward call wrote (NULL without the SSIM term). */
int grut_photo_loss_backward(void* stream, int B, int C, int H, int W, const float* pred, const int64_t* pred_stride, const float* gt,
                             const int64_t* gt_stride, const float* mask, const int64_t* mask_stride, int terms, int valid,
                             const float* grad_out, const float* dm_dmu1, const float* dm_ds1, const float* dm_ds12, float* grad_pred,
                             const int64_t* grad_stride);
/* How many floats of `partials` the forward call may write for this shape (three per workgroup; 0 for a bad shape). */
uint32_t grut_photo_loss_partials(int B, int C, int H, int W);

/* ---- PPISP post-processing (threedgrut/utils/render.py:110-151, trainer.py:1166-1168) ---------------------------------- */
/* The learned camera model the reference's trainer applies to every rendered frame before the loss (post_processing.method: ppisp), one
 * pass over the image each way.  P pixels; rgb / out / grad_out / grad_rgb [P,3] and pixel_coords [P,2] (x, y with their +0.5) are
 * contiguous fp32 DEVICE arrays; (res_w, res_h) is the image's resolution.  Stages, in order, with the ALREADY SELECTED parameter rows
 * (the caller adds the frame's or camera's offset; nothing here reads an index or waits for the host):
 *   exposure   [1]   x = rgb 2^e
 *   vignetting [3,5] per channel (centre x, centre y, a1, a2, a3): uv = (pc - (W/2, H/2)) / max(W, H), r2 = |uv - centre|^2,
 *                    x_c *= clamp(1 + a1 r2 + a2 r2^2 + a3 r2^3, 0, 1)
 *   color      [8]   latents blue, red, green, neutral (two each) -> a 3x3 homography Hm; v = Hm (r, g, I) with I = r + g + b,
 *                    v *= I / (v.z + 1e-5), rgb = (v.x, v.y, v.z - v.x - v.y)
 *   crf        [3,4] per channel raw (toe, shoulder, gamma, centre): toe, shoulder = 0.3 + softplus, gamma = 0.1 + softplus,
 *                    centre = clamp(sigmoid, 1e-6, 1 - 1e-6), l = max((shoulder - toe) centre + toe, 1e-6), a = shoulder centre / l,
 *                    x = clamp(x, 0, 1), y = a (x / centre)^toe for x <= centre, else 1 - (1 - a) ((1 - x) / (1 - centre))^shoulder,
 *                    out = max(y, 0)^gamma
 * A NULL parameter pointer makes its stage the identity (all four NULL: out = rgb); its gradient pointer must then be NULL as well.
 * pixel_coords may be NULL only when vignetting is NULL.
 * The backward pass recomputes the forward from rgb (nothing is saved) and writes grad_rgb (NULL: not wanted) and the gradients of the
 * four RAW parameter rows (each NULL or the row), with the chain rule through softplus, sigmoid and the homography construction done
 * here; the rows of the cross product that gave the homography's scale are treated as fixed.  Conventions at the kinks:
 *   vignetting clamp  gradient reaches the five parameters where 0 <= p <= 1, inclusive (p = 1 exactly at the zero initialisation)
 *   response curve    a channel whose input to the curve is <= 0 or >= 1 passes no gradient, neither to rgb nor to its four parameters
 * partials: grut_ppisp_partials(P) floats of scratch that belong to the caller; nothing has to be zeroed.  No atomics: two runs on the
 * same input are bitwise equal.  No allocation, no synchronisation, every launch on `stream`. */
uint32_t grut_ppisp_partials(uint32_t num_pixels);
int grut_ppisp_forward(void* stream, uint32_t num_pixels, const float* rgb, const float* pixel_coords, float res_w, float res_h,
                       const float* exposure, const float* color, const float* vignetting, const float* crf, float* out);
int grut_ppisp_backward(void* stream, uint32_t num_pixels, const float* rgb, const float* pixel_coords, float res_w, float res_h,
                        const float* exposure, const float* color, const float* vignetting, const float* crf, const float* grad_out,
                        float* grad_rgb, float* grad_exposure, float* grad_color, float* grad_vignetting, float* grad_crf, float* partials);

/* ---- PPISP controller (3dgrut_amd/ppisp.py: _PPISPController) ------------------------------------------------------------------ */
/* The per-camera network that predicts a frame's exposure and eight colour latents from the rendered image, all fp32:
 *   hdr [h, w, 3] -> conv1x1 3->16 + bias -> max over non-overlapping 3x3 windows (dsH = h / 3, dsW = w / 3; remainder rows and columns
 *   are dropped) -> ReLU -> conv1x1 16->32 + bias -> ReLU -> conv1x1 32->64 + bias -> adaptive average pool to 5x5 (cell g covers
 *   [floor(g ds / 5), ceil((g + 1) ds / 5)) in each direction) -> feat[c * 25 + cell] ++ prior -> three Linear + ReLU 1601->128->128->128
 *   -> exposure head 128->1 and colour head 128->8.
 * weights: HOST array of 16 DEVICE pointers, each the contiguous [out][in] tensor as the module holds it, in the order
 *   conv1 w, b; conv2 w, b; conv3 w, b; trunk0 w, b; trunk1 w, b; trunk2 w, b; exposure w, b; colour w, b.
 *   They are read at every launch: nothing is flattened or cached between calls.  grads: the same array of 16 pointers to write.
 * prior: DEVICE pointer to one float, read on the device (NULL: 0).  out[9]: exposure, then the colour latents.
 * saved: NULL, or GRUT_PPISP_CONTROLLER_SAVED floats the forward writes for the backward: the 1600 pooled features, then the three
 *   post-ReLU trunk activations.  A forward with saved == NULL gives the same bits in `out`.
 * scratch: grut_ppisp_controller_{forward,backward}_scratch(h, w) floats that belong to the caller (host arithmetic; 0 for a shape that
 *   is not taken); nothing has to be zeroed.
 * The backward reads grad_out[9] from device memory and writes all 16 gradient tensors completely; the CNN part is recomputed from hdr.
 * There is no gradient for hdr or prior.  A max-pool tie sends its gradient to the first maximum in row-major order within the window;
 * a ReLU passes gradient where its input is > 0.
 * No allocation, no synchronisation, no atomics: the order of every sum depends on (h, w) only, two calls on the same input are bitwise
 * equal.  h < 3, w < 3, h or w above 16384 or a NULL among the required pointers is GRUT_ERR_BAD_INPUT before any HIP call. */
#define GRUT_PPISP_CONTROLLER_SAVED 1984
uint64_t grut_ppisp_controller_forward_scratch(int h, int w);
uint64_t grut_ppisp_controller_backward_scratch(int h, int w);
int grut_ppisp_controller_forward(void* stream, int h, int w, const float* hdr, const float* prior, const float* const* weights,
                                  float* scratch, float* saved, float* out);
int grut_ppisp_controller_backward(void* stream, int h, int w, const float* hdr, const float* prior, const float* const* weights,
                                   const float* saved, const float* grad_out, float* scratch, float* const* grads);

/* ---- NHT decoder network (threedgrut/model/feature_decoder.py: tinycudann's NetworkWithInputEncoding) -------------------------- */
/* The network that turns a pixel's rendered features and ray direction into colour (model.feature_type: nht), forward only, as one
 * fused pass: encoding, every layer and the output activation, the activations never leaving registers.  The model, which is THIS
 * project's statement of what the reference's call surface leaves open:
 *   input   [P, F + 3] contiguous fp32 DEVICE rows: F feature columns, then u = (dir * sh_scale + 1) / 2
 *   encoding  columns 0 .. F-1 pass through; d = 2 u - 1 = (x, y, z), NOT normalised; the first L^2 (L = sh_degree, 1..4) of the real
 *           SH polynomials, written for general d:
 *             0.28209479177387814              -0.48860251190291987 y            0.48860251190291987 z          -0.48860251190291987 x
 *             1.0925484305920792 xy            -1.0925484305920792 yz            0.94617469575755997 z^2 - 0.31539156525251999
 *             -1.0925484305920792 xz           0.54627421529603959 (x^2 - y^2)   0.59004358992664352 y(-3x^2 + y^2)
 *             2.8906114426405538 xyz           0.45704579946446572 y(1 - 5z^2)   0.3731763325901154 z(5z^2 - 3)
 *             0.45704579946446572 x(1 - 5z^2)  1.4453057213202769 z(x^2 - y^2)   0.59004358992664352 x(-x^2 + 3y^2)
 *           the width F + L^2 is padded with ONES to the next multiple of 16, K0 (a learnable first-layer bias when there is padding)
 *   network n_hidden_layers layers of `width` neurons with ReLU, then an output layer; no biases; output activation GRUT_MLP_ACT_*
 *   params  one flat fp32 array, the matrices in layer order, each row-major [out][in]: width x K0, (n_hidden_layers - 1) times
 *           width x width, then 16 x width of which rows >= n_output_dims are never read
 *   precision  the weights, the encoded input and every hidden activation after its ReLU are rounded to bf16 (nearest even); every sum
 *           is fp32; the output layer's sum goes through its activation in fp32
 *   out     [P, n_output_dims] contiguous fp32
 * grut_mlp_forward takes width 64 or 128, K0 <= 128, 1 <= n_output_dims <= 16 and a configuration whose weight image fits into one
 * workgroup's LDS: grut_mlp_lds_bytes returns the image's size in bytes, or 0 when it does not fit or the configuration is not taken;
 * anything else is GRUT_ERR_BAD_INPUT before anything is launched.  Every workgroup builds the image from `params` (16-byte aligned) at
 * launch: there is no prepared copy of the weights, a change of `params` by any means is seen by the next call.  No atomics: two calls
 * on the same input are bitwise equal.  No allocation, no synchronisation, one launch on `stream`.
 * grut_mlp_num_params: the length of `params` (0 for a configuration that is not taken). */
enum { GRUT_MLP_ACT_NONE = 0, GRUT_MLP_ACT_RELU = 1, GRUT_MLP_ACT_SIGMOID = 2 };
typedef struct GrutMlpConfig {
    int32_t n_features;          /* F */
    int32_t sh_degree;           /* L: L^2 SH values */
    int32_t n_hidden_layers;
    int32_t width;
    int32_t n_output_dims;
    int32_t output_activation;   /* GRUT_MLP_ACT_* */
} GrutMlpConfig;
uint32_t grut_mlp_num_params(const GrutMlpConfig* config);
uint32_t grut_mlp_lds_bytes(const GrutMlpConfig* config);
int grut_mlp_forward(void* stream, const GrutMlpConfig* config, const float* params, const float* input, uint32_t num_pixels, float* out);

/* The backward of grut_mlp_forward, fused: from the saved input rows, the LIVE `params` and grad_out [P, n_output_dims] to
 * grad_input [P, F + 3] and grad_params [grut_mlp_num_params]; either may be NULL (then it is not computed), both NULL is
 * GRUT_ERR_BAD_INPUT.  This project's rules:
 *   recomputation  the forward is computed again from input and params with the forward's rounding points (bf16 nearest even for the
 *           weights, the encoded input and the post-ReLU hidden activations; fp32 sums).  No forward intermediate is kept between the two
 *           calls, and `params` is read afresh at every launch: nothing derived from the weights is cached anywhere.
 *   gates   a hidden ReLU passes gradient where its recomputed pre-activation is > 0 (read off the rounded activation: non-zero; the two
 *           differ only for a pre-activation below bf16's smallest subnormal).  The output activation's derivative is fp32 from the
 *           recomputed output: y (1 - y) for sigmoid, z > 0 for ReLU, 1 for none.
 *   dZ      the gradient with respect to a layer's pre-activation, after its gate or activation derivative, is rounded ONCE to bf16
 *           (nearest even) before it enters any product; the data gradient W^T dZ and the weight gradient dZ H^T use that same rounded dZ,
 *           and H is the very rounded operand of the recomputed forward.
 *   sums    every sum is fp32; the SH Jacobian, the factor 2 of d = 2 u - 1 and grad_input are fp32; the forward's bf16 roundings are
 *           straight-through.
 *   outputs grad_params is written completely: rows >= n_output_dims of the output matrix get +0.0, the ones-padded columns of the first
 *           matrix their real gradient (they are the learnable bias).  Nothing has to be zeroed by the caller.
 *   order   no atomics.  Every workgroup sums its pixels (steps of 128, workgroup b takes steps b, b + grid, ..) in registers and writes one
 *           partial of grad_params to `scratch`; a second kernel sums the partials in workgroup order.  The grid is
 *           min(ceil(P / 128), compute units, 256), so the order depends on (config, P, device) only: two calls are bitwise equal, and
 *           grad_input does not depend on whether grad_params is asked for.
 *   memory  `scratch` (needed only with grad_params): grut_mlp_backward_scratch_bytes(config, P) = min(ceil(P / 128), 256) partials of
 *           grut_mlp_num_params floats, whatever the device; bounded independently of P, no per-pixel data.  No allocation and no
 *           synchronisation inside the call; two launches on `stream`.
 * grut_mlp_backward_lds_bytes: the kernel's LDS (the forward's image plus two staged tiles of 128 pixels x max(width, K0 rounded up to 32)
 * bf16), or 0 for a configuration the backward does not take: one the forward does not take, more than 5 hidden layers, or an image that
 * leaves no room for the tiles within 160 KiB (3 layers of 128 with K0 > 96; 5 layers of 128).  grut_mlp_backward on such a configuration,
 * with unaligned `params` or with num_pixels == 0 is GRUT_ERR_BAD_INPUT before anything is launched. */
uint32_t grut_mlp_backward_lds_bytes(const GrutMlpConfig* config);
size_t grut_mlp_backward_scratch_bytes(const GrutMlpConfig* config, uint32_t num_pixels);
int grut_mlp_backward(void* stream, const GrutMlpConfig* config, const float* params, const float* input, const float* grad_out,
                      uint32_t num_pixels, void* scratch, float* grad_input, float* grad_params);

/* The decode stage around that network (threedgrut/utils/render.py: apply_feature_decoder, and FeatureDecoder._process of
 * threedgrut/model/feature_decoder.py) in the SAME pass: the kernel of grut_mlp_forward with another input source.  No [P, F + 3] rows exist.
 *   inputs  P = num_views * pixels_per_view < 2^32 pixels, all contiguous fp32 DEVICE:
 *             features [P, F]   alpha [P] (may be NULL)   rays_dir [P, 3] camera space (NULL only with center_ray)
 *             rot [num_views, 9] row-major T_to_world[:, :3, :3]
 *   direction  of a pixel of view b = pixel / pixels_per_view: w = R_b d_cam (fp32 sums, contraction free), or with center_ray column 2 of
 *           R_b; n = w / max(|w|, 1e-12) with a correctly rounded square root and IEEE divisions (no reciprocal);
 *           u = (n * sh_scale + 1) * 0.5; the network sees d = 2 u - 1 as grut_mlp_forward does.  One device function for the forward and
 *           the backward's recomputation.
 *   unpremultiply_alpha  (needs alpha) a_s = max(alpha, 1e-8f); the network's feature columns are features / a_s (IEEE division, before
 *           the bf16 rounding of the encoded input), the result is y * a_s.  Without the flag alpha is not read.
 *   network everything from the encoded input on is grut_mlp_forward's contract and its code: rounding points, layer order, activation.
 *           On inputs where every direction operation is exact, the result equals grut_mlp_forward on the assembled rows bit for bit.
 *   out     [P, n_output_dims]
 * One launch; no allocation, no synchronisation, no atomics; `params` is read live at every launch.  The configurations of grut_mlp_forward;
 * anything else, a missing pointer or P >= 2^32 is GRUT_ERR_BAD_INPUT before a launch. */
typedef struct GrutDecodeConfig {
    GrutMlpConfig mlp;
    float sh_scale;
    int32_t unpremultiply_alpha;
    int32_t center_ray;
} GrutDecodeConfig;
int grut_decode_forward(void* stream, const GrutDecodeConfig* config, const float* params, const float* features, const float* alpha,
                        const float* rays_dir, const float* rot, uint32_t num_views, uint32_t pixels_per_view, float* out);

/* The backward of grut_decode_forward: the kernel of grut_mlp_backward with that input source and another gradient sink.  Each of
 * grad_features [P, F], grad_alpha [P] and grad_params may be NULL; all NULL, or grad_alpha without unpremultiply_alpha, is
 * GRUT_ERR_BAD_INPUT.  Rays and poses get no gradient.  The rules of grut_mlp_backward, and:
 *   upstream  the network's upstream gradient is grad_out * a_s with unpremultiply_alpha (formed first; the activation's derivative is
 *           applied to that product), otherwise grad_out.
 *   gx      the fp32 gradient of the network's feature columns; the SH Jacobian is not evaluated.
 *           grad_features = gx / a_s (IEEE division) with unpremultiply_alpha, otherwise gx.
 *   grad_alpha = [alpha >= 1e-8f] * (sum_c grad_out_c y_c - (sum_j gx_j x_j) / a_s), fp32: x_j = features_j / a_s, the fp32 feature column
 *           before its bf16 rounding; y the recomputed fp32 output after its activation (before the product with a_s).  Both sums start
 *           from 0 and add one product at a time (possibly fused), j = 0 .. F - 1 ascending, then c = 0 .. n_output_dims - 1 ascending.
 *           The gate is inclusive, as the gradient of torch.clamp is; where it is closed the result is +0.0.
 *   order   grid, partials, reduction order and scratch of grut_mlp_backward (grut_mlp_backward_scratch_bytes and
 *           grut_mlp_backward_lds_bytes apply as they are): two calls are bitwise equal, and grad_features and grad_alpha do not depend on
 *           whether grad_params is asked for. */
int grut_decode_backward(void* stream, const GrutDecodeConfig* config, const float* params, const float* features, const float* alpha,
                         const float* rays_dir, const float* rot, uint32_t num_views, uint32_t pixels_per_view, const float* grad_out,
                         void* scratch, float* grad_features, float* grad_alpha, float* grad_params);

/* ---- nearest-neighbour initialisation (threedgrut/model/geometry.py) ----------------------------------------------- */
/* Exact k nearest neighbours in 3-D, the device side of what the reference's initialisation takes from sklearn.neighbors:
 * k_nearest_neighbors (geometry.py:42-49, called at model.py:732 for the Gaussians' initial size), nearest_neighbors (geometry.py:52-73)
 * and nearest_neighbor_dist_cpuKD (geometry.py:76-117, called at model.py:588 and :728).  points [num_points,3] and queries
 * [num_queries,3] are contiguous fp32 DEVICE tensors; queries = NULL (num_queries is then ignored): every point queries the set it
 * belongs to.  1 <= k <= 16, num_points and num_queries < 2^31.
 * Selection: the k points with the smallest fp32 key (dx dx + dy dy) + dz dz, dx = q.x - p.x rounded to fp32 (contracted or not), ties
 * broken by the LOWER point index - a total order, so the result does not depend on the order in which the search visits the points and
 * is bitwise reproducible.  exclude_self (only with queries = NULL) removes the query's own INDEX from its candidates (coincident other
 * points remain).  Reported: out_dist [Q,k] in the order of the key (ascending; where two keys differ only by their rounding, the
 * distances may be out of order by as little) (NULL: not wanted), for the selected points recomputed in double from the fp32
 * coordinates and rounded once, (float)sqrt(dx dx + dy dy + dz dz) - the number sklearn's float64 search returns after the cast of
 * geometry.py:49; out_index [Q,k] int32 original point indices in the same order (NULL: not wanted; not both NULL).
 * out_nonfinite [1] (device) receives the number of NaN / inf coordinates among points and queries; when it is not 0 the outputs are
 * unspecified (every access stays in bounds).  scratch: grut_knn_scratch_bytes(num_points, num_queries) bytes (num_queries = 0: self
 * query), 16-byte aligned, contents arbitrary - nothing relies on zeroed scratch.  No allocation, no synchronisation, every launch on
 * `stream`.  k > 16, k > num_points - exclude_self, exclude_self with queries, a missing pointer or a short scratch: GRUT_ERR_BAD_INPUT
 * before anything is launched. */
size_t grut_knn_scratch_bytes(uint32_t num_points, uint32_t num_queries);
int grut_knn(void* stream, uint32_t num_points, const float* points, uint32_t num_queries, const float* queries, int k, int exclude_self,
             float* out_dist, int32_t* out_index, void* scratch, size_t scratch_bytes, uint32_t* out_nonfinite);

/* ---- optimizer step --------------------------------------- */
/* One parameter group of SelectiveAdam (threedgrut/optimizers/__init__.py:85-124): contiguous fp32 [num_rows, row_width]
 * DEVICE tensors, 16-byte aligned. */
typedef struct GrutAdamGroup {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint32_t row_width;
    float lr, beta1, beta2, eps;
} GrutAdamGroup;
enum { GRUT_VIS_NONE = 0,        /* every row is updated */
       GRUT_VIS_BOOL_U8 = 1,     /* visibility = bool[num_rows] (what `visibility.bool().squeeze()` yields) */
       GRUT_VIS_INT32 = 2,       /* visibility = int32[num_rows], visible iff != 0 (gut_forward's out_visibility) */
       GRUT_VIS_FLOAT_BITS = 3   /* visibility = float[num_rows], visible iff != 0.0f (the tracers' `mog_visibility`) */ };
/* Replaces selective_adam_update_launch (threedgrut/optimizers/optimizers.cu:79-109, kernel :49-77), for ALL groups in
 * one launch: rows whose flag is zero keep parameter and moments; visible rows get
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g g; param -= lr m / (sqrt(v) + eps)   (no bias correction, as the reference). */
int grut_selective_adam_update(void* stream, const GrutAdamGroup* groups, int num_groups, uint32_t num_rows,
                               const void* visibility, int visibility_kind);

/* One tensor of the dense Adam update: what torch.optim.Adam(fused=True) keeps per parameter.  param / grad / exp_avg / exp_avg_sq
 * are contiguous fp32 DEVICE arrays of `numel` elements with 16-byte aligned bases; `step` is the DEVICE fp32 scalar torch keeps with
 * fused=True.  Hyper-parameters travel as double, as torch hands them to its kernel. */
typedef struct GrutDenseAdamGroup {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    uint64_t numel;
    double lr, beta1, beta2, eps, weight_decay;
} GrutDenseAdamGroup;
/* torch's fused Adam (no amsgrad, no maximize, no grad scaler, weight decay coupled) over ALL groups in one launch.  Statement order and
 * roundings of adam_math / FusedAdamMathFunctor (ATen/native/hip/fused_adam_utils.cuh), fp32 tensors:
 *   step += 1 (fp32);  bc1 = (float)(1 - pow(beta1, step)),  bc2s = (float)sqrt(1 - pow(beta2, step))   (pow and sqrt in double)
 *   g = (float)(g + p * weight_decay) when weight_decay != 0 (double);
 *   m = (float)(beta1 m + (1 - beta1) g);  v = (float)(beta2 v + (1 - beta2) g g)                     (double, one rounding each)
 *   step_size = (float)(lr / bc1) (double division);  denom = (float)(sqrtf(v) / bc2s + eps) (fp32 sqrt and division, double addition)
 *   p -= step_size * m / denom                                                                          (fp32, correctly rounded)
 * A prologue launch of one thread per group increments `step` and leaves {step_size, bc2s} of group i in scratch[2 i], scratch[2 i + 1]
 * (bc1 is used by step_size alone, so the quotient is stored in its place); the streaming launch reads the two floats and never
 * touches `step`, so no workgroup races with the increment.  scratch: [num_groups, 2] fp32 DEVICE, contents arbitrary before and
 * unspecified after.  A group with numel == 0 is skipped and its `step` stays.  Two launches per batch of 8 non-empty groups, no
 * atomics (equal inputs give equal bits), no allocation, no synchronisation, every launch on `stream`.
 * GRUT_ERR_BAD_INPUT before any HIP call: groups NULL with num_groups > 0, num_groups < 0, scratch NULL, and for a group with
 * numel > 0 a NULL pointer or a tensor base that is not 16-byte aligned. */
int grut_adam_update(void* stream, const GrutDenseAdamGroup* groups, int num_groups, float* scratch);

/* human-readable text of the last error raised on the calling thread */
const char* grut_last_error(void);
/* ABI version; bumped whenever a struct above changes */
int grut_abi_version(void);

/* Scratch memory.  Every per-frame buffer of the two renderers is grow-only device scratch (the role of the reference's CudaBuffer,
 * src/cudaBuffer.cpp:44-60, which calls cudaMalloc / cudaFree).  By default it comes from hipMalloc / hipFree; a host that has its own
 * device allocator — PyTorch's caching allocator in the plugins — installs it here BEFORE creating handles: alloc_fn returns device
 * memory usable on the stream of the API call it is made from (NULL = failure), free_fn takes it back.  Process-wide; NULL, NULL
 * restores hipMalloc.  gut_trim / grt_trim release everything a handle holds (the handle stays valid; 3DGRT needs its BVH rebuilt). */
typedef void* (*GrutAllocFn)(void* user, uint64_t bytes);
typedef void  (*GrutFreeFn)(void* user, void* ptr);
int grut_set_allocator(GrutAllocFn alloc_fn, GrutFreeFn free_fn, void* user);

#ifdef __cplusplus
}
#endif
#endif /* GRUT_AMD_H */
