/*
 * naruto_hip.h -- C ABI of libnaruto_hip.so: NARUTO's neural-implicit mapping / uncertainty hot path
 * (Co-SLAM-derived joint hash grid + OneBlob + two tiny MLPs, SDF-weighted compositing, uncertainty
 * aggregation, mapping losses) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference has no FFI: its seam is the Python attribute surface of one nn.Module
 * (reference src/slam/coslam/coslam.py:65).  Each entry point below names
 * the reference code it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer to fp32 data unless it says "host";
 *   - nothing here allocates, frees, synchronises or throws; work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream);
 *   - return value 0 = ok, negative = error (naruto_last_error() gives the text);
 *   - gradients are ACCUMULATED (+=) into the buffers of NarutoGrads, so the caller zeroes them
 *     (this is what torch's .grad accumulation needs, reference coslam.py:368-399);
 *   - a NarutoField handle is immutable after creation and may be shared by streams/threads.
 *
 * This file is the ONE statement of the ABI: naruto_amd/_lib.py reads it at import and derives its ctypes structures, constants and
 * argument types from the declarations below, and refuses what it cannot read.  So the declarations stay plain: `typedef struct X { ... } X;`
 * of fixed-width scalars, pointers and arrays; `#define NARUTO_X <integer literal>`; one prototype per function.  A parameter that
 * is a HOST pointer carries NARUTO_HOST (the macro is empty): the binding types it POINTER(<its scalar>), so that ctypes converts
 * arrays and passes a bare scalar by reference; every unmarked pointer is an address (c_void_p), or POINTER(<struct>) for the
 * structs declared here.
 */
#ifndef NARUTO_HIP_H
#define NARUTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NARUTO_HOST                   /* marks a parameter that points to HOST memory (see above) */
#define NARUTO_MAX_LEVELS 16
#define NARUTO_OK 0
#define NARUTO_ERR_INVALID (-22)      /* bad argument / unsupported configuration */
#define NARUTO_ERR_LAUNCH (-5)        /* HIP launch failure */

typedef struct NarutoField NarutoField;

/* Static description of the scene representation (reference: JointEncodingNaruto.__init__,
 * scene_rep.py:26-36; Co-SLAM get_encoder / tcnn HashGrid config; decoder.py:82-97). */
typedef struct NarutoFieldDesc {
    uint32_t n_levels;            /* tcnn n_levels; this build supports 16                      */
    uint32_t n_features;          /* tcnn n_features_per_level; this build supports 2           */
    uint32_t log2_hashmap_size;   /* config grid.hash_size; 4 .. 24                              */
    uint32_t base_resolution;     /* 16                                                         */
    float    per_level_scale;     /* exp2(log2(desired_res / base_res) / (n_levels-1))           */
    uint32_t n_bins;              /* OneBlob bins per input dim; this build supports 16          */
    uint32_t hidden_dim;          /* SDF net hidden width; this build supports 32                */
    uint32_t geo_feat_dim;        /* this build supports 15                                      */
    uint32_t hidden_dim_color;    /* this build supports 32                                      */
    uint32_t uncert_dims[3];      /* uncertainty voxel grid [Nx,Ny,Nz] (scene_rep.py:49-56)      */
    float    bbox_min[3];         /* config mapping.bound[:,0]                                   */
    float    bbox_max[3];         /* config mapping.bound[:,1]                                   */
    float    trunc;               /* training.trunc                                              */
    float    sc_factor;           /* data.sc_factor                                              */
    int32_t  white_bkgd;          /* training.white_bkgd                                         */
    uint32_t mlp_mode;            /* NARUTO_MLP_FP32 (exact fp32 MFMA chain: the parity mode) or
                                     NARUTO_MLP_BF16 (bf16 operands, fp32 accumulate, on v_mfma_f32_32x32x16_bf16: the
                                     speed mode; the reference's counterpart is its half-precision tcnn FullyFusedMLP
                                     option, decoder.py:43-59)                                  */
} NarutoFieldDesc;
#define NARUTO_MLP_FP32 0u
#define NARUTO_MLP_BF16 1u

/* Learnable parameters, in the reference's own layouts (state_dict tensors):
 *   table        embed_fn.params                         [n_entries * 2]
 *   uncert_grid  uncert_grid                             [Nx, Ny, Nz]
 *   sdf_w0       decoder.sdf_net.model.0.weight          [32, 80]  (in = 32 hash feats ++ 48 OneBlob)
 *   sdf_w1       decoder.sdf_net.model.2.weight          [16, 32]  (out = sdf ++ 15 geo feats)
 *   col_w0       decoder.color_net.model.0.weight        [32, 63]  (in = 48 OneBlob ++ 15 geo feats)
 *   col_w1       decoder.color_net.model.2.weight        [3, 32]                                   */
typedef struct NarutoParams {
    const float* table;
    const float* uncert_grid;
    const float* sdf_w0;
    const float* sdf_w1;
    const float* col_w0;
    const float* col_w1;
} NarutoParams;

typedef struct NarutoGrads {       /* same shapes; any pointer may be NULL = "not needed" */
    float* table;
    float* uncert_grid;
    float* sdf_w0;
    float* sdf_w1;
    float* col_w0;
    float* col_w1;
} NarutoGrads;

/* Where the M query points come from.  Either x != NULL: already-normalised points [M,3]
 * (query_sdf / query_color_sdf, scene_rep.py:98-148), or rays: M = n_rays * n_samples points
 * o + d * z, normalised by the bounding box (run_network [Co-SLAM], called at scene_rep.py:183-184). */
typedef struct NarutoPoints {
    const float* x;          /* [M,3] or NULL            */
    const float* rays_o;     /* [n_rays,3]               */
    const float* rays_d;     /* [n_rays,3]               */
    const float* z_vals;     /* [n_rays,n_samples]       */
    uint32_t     n_samples;
} NarutoPoints;

const char* naruto_last_error(void);
int naruto_version(void);

int  naruto_field_create(const NarutoFieldDesc* desc, NARUTO_HOST NarutoField** out);
void naruto_field_destroy(NarutoField* f);
/* Level tables the library derived (tcnn GridEncodingTemplated constructor): host arrays of
 * n_levels (scale, resolution, size) and n_levels+1 (offset, in entries). */
int  naruto_field_levels(const NarutoField* f, NARUTO_HOST float* scale, NARUTO_HOST uint32_t* resolution, NARUTO_HOST uint32_t* size,
                          NARUTO_HOST uint32_t* offset);
uint64_t naruto_field_n_entries(const NarutoField* f);

/* A1 -- depth sampling, scene_rep.py:158-180.  target_d may be NULL (then n_samples uniform depths,
 * scene_rep.py:171-173); rand [n_rays,S] may be NULL (perturb == 0).  S = n_samples_d + n_range_d
 * (or n_range_d if n_samples_d == 0, or n_samples if target_d == NULL).  z_vals [n_rays,S]. */
int naruto_sample_z(uint32_t n_rays, const float* target_d, float near_, float far_, uint32_t n_samples_d,
                    uint32_t n_range_d, float range_d, uint32_t n_samples, const float* rand,
                    float* z_vals, void* stream);

/* A3 alone -- embed_fn(x): query_sdf(embed=True), scene_rep.py:109-111.  feat [M,32] level-major. */
int naruto_hash_encode_fwd(const NarutoField* f, uint32_t M, const float* x, const float* table,
                           float* feat, void* stream);
/* its backward (tcnn HashGrid backward): d_table += scatter(d_feat).
 * workspace: naruto_scatter_workspace(f, M) bytes for lists of up to M points (per-split partial tables of the LDS-tiled
 * scatter; count matrix + 12-byte (corner, contribution) items of the binned scatter that serves levels of more than 2^17
 * entries).  No level uses global float atomics: the result is bitwise reproducible for any log2_hashmap_size <= 24.
 * naruto_field_scatter_overwrites(f): 1 if the scatter can WRITE the table gradient (NARUTO_BWD_OVERWRITE_TABLE_GRAD, the
 * fused optimiser) -- always, unless the debug switch NARUTO_DEBUG_SCATTER_ATOMIC sent the large levels through global atomics. */
size_t naruto_scatter_workspace(const NarutoField* f, uint32_t M);
int naruto_field_scatter_overwrites(const NarutoField* f);
int naruto_hash_encode_bwd(const NarutoField* f, uint32_t M, const float* x, const float* d_feat,
                           const float* d_feat_scale /* device scalar multiplying d_feat, or NULL */,
                           float* d_table, void* workspace, void* stream);

/* Feature-grid smoothness term of the mapping loss -- Co-SLAM CoSLAM.smoothness [not in tree], called by
 * get_loss_from_ret (coslam.py:166-169): TV of the hash features on a (sample_points-1)^3 lattice placed
 * at a random offset.  rand6 (device) = offset_rand[3] ++ jitter_rand[3] in [0,1).  Outputs: loss [1],
 * x_out [n^3,3] (the normalised lattice points) and d_feat [n^3,32] = d(loss)/d(features), which
 * naruto_hash_encode_bwd(x_out, d_feat, d_feat_scale = cotangent of the loss) turns into the table gradient. */
size_t naruto_smoothness_workspace(uint32_t sample_points);
int naruto_smoothness_fwd(const NarutoField* f, const float* table, uint32_t sample_points, float voxel_size,
                          float margin, const float* rand6, float* x_out, float* d_feat, float* loss,
                          void* workspace, void* stream);

/* A2-A5 fused -- calc_embedding + embedpos_fn + decoder (scene_rep.py:58-64,132-148, decoder.py:29-41,
 * 99-116).  Outputs (any may be NULL):
 *   raw        [M,5]  (r,g,b pre-sigmoid, sdf, uncert_raw)            -- query_color_sdf / run_network
 *   sdf_uncert [M,2]  (sdf, uncert_raw); colour net skipped when raw==NULL -- query_sdf(return_uncert)
 *   geo        [M,15]                                                  -- query_sdf(return_geo)
 *   feat_save  [16,M,2] hash features kept for naruto_query_bwd (training only)                    */
int naruto_query_fwd(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts,
                     float* raw, float* sdf_uncert, float* geo, float* feat_save, void* stream);

/* Backward of naruto_query_fwd (autograd of the above through nn.Linear / tcnn / grid_sample).
 * d_raw [M,5] required; d_geo [M,15] optional (NULL = 0).  feat_save from the forward call.
 * active_idx / n_active (both NULL, or both given): a list of the point indices to process and its length in
 * DEVICE memory -- every point NOT in the list must have an all-zero cotangent (see naruto_compact_active).
 * workspace: naruto_query_bwd_workspace(M) bytes, contents undefined on entry and exit.
 * extra (optional): E more points whose feature cotangents are already known (the smoothness lattice of
 * naruto_smoothness_fwd); they are appended to the scatter's point list so that ONE scatter pass produces the
 * whole table gradient.  flags: NARUTO_BWD_OVERWRITE_* make the reductions WRITE the weight / table gradients
 * instead of accumulating (saves the caller the zero fill).
 * Workspace: naruto_query_bwd_workspace(f, M + E). */
typedef struct NarutoExtraPoints {
    const float* x;        /* [E,3] normalised points                         */
    const float* d_feat;   /* [E,32] cotangent of their hash features         */
    const float* scale;    /* device scalar multiplying d_feat, or NULL (= 1)  */
    uint32_t     n;        /* E                                               */
} NarutoExtraPoints;
#define NARUTO_BWD_OVERWRITE_WEIGHT_GRADS 1u
#define NARUTO_BWD_OVERWRITE_TABLE_GRAD 2u
/* naruto_train_backward in two calls (data parallel: the small MLP-gradient bucket is all-reduced while the table scatter runs):
 * MLP_ONLY = loss backward, compaction, MLP backward, weight gradients (complete after this call); TABLE_ONLY = the table scatter
 * over the point list the MLP_ONLY call left in the workspace.  Not with the fused optimiser. */
#define NARUTO_TRAIN_BWD_MLP_ONLY 4u
#define NARUTO_TRAIN_BWD_TABLE_ONLY 8u
/* Forward and backward issued back to back (single process): naruto_train_forward(finalize = NARUTO_TRAIN_FWD_DEFER_TAIL) stops
 * after the loss stage, and naruto_train_backward(flags | NARUTO_TRAIN_BWD_DEFERRED_TAIL) starts with ONE launch that is the loss
 * tail (one workgroup: losses[10], the iteration counter), the composite backward and the compaction -- instead of three.
 * losses / sums are then valid after the BACKWARD call.  Both must be given together; above 4096 rays both calls run the
 * ordinary sequence (same results). */
#define NARUTO_TRAIN_FWD_DEFER_TAIL 2
#define NARUTO_TRAIN_BWD_DEFERRED_TAIL 16u
/* Data parallel counterpart: the forward ran with finalize = 0 and t->sums now holds the ALL-REDUCED sums.  The backward (one piece
 * or its MLP_ONLY phase) then replaces naruto_train_finalize | composite backward | compaction by the same single launch, whose
 * extra workgroup turns the sums into losses[0..7] and the total.  Do not call naruto_train_finalize in addition. */
#define NARUTO_TRAIN_BWD_SUMS_GIVEN 32u
/* ... and its five-launch form (round 5): naruto_train_forward(finalize = NARUTO_TRAIN_FWD_SUMS_TV_LATER) stops at this rank's sums like
 * finalize = 0, but where the launch plan allows it the forward samples its own depths and only ENCODES the smoothness lattice (no
 * k_sample_encode launch); naruto_train_backward(NARUTO_TRAIN_BWD_SUMS_GIVEN | NARUTO_TRAIN_BWD_TV_MOVED) then evaluates the term in its
 * first launch and adds its value to losses[8] / losses[9] at its end.  losses[8] is 0 in between.  Both must be given together. */
#define NARUTO_TRAIN_FWD_SUMS_TV_LATER 3
#define NARUTO_TRAIN_BWD_TV_MOVED 64u
/* The model's sub-modules called on their own (forward only; the query entry points above never need them -- they evaluate all of
 * this in registers).  naruto_oneblob_fwd = embedpos_fn(x) (tcnn OneBlob, 16 bins): x [M,3] -> out [M,48].
 * naruto_decoder_fwd, by `part`:
 *   NARUTO_DECODER_FULL      decoder(embed, embed_pos) (decoder.py:99-116):  a = embed [M,33] (channel 0 = uncertainty sample, 1..32 =
 *                            hash features), b = embed_pos [M,48] -> out [M,5] = (rgb pre-sigmoid, sdf, the uncertainty channel)
 *   NARUTO_DECODER_SDF_NET   sdf_net(cat(embed, embed_pos)) (decoder.py:29-41): a = [M,81], b unused -> out [M,17] = (sdf, geo15, uncertainty)
 *   NARUTO_DECODER_COLOR_NET color_net(cat(embed_pos, geo)):                    a = [M,63], b unused -> out [M,3] (pre-sigmoid)          */
#define NARUTO_DECODER_FULL 0
#define NARUTO_DECODER_SDF_NET 1
#define NARUTO_DECODER_COLOR_NET 2
int naruto_oneblob_fwd(const NarutoField* f, uint32_t M, const float* x, float* out, void* stream);
/* calc_embedding's channel 0 on its own (scene_rep.py:58-64): out[m] = trilinear sample of uncert_grid at the normalised point x[m]
 * (grid_sample semantics of the reference's call: align_corners=False, zero padding, x <-> z transposed).  Forward only. */
int naruto_uncert_sample(const NarutoField* f, uint32_t M, const float* x, const float* uncert_grid, float* out, void* stream);
int naruto_decoder_fwd(const NarutoField* f, const NarutoParams* p, uint32_t M, int part, const float* a, const float* b, float* out, void* stream);
size_t naruto_query_bwd_workspace(const NarutoField* f, uint32_t M);
int naruto_query_bwd(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts,
                     const float* feat_save, const float* d_raw, const float* d_geo,
                     const uint32_t* active_idx, const uint32_t* n_active,
                     const NarutoExtraPoints* extra, uint32_t flags,
                     const NarutoGrads* g, void* workspace, void* stream);

/* Gradient of naruto_query_fwd with respect to its POINTS (autograd of the same forward through x, or through rays_o / rays_d
 * of run_network's p = o + d * z): pose refinement and tracking differentiate the rendering through the rays
 * (global_BA's pose_optim, coslam.py:264-281, 330-347, 378-407; Co-SLAM tracking_render, coslam.py:595-602).  Terms:
 *   hash grid     d feat_l / d x = scale_l * sum_corners (d trilinear weight / d w) * value   (tcnn HashGrid, linear
 *                 interpolation; corner indices are piecewise constant and contribute nothing)   [parity unpinned]
 *   OneBlob       d quartic_cdf / du = 15/16 (1 - u^2)^2 for |u| <= 1, else 0; u = (b - x) * 16, with the +-1 periodic terms
 *                 and the wrapped last bin (tcnn OneBlob)                                           [parity unpinned]
 *   uncertainty   derivative of the trilinear grid_sample in its coordinates, d ix / d x = W etc. (scene_rep.py:58-64:
 *                 align_corners=False, zero padding, x <-> z transposed); reaches raw[...,4] only
 *   MLPs          nn.Linear + ReLU, ReLU'(0) = 0 (decoder.py:29-41, 99-116), evaluated in exact fp32 on the fp32 master
 *                 weights in BOTH MLP modes (in bf16 mode: the gradient of the exact network at the same point)
 *   ray points    run_network's box normalisation [Co-SLAM; called at scene_rep.py:183-184]: d rays_o[r] = sum_s g[r,s] / ext,
 *                 d rays_d[r] = sum_s z[r,s] g[r,s] / ext per axis, g = gradient w.r.t. the normalised point; z_vals are
 *                 constants (scene_rep.py:161-183)
 * d_raw [M,5] required; d_geo [M,15] or NULL (= 0).  active_idx / n_active: both NULL or both given, as naruto_query_bwd
 * (naruto_compact_active); points outside the list contribute zero.  Outputs: x points write d_x [M,3] (normalised space);
 * ray points write d_rays_o and / or d_rays_d [N,3] (N = M / n_samples) and need workspace =
 * naruto_query_bwd_points_workspace(f, M) bytes (x points: NULL allowed).  flags: NARUTO_BWD_POINTS_ACCUMULATE adds into the
 * outputs instead of writing them.  No float atomics: each ray's samples are summed in a fixed order, bitwise reproducible.
 * Parameter gradients are not touched (naruto_query_bwd gives them). */
#define NARUTO_BWD_POINTS_ACCUMULATE 1u
size_t naruto_query_bwd_points_workspace(const NarutoField* f, uint32_t M);
int naruto_query_bwd_points(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts,
                            const float* d_raw, const float* d_geo /* or NULL */,
                            const uint32_t* active_idx, const uint32_t* n_active /* both or neither */,
                            float* d_x /* [M,3] or NULL */, float* d_rays_o, float* d_rays_d /* [N,3] or NULL */,
                            uint32_t flags, void* workspace, void* stream);

/* A1-A7 in ONE launch -- render_rays as an inference call (scene_rep.py:150-225; eval-mode forward, planner-side queries): depth
 * sampling as naruto_sample_z, the field query of naruto_query_fwd and the compositing of naruto_composite_fwd per ray, raw kept
 * in LDS.  Outputs (any may be NULL): rgb [N,3], depth, disp, acc, depth_var, uncert_map [N], weights [N,S], raw [N,S,5],
 * z_vals [N,S] -- the per-sample ones cost their global writes only when asked for.  Sampling arguments as naruto_sample_z
 * (target_d NULL: n_samples uniform depths); rand [N,S] or rng {seed, counter} or neither (no jitter).  Not differentiable:
 * training goes through naruto_train_forward / the autograd operators. */
typedef struct NarutoRender {
    uint32_t n_rays;
    const float *rays_o, *rays_d, *target_d;
    float near_, far_;
    uint32_t n_samples_d, n_range_d;
    float range_d;
    uint32_t n_samples;
    const float* rand;
    const uint64_t* rng;
    float *rgb, *depth, *disp, *acc, *depth_var, *uncert_map, *weights, *raw, *z_vals;
} NarutoRender;
int naruto_render_fwd(const NarutoField* f, const NarutoParams* p, const NarutoRender* r, void* stream);

/* A6+A7 -- sdf2weights [Co-SLAM] + raw2outputs (scene_rep.py:66-96).  Outputs (any may be NULL):
 * rgb [N,3], disp [N], acc [N], weights [N,S], depth [N], depth_var [N], uncert_map [N]. */
int naruto_composite_fwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw,
                         const float* z_vals, float* rgb, float* disp, float* acc, float* weights,
                         float* depth, float* depth_var, float* uncert_map, void* stream);
/* Backward: cotangents of the outputs (any may be NULL = 0) -> d_raw [N,S,5].
 * accumulate != 0 adds into d_raw instead of overwriting it. */
int naruto_composite_bwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw,
                         const float* z_vals, const float* d_rgb, const float* d_disp, const float* d_acc,
                         const float* d_weights, const float* d_depth, const float* d_depth_var,
                         const float* d_uncert_map, float* d_raw, int accumulate, void* stream);

/* A8 -- the mapping losses of JointEncodingNaruto.forward (scene_rep.py:246-285 + Co-SLAM
 * get_sdf_loss/get_masks).  Three steps so that data-parallel ranks can all-reduce the sums in
 * between (the loss weights depend on GLOBAL sample counts):
 *   1. naruto_loss_sums     : this rank's rays -> sums[NARUTO_LOSS_NSUMS] (fp64, device)
 *   2. (optional) all-reduce (SUM) of slots [0, NARUTO_LOSS_SLOT_MINUNCERT) over ranks; slot
 *      NARUTO_LOSS_SLOT_MINUNCERT is a minimum (MIN-reduce it, or keep it per rank: it only feeds an assertion)
 *   3. naruto_loss_finalize : sums (+ total ray count over all ranks) -> losses[8] =
 *      {rgb_loss, depth_loss, sdf_loss, fs_loss, psnr, uncert_loss, min(uncert_map), n_valid_depth}
 * workspace: naruto_loss_workspace(n_rays) bytes. */
#define NARUTO_LOSS_NSUMS 16
#define NARUTO_LOSS_SLOT_MINUNCERT 9
size_t naruto_loss_workspace(uint32_t n_rays);
int naruto_loss_sums(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals,
                     const float* rgb, const float* depth, const float* uncert_map, const float* target_rgb,
                     const float* target_d, float depth_trunc, float rgb_missing, double* sums,
                     float* losses /* optional: single-process shortcut, = finalize(sums, n_rays) */,
                     void* workspace, void* stream);
int naruto_loss_finalize(const double* sums, uint64_t n_rays_total, uint32_t S, float* losses, void* stream);
/* Backward of the whole loss block down to d_raw [N,S,5] (composite backward fused in):
 * loss_grad [6] = d(total)/d{rgb_loss, depth_loss, sdf_loss, fs_loss, psnr(ignored), uncert_loss},
 * device array (e.g. the weights of get_loss_from_ret, coslam.py:154-174). */
int naruto_loss_bwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals,
                    const float* target_rgb, const float* target_d, float depth_trunc, float rgb_missing,
                    const double* sums, uint64_t n_rays_total, const float* loss_grad, float* d_raw,
                    uint32_t* ray_count, void* stream);
/* The mapping losses leave the cotangent of every sample behind the surface band identically zero, and
 * samples are depth-sorted, so the non-zero part of each ray is a PREFIX: naruto_loss_bwd can report its
 * length per ray (ray_count [n_rays], optional), and naruto_compact_active turns the lengths into the
 * flat list naruto_query_bwd consumes: active_idx [<= n_rays*S], n_active [1]; ray_offset [n_rays] scratch. */
int naruto_compact_active(uint32_t n_rays, uint32_t S, const uint32_t* ray_count, uint32_t* ray_offset,
                          uint32_t* active_idx, uint32_t* n_active, void* stream);

/* A10 helper -- one fused Adam step over a flat fp32 buffer (torch.optim.Adam semantics incl. L2
 * weight_decay, reference coslam.py:409-419).  The 1-based step count comes from `step`, or -- when
 * step_dev != NULL -- from device memory (int32), which keeps the launch valid under hipGraph replay. */
int naruto_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n,
                     float lr, float beta1, float beta2, float eps, float weight_decay, uint32_t step,
                     const int32_t* step_dev, void* stream);

/* A9 caller -- get_map_volumes' post-processing (coslam_utils.py:89-95): sdf_uncert [M,2] from
 * naruto_query_fwd -> out [2,M] = (uncertainty volume: softplus(raw)+0.01 where 0 <= sdf < 0.5 else 0 | sdf volume). */
int naruto_map_volumes(uint32_t M, const float* sdf_uncert, float* out, void* stream);

/* N1 ("next" row) -- ActiveRaySampler.sample_rays (reference src/slam/coslam/active_ray_sampler.py:77-149) on the
 * device.  Input batch of n_total rays = [oversampled keyframe rays ..., n_cur current-frame rays]; base =
 * mapping.sample (2048), K = num_uncert_sample (500), n_tail = ceil(n_cur / oversample_mul).  Candidates are rays
 * [base, n_total - n_tail); the K with the SMALLEST cached-uncertainty value at their measured end point
 * (round((o + d*depth - bbox_min) * voxel_scale), clipped; numpy argpartition semantics, ties by lower index) are
 * moved to the front: out = [K selected | rays [0, base-K) | last n_tail rays], base + n_tail rows.
 * uncert_vol [X,Y,Z] fp32 on the device; vol_dims / bbox_min are HOST arrays of 3.
 * workspace: naruto_active_ray_workspace(n_total, K) bytes. */
size_t naruto_active_ray_workspace(uint32_t n_total, uint32_t K);
int naruto_active_ray_select(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o,
                             const float* rays_d, const float* target_s, const float* target_d,
                             const float* uncert_vol, NARUTO_HOST const uint32_t* vol_dims, NARUTO_HOST const float* bbox_min,
                             float voxel_scale, float* out_o, float* out_d, float* out_s, float* out_t,
                             void* workspace, void* stream);

/* naruto_active_ray_select with the candidates' keys given (keys[j] for candidate base + j, as NarutoRayBatch.keys_out leaves them): the
 * lookup -- two dependent trips to memory per candidate -- is skipped.  At most 8 192 candidates (NARUTO_ERR_INVALID beyond). */
int naruto_active_ray_select_keyed(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o,
                                   const float* rays_d, const float* target_s, const float* target_d, const uint32_t* keys,
                                   float* out_o, float* out_d, float* out_s, float* out_t, void* stream);

/* The two selections with one more, optional output: src_rows [base + n_tail] = the input row each output row was taken from (NULL: the
 * calls above).  The selection permutes rows; whatever is known per assembled row (NarutoRayBatch.ids_out: the pose of a ray) follows the
 * rays through it: id of output row r = ids[src_rows[r]]. */
int naruto_active_ray_select_rows(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o,
                                  const float* rays_d, const float* target_s, const float* target_d,
                                  const float* uncert_vol, NARUTO_HOST const uint32_t* vol_dims, NARUTO_HOST const float* bbox_min,
                                  float voxel_scale, float* out_o, float* out_d, float* out_s, float* out_t,
                                  uint32_t* src_rows, void* workspace, void* stream);
int naruto_active_ray_select_keyed_rows(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o,
                                        const float* rays_d, const float* target_s, const float* target_d, const uint32_t* keys,
                                        float* out_o, float* out_d, float* out_s, float* out_t, uint32_t* src_rows, void* stream);

/* N2 ("next" row) -- camera-frame directions to world rays (coslam.py:342-344): rays_d[r] = R[pose_id[r]] . d_cam[r],
 * rays_o[r] = t[pose_id[r]]; poses [P,4,4] row-major camera-to-world, pose_id int64 [n]. */
int naruto_rays_to_world(uint32_t n, const float* d_cam, const int64_t* pose_id, const float* poses, float* rays_o,
                         float* rays_d, void* stream);

/* N2, store side -- one BA batch from a device-resident keyframe ray store (coslam.py:310-344 + Co-SLAM
 * KeyFrameDatabase.sample_global_rays [not in tree]): n_global DISTINCT rays drawn from the n_kf*rays_per_kf stored rows
 * (python random.sample semantics: without replacement), n_cur distinct pixels of the current frame (all pixels, or those
 * listed in cur_list = the valid-depth pixels), rotated to world with the pose of their keyframe
 * (frame_ids[kf] / keyframe_every; the current frame uses the LAST pose).  The distinct draw is a keyed Feistel
 * permutation of [0, n) with cycle walking: sample element i = perm(i); key = (seed, counter).
 * naruto_perm_index is the same permutation on the host (salt 2: store draw, 3: current-frame draw, 1: naruto_sample_distinct). */
typedef struct NarutoRayBatch {
    const float* store;        /* [n_kf*rays_per_kf, 7] (direction 3, rgb 3, depth 1), device                       */
    uint32_t n_kf, rays_per_kf;
    const int64_t* frame_ids;  /* [n_kf] device                                                                     */
    int64_t keyframe_every;
    uint32_t n_global;
    const float* current;      /* [pixels, 7] rays of the current frame                                             */
    const uint32_t* cur_list;  /* optional [n_cur_pop] admissible pixel indices; NULL: pixels 0..n_cur_pop-1         */
    uint64_t n_cur_pop;
    uint32_t n_cur;
    const float* poses;        /* [n_poses,4,4] camera-to-world                                                      */
    uint32_t n_poses;
    uint64_t seed, counter;
    float *rays_o, *rays_d, *target_s, *target_d;   /* [n_global+n_cur,3] x3, [n_global+n_cur]                      */
    int64_t* ids_out;          /* optional [n_global+n_cur]: pose index per ray, -1 for current-frame rays           */
    /* For a launch that is CAPTURED in a hipGraph and replayed over a growing store (optional, device memory):
     * rng = {seed, counter} -- the draw is keyed by (rng[0] ^ seed, rng[1] + counter), e.g. the trainer's iteration state, which
     * the training forward advances once per iteration; dyn = {n_kf, n_poses, n_cur_pop} replaces the three host values, so new
     * keyframes / poses / another current frame need no re-capture as long as n_global and n_cur stay the same.             */
    const uint64_t* rng;
    const uint64_t* dyn;
    /* optional (round 5): the active ray sampler's lookup done where the rows are in registers -- keys_out[r - key_base] = the sortable key
     * of row r's cached-uncertainty value (what naruto_active_ray_select derives from the row: round((o + d*depth - key_bbox_min) *
     * key_voxel_scale), clipped) for rows key_base <= r < n_global + n_cur - key_tail; consumed by naruto_active_ray_select_keyed.
     * keys_out NULL: off (the other key_* fields are then ignored). */
    uint32_t* keys_out;
    uint32_t key_base, key_tail;
    const float* key_vol;      /* [X,Y,Z] fp32, device                                                               */
    uint32_t key_dims[3];
    float key_bbox_min[3];
    float key_voxel_scale;
} NarutoRayBatch;
int naruto_assemble_rays(const NarutoRayBatch* b, void* stream);
/* N2 + N1 in ONE launch: naruto_assemble_rays | naruto_active_ray_select without the intermediate oversampled batch (coslam.py:310-359 as
 * one step of the mapping iteration).  Row r of the virtual batch is what naruto_assemble_rays would have written (b's own output
 * buffers and ids_out are ignored and may be NULL); base / K / n_tail / volume arguments and the result are naruto_active_ray_select's.
 * At most 8 192 candidates (n_global + n_cur - base - n_tail): NARUTO_ERR_INVALID beyond -- use the two calls. */
int naruto_assemble_select(const NarutoRayBatch* b, uint32_t base, uint32_t K, uint32_t n_tail, const float* uncert_vol,
                           NARUTO_HOST const uint32_t* vol_dims, NARUTO_HOST const float* bbox_min, float voxel_scale, float* out_o, float* out_d,
                           float* out_s, float* out_t, void* stream);
int naruto_sample_distinct(uint64_t n, uint32_t count, uint64_t seed, uint64_t counter, int64_t* out, void* stream);
uint64_t naruto_perm_index(uint64_t i, uint64_t n, uint64_t seed, uint64_t counter, uint64_t salt);

/* A mapped frame between the simulator and the mapping loop, without torch launches or host round trips in between.
 * naruto_frame_ingest: direction [n_pixels,3] (the cached camera-ray table, batch['direction']), rgb [n_pixels,3], depth [n_pixels],
 * fp32 device -> rays [n_pixels,7] = torch.cat([direction, rgb, depth[..., None]], -1) bit for bit, and *n_valid (device, 8 bytes) = the
 * number of pixels with depth > 0 && depth <= depth_trunc (keyframe.py:28, coslam.py:322; NaN is invalid).  The count is an integer sum
 * (one integer atomic per workgroup): exact, whatever the launch plan.
 * naruto_keyframe_row: row [rays_per_kf,7] of the keyframe store from that buffer (keyframe.py:38-60): stored ray i = pixel
 * perm(i mod n_take) of the population [0, n), n = *n_valid (NULL: n_pixels -- filter_depth off), n_take = min(n, rays_per_kf), perm the
 * permutation of naruto_sample_distinct(n, ., seed, counter) (salt 1).  With n_valid the draw indexes the UNFILTERED pixel list as the
 * reference does (the store's "reference" mode).  n = 0 leaves the row untouched.  Both run on the caller's stream without host
 * synchronisation, scratch allocation or float atomics. */
int naruto_frame_ingest(uint64_t n_pixels, const float* direction, const float* rgb, const float* depth, float depth_trunc, float* rays,
                        uint64_t* n_valid, void* stream);
int naruto_keyframe_row(const float* frame_rays, uint64_t n_pixels, const uint64_t* n_valid, uint32_t rays_per_kf, uint64_t seed,
                        uint64_t counter, float* row, void* stream);

/* The pose chain of a tracked run (tracking.disable: False; reference coslam.py:595-602 tracks every frame, :264-281 and :378-407 refine the
 * keyframe poses in global_BA and write them back to est_c2w_data; Co-SLAM's predict_current_pose, the relative pose tracking_render stores
 * and convert_relative_pose are not in the reference tree: parity unpinned, restated here).  est / rel are est_c2w_data / est_c2w_data_rel
 * as [num_frames,4,4] row-major float32 camera-to-world matrices on the device; kf(i) = (i / keyframe_every) * keyframe_every.  Arithmetic
 * in fp64, every output rounded to fp32 once, copies move the bits; one thread per pose, no atomics, no allocation, no synchronisation.
 *   naruto_pose_log      pose6[p] = (omega, t) of c2w[p], p < P: the unit quaternion through the largest of 4w^2, 4x^2, 4y^2, 4z^2, w >= 0,
 *                        omega = 2 atan2(|v|, w) v / |v| (2 v / w below |v| = 1e-12) -- naruto_amd.tracking.matrices_to_pose6, branch for branch
 *   naruto_pose_predict  est[i] = est[i-1] when i == 1 or const_speed == 0, else (est[i-1] @ inv(est[i-2])) @ est[i-1] (predict_current_pose);
 *                        inv is the general affine inverse (adjugate of the 3x3 block over its determinant, then -A^-1 t), not R^T.
 *                        pose6_out [6] = naruto_pose_log of est[i] AS STORED (rounded): the tracker's initial pose.  1 <= i < num_frames
 *   naruto_pose_commit   est[i] = c2w [4,4], the tracker's result; when i % keyframe_every != 0: rel[i] = est[i] @ inv(est[kf(i)])
 *   naruto_pose_scatter  coslam.py:401-407: est[k * keyframe_every] = refined[k] for k = 1 .. P-2 and est[cur_id] = refined[P-1] iff optim_cur;
 *                        est[0] is never written.  refined [P,4,4] (NarutoBAPoses.poses after the call) must not overlap est
 *   naruto_pose_resolve  convert_relative_pose: out[i] = est[i] for a keyframe, rel[i] @ est[kf(i)] otherwise, i < n; out [n,4,4]
 * naruto_debug_pose_log is naruto_pose_log's code on the host (host arrays, nothing launched). */
int naruto_pose_log(uint32_t P, const float* c2w, float* pose6, void* stream);
int naruto_pose_predict(float* est, uint32_t num_frames, uint32_t i, int32_t const_speed, float* pose6_out, void* stream);
int naruto_pose_commit(float* est, float* rel, uint32_t num_frames, uint32_t i, uint32_t keyframe_every, const float* c2w, void* stream);
int naruto_pose_scatter(float* est, uint32_t num_frames, const float* refined, uint32_t P, uint32_t keyframe_every, uint32_t cur_id,
                        int32_t optim_cur, void* stream);
int naruto_pose_resolve(const float* est, const float* rel, uint32_t n, uint32_t keyframe_every, float* out, void* stream);
int naruto_debug_pose_log(uint32_t P, const float* c2w, float* pose6);

/* N3 ("next" row) -- the planner's uncertainty aggregation in goal space (reference src/planner/naruto_planner.py,
 * NarutoPlanner.uncertainty_aggregation_v2 :596-735), consuming the volumes of naruto_map_volumes.
 * naruto_goal_targets: the target observations (:629-632) -- the top_k largest uncertainty voxels (ties: lower flat index),
 *   listed in flat-index order and thinned to top_k_subset entries at positions floor(i*top_k/subset); targets int32
 *   [subset,3] voxel indices.  (The reference takes whatever numpy's argpartition leaves in the last `subset` slots: an
 *   unspecified subset of the top_k.)  dims: HOST array {X,Y,Z}; workspace naruto_goal_targets_workspace() bytes.
 * naruto_goal_aggregate (:637-710): collections[g][k] = uncert[target k] if min_dist < |goal g - target k| < max_dist
 *   (voxels), goal g is not on the border and sdf >= safe_sdf at the goal and its 6 neighbours, and the sdf is > 0 at the
 *   30 points of the segment goal -> target (truncated to voxels); else 0.  aggregated[g] = sum_k collections[g][k].
 *   goal_idx int32 [G,3], targets int32 [k,3]. */
size_t naruto_goal_targets_workspace(uint32_t n_voxels, uint32_t top_k);
int naruto_goal_targets(NARUTO_HOST const uint32_t* dims, const float* uncert_vol, uint32_t top_k, uint32_t top_k_subset,
                        int32_t* targets, void* workspace, void* stream);
int naruto_goal_aggregate(NARUTO_HOST const uint32_t* dims, const float* uncert_vol, const float* sdf_vol, uint32_t n_goals,
                          const int32_t* goal_idx, uint32_t n_targets, const int32_t* targets, float min_dist,
                          float max_dist, float safe_sdf, float* collections, float* aggregated, void* stream);

/* The planner's goal search (reference goal_search_v2, naruto_planner.py:462-510) on the outputs of naruto_goal_aggregate, where
 * they are: one launch of one workgroup, one small buffer to read back.
 *   goal   = argmax of aggregated[G].  TIE RULE (ours: the reference's np.argpartition(a, -1)[-1] has none): among equal maxima
 *            the LOWEST flat index.  Values are ordered by the integer key naruto_goal_targets uses (NaN above +inf, +0 above -0).
 *   look-at = the top m = min(obs_per_goal, K) entries of row `goal` of collections[G,K], value descending, TIES: target index
 *            ascending; n_lookat = max(number of those m that are > 0, 1) (:501-502): the caller keeps the first n_lookat.
 * out (8-byte aligned, NARUTO_GOAL_SEARCH_BYTES(m) bytes, slot r = rank r):
 *   int32  head[8]          {goal flat index, goal_vxl x, y, z (= goal_idx[goal]), n_lookat, m, 0, 0}
 *   double lookat_loc[m][3] vox * voxel_size + bbox_min in fp64, product rounded before the sum (planner.py:99)
 *   int32  lookat_idx[m]    index into targets
 *   int32  lookat_vxl[m][3] targets[lookat_idx]
 *   float  lookat_val[m]
 * bbox_min: HOST double[3].  NARUTO_ERR_INVALID for G == 0, K == 0, obs_per_goal == 0 or K > 4096.  The result does not depend
 * on the launch shape: every comparison is on integer keys and indices. */
#define NARUTO_GOAL_SEARCH_HEAD_INTS 8
#define NARUTO_GOAL_SEARCH_MAX_TARGETS 4096     /* K beyond this is refused: the row's keys sit in LDS */
#define NARUTO_GOAL_SEARCH_BYTES(m) (4u * NARUTO_GOAL_SEARCH_HEAD_INTS + 44u * (size_t)(m))
int naruto_goal_search(uint32_t n_goals, uint32_t n_targets, const float* aggregated, const float* collections,
                       const int32_t* targets, const int32_t* goal_idx, uint32_t obs_per_goal, NARUTO_HOST const double* bbox_min,
                       double voxel_size, void* out, void* stream);

/* N4 ("next" row) -- the dense volume -> mesh path (reference src/slam/coslam/coslam_utils.py:100-226 extract_mesh,
 * callers coslam.py:421-492).  The reference pushes a host-built lattice through query_sdf in 65 536-point chunks with a
 * copy per chunk and runs the third-party `marching_cubes` module on the CPU (coslam_utils.py:26,145).
 * naruto_lattice_points: x[(i*Y + j)*Z + k] = (tx[i], ty[j], tz[k]) -- the (already normalised) lattice of
 *   coslam_utils.py:124-133 expanded on the device; feed x to naruto_query_fwd.  dims: HOST array {X,Y,Z}.
 * naruto_mesh_count: marching cubes over sdf_vol [X,Y,Z] (z fastest), pass 1: counts[0] = vertices, counts[1] =
 *   triangles (device uint64[2]); bit c of a cell's case = (double)value < isolevel at corner (c&1, (c>>1)&1, (c>>2)&1);
 *   cells with a corner |value| > truncation emit nothing; workspace: naruto_mesh_workspace(dims) bytes, kept for
 * naruto_mesh_emit: pass 2: vertices float64 [V,3] in lattice-index coordinates (one per crossed lattice edge, at
 *   t = (isolevel - v0) / (v1 - v0) in float64, ordered by (owner voxel, axis)), triangles int32 [F,3] ordered by
 *   (cell, case-table order), normals towards larger values.  At most cap_* entries are written. */
int naruto_lattice_points(NARUTO_HOST const uint32_t* dims, const float* tx, const float* ty, const float* tz, float* x,
                          void* stream);
size_t naruto_mesh_workspace(NARUTO_HOST const uint32_t* dims);
int naruto_mesh_count(NARUTO_HOST const uint32_t* dims, const float* sdf_vol, double isolevel, double truncation,
                      void* workspace, uint64_t* counts, void* stream);
int naruto_mesh_emit(NARUTO_HOST const uint32_t* dims, const float* sdf_vol, double isolevel, const void* workspace,
                     uint64_t cap_vertices, uint64_t cap_triangles, double* vertices, int32_t* triangles,
                     void* stream);

/* Reconstruction metrics (the reference's evaluation protocol, README "Evaluation": scripts/evaluation/eval_replica.sh:56-83 ->
 * src/evaluation/eval_recon.py -> third-party calc_3d_mesh_metric, which is not in its tree: 200 000 area-weighted surface samples
 * per mesh, nearest neighbour each way through scipy's cKDTree, Accuracy = mean rec->gt, Completion = mean gt->rec, Completion
 * ratio = share of gt->rec below 5 cm).  The chain stays on the device; the contract is restated in the evaluation module of the
 * Python package.  Counts are uint64 so that a count beyond int32 is an error code instead of a wrapped launch.
 *
 * naruto_surface_areas: areas[f] = 0.5 * |e1 x e2| in float64, e1 = v1 - v0, e2 = v2 - v0, cross product component by component
 *   with every product rounded (no fused multiply-add), norm as sqrt((cx*cx + cy*cy) + cz*cz).  vertices [V,3] float32, or float64
 *   when vertices_f64 != 0; faces int32 [F,3].  The data is on the device, so a face index outside [0, V) cannot be refused here: it
 *   is the caller's contract; such a face gets area 0 and is never read through.
 * naruto_surface_sample: sample s draws three float64 uniforms in [0,1) = (splitmix64(splitmix64(seed) + 3*s + draw) >> 11) * 2^-53;
 *   face = first index with cum_area[face] >= u0 * cum_area[F-1] (searchsorted, left side; cum_area: the caller's inclusive prefix
 *   sums of the areas, float64 [F]); (u1, u2) become (|u1 - 1|, |u2 - 1|) when u1 + u2 > 1; point = v0 + (e1*u1 + e2*u2) in float64,
 *   stored as float32 [count,3]; face_index int32 [count].  A zero-area face is picked only as searchsorted's boundary case: it leads
 *   the mesh and u0 is exactly 0.
 * naruto_nn_grid_plan (HOST only, launches nothing): fills grid->n_points, dims, lo, cell for a cloud with bounding box lo .. hi
 *   (host float64 [3] each).  cell = 0 derives the edge from the cloud: 2 * sqrt(box surface / n_points), or extent / cbrt(n_points)
 *   for a box without surface, or 1 for a single position.  dims[a] = floor(extent[a] / cell) + 1; while their product exceeds
 *   max_cells (0 = 2^21) the cell grows by a quarter.
 * naruto_nn_grid_build: the points (float32 [n,3]) counting-sorted by cell into grid->cell_start (uint32 [cells + 1]) and
 *   grid->points (16 bytes per point: x, y, z, original index), both caller-owned; workspace: naruto_nn_grid_workspace(grid) bytes,
 *   free afterwards.  Also used on a QUERY cloud with the target's geometry (cells clamped) to put queries in cell order.
 * naruto_nn_grid_query: per query the nearest target, dist float64 [n_queries] (Euclidean, d2 = (dx*dx + dy*dy) + dz*dz on float64-
 *   promoted coordinates, sqrt at the end: bit for bit what scipy's cKDTree.query returns) and index int32 [n_queries] (the original
 *   index; among equal distances the lowest).  queries float32 [n,3], or queries_sorted = the `points` array of a grid built over the
 *   queries (results still land at the original query index).  Rings of cells around the query's cell, `ring_budget` of them at
 *   most; what has not closed by then is served by the scan.  fallback: uint32 [1 + n_queries], [0] = number of such queries afterwards.
 * naruto_nn_scan: the same result by brute force over targets float32 [m,3], tiled through LDS.
 * naruto_dist_reduce: out[0] = mean of dist [n], out[1] = number of entries < threshold (device float64 [2]), fixed summation order
 *   (per-workgroup partials, one finishing pass), no atomics: bitwise reproducible.  workspace: naruto_dist_reduce_workspace(n) bytes. */
typedef struct NarutoNnGrid {
    uint64_t n_points;
    uint32_t dims[3];             /* cells per axis                                              */
    double   lo[3];               /* lower corner of the cloud's bounding box                    */
    double   cell;                /* cell edge                                                   */
    void*    cell_start;          /* DEVICE uint32 [dims[0]*dims[1]*dims[2] + 1]                 */
    void*    points;              /* DEVICE 16 bytes x n_points                                  */
} NarutoNnGrid;
int naruto_surface_areas(uint64_t n_faces, uint64_t n_vertices, const void* vertices, int vertices_f64, const int32_t* faces,
                         double* areas, void* stream);
int naruto_surface_sample(uint64_t n_faces, uint64_t n_vertices, const void* vertices, int vertices_f64, const int32_t* faces,
                          const double* cum_area, uint64_t count, uint64_t seed, float* points, int32_t* face_index, void* stream);
int naruto_nn_grid_plan(uint64_t n_points, NARUTO_HOST const double* lo, NARUTO_HOST const double* hi, double cell, uint64_t max_cells, NarutoNnGrid* grid);
size_t naruto_nn_grid_workspace(const NarutoNnGrid* grid);
int naruto_nn_grid_build(const NarutoNnGrid* grid, const float* points, void* workspace, void* stream);
int naruto_nn_grid_query(const NarutoNnGrid* grid, uint64_t n_queries, const float* queries, const void* queries_sorted,
                         uint32_t ring_budget, double* dist, int32_t* index, uint32_t* fallback, void* stream);
int naruto_nn_scan(uint64_t n_targets, const float* targets, uint64_t n_queries, const float* queries, double* dist, int32_t* index,
                   void* stream);
size_t naruto_dist_reduce_workspace(uint64_t n);
int naruto_dist_reduce(uint64_t n, const double* dist, double threshold, void* workspace, double* out, void* stream);

/* Rigid alignment of a source cloud to a target cloud: the loop of point-to-point ICP (Open3D's registration_icp, defaults), which the
 * reference's protocol runs on the mesh vertices before the metrics above (src/evaluation/eval_recon.py:80-85 -> neural_slam_eval's
 * get_align_transformation, third-party code outside the reference tree: PARITY UNPINNED; the contract is restated in
 * naruto_amd/evaluation.py).  One iteration = naruto_icp_transform -> naruto_nn_grid_query -> naruto_icp_accumulate -> naruto_icp_step
 * on one stream; nothing synchronises, allocates or uses float atomics; every buffer is the caller's.
 *
 * state: DEVICE float64 [NARUTO_ICP_STATE_DOUBLES]:  [0..15] T (row-major [4,4], cumulative), [16] fitness, [17] inlier_rmse,
 *   [18], [19] the previous evaluation's, [20] iteration (updates applied), [21] status (NARUTO_ICP_*), [22] s2 / s1 of the last
 *   cross-covariance, [23] 0.  The caller writes the initial T and zeros; naruto_icp_step maintains the rest.
 * naruto_icp_transform: out[i] = T points[i], i < n.  points / out are float32 [n,3], or float64 [n,3] both when points_f64; T = 16
 *   DEVICE doubles (the head of a state block).  fp64 arithmetic, out_a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3], every product
 *   and sum rounded (no contraction), then rounded once to the output type: the order is part of the ABI.
 * naruto_icp_accumulate: sums (DEVICE float64 [NARUTO_ICP_SUMS]) over the inliers i < n -- dist[i] <= max_distance and
 *   0 <= index[i] < n_targets -- of: 1, dist^2, p [3], q [3], p q^T [9, row-major], with p = points[i] - origin (the TRANSFORMED source
 *   points, float32 [n,3]) and q = targets[index[i]] - origin (targets float32 [n_targets,3] in original order; index / dist as
 *   naruto_nn_grid_query wrote them).  origin: HOST float64 [3], e.g. the target box's centre, so that the centred covariance does not
 *   cancel.  Two stages in a fixed order that depends on n alone: bitwise reproducible.  workspace:
 *   naruto_icp_accumulate_workspace of n, in bytes.
 * naruto_icp_step (one thread): fitness = count / n_source, inlier_rmse = sqrt(sum dist^2 / count) (0 without inliers) into the state; from
 *   the second evaluation on, status = CONVERGED when |fitness - previous| < relative_fitness and |rmse - previous| < relative_rmse;
 *   else status = MAX_ITERATION when `iteration` has reached max_iteration; else dT from the sums -- centroids, H = sum p q^T -
 *   (sum p)(sum q)^T / count = U S V^T (one-sided Jacobi), R = V diag(1, 1, det(V U^T)) U^T, t = mean q - R mean p (Kabsch with the
 *   determinant correction, no scale) -- and T = dT @ T, iteration += 1; or status = DEGENERATE with T unchanged when count < 3 or
 *   s2 <= 1e-10 s1.  A state whose status is not RUNNING is left as it is.
 * naruto_debug_icp_solve is the solver on the host (host arrays, nothing launched): sums [17], origin [3] (NULL = 0) -> dT [16],
 *   *status = NARUTO_ICP_RUNNING or NARUTO_ICP_DEGENERATE (dT = identity). */
#define NARUTO_ICP_SUMS 17
#define NARUTO_ICP_STATE_DOUBLES 24
#define NARUTO_ICP_RUNNING 0
#define NARUTO_ICP_CONVERGED 1
#define NARUTO_ICP_DEGENERATE 2
#define NARUTO_ICP_MAX_ITERATION 3
int naruto_icp_transform(uint64_t n, const void* points, int points_f64, const double* T, void* out, void* stream);
size_t naruto_icp_accumulate_workspace(uint64_t n);
int naruto_icp_accumulate(uint64_t n, const float* points, uint64_t n_targets, const float* targets, const int32_t* index,
                          const double* dist, double max_distance, NARUTO_HOST const double* origin, void* workspace, double* sums, void* stream);
int naruto_icp_step(const double* sums, uint64_t n_source, NARUTO_HOST const double* origin, uint32_t max_iteration, double relative_fitness,
                    double relative_rmse, double* state, void* stream);
int naruto_debug_icp_solve(NARUTO_HOST const double* sums, NARUTO_HOST const double* origin, NARUTO_HOST double* dT, NARUTO_HOST int32_t* status);

/* Depth odometry: the relative motion T (current camera to previous camera, est[i] = est[i-1] @ T) between two consecutive depth frames by
 * coarse-to-fine projective point-to-plane ICP, a motion prior for the tracker that needs no field (nothing like it is in the reference
 * tree: PARITY UNPINNED; the contract is restated in naruto_amd/odometry.py).  Camera convention: pixel (u, v) has direction
 * ((u-cx)/fx, -(v-cy)/fy, -1), depth is measured along -z; a depth that is not a finite positive number is missing.  Everything runs on the
 * caller's stream in the caller's buffers; nothing synchronises, allocates, reads back or uses atomics; results are bitwise reproducible.
 *
 * NarutoOdomDesc (HOST): the frame H x W and its intrinsics, `levels` pyramid levels (1 .. NARUTO_ODOM_MAX_LEVELS; level 0 is the frame),
 *   iters[k] the iteration cap of the k-th level FROM THE COARSEST (level levels-1-k), max_dist (association), jump (normals), band (pyramid).
 *   Level l+1 has floor(h/2) x floor(w/2) pixels, f/2 and c' = (c + 0.5)/2 - 0.5 (float32, level by level).
 * maps block: DEVICE float32, naruto_odom_maps_bytes; per level l, at 7 x (the pixels of the levels before it) floats:
 *   depth [h,w] | vertex [h,w,3] | normal [h,w,3].  depth: level 0 is the frame with missing depths as 0; a pixel of level l+1 is the mean of its
 *   2 x 2 block's valid depths d with d - m <= band, m the block's smallest valid depth, summed in the order (0,0), (0,1), (1,0), (1,1)
 *   (row, column), 0 when none is valid; an odd last row / column is not read.  vertex = depth * direction ((0,0,0) = missing).  normal =
 *   the normalised cross product of V(u+1,v) - V(u,v) and V(u,v+1) - V(u,v) when all three are valid, both differences have |dz| < jump
 *   and the length is positive, else (0,0,0); the last row and column have none.  float32, every operation rounded (no contraction).
 * state block: DEVICE float64 [NARUTO_ODOM_STATE_DOUBLES]: [0..15] T row-major [4,4]; then NARUTO_ODOM_LEVEL_WORDS per level l at
 *   16 + 8 l: done (0 / 1), status (NARUTO_ICP_*: RUNNING until done), updates applied, the last evaluation's inlier count and rmse,
 *   |omega| and |t| of the last update, 0.  naruto_odom_state_init writes it: T = init->T (a HOST struct, like the desc) when init is given, else
 *   inv(est[i-2]) @ est[i-1] (the last motion once more; est as in the pose chain) when est is given, const_speed != 0 and i > 1, else the
 *   identity; the level words 0.
 * naruto_odom_accumulate at `level`, per pixel of the CURRENT frame's vertex map, in fp64 without contraction: q = T p as
 *   ((r0*x + r1*y) + r2*z) + t; rejected when -q.z <= 1e-6; u = floor(((fx*q.x)/(-q.z) + cx) + 0.5), v = floor(((-(fy*q.y))/(-q.z) + cy) + 0.5),
 *   rejected outside the image, where the PREVIOUS frame's normal n is missing, or when |q - V_prev|^2 > max_dist^2.  r = n . (q - V_prev),
 *   J = [q x n, n] (left perturbation T <- exp(xi) T, xi = (omega, t)).  sums: DEVICE float64 [NARUTO_ODOM_SUMS] = the 21 upper entries of
 *   J^T J (row-major), the 6 of J^T r, sum r^2, the count; thread t of workgroup b adds pixels b*2048 + t + 256 k, k = 0..7 in turn, 256
 *   partial vectors fold by halves in LDS, a second launch folds the workgroups' vectors the same way.  workspace:
 *   naruto_odom_workspace_bytes.  rows (DEVICE float64 [pixels of the level, 2], or NULL): the associated previous pixel (-1 = rejected) and r.
 * naruto_odom_step (one thread): inliers and rmse into the state; DEGENERATE (T unchanged, level done) when the count is below 6 or a
 *   pivot of the Cholesky factorisation of J^T J is <= 1e-12 x its largest diagonal entry; else xi = -(J^T J)^-1 J^T r, T <- exp(xi) T
 *   (the se(3) exponential, Rodrigues), updates += 1, and the level is done CONVERGED when |omega| < 1e-6 and |t| < 1e-6, or
 *   MAX_ITERATION when the updates reached the level's cap.  Accumulate and step launches of a level that is done return at once and
 *   write nothing, so an estimate is a fixed sequence of launches: for each level from the coarsest, cap x (accumulate, step).
 * naruto_pose_predict_relative: est[i] = est[i-1] @ T (fp64 from the float32 matrix, rounded once; state_T = 16 DEVICE doubles, the head of
 *   a state block); pose6_out [6] = naruto_pose_log of est[i] as stored, exactly as naruto_pose_predict ends.  1 <= i < num_frames.
 * naruto_debug_odom_solve is the solver on the host (a HOST struct, nothing launched): sums [29] -> xi [6], dT = exp(xi) [16],
 *   status = NARUTO_ICP_RUNNING or NARUTO_ICP_DEGENERATE (xi = 0, dT = identity). */
#define NARUTO_ODOM_SUMS 29
#define NARUTO_ODOM_MAX_LEVELS 4
#define NARUTO_ODOM_LEVEL_WORDS 8
#define NARUTO_ODOM_STATE_DOUBLES 48
typedef struct NarutoOdomDesc {
    uint32_t H, W, levels;
    uint32_t iters[NARUTO_ODOM_MAX_LEVELS];
    float fx, fy, cx, cy;
    float max_dist, jump, band;
} NarutoOdomDesc;
typedef struct NarutoOdomInit {    /* HOST: an initial transform, row-major [4,4] */
    double T[16];
} NarutoOdomInit;
typedef struct NarutoOdomSolve {   /* HOST: naruto_debug_odom_solve's input (sums) and outputs */
    double sums[NARUTO_ODOM_SUMS];
    double xi[6];
    double dT[16];
    int32_t status;
} NarutoOdomSolve;
size_t naruto_odom_maps_bytes(const NarutoOdomDesc* desc);
size_t naruto_odom_workspace_bytes(const NarutoOdomDesc* desc);
int naruto_odom_frame_maps(const NarutoOdomDesc* desc, const float* depth, float* maps, void* stream);
int naruto_odom_state_init(const NarutoOdomInit* init, const float* est, uint32_t num_frames, uint32_t i, int32_t const_speed, double* state, void* stream);
int naruto_odom_accumulate(const NarutoOdomDesc* desc, uint32_t level, const float* maps_prev, const float* maps_cur, const double* state, double* sums,
                           void* workspace, double* rows, void* stream);
int naruto_odom_step(const NarutoOdomDesc* desc, uint32_t level, const double* sums, double* state, void* stream);
int naruto_pose_predict_relative(float* est, uint32_t num_frames, uint32_t i, const double* state_T, float* pose6_out, void* stream);
int naruto_debug_odom_solve(NarutoOdomSolve* solve);

/* RGB-D odometry: the depth odometry above with a photometric row per pixel beside the geometric one, which pins the motions a plane
 * leaves free (nothing like it is in the reference tree: PARITY UNPINNED; the contract is restated in naruto_amd/odometry.py and
 * tests/odometry_rgbd_spec.py is its numpy twin).  The camera convention, T, the desc, the state block, the level schedule, the done
 * words, naruto_odom_state_init and naruto_odom_step are the depth odometry's.  The intensity is assumed constant between the frames.
 *
 * intensity maps, float32, every operation rounded (no contraction): level 0 I = (0.299 r + 0.587 g) + 0.114 b of the colour frame
 *   [H,W,3] (float32, 0 .. 1); level l+1 (((a + b) + c) + d) * 0.25 over the 2 x 2 block in the order (0,0), (0,1), (1,0), (1,1) (row,
 *   column), an odd last row / column not read; gx(u,v) = (I(u+1,v) - I(u-1,v)) * 0.5 for 1 <= u <= w-2, else 0; gy the same in v.
 * RGB-D maps block: DEVICE float32, naruto_odom_rgbd_maps_bytes: the depth maps block, the layout and bits naruto_odom_frame_maps
 *   writes (7 x the pixels of all levels), then the intensity block: per level l, at 3 x (the pixels of the levels before it) floats,
 *   I [h,w] | gx [h,w] | gy [h,w].  naruto_odom_rgbd_frame_maps writes both in one launch.
 * naruto_odom_rgbd_accumulate at `level`, per pixel i of the CURRENT frame, fp64 without contraction, with q = T p, zc = -q.z > 1e-6,
 *   uc = (fx*q.x)/zc + cx, vc = (-(fy*q.y))/zc + cy and j the nearest pixel (floor(uc + 0.5), floor(vc + 0.5)) as naruto_odom_accumulate:
 *   1. the geometric row, exactly naruto_odom_accumulate's;
 *   2. the photometric row, only when photo->weight > 0: u0 = floor(uc), v0 = floor(vc); rejected unless 1 <= u0, u0 + 1 <= w - 2,
 *      1 <= v0, v0 + 1 <= h - 2, V_prev[j].z < 0 and |q - V_prev[j]|^2 <= max_dist^2 (an occlusion test; no normal is needed).  With
 *      a = uc - u0, b = vc - v0 a map m is sampled as top = m00 + a (m10 - m00), bot = m01 + a (m11 - m01), top + b (bot - top), m10 at
 *      (u0+1, v0).  r_I = I_prev(uc, vc) - I_cur[i]; rejected unless |r_I| <= photo->max_diff and the sampled gx, gy are finite (a NaN
 *      fails the comparison).  With w = photo->weight (metres per unit of intensity), A = gx*fx, B = gy*fy:
 *      g = (w*(A/zc), w*(-(B/zc)), w*((A*q.x - B*q.y)/(zc*zc))), r = w*r_I, J = [q x g, g]: the geometric row's form with g for n.
 *   sums: DEVICE float64 [NARUTO_ODOM_RGBD_SUMS]: [0..28] as NARUTO_ODOM_SUMS over the rows of BOTH kinds (the count [28] too), [29] the
 *   geometric rows, [30] the photometric rows, [31] sum r_I^2 unweighted.  Per pixel the geometric row's terms are added first, then the
 *   photometric row's; pixels, threads, the fold and the finishing launch in naruto_odom_accumulate's order: no atomics, bitwise
 *   reproducible.  workspace: naruto_odom_rgbd_workspace_bytes.  rows (DEVICE float64 [pixels of the level, 4], or NULL): the geometric
 *   j (-1 = rejected), r, the photometric j (-1 = rejected), r_I.  A level that is done: both launches return at once, nothing written.
 * naruto_odom_step runs unchanged on the first 29 sums: the level words' inliers and rmse then count and mix both kinds of rows. */
#define NARUTO_ODOM_RGBD_SUMS 32
typedef struct NarutoOdomPhoto {   /* HOST: the photometric term; weight 0 switches it off */
    float weight;
    float max_diff;
} NarutoOdomPhoto;
size_t naruto_odom_rgbd_maps_bytes(const NarutoOdomDesc* desc);
size_t naruto_odom_rgbd_workspace_bytes(const NarutoOdomDesc* desc);
int naruto_odom_rgbd_frame_maps(const NarutoOdomDesc* desc, const float* depth, const float* color, float* maps, void* stream);
int naruto_odom_rgbd_accumulate(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* maps_prev, const float* maps_cur,
                                const double* state, double* sums, void* workspace, double* rows, void* stream);

/* Scored starts and a verdict for the odometry prior (opt-in; nothing above changes its bits or its launches; the contract is restated in
 * naruto_amd/odometry.py and tests/odometry_gate_spec.py is the numpy twin).  A frame-to-frame estimate converges only from a start inside
 * its basin, and a failed one looks like any other: so K candidate starts are scored at the coarsest level and the cheapest one is
 * taken, and after the level loop four plain checks at level 0 give a verdict.  Launches only, nothing is read back.
 *
 * naruto_odom_score: K (1 .. NARUTO_ODOM_MAX_CANDS) transforms cands (DEVICE float64 [K,16], row-major [4,4] each; a state block's head
 *   is one) scored in one pass over `level`.  photo == NULL: the maps are depth blocks; photo given: RGB-D blocks.  Per pixel of the current
 *   level the vertex p is read once; sums[0] counts the pixels with p.z < 0.  Per candidate k, fp64 without contraction, the association,
 *   rejections and residual r of naruto_odom_accumulate (the same device function): sums[1+4k] = the accepted rows, sums[2+4k] = the sum of
 *   (r*r < trunc*trunc ? r*r : trunc*trunc), trunc in metres, finite and positive.  When photo->weight > 0 the acceptance of
 *   naruto_odom_rgbd_accumulate's photometric row, gradient test included: sums[3+4k] = the accepted rows, sums[4+4k] = the sum of r_I*r_I;
 *   both 0 otherwise.  sums: DEVICE float64 [1 + 4 K].  Pixels, threads, the halving tree and the finishing launch are
 *   naruto_odom_accumulate's: no atomics, bitwise reproducible; at K = 1 with a state's T and trunc = max_dist, sums[1], sums[2] are that
 *   call's sums[28], sums[27] in every bit, and sums[1], sums[3], sums[4] are naruto_odom_rgbd_accumulate's [29], [30], [31].  A candidate
 *   with a non-finite entry fails every comparison: its sums are 0 and no other candidate's change.  workspace:
 *   naruto_odom_score_workspace_bytes(desc, K).  No state block is read, so no done word stops it.
 * naruto_odom_candidates (one thread): cands[0] = the identity; cands[1] = inv(est[i-2]) @ est[i-1] for i > 1 (the constant-speed T of
 *   naruto_odom_state_init, the same device function and bits), else the identity.  cands: DEVICE float64 [2,16].  i < num_frames.
 * naruto_odom_choose (one thread): with n_valid = sums[0], t2 = tau*tau, term(n, s, tau) = (s + (n_valid - n)*t2) / (n_valid*t2), 1 when
 *   n_valid == 0, +inf when not finite: cost[k] = term(sums[1+4k], sums[2+4k], trunc), plus term(sums[3+4k], sums[4+4k], photo_max_diff)
 *   when photo_on != 0; +inf when not finite.  The lowest cost wins, ties go to the lowest index, index 0 when all are +inf.  The state
 *   block is written as naruto_odom_state_init writes it with T = cands[chosen]; the record (below) gets [1] and [2..5], the rest 0.
 * naruto_odom_verdict (one thread): sums = a K = 1 score of the state's T at level 0 with trunc = max_dist.  PASS iff level 0's status word
 *   is not NARUTO_ICP_DEGENERATE, n_geo >= min_overlap * n_valid, n_geo > 0, s_geo <= max_rmse^2 * n_geo, |t|^2 <= max_trans^2 and
 *   trace(R) >= min_trace (= 1 + 2 cos(max_rot), computed by the caller: the kernel has no transcendental function), with
 *   |t|^2 = (tx*tx + ty*ty) + tz*tz and trace = (r00 + r11) + r22 of the state's T.  A NaN fails its comparison: FAIL.  On FAIL the state's
 *   T becomes cands[record[1]], the candidate naruto_odom_choose took.  NarutoOdomGate is a HOST struct.
 * record: DEVICE float64 [NARUTO_ODOM_GATE_WORDS] per frame: [0] verdict (1 PASS, 0 FAIL), [1] the chosen index, [2..5] the costs (-1 =
 *   unused), [6] n_valid, [7] n_geo, [8] rmse = sqrt(s_geo / n_geo) (0 without rows), [9] |t|, [10] trace, [11] level 0's status,
 *   [12] n_photo, [13] sqrt(s_photo / n_photo) (0 without rows), [14], [15] 0.  A value of [8], [9], [10], [13] that is not finite is
 *   written as -1, so a record is always finite.
 * The gated estimate is the fixed sequence: maps, candidates, score at the coarsest level (K = 2, the score trunc), choose, the level
 * loop as it is, score at level 0 (K = 1 on the state block, trunc = max_dist), verdict, naruto_pose_predict_relative. */
#define NARUTO_ODOM_MAX_CANDS 4
#define NARUTO_ODOM_GATE_WORDS 16
typedef struct NarutoOdomGate {    /* HOST: the verdict's thresholds; min_trace = 1 + 2 cos(the largest rotation) */
    double max_trans, min_trace, min_overlap, max_rmse;
} NarutoOdomGate;
size_t naruto_odom_score_workspace_bytes(const NarutoOdomDesc* desc, uint32_t K);
int naruto_odom_score(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* maps_prev, const float* maps_cur,
                      const double* cands, uint32_t K, double trunc, double* sums, void* workspace, void* stream);
int naruto_odom_candidates(const float* est, uint32_t num_frames, uint32_t i, double* cands, void* stream);
int naruto_odom_choose(uint32_t K, const double* sums, const double* cands, int32_t photo_on, double trunc, double photo_max_diff, double* state,
                       double* record, void* stream);
int naruto_odom_verdict(const NarutoOdomDesc* desc, const NarutoOdomGate* gate, const double* sums, const double* cands, double* state, double* record,
                        void* stream);

/* Keyframe-anchored odometry prior: a ring of reference frames chosen on the device (opt-in; nothing above changes its bits or its
 * launches; the contract is restated in naruto_amd/odometry.py and tests/odometry_anchor_spec.py is the numpy twin; nothing like it is in
 * the reference tree: PARITY UNPINNED).  The gated estimate composes every T onto the frame before, so every estimate's bias and noise
 * stays in the pose; here frame i is registered to one of `slots` kept frames and est[i] = est[that frame] @ T.
 *
 * ring: DEVICE float32, `slots` (1 .. NARUTO_ODOM_MAX_REFS) maps blocks back to back, the stride a block's byte size: depth blocks when
 *   photo == NULL, RGB-D blocks when photo is given (as naruto_odom_score tells them apart).
 * head: DEVICE int32 [NARUTO_ODOM_ANCHOR_HEAD]: [0] the slot written last, [1] the count of consecutive refused estimates, [2] the slot
 *   chosen for the current frame, [3] the promote decision of the current frame (0 / 1), [4 + s] slot s's frame id (-1 = empty).  The
 *   caller initialises it (frame 0 in slot 0: {0, 0, 0, 0, 0, -1, ...}) and copies frame 0's maps into slot 0.  A slot's pose is not
 *   stored: it is est[frame id] as it stands when it is read.  A slot word that is not < slots reads slot slots - 1: no word leaves the ring.
 * naruto_odom_anchor_candidates (one thread, 1 <= i < num_frames): cands [slots,2,16] DEVICE float64: for slot s with frame f the starts
 *   R = inv(est[f]) @ est[i-1] and R @ M, M = inv(est[i-2]) @ est[i-1] (i > 1, else the identity), with the pose chain's inverse and
 *   product, fp64 from the float32 matrices.  f == i-1 (and an empty slot): the identity and M, naruto_odom_candidates' bits.
 * naruto_odom_score_refs: naruto_odom_score at K = 2 for every slot in one launch plus one finishing launch: slot s reads the ring's block s
 *   as the previous frame and cands[s]; sums [slots, 9] equal naruto_odom_score(K = 2) on that block in every bit; an empty slot's
 *   workgroups leave at once and its sums are zeros.  workspace: naruto_odom_score_refs_workspace_bytes.
 * naruto_odom_anchor_choose (one thread): naruto_odom_choose's cost per (slot, start) of the slots that are not empty; the lowest wins, ties
 *   go to the larger frame id, then to the lower start; no such slot or every cost +inf: the slot written last, start 0.  Writes head[2];
 *   cands [2,16] = the chosen slot's pair (what naruto_odom_verdict reads); the state block as naruto_odom_choose writes it; record [1] the
 *   start, [2], [3] the chosen slot's costs, [4], [5] -1, the rest 0; anchor_record [0], [1], [2], [6], [7] (below), [3..5] 0.
 * naruto_odom_accumulate_anchored, naruto_odom_score_anchored (K = 1): naruto_odom_accumulate (photo == NULL) or
 *   naruto_odom_rgbd_accumulate (photo given), and naruto_odom_score, with maps_prev = the ring's block head[2], resolved at kernel entry:
 *   the same kernel bodies, the same bits as those calls on that block.  naruto_odom_step and naruto_odom_verdict run unchanged.
 * naruto_odom_anchor_update (one thread), from the verdict's record (T is relative to the chosen reference): PASS: the streak is 0 and the
 *   frame is promoted when n_geo < min_overlap * n_valid, |t| > max_trans or trace < min_trace.  FAIL: the streak grows, and at `refail` the
 *   frame is promoted and the streak is 0 again.  A promoted frame takes slot (head[0] + 1) mod slots: head[0] and that slot's frame id = i
 *   are written here; head[1], head[3]; anchor_record [3], [4], [5].  NarutoOdomAnchor is a HOST struct, min_trace as NarutoOdomGate's.
 * naruto_odom_anchor_promote: when head[3] is set, maps_cur is copied into the ring's block head[0]; every workgroup reads head[3] first,
 *   the other blocks' bytes are untouched, the head is only read.
 * naruto_pose_predict_anchored: est[i] = est[f] @ T, f = anchor_record[1] (outside 0 .. i-1: i-1), fp64 from the float32 matrix, rounded once;
 *   pose6_out as naruto_pose_predict_relative ends.  Before or after the update and the promote: the record keeps the reference's frame id.
 * anchor_record: DEVICE float64 [NARUTO_ODOM_ANCHOR_WORDS] per frame: [0] the chosen slot, [1] its frame id, [2] the slots that were not
 *   empty, [3] promoted (0 / 1), [4] the slot written (-1 = none), [5] the fail streak after the frame, [6] the best cost, [7] the runner-up
 *   among all (slot, start) pairs (-1 where +inf).
 * The anchored estimate is the fixed sequence: maps, anchor_candidates, score_refs at the coarsest level, anchor_choose, the level loop with
 * accumulate_anchored, score_anchored at level 0, verdict, anchor_update, anchor_promote, pose_predict_anchored.  Nothing is read back. */
#define NARUTO_ODOM_MAX_REFS 8
#define NARUTO_ODOM_ANCHOR_HEAD 12
#define NARUTO_ODOM_ANCHOR_WORDS 8
typedef struct NarutoOdomAnchor {  /* HOST: the promote policy; min_trace = 1 + 2 cos(the largest rotation to a reference) */
    uint32_t slots, refail;
    double min_overlap, max_trans, min_trace;
} NarutoOdomAnchor;
size_t naruto_odom_score_refs_workspace_bytes(const NarutoOdomDesc* desc, uint32_t slots);
int naruto_odom_anchor_candidates(const float* est, uint32_t num_frames, uint32_t i, const int32_t* head, uint32_t slots, double* cands, void* stream);
int naruto_odom_score_refs(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head, uint32_t slots,
                           const float* maps_cur, const double* cands, double trunc, double* sums, void* workspace, void* stream);
int naruto_odom_anchor_choose(uint32_t slots, const double* sums, const double* cands_all, int32_t photo_on, double trunc, double photo_max_diff, int32_t* head,
                              double* cands, double* state, double* record, double* anchor_record, void* stream);
int naruto_odom_accumulate_anchored(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head,
                                    uint32_t slots, const float* maps_cur, const double* state, double* sums, void* workspace, void* stream);
int naruto_odom_score_anchored(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head, uint32_t slots,
                               const float* maps_cur, const double* cands, double trunc, double* sums, void* workspace, void* stream);
int naruto_odom_anchor_update(const NarutoOdomAnchor* anchor, uint32_t i, const double* record, int32_t* head, double* anchor_record, void* stream);
int naruto_odom_anchor_promote(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t slots, const int32_t* head, const float* maps_cur, float* ring,
                               void* stream);
int naruto_pose_predict_anchored(float* est, uint32_t num_frames, uint32_t i, const double* anchor_record, const double* state_T, float* pose6_out, void* stream);

/* Frame-to-model alignment: a depth frame registered to the field's own SDF, an opt-in refinement between any motion prior and the
 * tracker (nothing like it is in the reference tree: PARITY UNPINNED; the contract is restated in naruto_amd/registration.py and
 * tests/field_registration_spec.py is the numpy twin).  Conventions, the maps block, the pyramid (NarutoOdomDesc), the state block's
 * first NARUTO_ODOM_STATE_DOUBLES doubles and the level words are the depth odometry's, but T is the CAMERA-TO-FIELD POSE ITSELF,
 * not a relative motion.  state: DEVICE float64 [NARUTO_SDFREG_STATE_DOUBLES]: the odometry's state block, then the start's T [16].
 * The odom desc's iters hold this registration's caps (naruto_odom_step reads them); NarutoSdfRegDesc (HOST) holds trunc
 * (training.trunc), sdf_gate, the field's bounding box, and the levels used from the coarsest to the finest with their caps.
 *
 * One iteration at `level` is five launches, nothing read back:
 * 1. naruto_sdfreg_points, per pixel of the CURRENT frame's vertex map at `level` (thread t of workgroup b takes pixels b*2048 + t +
 *    256 k): q = T p in fp64 as ((r0*x + r1*y) + r2*z) + t, rounded once to float32; x = (q - bbox_min) / (bbox_max - bbox_min) per axis
 *    in float32 without contraction (run_network's normalisation); valid iff p.z < 0 and every x component is finite and in [0, 1].
 *    x [M,3] float32 ((0.5, 0.5, 0.5) for an invalid point), q [M,3] float32, valid [M] bytes; M = the pixels of the level.
 * 2. naruto_query_fwd on x: sdf_uncert [M,2] only.   3. naruto_query_bwd_points with d_raw = (0,0,0,1,0) per point, d_geo = NULL,
 *    x-points form: d_x [M,3] = d sdf / d x.
 * 4. naruto_sdfreg_accumulate, fp64 without contraction, per valid point: r = trunc * sdf, g = (trunc * d_x) / (bbox_max - bbox_min)
 *    per axis (the extent the float32 difference); rejected unless |sdf| < sdf_gate and 0 < (g0*g0 + g1*g1) + g2*g2 < inf (a NaN fails
 *    its comparison).  Row J = [q x g, g], residual r, left perturbation T <- exp(xi) T; no normalisation of g.  sums: DEVICE float64
 *    [NARUTO_SDFREG_SUMS]: [0..28] in naruto_odom_accumulate's layout, [29] the count of valid points; threads, the halving fold in LDS
 *    and the finishing launch as naruto_odom_accumulate: no atomics, bitwise reproducible.  workspace: naruto_sdfreg_workspace_bytes.
 *    rows (DEVICE float64 [M,2], or NULL): the accepted flag (1 / 0) and r (0 when rejected).
 * 5. naruto_odom_step, unchanged, on the first 29 sums.
 * gated != 0: a points / accumulate launch of a level whose done word is set returns at once and writes nothing; gated == 0: the
 * evaluation runs whatever the level words say (the start's and the final evaluation, which go to sums buffers of their own).
 *
 * naruto_sdfreg_init (one thread): T = est[i] (float32 -> fp64), the level words 0, the start's T = the same 16 doubles.
 * naruto_sdfreg_verdict (one thread): sums_start / sums_final = ungated evaluations at the finest level used, of the start (made right
 *   after init) and of the final T.  PASS iff that level's status is not NARUTO_ICP_DEGENERATE, rows >= min_overlap * n_valid, rows > 0,
 *   sum r^2 / rows of the final T <= that of the start, |t|^2 <= max_trans^2 with t = the difference of the two translations, and
 *   trace(R_start^T R) >= min_trace (= 1 + 2 cos(max_rot), computed by the caller).  A NaN fails its comparison.  On FAIL T becomes the
 *   start.  record: DEVICE float64 [NARUTO_SDFREG_RECORD]: verdict (1 / 0), n_valid, rows, the start's rmse, the final rmse, |t|, trace,
 *   that level's status; -1 where a figure is not finite.
 * naruto_sdfreg_commit (one thread): est[i] = T rounded once to float32; pose6_out [6] = naruto_pose_log of the stored matrix, exactly
 *   as naruto_pose_predict_relative ends.  i < num_frames. */
#define NARUTO_SDFREG_SUMS 30
#define NARUTO_SDFREG_STATE_DOUBLES 64
#define NARUTO_SDFREG_RECORD 8
typedef struct NarutoSdfRegDesc {  /* HOST */
    float trunc, sdf_gate;
    float bbox_min[3], bbox_max[3];
    uint32_t n_levels;
    uint32_t levels[NARUTO_ODOM_MAX_LEVELS];   /* from the coarsest to the finest */
    uint32_t iters[NARUTO_ODOM_MAX_LEVELS];    /* the cap of levels[k] */
} NarutoSdfRegDesc;
typedef struct NarutoSdfRegGate {  /* HOST: the verdict's thresholds; min_trace = 1 + 2 cos(the largest rotation) */
    double max_trans, min_trace, min_overlap;
} NarutoSdfRegGate;
size_t naruto_sdfreg_workspace_bytes(const NarutoOdomDesc* odom);
int naruto_sdfreg_points(const NarutoOdomDesc* odom, const NarutoSdfRegDesc* reg, uint32_t level, int32_t gated, const float* maps_cur, const double* state,
                         float* x, float* q, uint8_t* valid, void* stream);
int naruto_sdfreg_accumulate(const NarutoOdomDesc* odom, const NarutoSdfRegDesc* reg, uint32_t level, int32_t gated, const float* sdf_uncert, const float* d_x,
                             const float* q, const uint8_t* valid, const double* state, double* sums, void* workspace, double* rows, void* stream);
int naruto_sdfreg_init(const float* est, uint32_t num_frames, uint32_t i, double* state, void* stream);
int naruto_sdfreg_verdict(const NarutoSdfRegDesc* reg, const NarutoSdfRegGate* gate, const double* sums_start, const double* sums_final, double* state,
                          double* record, void* stream);
int naruto_sdfreg_commit(float* est, uint32_t num_frames, uint32_t i, const double* state, float* pose6_out, void* stream);

/* The planner's local RRT(reference src/planner/rrt.py and src/planner/rrt_naruto.py: class RRTNaruto, the
 * local_planner_method of every shipped config), on the volumes of naruto_map_volumes.  Unit: voxel.
 *
 * NarutoRrtPlan (HOST struct) describes one planner and its caller-owned device buffers:
 *   dims            {X,Y,Z} of sdf_vol
 *   range           x/y/z_range of RRT.__init__ (rrt.py:205-208), full_range full_x/y/z_range (:209-211): the box the rows
 *                   handed to naruto_rrt_grow are drawn from in mode RUN / FULL.  The library draws nothing; it checks lo <= hi.
 *   step_size, step_amplifier, collision_thre, enable_direct_line: the constructor arguments (rrt_naruto.py:37-50)
 *   sdf_vol         DEVICE float32 [X,Y,Z], z fastest
 *   workspace       DEVICE, naruto_rrt_workspace bytes, 16-byte aligned.  It opens with the state block int32[16] (indices
 *                   NARUTO_RRT_STATE_*) the caller reads back after a launch, then the goal and the per-voxel cell lists' heads.
 *   nodes_xyz       DEVICE float64 [capacity,3]  the reference's Node._xyz_arr
 *   nodes_xyz32     DEVICE float32 [capacity,3]  its nodes_tensor (rrt.py:144: the float64 coordinates rounded)
 *   parent, next    DEVICE int32 [capacity]      parent node (-1: the start) / next node of the same cell list (-1: end)
 *   capacity        entries of the four tree buffers; cell_threshold: node count from which the nearest-node search walks the
 *                   cell lists instead of scanning nodes_xyz32 (0: NARUTO_RRT_CELL_THRESHOLD).  Both give the same tree.
 * The tree lives in the caller's buffers, so a second naruto_rrt_grow continues it, as a second RRTNaruto.run() does.
 *
 * naruto_rrt_start (rrt.py:248-277 start_new_plan): tree = {start}, goal stored, counters zero.  start, goal: HOST fp64[3].
 * naruto_rrt_grow: mode NARUTO_RRT_MODE_RUN = RRTNaruto.run() (rrt_naruto.py:189-234): per iteration the direct line
 *   goal -> last node first (:92-133, if enable_direct_line), else / then the random extension (:135-187), early exit
 *   when a new node is within step_size of the goal in float32, and afterwards goal.parent = nearest node, reachable iff its
 *   fp64 distance <= step_size.  NARUTO_RRT_MODE_FULL = RRT.run_full() (rrt.py:350-355): max_iter random extensions, no goal
 *   test.  rows: DEVICE fp64 [n_rows,3], one row per random extension, in order.  max_iter counts from the call with
 *   restart != 0; a call with restart == 0 resumes the same run()/run_full() where the last launch stopped.  One persistent
 *   launch of one workgroup; it ends with state[NARUTO_RRT_STATE_STATUS] =
 *     NARUTO_RRT_DONE       finished (RUN: state GOAL_PARENT / REACHABLE are set),
 *     NARUTO_RRT_NEED_ROWS  every row used: call again (restart = 0) with fresh rows; state ROWS_USED rows were consumed,
 *     NARUTO_RRT_NEED_ROOM  the next append would exceed capacity: nothing of that step was consumed; grow the four tree
 *                           buffers (copy the first state NODES entries) and call again (restart = 0) with the unused rows.
 *   The tree does not depend on where such a stop fell.
 * naruto_rrt_path (rrt.py:376-387 find_path) as node indices: path DEVICE int32 [capacity+1], path[0] = count, then
 *   goal.parent, its parent, ..., the start, so that only the path has to be copied back.
 * naruto_segments_free (rrt.py:77-117 is_collision_free, imported at naruto_planner.py:34, called at :556) for n segments:
 *   pa, pb DEVICE fp64 [n,3]; num_collision_free DEVICE int32 [n], complete_free DEVICE uint8 [n].
 * naruto_reachable_mask (rrt.py:389-431 get_reachable_mask): mask DEVICE float32 [X,Y,Z] = 1 where some node of the plan's
 *   tree lies within step_size of the voxel (float32 arithmetic), else 0.
 * Differences to the reference: a sample outside [0, dim-1] counts as blocked (the reference raises on `None > thre`); at a
 * coordinate of exactly dim-1 the upper corner has weight 0 and its index is clamped (the reference indexes out of bounds);
 * a direct line of length 0 (start == goal, where the reference divides by zero) ends the run as reached. */
#define NARUTO_RRT_MODE_RUN 0
#define NARUTO_RRT_MODE_FULL 1
#define NARUTO_RRT_DONE 0
#define NARUTO_RRT_NEED_ROWS 1
#define NARUTO_RRT_NEED_ROOM 2
#define NARUTO_RRT_CELL_THRESHOLD 2048u
#define NARUTO_RRT_STATE_NODES 0        /* node count */
#define NARUTO_RRT_STATE_ITER 1         /* iterations of the current run()/run_full() completed */
#define NARUTO_RRT_STATE_RRT_ITER 2     /* the reference's rrt_iter (advanced by RUN only) */
#define NARUTO_RRT_STATE_STATUS 3
#define NARUTO_RRT_STATE_ROWS_USED 4    /* rows consumed by the last launch */
#define NARUTO_RRT_STATE_GOAL_PARENT 5  /* goal.parent as a node index, -1 before the first finished RUN */
#define NARUTO_RRT_STATE_REACHABLE 6
#define NARUTO_RRT_STATE_MID_ITER 7     /* the direct-line half of iteration ITER is already in the tree (a stop fell after it) */
#define NARUTO_RRT_STATE_USE_CELLS 9    /* the cell lists are valid (the start lay inside the grid): nearest search and mask may use them;
                                           clearing it sends naruto_reachable_mask through node tiles instead */
#define NARUTO_RRT_STATE_INTS 16        /* length of the state block, in int32 */
typedef struct NarutoRrtPlan {
    uint32_t dims[3];
    double range[3][2], full_range[3][2];
    double step_size, step_amplifier, collision_thre;
    int32_t enable_direct_line;
    const float* sdf_vol;
    void* workspace;
    double* nodes_xyz; float* nodes_xyz32; int32_t* parent; int32_t* next;
    uint32_t capacity, cell_threshold;
} NarutoRrtPlan;
size_t naruto_rrt_workspace(NARUTO_HOST const uint32_t* dims /* HOST {X,Y,Z} */);
int naruto_rrt_start(const NarutoRrtPlan* plan, NARUTO_HOST const double* start, NARUTO_HOST const double* goal, void* stream);
int naruto_rrt_grow(const NarutoRrtPlan* plan, int mode, const double* rows, uint32_t n_rows, uint32_t max_iter,
                    int restart, void* stream);
int naruto_rrt_path(const NarutoRrtPlan* plan, int32_t* path, void* stream);
int naruto_segments_free(NARUTO_HOST const uint32_t* dims /* HOST */, const float* sdf_vol, uint32_t n, const double* pa,
                         const double* pb, double step_size, double collision_thre, int32_t* num_collision_free,
                         uint8_t* complete_free, void* stream);
int naruto_reachable_mask(const NarutoRrtPlan* plan, float* mask, void* stream);

/* All parameter tensors of one optimiser in a single launch (<= 8 segments, per-segment lr / eps / weight_decay,
 * shared betas and step). */
typedef struct NarutoAdamSeg {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    uint64_t n; float lr, eps, weight_decay;
    uint32_t step_lag;     /* this tensor's step number is the launch's minus step_lag (torch.optim.Adam counts steps PER PARAMETER:
                              one that was added later, or sat a step out without a gradient, lags behind); 0 in the mapping loop */
} NarutoAdamSeg;
#define NARUTO_ADAM_ADVANCE 1u   /* step_dev = int32[2] {completed steps, 0}: this launch is step step_dev[0]+1 and stores it back */
#define NARUTO_ADAM_ZERO_GRAD 2u /* zero every gradient once consumed (the segments' grad buffers are written) */
int naruto_adam_multi(const NarutoAdamSeg* segs /* host array */, uint32_t n_segs, float beta1, float beta2,
                      uint32_t step, int32_t* step_dev, uint32_t flags, void* stream);

/* ---- The mapping iteration as two calls: naruto_amd.trainer.MappingTrainer's fast path ----------------------------
 * What JointEncodingNaruto.forward (scene_rep.py:227-287) + get_loss_from_ret incl. Co-SLAM smoothness
 * (coslam.py:154-174) + loss.backward() do in one global_BA iteration (coslam.py:361-399), as few launches as
 * possible: side work rides in a bigger launch as extra workgroups, the small reductions share one tail launch
 * (naruto_train.hip).  Same kernels' arithmetic as the modular entry points above.
 *   naruto_train_forward : z_vals, raw, feat_save, rgb, depth, uncert_map, sums[16]; with finalize != 0 also
 *                          losses[10] = {rgb, depth, sdf, fs, psnr, uncert, min(uncert_map), n_valid,
 *                                        smoothness term, total = sum_i loss_weights[i] * losses[i]}
 *   (data parallel: finalize = 0, all-reduce sums[0..9), naruto_train_finalize)
 *   naruto_train_backward: gradient of the total w.r.t. the parameters in g (table / MLP weights written or
 *                          accumulated per flags as in naruto_query_bwd; uncert_grid always accumulated) */
typedef struct NarutoTrainStep {
    uint32_t n_rays, n_samples_d, n_range_d;          /* S = n_samples_d + n_range_d samples per ray          */
    uint32_t perturb;                                 /* != 0: stratified depth jitter (training.perturb > 0) */
    float near_, far_, range_d, depth_trunc, rgb_missing;
    uint32_t smooth_points;                           /* 0: no smoothness term (else Co-SLAM sample_points)   */
    float smooth_voxel, smooth_margin;
    float smooth_grad_scale;                          /* extra factor on the term's gradient (0 = 1; 1/world) */
    uint64_t n_rays_total;                            /* rays over all ranks (0: n_rays)                      */
    const float *rays_o, *rays_d, *target_rgb, *target_d;      /* [N,3] [N,3] [N,3] [N]                       */
    const float *rand;                                /* [N,S] depth jitter in [0,1), with perturb (or rng)   */
    const float *rand6;                               /* [6] lattice placement, with smooth_points (or rng)   */
    uint64_t *rng;                                    /* {seed, counter}: where rand / rand6 is NULL the kernels
                                                         draw their own numbers (splitmix64 keyed by seed, counter,
                                                         index); the counter advances once per forward.        */
    const float *loss_weights;                        /* [10] device: d(total)/d(losses[i]); slots 4,6,7,9 ignored */
    float *z_vals, *raw, *feat_save;                  /* [N,S] [N,S,5] [16][N*S][2]: all three required        */
                                                      /* feat_save is PRIVATE to the forward / backward pair of one step: level-major as
                                                       * written above, or sample-major [N*S][16][2] where the forward runs in Morton
                                                       * order of the samples (tables > 64 MB, batches >= 4 M samples; round 6).  Same
                                                       * size either way; naruto_train_backward knows which from the same launch plan.  */
    float *rgb, *depth, *uncert_map;                  /* [N,3] [N] [N] (any may be NULL)                      */
    double *sums;                                     /* [NARUTO_LOSS_NSUMS]                                  */
    float *losses;                                    /* [10]                                                 */
    float *d_raw;                                     /* [N,S,5]          (backward)                          */
    uint32_t *ray_count, *ray_offset, *active_idx, *n_active;  /* [N] [N] [N*S] [1]  (backward)               */
    void *workspace;                                  /* naruto_train_workspace() bytes                       */
    const float *loss_weight_parts[10];               /* naruto_train_backward only, optional: per-slot device SCALARS added to
                                                         loss_weights (which may then be NULL = zeros) -- the cotangents autograd
                                                         hands back for the scalar losses of an unchanged caller's weighted sum
                                                         (coslam.py:154-174); gathered into the workspace by one tiny launch     */
    float *min_uncert_running;                        /* optional [1]: every iteration folds its min(uncert_map) into this word
                                                         (minimum; a NaN sticks) -- the reference's per-forward
                                                         `assert uncert_map.min() > 0` (scene_rep.py:280) as a value the host can
                                                         read whenever it likes, graph replays included; initialise to +inf   */
    void *fwd_image;                                  /* optional, exact (fp32) mode: naruto_fwd_image_bytes() bytes, 16-byte aligned, prepared
                                                         once by naruto_fwd_image_init -- the training forward's MLP weights in the order its
                                                         matrix instructions read them.  A naruto_train_backward with a fused optimiser (opt !=
                                                         NULL) rewrites every weight's entry in the launch that steps the weights.          */
    uint32_t fwd_image_fresh;                         /* the CALLER's statement that fwd_image matches the weights in p: naruto_train_forward
                                                         then copies it instead of re-deriving it in every workgroup (walk of S = 64 k <= 192
                                                         samples, short rays).  True exactly when the last thing that changed the MLP weights
                                                         was such a backward on THIS step (or naruto_fwd_image_init) -- the library cannot see
                                                         a load_state_dict, another optimiser or a copy into the weights.  0: never read.   */
} NarutoTrainStep;
/* Optimiser in the backward (single process): the launch that finishes the gradients applies torch.optim.Adam
 * (amsgrad off, L2 weight decay; reference create_optimizer, coslam.py:409-419) to the table and the MLP weights in
 * place.  Tensor order: table, sdf_w0, sdf_w1, col_w0, col_w1.  (Levels of more than 2^17 entries are stepped by the last
 * kernel of the binned scatter, one 8 192-entry slice per workgroup.) */
typedef struct NarutoFusedAdam {
    float* param[5]; float* exp_avg[5]; float* exp_avg_sq[5];
    float lr[5], eps[5], weight_decay[5];
    float beta1, beta2;
    const int32_t* step_dev;              /* device int32: this step's 1-based number                               */
    /* optional (round 5): the NEXT iteration's ray batch -- naruto_assemble_rays' work rides in the launch that finishes the gradients
     * (nothing of this iteration reads the ray buffers any more by then; a device-side rng is read AFTER this iteration's forward
     * advanced it, i.e. it keys the next iteration's draw).  NULL: off. */
    const struct NarutoRayBatch* next_batch;
    /* optional: the uncertainty grid's own optimiser (a separate Adam that steps every fifth iteration on the gradient accumulated in
     * g->uncert_grid) rides in the launch that finishes the gradients.  uncert_step != 0: the thread that adds voxel v's partial sums into the
     * accumulated gradient applies naruto_adam_multi's step to p->uncert_grid[v] and zeroes the gradient (NARUTO_ADAM_ADVANCE |
     * NARUTO_ADAM_ZERO_GRAD: uncert_step_dev = {completed steps, ticket word}, advanced by the last of the grid's workgroups; uncert_step_lag as
     * NarutoAdamSeg.step_lag).  Same arithmetic in the same order as the separate launch.  Needs a grid whose gradient goes through the scatter
     * (up to 2^20 voxels); uncert_step == 0: the gradient is accumulated and nothing else, the fields below are not read. */
    uint32_t uncert_step, uncert_step_lag;
    float* uncert_exp_avg; float* uncert_exp_avg_sq;
    int32_t* uncert_step_dev;
    float uncert_lr, uncert_eps, uncert_weight_decay, uncert_beta1, uncert_beta2;
} NarutoFusedAdam;
size_t naruto_train_workspace(const NarutoField* f, const NarutoTrainStep* t);
int naruto_train_forward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, int finalize, void* stream);
int naruto_train_finalize(const NarutoField* f, const NarutoTrainStep* t, void* stream);
int naruto_train_backward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoGrads* g,
                          uint32_t flags, const NarutoFusedAdam* opt /* NULL: gradients only; else g's table / weight
                          pointers may be NULL (gradients not materialised) */, void* stream);

/* NarutoTrainStep.fwd_image: its size (returned; optionally the image part's bytes and the number of MLP weights, 5 184), and its one-time
 * preparation from the weights in p (one small launch + one upload; NOT inside a stream capture). */
size_t naruto_fwd_image_bytes(NARUTO_HOST size_t* image_bytes, NARUTO_HOST uint32_t* n_weights);
int naruto_fwd_image_init(const NarutoField* f, const NarutoParams* p, void* fwd_image, void* stream);
/* tests: what one workgroup of the training forward stages from the weights in p, copied out (image_bytes bytes, 16-byte aligned), and -- host
 * only -- where the finishing launch puts each weight: slots [n_weights] (low half: byte offset of the first piece / of the float; high half:
 * byte stride to the other two pieces, 0 for col_w1's floats), zero_fill [image_bytes] or NULL (1: a byte of the staging's zero padding). */
int naruto_debug_fwd_image(const NarutoField* f, const NarutoParams* p, void* out, void* stream);
int naruto_debug_fwd_image_map(uint32_t* slots, uint8_t* zero_fill);

/* Measurement aid (bench.py): ONLY the field-query launch of naruto_train_forward, exactly as the iteration issues it (one wave per ray
 * with early termination when S % 64 == 0 -- and then with the loss stage riding in the same launch, k_query_fwd_loss); t->z_vals
 * must hold a previous forward's depths. */
int naruto_debug_train_query_fwd(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, void* stream);
/* profiling: a device buffer of 16 x (ray workgroups) uint64 into which the packed training forward (k_query_fwd_loss_packed) stamps the
 * shader clock at the start and behind each step of every workgroup's first chunk (tools/fwd_timeline.py); NULL switches it off. */
int naruto_debug_fwd_timeline(void* device_buffer);
/* profiling: a device buffer of 16 x (4 x workgroups of the fp32 MLP backward, at most one workgroup per compute unit) uint64.  While it is set
 * the backward launches the stamped build of k_query_bwd: every wave leaves the 100 MHz clock summed per phase of its tile loop and four stamps
 * of the kernel's own (tools/bwd_timeline.py); the gradients are the product kernel's.  NULL switches it off. */
int naruto_debug_bwd_timeline(void* device_buffer);
/* naruto_query_bwd / naruto_train_backward: the workspace must be 16-byte aligned (the fp32 MLP backward writes its per-workgroup weight-gradient
 * partials with 16-byte stores); NARUTO_ERR_INVALID otherwise. */
/* bytes of dynamic LDS the launcher reserves for the fp32 MLP backward (k_query_bwd) and passes to every launch of it */
size_t naruto_debug_query_bwd_lds_bytes(void);
/* profiling (bench.py's roofline): k_hash_scatter_lds alone, over the point list the preceding naruto_train_backward left in the
 * workspace, in the launch shape of the iteration; writes the scatter's partial tables only (no gradient, no parameter). */
int naruto_debug_train_scatter(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, void* stream);
/* testing (tests/test_gpu_scatter_visit.py): the table scatter over a caller-made point list in the training layout -- x_soa [3][cap]
 * normalised points, d_feat [16][cap][2] cotangents, cap a multiple of 4, *n_dev (device) the number of list points <= cap -- i.e. the
 * hashed levels' list route with prescribed cotangents.  Adds into d_table like naruto_hash_encode_bwd; workspace: naruto_scatter_workspace(f, cap). */
int naruto_debug_scatter_list(const NarutoField* f, uint32_t cap, const uint32_t* n_dev, const float* x_soa, const float* d_feat, float* d_table,
                              void* workspace, void* stream);

/* The launch plans, host only (nothing is launched, no GPU needed; tests/test_launch_plans_host.py, tests/test_gpu_launch_forms.py).
 * naruto_debug_train_plan: what naruto_train_forward's field-query launch is for this step (only n_rays, n_samples_d and n_range_d of t
 *   are read; the NARUTO_FWD_* / NARUTO_WALK_* / NARUTO_DEBUG_* knobs as the launcher reads them); with_loss = the loss stage may ride along
 *   (naruto_train_forward), deferred = forward + backward as one iteration.  out = {form (0 Flat, 1 Walk, 2 Packed, 3 Short, 4 Sorted), fused
 *   loss stage, two-phase tile, smoothness term moved to the backward, tiles per ray (Walk), rays per loss row, ray workgroups, threads per
 *   workgroup}.  Packed's fall-back to Flat, where not even one row fits the LDS, is reported as Flat.
 * naruto_debug_render_plan: naruto_render_fwd's launch for n_rays rays of S samples (bf16 != 0: NARUTO_MLP_BF16 mode); wide = -1 reads
 *   NARUTO_RENDER_WIDE as the launcher does, 0 / 1 / 2 override it.  out = {form (0 k_render_fwd, 1 k_render_fwd_packed<*, 256>,
 *   2 k_render_fwd_packed<*, 512>), rays per group, workgroups, rays per pass of the grid-stride loop, dynamic LDS bytes of the launch,
 *   dynamic LDS bytes reserved for the kernel, the kernel's static LDS bytes, threads per workgroup}. */
int naruto_debug_train_plan(const NarutoField* f, const NarutoTrainStep* t, int with_loss, int deferred, NARUTO_HOST uint32_t out[8]);
int naruto_debug_render_plan(const NarutoField* f, uint32_t n_rays, uint32_t S, int bf16, int wide, NARUTO_HOST uint32_t out[8]);

/* Measurement aid (bench.py, workloads whose table fits no cache): one launch that reads RANDOM 64-byte lines out of `table`
 * (table_bytes of it) -- the access pattern of the hash gather on the T = 2^22 levels, without the kernel around it; *n_lines_out
 * (host) = distinct lines the launch requests.  Timed with HIP events it gives the memory system's random-line rate, the ceiling
 * `roofline.random_line_roof` prices the gather against (tools/hbm_random_line_bench.hip: the standalone sweep). */
int naruto_debug_random_lines(const float* table, uint64_t table_bytes, uint32_t iters, float* sink, NARUTO_HOST uint64_t* n_lines_out, void* stream);

/* Hardware self-checks used by the GPU tests: the MFMA / permlane layouts the kernels rely on.
 * out: device buffer of 64*16 floats; returns 0 and fills out (see tests/test_gpu_parity.py: test_mfma_layout, test_permlane32_swap). */
int naruto_debug_mfma_layout(const float* a, const float* b, float* out, void* stream);
int naruto_debug_permlane_swap(const float* v0, const float* v1, float* out, void* stream);
/* a [32,16], b [16,32] fp32 (rounded to bf16 inside) -> out [64*16]: lane l, reg r of D = A.B by v_mfma_f32_32x32x16_bf16 with
 * A lane l = A[l&31][8*(l>>5) + e], B lane l = B[8*(l>>5) + e][l&31], e = 0..7 (test_mfma_bf16_layout). */
int naruto_debug_mfma_bf16_layout(const float* a, const float* b, float* out, void* stream);

/* Camera tracking: Co-SLAM tracking_render (reference call site coslam.py:594-602; parity unpinned), one frame's pose optimised with
 * the network frozen.  Pose = (omega [3], the axis-angle of the camera-to-world rotation; t [3]); R(omega) by Rodrigues' formula.
 * Per call: naruto_track_draw draws n_rays distinct pixels of the frame's interior [edge_h, H - edge_h) x [edge_w, W - edge_w) with the
 * keyed permutation of naruto_sample_distinct (key from rng = {seed, counter} with salt 4; flat interior index k maps to
 * h = edge_h + k % (H - 2 edge_h), w = edge_w + k / (H - 2 edge_h)) and gathers d_cam and the training step's target_rgb / target_d;
 * naruto_track_rays resets the state from pose_init, writes the training step's rays_o / rays_d of iteration 0 and advances rng[1].
 * Per iteration: naruto_train_forward with finalize = 1 and no smoothness term, then naruto_track_backward on the same training step:
 * the loss backward and compaction, the ray gradients of naruto_query_bwd_points, and ONE workgroup that sums the pose gradient in a
 * fixed order (no atomics), keeps the best pose (the first loss is the best, then loss < best resets thresh, else thresh + 1; thresh >
 * wait_iters stops the call: later iterations change nothing), takes one torch.optim.Adam step and writes the NEXT iteration's rays. */
typedef struct NarutoTrackStep {
    uint32_t n_rays;                                  /* pixels per call (= the training step's n_rays)             */
    uint32_t H, W, edge_h, edge_w;                    /* frame size and margins (0: no margin)                      */
    const float *direction, *rgb, *depth;             /* the frame: [H,W,3] camera-frame directions, [H,W,3], [H,W]  */
    uint64_t *rng;                                    /* {seed, counter}: keys the draw                              */
    float *d_cam;                                     /* [N,3] directions of the drawn pixels                        */
    int64_t *pix;                                     /* optional [N]: flat pixel index h * W + w of each ray        */
    const float *pose_init;                           /* [6] (omega, t) of the initial pose                          */
    float *pose, *exp_avg, *exp_avg_sq;               /* [6] the pose and its Adam moments                           */
    int32_t *state;                                   /* [4] {Adam step, thresh, stopped, iteration}                 */
    float lr_rot, lr_trans, beta1, beta2, eps;        /* Adam (no weight decay): lr_rot for omega, lr_trans for t    */
    uint32_t wait_iters;
    int32_t best;                                     /* != 0: c2w is the best pose, else the pose evaluated last    */
    float *best_pose, *best_loss;                     /* [6] [1]                                                    */
    float *c2w;                                       /* [16] the result, row-major camera-to-world                 */
    float *d_rays_o, *d_rays_d;                       /* [N,3] the iteration's ray gradients                         */
    float *trace_loss, *trace_pose, *trace_d_pose;    /* optional [max_trace] [max_trace,6] [max_trace,6]: per evaluated
                                                         iteration its total loss, pose and pose gradient              */
    uint32_t max_trace;
    void *workspace;                                  /* naruto_track_workspace bytes                                */
} NarutoTrackStep;
size_t naruto_track_workspace(const NarutoField* f, uint32_t n_rays, uint32_t n_samples);
int naruto_track_draw(const NarutoTrackStep* k, const NarutoTrainStep* t, void* stream);
int naruto_track_rays(const NarutoTrackStep* k, const NarutoTrainStep* t, void* stream);
int naruto_track_backward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoTrackStep* k, void* stream);
/* host only: R(w) (row-major) and the VJP d_w of sum(G * R(w)), in fp64, by the tracking kernels' own code (R or d_w may be NULL) */
int naruto_debug_rodrigues(NARUTO_HOST const double* w, NARUTO_HOST const double* G, NARUTO_HOST double* R, NARUTO_HOST double* d_w);


/* Pose refinement inside global_BA: the pose optimiser of the reference's loop (coslam.py:256-281, 342-344, 378-407; parity unpinned --
 * get_pose_param_optim and matrix_from_tensor are Co-SLAM functions that are not in the reference tree, the loop around them is the
 * contract).  Per call with P = dyn[1] poses (the current frame's last): pose 0 is fixed, poses 1 .. P-2 are parameters, pose P-1 is one
 * iff optim_cur.  A parameter pose is (omega [3], the absolute axis-angle of the camera-to-world rotation; t [3]), R(omega) by Rodrigues'
 * formula, stepped by torch.optim.Adam with lr_rot / lr_trans and ONE step count shared by all poses.
 *   naruto_ba_poses_init         once per call, before its first batch is assembled: pose6 <- pose_init (the caller's (omega, t), P rows), moments,
 *                                sums and state zeroed, the parameter poses' [4,4] rows of `poses` rewritten from R(omega) (fixed poses keep their bits)
 *   naruto_train_backward_poses  naruto_train_backward with, between its loss backward and the launches that scatter and step the network,
 *                                the iteration's ray gradients (naruto_query_bwd_points' kernels over the active list), their sums per pose
 *                                -- d_t[p] = sum d_rays_o[r], H[p] = sum d_rays_d[r] (x) rays_d[r] over the rays of pose p, fp64, fixed order, no
 *                                atomics -- added to `accum`, and ONE workgroup that counts the iteration (state[1]) and, when
 *                                (iteration + 1) % pose_accum_step == 0, steps every parameter pose: d_omega = VJP of Rodrigues with cotangent
 *                                H R(omega), d_t, one Adam step, sums zeroed, the new [4,4] rows written to `poses` -- before the launch that
 *                                assembles the next batch (NarutoFusedAdam.next_batch).  bap NULL: naruto_train_backward, launch for launch.
 * The pose of training ray r is ids[src_rows ? src_rows[r] : r] (-1 = the current frame = pose P-1): ids as NarutoRayBatch.ids_out leaves
 * them, src_rows as naruto_active_ray_select_rows does.  All pointers are device memory; a captured launch stays valid while P grows. */
typedef struct NarutoBAPoses {
    uint32_t max_poses;                               /* rows of poses, pose_init, pose6, the moments, accum and of a trace slice */
    uint32_t optim_cur;                               /* != 0: the current frame's pose (the last) is a parameter too (mapping.optim_cur) */
    uint32_t pose_accum_step;                         /* mapping.pose_accum_step (> 0)                               */
    const uint64_t *dyn;                              /* {n_kf, n_poses, n_cur_pop} as NarutoRayBatch.dyn            */
    float *poses;                                     /* [max_poses,4,4] camera-to-world: what the ray assembly reads */
    const float *pose_init;                           /* [max_poses,6] the caller's poses as (omega, t)              */
    float *pose6, *exp_avg, *exp_avg_sq;              /* [max_poses,6] the parameters and their Adam moments         */
    double *accum;                                    /* [max_poses,12] the window's sums: d_t[3] | H[9]             */
    int32_t *state;                                   /* [4] {pose steps, iterations} of this call, 0, 0             */
    const int64_t *ids;                               /* [n_ids] pose id per assembled row                           */
    uint32_t n_ids;
    const uint32_t *src_rows;                         /* optional [n_rays]: assembled row of each training ray       */
    float *d_rays_o, *d_rays_d;                       /* [n_rays,3] the iteration's ray gradients                    */
    float lr_rot, lr_trans, beta1, beta2, eps;        /* Adam (no weight decay): lr_rot for omega, lr_trans for t    */
    float *trace_pose, *trace_grad;                   /* optional [max_trace,max_poses,6] x2: per pose step the (omega, t) before the
                                                         step and the accumulated gradient (fixed poses: their (omega, t), 0)   */
    uint32_t max_trace;
    void *workspace;                                  /* naruto_ba_poses_workspace bytes                             */
} NarutoBAPoses;
size_t naruto_ba_poses_workspace(const NarutoField* f, uint32_t n_rays, uint32_t n_samples);
int naruto_ba_poses_init(const NarutoBAPoses* b, void* stream);
int naruto_train_backward_poses(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoGrads* g,
                                uint32_t flags, const NarutoFusedAdam* opt, const NarutoBAPoses* bap /* NULL: off */, void* stream);
/* host only (nothing is launched, no GPU needed; tests/test_ba_poses_host.py):
 * naruto_debug_ba_poses_check: the argument checks naruto_train_backward_poses applies to bap for a batch of n_rays rays.
 * naruto_debug_ba_poses_fields: the struct as the library reads it, field by field in declaration order (floats as their bits).
 * naruto_debug_pose_adam: one step (number `step`, 1-based) of the kernels' own Adam on a pose [6], its gradient and moments, in place.
 * naruto_debug_ba_pose_sums: pose `pose`'s sums of one batch in the accumulation kernel's order, ADDED to sums [12] (host arrays
 *   throughout); grad [6] (optional, needs pose6 [6]): (d_omega, d_t) from the sums as the pose step forms it. */
int naruto_debug_ba_poses_check(const NarutoBAPoses* b, uint32_t n_rays);
int naruto_debug_ba_poses_fields(const NarutoBAPoses* b, NARUTO_HOST uint64_t out[25]);
int naruto_debug_pose_adam(NARUTO_HOST float* pose, NARUTO_HOST const float* grad, NARUTO_HOST float* exp_avg, NARUTO_HOST float* exp_avg_sq, int32_t step,
                           float lr_rot, float lr_trans,
                           float beta1, float beta2, float eps);
int naruto_debug_ba_pose_sums(uint32_t n_rays, const int64_t* ids, uint32_t n_ids, const uint32_t* src_rows, uint32_t n_poses, uint32_t pose,
                              const float* rays_d, const float* d_rays_o, const float* d_rays_d, const float* pose6, double* sums, float* grad);

/* Mesh culling: the step between save_mesh and eval_recon.py of the reference's evaluation protocol (scripts/evaluation/eval_replica.sh:55-72;
 * cull_mesh.py --remove_occlusion is third-party code outside the reference tree: parity unpinned, the contract is restated in
 * naruto_amd/culling.py and csrc/naruto_cull.hip).  Camera: x right, y up, looking along -z; pixel (i, j) has the ray
 * ((i - cx)/fx, -(j - cy)/fy, -1).  Poses are row-major float32 camera-to-world [4,4].  All pointers are device memory.
 *   render depth        float32 [n_poses,H,W] depth maps (z along the viewing axis) of a double-sided mesh, one per pose; +inf where nothing is
 *                       hit inside (near, far).  face_mask (optional uint8 [F]): faces with 0 are not drawn.  A triangle whose candidate pixel
 *                       box has more than large_threshold pixels is spread over workgroups in 2048-pixel chunks (a second launch); the result
 *                       does not depend on the threshold, nor on anything else about the launch: every bit is fixed by the arithmetic.
 *   observed vertices   mask[v] |= 1 where vertex v is in the frustum of one of the poses and (depth given) zc < depth[pose, j, i] + eps
 *   cull faces          face_keep[f] = (inside NULL or any vertex of f inside) and (observed NULL or any vertex of f observed);
 *                       vertex_used (optional, zeroed first) = 1 on the vertices of kept faces
 *   cull compact        kept faces and used vertices to their rows (face_pos / vertex_pos: INCLUSIVE prefix sums of the flags, int32),
 *                       original order, faces re-indexed; vertices float32 or float64 [V,3], colors optional RGBA8 [V,4] */
typedef struct NarutoCullCam {
    uint32_t H, W;
    float fx, fy, cx, cy;
    float near_, far_;                                /* the depth render only                                       */
} NarutoCullCam;
size_t naruto_render_depth_workspace(uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses);
int naruto_render_depth(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const uint8_t* face_mask,
                        uint32_t n_poses, const float* poses, uint32_t large_threshold, void* workspace, float* depth, void* stream);
int naruto_observed_vertices(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint32_t n_poses, const float* poses, const float* depth, float eps,
                             uint8_t* mask, void* stream);
int naruto_cull_faces(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* observed, const uint8_t* inside, uint8_t* face_keep,
                      uint8_t* vertex_used, void* stream);
int naruto_cull_compact(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* face_keep, const int32_t* face_pos, const uint8_t* vertex_used,
                        const int32_t* vertex_pos, const void* vertices, int vertices_f64, const uint8_t* colors, uint64_t n_out_faces, uint64_t n_out_vertices,
                        int32_t* out_faces, void* out_vertices, uint8_t* out_colors, void* stream);
/* Measurement aid (tools/time_cull.py): n_lanes lanes (rounded up to workgroups of 256) each issue `iters` integer atomicMin at hashed
 * addresses of buf [n_words] with values that fall per iteration: the rate of scattered 4-byte integer atomics, without a rasteriser. */
int naruto_debug_atomic_min_rate(uint64_t n_words, uint32_t n_lanes, uint32_t iters, uint32_t* buf, void* stream);

/* Mesh subdivision: trimesh.remesh.subdivide_to_size, which the protocol's cull_mesh.py runs before the vertex test (third-party code outside
 * the reference tree: parity unpinned; the contract is restated in naruto_amd/remesh.py and csrc/naruto_subdiv.hip).  One generation splits
 * 1 -> 4 at the edge midpoints every face that has an edge longer than max_edge and leaves the others; the host repeats it.  All pointers
 * are device memory; the two prefix sums between the calls are the caller's (INCLUSIVE, int32).
 *   arithmetic   in the vertices' own type (float32, or float64 with vertices_f64), products and sums rounded, no contraction:
 *                an edge (a, b) is long iff ((dx*dx + dy*dy) + dz*dz) > max_edge*max_edge, d = v[b] - v[a], max_edge converted to the type
 *                once; the comparison is strict and false for NaN.  midpoint = (v[lo] + v[hi]) * 0.5; colour = (c[lo] + c[hi] + 1) >> 1
 *                per RGBA8 channel.
 *   mark         flags[f] = 1 iff face f has a long edge (a face with an index >= n_vertices is never long)
 *   edges        rank = prefix sum of flags, n_long = its last element.  The slots of the long faces, ordinal 3 * (rank[f] - 1) + k for
 *                the edges k = (v0v1), (v1v2), (v2v0), are keyed by their undirected edge in an open-addressing table of table_slots
 *                cells (>= 6 n_long: at most half full) in the workspace; own[s] (uint8 [3 n_long]) = 1 iff s is the LOWEST ordinal that
 *                carries its edge.  Integer atomics only (64-bit compare-and-swap, 32-bit minimum): own depends on the mesh alone, not on
 *                table_slots nor on anything about the launch.  The probe loop is bounded by table_slots.
 *   emit         mid_rank = prefix sum of own, n_mid = its last element: the midpoints in order of first appearance in the face-major edge
 *                list.  vertices [n_vertices + n_mid, 3] (and colors RGBA8 [n_vertices + n_mid, 4], optional) hold the existing rows on
 *                entry; midpoint number j is written to row n_vertices + j.  out_faces [n_faces + 3 n_long, 3]: the faces that are not
 *                long first, in their order and unchanged, then the children (v0,m0,m2) (m0,v1,m1) (m2,m1,v2) (m0,m1,m2) of every long
 *                face in the long faces' order, m_k the midpoint of edge k.  The workspace is the one edges filled.
 *   The workspace's first uint32 is an error word, zeroed by edges: bit 0 = an edge found no cell, bit 1 = flags, rank, mid_rank or the
 *   counts contradict each other (the lane then writes nothing out of range).  The caller reads it with n_mid.  The workspace query
 *   returns 0 beyond the supported sizes: n_long in 1 .. (2^31-1)/3, table_slots in 6 n_long .. 2^31. */
size_t naruto_subdivide_workspace(uint64_t n_long, uint64_t table_slots);
int naruto_subdivide_mark(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const void* vertices, int vertices_f64, double max_edge, uint8_t* flags,
                          void* stream);
int naruto_subdivide_edges(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* flags, const int32_t* rank, uint64_t n_long, uint64_t table_slots,
                           void* workspace, uint8_t* own, void* stream);
int naruto_subdivide_emit(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* flags, const int32_t* rank, uint64_t n_long, uint64_t table_slots,
                          void* workspace, const int32_t* mid_rank, uint64_t n_mid, void* vertices, int vertices_f64, uint8_t* colors, int32_t* out_faces, void* stream);

/* Mesh simulator: a mesh in the place of the reference's HabitatSim (src/simulator/habitat_simulator.py; an external renderer that is not
 * on this stack: parity unpinned; the contract is restated in naruto_amd/simulator.py and csrc/naruto_sim.hip).  Camera and poses as for
 * the culling above.  All pointers are device memory.
 *   render rgbd     the depth render with the winning face per pixel (among the faces whose depth equals the minimum in every bit, the
 *                   lowest index) and its vertex colours interpolated perspective-correctly: depth float32 [n_poses,H,W], color float32
 *                   [n_poses,H,W,3], face_id int32 [n_poses,H,W]; any of the three may be NULL.  colors: RGBA8 words [V] (c = byte/255) or,
 *                   with colors_f32, float32 [V,3]; needed iff color is asked for.  Nothing hit: depth 0 (+inf with NARUTO_SIM_KEEP_INF),
 *                   colour 0, id -1.  Independent of large_threshold and of the launch, as render depth is.
 *   cube to erp     erp[c][k] = cube[c][table[k]]: a nearest gather of [C,6,s,s] 32-bit words to [C,n_erp] through an index table
 *                   (naruto_amd.simulator.cube_table restates the reference's C2E, src/layers/c2e.py); entries must lie in [0, 6 s^2)
 *   depth to dist   dist = depth * sqrt(dx^2 + dy^2 + 1), dx = (i - cx)/fx, dy = (j - cy)/fy (erp_conversions.depth2dist), [n_images,H,W]
 *   sim erp         per panorama: six cube planes of depth [6,s,s] (rendered with fx = fy = cx = cy = (s-1)/2; 0 or +inf = nothing hit) and
 *                   optionally colour [6,s,s,3] -> radial distance [n_erp] (1e8 * ray norm where nothing is hit), colour [n_erp,3], and
 *                   stats uint32 [2]: the bit pattern of the minimum distance and the number of pixels with distance > invalid_thre.
 *                   erp_dist, erp_color and stats may each be NULL.
 *   textures        every texture's mip chain in ONE buffer of RGBA8 words (R in the lowest byte), texture after texture, level after
 *                   level; desc uint32 [n_textures][4] = word offset of level 0, W, H, n_levels = 1 + floor(log2(max(W, H))).  Level l+1 has
 *                   max(1, w >> 1) x max(1, h >> 1) texels; per channel, alpha included, texel (x, y) of it is
 *                   (t(xa,ya) + t(xb,ya) + t(xa,yb) + t(xb,yb) + 2) >> 2 with xa = min(2x, w-1), xb = min(2x+1, w-1), ya and yb likewise.
 *                   tex bytes: the bytes of ONE texture's chain (0: a side outside 1 .. 16384).  tex build: copies level0 (W x H words,
 *                   row-major from the first stored row; host or device memory) to word `offset` of texels, builds the texture's levels
 *                   behind it on the device in integer arithmetic, writes its four descriptor words to desc, and returns when all is
 *                   done.  All chains together stay below 2^32 words: descriptors hold 32-bit offsets.
 *   render rgbd tex render rgbd with materials (NarutoSimTextures; every pointer in it is device memory): depth and face id are render
 *                   rgbd's bits.  The colour of a hit pixel by its face's material face_material[f]:
 *                     -1 or out of range, or a texture index >= n_textures: render rgbd's vertex colours, in the same bits;
 *                     a material without a texture (index < 0): factor.rgb;
 *                     a texture: fp32, each operation rounded, no contraction -- u = (w_a*u_a + w_b*u_b) + w_c*u_c (v likewise) with render
 *                     rgbd's barycentrics; the same expression at the rays of pixels (i+1, j) and (i, j+1) with the same face's edge values
 *                     gives (u_x, v_x), (u_y, v_y); ax = (u_x - u)*W, bx = (v_x - v)*H, rx = ax*ax + bx*bx, ry likewise; rho2 = rx, or ry
 *                     where ry > rx; level = the number of k in 0 .. n_levels-2 with rho2 > 4^k (NaN: 0).  One bilinear tap at that level
 *                     (w, h): x = u*w - 0.5f, y = v*h - 0.5f; unless |x| < 2^30 and |y| < 2^30 the texel colour is 0; x0 = floor(x),
 *                     a = x - x0 (y0, b likewise); the indices x0, x0+1, y0, y0+1 wrapped by the axis's mode -- REPEAT 10497 (and any other
 *                     value): mod w; MIRRORED_REPEAT 33648: m = mod 2w, m < w ? m : 2w-1-m; CLAMP_TO_EDGE 33071: clamp to [0, w-1] --
 *                     t = byte/255.0f, top = t00 + a*(t10 - t00), bot = t01 + a*(t11 - t01), c = top + b*(bot - top); colour = c * factor.
 *                   Alpha is stored and ignored: blended and masked materials render opaque.  One level per pixel: no trilinear blend.
 *                   materials uint32 [n_materials][8] = texture index (int32), wrap_s, wrap_t, 0, factor[4] (float32).  The kernel trusts
 *                   no index it reads from memory; a NarutoSimTextures whose struct_size is below sizeof(NarutoSimTextures) is refused. */
#define NARUTO_SIM_KEEP_INF 1u
typedef struct NarutoSimTextures {
    uint32_t struct_size;                             /* sizeof(NarutoSimTextures)                                   */
    uint32_t n_materials, n_textures;
    uint32_t reserved_;                               /* 0                                                           */
    uint64_t n_texels;                                /* words in texels                                             */
    const float* uv;                                  /* [V,2]                                                       */
    const int32_t* face_material;                     /* [F], -1: none                                               */
    const uint32_t* materials;                        /* [n_materials][8]                                            */
    const uint32_t* tex_desc;                         /* [n_textures][4]                                             */
    const uint32_t* texels;                           /* [n_texels]                                                  */
} NarutoSimTextures;
size_t naruto_tex_bytes(uint32_t W, uint32_t H);
int naruto_tex_build(uint32_t W, uint32_t H, uint64_t offset, const void* level0, uint32_t* desc, uint32_t* texels, void* stream);
int naruto_render_rgbd_tex(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
                           uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
                           const NarutoSimTextures* tex, void* stream);
size_t naruto_render_rgbd_workspace(uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses, uint32_t H, uint32_t W);
int naruto_render_rgbd(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
                       uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
                       void* stream);
int naruto_cube_to_erp(uint32_t n_channels, uint32_t face_w, uint64_t n_erp, const int32_t* table, const void* cube, void* erp, void* stream);
int naruto_depth_to_dist(uint32_t n_images, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy, const float* depth, float* dist, void* stream);
int naruto_sim_erp(uint32_t n_panoramas, uint32_t face_w, uint64_t n_erp, const int32_t* table, const float* cube_depth, const float* cube_color, float invalid_thre,
                   float* erp_dist, float* erp_color, uint32_t* stats, void* stream);
/* Measurement aid (tools/time_sim.py): naruto_debug_atomic_min_rate on 8-byte cells, the winner raster's access pattern. */
int naruto_debug_atomic_min64_rate(uint64_t n_cells, uint32_t n_lanes, uint32_t iters, uint64_t* buf, void* stream);

/* Whole views from the field and their 2D scores (Co-SLAM's render_img is not in the reference tree and the surface search is this library's
 * own: parity unpinned; the contract is restated in naruto_amd/render.py and csrc/naruto_view.hip).  Camera and poses as for the culling
 * above; a flat pixel p of n_poses views is pose p / (H W), row (p % (H W)) / W, column p % W.  All pointers are device memory unless noted.
 *   view rays       rays_o / rays_d [p1 - p0, 3] of the flat pixels [p0, p1): the camera-frame direction ((i - cx)/fx, -(j - cy)/fy, -1), each
 *                   operation rounded once, rotated as naruto_rays_to_world does it
 *   view crossing   z_star[n] = z[k] + (z[k+1] - z[k]) * (sdf[k] / (sdf[k] - sdf[k+1])) at the first k with sdf[k] > 0 and !(sdf[k+1] > 0)
 *                   (sdf = raw[n,:,3]; float32, every operation rounded, no contraction); 0 where there is none
 *   render view     ONE launch, one wave per ray: ray, coarse pass of n_coarse uniform depths in [near, far] (skipped when target_d is given:
 *                   then z* = target_d), crossing, naruto_render_fwd's depth-guided pass around z* without jitter, compositing.  Outputs
 *                   are whole images [n_poses,H,W(,3)] written at the flat pixels of the range; any may be NULL.  Both sample counts must
 *                   lie in 2 .. 1024 (naruto_render_fwd's per-ray limit): NARUTO_ERR_INVALID otherwise.  The fine pass runs in the tiles
 *                   naruto_render_fwd's four-wave launch forms over the same rays (for at most 64 fine samples: groups of 16 rays counted
 *                   from p0, whose samples share 64-sample tiles), and equals it in every bit; a caller who wants bits that do not move
 *                   with the ranges starts every range at a multiple of 16.
 *   image metrics   out float64 [n_views,6] = sum of squared colour errors, pixels, sum of |d - d_gt| over the valid pixels (d_gt > 0 and,
 *                   with has_depth_trunc, d_gt <= depth_trunc), valid pixels, sum of SSIM, SSIM terms.  window: HOST array of the 11
 *                   normalised Gaussian taps.  Optional float64 maps: squared error [n_views,H,W,3], absolute depth error [n_views,H,W]
 *                   (0 where invalid), SSIM [n_views,H-10,W-10,3].  Per-workgroup partials and one finishing pass in a fixed order, no
 *                   atomics: bitwise reproducible.  workspace: naruto_image_metrics_workspace() bytes (0: unsupported sizes). */
typedef struct NarutoViewRender {
    uint32_t n_poses; const float* poses;             /* [n_poses,4,4]                                               */
    uint32_t p0, p1;                                  /* flat pixels [p0, p1) of the launch                          */
    const float* target_d;                            /* [n_poses,H,W] sensor depth, or NULL: search the surface     */
    uint32_t n_samples_d, n_range_d; float range_d;   /* the fine pass (training.n_samples_d / n_range_d / range_d)  */
    uint32_t n_coarse;
    float *rgb, *depth, *acc, *depth_var, *uncert_map, *surface_z;
} NarutoViewRender;
int naruto_view_rays(const NarutoCullCam* cam, uint32_t n_poses, const float* poses, uint32_t p0, uint32_t p1, float* rays_o, float* rays_d, void* stream);
int naruto_view_crossing(uint32_t n_rays, uint32_t n_samples, const float* raw, const float* z_vals, float* z_star, void* stream);
int naruto_render_view(const NarutoField* f, const NarutoParams* p, const NarutoCullCam* cam, const NarutoViewRender* r, void* stream);
size_t naruto_image_metrics_workspace(uint32_t n_views, uint32_t H, uint32_t W);
int naruto_image_metrics(uint32_t n_views, uint32_t H, uint32_t W, const float* rgb, const float* depth, const float* gt_rgb, const float* gt_depth, int has_depth_trunc,
                         float depth_trunc, NARUTO_HOST const double* window, void* workspace, double* out, double* se_map, double* de_map, double* ssim_map, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NARUTO_HIP_H */
