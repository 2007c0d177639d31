// Camera tracking (Co-SLAM tracking_render, called at coslam.py:594-602; parity unpinned -- the function is not in the reference tree):
// the pose of ONE frame is optimised with the network frozen.  Per call:
//   k_track_draw   tracking.sample distinct interior pixels (keyed Feistel permutation, naruto_rays.hip) -> d_cam, target_rgb, target_d
//   k_track_rays   state reset + iteration 0's rays from the initial pose
// and per iteration, after the training forward, the loss backward + compaction and the point gradients (k_query_bwd_points,
// k_ray_point_reduce):
//   k_track_step   ONE workgroup: d_t = sum_r d_rays_o[r], G = sum_r d_rays_d[r] (x) d_cam[r] in a fixed order (no atomics), d_omega as the
//                  VJP of Rodrigues' formula, the best-pose / wait_iters bookkeeping, one torch.optim.Adam step, and the NEXT iteration's rays.
// The pose is an absolute axis-angle omega of the camera-to-world rotation plus the translation t; R(omega) = exp([omega]x): the pose
// arithmetic (Rodrigues, its VJP, the Adam step) lives in naruto_pose.h, shared with naruto_bapose.hip.
#pragma once

#include "naruto_common.h"
#include "naruto_pose.h"

namespace naruto {

constexpr int kTrackStepThreads = 256;

struct TrackArgs {
    uint32_t n_rays;
    uint32_t H, W, edge_h, edge_w;
    const float* direction; const float* rgb; const float* depth;      // the frame [H,W,3] [H,W,3] [H,W]
    uint64_t* rng;                                                      // {seed, counter}
    float* d_cam; int64_t* pix;
    float* target_rgb; float* target_d;
    float* rays_o; float* rays_d;
    const float* pose_init;
    float* pose; float* exp_avg; float* exp_avg_sq;
    int32_t* state;                                                     // {step, thresh, stopped, iteration}
    float lr_rot, lr_trans, beta1, beta2, eps;
    uint32_t wait_iters; int32_t best;
    float* best_pose; float* best_loss; float* c2w;
    const float* d_rays_o; const float* d_rays_d;
    const float* losses;
    float* trace_loss; float* trace_pose; float* trace_d_pose; uint32_t max_trace;
};

// rays_o[r] = t, rays_d[r] = R d_cam[r] in fp32, in the order of coslam.py:343 (torch.sum(d[..., None, :] * R, -1)): three rounded
// products added left to right.  Contraction is switched off for it: the clang HIP headers define __fmul_rn / __fadd_rn as the plain
// operators, and hipcc fused the first two terms into one fma (tests/tracking_spec.py: rays_from_pose is the contract)
__device__ __forceinline__ void track_write_ray(const TrackArgs& a, uint32_t r, const float Rf[9], const float t[3]) {
#pragma clang fp contract(off)
    const float dx = a.d_cam[3 * (size_t)r], dy = a.d_cam[3 * (size_t)r + 1], dz = a.d_cam[3 * (size_t)r + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a.rays_d[3 * (size_t)r + i] = (dx * Rf[3 * i] + dy * Rf[3 * i + 1]) + dz * Rf[3 * i + 2];
        a.rays_o[3 * (size_t)r + i] = t[i];
    }
}

// row i of the draw: flat interior index k = perm(i) -> h = edge_h + k % Hi (h fastest, Co-SLAM's order), w = edge_w + k / Hi
__global__ __launch_bounds__(256) void k_track_draw(TrackArgs a, uint64_t n_int, uint32_t half_bits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rays) return;
    const uint64_t key = mix_key(a.rng[0], a.rng[1], 4);
    const uint64_t k = perm_index(i, n_int, half_bits, key);
    const uint32_t Hi = a.H - 2u * a.edge_h;
    const uint64_t h = a.edge_h + k % Hi, w = a.edge_w + k / Hi;
    const uint64_t px = h * a.W + w;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a.d_cam[3 * (size_t)i + d] = a.direction[3 * px + d];
        a.target_rgb[3 * (size_t)i + d] = a.rgb[3 * px + d];
    }
    a.target_d[i] = a.depth[px];
    if (a.pix != nullptr) a.pix[i] = (int64_t)px;
}

// zero fill of the per-point gradient rows k_query_bwd_points leaves alone (the samples off the active list) -- a kernel, not a memset
// node, so that a captured call is one chain of kernel nodes
__global__ __launch_bounds__(256) void k_track_zero(float* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0.0f;
}

// the call's state from the initial pose (one thread) + iteration 0's rays; advances the draw's counter for the next call
__global__ __launch_bounds__(256) void k_track_rays(TrackArgs a) {
    float p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = a.pose_init[k];
    float Rf[9];
    track_pose_matrix(p, Rf);
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < a.n_rays) track_write_ray(a, r, Rf, p + 3);
    if (r == 0) {
        for (int k = 0; k < 6; ++k) {
            a.pose[k] = p[k]; a.best_pose[k] = p[k]; a.exp_avg[k] = 0.0f; a.exp_avg_sq[k] = 0.0f;
        }
        a.state[0] = 0; a.state[1] = 0; a.state[2] = 0; a.state[3] = 0;
        a.best_loss[0] = __int_as_float(0x7F800000);
        track_write_c2w(a.c2w, p);
        a.rng[1] += 1ull;
    }
}

// after the point gradients of iteration i = state[3]: see the file header
__global__ __launch_bounds__(kTrackStepThreads) void k_track_step(TrackArgs a) {
    __shared__ double red[kTrackStepThreads][12];
    __shared__ float s_next[16];            // Rf[9] | t[3] of the next pose | go on
    const uint32_t tid = threadIdx.x;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (uint32_t r = tid; r < a.n_rays; r += kTrackStepThreads) {
        float dc[3], dro[3], drd[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            dc[d] = a.d_cam[3 * (size_t)r + d]; dro[d] = a.d_rays_o[3 * (size_t)r + d]; drd[d] = a.d_rays_d[3 * (size_t)r + d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            acc[d] += (double)dro[d];
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 + 3 * d + j] += (double)drd[d] * (double)dc[j];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) red[tid][k] = acc[k];
    __syncthreads();
    for (uint32_t h = kTrackStepThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 12; ++k) red[tid][k] += red[tid + h][k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int32_t it = a.state[3];
        a.state[3] = it + 1;
        s_next[15] = 0.0f;
        if (a.state[2] == 0) {
            float p[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) p[k] = a.pose[k];
            const double w[3] = {(double)p[0], (double)p[1], (double)p[2]};
            double G[9], dw[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) G[k] = red[0][3 + k];
            rodrigues_vjp(w, G, dw);
            const float g[6] = {(float)dw[0], (float)dw[1], (float)dw[2], (float)red[0][0], (float)red[0][1], (float)red[0][2]};
            const float L = a.losses[9];
            if (a.trace_loss != nullptr && (uint32_t)it < a.max_trace) {
                a.trace_loss[it] = L;
                for (int k = 0; k < 6; ++k) { a.trace_pose[6 * it + k] = p[k]; a.trace_d_pose[6 * it + k] = g[k]; }
            }
            // Co-SLAM's order: the first loss is the best so far, then the comparison (which the first loss fails: thresh = 1)
            float best = it == 0 ? L : a.best_loss[0];
            if (it == 0)
                for (int k = 0; k < 6; ++k) a.best_pose[k] = p[k];
            int32_t thresh = a.state[1];
            if (L < best) {
                best = L;
                for (int k = 0; k < 6; ++k) a.best_pose[k] = p[k];
                thresh = 0;
            } else {
                thresh += 1;
            }
            a.best_loss[0] = best;
            a.state[1] = thresh;
            if (a.best) {
                float bp[6];
                for (int k = 0; k < 6; ++k) bp[k] = a.best_pose[k];
                track_write_c2w(a.c2w, bp);
            } else {
                track_write_c2w(a.c2w, p);          // the pose evaluated last: Co-SLAM recomputes c2w_est before the step
            }
            if ((uint32_t)thresh > a.wait_iters) {
                a.state[2] = 1;
            } else {
                // torch.optim.Adam (pose_adam_step, naruto_pose.h)
                const int32_t step = a.state[0] + 1;
                a.state[0] = step;
                float m[6], v[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) { m[k] = a.exp_avg[k]; v[k] = a.exp_avg_sq[k]; }
                pose_adam_step(p, g, m, v, step, a.lr_rot, a.lr_trans, a.beta1, a.beta2, a.eps);
#pragma unroll
                for (int k = 0; k < 6; ++k) { a.exp_avg[k] = m[k]; a.exp_avg_sq[k] = v[k]; a.pose[k] = p[k]; }
                float Rf[9];
                track_pose_matrix(p, Rf);
                for (int k = 0; k < 9; ++k) s_next[k] = Rf[k];
                for (int k = 0; k < 3; ++k) s_next[9 + k] = p[3 + k];
                s_next[15] = 1.0f;
            }
        }
    }
    __syncthreads();
    if (s_next[15] == 0.0f) return;
    float Rf[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rf[k] = s_next[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = s_next[9 + k];
    for (uint32_t r = tid; r < a.n_rays; r += kTrackStepThreads) track_write_ray(a, r, Rf, t);
}

}  // namespace naruto
