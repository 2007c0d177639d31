// Co-SLAM's pose chain on the device: what a tracked run does to est_c2w_data / est_c2w_data_rel between the tracker and global_BA
// (reference coslam.py:595-602 tracks every frame, :264-281 / :401-407 refine the keyframe poses and write them back; Co-SLAM's
// predict_current_pose, tracking_render's relative pose and convert_relative_pose are not in the reference tree: parity unpinned, the
// contract is restated here).  With kf(i) = (i / keyframe_every) * keyframe_every:
//
//   log      (omega, t) of P matrices: the initial poses of a refining global_BA call (naruto_amd.tracking.matrices_to_pose6)
//   predict  est[i] = est[i-1]                                   (i == 1, or const_speed off)
//            est[i] = (est[i-1] @ inv(est[i-2])) @ est[i-1]      (the last motion once more)
//            and the tracker's initial (omega, t) = log of the ROUNDED est[i]
//   commit   est[i] = the tracker's result; rel[i] = est[i] @ inv(est[kf(i)]) for a frame that is no keyframe
//   scatter  est[k * keyframe_every] = refined[k], k = 1 .. P-2; est[cur_id] = refined[P-1] iff optim_cur (row 0 is never written)
//   resolve  out[i] = est[i] for a keyframe, rel[i] @ est[kf(i)] otherwise: where a frame stands after its keyframe was refined
//
// All arithmetic in fp64 from the fp32 matrices, every output rounded once (naruto_pose.h); copies move the bits.  One thread per pose,
// no atomics, nothing read back: a tracked frame never waits for the host.
#pragma once

#include "naruto_common.h"
#include "naruto_pose.h"

namespace naruto {

constexpr uint32_t kPoseChainThreads = 64;

__device__ inline void pose_copy(float* dst, const float* src) {
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k] = src[k];
}

__global__ __launch_bounds__(kPoseChainThreads) void k_pose_log(uint32_t P, const float* __restrict__ c2w, float* __restrict__ pose6) {
    const uint32_t p = blockIdx.x * kPoseChainThreads + threadIdx.x;
    if (p >= P) return;
    float q[6];
    pose_log(c2w + 16 * (size_t)p, q);
#pragma unroll
    for (int k = 0; k < 6; ++k) pose6[6 * (size_t)p + k] = q[k];
}

__global__ __launch_bounds__(kPoseChainThreads) void k_pose_predict(float* est, uint32_t i, int32_t const_speed, float* __restrict__ pose6_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float next[16];
    if (i == 1u || const_speed == 0) {
        pose_copy(next, est + 16 * (size_t)(i - 1u));
    } else {
        double A[16], B[16], Binv[16], D[16], N[16];
        pose_load(est + 16 * (size_t)(i - 1u), A);
        pose_load(est + 16 * (size_t)(i - 2u), B);
        pose_affine_inverse(B, Binv);
        pose_mul(A, Binv, D);
        pose_mul(D, A, N);
        pose_store(next, N);
    }
    pose_copy(est + 16 * (size_t)i, next);
    float q[6];
    pose_log(next, q);
#pragma unroll
    for (int k = 0; k < 6; ++k) pose6_out[k] = q[k];
}

__global__ __launch_bounds__(kPoseChainThreads) void k_pose_commit(float* est, float* __restrict__ rel, uint32_t i, uint32_t keyframe_every,
                                                                   const float* __restrict__ c2w) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float cur[16];
    pose_copy(cur, c2w);
    pose_copy(est + 16 * (size_t)i, cur);
    if (i % keyframe_every == 0u) return;
    const uint32_t kf = (i / keyframe_every) * keyframe_every;            // < i: another row than the one just written
    double A[16], K[16], Kinv[16], D[16];
    pose_load(cur, A);
    pose_load(est + 16 * (size_t)kf, K);
    pose_affine_inverse(K, Kinv);
    pose_mul(A, Kinv, D);
    pose_store(rel + 16 * (size_t)i, D);
}

__global__ __launch_bounds__(kPoseChainThreads) void k_pose_scatter(float* __restrict__ est, const float* __restrict__ refined, uint32_t P,
                                                                    uint32_t keyframe_every, uint32_t cur_id, int32_t optim_cur) {
    const uint32_t k = blockIdx.x * kPoseChainThreads + threadIdx.x;
    if (k == 0u || k >= P) return;
    if (k + 1u == P) {
        if (optim_cur != 0) pose_copy(est + 16 * (size_t)cur_id, refined + 16 * (size_t)k);
        return;
    }
    pose_copy(est + 16 * ((size_t)k * keyframe_every), refined + 16 * (size_t)k);
}

__global__ __launch_bounds__(kPoseChainThreads) void k_pose_resolve(const float* __restrict__ est, const float* __restrict__ rel, uint32_t n,
                                                                    uint32_t keyframe_every, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPoseChainThreads + threadIdx.x;
    if (i >= n) return;
    if (i % keyframe_every == 0u) {
        pose_copy(out + 16 * (size_t)i, est + 16 * (size_t)i);
        return;
    }
    const uint32_t kf = (i / keyframe_every) * keyframe_every;
    double A[16], K[16], D[16];
    pose_load(rel + 16 * (size_t)i, A);
    pose_load(est + 16 * (size_t)kf, K);
    pose_mul(A, K, D);
    pose_store(out + 16 * (size_t)i, D);
}

}  // namespace naruto
