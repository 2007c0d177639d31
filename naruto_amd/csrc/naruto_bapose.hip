// Pose refinement inside global_BA (reference coslam.py:256-281, 342-344, 378-407; parity unpinned -- get_pose_param_optim and
// matrix_from_tensor are Co-SLAM functions that are not in the reference tree, the loop around them is the contract).  Per call with
// P poses (the current frame's last):
//   * pose 0 is fixed; poses 1 .. P-2 are parameters; pose P-1 is one iff mapping.optim_cur.  A parameter pose is (omega, t): the absolute
//     axis-angle of the camera-to-world rotation and the translation; its rays are formed from R(omega) (Rodrigues) from the first iteration on.
//   * every iteration the gradient of the iteration's total loss w.r.t. the rays (k_query_bwd_points, k_ray_point_reduce) is summed per pose
//     into fp64 accumulators -- d_t[p] = sum d_rays_o[r], H[p] = sum d_rays_d[r] (x) rays_d[r] over the rays r of pose p -- in a fixed order,
//     without atomics.  The poses are constant between two pose steps and rays_d = R d_cam, so dL/dR = (sum d_rays_d (x) d_cam) = H R: the
//     world-frame directions stand in for the camera-frame ones, which need not follow the rays through the selection (at the price of
//     rays_d's fp32 rounding, 6e-8 relative).
//   * after the iterations with (i + 1) % pose_accum_step == 0: d_omega = rodrigues_vjp(omega, H R) (the VJP is linear in its cotangent, so
//     this is the accumulated omega.grad), ONE torch.optim.Adam step on every parameter pose with a shared step count (a pose that drew no
//     ray has gradient 0 and is still stepped), the accumulators are zeroed, and the new [4,4] rows land in the pose buffer the ray
//     assembly reads: every later batch of the call is formed from the new poses.
// Kernels:
//   k_ba_pose_init   per call: (omega, t) <- the caller's, moments / accumulators / state zeroed, the parameter poses' matrices from R(omega)
//                    (fixed poses keep the caller's matrix bits)
//   k_ba_pose_accum  one workgroup per parameter pose scans the batch's pose ids (k_track_step's tree)
//   k_ba_pose_step   ONE workgroup: counts the iteration and, when a pose step is due, steps every pose
#pragma once

#include "naruto_common.h"
#include "naruto_pose.h"

namespace naruto {

constexpr int kBaPoseThreads = 256;

struct BAPoseArgs {
    uint32_t max_poses;          // capacity of the per-pose buffers and of poses
    int32_t optim_cur;
    uint32_t accum_step;         // mapping.pose_accum_step
    const uint64_t* dyn;         // {n_kf, n_poses, n_cur_pop}: P = dyn[1]
    float* poses;                // [max_poses,4,4] row-major camera-to-world: what the ray assembly reads
    const float* pose_init;      // [max_poses,6] the caller's (omega, t)
    float* pose6; float* exp_avg; float* exp_avg_sq;      // [max_poses,6]
    double* accum;               // [max_poses,12] d_t[3] | H[9]
    int32_t* state;              // {pose steps of this call, iterations of this call, 0, 0}
    const int64_t* ids;          // [n_ids] pose id of every assembled row, -1 = the current frame (pose P-1)
    uint32_t n_ids;
    const uint32_t* src_rows;    // optional [n_rays]: the assembled row each training ray came from (active ray selection); NULL: row r
    uint32_t n_rays;
    const float* rays_d; const float* d_rays_o; const float* d_rays_d;      // [n_rays,3]
    float lr_rot, lr_trans, beta1, beta2, eps;
    float* trace_pose; float* trace_grad; uint32_t max_trace;               // optional [max_trace,max_poses,6] x2
};

__host__ __device__ inline uint32_t ba_n_poses(uint64_t dyn1, uint32_t max_poses) { return dyn1 < (uint64_t)max_poses ? (uint32_t)dyn1 : max_poses; }
// coslam.py:273-281: every keyframe but the first, and the current frame (the last pose) with mapping.optim_cur
__host__ __device__ inline bool ba_is_param(uint32_t p, uint32_t P, int32_t optim_cur) { return p >= 1u && p < P && (p + 1u < P || optim_cur != 0); }

// ray r's contribution to pose p's sums (nothing if the ray belongs to another pose)
__host__ __device__ inline void ba_row_add(double acc[12], uint32_t p, uint32_t P, uint32_t r, const int64_t* ids, uint32_t n_ids, const uint32_t* src_rows,
                                           const float* rays_d, const float* d_rays_o, const float* d_rays_d) {
    const uint32_t row = src_rows != nullptr ? src_rows[r] : r;
    if (row >= n_ids) return;
    int64_t id = ids[row];
    if (id < 0) id = (int64_t)P - 1;
    if (id != (int64_t)p) return;
    float rd[3], dro[3], drd[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { rd[d] = rays_d[3 * (size_t)r + d]; dro[d] = d_rays_o[3 * (size_t)r + d]; drd[d] = d_rays_d[3 * (size_t)r + d]; }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        acc[d] += (double)dro[d];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 + 3 * d + j] += (double)drd[d] * (double)rd[j];
    }
}

// the accumulated (d_omega, d_t) of the pose (omega, t) = pose6 from its sums: G = H R(omega), d_omega = rodrigues_vjp(omega, G)
__host__ __device__ inline void ba_pose_grad(const float pose6[6], const double acc[12], float g[6]) {
    const double w[3] = {(double)pose6[0], (double)pose6[1], (double)pose6[2]};
    double R[9], G[9], dw[3];
    rodrigues(w, R);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += acc[3 + 3 * i + k] * R[3 * k + j];
            G[3 * i + j] = s;
        }
    rodrigues_vjp(w, G, dw);
    g[0] = (float)dw[0]; g[1] = (float)dw[1]; g[2] = (float)dw[2];
    g[3] = (float)acc[0]; g[4] = (float)acc[1]; g[5] = (float)acc[2];
}

__global__ __launch_bounds__(kBaPoseThreads) void k_ba_pose_init(BAPoseArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t P = ba_n_poses(a.dyn[1], a.max_poses);
    if (p == 0u) { a.state[0] = 0; a.state[1] = 0; a.state[2] = 0; a.state[3] = 0; }
    if (p >= P) return;
    float q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        q[k] = a.pose_init[6 * (size_t)p + k];
        a.pose6[6 * (size_t)p + k] = q[k];
        a.exp_avg[6 * (size_t)p + k] = 0.0f;
        a.exp_avg_sq[6 * (size_t)p + k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) a.accum[12 * (size_t)p + k] = 0.0;
    if (ba_is_param(p, P, a.optim_cur)) track_write_c2w(a.poses + 16 * (size_t)p, q);
}

// workgroup p: the rays of pose p, thread t taking rays t, t + 256, ...; then the tree; added to the window's sums
__global__ __launch_bounds__(kBaPoseThreads) void k_ba_pose_accum(BAPoseArgs a) {
    __shared__ double red[kBaPoseThreads][12];
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint32_t P = ba_n_poses(a.dyn[1], a.max_poses);
    if (!ba_is_param(p, P, a.optim_cur)) return;           // workgroup-uniform
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (uint32_t r = tid; r < a.n_rays; r += kBaPoseThreads) ba_row_add(acc, p, P, r, a.ids, a.n_ids, a.src_rows, a.rays_d, a.d_rays_o, a.d_rays_d);
#pragma unroll
    for (int k = 0; k < 12; ++k) red[tid][k] = acc[k];
    __syncthreads();
    for (uint32_t h = kBaPoseThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 12; ++k) red[tid][k] += red[tid + h][k];
        }
        __syncthreads();
    }
    if (tid < 12u) a.accum[12 * (size_t)p + tid] += red[0][tid];
}

__global__ __launch_bounds__(kBaPoseThreads) void k_ba_pose_step(BAPoseArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint32_t P = ba_n_poses(a.dyn[1], a.max_poses);
    const int32_t n_steps = a.state[0], it = a.state[1];
    const bool due = a.accum_step != 0u && ((uint32_t)(it + 1) % a.accum_step) == 0u;
    __syncthreads();                                       // every thread has read the state before thread 0 writes it
    if (tid == 0u) { a.state[1] = it + 1; if (due) a.state[0] = n_steps + 1; }
    if (!due) return;
    const bool trace = a.trace_pose != nullptr && (uint32_t)n_steps < a.max_trace;
    for (uint32_t p = tid; p < P; p += kBaPoseThreads) {
        float q[6], g[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = a.pose6[6 * (size_t)p + k];
        const bool param = ba_is_param(p, P, a.optim_cur);
        if (param) {
            double acc[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) { acc[k] = a.accum[12 * (size_t)p + k]; a.accum[12 * (size_t)p + k] = 0.0; }
            ba_pose_grad(q, acc, g);
        }
        if (trace) {
            const size_t o = 6 * ((size_t)n_steps * a.max_poses + p);
#pragma unroll
            for (int k = 0; k < 6; ++k) { a.trace_pose[o + k] = q[k]; a.trace_grad[o + k] = g[k]; }
        }
        if (!param) continue;
        float m[6], v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { m[k] = a.exp_avg[6 * (size_t)p + k]; v[k] = a.exp_avg_sq[6 * (size_t)p + k]; }
        pose_adam_step(q, g, m, v, n_steps + 1, a.lr_rot, a.lr_trans, a.beta1, a.beta2, a.eps);
#pragma unroll
        for (int k = 0; k < 6; ++k) { a.exp_avg[6 * (size_t)p + k] = m[k]; a.exp_avg_sq[6 * (size_t)p + k] = v[k]; a.pose6[6 * (size_t)p + k] = q[k]; }
        track_write_c2w(a.poses + 16 * (size_t)p, q);
    }
}

}  // namespace naruto
