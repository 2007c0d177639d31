// Rigid mesh alignment on the device: the loop of point-to-point ICP (Open3D's registration_icp with its defaults; the reference's
// evaluation protocol aligns the reconstructed mesh to the ground truth with it before the metrics, src/evaluation/eval_recon.py:80-85
// -> neural_slam_eval's get_align_transformation, third-party code outside the reference tree: PARITY UNPINNED, the contract is
// restated in naruto_amd/evaluation.py).  One iteration is
//   k_icp_transform    p_i = T s_i                      (the ORIGINAL source points by the cumulative fp64 T, rounded to float32 once)
//   naruto_nn_grid_query (naruto_recon.hip)            nearest target and its fp64 distance per p_i, cKDTree.query's bits
//   k_icp_accumulate   17 fp64 sums over the inliers    (dist <= max_correspondence_distance)
//   k_icp_step         one thread: fitness / rmse, the convergence test, dT by Kabsch (naruto_icp.h), T = dT @ T
// and the host reads eight doubles of the state block to learn whether to enqueue another.
//
// Transform arithmetic: coordinates promoted to fp64, out_a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3] with every product and sum
// rounded (no contraction), stored in the output's type.  numpy makes the same bits, and because every evaluation starts from the
// original points nothing drifts across iterations.
//
// Sum order (k_icp_accumulate, k_icp_accumulate_finish): thread t of workgroup b adds points b*2048 + t + 256*k, k = 0..7 in turn; the 256
// partial vectors fold by halves in LDS; the finishing workgroup does the same over the workgroups' vectors.  The order depends on n
// alone: no atomics, bitwise reproducible.  p and q enter relative to a caller-given origin (the target box's centre), so the centred
// cross-covariance sum p q^T - (sum p)(sum q)^T / n does not cancel its leading digits.
#pragma once

#include "naruto_common.h"
#include "naruto_icp.h"

namespace naruto {

constexpr int kIcpThreads = 256;
constexpr uint32_t kIcpPer = 8;                                          // points per thread of k_icp_accumulate

struct IcpOrigin { double x, y, z; };

template <bool kF64>
__global__ __launch_bounds__(kIcpThreads) void k_icp_transform(uint32_t n, const void* __restrict__ points, const double* __restrict__ T, void* __restrict__ out) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * kIcpThreads + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    if (kF64) {
        const double* p = reinterpret_cast<const double*>(points) + (size_t)i * 3u;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const float* p = reinterpret_cast<const float*>(points) + (size_t)i * 3u;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
    const double ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    if (kF64) {
        double* o = reinterpret_cast<double*>(out) + (size_t)i * 3u;
        o[0] = ox; o[1] = oy; o[2] = oz;
    } else {
        float* o = reinterpret_cast<float*>(out) + (size_t)i * 3u;
        o[0] = (float)ox; o[1] = (float)oy; o[2] = (float)oz;
    }
}

// s: [kIcpSums][kIcpThreads] in LDS; on return acc[] of thread 0 holds the workgroup's sums
__device__ __forceinline__ void icp_fold(double* s, double acc[kIcpSums]) {
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) s[k * kIcpThreads + threadIdx.x] = acc[k];
    __syncthreads();
    for (uint32_t w = kIcpThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < kIcpSums; ++k) s[k * kIcpThreads + threadIdx.x] += s[k * kIcpThreads + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) acc[k] = s[k * kIcpThreads];
    }
}

// An inlier: 0 <= index < n_targets and dist <= max_distance (a NaN distance is none).  part: [workgroups][kIcpSums].
__global__ __launch_bounds__(kIcpThreads) void k_icp_accumulate(uint32_t n, const float* __restrict__ points, uint32_t n_targets, const float* __restrict__ targets,
                                                                        const int32_t* __restrict__ index, const double* __restrict__ dist, double max_distance,
                                                                        IcpOrigin origin, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s[kIcpSums * kIcpThreads];
    double acc[kIcpSums];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < kIcpPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kIcpThreads * kIcpPer) + k * kIcpThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        const double d = dist[i];
        const int32_t j = index[i];
        if (!(d <= max_distance) || j < 0 || (uint32_t)j >= n_targets) continue;
        const double p[3] = {(double)points[(size_t)i * 3u] - origin.x, (double)points[(size_t)i * 3u + 1u] - origin.y, (double)points[(size_t)i * 3u + 2u] - origin.z};
        const double q[3] = {(double)targets[(size_t)j * 3u] - origin.x, (double)targets[(size_t)j * 3u + 1u] - origin.y, (double)targets[(size_t)j * 3u + 2u] - origin.z};
        acc[0] += 1.0;
        acc[1] += d * d;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[2 + a] += p[a];
            acc[5 + a] += q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += p[a] * q[b];
        }
    }
    icp_fold(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) part[(size_t)blockIdx.x * kIcpSums + k] = acc[k];
    }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_accumulate_finish(uint32_t n_parts, const double* __restrict__ part, double* __restrict__ sums) {
    __shared__ double s[kIcpSums * kIcpThreads];
    double acc[kIcpSums];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) acc[k] = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kIcpThreads) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) acc[k] += part[(size_t)i * kIcpSums + k];
    }
    icp_fold(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) sums[k] = acc[k];
    }
}

// state: double [kIcpStateDoubles] (naruto_icp.h); a state that is not running is left as it is
__global__ __launch_bounds__(64) void k_icp_step(const double* __restrict__ sums, double n_source, IcpOrigin origin, double max_iteration, double relative_fitness,
                                                 double relative_rmse, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s[kIcpSums], st[kIcpStateDoubles];
    for (int k = 0; k < kIcpSums; ++k) s[k] = sums[k];
    for (int k = 0; k < kIcpStateDoubles; ++k) st[k] = state[k];
    const double o[3] = {origin.x, origin.y, origin.z};
    icp_step(s, n_source, o, max_iteration, relative_fitness, relative_rmse, st);
    for (int k = 0; k < kIcpStateDoubles; ++k) state[k] = st[k];
}

}  // namespace naruto
