// The solver of the frame-to-frame depth odometry (naruto_odom.hip; the contract is restated in naruto_amd/odometry.py): from the 29 sums
// of one point-to-plane evaluation -- the 21 upper entries of J^T J (row-major: (i, j), i <= j), the 6 of J^T r, sum r^2, the count -- to the
// twist xi = (omega, t) = -(J^T J)^-1 J^T r by a Cholesky factorisation, and the left update T <- exp(xi) T of the rigid transform.
// Host and device: naruto_debug_odom_solve runs the same code on the CPU.  The fold of the per-thread sums (odom_fold_n, odom_add_row,
// odom_fold_parts) is stated here once for naruto_odom.hip and naruto_sdfreg.hip.
#pragma once

#include "naruto_common.h"
#include "naruto_icp.h"
#include "naruto_pose.h"

namespace naruto {

constexpr int kOdomSums = 29;
constexpr int kOdomMaxLevels = 4;
constexpr int kOdomLevelWords = 8;                               // done, status, iterations, inliers, rmse, |omega|, |t|, 0
constexpr int kOdomStateDoubles = 16 + kOdomLevelWords * kOdomMaxLevels;
constexpr double kOdomPivotRatio = 1e-12;                        // a Cholesky pivot <= this x the largest diagonal entry: rank deficient
constexpr double kOdomConverged = 1e-6;                          // |omega| and |t| below this: the level is finished

// exp of the twist xi = (omega, t): R = I + A K + B K^2, translation V t with V = I + B K + C K^2, K = [omega]x,
// A = sin(th)/th, B = (1 - cos(th))/th^2 (rodrigues_coeffs), C = (1 - A)/th^2 (its series below th = 1e-2)
__host__ __device__ inline void odom_exp(const double xi[6], double E[16]) {
    const double w[3] = {xi[0], xi[1], xi[2]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, a, b;
    rodrigues_coeffs(th2, A, B, a, b);
    const double Cc = th2 < 1e-4 ? 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0 * (1.0 - th2 / 72.0)) : (1.0 - A) / th2;
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double tv = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) k2 += K[3 * i + m] * K[3 * m + j];
            E[4 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * k2;
            tv += ((i == j ? 1.0 : 0.0) + B * K[3 * i + j] + Cc * k2) * xi[3 + j];
        }
        E[4 * i + 3] = tv;
    }
    E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
}

// sums [29] -> xi [6].  Returns kIcpRunning, or kIcpDegenerate with xi = 0: count < 6, or a pivot of the Cholesky factorisation
// A = L L^T that is not above 1e-12 x the largest diagonal entry of A (a NaN lands there too).
__host__ __device__ inline int odom_solve(const double sums[kOdomSums], double xi[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = 0.0;
    if (!(sums[28] >= 6.0)) return kIcpDegenerate;
    double L[36];
    double top = 0.0;
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j, ++k) { L[6 * i + j] = sums[k]; L[6 * j + i] = sums[k]; }
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (L[7 * i] > top) top = L[7 * i];
    }
    if (!(top > 0.0)) return kIcpDegenerate;
#pragma unroll
    for (int j = 0; j < 6; ++j) {                                // in place: the lower triangle becomes L
        double d = L[7 * j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
        if (!(d > kOdomPivotRatio * top)) return kIcpDegenerate;
        const double p = sqrt(d);
        L[7 * j] = p;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = L[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = s / p;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                // L y = -b
        double s = -sums[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k];
        y[i] = s / L[7 * i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                               // L^T xi = y
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * xi[k];
        xi[i] = s / L[7 * i];
    }
    return kIcpRunning;
}

// One evaluation's bookkeeping and update at `level` (k_odom_step's body).  state: [0..15] T, then kOdomLevelWords per level.
__host__ __device__ inline void odom_step(const double sums[kOdomSums], int level, double cap, double* state) {
    double* w = state + 16 + kOdomLevelWords * level;
    if (w[0] != 0.0) return;
    const double count = sums[28];
    w[3] = count;
    w[4] = count > 0.0 ? sqrt(sums[27] / count) : 0.0;
    double xi[6];
    if (odom_solve(sums, xi) != kIcpRunning) { w[1] = (double)kIcpDegenerate; w[0] = 1.0; return; }
    double E[16], T0[16], T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T0[i] = state[i];
    odom_exp(xi, E);
    pose_mul(E, T0, T);
#pragma unroll
    for (int i = 0; i < 16; ++i) state[i] = T[i];
    w[2] += 1.0;
    w[5] = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    w[6] = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
    if (w[5] < kOdomConverged && w[6] < kOdomConverged) { w[1] = (double)kIcpConverged; w[0] = 1.0; }
    else if (w[2] >= cap) { w[1] = (double)kIcpMaxIteration; w[0] = 1.0; }
}

// ---- the summation rule of every accumulation over a pyramid level (naruto_odom.hip, naruto_sdfreg.hip): device only ----------------------
constexpr int kOdomThreads = 256;
constexpr uint32_t kOdomPer = 8;                                         // pixels per thread: thread t of workgroup b takes b*2048 + t + 256 k

// odom_fold over N sums: s is [N][kOdomThreads] in LDS
template <int N>
__device__ __forceinline__ void odom_fold_n(double* s, double acc[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k * kOdomThreads + threadIdx.x] = acc[k];
    __syncthreads();
    for (uint32_t w = kOdomThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < N; ++k) s[k * kOdomThreads + threadIdx.x] += s[k * kOdomThreads + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = s[k * kOdomThreads];
    }
}

// one row J = [q x n, n] with residual r into the sums [0..28], in k_odom_accumulate's order
__device__ __forceinline__ void odom_add_row(double* acc, const double q[3], const double nn[3], double r) {
#pragma clang fp contract(off)
    const double J[6] = {q[1] * nn[2] - q[2] * nn[1], q[2] * nn[0] - q[0] * nn[2], q[0] * nn[1] - q[1] * nn[0], nn[0], nn[1], nn[2]};
    int m = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++m) acc[m] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
    acc[27] += r * r;
    acc[28] += 1.0;
}

// the finishing workgroup of an accumulation over N sums: thread t adds the workgroups' vectors t, t + 256, ... in turn, then odom_fold_n
template <int N>
__device__ __forceinline__ void odom_fold_parts(double* s, uint32_t n_parts, const double* __restrict__ part, double acc[N]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kOdomThreads) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += part[(size_t)i * N + k];
    }
    odom_fold_n<N>(s, acc);
}

}  // namespace naruto
