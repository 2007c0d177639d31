// Frame-to-model alignment on the device: a depth frame registered to the field's own SDF by Gauss-Newton on the signed distance the
// field reports at the back-projected points (nothing like it is in the reference tree: PARITY UNPINNED; the contract is restated in
// naruto_amd/registration.py and include/naruto_hip.h, tests/field_registration_spec.py is the numpy twin).  T is the camera-to-field
// pose itself.  One iteration at a level is five launches: k_sdfreg_points, naruto_query_fwd, naruto_query_bwd_points,
// k_sdfreg_accumulate + k_sdfreg_finish, k_odom_step.
//
//   k_sdfreg_points      one thread per 8 pixels of the level's vertex map in turn: q = T p (fp64, rounded once to float32), the
//                        normalised point x = (q - bbox_min) / (bbox_max - bbox_min) in float32, the valid byte
//   k_sdfreg_accumulate  the same pixel order: r = trunc sdf, g = trunc d_x / extent, the row J = [q x g, g]; the 29 sums of
//                        k_odom_accumulate and the count of valid points, folded by odom_fold_n (naruto_odom.h); partials to the workspace
//   k_sdfreg_finish      one workgroup: the partials the same way (odom_fold_parts) -> sums
//   k_sdfreg_init        one thread: T = est[i], the level words 0, the start kept behind the state block
//   k_sdfreg_verdict     one thread: the five checks, the record; on FAIL T becomes the start
//   k_sdfreg_commit      one thread: est[i] = T rounded once, pose6_out = its log
//
// A gated launch of a level whose done word is set returns at once with nothing written.  No fused multiply-add is formed in the
// arithmetic that the twin restates; no atomics; the sums depend on the pixel count alone: bitwise reproducible.
#pragma once

#include "naruto_common.h"
#include "naruto_odom.h"

namespace naruto {

constexpr int kSdfRegSums = 30;                                          // [0..28] as kOdomSums, [29] the valid points
constexpr int kSdfRegStateDoubles = kOdomStateDoubles + 16;              // the odometry's state block, then the start's T
constexpr int kSdfRegRecord = 8;

struct SdfRegBox { float lo[3], hi[3]; };
struct SdfRegGate { double max_trans, min_trace, min_overlap; };

// the level's done word when the launch is gated
__device__ __forceinline__ bool sdfreg_finished(const double* __restrict__ state, int32_t level, int32_t gated) {
    return gated != 0 && state[16 + kOdomLevelWords * level] != 0.0;
}

// verts: the level's vertex map [n,3]; x, q: [n,3]; valid: [n]
__global__ __launch_bounds__(kOdomThreads) void k_sdfreg_points(uint32_t n, int32_t level, int32_t gated, SdfRegBox box, const float* __restrict__ verts,
                                                                const double* __restrict__ state, float* __restrict__ x, float* __restrict__ q,
                                                                uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    if (sdfreg_finished(state, level, gated)) return;                    // uniform: the level is finished
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = state[k];
    float ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ext[a] = box.hi[a] - box.lo[a];
#pragma unroll 1
    for (uint32_t k = 0; k < kOdomPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kOdomThreads * kOdomPer) + k * kOdomThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        const double px = (double)verts[3u * i], py = (double)verts[3u * i + 1u], pz = (double)verts[3u * i + 2u];
        bool ok = pz < 0.0;
        float qf[3], xf[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            qf[a] = (float)(((T[4 * a] * px + T[4 * a + 1] * py) + T[4 * a + 2] * pz) + T[4 * a + 3]);
            xf[a] = (qf[a] - box.lo[a]) / ext[a];
            ok = ok && xf[a] >= 0.0f && xf[a] <= 1.0f;                   // a NaN fails both; +-inf fails one
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            q[3u * (size_t)i + a] = qf[a];
            x[3u * (size_t)i + a] = ok ? xf[a] : 0.5f;
        }
        valid[i] = ok ? (uint8_t)1 : (uint8_t)0;
    }
}

// sdf_uncert: [n,2] (naruto_query_fwd's; the sdf is channel 0); d_x, q: [n,3]; part: [workgroups][kSdfRegSums]; rows (or NULL): [n][2]
__global__ __launch_bounds__(kOdomThreads) void k_sdfreg_accumulate(uint32_t n, int32_t level, int32_t gated, double trunc, double gate, SdfRegBox box,
                                                                    const float* __restrict__ sdf_uncert, const float* __restrict__ d_x,
                                                                    const float* __restrict__ q, const uint8_t* __restrict__ valid,
                                                                    const double* __restrict__ state, double* __restrict__ part, double* __restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double s[kSdfRegSums * kOdomThreads];
    if (sdfreg_finished(state, level, gated)) return;                    // uniform
    double ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ext[a] = (double)(box.hi[a] - box.lo[a]);
    double acc[kSdfRegSums];
#pragma unroll
    for (int k = 0; k < kSdfRegSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < kOdomPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kOdomThreads * kOdomPer) + k * kOdomThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        double flag = 0.0, r = 0.0;
        if (valid[i] != 0) {
            acc[29] += 1.0;
            const double sdf = (double)sdf_uncert[2u * (size_t)i];
            const double g[3] = {(trunc * (double)d_x[3u * (size_t)i]) / ext[0], (trunc * (double)d_x[3u * (size_t)i + 1u]) / ext[1],
                                 (trunc * (double)d_x[3u * (size_t)i + 2u]) / ext[2]};
            const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            // a NaN fails its comparison; an infinite g makes gg infinite
            if (fabs(sdf) < gate && gg > 0.0 && gg < (double)INFINITY) {
                const double qq[3] = {(double)q[3u * (size_t)i], (double)q[3u * (size_t)i + 1u], (double)q[3u * (size_t)i + 2u]};
                flag = 1.0;
                r = trunc * sdf;
                odom_add_row(acc, qq, g, r);
            }
        }
        if (rows != nullptr) { rows[2u * (size_t)i] = flag; rows[2u * (size_t)i + 1u] = r; }
    }
    odom_fold_n<kSdfRegSums>(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSdfRegSums; ++k) part[(size_t)blockIdx.x * kSdfRegSums + k] = acc[k];
    }
}

__global__ __launch_bounds__(kOdomThreads) void k_sdfreg_finish(int32_t level, int32_t gated, const double* __restrict__ state, uint32_t n_parts,
                                                                const double* __restrict__ part, double* __restrict__ sums) {
    __shared__ double s[kSdfRegSums * kOdomThreads];
    if (sdfreg_finished(state, level, gated)) return;
    double acc[kSdfRegSums];
    odom_fold_parts<kSdfRegSums>(s, n_parts, part, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSdfRegSums; ++k) sums[k] = acc[k];
    }
}

__global__ __launch_bounds__(64) void k_sdfreg_init(const float* __restrict__ est, uint32_t i, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double T[16];
    pose_load(est + 16 * (size_t)i, T);
    for (int k = 0; k < 16; ++k) state[k] = T[k];
    for (int k = 16; k < kOdomStateDoubles; ++k) state[k] = 0.0;
    for (int k = 0; k < 16; ++k) state[kOdomStateDoubles + k] = T[k];
}

__device__ inline double sdfreg_finite_or(double v, double other) { return fabs(v) < (double)INFINITY ? v : other; }

// start, fin: the 30 sums of the start's and the final T's evaluation at `level`, the finest level used
__global__ __launch_bounds__(64) void k_sdfreg_verdict(SdfRegGate gate, int32_t level, const double* __restrict__ start, const double* __restrict__ fin,
                                                       double* __restrict__ state, double* __restrict__ record) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double* T0 = state + kOdomStateDoubles;
    const double status = state[16 + kOdomLevelWords * level + 1];
    const double n_valid = fin[29], n_rows = fin[28];
    const double mse0 = start[27] / start[28], mse1 = fin[27] / n_rows;  // 0 / 0 = NaN fails the comparison below
    const double d[3] = {state[3] - T0[3], state[7] - T0[7], state[11] - T0[11]};
    const double t2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    double trace = 0.0;                                                  // trace(R_start^T R): the entries' products in row-major order
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) trace = trace + T0[4 * a + b] * state[4 * a + b];
    const bool pass = status != (double)kIcpDegenerate && n_rows >= gate.min_overlap * n_valid && n_rows > 0.0 && mse1 <= mse0 &&
                      t2 <= gate.max_trans * gate.max_trans && trace >= gate.min_trace;
    record[0] = pass ? 1.0 : 0.0;
    record[1] = n_valid;
    record[2] = n_rows;
    record[3] = sdfreg_finite_or(sqrt(mse0), -1.0);
    record[4] = sdfreg_finite_or(sqrt(mse1), -1.0);
    record[5] = sdfreg_finite_or(sqrt(t2), -1.0);
    record[6] = sdfreg_finite_or(trace, -1.0);
    record[7] = status;
    if (!pass)
        for (int k = 0; k < 16; ++k) state[k] = T0[k];
}

// est[i] = T rounded once to float32; pose6_out = the log of est[i] as stored, as k_pose_predict_relative ends
__global__ __launch_bounds__(64) void k_sdfreg_commit(float* est, uint32_t i, const double* __restrict__ state, float* __restrict__ pose6_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = state[k];
    float next[16];
    pose_store(next, T);
    for (int k = 0; k < 16; ++k) est[16 * (size_t)i + k] = next[k];
    float p[6];
    pose_log(next, p);
#pragma unroll
    for (int k = 0; k < 6; ++k) pose6_out[k] = p[k];
}

}  // namespace naruto
