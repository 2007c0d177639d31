// Depth odometry on the device: the relative motion between two consecutive depth frames by coarse-to-fine projective point-to-plane
// ICP, a motion prior for the tracker that needs no field (nothing like it is in the reference tree: PARITY UNPINNED; the contract is
// restated in naruto_amd/odometry.py and include/naruto_hip.h states the layout of the maps and state blocks).
//
//   k_odom_maps        one thread per pixel of every pyramid level: its depth from the frame itself (the 2 x 2 means nested down to level
//                      0, so no level waits for another), the vertex V = depth * direction and the normal from the two forward neighbours
//   k_odom_init        the state block: T = the given matrix, the last motion inv(est[i-2]) @ est[i-1], or the identity; level words 0
//   k_odom_accumulate  one thread per 8 current-frame pixels in turn: q = T p, projective association into the previous frame's maps,
//                      the 29 fp64 sums of the point-to-plane normal equations, folded by halves in LDS; partials to the workspace
//   k_odom_finish      one workgroup: the partials the same way -> sums
//   k_odom_step        one thread: Cholesky, xi = -A^-1 b, T <- exp(xi) T, the level's done word (naruto_odom.h)
//
// A level whose done word is set makes k_odom_accumulate, k_odom_finish and k_odom_step return at once with nothing written, so a whole
// estimate is a fixed sequence of launches and nothing is read back.  The maps are float32 with contraction off (no fused multiply-add
// is formed anywhere in this file: every product and sum is rounded, so numpy makes the same bits); the association and the sums are
// fp64 in an order that depends on the pixel count alone: no atomics, bitwise reproducible.
#pragma once

#include "naruto_common.h"
#include "naruto_odom.h"

namespace naruto {

constexpr int kOdomThreads = 256;
constexpr uint32_t kOdomPer = 8;                                         // pixels per thread of k_odom_accumulate

struct OdomLevel { uint32_t h, w, start, offset; float fx, fy, cx, cy; }; // start: first thread of k_odom_maps; offset: floats into the maps block
struct OdomGeom { OdomLevel lv[kOdomMaxLevels]; uint32_t levels, total, W; float band, jump; };
struct OdomInit { double T[16]; };

// depth of pixel (u, v) of level L from the level-0 frame: level 0 passes finite positive depths (anything else is 0 = missing); level
// L is the mean of its 2 x 2 block's valid depths within `band` of the block's smallest, summed in the order (0,0), (0,1), (1,0), (1,1)
template <int L>
__device__ inline float odom_depth(const float* __restrict__ depth, uint32_t W, uint32_t u, uint32_t v, float band) {
    if constexpr (L == 0) {
        const float d = depth[(size_t)v * W + u];
        return (d > 0.0f && d < INFINITY) ? d : 0.0f;
    } else {
        float c[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) c[k] = odom_depth<L - 1>(depth, W, 2u * u + (k & 1u), 2u * v + (k >> 1), band);
        float lo = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c[k] > 0.0f && c[k] < lo) lo = c[k];
        float sum = 0.0f, cnt = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c[k] > 0.0f && c[k] - lo <= band) { sum = sum + c[k]; cnt = cnt + 1.0f; }
        return cnt > 0.0f ? sum / cnt : 0.0f;
    }
}

__device__ inline float odom_depth_at(int level, const float* __restrict__ depth, uint32_t W, uint32_t u, uint32_t v, float band) {
    switch (level) {
        case 0: return odom_depth<0>(depth, W, u, v, band);
        case 1: return odom_depth<1>(depth, W, u, v, band);
        case 2: return odom_depth<2>(depth, W, u, v, band);
        default: return odom_depth<3>(depth, W, u, v, band);
    }
}

__device__ inline void odom_vertex(const OdomLevel& g, uint32_t u, uint32_t v, float d, float V[3]) {
#pragma clang fp contract(off)
    const float dx = ((float)u - g.cx) / g.fx, dy = -(((float)v - g.cy) / g.fy);
    V[0] = d * dx; V[1] = d * dy; V[2] = -d;
}

// maps block, per level at lv.offset: depth [h*w], vertex [h*w,3], normal [h*w,3]
__global__ __launch_bounds__(kOdomThreads) void k_odom_maps(OdomGeom g, const float* __restrict__ depth, float* __restrict__ maps) {
#pragma clang fp contract(off)
    const uint32_t gid = blockIdx.x * kOdomThreads + threadIdx.x;
    if (gid >= g.total) return;
    int level = 0;
    for (int l = 1; l < (int)g.levels; ++l)
        if (gid >= g.lv[l].start) level = l;
    const OdomLevel lv = g.lv[level];
    const uint32_t i = gid - lv.start, u = i % lv.w, v = i / lv.w, n = lv.h * lv.w;
    const float d = odom_depth_at(level, depth, g.W, u, v, g.band);
    float V[3], N[3] = {0.0f, 0.0f, 0.0f};
    odom_vertex(lv, u, v, d, V);
    if (d > 0.0f && u + 1u < lv.w && v + 1u < lv.h) {
        const float dr = odom_depth_at(level, depth, g.W, u + 1u, v, g.band), dd = odom_depth_at(level, depth, g.W, u, v + 1u, g.band);
        if (dr > 0.0f && dd > 0.0f) {
            float R[3], D[3];
            odom_vertex(lv, u + 1u, v, dr, R);
            odom_vertex(lv, u, v + 1u, dd, D);
            const float a[3] = {R[0] - V[0], R[1] - V[1], R[2] - V[2]}, b[3] = {D[0] - V[0], D[1] - V[1], D[2] - V[2]};
            const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            if (fabsf(a[2]) < g.jump && fabsf(b[2]) < g.jump && len > 0.0f) { N[0] = c[0] / len; N[1] = c[1] / len; N[2] = c[2] / len; }
        }
    }
    float* base = maps + lv.offset;
    base[i] = d;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        base[(size_t)n + 3u * i + k] = V[k];
        base[(size_t)n * 4u + 3u * i + k] = N[k];
    }
}

// mode 0: T = init.T; 1: T = inv(est[i-2]) @ est[i-1] (the last relative motion once more); 2: identity
__global__ __launch_bounds__(64) void k_odom_init(int32_t mode, OdomInit init, const float* __restrict__ est, uint32_t i, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double T[16];
    if (mode == 0) {
        for (int k = 0; k < 16; ++k) T[k] = init.T[k];
    } else if (mode == 1) {
        double A[16], B[16], Binv[16];
        pose_load(est + 16 * (size_t)(i - 1u), A);
        pose_load(est + 16 * (size_t)(i - 2u), B);
        pose_affine_inverse(B, Binv);
        pose_mul(Binv, A, T);
    } else {
        icp_identity(T);
    }
    for (int k = 0; k < 16; ++k) state[k] = T[k];
    for (int k = 16; k < kOdomStateDoubles; ++k) state[k] = 0.0;
}

// s: [kOdomSums][kOdomThreads] in LDS; on return acc[] of thread 0 holds the workgroup's sums (icp_fold's order)
__device__ __forceinline__ void odom_fold(double* s, double acc[kOdomSums]) {
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) s[k * kOdomThreads + threadIdx.x] = acc[k];
    __syncthreads();
    for (uint32_t w = kOdomThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < kOdomSums; ++k) s[k * kOdomThreads + threadIdx.x] += s[k * kOdomThreads + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) acc[k] = s[k * kOdomThreads];
    }
}

// part: [workgroups][kOdomSums]; rows (or NULL): [n][2] = (the associated previous pixel or -1, the residual or 0)
__global__ __launch_bounds__(kOdomThreads) void k_odom_accumulate(OdomLevel lv, int32_t level, double max_dist2, const float* __restrict__ prev,
                                                                  const float* __restrict__ cur, const double* __restrict__ state,
                                                                  double* __restrict__ part, double* __restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double s[kOdomSums * kOdomThreads];
    if (state[16 + kOdomLevelWords * level] != 0.0) return;              // uniform: the level is finished
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = state[k];
    const uint32_t n = lv.h * lv.w;
    const float* cv = cur + lv.offset + n;
    const float* pv = prev + lv.offset + n;
    const float* pn = prev + lv.offset + (size_t)n * 4u;
    const double fx = (double)lv.fx, fy = (double)lv.fy, cx = (double)lv.cx, cy = (double)lv.cy;
    double acc[kOdomSums];
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < kOdomPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kOdomThreads * kOdomPer) + k * kOdomThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        double index = -1.0, r = 0.0;
        const double x = (double)cv[3u * i], y = (double)cv[3u * i + 1u], z = (double)cv[3u * i + 2u];
        if (z < 0.0) {                                                   // a valid vertex lies in front of its camera
            const double q[3] = {((T[0] * x + T[1] * y) + T[2] * z) + T[3], ((T[4] * x + T[5] * y) + T[6] * z) + T[7],
                                 ((T[8] * x + T[9] * y) + T[10] * z) + T[11]};
            const double zc = -q[2];
            if (zc > 1e-6) {
                const double u = floor(((fx * q[0]) / zc + cx) + 0.5), v = floor(((-(fy * q[1])) / zc + cy) + 0.5);
                if (u >= 0.0 && u < (double)lv.w && v >= 0.0 && v < (double)lv.h) {
                    const uint32_t j = (uint32_t)v * lv.w + (uint32_t)u;
                    const double nn[3] = {(double)pn[3u * j], (double)pn[3u * j + 1u], (double)pn[3u * j + 2u]};
                    if (nn[0] != 0.0 || nn[1] != 0.0 || nn[2] != 0.0) {
                        const double d[3] = {q[0] - (double)pv[3u * j], q[1] - (double)pv[3u * j + 1u], q[2] - (double)pv[3u * j + 2u]};
                        if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= max_dist2) {
                            index = (double)j;
                            r = (nn[0] * d[0] + nn[1] * d[1]) + nn[2] * d[2];
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
                    }
                }
            }
        }
        if (rows != nullptr) { rows[2u * (size_t)i] = index; rows[2u * (size_t)i + 1u] = r; }
    }
    odom_fold(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) part[(size_t)blockIdx.x * kOdomSums + k] = acc[k];
    }
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_finish(int32_t level, const double* __restrict__ state, uint32_t n_parts, const double* __restrict__ part,
                                                              double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double s[kOdomSums * kOdomThreads];
    if (state[16 + kOdomLevelWords * level] != 0.0) return;
    double acc[kOdomSums];
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) acc[k] = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kOdomThreads) {
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) acc[k] += part[(size_t)i * kOdomSums + k];
    }
    odom_fold(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) sums[k] = acc[k];
    }
}

__global__ __launch_bounds__(64) void k_odom_step(int32_t level, double cap, const double* __restrict__ sums, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (state[16 + kOdomLevelWords * level] != 0.0) return;
    double s[kOdomSums];
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) s[k] = sums[k];
    odom_step(s, level, cap, state);                                     // on the state block itself: T and the level's words
}

// est[i] = est[i-1] @ T (fp64 from the float32 matrix, rounded once); pose6_out = the log of est[i] as stored
__global__ __launch_bounds__(64) void k_pose_predict_relative(float* est, uint32_t i, const double* __restrict__ state_T, float* __restrict__ pose6_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double A[16], T[16], N[16];
    pose_load(est + 16 * (size_t)(i - 1u), A);
    for (int k = 0; k < 16; ++k) T[k] = state_T[k];
    pose_mul(A, T, N);
    float next[16];
    pose_store(next, N);
    for (int k = 0; k < 16; ++k) est[16 * (size_t)i + k] = next[k];
    float q[6];
    pose_log(next, q);
#pragma unroll
    for (int k = 0; k < 6; ++k) pose6_out[k] = q[k];
}

}  // namespace naruto
