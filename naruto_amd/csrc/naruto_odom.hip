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
// k_odom_accumulate, k_odom_rgbd_accumulate, k_odom_score and k_odom_score_finish are one-line wrappers around __device__ bodies
// (odom_accumulate_body ...), which naruto_odom_anchor.hip wraps a second time with the previous frame taken from a ring of references.
//
// A level whose done word is set makes k_odom_accumulate, k_odom_finish and k_odom_step return at once with nothing written, so a whole
// estimate is a fixed sequence of launches and nothing is read back.  The maps are float32 with contraction off (no fused multiply-add
// is formed anywhere in this file: every product and sum is rounded, so numpy makes the same bits); the association and the sums are
// fp64 in an order that depends on the pixel count alone: no atomics, bitwise reproducible.
#pragma once

#include "naruto_common.h"
#include "naruto_odom.h"

namespace naruto {


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

// the pyramid level thread gid of a maps launch works on
__device__ inline int odom_level_of(const OdomGeom& g, uint32_t gid) {
    int level = 0;
    for (int l = 1; l < (int)g.levels; ++l)
        if (gid >= g.lv[l].start) level = l;
    return level;
}

// pixel i of `level` into the depth part of a maps block, per level at lv.offset: depth [h*w], vertex [h*w,3], normal [h*w,3]
__device__ inline void odom_maps_pixel(const OdomGeom& g, int level, const OdomLevel& lv, uint32_t i, const float* __restrict__ depth, float* __restrict__ maps) {
#pragma clang fp contract(off)
    const uint32_t u = i % lv.w, v = i / lv.w, n = lv.h * lv.w;
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

__global__ __launch_bounds__(kOdomThreads) void k_odom_maps(OdomGeom g, const float* __restrict__ depth, float* __restrict__ maps) {
    const uint32_t gid = blockIdx.x * kOdomThreads + threadIdx.x;
    if (gid >= g.total) return;
    const int level = odom_level_of(g, gid);
    const OdomLevel lv = g.lv[level];
    odom_maps_pixel(g, level, lv, gid - lv.start, depth, maps);
}

// the last relative motion inv(est[i-2]) @ est[i-1], i > 1: the constant-speed guess of k_odom_init and k_odom_candidates
__device__ inline void odom_last_motion(const float* __restrict__ est, uint32_t i, double T[16]) {
    double A[16], B[16], Binv[16];
    pose_load(est + 16 * (size_t)(i - 1u), A);
    pose_load(est + 16 * (size_t)(i - 2u), B);
    pose_affine_inverse(B, Binv);
    pose_mul(Binv, A, T);
}

// mode 0: T = init.T; 1: T = inv(est[i-2]) @ est[i-1] (the last relative motion once more); 2: identity
__global__ __launch_bounds__(64) void k_odom_init(int32_t mode, OdomInit init, const float* __restrict__ est, uint32_t i, double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double T[16];
    if (mode == 0) {
        for (int k = 0; k < 16; ++k) T[k] = init.T[k];
    } else if (mode == 1) {
        odom_last_motion(est, i, T);
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

// The association of one current-frame vertex (x, y, z), z < 0, under the transform T (its first 12 doubles): q = T p, the projection
// (uc, vc), the nearest previous pixel j, `near` (|q - V_prev[j]|^2 <= max_dist2) and the geometric row's acceptance and residual -- the
// one statement of the rule k_odom_accumulate, k_odom_rgbd_accumulate and k_odom_score share, fp64 without contraction.
struct OdomHit { double q[3], zc, uc, vc, nn[3], r; uint32_t j; bool inside, near, geo; };

__device__ __forceinline__ void odom_associate(const double* T, const OdomLevel& lv, const float* __restrict__ pv, const float* __restrict__ pn,
                                               double x, double y, double z, double max_dist2, OdomHit& h) {
#pragma clang fp contract(off)
    h.inside = false; h.near = false; h.geo = false; h.r = 0.0; h.j = 0u;
    h.q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    h.q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    h.q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    h.zc = -h.q[2];
    if (!(h.zc > 1e-6)) return;
    h.uc = ((double)lv.fx * h.q[0]) / h.zc + (double)lv.cx;
    h.vc = (-((double)lv.fy * h.q[1])) / h.zc + (double)lv.cy;
    const double u = floor(h.uc + 0.5), v = floor(h.vc + 0.5);
    if (!(u >= 0.0 && u < (double)lv.w && v >= 0.0 && v < (double)lv.h)) return;
    h.inside = true;
    const uint32_t j = (uint32_t)v * lv.w + (uint32_t)u;
    h.j = j;
    const double d[3] = {h.q[0] - (double)pv[3u * j], h.q[1] - (double)pv[3u * j + 1u], h.q[2] - (double)pv[3u * j + 2u]};
    h.near = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= max_dist2;
    h.nn[0] = (double)pn[3u * j]; h.nn[1] = (double)pn[3u * j + 1u]; h.nn[2] = (double)pn[3u * j + 2u];
    if ((h.nn[0] != 0.0 || h.nn[1] != 0.0 || h.nn[2] != 0.0) && h.near) {
        h.geo = true;
        h.r = (h.nn[0] * d[0] + h.nn[1] * d[1]) + h.nn[2] * d[2];
    }
}

// part: [workgroups][kOdomSums]; rows (or NULL): [n][2] = (the associated previous pixel or -1, the residual or 0)
__device__ __forceinline__ void odom_accumulate_body(const OdomLevel& lv, int32_t level, double max_dist2, const float* __restrict__ prev,
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
            OdomHit h;
            odom_associate(T, lv, pv, pn, x, y, z, max_dist2, h);
            if (h.geo) {
                index = (double)h.j;
                r = h.r;
                const double* q = h.q;
                const double* nn = h.nn;
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
        if (rows != nullptr) { rows[2u * (size_t)i] = index; rows[2u * (size_t)i + 1u] = r; }
    }
    odom_fold(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) part[(size_t)blockIdx.x * kOdomSums + k] = acc[k];
    }
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_accumulate(OdomLevel lv, int32_t level, double max_dist2, const float* __restrict__ prev,
                                                                  const float* __restrict__ cur, const double* __restrict__ state,
                                                                  double* __restrict__ part, double* __restrict__ rows) {
    odom_accumulate_body(lv, level, max_dist2, prev, cur, state, part, rows);
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

// ---- RGB-D odometry: the depth odometry plus a photometric row per pixel (contract: naruto_amd/odometry.py, include/naruto_hip.h) ----------
//
//   k_odom_rgbd_maps        one thread per pixel of every level: the depth part exactly as k_odom_maps (odom_maps_pixel), then the intensity
//                           I (the 2 x 2 means nested down to level 0) and its central differences gx, gy into the intensity block
//   k_odom_rgbd_accumulate  k_odom_accumulate over 32 sums: per pixel the geometric row first, then the photometric row
//   k_odom_rgbd_finish      k_odom_finish over 32 sums
constexpr int kOdomRgbdSums = 32;                                        // [0..28] as kOdomSums over both kinds of rows; geometric rows, photometric rows, sum r_I^2

// intensity of pixel (u, v) of level L from the level-0 colour frame [H,W,3]: level 0 is (0.299 r + 0.587 g) + 0.114 b, level L the mean
// (((a + b) + c) + d) * 0.25 of its 2 x 2 block in the order (0,0), (0,1), (1,0), (1,1)
template <int L>
__device__ inline float odom_intensity(const float* __restrict__ color, uint32_t W, uint32_t u, uint32_t v) {
#pragma clang fp contract(off)
    if constexpr (L == 0) {
        const float* c = color + 3u * ((size_t)v * W + u);
        return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2];
    } else {
        const float a = odom_intensity<L - 1>(color, W, 2u * u, 2u * v), b = odom_intensity<L - 1>(color, W, 2u * u + 1u, 2u * v);
        const float c = odom_intensity<L - 1>(color, W, 2u * u, 2u * v + 1u), d = odom_intensity<L - 1>(color, W, 2u * u + 1u, 2u * v + 1u);
        return (((a + b) + c) + d) * 0.25f;
    }
}

__device__ inline float odom_intensity_at(int level, const float* __restrict__ color, uint32_t W, uint32_t u, uint32_t v) {
    switch (level) {
        case 0: return odom_intensity<0>(color, W, u, v);
        case 1: return odom_intensity<1>(color, W, u, v);
        case 2: return odom_intensity<2>(color, W, u, v);
        default: return odom_intensity<3>(color, W, u, v);
    }
}

// RGB-D maps block: the depth maps block (7 x g.total floats), then per level at 7 x g.total + 3 x lv.start: I [h*w], gx [h*w], gy [h*w]
__global__ __launch_bounds__(kOdomThreads) void k_odom_rgbd_maps(OdomGeom g, const float* __restrict__ depth, const float* __restrict__ color,
                                                                 float* __restrict__ maps) {
#pragma clang fp contract(off)
    const uint32_t gid = blockIdx.x * kOdomThreads + threadIdx.x;
    if (gid >= g.total) return;
    const int level = odom_level_of(g, gid);
    const OdomLevel lv = g.lv[level];
    const uint32_t i = gid - lv.start, u = i % lv.w, v = i / lv.w, n = lv.h * lv.w;
    odom_maps_pixel(g, level, lv, i, depth, maps);
    float gx = 0.0f, gy = 0.0f;
    if (u >= 1u && u + 2u <= lv.w) gx = (odom_intensity_at(level, color, g.W, u + 1u, v) - odom_intensity_at(level, color, g.W, u - 1u, v)) * 0.5f;
    if (v >= 1u && v + 2u <= lv.h) gy = (odom_intensity_at(level, color, g.W, u, v + 1u) - odom_intensity_at(level, color, g.W, u, v - 1u)) * 0.5f;
    float* base = maps + (size_t)g.total * 7u + (size_t)lv.start * 3u;
    base[i] = odom_intensity_at(level, color, g.W, u, v);
    base[(size_t)n + i] = gx;
    base[(size_t)n * 2u + i] = gy;
}

// m at (u0 + a, v0 + b), a, b in [0, 1): top = s00 + a (s10 - s00), bot = s01 + a (s11 - s01), top + b (bot - top); s10 is (u0 + 1, v0)
__device__ __forceinline__ double odom_bilinear(const float* __restrict__ m, uint32_t j00, uint32_t w, double a, double b) {
#pragma clang fp contract(off)
    const double s00 = (double)m[j00], s10 = (double)m[j00 + 1u], s01 = (double)m[j00 + w], s11 = (double)m[j00 + w + 1u];
    const double top = s00 + a * (s10 - s00), bot = s01 + a * (s11 - s01);
    return top + b * (bot - top);
}

// The photometric row's acceptance for an associated vertex h (pi: the previous frame's I | gx | gy of the level, Icur: the current
// pixel's intensity): the four neighbours of (uc, vc) are interior pixels, the nearest pixel has a vertex close to q, |r_I| <= max_diff and
// the sampled gradients are finite.  res = r_I, gx, gy = the sampled gradients.
__device__ __forceinline__ bool odom_photo_accept(const OdomHit& h, const OdomLevel& lv, const float* __restrict__ pv, const float* __restrict__ pi,
                                                  double Icur, double max_diff, double& res, double& gx, double& gy) {
#pragma clang fp contract(off)
    if (!h.inside) return false;
    const uint32_t n = lv.h * lv.w;
    const double u0 = floor(h.uc), v0 = floor(h.vc);
    if (!(u0 >= 1.0 && u0 + 1.0 <= (double)lv.w - 2.0 && v0 >= 1.0 && v0 + 1.0 <= (double)lv.h - 2.0 && (double)pv[3u * h.j + 2u] < 0.0 && h.near))
        return false;
    const uint32_t j00 = (uint32_t)v0 * lv.w + (uint32_t)u0;
    const double a = h.uc - u0, b = h.vc - v0;
    res = odom_bilinear(pi, j00, lv.w, a, b) - Icur;
    gx = odom_bilinear(pi + n, j00, lv.w, a, b);
    gy = odom_bilinear(pi + 2u * (size_t)n, j00, lv.w, a, b);
    return fabs(res) <= max_diff && fabs(gx) < (double)INFINITY && fabs(gy) < (double)INFINITY;
}

// part: [workgroups][kOdomRgbdSums]; rows (or NULL): [n][4] = (geometric j or -1, r, photometric j or -1, r_I); ioff: floats to the level's I
__device__ __forceinline__ void odom_rgbd_accumulate_body(const OdomLevel& lv, uint32_t ioff, int32_t level, double max_dist2, double weight,
                                                          double max_diff, const float* __restrict__ prev, const float* __restrict__ cur,
                                                          const double* __restrict__ state, double* __restrict__ part, double* __restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double s[kOdomRgbdSums * kOdomThreads];
    if (state[16 + kOdomLevelWords * level] != 0.0) return;              // uniform: the level is finished
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = state[k];
    const uint32_t n = lv.h * lv.w;
    const float* cv = cur + lv.offset + n;
    const float* pv = prev + lv.offset + n;
    const float* pn = prev + lv.offset + (size_t)n * 4u;
    const float* ci = cur + ioff;
    const float* pi = prev + ioff;
    const double fx = (double)lv.fx, fy = (double)lv.fy;
    double acc[kOdomRgbdSums];
#pragma unroll
    for (int k = 0; k < kOdomRgbdSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < kOdomPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kOdomThreads * kOdomPer) + k * kOdomThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        double index = -1.0, r = 0.0, pindex = -1.0, rI = 0.0;
        const double x = (double)cv[3u * i], y = (double)cv[3u * i + 1u], z = (double)cv[3u * i + 2u];
        if (z < 0.0) {                                                   // a valid vertex lies in front of its camera
            OdomHit h;
            odom_associate(T, lv, pv, pn, x, y, z, max_dist2, h);
            if (h.geo) {
                index = (double)h.j;
                r = h.r;
                odom_add_row(acc, h.q, h.nn, r);
                acc[29] += 1.0;
            }
            double res, gx, gy;
            if (weight > 0.0 && odom_photo_accept(h, lv, pv, pi, (double)ci[i], max_diff, res, gx, gy)) {
                const double* q = h.q;
                const double zc = h.zc;
                const double ga = gx * fx, gb = gy * fy;
                const double g[3] = {weight * (ga / zc), weight * (-(gb / zc)), weight * ((ga * q[0] - gb * q[1]) / (zc * zc))};
                pindex = (double)h.j;
                rI = res;
                odom_add_row(acc, q, g, weight * res);
                acc[30] += 1.0;
                acc[31] += res * res;
            }
        }
        if (rows != nullptr) {
            rows[4u * (size_t)i] = index; rows[4u * (size_t)i + 1u] = r;
            rows[4u * (size_t)i + 2u] = pindex; rows[4u * (size_t)i + 3u] = rI;
        }
    }
    odom_fold_n<kOdomRgbdSums>(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomRgbdSums; ++k) part[(size_t)blockIdx.x * kOdomRgbdSums + k] = acc[k];
    }
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_rgbd_accumulate(OdomLevel lv, uint32_t ioff, int32_t level, double max_dist2, double weight,
                                                                       double max_diff, const float* __restrict__ prev, const float* __restrict__ cur,
                                                                       const double* __restrict__ state, double* __restrict__ part, double* __restrict__ rows) {
    odom_rgbd_accumulate_body(lv, ioff, level, max_dist2, weight, max_diff, prev, cur, state, part, rows);
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_rgbd_finish(int32_t level, const double* __restrict__ state, uint32_t n_parts,
                                                                   const double* __restrict__ part, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double s[kOdomRgbdSums * kOdomThreads];
    if (state[16 + kOdomLevelWords * level] != 0.0) return;
    double acc[kOdomRgbdSums];
#pragma unroll
    for (int k = 0; k < kOdomRgbdSums; ++k) acc[k] = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kOdomThreads) {
#pragma unroll
        for (int k = 0; k < kOdomRgbdSums; ++k) acc[k] += part[(size_t)i * kOdomRgbdSums + k];
    }
    odom_fold_n<kOdomRgbdSums>(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kOdomRgbdSums; ++k) sums[k] = acc[k];
    }
}

// ---- scored starts and a verdict (contract: naruto_amd/odometry.py, include/naruto_hip.h; numpy twin: tests/odometry_gate_spec.py) ---------
//
//   k_odom_score         k_odom_accumulate's pixel order over K candidate transforms at once: the vertex is read once, every candidate
//                        makes odom_associate's association (and, PHOTO, odom_photo_accept's); 1 + 4 K fp64 sums, no state, no done word
//   k_odom_score_finish  k_odom_finish over 1 + 4 K sums
//   k_odom_candidates    one thread: cands[0] = identity, cands[1] = the last motion (odom_last_motion) or the identity
//   k_odom_choose        one thread: the truncated cost per candidate, the lowest one's T into the state block, the record's head
//   k_odom_verdict       one thread: the five checks at level 0, the record's tail; on FAIL the state's T becomes the chosen candidate
constexpr int kOdomMaxCands = 4;
constexpr int kOdomGateWords = 16;

// cands: [K][16] row-major transforms; part: [workgroups][1 + 4 K]: [0] pixels with p.z < 0, then per candidate the geometric rows, the sum
// of min(r^2, trunc2), the photometric rows, the sum of r_I^2.  A candidate with a non-finite entry fails odom_associate's comparisons.
template <int K, bool PHOTO>
__device__ __forceinline__ void odom_score_body(const OdomLevel& lv, uint32_t ioff, double max_dist2, double trunc2, double max_diff,
                                                const float* __restrict__ prev, const float* __restrict__ cur,
                                                const double* __restrict__ cands, double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int N = 1 + 4 * K;
    __shared__ double s[N * kOdomThreads];
    const uint32_t n = lv.h * lv.w;
    const float* cv = cur + lv.offset + n;
    const float* pv = prev + lv.offset + n;
    const float* pn = prev + lv.offset + (size_t)n * 4u;
    const float* ci = cur + ioff;
    const float* pi = prev + ioff;
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < kOdomPer; ++k) {
        const uint64_t i64 = (uint64_t)blockIdx.x * (kOdomThreads * kOdomPer) + k * kOdomThreads + threadIdx.x;
        if (i64 >= n) continue;
        const uint32_t i = (uint32_t)i64;
        const double x = (double)cv[3u * i], y = (double)cv[3u * i + 1u], z = (double)cv[3u * i + 2u];
        if (!(z < 0.0)) continue;
        acc[0] += 1.0;
        double Icur = 0.0;
        if constexpr (PHOTO) Icur = (double)ci[i];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            OdomHit h;
            odom_associate(cands + 16 * c, lv, pv, pn, x, y, z, max_dist2, h);
            if (h.geo) {
                const double rr = h.r * h.r;
                acc[1 + 4 * c] += 1.0;
                acc[2 + 4 * c] += rr < trunc2 ? rr : trunc2;
            }
            if constexpr (PHOTO) {
                double res, gx, gy;
                if (odom_photo_accept(h, lv, pv, pi, Icur, max_diff, res, gx, gy)) {
                    acc[3 + 4 * c] += 1.0;
                    acc[4 + 4 * c] += res * res;
                }
            }
        }
    }
    odom_fold_n<N>(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[(size_t)blockIdx.x * N + k] = acc[k];
    }
}

template <int K, bool PHOTO>
__global__ __launch_bounds__(kOdomThreads) void k_odom_score(OdomLevel lv, uint32_t ioff, double max_dist2, double trunc2, double max_diff,
                                                             const float* __restrict__ prev, const float* __restrict__ cur,
                                                             const double* __restrict__ cands, double* __restrict__ part) {
    odom_score_body<K, PHOTO>(lv, ioff, max_dist2, trunc2, max_diff, prev, cur, cands, part);
}

template <int K>
__device__ __forceinline__ void odom_score_finish_body(uint32_t n_parts, const double* __restrict__ part, double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int N = 1 + 4 * K;
    __shared__ double s[N * kOdomThreads];
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kOdomThreads) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += part[(size_t)i * N + k];
    }
    odom_fold_n<N>(s, acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sums[k] = acc[k];
    }
}

template <int K>
__global__ __launch_bounds__(kOdomThreads) void k_odom_score_finish(uint32_t n_parts, const double* __restrict__ part, double* __restrict__ sums) {
    odom_score_finish_body<K>(n_parts, part, sums);
}

__global__ __launch_bounds__(64) void k_odom_candidates(const float* __restrict__ est, uint32_t i, double* __restrict__ cands) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double T[16];
    icp_identity(T);
    for (int k = 0; k < 16; ++k) cands[k] = T[k];
    if (i > 1u) odom_last_motion(est, i, T);
    for (int k = 0; k < 16; ++k) cands[16 + k] = T[k];
}

// (s + (n_valid - n) tau^2) / (n_valid tau^2): every valid pixel without a row costs tau^2; 1 when no pixel is valid; +inf when not finite
__device__ inline double odom_cost_term(double n_valid, double n, double s, double tau) {
#pragma clang fp contract(off)
    if (n_valid == 0.0) return 1.0;
    const double t2 = tau * tau;
    const double c = (s + (n_valid - n) * t2) / (n_valid * t2);
    return fabs(c) < (double)INFINITY ? c : (double)INFINITY;
}

__device__ inline double odom_finite_or(double v, double other) { return fabs(v) < (double)INFINITY ? v : other; }

__global__ __launch_bounds__(64) void k_odom_choose(uint32_t K, int32_t photo_on, double trunc, double photo_max_diff, const double* __restrict__ sums,
                                                    const double* __restrict__ cands, double* __restrict__ state, double* __restrict__ record) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double n_valid = sums[0];
    double best = (double)INFINITY;
    uint32_t chosen = 0u;
    for (int k = 0; k < kOdomGateWords; ++k) record[k] = 0.0;
    for (uint32_t k = 0; k < (uint32_t)kOdomMaxCands; ++k) {
        double c = -1.0;
        if (k < K) {
            c = odom_cost_term(n_valid, sums[1u + 4u * k], sums[2u + 4u * k], trunc);
            if (photo_on) c = c + odom_cost_term(n_valid, sums[3u + 4u * k], sums[4u + 4u * k], photo_max_diff);
            if (!(fabs(c) < (double)INFINITY)) c = (double)INFINITY;
            if (c < best) { best = c; chosen = k; }
        }
        record[2u + k] = c;
    }
    record[1] = (double)chosen;
    for (int k = 0; k < 16; ++k) state[k] = cands[16u * chosen + k];
    for (int k = 16; k < kOdomStateDoubles; ++k) state[k] = 0.0;
}

struct OdomGate { double max_trans, min_trace, min_overlap, max_rmse; };

// sums: a K = 1 score of the state's T at level 0 with trunc = max_dist.  A NaN fails every comparison it enters, so it is a FAIL.
__global__ __launch_bounds__(64) void k_odom_verdict(OdomGate gate, const double* __restrict__ sums, const double* __restrict__ cands,
                                                     double* __restrict__ state, double* __restrict__ record) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double n_valid = sums[0], n_geo = sums[1], s_geo = sums[2], n_photo = sums[3], s_photo = sums[4];
    const double status = state[16 + 1];
    const double t2 = (state[3] * state[3] + state[7] * state[7]) + state[11] * state[11];
    const double trace = (state[0] + state[5]) + state[10];
    const bool pass = status >= 0.0 && status != (double)kIcpDegenerate && n_geo >= gate.min_overlap * n_valid && n_geo > 0.0 &&
                      s_geo <= (gate.max_rmse * gate.max_rmse) * n_geo && t2 <= gate.max_trans * gate.max_trans && trace >= gate.min_trace;
    record[0] = pass ? 1.0 : 0.0;
    record[6] = n_valid;
    record[7] = n_geo;
    record[8] = n_geo > 0.0 ? odom_finite_or(sqrt(s_geo / n_geo), -1.0) : 0.0;
    record[9] = odom_finite_or(sqrt(t2), -1.0);
    record[10] = odom_finite_or(trace, -1.0);
    record[11] = status;
    record[12] = n_photo;
    record[13] = n_photo > 0.0 ? odom_finite_or(sqrt(s_photo / n_photo), -1.0) : 0.0;
    record[14] = 0.0;
    record[15] = 0.0;
    if (!pass) {
        const double c = record[1];                                      // k_odom_choose's; anything else reads candidate 0
        const uint32_t chosen = (c >= 0.0 && c < (double)kOdomMaxCands) ? (uint32_t)c : 0u;
        for (int k = 0; k < 16; ++k) state[k] = cands[16u * chosen + k];
    }
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
