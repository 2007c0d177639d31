// Gradient of the field query with respect to its POINTS (naruto_query_bwd_points): what autograd of the reference's forward gives
// for x / rays_o / rays_d -- pose refinement (global_BA's pose_optim, reference coslam.py:264-281, 330-347, 378-407) and Co-SLAM's
// tracking_render differentiate the rendering through the rays.  The parameter gradients stay with k_query_bwd; nothing here
// touches them, so they come out the same whether or not point gradients are asked for.
//
// One lane owns one point, from d_raw [5] (+ d_geo [15]) to d(point) [3]:
//   1. the 16 hash levels' corners (the forward's index arithmetic, hash_corner_index): each level's features AND its 2x3 spatial
//      Jacobian  d feat / d x_d = scale_l * sum_c (d w_c / d w_d) v_c  (tcnn linear interpolation; the corner indices are piecewise
//      constant in x and contribute nothing);
//   2. OneBlob (16 bins, quartic kernel) and its derivative  d cdf3(t) / dt = 15 (1 - u^2)^2, u = 16 (t - r), |u| <= 1 (0 outside:
//      torch.clamp passes no gradient where it clamps); the uncertainty sample's gradient (grid_sample, align_corners=False, zero
//      padding, d ix / d x = W, the x <-> z quirk) -- it reaches raw[...,4] only;
//   3. the two MLPs, forward for their ReLU masks (ReLU'(0) = 0) and backward to their INPUTS (no weight gradients), in exact fp32
//      on the fp32 master weights whatever the field's MLP mode -- in the bf16 speed mode this is the gradient of the exact network
//      at the same point;
//   4. the contraction of the input cotangents with the Jacobians.
// The weights are read with wave-uniform addresses (scalar loads, SGPR operands of the FMAs): every lane evaluates the same network
// on its own point, so no weight ever needs a per-lane copy.
//
// Ray points p = o + d z (run_network normalises by the box): the launch writes d p / ext per point, and k_ray_point_reduce sums each
// ray's samples in a fixed order (one wave per ray) -- no float atomics: the result is bitwise reproducible.
#pragma once

#include "naruto_common.h"

namespace naruto {

constexpr int kPgThreads = 128;

// d cdf3(t) / dt (oneblob_cdf3's derivative): only the non-saturated term C(t - r) depends on t
__device__ __forceinline__ float oneblob_dcdf3(float t) {
    const float r = fminf(fmaxf(rintf(t), -1.0f), 1.0f);
    const float u = (t - r) * 16.0f;
    const float v = 1.0f - u * u;
    return fabsf(u) <= 1.0f ? 15.0f * v * v : 0.0f;
}

__global__ __launch_bounds__(kPgThreads) void k_query_bwd_points(LevelTab lt, UncertTab ut, BoxTab bt, PointSrc ps, uint32_t M,
                                                                 const float2* __restrict__ table, const float* __restrict__ ugrid,
                                                                 const float* __restrict__ W0, const float* __restrict__ W1,
                                                                 const float* __restrict__ C0, const float* __restrict__ C1,
                                                                 const float* __restrict__ d_raw, const float* __restrict__ d_geo,
                                                                 const uint32_t* __restrict__ active_idx, const uint32_t* __restrict__ n_active,
                                                                 float* __restrict__ out, int world, int accumulate) {
    // out [M,3]: d x (world == 0, the caller's normalised space) or d p / ext per axis (world == 1: ray points, reduced per ray later)
    const uint32_t M_eff = n_active != nullptr ? n_active[0] : M;
    const uint32_t i = blockIdx.x * (uint32_t)kPgThreads + threadIdx.x;
    if (i >= M_eff) return;
    const uint32_t m = active_idx != nullptr ? active_idx[i] : i;
    float x, y, z;
    load_point(ps, bt, m, x, y, z);

    // ---- 1. hash levels: features in[0..31] and their Jacobian J[feature][axis]
    float in[kInSdf];
    float J[kFeat][3];
    static_for<0, kLevels>([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        uint32_t idx[8];
        float f[6];
        hash_corner_index<T>(lt, x, y, z, idx, f);
        const float2* __restrict__ tl = table + lt.off[T];
        float2 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = tl[idx[c]];
        float a0 = 0.0f, a1 = 0.0f;
        float j0[3] = {0.0f, 0.0f, 0.0f}, j1[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
            const float fx = f[bx], fy = f[2 + by], fz = f[4 + bz];
            const float w = fx * fy * fz;
            a0 = fmaf(w, v[c].x, a0);
            a1 = fmaf(w, v[c].y, a1);
            // d w / d w_axis: the other two factors, signed by the corner's side along the axis
            const float gx = bx ? fy * fz : -(fy * fz);
            const float gy = by ? fx * fz : -(fx * fz);
            const float gz = bz ? fx * fy : -(fx * fy);
            j0[0] = fmaf(gx, v[c].x, j0[0]); j1[0] = fmaf(gx, v[c].y, j1[0]);
            j0[1] = fmaf(gy, v[c].x, j0[1]); j1[1] = fmaf(gy, v[c].y, j1[1]);
            j0[2] = fmaf(gz, v[c].x, j0[2]); j1[2] = fmaf(gz, v[c].y, j1[2]);
        }
        const float s = lt.scale[T];            // d w / d x = scale (pos = fmaf(scale, x, 0.5))
        in[2 * T] = a0;
        in[2 * T + 1] = a1;
#pragma unroll
        for (int d = 0; d < 3; ++d) { J[2 * T][d] = s * j0[d]; J[2 * T + 1][d] = s * j1[d]; }
        // The level's results are pinned here (an empty asm that "changes" them) and the scheduler may not mix levels: otherwise the
        // blends sink to their uses in the MLP, all 128 gathers are hoisted to the top, 256 registers of table values stay live and the
        // kernel spills.  One level's eight gathers in flight at a time; the other waves on the SIMD hide the per-level latency.
        asm volatile("" : "+v"(in[2 * T]), "+v"(in[2 * T + 1]));
#pragma unroll
        for (int d = 0; d < 3; ++d) asm volatile("" : "+v"(J[2 * T][d]), "+v"(J[2 * T + 1][d]));
        __builtin_amdgcn_sched_barrier(0);
    });
    // ---- 2. OneBlob values (the MLP inputs in[32..79])
    {
        float e[kBins];
        oneblob16(x, e);
#pragma unroll
        for (int b = 0; b < kBins; ++b) in[kFeat + b] = e[b];
        oneblob16(y, e);
#pragma unroll
        for (int b = 0; b < kBins; ++b) in[kFeat + kBins + b] = e[b];
        oneblob16(z, e);
#pragma unroll
        for (int b = 0; b < kBins; ++b) in[kFeat + 2 * kBins + b] = e[b];
    }

    // ---- 3a. sdf net forward: h = W0 in, out16 = W1 relu(h)  (one hidden unit at a time; its ReLU mask kept as a bit)
    float o[kOut];
#pragma unroll
    for (int r = 0; r < kOut; ++r) o[r] = 0.0f;
    uint32_t hmask = 0;
#pragma unroll 1
    for (int u = 0; u < kHidden; ++u) {
        const float* __restrict__ w = W0 + u * kInSdf;
        float a = 0.0f, b = 0.0f;
#pragma unroll
        for (int k = 0; k < kInSdf; k += 2) { a = fmaf(w[k], in[k], a); b = fmaf(w[k + 1], in[k + 1], b); }
        const float h = a + b;
        if (h > 0.0f) hmask |= 1u << u;
        const float ha = fmaxf(h, 0.0f);
#pragma unroll
        for (int r = 0; r < kOut; ++r) o[r] = fmaf(W1[r * kHidden + u], ha, o[r]);
    }
    const float* __restrict__ g = d_raw + (size_t)m * 5;
    const float g_r = g[0], g_g = g[1], g_b = g[2], g_sdf = g[3], g_unc = g[4];

    // ---- 3b. colour net forward + backward, one hidden unit at a time: c = C0 [blob48, geo15]; d c = relu'(c) C1^T d rgb;
    //          d [blob48, geo15] += C0^T d c
    float de[kPos];                 // cotangent of the OneBlob inputs (both nets)
    float dout[kOut];               // cotangent of the sdf net's outputs (sdf, geo15)
#pragma unroll
    for (int k = 0; k < kPos; ++k) de[k] = 0.0f;
#pragma unroll
    for (int r = 0; r < kOut; ++r) dout[r] = 0.0f;
    const bool want_rgb = g_r != 0.0f || g_g != 0.0f || g_b != 0.0f;
    if (__any(want_rgb)) {
#pragma unroll 1
        for (int u = 0; u < kHidden; ++u) {
            const float* __restrict__ w = C0 + u * kInCol;
            float a = 0.0f, b = 0.0f;
#pragma unroll
            for (int k = 0; k < kPos; k += 2) { a = fmaf(w[k], in[kFeat + k], a); b = fmaf(w[k + 1], in[kFeat + k + 1], b); }
#pragma unroll
            for (int k = 0; k < kGeo; ++k) b = fmaf(w[kPos + k], o[1 + k], b);
            const float c = a + b;
            const float dc = c > 0.0f ? fmaf(C1[2 * kHidden + u], g_b, fmaf(C1[kHidden + u], g_g, C1[u] * g_r)) : 0.0f;
#pragma unroll
            for (int k = 0; k < kPos; ++k) de[k] = fmaf(w[k], dc, de[k]);
#pragma unroll
            for (int k = 0; k < kGeo; ++k) dout[1 + k] = fmaf(w[kPos + k], dc, dout[1 + k]);
        }
    }
    dout[0] += g_sdf;
    if (d_geo != nullptr) {
        const float* __restrict__ gg = d_geo + (size_t)m * kGeo;
#pragma unroll
        for (int k = 0; k < kGeo; ++k) dout[1 + k] += gg[k];
    }

    // ---- 3c. sdf net backward to its inputs: d h = relu'(h) W1^T d out; d in = W0^T d h
    float df[kFeat];
#pragma unroll
    for (int k = 0; k < kFeat; ++k) df[k] = 0.0f;
#pragma unroll 1
    for (int u = 0; u < kHidden; ++u) {
        float a = 0.0f;
#pragma unroll
        for (int r = 0; r < kOut; ++r) a = fmaf(W1[r * kHidden + u], dout[r], a);
        const float dh = ((hmask >> u) & 1u) ? a : 0.0f;
        const float* __restrict__ w = W0 + u * kInSdf;
#pragma unroll
        for (int k = 0; k < kFeat; ++k) df[k] = fmaf(w[k], dh, df[k]);
#pragma unroll
        for (int k = 0; k < kPos; ++k) de[k] = fmaf(w[kFeat + k], dh, de[k]);
    }

    // ---- 4. contraction: hash Jacobians, OneBlob derivative, uncertainty sample
    float gp[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kFeat; ++k) {
#pragma unroll
        for (int d = 0; d < 3; ++d) gp[d] = fmaf(df[k], J[k][d], gp[d]);
    }
    static_for<0, 3>([&](auto dc) {
        constexpr int D = decltype(dc)::value;
        const float xd = D == 0 ? x : (D == 1 ? y : z);
        // e[b] = cdf3(t_{b+1}) - cdf3(t_b) (bin 15: cdf3(t_0) + 1 - cdf3(t_15)), t_b = b/16 - x:  d e[b] / dx = L[b] - L[b+1],
        // L[b] = d cdf3(t_b) / dt
        float L[kBins];
#pragma unroll
        for (int b = 0; b < kBins; ++b) L[b] = oneblob_dcdf3((float)b * (1.0f / 16.0f) - xd);
        float acc = 0.0f;
#pragma unroll
        for (int b = 0; b < kBins; ++b) acc = fmaf(de[D * kBins + b], L[b] - L[(b + 1) & (kBins - 1)], acc);
        gp[D] += acc;
    });
    if (g_unc != 0.0f) {
        float fx, fy, fz;
        const uint32_t key = uncert_base(ut, x, y, z, fx, fy, fz);
        int32_t ui[8];
        uncert_base_corners(ut, key, ui);
        float su[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = ui[c] >= 0 ? ugrid[ui[c]] : 0.0f;
            const int bx = c & 1, by = (c >> 1) & 1, bz = c >> 2;
            const float wx = bx ? fx : 1.0f - fx, wy = by ? fy : 1.0f - fy, wz = bz ? fz : 1.0f - fz;
            su[0] = fmaf(bx ? wy * wz : -(wy * wz), v, su[0]);
            su[1] = fmaf(by ? wx * wz : -(wx * wz), v, su[1]);
            su[2] = fmaf(bz ? wx * wy : -(wx * wy), v, su[2]);
        }
        gp[0] = fmaf(g_unc * (float)ut.W, su[0], gp[0]);       // coordinate 0 walks the grid's LAST axis (W = Nz)
        gp[1] = fmaf(g_unc * (float)ut.H, su[1], gp[1]);
        gp[2] = fmaf(g_unc * (float)ut.D, su[2], gp[2]);
    }
    float* __restrict__ dst = out + 3 * (size_t)m;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float v = world ? __fdiv_rn(gp[d], bt.bext[d]) : gp[d];
        dst[d] = accumulate ? dst[d] + v : v;
    }
}

// d rays_o[n] = sum_s g[n,s],  d rays_d[n] = sum_s z[n,s] g[n,s]  (g = d p / ext per axis).  One wave per ray: lane l sums the samples
// l, l + 64, ... in order, then the fixed DPP tree of wave_sum -- the same order on every run.
__global__ __launch_bounds__(256) void k_ray_point_reduce(uint32_t n_rays, uint32_t S, const float* __restrict__ gp, const float* __restrict__ z_vals,
                                                          float* __restrict__ d_rays_o, float* __restrict__ d_rays_d, int accumulate) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (n >= n_rays) return;                       // wave-uniform: every lane of a working wave is active for wave_sum
    float so[3] = {0.0f, 0.0f, 0.0f}, sd[3] = {0.0f, 0.0f, 0.0f};
    const float* __restrict__ g = gp + 3 * (size_t)n * S;
    const float* __restrict__ zr = z_vals + (size_t)n * S;
    for (uint32_t s = lane; s < S; s += 64u) {
        const float t = zr[s];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = g[3 * s + d];
            so[d] += v;
            sd[d] = fmaf(t, v, sd[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        so[d] = wave_sum(so[d]);
        sd[d] = wave_sum(sd[d]);
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d_rays_o != nullptr) d_rays_o[3 * n + d] = accumulate ? d_rays_o[3 * n + d] + so[d] : so[d];
            if (d_rays_d != nullptr) d_rays_d[3 * n + d] = accumulate ? d_rays_d[3 * n + d] + sd[d] : sd[d];
        }
    }
}

}  // namespace naruto
