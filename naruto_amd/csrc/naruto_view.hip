// Whole views from the field, and their 2D scores (naruto_amd/render.py states the contract; Co-SLAM's render_img is not in the reference
// tree and the surface search is this library's own: parity unpinned).
//
//   k_view_rays      pixel range [p0, p1) of n_poses poses -> rays_o / rays_d: slam.camera_rays' direction, each operation rounded once,
//                    taken to the world as k_rays_to_world does it
//   k_view_crossing  the coarse pass's raw [N,S,5] / z_vals [N,S] -> z* [N]: the first k with sdf[k] > 0 and !(sdf[k+1] > 0), interpolated
//   k_render_view    ONE launch from pose and pixel to the images, one wave per ray as in k_render_fwd: ray -> coarse pass (n_coarse uniform
//                    depths, sdf net only, a tile's sdf in the wave's registers) -> crossing by a wave scan -> fine pass around z* ->
//                    compositing.  The coarse pass stops after the 64-sample tile that decides the first crossing: what the fusion saves.
//                    Same sampling, tile and compositing functions as naruto_render_fwd's kernels, same bits -- which takes two forms, as
//                    that launch has two: k_render_view for more than 64 fine samples, k_render_view_packed (16 rays per workgroup, the
//                    fine pass in the packed render's tiles) below.
//   k_metrics_tile / k_metrics_finish   squared error, absolute depth error and SSIM (Wang et al. 2004) per view in float64; the separable
//                    11-tap filter is tiled through LDS, per-workgroup partials and one finishing pass in a fixed order (no atomics).

#include "naruto_common.h"

namespace naruto {

struct ViewCam { uint32_t H, W; float fx, fy, cx, cy; };

// ray of flat pixel g (pose-major, then row, then column); every lane of a wave may compute the same one
__device__ __forceinline__ void view_ray(const ViewCam& c, const float* __restrict__ poses, uint32_t g, float o[3], float d[3]) {
#pragma clang fp contract(off)
    const uint32_t hw = c.H * c.W;
    const uint32_t pose = g / hw, pix = g - pose * hw;
    const uint32_t j = pix / c.W, i = pix - j * c.W;
    const float dx = __fdiv_rn(__fsub_rn((float)i, c.cx), c.fx);
    const float dy = -__fdiv_rn(__fsub_rn((float)j, c.cy), c.fy);
    const float dz = -1.0f;
    const float* P = poses + 16 * (size_t)pose;
    // k_rays_to_world's arithmetic as it is compiled (its sum of three products is contracted: ONE product is rounded on its own, the other two
    // are fused into the sum), written out so that it does not depend on what this function is inlined into: row 0 rounds dx P0, rows 1 and 2
    // round dy P1.  tests/test_gpu_view.py holds the two equal in every bit.
    d[0] = fmaf(dz, P[2], fmaf(dy, P[1], dx * P[0]));
    d[1] = fmaf(dz, P[6], fmaf(dx, P[4], dy * P[5]));
    d[2] = fmaf(dz, P[10], fmaf(dx, P[8], dy * P[9]));
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = P[4 * k + 3];
}

__global__ __launch_bounds__(256) void k_view_rays(ViewCam c, const float* __restrict__ poses, uint32_t p0, uint32_t n, float* __restrict__ rays_o,
                                                   float* __restrict__ rays_d) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    float o[3], d[3];
    view_ray(c, poses, p0 + r, o, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) { rays_o[3 * (size_t)r + k] = o[k]; rays_d[3 * (size_t)r + k] = d[k]; }
}

// the crossing rule's two halves: is (s0, s1) a crossing, and where
__device__ __forceinline__ bool is_crossing(float s0, float s1) { return s0 > 0.0f && !(s1 > 0.0f); }
__device__ __forceinline__ float crossing_depth(float z0, float z1, float s0, float s1) {
    // plain operators under contract(off): the __f*_rn forms are header functions compiled with contraction allowed, and the product would be
    // fused into the sum
#pragma clang fp contract(off)
    return z0 + (z1 - z0) * (s0 / (s0 - s1));
}

__global__ __launch_bounds__(256) void k_view_crossing(uint32_t n_rays, uint32_t S, const float* __restrict__ raw, const float* __restrict__ z_vals,
                                                       float* __restrict__ z_star) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const float* sdf = raw + (size_t)n * S * 5 + 3;
    uint32_t first = 0xFFFFFFFFu;
    for (uint32_t s = lane; s + 1 < S; s += 64) {
        if (is_crossing(sdf[(size_t)s * 5], sdf[(size_t)(s + 1) * 5])) { first = s; break; }       // lane-local first; strided => global min below
    }
    first = wave_min_u32(first);
    if (lane == 0) {
        const float* z = z_vals + (size_t)n * S;
        z_star[n] = first == 0xFFFFFFFFu ? 0.0f : crossing_depth(z[first], z[first + 1], sdf[(size_t)first * 5], sdf[(size_t)(first + 1) * 5]);
    }
}

struct ViewArgs {
    ViewCam cam;
    const float* poses;
    uint32_t p0, n_rays;                         // flat pixels [p0, p0 + n_rays); every output is indexed by the flat pixel
    const float* target_d;                       // [n_poses*H*W] or NULL (then the coarse pass finds z*)
    float near_, far_, range_d; uint32_t nu, nr, n_coarse;
    float trunc, sc_factor; int white_bkgd;
    float *rgb, *depth, *acc, *depth_var, *uncert_map, *surface_z;      // any may be NULL
};

// the 64-sample tile at depths t of one ray: the field's raw values of this lane's sample (k_render_fwd's arithmetic)
template <bool COLOR, typename LDS>
__device__ __forceinline__ void view_tile(const LDS& L, const LevelTab& lt, const UncertTab& ut, const BoxTab& bt, const NarutoParams& p, const float2* __restrict__ table,
                                          const float o[3], const float d[3], float t, int lane, FwdTileOut& to, float& u) {
    const float px = fmaf(d[0], t, o[0]), py = fmaf(d[1], t, o[1]), pz = fmaf(d[2], t, o[2]);
    const float x = __fdiv_rn(__fsub_rn(px, bt.bmin[0]), bt.bext[0]);
    const float y = __fdiv_rn(__fsub_rn(py, bt.bmin[1]), bt.bext[1]);
    const float z = __fdiv_rn(__fsub_rn(pz, bt.bmin[2]), bt.bext[2]);
    if constexpr (COLOR) u = uncert_sample(ut, p.uncert_grid, x, y, z);
    fwd_tile<COLOR>(L, lt, table, x, y, z, nullptr, nullptr, 0u, 0u, 0u, lane, to);
}

// the surface search of one ray by its wave: the coarse pass's 64-sample tiles from the camera, stopped after the tile that decides the first crossing
template <typename LDS>
__device__ __forceinline__ float view_search(const LDS& L, const LevelTab& lt, const UncertTab& ut, const BoxTab& bt, const NarutoParams& p, const float2* __restrict__ table,
                                             const float o[3], const float d[3], float near_, float far_, uint32_t nc, int lane) {
    const uint32_t n_tiles = (nc + 63u) / 64u;
    float prev_sdf = 0.0f, prev_z = 0.0f;
    for (uint32_t tq = 0; tq < n_tiles; ++tq) {
        const uint32_t s_raw = tq * 64u + (uint32_t)lane;
        const bool valid = s_raw < nc;
        const float t = linspace_at(near_, far_, nc, valid ? s_raw : nc - 1u);
        FwdTileOut to;
        float u_unused;
        view_tile<false>(L, lt, ut, bt, p, table, o, d, t, lane, to, u_unused);
        const float sdf = to.sdf;
        // the pair that straddles the tiles first: it lies before every pair of this tile
        if (tq > 0u && is_crossing(prev_sdf, lane_f32(sdf, 0))) return crossing_depth(prev_z, lane_f32(t, 0), prev_sdf, lane_f32(sdf, 0));
        const float nb = __shfl_down(sdf, 1, 64), tn = __shfl_down(t, 1, 64);
        const bool pair = lane < 63 && s_raw + 1u < nc && is_crossing(sdf, nb);
        const uint32_t first = wave_min_u32(pair ? (uint32_t)lane : 0xFFFFFFFFu);
        if (first != 0xFFFFFFFFu) return __shfl(crossing_depth(t, tn, sdf, nb), (int)first, 64);
        prev_sdf = lane_f32(sdf, 63);
        prev_z = lane_f32(t, 63);
    }
    return 0.0f;
}

template <bool BF>
__global__ __launch_bounds__(256, 2) void k_render_view(LevelTab lt, UncertTab ut, BoxTab bt, NarutoParams p, ViewArgs a) {
    using Lds = std::conditional_t<BF, FwdLdsBf, FwdLds>;
    __shared__ Lds L;
    extern __shared__ float ray_lds[];
    stage_fwd_weights<256>(L, p, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t S = a.nu + a.nr;
    const float2* __restrict__ table = reinterpret_cast<const float2*>(p.table);
    const RayScratch rs = ray_scratch(ray_lds, wave, S);
    const float trunc_sc = a.trunc * a.sc_factor;
    for (uint32_t n = blockIdx.x * 4u + wave; n < a.n_rays; n += gridDim.x * 4u) {
        const uint32_t g = a.p0 + n;
        float o[3], d[3];
        view_ray(a.cam, a.poses, g, o, d);
        const float zstar = a.target_d != nullptr ? a.target_d[g] : view_search(L, lt, ut, bt, p, table, o, d, a.near_, a.far_, a.n_coarse, lane);
        // the fine pass: naruto_render_fwd's launch with target_d = z*, no jitter
        sample_z_ray_core(0u, true, zstar, a.near_, a.far_, a.nu, a.nr, a.range_d, nullptr, false, 0ull, nullptr, rs.wb, rs.gw, lane, rs.z);
        wave_lds_sync();
        const uint32_t n_tiles = (S + 63u) / 64u;
        bool found = false;
        float zfirst = 0.0f, prev_sdf = 0.0f, prev_z = 0.0f;
        uint32_t s_done = S;                         // samples [s_done, S) were skipped: their raw is zero (k_render_fwd's early termination)
        for (uint32_t tq = 0; tq < n_tiles; ++tq) {
            const uint32_t s_raw = tq * 64u + (uint32_t)lane;
            const bool valid = s_raw < S;
            const uint32_t s = valid ? s_raw : S - 1u;
            const float t = rs.z[s];
            FwdTileOut to;
            float u;
            view_tile<true>(L, lt, ut, bt, p, table, o, d, t, lane, to, u);
            if (valid) {
                rs.c0[s] = to.rgb[0]; rs.c1[s] = to.rgb[1]; rs.c2[s] = to.rgb[2];
                rs.sdf[s] = to.sdf;
                rs.u[s] = u;
            }
            if (tq + 1u < n_tiles) {
                const float sdf = to.sdf;
                if (!found) {
                    if (tq > 0u && prev_sdf * lane_f32(sdf, 0) < 0.0f) {
                        found = true;
                        zfirst = prev_z;
                    } else {
                        const float nb = __shfl_down(sdf, 1, 64);
                        const uint32_t first = wave_min_u32((lane < 63 && sdf * nb < 0.0f) ? (uint32_t)lane : 0xFFFFFFFFu);
                        if (first != 0xFFFFFFFFu) {
                            found = true;
                            zfirst = __shfl(t, (int)first, 64);
                        }
                    }
                }
                const float z_last = lane_f32(t, 63);
                prev_sdf = lane_f32(sdf, 63);
                prev_z = z_last;
                if (found) {
                    const float lim = zfirst + trunc_sc;
                    if (z_last > lim + 1e-5f * fabsf(lim) + 1e-6f) {
                        s_done = (tq + 1u) * 64u;
                        break;
                    }
                }
            }
        }
        for (uint32_t s = s_done + (uint32_t)lane; s < S; s += 64u) { rs.c0[s] = 0.0f; rs.c1[s] = 0.0f; rs.c2[s] = 0.0f; rs.sdf[s] = 0.0f; rs.u[s] = 0.0f; }
        wave_lds_sync();
        const RayWeights rw = ray_weights(rs, S, a.trunc, a.sc_factor, lane);
        const RayOut out = ray_composite(rs, rw, 0u, S, a.white_bkgd, nullptr, lane);
        if (lane == 0) {
            if (a.rgb) { a.rgb[3 * (size_t)g] = out.rgb[0]; a.rgb[3 * (size_t)g + 1] = out.rgb[1]; a.rgb[3 * (size_t)g + 2] = out.rgb[2]; }
            if (a.acc) a.acc[g] = out.acc;
            if (a.depth) a.depth[g] = out.depth;
            if (a.depth_var) a.depth_var[g] = out.depth_var;
            if (a.uncert_map) a.uncert_map[g] = out.uncert;
            if (a.surface_z) a.surface_z[g] = zstar;
        }
        wave_lds_sync();                             // the image is reused by this wave's next ray
    }
}

// Fine passes of at most 64 samples: naruto_render_fwd runs them as k_render_fwd_packed<*, 256> -- kPackRays rays per workgroup, their samples back
// to back in 64-sample tiles -- and OneBlob's form is chosen per TILE (naruto_field.hip), so a sample's bits depend on the tile it shares.  This
// form keeps that launch's tiles: a workgroup takes the same kPackRays rays (groups counted from the launch's first ray), its waves search the
// surface ray by ray (one wave per ray), and the fine pass is that kernel's body.
template <bool BF>
__global__ __launch_bounds__(256, NARUTO_RENDER_PACKED_MINWAVES) void k_render_view_packed(LevelTab lt, UncertTab ut, BoxTab bt, NarutoParams p, ViewArgs a) {
    using Lds = std::conditional_t<BF, FwdLdsBf, FwdLds>;
    __shared__ Lds L;
    __shared__ FwdSlab slabs[4];
    __shared__ float ray_od[kPackRays][6];
    __shared__ float ray_zstar[kPackRays];
    extern __shared__ float ray_lds[];
    stage_fwd_weights<256>(L, p, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t S = a.nu + a.nr;
    const float inv_S = 1.0f / (float)S;
    const float2* __restrict__ table = reinterpret_cast<const float2*>(p.table);
    auto image = [&](uint32_t r) { return ray_scratch(ray_lds, (int)r, S); };
    for (uint32_t n0 = blockIdx.x * kPackRays; n0 < a.n_rays; n0 += gridDim.x * kPackRays) {
        const uint32_t R = a.n_rays - n0 < kPackRays ? a.n_rays - n0 : kPackRays;
        // rays, surface search and depths: wave w takes rays w, w + 4, ...
        for (uint32_t r = (uint32_t)wave; r < R; r += 4u) {
            const uint32_t g = a.p0 + n0 + r;
            float o[3], d[3];
            view_ray(a.cam, a.poses, g, o, d);
            const float zstar = a.target_d != nullptr ? a.target_d[g] : view_search(L, lt, ut, bt, p, table, o, d, a.near_, a.far_, a.n_coarse, lane);
            if (lane == 0) {
                ray_od[r][0] = o[0]; ray_od[r][1] = o[1]; ray_od[r][2] = o[2]; ray_od[r][3] = d[0]; ray_od[r][4] = d[1]; ray_od[r][5] = d[2];
                ray_zstar[r] = zstar;
            }
            const RayScratch rs = image(r);
            sample_z_ray_core(0u, true, zstar, a.near_, a.far_, a.nu, a.nr, a.range_d, nullptr, false, 0ull, nullptr, rs.wb, rs.gw, lane, rs.z);
        }
        __syncthreads();
        const uint32_t T = R * S, n_tiles = (T + 63u) / 64u;
        for (uint32_t tq = (uint32_t)wave; tq < n_tiles; tq += 4u) {
            const uint32_t g_raw = tq * 64u + (uint32_t)lane;
            const bool valid = g_raw < T;
            uint32_t s;
            const uint32_t r = fast_divmod(valid ? g_raw : T - 1u, S, inv_S, s);
            const RayScratch rs = image(r);
            const float t = rs.z[s];
            const float px = fmaf(ray_od[r][3], t, ray_od[r][0]), py = fmaf(ray_od[r][4], t, ray_od[r][1]), pz = fmaf(ray_od[r][5], t, ray_od[r][2]);
            const float x = __fdiv_rn(__fsub_rn(px, bt.bmin[0]), bt.bext[0]);
            const float y = __fdiv_rn(__fsub_rn(py, bt.bmin[1]), bt.bext[1]);
            const float z = __fdiv_rn(__fsub_rn(pz, bt.bmin[2]), bt.bext[2]);
            const float u = uncert_sample(ut, p.uncert_grid, x, y, z);
            FwdTileOut to;
            fwd_tile_split<true, false>(L, slabs[wave], lt, table, x, y, z, nullptr, nullptr, 0u, 0u, 0u, lane, to);
            if (valid) {
                rs.c0[s] = to.rgb[0]; rs.c1[s] = to.rgb[1]; rs.c2[s] = to.rgb[2];
                rs.sdf[s] = to.sdf;
                rs.u[s] = u;
            }
        }
        __syncthreads();
        for (uint32_t r = (uint32_t)wave; r < R; r += 4u) {
            const RayScratch rs = image(r);
            const uint32_t g = a.p0 + n0 + r;
            const RayWeights rw = ray_weights(rs, S, a.trunc, a.sc_factor, lane);
            const RayOut out = ray_composite(rs, rw, 0u, S, a.white_bkgd, nullptr, lane);
            if (lane == 0) {
                if (a.rgb) { a.rgb[3 * (size_t)g] = out.rgb[0]; a.rgb[3 * (size_t)g + 1] = out.rgb[1]; a.rgb[3 * (size_t)g + 2] = out.rgb[2]; }
                if (a.acc) a.acc[g] = out.acc;
                if (a.depth) a.depth[g] = out.depth;
                if (a.depth_var) a.depth_var[g] = out.depth_var;
                if (a.uncert_map) a.uncert_map[g] = out.uncert;
                if (a.surface_z) a.surface_z[g] = ray_zstar[r];
            }
        }
        __syncthreads();                             // the images are reused by the next group
    }
}

// ------------------------------------------------------------------------------------------------
// Image metrics.  One workgroup = one 16 x 16 tile of one view: its pixels' squared error and depth error, and the SSIM of the window
// positions whose top-left corner lies in the tile (a position (r, c) reads pixels r .. r+10, c .. c+10).
// ------------------------------------------------------------------------------------------------
constexpr int kMetTile = 16, kMetWin = 11, kMetIn = kMetTile + kMetWin - 1;      // 26 x 26 input pixels per tile
struct MetricWin { double w[kMetWin]; };
struct MetricArgs {
    uint32_t P, H, W, tiles_x, tiles_y;
    const float *rgb, *depth, *gt_rgb, *gt_depth;
    float depth_trunc; int has_trunc;
    double* partial;                             // [P][tiles][6]
    double *se_map, *de_map, *ssim_map;          // optional
};

// sum over the workgroup's 256 threads in a fixed order: the wave's butterfly, then the four waves in order
__device__ __forceinline__ double block_sum_256(double v, double* part /* LDS [4] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(256) void k_metrics_tile(MetricArgs a, MetricWin win) {
#pragma clang fp contract(off)
    __shared__ float tx[kMetIn][kMetIn], ty[kMetIn][kMetIn];
    __shared__ double hq[5][kMetIn][kMetTile];
    __shared__ double part[4];
    const uint32_t view = blockIdx.z, r0 = blockIdx.y * kMetTile, c0 = blockIdx.x * kMetTile;
    const uint32_t lr = threadIdx.x / kMetTile, lc = threadIdx.x % kMetTile, r = r0 + lr, c = c0 + lc;
    const bool in_image = r < a.H && c < a.W;
    const size_t pix = ((size_t)view * a.H + r) * a.W + c;
    const bool has_ssim = a.H >= (uint32_t)kMetWin && a.W >= (uint32_t)kMetWin;
    const uint32_t Hs = has_ssim ? a.H - (kMetWin - 1) : 0u, Ws = has_ssim ? a.W - (kMetWin - 1) : 0u;
    const bool in_ssim = r < Hs && c < Ws;
    double se = 0.0, de = 0.0, nv = 0.0, ss = 0.0;
    if (in_image) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double e = (double)a.rgb[pix * 3 + ch] - (double)a.gt_rgb[pix * 3 + ch];
            const double e2 = e * e;
            se += e2;
            if (a.se_map) a.se_map[pix * 3 + ch] = e2;
        }
        const float dg = a.gt_depth[pix];
        const bool valid = dg > 0.0f && (!a.has_trunc || dg <= a.depth_trunc);
        const double ad = valid ? fabs((double)a.depth[pix] - (double)dg) : 0.0;
        de = ad;
        nv = valid ? 1.0 : 0.0;
        if (a.de_map) a.de_map[pix] = ad;
    }
    if (has_ssim && r0 < Hs && c0 < Ws) {              // (uniform over the workgroup)
        for (int ch = 0; ch < 3; ++ch) {
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < (uint32_t)(kMetIn * kMetIn); k += 256u) {
                const uint32_t rr = k / kMetIn, cc = k % kMetIn;
                const bool ok = r0 + rr < a.H && c0 + cc < a.W;
                const size_t q = (((size_t)view * a.H + r0 + rr) * a.W + c0 + cc) * 3 + ch;
                tx[rr][cc] = ok ? a.rgb[q] : 0.0f;
                ty[rr][cc] = ok ? a.gt_rgb[q] : 0.0f;
            }
            __syncthreads();
            // horizontal pass: rows of the input tile x the tile's 16 columns
            for (uint32_t k = threadIdx.x; k < (uint32_t)(kMetIn * kMetTile); k += 256u) {
                const uint32_t rr = k / kMetTile, cc = k % kMetTile;
                double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
                for (int t = 0; t < kMetWin; ++t) {
                    const double x = (double)tx[rr][cc + t], y = (double)ty[rr][cc + t], w = win.w[t];
                    h0 = h0 + w * x; h1 = h1 + w * y; h2 = h2 + w * (x * x); h3 = h3 + w * (y * y); h4 = h4 + w * (x * y);
                }
                hq[0][rr][cc] = h0; hq[1][rr][cc] = h1; hq[2][rr][cc] = h2; hq[3][rr][cc] = h3; hq[4][rr][cc] = h4;
            }
            __syncthreads();
            if (in_ssim) {
                double v[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    double s = 0.0;
#pragma unroll
                    for (int t = 0; t < kMetWin; ++t) s = s + win.w[t] * hq[q][lr + t][lc];
                    v[q] = s;
                }
                const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
                const double mx = v[0], my = v[1];
                const double sx = v[2] - mx * mx, sy = v[3] - my * my, sxy = v[4] - mx * my;
                const double num = (2.0 * mx * my + C1) * (2.0 * sxy + C2);
                const double den = (mx * mx + my * my + C1) * (sx + sy + C2);
                const double s = num / den;
                ss += s;
                if (a.ssim_map) a.ssim_map[(((size_t)view * Hs + r) * Ws + c) * 3 + ch] = s;
            }
        }
    }
    const double v6[6] = {se, in_image ? 1.0 : 0.0, de, nv, ss, in_ssim ? 3.0 : 0.0};
    double* out = a.partial + ((size_t)view * a.tiles_x * a.tiles_y + (size_t)blockIdx.y * a.tiles_x + blockIdx.x) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double t = block_sum_256(v6[k], part);
        if (threadIdx.x == 0) out[k] = t;
    }
}

// partial [P][tiles][6] -> out [P][6]: thread k of workgroup `view` adds its column in tile order
__global__ __launch_bounds__(64) void k_metrics_finish(uint32_t n_tiles, const double* __restrict__ partial, double* __restrict__ out) {
    if (threadIdx.x >= 6) return;
    const double* p = partial + (size_t)blockIdx.x * n_tiles * 6 + threadIdx.x;
    double s = 0.0;
    for (uint32_t t = 0; t < n_tiles; ++t) s += p[(size_t)t * 6];
    out[(size_t)blockIdx.x * 6 + threadIdx.x] = s;
}

}  // namespace naruto
