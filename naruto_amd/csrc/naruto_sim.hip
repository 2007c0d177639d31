// Mesh simulator on the device (the first line of the reference's run loop, src/naruto/main.py: sim.simulate(c2w); HabitatSim is an external
// renderer that is not on this stack, so this is PARITY UNPINNED against it -- only the cube-to-panorama gather, src/layers/c2e.py, and
// erp_conversions.depth2dist are pinned, by recorded results in tests/golden/g13_c2e.npz).  A mesh stands in for the scene: RGB-D frames of
// a pinhole camera, the six cube faces around a pose, the equirectangular (ERP) panorama of radial distance the planner's movement check
// reads (naruto_planner.py:544-547), and its two scalars.  The contract is restated in naruto_amd/simulator.py and pinned by the numpy
// float32 restatement tests/sim_spec.py, which every kernel here equals bit for bit.
//
// The rasteriser is naruto_cull.hip's (camera space, CullTri, the candidate box, the small and the large route), instantiated on a 64-bit
// cell: (depth bits << 32) | face index under an integer atomicMin.  Depths are positive, so the minimum is the nearest depth and, among
// the faces that hit at exactly that depth, the lowest index -- independent of the order of arrival.  Cells start as (+inf, 0xFFFFFFFF).
//
// Kernels
//   k_sim_fill2      pairs of 32-bit words: the winner cells' start value, the statistics' start value
//   k_sim_shade      one thread per (pose, pixel): cell -> depth, face id, colour
//   k_sim_shade_tex  k_sim_shade with materials: a face's colour is its vertex colours (no material: k_sim_shade's bits), its material's factor,
//                    or one bilinear tap of its texture at the mip level of the pixel's footprint, times the factor
//   k_tex_down       one thread per texel of a mip level: the 2 x 2 box of the level above, in integers
//   k_sim_erp        one thread per (panorama, ERP pixel): table -> cube pixel; distance and colour gathered; minimum and count per wave,
//                    then one integer atomicMin and one integer atomicAdd per wave (both independent of the order)
//   k_sim_gather     cube_to_erp: [C,6,s,s] -> [C,h,w] through the table (32-bit words)
//   k_sim_dist       depth_to_dist: [N,H,W] depth times the norm of the pixel ray
//
// Arithmetic (fp32, this order, no contraction; divide and square root correctly rounded):
//   shade      e_ab, e_bc, e_ca: the rasteriser's edge values of the winning face at the pixel ray (naruto_cull.hip);
//              s = (e_ab + e_bc) + e_ca;  w_a = e_bc/s, w_b = e_ca/s, w_c = e_ab/s  (perspective correct: the edge planes pass through the eye)
//              colour_k = (w_a*ca_k + w_b*cb_k) + w_c*cc_k;  vertex colours RGBA8 (c = byte / 255.0f) or float32 [V,3]
//              nothing hit: depth 0 (or +inf with NARUTO_SIM_KEEP_INF), colour 0, id -1
//   textures   all mip chains in one buffer of RGBA8 words, R in the lowest byte; level l+1 is max(1, w >> 1) x max(1, h >> 1) and its texel
//              (x, y) is, per channel, (t(xa,ya) + t(xb,ya) + t(xa,yb) + t(xb,yb) + 2) >> 2, xa = min(2x, w-1), xb = min(2x+1, w-1), y likewise
//   shade tex  u = (w_a*u_a + w_b*u_b) + w_c*u_c, v likewise; (u_x, v_x) and (u_y, v_y): the same at the rays of pixels (i+1, j) and (i, j+1) with
//              the same face's edge values (extrapolated beyond the face); ax = (u_x - u)*W0, bx = (v_x - v)*H0, rx = ax*ax + bx*bx, ay, by, ry
//              likewise; rho2 = rx, or ry where ry > rx (a NaN never wins); level = the number of k in 0 .. n_levels-2 with rho2 > 4^k: no
//              log2, NaN gives level 0, +inf the last.  One level per pixel, one bilinear tap at its size (w, h), glTF's convention (uv (0, 0)
//              is the corner of the first stored row): x = u*w - 0.5f, y = v*h - 0.5f; unless |x| < 2^30 and |y| < 2^30 the texel colour is 0;
//              x0 = (int)floorf(x), a = x - x0, y0 and b likewise; x0, x0+1 (y0, y0+1) wrapped by the axis's mode into the level, whatever
//              the input; t = byte / 255.0f; top = t00 + a*(t10 - t00), bot = t01 + a*(t11 - t01), c = top + b*(bot - top); colour = c * factor.
//              Alpha is stored and ignored.  No lighting, no trilinear or anisotropic filtering, no texture transform.  Plain global loads,
//              a dword per texel: the level keeps a pixel's footprint near one texel, so neighbouring lanes read neighbouring dwords.
//   panorama   cube pixel (ci, cj) of plane p = table[k] / s^2:  dx = (ci - c)/c, dy = -((cj - c)/c), c = (s-1)/2;
//              r = sqrtf((dx*dx + dy*dy) + 1);  dist = t*r;  a miss (t = 0 or +inf): 1e8f * r
//   dist       dx = (i - cx)/fx, dy = (j - cy)/fy, r as above, dist = depth * r

#include "naruto_common.h"

namespace naruto {

constexpr int kSimThreads = 256;
constexpr uint32_t kSimNoFace = 0xFFFFFFFFu;
constexpr float kSimInvalid = 1e8f;

__global__ __launch_bounds__(kSimThreads) void k_sim_fill2(uint64_t n_pairs, uint32_t w0, uint32_t w1, uint2* __restrict__ p) {
    const uint64_t k = (uint64_t)blockIdx.x * kSimThreads + threadIdx.x;
    if (k < n_pairs) p[k] = make_uint2(w0, w1);
}

__device__ __forceinline__ void sim_vertex_colour(const void* __restrict__ colors, int colors_f32, uint32_t v, float* c) {
#pragma clang fp contract(off)
    if (colors_f32) {
        const float* p = reinterpret_cast<const float*>(colors) + (size_t)v * 3u;
        c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    } else {
        const uint32_t w = reinterpret_cast<const uint32_t*>(colors)[v];            // R in the lowest byte
        c[0] = (float)(w & 255u) / 255.0f; c[1] = (float)((w >> 8) & 255u) / 255.0f; c[2] = (float)((w >> 16) & 255u) / 255.0f;
    }
}

// grid (pixels / 256, poses).  camv is the raster's workspace: the camera-space vertices of the same poses.
__global__ __launch_bounds__(kSimThreads) void k_sim_shade(CullCam cam, uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                           const void* __restrict__ colors, int colors_f32, const float4* __restrict__ camv,
                                                           const unsigned long long* __restrict__ cells, int keep_inf, float* __restrict__ depth,
                                                           float* __restrict__ color, int32_t* __restrict__ face_id) {
#pragma clang fp contract(off)
    const uint32_t px = blockIdx.x * kSimThreads + threadIdx.x, pose = blockIdx.y, n_px = cam.H * cam.W;
    if (px >= n_px) return;
    const size_t at = (size_t)pose * n_px + px;
    const unsigned long long cell = cells[at];
    const uint32_t f = (uint32_t)cell;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    bool hit = f != kSimNoFace && f < n_faces;
    float4 a, b, c;
    hit = hit && cull_load_triangle(faces, f, n_vertices, camv + (size_t)pose * n_vertices, a, b, c);
    if (depth != nullptr) depth[at] = hit ? __uint_as_float((uint32_t)(cell >> 32)) : (keep_inf ? __uint_as_float(kCullInfBits) : 0.0f);
    if (face_id != nullptr) face_id[at] = hit ? (int32_t)f : -1;
    if (color == nullptr) return;
    if (hit) {
        const uint32_t j = px / cam.W, i = px - j * cam.W;
        const float dx = ((float)i - cam.cx) / cam.fx;
        const float dy = -(((float)j - cam.cy) / cam.fy);
        const float pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z}, pc[3] = {c.x, c.y, c.z};
        float nab[3], nbc[3], nca[3];
        cull_cross(pa, pb, nab);
        cull_cross(pb, pc, nbc);
        cull_cross(pc, pa, nca);
        const float e_ab = (dx * nab[0] + dy * nab[1]) - nab[2];
        const float e_bc = (dx * nbc[0] + dy * nbc[1]) - nbc[2];
        const float e_ca = (dx * nca[0] + dy * nca[1]) - nca[2];
        const float s = (e_ab + e_bc) + e_ca;
        const float wa = e_bc / s, wb = e_ca / s, wc = e_ab / s;
        float ca[3], cb[3], cc[3];
        sim_vertex_colour(colors, colors_f32, (uint32_t)faces[(size_t)f * 3u], ca);
        sim_vertex_colour(colors, colors_f32, (uint32_t)faces[(size_t)f * 3u + 1u], cb);
        sim_vertex_colour(colors, colors_f32, (uint32_t)faces[(size_t)f * 3u + 2u], cc);
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = (wa * ca[k] + wb * cb[k]) + wc * cc[k];
    }
    color[at * 3u] = rgb[0]; color[at * 3u + 1u] = rgb[1]; color[at * 3u + 2u] = rgb[2];
}

// ---- textures ------------------------------------------------------------------------------------------------------------------------
// One buffer of RGBA8 words holds every texture's mip chain, level after level; desc [texture][4] = word offset of level 0, W, H, n_levels.
constexpr uint32_t kSimTexMaxSide = 16384u, kSimTexMaxLevels = 15u;
constexpr uint32_t kSimWrapClamp = 33071u, kSimWrapMirror = 33648u;         // anything else: REPEAT (10497), glTF's default

struct SimTex {
    uint32_t n_materials, n_textures;
    unsigned long long n_texels;
    const float* uv;                    // [V,2]
    const int32_t* face_material;       // [F], -1: none
    const uint32_t* materials;          // [n_materials][8]: texture (int32, < 0: none), wrap_s, wrap_t, 0, factor[4] (float32 bits)
    const uint32_t* desc;               // [n_textures][4]
    const uint32_t* texels;             // [n_texels]
};

// grid (texels of the destination level / 256): one 2 x 2 box of the source level per lane, rounded half up per channel
__global__ __launch_bounds__(kSimThreads) void k_tex_down(uint32_t ws, uint32_t hs, uint32_t wd, uint32_t hd, const uint32_t* src, uint32_t* dst) {
    const uint32_t k = blockIdx.x * kSimThreads + threadIdx.x;
    if (k >= wd * hd) return;
    const uint32_t y = k / wd, x = k - y * wd;
    const uint32_t xa = min(2u * x, ws - 1u), xb = min(2u * x + 1u, ws - 1u), ya = min(2u * y, hs - 1u), yb = min(2u * y + 1u, hs - 1u);
    const uint32_t t0 = src[(size_t)ya * ws + xa], t1 = src[(size_t)ya * ws + xb], t2 = src[(size_t)yb * ws + xa], t3 = src[(size_t)yb * ws + xb];
    uint32_t out = 0u;
#pragma unroll
    for (int s = 0; s < 32; s += 8) out |= (((((t0 >> s) & 255u) + ((t1 >> s) & 255u)) + (((t2 >> s) & 255u) + ((t3 >> s) & 255u)) + 2u) >> 2) << s;
    dst[k] = out;
}

// the edge values of the face at the ray (dx, dy, -1) -> barycentrics, k_sim_shade's own expressions
__device__ __forceinline__ void sim_bary(const float* nab, const float* nbc, const float* nca, float dx, float dy, float& wa, float& wb, float& wc) {
#pragma clang fp contract(off)
    const float e_ab = (dx * nab[0] + dy * nab[1]) - nab[2];
    const float e_bc = (dx * nbc[0] + dy * nbc[1]) - nbc[2];
    const float e_ca = (dx * nca[0] + dy * nca[1]) - nca[2];
    const float s = (e_ab + e_bc) + e_ca;
    wa = e_bc / s; wb = e_ca / s; wc = e_ab / s;
}

// index (|i| <= 2^30) into [0, n), n in 1 .. 16384
__device__ __forceinline__ uint32_t sim_wrap(int i, int n, uint32_t mode) {
    if (mode == kSimWrapClamp) return (uint32_t)min(max(i, 0), n - 1);
    if (mode == kSimWrapMirror) {
        int m = i % (2 * n);
        if (m < 0) m += 2 * n;
        return (uint32_t)(m < n ? m : 2 * n - 1 - m);
    }
    int m = i % n;
    if (m < 0) m += n;
    return (uint32_t)m;
}

__device__ __forceinline__ uint32_t sim_texel(const SimTex& tex, unsigned long long at) {
    return at < tex.n_texels ? tex.texels[at] : 0u;                         // (never out of range with descriptors naruto_tex_build wrote)
}

// k_sim_shade with materials: grid (pixels / 256, poses).  A face without a material, with a material or a texture out of range or with a
// descriptor no texture can have takes k_sim_shade's vertex-colour path in its bits; no index read from memory is trusted.
__global__ __launch_bounds__(kSimThreads) void k_sim_shade_tex(CullCam cam, uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                               const void* __restrict__ colors, int colors_f32, const float4* __restrict__ camv,
                                                               const unsigned long long* __restrict__ cells, int keep_inf, SimTex tex,
                                                               float* __restrict__ depth, float* __restrict__ color, int32_t* __restrict__ face_id) {
#pragma clang fp contract(off)
    const uint32_t px = blockIdx.x * kSimThreads + threadIdx.x, pose = blockIdx.y, n_px = cam.H * cam.W;
    if (px >= n_px) return;
    const size_t at = (size_t)pose * n_px + px;
    const unsigned long long cell = cells[at];
    const uint32_t f = (uint32_t)cell;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    bool hit = f != kSimNoFace && f < n_faces;
    float4 a, b, c;
    hit = hit && cull_load_triangle(faces, f, n_vertices, camv + (size_t)pose * n_vertices, a, b, c);
    if (depth != nullptr) depth[at] = hit ? __uint_as_float((uint32_t)(cell >> 32)) : (keep_inf ? __uint_as_float(kCullInfBits) : 0.0f);
    if (face_id != nullptr) face_id[at] = hit ? (int32_t)f : -1;
    if (color == nullptr) return;
    if (hit) {
        const uint32_t j = px / cam.W, i = px - j * cam.W;
        const float dx = ((float)i - cam.cx) / cam.fx;
        const float dy = -(((float)j - cam.cy) / cam.fy);
        const float pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z}, pc[3] = {c.x, c.y, c.z};
        float nab[3], nbc[3], nca[3];
        cull_cross(pa, pb, nab);
        cull_cross(pb, pc, nbc);
        cull_cross(pc, pa, nca);
        float wa, wb, wc;
        sim_bary(nab, nbc, nca, dx, dy, wa, wb, wc);
        const uint32_t i0 = (uint32_t)faces[(size_t)f * 3u], i1 = (uint32_t)faces[(size_t)f * 3u + 1u], i2 = (uint32_t)faces[(size_t)f * 3u + 2u];
        const int32_t mat = tex.face_material[f];
        bool shaded = false;
        if (mat >= 0 && (uint32_t)mat < tex.n_materials) {
            const uint32_t* m = tex.materials + (size_t)mat * 8u;
            const int32_t ti = (int32_t)m[0];
            const float fac[3] = {__uint_as_float(m[4]), __uint_as_float(m[5]), __uint_as_float(m[6])};
            if (ti < 0) {
                rgb[0] = fac[0]; rgb[1] = fac[1]; rgb[2] = fac[2];
                shaded = true;
            } else if ((uint32_t)ti < tex.n_textures) {
                const uint32_t* d = tex.desc + (size_t)ti * 4u;
                const uint32_t W0 = d[1], H0 = d[2], n_levels = d[3];
                if (W0 >= 1u && W0 <= kSimTexMaxSide && H0 >= 1u && H0 <= kSimTexMaxSide && n_levels >= 1u && n_levels <= kSimTexMaxLevels) {
                    shaded = true;
                    const float ua = tex.uv[(size_t)i0 * 2u], va = tex.uv[(size_t)i0 * 2u + 1u];
                    const float ub = tex.uv[(size_t)i1 * 2u], vb = tex.uv[(size_t)i1 * 2u + 1u];
                    const float uc = tex.uv[(size_t)i2 * 2u], vc = tex.uv[(size_t)i2 * 2u + 1u];
                    const float u = (wa * ua + wb * ub) + wc * uc, v = (wa * va + wb * vb) + wc * vc;
                    // the footprint: the same face's uv at the rays of the pixels to the right and below
                    const float dx1 = ((float)(i + 1u) - cam.cx) / cam.fx;
                    const float dy1 = -(((float)(j + 1u) - cam.cy) / cam.fy);
                    float xa, xb, xc, ya, yb, yc;
                    sim_bary(nab, nbc, nca, dx1, dy, xa, xb, xc);
                    sim_bary(nab, nbc, nca, dx, dy1, ya, yb, yc);
                    const float u_x = (xa * ua + xb * ub) + xc * uc, v_x = (xa * va + xb * vb) + xc * vc;
                    const float u_y = (ya * ua + yb * ub) + yc * uc, v_y = (ya * va + yb * vb) + yc * vc;
                    const float ax = (u_x - u) * (float)W0, bx = (v_x - v) * (float)H0;
                    const float ay = (u_y - u) * (float)W0, by = (v_y - v) * (float)H0;
                    const float rx = ax * ax + bx * bx, ry = ay * ay + by * by;
                    float rho2 = rx;
                    if (ry > rx) rho2 = ry;
                    // the level: the number of k in 0 .. n_levels - 2 with rho2 > 4^k (a prefix: the powers grow)
                    uint32_t w = W0, h = H0;
                    unsigned long long off = d[0];
                    float power = 1.0f;
#pragma unroll 1
                    for (uint32_t k = 0; k + 1u < n_levels && rho2 > power; ++k) {
                        off += (unsigned long long)w * h;
                        w = max(1u, w >> 1); h = max(1u, h >> 1);
                        power *= 4.0f;
                    }
                    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
                    float tc[3] = {0.0f, 0.0f, 0.0f};
                    if (fabsf(x) < 1073741824.0f && fabsf(y) < 1073741824.0f) {
                        const float fx0 = floorf(x), fy0 = floorf(y);
                        const int x0 = (int)fx0, y0 = (int)fy0;
                        const float fa = x - fx0, fb = y - fy0;
                        const uint32_t ws = m[1], wt = m[2];
                        const uint32_t cx0 = sim_wrap(x0, (int)w, ws), cx1 = sim_wrap(x0 + 1, (int)w, ws);
                        const uint32_t cy0 = sim_wrap(y0, (int)h, wt), cy1 = sim_wrap(y0 + 1, (int)h, wt);
                        const uint32_t t00 = sim_texel(tex, off + (unsigned long long)cy0 * w + cx0), t10 = sim_texel(tex, off + (unsigned long long)cy0 * w + cx1);
                        const uint32_t t01 = sim_texel(tex, off + (unsigned long long)cy1 * w + cx0), t11 = sim_texel(tex, off + (unsigned long long)cy1 * w + cx1);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float c00 = (float)((t00 >> (8 * k)) & 255u) / 255.0f, c10 = (float)((t10 >> (8 * k)) & 255u) / 255.0f;
                            const float c01 = (float)((t01 >> (8 * k)) & 255u) / 255.0f, c11 = (float)((t11 >> (8 * k)) & 255u) / 255.0f;
                            const float top = c00 + fa * (c10 - c00), bot = c01 + fa * (c11 - c01);
                            tc[k] = top + fb * (bot - top);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) rgb[k] = tc[k] * fac[k];
                }
            }
        }
        if (!shaded) {
            float ca[3], cb[3], cc[3];
            sim_vertex_colour(colors, colors_f32, i0, ca);
            sim_vertex_colour(colors, colors_f32, i1, cb);
            sim_vertex_colour(colors, colors_f32, i2, cc);
#pragma unroll
            for (int k = 0; k < 3; ++k) rgb[k] = (wa * ca[k] + wb * cb[k]) + wc * cc[k];
        }
    }
    color[at * 3u] = rgb[0]; color[at * 3u + 1u] = rgb[1]; color[at * 3u + 2u] = rgb[2];
}

__device__ __forceinline__ float sim_ray_norm(float dx, float dy) {
#pragma clang fp contract(off)
    return sqrtf((dx * dx + dy * dy) + 1.0f);
}

// grid (ERP pixels / 256, panoramas).  table [n_erp]: index into one panorama's six cube planes [6, s, s], checked on the host.
// stats [panorama][2]: the minimum distance's bit pattern (distances are positive) and the number of pixels above the threshold.
__global__ __launch_bounds__(kSimThreads) void k_sim_erp(uint32_t face_w, uint32_t n_erp, const int32_t* __restrict__ table, const float* __restrict__ cube_depth,
                                                         const float* __restrict__ cube_color, float invalid_thre, float* __restrict__ erp_dist,
                                                         float* __restrict__ erp_color, uint32_t* __restrict__ stats) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * kSimThreads + threadIdx.x, pano = blockIdx.y;
    const uint32_t plane_px = face_w * face_w, cube_px = 6u * plane_px;
    const bool live = k < n_erp;
    uint32_t bits = 0xFFFFFFFFu;
    bool above = false;
    if (live) {
        uint32_t src = (uint32_t)table[k];
        if (src >= cube_px) src = 0u;                                       // (never: the host checks the table)
        const uint32_t rem = src % plane_px, cj = rem / face_w, ci = rem - cj * face_w;
        const float c = (float)(face_w - 1u) / 2.0f;
        const float dx = ((float)ci - c) / c;
        const float dy = -(((float)cj - c) / c);
        const float r = sim_ray_norm(dx, dy);
        const size_t at = (size_t)pano * cube_px + src;
        const float t = cube_depth[at];
        const bool miss = !(t > 0.0f) || __float_as_uint(t) >= kCullInfBits;
        const float dist = miss ? kSimInvalid * r : t * r;
        bits = __float_as_uint(dist);
        above = dist > invalid_thre;
        const size_t out = (size_t)pano * n_erp + k;
        if (erp_dist != nullptr) erp_dist[out] = dist;
        if (erp_color != nullptr) {
            erp_color[out * 3u] = cube_color[at * 3u]; erp_color[out * 3u + 1u] = cube_color[at * 3u + 1u]; erp_color[out * 3u + 2u] = cube_color[at * 3u + 2u];
        }
    }
    if (stats == nullptr) return;                                           // (uniform)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) bits = min(bits, (uint32_t)__shfl_xor((int)bits, s, 64));
    const uint32_t count = (uint32_t)__popcll(__ballot(above));
    if ((threadIdx.x & 63) == 0) {
        if (bits != 0xFFFFFFFFu) atomicMin(stats + 2u * pano, bits);
        if (count != 0u) atomicAdd(stats + 2u * pano + 1u, count);
    }
}

// grid (ERP pixels / 256, channels)
__global__ __launch_bounds__(kSimThreads) void k_sim_gather(uint32_t cube_px, uint32_t n_erp, const int32_t* __restrict__ table, const uint32_t* __restrict__ src,
                                                            uint32_t* __restrict__ dst) {
    const uint32_t k = blockIdx.x * kSimThreads + threadIdx.x, ch = blockIdx.y;
    if (k >= n_erp) return;
    uint32_t at = (uint32_t)table[k];
    if (at >= cube_px) at = 0u;
    dst[(size_t)ch * n_erp + k] = src[(size_t)ch * cube_px + at];
}

// grid (pixels / 256, images)
__global__ __launch_bounds__(kSimThreads) void k_sim_dist(uint32_t H, uint32_t W, float fx, float fy, float cx, float cy, const float* __restrict__ depth,
                                                          float* __restrict__ dist) {
#pragma clang fp contract(off)
    const uint32_t px = blockIdx.x * kSimThreads + threadIdx.x, n_px = H * W;
    if (px >= n_px) return;
    const uint32_t j = px / W, i = px - j * W;
    const float dx = ((float)i - cx) / fx;
    const float dy = ((float)j - cy) / fy;
    const size_t at = (size_t)blockIdx.y * n_px + px;
    dist[at] = depth[at] * sim_ray_norm(dx, dy);
}

// Measurement aid (tools/time_sim.py): k_cull_atomic_probe on 8-byte cells -- `iters` 64-bit integer atomicMin per lane at hashed cells of
// buf [n_cells]; the value falls with the iteration.
__global__ __launch_bounds__(kSimThreads) void k_sim_atomic_probe(uint32_t n_cells, uint32_t iters, unsigned long long* __restrict__ buf) {
    const uint64_t lane = (uint64_t)blockIdx.x * kSimThreads + threadIdx.x;
#pragma unroll 1
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t idx = (uint32_t)(splitmix64(lane * 0x100000000ull + it) % n_cells);
        atomicMin(buf + idx, ((unsigned long long)(0x7F000000u - it) << 32) | (uint32_t)lane);
    }
}

}  // namespace naruto
