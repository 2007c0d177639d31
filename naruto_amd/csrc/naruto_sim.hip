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
