// Mesh culling on the device (the step between save_mesh and eval_recon.py in the reference's evaluation protocol,
// scripts/evaluation/eval_replica.sh:55-72 -> third_parties/neural_slam_eval/cull_mesh.py --remove_occlusion): one depth render of an
// occluder mesh per estimated camera pose, a per-vertex frustum / occlusion test against it, and the compaction of what was seen.
// cull_mesh.py is not part of the reference tree (an empty submodule; it needs trimesh and off-screen OpenGL through pyrender), so this is
// PARITY UNPINNED: the contract is restated in naruto_amd/culling.py from the published strategy (Co-SLAM / GO-Surf culling) and pinned by
// the numpy float32 restatement tests/cull_spec.py, which every kernel here equals bit for bit.
//
// Kernels
//   k_cull_transform     one thread per (pose, vertex): camera space once per pose, into workspace (float4: x, y, z, 0; zc = -z)
//   k_cull_raster_small  one lane per (pose, triangle): the candidate pixel box; a box of up to `threshold` pixels is walked by the lane,
//                        a larger one goes onto a list with its number of 2048-pixel chunks (ONE 64-bit atomic per wave hands out list
//                        slots and chunk ranges together, so the slots are in the order of their chunk ranges)
//   k_cull_raster_large  one workgroup per 2048-pixel chunk of a listed box (grid-stride over the chunks: their number is on the device);
//                        binary search chunk -> list slot; every lane tests 8 pixels, whatever the box: a full-screen box at
//                        1200 x 680 is 399 chunks spread over the device, not 816 000 pixels in one lane
//   k_cull_observed      one thread per vertex, the chunk's poses in turn: in frustum [and not occluded] -> mask[v] = 1
//   k_cull_faces         one thread per face: kept iff (any vertex inside the bounds) and (any vertex observed); marks its vertices
//   k_cull_compact_faces / k_cull_compact_vertices   kept rows to their prefix-sum positions, original order, faces re-indexed
//
// Arithmetic (fp32, this order, no contraction; hipcc's default fp32 divide is correctly rounded):
//   camera space   q = p - t,  x_k = (q0*R0k + q1*R1k) + q2*R2k,  zc = -x_2                      (R, t from the row-major c2w)
//   pixel ray      d = (dx, dy, -1),  dx = (i - cx)/fx,  dy = -((j - cy)/fy)
//   edge value     e(p,q) = (dx*n0 + dy*n1) - n2,  n = p x q,  n0 = p1*q2 - p2*q1, n1 = p2*q0 - p0*q2, n2 = p0*q1 - p1*q0
//   covered        e(a,b), e(b,c), e(c,a) all >= 0 or all <= 0, and not all zero       (double sided: winding never matters)
//   depth          n = (b-a) x (c-a), den = (dx*n0 + dy*n1) - n2, num = (a0*n0 + a1*n1) + a2*n2, t = num/den;
//                  a hit iff covered, den != 0 and near < t < far;  D[j,i] = min t
//   This is homogeneous rasterisation: the edge planes pass through the eye, so a triangle with vertices behind the camera needs no clipping.
//   candidate box  all three zc > near: u = cx + fx*(x/zc), v = cy - fy*(y/zc), [ceil(min) - 1, floor(max) + 1] clamped to the image;
//                  none: no candidates; otherwise the whole image
//   vertex test    u = (fx*x)/zc + cx, v = cy - (fy*y)/zc, i = floor(u + 0.5), j = floor(v + 0.5);
//                  in frustum iff zc > 0, 0 <= i < W, 0 <= j < H; observed iff in frustum [and zc < D[j,i] + eps]
// The minimum is an integer atomicMin on the depth's bit pattern: depths are positive, so the integer order is the float order and the
// result does not depend on the order of arrival -- bitwise reproducible.  A pixel nothing covers keeps +inf.

#include "naruto_common.h"

namespace naruto {

constexpr int kCullThreads = 256;
constexpr uint32_t kCullLargePer = 8;                                    // pixels per lane of one large-route chunk
constexpr uint32_t kCullChunk = kCullThreads * kCullLargePer;            // 2048 pixels per chunk
constexpr uint32_t kCullInfBits = 0x7F800000u;
constexpr int kCullSlotShift = 36;                                       // list counter: slots in the top 28 bits, chunks in the low 36
constexpr unsigned long long kCullChunkMask = (1ull << kCullSlotShift) - 1ull;

struct CullCam { uint32_t H, W; float fx, fy, cx, cy, near_, far_; };
struct CullBox { int x0, y0, x1, y1; };                                  // inclusive
struct CullTri { float nab[3], nbc[3], nca[3], n[3], num; };

__device__ __forceinline__ void cull_cross(const float* p, const float* q, float* n) {
#pragma clang fp contract(off)
    n[0] = p[1] * q[2] - p[2] * q[1];
    n[1] = p[2] * q[0] - p[0] * q[2];
    n[2] = p[0] * q[1] - p[1] * q[0];
}

__device__ __forceinline__ float4 cull_to_camera(const float* __restrict__ c2w, float px, float py, float pz) {
#pragma clang fp contract(off)
    const float q0 = px - c2w[3], q1 = py - c2w[7], q2 = pz - c2w[11];
    float4 x;
    x.x = (q0 * c2w[0] + q1 * c2w[4]) + q2 * c2w[8];
    x.y = (q0 * c2w[1] + q1 * c2w[5]) + q2 * c2w[9];
    x.z = (q0 * c2w[2] + q1 * c2w[6]) + q2 * c2w[10];
    x.w = 0.0f;
    return x;
}

// false: no candidate pixel
__device__ __forceinline__ bool cull_box(const CullCam& c, const float4 a, const float4 b, const float4 d, CullBox& box) {
#pragma clang fp contract(off)
    const float za = -a.z, zb = -b.z, zd = -d.z;
    const bool fa = za > c.near_, fb = zb > c.near_, fd = zd > c.near_;
    if (!fa && !fb && !fd) return false;
    if (!(fa && fb && fd)) {
        box.x0 = 0; box.y0 = 0; box.x1 = (int)c.W - 1; box.y1 = (int)c.H - 1;
        return true;
    }
    const float ua = c.cx + c.fx * (a.x / za), ub = c.cx + c.fx * (b.x / zb), ud = c.cx + c.fx * (d.x / zd);
    const float va = c.cy - c.fy * (a.y / za), vb = c.cy - c.fy * (b.y / zb), vd = c.cy - c.fy * (d.y / zd);
    const float x0 = fmaxf(ceilf(fminf(fminf(ua, ub), ud)) - 1.0f, 0.0f), x1 = fminf(floorf(fmaxf(fmaxf(ua, ub), ud)) + 1.0f, (float)(c.W - 1u));
    const float y0 = fmaxf(ceilf(fminf(fminf(va, vb), vd)) - 1.0f, 0.0f), y1 = fminf(floorf(fmaxf(fmaxf(va, vb), vd)) + 1.0f, (float)(c.H - 1u));
    if (!(x0 <= x1 && y0 <= y1)) return false;
    box.x0 = (int)x0; box.x1 = (int)x1; box.y0 = (int)y0; box.y1 = (int)y1;        // all within [0, W-1] x [0, H-1]
    return true;
}

__device__ __forceinline__ void cull_setup(const float4 a4, const float4 b4, const float4 c4, CullTri& t) {
#pragma clang fp contract(off)
    const float a[3] = {a4.x, a4.y, a4.z}, b[3] = {b4.x, b4.y, b4.z}, c[3] = {c4.x, c4.y, c4.z};
    cull_cross(a, b, t.nab);
    cull_cross(b, c, t.nbc);
    cull_cross(c, a, t.nca);
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cull_cross(e1, e2, t.n);
    t.num = (a[0] * t.n[0] + a[1] * t.n[1]) + a[2] * t.n[2];
}

// pixel (i, j) of one pose's depth plane (H*W cells).  Cell uint32_t: the depth's bit pattern (the cull).  Cell unsigned long long: depth
// bits in the high word, the face index in the low one (the simulator, naruto_sim.hip): the minimum is the nearest depth and, among the
// faces whose depth equals it in every bit, the lowest index -- whatever the order of arrival.
template <typename Cell>
__device__ __forceinline__ void cull_pixel(const CullCam& c, const CullTri& t, int i, int j, Cell* __restrict__ plane, uint32_t face) {
#pragma clang fp contract(off)
    const float dx = ((float)i - c.cx) / c.fx;
    const float dy = -(((float)j - c.cy) / c.fy);
    const float e0 = (dx * t.nab[0] + dy * t.nab[1]) - t.nab[2];
    const float e1 = (dx * t.nbc[0] + dy * t.nbc[1]) - t.nbc[2];
    const float e2 = (dx * t.nca[0] + dy * t.nca[1]) - t.nca[2];
    const bool pos = e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f, neg = e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f;
    const bool zero = e0 == 0.0f && e1 == 0.0f && e2 == 0.0f;
    if (!(pos || neg) || zero) return;
    const float den = (dx * t.n[0] + dy * t.n[1]) - t.n[2];
    if (den == 0.0f) return;
    const float depth = t.num / den;
    if (!(depth > c.near_ && depth < c.far_)) return;
    Cell key = (Cell)__float_as_uint(depth);
    if constexpr (sizeof(Cell) == 8) key = (key << 32) | face;
    Cell* cell = plane + (size_t)j * c.W + (uint32_t)i;
    if (key < *cell) atomicMin(cell, key);                  // (a stale read is only ever too large: the atomic decides)
}

__device__ __forceinline__ bool cull_load_triangle(const int32_t* __restrict__ faces, uint32_t f, uint32_t n_vertices, const float4* __restrict__ camv,
                                                   float4& a, float4& b, float4& c) {
    const uint32_t i0 = (uint32_t)faces[(size_t)f * 3u], i1 = (uint32_t)faces[(size_t)f * 3u + 1u], i2 = (uint32_t)faces[(size_t)f * 3u + 2u];
    if (i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) return false;
    a = camv[i0]; b = camv[i1]; c = camv[i2];
    return true;
}

// grid (vertices / 256, poses): camv [B][V]
__global__ __launch_bounds__(kCullThreads) void k_cull_transform(uint32_t n_vertices, const float* __restrict__ vertices, const float* __restrict__ poses,
                                                                  float4* __restrict__ camv) {
    const uint32_t v = blockIdx.x * kCullThreads + threadIdx.x, pose = blockIdx.y;
    if (v >= n_vertices) return;
    const float* p = vertices + (size_t)v * 3u;
    camv[(size_t)pose * n_vertices + v] = cull_to_camera(poses + (size_t)pose * 16u, p[0], p[1], p[2]);
}

// grid (faces / 256, poses).  No lane leaves before the list allocation: a wave's large boxes take their slots and chunk ranges with ONE
// atomic (inclusive scans of the flags and the chunk counts over the wave; lane order = slot order, so the slots stay sorted by chunk range).
template <typename Cell>
__global__ __launch_bounds__(kCullThreads) void k_cull_raster_small(CullCam cam, uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                                     const uint8_t* __restrict__ face_mask, const float4* __restrict__ camv, uint32_t threshold,
                                                                     Cell* __restrict__ depth, unsigned long long* __restrict__ counter,
                                                                     uint32_t* __restrict__ ent_id, unsigned long long* __restrict__ ent_start, uint32_t cap) {
    const uint32_t f = blockIdx.x * kCullThreads + threadIdx.x, pose = blockIdx.y;
    float4 a, b, c;
    CullBox box;
    bool valid = f < n_faces && (face_mask == nullptr || face_mask[f] != 0);
    valid = valid && cull_load_triangle(faces, f, n_vertices, camv + (size_t)pose * n_vertices, a, b, c);
    valid = valid && cull_box(cam, a, b, c, box);
    const uint32_t px = valid ? (uint32_t)(box.x1 - box.x0 + 1) * (uint32_t)(box.y1 - box.y0 + 1) : 0u;
    const bool large = valid && px > threshold;
    if (__ballot(large) != 0ull) {                                          // (uniform over the wave)
        const int lane = threadIdx.x & 63;
        const uint32_t chunks = large ? (px + kCullChunk - 1u) / kCullChunk : 0u;
        uint32_t slots_incl = large ? 1u : 0u, chunks_incl = chunks;        // a wave's chunks: <= 64 * 2^19
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t us = (uint32_t)__shfl_up((int)slots_incl, s, 64), uc = (uint32_t)__shfl_up((int)chunks_incl, s, 64);
            if (lane >= s) { slots_incl += us; chunks_incl += uc; }
        }
        unsigned long long old = 0ull;
        if (lane == 63) old = atomicAdd(counter, ((unsigned long long)slots_incl << kCullSlotShift) | (unsigned long long)chunks_incl);
        const uint32_t old_lo = (uint32_t)__shfl((int)(uint32_t)old, 63, 64), old_hi = (uint32_t)__shfl((int)(uint32_t)(old >> 32), 63, 64);
        old = ((unsigned long long)old_hi << 32) | old_lo;
        if (large) {
            const unsigned long long slot = (old >> kCullSlotShift) + (slots_incl - 1u);
            if (slot < cap) {
                ent_id[slot] = pose * n_faces + f;
                ent_start[slot] = (old & kCullChunkMask) + (chunks_incl - chunks);
            }
        }
    }
    if (!valid || large) return;
    CullTri t;
    cull_setup(a, b, c, t);
    Cell* plane = depth + (size_t)pose * cam.H * cam.W;
#pragma unroll 1
    for (int j = box.y0; j <= box.y1; ++j)
#pragma unroll 1
        for (int i = box.x0; i <= box.x1; ++i) cull_pixel(cam, t, i, j, plane, f);
}

template <typename Cell>
__global__ __launch_bounds__(kCullThreads) void k_cull_raster_large(CullCam cam, uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                                     const float4* __restrict__ camv, Cell* __restrict__ depth,
                                                                     const unsigned long long* __restrict__ counter, const uint32_t* __restrict__ ent_id,
                                                                     const unsigned long long* __restrict__ ent_start, uint32_t cap) {
    const unsigned long long word = *counter;
    const unsigned long long total = word & kCullChunkMask;
    const uint32_t n_ent = (uint32_t)min(word >> kCullSlotShift, (unsigned long long)cap);
    if (n_ent == 0) return;
#pragma unroll 1
    for (unsigned long long chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
        uint32_t lo = 0, hi = n_ent - 1u;                   // the last slot whose first chunk is <= chunk (slot 0 starts at chunk 0)
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
            if (ent_start[mid] <= chunk) lo = mid; else hi = mid - 1u;
        }
        const uint32_t id = ent_id[lo], pose = id / n_faces, f = id - pose * n_faces;
        const uint32_t first = (uint32_t)(chunk - ent_start[lo]) * kCullChunk;
        float4 a, b, c;
        if (f >= n_faces || !cull_load_triangle(faces, f, n_vertices, camv + (size_t)pose * n_vertices, a, b, c)) continue;
        CullBox box;
        if (!cull_box(cam, a, b, c, box)) continue;
        const uint32_t bw = (uint32_t)(box.x1 - box.x0 + 1), bh = (uint32_t)(box.y1 - box.y0 + 1), px = bw * bh;
        CullTri t;
        cull_setup(a, b, c, t);
        Cell* plane = depth + (size_t)pose * cam.H * cam.W;
#pragma unroll 1
        for (uint32_t r = 0; r < kCullLargePer; ++r) {
            const uint32_t k = first + r * kCullThreads + threadIdx.x;
            if (k < px) {
                const uint32_t row = k / bw;
                cull_pixel(cam, t, box.x0 + (int)(k - row * bw), box.y0 + (int)row, plane, f);
            }
        }
    }
}

__global__ __launch_bounds__(kCullThreads) void k_cull_observed(CullCam cam, uint32_t n_vertices, const float* __restrict__ vertices, uint32_t n_poses,
                                                                const float* __restrict__ poses, const uint32_t* __restrict__ depth, float eps,
                                                                uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
    const uint32_t v = blockIdx.x * kCullThreads + threadIdx.x;
    if (v >= n_vertices) return;
    const float px = vertices[(size_t)v * 3u], py = vertices[(size_t)v * 3u + 1u], pz = vertices[(size_t)v * 3u + 2u];
    bool seen = false;
#pragma unroll 1
    for (uint32_t pose = 0; pose < n_poses && !seen; ++pose) {
        const float4 x = cull_to_camera(poses + (size_t)pose * 16u, px, py, pz);
        const float zc = -x.z;
        if (!(zc > 0.0f)) continue;
        const float u = (cam.fx * x.x) / zc + cam.cx, w = cam.cy - (cam.fy * x.y) / zc;
        const float fi = floorf(u + 0.5f), fj = floorf(w + 0.5f);
        if (!(fi >= 0.0f && fi < (float)cam.W && fj >= 0.0f && fj < (float)cam.H)) continue;
        if (depth == nullptr) { seen = true; break; }
        const float d = __uint_as_float(depth[((size_t)pose * cam.H + (uint32_t)fj) * cam.W + (uint32_t)fi]);
        seen = zc < d + eps;
    }
    if (seen) mask[v] = 1;
}

__global__ __launch_bounds__(kCullThreads) void k_cull_faces(uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                             const uint8_t* __restrict__ observed, const uint8_t* __restrict__ inside,
                                                             uint8_t* __restrict__ face_keep, uint8_t* __restrict__ vertex_used) {
    const uint32_t f = blockIdx.x * kCullThreads + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t i0 = (uint32_t)faces[(size_t)f * 3u], i1 = (uint32_t)faces[(size_t)f * 3u + 1u], i2 = (uint32_t)faces[(size_t)f * 3u + 2u];
    bool keep = i0 < n_vertices && i1 < n_vertices && i2 < n_vertices;
    if (keep && inside != nullptr) keep = inside[i0] != 0 || inside[i1] != 0 || inside[i2] != 0;
    if (keep && observed != nullptr) keep = observed[i0] != 0 || observed[i1] != 0 || observed[i2] != 0;
    face_keep[f] = keep ? 1 : 0;
    if (keep && vertex_used != nullptr) { vertex_used[i0] = 1; vertex_used[i1] = 1; vertex_used[i2] = 1; }
}

// positions are INCLUSIVE prefix sums of the flags: row r of the kept rows is pos - 1
__global__ __launch_bounds__(kCullThreads) void k_cull_compact_faces(uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces,
                                                                      const uint8_t* __restrict__ face_keep, const int32_t* __restrict__ face_pos,
                                                                      const int32_t* __restrict__ vertex_pos, uint32_t n_out, int32_t* __restrict__ out) {
    const uint32_t f = blockIdx.x * kCullThreads + threadIdx.x;
    if (f >= n_faces || face_keep[f] == 0) return;
    const uint32_t row = (uint32_t)(face_pos[f] - 1);
    if (row >= n_out) return;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t i = (uint32_t)faces[(size_t)f * 3u + k];
        out[(size_t)row * 3u + k] = i < n_vertices ? vertex_pos[i] - 1 : 0;
    }
}

// a vertex row is `words` 32-bit words (3: float32 xyz, 6: float64 xyz); colours are one word (RGBA8)
__global__ __launch_bounds__(kCullThreads) void k_cull_compact_vertices(uint32_t n_vertices, const uint8_t* __restrict__ vertex_used, const int32_t* __restrict__ vertex_pos,
                                                                         const uint32_t* __restrict__ vertices, uint32_t words, const uint32_t* __restrict__ colors,
                                                                         uint32_t n_out, uint32_t* __restrict__ out_vertices, uint32_t* __restrict__ out_colors) {
    const uint32_t v = blockIdx.x * kCullThreads + threadIdx.x;
    if (v >= n_vertices || vertex_used[v] == 0) return;
    const uint32_t row = (uint32_t)(vertex_pos[v] - 1);
    if (row >= n_out) return;
    for (uint32_t k = 0; k < words; ++k) out_vertices[(size_t)row * words + k] = vertices[(size_t)v * words + k];
    if (colors != nullptr) out_colors[row] = colors[v];
}

// Measurement aid (tools/time_cull.py): `iters` integer atomicMin per lane at hashed word addresses of buf [n_words] -- the access pattern of
// the rasteriser's depth minimum without the rasteriser.  The value falls with the iteration, so an atomic is never a no-op by construction.
__global__ __launch_bounds__(kCullThreads) void k_cull_atomic_probe(uint32_t n_words, uint32_t iters, uint32_t* __restrict__ buf) {
    const uint64_t lane = (uint64_t)blockIdx.x * kCullThreads + threadIdx.x;
#pragma unroll 1
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t idx = (uint32_t)(splitmix64(lane * 0x100000000ull + it) % n_words);
        atomicMin(buf + idx, 0x7F000000u - it);
    }
}

}  // namespace naruto
