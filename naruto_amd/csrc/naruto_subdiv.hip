// Mesh subdivision on the device: trimesh.remesh.subdivide_to_size, the step the evaluation protocol's cull_mesh.py runs before it decides,
// per vertex, what the cameras saw (scripts/evaluation/eval_replica.sh:55-72).  trimesh is third-party code outside the reference tree, so
// this is PARITY UNPINNED like the cull itself: the contract is restated in naruto_amd/remesh.py from the published algorithm and pinned by
// the numpy restatement tests/subdivide_spec.py, which every kernel here equals bit for bit.
//
// One generation (the host drives it: naruto_amd/remesh.py; the two prefix sums between the stages are torch.cumsum)
//   k_subdiv_mark     one thread per face: flag[f] = 1 iff one of its edges is longer than max_edge
//   k_subdiv_insert   one thread per face, three edges of a long face: the undirected key (lo << 32) | hi goes into an open-addressing
//                     table (at most half full) with a 64-bit compare-and-swap, and the cell's ordinal word takes the integer minimum of
//                     the slot ordinals 3 * rank + slot that carry the key.  A minimum does not depend on the order of arrival, so the
//                     owner of every key is fixed by the mesh alone.  Where a key landed depends on the arrival order, and nothing that
//                     leaves the workspace depends on where a key landed.  The probe loop is bounded by the table size; a key that finds no
//                     cell sets the error word and the lane goes on: nothing spins.
//   k_subdiv_own      one thread per slot: own[s] = 1 iff s is the lowest ordinal of its key.  The inclusive prefix sum of own numbers the
//                     midpoints in order of first appearance in the face-major edge list (v0v1), (v1v2), (v2v0).
//   k_subdiv_emit     one thread per face.  A short face goes unchanged to row f - (long faces before f).  A long face of rank r writes the
//                     midpoints it owns to row V + (midpoint number) and its four children (v0,m0,m2) (m0,v1,m1) (m2,m1,v2) (m0,m1,m2) to
//                     rows n_short + 4 r: 48 contiguous bytes per lane, contiguous over the wave's long faces.
//
// Arithmetic, in the vertices' own type (float32 or float64), no contraction:
//   long      ((dx*dx + dy*dy) + dz*dz) > max_edge*max_edge, d = v[b] - v[a], max_edge converted to the type once; strict; NaN is false
//   midpoint  (v[lo] + v[hi]) * 0.5 per axis, lo < hi the edge's vertex indices (so both faces of an edge would form the same bits)
//   colour    (c[lo] + c[hi] + 1) >> 1 per RGBA8 channel

#include "naruto_common.h"

namespace naruto {

constexpr int kSubdivThreads = 256;
constexpr unsigned long long kSubdivEmptyKey = ~0ull;                    // lo < 2^31: no key has the top bit set
constexpr uint32_t kSubdivNone = 0xFFFFFFFFu;
constexpr uint32_t kSubdivErrTableFull = 1u, kSubdivErrInconsistent = 2u;

template <typename T>
__device__ __forceinline__ bool subdiv_edge_long(const T* __restrict__ v, uint32_t a, uint32_t b, T limit2) {
#pragma clang fp contract(off)
    const T dx = v[(size_t)b * 3u] - v[(size_t)a * 3u], dy = v[(size_t)b * 3u + 1u] - v[(size_t)a * 3u + 1u], dz = v[(size_t)b * 3u + 2u] - v[(size_t)a * 3u + 2u];
    return ((dx * dx + dy * dy) + dz * dz) > limit2;
}

template <typename T>
__global__ __launch_bounds__(kSubdivThreads) void k_subdiv_mark(uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces, const T* __restrict__ vertices,
                                                                T limit2, uint8_t* __restrict__ flags) {
    const uint32_t f = blockIdx.x * kSubdivThreads + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t i0 = (uint32_t)faces[(size_t)f * 3u], i1 = (uint32_t)faces[(size_t)f * 3u + 1u], i2 = (uint32_t)faces[(size_t)f * 3u + 2u];
    bool is_long = false;
    if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices)
        is_long = subdiv_edge_long(vertices, i0, i1, limit2) || subdiv_edge_long(vertices, i1, i2, limit2) || subdiv_edge_long(vertices, i2, i0, limit2);
    flags[f] = is_long ? 1 : 0;
}

__device__ __forceinline__ unsigned long long subdiv_key(uint32_t a, uint32_t b) {
    return ((unsigned long long)min(a, b) << 32) | (unsigned long long)max(a, b);
}

// rank: INCLUSIVE int32 prefix sum of flags.  pos [3 n_long]: the table cell of every slot (kSubdivNone where none was found).
__global__ __launch_bounds__(kSubdivThreads) void k_subdiv_insert(uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces, const uint8_t* __restrict__ flags,
                                                                  const int32_t* __restrict__ rank, uint32_t n_long, uint32_t table_slots,
                                                                  unsigned long long* __restrict__ keys, uint32_t* __restrict__ ord, uint32_t* __restrict__ pos,
                                                                  uint32_t* __restrict__ err) {
    const uint32_t f = blockIdx.x * kSubdivThreads + threadIdx.x;
    if (f >= n_faces || flags[f] == 0) return;
    const uint32_t r = (uint32_t)(rank[f] - 1);
    const uint32_t i[3] = {(uint32_t)faces[(size_t)f * 3u], (uint32_t)faces[(size_t)f * 3u + 1u], (uint32_t)faces[(size_t)f * 3u + 2u]};
    if (r >= n_long || i[0] >= n_vertices || i[1] >= n_vertices || i[2] >= n_vertices) { atomicOr(err, kSubdivErrInconsistent); return; }
#pragma unroll 1
    for (uint32_t k = 0; k < 3u; ++k) {
        const unsigned long long key = subdiv_key(i[k], i[k == 2u ? 0u : k + 1u]);
        const uint32_t s = 3u * r + k;
        uint32_t cell = (uint32_t)(((splitmix64(key) >> 32) * (unsigned long long)table_slots) >> 32);          // < table_slots
        uint32_t found = kSubdivNone;
#pragma unroll 1
        for (uint32_t probe = 0; probe < table_slots; ++probe) {                                                 // bounded: never spins
            unsigned long long seen = keys[cell];
            if (seen == kSubdivEmptyKey) seen = atomicCAS(keys + cell, kSubdivEmptyKey, key);
            if (seen == kSubdivEmptyKey || seen == key) { found = cell; break; }
            cell = cell + 1u == table_slots ? 0u : cell + 1u;
        }
        if (found != kSubdivNone) atomicMin(ord + found, s);
        else atomicOr(err, kSubdivErrTableFull);
        pos[s] = found;
    }
}

__global__ __launch_bounds__(kSubdivThreads) void k_subdiv_own(uint32_t n_slots, uint32_t table_slots, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ ord,
                                                               uint8_t* __restrict__ own) {
    const uint32_t s = blockIdx.x * kSubdivThreads + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t p = pos[s];
    own[s] = (p < table_slots && ord[p] == s) ? 1 : 0;
}

// vertices [V + n_mid, 3] and colors [V + n_mid] (RGBA8 words, optional): rows below V are read, rows from V on are written (no
// __restrict__: one array).  mid_rank: INCLUSIVE int32 prefix sum of own.  out_faces [n_faces + 3 n_long, 3].
template <typename T>
__global__ __launch_bounds__(kSubdivThreads) void k_subdiv_emit(uint32_t n_faces, uint32_t n_vertices, const int32_t* __restrict__ faces, const uint8_t* __restrict__ flags,
                                                                const int32_t* __restrict__ rank, uint32_t n_long, uint32_t table_slots, const uint32_t* __restrict__ pos,
                                                                const uint32_t* __restrict__ ord, const int32_t* __restrict__ mid_rank, uint32_t n_mid, T* vertices,
                                                                uint32_t* colors, int32_t* __restrict__ out_faces, uint32_t* __restrict__ err) {
#pragma clang fp contract(off)
    const uint32_t f = blockIdx.x * kSubdivThreads + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t n_short = n_faces - n_long, before = (uint32_t)rank[f];         // long faces up to and including f
    const int32_t i0 = faces[(size_t)f * 3u], i1 = faces[(size_t)f * 3u + 1u], i2 = faces[(size_t)f * 3u + 2u];
    if (flags[f] == 0) {
        if (before > n_long || f - before >= n_short) { atomicOr(err, kSubdivErrInconsistent); return; }
        int32_t* o = out_faces + (size_t)(f - before) * 3u;
        o[0] = i0; o[1] = i1; o[2] = i2;
        return;
    }
    const uint32_t r = before - 1u;
    const uint32_t i[3] = {(uint32_t)i0, (uint32_t)i1, (uint32_t)i2};
    if (r >= n_long || i[0] >= n_vertices || i[1] >= n_vertices || i[2] >= n_vertices) { atomicOr(err, kSubdivErrInconsistent); return; }
    int32_t m[3];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t s = 3u * r + k, p = pos[s];
        const uint32_t owner = p < table_slots ? ord[p] : kSubdivNone;
        const uint32_t number = owner < 3u * n_long ? (uint32_t)mid_rank[owner] - 1u : kSubdivNone;
        if (number >= n_mid) { atomicOr(err, kSubdivErrInconsistent); m[k] = i0; continue; }
        const uint32_t row = n_vertices + number;
        m[k] = (int32_t)row;
        if (owner != s) continue;
        const uint32_t a = i[k], b = i[k == 2u ? 0u : k + 1u], lo = min(a, b), hi = max(a, b);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) vertices[(size_t)row * 3u + c] = (vertices[(size_t)lo * 3u + c] + vertices[(size_t)hi * 3u + c]) * (T)0.5;
        if (colors != nullptr) {
            const uint32_t ca = colors[lo], cb = colors[hi];
            uint32_t w = 0;
#pragma unroll
            for (uint32_t c = 0; c < 32u; c += 8u) w |= ((((ca >> c) & 0xFFu) + ((cb >> c) & 0xFFu) + 1u) >> 1) << c;
            colors[row] = w;
        }
    }
    int32_t* o = out_faces + ((size_t)n_short + 4u * (size_t)r) * 3u;
    o[0] = i0;   o[1] = m[0];  o[2] = m[2];
    o[3] = m[0]; o[4] = i1;    o[5] = m[1];
    o[6] = m[2]; o[7] = m[1];  o[8] = i2;
    o[9] = m[0]; o[10] = m[1]; o[11] = m[2];
}

}  // namespace naruto
