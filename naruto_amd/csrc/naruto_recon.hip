// Reconstruction metrics on the device (Accuracy / Completion / Completion ratio of the reference's evaluation protocol,
// README "Evaluation", scripts/evaluation/eval_replica.sh:56-83 -> src/evaluation/eval_recon.py): the chain
//   mesh -> area-weighted surface samples -> nearest-neighbour distances (both ways) -> mean / share below a threshold.
// The reference hands this to third-party code (neural_slam_eval's calc_3d_mesh_metric: trimesh.sample.sample_surface + two
// scipy cKDTree queries on the host) that is not part of its tree; the contract is restated in naruto_amd/evaluation.py from
// the published algorithms.  What CAN be pinned is: k_nn_grid and k_nn_scan return cKDTree.query's distances bit for bit.
//
// Kernels
//   k_face_areas      one thread per face: the triangle's area in fp64
//   k_surface_sample  one thread per sample: face by binary search in the cumulative areas, point by reflected barycentrics
//   k_grid_count / k_grid_scan_local / k_grid_scan_totals / k_grid_scan_add / k_grid_fill
//                     a uniform grid over the target cloud: the points counting-sorted by cell (integer atomics; the order
//                     INSIDE a cell is whatever the atomics give and nothing depends on it: candidates are compared by
//                     (squared distance, original index))
//   k_nn_grid         one thread per query: rings of cells around the query's cell until the bound below closes
//   k_nn_scan         the same answer by brute force, target tiles through LDS; serves small targets and the queries whose
//                     ring search did not close inside its budget (a compacted list)
//   k_dist_partial / k_dist_finish   mean and count-below-threshold in fp64, fixed order, no float atomics
//
// Distance arithmetic (both search kernels): coordinates are float32 in memory and promoted to fp64;
//   d2 = (dx*dx + dy*dy) + dz*dz   -- no contraction, this association -- minimum on d2, one sqrt at the end.
// This is what cKDTree.query(k=1) returns for float32 data (it widens to fp64 and sums the squares x, y, z in order).
//
// Why a ring search may stop (the argument of the RRT's cell lists, DESIGN.md 7b, with the out-of-box case):
//   cell_a(x) = clamp(floor((x - lo_a) * inv_h), 0, n_a - 1) is a NONDECREASING function of x in fp64 (a subtraction of a constant,
//   a multiplication by a positive constant, floor and clamp are all monotone under rounding).  Let b_k be the least x with
//   cell_a(x) >= k; in exact arithmetic b_k = lo_a + k*h, in fp64 it is off by a few ulp of the box extent.  A query q lies in
//   [b_c, b_{c+1}) of its cell c on every axis -- or, where it is outside the box and its cell was clamped, further out on the far
//   side of that interval (q < b_1 for c = 0, q >= b_{n-1} for c = n-1), which only makes the following larger.  After ring R every cell with
//   Chebyshev distance <= R from the query's cell has been seen, so an unseen point p sits in a cell with |c_p - c| >= R + 1 on some
//   axis a, hence |p_a - q_a| > b_{c+R+1} - b_{c+1} >= R*h - slack, where slack (2^-40 of the largest box extent) is far above the
//   rounding of the b_k.  So a best distance < R*h - slack is final, ties included (the unseen points are strictly farther).
//   The search is also final once the rings cover the whole grid.  A query far outside the box would need about distance / h rings:
//   after `ring_budget` rings it goes onto a list that k_nn_scan serves, so it costs a scan, not a million empty cells.

#include "naruto_common.h"

namespace naruto {

constexpr int kReconThreads = 256;
constexpr uint32_t kGridScanPer = 8;                                     // cells per thread of k_grid_scan_local
constexpr uint32_t kGridScanItems = kReconThreads * kGridScanPer;        // cells per scan block
constexpr int kScanQ = 4;                                                // queries per lane of k_nn_scan
constexpr uint32_t kScanTile = 1024;                                     // targets per LDS tile (16 KB)
constexpr uint32_t kDistPer = 8;                                         // distances per thread of k_dist_partial
constexpr int32_t kNoIndex = 0x7FFFFFFF;

struct NnGrid {
    uint32_t nx, ny, nz, n;          // cells per axis (x fastest), points
    double lo[3];                    // the box's lower corner
    double inv_h, h, slack;
    const uint32_t* start;           // [cells + 1]
    const float4* pts;               // [n] in cell order: x, y, z, original index (bits)
};

// uniform in [0,1) from the top 53 bits of the keyed stream: key = splitmix64(seed), number (sample, draw) = splitmix64(key + 3*sample + draw)
__device__ __forceinline__ double recon_uniform(uint64_t key, uint64_t sample, uint32_t draw) {
    return (double)(splitmix64(key + 3ull * sample + draw) >> 11) * 0x1p-53;
}

template <bool kF64>
__device__ __forceinline__ void load_vertex(const void* __restrict__ v, uint32_t i, double& x, double& y, double& z) {
    if (kF64) {
        const double* p = reinterpret_cast<const double*>(v) + (size_t)i * 3u;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const float* p = reinterpret_cast<const float*>(v) + (size_t)i * 3u;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
}

// area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = e1 x e2 with e1 = v1 - v0, e2 = v2 - v0 and
// cx = e1y*e2z - e1z*e2y, cy = e1z*e2x - e1x*e2z, cz = e1x*e2y - e1y*e2x: every product rounded, then the difference (no contraction).
// A face with an index outside [0, n_vertices) gets area 0, so it is never drawn and nothing is read out of bounds.
template <bool kF64>
__global__ __launch_bounds__(kReconThreads) void k_face_areas(uint32_t n_faces, uint32_t n_vertices, const void* __restrict__ vertices,
                                                               const int32_t* __restrict__ faces, double* __restrict__ areas) {
#pragma clang fp contract(off)
    const uint32_t f = blockIdx.x * kReconThreads + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t i0 = (uint32_t)faces[(size_t)f * 3u], i1 = (uint32_t)faces[(size_t)f * 3u + 1u], i2 = (uint32_t)faces[(size_t)f * 3u + 2u];
    double area = 0.0;
    if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices) {
        double ax, ay, az, bx, by, bz, cx, cy, cz;
        load_vertex<kF64>(vertices, i0, ax, ay, az);
        load_vertex<kF64>(vertices, i1, bx, by, bz);
        load_vertex<kF64>(vertices, i2, cx, cy, cz);
        const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    }
    areas[f] = area;
}

// sample s: u0, u1, u2 = draws 0, 1, 2; face = first index with cum[face] >= u0 * cum[F-1] (searchsorted, left side);
// (u1, u2) -> (|u1 - 1|, |u2 - 1|) when u1 + u2 > 1; point = v0 + (e1*u1 + e2*u2) in fp64 without contraction, stored as float32.
template <bool kF64>
__global__ __launch_bounds__(kReconThreads) void k_surface_sample(uint32_t n_faces, uint32_t n_vertices, const void* __restrict__ vertices,
                                                                   const int32_t* __restrict__ faces, const double* __restrict__ cum, uint32_t count,
                                                                   uint64_t seed, float* __restrict__ points, int32_t* __restrict__ face_index) {
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * kReconThreads + threadIdx.x;
    if (s >= count) return;
    const uint64_t key = splitmix64(seed);
    const double u0 = recon_uniform(key, s, 0);
    double u1 = recon_uniform(key, s, 1), u2 = recon_uniform(key, s, 2);
    const double t = u0 * cum[n_faces - 1u];
    uint32_t lo = 0, hi = n_faces - 1u;                    // the answer lies in [lo, hi]: t <= cum[F-1] always (u0 < 1)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] < t) lo = mid + 1u; else hi = mid;
    }
    if (u1 + u2 > 1.0) { u1 = fabs(u1 - 1.0); u2 = fabs(u2 - 1.0); }
    const uint32_t i0 = (uint32_t)faces[(size_t)lo * 3u], i1 = (uint32_t)faces[(size_t)lo * 3u + 1u], i2 = (uint32_t)faces[(size_t)lo * 3u + 2u];
    double px = __builtin_nan(""), py = px, pz = px;
    if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices) {
        double ax, ay, az, bx, by, bz, cx, cy, cz;
        load_vertex<kF64>(vertices, i0, ax, ay, az);
        load_vertex<kF64>(vertices, i1, bx, by, bz);
        load_vertex<kF64>(vertices, i2, cx, cy, cz);
        px = ax + ((bx - ax) * u1 + (cx - ax) * u2);
        py = ay + ((by - ay) * u1 + (cy - ay) * u2);
        pz = az + ((bz - az) * u1 + (cz - az) * u2);
    }
    points[(size_t)s * 3u] = (float)px;
    points[(size_t)s * 3u + 1u] = (float)py;
    points[(size_t)s * 3u + 2u] = (float)pz;
    face_index[s] = (int32_t)lo;
}

// ---- the grid -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t grid_axis_cell(double x, double lo, double inv_h, uint32_t n) {
    const double c = floor((x - lo) * inv_h);
    return (uint32_t)fmin(fmax(c, 0.0), (double)(n - 1u));               // (a NaN comes out as cell 0: never out of range)
}
__device__ __forceinline__ uint32_t grid_cell(const NnGrid& g, float x, float y, float z, uint32_t& cx, uint32_t& cy, uint32_t& cz) {
    cx = grid_axis_cell((double)x, g.lo[0], g.inv_h, g.nx);
    cy = grid_axis_cell((double)y, g.lo[1], g.inv_h, g.ny);
    cz = grid_axis_cell((double)z, g.lo[2], g.inv_h, g.nz);
    return (cz * g.ny + cy) * g.nx + cx;
}

__global__ __launch_bounds__(kReconThreads) void k_grid_count(NnGrid g, const float* __restrict__ xyz, uint32_t* __restrict__ cells, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * kReconThreads + threadIdx.x;
    if (i >= g.n) return;
    uint32_t cx, cy, cz;
    const uint32_t c = grid_cell(g, xyz[(size_t)i * 3u], xyz[(size_t)i * 3u + 1u], xyz[(size_t)i * 3u + 2u], cx, cy, cz);
    cells[i] = c;
    atomicAdd(count + c, 1u);
}

// exclusive prefix of the cell counts: inside blocks of kGridScanItems cells, then the blocks' totals (one workgroup), then the add
__global__ __launch_bounds__(kReconThreads) void k_grid_scan_local(uint32_t n_cells, const uint32_t* __restrict__ count, uint32_t* __restrict__ start,
                                                                    uint32_t* __restrict__ block_total) {
    __shared__ uint32_t wave_tot[kReconThreads / 64];
    const uint32_t c0 = blockIdx.x * kGridScanItems + threadIdx.x * kGridScanPer;
    uint32_t cnt[kGridScanPer];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < kGridScanPer; ++t) {
        cnt[t] = c0 + t < n_cells ? count[c0 + t] : 0u;
        mine += cnt[t];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, s, 64);
        if (lane >= s) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    uint32_t run = base + incl - mine;
#pragma unroll
    for (uint32_t t = 0; t < kGridScanPer; ++t) {
        if (c0 + t < n_cells) start[c0 + t] = run;
        run += cnt[t];
    }
    if (threadIdx.x == kReconThreads - 1) block_total[blockIdx.x] = run;
}

__global__ __launch_bounds__(1024) void k_grid_scan_totals(uint32_t n_blocks, uint32_t* __restrict__ block_total) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024u) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t mine = b < n_blocks ? block_total[b] : 0u;
        uint32_t incl = mine;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, s, 64);
            if (lane >= s) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t base = carry_s;
        for (int w = 0; w < wave; ++w) base += wave_tot[w];
        if (b < n_blocks) block_total[b] = base + incl - mine;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = base + incl;
        __syncthreads();
    }
}

// start[c] += its block's base; start[n_cells] = n; the counts go back to zero (they become k_grid_fill's cursors)
__global__ __launch_bounds__(kReconThreads) void k_grid_scan_add(uint32_t n_cells, uint32_t n_points, const uint32_t* __restrict__ block_total,
                                                                  uint32_t* __restrict__ start, uint32_t* __restrict__ count) {
    const uint32_t c = blockIdx.x * kReconThreads + threadIdx.x;
    if (c < n_cells) {
        start[c] += block_total[c / kGridScanItems];
        count[c] = 0u;
    } else if (c == n_cells) {
        start[c] = n_points;
    }
}

__global__ __launch_bounds__(kReconThreads) void k_grid_fill(NnGrid g, const float* __restrict__ xyz, const uint32_t* __restrict__ cells,
                                                              const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor, float4* __restrict__ pts) {
    const uint32_t i = blockIdx.x * kReconThreads + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t c = cells[i];
    const uint32_t pos = start[c] + atomicAdd(cursor + c, 1u);
    if (pos < g.n) pts[pos] = make_float4(xyz[(size_t)i * 3u], xyz[(size_t)i * 3u + 1u], xyz[(size_t)i * 3u + 2u], __int_as_float((int)i));
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------------------
struct NnBest { double d2; int32_t idx; };

__device__ __forceinline__ void nn_consider(NnBest& b, double qx, double qy, double qz, const float4 p) {
#pragma clang fp contract(off)
    const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const int32_t pi = __float_as_int(p.w);
    if (d2 < b.d2 || (d2 == b.d2 && pi < b.idx)) { b.d2 = d2; b.idx = pi; }
}

__device__ __forceinline__ void nn_store(const NnBest& b, uint32_t out, double* __restrict__ dist, int32_t* __restrict__ index) {
    dist[out] = sqrt(b.d2);
    index[out] = b.idx == kNoIndex ? -1 : b.idx;
}

// queries: q3 [nq,3] float32 (result i -> dist[i]) or, when q4 is given, q4 [nq] = x, y, z, original index in the queries' own cell
// order (result -> dist[original index]).  Queries that do not close inside `ring_budget` rings go to fb_list (positions in the query array).
__global__ __launch_bounds__(kReconThreads) void k_nn_grid(NnGrid g, uint32_t nq, const float* __restrict__ q3, const float4* __restrict__ q4, uint32_t ring_budget,
                                                            double* __restrict__ dist, int32_t* __restrict__ index, uint32_t* __restrict__ fb_list,
                                                            uint32_t* __restrict__ fb_count) {
    const uint32_t i = blockIdx.x * kReconThreads + threadIdx.x;
    if (i >= nq) return;
    float fx, fy, fz;
    uint32_t out = i;
    if (q4 != nullptr) {
        const float4 q = q4[i];
        fx = q.x; fy = q.y; fz = q.z; out = (uint32_t)__float_as_int(q.w);
    } else {
        fx = q3[(size_t)i * 3u]; fy = q3[(size_t)i * 3u + 1u]; fz = q3[(size_t)i * 3u + 2u];
    }
    const double qx = (double)fx, qy = (double)fy, qz = (double)fz;
    uint32_t ucx, ucy, ucz;
    grid_cell(g, fx, fy, fz, ucx, ucy, ucz);
    const int cx = (int)ucx, cy = (int)ucy, cz = (int)ucz;
    const int nx = (int)g.nx, ny = (int)g.ny, nz = (int)g.nz;
    NnBest best{__builtin_inf(), kNoIndex};
    bool closed = false;
#pragma unroll 1
    for (int R = 0; R < (int)ring_budget; ++R) {
        const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1), y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1), x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
#pragma unroll 1
        for (int zz = z0; zz <= z1; ++zz) {
#pragma unroll 1
            for (int yy = y0; yy <= y1; ++yy) {
                const uint32_t row = ((uint32_t)zz * g.ny + (uint32_t)yy) * g.nx;
                if (abs(zz - cz) == R || abs(yy - cy) == R) {                       // a face of the shell: the whole x run is one contiguous range
                    const uint32_t e = g.start[row + (uint32_t)x1 + 1u];
                    for (uint32_t p = g.start[row + (uint32_t)x0]; p < e; ++p) nn_consider(best, qx, qy, qz, g.pts[p]);
                } else {                                                            // only the two end cells of the run lie on the shell (R >= 1 here)
#pragma unroll 1
                    for (int k = 0; k < 2; ++k) {
                        const int xx = k ? cx + R : cx - R;
                        if (xx < 0 || xx >= nx) continue;
                        const uint32_t e = g.start[row + (uint32_t)xx + 1u];
                        for (uint32_t p = g.start[row + (uint32_t)xx]; p < e; ++p) nn_consider(best, qx, qy, qz, g.pts[p]);
                    }
                }
            }
        }
        const double lim = (double)R * g.h - g.slack;
        const bool covered = cx - R <= 0 && cx + R >= nx - 1 && cy - R <= 0 && cy + R >= ny - 1 && cz - R <= 0 && cz + R >= nz - 1;
        if (covered || (lim > 0.0 && best.d2 < lim * lim)) { closed = true; break; }
    }
    if (closed) {
        nn_store(best, out, dist, index);
    } else {
        const uint32_t slot = atomicAdd(fb_count, 1u);
        if (slot < nq) fb_list[slot] = i;
    }
}

// Brute force.  targets: t4 [m] (x, y, z, original index) when given, else t3 [m,3] with index = position.  Queries as in k_nn_grid; with
// `list` only the query positions list[0 .. *list_count) are served.  Every lane reads the same LDS entry (a broadcast: no bank conflict).
// A workgroup walks ALL targets whatever its number of queries, so its time is the targets' (fp64 rate: ~160 cycles per target and query slot).
__global__ __launch_bounds__(kReconThreads) void k_nn_scan(uint32_t m, const float* __restrict__ t3, const float4* __restrict__ t4, uint32_t nq,
                                                            const float* __restrict__ q3, const float4* __restrict__ q4, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ list_count, double* __restrict__ dist, int32_t* __restrict__ index) {
    __shared__ float4 tile[kScanTile];
    const uint32_t n_eff = list != nullptr ? min(*list_count, nq) : nq;
    const uint32_t base = blockIdx.x * (uint32_t)(kReconThreads * kScanQ);
    if (base >= n_eff) return;                                                      // (uniform over the workgroup)
    double qx[kScanQ], qy[kScanQ], qz[kScanQ];
    uint32_t out[kScanQ];
    bool valid[kScanQ];
    NnBest best[kScanQ];
#pragma unroll
    for (int k = 0; k < kScanQ; ++k) {
        const uint32_t slot = base + (uint32_t)k * kReconThreads + threadIdx.x;
        valid[k] = slot < n_eff;
        const uint32_t id = valid[k] ? (list != nullptr ? min(list[slot], nq - 1u) : slot) : 0u;
        out[k] = id;
        if (q4 != nullptr) {
            const float4 q = q4[id];
            qx[k] = (double)q.x; qy[k] = (double)q.y; qz[k] = (double)q.z; out[k] = (uint32_t)__float_as_int(q.w);
        } else {
            qx[k] = (double)q3[(size_t)id * 3u]; qy[k] = (double)q3[(size_t)id * 3u + 1u]; qz[k] = (double)q3[(size_t)id * 3u + 2u];
        }
        best[k] = NnBest{__builtin_inf(), kNoIndex};
    }
    for (uint32_t t0 = 0; t0 < m; t0 += kScanTile) {
#pragma unroll
        for (uint32_t r = 0; r < kScanTile / kReconThreads; ++r) {
            const uint32_t j = t0 + r * kReconThreads + threadIdx.x;
            if (j < m)
                tile[r * kReconThreads + threadIdx.x] = t4 != nullptr ? t4[j] : make_float4(t3[(size_t)j * 3u], t3[(size_t)j * 3u + 1u], t3[(size_t)j * 3u + 2u], __int_as_float((int)j));
        }
        __syncthreads();
        const uint32_t cnt = min(kScanTile, m - t0);
        for (uint32_t j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
#pragma unroll
            for (int k = 0; k < kScanQ; ++k) nn_consider(best[k], qx[k], qy[k], qz[k], p);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kScanQ; ++k)
        if (valid[k]) nn_store(best[k], out[k], dist, index);
}

// ---- reduction --------------------------------------------------------------------------------------------------------------------------------
// fixed order: thread t of workgroup b adds d[b*2048 + t + 256*k], k = 0..7 in turn; the 256 sums fold by halves in LDS; k_dist_finish does the same
// over the workgroups' partials.  out[0] = mean, out[1] = number of distances < threshold (exact: an integer count carried in a double).
__device__ __forceinline__ void dist_fold(double* s_sum, unsigned long long* s_cnt, double& sum, unsigned long long& cnt) {
    s_sum[threadIdx.x] = sum;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (uint32_t w = kReconThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w];
        }
        __syncthreads();
    }
    sum = s_sum[0];
    cnt = s_cnt[0];
}

__global__ __launch_bounds__(kReconThreads) void k_dist_partial(uint32_t n, const double* __restrict__ d, double threshold, double* __restrict__ part_sum,
                                                                 unsigned long long* __restrict__ part_cnt) {
    __shared__ double s_sum[kReconThreads];
    __shared__ unsigned long long s_cnt[kReconThreads];
    double sum = 0.0;
    unsigned long long cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDistPer; ++k) {
        const uint32_t i = blockIdx.x * (kReconThreads * kDistPer) + k * kReconThreads + threadIdx.x;
        if (i < n) {
            const double v = d[i];
            sum += v;
            cnt += v < threshold ? 1ull : 0ull;
        }
    }
    dist_fold(s_sum, s_cnt, sum, cnt);
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = sum; part_cnt[blockIdx.x] = cnt; }
}

__global__ __launch_bounds__(kReconThreads) void k_dist_finish(uint32_t n, uint32_t n_parts, const double* __restrict__ part_sum,
                                                                const unsigned long long* __restrict__ part_cnt, double* __restrict__ out) {
    __shared__ double s_sum[kReconThreads];
    __shared__ unsigned long long s_cnt[kReconThreads];
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kReconThreads) {
        sum += part_sum[i];
        cnt += part_cnt[i];
    }
    dist_fold(s_sum, s_cnt, sum, cnt);
    if (threadIdx.x == 0) { out[0] = sum / (double)n; out[1] = (double)cnt; }
}

}  // namespace naruto
