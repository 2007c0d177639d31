// The planner's local RRT on the device (reference src/planner/rrt.py, src/planner/rrt_naruto.py: RRTNaruto).
//
// k_rrt_grow      RRTNaruto.run() / run_full() as ONE persistent launch of one workgroup: the algorithm is sequential over
//                 iterations, the parallelism is inside an iteration (segment samples, nearest-node candidates, new nodes
//                 spread over the lanes).  It returns to the host only when it is done, out of random rows or out of room.
// k_segments_free is_collision_free (rrt.py:77-117) for many segments, one wave per segment, the grower's device functions.
// k_reachable_mask get_reachable_mask (rrt.py:389-431) over the grower's per-voxel cell lists (or node tiles through LDS).
//
// Everything that DECIDES something is fp64 in the reference's operation order, with contraction switched off in these
// functions (the library is built with -O3, which contracts a*b+c into one rounding): np.linspace's start + i*(delta/div)
// with the last sample set to the end point, the eight-term trilinear sum left to right with the float32 volume values
// promoted, sqrt((x*x + y*y) + z*z).  The two goal tests and the mask are float32 because the reference's are (torch.norm
// of float32 tensors).

#include "naruto_common.h"

namespace naruto {

#define RRT_FP _Pragma("clang fp contract(off)")

struct D3 { double x, y, z; };
struct RrtVol { const float* v; int X, Y, Z; };

// layout of the int32 state block at the head of the workspace (NARUTO_RRT_STATE_* in the header)
enum { kRrtNodes = NARUTO_RRT_STATE_NODES, kRrtIter = NARUTO_RRT_STATE_ITER, kRrtRrtIter = NARUTO_RRT_STATE_RRT_ITER, kRrtStatus = NARUTO_RRT_STATE_STATUS,
       kRrtRowsUsed = NARUTO_RRT_STATE_ROWS_USED, kRrtGoalParent = NARUTO_RRT_STATE_GOAL_PARENT, kRrtReachable = NARUTO_RRT_STATE_REACHABLE,
       kRrtMidIter = NARUTO_RRT_STATE_MID_ITER, kRrtUseCells = NARUTO_RRT_STATE_USE_CELLS, kRrtStateInts = NARUTO_RRT_STATE_INTS };
constexpr int kRrtGoalOffset = 64;        // bytes: fp64[4]
constexpr int kRrtHeadOffset = 128;       // bytes: int32[X*Y*Z]

__device__ __forceinline__ double rrt_norm(double x, double y, double z) {
    RRT_FP
    return sqrt((x * x + y * y) + z * z);
}
__device__ __forceinline__ float rrt_norm32(float x, float y, float z) {
    RRT_FP
    return sqrtf((x * x + y * y) + z * z);
}

// trilinear_interpolation (rrt.py:12-60) > thre.  Outside [0, dim-1] (or NaN) counts as blocked; at exactly dim-1 the upper
// corner has weight 0 and its index is clamped (the reference returns None / indexes out of bounds there).
__device__ __forceinline__ bool rrt_free_at(const RrtVol& vol, double x, double y, double z, double thre) {
    RRT_FP
    const double hx = (double)(vol.X - 1), hy = (double)(vol.Y - 1), hz = (double)(vol.Z - 1);
    if (!(x >= 0.0 && x <= hx && y >= 0.0 && y <= hy && z >= 0.0 && z <= hz)) return false;
    const int x0 = (int)x, y0 = (int)y, z0 = (int)z;
    const int x1 = min(x0 + 1, vol.X - 1), y1 = min(y0 + 1, vol.Y - 1), z1 = min(z0 + 1, vol.Z - 1);
    const double dx = x - (double)x0, dy = y - (double)y0, dz = z - (double)z0;
    const double ux = 1.0 - dx, uy = 1.0 - dy, uz = 1.0 - dz;
    const float* __restrict__ v = vol.v;
    const int r00 = (x0 * vol.Y + y0) * vol.Z, r01 = (x0 * vol.Y + y1) * vol.Z, r10 = (x1 * vol.Y + y0) * vol.Z, r11 = (x1 * vol.Y + y1) * vol.Z;
    const double c000 = (double)v[r00 + z0], c001 = (double)v[r00 + z1], c010 = (double)v[r01 + z0], c011 = (double)v[r01 + z1];
    const double c100 = (double)v[r10 + z0], c101 = (double)v[r10 + z1], c110 = (double)v[r11 + z0], c111 = (double)v[r11 + z1];
    double s = ((ux * uy) * uz) * c000;
    s = s + ((ux * uy) * dz) * c001;
    s = s + ((ux * dy) * uz) * c010;
    s = s + ((ux * dy) * dz) * c011;
    s = s + ((dx * uy) * uz) * c100;
    s = s + ((dx * uy) * dz) * c101;
    s = s + ((dx * dy) * uz) * c110;
    s = s + ((dx * dy) * dz) * c111;
    return s > thre;
}

// the samples of is_collision_free: np.linspace(pa, pb, num), num = ceil(|pb - pa| / (step / 5)) + 1
struct RrtSeg {
    D3 pa, pb, m;        // m: delta / div, or delta itself in numpy's zero-step form ((i / div) * delta)
    double div;
    int num;             // -1: not a finite segment
    bool zero_form;
};
__device__ __forceinline__ RrtSeg rrt_seg_setup(const D3& pa, const D3& pb, double step_size) {
    RRT_FP
    RrtSeg s;
    s.pa = pa; s.pb = pb;
    const double ex = pb.x - pa.x, ey = pb.y - pa.y, ez = pb.z - pa.z;
    const double arg = rrt_norm(ex, ey, ez) / (step_size / 5.0);
    s.num = (arg < 1.0e9) ? (int)ceil(arg) + 1 : -1;
    s.div = (double)(s.num - 1);
    s.m = D3{ex, ey, ez};
    s.zero_form = true;
    if (s.num > 1) {
        const double sx = ex / s.div, sy = ey / s.div, sz = ez / s.div;
        s.zero_form = sx == 0.0 || sy == 0.0 || sz == 0.0;
        if (!s.zero_form) s.m = D3{sx, sy, sz};
    }
    return s;
}
__device__ __forceinline__ bool rrt_seg_free(const RrtVol& vol, const RrtSeg& s, int i, double thre) {
    RRT_FP
    double x, y, z;
    if (i == s.num - 1 && s.num > 1) { x = s.pb.x; y = s.pb.y; z = s.pb.z; }
    else if (s.num == 1) { x = s.pa.x; y = s.pa.y; z = s.pa.z; }
    else {
        double t = (double)i;
        if (s.zero_form) t = t / s.div;
        x = t * s.m.x + s.pa.x; y = t * s.m.y + s.pa.y; z = t * s.m.z + s.pa.z;
    }
    return rrt_free_at(vol, x, y, z, thre);
}
// first_blocked >= num: every sample free.  Python's floor division: a blocked first sample gives -1.
__device__ __forceinline__ int rrt_seg_result(int num, uint32_t first_blocked, bool& complete) {
    complete = num > 0 && first_blocked >= (uint32_t)num;
    if (num <= 0) return -1;
    if (complete) return max((num - 1) / 5, 1);
    return first_blocked == 0u ? -1 : (int)((first_blocked - 1u) / 5u);
}

__device__ __forceinline__ int rrt_cell(const RrtVol& vol, float x, float y, float z) {
    const int ix = (int)fminf(fmaxf(floorf(x), 0.0f), (float)(vol.X - 1));
    const int iy = (int)fminf(fmaxf(floorf(y), 0.0f), (float)(vol.Y - 1));
    const int iz = (int)fminf(fmaxf(floorf(z), 0.0f), (float)(vol.Z - 1));
    return (ix * vol.Y + iy) * vol.Z + iz;
}

// ---- is_collision_free for N segments: one wave per segment ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_segments_free(RrtVol vol, uint32_t n, const double* __restrict__ pa, const double* __restrict__ pb, double step_size,
                                                       double thre, int32_t* __restrict__ n_free, uint8_t* __restrict__ complete_free) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n) return;
    const D3 a{pa[3 * (size_t)g], pa[3 * (size_t)g + 1], pa[3 * (size_t)g + 2]}, b{pb[3 * (size_t)g], pb[3 * (size_t)g + 1], pb[3 * (size_t)g + 2]};
    const RrtSeg s = rrt_seg_setup(a, b, step_size);
    uint32_t fb = 0xFFFFFFFFu;
    for (int base = 0; base < s.num; base += 64) {
        const int i = base + lane;
        const bool blocked = i < s.num && !rrt_seg_free(vol, s, i, thre);
        const unsigned long long m = __ballot(blocked);
        if (m != 0ull) { fb = (uint32_t)base + (uint32_t)__builtin_ctzll(m); break; }
    }
    bool complete;
    const int c = rrt_seg_result(s.num, fb, complete);
    if (lane == 0) { n_free[g] = c; complete_free[g] = complete ? 1 : 0; }
}

// ---- the grower ------------------------------------------------------------------------------------------------------------
struct RrtShared {
    unsigned long long dkey[2][16];
    int didx[2][16];
    uint32_t umin[2][16];
    int cells[1024];
};

struct RrtArgs {
    RrtVol vol;
    double step, amp, thre;
    int direct, mode, restart;
    double* xyz64; float* xyz32; int32_t* parent; int32_t* next; int32_t* head; int32_t* state; const double* goal;
    const double* rows;
    int n_rows, max_iter, cap, cell_threshold;
};

// workgroup minimum; the result buffers alternate (par) so that a reduction needs one barrier: a buffer is written again only
// after another reduction's barrier, which every thread reaches after it has read this one
__device__ __forceinline__ uint32_t rrt_wg_min(RrtShared& sh, int& par, uint32_t v) {
    v = wave_min_u32(v);
    const int nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) sh.umin[par][threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0xFFFFFFFFu;
    for (int w = 0; w < nw; ++w) r = min(r, sh.umin[par][w]);
    par ^= 1;
    return r;
}
// workgroup minimum of (distance, index), lexicographic: non-negative doubles order as their bit patterns
__device__ __forceinline__ void rrt_wg_argmin(RrtShared& sh, int& par, double& d, int& idx) {
    unsigned long long k = (unsigned long long)__double_as_longlong(d);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long ko = __shfl_xor(k, o);
        const int io = __shfl_xor(idx, o);
        if (ko < k || (ko == k && io < idx)) { k = ko; idx = io; }
    }
    const int nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) { sh.dkey[par][threadIdx.x >> 6] = k; sh.didx[par][threadIdx.x >> 6] = idx; }
    __syncthreads();
    k = sh.dkey[par][0]; idx = sh.didx[par][0];
    for (int w = 1; w < nw; ++w) {
        const unsigned long long ko = sh.dkey[par][w];
        const int io = sh.didx[par][w];
        if (ko < k || (ko == k && io < idx)) { k = ko; idx = io; }
    }
    par ^= 1;
    d = __longlong_as_double((long long)k);
}

// find_nearest_node (rrt.py:299-311): fp64 differences against the float32 node coordinates, lowest index among equals
__device__ __forceinline__ void rrt_candidate(const float* xyz32, int j, const D3& q, double& bd, int& bi) {
    RRT_FP
    const double ex = q.x - (double)xyz32[3 * j], ey = q.y - (double)xyz32[3 * j + 1], ez = q.z - (double)xyz32[3 * j + 2];
    const double d = rrt_norm(ex, ey, ez);
    if (d < bd || (d == bd && j < bi)) { bd = d; bi = j; }
}
__device__ int rrt_nearest(const RrtArgs& a, RrtShared& sh, int& par, int n, bool cells, const D3& q) {
    double bd = __builtin_huge_val();
    int bi = 0x7FFFFFFF;
    if (!cells) {
        for (int j = (int)threadIdx.x; j < n; j += (int)blockDim.x) rrt_candidate(a.xyz32, j, q, bd, bi);
        rrt_wg_argmin(sh, par, bd, bi);
        return bi < n ? bi : 0;                                         // a query that is not a number compares with nothing
    }
    // cubes of cells growing outward from the query's cell: once every cell within Chebyshev distance R has been examined, every
    // unseen node is farther than R from the query, so a best distance <= R is final (ties included: equal distances are all seen)
    const RrtVol& vol = a.vol;
    const int cx = (int)fmin(fmax(floor(q.x), 0.0), (double)(vol.X - 1)), cy = (int)fmin(fmax(floor(q.y), 0.0), (double)(vol.Y - 1)),
              cz = (int)fmin(fmax(floor(q.z), 0.0), (double)(vol.Z - 1));
    int r_prev = -1, r = 1;
    for (;;) {
        const int side = 2 * r + 1, total = side * side * side;
        for (int t = (int)threadIdx.x; t < total; t += (int)blockDim.x) {
            const int oz = t % side - r, oy = (t / side) % side - r, ox = t / (side * side) - r;
            if (max(max(abs(ox), abs(oy)), abs(oz)) <= r_prev) continue;
            const int x = cx + ox, y = cy + oy, z = cz + oz;
            if (x < 0 || x >= vol.X || y < 0 || y >= vol.Y || z < 0 || z >= vol.Z) continue;
            for (int j = a.head[(x * vol.Y + y) * vol.Z + z]; j >= 0; j = a.next[j]) rrt_candidate(a.xyz32, j, q, bd, bi);
        }
        rrt_wg_argmin(sh, par, bd, bi);
        if (bd <= (double)r) break;
        if (cx - r <= 0 && cy - r <= 0 && cz - r <= 0 && cx + r >= vol.X - 1 && cy + r >= vol.Y - 1 && cz + r >= vol.Z - 1) break;
        r_prev = r;
        r += max(1, r >> 1);
    }
    return bi < n ? bi : 0;
}

// first blocked sample of a segment over the whole workgroup (num if none)
__device__ __forceinline__ uint32_t rrt_first_blocked(const RrtArgs& a, RrtShared& sh, int& par, const RrtSeg& s, double thre) {
    uint32_t fb = 0xFFFFFFFFu;
    for (int base = 0; base < s.num; base += (int)blockDim.x) {
        const int i = base + (int)threadIdx.x;
        const bool blocked = i < s.num && !rrt_seg_free(a.vol, s, i, thre);
        fb = rrt_wg_min(sh, par, blocked ? (uint32_t)i : 0xFFFFFFFFu);
        if (fb != 0xFFFFFFFFu) break;
    }
    return fb;
}

// nodes n .. n+cnt-1 = base + dir * min(step * (i + 1), dist), each the parent of the next (rrt_naruto.py:115-125, :176-185), linked
// into the cell lists without atomics (one workgroup: a node's predecessor in its cell is found among the batch through LDS).
// Returns whether a new node (the last one only if !test_all) is closer to the goal than step in float32.
// Cost: a thread looks through its batch's cells in LDS, so a batch of c nodes costs c reads per thread.  The design assumes what the planner
// produces: cnt <= step_amplifier for an extension (10 in the shipped configs) and cnt <= the volume's diagonal / step for a direct line (82 at
// office_0), i.e. one batch of well under 100.  Longer lines stay correct (batches of 1024, up to 1024 LDS reads per thread and batch) but are
// not what this loop is tuned for.
__device__ bool rrt_append(const RrtArgs& a, RrtShared& sh, int& par, int n, int cnt, int parent0, const D3& base, const D3& dir, double dist,
                           bool test_all, float gx, float gy, float gz) {
    RRT_FP
    bool hit = false;
    for (int b = 0; b < cnt; b += (int)blockDim.x) {
        const int i = b + (int)threadIdx.x, chunk = min(cnt - b, (int)blockDim.x);
        int cell = -1, old_head = -1;
        bool mine = false;
        if (i < cnt) {
            const double m = fmin(a.step * (double)(i + 1), dist);
            const double x = base.x + dir.x * m, y = base.y + dir.y * m, z = base.z + dir.z * m;
            const float fx = (float)x, fy = (float)y, fz = (float)z;
            const int j = n + i;
            a.xyz64[3 * j] = x; a.xyz64[3 * j + 1] = y; a.xyz64[3 * j + 2] = z;
            a.xyz32[3 * j] = fx; a.xyz32[3 * j + 1] = fy; a.xyz32[3 * j + 2] = fz;
            a.parent[j] = i == 0 ? parent0 : j - 1;
            cell = rrt_cell(a.vol, fx, fy, fz);
            old_head = a.head[cell];
            if (test_all || i == cnt - 1) mine = rrt_norm32(fx - gx, fy - gy, fz - gz) < (float)a.step;
        }
        sh.cells[threadIdx.x] = cell;
        const bool any = rrt_wg_min(sh, par, mine ? 0u : 1u) == 0u;        // its barrier also publishes cells[] and the old heads read above
        hit = hit || any;
        if (i < cnt) {
            int prev = -1;
            for (int t = (int)threadIdx.x - 1; t >= 0; --t)
                if (sh.cells[t] == cell) { prev = t; break; }
            bool later = false;
            for (int t = (int)threadIdx.x + 1; t < chunk; ++t)
                if (sh.cells[t] == cell) { later = true; break; }
            a.next[n + i] = prev >= 0 ? n + b + prev : old_head;
            if (!later) a.head[cell] = n + i;
        }
        __syncthreads();                                                  // cells[] is rewritten by the next batch; heads / nodes are read next
    }
    return hit;
}

__global__ __launch_bounds__(1024) void k_rrt_grow(RrtArgs a) {
    RRT_FP
    __shared__ RrtShared sh;
    int par = 0;
    int n = a.state[kRrtNodes], it = a.restart ? 0 : a.state[kRrtIter], rrt_iter = a.state[kRrtRrtIter];
    bool mid = a.restart ? false : a.state[kRrtMidIter] != 0;         // the direct-line half of iteration `it` is already done
    const bool use_cells = a.state[kRrtUseCells] != 0;
    int rows_used = 0, status = NARUTO_RRT_DONE;
    const D3 goal{a.goal[0], a.goal[1], a.goal[2]};
    const float gx = (float)goal.x, gy = (float)goal.y, gz = (float)goal.z;
    const bool run = a.mode == NARUTO_RRT_MODE_RUN;
    const double reach = a.step * a.amp;
    __syncthreads();                                                   // everyone has read the state before anyone writes it again

    while (it < a.max_iter) {
        if (!mid) {
            if (run && a.direct) {
                // extend_tree_straight (rrt_naruto.py:92-133): sampled FROM THE GOAL, default threshold 0.5
                const int last = n - 1;
                const D3 pl{a.xyz64[3 * last], a.xyz64[3 * last + 1], a.xyz64[3 * last + 2]};
                const RrtSeg s = rrt_seg_setup(goal, pl, a.step);
                bool complete;
                const int cnt = rrt_seg_result(s.num, rrt_first_blocked(a, sh, par, s, 0.5), complete);
                bool reached = false;
                if (cnt > 0) {
                    if (n + cnt > a.cap) { status = NARUTO_RRT_NEED_ROOM; break; }
                    const double ex = goal.x - pl.x, ey = goal.y - pl.y, ez = goal.z - pl.z;
                    const double dist = rrt_norm(ex, ey, ez);
                    if (dist == 0.0) reached = true;                   // the reference divides by zero here
                    else {
                        reached = rrt_append(a, sh, par, n, cnt, last, pl, D3{ex / dist, ey / dist, ez / dist}, dist, false, gx, gy, gz);
                        n += cnt;
                    }
                }
                ++rrt_iter;
                if (reached) { ++it; break; }
            } else if (run) ++rrt_iter;
            mid = true;
        }
        // extend_tree (rrt_naruto.py:135-187)
        if (rows_used >= a.n_rows) { status = NARUTO_RRT_NEED_ROWS; break; }
        const D3 rp{a.rows[3 * (size_t)rows_used], a.rows[3 * (size_t)rows_used + 1], a.rows[3 * (size_t)rows_used + 2]};
        const int near = rrt_nearest(a, sh, par, n, use_cells && n >= a.cell_threshold, rp);
        const D3 pn{a.xyz64[3 * near], a.xyz64[3 * near + 1], a.xyz64[3 * near + 2]};
        D3 pnew = rp;
        {
            const double ex = rp.x - pn.x, ey = rp.y - pn.y, ez = rp.z - pn.z;
            const double dist = rrt_norm(ex, ey, ez);
            if (dist > reach) {
                const double m = fmin(reach, dist);
                pnew = D3{pn.x + ex / dist * m, pn.y + ey / dist * m, pn.z + ez / dist * m};
            }
        }
        const RrtSeg s = rrt_seg_setup(pn, pnew, a.step);
        bool complete;
        int cnt = rrt_seg_result(s.num, rrt_first_blocked(a, sh, par, s, a.thre), complete);
        const double ex = pnew.x - pn.x, ey = pnew.y - pn.y, ez = pnew.z - pn.z;
        const double dist = rrt_norm(ex, ey, ez);
        if (!(dist > 0.0)) cnt = 0;                                     // the random point IS the nearest node: nothing to add
        if (cnt > 0 && n + cnt > a.cap) { status = NARUTO_RRT_NEED_ROOM; break; }
        ++rows_used;
        ++it;
        mid = false;
        if (cnt > 0) {
            const bool hit = rrt_append(a, sh, par, n, cnt, near, pn, D3{ex / dist, ey / dist, ez / dist}, dist, true, gx, gy, gz);
            n += cnt;
            if (run && hit) break;
        }
    }

    int goal_parent = a.state[kRrtGoalParent], reachable = a.state[kRrtReachable];
    if (status == NARUTO_RRT_DONE && run) {
        // run() after the loop (rrt_naruto.py:226-234)
        goal_parent = rrt_nearest(a, sh, par, n, use_cells && n >= a.cell_threshold, goal);
        const double d = rrt_norm(a.xyz64[3 * goal_parent] - goal.x, a.xyz64[3 * goal_parent + 1] - goal.y, a.xyz64[3 * goal_parent + 2] - goal.z);
        reachable = d <= a.step ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.state[kRrtNodes] = n; a.state[kRrtIter] = it; a.state[kRrtRrtIter] = rrt_iter; a.state[kRrtStatus] = status;
        a.state[kRrtRowsUsed] = rows_used; a.state[kRrtGoalParent] = goal_parent; a.state[kRrtReachable] = reachable;
        a.state[kRrtMidIter] = mid ? 1 : 0;
    }
}

// start_new_plan (rrt.py:248-277): the tree is the start node alone, every cell list empty but the start's
__global__ __launch_bounds__(256) void k_rrt_start(RrtVol vol, D3 start, D3 goal, int use_cells, double* __restrict__ xyz64, float* __restrict__ xyz32,
                                                   int32_t* __restrict__ parent, int32_t* __restrict__ next, int32_t* __restrict__ head,
                                                   int32_t* __restrict__ state, double* __restrict__ goal_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const float sx = (float)start.x, sy = (float)start.y, sz = (float)start.z;
    const int c0 = rrt_cell(vol, sx, sy, sz);
    if (i < vol.X * vol.Y * vol.Z) head[i] = i == c0 ? 0 : -1;
    if (i == 0) {
        xyz64[0] = start.x; xyz64[1] = start.y; xyz64[2] = start.z;
        xyz32[0] = sx; xyz32[1] = sy; xyz32[2] = sz;
        parent[0] = -1; next[0] = -1;
        goal_out[0] = goal.x; goal_out[1] = goal.y; goal_out[2] = goal.z; goal_out[3] = 0.0;
        for (int k = 0; k < kRrtStateInts; ++k) state[k] = 0;
        state[kRrtNodes] = 1; state[kRrtGoalParent] = -1; state[kRrtUseCells] = use_cells;
    }
}

// get_reachable_mask (rrt.py:389-431): 1 where some node lies within step_size of the voxel, float32 arithmetic as torch.norm.
// A node within step of voxel p has floor(coordinate) in [p - ceil(step), p + ceil(step)] on every axis.
__global__ __launch_bounds__(256) void k_reachable_mask(RrtVol vol, float step, const float* __restrict__ xyz32, const int32_t* __restrict__ head,
                                                        const int32_t* __restrict__ next, const int32_t* __restrict__ state, float* __restrict__ mask) {
    __shared__ float tile[256 * 3];
    __shared__ int pending;
    const int n_vox = vol.X * vol.Y * vol.Z;
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool live = v < n_vox;
    const int z = v % vol.Z, y = (v / vol.Z) % vol.Y, x = v / (vol.Z * vol.Y);
    const float px = (float)x, py = (float)y, pz = (float)z;
    bool found = false;
    if (state[kRrtUseCells]) {
        if (live) {
            const int r = (int)ceilf(step);
            for (int cx = max(x - r, 0); cx <= min(x + r, vol.X - 1) && !found; ++cx)
                for (int cy = max(y - r, 0); cy <= min(y + r, vol.Y - 1) && !found; ++cy)
                    for (int cz = max(z - r, 0); cz <= min(z + r, vol.Z - 1) && !found; ++cz)
                        for (int j = head[(cx * vol.Y + cy) * vol.Z + cz]; j >= 0; j = next[j])
                            if (rrt_norm32(px - xyz32[3 * j], py - xyz32[3 * j + 1], pz - xyz32[3 * j + 2]) <= step) { found = true; break; }
        }
    } else {
        const int n = state[kRrtNodes];
        for (int b = 0; b < n; b += 256) {
            if (threadIdx.x == 0) pending = 0;
            __syncthreads();
            const int m = min(256, n - b);
            for (int t = (int)threadIdx.x; t < 3 * m; t += 256) tile[t] = xyz32[3 * b + t];
            if (live && !found) pending = 1;
            __syncthreads();
            if (!pending) break;                                        // every voxel of the workgroup has its node
            if (live && !found)
                for (int t = 0; t < m; ++t)
                    if (rrt_norm32(px - tile[3 * t], py - tile[3 * t + 1], pz - tile[3 * t + 2]) <= step) { found = true; break; }
            __syncthreads();
        }
    }
    if (live) mask[v] = found ? 1.0f : 0.0f;
}

// One thread chasing parent pointers through global memory: a path is a chain of dependent loads whatever runs it, and it is as long as the
// tree is deep (tens of nodes at office_0), once per plan.
// find_path (rrt.py:376-387) as node indices: path[0] = count, then goal.parent, its parent, ..., the start (the walk stops after cap entries)
__global__ void k_rrt_path(const int32_t* __restrict__ parent, const int32_t* __restrict__ state, int cap, int32_t* __restrict__ path) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n = state[kRrtNodes];
    int c = 0;
    for (int j = state[kRrtGoalParent]; j >= 0 && j < n && c < cap; j = parent[j]) path[1 + c++] = j;
    path[0] = c;
}

#undef RRT_FP

}  // namespace naruto
