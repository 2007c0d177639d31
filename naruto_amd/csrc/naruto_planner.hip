// "Next" row N3 of SURVEY.md section 8(f): the planner's uncertainty aggregation in goal space
// (reference src/planner/naruto_planner.py, NarutoPlanner.uncertainty_aggregation_v2 :596-735).
//
// The reference materialises [G, k, 3] view vectors, a [G, k] distance mask and a [valid, 30, 3] visibility ray-march as
// broadcast torch ops every time new volumes arrive.  Here: one wave per goal candidate, the k target voxels strided over
// the lanes, the 30-step march in registers; plus the target selection (top_k largest uncertainties, thinned to a
// subset) as a radix select on the device.

#include "naruto_common.h"

namespace naruto {

struct VolDims { int X, Y, Z; };

// keys whose ascending order is DESCENDING value order (NaN first): the K smallest keys are the K largest values
__global__ __launch_bounds__(256) void k_topk_keys(uint32_t n, const float* __restrict__ vol, uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ~sortable_key(vol[i]);
}

// sel = the top_k flat indices in ascending index order -> targets[i] = unravel(sel[floor(i * top_k / subset)])
__global__ __launch_bounds__(256) void k_topk_thin(const uint32_t* __restrict__ sel, uint32_t top_k, uint32_t subset, VolDims d, int32_t* __restrict__ targets) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= subset) return;
    const uint32_t flat = sel[(uint32_t)(((uint64_t)i * top_k) / subset)];
    targets[3 * i + 0] = (int32_t)(flat / (uint32_t)(d.Y * d.Z));
    targets[3 * i + 1] = (int32_t)((flat / (uint32_t)d.Z) % (uint32_t)d.Y);
    targets[3 * i + 2] = (int32_t)(flat % (uint32_t)d.Z);
}

// torch.linspace(0, 1, 30) in fp32 (aten RangeFactories: symmetric two-sided formula)
__device__ __forceinline__ float linspace30(int i) {
    const float step = __fdiv_rn(1.0f, 29.0f);
    return i < 15 ? __fmul_rn(step, (float)i) : __fsub_rn(1.0f, __fmul_rn(step, (float)(29 - i)));
}

// one wave per goal: collections[g][k] = uncert[target k] if the pair is in sensing range, the goal is safe and the segment
// goal -> target sees only positive sdf; aggregated[g] = sum_k collections[g][k]
__global__ __launch_bounds__(256) void k_goal_aggregate(VolDims d, const float* __restrict__ uncert, const float* __restrict__ sdf, uint32_t n_goals,
                                                        const int32_t* __restrict__ goal_idx, uint32_t n_targets, const int32_t* __restrict__ targets,
                                                        float min_dist, float max_dist, float safe_sdf, float* __restrict__ collections,
                                                        float* __restrict__ aggregated) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n_goals) return;
    const int gx = goal_idx[3 * g], gy = goal_idx[3 * g + 1], gz = goal_idx[3 * g + 2];
    auto at = [&](const float* __restrict__ v, int x, int y, int z) { return v[((size_t)x * d.Y + y) * d.Z + z]; };
    auto cl = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    // naruto_planner.py:657-668: goals on the volume border, or with sdf < safe_sdf at the goal or a 6-neighbour, are unsafe
    bool unsafe = gx < 1 || gx + 1 >= d.X || gy < 1 || gy + 1 >= d.Y || gz < 1 || gz + 1 >= d.Z;
    const int gxc = cl(gx, d.X), gyc = cl(gy, d.Y), gzc = cl(gz, d.Z);
    unsafe = unsafe || at(sdf, gxc, gyc, gzc) < safe_sdf || at(sdf, cl(gx + 1, d.X), gyc, gzc) < safe_sdf || at(sdf, cl(gx - 1, d.X), gyc, gzc) < safe_sdf ||
             at(sdf, gxc, cl(gy + 1, d.Y), gzc) < safe_sdf || at(sdf, gxc, cl(gy - 1, d.Y), gzc) < safe_sdf ||
             at(sdf, gxc, gyc, cl(gz + 1, d.Z)) < safe_sdf || at(sdf, gxc, gyc, cl(gz - 1, d.Z)) < safe_sdf;
    const float px = (float)gx, py = (float)gy, pz = (float)gz;
    float acc = 0.0f;
    for (uint32_t k = lane; k < n_targets; k += 64u) {
        const int tx = targets[3 * k], ty = targets[3 * k + 1], tz = targets[3 * k + 2];
        const float vx = px - (float)tx, vy = py - (float)ty, vz = pz - (float)tz;          // view_vec (:640)
        const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz)));
        bool ok = !unsafe && dist < max_dist && dist > min_dist;
        if (ok) {
            // visibility (:673-681): 30 points goal - t * view_vec, truncated to voxel indices, all with sdf > 0
            float m = __builtin_huge_valf();
#pragma unroll 6
            for (int i = 0; i < 30; ++i) {
                const float t = linspace30(i);
                const int ix = (int)__fsub_rn(px, __fmul_rn(t, vx)), iy = (int)__fsub_rn(py, __fmul_rn(t, vy)), iz = (int)__fsub_rn(pz, __fmul_rn(t, vz));
                m = fminf(m, at(sdf, cl(ix, d.X), cl(iy, d.Y), cl(iz, d.Z)));
            }
            ok = m > 0.0f;
        }
        const float v = ok ? at(uncert, tx, ty, tz) : 0.0f;
        collections[(size_t)g * n_targets + k] = v;
        acc += v;
    }
    acc = wave_sum(acc);
    if (lane == 0) aggregated[g] = acc;
}

// ---- goal search (reference goal_search_v2, naruto_planner.py:462-510) ---------------------------------------------------------
// One workgroup, one launch: the goal is the argmax of aggregated[G] (ties: lowest flat index), the look-at targets are the top
// m = min(obs_per_goal, K) entries of the goal's row of collections[G,K] (value descending, then target index ascending).  Values are
// ordered by the key of k_topk_keys above (~sortable_key: ascending key = descending value, NaN first), so every comparison is an
// integer one and the result does not depend on the number of threads or on which lane meets which element.

constexpr uint32_t kGoalSearchMaxTargets = NARUTO_GOAL_SEARCH_MAX_TARGETS;     // the row's keys sit in LDS (16 KiB)
constexpr uint32_t kGoalSearchHeadInts = NARUTO_GOAL_SEARCH_HEAD_INTS;

struct GoalSearchFrame { double bx, by, bz, voxel; };

// min over the wave of the pair (hi, lo) in lexicographic order
__device__ __forceinline__ void wave_min_pair(uint32_t& hi, uint32_t& lo) {
    const uint32_t k = wave_min_u32(hi);
    lo = wave_min_u32(hi == k ? lo : 0xFFFFFFFFu);
    hi = k;
}

// vox2loc (planner.py:99): vox * voxel_size + bbox[:, 0] in fp64, the product rounded before the sum (no fused multiply-add)
__device__ __forceinline__ void goal_search_loc(int32_t tx, int32_t ty, int32_t tz, const GoalSearchFrame& fr, double* __restrict__ loc) {
#pragma clang fp contract(off)
    const double px = (double)tx * fr.voxel, py = (double)ty * fr.voxel, pz = (double)tz * fr.voxel;
    loc[0] = px + fr.bx;
    loc[1] = py + fr.by;
    loc[2] = pz + fr.bz;
}

// out: int32 head[8] = {goal flat index, goal_vxl[3], n_lookat, m, 0, 0}; double lookat_loc[m][3]; int32 lookat_idx[m];
// int32 lookat_vxl[m][3]; float lookat_val[m] -- slot r holds the entry of rank r.
__global__ __launch_bounds__(1024) void k_goal_search(uint32_t n_goals, uint32_t n_targets, const float* __restrict__ aggregated,
                                                      const float* __restrict__ collections, const int32_t* __restrict__ targets,
                                                      const int32_t* __restrict__ goal_idx, uint32_t m, GoalSearchFrame fr, int32_t* __restrict__ out) {
    __shared__ uint32_t s_key[kGoalSearchMaxTargets];
    __shared__ uint32_t s_whi[16], s_wlo[16];
    __shared__ uint32_t s_goal, s_positive;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;

    // (1) argmax: per thread the smallest (key, index) of its strided share, then the wave, then the workgroup
    uint32_t hi = 0xFFFFFFFFu, lo = 0xFFFFFFFFu;
    for (uint32_t g = tid; g < n_goals; g += blockDim.x) {
        const uint32_t key = ~sortable_key(aggregated[g]);
        if (key < hi || (key == hi && g < lo)) { hi = key; lo = g; }
    }
    wave_min_pair(hi, lo);
    if (lane == 0) { s_whi[wave] = hi; s_wlo[wave] = lo; }
    __syncthreads();
    if (wave == 0) {
        hi = lane < n_waves ? s_whi[lane] : 0xFFFFFFFFu;
        lo = lane < n_waves ? s_wlo[lane] : 0xFFFFFFFFu;
        wave_min_pair(hi, lo);
        if (lane == 0) { s_goal = lo; s_positive = 0u; }
    }
    __syncthreads();
    const uint32_t goal = s_goal;                                          // < n_goals: n_goals >= 1 and every index is below 2^32 - 1

    // (2) the goal's row: rank of entry k = how many entries come before it in (key, index) order
    const float* __restrict__ row = collections + (size_t)goal * n_targets;
    for (uint32_t k = tid; k < n_targets; k += blockDim.x) s_key[k] = ~sortable_key(row[k]);
    __syncthreads();
    double* __restrict__ loc = reinterpret_cast<double*>(out + kGoalSearchHeadInts);
    int32_t* __restrict__ idx = out + kGoalSearchHeadInts + 6u * m;
    int32_t* __restrict__ vxl = idx + m;
    float* __restrict__ val = reinterpret_cast<float*>(vxl + 3u * m);
    for (uint32_t k = tid; k < n_targets; k += blockDim.x) {
        const uint32_t mine = s_key[k];
        uint32_t rank = 0u;
        for (uint32_t j = 0u; j < n_targets && rank < m; ++j) {
            const uint32_t other = s_key[j];
            rank += (other < mine || (other == mine && j < k)) ? 1u : 0u;
        }
        if (rank < m) {
            const float v = row[k];
            const int32_t tx = targets[3u * k], ty = targets[3u * k + 1u], tz = targets[3u * k + 2u];
            idx[rank] = (int32_t)k;
            vxl[3u * rank] = tx; vxl[3u * rank + 1u] = ty; vxl[3u * rank + 2u] = tz;
            val[rank] = v;
            goal_search_loc(tx, ty, tz, fr, loc + 3u * rank);
            if (v > 0.0f) atomicAdd(&s_positive, 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        out[0] = (int32_t)goal;
        out[1] = goal_idx[3u * goal]; out[2] = goal_idx[3u * goal + 1u]; out[3] = goal_idx[3u * goal + 2u];
        out[4] = (int32_t)(s_positive > 0u ? s_positive : 1u);               // :502: max(#positive among the top m, 1)
        out[5] = (int32_t)m;
        out[6] = 0; out[7] = 0;
    }
}

}  // namespace naruto
