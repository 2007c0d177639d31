// Keyframe-anchored odometry prior: a ring of reference maps blocks chosen on the device (contract: naruto_amd/odometry.py,
// include/naruto_hip.h; numpy twin: tests/odometry_anchor_spec.py).  Every estimate of the frame-to-frame chain is composed onto the one
// before it, so its bias stays in the pose for good; here a frame is registered to one of `slots` kept frames and its pose is
// est[that frame] @ T.  Opt-in: no kernel of naruto_odom.hip changes, the kernels below call the bodies those kernels are made of.
//
//   k_odom_anchor_candidates    one thread: per slot the two starts inv(est[f_s]) @ est[i-1] @ M, M = identity / the last motion
//   k_odom_score_refs           odom_score_body<2, PHOTO> with blockIdx.y = the slot: previous maps = ring + s stride, candidates = slot s's pair
//   k_odom_score_refs_finish    one workgroup per slot: odom_score_finish_body<2>; an empty slot's sums are zeros
//   k_odom_anchor_choose        one thread: k_odom_choose's cost per (slot, start), the winner into the head, cands[2], the state, the records
//   k_odom_accumulate_anchored, k_odom_rgbd_accumulate_anchored, k_odom_score_anchored
//                               the level loop's and the level-0 score's bodies; the previous maps are resolved at entry from the head
//   k_odom_anchor_update        one thread: the promote decision from the verdict's record, the fail streak, the head's next slot
//   k_odom_anchor_promote       a copy of the current maps into the head's slot; every workgroup reads the decision word first
//   k_pose_predict_anchored     est[i] = est[f_chosen] @ T
//
// head: int32 [kOdomAnchorHead]: [0] the slot written last, [1] consecutive refused estimates, [2] the slot chosen for the current frame,
// [3] the promote decision of the current frame, [4 + s] slot s's frame id (-1 = empty).  No atomics, nothing waits on a device word.
#pragma once

#include "naruto_odom.hip"

namespace naruto {

constexpr int kOdomMaxRefs = 8;
constexpr int kOdomAnchorHead = 4 + kOdomMaxRefs;
constexpr int kOdomAnchorWords = 8;
constexpr int kOdomRefSums = 1 + 4 * 2;                                  // a K = 2 score per slot

// a slot word of the head, kept inside the ring whatever it holds
__device__ __forceinline__ uint32_t odom_anchor_slot(int32_t word, uint32_t slots) {
    const uint32_t s = (uint32_t)word;
    return s < slots ? s : slots - 1u;
}

// cands: [slots][2][16].  A slot that holds frame i-1 gets k_odom_candidates' two matrices (no inverse times itself); an empty slot too
__global__ __launch_bounds__(64) void k_odom_anchor_candidates(const float* __restrict__ est, uint32_t i, const int32_t* __restrict__ head, uint32_t slots,
                                                               double* __restrict__ cands) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double M[16], P[16];
    icp_identity(M);
    if (i > 1u) odom_last_motion(est, i, M);
    pose_load(est + 16 * (size_t)(i - 1u), P);
    for (uint32_t s = 0; s < slots; ++s) {
        const int32_t f = head[4 + s];
        double R[16], C1[16];
        if (f < 0 || (uint32_t)f >= i - 1u) {
            icp_identity(R);
#pragma unroll
            for (int k = 0; k < 16; ++k) C1[k] = M[k];
        } else {
            double F[16], Finv[16];
            pose_load(est + 16 * (size_t)f, F);
            pose_affine_inverse(F, Finv);
            pose_mul(Finv, P, R);
            pose_mul(R, M, C1);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { cands[32u * s + k] = R[k]; cands[32u * s + 16u + k] = C1[k]; }
    }
}

// grid (workgroups of the level, slots); part: [slots][parts][kOdomRefSums]; stride: floats between two blocks of the ring
template <bool PHOTO>
__global__ __launch_bounds__(kOdomThreads) void k_odom_score_refs(OdomLevel lv, uint32_t ioff, double max_dist2, double trunc2, double max_diff, uint64_t stride,
                                                                  uint32_t parts, const int32_t* __restrict__ head, const float* __restrict__ ring,
                                                                  const float* __restrict__ cur, const double* __restrict__ cands, double* __restrict__ part) {
    const uint32_t s = blockIdx.y;
    if (head[4 + s] < 0) return;                                         // uniform: an empty slot
    odom_score_body<2, PHOTO>(lv, ioff, max_dist2, trunc2, max_diff, ring + (size_t)s * stride, cur, cands + 32u * s, part + (size_t)s * parts * kOdomRefSums);
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_score_refs_finish(uint32_t parts, const int32_t* __restrict__ head, const double* __restrict__ part,
                                                                         double* __restrict__ sums) {
    const uint32_t s = blockIdx.x;
    if (head[4 + s] < 0) {
        if (threadIdx.x < (uint32_t)kOdomRefSums) sums[(size_t)s * kOdomRefSums + threadIdx.x] = 0.0;
        return;
    }
    odom_score_finish_body<2>(parts, part + (size_t)s * parts * kOdomRefSums, sums + (size_t)s * kOdomRefSums);
}

// sums: [slots][kOdomRefSums]; cands_all: [slots][2][16].  The lowest cost wins, ties go to the larger frame id, then to the lower start;
// no valid slot or every cost +inf: the slot written last, start 0.  anchor: [0] slot, [1] its frame id, [2] valid slots, [6] the best
// cost, [7] the runner-up (-1 where +inf), the rest 0 (k_odom_anchor_update's)
__global__ __launch_bounds__(64) void k_odom_anchor_choose(uint32_t slots, int32_t photo_on, double trunc, double photo_max_diff, const double* __restrict__ sums,
                                                           const double* __restrict__ cands_all, int32_t* __restrict__ head, double* __restrict__ cands,
                                                           double* __restrict__ state, double* __restrict__ record, double* __restrict__ anchor) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double best = (double)INFINITY, second = (double)INFINITY;
    int32_t bs = -1, bf = -1;
    uint32_t bk = 0u, valid = 0u;
    for (uint32_t s = 0; s < slots; ++s) {
        const int32_t f = head[4 + s];
        if (f < 0) continue;
        ++valid;
        const double* q = sums + (size_t)s * kOdomRefSums;
        for (uint32_t k = 0; k < 2u; ++k) {
            double c = odom_cost_term(q[0], q[1u + 4u * k], q[2u + 4u * k], trunc);
            if (photo_on) c = c + odom_cost_term(q[0], q[3u + 4u * k], q[4u + 4u * k], photo_max_diff);
            if (!(fabs(c) < (double)INFINITY)) c = (double)INFINITY;
            if (c < best || (c == best && c < (double)INFINITY && f > bf)) { second = best; best = c; bs = (int32_t)s; bf = f; bk = k; }
            else if (c < second) second = c;
        }
    }
    const uint32_t slot = bs >= 0 ? (uint32_t)bs : odom_anchor_slot(head[0], slots);
    const double* q = sums + (size_t)slot * kOdomRefSums;
    for (int k = 0; k < kOdomGateWords; ++k) record[k] = 0.0;
    record[1] = (double)bk;
    for (uint32_t k = 0; k < (uint32_t)kOdomMaxCands; ++k) {
        double c = -1.0;
        if (k < 2u) {
            c = odom_cost_term(q[0], q[1u + 4u * k], q[2u + 4u * k], trunc);
            if (photo_on) c = c + odom_cost_term(q[0], q[3u + 4u * k], q[4u + 4u * k], photo_max_diff);
            if (!(fabs(c) < (double)INFINITY)) c = (double)INFINITY;
        }
        record[2u + k] = c;
    }
    head[2] = (int32_t)slot;
    for (int k = 0; k < 32; ++k) cands[k] = cands_all[32u * slot + k];
    for (int k = 0; k < 16; ++k) state[k] = cands_all[32u * slot + 16u * bk + k];
    for (int k = 16; k < kOdomStateDoubles; ++k) state[k] = 0.0;
    anchor[0] = (double)slot;
    anchor[1] = (double)head[4 + slot];
    anchor[2] = (double)valid;
    anchor[3] = 0.0; anchor[4] = 0.0; anchor[5] = 0.0;
    anchor[6] = odom_finite_or(best, -1.0);
    anchor[7] = odom_finite_or(second, -1.0);
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_accumulate_anchored(OdomLevel lv, int32_t level, double max_dist2, uint64_t stride, uint32_t slots,
                                                                           const int32_t* __restrict__ head, const float* __restrict__ ring,
                                                                           const float* __restrict__ cur, const double* __restrict__ state,
                                                                           double* __restrict__ part) {
    odom_accumulate_body(lv, level, max_dist2, ring + (size_t)odom_anchor_slot(head[2], slots) * stride, cur, state, part, nullptr);
}

__global__ __launch_bounds__(kOdomThreads) void k_odom_rgbd_accumulate_anchored(OdomLevel lv, uint32_t ioff, int32_t level, double max_dist2, double weight,
                                                                                double max_diff, uint64_t stride, uint32_t slots,
                                                                                const int32_t* __restrict__ head, const float* __restrict__ ring,
                                                                                const float* __restrict__ cur, const double* __restrict__ state,
                                                                                double* __restrict__ part) {
    odom_rgbd_accumulate_body(lv, ioff, level, max_dist2, weight, max_diff, ring + (size_t)odom_anchor_slot(head[2], slots) * stride, cur, state, part, nullptr);
}

template <bool PHOTO>
__global__ __launch_bounds__(kOdomThreads) void k_odom_score_anchored(OdomLevel lv, uint32_t ioff, double max_dist2, double trunc2, double max_diff, uint64_t stride,
                                                                      uint32_t slots, const int32_t* __restrict__ head, const float* __restrict__ ring,
                                                                      const float* __restrict__ cur, const double* __restrict__ cands, double* __restrict__ part) {
    odom_score_body<1, PHOTO>(lv, ioff, max_dist2, trunc2, max_diff, ring + (size_t)odom_anchor_slot(head[2], slots) * stride, cur, cands, part);
}

struct OdomAnchor { double min_overlap, max_trans, min_trace; uint32_t slots, refail; };

// record: the verdict's, with T relative to the chosen reference.  A promoted frame takes the slot after the one written last; the head
// records it here, before k_odom_anchor_promote copies (which only reads the head).  anchor [3] promoted, [4] the slot written (-1 = none),
// [5] the fail streak after this frame
__global__ __launch_bounds__(64) void k_odom_anchor_update(OdomAnchor a, uint32_t i, const double* __restrict__ record, int32_t* __restrict__ head,
                                                           double* __restrict__ anchor) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool pass = record[0] == 1.0;
    const double valid = record[6], rows = record[7], t = record[9], trace = record[10];
    int32_t streak = head[1];
    bool promote;
    if (pass) {
        promote = rows < a.min_overlap * valid || t > a.max_trans || trace < a.min_trace;
        streak = 0;
    } else {
        streak = streak < 0 ? 1 : (streak < (int32_t)a.refail ? streak + 1 : (int32_t)a.refail);
        promote = (uint32_t)streak >= a.refail;
        if (promote) streak = 0;
    }
    int32_t written = -1;
    if (promote) {
        written = (int32_t)((odom_anchor_slot(head[0], a.slots) + 1u) % a.slots);
        head[0] = written;
        head[4 + written] = (int32_t)i;
    }
    head[1] = streak;
    head[3] = promote ? 1 : 0;
    anchor[3] = promote ? 1.0 : 0.0;
    anchor[4] = (double)written;
    anchor[5] = (double)streak;
}

// n: floats of a maps block.  float4 when the block size and both bases allow it (uniform), else float by float
__global__ __launch_bounds__(256) void k_odom_anchor_promote(uint64_t n, uint32_t slots, const int32_t* __restrict__ head, const float* __restrict__ cur,
                                                             float* __restrict__ ring) {
    if (head[3] == 0) return;                                            // uniform: not promoted
    float* dst = ring + (size_t)odom_anchor_slot(head[0], slots) * n;
    const uint64_t first = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
    if ((n & 3u) == 0u && (((uintptr_t)cur | (uintptr_t)ring) & 15u) == 0u) {
        const float4* src4 = reinterpret_cast<const float4*>(cur);
        float4* dst4 = reinterpret_cast<float4*>(dst);
        for (uint64_t k = first; k < n / 4u; k += step) dst4[k] = src4[k];
    } else {
        for (uint64_t k = first; k < n; k += step) dst[k] = cur[k];
    }
}

// est[i] = est[f] @ T with f = anchor[1], the chosen slot's frame id as k_odom_anchor_choose recorded it (anything outside 0 .. i-1 reads
// frame i-1); the rest is k_pose_predict_relative
__global__ __launch_bounds__(64) void k_pose_predict_anchored(float* est, uint32_t i, const double* __restrict__ anchor, const double* __restrict__ state_T,
                                                              float* __restrict__ pose6_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double f = anchor[1];
    const uint32_t ref = (f >= 0.0 && f < (double)i) ? (uint32_t)f : i - 1u;
    double A[16], T[16], N[16];
    pose_load(est + 16 * (size_t)ref, A);
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
