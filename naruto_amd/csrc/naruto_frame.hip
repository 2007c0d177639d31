// Frame ingest and keyframe row on the device: what a mapped frame needs between the simulator and the mapping loop.
//
//   ingest        current_rays = torch.cat([direction, rgb, depth[..., None]], -1).reshape(-1, 7) (reference coslam.py:306-308,
//                 keyframe.py:42-43) plus the count of pixels with a valid depth (keyframe.py:28, coslam.py:322) in ONE streaming launch;
//   keyframe row  KeyFrameDatabaseNaruto.add_keyframe (keyframe.py:38-60): num_rays_to_save distinct pixels of that buffer, tiled
//                 periodically when the frame has fewer, drawn with the keyed permutation of naruto_sample_distinct -- the population is
//                 read from the device word the ingest wrote, so no host value is needed in between.

#include "naruto_common.h"

namespace naruto {

constexpr uint32_t kFrameThreads = 256;

// One thread per OUTPUT word (grid-stride): the [n,7] rows are written as one contiguous stream, the three inputs are read in
// runs of 3 / 3 / 1 words.  Words move as uint32: every bit pattern (NaN payloads, -0) arrives unchanged.  The thread that moves a
// pixel's depth also tests it; the count is an integer sum -- wave partials, one LDS add per wave, ONE global integer atomic per
// workgroup -- so it does not depend on the launch plan.
__global__ __launch_bounds__(kFrameThreads) void k_frame_ingest(uint64_t n_words, const uint32_t* __restrict__ direction, const uint32_t* __restrict__ rgb,
                                                                 const uint32_t* __restrict__ depth, float depth_trunc, uint32_t* __restrict__ rays,
                                                                 unsigned long long* __restrict__ n_valid) {
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    uint32_t mine = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * kFrameThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kFrameThreads + threadIdx.x; e < n_words; e += stride) {
        const uint64_t p = e / 7u;
        const uint32_t c = (uint32_t)(e - p * 7u);
        uint32_t w;
        if (c < 3u) w = direction[3u * p + c];
        else if (c < 6u) w = rgb[3u * p + (c - 3u)];
        else {
            w = depth[p];
            const float d = __uint_as_float(w);
            mine += (d > 0.0f && d <= depth_trunc) ? 1u : 0u;          // NaN fails both comparisons: invalid
        }
        rays[e] = w;
    }
    const uint32_t wave_total = wave_sum_u32(mine);                     // every lane of the wave is here (no early return above)
    if ((threadIdx.x & 63u) == 0u && wave_total != 0u) atomicAdd(&s_count, wave_total);
    __syncthreads();
    if (threadIdx.x == 0 && s_count != 0u) atomicAdd(n_valid, (unsigned long long)s_count);
}

// Stored ray i = pixel perm(i mod n_take) of the population [0, n): n = *n_valid (the store's "reference" mode: the draw indexes the
// UNFILTERED pixel list) or n_pixels; n_take = min(n, rays_per_kf); n = 0 leaves the row as it is.
__global__ __launch_bounds__(kFrameThreads) void k_keyframe_row(const uint32_t* __restrict__ frame, uint64_t n_pixels, const unsigned long long* __restrict__ n_valid,
                                                                 uint32_t rays_per_kf, uint64_t key, uint32_t* __restrict__ row) {
    const uint32_t i = blockIdx.x * kFrameThreads + threadIdx.x;
    if (i >= rays_per_kf) return;
    uint64_t n = n_pixels;
    if (n_valid != nullptr) n = min((uint64_t)*n_valid, n_pixels);      // (a count can never exceed the frame: the clamp only guards the gather)
    if (n == 0) return;
    const uint32_t n_take = n < (uint64_t)rays_per_kf ? (uint32_t)n : rays_per_kf;
    const uint64_t j = perm_index(i % n_take, n, half_bits_for(n), key);
    const uint32_t* src = frame + j * 7u;
    uint32_t* dst = row + (size_t)i * 7u;
#pragma unroll
    for (int c = 0; c < 7; ++c) dst[c] = src[c];
}

}  // namespace naruto
