// extern "C" entry points of libnaruto_hip.so (see include/naruto_hip.h for the contract).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <unordered_set>
#include <vector>

#include "naruto_field.hip"
#include "naruto_binned.hip"
#include "naruto_render.hip"
#include "naruto_rays.hip"
#include "naruto_train.hip"
#include "naruto_sorted.hip"
#include "naruto_renderfused.hip"
#include "naruto_planner.hip"
#include "naruto_mesh.hip"
#include "naruto_parts.hip"
#include "naruto_pointgrad.hip"
#include "naruto_track.hip"
#include "naruto_bapose.hip"
#include "naruto_rrt.hip"
#include "naruto_recon.hip"
#include "naruto_cull.hip"
#include "naruto_subdiv.hip"
#include "naruto_sim.hip"
#include "naruto_frame.hip"
#include "naruto_posechain.hip"
#include "naruto_icp.hip"
#include "naruto_odom.hip"
#include "naruto_odom_anchor.hip"
#include "naruto_sdfreg.hip"
#include "naruto_view.hip"

using namespace naruto;

struct NarutoField {
    NarutoFieldDesc desc;
    LevelTab lt;
    UncertTab ut;
    BoxTab bt;
    uint32_t offset[NARUTO_MAX_LEVELS + 1];
    uint64_t n_entries;
    int n_cu;
    ScatterPlan plan;          // LDS-tiled scatter: the levels of up to kMaxChunksPerLevel chunks (a prefix of the levels)
    BinPlan bplan;             // binned scatter: the larger levels (the rest)
    uint64_t n_tiled_entries;  // entries of the LDS-tiled prefix = offset of the first larger level
};

namespace {

thread_local char g_err[512] = "";
unsigned long long* g_fwd_timeline = nullptr;       // profiling: naruto_debug_fwd_timeline
unsigned long long* g_bwd_timeline = nullptr;       // profiling: naruto_debug_bwd_timeline

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NARUTO_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return NARUTO_OK;
}

PointSrc make_points(const NarutoPoints* pts) {
    PointSrc ps{};
    ps.x = pts->x;
    ps.rays_o = pts->rays_o;
    ps.rays_d = pts->rays_d;
    ps.z_vals = pts->z_vals;
    ps.S = pts->n_samples ? pts->n_samples : 1u;
    return ps;
}

int check_points(const NarutoPoints* pts) {
    if (pts == nullptr) return fail(NARUTO_ERR_INVALID, "points: NULL");
    if (pts->x == nullptr && (pts->rays_o == nullptr || pts->rays_d == nullptr || pts->z_vals == nullptr || pts->n_samples == 0))
        return fail(NARUTO_ERR_INVALID, "points: give x, or rays_o + rays_d + z_vals + n_samples");
    return NARUTO_OK;
}

// The parameter tensors an entry point reads must be there: the encoding (table, uncertainty grid), the SDF net, the colour net.  `what` is the
// refusal's text after "<who>: ".
constexpr uint32_t kParamsEncoding = 1u, kParamsSdf = 2u, kParamsColour = 4u, kParamsAll = 7u;
int check_params(const NarutoParams* p, const char* who, uint32_t need = kParamsAll, const char* what = "NULL parameter") {
    const bool missing = ((need & kParamsEncoding) != 0u && (p->table == nullptr || p->uncert_grid == nullptr)) ||
                         ((need & kParamsSdf) != 0u && (p->sdf_w0 == nullptr || p->sdf_w1 == nullptr)) ||
                         ((need & kParamsColour) != 0u && (p->col_w0 == nullptr || p->col_w1 == nullptr));
    return missing ? fail(NARUTO_ERR_INVALID, "%s: %s", who, what) : NARUTO_OK;
}

uint32_t cu_count(const NarutoField* f) { return f->n_cu > 0 ? (uint32_t)f->n_cu : 256u; }

// a profiling / forcing knob of the environment; the sites keep it in a `static const`, so it is read once per process
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e != nullptr ? atoi(e) : dflt; }

inline size_t align_up(size_t b, size_t a = 256u) { return (b + a - 1u) / a * a; }

// The cursor every workspace layout is written with.  A layout function carves its sections from `base` in order and returns them with the
// total; over a NULL base the same walk only measures, which is what the naruto_*_workspace() function reports -- a layout is stated once.
// A section starts where the last one ended; `align` rounds its LENGTH up (1: the next section follows unpadded).
struct Carve {
    char* base;
    size_t off = 0;
    explicit Carve(void* b) : base(reinterpret_cast<char*>(b)) {}
    template <typename T> T* take(size_t bytes, size_t align = 256u) {
        T* p = base != nullptr ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up(bytes, align);
        return p;
    }
    size_t size() const { return off; }
};

// Dynamic LDS beyond the default limit is reserved per kernel, once per process: `latch` is set only after every kernel of the list has
// its bytes, so a failed reservation is tried again by the next call.  `what` heads the failure message and may print `told` (%zu).
struct LdsUse { const void* kernel; size_t bytes; };
template <typename K> LdsUse lds_use(K* kernel, size_t bytes) { return LdsUse{reinterpret_cast<const void*>(kernel), bytes}; }
int reserve_lds(bool& latch, std::initializer_list<LdsUse> uses, const char* what, size_t told = 0) {
    if (latch) return NARUTO_OK;
    for (const LdsUse& u : uses) {
        if (hipFuncSetAttribute(u.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)u.bytes) == hipSuccess) continue;
        char head[128];
        snprintf(head, sizeof(head), what, told);
        return fail(NARUTO_ERR_LAUNCH, "%s: %s", head, hipGetErrorString(hipGetLastError()));
    }
    latch = true;
    return NARUTO_OK;
}

// the stand-alone smoothness term over a lattice of n^3 cells: | features [n3][32] | one partial sum per 256 of them | pad |
struct TvWs { float* feat; double* partial; char* pad; size_t total; };
TvWs tv_ws(void* base, size_t n) {
    static_assert(kFeat * sizeof(float) % 64u == 0u, "the partial sums follow the features 64-byte aligned without a gap");
    const size_t n3 = n * n * n;
    Carve c(base);
    return {c.take<float>(n3 * kFeat * sizeof(float), 64u), c.take<double>((n3 * kFeat + 255u) / 256u * sizeof(double), 1u), c.take<char>(64u, 1u), c.size()};
}
// the point gradients of M ray samples (naruto_query_bwd_points, tracking, the BA pose step): | d_x [M][3] | pad |
struct PointGradWs { float* d_x; char* pad; size_t total; };
PointGradWs point_grad_ws(void* base, size_t M) {
    Carve c(base);
    return {c.take<float>(3u * sizeof(float) * M, 1u), c.take<char>(256u, 1u), c.size()};
}
// naruto_loss_sums: | per-ray terms [n_rays][16] |
struct LossWs { float* terms; size_t total; };
LossWs loss_ws(void* base, size_t n_rays) {
    Carve c(base);
    return {c.take<float>(n_rays * 16u * sizeof(float), 1u), c.size()};
}
// a top-K selection (k_ars_select) over n_keys keys: | keys [n_keys] | selected [K] | pad |.  A launch over fewer keys than the workspace
// was sized for packs its selection right behind them.
struct SelectWs { uint32_t* keys; uint32_t* sel; uint32_t* pad; size_t total; };
SelectWs select_ws(void* base, size_t n_keys, size_t K, size_t pad_words) {
    Carve c(base);
    return {c.take<uint32_t>(n_keys * sizeof(uint32_t), 1u), c.take<uint32_t>(K * sizeof(uint32_t), 1u), c.take<uint32_t>(pad_words * sizeof(uint32_t), 1u), c.size()};
}
constexpr size_t kArsPadWords = 16, kGoalPadWords = 64;

// leading dimension of the scatter's point list: a multiple of 4 so that every row (x [3][cap], d_feat [16][cap][2]) starts
// 16-byte aligned and the scatter can stream it with 16-byte loads
inline uint32_t list_cap(uint32_t n) { return (n + 3u) & ~3u; }

// k_query_fwd_loss keeps its weights (21 KB, static) next to the rays' images: two workgroups per CU up to this much dynamic LDS
constexpr size_t kFwdLossMaxRayLds = 48u * 1024u;       // S <= 384 samples per ray

// the per-ray kernels keep one ray per wave in dynamic LDS (kRayFields x S floats): allow the kMaxSamples case (128 KB)
int ray_lds_attr() {
    static bool done = false;
    const size_t bytes = ray_scratch_bytes(kMaxSamples);
    return reserve_lds(done,
                       {lds_use(k_composite_fwd, bytes), lds_use(k_composite_bwd<true>, bytes), lds_use(k_composite_bwd<false>, bytes), lds_use(k_loss_stage, bytes),
                        lds_use(k_loss_bwd_fused, bytes), lds_use(k_query_fwd_loss<false, false>, kFwdLossMaxRayLds), lds_use(k_query_fwd_loss<true, false>, kFwdLossMaxRayLds),
                        lds_use(k_query_fwd_loss<false, true>, kFwdLossMaxRayLds), lds_use(k_query_fwd_loss<true, true>, kFwdLossMaxRayLds),
                        lds_use(k_query_fwd_loss_short<false>, 16u * 1024u), lds_use(k_query_fwd_loss_short<true>, 16u * 1024u),
                        lds_use(k_query_fwd_loss_img, kFwdLossMaxRayLds), lds_use(k_query_fwd_loss_short_img, 16u * 1024u)},
                       "per-ray kernels: cannot reserve %zu bytes of LDS", bytes);
}

constexpr uint32_t kBwdMaxBlocks = 512;     // fp32: one 145 KB-LDS block per CU; bf16 mode: NARUTO_BWD_BF_MINWAVES 53 KB blocks per CU

// Point splits per level for a launch over a list of up to M points.  The plan's own counts (field_create) are an integer partition of
// the CUs for lists of a few hundred thousand points, where every workgroup is one round.  A long list is cut finer, so that the
// hardware's workgroup scheduler evens out the unit types over several rounds -- at 3.4 M points the hashed units (2 splits) took
// 3.4 ms while the dense units (4 splits) were done after 0.85 ms and their CUs idled.  Hashed levels only.  More splits cost partial tables (read
// once more each by the reduce), nothing else: the sums are fixed point.
inline uint32_t split_multiplier(uint32_t M) {
    static const int dbg = env_int("NARUTO_DEBUG_SCATTER_SPLIT_MULT", 0);      // profiling knob
    if (dbg > 0) return (uint32_t)dbg;
    return M > 1500000u ? 4u : 1u;            // measured (131 072 x 43 rays, T = 2^16): x2 no gain, x4 6.42 -> 5.70 ms; at 352 k / 554 k points x2 and x4 lose
}
inline LevelSplits level_splits(const NarutoField* f, uint32_t M) {
    LevelSplits ls;
    for (uint32_t mult = split_multiplier(M);; mult >>= 1) {
        uint32_t blocks = 0;
        for (int l = 0; l < kLevels; ++l) {
            // hashed levels only: the dense units are bound by their LDS adds and gain nothing from shorter shares (T = 2^22, where only
            // dense levels are tiled: 10.12 -> 10.63 ms with the multiplier on them)
            // (the long list's count is `mult` splits in all -- measured from a planned 1: x2 no gain, x4 6.42 -> 5.70 ms --, not mult
            // times whatever the one-round plan chose: 2 x 4 = 8 splits lost 7 % at 131 072 x 43 against 4)
            const uint32_t base = (uint32_t)f->plan.s_lvl[l];
            // (the dense levels of a long list take the most the partial tables allow: such a launch is several rounds of workgroups, and a
            // dense unit cut in 4 -- the one-round plan's count -- is a 1.9 ms workgroup at 131 072 x 43: the launch's whole time)
            const uint32_t s = mult > 1u ? (((f->lt.hashed >> l) & 1u) ? (base > mult ? base : mult) : 8u) : base;
            ls.s[l] = (uint8_t)(s > 8u ? 8u : s);
        }
        for (uint32_t u = 0; u < f->plan.n_dense + f->plan.n_hashed; ++u) blocks += ls.s[f->plan.level[u]];
        if (blocks <= (uint32_t)kMaxLevelBlocks || mult <= 1u) break;          // (field_create checked the plan's own counts)
    }
    return ls;
}
// the field's scatter plan with the splits of this launch and the workgroup -> (unit, split) table that goes with them
inline ScatterPlan scatter_plan(const NarutoField* f, uint32_t M) {
    ScatterPlan plan = f->plan;
    const LevelSplits ls = level_splits(f, M);
    memcpy(plan.s_lvl, ls.s, sizeof(plan.s_lvl));
    uint32_t nb = 0;
    for (uint32_t u = 0; u < plan.n_dense + plan.n_hashed; ++u) {
        const uint32_t sp = plan.s_lvl[plan.level[u]];
        for (uint32_t k = 0; k < sp && nb < (uint32_t)kMaxLevelBlocks; ++k, ++nb) {
            plan.blk_unit[nb] = (uint8_t)u;
            plan.blk_split[nb] = (uint8_t)k;
        }
    }
    plan.n_level_blocks = (uint16_t)nb;
    // a level's slice of the list (16 B per point and feature) stays in an XCD's 4 MB L2 up to ~300 k points
    static const int dbg_xcd = env_int("NARUTO_DEBUG_SCATTER_XCD_AWARE", -1);       // profiling knob
    plan.xcd_aware = (uint8_t)(dbg_xcd >= 0 ? (dbg_xcd != 0) : (M <= 300000u));
    static const int dbg_cyc = env_int("NARUTO_DEBUG_SCATTER_CYCLIC", -1);             // profiling knob
    plan.cyclic = (uint8_t)(dbg_cyc >= 0 ? (dbg_cyc != 0) : (M <= 300000u));
    return plan;
}

// rows of the binned scatter's count matrix: one per kBinRound points, at most kBinMaxRows
inline uint32_t bin_rows(uint32_t M) {
    const uint32_t r = (M + (uint32_t)kBinRound - 1u) / (uint32_t)kBinRound;
    return r < 1u ? 1u : (r > (uint32_t)kBinMaxRows ? (uint32_t)kBinMaxRows : r);
}

// workspace of the table scatter for a list of up to M points: | tiled partial tables | counts | totals | starts | items |
struct ScatterWs {
    float* partial; float* unc_partial; uint32_t* counts; uint32_t* totals; uint32_t* starts; BinItem* items;
    size_t total;
};
// entries per feature plane of a partial table: the tiled levels
inline size_t partial_plane(const NarutoField* f) { return (size_t)f->n_tiled_entries; }
// the uncertainty grid's units: point splits per chunk for a list of up to M points -- the planned count for the mapping batches
// (workgroup budget), more for long lists (a unit should not stream more than ~100 k active points), at most kMaxUncertSplits
constexpr uint32_t kMaxUncertSplits = 32;
inline uint32_t uncert_splits(const NarutoField* f, uint32_t M) {
    uint32_t s = (M + 262143u) / 262144u;             // M is the list's CAPACITY (all samples); about a third of it carries a cotangent
    if (s < f->plan.s_uncert) s = f->plan.s_uncert;
    // (long lists raise the count above the one-round plan's only while the grid's units stay few; the plan's own count -- chosen against the
    // launch's budget of workgroups, field_create -- always stands: MP3D's 57-chunk grid had been cut back to ONE split here, 57 workgroups of
    // 183 us next to 63 idle CUs)
    uint32_t cap = f->plan.n_uncert ? (64u / f->plan.n_uncert > 1u ? 64u / f->plan.n_uncert : 1u) : 1u;
    if (cap < f->plan.s_uncert) cap = f->plan.s_uncert;
    if (s > cap) s = cap;
    if (s > kMaxUncertSplits) s = kMaxUncertSplits;
    return s < 1u ? 1u : s;
}
inline uint32_t uncert_pad(const NarutoField* f) { return (f->plan.uncert_voxels + 3u) / 4u * 4u; }

ScatterWs scatter_ws(const NarutoField* f, void* base, uint32_t M) {
    ScatterWs w{};
    Carve c(base);
    uint32_t smax = 1;
    const LevelSplits ls_ = level_splits(f, M);
    for (int l = 0; l < kLevels; ++l) smax = ls_.s[l] > smax ? ls_.s[l] : smax;
    w.partial = c.take<float>((f->plan.n_dense + f->plan.n_hashed) ? (size_t)smax * partial_plane(f) * 2u * sizeof(float) : 16u);
    w.unc_partial = c.take<float>(f->plan.n_uncert ? (size_t)uncert_splits(f, M) * uncert_pad(f) * sizeof(float) : 16u);
    if (f->bplan.n_levels != 0) {
        w.counts = c.take<uint32_t>((size_t)bin_rows(M) * f->bplan.n_bins * sizeof(uint32_t));
        w.totals = c.take<uint32_t>((size_t)f->bplan.n_bins * sizeof(uint32_t));
        w.starts = c.take<uint32_t>(((size_t)f->bplan.n_bins + 1u) * sizeof(uint32_t));
        w.items = c.take<BinItem>((size_t)M * f->bplan.n_levels * kBinItemsPerPoint * sizeof(BinItem));
    }
    w.total = c.size();
    return w;
}

// table scatter.  Levels of up to kMaxChunksPerLevel chunks: LDS-tiled units (+ k_scatter_reduce unless the caller finishes the
// gradient itself); larger levels: the binned scatter (naruto_binned.hip), whose last kernel writes / adds the gradient slice or,
// with ``adam``, steps the optimiser on it.  (Debug: NARUTO_DEBUG_SCATTER_ATOMIC=1 sends the larger levels through global
// float atomics instead -- for A/B timing only.)
// unc_g / d_uncert (both or neither; training list layout only): row 3 of the point list and the grid's gradient it is scattered into
int launch_scatter(const NarutoField* f, const PointSrc& ps, uint32_t M, const float* d_feat, size_t stride_m, size_t stride_l, float* d_table,
                   void* workspace, hipStream_t st, const uint32_t* m_dev = nullptr, const float* scale_dev = nullptr, int overwrite = 0,
                   bool do_reduce = true, const AdamFuse* adam = nullptr, const float* unc_g = nullptr, float* d_uncert = nullptr, uint32_t unc_first = 0) {
    if ((overwrite || adam != nullptr) && f->plan.atomic_levels != 0)
        return fail(NARUTO_ERR_INVALID, "scatter: written (not accumulated) gradients / the fused optimiser are not available with NARUTO_DEBUG_SCATTER_ATOMIC");
    const ScatterWs w = scatter_ws(f, workspace, M);
    const size_t n_tiled_params = (size_t)f->n_tiled_entries * 2u;
    const size_t n_plane = partial_plane(f);
    UncertScatter us{};
    UncertReduce ur{};
    if (unc_g != nullptr && d_uncert != nullptr && f->plan.n_uncert != 0) {
        us.g = unc_g; us.ut = f->ut; us.partial = w.unc_partial; us.voxels_pad = uncert_pad(f); us.n_splits = uncert_splits(f, M); us.first = unc_first & ~3u;
        ur.d_uncert = d_uncert; ur.partial = w.unc_partial; ur.n_voxels = f->plan.uncert_voxels; ur.n_splits = us.n_splits; ur.voxels_pad = us.voxels_pad;
    }
    if (d_table == nullptr && adam == nullptr && us.g == nullptr) return NARUTO_OK;
    ScatterPlan plan = scatter_plan(f, M);
    if (d_table == nullptr && adam == nullptr) { plan.n_dense = plan.n_hashed = 0; plan.n_level_blocks = 0; }        // only the uncertainty grid's gradient is wanted
    if (f->plan.n_dense + f->plan.n_hashed > 0) {
        static bool attr_set = false;
        const size_t lds = kScatterLdsBytes;
        if (!attr_set) {
            // the hashed units' list visit addresses the image from LDS offset 0 (the contract at `acc` in k_hash_scatter_lds): static LDS in
            // the kernel would put the dynamic allocation behind it, and the visit would add into whatever lies at the front
            hipFuncAttributes fa{};
            if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_hash_scatter_lds)) != hipSuccess)
                return fail(NARUTO_ERR_LAUNCH, "hash_scatter: cannot read the kernel's attributes: %s", hipGetErrorString(hipGetLastError()));
            if (fa.sharedSizeBytes != 0)
                return fail(NARUTO_ERR_LAUNCH, "hash_scatter: k_hash_scatter_lds has %zu bytes of static LDS; its image must start at LDS offset 0", (size_t)fa.sharedSizeBytes);
        }
        if (int rc = reserve_lds(attr_set, {lds_use(k_hash_scatter_lds, lds)}, "hash_scatter: cannot reserve %zu bytes of LDS", lds)) return rc;
        const uint32_t blocks = ((uint32_t)plan.n_level_blocks + (us.g != nullptr ? plan.n_uncert * us.n_splits : 0u) + 7u) / 8u * 8u;      // XCD-aware order: multiple of 8
        hipLaunchKernelGGL(k_hash_scatter_lds, dim3(blocks), dim3(kScatterThreads), lds, st, f->lt, f->bt, ps, M, d_feat, stride_m, stride_l, plan,
                           w.partial, 2u * n_plane, m_dev, scale_dev, us, g_fwd_timeline);
        if (int rc = check_launch("hash_scatter_lds")) return rc;
        if (do_reduce) {
            const uint32_t n_table_blocks = d_table != nullptr ? (uint32_t)((n_tiled_params / 4u + 255u) / 256u) : 0u;
            const uint32_t n_unc_blocks = ur.d_uncert != nullptr ? (ur.n_voxels + 255u) / 256u : 0u;
            if (n_table_blocks + n_unc_blocks > 0) {
                hipLaunchKernelGGL(k_scatter_reduce, dim3(n_table_blocks + n_unc_blocks), dim3(256), 0, st, f->lt, f->plan.atomic_levels, w.partial,
                                   level_splits(f, M), n_tiled_params, n_plane, d_table, overwrite, n_table_blocks, ur);
                if (int rc = check_launch("scatter_reduce")) return rc;
            }
        }
    }
    if (f->bplan.n_levels != 0 && (d_table != nullptr || adam != nullptr)) {
        // the binned scatter's counts, prefix sums and item offsets are 32-bit: 8 items per (list point, binned level)
        if ((uint64_t)M * kBinItemsPerPoint * f->bplan.n_levels >= (1ull << 32))
            return fail(NARUTO_ERR_INVALID, "scatter: %u list points x %u binned levels x 8 items overflow the 32-bit item offsets (split the batch)", M, f->bplan.n_levels);
        uint32_t nb_max = 0;
        for (uint32_t k = 0; k < f->bplan.n_levels; ++k) nb_max = f->bplan.bin0[k + 1] - f->bplan.bin0[k] > nb_max ? f->bplan.bin0[k + 1] - f->bplan.bin0[k] : nb_max;
        static const bool force_512 = env_int("NARUTO_DEBUG_BIN_ROUND", 0) == 512;      // same bits: fixed-point sums
        const bool round_1024 = !force_512 && bin_fill_lds_bytes(1024u, nb_max) <= (size_t)160u * 1024u;            // else 512-point rounds (T = 2^24)
        static bool attr_set = false;
        if (int rc = reserve_lds(attr_set,
                                 {lds_use(k_bin_fill<1024>, 160u * 1024u), lds_use(k_bin_fill<512>, bin_fill_lds_bytes(512u, (uint32_t)kMaxBinsPerLevel)),
                                  lds_use(k_bin_apply, 2u * kBinEntries * sizeof(unsigned long long))},
                                 "binned scatter: cannot reserve LDS"))
            return rc;
        const BinPlan& bp = f->bplan;
        const uint32_t rows = bin_rows(M);
        hipLaunchKernelGGL(k_bin_count, dim3(rows, bp.n_levels), dim3(kBinThreads), 0, st, f->lt, f->bt, ps, M, d_feat, stride_m, stride_l, bp, w.counts, m_dev);
        if (int rc = check_launch("bin_count")) return rc;
        hipLaunchKernelGGL(k_bin_colscan, dim3((bp.n_bins + 255u) / 256u), dim3(256), 0, st, w.counts, rows, bp.n_bins, w.totals);
        if (int rc = check_launch("bin_colscan")) return rc;
        hipLaunchKernelGGL(k_bin_start, dim3(1), dim3(1024), 0, st, w.totals, bp.n_bins, w.starts);
        if (int rc = check_launch("bin_start")) return rc;
        if (round_1024)
            hipLaunchKernelGGL(k_bin_fill<1024>, dim3(rows, bp.n_levels), dim3(1024), bin_fill_lds_bytes(1024u, nb_max), st, f->lt, f->bt, ps, M, d_feat, stride_m, stride_l,
                               bp, nb_max, w.counts, w.starts, w.items, m_dev);
        else
            hipLaunchKernelGGL(k_bin_fill<512>, dim3(rows, bp.n_levels), dim3(512), bin_fill_lds_bytes(512u, nb_max), st, f->lt, f->bt, ps, M, d_feat, stride_m, stride_l,
                               bp, nb_max, w.counts, w.starts, w.items, m_dev);
        if (int rc = check_launch("bin_fill")) return rc;
        AdamFuse none{};
        hipLaunchKernelGGL(k_bin_apply, dim3(bp.n_bins), dim3(kBinApplyThreads), 2u * kBinEntries * sizeof(unsigned long long), st, f->lt, bp, w.starts, w.items,
                           d_table, overwrite, scale_dev, adam != nullptr ? *adam : none);
        if (int rc = check_launch("bin_apply")) return rc;
    }
    if (f->plan.atomic_levels != 0 && d_table != nullptr) {
        hipLaunchKernelGGL(k_hash_scatter_atomic, dim3((M + 255u) / 256u, kLevels), dim3(256), 0, st, f->lt, f->bt, ps, M, d_feat, stride_m, stride_l,
                           f->plan.atomic_levels, d_table, m_dev, scale_dev);
        if (int rc = check_launch("hash_scatter_atomic")) return rc;
    }
    return NARUTO_OK;
}

}  // namespace

extern "C" {

const char* naruto_last_error(void) { return g_err; }
int naruto_version(void) { return 1; }

int naruto_field_create(const NarutoFieldDesc* d, NarutoField** out) {
    if (d == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "create: NULL argument");
    if (d->n_levels != kLevels || d->n_features != 2)
        return fail(NARUTO_ERR_INVALID, "create: this build supports n_levels=16, n_features=2 (got %u, %u)", d->n_levels, d->n_features);
    if (d->n_bins != kBins || d->hidden_dim != kHidden || d->hidden_dim_color != kHidden || d->geo_feat_dim != kGeo)
        return fail(NARUTO_ERR_INVALID, "create: this build supports n_bins=16, hidden_dim=32, hidden_dim_color=32, geo_feat_dim=15");
    if (d->log2_hashmap_size < 4 || d->log2_hashmap_size > 24) return fail(NARUTO_ERR_INVALID, "create: log2_hashmap_size out of range");
    if (d->uncert_dims[0] == 0 || d->uncert_dims[1] == 0 || d->uncert_dims[2] == 0) return fail(NARUTO_ERR_INVALID, "create: empty uncert grid");
    if (d->uncert_dims[0] > 1000 || d->uncert_dims[1] > 1000 || d->uncert_dims[2] > 1000) return fail(NARUTO_ERR_INVALID, "create: uncert grid axes of more than 1000 voxels are not supported");
    if (!(d->trunc > 0.0f)) return fail(NARUTO_ERR_INVALID, "create: trunc must be > 0");
    if (d->mlp_mode != NARUTO_MLP_FP32 && d->mlp_mode != NARUTO_MLP_BF16) return fail(NARUTO_ERR_INVALID, "create: unknown mlp_mode %u", d->mlp_mode);
    NarutoField* f = new (std::nothrow) NarutoField;
    if (f == nullptr) return fail(NARUTO_ERR_INVALID, "create: out of memory");
    f->desc = *d;
    // tcnn GridEncodingTemplated constructor: per-level scale / resolution / size / offset
    const float log2_pls = std::log2(d->per_level_scale);
    uint64_t offset = 0;
    f->lt.hashed = 0;
    for (uint32_t l = 0; l < d->n_levels; ++l) {
        const float scale = exp2f((float)l * log2_pls) * (float)d->base_resolution - 1.0f;
        const uint32_t res = (uint32_t)ceilf(scale) + 1u;
        const uint32_t max_params = 0xFFFFFFFFu / 2u;
        const double dense = (double)res * (double)res * (double)res;
        uint64_t params = powf((float)res, 3.0f) > (float)max_params ? (uint64_t)max_params : (uint64_t)dense;
        params = (params + 7u) / 8u * 8u;
        const uint64_t cap = 1ull << d->log2_hashmap_size;
        if (params > cap) params = cap;
        // grid_index(): the spatial hash is used iff the level's size is smaller than res^3
        const bool hashed = (double)params < dense;
        if (hashed) f->lt.hashed |= 1u << l;
        f->lt.scale[l] = scale;
        f->lt.res[l] = res;
        f->lt.size[l] = (uint32_t)params;
        f->lt.magic[l] = 0xFFFFFFFFu / (uint32_t)params;
        f->lt.off[l] = (uint32_t)offset;
        f->offset[l] = (uint32_t)offset;
        offset += params;
        if (offset > 0x7FFFFFFFull) { delete f; return fail(NARUTO_ERR_INVALID, "create: hash table too large for 32-bit entry offsets"); }
    }
    f->offset[d->n_levels] = (uint32_t)offset;
    f->n_entries = offset;
    f->ut.D = (int32_t)d->uncert_dims[0];
    f->ut.H = (int32_t)d->uncert_dims[1];
    f->ut.W = (int32_t)d->uncert_dims[2];
    for (int i = 0; i < 3; ++i) {
        f->bt.bmin[i] = d->bbox_min[i];
        f->bt.bext[i] = d->bbox_max[i] - d->bbox_min[i];
    }
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) f->n_cu = cus;
    else { f->n_cu = 0; (void)hipGetLastError(); }
    // scatter plan: levels of up to kMaxChunksPerLevel 16 384-entry chunks are LDS-tiled, one unit per (chunk, feature),
    // dense levels first; larger levels use global atomics
    memset(&f->plan, 0, sizeof(f->plan));
    memset(&f->bplan, 0, sizeof(f->bplan));
    uint32_t n_units = 0, big_levels = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t l = 0; l < d->n_levels; ++l) {
            const bool hashed = (f->lt.hashed >> l) & 1u;
            if ((pass == 1) != hashed) continue;
            const uint32_t chunks = (f->lt.size[l] + kChunk - 1u) / kChunk;
            if (chunks > (uint32_t)kMaxChunksPerLevel) { big_levels |= 1u << l; continue; }
            for (uint32_t c = 0; c < chunks; ++c) {
                for (uint32_t ft = 0; ft < 2u; ++ft) {
                    f->plan.level[n_units] = (uint8_t)l;
                    f->plan.chunk[n_units] = (uint8_t)(c | (ft << 7));
                    ++n_units;
                }
            }
            if (hashed) f->plan.n_hashed += 2u * chunks; else f->plan.n_dense += 2u * chunks;
        }
    }
    // the larger levels (a suffix of the levels: sizes never decrease) go through the binned scatter
    f->n_tiled_entries = f->n_entries;
    if (big_levels != 0) {
        uint32_t first = 0;
        while (!((big_levels >> first) & 1u)) ++first;
        if (big_levels != ((0xFFFFFFFFu << first) & ((1u << d->n_levels) - 1u))) { delete f; return fail(NARUTO_ERR_INVALID, "create: level sizes are not monotone"); }
        f->n_tiled_entries = f->offset[first];
        if (getenv("NARUTO_DEBUG_SCATTER_ATOMIC") != nullptr) {
            f->plan.atomic_levels = big_levels;
        } else {
            BinPlan& bp = f->bplan;
            bp.level_mask = big_levels;
            bp.first_level = first;
            bp.n_levels = d->n_levels - first;
            uint32_t nb = 0;
            for (uint32_t k = 0; k < bp.n_levels; ++k) {
                const uint32_t bins = (f->lt.size[first + k] + kBinEntries - 1u) / kBinEntries;
                if (bins > (uint32_t)kMaxBinsPerLevel) { delete f; return fail(NARUTO_ERR_INVALID, "create: log2_hashmap_size > 24 is not supported by the table scatter"); }
                bp.bin0[k] = nb;
                nb += bins;
            }
            bp.bin0[bp.n_levels] = nb;
            bp.n_bins = nb;
        }
    }
    // one 128 KB-LDS workgroup per CU and every workgroup takes about the same time (it is bound by the points it
    // streams, not by its unit): never launch more workgroups than CUs (a second round doubles the kernel time).  About
    // 70 % of the CUs go to the hashed units, the rest to the dense ones (measured optimum on MI355X: 2 x 88 + 5 x 16).
    {
        // the uncertainty grid rides along as 16 384-voxel units (grids beyond kMaxUncertChunks chunks keep float atomics in k_query_bwd)
        const uint64_t vox = (uint64_t)d->uncert_dims[0] * d->uncert_dims[1] * d->uncert_dims[2];
        const uint64_t uch = (vox + kChunk - 1u) / kChunk;
        if (uch <= (uint64_t)kMaxUncertChunks && vox < 0x7FFFFFFFull) {
            f->plan.n_uncert = (uint32_t)uch;
            f->plan.uncert_voxels = (uint32_t)vox;
            f->plan.s_uncert = uch <= 8u ? 2u : 1u;
        }
        const uint32_t cus = cu_count(f);
        // Point splits per level and for the grid's chunks (round 5; it was "70 % of the CUs to the hashed units, the rest to the dense
        // ones", one count per unit type).  A workgroup's time is its share of the list times what a visit costs in its unit type --
        // measured per workgroup with tools/scatter_timeline.py at the headline batch (123 k list points; relative to a hashed unit's
        // visit, hashed_corner_addr8 form): dense levels 1.75 (every point applies all eight corners, same-address conflicts), the
        // uncertainty grid 1.1 over the 3/4 of the list behind the lattice -- and the launch ends with its slowest workgroup.  So: start
        // from one split each and keep giving one more to whatever is slowest while the workgroups still fit the CUs in ONE round.
        {
            float cost[kLevels + 1];                 // per unit of level l; [kLevels]: per chunk of the uncertainty grid
            uint32_t units[kLevels + 1] = {}, sp[kLevels + 1];
            for (uint32_t u = 0; u < f->plan.n_dense + f->plan.n_hashed; ++u) ++units[f->plan.level[u]];
            units[kLevels] = f->plan.n_uncert;
            for (uint32_t l = 0; l <= (uint32_t)kLevels; ++l) {
                sp[l] = 1u;
                cost[l] = l == (uint32_t)kLevels ? 1.1f : (((f->lt.hashed >> l) & 1u) ? 1.0f : 1.75f);
            }
            uint32_t used = 0;
            for (uint32_t l = 0; l <= (uint32_t)kLevels; ++l) used += units[l];
            bool full[kLevels + 1] = {};             // one more split of this type would not fit any more
            for (;;) {
                int worst = -1;
                for (uint32_t l = 0; l <= (uint32_t)kLevels; ++l)
                    if (units[l] != 0u && sp[l] < 8u && !full[l] && (worst < 0 || cost[l] / (float)sp[l] > cost[worst] / (float)sp[worst])) worst = (int)l;
                if (worst < 0) break;
                // (a type that no longer fits is also the one the launch waits for: speeding up the others buys nothing, stop there --
                // unless the others are within 10 % of it, where a finer cut of THEM still trims the tail)
                if (used + units[worst] > cus) { full[worst] = true; continue; }
                bool slowest_is_full = false;
                for (uint32_t l = 0; l <= (uint32_t)kLevels; ++l)
                    if (full[l] && cost[l] / (float)sp[l] > 1.1f * cost[worst] / (float)sp[worst]) slowest_is_full = true;
                if (slowest_is_full) break;
                used += units[worst];
                ++sp[worst];
            }
            for (uint32_t l = 0; l < (uint32_t)kLevels; ++l) f->plan.s_lvl[l] = (uint8_t)sp[l];
            f->plan.s_uncert = f->plan.n_uncert ? sp[kLevels] : 1u;
            uint32_t sh = 1u, sd = 1u;                   // (the defaults the per-type knobs below start from)
            for (uint32_t l = 0; l < (uint32_t)kLevels; ++l) {
                if (!units[l]) continue;
                if ((f->lt.hashed >> l) & 1u) sh = sp[l]; else sd = sp[l];
            }
            f->plan.s_hashed = sh;
            f->plan.s_dense = sd;
        }
        // profiling knobs (performance only: the split counts change the summation order, nothing else)
        if (const char* e1 = getenv("NARUTO_DEBUG_SCATTER_SPLITS_HASHED")) f->plan.s_hashed = (uint32_t)atoi(e1) < 1 ? 1u : ((uint32_t)atoi(e1) > 8u ? 8u : (uint32_t)atoi(e1));
        f->plan.role_mask = 7u;
        if (const char* e0 = getenv("NARUTO_DEBUG_SCATTER_ROLES")) f->plan.role_mask = (uint32_t)atoi(e0);
        if (const char* e3 = getenv("NARUTO_DEBUG_SCATTER_SPLITS_UNCERT")) { const uint32_t v = (uint32_t)atoi(e3); f->plan.s_uncert = v < 1u ? 1u : (v > 8u ? 8u : v); }
        if (const char* e2 = getenv("NARUTO_DEBUG_SCATTER_SPLITS_DENSE")) f->plan.s_dense = (uint32_t)atoi(e2) < 1 ? 1u : ((uint32_t)atoi(e2) > 8u ? 8u : (uint32_t)atoi(e2));
        for (uint32_t l = 0; l < (uint32_t)kLevels; ++l) {
            if (((f->lt.hashed >> l) & 1u) && getenv("NARUTO_DEBUG_SCATTER_SPLITS_HASHED") != nullptr) f->plan.s_lvl[l] = (uint8_t)f->plan.s_hashed;
            if (!((f->lt.hashed >> l) & 1u) && getenv("NARUTO_DEBUG_SCATTER_SPLITS_DENSE") != nullptr) f->plan.s_lvl[l] = (uint8_t)f->plan.s_dense;
        }
        // NARUTO_DEBUG_SCATTER_SPLITS_LEVELS="l:s,l:s,...": per-level override
        if (const char* e4 = getenv("NARUTO_DEBUG_SCATTER_SPLITS_LEVELS")) {
            const char* q = e4;
            while (*q) {
                char* end = nullptr;
                const long l = strtol(q, &end, 10);
                if (end == q || *end != ':') break;
                q = end + 1;
                const long v = strtol(q, &end, 10);
                if (end == q) break;
                if (l >= 0 && l < kLevels && v >= 1 && v <= 8) f->plan.s_lvl[l] = (uint8_t)v;
                q = *end == ',' ? end + 1 : end;
            }
        }
        uint32_t nb = 0;
        for (uint32_t u = 0; u < f->plan.n_dense + f->plan.n_hashed; ++u) {
            const uint32_t s = f->plan.s_lvl[f->plan.level[u]];
            for (uint32_t k = 0; k < s; ++k, ++nb) {
                if (nb >= (uint32_t)kMaxLevelBlocks) { delete f; return fail(NARUTO_ERR_INVALID, "field_create: scatter plan exceeds its workgroup table"); }
                f->plan.blk_unit[nb] = (uint8_t)u;
                f->plan.blk_split[nb] = (uint8_t)k;
            }
        }
        f->plan.n_level_blocks = (uint16_t)nb;
        if (getenv("NARUTO_DEBUG_PLAN") != nullptr) {
            fprintf(stderr, "naruto scatter plan: %u dense + %u hashed units, %u uncertainty chunks x %u; splits per level:", f->plan.n_dense, f->plan.n_hashed, f->plan.n_uncert, f->plan.s_uncert);
            for (int l = 0; l < kLevels; ++l) fprintf(stderr, " %u%s", (unsigned)f->plan.s_lvl[l], ((f->lt.hashed >> l) & 1u) ? "h" : "d");
            fprintf(stderr, "; %u level workgroups\n", nb);
        }
    }
    *out = f;
    return NARUTO_OK;
}

void naruto_field_destroy(NarutoField* f) { delete f; }

int naruto_field_levels(const NarutoField* f, float* scale, uint32_t* resolution, uint32_t* size, uint32_t* offset) {
    if (f == nullptr) return fail(NARUTO_ERR_INVALID, "levels: NULL field");
    for (uint32_t l = 0; l < f->desc.n_levels; ++l) {
        if (scale) scale[l] = f->lt.scale[l];
        if (resolution) resolution[l] = f->lt.res[l];
        if (size) size[l] = f->lt.size[l];
        if (offset) offset[l] = f->offset[l];
    }
    if (offset) offset[f->desc.n_levels] = f->offset[f->desc.n_levels];
    return NARUTO_OK;
}

uint64_t naruto_field_n_entries(const NarutoField* f) { return f ? f->n_entries : 0; }

int naruto_sample_z(uint32_t n_rays, const float* target_d, float near_, float far_, uint32_t n_samples_d, uint32_t n_range_d,
                    float range_d, uint32_t n_samples, const float* rand, float* z_vals, void* stream) {
    if (z_vals == nullptr) return fail(NARUTO_ERR_INVALID, "sample_z: NULL output");
    if (n_rays == 0) return NARUTO_OK;
    uint32_t nu, nr;
    if (target_d != nullptr) { nu = n_samples_d; nr = n_range_d; }
    else { nu = n_samples; nr = 0; }
    const uint32_t S = nu + nr;
    if (S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "sample_z: need 2 <= samples per ray <= %d (got %u)", kMaxSamples, S);
    hipLaunchKernelGGL(k_sample_z, dim3(n_rays), dim3(64), 0, (hipStream_t)stream, n_rays, target_d, near_, far_, nu, nr, range_d, rand,
                       static_cast<const uint64_t*>(nullptr), z_vals);
    return check_launch("sample_z");
}

int naruto_hash_encode_fwd(const NarutoField* f, uint32_t M, const float* x, const float* table, float* feat, void* stream) {
    if (f == nullptr || table == nullptr) return fail(NARUTO_ERR_INVALID, "hash_encode_fwd: NULL argument");
    if (M == 0) return NARUTO_OK;                     // empty batch: its (NULL) point and feature pointers are not an error
    if (x == nullptr || feat == nullptr) return fail(NARUTO_ERR_INVALID, "hash_encode_fwd: NULL argument");
    hipLaunchKernelGGL(k_hash_encode_fwd, dim3((M + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, f->lt, x,
                       reinterpret_cast<const float2*>(table), M, feat);
    return check_launch("hash_encode_fwd");
}

int naruto_oneblob_fwd(const NarutoField* f, uint32_t M, const float* x, float* out, void* stream) {
    if (f == nullptr || x == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "oneblob_fwd: NULL argument");
    if (M == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_oneblob_fwd, dim3((M + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, M, x, out);
    return check_launch("oneblob_fwd");
}

int naruto_uncert_sample(const NarutoField* f, uint32_t M, const float* x, const float* uncert_grid, float* out, void* stream) {
    if (f == nullptr || x == nullptr || uncert_grid == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "uncert_sample: NULL argument");
    if (M == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_uncert_sample, dim3((M + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, f->ut, M, x, uncert_grid, out);
    return check_launch("uncert_sample");
}

int naruto_decoder_fwd(const NarutoField* f, const NarutoParams* p, uint32_t M, int part, const float* a, const float* b, float* out, void* stream) {
    if (f == nullptr || p == nullptr || a == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "decoder_fwd: NULL argument");
    if (part < 0 || part > 2) return fail(NARUTO_ERR_INVALID, "decoder_fwd: part must be NARUTO_DECODER_FULL, _SDF_NET or _COLOR_NET");
    if (part == NARUTO_DECODER_FULL && b == nullptr) return fail(NARUTO_ERR_INVALID, "decoder_fwd: the full decoder takes embed and embed_pos");
    if (p->sdf_w0 == nullptr || p->sdf_w1 == nullptr || p->col_w0 == nullptr || p->col_w1 == nullptr) return fail(NARUTO_ERR_INVALID, "decoder_fwd: NULL weights");
    if (M == 0) return NARUTO_OK;
    const uint32_t lda = part == NARUTO_DECODER_FULL ? 1u + kFeat : (part == NARUTO_DECODER_SDF_NET ? 1u + kFeat + kPos : (uint32_t)kInCol);
    hipLaunchKernelGGL(k_decoder_parts, dim3((M + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, M, part, a, lda, b, (uint32_t)kPos, *p, out);
    return check_launch("decoder_fwd");
}

size_t naruto_scatter_workspace(const NarutoField* f, uint32_t M) {
    if (f == nullptr) return 16;
    return scatter_ws(f, nullptr, M).total;
}

int naruto_field_scatter_overwrites(const NarutoField* f) { return (f != nullptr && f->plan.atomic_levels == 0) ? 1 : 0; }

int naruto_hash_encode_bwd(const NarutoField* f, uint32_t M, const float* x, const float* d_feat, const float* d_feat_scale, float* d_table,
                           void* workspace, void* stream) {
    if (f == nullptr || d_table == nullptr) return fail(NARUTO_ERR_INVALID, "hash_encode_bwd: NULL argument");
    if (M == 0) return NARUTO_OK;                     // empty batch: d_table is left as it is
    if (x == nullptr || d_feat == nullptr || workspace == nullptr) return fail(NARUTO_ERR_INVALID, "hash_encode_bwd: NULL argument");
    PointSrc ps{};
    ps.x = x;
    ps.S = 1;
    return launch_scatter(f, ps, M, d_feat, (size_t)kFeat, (size_t)2, d_table, workspace, (hipStream_t)stream, nullptr, d_feat_scale);
}

size_t naruto_smoothness_workspace(uint32_t sample_points) { return tv_ws(nullptr, sample_points > 1 ? sample_points - 1 : 1).total; }

int naruto_smoothness_fwd(const NarutoField* f, const float* table, uint32_t sample_points, float voxel_size, float margin, const float* rand6,
                          float* x_out, float* d_feat, float* loss, void* workspace, void* stream) {
    if (f == nullptr || table == nullptr || rand6 == nullptr || x_out == nullptr || d_feat == nullptr || loss == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "smoothness_fwd: NULL argument");
    if (sample_points < 3 || sample_points > 257) return fail(NARUTO_ERR_INVALID, "smoothness_fwd: sample_points must be in [3, 257]");
    TvArgs a{};
    a.n = sample_points - 1;
    a.voxel = voxel_size;
    a.margin = margin;
    a.grid_size = (float)(sample_points - 1) * voxel_size;
    a.inv_p3 = 1.0f / ((float)sample_points * (float)sample_points * (float)sample_points);
    const uint32_t n3 = a.n * a.n * a.n;
    const TvWs w = tv_ws(workspace, a.n);
    const uint32_t nb = (n3 * kFeat + 255u) / 256u;
    hipLaunchKernelGGL(k_tv_encode, dim3(tv_encode_blocks(n3)), dim3(256), 0, (hipStream_t)stream, f->lt, f->bt, a, rand6,
                       static_cast<const uint64_t*>(nullptr), reinterpret_cast<const float2*>(table), x_out, w.feat);
    if (int rc = check_launch("tv_encode")) return rc;
    hipLaunchKernelGGL(k_tv_loss, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, w.feat, d_feat, w.partial);
    if (int rc = check_launch("tv_loss")) return rc;
    hipLaunchKernelGGL(k_tv_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, w.partial, nb, a.inv_p3, loss);
    return check_launch("tv_finalize");
}

}  // extern "C"

namespace {
// The flat launch of the field query (64-sample tiles over the flat point list; measured in tools/fwd_lab.hip / profiles/r04_fwd_lab.txt): four-wave
// workgroups up to one per CU; between one and two per CU two-wave workgroups, so that no CU holds more tiles than it must (see k_query_fwd; 1 376
// tiles: 42.2 us against 45.6 as eight-wave ones); from two per CU on ONE persistent eight-wave workgroup per CU (one weight image, the waves walk
// their tiles: 76.5 -> 69.0 us at 4 096 tiles).  NARUTO_DEBUG_FWD_SMALL_WG=0: no two-wave form (A/B timing).
// big_wg_on: naruto_query_fwd alone passes NARUTO_DEBUG_FWD_SHAPE here (0: no eight-wave form); the training forward's plan does not read that knob.
struct FlatShape { uint32_t blocks, threads; };
FlatShape flat_fwd_shape(const NarutoField* f, uint32_t n_tiles, bool big_wg_on = true) {
    static const bool small_wg_on = env_int("NARUTO_DEBUG_FWD_SMALL_WG", 1) != 0;
    const uint32_t cu = cu_count(f);
    if (small_wg_on && n_tiles > cu * 4u && n_tiles < cu * 8u) return {(n_tiles + 1u) / 2u, 128u};
    if (big_wg_on && n_tiles >= cu * 8u) return {cu, 512u};
    return {(n_tiles + 3u) / 4u < cu * 4u ? (n_tiles + 3u) / 4u : cu * 4u, 256u};
}
// k_query_fwd / k_query_fwd_bf in that shape.  walk: the unfused depth-ordered walk (ee.tiles_per_ray != 0; colour, 256 threads) has an
// instantiation of its own, so that the flat launches carry none of its code.
int launch_flat_fwd(const NarutoField* f, const NarutoParams& p, const PointSrc& ps, uint32_t M, float* raw, float* sdf_uncert, float* geo, float* feat_save,
                    const EarlyExit& ee, bool color, FlatShape sh, bool walk, hipStream_t st) {
    const bool bf = f->desc.mlp_mode == NARUTO_MLP_BF16;
    if (walk && (!color || sh.threads != 256u)) return fail(NARUTO_ERR_INVALID, "query_fwd: the walk is a colour launch of 256 threads");
#define NARUTO_FLAT(KERNEL, COLOR, NT, EE) \
    hipLaunchKernelGGL((KERNEL<COLOR, NT, EE>), dim3(sh.blocks), dim3(NT), 0, st, f->lt, f->ut, f->bt, p, ps, M, raw, sdf_uncert, geo, feat_save, ee)
#define NARUTO_FLAT_NT(KERNEL, COLOR)                                   \
    do {                                                                \
        if (sh.threads == 128u) NARUTO_FLAT(KERNEL, COLOR, 128, false); \
        else if (sh.threads == 512u) NARUTO_FLAT(KERNEL, COLOR, 512, false); \
        else NARUTO_FLAT(KERNEL, COLOR, 256, false);                    \
    } while (0)
    if (!walk && color && bf) NARUTO_FLAT_NT(k_query_fwd_bf, true);
    else if (!walk && color) NARUTO_FLAT_NT(k_query_fwd, true);
    else if (!walk && bf) NARUTO_FLAT_NT(k_query_fwd_bf, false);
    else if (!walk) NARUTO_FLAT_NT(k_query_fwd, false);
    else if (bf) NARUTO_FLAT(k_query_fwd_bf, true, 256, true);
    else NARUTO_FLAT(k_query_fwd, true, 256, true);
#undef NARUTO_FLAT_NT
#undef NARUTO_FLAT
    return check_launch("query_fwd");
}
}  // namespace

extern "C" {

int naruto_query_fwd(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts, float* raw, float* sdf_uncert,
                     float* geo, float* feat_save, void* stream) {
    if (f == nullptr || p == nullptr) return fail(NARUTO_ERR_INVALID, "query_fwd: NULL argument");
    if (int rc = check_params(p, "query_fwd", kParamsEncoding | kParamsSdf)) return rc;
    if (M == 0) return NARUTO_OK;                     // empty batch: its (NULL) point pointers are not an error
    if (int rc = check_points(pts)) return rc;
    const bool color = raw != nullptr;
    if (color) {
        if (int rc = check_params(p, "query_fwd", kParamsColour, "colour net parameters missing")) return rc;
    }
    if (!color && sdf_uncert == nullptr && geo == nullptr && feat_save == nullptr) return fail(NARUTO_ERR_INVALID, "query_fwd: no output requested");
    if (feat_save != nullptr && M > (1u << 29)) return fail(NARUTO_ERR_INVALID, "query_fwd: feat_save is addressed with 32-bit byte offsets: at most 2^29 points per call");
    NarutoParams pp = *p;
    if (!color) { pp.col_w0 = p->sdf_w0; pp.col_w1 = p->sdf_w0; }       // staged but unused; keep the loads in bounds
    static const bool big_wg_on = env_int("NARUTO_DEBUG_FWD_SHAPE", 1) != 0;      // 0: the shapes from before the eight-wave form (A/B timing)
    return launch_flat_fwd(f, pp, make_points(pts), M, raw, sdf_uncert, geo, feat_save, EarlyExit{}, color, flat_fwd_shape(f, (M + 63u) / 64u, big_wg_on), false, (hipStream_t)stream);
}

}  // extern "C"

namespace {
// workspace of the query backward for a list of `cap` = list_cap(points + extra points) points; the float runs follow each other unpadded:
// | d_feat [16][cap][2] | x [4][cap] (x, y, z, cotangent of raw[...,4]) | wgrad partials | the scatter's workspace | count word + pad |
struct BwdWs { float* d_feat; float* x_soa; float* partials; float* scatter_ws; uint32_t* n_total; size_t total; };
BwdWs bwd_ws(const NarutoField* f, void* workspace, uint32_t cap) {
    Carve c(workspace);
    return {c.take<float>((size_t)kLevels * 2u * (size_t)cap * sizeof(float), 1u), c.take<float>(4u * (size_t)cap * sizeof(float), 1u),
            c.take<float>((size_t)kBwdMaxBlocks * kAccFloats * sizeof(float), 1u), c.take<float>(naruto_scatter_workspace(f, cap), 1u), c.take<uint32_t>(64u, 1u), c.size()};
}

// the scatter's point list as a point source: x [3][cap] in the query backward's workspace (BwdWs.x_soa), one "sample" per point
PointSrc list_points(const float* x_soa, uint32_t cap) {
    PointSrc ps{};
    ps.xsoa = x_soa;
    ps.M = cap;
    ps.S = 1;
    return ps;
}

// What a query backward is given besides the field and the parameters.  naruto_query_bwd fills the public call's arguments; the rest is the fused
// training path (naruto_train_backward) and stays zero otherwise.
struct QueryBwd {
    uint32_t M;
    const NarutoPoints* pts;
    const float* feat_save; const float* d_raw; const float* d_geo;
    const uint32_t* active_idx; const uint32_t* n_active;
    const NarutoExtraPoints* extra;
    uint32_t flags;
    const NarutoGrads* g;
    void* workspace;
    hipStream_t stream;
    // n_front > 0: list positions [0, n_front) were filled by the caller (smoothness lattice: points and weighted feature cotangents), this
    // launch's points follow; n_list_dev = device word holding n_front + n_active
    uint32_t n_front;
    const uint32_t* n_list_dev;
    const AdamFuse* adam;           // the optimiser steps in the launch that finishes the gradients
    const UncertAdam* unc_adam;     // ... and, on its stepping iterations, the uncertainty grid's own (needs adam; p is filled in here)
    const void* w_img;              // the MLP backward's weight images, prepared by k_loss_bwd_fused
    const TvLate* tv_late;          // the moved smoothness term's value lands in the losses with that launch (needs adam)
    const AssembleArgs* next;       // ... which also assembles the next iteration's ray batch (needs adam)
    bool feat_sample_major;         // feat_save is [M][16][2] -- the Morton-ordered forward of the large tables wrote it, see naruto_sorted.hip
};
int query_bwd_impl(const NarutoField* f, const NarutoParams* p, const QueryBwd& q) {
    const uint32_t M = q.M, n_front = q.n_front;
    const NarutoGrads* g = q.g;
    const hipStream_t st = q.stream;
    const uint32_t feat_M = q.feat_sample_major ? 1u : M, feat_mul = q.feat_sample_major ? (uint32_t)kLevels : 1u;
    if ((q.active_idx == nullptr) != (q.n_active == nullptr)) return fail(NARUTO_ERR_INVALID, "query_bwd: active_idx and n_active go together");
    if (n_front > 0 && (q.extra != nullptr || q.n_list_dev == nullptr)) return fail(NARUTO_ERR_INVALID, "query_bwd: front list excludes extra points");
    const uint32_t E = n_front > 0 ? n_front : ((q.extra != nullptr && g != nullptr && g->table != nullptr) ? q.extra->n : 0u);
    if (n_front == 0 && E > 0 && (q.extra->x == nullptr || q.extra->d_feat == nullptr)) return fail(NARUTO_ERR_INVALID, "query_bwd: extra points need x and d_feat");
    const uint32_t cap = list_cap(M + E);            // leading dimension of the scatter's point list
    if (f == nullptr || p == nullptr || g == nullptr || q.feat_save == nullptr || q.d_raw == nullptr || q.workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "query_bwd: NULL argument");
    if (int rc = check_params(p, "query_bwd")) return rc;
    if (M == 0) return NARUTO_OK;
    if (int rc = check_points(q.pts)) return rc;
    const BwdWs w = bwd_ws(f, q.workspace, cap);
    if ((reinterpret_cast<uintptr_t>(w.partials) & 15u) != 0u) return fail(NARUTO_ERR_INVALID, "query_bwd: the workspace must be 16-byte aligned");
    const bool bf = f->desc.mlp_mode == NARUTO_MLP_BF16;
    const uint32_t n_tiles = bf ? (M + 63u) / 64u : (M + 31u) / 32u;
    const uint32_t waves = bf ? 4u : (uint32_t)kBwdWaves;
    uint32_t blocks = (n_tiles + waves - 1u) / waves;
    uint32_t max_blocks = cu_count(f) * (bf ? (uint32_t)NARUTO_BWD_BF_MINWAVES : 1u);
    if (max_blocks > kBwdMaxBlocks) max_blocks = kBwdMaxBlocks;
    static const int dbg_blocks = env_int("NARUTO_DEBUG_BWD_BLOCKS", 0);       // profiling knob
    if (dbg_blocks > 0 && (uint32_t)dbg_blocks < max_blocks) max_blocks = (uint32_t)dbg_blocks;
    if (blocks > max_blocks) blocks = max_blocks;
    const PointSrc ps = make_points(q.pts);
    static bool attr_set = false;
    if (int rc = reserve_lds(attr_set, {lds_use(k_query_bwd, sizeof(BwdLds)), lds_use(k_query_bwd_timeline, sizeof(BwdLds)), lds_use(k_query_bwd_bf, kBwdBfLdsBytes)}, "query_bwd: cannot reserve %zu bytes of LDS", sizeof(BwdLds)))
        return rc;
    // the uncertainty grid's gradient: through the scatter (row 3 of the point list) unless the grid is too large for that
    const bool unc_scatter = g->uncert_grid != nullptr && f->plan.n_uncert != 0;
    const int unc_atomic = (g->uncert_grid != nullptr && f->plan.n_uncert == 0) ? 1 : 0;
    const float* unc_g = unc_scatter ? w.x_soa + 3u * (size_t)cap : nullptr;
    float* d_unc = unc_scatter ? g->uncert_grid : nullptr;
    float* x_list = (g->table != nullptr || q.adam != nullptr || unc_scatter) ? w.x_soa : nullptr;
    const bool phase_mlp = (q.flags & NARUTO_TRAIN_BWD_TABLE_ONLY) == 0u;        // phases: see naruto_train_backward
    const bool phase_table = (q.flags & NARUTO_TRAIN_BWD_MLP_ONLY) == 0u;
    if (!phase_mlp) { /* the point list, d_feat and the wgrad partials are those of the preceding MLP-only call */ }
    else if (bf)
        hipLaunchKernelGGL(k_query_bwd_bf, dim3(blocks), dim3(256), kBwdBfLdsBytes, st, f->lt, f->ut, f->bt, *p, ps, M, cap, q.feat_save, q.d_raw,
                           q.d_geo, w.d_feat, x_list, g->uncert_grid, w.partials, q.active_idx, q.n_active, n_front, unc_atomic, q.w_img, feat_M, feat_mul);
    else if (g_bwd_timeline != nullptr)         // profiling build of the same kernel: a row of kBwdTlSlots stamps per wave
        hipLaunchKernelGGL(k_query_bwd_timeline, dim3(blocks), dim3(64 * kBwdWaves), sizeof(BwdLds), st, f->lt, f->ut, f->bt, *p, ps, M, cap, q.feat_save, q.d_raw,
                           q.d_geo, w.d_feat, x_list, g->uncert_grid, w.partials, q.active_idx, q.n_active, n_front, unc_atomic, q.w_img, feat_M, feat_mul,
                           g_bwd_timeline);
    else
        hipLaunchKernelGGL(k_query_bwd, dim3(blocks), dim3(64 * kBwdWaves), sizeof(BwdLds), st, f->lt, f->ut, f->bt, *p, ps, M, cap, q.feat_save, q.d_raw,
                           q.d_geo, w.d_feat, x_list, g->uncert_grid, w.partials, q.active_idx, q.n_active, n_front, unc_atomic, q.w_img, feat_M, feat_mul);
    if (int rc = check_launch("query_bwd")) return rc;
    const PointSrc pss = list_points(w.x_soa, cap);
    if (q.adam != nullptr) {
        if (!phase_mlp || !phase_table) return fail(NARUTO_ERR_INVALID, "query_bwd: the fused optimiser runs the backward in one piece");
        // optimiser in the backward: the tiled scatter without its reduce, then ONE launch finishes the tiled levels' table
        // gradient + the weight gradients and steps them; the binned scatter's last kernel steps the larger levels itself
        const uint32_t* cnt = n_front > 0 ? q.n_list_dev : q.n_active;
        const uint32_t Ml = cnt != nullptr ? cap : M;
        if (int rc = launch_scatter(f, pss, Ml, w.d_feat, (size_t)2, (size_t)2 * (size_t)cap, g->table, w.scatter_ws, st, cnt, nullptr, 1, false, q.adam, unc_g, d_unc, n_front))
            return rc;
        const size_t n_params = (size_t)f->n_tiled_entries * 2u;
        const uint32_t n_table_blocks = (uint32_t)((n_params / 4u + 255u) / 256u);
        UncertReduce ur{};
        if (unc_scatter) {
            ur.d_uncert = d_unc; ur.partial = scatter_ws(f, w.scatter_ws, Ml).unc_partial; ur.n_voxels = f->plan.uncert_voxels; ur.n_splits = uncert_splits(f, Ml);
            ur.voxels_pad = uncert_pad(f);
        }
        if (q.unc_adam != nullptr && q.unc_adam->on) {
            if (!unc_scatter || p->uncert_grid == nullptr)
                return fail(NARUTO_ERR_INVALID, "query_bwd: the uncertainty grid's step rides in the finishing launch only where its gradient goes through the scatter");
            ur.adam = *q.unc_adam;
            ur.adam.p = const_cast<float*>(p->uncert_grid);          // (NarutoParams is read-only to a backward; the fused optimisers step in place)
            ur.adam.n_blocks = (ur.n_voxels + 255u) / 256u;
        }
        const uint32_t n_unc_blocks = unc_scatter ? (ur.n_voxels + 255u) / 256u : 0u;
        const TvLate tvl = q.tv_late != nullptr ? *q.tv_late : TvLate{};
        const uint32_t n_finish = n_table_blocks + kAccFloats / 32 + n_unc_blocks + (tvl.n_tv_blocks != 0u ? 1u : 0u);
        if (q.next != nullptr) {
            const uint32_t n_asm = (q.next->n_global + q.next->n_cur + 255u) / 256u;
            hipLaunchKernelGGL(k_bwd_finish_next, dim3(n_finish + n_asm), dim3(256), 0, st, f->lt, w.scatter_ws, level_splits(f, Ml),
                               n_params, partial_plane(f), w.partials, blocks, *g, *q.adam, n_table_blocks, ur, tvl, n_unc_blocks, n_asm, *q.next);
            return check_launch("bwd_finish_next");
        }
        hipLaunchKernelGGL(k_bwd_finish, dim3(n_finish), dim3(256), 0, st, f->lt, w.scatter_ws, level_splits(f, Ml),
                           n_params, partial_plane(f), w.partials, blocks, *g, *q.adam, n_table_blocks, ur, tvl, n_unc_blocks);
        return check_launch("bwd_finish");
    }
    const bool want_w = g->sdf_w0 || g->sdf_w1 || g->col_w0 || g->col_w1;
    if (want_w && phase_mlp) {
        hipLaunchKernelGGL(k_wgrad_reduce, dim3(kAccFloats / 32), dim3(256), 0, st, w.partials, blocks, *g, (int)(q.flags & NARUTO_BWD_OVERWRITE_WEIGHT_GRADS));
        if (int rc = check_launch("wgrad_reduce")) return rc;
    }
    if (!phase_table) return NARUTO_OK;
    if (g->table == nullptr && !unc_scatter) return NARUTO_OK;
    if (n_front > 0)
        return launch_scatter(f, pss, cap, w.d_feat, (size_t)2, (size_t)2 * (size_t)cap, g->table, w.scatter_ws, st, q.n_list_dev, nullptr,
                              (int)(q.flags & NARUTO_BWD_OVERWRITE_TABLE_GRAD), true, nullptr, unc_g, d_unc, n_front);
    const uint32_t* count_dev = q.n_active;
    if (E > 0) {          // the smoothness lattice rides along in the same scatter launch
        hipLaunchKernelGGL(k_append_points, dim3((E * kLevels + 255u) / 256u), dim3(256), 0, st, E, q.extra->x, q.extra->d_feat, q.extra->scale,
                           q.n_active, M, cap, w.x_soa, w.d_feat, w.n_total);
        if (int rc = check_launch("append_points")) return rc;
        count_dev = w.n_total;
    }
    // host-side point count: the padded capacity only bounds a device-side count; without one the list holds exactly M points
    return launch_scatter(f, pss, count_dev != nullptr ? cap : M, w.d_feat, (size_t)2, (size_t)2 * (size_t)cap, g->table, w.scatter_ws, st, count_dev, nullptr,
                          (int)(q.flags & NARUTO_BWD_OVERWRITE_TABLE_GRAD), true, nullptr, unc_g, d_unc);
}
}  // namespace

extern "C" {

size_t naruto_query_bwd_workspace(const NarutoField* f, uint32_t M) { return bwd_ws(f, nullptr, list_cap(M)).total; }

int naruto_query_bwd(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts, const float* feat_save,
                     const float* d_raw, const float* d_geo, const uint32_t* active_idx, const uint32_t* n_active, const NarutoExtraPoints* extra,
                     uint32_t flags, const NarutoGrads* g, void* workspace, void* stream) {
    QueryBwd q{};
    q.M = M; q.pts = pts; q.feat_save = feat_save; q.d_raw = d_raw; q.d_geo = d_geo;
    q.active_idx = active_idx; q.n_active = n_active; q.extra = extra;
    q.flags = flags; q.g = g; q.workspace = workspace; q.stream = (hipStream_t)stream;
    return query_bwd_impl(f, p, q);
}

// ------------------------------------------------------------------------------------------------
// Gradient of the query with respect to its points (see naruto_pointgrad.hip)
// ------------------------------------------------------------------------------------------------
size_t naruto_query_bwd_points_workspace(const NarutoField*, uint32_t M) { return point_grad_ws(nullptr, M).total; }

int naruto_query_bwd_points(const NarutoField* f, const NarutoParams* p, uint32_t M, const NarutoPoints* pts, const float* d_raw, const float* d_geo,
                            const uint32_t* active_idx, const uint32_t* n_active, float* d_x, float* d_rays_o, float* d_rays_d, uint32_t flags,
                            void* workspace, void* stream) {
    if (f == nullptr || p == nullptr || pts == nullptr || d_raw == nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: NULL argument");
    if (int rc = check_params(p, "query_bwd_points")) return rc;
    if ((active_idx == nullptr) != (n_active == nullptr)) return fail(NARUTO_ERR_INVALID, "query_bwd_points: active_idx and n_active go together");
    if ((flags & ~NARUTO_BWD_POINTS_ACCUMULATE) != 0u) return fail(NARUTO_ERR_INVALID, "query_bwd_points: unknown flags 0x%x", flags);
    if (int rc = check_points(pts)) return rc;
    if (M > (1u << 29)) return fail(NARUTO_ERR_INVALID, "query_bwd_points: at most 2^29 points per call (got %u)", M);
    const bool rays = pts->x == nullptr;
    const int acc = (flags & NARUTO_BWD_POINTS_ACCUMULATE) ? 1 : 0;
    const hipStream_t st = (hipStream_t)stream;
    const PointSrc ps = make_points(pts);
    if (!rays) {
        if (d_rays_o != nullptr || d_rays_d != nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: d_rays_o / d_rays_d belong to ray points, these are x points");
        if (d_x == nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: no output (x points write d_x)");
    } else {
        if (d_x != nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: d_x belongs to x points; ray points write d_rays_o / d_rays_d");
        if (d_rays_o == nullptr && d_rays_d == nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: no output (ray points write d_rays_o and / or d_rays_d)");
        if (pts->n_samples > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "query_bwd_points: at most %d samples per ray (got %u)", kMaxSamples, pts->n_samples);
        if (M % pts->n_samples != 0u) return fail(NARUTO_ERR_INVALID, "query_bwd_points: M = %u is not a whole number of rays of %u samples", M, pts->n_samples);
        if (workspace == nullptr) return fail(NARUTO_ERR_INVALID, "query_bwd_points: ray points need naruto_query_bwd_points_workspace(f, M) bytes of workspace");
    }
    if (M == 0) return NARUTO_OK;
    float* out = rays ? point_grad_ws(workspace, M).d_x : d_x;
    // a list leaves the other points' rows alone: they must read as zero where the result is written, not added
    if (active_idx != nullptr && (rays || !acc)) {
        if (hipMemsetAsync(out, 0, 3u * sizeof(float) * (size_t)M, st) != hipSuccess) return check_launch("query_bwd_points: zero fill");
    }
    const uint32_t blocks = (M + (uint32_t)kPgThreads - 1u) / (uint32_t)kPgThreads;
    hipLaunchKernelGGL(k_query_bwd_points, dim3(blocks), dim3(kPgThreads), 0, st, f->lt, f->ut, f->bt, ps, M, reinterpret_cast<const float2*>(p->table),
                       p->uncert_grid, p->sdf_w0, p->sdf_w1, p->col_w0, p->col_w1, d_raw, d_geo, active_idx, n_active, out, rays ? 1 : 0, rays ? 0 : acc);
    if (int rc = check_launch("query_bwd_points")) return rc;
    if (!rays) return NARUTO_OK;
    const uint32_t n_rays = M / pts->n_samples;
    hipLaunchKernelGGL(k_ray_point_reduce, dim3((n_rays + 3u) / 4u), dim3(256), 0, st, n_rays, pts->n_samples, out, pts->z_vals, d_rays_o, d_rays_d, acc);
    return check_launch("ray_point_reduce");
}

// ------------------------------------------------------------------------------------------------
// The mapping iteration as two calls (see naruto_train.hip)
// ------------------------------------------------------------------------------------------------
namespace {
struct TrainWs {
    float* terms; float* tv_feat; double* tv_partial; void* bwd; double* fold; uint32_t* block_sums; void* w_img; float* w10;
    void* sort;                   // the Morton-ordered forward's buffers: sort_ws
    uint32_t n3, n_tv_blocks;
    size_t total;
};
// the Morton-ordered forward's buffers (naruto_sorted.hip) for M samples, Mp = M rounded up to whole 64-sample tiles; unpadded:
// | count | cursor | base [3][kSortCells] | the two list lengths, 6 unused words, k_sort_sum's totals at word 8 [320] | cells | list | list2 [3][Mp] | pts [Mp] float4 |
struct SortWs { uint32_t* count; uint32_t* cursor; uint32_t* base; uint32_t* n_list; uint32_t* cells; uint32_t* list; uint32_t* list2; float4* pts; size_t total; };
SortWs sort_ws(void* base, size_t M) {
    const size_t per_cell = (size_t)kSortCells * sizeof(uint32_t), per_sample = (M + 63u) / 64u * 64u * sizeof(uint32_t);
    Carve c(base);
    return {c.take<uint32_t>(per_cell, 1u), c.take<uint32_t>(per_cell, 1u), c.take<uint32_t>(per_cell, 1u), c.take<uint32_t>(320u * sizeof(uint32_t), 1u),
            c.take<uint32_t>(per_sample, 1u), c.take<uint32_t>(per_sample, 1u), c.take<uint32_t>(per_sample, 1u), c.take<float4>(4u * per_sample, 1u), c.size()};
}
TrainWs train_ws(const NarutoField* f, const NarutoTrainStep* t) {
    TrainWs w{};
    const uint32_t S = t->n_samples_d + t->n_range_d;
    const size_t M = (size_t)t->n_rays * S;
    const uint32_t n = t->smooth_points > 1 ? t->smooth_points - 1 : 0;
    w.n3 = n * n * n;
    w.n_tv_blocks = (w.n3 * (uint32_t)kFeat + 255u) / 256u;        // smoothness role blocks of the loss stage (grid-stride beyond 512: more
    if (w.n_tv_blocks > 512u) w.n_tv_blocks = 512u;                // blocks only move the time into the one-workgroup tail)
    Carve c(t->workspace);
    w.terms = c.take<float>((size_t)t->n_rays * 16u * sizeof(float));
    w.tv_feat = c.take<float>((size_t)w.n3 * kFeat * sizeof(float));
    w.tv_partial = c.take<double>((size_t)w.n_tv_blocks * sizeof(double));
    w.fold = c.take<double>((size_t)kTailRows * 16u * sizeof(double));
    w.block_sums = c.take<uint32_t>(((size_t)t->n_rays / kCompactBlock + 2u) * sizeof(uint32_t));
    w.w_img = c.take<void>(bwd_weight_image_bytes());
    w.w10 = c.take<float>(16u * sizeof(float));          // gathered loss_weight_parts
    w.bwd = c.take<void>(bwd_ws(f, nullptr, list_cap((uint32_t)(M + w.n3))).total);
    w.sort = c.take<void>(sort_ws(nullptr, M).total);    // (every plan: the plan is not known here; 28 B per sample in whole tiles + 3 MB of cell arrays + 1 280 B)
    w.total = c.size();
    return w;
}
// NarutoTrainStep.fwd_image, the exact mode's forward weight image kept from one iteration to the next (naruto_field.hip, fwd_image_put):
// | FwdLdsX3, 16-byte aligned | the slot of every MLP weight, uint32 [kNumWeights] |.  The caller's buffer, not part of the workspace above.
struct FwdImageWs { void* image; uint32_t* slots; size_t total; };
FwdImageWs fwd_image_ws(void* base) {
    Carve c(base);
    return {c.take<void>(kFwdImageBytes, 16u), c.take<uint32_t>((size_t)kNumWeights * sizeof(uint32_t), 16u), c.size()};
}
// the image a training forward may read: only on the caller's word that it is fresh, and only where a kernel takes one (exact mode, x3 chain)
inline const void* fresh_fwd_image(const NarutoField* f, const NarutoTrainStep* t) {
    return (t->fwd_image != nullptr && t->fwd_image_fresh != 0u && f->desc.mlp_mode != NARUTO_MLP_BF16) ? fwd_image_ws(t->fwd_image).image : nullptr;
}
TvArgs tv_args(const NarutoTrainStep* t) {
    TvArgs a{};
    if (t->smooth_points == 0) return a;
    a.n = t->smooth_points - 1;
    a.voxel = t->smooth_voxel;
    a.margin = t->smooth_margin;
    a.grid_size = (float)(t->smooth_points - 1) * t->smooth_voxel;
    a.inv_p3 = 1.0f / ((float)t->smooth_points * (float)t->smooth_points * (float)t->smooth_points);
    return a;
}
// What every training entry point derives from (f, t), once per call: the batch's counts, the capacity of the backward's point list (the
// smoothness lattice in front of the samples), the two workspace layouts and the lattice's arguments in that list's layout.
struct TrainCtx {
    uint32_t N, S, M;       // rays, samples per ray, samples
    uint32_t cap;           // list_cap(M + n3)
    TrainWs w;
    BwdWs bw;               // over w.bwd
    TvArgs tva;             // cap filled in
    // depth sampling of the batch's rays (k_sample_encode, or the walk itself where the plan moved it there)
    SampleArgs sample_args(const NarutoTrainStep* t) const {
        const float* jitter = t->perturb ? t->rand : nullptr;
        const uint64_t* jitter_rng = (t->perturb && t->rand == nullptr) ? t->rng : nullptr;
        return SampleArgs{N, t->target_d, t->near_, t->far_, t->n_samples_d, t->n_range_d, t->range_d, jitter, jitter_rng, t->z_vals, (N + 3u) / 4u};
    }
};
TrainCtx train_ctx(const NarutoField* f, const NarutoTrainStep* t) {
    TrainCtx c{};
    c.N = t->n_rays; c.S = t->n_samples_d + t->n_range_d; c.M = c.N * c.S;
    c.w = train_ws(f, t);
    c.cap = list_cap(c.M + c.w.n3);
    c.bw = bwd_ws(f, c.w.bwd, c.cap);
    c.tva = tv_args(t);
    c.tva.cap = c.cap;
    return c;
}
int train_check(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const char* who) {
    if (f == nullptr || p == nullptr || t == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_params(p, who)) return rc;
    if (t->rays_o == nullptr || t->rays_d == nullptr || t->target_rgb == nullptr || t->target_d == nullptr || t->z_vals == nullptr || t->raw == nullptr ||
        t->feat_save == nullptr || t->sums == nullptr || t->losses == nullptr || t->workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL buffer in NarutoTrainStep", who);
    const uint32_t S = t->n_samples_d + t->n_range_d;
    if (t->n_rays == 0 || S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "%s: need rays and 2..%d samples per ray", who, kMaxSamples);
    if ((uint64_t)t->n_rays * S > 0x7FFFFFFFull) return fail(NARUTO_ERR_INVALID, "%s: too many samples for 32-bit indices", who);
    if (t->smooth_points != 0 && (t->smooth_points < 3 || t->smooth_points > 257)) return fail(NARUTO_ERR_INVALID, "%s: smooth_points must be 0 or in [3, 257]", who);
    if (t->perturb && t->rand == nullptr && t->rng == nullptr) return fail(NARUTO_ERR_INVALID, "%s: perturb needs rand or rng", who);
    if (t->smooth_points != 0 && t->rand6 == nullptr && t->rng == nullptr) return fail(NARUTO_ERR_INVALID, "%s: the smoothness term needs rand6 or rng", who);
    if (t->smooth_points != 0 && t->loss_weights == nullptr) return fail(NARUTO_ERR_INVALID, "%s: the smoothness term needs loss_weights", who);
    if ((reinterpret_cast<uintptr_t>(t->fwd_image) & 15u) != 0u) return fail(NARUTO_ERR_INVALID, "%s: fwd_image must be 16-byte aligned", who);
    return NARUTO_OK;
}
// A2..A5 of the training forward.  ONE decision, used by everyone who has to know which launch form it takes (the forward itself, the backward's
// moved smoothness term, the debug re-launches):
//   Flat    64-sample tiles over the flat point list (k_query_fwd in flat_fwd_shape), loss stage and depth sampling in launches of their own;
//           where every other form falls back to
//   Walk    one wave per ray, front to back with depth-ordered early termination (k_query_fwd_loss when the loss stage rides along -- `fused` --,
//           k_query_fwd<EE> otherwise: S a multiple of 64 only); since round 5 the fused form also takes sample counts that are not a multiple
//           of 64 -- the ray's last tile is partly filled, its dead lanes issue no loads -- (NARUTO_WALK_PARTIAL: 0 never, 1 (default) up to
//           NARUTO_WALK_PARTIAL_MAX tiles per CU, 2 always)
//   Packed  k_query_fwd_loss_packed (see launch_train_query)
//   Short   S <= 64 (round 5): a workgroup packs 256 / S rays into its four waves' tiles (k_query_fwd_loss_short), loss stage inside, one row
//           of loss partials per workgroup -- the shipped 32 + 11 sampling without a second round of workgroups
//   Sorted  tables no cache holds (round 6): the flat field query in Morton order of the samples a consumer can see (naruto_sorted.hip), loss stage
//           in its own launch; feat_save sample-major
// The five-launch iteration (round 4, see WalkExtra in naruto_train.hip; `tv_moved`): where the form is the fused Walk in its two-phase form, or Short,
// and forward + backward are issued as one iteration (deferred tail), the forward samples its own depths, its tail workgroups encode the smoothness
// lattice, the term itself is evaluated by workgroups of the backward's first launch and its value lands in the losses with the backward's last
// launch -- k_sample_encode has no launch of its own.  NARUTO_TV_MOVE=0: the six-launch form (same bits).
enum class FwdForm { Flat, Walk, Packed, Short, Sorted };
struct TrainFwdPlan {
    FwdForm form;
    bool fused;         // the loss stage rides in the field query's launch
    bool split;         // Walk: the two-phase tile (k_query_fwd_loss<*, true>)
    bool tv_moved;      // the walk samples its own depths and encodes the lattice; the term is evaluated in the backward's first launch
    uint32_t tpr;       // Walk: tiles per ray
    uint32_t rays_per_row;      // rays per row of the loss stage's partial sums (kRaysPerBlock, or Short's rays per workgroup)
    uint32_t blocks;            // workgroups of the field-query launch (ray workgroups: the smoothness tail's are not counted)
    uint32_t threads;           // threads per workgroup of that launch
    uint32_t pack_rows;         // Packed: loss rows a workgroup holds at a time
    uint32_t pack_waves;        // Packed: waves per workgroup
};
// what a Packed workgroup of W waves keeps besides its rays: the static LDS of the fp32 form (the larger) + 256 B
inline size_t packed_fixed_lds(uint32_t W) { return (W == 4u ? packed_static_lds<false, 4>() : packed_static_lds<false, 8>()) + 256u; }
TrainFwdPlan train_fwd_plan(const NarutoField* f, const NarutoTrainStep* t, bool with_loss, bool deferred) {
    static const bool tv_on = env_int("NARUTO_TV_MOVE", 1) != 0;
    static const bool no_fuse = getenv("NARUTO_DEBUG_NO_FUSED_LOSS_STAGE") != nullptr, no_ee = getenv("NARUTO_DEBUG_NO_EARLY_EXIT") != nullptr;
    static const int packed_mode = env_int("NARUTO_FWD_PACKED", 1);
    static const int partial_mode = env_int("NARUTO_WALK_PARTIAL", 1);
    // measured (tools/walk_ab.sh, profiles/r05_walk_ab.txt): Short wins while its workgroups are ONE round (two per CU: 8 tiles) -- 2 048 x 43
    // 0.171 -> 0.159 ms, the BA batch 0.1875 -> 0.1795 -- and loses beyond (8 192 x 43: 0.391 -> 0.408, 131 072 x 43: 4.86 -> 4.92)
    static const uint32_t partial_max = (uint32_t)env_int("NARUTO_WALK_PARTIAL_MAX", 8);
    const uint32_t N = t->n_rays, S = t->n_samples_d + t->n_range_d;
    static const int pack_waves = env_int("NARUTO_PACK_WAVES", 8);
    const FlatShape flat = flat_fwd_shape(f, (uint32_t)(((uint64_t)N * S + 63u) / 64u));
    TrainFwdPlan pl{FwdForm::Flat, false, false, false, 0u, (uint32_t)kRaysPerBlock, flat.blocks, flat.threads, 0u, 0u};
    const bool exact = S % 64u == 0u && S > 64u;
    const bool can_fuse = with_loss && !no_fuse && ray_scratch_bytes(S) <= kFwdLossMaxRayLds;
    bool packed_on = packed_mode == 2 || ((packed_mode == 1 || packed_mode == 3) && !exact);
    if (packed_on && packed_mode == 1) packed_on = (size_t)f->n_entries * 2u * sizeof(float) > ((size_t)64u << 20);
    // NARUTO_FWD_SORTED: 1 (default) the Morton-ordered forward for tables of more than 64 MB -- where every gather is an HBM line --, 2 for
    // every table (tests), 0 never (the packed forward as in round 4 / 5)
    static const int sorted_mode = env_int("NARUTO_FWD_SORTED", 1);
    const bool big_table = (size_t)f->n_entries * 2u * sizeof(float) > ((size_t)64u << 20);
    // (cache-resident tables too once the batch is millions of samples -- 131 072 x 43 at T = 2^16: 5.05 -> 4.71 ms -- but not below: 8 192 x 43 0.349 -> 0.380)
    const bool big_batch = (uint64_t)N * S >= 4000000ull && S <= 64u;
    if (with_loss && (sorted_mode == 2 || (sorted_mode == 1 && (big_table || big_batch) && packed_mode == 1)) && (uint64_t)N * S < 0x0FFFFFFFull) {
        pl.form = FwdForm::Sorted;
        pl.blocks = cu_count(f);            // the list queries (k_query_fwd_list)
        pl.threads = 512u;
        return pl;
    }
    if (packed_on && with_loss && !no_fuse && S <= 4095u && N >= 1u) {
        // workgroup shape: 8 waves x 1 per CU, or 4 waves x 2 per CU (NARUTO_PACK_WAVES); rows (of four rays) a workgroup holds at a time: as many as
        // the LDS next to the weights, the feature slabs and the tiles' points takes, at most three
        const uint32_t W = pack_waves == 4 ? 4u : 8u, per_cu = W == 4u ? 2u : 1u;
        const size_t lds_free = (size_t)160u * 1024u / per_cu > packed_fixed_lds(W) ? (size_t)160u * 1024u / per_cu - packed_fixed_lds(W) : 0u;
        uint32_t rows = kPackMaxRows;
        while (rows > 0u && packed_lds_bytes(rows, S) > lds_free) --rows;
        if (rows > 0u) {                    // (else not even one row fits the LDS: the flat launch, its loss stage in a launch of its own)
            const uint32_t n_rows = (N + (uint32_t)kRaysPerBlock - 1u) / (uint32_t)kRaysPerBlock;
            const uint32_t slots = cu_count(f) * per_cu;
            pl.form = FwdForm::Packed;
            pl.fused = true;
            pl.blocks = n_rows < slots ? n_rows : slots;        // every workgroup resident at once, the rows spread evenly over them
            pl.threads = 64u * W;
            pl.pack_rows = rows;
            pl.pack_waves = W;
        }
        return pl;
    }
    if (S <= 64u && can_fuse && partial_mode != 0) {
        const uint32_t R = short_rays_per_block(S);
        if (partial_mode == 2 || (uint64_t)((N + R - 1u) / R) * 4u <= (uint64_t)cu_count(f) * partial_max) {
            pl.form = FwdForm::Short;
            pl.fused = true;
            pl.split = true;
            pl.rays_per_row = R;
            pl.blocks = (N + R - 1u) / R < cu_count(f) * 4u ? (N + R - 1u) / R : cu_count(f) * 4u;
            pl.threads = 256u;
            pl.tv_moved = tv_on && deferred && t->smooth_points != 0;
            return pl;
        }
    }
    const uint32_t tpr = (S + 63u) / 64u;
    bool walk = exact && !no_ee;
    if (!walk && !exact && !no_ee && can_fuse && partial_mode != 0)
        walk = partial_mode == 2 || (uint64_t)N * tpr <= (uint64_t)cu_count(f) * partial_max * 2u;
    if (!walk) return pl;
    pl.form = FwdForm::Walk;
    pl.tpr = tpr;
    pl.blocks = (N + 3u) / 4u < cu_count(f) * 4u ? (N + 3u) / 4u : cu_count(f) * 4u;          // one wave per ray
    pl.threads = 256u;
    pl.fused = can_fuse;
    // (two workgroups per CU: static LDS -- weight images, four slabs, the loss rows -- + the rays' images within half a CU's 160 KB)
    pl.split = pl.fused && sizeof(FwdLdsX3) + (size_t)kRaysPerBlock * sizeof(FwdSlab) + ray_scratch_fwd_bytes(S) + 256u <= (size_t)80u * 1024u;
    pl.tv_moved = tv_on && deferred && t->smooth_points != 0 && pl.fused && pl.split;
    return pl;
}
// What the walk of plan `pl` does besides the field query: it may read the weight image, and where the plan moved the smoothness term it samples
// its rays' depths and its tail workgroups encode the lattice (NARUTO_TV_TAIL_GROUPS: level groups per lattice-encode workgroup, 1, 2 or 4)
WalkExtra walk_extra(const NarutoField* f, const NarutoTrainStep* t, const TrainCtx& c, const TrainFwdPlan& pl) {
    static const uint32_t tv_groups = (uint32_t)env_int("NARUTO_TV_TAIL_GROUPS", 1);
    WalkExtra wx{};
    wx.w_img = fresh_fwd_image(f, t);
    if (!pl.tv_moved) return wx;
    wx.on = 1u;
    wx.tv_groups = tv_groups;
    wx.sa = c.sample_args(t);
    wx.rand6 = t->rand6; wx.rng = t->rng; wx.x_out = c.bw.x_soa;
    return wx;
}
// rows of per-workgroup partial sums the FUSED loss stage of the plan's form leaves (the stand-alone k_loss_stage: one per kRaysPerBlock rays)
inline uint32_t loss_rows(const TrainFwdPlan& pl, uint32_t n_rays) { return (n_rays + pl.rays_per_row - 1u) / pl.rays_per_row; }
// The field query of the training forward in the form `pl` (a plan with the loss stage: train_fwd_plan(f, t, true, ...)); *fused tells whether the
// loss stage rode in it.  wx.on goes with pl.tv_moved: the caller left k_sample_encode out because the plan has the walk sample its own depths.
int launch_train_query(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const TrainCtx& c, const TrainFwdPlan& pl, hipStream_t st,
                       const LossStageArgs& loss, const WalkExtra& wx, bool* fused) {
    if (fused != nullptr) *fused = false;
    const uint32_t N = c.N, S = c.S, M = c.M;
    PointSrc ps{};
    ps.rays_o = t->rays_o; ps.rays_d = t->rays_d; ps.z_vals = t->z_vals; ps.S = S;
    const uint32_t blocks = pl.blocks;
    const bool bfm = f->desc.mlp_mode == NARUTO_MLP_BF16;
    EarlyExit ee{};
    if (pl.form == FwdForm::Walk) {      // depth-ordered early termination: one wave per ray, front to back
        ee.target_d = t->target_d;
        ee.trunc_sc = f->desc.trunc * f->desc.sc_factor;
        ee.tiles_per_ray = pl.tpr;
    }
    // the packed forward (k_query_fwd_loss_packed: only the samples a consumer can see, packed across rays, loss stage from LDS; any
    // samples-per-ray count).  Its workgroup works in barrier-separated steps -- all gathers of a pass, then all matrix chains -- so what it
    // gains is the samples it does NOT evaluate, and what it loses is the flat launch's overlap of one wave's gathers with another's matrix
    // chain.  Measured (tools/ba_ab.sh, tools/fwd_timeline_ba.py):
    //   * tables no cache holds (T = 2^22, 281 MB): every gather is an HBM line -- 131 072 x 43: 8.09 against 9.41 ms per step: ON;
    //   * cache-resident tables: scene dependent.  2 048 random benchmark rays x 43: 0.166 against 0.1715 ms per step; the BA batch (2 148
    //     rays from the keyframe store, random-initialised network: nearly every sample ends up evaluated, in two passes): ray workgroups
    //     55 us + the smoothness tail against 42.7 + 8.6 us flat, 0.206 against 0.188 ms per iteration; 131 072 x 43: 5.92 against 4.87 ms.
    //     Nothing known at launch time tells these apart: OFF (S = 64 k keeps the depth-ordered walk, everything else the flat launch).
    // NARUTO_FWD_PACKED: 0 never, 1 (default) as above, 2 everywhere incl. S = 64 k, 3 wherever the walk cannot run.  Losses and gradients
    // agree with the other launch shapes to the distance between OneBlob's closed and dense forms, ~1e-6 (which form a point gets depends on
    // the tile it shares).  NARUTO_PACK_ONE_PASS=1: every sample in the first pass (measured: 0.200 / 0.180 ms at the two batches above).
    if (pl.form == FwdForm::Sorted) {
        const SortWs sw = sort_ws(c.w.sort, M);
        SortArgs sa{};
        sa.M = M; sa.S = S; sa.target_d = t->target_d; sa.trunc_sc = f->desc.trunc * f->desc.sc_factor;
        sa.count = sw.count; sa.cursor = sw.cursor; sa.base = sw.base; sa.n_list = sw.n_list;
        sa.cells = sw.cells; sa.list = sw.list; sa.list2 = sw.list2; sa.pts = sw.pts;
        hipLaunchKernelGGL(k_sort_zero, dim3(2u * kSortCells / 4u / 256u), dim3(256), 0, st, reinterpret_cast<uint4*>(sa.count), 2u * kSortCells / 4u);
        const uint32_t mblocks = (M + 256u * kSortPer - 1u) / (256u * kSortPer);
        hipLaunchKernelGGL(k_sort_count, dim3(mblocks), dim3(256), 0, st, sa, ps, f->bt, t->raw);
        hipLaunchKernelGGL(k_sort_sum, dim3(256), dim3(256), 0, st, sa, sa.n_list + 8);          // (the totals: 256 words behind the two list lengths)
        hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(256), 0, st, sa, sa.n_list + 8);
        hipLaunchKernelGGL(k_sort_fill, dim3(mblocks), dim3(256), 0, st, sa, ps, f->bt);
        if (int rc = check_launch("sort_count / scan / fill")) return rc;
#define NARUTO_LAUNCH_LIST(LISTV, PTSV, NV) do { \
            if (bfm) hipLaunchKernelGGL(k_query_fwd_list<true>, dim3(blocks), dim3(512), 0, st, f->lt, f->ut, f->bt, *p, ps, LISTV, PTSV, NV, t->raw, t->feat_save); \
            else hipLaunchKernelGGL(k_query_fwd_list<false>, dim3(blocks), dim3(512), 0, st, f->lt, f->ut, f->bt, *p, ps, LISTV, PTSV, NV, t->raw, t->feat_save); } while (0)
        NARUTO_LAUNCH_LIST(sa.list, sa.pts, sa.n_list);
        if (int rc = check_launch("query_fwd_list")) return rc;
        hipLaunchKernelGGL(k_sort_more, dim3((N + 255u) / 256u), dim3(256), 0, st, sa, N, t->z_vals, t->raw);
        NARUTO_LAUNCH_LIST(sa.list2, static_cast<const float4*>(nullptr), sa.n_list + 1);
#undef NARUTO_LAUNCH_LIST
        return check_launch("sort_more / query_fwd_list");          // (*fused stays false: the caller launches the loss stage)
    }
    if (pl.form == FwdForm::Packed) {
        const uint32_t W = pl.pack_waves, per_cu = W == 4u ? 2u : 1u, rows = pl.pack_rows;
        const size_t lds_free = (size_t)160u * 1024u / per_cu - packed_fixed_lds(W);
        // (each shape reserves all its workgroup can have, once: the plan's rows never need more)
        static bool attr_set[2] = {false, false};
        const size_t need = packed_lds_bytes(rows, S);
        const char* const cannot = "query_fwd_loss_packed: cannot reserve %zu bytes of LDS";
        if (int rc = W == 4u ? reserve_lds(attr_set[1], {lds_use(k_query_fwd_loss_packed<false, 4>, lds_free), lds_use(k_query_fwd_loss_packed<true, 4>, lds_free)}, cannot, lds_free)
                             : reserve_lds(attr_set[0], {lds_use(k_query_fwd_loss_packed<false, 8>, lds_free), lds_use(k_query_fwd_loss_packed<true, 8>, lds_free)}, cannot, lds_free))
            return rc;
        EarlyExit pe{};
        pe.target_d = t->target_d;
        pe.trunc_sc = f->desc.trunc * f->desc.sc_factor;
        static const int one_pass_env = env_int("NARUTO_PACK_ONE_PASS", -1);
        const bool one_pass = one_pass_env == 1;
        uint32_t rays_cap = rows * (uint32_t)kRaysPerBlock;
        if (one_pass && rays_cap * S > 64u * W && 64u * W / S >= 1u) rays_cap = 64u * W / S;           // one pass: all of a chunk's samples in one group of tiles
        const uint32_t rows_arg = rays_cap | (one_pass ? 0x100u : 0u);
#define NARUTO_LAUNCH_PACKED(BFV, WV) hipLaunchKernelGGL((k_query_fwd_loss_packed<BFV, WV>), dim3(blocks + loss.n_tv_blocks), dim3(64 * WV), need, st, f->lt, f->ut, f->bt, *p, ps, M, \
                                                         t->raw, t->feat_save, pe, loss, blocks, rows_arg, g_fwd_timeline)
        if (W == 4u) { if (bfm) NARUTO_LAUNCH_PACKED(true, 4); else NARUTO_LAUNCH_PACKED(false, 4); }
        else { if (bfm) NARUTO_LAUNCH_PACKED(true, 8); else NARUTO_LAUNCH_PACKED(false, 8); }
#undef NARUTO_LAUNCH_PACKED
        if (fused != nullptr) *fused = true;
        return check_launch("query_fwd_loss_packed");
    }
    if (pl.form == FwdForm::Short) {
        if (int rc = ray_lds_attr()) return rc;
        const uint32_t tail_blocks = wx.on ? tv_encode_blocks(loss.tv.n * loss.tv.n * loss.tv.n, wx.tv_groups) : loss.n_tv_blocks;
        // (the weight image, where the caller called it fresh: the exact mode's kernel that copies it instead of staging the weights)
        if (!bfm && wx.w_img != nullptr) hipLaunchKernelGGL(k_query_fwd_loss_short_img, dim3(blocks + tail_blocks), dim3(256), short_lds_bytes(S), st, f->lt, f->ut, f->bt, *p, ps, M, t->raw, t->feat_save, loss, blocks, wx, pl.rays_per_row, g_fwd_timeline);
        else if (bfm) hipLaunchKernelGGL(k_query_fwd_loss_short<true>, dim3(blocks + tail_blocks), dim3(256), short_lds_bytes(S), st, f->lt, f->ut, f->bt, *p, ps, M, t->raw, t->feat_save, loss, blocks, wx, pl.rays_per_row, g_fwd_timeline);
        else hipLaunchKernelGGL(k_query_fwd_loss_short<false>, dim3(blocks + tail_blocks), dim3(256), short_lds_bytes(S), st, f->lt, f->ut, f->bt, *p, ps, M, t->raw, t->feat_save, loss, blocks, wx, pl.rays_per_row, g_fwd_timeline);
        if (fused != nullptr) *fused = true;
        return check_launch("query_fwd_loss_short");
    }
    if (pl.form == FwdForm::Walk && pl.fused) {
        if (int rc = ray_lds_attr()) return rc;
        // the two-phase tile costs 32 KB of slabs per workgroup: only while two workgroups still share a CU (S <= 192), see k_query_fwd_loss
        const uint32_t tail_blocks = wx.on ? tv_encode_blocks(loss.tv.n * loss.tv.n * loss.tv.n, wx.tv_groups) : loss.n_tv_blocks;
#define NARUTO_LAUNCH_WALK(BFV, SPV) hipLaunchKernelGGL((k_query_fwd_loss<BFV, SPV>), dim3(blocks + tail_blocks), dim3(256), ray_scratch_fwd_bytes(S), st, f->lt, f->ut, f->bt, *p, ps, M, \
                                                        t->raw, t->feat_save, ee, loss, blocks, wx, g_fwd_timeline)
        if (pl.split && !bfm && wx.w_img != nullptr)          // (the weight image, where the caller called it fresh)
            hipLaunchKernelGGL(k_query_fwd_loss_img, dim3(blocks + tail_blocks), dim3(256), ray_scratch_fwd_bytes(S), st, f->lt, f->ut, f->bt, *p, ps, M, t->raw, t->feat_save, ee, loss, blocks, wx,
                               g_fwd_timeline);
        else if (pl.split) { if (bfm) NARUTO_LAUNCH_WALK(true, true); else NARUTO_LAUNCH_WALK(false, true); }
        else { if (bfm) NARUTO_LAUNCH_WALK(true, false); else NARUTO_LAUNCH_WALK(false, false); }
#undef NARUTO_LAUNCH_WALK
        if (fused != nullptr) *fused = true;
        return check_launch("query_fwd_loss");
    }
    // flat tiles in the plan's workgroup shape, or the unfused walk (full tiles only: S = 64 k)
    return launch_flat_fwd(f, *p, ps, M, t->raw, nullptr, nullptr, t->feat_save, ee, true, {blocks, pl.threads}, ee.tiles_per_ray != 0u, st);
}
// NARUTO_TRAIN_FWD_DEFER_TAIL / NARUTO_TRAIN_BWD_DEFERRED_TAIL apply up to kFusedTailMaxRays rays; beyond that both calls run the ordinary path
inline bool tail_rides_in_backward(const NarutoTrainStep* t) { return t->n_rays <= kFusedTailMaxRays && t->ray_count != nullptr; }
LossTailArgs loss_tail_args(const NarutoTrainStep* t, const TrainWs& w, uint32_t n_ray_blocks, uint32_t n_tv_blocks, float tv_inv_p3, int finalize) {
    LossTailArgs tl{};
    tl.partials = reinterpret_cast<const double*>(w.terms); tl.n_ray_blocks = n_ray_blocks;
    tl.tv_partial = w.tv_partial; tl.n_tv_blocks = n_tv_blocks; tl.tv_inv_p3 = tv_inv_p3;
    tl.sums = t->sums; tl.losses = t->losses; tl.loss_weights = t->loss_weights;
    tl.n_rays_total = t->n_rays_total ? t->n_rays_total : t->n_rays; tl.S = t->n_samples_d + t->n_range_d;
    tl.finalize = finalize;
    tl.rng = t->rng;                                        // the iteration counter advances once per forward, used or not
    tl.min_run = t->min_uncert_running;
    return tl;
}
LossStageArgs loss_stage_args(const NarutoField* f, const NarutoTrainStep* t, const TrainCtx& c) {
    const TrainWs& w = c.w;
    LossStageArgs a{};
    a.n_rays = c.N; a.S = c.S;
    a.trunc = f->desc.trunc; a.sc_factor = f->desc.sc_factor; a.trunc_sc = f->desc.trunc * f->desc.sc_factor;
    a.depth_trunc = t->depth_trunc; a.rgb_missing = t->rgb_missing; a.white_bkgd = f->desc.white_bkgd;
    a.raw = t->raw; a.z_vals = t->z_vals; a.target_rgb = t->target_rgb; a.target_d = t->target_d;
    a.rgb = t->rgb; a.depth = t->depth; a.uncert_map = t->uncert_map;
    a.partials = reinterpret_cast<double*>(w.terms);       // n_rays/4 x 16 doubles fit the n_rays x 16 floats of the modular path
    a.n_ray_blocks = (c.N + kRaysPerBlock - 1) / kRaysPerBlock;
    a.tv = c.tva; a.tv_feat = w.tv_feat; a.tv_d_list = c.bw.d_feat; a.tv_partial = w.tv_partial;
    a.tv_scale_dev = t->loss_weights != nullptr ? t->loss_weights + 8 : nullptr;
    a.tv_scale_host = t->smooth_grad_scale != 0.0f ? t->smooth_grad_scale : 1.0f;
    a.n_tv_blocks = t->smooth_points != 0 ? w.n_tv_blocks : 0u;
    if (tail_rides_in_backward(t)) a.ray_count = t->ray_count;      // list lengths for the backward's fused first launch (either flag)
    return a;
}
// The eval render's launch (naruto_render_fwd), ONE decision for the launcher and naruto_debug_render_plan:
//   Ray      S > 64: k_render_fwd, one wave per ray (four per workgroup), the ray's image in dynamic LDS
//   Packed4  S <= 64: k_render_fwd_packed<*, 256>, kPackRays rays per workgroup, samples packed into full 64-sample tiles
//   Packed8  S <= 64 from one group per CU upwards (round 6): k_render_fwd_packed<*, 512>, one eight-wave workgroup per CU whose exact-mode
//            matrix phase is the x3 chain; R8(S) rays per group.  NARUTO_RENDER_WIDE: 0 never, 1 (default) exact mode from one group per
//            CU upwards (measured, 8 192 x 43: exact mode 0.1213 -> 0.1077 ms; bf16 mode 0.1041 -> 0.1057: its chain is short either way,
//            the four-wave form stays), 2 at any ray count
// Every form loops over its ray groups with a grid capped near the CU count: rays_per_pass rays per trip.
enum class RenderForm { Ray, Packed4, Packed8 };
struct RenderPlan {
    RenderForm form;
    uint32_t rays_per_group, blocks, rays_per_pass, threads;
    size_t dyn_lds;             // dynamic LDS of the launch
    size_t reserved;            // what naruto_render_fwd reserves for the kernel (hipFuncAttributeMaxDynamicSharedMemorySize), for any S it may get
    size_t static_lds;          // the kernel's static LDS (the larger of its two MLP modes' forms is what the reservation has to fit next to)
};
// the eight-wave form's reservation: its largest launch over every S it runs at
inline size_t render_packed8_reserve() {
    size_t m = 0;
    for (uint32_t S = 2; S <= 64u; ++S) {
        const size_t b = render_packed_lds_bytes(S, render_packed8_rays(S));
        if (b > m) m = b;
    }
    return m;
}
RenderPlan render_plan(const NarutoField* f, uint32_t n_rays, uint32_t S, bool bf, int wide) {
    static const int wide_env = env_int("NARUTO_RENDER_WIDE", 1);
    if (wide < 0) wide = wide_env;
    RenderPlan pl{};
    const uint32_t cap = cu_count(f) * 4u;
    if (S <= 64u) {
        const uint32_t R8 = render_packed8_rays(S);
        if (wide != 0 && R8 >= 8u && (wide == 2 || (!bf && (n_rays + R8 - 1u) / R8 >= cu_count(f)))) {
            pl.form = RenderForm::Packed8;
            pl.rays_per_group = R8;
            pl.blocks = (n_rays + R8 - 1u) / R8 < cu_count(f) ? (n_rays + R8 - 1u) / R8 : cu_count(f);
            pl.rays_per_pass = cu_count(f) * R8;
            pl.threads = 512u;
            pl.dyn_lds = render_packed_lds_bytes(S, R8);
            pl.reserved = render_packed8_reserve();
            pl.static_lds = (bf ? sizeof(FwdLdsBf) : sizeof(FwdLdsX3)) + 8u * sizeof(FwdSlab);
            return pl;
        }
        pl.form = RenderForm::Packed4;
        pl.rays_per_group = kPackRays;
        pl.blocks = (n_rays + kPackRays - 1u) / kPackRays < cap ? (n_rays + kPackRays - 1u) / kPackRays : cap;
        pl.rays_per_pass = cap * kPackRays;
        pl.threads = 256u;
        pl.dyn_lds = render_packed_lds_bytes(S);
        pl.reserved = render_packed_lds_bytes(64u);
        pl.static_lds = (bf ? sizeof(FwdLdsBf) : sizeof(FwdLds)) + 4u * sizeof(FwdSlab);
        return pl;
    }
    pl.form = RenderForm::Ray;
    pl.rays_per_group = 4u;
    pl.blocks = (n_rays + 3u) / 4u < cap ? (n_rays + 3u) / 4u : cap;
    pl.rays_per_pass = cap * 4u;
    pl.threads = 256u;
    pl.dyn_lds = ray_scratch_bytes(S);
    pl.reserved = ray_scratch_bytes(kMaxSamples);
    pl.static_lds = bf ? sizeof(FwdLdsBf) : sizeof(FwdLds);
    return pl;
}
}  // namespace

size_t naruto_train_workspace(const NarutoField* f, const NarutoTrainStep* t) {
    if (f == nullptr || t == nullptr) return 0;
    NarutoTrainStep c = *t;
    c.workspace = nullptr;
    return train_ws(f, &c).total;
}

// (advisor, round 5) NARUTO_TRAIN_FWD_SUMS_TV_LATER and NARUTO_TRAIN_BWD_TV_MOVED must be paired: a forward that LEFT the smoothness term to the backward,
// followed by a backward that is not told so, would silently drop the term (no value, stale cotangents on the front list).  The training workspaces whose
// LAST forward left the term are kept in a set (host side, under a mutex: fields and steps may be used from several threads): every forward inserts or
// erases its workspace, naruto_train_backward looks its own up and refuses the mismatch.  The one limit: a workspace freed in that state whose address is
// handed out again passes the flag on to the new owner until that one's first forward.
namespace {
std::mutex g_tv_later_mutex;
std::unordered_set<const void*> g_tv_later;
void note_tv_left(const void* ws, bool left) {
    const std::lock_guard<std::mutex> lock(g_tv_later_mutex);
    if (left) g_tv_later.insert(ws);
    else g_tv_later.erase(ws);
}
bool tv_was_left(const void* ws) {
    const std::lock_guard<std::mutex> lock(g_tv_later_mutex);
    return g_tv_later.count(ws) != 0u;
}
}  // namespace

int naruto_train_forward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, int finalize, void* stream) {
    if (int rc = train_check(f, p, t, "train_forward")) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const TrainCtx c = train_ctx(f, t);
    const uint32_t N = c.N, S = c.S;
    const TrainWs& w = c.w;
    // (the smoothness term is left to the backward: the single-process deferred tail, or the data-parallel SUMS_TV_LATER form)
    const bool deferred_ = (finalize == NARUTO_TRAIN_FWD_DEFER_TAIL || finalize == NARUTO_TRAIN_FWD_SUMS_TV_LATER) && tail_rides_in_backward(t);
    const TrainFwdPlan pl = train_fwd_plan(f, t, true, deferred_);
    const WalkExtra wx = walk_extra(f, t, c, pl);
    note_tv_left(t->workspace, finalize == NARUTO_TRAIN_FWD_SUMS_TV_LATER && pl.tv_moved);
    // A1 (+ the smoothness lattice: its points go straight to the FRONT of the backward's scatter list, features level-major); with the term moved
    // the walk samples the depths itself and its tail workgroups encode the lattice (walk_extra)
    SampleArgs sa = c.sample_args(t);
    if (!pl.tv_moved && t->smooth_points != 0) {
        static const int dbg_roles = env_int("NARUTO_DEBUG_SAMPLE_ROLES", 3);   // profiling knob: 1 rays, 2 lattice
        if (dbg_roles == 2) sa.n_rays = 0;
        hipLaunchKernelGGL(k_sample_encode, dim3(sa.n_ray_blocks + (dbg_roles == 1 ? 0u : tv_encode_blocks(w.n3))), dim3(256), (size_t)4u * 2u * S * sizeof(float), st, sa, f->lt,
                           f->bt, c.tva, t->rand6, t->rng, reinterpret_cast<const float2*>(p->table), c.bw.x_soa, w.tv_feat);
        if (int rc = check_launch("sample_encode")) return rc;
    } else if (!pl.tv_moved) {
        hipLaunchKernelGGL(k_sample_z, dim3(N), dim3(64), 0, st, N, sa.target_d, sa.near_, sa.far_, sa.nu, sa.nr, sa.range_d, sa.rand, sa.rng, sa.z_vals);
        if (int rc = check_launch("sample_z")) return rc;
    }
    // A2..A5 and A6..A8 (+ the lattice's TV term): one launch where the forward walks one ray per wave, else two; then the one-workgroup tail
    LossStageArgs a = loss_stage_args(f, t, c);
    const bool deferred = finalize == NARUTO_TRAIN_FWD_DEFER_TAIL && tail_rides_in_backward(t);
    if (int rc = ray_lds_attr()) return rc;
    bool loss_done = false;
    if (int rc = launch_train_query(f, p, t, c, pl, st, a, wx, &loss_done)) return rc;
    if (!loss_done) {
        static const int dbg_ls_roles = env_int("NARUTO_DEBUG_LOSS_STAGE_ROLES", 3);     // profiling knob: 1 rays, 2 lattice
        if (dbg_ls_roles == 1) a.n_tv_blocks = 0;
        if (dbg_ls_roles == 2) a.n_rays = 0;
        hipLaunchKernelGGL(k_loss_stage, dim3(a.n_ray_blocks + a.n_tv_blocks), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), st, a);
        if (int rc = check_launch("loss_stage")) return rc;
    }
    if (deferred) return NARUTO_OK;                          // the tail is a workgroup of the backward's first launch
    const uint32_t n_rows = loss_done ? loss_rows(pl, N) : a.n_ray_blocks;      // rows of partial sums the loss stage left
    // (SUMS_TV_LATER with the term moved: nothing has evaluated it yet -- the tail writes losses[8] = 0, the backward adds the value)
    LossTailArgs tl = loss_tail_args(t, w, n_rows, wx.on != 0u ? 0u : a.n_tv_blocks, c.tva.inv_p3,
                                     finalize == 1 || finalize == NARUTO_TRAIN_FWD_DEFER_TAIL);      // (DEFER_TAIL beyond kFusedTailMaxRays rays: the ordinary tail, here)
    if (n_rows > 4u * kTailRows) {          // large batch: fold the per-workgroup rows first
        hipLaunchKernelGGL(k_loss_fold, dim3(kTailRows), dim3(64), 0, st, tl.partials, n_rows, w.fold);
        if (int rc = check_launch("loss_fold")) return rc;
        tl.partials = w.fold; tl.n_ray_blocks = kTailRows;
    }
    hipLaunchKernelGGL(k_loss_tail, dim3(1), dim3(256), 0, st, tl);
    return check_launch("loss_tail");
}

int naruto_train_finalize(const NarutoField* f, const NarutoTrainStep* t, void* stream) {
    if (f == nullptr || t == nullptr || t->sums == nullptr || t->losses == nullptr) return fail(NARUTO_ERR_INVALID, "train_finalize: NULL argument");
    const uint32_t S = t->n_samples_d + t->n_range_d;
    hipLaunchKernelGGL(k_loss_finalize_total, dim3(1), dim3(64), 0, (hipStream_t)stream, t->sums, t->n_rays_total ? t->n_rays_total : t->n_rays, S, t->losses,
                       t->loss_weights, t->min_uncert_running);
    return check_launch("loss_finalize_total");
}

size_t naruto_fwd_image_bytes(size_t* image_bytes, uint32_t* n_weights) {
    if (image_bytes != nullptr) *image_bytes = kFwdImageBytes;
    if (n_weights != nullptr) *n_weights = (uint32_t)kNumWeights;
    return fwd_image_ws(nullptr).total;
}

namespace {
const uint32_t* fwd_image_slots_host() {
    static const std::vector<uint32_t> slots = [] { std::vector<uint32_t> s((size_t)kNumWeights); fwd_image_slot_map(s.data(), nullptr); return s; }();
    return slots.data();
}
int fwd_image_args(const NarutoField* f, const NarutoParams* p, const void* buf, const char* who) {
    if (f == nullptr || p == nullptr || buf == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL argument", who);
    if (int rc = check_params(p, who, kParamsSdf | kParamsColour, "NULL weights")) return rc;
    if ((reinterpret_cast<uintptr_t>(buf) & 15u) != 0u) return fail(NARUTO_ERR_INVALID, "%s: the buffer must be 16-byte aligned", who);
    return NARUTO_OK;
}
}  // namespace

int naruto_fwd_image_init(const NarutoField* f, const NarutoParams* p, void* fwd_image, void* stream) {
    if (int rc = fwd_image_args(f, p, fwd_image, "fwd_image_init")) return rc;
    const FwdImageWs w = fwd_image_ws(fwd_image);
    if (hipMemcpyAsync(w.slots, fwd_image_slots_host(), (size_t)kNumWeights * sizeof(uint32_t), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
        return fail(NARUTO_ERR_LAUNCH, "fwd_image_init: slot upload: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(k_fwd_image_init, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, static_cast<FwdLdsX3*>(w.image));
    return check_launch("fwd_image_init");
}

int naruto_debug_fwd_image(const NarutoField* f, const NarutoParams* p, void* out, void* stream) {
    if (int rc = fwd_image_args(f, p, out, "debug_fwd_image")) return rc;
    hipLaunchKernelGGL(k_debug_fwd_image, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, static_cast<uint4*>(out));
    return check_launch("debug_fwd_image");
}

int naruto_debug_fwd_image_map(uint32_t* slots, uint8_t* zero_fill) {
    if (slots == nullptr) return fail(NARUTO_ERR_INVALID, "debug_fwd_image_map: NULL argument");
    fwd_image_slot_map(slots, zero_fill);
    return NARUTO_OK;
}

// profiling: device buffer of 16 x (workgroups) uint64 the packed training forward stamps s_memtime into (NULL: off) -- the per-step timeline of
// k_query_fwd_loss_packed's first chunk, see its header
int naruto_debug_fwd_timeline(void* device_buffer) {
    g_fwd_timeline = static_cast<unsigned long long*>(device_buffer);
    return NARUTO_OK;
}

// profiling: device buffer of kBwdTlSlots x 4 waves x kBwdMaxBlocks uint64; while it is set the fp32 MLP backward launches k_query_bwd_timeline,
// the stamped build of k_query_bwd (NULL: off, the product kernel) -- tools/bwd_timeline.py
int naruto_debug_bwd_timeline(void* device_buffer) {
    g_bwd_timeline = static_cast<unsigned long long*>(device_buffer);
    return NARUTO_OK;
}

// the dynamic LDS the launcher reserves for k_query_bwd and passes to its launches (the kernel has no static LDS): weight images + per-wave stages
size_t naruto_debug_query_bwd_lds_bytes(void) { return sizeof(BwdLds); }

int naruto_debug_train_query_fwd(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, void* stream) {
    if (int rc = train_check(f, p, t, "debug_train_query_fwd")) return rc;
    // exactly the launch naruto_train_forward issues for the field query: with the loss stage riding in it where that applies
    const TrainCtx c = train_ctx(f, t);
    // (the five-launch iteration's form of it -- depth sampling in the walk, the lattice encode in its tail workgroups -- where the trainer's
    // iteration takes that form; the jitter is whatever the step's generator state gives: timing only)
    const TrainFwdPlan pl = train_fwd_plan(f, t, true, tail_rides_in_backward(t));
    return launch_train_query(f, p, t, c, pl, (hipStream_t)stream, loss_stage_args(f, t, c), walk_extra(f, t, c, pl), nullptr);
}

// profiling: k_hash_scatter_lds ALONE over the point list the last naruto_train_backward left in the workspace, in the launch shape
// the iteration uses (lattice front + active samples, level units + uncertainty-grid units); writes only the partial tables
int naruto_debug_train_scatter(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, void* stream) {
    if (int rc = train_check(f, p, t, "debug_train_scatter")) return rc;
    if (f->bplan.n_levels != 0) return fail(NARUTO_ERR_INVALID, "debug_train_scatter: this field has binned levels (the tiled launch is not its whole scatter)");
    const TrainCtx c = train_ctx(f, t);
    const uint32_t cap = c.cap;
    const BwdWs& bw = c.bw;
    const uint32_t n_front = t->smooth_points != 0 ? c.w.n3 : 0u;
    const uint32_t* cnt = n_front > 0 ? bw.n_total : t->n_active;
    const float* unc_g = f->plan.n_uncert != 0 ? bw.x_soa + 3u * (size_t)cap : nullptr;
    // d_table / d_uncert only select the roles here: without the reduce nothing is written through them
    return launch_scatter(f, list_points(bw.x_soa, cap), cap, bw.d_feat, (size_t)2, (size_t)2 * (size_t)cap, const_cast<float*>(p->table), bw.scatter_ws, (hipStream_t)stream, cnt, nullptr, 1, false,
                          nullptr, unc_g, unc_g != nullptr ? const_cast<float*>(p->uncert_grid) : nullptr, n_front);
}

// testing: the table scatter over a caller-made point list in the TRAINING layout (x_soa [3][cap], d_feat [16][cap][2], cap % 4 == 0, the count
// on the device) -- the hashed units' list route with prescribed cotangents, which the public backward derives itself.  Adds into d_table, as
// naruto_hash_encode_bwd does over the generic layout: same count, same plan, same split bounds.
int naruto_debug_scatter_list(const NarutoField* f, uint32_t cap, const uint32_t* n_dev, const float* x_soa, const float* d_feat, float* d_table,
                              void* workspace, void* stream) {
    if (f == nullptr || n_dev == nullptr || x_soa == nullptr || d_feat == nullptr || d_table == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "debug_scatter_list: NULL argument");
    if (cap == 0 || (cap & 3u) != 0u) return fail(NARUTO_ERR_INVALID, "debug_scatter_list: the list's capacity must be a positive multiple of 4");
    return launch_scatter(f, list_points(x_soa, cap), cap, d_feat, (size_t)2, (size_t)2 * (size_t)cap, d_table, workspace, (hipStream_t)stream, n_dev);
}

namespace {
int assemble_args(const NarutoRayBatch* b, bool need_out, AssembleArgs& a, const char* who);

LossArgs train_loss_args(const NarutoField* f, const NarutoTrainStep* t) {
    return LossArgs{t->target_rgb, t->target_d, t->sums, t->loss_weights, t->n_rays_total ? t->n_rays_total : t->n_rays, t->depth_trunc, t->rgb_missing,
                    f->desc.trunc * f->desc.sc_factor};
}

// The loss block's backward (k_composite_bwd: d_raw and the per-ray sample counts) and the compaction of the samples whose cotangent
// is not zero into the active list (k_count_blocks for large batches, then k_compact), after a forward that finalised its losses: the
// sequence naruto_train_backward runs where the tail was not deferred, and naruto_track_backward in front of the point gradients.
int loss_bwd_compact(const NarutoField* f, const NarutoTrainStep* t, const TrainWs& w, const LossArgs& la, uint32_t n_front, uint32_t* n_total, hipStream_t st) {
    const uint32_t N = t->n_rays, S = t->n_samples_d + t->n_range_d;
    CompositeCot cot{};
    hipLaunchKernelGGL(k_composite_bwd<true>, dim3((N + kRaysPerBlock - 1) / kRaysPerBlock), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), st, N, S, f->desc.trunc,
                       f->desc.sc_factor, f->desc.white_bkgd, t->raw, t->z_vals, cot, la, t->d_raw, 0, t->ray_count);
    if (int rc = check_launch("loss_bwd")) return rc;
    const uint32_t* block_sums = nullptr;
    if (N > 4u * kCompactBlock) {     // large batch: two-level prefix of the per-ray counts
        hipLaunchKernelGGL(k_count_blocks, dim3((N + kCompactBlock - 1u) / kCompactBlock), dim3(256), 0, st, N, t->ray_count, w.block_sums);
        if (int rc = check_launch("count_blocks")) return rc;
        block_sums = w.block_sums;
    }
    hipLaunchKernelGGL(k_compact, dim3((N + 3u) / 4u), dim3(256), 0, st, N, S, t->ray_count, t->ray_offset, t->active_idx, t->n_active, n_front, n_total,
                       block_sums);
    return check_launch("compact");
}
}  // namespace

namespace {
int ba_poses_check(const NarutoBAPoses* b, const NarutoTrainStep* t, bool backward, const char* who);
int ba_poses_launch(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoBAPoses* b, hipStream_t st);
}  // namespace

int naruto_train_backward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t_in, const NarutoGrads* g, uint32_t flags,
                          const NarutoFusedAdam* opt, void* stream) {
    return naruto_train_backward_poses(f, p, t_in, g, flags, opt, nullptr, stream);
}

// naruto_train_backward's body; bap != NULL: the iteration's pose gradients and the pose step ride between the loss backward and the
// launches that scatter and step the network (see naruto_bapose.hip)
int naruto_train_backward_poses(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t_in, const NarutoGrads* g, uint32_t flags,
                                const NarutoFusedAdam* opt, const NarutoBAPoses* bap, void* stream) {
    if (int rc = train_check(f, p, t_in, "train_backward")) return rc;
    if (bap != nullptr) {
        if (flags & (NARUTO_TRAIN_BWD_MLP_ONLY | NARUTO_TRAIN_BWD_TABLE_ONLY | NARUTO_TRAIN_BWD_SUMS_GIVEN))
            return fail(NARUTO_ERR_INVALID, "train_backward_poses: pose refinement belongs to the one-piece single-process backward");
        if (int rc = ba_poses_check(bap, t_in, true, "train_backward_poses")) return rc;
    }
    const hipStream_t st = (hipStream_t)stream;
    const TrainCtx c = train_ctx(f, t_in);          // (nothing in it reads the loss weights, which the next lines may swap)
    const TrainWs& w = c.w;
    const BwdWs& bw = c.bw;
    const uint32_t N = c.N, S = c.S, M = c.M;
    // loss weights given as separate device scalars: gather them (+ the vector, if any) into the workspace first
    NarutoTrainStep t_local;
    const NarutoTrainStep* t = t_in;
    bool parts = false;
    for (int i = 0; i < 10; ++i) parts = parts || t_in->loss_weight_parts[i] != nullptr;
    if (parts) {
        if ((flags & NARUTO_TRAIN_BWD_TABLE_ONLY) == 0u) {           // (TABLE_ONLY: gathered by the preceding MLP_ONLY call)
            WeightParts wp{};
            for (int i = 0; i < 10; ++i) wp.part[i] = t_in->loss_weight_parts[i];
            wp.base = t_in->loss_weights;
            hipLaunchKernelGGL(k_gather_loss_weights, dim3(1), dim3(64), 0, st, wp, w.w10);
            if (int rc = check_launch("gather_loss_weights")) return rc;
        }
        t_local = *t_in;
        t_local.loss_weights = w.w10;
        t = &t_local;
    }
    AdamFuse adam{};
    if (opt != nullptr) {
        if (opt->step_dev == nullptr) return fail(NARUTO_ERR_INVALID, "train_backward: the fused optimiser needs step_dev");
        for (int k = 0; k < 5; ++k) {
            if (opt->param[k] == nullptr || opt->exp_avg[k] == nullptr || opt->exp_avg_sq[k] == nullptr)
                return fail(NARUTO_ERR_INVALID, "train_backward: NULL tensor %d in NarutoFusedAdam", k);
            adam.p[k] = opt->param[k]; adam.m[k] = opt->exp_avg[k]; adam.v[k] = opt->exp_avg_sq[k];
            adam.lr[k] = opt->lr[k]; adam.eps[k] = opt->eps[k]; adam.wd[k] = opt->weight_decay[k];
        }
        adam.b1 = opt->beta1; adam.b2 = opt->beta2; adam.step_dev = opt->step_dev; adam.on = 1;
        // the finishing launch keeps the forward's weight image in step with the weights it updates (exact mode; whoever reads it decides per forward)
        if (f->desc.mlp_mode != NARUTO_MLP_BF16) adam.fwd_img = t_in->fwd_image;
    }
    UncertAdam unc_adam{};
    if (opt != nullptr && opt->uncert_step != 0u) {
        if (opt->uncert_exp_avg == nullptr || opt->uncert_exp_avg_sq == nullptr || opt->uncert_step_dev == nullptr)
            return fail(NARUTO_ERR_INVALID, "train_backward: NarutoFusedAdam.uncert_step needs the grid's moments and step word");
        unc_adam.on = 1; unc_adam.m = opt->uncert_exp_avg; unc_adam.v = opt->uncert_exp_avg_sq; unc_adam.step_dev = opt->uncert_step_dev;
        unc_adam.lag = opt->uncert_step_lag; unc_adam.lr = opt->uncert_lr; unc_adam.eps = opt->uncert_eps; unc_adam.wd = opt->uncert_weight_decay;
        unc_adam.b1 = opt->uncert_beta1; unc_adam.b2 = opt->uncert_beta2;
    }
    if (g == nullptr || t->loss_weights == nullptr || t->feat_save == nullptr || t->d_raw == nullptr || t->ray_count == nullptr || t->ray_offset == nullptr ||
        t->active_idx == nullptr || t->n_active == nullptr)
        return fail(NARUTO_ERR_INVALID, "train_backward: NULL buffer");
    const LossArgs la = train_loss_args(f, t);
    if ((flags & NARUTO_TRAIN_BWD_MLP_ONLY) && (flags & NARUTO_TRAIN_BWD_TABLE_ONLY)) return fail(NARUTO_ERR_INVALID, "train_backward: pick one phase");
    const bool table_only = (flags & NARUTO_TRAIN_BWD_TABLE_ONLY) != 0u;
    if ((flags & NARUTO_TRAIN_BWD_DEFERRED_TAIL) && (flags & (NARUTO_TRAIN_BWD_MLP_ONLY | NARUTO_TRAIN_BWD_TABLE_ONLY | NARUTO_TRAIN_BWD_SUMS_GIVEN)))
        return fail(NARUTO_ERR_INVALID, "train_backward: the deferred tail belongs to the one-piece single-process backward");
    const bool sums_given = (flags & NARUTO_TRAIN_BWD_SUMS_GIVEN) != 0u && !table_only;
    const bool deferred = ((flags & NARUTO_TRAIN_BWD_DEFERRED_TAIL) != 0u || sums_given) && tail_rides_in_backward(t);
    if (sums_given && !deferred) {           // too many rays for the fused launch: the ordinary finalize, then the ordinary sequence
        if (int rc = naruto_train_finalize(f, t, stream)) return rc;
    }
    if (int rc = ray_lds_attr()) return rc;
    // the smoothness term moved into this backward only where the FORWARD was told to defer its tail (NARUTO_TRAIN_BWD_DEFERRED_TAIL): with
    // NARUTO_TRAIN_BWD_SUMS_GIVEN (data parallel, the autograd node) the forward ran k_sample_encode, evaluated the term itself and its
    // value is already in losses[8] -- evaluating it here again would count it twice in the total (round-4 advisor finding)
    // the plan of this step's forward as the first half of one iteration (`deferred` decides tv_moved and nothing else: the form is any forward's)
    const TrainFwdPlan pl = train_fwd_plan(f, t, true, true);
    const bool moved = (flags & (NARUTO_TRAIN_BWD_DEFERRED_TAIL | NARUTO_TRAIN_BWD_TV_MOVED)) != 0u && deferred && pl.tv_moved;
    if ((flags & NARUTO_TRAIN_BWD_TV_MOVED) != 0u && !sums_given && !table_only)
        return fail(NARUTO_ERR_INVALID, "train_backward: NARUTO_TRAIN_BWD_TV_MOVED belongs to NARUTO_TRAIN_BWD_SUMS_GIVEN (a forward with NARUTO_TRAIN_FWD_SUMS_TV_LATER)");
    if (sums_given && !table_only && (flags & NARUTO_TRAIN_BWD_TV_MOVED) == 0u && tv_was_left(t_in->workspace))
        return fail(NARUTO_ERR_INVALID, "train_backward: the forward on this workspace ran with NARUTO_TRAIN_FWD_SUMS_TV_LATER (it left the smoothness term to the "
                                        "backward): pass NARUTO_TRAIN_BWD_TV_MOVED with NARUTO_TRAIN_BWD_SUMS_GIVEN, or the term is dropped");
    if (deferred) {
        const bool smooth_d = t->smooth_points != 0 && (g->table != nullptr || opt != nullptr);
        FusedBwdArgs fa{};
        fa.n_rays = N; fa.S = S; fa.trunc = f->desc.trunc; fa.sc_factor = f->desc.sc_factor; fa.white_bkgd = f->desc.white_bkgd;
        fa.raw = t->raw; fa.z_vals = t->z_vals; fa.la = la; fa.d_raw = t->d_raw;
        fa.partials = reinterpret_cast<const double*>(w.terms); fa.n_ray_blocks = (N + kRaysPerBlock - 1) / kRaysPerBlock;
        fa.ray_count = t->ray_count; fa.ray_off = t->ray_offset; fa.active_idx = t->active_idx; fa.n_active = t->n_active;
        fa.n_front = smooth_d ? w.n3 : 0u; fa.n_list = bw.n_total;
        // (the term moved into this launch: the tail cannot see its partial sums -- the last launch of the backward adds the value, TvLate)
        // rows the forward's loss stage left: the plan's, when this backward belongs to a forward that deferred its tail (sums_given: unused)
        fa.n_rows = (flags & (NARUTO_TRAIN_BWD_DEFERRED_TAIL | NARUTO_TRAIN_BWD_TV_MOVED)) != 0u ? loss_rows(pl, N) : fa.n_ray_blocks;
        fa.tail = loss_tail_args(t, w, fa.n_rows, (t->smooth_points != 0 && !moved) ? w.n_tv_blocks : 0u, c.tva.inv_p3, 1);
        fa.sums_given = sums_given ? 1 : 0;
        // one more workgroup prepares the MLP backward's weight images (the parameters do not change before k_query_bwd reads them)
        fa.w_img = w.w_img; fa.w_bf = f->desc.mlp_mode == NARUTO_MLP_BF16 ? 1 : 0; fa.params = *p;
        if (moved) {
            fa.tv = c.tva; fa.tv_feat = w.tv_feat; fa.tv_d_list = bw.d_feat; fa.tv_partial = w.tv_partial;
            fa.tv_scale_dev = t->loss_weights != nullptr ? t->loss_weights + 8 : nullptr;
            fa.tv_scale_host = t->smooth_grad_scale != 0.0f ? t->smooth_grad_scale : 1.0f;
            fa.tv_n_blocks = w.n_tv_blocks;
        }
        hipLaunchKernelGGL(k_loss_bwd_fused, dim3(fa.n_ray_blocks + 2u + fa.tv_n_blocks), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), st, fa);
        if (int rc = check_launch("loss_bwd_fused")) return rc;
    }
    const bool smooth = t->smooth_points != 0 && (g->table != nullptr || opt != nullptr);
    const uint32_t n_front = smooth ? w.n3 : 0u;
    if (!table_only && !deferred) {
        if (int rc = loss_bwd_compact(f, t, w, la, n_front, bw.n_total, st)) return rc;
    }
    // pose refinement: d_raw and the active list are there, the parameters are still the ones the forward used, and the launch that
    // assembles the next batch (below) comes after the pose step
    if (bap != nullptr) {
        if (int rc = ba_poses_launch(f, p, t, bap, st)) return rc;
    }
    NarutoPoints pts{};
    pts.rays_o = t->rays_o; pts.rays_d = t->rays_d; pts.z_vals = t->z_vals; pts.n_samples = S;
    const AdamFuse* ad = opt != nullptr ? &adam : nullptr;
    // the next iteration's ray batch assembled by the launch that finishes this one's gradients (NarutoFusedAdam.next_batch)
    AssembleArgs next_args{};
    const AssembleArgs* next = nullptr;
    if (opt != nullptr && opt->next_batch != nullptr) {
        if (int rc2 = assemble_args(opt->next_batch, true, next_args, "train_backward (next_batch)")) return rc2;
        if (next_args.n_global + next_args.n_cur != 0u) next = &next_args;
    }
    TvLate tvl{};
    if (moved) { tvl.tv_partial = w.tv_partial; tvl.n_tv_blocks = w.n_tv_blocks; tvl.inv_p3 = c.tva.inv_p3; tvl.losses = t->losses; tvl.loss_weights = t->loss_weights; }
    QueryBwd q{};
    q.M = M; q.pts = &pts; q.feat_save = t->feat_save; q.d_raw = t->d_raw;
    q.active_idx = t->active_idx; q.n_active = t->n_active;
    q.flags = flags; q.g = g; q.workspace = w.bwd; q.stream = st;
    q.n_front = n_front;            // (0: no smoothness term in this backward -- the list is the samples alone, in a workspace sized for cap = M + n3)
    q.n_list_dev = n_front > 0 ? bw.n_total : nullptr;
    q.adam = ad;
    q.unc_adam = unc_adam.on ? &unc_adam : nullptr;
    q.w_img = deferred ? w.w_img : nullptr;                      // prepared by k_loss_bwd_fused just above
    q.tv_late = (moved && ad != nullptr) ? &tvl : nullptr;
    q.next = next;
    q.feat_sample_major = pl.form == FwdForm::Sorted;            // the layout the forward of this plan left feat_save in
    if (int rc = query_bwd_impl(f, p, q)) return rc;
    if (moved && ad == nullptr) {                                 // no optimiser in the backward: the value gets a (tiny) launch of its own
        hipLaunchKernelGGL(k_tv_late, dim3(1), dim3(256), 0, st, tvl);
        return check_launch("tv_late");
    }
    return NARUTO_OK;
}

int naruto_render_fwd(const NarutoField* f, const NarutoParams* p, const NarutoRender* r, void* stream) {
    if (f == nullptr || p == nullptr || r == nullptr) return fail(NARUTO_ERR_INVALID, "render_fwd: NULL argument");
    if (int rc = check_params(p, "render_fwd")) return rc;
    if (r->n_rays == 0) return NARUTO_OK;
    if (r->rays_o == nullptr || r->rays_d == nullptr) return fail(NARUTO_ERR_INVALID, "render_fwd: NULL rays");
    RenderArgs a{};
    a.n_rays = r->n_rays; a.rays_o = r->rays_o; a.rays_d = r->rays_d; a.target_d = r->target_d;
    a.near_ = r->near_; a.far_ = r->far_; a.range_d = r->range_d;
    if (r->target_d != nullptr) { a.nu = r->n_samples_d; a.nr = r->n_range_d; }
    else { a.nu = r->n_samples; a.nr = 0; }
    const uint32_t S = a.nu + a.nr;
    if (S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "render_fwd: need 2 <= samples per ray <= %d (got %u)", kMaxSamples, S);
    a.rand = r->rand; a.rng = r->rng;
    a.trunc = f->desc.trunc; a.sc_factor = f->desc.sc_factor; a.white_bkgd = f->desc.white_bkgd;
    a.rgb = r->rgb; a.depth = r->depth; a.disp = r->disp; a.acc = r->acc; a.depth_var = r->depth_var; a.uncert_map = r->uncert_map;
    a.weights = r->weights; a.raw = r->raw; a.z_vals = r->z_vals;
    const bool bf = f->desc.mlp_mode == NARUTO_MLP_BF16;
    const RenderPlan pl = render_plan(f, r->n_rays, S, bf, -1);
    // every kernel reserves, once, the dynamic LDS of the largest launch it may get (render_plan's reserved)
    static bool attr_set[3] = {false, false, false};
    const void* fn_fp32 = pl.form == RenderForm::Ray ? reinterpret_cast<const void*>(k_render_fwd<false>)
                        : pl.form == RenderForm::Packed4 ? reinterpret_cast<const void*>(k_render_fwd_packed<false, 256>) : reinterpret_cast<const void*>(k_render_fwd_packed<false, 512>);
    const void* fn_bf = pl.form == RenderForm::Ray ? reinterpret_cast<const void*>(k_render_fwd<true>)
                      : pl.form == RenderForm::Packed4 ? reinterpret_cast<const void*>(k_render_fwd_packed<true, 256>) : reinterpret_cast<const void*>(k_render_fwd_packed<true, 512>);
    if (int rc = reserve_lds(attr_set[(int)pl.form], {LdsUse{fn_fp32, pl.reserved}, LdsUse{fn_bf, pl.reserved}}, "render_fwd: cannot reserve %zu bytes of LDS", pl.reserved)) return rc;
    if (pl.dyn_lds > pl.reserved) return fail(NARUTO_ERR_LAUNCH, "render_fwd: %zu bytes of dynamic LDS, %zu reserved", pl.dyn_lds, pl.reserved);
    const hipStream_t st = (hipStream_t)stream;
    if (pl.form == RenderForm::Packed8) {
        if (bf) hipLaunchKernelGGL((k_render_fwd_packed<true, 512>), dim3(pl.blocks), dim3(512), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a, pl.rays_per_group);
        else hipLaunchKernelGGL((k_render_fwd_packed<false, 512>), dim3(pl.blocks), dim3(512), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a, pl.rays_per_group);
        return check_launch("render_fwd_packed8");
    }
    if (pl.form == RenderForm::Packed4) {
        if (bf) hipLaunchKernelGGL((k_render_fwd_packed<true, 256>), dim3(pl.blocks), dim3(256), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a, pl.rays_per_group);
        else hipLaunchKernelGGL((k_render_fwd_packed<false, 256>), dim3(pl.blocks), dim3(256), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a, pl.rays_per_group);
        return check_launch("render_fwd_packed");
    }
    if (bf) hipLaunchKernelGGL(k_render_fwd<true>, dim3(pl.blocks), dim3(256), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a);
    else hipLaunchKernelGGL(k_render_fwd<false>, dim3(pl.blocks), dim3(256), pl.dyn_lds, st, f->lt, f->ut, f->bt, *p, a);
    return check_launch("render_fwd");
}

int naruto_debug_render_plan(const NarutoField* f, uint32_t n_rays, uint32_t S, int bf16, int wide, uint32_t out[8]) {
    if (f == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_render_plan: NULL argument");
    if (S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "debug_render_plan: need 2 <= samples per ray <= %d (got %u)", kMaxSamples, S);
    if (wide < -1 || wide > 2) return fail(NARUTO_ERR_INVALID, "debug_render_plan: wide must be -1, 0, 1 or 2 (got %d)", wide);
    const RenderPlan pl = render_plan(f, n_rays, S, bf16 != 0, wide);
    out[0] = (uint32_t)pl.form; out[1] = pl.rays_per_group; out[2] = pl.blocks; out[3] = pl.rays_per_pass;
    out[4] = (uint32_t)pl.dyn_lds; out[5] = (uint32_t)pl.reserved; out[6] = (uint32_t)pl.static_lds; out[7] = pl.threads;
    return NARUTO_OK;
}

int naruto_debug_train_plan(const NarutoField* f, const NarutoTrainStep* t, int with_loss, int deferred, uint32_t out[8]) {
    if (f == nullptr || t == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_train_plan: NULL argument");
    const uint32_t S = t->n_samples_d + t->n_range_d;
    if (t->n_rays == 0 || S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "debug_train_plan: need rays and 2..%d samples per ray", kMaxSamples);
    const TrainFwdPlan pl = train_fwd_plan(f, t, with_loss != 0, deferred != 0);
    out[0] = (uint32_t)pl.form; out[1] = pl.fused; out[2] = pl.split; out[3] = pl.tv_moved;
    out[4] = pl.tpr; out[5] = pl.rays_per_row; out[6] = pl.blocks; out[7] = pl.threads;
    return NARUTO_OK;
}

int naruto_composite_fwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals, float* rgb, float* disp,
                         float* acc, float* weights, float* depth, float* depth_var, float* uncert_map, void* stream) {
    if (f == nullptr || raw == nullptr || z_vals == nullptr) return fail(NARUTO_ERR_INVALID, "composite_fwd: NULL argument");
    if (S < 1 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "composite_fwd: samples per ray must be in [1, %d]", kMaxSamples);
    if (n_rays == 0) return NARUTO_OK;
    if (int rc = ray_lds_attr()) return rc;
    hipLaunchKernelGGL(k_composite_fwd, dim3((n_rays + kRaysPerBlock - 1) / kRaysPerBlock), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), (hipStream_t)stream, n_rays, S,
                       f->desc.trunc, f->desc.sc_factor, f->desc.white_bkgd, raw, z_vals, rgb, disp, acc, weights, depth, depth_var, uncert_map);
    return check_launch("composite_fwd");
}

int naruto_composite_bwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals, const float* d_rgb,
                         const float* d_disp, const float* d_acc, const float* d_weights, const float* d_depth, const float* d_depth_var,
                         const float* d_uncert_map, float* d_raw, int accumulate, void* stream) {
    if (f == nullptr || raw == nullptr || z_vals == nullptr || d_raw == nullptr) return fail(NARUTO_ERR_INVALID, "composite_bwd: NULL argument");
    if (S < 1 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "composite_bwd: samples per ray must be in [1, %d]", kMaxSamples);
    if (n_rays == 0) return NARUTO_OK;
    CompositeCot cot{d_rgb, d_disp, d_acc, d_weights, d_depth, d_depth_var, d_uncert_map};
    LossArgs la{};
    if (int rc = ray_lds_attr()) return rc;
    hipLaunchKernelGGL(k_composite_bwd<false>, dim3((n_rays + kRaysPerBlock - 1) / kRaysPerBlock), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), (hipStream_t)stream,
                       n_rays, S, f->desc.trunc, f->desc.sc_factor, f->desc.white_bkgd, raw, z_vals, cot, la, d_raw, accumulate, (uint32_t*)nullptr);
    return check_launch("composite_bwd");
}

size_t naruto_loss_workspace(uint32_t n_rays) { return loss_ws(nullptr, n_rays).total; }

int naruto_loss_sums(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals, const float* rgb, const float* depth,
                     const float* uncert_map, const float* target_rgb, const float* target_d, float depth_trunc, float rgb_missing, double* sums,
                     float* losses, void* workspace, void* stream) {
    if (f == nullptr || raw == nullptr || z_vals == nullptr || rgb == nullptr || depth == nullptr || uncert_map == nullptr || target_rgb == nullptr ||
        target_d == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "loss_sums: NULL argument");
    if (n_rays == 0) return fail(NARUTO_ERR_INVALID, "loss_sums: no rays");
    float* terms = loss_ws(workspace, n_rays).terms;
    hipLaunchKernelGGL(k_loss_terms, dim3((n_rays + kRaysPerBlock - 1) / kRaysPerBlock), dim3(64 * kRaysPerBlock), 0, (hipStream_t)stream, n_rays, S,
                       f->desc.trunc * f->desc.sc_factor, raw, z_vals, rgb, depth, uncert_map, target_rgb, target_d, depth_trunc, rgb_missing, terms);
    if (int rc = check_launch("loss_terms")) return rc;
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, n_rays, sums, S, losses);
    return check_launch("loss_reduce");
}

int naruto_loss_finalize(const double* sums, uint64_t n_rays_total, uint32_t S, float* losses, void* stream) {
    if (sums == nullptr || losses == nullptr || n_rays_total == 0 || S == 0) return fail(NARUTO_ERR_INVALID, "loss_finalize: bad argument");
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, n_rays_total, S, losses);
    return check_launch("loss_finalize");
}

int naruto_loss_bwd(const NarutoField* f, uint32_t n_rays, uint32_t S, const float* raw, const float* z_vals, const float* target_rgb,
                    const float* target_d, float depth_trunc, float rgb_missing, const double* sums, uint64_t n_rays_total, const float* loss_grad,
                    float* d_raw, uint32_t* ray_count, void* stream) {
    if (f == nullptr || raw == nullptr || z_vals == nullptr || target_rgb == nullptr || target_d == nullptr || sums == nullptr || loss_grad == nullptr ||
        d_raw == nullptr)
        return fail(NARUTO_ERR_INVALID, "loss_bwd: NULL argument");
    if (S < 1 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "loss_bwd: samples per ray must be in [1, %d]", kMaxSamples);
    if (n_rays == 0) return NARUTO_OK;
    CompositeCot cot{};
    LossArgs la{target_rgb, target_d, sums, loss_grad, n_rays_total, depth_trunc, rgb_missing, f->desc.trunc * f->desc.sc_factor};
    if (int rc = ray_lds_attr()) return rc;
    hipLaunchKernelGGL(k_composite_bwd<true>, dim3((n_rays + kRaysPerBlock - 1) / kRaysPerBlock), dim3(64 * kRaysPerBlock), ray_scratch_bytes(S), (hipStream_t)stream,
                       n_rays, S, f->desc.trunc, f->desc.sc_factor, f->desc.white_bkgd, raw, z_vals, cot, la, d_raw, 0, ray_count);
    return check_launch("loss_bwd");
}

int naruto_compact_active(uint32_t n_rays, uint32_t S, const uint32_t* ray_count, uint32_t* ray_offset, uint32_t* active_idx, uint32_t* n_active,
                          void* stream) {
    if (ray_count == nullptr || ray_offset == nullptr || active_idx == nullptr || n_active == nullptr)
        return fail(NARUTO_ERR_INVALID, "compact_active: NULL argument");
    if (n_rays == 0) return fail(NARUTO_ERR_INVALID, "compact_active: no rays");
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_rays, ray_count, ray_offset, n_active);
    if (int rc = check_launch("compact_scan")) return rc;
    hipLaunchKernelGGL(k_compact_write, dim3((n_rays + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, n_rays, S, ray_count, ray_offset, active_idx);
    return check_launch("compact_write");
}

int naruto_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, uint32_t step, const int32_t* step_dev, void* stream) {
    if (param == nullptr || grad == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr) return fail(NARUTO_ERR_INVALID, "adam_step: NULL argument");
    if (n == 0) return NARUTO_OK;
    if (step == 0 && step_dev == nullptr) return fail(NARUTO_ERR_INVALID, "adam_step: step is 1-based (or pass step_dev)");
    const float bc1 = step ? 1.0f - powf(beta1, (float)step) : 1.0f;
    const float bc2_sqrt = step ? sqrtf(1.0f - powf(beta2, (float)step)) : 1.0f;
    uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(k_adam, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                       weight_decay, bc1, bc2_sqrt, step_dev);
    return check_launch("adam_step");
}

size_t naruto_active_ray_workspace(uint32_t n_total, uint32_t K) { return select_ws(nullptr, n_total, K, kArsPadWords).total; }

int naruto_active_ray_select(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o, const float* rays_d, const float* target_s,
                             const float* target_d, const float* uncert_vol, const uint32_t* vol_dims, const float* bbox_min, float voxel_scale,
                             float* out_o, float* out_d, float* out_s, float* out_t, void* workspace, void* stream) {
    return naruto_active_ray_select_rows(n_total, base, K, n_tail, rays_o, rays_d, target_s, target_d, uncert_vol, vol_dims, bbox_min, voxel_scale, out_o, out_d,
                                         out_s, out_t, nullptr, workspace, stream);
}

int naruto_active_ray_select_rows(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o, const float* rays_d, const float* target_s,
                                  const float* target_d, const float* uncert_vol, const uint32_t* vol_dims, const float* bbox_min, float voxel_scale,
                                  float* out_o, float* out_d, float* out_s, float* out_t, uint32_t* src_rows, void* workspace, void* stream) {
    if (rays_o == nullptr || rays_d == nullptr || target_s == nullptr || target_d == nullptr || uncert_vol == nullptr || vol_dims == nullptr ||
        bbox_min == nullptr || out_o == nullptr || out_d == nullptr || out_s == nullptr || out_t == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "active_ray_select: NULL argument");
    if (n_tail == 0 || K == 0 || K > base || (uint64_t)base + n_tail >= n_total)
        return fail(NARUTO_ERR_INVALID, "active_ray_select: need 0 < K <= base, n_tail > 0, base + n_tail < n_total");
    const uint32_t n_cand = n_total - n_tail - base;
    if (n_cand <= K) return fail(NARUTO_ERR_INVALID, "active_ray_select: %u candidates for K = %u (numpy argpartition needs K < n)", n_cand, K);
    static const bool fused_on = env_int("NARUTO_DEBUG_ARS_FUSED", 1) != 0;
    if (fused_on && n_cand <= kArsFusedMax) {
        // lookup, selection and gather in one launch (k_ars_fused); NARUTO_DEBUG_ARS_FUSED=0: the three launches below (same result)
        ArsArgs a{};
        a.n_total = n_total; a.base = base; a.K = K; a.n_tail = n_tail; a.n_cand = n_cand;
        a.rays_o = rays_o; a.rays_d = rays_d; a.target_s = target_s; a.target_d = target_d; a.vol = uncert_vol;
        a.X = (int)vol_dims[0]; a.Y = (int)vol_dims[1]; a.Z = (int)vol_dims[2];
        a.bx = bbox_min[0]; a.by = bbox_min[1]; a.bz = bbox_min[2]; a.voxel_scale = voxel_scale;
        a.o_out = out_o; a.d_out = out_d; a.s_out = out_s; a.t_out = out_t; a.src_out = src_rows;
        const uint32_t n_copy = base + n_tail - K;
        hipLaunchKernelGGL(k_ars_fused<false>, dim3(1u + (n_copy + kArsFusedThreads - 1u) / kArsFusedThreads), dim3(kArsFusedThreads), 0, (hipStream_t)stream, a, AssembleArgs{});
        return check_launch("ars_fused");
    }
    const SelectWs w = select_ws(workspace, n_cand, K, kArsPadWords);
    hipLaunchKernelGGL(k_ars_lookup, dim3((n_cand + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n_cand, base, rays_o, rays_d, target_d, uncert_vol,
                       (int)vol_dims[0], (int)vol_dims[1], (int)vol_dims[2], bbox_min[0], bbox_min[1], bbox_min[2], voxel_scale, w.keys);
    if (int rc = check_launch("ars_lookup")) return rc;
    if (n_cand <= 1024u * kArsPer) hipLaunchKernelGGL(k_ars_select_small, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_cand, K, w.keys, w.sel);
    else hipLaunchKernelGGL(k_ars_select, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_cand, K, w.keys, w.sel);
    if (int rc = check_launch("ars_select")) return rc;
    const uint32_t n_out = base + n_tail;
    hipLaunchKernelGGL(k_ars_gather, dim3((n_out + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n_out, K, base, n_total, n_tail, w.sel, rays_o, rays_d,
                       target_s, target_d, out_o, out_d, out_s, out_t, src_rows);
    return check_launch("ars_gather");
}

int naruto_active_ray_select_keyed(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o, const float* rays_d, const float* target_s,
                                   const float* target_d, const uint32_t* keys, float* out_o, float* out_d, float* out_s, float* out_t, void* stream) {
    return naruto_active_ray_select_keyed_rows(n_total, base, K, n_tail, rays_o, rays_d, target_s, target_d, keys, out_o, out_d, out_s, out_t, nullptr, stream);
}

int naruto_active_ray_select_keyed_rows(uint32_t n_total, uint32_t base, uint32_t K, uint32_t n_tail, const float* rays_o, const float* rays_d,
                                        const float* target_s, const float* target_d, const uint32_t* keys, float* out_o, float* out_d, float* out_s,
                                        float* out_t, uint32_t* src_rows, void* stream) {
    if (rays_o == nullptr || rays_d == nullptr || target_s == nullptr || target_d == nullptr || keys == nullptr || out_o == nullptr || out_d == nullptr ||
        out_s == nullptr || out_t == nullptr)
        return fail(NARUTO_ERR_INVALID, "active_ray_select_keyed: NULL argument");
    if (n_tail == 0 || K == 0 || K > base || (uint64_t)base + n_tail >= n_total)
        return fail(NARUTO_ERR_INVALID, "active_ray_select_keyed: need 0 < K <= base, n_tail > 0, base + n_tail < n_total");
    const uint32_t n_cand = n_total - n_tail - base;
    if (n_cand <= K || n_cand > kArsFusedMax)
        return fail(NARUTO_ERR_INVALID, "active_ray_select_keyed: %u candidates for K = %u (need K < candidates <= %u)", n_cand, K, kArsFusedMax);
    ArsArgs a{};
    a.n_total = n_total; a.base = base; a.K = K; a.n_tail = n_tail; a.n_cand = n_cand;
    a.rays_o = rays_o; a.rays_d = rays_d; a.target_s = target_s; a.target_d = target_d; a.keys = keys;
    a.o_out = out_o; a.d_out = out_d; a.s_out = out_s; a.t_out = out_t; a.src_out = src_rows;
    const uint32_t n_copy = base + n_tail - K;
    hipLaunchKernelGGL(k_ars_fused<false>, dim3(1u + (n_copy + kArsFusedThreads - 1u) / kArsFusedThreads), dim3(kArsFusedThreads), 0, (hipStream_t)stream, a, AssembleArgs{});
    return check_launch("ars_fused (keyed)");
}

int naruto_rays_to_world(uint32_t n, const float* d_cam, const int64_t* pose_id, const float* poses, float* rays_o, float* rays_d, void* stream) {
    if (d_cam == nullptr || pose_id == nullptr || poses == nullptr || rays_o == nullptr || rays_d == nullptr)
        return fail(NARUTO_ERR_INVALID, "rays_to_world: NULL argument");
    if (n == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_rays_to_world, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, d_cam, pose_id, poses, rays_o, rays_d);
    return check_launch("rays_to_world");
}

size_t naruto_goal_targets_workspace(uint32_t n_voxels, uint32_t top_k) { return select_ws(nullptr, n_voxels, top_k, kGoalPadWords).total; }

int naruto_goal_targets(const uint32_t* dims, const float* uncert_vol, uint32_t top_k, uint32_t top_k_subset, int32_t* targets, void* workspace, void* stream) {
    if (dims == nullptr || uncert_vol == nullptr || targets == nullptr || workspace == nullptr) return fail(NARUTO_ERR_INVALID, "goal_targets: NULL argument");
    const uint64_t n64 = (uint64_t)dims[0] * dims[1] * dims[2];
    if (n64 == 0 || n64 > 0x7FFFFFFFull) return fail(NARUTO_ERR_INVALID, "goal_targets: bad volume dimensions");
    const uint32_t n = (uint32_t)n64;
    if (top_k == 0 || top_k > n || top_k_subset == 0 || top_k_subset > top_k) return fail(NARUTO_ERR_INVALID, "goal_targets: need 1 <= subset <= top_k <= voxels");
    const SelectWs w = select_ws(workspace, n, top_k, kGoalPadWords);
    const VolDims d{(int)dims[0], (int)dims[1], (int)dims[2]};
    hipLaunchKernelGGL(k_topk_keys, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, uncert_vol, w.keys);
    if (int rc = check_launch("topk_keys")) return rc;
    hipLaunchKernelGGL(k_ars_select, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, top_k, w.keys, w.sel);
    if (int rc = check_launch("topk_select")) return rc;
    hipLaunchKernelGGL(k_topk_thin, dim3((top_k_subset + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, w.sel, top_k, top_k_subset, d, targets);
    return check_launch("topk_thin");
}

int naruto_goal_aggregate(const uint32_t* dims, const float* uncert_vol, const float* sdf_vol, uint32_t n_goals, const int32_t* goal_idx, uint32_t n_targets,
                          const int32_t* targets, float min_dist, float max_dist, float safe_sdf, float* collections, float* aggregated, void* stream) {
    if (dims == nullptr || uncert_vol == nullptr || sdf_vol == nullptr || goal_idx == nullptr || targets == nullptr || collections == nullptr ||
        aggregated == nullptr)
        return fail(NARUTO_ERR_INVALID, "goal_aggregate: NULL argument");
    if ((uint64_t)dims[0] * dims[1] * dims[2] == 0 || (uint64_t)dims[0] * dims[1] * dims[2] > 0x7FFFFFFFull)
        return fail(NARUTO_ERR_INVALID, "goal_aggregate: bad volume dimensions");
    if (n_goals == 0 || n_targets == 0) return NARUTO_OK;
    const VolDims d{(int)dims[0], (int)dims[1], (int)dims[2]};
    hipLaunchKernelGGL(k_goal_aggregate, dim3((n_goals + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d, uncert_vol, sdf_vol, n_goals, goal_idx, n_targets,
                       targets, min_dist, max_dist, safe_sdf, collections, aggregated);
    return check_launch("goal_aggregate");
}

int naruto_goal_search(uint32_t n_goals, uint32_t n_targets, const float* aggregated, const float* collections, const int32_t* targets, const int32_t* goal_idx,
                       uint32_t obs_per_goal, const double* bbox_min, double voxel_size, void* out, void* stream) {
    if (aggregated == nullptr || collections == nullptr || targets == nullptr || goal_idx == nullptr || bbox_min == nullptr || out == nullptr)
        return fail(NARUTO_ERR_INVALID, "goal_search: NULL argument");
    if (n_goals == 0 || n_targets == 0 || obs_per_goal == 0) return fail(NARUTO_ERR_INVALID, "goal_search: need at least one goal, one target and obs_per_goal >= 1");
    if (n_goals == 0xFFFFFFFFu) return fail(NARUTO_ERR_INVALID, "goal_search: too many goals");
    if (n_targets > kGoalSearchMaxTargets) return fail(NARUTO_ERR_INVALID, "goal_search: at most %u targets (got %u)", kGoalSearchMaxTargets, n_targets);
    if (((uintptr_t)out & 7u) != 0u) return fail(NARUTO_ERR_INVALID, "goal_search: out must be 8-byte aligned");
    const uint32_t m = obs_per_goal < n_targets ? obs_per_goal : n_targets;
    const GoalSearchFrame fr{bbox_min[0], bbox_min[1], bbox_min[2], voxel_size};
    hipLaunchKernelGGL(k_goal_search, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_goals, n_targets, aggregated, collections, targets, goal_idx, m, fr, (int32_t*)out);
    return check_launch("goal_search");
}

// ---- the planner's local RRT (naruto_rrt.hip) --------------------------------------------------------------------------
namespace {
int rrt_dims(const uint32_t* dims, const char* who, RrtVol* vol, const float* sdf) {
    if (dims == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL dims", who);
    const uint64_t n64 = (uint64_t)dims[0] * dims[1] * dims[2];
    if (n64 == 0 || n64 > (1ull << 28) || dims[0] > (1u << 28) || dims[1] > (1u << 28) || dims[2] > (1u << 28))
        return fail(NARUTO_ERR_INVALID, "%s: volume must have 1 .. 2^28 voxels", who);
    *vol = RrtVol{sdf, (int)dims[0], (int)dims[1], (int)dims[2]};
    return NARUTO_OK;
}
int rrt_plan(const NarutoRrtPlan* p, const char* who, RrtVol* vol) {
    if (p == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL plan", who);
    if (int rc = rrt_dims(p->dims, who, vol, p->sdf_vol)) return rc;
    if (p->sdf_vol == nullptr || p->workspace == nullptr || p->nodes_xyz == nullptr || p->nodes_xyz32 == nullptr || p->parent == nullptr || p->next == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL buffer in the plan", who);
    if (p->capacity == 0 || p->capacity > 0x7FFFFFFFu / 3u) return fail(NARUTO_ERR_INVALID, "%s: capacity must be 1 .. %u nodes", who, 0x7FFFFFFFu / 3u);
    if (!(p->step_size > 0.0) || !(p->step_amplifier > 0.0) || !(p->step_size < 1.0e9) || !(p->step_amplifier < 1.0e9) || !(p->collision_thre == p->collision_thre))
        return fail(NARUTO_ERR_INVALID, "%s: step_size and step_amplifier must be positive and finite, collision_thre a number", who);
    for (int a = 0; a < 3; ++a)
        if (!(p->range[a][0] <= p->range[a][1]) || !(p->full_range[a][0] <= p->full_range[a][1]))
            return fail(NARUTO_ERR_INVALID, "%s: a sampling range has lo > hi", who);
    return NARUTO_OK;
}
// workspace of the RRT over a volume: | state int32[16] (to kRrtGoalOffset) | goal fp64[4] (to kRrtHeadOffset) | head of every cell's node list int32[X*Y*Z] |
struct RrtWs { int32_t* state; double* goal; int32_t* head; size_t total; };
RrtWs rrt_ws(void* base, const RrtVol& vol) {
    static_assert(kRrtGoalOffset >= (int)(kRrtStateInts * sizeof(int32_t)) && kRrtHeadOffset >= kRrtGoalOffset + (int)(4u * sizeof(double)), "sections overlap");
    Carve c(base);
    return {c.take<int32_t>(kRrtGoalOffset, 1u), c.take<double>(kRrtHeadOffset - kRrtGoalOffset, 1u), c.take<int32_t>((size_t)vol.X * vol.Y * vol.Z * sizeof(int32_t), 1u), c.size()};
}
}  // namespace

size_t naruto_rrt_workspace(const uint32_t* dims) {
    RrtVol vol;
    return rrt_dims(dims, "rrt_workspace", &vol, nullptr) ? 0 : rrt_ws(nullptr, vol).total;
}

int naruto_rrt_start(const NarutoRrtPlan* plan, const double* start, const double* goal, void* stream) {
    RrtVol vol;
    if (int rc = rrt_plan(plan, "rrt_start", &vol)) return rc;
    const RrtWs w = rrt_ws(plan->workspace, vol);
    if (start == nullptr || goal == nullptr) return fail(NARUTO_ERR_INVALID, "rrt_start: NULL start or goal");
    bool inside = true;
    for (int a = 0; a < 3; ++a) {
        if (!(start[a] == start[a]) || !(goal[a] == goal[a])) return fail(NARUTO_ERR_INVALID, "rrt_start: start or goal is not a number");
        inside = inside && start[a] >= 0.0 && start[a] <= (double)(plan->dims[a] - 1u);
    }
    // the shell search's bound needs every node inside the grid; the nodes lie on segments between the start and in-grid points
    const uint32_t n = (uint32_t)(vol.X * vol.Y * vol.Z);
    hipLaunchKernelGGL(k_rrt_start, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, vol, D3{start[0], start[1], start[2]}, D3{goal[0], goal[1], goal[2]},
                       inside ? 1 : 0, plan->nodes_xyz, plan->nodes_xyz32, plan->parent, plan->next, w.head, w.state, w.goal);
    return check_launch("rrt_start");
}

int naruto_rrt_grow(const NarutoRrtPlan* plan, int mode, const double* rows, uint32_t n_rows, uint32_t max_iter, int restart, void* stream) {
    RrtVol vol;
    if (int rc = rrt_plan(plan, "rrt_grow", &vol)) return rc;
    const RrtWs w = rrt_ws(plan->workspace, vol);
    if (mode != NARUTO_RRT_MODE_RUN && mode != NARUTO_RRT_MODE_FULL) return fail(NARUTO_ERR_INVALID, "rrt_grow: unknown mode %d", mode);
    if (n_rows != 0 && rows == nullptr) return fail(NARUTO_ERR_INVALID, "rrt_grow: NULL rows");
    if (n_rows > 0x7FFFFFFFu || max_iter > 0x7FFFFFFFu) return fail(NARUTO_ERR_INVALID, "rrt_grow: n_rows and max_iter must fit int32");
    RrtArgs a;
    a.vol = vol;
    a.step = plan->step_size; a.amp = plan->step_amplifier; a.thre = plan->collision_thre;
    a.direct = plan->enable_direct_line != 0; a.mode = mode; a.restart = restart != 0;
    a.xyz64 = plan->nodes_xyz; a.xyz32 = plan->nodes_xyz32; a.parent = plan->parent; a.next = plan->next;
    a.head = w.head; a.state = w.state; a.goal = w.goal;
    a.rows = rows; a.n_rows = (int)n_rows; a.max_iter = (int)max_iter; a.cap = (int)plan->capacity;
    a.cell_threshold = (int)(plan->cell_threshold ? std::min(plan->cell_threshold, 0x7FFFFFFFu) : NARUTO_RRT_CELL_THRESHOLD);
    hipLaunchKernelGGL(k_rrt_grow, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return check_launch("rrt_grow");
}

int naruto_segments_free(const uint32_t* dims, const float* sdf_vol, uint32_t n, const double* pa, const double* pb, double step_size, double collision_thre,
                         int32_t* num_collision_free, uint8_t* complete_free, void* stream) {
    RrtVol vol;
    if (int rc = rrt_dims(dims, "segments_free", &vol, sdf_vol)) return rc;
    if (sdf_vol == nullptr || pa == nullptr || pb == nullptr || num_collision_free == nullptr || complete_free == nullptr)
        return fail(NARUTO_ERR_INVALID, "segments_free: NULL argument");
    if (!(step_size > 0.0) || !(step_size < 1.0e9) || !(collision_thre == collision_thre))
        return fail(NARUTO_ERR_INVALID, "segments_free: step_size must be positive and finite, collision_thre a number");
    if (n > 0x40000000u) return fail(NARUTO_ERR_INVALID, "segments_free: at most 2^30 segments");
    if (n == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_segments_free, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, vol, n, pa, pb, step_size, collision_thre, num_collision_free,
                       complete_free);
    return check_launch("segments_free");
}

int naruto_rrt_path(const NarutoRrtPlan* plan, int32_t* path, void* stream) {
    RrtVol vol;
    if (int rc = rrt_plan(plan, "rrt_path", &vol)) return rc;
    const RrtWs w = rrt_ws(plan->workspace, vol);
    if (path == nullptr) return fail(NARUTO_ERR_INVALID, "rrt_path: NULL path");
    hipLaunchKernelGGL(k_rrt_path, dim3(1), dim3(64), 0, (hipStream_t)stream, plan->parent, w.state, (int)plan->capacity, path);
    return check_launch("rrt_path");
}

int naruto_reachable_mask(const NarutoRrtPlan* plan, float* mask, void* stream) {
    RrtVol vol;
    if (int rc = rrt_plan(plan, "reachable_mask", &vol)) return rc;
    const RrtWs w = rrt_ws(plan->workspace, vol);
    if (mask == nullptr) return fail(NARUTO_ERR_INVALID, "reachable_mask: NULL mask");
    const uint32_t n = (uint32_t)(vol.X * vol.Y * vol.Z);
    hipLaunchKernelGGL(k_reachable_mask, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, vol, (float)plan->step_size, plan->nodes_xyz32, w.head,
                       plan->next, w.state, mask);
    return check_launch("reachable_mask");
}

// ---- N4: dense volume -> mesh (naruto_mesh.hip) ----------------------------------------------------------------------
namespace {
// workspace of the mesh extraction over n voxels: | cases [n] | flags [n] | prefix [n] | one total per block of kMcBlockItems voxels |
struct McWs { uint8_t* cases; uint8_t* flags; uint2* prefix; unsigned long long* block_total; uint32_t n, n_blocks; size_t total; };
int mc_dims(const uint32_t* dims, const char* who, McDims* d, uint32_t* n) {
    if (dims == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL dims", who);
    const uint64_t n64 = (uint64_t)dims[0] * dims[1] * dims[2];
    if (n64 == 0 || n64 > (1ull << 30) || dims[0] > (1u << 30) || dims[1] > (1u << 30) || dims[2] > (1u << 30))
        return fail(NARUTO_ERR_INVALID, "%s: volume must have 1 .. 2^30 voxels", who);
    *d = McDims{dims[0], dims[1], dims[2]};
    *n = (uint32_t)n64;
    return NARUTO_OK;
}
McWs mc_ws(void* workspace, uint32_t n) {
    const uint32_t n_blocks = (n + kMcBlockItems - 1u) / kMcBlockItems;
    Carve c(workspace);
    return {c.take<uint8_t>(n), c.take<uint8_t>(n), c.take<uint2>((size_t)n * sizeof(uint2)), c.take<unsigned long long>((size_t)n_blocks * sizeof(unsigned long long)), n, n_blocks, c.size()};
}
}  // namespace

int naruto_lattice_points(const uint32_t* dims, const float* tx, const float* ty, const float* tz, float* x, void* stream) {
    McDims d; uint32_t n;
    if (int rc = mc_dims(dims, "lattice_points", &d, &n)) return rc;
    if (tx == nullptr || ty == nullptr || tz == nullptr || x == nullptr) return fail(NARUTO_ERR_INVALID, "lattice_points: NULL argument");
    hipLaunchKernelGGL(k_lattice_points, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d, tx, ty, tz, x);
    return check_launch("lattice_points");
}

size_t naruto_mesh_workspace(const uint32_t* dims) {
    McDims d; uint32_t n;
    return mc_dims(dims, "mesh_workspace", &d, &n) ? 0 : mc_ws(nullptr, n).total;
}

int naruto_mesh_count(const uint32_t* dims, const float* sdf_vol, double isolevel, double truncation, void* workspace, uint64_t* counts, void* stream) {
    McDims d; uint32_t n;
    if (int rc = mc_dims(dims, "mesh_count", &d, &n)) return rc;
    if (sdf_vol == nullptr || workspace == nullptr || counts == nullptr) return fail(NARUTO_ERR_INVALID, "mesh_count: NULL argument");
    const McWs w = mc_ws(workspace, n);
    hipLaunchKernelGGL(k_mc_cases, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d, sdf_vol, isolevel, truncation, w.cases);
    if (int rc = check_launch("mc_cases")) return rc;
    hipLaunchKernelGGL(k_mc_count, dim3(w.n_blocks), dim3(kMcThreads), 0, (hipStream_t)stream, d, sdf_vol, w.cases, isolevel, w.flags, w.prefix, w.block_total);
    if (int rc = check_launch("mc_count")) return rc;
    hipLaunchKernelGGL(k_mc_scan_blocks, dim3(1), dim3(1024), 0, (hipStream_t)stream, w.n_blocks, w.block_total, reinterpret_cast<unsigned long long*>(counts));
    return check_launch("mc_scan_blocks");
}

int naruto_mesh_emit(const uint32_t* dims, const float* sdf_vol, double isolevel, const void* workspace, uint64_t cap_vertices, uint64_t cap_triangles,
                     double* vertices, int32_t* triangles, void* stream) {
    McDims d; uint32_t n;
    if (int rc = mc_dims(dims, "mesh_emit", &d, &n)) return rc;
    if (sdf_vol == nullptr || workspace == nullptr) return fail(NARUTO_ERR_INVALID, "mesh_emit: NULL argument");
    if ((cap_vertices != 0 && vertices == nullptr) || (cap_triangles != 0 && triangles == nullptr))
        return fail(NARUTO_ERR_INVALID, "mesh_emit: NULL output with a non-zero capacity");
    if (cap_vertices > 0x7FFFFFFFull) return fail(NARUTO_ERR_INVALID, "mesh_emit: triangles index vertices with int32");
    if (cap_vertices == 0 && cap_triangles == 0) return NARUTO_OK;
    const McWs w = mc_ws(const_cast<void*>(workspace), n);
    hipLaunchKernelGGL(k_mc_emit, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d, sdf_vol, w.cases, w.flags, w.prefix, w.block_total, isolevel,
                       cap_vertices, cap_triangles, vertices, triangles);
    return check_launch("mc_emit");
}

// ---- reconstruction metrics (naruto_recon.hip) ------------------------------------------------------------------------
namespace {
constexpr uint64_t kReconMaxCount = 0x7FFFFFFFull;
constexpr uint64_t kNnGridDefaultCap = 1ull << 21;          // cells: 8 MB of starts; above it the cell edge grows
uint64_t nn_grid_cells(const NarutoNnGrid* g) { return (uint64_t)g->dims[0] * g->dims[1] * g->dims[2]; }
int nn_grid_check(const NarutoNnGrid* g, const char* who) {
    if (g == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL grid", who);
    if (g->n_points == 0 || g->n_points > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "%s: grid over 1 .. 2^31-1 points", who);
    const uint64_t cells = nn_grid_cells(g);
    if (cells == 0 || cells > (1ull << 26) || g->dims[0] > (1u << 26) || g->dims[1] > (1u << 26) || g->dims[2] > (1u << 26))
        return fail(NARUTO_ERR_INVALID, "%s: grid must have 1 .. 2^26 cells", who);
    if (!(g->cell > 0.0) || !std::isfinite(g->cell)) return fail(NARUTO_ERR_INVALID, "%s: cell edge must be finite and positive", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(g->lo[a])) return fail(NARUTO_ERR_INVALID, "%s: non-finite box", who);
    return NARUTO_OK;
}
NnGrid nn_grid_args(const NarutoNnGrid* g) {
    NnGrid a{};
    a.nx = g->dims[0]; a.ny = g->dims[1]; a.nz = g->dims[2]; a.n = (uint32_t)g->n_points;
    for (int k = 0; k < 3; ++k) a.lo[k] = g->lo[k];
    a.h = g->cell;
    a.inv_h = 1.0 / g->cell;
    const double ext = g->cell * (double)std::max(g->dims[0], std::max(g->dims[1], g->dims[2]));
    a.slack = ext * 0x1p-40;
    a.start = reinterpret_cast<const uint32_t*>(g->cell_start);
    a.pts = reinterpret_cast<const float4*>(g->points);
    return a;
}
// workspace of the grid build: | each point's cell [n_points] | points per cell [cells] | one total per block of kGridScanItems cells |
struct NnGridWs { uint32_t* cells; uint32_t* count; uint32_t* block_total; uint32_t n_blocks; size_t total; };
NnGridWs nn_grid_ws(const NarutoNnGrid* g, void* workspace) {
    const uint64_t cells = nn_grid_cells(g);
    const uint32_t n_blocks = (uint32_t)((cells + kGridScanItems - 1u) / kGridScanItems);
    Carve c(workspace);
    return {c.take<uint32_t>((size_t)g->n_points * 4u), c.take<uint32_t>((size_t)cells * 4u), c.take<uint32_t>((size_t)n_blocks * 4u), n_blocks, c.size()};
}
// workspace of the distance reduce over n values: | one partial sum | and one count | per workgroup of kReconThreads * kDistPer values
struct DistWs { double* part_sum; unsigned long long* part_cnt; uint32_t parts; size_t total; };
DistWs dist_ws(uint64_t n, void* workspace) {
    const uint32_t parts = (uint32_t)((n + kReconThreads * kDistPer - 1u) / (kReconThreads * kDistPer));
    Carve c(workspace);
    return {c.take<double>((size_t)parts * 8u), c.take<unsigned long long>((size_t)parts * 8u), parts, c.size()};
}
int mesh_args_check(uint64_t n_faces, uint64_t n_vertices, const void* vertices, const int32_t* faces, const char* who) {
    if (n_faces == 0) return fail(NARUTO_ERR_INVALID, "%s: a mesh without faces has no surface to sample", who);
    if (n_vertices == 0) return fail(NARUTO_ERR_INVALID, "%s: zero vertices", who);
    if (n_faces > kReconMaxCount || n_vertices > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "%s: counts beyond int32", who);
    if (vertices == nullptr || faces == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL argument", who);
    return NARUTO_OK;
}
}  // namespace

int naruto_surface_areas(uint64_t n_faces, uint64_t n_vertices, const void* vertices, int vertices_f64, const int32_t* faces, double* areas, void* stream) {
    if (int rc = mesh_args_check(n_faces, n_vertices, vertices, faces, "surface_areas")) return rc;
    if (areas == nullptr) return fail(NARUTO_ERR_INVALID, "surface_areas: NULL output");
    const dim3 grid((uint32_t)((n_faces + kReconThreads - 1u) / kReconThreads)), block(kReconThreads);
    if (vertices_f64) hipLaunchKernelGGL(k_face_areas<true>, grid, block, 0, (hipStream_t)stream, (uint32_t)n_faces, (uint32_t)n_vertices, vertices, faces, areas);
    else hipLaunchKernelGGL(k_face_areas<false>, grid, block, 0, (hipStream_t)stream, (uint32_t)n_faces, (uint32_t)n_vertices, vertices, faces, areas);
    return check_launch("face_areas");
}

int naruto_surface_sample(uint64_t n_faces, uint64_t n_vertices, const void* vertices, int vertices_f64, const int32_t* faces, const double* cum_area,
                          uint64_t count, uint64_t seed, float* points, int32_t* face_index, void* stream) {
    if (int rc = mesh_args_check(n_faces, n_vertices, vertices, faces, "surface_sample")) return rc;
    if (count > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "surface_sample: counts beyond int32");
    if (count == 0) return NARUTO_OK;
    if (cum_area == nullptr || points == nullptr || face_index == nullptr) return fail(NARUTO_ERR_INVALID, "surface_sample: NULL argument");
    const dim3 grid((uint32_t)((count + kReconThreads - 1u) / kReconThreads)), block(kReconThreads);
    if (vertices_f64) hipLaunchKernelGGL(k_surface_sample<true>, grid, block, 0, (hipStream_t)stream, (uint32_t)n_faces, (uint32_t)n_vertices, vertices, faces, cum_area, (uint32_t)count, seed, points, face_index);
    else hipLaunchKernelGGL(k_surface_sample<false>, grid, block, 0, (hipStream_t)stream, (uint32_t)n_faces, (uint32_t)n_vertices, vertices, faces, cum_area, (uint32_t)count, seed, points, face_index);
    return check_launch("surface_sample");
}

int naruto_nn_grid_plan(uint64_t n_points, const double* lo, const double* hi, double cell, uint64_t max_cells, NarutoNnGrid* grid) {
    if (grid == nullptr || lo == nullptr || hi == nullptr) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: NULL argument");
    if (n_points == 0) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: zero points");
    if (n_points > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: counts beyond int32");
    if (!std::isfinite(cell) || cell < 0.0) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: cell edge must be finite and not negative (0 = derive it from the cloud)");
    if (max_cells == 0) max_cells = kNnGridDefaultCap;
    if (max_cells > (1ull << 26)) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: at most 2^26 cells");
    double ext[3], top = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: the box must be finite with lo <= hi");
        ext[a] = hi[a] - lo[a];
        if (!std::isfinite(ext[a])) return fail(NARUTO_ERR_INVALID, "nn_grid_plan: the box must be finite with lo <= hi");
        top = std::max(top, ext[a]);
    }
    double h = cell;
    if (h == 0.0) {
        // the clouds of this path are surface samples: n points spread over an area of the order of the box's own surface, so a cell of edge
        // 2 * sqrt(box surface / n) holds a handful of them; a box without surface (a line, a point) falls back to extent / cbrt(n), then to 1
        const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
        if (area > 0.0) h = 2.0 * std::sqrt(area / (double)n_points);
        else if (top > 0.0) h = top / std::cbrt((double)n_points);
        else h = 1.0;
    }
    if (!(h > 0.0) || !std::isfinite(h)) h = top > 0.0 ? top : 1.0;
    double dims[3];
    for (;;) {
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) { dims[a] = std::floor(ext[a] / h) + 1.0; cells *= dims[a]; }
        if (cells <= (double)max_cells) break;
        h *= 1.25;                                          // the cap enlarges the cell
    }
    grid->n_points = n_points;
    for (int a = 0; a < 3; ++a) { grid->dims[a] = (uint32_t)dims[a]; grid->lo[a] = lo[a]; }
    grid->cell = h;
    return NARUTO_OK;
}

size_t naruto_nn_grid_workspace(const NarutoNnGrid* grid) {
    return nn_grid_check(grid, "nn_grid_workspace") ? 0 : nn_grid_ws(grid, nullptr).total;
}

int naruto_nn_grid_build(const NarutoNnGrid* grid, const float* points, void* workspace, void* stream) {
    if (int rc = nn_grid_check(grid, "nn_grid_build")) return rc;
    if (points == nullptr || workspace == nullptr || grid->cell_start == nullptr || grid->points == nullptr) return fail(NARUTO_ERR_INVALID, "nn_grid_build: NULL argument");
    const NnGrid g = nn_grid_args(grid);
    const NnGridWs w = nn_grid_ws(grid, workspace);
    const uint32_t cells = (uint32_t)nn_grid_cells(grid);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* start = reinterpret_cast<uint32_t*>(grid->cell_start);
    if (hipMemsetAsync(w.count, 0, (size_t)cells * 4u, st) != hipSuccess) return check_launch("nn_grid_build: memset");
    const dim3 block(kReconThreads), per_point((g.n + kReconThreads - 1u) / kReconThreads);
    hipLaunchKernelGGL(k_grid_count, per_point, block, 0, st, g, points, w.cells, w.count);
    if (int rc = check_launch("grid_count")) return rc;
    hipLaunchKernelGGL(k_grid_scan_local, dim3(w.n_blocks), block, 0, st, cells, w.count, start, w.block_total);
    if (int rc = check_launch("grid_scan_local")) return rc;
    hipLaunchKernelGGL(k_grid_scan_totals, dim3(1), dim3(1024), 0, st, w.n_blocks, w.block_total);
    if (int rc = check_launch("grid_scan_totals")) return rc;
    hipLaunchKernelGGL(k_grid_scan_add, dim3(cells / kReconThreads + 1u), block, 0, st, cells, g.n, w.block_total, start, w.count);
    if (int rc = check_launch("grid_scan_add")) return rc;
    hipLaunchKernelGGL(k_grid_fill, per_point, block, 0, st, g, points, w.cells, start, w.count, reinterpret_cast<float4*>(grid->points));
    return check_launch("grid_fill");
}

int naruto_nn_grid_query(const NarutoNnGrid* grid, uint64_t n_queries, const float* queries, const void* queries_sorted, uint32_t ring_budget,
                         double* dist, int32_t* index, uint32_t* fallback, void* stream) {
    if (int rc = nn_grid_check(grid, "nn_grid_query")) return rc;
    if (n_queries > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "nn_grid_query: counts beyond int32");
    if (n_queries == 0) return NARUTO_OK;
    if ((queries == nullptr && queries_sorted == nullptr) || dist == nullptr || index == nullptr || fallback == nullptr || grid->cell_start == nullptr || grid->points == nullptr)
        return fail(NARUTO_ERR_INVALID, "nn_grid_query: NULL argument");
    const NnGrid g = nn_grid_args(grid);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nq = (uint32_t)n_queries;
    const float4* q4 = reinterpret_cast<const float4*>(queries_sorted);
    if (hipMemsetAsync(fallback, 0, 4u, st) != hipSuccess) return check_launch("nn_grid_query: memset");
    hipLaunchKernelGGL(k_nn_grid, dim3((nq + kReconThreads - 1u) / kReconThreads), dim3(kReconThreads), 0, st, g, nq, queries, q4, ring_budget, dist, index,
                       fallback + 1, fallback);
    if (int rc = check_launch("nn_grid")) return rc;
    // the queries whose rings did not close: their number is on the device, so the launch covers the worst case and empty workgroups leave at once
    const uint32_t per = (uint32_t)(kReconThreads * kScanQ);
    hipLaunchKernelGGL(k_nn_scan, dim3((nq + per - 1u) / per), dim3(kReconThreads), 0, st, g.n, (const float*)nullptr, g.pts, nq, queries, q4, fallback + 1, fallback, dist, index);
    return check_launch("nn_scan (fallback)");
}

int naruto_nn_scan(uint64_t n_targets, const float* targets, uint64_t n_queries, const float* queries, double* dist, int32_t* index, void* stream) {
    if (n_targets == 0) return fail(NARUTO_ERR_INVALID, "nn_scan: zero points");
    if (n_targets > kReconMaxCount || n_queries > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "nn_scan: counts beyond int32");
    if (n_queries == 0) return NARUTO_OK;
    if (targets == nullptr || queries == nullptr || dist == nullptr || index == nullptr) return fail(NARUTO_ERR_INVALID, "nn_scan: NULL argument");
    const uint32_t nq = (uint32_t)n_queries, per = (uint32_t)(kReconThreads * kScanQ);
    hipLaunchKernelGGL(k_nn_scan, dim3((nq + per - 1u) / per), dim3(kReconThreads), 0, (hipStream_t)stream, (uint32_t)n_targets, targets, (const float4*)nullptr, nq, queries,
                       (const float4*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, dist, index);
    return check_launch("nn_scan");
}

size_t naruto_dist_reduce_workspace(uint64_t n) {
    return (n == 0 || n > kReconMaxCount) ? 0 : dist_ws(n, nullptr).total;
}

int naruto_dist_reduce(uint64_t n, const double* dist, double threshold, void* workspace, double* out, void* stream) {
    if (n == 0) return fail(NARUTO_ERR_INVALID, "dist_reduce: zero points");
    if (n > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "dist_reduce: counts beyond int32");
    if (std::isnan(threshold)) return fail(NARUTO_ERR_INVALID, "dist_reduce: the threshold is not a number");
    if (dist == nullptr || workspace == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "dist_reduce: NULL argument");
    const DistWs w = dist_ws(n, workspace);
    hipLaunchKernelGGL(k_dist_partial, dim3(w.parts), dim3(kReconThreads), 0, (hipStream_t)stream, (uint32_t)n, dist, threshold, w.part_sum, w.part_cnt);
    if (int rc = check_launch("dist_partial")) return rc;
    hipLaunchKernelGGL(k_dist_finish, dim3(1), dim3(kReconThreads), 0, (hipStream_t)stream, (uint32_t)n, w.parts, w.part_sum, w.part_cnt, out);
    return check_launch("dist_finish");
}

// ---- rigid alignment (naruto_icp.hip) -----------------------------------------------------------------------------------
namespace {
struct IcpWs { double* part; uint32_t parts; size_t total; };
IcpWs icp_ws(uint64_t n, void* workspace) {
    const uint32_t parts = (uint32_t)((n + kIcpThreads * kIcpPer - 1u) / (kIcpThreads * kIcpPer));
    Carve c(workspace);
    return {c.take<double>((size_t)parts * kIcpSums * sizeof(double)), parts, c.size()};
}
int icp_origin(const double* origin, const char* who, IcpOrigin* out) {
    if (origin == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL origin", who);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return fail(NARUTO_ERR_INVALID, "%s: non-finite origin", who);
    *out = IcpOrigin{origin[0], origin[1], origin[2]};
    return NARUTO_OK;
}
}  // namespace

int naruto_icp_transform(uint64_t n, const void* points, int points_f64, const double* T, void* out, void* stream) {
    if (n == 0) return fail(NARUTO_ERR_INVALID, "icp_transform: zero points");
    if (n > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "icp_transform: counts beyond int32");
    if (points == nullptr || T == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "icp_transform: NULL argument");
    const dim3 grid((uint32_t)((n + kIcpThreads - 1u) / kIcpThreads)), block(kIcpThreads);
    if (points_f64) hipLaunchKernelGGL(k_icp_transform<true>, grid, block, 0, (hipStream_t)stream, (uint32_t)n, points, T, out);
    else hipLaunchKernelGGL(k_icp_transform<false>, grid, block, 0, (hipStream_t)stream, (uint32_t)n, points, T, out);
    return check_launch("icp_transform");
}

size_t naruto_icp_accumulate_workspace(uint64_t n) {
    return (n == 0 || n > kReconMaxCount) ? 0 : icp_ws(n, nullptr).total;
}

int naruto_icp_accumulate(uint64_t n, const float* points, uint64_t n_targets, const float* targets, const int32_t* index, const double* dist,
                          double max_distance, const double* origin, void* workspace, double* sums, void* stream) {
    if (n == 0 || n_targets == 0) return fail(NARUTO_ERR_INVALID, "icp_accumulate: zero points");
    if (n > kReconMaxCount || n_targets > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "icp_accumulate: counts beyond int32");
    if (std::isnan(max_distance) || max_distance < 0.0) return fail(NARUTO_ERR_INVALID, "icp_accumulate: the correspondence distance must be a number >= 0");
    IcpOrigin o;
    if (int rc = icp_origin(origin, "icp_accumulate", &o)) return rc;
    if (points == nullptr || targets == nullptr || index == nullptr || dist == nullptr || workspace == nullptr || sums == nullptr)
        return fail(NARUTO_ERR_INVALID, "icp_accumulate: NULL argument");
    const IcpWs w = icp_ws(n, workspace);
    hipLaunchKernelGGL(k_icp_accumulate, dim3(w.parts), dim3(kIcpThreads), 0, (hipStream_t)stream, (uint32_t)n, points, (uint32_t)n_targets, targets, index, dist,
                       max_distance, o, w.part);
    if (int rc = check_launch("icp_accumulate")) return rc;
    hipLaunchKernelGGL(k_icp_accumulate_finish, dim3(1), dim3(kIcpThreads), 0, (hipStream_t)stream, w.parts, w.part, sums);
    return check_launch("icp_accumulate_finish");
}

int naruto_icp_step(const double* sums, uint64_t n_source, const double* origin, uint32_t max_iteration, double relative_fitness, double relative_rmse,
                    double* state, void* stream) {
    if (n_source == 0) return fail(NARUTO_ERR_INVALID, "icp_step: zero points");
    if (n_source > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "icp_step: counts beyond int32");
    if (std::isnan(relative_fitness) || std::isnan(relative_rmse)) return fail(NARUTO_ERR_INVALID, "icp_step: a convergence criterion is not a number");
    IcpOrigin o;
    if (int rc = icp_origin(origin, "icp_step", &o)) return rc;
    if (sums == nullptr || state == nullptr) return fail(NARUTO_ERR_INVALID, "icp_step: NULL argument");
    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, (double)n_source, o, (double)max_iteration, relative_fitness, relative_rmse, state);
    return check_launch("icp_step");
}

// ---- depth odometry (naruto_odom.hip) -----------------------------------------------------------------------------------
namespace {
// the pyramid of a desc: sizes, intrinsics (float32, level by level), where each level's maps start; false when the desc is refused
bool odom_geom(const NarutoOdomDesc* d, const char* who, OdomGeom* g) {
    if (d == nullptr) { fail(NARUTO_ERR_INVALID, "%s: NULL desc", who); return false; }
    if (d->H == 0u || d->W == 0u || d->H > 16384u || d->W > 16384u || (uint64_t)d->H * d->W > (1ull << 27)) {
        fail(NARUTO_ERR_INVALID, "%s: a frame of %u x %u pixels", who, d->H, d->W);
        return false;
    }
    if (d->levels == 0u || d->levels > (uint32_t)kOdomMaxLevels) { fail(NARUTO_ERR_INVALID, "%s: %u levels (1 .. %d)", who, d->levels, kOdomMaxLevels); return false; }
    if (!(d->fx > 0.0f) || !(d->fy > 0.0f) || !std::isfinite(d->fx) || !std::isfinite(d->fy) || !std::isfinite(d->cx) || !std::isfinite(d->cy)) {
        fail(NARUTO_ERR_INVALID, "%s: intrinsics must be finite and the focal lengths positive", who);
        return false;
    }
    if (!(d->max_dist >= 0.0f) || !(d->jump >= 0.0f) || !(d->band >= 0.0f)) { fail(NARUTO_ERR_INVALID, "%s: a threshold is negative or not a number", who); return false; }
    *g = OdomGeom{};
    g->levels = d->levels; g->W = d->W; g->band = d->band; g->jump = d->jump;
    uint32_t h = d->H, w = d->W, start = 0u, offset = 0u;
    float fx = d->fx, fy = d->fy, cx = d->cx, cy = d->cy;
    for (uint32_t l = 0; l < d->levels; ++l) {
        g->lv[l] = OdomLevel{h, w, start, offset, fx, fy, cx, cy};
        start += h * w;
        offset += 7u * h * w;
        h /= 2u; w /= 2u;
        fx = fx / 2.0f; fy = fy / 2.0f;
        cx = (cx + 0.5f) / 2.0f - 0.5f; cy = (cy + 0.5f) / 2.0f - 0.5f;
    }
    g->total = start;
    return true;
}
uint32_t odom_parts(const OdomLevel& lv) {
    const uint32_t n = lv.h * lv.w, per = kOdomThreads * kOdomPer;
    return n == 0u ? 1u : (n + per - 1u) / per;
}
}  // namespace

size_t naruto_odom_maps_bytes(const NarutoOdomDesc* desc) {
    OdomGeom g;
    return odom_geom(desc, "odom_maps_bytes", &g) ? (size_t)g.total * 7u * sizeof(float) : 0;
}

size_t naruto_odom_workspace_bytes(const NarutoOdomDesc* desc) {
    OdomGeom g;
    return odom_geom(desc, "odom_workspace_bytes", &g) ? (size_t)odom_parts(g.lv[0]) * kOdomSums * sizeof(double) : 0;
}

int naruto_odom_frame_maps(const NarutoOdomDesc* desc, const float* depth, float* maps, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_frame_maps", &g)) return NARUTO_ERR_INVALID;
    if (depth == nullptr || maps == nullptr) return fail(NARUTO_ERR_INVALID, "odom_frame_maps: NULL argument");
    hipLaunchKernelGGL(k_odom_maps, dim3((g.total + kOdomThreads - 1u) / kOdomThreads), dim3(kOdomThreads), 0, (hipStream_t)stream, g, depth, maps);
    return check_launch("odom_maps");
}

int naruto_odom_state_init(const NarutoOdomInit* T_init, const float* est, uint32_t num_frames, uint32_t i, int32_t const_speed, double* state, void* stream) {
    if (state == nullptr) return fail(NARUTO_ERR_INVALID, "odom_state_init: NULL state");
    OdomInit init{};
    int32_t mode = 2;
    if (T_init != nullptr) {
        for (int k = 0; k < 16; ++k) {
            if (!std::isfinite(T_init->T[k])) return fail(NARUTO_ERR_INVALID, "odom_state_init: the initial transform is not finite");
            init.T[k] = T_init->T[k];
        }
        mode = 0;
    } else if (est != nullptr && const_speed != 0 && i > 1u) {
        if (i >= num_frames) return fail(NARUTO_ERR_INVALID, "odom_state_init: frame %u of %u", i, num_frames);
        mode = 1;
    }
    hipLaunchKernelGGL(k_odom_init, dim3(1), dim3(64), 0, (hipStream_t)stream, mode, init, est, i, state);
    return check_launch("odom_init");
}

int naruto_odom_accumulate(const NarutoOdomDesc* desc, uint32_t level, const float* maps_prev, const float* maps_cur, const double* state, double* sums,
                           void* workspace, double* rows, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_accumulate", &g)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_accumulate: level %u of %u", level, g.levels);
    if (maps_prev == nullptr || maps_cur == nullptr || state == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_accumulate: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv);
    const double md = (double)desc->max_dist;
    hipLaunchKernelGGL(k_odom_accumulate, dim3(parts), dim3(kOdomThreads), 0, (hipStream_t)stream, lv, (int32_t)level, md * md, maps_prev, maps_cur, state,
                       reinterpret_cast<double*>(workspace), rows);
    if (int rc = check_launch("odom_accumulate")) return rc;
    hipLaunchKernelGGL(k_odom_finish, dim3(1), dim3(kOdomThreads), 0, (hipStream_t)stream, (int32_t)level, state, parts,
                       reinterpret_cast<const double*>(workspace), sums);
    return check_launch("odom_finish");
}

int naruto_odom_step(const NarutoOdomDesc* desc, uint32_t level, const double* sums, double* state, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_step", &g)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_step: level %u of %u", level, g.levels);
    if (sums == nullptr || state == nullptr) return fail(NARUTO_ERR_INVALID, "odom_step: NULL argument");
    const uint32_t cap = desc->iters[g.levels - 1u - level];
    hipLaunchKernelGGL(k_odom_step, dim3(1), dim3(64), 0, (hipStream_t)stream, (int32_t)level, (double)cap, sums, state);
    return check_launch("odom_step");
}

size_t naruto_odom_rgbd_maps_bytes(const NarutoOdomDesc* desc) {
    OdomGeom g;
    return odom_geom(desc, "odom_rgbd_maps_bytes", &g) ? (size_t)g.total * 10u * sizeof(float) : 0;
}

size_t naruto_odom_rgbd_workspace_bytes(const NarutoOdomDesc* desc) {
    OdomGeom g;
    return odom_geom(desc, "odom_rgbd_workspace_bytes", &g) ? (size_t)odom_parts(g.lv[0]) * kOdomRgbdSums * sizeof(double) : 0;
}

int naruto_odom_rgbd_frame_maps(const NarutoOdomDesc* desc, const float* depth, const float* color, float* maps, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_rgbd_frame_maps", &g)) return NARUTO_ERR_INVALID;
    if (depth == nullptr || color == nullptr || maps == nullptr) return fail(NARUTO_ERR_INVALID, "odom_rgbd_frame_maps: NULL argument");
    hipLaunchKernelGGL(k_odom_rgbd_maps, dim3((g.total + kOdomThreads - 1u) / kOdomThreads), dim3(kOdomThreads), 0, (hipStream_t)stream, g, depth, color, maps);
    return check_launch("odom_rgbd_maps");
}

int naruto_odom_rgbd_accumulate(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* maps_prev, const float* maps_cur,
                                const double* state, double* sums, void* workspace, double* rows, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_rgbd_accumulate", &g)) return NARUTO_ERR_INVALID;
    if (photo == nullptr) return fail(NARUTO_ERR_INVALID, "odom_rgbd_accumulate: NULL photo");
    if (!(photo->weight >= 0.0f) || !std::isfinite(photo->weight) || !(photo->max_diff >= 0.0f))
        return fail(NARUTO_ERR_INVALID, "odom_rgbd_accumulate: the photometric weight must be finite and >= 0, max_diff >= 0");
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_rgbd_accumulate: level %u of %u", level, g.levels);
    if (maps_prev == nullptr || maps_cur == nullptr || state == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_rgbd_accumulate: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv), ioff = g.total * 7u + lv.start * 3u;
    const double md = (double)desc->max_dist;
    hipLaunchKernelGGL(k_odom_rgbd_accumulate, dim3(parts), dim3(kOdomThreads), 0, (hipStream_t)stream, lv, ioff, (int32_t)level, md * md,
                       (double)photo->weight, (double)photo->max_diff, maps_prev, maps_cur, state, reinterpret_cast<double*>(workspace), rows);
    if (int rc = check_launch("odom_rgbd_accumulate")) return rc;
    hipLaunchKernelGGL(k_odom_rgbd_finish, dim3(1), dim3(kOdomThreads), 0, (hipStream_t)stream, (int32_t)level, state, parts,
                       reinterpret_cast<const double*>(workspace), sums);
    return check_launch("odom_rgbd_finish");
}

// ---- scored starts and a verdict for the odometry prior -------------------------------------------------------------------
extern "C++" {
namespace {
template <int K>
int odom_score_launch(bool photo_on, const OdomLevel& lv, uint32_t ioff, uint32_t parts, double md2, double trunc2, double max_diff, const float* maps_prev,
                      const float* maps_cur, const double* cands, double* sums, double* part, hipStream_t stream) {
    if (photo_on)
        hipLaunchKernelGGL((k_odom_score<K, true>), dim3(parts), dim3(kOdomThreads), 0, stream, lv, ioff, md2, trunc2, max_diff, maps_prev, maps_cur, cands, part);
    else
        hipLaunchKernelGGL((k_odom_score<K, false>), dim3(parts), dim3(kOdomThreads), 0, stream, lv, ioff, md2, trunc2, max_diff, maps_prev, maps_cur, cands, part);
    if (int rc = check_launch("odom_score")) return rc;
    hipLaunchKernelGGL((k_odom_score_finish<K>), dim3(1), dim3(kOdomThreads), 0, stream, parts, (const double*)part, sums);
    return check_launch("odom_score_finish");
}
}  // namespace
}  // extern "C++"

size_t naruto_odom_score_workspace_bytes(const NarutoOdomDesc* desc, uint32_t K) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_score_workspace_bytes", &g)) return 0;
    if (K == 0u || K > (uint32_t)kOdomMaxCands) { fail(NARUTO_ERR_INVALID, "odom_score_workspace_bytes: %u candidates (1 .. %d)", K, kOdomMaxCands); return 0; }
    return (size_t)odom_parts(g.lv[0]) * (1u + 4u * K) * sizeof(double);
}

int naruto_odom_score(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* maps_prev, const float* maps_cur,
                      const double* cands, uint32_t K, double trunc, double* sums, void* workspace, void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_score", &g)) return NARUTO_ERR_INVALID;
    if (photo != nullptr && (!(photo->weight >= 0.0f) || !std::isfinite(photo->weight) || !(photo->max_diff >= 0.0f)))
        return fail(NARUTO_ERR_INVALID, "odom_score: the photometric weight must be finite and >= 0, max_diff >= 0");
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_score: level %u of %u", level, g.levels);
    if (K == 0u || K > (uint32_t)kOdomMaxCands) return fail(NARUTO_ERR_INVALID, "odom_score: %u candidates (1 .. %d)", K, kOdomMaxCands);
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return fail(NARUTO_ERR_INVALID, "odom_score: trunc must be a finite positive number of metres");
    if (maps_prev == nullptr || maps_cur == nullptr || cands == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_score: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv), ioff = g.total * 7u + lv.start * 3u;     // ioff is read with a photometric term only (RGB-D blocks)
    const double md = (double)desc->max_dist;
    const bool photo_on = photo != nullptr && photo->weight > 0.0f;
    const double max_diff = photo != nullptr ? (double)photo->max_diff : 0.0;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
        case 1: return odom_score_launch<1>(photo_on, lv, ioff, parts, md * md, trunc * trunc, max_diff, maps_prev, maps_cur, cands, sums, part, st);
        case 2: return odom_score_launch<2>(photo_on, lv, ioff, parts, md * md, trunc * trunc, max_diff, maps_prev, maps_cur, cands, sums, part, st);
        case 3: return odom_score_launch<3>(photo_on, lv, ioff, parts, md * md, trunc * trunc, max_diff, maps_prev, maps_cur, cands, sums, part, st);
        default: return odom_score_launch<4>(photo_on, lv, ioff, parts, md * md, trunc * trunc, max_diff, maps_prev, maps_cur, cands, sums, part, st);
    }
}

int naruto_odom_candidates(const float* est, uint32_t num_frames, uint32_t i, double* cands, void* stream) {
    if (est == nullptr || cands == nullptr) return fail(NARUTO_ERR_INVALID, "odom_candidates: NULL argument");
    if (i >= num_frames) return fail(NARUTO_ERR_INVALID, "odom_candidates: frame %u of %u", i, num_frames);
    hipLaunchKernelGGL(k_odom_candidates, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, cands);
    return check_launch("odom_candidates");
}

int naruto_odom_choose(uint32_t K, const double* sums, const double* cands, int32_t photo_on, double trunc, double photo_max_diff, double* state,
                       double* record, void* stream) {
    if (K == 0u || K > (uint32_t)kOdomMaxCands) return fail(NARUTO_ERR_INVALID, "odom_choose: %u candidates (1 .. %d)", K, kOdomMaxCands);
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return fail(NARUTO_ERR_INVALID, "odom_choose: trunc must be a finite positive number of metres");
    if (photo_on != 0 && (!(photo_max_diff > 0.0) || !std::isfinite(photo_max_diff)))
        return fail(NARUTO_ERR_INVALID, "odom_choose: photo_max_diff must be a finite positive number when the photometric cost is on");
    if (sums == nullptr || cands == nullptr || state == nullptr || record == nullptr) return fail(NARUTO_ERR_INVALID, "odom_choose: NULL argument");
    hipLaunchKernelGGL(k_odom_choose, dim3(1), dim3(64), 0, (hipStream_t)stream, K, photo_on, trunc, photo_max_diff, sums, cands, state, record);
    return check_launch("odom_choose");
}

int naruto_odom_verdict(const NarutoOdomDesc* desc, const NarutoOdomGate* gate, const double* sums, const double* cands, double* state, double* record,
                        void* stream) {
    OdomGeom g;
    if (!odom_geom(desc, "odom_verdict", &g)) return NARUTO_ERR_INVALID;
    if (gate == nullptr) return fail(NARUTO_ERR_INVALID, "odom_verdict: NULL gate");
    if (!(gate->max_trans >= 0.0) || !(gate->min_trace >= -1.0 && gate->min_trace <= 3.0) || !(gate->min_overlap >= 0.0 && gate->min_overlap <= 1.0) ||
        !(gate->max_rmse >= 0.0) || !std::isfinite(gate->max_trans) || !std::isfinite(gate->max_rmse))
        return fail(NARUTO_ERR_INVALID, "odom_verdict: the gate needs finite max_trans, max_rmse >= 0, min_trace in -1 .. 3, min_overlap in 0 .. 1");
    if (sums == nullptr || cands == nullptr || state == nullptr || record == nullptr) return fail(NARUTO_ERR_INVALID, "odom_verdict: NULL argument");
    hipLaunchKernelGGL(k_odom_verdict, dim3(1), dim3(64), 0, (hipStream_t)stream, OdomGate{gate->max_trans, gate->min_trace, gate->min_overlap, gate->max_rmse},
                       sums, cands, state, record);
    return check_launch("odom_verdict");
}

int naruto_pose_predict_relative(float* est, uint32_t num_frames, uint32_t i, const double* state_T, float* pose6_out, void* stream) {
    if (est == nullptr || state_T == nullptr || pose6_out == nullptr) return fail(NARUTO_ERR_INVALID, "pose_predict_relative: NULL argument");
    if (i < 1u || i >= num_frames) return fail(NARUTO_ERR_INVALID, "pose_predict_relative: frame %u of %u (the first frame is given, not predicted)", i, num_frames);
    hipLaunchKernelGGL(k_pose_predict_relative, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, state_T, pose6_out);
    return check_launch("pose_predict_relative");
}

// ---- keyframe-anchored odometry prior (naruto_odom_anchor.hip) --------------------------------------------------------------
namespace {
static_assert(kOdomMaxRefs == NARUTO_ODOM_MAX_REFS && kOdomAnchorHead == NARUTO_ODOM_ANCHOR_HEAD && kOdomAnchorWords == NARUTO_ODOM_ANCHOR_WORDS, "naruto_hip.h");
// what every call on a ring checks: the desc, the photometric term and the slot count; the ring's stride in floats (photo given: RGB-D blocks)
bool odom_ring(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t slots, const char* who, OdomGeom* g, uint64_t* stride) {
    if (!odom_geom(desc, who, g)) return false;
    if (photo != nullptr && (!(photo->weight >= 0.0f) || !std::isfinite(photo->weight) || !(photo->max_diff >= 0.0f))) {
        fail(NARUTO_ERR_INVALID, "%s: the photometric weight must be finite and >= 0, max_diff >= 0", who);
        return false;
    }
    if (slots == 0u || slots > (uint32_t)kOdomMaxRefs) { fail(NARUTO_ERR_INVALID, "%s: %u slots (1 .. %d)", who, slots, kOdomMaxRefs); return false; }
    *stride = (uint64_t)g->total * (photo != nullptr ? 10u : 7u);
    return true;
}
}  // namespace

size_t naruto_odom_score_refs_workspace_bytes(const NarutoOdomDesc* desc, uint32_t slots) {
    OdomGeom g;
    uint64_t stride;
    if (!odom_ring(desc, nullptr, slots, "odom_score_refs_workspace_bytes", &g, &stride)) return 0;
    return (size_t)slots * odom_parts(g.lv[0]) * kOdomRefSums * sizeof(double);
}

int naruto_odom_anchor_candidates(const float* est, uint32_t num_frames, uint32_t i, const int32_t* head, uint32_t slots, double* cands, void* stream) {
    if (est == nullptr || head == nullptr || cands == nullptr) return fail(NARUTO_ERR_INVALID, "odom_anchor_candidates: NULL argument");
    if (i < 1u || i >= num_frames) return fail(NARUTO_ERR_INVALID, "odom_anchor_candidates: frame %u of %u (the first frame has no reference)", i, num_frames);
    if (slots == 0u || slots > (uint32_t)kOdomMaxRefs) return fail(NARUTO_ERR_INVALID, "odom_anchor_candidates: %u slots (1 .. %d)", slots, kOdomMaxRefs);
    hipLaunchKernelGGL(k_odom_anchor_candidates, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, head, slots, cands);
    return check_launch("odom_anchor_candidates");
}

int naruto_odom_score_refs(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head, uint32_t slots,
                           const float* maps_cur, const double* cands, double trunc, double* sums, void* workspace, void* stream) {
    OdomGeom g;
    uint64_t stride;
    if (!odom_ring(desc, photo, slots, "odom_score_refs", &g, &stride)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_score_refs: level %u of %u", level, g.levels);
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return fail(NARUTO_ERR_INVALID, "odom_score_refs: trunc must be a finite positive number of metres");
    if (ring == nullptr || head == nullptr || maps_cur == nullptr || cands == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_score_refs: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv), ioff = g.total * 7u + lv.start * 3u;
    const double md = (double)desc->max_dist, max_diff = photo != nullptr ? (double)photo->max_diff : 0.0;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (photo != nullptr && photo->weight > 0.0f)
        hipLaunchKernelGGL((k_odom_score_refs<true>), dim3(parts, slots), dim3(kOdomThreads), 0, st, lv, ioff, md * md, trunc * trunc, max_diff, stride, parts, head,
                           ring, maps_cur, cands, part);
    else
        hipLaunchKernelGGL((k_odom_score_refs<false>), dim3(parts, slots), dim3(kOdomThreads), 0, st, lv, ioff, md * md, trunc * trunc, max_diff, stride, parts, head,
                           ring, maps_cur, cands, part);
    if (int rc = check_launch("odom_score_refs")) return rc;
    hipLaunchKernelGGL(k_odom_score_refs_finish, dim3(slots), dim3(kOdomThreads), 0, st, parts, head, (const double*)part, sums);
    return check_launch("odom_score_refs_finish");
}

int naruto_odom_anchor_choose(uint32_t slots, const double* sums, const double* cands_all, int32_t photo_on, double trunc, double photo_max_diff, int32_t* head,
                              double* cands, double* state, double* record, double* anchor_record, void* stream) {
    if (slots == 0u || slots > (uint32_t)kOdomMaxRefs) return fail(NARUTO_ERR_INVALID, "odom_anchor_choose: %u slots (1 .. %d)", slots, kOdomMaxRefs);
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return fail(NARUTO_ERR_INVALID, "odom_anchor_choose: trunc must be a finite positive number of metres");
    if (photo_on != 0 && (!(photo_max_diff > 0.0) || !std::isfinite(photo_max_diff)))
        return fail(NARUTO_ERR_INVALID, "odom_anchor_choose: photo_max_diff must be a finite positive number when the photometric cost is on");
    if (sums == nullptr || cands_all == nullptr || head == nullptr || cands == nullptr || state == nullptr || record == nullptr || anchor_record == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_anchor_choose: NULL argument");
    hipLaunchKernelGGL(k_odom_anchor_choose, dim3(1), dim3(64), 0, (hipStream_t)stream, slots, photo_on, trunc, photo_max_diff, sums, cands_all, head, cands, state,
                       record, anchor_record);
    return check_launch("odom_anchor_choose");
}

int naruto_odom_accumulate_anchored(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head,
                                    uint32_t slots, const float* maps_cur, const double* state, double* sums, void* workspace, void* stream) {
    OdomGeom g;
    uint64_t stride;
    if (!odom_ring(desc, photo, slots, "odom_accumulate_anchored", &g, &stride)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_accumulate_anchored: level %u of %u", level, g.levels);
    if (ring == nullptr || head == nullptr || maps_cur == nullptr || state == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_accumulate_anchored: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv), ioff = g.total * 7u + lv.start * 3u;
    const double md = (double)desc->max_dist;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (photo == nullptr) {
        hipLaunchKernelGGL(k_odom_accumulate_anchored, dim3(parts), dim3(kOdomThreads), 0, st, lv, (int32_t)level, md * md, stride, slots, head, ring, maps_cur, state,
                           part);
        if (int rc = check_launch("odom_accumulate_anchored")) return rc;
        hipLaunchKernelGGL(k_odom_finish, dim3(1), dim3(kOdomThreads), 0, st, (int32_t)level, state, parts, (const double*)part, sums);
        return check_launch("odom_finish");
    }
    hipLaunchKernelGGL(k_odom_rgbd_accumulate_anchored, dim3(parts), dim3(kOdomThreads), 0, st, lv, ioff, (int32_t)level, md * md, (double)photo->weight,
                       (double)photo->max_diff, stride, slots, head, ring, maps_cur, state, part);
    if (int rc = check_launch("odom_rgbd_accumulate_anchored")) return rc;
    hipLaunchKernelGGL(k_odom_rgbd_finish, dim3(1), dim3(kOdomThreads), 0, st, (int32_t)level, state, parts, (const double*)part, sums);
    return check_launch("odom_rgbd_finish");
}

int naruto_odom_score_anchored(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t level, const float* ring, const int32_t* head, uint32_t slots,
                               const float* maps_cur, const double* cands, double trunc, double* sums, void* workspace, void* stream) {
    OdomGeom g;
    uint64_t stride;
    if (!odom_ring(desc, photo, slots, "odom_score_anchored", &g, &stride)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "odom_score_anchored: level %u of %u", level, g.levels);
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return fail(NARUTO_ERR_INVALID, "odom_score_anchored: trunc must be a finite positive number of metres");
    if (ring == nullptr || head == nullptr || maps_cur == nullptr || cands == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "odom_score_anchored: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv), ioff = g.total * 7u + lv.start * 3u;
    const double md = (double)desc->max_dist, max_diff = photo != nullptr ? (double)photo->max_diff : 0.0;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (photo != nullptr && photo->weight > 0.0f)
        hipLaunchKernelGGL((k_odom_score_anchored<true>), dim3(parts), dim3(kOdomThreads), 0, st, lv, ioff, md * md, trunc * trunc, max_diff, stride, slots, head, ring,
                           maps_cur, cands, part);
    else
        hipLaunchKernelGGL((k_odom_score_anchored<false>), dim3(parts), dim3(kOdomThreads), 0, st, lv, ioff, md * md, trunc * trunc, max_diff, stride, slots, head, ring,
                           maps_cur, cands, part);
    if (int rc = check_launch("odom_score_anchored")) return rc;
    hipLaunchKernelGGL((k_odom_score_finish<1>), dim3(1), dim3(kOdomThreads), 0, st, parts, (const double*)part, sums);
    return check_launch("odom_score_finish");
}

int naruto_odom_anchor_update(const NarutoOdomAnchor* anchor, uint32_t i, const double* record, int32_t* head, double* anchor_record, void* stream) {
    if (anchor == nullptr || record == nullptr || head == nullptr || anchor_record == nullptr) return fail(NARUTO_ERR_INVALID, "odom_anchor_update: NULL argument");
    if (anchor->slots == 0u || anchor->slots > (uint32_t)kOdomMaxRefs) return fail(NARUTO_ERR_INVALID, "odom_anchor_update: %u slots (1 .. %d)", anchor->slots, kOdomMaxRefs);
    if (anchor->refail == 0u || anchor->refail > (1u << 30)) return fail(NARUTO_ERR_INVALID, "odom_anchor_update: refail = %u (at least 1)", anchor->refail);
    if (!(anchor->min_overlap >= 0.0 && anchor->min_overlap <= 1.0) || !(anchor->max_trans >= 0.0) || !std::isfinite(anchor->max_trans) ||
        !(anchor->min_trace >= -1.0 && anchor->min_trace <= 3.0))
        return fail(NARUTO_ERR_INVALID, "odom_anchor_update: the policy needs min_overlap in 0 .. 1, a finite max_trans >= 0 and min_trace in -1 .. 3");
    if (i > 0x7fffffffu) return fail(NARUTO_ERR_INVALID, "odom_anchor_update: frame %u", i);
    hipLaunchKernelGGL(k_odom_anchor_update, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       OdomAnchor{anchor->min_overlap, anchor->max_trans, anchor->min_trace, anchor->slots, anchor->refail}, i, record, head, anchor_record);
    return check_launch("odom_anchor_update");
}

int naruto_odom_anchor_promote(const NarutoOdomDesc* desc, const NarutoOdomPhoto* photo, uint32_t slots, const int32_t* head, const float* maps_cur, float* ring,
                               void* stream) {
    OdomGeom g;
    uint64_t stride;
    if (!odom_ring(desc, photo, slots, "odom_anchor_promote", &g, &stride)) return NARUTO_ERR_INVALID;
    if (head == nullptr || maps_cur == nullptr || ring == nullptr) return fail(NARUTO_ERR_INVALID, "odom_anchor_promote: NULL argument");
    const uint64_t groups = (stride + 1023u) / 1024u;                     // four floats per thread when the block vectorises
    hipLaunchKernelGGL(k_odom_anchor_promote, dim3((uint32_t)std::min<uint64_t>(groups, 4096u)), dim3(256), 0, (hipStream_t)stream, stride, slots, head, maps_cur,
                       ring);
    return check_launch("odom_anchor_promote");
}

int naruto_pose_predict_anchored(float* est, uint32_t num_frames, uint32_t i, const double* anchor_record, const double* state_T, float* pose6_out, void* stream) {
    if (est == nullptr || anchor_record == nullptr || state_T == nullptr || pose6_out == nullptr)
        return fail(NARUTO_ERR_INVALID, "pose_predict_anchored: NULL argument");
    if (i < 1u || i >= num_frames) return fail(NARUTO_ERR_INVALID, "pose_predict_anchored: frame %u of %u (the first frame is given, not predicted)", i, num_frames);
    hipLaunchKernelGGL(k_pose_predict_anchored, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, anchor_record, state_T, pose6_out);
    return check_launch("pose_predict_anchored");
}

// ---- frame-to-model alignment (naruto_sdfreg.hip) -------------------------------------------------------------------------
namespace {
static_assert(kSdfRegSums == NARUTO_SDFREG_SUMS && kSdfRegStateDoubles == NARUTO_SDFREG_STATE_DOUBLES && kSdfRegRecord == NARUTO_SDFREG_RECORD, "naruto_hip.h");
// the registration's desc: false when it is refused
bool sdfreg_desc(const NarutoSdfRegDesc* r, const OdomGeom& g, const char* who, SdfRegBox* box) {
    if (r == nullptr) { fail(NARUTO_ERR_INVALID, "%s: NULL registration desc", who); return false; }
    if (!(r->trunc > 0.0f) || !std::isfinite(r->trunc) || !(r->sdf_gate > 0.0f) || !std::isfinite(r->sdf_gate)) {
        fail(NARUTO_ERR_INVALID, "%s: trunc and sdf_gate must be finite and positive", who);
        return false;
    }
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(r->bbox_min[a]) || !std::isfinite(r->bbox_max[a]) || !(r->bbox_max[a] > r->bbox_min[a])) {
            fail(NARUTO_ERR_INVALID, "%s: the bounding box must be finite with bbox_max > bbox_min", who);
            return false;
        }
        box->lo[a] = r->bbox_min[a]; box->hi[a] = r->bbox_max[a];
    }
    if (r->n_levels == 0u || r->n_levels > g.levels) { fail(NARUTO_ERR_INVALID, "%s: %u levels of a pyramid of %u", who, r->n_levels, g.levels); return false; }
    for (uint32_t k = 0; k < r->n_levels; ++k) {
        if (r->levels[k] >= g.levels || (k > 0u && r->levels[k] >= r->levels[k - 1u]) || r->iters[k] == 0u) {
            fail(NARUTO_ERR_INVALID, "%s: the levels run from the coarsest to the finest inside the pyramid, each with a cap >= 1", who);
            return false;
        }
    }
    return true;
}
}  // namespace

size_t naruto_sdfreg_workspace_bytes(const NarutoOdomDesc* odom) {
    OdomGeom g;
    return odom_geom(odom, "sdfreg_workspace_bytes", &g) ? (size_t)odom_parts(g.lv[0]) * kSdfRegSums * sizeof(double) : 0;
}

int naruto_sdfreg_points(const NarutoOdomDesc* odom, const NarutoSdfRegDesc* reg, uint32_t level, int32_t gated, const float* maps_cur, const double* state,
                         float* x, float* q, uint8_t* valid, void* stream) {
    OdomGeom g;
    SdfRegBox box;
    if (!odom_geom(odom, "sdfreg_points", &g) || !sdfreg_desc(reg, g, "sdfreg_points", &box)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "sdfreg_points: level %u of %u", level, g.levels);
    if (maps_cur == nullptr || state == nullptr || x == nullptr || q == nullptr || valid == nullptr) return fail(NARUTO_ERR_INVALID, "sdfreg_points: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t n = lv.h * lv.w;
    hipLaunchKernelGGL(k_sdfreg_points, dim3(odom_parts(lv)), dim3(kOdomThreads), 0, (hipStream_t)stream, n, (int32_t)level, gated, box,
                       maps_cur + lv.offset + n, state, x, q, valid);
    return check_launch("sdfreg_points");
}

int naruto_sdfreg_accumulate(const NarutoOdomDesc* odom, const NarutoSdfRegDesc* reg, uint32_t level, int32_t gated, const float* sdf_uncert, const float* d_x,
                             const float* q, const uint8_t* valid, const double* state, double* sums, void* workspace, double* rows, void* stream) {
    OdomGeom g;
    SdfRegBox box;
    if (!odom_geom(odom, "sdfreg_accumulate", &g) || !sdfreg_desc(reg, g, "sdfreg_accumulate", &box)) return NARUTO_ERR_INVALID;
    if (level >= g.levels) return fail(NARUTO_ERR_INVALID, "sdfreg_accumulate: level %u of %u", level, g.levels);
    if (sdf_uncert == nullptr || d_x == nullptr || q == nullptr || valid == nullptr || state == nullptr || sums == nullptr || workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "sdfreg_accumulate: NULL argument");
    const OdomLevel lv = g.lv[level];
    const uint32_t parts = odom_parts(lv);
    hipLaunchKernelGGL(k_sdfreg_accumulate, dim3(parts), dim3(kOdomThreads), 0, (hipStream_t)stream, lv.h * lv.w, (int32_t)level, gated, (double)reg->trunc,
                       (double)reg->sdf_gate, box, sdf_uncert, d_x, q, valid, state, reinterpret_cast<double*>(workspace), rows);
    if (int rc = check_launch("sdfreg_accumulate")) return rc;
    hipLaunchKernelGGL(k_sdfreg_finish, dim3(1), dim3(kOdomThreads), 0, (hipStream_t)stream, (int32_t)level, gated, state, parts,
                       reinterpret_cast<const double*>(workspace), sums);
    return check_launch("sdfreg_finish");
}

int naruto_sdfreg_init(const float* est, uint32_t num_frames, uint32_t i, double* state, void* stream) {
    if (est == nullptr || state == nullptr) return fail(NARUTO_ERR_INVALID, "sdfreg_init: NULL argument");
    if (i >= num_frames) return fail(NARUTO_ERR_INVALID, "sdfreg_init: frame %u of %u", i, num_frames);
    hipLaunchKernelGGL(k_sdfreg_init, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, state);
    return check_launch("sdfreg_init");
}

int naruto_sdfreg_verdict(const NarutoSdfRegDesc* reg, const NarutoSdfRegGate* gate, const double* sums_start, const double* sums_final, double* state,
                          double* record, void* stream) {
    if (reg == nullptr || gate == nullptr) return fail(NARUTO_ERR_INVALID, "sdfreg_verdict: NULL desc or gate");
    if (reg->n_levels == 0u || reg->n_levels > (uint32_t)kOdomMaxLevels || reg->levels[reg->n_levels - 1u] >= (uint32_t)kOdomMaxLevels)
        return fail(NARUTO_ERR_INVALID, "sdfreg_verdict: the desc names no finest level");
    if (!(gate->max_trans >= 0.0) || !std::isfinite(gate->max_trans) || !(gate->min_trace >= -1.0 && gate->min_trace <= 3.0) ||
        !(gate->min_overlap >= 0.0 && gate->min_overlap <= 1.0))
        return fail(NARUTO_ERR_INVALID, "sdfreg_verdict: the gate needs a finite max_trans >= 0, min_trace in -1 .. 3, min_overlap in 0 .. 1");
    if (sums_start == nullptr || sums_final == nullptr || state == nullptr || record == nullptr) return fail(NARUTO_ERR_INVALID, "sdfreg_verdict: NULL argument");
    hipLaunchKernelGGL(k_sdfreg_verdict, dim3(1), dim3(64), 0, (hipStream_t)stream, SdfRegGate{gate->max_trans, gate->min_trace, gate->min_overlap},
                       (int32_t)reg->levels[reg->n_levels - 1u], sums_start, sums_final, state, record);
    return check_launch("sdfreg_verdict");
}

int naruto_sdfreg_commit(float* est, uint32_t num_frames, uint32_t i, const double* state, float* pose6_out, void* stream) {
    if (est == nullptr || state == nullptr || pose6_out == nullptr) return fail(NARUTO_ERR_INVALID, "sdfreg_commit: NULL argument");
    if (i >= num_frames) return fail(NARUTO_ERR_INVALID, "sdfreg_commit: frame %u of %u", i, num_frames);
    hipLaunchKernelGGL(k_sdfreg_commit, dim3(1), dim3(64), 0, (hipStream_t)stream, est, i, state, pose6_out);
    return check_launch("sdfreg_commit");
}

// ---- mesh culling (naruto_cull.hip) -------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kCullLargeGrid = 2048;                     // workgroups of the large route: 8 per CU, grid-stride over the chunks
int cull_cam_check(const NarutoCullCam* cam, const char* who) {
    if (cam == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL camera", who);
    if (cam->H == 0 || cam->W == 0 || cam->H >= (1u << 24) || cam->W >= (1u << 24) || (uint64_t)cam->H * cam->W > (1ull << 30))
        return fail(NARUTO_ERR_INVALID, "%s: image of %u x %u pixels (1 .. 2^30 pixels)", who, cam->W, cam->H);
    if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0f || cam->fy == 0.0f || !std::isfinite(cam->cx) || !std::isfinite(cam->cy))
        return fail(NARUTO_ERR_INVALID, "%s: intrinsics must be finite with fx, fy != 0", who);
    return NARUTO_OK;
}
CullCam cull_cam_args(const NarutoCullCam* cam) {
    CullCam c{};
    c.H = cam->H; c.W = cam->W; c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy; c.near_ = cam->near_; c.far_ = cam->far_;
    return c;
}
int cull_raster_sizes_check(const NarutoCullCam* cam, uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses, const char* who) {
    if (n_faces == 0 || n_vertices == 0 || n_poses == 0) return fail(NARUTO_ERR_INVALID, "%s: zero faces, vertices or poses", who);
    if (n_faces > kReconMaxCount || n_vertices > kReconMaxCount || n_poses > 65535u) return fail(NARUTO_ERR_INVALID, "%s: counts beyond int32 (poses: 65535 per call)", who);
    const uint64_t chunks_per_box = ((uint64_t)cam->H * cam->W + kCullChunk - 1u) / kCullChunk;
    if (n_faces * n_poses >= (1ull << 28) || n_faces * n_poses * chunks_per_box >= (1ull << kCullSlotShift))
        return fail(NARUTO_ERR_INVALID, "%s: faces x poses per call must stay below 2^28 (and x 2048-pixel chunks of the image below 2^36): use fewer poses per call", who);
    return NARUTO_OK;
}
// workspace of the depth raster: | counter of large boxes | camera-space vertices [poses][vertices] | a large box's first chunk | and its face [poses][faces] |;
// the simulator's 64-bit (depth, face) cells [poses][H][W] follow it (H = 0: the culling raster, which has none)
struct CullWs { unsigned long long* counter; float4* camv; unsigned long long* ent_start; uint32_t* ent_id; unsigned long long* cells; size_t total; };
CullWs cull_ws(uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses, void* workspace, uint32_t H = 0, uint32_t W = 0) {
    Carve c(workspace);
    return {c.take<unsigned long long>(8u), c.take<float4>((size_t)n_vertices * n_poses * 16u), c.take<unsigned long long>((size_t)n_faces * n_poses * 8u),
            c.take<uint32_t>((size_t)n_faces * n_poses * 4u), H != 0 ? c.take<unsigned long long>((size_t)n_poses * H * W * 8u) : nullptr, c.size()};
}
}  // namespace

size_t naruto_render_depth_workspace(uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses) {
    if (n_faces == 0 || n_vertices == 0 || n_poses == 0 || n_faces > kReconMaxCount || n_vertices > kReconMaxCount || n_poses > 65535u || n_faces * n_poses >= (1ull << 28)) return 0;
    return cull_ws(n_vertices, n_faces, n_poses, nullptr).total;
}

int naruto_render_depth(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const uint8_t* face_mask,
                        uint32_t n_poses, const float* poses, uint32_t large_threshold, void* workspace, float* depth, void* stream) {
    if (int rc = cull_cam_check(cam, "render_depth")) return rc;
    if (!(cam->near_ > 0.0f) || !(cam->near_ < cam->far_)) return fail(NARUTO_ERR_INVALID, "render_depth: need 0 < near < far");
    if (int rc = cull_raster_sizes_check(cam, n_vertices, n_faces, n_poses, "render_depth")) return rc;
    if (vertices == nullptr || faces == nullptr || poses == nullptr || workspace == nullptr || depth == nullptr) return fail(NARUTO_ERR_INVALID, "render_depth: NULL argument");
    const CullCam c = cull_cam_args(cam);
    const CullWs w = cull_ws(n_vertices, n_faces, n_poses, workspace);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nv = (uint32_t)n_vertices, nf = (uint32_t)n_faces, cap = (uint32_t)(n_faces * n_poses);
    uint32_t* bits = reinterpret_cast<uint32_t*>(depth);
    if (hipMemsetAsync(w.counter, 0, 8u, st) != hipSuccess) return check_launch("render_depth: memset");
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bits), (int)kCullInfBits, (size_t)n_poses * cam->H * cam->W, st) != hipSuccess) return check_launch("render_depth: fill");
    const dim3 block(kCullThreads);
    hipLaunchKernelGGL(k_cull_transform, dim3((nv + kCullThreads - 1u) / kCullThreads, n_poses), block, 0, st, nv, vertices, poses, w.camv);
    if (int rc = check_launch("cull_transform")) return rc;
    hipLaunchKernelGGL(k_cull_raster_small<uint32_t>, dim3((nf + kCullThreads - 1u) / kCullThreads, n_poses), block, 0, st, c, nf, nv, faces, face_mask, w.camv, large_threshold, bits,
                       w.counter, w.ent_id, w.ent_start, cap);
    if (int rc = check_launch("cull_raster_small")) return rc;
    // the large boxes: their number is on the device, so the launch is a fixed grid and a workgroup without a chunk leaves at once
    hipLaunchKernelGGL(k_cull_raster_large<uint32_t>, dim3(kCullLargeGrid), block, 0, st, c, nf, nv, faces, w.camv, bits, w.counter, w.ent_id, w.ent_start, cap);
    return check_launch("cull_raster_large");
}

int naruto_observed_vertices(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint32_t n_poses, const float* poses, const float* depth, float eps,
                             uint8_t* mask, void* stream) {
    if (int rc = cull_cam_check(cam, "observed_vertices")) return rc;
    if (n_vertices > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "observed_vertices: counts beyond int32");
    if (std::isnan(eps)) return fail(NARUTO_ERR_INVALID, "observed_vertices: eps is not a number");
    if (n_vertices == 0 || n_poses == 0) return NARUTO_OK;
    if (vertices == nullptr || poses == nullptr || mask == nullptr) return fail(NARUTO_ERR_INVALID, "observed_vertices: NULL argument");
    const uint32_t nv = (uint32_t)n_vertices;
    hipLaunchKernelGGL(k_cull_observed, dim3((nv + kCullThreads - 1u) / kCullThreads), dim3(kCullThreads), 0, (hipStream_t)stream, cull_cam_args(cam), nv, vertices, n_poses, poses,
                       reinterpret_cast<const uint32_t*>(depth), eps, mask);
    return check_launch("cull_observed");
}

int naruto_cull_faces(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* observed, const uint8_t* inside, uint8_t* face_keep, uint8_t* vertex_used,
                      void* stream) {
    if (n_faces > kReconMaxCount || n_vertices > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "cull_faces: counts beyond int32");
    hipStream_t st = (hipStream_t)stream;
    if (vertex_used != nullptr && n_vertices > 0 && hipMemsetAsync(vertex_used, 0, (size_t)n_vertices, st) != hipSuccess) return check_launch("cull_faces: memset");
    if (n_faces == 0) return NARUTO_OK;
    if (faces == nullptr || face_keep == nullptr) return fail(NARUTO_ERR_INVALID, "cull_faces: NULL argument");
    const uint32_t nf = (uint32_t)n_faces;
    hipLaunchKernelGGL(k_cull_faces, dim3((nf + kCullThreads - 1u) / kCullThreads), dim3(kCullThreads), 0, st, nf, (uint32_t)n_vertices, faces, observed, inside, face_keep, vertex_used);
    return check_launch("cull_faces");
}

int naruto_cull_compact(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* face_keep, const int32_t* face_pos, const uint8_t* vertex_used,
                        const int32_t* vertex_pos, const void* vertices, int vertices_f64, const uint8_t* colors, uint64_t n_out_faces, uint64_t n_out_vertices,
                        int32_t* out_faces, void* out_vertices, uint8_t* out_colors, void* stream) {
    if (n_faces > kReconMaxCount || n_vertices > kReconMaxCount || n_out_faces > n_faces || n_out_vertices > n_vertices) return fail(NARUTO_ERR_INVALID, "cull_compact: counts out of range");
    if (n_out_faces == 0 || n_out_vertices == 0) return NARUTO_OK;
    if (faces == nullptr || face_keep == nullptr || face_pos == nullptr || vertex_used == nullptr || vertex_pos == nullptr || vertices == nullptr || out_faces == nullptr ||
        out_vertices == nullptr || (colors != nullptr && out_colors == nullptr))
        return fail(NARUTO_ERR_INVALID, "cull_compact: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nf = (uint32_t)n_faces, nv = (uint32_t)n_vertices;
    hipLaunchKernelGGL(k_cull_compact_faces, dim3((nf + kCullThreads - 1u) / kCullThreads), dim3(kCullThreads), 0, st, nf, nv, faces, face_keep, face_pos, vertex_pos,
                       (uint32_t)n_out_faces, out_faces);
    if (int rc = check_launch("cull_compact_faces")) return rc;
    hipLaunchKernelGGL(k_cull_compact_vertices, dim3((nv + kCullThreads - 1u) / kCullThreads), dim3(kCullThreads), 0, st, nv, vertex_used, vertex_pos,
                       reinterpret_cast<const uint32_t*>(vertices), vertices_f64 ? 6u : 3u, reinterpret_cast<const uint32_t*>(colors), (uint32_t)n_out_vertices,
                       reinterpret_cast<uint32_t*>(out_vertices), reinterpret_cast<uint32_t*>(out_colors));
    return check_launch("cull_compact_vertices");
}

int naruto_debug_atomic_min_rate(uint64_t n_words, uint32_t n_lanes, uint32_t iters, uint32_t* buf, void* stream) {
    if (n_words == 0 || n_words > 0xFFFFFFFFull || n_lanes == 0 || iters == 0 || iters > (1u << 20)) return fail(NARUTO_ERR_INVALID, "debug_atomic_min_rate: sizes out of range");
    if (buf == nullptr) return fail(NARUTO_ERR_INVALID, "debug_atomic_min_rate: NULL argument");
    hipLaunchKernelGGL(k_cull_atomic_probe, dim3((n_lanes + kCullThreads - 1u) / kCullThreads), dim3(kCullThreads), 0, (hipStream_t)stream, (uint32_t)n_words, iters, buf);
    return check_launch("cull_atomic_probe");
}

// ---- mesh subdivision (naruto_subdiv.hip) ---------------------------------------------------------------------------------
namespace {
constexpr uint64_t kSubdivMaxLong = kReconMaxCount / 3u;       // slot ordinals 3 * rank + slot stay below 2^31
constexpr uint64_t kSubdivMaxTable = 1ull << 31;
// workspace of one generation: | error word | keys [table] | lowest slot ordinal of the key [table] | table cell of every slot [3 n_long] |
struct SubdivWs { uint32_t* err; unsigned long long* keys; uint32_t* ord; uint32_t* pos; size_t total; };
SubdivWs subdiv_ws(uint64_t n_long, uint64_t table_slots, void* workspace) {
    Carve c(workspace);
    return {c.take<uint32_t>(4u), c.take<unsigned long long>((size_t)table_slots * 8u), c.take<uint32_t>((size_t)table_slots * 4u), c.take<uint32_t>((size_t)n_long * 12u), c.size()};
}
bool subdiv_sizes_ok(uint64_t n_long, uint64_t table_slots) {
    return n_long != 0 && n_long <= kSubdivMaxLong && table_slots >= 6u * n_long && table_slots <= kSubdivMaxTable;
}
}  // namespace

size_t naruto_subdivide_workspace(uint64_t n_long, uint64_t table_slots) {
    if (!subdiv_sizes_ok(n_long, table_slots)) return 0;
    return subdiv_ws(n_long, table_slots, nullptr).total;
}

int naruto_subdivide_mark(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const void* vertices, int vertices_f64, double max_edge, uint8_t* flags, void* stream) {
    if (n_faces > kReconMaxCount || n_vertices > kReconMaxCount) return fail(NARUTO_ERR_INVALID, "subdivide_mark: counts beyond int32");
    if (!(max_edge > 0.0) || !std::isfinite(max_edge)) return fail(NARUTO_ERR_INVALID, "subdivide_mark: max_edge must be finite and > 0");
    if (n_faces == 0) return NARUTO_OK;
    if (faces == nullptr || vertices == nullptr || flags == nullptr) return fail(NARUTO_ERR_INVALID, "subdivide_mark: NULL argument");
    const uint32_t nf = (uint32_t)n_faces, nv = (uint32_t)n_vertices;
    const dim3 grid((nf + kSubdivThreads - 1u) / kSubdivThreads), block(kSubdivThreads);
    if (vertices_f64) {
        hipLaunchKernelGGL(k_subdiv_mark<double>, grid, block, 0, (hipStream_t)stream, nf, nv, faces, reinterpret_cast<const double*>(vertices), max_edge * max_edge, flags);
    } else {
        const float me = (float)max_edge;                     // converted once; the square is a float32 product
        hipLaunchKernelGGL(k_subdiv_mark<float>, grid, block, 0, (hipStream_t)stream, nf, nv, faces, reinterpret_cast<const float*>(vertices), me * me, flags);
    }
    return check_launch("subdiv_mark");
}

int naruto_subdivide_edges(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* flags, const int32_t* rank, uint64_t n_long, uint64_t table_slots,
                           void* workspace, uint8_t* own, void* stream) {
    if (n_faces == 0 || n_faces > kReconMaxCount || n_vertices == 0 || n_vertices > kReconMaxCount || n_long > n_faces) return fail(NARUTO_ERR_INVALID, "subdivide_edges: counts out of range");
    if (!subdiv_sizes_ok(n_long, table_slots))
        return fail(NARUTO_ERR_INVALID, "subdivide_edges: 1 .. (2^31-1)/3 long faces and a table of 6 n_long .. 2^31 cells (got %llu, %llu)", (unsigned long long)n_long, (unsigned long long)table_slots);
    if (faces == nullptr || flags == nullptr || rank == nullptr || workspace == nullptr || own == nullptr) return fail(NARUTO_ERR_INVALID, "subdivide_edges: NULL argument");
    const SubdivWs w = subdiv_ws(n_long, table_slots, workspace);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nf = (uint32_t)n_faces, n_slots = (uint32_t)(3u * n_long), ts = (uint32_t)table_slots;           // (2^31 cells: the kernels take the count as uint32)
    if (hipMemsetAsync(w.err, 0, 4u, st) != hipSuccess) return check_launch("subdivide_edges: memset");
    // keys, ordinals and cells are contiguous up to the carve's padding: 0xFF bytes are the empty key, the largest ordinal and "no cell"
    if (hipMemsetAsync(w.keys, 0xFF, (size_t)(reinterpret_cast<char*>(w.pos) - reinterpret_cast<char*>(w.keys)) + (size_t)n_slots * 4u, st) != hipSuccess)
        return check_launch("subdivide_edges: fill");
    hipLaunchKernelGGL(k_subdiv_insert, dim3((nf + kSubdivThreads - 1u) / kSubdivThreads), dim3(kSubdivThreads), 0, st, nf, (uint32_t)n_vertices, faces, flags, rank, (uint32_t)n_long, ts,
                       w.keys, w.ord, w.pos, w.err);
    if (int rc = check_launch("subdiv_insert")) return rc;
    hipLaunchKernelGGL(k_subdiv_own, dim3((n_slots + kSubdivThreads - 1u) / kSubdivThreads), dim3(kSubdivThreads), 0, st, n_slots, ts, w.pos, w.ord, own);
    return check_launch("subdiv_own");
}

int naruto_subdivide_emit(uint64_t n_faces, uint64_t n_vertices, const int32_t* faces, const uint8_t* flags, const int32_t* rank, uint64_t n_long, uint64_t table_slots,
                          void* workspace, const int32_t* mid_rank, uint64_t n_mid, void* vertices, int vertices_f64, uint8_t* colors, int32_t* out_faces, void* stream) {
    if (n_faces == 0 || n_faces > kReconMaxCount || n_vertices == 0 || n_long > n_faces || n_mid == 0 || n_mid > 3u * n_long || n_vertices + n_mid > kReconMaxCount ||
        n_faces + 3u * n_long > kReconMaxCount)
        return fail(NARUTO_ERR_INVALID, "subdivide_emit: counts out of range");
    if (!subdiv_sizes_ok(n_long, table_slots)) return fail(NARUTO_ERR_INVALID, "subdivide_emit: 1 .. (2^31-1)/3 long faces and a table of 6 n_long .. 2^31 cells");
    if (faces == nullptr || flags == nullptr || rank == nullptr || workspace == nullptr || mid_rank == nullptr || vertices == nullptr || out_faces == nullptr)
        return fail(NARUTO_ERR_INVALID, "subdivide_emit: NULL argument");
    const SubdivWs w = subdiv_ws(n_long, table_slots, workspace);
    const uint32_t nf = (uint32_t)n_faces, nv = (uint32_t)n_vertices, nl = (uint32_t)n_long, ts = (uint32_t)table_slots, nm = (uint32_t)n_mid;
    const dim3 grid((nf + kSubdivThreads - 1u) / kSubdivThreads), block(kSubdivThreads);
    uint32_t* col = reinterpret_cast<uint32_t*>(colors);
    if (vertices_f64)
        hipLaunchKernelGGL(k_subdiv_emit<double>, grid, block, 0, (hipStream_t)stream, nf, nv, faces, flags, rank, nl, ts, w.pos, w.ord, mid_rank, nm, reinterpret_cast<double*>(vertices), col,
                           out_faces, w.err);
    else
        hipLaunchKernelGGL(k_subdiv_emit<float>, grid, block, 0, (hipStream_t)stream, nf, nv, faces, flags, rank, nl, ts, w.pos, w.ord, mid_rank, nm, reinterpret_cast<float*>(vertices), col,
                           out_faces, w.err);
    return check_launch("subdiv_emit");
}

// ---- mesh simulator (naruto_sim.hip) --------------------------------------------------------------------------------------
namespace {
int sim_fill2(uint64_t n_pairs, uint32_t w0, uint32_t w1, void* p, hipStream_t st, const char* who) {
    hipLaunchKernelGGL(k_sim_fill2, dim3((uint32_t)((n_pairs + kSimThreads - 1u) / kSimThreads)), dim3(kSimThreads), 0, st, n_pairs, w0, w1, reinterpret_cast<uint2*>(p));
    return check_launch(who);
}
}  // namespace

size_t naruto_render_rgbd_workspace(uint64_t n_vertices, uint64_t n_faces, uint32_t n_poses, uint32_t H, uint32_t W) {
    if (naruto_render_depth_workspace(n_vertices, n_faces, n_poses) == 0 || H == 0 || W == 0 || (uint64_t)H * W > (1ull << 30)) return 0;
    return cull_ws(n_vertices, n_faces, n_poses, nullptr, H, W).total;
}

namespace {
// the texel words of one texture's chain, level 0 included; 0: a side outside 1 .. 16384
uint64_t tex_chain_words(uint32_t w, uint32_t h, uint32_t* n_levels) {
    if (w == 0 || h == 0 || w > kSimTexMaxSide || h > kSimTexMaxSide) return 0;
    uint64_t words = 0;
    uint32_t levels = 0;
    for (;;) {
        words += (uint64_t)w * h;
        ++levels;
        if (w == 1u && h == 1u) break;
        w = std::max(1u, w >> 1); h = std::max(1u, h >> 1);
    }
    if (n_levels != nullptr) *n_levels = levels;                 // = 1 + floor(log2(max(W, H)))
    return words;
}
}  // namespace

size_t naruto_tex_bytes(uint32_t W, uint32_t H) { return (size_t)(tex_chain_words(W, H, nullptr) * 4u); }

int naruto_tex_build(uint32_t W, uint32_t H, uint64_t offset, const void* level0, uint32_t* desc, uint32_t* texels, void* stream) {
    if (level0 == nullptr || desc == nullptr || texels == nullptr) return fail(NARUTO_ERR_INVALID, "tex_build: NULL argument");
    uint32_t levels = 0;
    const uint64_t words = tex_chain_words(W, H, &levels);
    if (words == 0 || offset + words >= (1ull << 32))
        return fail(NARUTO_ERR_INVALID, "tex_build: a texture of %u x %u at word %llu (sides 1 .. 16384, all chains within 2^32 words)", W, H, (unsigned long long)offset);
    hipStream_t st = (hipStream_t)stream;
    // level 0 from wherever it lies, then the chain on the stream; the call returns when all is done, so the source may be freed
    if (hipMemcpyAsync(texels + offset, level0, (size_t)W * H * 4u, hipMemcpyDefault, st) != hipSuccess) return check_launch("tex_build: upload");
    uint32_t w = W, h = H;
    uint64_t at = offset;
    for (uint32_t l = 1; l < levels; ++l) {
        const uint32_t wd = std::max(1u, w >> 1), hd = std::max(1u, h >> 1);
        hipLaunchKernelGGL(k_tex_down, dim3((wd * hd + kSimThreads - 1u) / kSimThreads), dim3(kSimThreads), 0, st, w, h, wd, hd, texels + at, texels + at + (uint64_t)w * h);
        if (int rc = check_launch("tex_down")) return rc;
        at += (uint64_t)w * h;
        w = wd; h = hd;
    }
    const uint32_t d[4] = {(uint32_t)offset, W, H, levels};
    if (hipMemcpyAsync(desc, d, sizeof(d), hipMemcpyHostToDevice, st) != hipSuccess) return check_launch("tex_build: descriptor");
    if (hipStreamSynchronize(st) != hipSuccess) return check_launch("tex_build: synchronise");
    return NARUTO_OK;
}

namespace {
int sim_render(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
               uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
               const NarutoSimTextures* tex, void* stream);
}  // namespace

int naruto_render_rgbd(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
                       uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
                       void* stream) {
    return sim_render(cam, n_vertices, vertices, n_faces, faces, colors, colors_f32, n_poses, poses, large_threshold, flags, workspace, depth, color, face_id,
                      nullptr, stream);
}

int naruto_render_rgbd_tex(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
                           uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
                           const NarutoSimTextures* tex, void* stream) {
    if (tex == nullptr) return fail(NARUTO_ERR_INVALID, "render_rgbd_tex: NULL textures");
    if (tex->struct_size < sizeof(NarutoSimTextures))
        return fail(NARUTO_ERR_INVALID, "render_rgbd_tex: NarutoSimTextures of %u bytes, this library reads %zu", tex->struct_size, sizeof(NarutoSimTextures));
    if (tex->uv == nullptr || tex->face_material == nullptr || (tex->n_materials != 0 && tex->materials == nullptr) ||
        (tex->n_textures != 0 && (tex->tex_desc == nullptr || tex->texels == nullptr)))
        return fail(NARUTO_ERR_INVALID, "render_rgbd_tex: NULL uv, face materials, material table, descriptors or texels");
    if (tex->n_texels >= (1ull << 32)) return fail(NARUTO_ERR_INVALID, "render_rgbd_tex: 2^32 texels or more");
    return sim_render(cam, n_vertices, vertices, n_faces, faces, colors, colors_f32, n_poses, poses, large_threshold, flags, workspace, depth, color, face_id,
                      tex, stream);
}

namespace {
int sim_render(const NarutoCullCam* cam, uint64_t n_vertices, const float* vertices, uint64_t n_faces, const int32_t* faces, const void* colors, int colors_f32,
               uint32_t n_poses, const float* poses, uint32_t large_threshold, uint32_t flags, void* workspace, float* depth, float* color, int32_t* face_id,
               const NarutoSimTextures* tex, void* stream) {
    if (int rc = cull_cam_check(cam, "render_rgbd")) return rc;
    if (!(cam->near_ > 0.0f) || !(cam->near_ < cam->far_)) return fail(NARUTO_ERR_INVALID, "render_rgbd: need 0 < near < far");
    if (int rc = cull_raster_sizes_check(cam, n_vertices, n_faces, n_poses, "render_rgbd")) return rc;
    if ((uint64_t)n_poses * cam->H * cam->W >= (1ull << 32)) return fail(NARUTO_ERR_INVALID, "render_rgbd: poses x pixels per call must stay below 2^32: use fewer poses per call");
    if (flags & ~(uint32_t)NARUTO_SIM_KEEP_INF) return fail(NARUTO_ERR_INVALID, "render_rgbd: unknown flag");
    if (vertices == nullptr || faces == nullptr || poses == nullptr || workspace == nullptr) return fail(NARUTO_ERR_INVALID, "render_rgbd: NULL argument");
    if (depth == nullptr && color == nullptr && face_id == nullptr) return fail(NARUTO_ERR_INVALID, "render_rgbd: no output");
    if (color != nullptr && colors == nullptr) return fail(NARUTO_ERR_INVALID, "render_rgbd: a colour image needs vertex colours");
    const CullCam c = cull_cam_args(cam);
    const CullWs w = cull_ws(n_vertices, n_faces, n_poses, workspace, cam->H, cam->W);
    unsigned long long* cells = w.cells;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nv = (uint32_t)n_vertices, nf = (uint32_t)n_faces, cap = (uint32_t)(n_faces * n_poses), n_px = cam->H * cam->W;
    if (hipMemsetAsync(w.counter, 0, 8u, st) != hipSuccess) return check_launch("render_rgbd: memset");
    if (int rc = sim_fill2((uint64_t)n_poses * n_px, kSimNoFace, kCullInfBits, cells, st, "render_rgbd: fill")) return rc;
    const dim3 block(kCullThreads);
    hipLaunchKernelGGL(k_cull_transform, dim3((nv + kCullThreads - 1u) / kCullThreads, n_poses), block, 0, st, nv, vertices, poses, w.camv);
    if (int rc = check_launch("cull_transform")) return rc;
    hipLaunchKernelGGL(k_cull_raster_small<unsigned long long>, dim3((nf + kCullThreads - 1u) / kCullThreads, n_poses), block, 0, st, c, nf, nv, faces,
                       (const uint8_t*)nullptr, w.camv, large_threshold, cells, w.counter, w.ent_id, w.ent_start, cap);
    if (int rc = check_launch("sim_raster_small")) return rc;
    hipLaunchKernelGGL(k_cull_raster_large<unsigned long long>, dim3(kCullLargeGrid), block, 0, st, c, nf, nv, faces, w.camv, cells, w.counter, w.ent_id, w.ent_start, cap);
    if (int rc = check_launch("sim_raster_large")) return rc;
    const dim3 shade_grid((n_px + kSimThreads - 1u) / kSimThreads, n_poses);
    if (tex == nullptr) {
        hipLaunchKernelGGL(k_sim_shade, shade_grid, dim3(kSimThreads), 0, st, c, nf, nv, faces, colors, colors_f32, w.camv, cells, (int)(flags & NARUTO_SIM_KEEP_INF), depth, color,
                           face_id);
        return check_launch("sim_shade");
    }
    const SimTex t{tex->n_materials, tex->n_textures, (unsigned long long)tex->n_texels, tex->uv, tex->face_material, tex->materials, tex->tex_desc, tex->texels};
    hipLaunchKernelGGL(k_sim_shade_tex, shade_grid, dim3(kSimThreads), 0, st, c, nf, nv, faces, colors, colors_f32, w.camv, cells, (int)(flags & NARUTO_SIM_KEEP_INF), t, depth,
                       color, face_id);
    return check_launch("sim_shade_tex");
}
}  // namespace

int naruto_cube_to_erp(uint32_t n_channels, uint32_t face_w, uint64_t n_erp, const int32_t* table, const void* cube, void* erp, void* stream) {
    if (n_channels == 0 || n_erp == 0) return NARUTO_OK;
    if (face_w == 0 || face_w > 8192u || n_erp > (1ull << 30) || n_channels > 65535u) return fail(NARUTO_ERR_INVALID, "cube_to_erp: sizes out of range");
    if (table == nullptr || cube == nullptr || erp == nullptr) return fail(NARUTO_ERR_INVALID, "cube_to_erp: NULL argument");
    hipLaunchKernelGGL(k_sim_gather, dim3((uint32_t)((n_erp + kSimThreads - 1u) / kSimThreads), n_channels), dim3(kSimThreads), 0, (hipStream_t)stream, 6u * face_w * face_w,
                       (uint32_t)n_erp, table, reinterpret_cast<const uint32_t*>(cube), reinterpret_cast<uint32_t*>(erp));
    return check_launch("sim_gather");
}

int naruto_depth_to_dist(uint32_t n_images, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy, const float* depth, float* dist, void* stream) {
    if (n_images == 0) return NARUTO_OK;
    if (H == 0 || W == 0 || (uint64_t)H * W > (1ull << 30) || n_images > 65535u) return fail(NARUTO_ERR_INVALID, "depth_to_dist: sizes out of range");
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0f || fy == 0.0f || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(NARUTO_ERR_INVALID, "depth_to_dist: intrinsics must be finite with fx, fy != 0");
    if (depth == nullptr || dist == nullptr) return fail(NARUTO_ERR_INVALID, "depth_to_dist: NULL argument");
    hipLaunchKernelGGL(k_sim_dist, dim3((H * W + kSimThreads - 1u) / kSimThreads, n_images), dim3(kSimThreads), 0, (hipStream_t)stream, H, W, fx, fy, cx, cy, depth, dist);
    return check_launch("sim_dist");
}

int naruto_sim_erp(uint32_t n_panoramas, uint32_t face_w, uint64_t n_erp, const int32_t* table, const float* cube_depth, const float* cube_color, float invalid_thre,
                   float* erp_dist, float* erp_color, uint32_t* stats, void* stream) {
    if (n_panoramas == 0 || n_erp == 0) return NARUTO_OK;
    if (face_w < 2 || face_w > 8192u || n_erp > (1ull << 30) || n_panoramas > 65535u) return fail(NARUTO_ERR_INVALID, "sim_erp: sizes out of range (face_w 2 .. 8192)");
    if (std::isnan(invalid_thre)) return fail(NARUTO_ERR_INVALID, "sim_erp: the threshold is not a number");
    if (table == nullptr || cube_depth == nullptr || (erp_color != nullptr && cube_color == nullptr)) return fail(NARUTO_ERR_INVALID, "sim_erp: NULL argument");
    if (erp_dist == nullptr && erp_color == nullptr && stats == nullptr) return fail(NARUTO_ERR_INVALID, "sim_erp: no output");
    hipStream_t st = (hipStream_t)stream;
    if (stats != nullptr)
        if (int rc = sim_fill2(n_panoramas, kCullInfBits, 0u, stats, st, "sim_erp: fill")) return rc;
    hipLaunchKernelGGL(k_sim_erp, dim3((uint32_t)((n_erp + kSimThreads - 1u) / kSimThreads), n_panoramas), dim3(kSimThreads), 0, st, face_w, (uint32_t)n_erp, table, cube_depth,
                       cube_color, invalid_thre, erp_dist, erp_color, stats);
    return check_launch("sim_erp");
}

int naruto_debug_atomic_min64_rate(uint64_t n_cells, uint32_t n_lanes, uint32_t iters, uint64_t* buf, void* stream) {
    if (n_cells == 0 || n_cells > 0xFFFFFFFFull || n_lanes == 0 || iters == 0 || iters > (1u << 20)) return fail(NARUTO_ERR_INVALID, "debug_atomic_min64_rate: sizes out of range");
    if (buf == nullptr) return fail(NARUTO_ERR_INVALID, "debug_atomic_min64_rate: NULL argument");
    hipLaunchKernelGGL(k_sim_atomic_probe, dim3((n_lanes + kSimThreads - 1u) / kSimThreads), dim3(kSimThreads), 0, (hipStream_t)stream, (uint32_t)n_cells, iters,
                       reinterpret_cast<unsigned long long*>(buf));
    return check_launch("sim_atomic_probe");
}

int naruto_sample_distinct(uint64_t n, uint32_t count, uint64_t seed, uint64_t counter, int64_t* out, void* stream) {
    if (out == nullptr) return fail(NARUTO_ERR_INVALID, "sample_distinct: NULL output");
    if (count == 0) return NARUTO_OK;
    if (n == 0 || count > n) return fail(NARUTO_ERR_INVALID, "sample_distinct: cannot draw %u distinct indices out of %llu", count, (unsigned long long)n);
    hipLaunchKernelGGL(k_sample_distinct, dim3((count + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, count, (uint64_t)0, half_bits_for(n),
                       mix_key(seed, counter, 1), out);
    return check_launch("sample_distinct");
}

int naruto_frame_ingest(uint64_t n_pixels, const float* direction, const float* rgb, const float* depth, float depth_trunc, float* rays,
                        uint64_t* n_valid, void* stream) {
    if (direction == nullptr || rgb == nullptr || depth == nullptr || rays == nullptr || n_valid == nullptr) return fail(NARUTO_ERR_INVALID, "frame_ingest: NULL argument");
    if (n_pixels == 0 || n_pixels > (1ull << 32)) return fail(NARUTO_ERR_INVALID, "frame_ingest: %llu pixels out of range", (unsigned long long)n_pixels);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_valid, 0, 8u, st) != hipSuccess) return check_launch("frame_ingest: memset");
    const uint64_t n_words = n_pixels * 7u;
    // at most 8 workgroups per CU's worth of grid: beyond that the grid-stride loop takes over (one atomic per workgroup)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_words + kFrameThreads - 1u) / kFrameThreads, 256u * 8u);
    hipLaunchKernelGGL(k_frame_ingest, dim3(blocks), dim3(kFrameThreads), 0, st, n_words, reinterpret_cast<const uint32_t*>(direction),
                       reinterpret_cast<const uint32_t*>(rgb), reinterpret_cast<const uint32_t*>(depth), depth_trunc, reinterpret_cast<uint32_t*>(rays),
                       reinterpret_cast<unsigned long long*>(n_valid));
    return check_launch("frame_ingest");
}

int naruto_keyframe_row(const float* frame_rays, uint64_t n_pixels, const uint64_t* n_valid, uint32_t rays_per_kf, uint64_t seed, uint64_t counter,
                        float* row, void* stream) {
    if (frame_rays == nullptr || row == nullptr) return fail(NARUTO_ERR_INVALID, "keyframe_row: NULL argument");
    if (n_pixels == 0 || n_pixels > (1ull << 32) || rays_per_kf == 0) return fail(NARUTO_ERR_INVALID, "keyframe_row: sizes out of range");
    hipLaunchKernelGGL(k_keyframe_row, dim3((rays_per_kf + kFrameThreads - 1u) / kFrameThreads), dim3(kFrameThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(frame_rays), n_pixels, reinterpret_cast<const unsigned long long*>(n_valid), rays_per_kf,
                       mix_key(seed, counter, 1), reinterpret_cast<uint32_t*>(row));
    return check_launch("keyframe_row");
}

int naruto_pose_log(uint32_t P, const float* c2w, float* pose6, void* stream) {
    if (c2w == nullptr || pose6 == nullptr) return fail(NARUTO_ERR_INVALID, "pose_log: NULL argument");
    if (P == 0) return fail(NARUTO_ERR_INVALID, "pose_log: no pose");
    hipLaunchKernelGGL(k_pose_log, dim3((P + kPoseChainThreads - 1u) / kPoseChainThreads), dim3(kPoseChainThreads), 0, (hipStream_t)stream, P, c2w, pose6);
    return check_launch("pose_log");
}

int naruto_pose_predict(float* est, uint32_t num_frames, uint32_t i, int32_t const_speed, float* pose6_out, void* stream) {
    if (est == nullptr || pose6_out == nullptr) return fail(NARUTO_ERR_INVALID, "pose_predict: NULL argument");
    if (i < 1u || i >= num_frames) return fail(NARUTO_ERR_INVALID, "pose_predict: frame %u of %u (the first frame is given, not predicted)", i, num_frames);
    hipLaunchKernelGGL(k_pose_predict, dim3(1), dim3(kPoseChainThreads), 0, (hipStream_t)stream, est, i, const_speed, pose6_out);
    return check_launch("pose_predict");
}

int naruto_pose_commit(float* est, float* rel, uint32_t num_frames, uint32_t i, uint32_t keyframe_every, const float* c2w, void* stream) {
    if (est == nullptr || rel == nullptr || c2w == nullptr) return fail(NARUTO_ERR_INVALID, "pose_commit: NULL argument");
    if (keyframe_every == 0u) return fail(NARUTO_ERR_INVALID, "pose_commit: keyframe_every = 0");
    if (i < 1u || i >= num_frames) return fail(NARUTO_ERR_INVALID, "pose_commit: frame %u of %u (the first frame is given, not tracked)", i, num_frames);
    hipLaunchKernelGGL(k_pose_commit, dim3(1), dim3(kPoseChainThreads), 0, (hipStream_t)stream, est, rel, i, keyframe_every, c2w);
    return check_launch("pose_commit");
}

int naruto_pose_scatter(float* est, uint32_t num_frames, const float* refined, uint32_t P, uint32_t keyframe_every, uint32_t cur_id, int32_t optim_cur,
                        void* stream) {
    if (est == nullptr || refined == nullptr) return fail(NARUTO_ERR_INVALID, "pose_scatter: NULL argument");
    if (P == 0u || keyframe_every == 0u) return fail(NARUTO_ERR_INVALID, "pose_scatter: P = %u poses, keyframe_every = %u", P, keyframe_every);
    if (cur_id >= num_frames) return fail(NARUTO_ERR_INVALID, "pose_scatter: current frame %u of %u", cur_id, num_frames);
    if (P > 2u && (uint64_t)(P - 2u) * keyframe_every >= (uint64_t)num_frames)
        return fail(NARUTO_ERR_INVALID, "pose_scatter: keyframe %u at frame %llu of %u", P - 2u, (unsigned long long)(P - 2u) * keyframe_every, num_frames);
    hipLaunchKernelGGL(k_pose_scatter, dim3((P + kPoseChainThreads - 1u) / kPoseChainThreads), dim3(kPoseChainThreads), 0, (hipStream_t)stream, est, refined, P,
                       keyframe_every, cur_id, optim_cur);
    return check_launch("pose_scatter");
}

int naruto_pose_resolve(const float* est, const float* rel, uint32_t n, uint32_t keyframe_every, float* out, void* stream) {
    if (est == nullptr || rel == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "pose_resolve: NULL argument");
    if (n == 0u || keyframe_every == 0u) return fail(NARUTO_ERR_INVALID, "pose_resolve: n = %u frames, keyframe_every = %u", n, keyframe_every);
    hipLaunchKernelGGL(k_pose_resolve, dim3((n + kPoseChainThreads - 1u) / kPoseChainThreads), dim3(kPoseChainThreads), 0, (hipStream_t)stream, est, rel, n,
                       keyframe_every, out);
    return check_launch("pose_resolve");
}

namespace {
// NarutoRayBatch -> the kernels' argument block (need_out: the batch's own output buffers are written)
int assemble_args(const NarutoRayBatch* b, bool need_out, AssembleArgs& a, const char* who) {
    if (b == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL argument", who);
    if (b->poses == nullptr || b->n_poses == 0 || (need_out && (b->rays_o == nullptr || b->rays_d == nullptr || b->target_s == nullptr || b->target_d == nullptr)))
        return fail(NARUTO_ERR_INVALID, "%s: NULL pose / output buffer", who);
    if (b->n_global > 0 && (b->store == nullptr || b->frame_ids == nullptr || b->rays_per_kf == 0 || b->n_kf == 0 || b->keyframe_every <= 0))
        return fail(NARUTO_ERR_INVALID, "%s: the keyframe store is incomplete", who);
    const uint64_t n_pop = (uint64_t)b->n_kf * b->rays_per_kf;
    if (b->n_global > n_pop) return fail(NARUTO_ERR_INVALID, "%s: %u distinct rays out of %llu stored", who, b->n_global, (unsigned long long)n_pop);
    if (b->n_cur > 0 && (b->current == nullptr || b->n_cur_pop == 0 || b->n_cur > b->n_cur_pop))
        return fail(NARUTO_ERR_INVALID, "%s: %u distinct current-frame rays out of %llu", who, b->n_cur, (unsigned long long)b->n_cur_pop);
    a = AssembleArgs{};
    a.store = b->store; a.n_pop = n_pop ? n_pop : 1; a.rays_per_kf = b->rays_per_kf ? b->rays_per_kf : 1; a.frame_ids = b->frame_ids;
    a.keyframe_every = b->keyframe_every; a.n_global = b->n_global;
    a.current = b->current; a.cur_list = b->cur_list; a.n_cur_pop = b->n_cur_pop ? b->n_cur_pop : 1; a.n_cur = b->n_cur;
    a.poses = b->poses; a.n_poses = b->n_poses;
    a.key_global = mix_key(b->seed, b->counter, 2); a.key_cur = mix_key(b->seed, b->counter, 3);
    a.hb_global = half_bits_for(a.n_pop); a.hb_cur = half_bits_for(a.n_cur_pop);
    a.rays_o = b->rays_o; a.rays_d = b->rays_d; a.target_s = b->target_s; a.target_d = b->target_d; a.ids_out = b->ids_out;
    a.rng = b->rng; a.dyn = b->dyn; a.seed_host = b->seed; a.counter_host = b->counter;
    if (b->keys_out != nullptr) {
        const uint32_t n = b->n_global + b->n_cur;
        if (b->key_vol == nullptr || b->key_dims[0] == 0 || b->key_dims[1] == 0 || b->key_dims[2] == 0 || (uint64_t)b->key_base + b->key_tail > n)
            return fail(NARUTO_ERR_INVALID, "%s: keys_out needs key_vol, key_dims and key_base + key_tail <= rows", who);
        a.keys_out = b->keys_out; a.key_base = b->key_base; a.key_end = n - b->key_tail;
        a.kv = ArsVol{b->key_vol, (int)b->key_dims[0], (int)b->key_dims[1], (int)b->key_dims[2], b->key_bbox_min[0], b->key_bbox_min[1], b->key_bbox_min[2],
                      b->key_voxel_scale};
    }
    return NARUTO_OK;
}
}  // namespace

int naruto_assemble_rays(const NarutoRayBatch* b, void* stream) {
    AssembleArgs a{};
    if (int rc = assemble_args(b, true, a, "assemble_rays")) return rc;
    const uint32_t n = b->n_global + b->n_cur;
    if (n == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_assemble_rays, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("assemble_rays");
}

// N2 + N1 in one launch (round 5): the oversampled batch of naruto_assemble_rays is never written -- k_ars_fused<true> draws and rotates a
// row where it needs one.  Same rows, same selection as naruto_assemble_rays | naruto_active_ray_select (the batch's own output buffers
// and ids_out are not used).  Up to 8 192 candidates (n_global + n_cur - base - n_tail); beyond: NARUTO_ERR_INVALID, use the two calls.
int naruto_assemble_select(const NarutoRayBatch* b, uint32_t base, uint32_t K, uint32_t n_tail, const float* uncert_vol, const uint32_t* vol_dims,
                           const float* bbox_min, float voxel_scale, float* out_o, float* out_d, float* out_s, float* out_t, void* stream) {
    AssembleArgs s{};
    if (int rc = assemble_args(b, false, s, "assemble_select")) return rc;
    if (uncert_vol == nullptr || vol_dims == nullptr || bbox_min == nullptr || out_o == nullptr || out_d == nullptr || out_s == nullptr || out_t == nullptr)
        return fail(NARUTO_ERR_INVALID, "assemble_select: NULL argument");
    const uint32_t n_total = b->n_global + b->n_cur;
    if (n_tail == 0 || K == 0 || K > base || (uint64_t)base + n_tail >= n_total)
        return fail(NARUTO_ERR_INVALID, "assemble_select: need 0 < K <= base, n_tail > 0, base + n_tail < n_total");
    const uint32_t n_cand = n_total - n_tail - base;
    if (n_cand <= K) return fail(NARUTO_ERR_INVALID, "assemble_select: %u candidates for K = %u (numpy argpartition needs K < n)", n_cand, K);
    if (n_cand > kArsFusedMax) return fail(NARUTO_ERR_INVALID, "assemble_select: %u candidates (the one-launch form takes up to %u)", n_cand, kArsFusedMax);
    ArsArgs a{};
    a.n_total = n_total; a.base = base; a.K = K; a.n_tail = n_tail; a.n_cand = n_cand;
    a.vol = uncert_vol;
    a.X = (int)vol_dims[0]; a.Y = (int)vol_dims[1]; a.Z = (int)vol_dims[2];
    a.bx = bbox_min[0]; a.by = bbox_min[1]; a.bz = bbox_min[2]; a.voxel_scale = voxel_scale;
    a.o_out = out_o; a.d_out = out_d; a.s_out = out_s; a.t_out = out_t;
    const uint32_t n_copy = base + n_tail - K;
    hipLaunchKernelGGL(k_ars_fused<true>, dim3(1u + (n_copy + kArsFusedThreads - 1u) / kArsFusedThreads), dim3(kArsFusedThreads), 0, (hipStream_t)stream, a, s);
    return check_launch("assemble_select");
}

uint64_t naruto_perm_index(uint64_t i, uint64_t n, uint64_t seed, uint64_t counter, uint64_t salt) {
    return n ? perm_index(i, n, half_bits_for(n), mix_key(seed, counter, salt)) : 0;
}

int naruto_map_volumes(uint32_t M, const float* sdf_uncert, float* out, void* stream) {
    if (sdf_uncert == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "map_volumes: NULL argument");
    if (M == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_map_post, dim3((M + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, M, reinterpret_cast<const float2*>(sdf_uncert), out);
    return check_launch("map_volumes");
}

int naruto_adam_multi(const NarutoAdamSeg* segs, uint32_t n_segs, float beta1, float beta2, uint32_t step, int32_t* step_dev, uint32_t flags, void* stream) {
    if (segs == nullptr || n_segs == 0 || n_segs > (uint32_t)kAdamMaxSegs) return fail(NARUTO_ERR_INVALID, "adam_multi: 1..%d segments", kAdamMaxSegs);
    if ((flags & NARUTO_ADAM_ADVANCE) && step_dev == nullptr) return fail(NARUTO_ERR_INVALID, "adam_multi: NARUTO_ADAM_ADVANCE needs step_dev");
    if (step == 0 && step_dev == nullptr) return fail(NARUTO_ERR_INVALID, "adam_multi: step is 1-based (or pass step_dev)");
    AdamSegs a{};
    a.n_segs = n_segs;
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < n_segs; ++k) {
        if (segs[k].param == nullptr || segs[k].grad == nullptr || segs[k].exp_avg == nullptr || segs[k].exp_avg_sq == nullptr)
            return fail(NARUTO_ERR_INVALID, "adam_multi: NULL pointer in segment %u", k);
        a.p[k] = segs[k].param; a.g[k] = segs[k].grad; a.m[k] = segs[k].exp_avg; a.v[k] = segs[k].exp_avg_sq;
        a.n[k] = segs[k].n; a.lr[k] = segs[k].lr; a.eps[k] = segs[k].eps; a.wd[k] = segs[k].weight_decay; a.lag[k] = segs[k].step_lag;
        a.block_begin[k] = blocks;
        uint64_t nb = (segs[k].n + 1023u) / 1024u;          // >= 4 elements per thread, grid-stride beyond 1024 workgroups
        if (nb < 1) nb = 1;
        if (nb > 1024u) nb = 1024u;
        blocks += (uint32_t)nb;
    }
    for (uint32_t k = n_segs; k <= (uint32_t)kAdamMaxSegs; ++k) a.block_begin[k] = blocks;
    hipLaunchKernelGGL(k_adam_multi, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, beta1, beta2, step_dev, step, flags);
    return check_launch("adam_multi");
}

// ---- hardware layout probes (tests/test_gpu_parity.py: test_mfma_layout, test_mfma_bf16_layout, test_permlane32_swap) ---------------------------------------
__global__ void k_debug_mfma(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
    const int lane = threadIdx.x;
    f32x16 c = zero16();
    c = mfma32(a[lane], b[lane], c);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[lane * 16 + r] = c[r];
}

__global__ void k_debug_swap(const float* __restrict__ v0, const float* __restrict__ v1, float* __restrict__ out) {
    const int lane = threadIdx.x;
    float a = v0[lane], b = v1[lane];
    swap32(a, b);
    out[lane] = a;
    out[64 + lane] = b;
}

__global__ void k_debug_mfma_bf16(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
    const int lane = threadIdx.x, i = lane & 31, hh = lane >> 5;
    float av[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        av[e] = a[i * 16 + 8 * hh + e];                 // A[i][k = 8 hh + e]
        bv[e] = b[(8 * hh + e) * 32 + i];               // B[k = 8 hh + e][j = i]
    }
    f32x16 c = zero16();
    c = mfma16(pack8(av), pack8(bv), c);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[lane * 16 + r] = c[r];
}

int naruto_debug_random_lines(const float* table, uint64_t table_bytes, uint32_t iters, float* sink, uint64_t* n_lines_out, void* stream) {
    if (table == nullptr || sink == nullptr || table_bytes < 64 || iters == 0) return fail(NARUTO_ERR_INVALID, "debug_random_lines: bad argument");
    const uint32_t blocks = 256u * 8u;
    hipLaunchKernelGGL(k_debug_random_lines, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(table), (uint32_t)(table_bytes / 64u), iters, sink);
    if (n_lines_out != nullptr) *n_lines_out = (uint64_t)blocks * 4u * iters * 8u * 32u;         // waves x iterations x loads x distinct lines per load
    return check_launch("debug_random_lines");
}

int naruto_debug_mfma_bf16_layout(const float* a, const float* b, float* out, void* stream) {
    if (a == nullptr || b == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_mfma_bf16_layout: NULL argument");
    hipLaunchKernelGGL(k_debug_mfma_bf16, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, out);
    return check_launch("debug_mfma_bf16_layout");
}

int naruto_debug_mfma_layout(const float* a, const float* b, float* out, void* stream) {
    if (a == nullptr || b == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_mfma_layout: NULL argument");
    hipLaunchKernelGGL(k_debug_mfma, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, out);
    return check_launch("debug_mfma_layout");
}

int naruto_debug_permlane_swap(const float* v0, const float* v1, float* out, void* stream) {
    if (v0 == nullptr || v1 == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_permlane_swap: NULL argument");
    hipLaunchKernelGGL(k_debug_swap, dim3(1), dim3(64), 0, (hipStream_t)stream, v0, v1, out);
    return check_launch("debug_permlane_swap");
}

// ------------------------------------------------------------------------------------------------
// Camera tracking (see naruto_track.hip)
// ------------------------------------------------------------------------------------------------
namespace {
int track_check(const NarutoTrackStep* k, const NarutoTrainStep* t, bool frame, const char* who) {
    if (k == nullptr || t == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL argument", who);
    if (k->n_rays == 0 || k->n_rays != t->n_rays)
        return fail(NARUTO_ERR_INVALID, "%s: NarutoTrackStep.n_rays (%u) must be the training step's n_rays (%u), not 0", who, k->n_rays, t->n_rays);
    if (t->rays_o == nullptr || t->rays_d == nullptr || t->target_rgb == nullptr || t->target_d == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL ray / target buffer in NarutoTrainStep", who);
    if (k->rng == nullptr || k->d_cam == nullptr || k->pose_init == nullptr || k->pose == nullptr || k->exp_avg == nullptr || k->exp_avg_sq == nullptr ||
        k->state == nullptr || k->best_pose == nullptr || k->best_loss == nullptr || k->c2w == nullptr || k->d_rays_o == nullptr || k->d_rays_d == nullptr ||
        k->workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL buffer in NarutoTrackStep", who);
    const bool any_trace = k->trace_loss != nullptr || k->trace_pose != nullptr || k->trace_d_pose != nullptr || k->max_trace != 0;
    const bool all_trace = k->trace_loss != nullptr && k->trace_pose != nullptr && k->trace_d_pose != nullptr && k->max_trace != 0;
    if (any_trace && !all_trace) return fail(NARUTO_ERR_INVALID, "%s: the trace needs trace_loss, trace_pose, trace_d_pose and max_trace together", who);
    if (!(k->lr_rot >= 0.0f) || !(k->lr_trans >= 0.0f) || !(k->beta1 >= 0.0f && k->beta1 < 1.0f) || !(k->beta2 >= 0.0f && k->beta2 < 1.0f) || !(k->eps >= 0.0f))
        return fail(NARUTO_ERR_INVALID, "%s: Adam needs lr >= 0, 0 <= betas < 1 and eps >= 0", who);
    if (frame) {
        if (k->direction == nullptr || k->rgb == nullptr || k->depth == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL frame", who);
        if (k->H == 0 || k->W == 0 || 2ull * k->edge_h >= k->H || 2ull * k->edge_w >= k->W)
            return fail(NARUTO_ERR_INVALID, "%s: the edges %u / %u leave no interior of a %u x %u frame", who, k->edge_h, k->edge_w, k->H, k->W);
        const uint64_t n_int = (uint64_t)(k->H - 2u * k->edge_h) * (k->W - 2u * k->edge_w);
        if (k->n_rays > n_int) return fail(NARUTO_ERR_INVALID, "%s: %u distinct pixels out of %llu interior pixels", who, k->n_rays, (unsigned long long)n_int);
    }
    return NARUTO_OK;
}

TrackArgs track_args(const NarutoTrackStep* k, const NarutoTrainStep* t) {
    TrackArgs a{};
    a.n_rays = k->n_rays; a.H = k->H; a.W = k->W; a.edge_h = k->edge_h; a.edge_w = k->edge_w;
    a.direction = k->direction; a.rgb = k->rgb; a.depth = k->depth; a.rng = k->rng;
    a.d_cam = k->d_cam; a.pix = k->pix;
    // the training step's ray and target buffers are the tracker's own: written by the draw, the ray launch and the pose step
    a.target_rgb = const_cast<float*>(t->target_rgb); a.target_d = const_cast<float*>(t->target_d);
    a.rays_o = const_cast<float*>(t->rays_o); a.rays_d = const_cast<float*>(t->rays_d);
    a.pose_init = k->pose_init; a.pose = k->pose; a.exp_avg = k->exp_avg; a.exp_avg_sq = k->exp_avg_sq; a.state = k->state;
    a.lr_rot = k->lr_rot; a.lr_trans = k->lr_trans; a.beta1 = k->beta1; a.beta2 = k->beta2; a.eps = k->eps;
    a.wait_iters = k->wait_iters; a.best = k->best;
    a.best_pose = k->best_pose; a.best_loss = k->best_loss; a.c2w = k->c2w;
    a.d_rays_o = k->d_rays_o; a.d_rays_d = k->d_rays_d; a.losses = t->losses;
    a.trace_loss = k->trace_loss; a.trace_pose = k->trace_pose; a.trace_d_pose = k->trace_d_pose; a.max_trace = k->max_trace;
    return a;
}

// The gradient of the iteration's loss with respect to its rays, after the loss backward and the compaction: naruto_query_bwd_points' launches for
// ray points over the active list, written (not accumulated) into d_rays_o / d_rays_d.  The zero fill is a kernel, so that a captured call stays one
// chain of kernel nodes.  `workspace`: naruto_track_workspace / naruto_ba_poses_workspace bytes; `who` heads a failed launch's message.
int launch_ray_point_grads(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, void* workspace, float* d_rays_o, float* d_rays_d, const char* who,
                           hipStream_t st) {
    const uint32_t S = t->n_samples_d + t->n_range_d, M = t->n_rays * S;
    NarutoPoints pts{};
    pts.rays_o = t->rays_o; pts.rays_d = t->rays_d; pts.z_vals = t->z_vals; pts.n_samples = S;
    if (int rc = check_points(&pts)) return rc;
    auto launched = [who](const char* kernel) {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? NARUTO_OK : fail(NARUTO_ERR_LAUNCH, "%s: %s: %s", who, kernel, hipGetErrorString(e));
    };
    float* gp = point_grad_ws(workspace, M).d_x;
    const uint64_t n_gp = 3u * (uint64_t)M;
    hipLaunchKernelGGL(k_track_zero, dim3((uint32_t)((n_gp + 255u) / 256u)), dim3(256), 0, st, gp, n_gp);
    if (int rc = launched("zero")) return rc;
    hipLaunchKernelGGL(k_query_bwd_points, dim3((M + (uint32_t)kPgThreads - 1u) / (uint32_t)kPgThreads), dim3(kPgThreads), 0, st, f->lt, f->ut, f->bt, make_points(&pts), M,
                       reinterpret_cast<const float2*>(p->table), p->uncert_grid, p->sdf_w0, p->sdf_w1, p->col_w0, p->col_w1, t->d_raw, nullptr, t->active_idx,
                       t->n_active, gp, 1, 0);
    if (int rc = launched("query_bwd_points")) return rc;
    hipLaunchKernelGGL(k_ray_point_reduce, dim3((t->n_rays + 3u) / 4u), dim3(256), 0, st, t->n_rays, S, gp, t->z_vals, d_rays_o, d_rays_d, 0);
    return launched("ray_point_reduce");
}
}  // namespace

size_t naruto_track_workspace(const NarutoField*, uint32_t n_rays, uint32_t n_samples) {
    const uint64_t M = (uint64_t)n_rays * n_samples;
    return M > (1ull << 29) ? 0u : point_grad_ws(nullptr, (size_t)M).total;
}

int naruto_track_draw(const NarutoTrackStep* k, const NarutoTrainStep* t, void* stream) {
    if (int rc = track_check(k, t, true, "track_draw")) return rc;
    const uint64_t n_int = (uint64_t)(k->H - 2u * k->edge_h) * (k->W - 2u * k->edge_w);
    hipLaunchKernelGGL(k_track_draw, dim3((k->n_rays + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, track_args(k, t), n_int, half_bits_for(n_int));
    return check_launch("track_draw");
}

int naruto_track_rays(const NarutoTrackStep* k, const NarutoTrainStep* t, void* stream) {
    if (int rc = track_check(k, t, false, "track_rays")) return rc;
    hipLaunchKernelGGL(k_track_rays, dim3((k->n_rays + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, track_args(k, t));
    return check_launch("track_rays");
}

int naruto_track_backward(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoTrackStep* k, void* stream) {
    if (int rc = train_check(f, p, t, "track_backward")) return rc;
    if (int rc = track_check(k, t, false, "track_backward")) return rc;
    if (t->smooth_points != 0) return fail(NARUTO_ERR_INVALID, "track_backward: tracking has no smoothness term (smooth_points must be 0)");
    if (t->loss_weights == nullptr || t->d_raw == nullptr || t->ray_count == nullptr || t->ray_offset == nullptr || t->active_idx == nullptr || t->n_active == nullptr)
        return fail(NARUTO_ERR_INVALID, "track_backward: NULL buffer in NarutoTrainStep");
    const hipStream_t st = (hipStream_t)stream;
    const TrainCtx c = train_ctx(f, t);
    if (c.M > (1u << 29)) return fail(NARUTO_ERR_INVALID, "track_backward: at most 2^29 samples per iteration (got %u)", c.M);
    if (int rc = ray_lds_attr()) return rc;
    if (int rc = loss_bwd_compact(f, t, c.w, train_loss_args(f, t), 0u, c.bw.n_total, st)) return rc;
    if (int rc = launch_ray_point_grads(f, p, t, k->workspace, k->d_rays_o, k->d_rays_d, "track_backward", st)) return rc;
    hipLaunchKernelGGL(k_track_step, dim3(1), dim3(kTrackStepThreads), 0, st, track_args(k, t));
    return check_launch("track_step");
}

// ------------------------------------------------------------------------------------------------
// Pose refinement inside global_BA (see naruto_bapose.hip)
// ------------------------------------------------------------------------------------------------
namespace {
int ba_poses_check(const NarutoBAPoses* b, const NarutoTrainStep* t, bool backward, const char* who) {
    if (b == nullptr) return fail(NARUTO_ERR_INVALID, "%s: NULL NarutoBAPoses", who);
    if (b->max_poses < 2u) return fail(NARUTO_ERR_INVALID, "%s: NarutoBAPoses.max_poses = %u (pose refinement needs at least 2 poses)", who, b->max_poses);
    if (b->pose_accum_step == 0u) return fail(NARUTO_ERR_INVALID, "%s: NarutoBAPoses.pose_accum_step must be positive", who);
    if (b->dyn == nullptr || b->poses == nullptr || b->pose_init == nullptr || b->pose6 == nullptr || b->exp_avg == nullptr || b->exp_avg_sq == nullptr ||
        b->accum == nullptr || b->state == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL buffer in NarutoBAPoses", who);
    const bool any_trace = b->trace_pose != nullptr || b->trace_grad != nullptr || b->max_trace != 0;
    const bool all_trace = b->trace_pose != nullptr && b->trace_grad != nullptr && b->max_trace != 0;
    if (any_trace && !all_trace) return fail(NARUTO_ERR_INVALID, "%s: the trace needs trace_pose, trace_grad and max_trace together", who);
    if (!(b->lr_rot >= 0.0f) || !(b->lr_trans >= 0.0f) || !(b->beta1 >= 0.0f && b->beta1 < 1.0f) || !(b->beta2 >= 0.0f && b->beta2 < 1.0f) || !(b->eps >= 0.0f))
        return fail(NARUTO_ERR_INVALID, "%s: Adam needs lr >= 0, 0 <= betas < 1 and eps >= 0", who);
    if (!backward) return NARUTO_OK;
    if (b->ids == nullptr || b->d_rays_o == nullptr || b->d_rays_d == nullptr || b->workspace == nullptr)
        return fail(NARUTO_ERR_INVALID, "%s: NULL ids / d_rays_o / d_rays_d / workspace in NarutoBAPoses", who);
    // without src_rows row r of the training batch IS assembled row r
    if (b->n_ids == 0u || (b->src_rows == nullptr && b->n_ids < t->n_rays))
        return fail(NARUTO_ERR_INVALID, "%s: NarutoBAPoses.n_ids = %u pose ids for %u rays", who, b->n_ids, t->n_rays);
    const uint64_t M = (uint64_t)t->n_rays * (t->n_samples_d + t->n_range_d);
    if (M > (1ull << 29)) return fail(NARUTO_ERR_INVALID, "%s: at most 2^29 samples per iteration (got %llu)", who, (unsigned long long)M);
    return NARUTO_OK;
}

BAPoseArgs ba_pose_args(const NarutoBAPoses* b, const NarutoTrainStep* t) {
    BAPoseArgs a{};
    a.max_poses = b->max_poses; a.optim_cur = b->optim_cur != 0u ? 1 : 0; a.accum_step = b->pose_accum_step; a.dyn = b->dyn;
    a.poses = b->poses; a.pose_init = b->pose_init; a.pose6 = b->pose6; a.exp_avg = b->exp_avg; a.exp_avg_sq = b->exp_avg_sq; a.accum = b->accum; a.state = b->state;
    a.ids = b->ids; a.n_ids = b->n_ids; a.src_rows = b->src_rows;
    if (t != nullptr) { a.n_rays = t->n_rays; a.rays_d = t->rays_d; }
    a.d_rays_o = b->d_rays_o; a.d_rays_d = b->d_rays_d;
    a.lr_rot = b->lr_rot; a.lr_trans = b->lr_trans; a.beta1 = b->beta1; a.beta2 = b->beta2; a.eps = b->eps;
    a.trace_pose = b->trace_pose; a.trace_grad = b->trace_grad; a.max_trace = b->max_trace;
    return a;
}

// after the loss backward and the compaction: the rays' gradients, the per-pose sums and the pose step
int ba_poses_launch(const NarutoField* f, const NarutoParams* p, const NarutoTrainStep* t, const NarutoBAPoses* b, hipStream_t st) {
    if (int rc = launch_ray_point_grads(f, p, t, b->workspace, b->d_rays_o, b->d_rays_d, "ba_poses", st)) return rc;
    const BAPoseArgs a = ba_pose_args(b, t);
    hipLaunchKernelGGL(k_ba_pose_accum, dim3(b->max_poses), dim3(kBaPoseThreads), 0, st, a);
    if (int rc = check_launch("ba_pose_accum")) return rc;
    hipLaunchKernelGGL(k_ba_pose_step, dim3(1), dim3(kBaPoseThreads), 0, st, a);
    return check_launch("ba_pose_step");
}
}  // namespace

size_t naruto_ba_poses_workspace(const NarutoField*, uint32_t n_rays, uint32_t n_samples) {
    const uint64_t M = (uint64_t)n_rays * n_samples;
    return M > (1ull << 29) ? 0u : point_grad_ws(nullptr, (size_t)M).total;
}

int naruto_ba_poses_init(const NarutoBAPoses* b, void* stream) {
    if (int rc = ba_poses_check(b, nullptr, false, "ba_poses_init")) return rc;
    hipLaunchKernelGGL(k_ba_pose_init, dim3((b->max_poses + (uint32_t)kBaPoseThreads - 1u) / (uint32_t)kBaPoseThreads), dim3(kBaPoseThreads), 0, (hipStream_t)stream,
                       ba_pose_args(b, nullptr));
    return check_launch("ba_pose_init");
}

int naruto_debug_ba_poses_check(const NarutoBAPoses* b, uint32_t n_rays) {
    NarutoTrainStep t{};
    t.n_rays = n_rays; t.n_samples_d = 1; t.n_range_d = 1;
    return ba_poses_check(b, &t, true, "debug_ba_poses_check");
}

int naruto_debug_ba_poses_fields(const NarutoBAPoses* b, uint64_t out[25]) {
    if (b == nullptr || out == nullptr) return fail(NARUTO_ERR_INVALID, "debug_ba_poses_fields: NULL argument");
    auto fbits = [](float v) { uint32_t u; memcpy(&u, &v, 4); return (uint64_t)u; };
    const uint64_t v[25] = {b->max_poses, b->optim_cur, b->pose_accum_step, (uint64_t)(uintptr_t)b->dyn, (uint64_t)(uintptr_t)b->poses, (uint64_t)(uintptr_t)b->pose_init,
                            (uint64_t)(uintptr_t)b->pose6, (uint64_t)(uintptr_t)b->exp_avg, (uint64_t)(uintptr_t)b->exp_avg_sq, (uint64_t)(uintptr_t)b->accum,
                            (uint64_t)(uintptr_t)b->state, (uint64_t)(uintptr_t)b->ids, b->n_ids, (uint64_t)(uintptr_t)b->src_rows, (uint64_t)(uintptr_t)b->d_rays_o,
                            (uint64_t)(uintptr_t)b->d_rays_d, fbits(b->lr_rot), fbits(b->lr_trans), fbits(b->beta1), fbits(b->beta2), fbits(b->eps),
                            (uint64_t)(uintptr_t)b->trace_pose, (uint64_t)(uintptr_t)b->trace_grad, b->max_trace, (uint64_t)(uintptr_t)b->workspace};
    for (int i = 0; i < 25; ++i) out[i] = v[i];
    return NARUTO_OK;
}

int naruto_debug_pose_adam(float* pose, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t step, float lr_rot, float lr_trans, float beta1, float beta2,
                           float eps) {
    if (pose == nullptr || grad == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || step < 1) return fail(NARUTO_ERR_INVALID, "debug_pose_adam: NULL argument or step < 1");
    pose_adam_step(pose, grad, exp_avg, exp_avg_sq, step, lr_rot, lr_trans, beta1, beta2, eps);
    return NARUTO_OK;
}

int naruto_debug_ba_pose_sums(uint32_t n_rays, const int64_t* ids, uint32_t n_ids, const uint32_t* src_rows, uint32_t n_poses, uint32_t pose, const float* rays_d,
                              const float* d_rays_o, const float* d_rays_d, const float* pose6, double* sums, float* grad) {
    if (ids == nullptr || rays_d == nullptr || d_rays_o == nullptr || d_rays_d == nullptr || sums == nullptr)
        return fail(NARUTO_ERR_INVALID, "debug_ba_pose_sums: NULL argument");
    if (pose >= n_poses) return fail(NARUTO_ERR_INVALID, "debug_ba_pose_sums: pose %u of %u", pose, n_poses);
    if (grad != nullptr && pose6 == nullptr) return fail(NARUTO_ERR_INVALID, "debug_ba_pose_sums: the gradient needs the pose");
    // k_ba_pose_accum's order: thread t takes rays t, t + 256, ...; then the tree
    double red[kBaPoseThreads][12];
    for (uint32_t tid = 0; tid < (uint32_t)kBaPoseThreads; ++tid) {
        for (int k = 0; k < 12; ++k) red[tid][k] = 0.0;
        for (uint32_t r = tid; r < n_rays; r += kBaPoseThreads) ba_row_add(red[tid], pose, n_poses, r, ids, n_ids, src_rows, rays_d, d_rays_o, d_rays_d);
    }
    for (uint32_t h = kBaPoseThreads / 2; h > 0; h >>= 1)
        for (uint32_t tid = 0; tid < h; ++tid)
            for (int k = 0; k < 12; ++k) red[tid][k] += red[tid + h][k];
    for (int k = 0; k < 12; ++k) sums[k] += red[0][k];
    if (grad != nullptr) ba_pose_grad(pose6, sums, grad);
    return NARUTO_OK;
}

int naruto_debug_rodrigues(const double* w, const double* G, double* R, double* d_w) {
    if (w == nullptr || (d_w != nullptr && G == nullptr)) return fail(NARUTO_ERR_INVALID, "debug_rodrigues: NULL argument");
    if (R != nullptr) rodrigues(w, R);
    if (d_w != nullptr) rodrigues_vjp(w, G, d_w);
    return NARUTO_OK;
}

int naruto_debug_pose_log(uint32_t P, const float* c2w, float* pose6) {
    if (c2w == nullptr || pose6 == nullptr) return fail(NARUTO_ERR_INVALID, "debug_pose_log: NULL argument");
    for (uint32_t p = 0; p < P; ++p) pose_log(c2w + 16 * (size_t)p, pose6 + 6 * (size_t)p);
    return NARUTO_OK;
}

int naruto_debug_icp_solve(const double* sums, const double* origin, double* dT, int32_t* status) {
    if (sums == nullptr || dT == nullptr || status == nullptr) return fail(NARUTO_ERR_INVALID, "debug_icp_solve: NULL argument");
    const double zero[3] = {0.0, 0.0, 0.0};
    double ratio;
    *status = icp_solve(sums, origin != nullptr ? origin : zero, dT, ratio);
    return NARUTO_OK;
}

int naruto_debug_odom_solve(NarutoOdomSolve* solve) {
    if (solve == nullptr) return fail(NARUTO_ERR_INVALID, "debug_odom_solve: NULL argument");
    solve->status = odom_solve(solve->sums, solve->xi);
    odom_exp(solve->xi, solve->dT);
    return NARUTO_OK;
}

}  // extern "C"

namespace {
// workspace of the image metrics over P views of H x W: | six partial sums per 16 x 16 tile and view |
struct MetricWs { double* partial; uint32_t tiles_x, tiles_y; size_t total; };
MetricWs metric_ws(uint32_t P, uint32_t H, uint32_t W, void* workspace) {
    const uint32_t tx = (W + kMetTile - 1u) / kMetTile, ty = (H + kMetTile - 1u) / kMetTile;
    Carve c(workspace);
    return {c.take<double>((size_t)P * tx * ty * 6u * sizeof(double)), tx, ty, c.size()};
}
int view_check(const NarutoCullCam* cam, uint32_t n_poses, const float* poses, uint32_t p0, uint32_t p1, const char* who) {
    if (int rc = cull_cam_check(cam, who)) return rc;
    if (n_poses == 0 || poses == nullptr) return fail(NARUTO_ERR_INVALID, "%s: no poses", who);
    if ((uint64_t)n_poses * cam->H * cam->W >= (1ull << 32)) return fail(NARUTO_ERR_INVALID, "%s: poses x pixels per call must stay below 2^32: use fewer poses per call", who);
    if (p0 > p1 || (uint64_t)p1 > (uint64_t)n_poses * cam->H * cam->W) return fail(NARUTO_ERR_INVALID, "%s: pixel range [%u, %u) of %u poses x %u x %u", who, p0, p1, n_poses, cam->H, cam->W);
    return NARUTO_OK;
}
ViewCam view_cam(const NarutoCullCam* cam) { return ViewCam{cam->H, cam->W, cam->fx, cam->fy, cam->cx, cam->cy}; }
}  // namespace

extern "C" {

int naruto_view_rays(const NarutoCullCam* cam, uint32_t n_poses, const float* poses, uint32_t p0, uint32_t p1, float* rays_o, float* rays_d, void* stream) {
    if (int rc = view_check(cam, n_poses, poses, p0, p1, "view_rays")) return rc;
    if (rays_o == nullptr || rays_d == nullptr) return fail(NARUTO_ERR_INVALID, "view_rays: NULL output");
    const uint32_t n = p1 - p0;
    if (n == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_view_rays, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, view_cam(cam), poses, p0, n, rays_o, rays_d);
    return check_launch("view_rays");
}

int naruto_view_crossing(uint32_t n_rays, uint32_t n_samples, const float* raw, const float* z_vals, float* z_star, void* stream) {
    if (raw == nullptr || z_vals == nullptr || z_star == nullptr) return fail(NARUTO_ERR_INVALID, "view_crossing: NULL argument");
    if (n_samples < 2 || n_samples > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "view_crossing: need 2 <= samples per ray <= %d (got %u)", kMaxSamples, n_samples);
    if (n_rays == 0) return NARUTO_OK;
    hipLaunchKernelGGL(k_view_crossing, dim3((n_rays + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, n_rays, n_samples, raw, z_vals, z_star);
    return check_launch("view_crossing");
}

int naruto_render_view(const NarutoField* f, const NarutoParams* p, const NarutoCullCam* cam, const NarutoViewRender* r, void* stream) {
    if (f == nullptr || p == nullptr || r == nullptr) return fail(NARUTO_ERR_INVALID, "render_view: NULL argument");
    if (int rc = check_params(p, "render_view")) return rc;
    if (int rc = view_check(cam, r->n_poses, r->poses, r->p0, r->p1, "render_view")) return rc;
    const uint32_t S = r->n_samples_d + r->n_range_d;
    // the per-ray LDS limit of naruto_render_fwd's one-wave-per-ray launch
    if (S < 2 || S > (uint32_t)kMaxSamples) return fail(NARUTO_ERR_INVALID, "render_view: need 2 <= fine samples per ray <= %d (got %u)", kMaxSamples, S);
    if (r->target_d == nullptr && (r->n_coarse < 2 || r->n_coarse > (uint32_t)kMaxSamples))
        return fail(NARUTO_ERR_INVALID, "render_view: need 2 <= n_coarse <= %d (got %u)", kMaxSamples, r->n_coarse);
    const uint32_t n = r->p1 - r->p0;
    if (n == 0) return NARUTO_OK;
    ViewArgs a{};
    a.cam = view_cam(cam); a.poses = r->poses; a.p0 = r->p0; a.n_rays = n; a.target_d = r->target_d;
    a.near_ = cam->near_; a.far_ = cam->far_; a.range_d = r->range_d; a.nu = r->n_samples_d; a.nr = r->n_range_d; a.n_coarse = r->n_coarse;
    a.trunc = f->desc.trunc; a.sc_factor = f->desc.sc_factor; a.white_bkgd = f->desc.white_bkgd;
    a.rgb = r->rgb; a.depth = r->depth; a.acc = r->acc; a.depth_var = r->depth_var; a.uncert_map = r->uncert_map; a.surface_z = r->surface_z;
    // naruto_render_fwd's two four-wave forms, chosen as it chooses them: the fine pass's tiles are then that launch's
    const bool bf = f->desc.mlp_mode == NARUTO_MLP_BF16;
    const uint32_t cap = cu_count(f) * 4u;
    const hipStream_t st = (hipStream_t)stream;
    if (S <= 64u) {
        static bool attr_packed = false;
        const size_t reserved = render_packed_lds_bytes(64u), dyn = render_packed_lds_bytes(S);
        if (int rc = reserve_lds(attr_packed, {lds_use(k_render_view_packed<false>, reserved), lds_use(k_render_view_packed<true>, reserved)}, "render_view: cannot reserve %zu bytes of LDS", reserved)) return rc;
        const uint32_t groups = (n + kPackRays - 1u) / kPackRays, blocks = groups < cap ? groups : cap;
        if (bf) hipLaunchKernelGGL(k_render_view_packed<true>, dim3(blocks), dim3(256), dyn, st, f->lt, f->ut, f->bt, *p, a);
        else hipLaunchKernelGGL(k_render_view_packed<false>, dim3(blocks), dim3(256), dyn, st, f->lt, f->ut, f->bt, *p, a);
        return check_launch("render_view_packed");
    }
    static bool attr_set = false;
    const size_t reserved = ray_scratch_bytes(kMaxSamples), dyn = ray_scratch_bytes(S);
    if (int rc = reserve_lds(attr_set, {lds_use(k_render_view<false>, reserved), lds_use(k_render_view<true>, reserved)}, "render_view: cannot reserve %zu bytes of LDS", reserved)) return rc;
    const uint32_t blocks = (n + 3u) / 4u < cap ? (n + 3u) / 4u : cap;
    if (bf) hipLaunchKernelGGL(k_render_view<true>, dim3(blocks), dim3(256), dyn, st, f->lt, f->ut, f->bt, *p, a);
    else hipLaunchKernelGGL(k_render_view<false>, dim3(blocks), dim3(256), dyn, st, f->lt, f->ut, f->bt, *p, a);
    return check_launch("render_view");
}

size_t naruto_image_metrics_workspace(uint32_t n_views, uint32_t H, uint32_t W) {
    if (n_views == 0 || H == 0 || W == 0 || n_views > 65535u || (uint64_t)H * W > (1ull << 30)) return 0;
    return metric_ws(n_views, H, W, nullptr).total;
}

int naruto_image_metrics(uint32_t n_views, uint32_t H, uint32_t W, const float* rgb, const float* depth, const float* gt_rgb, const float* gt_depth, int has_depth_trunc,
                         float depth_trunc, const double* window, void* workspace, double* out, double* se_map, double* de_map, double* ssim_map, void* stream) {
    if (naruto_image_metrics_workspace(n_views, H, W) == 0) return fail(NARUTO_ERR_INVALID, "image_metrics: need 1 .. 65535 views of 1 .. 2^30 pixels");
    if (rgb == nullptr || depth == nullptr || gt_rgb == nullptr || gt_depth == nullptr || window == nullptr || workspace == nullptr || out == nullptr)
        return fail(NARUTO_ERR_INVALID, "image_metrics: NULL argument");
    const MetricWs w = metric_ws(n_views, H, W, workspace);
    MetricArgs a{};
    a.P = n_views; a.H = H; a.W = W; a.tiles_x = w.tiles_x; a.tiles_y = w.tiles_y;
    a.rgb = rgb; a.depth = depth; a.gt_rgb = gt_rgb; a.gt_depth = gt_depth; a.depth_trunc = depth_trunc; a.has_trunc = has_depth_trunc != 0;
    a.partial = w.partial; a.se_map = se_map; a.de_map = de_map; a.ssim_map = ssim_map;
    MetricWin win;
    for (int t = 0; t < kMetWin; ++t) win.w[t] = window[t];                 // HOST array of 11 doubles
    hipLaunchKernelGGL(k_metrics_tile, dim3(w.tiles_x, w.tiles_y, n_views), dim3(256), 0, (hipStream_t)stream, a, win);
    if (int rc = check_launch("metrics_tile")) return rc;
    hipLaunchKernelGGL(k_metrics_finish, dim3(n_views), dim3(64), 0, (hipStream_t)stream, w.tiles_x * w.tiles_y, w.partial, out);
    return check_launch("metrics_finish");
}

}  // extern "C"
