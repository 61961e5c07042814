// Launch plan of the weight gradients (igemm_tn.hip): which kernel a shape runs on, how its K range is split, where the splits store
// and how their slabs are summed -- decided here, once per launch, by a pure function of the shape.  Plain C++: no device call, so the
// decision can be read from the CPU (frhip_wgrad_plan) and is pinned by tests/test_tn_plan_cpu.py.
#pragma once
#include <cstddef>
#include "frhip.h"

namespace frhip {

constexpr int TN_PLAN_KP = 64;         // pixels per K step of the per-tap and nine-tap kernels (TN_KP)
constexpr int TN_PLAN_T9_MAXW = 56;    // widest map of the nine-tap kernel (T9_MAXW)

enum TnFamily { TN_TAP128 = 0, TN_TAP256 = 1, TN_TAPS9 = 2, TN_ROWS = 3 };      // per-tap tile of 128-byte / 256-byte rows, nine-tap, rows (14 x 14)
enum TnStore { TN_STORE_OUT = 0, TN_STORE_SLABS = 1, TN_STORE_OVERWRITE = 2 };

// the validated shape: P = [M = n ho wo][ldp] (kc valid columns), Q = [n][h][w][c]
struct TnShape {
    int dtype, n, h, w, c, kc, ldp, r, s, stride, pad;
    int es() const { return dtype == FRHIP_DT_BF16 ? 2 : 4; }
    int ho() const { return (h + 2 * pad - r) / stride + 1; }
    int wo() const { return (w + 2 * pad - s) / stride + 1; }
    long long M() const { return 1LL * n * ho() * wo(); }
    size_t out_elems() const { return (size_t)kc * r * s * c; }
};

struct TnPlan {
    // family: TnFamily.  Nine-tap instantiation: window stages (2 of 192 rows, 3 of 128, 4 of 96), lane-mask table wanted, operand transform.
    // Whether the table can be had (stream capture, cache full, period too long) is known at launch only: without it the same plan runs
    // table = false.  clear_out: out = result with several splits, `out` is cleared first
    int family, stages;
    bool table, transform, clear_out;
    int splits, ksteps, ksteps_per_split;       // rows family: a K step is one image
    // TN_STORE_OUT: one split, added into `out`; TN_STORE_SLABS: every split stores a slab of the workspace and the reduce tree adds them to
    // `out`; TN_STORE_OVERWRITE: out = result with one split -- the slab store path with slab 0 = `out` itself, no reduce
    int store;
    size_t out_elems;
    // reduce tree (groups = 0: none): `groups` > 1 groups of `per_group` slabs are summed first, in place, then one final pass over the
    // group sums; groups = 1: the final pass alone.  `blocks` workgroups per pass
    int groups, per_group, blocks;

    // the instantiation as one number, 100 transform + 10 table + stages (0 for the other families): frhip_wgrad_plan reports it
    int inst() const { return family == TN_TAPS9 ? 100 * transform + 10 * table + stages : 0; }
};

inline bool tn_taps9_ok(const TnShape& sh, int taps9) {
    // 3 x 3 / stride 1 / pad 1 keeps the map size: M = n h w
    return taps9 && sh.dtype == FRHIP_DT_BF16 && sh.r == 3 && sh.s == 3 && sh.stride == 1 && sh.pad == 1 && sh.w <= TN_PLAN_T9_MAXW &&
           1LL * (1LL * sh.n * sh.h * sh.w + 64 + 2LL * sh.w + 2) * (sh.ldp > sh.c ? sh.ldp : sh.c) * 2 < 0x7fffffffLL;
}
inline bool tn_rows_ok(const TnShape& sh, int taps9) {
    return tn_taps9_ok(sh, taps9) && sh.h == 14 && sh.w == 14 && (sh.c % 64) == 0 && (sh.kc % 64) == 0;
}

// Split-K search: the grid should fill whole "rounds" of the chip (`slots` resident workgroups) with as few splits as possible -- every
// extra split adds a full slab of the output tile to store and to reduce, and a partially filled last round wastes up to a third of the
// launch.  time ~ rounds * (K steps per split + the epilogue's cost in K steps); a split count is taken when it is 2 % better.
// The three families were tuned apart and differ in MORE than the constants: the rows kernel counts whole images per split where the
// other two divide exactly, and the per-tap kernel states "2 % better" on 1 / t (t < best / 1.02) where the other two state it on t
// (t < 0.98 best).  Neither pair is the same inequality, so both forms are parameters: every launch keeps the split count it had.
struct TnCost { int slots, cap; double epilogue; bool whole_steps, on_score; };
constexpr TnCost TN_COST_ROWS = {256, 1024, 2.0, true, false};        // one workgroup per CU; nine store passes of 36 KB per wave ~ two images
constexpr TnCost TN_COST_TAPS9 = {256, 1024, 8.0, false, false};      // one workgroup per CU; nine store passes ~ 8 K steps
constexpr TnCost TN_COST_TAP128 = {256 * 4, 512, 6.0, false, true};   // LDS-limited residency: 4 (32 KB) per CU
constexpr TnCost TN_COST_TAP256 = {256 * 2, 512, 6.0, false, true};   //                        2 (64 KB) per CU
inline int tn_search_splits(long long tiles, int ksteps, int max_splits, const TnCost& cost) {
    int best = 1; double best_t = 1e30;
    for (int sp = 1; sp <= max_splits && sp <= cost.cap; ++sp) {
        const long long rounds = (tiles * sp + cost.slots - 1) / cost.slots;
        const double per = cost.whole_steps ? (double)((ksteps + sp - 1) / sp) : (double)ksteps / sp;
        const double t = (double)rounds * (per + cost.epilogue);
        if (cost.on_score ? 1.0 / t > 1.0 / best_t * 1.02 : t < best_t * 0.98) { best_t = t; best = sp; }
    }
    return best;
}

// K splits that added their partial tiles into `out` with fp32 atomics would sum them in whatever order they land, and the
// weight gradient would change from run to run.  So a launch uses no more K splits than the workspace has slabs for (one split
// -- each element added once -- where the slab path is closed: no workspace, or an output that the float4 slab layout does not
// hold, `quads` false: out_elems % 4, and kc % 4 for the nine-tap writer, which packs co in fours).
inline int tn_slab_splits(int splits, size_t out_elems, bool quads, bool have_ws, size_t ws_bytes) {
    if (splits <= 1) return splits;
    if (!have_ws || !quads) return 1;
    const size_t fit = ws_bytes / (out_elems * sizeof(float));
    return fit < 1 ? 1 : ((size_t)splits > fit ? (int)fit : splits);
}

// one pass while it has enough blocks to stream (or few slabs); else a two-level tree: groups of slabs first
inline void tn_reduce_tree(TnPlan& pl) {
    if (pl.store != TN_STORE_SLABS) return;         // groups = 0
    const size_t n4 = pl.out_elems / 4;
    pl.blocks = (int)((n4 + 255) / 256); if (pl.blocks > 2048) pl.blocks = 2048;
    int groups = 1;
    while (pl.splits > 32 * groups && pl.blocks * groups < 512) groups *= 2;
    pl.per_group = (pl.splits + groups - 1) / groups;
    pl.groups = (pl.splits + pl.per_group - 1) / pl.per_group;
}

// at most `splits` K splits (at most ksteps) of whole K steps; more than one: they store to slabs, which the caller has made sure of
inline TnPlan tn_split(int family, size_t out_elems, int ksteps, int splits) {
    TnPlan pl{};
    pl.family = family; pl.out_elems = out_elems; pl.ksteps = ksteps;
    if (splits > ksteps) splits = ksteps;
    pl.ksteps_per_split = (ksteps + splits - 1) / splits;
    pl.splits = (ksteps + pl.ksteps_per_split - 1) / pl.ksteps_per_split;
    pl.store = pl.splits > 1 ? TN_STORE_SLABS : TN_STORE_OUT;
    tn_reduce_tree(pl);
    return pl;
}

// Rows kernel: K split over whole images.  It has no single-split form that adds into `out`: the caller checks that every split has a slab.
inline TnPlan tn_plan_rows(const TnShape& sh, int splits) {
    if (splits <= 0) splits = tn_search_splits(1LL * (sh.kc / 64) * (sh.c / 64), sh.n, sh.n, TN_COST_ROWS);
    return tn_split(TN_ROWS, sh.out_elems(), sh.n, splits);
}

// The plan of one launch.  splits <= 0: the search picks; overwrite: out = result (per-tap family only -- the head's dW); taps9: the
// frhip_set_wgrad_taps9 switch.  The nine-tap kernel covers every 3x3/s1/p1 bf16 layer, the rows kernel those of 14 x 14 maps whose
// splits all have slabs (else the layer falls through to the nine-tap kernel), the per-tap kernel everything else.
inline TnPlan tn_plan(const TnShape& sh, int splits, bool have_ws, size_t ws_bytes, bool overwrite, bool transform, int taps9) {
    const size_t out_elems = sh.out_elems();
    const bool quads = (out_elems % 4) == 0, nine = tn_taps9_ok(sh, taps9);
    if (!transform && tn_rows_ok(sh, taps9)) {
        const TnPlan rows = tn_plan_rows(sh, splits);
        if (rows.splits > 1 && tn_slab_splits(rows.splits, out_elems, quads, have_ws, ws_bytes) == rows.splits) return rows;
    }
    const int ksteps = (int)((sh.M() + TN_PLAN_KP - 1) / TN_PLAN_KP), es = sh.es();
    const bool big = (sh.c * es >= 256) && (sh.kc * es >= 256);
    if (splits <= 0 && nine) splits = tn_search_splits(1LL * ((sh.kc + 63) / 64) * ((sh.c + 63) / 64), ksteps, ksteps / 8, TN_COST_TAPS9);
    if (splits <= 0) {
        const int bc = (big ? 256 : 128) / es;
        const long long tiles = 1LL * ((sh.kc + bc - 1) / bc) * ((sh.c + bc - 1) / bc) * sh.r * sh.s;
        splits = tn_search_splits(tiles, ksteps, (ksteps + 7) / 8, big ? TN_COST_TAP256 : TN_COST_TAP128);      // >= 8 K steps per workgroup
    }
    TnPlan pl = tn_split(nine ? TN_TAPS9 : big ? TN_TAP256 : TN_TAP128, out_elems, ksteps,
                         tn_slab_splits(splits, out_elems, quads && (!nine || sh.kc % 4 == 0), have_ws, ws_bytes));
    if (nine) {
        // W <= 14: a 96-row window, 20-KB stages -- FOUR fit the co-resident tile's 82-KB request, so an operand load has three K steps to
        // land (not with the operand transform); W <= 31: three stages of a 128-row window
        const int window = 64 + 2 * sh.w + 2;
        pl.stages = window > 128 ? 2 : (window > 96 || transform) ? 3 : 4;
        pl.transform = transform;
        pl.table = !transform;
    } else if (overwrite) {
        // out = result (not +=).  A single K split: plain coalesced stores, no zero fill by the caller and no fp32 atomic read-modify-write
        // pass over the output (the head's 250-MB dW)
        if (pl.splits == 1) pl.store = TN_STORE_OVERWRITE;
        pl.clear_out = pl.splits > 1;
    }
    return pl;
}

}  // namespace frhip
