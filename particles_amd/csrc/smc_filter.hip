// smc_filter.hip -- host side of the fused on-device SMC step loop
// (smc_filter_* of include/smc_hip.h).  The kernels and the description of the
// two-kernel step are in smc_filter_kernels.h.
#include <type_traits>
#include <vector>

#include "smc_filter_mv.h"
#include "smc_filter_small.h"
#include "smc_filter_sqmc.h"
#include "smc_filter_wide.h"
#include "smc_filter_strict.h"
#include "smc_smooth.h"
#include "smc_smooth_qmc.h"
#include "smc_online.h"
#include "smc_twofilter.h"
#include "smc_csmc.h"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
#define PROF_MAX 4096
#define F_OPT 4        /* new particles per thread of k_propagate */
#define F_WIDE_TPW 2   /* tiles per workgroup of k_ancestors2w (C2: 17.6 us per step, 4 tiles 18.3, one tile 18.1: profiles/r12d) */

// The step plan: which launches one time step of this filter makes.  plan_step decides it once, in
// smc_filter_create; enqueue_step, smc_filter_describe, small_filter_ok and smc_filter_step read it and decide
// nothing themselves.  What may change after create stays an input of the call: a.ut (smc_filter_set_replay: the
// uniforms come from a tape, no spacings launches), f->prof, whether the step's time index is known (graph capture).
//
//   kind            resampling part of the step                                          step record
//   STEP_FLAT       [SQMC prologue] [k_mv_aux, k_mv_aux_restate] [k_prepare] [spacings: three passes]
//                   k_ancestors [k_sqmv_compose]                                          k_propagate's tail
//   STEP_TWO_LEVEL  [reduce] [spacings: one pass (+ reduce merged) | three passes] k_ancestors2 | k_ancestors2w
//                                                                                         two-level (k_flush2)
//   STEP_STRICT     [reduce] [spacings: one pass (+ reduce merged) | per island] then by strict_form
//                   literal:   k_strict_W, k_strict_cdf, k_strict_search_S
//                   two-level: k_strict_classify, k_strict_search
//                   array:     k_strict_W, k_sqx_classify, k_sqx_fill, k_strict_search_S      as two_level says
//   STEP_SQMC       t = 0: k_sq_init; else sort, k_sq_permute, reduce, k_ancestors2<tape, sorted positions>
//                                                                                         two-level
//   every kind then: k_propagate | k_propagate_mv, [k_flush2 (two-level record)], [moments kernels]
//
// Which combinations exist:
//   * two_level: univariate, 2 tiles <= N <= 2^30, neither SMC_PATH_FLAT_CDF nor SMC_PATH_FORCE_UNFUSED.  STEP_TWO_LEVEL
//     and STEP_SQMC always are; STEP_STRICT is where the filter would be otherwise; STEP_FLAT never is (MVLINGAUSS,
//     one tile, N > 2^30, the two test flags).
//   * SQMC (SMC_FLAG_SQMC; the scheme is multinomial over a tape of sorted points, every step resamples): univariate
//     N = 2^k >= 2 tiles is STEP_SQMC; MVLINGAUSS and N < 2 tiles are STEP_FLAT with sq_flat.  Never strict.
//   * reduce: REDUCE_NONE where the resampling kernel's workgroups reduce the island's partials themselves (resident
//     grid of at most 1024 tiles per island, closed-form counts, no APF); otherwise a launch opens the step --
//     k_reduce2w for islands of 1025 .. 4096 tiles (the same bits from 1024 threads), k_reduce2 for the rest, for the
//     APF's two sets of partials and under SMC_PATH_NO_WIDE.  Always with multinomial counts, SQMC, the strict literal
//     walk on a two-level record; never on a flat record.
//   * spacings (multinomial scheme with Philox draws only: SP_NONE for the other schemes and for SQMC):
//     SP_ONEPASS[_MERGED] needs two_level and a launch that stays resident (sp_tpw tiles of draws per workgroup, sp_nwg
//     workgroups per island), not the strict literal walk, not SMC_PATH_SPACING_3PASS; _MERGED (the reduction is
//     workgroup 0 of that launch while the time index is known) also needs eager launches and no
//     SMC_PATH_SPLIT_REDUCE.  Otherwise SP_THREE_PASS, or SP_PER_ISLAND under STEP_STRICT.
//   * resampler: RS_PREPARE / RS_FUSED (k_ancestors; fused while every workgroup is resident) without two_level,
//     RS_TILE / RS_WIDE with it.  RS_WIDE (k_ancestors2w) only under STEP_TWO_LEVEL with reduce == REDUCE_NONE: N = 2^k
//     with an even number of tiles (either closed-form scheme) or any other N under the systematic scheme; SMC_PATH_NO_WIDE
//     keeps RS_TILE.  The template arguments come from a.log2N (POW2) and a.scheme.
//   * lazy_lw: on a step that resamples, k_propagate's log-weights are read by nobody unless the NEXT step does not
//     resample -- and that step can form them again from X (bootstrap move behind a resampling: lw = log p(y | x)).  Where
//     the plan says so, the steps in the INTERIOR of one smc_filter_step call leave that store out (8 of the 24 bytes per
//     particle the launch writes); the last step of every call stores, so whoever holds the filter between two calls
//     sees lw as ever.  Needs STEP_TWO_LEVEL (strict and flat steps read lw when they resample; SQMC sorts them), two
//     alternating slots (hist == 0: the kernels that take their slots from a.par), no device moments (they read lw of
//     every step), a bootstrap filter of a model whose observation density reads the new particle only (not SVLEVERAGE;
//     MVLINGAUSS is never two-level), eager launches (no use_graph) and not SMC_PATH_EAGER_LW (the verification twin:
//     every step stores).  The theta level's loop and captured steps never ask for it (enqueue_step's `lazy`).
//   * small: N <= 1024, univariate, no moments: smc_filter_step runs k_filter_small instead of any of the above unless
//     profiling is on or the draws are Philox multinomial (small_filter_ok); SMC_PATH_NO_SMALL, strict and SQMC never do.
enum StepKind { STEP_FLAT, STEP_TWO_LEVEL, STEP_STRICT, STEP_SQMC };
enum StrictForm { STRICT_LITERAL, STRICT_TWO_LEVEL, STRICT_ARRAY };
enum ReduceKernel { REDUCE_NONE, REDUCE_NARROW, REDUCE_WIDE };
enum Spacings { SP_NONE, SP_ONEPASS, SP_ONEPASS_MERGED, SP_THREE_PASS, SP_PER_ISLAND };
enum Resampler { RS_PREPARE, RS_FUSED, RS_TILE, RS_WIDE };

struct StepPlan {
    StepKind kind = STEP_FLAT;
    bool two_level = false;        // the step record is the two-level one: tail-free k_propagate, k_flush2, a.kform
    bool sq_flat = false;          // STEP_FLAT behind the SQMC prologue / epilogue
    StrictForm strict_form = STRICT_ARRAY;
    ReduceKernel reduce = REDUCE_NONE;
    Spacings spacings = SP_NONE;
    int sp_tpw = 0, sp_nwg = 0;    // (copied into the argument block: the kernel reads them)
    Resampler resampler = RS_PREPARE;
    int ragged = 0;                // two-level record with N not a multiple of the tile: 1 (N even), 2 (N odd or history
                                   // slots), else 0 (k_propagate<.., RAGGED>)
    bool xcd_chunks = false;       // consecutive tiles on one XCD (f_tile_xcd; copied into the argument block)
    bool heavy_list = false;       // heavy parents registered by the resampling kernel (a.hcnt, a.hlist)
    bool apf2 = false;             // APF on the two-level record: the reduction forms two sets of partials (a.pm2 ..)
    bool small = false;            // the one-launch filter may run (see small_filter_ok)
    bool sq_recompute = false;     // STEP_SQMC: sorted weights recomputed from the sorted keys (k_sq_permute<.., true>)
    bool mv_collapsed = false;     // MVLINGAUSS guided: log G = log p(y_t | x_{t-1}) in one product (opts.flags)
    bool no_tk = false;            // SMC_PATH_NO_TK: kernels never start on the host's time index (A/B)
    bool lazy_lw = false;          // interior steps of a smc_filter_step call may leave a resampling step's lw unwritten

    bool strict() const { return kind == STEP_STRICT; }
    bool sqmc() const { return kind == STEP_SQMC || sq_flat; }
};

struct smc_filter {
    smc_ctx* ctx = nullptr;
    FArgs a;               // the argument block: passed BY VALUE (kernarg segment: one scalar-load hop,
                           // and the compiler knows its pointers address global memory)
    StepPlan plan;
    int kind = 0, fk = 0;
    i64 t_host = 0;
    void* slab = nullptr;  // one allocation holding every device array
    size_t slab_bytes = 0;
    bool use_graph = false;
    double* strict_ws = nullptr;   // (n_islands, N) W | (n_islands, N) S | scratch of smc_seqsum.h
    bool sq_plan_zero = false;     // SQMC: the sort workspace's plan words are zero (smc_rs_sort_ws leaves them so)
    u64 sp_epoch = 0;      // launches of the merged spacings + reduction kernel so far (see FArgs::sp_epoch)
    bool flush_pending = false;    // two-level record: the summary row of the last step enqueued is still to be written
                                   // (k_flush2 on demand)
    // SMC_FLAG_SQMC (smc_filter_sqmc.h): the point stream, the tape of ndtri(second coordinate), the
    // sort's workspace and -- more than one island -- the islands' permutations
    u64 sq_seed = 0, sq_ctr0 = 1;
    // plan.lazy_lw: the time indices enqueued with a.lw_lazy set whose decisions smc_filter_lazy_lw_steps has not looked
    // up yet, and the count of those it has found resampled (= launched without the lw store)
    std::vector<i64> lazy_pending;
    i64 lazy_elided = 0;
    double* sq_z = nullptr;
    u64* sq_perm = nullptr;
    void* sq_ws = nullptr;
    i64 perm_t = -1;       // t_host at the last smc_filter_permute_islands (A / Xp undefined there)
    hipGraphExec_t gexec[3] = {nullptr, nullptr, nullptr};   // captured step sequences of F_GRAPH_SIZES steps (even: see
                                                             // enqueue_step)
    bool graph_failed = false;
    bool prof = false;
    std::vector<hipEvent_t> ev;
    int prof_n = 0;
    double* tmp = nullptr;         // (N,) staging for W / Xp downloads
    double* ll_stage = nullptr;    // (n_islands,) staging for smc_filter_logLt: PINNED host memory the
                                   // collect kernel writes straight into (no copy engine, no staging)
    // SMC^2 theta level (smc_filter_theta_enable): theta log-weights, stop record, ESS log
    double *lwth = nullptr, *th = nullptr, *th_ess = nullptr;
    double th_ess_min = 0.0;
    void* th_buf = nullptr;
    // ... of a population sharded over ranks (smc_filter_theta_enable_sharded): the theta level is
    // replicated -- th_n = nranks x n_islands log-weights on every rank -- and fed by an all-gather of the
    // ranks' evidence increments enqueued behind every step
    smc_comm* th_comm = nullptr;
    int th_n = 0;
    double *th_send = nullptr, *th_recv = nullptr;
    // conditional SMC (smc_filter_set_conditional, smc_csmc.h): the retained trajectories (n_islands, T), caller-owned
    // like the replay tapes; smc_filter_step then runs k_csmc_small.  Not part of a saved state; shared by a clone.
    const double* xstar = nullptr;
};

// ---- from a run-time word to a template argument.  Every launch below that chooses among instantiations of one kernel
// goes through these: the word becomes a type (fn(std::integral_constant<..>{})), the kernel template is named once, and its
// grid, block, stream and arguments are written once.  A combination that does not exist is left out with `if constexpr` in
// the lambda, so it is never instantiated; a word outside the set calls nothing.
// F_VAL(x): the value of such a type by its parameter's name (remove_reference: g++ gives decltype of a parameter that an
// inner lambda captures by reference as T&)
#define F_VAL(x) std::remove_reference_t<decltype(x)>::value
template <class F>
static void f_with_bool(bool b, F&& fn)
{
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}
template <int... VS, class F>
static void f_with_value(int v, F&& fn)
{
    (void)((v == VS ? (fn(std::integral_constant<int, VS>{}), true) : false) || ...);
}
// the one-workgroup kernels (k_filter_small, k_csmc_small, k_csmc_path): one wave up to N = 256
template <class F>
static void f_with_small_block(i64 N, F&& fn)
{
    f_with_value<64, SMC_BLOCK>(N <= 256 ? 64 : SMC_BLOCK, fn);
}
// k_f_spacing_onepass<tiles of draws per workgroup>: launch_spacings launches it, plan_step asks for its occupancy
template <class F>
static void f_with_onepass(int tpw, F&& fn)
{
    f_with_value<1, 2, 4, 8>(tpw, [&](auto v) { fn(k_f_spacing_onepass<F_VAL(v)>); });
}

// The univariate models of the fused filter are named here and nowhere else: the six kinds in f_with_kind, the Feynman-Kac
// kinds each of them runs under in f_pair_ok.  smc_filter_create refuses what f_model_ok does not find, so the launches
// (k_propagate, k_filter_small, k_sq_permute) meet existing pairs only.  No default, as in sm_with_kind.
template <int KIND, int FK>
constexpr bool f_pair_ok()
{
    return FK == SMC_FK_BOOTSTRAP || ((FK == SMC_FK_GUIDED || FK == SMC_FK_APF || FK == SMC_FK_APF_BOOT) &&
                                      (KIND == SMC_MODEL_LINGAUSS || KIND == SMC_MODEL_STOCHVOL));
}
template <class F>
static void f_with_kind(int kind, F&& fn)
{
    switch (kind) {
    case SMC_MODEL_LINGAUSS: fn(std::integral_constant<int, SMC_MODEL_LINGAUSS>{}); break;
    case SMC_MODEL_STOCHVOL: fn(std::integral_constant<int, SMC_MODEL_STOCHVOL>{}); break;
    case SMC_MODEL_GORDON: fn(std::integral_constant<int, SMC_MODEL_GORDON>{}); break;
    case SMC_MODEL_THETALOGISTIC: fn(std::integral_constant<int, SMC_MODEL_THETALOGISTIC>{}); break;
    case SMC_MODEL_SVLEVERAGE: fn(std::integral_constant<int, SMC_MODEL_SVLEVERAGE>{}); break;
    case SMC_MODEL_DISCRETECOX: fn(std::integral_constant<int, SMC_MODEL_DISCRETECOX>{}); break;
    }
}
template <class F>
static void f_with_model(int kind, int fk, F&& fn)
{
    f_with_kind(kind, [&](auto k) {
        f_with_value<SMC_FK_BOOTSTRAP, SMC_FK_GUIDED, SMC_FK_APF, SMC_FK_APF_BOOT>(fk, [&](auto q) {
            if constexpr (f_pair_ok<F_VAL(k), F_VAL(q)>()) fn(k, q);
        });
    });
}
static bool f_kind_ok(int kind)
{
    bool ok = false;
    f_with_kind(kind, [&](auto) { ok = true; });
    return ok;
}
static bool f_model_ok(int kind, int fk)
{
    bool ok = false;
    f_with_model(kind, fk, [&](auto, auto) { ok = true; });
    return ok;
}

// the uniforms of a multinomial step are drawn on the device (no replay tape: smc_filter_set_replay may set one later)
static bool philox_multinomial(const FArgs& a) { return a.scheme == SMC_MULTINOMIAL && !a.ut; }

// SMC_FLAG_SQMC on the flat step: multivariate filters; univariate ones below two tiles
static bool sqmc_on_flat_step(const smc_model* model, const smc_filter_opts* o)
{
    return model->kind == SMC_MODEL_MVLINGAUSS || o->N < 2 * F_TILE;
}

// Fills the plan from the model, the options and the shape words of the argument block (N, n_islands, ntiles,
// nparts, log2N, hist, scheme).  Nothing is allocated yet; the device is current (the occupancy query).
static int plan_step(const smc_ctx* ctx, const smc_model* model, const smc_filter_opts* o, const FArgs& a, StepPlan* out)
{
    const unsigned flags = (unsigned)o->flags;
    const bool mv = model->kind == SMC_MODEL_MVLINGAUSS;
    const bool strict = (flags & SMC_FLAG_STRICT_ANCESTORS) != 0, literal = (flags & SMC_PATH_STRICT_LITERAL) != 0;
    const bool sqmc = (flags & SMC_FLAG_SQMC) != 0;
    const i64 M = a.n_islands;
    StepPlan p;
    p.sq_flat = sqmc && sqmc_on_flat_step(model, o);
    // two-level CDF: closed-form offspring counts (N = 2^k with integers, other N with the general counts; systematic /
    // stratified), at least 2 tiles (below, the one-workgroup filter)
    // (multinomial: the counts are searches over the sorted uniforms -- the tape's, or the exponential
    //  spacings drawn between the reduction, which decides the step, and k_ancestors2)
    p.two_level = !mv && o->N <= ((int64_t)1 << 30) && a.ntiles >= 2 && !(flags & (SMC_PATH_FLAT_CDF | SMC_PATH_FORCE_UNFUSED));
    p.apf2 = !mv && f_is_apf(model->fk) && o->N > F_TILE;
    if (p.apf2 && !p.two_level) {
        smc_set_error("the auxiliary particle filter beyond N = 1024 runs on the two-level step only");
        return SMC_ERR_INVALID;
    }
    if (sqmc && !p.sq_flat && !p.two_level) {
        smc_set_error("SMC_FLAG_SQMC needs the two-level step");
        return SMC_ERR_INVALID;
    }
    p.kind = (sqmc && !p.sq_flat) ? STEP_SQMC : strict ? STEP_STRICT : p.two_level ? STEP_TWO_LEVEL : STEP_FLAT;
    p.strict_form = literal ? STRICT_LITERAL : p.two_level ? STRICT_TWO_LEVEL : STRICT_ARRAY;
    // (published tile totals pay off only while every workgroup of the launch is resident; SMC_PATH_FORCE_UNFUSED
    //  (tests): the k_prepare path at any size)
    const bool resident = (i64)a.ntiles * M <= F_DIRECT_PREFIX_MAX && !(flags & SMC_PATH_FORCE_UNFUSED);
    // every workgroup reduces the partials itself while the launch is resident and an island has
    // at most 1024 tiles (4 per thread); otherwise one workgroup per island does it first
    const bool mid = p.two_level && (!resident || a.ntiles > 1024 || (flags & SMC_PATH_TWO_LEVEL_MID) ||
                                     a.scheme == SMC_MULTINOMIAL || p.apf2);
    if (p.two_level && (mid || (strict && literal))) {
        const int nchunks = (a.nparts + 4 * SMC_BLOCK - 1) / (4 * SMC_BLOCK);
        p.reduce = (nchunks >= 2 && nchunks <= 4 && !p.apf2 && !(flags & SMC_PATH_NO_WIDE)) ? REDUCE_WIDE : REDUCE_NARROW;
    }
    // resident grids: F_WIDE_TPW tiles per workgroup (smc_filter_wide.h) -- N = 2^k with whole pairs of tiles, any other N
    // under the systematic scheme (the general counts: the last workgroup of a run may hold one tile);
    // SMC_PATH_NO_WIDE keeps the one-tile kernel testable at these sizes
    const bool wide = p.kind == STEP_TWO_LEVEL && !mid && !(flags & SMC_PATH_NO_WIDE) &&
                      (a.log2N >= 0 ? a.ntiles % F_WIDE_TPW == 0 : a.scheme == SMC_SYSTEMATIC);
    p.resampler = p.two_level ? (wide ? RS_WIDE : RS_TILE) : (resident ? RS_FUSED : RS_PREPARE);
    // consecutive tiles on one XCD (f_tile_xcd): any number of tiles with one tile per resampling workgroup; with
    // k_ancestors2w whole multiples of 8 x (its tiles per workgroup) -- else the wide kernel keeps its own XCD-strided map
    p.xcd_chunks = p.kind == STEP_TWO_LEVEL && !(flags & SMC_PATH_NO_XCD_CHUNKS) && a.ntiles >= 16 &&
                   (!wide || a.log2N < 0 || a.ntiles % (8 * F_WIDE_TPW) == 0);
    // (measured and kept out, round 4: the reduction MERGED into the resampling launch on grids beyond 2048 workgroups --
    //  (a) every workgroup of k_ancestors2w reducing: C5 99.2 us per step (2 tiles per workgroup) / 117.2 (4) against 92.9
    //  behind k_reduce2 (r12h); (b) workgroup 0 of k_ancestors2 reducing, the others waiting for its word with their
    //  loads in flight and reading (G_b, Q_b) past their L2: C3 60.7 against 57.6 us, C5 159 against 99 -- a dependent
    //  global round trip in every workgroup costs more than the launch it saves (r12j))
    // (SQMC: k_ancestors2 counts in SORTED positions; a heavy parent's blocks would be filled with that index)
    p.heavy_list = !mv && !strict && !sqmc && !(flags & SMC_PATH_NO_HEAVY);
    // (history slots are written step by step: the lanes beyond N of a slot would read indices nobody
    //  initialised -- every access tests its index there as well)
    p.ragged = (p.two_level && (o->N % F_TILE) != 0) ? (((o->N & 1) || a.hist) ? 2 : 1) : 0;
    // one-pass uniform_spacings (two-level record, Philox draws): 1, 2, 4 or 8 tiles of draws per workgroup,
    // the fewest that keep the whole launch resident (<= 1024 workgroups: half of what the chip holds);
    // more islands than that: the three-pass form
    bool merge_fits = false;
    if (a.scheme == SMC_MULTINOMIAL && p.two_level && !(strict && literal) && !sqmc && !(flags & SMC_PATH_SPACING_3PASS))
        for (int tpw = 1; tpw <= 8 && !p.sp_tpw; tpw *= 2) {
            const int forced_tpw = (o->flags >> 25) & 15;          // SMC_PATH_SP_TPW (A/B: workgroups wait for
            if (forced_tpw && tpw != forced_tpw) continue;         //  lower-numbered ones only, dispatch is in order)
            const i64 nwg = (a.ntiles + tpw - 1) / tpw;
#ifdef SMC_EMULATE
            const i64 cap = 1024, cap_merged = ((i64)1 << 62);     // (workgroups run one after the other, in order)
            (void)ctx;
#else
            int per_cu = 0;                        // workgroups of this instantiation a CU holds at once
            const void* fn = nullptr;
            f_with_onepass(tpw, [&](auto kernel) { fn = (const void*)kernel; });
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, SMC_BLOCK, 0) != hipSuccess) per_cu = 0;
            (void)hipGetLastError();
            // (a margin of one workgroup per CU: the occupancy API is optimistic near register-file edges)
            const i64 cap = (i64)(per_cu > 1 ? per_cu - 1 : 0) * ctx->n_cu, cap_merged = (i64)per_cu * ctx->n_cu;
#endif
            if ((nwg * M <= cap && nwg * M <= 1024) || (forced_tpw && nwg <= 1024)) {
                p.sp_tpw = tpw;
                p.sp_nwg = (int)nwg;
                // one workgroup more per island when the reduction rides along: it is the first of the launch and
                // waits for nobody, the others wait for lower-numbered ones only -- dispatch is in order, so the
                // margin kept above is not needed for it, the chip's nominal capacity is
                merge_fits = (nwg + 1) * M <= cap_merged || forced_tpw;
            }
        }
    // (inside a replayed graph the argument block -- the epoch with it -- is frozen: separate launches there)
    const bool merge = p.sp_tpw && merge_fits && !o->use_graph && !(flags & SMC_PATH_SPLIT_REDUCE);
    p.spacings = (a.scheme != SMC_MULTINOMIAL || sqmc) ? SP_NONE
                 : p.sp_tpw ? (merge ? SP_ONEPASS_MERGED : SP_ONEPASS)
                 : strict ? SP_PER_ISLAND : SP_THREE_PASS;
    p.small = o->N <= F_TILE && !mv && !o->moments && !strict && !sqmc && !(flags & SMC_PATH_NO_SMALL);
    // bootstrap filters whose weight depends on the new particle only: the sorted weights are recomputed
    // from the sorted keys; SMC_PATH_SQ_GATHER (A/B) and the others gather them
    // (one island, N beyond the one-workgroup sort: the workspace then holds the key images of that island)
    p.sq_recompute = model->fk == SMC_FK_BOOTSTRAP && model->kind != SMC_MODEL_SVLEVERAGE && !(flags & SMC_PATH_SQ_GATHER) &&
                     a.n_islands == 1 && a.N > 2048;
    p.mv_collapsed = mv && model->fk == SMC_FK_GUIDED && (flags & SMC_FLAG_COLLAPSED_PROPOSAL);
    p.no_tk = (flags & SMC_PATH_NO_TK) != 0;
    p.lazy_lw = p.kind == STEP_TWO_LEVEL && a.hist == 0 && !o->moments && !o->use_graph &&
                model->fk == SMC_FK_BOOTSTRAP && model->kind != SMC_MODEL_SVLEVERAGE && !mv && !(flags & SMC_PATH_EAGER_LW);
    *out = p;
    return SMC_OK;
}

// the island's reduction as a launch of its own (plan.reduce)
static void launch_reduce2(smc_filter* f, hipStream_t st)
{
    if (f->plan.reduce == REDUCE_WIDE)
        SMC_LAUNCH(k_reduce2w, dim3(f->a.n_islands), dim3(4 * SMC_BLOCK), st, f->a);
    else
        SMC_LAUNCH(k_reduce2, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
}

static void launch_propagate(smc_filter* f)
{
    hipStream_t st = f->ctx->stream;
    const dim3 grid(f->a.nparts, f->a.n_islands);
    if (f->kind == SMC_MODEL_MVLINGAUSS) {
        // fk, dp, dx == dp, the collapsed proposal (guided only), diagonal covariances
        f_with_value<SMC_FK_BOOTSTRAP, SMC_FK_GUIDED, SMC_FK_APF>(f->fk, [&](auto q) {
            f_with_value<16, 32>(f->a.dp, [&](auto dp) {
                f_with_bool(f->a.dx == f->a.dp, [&](auto dfull) {
                    f_with_bool(f->plan.mv_collapsed, [&](auto coll) {
                        f_with_bool(f->a.mv_diag != 0, [&](auto dg) {
                            constexpr int FK = F_VAL(q), DP = F_VAL(dp);
                            constexpr bool DFULL = F_VAL(dfull), COLL = F_VAL(coll), DG = F_VAL(dg);
                            if constexpr (!COLL || FK == SMC_FK_GUIDED)
                                SMC_LAUNCH((k_propagate_mv<FK, DP, DFULL, COLL, DG>), grid, dim3(SMC_BLOCK), st, f->a, f->a.mvc);
                        });
                    });
                });
            });
        });
        return;
    }
    // the record's shape: -1 the flat step (k_propagate's tail), else tail-free with the plan's RAGGED
    const int shape = f->plan.two_level ? f->plan.ragged : -1;
    f_with_model(f->kind, f->fk, [&](auto k, auto q) {      // (APF: tail-free two-level launches only: create checks)
        f_with_bool(f->a.par >= 0, [&](auto spec) {
            f_with_value<-1, 0, 1, 2>(shape, [&](auto sh) {
                constexpr int SH = F_VAL(sh);
                // (the leading arguments: the fields the kernel's first loads are addressed with, preloaded into SGPRs)
                SMC_LAUNCH((k_propagate<F_VAL(k), F_VAL(q), F_OPT, F_VAL(spec), (SH < 0), (SH < 0 ? 0 : SH)>), grid,
                           dim3(SMC_BLOCK), st, f->a.A, f->a.info, f->a.params, f->a.hcnt, f->a.N,
                           f->a.ntiles | (f->a.xcd_chunks ? 1 << 30 : 0), f->a);
            });
        });
    });
}

// uniform_spacings for the Philox draws of a multinomial step, in the plan's form; merge: the island's reduction is
// workgroup 0 of the one-pass launch
static void launch_spacings(smc_filter* f, hipStream_t st, bool merge)
{
    const FArgs& a = f->a;
    const dim3 g1(a.ntiles1, a.n_islands);
    switch (f->plan.spacings) {
    case SP_ONEPASS:
    case SP_ONEPASS_MERGED: {          // decoupled look-back: every workgroup resident
        const dim3 gw(a.sp_nwg + (merge ? 1 : 0), a.n_islands);
        f_with_onepass(a.sp_tpw, [&](auto kernel) { SMC_LAUNCH(kernel, gw, dim3(SMC_BLOCK), st, a); });
        break;
    }
    case SP_THREE_PASS:                // two passes over the same draws (tile sums, their prefixes, the uniforms written once)
        SMC_LAUNCH(k_f_spacing_sums, g1, dim3(SMC_BLOCK), st, a);
        SMC_LAUNCH(k_f_spacing_scan, dim3(a.n_islands), dim3(SMC_BLOCK), st, a);
        SMC_LAUNCH(k_f_spacing_write, g1, dim3(SMC_BLOCK), st, a);
        break;
    case SP_PER_ISLAND:                // (the strict literal walk and one-tile strict filters)
        for (int i = 0; i < a.n_islands; ++i)
            SMC_LAUNCH(k_f_spacings_step, dim3(1), dim3(SMC_BLOCK), st, a, i, a.su + (size_t)i * a.N);
        break;
    case SP_NONE: break;
    }
}

// the step's sorted uniforms are drawn on the device: multinomial scheme, Philox mode, no replay tape set since
static bool draws_spacings(const smc_filter* f) { return f->plan.spacings != SP_NONE && !f->a.ut; }

// what opens a two-level or strict step: the island's reduction (decision + normalisation of step t-1) and the
// spacings -- the reduction as a launch of its own, or as workgroup 0 of the one-pass spacings kernel
static void open_step(smc_filter* f, hipStream_t st, bool t_known)
{
    const bool draws = draws_spacings(f);
    const bool merge = draws && f->plan.spacings == SP_ONEPASS_MERGED && t_known;
    f->a.sp_epoch = merge ? ++f->sp_epoch : 0ull;
    if (f->plan.reduce != REDUCE_NONE && !merge) launch_reduce2(f, st);
    if (draws) launch_spacings(f, st, merge);
}

// STEP_SQMC (smc_filter_sqmc.h).  The step's normals come from a tape that is ONE step's buffer (zt_ts = 0),
// written by k_sq_init / k_sq_permute just before; the thresholds are a function of n (f2_sq_T)
static void resample_sqmc(smc_filter* f, hipStream_t st, i64 t, bool t_known)
{
    FArgs& a = f->a;
    const dim3 grid(a.ntiles, a.n_islands);
    a.zt = f->sq_z;
    a.zt_ts = 0;
    a.sq_seed = f->sq_seed;
    a.sq_ctr = f->sq_ctr0;
    // (inside a captured graph only the parity of t is static: replays start at t >= 2, see smc_filter_step)
    if (t_known && t == 0) {
        SMC_LAUNCH(k_sq_init, dim3((unsigned)((a.N + SMC_BLOCK - 1) / SMC_BLOCK), a.n_islands), dim3(SMC_BLOCK), st,
                   f->a, f->sq_z, f->sq_seed, f->sq_ctr0);
        return;
    }
    const bool recompute = f->plan.sq_recompute;
    const u64 *perm = f->sq_perm, *skeys = nullptr;
    for (int i = 0; i < a.n_islands; ++i) {        // h_order = argsort(X_{t-1}) (hilbert.py:52-54, d = 1)
        u64 *k0 = nullptr, *v0 = nullptr;
        (void)smc_rs_sort_ws(f->ctx, f_X(a, t - 1) + (i64)i * a.N, nullptr, a.N, 0, f->sq_ws, recompute ? &k0 : nullptr, &v0, f->sq_plan_zero);
        f->sq_plan_zero = true;               // (every sort leaves its plan words zeroed for the next)
        if (a.n_islands == 1) { perm = v0; skeys = k0; }
        else (void)hipMemcpyAsync(f->sq_perm + (i64)i * a.N, v0, (size_t)a.N * 8, hipMemcpyDeviceToDevice, st);
    }
    f_with_kind(f->kind, [&](auto k) {
        f_with_bool(recompute, [&](auto rc) {
            SMC_LAUNCH((k_sq_permute<F_VAL(k), F_VAL(rc)>), grid, dim3(SMC_BLOCK), st, f->a, perm, skeys,
                       f->sq_z, f->sq_seed, f->sq_ctr0);
        });
    });
    launch_reduce2(f, st);
    f->a.sq_perm = perm;                     // (A = h_order[sorted position]: composed where the ancestors are stored)
    SMC_LAUNCH((k_ancestors2<true, true, true, false, true>), grid, dim3(SMC_BLOCK), st, f->a);
}

// STEP_STRICT: the sequential CDF of W_{t-1} and the searches, behind open_step (flat record: k_propagate's tail
// decided and normalised)
static void resample_strict(smc_filter* f, hipStream_t st, bool t_known)
{
    open_step(f, st, t_known);
    const unsigned nb = (unsigned)((f->a.N + 1023) / 1024);
    const dim3 gt(nb, f->a.n_islands);
    const dim3 gs((unsigned)((f->a.N / 2 + SMC_BLOCK) / SMC_BLOCK), f->a.n_islands);
    // (strict_ws: (n_islands, N) W | (n_islands, N) S | the scratch of smc_seqx.h | (n_islands, ntiles) tile sums)
    double* S = f->strict_ws + (size_t)f->a.n_islands * f->a.N;
    void* sqx_scr = (void*)(S + (size_t)f->a.n_islands * f->a.N);
    SqxArgs q = sqx_carve(sqx_scr, f->a.N, f->a.n_islands);
#ifdef SMC_TRACE
    q.trace = f->a.trace + (size_t)f->a.n_islands * (f->a.nparts + f->a.ntiles) * 8;
#endif
    const SeqGate gate{f->a.info, INFO_STRIDE, f->a.T, nullptr};
    switch (f->plan.strict_form) {
    case STRICT_LITERAL:
        // the definition: W written out, ONE lane adding it up in place (44 ms at N = 2^20), a search per offspring
        SMC_LAUNCH(k_strict_W, gt, dim3(SMC_BLOCK), st, f->a, f->strict_ws, (double*)nullptr);
        SMC_LAUNCH(k_strict_cdf, dim3(1, f->a.n_islands), dim3(64), st, f->a, f->strict_ws);
        SMC_LAUNCH(k_strict_search_S, gs, dim3(SMC_BLOCK), st, f->a, (const double*)f->strict_ws, (const double*)f->a.su);
        break;
    case STRICT_TWO_LEVEL:
        // the same doubles in two launches, S never written (smc_filter_strict.h)
        f_with_bool(f->plan.reduce != REDUCE_NONE,
                    [&](auto mid) { SMC_LAUNCH(k_strict_classify<F_VAL(mid)>, gt, dim3(SMC_BLOCK), st, f->a, q); });
        SMC_LAUNCH(k_strict_search, gt, dim3(SMC_BLOCK), st, f->a, q);
        break;
    case STRICT_ARRAY: {
        // one tile (or a flat test path): W materialised, the two launches of smc_seqx.h on the array, S written
        size_t used = 0;
        (void)sqx_carve(sqx_scr, f->a.N, f->a.n_islands, &used);
        double* tsum = (double*)((char*)sqx_scr + used);
        SMC_LAUNCH(k_strict_W, gt, dim3(SMC_BLOCK), st, f->a, f->strict_ws, tsum);
        SMC_LAUNCH(k_sqx_classify, gt, dim3(SMC_BLOCK), st, (const double*)f->strict_ws, (const double*)tsum, q, gate);
        SMC_LAUNCH(k_sqx_fill, gt, dim3(SMC_BLOCK), st, q, S, gate);
        SMC_LAUNCH(k_strict_search_S, gs, dim3(SMC_BLOCK), st, f->a, (const double*)S, (const double*)f->a.su);
        break;
    }
    }
}

// STEP_TWO_LEVEL: k_ancestors2 / k_ancestors2w behind open_step
static void resample_two_level(smc_filter* f, hipStream_t st, bool t_known)
{
    open_step(f, st, t_known);
    const dim3 grid(f->a.ntiles, f->a.n_islands);
    if (f->a.scheme == SMC_MULTINOMIAL) {
        // searches over the sorted uniforms: the spacings just drawn (k_ancestors2 finds its window through the
        // tile prefixes) or the tape's
        f_with_bool(!f->a.ut, [&](auto regen) {
            SMC_LAUNCH((k_ancestors2<true, true, true, F_VAL(regen)>), grid, dim3(SMC_BLOCK), st, f->a);
        });
        return;
    }
    // closed-form counts: one instantiation per scheme (see k_ancestors2's SCH); a launch of its own has reduced the
    // island (MID), or the resampling workgroups do: one tile each, or F_WIDE_TPW tiles (k_ancestors2w)
    const bool sys = f->a.scheme == SMC_SYSTEMATIC, p2 = f->a.log2N >= 0, mid = f->plan.reduce != REDUCE_NONE;
    const bool wide = !mid && f->plan.resampler == RS_WIDE;
    // k_ancestors2w's grid.  N = 2^k: the partials reduced by the workgroup's first 4 waves only; any N, systematic: the
    // runs of tiles f_tile_xcd gives the XCDs, two tiles per workgroup
    const int per_run = (f->a.ntiles + 7) / 8;
    const dim3 gridw(p2 ? f->a.ntiles / F_WIDE_TPW : f->a.xcd_chunks ? 8 * ((per_run + 1) / 2) : (f->a.ntiles + 1) / 2,
                     f->a.n_islands);
    f_with_bool(sys, [&](auto s) {
        f_with_bool(p2, [&](auto p) {
            constexpr int SCH = F_VAL(s) ? SMC_SYSTEMATIC_ : SMC_STRATIFIED_;
            constexpr bool POW2 = F_VAL(p);
#ifdef SMC_NO_SCHEME_SPLIT                         /* (A/B builds: tools/build_ablations.sh) */
            constexpr int SCH_A2 = 0;
#else
            constexpr int SCH_A2 = SCH;
#endif
            if (!wide) {
                f_with_bool(mid, [&](auto m) {
                    SMC_LAUNCH((k_ancestors2<F_VAL(m), false, POW2, false, false, SCH_A2>), grid, dim3(SMC_BLOCK), st, f->a);
                });
            } else if constexpr (POW2 || SCH == SMC_SYSTEMATIC_) {
                // (leading arguments: the fields the kernel's first loads are addressed with, preloaded into SGPRs)
                SMC_LAUNCH((k_ancestors2w<F_WIDE_TPW, SCH, POW2>), gridw, dim3(SMC_BLOCK * 2), st, f->a.info2, f->a.pm, f->a.ps,
                           f->a.pss, f->a.cq, f->a.N, f->a.ntiles | (f->a.xcd_chunks ? 1 << 30 : 0), f->a);
            }
        });
    });
}

// sq_flat: SQMC of a multivariate filter, or of a univariate one of fewer than two tiles (smc_filter_sqmc.h):
// Hilbert order (d = 1: the radix argsort), the step's points, the tapes; the flat step then runs as it
// is -- its multinomial search over the sorted uniforms in a.su, its propagate kernel fed from the tape
// of ndtri values
static void sqmc_flat_prologue(smc_filter* f, hipStream_t st, i64 t)
{
    FArgs& a = f->a;
    const int d = a.dx;
    const unsigned nb = (unsigned)((a.N + SMC_BLOCK - 1) / SMC_BLOCK);
    double* U = (double*)f->sq_ws;
    double* lws = U + (size_t)a.N * (d + 1);
    a.zt = f->sq_z;
    a.zt_ts = 0;
    for (int i = 0; i < a.n_islands; ++i) {
        const u64 ctr = f->sq_ctr0 + (u64)t + ((u64)(u32)(a.island_offset + i) << 32);
        if (t == 0) {
            (void)smc_sobol_points(f->ctx, f->sq_seed, a.N, d, ctr, 0, U);
            SMC_LAUNCH(k_sqmv_tapes, dim3(nb), dim3(SMC_BLOCK), st, f->a, i, (const i64*)nullptr, (const double*)U, d,
                       lws, f->sq_z);
        } else {
            i64* perm = (i64*)f->sq_perm + (size_t)i * a.N;
            if (d == 1) {                      // hilbert.py:52-54: argsort
                u64* v0 = nullptr;
                (void)smc_rs_sort_ws(f->ctx, f_X(a, t - 1) + (size_t)i * a.N, nullptr, a.N, 0, (void*)(lws + a.N), nullptr, &v0, f->sq_plan_zero);
                f->sq_plan_zero = true;
                (void)hipMemcpyAsync(perm, v0, (size_t)a.N * 8, hipMemcpyDeviceToDevice, st);
            } else {
                (void)smc_hilbert_sort(f->ctx, f_X(a, t - 1) + (size_t)i * a.N * d, a.N, d, (int64_t*)perm, nullptr);
            }
            (void)smc_sobol_points(f->ctx, f->sq_seed, a.N, d + 1, ctr, 1, U);
            SMC_LAUNCH(k_sqmv_tapes, dim3(nb), dim3(SMC_BLOCK), st, f->a, i, (const i64*)perm, (const double*)U, d + 1,
                       lws, f->sq_z);
            (void)hipMemcpyAsync(f_lw(a, t - 1) + (size_t)i * a.N, lws, (size_t)a.N * 8, hipMemcpyDeviceToDevice, st);
        }
    }
}

// STEP_FLAT: [k_prepare, (spacings), k_ancestors] do nothing unless the step resamples (decided on the device by
// the previous k_propagate)
static void resample_flat(smc_filter* f, hipStream_t st, i64 t)
{
    const dim3 grid(f->a.ntiles, f->a.n_islands);
    if (f->plan.sq_flat) sqmc_flat_prologue(f, st, t);
    if (f->kind == SMC_MODEL_MVLINGAUSS && f->fk == SMC_FK_APF) {
        // auxiliary weights of step t (core.py:307-313) before its resampling: smc_filter_mv.h
        const dim3 gp(f->a.nparts, f->a.n_islands);
        auto go = [&](auto kernel) { SMC_LAUNCH(kernel, gp, dim3(SMC_BLOCK), st, f->a, f->a.mvc); };
        f_with_value<16, 32>(f->a.dp, [&](auto dp) {
            f_with_bool(f->a.dx == f->a.dp, [&](auto dfull) { go(k_mv_aux<F_VAL(dp), F_VAL(dfull)>); });
        });
        SMC_LAUNCH(k_mv_aux_restate, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
    }
    const bool fused = f->plan.resampler == RS_FUSED;
    if (!fused) SMC_LAUNCH(k_prepare, grid, dim3(SMC_BLOCK), st, f->a);
    if (draws_spacings(f)) launch_spacings(f, st, false);
    // 0: behind k_prepare; 1: fused; 2: fused and SPEC (the slot parity is known) -- SPEC exists with the fused form only
    f_with_value<0, 1, 2>(!fused ? 0 : f->a.par < 0 ? 1 : 2, [&](auto v) {
        SMC_LAUNCH((k_ancestors<(F_VAL(v) >= 1), (F_VAL(v) == 2)>), grid, dim3(SMC_BLOCK), st, f->a);
    });
    if (f->plan.sq_flat && t > 0)                  // A <- h_order[A] (core.py:344)
        for (int i = 0; i < f->a.n_islands; ++i)
            SMC_LAUNCH(k_sqmv_compose, dim3((unsigned)((f->a.N + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, f->a, i,
                       (const i64*)f->sq_perm + (size_t)i * f->a.N);
}

// one time step: the resampling part of the plan's kind, then k_propagate and the moments
// lazy: the caller enqueues another step behind this one before it returns to ITS caller (plan.lazy_lw then lets
// k_propagate leave a resampling step's log-weights unwritten)
static void enqueue_step(smc_filter* f, int k_prof, i64 t, bool t_known = true, bool lazy = false)
{
    f->a.lw_prev_lazy = f->a.lw_lazy;               // (0 behind the last step of a call, a captured step, a theta step)
    f->a.lw_lazy = (lazy && t_known && f->plan.lazy_lw && !f->lwth) ? 1 : 0;
    if (f->a.lw_lazy) f->lazy_pending.push_back(t);
    // the host knows the time index of every step it enqueues; inside a replayed graph
    // only its parity is static (graphs hold an even number of steps and start at even t)
    f->a.par = f->a.hist ? -1 : (int)(t & 1);
    f->a.tk = (t_known && !f->plan.no_tk) ? t : -1;
    hipStream_t st = f->ctx->stream;
    if (k_prof >= 0) (void)hipEventRecord(f->ev[3 * k_prof], st);
    switch (f->plan.kind) {
    case STEP_SQMC: resample_sqmc(f, st, t, t_known); break;
    case STEP_STRICT: resample_strict(f, st, t_known); break;
    case STEP_TWO_LEVEL: resample_two_level(f, st, t_known); break;
    case STEP_FLAT: resample_flat(f, st, t); break;
    }
    // samples come in three kinds (k mod 3): 0 times the whole step, 1 the interval [start,
    // resampling kernels done], 2 the interval [resampling kernels done, end].  Every event
    // interval carries the same ~4 us of marker processing on MI355X (tools/micro/events.hip),
    // which cancels in propagate = whole - first part, resampling = whole - second part: both
    // kernels are MEASURED (smc_filter_kernel_ms), neither is derived from the step time.
    if (k_prof >= 0 && (k_prof % 3)) (void)hipEventRecord(f->ev[3 * k_prof + 1], st);
    launch_propagate(f);
    if (k_prof >= 0) (void)hipEventRecord(f->ev[3 * k_prof + 2], st);
    if (f->a.mom) {      // device-side Moments; two-level record: the row of the step just done (K, 1/s) first
        if (f->plan.two_level) SMC_LAUNCH(k_flush2, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
        SMC_LAUNCH(k_f_moments_partials, dim3(f->a.nmb, f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
        SMC_LAUNCH(k_f_moments_final, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
    }
}


// ---- smc_filter_create in stages: validate (in the entry itself: its messages carry its name), shape, plan_step,
// slab_layout, allocation, fill_filter; nothing is allocated before the layout is known

// what validation works out about a MVLINGAUSS model
struct MvSetup {
    int dx = 1, dy = 1, dp = 1;
    std::vector<double> mvc_host;
    bool diag = false;
};

// the shape words of the argument block: sizes, grids, scheme
static void shape_args(FArgs& a, const smc_model* model, const smc_filter_opts* o, const MvSetup& m)
{
    const bool mv = model->kind == SMC_MODEL_MVLINGAUSS;
    const bool sqmc = (o->flags & SMC_FLAG_SQMC) != 0;
    memset(&a, 0, sizeof a);
    a.N = o->N;
    a.T = o->T;
    a.n_islands = o->n_islands;
    a.ntiles = (int)((o->N + F_TILE - 1) / F_TILE);
    a.ntiles1 = (int)((o->N + 1 + F_TILE - 1) / F_TILE);
    a.scheme = sqmc ? (int)SMC_MULTINOMIAL : (int)o->scheme;            // (sorted uniforms from a tape)
    a.rng_mode = o->rng_mode;
    a.island_offset = o->island_offset;
    a.ess_thresh = sqmc ? INFINITY : (double)o->N * o->ESSrmin;         // (SQMC always resamples, core.py:340)
    a.seed = o->seed;
    a.log2N = -1;
    for (int k = 0; k < 62; ++k)
        if (((i64)1 << k) == o->N) a.log2N = k;
    {
        int lg = 0;
        while (((i64)1 << lg) < o->N + 2) ++lg;
        a.spacing_scale = ldexp(1.0, 57 - lg < 21 ? 57 - lg : 21);        // (see smc_ops.hip spacing_scale)
    }
    a.dx = m.dx; a.dy = m.dy; a.dp = m.dp;
    a.hist = o->keep_history;                      // 0 / 1 (whole history) / k >= 2 (rolling window)
    if (a.hist >= 2 && (i64)a.hist >= a.T) a.hist = 1;       // a window as long as the run: all of it
    a.xslot = a.N * a.n_islands * m.dx;
    a.lslot = a.N * a.n_islands;
    // MV: a workgroup stages the step's matrices in LDS once and then walks
    // mv_chunks chunks of 256 particles (2 workgroups per CU when N allows)
    a.mv_chunks = 1;
    a.mv_diag = (mv && m.diag && !(o->flags & SMC_PATH_MV_DENSE)) ? 1 : 0;
    if (mv) {
        // 8 by default, halved until the grid has at least 512 workgroups (element-wise form: 2 workgroups per CU) or
        // 1024 (dense form: 3 per CU fit); SMC_PATH_MV_CHUNKS(1|2|4|8) (tests) is taken as given, so that the
        // multi-chunk prefetch loop is audited at small N too
        const int forced = (o->flags >> 20) & 15;
        if (forced == 1 || forced == 2 || forced == 4 || forced == 8) a.mv_chunks = forced;
        else {
            const i64 min_grid = a.mv_diag ? 512 : 1024;
            a.mv_chunks = 8;
            while (a.mv_chunks > 1 && a.N / (SMC_BLOCK * a.mv_chunks) < min_grid) a.mv_chunks >>= 1;
        }
    }
    const i64 per_wg = mv ? (i64)SMC_BLOCK * a.mv_chunks : (i64)SMC_BLOCK * F_OPT;
    a.nparts = (int)((o->N + per_wg - 1) / per_wg);
    a.ncq = (i64)a.ntiles * F_TILE;
    a.nmb = (int)((o->N + F_MOM_CHUNK - 1) / F_MOM_CHUNK);
    a.exact_counts = (o->flags & SMC_PATH_EXACT_COUNTS) ? 1 : 0;
    a.tk = -1;
    // streaming stores pay while a launch is short (its end-of-kernel write-back shows): C2 +8 %;
    // on the large grids they cost 2 % (C5)
    a.nt = ((i64)a.ntiles * a.n_islands <= F_DIRECT_PREFIX_MAX && !mv) ? 15 : 0;
    // (bits: 1 X, 2 lw, 4 the tile CDF, 8 A.  Measured at C2, r12f: any mask that streams lw -- written every step, read
    //  only on the steps that do not resample -- is as fast as streaming everything, 17.63 us; none: 19.31.  With
    //  consecutive tiles per XCD, r12w: 15: 17.4, X plain 17.5, X and the tile CDF plain 18.0, lw only 18.3)
}

// Offsets of every device array in the slab.  The order and the sizes are part of the saved-state format
// (smc_filter_save_state / load_state / clone go by slab_bytes): do not reorder.
struct SlabLayout {
    size_t X, lw, A, Q, Qpre, pm, ps, pss, summ, params, y, aux, mvc, cnt, spart, info, info2, cq, tq, p2, hcnt, hlist, su, E,
        sst, sdec, tmp, strict_ws, eta, sq_z, sq_perm, sq_ws, mom, mpart, trace, bytes;
};

static SlabLayout slab_layout(const FArgs& a, const StepPlan& p, const smc_model* model, const smc_filter_opts* o, size_t mvc_words)
{
    const bool mv = model->kind == SMC_MODEL_MVLINGAUSS;
    const size_t M = (size_t)a.n_islands, N = (size_t)a.N, T = (size_t)a.T, dx = (size_t)a.dx;
    const bool need_su = a.scheme == SMC_MULTINOMIAL;
    const size_t nslots = a.hist == 1 ? T : (a.hist >= 2 ? (size_t)a.hist : 2);
    SlabLayout L;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o0 = off; off = smc_align_up(off + bytes, 256); return o0; };
    // (+ one tile of padding each: the ragged last tile's loads are unconditional, k_propagate<RAGGED = 1>)
    L.X = carve(nslots * M * N * dx * 8 + F_TILE * dx * 8);
    L.lw = carve(nslots * M * N * 8 + F_TILE * 8);
    L.A = carve(((a.hist ? nslots : 1) * M * N + F_TILE) * 4);
    L.Q = carve(M * a.ntiles * 8);
    L.Qpre = carve(M * a.ntiles * 8);
    L.pm = carve(M * a.nparts * 8);
    L.ps = carve(M * a.nparts * 8);
    L.pss = carve(M * a.nparts * 8);
    L.summ = carve(M * (T + 1) * SUMM_STRIDE * 8);
    L.params = carve(M * PARAM_STRIDE * 8);
    L.y = carve(T * a.dy * 8);
    L.aux = carve(T * 8);
    L.mvc = carve(mvc_words * 8 + 8);
    L.cnt = carve(M * 2 * F_CNT_WORDS * sizeof(unsigned));
    L.spart = carve(M * 96 * 8);
    L.info = carve(M * INFO_STRIDE * 8);
    L.info2 = carve(M * INFO_STRIDE * 8);
    L.cq = carve(p.two_level ? M * (size_t)a.ncq * 8 : 8);
    L.tq = carve(p.two_level ? M * a.ntiles * 8 : 8);
    L.p2 = carve(p.apf2 ? 3 * M * a.nparts * 8 : 8);
    L.hcnt = carve(p.heavy_list ? M * 2 * sizeof(unsigned) : 8);
    L.hlist = carve(p.heavy_list ? M * 2 * F_HMAX * 3 * 8 : 8);
    L.su = carve(need_su ? M * N * 8 + 16 : 8);
    L.E = carve(need_su ? M * (a.ntiles1 + 1) * 8 : 8);
    L.sst = carve(p.sp_tpw ? M * p.sp_nwg * 8 : 8);
    L.sdec = carve(M * 8);
    L.tmp = carve(N * dx * 8);
    L.strict_ws = carve(p.strict() ? 2 * M * N * 8 + sqx_scratch_bytes((i64)N, (int)M) + M * a.ntiles * 8 + 64 : 8);
    L.eta = carve(mv && model->fk == SMC_FK_APF ? 2 * M * N * 8 : 8);
    L.sq_z = carve(p.sqmc() ? M * N * dx * 8 : 8);
    L.sq_perm = carve(p.sqmc() && (M > 1 || p.sq_flat) ? M * N * 8 : 8);
    // (two-level: the sort's workspace; flat: the step's points (N, d + 1), a row of sorted log-weights and -- d = 1
    // -- the sort's workspace behind them)
    L.sq_ws = carve(!p.sqmc() ? 8 : p.sq_flat ? (N * (dx + 1) + N) * 8 + (mv ? 0 : smc_rs_ws_bytes((i64)N))
                                               : smc_rs_ws_bytes((i64)N));
    L.mom = carve(o->moments ? M * T * 2 * dx * 8 : 8);
    L.mpart = carve(o->moments ? M * a.nmb * dx * 3 * 8 : 8);
    L.trace = carve(M * (size_t)(2 * a.ntiles + 8) * 8 * 8 + (size_t)(2 * a.ntiles + 16) * 8 * 8);
    L.bytes = off;
    return L;
}

// points the argument block into the slab, zeroes what the kernels expect zero and uploads the model and the data
static int fill_filter(smc_filter* f, const SlabLayout& L, const smc_model* model, const smc_filter_opts* o, const double* y_host,
                       const MvSetup& m)
{
    smc_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    FArgs& a = f->a;
    const StepPlan& p = f->plan;
    const bool mv = f->kind == SMC_MODEL_MVLINGAUSS;
    const size_t M = (size_t)a.n_islands, N = (size_t)a.N, T = (size_t)a.T;
    char* base = (char*)f->slab;
    a.X = (double*)(base + L.X);
    a.lw = (double*)(base + L.lw);
    a.A = (u32*)(base + L.A);
    a.Q = (u64*)(base + L.Q);
    a.Qpre = (u64*)(base + L.Qpre);
    a.pm = (double*)(base + L.pm); a.ps = (double*)(base + L.ps); a.pss = (double*)(base + L.pss);
    a.summ = (double*)(base + L.summ);
    double* dpar = (double*)(base + L.params);
    double* dy = (double*)(base + L.y);
    a.params = dpar;
    a.y = dy;
    a.cnt = (unsigned*)(base + L.cnt);
    a.cq = (u64*)(base + L.cq);
    a.tq = (u64*)(base + L.tq);
    a.spart = (double*)(base + L.spart);
    a.info = (double*)(base + L.info);
    a.info2 = (double*)(base + L.info2);
    if (p.heavy_list) {
        a.hcnt = (unsigned*)(base + L.hcnt);
        a.hlist = (i64*)(base + L.hlist);
        SMC_HIP_CHECK(hipMemsetAsync(a.hcnt, 0, M * 2 * sizeof(unsigned), st));
    }
    if (p.apf2) {
        a.pm2 = (double*)(base + L.p2);
        a.ps2 = a.pm2 + M * a.nparts;
        a.pss2 = a.ps2 + M * a.nparts;
    }
    a.su = (double*)(base + L.su);
    a.E = (u64*)(base + L.E);
    a.sst = (u64*)(base + L.sst);
    if (a.sp_tpw) SMC_HIP_CHECK(hipMemsetAsync(a.sst, 0, M * a.sp_nwg * 8, st));
    a.sdec = (u64*)(base + L.sdec);
    SMC_HIP_CHECK(hipMemsetAsync(a.sdec, 0, M * 8, st));
    f->tmp = (double*)(base + L.tmp);
    f->strict_ws = (double*)(base + L.strict_ws);
    if (p.strict())        // (the counters of smc_seqx.h: zero once, re-armed by its passes)
        sqx_zero_counters(st, (void*)(f->strict_ws + 2 * M * N), (i64)N, (int)M);
    if (mv && f->fk == SMC_FK_APF) {
        a.eta = (double*)(base + L.eta);
        a.lwsv = a.eta + M * N;
    }
    if (p.sqmc()) {
        f->sq_z = (double*)(base + L.sq_z);
        f->sq_perm = (u64*)(base + L.sq_perm);
        f->sq_ws = base + L.sq_ws;
    }
    {
        auto it = ctx->pinned.find(M * 8);
        if (it != ctx->pinned.end() && !it->second.empty()) {
            f->ll_stage = (double*)it->second.back();
            it->second.pop_back();
        } else if (hipHostMalloc((void**)&f->ll_stage, M * 8, hipHostMallocMapped) != hipSuccess) {
            f->ll_stage = nullptr;
        }
    }
    (void)hipGetLastError();
    if (o->moments) {
        a.mom = (double*)(base + L.mom);
        a.mpart = (double*)(base + L.mpart);
    }
    a.trace = (u64*)(base + L.trace);
    SMC_HIP_CHECK(hipMemsetAsync(a.summ, 0, M * (T + 1) * SUMM_STRIDE * 8, st));
    SMC_HIP_CHECK(hipMemsetAsync(a.cnt, 0, M * 2 * F_CNT_WORDS * sizeof(unsigned), st));
    SMC_HIP_CHECK(hipMemsetAsync(a.Q, 0, M * a.ntiles * 8, st));
    {   // step record of t = 0: {t, rs_flag, y_0, m, 1/s}
        std::vector<double> h(M * INFO_STRIDE, 0.0);
        for (size_t i = 0; i < M; ++i) {
            h[i * INFO_STRIDE + 2] = y_host[0];
            h[i * INFO_STRIDE + 5] = model->aux_host ? model->aux_host[0] : 0.0;
        }
        SMC_HIP_CHECK(hipMemcpyAsync(a.info, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
        SMC_HIP_CHECK(hipMemsetAsync(a.info2, 0, M * INFO_STRIDE * 8, st));
        SMC_HIP_CHECK(hipStreamSynchronize(st));
    }
    SMC_HIP_CHECK(hipMemsetAsync(a.A, 0, (M * N + F_TILE) * 4, st));     // (+ the padding tile: valid indices)
    std::vector<double> par_host(M * PARAM_STRIDE, 0.0);
    if (!mv) {       // the host's rows + the correctly rounded reciprocals smc_div_c works with
        for (size_t i = 0; i < M; ++i)
            for (int k = 0; k < PARAM_HOST; ++k) {
                const double v = model->params_host[i * PARAM_HOST + k];
                par_host[i * PARAM_STRIDE + k] = v;
                const double av = v < 0 ? -v : v;
                par_host[i * PARAM_STRIDE + PARAM_HOST + k] = (av > 1e-20 && av < 1e20) ? 1.0 / v : 0.0;
            }
        SMC_HIP_CHECK(hipMemcpyAsync(dpar, par_host.data(), M * PARAM_STRIDE * 8, hipMemcpyHostToDevice, st));
    }
    a.mvc = (const double*)(base + L.mvc);
    if (mv)
        SMC_HIP_CHECK(hipMemcpyAsync((void*)a.mvc, m.mvc_host.data(), m.mvc_host.size() * 8, hipMemcpyHostToDevice, st));
    SMC_HIP_CHECK(hipMemcpyAsync(dy, y_host, T * a.dy * 8, hipMemcpyHostToDevice, st));
    if (model->aux_host) {
        a.aux = (const double*)(base + L.aux);
        SMC_HIP_CHECK(hipMemcpyAsync((void*)a.aux, model->aux_host, T * 8, hipMemcpyHostToDevice, st));
    }
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

// The univariate kinds SmTrans evaluates the transition density of -- what backward sampling, on-line and two-filter
// smoothing and conditional SMC take: the fused filter's kinds (f_with_kind) without SVLEVERAGE (its transition
// reads y_{t-1}).  fn(std::integral_constant<int, kind>{}) is the one switch from a kind to a template argument of their
// launches; another kind launches nothing, and every caller has passed sm_kind_ok.  The lambdas hold launches only
// (SMC_REQUIRE, SMC_HIP_CHECK return from the function they stand in).
template <class F>
static void sm_with_kind(int kind, F&& fn)
{
    f_with_kind(kind, [&](auto k) {
        if constexpr (F_VAL(k) != SMC_MODEL_SVLEVERAGE) fn(k);
    });
}
static bool sm_kind_ok(int kind)
{
    bool ok = false;
    sm_with_kind(kind, [&](auto) { ok = true; });
    return ok;
}

extern "C" {

static int filter_fetch(smc_filter* f, int field, i64 s, int island, void* out_host);
static void flush_rows(smc_filter* f);

int smc_filter_create(smc_ctx* ctx, const smc_model* model, const smc_filter_opts* o,
                      const double* y_host, smc_filter** out)
{
    // ---- validate
    SMC_REQUIRE(ctx && model && o && y_host && out, "null argument");
    SMC_REQUIRE(o->N > 0 && o->T > 0 && o->n_islands > 0, "N, T, n_islands must be positive");
    if (o->scheme != SMC_MULTINOMIAL && o->scheme != SMC_STRATIFIED &&
        o->scheme != SMC_SYSTEMATIC) {
        smc_set_error("%d is not a valid resampling scheme", o->scheme);
        return SMC_ERR_SCHEME;
    }
    const bool mv = model->kind == SMC_MODEL_MVLINGAUSS;
    SMC_REQUIRE(mv || f_kind_ok(model->kind), "fused filter: unknown model kind");
    SMC_REQUIRE(mv ? (model->fk == SMC_FK_BOOTSTRAP || model->fk == SMC_FK_GUIDED || model->fk == SMC_FK_APF)
                   : f_model_ok(model->kind, model->fk),
                "guided filter: LINGAUSS, STOCHVOL, MVLINGAUSS; auxiliary filter: STOCHVOL, LINGAUSS, MVLINGAUSS; "
                "auxiliary bootstrap filter: STOCHVOL, LINGAUSS");
    {
        const bool big = o->N > F_TILE && o->N <= ((int64_t)1 << 30);
        if (!mv && f_is_apf(model->fk) && ((o->N > F_TILE && !big) || (!big && (o->moments || o->keep_history >= 2)))) {
            smc_set_error("the auxiliary particle filter is fused for N <= 1024 (the one-launch filter: no moments, no "
                          "rolling window) and for 1024 < N <= 2^30 (the two-level step)");
            return SMC_ERR_INVALID;
        }
    }
    SMC_REQUIRE(model->kind != SMC_MODEL_GORDON || model->aux_host,
                "GORDON needs aux_host (d*cos(e*(t-1)) per step)");
    SMC_REQUIRE(model->kind != SMC_MODEL_DISCRETECOX || model->aux_host,
                "DISCRETECOX needs aux_host (gammaln(y_t + 1) per step)");
    SMC_REQUIRE(mv || model->params_host, "params_host is required");
    MvSetup m;
    if (mv) {
        m.dx = model->dx; m.dy = model->dy;
        SMC_REQUIRE(m.dx >= 1 && m.dx <= 32 && m.dy >= 1 && m.dy <= m.dx,
                    "MVLINGAUSS needs 1 <= dy <= dx <= 32");
        SMC_REQUIRE(model->F_host && model->G_host && model->covX_host && model->covY_host &&
                        model->mu0_host && model->cov0_host, "MVLINGAUSS matrices are required");
        m.dp = m.dx <= 16 ? 16 : 32;            // padded to whole 16x16 MFMA blocks
        if (!mv_build_constants(model, model->fk, m.dp, o->T, y_host, m.mvc_host, &m.diag)) {
            // same failure as MvNormal.__init__ (distributions.py:935-940)
            smc_set_error("MvNormal: argument cov must be a (d, d) pos. definite matrix");
            return SMC_ERR_INVALID;
        }
    }
    SMC_REQUIRE(o->N < ((i64)1 << 32), "N must be below 2^32");
    SMC_HIP_CHECK(hipSetDevice(ctx->device));
    const bool strict = (o->flags & SMC_FLAG_STRICT_ANCESTORS) != 0;
    if (o->flags & SMC_FLAG_SQMC) {
        // core.py:339-349 as a fused loop.  Univariate Normal kernels (Gamma = ppf), N = 2^k >= 2 tiles: the
        // two-level step (the sorted Sobol' order in closed form).  MVLINGAUSS (2 <= d <= 9: d + 1 Sobol'
        // coordinates) and univariate filters of N = 2^k < 2 tiles: the flat step behind the Hilbert sort / the
        // argsort, N >= 32, no history slots (the sorted weights take the slot).
        bool pow2 = false;
        for (int k = 5; k <= 30; ++k) pow2 = pow2 || (((i64)1 << k) == o->N);
        const bool flat = sqmc_on_flat_step(model, o);
        const bool fk_ok = model->fk == SMC_FK_BOOTSTRAP || model->fk == SMC_FK_GUIDED;
        const bool mv_ok = !flat || ((!mv || (model->dx >= 2 && model->dx <= 9)) && !o->keep_history && !o->moments &&
                                     !(o->flags & SMC_FLAG_COLLAPSED_PROPOSAL));
        if (!fk_ok || !pow2 || !mv_ok || strict || o->rng_mode != SMC_RNG_PHILOX || (flat && o->use_graph) ||
            (o->flags & (SMC_PATH_FLAT_CDF | SMC_PATH_FORCE_UNFUSED))) {
            smc_set_error("SMC_FLAG_SQMC: Bootstrap / Guided filters, N = 2^k with 5 <= k <= 30, Philox mode; MVLINGAUSS "
                          "(2 <= d <= 9) and univariate models with k <= 10: eager launches, no history slots, no moments");
            return SMC_ERR_INVALID;
        }
    }
    if (strict && (mv || f_is_apf(model->fk) || o->N >= ((i64)1 << 32))) {
        smc_set_error("SMC_FLAG_STRICT_ANCESTORS: univariate Bootstrap / Guided filters");
        return SMC_ERR_INVALID;
    }
    SMC_REQUIRE(o->keep_history >= 0, "keep_history must be 0, 1 or a window length >= 2");

    // ---- shape, plan, layout: host arithmetic only
    smc_filter* f = new smc_filter();
    f->ctx = ctx;
    f->kind = model->kind;
    f->fk = model->fk;
    f->use_graph = o->use_graph != 0;
    f->sq_seed = o->seed;
    shape_args(f->a, model, o, m);
    int rc = plan_step(ctx, model, o, f->a, &f->plan);
    if (rc == SMC_OK) {
        // (the plan's words the kernels read)
        f->a.kform = f->plan.two_level ? 1 : 0;
        f->a.strict_e = (f->plan.strict() && f->plan.strict_form == STRICT_TWO_LEVEL) ? 1 : 0;
        f->a.xcd_chunks = f->plan.xcd_chunks ? 1 : 0;
        f->a.sp_tpw = f->plan.sp_tpw;
        f->a.sp_nwg = f->plan.sp_nwg;
        const SlabLayout L = slab_layout(f->a, f->plan, model, o, m.mvc_host.size());
        // ---- allocate, fill
        // the slab comes from the context's pool (smc_malloc: blocks recycled by exact size, ordered on
        // the context's one stream): a PMMH chain or the PMCMC moves of SMC^2 create and destroy a filter
        // of the same shape per proposal, and hipMalloc / hipFree of tens of MB cost milliseconds each
        f->slab_bytes = L.bytes;
        rc = smc_malloc(ctx, L.bytes, &f->slab) == SMC_OK ? SMC_OK : SMC_ERR_NOMEM;
        if (rc == SMC_OK) rc = fill_filter(f, L, model, o, y_host, m);
    }
    if (rc != SMC_OK) {        // the one failure exit: whatever exists by now
        if (f->slab) (void)smc_free(ctx, f->slab);
        if (f->ll_stage) (void)hipHostFree(f->ll_stage);
        delete f;
        return rc;
    }
    *out = f;
    return SMC_OK;
}

#ifdef SMC_TRACE
// debug builds only (tools/trace_step.py): per-workgroup phase stamps of the last step
int smc_debug_trace(smc_filter* f, uint64_t* out_host)
{
    // (n_islands, nparts, 8) stamps of k_propagate, then (n_islands, ntiles, 8) of k_ancestors
    SMC_HIP_CHECK(hipMemcpyAsync(out_host, f->a.trace,
                                 (size_t)f->a.n_islands * (f->a.nparts + f->a.ntiles) * 64,
                                 hipMemcpyDeviceToHost, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}
// ... of the strict step's two launches (island 0): (2 ntiles + 8, 8) stamps -- classify per tile, the chain, search per tile
int smc_debug_trace_strict(smc_filter* f, uint64_t* out_host)
{
    SMC_HIP_CHECK(hipMemcpyAsync(out_host, f->a.trace + (size_t)f->a.n_islands * (f->a.nparts + f->a.ntiles) * 8,
                                 (size_t)(2 * f->a.ntiles + 8) * 64, hipMemcpyDeviceToHost, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}
#endif

int smc_filter_destroy(smc_filter* f)
{
    if (!f) return SMC_OK;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    for (hipGraphExec_t g : f->gexec)
        if (g) (void)hipGraphExecDestroy(g);
    for (hipEvent_t e : f->ev) (void)hipEventDestroy(e);
    (void)smc_free(f->ctx, f->slab);
    if (f->ll_stage) {
        auto& v = f->ctx->pinned[(size_t)f->a.n_islands * 8];
        if (v.size() < 4) v.push_back(f->ll_stage);
        else (void)hipHostFree(f->ll_stage);
    }
    if (f->th_buf) (void)hipFree(f->th_buf);
    delete f;
    return SMC_OK;
}

// An independent copy of a filter in its current state: what copy.deepcopy(pf) is to the reference
// (smc_samplers.py:319-361: theta-level resampling of SMC^2 deep-copies every duplicated filter).
// One slab allocation, one device-to-device copy, every slab pointer of the argument block re-based;
// replay tapes (caller-owned, read-only) are shared.  Philox streams are a function of
// (seed, island id, particle, t): a clone continues with the SAME draws as its source -- exactly
// what deepcopy of a filter plus numpy's global generator gives the reference NOT; callers that
// need the copies to diverge re-seed them (smc_filter_reseed).
int smc_filter_clone(smc_filter* src, smc_filter** out)
{
    if (src) { (void)hipSetDevice(src->ctx->device); flush_rows(src); }
    SMC_REQUIRE(src && out, "null argument");
    smc_ctx* ctx = src->ctx;
    SMC_HIP_CHECK(hipSetDevice(ctx->device));
    void* slab = nullptr;
    if (smc_malloc(ctx, src->slab_bytes, &slab) != SMC_OK) return SMC_ERR_NOMEM;
    smc_filter* f = new smc_filter(*src);
    f->slab = slab;
    f->gexec[0] = f->gexec[1] = f->gexec[2] = nullptr;      // graphs hold the source's addresses
    f->graph_failed = false;
    f->prof = false;
    f->prof_n = 0;
    f->ev.clear();
    f->lazy_pending.clear();                                // (counts what THIS filter enqueues)
    f->lazy_elided = 0;
    f->ll_stage = nullptr;
    f->th_buf = nullptr;
    f->lwth = f->th = f->th_ess = nullptr;
    const char* s0 = (const char*)src->slab;
    const ptrdiff_t delta = (char*)slab - s0;
    auto rebase = [&](auto*& p) {
        const char* c = (const char*)p;
        if (c && c >= s0 && c < s0 + src->slab_bytes) p = (std::remove_reference_t<decltype(p)>)((char*)p + delta);
    };
    FArgs& a = f->a;
    rebase(a.X); rebase(a.lw); rebase(a.A); rebase(a.Q); rebase(a.Qpre); rebase(a.pm); rebase(a.ps); rebase(a.pss);
    rebase(a.cq); rebase(a.tq); rebase(a.cnt); rebase(a.spart); rebase(a.summ); rebase(a.params); rebase(a.y);
    rebase(a.mom); rebase(a.mpart); rebase(a.aux); rebase(a.info); rebase(a.hcnt); rebase(a.hlist); rebase(a.info2);
    rebase(a.su); rebase(a.E); rebase(a.sst); rebase(a.mvc); rebase(a.trace); rebase(a.pm2); rebase(a.ps2); rebase(a.pss2);
    rebase(a.eta); rebase(a.lwsv); rebase(a.sdec);
    rebase(f->tmp); rebase(f->strict_ws); rebase(f->sq_z); rebase(f->sq_perm); rebase(f->sq_ws);
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(slab, src->slab, src->slab_bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && src->th_buf) {
        const size_t M = (size_t)a.n_islands, T = (size_t)a.T, Ng = (size_t)src->th_n;
        const size_t nb = (Ng + TH_STRIDE + 2 * T + (src->th_comm ? M + Ng : 0)) * 8;
        e = hipMalloc(&f->th_buf, nb);
        if (e == hipSuccess) e = hipMemcpyAsync(f->th_buf, src->th_buf, nb, hipMemcpyDeviceToDevice, st);
        f->lwth = (double*)f->th_buf;
        f->th = f->lwth + Ng;
        f->th_ess = f->th + TH_STRIDE;
        f->th_send = src->th_comm ? f->th_ess + 2 * T : nullptr;
        f->th_recv = src->th_comm ? f->th_send + M : nullptr;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        smc_set_error("smc_filter_clone: %s", hipGetErrorString(e));
        if (f->th_buf) (void)hipFree(f->th_buf);
        (void)smc_free(ctx, slab);
        delete f;
        return SMC_ERR_HIP;
    }
    if (hipHostMalloc((void**)&f->ll_stage, (size_t)a.n_islands * 8, hipHostMallocMapped) != hipSuccess)
        f->ll_stage = nullptr;
    (void)hipGetLastError();
    *out = f;
    return SMC_OK;
}

// ---- checkpoint / resume (pickling of a device filter: core.py:415-428 returns SMC objects from worker processes,
// utils.py:178-186).  The state of a filter is its slab -- every device array, no pointers inside -- plus a handful of
// host words; a filter created from the same (model, options, data) has the same layout, so the slab of one can be
// loaded into the other and the run continues bit for bit.
struct FStateHeader {
    u64 magic, slab_bytes;
    i64 N, T, t_host, perm_t;
    int n_islands, scheme, kind, fk, hist, dx, flags_strict, flags_sqmc;
    u64 seed, sp_epoch, sq_seed, sq_ctr0;
    int flush_pending, island_offset;
};
#define F_STATE_MAGIC 0x534d435f53544131ull    /* "SMC_STA1" */
int smc_filter_state_bytes(smc_filter* f, int64_t* nbytes)
{
    SMC_REQUIRE(f && nbytes, "null argument");
    SMC_REQUIRE(!f->th_buf, "a filter with a theta level (SMC^2) is checkpointed by its owner, not as a filter");
    *nbytes = (int64_t)(sizeof(FStateHeader) + f->slab_bytes);
    return SMC_OK;
}
int smc_filter_save_state(smc_filter* f, void* out_host, int64_t nbytes)
{
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(!f->th_buf, "a filter with a theta level (SMC^2) is checkpointed by its owner, not as a filter");
    SMC_REQUIRE(nbytes == (int64_t)(sizeof(FStateHeader) + f->slab_bytes), "buffer size: smc_filter_state_bytes");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    flush_rows(f);
    FStateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = F_STATE_MAGIC; h.slab_bytes = f->slab_bytes;
    h.N = f->a.N; h.T = f->a.T; h.t_host = f->t_host; h.perm_t = f->perm_t;
    h.n_islands = f->a.n_islands; h.scheme = f->a.scheme; h.kind = f->kind; h.fk = f->fk; h.hist = f->a.hist; h.dx = f->a.dx;
    h.flags_strict = f->plan.strict() ? 1 : 0; h.flags_sqmc = f->plan.sqmc() ? 1 : 0;
    h.seed = f->a.seed; h.sp_epoch = f->sp_epoch; h.sq_seed = f->sq_seed; h.sq_ctr0 = f->sq_ctr0;
    h.flush_pending = f->flush_pending ? 1 : 0; h.island_offset = f->a.island_offset;
    memcpy(out_host, &h, sizeof h);
    SMC_HIP_CHECK(hipMemcpyAsync((char*)out_host + sizeof h, f->slab, f->slab_bytes, hipMemcpyDeviceToHost, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}
int smc_filter_load_state(smc_filter* f, const void* in_host, int64_t nbytes)
{
    SMC_REQUIRE(f && in_host, "null argument");
    SMC_REQUIRE(!f->th_buf, "a filter with a theta level (SMC^2) is checkpointed by its owner, not as a filter");
    SMC_REQUIRE(nbytes >= (int64_t)sizeof(FStateHeader), "truncated state");
    FStateHeader h;
    memcpy(&h, in_host, sizeof h);
    SMC_REQUIRE(h.magic == F_STATE_MAGIC, "not a filter state (magic)");
    SMC_REQUIRE(h.slab_bytes == f->slab_bytes && nbytes == (int64_t)(sizeof h + h.slab_bytes) && h.N == f->a.N && h.T == f->a.T &&
                    h.n_islands == f->a.n_islands && h.scheme == f->a.scheme && h.kind == f->kind && h.fk == f->fk &&
                    h.hist == f->a.hist && h.dx == f->a.dx && h.flags_strict == (f->plan.strict() ? 1 : 0) &&
                    h.flags_sqmc == (f->plan.sqmc() ? 1 : 0),
                "the state belongs to a filter of another shape (model, N, T, islands, scheme, history or flags differ)");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    { int64_t n; const int rc = smc_filter_lazy_lw_steps(f, &n); if (rc) return rc; }    // (its rows are about to be replaced)
    SMC_HIP_CHECK(hipMemcpyAsync(f->slab, (const char*)in_host + sizeof h, f->slab_bytes, hipMemcpyHostToDevice, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    f->t_host = h.t_host; f->perm_t = h.perm_t;
    f->a.seed = h.seed; f->sp_epoch = h.sp_epoch; f->sq_seed = h.sq_seed; f->sq_ctr0 = h.sq_ctr0;
    f->flush_pending = h.flush_pending != 0;
    f->a.island_offset = h.island_offset;
    for (hipGraphExec_t& g : f->gexec)          // captured launches carry the old key / counters by value
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    return SMC_OK;
}

// New Philox key for the steps still to run (a clone that must not repeat its source's draws).
int smc_filter_reseed(smc_filter* f, uint64_t seed)
{
    SMC_REQUIRE(f, "null filter");
    f->a.seed = seed;
    for (hipGraphExec_t& g : f->gexec)          // captured launches carry the old key by value
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    return SMC_OK;
}

// SMC_FLAG_SQMC: which points the run uses -- the stand-alone operator's stream (smc_sobol with
// scramble = safe = 1 under a context seeded with `point_seed`): point set counter0 at t = 0 (one
// coordinate), counter0 + t at step t (two coordinates, sorted by the first).  Default: the filter's own
// seed, counter0 = 1.
int smc_filter_sqmc_points(smc_filter* f, uint64_t point_seed, uint64_t counter0)
{
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(f->plan.sqmc(), "the filter was not created with SMC_FLAG_SQMC");
    SMC_REQUIRE(f->t_host == 0, "the point stream must be chosen before the first step");
    f->sq_seed = point_seed;
    f->sq_ctr0 = counter0;
    return SMC_OK;
}

int smc_filter_set_replay(smc_filter* f, const double* z, const double* u)
{
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(!f->plan.sqmc(), "SMC_FLAG_SQMC filters generate their points on the device");
    SMC_REQUIRE(f->t_host == 0, "replay tapes must be set before the first step");
    SMC_REQUIRE(z && u, "both tapes are required");
    f->a.zt = z;
    f->a.zt_ts = (i64)f->a.n_islands * f->a.N * f->a.dx;
    f->a.ut = u;
    f->a.ut_stride = (f->a.scheme == SMC_SYSTEMATIC) ? 1 : f->a.N;
    f->a.rng_mode = SMC_RNG_REPLAY;
    return SMC_OK;      // (the argument block travels by value with every launch)
}

// N <= 1024, univariate, no per-step side kernels: one persistent workgroup per island runs the
// requested steps in a single launch (smc_filter_small.h)
static bool small_filter_ok(const smc_filter* f)
{
    return f->plan.small && !f->prof && !philox_multinomial(f->a);
}

static void launch_small(smc_filter* f, int nsteps)
{
    hipStream_t st = f->ctx->stream;
    const dim3 grid(1, f->a.n_islands);
    f->a.par = -1;
    f_with_model(f->kind, f->fk, [&](auto k, auto q) {
        f_with_small_block(f->a.N, [&](auto bs) {
            SMC_LAUNCH((k_filter_small<F_VAL(k), F_VAL(q), F_VAL(bs)>), grid, dim3(F_VAL(bs)), st, f->a, nsteps);
        });
    });
}

// Conditional SMC (smc_csmc.h): particle 0 of every island follows xstar (n_islands, T), a device buffer the caller owns.
// Accepted where k_csmc_small can run -- a fresh bootstrap filter of a kind backward sampling takes, one tile,
// multinomial, whole history, none of the side kernels; smc_filter_step then launches k_csmc_small (Philox or replay).
int smc_filter_set_conditional(smc_filter* f, const double* xstar_dev)
{
    SMC_REQUIRE(f && xstar_dev, "null argument");
    SMC_REQUIRE(sm_kind_ok(f->kind) && f->fk == SMC_FK_BOOTSTRAP,
                "conditional SMC on the device: bootstrap filters of LINGAUSS, STOCHVOL, GORDON, THETALOGISTIC, DISCRETECOX");
    SMC_REQUIRE(!f->plan.sqmc(), "conditional SMC on the device: not with SMC_FLAG_SQMC");
    SMC_REQUIRE(!f->plan.strict(), "conditional SMC on the device: not with SMC_FLAG_STRICT_ANCESTORS");
    SMC_REQUIRE(!f->use_graph, "conditional SMC on the device: not with use_graph");
    SMC_REQUIRE(f->a.N <= F_TILE, "conditional SMC on the device: N <= 1024 (one workgroup per filter)");
    SMC_REQUIRE(f->a.scheme == SMC_MULTINOMIAL, "conditional SMC on the device: multinomial resampling only");
    SMC_REQUIRE(f->a.hist == 1, "conditional SMC on the device: the filter must keep its whole history (keep_history = 1)");
    SMC_REQUIRE(!f->a.mom, "conditional SMC on the device: no device moments");
    SMC_REQUIRE(f->plan.small && !f->lwth && !f->prof,
                "conditional SMC on the device: the one-launch filter must be available (no SMC_PATH_NO_SMALL, theta level "
                "or profiling)");
    if (f->t_host != 0) {
        smc_set_error("smc_filter_set_conditional: the retained trajectory must be set before the first step");
        return SMC_ERR_STATE;
    }
    f->xstar = xstar_dev;
    return SMC_OK;
}

static void launch_csmc(smc_filter* f, int nsteps)
{
    hipStream_t st = f->ctx->stream;
    const dim3 grid(1, f->a.n_islands);
    f->a.par = -1;
    sm_with_kind(f->kind, [&](auto k) {
        f_with_small_block(f->a.N, [&](auto bs) {
            SMC_LAUNCH((k_csmc_small<F_VAL(k), F_VAL(bs)>), grid, dim3(F_VAL(bs)), st, f->a, nsteps, f->xstar);
        });
    });
}

// The summary row of step t (ESS, evidence terms, the (K, 1/s) its weights are normalised with) is written by the
// reduction that OPENS step t + 1; behind the last step enqueued nobody has done it yet.  k_flush2 does -- when
// somebody asks for results (every accessor below calls this), not at the end of every smc_filter_step call: a
// caller that steps in pieces (20 steps, sync, 20 steps ...) paid a launch per piece for a row the next piece's first
// kernel writes anyway.
static void flush_rows(smc_filter* f)
{
    if (f && f->flush_pending) {
        f->flush_pending = false;
        SMC_LAUNCH(k_flush2, dim3(f->a.n_islands), dim3(SMC_BLOCK), f->ctx->stream, f->a);
    }
}

int smc_filter_step(smc_filter* f, int64_t nsteps)
{
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(nsteps >= 0, "nsteps must be non-negative");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    i64 todo = nsteps;
    if (f->t_host + todo > f->a.T) todo = f->a.T - f->t_host;
    if (todo < 0) todo = 0;
    if (todo > 0 && f_is_apf(f->fk) && f->kind != SMC_MODEL_MVLINGAUSS && !small_filter_ok(f) && !f->a.pm2) {
        smc_set_error("the auxiliary particle filter with N <= 1024 runs on the one-launch filter only (no "
                      "profiling, no Philox multinomial)");
        return SMC_ERR_STATE;
    }
    if (todo > 0 && f->xstar) {
        if (f->lwth || f->prof) {
            smc_set_error("a conditional filter runs neither under a theta level nor with profiling on");
            return SMC_ERR_STATE;
        }
        launch_csmc(f, (int)(todo > 0x7fffffff ? 0x7fffffff : todo));
        SMC_LAUNCH_CHECK();
        f->t_host += todo;
        return SMC_OK;
    }
    if (todo > 0 && f->lwth) {
        // theta level on: the theta-weights are updated behind every step (and may freeze the batch)
        const bool small = small_filter_ok(f);
        for (i64 k = 0; k < todo; ++k) {
            if (small) launch_small(f, 1);
            else {
                enqueue_step(f, -1, f->t_host + k);
                if (f->plan.two_level) SMC_LAUNCH(k_flush2, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
            }
            if (f->th_comm) {
                // sharded population: my filters' increments -> all ranks' (ncclAllGather on this stream, no
                // host round trip) -> the replicated theta level, the same arithmetic on every rank
                SMC_LAUNCH(k_theta_pack, dim3(1), dim3(SMC_BLOCK), st, f->a, (const double*)f->th, f->th_send,
                           f->plan.two_level ? 1 : 0);
                const int rc = smc_comm_allgather_f64_async(f->th_comm, f->th_send, f->a.n_islands, f->th_recv);
                if (rc) return rc;
            }
            SMC_LAUNCH(k_theta_update, dim3(1), dim3(SMC_BLOCK), st, f->a, f->lwth, f->th, f->th_ess,
                       f->th_ess_min, f->plan.two_level ? 1 : 0, (const double*)(f->th_comm ? f->th_recv : nullptr),
                       f->th_comm ? f->th_n : f->a.n_islands);
        }
        SMC_LAUNCH_CHECK();
        f->t_host += todo;
        return SMC_OK;
    }
    if (todo > 0 && small_filter_ok(f)) {
        launch_small(f, (int)(todo > 0x7fffffff ? 0x7fffffff : todo));
        SMC_LAUNCH_CHECK();
        f->t_host += todo;
        return SMC_OK;
    }
    i64 done = 0;
#ifndef SMC_EMULATE
    // hipGraphs of 24, 8 and 2 steps (even sizes, entered at even t: the slot parity is baked into
    // the nodes), captured on first use; any request of two or more steps replays them greedily
    static const int F_GRAPH_SIZES[3] = {24, 8, 2};
    if (f->use_graph && !f->prof && !f->graph_failed && todo >= 2) {
        // graphs start at even t (SQMC: at even t >= 2 -- step 0 has no sort, the captured sequence always does)
        while (done < todo && (((f->t_host + done) & 1) || (f->plan.sqmc() && f->t_host + done < 2))) {
            enqueue_step(f, -1, f->t_host + done);
            ++done;
        }
        for (int gi = 0; gi < 3 && !f->graph_failed; ++gi) {
            const int GS = F_GRAPH_SIZES[gi];
            if (todo - done < GS) continue;
            if (!f->gexec[gi]) {   // (kernel arguments are final by the first step call)
                hipGraph_t g = nullptr;
                bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
                if (ok) {
                    for (int k = 0; k < GS; ++k) enqueue_step(f, -1, k, false);
                    ok = hipStreamEndCapture(st, &g) == hipSuccess && g &&
                         hipGraphInstantiate(&f->gexec[gi], g, nullptr, nullptr, 0) == hipSuccess;
                }
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                if (!ok) { f->gexec[gi] = nullptr; f->graph_failed = true; break; }
            }
            while (todo - done >= GS) {
                SMC_HIP_CHECK(hipGraphLaunch(f->gexec[gi], st));
                done += GS;
            }
        }
    }
#endif
    for (; done < todo; ++done) {
        int kp = -1;
        if (f->prof && f->prof_n < PROF_MAX) kp = f->prof_n++;
        enqueue_step(f, kp, f->t_host + done, true, done + 1 < todo);
    }
    if (f->plan.two_level && todo > 0) f->flush_pending = true;      // summary row of the last step: flush_rows, on demand
    SMC_LAUNCH_CHECK();
    f->t_host += todo;
    return SMC_OK;
}

// How many steps this filter has launched WITHOUT the log-weight store (plan.lazy_lw): the steps enqueued with
// a.lw_lazy set in which some island resampled -- the host knows the former, the decisions are word 4 of the steps'
// summary rows (written by the launch that opens the step).  Synchronises.
int smc_filter_lazy_lw_steps(smc_filter* f, int64_t* out)
{
    SMC_REQUIRE(f && out, "null argument");
    if (!f->lazy_pending.empty()) {
        SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
        const i64 T = f->a.T;
        std::vector<double> h((size_t)f->a.n_islands * (T + 1) * SUMM_STRIDE);
        SMC_HIP_CHECK(hipMemcpyAsync(h.data(), f->a.summ, h.size() * 8, hipMemcpyDeviceToHost, f->ctx->stream));
        SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
        for (const i64 t : f->lazy_pending) {
            bool any = false;
            for (int i = 0; i < f->a.n_islands; ++i) any = any || h[((size_t)i * (T + 1) + t) * SUMM_STRIDE + 4] != 0.0;
            f->lazy_elided += any ? 1 : 0;
        }
        f->lazy_pending.clear();
    }
    *out = f->lazy_elided;
    return SMC_OK;
}

int smc_filter_sync(smc_filter* f)
{
    SMC_REQUIRE(f, "null filter");
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}

int smc_filter_t(smc_filter* f, int64_t* t_out)
{
    SMC_REQUIRE(f && t_out, "null argument");
    *t_out = f->t_host;
    return SMC_OK;
}

int smc_filter_summaries(smc_filter* f, double* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    const i64 t = f->t_host, T = f->a.T;
    if (t == 0) return SMC_OK;
    std::vector<double> h((size_t)f->a.n_islands * (T + 1) * SUMM_STRIDE);
    SMC_HIP_CHECK(hipMemcpyAsync(h.data(), f->a.summ, h.size() * 8, hipMemcpyDeviceToHost,
                                 f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    for (int i = 0; i < f->a.n_islands; ++i)
        for (i64 s = 0; s < t; ++s)
            for (int c = 0; c < SMC_SUMMARY_COLS; ++c)
                out_host[((size_t)i * t + s) * SMC_SUMMARY_COLS + c] =
                    h[((size_t)i * (T + 1) + s) * SUMM_STRIDE + c];
    return SMC_OK;
}

// gather logLt of step t-1 of every island into one staging array (one D2H copy, one sync)
__global__ void k_f_collect_logLt(const double* summ, i64 T, i64 t, int n, double* out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = summ[((i64)i * (T + 1) + (t - 1)) * SUMM_STRIDE + 3];
}

int smc_filter_logLt(smc_filter* f, double* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    const i64 t = f->t_host, T = f->a.T;
    const int M = f->a.n_islands;
    for (int i = 0; i < M; ++i) out_host[i] = 0.0;
    if (t == 0) return SMC_OK;
    hipStream_t st = f->ctx->stream;
    if (f->ll_stage) {
        // the kernel writes into pinned host memory: one launch + one (spinning) stream sync
        SMC_LAUNCH(k_f_collect_logLt, dim3((M + 255) / 256), dim3(256), st, f->a.summ, T, t, M, f->ll_stage);
        SMC_LAUNCH_CHECK();
        SMC_HIP_CHECK(hipStreamSynchronize(st));
        memcpy(out_host, f->ll_stage, (size_t)M * 8);
        return SMC_OK;
    }
    for (int i = 0; i < M; ++i)
        SMC_HIP_CHECK(hipMemcpyAsync(out_host + i, f->a.summ + ((size_t)i * (T + 1) + (t - 1)) * SUMM_STRIDE + 3, 8,
                                     hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

int smc_filter_get(smc_filter* f, int field, int island, void* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    const i64 t = f->t_host;
    if (t == 0) {
        smc_set_error("smc_filter_get: no step has run yet");
        return SMC_ERR_STATE;
    }
    return filter_fetch(f, field, t - 1, island, out_host);
}

/* state of step s (the filter's current one, or -- keep_history -- any earlier one) */
static int filter_fetch(smc_filter* f, int field, i64 s, int island, void* out_host)
{
    const i64 N = f->a.N;
    const i64 t = s + 1;
    hipStream_t st = f->ctx->stream;
    const int dx = f->a.dx;
    const double* X = f_X(f->a, s) + (size_t)island * N * dx;
    const double* Xo = f_X(f->a, s - 1) + (size_t)island * N * dx;
    size_t nbytes = (size_t)N * 8;
    const double* lw = f_lw(f->a, s) + (size_t)island * N;
    const u32* A = f_A(f->a, s) + (size_t)island * N;
    const void* src = nullptr;
    const unsigned nb = (unsigned)((N + SMC_BLOCK - 1) / SMC_BLOCK);
    switch (field) {
    case SMC_FIELD_X: src = X; nbytes *= dx; break;
    case SMC_FIELD_LW: src = lw; break;
    case SMC_FIELD_A:
    case SMC_FIELD_XP: {
        if (t < 2) { smc_set_error("smc_filter_get: A / Xp are undefined before step 1"); return SMC_ERR_STATE; }
        if (f->perm_t == f->t_host && s == f->t_host - 1) {
            smc_set_error("smc_filter_get: A / Xp are undefined right after smc_filter_permute_islands");
            return SMC_ERR_STATE;
        }
        // did the last step resample?  (core.py:329-336: else A = arange(N), Xp = X)
        double flag = 0.0;
        SMC_HIP_CHECK(hipMemcpyAsync(&flag, f->a.summ + ((size_t)island * (f->a.T + 1) + (t - 1)) * SUMM_STRIDE + 4,
                                     8, hipMemcpyDeviceToHost, st));
        SMC_HIP_CHECK(hipStreamSynchronize(st));
        if (flag == 0.0) {
            if (field == SMC_FIELD_A) {
                int64_t* o = (int64_t*)out_host;
                for (i64 i = 0; i < N; ++i) o[i] = i;
                return SMC_OK;
            }
            src = Xo;
            nbytes *= dx;
        } else if (field == SMC_FIELD_A) {
            SMC_LAUNCH(k_f_widen, dim3(nb), dim3(SMC_BLOCK), st, A, N, (i64*)f->tmp);
            src = f->tmp;
        } else {
            SMC_LAUNCH(k_f_gather_rows, dim3((unsigned)((N * dx + SMC_BLOCK - 1) / SMC_BLOCK)),
                       dim3(SMC_BLOCK), st, Xo, A, N, dx, f->tmp);
            src = f->tmp;
            nbytes *= dx;
        }
        break;
    }
    case SMC_FIELD_W: {
        const double* row = f->a.summ + ((size_t)island * (f->a.T + 1) + (t - 1)) * SUMM_STRIDE;
        SMC_LAUNCH(k_f_write_W, dim3(nb), dim3(SMC_BLOCK), st, lw, N, row, f->tmp, f->plan.two_level ? 1 : 0);
        src = f->tmp;
        break;
    }
    default:
        smc_set_error("smc_filter_get: unknown field %d", field);
        return SMC_ERR_INVALID;
    }
    SMC_LAUNCH_CHECK();
    SMC_HIP_CHECK(hipMemcpyAsync(out_host, src, nbytes, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

// Replace the particles and / or log-weights of the step just done (island `island`) by host
// arrays: what a caller does that moves particles itself between two steps (an MCMC
// rejuvenation of the x-particles, importing a particle system; the reference's counterpart is
// assigning pf.X / pf.wgts, core.py:222-233).  Everything the next step derives from the
// log-weights (ESS, log-mean weight and evidence of this step, the resample decision and the
// CDF of the next) is recomputed on the device as if the step had produced these values.
int smc_filter_set_state(smc_filter* f, int island, const double* X_host, const double* lw_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    if (f->t_host == 0) {
        smc_set_error("smc_filter_set_state: no step has run yet");
        return SMC_ERR_STATE;
    }
    if (f->kind == SMC_MODEL_MVLINGAUSS && lw_host) {
        smc_set_error("smc_filter_set_state: log-weights of a multivariate filter cannot be replaced");
        return SMC_ERR_STATE;
    }
    if (f_is_apf(f->fk)) {
        // the next step of an auxiliary filter resamples on lw + logeta(X) and resets the weights to a
        // constant formed from both (core.py:299-313): replacing X or lw alone would leave the record's
        // auxiliary normalisation and reset constant stale (one-launch filter and two-level step alike)
        smc_set_error("smc_filter_set_state: not available for the auxiliary particle filter");
        return SMC_ERR_STATE;
    }
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    const i64 N = f->a.N, ts = f->t_host - 1;
    if (X_host)
        SMC_HIP_CHECK(hipMemcpyAsync(f_X(f->a, ts) + (size_t)island * N * f->a.dx, X_host,
                                     (size_t)N * f->a.dx * 8, hipMemcpyHostToDevice, st));
    if (lw_host) {
        SMC_HIP_CHECK(hipMemcpyAsync(f_lw(f->a, ts) + (size_t)island * N, lw_host, (size_t)N * 8,
                                     hipMemcpyHostToDevice, st));
        SMC_LAUNCH(k_f_partials, dim3(f->a.nparts, f->a.n_islands), dim3(SMC_BLOCK), st, f->a, ts,
                   f->plan.two_level ? 1 : 0);
        if (f->plan.two_level) SMC_LAUNCH(k_flush2, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a);
        else SMC_LAUNCH(k_f_restate, dim3(f->a.n_islands), dim3(SMC_BLOCK), st, f->a, ts);
    }
    SMC_LAUNCH_CHECK();
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

// The per-island arrays that make up the state of a filter at step t-1 (what theta-level
// resampling and the PMCMC move transport): (pointer, 8-byte words per island)
struct IslandArray { void* p; i64 words; };
static int island_arrays(smc_filter* f, i64 t, IslandArray* out)
{
    const FArgs& a = f->a;
    const i64 N = a.N, T = a.T;
    int n = 0;
    out[n++] = {f_X(a, t - 1), N * a.dx};
    out[n++] = {f_lw(a, t - 1), N};
    out[n++] = {a.summ, (T + 1) * SUMM_STRIDE};
    out[n++] = {a.info, INFO_STRIDE};
    if (f->kind != SMC_MODEL_MVLINGAUSS) out[n++] = {(void*)a.params, PARAM_STRIDE};
    if (f->plan.two_level) {
        out[n++] = {a.pm, a.nparts};
        out[n++] = {a.ps, a.nparts};
        out[n++] = {a.pss, a.nparts};
        out[n++] = {a.tq, a.nparts};
        out[n++] = {a.info2, INFO_STRIDE};
        out[n++] = {a.cq, a.ncq};
    }
    return n;
}

// theta-level resampling of whole filters (SMC^2: smc_samplers.py:319-361 FancyList
// deep copies): island i continues from the state of island src[i] -- particles,
// log-weights, per-step summaries, step record and parameter row move together; the
// Philox streams stay tied to the SLOT (two copies of one island evolve independently).
// One gather kernel + one contiguous copy per array (a dozen launches, whatever n_islands).
int smc_filter_permute_islands(smc_filter* f, const int64_t* src_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && src_host, "null argument");
    if (f->a.pm2) {
        smc_set_error("whole-island moves are not available for the auxiliary filter on the two-level step");
        return SMC_ERR_STATE;
    }
    if (f->a.hist) {
        smc_set_error("smc_filter_permute_islands: not available with keep_history");
        return SMC_ERR_STATE;
    }
    const int M = f->a.n_islands;
    const i64 t = f->t_host;
    for (int i = 0; i < M; ++i)
        if (src_host[i] < 0 || src_host[i] >= M) {
            smc_set_error("smc_filter_permute_islands: source %lld out of range", (long long)src_host[i]);
            return SMC_ERR_INVALID;
        }
    if (t == 0 || M == 1) return SMC_OK;
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    IslandArray arr[16];
    const int na = island_arrays(f, t, arr);
    i64 maxw = 0;
    for (int k = 0; k < na; ++k) maxw = arr[k].words > maxw ? arr[k].words : maxw;
    char* tmp = nullptr;
    const size_t stage = (size_t)M * maxw * 8, idxb = (size_t)M * 8;
    hipError_t e = hipMalloc((void**)&tmp, stage + idxb);
    if (e != hipSuccess) {
        smc_set_error("smc_filter_permute_islands: %zu bytes: %s", stage + idxb, hipGetErrorString(e));
        return SMC_ERR_NOMEM;
    }
    i64* src = (i64*)(tmp + stage);
    hipError_t rc = hipMemcpyAsync(src, src_host, idxb, hipMemcpyHostToDevice, st);
    for (int k = 0; k < na && rc == hipSuccess; ++k) {
        const i64 w = arr[k].words;
        const unsigned chunks = (unsigned)((w + SMC_BLOCK - 1) / SMC_BLOCK > 64 ? 64 : (w + SMC_BLOCK - 1) / SMC_BLOCK);
        SMC_LAUNCH(k_island_gather, dim3(chunks, M), dim3(SMC_BLOCK), st, (const u64*)arr[k].p, (u64*)tmp,
                   (const i64*)src, (const unsigned char*)nullptr, w);
        rc = hipMemcpyAsync(arr[k].p, tmp, (size_t)M * w * 8, hipMemcpyDeviceToDevice, st);
    }
    if (rc == hipSuccess) rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    SMC_HIP_CHECK(rc);
    f->perm_t = t;
    return SMC_OK;
}

// PMCMC move of SMC^2 (smc_samplers.py:1129-1143): a second batch of filters was run on the
// proposed thetas; where the proposal is accepted, island i of `dst` takes over island i of `src`.
int smc_filter_copy_islands(smc_filter* dst, smc_filter* src, const unsigned char* accept_host)
{
    if (dst) { (void)hipSetDevice(dst->ctx->device); flush_rows(dst); }
    if (src) flush_rows(src);
    SMC_REQUIRE(dst && src && accept_host, "null argument");
    SMC_REQUIRE(dst->ctx == src->ctx, "both filters must live on one context");
    const FArgs &a = dst->a, &b = src->a;
    if (a.pm2 || b.pm2) {
        smc_set_error("whole-island moves are not available for the auxiliary filter on the two-level step");
        return SMC_ERR_STATE;
    }
    if (a.hist || b.hist) {
        smc_set_error("smc_filter_copy_islands: not available with keep_history");
        return SMC_ERR_STATE;
    }
    SMC_REQUIRE(a.N == b.N && a.T == b.T && a.n_islands == b.n_islands && a.dx == b.dx &&
                    dst->kind == src->kind && dst->fk == src->fk && dst->t_host == src->t_host &&
                    dst->plan.two_level == src->plan.two_level,
                "the two filters must have the same shape, model kind and time index");
    const i64 t = dst->t_host;
    if (t == 0) return SMC_OK;
    SMC_HIP_CHECK(hipSetDevice(dst->ctx->device));
    hipStream_t st = dst->ctx->stream;
    const int M = a.n_islands;
    unsigned char* mask = nullptr;
    SMC_HIP_CHECK(hipMalloc((void**)&mask, (size_t)M));
    hipError_t rc = hipMemcpyAsync(mask, accept_host, (size_t)M, hipMemcpyHostToDevice, st);
    IslandArray da[16], sa[16];
    const int na = island_arrays(dst, t, da);
    (void)island_arrays(src, t, sa);
    for (int k = 0; k < na && rc == hipSuccess; ++k) {
        const i64 w = da[k].words;
        const unsigned chunks = (unsigned)((w + SMC_BLOCK - 1) / SMC_BLOCK > 64 ? 64 : (w + SMC_BLOCK - 1) / SMC_BLOCK);
        SMC_LAUNCH(k_island_gather, dim3(chunks, M), dim3(SMC_BLOCK), st, (const u64*)sa[k].p, (u64*)da[k].p,
                   (const i64*)nullptr, (const unsigned char*)mask, w);
    }
    if (rc == hipSuccess) rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    (void)hipFree(mask);
    SMC_HIP_CHECK(rc);
    dst->perm_t = t;
    return SMC_OK;
}

// ---- island migration between GPUs (multi-GPU SMC^2: theta-particles sharded over ranks, a
// global theta-resampling moves whole filters; smc_comm_alltoallv carries the packed states) ----
int smc_filter_island_bytes(smc_filter* f, int64_t* bytes)
{
    SMC_REQUIRE(f && bytes, "null argument");
    IslandArray arr[16];
    const int na = island_arrays(f, f->t_host > 0 ? f->t_host : 1, arr);
    i64 w = 0;
    for (int k = 0; k < na; ++k) w += arr[k].words;
    *bytes = w * 8;
    return SMC_OK;
}

static int island_pack(smc_filter* f, const int64_t* islands_host, int n, void* pack_dev, int unpack)
{
    SMC_REQUIRE(f && (n == 0 || (islands_host && pack_dev)), "null argument");
    if (f->a.pm2) {
        smc_set_error("whole-island moves are not available for the auxiliary filter on the two-level step");
        return SMC_ERR_STATE;
    }
    if (f->a.hist) {
        smc_set_error("island migration is not available with keep_history");
        return SMC_ERR_STATE;
    }
    if (n == 0 || f->t_host == 0) return SMC_OK;
    for (int j = 0; j < n; ++j)
        SMC_REQUIRE(islands_host[j] >= 0 && islands_host[j] < f->a.n_islands, "island out of range");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    IslandArray arr[16];
    const int na = island_arrays(f, f->t_host, arr);
    i64 stride = 0;
    for (int k = 0; k < na; ++k) stride += arr[k].words;
    i64* idx = nullptr;
    SMC_HIP_CHECK(hipMalloc((void**)&idx, (size_t)n * 8));
    hipError_t rc = hipMemcpyAsync(idx, islands_host, (size_t)n * 8, hipMemcpyHostToDevice, st);
    i64 off = 0;
    for (int k = 0; k < na && rc == hipSuccess; ++k) {
        const i64 w = arr[k].words;
        const unsigned chunks = (unsigned)((w + SMC_BLOCK - 1) / SMC_BLOCK > 64 ? 64 : (w + SMC_BLOCK - 1) / SMC_BLOCK);
        SMC_LAUNCH(k_island_pack, dim3(chunks, n), dim3(SMC_BLOCK), st, (u64*)arr[k].p, w, (u64*)pack_dev, stride,
                   off, (const i64*)idx, unpack);
        off += w;
    }
    if (rc == hipSuccess) rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    (void)hipFree(idx);
    SMC_HIP_CHECK(rc);
    if (unpack) f->perm_t = f->t_host;
    return SMC_OK;
}
int smc_filter_pack_islands(smc_filter* f, const int64_t* islands_host, int n, void* pack_dev)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    return island_pack(f, islands_host, n, pack_dev, 0);
}
int smc_filter_unpack_islands(smc_filter* f, const int64_t* islands_host, int n, const void* pack_dev)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    return island_pack(f, islands_host, n, (void*)pack_dev, 1);
}

// A filter that has not stepped yet takes the time index t: its state at t - 1 is then whatever
// smc_filter_unpack_islands puts there (waste-free SMC^2 assembles its new population from the chains'
// batches this way: smc_samplers.py:669-684 keeps every intermediate state WITH its particle filter).
// Islands that receive no state must not be stepped.
int smc_filter_fast_forward(smc_filter* f, int64_t t)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(f->t_host == 0, "smc_filter_fast_forward: the filter has already stepped");
    SMC_REQUIRE(t >= 0 && t <= f->a.T, "smc_filter_fast_forward: t must be in [0, T]");
    SMC_REQUIRE(!f->a.hist && !f->plan.sqmc() && !f->lwth, "smc_filter_fast_forward: no history slots, SQMC or theta level");
    f->t_host = t;
    f->perm_t = t;
    return SMC_OK;
}

// ---- SMC^2: the theta level (see k_theta_update) -------------------------------------------
static int theta_enable(smc_filter* f, double ess_rmin, smc_comm* comm)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(!f->a.hist && !f->a.mom, "the theta level is not available with keep_history / moments");
    SMC_REQUIRE(!f->a.pm2, "the theta level is not available for the auxiliary filter on the two-level step");
    SMC_REQUIRE(!comm || comm->ctx == f->ctx, "the communicator belongs to another context");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    const size_t M = (size_t)f->a.n_islands, T = (size_t)f->a.T;
    const size_t Ng = comm ? M * (size_t)comm->nranks : M;
    const size_t nb = (Ng + TH_STRIDE + 2 * T + (comm ? M + Ng : 0)) * 8;
    if (f->th_buf && (size_t)f->th_n != Ng) { (void)hipFree(f->th_buf); f->th_buf = nullptr; }
    if (!f->th_buf) SMC_HIP_CHECK(hipMalloc(&f->th_buf, nb));
    SMC_HIP_CHECK(hipMemsetAsync(f->th_buf, 0, nb, f->ctx->stream));
    f->lwth = (double*)f->th_buf;
    f->th = f->lwth + Ng;
    f->th_ess = f->th + TH_STRIDE;
    f->th_comm = comm;
    f->th_n = (int)Ng;
    f->th_send = comm ? f->th_ess + 2 * T : nullptr;
    f->th_recv = comm ? f->th_send + M : nullptr;
    f->th_ess_min = ess_rmin * (double)Ng;
    // (enabled on a batch that has already run t steps -- the exchange step: the theta weights
    //  start at zero, or at what smc_filter_theta_resume sets, and account for steps >= t)
    const double done = (double)f->t_host;
    SMC_HIP_CHECK(hipMemcpyAsync(f->th + 2, &done, 8, hipMemcpyHostToDevice, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}
int smc_filter_theta_enable(smc_filter* f, double ess_rmin) { return theta_enable(f, ess_rmin, nullptr); }

// The theta level of a population sharded over the ranks of `comm` (every rank: the same number of
// islands, rank r holds the global theta indices r M .. r M + M - 1): replicated on every rank, fed behind
// every step by ONE ncclAllGather of the ranks' evidence increments enqueued on the context's stream --
// the same arithmetic on the same N_theta values in the same order everywhere, hence the same decisions
// on every rank and for every world size, and no host synchronisation per step.  smc_filter_theta_state /
// _resume / _logmeans then speak of all nranks x n_islands theta-particles.  Every rank must make the same
// calls in the same order (smc_filter_step enqueues a collective per step).
int smc_filter_theta_enable_sharded(smc_filter* f, smc_comm* comm, double ess_rmin)
{
    SMC_REQUIRE(comm, "null communicator");
    return theta_enable(f, ess_rmin, comm);
}

int smc_filter_theta_state(smc_filter* f, double* lw_theta_host, int64_t* stop_t, int64_t* steps_done,
                           double* ess_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && f->lwth, "the theta level is not enabled");
    hipStream_t st = f->ctx->stream;
    double th[TH_STRIDE];
    SMC_HIP_CHECK(hipMemcpyAsync(th, f->th, sizeof th, hipMemcpyDeviceToHost, st));
    if (lw_theta_host)
        SMC_HIP_CHECK(hipMemcpyAsync(lw_theta_host, f->lwth, (size_t)f->th_n * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    if (stop_t) *stop_t = (int64_t)th[0];
    if (steps_done) *steps_done = (int64_t)th[2];
    if (ess_host && th[2] > 0) {
        SMC_HIP_CHECK(hipMemcpyAsync(ess_host, f->th_ess, (size_t)th[2] * 8, hipMemcpyDeviceToHost, st));
        SMC_HIP_CHECK(hipStreamSynchronize(st));
    }
    return SMC_OK;
}

// log-mean of the theta weights after every step accounted for (the outer SMC's log_mean_w,
// core.py:351-359: its differences between resamplings are the evidence increments of the model)
int smc_filter_theta_logmeans(smc_filter* f, double* out_host, int64_t* steps_done)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && f->lwth && out_host, "the theta level is not enabled, or null output");
    hipStream_t st = f->ctx->stream;
    double th[TH_STRIDE];
    SMC_HIP_CHECK(hipMemcpyAsync(th, f->th, sizeof th, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    if (steps_done) *steps_done = (int64_t)th[2];
    if (th[2] > 0) {
        SMC_HIP_CHECK(hipMemcpyAsync(out_host, f->th_ess + f->a.T, (size_t)th[2] * 8, hipMemcpyDeviceToHost, st));
        SMC_HIP_CHECK(hipStreamSynchronize(st));
    }
    return SMC_OK;
}

// After a stop: new theta log-weights (null: zeros -- the outer resampling, core.py:299-305),
// the time records back to the stop step, the host's step count with them; the filter then
// continues from there.  Also valid when nothing stopped (lw_theta replaced, time unchanged).
int smc_filter_theta_resume(smc_filter* f, const double* lw_theta_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && f->lwth, "the theta level is not enabled");
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    double th[TH_STRIDE];
    SMC_HIP_CHECK(hipMemcpyAsync(th, f->th, sizeof th, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    if (lw_theta_host)
        SMC_HIP_CHECK(hipMemcpyAsync(f->lwth, lw_theta_host, (size_t)f->th_n * 8, hipMemcpyHostToDevice, st));
    else
        SMC_HIP_CHECK(hipMemsetAsync(f->lwth, 0, (size_t)f->th_n * 8, st));
    if (th[0] != 0.0) {
        SMC_LAUNCH(k_theta_thaw, dim3(1), dim3(SMC_BLOCK), st, f->a, f->th, th[0]);
        SMC_LAUNCH_CHECK();
        f->t_host = (i64)th[0];
    }
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

int smc_filter_moments(smc_filter* f, double* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    if (!f->a.mom) {
        smc_set_error("smc_filter_moments: the filter was created without opts.moments");
        return SMC_ERR_STATE;
    }
    const i64 t = f->t_host, T = f->a.T;
    const size_t w = (size_t)2 * f->a.dx;
    for (int i = 0; i < f->a.n_islands && t > 0; ++i)
        SMC_HIP_CHECK(hipMemcpyAsync(out_host + (size_t)i * t * w, f->a.mom + (size_t)i * T * w,
                                     (size_t)t * w * 8, hipMemcpyDeviceToHost, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    return SMC_OK;
}

int smc_filter_history(smc_filter* f, int field, int64_t step, int island, void* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    if (!f->a.hist) {
        smc_set_error("smc_filter_history: the filter was created without keep_history");
        return SMC_ERR_STATE;
    }
    if (step < 0 || step >= f->t_host) {
        smc_set_error("smc_filter_history: step %lld has not run (t = %lld)", (long long)step,
                      (long long)f->t_host);
        return SMC_ERR_STATE;
    }
    if (f->a.hist >= 2) {          // rolling window: the f->a.hist most recent steps are resident
        const i64 oldest = f->t_host - f->a.hist;
        const bool needs_prev = field == SMC_FIELD_XP;         // Xp gathers from step - 1
        if (step < oldest || (needs_prev && step - 1 < oldest && step > 0)) {
            smc_set_error("smc_filter_history: step %lld has left the rolling window of %d steps",
                          (long long)step, f->a.hist);
            return SMC_ERR_STATE;
        }
    }
    return filter_fetch(f, field, step, island, out_host);
}

int smc_filter_spacings(smc_filter* f, int64_t t, int island, double* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    SMC_REQUIRE(t >= 1 && t < f->a.T, "resampling happens at steps 1 .. T - 1");
    if (f->a.scheme != SMC_MULTINOMIAL || f->a.ut || f->kind == SMC_MODEL_MVLINGAUSS) {
        smc_set_error("smc_filter_spacings: a univariate multinomial filter in production (Philox) mode only");
        return SMC_ERR_STATE;
    }
    SMC_HIP_CHECK(hipSetDevice(f->ctx->device));
    hipStream_t st = f->ctx->stream;
    SMC_LAUNCH(k_f_spacings_out, dim3(1), dim3(SMC_BLOCK), st, f->a, (i64)t, island, f->tmp);
    SMC_LAUNCH_CHECK();
    SMC_HIP_CHECK(hipMemcpyAsync(out_host, f->tmp, (size_t)f->a.N * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

int smc_filter_trajectories(smc_filter* f, int island, int64_t* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    if (!f->a.hist) {
        smc_set_error("smc_filter_trajectories: the filter was created without keep_history");
        return SMC_ERR_STATE;
    }
    const i64 t = f->t_host, N = f->a.N, T = f->a.T;
    if (t == 0) {
        smc_set_error("smc_filter_trajectories: no step has run yet");
        return SMC_ERR_STATE;
    }
    hipStream_t st = f->ctx->stream;
    // which steps resampled (A_s = arange otherwise, core.py:336)
    std::vector<double> rows((size_t)t * SUMM_STRIDE);
    SMC_HIP_CHECK(hipMemcpyAsync(rows.data(), f->a.summ + (size_t)island * (T + 1) * SUMM_STRIDE,
                                 rows.size() * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    // rolling window: the genealogy of the resident steps only (RollingParticleHistory,
    // smoothing.py:209-219 over its deque); out_host then holds min(t, window) rows
    const i64 first = (f->a.hist >= 2 && t > f->a.hist) ? t - f->a.hist : 0;
    const i64 nrows = t - first;
    i64* B = nullptr;
    hipError_t e = hipMalloc((void**)&B, (size_t)nrows * N * 8);
    if (e != hipSuccess) {
        smc_set_error("smc_filter_trajectories: %zu bytes: %s", (size_t)nrows * N * 8, hipGetErrorString(e));
        return SMC_ERR_NOMEM;
    }
    const dim3 grid((unsigned)((N + SMC_BLOCK - 1) / SMC_BLOCK));
    SMC_LAUNCH(k_f_iota, grid, dim3(SMC_BLOCK), st, N, B + (size_t)(nrows - 1) * N);
    for (i64 s = t - 1; s >= first + 1; --s) {          // smoothing.py:213-216
        const u32* A = rows[(size_t)s * SUMM_STRIDE + 4] != 0.0 ? f_A(f->a, s) + (size_t)island * N : nullptr;
        SMC_LAUNCH(k_f_genealogy, grid, dim3(SMC_BLOCK), st, A, (const i64*)(B + (size_t)(s - first) * N), N,
                   B + (size_t)(s - first - 1) * N);
    }
    hipError_t e2 = hipMemcpyAsync(out_host, B, (size_t)nrows * N * 8, hipMemcpyDeviceToHost, st);
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
    (void)hipFree(B);
    SMC_HIP_CHECK(e2);
    return SMC_OK;
}

int smc_filter_one_trajectory(smc_filter* f, int island, int64_t n_last, double* out_host)
{
    if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); }
    SMC_REQUIRE(f && out_host, "null argument");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    if (f->a.hist != 1) {
        smc_set_error("smc_filter_one_trajectory: the filter was created without keep_history = 1");
        return SMC_ERR_STATE;
    }
    const i64 t = f->t_host;
    SMC_REQUIRE(t > 0 && n_last >= 0 && n_last < f->a.N, "no step has run, or particle index out of range");
    hipStream_t st = f->ctx->stream;
    double* buf = nullptr;
    hipError_t e = hipMalloc((void**)&buf, (size_t)t * f->a.dx * 8);
    if (e != hipSuccess) {
        smc_set_error("smc_filter_one_trajectory: %s", hipGetErrorString(e));
        return SMC_ERR_NOMEM;
    }
    const double* rows = f->a.summ + (size_t)island * (f->a.T + 1) * SUMM_STRIDE;
    SMC_LAUNCH(k_f_one_trajectory, dim3(1), dim3(64), st, f->a, island, (i64)n_last, t, rows, buf);
    hipError_t rc = hipMemcpyAsync(out_host, buf, (size_t)t * f->a.dx * 8, hipMemcpyDeviceToHost, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    (void)hipFree(buf);
    SMC_HIP_CHECK(rc);
    return SMC_OK;
}

// Backward sampling over the resident history (smc_smooth.h).  Workspaces come from the context's pool and are used
// on its stream only; the one synchronisation is the download at the end.  The sm_* helpers serve all the smoothing
// entries; a check hands back the text of the first refusal (null: none) and the entry raises it with SMC_REQUIRE.
static const char* sm_check_filter(smc_filter* f, int island, const void* idx_out_host, bool whole_history = true)
{
    if (!(f && idx_out_host)) return "null argument";
    if (!(!f->plan.sqmc())) return "SQMC filters are not supported (backward_sampling_qmc is a different algorithm)";
    if (!(f->kind != SMC_MODEL_SVLEVERAGE)) return "model kind SVLEVERAGE is not supported: its transition reads y_{t-1}";
    if (!(f->kind != SMC_MODEL_MVLINGAUSS)) return "model kind MVLINGAUSS is not supported: univariate models only";
    if (!sm_kind_ok(f->kind)) return "model kind is not supported";
    if (!(!whole_history || f->a.hist == 1)) return "the filter was created without a whole history (keep_history = 1)";
    if (!(island >= 0 && island < f->a.n_islands)) return "island out of range";
    return nullptr;
}
static const char* sm_check_idx_last(smc_filter* f, int64_t M, const int64_t* idx_last_host)
{
    for (i64 m = 0; idx_last_host && m < M; ++m)
        if (!(idx_last_host[m] >= 0 && idx_last_host[m] < f->a.N)) return "idx_last out of range";
    return nullptr;
}
// what every launch of one call shares
static SmArgs sm_args(smc_filter* f, int island, int64_t M, uint64_t seed, const u64* cdf)
{
    SmArgs s{};
    s.p = f->a.params + (size_t)island * PARAM_STRIDE;
    s.N = f->a.N; s.M = M;
    s.seed = seed;
    s.island = (u32)(f->a.island_offset + island);
    s.kform = f->plan.two_level ? 1 : 0;
    s.shift = sm_shift(f->a.N);
    s.nsteps = 1;
    s.cdf = cdf;
    return s;
}
// every entry opens with this: the filter's device, and the summary row behind the last step
static void sm_enter(smc_filter* f) { if (f) { (void)hipSetDevice(f->ctx->device); flush_rows(f); } }
// an island's summary rows, its arrays of step t, and &aux[t] (or null)
static const double* sm_rows(smc_filter* f, int island) { return f->a.summ + (size_t)island * (f->a.T + 1) * SUMM_STRIDE; }
static const double* sm_X(smc_filter* f, int island, i64 t) { return f_X(f->a, t) + (size_t)island * f->a.N; }
static const double* sm_lw(smc_filter* f, int island, i64 t) { return f_lw(f->a, t) + (size_t)island * f->a.N; }
static const u32* sm_A(smc_filter* f, int island, i64 t) { return f_A(f->a, t) + (size_t)island * f->a.N; }
static const double* sm_aux(smc_filter* f, i64 t) { return f->a.aux ? f->a.aux + t : nullptr; }
// cdf = the integer CDF of the weights (lw, row) normalise to
static void sm_cdf_of(smc_filter* f, const double* lw, const double* row, const SmArgs& s, u64* tot, u64* cdf)
{
    const i64 N = f->a.N;
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    hipStream_t st = f->ctx->stream;
    SMC_LAUNCH(k_sm_cdf_totals, dim3(nch), dim3(SMC_BLOCK), st, lw, row, N, s.kform, s.shift, tot);
    SMC_LAUNCH(k_sm_cdf_scan, dim3(nch), dim3(SMC_BLOCK), st, lw, row, N, s.kform, s.shift, (const u64*)tot, cdf);
}
// cdf = the integer CDF of W_step
static void sm_weights_cdf(smc_filter* f, int island, i64 step, const SmArgs& s, u64* tot, u64* cdf)
{
    sm_cdf_of(f, sm_lw(f, island, step), sm_rows(f, island) + (size_t)step * SUMM_STRIDE, s, tot, cdf);
}
// last row: M iid draws from W_{t-1} (smoothing.py:278-281), or the caller's indices
static int sm_last_row(smc_filter* f, int island, SmArgs& s, i64* idx, const int64_t* idx_last_host, const double* d_ulast,
                       u64* tot, u64* cdf)
{
    const i64 t = f->t_host, M = s.M;
    hipStream_t st = f->ctx->stream;
    if (idx_last_host) {
        SMC_HIP_CHECK(hipMemcpyAsync(idx + (size_t)(t - 1) * M, idx_last_host, (size_t)M * 8, hipMemcpyHostToDevice, st));
    } else {
        sm_weights_cdf(f, island, t - 1, s, tot, cdf);
        s.t = (u32)(t - 1);
        s.u = d_ulast;
        s.idx_out = idx + (size_t)(t - 1) * M;
        SMC_LAUNCH(k_sm_draw_last, dim3((unsigned)((M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, s);
    }
    return SMC_OK;
}
// the history pointers of backward step b: X_b, lw_b against the row drawn for step b + 1
static void sm_step_args(smc_filter* f, int island, i64 b, i64* idx, SmArgs& s)
{
    const double* rows = sm_rows(f, island);
    s.t = (u32)b;
    s.Xt = sm_X(f, island, b);
    s.lwt = sm_lw(f, island, b);
    s.Xn = sm_X(f, island, b + 1);
    s.An = sm_A(f, island, b + 1);
    s.rowt = rows + (size_t)b * SUMM_STRIDE;
    s.rown = rows + (size_t)(b + 1) * SUMM_STRIDE;
    s.aux = sm_aux(f, b + 1);
    s.idx_next = idx + (size_t)(b + 1) * s.M;
    s.idx_out = idx + (size_t)b * s.M;
}
// paths = X_s[idx[s]] if asked for, then the one download and synchronisation of a call
static int sm_download(smc_filter* f, int island, i64 M, const i64* idx, double* paths, int64_t* idx_out_host,
                       double* paths_out_host)
{
    const i64 t = f->t_host;
    hipStream_t st = f->ctx->stream;
    if (paths)
        SMC_LAUNCH(k_sm_paths, dim3((unsigned)(((size_t)t * M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, f->a, island,
                   t, (i64)M, idx, paths);
    SMC_LAUNCH_CHECK();
    SMC_HIP_CHECK(hipMemcpyAsync(idx_out_host, idx, (size_t)t * M * 8, hipMemcpyDeviceToHost, st));
    if (paths) SMC_HIP_CHECK(hipMemcpyAsync(paths_out_host, paths, (size_t)t * M * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}
// The rejection stage of `steps` backward steps: their counters (ctr, a row of SM_CTR_STRIDE per step, the caller zeroes
// them) and the two lists from the pool, the trials clamped.  u_prop, u_acc, logC and ctr are the caller's, per step.
static SmRej sm_rej_stage(SmPool& pool, size_t steps, i64 M, int64_t& max_trials, u64** ctr)
{
    SmRej r{};
    pool.get(steps * SM_CTR_STRIDE, ctr);
    pool.get((size_t)M, &r.listA);
    pool.get((size_t)M, &r.listB);
    if (max_trials > SM_REJ_MAX_TRIALS) max_trials = SM_REJ_MAX_TRIALS;    // then the exact draw: still the exact law
    r.max_trials = max_trials;
    r.solo = max_trials < sm_reject_solo_trials() ? max_trials : sm_reject_solo_trials();
    return r;
}
// loc[n] = the transition's location at source n (k_os_loc); returns the slot of its scale in the params row
static int sm_launch_loc(smc_filter* f, const SmArgs& s, double* loc)
{
    int slot = 1;
    sm_with_kind(f->kind, [&](auto k) {
        SMC_LAUNCH((k_os_loc<F_VAL(k)>), dim3((unsigned)((s.N + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK),
                   f->ctx->stream, s, loc);
        slot = sm_scale_slot<F_VAL(k)>();
    });
    return slot;
}

int smc_filter_backward_sample(smc_filter* f, int island, int method, int64_t M, int nsteps, uint64_t seed,
                               const int64_t* idx_last_host, const double* u_last_host,
                               const double* u_host, const double* u_acc_host,
                               int64_t* idx_out_host, double* paths_out_host)
{
    sm_enter(f);
    const char* bad = sm_check_filter(f, island, idx_out_host);
    SMC_REQUIRE(!bad, bad);
    SMC_REQUIRE(method == SMC_BACKWARD_ON2 || method == SMC_BACKWARD_MCMC, "unknown method");
    SMC_REQUIRE(M >= 1 && M < ((int64_t)1 << 31), "M must be at least 1 (and below 2^31)");
    SMC_REQUIRE(nsteps >= 1, "nsteps must be at least 1");
    const i64 t = f->t_host, N = f->a.N;
    SMC_REQUIRE(f->t_host >= 1, "no step has run yet");
    if (method == SMC_BACKWARD_ON2) nsteps = 1;
    SMC_REQUIRE((i64)nsteps * M < ((i64)1 << 32), "nsteps * M must stay below 2^32 (Philox counter)");
    SMC_REQUIRE(!(bad = sm_check_idx_last(f, M, idx_last_host)), bad);
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    const bool mcmc = method == SMC_BACKWARD_MCMC;
    const bool need_cdf = mcmc || !idx_last_host;
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    i64* idx = nullptr;
    u64 *cdf = nullptr, *tot = nullptr;
    double *paths = nullptr, *d_ulast = nullptr, *d_u = nullptr, *d_uacc = nullptr;
    const size_t per_step = (size_t)nsteps * M;
    pool.get((size_t)t * M, &idx);
    if (need_cdf) { pool.get((size_t)N, &cdf); pool.get((size_t)nch, &tot); }
    if (paths_out_host) pool.get((size_t)t * M, &paths);
    if (!idx_last_host) pool.upload(u_last_host, (size_t)M, &d_ulast);
    pool.upload(u_host, (size_t)(t - 1) * per_step, &d_u);
    if (mcmc) pool.upload(u_acc_host, (size_t)(t - 1) * per_step, &d_uacc);
    int rc = pool.status();
    if (rc != SMC_OK) return rc;
    SMC_HIP_CHECK(hipMemsetAsync(idx, 0, (size_t)t * M * 8, st));          // (every index a kernel reads is in range)

    SmArgs s = sm_args(f, island, M, seed, cdf);
    s.nsteps = nsteps;
    if ((rc = sm_last_row(f, island, s, idx, idx_last_host, d_ulast, tot, cdf)) != SMC_OK) return rc;
    for (i64 b = t - 2; b >= 0; --b) {
        if (mcmc) sm_weights_cdf(f, island, b, s, tot, cdf);
        sm_step_args(f, island, b, idx, s);
        s.u = d_u ? d_u + (size_t)b * per_step : nullptr;
        s.u_acc = d_uacc ? d_uacc + (size_t)b * per_step : nullptr;
        sm_with_kind(f->kind, [&](auto k) {
            if (mcmc) SMC_LAUNCH((k_sm_mcmc<F_VAL(k)>), dim3((unsigned)((M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, s);
            else SMC_LAUNCH((k_sm_on2<F_VAL(k)>), dim3((unsigned)M), dim3(SMC_BLOCK), st, s);
        });
    }
    return sm_download(f, island, M, idx, paths, idx_out_host, paths_out_host);
}

// One new trajectory per island in ONE launch (smc_csmc.h, k_csmc_path): the state update of Particle Gibbs for all chains.
// backward = 0: the genealogy of a particle drawn from the last weights; 1: backward sampling, for every island the
// indices smc_filter_backward_sample(SMC_BACKWARD_ON2, M = 1) returns from the same uniforms.
int smc_filter_csmc_paths(smc_filter* f, int backward, uint64_t seed, const double* u_last_host, const double* u_host,
                          int64_t* idx_out_host, double* paths_out_host, double* paths_out_dev)
{
    sm_enter(f);
    SMC_REQUIRE(f && (idx_out_host || paths_out_host || paths_out_dev), "null filter, or no output asked for");
    SMC_REQUIRE(!f->plan.sqmc(), "SQMC filters are not supported");
    SMC_REQUIRE(sm_kind_ok(f->kind), "model kind is not supported: LINGAUSS, STOCHVOL, GORDON, THETALOGISTIC, DISCRETECOX");
    SMC_REQUIRE(f->a.hist == 1, "the filter was created without a whole history (keep_history = 1)");
    SMC_REQUIRE(f->a.N <= F_TILE, "N <= 1024: one workgroup walks an island's history");
    SMC_REQUIRE(f->t_host >= 1, "no step has run yet");
    const i64 t = f->t_host;
    const size_t C = (size_t)f->a.n_islands;
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    i64* idx = nullptr;
    double *paths = paths_out_dev, *d_ulast = nullptr, *d_u = nullptr;
    pool.get(C * t, &idx);
    if (!paths) pool.get(C * t, &paths);
    pool.upload(u_last_host, C, &d_ulast);
    if (backward) pool.upload(u_host, (size_t)(t - 1) * C, &d_u);
    if (pool.status() != SMC_OK) return pool.status();
    const dim3 grid(1, f->a.n_islands);
    const int kform = f->plan.two_level ? 1 : 0, bw = backward ? 1 : 0;
    sm_with_kind(f->kind, [&](auto k) {
        f_with_small_block(f->a.N, [&](auto bs) {
            SMC_LAUNCH((k_csmc_path<F_VAL(k), F_VAL(bs)>), grid, dim3(F_VAL(bs)), st, f->a, t, bw, kform, (u64)seed,
                       (const double*)d_ulast, (const double*)d_u, idx, paths);
        });
    });
    SMC_LAUNCH_CHECK();
    if (idx_out_host) SMC_HIP_CHECK(hipMemcpyAsync(idx_out_host, idx, C * t * 8, hipMemcpyDeviceToHost, st));
    if (paths_out_host) SMC_HIP_CHECK(hipMemcpyAsync(paths_out_host, paths, C * t * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    return SMC_OK;
}

// The hybrid of rejection trials and the exact draw (smc_smooth.h, k_sm_reject_*).  Per backward step: the CDF of W_b,
// then three launches whose grids the host sizes by M -- the lists' counts are read on the device, so the loop has no
// synchronisation.  The counters of all steps are zeroed once, in front of the loop.
int smc_filter_backward_reject(smc_filter* f, int island, int64_t M, int64_t max_trials, uint64_t seed,
                               const double* log_bound_host,
                               const int64_t* idx_last_host, const double* u_last_host,
                               const double* u_prop_host, const double* u_acc_host,
                               const double* u_host,
                               int64_t* idx_out_host, double* paths_out_host,
                               int64_t* nprops_out_host, int64_t* nexact_out_host)
{
    sm_enter(f);
    const char* bad = sm_check_filter(f, island, idx_out_host);
    SMC_REQUIRE(!bad, bad);
    SMC_REQUIRE(M >= 1 && M < ((int64_t)1 << 31), "M must be at least 1 (and below 2^31)");
    SMC_REQUIRE(max_trials >= 1, "max_trials must be at least 1");
    SMC_REQUIRE(f->t_host >= 1, "no step has run yet");
    const i64 t = f->t_host, N = f->a.N;
    SMC_REQUIRE(t < 2 || log_bound_host, "null log_bound: the bounds log C_s, s = 1 .. t - 1, are the caller's");
    SMC_REQUIRE(!(bad = sm_check_idx_last(f, M, idx_last_host)), bad);
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    const size_t nb = (size_t)(t - 1);                                       // backward steps
    i64* idx = nullptr;
    u64 *cdf = nullptr, *tot = nullptr, *ctr = nullptr;
    double *paths = nullptr, *d_ulast = nullptr, *d_u = nullptr, *d_uprop = nullptr, *d_uacc = nullptr, *d_logC = nullptr;
    pool.get((size_t)t * M, &idx);
    pool.get((size_t)N, &cdf);
    pool.get((size_t)nch, &tot);
    SmRej r = sm_rej_stage(pool, nb, M, max_trials, &ctr);
    if (paths_out_host) pool.get((size_t)t * M, &paths);
    if (!idx_last_host) pool.upload(u_last_host, (size_t)M, &d_ulast);
    const size_t per_step = (size_t)max_trials * M;
    if (nb) pool.upload(log_bound_host, nb, &d_logC);
    pool.upload(u_host, nb * M, &d_u);
    pool.upload(u_prop_host, nb * per_step, &d_uprop);
    pool.upload(u_acc_host, nb * per_step, &d_uacc);
    int rc = pool.status();
    if (rc != SMC_OK) return rc;
    SMC_HIP_CHECK(hipMemsetAsync(idx, 0, (size_t)t * M * 8, st));          // (every index a kernel reads is in range)
    SMC_HIP_CHECK(hipMemsetAsync(ctr, 0, (nb ? nb : 1) * SM_CTR_STRIDE * 8, st));

    SmArgs s = sm_args(f, island, M, seed, cdf);
    if ((rc = sm_last_row(f, island, s, idx, idx_last_host, d_ulast, tot, cdf)) != SMC_OK) return rc;
    for (i64 b = t - 2; b >= 0; --b) {
        sm_weights_cdf(f, island, b, s, tot, cdf);
        sm_step_args(f, island, b, idx, s);
        s.u = d_u ? d_u + (size_t)b * M : nullptr;
        r.u_prop = d_uprop ? d_uprop + (size_t)b * per_step : nullptr;
        r.u_acc = d_uacc ? d_uacc + (size_t)b * per_step : nullptr;
        r.logC = d_logC + b;
        r.ctr = ctr + (size_t)b * SM_CTR_STRIDE;
        sm_with_kind(f->kind, [&](auto k) { sm_launch_reject<F_VAL(k)>(st, s, r); });
    }
    std::vector<u64> counts(nb * SM_CTR_STRIDE);
    if (nb && (nprops_out_host || nexact_out_host))
        SMC_HIP_CHECK(hipMemcpyAsync(counts.data(), ctr, nb * SM_CTR_STRIDE * 8, hipMemcpyDeviceToHost, st));
    if ((rc = sm_download(f, island, M, idx, paths, idx_out_host, paths_out_host)) != SMC_OK) return rc;
    for (size_t b = 0; b < nb; ++b) {
        if (nprops_out_host) nprops_out_host[b] = (int64_t)counts[b * SM_CTR_STRIDE + SM_CTR_NPROPS];
        if (nexact_out_host) nexact_out_host[b] = (int64_t)counts[b * SM_CTR_STRIDE + SM_CTR_NEXACT];
    }
    return SMC_OK;
}

// Backward sampling for SQMC filters (smc_smooth_qmc.h): exact FFBS whose lookups are made in the sorted order of each
// step's particles, with the caller's point set.  Per step: the sort, one gather into the one-step slab, one draw launch
// in either geometry.  smc_debug_backward_qmc_timing: HIP events around the sort + gather launches of every step
// (measurements only: tools/ffbs_qmc_perf.py).
static const char* smq_check_filter(smc_filter* f, int island, const void* u_host, const void* idx_out_host)
{
    if (!(f && u_host && idx_out_host)) return "null argument";
    if (!f->plan.sqmc()) return "QMC FFBS requires particles have been Hilbert ordered during the forward pass";
    if (!(f->a.hist == 1)) return "the filter was created without a whole history (keep_history = 1)";
    if (!(f->kind != SMC_MODEL_SVLEVERAGE)) return "model kind SVLEVERAGE is not supported: its transition reads y_{t-1}";
    if (!(f->kind != SMC_MODEL_MVLINGAUSS)) return "model kind MVLINGAUSS is not supported: univariate models only";
    if (!sm_kind_ok(f->kind)) return "model kind is not supported";
    if (!(island >= 0 && island < f->a.n_islands)) return "island out of range";
    return nullptr;
}
static bool g_smq_timing = false;
static double g_smq_sort_ms = 0.0;
int smc_debug_backward_qmc_timing(int enable, double* last_sort_ms)
{
    g_smq_timing = enable != 0;
    if (last_sort_ms) *last_sort_ms = g_smq_sort_ms;
    return SMC_OK;
}
struct SmqEvents {                     // one pair per sorted step, read after the call's synchronisation
    std::vector<hipEvent_t> ev;
    bool on;
    explicit SmqEvents(bool enable) : on(enable) {}
    ~SmqEvents() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark(hipStream_t st)
    {
        hipEvent_t e;
        if (on && hipEventCreate(&e) == hipSuccess) { ev.push_back(e); (void)hipEventRecord(e, st); }
    }
    double total_ms() const
    {
        double ms = 0.0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float d = 0.f;
            if (hipEventElapsedTime(&d, ev[i], ev[i + 1]) == hipSuccess) ms += d;
        }
        return ms;
    }
};

int smc_filter_backward_qmc(smc_filter* f, int island, int64_t M, int geometry, const double* u_host,
                            int64_t* idx_out_host, double* paths_out_host)
{
    sm_enter(f);
    const char* bad = smq_check_filter(f, island, u_host, idx_out_host);
    SMC_REQUIRE(!bad, bad);
    SMC_REQUIRE(M >= 1 && M < ((int64_t)1 << 31), "M must be at least 1 (and below 2^31)");
    SMC_REQUIRE(f->t_host >= 1, "no step has run yet");
    SMC_REQUIRE(geometry >= 0 && geometry <= 2, "geometry must be 0 (auto), 1 (workgroup per trajectory) or 2 (thread per trajectory)");
    const i64 t = f->t_host, N = f->a.N;
    SMC_REQUIRE(N < ((i64)1 << 31), "N must stay below 2^31 (the radix sort)");
    if (geometry == 0) geometry = M >= SMQ_THREAD_MIN_M ? 2 : 1;
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    const unsigned nblkN = (unsigned)((N + SMC_BLOCK - 1) / SMC_BLOCK), nblkM = (unsigned)((M + SMC_BLOCK - 1) / SMC_BLOCK);
    i64* idx = nullptr;
    u64 *cdf = nullptr, *tot = nullptr;
    double *paths = nullptr, *d_u = nullptr, *d_ut = nullptr, *xs = nullptr, *ls = nullptr;
    char* ws = nullptr;
    pool.get((size_t)t * M, &idx);
    pool.get((size_t)N, &cdf);
    pool.get((size_t)nch, &tot);
    pool.get((size_t)N, &xs);
    pool.get((size_t)N, &ls);
    pool.get(smc_rs_ws_bytes(N), &ws);
    pool.get((size_t)t * M, &d_ut);
    if (paths_out_host) pool.get((size_t)t * M, &paths);
    pool.upload(u_host, (size_t)t * M, &d_u);
    int rc = pool.status();
    if (rc != SMC_OK) return rc;
    SMC_HIP_CHECK(hipMemsetAsync(idx, 0, (size_t)t * M * 8, st));          // (every index a kernel reads is in range)
    SMC_LAUNCH(k_smq_transpose, dim3((unsigned)(((size_t)t * M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st,
               (const double*)d_u, (i64)M, t, d_ut);

    SmqEvents events(g_smq_timing);
    SmArgs s = sm_args(f, island, M, 0, cdf);
    for (i64 b = t - 1; b >= 0; --b) {
        u64* order = nullptr;
        events.mark(st);
        if ((rc = smc_rs_sort_ws(f->ctx, sm_X(f, island, b), nullptr, N, 0, ws, nullptr, &order, b != t - 1)) != SMC_OK) {
            smc_set_error("smc_filter_backward_qmc: the sort failed: %s", hipGetErrorString(hipGetLastError()));
            return rc;
        }
        SMC_LAUNCH(k_smq_gather, dim3(nblkN), dim3(SMC_BLOCK), st, (const i64*)order, sm_X(f, island, b), sm_lw(f, island, b), N,
                   xs, ls);
        events.mark(st);
        if (b == t - 1) {
            s.t = (u32)b;
            s.idx_out = idx + (size_t)b * M;
        } else {
            sm_step_args(f, island, b, idx, s);
        }
        s.Xt = xs; s.lwt = ls;                                                // the slab, and what its positions stand for
        s.h = (const i64*)order;
        s.u = d_ut + (size_t)b * M;
        if (b == t - 1) {
            sm_cdf_of(f, ls, sm_rows(f, island) + (size_t)b * SUMM_STRIDE, s, tot, cdf);
            SMC_LAUNCH(k_smq_draw_last, dim3(nblkM), dim3(SMC_BLOCK), st, s);
            continue;
        }
        sm_with_kind(f->kind, [&](auto k) {
            if (geometry == 2) SMC_LAUNCH((k_smq_thread<F_VAL(k)>), dim3(nblkM), dim3(SMC_BLOCK), st, s);
            else SMC_LAUNCH((k_smq_wg<F_VAL(k)>), dim3((unsigned)M), dim3(SMC_BLOCK), st, s);
        });
    }
    rc = sm_download(f, island, M, idx, paths, idx_out_host, paths_out_host);
    if (rc == SMC_OK && events.on) g_smq_sort_ms = events.total_ms();
    return rc;
}

// On-line smoothing (smc_online.h): one update behind the step just run.  Stateless: Phi, X_{t-1} and lw_{t-1} are the
// caller's device arrays, everything else is read from the filter's current step or lives in pool workspaces for the
// duration of the call.  One synchronisation: the download of the K estimates (and what else was asked for).
struct OsParis {                       // the PaRIS draw of one call
    int n_paris;                       // indices per target; 0: no draw (SMC_ONLINE_NAIVE)
    int64_t max_trials;
    double log_bound;
    const double *u_prop, *u_acc, *u;  // the caller's tapes (host) or null
    i64* idx;                          // (N n_paris) the drawn indices
    u64* ctr;                          // the draw's counters (both: for the download)
};
// t == 0: Phi_0 = psi_0(X_0)
static int os_init(smc_filter* f, const OsPsi& psi, const double* X, double* Phi_dev)
{
    SMC_LAUNCH(k_os_init, dim3((unsigned)((f->a.N + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), f->ctx->stream, psi, X, f->a.N,
               Phi_dev);
    return SMC_OK;
}
// SMC_ONLINE_ON2: all pairs, by source slices; s holds the step (Xt, lwt: the previous particles, Xn: the current ones)
static int os_update_on2(smc_filter* f, SmPool& pool, const SmArgs& s, const OsPsi& psi, double* Phi_dev)
{
    const i64 N = s.N;
    const int K = psi.K, KP = K == 1 ? 1 : K <= 4 ? 4 : 8, nslices = os_slices(N);
    hipStream_t st = f->ctx->stream;
    double *loc = nullptr, *part = nullptr;
    pool.get((size_t)N, &loc);
    pool.get((size_t)nslices * N * OS_PART(KP), &part);
    if (pool.status() != SMC_OK) return pool.status();
    OsOn2 o{};
    o.X = s.Xn; o.Xprev = s.Xt; o.lwprev = s.lwt; o.loc = loc; o.Phi = Phi_dev;
    o.part = part; o.p = s.p; o.slot = sm_launch_loc(f, s, loc); o.N = N; o.K = K;
    const i64 ntile = (N + OS_TILE - 1) / OS_TILE;
    o.per_slice = ((ntile + nslices - 1) / nslices) * OS_TILE;
    const int used = (int)((N + o.per_slice - 1) / o.per_slice);            // (no empty slice is launched or merged)
    // (the merge reads every partial before it writes a target's Phi, and k_os_on2 is done: Phi_dev in place)
    if (KP == 1) os_launch_on2<1>(st, o, used, psi, Phi_dev);
    else if (KP == 4) os_launch_on2<4>(st, o, used, psi, Phi_dev);
    else os_launch_on2<8>(st, o, used, psi, Phi_dev);
    return SMC_OK;
}
// SMC_ONLINE_PARIS: d.n_paris indices per target by rejection, the targets of s.idx_next drawing from W_{t-1}
static int os_paris_draw(smc_filter* f, SmPool& pool, SmArgs& s, OsParis& d)
{
    const i64 N = s.N, M = s.M;
    hipStream_t st = f->ctx->stream;
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    u64 *cdf = nullptr, *tot = nullptr;
    i64* targets = nullptr;
    double *d_u = nullptr, *d_uprop = nullptr, *d_uacc = nullptr, *d_logC = nullptr;
    pool.get((size_t)N, &cdf);
    pool.get((size_t)nch, &tot);
    SmRej r = sm_rej_stage(pool, 1, M, d.max_trials, &d.ctr);
    pool.get((size_t)M, &targets);
    pool.get((size_t)M, &d.idx);
    pool.upload(&d.log_bound, 1, &d_logC);
    pool.upload(d.u, (size_t)M, &d_u);
    pool.upload(d.u_prop, (size_t)d.max_trials * M, &d_uprop);
    pool.upload(d.u_acc, (size_t)d.max_trials * M, &d_uacc);
    if (pool.status() != SMC_OK) return pool.status();
    SMC_HIP_CHECK(hipMemsetAsync(d.idx, 0, (size_t)M * 8, st));                // (every index a kernel reads is in range)
    SMC_HIP_CHECK(hipMemsetAsync(d.ctr, 0, SM_CTR_STRIDE * 8, st));
    SMC_LAUNCH(k_os_targets, dim3((unsigned)((M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, M, d.n_paris, targets);
    s.cdf = cdf;
    sm_cdf_of(f, s.lwt, s.rowt, s, tot, cdf);
    s.u = d_u; s.idx_next = targets; s.idx_out = d.idx;
    r.u_prop = d_uprop; r.u_acc = d_uacc; r.logC = d_logC; r.ctr = d.ctr;
    sm_with_kind(f->kind, [&](auto k) { sm_launch_reject<F_VAL(k)>(st, s, r); });
    return SMC_OK;
}
// SMC_ONLINE_NAIVE, SMC_ONLINE_PARIS: Phi gathered along the ancestors, or the drawn indices (d.n_paris of them)
static int os_update_gather(smc_filter* f, SmPool& pool, SmArgs& s, const OsPsi& psi, double* Phi_dev, OsParis& d)
{
    const i64 N = s.N;
    hipStream_t st = f->ctx->stream;
    double* Phi_new = nullptr;
    pool.get((size_t)N * psi.K, &Phi_new);
    const int rc = d.n_paris ? os_paris_draw(f, pool, s, d) : pool.status();
    if (rc != SMC_OK) return rc;
    SMC_LAUNCH(k_os_gather, dim3((unsigned)((N + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, psi, s.Xn, s.Xt,
               (const double*)Phi_dev, s.An, s.rown, (const i64*)d.idx, d.n_paris, N, Phi_new);
    SMC_HIP_CHECK(hipMemcpyAsync(Phi_dev, Phi_new, (size_t)N * psi.K * 8, hipMemcpyDeviceToDevice, st));
    return SMC_OK;
}
int smc_filter_online_smooth(smc_filter* f, int island, int method, const smc_addfunc* psi_host,
                             double* Phi_dev, double* Xprev_dev, double* lwprev_dev,
                             int n_paris, int64_t max_trials, uint64_t seed, double log_bound,
                             const double* u_prop_host, const double* u_acc_host, const double* u_host,
                             int64_t* idx_out_host, int64_t* nprop_out, double* est_out_host)
{
    sm_enter(f);
    const char* bad = sm_check_filter(f, island, est_out_host, false);
    SMC_REQUIRE(!bad, bad);
    SMC_REQUIRE(psi_host && Phi_dev && Xprev_dev && lwprev_dev, "null argument");
    SMC_REQUIRE(psi_host->K >= 1 && psi_host->K <= OS_KMAX, "K must be 1 .. 8");
    SMC_REQUIRE(method == SMC_ONLINE_NAIVE || method == SMC_ONLINE_ON2 || method == SMC_ONLINE_PARIS, "unknown method");
    SMC_REQUIRE(f->t_host >= 1, "no step has run yet");
    const bool paris = method == SMC_ONLINE_PARIS;
    const i64 N = f->a.N, t = f->t_host - 1;
    if (paris) {
        SMC_REQUIRE(n_paris >= 1, "n_paris must be at least 1");
        SMC_REQUIRE(max_trials >= 1, "max_trials must be at least 1");
        SMC_REQUIRE(N * (i64)n_paris < ((i64)1 << 31), "N n_paris must stay below 2^31");
    }
    OsPsi psi{};
    const int K = psi.K = psi_host->K;
    memcpy(psi.c0, psi_host->c0, sizeof psi.c0);
    memcpy(psi.c, psi_host->c, sizeof psi.c);
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    const int nest = (int)((N + OS_EST_CHUNK - 1) / OS_EST_CHUNK);
    const double *X = sm_X(f, island, t), *lw = sm_lw(f, island, t);
    const double* rows = sm_rows(f, island);
    const double* row = rows + (size_t)t * SUMM_STRIDE;
    double *est = nullptr, *epart = nullptr;
    pool.get((size_t)OS_KMAX, &est);
    pool.get((size_t)nest * OS_KMAX, &epart);
    int rc = pool.status();
    if (rc != SMC_OK) return rc;
    OsParis d{paris ? n_paris : 0, max_trials, log_bound, u_prop_host, u_acc_host, u_host, nullptr, nullptr};
    const i64 M = N * d.n_paris;
    if (t == 0) {
        rc = os_init(f, psi, X, Phi_dev);
    } else {
        SmArgs s = sm_args(f, island, M, seed, nullptr);
        s.t = (u32)(t - 1);
        s.Xt = Xprev_dev; s.lwt = lwprev_dev; s.Xn = X;
        s.An = sm_A(f, island, t);
        s.rowt = rows + (size_t)(t - 1) * SUMM_STRIDE;
        s.rown = row;
        s.aux = sm_aux(f, t);
        rc = method == SMC_ONLINE_ON2 ? os_update_on2(f, pool, s, psi, Phi_dev) : os_update_gather(f, pool, s, psi, Phi_dev, d);
    }
    if (rc != SMC_OK) return rc;
    SMC_LAUNCH(k_os_est_partials, dim3((unsigned)nest), dim3(SMC_BLOCK), st, lw, row, (const double*)Phi_dev, N, K,
               f->plan.two_level ? 1 : 0, epart);
    SMC_LAUNCH(k_os_est_final, dim3(1), dim3(64), st, (const double*)epart, nest, K, est);
    SMC_LAUNCH_CHECK();
    SMC_HIP_CHECK(hipMemcpyAsync(Xprev_dev, X, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
    SMC_HIP_CHECK(hipMemcpyAsync(lwprev_dev, lw, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
    u64 counts[SM_CTR_STRIDE] = {0, 0, 0, 0};
    if (d.ctr && nprop_out) SMC_HIP_CHECK(hipMemcpyAsync(counts, d.ctr, sizeof counts, hipMemcpyDeviceToHost, st));
    if (d.idx && idx_out_host) SMC_HIP_CHECK(hipMemcpyAsync(idx_out_host, d.idx, (size_t)M * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipMemcpyAsync(est_out_host, est, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    if (nprop_out) *nprop_out = (int64_t)counts[SM_CTR_NPROPS];
    return SMC_OK;
}

// Two-filter smoothing (smc_twofilter.h).  Reads both filters only; workspaces from the pool, launches on the context's
// stream (the two filters share it: one stream orders the call).  One synchronisation: the download of the estimates,
// the ESS and, when asked for, the pair indices.
struct TfWork {                        // what the two item functions share
    const double* Xi;                  // (Ni) the information filter's particles
    double *lwi, *bmaxi;               // (Ni) their log-weights less log gamma plus modif_info; the block maxima of those
    double *gmax, *items;              // 3 maxima: of the items, and one for each CDF of the sampled pairs; (nitems, K + 2)
    double *d_mf, *d_mi;               // modif_forward, modif_info on the device or null
    i64 Ni;
};
// SMC_TWOFILTER_ON2: one item per particle of the information filter, all forward particles summed over in slices
static int tf_items_on2(smc_filter* f, SmPool& pool, const SmArgs& s, const OsPsi& psi, const TfWork& w)
{
    const i64 Ni = w.Ni, Nf = s.N;
    const unsigned nbi = (unsigned)((Ni + SMC_BLOCK - 1) / SMC_BLOCK);
    const int nslices = tf_slices(Ni, Nf);
    hipStream_t st = f->ctx->stream;
    double *loc = nullptr, *part = nullptr;
    pool.get((size_t)Nf, &loc);
    pool.get((size_t)nslices * Ni * 4, &part);
    if (pool.status() != SMC_OK) return pool.status();
    TfOn2 o{};
    o.Xi = w.Xi; o.Xf = s.Xt; o.lwf = s.lwt; o.loc = loc; o.part = part; o.p = s.p; o.slot = sm_launch_loc(f, s, loc);
    o.Ni = Ni; o.Nf = Nf;
    const i64 ntile = (Nf + SMC_BLOCK - 1) / SMC_BLOCK;
    o.per_slice = ((ntile + nslices - 1) / nslices) * SMC_BLOCK;
    const int used = (int)((Nf + o.per_slice - 1) / o.per_slice);               // (no empty slice is launched or merged)
    SMC_LAUNCH(k_tf_on2, dim3(nbi, (unsigned)used), dim3(SMC_BLOCK), st, o);
    SMC_LAUNCH(k_tf_merge, dim3(nbi), dim3(SMC_BLOCK), st, psi, w.Xi, (const double*)w.lwi, (const double*)part, used, Ni, w.items);
    return SMC_OK;
}
// SMC_TWOFILTER_ON: one item per pair (J, I) -- the caller's, or drawn from the two (modified) weight vectors.  q.J and
// q.I stay for the download.
static int tf_items_pairs(smc_filter* f, int island, SmPool& pool, const SmArgs& s, const OsPsi& psi, const TfWork& w,
                          const int64_t* idx_fwd_host, const int64_t* idx_info_host, const double* u_fwd_host,
                          const double* u_info_host, TfPairs& q)
{
    const i64 Ni = w.Ni, Nf = s.N, P = s.M;
    const bool given = idx_fwd_host || idx_info_host;
    hipStream_t st = f->ctx->stream;
    const i64 Nmax = Nf > Ni ? Nf : Ni;
    const unsigned nbf = (unsigned)((Nf + SMC_BLOCK - 1) / SMC_BLOCK);
    i64 *J_in = nullptr, *I_in = nullptr;
    u64 *cdf_f = nullptr, *cdf_i = nullptr, *tot = nullptr;
    double *d_uf = nullptr, *d_ui = nullptr, *lf = nullptr, *bmaxf = nullptr;
    pool.get((size_t)P, &q.J);
    pool.get((size_t)P, &q.I);
    if (given) {
        pool.upload((const i64*)idx_fwd_host, (size_t)P, &J_in);
        pool.upload((const i64*)idx_info_host, (size_t)P, &I_in);
    } else {
        pool.upload(u_fwd_host, (size_t)P, &d_uf);
        pool.upload(u_info_host, (size_t)P, &d_ui);
        pool.get((size_t)Nf, &cdf_f);
        pool.get((size_t)Ni, &cdf_i);
        pool.get((size_t)((Nmax + SM_CHUNK - 1) / SM_CHUNK), &tot);
        if (w.d_mf) { pool.get((size_t)Nf, &lf); pool.get((size_t)nbf, &bmaxf); }
    }
    if (pool.status() != SMC_OK) return pool.status();
    if (!given) {
        if (w.d_mf) {
            const TfGamma none{0.0, 0.0, 0.0, 0};
            SMC_LAUNCH(k_tf_lwi, dim3(nbf), dim3(SMC_BLOCK), st, s.lwt, s.Xt, none, (const double*)w.d_mf, Nf, lf, bmaxf);
            tf_cdf_of(st, lf, bmaxf, Nf, w.gmax + 1, tot, cdf_f);
        } else {
            sm_weights_cdf(f, island, s.t, s, tot, cdf_f);
        }
        tf_cdf_of(st, w.lwi, w.bmaxi, Ni, w.gmax + 2, tot, cdf_i);               // (the stream orders the two uses of tot)
        q.cdf_f = cdf_f; q.cdf_i = cdf_i;
    }
    q.Xi = w.Xi; q.u_f = d_uf; q.u_i = d_ui; q.J_in = J_in; q.I_in = I_in; q.mf = w.d_mf; q.mi = w.d_mi;
    q.items = w.items; q.Ni = Ni; q.P = P;
    sm_with_kind(f->kind, [&](auto k) {
        SMC_LAUNCH((k_tf_pairs<F_VAL(k)>), dim3((unsigned)((P + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, s, q, psi);
    });
    return SMC_OK;
}
int smc_filter_two_filter(smc_filter* f, int island, smc_filter* info, int island_info, int64_t t, int method,
                          const smc_addfunc* phi, const double* loggamma3,
                          const double* modif_forward_host, const double* modif_info_host,
                          int64_t npairs, uint64_t seed,
                          const double* u_fwd_host, const double* u_info_host,
                          const int64_t* idx_fwd_host, const int64_t* idx_info_host,
                          int64_t* idx_fwd_out_host, int64_t* idx_info_out_host,
                          double* est_out_host, double* ess_out_host)
{
    sm_enter(f);
    SMC_REQUIRE(f && info && phi && loggamma3 && est_out_host, "null argument");
    SMC_REQUIRE(f->ctx == info->ctx, "the two filters must share a context");
    flush_rows(info);
    const char* bad = sm_check_filter(f, island, est_out_host);
    SMC_REQUIRE(!bad, bad);
    SMC_REQUIRE(info->kind != SMC_MODEL_MVLINGAUSS, "the information filter must be univariate");
    SMC_REQUIRE(!info->plan.sqmc(), "SQMC information filters are not supported");
    SMC_REQUIRE(info->a.hist == 1, "the information filter was created without a whole history (keep_history = 1)");
    SMC_REQUIRE(island_info >= 0 && island_info < info->a.n_islands, "island_info out of range");
    SMC_REQUIRE(method == SMC_TWOFILTER_ON2 || method == SMC_TWOFILTER_ON, "unknown method");
    SMC_REQUIRE(phi->K >= 1 && phi->K <= OS_KMAX, "K must be 1 .. 8");
    SMC_REQUIRE(t >= 0 && t <= f->t_host - 2, "t must be in range 0 .. T - 2, T the steps the forward filter has run");
    const i64 ti = f->t_host - 2 - t;
    SMC_REQUIRE(ti < info->t_host, "step T - 2 - t of the information filter has not run");
    const bool on = method == SMC_TWOFILTER_ON;
    const i64 Nf = f->a.N, Ni = info->a.N, P = on ? (i64)npairs : 0;
    const bool given = on && (idx_fwd_host || idx_info_host);
    if (on) {
        SMC_REQUIRE(npairs >= 1 && npairs < ((int64_t)1 << 31), "npairs must be at least 1 (and below 2^31)");
        SMC_REQUIRE(!given || (idx_fwd_host && idx_info_host), "idx_fwd and idx_info are given together");
        for (i64 j = 0; given && j < P; ++j)
            SMC_REQUIRE(idx_fwd_host[j] >= 0 && idx_fwd_host[j] < Nf && idx_info_host[j] >= 0 && idx_info_host[j] < Ni,
                        "pair index out of range");
    }
    OsPsi psi{};
    const int K = psi.K = phi->K;
    memcpy(psi.c, phi->c, sizeof psi.c);
    hipStream_t st = f->ctx->stream;
    SmPool pool(f->ctx);
    const double* lwg = sm_lw(info, island_info, ti);
    const unsigned nbi = (unsigned)((Ni + SMC_BLOCK - 1) / SMC_BLOCK);
    const i64 nitems = on ? P : Ni;
    const int nchunks = (int)((nitems + TF_CHUNK - 1) / TF_CHUNK);
    TfWork w{};
    w.Xi = sm_X(info, island_info, ti);
    w.Ni = Ni;
    double *out = nullptr, *cmax = nullptr, *cpart = nullptr;
    pool.get((size_t)Ni, &w.lwi);
    pool.get((size_t)nbi, &w.bmaxi);
    pool.get((size_t)3, &w.gmax);
    pool.get((size_t)OS_KMAX + 1, &out);
    pool.get((size_t)nitems * (K + 2), &w.items);
    pool.get((size_t)nchunks, &cmax);
    pool.get((size_t)nchunks * TF_PART, &cpart);
    if (on) { pool.upload(modif_forward_host, (size_t)Nf, &w.d_mf); pool.upload(modif_info_host, (size_t)Ni, &w.d_mi); }
    int rc = pool.status();
    if (rc != SMC_OK) return rc;
    const TfGamma gam{loggamma3[0], loggamma3[1], loggamma3[2], 1};
    SMC_LAUNCH(k_tf_lwi, dim3(nbi), dim3(SMC_BLOCK), st, lwg, w.Xi, gam, (const double*)w.d_mi, Ni, w.lwi, w.bmaxi);
    SmArgs s = sm_args(f, island, P, seed, nullptr);
    s.t = (u32)t;
    s.Xt = sm_X(f, island, t); s.lwt = sm_lw(f, island, t);
    s.aux = sm_aux(f, t + 1);
    TfPairs q{};
    rc = on ? tf_items_pairs(f, island, pool, s, psi, w, idx_fwd_host, idx_info_host, u_fwd_host, u_info_host, q)
            : tf_items_on2(f, pool, s, psi, w);
    if (rc != SMC_OK) return rc;
    SMC_LAUNCH(k_tf_item_max, dim3((unsigned)nchunks), dim3(SMC_BLOCK), st, (const double*)w.items, K + 2, nitems, cmax);
    SMC_LAUNCH(k_tf_max_final, dim3(1), dim3(SMC_BLOCK), st, (const double*)cmax, (i64)nchunks, w.gmax);
    SMC_LAUNCH(k_tf_item_sums, dim3((unsigned)nchunks), dim3(SMC_BLOCK), st, (const double*)w.items, K + 2, nitems, K,
               (const double*)w.gmax, cpart);
    SMC_LAUNCH(k_tf_final, dim3(1), dim3(64), st, (const double*)cpart, nchunks, K, out);
    SMC_LAUNCH_CHECK();
    double res[OS_KMAX + 1];
    SMC_HIP_CHECK(hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, st));
    if (on && idx_fwd_out_host) SMC_HIP_CHECK(hipMemcpyAsync(idx_fwd_out_host, q.J, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    if (on && idx_info_out_host) SMC_HIP_CHECK(hipMemcpyAsync(idx_info_out_host, q.I, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    SMC_HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) est_out_host[k] = res[k];
    if (ess_out_host) *ess_out_host = res[OS_KMAX];
    return SMC_OK;
}

int smc_filter_info(smc_filter* f, double* bytes_per_particle_step, int* kernels_per_step)
{
    SMC_REQUIRE(f, "null filter");
    if (bytes_per_particle_step) *bytes_per_particle_step = 16.0 * f->a.dx + 40.0;
    if (kernels_per_step) *kernels_per_step = philox_multinomial(f->a) ? 5 : 3;
    return SMC_OK;
}

int smc_filter_profile(smc_filter* f, int enable)
{
    SMC_REQUIRE(f, "null filter");
    SMC_REQUIRE(!(enable && f->xstar), "a conditional filter (smc_filter_set_conditional) cannot be profiled per step");
    f->prof = enable != 0;
    f->prof_n = 0;
    if (f->prof && f->ev.empty()) {
        f->ev.resize(3 * PROF_MAX);
        for (auto& e : f->ev) SMC_HIP_CHECK(hipEventCreate(&e));
    }
    return SMC_OK;
}

int smc_filter_strict_stats(smc_filter* f, int32_t island, int64_t* exact_path, int64_t* exceptions)
{
    SMC_REQUIRE(f && exact_path && exceptions, "null argument");
    SMC_REQUIRE(f->plan.strict() && f->plan.strict_form != STRICT_LITERAL, "not a strict_ancestors filter");
    SMC_REQUIRE(island >= 0 && island < f->a.n_islands, "island out of range");
    const SqxArgs q = sqx_carve((void*)(f->strict_ws + 2 * (size_t)f->a.n_islands * f->a.N), f->a.N, f->a.n_islands);
    unsigned long long c[2] = {0ull, 0ull};
    SMC_HIP_CHECK(hipMemcpyAsync(c, q.ctr + (size_t)island * 4 + 2, 16, hipMemcpyDeviceToHost, f->ctx->stream));
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    *exact_path = (int64_t)c[0];
    *exceptions = (int64_t)c[1];
    return SMC_OK;
}

int smc_filter_describe(smc_filter* f, char* out, size_t n)
{
    SMC_REQUIRE(f && out && n > 0, "null argument");
    const StepPlan& p = f->plan;
    const bool mv = f->kind == SMC_MODEL_MVLINGAUSS;
    const bool draws = draws_spacings(f);
    const std::string reduce = p.reduce == REDUCE_WIDE ? "k_reduce2w+" : p.reduce == REDUCE_NARROW ? "k_reduce2+" : "";
    const std::string mv_chunks = " [mv_chunks=" + std::to_string(f->a.mv_chunks) + "]";
    const char* ancestors = p.resampler == RS_FUSED ? "k_ancestors<fused>" : p.resampler == RS_PREPARE ? "k_prepare+k_ancestors"
                            : p.resampler == RS_WIDE ? "k_ancestors2w" : "k_ancestors2";
    // (the strict kinds do not list their spacings and moments launches, SQMC on the flat step not its moments: kept as
    //  they are, tests and the benchmark's model compare these strings)
    std::string s;
    if (f->xstar) s = "k_csmc_small";
    else if (small_filter_ok(f)) s = "k_filter_small";
    else if (p.sq_flat)
        s = std::string(mv ? "smc_hilbert_sort" : "k_rs_sort") + "+k_sobol+k_sqmv_tapes+" + ancestors + "+k_sqmv_compose+" +
            (mv ? "k_propagate_mv" + mv_chunks : std::string("k_propagate"));
    else if (p.kind == STEP_SQMC) {
        s = "k_rs_sort+k_sq_permute+" + reduce + "k_ancestors2+k_propagate";
        if (f->a.mom) s += "+k_f_moments_partials+k_f_moments_final";
    } else if (p.kind == STEP_STRICT) {
        s = reduce + (p.strict_form == STRICT_LITERAL     ? "k_strict_W+k_strict_cdf+k_strict_search_S"
                      : p.strict_form == STRICT_TWO_LEVEL ? "k_strict_classify+k_strict_search"
                                                          : "k_strict_W+k_sqx_classify+k_sqx_fill+k_strict_search_S") + "+k_propagate";
    } else {
        if (draws && p.spacings == SP_ONEPASS_MERGED) s = "k_f_spacing_onepass<with k_reduce2>+";
        else s = (!draws ? "" : p.spacings == SP_THREE_PASS ? "k_f_spacing_sums+k_f_spacing_scan+k_f_spacing_write+"
                                                              : "k_f_spacing_onepass+") + reduce;
        s += ancestors;
        if (mv && f->fk == SMC_FK_APF) s = "k_mv_aux+k_mv_aux_restate+" + s;
        s += mv ? (p.mv_collapsed ? "+k_propagate_mv<collapsed>" : "+k_propagate_mv") : "+k_propagate";
        if (mv) s += mv_chunks + (f->a.mv_diag ? " [diagonal factors]" : "");
        if (f->a.mom) s += "+k_f_moments_partials+k_f_moments_final";
    }
    snprintf(out, n, "%s", s.c_str());
    return SMC_OK;
}

int smc_filter_kernel_ms(smc_filter* f, double* move_ms_avg, double* prepare_ms_avg,
                         int64_t* n_samples)
{
    SMC_REQUIRE(f && move_ms_avg && prepare_ms_avg && n_samples, "null argument");
    SMC_HIP_CHECK(hipStreamSynchronize(f->ctx->stream));
    double whole = 0.0, pre = 0.0, post = 0.0;
    int nw = 0, np = 0, nq = 0;
    for (int k = 0; k < f->prof_n; ++k) {
        float a = 0.f;
        if (k % 3 == 1) {
            SMC_HIP_CHECK(hipEventElapsedTime(&a, f->ev[3 * k], f->ev[3 * k + 1]));
            pre += a; ++np;
        } else if (k % 3 == 2) {
            SMC_HIP_CHECK(hipEventElapsedTime(&a, f->ev[3 * k + 1], f->ev[3 * k + 2]));
            post += a; ++nq;
        } else {
            SMC_HIP_CHECK(hipEventElapsedTime(&a, f->ev[3 * k], f->ev[3 * k + 2]));
            whole += a; ++nw;
        }
    }
    *n_samples = f->prof_n;
    const double w = nw ? whole / nw : 0.0, p = np ? pre / np : 0.0, q = nq ? post / nq : 0.0;
    *move_ms_avg = (nw && np) ? w - p : 0.0;
    *prepare_ms_avg = (nw && nq) ? w - q : 0.0;
    f->prof_n = 0;
    return SMC_OK;
}

}  // extern "C"
