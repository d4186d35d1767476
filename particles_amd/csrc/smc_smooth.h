// smc_smooth.h -- backward sampling over the resident particle history (keep_history = 1):
// particles/smoothing.py:278-423, ParticleHistory.backward_sampling_ON2 (exact FFBS),
// backward_sampling_mcmc (independent Metropolis steps, Dau & Chopin 2022) and backward_sampling_reject
// (their hybrid: rejection trials, then the exact draw).  Host side: smc_filter_backward_sample and
// smc_filter_backward_reject in smc_filter.hip.  The kernels read the history and write their
// own workspaces only.
//
// Every draw is an inverse-CDF lookup of ONE uniform in an INTEGER CDF, so the drawn index is a
// function of (history, uniform) alone -- not of the launch geometry or the order of a sum:
//   q_n = rint(e_n 2^s), s = 61 - ceil(log2 N)     e_n in [0, 1 + eps]: the N terms sum below 2^62
//   Q   = sum q_n                                   64-bit integers: exact in any order
//   thr = floor(u Q)                                the 53-bit significand of u times Q, 128 bits, shifted
//   n*  = the first n whose inclusive prefix exceeds thr
// q_n = 0 is never drawn (its prefix does not move), u >= 1 is held to thr = Q - 1: the last n with
// q_n > 0.  Q = 0 (no finite weight at all: the reference's weights are NaN then) gives N - 1.
//   e_n: ON2   exp(l_n - max l), l_n = lw_t[n] + log p_{t+1}(x_{t+1} | X_t[n])       (smoothing.py:307-310)
//        W_t   exp(lw_t[n] - m) / s exactly as k_f_write_W forms SMC_FIELD_W          (last row, MCMC proposals)
//
// Uniforms: a replay tape, or Philox stream SMC_STREAM_BACKWARD with counter
// (i M + m, t, island, 3): word x01 -> [0, 1) (index / proposal), word x23 -> (0, 1) (acceptance);
// i = Metropolis step, 0 for ON2 and for the last row.  Rejection trials have a stream of their own
// (SMC_STREAM_REJECT, see k_sm_reject_solo).
#pragma once
#include "smc_filter_kernels.h"

#define SM_CHUNK (16 * SMC_BLOCK)      /* particles per workgroup of the two CDF launches */

struct SmArgs {
    const double *Xt, *lwt;     // (N) particles and log-weights of step t, this island
    const double* Xn;           // (N) particles of step t + 1
    const u32* An;              // (N) ancestors of step t + 1 (meaningful iff rown[4] != 0)
    const double* rowt;         // summary row of step t: [5] m (kform: K), [6] 1/s
    const double* rown;         // summary row of step t + 1: [4] resampled?
    const double* p;            // the island's params row (PARAM_STRIDE)
    const double* aux;          // &aux[t + 1] or null
    const double *u, *u_acc;    // replay tapes of this step ((nsteps,) M) or null: Philox
    const i64* idx_next;        // (M) indices drawn for step t + 1
    i64* idx_out;               // (M) indices of step t
    const u64* cdf;             // (N) inclusive integer CDF of W_t (MCMC, last row)
    const i64* h;               // null, or (N): Xt, lwt (and cdf) are a slab in sorted order whose position j holds
                                // particle h[j] (smc_smooth_qmc.h); a draw finds a position and stores h[position]
    i64 N, M;
    u64 seed;
    u32 t, island;
    int kform, shift, nsteps;
};

__host__ __device__ __forceinline__ int sm_shift(i64 N)
{
    int c = 0;
    while (((i64)1 << c) < N) ++c;
    return 61 - c;
}
__device__ __forceinline__ u64 sm_q(double e, int shift)
{
    return (e > 0.0) ? (u64)rint(ldexp(e, shift)) : 0ull;       // (NaN weighs 0)
}
// floor(u Q) for any double u, held to [0, Q - 1]; Q >= 1
__device__ __forceinline__ u64 sm_threshold(double u, u64 Q)
{
    if (!(u > 0.0)) return 0ull;
    if (u >= 1.0) return Q - 1;
    const u64 b = (u64)__double_as_longlong(u);
    const int E = (int)((b >> 52) & 0x7ffu);
    const u64 frac = b & 0xfffffffffffffull;
    const u64 sig = E ? (frac | (1ull << 52)) : frac;           // u = sig 2^-k
    const int k = E ? 1075 - E : 1074;                          // >= 53 (u < 1)
    const u64 lo = sig * Q, hi = __umul64hi(sig, Q);
    const u64 r = k >= 128 ? 0ull : k >= 64 ? (hi >> (k - 64)) : ((lo >> k) | (hi << (64 - k)));
    return r < Q ? r : Q - 1;
}
__device__ __forceinline__ void sm_draws(const SmArgs& s, i64 i, i64 m, double& u, double& u_acc)
{
    if (s.u && s.u_acc) {
        u = smc_ldg(s.u + i * s.M + m);
        u_acc = smc_ldg(s.u_acc + i * s.M + m);
        return;
    }
    u64 a, b;
    smc_philox((u32)(i * s.M + m), s.t, s.island, SMC_STREAM_BACKWARD, s.seed, a, b);
    u = s.u ? smc_ldg(s.u + i * s.M + m) : smc_u01_halfopen(a);
    u_acc = s.u_acc ? smc_ldg(s.u_acc + i * s.M + m) : smc_u01_open(b);
}
// W_t[n] as SMC_FIELD_W hands it out (k_f_write_W)
__device__ __forceinline__ double sm_W(double l, double m, double rs, int kform)
{
    if (!kform) return f_weight(l, m, rs);
    double k;
    double p = smc_expk(l, k);
    const bool ok = l > -INFINITY;
    p = ok ? p : 0.0;
    k = ok ? k : -INFINITY;
    return smc_scale_pk(p, k, m) * rs;
}
template <int KIND>
__host__ __device__ __forceinline__ int sm_scale_slot()
{
    return (KIND == SMC_MODEL_STOCHVOL || KIND == SMC_MODEL_SVLEVERAGE || KIND == SMC_MODEL_DISCRETECOX) ? 2 : 1;
}
// log p_{t+1}(xn | xp) = PX(t + 1, xp).logpdf(xn)   (state_space_models.py:341)
template <int KIND>
struct SmTrans {
    const double* p;
    double sc, rsc, lsc, aux;
    __device__ __forceinline__ SmTrans(const SmArgs& s) : p(s.p)
    {
        sc = m_trans_scale<KIND>(p);
        rsc = p[16 + sm_scale_slot<KIND>()];
        lsc = log(sc);
        aux = (KIND == SMC_MODEL_GORDON && s.aux) ? smc_ldg(s.aux) : 0.0;
    }
    __device__ __forceinline__ double loc(double xp) const { return m_trans_loc<KIND>(p, xp, aux); }
    // ... with the location of the source already formed (k_smq_thread stages it once per tile)
    __device__ __forceinline__ double logpt_at(double loc_p, double xn) const
    {
        return m_norm_logpdf(xn, loc_p, sc, rsc, lsc);
    }
    __device__ __forceinline__ double logpt(double xp, double xn) const { return logpt_at(loc(xp), xn); }
};
// the particle a drawn position stands for
__device__ __forceinline__ i64 sm_particle(const SmArgs& s, i64 pos) { return s.h ? smc_ldg(s.h + pos) : pos; }

// ---------------------------------------------------------------------------
// integer CDF of W_t: chunk totals, then every chunk scans itself behind the totals before it
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SMC_BLOCK)
k_sm_cdf_totals(const double* lw, const double* row, i64 N, int kform, int shift, u64* tot)
{
    __shared__ u64 smu[SMC_SM];
    const double m = smc_ldg(row + 5), rs = smc_ldg(row + 6);
    const i64 base = (i64)blockIdx.x * SM_CHUNK;
    u64 acc = 0;
    for (int k = 0; k < SM_CHUNK / SMC_BLOCK; ++k) {
        const i64 n = base + (i64)k * SMC_BLOCK + threadIdx.x;
        if (n < N) acc += sm_q(sm_W(smc_ldg(lw + n), m, rs, kform), shift);
    }
    acc = smc_block_sum_u64(acc, smu);
    if (threadIdx.x == 0) tot[blockIdx.x] = acc;
}
__global__ void __launch_bounds__(SMC_BLOCK)
k_sm_cdf_scan(const double* lw, const double* row, i64 N, int kform, int shift, const u64* tot, u64* cdf)
{
    __shared__ u64 smu[SMC_SM];
    const double m = smc_ldg(row + 5), rs = smc_ldg(row + 6);
    u64 before = 0;
    for (int b = (int)threadIdx.x; b < (int)blockIdx.x; b += SMC_BLOCK) before += tot[b];
    u64 run = smc_block_sum_u64(before, smu);
    const i64 base = (i64)blockIdx.x * SM_CHUNK;
    for (int k = 0; k < SM_CHUNK / SMC_BLOCK; ++k) {
        const i64 n = base + (i64)k * SMC_BLOCK + threadIdx.x;
        const u64 q = (n < N) ? sm_q(sm_W(smc_ldg(lw + n), m, rs, kform), shift) : 0ull;
        u64 total;
        const u64 ex = smc_block_exscan_u64(q, smu, total);
        if (n < N) cdf[n] = run + ex + q;
        run += total;
    }
}
// the first n with cdf[n] > floor(u Q), Q = cdf[N - 1]
__device__ __forceinline__ i64 sm_search(const u64* cdf, i64 N, double u)
{
    const u64 Q = smc_ldg(cdf + (N - 1));
    if (Q == 0) return N - 1;
    const u64 thr = sm_threshold(u, Q);
    i64 lo = 0, len = N;
    while (len > 0) {
        const i64 half = len >> 1;
        const bool le = smc_ldg(cdf + lo + half) <= thr;
        lo = le ? lo + half + 1 : lo;
        len = le ? len - half - 1 : half;
    }
    return lo < N ? lo : N - 1;
}

// last row: idx[t, m] drawn from W_t, M iid draws (smoothing.py:278-281; the reference's come sorted)
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_draw_last(const SmArgs s)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (m >= s.M) return;
    double u;
    if (s.u) {
        u = smc_ldg(s.u + m);
    } else {
        u64 a, b;
        smc_philox((u32)m, s.t, s.island, SMC_STREAM_BACKWARD, s.seed, a, b);
        u = smc_u01_halfopen(a);
    }
    s.idx_out[m] = sm_search(s.cdf, s.N, u);
}

// ---------------------------------------------------------------------------
// exact backward step (smoothing.py:305-310): one workgroup per trajectory, three sweeps over the N
// particles of step t -- the maximum of l, the integer total Q, the search -- the weights formed again in
// each (cheaper than N words per trajectory through memory).  Wave w owns the contiguous quarter
// [w R, (w + 1) R) of the particles, R a multiple of 64: its lanes read consecutive particles, and the
// third sweep is walked by the one wave whose quarter holds the threshold, until it is found.
// sm_on2_draw is the body of both k_sm_on2 (m = blockIdx.x) and k_sm_reject_exact (m from list B).  A wave
// returns from it after the last barrier, which is safe only because a workgroup draws for ONE trajectory:
// do not call it in a loop.
// ---------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ void sm_on2_draw(const SmArgs& s, const i64 m, double* smd, u64* smu)
{
    const i64 N = s.N;
    const SmTrans<KIND> tr(s);
    const double xn = smc_ldg(s.Xn + smc_ldg(s.idx_next + m));
    double mx = -INFINITY;
    for (i64 n = threadIdx.x; n < N; n += SMC_BLOCK) {
        const double l = smc_ldg(s.lwt + n) + tr.logpt(smc_ldg(s.Xt + n), xn);
        mx = (l > mx) ? l : mx;                                  // (NaN never wins)
    }
    mx = smc_block_max(mx, smd);
    if (!(mx > -INFINITY)) {
        if (threadIdx.x == 0) s.idx_out[m] = sm_particle(s, N - 1);
        return;
    }
    const i64 R = ((N + SMC_BLOCK - 1) / SMC_BLOCK) * 64;
    const i64 first = (i64)smc_wave() * R, last = (first + R < N) ? first + R : N;
    u64 acc = 0;
    for (i64 c = first; c < last; c += 64) {
        const i64 n = c + smc_lane();
        if (n < last) {
            const double l = smc_ldg(s.lwt + n) + tr.logpt(smc_ldg(s.Xt + n), xn);
            acc += sm_q((l > -INFINITY) ? smc_exp_nonpos(l - mx) : 0.0, s.shift);
        }
    }
    acc = smc_wave_sum_u64(acc);
    __syncthreads();
    if (smc_lane() == 0) smu[smc_wave()] = acc;
    __syncthreads();
    u64 Q = 0, run = 0;
    for (int w = 0; w < SMC_NWAVE; ++w) {
        if (w < smc_wave()) run += smu[w];
        Q += smu[w];
    }
    double u;
    if (s.u) {
        u = smc_ldg(s.u + m);
    } else {
        u64 a, b;
        smc_philox((u32)m, s.t, s.island, SMC_STREAM_BACKWARD, s.seed, a, b);
        u = smc_u01_halfopen(a);
    }
    const u64 thr = sm_threshold(u, Q);                          // (Q >= 2^shift: the maximum itself)
    if (thr < run || thr >= run + acc) return;                   // wave-uniform: another quarter's
    for (i64 c = first; c < last; c += 64) {
        const i64 n = c + smc_lane();
        u64 q = 0;
        if (n < last) {
            const double l = smc_ldg(s.lwt + n) + tr.logpt(smc_ldg(s.Xt + n), xn);
            q = sm_q((l > -INFINITY) ? smc_exp_nonpos(l - mx) : 0.0, s.shift);
        }
        const u64 inc = smc_wave_scan_add_u64(q);
        const u64 cum = run + inc;
        if (cum > thr && cum - q <= thr) s.idx_out[m] = sm_particle(s, n);   // exactly one lane of the launch's workgroup
        run += smc_readlane64(inc, 63);
        if (run > thr) break;
    }
}
template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_on2(const SmArgs s)
{
    __shared__ double smd[SMC_SM];
    __shared__ u64 smu[SMC_SM];
    sm_on2_draw<KIND>(s, (i64)blockIdx.x, smd, smu);
}

// ---------------------------------------------------------------------------
// MCMC backward step (smoothing.py:340-349): one thread per trajectory; start from the ancestor of the
// particle drawn for step t + 1, then nsteps independent Metropolis steps with proposals iid from W_t
// ---------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_mcmc(const SmArgs s)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (m >= s.M) return;
    const SmTrans<KIND> tr(s);
    const i64 nx = smc_ldg(s.idx_next + m);
    const double xn = smc_ldg(s.Xn + nx);
    // a step that did not resample has A = arange (core.py:336); its A slot is not meaningful
    i64 cur = (smc_ldg(s.rown + 4) != 0.0) ? (i64)smc_ldg(s.An + nx) : nx;
    double lp_cur = tr.logpt(smc_ldg(s.Xt + cur), xn);
    for (i64 i = 0; i < s.nsteps; ++i) {
        double u, ua;
        sm_draws(s, i, m, u, ua);
        const i64 prop = sm_search(s.cdf, s.N, u);
        const double lp_prop = tr.logpt(smc_ldg(s.Xt + prop), xn);
        if (log(ua) < lp_prop - lp_cur) {
            cur = prop;
            lp_cur = lp_prop;
        }
    }
    s.idx_out[m] = cur;
}

// ---------------------------------------------------------------------------
// hybrid rejection step (smoothing.py:352-423, backward_sampling_reject; Dau & Chopin 2022).  Trial i of
// trajectory m proposes prop_i = sm_search(cdf(W_t), u_prop[i]) and accepts iff
//   log(u_acc[i]) < log p_{t+1}(xn | X_t[prop_i]) - log C_{t+1};
// idx[t, m] = prop_i of the smallest accepted i < max_trials, else the exact draw of sm_on2_draw with ITS uniform.
// Three launches, ordered by the stream alone (no kernel waits for another workgroup):
//   k_sm_reject_solo   one thread per trajectory runs trials 0 .. solo - 1; the unresolved go to list A
//   k_sm_reject_wave   one wave per entry of A: 64 trials a round, the lowest accepted lane wins -- the index a
//                      sequential loop finds; a trajectory out of trials goes to list B
//   k_sm_reject_exact  one workgroup per entry of B
// The order of a list is arbitrary; nothing reads it but the next launch.  ctr: the step's four u64 slots.
// Uniforms of trial i: tapes (max_trials, M), or Philox counter (m, t, island, SMC_STREAM_REJECT | i << 8):
// word x01 -> [0, 1) proposal, word x23 -> (0, 1) acceptance.
// ---------------------------------------------------------------------------
#define SM_REJ_SOLO 4                    /* trials of the one-thread-per-trajectory launch */
#define SM_REJ_MAX_TRIALS 0xffffff       /* the trial index shares the stream word with SMC_STREAM_REJECT */
enum { SM_CTR_A = 0, SM_CTR_B = 1, SM_CTR_NPROPS = 2, SM_CTR_NEXACT = 3, SM_CTR_STRIDE = 4 };

struct SmRej {
    const double *u_prop, *u_acc;   // replay tapes of this step (max_trials, M) or null: Philox
    const double* logC;             // log C_{t+1}, one word
    u64* ctr;                       // SM_CTR_* of this step
    u32 *listA, *listB;             // (M) each
    i64 max_trials, solo;           // solo = min(max_trials, trials of the first launch)
};

template <int KIND>
__device__ __forceinline__ bool sm_rej_trial(const SmArgs& s, const SmRej& r, const SmTrans<KIND>& tr, i64 m, i64 i,
                                             double xn, double logC, i64& prop)
{
    double u, ua;
    if (r.u_prop && r.u_acc) {
        u = smc_ldg(r.u_prop + i * s.M + m);
        ua = smc_ldg(r.u_acc + i * s.M + m);
    } else {
        u64 a, b;
        smc_philox((u32)m, s.t, s.island, SMC_STREAM_REJECT | ((u32)i << 8), s.seed, a, b);
        u = r.u_prop ? smc_ldg(r.u_prop + i * s.M + m) : smc_u01_halfopen(a);
        ua = r.u_acc ? smc_ldg(r.u_acc + i * s.M + m) : smc_u01_open(b);
    }
    prop = sm_search(s.cdf, s.N, u);
    const double lp = tr.logpt(smc_ldg(s.Xt + prop), xn);
    return log(ua) < lp - logC;                                  // (a NaN or +inf bound accepts nothing)
}
// lanes below `lane` of a ballot
__device__ __forceinline__ int sm_rank(u64 mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_reject_solo(const SmArgs s, const SmRej r)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    const bool live = m < s.M;                                   // (every lane stays for the wave's ballot and sum)
    const SmTrans<KIND> tr(s);
    const double logC = smc_ldg(r.logC);
    const double xn = live ? smc_ldg(s.Xn + smc_ldg(s.idx_next + m)) : 0.0;
    bool open = live;
    u64 ntrials = 0;
    for (i64 i = 0; i < r.solo; ++i) {
        if (open) {
            i64 prop;
            ++ntrials;
            if (sm_rej_trial<KIND>(s, r, tr, m, i, xn, logC, prop)) {
                s.idx_out[m] = prop;
                open = false;
            }
        }
    }
    const u64 mask = __ballot(open ? 1 : 0);
    const u64 sum = smc_wave_sum_u64(ntrials);
    u64 at = 0;
    if (smc_lane() == 0) {
        if (sum) (void)atomicAdd(r.ctr + SM_CTR_NPROPS, sum);
        if (mask) at = atomicAdd(r.ctr + SM_CTR_A, (u64)__popcll(mask));
    }
    at = smc_readlane64(at, 0);
    if (open) r.listA[at + sm_rank(mask, smc_lane())] = (u32)m;  // (at + popcount <= M: one slot per trajectory)
}

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_reject_wave(const SmArgs s, const SmRej r)
{
    const u64 e = (u64)blockIdx.x * SMC_NWAVE + smc_wave();
    if (e >= r.ctr[SM_CTR_A]) return;                            // wave-uniform; the kernel has no barrier
    const i64 m = (i64)r.listA[e];
    const SmTrans<KIND> tr(s);
    const double logC = smc_ldg(r.logC);
    const double xn = smc_ldg(s.Xn + smc_ldg(s.idx_next + m));
    u64 ntrials = 0;
    bool found = false;
    for (i64 base = r.solo; base < r.max_trials; base += 64) {
        const i64 i = base + smc_lane();
        i64 prop = 0;
        const bool acc = (i < r.max_trials) ? sm_rej_trial<KIND>(s, r, tr, m, i, xn, logC, prop) : false;
        const u64 mask = __ballot(acc ? 1 : 0);
        if (mask) {
            const int win = __popcll(~mask & (mask - 1ull));     // the lowest accepted lane
            if (smc_lane() == win) s.idx_out[m] = prop;
            ntrials += (u64)win + 1;                             // (the speculative lanes behind it do not count)
            found = true;
            break;
        }
        ntrials += (u64)((r.max_trials - base < 64) ? r.max_trials - base : 64);
    }
    if (smc_lane() != 0) return;
    if (ntrials) (void)atomicAdd(r.ctr + SM_CTR_NPROPS, ntrials);
    if (!found) {
        r.listB[atomicAdd(r.ctr + SM_CTR_B, 1ull)] = (u32)m;     // (at most one slot per entry of A)
        (void)atomicAdd(r.ctr + SM_CTR_NEXACT, 1ull);
    }
}

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_reject_exact(const SmArgs s, const SmRej r)
{
    __shared__ double smd[SMC_SM];
    __shared__ u64 smu[SMC_SM];
    if ((u64)blockIdx.x >= r.ctr[SM_CTR_B]) return;              // the whole workgroup, before its first barrier
    sm_on2_draw<KIND>(s, (i64)r.listB[blockIdx.x], smd, smu);
}

// paths[t, m] = X_t[idx[t, m]]   (smoothing.py:288)
__global__ void __launch_bounds__(SMC_BLOCK)
k_sm_paths(const FArgs av, int isl, i64 t_end, i64 M, const i64* idx, double* out)
{
    const FArgs& a = av;
    const i64 j = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (j >= t_end * M) return;
    const double* X = f_X(a, j / M) + (i64)isl * a.N;
    out[j] = smc_ldg(X + idx[j]);
}

// ---------------------------------------------------------------------------
// host side helpers of smc_filter_backward_sample
// ---------------------------------------------------------------------------
// Blocks handed back to the pool on every way out.  The status is sticky: after the first failure get and upload do
// nothing and hand back null, so a caller acquires in plain statements and looks at status() once.
struct SmPool {
    smc_ctx* ctx;
    std::vector<void*> blocks;
    int rc = SMC_OK;
    explicit SmPool(smc_ctx* c) : ctx(c) {}
    ~SmPool() { for (void* b : blocks) (void)smc_free(ctx, b); }
    int status() const { return rc; }                // the first failure's code
    template <class T> void get(size_t n, T** out)     // (n == 0: one element)
    {
        void* p = nullptr;
        if (rc == SMC_OK && (rc = smc_malloc(ctx, (n ? n : 1) * sizeof(T), &p)) == SMC_OK) blocks.push_back(p);
        *out = (T*)p;
    }
    template <class T> void upload(const T* host, size_t n, T** out)    // (null host: nothing uploaded, *out = null, no error)
    {
        *out = nullptr;
        if (host) get(n, out);
        if (*out) rc = copy_in(host, n, out);
    }
    template <class T> int copy_in(const T* host, size_t n, T** out)
    {
        SMC_HIP_CHECK(hipMemcpyAsync(*out, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return SMC_OK;
    }
};
// Trials of the first launch.  SMC_REJECT_SOLO_TRIALS (measurements only, tools/ffbs_perf.py): a value >= max_trials
// leaves the wave launch nothing but to pass the unresolved on.  The drawn indices do not depend on it.
static i64 sm_reject_solo_trials()
{
    const char* e = getenv("SMC_REJECT_SOLO_TRIALS");
    const long long v = e ? atoll(e) : 0;
    return v >= 1 ? (i64)v : (i64)SM_REJ_SOLO;
}
template <int KIND>
static void sm_launch_reject(hipStream_t st, const SmArgs& s, const SmRej& r)
{
    const unsigned M = (unsigned)s.M;                            // (the grids are sized by M: the lists' counts stay on the device)
    SMC_LAUNCH((k_sm_reject_solo<KIND>), dim3((M + SMC_BLOCK - 1) / SMC_BLOCK), dim3(SMC_BLOCK), st, s, r);
    SMC_LAUNCH((k_sm_reject_wave<KIND>), dim3((M + SMC_NWAVE - 1) / SMC_NWAVE), dim3(SMC_BLOCK), st, s, r);
    SMC_LAUNCH((k_sm_reject_exact<KIND>), dim3(M), dim3(SMC_BLOCK), st, s, r);
}
