// smc_smooth.h -- backward sampling over the resident particle history (keep_history = 1):
// particles/smoothing.py:278-350, ParticleHistory.backward_sampling_ON2 (exact FFBS) and
// backward_sampling_mcmc (independent Metropolis steps, Dau & Chopin 2022).  Host side:
// smc_filter_backward_sample in smc_filter.hip.  The kernels read the history and write their
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
// i = Metropolis step, 0 for ON2 and for the last row.
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
__device__ __forceinline__ int sm_scale_slot()
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
    __device__ __forceinline__ double logpt(double xp, double xn) const
    {
        return m_norm_logpdf(xn, m_trans_loc<KIND>(p, xp, aux), sc, rsc, lsc);
    }
};

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
// ---------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_sm_on2(const SmArgs s)
{
    __shared__ double smd[SMC_SM];
    __shared__ u64 smu[SMC_SM];
    const i64 m = (i64)blockIdx.x, N = s.N;
    const SmTrans<KIND> tr(s);
    const double xn = smc_ldg(s.Xn + smc_ldg(s.idx_next + m));
    double mx = -INFINITY;
    for (i64 n = threadIdx.x; n < N; n += SMC_BLOCK) {
        const double l = smc_ldg(s.lwt + n) + tr.logpt(smc_ldg(s.Xt + n), xn);
        mx = (l > mx) ? l : mx;                                  // (NaN never wins)
    }
    mx = smc_block_max(mx, smd);
    if (!(mx > -INFINITY)) {
        if (threadIdx.x == 0) s.idx_out[m] = N - 1;
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
        if (cum > thr && cum - q <= thr) s.idx_out[m] = n;       // exactly one lane of the launch's workgroup
        run += smc_readlane64(inc, 63);
        if (run > thr) break;
    }
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
struct SmPool {                    // blocks handed back to the pool on every way out
    smc_ctx* ctx;
    std::vector<void*> blocks;
    explicit SmPool(smc_ctx* c) : ctx(c) {}
    ~SmPool() { for (void* b : blocks) (void)smc_free(ctx, b); }
    template <class T> int get(size_t n, T** out)
    {
        void* p = nullptr;
        const int rc = smc_malloc(ctx, (n ? n : 1) * sizeof(T), &p);
        if (rc == SMC_OK) blocks.push_back(p);
        *out = (T*)p;
        return rc;
    }
    template <class T> int upload(const T* host, size_t n, T** out)
    {
        *out = nullptr;
        if (!host) return SMC_OK;
        const int rc = get(n, out);
        if (rc != SMC_OK) return rc;
        SMC_HIP_CHECK(hipMemcpyAsync(*out, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return SMC_OK;
    }
};
template <int KIND>
static void sm_launch_step(int method, hipStream_t st, const SmArgs& s)
{
    if (method == SMC_BACKWARD_ON2)
        SMC_LAUNCH((k_sm_on2<KIND>), dim3((unsigned)s.M), dim3(SMC_BLOCK), st, s);
    else
        SMC_LAUNCH((k_sm_mcmc<KIND>), dim3((unsigned)((s.M + SMC_BLOCK - 1) / SMC_BLOCK)), dim3(SMC_BLOCK), st, s);
}
