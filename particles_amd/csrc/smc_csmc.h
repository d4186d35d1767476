// smc_csmc.h -- conditional SMC (particles/mcmc.py:453-475, CSMC: the state update of Particle Gibbs; Andrieu, Doucet &
// Holenstein 2010) for many chains at once.  Host side: smc_filter_set_conditional, smc_filter_csmc_paths and the
// branch of smc_filter_step in smc_filter.hip.
//
//   k_csmc_small  the conditional twin of k_filter_small (smc_filter_small.h): one persistent workgroup per island, the
//                 whole time loop in one launch, particle 0 pinned to the retained trajectory xstar (n_islands, T).  The
//                 loop is restated here, not templated into the old one: k_filter_small keeps its bits by construction.
//                 State, summary rows and the step record are written exactly as k_filter_small writes them, so every
//                 accessor, backward sampling, cloning and checkpointing work on a conditional filter unchanged.
//   k_csmc_path   one new trajectory per island in one launch: the last index from W_{t-1}, then either the genealogy
//                 (extract_one_trajectory, smoothing.py:256-269) or one exact backward draw per step
//                 (backward_sampling_ON2(1), smoothing.py:291-311).
//
// Contract of k_csmc_small, island i, step t (bootstrap filters of the five kinds backward sampling takes, N <= 1024,
// multinomial):
//   decision   k_filter_small's: ESS of step t - 1 against ess_thresh, never at t = 0
//   ancestors  (resampling step) A[0] = 0; A[n], n >= 1, is the inverse of ONE uniform u_n in the integer CDF of W_{t-1}
//              under the contract of smc_smooth.h: e_n = W_{t-1}[n] as SMC_FIELD_W forms it, q_n = sm_q(e_n, sm_shift(N)),
//              thr = sm_threshold(u_n, Q), the first inclusive prefix exceeding thr; Q = 0 gives N - 1.  The prefix is a
//              block scan kept in LDS (8 KiB), the search a binary search in LDS.
//              u_n: the replay tape a.ut[t, i, n] (the tape smc_filter_set_replay documents for multinomial -- the SORTED
//              uniforms; slot 0 is ignored), else Philox stream SMC_STREAM_CSMC, counter (n, t, island, 6), word
//              x01 -> [0, 1).  The N - 1 free ancestors are therefore iid draws from W in draw order; the reference draws
//              N sorted indices and overwrites the first.
//              (no resampling) parents are the particles themselves; A is left as k_filter_small leaves it
//   weights    restart from 0 behind a resampling
//   move       every particle moves with m_step<KIND, SMC_FK_BOOTSTRAP> on the normals of stream 0 with k_filter_small's
//              counters (or the zt tape): at t = 0 particles 1 .. N-1 are those of the unconditional filter of the same
//              seed.  Then x_0 = xstar[i, t] and its increment is formed again, m_obs_logpdf<KIND>(p, y_t, x_0, xp_0,
//              first, aux), NaN -> -inf, xp_0 = X_{t-1}[A[0]].
#pragma once
#include "smc_smooth.h"

// the first n < N whose inclusive prefix c[n] exceeds thr (c in LDS, non-decreasing, c[N - 1] = Q > thr)
__device__ __forceinline__ i64 cs_search_lds(const u64* c, i64 N, u64 thr)
{
    i64 lo = 0, len = N;
    while (len > 0) {
        const i64 half = len >> 1;
        const bool le = c[lo + half] <= thr;
        lo = le ? lo + half + 1 : lo;
        len = le ? len - half - 1 : half;
    }
    return lo < N ? lo : N - 1;
}

template <int KIND, int BS>
__global__ void __launch_bounds__(BS)
k_csmc_small(const FArgs av, const int nsteps, const double* xstar)
{
    constexpr int FK = SMC_FK_BOOTSTRAP;
    const FArgs& a = av;
    __shared__ u64 sC[BS * F_IPT];          // inclusive integer CDF of W_{t-1}
    __shared__ double sX[BS * F_IPT];       // the parents' states
    __shared__ u64 smu[SMC_SM];
    __shared__ double smd[SMC_SM];          // sums
    __shared__ double smm[SMC_SM];          // maxima
    SMC_NTAB_LDS(s_ntab);
    const int isl = (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    // (fewer than SMC_NWAVE waves: the unused slots of the collectives keep the neutral element, as in k_filter_small)
    if (tid < SMC_SM) { smu[tid] = 0ull; smd[tid] = 0.0; smm[tid] = -INFINITY; }
    smc_ntab_stage<BS>(s_ntab, tid);
    __shared__ double s_par[PARAM_STRIDE];
    static_assert(BS >= PARAM_STRIDE, "one constant per thread");
    if (tid < PARAM_STRIDE) s_par[tid] = smc_ldg(a.params + (i64)isl * PARAM_STRIDE + tid);
    __syncthreads();
    const i64 N = a.N;
    double* info = a.info + (i64)isl * INFO_STRIDE;
    const u32 gisl = (u32)(a.island_offset + isl);
    const double* p = s_par;
    const double* xs = xstar + (i64)isl * a.T;
    const i64 jt = (i64)tid * F_IPT;                       // this thread's particles jt..jt+3
    const bool vec = (N & 3) == 0;
    const int shift = sm_shift(N);

    i64 t = (i64)smc_uniform(smc_ldg(info));
    if (t >= a.T) return;
    bool resample = smc_uniform(smc_ldg(info + 1)) != 0.0;
    double m = smc_uniform(smc_ldg(info + 3)), rs = smc_uniform(smc_ldg(info + 4));
    double prev_log_mean = 0.0, prev_logLt = 0.0;          // of step t-1 (core.py:355-359)
    if (t > 0) {
        const double* prow = a.summ + ((i64)isl * (a.T + 1) + (t - 1)) * SUMM_STRIDE;
        prev_log_mean = smc_uniform(smc_ldg(prow + 1));
        prev_logLt = smc_uniform(smc_ldg(prow + 3));
    }
    double y_next = a.y[t * a.dy];
    double aux_next = (m_has_aux<KIND>() && a.aux) ? a.aux[t] : 0.0;
    double x[4], lw[4];
    if (t > 0) {                                           // continue a run
        f_load4<double>(f_X(a, t - 1) + (i64)isl * N, jt, N, vec, 0.0, x);
        f_load4<double>(f_lw(a, t - 1) + (i64)isl * N, jt, N, vec, -INFINITY, lw);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] = 0.0; lw[k] = -INFINITY; }
    }

    for (int step = 0; step < nsteps && t < a.T; ++step, ++t) {
        const bool first = (t == 0);
        const bool rsp = !first && resample;
        const double yt = y_next, aux = aux_next;
        if (t + 1 < a.T) {
            y_next = a.y[(t + 1) * a.dy];
            if (m_has_aux<KIND>() && a.aux) aux_next = a.aux[t + 1];
        }
        double xp[4], lwp[4];
        if (rsp) {
            // ---- the integer CDF of W_{t-1} (smc_smooth.h: k_sm_cdf_scan's terms), inclusive, in LDS
            u64 q4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q4[k] = (jt + k < N) ? sm_q(f_weight(lw[k], m, rs), shift) : 0ull;
            u64 Q;
            u64 c = smc_block_exscan_u64(q4[0] + q4[1] + q4[2] + q4[3], smu, Q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c += q4[k];
                sC[jt + k] = c;
                sX[jt + k] = x[k];
            }
            __syncthreads();
            // ---- one inverse-CDF draw per free particle; particle 0 keeps the retained line
            const double* ut = a.ut ? a.ut + ((i64)t * a.n_islands + isl) * a.ut_stride : nullptr;
            u32 an[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const i64 n = jt + k;
                i64 r = 0;
                if (n >= 1 && n < N) {
                    double u;
                    if (ut) {
                        u = smc_ldg(ut + n);
                    } else {
                        u64 b0, b1;
                        smc_philox((u32)n, (u32)t, gisl, SMC_STREAM_CSMC, a.seed, b0, b1);
                        u = smc_u01_halfopen(b0);
                    }
                    r = Q ? cs_search_lds(sC, N, sm_threshold(u, Q)) : N - 1;
                }
                an[k] = (u32)r;
            }
            u32* A = f_A(a, t) + (i64)isl * N;
            if (vec && jt + 3 < N) {
                smc_st4g(A + jt, an);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (jt + k < N) smc_stg(A + jt + k, an[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { xp[k] = sX[an[k]]; lwp[k] = 0.0; }          // core.py:332, reset_weights
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { xp[k] = first ? 0.0 : x[k]; lwp[k] = first ? 0.0 : lw[k]; }
        }
        // ---- standard normals (k_filter_small's counters), propagate, weigh
        double z[4];
        if (a.zt) {
            const double* zt = a.zt + ((i64)t * a.zt_ts + (i64)isl * N);
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = (jt + k < N) ? smc_ldg(zt + jt + k) : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k += 2)
                smc_normal_pair(s_ntab, a.seed, (u32)((jt + k) >> 1), (u32)t, gisl, SMC_STREAM_NORMAL, z[k], z[k + 1]);
        }
        const double x0 = smc_ldg(xs + t);                 // mcmc.py:463, :472: X[0] = xstar[t]
        bool okp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            okp[k] = jt + k < N;
            double inc;
            x[k] = m_step<KIND, FK>(p, first, yt, aux, xp[k], z[k], inc);
            if (k == 0 && tid == 0) {                      // the pinned particle: its increment is formed again
                x[k] = x0;
                inc = m_obs_logpdf<KIND>(p, yt, x0, xp[k], first, aux);
            }
            double l = first ? inc : lwp[k] + inc;                                  // resampling.py:241-244
            if (l != l) l = -INFINITY;                                              // resampling.py:220
            lw[k] = okp[k] ? l : -INFINITY;
        }
        f_store4<double>(f_X(a, t) + (i64)isl * N, jt, vec && okp[3], okp, x);
        f_store4<double>(f_lw(a, t) + (i64)isl * N, jt, vec && okp[3], okp, lw);
        // ---- log-sum-exp of the workgroup = of the filter (as in k_filter_small)
        double tm = lw[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) tm = smc_max2(tm, lw[k]);
        const double gm = smc_block_max(tm, smm);
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double e = (lw[k] > -INFINITY) ? smc_exp_nonpos(lw[k] - gm) : 0.0;
            s1 += e;
            s2 = fma(e, e, s2);
        }
        smc_block_sum2(s1, s2, smd);
        // ---- finalise step t (every thread computes the same scalars), decide step t+1
        const bool bad = !(gm > -INFINITY) || !(gm < INFINITY);
        const double ess = bad ? NAN : (s1 * s1) / s2;                              // resampling.py:226
        const double log_mean = bad ? NAN : gm + log(s1 / (double)N);               // resampling.py:224
        double* row = a.summ + ((i64)isl * (a.T + 1) + t) * SUMM_STRIDE;
        double loglt;                                                               // core.py:355-359
        if (first || rsp) loglt = log_mean;
        else loglt = log_mean - prev_log_mean;
        const double logLt = (first ? 0.0 : prev_logLt) + loglt;
        prev_log_mean = log_mean;
        prev_logLt = logLt;
        if (tid == 0) {
            row[0] = ess;
            row[1] = log_mean;
            row[2] = loglt;
            row[3] = logLt;
            row[4] = rsp ? 1.0 : 0.0;
            row[5] = gm;
            row[6] = bad ? NAN : 1.0 / s1;
        }
        m = gm;
        rs = bad ? NAN : 1.0 / s1;
        resample = (t + 1 < a.T) && (ess < a.ess_thresh);                           // core.py:181-183
    }
    if (tid == 0) {                 // the step record, as k_filter_small leaves it
        info[0] = (double)t;
        info[1] = resample ? 1.0 : 0.0;
        info[2] = (t < a.T) ? a.y[t * a.dy] : 0.0;
        info[3] = m;
        info[4] = rs;
        info[5] = (a.aux && t < a.T) ? a.aux[t] : 0.0;
    }
}

// ---------------------------------------------------------------------------
// One trajectory per island over the t_end steps run: idx[i, s], paths[i, s] = X_s[idx[i, s]], s = t_end - 1 .. 0.
//   last index  the inverse of u_last[i] in the integer CDF of W_{t_end-1} (what k_sm_draw_last computes for M = 1)
//   genealogy   n_{s-1} = A_s[n_s] where step s resampled (summary row, slot 4), else n_s: k_f_one_trajectory's rule
//   backward    per step the exact draw of sm_on2_draw for the one trajectory: the maximum of
//               l_n = lw_s[n] + logpt(s + 1, X_s[n], x_{s+1}), q_n = sm_q(exp(l_n - max), shift), their total Q, the
//               threshold and the first prefix above it -- the same terms from the same operations, and an index is a
//               function of (history, uniform) alone: the indices are those of smc_filter_backward_sample at M = 1.
// Uniforms: tapes u_last (n_islands) and u (t_end - 1, n_islands), or Philox stream SMC_STREAM_BACKWARD with the
// counters of backward sampling at M = 1: (0, s, island, 3), word x01 -> [0, 1).
// The one workgroup holds the island's N <= 4 BS particles, 4 per thread; LDS: the prefix of 4 BS integers (8 KiB).
// ---------------------------------------------------------------------------
template <int KIND, int BS>
__global__ void __launch_bounds__(BS)
k_csmc_path(const FArgs av, const i64 t_end, const int backward, const int kform, const u64 seed, const double* u_last,
            const double* u, i64* idx, double* paths)
{
    const FArgs& a = av;
    __shared__ u64 sC[BS * F_IPT];
    __shared__ u64 smu[SMC_SM];
    __shared__ double smm[SMC_SM];
    __shared__ double s_par[PARAM_STRIDE];
    __shared__ i64 s_n;
    const int isl = (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    if (tid < SMC_SM) { smu[tid] = 0ull; smm[tid] = -INFINITY; }
    static_assert(BS >= PARAM_STRIDE, "one constant per thread");
    if (tid < PARAM_STRIDE) s_par[tid] = smc_ldg(a.params + (i64)isl * PARAM_STRIDE + tid);
    __syncthreads();
    const i64 N = a.N;
    const u32 gisl = (u32)(a.island_offset + isl);
    const i64 jt = (i64)tid * F_IPT;
    const int shift = sm_shift(N);
    const double* rows = a.summ + (i64)isl * (a.T + 1) * SUMM_STRIDE;
    i64* idx_i = idx + (i64)isl * t_end;
    double* path_i = paths + (i64)isl * t_end;
    auto uniform_of = [&](const double* tape, i64 s) {
        if (tape) return smc_ldg(tape);
        u64 b0, b1;
        smc_philox(0u, (u32)s, gisl, SMC_STREAM_BACKWARD, seed, b0, b1);
        return smc_u01_halfopen(b0);
    };
    // every thread's four terms q -> the inclusive prefix in LDS; thread 0 draws, all threads return the index
    auto draw = [&](const u64 (&q4)[4], double uu) {
        u64 Q;
        u64 c = smc_block_exscan_u64(q4[0] + q4[1] + q4[2] + q4[3], smu, Q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c += q4[k];
            sC[jt + k] = c;
        }
        __syncthreads();
        if (tid == 0) s_n = Q ? cs_search_lds(sC, N, sm_threshold(uu, Q)) : N - 1;
        __syncthreads();
        return s_n;
    };

    // ---- the last index, from W_{t_end-1} as SMC_FIELD_W forms it
    i64 s = t_end - 1;
    i64 n_cur;
    {
        const double m = smc_ldg(rows + s * SUMM_STRIDE + 5), rs = smc_ldg(rows + s * SUMM_STRIDE + 6);
        const double* lws = f_lw(a, s) + (i64)isl * N;
        u64 q4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q4[k] = (jt + k < N) ? sm_q(sm_W(smc_ldg(lws + jt + k), m, rs, kform), shift) : 0ull;
        n_cur = draw(q4, uniform_of(u_last ? u_last + isl : nullptr, s));
    }
    double x_cur = smc_ldg(f_X(a, s) + (i64)isl * N + n_cur);
    if (tid == 0) { idx_i[s] = n_cur; path_i[s] = x_cur; }

    if (!backward) {                                       // one line of ancestors: no other thread is needed
        if (tid != 0) return;
        for (--s; s >= 0; --s) {
            if (smc_ldg(rows + (s + 1) * SUMM_STRIDE + 4) != 0.0) n_cur = (i64)smc_ldg(f_A(a, s + 1) + (i64)isl * N + n_cur);
            idx_i[s] = n_cur;
            path_i[s] = smc_ldg(f_X(a, s) + (i64)isl * N + n_cur);
        }
        return;
    }

    SmArgs sa{};
    sa.p = s_par;
    SmTrans<KIND> tr(sa);
    for (--s; s >= 0; --s) {
        tr.aux = (KIND == SMC_MODEL_GORDON && a.aux) ? smc_ldg(a.aux + (s + 1)) : 0.0;
        const double* Xs = f_X(a, s) + (i64)isl * N;
        const double* lws = f_lw(a, s) + (i64)isl * N;
        double l4[4], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            l4[k] = (jt + k < N) ? smc_ldg(lws + jt + k) + tr.logpt(smc_ldg(Xs + jt + k), x_cur) : -INFINITY;
            mx = (l4[k] > mx) ? l4[k] : mx;                              // (NaN never wins)
        }
        mx = smc_block_max(mx, smm);
        if (!(mx > -INFINITY)) {                                         // (uniform over the workgroup)
            n_cur = N - 1;
        } else {
            u64 q4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q4[k] = sm_q((l4[k] > -INFINITY) ? smc_exp_nonpos(l4[k] - mx) : 0.0, shift);
            n_cur = draw(q4, uniform_of(u ? u + s * a.n_islands + isl : nullptr, s));
        }
        x_cur = smc_ldg(Xs + n_cur);
        if (tid == 0) { idx_i[s] = n_cur; path_i[s] = x_cur; }
    }
}
