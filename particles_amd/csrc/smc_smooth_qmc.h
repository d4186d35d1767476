// smc_smooth_qmc.h -- backward sampling for SQMC filters over the resident particle history (keep_history = 1):
// particles/smoothing.py:425-456, ParticleHistory.backward_sampling_qmc.  Exact FFBS (smc_smooth.h) with two differences:
// the M x T uniforms are ONE point set (row m = the point of trajectory m, the caller's), and every inverse-CDF lookup is
// made in the HILBERT ORDER of the particles of its step -- for univariate particles argsort(X_t), ties by index, -0.0
// before +0.0, NaN last (smc_argsort).  Host side: smc_filter_backward_qmc in smc_filter.hip.
//
// Per backward step b the host sorts X_b (smc_rs_sort_ws; its payloads ARE h_b: position j holds particle h_b[j]) and
// k_smq_gather writes ONE step's slab in sorted order, xs[j] = X_b[h[j]] and ls[j] = lw_b[h[j]]; the slab of step b + 1
// is overwritten (stream order), so a call holds 2 N words of slab whatever T is.  A draw finds a POSITION in the slab and
// stores the PARTICLE h[position]: idx stays in particle numbering, x_{b+1}^m = X_{b+1}[idx[b + 1, m]] is read from the
// unsorted history.
//
// The contract is smc_smooth.h's: l_j = ls[j] + SmTrans::logpt(xs[j], x_{b+1}^m), e_j = smc_exp_nonpos(l_j - max l),
// q_j = sm_q(e_j, sm_shift(N)), Q = sum q_j, position = the first j whose inclusive prefix exceeds sm_threshold(u, Q).
// The maximum and the 64-bit sums are exact in any order, so the two launch geometries return IDENTICAL indices:
//   geometry 1  k_smq_wg      one workgroup per trajectory: sm_on2_draw itself on the slab (SmArgs::h maps the store)
//   geometry 2  k_smq_thread  one thread per trajectory, workgroups of SMC_BLOCK trajectories.  The slab passes through
//               LDS in tiles of SMQ_TILE sources, staged as (loc_j, ls[j]) with loc_j = SmTrans::loc(xs[j]) formed once per
//               tile and workgroup; every thread reads the same address (a broadcast, no bank conflict).  Three sweeps over
//               the slab per thread: the running maximum of l, then Q, then the prefix until it exceeds the threshold.
//               A wave whose 64 lanes have all found their position does no more pair work in the third sweep; it still
//               stages and meets every barrier, as a thread past M does from the start.
// Edge rules as in smc_smooth.h: q = 0 is never drawn, u >= 1 selects the last positive weight, no finite l at all gives
// position N - 1; a NaN state or log-weight gives a NaN l, which weighs 0 and never wins the maximum.
// LDS of k_smq_thread: SMQ_TILE x 2 doubles = 16 KiB (ten workgroups' worth in a CU's 160 KiB; the eight workgroups a CU's
// wave slots hold take 128 KiB).
#pragma once
#include "smc_smooth.h"

#define SMQ_TILE (4 * SMC_BLOCK)       /* sources per LDS tile: four staged by each thread */
// geometry 0 takes k_smq_thread from this M on.  Above every M the entry accepts: at N = 2^14 k_smq_thread lost at every
// measured M (256 .. 2^14: x64 .. x10 of k_smq_wg; DESIGN section 6, profiles/ffbs_qmc_perf.txt).  M / 256 workgroups of
// one wave per SIMD run a thread's serial chain of 3 N pair evaluations with nothing to hide its latency behind, and its
// time does not move with M until they fill the machine; geometry = 2 still selects it.
#define SMQ_THREAD_MIN_M ((i64)1 << 31)

// the slab of one step in sorted order
__global__ void __launch_bounds__(SMC_BLOCK)
k_smq_gather(const i64* h, const double* X, const double* lw, i64 N, double* xs, double* ls)
{
    const i64 j = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (j >= N) return;
    i64 n = smc_ldg(h + j);
    n = (n >= 0 && n < N) ? n : j;                               // (a permutation: always in range)
    xs[j] = smc_ldg(X + n);
    ls[j] = smc_ldg(lw + n);
}
// ut[b, m] = u[m, b]: the caller's points (M, t) as the per-step rows the draws read
__global__ void __launch_bounds__(SMC_BLOCK) k_smq_transpose(const double* u, i64 M, i64 t, double* ut)
{
    const i64 j = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (j >= M * t) return;
    const i64 b = j / M, m = j - b * M;
    ut[j] = smc_ldg(u + m * t + b);
}
// last row: the position of u[m] in the integer CDF of W_{t-1} in sorted order (s.cdf, on the gathered ls), as a particle
__global__ void __launch_bounds__(SMC_BLOCK) k_smq_draw_last(const SmArgs s)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (m >= s.M) return;
    s.idx_out[m] = sm_particle(s, sm_search(s.cdf, s.N, smc_ldg(s.u + m)));
}

// geometry 1: s.Xt, s.lwt = the slab, s.h = its order
template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_smq_wg(const SmArgs s)
{
    __shared__ double smd[SMC_SM];
    __shared__ u64 smu[SMC_SM];
    sm_on2_draw<KIND>(s, (i64)blockIdx.x, smd, smu);
}

// geometry 2
template <int KIND>
struct SmqTile {
    double (&loc)[SMQ_TILE];
    double (&lw)[SMQ_TILE];
    // sources [base, base + cnt) of the slab into LDS; the barriers are every thread's
    __device__ __forceinline__ int stage(const SmArgs& s, const SmTrans<KIND>& tr, i64 base) const
    {
        const int cnt = (int)((s.N - base < SMQ_TILE) ? s.N - base : SMQ_TILE);
        __syncthreads();                                         // the tile before is read out
        for (int j = (int)threadIdx.x; j < cnt; j += SMC_BLOCK) {
            loc[j] = tr.loc(smc_ldg(s.Xt + base + j));
            lw[j] = smc_ldg(s.lwt + base + j);
        }
        __syncthreads();
        return cnt;
    }
    __device__ __forceinline__ double l(const SmTrans<KIND>& tr, int j, double xn) const
    {
        return lw[j] + tr.logpt_at(loc[j], xn);
    }
    __device__ __forceinline__ u64 q(const SmArgs& s, const SmTrans<KIND>& tr, int j, double xn, double mx) const
    {
        const double lj = l(tr, j, xn);
        return sm_q((lj > -INFINITY) ? smc_exp_nonpos(lj - mx) : 0.0, s.shift);
    }
};

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_smq_thread(const SmArgs s)
{
    __shared__ double s_loc[SMQ_TILE], s_lw[SMQ_TILE];
    const SmqTile<KIND> tile{s_loc, s_lw};
    const i64 N = s.N;
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    const bool live = m < s.M;                                   // (a thread past M stages and idles: every barrier is its too)
    const SmTrans<KIND> tr(s);
    const double xn = live ? smc_ldg(s.Xn + smc_ldg(s.idx_next + m)) : 0.0;
    double mx = -INFINITY;
    for (i64 base = 0; base < N; base += SMQ_TILE) {
        const int cnt = tile.stage(s, tr, base);
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const double l = tile.l(tr, j, xn);
                mx = (l > mx) ? l : mx;                          // (NaN never wins)
            }
    }
    const bool draws = live && mx > -INFINITY;
    u64 Q = 0;
    for (i64 base = 0; base < N; base += SMQ_TILE) {
        const int cnt = tile.stage(s, tr, base);
        if (draws)
            for (int j = 0; j < cnt; ++j) Q += tile.q(s, tr, j, xn, mx);
    }
    const u64 thr = draws ? sm_threshold(smc_ldg(s.u + m), Q) : 0ull;     // (Q >= 2^shift: the maximum itself)
    i64 pos = N - 1;                                             // no finite l at all
    bool open = draws;
    u64 run = 0;
    for (i64 base = 0; base < N; base += SMQ_TILE) {
        const int cnt = tile.stage(s, tr, base);
        if (__ballot(open ? 1 : 0) == 0ull) continue;            // wave-uniform: all 64 positions are found
        if (open)
            for (int j = 0; j < cnt; ++j) {
                run += tile.q(s, tr, j, xn, mx);
                if (run > thr) {
                    pos = base + j;
                    open = false;
                    break;
                }
            }
    }
    if (live) s.idx_out[m] = sm_particle(s, pos);
}
