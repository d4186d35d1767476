// smc_online.h -- on-line smoothing of additive functions (particles/collectors.py:345-449; book 11.1, 11.3):
// the forward recursions of Online_smooth_naive, Online_smooth_ON2 and Paris, one update per time step behind the
// step the filter has just run.  Host side: smc_filter_online_smooth in smc_filter.hip.  The kernels read the
// filter's current step and write the caller's arrays and their own workspaces only.
//
//   psi_0(x)     = sum_j  c0[k][j]   x^j               t = 0:  Phi_0[n] = psi_0(X_0[n])
//   psi_t(xp, x) = sum_ij c[k][i][j] xp^i x^j          i, j in 0..2, k < K <= 8
//   naive  Phi_t[n] = Phi_{t-1}[a] + psi(X_{t-1}[a], X_t[n]),  a = A_t[n] (n when the step did not resample)
//   ON2    Phi_t[n] = sum_m e_m (Phi_{t-1}[m] + psi(X_{t-1}[m], X_t[n])) / sum_m e_m,
//          e_m = exp(l_m - max l), l_m = lw_{t-1}[m] + log p_t(X_t[n] | X_{t-1}[m])   (-inf, NaN: weight 0)
//   Paris  Phi_t[n] = mean over r < R of Phi_{t-1}[a] + psi(X_{t-1}[a], X_t[n]), a = As[n, r], drawn by the
//          k_sm_reject_* launches of smc_smooth.h with N R "trajectories" (trajectory j: target X_t[j / R])
//   est[k] = sum_n W_t[n] Phi_t[n, k], W_t as SMC_FIELD_W hands it out (sm_W)
//
// ON2 is the all-pairs kernel.  psi is a polynomial in the source xp for a fixed target x,
//   psi_k = a_0k(x) + a_1k(x) xp + a_2k(x) xp^2,   a_ik(x) = sum_j c[k][i][j] x^j,
// so a target needs four moments of its weights and K weighted sums of Phi_{t-1} -- no polynomial per pair:
//   S0 = sum e, S1 = sum e xp, S2 = sum e xp^2, P_k = sum e Phi_{t-1}[m, k]
//   Phi_t[n, k] = (P_k + a_0k S0 + a_1k S1 + a_2k S2) / S0.
// The density's constant -log(scale sqrt(2 pi)) is the same for every source and cancels: l is formed without it.
//   k_os_loc<KIND>   loc_m = m_trans_loc<KIND>(p, X_{t-1}[m], aux_t), once per source (ThetaLogistic's holds an exp)
//   k_os_on2<KP>     one target per thread, grid (target blocks, source slices).  A slice's sources pass through LDS
//                    in tiles of OS_TILE: loc, lw, xp, xp^2 and KP values of Phi, every read a broadcast.  Per tile two
//                    sweeps over LDS -- the tile's maximum of l (no exponential), one rescale of the running sums
//                    when the maximum moved, then the sums: a pair costs a subtract-square twice, one smc_exp_nonpos
//                    and KP + 3 fma.  A thread's sums are sequential: the same bits from run to run.  Writes the
//                    slice's partial (max, S0, S1, S2, P) of every target.
//   k_os_on2_merge   the slices of a target in slice order on the largest of their maxima, then Phi_t[n, :].
// LDS: OS_TILE (4 + KP) doubles = 10, 16, 24 KiB for KP = 1, 4, 8.
#pragma once
#include "smc_smooth.h"

#define OS_TILE SMC_BLOCK              /* sources per LDS tile: one staged by each thread */
#define OS_KMAX 8
#define OS_PART(KP) ((KP) + 4)         /* doubles per (slice, target) partial: max, S0, S1, S2, P[KP] */
// Source slices: enough workgroups for the 256 CUs at small N (fixed by N alone: the merge order is part of the result).
// With B = ceil(N / 256) target blocks (= source tiles) the launch has min(ceil(OS_TARGET_WGS / B), B) slices, so the
// geometry changes twice with N:
//   N <= OS_N_ONE_TILE                    every slice is ONE tile (B slices): the sums are never rescaled inside a slice
//   OS_N_ONE_TILE < N <= OS_N_SLICED      several slices of several tiles, the last one shorter or absent
//   N > OS_N_SLICED                       one slice holds every tile: the merge only finishes it
#define OS_TARGET_WGS 1024
#define OS_N_ONE_TILE 8192             /* 32 blocks x 32 one-tile slices = OS_TARGET_WGS */
#define OS_N_SLICED ((OS_TARGET_WGS - 1) * SMC_BLOCK)       /* 261 888: from 1024 target blocks on, one slice */

struct OsPsi {                         // smc_addfunc as the kernels take it
    int K;
    double c0[OS_KMAX][3];
    double c[OS_KMAX][3][3];
};

// a_ik(x), i = 0..2
__device__ __forceinline__ void os_poly_x(const OsPsi& f, int k, double x, double (&a)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = fma(fma(f.c[k][i][2], x, f.c[k][i][1]), x, f.c[k][i][0]);
}
__device__ __forceinline__ double os_psi(const OsPsi& f, int k, double xp, double x)
{
    double a[3];
    os_poly_x(f, k, x, a);
    return fma(fma(a[2], xp, a[1]), xp, a[0]);
}

// t = 0: Phi[n, k] = psi_0(X_0[n])
__global__ void __launch_bounds__(SMC_BLOCK) k_os_init(const OsPsi f, const double* X, i64 N, double* Phi)
{
    const i64 n = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (n >= N) return;
    const double x = smc_ldg(X + n);
    for (int k = 0; k < f.K; ++k) Phi[n * f.K + k] = fma(fma(f.c0[k][2], x, f.c0[k][1]), x, f.c0[k][0]);
}

// naive (R = 0: the step's ancestors, identity when row[4] == 0) and Paris (R >= 1: idx (N, R)); out != Phi
__global__ void __launch_bounds__(SMC_BLOCK)
k_os_gather(const OsPsi f, const double* X, const double* Xprev, const double* Phi, const u32* A, const double* row,
            const i64* idx, int R, i64 N, double* out)
{
    const i64 n = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (n >= N) return;
    const double x = smc_ldg(X + n);
    if (R == 0) {
        const i64 a = (smc_ldg(row + 4) != 0.0) ? (i64)smc_ldg(A + n) : n;
        const double xp = smc_ldg(Xprev + a);
        for (int k = 0; k < f.K; ++k) out[n * f.K + k] = smc_ldg(Phi + a * f.K + k) + os_psi(f, k, xp, x);
        return;
    }
    for (int k = 0; k < f.K; ++k) {
        double acc = 0.0;
        for (int r = 0; r < R; ++r) {
            const i64 a = smc_ldg(idx + n * R + r);
            acc += smc_ldg(Phi + a * f.K + k) + os_psi(f, k, smc_ldg(Xprev + a), x);
        }
        out[n * f.K + k] = acc / (double)R;
    }
}
// idx_next of the rejection launches: trajectory j belongs to target j / R
__global__ void __launch_bounds__(SMC_BLOCK) k_os_targets(i64 M, int R, i64* out)
{
    const i64 j = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (j < M) out[j] = j / R;
}

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_os_loc(const SmArgs s, double* loc)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (m >= s.N) return;
    const SmTrans<KIND> tr(s);
    loc[m] = m_trans_loc<KIND>(s.p, smc_ldg(s.Xt + m), tr.aux);
}

struct OsOn2 {
    const double *X, *Xprev, *lwprev, *loc, *Phi;   // (N) targets; (N) sources: state, log-weight, loc; (N, K)
    double* part;                                   // (nslices, N, OS_PART(KP))
    const double* p;                                // the island's params row
    int slot;                                       // ... its transition scale: p[slot], RN(1 / scale) at p[16 + slot]
    i64 N, per_slice;                               // sources per slice: a multiple of OS_TILE
    int K;
};

template <int KP>
__global__ void __launch_bounds__(SMC_BLOCK) k_os_on2(const OsOn2 o)
{
    __shared__ double s_loc[OS_TILE], s_lw[OS_TILE], s_x[OS_TILE], s_x2[OS_TILE];
    __shared__ double s_phi[KP][OS_TILE];
    const i64 N = o.N;
    const i64 n = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    const double x = (n < N) ? smc_ldg(o.X + n) : 0.0;          // (a thread past N stages and idles: every barrier is its too)
    const i64 first = (i64)blockIdx.y * o.per_slice;
    const i64 last = (first + o.per_slice < N) ? first + o.per_slice : N;
    // l is formed with the product (x - loc) RN(1 / scale), not with the correctly rounded quotient SmTrans::logpt forms
    // through smc_div_c: one multiply per pair instead of three fma and a branch.  The two differ by 1 ulp of v, a few
    // ulp of |l| in the weight -- inside the contract's tolerance, but ON2's l is not bit for bit the log-density the
    // rejection and exact-draw kernels evaluate.  RN(1 / scale) = 0 marks a reciprocal the host would not vouch for
    // (smc_div_c then divides): the quotient's reciprocal is formed here instead.
    double rsc = smc_ldg(o.p + 16 + o.slot);
    if (!(rsc > 0.0)) rsc = 1.0 / smc_ldg(o.p + o.slot);
    double mx = -INFINITY, S0 = 0.0, S1 = 0.0, S2 = 0.0, P[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) P[k] = 0.0;
    for (i64 base = first; base < last; base += OS_TILE) {
        const int cnt = (int)((last - base < OS_TILE) ? last - base : OS_TILE);
        __syncthreads();                                         // the tile before is read out
        if ((int)threadIdx.x < cnt) {
            const i64 m = base + threadIdx.x;
            const double xp = smc_ldg(o.Xprev + m);
            s_loc[threadIdx.x] = smc_ldg(o.loc + m);
            s_lw[threadIdx.x] = smc_ldg(o.lwprev + m);
            s_x[threadIdx.x] = xp;
            s_x2[threadIdx.x] = xp * xp;
#pragma unroll
            for (int k = 0; k < KP; ++k) s_phi[k][threadIdx.x] = (k < o.K) ? smc_ldg(o.Phi + m * o.K + k) : 0.0;
        }
        __syncthreads();
        double tm = -INFINITY;
        for (int j = 0; j < cnt; ++j) {
            const double v = (x - s_loc[j]) * rsc;
            const double l = fma(-0.5 * v, v, s_lw[j]);
            tm = (l > tm) ? l : tm;                              // (NaN never wins)
        }
        if (tm > mx) {                                           // once per tile at most: the sums move to the new maximum
            const double sc = (mx > -INFINITY) ? smc_exp_nonpos(mx - tm) : 0.0;
            S0 *= sc; S1 *= sc; S2 *= sc;
#pragma unroll
            for (int k = 0; k < KP; ++k) P[k] *= sc;
            mx = tm;
        }
        if (mx > -INFINITY) {
            for (int j = 0; j < cnt; ++j) {
                const double v = (x - s_loc[j]) * rsc;
                const double l = fma(-0.5 * v, v, s_lw[j]);
                const double e = (l > -INFINITY) ? smc_exp_nonpos(l - mx) : 0.0;      // (NaN weighs 0)
                S0 += e;
                S1 = fma(e, s_x[j], S1);
                S2 = fma(e, s_x2[j], S2);
#pragma unroll
                for (int k = 0; k < KP; ++k) P[k] = fma(e, s_phi[k][j], P[k]);
            }
        }
    }
    if (n >= N) return;
    double* out = o.part + ((i64)blockIdx.y * N + n) * OS_PART(KP);
    out[0] = mx; out[1] = S0; out[2] = S1; out[3] = S2;
#pragma unroll
    for (int k = 0; k < KP; ++k) out[4 + k] = P[k];
}

template <int KP>
__global__ void __launch_bounds__(SMC_BLOCK)
k_os_on2_merge(const OsPsi f, const double* X, const double* part, int nslices, i64 N, double* Phi)
{
    const i64 n = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (n >= N) return;
    double mx = -INFINITY;
    for (int s = 0; s < nslices; ++s) {
        const double m = smc_ldg(part + ((i64)s * N + n) * OS_PART(KP));
        mx = (m > mx) ? m : mx;
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, P[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) P[k] = 0.0;
    for (int s = 0; s < nslices; ++s) {                          // slice order: a fixed association
        const double* q = part + ((i64)s * N + n) * OS_PART(KP);
        const double m = smc_ldg(q);
        if (!(m > -INFINITY)) continue;
        const double sc = smc_exp_nonpos(m - mx);
        S0 = fma(sc, smc_ldg(q + 1), S0);
        S1 = fma(sc, smc_ldg(q + 2), S1);
        S2 = fma(sc, smc_ldg(q + 3), S2);
#pragma unroll
        for (int k = 0; k < KP; ++k) P[k] = fma(sc, smc_ldg(q + 4 + k), P[k]);
    }
    const double x = smc_ldg(X + n);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k >= f.K) break;
        double a[3];
        os_poly_x(f, k, x, a);
        // no finite l at all: the reference's exp_and_normalise gives NaN weights
        Phi[n * f.K + k] = (mx > -INFINITY) ? (((P[k] + a[0] * S0) + a[1] * S1) + a[2] * S2) / S0 : NAN;
    }
}

// est[k] = sum_n W_t[n] Phi[n, k]: chunk sums in a fixed order, then the chunks in order
#define OS_EST_CHUNK (16 * SMC_BLOCK)
__global__ void __launch_bounds__(SMC_BLOCK)
k_os_est_partials(const double* lw, const double* row, const double* Phi, i64 N, int K, int kform, double* part)
{
    __shared__ double smd[SMC_SM];
    const double m = smc_ldg(row + 5), rs = smc_ldg(row + 6);
    const i64 base = (i64)blockIdx.x * OS_EST_CHUNK;
    double acc[OS_KMAX];
#pragma unroll
    for (int k = 0; k < OS_KMAX; ++k) acc[k] = 0.0;
    for (int c = 0; c < OS_EST_CHUNK / SMC_BLOCK; ++c) {
        const i64 n = base + (i64)c * SMC_BLOCK + threadIdx.x;
        if (n < N) {
            const double w = sm_W(smc_ldg(lw + n), m, rs, kform);
#pragma unroll
            for (int k = 0; k < OS_KMAX; ++k)
                if (k < K) acc[k] = fma(w, smc_ldg(Phi + n * K + k), acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < OS_KMAX; ++k) {
        if (k >= K) break;                                       // (K is the workgroup's: every thread leaves together)
        const double v = smc_block_sum(acc[k], smd);
        if (threadIdx.x == 0) part[(i64)blockIdx.x * OS_KMAX + k] = v;
    }
}
__global__ void __launch_bounds__(64) k_os_est_final(const double* part, int nchunks, int K, double* est)
{
    const int k = (int)threadIdx.x;
    if (k >= K) return;
    double v = 0.0;
    for (int b = 0; b < nchunks; ++b) v += part[(i64)b * OS_KMAX + k];
    est[k] = v;
}

// ---------------------------------------------------------------------------
// host side helpers of smc_filter_online_smooth
// ---------------------------------------------------------------------------
// Source slices of the all-pairs launch.  SMC_ONLINE_SLICES (tests, measurements): another count; the result then differs
// in the association of the merge only.
static int os_slices(i64 N)
{
    const i64 nblk = (N + SMC_BLOCK - 1) / SMC_BLOCK, ntile = (N + OS_TILE - 1) / OS_TILE;
    const char* e = getenv("SMC_ONLINE_SLICES");
    i64 s = e && atoll(e) >= 1 ? (i64)atoll(e) : (OS_TARGET_WGS + nblk - 1) / nblk;
    s = s > ntile ? ntile : s;
    return (int)(s > 1024 ? 1024 : s < 1 ? 1 : s);
}
template <int KP>
static void os_launch_on2(hipStream_t st, const OsOn2& o, int nslices, const OsPsi& psi, double* Phi_out)
{
    const unsigned nblk = (unsigned)((o.N + SMC_BLOCK - 1) / SMC_BLOCK);
    SMC_LAUNCH((k_os_on2<KP>), dim3(nblk, (unsigned)nslices), dim3(SMC_BLOCK), st, o);
    SMC_LAUNCH((k_os_on2_merge<KP>), dim3(nblk), dim3(SMC_BLOCK), st, psi, o.X, (const double*)o.part, nslices, o.N, Phi_out);
}
