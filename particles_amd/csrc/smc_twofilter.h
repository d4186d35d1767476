// smc_twofilter.h -- two-filter smoothing (particles/smoothing.py:487-575, ParticleHistory.two_filter_smoothing; the
// O(N) form is Fearnhead, Wyncoll & Tawn 2010) over two resident histories: the forward filter f and the information
// filter g.  Host side: smc_filter_two_filter in smc_filter.hip.  The kernels read both histories and write their own
// workspaces only.
//
//   x_n = X_t[n] of f, n < N_f;   x'_m = X_ti[m] of g, m < N_i, ti = T_f - 2 - t
//   lwi_m = lw^g_ti[m] - loggamma(x'_m) [+ modif_info[m], O(N) form],  loggamma(x) = g0 + g1 x + g2 x^2
//   log p = the FORWARD filter's log p_{t+1}(x' | x); its constant -log(scale sqrt(2 pi)) -- and the reference's upb --
//           is the same for every pair, cancels in both estimators and is not formed in the all-pairs launch
//   phi_k(x, x') = sum_ij c[k][i][j] x^i x'^j   (smc_addfunc's t >= 1 form: os_psi(f, k, x, x'))
//
//   ON2  est[k] = sum_m sum_n w_nm phi_k(x_n, x'_m) / sum_m sum_n w_nm,  w_nm = exp(lw_t[n] + lwi_m + log p(x'_m | x_n) - c).
//        phi is a polynomial in the source x for a fixed target x', so a target needs three moments of its weights:
//        S0 = sum e, S1 = sum e x, S2 = sum e x^2 on the target's own maximum mx_m of l_n = lw_t[n] + log p, and hands on
//        ONE item (L_m = mx_m + lwi_m, S0, v_k = a_0k(x'_m) S0 + a_1k(x'_m) S1 + a_2k(x'_m) S2), a_ik as os_poly_x.
//        A -inf or NaN exponent weighs 0; no finite exponent at all: NaN.  This is the reference's value, not its rounding
//        order; and a NaN exponent poisons the reference's sum, here it weighs 0.
//   ON   P pairs (J_j, I_j): J the inverse of u_fwd[j] in the integer CDF of the forward weights (W_t as SMC_FIELD_W,
//        or e_n = exp(lw_t[n] + modif_forward[n] - max)), I the inverse of u_info[j] in the integer CDF of
//        e_m = exp(lwi_m - max lwi) -- sm_q, sm_threshold, sm_search of smc_smooth.h as they stand.
//        lo_j = log p(x'_I | x_J) - modif_forward[J] - modif_info[I]; item j = (lo_j, 1, phi_k(x_J, x'_I)).
//        Uniforms: replay tapes, or Philox stream SMC_STREAM_TWOFILTER, counter (j, t, island, 5): word x01 -> u_fwd,
//        word x23 -> u_info, both [0, 1).
//   both  items (L, s0, v[K]) reduce to G = max L, A = sum e^{L-G} s0, B_k = sum e^{L-G} v_k, C = sum (e^{L-G} s0)^2:
//        est[k] = B_k / A, ess = A^2 / C (= 1 / sum Om^2 of the O(N) form).  Chunk sums in a fixed order, then the chunks
//        in order: the same bits from run to run.
//
//   k_tf_lwi        lwi and its block maxima (also l_n = lw_t[n] + modif_forward[n] of the forward side)
//   k_tf_max_final  one workgroup: the maximum of the block maxima
//   k_tf_cdf_*      k_sm_cdf_totals / k_sm_cdf_scan on plain e = exp(l - max) instead of (lw, row)
//   k_tf_on2        one target (information-filter particle) per thread, grid (target blocks, source slices): k_os_on2's
//                   loop without the P[k] sums -- per tile the max sweep, at most one rescale, then S0, S1, S2; one
//                   smc_exp_nonpos and three fma per pair.  LDS: 4 SMC_BLOCK doubles = 8 KiB.
//   k_tf_merge      the slices of a target in slice order, then its item
//   k_tf_pairs      one pair per thread: two sm_search, one SmTrans::logpt; writes J, I and the pair's item (lo first)
//   k_tf_item_max / k_tf_item_sums / k_tf_final   the reduction of the items
#pragma once
#include "smc_online.h"

#define TF_CHUNK (16 * SMC_BLOCK)      /* items per workgroup of the two item launches */
#define TF_PART (OS_KMAX + 2)          /* doubles per chunk partial: A, C, B[OS_KMAX] */

struct TfGamma { double g0, g1, g2; int on; };

// out[m] = lw[m] - loggamma(X[m]) (g.on) + modif[m] (modif != null); bmax[block] = the block's maximum (NaN never wins)
__global__ void __launch_bounds__(SMC_BLOCK)
k_tf_lwi(const double* lw, const double* X, const TfGamma g, const double* modif, i64 N, double* out, double* bmax)
{
    __shared__ double smd[SMC_SM];
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    double l = -INFINITY;
    if (m < N) {
        l = smc_ldg(lw + m);
        if (g.on) {
            const double x = smc_ldg(X + m);
            l -= fma(fma(g.g2, x, g.g1), x, g.g0);
        }
        if (modif) l += smc_ldg(modif + m);
        out[m] = l;
    }
    const double mx = smc_block_max((l > -INFINITY) ? l : -INFINITY, smd);
    if (threadIdx.x == 0) bmax[blockIdx.x] = mx;
}
__global__ void __launch_bounds__(SMC_BLOCK) k_tf_max_final(const double* bmax, i64 nb, double* out)
{
    __shared__ double smd[SMC_SM];
    double mx = -INFINITY;
    for (i64 b = threadIdx.x; b < nb; b += SMC_BLOCK) {
        const double v = bmax[b];
        mx = (v > mx) ? v : mx;
    }
    mx = smc_block_max(mx, smd);
    if (threadIdx.x == 0) out[0] = mx;
}

// e = exp(l - max), 0 for -inf and NaN; max = -inf (no finite l): every e is 0, Q = 0 and sm_search gives N - 1
__device__ __forceinline__ double tf_e(double l, double mx)
{
    return (l > -INFINITY && mx > -INFINITY) ? smc_exp_nonpos(fmin(l - mx, 0.0)) : 0.0;
}
__global__ void __launch_bounds__(SMC_BLOCK) k_tf_cdf_totals(const double* l, const double* gmax, i64 N, int shift, u64* tot)
{
    __shared__ u64 smu[SMC_SM];
    const double mx = gmax[0];
    const i64 base = (i64)blockIdx.x * SM_CHUNK;
    u64 acc = 0;
    for (int k = 0; k < SM_CHUNK / SMC_BLOCK; ++k) {
        const i64 n = base + (i64)k * SMC_BLOCK + threadIdx.x;
        if (n < N) acc += sm_q(tf_e(smc_ldg(l + n), mx), shift);
    }
    acc = smc_block_sum_u64(acc, smu);
    if (threadIdx.x == 0) tot[blockIdx.x] = acc;
}
__global__ void __launch_bounds__(SMC_BLOCK)
k_tf_cdf_scan(const double* l, const double* gmax, i64 N, int shift, const u64* tot, u64* cdf)
{
    __shared__ u64 smu[SMC_SM];
    const double mx = gmax[0];
    u64 before = 0;
    for (int b = (int)threadIdx.x; b < (int)blockIdx.x; b += SMC_BLOCK) before += tot[b];
    u64 run = smc_block_sum_u64(before, smu);
    const i64 base = (i64)blockIdx.x * SM_CHUNK;
    for (int k = 0; k < SM_CHUNK / SMC_BLOCK; ++k) {
        const i64 n = base + (i64)k * SMC_BLOCK + threadIdx.x;
        const u64 q = (n < N) ? sm_q(tf_e(smc_ldg(l + n), mx), shift) : 0ull;
        u64 total;
        const u64 ex = smc_block_exscan_u64(q, smu, total);
        if (n < N) cdf[n] = run + ex + q;
        run += total;
    }
}

// ---------------------------------------------------------------------------
// ON2: the all-pairs launch and its merge
// ---------------------------------------------------------------------------
struct TfOn2 {
    const double *Xi;                  // (Ni) targets: the information filter's particles
    const double *Xf, *lwf, *loc;      // (Nf) sources: state, log-weight, loc = m_trans_loc(p, x_n, aux[t + 1])
    double* part;                      // (nslices, Ni, 4): max, S0, S1, S2
    const double* p;                   // the forward island's params row
    int slot;                          // ... its transition scale: p[slot], RN(1 / scale) at p[16 + slot]
    i64 Ni, Nf, per_slice;             // sources per slice: a multiple of SMC_BLOCK
};

__global__ void __launch_bounds__(SMC_BLOCK) k_tf_on2(const TfOn2 o)
{
    __shared__ double s_loc[SMC_BLOCK], s_lw[SMC_BLOCK], s_x[SMC_BLOCK], s_x2[SMC_BLOCK];
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    const double x = (m < o.Ni) ? smc_ldg(o.Xi + m) : 0.0;      // (a thread past Ni stages and idles: every barrier is its too)
    const i64 first = (i64)blockIdx.y * o.per_slice;
    const i64 last = (first + o.per_slice < o.Nf) ? first + o.per_slice : o.Nf;
    // the product form of k_os_on2, with its fallback when the stored reciprocal is 0 (see there)
    double rsc = smc_ldg(o.p + 16 + o.slot);
    if (!(rsc > 0.0)) rsc = 1.0 / smc_ldg(o.p + o.slot);
    double mx = -INFINITY, S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (i64 base = first; base < last; base += SMC_BLOCK) {
        const int cnt = (int)((last - base < SMC_BLOCK) ? last - base : SMC_BLOCK);
        __syncthreads();                                         // the tile before is read out
        if ((int)threadIdx.x < cnt) {
            const i64 n = base + threadIdx.x;
            const double xs = smc_ldg(o.Xf + n);
            s_loc[threadIdx.x] = smc_ldg(o.loc + n);
            s_lw[threadIdx.x] = smc_ldg(o.lwf + n);
            s_x[threadIdx.x] = xs;
            s_x2[threadIdx.x] = xs * xs;
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
            }
        }
    }
    if (m >= o.Ni) return;
    double* out = o.part + ((i64)blockIdx.y * o.Ni + m) * 4;
    out[0] = mx; out[1] = S0; out[2] = S1; out[3] = S2;
}

// items[m] = (L, S0, v[K]), stride K + 2
__global__ void __launch_bounds__(SMC_BLOCK)
k_tf_merge(const OsPsi f, const double* Xi, const double* lwi, const double* part, int nslices, i64 Ni, double* items)
{
    const i64 m = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (m >= Ni) return;
    double mx = -INFINITY;
    for (int s = 0; s < nslices; ++s) {
        const double v = smc_ldg(part + ((i64)s * Ni + m) * 4);
        mx = (v > mx) ? v : mx;
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (int s = 0; s < nslices; ++s) {                          // slice order: a fixed association
        const double* q = part + ((i64)s * Ni + m) * 4;
        const double v = smc_ldg(q);
        if (!(v > -INFINITY)) continue;
        const double sc = smc_exp_nonpos(v - mx);
        S0 = fma(sc, smc_ldg(q + 1), S0);
        S1 = fma(sc, smc_ldg(q + 2), S1);
        S2 = fma(sc, smc_ldg(q + 3), S2);
    }
    const double x = smc_ldg(Xi + m);
    double* it = items + m * (f.K + 2);
    it[0] = mx + smc_ldg(lwi + m);
    it[1] = S0;
    for (int k = 0; k < f.K; ++k) {
        double a[3];
        os_poly_x(f, k, x, a);
        it[2 + k] = (a[0] * S0 + a[1] * S1) + a[2] * S2;
    }
}

// ---------------------------------------------------------------------------
// ON: the pairs
// ---------------------------------------------------------------------------
struct TfPairs {
    const double *Xi;                  // (Ni) the information filter's particles (SmArgs: Xt = the forward ones, N = Nf)
    const u64 *cdf_f, *cdf_i;          // (Nf), (Ni) inclusive integer CDFs; null with given indices
    const double *u_f, *u_i;           // (P) replay tapes or null: Philox
    const i64 *J_in, *I_in;            // (P) given pairs or null
    const double *mf, *mi;             // (Nf), (Ni) modif_forward, modif_info or null
    i64 *J, *I;                        // (P) out
    double* items;                     // (P, K + 2): item j = (lo_j, 1, phi_k)
    i64 Ni, P;
};

template <int KIND>
__global__ void __launch_bounds__(SMC_BLOCK) k_tf_pairs(const SmArgs s, const TfPairs q, const OsPsi f)
{
    const i64 j = (i64)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (j >= q.P) return;
    i64 J, I;
    if (q.J_in) {
        J = smc_ldg(q.J_in + j);
        I = smc_ldg(q.I_in + j);
    } else {
        double uf, ui;
        if (q.u_f && q.u_i) {
            uf = smc_ldg(q.u_f + j);
            ui = smc_ldg(q.u_i + j);
        } else {
            u64 a, b;
            smc_philox((u32)j, s.t, s.island, SMC_STREAM_TWOFILTER, s.seed, a, b);
            uf = q.u_f ? smc_ldg(q.u_f + j) : smc_u01_halfopen(a);
            ui = q.u_i ? smc_ldg(q.u_i + j) : smc_u01_halfopen(b);
        }
        J = sm_search(q.cdf_f, s.N, uf);
        I = sm_search(q.cdf_i, q.Ni, ui);
    }
    const SmTrans<KIND> tr(s);
    const double x = smc_ldg(s.Xt + J), xi = smc_ldg(q.Xi + I);
    double lo = tr.logpt(x, xi);
    if (q.mf) lo -= smc_ldg(q.mf + J);
    if (q.mi) lo -= smc_ldg(q.mi + I);
    q.J[j] = J;
    q.I[j] = I;
    double* it = q.items + j * (f.K + 2);
    it[0] = lo;
    it[1] = 1.0;
    for (int k = 0; k < f.K; ++k) it[2 + k] = os_psi(f, k, x, xi);
}

// ---------------------------------------------------------------------------
// the reduction of the items (both methods)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SMC_BLOCK) k_tf_item_max(const double* items, int stride, i64 n, double* cmax)
{
    __shared__ double smd[SMC_SM];
    const i64 base = (i64)blockIdx.x * TF_CHUNK;
    double mx = -INFINITY;
    for (int c = 0; c < TF_CHUNK / SMC_BLOCK; ++c) {
        const i64 i = base + (i64)c * SMC_BLOCK + threadIdx.x;
        if (i < n) {
            const double L = smc_ldg(items + i * stride);
            mx = (L > mx) ? L : mx;                              // (NaN never wins)
        }
    }
    mx = smc_block_max(mx, smd);
    if (threadIdx.x == 0) cmax[blockIdx.x] = mx;
}
// part[chunk] = (A, C, B[K]) on G = gmax[0]
__global__ void __launch_bounds__(SMC_BLOCK)
k_tf_item_sums(const double* items, int stride, i64 n, int K, const double* gmax, double* part)
{
    __shared__ double smd[SMC_SM];
    const double G = gmax[0];
    const i64 base = (i64)blockIdx.x * TF_CHUNK;
    double A = 0.0, C = 0.0, B[OS_KMAX];
#pragma unroll
    for (int k = 0; k < OS_KMAX; ++k) B[k] = 0.0;
    for (int c = 0; c < TF_CHUNK / SMC_BLOCK; ++c) {
        const i64 i = base + (i64)c * SMC_BLOCK + threadIdx.x;
        if (i < n) {
            const double* it = items + i * stride;
            const double e = tf_e(smc_ldg(it), G);
            if (e > 0.0) {                                       // (a weightless item's sums may be anything: NaN moments of no pair)
                const double w = e * smc_ldg(it + 1);
                A += w;
                C = fma(w, w, C);
#pragma unroll
                for (int k = 0; k < OS_KMAX; ++k)
                    if (k < K) B[k] = fma(e, smc_ldg(it + 2 + k), B[k]);
            }
        }
    }
    double* out = part + (i64)blockIdx.x * TF_PART;
    double v = smc_block_sum(A, smd);
    if (threadIdx.x == 0) out[0] = v;
    v = smc_block_sum(C, smd);
    if (threadIdx.x == 0) out[1] = v;
#pragma unroll
    for (int k = 0; k < OS_KMAX; ++k) {
        if (k >= K) break;                                       // (K is the workgroup's: every thread leaves together)
        v = smc_block_sum(B[k], smd);
        if (threadIdx.x == 0) out[2 + k] = v;
    }
}
// out[k] = est[k], k < K; out[OS_KMAX] = ess.  A = 0 (no finite exponent at all): NaN
__global__ void __launch_bounds__(64) k_tf_final(const double* part, int nchunks, int K, double* out)
{
    const int k = (int)threadIdx.x;
    if (k > K) return;
    double A = 0.0;
    for (int b = 0; b < nchunks; ++b) A += part[(i64)b * TF_PART];
    double v = 0.0;
    const int col = (k < K) ? 2 + k : 1;
    for (int b = 0; b < nchunks; ++b) v += part[(i64)b * TF_PART + col];
    if (k < K) out[k] = v / A;
    else out[OS_KMAX] = (A * A) / v;
}

// ---------------------------------------------------------------------------
// host side helpers of smc_filter_two_filter
// ---------------------------------------------------------------------------
// Source slices of the all-pairs launch: os_slices with targets = Ni and sources = Nf -- a function of the sizes alone,
// because the merge order is part of the result.  SMC_TWOFILTER_SLICES (tests, measurements): another count.
static int tf_slices(i64 Ni, i64 Nf)
{
    const i64 nblk = (Ni + SMC_BLOCK - 1) / SMC_BLOCK, ntile = (Nf + SMC_BLOCK - 1) / SMC_BLOCK;
    const char* e = getenv("SMC_TWOFILTER_SLICES");
    i64 s = e && atoll(e) >= 1 ? (i64)atoll(e) : (OS_TARGET_WGS + nblk - 1) / nblk;
    s = s > ntile ? ntile : s;
    return (int)(s > 1024 ? 1024 : s < 1 ? 1 : s);
}
// cdf = the integer CDF of e = exp(l - max l); bmax: the block maxima of l (k_tf_lwi), gmax: one word
static void tf_cdf_of(hipStream_t st, const double* l, const double* bmax, i64 N, double* gmax, u64* tot, u64* cdf)
{
    const unsigned nch = (unsigned)((N + SM_CHUNK - 1) / SM_CHUNK);
    SMC_LAUNCH(k_tf_max_final, dim3(1), dim3(SMC_BLOCK), st, bmax, (N + SMC_BLOCK - 1) / SMC_BLOCK, gmax);
    SMC_LAUNCH(k_tf_cdf_totals, dim3(nch), dim3(SMC_BLOCK), st, l, (const double*)gmax, N, sm_shift(N), tot);
    SMC_LAUNCH(k_tf_cdf_scan, dim3(nch), dim3(SMC_BLOCK), st, l, (const double*)gmax, N, sm_shift(N), (const u64*)tot, cdf);
}
