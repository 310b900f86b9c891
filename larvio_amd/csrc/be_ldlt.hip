// be_ldlt.hip — pivoted LDL^T of the innovation covariance for gfx950 (wave64), FP64: the route the measurement update takes when
// S = H P H^T + sigma^2 I is not positive definite (lvk_ekf_update_ldlt, LVK_INDEFINITE_LDLT).  The algorithm is the one the
// reference runs, S.ldlt().solve(H P) (larvio.cpp:1456, 1655, 2830), as oracle/ref_shim2/lvref_eigen2.hpp (LDLTx) states it:
//     P_pi S P_pi^T = L D L^T,   at step k the remaining diagonal entry of largest magnitude becomes the pivot (first one on a tie),
//     X = P_pi^T L^-T D^-1 L^-1 P_pi B,   a D entry of magnitude <= DBL_MIN gives a zero component instead of a division.
// This path runs once in a diverging filter's lifetime: it is written for a bounded run time and no dependence on anything another
// workgroup does, not for speed.
//   k_ldlt_factor: ONE workgroup.  m reaches the state size, so S (m x m doubles, 871 KB at m = 330) stays in global memory (L2
//     resident) and the factor works on panels of LDLT_NB columns: the finished columns of the active panel live in LDS, column k is
//     formed left-looking from the raw column in global memory minus the panel's finished columns, and the diagonal every pivot search
//     looks at is kept up to date in LDS (dg: one subtraction per step and entry, the same sequence an unblocked right-looking
//     factorisation applies).  After a panel the trailing lower triangle takes S22 -= L21 D L21^T on the FP64 matrix cores
//     (v_mfma_f64_16x16x4_f64, operand layout as in k_dgemm_sk).  Only the lower triangle of S is read; symmetric swaps move the
//     row part left of the diagonal and the column part below it.
//   k_ldlt_solve: one thread per right-hand column, no communication at all: gathers the permuted rows, forward substitution,
//     D^-1 with the zero rule, backward substitution.  The result stays in pivot order (row i belongs to row perm[i] of S) next to
//     the equally permuted copy of B: every product the update needs is a sum over rows, which the order does not change.
#include "lvk_internal.h"
#include "be_host.h"
#include "lvk_wave.h"
#include <cfloat>

typedef double d4 __attribute__((ext_vector_type(4)));

#define LDLT_NB 16
#define LS_RB 16            // rows per register block of the substitutions
#define LDLT_LD 17          // LDS row stride of the panel (odd: the 16 rows an MFMA operand reads fall into different banks)

// report words: cnt[0] = negative D entries, cnt[1] = zero D entries (|d| <= DBL_MIN)
__global__ void __launch_bounds__(256) k_ldlt_factor(double* __restrict__ S, int ld, int m, double* __restrict__ Dg, int* __restrict__ perm, int* __restrict__ cnt)
{
    extern __shared__ __attribute__((aligned(16))) double ldlt_smem[];
    double* dg = ldlt_smem;                                  // m (rounded up to even): the up-to-date diagonal of the trailing block
    double* Lp = ldlt_smem + ((m + 1) & ~1);                 // (m - k0) x LDLT_LD: finished columns of the active panel, row i - k0
    __shared__ double red_v[4]; __shared__ int red_i[4]; __shared__ double Dp[LDLT_NB]; __shared__ int s_cnt[2];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kk = lane >> 4;
    for (int i = t; i < m; i += 256) { dg[i] = S[(size_t)i * ld + i]; perm[i] = i; }
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    for (int k0 = 0; k0 < m; k0 += LDLT_NB) {
        const int nb = min(LDLT_NB, m - k0);
        for (int j = 0; j < nb; ++j) {
            const int k = k0 + j;
            // ---- pivot: the first index of the largest |dg[i]|, i >= k (a NaN never wins; all NaN: k stays)
            double best = -1.0; int bi = m;
            for (int i = k + t; i < m; i += 256) { const double a = fabs(dg[i]); if (a > best) { best = a; bi = i; } }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off); const int oi = __shfl_xor(bi, off);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (lane == 0) { red_v[wave] = best; red_i[wave] = bi; }
            __syncthreads();
            int p = red_i[0]; { double b = red_v[0]; for (int w = 1; w < 4; ++w) if (red_v[w] > b || (red_v[w] == b && red_i[w] < p)) { b = red_v[w]; p = red_i[w]; } }
            if (p >= m) p = k;
            // ---- symmetric swap of k and p in the lower triangle (columns k0..k-1 of the two rows live in Lp)
            if (p != k) {
                double* Sk = S + (size_t)k * ld; double* Sp = S + (size_t)p * ld;
                for (int c = t; c < k0; c += 256) { const double a = Sk[c]; Sk[c] = Sp[c]; Sp[c] = a; }
                if (t < j) { double* a = Lp + (size_t)(k - k0) * LDLT_LD + t; double* b = Lp + (size_t)(p - k0) * LDLT_LD + t; const double v = *a; *a = *b; *b = v; }
                for (int i = k + 1 + t; i < p; i += 256) { double* a = S + (size_t)i * ld + k; const double v = *a; *a = Sp[i]; Sp[i] = v; }
                for (int i = p + 1 + t; i < m; i += 256) { double* a = S + (size_t)i * ld; const double v = a[k]; a[k] = a[p]; a[p] = v; }
                if (t == 0) { const double v = dg[k]; dg[k] = dg[p]; dg[p] = v; const int q = perm[k]; perm[k] = perm[p]; perm[p] = q; }
            }
            __syncthreads();
            // ---- column k: raw column minus the panel's finished columns, scaled by the pivot (a zero pivot leaves a zero column)
            const double d = dg[k];
            double lk[LDLT_NB];                               // D_t L[k][t] of the finished columns
#pragma unroll
            for (int u = 0; u < LDLT_NB; ++u) lk[u] = u < j ? Lp[(size_t)(k - k0) * LDLT_LD + u] * Dp[u] : 0.0;
            for (int i = k + 1 + t; i < m; i += 256) {
                double* li = Lp + (size_t)(i - k0) * LDLT_LD;
                double v = S[(size_t)i * ld + k];
#pragma unroll
                for (int u = 0; u < LDLT_NB; ++u) if (u < j) v -= li[u] * lk[u];
                const double l = d != 0.0 ? v / d : 0.0;
                li[j] = l;
                dg[i] -= l * (l * d);
            }
            if (t == 0) {
                Dg[k] = d; Dp[j] = d;
                if (d < -DBL_MIN) s_cnt[0]++; else if (!(d > DBL_MIN)) s_cnt[1]++;       // (a NaN pivot counts as zero: it solves to a zero component)
            }
            __syncthreads();
        }
        // ---- the panel's columns go to their place in S (strictly lower part; the diagonal of L is 1 and is not stored)
        for (int e = t; e < (m - k0) * LDLT_NB; e += 256) {
            const int a = e / LDLT_NB, u = e % LDLT_NB;
            if (u < nb && u < a) S[(size_t)(k0 + a) * ld + k0 + u] = Lp[(size_t)a * LDLT_LD + u];
        }
        // ---- trailing update of the lower triangle right of the panel: S22 -= L21 D L21^T, one 16 x 16 tile per wavefront and turn
        const int c0 = k0 + LDLT_NB;
        if (c0 < m) {                                         // (then nb == LDLT_NB)
            const int nt = (m - c0 + 15) / 16;
            int u = 0;
            for (int ti = 0; ti < nt; ++ti)
                for (int tj = 0; tj <= ti; ++tj, ++u) {
                    if ((u & 3) != wave) continue;
                    const int ra = c0 + 16 * ti + i16, rb = c0 + 16 * tj + i16;       // rows of L21 feeding A (tile rows) and B (tile columns)
                    d4 acc = {0., 0., 0., 0.};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int kq = 4 * q + kk;
                        const double a = ra < m ? Lp[(size_t)(ra - k0) * LDLT_LD + kq] : 0.0;
                        const double b = rb < m ? Lp[(size_t)(rb - k0) * LDLT_LD + kq] * Dp[kq] : 0.0;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = c0 + 16 * ti + kk + 4 * r, col = c0 + 16 * tj + i16;
                        if (row < m && col < row) S[(size_t)row * ld + col] -= acc[r];       // (the diagonal lives in dg)
                    }
                }
        }
        __syncthreads();
    }
    if (t < 2) cnt[t] = s_cnt[t];
}

// Bp (m x ldb) <- rows of B in pivot order; X (m x ldb) <- D^-1-scaled two-sided triangular solve of the same, in pivot order.
// L: strictly lower triangle of S (unit diagonal implied).  One thread per column, columns coalesced across the wavefront; the
// entries of L are uniform over the workgroup.
__global__ void __launch_bounds__(64) k_ldlt_solve(const double* __restrict__ S, int ld, int m, const double* __restrict__ Dg, const int* __restrict__ perm,
                                                  const double* __restrict__ B, int ldb, int nbcols, double* __restrict__ Bp, double* __restrict__ X)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nbcols) return;
    for (int i = 0; i < m; ++i) { const double v = B[(size_t)perm[i] * ldb + c]; Bp[(size_t)i * ldb + c] = v; X[(size_t)i * ldb + c] = v; }
    // forward: LS_RB rows at a time in registers - every earlier x_k is loaded once for LS_RB independent subtractions (the one-row
    // form, a dependent chain of m^2 / 2 loads per thread, took 12 ms at m = 330) - then the block's own triangle
    for (int i0 = 0; i0 < m; i0 += LS_RB) {
        const int nr = min(LS_RB, m - i0);
        double y[LS_RB];
#pragma unroll
        for (int u = 0; u < LS_RB; ++u) y[u] = u < nr ? X[(size_t)(i0 + u) * ldb + c] : 0.0;
        for (int k = 0; k < i0; ++k) {
            const double xk = X[(size_t)k * ldb + c];
#pragma unroll
            for (int u = 0; u < LS_RB; ++u) if (u < nr) y[u] -= S[(size_t)(i0 + u) * ld + k] * xk;
        }
#pragma unroll
        for (int u = 1; u < LS_RB; ++u)
#pragma unroll
            for (int v = 0; v < u; ++v) if (u < nr) y[u] -= S[(size_t)(i0 + u) * ld + i0 + v] * y[v];
#pragma unroll
        for (int u = 0; u < LS_RB; ++u) if (u < nr) X[(size_t)(i0 + u) * ldb + c] = y[u];
    }
    for (int i = 0; i < m; ++i) { const double d = Dg[i]; double* x = X + (size_t)i * ldb + c; *x = fabs(d) > DBL_MIN ? *x / d : 0.0; }
    // backward (L^T), the same way from the last block up: row k of L holds the LS_RB factors of a block side by side
    for (int i0 = ((m - 1) / LS_RB) * LS_RB; i0 >= 0; i0 -= LS_RB) {
        const int nr = min(LS_RB, m - i0);
        double y[LS_RB];
#pragma unroll
        for (int u = 0; u < LS_RB; ++u) y[u] = u < nr ? X[(size_t)(i0 + u) * ldb + c] : 0.0;
        for (int k = i0 + nr; k < m; ++k) {
            const double xk = X[(size_t)k * ldb + c];
            const double* lk = S + (size_t)k * ld + i0;
#pragma unroll
            for (int u = 0; u < LS_RB; ++u) if (u < nr) y[u] -= lk[u] * xk;
        }
#pragma unroll
        for (int u = LS_RB - 2; u >= 0; --u)
#pragma unroll
            for (int v = u + 1; v < LS_RB; ++v) if (v < nr) y[u] -= S[(size_t)(i0 + v) * ld + i0 + u] * y[v];
#pragma unroll
        for (int u = 0; u < LS_RB; ++u) if (u < nr) X[(size_t)(i0 + u) * ldb + c] = y[u];
    }
}

// P <- (P + P^T) / 2 (larvio.cpp:1592-1594): thread (i, j), j < i, owns the pair - exactly symmetric, nothing else is touched
__global__ void __launch_bounds__(256) k_cov_symmetrize(double* __restrict__ P, int ld, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= i || i >= n) return;
    double* a = P + (size_t)i * ld + j; double* b = P + (size_t)j * ld + i;
    const double v = (*a + *b) / 2.0;
    *a = v; *b = v;
}

size_t lvk_ldlt_lds_bytes(int m) { return sizeof(double) * ((size_t)((m + 1) & ~1) + (size_t)m * LDLT_LD); }

// S (m x m, lower triangle read, overwritten by L), B (m x nbcols) -> Bp, X in pivot order; Dg (m), perm (m), cnt (2 ints) on the device
lvk_status lvk_ldlt_factor_solve(lvk_context* ctx, double* S, int ld, int m, const double* B, int ldb, int nbcols, double* Bp, double* X,
                                 double* Dg, int* perm, int* cnt)
{
    const size_t shm = lvk_ldlt_lds_bytes(m);
    if (shm > 158 * 1024) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "pivoted LDLT: %d rows do not fit the factor kernel's LDS", m);
    if (shm > 60 * 1024) LVK_LDS_OPTIN(ctx, k_ldlt_factor, shm);
    hipLaunchKernelGGL(k_ldlt_factor, dim3(1), dim3(256), shm, ctx->stream, S, ld, m, Dg, perm, cnt);
    hipLaunchKernelGGL(k_ldlt_solve, dim3((nbcols + 63) / 64), dim3(64), 0, ctx->stream, (const double*)S, ld, m, (const double*)Dg, (const int*)perm, B, ldb, nbcols, Bp, X);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
void lvk_cov_symmetrize(lvk_context* ctx, double* P, int ld, int n)
{
    if (n > 1) hipLaunchKernelGGL(k_cov_symmetrize, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, P, ld, n);
}
