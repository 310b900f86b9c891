// be_landmark_fix.hip — image observations of points whose world position is known, fused on one clone of the window
// (lvk_ekf_update_landmarks, include/lvk_c.h: up to 1024 observations of one image, twelve columns of P, a chi-square gate per
// observation, a Householder compression to twelve rows, gate and "nothing to apply" decided on the device) with its three kernels, and
// the filter's batch queue (lvk_ekf_add_landmark_obs and what goes with it; lvk_ekf_apply_landmarks is the stage backend.hip's
// ekf_process_impl runs behind lvk_ekf_apply_fixes).
#include "be_filter.h"
#include "be_host_math.h"
#include "lvk_wave.h"
#include <math.h>

#define LM_COLS 12
#define LM_ROWS 12
#define LM_W 13                   // the twelve columns and the residual
#define LM_MAX_OBS 1024
#define LM_HDR 4                  // doubles in front of the compressed system: rows m, then three spare
// A column of the compression counts as dependent on the columns before it when what the reflections before it have left of its squared
// norm is at most this fraction of the squared norm it started with (2^-60: 2^-30 of the norm).  The twelve columns act through the
// camera's pose alone, so the rows have rank 6 at the most; what is left of a dependent column is the rounding of a dozen operations per
// entry, some 1e-15 of the norm, while a pose direction a handful of points in general position determine keeps 1e-3 of it and more.
#define LM_RANK_TOL2 8.673617379884035e-19

// column of P behind entry k of [d_theta_e d_t | d_theta_b d_p_b]
__device__ __forceinline__ int lm_col(int k, int clone_col) { return k < 6 ? 15 + k : clone_col + (k - 6); }

// Eigen's Quaternion::toRotationMatrix, q = [x y z w] (be_host_math.h, quat_to_rot)
__device__ __forceinline__ void lm_quat_to_rot(const double* q, double* R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy; R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// First launch, ONE workgroup, one lane per observation.  With R_b = R(q_b) (body to world), R_e = R_b2c, M = R_e R_b^T (formed once,
// by lane 0, and read by all):
//   g = p_w - p_b (first: the size of the world coordinates stays out of the rounding),  y = R_b^T g - t_c_b,  p_c = R_e y,
//   D = [R_e [y]x | -R_e | M [g]x | -M],  J = [1/z 0 -x/z^2; 0 1/z -y/z^2],  H = J D (2 x 12),  r = uv - (x/z, y/z),
//   R_k = sigma^2 I + (J M) Sigma_w (J M)^T,  S = H P_s H^T + R_k = L L^T,  gamma = |L^-1 r|^2,
// P_s the 12 x 12 sub-block of P every lane reads from LDS (nothing else of P is read here).  Status: 2 behind (not p_c.z > min_depth;
// nothing else is computed, gamma 0), 1 gated (gate > 0 and not gamma <= gate; also a pivot of S or of R_k that is not > 0, gamma 0), 0 used.
// A used lane whitens its two rows and residual by the Cholesky factor of R_k and gets its index among the used observations - a
// count of ballots, so the compact order is the batch's order - and stores its 2 x 13 block there (work space `rows`).
// Then the compression.  n_used <= 6: the blocks ARE the system, m = 2 n_used rows.  Otherwise lane t takes block t back (lanes beyond
// n_used hold zeros) and the workgroup runs twelve Householder reflections on [0 (12 x 13); A]: reflection j involves row j of the zero
// block and all of A, its vector is [-|a_j|; a_j], and it leaves
//   R[j][j] = |a_j|,  R[j][k] = a_j.a_k / |a_j|,  a_k <- a_k - (a_j.a_k / a_j.a_j) a_j   (k = j+1..12, the residual being column 12)
// - no Gram matrix is formed or factored.  The rank is decided here: a column of which the reflections before it have left no more than
// LM_RANK_TOL2 of its squared norm depends on them, its reflection is dropped and it gives no row - so the system has m = rank rows
// (6 for points in general position), none of them rounding noise, and gamma of the batch is that of the residual inside their range.  Every inner product is summed the same way whatever the launch: a lane's two rows, the
// wavefront's 64 lanes by wave_sum_f64 (a fixed tree; idle lanes add zeros), then the wavefronts' sums in ascending order (absent
// wavefronts would add zeros) - so the system depends on the used observations and their order only, not on what lay between them.
// sys: [m, 0, 0, 0 | m x 13 row-major].  info (8 doubles): this launch writes [3] n_used [4] n_gated [5] n_behind [6] m [7] 0.
// NT: the most lanes a launch may have (256 leaves every lane the registers its two rows need; the arithmetic is the same).
template <int NT>
__global__ __launch_bounds__(NT) void k_lm_rows(const double* __restrict__ P, int ld, const lvk_landmark_fix_job* __restrict__ job,
                                                const lvk_landmark_obs* __restrict__ obs, int n_obs, double* __restrict__ rows, double* __restrict__ sys,
                                                int* __restrict__ status_out, double* __restrict__ gamma_out, double* __restrict__ info)
{
    __shared__ double Ps[LM_COLS * LM_COLS], Rbs[9], Res[9], Ms[9], red[2][NT / 64][LM_W], c0w[NT / 64][LM_COLS], c0[LM_COLS];
    __shared__ int cnt[NT / 64][3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
    const int cc = job->clone_col;
    for (int k = t; k < LM_COLS * LM_COLS; k += blockDim.x) Ps[k] = P[(size_t)lm_col(k / LM_COLS, cc) * ld + lm_col(k % LM_COLS, cc)];
    if (t == 0) {
        double Rb[9];
        lm_quat_to_rot(job->q_b, Rb);
        for (int i = 0; i < 9; ++i) { Rbs[i] = Rb[i]; Res[i] = job->R_b2c[i]; }
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0.; for (int k = 0; k < 3; ++k) s += job->R_b2c[i * 3 + k] * Rb[j * 3 + k]; Ms[i * 3 + j] = s; }
    }
    __syncthreads();
    double a0[LM_W], a1[LM_W];                          // the lane's two whitened rows, residual last
#pragma unroll
    for (int k = 0; k < LM_W; ++k) { a0[k] = 0.; a1[k] = 0.; }
    int st = -1;                                        // (no observation on this lane)
    double gamma = 0.;
    if (t < n_obs) {
        const lvk_landmark_obs* o = obs + t;
        double Rb[9], Re[9], M[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { Rb[i] = Rbs[i]; Re[i] = Res[i]; M[i] = Ms[i]; }
        const double g[3] = {o->p_w[0] - job->p_b[0], o->p_w[1] - job->p_b[1], o->p_w[2] - job->p_b[2]};
        double y[3], pc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) y[i] = (Rb[i] * g[0] + Rb[3 + i] * g[1] + Rb[6 + i] * g[2]) - job->t_c_b[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pc[i] = Re[i * 3] * y[0] + Re[i * 3 + 1] * y[1] + Re[i * 3 + 2] * y[2];
        st = pc[2] > job->min_depth ? 0 : 2;            // (a NaN would land on 2; the host lets none in)
        if (st == 0) {
            const double Sy[9] = {0, -y[2], y[1], y[2], 0, -y[0], -y[1], y[0], 0};
            const double Sg[9] = {0, -g[2], g[1], g[2], 0, -g[0], -g[1], g[0], 0};
            double D[3 * LM_COLS];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    D[i * LM_COLS + c] = Re[i * 3] * Sy[c] + Re[i * 3 + 1] * Sy[3 + c] + Re[i * 3 + 2] * Sy[6 + c];
                    D[i * LM_COLS + 3 + c] = -Re[i * 3 + c];
                    D[i * LM_COLS + 6 + c] = M[i * 3] * Sg[c] + M[i * 3 + 1] * Sg[3 + c] + M[i * 3 + 2] * Sg[6 + c];
                    D[i * LM_COLS + 9 + c] = -M[i * 3 + c];
                }
            const double iz = 1. / pc[2], zz = pc[2] * pc[2];
            const double jx = -(pc[0] / zz), jy = -(pc[1] / zz);
            double h0[LM_COLS], h1[LM_COLS], jm0[3], jm1[3];
#pragma unroll
            for (int c = 0; c < LM_COLS; ++c) { h0[c] = iz * D[c] + jx * D[2 * LM_COLS + c]; h1[c] = iz * D[LM_COLS + c] + jy * D[2 * LM_COLS + c]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) { jm0[c] = iz * M[c] + jx * M[6 + c]; jm1[c] = iz * M[3 + c] + jy * M[6 + c]; }
            const double r0 = o->uv[0] - pc[0] / pc[2], r1 = o->uv[1] - pc[1] / pc[2];
            // R_k: Sigma_w from its upper triangle
            const double* cw = o->cov_w;
            const double Sw[9] = {cw[0], cw[1], cw[2], cw[1], cw[4], cw[5], cw[2], cw[5], cw[8]};
            double t0[3], t1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { t0[c] = jm0[0] * Sw[c] + jm0[1] * Sw[3 + c] + jm0[2] * Sw[6 + c]; t1[c] = jm1[0] * Sw[c] + jm1[1] * Sw[3 + c] + jm1[2] * Sw[6 + c]; }
            const double s2 = o->sigma * o->sigma;
            const double R00 = (t0[0] * jm0[0] + t0[1] * jm0[1] + t0[2] * jm0[2]) + s2, R01 = t0[0] * jm1[0] + t0[1] * jm1[1] + t0[2] * jm1[2],
                         R11 = (t1[0] * jm1[0] + t1[1] * jm1[1] + t1[2] * jm1[2]) + s2;
            // S = H P_s H^T + R_k, every sum over the twelve columns ascending
            double S00 = 0., S01 = 0., S11 = 0.;
#pragma unroll
            for (int l = 0; l < LM_COLS; ++l) {
                double u0 = 0., u1 = 0.;
#pragma unroll
                for (int k = 0; k < LM_COLS; ++k) { u0 += h0[k] * Ps[k * LM_COLS + l]; u1 += h1[k] * Ps[k * LM_COLS + l]; }
                S00 += u0 * h0[l]; S01 += u0 * h1[l]; S11 += u1 * h1[l];
            }
            S00 = S00 + R00; S01 = S01 + R01; S11 = S11 + R11;
            // R_k = [a 0; b c] [a 0; b c]^T whitens; a Sigma_w so far above sigma^2 that rounding leaves R_k no positive pivot gates the observation
            const double wa = sqrt(R00), wb = R01 / wa, wc2 = R11 - wb * wb;
            st = 1;
            if (S00 > 0. && wc2 > 0.) {
                const double l00 = sqrt(S00), l10 = S01 / l00, d = S11 - l10 * l10;
                if (d > 0.) {
                    const double l11 = sqrt(d), y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11;
                    gamma = y0 * y0 + y1 * y1;
                    const double gate = job->gate;
                    if (!(gate > 0.) || gamma <= gate) st = 0;
                }
            }
            if (st == 0) {
                const double wc = sqrt(wc2);
#pragma unroll
                for (int c = 0; c < LM_COLS; ++c) { a0[c] = h0[c] / wa; a1[c] = (h1[c] - wb * a0[c]) / wc; }
                a0[LM_COLS] = r0 / wa; a1[LM_COLS] = (r1 - wb * a0[LM_COLS]) / wc;
            }
        }
        status_out[t] = st; gamma_out[t] = gamma;
    }
    // the compact index of every used observation, and the three counts
    const unsigned long long bu = __ballot(st == 0), bg = __ballot(st == 1), bb = __ballot(st == 2);
    if (lane == 0) { cnt[wave][0] = __popcll(bu); cnt[wave][1] = __popcll(bg); cnt[wave][2] = __popcll(bb); }
    __syncthreads();
    int base = 0, n_used = 0, n_gated = 0, n_behind = 0;
    for (int w = 0; w < nw; ++w) { if (w < wave) base += cnt[w][0]; n_used += cnt[w][0]; n_gated += cnt[w][1]; n_behind += cnt[w][2]; }
    const int ci = base + __popcll(bu & ((1ull << lane) - 1ull));
    if (t == 0) { sys[1] = 0.; sys[2] = 0.; sys[3] = 0.; info[3] = (double)n_used; info[4] = (double)n_gated; info[5] = (double)n_behind; info[7] = 0.; }
    double* Hc = sys + LM_HDR;
    if (n_used <= LM_ROWS / 2) {                        // (uniform over the workgroup)
        if (st == 0) {
#pragma unroll
            for (int k = 0; k < LM_W; ++k) { Hc[(2 * ci) * LM_W + k] = a0[k]; Hc[(2 * ci + 1) * LM_W + k] = a1[k]; }
        }
        if (t == 0) { sys[0] = (double)(2 * n_used); info[6] = (double)(2 * n_used); }
        return;
    }
    if (st == 0) {
#pragma unroll
        for (int k = 0; k < LM_W; ++k) { rows[(size_t)ci * 2 * LM_W + k] = a0[k]; rows[(size_t)ci * 2 * LM_W + LM_W + k] = a1[k]; }
    }
    __syncthreads();                                    // (orders the workgroup's global stores before its loads as well)
#pragma unroll
    for (int k = 0; k < LM_W; ++k) { a0[k] = t < n_used ? rows[(size_t)t * 2 * LM_W + k] : 0.; a1[k] = t < n_used ? rows[(size_t)t * 2 * LM_W + LM_W + k] : 0.; }
    // the squared norm every column starts with, summed as every inner product below
#pragma unroll
    for (int k = 0; k < LM_COLS; ++k) {
        const double part = wave_sum_f64(a0[k] * a0[k] + a1[k] * a1[k]);
        if (lane == 0) c0w[wave][k] = part;
    }
    __syncthreads();
    if (t < LM_COLS) { double s = 0.; for (int w = 0; w < nw; ++w) s += c0w[w][t]; c0[t] = s; }
    __syncthreads();
    int m = 0;                                          // rows so far (uniform over the workgroup)
#pragma unroll
    for (int j = 0; j < LM_COLS; ++j) {
        double tot[LM_W];
#pragma unroll
        for (int k = j; k < LM_W; ++k) {
            const double part = wave_sum_f64(a0[j] * a0[k] + a1[j] * a1[k]);
            if (lane == 0) red[j & 1][wave][k] = part;
        }
        __syncthreads();                                // (one per reflection: red is double-buffered)
#pragma unroll
        for (int k = j; k < LM_W; ++k) { double s = 0.; for (int w = 0; w < nw; ++w) s += red[j & 1][w][k]; tot[k] = s; }
        const double sig = tot[j];
        if (!(sig > LM_RANK_TOL2 * c0[j])) continue;    // depends on the columns before it (or is zero): no reflection, no row
        const double nrm = sqrt(sig);
#pragma unroll
        for (int k = j + 1; k < LM_W; ++k) {
            const double f = tot[k] / sig;
            a0[k] = a0[k] - f * a0[j]; a1[k] = a1[k] - f * a1[j];
        }
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < LM_W; ++k) Hc[m * LM_W + k] = k < j ? 0. : k == j ? nrm : tot[k] / nrm;
        }
        ++m;
    }
    if (t == 0) { sys[0] = (double)m; info[6] = (double)m; }
}

// Second launch, one wavefront per 64 columns of P, in the manner of k_fix_gain (be_fix.hip) with up to twelve rows and unit noise.
// Every workgroup reads the compressed system (m x 13) and gathers P_s, forms T_s = H P_s, S = T_s H^T + I (upper triangle, mirrored),
// S = L L^T, y = L^-1 r, gamma = y^T y by itself - the same operands in the same order everywhere - lane 0 factoring.  Status: 1 when
// m = 0 (nothing was used), 2 when a pivot is not > 0, else 0.  Then lane l takes column j = 64 blockIdx.x + l:
//   t_i = sum_k H[i][k] P[cols[k]][j] (k ascending),   w_i = (t_i - sum_{k<i} L[i][k] w_k) / L[i][i],   dx_j = sum_i w_i y_i,
// W (m x n) going to the work space the third launch reads.  A status other than 0 writes dx = 0 and no W, and reads no more of P.
// info: workgroup 0 writes [0] status [1] gamma [2] the smallest pivot.
__global__ __launch_bounds__(64) void k_lm_gain(const double* __restrict__ P, int ld, int n, int clone_col, const double* __restrict__ sys, double* __restrict__ W,
                                                double* __restrict__ dx, double* __restrict__ info)
{
    __shared__ double Hs[LM_ROWS * LM_COLS], rs[LM_ROWS], Ps[LM_COLS * LM_COLS], Ts[LM_ROWS * LM_COLS], S[LM_ROWS * LM_ROWS], Ls[LM_ROWS * LM_ROWS], y[LM_ROWS];
    __shared__ int status_s;
    const int lane = threadIdx.x, m = (int)sys[0];
    const int j = blockIdx.x * 64 + lane;
    if (m == 0) {                                       // (uniform over the grid)
        if (blockIdx.x == 0 && lane == 0) { info[0] = 1.; info[1] = 0.; info[2] = 0.; }
        if (j < n) dx[j] = 0.;
        return;
    }
    const double* Hc = sys + LM_HDR;
    for (int t = lane; t < m * LM_COLS; t += 64) Hs[t] = Hc[(t / LM_COLS) * LM_W + t % LM_COLS];
    if (lane < m) rs[lane] = Hc[lane * LM_W + LM_COLS];
    for (int t = lane; t < LM_COLS * LM_COLS; t += 64) Ps[t] = P[(size_t)lm_col(t / LM_COLS, clone_col) * ld + lm_col(t % LM_COLS, clone_col)];
    __syncthreads();
    for (int t = lane; t < m * LM_COLS; t += 64) {
        const int i = t / LM_COLS, l = t % LM_COLS;
        double s = 0.;
        for (int k = 0; k < LM_COLS; ++k) s += Hs[i * LM_COLS + k] * Ps[k * LM_COLS + l];
        Ts[t] = s;
    }
    __syncthreads();
    for (int t = lane; t < m * m; t += 64) {
        const int i = t / m, c = t % m;
        if (i <= c) {
            double s = 0.;
            for (int l = 0; l < LM_COLS; ++l) s += Ts[i * LM_COLS + l] * Hs[c * LM_COLS + l];
            if (i == c) s = s + 1.;
            S[i * m + c] = s; S[c * m + i] = s;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int status = 0;
        double pmin = 0., gamma = 0.;
        for (int c = 0; c < m; ++c) {
            double d = S[c * m + c];
            for (int k = 0; k < c; ++k) d -= Ls[c * m + k] * Ls[c * m + k];
            if (!(d > 0.)) { status = 2; pmin = d; break; }              // (a NaN lands here too)
            if (c == 0 || d < pmin) pmin = d;
            const double lcc = sqrt(d);
            Ls[c * m + c] = lcc;
            for (int i = c + 1; i < m; ++i) {
                double s = S[i * m + c];
                for (int k = 0; k < c; ++k) s -= Ls[i * m + k] * Ls[c * m + k];
                Ls[i * m + c] = s / lcc;
            }
        }
        if (status == 0) {
            for (int i = 0; i < m; ++i) {
                double s = rs[i];
                for (int k = 0; k < i; ++k) s -= Ls[i * m + k] * y[k];
                y[i] = s / Ls[i * m + i];
            }
            for (int i = 0; i < m; ++i) gamma += y[i] * y[i];
        }
        status_s = status;
        if (blockIdx.x == 0) { info[0] = (double)status; info[1] = gamma; info[2] = pmin; }
    }
    __syncthreads();
    if (j >= n) return;
    if (status_s != 0) { dx[j] = 0.; return; }
    double p[LM_COLS], w[LM_ROWS];
#pragma unroll
    for (int k = 0; k < LM_COLS; ++k) p[k] = P[(size_t)lm_col(k, clone_col) * ld + j];
    double d = 0.;
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) {
        if (i < m) {
            double s = 0.;
#pragma unroll
            for (int k = 0; k < LM_COLS; ++k) s += Hs[i * LM_COLS + k] * p[k];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= Ls[i * m + k] * w[k];
            w[i] = s / Ls[i * m + i];
            W[(size_t)i * n + j] = w[i];
            d += w[i] * y[i];
        }
    }
    dx[j] = d;
}

// Third launch: P[a][b] <- P[a][b] - sum_i W[i][a] W[i][b] (i ascending), one entry per thread and four rows per thread; (a, b) and
// (b, a) multiply the same pairs in the same order.  Nothing happens unless the second launch reported status 0.
__global__ __launch_bounds__(256) void k_lm_downdate(double* __restrict__ P, int ld, int n, const double* __restrict__ sys, const double* __restrict__ W, const double* __restrict__ info)
{
    if (info[0] != 0.) return;                          // (uniform over the grid)
    const int m = (int)sys[0];
    const int b = blockIdx.x * 64 + threadIdx.x, a0 = (blockIdx.y * 4 + threadIdx.y) * 4;
    if (b >= n) return;
    double wb[LM_ROWS];
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) wb[i] = i < m ? W[(size_t)i * n + b] : 0.;
    for (int q = 0; q < 4; ++q) {
        const int a = a0 + q;
        if (a >= n) return;
        double s = 0.;
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) if (i < m) s += W[(size_t)i * n + a] * wb[i];
        P[(size_t)a * ld + b] = P[(size_t)a * ld + b] - s;
    }
}

// the upper triangle of a 3 x 3 matrix, mirrored: positive semi-definite?  Every principal minor >= 0, each against the rounding of its
// own terms (a covariance of rank 1 or 2 written down in double precision has minors a few units in the last place either side of 0)
static bool psd3_upper(const double* c)
{
    const double a = c[0], b = c[4], d = c[8], ab = c[1], ad = c[2], bd = c[5];
    const double eps = 64 * 2.220446049250313e-16;
    if (!(a >= 0. && b >= 0. && d >= 0.)) return false;
    if (!(a * b - ab * ab >= -eps * a * b) || !(a * d - ad * ad >= -eps * a * d) || !(b * d - bd * bd >= -eps * b * d)) return false;
    const double det = a * (b * d - bd * bd) - ab * (ab * d - bd * ad) + ad * (ab * bd - b * ad);
    return det >= -eps * a * b * d;
}
// what the kernels assume of one observation
static const char* landmark_obs_flaw(const lvk_landmark_obs* o)
{
    for (int k = 0; k < 3; ++k) if (!std::isfinite(o->p_w[k])) return "p_w is not finite";
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) if (!std::isfinite(o->cov_w[i * 3 + j])) return "cov_w is not finite";
    if (!std::isfinite(o->uv[0]) || !std::isfinite(o->uv[1])) return "uv is not finite";
    if (!std::isfinite(o->sigma) || !(o->sigma > 0.)) return "sigma is not a finite number > 0";
    if (!psd3_upper(o->cov_w)) return "the upper triangle of cov_w is not positive semi-definite";
    return nullptr;
}
static const char* landmark_job_flaw(const lvk_landmark_fix_job* j, int n)
{
    if (j->clone_col < 21 || j->clone_col + 6 > n) return "clone_col is below 21 or its six columns leave [0, n)";
    bool finite = std::isfinite(j->gate) && std::isfinite(j->min_depth);
    for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(j->q_b[k]);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(j->p_b[k]) && std::isfinite(j->t_c_b[k]);
    for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(j->R_b2c[k]);
    if (!finite) return "a value of the job is not finite";
    if (!(fabs(sqrt(j->q_b[0] * j->q_b[0] + j->q_b[1] * j->q_b[1] + j->q_b[2] * j->q_b[2] + j->q_b[3] * j->q_b[3]) - 1.0) <= 1e-6)) return "q_b is not a unit quaternion";
    if (j->min_depth < 0.) return "min_depth is negative";
    return nullptr;
}

// (C ABI) job and observations go up in the stage's input blob, the compact rows, the system and W live in its work space, dx and the
// reports come back through its output blob; the three launches are queued at once and the call waits once
extern "C" lvk_status lvk_ekf_update_landmarks(lvk_context* ctx, double* d_P, int ldp, int n, const lvk_landmark_fix_job* h_job, const lvk_landmark_obs* h_obs, int n_obs,
                                               double* h_dx, double* h_info8, int* h_status, double* h_gamma)
{
    if (!ctx || !d_P || !h_job || (!h_obs && n_obs > 0) || !h_dx || !h_info8 || !h_status || !h_gamma || n <= 0 || ldp < n || n_obs < 0)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_update_landmarks: bad argument");
    if (n_obs > LM_MAX_OBS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_ekf_update_landmarks: %d observations (at most %d per batch)", n_obs, LM_MAX_OBS);
    if (const char* flaw = landmark_job_flaw(h_job, n)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_update_landmarks: %s (clone_col %d, n %d)", flaw, h_job->clone_col, n);
    for (int k = 0; k < n_obs; ++k)
        if (const char* flaw = landmark_obs_flaw(h_obs + k)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_update_landmarks: observation %d: %s", k, flaw);
    if (n_obs == 0) return LVK_OK;
    const size_t dxb = sizeof(double) * (size_t)n, ob = sizeof(lvk_landmark_obs) * (size_t)n_obs;
    Stage sg(ctx);
    const size_t o_job = sg.take(Stage::IN, sizeof *h_job), o_obs = sg.take(Stage::IN, ob);
    const size_t o_rows = sg.take(Stage::MID, sizeof(double) * 2 * LM_W * (size_t)n_obs), o_sys = sg.take(Stage::MID, sizeof(double) * (LM_HDR + LM_ROWS * LM_W)),
                 o_w = sg.take(Stage::MID, sizeof(double) * LM_ROWS * (size_t)n);
    const size_t o_dx = sg.take(Stage::OUT, dxb), o_info = sg.take(Stage::OUT, 8 * sizeof(double)), o_st = sg.take(Stage::OUT, sizeof(int) * (size_t)n_obs),
                 o_g = sg.take(Stage::OUT, sizeof(double) * (size_t)n_obs);
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_job, h_job, sizeof *h_job));
    LVK_TRY(sg.put(Stage::IN, o_obs, h_obs, ob));
    double* sys = sg.at<double>(Stage::MID, o_sys); double* W = sg.at<double>(Stage::MID, o_w); double* info = sg.at<double>(Stage::OUT, o_info);
    hipLaunchKernelGGL(n_obs <= 256 ? k_lm_rows<256> : k_lm_rows<LM_MAX_OBS>, dim3(1), dim3((n_obs + 63) / 64 * 64), 0, ctx->stream, d_P, ldp, sg.at<lvk_landmark_fix_job>(Stage::IN, o_job),
                       sg.at<lvk_landmark_obs>(Stage::IN, o_obs), n_obs, sg.at<double>(Stage::MID, o_rows), sys, sg.at<int>(Stage::OUT, o_st), sg.at<double>(Stage::OUT, o_g), info);
    LVK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_lm_gain, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_P, ldp, n, h_job->clone_col, sys, W, sg.at<double>(Stage::OUT, o_dx), info);
    LVK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_lm_downdate, dim3((n + 63) / 64, (n + 15) / 16), dim3(64, 4), 0, ctx->stream, d_P, ldp, n, sys, W, info);
    LVK_LAUNCH_CHECK(ctx);
    LVK_TRY(sg.get(h_dx, Stage::OUT, o_dx, dxb));
    LVK_TRY(sg.get(h_info8, Stage::OUT, o_info, 8 * sizeof(double)));
    LVK_TRY(sg.get(h_status, Stage::OUT, o_st, sizeof(int) * (size_t)n_obs));
    LVK_TRY(sg.get(h_gamma, Stage::OUT, o_g, sizeof(double) * (size_t)n_obs));
    return sg.wait();
}

// ------------------------------------------------------------------------- the filter's batch queue
static void landmark_report(lvk_ekf* e, const lvk_ekf::LmBatch& b, int status, long long clone_id, const double* info)
{
    lvk_landmark_report r; memset(&r, 0, sizeof r);
    r.tag = b.tag; r.status = status; r.clone_id = clone_id; r.n_obs = (int)b.obs.size();
    if (info) { r.n_used = (int)info[3]; r.n_gated = (int)info[4]; r.n_behind = (int)info[5]; r.gamma = status == LVK_LANDMARKS_APPLIED ? info[1] : 0.0; }
    drain_append(e->lm_reports, r);
    e->lm_stats[1 + status]++;
    e->lm_stats[7] += r.n_obs; e->lm_stats[8] += r.n_used; e->lm_stats[9] += r.n_gated; e->lm_stats[10] += r.n_behind;
}
// The queue, in order: every batch whose clone can be named is consumed - applied through lvk_ekf_update_landmarks and the injection,
// or reported with the reason it was not - and one that is newer than the newest clone waits for a later message.
lvk_status lvk_ekf_apply_landmarks(lvk_ekf* e)
{
    std::vector<lvk_ekf::LmBatch> waiting;
    std::vector<double> dx, gamma; std::vector<int> status;
    for (lvk_ekf::LmBatch& b : e->lm_queue) {
        const int nc = (int)e->clones.size();
        int i = -1, miss = -1;
        if (nc == 0) { waiting.push_back(std::move(b)); continue; }
        if (b.clone_id >= 0) { i = clone_rank(e, b.clone_id); if (i < 0) miss = LVK_LANDMARKS_STALE; }
        else if (b.time < e->clones.front().time) miss = LVK_LANDMARKS_STALE;
        else if (b.time > e->clones.back().time) { waiting.push_back(std::move(b)); continue; }
        else {
            for (int k = 0; k < nc && i < 0; ++k) if (e->clones[(size_t)k].time == b.time) i = k;
            if (i < 0) miss = LVK_LANDMARKS_NO_CLONE;
        }
        if (miss >= 0) { landmark_report(e, b, miss, -1, nullptr); continue; }
        const Clone& c = e->clones[(size_t)i];
        double info[8] = {(double)LVK_LANDMARKS_ALL_REJECTED, 0, 0, 0, 0, 0, 0, 0};
        if (!b.obs.empty()) {                           // (an empty batch launches nothing)
            lvk_landmark_fix_job job; memset(&job, 0, sizeof job);
            job.clone_col = e->leg + 6 * i;
            memcpy(job.q_b, c.q, 32); memcpy(job.p_b, c.p, 24); memcpy(job.R_b2c, e->R_b2c, 72); memcpy(job.t_c_b, e->t_c_b, 24);
            job.gate = e->lm_gate_scale > 0 ? e->lm_gate_scale * lvk_chi2_005(2) : 0.0; job.min_depth = e->lm_min_depth;
            const int no = (int)b.obs.size();
            dx.assign((size_t)e->N, 0.0); status.assign((size_t)no, 0); gamma.assign((size_t)no, 0.0);
            const lvk_status st = lvk_ekf_update_landmarks(e->ctx, e->dP[e->cur], e->ld, e->N, &job, b.obs.data(), no, dx.data(), info, status.data(), gamma.data());
            if (st != LVK_OK) {                         // keep what waits and what was not reached; this batch is dropped
                for (lvk_ekf::LmBatch* q = &b + 1; q != e->lm_queue.data() + e->lm_queue.size(); ++q) waiting.push_back(std::move(*q));
                e->lm_queue.swap(waiting);
                return st;
            }
            e->n_sync++;
            if ((int)info[0] == LVK_LANDMARKS_APPLIED) { lvk_ekf_inject(e, dx.data()); e->p00_valid = false; }
        }
        landmark_report(e, b, (int)info[0], c.id, info);
    }
    e->lm_queue.swap(waiting);
    return LVK_OK;
}

extern "C" {

lvk_status lvk_ekf_add_landmark_obs(lvk_ekf* e, int64_t tag, int64_t clone_id, double time, const lvk_landmark_obs* obs, int n_obs)
{
    if (!e || n_obs < 0 || (n_obs > 0 && !obs)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_add_landmark_obs: bad argument");
    // "pending" as for lvk_ekf_add_fix: the update consumes the queue as it was when it was issued
    if (e->async && e->async->unwaited) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_landmark_obs: an update is in flight (lvk_ekf_wait first)");
    ekf_quiesce(e);
    if (e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_add_landmark_obs: the sharded update does not apply landmark observations (lvk_ekf_set_shard is set)");
    if (clone_id < -1) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_landmark_obs: clone_id %lld", (long long)clone_id);
    if (!std::isfinite(time)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_landmark_obs: time is not finite");
    if (n_obs > LM_MAX_OBS) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "lvk_ekf_add_landmark_obs: %d observations (at most %d per batch)", n_obs, LM_MAX_OBS);
    for (int k = 0; k < n_obs; ++k)
        if (const char* flaw = landmark_obs_flaw(obs + k)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_landmark_obs: observation %d: %s", k, flaw);
    if (e->lm_queue.size() >= (size_t)lvk_ekf::LM_CAP) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "lvk_ekf_add_landmark_obs: %d batches wait already", (int)lvk_ekf::LM_CAP);
    lvk_ekf::LmBatch b; b.tag = tag; b.clone_id = clone_id; b.time = time; b.obs.assign(obs, obs + n_obs);
    e->lm_queue.push_back(std::move(b));
    e->lm_stats[0]++;
    return LVK_OK;
}
lvk_status lvk_ekf_set_landmark_options(lvk_ekf* e, double gate_scale, double min_depth)
{
    if (!e || std::isnan(gate_scale) || !(min_depth >= 0.0) || !std::isfinite(min_depth)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_landmark_options: bad argument");
    ekf_quiesce(e);
    e->lm_gate_scale = gate_scale; e->lm_min_depth = min_depth;
    return LVK_OK;
}
int lvk_ekf_take_landmark_reports(lvk_ekf* e, lvk_landmark_report* out, int cap)
{
    if (!e || !out || cap <= 0) return 0;
    ekf_quiesce(e);
    const int n = std::min((int)e->lm_reports.size(), cap);
    std::copy(e->lm_reports.begin(), e->lm_reports.begin() + n, out);
    e->lm_reports.erase(e->lm_reports.begin(), e->lm_reports.begin() + n);
    return n;
}
void lvk_ekf_landmark_stats(const lvk_ekf* e, long* out12)
{
    if (!e || !out12) return;
    ekf_quiesce(e);
    memcpy(out12, e->lm_stats, sizeof e->lm_stats);
    out12[6] = (long)e->lm_queue.size();
}

}  // extern "C"
