// fe_align.hip — relocalisation against a prior map for gfx950 (wave64): the yaw and translation that take the map's frame into the
// filter's world frame, from up to 1024 putative 2D-3D matches, by two-point RANSAC.  No reference counterpart.  include/lvk_c.h states
// the definition (lvk_align_ransac_2pt); every expression here is written in the order stated there, FP64, no contraction.
//   k_align_hypotheses     one wavefront per pair, four pairs per workgroup.  The workgroup stages the matches in LDS once (40 bytes each,
//                          40 KB at the 1024-match cap: inside the default 64 KB); every lane solves the pair's quadratic (the same
//                          values on all 64 lanes, so the model is in registers everywhere and nothing is broadcast), then the wavefront
//                          scores the pair's one or two models over the matches 64 at a time; lane k reads match k with 8-byte LDS reads
//                          40 bytes apart, which are conflict free inside a 32-lane half.  wave_sum_i32 gives the counts, lane 0 writes
//                          the hypothesis record.
//   k_align_select_refine  one workgroup of four wavefronts.  The arg-max over the records with the integer key
//                          count << 13 | (8191 - (2 hypothesis + slot)): the largest key is the largest count, then the lowest hypothesis,
//                          then the lower root.  The winner's inlier test again for the mask (the same device function on the same
//                          operands: the same bits), then Gauss-Newton on (yaw, t) over the inliers: every thread sums its matches
//                          tid, tid + 256, .. in that order, wave_sum_f64 adds the lanes, the four wavefront sums are added in order -
//                          one fixed shape whatever n is.  The 4 x 4 solve is done by every thread on the same sums.
// Neither kernel overwrites anything a sibling workgroup reads: the hypotheses kernel writes its own records only, the second launch is
// one workgroup.
#include "lvk_internal.h"
#include "fe_track_dev.h"
#include "lvk_wave.h"
#include <math.h>

#define ALIGN_MAX_N      1024
#define ALIGN_MAX_PAIRS  4096
#define ALIGN_WAVES      4                  // pairs per workgroup
#define ALIGN_THREADS    (64 * ALIGN_WAVES)
#define ALIGN_STEP_TOL2  1e-20              // the refinement stops behind a step with dpsi^2 + |dt|^2 <= this
#define ALIGN_PIVOT_REL  1e-12              // a Cholesky pivot at or below this share of its diagonal entry counts as non-positive

struct AlignCam { double R[9], p[3]; };                           // R_wc row-major, p_wc
struct AlignOpt { double thresh2, min_depth, min_dz; int min_inliers, max_iters; };

// p_c = R_wc^T (Rz X + t - p_wc) of the match at m (X, Y, Z, u, v); q0, q1 = the xy of Rz X
__device__ __forceinline__ void align_cam_point(const AlignCam& cam, double c, double s, const double* t, const double* m, double& q0, double& q1, double& x, double& y,
                                                double& z)
{
    q0 = c * m[0] - s * m[1]; q1 = s * m[0] + c * m[1];
    const double g0 = (q0 + t[0]) - cam.p[0], g1 = (q1 + t[1]) - cam.p[1], g2 = (m[2] + t[2]) - cam.p[2];
    x = (cam.R[0] * g0 + cam.R[3] * g1) + cam.R[6] * g2;
    y = (cam.R[1] * g0 + cam.R[4] * g1) + cam.R[7] * g2;
    z = (cam.R[2] * g0 + cam.R[5] * g1) + cam.R[8] * g2;
}
__device__ __forceinline__ int align_inlier(const AlignCam& cam, double c, double s, const double* t, const double* m, double thresh2, double min_depth)
{
    double q0, q1, x, y, z;
    align_cam_point(cam, c, s, t, m, q0, q1, x, y, z);
    if (!(z > min_depth)) return 0;
    const double rx = x / z - m[3], ry = y / z - m[4];
    return rx * rx + ry * ry <= thresh2 ? 1 : 0;
}

// the minimal solver: the models of pair (i, j), lower root first.  sm: the matches, 5 doubles each
__device__ __forceinline__ int align_solve(const double* sm, int n, int i, int j, const AlignCam& cam, double min_dz, lvk_align_model* md)
{
    if (i == j || i < 0 || j < 0 || i >= n || j >= n) return 0;
    const double* mi = sm + 5 * i; const double* mj = sm + 5 * j;
    double di[3], dj[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        di[r] = (cam.R[3 * r] * mi[3] + cam.R[3 * r + 1] * mi[4]) + cam.R[3 * r + 2];
        dj[r] = (cam.R[3 * r] * mj[3] + cam.R[3 * r + 1] * mj[4]) + cam.R[3 * r + 2];
    }
    const double ax = mi[0] - mj[0], ay = mi[1] - mj[1], az = mi[2] - mj[2];
    const double rho2 = ax * ax + ay * ay;
    if (!(rho2 > 0.)) return 0;
    const bool pi = fabs(di[2]) >= fabs(dj[2]);                 // divide by the bearing with the larger |d_z|: lambda_p = alpha + beta lambda_q
    if (!((pi ? fabs(di[2]) : fabs(dj[2])) >= min_dz)) return 0;
    double alpha, beta, e0, e1, f0, f1;
    if (pi) {
        alpha = az / di[2]; beta = dj[2] / di[2];
        e0 = alpha * di[0]; e1 = alpha * di[1]; f0 = beta * di[0] - dj[0]; f1 = beta * di[1] - dj[1];
    } else {
        alpha = -az / dj[2]; beta = di[2] / dj[2];
        e0 = -alpha * dj[0]; e1 = -alpha * dj[1]; f0 = di[0] - beta * dj[0]; f1 = di[1] - beta * dj[1];
    }
    const double A = f0 * f0 + f1 * f1, B = e0 * f0 + e1 * f1, C = (e0 * e0 + e1 * e1) - rho2;
    if (!(A > 0.)) return 0;
    const double disc = B * B - A * C;
    if (!(disc >= 0.)) return 0;
    const double sq = sqrt(disc);
    int nm = 0;
#pragma unroll
    for (int root = 0; root < 2; ++root) {
        const double mu = (root == 0 ? -B - sq : -B + sq) / A;
        const double lp = alpha + beta * mu;
        if (!(mu > 0. && lp > 0.)) continue;
        const double li = pi ? lp : mu;
        const double w0 = e0 + mu * f0, w1 = e1 + mu * f1;   // = Rz (X_i - X_j), xy
        const double dot = ax * w0 + ay * w1, crs = ax * w1 - ay * w0;
        const double nrm = sqrt(dot * dot + crs * crs);
        if (!(nrm > 0.)) continue;
        lvk_align_model& o = md[nm++];
        o.count = 0; o.root = root;
        o.c = dot / nrm; o.s = crs / nrm;
        o.t[0] = (cam.p[0] + li * di[0]) - (o.c * mi[0] - o.s * mi[1]);
        o.t[1] = (cam.p[1] + li * di[1]) - (o.s * mi[0] + o.c * mi[1]);
        o.t[2] = (cam.p[2] + li * di[2]) - mi[2];
    }
    return nm;
}

__global__ void __launch_bounds__(ALIGN_THREADS) k_align_hypotheses(const double* __restrict__ m, int n, const lvk_align_pair* __restrict__ pairs, int n_pairs, AlignCam cam,
                                                                   AlignOpt opt, lvk_align_hyp* __restrict__ hyp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* sm = reinterpret_cast<double*>(s_raw);
    for (int i = threadIdx.x; i < 5 * n; i += ALIGN_THREADS) sm[i] = m[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * ALIGN_WAVES + (threadIdx.x >> 6);
    if (h >= n_pairs) return;
    const lvk_align_pair pr = pairs[h];
    lvk_align_hyp rec;
    memset(&rec, 0, sizeof rec);
    const int nm = __builtin_amdgcn_readfirstlane(align_solve(sm, n, pr.i, pr.j, cam, opt.min_dz, rec.m));      // the same on every lane
    rec.n_models = nm;
    for (int r = 0; r < nm; ++r) {
        int cnt = 0;
        for (int k = lane; k < n; k += 64) cnt += align_inlier(cam, rec.m[r].c, rec.m[r].s, rec.m[r].t, sm + 5 * k, opt.thresh2, opt.min_depth);
        rec.m[r].count = wave_sum_i32(cnt);
    }
    if (lane == 0) hyp[h] = rec;
}

#define ALIGN_NSUM 15                        // 10 entries of A's upper triangle, 4 of the gradient, the sum of squares
__global__ void __launch_bounds__(ALIGN_THREADS) k_align_select_refine(const double* __restrict__ m, int n, const lvk_align_pair* __restrict__ pairs,
                                                                      const lvk_align_hyp* __restrict__ hyp, int n_pairs, AlignCam cam, AlignOpt opt,
                                                                      uint8_t* __restrict__ mask, lvk_align_result* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* sm = reinterpret_cast<double*>(s_raw);
    __shared__ int s_key[ALIGN_WAVES];
    __shared__ double s_red[ALIGN_WAVES][ALIGN_NSUM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 5 * n; i += ALIGN_THREADS) sm[i] = m[i];
    int key = -1;
    for (int h = tid; h < n_pairs; h += ALIGN_THREADS) {
        const int nm = hyp[h].n_models;
        for (int r = 0; r < nm && r < 2; ++r) { const int k = (hyp[h].m[r].count << 13) | (8191 - (2 * h + r)); key = k > key ? k : key; }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) { const int o = __shfl_xor(key, x, 64); key = o > key ? o : key; }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = s_key[0];
#pragma unroll
    for (int w = 1; w < ALIGN_WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;

    lvk_align_result res;
    memset(&res, 0, sizeof res);
    res.hyp = -1; res.root = -1; res.pair_i = -1; res.pair_j = -1; res.c = 1.; res.c0 = 1.;
    if (key < 0) {
        for (int k = tid; k < n; k += ALIGN_THREADS) mask[k] = 0;
        res.status = LVK_ALIGN_NO_MODEL;
        if (tid == 0) *out = res;
        return;
    }
    const int slot = 8191 - (key & 8191), wh = slot >> 1;
    const lvk_align_model win = hyp[wh].m[slot & 1];
    res.hyp = wh; res.root = win.root; res.pair_i = pairs[wh].i; res.pair_j = pairs[wh].j; res.n_inliers = win.count;
    res.c0 = win.c; res.s0 = win.s; res.c = win.c; res.s = win.s;
#pragma unroll
    for (int r = 0; r < 3; ++r) { res.t0[r] = win.t[r]; res.t[r] = win.t[r]; }
    unsigned in_bits = 0;                    // this thread's matches tid + 256 q, q < 4
#pragma unroll
    for (int q = 0; q < ALIGN_MAX_N / ALIGN_THREADS; ++q) {
        const int k = tid + ALIGN_THREADS * q;
        if (k < n) {
            const int in = align_inlier(cam, win.c, win.s, win.t, sm + 5 * k, opt.thresh2, opt.min_depth);
            mask[k] = (uint8_t)in; in_bits |= (unsigned)in << q;
        }
    }
    if (win.count < opt.min_inliers) {
        res.status = LVK_ALIGN_FEW_INLIERS;
        if (tid == 0) *out = res;
        return;
    }
    double c = win.c, s = win.s, t[3] = {win.t[0], win.t[1], win.t[2]};
    double A[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.}, ssq = 0.;
    int iters = 0, status = LVK_ALIGN_OK;
    bool last = false;                       // the evaluation behind the final step: A and the rms of the model that is returned
    for (;;) {
        double acc[ALIGN_NSUM];
#pragma unroll
        for (int q = 0; q < ALIGN_NSUM; ++q) acc[q] = 0.;
#pragma unroll
        for (int q = 0; q < ALIGN_MAX_N / ALIGN_THREADS; ++q) {
            if (!((in_bits >> q) & 1u)) continue;
            const double* mk = sm + 5 * (tid + ALIGN_THREADS * q);
            double q0, q1, x, y, z;
            align_cam_point(cam, c, s, t, mk, q0, q1, x, y, z);
            const double iz = 1. / z, a = x * iz, b = y * iz;
            const double rx = a - mk[3], ry = b - mk[4];
            // d p_c / d psi = R_wc^T (-q1, q0, 0),  d p_c / d t_k = row k of R_wc
            const double dx[4] = {cam.R[3] * q0 - cam.R[0] * q1, cam.R[0], cam.R[3], cam.R[6]};
            const double dy[4] = {cam.R[4] * q0 - cam.R[1] * q1, cam.R[1], cam.R[4], cam.R[7]};
            const double dz[4] = {cam.R[5] * q0 - cam.R[2] * q1, cam.R[2], cam.R[5], cam.R[8]};
            double jx[4], jy[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) { jx[p] = (dx[p] - a * dz[p]) * iz; jy[p] = (dy[p] - b * dz[p]) * iz; }
            int e = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int r = p; r < 4; ++r) acc[e++] += jx[p] * jx[r] + jy[p] * jy[r];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[10 + p] += jx[p] * rx + jy[p] * ry;
            acc[14] += rx * rx + ry * ry;
        }
        __syncthreads();                     // the previous round's sums have been read (and, first round, the matches are staged)
#pragma unroll
        for (int q = 0; q < ALIGN_NSUM; ++q) { const double v = wave_sum_f64(acc[q]); if (lane == 0) s_red[wave][q] = v; }
        __syncthreads();
        double g[4];
#pragma unroll
        for (int q = 0; q < ALIGN_NSUM; ++q) {
            const double v = ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
            if (q < 10) A[q] = v; else if (q < 14) g[q - 10] = v; else ssq = v;
        }
        if (last || iters >= opt.max_iters) break;
        // A = L L^T (upper triangle stored by rows: 00 01 02 03 11 12 13 22 23 33), then L L^T d = -g
        const double a00 = A[0], a01 = A[1], a02 = A[2], a03 = A[3], a11 = A[4], a12 = A[5], a13 = A[6], a22 = A[7], a23 = A[8], a33 = A[9];
        bool pd = a00 > 0.;
        const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00, l30 = a03 / l00;
        const double p1 = a11 - l10 * l10;
        pd = pd && p1 > ALIGN_PIVOT_REL * a11;
        const double l11 = sqrt(p1), l21 = (a12 - l20 * l10) / l11, l31 = (a13 - l30 * l10) / l11;
        const double p2 = (a22 - l20 * l20) - l21 * l21;
        pd = pd && p2 > ALIGN_PIVOT_REL * a22;
        const double l22 = sqrt(p2), l32 = ((a23 - l30 * l20) - l31 * l21) / l22;
        const double p3 = ((a33 - l30 * l30) - l31 * l31) - l32 * l32;
        pd = pd && p3 > ALIGN_PIVOT_REL * a33;
        if (!pd) { status = LVK_ALIGN_SINGULAR; break; }
        const double l33 = sqrt(p3);
        const double y0 = -g[0] / l00, y1 = (-g[1] - l10 * y0) / l11, y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22, y3 = (((-g[3] - l30 * y0) - l31 * y1) - l32 * y2) / l33;
        const double d3 = y3 / l33, d2 = (y2 - l32 * d3) / l22, d1 = ((y1 - l21 * d2) - l31 * d3) / l11, d0 = (((y0 - l10 * d1) - l20 * d2) - l30 * d3) / l00;
        // yaw by the half-angle form: a rotation by 2 atan(d0 / 2), exact in (c, s) and free of libm
        const double hh = 0.5 * d0, h2 = hh * hh, den = 1. + h2, cd = (1. - h2) / den, sd = (hh + hh) / den;
        const double cn = c * cd - s * sd, sn = s * cd + c * sd;
        c = cn; s = sn; t[0] += d1; t[1] += d2; t[2] += d3;
        ++iters;
        last = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3 <= ALIGN_STEP_TOL2;
    }
    res.status = status; res.iters = iters;
    if (status == LVK_ALIGN_OK) { res.c = c; res.s = s; res.t[0] = t[0]; res.t[1] = t[1]; res.t[2] = t[2]; }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int lo = p < r ? p : r, hi = p < r ? r : p; res.A[4 * p + r] = A[4 * lo - lo * (lo - 1) / 2 + (hi - lo)]; }
    res.rms = sqrt(ssq / (double)win.count);
    if (tid == 0) *out = res;
}

static bool align_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// the options with their defaults filled in and their ranges checked; false: *why names the field
static bool align_options(const lvk_align_options* opt, AlignOpt* o, const char** why)
{
    lvk_align_options a = {0., 0., 0., 0, 0};
    if (opt) a = *opt;
    if (a.thresh == 0.) a.thresh = 0.01;
    if (a.min_depth == 0.) a.min_depth = 0.1;
    if (a.min_dz == 0.) a.min_dz = 1e-6;
    if (a.min_inliers == 0) a.min_inliers = 6;
    if (a.max_refine_iters == 0) a.max_refine_iters = 10;
    if (!(std::isfinite(a.thresh) && a.thresh > 0.)) { *why = "thresh must be positive and finite"; return false; }
    if (!(std::isfinite(a.min_depth) && a.min_depth > 0.)) { *why = "min_depth must be positive and finite"; return false; }
    if (!(std::isfinite(a.min_dz) && a.min_dz > 0.)) { *why = "min_dz must be positive and finite"; return false; }
    if (a.min_inliers < 2 || a.min_inliers > ALIGN_MAX_N) { *why = "min_inliers outside 2..1024"; return false; }
    if (a.max_refine_iters < 1 || a.max_refine_iters > 100) { *why = "max_refine_iters outside 1..100"; return false; }
    o->thresh2 = a.thresh * a.thresh; o->min_depth = a.min_depth; o->min_dz = a.min_dz; o->min_inliers = a.min_inliers; o->max_iters = a.max_refine_iters;
    return true;
}

extern "C" lvk_status lvk_align_ransac_2pt(lvk_context* ctx, const lvk_align_match* d_m, int n, const lvk_align_pair* d_pairs, int n_pairs, const double* R_wc,
                                           const double* p_wc, const lvk_align_options* opt, lvk_align_hyp* d_hyp, uint8_t* d_mask, lvk_align_result* d_out)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n < 0 || n_pairs < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_2pt: negative count (n %d, n_pairs %d)", n, n_pairs);
    if (!R_wc || !p_wc || !d_out || (n > 0 && (!d_m || !d_mask)) || (n_pairs > 0 && !d_pairs)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_2pt: null pointer");
    AlignOpt o; const char* why = "";
    if (!align_options(opt, &o, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_2pt: %s", why);
    if (!align_finite(R_wc, 9) || !align_finite(p_wc, 3)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_2pt: R_wc or p_wc is not finite");
    if (n > ALIGN_MAX_N) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_align_ransac_2pt: %d matches, at most %d (they are staged in LDS)", n, ALIGN_MAX_N);
    if (n_pairs > ALIGN_MAX_PAIRS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_align_ransac_2pt: %d pairs, at most %d", n_pairs, ALIGN_MAX_PAIRS);
    AlignCam cam;
    memcpy(cam.R, R_wc, sizeof cam.R); memcpy(cam.p, p_wc, sizeof cam.p);
    const int np = n < 2 ? 0 : n_pairs;                    // fewer than two matches: no pair can give a model, none is looked at
    lvk_align_hyp* hyp = d_hyp;
    if (np > 0 && !hyp) {
        hyp = (lvk_align_hyp*)lvk_ctx_scratch(ctx, LVK_SCR_ALIGN_HYP, sizeof(lvk_align_hyp) * ALIGN_MAX_PAIRS);
        if (!hyp) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_align_ransac_2pt: scratch allocation failed");
    }
    const double* m = reinterpret_cast<const double*>(d_m);
    const size_t lds = sizeof(lvk_align_match) * (size_t)n;
    if (np > 0)
        hipLaunchKernelGGL(k_align_hypotheses, dim3((np + ALIGN_WAVES - 1) / ALIGN_WAVES), dim3(ALIGN_THREADS), lds, ctx->stream, m, n, d_pairs, np, cam, o, hyp);
    hipLaunchKernelGGL(k_align_select_refine, dim3(1), dim3(ALIGN_THREADS), lds, ctx->stream, m, n, d_pairs, (const lvk_align_hyp*)hyp, np, cam, o, d_mask, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// the pairs lvk_frontend_align_landmarks tries (host only): every pair in lexicographic order when there are at most max_hypotheses of
// them, draws of the multiply-with-carry generator of the RANSAC stage (d_rng_next, fe_track_dev.h) otherwise
extern "C" int lvk_align_draw_pairs(int n, int max_hypotheses, uint32_t seed, lvk_align_pair* h_pairs)
{
    if (max_hypotheses == 0) max_hypotheses = ALIGN_MAX_PAIRS;
    if (n < 0 || max_hypotheses < 0 || max_hypotheses > ALIGN_MAX_PAIRS || !h_pairs) return -1;
    if (n < 2) return 0;
    const long long all = (long long)n * (n - 1) / 2;
    if (all <= max_hypotheses) {
        int k = 0;
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) { h_pairs[k].i = i; h_pairs[k].j = j; ++k; }
        return k;
    }
    unsigned long long state = seed ? (unsigned long long)seed : (unsigned long long)LVK_ALIGN_DEFAULT_SEED;
    auto next = [&state]() { state = (unsigned long long)(unsigned)state * 4164903690ULL + (unsigned)(state >> 32); return (unsigned)state; };
    for (int h = 0; h < max_hypotheses; ++h) {
        const int i = (int)(next() % (unsigned)n);
        int j = (int)(next() % (unsigned)(n - 1));
        j += j >= i;
        h_pairs[h].i = i; h_pairs[h].j = j;
    }
    return max_hypotheses;
}
