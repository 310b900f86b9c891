// fe_align3d.hip — a second session into the resident prior map, for gfx950 (wave64): the yaw and translation between two sessions' frames
// from up to 1024 putative 3D-3D matches by two-point RANSAC, and that alignment applied to a point set where it lies.  No reference
// counterpart.  include/lvk_c.h states the definitions (lvk_align_ransac_3d, lvk_map_transform, lvk_align_invert); every expression here is
// written in the order stated there, FP64, no contraction.
//   k_align3d_hypotheses     one wavefront per pair, four pairs per workgroup.  The workgroup stages the matches in LDS once (48 bytes each,
//                            48 KB at the 1024-match cap: inside the default 64 KB); every lane solves the pair (the same values on all 64
//                            lanes, so the model is in registers everywhere and nothing is broadcast), then the wavefront scores it over
//                            the matches 64 at a time.  The count is the popcount of the wavefront's ballot, added up on the scalar side.
//   k_align3d_select_refine  one workgroup of four wavefronts.  The arg-max over the records with the integer key
//                            count << 12 | (4095 - hypothesis): the largest key is the largest count, then the lowest hypothesis.  The
//                            winner's inlier test again for the mask (the same device function on the same operands: the same bits), then
//                            the closed form in three sweeps over the inliers - centroids; D, C, W; A and the residual -: every thread sums
//                            its matches tid, tid + 256, .. in that order, wave_sum_f64 adds the lanes, the four wavefront sums are added in
//                            order - one fixed shape whatever n is.
//   k_map_transform          one lane per point, chunks of 256.
//   k_merge_gather           lvk_frontend_merge_map's match records from the search's selection (frontend.hip).
// No kernel overwrites anything a sibling workgroup reads, there is no atomic, and no result depends on the order in which anything ran.
#include "lvk_internal.h"
#include "fe_frontend.h"
#include "lvk_wave.h"
#include <cmath>

#define A3_MAX_N      1024
#define A3_MAX_PAIRS  4096
#define A3_WAVES      4                     // pairs per workgroup
#define A3_THREADS    (64 * A3_WAVES)
#define A3_SING_REL   1e-12                 // the refinement's nrm at or below this share of W / 2 counts as zero
#define MT_CHUNK      256

struct A3Opt { double thresh2, two_thresh, min_rho2; int min_inliers, pad; };

// match k in LDS: X at m[0..2], Y at m[3..5]
__device__ __forceinline__ int a3_inlier(double c, double s, double t0, double t1, double t2, const double* m, double thresh2)
{
    const double q0 = c * m[0] - s * m[1], q1 = s * m[0] + c * m[1];
    const double dx = (q0 + t0) - m[3], dy = (q1 + t1) - m[4], dz = (m[2] + t2) - m[5];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= thresh2 ? 1 : 0;           // (false for a NaN)
}

// the minimal solver of pair (i, j); sm: the matches, 6 doubles each.  false: no model, nothing is written
__device__ __forceinline__ bool a3_solve(const double* sm, int n, int i, int j, const A3Opt& o, double& c, double& s, double& t0, double& t1, double& t2)
{
    if (i == j || i < 0 || j < 0 || i >= n || j >= n) return false;
    const double* mi = sm + 6 * i; const double* mj = sm + 6 * j;
    const double ax = mi[0] - mj[0], ay = mi[1] - mj[1], az = mi[2] - mj[2];
    const double bx = mi[3] - mj[3], by = mi[4] - mj[4], bz = mi[5] - mj[5];
    const double ra2 = ax * ax + ay * ay, rb2 = bx * bx + by * by;
    if (!(ra2 > o.min_rho2) || !(rb2 > o.min_rho2)) return false;
    if (fabs(az - bz) > o.two_thresh) return false;
    if (fabs(sqrt(ra2) - sqrt(rb2)) > o.two_thresh) return false;
    const double dot = ax * bx + ay * by, crs = ax * by - ay * bx;
    const double nrm = sqrt(dot * dot + crs * crs);
    if (!(nrm > 0.)) return false;
    c = dot / nrm; s = crs / nrm;
    const double qi0 = c * mi[0] - s * mi[1], qi1 = s * mi[0] + c * mi[1];
    const double qj0 = c * mj[0] - s * mj[1], qj1 = s * mj[0] + c * mj[1];
    t0 = ((mi[3] - qi0) + (mj[3] - qj0)) / 2.;
    t1 = ((mi[4] - qi1) + (mj[4] - qj1)) / 2.;
    t2 = ((mi[5] - mi[2]) + (mj[5] - mj[2])) / 2.;
    return true;
}

__global__ void __launch_bounds__(A3_THREADS) k_align3d_hypotheses(const double* __restrict__ m, int n, const lvk_align_pair* __restrict__ pairs, int n_pairs, A3Opt opt,
                                                                   lvk_align3d_hyp* __restrict__ hyp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* sm = reinterpret_cast<double*>(s_raw);
    for (int i = threadIdx.x; i < 6 * n; i += A3_THREADS) sm[i] = m[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * A3_WAVES + (threadIdx.x >> 6);
    if (h >= n_pairs) return;
    const lvk_align_pair pr = pairs[h];
    double c = 0., s = 0., t0 = 0., t1 = 0., t2 = 0.;
    const bool have = a3_solve(sm, n, pr.i, pr.j, opt, c, s, t0, t1, t2);       // the same on every lane
    int count = 0;
    if (have)
        for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            const int in = k < n ? a3_inlier(c, s, t0, t1, t2, sm + 6 * k, opt.thresh2) : 0;
            count += __popcll(__ballot(in));
        }
    if (lane == 0) {
        lvk_align3d_hyp* o = hyp + h;
        o->n_models = have ? 1 : 0; o->count = count; o->pad[0] = 0; o->pad[1] = 0;
        o->c = c; o->s = s; o->t[0] = t0; o->t[1] = t1; o->t[2] = t2;
    }
}

#define A3_NSUM 6
// the workgroup's sum of each of acc[0 .. cnt): lanes by wave_sum_f64, then the four wavefronts in order
__device__ __forceinline__ void a3_block_sums(double* acc, int cnt, double (*s_red)[A3_NSUM])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                         // the previous round's sums have been read
#pragma unroll
    for (int q = 0; q < A3_NSUM; ++q) if (q < cnt) { const double v = wave_sum_f64(acc[q]); if (lane == 0) s_red[wave][q] = v; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < A3_NSUM; ++q) if (q < cnt) acc[q] = ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
}

__global__ void __launch_bounds__(A3_THREADS) k_align3d_select_refine(const double* __restrict__ m, int n, const lvk_align_pair* __restrict__ pairs,
                                                                      const lvk_align3d_hyp* __restrict__ hyp, int n_pairs, A3Opt opt, uint8_t* __restrict__ mask,
                                                                      lvk_align_result* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* sm = reinterpret_cast<double*>(s_raw);
    __shared__ int s_key[A3_WAVES];
    __shared__ double s_red[A3_WAVES][A3_NSUM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 6 * n; i += A3_THREADS) sm[i] = m[i];
    int key = -1;
    for (int h = tid; h < n_pairs; h += A3_THREADS)
        if (hyp[h].n_models == 1) { const int k = (hyp[h].count << 12) | (4095 - h); key = k > key ? k : key; }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) { const int o = __shfl_xor(key, x, 64); key = o > key ? o : key; }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();                         // (the matches are staged, too)
    key = s_key[0];
#pragma unroll
    for (int w = 1; w < A3_WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;

    lvk_align_result res;
    memset(&res, 0, sizeof res);
    res.hyp = -1; res.root = -1; res.pair_i = -1; res.pair_j = -1; res.c = 1.; res.c0 = 1.;
    if (key < 0) {
        for (int k = tid; k < n; k += A3_THREADS) mask[k] = 0;
        res.status = LVK_ALIGN_NO_MODEL;
        if (tid == 0) *out = res;
        return;
    }
    const int wh = 4095 - (key & 4095);
    const int count = hyp[wh].count;
    const double wc = hyp[wh].c, ws = hyp[wh].s, wt0 = hyp[wh].t[0], wt1 = hyp[wh].t[1], wt2 = hyp[wh].t[2];
    res.hyp = wh; res.root = 0; res.pair_i = pairs[wh].i; res.pair_j = pairs[wh].j; res.n_inliers = count;
    res.c0 = wc; res.s0 = ws; res.c = wc; res.s = ws;
    res.t0[0] = wt0; res.t0[1] = wt1; res.t0[2] = wt2; res.t[0] = wt0; res.t[1] = wt1; res.t[2] = wt2;
    unsigned in_bits = 0;                    // this thread's matches tid + 256 q, q < 4
#pragma unroll
    for (int q = 0; q < A3_MAX_N / A3_THREADS; ++q) {
        const int k = tid + A3_THREADS * q;
        if (k < n) {
            const int in = a3_inlier(wc, ws, wt0, wt1, wt2, sm + 6 * k, opt.thresh2);
            mask[k] = (uint8_t)in; in_bits |= (unsigned)in << q;
        }
    }
    if (count < opt.min_inliers) {
        res.status = LVK_ALIGN_FEW_INLIERS;
        if (tid == 0) *out = res;
        return;
    }
    const double cnt = (double)count;
    double acc[A3_NSUM];
    // sweep 1: the centroids
#pragma unroll
    for (int q = 0; q < A3_NSUM; ++q) acc[q] = 0.;
#pragma unroll
    for (int q = 0; q < A3_MAX_N / A3_THREADS; ++q) {
        if (!((in_bits >> q) & 1u)) continue;
        const double* mk = sm + 6 * (tid + A3_THREADS * q);
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[r] += mk[r];
    }
    a3_block_sums(acc, 6, s_red);
    const double mX0 = acc[0] / cnt, mX1 = acc[1] / cnt, mX2 = acc[2] / cnt, mY0 = acc[3] / cnt, mY1 = acc[4] / cnt, mY2 = acc[5] / cnt;
    // sweep 2: D, C, W over the centred horizontal parts
#pragma unroll
    for (int q = 0; q < A3_NSUM; ++q) acc[q] = 0.;
#pragma unroll
    for (int q = 0; q < A3_MAX_N / A3_THREADS; ++q) {
        if (!((in_bits >> q) & 1u)) continue;
        const double* mk = sm + 6 * (tid + A3_THREADS * q);
        const double x0 = mk[0] - mX0, x1 = mk[1] - mX1, y0 = mk[3] - mY0, y1 = mk[4] - mY1;
        acc[0] += x0 * y0 + x1 * y1;
        acc[1] += x0 * y1 - x1 * y0;
        acc[2] += (x0 * x0 + x1 * x1) + (y0 * y0 + y1 * y1);
    }
    a3_block_sums(acc, 3, s_red);
    const double D = acc[0], C = acc[1], W = acc[2];
    const double nrm = sqrt(D * D + C * C);
    double c = wc, s = ws, t0 = wt0, t1 = wt1, t2 = wt2;
    int status = LVK_ALIGN_SINGULAR;
    if (nrm > A3_SING_REL * (W / 2.)) {
        status = LVK_ALIGN_OK;
        c = D / nrm; s = C / nrm;
        t0 = mY0 - (c * mX0 - s * mX1); t1 = mY1 - (s * mX0 + c * mX1); t2 = mY2 - mX2;
    }
    // sweep 3: A and the residual at the model that is returned
#pragma unroll
    for (int q = 0; q < A3_NSUM; ++q) acc[q] = 0.;
#pragma unroll
    for (int q = 0; q < A3_MAX_N / A3_THREADS; ++q) {
        if (!((in_bits >> q) & 1u)) continue;
        const double* mk = sm + 6 * (tid + A3_THREADS * q);
        const double q0 = c * mk[0] - s * mk[1], q1 = s * mk[0] + c * mk[1];
        const double rx = (q0 + t0) - mk[3], ry = (q1 + t1) - mk[4], rz = (mk[2] + t2) - mk[5];
        acc[0] += q1 * q1 + q0 * q0;
        acc[1] += -q1;
        acc[2] += q0;
        acc[3] += (rx * rx + ry * ry) + rz * rz;
    }
    a3_block_sums(acc, 4, s_red);
    res.status = status;
    res.c = c; res.s = s; res.t[0] = t0; res.t[1] = t1; res.t[2] = t2;
    res.A[0] = acc[0]; res.A[1] = acc[1]; res.A[4] = acc[1]; res.A[2] = acc[2]; res.A[8] = acc[2];
    res.A[5] = cnt; res.A[10] = cnt; res.A[15] = cnt;
    res.rms = sqrt(acc[3] / cnt);
    if (tid == 0) *out = res;
}

// the options with their defaults filled in and their ranges checked; false: *why names the field
static bool a3_options(const lvk_align3d_options* opt, A3Opt* o, const char** why)
{
    lvk_align3d_options a = {0., 0., 0, 0};
    if (opt) a = *opt;
    if (a.thresh == 0.) a.thresh = 0.10;
    if (a.min_rho == 0.) a.min_rho = 0.5;
    if (a.min_inliers == 0) a.min_inliers = 6;
    if (!(std::isfinite(a.thresh) && a.thresh > 0.)) { *why = "thresh must be positive and finite"; return false; }
    if (!(std::isfinite(a.min_rho) && a.min_rho > 0.)) { *why = "min_rho must be positive and finite"; return false; }
    if (a.min_inliers < 2 || a.min_inliers > A3_MAX_N) { *why = "min_inliers outside 2..1024"; return false; }
    if (o) { o->thresh2 = a.thresh * a.thresh; o->two_thresh = 2. * a.thresh; o->min_rho2 = a.min_rho * a.min_rho; o->min_inliers = a.min_inliers; o->pad = 0; }
    return true;
}
bool fe_align3d_options_ok(const lvk_align3d_options* opt, const char** why) { return a3_options(opt, nullptr, why); }

extern "C" lvk_status lvk_align_ransac_3d(lvk_context* ctx, const lvk_align3d_match* d_m, int n, const lvk_align_pair* d_pairs, int n_pairs, const lvk_align3d_options* opt,
                                          lvk_align3d_hyp* d_hyp, uint8_t* d_mask, lvk_align_result* d_out)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n < 0 || n_pairs < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_3d: negative count (n %d, n_pairs %d)", n, n_pairs);
    if (!d_out || (n > 0 && (!d_m || !d_mask)) || (n_pairs > 0 && !d_pairs)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_3d: null pointer");
    A3Opt o; const char* why = "";
    if (!a3_options(opt, &o, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_align_ransac_3d: %s", why);
    if (n > A3_MAX_N) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_align_ransac_3d: %d matches, at most %d (they are staged in LDS)", n, A3_MAX_N);
    if (n_pairs > A3_MAX_PAIRS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_align_ransac_3d: %d pairs, at most %d", n_pairs, A3_MAX_PAIRS);
    const int np = n < 2 ? 0 : n_pairs;                    // fewer than two matches: no pair can give a model, none is looked at
    lvk_align3d_hyp* hyp = d_hyp;
    if (np > 0 && !hyp) {
        hyp = (lvk_align3d_hyp*)lvk_ctx_scratch(ctx, LVK_SCR_ALIGN3D_HYP, sizeof(lvk_align3d_hyp) * A3_MAX_PAIRS);
        if (!hyp) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_align_ransac_3d: scratch allocation failed");
    }
    const double* m = reinterpret_cast<const double*>(d_m);
    const size_t lds = sizeof(lvk_align3d_match) * (size_t)n;
    if (np > 0) hipLaunchKernelGGL(k_align3d_hypotheses, dim3((np + A3_WAVES - 1) / A3_WAVES), dim3(A3_THREADS), lds, ctx->stream, m, n, d_pairs, np, o, hyp);
    hipLaunchKernelGGL(k_align3d_select_refine, dim3(1), dim3(A3_THREADS), lds, ctx->stream, m, n, d_pairs, (const lvk_align3d_hyp*)hyp, np, o, d_mask, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

extern "C" lvk_status lvk_align_invert(const lvk_align_result* in, lvk_align_result* out)
{
    if (!in || !out) return LVK_ERR_ARG;
    const double c = in->c, s = in->s, t0 = in->t[0], t1 = in->t[1], t2 = in->t[2];
    memset(out, 0, sizeof *out);
    out->c = c; out->s = -s;
    out->t[0] = -(c * t0 + s * t1); out->t[1] = -(c * t1 - s * t0); out->t[2] = -t2;
    return LVK_OK;
}

// ------------------------------------------------------------------------------------------------ the alignment applied to a point set
struct MtArgs { double c, s, t[3], P[16]; int have_P, pad; };

__global__ void __launch_bounds__(MT_CHUNK) k_map_transform(const double* __restrict__ X, const double* __restrict__ cov, const unsigned long long* __restrict__ desc, int n,
                                                            MtArgs a, double* __restrict__ X_out, double* __restrict__ cov_out, unsigned long long* __restrict__ desc_out)
{
    const int i = blockIdx.x * MT_CHUNK + threadIdx.x;
    if (i >= n) return;
    const size_t I = (size_t)i;
    const double c = a.c, s = a.s;
    const double x0 = X[3 * I], x1 = X[3 * I + 1], x2 = X[3 * I + 2];
    const double q0 = c * x0 - s * x1, q1 = s * x0 + c * x1;
    X_out[3 * I] = q0 + a.t[0]; X_out[3 * I + 1] = q1 + a.t[1]; X_out[3 * I + 2] = x2 + a.t[2];
    if (cov_out) {
        double w[6] = {0., 0., 0., 0., 0., 0.};          // 00 01 02 11 12 22
        if (cov) {
            const double* S = cov + 9 * I;
            const double sa = S[0], sb = S[1], sd = S[4], se = S[2], sf = S[5], sg = S[8];
            const double m00 = c * sa - s * sb, m01 = c * sb - s * sd, m10 = s * sa + c * sb, m11 = s * sb + c * sd;
            w[0] = m00 * c - m01 * s; w[1] = m00 * s + m01 * c; w[3] = m10 * s + m11 * c;
            w[2] = c * se - s * sf; w[4] = s * se + c * sf; w[5] = sg;
        }
        if (a.have_P) {
            const double j[3] = {-q1, q0, 0.};
            int e = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int u = r; u < 3; ++u, ++e) {
                    const double k = (((j[r] * j[u]) * a.P[0] + j[r] * a.P[1 + u]) + j[u] * a.P[1 + r]) + a.P[4 * (1 + r) + (1 + u)];
                    w[e] = cov ? w[e] + k : k;
                }
        }
        double* o = cov_out + 9 * I;
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[1]; o[4] = w[3]; o[5] = w[4]; o[6] = w[2]; o[7] = w[4]; o[8] = w[5];
    }
    if (desc_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) desc_out[4 * I + k] = desc[4 * I + k];
    }
}

static bool a3_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

extern "C" lvk_status lvk_map_transform(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, int n, const lvk_align_result* align,
                                        const double* cov_align16, double* d_X_out, double* d_cov_out, uint8_t* d_desc_out)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_transform: negative count (n %d)", n);
    const bool want_cov = d_cov || cov_align16;
    if (n > 0 && (!d_X || !d_X_out || (want_cov && !d_cov_out) || (d_desc && !d_desc_out))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_transform: null pointer");
    MtArgs a;
    memset(&a, 0, sizeof a);
    a.c = 1.;
    if (align) { a.c = align->c; a.s = align->s; a.t[0] = align->t[0]; a.t[1] = align->t[1]; a.t[2] = align->t[2]; }
    if (!a3_finite(&a.c, 1) || !a3_finite(&a.s, 1) || !a3_finite(a.t, 3)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_transform: the alignment is not finite");
    if (cov_align16) {
        if (!a3_finite(cov_align16, 16)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_transform: cov_align16 is not finite");
        memcpy(a.P, cov_align16, sizeof a.P); a.have_P = 1;
    }
    if (d_desc && ((((uintptr_t)d_desc) | ((uintptr_t)d_desc_out)) & 7u)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_transform: descriptors must be 8-byte aligned");
    if (n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_map_transform: %d points, at most %d", n, LVK_MAP_MAX_POINTS);
    if (n == 0) return LVK_OK;
    // an output whose inputs are NULL is not touched, whatever the caller passed for it
    hipLaunchKernelGGL(k_map_transform, dim3((n + MT_CHUNK - 1) / MT_CHUNK), dim3(MT_CHUNK), 0, ctx->stream, d_X, d_cov, reinterpret_cast<const unsigned long long*>(d_desc), n, a,
                       d_X_out, want_cov ? d_cov_out : (double*)nullptr, d_desc ? reinterpret_cast<unsigned long long*>(d_desc_out) : (unsigned long long*)nullptr);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// ------------------------------------------------------------------------------------------------ lvk_frontend_merge_map's gather
// record k: X = point sel[k].cand of the n_b sorted points of B, Y = point sel[k].index of the n_a resident points; an index outside its
// array is compared before it is followed and gives a record of NaNs, which no model holds
__global__ void __launch_bounds__(MT_CHUNK) k_merge_gather(const lvk_global_match* __restrict__ sel, int n, const double* __restrict__ XB, int n_b, const double* __restrict__ XA,
                                                           int n_a, double* __restrict__ out)
{
    const int k = blockIdx.x * MT_CHUNK + threadIdx.x;
    if (k >= n) return;
    const int ib = sel[k].cand, ia = sel[k].index;
    const bool ok = ib >= 0 && ib < n_b && ia >= 0 && ia < n_a;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[6 * (size_t)k + r] = ok ? XB[3 * (size_t)ib + r] : nan;
        out[6 * (size_t)k + 3 + r] = ok ? XA[3 * (size_t)ia + r] : nan;
    }
}
lvk_status fe_merge_gather(lvk_context* ctx, const lvk_global_match* d_sel, int n, const double* d_XB, int n_b, const double* d_XA, int n_a, lvk_align3d_match* d_out)
{
    if (n <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_merge_gather, dim3((n + MT_CHUNK - 1) / MT_CHUNK), dim3(MT_CHUNK), 0, ctx->stream, d_sel, n, d_XB, n_b, d_XA, n_a, reinterpret_cast<double*>(d_out));
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
