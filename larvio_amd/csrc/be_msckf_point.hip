// be_msckf_point.hip — first-order position covariance of the MSCKF points the filter triangulates (lvk_ekf_msckf_point_cov,
// include/lvk_c.h).  For a point with M observations from distinct clones, with Hx_t / He_t / Hf_t of d_msckf_obs_jacobian (be_dev.h):
//   A = sum_t Hf_t^T Hf_t,  G_t = A^-1 Hf_t^T,  B = sum_t G_t Hc[2t:2t+2, :],  Sigma = sigma2 A^-1 + B P[cc, cc] B^T
// where Hc (2M x c, c = fj_cols(JOB_MSCKF, M)) is the compact block k_feature_rows builds before its Householder step and cc its column map.
#include "be_host.h"
#include <math.h>
#include <vector>

#define MP_THREADS 256
#define MP_MAX_OBS 64
#define MP_MAX_C fj_cols(JOB_MSCKF, MP_MAX_OBS)

// One workgroup per point.  Hc is never formed: row block t of it is non-zero in columns 0..6 (He_t and, under estimate_td, the
// observation's zv) and 7+6t..7+6t+5 (Hx_t), so thread t < M
//   - computes its observation's Jacobians and parks Hf_t in LDS,
//   - forms A (every thread the same sum, in observation order), its LDL^T pivots and G_t (two solves with d_solve3_spd),
//   - writes its own six columns of B (G_t Hx_t: one term each) and E_t = G_t [He_t | zv_t] (3 x 7);
// threads 0..20 then sum the E_t in observation order into columns 0..6 of B.  T = B P[cc, cc] is streamed one column of cc per
// thread: for a fixed row cc[l] the threads read consecutive entries of P, B and cc come from LDS as broadcasts, every sum runs over
// l = 0..c-1 in that order.  T takes the LDS the E_t held.  Threads 0..5 form the six upper entries of sigma2 A^-1 + T B^T and write
// their mirrors.  LDS: 3 KB (Hf) + 10.5 KB (E / T) + 9.2 KB (B) + 1.5 KB (cc), whatever M.  Nothing of P outside rows and columns cc
// is read, and nothing but the point's own outputs is written.
// A point whose A has a non-positive pivot (or whose pending triangulation failed) gets nine NaNs and ok = 0.
__global__ __launch_bounds__(MP_THREADS) void k_msckf_point_cov(const double* __restrict__ P, int ldp, const PointJob* __restrict__ jobs, int n_jobs,
                                                                const CloneDev* __restrict__ clones, const int* __restrict__ obs_rank,
                                                                const double* __restrict__ obs_z, const double* __restrict__ obs_zv, FilterFlags fl,
                                                                const TriResult* __restrict__ tri /* optional: PointJob::tri_slot1 - 1 indexes it */,
                                                                double* __restrict__ out_cov9, int* __restrict__ out_ok)
{
    __shared__ double sHf[MP_MAX_OBS * 6], sET[MP_MAX_OBS * 21], sB[3 * MP_MAX_C], sAinv[6];
    __shared__ int scc[MP_MAX_C], sbad;
    const int jb = blockIdx.x, t = threadIdx.x;
    if (jb >= n_jobs) return;                            // (uniform over the workgroup)
    const PointJob job = jobs[jb];
    const int M = job.n_obs, c = fj_cols(JOB_MSCKF, M);
    double p_w[3] = {job.p_w[0], job.p_w[1], job.p_w[2]};
    int tri_ok = 1;
    if (tri && job.tri_slot1 > 0) {                      // the triangulation queued ahead of this launch, as k_feature_rows reads it
        const TriResult* r = tri + (job.tri_slot1 - 1);
        tri_ok = r->ok; p_w[0] = r->position[0]; p_w[1] = r->position[1]; p_w[2] = r->position[2];
    }
    if (M < 2 || M > MP_MAX_OBS || !tri_ok) {            // (uniform) the host entry refuses such a count; a failed triangulation has no point
        if (t < 9) out_cov9[(size_t)jb * 9 + t] = NAN;
        if (t == 0) out_ok[jb] = 0;
        return;
    }
    double Hx[12], He[12], zvv[2] = {0., 0.};
    if (t < M) {
        const int oi = job.obs_off + t;
        const CloneDev ck = clones[obs_rank[oi]];
        const double z[2] = {obs_z[2 * oi], obs_z[2 * oi + 1]};
        zvv[0] = obs_zv[2 * oi]; zvv[1] = obs_zv[2 * oi + 1];
        double hf[6], r2[2];
        d_msckf_obs_jacobian(ck, p_w, z, fl.if_fej, Hx, He, hf, r2);
        for (int k = 0; k < 6; ++k) sHf[6 * t + k] = hf[k];
    }
    for (int e = t; e < c; e += MP_THREADS) scc[e] = e < 7 ? 15 + e : fl.leg_dim + 6 * obs_rank[job.obs_off + (e - 7) / 6] + (e - 7) % 6;
    __syncthreads();
    if (t < M) {
        double A[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        for (int s = 0; s < M; ++s) {
            const double* h = sHf + 6 * s;
            for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) A[i * 3 + j] += h[i] * h[j] + h[3 + i] * h[3 + j];
        }
        A[3] = A[1]; A[6] = A[2]; A[7] = A[5];
        // the pivots of d_solve3_spd's unpivoted LDL^T, as it forms them
        const double d0 = A[0];
        const double l10 = A[3] / d0, l20 = A[6] / d0;
        const double d1 = A[4] - l10 * l10 * d0;
        const double l21 = (A[7] - l20 * l10 * d0) / d1;
        const double d2 = A[8] - l20 * l20 * d0 - l21 * l21 * d1;
        const int bad = !(d0 > 0.) || !(d1 > 0.) || !(d2 > 0.);
        double g0[3], g1[3];                             // G_t = [g0 g1]
        d_solve3_spd(A, sHf + 6 * t, g0); d_solve3_spd(A, sHf + 6 * t + 3, g1);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 6; ++j) {
                sB[i * c + 7 + 6 * t + j] = g0[i] * Hx[j] + g1[i] * Hx[6 + j];
                sET[21 * t + 7 * i + j] = g0[i] * He[j] + g1[i] * He[6 + j];
            }
            sET[21 * t + 7 * i + 6] = fl.estimate_td ? g0[i] * zvv[0] + g1[i] * zvv[1] : 0.;
        }
        if (t == 0) {
            const double e0[3] = {1., 0., 0.}, e1[3] = {0., 1., 0.}, e2[3] = {0., 0., 1.};
            double x0[3], x1[3], x2[3];                  // columns of A^-1: the upper triangle is kept
            d_solve3_spd(A, e0, x0); d_solve3_spd(A, e1, x1); d_solve3_spd(A, e2, x2);
            sAinv[0] = x0[0]; sAinv[1] = x1[0]; sAinv[2] = x2[0]; sAinv[3] = x1[1]; sAinv[4] = x2[1]; sAinv[5] = x2[2];
            sbad = bad;
        }
    }
    __syncthreads();
    if (t < 21) {
        double s = 0.;
        for (int k = 0; k < M; ++k) s += sET[21 * k + t];
        sB[(t / 7) * c + t % 7] = s;
    }
    __syncthreads();
    if (sbad) {                                          // (uniform)
        if (t < 9) out_cov9[(size_t)jb * 9 + t] = NAN;
        if (t == 0) out_ok[jb] = 0;
        return;
    }
    double* sT = sET;                                    // the E_t are summed: T = B P[cc, cc] takes their place
    for (int j = t; j < c; j += MP_THREADS) {
        const double* Pj = P + scc[j];
        double s0 = 0., s1 = 0., s2 = 0.;
        for (int l = 0; l < c; ++l) {
            const double p = Pj[(size_t)scc[l] * ldp];
            s0 += sB[l] * p; s1 += sB[c + l] * p; s2 += sB[2 * c + l] * p;
        }
        sT[j] = s0; sT[c + j] = s1; sT[2 * c + j] = s2;
    }
    __syncthreads();
    if (t < 6) {
        const int i = t < 3 ? 0 : t < 5 ? 1 : 2, k = t < 3 ? t : t < 5 ? t - 2 : 2;
        double s = 0.;
        for (int j = 0; j < c; ++j) s += sT[i * c + j] * sB[k * c + j];
        const double v = fl.sigma2 * sAinv[t] + s;
        out_cov9[(size_t)jb * 9 + i * 3 + k] = v;
        if (i != k) out_cov9[(size_t)jb * 9 + k * 3 + i] = v;
    }
    if (t == 0) out_ok[jb] = 1;
}

lvk_status lvk_launch_msckf_point_cov(lvk_context* ctx, const double* d_P, int ldp, const PointJob* d_jobs, int n_jobs, const CloneDev* d_clones, const int* d_rank,
                                      const double* d_z, const double* d_zv, FilterFlags fl, const TriResult* d_tri, double* d_cov9, int* d_ok)
{
    if (n_jobs <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_msckf_point_cov, dim3(n_jobs), dim3(MP_THREADS), 0, ctx->stream, d_P, ldp, d_jobs, n_jobs, d_clones, d_rank, d_z, d_zv, fl, d_tri, d_cov9, d_ok);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// (C ABI) clone table, jobs and observations go up in one blob, the results come back through the output blob; one wait per call
extern "C" lvk_status lvk_ekf_msckf_point_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_clone* h_clones, int n_clones,
                                              const lvk_msckf_point_job* h_jobs, int n_jobs, const int* h_clone_rank, const double* h_obs, const double* h_obs_vel,
                                              int leg_dim, int if_fej, int estimate_td, double sigma2, double* h_cov9, int* h_ok)
{
    if (!ctx || !d_P || !h_clones || !h_jobs || !h_clone_rank || !h_obs || !h_obs_vel || !h_cov9 || !h_ok || n_jobs < 0 || n_clones < 0 || n <= 0 || ldp < n)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: bad argument");
    if (leg_dim != 22 && leg_dim != 46) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: leg_dim %d (22 or 46)", leg_dim);
    size_t tot = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const lvk_msckf_point_job& f = h_jobs[j];
        const int M = f.n_obs;
        if (M < 2 || M > MP_MAX_OBS) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: job %d: %d observations (2..64)", j, M);
        if (f.obs_off < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: job %d: negative observation offset", j);
        for (int k = 0; k < M; ++k) {
            const int cr = h_clone_rank[f.obs_off + k];
            if (cr < 0 || cr >= n_clones || leg_dim + 6 * (long long)cr + 6 > n)
                return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: job %d: clone rank %d (columns %lld..%lld) does not fit %d clones / a %d x %d covariance",
                                     j, cr, leg_dim + 6 * (long long)cr, leg_dim + 6 * (long long)cr + 5, n_clones, n, n);
            for (int q = 0; q < k; ++q)
                if (h_clone_rank[f.obs_off + q] == cr) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_msckf_point_cov: job %d: clone rank %d observed twice", j, cr);
        }
        tot = std::max(tot, (size_t)f.obs_off + (size_t)M);
    }
    if (n_jobs == 0) return LVK_OK;
    Stage sg(ctx);
    const size_t o_cl = sg.take(Stage::IN, sizeof(CloneDev) * (size_t)n_clones), o_job = sg.take(Stage::IN, sizeof(PointJob) * (size_t)n_jobs), o_rk = sg.take(Stage::IN, sizeof(int) * tot),
                 o_z = sg.take(Stage::IN, 16 * tot), o_zv = sg.take(Stage::IN, 16 * tot);
    const size_t n_cov = sizeof(double) * 9 * (size_t)n_jobs, n_ok = sizeof(int) * (size_t)n_jobs, o_cov = sg.take(Stage::OUT, n_cov), o_ok = sg.take(Stage::OUT, n_ok);
    LVK_TRY(sg.alloc());
    for (int i = 0; i < n_clones; ++i) clone_dev_from(h_clones[i], sg.host<CloneDev>(o_cl) + i);
    PointJob* hj = sg.host<PointJob>(o_job);
    for (int j = 0; j < n_jobs; ++j) { hj[j].n_obs = h_jobs[j].n_obs; hj[j].obs_off = h_jobs[j].obs_off; hj[j].tri_slot1 = 0; hj[j].pad = 0; memcpy(hj[j].p_w, h_jobs[j].p_w, 24); }
    memcpy(sg.host<int>(o_rk), h_clone_rank, sizeof(int) * tot);
    memcpy(sg.host<double>(o_z), h_obs, 16 * tot); memcpy(sg.host<double>(o_zv), h_obs_vel, 16 * tot);
    LVK_TRY(sg.upload());
    LVK_TRY(lvk_launch_msckf_point_cov(ctx, d_P, ldp, sg.at<PointJob>(Stage::IN, o_job), n_jobs, sg.at<CloneDev>(Stage::IN, o_cl), sg.at<int>(Stage::IN, o_rk),
                                       sg.at<double>(Stage::IN, o_z), sg.at<double>(Stage::IN, o_zv), filter_flags(leg_dim, if_fej, estimate_td, sigma2), nullptr,
                                       sg.at<double>(Stage::OUT, o_cov), sg.at<int>(Stage::OUT, o_ok)));
    LVK_TRY(sg.get(h_cov9, Stage::OUT, o_cov, n_cov));
    LVK_TRY(sg.get(h_ok, Stage::OUT, o_ok, n_ok));
    return sg.wait();
}
