// be_landmark.hip — first-order position covariance of anchored inverse-depth landmarks (lvk_ekf_landmark_cov, include/lvk_c.h).
// Sigma = J P_s J^T, P_s the 13 x 13 sub-block of the filter's covariance over [extrinsics 15..20 | the anchor clone's six columns |
// the feature's column], J the 3 x 13 derivative of Feature::position under the filter's own state injection (be_propagate.hip, lvk_ekf_inject).
#include "be_host.h"
#include <math.h>

#define LM_COLS 13

// column of P behind entry k of the 13-vector [d_theta_e d_t | d_theta d_p | d_rho]
__device__ __forceinline__ int lm_col(int k, int anchor_col, int feat_col) { return k < 6 ? 15 + k : k < 12 ? anchor_col + (k - 6) : feat_col; }

// One wavefront per landmark.  With R = R(q_anchor) (body to world), R_c2w = R R_b2c^T taken through a quaternion and back as the
// filter's clone bookkeeping does, r_c = R_c2w [u v 1] / rho (camera to point, world frame) and r = r_c + R t_c_b (clone to point),
// the injection's conventions give
//   d p_w = -[r_c]x R d_theta_e + R d_t - [r]x d_theta + d_p - (r_c / rho) d_rho.
// The lanes gather the 169 entries of P_s into LDS (nothing else of P is read), lanes 0..38 form T = J P_s one entry each, lanes 0..5
// the six upper entries of T J^T - every sum runs over l = 0..12 in that order inside one lane - and each writes its mirror as well.
__global__ __launch_bounds__(64) void k_landmark_cov(const double* __restrict__ P, int ld, const lvk_landmark_job* __restrict__ jobs, int n_jobs, double* __restrict__ out)
{
    __shared__ double Ps[LM_COLS * LM_COLS], J[3 * LM_COLS], T[3 * LM_COLS];
    const int lane = threadIdx.x, job = blockIdx.x;
    if (job >= n_jobs) return;                          // (uniform over the workgroup)
    const lvk_landmark_job* jb = jobs + job;
    const int anchor_col = jb->anchor_col, feat_col = jb->feat_col;
    for (int t = lane; t < LM_COLS * LM_COLS; t += 64)
        Ps[t] = P[(size_t)lm_col(t / LM_COLS, anchor_col, feat_col) * ld + lm_col(t % LM_COLS, anchor_col, feat_col)];
    if (lane == 0) {
        // Eigen's Quaternion::toRotationMatrix, q = [x y z w] (be_host_math.h, quat_to_rot)
        const double x = jb->q_anchor[0], y = jb->q_anchor[1], z = jb->q_anchor[2], w = jb->q_anchor[3];
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
        // The filter's own camera attitude (clone_refresh_cam): R(q) R_b2c^T goes through a quaternion and back, so that r_c below is
        // the vector Feature::position was formed with even when the configured R_b2c is orthonormal to 1e-12 only.
        // Eigen's Quaternion(Matrix3) (be_host_math.h, rot_to_quat), then toRotationMatrix again.
        double M[9], qc[4];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0.; for (int k = 0; k < 3; ++k) s += R[i * 3 + k] * jb->R_b2c[j * 3 + k]; M[i * 3 + j] = s; }
        double t = M[0] + M[4] + M[8];
        if (t > 0) {
            t = sqrt(t + 1.0);
            qc[3] = 0.5 * t;
            t = 0.5 / t;
            qc[0] = (M[7] - M[5]) * t; qc[1] = (M[2] - M[6]) * t; qc[2] = (M[3] - M[1]) * t;
        } else {
            // (i, j, k) = the largest diagonal entry and its cyclic successors; written out: no run-time index into a register array
            const int i = M[8] > (M[4] > M[0] ? M[4] : M[0]) ? 2 : M[4] > M[0] ? 1 : 0;
            const double mii = i == 0 ? M[0] : i == 1 ? M[4] : M[8], mjj = i == 0 ? M[4] : i == 1 ? M[8] : M[0], mkk = i == 0 ? M[8] : i == 1 ? M[0] : M[4];
            const double mkj = i == 0 ? M[7] : i == 1 ? M[2] : M[3], mjk = i == 0 ? M[5] : i == 1 ? M[6] : M[1];
            const double mji = i == 0 ? M[3] : i == 1 ? M[7] : M[2], mij = i == 0 ? M[1] : i == 1 ? M[5] : M[6];
            const double mki = i == 0 ? M[6] : i == 1 ? M[1] : M[5], mik = i == 0 ? M[2] : i == 1 ? M[3] : M[7];
            t = sqrt(mii - mjj - mkk + 1.0);
            const double qi = 0.5 * t;
            t = 0.5 / t;
            const double qw = (mkj - mjk) * t, qj = (mji + mij) * t, qk = (mki + mik) * t;
            qc[3] = qw;
            qc[0] = i == 0 ? qi : i == 1 ? qk : qj; qc[1] = i == 0 ? qj : i == 1 ? qi : qk; qc[2] = i == 0 ? qk : i == 1 ? qj : qi;
        }
        double Rc[9];
        {
            const double cx = qc[0], cy = qc[1], cz = qc[2], cw = qc[3];
            const double ux = 2 * cx, uy = 2 * cy, uz = 2 * cz;
            const double uwx = ux * cw, uwy = uy * cw, uwz = uz * cw, uxx = ux * cx, uxy = uy * cx, uxz = uz * cx, uyy = uy * cy, uyz = uz * cy, uzz = uz * cz;
            Rc[0] = 1 - (uyy + uzz); Rc[1] = uxy - uwz; Rc[2] = uxz + uwy; Rc[3] = uxy + uwz; Rc[4] = 1 - (uxx + uzz); Rc[5] = uyz - uwx;
            Rc[6] = uxz - uwy; Rc[7] = uyz + uwx; Rc[8] = 1 - (uxx + uyy);
        }
        const double rho = jb->inv_depth;
        const double pc[3] = {jb->obs_anchor[0] / rho, jb->obs_anchor[1] / rho, 1 / rho};
        double rc[3], r[3];
        for (int i = 0; i < 3; ++i) {
            rc[i] = Rc[i * 3] * pc[0] + Rc[i * 3 + 1] * pc[1] + Rc[i * 3 + 2] * pc[2];
            r[i] = rc[i] + (R[i * 3] * jb->t_c_b[0] + R[i * 3 + 1] * jb->t_c_b[1] + R[i * 3 + 2] * jb->t_c_b[2]);
        }
        // -[v]x, row-major
        const double Sc[9] = {0, rc[2], -rc[1], -rc[2], 0, rc[0], rc[1], -rc[0], 0};
        const double Sr[9] = {0, r[2], -r[1], -r[2], 0, r[0], r[1], -r[0], 0};
        for (int i = 0; i < 3; ++i) {
            for (int c = 0; c < 3; ++c) {
                J[i * LM_COLS + c] = Sc[i * 3] * R[c] + Sc[i * 3 + 1] * R[3 + c] + Sc[i * 3 + 2] * R[6 + c];
                J[i * LM_COLS + 3 + c] = R[i * 3 + c];
                J[i * LM_COLS + 6 + c] = Sr[i * 3 + c];
                J[i * LM_COLS + 9 + c] = i == c ? 1.0 : 0.0;
            }
            J[i * LM_COLS + 12] = -(rc[i] / rho);
        }
    }
    __syncthreads();
    if (lane < 3 * LM_COLS) {
        const int i = lane / LM_COLS, j = lane % LM_COLS;
        double s = 0.;
        for (int l = 0; l < LM_COLS; ++l) s += J[i * LM_COLS + l] * Ps[l * LM_COLS + j];
        T[lane] = s;
    }
    __syncthreads();
    if (lane < 6) {
        const int i = lane < 3 ? 0 : lane < 5 ? 1 : 2, j = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
        double s = 0.;
        for (int l = 0; l < LM_COLS; ++l) s += T[i * LM_COLS + l] * J[j * LM_COLS + l];
        out[(size_t)job * 9 + i * 3 + j] = s;
        if (i != j) out[(size_t)job * 9 + j * 3 + i] = s;
    }
}

// what the kernel assumes of one job on an n x n covariance: every column it names lies in [0, n) and the depth is finite
bool lvk_landmark_job_ok(const lvk_landmark_job* j, int n)
{
    return n >= 21 && j->anchor_col >= 0 && j->anchor_col <= n - 6 && j->feat_col >= 0 && j->feat_col < n && j->inv_depth != 0.0;
}

lvk_status lvk_launch_landmark_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_landmark_job* d_jobs, int n_jobs, double* d_cov9)
{
    if (n_jobs <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_landmark_cov, dim3(n_jobs), dim3(64), 0, ctx->stream, d_P, ldp, d_jobs, n_jobs, d_cov9);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// (C ABI) jobs go up in the stage's input blob, the results come back through its output blob; one wait per call
extern "C" lvk_status lvk_ekf_landmark_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_landmark_job* h_jobs, int n_jobs, double* h_cov9)
{
    if (!ctx || !d_P || !h_jobs || !h_cov9 || n_jobs < 0 || ldp < n)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_landmark_cov: bad argument");
    for (int k = 0; k < n_jobs; ++k)
        if (!lvk_landmark_job_ok(h_jobs + k, n))
            return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_landmark_cov: job %d (anchor columns %d..%d, feature column %d, inverse depth %g) does not fit a %d x %d covariance",
                                 k, h_jobs[k].anchor_col, h_jobs[k].anchor_col + 5, h_jobs[k].feat_col, h_jobs[k].inv_depth, n, n);
    if (n_jobs == 0) return LVK_OK;
    const size_t jbytes = sizeof(lvk_landmark_job) * (size_t)n_jobs, obytes = sizeof(double) * 9 * (size_t)n_jobs;
    Stage sg(ctx);
    const size_t o_jobs = sg.take(Stage::IN, jbytes), o_out = sg.take(Stage::OUT, obytes);
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_jobs, h_jobs, jbytes));
    LVK_TRY(lvk_launch_landmark_cov(ctx, d_P, ldp, sg.at<lvk_landmark_job>(Stage::IN, o_jobs), n_jobs, sg.at<double>(Stage::OUT, o_out)));
    LVK_TRY(sg.get(h_cov9, Stage::OUT, o_out, obytes));
    return sg.wait();
}
