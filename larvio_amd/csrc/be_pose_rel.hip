// be_pose_rel.hip — first-order covariance of one pose relative to another, and the absolute 6 x 6 block of one pose
// (lvk_ekf_pose_rel_cov, include/lvk_c.h).  Sigma_rel = J P_s J^T, P_s the 12 x 12 sub-block of the filter's covariance over
// [d_theta_a d_p_a d_theta_b d_p_b], J the 6 x 12 derivative of (R_a^T R_b, R_a^T (p_b - p_a)) under the filter's own state injection
// (be_propagate.hip, lvk_ekf_inject).
#include "be_host.h"
#include <math.h>

#define PR_COLS 12
#define PR_OUT 6

// column of P behind entry k of the 12-vector [d_theta_a d_p_a | d_theta_b d_p_b]
__device__ __forceinline__ int pr_col(int k, int at, int ap, int bt, int bp) { return k < 3 ? at + k : k < 6 ? ap + (k - 3) : k < 9 ? bt + (k - 6) : bp + (k - 9); }

// One wavefront per job.  With R_a = R(q_a) (body to world) and d = p_b - p_a, the injection's conventions (R <- (I + [d_theta]x) R,
// p <- p + d_p) give, for the error of the relative pose defined by R_ab,true = (I + [d_phi]x) R_ab and p_ab,true = p_ab + d_rho,
//   d_phi = R_a^T (d_theta_b - d_theta_a),   d_rho = R_a^T [d]x d_theta_a + R_a^T (d_p_b - d_p_a),
// i.e. J = [ -R_a^T 0 R_a^T 0 ; R_a^T [d]x  -R_a^T  0  R_a^T ].
// The lanes gather the 144 entries of P_s into LDS (nothing else of P is read), T = J P_s one entry per lane (72 entries: lanes 0..7
// take a second one), lanes 0..20 the upper entries of T J^T - every sum runs over l = 0..11 in that order inside one lane - and each
// writes its mirror as well.  An absolute job (a_theta_col < 0) copies the 36 entries of b's block, order [d_theta_b d_p_b].
__global__ __launch_bounds__(64) void k_pose_rel_cov(const double* __restrict__ P, int ld, const lvk_pose_rel_job* __restrict__ jobs, int n_jobs, double* __restrict__ out)
{
    __shared__ double Ps[PR_COLS * PR_COLS], J[PR_OUT * PR_COLS], T[PR_OUT * PR_COLS];
    const int lane = threadIdx.x, job = blockIdx.x;
    if (job >= n_jobs) return;                          // (uniform over the workgroup)
    const lvk_pose_rel_job* jb = jobs + job;
    const int at = jb->a_theta_col, ap = jb->a_p_col, bt = jb->b_theta_col, bp = jb->b_p_col;
    double* o = out + (size_t)job * 36;
    if (at < 0) {                                       // (uniform) a pure gather
        if (lane < 36) {
            const int i = lane / 6, j = lane % 6;
            o[lane] = P[(size_t)(i < 3 ? bt + i : bp + (i - 3)) * ld + (j < 3 ? bt + j : bp + (j - 3))];
        }
        return;
    }
    for (int t = lane; t < PR_COLS * PR_COLS; t += 64)
        Ps[t] = P[(size_t)pr_col(t / PR_COLS, at, ap, bt, bp) * ld + pr_col(t % PR_COLS, at, ap, bt, bp)];
    if (lane == 0) {
        // Eigen's Quaternion::toRotationMatrix, q = [x y z w] (be_host_math.h, quat_to_rot)
        const double x = jb->q_a[0], y = jb->q_a[1], z = jb->q_a[2], w = jb->q_a[3];
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
        const double d[3] = {jb->p_b[0] - jb->p_a[0], jb->p_b[1] - jb->p_a[1], jb->p_b[2] - jb->p_a[2]};
        // [d]x, row-major
        const double S[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) {
                const double rt = R[c * 3 + i];         // R_a^T
                J[i * PR_COLS + c] = -rt; J[i * PR_COLS + 3 + c] = 0.0; J[i * PR_COLS + 6 + c] = rt; J[i * PR_COLS + 9 + c] = 0.0;
                J[(3 + i) * PR_COLS + c] = R[i] * S[c] + R[3 + i] * S[3 + c] + R[6 + i] * S[6 + c];
                J[(3 + i) * PR_COLS + 3 + c] = -rt; J[(3 + i) * PR_COLS + 6 + c] = 0.0; J[(3 + i) * PR_COLS + 9 + c] = rt;
            }
    }
    __syncthreads();
    for (int t = lane; t < PR_OUT * PR_COLS; t += 64) {
        const int i = t / PR_COLS, j = t % PR_COLS;
        double s = 0.;
        for (int l = 0; l < PR_COLS; ++l) s += J[i * PR_COLS + l] * Ps[l * PR_COLS + j];
        T[t] = s;
    }
    __syncthreads();
    if (lane < 21) {
        // upper triangle of a 6 x 6 matrix, row by row: rows start at 0, 6, 11, 15, 18, 20
        const int i = lane < 6 ? 0 : lane < 11 ? 1 : lane < 15 ? 2 : lane < 18 ? 3 : lane < 20 ? 4 : 5;
        const int j = lane - (i == 0 ? 0 : i == 1 ? 6 : i == 2 ? 11 : i == 3 ? 15 : i == 4 ? 18 : 20) + i;
        double s = 0.;
        for (int l = 0; l < PR_COLS; ++l) s += T[i * PR_COLS + l] * J[j * PR_COLS + l];
        o[i * 6 + j] = s;
        if (i != j) o[j * 6 + i] = s;
    }
}

// what the kernel assumes of one job on an n x n covariance: every column triple it names lies in [0, n)
bool lvk_pose_rel_job_ok(const lvk_pose_rel_job* j, int n)
{
    const auto fits = [n](int c) { return c >= 0 && c <= n - 3; };
    if (!fits(j->b_theta_col) || !fits(j->b_p_col)) return false;
    return j->a_theta_col < 0 || (fits(j->a_theta_col) && fits(j->a_p_col));
}

lvk_status lvk_launch_pose_rel_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_pose_rel_job* d_jobs, int n_jobs, double* d_cov36)
{
    if (n_jobs <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_pose_rel_cov, dim3(n_jobs), dim3(64), 0, ctx->stream, d_P, ldp, d_jobs, n_jobs, d_cov36);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// (C ABI) jobs go up in the stage's input blob, the results come back through its output blob; one wait per call
extern "C" lvk_status lvk_ekf_pose_rel_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_pose_rel_job* h_jobs, int n_jobs, double* h_cov36)
{
    if (!ctx || !d_P || !h_jobs || !h_cov36 || n_jobs < 0 || ldp < n)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_pose_rel_cov: bad argument");
    for (int k = 0; k < n_jobs; ++k)
        if (!lvk_pose_rel_job_ok(h_jobs + k, n))
            return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_pose_rel_cov: job %d (columns a %d.. / %d.., b %d.. / %d..) does not fit a %d x %d covariance",
                                 k, h_jobs[k].a_theta_col, h_jobs[k].a_p_col, h_jobs[k].b_theta_col, h_jobs[k].b_p_col, n, n);
    if (n_jobs == 0) return LVK_OK;
    const size_t jbytes = sizeof(lvk_pose_rel_job) * (size_t)n_jobs, obytes = sizeof(double) * 36 * (size_t)n_jobs;
    Stage sg(ctx);
    const size_t o_jobs = sg.take(Stage::IN, jbytes), o_out = sg.take(Stage::OUT, obytes);
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_jobs, h_jobs, jbytes));
    LVK_TRY(lvk_launch_pose_rel_cov(ctx, d_P, ldp, sg.at<lvk_pose_rel_job>(Stage::IN, o_jobs), n_jobs, sg.at<double>(Stage::OUT, o_out)));
    LVK_TRY(sg.get(h_cov36, Stage::OUT, o_out, obytes));
    return sg.wait();
}
