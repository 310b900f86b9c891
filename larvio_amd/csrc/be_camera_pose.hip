// be_camera_pose.hip — the camera pose of one clone of the window and its 6 x 6 covariance in the order [dtheta dp] that
// lvk_map_select_queries takes as cov_cam (lvk_ekf_camera_pose_cov, include/lvk_c.h).  cov_cam = J P_s J^T, P_s the 12 x 12 sub-block of
// the filter's covariance over [extrinsics 15..20 | the clone's six columns], J the 6 x 12 derivative of (R_wc, p_wc) = (R_b R_b2c^T,
// p_b + R_b t_c_b) under the filter's own state injection (be_propagate.hip, lvk_ekf_inject), the rotation error on the camera side.
#include "be_host.h"
#include <math.h>
#include <cmath>

#define CP_COLS 12
#define CP_OUT  48                               // R_wc (9), p_wc (3), cov_cam (36)

// column of P behind entry k of the 12-vector [d_theta_e d_t | d_theta_b d_p_b]
__device__ __forceinline__ int cp_col(int k, int clone_col) { return k < 6 ? 15 + k : clone_col + (k - 6); }

// Eigen's Quaternion::toRotationMatrix, q = [x y z w] (be_host_math.h, quat_to_rot; be_landmark_rel.hip has the same lines)
__device__ __forceinline__ void cp_quat_to_rot(const double* q, double* R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy; R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// One wavefront.  The lanes gather the 144 entries of P_s into LDS (nothing else of P is read); lane 0 forms R_b, R_wc, u = R_b t_c_b,
// p_wc and J; the lanes form T = J P_s, 72 entries, each a sum over l = 0..11 in that order inside one lane (the zero entries of J are
// terms like any other); lanes 0..20 form the 21 upper entries of T J^T the same way and each writes its mirror as well.
__global__ __launch_bounds__(64) void k_camera_pose_cov(const double* __restrict__ P, int ld, const lvk_camera_pose_job* __restrict__ job, double* __restrict__ out)
{
    __shared__ double Ps[CP_COLS * CP_COLS], J[6 * CP_COLS], T[6 * CP_COLS];
    const int lane = threadIdx.x;
    const int clone_col = job->clone_col;
    for (int t = lane; t < CP_COLS * CP_COLS; t += 64) Ps[t] = P[(size_t)cp_col(t / CP_COLS, clone_col) * ld + cp_col(t % CP_COLS, clone_col)];
    if (lane == 0) {
        double Rb[9], Re[9], Rwc[9], u[3];
        cp_quat_to_rot(job->q_b, Rb);
        for (int i = 0; i < 9; ++i) Re[i] = job->R_b2c[i];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rwc[i * 3 + j] = (Rb[i * 3] * Re[j * 3] + Rb[i * 3 + 1] * Re[j * 3 + 1]) + Rb[i * 3 + 2] * Re[j * 3 + 2];
        for (int i = 0; i < 3; ++i) u[i] = (Rb[i * 3] * job->t_c_b[0] + Rb[i * 3 + 1] * job->t_c_b[1]) + Rb[i * 3 + 2] * job->t_c_b[2];
        for (int i = 0; i < 9; ++i) out[i] = Rwc[i];
        for (int i = 0; i < 3; ++i) out[9 + i] = job->p_b[i] + u[i];
        for (int i = 0; i < 6 * CP_COLS; ++i) J[i] = 0.;
        const double Su[9] = {0, u[2], -u[1], -u[2], 0, u[0], u[1], -u[0], 0};        // -[u]x, row-major
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) {
                J[i * CP_COLS + c] = Re[i * 3 + c];                   // dtheta: R_b2c d_theta_e ...
                J[i * CP_COLS + 6 + c] = Rwc[c * 3 + i];              //         ... + R_wc^T d_theta_b
                J[(3 + i) * CP_COLS + 3 + c] = Rb[i * 3 + c];         // dp: R_b d_t ...
                J[(3 + i) * CP_COLS + 6 + c] = Su[i * 3 + c];         //     ... - [R_b t_c_b]x d_theta_b ...
                J[(3 + i) * CP_COLS + 9 + c] = i == c ? 1. : 0.;      //     ... + d_p_b
            }
    }
    __syncthreads();
    for (int t = lane; t < 6 * CP_COLS; t += 64) {
        const int i = t / CP_COLS, j = t % CP_COLS;
        double s = 0.;
        for (int l = 0; l < CP_COLS; ++l) s += J[i * CP_COLS + l] * Ps[l * CP_COLS + j];
        T[t] = s;
    }
    __syncthreads();
    if (lane < 21) {
        int i = 0, j = lane;
        while (j >= 6 - i) { j -= 6 - i; ++i; }         // lane -> (i, i + j) of the upper triangle, row by row
        j += i;
        double s = 0.;
        for (int l = 0; l < CP_COLS; ++l) s += T[i * CP_COLS + l] * J[j * CP_COLS + l];
        out[12 + i * 6 + j] = s;
        if (i != j) out[12 + j * 6 + i] = s;
    }
}

// what the kernel assumes of the job on an n x n covariance (null: nothing)
static const char* camera_pose_job_flaw(const lvk_camera_pose_job* j, int n)
{
    if (j->clone_col < 21 || j->clone_col + 6 > n) return "clone_col is below 21 or its six columns leave [0, n)";
    bool finite = true;
    for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(j->q_b[k]);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(j->p_b[k]) && std::isfinite(j->t_c_b[k]);
    for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(j->R_b2c[k]);
    if (!finite) return "a value of the job is not finite";
    if (!(fabs(sqrt(j->q_b[0] * j->q_b[0] + j->q_b[1] * j->q_b[1] + j->q_b[2] * j->q_b[2] + j->q_b[3] * j->q_b[3]) - 1.0) <= 1e-6)) return "q_b is not a unit quaternion";
    return nullptr;
}

// (C ABI) the job goes up in the stage's input blob, the 48 doubles come back through its output blob; one launch, one wait
extern "C" lvk_status lvk_ekf_camera_pose_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_camera_pose_job* h_job, double* h_R_wc, double* h_p_wc,
                                              double* h_cov36)
{
    if (!ctx || !d_P || !h_job || !h_R_wc || !h_p_wc || !h_cov36 || ldp < n) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_camera_pose_cov: bad argument");
    if (const char* flaw = camera_pose_job_flaw(h_job, n)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_camera_pose_cov: %s (clone_col %d, n %d)", flaw, h_job->clone_col, n);
    double got[CP_OUT];
    Stage sg(ctx);
    const size_t o_job = sg.take(Stage::IN, sizeof *h_job), o_out = sg.take(Stage::OUT, sizeof got);
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_job, h_job, sizeof *h_job));
    hipLaunchKernelGGL(k_camera_pose_cov, dim3(1), dim3(64), 0, ctx->stream, d_P, ldp, sg.at<lvk_camera_pose_job>(Stage::IN, o_job), sg.at<double>(Stage::OUT, o_out));
    LVK_LAUNCH_CHECK(ctx);
    LVK_TRY(sg.get(got, Stage::OUT, o_out, sizeof got));
    LVK_TRY(sg.wait());
    for (int k = 0; k < 9; ++k) h_R_wc[k] = got[k];
    for (int k = 0; k < 3; ++k) h_p_wc[k] = got[9 + k];
    for (int k = 0; k < 36; ++k) h_cov36[k] = got[12 + k];
    return LVK_OK;
}
