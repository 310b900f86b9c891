// be_landmark_rel.hip — anchored inverse-depth landmarks in the camera frame of a target pose, with their first-order covariance
// (lvk_ekf_landmark_rel_cov, include/lvk_c.h).  Sigma = J P_s J^T, P_s the 19 x 19 sub-block of the filter's covariance over
// [extrinsics 15..20 | the anchor clone's six columns | the target's d_theta and d_p columns | the feature's column], J the 3 x 19
// derivative of p_c = R_b2c (R_b^T (p_w - p_b) - t_c_b) under the filter's own state injection (be_propagate.hip, lvk_ekf_inject).
#include "be_host.h"
#include <math.h>

#define LR_COLS 19
#define LR_OUT 12

// column of P behind entry k of the 19-vector [d_theta_e d_t | d_theta_a d_p_a | d_theta_b | d_p_b | d_rho]
__device__ __forceinline__ int lr_col(int k, int anchor_col, int bt, int bp, int feat_col)
{
    return k < 6 ? 15 + k : k < 12 ? anchor_col + (k - 6) : k < 15 ? bt + (k - 12) : k < 18 ? bp + (k - 15) : feat_col;
}

// Eigen's Quaternion::toRotationMatrix, q = [x y z w] (be_host_math.h, quat_to_rot)
__device__ __forceinline__ void lr_quat_to_rot(const double* q, double* R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy; R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// Eigen's Quaternion(Matrix3) (be_host_math.h, rot_to_quat); written out as in be_landmark.hip: no run-time index into a register array
__device__ __forceinline__ void lr_rot_to_quat(const double* M, double* qc)
{
    double t = M[0] + M[4] + M[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        qc[3] = 0.5 * t;
        t = 0.5 / t;
        qc[0] = (M[7] - M[5]) * t; qc[1] = (M[2] - M[6]) * t; qc[2] = (M[3] - M[1]) * t;
    } else {
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
}

// C = A B (row-major 3 x 3), every entry a 3-term inner product summed in order
__device__ __forceinline__ void lr_mm(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
// y = A x
__device__ __forceinline__ void lr_mv(const double* A, const double* x, double* y)
{
    for (int i = 0; i < 3; ++i) y[i] = A[i * 3] * x[0] + A[i * 3 + 1] * x[1] + A[i * 3 + 2] * x[2];
}

// One wavefront per job.  With R_a = R(q_anchor), R_b = R(q_b) (body to world), R_e = R_b2c, M = R_e R_b^T, the world vectors of
// k_landmark_cov - r_c = R_c2w [u v 1] / rho (R_c2w = R_a R_e^T through a quaternion and back), r = r_c + R_a t_c_b - and
//   g = p_w - p_b = r + (p_anchor - p_b)   (the difference of the two positions first: no world coordinate is added and taken away again),
//   y = R_b^T g - t_c_b,   p_c = R_e y,
// the injection's conventions give d p_w as in be_landmark.hip and
//   d p_c = (R_e [y]x - M [r_c]x R_a) d_theta_e + (M R_a - R_e) d_t - M [r]x d_theta_a + M d_p_a + M [g]x d_theta_b - M d_p_b - (M r_c / rho) d_rho
// ([r_c]x R_a = R_a [x]x with x = R_e^T [u v 1] / rho).  The lanes gather the 361 entries of P_s into LDS (nothing else of P is read;
// columns named twice - target == anchor - are simply gathered twice), lane 0 builds J and writes p_c, lanes 0..56 form T = J P_s one
// entry each, lanes 0..5 the six upper entries of T J^T - every sum runs over l = 0..18 in that order inside one lane - and each writes
// its mirror as well.
__global__ __launch_bounds__(64) void k_landmark_rel_cov(const double* __restrict__ P, int ld, const lvk_landmark_rel_job* __restrict__ jobs, int n_jobs, double* __restrict__ out)
{
    __shared__ double Ps[LR_COLS * LR_COLS], J[3 * LR_COLS], T[3 * LR_COLS];
    const int lane = threadIdx.x, job = blockIdx.x;
    if (job >= n_jobs) return;                          // (uniform over the workgroup)
    const lvk_landmark_rel_job* jb = jobs + job;
    const int anchor_col = jb->anchor_col, feat_col = jb->feat_col, bt = jb->b_theta_col, bp = jb->b_p_col;
    double* o = out + (size_t)job * LR_OUT;
    for (int t = lane; t < LR_COLS * LR_COLS; t += 64)
        Ps[t] = P[(size_t)lr_col(t / LR_COLS, anchor_col, bt, bp, feat_col) * ld + lr_col(t % LR_COLS, anchor_col, bt, bp, feat_col)];
    if (lane == 0) {
        double Ra[9], Rb[9], Re[9], Mc[9], qc[4], Rc[9];
        lr_quat_to_rot(jb->q_anchor, Ra);
        lr_quat_to_rot(jb->q_b, Rb);
        for (int i = 0; i < 9; ++i) Re[i] = jb->R_b2c[i];
        const double te[3] = {jb->t_c_b[0], jb->t_c_b[1], jb->t_c_b[2]};
        // the filter's own camera attitude (clone_refresh_cam): R(q) R_b2c^T through a quaternion and back, as k_landmark_cov takes it
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0.; for (int k = 0; k < 3; ++k) s += Ra[i * 3 + k] * Re[j * 3 + k]; Mc[i * 3 + j] = s; }
        lr_rot_to_quat(Mc, qc);
        lr_quat_to_rot(qc, Rc);
        const double rho = jb->inv_depth;
        const double fa[3] = {jb->obs_anchor[0] / rho, jb->obs_anchor[1] / rho, 1 / rho};
        double rc[3], rt[3], r[3], g[3];
        lr_mv(Rc, fa, rc);
        lr_mv(Ra, te, rt);
        for (int i = 0; i < 3; ++i) { r[i] = rc[i] + rt[i]; g[i] = r[i] + (jb->p_anchor[i] - jb->p_b[i]); }
        // M = R_e R_b^T;  y = R_b^T g - t_c_b;  p_c = R_e y
        double M[9], y[3], pc[3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0.; for (int k = 0; k < 3; ++k) s += Re[i * 3 + k] * Rb[j * 3 + k]; M[i * 3 + j] = s; }
        for (int i = 0; i < 3; ++i) y[i] = (Rb[i] * g[0] + Rb[3 + i] * g[1] + Rb[6 + i] * g[2]) - te[i];
        lr_mv(Re, y, pc);
        o[0] = pc[0]; o[1] = pc[1]; o[2] = pc[2];
        // -[v]x and [v]x, row-major
        const double Sc[9] = {0, rc[2], -rc[1], -rc[2], 0, rc[0], rc[1], -rc[0], 0};
        const double Sr[9] = {0, r[2], -r[1], -r[2], 0, r[0], r[1], -r[0], 0};
        const double Sg[9] = {0, -g[2], g[1], g[2], 0, -g[0], -g[1], g[0], 0};
        const double Sy[9] = {0, -y[2], y[1], y[2], 0, -y[0], -y[1], y[0], 0};
        double Ae[9], MAe[9], ReSy[9], MRa[9], MSr[9], MSg[9], mrc[3];
        lr_mm(Sc, Ra, Ae);                              // -[r_c]x R_a, the d_theta_e block of d p_w
        lr_mm(M, Ae, MAe);
        lr_mm(Re, Sy, ReSy);
        lr_mm(M, Ra, MRa);
        lr_mm(M, Sr, MSr);
        lr_mm(M, Sg, MSg);
        lr_mv(M, rc, mrc);
        for (int i = 0; i < 3; ++i) {
            for (int c = 0; c < 3; ++c) {
                const int e = i * 3 + c;
                J[i * LR_COLS + c] = ReSy[e] + MAe[e];
                J[i * LR_COLS + 3 + c] = MRa[e] - Re[e];
                J[i * LR_COLS + 6 + c] = MSr[e];
                J[i * LR_COLS + 9 + c] = M[e];
                J[i * LR_COLS + 12 + c] = MSg[e];
                J[i * LR_COLS + 15 + c] = -M[e];
            }
            J[i * LR_COLS + 18] = -(mrc[i] / rho);
        }
    }
    __syncthreads();
    if (lane < 3 * LR_COLS) {
        const int i = lane / LR_COLS, j = lane % LR_COLS;
        double s = 0.;
        for (int l = 0; l < LR_COLS; ++l) s += J[i * LR_COLS + l] * Ps[l * LR_COLS + j];
        T[lane] = s;
    }
    __syncthreads();
    if (lane < 6) {
        const int i = lane < 3 ? 0 : lane < 5 ? 1 : 2, j = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
        double s = 0.;
        for (int l = 0; l < LR_COLS; ++l) s += T[i * LR_COLS + l] * J[j * LR_COLS + l];
        o[3 + i * 3 + j] = s;
        if (i != j) o[3 + j * 3 + i] = s;
    }
}

// what the kernel assumes of one job on an n x n covariance: every column it names lies in [0, n) and the depth is not zero
bool lvk_landmark_rel_job_ok(const lvk_landmark_rel_job* j, int n)
{
    const auto fits = [n](int c, int w) { return c >= 0 && c <= n - w; };
    return n >= 21 && fits(j->anchor_col, 6) && fits(j->b_theta_col, 3) && fits(j->b_p_col, 3) && fits(j->feat_col, 1) && j->inv_depth != 0.0;
}

lvk_status lvk_launch_landmark_rel_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_landmark_rel_job* d_jobs, int n_jobs, double* d_out12)
{
    if (n_jobs <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_landmark_rel_cov, dim3(n_jobs), dim3(64), 0, ctx->stream, d_P, ldp, d_jobs, n_jobs, d_out12);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// (C ABI) jobs go up in the stage's input blob, the results come back through its output blob; one wait per call
extern "C" lvk_status lvk_ekf_landmark_rel_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_landmark_rel_job* h_jobs, int n_jobs, double* h_out12)
{
    if (!ctx || !d_P || !h_jobs || !h_out12 || n_jobs < 0 || ldp < n)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_landmark_rel_cov: bad argument");
    for (int k = 0; k < n_jobs; ++k)
        if (!lvk_landmark_rel_job_ok(h_jobs + k, n))
            return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_landmark_rel_cov: job %d (anchor columns %d..%d, target columns %d.. / %d.., feature column %d, inverse depth %g) does not fit a %d x %d covariance",
                                 k, h_jobs[k].anchor_col, h_jobs[k].anchor_col + 5, h_jobs[k].b_theta_col, h_jobs[k].b_p_col, h_jobs[k].feat_col, h_jobs[k].inv_depth, n, n);
    if (n_jobs == 0) return LVK_OK;
    const size_t jbytes = sizeof(lvk_landmark_rel_job) * (size_t)n_jobs, obytes = sizeof(double) * LR_OUT * (size_t)n_jobs;
    Stage sg(ctx);
    const size_t o_jobs = sg.take(Stage::IN, jbytes), o_out = sg.take(Stage::OUT, obytes);
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_jobs, h_jobs, jbytes));
    LVK_TRY(lvk_launch_landmark_rel_cov(ctx, d_P, ldp, sg.at<lvk_landmark_rel_job>(Stage::IN, o_jobs), n_jobs, sg.at<double>(Stage::OUT, o_out)));
    LVK_TRY(sg.get(h_out12, Stage::OUT, o_out, obytes));
    return sg.wait();
}
