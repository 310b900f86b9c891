// backend.hip — the frame-level back-end object of liblvk_hip.so: lvk_ekf_process replaces
// LarVio::processFeatures (/root/reference/src/larvio.cpp:363-461).
//
// Split of labour.  The HOST keeps what is pointer-chasing bookkeeping in the reference — the feature map with
// its per-clone observations (feature.hpp:34-250), the clone list, triage of lost / long / in-state features
// (larvio.cpp:1897-2005), key-frame selection (:2259-2307) — and the 22-dimensional IMU state integration.
// The DEVICE keeps the covariance P resident in HBM (fixed leading dimension, logical N) and does every
// O(N^2)/O(N^3) operation and every per-feature numerical block: covariance propagation with the frame's
// composed transition matrix, clone augmentation / deletion as index gathers, LM triangulation (one wavefront
// per feature), Jacobians + null-space projection + chi-square gate (one workgroup per feature, compact columns),
// row stacking, Householder compression, and the FP64-MFMA update.  feature_idp_dim = 1, use_schmidt = 0,
// calib_imu = 0 or 1 (LEG_DIM 22 / 46) — config/euroc.yaml:8-10,105,108 and its calibration variant; anything else is refused.
// The filter object and the helpers its files share are in be_filter.h; the exports beside the state (drain lists, covariance
// getters) are in be_export.hip, the pipelined driver in be_pipe.hip.
#include "be_filter.h"
#include "be_host_math.h"
#include "be_init.h"
#include <new>
#include <float.h>
#include <sched.h>
#include <pthread.h>

#define GRAV 9.81

// ------------------------------------------------------------------------- host-side phase tracer (LVK_EKF_TRACE=1)
#include <chrono>
enum { TR_IMU, TR_PROP, TR_FETCH, TR_ADDOBS, TR_ZUPT, TR_RLF_PRE, TR_RLF_TRI, TR_RLF_TRIAGE, TR_RLF_ROWS, TR_RLF_UPD, TR_RLF_DX, TR_RLF_INJ,
       TR_PR_PRE, TR_PR_TRI, TR_PR_ROWS, TR_PR_UPD, TR_PR_DX, TR_PR_END, TR_FINAL, TR_N };
static const char* const TR_NAMES[TR_N] = {"batch_imu", "propagate+augment(launch)", "message fetch (front-end wait)", "add_obs", "zupt_check", "lost:prepare", "lost:triangulate+sync",
    "lost:triage+jobs", "lost:rows+sync", "lost:stack+update(launch)", "lost:dx sync", "lost:inject", "prune:prepare(+reanchor)", "prune:triangulate+sync",
    "prune:rows+sync", "prune:update(launch)", "prune:dx sync", "prune:inject+delete", "final sync"};
struct EkfTrace {
    bool on = false; double acc[TR_N] = {0}; long n = 0;
    double sub_acc[8] = {0}; std::chrono::steady_clock::time_point last_sub; long cnt[4] = {0, 0, 0, 0};      // cnt: updates above 160 rows / plans drawn up / compressions taken / rows of those updates      // finer marks inside one phase (TRS): time since the previous mark of either kind
    double cur[TR_N] = {0};                              // this update's phases: an update above LVK_EKF_TRACE_SLOW_US is printed on its own
    std::chrono::steady_clock::time_point last;
    void start() { if (on) { last = last_sub = std::chrono::steady_clock::now(); for (int i = 0; i < TR_N; ++i) cur[i] = 0; } }
    void mark(int slot) { if (!on) return; auto t = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double, std::micro>(t - last).count(); acc[slot] += d; cur[slot] += d; last = t; last_sub = t; }
    void sub(int k) { if (!on) return; auto t = std::chrono::steady_clock::now(); sub_acc[k] += std::chrono::duration<double, std::micro>(t - last_sub).count(); last_sub = t; }
    void end_update(const char* const* names)
    {
        static const double slow = [] { const char* v = getenv("LVK_EKF_TRACE_SLOW_US"); return v ? atof(v) : 0.0; }();
        if (!on || slow <= 0) return;
        double tot = 0; for (int i = 0; i < TR_N; ++i) tot += cur[i];
        if (tot < slow) return;
        fprintf(stderr, "[lvk_ekf trace] slow update %ld: %.0f us:", n, tot);
        for (int i = 0; i < TR_N; ++i) if (cur[i] > 0.02 * tot) fprintf(stderr, " %s %.0f;", names[i], cur[i]);
        fprintf(stderr, "\n");
    }
};
static EkfTrace g_tr;
#define TR(slot) g_tr.mark(slot)
#define TRS(k) g_tr.sub(k)
static const char* const TRS_NAMES[8] = {"update w/o new feature: jobs staged (launch_feature_rows)", "  row slots + groups (push_rows)", "  uploads flushed, row kernel launched (end_defer)",
    "  compression planned / launched", "  update core launched (4 kernels)", "batch_imu: (unused)", "(unused)", "(unused)"};

// ------------------------------------------------------------------------- small helpers
// R(q_cam) of clone `rank`: checkMotion (feature.hpp:334-381) asks for it twice per feature, thousands of times per update at
// configs[4]; the clones' poses only change at state injection and when the window changes
static const double* clone_Rcam(const lvk_ekf* e, int rank)
{
    if (!e->rcam_valid || e->rcam.size() != 9 * e->clones.size()) {
        e->rcam.resize(9 * e->clones.size());
        for (size_t i = 0; i < e->clones.size(); ++i) quat_to_rot(e->clones[i].q_cam, &e->rcam[9 * i]);
        e->rcam_valid = true;
    }
    return &e->rcam[9 * (size_t)rank];
}
static void clone_refresh_cam(const lvk_ekf* e, Clone* c)
{   // larvio.cpp:1529-1541
    double R_c2b[9], R_b2w[9], R_c2w[9], t[3];
    m3_t(e->R_b2c, R_c2b); quat_to_rot(c->q, R_b2w); m3_mul(R_b2w, R_c2b, R_c2w);
    rot_to_quat(R_c2w, c->q_cam);
    m3_v(R_b2w, e->t_c_b, t);
    for (int i = 0; i < 3; ++i) c->p_cam[i] = c->p[i] + t[i];
}
static void begin_defer(lvk_ekf* e) { e->defer += 1; }
static lvk_status end_defer(lvk_ekf* e)
{
    if (--e->defer > 0) return LVK_OK;
    lvk_status st = flush_uploads(e);
    for (auto& fn : e->deferred) if (st == LVK_OK) st = fn();
    e->deferred.clear();
    return st;
}
// The factorisation of S = H P H^T + sigma^2 I reports into device-mapped words (be_linalg.hip): a non-positive pivot means the
// covariance has lost positive definiteness - the reference's pivoted LDLT (larvio.cpp:1456) would go on with an indefinite S and
// produce a state nobody should fly on; here, by default, the update fails and the failure is sticky (ekf_process_guarded).  Under
// LVK_INDEFINITE_LDLT the update is run again through that pivoted LDLT instead (be_ldlt.hip) - the failed one has written neither P
// nor dx - and the call goes on.  Called after a stream sync that covers the update.
static lvk_status update_health(lvk_ekf* e)
{
    int* w = (int*)(e->h_down + e->down_info);
    if (w[0] == 0 && w[1] == 0) return LVK_OK;
    const int piv = w[0], gave_up = w[1]; w[0] = 0; w[1] = 0;
    EKF_HIP(hipMemsetAsync(e->ws.info, 0, 64, e->ctx->stream));
    // (last.n == N always holds here - every caller syncs before it changes N; were it ever not so, the default applies.  A system of more
    // rows than the factor kernel's LDS holds - m > ~1100, beyond what the filter's row capacity allows at the supported window sizes -
    // ends in LVK_ERR_CAPACITY from lvk_update_ldlt_core: lvk_c.h says both.)
    if (!gave_up && e->indefinite_policy == LVK_INDEFINITE_LDLT && e->last.m > 0 && e->last.n == e->N) {
        // the reference's route (larvio.cpp:1456): P and dx are as they were before the failed update; this one update again, pivoted
        UpdateWs ws = e->ws; ws.dx_host = (double*)(e->dh_down + e->down_dx);
        int* d_cnt = nullptr;
        lvk_status st = lvk_update_ldlt_core(e->ctx, e->dP[e->cur], e->ld, e->N, e->last.H, e->ld, e->last.m, e->last.r, e->sigma2, e->d_dx, ws, &d_cnt, nullptr);
        if (st == LVK_OK && e->redo) st = e->redo();
        if (st != LVK_OK) return st;
        EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
        e->p00_valid = false; e->fell_back = true; e->indefinite_fallbacks++;
        return LVK_OK;
    }
    if (gave_up) return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "measurement update: a solver workgroup waited for panel %d of the factorisation in vain", gave_up);
    return lvk_set_error(e->ctx, LVK_ERR_NUMERIC, "measurement update: the innovation covariance is not positive definite (pivot %d of %ld rows) - the filter has diverged", piv - 1, e->counters[2]);
}
static lvk_status d2h_sync(lvk_ekf* e, void* dst, const void* src, size_t bytes)
{
    if (bytes) EKF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->ctx->stream));
    EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
    if (e->shard.fn) { int* f = (int*)(e->h_down + e->down_flag); if (*f) { const int mask = *f; *f = 0; return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "sharded update: the block of a peer rank (mask 0x%x) arrived invalid - that rank failed before the exchange", mask); } }
    e->fell_back = false;
    lvk_status hs = update_health(e);
    if (hs == LVK_OK && e->fell_back && bytes) {        // the copy above was queued behind the update that failed: fetch what the pivoted one wrote
        EKF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->ctx->stream));
        EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
    }
    return hs;
}
// P <- P[idx, idx] (ping-pong)
static lvk_status cov_gather(lvk_ekf* e, const std::vector<int>& idx)
{
    int* h = up_alloc<int>(e, idx.size());
    if (!h) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memcpy(h, idx.data(), sizeof(int) * idx.size());
    double* src = e->dP[e->cur]; double* dst = e->dP[e->cur ^ 1];
    const int* d_idx = dev(e, h); const int n = (int)idx.size();
    lvk_status st = run_or_defer(e, [=]() { return lvk_cov_gather(e->ctx, src, e->ld, dst, e->ld, d_idx, n); });
    if (st != LVK_OK) return st;
    e->cur ^= 1; e->N = n;
    return LVK_OK;
}
// P loses the rows / columns marked in drop (N flags)
static lvk_status cov_drop(lvk_ekf* e, const std::vector<char>& drop)
{
    std::vector<int> idx; idx.reserve(e->N);
    for (int i = 0; i < e->N; ++i) if (!drop[i]) idx.push_back(i);
    return cov_gather(e, idx);
}
static lvk_status cov_delete(lvk_ekf* e, int start, int len)
{
    std::vector<int> idx; idx.reserve(e->N);
    for (int i = 0; i < e->N; ++i) if (i < start || i >= start + len) idx.push_back(i);
    return cov_gather(e, idx);
}

// ------------------------------------------------------------------------- propagation (host state, composed Phi for the device)
static void predict_new_state(lvk_ekf* e, double dt, const double* gyro, const double* acc)
{   // larvio.cpp:581-649
    const double gn = v3_norm(gyro);
    double Om[16] = {0}, S[9]; skew3(gyro, S);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Om[i * 4 + j] = -S[i * 3 + j]; Om[i * 4 + 3] = gyro[i]; Om[12 + i] = -gyro[i]; }
    e->s_old = e->s;
    double* q = e->s.q; double* v = e->s.v; double* p = e->s.p;
    double dq[4], dq2[4];
    for (int half = 0; half < 2; ++half) {
        double* o = half ? dq2 : dq;
        const double ang = half ? gn * dt * 0.25 : gn * dt * 0.5;
        double M[16];
        if (gn > 1e-5) { const double c = cos(ang), s = 1 / gn * sin(ang); for (int i = 0; i < 16; ++i) M[i] = c * ((i % 5 == 0) ? 1.0 : 0.0) + s * Om[i]; }
        else { const double f = half ? 0.25 * dt : 0.5 * dt, c = cos(ang); for (int i = 0; i < 16; ++i) M[i] = (((i % 5 == 0) ? 1.0 : 0.0) + f * Om[i]) * c; }
        for (int i = 0; i < 4; ++i) { double a = 0; for (int k = 0; k < 4; ++k) a += M[i * 4 + k] * q[k]; o[i] = a; }
    }
    double Rdt[9], Rdt2[9], R0[9];
    quat_to_rot(dq, Rdt); quat_to_rot(dq2, Rdt2); quat_to_rot(q, R0);
    const double g[3] = {0, 0, -GRAV};
    double k1v[3], k2v[3], k3v[3], k4v[3], k1p[3], k2p[3], k3p[3], k4p[3], t1[3], t2[3], k1_v[3], k2_v[3], k3_v[3];
    m3_v(R0, acc, t1); for (int i = 0; i < 3; ++i) { k1v[i] = t1[i] + g[i]; k1p[i] = v[i]; k1_v[i] = v[i] + k1v[i] * dt / 2; }
    m3_v(Rdt2, acc, t2); for (int i = 0; i < 3; ++i) { k2v[i] = t2[i] + g[i]; k2p[i] = k1_v[i]; k2_v[i] = v[i] + k2v[i] * dt / 2; }
    for (int i = 0; i < 3; ++i) { k3v[i] = t2[i] + g[i]; k3p[i] = k2_v[i]; k3_v[i] = v[i] + k3v[i] * dt; }
    m3_v(Rdt, acc, t1); for (int i = 0; i < 3; ++i) { k4v[i] = t1[i] + g[i]; k4p[i] = k3_v[i]; }
    const double n = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int i = 0; i < 4; ++i) q[i] = dq[i] / n;
    for (int i = 0; i < 3; ++i) {
        double nv = v[i] + dt / 6 * (k1v[i] + 2 * k2v[i] + 2 * k3v[i] + k4v[i]);
        double np = p[i] + dt / 6 * (k1p[i] + 2 * k2p[i] + 2 * k3p[i] + k4p[i]);
        v[i] = nv; p[i] = np;
    }
    e->s_fej_old = e->s_fej_now; e->s_fej_now = e->s;
}

static void cal_phi(const lvk_ekf* e, double* Phi, double dt, const double* gyro, const double* gyro_old)
{   // larvio.cpp:3475-3530 with Ma = Tg = I, As = 0 (calib_imu = 0)
    double cr[3] = {gyro_old[1] * gyro[2] - gyro_old[2] * gyro[1], gyro_old[2] * gyro[0] - gyro_old[0] * gyro[2], gyro_old[0] * gyro[1] - gyro_old[1] * gyro[0]};
    double aa[3]; for (int i = 0; i < 3; ++i) aa[i] = dt * (gyro_old[i] + gyro[i]) / 2 + dt * dt * cr[i] / 12;
    double Ah[9]; skew3(aa, Ah);
    double C[9]; quat_to_rot(e->s_old.q, C);
    memset(Phi, 0, sizeof(double) * LEG * LEG);
    for (int i = 0; i < LEG; ++i) Phi[i * (LEG + 1)] = 1.0;
    const ImuS* so = e->if_fej ? &e->s_fej_old : &e->s_old;
    const ImuS* sn = e->if_fej ? &e->s_fej_now : &e->s;
    const double *vk = so->v, *pk = so->p, *vk1 = sn->v, *pk1 = sn->p;
    const double g[3] = {0, 0, -GRAV};
    double I2A[9]; for (int i = 0; i < 9; ++i) I2A[i] = 2 * ((i % 4 == 0) ? 1.0 : 0.0) + Ah[i];
    double CI2A[9]; m3_mul(C, I2A, CI2A);
#define BLK(r, c, M, sc) for (int i_ = 0; i_ < 3; ++i_) for (int j_ = 0; j_ < 3; ++j_) Phi[((r) + i_) * LEG + (c) + j_] = (sc) * (M)[i_ * 3 + j_]
    { double M[9]; for (int i = 0; i < 9; ++i) M[i] = -0.5 * CI2A[i] * dt; BLK(0, 9, M, 1.0); }
    { double Z[9] = {0}; BLK(0, 12, Z, 1.0); }
    { double a[3], S[9]; for (int i = 0; i < 3; ++i) a[i] = vk1[i] - vk[i] - g[i] * dt; skew3(a, S); BLK(3, 0, S, -1.0); }
    { double a[3], b[3], S1[9], S2[9], T1[9], T2[9], T3[9], M[9];
      for (int i = 0; i < 3; ++i) { a[i] = -pk1[i] + pk[i] + vk1[i] * dt - 0.5 * g[i] * dt * dt; b[i] = -0.5 * pk1[i] + 0.5 * pk[i] + 0.5 * vk1[i] * dt - g[i] * dt * dt / 6; }
      skew3(a, S1); skew3(b, S2); m3_mul(S1, C, T1); m3_mul(S2, C, T2); m3_mul(T2, Ah, T3);
      for (int i = 0; i < 9; ++i) M[i] = T1[i] + T3[i];
      BLK(3, 9, M, 1.0); }
    { double M[9]; for (int i = 0; i < 9; ++i) M[i] = -0.5 * CI2A[i] * dt - 0.0; BLK(3, 12, M, 1.0); }
    { double a[3], S[9]; for (int i = 0; i < 3; ++i) a[i] = pk1[i] - pk[i] - vk[i] * dt - 0.5 * g[i] * dt * dt; skew3(a, S); BLK(6, 0, S, -1.0); }
    { double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; BLK(6, 3, I, dt); }
    { double Sg[9], T1[9], a[3], S2[9], T2[9], T3[9], M[9];
      skew3(g, Sg); m3_mul(Sg, C, T1);
      for (int i = 0; i < 3; ++i) a[i] = pk1[i] - pk[i] - g[i] * dt * dt / 6;
      skew3(a, S2); m3_mul(S2, C, T2); m3_mul(T2, Ah, T3);
      for (int i = 0; i < 9; ++i) M[i] = -dt * dt * dt * T1[i] / 6 + dt * T3[i] / 4;
      BLK(6, 9, M, 1.0); }
    { double I3A[9], T[9], M[9]; for (int i = 0; i < 9; ++i) I3A[i] = 3 * ((i % 4 == 0) ? 1.0 : 0.0) + Ah[i];
      m3_mul(C, I3A, T); for (int i = 0; i < 9; ++i) M[i] = -T[i] * dt * dt / 6; BLK(6, 12, M, 1.0); }
#undef BLK
}

static void update_imu_mx(lvk_ekf* e)
{   // larvio.cpp:3803-3846
    const double *T1 = e->imx, *T2 = e->imx + 3, *T3 = e->imx + 6, *A1 = e->imx + 9, *A2 = e->imx + 12, *A3 = e->imx + 15, *M1 = e->imx + 18, *M2 = e->imx + 21;
    double* Tg = e->Tg; double* As = e->As; double* Ma = e->Ma;
    Tg[0] = T2[0]; Tg[1] = T3[0]; Tg[2] = T3[1]; Tg[3] = T1[0]; Tg[4] = T2[1]; Tg[5] = T3[2]; Tg[6] = T1[1]; Tg[7] = T1[2]; Tg[8] = T2[2];
    As[0] = A2[0]; As[1] = A3[0]; As[2] = A3[1]; As[3] = A1[0]; As[4] = A2[1]; As[5] = A3[2]; As[6] = A1[1]; As[7] = A1[2]; As[8] = A2[2];
    Ma[0] = M2[0]; Ma[1] = 0; Ma[2] = 0; Ma[3] = M1[0]; Ma[4] = M2[1]; Ma[5] = 0; Ma[6] = M1[1]; Ma[7] = M1[2]; Ma[8] = M2[2];
}

// calPhi for calib_imu = 1 (larvio.cpp:3475-3800): Tg / Tg As / Ma enter the bias columns, and 24 columns are added for the
// intrinsic parameters.  Every extra 3x3 block follows one recipe per parameter group (T1-T3: gyro matrix, A1-A3: g-sensitivity,
// M1-M2: accelerometer matrix): Simpson-weighted sensitivity of the rotation (RX), then of the velocity (fRX), then of the
// position, built from strictly-lower / diagonal / strictly-upper patterns of w, acc or f at t_k, the midpoint and t_k+1.
static void imx_pattern(int kind, const double* v, double* M)
{
    for (int i = 0; i < 9; ++i) M[i] = 0;
    if (kind == 0) { M[3] = v[0]; M[7] = v[0]; M[8] = v[1]; }          // d(X v)/d(lower entries (1,0) (2,0) (2,1))
    else if (kind == 1) { M[0] = v[0]; M[4] = v[1]; M[8] = v[2]; }     // d/d(diagonal)
    else { M[0] = v[1]; M[1] = v[2]; M[5] = v[2]; }                    // d/d(upper entries (0,1) (0,2) (1,2))
}
static void cal_phi_calib(const lvk_ekf* e, double* Phi, double dt, const double* f, const double* w, const double* acc, const double* gyro,
                          const double* f_old, const double* w_old, const double* acc_old, const double* gyro_old)
{
    const int L = e->leg;
    double f_mid[3], acc_mid[3], w_mid[3];
    const double cw[3] = {w_old[1] * w[2] - w_old[2] * w[1], w_old[2] * w[0] - w_old[0] * w[2], w_old[0] * w[1] - w_old[1] * w[0]};
    for (int i = 0; i < 3; ++i) { f_mid[i] = (f[i] + f_old[i]) / 2; acc_mid[i] = (acc[i] + acc_old[i]) / 2; w_mid[i] = (w_old[i] + w[i]) / 2 + dt * cw[i] / 12; }
    const double cr[3] = {gyro_old[1] * gyro[2] - gyro_old[2] * gyro[1], gyro_old[2] * gyro[0] - gyro_old[0] * gyro[2], gyro_old[0] * gyro[1] - gyro_old[1] * gyro[0]};
    double aa[3]; for (int i = 0; i < 3; ++i) aa[i] = dt * (gyro_old[i] + gyro[i]) / 2 + dt * dt * cr[i] / 12;
    double Ah[9]; skew3(aa, Ah);
    double C[9]; quat_to_rot(e->s_old.q, C);
    memset(Phi, 0, sizeof(double) * L * L);
    for (int i = 0; i < L; ++i) Phi[i * (L + 1)] = 1.0;
    double TA[9], TAMa[9]; m3_mul(e->Tg, e->As, TA); m3_mul(TA, e->Ma, TAMa);
    const ImuS* so = e->if_fej ? &e->s_fej_old : &e->s_old;
    const ImuS* sn = e->if_fej ? &e->s_fej_now : &e->s;
    const double *vk = so->v, *pk = so->p, *vk1 = sn->v, *pk1 = sn->p;
    const double g[3] = {0, 0, -GRAV};
    double I2A[9]; for (int i = 0; i < 9; ++i) I2A[i] = 2 * ((i % 4 == 0) ? 1.0 : 0.0) + Ah[i];
    double CI2A[9]; m3_mul(C, I2A, CI2A);
#define BLK(r, c, M, sc) for (int i_ = 0; i_ < 3; ++i_) for (int j_ = 0; j_ < 3; ++j_) Phi[((r) + i_) * L + (c) + j_] = (sc) * (M)[i_ * 3 + j_]
    { double M[9], T[9]; for (int i = 0; i < 9; ++i) M[i] = -0.5 * CI2A[i] * dt; m3_mul(M, e->Tg, T); BLK(0, 9, T, 1.0); }
    { double M[9], T[9]; for (int i = 0; i < 9; ++i) M[i] = 0.5 * CI2A[i] * dt; m3_mul(M, TAMa, T); BLK(0, 12, T, 1.0); }
    { double a[3], S[9]; for (int i = 0; i < 3; ++i) a[i] = vk1[i] - vk[i] - g[i] * dt; skew3(a, S); BLK(3, 0, S, -1.0); }
    double Pvbg[9], Ppbg[9];
    { double a[3], b[3], S1[9], S2[9], T1[9], T2[9], T3[9];
      for (int i = 0; i < 3; ++i) { a[i] = -pk1[i] + pk[i] + vk1[i] * dt - 0.5 * g[i] * dt * dt; b[i] = -0.5 * pk1[i] + 0.5 * pk[i] + 0.5 * vk1[i] * dt - g[i] * dt * dt / 6; }
      skew3(a, S1); skew3(b, S2); m3_mul(S1, C, T1); m3_mul(S2, C, T2); m3_mul(T2, Ah, T3);
      for (int i = 0; i < 9; ++i) Pvbg[i] = T1[i] + T3[i];
      BLK(3, 9, Pvbg, 1.0); }
    { double M[9], T1[9], T2[9]; for (int i = 0; i < 9; ++i) M[i] = -0.5 * CI2A[i] * dt; m3_mul(M, e->Ma, T1); m3_mul(Pvbg, TAMa, T2);
      for (int i = 0; i < 9; ++i) M[i] = T1[i] - T2[i]; BLK(3, 12, M, 1.0); }
    { double a[3], S[9]; for (int i = 0; i < 3; ++i) a[i] = pk1[i] - pk[i] - vk[i] * dt - 0.5 * g[i] * dt * dt; skew3(a, S); BLK(6, 0, S, -1.0); }
    { double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; BLK(6, 3, I, dt); }
    { double Sg[9], T1[9], a[3], S2[9], T2[9], T3[9];
      skew3(g, Sg); m3_mul(Sg, C, T1);
      for (int i = 0; i < 3; ++i) a[i] = pk1[i] - pk[i] - g[i] * dt * dt / 6;
      skew3(a, S2); m3_mul(S2, C, T2); m3_mul(T2, Ah, T3);
      for (int i = 0; i < 9; ++i) Ppbg[i] = -dt * dt * dt * T1[i] / 6 + dt * T3[i] / 4;
      BLK(6, 9, Ppbg, 1.0); }
    { double I3A[9], T[9], M[9], T1[9], T2[9]; for (int i = 0; i < 9; ++i) I3A[i] = 3 * ((i % 4 == 0) ? 1.0 : 0.0) + Ah[i];
      m3_mul(C, I3A, T); for (int i = 0; i < 9; ++i) M[i] = -T[i] * dt * dt / 6; m3_mul(M, e->Ma, T1); m3_mul(Ppbg, TAMa, T2);
      for (int i = 0; i < 9; ++i) M[i] = T1[i] - T2[i]; BLK(6, 12, M, 1.0); }
    double R_mid[9], R_kp1[9];
    for (int i = 0; i < 9; ++i) { const double id = (i % 4 == 0) ? 1.0 : 0.0; R_mid[i] = id + 0.5 * Ah[i]; R_kp1[i] = id + Ah[i]; }
    double ram[3], rka[3], Sm[9], Sk[9];
    m3_v(R_mid, acc_mid, ram); m3_v(R_kp1, acc, rka); skew3(ram, Sm); skew3(rka, Sk);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    struct Grp { int col, kind; const double *a, *m, *b; const double* Pm; bool has_f; double sq, sv; };
    const Grp grp[8] = {
        {22, 0, w_old, w_mid, w, I3, false, 1.0, -1.0}, {25, 1, w_old, w_mid, w, I3, false, 1.0, -1.0}, {28, 2, w_old, w_mid, w, I3, false, 1.0, -1.0},
        {31, 0, acc_old, acc_mid, acc, e->Tg, false, -1.0, 1.0}, {34, 1, acc_old, acc_mid, acc, e->Tg, false, -1.0, 1.0}, {37, 2, acc_old, acc_mid, acc, e->Tg, false, -1.0, 1.0},
        {40, 0, f_old, f_mid, f, TA, true, -1.0, 1.0}, {43, 1, f_old, f_mid, f, TA, true, -1.0, 1.0}};
    for (const Grp& gq : grp) {
        double Xk[9], Xm[9], Xp[9], kq1[9], kq2[9], kq4[9], T[9], RX[9];
        imx_pattern(gq.kind, gq.a, Xk); imx_pattern(gq.kind, gq.m, Xm); imx_pattern(gq.kind, gq.b, Xp);
        m3_mul(gq.Pm, Xk, kq1);
        m3_mul(gq.Pm, Xm, T); m3_mul(R_mid, T, kq2);
        m3_mul(gq.Pm, Xp, T); m3_mul(R_kp1, T, kq4);
        for (int i = 0; i < 9; ++i) RX[i] = dt * (kq1[i] + 4 * kq2[i] + kq4[i]) / 6;
        m3_mul(C, RX, T); BLK(0, gq.col, T, gq.sq);
        double kv1[9], kv2[9], kv3[9], kv4[9], A[9], fRX[9];
        for (int i = 0; i < 9; ++i) kv1[i] = gq.has_f ? Xk[i] : 0.0;
        m3_mul(Sm, kq1, A); for (int i = 0; i < 9; ++i) kv2[i] = A[i] * dt / 2;
        m3_mul(Sm, kq2, A); for (int i = 0; i < 9; ++i) kv3[i] = A[i] * dt / 2;
        m3_mul(Sk, RX, kv4);
        if (gq.has_f) {
            double RF[9];
            m3_mul(R_mid, Xm, RF); for (int i = 0; i < 9; ++i) { kv2[i] += RF[i]; kv3[i] += RF[i]; }
            m3_mul(R_kp1, Xp, RF); for (int i = 0; i < 9; ++i) kv4[i] += RF[i];
        }
        for (int i = 0; i < 9; ++i) fRX[i] = dt * (kv1[i] + 2 * kv2[i] + 2 * kv3[i] + kv4[i]) / 6;
        m3_mul(C, fRX, T); BLK(3, gq.col, T, gq.sv);
        double kp[9];
        for (int i = 0; i < 9; ++i) kp[i] = dt * (2 * (dt * kv1[i] / 2) + 2 * (dt * kv2[i] / 2) + fRX[i]) / 6;
        m3_mul(C, kp, T); BLK(6, gq.col, T, gq.sv);
    }
#undef BLK
}

// Phi_tot <- Phi Phi_tot ; Q_tot <- Phi Q_tot Phi^T + Q for one IMU sample, with the legacy dimension as a compile-time constant
// (22, or 46 when the IMU intrinsics are calibrated) so that the short fixed-length loops unroll and vectorise.
#ifndef LVK_COMPOSE_TIMING
#define CT_DECL do { } while (0)
#define CT(k) do { } while (0)
#endif
template <int L, bool CALIB>
static void compose_transition(lvk_ekf* e, const double* Phi, double dtime)
{
    CT_DECL;
    double C[9]; quat_to_rot(e->s_old.q, C);
    double G[15 * 12]; memset(G, 0, sizeof G);                      // rows 15.. of G are zero
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { G[i * 12 + j] = -C[i * 3 + j]; G[(3 + i) * 12 + 3 + j] = -C[i * 3 + j]; }
    for (int i = 0; i < 3; ++i) { G[(9 + i) * 12 + 6 + i] = 1.0; G[(12 + i) * 12 + 9 + i] = 1.0; }
    // Structure of the discrete model: rows 9.. of Phi are identity rows; rows 0..8 (q, v, p) are zero outside the columns of
    // q, v, p, bg, ba (0..14) and, when calibrating, the 24 intrinsic columns (22..45).  G is zero below row 14.  Skipping the
    // exact-zero products leaves every sum identical to the dense triple loops and cuts the per-sample host work several times.
    constexpr int A = 9, B = 15, NNZ = CALIB ? 39 : 15;
    int nzc[NNZ];                                                   // columns where rows 0..8 of Phi may be non-zero
    for (int k = 0; k < 15; ++k) nzc[k] = k;
    if (CALIB) for (int k = 22; k < 46; ++k) nzc[15 + k - 22] = k;
    constexpr int nnz = NNZ;
    // Every sum below runs over its summation index in ascending order, one element at a time, exactly as the plain triple loops
    // would; the loops are only nested so that the innermost one walks independent output elements (it vectorises, the dependent
    // scalar reductions it replaced did not).  Round 6: terms whose factor is an EXACT zero are not formed at all - of the 9 x 15 block of
    // Phi that differs from the identity only ~70 entries are non-zero (skew-symmetric blocks, dt I, the identity's own diagonal; without
    // calibration the theta-row's accelerometer-bias block is zero as a whole), G has two 3 x 3 blocks and six ones, and the rows 9..14 of
    // Phi G are unit rows.  A sum without its zero terms is the same double (x + 0 = x); tests/host/imu_compose_check.hip holds this
    // function to the dense recurrences bit for bit.  The IMU batch is host work on the filter's critical path (the GPU idles through it
    // between two messages): 16.6 -> ~9 us per message of 20 samples.
    // ---- the non-zeros of Phi's rows 0..8 (ascending column order per row, as (column slot q, value)); column lists for the right product
    int rz_q[A][NNZ]; int rz_n[A];
    for (int i = 0; i < A; ++i) { int n = 0; for (int q = 0; q < nnz; ++q) if (Phi[i * L + nzc[q]] != 0.0) rz_q[i][n++] = q; rz_n[i] = n; }
    CT(0);
    double PG[B * 12], PGT[12 * B], Q[B * B], PhiT[NNZ * 12];
    for (int q = 0; q < nnz; ++q) { for (int j = 0; j < A; ++j) PhiT[q * 12 + j] = Phi[j * L + nzc[q]]; PhiT[q * 12 + 9] = PhiT[q * 12 + 10] = PhiT[q * 12 + 11] = 0.0; }
    // PG = Phi G (rows 0..8; rows 9..14 of Phi are identity rows: PG = G there).  G: -C in (0..2, 0..2) and (3..5, 3..5), ones at (9+i, 6+i), (12+i, 9+i)
    for (int i = 0; i < A; ++i) {
        double* pg = PG + i * 12;
        for (int j = 0; j < 3; ++j) {
            double s0 = 0, s1 = 0;
            for (int k = 0; k < 3; ++k) { s0 += Phi[i * L + k] * G[k * 12 + j]; s1 += Phi[i * L + 3 + k] * G[(3 + k) * 12 + 3 + j]; }
            pg[j] = s0; pg[3 + j] = s1;
            pg[6 + j] = 0.0 + Phi[i * L + 9 + j] * 1.0; pg[9 + j] = 0.0 + Phi[i * L + 12 + j] * 1.0;
        }
    }
    for (int i = A; i < B; ++i) for (int j = 0; j < 12; ++j) PG[i * 12 + j] = G[i * 12 + j];
    for (int i = 0; i < B; ++i) for (int k = 0; k < 12; ++k) PGT[k * B + i] = PG[i * 12 + k];
    CT(1);
    // Q = (PG diag(Qc) PG^T) dt: rows / columns 9..14 of PG are unit rows (a single 1 at column 6 + (r - 9))
    for (int i = 0; i < A; ++i) {
        double* qr = Q + i * B;
        for (int j = 0; j < A; ++j) qr[j] = 0;
        for (int k = 0; k < 12; ++k) { const double a = PG[i * 12 + k] * e->Qc[k]; const double* g = PGT + k * B; for (int j = 0; j < A; ++j) qr[j] += a * g[j]; }
        for (int j = A; j < B; ++j) { const int kj = 6 + (j - A); qr[j] = 0.0 + (PG[i * 12 + kj] * e->Qc[kj]) * 1.0; }
        for (int j = 0; j < B; ++j) qr[j] *= dtime;
    }
    for (int i = A; i < B; ++i) {
        double* qr = Q + i * B; const int ki = 6 + (i - A);
        for (int j = 0; j < A; ++j) qr[j] = 0.0 + (1.0 * e->Qc[ki]) * PG[j * 12 + ki];
        for (int j = A; j < B; ++j) qr[j] = (j == i) ? 0.0 + (1.0 * e->Qc[ki]) * 1.0 : 0.0;
        for (int j = 0; j < B; ++j) qr[j] *= dtime;
    }
    CT(2);
    if (!e->have_prop) {
        memcpy(e->Phi_tot, Phi, sizeof(double) * L * L);
        memset(e->Q_tot, 0, sizeof(double) * L * L);
        for (int i = 0; i < B; ++i) for (int j = 0; j < B; ++j) e->Q_tot[i * L + j] = Q[i * B + j];
        e->have_prop = true;
    } else {
        double T[A * LEG_MAX];
        // Phi_tot <- Phi Phi_tot : only rows 0..8 change.  Rows 9.. of Phi_tot ARE identity rows (they start as Phi's and never change), so
        // a non-zero Phi[i][k] with k >= 9 contributes Phi[i][k] * 1 to column k alone - after the dense part k < 9, which is its place
        // in the ascending sum
        // (k outermost: the nine rows' accumulators are independent chains the core overlaps; each element still sums over k ascending)
        for (int e_ = 0; e_ < A * L; ++e_) T[e_] = 0;
        for (int k = 0; k < A; ++k) {
            const double* x = e->Phi_tot + k * L;
            for (int i = 0; i < A; ++i) {
                const double a = Phi[i * L + k];
                if (a == 0.0) continue;
                double* t = T + i * L;
                for (int j = 0; j < L; ++j) t[j] += a * x[j];
            }
        }
        for (int i = 0; i < A; ++i) { double* t = T + i * L; for (int z = 0; z < rz_n[i]; ++z) { const int k = nzc[rz_q[i][z]]; if (k >= A) t[k] += Phi[i * L + k] * 1.0; } }
        memcpy(e->Phi_tot, T, sizeof(double) * A * L);
        CT(3);
        // Q_tot <- Phi Q_tot Phi^T + Q.  Q_tot is zero outside its leading 15 x 15 block (rows 9.. of Phi are identity rows and G is zero
        // below row 14), so only k < 15 and the first 15 columns / rows take part: rows 0..8 of (Phi Q_tot), then columns 0..8 of (. Phi^T)
        for (int e_ = 0; e_ < A * 16; ++e_) T[e_] = 0;
        for (int k = 0; k < B; ++k) {
            const double* x = e->Q_tot + k * L;
            for (int i = 0; i < A; ++i) {
                const double a = Phi[i * L + k];
                if (a == 0.0) continue;
                double* t = T + i * 16;
                for (int j = 0; j < 16; ++j) t[j] += a * x[j];          // (column 15 of Q_tot is zero: a full fourth vector instead of a tail)
            }
        }
        for (int i = 0; i < A; ++i) for (int j = 0; j < B; ++j) e->Q_tot[i * L + j] = T[i * 16 + j];
        CT(4);
        for (int i = 0; i < B; ++i) {
            double u[12];                                  // three full AVX2 vectors: the rows of PhiT are padded with zeros to 12 (lanes 9..11 are not stored)
            double* t = e->Q_tot + i * L;
            for (int j = 0; j < 12; ++j) u[j] = 0;
            for (int q = 0; q < 15; ++q) { const double a = t[q]; const double* ph = PhiT + q * 12; for (int j = 0; j < 12; ++j) u[j] += a * ph[j]; }
            for (int j = 0; j < A; ++j) t[j] = u[j];
        }
        CT(5);
        for (int i = 0; i < B; ++i) for (int j = 0; j < B; ++j) e->Q_tot[i * L + j] += Q[i * B + j];
        CT(6);
    }
}

static void process_model(lvk_ekf* e, double time, const double* m_gyro, const double* m_acc)
{   // larvio.cpp:520-578.  The covariance part is COMPOSED over the frame's IMU samples:
    //   Phi_tot <- Phi Phi_tot ;  Q_tot <- Phi Q_tot Phi^T + Q     (then applied once on the device)
    const bool calib = e->cfg.calib_imu_instrinsic != 0;
    double f[3], w[3], w_old[3], f_old[3], acc[3], gyro[3], acc_old[3], gyro_old[3];
    for (int i = 0; i < 3; ++i) { f[i] = m_acc[i] - e->s.ba[i]; f_old[i] = e->m_acc_old[i] - e->s.ba[i]; }
    if (calib) {
        double t[3];
        m3_v(e->Ma, f, acc); m3_v(e->As, acc, t); for (int i = 0; i < 3; ++i) w[i] = m_gyro[i] - t[i] - e->s.bg[i]; m3_v(e->Tg, w, gyro);
        m3_v(e->Ma, f_old, acc_old); m3_v(e->As, acc_old, t); for (int i = 0; i < 3; ++i) w_old[i] = e->m_gyro_old[i] - t[i] - e->s.bg[i]; m3_v(e->Tg, w_old, gyro_old);
    } else {
        for (int i = 0; i < 3; ++i) { w[i] = m_gyro[i] - e->s.bg[i]; w_old[i] = e->m_gyro_old[i] - e->s.bg[i]; acc[i] = f[i]; gyro[i] = w[i]; acc_old[i] = f_old[i]; gyro_old[i] = w_old[i]; }
    }
    const double dtime = time - e->s.t;
    predict_new_state(e, dtime, gyro, acc);
    double Phi[LEG_MAX * LEG_MAX];
    if (calib) cal_phi_calib(e, Phi, dtime, f, w, acc, gyro, f_old, w_old, acc_old, gyro_old);
    else cal_phi(e, Phi, dtime, w, w_old);
    if (calib) compose_transition<46, true>(e, Phi, dtime); else compose_transition<22, false>(e, Phi, dtime);
    e->s.t = time; e->s_fej_now.t = time;
}

static int batch_imu(lvk_ekf* e, double time_bound, const lvk_imu* imu, int n_imu)
{   // larvio.cpp:464-517
    int used = 0; double dt = 0.0;
    for (int i = 0; i < n_imu; ++i) {
        const double imu_time = imu[i].t;
        if (imu_time <= e->s.t) { ++used; continue; }
        if (imu_time - time_bound > e->imu_img_time_th) break;
        dt = imu_time - time_bound;
        process_model(e, imu_time, imu[i].gyro, imu[i].acc);
        ++used;
        memcpy(e->m_gyro_old, imu[i].gyro, 24); memcpy(e->m_acc_old, imu[i].acc, 24);
    }
    e->imu_id = e->next_state_id++;
    e->imu_dt = dt;
    return used;
}

static lvk_status state_augmentation(lvk_ekf* e)
{   // larvio.cpp:720-801; the covariance part is an index gather (rows/cols {0,1,2,6,7,8} duplicated before the feature block)
    Clone c; memset(&c, 0, sizeof c);
    c.id = e->imu_id; c.time = e->s.t; c.dt = e->imu_dt;
    memcpy(c.q, e->s.q, 32); memcpy(c.p, e->s.p, 24); memcpy(c.p_fej, e->s_fej_now.p, 24);
    memcpy(c.R_b2c, e->R_b2c, 72); memcpy(c.t_c_b, e->t_c_b, 24);
    {
        double R_b2w[9], R_w2b[9], R_w2c[9], R_c2w[9], t[3];
        quat_to_rot(c.q, R_b2w); m3_t(R_b2w, R_w2b); m3_mul(e->R_b2c, R_w2b, R_w2c); m3_t(R_w2c, R_c2w);
        rot_to_quat(R_c2w, c.q_cam);
        m3_v(R_b2w, e->t_c_b, t);
        for (int i = 0; i < 3; ++i) c.p_cam[i] = e->s.p[i] + t[i];
    }
    const int pose_rows = LEG + 6 * (int)e->clones.size();
    if (e->N + 6 > e->nmax) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "state dimension %d exceeds capacity %d", e->N + 6, e->nmax);
    e->clones.push_back(c); e->ranks_dirty = true; e->rcam_valid = false;
    static const int sel[6] = {0, 1, 2, 6, 7, 8};
    std::vector<int> idx; idx.reserve(e->N + 6);
    for (int i = 0; i < pose_rows; ++i) idx.push_back(i);
    for (int i = 0; i < 6; ++i) idx.push_back(sel[i]);
    for (int i = pose_rows; i < e->N; ++i) idx.push_back(i);
    e->p00_valid = false;                                // the IMU block is about to be propagated
    if (!e->have_prop) return cov_gather(e, idx);
    // the frame's propagation (composed Phi, Q) rides in the same launch: k_cov_propagate_augment (the index map is analytic there)
    const int n_out = (int)idx.size(), L = LEG;
    double* h_pq = up_alloc<double>(e, (size_t)2 * L * L);            // the launch may be deferred: Phi_tot / Q_tot are copied now
    if (!h_pq) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memcpy(h_pq, e->Phi_tot, sizeof(double) * L * L); memcpy(h_pq + L * L, e->Q_tot, sizeof(double) * L * L);
    e->have_prop = false;
    double* src = e->dP[e->cur]; double* dst = e->dP[e->cur ^ 1];
    const double* d_pq = dev(e, h_pq);
    lvk_status st = run_or_defer(e, [=]() { return lvk_cov_propagate_augment(e->ctx, src, e->ld, dst, e->ld, n_out, pose_rows, L, h_pq, h_pq + L * L, d_pq); });
    if (st != LVK_OK) return st;
    e->cur ^= 1; e->N = n_out;
    return LVK_OK;
}

static void add_observations(lvk_ekf* e, const lvk_feature_obs* f, int n)
{   // larvio.cpp:804-856
    const long long sid = e->imu_id;
    const int curr_num = (int)e->map.size();
    int tracked = 0;
    const double dt = e->imu_dt;
    const int prev_rank = clone_rank(e, sid - 1);
    // The message lists the tracks in table order, i.e. by ascending id: a cursor walks the (ordered) map alongside - one step per
    // feature instead of a tree descent; an id out of order falls back to find().
    auto cur = e->map.begin();
    long long last_id = -1;
    for (int i = 0; i < n; ++i) {
        const long long id = (long long)f[i].id;
        decltype(cur) it;
        if (id > last_id) { while (cur != e->map.end() && cur->first < id) ++cur; it = (cur != e->map.end() && cur->first == id) ? cur : e->map.end(); }
        else it = e->map.find(id);
        const bool ordered = id > last_id;
        last_id = ordered ? id : last_id;
        if (it == e->map.end()) {
            auto ins = ordered ? e->map.emplace_hint(cur, id, Feature()) : e->map.emplace(id, Feature()).first;
            if (ordered) cur = ins;
            Feature& ft = ins->second; ft.id = id;
            ft.set(sid, f[i].u + f[i].u_vel * dt, f[i].v + f[i].v_vel * dt, f[i].u_vel, f[i].v_vel);
            ft.total_obs++;
            if (!(f[i].u_init == -1 && f[i].v_init == -1) && prev_rank >= 0) {
                const double dt_ = e->clones[prev_rank].dt;
                ft.set(sid - 1, f[i].u_init + f[i].u_init_vel * dt_, f[i].v_init + f[i].v_init_vel * dt_, f[i].u_init_vel, f[i].v_init_vel);
                ft.total_obs++;
            }
        } else {
            Feature& ft = it->second;
            ft.set(sid, f[i].u + f[i].u_vel * dt, f[i].v + f[i].v_vel * dt, f[i].u_vel, f[i].v_vel);
            ft.total_obs++;
            ++tracked;
            int pi;
            if (e->cfg.if_zupt_valid && (pi = ft.find(sid - 1)) >= 0) {
                double dx = f[i].u - ft.obs[pi].z[0], dy = f[i].v - ft.obs[pi].z[1];
                e->coarse_dis.push_back(sqrt(dx * dx + dy * dy));
            }
        }
    }
    e->tracking_rate = (double)tracked / (double)curr_num;
    e->map.purge();                                      // features erased by the previous update and not re-created by this message
}

// ------------------------------------------------------------------------- state injection (larvio.cpp:1476-1575 etc.)
static void inject(lvk_ekf* e, const double* dx)
{
    e->rcam_valid = false;
    double dq[4], q[4];
    small_angle_quat(dx, dq); quat_mul(dq, e->s.q, q); memcpy(e->s.q, q, 32);
    for (int i = 0; i < 3; ++i) { e->s.v[i] += dx[3 + i]; e->s.p[i] += dx[6 + i]; e->s.bg[i] += dx[9 + i]; e->s.ba[i] += dx[12 + i]; }
    double dqe[4], Re[9], Ret[9], Rn[9];
    small_angle_quat(dx + 15, dqe); quat_to_rot(dqe, Re); m3_t(Re, Ret); m3_mul(e->R_b2c, Ret, Rn); memcpy(e->R_b2c, Rn, 72);
    for (int i = 0; i < 3; ++i) e->t_c_b[i] += dx[18 + i];
    e->td += dx[21];
    if (e->cfg.calib_imu_instrinsic) { for (int i = 0; i < 24; ++i) e->imx[i] += dx[22 + i]; update_imu_mx(e); }      // :1497-1507
    for (size_t c = 0; c < e->clones.size(); ++c) {
        Clone* cl = &e->clones[c];
        const double* d = dx + LEG + 6 * c;
        double dqc[4], qc[4];
        small_angle_quat(d, dqc); quat_mul(dqc, cl->q, qc); memcpy(cl->q, qc, 32);
        for (int i = 0; i < 3; ++i) cl->p[i] += d[3 + i];
        clone_refresh_cam(e, cl);
    }
    const int base = LEG + 6 * (int)e->clones.size();
    for (size_t i = 0; i < e->feature_states.size(); ++i) {
        Feature& f = e->map[e->feature_states[i]];
        const int ar = clone_rank(e, f.id_anchor);
        if (ar < 0) continue;
        const Clone* a = &e->clones[ar];
        double R_c2w[9]; quat_to_rot(a->q_cam, R_c2w);
        f.inv_depth += dx[base + i];
        double pc[3] = {f.obs_anchor[0] / f.inv_depth, f.obs_anchor[1] / f.inv_depth, 1 / f.inv_depth}, pw[3];
        m3_v(R_c2w, pc, pw);
        for (int k = 0; k < 3; ++k) f.position[k] = pw[k] + a->p_cam[k];
    }
}

// ------------------------------------------------------------------------- device job batches
// one triangulation request: its views live in the filter's request pools (tri_ranks / tri_z) at [off, off + n) - no per-request
// vectors (at configs[4] an update issues hundreds of requests)
struct TriReq { Feature* f; int mode; int off, n; long long last_id; bool use_pos; int slot = -1; };   // slot >= 0: the row job that takes the result on the device (launch_triangulation)
struct TriAns { bool ok; double position[3], inv_depth, obs_anchor[3]; long long id_anchor; };

static lvk_status upload_clones(lvk_ekf* e)
{
    const size_t n = e->clones.size();
    CamPose* hc = up_alloc<CamPose>(e, n); CloneDev* hd = up_alloc<CloneDev>(e, n);
    if (!hc || !hd) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    for (size_t i = 0; i < n; ++i) {
        const Clone& c = e->clones[i];
        quat_to_rot(c.q_cam, hc[i].R); memcpy(hc[i].t, c.p_cam, 24);
        clone_dev_from(c, &hd[i]);
    }
    // (pinned-host arena only.)  The two tables are read by EVERY workgroup of the triangulation and row kernels that follow (40..2000 of them), and the arena is host
    // memory: each of those reads would cross PCIe (k_feature_rows spent 9 of its 29 us fetching 5 KB of clone poses per workgroup,
    // profiles/r4_c_be_ticks.json).  One small kernel copies them to device memory once; it runs while this thread is still building
    // the jobs that use them.
    if (e->bar_push) {                                  // the arena IS device memory: the tables are read where the host pushed them
        lvk_status fs = flush_uploads(e);
        if (fs != LVK_OK) return fs;
        e->dv_cams = dev(e, hc); e->dv_clones = dev(e, hd);
        return LVK_OK;
    }
    const size_t nb_c = sizeof(CamPose) * n, nb_d = sizeof(CloneDev) * n;
    lvk_status st = lvk_stage_copy2(e->ctx, e->d_cams, dev(e, hc), nb_c, e->d_clones, dev(e, hd), nb_d);
    if (st != LVK_OK) return st;
    e->dv_cams = e->d_cams; e->dv_clones = e->d_clones;
    return LVK_OK;
}

// mode 0 initializePosition(curr_id), 1 initializePosition_AssignAnchor, 2 initializeInvParamPosition(curr_id) (feature.hpp:383-890)
static void make_tri_req(lvk_ekf* e, Feature* f, int mode, TriReq* rq)
{
    rq->f = f; rq->mode = mode; rq->off = (int)e->tri_ranks.size(); rq->n = 0; rq->last_id = -1;
    for (const Obs& o : f->obs) {
        int r = clone_rank(e, o.sid);
        if (r < 0) continue;
        if (mode != 1 && o.sid == e->imu_id) continue;
        e->tri_ranks.push_back(r); e->tri_z.push_back(o.z[0]); e->tri_z.push_back(o.z[1]); rq->last_id = o.sid; rq->n += 1;
    }
    rq->use_pos = (mode != 2) && f->is_initialized;
}
static void apply_tri(Feature* f, int mode, const TriAns& a)
{   // feature.hpp:537-546 incl. the FEJ quirk (position_FEJ takes the OLD position of a first-time feature)
    if (!a.ok) return;
    if (!f->is_initialized) memcpy(f->position_fej, f->position, 24);
    f->is_initialized = true;
    memcpy(f->position, a.position, 24);
    f->id_anchor = a.id_anchor;
    f->inv_depth = a.inv_depth; memcpy(f->obs_anchor, a.obs_anchor, 24);
    if (mode == 2) f->ekf_feature = true;
}
// queues the batch; results go to the device-mapped host mirror (d_triout) and to d_tridev, at the request's slot when it names one
static lvk_status launch_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs)
{
    if (reqs.empty()) return LVK_OK;
    size_t tot = 0; for (auto& r : reqs) tot += (size_t)r.n;
    if ((int)reqs.size() > e->feat_cap || (int)tot > e->obs_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "triangulation batch of %d features / %zu observations exceeds capacity (%d / %d): lvk_ekf_config.max_features is %d - set it to the tracker's budget (max_features_num)",
                                                                                            (int)reqs.size(), tot, e->feat_cap, e->obs_cap, e->cfg.max_features);
    for (auto& r : reqs) if (r.slot >= 2 * e->feat_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "feature batch exceeds capacity");
    TriJob* hj = up_alloc<TriJob>(e, reqs.size()); int* hr = up_alloc<int>(e, tot); double* hz = up_alloc<double>(e, 2 * tot);
    if (!hj || !hr || !hz) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    size_t off = 0;
    for (size_t i = 0; i < reqs.size(); ++i) {
        TriReq& r = reqs[i];
        hj[i].n = r.n; hj[i].use_position = r.use_pos ? 1 : 0; hj[i].obs_off = (int)off; hj[i].out_slot1 = r.slot >= 0 ? r.slot + 1 : 0;
        memcpy(hj[i].position_in, r.f->position, 24);
        memcpy(hr + off, e->tri_ranks.data() + r.off, sizeof(int) * (size_t)r.n); memcpy(hz + 2 * off, e->tri_z.data() + 2 * (size_t)r.off, sizeof(double) * 2 * (size_t)r.n);
        off += (size_t)r.n;
    }
    lvk_status st = flush_uploads(e);
    if (st == LVK_OK) st = lvk_launch_triangulate(e->ctx, dev(e, hj), (int)reqs.size(), e->dv_cams, dev(e, hr), dev(e, hz), e->d_triout, e->d_tridev);
    if (st == LVK_OK) e->counters[7] += (long)reqs.size();
    return st;
}
static TriAns tri_answer(const lvk_ekf* e, const TriReq& rq, size_t slot)
{   // after a stream sync that covers the batch: d_triout IS the mapped view of h_down
    const TriResult& o = ((const TriResult*)e->h_down)[slot];
    TriAns a; a.ok = o.ok != 0; memcpy(a.position, o.position, 24); a.inv_depth = o.inv_depth; memcpy(a.obs_anchor, o.obs_anchor, 24); a.id_anchor = rq.last_id;
    return a;
}
static lvk_status run_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs, std::vector<TriAns>& ans)
{
    ans.assign(reqs.size(), TriAns());
    if (reqs.empty()) return LVK_OK;
    lvk_status st = launch_triangulation(e, reqs);
    if (st != LVK_OK) return st;
    EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
    for (size_t i = 0; i < reqs.size(); ++i) ans[i] = tri_answer(e, reqs[i], reqs[i].slot >= 0 ? (size_t)reqs[i].slot : i);
    return LVK_OK;
}
static bool feat_check_motion(const lvk_ekf* e, const Feature& f, bool if_tracked)
{   // Feature::checkMotion (feature.hpp:334-381)
    const int first = 0, last = if_tracked ? (int)f.obs.size() - 2 : (int)f.obs.size() - 1;
    const int ra = clone_rank(e, f.obs[first].sid);
    const Clone& a = e->clones[ra]; const Clone& b = e->clones[clone_rank(e, f.obs[last].sid)];
    const double* Ra = clone_Rcam(e, ra);
    double d[3] = {f.obs[first].z[0], f.obs[first].z[1], 1.0};
    const double n = v3_norm(d); d[0] /= n; d[1] /= n; d[2] /= n;
    double dw[3]; m3_v(Ra, d, dw);
    double tr[3] = {b.p_cam[0] - a.p_cam[0], b.p_cam[1] - a.p_cam[1], b.p_cam[2] - a.p_cam[2]};
    const double par = tr[0] * dw[0] + tr[1] * dw[1] + tr[2] * dw[2];
    double o[3] = {tr[0] - par * dw[0], tr[1] - par * dw[1], tr[2] - par * dw[2]};
    return v3_norm(o) > e->cfg.feature_translation_threshold;
}

// One feature-rows job (rows on the device) ------------------------------------------------------------
// the job of an MSCKF feature over the given observations, or over all it has
static RowJob msckf_job(Feature* f, std::vector<long long> sids, int tri = -1)
{
    RowJob r; r.f = f; r.type = JOB_MSCKF; r.want_gate = true; r.dof = 2 * (int)sids.size() - 3; r.tri = tri; r.sids = std::move(sids);
    return r;
}
static RowJob msckf_job(Feature* f, int tri = -1)
{
    std::vector<long long> sids; sids.reserve(f->obs.size()); for (const Obs& o : f->obs) sids.push_back(o.sid);
    return msckf_job(f, std::move(sids), tri);
}
// the two rows of a tracked in-state feature's newest observation
static RowJob tracked_job(const lvk_ekf* e, Feature* f)
{
    RowJob r; r.f = f; r.type = JOB_EKF_TRACKED; r.sids = {e->imu_id}; r.want_gate = true; r.dof = 2;
    return r;
}
// a feature about to enter the state: its MSCKF-form gate job, then its rows over every observation but the anchor's
static void new_feature_jobs(Feature* f, std::vector<RowJob>& jobs)
{
    jobs.push_back(msckf_job(f));
    RowJob r; r.f = f; r.type = JOB_EKF_NEW; r.want_gate = false; r.dof = 0;
    for (const Obs& o : f->obs) if (o.sid != f->id_anchor) r.sids.push_back(o.sid);
    jobs.push_back(r);
}

typedef std::vector<std::pair<size_t, size_t>> JobRanges;
static lvk_status launch_feature_rows(lvk_ekf* e, std::vector<RowJob>& jobs, const JobRanges* ranges = nullptr, RowObs* obs_out = nullptr)
{   // stages the jobs and queues k_feature_rows (for the given index ranges only, in the sharded update); nothing is read back
    // (fetch_feature_results does that)
    if (jobs.empty()) return LVK_OK;
    if ((int)jobs.size() > 2 * e->feat_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "feature batch exceeds capacity");
    size_t tot = 0, stage = 0, ccols = 0; int max_rows = 2, gate_max = 0;
    size_t m_max = 1; for (auto& j : jobs) { tot += j.sids.size(); m_max = std::max(m_max, j.sids.size()); }
    // short tracks only (always, with max_track_len 6) and one launch for the whole batch: the observations go to fixed-stride slots,
    // so that the row kernel can ask for them without having read the job record first (k_feature_rows: one PCIe round trip less)
    const int obs_stride = (!ranges && m_max <= 8) ? (int)m_max : 0;
    if (obs_stride) tot = jobs.size() * (size_t)obs_stride;
    if ((int)tot > e->obs_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "observation batch exceeds capacity");
    FeatJob* hj = up_alloc<FeatJob>(e, jobs.size()); int* hr = up_alloc<int>(e, tot); double* hz = up_alloc<double>(e, 2 * tot); double* hv = up_alloc<double>(e, 2 * tot);
    if (!hj || !hr || !hz || !hv) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    size_t off = 0; bool any_pending = false;
    for (size_t i = 0; i < jobs.size(); ++i) {
        RowJob& j = jobs[i]; Feature* f = j.f;
        const int M = (int)j.sids.size();
        FeatJob& d = j.dev; memset(&d, 0, sizeof d);
        if (obs_stride) off = i * (size_t)obs_stride;
        d.type = j.type; d.n_obs = M; d.obs_off = (int)off; d.want_gate = (j.want_gate ? FJ_GATE : 0) | (j.tri >= 0 ? FJ_TRI_PENDING : 0);
        any_pending = any_pending || j.tri >= 0;
        d.anchor_rank = (j.type == JOB_MSCKF) ? 0 : clone_rank(e, f->id_anchor);
        d.fcol = (j.type == JOB_MSCKF) ? 0 : LEG + 6 * (int)e->clones.size() + fs_rank(e, f->id);
        d.stage_off = (long long)stage; d.ccol_off = (int)ccols;
        d.gate_thr = j.want_gate ? lvk_chi2_005(j.dof) : 0.0;
        memcpy(d.p_w, f->position, 24); memcpy(d.p_fej, f->position_fej, 24); d.inv_depth = f->inv_depth; memcpy(d.obs_anchor, f->obs_anchor, 24);
        for (int k = 0; k < M; ++k) {
            const int oi = f->find(j.sids[k]);
            hr[off + k] = clone_rank(e, j.sids[k]);
            hz[2 * (off + k)] = f->obs[oi].z[0]; hz[2 * (off + k) + 1] = f->obs[oi].z[1];
            hv[2 * (off + k)] = f->obs[oi].zv[0]; hv[2 * (off + k) + 1] = f->obs[oi].zv[1];
        }
        if (obs_stride) for (int k = M; k < obs_stride; ++k) { hr[off + k] = 0; hz[2 * (off + k)] = hz[2 * (off + k) + 1] = hv[2 * (off + k)] = hv[2 * (off + k) + 1] = 0.; }
        off += M;
        stage += (size_t)fj_stage_doubles(j.type, M); ccols += (size_t)fj_cols(j.type, M);
        max_rows = std::max(max_rows, 2 * M);
        if (j.want_gate) gate_max = std::max(gate_max, fj_rows(j.type, M));
        hj[i] = d; j.hdev = &hj[i];
    }
    max_rows = lvk_feature_rows_route(max_rows, gate_max);
    if (stage > e->staging_cap || ccols > e->ccols_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "staging buffer too small (%zu doubles needed)", stage);
    const FilterFlags fl = filter_flags(LEG, e->if_fej, e->cfg.estimate_td, e->sigma2);
    const FeatJob* d_j = dev(e, hj); const int* d_r = dev(e, hr); const double* d_z = dev(e, hz); const double* d_v = dev(e, hv);
    const int nj = (int)jobs.size(); const CloneDev* d_cl = e->dv_clones; double* P = e->dP[e->cur];
    FeatResult* d_fh = (FeatResult*)(e->dh_down + e->down_feat);
    double* Ho = e->d_H; double* ro = e->d_r; const int ldh = e->ld, ncols_out = e->N;       // direct output of the jobs that carry a destination row (FeatJob::dst_row1, patched by gated_update)
    const int n_cl = (int)e->clones.size();
    const TriResult* d_tri = any_pending ? e->d_tridev : nullptr;      // results of the triangulation queued ahead, by job index (whole-batch launches only)
    if (obs_out) { obs_out->rank = d_r; obs_out->z = d_z; obs_out->zv = d_v; }
    if (any_pending && ranges) return lvk_set_error(e->ctx, LVK_ERR_ARG, "internal: device-consumed triangulation in a ranged launch");
    if (!ranges) return run_or_defer(e, [=]() { return lvk_launch_feature_rows(e->ctx, d_j, nj, max_rows, d_cl, d_r, d_z, d_v, P, e->ld, fl, e->d_staging, e->d_ccols, e->d_fout, d_fh, Ho, ldh, ncols_out, ro, obs_stride, n_cl, d_tri); });
    for (const auto& rg : *ranges) {                    // jobs carry absolute offsets into the observation / staging / column arrays
        const size_t lo = rg.first; const int n = (int)(rg.second - rg.first);
        if (n <= 0) continue;
        lvk_status st = run_or_defer(e, [=]() { return lvk_launch_feature_rows(e->ctx, d_j + lo, n, max_rows, d_cl, d_r, d_z, d_v, P, e->ld, fl, e->d_staging, e->d_ccols, e->d_fout + lo, d_fh + lo, nullptr, 0, 0, nullptr, 0, n_cl, nullptr); });
        if (st != LVK_OK) return st;
    }
    return LVK_OK;
}
static lvk_status shard_peer_check(lvk_ekf* e);
// results of the queued jobs (+ optionally n_dx doubles of d_dx in the same sync)
static lvk_status fetch_feature_results(lvk_ekf* e, std::vector<RowJob>& jobs, double* dx = nullptr, size_t n_dx = 0)
{
    const FeatResult* ho = (const FeatResult*)(e->h_down + e->down_feat);
    EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
    { lvk_status ps = shard_peer_check(e); if (ps != LVK_OK) return ps; }
    { lvk_status hs = update_health(e); if (hs != LVK_OK) return hs; }
    for (size_t i = 0; i < jobs.size(); ++i) jobs[i].res = ho[i];
    if (n_dx) memcpy(dx, e->h_down + e->down_dx, sizeof(double) * n_dx);      // written by the W^T[W|w] launch of the update
    return LVK_OK;
}
// row layout of a job, known before it runs: MSCKF blocks lose the 3 rows of the null-space projection, a new in-state
// feature's block keeps its range row first, a tracked in-state feature contributes its 2 rows as they are
static int job_first_row(const RowJob& j) { return fj_first_row(j.type); }
static int job_rows(const RowJob& j) { return fj_rows(j.type, (int)j.sids.size()); }
static bool gate_ok(lvk_ekf* e, const RowJob& j)
{
    const bool ok = j.res.gamma < lvk_chi2_005(j.dof);
    e->counters[ok ? 4 : 5]++;
    return ok;
}
// A run of consecutive stacked rows that share one column set (the rows of one feature job): what the structure-aware compression
// plans its TSQR tree from.  cols = the dense columns the rows can be non-zero in (ascending), as k_feature_rows lays them out:
// extrinsics + td 15..21, the observing clones' 6-blocks, the anchor's block and the feature's own column for in-state features.
static void job_dense_cols_build(const lvk_ekf* e, const RowJob& j, int ncols, std::vector<int>& out)
{
    out.clear();
    for (int k = 15; k < 22; ++k) out.push_back(k);
    auto block = [&](int rank) { for (int k = 0; k < 6; ++k) out.push_back(LEG + 6 * rank + k); };
    if (j.type != JOB_MSCKF) block(j.dev.anchor_rank);
    for (long long sid : j.sids) block(clone_rank(e, sid));
    if (j.type != JOB_MSCKF) out.push_back(j.dev.fcol);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    while (!out.empty() && out.back() >= ncols) out.pop_back();      // a new feature's own column is not part of H_o (k_stack_rows drops it)
}
// the shared column list of a job: consecutive jobs with the same observation set (a generation of tracks at configs[4]) reuse one
static ColList job_dense_cols(const lvk_ekf* e, const RowJob& j, int ncols)
{
    auto& c = e->colcache;
    if (c.cols && c.type == j.type && c.ncols == ncols && c.sids == j.sids && (j.type == JOB_MSCKF || (c.anchor == j.dev.anchor_rank && c.fcol == j.dev.fcol))) return c.cols;
    auto v = std::make_shared<std::vector<int>>();
    job_dense_cols_build(e, j, ncols, *v);
    c.type = j.type; c.ncols = ncols; c.sids = j.sids; c.anchor = j.dev.anchor_rank; c.fcol = j.dev.fcol; c.cols = v;
    return c.cols;
}
// rows [first, first+count) of a job's compact block -> consecutive dense rows starting at dst
static void push_rows(std::vector<StackRow>& map, const RowJob& j, int first, int count, int dst, int gate_job = -1,
                      std::vector<RowGroup>* groups = nullptr, const lvk_ekf* e = nullptr, int ncols = 0, int owner = 0)
{
    if (groups && count > 0) { groups->emplace_back(); RowGroup& g = groups->back(); g.start = dst; g.rows = count; g.owner = owner; g.cols = job_dense_cols(e, j, ncols); }
    for (int k = 0; k < count; ++k) map.push_back(fj_stack_row(j.dev, first + k, dst + k, gate_job));
}
static lvk_status stack_rows(lvk_ekf* e, const std::vector<StackRow>& map, double* dH, int ncols, double* dr)
{
    if (map.empty()) return LVK_OK;
    StackRow* h = up_alloc<StackRow>(e, map.size());
    if (!h) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memcpy(h, map.data(), sizeof(StackRow) * map.size());
    const StackRow* d_map = dev(e, h); const int n = (int)map.size();
    return run_or_defer(e, [=]() { return lvk_launch_stack_rows(e->ctx, e->d_fout, d_map, n, e->d_staging, e->d_ccols, dH, e->ld, ncols, dr); });
}
// ---- sharded update: job ownership, stage 1 (own rows -> compressed block), the exchange, the rank-ordered stack
// contiguous split of jobs [first, last) into `world` ranges of about equal raw row counts (the reference's stacking order is kept:
// rank g's rows precede rank g+1's)
static void shard_bounds(const std::vector<RowJob>& jobs, size_t first, size_t last, int world, std::vector<size_t>& b)
{
    b.assign((size_t)world + 1, last); b[0] = first;
    long total = 0; for (size_t k = first; k < last; ++k) total += 2 * (long)jobs[k].sids.size();
    long cum = 0; int g = 1;
    for (size_t k = first; k < last && g < world; ++k) {
        cum += 2 * (long)jobs[k].sids.size();
        while (g < world && cum * world >= total * g) { b[(size_t)g] = k + 1; ++g; }
    }
}
static int shard_owner(const std::vector<size_t>& b, size_t job) { int g = 0; while ((size_t)g + 2 < b.size() && job >= b[(size_t)g + 1]) ++g; return g; }
// Stage 1 + exchange.  `map` / `groups` describe ALL stacked rows (every rank computes the same description); this rank stacks the
// rows of the groups it owns, compresses them (structure-aware TSQR), packs the block together with the gate results of its jobs
// (job_b != nullptr), all-gathers, and unpacks every rank's block into d_H / d_r in rank order.  On return `groups` describes the
// stacked blocks (the input of the replicated second stage) and *m_out is their row count.
// Householder flops of one level of the structure-aware compression, on the structure actually factored (2 r c^2 - 2/3 c^3
// per node, here summed exactly): a node of r rows restricted to its c columns (+ the residual column) applies min(r, c) reflectors,
// reflector j costing 4 (r - j)(c + 1 - j) flops (dot products + updates of the trailing columns).  Pass-through nodes cost nothing.
static double qr_level_flops(const QrPlanLevel& L)
{
    double f = 0;
    for (const QrBlock& b : L.blocks) {
        if (b.copy) continue;
        const int k = std::min(b.in_rows, b.ncols);
        for (int j = 0; j < k; ++j) f += 4.0 * (double)(b.in_rows - j) * (double)(b.ncols + 1 - j);
    }
    return f;
}
// a HIP event for a profiling bracket: recycled (prof_free) once its bracket has been read
static hipEvent_t prof_take_event(lvk_ekf* e)
{
    hipEvent_t ev;
    if (!e->prof_free.empty()) { ev = e->prof_free.back(); e->prof_free.pop_back(); } else hipEventCreate(&ev);
    return ev;
}
// one level of the compression, bracketed by HIP events on the filter's stream when profiling is on (bench: roofline of the TSQR)
static lvk_status qr_level_launch(lvk_ekf* e, const QrPlanLevel& L, const double* Hin, const double* rin, double* Hout, double* rout, const QrBlock* d_blocks, const int* d_cols, int ncols)
{
    hipEvent_t a = nullptr, b = nullptr;
    if (e->prof_on) {
        a = prof_take_event(e); b = prof_take_event(e);
        hipEventRecord(a, e->ctx->stream);
    }
    lvk_status st = lvk_qr_sparse_level(e->ctx, Hin, e->ld, rin, Hout, e->ld, rout, d_blocks, (int)L.blocks.size(), d_cols, ncols, L.lds, L.max_rows, L.max_cols);
    if (a) { hipEventRecord(b, e->ctx->stream); e->prof_pending.push_back({a, b, qr_level_flops(L), 1, (double)L.in_rows}); }
    return st;
}
// all levels of a plan: each level's blocks and column lists go up, the level reads *H / *r and writes their ping-pong partner
// (d_H <-> d_Hb, d_r <-> d_rb); on return *H / *r name the result
static lvk_status run_qr_levels(lvk_ekf* e, const std::vector<QrPlanLevel>& levels, double** H, double** r, int ncols)
{
    for (const QrPlanLevel& L : levels) {
        QrBlock* hb = up_alloc<QrBlock>(e, L.blocks.size()); int* hc = up_alloc<int>(e, L.cols.size() + 1);
        if (!hb || !hc) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
        memcpy(hb, L.blocks.data(), sizeof(QrBlock) * L.blocks.size()); memcpy(hc, L.cols.data(), sizeof(int) * L.cols.size());
        lvk_status st = flush_uploads(e);
        double* Ho = (*H == e->d_H) ? e->d_Hb : e->d_H; double* ro = (*r == e->d_r) ? e->d_rb : e->d_r;
        if (st == LVK_OK) st = qr_level_launch(e, L, *H, *r, Ho, ro, dev(e, hb), dev(e, hc), ncols);
        if (st != LVK_OK) return st;
        *H = Ho; *r = ro;
    }
    return LVK_OK;
}
// A rank that fails locally BEFORE the exchange's size is known to it (the layout of an update that admits new in-state features
// depends on gate results it could not read) cannot post a poisoned block; it tells the transport to break the collective instead:
// the exchange callback with bytes_per_rank == 0 means "abort" (lvk_shard_allgather_rccl: ncclCommAbort - the peers' pending
// all-gather returns an error instead of waiting for this rank).
static void shard_abort(lvk_ekf* e)
{
    if (e->shard.fn) (void)e->shard.fn(e->shard.user, nullptr, nullptr, 0, (void*)e->ctx->stream);
}
static lvk_status shard_peer_check(lvk_ekf* e)
{   // call after a stream sync: did k_shard_unpack find a peer's block poisoned (that rank failed before the exchange)?
    if (!e->shard.fn) return LVK_OK;
    int* f = (int*)(e->h_down + e->down_flag);
    if (*f == 0) return LVK_OK;
    const int mask = *f; *f = 0;
    return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "sharded update: the block of a peer rank (mask 0x%x) arrived invalid - that rank failed before the exchange", mask);
}
// pre_fail: this rank already failed locally (a launch error while queueing its rows) - it still plans (host only), posts a poisoned
// header and takes part in the collective, then returns that error: its peers are told by k_shard_unpack instead of waiting forever.
static lvk_status shard_stage1(lvk_ekf* e, const std::vector<StackRow>& map, std::vector<RowGroup>& groups, int ncols, const std::vector<size_t>* job_b, int* m_out,
                               lvk_status pre_fail = LVK_OK)
{
    auto& S = e->shard; const int W = S.world, me = S.rank;
    std::vector<std::vector<RowGroup>> gr((size_t)W), outg((size_t)W);
    std::vector<StackRow> lmap; std::vector<int> m_of((size_t)W, 0);
    { size_t mi = 0; int lrow = 0;
      for (const RowGroup& g : groups) {
          gr[(size_t)g.owner].push_back(g); m_of[(size_t)g.owner] += g.rows;
          if (g.owner == me) for (int k = 0; k < g.rows; ++k) { StackRow sr = map[mi + (size_t)k]; sr.dst_row = lrow++; lmap.push_back(sr); }
          mi += (size_t)g.rows;
      } }
    std::vector<int> kk((size_t)W, 0); std::vector<QrPlanLevel> my_levels; std::vector<size_t> need((size_t)W, 0);
    for (int g = 0; g < W; ++g) {
        std::vector<QrPlanLevel> lv;
        lvk_qr_sparse_plan(gr[(size_t)g], ncols, lv, &kk[(size_t)g], &outg[(size_t)g]);
        need[(size_t)g] = sizeof(StackRow) * (size_t)m_of[(size_t)g] + 64;
        for (const QrPlanLevel& L : lv) need[(size_t)g] += sizeof(QrBlock) * L.blocks.size() + sizeof(int) * (L.cols.size() + 1) + 128;
        if (g == me) my_levels.swap(lv);
    }
    // ---- capacity checks.  Every rank plans every rank's share from the same inputs, so each test below has the same outcome on
    //      all ranks: a capacity error is raised everywhere, BEFORE anybody enters the collective (nobody is left waiting in it).
    int k_max = 0, j_max = 0, m_tot = 0;
    for (int g = 0; g < W; ++g) {
        if (m_of[(size_t)g] > e->hrows) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "sharded update: rank %d would stack %d measurement rows (capacity %d)", g, m_of[(size_t)g], e->hrows);
        if (kk[(size_t)g] > S.xk_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "sharded update: rank %d's compressed block has %d rows (exchange capacity %d)", g, kk[(size_t)g], S.xk_cap);
        if (e->up_off + need[(size_t)g] + sizeof(ShardMeta) * (size_t)W + 256 > e->up_lim) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "sharded update: upload arena too small for rank %d's plan", g);
        k_max = std::max(k_max, kk[(size_t)g]); m_tot += kk[(size_t)g];
        if (job_b) j_max = std::max(j_max, (int)((*job_b)[(size_t)g + 1] - (*job_b)[(size_t)g]));
    }
    if (m_tot > e->hrows) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "too many measurement rows (%d)", m_tot);
    const size_t res_bytes = ((size_t)j_max * sizeof(FeatResult) + 255) & ~(size_t)255;
    const size_t bytes = LVK_SHARD_HDR + res_bytes + std::max((size_t)k_max * (size_t)(ncols + 1) * sizeof(double), (size_t)256);
    if (bytes > S.cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "sharded update: %zu bytes per rank exceed the exchange buffers (%zu)", bytes, S.cap);
    ShardMeta* hm = up_alloc<ShardMeta>(e, (size_t)W);
    if (!hm) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    { int off = 0;
      for (int g = 0; g < W; ++g) {
          hm[g].job_lo = job_b ? (int)(*job_b)[(size_t)g] : 0; hm[g].job_n = job_b ? (int)((*job_b)[(size_t)g + 1] - (*job_b)[(size_t)g]) : 0;
          hm[g].k = kk[(size_t)g]; hm[g].row_off = off; off += kk[(size_t)g];
      } }
    // ---- this rank's share.  From here on a failure is local (a launch error, a broken device): the rank still enters the
    //      collective, with a poisoned header, so that its peers get an error from k_shard_unpack instead of waiting forever.
    const int m_loc = (int)lmap.size();
    double* X = e->d_H; double* rX = e->d_r;
    auto local = [&]() -> lvk_status {
        lvk_status st = stack_rows(e, lmap, e->d_H, ncols, e->d_r);
        if (st == LVK_OK) st = run_qr_levels(e, my_levels, &X, &rX, ncols);
        if (st != LVK_OK) return st;
        st = flush_uploads(e);
        if (st == LVK_OK) st = lvk_shard_pack(e->ctx, e->d_fout + hm[me].job_lo, hm[me].job_n, X, e->ld, rX, kk[(size_t)me], ncols, S.d_send, res_bytes, me);
        return st;
    };
    const lvk_status st_local = pre_fail != LVK_OK ? pre_fail : local();
    if (st_local != LVK_OK) { (void)hipGetLastError(); (void)hipMemsetAsync(S.d_send, 0xFF, LVK_SHARD_HDR, e->ctx->stream); }
    lvk_status st = S.fn(S.user, S.d_send, S.d_recv, bytes, (void*)e->ctx->stream);
    if (st_local != LVK_OK) return st_local;
    if (st != LVK_OK) return lvk_set_error(e->ctx, st, "sharded update: the exchange callback failed");
    FeatResult* d_fh = (FeatResult*)(e->dh_down + e->down_feat);
    st = flush_uploads(e);
    if (st == LVK_OK) st = lvk_shard_unpack(e->ctx, S.d_recv, bytes, res_bytes, dev(e, hm), W, ncols, k_max, e->d_fout, d_fh, e->d_H, e->ld, e->d_r, (int*)(e->dh_down + e->down_flag));
    if (st != LVK_OK) return st;
    S.stats[0]++; S.stats[1] += (long)bytes; S.stats[3] += m_loc;
    groups.clear();
    int off = 0;
    for (int g = 0; g < W; ++g) for (RowGroup& og : outg[(size_t)g]) { groups.push_back(og); groups.back().start = off; groups.back().owner = 0; off += og.rows; }
    *m_out = m_tot;
    return LVK_OK;
}

// dense update with m stacked rows already in d_H/d_r: compress (structure-aware when the row groups are known and it pays, dense
// Householder TSQR when the block is still too tall), update P, fetch dx
static lvk_status dense_update(lvk_ekf* e, int m, std::vector<double>& dx, int extra, const std::vector<RowGroup>* groups = nullptr)
{
    lvk_status st = LVK_OK;
    double* H = e->d_H; double* r = e->d_r;
    // The nodes cost 1-2 us per column of their union (one barrier-separated Householder step each, ~50..60 steps): measured on
    // MI355X the compression pays once it saves more than a few 32-row Cholesky panels - not for the typical update of the
    // north-star size (m ~ 110..260 rows of 9-row feature blocks over ~50 columns), decisively at configs[4] (thousands of rows).
    // From sparse_qr_min_rows (480) rows on it is always taken; between one fused Cholesky launch (160 rows) and that, it is taken
    // when a cost model of both routes says so - the case that matters is a pruning update at configs[4] depth: ~400 one-row blocks
    // that all live in the same 19 columns compress to 19 rows in one ~60 us level instead of a 400-row factorisation.  Constants
    // from profiles/r4_a_kernel_stats.csv: k_qr_sparse 124 us for a 55-column node over ~250 rows; k_chol_fused 31 us per 160-row
    // super-panel (~5 us per 32-row panel + 8), two k_dgemm_sk launches (~12 us) per further super-panel.
    auto t_chol = [](int rows) { const int p = (rows + 31) / 32, sp = (rows + 159) / 160; return 8.0 + 5.0 * p + 12.0 * (sp - 1) + 1.0e-4 * rows * rows; };
    bool worth_planning = groups && m > 160;
    if (g_tr.on && m > 160) { g_tr.cnt[0]++; g_tr.cnt[3] += m; }
    if (worth_planning && m < e->sparse_qr_min_rows && !e->shard.fn) {
        // the plan itself costs the filter's thread ~20 us: not drawn up when even its best case cannot win - one level whose widest
        // node has only the widest row group's columns (c), compressing to c rows
        size_t c = 0; for (const RowGroup& g : *groups) if (g.cols) c = std::max(c, g.cols->size());
        worth_planning = 12.0 + (double)c + t_chol((int)c) < t_chol(m);
    }
    if (worth_planning) {
        std::vector<QrPlanLevel> levels; int m2 = m;
        lvk_qr_sparse_plan(*groups, e->N, levels, &m2);
        bool take = !levels.empty() && m2 + 32 <= m;
        if (g_tr.on) g_tr.cnt[1]++;
        if (take && m < e->sparse_qr_min_rows) {
            double t_qr = 0;                               // microseconds: launch + the longest node's reflector chain per level
            for (const QrPlanLevel& L : levels) {
                double worst = 0;
                for (const QrBlock& b : L.blocks) if (!b.copy) worst = std::max(worst, (double)std::min(b.ncols, b.in_rows) * (1.0 + 0.004 * b.in_rows));
                t_qr += 12.0 + worst;
            }
            take = t_qr + t_chol(m2) < t_chol(m);
        }
        if (take && g_tr.on) g_tr.cnt[2]++;
        if (take) {
            st = run_qr_levels(e, levels, &H, &r, e->N);
            if (st != LVK_OK) return st;
            e->qr_stats[0]++; e->qr_stats[1] += (long)levels.size(); e->qr_stats[2] += m; e->qr_stats[3] += m2;
            m = m2;
        }
    }
    if (m > e->rows_cap - 32) {
        int m2 = m;
        st = lvk_qr_compress_dev(e->ctx, H, e->ld, m, e->N, r, &m2);
        if (st != LVK_OK) return st;
        m = m2;
    }
    TRS(3);
    UpdateWs ws = e->ws;
    ws.dx_host = (double*)(e->dh_down + e->down_dx);
    ws.p00_host = (double*)(e->dh_down + e->down_p00);
    e->last.H = H; e->last.r = r; e->last.m = m; e->last.n = e->N; e->redo = nullptr;
    if (e->prof_on && m > 0) {
        ws.ev_a = prof_take_event(e); ws.ev_b = prof_take_event(e);
        e->prof_pending.push_back({ws.ev_a, ws.ev_b, lvk_update_first_launch_flops(m, e->N), 0, 0.0});
    }
#ifdef LVK_NPD_DEBUG   // debug builds only: the stacked system of every small update, as the update kernels are about to read it
    if (m > 0 && m <= 40) {
        hipDeviceSynchronize();
        std::vector<double> hH((size_t)m * e->ld), hr((size_t)m), hP((size_t)e->N * e->ld);
        hipMemcpy(hH.data(), H, sizeof(double) * hH.size(), hipMemcpyDeviceToHost); hipMemcpy(hr.data(), r, sizeof(double) * m, hipMemcpyDeviceToHost);
        hipMemcpy(hP.data(), e->dP[e->cur], sizeof(double) * hP.size(), hipMemcpyDeviceToHost);
        double pmin = 1e300; bool pnan = false; for (int i = 0; i < e->N; ++i) { pmin = std::min(pmin, hP[(size_t)i * e->ld + i]); for (int j = 0; j < e->N; ++j) pnan = pnan || !std::isfinite(hP[(size_t)i * e->ld + j]); }
        fprintf(stderr, "[npd] update t %.2f: %d rows, N %d, min diag P %.3e, P finite %d\n", e->s.t, m, e->N, pmin, (int)!pnan);
        for (int i = 0; i < m; ++i) {
            double n2 = 0, s00 = 0; bool bad = false; int nz = 0;
            for (int j = 0; j < e->N; ++j) { const double v = hH[(size_t)i * e->ld + j]; bad = bad || !std::isfinite(v); n2 += v * v; nz += v != 0.; }
            for (int j = 0; j < e->N; ++j) for (int k = 0; k < e->N; ++k) s00 += hH[(size_t)i * e->ld + j] * hP[(size_t)j * e->ld + k] * hH[(size_t)i * e->ld + k];
            fprintf(stderr, "[npd]   row %2d: |h| %.3e nonzeros %d finite %d r %.3e  h P h' %.3e\n", i, sqrt(n2), nz, (int)!bad, hr[(size_t)i], s00);
        }
    }
#endif
    st = lvk_update_core(e->ctx, e->dP[e->cur], e->ld, e->N, H, e->ld, m, r, e->sigma2, e->d_dx, ws);
    if (st != LVK_OK) return st;
    e->p00_valid = m > 0;
    TRS(4);
    dx.assign((size_t)e->N + extra, 0.0);
    e->counters[2] = m;
    return LVK_OK;
}

// ------------------------------------------------------------------------- removeLostFeatures (larvio.cpp:1883-2256)
static int grid_code(const lvk_ekf* e, const double* xy)
{
    int row = (int)((xy[1] - e->y_min) / e->grid_h), col = (int)((xy[0] - e->x_min) / e->grid_w);
    return row * e->cfg.aug_grid_cols + col;
}
static inline int grid_occupancy(lvk_ekf* e, int code, int cells)
{   // grid_map[code].size() (larvio.cpp:1974)
    if (code >= 0 && code < cells) return e->grid_count[(size_t)code];
    return e->reference_grid ? e->grid_phantom[code] : 0;
}
static inline void grid_add(lvk_ekf* e, int code, int cells)
{   // grid_map[code].push_back(id) (:1990, :3366)
    if (code >= 0 && code < cells) e->grid_count[(size_t)code]++;
    else if (e->reference_grid) e->grid_phantom[code]++;
}
// The gated update in one sync.  No feature enters the state, so nothing on the host depends on a gate result before the update is
// launched: every candidate row gets its slot, the device zeroes the rows of rejected jobs (a zero row with a zero residual leaves
// the update unchanged), and gate results (jobs[].res), pending triangulation answers and dx come back in ONE sync.
// order: the job index ranges in stacking order - MSCKF jobs first, then the tracked in-state features' two rows each:
// H_o = [H_msckf ; H_ekf], the reference's order (larvio.cpp:1612-1626).  Unsharded, the row kernel (held back by begin_defer until
// the slots are known) writes its rows straight into H_o (FeatJob::dst_row1); sharded, this rank builds the rows of its slice of
// the jobs and shard_stage1 exchanges the compressed blocks.  tr: the trace slots that close after the row launch is staged (-1:
// none), after the update is launched and after the sync.  retire: state ids whose observations leave every feature once the jobs
// are staged (pruning: the clones about to go) - host work done here, while the device still runs what was queued ahead.
static void drop_observations(lvk_ekf* e, const long long* sids, int n) { for (auto kv : e->map) for (int k = 0; k < n; ++k) kv.second.erase(sids[k]); }
static lvk_status gated_update(lvk_ekf* e, std::vector<RowJob>& jobs, const size_t (&order)[2][2], const int (&tr)[3], std::vector<double>& dx,
                               const long long* retire = nullptr, int n_retire = 0, size_t mp_lo = 0, size_t mp_hi = 0)
{
    const int N = e->N;
    const bool sharded = e->shard.fn != nullptr;
    std::vector<size_t> jb; JobRanges own;
    if (sharded) { shard_bounds(jobs, 0, jobs.size(), e->shard.world, jb); own.push_back({jb[(size_t)e->shard.rank], jb[(size_t)e->shard.rank + 1]}); }
    begin_defer(e);                                     // the jobs (and their row slots) go up in one copy
    RowObs obs;
    lvk_status st = launch_feature_rows(e, jobs, sharded ? &own : nullptr, &obs);
    if (st == LVK_OK && !sharded) st = lvk_ekf_msckf_points_queue(e, jobs, mp_lo, mp_hi, obs);      // [mp_lo, mp_hi): the MSCKF jobs of a lost-feature update (lvk_ekf_set_msckf_points)
    if (tr[0] >= 0) TR(tr[0]);
    TRS(0);
    if (st != LVK_OK && !sharded) { end_defer(e); return st; }      // sharded: a local failure still goes through the exchange (shard_stage1, pre_fail)
    std::vector<StackRow> map_o; std::vector<RowGroup> grp;
    int m = 0;
    for (const auto& rg : order)
        for (size_t k = rg[0]; k < rg[1]; ++k) {
            const int r = job_rows(jobs[k]);
            push_rows(map_o, jobs[k], job_first_row(jobs[k]), r, m, (int)k, &grp, e, N, sharded ? shard_owner(jb, k) : 0);
            if (!sharded) jobs[k].hdev->dst_row1 = m + 1;
            m += r;
        }
    // k_feature_rows does not bound dst_row1 itself: no job may keep a slot beyond the hrows rows of d_H (the same on every rank)
    if (m > e->hrows) { for (RowJob& j : jobs) if (j.hdev) j.hdev->dst_row1 = 0; end_defer(e); return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "too many measurement rows (%d)", m); }
    TRS(1);
    drop_observations(e, retire, n_retire);
    { lvk_status s2 = end_defer(e); if (st == LVK_OK) st = s2; }
    TRS(2);
    if (sharded) { st = shard_stage1(e, map_o, grp, N, &jb, &m, st); e->shard.stats[2]++; }
    if (st == LVK_OK) st = dense_update(e, m, dx, 0, &grp);
    TR(tr[1]);
    if (st == LVK_OK) st = fetch_feature_results(e, jobs, dx.data(), (size_t)N);
    if (st != LVK_OK) return st;
    TR(tr[2]);
    return LVK_OK;
}
// ... and its effect on the host state, when any row passed its gate; counter: 0 feature update, 1 pruning update
static void gated_update_apply(lvk_ekf* e, const std::vector<double>& dx, int accepted, int counter)
{
    if (accepted <= 0) return;
    inject(e, dx.data());
    e->last_update_time = e->s.t;
    e->counters[counter]++;
    e->counters[2] = accepted;
}
// What a gated update leaves to the host, after its sync.  The MSCKF jobs [order[0]) in ascending order: a job whose triangulation
// was consumed on the device (RowJob::tri) has its answer read and applied in `mode`, and one whose triangulation failed is not used
// (its rows were zeroed on the device); the others pass through gate_ok and are recorded as MSCKF points.  retire(job, tri_ok) is
// the caller's bookkeeping for each of them.  Then the tracked in-state jobs [order[1]), two rows each.  Returns the accepted rows.
template <class Retire>
static int settle_update(lvk_ekf* e, const std::vector<RowJob>& jobs, const size_t (&order)[2][2], const std::vector<TriReq>& reqs, int mode, Retire retire)
{
    int accepted = 0;
    for (size_t k = order[0][0]; k < order[0][1]; ++k) {
        const RowJob& j = jobs[k];
        bool tri_ok = true;
        if (j.tri >= 0) { const TriAns a = tri_answer(e, reqs[(size_t)j.tri], k); apply_tri(j.f, mode, a); tri_ok = a.ok; }
        if (tri_ok && gate_ok(e, j)) { accepted += job_rows(j); lvk_ekf_msckf_point_record(e, j, k); }
        retire(j, tri_ok);
    }
    for (size_t k = order[1][0]; k < order[1][1]; ++k) if (gate_ok(e, jobs[k])) accepted += 2;
    return accepted;
}
// The triage of removeLostFeatures (larvio.cpp:1897-2005) over the features outside the state, in map order: which are invalid, which
// wait (not listed), which are candidates for this update, and which triangulations those ask for (reqs).  admission: may the EKF
// branch (:1945-1960) be taken in this message?  If not, only the MSCKF branch's request is made - initializePosition (mode 0) for a
// feature that is not initialised and has moved enough - and a tracked feature that has not moved waits.  If it may, a long tracked
// feature asks for both branches (mode 2, always from the two-view guess, and mode 0: the EKF branch resets is_initialized first) and
// stays listed whatever its motion, because the replay decides its branch.
struct Cand { Feature* f; bool tracked, invalid, motion; int idx_pos, idx_inv; };
static void lost_triage(lvk_ekf* e, bool admission, std::vector<Cand>& cands, std::vector<TriReq>& reqs)
{
    const lvk_ekf_config& c = e->cfg;
    cands.clear(); reqs.clear(); e->tri_ranks.clear(); e->tri_z.clear();
    for (auto kv : e->map) {
        Feature& f = kv.second;
        if (f.in_state) continue;
        Cand cd = {&f, f.find(e->imu_id) >= 0, false, false, -1, -1};
        if (cd.tracked && (int)f.obs.size() < c.max_track_len) continue;
        const bool both = cd.tracked && admission;
        if (!cd.tracked && (int)f.obs.size() < c.least_observation_number) cd.invalid = true;
        else if (!f.is_initialized || both) {
            cd.motion = feat_check_motion(e, f, cd.tracked);
            if (!cd.motion && !both) { if (cd.tracked) continue; cd.invalid = true; }     // a lost feature that has not moved is invalid (:1911-1916); a tracked one waits for more views
        }
        if (cd.motion) {
            if (both && !f.ekf_feature) { reqs.emplace_back(); make_tri_req(e, &f, 2, &reqs.back()); reqs.back().use_pos = false; cd.idx_inv = (int)reqs.size() - 1; }
            if (!f.is_initialized || (both && !f.ekf_feature)) { reqs.emplace_back(); make_tri_req(e, &f, 0, &reqs.back()); cd.idx_pos = (int)reqs.size() - 1; }
        }
        cands.push_back(cd);
    }
}
static lvk_status remove_lost_features(lvk_ekf* e)
{
    const lvk_ekf_config& c = e->cfg;
    const int cells = c.aug_grid_rows * c.aug_grid_cols;
    std::vector<Feature*> ekf_tracked; std::vector<long long> ekf_lost;
    std::vector<const Feature*> long_tracked;                    // tracked, not in the state, max_track_len observations: what may ask for admission
    for (auto kv : e->map) {
        Feature& f = kv.second;
        const bool tracked = f.find(e->imu_id) >= 0;
        if (f.in_state) { if (tracked) ekf_tracked.push_back(&f); else ekf_lost.push_back(f.id); }
        else if (tracked && (int)f.obs.size() >= c.max_track_len) long_tracked.push_back(&f);
    }
    lvk_status st;
    if (!ekf_lost.empty()) {                                     // rmLostFeaturesCov (:3296-3348): all lost columns in one gather
        std::vector<char> drop(e->N, 0);
        for (long long id : ekf_lost) drop[LEG + 6 * (int)e->clones.size() + fs_rank(e, id)] = 1;
        if (e->lost_cov_on) { st = lvk_ekf_lost_cov_queue(e, ekf_lost); if (st != LVK_OK) return st; }
        st = cov_drop(e, drop);
        if (st != LVK_OK) return st;
        for (long long id : ekf_lost) {
            const Feature& f = e->map.at(id);                    // lost_slam_features (:3342): kept for getStableMapPointPositions
            lvk_ekf::LostPoint lp = {id, {f.position[0], f.position[1], f.position[2]}, {}};
            for (double& v : lp.cov) v = NAN;
            drain_append(e->lost_slam, lp);
            e->feature_states.erase(e->feature_states.begin() + fs_rank(e, id)); e->map.erase(id);
        }
    }
    if (cells) {                                                 // updateGridMap (:3351-3370)
        std::fill(e->grid_count.begin(), e->grid_count.end(), 0);
        for (long long id : e->feature_states) {
            Feature& f = e->map[id];
            const int oi = f.find(e->imu_id);
            double xy[2] = {0, 0}; if (oi >= 0) { xy[0] = f.obs[oi].z[0]; xy[1] = f.obs[oi].z[1]; }
            const int code = grid_code(e, xy);
            grid_add(e, code, cells);
        }
    }
    st = upload_clones(e);
    if (st != LVK_OK) return st;
    // Two routes consume one triage.  DEVICE-CONSUMED, when no feature can enter the state in this update (the usual message: the
    // augmentation grid is full, or no track has reached max_track_len in a free cell) and the update is not sharded: NOTHING on the
    // host depends on a device result before the update is launched.  The triangulations are queued and consumed on the device by the
    // row kernel (FJ_TRI_PENDING: a failed triangulation = a rejected job = zero rows, which leave the update unchanged), every
    // candidate is a job and has its row slots, and triangulation results, gate results and dx come back in ONE sync.
    // HOST-REPLAYED otherwise: the triangulations are waited for and the candidates replayed in map order, the grid filling while the
    // replay runs.  Same decisions, same rows, same update (larvio.cpp:1897-2005): only the order in which the host learns them differs.
    bool on_device = false;
    if (!e->if_zupt && !e->shard.fn) {
        // can the replay take its EKF branch for anybody (:1945-1960)?  The grid only fills up while it runs, so "nobody now" is final.
        bool admission = false;
        if (e->s.t - e->last_zupt_time > 5 && (int)e->feature_states.size() < c.max_features_in_one_grid * cells)
            for (const Feature* f : long_tracked) {
                const int code = grid_code(e, f->obs[(size_t)f->find(e->imu_id)].z);
                const int gcount = grid_occupancy(e, code, cells);
                if (gcount < c.max_features_in_one_grid) { admission = true; break; }
            }
        on_device = !admission;
    }
    std::vector<Cand> cands; std::vector<TriReq> reqs; std::vector<RowJob> jobs;
    lost_triage(e, !on_device, cands, reqs);
    if (on_device) {
        // Every candidate keeps its row slots on this route, also the ones whose (pending) triangulation will fail - the replay drops
        // those before it stacks.  If the slots could exceed the stacked-row capacity while the rows that survive might still fit,
        // replay on the host (two waits) instead of failing the handle with LVK_ERR_CAPACITY.
        long bound = 2L * (long)ekf_tracked.size(); size_t n_jobs = ekf_tracked.size();
        for (const Cand& cd : cands) if (!cd.invalid) { bound += 2L * (long)cd.f->obs.size() - 3; ++n_jobs; }
        jobs.reserve(n_jobs);
        if (bound > (long)e->hrows && !reqs.empty()) { on_device = false; lost_triage(e, true, cands, reqs); }
    }
    for (const Cand& cd : cands) if (cd.invalid) e->map.erase(cd.f->id);
    // ---- device batch: [new: msckf-form gate | new: ekf rows] [tracked ekf] [msckf]
    std::vector<Feature*> msckf, ekf_new;
    size_t j_ekf = 0, j_msckf = ekf_tracked.size();
    if (on_device) {
        for (Feature* f : ekf_tracked) jobs.push_back(tracked_job(e, f));
        for (const Cand& cd : cands) {
            if (cd.invalid) continue;
            if (cd.idx_pos >= 0) reqs[(size_t)cd.idx_pos].slot = (int)jobs.size();
            jobs.push_back(msckf_job(cd.f, cd.idx_pos));
        }
        if (jobs.empty()) return LVK_OK;
        TR(TR_RLF_PRE);
        st = launch_triangulation(e, reqs);
        if (st != LVK_OK) return st;
        TR(TR_RLF_TRI);
    } else {
        std::vector<TriAns> ans;
        TR(TR_RLF_PRE);
        st = run_triangulation(e, reqs, ans);
        if (st != LVK_OK) return st;
        TR(TR_RLF_TRI);
        for (const Cand& cd : cands) {
            if (cd.invalid) continue;
            Feature& f = *cd.f;
            if (!cd.tracked) {
                if (!f.is_initialized) {
                    apply_tri(&f, 0, ans[(size_t)cd.idx_pos]);
                    if (!ans[(size_t)cd.idx_pos].ok) { e->map.erase(f.id); continue; }      // a lost feature that cannot be triangulated is invalid (:1921-1925)
                }
                msckf.push_back(&f);
                continue;
            }
            const int code = grid_code(e, f.obs[(size_t)f.find(e->imu_id)].z);
            const int gcount = grid_occupancy(e, code, cells);
            if (gcount < c.max_features_in_one_grid && e->s.t - e->last_zupt_time > 5 &&
                (int)(e->feature_states.size() + ekf_new.size()) < c.max_features_in_one_grid * cells) {
                if (!f.ekf_feature) {
                    f.is_initialized = false;
                    if (cd.motion) apply_tri(&f, 2, ans[(size_t)cd.idx_inv]);
                }
                if (!f.is_initialized) continue;
                ekf_new.push_back(&f);
                grid_add(e, code, cells);
            } else {
                if (!f.is_initialized && cd.idx_pos >= 0) apply_tri(&f, 0, ans[(size_t)cd.idx_pos]);
                if (!f.is_initialized) continue;
                msckf.push_back(&f);
            }
        }
        if (msckf.empty() && ekf_new.empty() && ekf_tracked.empty()) return LVK_OK;
        if (e->if_zupt) {
            for (Feature* f : msckf) { f->is_initialized = false; e->map.erase(f->id); }
            TR(TR_RLF_INJ);
            return LVK_OK;
        }
        for (Feature* f : ekf_new) new_feature_jobs(f, jobs);
        j_ekf = jobs.size();
        for (Feature* f : ekf_tracked) jobs.push_back(tracked_job(e, f));
        j_msckf = jobs.size();
        for (Feature* f : msckf) jobs.push_back(msckf_job(f));
    }
    TR(TR_RLF_TRIAGE);
    const int N = e->N;
    const size_t order[2][2] = {{j_msckf, jobs.size()}, {j_ekf, j_msckf}};      // H_o = [H_msckf ; H_ekf], the reference's order (:1612-1626)
    if (ekf_new.empty()) {
        std::vector<double> dx;                         // no feature enters the state: gate results and dx in one sync
        st = gated_update(e, jobs, order, {-1, TR_RLF_UPD, TR_RLF_DX}, dx, nullptr, 0, j_msckf, jobs.size());
        if (st != LVK_OK) return st;
        // used features leave the map (:2240-2246); so does a lost one that cannot be triangulated, while a tracked one waits for more views
        const int accepted = settle_update(e, jobs, order, reqs, 0, [e](const RowJob& j, bool tri_ok) { if (tri_ok || j.f->find(e->imu_id) < 0) e->map.erase(j.f->id); });
        gated_update_apply(e, dx, accepted, 0);
        TR(TR_RLF_INJ);
        return LVK_OK;
    }
    // A feature is about to enter the state: its gate has to be read before the rows are laid out.  Sharded: the (few) new
    // features' jobs run on every rank (their first rows initialise the new covariance columns everywhere, and every rank reads
    // their gate from its own results), the rest is split.  The other jobs' rows all get their slot and the device zeroes the
    // rows of rejected features - exactly as in the branch above - so their gate results travel WITH the compressed blocks:
    // one exchange per update, and the host reads them after the update together with dx.
    // NOTE: the feature column index of a new feature must be its FINAL one (after rejected candidates are dropped);
    // it is not used by JOB_EKF_NEW rows (the feature column never reaches H_o), so any value works here.
    const size_t n_fs_old = e->feature_states.size();
    for (Feature* f : ekf_new) { f->in_state = true; e->feature_states.push_back(f->id); }
    const bool sharded = e->shard.fn != nullptr;
    std::vector<size_t> jb; JobRanges rgs;
    if (sharded) {
        shard_bounds(jobs, j_ekf, jobs.size(), e->shard.world, jb);
        rgs.push_back({0, j_ekf}); rgs.push_back({jb[(size_t)e->shard.rank], jb[(size_t)e->shard.rank + 1]});
        st = launch_feature_rows(e, jobs, &rgs);
        if (st == LVK_OK) st = fetch_feature_results(e, jobs);          // local sync: only jobs [0, j_ekf) are looked at before the exchange
        if (st != LVK_OK) shard_abort(e);                               // the exchange's size depends on those results: cannot post a poisoned block
    } else {
        RowObs obs;
        st = launch_feature_rows(e, jobs, nullptr, &obs);
        if (st == LVK_OK) st = lvk_ekf_msckf_points_queue(e, jobs, j_msckf, jobs.size(), obs);
        if (st == LVK_OK) st = fetch_feature_results(e, jobs);
    }
    if (st != LVK_OK) return st;
    TR(TR_RLF_ROWS);
    // ---- accepted sets and row layout: H_o = [H_msckf ; H_ekf ; top rows of the new block] (:1612-1626).  Sharded, every job keeps
    //      its slot (the device zeroes the rows of a rejected one); unsharded, only the accepted jobs are laid out, as they came back
    std::vector<StackRow> map_o, map_1; std::vector<RowGroup> grp;
    int m = 0;
    for (const auto& rg : order)
        for (size_t k = rg[0]; k < rg[1]; ++k) {
            const RowJob& j = jobs[k];
            if (sharded) { push_rows(map_o, j, job_first_row(j), job_rows(j), m, (int)k, &grp, e, N, shard_owner(jb, k)); m += job_rows(j); continue; }
            if (!gate_ok(e, j)) continue;
            const bool tracked = j.type == JOB_EKF_TRACKED;
            const int first = tracked ? 0 : j.res.first_row, rows = tracked ? 2 : j.res.rows;
            push_rows(map_o, j, first, rows, m, -1, &grp, e, N); m += rows;
            if (!tracked) lvk_ekf_msckf_point_record(e, j, k);
        }
    std::vector<long long> acc_ids; std::vector<double> h2;
    int top = 0;
    for (size_t k = 0; k < j_ekf; k += 2) {
        Feature* f = jobs[k].f;
        if (!gate_ok(e, jobs[k])) { f->in_state = false; continue; }
        const RowJob& j = jobs[k + 1];
        push_rows(map_1, j, 0, 1, (int)acc_ids.size());
        push_rows(map_o, j, 1, j.res.rows, m, -1, &grp, e, N); m += j.res.rows; top += j.res.rows;
        acc_ids.push_back(f->id); h2.push_back(j.res.h2);
    }
    e->feature_states.resize(n_fs_old);
    for (long long id : acc_ids) e->feature_states.push_back(id);
    const int n_acc = (int)acc_ids.size();
    if (m + n_acc > 0) {
        if (m > e->hrows) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "too many measurement rows (%d)", m);
        if (sharded) { st = shard_stage1(e, map_o, grp, N, &jb, &m); e->shard.stats[2]++; }         // the new features' top rows belong to rank 0 (owner 0)
        else st = stack_rows(e, map_o, e->d_H, N, e->d_r);
        if (st == LVK_OK && n_acc) st = stack_rows(e, map_1, e->d_H1, N, e->d_r1);
        if (st != LVK_OK) return st;
        std::vector<double> dx;
        st = dense_update(e, m, dx, n_acc, &grp);
        if (st != LVK_OK) return st;
        if (n_acc) {
            double* hh = up_alloc<double>(e, n_acc);
            if (!hh) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
            memcpy(hh, h2.data(), sizeof(double) * n_acc);
            st = flush_uploads(e);
            if (N + n_acc > e->nmax) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "state dimension exceeds capacity");
            const double* d_hh = dev(e, hh);
            e->redo = [e, N, n_acc, d_hh]() { return lvk_cov_append_features(e->ctx, e->dP[e->cur], e->ld, N, n_acc, e->d_H1, e->ld, d_hh, e->d_r1, e->d_dx, e->sigma2, e->d_tmp, e->d_dx + N); };
            if (st == LVK_OK) st = e->redo();
            if (st != LVK_OK) return st;
        }
        TR(TR_RLF_UPD);
        st = d2h_sync(e, dx.data(), e->d_dx, sizeof(double) * (size_t)(N + n_acc));
        if (st != LVK_OK) return st;
        TR(TR_RLF_DX);
        bool effective = true;
        if (sharded) {                              // every rank's gate results arrived with the blocks (k_shard_unpack wrote the host mirror)
            const FeatResult* ho = (const FeatResult*)(e->h_down + e->down_feat);
            int accepted = top;
            for (size_t k = j_ekf; k < jobs.size(); ++k) { jobs[k].res = ho[k]; if (gate_ok(e, jobs[k])) accepted += k >= j_msckf ? job_rows(jobs[k]) : 2; }
            effective = accepted + n_acc > 0;       // everything gated out: all stacked rows were zero, the update changed nothing (as the unsharded filter, which skips it)
        }
        if (effective) {
            inject(e, dx.data());
            e->N = N + n_acc;
            e->last_update_time = e->s.t;
            e->counters[0]++;
        }
    }
    for (Feature* f : msckf) e->map.erase(f->id);
    TR(TR_RLF_INJ);
    return LVK_OK;
}

// ------------------------------------------------------------------------- pruning (larvio.cpp:2259-2641)
static void find_redundant(lvk_ekf* e, long long* rm)
{
    int key = (int)e->clones.size() - 4, si = key + 1, fi = 0, n = 0;
    double Rk[9]; quat_to_rot(e->clones[key].q_cam, Rk);
    for (int i = 0; i < 2; ++i) {
        const Clone* c = &e->clones[si];
        double R[9], Rt[9], M[9], q[4];
        quat_to_rot(c->q_cam, R); m3_t(R, Rt); m3_mul(Rt, Rk, M);
        double d[3] = {c->p_cam[0] - e->clones[key].p_cam[0], c->p_cam[1] - e->clones[key].p_cam[1], c->p_cam[2] - e->clones[key].p_cam[2]};
        const double distance = v3_norm(d);
        rot_to_quat(M, q);
        const double angle = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), fabs(q[3]));
        if (angle < e->cfg.rotation_threshold && distance < e->cfg.translation_threshold && e->tracking_rate > e->cfg.tracking_rate_threshold) { rm[n++] = c->id; ++si; }
        else { rm[n++] = e->clones[fi].id; ++fi; si -= 2; }
    }
    if (rm[0] > rm[1]) std::swap(rm[0], rm[1]);
}
static long long get_new_anchor_id(lvk_ekf* e, Feature& f, const long long* rm, int nrm)
{   // :3412-3472
    const int size = (int)e->clones.size();
    if (size <= 2) return e->clones[size - 1].id;
    bool valid = false; double min_dis = 99999; long long id_min = 0;
    for (int i = 0; i < size - 2; ++i) {
        const Clone* c = &e->clones[i];
        const int oi = f.find(c->id);
        if (oi < 0) continue;
        bool removed = false; for (int k = 0; k < nrm; ++k) if (rm[k] == c->id) removed = true;
        if (removed) continue;
        double R[9], d[3] = {f.position[0] - c->p_cam[0], f.position[1] - c->p_cam[1], f.position[2] - c->p_cam[2]}, pn[3];
        quat_to_rot(c->q_cam, R); m3t_v(R, d, pn);
        const double a = pn[0] / pn[2] - f.obs[oi].z[0], b = pn[1] / pn[2] - f.obs[oi].z[1];
        const double dis = sqrt(a * a + b * b);
        if (min_dis > dis) { min_dis = dis; id_min = c->id; valid = true; }
    }
    return valid ? id_min : e->clones[size - 1].id;
}
static lvk_status update_feature_cov_1d(lvk_ekf* e, const Feature& f, long long old_id, long long new_id)
{   // :3125-3293 — the row J is built on the host (a few 3x3 products), J P and J P J^T on the device
    const int N = e->N;
    const Clone* co = &e->clones[clone_rank(e, old_id)];
    const Clone* cn = &e->clones[clone_rank(e, new_id)];
    const double* R_b2c = e->R_b2c; const double* t_c_b = e->t_c_b; const double* p_w = f.position;
    double R_b2w_old[9], R_c2w_old[9], R_w2c_old[9];
    quat_to_rot(co->q, R_b2w_old); quat_to_rot(co->q_cam, R_c2w_old); m3_t(R_c2w_old, R_w2c_old);
    double d[3] = {p_w[0] - co->p_cam[0], p_w[1] - co->p_cam[1], p_w[2] - co->p_cam[2]}, p_old_[3], p_old[3];
    m3_v(R_w2c_old, d, p_old_);
    if (e->if_fej) {
        double dd[3] = {f.position_fej[0] - co->p_fej[0], f.position_fej[1] - co->p_fej[1], f.position_fej[2] - co->p_fej[2]}, q[3];
        m3t_v(R_b2w_old, dd, q); q[0] -= t_c_b[0]; q[1] -= t_c_b[1]; q[2] -= t_c_b[2];
        m3_v(R_b2c, q, p_old);
    } else memcpy(p_old, p_old_, 24);
    const double inv_old = 1 / p_old_[2];
    const double f_old[3] = {p_old_[0] / p_old_[2], p_old_[1] / p_old_[2], 1};
    double R_b2w_new[9], R_w2b_new[9], R_c2w_new[9], R_w2c_new[9];
    quat_to_rot(cn->q, R_b2w_new); m3_t(R_b2w_new, R_w2b_new); quat_to_rot(cn->q_cam, R_c2w_new); m3_t(R_c2w_new, R_w2c_new);
    const double inv_new = f.inv_depth;
    double pbo[3], pbn[3];
    for (int i = 0; i < 3; ++i) { pbo[i] = e->if_fej ? f.position_fej[i] - co->p_fej[i] : p_w[i] - co->p[i]; pbn[i] = e->if_fej ? f.position_fej[i] - cn->p_fej[i] : p_w[i] - cn->p[i]; }
    const double J_rho_d_new = -inv_new * inv_new;
    double M[9], Jd_[3]; m3_mul(R_w2c_new, R_c2w_old, M); m3_v(M, f_old, Jd_);
    double So[9], Sn[9], Jto[9], Jtn[9];
    skew3(pbo, So); skew3(pbn, Sn); m3_mul(R_w2c_new, So, Jto); m3_mul(R_w2c_new, Sn, Jtn);
    double v1[3], SkewMx[9], RR[9], R_c2b[9], v2[3], S2[9], Mx[9], D[9], JeT[9], E[9], JeP[9];
    m3_v(R_w2b_new, pbn, v1); v1[0] -= t_c_b[0]; v1[1] -= t_c_b[1]; v1[2] -= t_c_b[2]; skew3(v1, SkewMx);
    m3_mul(R_w2b_new, R_b2w_old, RR);
    m3_t(R_b2c, R_c2b); m3_v(R_c2b, p_old, v2); skew3(v2, S2); m3_mul(RR, S2, Mx);
    for (int i = 0; i < 9; ++i) D[i] = SkewMx[i] - Mx[i];
    m3_mul(R_b2c, D, JeT);
    for (int i = 0; i < 9; ++i) E[i] = RR[i] - ((i % 4 == 0) ? 1.0 : 0.0);
    m3_mul(R_b2c, E, JeP);
    const double J_d_rho_old = -1 / (inv_old * inv_old);
    double* J = up_alloc<double>(e, N);
    if (!J) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memset(J, 0, sizeof(double) * N);
    const int fc = LEG + 6 * (int)e->clones.size() + fs_rank(e, f.id);
    const int oc = LEG + 6 * clone_rank(e, old_id), ncn = LEG + 6 * clone_rank(e, new_id);
    J[fc] = J_rho_d_new * Jd_[2] * J_d_rho_old;
    for (int j = 0; j < 3; ++j) { J[oc + j] = J_rho_d_new * (-Jto[6 + j]); J[oc + 3 + j] = J_rho_d_new * R_w2c_new[6 + j]; }
    for (int j = 0; j < 3; ++j) { J[ncn + j] = J_rho_d_new * Jtn[6 + j]; J[ncn + 3 + j] = J_rho_d_new * (-R_w2c_new[6 + j]); }
    for (int j = 0; j < 3; ++j) { J[15 + j] = J_rho_d_new * JeT[6 + j]; J[18 + j] = J_rho_d_new * JeP[6 + j]; }
    lvk_status st = flush_uploads(e);
    if (st == LVK_OK) st = lvk_cov_reanchor(e->ctx, e->dP[e->cur], e->ld, N, dev(e, J), fc);
    return st;
}

// the feature seen from its new anchor clone: pn = R_cam^T (p - p_cam), inv_depth = 1 / pn.z
static void reanchor_depth(Feature& f, const Clone& cn, double* pn)
{
    double R[9], d[3] = {f.position[0] - cn.p_cam[0], f.position[1] - cn.p_cam[1], f.position[2] - cn.p_cam[2]};
    quat_to_rot(cn.q_cam, R); m3t_v(R, d, pn);
    f.inv_depth = 1 / pn[2];
}
static lvk_status prune_imu_state_buffer(lvk_ekf* e)
{
    long long rm[2]; int nrm = 0;
    if (!e->if_zupt) {
        if ((int)e->clones.size() < e->cfg.sw_size) return LVK_OK;
        find_redundant(e, rm); nrm = 2;
    } else { rm[0] = e->imu_id - 1; nrm = 1; }
    lvk_status st;
    // pass A: re-anchoring (host + rank-1 covariance op) and collection of the features the update uses, with the triangulations they need.
    // Unsharded, those are consumed on the device by the row kernel (FJ_TRI_PENDING, see remove_lost_features): each names the job slot
    // of its feature, and the host reads it together with the gate results and dx, after the update.  Sharded, they are waited for.
    struct Use { Feature* f; std::vector<long long> inv; int tri = -1; };
    std::vector<Use> uses; std::vector<TriReq> reqs; std::vector<TriAns> ans;
    const bool tri_on_device = !e->shard.fn;
    e->tri_ranks.clear(); e->tri_z.clear();
    for (auto kv : e->map) {
        Feature& f = kv.second;
        struct { long long v[2]; int n = 0; void push_back(long long x) { v[n++] = x; } bool empty() const { return n == 0; } size_t size() const { return (size_t)n; }
                 const long long* data() const { return v; } const long long* begin() const { return v; } const long long* end() const { return v + n; } } inv;   // nrm <= 2: no heap traffic per feature
        for (int k = 0; k < nrm; ++k) if (f.find(rm[k]) >= 0) inv.push_back(rm[k]);
        if (inv.empty()) continue;
        const bool anchor_involved = std::find(inv.begin(), inv.end(), f.id_anchor) != inv.end();
        if (f.in_state) {
            if (anchor_involved) {
                const long long new_id = get_new_anchor_id(e, f, inv.data(), (int)inv.size());
                double pn[3]; reanchor_depth(f, e->clones[clone_rank(e, new_id)], pn);
                f.obs_anchor[0] = pn[0] / pn[2]; f.obs_anchor[1] = pn[1] / pn[2];
                st = update_feature_cov_1d(e, f, f.id_anchor, new_id);
                if (st != LVK_OK) return st;
                f.id_anchor = new_id;
            }
        } else {
            if (f.is_initialized && anchor_involved) {
                const long long new_id = get_new_anchor_id(e, f, inv.data(), (int)inv.size());
                double pn[3]; reanchor_depth(f, e->clones[clone_rank(e, new_id)], pn);
                const int oi = f.find(new_id);
                if (oi >= 0) { f.obs_anchor[0] = f.obs[oi].z[0]; f.obs_anchor[1] = f.obs[oi].z[1]; } else { f.obs_anchor[0] = 0; f.obs_anchor[1] = 0; }
                f.id_anchor = new_id;
            }
            if (!e->if_zupt && !f.ekf_feature && inv.size() > 1) {
                Use u; u.f = &f; u.inv.assign(inv.begin(), inv.end());
                if (!f.is_initialized) {
                    if (!feat_check_motion(e, f, f.find(e->imu_id) >= 0)) continue;      // has not moved enough: not used
                    reqs.emplace_back(); make_tri_req(e, &f, 1, &reqs.back()); u.tri = (int)reqs.size() - 1;
                    if (tri_on_device) reqs.back().slot = (int)uses.size();
                }
                uses.push_back(u);
            }
        }
    }
    TR(TR_PR_PRE);
    std::vector<RowJob> jobs;
    if (!uses.empty()) {
        st = upload_clones(e);
        if (st == LVK_OK && !reqs.empty()) st = tri_on_device ? launch_triangulation(e, reqs) : run_triangulation(e, reqs, ans);
        if (st != LVK_OK) return st;
    }
    for (const Use& u : uses) {
        if (u.tri >= 0 && !tri_on_device) { apply_tri(u.f, 1, ans[(size_t)u.tri]); if (!ans[(size_t)u.tri].ok) continue; }
        jobs.push_back(msckf_job(u.f, u.inv, tri_on_device ? u.tri : -1));
    }
    TR(TR_PR_TRI);
    if (!jobs.empty()) {
        // measurementUpdate_msckf (:1420-1602), gate decided on the device (gated_update): one sync for gate + dx, and for
        // initializePosition_AssignAnchor's pending results (:2420-2440)
        std::vector<double> dx;
        const size_t order[2][2] = {{0, jobs.size()}, {0, 0}};
        st = gated_update(e, jobs, order, {TR_PR_ROWS, TR_PR_UPD, TR_PR_DX}, dx, rm, nrm);
        if (st != LVK_OK) return st;
        gated_update_apply(e, dx, settle_update(e, jobs, order, reqs, 1, [](const RowJob&, bool) {}), 1);
    } else drop_observations(e, rm, nrm);
    {   // both clones' rows/columns leave P in ONE gather (the reference deletes them one after the other, :2563-2638)
        std::vector<char> drop(e->N, 0);
        bool any = false;
        for (int k = 0; k < nrm; ++k) {
            const int seq = clone_rank(e, rm[k]);
            if (seq < 0) continue;
            for (int j = 0; j < 6; ++j) drop[LEG + 6 * seq + j] = 1;
            any = true;
        }
        if (any) {
            if (e->keyframes_on) { st = lvk_ekf_keyframes_queue(e, rm, nrm); if (st != LVK_OK) return st; }
            st = cov_drop(e, drop);
            if (st != LVK_OK) return st;
            for (int k = 0; k < nrm; ++k) { const int seq = clone_rank(e, rm[k]); if (seq >= 0) { e->clones.erase(e->clones.begin() + seq); e->ranks_dirty = true; e->rcam_valid = false; } }
        }
    }
    return LVK_OK;
}

// ------------------------------------------------------------------------- ZUPT (larvio.cpp:2751-2962)
static lvk_status update_zupt(lvk_ekf* e)
{
    const int N = e->N, n = (int)e->clones.size();
    double* H = up_alloc<double>(e, (size_t)9 * e->ld); double* r = up_alloc<double>(e, 16);
    if (!H || !r) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memset(H, 0, sizeof(double) * 9 * e->ld);
    for (int i = 0; i < 3; ++i) {
        H[(size_t)i * e->ld + 3 + i] = 1.0;
        H[(size_t)(3 + i) * e->ld + LEG + 6 * n - 3 + i] = 1.0; H[(size_t)(3 + i) * e->ld + LEG + 6 * n - 9 + i] = -1.0;
        H[(size_t)(6 + i) * e->ld + LEG + 6 * n - 6 + i] = -0.5; H[(size_t)(6 + i) * e->ld + LEG + 6 * n - 12 + i] = 0.5;
    }
    const Clone* cc = &e->clones[clone_rank(e, e->imu_id)]; const Clone* cp = &e->clones[clone_rank(e, e->imu_id - 1)];
    for (int i = 0; i < 3; ++i) { r[i] = -e->s.v[i]; r[3 + i] = -(cc->p[i] - cp->p[i]); }
    double qpc[4] = {-cp->q[0], -cp->q[1], -cp->q[2], cp->q[3]}, dq[4];
    quat_mul(cc->q, qpc, dq);
    r[6] = dq[0]; r[7] = dq[1]; r[8] = dq[2];
    // rows are whitened by sigma/sqrt(R_ii) so the shared isotropic update applies (K r and K H are unchanged)
    const double Rd[9] = {e->zupt_v2, e->zupt_v2, e->zupt_v2, e->zupt_p2, e->zupt_p2, e->zupt_p2, e->zupt_q2, e->zupt_q2, e->zupt_q2};
    for (int i = 0; i < 9; ++i) { const double s = sqrt(e->sigma2 / Rd[i]); for (int j = 0; j < N; ++j) H[(size_t)i * e->ld + j] *= s; r[i] *= s; }
    lvk_status st = flush_uploads(e);
    if (st == LVK_OK) { EKF_HIP(hipMemcpyAsync(e->d_H, dev(e, H), sizeof(double) * 9 * e->ld, hipMemcpyDeviceToDevice, e->ctx->stream));
                        EKF_HIP(hipMemcpyAsync(e->d_r, dev(e, r), sizeof(double) * 9, hipMemcpyDeviceToDevice, e->ctx->stream)); }
    std::vector<double> dx;
    if (st == LVK_OK) st = dense_update(e, 9, dx, 0);
    if (st == LVK_OK) st = d2h_sync(e, dx.data(), e->d_dx, sizeof(double) * (size_t)N);
    if (st != LVK_OK) return st;
    inject(e, dx.data());
    e->last_update_time = e->s.t; e->last_zupt_time = e->s.t;
    e->counters[3]++;
    return LVK_OK;
}
static lvk_status check_zupt(lvk_ekf* e, bool* out)
{
    *out = false;
    if (e->coarse_dis.size() < 20) { e->coarse_dis.clear(); return LVK_OK; }
    // the reference sorts the whole list and reads one order statistic (larvio.cpp:2759-2761): nth_element gives the same value
    std::nth_element(e->coarse_dis.begin(), e->coarse_dis.end() - 9, e->coarse_dis.end());
    const double max_dis = e->coarse_dis[e->coarse_dis.size() - 9];
    e->coarse_dis.clear();
    if (max_dis < e->cfg.zupt_max_feature_dis) {
        if (!e->feature_states.empty()) {
            lvk_status st = cov_delete(e, e->N - (int)e->feature_states.size(), (int)e->feature_states.size());
            if (st != LVK_OK) return st;
            for (long long id : e->feature_states) { Feature& f = e->map[id]; f.is_initialized = false; f.ekf_feature = false; f.in_state = false; }
            e->feature_states.clear();
        }
        lvk_status st = update_zupt(e);
        if (st != LVK_OK) return st;
        *out = true;
    }
    return LVK_OK;
}

// ------------------------------------------------------------------------- static initializer (StaticInitializer.cpp:12-163)
static bool static_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased)
{
    *n_erased = 0;
    auto snapshot = [&]() { e->init_features.clear(); for (int i = 0; i < n; ++i) e->init_features[(long long)f[i].id] = std::make_pair(f[i].u, f[i].v); };
    if (e->static_counter == 0) { e->static_counter++; snapshot(); e->lower_time_bound = ts + e->td; return false; }
    std::vector<double> dis;
    for (int i = 0; i < n; ++i) { auto it = e->init_features.find((long long)f[i].id); if (it != e->init_features.end()) { double dx = f[i].u - it->second.first, dy = f[i].v - it->second.second; dis.push_back(sqrt(dx * dx + dy * dy)); } }
    if (dis.size() < 20) { e->static_counter = 0; return false; }
    std::sort(dis.begin(), dis.end());
    const double max_dis = dis[dis.size() - 19];
    if (max_dis < e->cfg.zupt_max_feature_dis) { e->static_counter++; snapshot(); if (e->static_counter < e->static_num) return false; }
    else { e->static_counter = 0; return false; }
    const double time_bound = ts + e->td;
    double sw[3] = {0, 0, 0}, sa[3] = {0, 0, 0}; int cnt = 0; double last_t = 0;
    for (int i = 0; i < n_imu; ++i) {
        if (imu[i].t < e->lower_time_bound) continue;
        if (imu[i].t > time_bound) break;
        {   // Tg (w - As Ma a) and Ma a (StaticInitializer.cpp:84-85): the identity / zero matrices of a filter that does not calibrate them change no bit
            double la[3], t3[3], w[3], ga[3];
            m3_v(e->Ma, imu[i].acc, la); m3_v(e->As, la, t3);
            for (int k = 0; k < 3; ++k) w[k] = imu[i].gyro[k] - t3[k];
            m3_v(e->Tg, w, ga);
            for (int k = 0; k < 3; ++k) { sw[k] += ga[k]; sa[k] += la[k]; }
        }
        cnt++; last_t = imu[i].t;
    }
    double gi[3];
    for (int k = 0; k < 3; ++k) { e->s.bg[k] = sw[k] / cnt; gi[k] = sa[k] / cnt; }
    const double gn = v3_norm(gi);
    {   // Quaterniond::FromTwoVectors(gravity_imu, (0,0,|g|))
        double v0[3] = {gi[0] / gn, gi[1] / gn, gi[2] / gn}, v1[3] = {0, 0, 1.0};
        const double cdot = v1[0] * v0[0] + v1[1] * v0[1] + v1[2] * v0[2];
        double ax[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
        const double s = sqrt((1 + cdot) * 2), invs = 1 / s;
        e->s.q[0] = ax[0] * invs; e->s.q[1] = ax[1] * invs; e->s.q[2] = ax[2] * invs; e->s.q[3] = s * 0.5;
    }
    e->s.t = last_t;
    memset(e->s.p, 0, 24); memset(e->s.v, 0, 24); memset(e->s.ba, 0, 24);
    int useful = 0;
    for (int i = 0; i < n_imu; ++i) { if (imu[i].t > last_t) break; useful++; }
    if (useful >= n_imu) useful--;
    memcpy(e->m_gyro_old, imu[useful].gyro, 24); memcpy(e->m_acc_old, imu[useful].acc, 24);
    *n_erased = useful;
    return true;
}

// ------------------------------------------------------------------------- dynamic initializer (DynamicInitializer.cpp, be_init.h)
// cv::findFundamentalMat (mask and matrix) from the library's own kernel (fe_track.hip).  Its device buffers live in the filter
// (grow-only, freed with it): with a full window this runs on every message for up to ten candidate frames, and a hipFree per
// attempt would synchronise the whole device under the front-end's streams.  A pair list beyond the kernel's capacity (no front-end
// of this library produces one) is "no relative pose from this frame", not a failure of the handle.
static bool dyn_ransac(void* user, const std::vector<lvk_init::Pt2>& ll, const std::vector<lvk_init::Pt2>& rr, double thresh, double conf, std::vector<unsigned char>& mask, double* F)
{
    lvk_ekf* e = (lvk_ekf*)user;
    const int n = (int)ll.size();
    e->init_ransac_calls += 1;
    mask.assign((size_t)n, 0);
    if (n > 4096) return false;                                          // FM_MAX_N (fe_track_dev.h)
    std::vector<lvk_pt2f> h((size_t)2 * n);
    for (int i = 0; i < n; ++i) { h[(size_t)i] = lvk_pt2f{(float)ll[(size_t)i].x, (float)ll[(size_t)i].y}; h[(size_t)n + i] = lvk_pt2f{(float)rr[(size_t)i].x, (float)rr[(size_t)i].y}; }
    const size_t off_mask = sizeof(lvk_pt2f) * 2 * (size_t)n, off_info = (off_mask + (size_t)n + 15) & ~(size_t)15, off_F = off_info + 16, need = off_F + 9 * sizeof(double);
    bool ok = true;
    if (need > e->dyn_cap) {
        if (e->d_dyn) { hipStreamSynchronize(e->ctx->stream); hipFree(e->d_dyn); e->d_dyn = nullptr; e->dyn_cap = 0; }
        const size_t cap = std::max(need, (size_t)64 * 1024);
        ok = hipMalloc((void**)&e->d_dyn, cap) == hipSuccess;
        if (ok) e->dyn_cap = cap; else (void)hipGetLastError();
    }
    int info[2] = {0, 0};
    if (ok) {
        lvk_pt2f* d_p = (lvk_pt2f*)e->d_dyn; uint8_t* d_mask = (uint8_t*)(e->d_dyn + off_mask); int* d_info = (int*)(e->d_dyn + off_info); double* d_F = (double*)(e->d_dyn + off_F);
        ok = hipMemcpyAsync(d_p, h.data(), sizeof(lvk_pt2f) * 2 * n, hipMemcpyHostToDevice, e->ctx->stream) == hipSuccess;
        ok = ok && lvk_find_fundamental(e->ctx, d_p, d_p + n, n, thresh, conf, d_mask, d_info, d_F) == LVK_OK;
        ok = ok && hipMemcpyAsync(mask.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, e->ctx->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, e->ctx->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(F, d_F, 9 * sizeof(double), hipMemcpyDeviceToHost, e->ctx->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(e->ctx->stream) == hipSuccess;
    }
    if (!ok) e->dyn_status = lvk_set_error(e->ctx, LVK_ERR_DEVICE, "dynamic initialiser: RANSAC stage failed on the device");
    return ok && info[0] == 1;
}
static bool dynamic_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased)
{
    *n_erased = 0;
    if (!e->dyn) {                                       // DynamicInitializer's constructor (DynamicInitializer.h:40-75, larvio.cpp:343-349)
        e->dyn = new lvk_init::DynInit();
        lvk_init::DynInit& d = *e->dyn;
        d.reset();
        d.td = e->td; d.imu_img_time_th = e->imu_img_time_th;
        m3_t(e->R_b2c, d.RIC); memcpy(d.TIC, e->t_c_b, 24);
        memcpy(d.Ma, e->Ma, 72); memcpy(d.Tg, e->Tg, 72); memcpy(d.As, e->As, 72);
        d.ransac = dyn_ransac; d.ransac_user = e;
    }
    lvk_init::DynInit& d = *e->dyn;
    const int call = e->init_calls++;
    if (!d.try_init(ts, f, n, imu, n_imu, n_erased)) return false;
    {
        lvk_init_report& r = e->init_report; memset(&r, 0, sizeof r);
        r.valid = 1; r.message = call; r.attempts = d.diag.attempts; r.ransac_calls = e->init_ransac_calls; r.l = d.diag.l; r.n_points = d.diag.n_points; r.erase = *n_erased;
        r.state_time = d.out.state_time; r.scale = d.diag.scale;
        memcpy(r.rel_R, d.diag.relR, 72); memcpy(r.rel_T, d.diag.relT, 24);
        for (size_t i = 0; i < d.diag.sfm_R.size() && i < 11; ++i) { memcpy(r.sfm_R + 9 * i, d.diag.sfm_R[i].data(), 72); memcpy(r.sfm_T + 3 * i, d.diag.sfm_T[i].data(), 24); }
        memcpy(r.bg, d.out.bg, 24); memcpy(r.g, d.diag.g, 24); memcpy(r.q, d.out.q, 32); memcpy(r.v, d.out.v, 24);
    }
    e->s.t = d.out.state_time;
    memcpy(e->s.q, d.out.q, 32); memcpy(e->s.p, d.out.p, 24); memcpy(e->s.v, d.out.v, 24); memcpy(e->s.bg, d.out.bg, 24); memcpy(e->s.ba, d.out.ba, 24);
    memcpy(e->m_gyro_old, d.out.last_gyro, 24); memcpy(e->m_acc_old, d.out.last_acc, 24);
    return true;
}

// ------------------------------------------------------------------------- C ABI
template <typename T> static bool dalloc(T** p, size_t n) { return hipMalloc((void**)p, sizeof(T) * (n ? n : 1)) == hipSuccess; }

extern "C" {

void lvk_ekf_destroy(lvk_ekf* e)
{
    if (!e) return;
    if (e->async) {
        ekf_quiesce(e);
        { std::lock_guard<std::mutex> lk(e->async->mu); e->async->stop.store(true); }
        e->async->cv.notify_all();
        if (e->async->th.joinable()) e->async->th.join();
        delete e->async; e->async = nullptr;
    }
    hipStreamSynchronize(e->ctx->stream);
    for (auto& pe : e->prof_pending) { hipEventDestroy(pe.a); hipEventDestroy(pe.b); }
    for (hipEvent_t ev : e->prof_free) hipEventDestroy(ev);
    if (g_tr.on && g_tr.n > 0) {
        double tot = 0; for (int i = 0; i < TR_N; ++i) tot += g_tr.acc[i];
        fprintf(stderr, "[lvk_ekf trace] %ld updates, %.1f us/update host wall\n", g_tr.n, tot / g_tr.n);
        for (int i = 0; i < TR_N; ++i) fprintf(stderr, "  %-28s %8.1f us\n", TR_NAMES[i], g_tr.acc[i] / g_tr.n);
        for (int i = 0; i < 8; ++i) if (g_tr.sub_acc[i] > 0) fprintf(stderr, "    [%s] %.1f us\n", TRS_NAMES[i], g_tr.sub_acc[i] / g_tr.n);
        fprintf(stderr, "    updates above 160 rows: %ld (mean %.0f rows), compression plans drawn up: %ld, taken: %ld\n", g_tr.cnt[0], g_tr.cnt[0] ? (double)g_tr.cnt[3] / g_tr.cnt[0] : 0.0, g_tr.cnt[1], g_tr.cnt[2]);
        g_tr = EkfTrace();
    }
    void* ptrs[] = {e->dP[0], e->dP[1], e->d_idx, e->d_phiq, e->d_J, e->d_dx, e->d_tmp, e->d_tri, e->d_tridev, e->d_fj, e->d_fout, e->d_rank, e->d_z, e->d_zv,
                    e->d_cams, e->d_clones, e->d_staging, e->d_ccols, e->d_map, e->d_H, e->d_r, e->d_Hb, e->d_rb, e->d_H1, e->d_H2, e->d_r1, e->ws.B, e->ws.S, e->ws.info, e->zero_copy ? nullptr : (void*)e->d_up};
    for (void* p : ptrs) if (p) hipFree(p);
    if (e->h_up) hipHostFree(e->h_up);
    if (e->h_down) hipHostFree(e->h_down);
    if (e->shard.d_send) hipFree(e->shard.d_send);
    if (e->shard.d_recv) hipFree(e->shard.d_recv);
    if (e->d_dyn) hipFree(e->d_dyn);
    delete e->dyn;
    delete e;
}

static lvk_status ekf_process_guarded(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated,
                                      lvk_feats_fn fetch, void* fetch_user);
lvk_status lvk_ekf_create(lvk_context* ctx, const lvk_ekf_config* cfg, lvk_ekf** out)
{
    if (!ctx || !cfg || !out) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_create: bad argument");
    if (cfg->feature_idp_dim != 1 || cfg->use_schmidt != 0 || (cfg->calib_imu_instrinsic != 0 && cfg->calib_imu_instrinsic != 1))
        return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "only feature_idp_dim 1, use_schmidt 0, calib_imu_instrinsic 0/1 are implemented");
    if (cfg->sw_size < 5 || cfg->sw_size > 62) return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "sw_size must be in 5..62");
    g_tr.on = getenv("LVK_EKF_TRACE") != nullptr;
    lvk_ekf* e = new (std::nothrow) lvk_ekf();
    if (!e) return LVK_ERR_DEVICE;
    e->ctx = ctx; e->cfg = *cfg; e->process = ekf_process_guarded;
    const lvk_ekf_config& c = e->cfg;
    e->leg = c.calib_imu_instrinsic ? 46 : 22;
    memset(e->imx, 0, sizeof e->imx);
    for (int i = 0; i < 3; ++i) { e->imx[3 + i] = 1.0; e->imx[21 + i] = 1.0; }      // Tg = Ma = I, As = 0 (larvio.cpp:129-131)
    update_imu_mx(e);
    e->td = c.td;
    e->sigma2 = c.noise_feature * c.noise_feature;
    e->zupt_v2 = c.zupt_noise_v * c.zupt_noise_v; e->zupt_p2 = c.zupt_noise_p * c.zupt_noise_p; e->zupt_q2 = c.zupt_noise_q * c.zupt_noise_q;
    e->imu_img_time_th = 1.0 / (2 * c.imu_rate);
    for (int i = 0; i < 3; ++i) { e->Qc[i] = c.noise_gyro * c.noise_gyro; e->Qc[3 + i] = c.noise_acc * c.noise_acc; e->Qc[6 + i] = c.noise_gyro_bias * c.noise_gyro_bias; e->Qc[9 + i] = c.noise_acc_bias * c.noise_acc_bias; }
    memset(&e->s, 0, sizeof e->s); e->s.q[3] = 1.0; e->s_old = e->s; e->s_fej_now = e->s; e->s_fej_old = e->s;
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) R[i * 3 + j] = c.T_cam_imu[i * 4 + j]; t[i] = c.T_cam_imu[i * 4 + 3]; }
    memcpy(e->R_b2c, R, sizeof R);
    double a[3]; m3t_v(R, t, a);
    for (int i = 0; i < 3; ++i) e->t_c_b[i] = -a[i];
    const double fx = c.intrinsics[0], fy = c.intrinsics[1], cx = c.intrinsics[2], cy = c.intrinsics[3];
    e->x_min = -cx / fx; e->y_min = -cy / fy;
    const double x_max = (c.width - cx) / fx, y_max = (c.height - cy) / fy;
    const int cells = c.aug_grid_rows * c.aug_grid_cols;
    if (cells != 0) { e->grid_w = (x_max - e->x_min) / c.aug_grid_cols; e->grid_h = (y_max - e->y_min) / c.aug_grid_rows; }
    else { e->grid_w = x_max - e->x_min; e->grid_h = y_max - e->y_min; }
    e->grid_count.assign((size_t)cells + 1, 0);
    e->grid_phantom.clear();
    e->reference_grid = c.legacy_grid == 0;
    if (const char* g = getenv("LVK_GRID_REFERENCE")) e->reference_grid = atoi(g) != 0;
    e->static_num = (int)((float)c.static_duration * (double)c.pub_frequency);
    // capacities
    const int max_feat_state = std::max(0, c.max_features_in_one_grid) * cells;
    e->nmax = LEG + 6 * (c.sw_size + 2) + max_feat_state + 8;
    e->ld = ((e->nmax + 15) & ~15) + 8;                  // not a power of two: see ws.lds
    e->rows_cap = 1024;                                      // dense update up to this many stacked rows; taller blocks are QR-compressed first
    e->feat_cap = std::max(1024, 4 * c.max_features);        // jobs per batch: the map holds lost and young features besides the tracked ones
    e->obs_cap = 2 * e->feat_cap * (c.sw_size + 2);
    e->staging_cap = std::min((size_t)2 * e->feat_cap * (size_t)fj_stage_doubles(JOB_EKF_NEW, c.sw_size + 2), (size_t)48 << 20);   // doubles; checked per batch
    e->ccols_cap = (size_t)2 * e->feat_cap * fj_cols(JOB_EKF_NEW, c.sw_size + 2);
    // stacked rows before compression: every feature of a message can contribute 2M-3 rows (18,000 at 2000 tracks, M = 6).
    // The row kernel's direct output relies on it: d_H / d_r have hrows rows and k_feature_rows does not bound FeatJob::dst_row1,
    // so gated_update refuses a layout of more rows.  (A pruning update cannot get there: one row per job, at most 2 * feat_cap jobs
    // per batch, and 2 * feat_cap = max(2048, 8 * max_features) <= hrows.)
    e->hrows = std::max(8 * e->rows_cap, 12 * c.max_features);
    const size_t hrows = (size_t)e->hrows;
    bool ok = dalloc(&e->dP[0], (size_t)e->ld * e->ld) && dalloc(&e->dP[1], (size_t)e->ld * e->ld) && dalloc(&e->d_idx, e->ld) && dalloc(&e->d_phiq, 2 * LEG_MAX * LEG_MAX) &&
              dalloc(&e->d_J, e->ld) && dalloc(&e->d_dx, e->ld + 64) && dalloc(&e->d_tmp, (size_t)64 * e->ld) &&
              dalloc(&e->d_tri, (size_t)2 * e->feat_cap) && dalloc(&e->d_tridev, (size_t)2 * e->feat_cap) && dalloc(&e->d_fj, (size_t)2 * e->feat_cap) && dalloc(&e->d_fout, (size_t)2 * e->feat_cap) &&
              dalloc(&e->d_rank, e->obs_cap) && dalloc(&e->d_z, (size_t)2 * e->obs_cap) && dalloc(&e->d_zv, (size_t)2 * e->obs_cap) &&
              dalloc(&e->d_cams, c.sw_size + 4) && dalloc(&e->d_clones, c.sw_size + 4) && dalloc(&e->d_staging, e->staging_cap) && dalloc(&e->d_ccols, e->ccols_cap) &&
              dalloc(&e->d_map, hrows) && dalloc(&e->d_H, hrows * e->ld) && dalloc(&e->d_r, hrows) && dalloc(&e->d_Hb, hrows * e->ld) && dalloc(&e->d_rb, hrows) && dalloc(&e->d_H1, (size_t)64 * e->ld) && dalloc(&e->d_H2, 64) && dalloc(&e->d_r1, 64);
    e->ws.ldb = ((e->ld + 8 + 7) & ~7) | 8; e->ws.lds = e->rows_cap + 8;      // odd multiples of 64 B: power-of-two row strides pile onto one L2 channel
    ok = ok && dalloc(&e->ws.B, (size_t)e->rows_cap * e->ws.ldb) && dalloc(&e->ws.S, (size_t)e->rows_cap * e->ws.lds);
    e->up_cap = (size_t)64 << 20; e->up_lim = e->up_cap / 2;     // two halves, alternating per call (ekf_process_impl)
    e->down_feat = (sizeof(TriResult) * (size_t)2 * e->feat_cap + 255) & ~(size_t)255;
    e->down_dx = (e->down_feat + sizeof(FeatResult) * (size_t)2 * e->feat_cap + 255) & ~(size_t)255;
    e->down_flag = (e->down_dx + sizeof(double) * (size_t)(e->ld + 64) + 255) & ~(size_t)255;
    e->down_info = e->down_flag + 256;                  // [0] first non-positive Cholesky pivot (+1), [1] a solver workgroup gave up waiting: written by k_chol_fused
    e->down_p00 = e->down_info + 256;                   // 16 x 16 doubles
    e->down_lm = e->down_p00 + 2048;                    // lvk_ekf_set_lost_feature_cov: 9 doubles per lost in-state feature of one update
    e->lm_cap = max_feat_state + 8;
    e->down_mp = e->down_lm + ((sizeof(double) * 9 * (size_t)e->lm_cap + 255) & ~(size_t)255);     // lvk_ekf_set_msckf_points: 9 doubles + an ok word per MSCKF job of one update
    e->mp_cap = 2 * e->feat_cap;
    e->down_mpok = e->down_mp + ((sizeof(double) * 9 * (size_t)e->mp_cap + 255) & ~(size_t)255);
    e->down_kf = e->down_mpok + ((sizeof(int) * (size_t)e->mp_cap + 255) & ~(size_t)255);         // lvk_ekf_set_keyframe_export: 2 x 36 doubles per removed clone, two clones per pruning
    e->down_cap = e->down_kf + 4 * 36 * sizeof(double);
    ok = ok && hipHostMalloc((void**)&e->h_up, e->up_cap) == hipSuccess && hipHostMalloc((void**)&e->h_down, e->down_cap) == hipSuccess;
    if (ok) {
        // No copy commands on the filter's chain (each ~8 us of API + copy + barrier; ten of them were 385 -> 336 us per update):
        // what the kernels write for the host (results, dx) goes to device-mapped pinned memory, and what the host stages for the
        // kernels goes the other way round - since round 4 into DEVICE memory that this thread writes through the PCIe BAR (every
        // MI355X host maps the whole HBM: hipDeviceAttributeIsLargeBar).  The first read of staged data by a workgroup is then an HBM
        // access (~1 us) instead of a PCIe round trip to host memory (2-3 us each, three dependent ones in k_feature_rows, and ~23 GB/s
        // in total for tables every workgroup reads): tools/gpu/bar_probe.hip.  Staging is built in a host shadow (h_up, patched until
        // the launch) and pushed with one sequential copy + sfence per launch group (flush_uploads).  Without a large BAR the kernels
        // read the pinned shadow in place as before.
        if (void* da = lvk_bar_alloc(ctx->device, e->up_cap)) { e->d_up = (char*)da; e->bar_push = true; }
        void* dp = nullptr;
        if (!e->bar_push) { ok = hipHostGetDevicePointer(&dp, e->h_up, 0) == hipSuccess && dp; e->d_up = (char*)dp; e->zero_copy = ok; }
        void* dd = nullptr;
        ok = ok && hipHostGetDevicePointer(&dd, e->h_down, 0) == hipSuccess && dd; e->dh_down = (char*)dd;
        e->d_triout = (TriResult*)e->dh_down;
        e->ws.info_host = (int*)(e->dh_down + e->down_info); memset(e->h_down + e->down_info, 0, 256);
        ok = ok && hipMalloc((void**)&e->ws.info, 64) == hipSuccess && hipMemset(e->ws.info, 0, 64) == hipSuccess;
    }
    if (!ok) { lvk_ekf_destroy(e); return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_ekf_create: allocation failed"); }
    // initial covariance (larvio.cpp:163-186)
    std::vector<double> P0((size_t)e->ld * e->ld, 0.0);
    for (int i = 0; i < 3; ++i) {
        P0[(size_t)i * e->ld + i] = c.initial_covariance_orientation; P0[(size_t)(3 + i) * e->ld + 3 + i] = c.initial_covariance_velocity;
        P0[(size_t)(6 + i) * e->ld + 6 + i] = c.initial_covariance_position; P0[(size_t)(9 + i) * e->ld + 9 + i] = c.initial_covariance_gyro_bias;
        P0[(size_t)(12 + i) * e->ld + 12 + i] = c.initial_covariance_acc_bias;
        if (c.estimate_extrin) { P0[(size_t)(15 + i) * e->ld + 15 + i] = c.initial_covariance_extrin_rot; P0[(size_t)(18 + i) * e->ld + 18 + i] = c.initial_covariance_extrin_trans; }
    }
    if (c.estimate_td) P0[(size_t)21 * e->ld + 21] = 4e-6;
    if (c.calib_imu_instrinsic) for (int i = 22; i < 46; ++i) P0[(size_t)i * e->ld + i] = 1e-4;      // :183-186
    if (hipMemcpy(e->dP[0], P0.data(), sizeof(double) * P0.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(e->dP[1], 0, sizeof(double) * P0.size(), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { lvk_ekf_destroy(e); return lvk_set_error(ctx, LVK_ERR_DEVICE, "covariance upload failed"); }
    e->N = LEG; e->cur = 0;
    *out = e;
    return LVK_OK;
}

lvk_status lvk_ekf_set_state(lvk_ekf* e, double t, const double q[4], const double p[3], const double v[3], const double bg[3], const double ba[3],
                             const double gyro_old[3], const double acc_old[3])
{
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    e->s.t = t; memcpy(e->s.q, q, 32); memcpy(e->s.p, p, 24); memcpy(e->s.v, v, 24); memcpy(e->s.bg, bg, 24); memcpy(e->s.ba, ba, 24);
    memcpy(e->m_gyro_old, gyro_old, 24); memcpy(e->m_acc_old, acc_old, 24);
    e->is_gravity_set = true; e->b_first_features = true;
    e->take_off_stamp = t; e->last_zupt_time = t - 10.0; e->last_update_time = t;     // initializer bypass: EKF-SLAM features allowed at once
    e->s_fej_now = e->s;
    return LVK_OK;
}

// feats == nullptr && fetch != nullptr: the message is collected through fetch() as late as the algorithm allows - after the IMU
// samples have been integrated and the propagation / augmentation kernels are queued - so that a pipelined driver overlaps that
// work with the front-end that is still producing the message (the static initializer needs the message first and asks at once).
// event brackets of the profiled launches (lvk_ekf_profile): harvested when both events have fired (all = after a stream sync)
static void prof_harvest(lvk_ekf* e, bool all)
{
    size_t w = 0;
    for (size_t i = 0; i < e->prof_pending.size(); ++i) {
        auto pe = e->prof_pending[i];
        if (!all && hipEventQuery(pe.b) != hipSuccess) { (void)hipGetLastError(); e->prof_pending[w++] = pe; continue; }      // (hipErrorNotReady is not an error: keep it out of the next launch check)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            if (pe.kind == 0) { e->prof_ms += ms; e->prof_flops += pe.flops; e->prof_n += 1; }
            else { e->prof_qr_ms += ms; e->prof_qr_flops += pe.flops; e->prof_qr_rows += pe.rows; e->prof_qr_n += 1; }
        }
        e->prof_free.push_back(pe.a); e->prof_free.push_back(pe.b);
    }
    e->prof_pending.resize(w);
}
static lvk_status ekf_process_impl(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated,
                                   lvk_feats_fn fetch, void* fetch_user);

lvk_status lvk_ekf_process(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated)
{
    if (n_feats > 0 && !feats) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_process: bad argument");
    if (e) ekf_quiesce(e);
    return ekf_process_guarded(e, ts, feats, n_feats, imu, n_imu, n_consumed, updated, nullptr, nullptr);
}

static void ekf_async_worker(lvk_ekf* e)
{
    hipSetDevice(e->ctx->device);
    lvk_ekf::Async* a = e->async;
    for (;;) {
        for (int spin = 0; spin < 40000 && a->state.load(std::memory_order_acquire) != 1 && !a->stop.load(); ++spin) LVK_CPU_RELAX();
        {
            std::unique_lock<std::mutex> lk(a->mu);
            a->cv.wait(lk, [&] { return a->stop.load() || a->state.load(std::memory_order_acquire) == 1; });
            if (a->stop.load()) return;
        }
        int used = 0, upd = 0;
        lvk_status st = ekf_process_guarded(e, a->ts, a->feats.data(), (int)a->feats.size(), a->imu.data(), (int)a->imu.size(), &used, &upd, nullptr, nullptr);
        if (st == LVK_OK && used != a->expect_used) {
            st = lvk_set_error(e->ctx, LVK_ERR_DEVICE, "internal: the deferred update consumed %d IMU samples, %d were announced", used, a->expect_used);
            e->failed = st; snprintf(e->failed_msg, sizeof e->failed_msg, "%s", e->ctx->err);
        }
        { std::lock_guard<std::mutex> lk(a->mu); a->st = st; a->updated = upd; a->state.store(0, std::memory_order_release); }
        a->cv.notify_all();
    }
}

lvk_status lvk_ekf_process_async(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* will_update)
{
    if (!e || !n_consumed || !will_update || (n_feats > 0 && !feats) || (n_imu > 0 && !imu)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_process_async: bad argument");
    ekf_quiesce(e);
    // Cold paths (before the first usable IMU sample, the static initializer, a failed filter) decide their return value from the
    // message itself: they run here, synchronously.  Once the filter is initialized an update always consumes the samples up to
    // ts + td (a count that depends on time stamps, the state time and td only - all final now) and always reports `true`.
    if (!e->b_first_features || !e->is_gravity_set || e->failed != LVK_OK)
        return ekf_process_guarded(e, ts, feats, n_feats, imu, n_imu, n_consumed, will_update, nullptr, nullptr);
    if (!e->async) {
        e->async = new (std::nothrow) lvk_ekf::Async();
        if (!e->async) return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "lvk_ekf_process_async: out of memory");
        e->async->th = std::thread(ekf_async_worker, e);
    }
    lvk_ekf::Async* a = e->async;
    *n_consumed = batch_imu_count(e, ts + e->td, imu, n_imu);
    *will_update = 1;
    a->ts = ts; a->feats.assign(feats, feats + n_feats); a->imu.assign(imu, imu + n_imu); a->expect_used = *n_consumed;
    { std::lock_guard<std::mutex> lk(a->mu); a->st = LVK_OK; a->updated = 0; a->n_deferred += 1; a->unwaited = true; a->state.store(1, std::memory_order_release); }
    a->cv.notify_all();
    return LVK_OK;
}

lvk_status lvk_ekf_wait(lvk_ekf* e, int* updated)
{
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (updated) *updated = e->async ? e->async->updated : 0;
    if (e->async && e->async->st != LVK_OK) return e->async->st;
    return LVK_OK;
}

static lvk_status ekf_process_guarded(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated,
                                      lvk_feats_fn fetch, void* fetch_user)
{
    if (!e || !n_consumed || !updated || (n_imu > 0 && !imu)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_process: bad argument");
    *n_consumed = 0; *updated = 0;
    // An update that failed half way (capacity, device error) leaves clone list, feature map and covariance layout out of step with
    // each other: the handle stays failed and says so, instead of computing on with wrong column offsets.
    if (e->failed != LVK_OK) {
        if (e->on_consumed) e->on_consumed(e->on_consumed_user, 0);      // a pipelined driver counts every job's consumption, also the refused ones
        return lvk_set_error(e->ctx, e->failed, "lvk_ekf_process: the filter is in a failed state after an earlier error (%s); destroy and re-create it", e->failed_msg);
    }
    const lvk_status st = ekf_process_impl(e, ts, feats, n_feats, imu, n_imu, n_consumed, updated, fetch, fetch_user);
    if (st != LVK_OK) {
        e->failed = st;
        snprintf(e->failed_msg, sizeof e->failed_msg, "%s", e->ctx->err);
        hipStreamSynchronize(e->ctx->stream);            // queued kernels may still read the pinned upload arena the next call would reset
    }
    return st;
}

static lvk_status ekf_process_impl(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated,
                                   lvk_feats_fn fetch, void* fetch_user)
{
    struct Notify {                                     // every return path reports the consumption exactly once
        lvk_ekf* e; int* n; bool fired = false;
        void fire() { if (!fired) { fired = true; if (e->on_consumed) e->on_consumed(e->on_consumed_user, *n); } }
        ~Notify() { fire(); }
    } notify{e, n_consumed};
    e->up_half ^= 1; e->n_sync = 0;
    e->up_off = e->up_flushed = e->up_half ? e->up_cap / 2 : 0; e->up_lim = e->up_off + e->up_cap / 2;
    e->colcache.cols.reset();                           // column lists depend on the clones' ranks, which this call changes
    e->lost_cov_slot.clear(); e->mp_n = 0; e->kf_pending = 0;
    if (!e->b_first_features) {
        if (n_imu > 0 && imu[0].t - ts - e->td <= 0.0) e->b_first_features = true;
        else return LVK_OK;
    }
    int off = 0;
    if (!e->is_gravity_set) {
        if (fetch) { lvk_status fs = fetch(fetch_user, &feats, &n_feats); if (fs != LVK_OK) return fs; fetch = nullptr; }
        int erased = 0;
        // FlexibleInitializer::tryIncInit (FlexibleInitializer.cpp:11-25): the static initialiser first, the dynamic one when that says no
        bool ok = static_try_init(e, ts, feats, n_feats, imu, n_imu, &erased);
        if (!ok) { e->dyn_status = LVK_OK; ok = dynamic_try_init(e, ts, feats, n_feats, imu, n_imu, &erased); if (e->dyn_status != LVK_OK) return e->dyn_status; }
        if (ok) {
            e->is_gravity_set = true;
            e->take_off_stamp = e->s.t; e->last_zupt_time = e->s.t; e->last_update_time = e->s.t;
            e->s_fej_now = e->s;
            off = erased;
            delete e->dyn; e->dyn = nullptr;
        } else return LVK_OK;
    }
    g_tr.start();
    const double td_before = e->td; (void)td_before;
    *n_consumed = off + batch_imu_count(e, ts + e->td, imu + off, n_imu - off);
    notify.fire();                                      // a pipelined driver may start the next frame's front-end now
    const int used = batch_imu(e, ts + e->td, imu + off, n_imu - off);
    if (off + used != *n_consumed) return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "internal: IMU consumption count mismatch");
    TR(TR_IMU);
    lvk_status st = state_augmentation(e);             // ONE launch: the frame's propagation + the augmentation gather
    if (st != LVK_OK) return st;
    TR(TR_PROP);
    if (fetch) { lvk_status fs = fetch(fetch_user, &feats, &n_feats); if (fs != LVK_OK) return fs; }
    TR(TR_FETCH);
    add_observations(e, feats, n_feats);
    TR(TR_ADDOBS);
    if (e->cfg.if_zupt_valid) { bool z = false; st = check_zupt(e, &z); if (st != LVK_OK) return st; e->if_zupt = z; }
    TR(TR_ZUPT);
    st = remove_lost_features(e);
    if (st != LVK_OK) return st;
    st = prune_imu_state_buffer(e);
    if (st != LVK_OK) return st;
    TR(TR_PR_END);
    if (e->cfg.if_fej && !e->if_fej && e->s.t - e->take_off_stamp >= 0) e->if_fej = true;
    e->counters[6] = (long)e->map.size();
    // What is still queued now (the pruning's covariance gather, at most) changes neither the state nor anything the host reads, and
    // it reads the half of the upload arena the NEXT call leaves alone: the call returns without waiting for it.  The call after
    // that reuses this half - behind at least one stream sync of the call in between, which is why a call that had none ends with one.
    if (e->n_sync == 0) { EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++; }
    st = lvk_ekf_exports_attach(e);
    if (st != LVK_OK) return st;
    prof_harvest(e, false);
#ifdef LVK_MSG_HASH_LOG   // debugging aid, compiled out of the product (make CXXFLAGS+=-DLVK_MSG_HASH_LOG); bounded: the first 65536 messages
    {   // LVK_MSG_HASH=<file>: one line per processed message (time stamp, size, FNV-1a of its bytes, IMU samples used + their hash, td
        // before, state after).  Debugging aid: the message is only COPIED here (a few us); hashing and the file are left to exit.
        struct Rec { double ts, td, st[16]; int n, used, N, rows; std::vector<unsigned char> msg, imu; };
        struct Log { std::vector<Rec> recs; const char* path; ~Log() {
            if (!path) return; FILE* f = fopen(path, "a"); if (!f) return;
            auto fnv = [](const std::vector<unsigned char>& b) { unsigned long long h = 1469598103934665603ull; for (unsigned char c : b) { h ^= c; h *= 1099511628211ull; } return h; };
            for (auto& r : recs) { fprintf(f, "%.6f n %d msg %016llx imu %d %016llx td %.12g N %d rows %d state", r.ts, r.n, fnv(r.msg), r.used, fnv(r.imu), r.td, r.N, r.rows);
                                   for (double v : r.st) fprintf(f, " %.17g", v); fprintf(f, "\n"); }
            fclose(f); } };
        static Log lg{{}, getenv("LVK_MSG_HASH")};
        if (lg.path && lg.recs.size() < 65536) {
            Rec r; r.ts = ts; r.td = td_before; r.n = n_feats; r.used = used; r.N = e->N; r.rows = (int)e->counters[2];
            r.msg.assign((const unsigned char*)feats, (const unsigned char*)feats + sizeof(lvk_feature_obs) * (size_t)n_feats);
            r.imu.assign((const unsigned char*)(imu + off), (const unsigned char*)(imu + off) + sizeof(lvk_imu) * (size_t)used);
            memcpy(r.st, e->s.q, 32); memcpy(r.st + 4, e->s.v, 24); memcpy(r.st + 7, e->s.p, 24); memcpy(r.st + 10, e->s.bg, 24); memcpy(r.st + 13, e->s.ba, 24);
            lg.recs.push_back(std::move(r));
        }
    }
#endif
    TR(TR_FINAL);
    g_tr.end_update(TR_NAMES);
    g_tr.n++;
    *updated = 1;
    return LVK_OK;
}

lvk_status lvk_ekf_set_shard(lvk_ekf* e, int rank, int world, lvk_exchange_fn fn, void* user)
{
    if (!e || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_shard: bad argument");
    auto& S = e->shard;
    ekf_quiesce(e);
    if (fn && e->indefinite_policy == LVK_INDEFINITE_LDLT) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update has no pivoted fallback (LVK_INDEFINITE_LDLT is set)");
    if (fn && e->msckf_points_on) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not export MSCKF points (lvk_ekf_set_msckf_points is on)");
    if (fn && e->keyframes_on) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not export keyframes (lvk_ekf_set_keyframe_export is on)");
    EKF_HIP(hipStreamSynchronize(e->ctx->stream));
    if (S.d_send) hipFree(S.d_send); if (S.d_recv) hipFree(S.d_recv);
    S.d_send = S.d_recv = nullptr; S.cap = 0; S.xk_cap = 0;
    S.rank = rank; S.world = world; S.fn = fn; S.user = user;
    if (!fn) return LVK_OK;                             // world 1 without a transport: the unsharded filter
    // Exchange buffers for the largest block a rank may send: every job's gate result + xk_cap rows of R.  Allocated here, once, so
    // that an allocation failure is a set-up error on the rank it happens on and never a rank missing from a collective later.
    S.xk_cap = std::min(e->hrows, 4 * e->nmax);
    const size_t res_cap = (sizeof(FeatResult) * (size_t)2 * e->feat_cap + 255) & ~(size_t)255;
    S.cap = LVK_SHARD_HDR + res_cap + (size_t)S.xk_cap * (size_t)(e->nmax + 1) * sizeof(double);
    if (hipMalloc((void**)&S.d_send, S.cap) != hipSuccess || hipMalloc((void**)&S.d_recv, S.cap * (size_t)world) != hipSuccess) {
        (void)hipGetLastError();
        if (S.d_send) hipFree(S.d_send);
        const size_t want = S.cap;
        S.d_send = S.d_recv = nullptr; S.cap = 0; S.fn = nullptr; S.world = 1; S.rank = 0;
        return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "lvk_ekf_set_shard: exchange buffers (%zu bytes x %d) could not be allocated", want, world + 1);
    }
    *(int*)(e->h_down + e->down_flag) = 0;
    return LVK_OK;
}
void lvk_ekf_shard_stats(const lvk_ekf* e, long* out8)
{
    if (!e || !out8) return;
    ekf_quiesce(e);
    memcpy(out8, e->shard.stats, sizeof e->shard.stats); memcpy(out8 + 4, e->qr_stats, sizeof e->qr_stats);
}

lvk_status lvk_ekf_init_report(const lvk_ekf* e, lvk_init_report* out)
{
    if (!e || !out) return LVK_ERR_ARG;
    ekf_quiesce(e);
    *out = e->init_report;
    return LVK_OK;
}
lvk_status lvk_ekf_profile(lvk_ekf* e, int enable, double* out3)
{   // out3 (optional): [ms inside the update's first launch, its flops (lvk_update_first_launch_flops: H P, plus S's tiles where fused), launches] since the last call, then reset
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    hipStreamSynchronize(e->ctx->stream); prof_harvest(e, true);
    if (out3) { out3[0] = e->prof_ms; out3[1] = e->prof_flops; out3[2] = (double)e->prof_n; }
    e->prof_ms = e->prof_flops = 0; e->prof_n = 0; e->prof_on = enable != 0;
    return LVK_OK;
}
lvk_status lvk_ekf_profile_qr(lvk_ekf* e, double* out4)
{   // [ms inside k_qr_sparse levels, their Householder flops on the structure factored, launches, rows entering the levels] since the last call, then reset
    if (!e || !out4) return LVK_ERR_ARG;
    ekf_quiesce(e);
    hipStreamSynchronize(e->ctx->stream); prof_harvest(e, true);
    out4[0] = e->prof_qr_ms; out4[1] = e->prof_qr_flops; out4[2] = (double)e->prof_qr_n; out4[3] = e->prof_qr_rows;
    e->prof_qr_ms = e->prof_qr_flops = e->prof_qr_rows = 0; e->prof_qr_n = 0;
    return LVK_OK;
}
int lvk_ekf_dim(const lvk_ekf* e) { if (!e) return 0; ekf_quiesce(e); return e->N; }
lvk_status lvk_ekf_get_imu_intrinsics(const lvk_ekf* e, double* o24) { if (!e || !o24) return LVK_ERR_ARG; ekf_quiesce(e); memcpy(o24, e->imx, sizeof e->imx); return LVK_OK; }
lvk_status lvk_ekf_set_imu_intrinsics(lvk_ekf* e, const double* i24) { if (!e || !i24) return LVK_ERR_ARG; ekf_quiesce(e); memcpy(e->imx, i24, sizeof e->imx); update_imu_mx(e); return LVK_OK; }
int lvk_ekf_is_initialized(const lvk_ekf* e) { if (!e) return 0; ekf_quiesce(e); return e->is_gravity_set ? 1 : 0; }
double lvk_ekf_take_off_stamp(const lvk_ekf* e) { if (!e) return 0.0; ekf_quiesce(e); return e->take_off_stamp; }
lvk_status lvk_ekf_get_state(const lvk_ekf* e, double* o)
{
    if (!e || !o) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;           // a half-applied update: state, clone list and covariance layout are out of step
    ekf_state30(e, o);
    return LVK_OK;
}
lvk_status lvk_ekf_get_cov(lvk_ekf* e, double* h_P)
{
    if (!e || !h_P) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    EKF_HIP(hipMemcpy2DAsync(h_P, sizeof(double) * e->N, e->dP[e->cur], sizeof(double) * e->ld, sizeof(double) * e->N, e->N, hipMemcpyDeviceToHost, e->ctx->stream));
    EKF_HIP(hipStreamSynchronize(e->ctx->stream));       // (an update returns with its last covariance gather still queued)
    return LVK_OK;
}
lvk_status lvk_ekf_set_cov(lvk_ekf* e, const double* h_P, int n)
{
    if (!e || !h_P) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_cov: bad argument");
    // "in flight" = queued and not yet waited for, whether or not the worker has finished meanwhile: the answer does not depend on timing
    if (e->async && e->async->unwaited) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_set_cov: an update is in flight (lvk_ekf_wait first)");
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    if (n != e->N) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_set_cov: n = %d, the state has %d dimensions", n, e->N);
    EKF_HIP(hipStreamSynchronize(e->ctx->stream));
    EKF_HIP(hipMemcpy2DAsync(e->dP[e->cur], sizeof(double) * e->ld, h_P, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyHostToDevice, e->ctx->stream));
    EKF_HIP(hipStreamSynchronize(e->ctx->stream));
    e->p00_valid = false;
    return LVK_OK;
}
lvk_status lvk_ekf_set_indefinite_policy(lvk_ekf* e, int policy)
{
    if (!e || (policy != LVK_INDEFINITE_FAIL && policy != LVK_INDEFINITE_LDLT)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_indefinite_policy: bad argument");
    ekf_quiesce(e);
    if (policy == LVK_INDEFINITE_LDLT && e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_indefinite_policy: the sharded update has no pivoted fallback");
    e->indefinite_policy = policy;
    return LVK_OK;
}
lvk_status lvk_ekf_last_update(lvk_ekf* e, int* m, int* n, double* h_H, double* h_r, double* h_P, double* h_state30)
{
    if (!e || !m || !n) return LVK_ERR_ARG;
    ekf_quiesce(e);
    *m = e->last.m; *n = e->last.n;
    if (!h_H && !h_r && !h_P && !h_state30) return LVK_OK;
    if (e->last.m <= 0 || e->last.n != e->N) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_last_update: no update on record for the present state");
    (void)hipGetLastError();
    hipStream_t st = e->ctx->stream;
    const size_t row = sizeof(double) * (size_t)e->N;
    if (h_H) EKF_HIP(hipMemcpy2DAsync(h_H, row, e->last.H, sizeof(double) * e->ld, row, e->last.m, hipMemcpyDeviceToHost, st));
    if (h_r) EKF_HIP(hipMemcpyAsync(h_r, e->last.r, sizeof(double) * (size_t)e->last.m, hipMemcpyDeviceToHost, st));
    if (h_P) EKF_HIP(hipMemcpy2DAsync(h_P, row, e->dP[e->cur], sizeof(double) * e->ld, row, e->N, hipMemcpyDeviceToHost, st));
    EKF_HIP(hipStreamSynchronize(st));
    if (h_state30) { double* o = h_state30; o[0] = e->s.t; memcpy(o + 1, e->s.q, 32); memcpy(o + 5, e->s.v, 24); memcpy(o + 8, e->s.p, 24); memcpy(o + 11, e->s.bg, 24); memcpy(o + 14, e->s.ba, 24);
                     memcpy(o + 17, e->R_b2c, 72); memcpy(o + 26, e->t_c_b, 24); o[29] = e->td; }
    return LVK_OK;
}
long lvk_ekf_indefinite_fallbacks(const lvk_ekf* e) { if (!e) return 0; ekf_quiesce(e); return e->indefinite_fallbacks; }
// the leading n x n block (n <= 16: q v p bg ba[0]) - what getPpose / getPvel read (larvio.cpp:2673-2690) - without moving the
// covariance: the update's last GEMM mirrors that tile into host-mapped memory, and the host waited for that launch when it read dx
lvk_status lvk_ekf_get_cov_imu(lvk_ekf* e, int n, double* h_out)
{
    if (!e || !h_out || n < 1 || n > 16) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    if (e->p00_valid) {
        const double* m = (const double*)(e->h_down + e->down_p00);
        for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) h_out[a * n + b] = m[a * 16 + b];
        return LVK_OK;
    }
    EKF_HIP(hipMemcpy2DAsync(h_out, sizeof(double) * n, e->dP[e->cur], sizeof(double) * e->ld, sizeof(double) * n, n, hipMemcpyDeviceToHost, e->ctx->stream));
    EKF_HIP(hipStreamSynchronize(e->ctx->stream));
    return LVK_OK;
}
int lvk_ekf_get_clones(const lvk_ekf* e, lvk_clone* out, int cap)
{
    if (!e || !out) return 0;
    ekf_quiesce(e);
    int n = std::min((int)e->clones.size(), cap);
    for (int i = 0; i < n; ++i) {
        const Clone& c = e->clones[i]; lvk_clone& o = out[i];
        o.id = c.id; o.time = c.time; o.dt = c.dt; memcpy(o.q, c.q, 32); memcpy(o.p, c.p, 24); memcpy(o.p_fej, c.p_fej, 24);
        memcpy(o.R_b2c, c.R_b2c, 72); memcpy(o.t_c_b, c.t_c_b, 24); memcpy(o.q_cam, c.q_cam, 32); memcpy(o.p_cam, c.p_cam, 24);
    }
    return n;
}
int lvk_ekf_get_features(const lvk_ekf* e, int64_t* ids, double* inv_depth, double* pos_w, int cap)
{
    if (!e) return 0;
    ekf_quiesce(e);
    int n = std::min((int)e->feature_states.size(), cap);
    for (int i = 0; i < n; ++i) {
        const Feature& f = e->map.at(e->feature_states[i]);
        ids[i] = f.id; inv_depth[i] = f.inv_depth; memcpy(pos_w + 3 * i, f.position, 24);
    }
    return n;
}
void lvk_ekf_counters(const lvk_ekf* e, long* out8) { if (e && out8) { ekf_quiesce(e); memcpy(out8, e->counters, sizeof e->counters); } }

// one frame through both halves: the front-end waits for its feature message, `process` (lvk_ekf_process, or lvk_ekf_process_async: what
// the adapter classes do under the reference's blocking drivers, processImage returning the message to the caller) takes it
static lvk_status vio_step(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* updated,
                           lvk_status (*process)(lvk_ekf*, double, const lvk_feature_obs*, int, const lvk_imu*, int, int*, int*))
{
    if (!fe || !ekf || !n_consumed || !has_msg || !updated) return LVK_ERR_ARG;
    *n_consumed = 0; *updated = 0; *has_msg = 0;
    static thread_local std::vector<lvk_feature_obs> msg;
    if (msg.size() < 8192) msg.resize(8192);
    int n_out = 0;
    lvk_status st = lvk_frontend_process(fe, img, ts, h_imu, n_imu, msg.data(), (int)msg.size(), &n_out, has_msg);
    if (st != LVK_OK || !*has_msg) return st;
    return process(ekf, ts, msg.data(), n_out, h_imu, n_imu, n_consumed, updated);
}
lvk_status lvk_vio_process(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* updated)
{
    return vio_step(fe, ekf, img, ts, h_imu, n_imu, n_consumed, has_msg, updated, lvk_ekf_process);
}
lvk_status lvk_vio_process_deferred(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* will_update)
{
    return vio_step(fe, ekf, img, ts, h_imu, n_imu, n_consumed, has_msg, will_update, lvk_ekf_process_async);
}

}  // extern "C"
