// be_propagate.hip — the filter's propagation stage (host code only, no kernel): the IMU samples of a frame integrated on the host
// and composed into one (Phi, Q) pair, the clone augmentation that carries it to the device in one launch, the message's
// observations entering the feature map, and the injection of an update's dx into the host state.
#include "be_filter.h"
#include "be_host_math.h"

#define GRAV 9.81

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

int lvk_ekf_batch_imu(lvk_ekf* e, double time_bound, const lvk_imu* imu, int n_imu)
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

lvk_status lvk_ekf_state_augmentation(lvk_ekf* e)
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

void lvk_ekf_add_observations(lvk_ekf* e, const lvk_feature_obs* f, int n)
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

static void clone_refresh_cam(const lvk_ekf* e, Clone* c)
{   // larvio.cpp:1529-1541
    double R_c2b[9], R_b2w[9], R_c2w[9], t[3];
    m3_t(e->R_b2c, R_c2b); quat_to_rot(c->q, R_b2w); m3_mul(R_b2w, R_c2b, R_c2w);
    rot_to_quat(R_c2w, c->q_cam);
    m3_v(R_b2w, e->t_c_b, t);
    for (int i = 0; i < 3; ++i) c->p_cam[i] = c->p[i] + t[i];
}
// ------------------------------------------------------------------------- state injection (larvio.cpp:1476-1575 etc.)
void lvk_ekf_inject(lvk_ekf* e, const double* dx)
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
