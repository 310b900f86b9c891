// be_initialize.hip — the filter's two initialisers (host code; the RANSAC stage of the moving start runs fe_track.hip's kernel).
#include "be_filter.h"
#include "be_host_math.h"
#include "be_init.h"

// ------------------------------------------------------------------------- static initializer (StaticInitializer.cpp:12-163)
bool lvk_ekf_static_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased)
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
bool lvk_ekf_dynamic_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased)
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
