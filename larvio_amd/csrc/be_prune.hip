// be_prune.hip — the filter's pruning stage and the zero-velocity update (host code only, no kernel).
#include "be_filter.h"
#include "be_host_math.h"

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
lvk_status lvk_ekf_prune_imu_state_buffer(lvk_ekf* e)
{
    long long rm[2]; int nrm = 0;
    if (!e->if_zupt) {
        if ((int)e->clones.size() < e->cfg.sw_size) return LVK_OK;
        find_redundant(e, rm); nrm = 2;
    } else { rm[0] = e->imu_id - 1; nrm = 1; }
    lvk_status st;
    // pass A: re-anchoring (host + rank-1 covariance op) and collection of the features the update uses, with the triangulations they need.
    // Unsharded, those are consumed on the device by the row kernel (FJ_TRI_PENDING, see lvk_ekf_remove_lost_features, be_update.hip): each names the job slot
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
                    if (!lvk_ekf_check_motion(e, f, f.find(e->imu_id) >= 0)) continue;      // has not moved enough: not used
                    reqs.emplace_back(); lvk_ekf_make_tri_req(e, &f, 1, &reqs.back()); u.tri = (int)reqs.size() - 1;
                    if (tri_on_device) reqs.back().slot = (int)uses.size();
                }
                uses.push_back(u);
            }
        }
    }
    TR(TR_PR_PRE);
    std::vector<RowJob> jobs;
    if (!uses.empty()) {
        st = lvk_ekf_upload_clones(e);
        if (st == LVK_OK && !reqs.empty()) st = tri_on_device ? lvk_ekf_launch_triangulation(e, reqs) : lvk_ekf_run_triangulation(e, reqs, ans);
        if (st != LVK_OK) return st;
    }
    for (const Use& u : uses) {
        if (u.tri >= 0 && !tri_on_device) { apply_tri(u.f, 1, ans[(size_t)u.tri]); if (!ans[(size_t)u.tri].ok) continue; }
        jobs.push_back(msckf_job(u.f, u.inv, tri_on_device ? u.tri : -1));
    }
    TR(TR_PR_TRI);
    if (!jobs.empty()) {
        // measurementUpdate_msckf (:1420-1602), gate decided on the device (lvk_ekf_gated_update): one sync for gate + dx, and for
        // initializePosition_AssignAnchor's pending results (:2420-2440)
        std::vector<double> dx;
        const size_t order[2][2] = {{0, jobs.size()}, {0, 0}};
        st = lvk_ekf_gated_update(e, jobs, order, {TR_PR_ROWS, TR_PR_UPD, TR_PR_DX}, dx, rm, nrm);
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

static lvk_status cov_delete(lvk_ekf* e, int start, int len)
{
    std::vector<int> idx; idx.reserve(e->N);
    for (int i = 0; i < e->N; ++i) if (i < start || i >= start + len) idx.push_back(i);
    return cov_gather(e, idx);
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
    if (st == LVK_OK) st = lvk_ekf_dense_update(e, 9, dx, 0);
    if (st == LVK_OK) st = lvk_ekf_d2h_sync(e, dx.data(), e->d_dx, sizeof(double) * (size_t)N);
    if (st != LVK_OK) return st;
    lvk_ekf_inject(e, dx.data());
    e->last_update_time = e->s.t; e->last_zupt_time = e->s.t;
    e->counters[3]++;
    return LVK_OK;
}
lvk_status lvk_ekf_check_zupt(lvk_ekf* e, bool* out)
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
