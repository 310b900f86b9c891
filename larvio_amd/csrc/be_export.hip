// be_export.hip — what the filter hands out beside its state (host code only, no kernel): the drain lists of lost in-state features,
// used MSCKF points and pruned clones (lvk_ekf_set_lost_feature_cov / _msckf_points / _keyframe_export), each queued on the covariance
// before the columns it needs leave it and attached behind a stream sync, and the covariance getters that build the same jobs.
#include "be_filter.h"
#include "be_host_math.h"

// The results of a launch queued in this call (mark = n_sync when it was queued) are readable behind one more stream sync, made
// here only if none has followed the launch
static lvk_status results_readable(lvk_ekf* e, int mark)
{
    if (e->n_sync == mark) { EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++; }
    return LVK_OK;
}
// the jobs of the clone at rank ra, from the host state: *ja its absolute 6 x 6 block, *jr the covariance of its pose relative to the
// clone at rank rb (rb < 0: there is none, and *jr repeats *ja)
static void pose_rel_pair(const lvk_ekf* e, int ra, int rb, lvk_pose_rel_job* ja, lvk_pose_rel_job* jr)
{
    const Clone& a = e->clones[(size_t)ra];
    memset(ja, 0, sizeof *ja);
    ja->a_theta_col = ja->a_p_col = -1; ja->b_theta_col = LEG + 6 * ra; ja->b_p_col = ja->b_theta_col + 3;
    memcpy(ja->q_b, a.q, 32); memcpy(ja->p_b, a.p, 24);
    *jr = *ja;
    if (rb < 0) return;
    const Clone& b = e->clones[(size_t)rb];
    jr->a_theta_col = LEG + 6 * ra; jr->a_p_col = jr->a_theta_col + 3; jr->b_theta_col = LEG + 6 * rb; jr->b_p_col = jr->b_theta_col + 3;
    memcpy(jr->q_a, a.q, 32); memcpy(jr->p_a, a.p, 24); memcpy(jr->q_b, b.q, 32); memcpy(jr->p_b, b.p, 24);
}
// the landmark-covariance job of in-state feature f (state column LEG + 6 clones + fs_index) from the host state, as inject() reads it;
// false when the injection would skip the feature (anchor not in the window) or the depth is degenerate
static bool landmark_job(const lvk_ekf* e, const Feature& f, int fs_index, lvk_landmark_job* j)
{
    const int ar = clone_rank(e, f.id_anchor);
    if (ar < 0) return false;
    memset(j, 0, sizeof *j);
    j->anchor_col = LEG + 6 * ar; j->feat_col = LEG + 6 * (int)e->clones.size() + fs_index;
    memcpy(j->q_anchor, e->clones[(size_t)ar].q, 32); memcpy(j->R_b2c, e->R_b2c, 72); memcpy(j->t_c_b, e->t_c_b, 24);
    j->obs_anchor[0] = f.obs_anchor[0]; j->obs_anchor[1] = f.obs_anchor[1]; j->inv_depth = f.inv_depth;
    return lvk_landmark_job_ok(j, e->N);
}
// lvk_ekf_set_lost_feature_cov: queue k_landmark_cov for the lost in-state features on the covariance as it is now (their columns
// still in place); the results go to the pinned download buffer and are attached by lost_cov_attach()
lvk_status lvk_ekf_lost_cov_queue(lvk_ekf* e, const std::vector<long long>& ekf_lost)
{
    e->lost_cov_slot.assign(ekf_lost.size(), -1);
    lvk_landmark_job* hj = up_alloc<lvk_landmark_job>(e, ekf_lost.size());
    if (!hj) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    int n = 0;
    for (size_t k = 0; k < ekf_lost.size(); ++k)
        if (n < e->lm_cap && landmark_job(e, e->map.at(ekf_lost[k]), fs_rank(e, ekf_lost[k]), hj + n)) e->lost_cov_slot[k] = n++;
    e->lost_cov_mark = e->n_sync;
    if (n == 0) return LVK_OK;
    const double* P = e->dP[e->cur]; const lvk_landmark_job* d_jobs = dev(e, hj); double* out = (double*)(e->dh_down + e->down_lm);
    return run_or_defer(e, [=]() { return lvk_launch_landmark_cov(e->ctx, P, e->ld, d_jobs, n, out); });
}
static lvk_status lost_cov_attach(lvk_ekf* e)
{
    if (e->lost_cov_slot.empty()) return LVK_OK;
    LVK_TRY(results_readable(e, e->lost_cov_mark));
    const size_t k = e->lost_cov_slot.size(), base = e->lost_slam.size() - k;
    const double* src = (const double*)(e->h_down + e->down_lm);
    for (size_t i = 0; i < k; ++i) if (e->lost_cov_slot[i] >= 0) memcpy(e->lost_slam[base + i].cov, src + 9 * (size_t)e->lost_cov_slot[i], 72);
    e->lost_cov_slot.clear();
    return LVK_OK;
}
// lvk_ekf_set_keyframe_export: one record per clone in rm (those in the window, ascending rank), and k_pose_rel_cov queued for them on the
// covariance as it is now (the pruning update applied, their columns still in place); b = the nearest newer clone not in rm
lvk_status lvk_ekf_keyframes_queue(lvk_ekf* e, const long long* rm, int nrm)
{
    int ra[2], n = 0;
    for (int k = 0; k < nrm && k < 2; ++k) { const int r = clone_rank(e, rm[k]); if (r >= 0) ra[n++] = r; }
    if (n == 2 && ra[0] > ra[1]) std::swap(ra[0], ra[1]);
    if (n == 0) return LVK_OK;
    lvk_pose_rel_job* hj = up_alloc<lvk_pose_rel_job>(e, (size_t)2 * n);
    if (!hj) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    for (int i = 0; i < n; ++i) {
        const Clone& a = e->clones[(size_t)ra[i]];
        int rb = ra[i] + 1;
        while (rb < (int)e->clones.size() && (rb == ra[0] || rb == ra[n - 1])) ++rb;
        lvk_keyframe kf; memset(&kf, 0, sizeof kf);
        kf.id = a.id; kf.time = a.time; memcpy(kf.q, a.q, 32); memcpy(kf.p, a.p, 24);
        for (int t = 0; t < 36; ++t) kf.cov_abs[t] = kf.cov_rel[t] = NAN;
        lvk_pose_rel_job* ja = hj + 2 * i; lvk_pose_rel_job* jr = ja + 1;
        pose_rel_pair(e, ra[i], rb < (int)e->clones.size() ? rb : -1, ja, jr);      // no newer clone survives (the pruning never removes the newest): the absolute block twice, NaN kept below
        kf.to_id = -1; kf.to_time = NAN;
        for (int t = 0; t < 4; ++t) kf.rel_q[t] = NAN;
        for (int t = 0; t < 3; ++t) kf.rel_p[t] = NAN;
        if (rb < (int)e->clones.size()) {
            const Clone& b = e->clones[(size_t)rb];
            kf.to_id = b.id; kf.to_time = b.time;
            const double qa_inv[4] = {-a.q[0], -a.q[1], -a.q[2], a.q[3]}, d[3] = {b.p[0] - a.p[0], b.p[1] - a.p[1], b.p[2] - a.p[2]};
            double Ra[9];
            quat_mul(qa_inv, b.q, kf.rel_q); quat_to_rot(a.q, Ra); m3t_v(Ra, d, kf.rel_p);
        }
        if (!lvk_pose_rel_job_ok(ja, e->N) || !lvk_pose_rel_job_ok(jr, e->N)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "internal: a keyframe job leaves the %d x %d covariance", e->N, e->N);
        drain_append(e->keyframes, kf);
    }
    e->kf_pending = n; e->kf_mark = e->n_sync;
    const double* P = e->dP[e->cur]; const lvk_pose_rel_job* d_jobs = dev(e, hj); double* out = (double*)(e->dh_down + e->down_kf);
    return run_or_defer(e, [=]() { return lvk_launch_pose_rel_cov(e->ctx, P, e->ld, d_jobs, 2 * n, out); });
}
static lvk_status keyframes_attach(lvk_ekf* e)
{
    if (e->kf_pending <= 0) return LVK_OK;
    LVK_TRY(results_readable(e, e->kf_mark));
    const size_t k = (size_t)e->kf_pending, base = e->keyframes.size() - k;
    const double* src = (const double*)(e->h_down + e->down_kf);
    for (size_t i = 0; i < k; ++i) {
        lvk_keyframe& kf = e->keyframes[base + i];
        memcpy(kf.cov_abs, src + 72 * i, 288);
        if (kf.to_id >= 0) memcpy(kf.cov_rel, src + 72 * i + 36, 288);
    }
    e->kf_pending = 0;
    return LVK_OK;
}
// lvk_ekf_set_msckf_points: queue k_msckf_point_cov for the MSCKF jobs [lo, hi) of the batch launch_feature_rows has just staged, on the
// covariance as it is now (the one the update starts from), on the observations that launch staged (obs); the results go to the pinned
// download buffer, lvk_ekf_msckf_point_record() reads them behind the wait the update makes for its gate results
lvk_status lvk_ekf_msckf_points_queue(lvk_ekf* e, const std::vector<RowJob>& jobs, size_t lo, size_t hi, const RowObs& obs)
{
    e->mp_n = 0;
    if (!e->msckf_points_on || hi <= lo) return LVK_OK;
    if (!obs.rank || !obs.z || !obs.zv) return lvk_set_error(e->ctx, LVK_ERR_ARG, "internal: MSCKF points queued without a staged batch");
    if (hi - lo > (size_t)e->mp_cap) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "internal: %zu MSCKF jobs exceed the %d result slots of the point export", hi - lo, e->mp_cap);
    const int n = (int)(hi - lo);
    PointJob* hj = up_alloc<PointJob>(e, (size_t)n);
    if (!hj) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    for (int k = 0; k < n; ++k) {
        const RowJob& j = jobs[lo + (size_t)k];
        hj[k].n_obs = j.dev.n_obs; hj[k].obs_off = j.dev.obs_off; hj[k].tri_slot1 = j.tri >= 0 ? (int)(lo + (size_t)k) + 1 : 0; hj[k].pad = 0;
        memcpy(hj[k].p_w, j.dev.p_w, 24);
    }
    e->mp_lo = lo; e->mp_n = n;
    const FilterFlags fl = filter_flags(LEG, e->if_fej, e->cfg.estimate_td, e->sigma2);
    const double* P = e->dP[e->cur]; const PointJob* d_jobs = dev(e, hj); const CloneDev* d_cl = e->dv_clones;
    const int* d_r = obs.rank; const double* d_z = obs.z; const double* d_v = obs.zv; const TriResult* d_tri = e->d_tridev;
    double* out = (double*)(e->dh_down + e->down_mp); int* ok = (int*)(e->dh_down + e->down_mpok);
    return run_or_defer(e, [=]() { return lvk_launch_msckf_point_cov(e->ctx, P, e->ld, d_jobs, n, d_cl, d_r, d_z, d_v, fl, d_tri, out, ok); });
}
// job k of the batch was an MSCKF feature that triangulated and passed its gate, and is about to be erased: keep it (after the stream
// wait that covers the launch above)
void lvk_ekf_msckf_point_record(lvk_ekf* e, const RowJob& j, size_t k)
{
    if (e->mp_n <= 0 || k < e->mp_lo || k >= e->mp_lo + (size_t)e->mp_n) return;
    const size_t slot = k - e->mp_lo;
    if (!((const int*)(e->h_down + e->down_mpok))[slot]) return;
    lvk_ekf::MsckfPoint mp; mp.id = j.f->id; memcpy(mp.p, j.f->position, 24); mp.n_obs = (int)j.sids.size();
    memcpy(mp.cov, (const double*)(e->h_down + e->down_mp) + 9 * slot, 72);
    drain_append(e->msckf_points, mp);
}
// drain on read: the oldest min(size, cap) records go to copy(i, record) and leave the list
template <typename T, typename Copy> static int drain_take(std::vector<T>& list, int cap, Copy copy)
{
    const int n = std::min((int)list.size(), cap);
    for (int i = 0; i < n; ++i) copy(i, list[(size_t)i]);
    list.erase(list.begin(), list.begin() + n);
    return n;
}
// end of an update: what was queued in this call joins its records
lvk_status lvk_ekf_exports_attach(lvk_ekf* e) { LVK_TRY(lost_cov_attach(e)); return keyframes_attach(e); }

extern "C" {

int lvk_ekf_take_lost_features_cov(lvk_ekf* e, int64_t* ids, double* pos_w, double* cov9, int cap)
{
    if (!e || cap <= 0) return 0;
    ekf_quiesce(e);
    return drain_take(e->lost_slam, cap, [=](int i, const lvk_ekf::LostPoint& lp) {
        if (ids) ids[i] = lp.id;
        if (pos_w) memcpy(pos_w + 3 * i, lp.p, 24);
        if (cov9) memcpy(cov9 + 9 * i, lp.cov, 72);
    });
}
int lvk_ekf_take_lost_features(lvk_ekf* e, int64_t* ids, double* pos_w, int cap)
{
    return ids && pos_w ? lvk_ekf_take_lost_features_cov(e, ids, pos_w, nullptr, cap) : 0;
}
lvk_status lvk_ekf_set_lost_feature_cov(lvk_ekf* e, int on)
{
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    e->lost_cov_on = on != 0;
    return LVK_OK;
}
lvk_status lvk_ekf_set_msckf_points(lvk_ekf* e, int on)
{
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (on && e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_msckf_points: the sharded update does not export MSCKF points");
    e->msckf_points_on = on != 0;
    return LVK_OK;
}
int lvk_ekf_take_msckf_points(lvk_ekf* e, int64_t* ids, double* pos_w, double* cov9, int* n_obs, int cap)
{
    if (!e || cap <= 0) return 0;
    ekf_quiesce(e);
    return drain_take(e->msckf_points, cap, [=](int i, const lvk_ekf::MsckfPoint& mp) {
        if (ids) ids[i] = mp.id;
        if (pos_w) memcpy(pos_w + 3 * i, mp.p, 24);
        if (cov9) memcpy(cov9 + 9 * i, mp.cov, 72);
        if (n_obs) n_obs[i] = mp.n_obs;
    });
}
lvk_status lvk_ekf_set_keyframe_export(lvk_ekf* e, int on)
{
    if (!e) return LVK_ERR_ARG;
    ekf_quiesce(e);
    if (on && e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_keyframe_export: the sharded update does not export keyframes");
    e->keyframes_on = on != 0;
    return LVK_OK;
}
int lvk_ekf_take_keyframes(lvk_ekf* e, lvk_keyframe* out, int cap)
{
    if (!e || !out || cap <= 0) return 0;
    ekf_quiesce(e);
    return drain_take(e->keyframes, cap, [=](int i, const lvk_keyframe& kf) { out[i] = kf; });
}
lvk_status lvk_ekf_get_window_cov(lvk_ekf* e, int64_t* ids, double* cov_abs36, double* cov_rel36, int cap, int* n_out)
{
    if (!e || !n_out || cap < 0) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_get_window_cov: bad argument");
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    const int n = std::min((int)e->clones.size(), cap);
    *n_out = n;
    if (ids) for (int i = 0; i < n; ++i) ids[i] = e->clones[(size_t)i].id;
    if (n == 0 || (!cov_abs36 && !cov_rel36)) return LVK_OK;
    // jobs 0..n-1: the absolute blocks; n..2n-2: clone i relative to clone i + 1 (against the whole window, also when cap cuts the list)
    const int n_rel = std::min(n, (int)e->clones.size() - 1);
    std::vector<lvk_pose_rel_job> jobs((size_t)(n + n_rel));
    lvk_pose_rel_job none;                              // the newest clone has no relative job
    for (int i = 0; i < n; ++i) pose_rel_pair(e, i, i < n_rel ? i + 1 : -1, &jobs[(size_t)i], i < n_rel ? &jobs[(size_t)(n + i)] : &none);
    std::vector<double> out(36 * jobs.size());
    lvk_status st = lvk_ekf_pose_rel_cov(e->ctx, e->dP[e->cur], e->ld, e->N, jobs.data(), (int)jobs.size(), out.data());
    if (st != LVK_OK) return st;
    if (cov_abs36) memcpy(cov_abs36, out.data(), sizeof(double) * 36 * (size_t)n);
    if (cov_rel36) {
        for (int i = 36 * n_rel; i < 36 * n; ++i) cov_rel36[i] = NAN;
        memcpy(cov_rel36, out.data() + 36 * (size_t)n, sizeof(double) * 36 * (size_t)n_rel);
    }
    return LVK_OK;
}
lvk_status lvk_ekf_get_feature_cov(lvk_ekf* e, int64_t* ids, int64_t* anchor_ids, double* pos_w, double* cov9, int cap, int* n_out)
{
    if (!e || !n_out || cap < 0) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_get_feature_cov: bad argument");
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    const int n = std::min((int)e->feature_states.size(), cap);
    std::vector<lvk_landmark_job> jobs; std::vector<int> slot((size_t)n, -1);
    jobs.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        const Feature& f = e->map.at(e->feature_states[i]);
        if (ids) ids[i] = f.id;
        if (anchor_ids) anchor_ids[i] = f.id_anchor;
        if (pos_w) memcpy(pos_w + 3 * i, f.position, 24);
        lvk_landmark_job j;
        if (cov9 && landmark_job(e, f, i, &j)) { slot[(size_t)i] = (int)jobs.size(); jobs.push_back(j); }
    }
    *n_out = n;
    if (!cov9) return LVK_OK;
    for (int i = 0; i < 9 * n; ++i) cov9[i] = NAN;
    if (jobs.empty()) return LVK_OK;
    std::vector<double> out(9 * jobs.size());
    lvk_status st = lvk_ekf_landmark_cov(e->ctx, e->dP[e->cur], e->ld, e->N, jobs.data(), (int)jobs.size(), out.data());
    if (st != LVK_OK) return st;
    for (int i = 0; i < n; ++i) if (slot[(size_t)i] >= 0) memcpy(cov9 + 9 * i, &out[9 * (size_t)slot[(size_t)i]], 72);
    return LVK_OK;
}
lvk_status lvk_ekf_get_feature_rel(lvk_ekf* e, int64_t to_clone_id, int64_t* ids, int64_t* anchor_ids, double* pos_c, double* cov9, int cap, int* n_out)
{
    if (!e || !n_out || cap < 0) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_get_feature_rel: bad argument");
    ekf_quiesce(e);
    if (e->failed != LVK_OK) return e->failed;
    // the target: the IMU state (columns 0.. and 6..) or a clone of the window
    int bt = 0, bp = 6; const double* q_b = e->s.q; const double* p_b = e->s.p;
    if (to_clone_id != -1) {
        const int br = clone_rank(e, to_clone_id);
        if (br < 0) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_get_feature_rel: clone %lld is not in the window", (long long)to_clone_id);
        bt = LEG + 6 * br; bp = bt + 3; q_b = e->clones[(size_t)br].q; p_b = e->clones[(size_t)br].p;
    }
    const int n = std::min((int)e->feature_states.size(), cap);
    std::vector<lvk_landmark_rel_job> jobs; std::vector<int> slot((size_t)n, -1);
    jobs.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        const Feature& f = e->map.at(e->feature_states[i]);
        if (ids) ids[i] = f.id;
        if (anchor_ids) anchor_ids[i] = f.id_anchor;
        lvk_landmark_job lj;
        if ((!pos_c && !cov9) || !landmark_job(e, f, i, &lj)) continue;
        lvk_landmark_rel_job j; memset(&j, 0, sizeof j);
        static_assert(offsetof(lvk_landmark_rel_job, b_theta_col) == sizeof(lvk_landmark_job) && offsetof(lvk_landmark_rel_job, inv_depth) == offsetof(lvk_landmark_job, inv_depth),
                      "lvk_landmark_rel_job starts with the fields of lvk_landmark_job");
        memcpy(&j, &lj, sizeof lj);
        j.b_theta_col = bt; j.b_p_col = bp; memcpy(j.q_b, q_b, 32); memcpy(j.p_b, p_b, 24);
        memcpy(j.p_anchor, e->clones[(size_t)clone_rank(e, f.id_anchor)].p, 24);
        if (!lvk_landmark_rel_job_ok(&j, e->N)) continue;
        slot[(size_t)i] = (int)jobs.size(); jobs.push_back(j);
    }
    *n_out = n;
    if (!pos_c && !cov9) return LVK_OK;
    if (pos_c) for (int i = 0; i < 3 * n; ++i) pos_c[i] = NAN;
    if (cov9) for (int i = 0; i < 9 * n; ++i) cov9[i] = NAN;
    if (jobs.empty()) return LVK_OK;
    std::vector<double> out(12 * jobs.size());
    lvk_status st = lvk_ekf_landmark_rel_cov(e->ctx, e->dP[e->cur], e->ld, e->N, jobs.data(), (int)jobs.size(), out.data());
    if (st != LVK_OK) return st;
    for (int i = 0; i < n; ++i) {
        if (slot[(size_t)i] < 0) continue;
        const double* o = &out[12 * (size_t)slot[(size_t)i]];
        if (pos_c) memcpy(pos_c + 3 * i, o, 24);
        if (cov9) memcpy(cov9 + 9 * i, o + 3, 72);
    }
    return LVK_OK;
}

}  // extern "C"
