// be_triangulate.hip — what both feature updates (be_update.hip, be_prune.hip) ask of the clone window before they build rows (host
// code only, no kernel): the clone tables on the device, the triangulation requests of a batch and their launch, the motion check.
#include "be_filter.h"
#include "be_host_math.h"

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
lvk_status lvk_ekf_upload_clones(lvk_ekf* e)
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
void lvk_ekf_make_tri_req(lvk_ekf* e, Feature* f, int mode, TriReq* rq)
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
// queues the batch; results go to the device-mapped host mirror (d_triout) and to d_tridev, at the request's slot when it names one
lvk_status lvk_ekf_launch_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs)
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
lvk_status lvk_ekf_run_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs, std::vector<TriAns>& ans)
{
    ans.assign(reqs.size(), TriAns());
    if (reqs.empty()) return LVK_OK;
    lvk_status st = lvk_ekf_launch_triangulation(e, reqs);
    if (st != LVK_OK) return st;
    EKF_HIP(hipStreamSynchronize(e->ctx->stream)); e->n_sync++;
    for (size_t i = 0; i < reqs.size(); ++i) ans[i] = tri_answer(e, reqs[i], reqs[i].slot >= 0 ? (size_t)reqs[i].slot : i);
    return LVK_OK;
}
bool lvk_ekf_check_motion(const lvk_ekf* e, const Feature& f, bool if_tracked)
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
