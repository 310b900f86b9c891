// be_update.hip — the filter's feature update (host code only, no kernel): the feature-row jobs of a batch and their row layout, the
// host side of the sharded update, the dense update and its health check, the gated update in one sync, and the lost-feature
// update (removeLostFeatures) whose admission branch lays out the same rows by hand.
#include "be_filter.h"
#include "be_host_math.h"

// ------------------------------------------------------------------------- deferred launches, the health check behind every update
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
lvk_status lvk_ekf_d2h_sync(lvk_ekf* e, void* dst, const void* src, size_t bytes)
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

// ------------------------------------------------------------------------- feature-row jobs (be_filter.h has the MSCKF job and the row counts)
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
    double* Ho = e->d_H; double* ro = e->d_r; const int ldh = e->ld, ncols_out = e->N;       // direct output of the jobs that carry a destination row (FeatJob::dst_row1, patched by lvk_ekf_gated_update)
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
static lvk_status shard_peer_check(lvk_ekf* e)
{   // call after a stream sync: did k_shard_unpack find a peer's block poisoned (that rank failed before the exchange)?
    if (!e->shard.fn) return LVK_OK;
    int* f = (int*)(e->h_down + e->down_flag);
    if (*f == 0) return LVK_OK;
    const int mask = *f; *f = 0;
    return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "sharded update: the block of a peer rank (mask 0x%x) arrived invalid - that rank failed before the exchange", mask);
}
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
lvk_status lvk_ekf_dense_update(lvk_ekf* e, int m, std::vector<double>& dx, int extra, const std::vector<RowGroup>* groups)
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

// The gated update in one sync.  No feature enters the state, so nothing on the host depends on a gate result before the update is
// launched: every candidate row gets its slot, the device zeroes the rows of rejected jobs (a zero row with a zero residual leaves
// the update unchanged), and gate results (jobs[].res), pending triangulation answers and dx come back in ONE sync.
// order: the job index ranges in stacking order - MSCKF jobs first, then the tracked in-state features' two rows each:
// H_o = [H_msckf ; H_ekf], the reference's order (larvio.cpp:1612-1626).  Unsharded, the row kernel (held back by begin_defer until
// the slots are known) writes its rows straight into H_o (FeatJob::dst_row1); sharded, this rank builds the rows of its slice of
// the jobs and shard_stage1 exchanges the compressed blocks.  tr: the trace slots that close after the row launch is staged (-1:
// none), after the update is launched and after the sync.  retire: state ids whose observations leave every feature once the jobs
// are staged (pruning: the clones about to go) - host work done here, while the device still runs what was queued ahead.
lvk_status lvk_ekf_gated_update(lvk_ekf* e, std::vector<RowJob>& jobs, const size_t (&order)[2][2], const int (&tr)[3], std::vector<double>& dx,
                                const long long* retire, int n_retire, size_t mp_lo, size_t mp_hi)
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
    if (st == LVK_OK) st = lvk_ekf_dense_update(e, m, dx, 0, &grp);
    TR(tr[1]);
    if (st == LVK_OK) st = fetch_feature_results(e, jobs, dx.data(), (size_t)N);
    if (st != LVK_OK) return st;
    TR(tr[2]);
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
            cd.motion = lvk_ekf_check_motion(e, f, cd.tracked);
            if (!cd.motion && !both) { if (cd.tracked) continue; cd.invalid = true; }     // a lost feature that has not moved is invalid (:1911-1916); a tracked one waits for more views
        }
        if (cd.motion) {
            if (both && !f.ekf_feature) { reqs.emplace_back(); lvk_ekf_make_tri_req(e, &f, 2, &reqs.back()); reqs.back().use_pos = false; cd.idx_inv = (int)reqs.size() - 1; }
            if (!f.is_initialized || (both && !f.ekf_feature)) { reqs.emplace_back(); lvk_ekf_make_tri_req(e, &f, 0, &reqs.back()); cd.idx_pos = (int)reqs.size() - 1; }
        }
        cands.push_back(cd);
    }
}
lvk_status lvk_ekf_remove_lost_features(lvk_ekf* e)
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
    st = lvk_ekf_upload_clones(e);
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
        st = lvk_ekf_launch_triangulation(e, reqs);
        if (st != LVK_OK) return st;
        TR(TR_RLF_TRI);
    } else {
        std::vector<TriAns> ans;
        TR(TR_RLF_PRE);
        st = lvk_ekf_run_triangulation(e, reqs, ans);
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
        st = lvk_ekf_gated_update(e, jobs, order, {-1, TR_RLF_UPD, TR_RLF_DX}, dx, nullptr, 0, j_msckf, jobs.size());
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
        st = lvk_ekf_dense_update(e, m, dx, n_acc, &grp);
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
        st = lvk_ekf_d2h_sync(e, dx.data(), e->d_dx, sizeof(double) * (size_t)(N + n_acc));
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
            lvk_ekf_inject(e, dx.data());
            e->N = N + n_acc;
            e->last_update_time = e->s.t;
            e->counters[0]++;
        }
    }
    for (Feature* f : msckf) e->map.erase(f->id);
    TR(TR_RLF_INJ);
    return LVK_OK;
}
