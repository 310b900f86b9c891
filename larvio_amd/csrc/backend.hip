// backend.hip — the frame-level back-end object of liblvk_hip.so: lvk_ekf_process replaces
// LarVio::processFeatures (src/larvio.cpp:363-461).
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
//
// This file is the filter's C ABI and the sequence of one message (ekf_process_impl); each stage it calls has a file of its own:
// be_initialize.hip (static and moving start), be_propagate.hip (IMU batch, augmentation, new observations, state injection),
// be_update.hip (feature-row jobs, sharded / dense / gated update, the lost-feature update), be_triangulate.hip (the clone tables and
// triangulation batches of both feature updates), be_prune.hip (pruning and ZUPT).  The filter object, the records the stages pass
// and the helpers they share are in be_filter.h, the stages' prototypes in be_host.h; the exports beside the state (drain lists,
// covariance getters) are in be_export.hip, the sequential and the pipelined driver in be_pipe.hip.
#include "be_filter.h"
#include "be_host_math.h"
#include "be_init.h"        // lvk_init::DynInit is deleted here (lvk_ekf_destroy, and once the filter has its state)
#include <new>
#include <float.h>
#include <sched.h>
#include <pthread.h>

// ------------------------------------------------------------------------- host-side phase tracer (LVK_EKF_TRACE=1): the one instance
EkfTrace g_tr;
static const char* const TR_NAMES[TR_N] = {"batch_imu", "propagate+augment(launch)", "message fetch (front-end wait)", "add_obs", "zupt_check", "lost:prepare", "lost:triangulate+sync",
    "lost:triage+jobs", "lost:rows+sync", "lost:stack+update(launch)", "lost:dx sync", "lost:inject", "prune:prepare(+reanchor)", "prune:triangulate+sync",
    "prune:rows+sync", "prune:update(launch)", "prune:dx sync", "prune:inject+delete", "final sync"};
static const char* const TRS_NAMES[8] = {"update w/o new feature: jobs staged (launch_feature_rows)", "  row slots + groups (push_rows)", "  uploads flushed, row kernel launched (end_defer)",
    "  compression planned / launched", "  update core launched (4 kernels)", "batch_imu: (unused)", "(unused)", "(unused)"};

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
// feats == nullptr && fetch != nullptr: the message is collected through fetch() as late as the algorithm allows - after the IMU
// samples have been integrated and the propagation / augmentation kernels are queued - so that a pipelined driver overlaps that
// work with the front-end that is still producing the message (the static initializer needs the message first and asks at once).
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
        bool ok = lvk_ekf_static_try_init(e, ts, feats, n_feats, imu, n_imu, &erased);
        if (!ok) { e->dyn_status = LVK_OK; ok = lvk_ekf_dynamic_try_init(e, ts, feats, n_feats, imu, n_imu, &erased); if (e->dyn_status != LVK_OK) return e->dyn_status; }
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
    const int used = lvk_ekf_batch_imu(e, ts + e->td, imu + off, n_imu - off);
    if (off + used != *n_consumed) return lvk_set_error(e->ctx, LVK_ERR_DEVICE, "internal: IMU consumption count mismatch");
    TR(TR_IMU);
    lvk_status st = lvk_ekf_state_augmentation(e);             // ONE launch: the frame's propagation + the augmentation gather
    if (st != LVK_OK) return st;
    TR(TR_PROP);
    if (fetch) { lvk_status fs = fetch(fetch_user, &feats, &n_feats); if (fs != LVK_OK) return fs; }
    TR(TR_FETCH);
    lvk_ekf_add_observations(e, feats, n_feats);
    TR(TR_ADDOBS);
    if (e->cfg.if_zupt_valid) { bool z = false; st = lvk_ekf_check_zupt(e, &z); if (st != LVK_OK) return st; e->if_zupt = z; }
    TR(TR_ZUPT);
    if (!e->fix_queue.empty()) { st = lvk_ekf_apply_fixes(e); if (st != LVK_OK) return st; }      // external fixes (lvk_ekf_add_fix): the message's clone exists, none is pruned yet
    if (!e->lm_queue.empty()) { st = lvk_ekf_apply_landmarks(e); if (st != LVK_OK) return st; }   // observations of known landmarks (lvk_ekf_add_landmark_obs), behind the fixes
    st = lvk_ekf_remove_lost_features(e);
    if (st != LVK_OK) return st;
    st = lvk_ekf_prune_imu_state_buffer(e);
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

// ------------------------------------------------------------------------- C ABI
extern "C" {

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
    // so lvk_ekf_gated_update refuses a layout of more rows.  (A pruning update cannot get there: one row per job, at most 2 * feat_cap jobs
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

lvk_status lvk_ekf_set_shard(lvk_ekf* e, int rank, int world, lvk_exchange_fn fn, void* user)
{
    if (!e || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_shard: bad argument");
    auto& S = e->shard;
    ekf_quiesce(e);
    if (fn && e->indefinite_policy == LVK_INDEFINITE_LDLT) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update has no pivoted fallback (LVK_INDEFINITE_LDLT is set)");
    if (fn && e->msckf_points_on) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not export MSCKF points (lvk_ekf_set_msckf_points is on)");
    if (fn && e->keyframes_on) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not export keyframes (lvk_ekf_set_keyframe_export is on)");
    if (fn && !e->fix_queue.empty()) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not apply fixes (%zu wait, lvk_ekf_add_fix)", e->fix_queue.size());
    if (fn && !e->lm_queue.empty()) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_set_shard: the sharded update does not apply landmark observations (%zu batches wait, lvk_ekf_add_landmark_obs)", e->lm_queue.size());
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

}  // extern "C"
