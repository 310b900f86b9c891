// frontend.hip — the front-end's state machine and its ABI: what a frame queues, on which stream, behind which event; the kernels of
// the frame path and their launches are in fe_frame.hip, the object itself in fe_frontend.h.
// lvk_frontend_process replaces ImageProcessor::processImage (/root/reference/src/image_processor.cpp:130-219).
//
// Device-resident design (MI355X): the track table (ids, points, first-seen descriptors, lifetimes),
// the three pyramids and the three ORB mosaics (previous, current, spare) stay in HBM across frames; every data-dependent count
// (tracks alive, new corners, survivors per stage) lives in a device struct, kernels are launched
// over the full capacity and dead wavefronts exit at once.  The host therefore never waits on the
// GPU inside a steady-state frame except to fetch the feature message on publish frames.
// Stages keep points IN PLACE with a stage code instead of compacting six vectors four times
// (image_processor.h:215-230); the one order-preserving compaction happens inside the RANSAC
// workgroup, which needs the compacted order anyway (OpenCV's RNG draws indices into it).
#include "lvk_internal.h"
#include "fe_pixfmt_dev.h"
#include "fe_track_dev.h"
#include "fe_frontend.h"
#include <math.h>
#include <float.h>
#include <new>

FeTrace g_ft;
static const char* const FT_NAMES[FT_N] = {"staging slot free (end-of-frame event of f-2)", "image -> pinned staging slot (memcpy)", "H2D copy command", "image stage: event queries + 5 launches",
    "OUTSIDE the front-end: between lvk_frontend_begin and lvk_frontend_process of the frame (the pipelined caller's own submit logic and its wait for the erase count)",
    "frame start: query / wait for the pyramid event (ev_pyr or ev_orb) + the side stream's wait for the previous frame's end event", "frame checks + predict_homography (host math)",
    "track chains: 2 launches + events", "commits: 2 launches + events", "message: slot + launch + event", "detection: 4 launches", "end-of-frame events + rotation"};

static void prof_collect(lvk_frontend* fe)
{
    if (fe->pending.empty()) return;
    hipStreamSynchronize(fe->ctx->stream);
    for (int i = 0; i < 2; ++i) if (fe->side[i]) hipStreamSynchronize(fe->side[i]->stream);
    for (auto& p : fe->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { fe->prof_ms[p.stage] += ms; fe->prof_n[p.stage] += 1; }
        fe->ev_free.push_back(p.a); fe->ev_free.push_back(p.b);
    }
    fe->pending.clear();
}

static void set_free(TrackSet& s)
{
    if (s.id) hipFree(s.id); if (s.pts) hipFree(s.pts); if (s.ppts) hipFree(s.ppts); if (s.init) hipFree(s.init);
    if (s.life) hipFree(s.life); if (s.desc) hipFree(s.desc);
    memset(&s, 0, sizeof s);
}

lvk_context* lvk_frontend_context(lvk_frontend* fe) { return fe ? fe->ctx : nullptr; }

extern "C" {

// ---- gyro prediction: host math, float32 as the reference (image_processor.cpp:222-293) -----------
lvk_status lvk_predict_homography(const lvk_imu* imu, int n_imu, double t_prev, double t_curr, const double R_cam_imu[9],
                                  const double intr[4], float H[9])
{
    if ((n_imu > 0 && !imu) || !R_cam_imu || !intr || !H) return LVK_ERR_ARG;
    int b = 0;
    while (b < n_imu && imu[b].t - t_prev < -0.0049) ++b;
    int e = b;
    while (e < n_imu && imu[e].t - t_curr < 0.0049) ++e;
    float mw[3] = {0.f, 0.f, 0.f};
    for (int i = b; i < e; ++i) { mw[0] += (float)imu[i].gyro[0]; mw[1] += (float)imu[i].gyro[1]; mw[2] += (float)imu[i].gyro[2]; }
    if (e - b > 0) { float s = 1.0f / (e - b); mw[0] *= s; mw[1] *= s; mw[2] *= s; }
    float cw[3];
    for (int i = 0; i < 3; ++i) {
        double s = 0.;
        for (int k = 0; k < 3; ++k) s += R_cam_imu[k * 3 + i] * (double)mw[k];
        cw[i] = (float)s;
    }
    const double dtime = t_curr - t_prev;
    const float rv[3] = {(float)(cw[0] * dtime), (float)(cw[1] * dtime), (float)(cw[2] * dtime)};
    double rx = rv[0], ry = rv[1], rz = rv[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    double R[9];
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1. : 0.;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1. - c, it = theta ? 1. / theta : 0.;
        rx *= it; ry *= it; rz *= it;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
        for (int i = 0; i < 9; ++i) R[i] = c * ((i % 4 == 0) ? 1. : 0.) + c1 * rrt[i] + s * r_x[i];
    }
    float Rt[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = (float)R[j * 3 + i];
    const float K[9] = {(float)intr[0], 0.f, (float)intr[2], 0.f, (float)intr[1], (float)intr[3], 0.f, 0.f, 1.f};
    float Ki[9];
    {
        const float* a = K;
        float d = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[6] * a[5]) + a[2] * (a[3] * a[7] - a[6] * a[4]);
        if (d == 0) { for (int i = 0; i < 9; ++i) Ki[i] = 0.f; }
        else {
            d = 1 / d;
            Ki[0] = (a[4] * a[8] - a[5] * a[7]) * d; Ki[1] = (a[2] * a[7] - a[1] * a[8]) * d; Ki[2] = (a[1] * a[5] - a[2] * a[4]) * d;
            Ki[3] = (a[5] * a[6] - a[3] * a[8]) * d; Ki[4] = (a[0] * a[8] - a[2] * a[6]) * d; Ki[5] = (a[2] * a[3] - a[0] * a[5]) * d;
            Ki[6] = (a[3] * a[7] - a[4] * a[6]) * d; Ki[7] = (a[1] * a[6] - a[0] * a[7]) * d; Ki[8] = (a[0] * a[4] - a[1] * a[3]) * d;
        }
    }
    float T[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { float s = 0; for (int k = 0; k < 3; ++k) s += K[i * 3 + k] * Rt[k * 3 + j]; T[i * 3 + j] = s; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { float s = 0; for (int k = 0; k < 3; ++k) s += T[i * 3 + k] * Ki[k * 3 + j]; H[i * 3 + j] = s; }
    return LVK_OK;
}

void lvk_frontend_destroy(lvk_frontend* fe)
{
    if (!fe) return;
    if (g_ft.on && g_ft.n > 0) {
        double tot = 0; for (int i = 0; i < FT_N; ++i) tot += g_ft.acc[i];
        fprintf(stderr, "[lvk_frontend trace] %ld frames, %.1f us/frame of caller time inside the front-end\n", g_ft.n, tot / g_ft.n);
        for (int i = 0; i < FT_N; ++i) fprintf(stderr, "  %-44s %8.1f us\n", FT_NAMES[i], g_ft.acc[i] / g_ft.n);
        g_ft = FeTrace();
    }
    prof_collect(fe);
    hipStreamSynchronize(fe->ctx->stream);
#ifdef LVK_LK_BOUNDS
    fe_lk_bounds_report();
#endif
    for (int i = 0; i < 2; ++i) if (fe->side[i]) { hipStreamSynchronize(fe->side[i]->stream); lvk_context_destroy(fe->side[i]); }
    hipEvent_t evs[] = {fe->ev_pyr, fe->ev_orb, fe->ev_new, fe->ev_commit, fe->ev_tail, fe->ev_main[0], fe->ev_main[1], fe->ev_side[0], fe->ev_side[1]};
    for (hipEvent_t e : evs) if (e) hipEventDestroy(e);
    for (hipEvent_t e : fe->ev_free) hipEventDestroy(e);
    for (int i = 0; i < 3; ++i) {
        if (fe->pyr[i]) lvk_pyramid_destroy(fe->pyr[i]);
        if (fe->ext[i]) hipFree(fe->ext[i]); if (fe->blur[i]) hipFree(fe->blur[i]);
        if (i < 2) set_free(fe->set[i]);
    }
    void* ptrs[] = {fe->d_img, fe->w_curr, fe->wn_curr, fe->w_und, fe->wn_und, fe->new_pts, fe->w_status, fe->wn_status, fe->wn_desc, fe->eig, fe->mask,
                    fe->gf_scratch, fe->gf_cands, fe->dev, fe->user_mask, fe->d_gray,
                    fe->match.eig, fe->match.cand_pts, fe->match.n_cand, fe->match.cand_desc, fe->match.q, fe->match.q_desc, fe->match.res, fe->match.px, fe->match.und, fe->match.out,
                    fe->align.m, fe->align.pairs, fe->align.mask, fe->align.out, fe->map.X, fe->map.cov, fe->map.desc, fe->map.sel, fe->map.info,
                    fe->reloc.best, fe->reloc.sel, fe->reloc.px, fe->reloc.und, fe->reloc.blob, fe->loc.blob,
                    fe->merge.best, fe->merge.sel, fe->merge.ginfo, fe->merge.m, fe->merge.pairs, fe->merge.mask, fe->merge.res};
    for (void* p : ptrs) if (p) hipFree(p);
    for (int i = 0; i < 3; ++i) { if (fe->h_stage[i]) hipHostFree(fe->h_stage[i]); if (fe->d_ring[i]) hipFree(fe->d_ring[i]); if (fe->ev_img[i]) hipEventDestroy(fe->ev_img[i]); }
    for (int i = 0; i < LVK_MSG_SLOTS; ++i) if (fe->ev_msg[i]) hipEventDestroy(fe->ev_msg[i]);
    if (fe->h_msg) hipHostFree(fe->h_msg);
    if (fe->h_nmsg) hipHostFree(fe->h_nmsg);
    if (fe->h_dev) hipHostFree(fe->h_dev);
    delete fe;
}

lvk_status lvk_frontend_create(lvk_context* ctx, const lvk_fe_config* cfg, lvk_frontend** out)
{
    if (!ctx || !cfg || !out) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_create: bad argument");
    g_ft.on = getenv("LVK_FE_TRACE") != nullptr;
    if (cfg->width < 64 || cfg->height < 64) return lvk_set_error(ctx, LVK_ERR_ARG, "image too small");
    if (cfg->max_features_num <= 0 || cfg->max_features_num > FM_MAX_N) return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "max_features_num must be in 1..%d", FM_MAX_N);
    if (cfg->distortion_model != 0 && cfg->distortion_model != 1) return lvk_set_error(ctx, LVK_ERR_ARG, "distortion_model must be 0 (radtan) or 1 (equidistant)");
    if (cfg->min_distance < 1 || cfg->pub_frequency <= 0) return lvk_set_error(ctx, LVK_ERR_ARG, "min_distance >= 1 and pub_frequency > 0 required");
    if (cfg->patch_size != 15 && cfg->patch_size != 21 && cfg->patch_size != 31)
        return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "patch_size %d not instantiated (15, 21, 31)", cfg->patch_size);
    if (cfg->max_iteration < 1 || cfg->max_iteration > 100)      // cv::calcOpticalFlowPyrLK clamps the count to 0..100; 0 iterations is not a tracker
        return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "max_iteration must be in 1..100");
    if (cfg->pyramid_levels < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "pyramid_levels must be >= 0");
    {   // more levels than buffers exist only matter if the image is large enough for OpenCV's stop rule to build them
        const int small = cfg->width < cfg->height ? cfg->width : cfg->height;
        if (cfg->pyramid_levels >= LVK_MAX_LEVELS && (small >> (LVK_MAX_LEVELS - 1)) > cfg->patch_size)
            return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "pyramid_levels %d: at most %d levels are buffered", cfg->pyramid_levels, LVK_MAX_LEVELS - 1);
    }
    lvk_frontend* fe = new (std::nothrow) lvk_frontend();     // value-initialised: all PODs zero
    if (!fe) return LVK_ERR_DEVICE;
    fe->ctx = ctx; fe->cfg = *cfg; fe->cap = cfg->max_features_num; fe->image_state = 1;
    { const char* v = getenv("LVK_FE_EVENT_TRIM"); fe->ev_trim = !(v && !strcmp(v, "0")); }
    const int w = cfg->width, h = cfg->height, cap = fe->cap;
    const size_t esz = (size_t)(w + 64) * (h + 64);
    bool ok = true;
    for (int i = 0; i < 3 && ok; ++i) {
        ok = ok && lvk_pyramid_create(ctx, w, h, cfg->patch_size, cfg->pyramid_levels, &fe->pyr[i]) == LVK_OK;
        ok = ok && dalloc(&fe->ext[i], esz) && dalloc(&fe->blur[i], esz);
        if (i == 2) break;
        TrackSet& s = fe->set[i];
        ok = ok && dalloc(&s.id, cap) && dalloc(&s.pts, cap) && dalloc(&s.ppts, cap) && dalloc(&s.init, cap) && dalloc(&s.life, cap) && dalloc(&s.desc, (size_t)cap * 4);
    }
    fe->gf_cand_cap = w * h;
    size_t cand_alloc = 1; while (cand_alloc < (size_t)fe->gf_cand_cap) cand_alloc <<= 1;
    ok = ok && dalloc(&fe->d_img, (size_t)w * h) && dalloc(&fe->w_curr, cap) && dalloc(&fe->wn_curr, cap) && dalloc(&fe->w_und, 2 * (size_t)cap) && dalloc(&fe->wn_und, 2 * (size_t)cap) && dalloc(&fe->new_pts, cap) &&
         dalloc(&fe->w_status, cap) && dalloc(&fe->wn_status, cap) && dalloc(&fe->wn_desc, (size_t)cap * 4) && dalloc(&fe->eig, (size_t)w * h) &&
         dalloc(&fe->mask, (size_t)w * h) && dalloc(&fe->gf_scratch, 4 + 8192) && dalloc(&fe->gf_cands, cand_alloc) && dalloc(&fe->dev, 1);
    ok = ok && hipHostMalloc((void**)&fe->h_msg, sizeof(lvk_feature_obs) * (size_t)cap * LVK_MSG_SLOTS) == hipSuccess &&
         hipHostMalloc((void**)&fe->h_nmsg, 64 * LVK_MSG_SLOTS) == hipSuccess && hipHostMalloc((void**)&fe->h_dev, sizeof(FeDev)) == hipSuccess;
    for (int i = 0; i < LVK_MSG_SLOTS && ok; ++i) { fe->msg_pending[i].store(0); ok = hipEventCreateWithFlags(&fe->ev_msg[i], hipEventDisableTiming) == hipSuccess; }
    if (ok) {
        void *dm = nullptr, *dn = nullptr;
        ok = hipHostGetDevicePointer(&dm, fe->h_msg, 0) == hipSuccess && hipHostGetDevicePointer(&dn, fe->h_nmsg, 0) == hipSuccess && dm && dn;
        fe->d_msg = (lvk_feature_obs*)dm; fe->d_nmsg = (int*)dn;
    }
    fe->bar_push = true;
    for (int i = 0; i < 3 && fe->bar_push; ++i) {
        fe->d_ring[i] = (uint8_t*)lvk_bar_alloc(ctx->device, (size_t)w * h);
        if (!fe->d_ring[i] || hipEventCreateWithFlags(&fe->ev_img[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); fe->bar_push = false; }
    }
    for (int i = 0; i < 3 && ok; ++i) ok = hipHostMalloc((void**)&fe->h_stage[i], (size_t)w * h) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i) ok = lvk_context_create(ctx->device, &fe->side[i]) == LVK_OK;
    hipEvent_t* evs[] = {&fe->ev_pyr, &fe->ev_orb, &fe->ev_new, &fe->ev_commit, &fe->ev_tail, &fe->ev_main[0], &fe->ev_main[1], &fe->ev_side[0], &fe->ev_side[1]};
    for (hipEvent_t* e : evs) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) { lvk_frontend_destroy(fe); return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_create: allocation failed"); }
    hipMemsetAsync(fe->dev, 0, sizeof(FeDev), ctx->stream);
    hipMemsetAsync(fe->gf_scratch, 0, sizeof(unsigned) * (4 + 8192), ctx->stream);      // the selection kernel keeps its words zeroed from here on (fe_detect_new queues no fill)
    memset(&fe->cam, 0, sizeof fe->cam);
    for (int i = 0; i < 4; ++i) { fe->cam.intr[i] = cfg->intrinsics[i]; fe->cam.dist[i] = cfg->distortion[i]; }
    fe->cam.model = cfg->distortion_model; fe->cam.width = w; fe->cam.height = h;
    hipStreamSynchronize(ctx->stream);                  // the clears above are done before any of the three streams is used
    *out = fe;
    return LVK_OK;
}

static lvk_status fe_quiesce(lvk_frontend* fe)
{   // the getters look at buffers the side streams may still be filling
    for (int i = 0; i < 2; ++i) LVK_HIP(fe->ctx, hipStreamSynchronize(fe->side[i]->stream));
    return LVK_OK;
}
static lvk_status fe_read_dev(lvk_frontend* fe)
{
    LVK_HIP(fe->ctx, hipMemcpyAsync(fe->h_dev, fe->dev, sizeof(FeDev), hipMemcpyDeviceToHost, fe->ctx->stream));
    LVK_HIP(fe->ctx, hipStreamSynchronize(fe->ctx->stream));
    return LVK_OK;
}

// findNewFeaturesToBeTracked (:1005-1037).  Nothing in this frame's message depends on it, so it runs on side[0] behind the
// commit and overlaps the message read-back, the filter update and the next frame's pyramid; the next frame's LK of the new
// points is queued on the same stream, right behind it.
static lvk_status fe_detect_new(lvk_frontend* fe, int dst)
{
    lvk_context* cx = fe->side[0];
    const lvk_fe_config& c = fe->cfg;
    lvk_status st;
    // no fill launches: the mask is written whole by k_mask_max, the previous selection left the scratch words zeroed
    { ProfScope ps(fe, 6, cx->stream); st = lvk_min_eigen_map(cx, fe->pyr[1], fe->eig); }
    if (st != LVK_OK) return lvk_set_error(fe->ctx, st, "%s", cx->err);
    // the frame's tracks are final behind its second commit; with the event trims the detection waits for the message's own event instead
    // (recorded right behind the message kernel, one launch later): one record less between the commit and the message the caller waits for
    // (blocking schedules only: there the caller waits for the message; in the pipelined driver the detection is on the frame rate's recurrence
    //  and starts behind the commit, without the message kernel in front of it)
    hipStreamWaitEvent(cx->stream, (fe->ev_trim && !fe->frame_early && fe->last_msg_slot >= 0) ? fe->ev_msg[fe->last_msg_slot] : fe->ev_commit, 0);
    ProfScope ps(fe, 7, cx->stream);
    if (fe->has_user_mask) st = lvk_mask_and_max_user(cx, fe->set[dst].pts, &fe->dev->n_tracks[dst], c.width, c.height, c.min_distance, fe->eig, fe->mask, fe->gf_scratch, fe->user_mask);
    else st = lvk_mask_and_max(cx, fe->set[dst].pts, &fe->dev->n_tracks[dst], c.width, c.height, c.min_distance, fe->eig, fe->mask, fe->gf_scratch);
    if (st == LVK_OK) st = lvk_gftt_run(cx, fe->eig, fe->mask, c.width, c.height, c.max_features_num, 0.01, (double)c.min_distance, fe->gf_scratch,
                                        fe->gf_cands, fe->gf_cand_cap, fe->new_pts, fe->cap, &fe->dev->n_new, &fe->dev->n_tracks[dst], true, true);
    if (st != LVK_OK) return lvk_set_error(fe->ctx, st, "%s", cx->err);
    return LVK_OK;
}
// getFeatureMsg (:1076-1128) + publish bookkeeping (:1170-1172).  async_slot == nullptr: wait for the message and copy it out (the
// reference's synchronous processImage); otherwise return the ring slot at once - lvk_frontend_fetch_msg collects it later.
// ring entry for this frame's message (waits only if the consumer is four publishes behind)
static lvk_status fe_publish_slot(lvk_frontend* fe, int* slot_out)
{
    lvk_context* ctx = fe->ctx;
    const int slot = fe->msg_next; fe->msg_next = (slot + 1) % LVK_MSG_SLOTS;
    if (fe->msg_pending[slot].load(std::memory_order_acquire)) {       // four publishes ago and still not fetched: the consumer is far behind
        LVK_HIP(ctx, hipEventSynchronize(fe->ev_msg[slot]));
        for (int spin = 0; fe->msg_pending[slot].load(std::memory_order_acquire); ++spin) { if (spin > 2000000) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "feature-message ring overrun"); LVK_CPU_RELAX(); }
    }
    *slot_out = slot;
    return LVK_OK;
}
static FeMsgArgs fe_msg_args(lvk_frontend* fe, int slot)
{
    FeMsgArgs m;
    m.publish = 1;
    m.dt_1 = fe->curr_img_time - fe->prev_img_time;
    m.prev_is_last = fe->prev_img_time == fe->last_pub_time;
    m.dt_2 = m.prev_is_last ? m.dt_1 : fe->prev_img_time - fe->last_pub_time;
    m.out = fe->d_msg + (size_t)slot * fe->cap; m.n_host = fe->d_nmsg + 16 * slot;
    return m;
}
// after the kernel that writes the message has been queued on the main stream: event, detection of new corners, bookkeeping
// (:1170-1172); async_slot == nullptr: wait for the message and copy it out (the reference's synchronous processImage)
static lvk_status fe_publish_finish(lvk_frontend* fe, int dst, double ts, int slot, lvk_feature_obs* h_out, int cap, int* n_out, int* async_slot)
{
    hipEventRecord(fe->ev_msg[slot], fe->ctx->stream);
    fe->last_msg_slot = slot;
    fe->msg_pending[slot].store(1, std::memory_order_release);
    FT(FT_PUBLISH);
    lvk_status st = fe_detect_new(fe, dst);              // queued on side[0] before anybody blocks on the message
    if (st != LVK_OK) return st;
    FT(FT_DETECT);
    fe->last_pub_time = ts; fe->pub_counter++;
    if (async_slot) { *async_slot = slot; *n_out = 0; return LVK_OK; }
    return lvk_frontend_fetch_msg(fe, slot, h_out, cap, n_out);
}
// getFeatureMsg (:1076-1128) + publish bookkeeping (:1170-1172)
static lvk_status fe_publish(lvk_frontend* fe, int dst, double ts, lvk_feature_obs* h_out, int cap, int* n_out, int* async_slot)
{
    int slot = 0;
    lvk_status st = fe_publish_slot(fe, &slot);
    if (st != LVK_OK) return st;
    st = fe_msg_launch(fe, dst, fe_msg_args(fe, slot));
    if (st != LVK_OK) return st;
    return fe_publish_finish(fe, dst, ts, slot, h_out, cap, n_out, async_slot);
}

// The IMU-independent part of a frame: image upload, createImagePyramids (:318-334) on the main stream, ORBdescriptor ctor (:150)
// on the side stream as soon as level 0 exists (steady state) or in line (bootstrap frames).  Split out so that a pipelined
// driver can queue it before it knows which IMU samples the previous update erased (lvk_frontend_begin).
// A stream wait is a barrier packet on the waiting queue, ~6 us of queue time between two kernels even when the event fired long ago
// (profiles/r5_d_a_queue_gaps.txt: scharr -> blur 8.3 us with one event record between them against 1.5 us without; the last kernel of
// a frame -> the next frame's LK 26 us with three).  An event that HAS fired needs no packet: everything recorded before it is done.
static inline void fe_wait_unless_done(const lvk_frontend* fe, hipStream_t s, hipEvent_t ev)
{
    if (fe->ev_trim && hipEventQuery(ev) == hipSuccess) return;
    (void)hipGetLastError();                             // hipErrorNotReady is not an error
    hipStreamWaitEvent(s, ev, 0);
}
static lvk_status fe_check_image(lvk_frontend* fe, const lvk_image* img)
{   // a cv::Mat carries its own size; a caller that hands over anything but the configured resolution gets an error, not a read
    // past its buffer (e.g. TUM-VI 512x512 images under a 752x480 configuration)
    const lvk_fe_config& c = fe->cfg;
    if (!img || !img->data) return lvk_set_error(fe->ctx, LVK_ERR_ARG, "image: null pointer");
    if (img->width != c.width || img->height != c.height)
        return lvk_set_error(fe->ctx, LVK_ERR_ARG, "image is %dx%d, the front-end is configured for %dx%d", img->width, img->height, c.width, c.height);
    if (fe->pix_format == LVK_PIX_MONO8) {
        if (img->stride < c.width) return lvk_set_error(fe->ctx, LVK_ERR_ARG, "image stride %d is smaller than the width %d", img->stride, c.width);
        return LVK_OK;
    }
    const int row = c.width * lvk_pixfmt_bpp(fe->pix_format);
    if (img->stride < row)
        return lvk_set_error(fe->ctx, LVK_ERR_ARG, "image stride %d is smaller than a %s row of %d pixels (%d bytes)", img->stride, lvk_pixfmt_name(fe->pix_format), c.width, row);
    if (fe->pix_format == LVK_PIX_MONO16 && img->is_device && ((((uintptr_t)img->data) | (unsigned)img->stride) & 1u))
        return lvk_set_error(fe->ctx, LVK_ERR_ARG, "a mono16 device image needs an even address and stride");
    return LVK_OK;
}

static lvk_status fe_image_stage(lvk_frontend* fe, const lvk_image* image, bool early)
{
    lvk_context* ctx = fe->ctx;
    const lvk_fe_config& c = fe->cfg;
    lvk_status stc = fe_check_image(fe, image);
    if (stc != LVK_OK) return stc;
    const uint8_t* d_img = image->data; int d_stride = image->stride;
    const size_t row = (size_t)c.width * lvk_pixfmt_bpp(fe->pix_format);     // bytes of one raw row (= width for MONO8)
    int slot = -1;
    g_ft.start();
    if (!image->is_device && fe->bar_push && !early) {
        slot = fe->stage_next; fe->stage_next = (slot + 1) % 3;
        if (fe->ev_img_set[slot]) LVK_HIP(ctx, hipEventSynchronize(fe->ev_img[slot]));      // the kernels that read this buffer three frames ago
        if (fe->n_img >= 3) LVK_HIP(ctx, hipEventSynchronize(fe->ev_end[fe->n_img & 1]));   // (the same bound on frames in flight as the pinned-slot path)
        FT(FT_SLOT_WAIT);
        uint8_t* dd = fe->d_ring[slot];
        if ((size_t)image->stride == row) memcpy(dd, image->data, row * c.height);
        else for (int y = 0; y < c.height; ++y) memcpy(dd + (size_t)y * row, image->data + (size_t)y * image->stride, row);
        LVK_STORE_FENCE();
        FT(FT_STAGE_COPY);
        d_img = dd; d_stride = (int)row;
        FT(FT_UPLOAD);
    } else if (!image->is_device) {
        slot = fe->stage_next; fe->stage_next = (slot + 1) % 3;
        // The slot was last used three frames back.  Its upload precedes frame f-2's image stage on the image stream, which the
        // main stream waited for before it recorded the end of frame f-2: that event covers it (and has long fired) - no per-slot event.
        if (fe->n_img >= 3) LVK_HIP(ctx, hipEventSynchronize(fe->ev_end[fe->n_img & 1]));
        FT(FT_SLOT_WAIT);
        uint8_t* hs = fe->h_stage[slot];
        if ((size_t)image->stride == row) memcpy(hs, image->data, row * c.height);
        else for (int y = 0; y < c.height; ++y) memcpy(hs + (size_t)y * row, image->data + (size_t)y * image->stride, row);
        FT(FT_STAGE_COPY);
        LVK_HIP(ctx, hipMemcpyAsync(fe->d_img, hs, row * c.height, hipMemcpyHostToDevice, fe->side[1]->stream)); d_img = fe->d_img;
        d_stride = (int)row;
        FT(FT_UPLOAD);
    }
    lvk_status st;
    lvk_context* icx = fe->side[1];
    hipStream_t S0 = icx->stream;
    // The buffer set about to be written (frame f) was the spare set of frame f-1 and the "prev" set of frame f-2: its last readers are
    // frame f-2's tracking chains and the detection queued behind frame f-3 (same side stream, earlier in order).  Waiting for the
    // ends of frame f-2's two chains is therefore enough, and frame f-1's tracking runs concurrently with this image stage.
    if (fe->n_img >= 2) {
        const int par = (int)(fe->n_img & 1);            // parity of f-2
        fe_wait_unless_done(fe, S0, fe->ev_end[par]); fe_wait_unless_done(fe, S0, fe->ev_side[par]);
    }
    int mosaic_done = 0;
    {
        ProfScope ps(fe, 0, S0);
        st = LVK_OK;
        if (fe->pix_format != LVK_PIX_MONO8) {               // raw bytes of any of the three routes -> the packed grey plane
            st = lvk_image_to_gray(icx, d_img, d_stride, c.width, c.height, fe->pix_format, fe->pix_shift, fe->d_gray, c.width);
            d_img = fe->d_gray; d_stride = c.width;
        }
        if (st == LVK_OK) st = lvk_pyramid_build_with_orb(icx, fe->pyr[1], d_img, d_stride, c.flag_equalize, 3.0, 8, 8, fe->ext[1], &mosaic_done);
    }
    if (st != LVK_OK) return lvk_set_error(ctx, st, "%s", icx->err);
    // (the slot's readers - the two kernels above - are covered by the end-of-frame event of frame f-2 the caller waits for anyway, as in
    //  the pinned-slot path: no event of their own)
    if (slot >= 0 && fe->bar_push && !fe->ev_trim) { hipEventRecord(fe->ev_img[slot], S0); fe->ev_img_set[slot] = true; }
    // queued ahead of the frame's tracking (pipelined driver): the ORB planes are done long before anybody asks, one event (ev_orb)
    // stands for the whole stage; queued together with the tracking (blocking API): LK may start as soon as the pyramid exists
    // (rounds 1-4 recorded ev_pyr here in the blocking schedules so that the frame could start on the pyramid alone; but the first thing a
    //  steady-state frame queues is LK, whose second wavefront reads the ORB planes and waits for ev_orb anyway: the split only put a
    //  record between the last Scharr launch and the blur, and a second wait on both tracking streams)
    fe->frame_early = early;
    const bool split = !early && !fe->ev_trim;
    if (split) hipEventRecord(fe->ev_pyr, S0);
    fe->pyr_event = split;
    { ProfScope ps(fe, 1, S0); st = mosaic_done ? lvk_orb_blur_only(icx, fe->pyr[1], fe->ext[1], fe->blur[1]) : lvk_orb_prepare(icx, fe->pyr[1], fe->ext[1], fe->blur[1]); }
    if (st != LVK_OK) return lvk_set_error(ctx, st, "%s", icx->err);
    hipEventRecord(fe->ev_orb, S0);
    fe->n_img += 1;
    FT(FT_IMAGE_LAUNCH);
    return LVK_OK;
}

static lvk_status fe_check_failed(lvk_frontend* fe)
{
    if (fe->failed == LVK_OK) return LVK_OK;
    return lvk_set_error(fe->ctx, fe->failed, "the front-end is in a failed state after an earlier error (%s); destroy and re-create it", fe->failed_msg);
}
static lvk_status fe_note_failure(lvk_frontend* fe, lvk_status st)
{   // argument errors are raised before anything is queued and leave the handle usable; everything else is sticky
    if (st != LVK_OK && st != LVK_ERR_ARG && fe->failed == LVK_OK) {
        fe->failed = st; snprintf(fe->failed_msg, sizeof fe->failed_msg, "%s", fe->ctx->err);
        hipStreamSynchronize(fe->ctx->stream);
        for (int i = 0; i < 2; ++i) if (fe->side[i]) hipStreamSynchronize(fe->side[i]->stream);
    }
    return st;
}

lvk_status lvk_frontend_begin(lvk_frontend* fe, const lvk_image* img, double ts)
{
    if (!fe || !img) return LVK_ERR_ARG;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (!fe->b_first_img) return fe_check_image(fe, img);   // the first-image gate needs the IMU buffer (:134-142): nothing to do early
    // one image stage per frame: the buffer-set rotation and the end-of-frame events are indexed by the stages queued so far
    if (fe->image_done) return lvk_set_error(fe->ctx, LVK_ERR_ARG, "lvk_frontend_begin: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    lvk_status st = fe_image_stage(fe, img, true);
    if (st != LVK_OK) return fe_note_failure(fe, st);
    fe->image_done = true; fe->image_done_ts = ts;
    return LVK_OK;
}

// processImage is synchronous in the reference: when it returns the caller may free or overwrite the image.  Same here: a host
// image has been copied into the pinned staging ring by the time the call returns (the frame's kernels keep running).
static lvk_status frontend_process(lvk_frontend* fe, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu,
                                   lvk_feature_obs* h_out, int cap, int* n_out, int* has_msg, int* async_slot)
{
    if (!fe || !img || !n_out || !has_msg || (n_imu > 0 && !h_imu)) return lvk_set_error(fe ? fe->ctx : nullptr, LVK_ERR_ARG, "lvk_frontend_process: bad argument");
    lvk_context* ctx = fe->ctx;
    const lvk_fe_config& c = fe->cfg;
    *n_out = 0; *has_msg = 0;
    if (!fe->b_first_img) {                                          // :134-142
        if (n_imu > 0 && h_imu[0].t - ts <= 0.0) fe->b_first_img = true;
        else return fe_check_image(fe, img);
    }
    lvk_status st = LVK_OK;
    if (fe->image_done && fe->image_done_ts != ts)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_process(t = %.6f) after lvk_frontend_begin(t = %.6f): the queued image stage belongs to another frame", ts, fe->image_done_ts);
    if (!fe->image_done) st = fe_image_stage(fe, img, false);
    else FT(FT_OUTSIDE);                                 // (the stage was queued by lvk_frontend_begin: what lies between is the caller's)
    fe->image_done = false;
    if (st != LVK_OK) return st;
    hipStream_t S1 = ctx->stream, S2 = fe->side[0]->stream;
    {   // this frame's pyramid (and ORB planes) come from the image stream
        hipEvent_t ready = fe->pyr_event ? fe->ev_pyr : fe->ev_orb;
        if (!(fe->ev_trim && hipEventQuery(ready) == hipSuccess)) { (void)hipGetLastError(); hipStreamWaitEvent(S1, ready, 0); hipStreamWaitEvent(S2, ready, 0); }
    }
    // the side stream reads (new points, their count) and overwrites (wn_*) what the previous frame's commits on the main stream used
    if (fe->n_img >= 2) fe_wait_unless_done(fe, S2, fe->ev_end[fe->n_img & 1]);
    FT(FT_FRAME_WAITS);
    fe->prof_take = fe->prof_stride <= 1 || fe->n_img % fe->prof_stride == 0;
    fe->last_msg_slot = -1;
    fe->curr_img_time = ts;
    const double pub_gate = 0.9 * (1.0 / c.pub_frequency);
    const int src = fe->cur, dst = fe->cur ^ 1;
    bool curr_valid = false;            // curr_pts_ (set[dst]) holds this frame's tracks

    if (fe->image_state != 3) {
        // bootstrap frames run on the main stream alone, behind whatever side[0] still has in flight
        hipEventRecord(fe->ev_tail, S2);
        hipStreamWaitEvent(S1, fe->ev_tail, 0);
    }
    if (fe->image_state == 1) {
        // initializeFirstFrame (:337-352): goodFeaturesToTrack(max_features_num, 0.01, min_distance), no mask - or the caller's
        { ProfScope ps(fe, 6); st = lvk_min_eigen_map(ctx, fe->pyr[1], fe->eig); }
        if (st == LVK_OK) st = lvk_gftt_run(ctx, fe->eig, fe->has_user_mask ? fe->user_mask : nullptr, c.width, c.height, c.max_features_num, 0.01, (double)c.min_distance, fe->gf_scratch,
                                            fe->gf_cands, fe->gf_cand_cap, fe->new_pts, fe->cap, &fe->dev->n_new, nullptr, false, false);
        if (st == LVK_OK) st = fe_read_dev(fe);
        if (st != LVK_OK) return st;
        fe->last_pub_time = ts;
        if (fe->h_dev->n_new > 20) fe->image_state = 2;
    } else {
        HMat H;
        st = lvk_predict_homography(h_imu, n_imu, fe->prev_img_time, ts, c.R_cam_imu, c.intrinsics, H.h);
        if (st != LVK_OK) return lvk_set_error(ctx, st, "predict_homography failed");
        FT(FT_PREDICT);
        if (fe->image_state == 2) {
            // initializeFirstFeatures (:355-537)
            st = track_chain(fe, S1, fe->new_pts, &fe->dev->n_new, H, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, 1);
            if (st == LVK_OK) st = commit(fe, 2, fe->new_pts, &fe->dev->n_new, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, dst);
            if (st == LVK_OK) st = fe_read_dev(fe);
            if (st != LVK_OK) return st;
            if (!fe->h_dev->boot_ok) fe->image_state = 1;
            else {
                curr_valid = true;
                if (!fe->ev_trim || (fe->frame_early && ts - fe->last_pub_time >= pub_gate)) hipEventRecord(fe->ev_commit, S1);      // only the detection of a publish frame waits for it - and in the blocking schedules for the message's event instead (fe_detect_new)
                if (ts - fe->last_pub_time >= pub_gate) {
                    st = fe_publish(fe, dst, ts, h_out, cap, n_out, async_slot);
                    if (st != LVK_OK) return st;
                    *has_msg = 1;
                }
                fe->image_state = 3;
            }
        } else {
            // trackFeatures (:540-811) on the main stream; trackNewFeatures' LK and descriptor gate (:813-931) on side[0], queued
            // behind the detection that produced the points; its RANSAC + append (:932-1001) joins the main stream.
            // (the side stream already waited for ev_pyr before the ORB planes: this frame's pyramid and everything the previous
            //  frame left on the main stream are done)
            const TrackSet& so = fe->set[src];
            if (lvk_lk_choice(c.patch_size, fe->cap, fe->pyr[0]->n_levels, fe->pyr[1]->n_levels).merged) {
                // ONE launch for both chains (LkSet), on the main stream.  The new points were written by the detection the previous publish
                // frame queued on side[0]: its end-of-frame event (fired long ago unless the caller runs a frame ahead of the GPU)
                if (fe->n_img >= 2) fe_wait_unless_done(fe, S1, fe->ev_side[(int)(fe->n_img & 1)]);
                st = track_chain_merged(fe, S1, src, H);
                if (st != LVK_OK) return st;
                FT(FT_TRACK_LAUNCH);
                st = commit(fe, 0, so.pts, &fe->dev->n_tracks[src], fe->w_curr, fe->w_status, &so, so.desc, dst);
                if (st == LVK_OK) st = commit(fe, 1, fe->new_pts, &fe->dev->n_new, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, dst);
                if (st != LVK_OK) return st;
            } else {
            st = track_chain(fe, S2, fe->new_pts, &fe->dev->n_new, H, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, 1);
            hipEventRecord(fe->ev_new, S2);
            if (st == LVK_OK) st = track_chain(fe, S1, fe->set[src].pts, &fe->dev->n_tracks[src], H, fe->w_curr, fe->w_status, fe->set[src].desc, nullptr, 0);
            if (st != LVK_OK) return st;
            FT(FT_TRACK_LAUNCH);
            // the old tracks' RANSAC + commit overlaps the wait for the new points' chain; their append and the message follow.
            // (Both commits - and all three stages - as ONE launch were measured in same-box A/B runs and were slower: the old tracks'
            //  commit then waits for the new points' chain; profiles/r3_jk_frontend_chain_ab.json)
            st = commit(fe, 0, so.pts, &fe->dev->n_tracks[src], fe->w_curr, fe->w_status, &so, so.desc, dst);
            hipStreamWaitEvent(S1, fe->ev_new, 0);
            if (st == LVK_OK) st = commit(fe, 1, fe->new_pts, &fe->dev->n_new, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, dst);
            if (st != LVK_OK) return st;
            }
            curr_valid = true;
            if (!fe->ev_trim || (fe->frame_early && ts - fe->last_pub_time >= pub_gate)) hipEventRecord(fe->ev_commit, S1);          // only the detection of a publish frame waits for it - and in the blocking schedules for the message's event instead (fe_detect_new)
            FT(FT_COMMIT_LAUNCH);
            if (ts - fe->last_pub_time >= pub_gate) {
                st = fe_publish(fe, dst, ts, h_out, cap, n_out, async_slot);
                if (st != LVK_OK) return st;
                *has_msg = 1;
            }
        }
    }
    if (!curr_valid) LVK_HIP(ctx, hipMemsetAsync(&fe->dev->n_tracks[dst], 0, sizeof(int), ctx->stream));
    {   const int par = (int)((fe->n_img - 1) & 1);
        if (fe->ev_trim && fe->last_msg_slot >= 0 && curr_valid) fe->ev_end[par] = fe->ev_msg[fe->last_msg_slot];     // recorded right behind the message kernel, the frame's last launch on this stream
        else { hipEventRecord(fe->ev_main[par], S1); fe->ev_end[par] = fe->ev_main[par]; }
        hipEventRecord(fe->ev_side[par], S2); }
    // rotation (:207-216), three-way: curr becomes prev, the spare set becomes the next frame's curr
    { lvk_pyramid* p = fe->pyr[0]; fe->pyr[0] = fe->pyr[1]; fe->pyr[1] = fe->pyr[2]; fe->pyr[2] = p; }
    { uint8_t* p = fe->ext[0]; fe->ext[0] = fe->ext[1]; fe->ext[1] = fe->ext[2]; fe->ext[2] = p;
      p = fe->blur[0]; fe->blur[0] = fe->blur[1]; fe->blur[1] = fe->blur[2]; fe->blur[2] = p; }
    fe->cur = dst;
    fe->prev_img_time = ts;
    if (fe->pending.size() > 4096) prof_collect(fe);
    FT(FT_END); g_ft.n++;
    return LVK_OK;
}
// the blocking entry: a publish frame waits for its message and copies it out
lvk_status lvk_frontend_process(lvk_frontend* fe, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu,
                                lvk_feature_obs* h_out, int cap, int* n_out, int* has_msg)
{
    if (fe) { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    const lvk_status st = frontend_process(fe, img, ts, h_imu, n_imu, h_out, cap, n_out, has_msg, nullptr);
    return fe ? fe_note_failure(fe, st) : st;
}
// the pipelined driver's variant: nothing waits for the GPU; *slot names the ring entry the message will appear in
lvk_status lvk_frontend_process_async(lvk_frontend* fe, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* has_msg, int* slot)
{
    int n = 0;
    if (!slot) return LVK_ERR_ARG;
    *slot = -1;
    if (fe) { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    const lvk_status st = frontend_process(fe, img, ts, h_imu, n_imu, nullptr, 0, &n, has_msg, slot);
    return fe ? fe_note_failure(fe, st) : st;
}
// wait for the message of ring entry `slot` and copy it out (any thread)
lvk_status lvk_frontend_fetch_msg(lvk_frontend* fe, int slot, lvk_feature_obs* h_out, int cap, int* n_out)
{
    if (!fe || slot < 0 || slot >= LVK_MSG_SLOTS || !n_out) return LVK_ERR_ARG;
    const hipError_t er = hipEventSynchronize(fe->ev_msg[slot]);
    if (er != hipSuccess) return lvk_set_error(fe->ctx, LVK_ERR_DEVICE, "feature message: %s", hipGetErrorString(er));
    int n = fe->h_nmsg[16 * slot];
    if (n > cap) n = cap;
    if (h_out && n > 0) memcpy(h_out, fe->h_msg + (size_t)slot * fe->cap, sizeof(lvk_feature_obs) * (size_t)n);
    *n_out = n;
    fe->msg_pending[slot].store(0, std::memory_order_release);
    return LVK_OK;
}

lvk_status lvk_frontend_tracks(lvk_frontend* fe, uint64_t* h_ids, lvk_pt2f* h_pts, int* h_lifetime, lvk_pt2f* h_init, uint8_t* h_desc, int cap, int* n_out)
{
    if (!fe || !n_out) return LVK_ERR_ARG;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    lvk_status st = fe_read_dev(fe);
    if (st != LVK_OK) return st;
    const TrackSet& s = fe->set[fe->cur];
    int n = fe->h_dev->n_tracks[fe->cur];
    if (n > cap) n = cap;
    lvk_context* ctx = fe->ctx;
    if (n > 0) {
        if (h_ids) LVK_HIP(ctx, hipMemcpy(h_ids, s.id, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
        if (h_pts) LVK_HIP(ctx, hipMemcpy(h_pts, s.pts, sizeof(lvk_pt2f) * (size_t)n, hipMemcpyDeviceToHost));
        if (h_lifetime) LVK_HIP(ctx, hipMemcpy(h_lifetime, s.life, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        if (h_init) LVK_HIP(ctx, hipMemcpy(h_init, s.init, sizeof(lvk_pt2f) * (size_t)n, hipMemcpyDeviceToHost));
        if (h_desc) LVK_HIP(ctx, hipMemcpy(h_desc, s.desc, (size_t)32 * n, hipMemcpyDeviceToHost));
    }
    *n_out = n;
    return LVK_OK;
}

lvk_status lvk_frontend_new_pts(lvk_frontend* fe, lvk_pt2f* h_pts, int cap, int* n_out)
{
    if (!fe || !n_out) return LVK_ERR_ARG;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    lvk_status st = fe_read_dev(fe);
    if (st != LVK_OK) return st;
    int n = fe->h_dev->n_new; if (n > cap) n = cap;
    if (n > 0 && h_pts) LVK_HIP(fe->ctx, hipMemcpy(h_pts, fe->new_pts, sizeof(lvk_pt2f) * (size_t)n, hipMemcpyDeviceToHost));
    *n_out = n;
    return LVK_OK;
}

int lvk_frontend_state(const lvk_frontend* fe) { return fe ? fe->image_state : 0; }

// A caller's region mask for corner detection (OpenCV's mask argument; no reference counterpart).  Everything queued so far is waited
// for first, so a detection already in flight keeps the mask it was queued with; the mask is then stored packed and 0 / 255.
lvk_status lvk_frontend_set_mask(lvk_frontend* fe, const lvk_image* mask)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    const int w = fe->cfg.width, h = fe->cfg.height;
    if (mask) {
        if (!mask->data) return lvk_set_error(ctx, LVK_ERR_ARG, "mask: null pointer");
        if (mask->width != w || mask->height != h)
            return lvk_set_error(ctx, LVK_ERR_ARG, "mask is %dx%d, the front-end is configured for %dx%d", mask->width, mask->height, w, h);
        if (mask->stride < w) return lvk_set_error(ctx, LVK_ERR_ARG, "mask stride %d is smaller than the width %d", mask->stride, w);
    }
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 2; ++i) LVK_HIP(ctx, hipStreamSynchronize(fe->side[i]->stream));
    if (!mask) { fe->has_user_mask = false; return LVK_OK; }
    const size_t n = (size_t)w * h;
    if (!fe->user_mask && !dalloc(&fe->user_mask, n)) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_set_mask: allocation failed");
    if (mask->is_device) {
        lvk_status st = lvk_mask_normalise(ctx, mask->data, mask->stride, w, h, fe->user_mask);
        if (st != LVK_OK) return st;
        LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<uint8_t> packed(n);
        for (int y = 0; y < h; ++y) {
            const uint8_t* src = mask->data + (size_t)y * mask->stride; uint8_t* dst = packed.data() + (size_t)y * w;
            for (int x = 0; x < w; ++x) dst[x] = src[x] ? 255 : 0;
        }
        LVK_HIP(ctx, hipMemcpy(fe->user_mask, packed.data(), n, hipMemcpyHostToDevice));
    }
    fe->has_user_mask = true;
    return LVK_OK;
}
int lvk_frontend_has_mask(const lvk_frontend* fe) { return fe && fe->has_user_mask ? 1 : 0; }

// The caller's pixel format (no reference counterpart: its ROS caller converts on the host).  Everything queued so far is waited for
// first, as in lvk_frontend_set_mask: a frame in flight keeps the buffers it was queued with.  The new upload buffers are all allocated
// before an old one is freed, so that a failure leaves the front-end exactly as it was.
lvk_status lvk_frontend_set_input_format(lvk_frontend* fe, int format, int shift)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    const int w = fe->cfg.width, h = fe->cfg.height, bpp = lvk_pixfmt_bpp(format);
    if (!bpp) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_input_format: unknown format %d", format);
    if (shift < 0 || shift > 8 || (shift != 0 && format != LVK_PIX_MONO16))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_input_format: shift %d (0..8, and only with mono16; the format is %s)", shift, lvk_pixfmt_name(format));
    if ((format == LVK_PIX_YUYV || format == LVK_PIX_UYVY) && (w & 1))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_input_format: %s needs an even width, the front-end is configured for %dx%d", lvk_pixfmt_name(format), w, h);
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_input_format: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 2; ++i) LVK_HIP(ctx, hipStreamSynchronize(fe->side[i]->stream));
    const size_t old_bytes = (size_t)w * h * lvk_pixfmt_bpp(fe->pix_format), bytes = (size_t)w * h * bpp;
    uint8_t *n_stage[3] = {nullptr, nullptr, nullptr}, *n_ring[3] = {nullptr, nullptr, nullptr}, *n_img = nullptr, *n_gray = nullptr;
    bool ok = true;
    if (bytes != old_bytes) {
        for (int i = 0; i < 3 && ok; ++i) ok = hipHostMalloc((void**)&n_stage[i], bytes) == hipSuccess;
        for (int i = 0; i < 3 && ok && fe->bar_push; ++i) ok = (n_ring[i] = (uint8_t*)lvk_bar_alloc(ctx->device, bytes)) != nullptr;
        ok = ok && dalloc(&n_img, bytes);
    }
    if (format != LVK_PIX_MONO8 && !fe->d_gray) ok = ok && dalloc(&n_gray, (size_t)w * h);
    if (!ok) {
        (void)hipGetLastError();
        for (int i = 0; i < 3; ++i) { if (n_stage[i]) hipHostFree(n_stage[i]); if (n_ring[i]) hipFree(n_ring[i]); }
        if (n_img) hipFree(n_img); if (n_gray) hipFree(n_gray);
        return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_set_input_format: allocation failed (%s stays in force)", lvk_pixfmt_name(fe->pix_format));
    }
    if (bytes != old_bytes) {
        for (int i = 0; i < 3; ++i) {
            hipHostFree(fe->h_stage[i]); fe->h_stage[i] = n_stage[i];
            if (fe->bar_push) { hipFree(fe->d_ring[i]); fe->d_ring[i] = n_ring[i]; fe->ev_img_set[i] = false; }
        }
        hipFree(fe->d_img); fe->d_img = n_img;
    }
    if (n_gray) fe->d_gray = n_gray;
    if (format == LVK_PIX_MONO8 && fe->d_gray) { hipFree(fe->d_gray); fe->d_gray = nullptr; }
    fe->pix_format = format; fe->pix_shift = shift;
    return LVK_OK;
}
int lvk_frontend_input_format(const lvk_frontend* fe) { return fe ? fe->pix_format : -1; }

// Map points in the last processed frame (no reference counterpart): fresh corners of that frame without any mask, their descriptors, the
// guided matcher, the matched pixels normalised.  After the rotation the frame's pyramid and ORB planes are pyr[0], ext[0], blur[0]; the next
// frame's image stage writes set [1], so nothing here races with a frame queued later on the main stream, and every buffer written is the
// call's own (fe->match) or the main context's stage scratch: the detection's eig / mask / scratch on side[0] are not touched.
#define FE_MATCH_MAX_CAND 4096
#define FE_MATCH_MAX_Q    1024
// the options with their defaults filled in and their ranges checked, as lvk_frontend_match_landmarks states them
static lvk_status fe_match_options(lvk_frontend* fe, const char* who, const lvk_match_options* opt, lvk_match_options* out)
{
    lvk_context* ctx = fe->ctx;
    lvk_match_options o = {0, 0., 0., 0, 0};
    if (opt) o = *opt;
    if (o.max_candidates == 0) o.max_candidates = FE_MATCH_MAX_CAND;
    if (o.quality == 0.) o.quality = 0.01;
    if (o.min_distance == 0.) o.min_distance = (double)fe->cfg.min_distance;
    if (o.max_dist == 0) o.max_dist = 58;
    if (o.ratio_pct == 0) o.ratio_pct = 100;
    if (o.max_candidates < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: max_candidates %d", who, o.max_candidates);
    if (o.max_candidates > FE_MATCH_MAX_CAND) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "%s: max_candidates %d, at most %d", who, o.max_candidates, FE_MATCH_MAX_CAND);
    if (!(o.quality > 0. && o.quality <= 1.)) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: quality must be in (0, 1]", who);
    if (!std::isfinite(o.min_distance) || o.min_distance < 0.) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: min_distance is negative or not finite", who);
    if (o.max_dist < 0 || o.max_dist > 256) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: max_dist %d outside 1..256", who, o.max_dist);
    if (o.ratio_pct < 1 || o.ratio_pct > 100) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: ratio_pct %d outside 1..100", who, o.ratio_pct);
    if (fe->n_img == 0) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: no frame has been processed yet", who);
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "%s: the image stage of t = %.6f is still waiting for its lvk_frontend_process", who, fe->image_done_ts);
    *out = o;
    return LVK_OK;
}
// the matcher's buffers, allocated by the first call that needs them
static lvk_status fe_match_buffers(lvk_frontend* fe)
{
    if (fe->match.eig) return LVK_OK;
    const int w = fe->cfg.width, h = fe->cfg.height;
    lvk_frontend::Match a = {};
    const bool ok = dalloc(&a.eig, (size_t)w * h) && dalloc(&a.cand_pts, FE_MATCH_MAX_CAND) && dalloc(&a.n_cand, 1) && dalloc(&a.cand_desc, (size_t)32 * FE_MATCH_MAX_CAND) &&
                    dalloc(&a.q, FE_MATCH_MAX_Q) && dalloc(&a.q_desc, (size_t)32 * FE_MATCH_MAX_Q) && dalloc(&a.res, FE_MATCH_MAX_Q) && dalloc(&a.px, FE_MATCH_MAX_Q) &&
                    dalloc(&a.und, FE_MATCH_MAX_Q) && dalloc(&a.out, FE_MATCH_MAX_Q);
    if (!ok) {
        (void)hipGetLastError();
        void* ptrs[] = {a.eig, a.cand_pts, a.n_cand, a.cand_desc, a.q, a.q_desc, a.res, a.px, a.und, a.out};
        for (void* p : ptrs) if (p) hipFree(p);
        return lvk_set_error(fe->ctx, LVK_ERR_DEVICE, "lvk_frontend_match_landmarks: allocation failed");
    }
    fe->match = a;
    return LVK_OK;
}
// The device chain of lvk_frontend_match_landmarks on n_q queries that are already in fe->match.q / q_desc (their upload, or the kernels
// that wrote them, queued on the main stream): corners of the last processed frame, their descriptors, the matcher, the records in
// fe->match.out.  Waits once, for the corner count; the records are not waited for.
// The first half of that chain, shared with lvk_frontend_relocalise_map: the corners of the last processed frame into fe->match.cand_pts
// (no mask), a wait for their count, and - when describe - their descriptors into fe->match.cand_desc, queued and not waited for.
static lvk_status fe_match_corners(lvk_frontend* fe, const char* who, const lvk_match_options& o, bool describe, int* n_cand_out)
{
    lvk_context* ctx = fe->ctx;
    const int w = fe->cfg.width, h = fe->cfg.height;
    lvk_frontend::Match& m = fe->match;
    lvk_status st = lvk_min_eigen_map(ctx, fe->pyr[0], m.eig);
    if (st == LVK_OK) st = lvk_good_features_from_map(ctx, m.eig, nullptr, w, h, o.max_candidates, o.quality, o.min_distance, m.cand_pts, FE_MATCH_MAX_CAND, m.n_cand);
    if (st != LVK_OK) return st;
    int n_cand = 0;
    LVK_HIP(ctx, hipMemcpyAsync(&n_cand, m.n_cand, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_cand < 0 || n_cand > FE_MATCH_MAX_CAND) return lvk_set_error(ctx, LVK_ERR_DEVICE, "%s: the selection reported %d corners", who, n_cand);
    *n_cand_out = n_cand;
    if (!describe) return LVK_OK;
    return lvk_orb_describe(ctx, fe->ext[0], fe->blur[0], w, h, m.cand_pts, n_cand, m.cand_desc, nullptr);
}
static lvk_status fe_match_chain(lvk_frontend* fe, const char* who, const lvk_match_options& o, int n_q, int* n_cand_out)
{
    lvk_context* ctx = fe->ctx;
    lvk_frontend::Match& m = fe->match;
    int n_cand = 0;
    lvk_status st = fe_match_corners(fe, who, o, n_q > 0, &n_cand);
    if (st != LVK_OK) return st;
    if (n_cand_out) *n_cand_out = n_cand;
    if (n_q == 0) return LVK_OK;
    st = lvk_orb_match_guided(ctx, m.cand_pts, m.cand_desc, n_cand, m.q, m.q_desc, n_q, o.max_dist, o.ratio_pct, m.res);
    if (st == LVK_OK) st = fe_match_finish(ctx, fe->cam, m.res, m.cand_pts, n_q, m.px, m.und, m.out);
    return st;
}

lvk_status lvk_frontend_match_landmarks(lvk_frontend* fe, const lvk_match_query* h_q, const uint8_t* h_desc, int n_q, const lvk_match_options* opt,
                                        lvk_landmark_match* h_out, int* n_cand_out)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (n_q < 0 || (n_q > 0 && (!h_q || !h_desc || !h_out))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_match_landmarks: bad argument");
    if (n_q > FE_MATCH_MAX_Q) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_match_landmarks: %d queries, at most %d", n_q, FE_MATCH_MAX_Q);
    lvk_match_options o;
    lvk_status st = fe_match_options(fe, "lvk_frontend_match_landmarks", opt, &o);
    if (st == LVK_OK) st = fe_match_buffers(fe);
    if (st != LVK_OK) return st;
    lvk_frontend::Match& m = fe->match;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    if (n_q > 0) {
        LVK_HIP(ctx, hipMemcpyAsync(m.q, h_q, sizeof(lvk_match_query) * (size_t)n_q, hipMemcpyHostToDevice, ctx->stream));
        LVK_HIP(ctx, hipMemcpyAsync(m.q_desc, h_desc, (size_t)32 * n_q, hipMemcpyHostToDevice, ctx->stream));
    }
    st = fe_match_chain(fe, "lvk_frontend_match_landmarks", o, n_q, n_cand_out);
    if (st != LVK_OK) { (void)hipStreamSynchronize(ctx->stream); return st; }      // (the uploads read the caller's arrays)
    if (n_q == 0) return LVK_OK;
    LVK_HIP(ctx, hipMemcpyAsync(h_out, m.out, sizeof(lvk_landmark_match) * (size_t)n_q, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (h_q and h_desc are the caller's pageable arrays: their copies are done too)
    return LVK_OK;
}

// The prior map, resident on the device (no reference counterpart).  New buffers are filled before the old ones go, so a refusal leaves
// the map in force; lvk_frontend_match_map always returns with its work done, so nothing reads the old buffers when they are freed.
lvk_status lvk_frontend_set_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, int n)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (n < 0 || (n > 0 && (!h_X || !h_desc))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_map: bad argument");
    if (n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_set_map: %d points, at most %d", n, LVK_MAP_MAX_POINTS);
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_set_map: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    lvk_frontend::Map b = {};
    if (n > 0) {
        const bool ok = dalloc(&b.X, (size_t)3 * n) && (!h_cov9 || dalloc(&b.cov, (size_t)9 * n)) && dalloc(&b.desc, (size_t)32 * n) && dalloc(&b.sel, LVK_MAP_MAX_QUERIES) &&
                        dalloc(&b.info, 1);
        hipError_t e = ok ? hipMemcpyAsync(b.X, h_X, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream) : hipErrorOutOfMemory;
        if (e == hipSuccess && h_cov9) e = hipMemcpyAsync(b.cov, h_cov9, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.desc, h_desc, (size_t)32 * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            void* ptrs[] = {b.X, b.cov, b.desc, b.sel, b.info};
            for (void* p : ptrs) if (p) hipFree(p);
            return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_set_map: %s", ok ? hipGetErrorString(e) : "allocation failed");
        }
        b.n = n;
    }
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void* old[] = {fe->map.X, fe->map.cov, fe->map.desc, fe->map.sel, fe->map.info};
    for (void* p : old) if (p) hipFree(p);
    fe->map = b;
    return LVK_OK;
}
int lvk_frontend_map_size(const lvk_frontend* fe) { return fe ? fe->map.n : -1; }

// A session's raw exports into the map in force (no reference counterpart): upload, lvk_map_build in buffers the call owns, one wait for the
// counts, then the map's own buffers at their final size are filled from the gathered arrays before the old ones go - as in
// lvk_frontend_set_map, a refusal leaves the map in force.
lvk_status lvk_frontend_build_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, const double* h_score, int n,
                                  const lvk_map_build_options* opt, int* h_order, int cap_order, lvk_map_build_info* info)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (n < 0 || cap_order < 0 || (n > 0 && (!h_X || !h_desc))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_build_map: bad argument");
    const char* why = "";
    if (!fe_map_build_options_ok(opt, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_build_map: %s", why);
    if (n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_build_map: %d points, at most %d", n, LVK_MAP_MAX_POINTS);
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_build_map: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    // the call's own buffers: the inputs, the gathered outputs (room for n each), the order and the counts
    double *in_X = nullptr, *in_cov = nullptr, *in_score = nullptr, *out_X = nullptr, *out_cov = nullptr;
    uint8_t *in_desc = nullptr, *out_desc = nullptr; int* order = nullptr; lvk_map_build_info* d_info = nullptr;
    lvk_frontend::Map b = {};
    lvk_map_build_info got;
    memset(&got, 0, sizeof got);
    auto release = [&]() {
        void* ptrs[] = {in_X, in_cov, in_score, out_X, out_cov, in_desc, out_desc, order, d_info};
        for (void* p : ptrs) if (p) hipFree(p);
    };
    auto fail = [&](lvk_status code, const char* what) {
        (void)hipStreamSynchronize(ctx->stream);         // (the uploads read the caller's arrays)
        (void)hipGetLastError();
        release();
        void* ptrs[] = {b.X, b.cov, b.desc, b.sel, b.info};
        for (void* p : ptrs) if (p) hipFree(p);
        return lvk_set_error(ctx, code, "lvk_frontend_build_map: %s", what);
    };
    if (n > 0) {
        const size_t N = (size_t)n;
        const bool ok = dalloc(&in_X, 3 * N) && (!h_cov9 || dalloc(&in_cov, 9 * N)) && dalloc(&in_desc, 32 * N) && (!h_score || dalloc(&in_score, N)) && dalloc(&out_X, 3 * N) &&
                        (!h_cov9 || dalloc(&out_cov, 9 * N)) && dalloc(&out_desc, 32 * N) && dalloc(&order, N) && dalloc(&d_info, 1);
        if (!ok) return fail(LVK_ERR_DEVICE, "allocation failed");
        hipError_t e = hipMemcpyAsync(in_X, h_X, sizeof(double) * 3 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && h_cov9) e = hipMemcpyAsync(in_cov, h_cov9, sizeof(double) * 9 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(in_desc, h_desc, 32 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && h_score) e = hipMemcpyAsync(in_score, h_score, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        const lvk_status st = lvk_map_build(ctx, in_X, in_cov, in_desc, in_score, n, opt, order, out_X, out_cov, out_desc, nullptr, d_info);
        if (st != LVK_OK) { (void)hipStreamSynchronize(ctx->stream); release(); return st; }
        e = hipMemcpyAsync(&got, d_info, sizeof got, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        const int k = got.n_kept;
        if (k < 0 || k > n) return fail(LVK_ERR_DEVICE, "the build reported an impossible count");
        if (h_order && cap_order < k) {
            char msg[96]; snprintf(msg, sizeof msg, "room for %d indices, %d points are kept", cap_order, k);
            return fail(LVK_ERR_CAPACITY, msg);
        }
        if (k > 0) {
            const size_t K = (size_t)k;
            if (!(dalloc(&b.X, 3 * K) && (!h_cov9 || dalloc(&b.cov, 9 * K)) && dalloc(&b.desc, 32 * K) && dalloc(&b.sel, LVK_MAP_MAX_QUERIES) && dalloc(&b.info, 1)))
                return fail(LVK_ERR_DEVICE, "allocation failed");
            e = hipMemcpyAsync(b.X, out_X, sizeof(double) * 3 * K, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess && h_cov9) e = hipMemcpyAsync(b.cov, out_cov, sizeof(double) * 9 * K, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(b.desc, out_desc, 32 * K, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess && h_order) e = hipMemcpyAsync(h_order, order, sizeof(int) * K, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
            b.n = k;
        }
        release();
    }
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) { void* ptrs[] = {b.X, b.cov, b.desc, b.sel, b.info}; for (void* p : ptrs) if (p) hipFree(p); return qs; } }
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void* old[] = {fe->map.X, fe->map.cov, fe->map.desc, fe->map.sel, fe->map.info};
    for (void* p : old) if (p) hipFree(p);
    fe->map = b;
    if (info) *info = got;
    return LVK_OK;
}

// The device side of lvk_frontend_match_map, shared with lvk_frontend_localise_obs: the checks that need no argument of the caller's own,
// the matcher's buffers, a wait for the front-end's streams, lvk_map_select_queries straight into the matcher's buffers, a wait for the
// selection's count, and the chain of lvk_frontend_match_landmarks on the selected queries.  On LVK_OK the n_q selected points' records
// are in fe->map.sel and their matches in fe->match.out, queued and not waited for; *info holds the counts.  cap: the caller's room.
static lvk_status fe_match_map_device(lvk_frontend* fe, const char* who, const lvk_align_result* align, const double* R_wc, const double* p_wc, const double* cov_cam36,
                                      const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, int cap, int* n_q_out, lvk_map_info* info_out)
{
    lvk_context* ctx = fe->ctx;
    if (fe->map.n == 0) return lvk_set_error(ctx, LVK_ERR_ARG, "%s: no map is set (lvk_frontend_set_map)", who);
    const int most = fe_map_max_selected(select_opt);
    if (most >= 0 && cap < most) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "%s: room for %d records, the options can select %d", who, cap, most);
    lvk_match_options o;
    lvk_status st = fe_match_options(fe, who, match_opt, &o);
    if (st == LVK_OK) st = fe_match_buffers(fe);
    if (st != LVK_OK) return st;
    lvk_frontend::Match& m = fe->match;
    lvk_frontend::Map& mp = fe->map;
    lvk_map_camera cam;
    memset(&cam, 0, sizeof cam);
    for (int k = 0; k < 4; ++k) { cam.intr[k] = fe->cam.intr[k]; cam.dist[k] = fe->cam.dist[k]; }
    cam.model = fe->cam.model; cam.width = fe->cam.width; cam.height = fe->cam.height;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    st = lvk_map_select_queries(ctx, mp.X, mp.cov, mp.desc, mp.n, &cam, align, R_wc, p_wc, cov_cam36, select_opt, mp.sel, m.q, m.q_desc, mp.info, nullptr);
    if (st != LVK_OK) return st;
    lvk_map_info info;
    LVK_HIP(ctx, hipMemcpyAsync(&info, mp.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int n_q = info.n_selected;
    if (n_q < 0 || n_q > most) return lvk_set_error(ctx, LVK_ERR_DEVICE, "%s: the selection reported %d points", who, n_q);
    st = fe_match_chain(fe, who, o, n_q, &info.n_candidates);
    if (st != LVK_OK) return st;
    *n_q_out = n_q; *info_out = info;
    return LVK_OK;
}

// The map's points in the last processed frame: lvk_map_select_queries writes the queries and their descriptors straight into the
// matcher's buffers, the chain of lvk_frontend_match_landmarks runs on them, the host joins the two record arrays.
lvk_status lvk_frontend_match_map(lvk_frontend* fe, const lvk_align_result* align, const double* R_wc, const double* p_wc, const double* cov_cam36,
                                  const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, lvk_map_match* h_out, int cap, int* n_out,
                                  lvk_map_info* h_info)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (!R_wc || !p_wc || !h_out || !n_out || cap < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_match_map: bad argument");
    lvk_frontend::Match& m = fe->match;
    lvk_frontend::Map& mp = fe->map;
    int n_q = 0;
    lvk_map_info info;
    const lvk_status st = fe_match_map_device(fe, "lvk_frontend_match_map", align, R_wc, p_wc, cov_cam36, select_opt, match_opt, cap, &n_q, &info);
    if (st != LVK_OK) return st;
    *n_out = n_q;
    if (h_info) *h_info = info;
    if (n_q == 0) return LVK_OK;
    std::vector<lvk_map_sel> sel((size_t)n_q);
    std::vector<lvk_landmark_match> res((size_t)n_q);
    LVK_HIP(ctx, hipMemcpyAsync(sel.data(), mp.sel, sizeof(lvk_map_sel) * (size_t)n_q, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipMemcpyAsync(res.data(), m.out, sizeof(lvk_landmark_match) * (size_t)n_q, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_q; ++k) {
        lvk_map_match& r = h_out[k];
        r.index = sel[k].index; r.cell = sel[k].cell;
        r.q.x = sel[k].x; r.q.y = sel[k].y; r.q.radius = sel[k].radius; r.q.pad = 0.f;
        r.depth = sel[k].depth; r.pad = 0.f;
        r.m = res[k];
    }
    return LVK_OK;
}

// The front-end's part of lvk_vio_localise_map: the device chain of lvk_frontend_match_map, then lvk_map_gather_obs' launch on the
// selection's and the matcher's records where they lie (no joined copy is made), then ONE copy back of the counts, the source rows and
// the observations, laid out for this frame's n_selected: [lvk_map_obs_info | int idx[n_q], padded to 8 bytes | lvk_landmark_obs obs[n_q]].
// sigma = sigma_px / ((fx + fy) / 2), as larvio_amd.localize.map_obs defines it.
#define FE_LOC_BLOB (sizeof(lvk_map_obs_info) + sizeof(int) * LVK_MAP_MAX_QUERIES + sizeof(lvk_landmark_obs) * LVK_MAP_MAX_QUERIES)
lvk_status lvk_frontend_localise_obs(lvk_frontend* fe, const lvk_align_result* align, const double* R_wc, const double* p_wc, const double* cov_cam36,
                                     const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, double sigma_px,
                                     lvk_landmark_obs* h_obs, int* h_idx, lvk_map_info* h_info, lvk_map_obs_info* h_oinfo)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (!R_wc || !p_wc || !h_obs || !h_idx || !h_info || !h_oinfo) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_vio_localise_map: bad argument");
    if (!std::isfinite(sigma_px) || !(sigma_px > 0.)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_vio_localise_map: sigma_px is not a finite number > 0");
    if (!fe->loc.blob && fe->map.n > 0) {
        if (hipMalloc((void**)&fe->loc.blob, FE_LOC_BLOB) != hipSuccess) { (void)hipGetLastError(); fe->loc.blob = nullptr; return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_vio_localise_map: allocation failed"); }
    }
    int n_q = 0;
    lvk_status st = fe_match_map_device(fe, "lvk_vio_localise_map", align, R_wc, p_wc, cov_cam36, select_opt, match_opt, LVK_MAP_MAX_QUERIES, &n_q, h_info);
    if (st != LVK_OK) return st;
    memset(h_oinfo, 0, sizeof *h_oinfo);
    if (n_q == 0) return LVK_OK;
    const size_t o_idx = sizeof(lvk_map_obs_info), o_obs = o_idx + ((sizeof(int) * (size_t)n_q + 7) & ~(size_t)7), bytes = o_obs + sizeof(lvk_landmark_obs) * (size_t)n_q;
    char* blob = fe->loc.blob;
    const double sigma = sigma_px / ((fe->cam.intr[0] + fe->cam.intr[1]) / 2);
    st = fe_map_gather_launch(ctx, &fe->map.sel->index, (int)sizeof(lvk_map_sel), fe->match.out, (int)sizeof(lvk_landmark_match), n_q, fe->map.X, fe->map.cov, fe->map.n, align,
                              sigma, (lvk_landmark_obs*)(blob + o_obs), (int*)(blob + o_idx), (lvk_map_obs_info*)blob);
    if (st != LVK_OK) return st;
    std::vector<char> got(bytes);
    LVK_HIP(ctx, hipMemcpyAsync(got.data(), blob, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(h_oinfo, got.data(), sizeof *h_oinfo);
    const int n_ok = h_oinfo->n_ok;
    if (n_ok < 0 || n_ok > n_q) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_vio_localise_map: the gather reported %d observations of %d records", n_ok, n_q);
    memcpy(h_idx, got.data() + o_idx, sizeof(int) * (size_t)n_ok);
    memcpy(h_obs, got.data() + o_obs, sizeof(lvk_landmark_obs) * (size_t)n_ok);
    return LVK_OK;
}

// The yaw and translation of a prior map from its matches in the last processed frame (no reference counterpart): the pairs are drawn
// on the host, the matches and pairs go up, lvk_align_ransac_2pt runs on the main stream in buffers the call owns, the result and the
// mask come back.  Nothing a frame reads or writes is touched.
#define FE_ALIGN_MAX_N     1024
#define FE_ALIGN_MAX_PAIRS 4096
// the alignment's buffers, allocated by the first call that needs them
static lvk_status fe_align_buffers(lvk_frontend* fe)
{
    if (fe->align.m) return LVK_OK;
    lvk_frontend::Align b = {};
    if (!(dalloc(&b.m, FE_ALIGN_MAX_N) && dalloc(&b.pairs, FE_ALIGN_MAX_PAIRS) && dalloc(&b.mask, FE_ALIGN_MAX_N) && dalloc(&b.out, 1))) {
        (void)hipGetLastError();
        void* ptrs[] = {b.m, b.pairs, b.mask, b.out};
        for (void* p : ptrs) if (p) hipFree(p);
        return lvk_set_error(fe->ctx, LVK_ERR_DEVICE, "lvk_frontend_align_landmarks: allocation failed");
    }
    fe->align = b;
    return LVK_OK;
}
lvk_status lvk_frontend_align_landmarks(lvk_frontend* fe, const lvk_align_match* h_m, int n, const double* R_wc, const double* p_wc, const lvk_align_options* opt,
                                        int max_hypotheses, uint32_t seed, lvk_align_result* h_out, uint8_t* h_mask)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (n < 0 || max_hypotheses < 0 || !R_wc || !p_wc || !h_out || (n > 0 && !h_m)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_align_landmarks: bad argument");
    if (n > FE_ALIGN_MAX_N) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_align_landmarks: %d matches, at most %d", n, FE_ALIGN_MAX_N);
    if (max_hypotheses > FE_ALIGN_MAX_PAIRS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_align_landmarks: max_hypotheses %d, at most %d", max_hypotheses, FE_ALIGN_MAX_PAIRS);
    if (fe->n_img == 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_align_landmarks: no frame has been processed yet");
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_align_landmarks: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    { lvk_status as = fe_align_buffers(fe); if (as != LVK_OK) return as; }
    lvk_frontend::Align& a = fe->align;
    std::vector<lvk_align_pair> pairs(FE_ALIGN_MAX_PAIRS);
    const int n_pairs = lvk_align_draw_pairs(n, max_hypotheses, seed, pairs.data());
    if (n_pairs < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_align_landmarks: the pairs could not be drawn");
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    if (n > 0) LVK_HIP(ctx, hipMemcpyAsync(a.m, h_m, sizeof(lvk_align_match) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (n_pairs > 0) LVK_HIP(ctx, hipMemcpyAsync(a.pairs, pairs.data(), sizeof(lvk_align_pair) * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
    const lvk_status st = lvk_align_ransac_2pt(ctx, a.m, n, a.pairs, n_pairs, R_wc, p_wc, opt, nullptr, a.mask, a.out);
    if (st != LVK_OK) { (void)hipStreamSynchronize(ctx->stream); return st; }      // (the uploads read this call's own vector)
    LVK_HIP(ctx, hipMemcpyAsync(h_out, a.out, sizeof(lvk_align_result), hipMemcpyDeviceToHost, ctx->stream));
    if (h_mask && n > 0) LVK_HIP(ctx, hipMemcpyAsync(h_mask, a.mask, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LVK_OK;
}

// The map's yaw and translation from the last processed frame in one call (no reference counterpart): the frame's corners and descriptors
// as the matcher detects them, lvk_orb_match_global of the resident map against them, the pairs drawn on the host for n_selected, the
// alignment's records gathered on the device, lvk_align_ransac_2pt, one copy back.  Buffers: the matcher's corner buffers, the alignment's,
// and fe->reloc; nothing a frame reads or writes is touched.
lvk_status lvk_frontend_relocalise_map(lvk_frontend* fe, const double* R_wc, const double* p_wc, const lvk_match_options* match_opt, const lvk_align_options* align_opt,
                                       int max_matches, int max_hypotheses, uint32_t seed, lvk_align_result* h_out, lvk_reloc_match* h_matches, int cap, int* n_out,
                                       lvk_global_info* h_info)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (!R_wc || !p_wc || !h_out || !h_matches || !n_out || cap < 0 || max_matches < 0 || max_hypotheses < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_relocalise_map: bad argument");
    if (fe->map.n == 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_relocalise_map: no map is set (lvk_frontend_set_map)");
    if (max_matches == 0) max_matches = FE_ALIGN_MAX_N;
    if (max_matches > FE_ALIGN_MAX_N) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_relocalise_map: max_matches %d outside 0..%d", max_matches, FE_ALIGN_MAX_N);   // (as the stage entry refuses it)
    if (cap < max_matches) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_relocalise_map: room for %d records, max_matches is %d", cap, max_matches);
    if (max_hypotheses > FE_ALIGN_MAX_PAIRS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_relocalise_map: max_hypotheses %d, at most %d", max_hypotheses, FE_ALIGN_MAX_PAIRS);
    lvk_match_options o;
    lvk_status st = fe_match_options(fe, "lvk_frontend_relocalise_map", match_opt, &o);
    if (st == LVK_OK) st = fe_match_buffers(fe);
    if (st == LVK_OK) st = fe_align_buffers(fe);
    if (st != LVK_OK) return st;
    lvk_frontend::Reloc& r = fe->reloc;
    if (!r.best) {
        lvk_frontend::Reloc b = {};
        if (!(dalloc(&b.best, FE_MATCH_MAX_CAND) && dalloc(&b.sel, FE_ALIGN_MAX_N) && dalloc(&b.px, FE_ALIGN_MAX_N) && dalloc(&b.und, FE_ALIGN_MAX_N) && dalloc(&b.blob, 1))) {
            (void)hipGetLastError();
            void* ptrs[] = {b.best, b.sel, b.px, b.und, b.blob};
            for (void* p : ptrs) if (p) hipFree(p);
            return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_relocalise_map: allocation failed");
        }
        r = b;
    }
    lvk_frontend::Match& m = fe->match;
    lvk_frontend::Align& a = fe->align;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    int n_cand = 0;
    st = fe_match_corners(fe, "lvk_frontend_relocalise_map", o, true, &n_cand);
    if (st != LVK_OK) return st;
    lvk_global_info info;
    memset(&info, 0, sizeof info);
    if (n_cand > 0) {
        st = lvk_orb_match_global(ctx, fe->map.desc, fe->map.n, m.cand_desc, n_cand, o.max_dist, o.ratio_pct, max_matches, r.best, r.sel, &r.blob->info);
        if (st != LVK_OK) return st;
        LVK_HIP(ctx, hipMemcpyAsync(&info, &r.blob->info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
        LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else
        LVK_HIP(ctx, hipMemsetAsync(&r.blob->info, 0, sizeof info, ctx->stream));      // (a frame without a corner: the search launches nothing)
    const int n = info.n_selected;
    if (n < 0 || n > max_matches) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_relocalise_map: the search reported %d matches", n);
    std::vector<lvk_align_pair> pairs(FE_ALIGN_MAX_PAIRS);
    const int n_pairs = lvk_align_draw_pairs(n, max_hypotheses, seed, pairs.data());
    if (n_pairs < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_relocalise_map: the pairs could not be drawn");
    if (n_pairs > 0) LVK_HIP(ctx, hipMemcpyAsync(a.pairs, pairs.data(), sizeof(lvk_align_pair) * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
    st = fe_reloc_gather(ctx, fe->cam, r.sel, n, m.cand_pts, fe->map.X, r.px, r.und, a.m, r.blob->m);
    if (st == LVK_OK) st = lvk_align_ransac_2pt(ctx, a.m, n, a.pairs, n_pairs, R_wc, p_wc, align_opt, nullptr, a.mask, &r.blob->res);
    if (st == LVK_OK) st = fe_reloc_inliers(ctx, a.mask, n, r.blob->m);
    if (st != LVK_OK) { (void)hipStreamSynchronize(ctx->stream); return st; }      // (the upload reads this call's own vector)
    const size_t head = offsetof(lvk_frontend::RelocBlob, m);
    std::vector<uint8_t> back(head + sizeof(lvk_reloc_match) * (size_t)n);
    LVK_HIP(ctx, hipMemcpyAsync(back.data(), r.blob, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(h_out, back.data() + offsetof(lvk_frontend::RelocBlob, res), sizeof *h_out);
    if (h_info) memcpy(h_info, back.data() + offsetof(lvk_frontend::RelocBlob, info), sizeof *h_info);
    if (n > 0) memcpy(h_matches, back.data() + head, sizeof(lvk_reloc_match) * (size_t)n);
    *n_out = n;
    return LVK_OK;
}

// A second session into the map in force (no reference counterpart): B is uploaded and built on its own, aligned to the resident map (a given
// alignment, or lvk_orb_match_global of the sorted B against the resident descriptors and lvk_align_ransac_3d), transformed behind a copy of
// the resident arrays, and the concatenation is built and installed as lvk_frontend_build_map installs its result.  The buffers sized by
// the maps live for the call; fe->merge keeps the small ones.  A refusal, and an alignment that is not found, leave the map in force.
lvk_status lvk_frontend_merge_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, int n, const lvk_align_result* align,
                                  const double* cov_align16, const lvk_match_options* match_opt, const lvk_align3d_options* align_opt, int max_hypotheses, uint32_t seed,
                                  const lvk_map_build_options* build_opt, lvk_align_result* h_align_out, int* h_order, int cap_order, lvk_map_build_info* info,
                                  lvk_global_info* h_match_info)
{
    if (!fe) return LVK_ERR_ARG;
    lvk_context* ctx = fe->ctx;
    { lvk_status fs = fe_check_failed(fe); if (fs != LVK_OK) return fs; }
    if (n < 0 || cap_order < 0 || max_hypotheses < 0 || !h_align_out || (n > 0 && (!h_X || !h_cov9 || !h_desc))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: bad argument");
    if (fe->map.n == 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: no map is set (lvk_frontend_set_map)");
    if (!fe->map.cov) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: the resident map has no covariances (they are the score of the merge)");
    // what the stage entries would refuse is refused here, before anything is uploaded or launched; the search's options are read only
    // when the search runs
    int max_dist = match_opt ? match_opt->max_dist : 0, ratio_pct = match_opt ? match_opt->ratio_pct : 0;
    if (max_dist == 0) max_dist = 58;
    if (ratio_pct == 0) ratio_pct = 100;
    if (!align && (max_dist < 0 || max_dist > 256)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: max_dist %d outside 0..256", max_dist);
    if (!align && (ratio_pct < 1 || ratio_pct > 100)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: ratio_pct %d outside 0..100", ratio_pct);
    if (align && !(std::isfinite(align->c) && std::isfinite(align->s) && std::isfinite(align->t[0]) && std::isfinite(align->t[1]) && std::isfinite(align->t[2])))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: the alignment is not finite");
    if (cov_align16)
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(cov_align16[k])) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: cov_align16 is not finite");
    const char* why = "";
    if (!fe_map_build_options_ok(build_opt, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: %s", why);
    if (!fe_align3d_options_ok(align_opt, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: %s", why);
    if (max_hypotheses > FE_ALIGN_MAX_PAIRS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_merge_map: max_hypotheses %d, at most %d", max_hypotheses, FE_ALIGN_MAX_PAIRS);
    const int n_a = fe->map.n;
    if ((long long)n_a + n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_frontend_merge_map: %d resident and %d new points, at most %d together", n_a, n, LVK_MAP_MAX_POINTS);
    if (fe->image_done)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_frontend_merge_map: the image stage of t = %.6f is still waiting for its lvk_frontend_process", fe->image_done_ts);
    lvk_frontend::Merge& mg = fe->merge;
    if (!mg.best) {
        lvk_frontend::Merge b = {};
        if (!(dalloc(&b.best, 4096) && dalloc(&b.sel, FE_ALIGN_MAX_N) && dalloc(&b.ginfo, 1) && dalloc(&b.m, FE_ALIGN_MAX_N) && dalloc(&b.pairs, FE_ALIGN_MAX_PAIRS) &&
              dalloc(&b.mask, FE_ALIGN_MAX_N) && dalloc(&b.res, 1))) {
            (void)hipGetLastError();
            void* ptrs[] = {b.best, b.sel, b.ginfo, b.m, b.pairs, b.mask, b.res};
            for (void* p : ptrs) if (p) hipFree(p);
            return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_frontend_merge_map: allocation failed");
        }
        mg = b;
    }
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    // the call's own buffers: B as uploaded, B sorted, its order; then the concatenation, its build and that build's order
    double *in_X = nullptr, *in_cov = nullptr, *sb_X = nullptr, *sb_cov = nullptr, *cat_X = nullptr, *cat_cov = nullptr, *out_X = nullptr, *out_cov = nullptr;
    uint8_t *in_desc = nullptr, *sb_desc = nullptr, *cat_desc = nullptr, *out_desc = nullptr;
    int *order_b = nullptr, *order_m = nullptr; lvk_map_build_info* d_info = nullptr;
    lvk_frontend::Map b = {};
    auto release = [&]() {
        void* ptrs[] = {in_X, in_cov, sb_X, sb_cov, cat_X, cat_cov, out_X, out_cov, in_desc, sb_desc, cat_desc, out_desc, order_b, order_m, d_info};
        for (void* p : ptrs) if (p) hipFree(p);
    };
    auto fail = [&](lvk_status code, const char* what) {
        (void)hipStreamSynchronize(ctx->stream);         // (the uploads read the caller's arrays)
        (void)hipGetLastError();
        release();
        void* ptrs[] = {b.X, b.cov, b.desc, b.sel, b.info};
        for (void* p : ptrs) if (p) hipFree(p);
        return lvk_set_error(ctx, code, "lvk_frontend_merge_map: %s", what);
    };
    auto pass = [&](lvk_status st) {                     // a stage entry's refusal: its own message stands
        (void)hipStreamSynchronize(ctx->stream);
        release();
        void* ptrs[] = {b.X, b.cov, b.desc, b.sel, b.info};
        for (void* p : ptrs) if (p) hipFree(p);
        return st;
    };
    lvk_map_build_info got_b, got;
    memset(&got_b, 0, sizeof got_b); memset(&got, 0, sizeof got);
    lvk_global_info ginfo;
    memset(&ginfo, 0, sizeof ginfo);
    hipError_t e = hipSuccess;
    if (!dalloc(&d_info, 1)) return fail(LVK_ERR_DEVICE, "allocation failed");
    // ---- 1: B alone
    if (n > 0) {
        const size_t N = (size_t)n;
        if (!(dalloc(&in_X, 3 * N) && dalloc(&in_cov, 9 * N) && dalloc(&in_desc, 32 * N) && dalloc(&sb_X, 3 * N) && dalloc(&sb_cov, 9 * N) && dalloc(&sb_desc, 32 * N) && dalloc(&order_b, N)))
            return fail(LVK_ERR_DEVICE, "allocation failed");
        e = hipMemcpyAsync(in_X, h_X, sizeof(double) * 3 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(in_cov, h_cov9, sizeof(double) * 9 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(in_desc, h_desc, 32 * N, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        const lvk_status st = lvk_map_build(ctx, in_X, in_cov, in_desc, nullptr, n, build_opt, order_b, sb_X, sb_cov, sb_desc, nullptr, d_info);
        if (st != LVK_OK) return pass(st);
        e = hipMemcpyAsync(&got_b, d_info, sizeof got_b, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        if (got_b.n_kept < 0 || got_b.n_kept > n) return fail(LVK_ERR_DEVICE, "the build of the new session reported an impossible count");
    }
    const int k_b = got_b.n_kept;
    // ---- 2: the alignment
    lvk_align_result al;
    if (align) al = *align;
    else {
        const int n_q = k_b < 4096 ? k_b : 4096;
        if (n_q > 0) {
            const lvk_status st = lvk_orb_match_global(ctx, fe->map.desc, n_a, sb_desc, n_q, max_dist, ratio_pct, FE_ALIGN_MAX_N, mg.best, mg.sel, mg.ginfo);
            if (st != LVK_OK) return pass(st);
            e = hipMemcpyAsync(&ginfo, mg.ginfo, sizeof ginfo, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        }
        const int n_sel = ginfo.n_selected;
        if (n_sel < 0 || n_sel > FE_ALIGN_MAX_N) return fail(LVK_ERR_DEVICE, "the search reported an impossible count");
        std::vector<lvk_align_pair> pairs(FE_ALIGN_MAX_PAIRS);
        const int n_pairs = lvk_align_draw_pairs(n_sel, max_hypotheses, seed, pairs.data());
        if (n_pairs < 0) return fail(LVK_ERR_ARG, "the pairs could not be drawn");
        if (n_pairs > 0) e = hipMemcpyAsync(mg.pairs, pairs.data(), sizeof(lvk_align_pair) * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        lvk_status st = fe_merge_gather(ctx, mg.sel, n_sel, sb_X, n_q, fe->map.X, n_a, mg.m);
        if (st == LVK_OK) st = lvk_align_ransac_3d(ctx, mg.m, n_sel, mg.pairs, n_pairs, align_opt, nullptr, mg.mask, mg.res);
        if (st != LVK_OK) return pass(st);
        e = hipMemcpyAsync(&al, mg.res, sizeof al, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // (the upload read this call's own vector)
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        if (al.status != LVK_ALIGN_OK) {                 // an answer, not an error: the map in force stays
            release();
            *h_align_out = al;
            if (info) memset(info, 0, sizeof *info);
            if (h_match_info) *h_match_info = ginfo;
            return LVK_OK;
        }
    }
    // ---- 3: [A | the sorted B in A's frame]
    const int n_cat = n_a + k_b;
    const size_t NA = (size_t)n_a, NC = (size_t)n_cat;
    if (!(dalloc(&cat_X, 3 * NC) && dalloc(&cat_cov, 9 * NC) && dalloc(&cat_desc, 32 * NC) && dalloc(&out_X, 3 * NC) && dalloc(&out_cov, 9 * NC) && dalloc(&out_desc, 32 * NC) &&
          dalloc(&order_m, NC)))
        return fail(LVK_ERR_DEVICE, "allocation failed");
    e = hipMemcpyAsync(cat_X, fe->map.X, sizeof(double) * 3 * NA, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cat_cov, fe->map.cov, sizeof(double) * 9 * NA, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cat_desc, fe->map.desc, 32 * NA, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
    {
        lvk_status st = lvk_map_transform(ctx, sb_X, sb_cov, sb_desc, k_b, &al, cov_align16, cat_X + 3 * NA, cat_cov + 9 * NA, cat_desc + 32 * NA);
        // ---- 4: the merged map
        if (st == LVK_OK) st = lvk_map_build(ctx, cat_X, cat_cov, cat_desc, nullptr, n_cat, build_opt, order_m, out_X, out_cov, out_desc, nullptr, d_info);
        if (st != LVK_OK) return pass(st);
    }
    e = hipMemcpyAsync(&got, d_info, sizeof got, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
    const int k = got.n_kept;
    if (k < 0 || k > n_cat) return fail(LVK_ERR_DEVICE, "the build reported an impossible count");
    if (h_order && cap_order < k) {
        char msg[96]; snprintf(msg, sizeof msg, "room for %d indices, %d points are kept", cap_order, k);
        return fail(LVK_ERR_CAPACITY, msg);
    }
    // ---- 5, 6: the map's own buffers at their final size, and the order in the caller's view
    std::vector<int> ord_m, ord_b;
    if (k > 0) {
        const size_t K = (size_t)k;
        if (!(dalloc(&b.X, 3 * K) && dalloc(&b.cov, 9 * K) && dalloc(&b.desc, 32 * K) && dalloc(&b.sel, LVK_MAP_MAX_QUERIES) && dalloc(&b.info, 1))) return fail(LVK_ERR_DEVICE, "allocation failed");
        e = hipMemcpyAsync(b.X, out_X, sizeof(double) * 3 * K, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.cov, out_cov, sizeof(double) * 9 * K, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b.desc, out_desc, 32 * K, hipMemcpyDeviceToDevice, ctx->stream);
        if (h_order) {
            ord_m.resize(K); ord_b.resize(k_b > 0 ? (size_t)k_b : 1);
            if (e == hipSuccess) e = hipMemcpyAsync(ord_m.data(), order_m, sizeof(int) * K, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && k_b > 0) e = hipMemcpyAsync(ord_b.data(), order_b, sizeof(int) * (size_t)k_b, hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(LVK_ERR_DEVICE, hipGetErrorString(e));
        if (h_order)
            for (int p = 0; p < k; ++p) {
                const int o = ord_m[(size_t)p];
                if (o < 0 || o >= n_cat) return fail(LVK_ERR_DEVICE, "the build reported an impossible index");
                h_order[p] = o < n_a ? o : n_a + ord_b[(size_t)(o - n_a)];
            }
        b.n = k;
    }
    release();
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void* old[] = {fe->map.X, fe->map.cov, fe->map.desc, fe->map.sel, fe->map.info};
    for (void* p : old) if (p) hipFree(p);
    fe->map = b;
    *h_align_out = al;
    if (info) *info = got;
    if (h_match_info) *h_match_info = ginfo;
    return LVK_OK;
}

lvk_status lvk_frontend_profile_enable(lvk_frontend* fe, unsigned stage_mask)
{
    if (!fe) return LVK_ERR_ARG;
    prof_collect(fe);
    fe->prof_mask = stage_mask & 0xFFFFu; fe->prof_stride = (stage_mask >> 16) & 0xFFu; fe->prof_take = true;
    return LVK_OK;
}
lvk_status lvk_frontend_profile_read(lvk_frontend* fe, double ms_sum[LVK_FE_STAGES], uint64_t launches[LVK_FE_STAGES], int reset)
{
    if (!fe) return LVK_ERR_ARG;
    prof_collect(fe);
    for (int i = 0; i < LVK_FE_STAGES; ++i) {
        if (ms_sum) ms_sum[i] = fe->prof_ms[i];
        if (launches) launches[i] = fe->prof_n[i];
        if (reset) { fe->prof_ms[i] = 0.; fe->prof_n[i] = 0; }
    }
    return LVK_OK;
}
const char* lvk_frontend_stage_name(int stage)
{
    static const char* names[LVK_FE_STAGES] = {"pyramid_clahe", "orb_prepare", "lk_fwd_rev", "(unused)", "orb_gate", "ransac_commit", "min_eigen", "gftt_select", "feature_msg"};
    return stage >= 0 && stage < LVK_FE_STAGES ? names[stage] : "?";
}

lvk_status lvk_frontend_lk_stats(lvk_frontend* fe, uint64_t* point_levels, uint64_t* iterations)
{
    if (!fe) return LVK_ERR_ARG;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    lvk_status st = fe_read_dev(fe);
    if (st != LVK_OK) return st;
    if (point_levels) *point_levels = fe->h_dev->lk_point_levels;
    if (iterations) *iterations = fe->h_dev->lk_iterations;
    return LVK_OK;
}

lvk_status lvk_frontend_msg_stats(lvk_frontend* fe, uint64_t* messages, uint64_t* features)
{
    if (!fe) return LVK_ERR_ARG;
    { lvk_status qs = fe_quiesce(fe); if (qs != LVK_OK) return qs; }
    lvk_status st = fe_read_dev(fe);
    if (st != LVK_OK) return st;
    if (messages) *messages = fe->h_dev->msg_count;
    if (features) *features = fe->h_dev->msg_features;
    return LVK_OK;
}

}  // extern "C"
