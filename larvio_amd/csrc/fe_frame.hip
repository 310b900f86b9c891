// fe_frame.hip — the kernels of a steady-state frame and their launchers: LK forward + reverse with the ORB descriptor gate in their
// shadow (k_fe_lk_both, k_fe_lk_pipe), RANSAC + commit of a track set (k_fe_ransac_commit), the feature message (k_fe_msg).
// frontend.hip decides what a frame queues and on which stream; the launches themselves are here, next to the kernels (fe_frontend.h).
#include "lvk_internal.h"
#include "fe_track_dev.h"
#include "fe_frontend.h"
#include <math.h>

__device__ __forceinline__ lvk_pt2f apply_h(const HMat& H, lvk_pt2f p)
{   // predictFeatureTracking (:285-290): Matx33f * Vec3f, s = 0; s += H(i,k)*p(k)
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { float s = 0.f; s += H.h[r * 3] * p.x; s += H.h[r * 3 + 1] * p.y; s += H.h[r * 3 + 2] * 1.0f; q[r] = s; }
    lvk_pt2f o; o.x = q[0] / q[2]; o.y = q[1] / q[2];
    return o;
}

// ---- what the two frame kernels below share; none of these pieces contains a block barrier
// per-block spans (-DLVK_LK_TIMING, tools/gpu/lk_ticks.py); an empty object in every other build
#ifdef LVK_LK_TIMING
static __device__ unsigned long long g_lk_span[4096][4];     // per block: cycles entry -> forward done, -> reverse done, -> end; 100 MHz ticks entry -> end
struct LkSpan {
    unsigned long long c0, w0, c1 = 0, c2 = 0;
    __device__ __forceinline__ LkSpan() : c0(clock64()), w0(wall_clock64()) { }
    __device__ __forceinline__ void fwd_done() { c1 = clock64(); }
    __device__ __forceinline__ void rev_done() { c2 = clock64(); }
    __device__ __forceinline__ void write(int p) const
    {
        if (p < 4096) { g_lk_span[p][0] = c1 - c0; g_lk_span[p][1] = c2 - c0; g_lk_span[p][2] = clock64() - c0; g_lk_span[p][3] = wall_clock64() - w0; }
    }
};
#else
struct LkSpan {
    __device__ __forceinline__ void fwd_done() { }
    __device__ __forceinline__ void rev_done() { }
    __device__ __forceinline__ void write(int) const { }
};
#endif
// -DLVK_LK_BOUNDS: is a point handed to the LK / ORB wavefronts inside the image?  The first one that is not is recorded by `reporter`
// (one thread of the callers) as site 5 (the source point) or 6 (the forward result).  Always true in every other build.
__device__ __forceinline__ bool fe_lk_point_ok(lvk_pt2f pt, int width, int height, bool reporter, int site, int n, int p, int is_new)
{
#ifdef LVK_LK_BOUNDS
    if (!(pt.x >= 0 && pt.x <= width - 1 && pt.y >= 0 && pt.y <= height - 1)) {
        if (reporter && atomicAdd(&g_lk_oob[0], 1) == 0) { g_lk_oob[1] = site; g_lk_oob[2] = n; g_lk_oob[3] = p; g_lk_oob[4] = is_new; g_lk_oob[7] = __builtin_bit_cast(int, pt.x); g_lk_oob[8] = __builtin_bit_cast(int, pt.y); g_lk_oob[9] = blockIdx.x; }
        return false;
    }
#endif
    return true;
}
__device__ __forceinline__ bool fe_outside_image(lvk_pt2f p, int width, int height) { return p.y < 0 || p.y > height - 1 || p.x < 0 || p.x > width - 1; }
// the LK wavefront after the forward pass: the in-image test, then the point and the verdict for the block
__device__ __forceinline__ void fe_lk_forward_done(lvk_pt2f np, int& st, int width, int height, lvk_pt2f& s_np, int& s_st)
{
    if (st && fe_outside_image(np, width, height)) st = 0;
    if ((threadIdx.x & 63) == 0) { s_np = np; s_st = st; }
}
// the LK wavefront after the reverse pass: the status code of a point that came back at `back` (:616-642)
__device__ __forceinline__ int fe_lk_round_trip(lvk_pt2f pp, lvk_pt2f back, int sr, int width, int height)
{
    if (sr) {
        if (fe_outside_image(back, width, height)) sr = 0;
        else {
            float dx = back.x - pp.x, dy = back.y - pp.y;
            float dis = (float)sqrt((double)dx * dx + (double)dy * dy);      // cv::norm(Point2f) is double
            if (dis > 1) sr = 0;
        }
    }
    return sr ? ST_ALIVE : ST_REV;
}
// the descriptor / undistortion wavefront, during the forward pass: the previous-image descriptor of a new point (kept in dp and
// written out), the undistorted source point
__device__ __forceinline__ void fe_desc_before(const uint8_t* __restrict__ prv_ext, const uint8_t* __restrict__ prv_blur, int step, lvk_pt2f pp, int p, int is_new,
                                               unsigned long long (&dp)[4], unsigned long long* __restrict__ w_desc, const CamParams& cam, lvk_pt2f* __restrict__ w_und)
{
    const int lane = threadIdx.x & 63;
    if (is_new) {
        orb_point(prv_ext, prv_blur, step, pp, dp);
        if (lane == 0) { unsigned long long* o = w_desc + (size_t)p * 4; o[0] = dp[0]; o[1] = dp[1]; o[2] = dp[2]; o[3] = dp[3]; }
    }
    if (lane == 0) w_und[2 * (size_t)p] = undistort_point(pp, cam, cam.intr);
}
// ... and once the forward pass has produced the point np (in_plane: fe_lk_point_ok of it): the current-image descriptor, its distance to
// the previous-image one (new points) or the stored first-seen one (old tracks) for the block, the undistorted np
__device__ __forceinline__ void fe_desc_after(const uint8_t* __restrict__ cur_ext, const uint8_t* __restrict__ cur_blur, int step, lvk_pt2f np, bool in_plane, int p, int is_new,
                                              const unsigned long long (&dp)[4], const unsigned long long* __restrict__ stored_desc, const CamParams& cam,
                                              lvk_pt2f* __restrict__ w_und, int& s_dist)
{
    unsigned long long dc[4];
    if (in_plane) orb_point(cur_ext, cur_blur, step, np, dc);
    const int dist = is_new ? hamming256_u64(dc, dp) : hamming256_u64(dc, stored_desc + (size_t)p * 4);
    if ((threadIdx.x & 63) == 0) { s_dist = dist; w_und[2 * (size_t)p + 1] = undistort_point(np, cam, cam.intr); }
}
// one thread, after the last barrier: the descriptor gate (:677-699 / :909-930), then point, status code, counters and span
__device__ __forceinline__ void fe_lk_finish(int p, lvk_pt2f np, int code, const int& s_dist, int passes, int n_levels, int its,
                                             lvk_pt2f* __restrict__ w_curr, uint8_t* __restrict__ w_status, FeDev* __restrict__ dev, const LkSpan& span, bool span_on)
{
    if (code == ST_ALIVE && s_dist > 58) code = ST_ORB;
    w_curr[p] = np; w_status[p] = (uint8_t)code;
    atomicAdd(&dev->lk_point_levels, (unsigned long long)(passes * n_levels));
    atomicAdd(&dev->lk_iterations, (unsigned long long)its);
    if (span_on) span.write(p);
}

// Forward LK (prev -> curr, seeded with the gyro-predicted point, :558-590 / :830-860), reverse LK (curr -> prev, seeded with the
// original point; in-image and <= 1 px tests, :616-642) and the ORB descriptor gate (:677-699 old tracks: descriptor at the current
// point vs the stored first-seen one; :909-930 new points: descriptor in the previous image vs in the current one, the previous one is
// kept) of a point in ONE launch, TWO wavefronts per point: wavefront 0 runs the two LK passes back to back; wavefront 1 computes the
// descriptors in their shadow - the previous-image one (new points) during the forward pass, the current-image one as soon as the
// forward pass has produced the point, i.e. while the reverse pass runs.  The gate's launch (13 us + its barrier) leaves the frame's
// dependent chain altogether; a descriptor computed for a point that then fails the reverse check is simply not used.  The same
// wavefront also undistorts the point pair (K -> K, what findFundamentalMat is fed, :701-712 / :932-943) into w_und[2p], [2p+1]:
// two sequential double-precision fixed-point loops per point that the one-workgroup commit kernel would otherwise run for
// every point of its set (24 us of its 120 at 2000 tracks).
template <int WIN>
__global__ void __launch_bounds__(128) k_fe_lk_both(PyrView prev, PyrView next, const lvk_pt2f* __restrict__ src_pts, const int* __restrict__ n_ptr,
                                                   HMat H, int width, int height, int max_count, double epsilon,
                                                   lvk_pt2f* __restrict__ w_curr, uint8_t* __restrict__ w_status, FeDev* __restrict__ dev,
                                                   const uint8_t* __restrict__ cur_ext, const uint8_t* __restrict__ cur_blur,
                                                   const uint8_t* __restrict__ prv_ext, const uint8_t* __restrict__ prv_blur,
                                                   const unsigned long long* __restrict__ stored_desc /*old*/, unsigned long long* __restrict__ w_desc /*new: out*/, int is_new,
                                                   CamParams cam, lvk_pt2f* __restrict__ w_und)
{
    __shared__ lvk_pt2f s_np;
    __shared__ int s_st, s_dist;
    __shared__ __attribute__((aligned(16))) unsigned long long s_acc[4];
    const int p = blockIdx.x;
    LkSpan span;
    if (p >= *n_ptr) return;
    const int wave = threadIdx.x >> 6;
    const int n_levels = prev.n_levels < next.n_levels ? prev.n_levels : next.n_levels;
    const int step = width + 2 * LVK_ORB_BORDER;
    const lvk_pt2f pp = src_pts[p];
    lvk_pt2f np = pp;
    int st = 1, its = 0;
    unsigned long long dp[4] = {0, 0, 0, 0};
    LkLdsAcc acc; acc.off = 0; acc.prev[0] = acc.prev[1] = acc.prev[2] = 0;
    if (wave == 0) {
        acc = lk_acc_init(s_acc);
        np = apply_h(H, pp);
        its = lk_point<WIN>(prev, next, n_levels, pp, np, st, max_count, epsilon, nullptr, acc);
        fe_lk_forward_done(np, st, width, height, s_np, s_st);
        span.fwd_done();
    } else fe_desc_before(prv_ext, prv_blur, step, pp, p, is_new, dp, w_desc, cam, w_und);
    __syncthreads();
    int code = ST_FWD, passes = 1;
    if (wave == 0) {
        if (st) {
            lvk_pt2f back = pp;
            int sr = 1;
            its += lk_point<WIN, 1>(next, prev, n_levels, np, back, sr, max_count, epsilon, nullptr, acc);
            passes = 2;
            code = fe_lk_round_trip(pp, back, sr, width, height);
        }
        span.rev_done();
    } else if (s_st) {
        const lvk_pt2f fnp = s_np;
        fe_desc_after(cur_ext, cur_blur, step, fnp, fe_lk_point_ok(fnp, width, height, (threadIdx.x & 63) == 0, 6, *n_ptr, p, is_new), p, is_new, dp, stored_desc, cam, w_und, s_dist);
    }
    __syncthreads();
    if (threadIdx.x == 0) fe_lk_finish(p, np, code, s_dist, passes, n_levels, its, w_curr, w_status, dev, span, true);
}

// The same stages with the track's work spread over FIVE wavefronts (lk_tpl_build21 + lk_pass_iterate21, fe_track_dev.h): wavefront 0 owns the
// track and only iterates; wavefronts 1-3 build the levels' templates of a pass at once (level w - 1, w + 2, ...) before it starts - forward: from
// the point in the previous image, known at launch; reverse: from the forward result - and wavefront 4 is the descriptor / undistortion
// wavefront of k_fe_lk_both.  Four block barriers, every wavefront passes each of them.
// One track set of a launch: the old tracks (trackFeatures) or the new points (trackNewFeatures).  The kernel can carry BOTH in one launch
// (blocks [0, grid0) the first set, the rest the second; LVK_LK_MERGED=1): the two chains are normally two launches on two streams joined
// by an event between the commits - a barrier packet of ~7 us on every frame's dependent chain (profiles/r6_final_a_queue_gaps.txt:
// k_fe_ransac_commit -> k_fe_ransac_commit 6.6-7.3 us).  Measured: the merged launch loses more than that packet costs (lvk_lk_choice, lvk_internal.h).
struct LkSet {
    const lvk_pt2f* src_pts; const int* n_ptr;
    lvk_pt2f* w_curr; uint8_t* w_status;
    const unsigned long long* stored_desc;   // old tracks: the first-seen descriptors the gate compares with
    unsigned long long* w_desc;              // new points: the previous-image descriptor (out)
    lvk_pt2f* w_und;
    int is_new, pad_;
};
template <int WIN>
__global__ void __launch_bounds__(320) k_fe_lk_pipe(PyrView prev, PyrView next, LkSet set0, LkSet set1, int grid0,
                                                   HMat H, int width, int height, int max_count, double epsilon, FeDev* __restrict__ dev,
                                                   const uint8_t* __restrict__ cur_ext, const uint8_t* __restrict__ cur_blur,
                                                   const uint8_t* __restrict__ prv_ext, const uint8_t* __restrict__ prv_blur, CamParams cam)
{
    static_assert(WIN == 21, "row-segment layout");
    __shared__ lvk_pt2f s_np;
    __shared__ int s_st, s_dist;
    __shared__ __attribute__((aligned(16))) unsigned long long s_acc[4][4];
    __shared__ __attribute__((aligned(16))) LkTplLevel s_tpl[LK_PIPE_MAX_LEVELS];
    const bool second = (int)blockIdx.x >= grid0;
    const LkSet& S = second ? set1 : set0;
    const int p = (int)blockIdx.x - (second ? grid0 : 0);
    const lvk_pt2f* __restrict__ src_pts = S.src_pts; const int* __restrict__ n_ptr = S.n_ptr;
    lvk_pt2f* __restrict__ w_curr = S.w_curr; uint8_t* __restrict__ w_status = S.w_status;
    const unsigned long long* __restrict__ stored_desc = S.stored_desc; unsigned long long* __restrict__ w_desc = S.w_desc;
    lvk_pt2f* __restrict__ w_und = S.w_und; const int is_new = S.is_new;
    LkSpan span;
    if (p >= *n_ptr) return;
    const int wave = threadIdx.x >> 6;
    const int n_levels = prev.n_levels < next.n_levels ? prev.n_levels : next.n_levels;
    const int step = width + 2 * LVK_ORB_BORDER;
    const lvk_pt2f pp = src_pts[p];
    lvk_pt2f np = pp;
    int st = 1, its = 0;
    unsigned long long dp[4] = {0, 0, 0, 0};
    LkLdsAcc acc; acc.off = 0; acc.prev[0] = acc.prev[1] = acc.prev[2] = 0;
    if (wave < 4) acc = lk_acc_init(s_acc[wave]);
    if (!fe_lk_point_ok(pp, width, height, threadIdx.x == 0, 5, *n_ptr, p, is_new)) return;
    // ---- before the forward pass: its templates, the gyro-predicted start, the previous-image descriptor of a new point
    if (wave == 0) np = apply_h(H, pp);
    else if (wave < 4) { for (int level = wave - 1; level < n_levels; level += 3) lk_tpl_build21(prev, level, pp, s_tpl[level], acc); }
    else fe_desc_before(prv_ext, prv_blur, step, pp, p, is_new, dp, w_desc, cam, w_und);
    __syncthreads();
    if (wave == 0) {
        its = lk_pass_iterate21(next, n_levels, s_tpl, np, st, max_count, epsilon, acc);
        fe_lk_forward_done(np, st, width, height, s_np, s_st);
        span.fwd_done();
    }
    __syncthreads();
    const int fwd_ok = s_st;
    const lvk_pt2f fnp = s_np;
    // ---- before the reverse pass: its templates, from the point the forward pass found in the current image
    if (fwd_ok && wave >= 1 && wave < 4) { for (int level = wave - 1; level < n_levels; level += 3) lk_tpl_build21(next, level, fnp, s_tpl[level], acc); }
    __syncthreads();
    int code = ST_FWD, passes = 1;
    if (wave == 0) {
        if (st) {
            lvk_pt2f back = pp;
            int sr = 1;
            its += lk_pass_iterate21(prev, n_levels, s_tpl, back, sr, max_count, epsilon, acc);
            passes = 2;
            code = fe_lk_round_trip(pp, back, sr, width, height);
        }
        span.rev_done();
    } else if (wave == 4 && fwd_ok)
        fe_desc_after(cur_ext, cur_blur, step, fnp, fe_lk_point_ok(fnp, width, height, (threadIdx.x & 63) == 0, 6, *n_ptr, p, is_new), p, is_new, dp, stored_desc, cam, w_und, s_dist);
    __syncthreads();
    if (threadIdx.x == 0) fe_lk_finish(p, np, code, s_dist, passes, n_levels, its, w_curr, w_status, dev, span, !second);
}

// One workgroup of NT threads: count survivors per stage, order-preserving compaction of the alive points (wavefront ballots), the
// undistorted pairs the LK kernel left in w_und, cv::findFundamentalMat mask, then write the destination
// track set.  mode 0: old tracks (trackFeatures :701-808), 1: new points appended (trackNewFeatures
// :932-1001), 2: bootstrap (initializeFirstFeatures :464-536).
template <int NT>
__device__ __forceinline__ void fe_commit_block(int mode, int cap,
                                                const lvk_pt2f* src_pts, const int* n_ptr, const lvk_pt2f* w_curr, const uint8_t* w_status, const lvk_pt2f* w_und,
                                                const unsigned long long* src_id, const lvk_pt2f* src_init, const int* src_life, const unsigned long long* src_desc,
                                                const TrackSet& dst, int* dst_n, FeDev* dev,
                                                lvk_pt2f* s1, lvk_pt2f* s2, uint8_t* smask, unsigned short* sidx)
{   // s1, s2, smask, sidx: LDS scratch for FM_MAX_N points, owned by the calling kernel
    __shared__ int cnt[4];
    __shared__ int wtot[NT / 64];
    const int t = threadIdx.x;
#ifdef LVK_FM_TIMING
    if (t == 0) g_fm_on = mode == 0;
#endif
    FM_TICK(0);
    const int n = min(*n_ptr, cap);
    if (t < 4) cnt[t] = 0;
    __syncthreads();
    // survivors after each stage + ordered compaction of the alive ones (block scan over chunks)
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int i = c0 + t;
        const int st = i < n ? w_status[i] : 255;
        const bool alive = st == ST_ALIVE;
        const unsigned long long b_fwd = __ballot(i < n && st != ST_FWD);                    // after forward LK
        const unsigned long long b_rev = __ballot(i < n && st != ST_FWD && st != ST_REV);    // after reverse LK
        if ((t & 63) == 0) { atomicAdd(&cnt[0], (int)__popcll(b_fwd)); atomicAdd(&cnt[1], (int)__popcll(b_rev)); }
        int tot;
        const int rk = block_rank<NT>(alive, wtot, tot);
        if (alive) sidx[base + rk] = (unsigned short)i;
        base += tot;
    }
    __syncthreads();
    FM_TICK(1);
    const int m = base;                                                    // after the ORB gate
    bool fail = false;
    if (mode == 2) fail = cnt[0] < 20 || cnt[1] < 20 || m < 20;
    else if (mode == 1) fail = m < 20;
    int wrote = 0, iters = 0;
    if (!fail && m > 0) {
        for (int k = t; k < m; k += NT) {
            const int i = sidx[k];
            s1[k] = w_und[2 * (size_t)i];
            s2[k] = w_und[2 * (size_t)i + 1];
        }
        __syncthreads();
        FM_TICK(2);
        wrote = fm_mask_block<NT>(s1, s2, m, 1.0, 0.99, 1000, 0, smask, &iters);
        __syncthreads();
        FM_TICK(9);
    }
    // survivors of the mask (size mismatch => everything is kept, image_processor.h:219-223)
    int kept = 0;
    if (!fail) {
        int basek = 0;
        const int dst_base = (mode == 1) ? *dst_n : 0;
        for (int c0 = 0; c0 < m; c0 += NT) {
            const int k = c0 + t;
            const bool keep = k < m ? (wrote ? smask[k] != 0 : true) : false;
            int tot;
            const int rk = block_rank<NT>(keep, wtot, tot);
            if (keep) {
                const int i = sidx[k];
                const int d = dst_base + basek + rk;
                if (d < cap) {
                    dst.pts[d] = w_curr[i];
                    dst.ppts[d] = src_pts[i];
                    const unsigned long long* ds = src_desc + (size_t)i * 4;
                    unsigned long long* dd = dst.desc + (size_t)d * 4;
                    dd[0] = ds[0]; dd[1] = ds[1]; dd[2] = ds[2]; dd[3] = ds[3];
                    if (mode == 0) { dst.id[d] = src_id[i]; dst.life[d] = src_life[i] + 1; dst.init[d] = src_init[i]; }
                    else {
                        dst.id[d] = dev->next_id + (unsigned long long)(basek + rk);
                        dst.life[d] = 2;
                        if (mode == 1) dst.init[d] = src_pts[i];
                        else { dst.init[d].x = -1.f; dst.init[d].y = -1.f; }
                    }
                }
            }
            basek += tot;
        }
        kept = basek;
    }
    if (mode == 2 && kept < 20) fail = true;
    if (mode == 1 && kept <= 0) fail = true;
    __syncthreads();
    FM_TICK(10);
#ifdef LVK_FM_TIMING
    if (t == 0 && g_fm_on) { g_fm_tick[16 + 0] = m; g_fm_tick[16 + 1] = iters; g_fm_tick[16 + 2] = mode; }
#endif
    if (t == 0) {
        if (mode == 0) *dst_n = kept;
        else if (mode == 1) { if (!fail) { *dst_n = min(*dst_n + kept, cap); dev->next_id += (unsigned long long)kept; dev->n_new = 0; } }
        else {
            dev->boot_ok = fail ? 0 : 1;
            if (!fail) { *dst_n = kept; dev->next_id += (unsigned long long)kept; dev->n_new = 0; }
            else *dst_n = 0;
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(NT) k_fe_ransac_commit(int mode, int cap,
                                                       const lvk_pt2f* __restrict__ src_pts, const int* __restrict__ n_ptr,
                                                       const lvk_pt2f* __restrict__ w_curr, const uint8_t* __restrict__ w_status, const lvk_pt2f* __restrict__ w_und,
                                                       const unsigned long long* __restrict__ src_id, const lvk_pt2f* __restrict__ src_init,
                                                       const int* __restrict__ src_life, const unsigned long long* __restrict__ src_desc,
                                                       TrackSet dst, int* __restrict__ dst_n, FeDev* __restrict__ dev)
{
    __shared__ lvk_pt2f s1[FM_MAX_N], s2[FM_MAX_N];
    __shared__ uint8_t smask[FM_MAX_N];
    __shared__ unsigned short sidx[FM_MAX_N];
    fe_commit_block<NT>(mode, cap, src_pts, n_ptr, w_curr, w_status, w_und, src_id, src_init, src_life, src_desc, dst, dst_n, dev, s1, s2, smask, sidx);
}

// getFeatureMsg (:1076-1128): undistort to normalised coordinates, finite-difference velocities
__device__ __forceinline__ void fe_msg_one(const TrackSet& ts, int i, const CamParams& cam, double dt_1, double dt_2, int prev_is_last, lvk_feature_obs* out)
{
    const double unit[4] = {1, 1, 0, 0};
    const lvk_pt2f uc = undistort_point(ts.pts[i], cam, unit);
    const lvk_pt2f ini = ts.init[i];
    const lvk_pt2f ui = undistort_point(ini, cam, unit);
    const lvk_pt2f up = undistort_point(ts.ppts[i], cam, unit);
    lvk_feature_obs f;
    f.id = ts.id[i];
    f.u = uc.x; f.v = uc.y;
    f.u_vel = (uc.x - up.x) / dt_1;
    f.v_vel = (uc.y - up.y) / dt_1;
    f.u_init_vel = 0.0; f.v_init_vel = 0.0;
    if (ini.x == -1 && ini.y == -1) { f.u_init = -1; f.v_init = -1; }
    else {
        f.u_init = ui.x; f.v_init = ui.y;
        ts.init[i].x = -1.f; ts.init[i].y = -1.f;
        if (prev_is_last) { f.u_init_vel = (uc.x - ui.x) / dt_2; f.v_init_vel = (uc.y - ui.y) / dt_2; }
        else { f.u_init_vel = (up.x - ui.x) / dt_2; f.v_init_vel = (up.y - ui.y) / dt_2; }
    }
    out[i] = f;
}
__global__ void k_fe_msg(TrackSet ts, const int* __restrict__ n_ptr, CamParams cam, double dt_1, double dt_2, int prev_is_last,
                         lvk_feature_obs* __restrict__ out, FeDev* __restrict__ dev, int* __restrict__ n_host)
{   // `out` and `n_host` are device-mapped pinned host memory: the message needs no copy command, only the stream sync
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *n_ptr;
    if (i == 0) { dev->n_msg = n; *n_host = n; dev->msg_features += (unsigned long long)n; dev->msg_count += 1ull; }
    if (i >= n) return;
    fe_msg_one(ts, i, cam, dt_1, dt_2, prev_is_last, out);
}

// =========================================================================== launchers (what frontend.hip calls: fe_frontend.h)
static LkSet lk_set(const lvk_pt2f* src_pts, const int* n_ptr, lvk_pt2f* w_curr, uint8_t* w_status, const unsigned long long* stored_desc,
                    unsigned long long* w_desc, lvk_pt2f* w_und, int is_new)
{
    return LkSet{src_pts, n_ptr, w_curr, w_status, stored_desc, w_desc, w_und, is_new, 0};
}

template <int WIN>
static void launch_track_chain(lvk_frontend* fe, hipStream_t s, const PyrView& pv, const PyrView& cv, const lvk_pt2f* src_pts, const int* n_ptr, int grid,
                               const HMat& H, lvk_pt2f* w_curr, uint8_t* w_status, const unsigned long long* stored_desc,
                               unsigned long long* w_desc, int is_new, int max_count, double epsilon)
{
    const int W = fe->cfg.width, Hh = fe->cfg.height;
    if (fe->pyr_event) hipStreamWaitEvent(s, fe->ev_orb, 0);      // the frame start waited for the pyramid only: the ORB planes (read by the kernel's second wavefront) follow it on the image stream
    ProfScope ps(fe, 2, s);
    lvk_pt2f* const w_und = w_curr == fe->w_curr ? fe->w_und : fe->wn_und;
    if constexpr (WIN == 21) {
        if (lvk_lk_choice(WIN, fe->cap, pv.n_levels, cv.n_levels).pipe) {
            const LkSet a = lk_set(src_pts, n_ptr, w_curr, w_status, stored_desc, w_desc, w_und, is_new);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_lk_pipe<21>), dim3(grid), dim3(320), 0, s, pv, cv, a, a, grid, H, W, Hh, max_count, epsilon, fe->dev,
                               (const uint8_t*)fe->ext[1], (const uint8_t*)fe->blur[1], (const uint8_t*)fe->ext[0], (const uint8_t*)fe->blur[0], fe->cam);
            return;
        }
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_lk_both<WIN>), dim3(grid), dim3(128), 0, s, pv, cv, src_pts, n_ptr, H, W, Hh, max_count, epsilon, w_curr, w_status, fe->dev,
                       (const uint8_t*)fe->ext[1], (const uint8_t*)fe->blur[1], (const uint8_t*)fe->ext[0], (const uint8_t*)fe->blur[0], stored_desc, w_desc, is_new,
                       fe->cam, w_und);
}

lvk_status track_chain(lvk_frontend* fe, hipStream_t stream, const lvk_pt2f* src_pts, const int* n_ptr, const HMat& H, lvk_pt2f* w_curr, uint8_t* w_status,
                       const unsigned long long* stored_desc, unsigned long long* w_desc, int is_new)
{
    const LkTerm term = lvk_lk_term(fe->cfg.max_iteration, fe->cfg.track_precision);
    PyrView pv = make_view(fe->pyr[0]), cv = make_view(fe->pyr[1]);
    switch (fe->cfg.patch_size) {
        case 21: launch_track_chain<21>(fe, stream, pv, cv, src_pts, n_ptr, fe->cap, H, w_curr, w_status, stored_desc, w_desc, is_new, term.max_count, term.epsilon); break;
        case 15: launch_track_chain<15>(fe, stream, pv, cv, src_pts, n_ptr, fe->cap, H, w_curr, w_status, stored_desc, w_desc, is_new, term.max_count, term.epsilon); break;
        case 31: launch_track_chain<31>(fe, stream, pv, cv, src_pts, n_ptr, fe->cap, H, w_curr, w_status, stored_desc, w_desc, is_new, term.max_count, term.epsilon); break;
        default: return lvk_set_error(fe->ctx, LVK_ERR_UNSUPPORTED, "patch_size %d not instantiated (15, 21, 31)", fe->cfg.patch_size);
    }
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// trackFeatures' and trackNewFeatures' LK + descriptor gate in one launch on `stream`: blocks [0, cap) the old tracks of set `src`, [cap, 2 cap) the new points
lvk_status track_chain_merged(lvk_frontend* fe, hipStream_t stream, int src, const HMat& H)
{
    const LkTerm term = lvk_lk_term(fe->cfg.max_iteration, fe->cfg.track_precision);
    PyrView pv = make_view(fe->pyr[0]), cv = make_view(fe->pyr[1]);
    const LkSet a = lk_set(fe->set[src].pts, &fe->dev->n_tracks[src], fe->w_curr, fe->w_status, fe->set[src].desc, nullptr, fe->w_und, 0);
    const LkSet b = lk_set(fe->new_pts, &fe->dev->n_new, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, fe->wn_und, 1);
    if (fe->pyr_event) hipStreamWaitEvent(stream, fe->ev_orb, 0);
    {
        ProfScope ps(fe, 2, stream);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_lk_pipe<21>), dim3(2 * fe->cap), dim3(320), 0, stream, pv, cv, a, b, fe->cap, H, fe->cfg.width, fe->cfg.height, term.max_count, term.epsilon, fe->dev,
                           (const uint8_t*)fe->ext[1], (const uint8_t*)fe->blur[1], (const uint8_t*)fe->ext[0], (const uint8_t*)fe->blur[0], fe->cam);
    }
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

lvk_status commit(lvk_frontend* fe, int mode, const lvk_pt2f* src_pts, const int* n_ptr, const lvk_pt2f* w_curr, const uint8_t* w_status,
                  const TrackSet* src, const unsigned long long* desc_src, int dst_set)
{
    ProfScope ps(fe, 5);
    const lvk_pt2f* w_und = w_curr == fe->w_curr ? fe->w_und : fe->wn_und;
    // one workgroup either way: 1024 threads when the per-point loops (compaction, scoring, mask) are what the call costs
#define COMMIT_LAUNCH(NT) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_ransac_commit<NT>), dim3(1), dim3(NT), 0, fe->ctx->stream, mode, fe->cap, src_pts, n_ptr, w_curr, w_status, w_und, \
                           (const unsigned long long*)(src ? src->id : nullptr), (const lvk_pt2f*)(src ? src->init : nullptr),                                                       \
                           (const int*)(src ? src->life : nullptr), desc_src, fe->set[dst_set], &fe->dev->n_tracks[dst_set], fe->dev)
    if (fe->cap > FM_WIDE_FROM) COMMIT_LAUNCH(FM_THREADS_WIDE); else COMMIT_LAUNCH(FM_THREADS);
#undef COMMIT_LAUNCH
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// getFeatureMsg (:1076-1128) of set `dst` into the ring slot m names
lvk_status fe_msg_launch(lvk_frontend* fe, int dst, const FeMsgArgs& m)
{
    ProfScope ps8(fe, 8);
    hipLaunchKernelGGL(k_fe_msg, dim3((fe->cap + 63) / 64), dim3(64), 0, fe->ctx->stream, fe->set[dst], (const int*)&fe->dev->n_tracks[dst], fe->cam, m.dt_1, m.dt_2,
                       m.prev_is_last, m.out, fe->dev, m.n_host);
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// ---- readers of the instrumentation arrays: each is one copy per file, so what reads one lives with the kernels that write it
#ifdef LVK_LK_TIMING
extern "C" void lvk_debug_lk_ticks(unsigned long long* out, unsigned long long* span) { hipDeviceSynchronize(); hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lk_tick), sizeof(unsigned long long) * 4096 * 12); hipMemcpyFromSymbol(span, HIP_SYMBOL(g_lk_span), sizeof(unsigned long long) * 4096 * 4); }
#endif
#ifdef LVK_FM_TIMING
extern "C" void lvk_debug_fm_ticks(unsigned long long* out) { hipDeviceSynchronize(); hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fm_tick), sizeof(unsigned long long) * 32); }
#endif
#ifdef LVK_LK_BOUNDS
void fe_lk_bounds_report()
{
    int o[16] = {0}; hipDeviceSynchronize(); hipMemcpyFromSymbol(o, HIP_SYMBOL(g_lk_oob), sizeof o);
    float fx, fy; memcpy(&fx, &o[7], 4); memcpy(&fy, &o[8], 4);
    fprintf(stderr, "[lvk LK bounds] %d window loads outside their plane; first: site %d level %d of %d, row %d col %d of %d x %d, position (%g, %g), block %d thread %d\n",
            o[0], o[1], o[2], o[11], o[3], o[4], o[5], o[6], fx, fy, o[9], o[10]);
}
#endif
