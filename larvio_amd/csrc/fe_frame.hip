// fe_frame.hip — the kernels of a steady-state frame and their launchers: LK forward + reverse with the ORB descriptor gate in their
// shadow (k_fe_lk_both, k_fe_lk_pipe), RANSAC + commit of a track set (k_fe_ransac_commit), the feature message (k_fe_msg).
// frontend.hip decides what a frame queues and on which stream; the launches themselves are here, next to the kernels (fe_frontend.h),
// and so are the three stage entries that run one such launch on a caller's host arrays (lvk_fe_track_stage, lvk_fe_commit_stage,
// lvk_fe_msg_stage, include/lvk_c.h).
#include "lvk_internal.h"
#include "fe_track_dev.h"
#include "fe_frontend.h"
#include <math.h>
#include <cmath>

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

// ---- the launch code itself: ONE place per kernel, for the frame path (an lvk_frontend owns the buffers) and the stage entries (a caller does)
struct LkFrame {        // what an LK launch reads besides its track sets
    hipStream_t stream; PyrView pv, cv; int width, height; LkTerm term; FeDev* dev;
    const uint8_t *cur_ext, *cur_blur, *prv_ext, *prv_blur; CamParams cam;
};
// pipe: k_fe_lk_pipe<21> over `grid` blocks, [0, grid0) set a, the rest set b (one set: b = a, grid = grid0); otherwise k_fe_lk_both<WIN> over set a's grid0
template <int WIN>
static void lk_launch(const LkFrame& f, bool pipe, const LkSet& a, const LkSet& b, int grid0, int grid, const HMat& H)
{
    if constexpr (WIN == 21) {
        if (pipe) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_lk_pipe<21>), dim3(grid), dim3(320), 0, f.stream, f.pv, f.cv, a, b, grid0, H, f.width, f.height, f.term.max_count, f.term.epsilon, f.dev,
                               f.cur_ext, f.cur_blur, f.prv_ext, f.prv_blur, f.cam);
            return;
        }
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_lk_both<WIN>), dim3(grid0), dim3(128), 0, f.stream, f.pv, f.cv, a.src_pts, a.n_ptr, H, f.width, f.height, f.term.max_count, f.term.epsilon,
                       a.w_curr, a.w_status, f.dev, f.cur_ext, f.cur_blur, f.prv_ext, f.prv_blur, a.stored_desc, a.w_desc, a.is_new, f.cam, a.w_und);
}
static bool lk_launch_window(int patch_size, const LkFrame& f, bool pipe, const LkSet& a, const LkSet& b, int grid0, int grid, const HMat& H)
{   // false: window not instantiated, nothing launched
    switch (patch_size) {
        case 21: lk_launch<21>(f, pipe, a, b, grid0, grid, H); return true;
        case 15: lk_launch<15>(f, false, a, b, grid0, grid, H); return true;
        case 31: lk_launch<31>(f, false, a, b, grid0, grid, H); return true;
        default: return false;
    }
}
// one workgroup either way: FM_THREADS_WIDE threads when the per-point loops (compaction, scoring, mask) are what the call costs - by the slot count, not by n
static void commit_launch(hipStream_t stream, int mode, int cap, const lvk_pt2f* src_pts, const int* n_ptr, const lvk_pt2f* w_curr, const uint8_t* w_status, const lvk_pt2f* w_und,
                          const unsigned long long* src_id, const lvk_pt2f* src_init, const int* src_life, const unsigned long long* desc_src,
                          const TrackSet& dst, int* dst_n, FeDev* dev)
{
#define COMMIT_LAUNCH(NT) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_ransac_commit<NT>), dim3(1), dim3(NT), 0, stream, mode, cap, src_pts, n_ptr, w_curr, w_status, w_und, \
                           src_id, src_init, src_life, desc_src, dst, dst_n, dev)
    if (cap > FM_WIDE_FROM) COMMIT_LAUNCH(FM_THREADS_WIDE); else COMMIT_LAUNCH(FM_THREADS);
#undef COMMIT_LAUNCH
}
static void msg_launch(hipStream_t stream, int cap, const TrackSet& ts, const int* n_ptr, const CamParams& cam, double dt_1, double dt_2, int prev_is_last,
                       lvk_feature_obs* out, FeDev* dev, int* n_host)
{
    hipLaunchKernelGGL(k_fe_msg, dim3((cap + 63) / 64), dim3(64), 0, stream, ts, n_ptr, cam, dt_1, dt_2, prev_is_last, out, dev, n_host);
}

// ---- the frame path's side of it
static LkFrame lk_frame_of(const lvk_frontend* fe, hipStream_t stream)
{
    return LkFrame{stream, make_view(fe->pyr[0]), make_view(fe->pyr[1]), fe->cfg.width, fe->cfg.height, lvk_lk_term(fe->cfg.max_iteration, fe->cfg.track_precision), fe->dev,
                   fe->ext[1], fe->blur[1], fe->ext[0], fe->blur[0], fe->cam};
}

lvk_status track_chain(lvk_frontend* fe, hipStream_t stream, const lvk_pt2f* src_pts, const int* n_ptr, const HMat& H, lvk_pt2f* w_curr, uint8_t* w_status,
                       const unsigned long long* stored_desc, unsigned long long* w_desc, int is_new)
{
    const LkFrame f = lk_frame_of(fe, stream);
    const LkSet a = lk_set(src_pts, n_ptr, w_curr, w_status, stored_desc, w_desc, w_curr == fe->w_curr ? fe->w_und : fe->wn_und, is_new);
    const bool pipe = lvk_lk_choice(fe->cfg.patch_size, fe->cap, f.pv.n_levels, f.cv.n_levels).pipe;
    if (fe->pyr_event) hipStreamWaitEvent(stream, fe->ev_orb, 0);      // the frame start waited for the pyramid only: the ORB planes (read by the kernel's second wavefront) follow it on the image stream
    {
        ProfScope ps(fe, 2, stream);
        if (!lk_launch_window(fe->cfg.patch_size, f, pipe, a, a, fe->cap, fe->cap, H))
            return lvk_set_error(fe->ctx, LVK_ERR_UNSUPPORTED, "patch_size %d not instantiated (15, 21, 31)", fe->cfg.patch_size);
    }
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// trackFeatures' and trackNewFeatures' LK + descriptor gate in one launch on `stream`: blocks [0, cap) the old tracks of set `src`, [cap, 2 cap) the new points
lvk_status track_chain_merged(lvk_frontend* fe, hipStream_t stream, int src, const HMat& H)
{
    const LkFrame f = lk_frame_of(fe, stream);
    const LkSet a = lk_set(fe->set[src].pts, &fe->dev->n_tracks[src], fe->w_curr, fe->w_status, fe->set[src].desc, nullptr, fe->w_und, 0);
    const LkSet b = lk_set(fe->new_pts, &fe->dev->n_new, fe->wn_curr, fe->wn_status, nullptr, fe->wn_desc, fe->wn_und, 1);
    if (fe->pyr_event) hipStreamWaitEvent(stream, fe->ev_orb, 0);
    {
        ProfScope ps(fe, 2, stream);
        lk_launch<21>(f, true, a, b, fe->cap, 2 * fe->cap, H);
    }
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

lvk_status commit(lvk_frontend* fe, int mode, const lvk_pt2f* src_pts, const int* n_ptr, const lvk_pt2f* w_curr, const uint8_t* w_status,
                  const TrackSet* src, const unsigned long long* desc_src, int dst_set)
{
    ProfScope ps(fe, 5);
    commit_launch(fe->ctx->stream, mode, fe->cap, src_pts, n_ptr, w_curr, w_status, w_curr == fe->w_curr ? fe->w_und : fe->wn_und,
                  src ? src->id : nullptr, src ? src->init : nullptr, src ? src->life : nullptr, desc_src, fe->set[dst_set], &fe->dev->n_tracks[dst_set], fe->dev);
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// getFeatureMsg (:1076-1128) of set `dst` into the ring slot m names
lvk_status fe_msg_launch(lvk_frontend* fe, int dst, const FeMsgArgs& m)
{
    ProfScope ps8(fe, 8);
    msg_launch(fe->ctx->stream, fe->cap, fe->set[dst], &fe->dev->n_tracks[dst], fe->cam, m.dt_1, m.dt_2, m.prev_is_last, m.out, fe->dev, m.n_host);
    LVK_LAUNCH_CHECK(fe->ctx);
    return LVK_OK;
}

// =========================================================================== stage entries (include/lvk_c.h): the same launches on a caller's host arrays
// Everything is checked on the host before anything is queued; buffers live for the call and every entry ends with a wait for the stream.
namespace {
struct StageBufs {      // device buffers of one stage call
    lvk_context* ctx; std::vector<void*> all; bool ok = true;
    explicit StageBufs(lvk_context* c) : ctx(c) { }
    ~StageBufs() { for (void* p : all) hipFree(p); }
    template <typename T> T* get(size_t n) { T* p = nullptr; if (!dalloc(&p, n)) { ok = false; (void)hipGetLastError(); return nullptr; } all.push_back(p); return p; }
    template <typename T> T* filled(size_t n, int byte) { T* p = get<T>(n); if (p && hipMemsetAsync(p, byte, sizeof(T) * (n ? n : 1), ctx->stream) != hipSuccess) ok = false; return p; }
    template <typename T> T* up(const T* h, size_t n) { T* p = get<T>(n); if (p && n && hipMemcpyAsync(p, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ok = false; return p; }
    template <typename T> void down(T* h, const T* d, size_t n) { if (ok && n && hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ok = false; }
};
bool pt_finite(lvk_pt2f p) { return std::isfinite(p.x) && std::isfinite(p.y); }
bool stage_cam(CamParams* cam, int model, const double* intr, const double* dist, int width, int height)
{
    if ((model != 0 && model != 1) || !intr || !dist) return false;
    memset(cam, 0, sizeof *cam);
    for (int i = 0; i < 4; ++i) { if (!std::isfinite(intr[i]) || !std::isfinite(dist[i])) return false; cam->intr[i] = intr[i]; cam->dist[i] = dist[i]; }
    cam->model = model; cam->width = width; cam->height = height;
    return true;
}
const char* track_set_refusal(const lvk_fe_track_io* s, int width, int height, lvk_status* code)
{
    *code = LVK_ERR_ARG;
    if (s->n < 0 || s->grid < 0 || s->n > s->grid) return "0 <= n <= grid required";
    if (s->grid > FM_MAX_N) { *code = LVK_ERR_CAPACITY; return "more slots than a front-end can have"; }
    if (s->is_new != 0 && s->is_new != 1) return "is_new must be 0 or 1";
    if (s->grid > 0 && (!s->h_curr || !s->h_status || !s->h_und || (s->is_new && !s->h_desc))) return "null output array";
    if (s->n > 0 && (!s->h_src_pts || (!s->is_new && !s->h_stored_desc))) return "null input array";
    for (int i = 0; i < s->n; ++i) {
        const lvk_pt2f p = s->h_src_pts[i];
        if (!pt_finite(p) || p.x < 0 || p.x > width - 1 || p.y < 0 || p.y > height - 1) return "a source point outside the image";
    }
    return nullptr;
}
}   // namespace

extern "C" {

lvk_status lvk_fe_track_stage(lvk_context* ctx, const lvk_pyramid* prev, const lvk_pyramid* next, const uint8_t* d_prev_ext, const uint8_t* d_prev_blur,
                              const uint8_t* d_next_ext, const uint8_t* d_next_blur, int width, int height, int patch_size, int variant, const float H[9],
                              int model, const double intr[4], const double dist[4], int max_iteration, double track_precision, int fill_byte,
                              const lvk_fe_track_io* set0, const lvk_fe_track_io* set1, uint64_t h_counters[2])
{
    if (!ctx) return LVK_ERR_ARG;
    if (!prev || !next || !d_prev_ext || !d_prev_blur || !d_next_ext || !d_next_blur || !H || !set0 || !h_counters) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: null pointer");
    if (width < 1 || height < 1 || prev->w[0] != width || prev->h[0] != height || next->w[0] != width || next->h[0] != height)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: pyramids are not %d x %d", width, height);
    if (patch_size != 15 && patch_size != 21 && patch_size != 31) return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "lvk_fe_track_stage: patch_size %d not instantiated (15, 21, 31)", patch_size);
    if (prev->pad != patch_size || next->pad != patch_size) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: pyramids not built for window %d", patch_size);
    if (prev->n_levels < 1 || next->n_levels < 1) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: a pyramid has not been built");
    if (variant != 1 && variant != 2) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: variant must be 1 (k_fe_lk_both) or 2 (k_fe_lk_pipe)");
    if (variant == 2 && patch_size != 21) return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "lvk_fe_track_stage: the five-wavefront kernel has the 21 x 21 window only");
    if (variant == 2 && (prev->n_levels > LK_PIPE_MAX_LEVELS || next->n_levels > LK_PIPE_MAX_LEVELS))
        return lvk_set_error(ctx, LVK_ERR_UNSUPPORTED, "lvk_fe_track_stage: the five-wavefront kernel keeps templates for %d levels", LK_PIPE_MAX_LEVELS);
    if (variant == 1 && set1) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: the two-set launch is the five-wavefront kernel's");
    for (int i = 0; i < 9; ++i) if (!std::isfinite(H[i])) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: H is not finite");
    LkFrame f;
    if (!stage_cam(&f.cam, model, intr, dist, width, height)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_track_stage: bad camera");
    const lvk_fe_track_io* io[2] = {set0, set1};
    const int n_sets = set1 ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        lvk_status code;
        if (const char* why = track_set_refusal(io[k], width, height, &code)) return lvk_set_error(ctx, code, "lvk_fe_track_stage: set %d: %s", k, why);
    }
    StageBufs B(ctx);
    FeDev hd; memset(&hd, 0, sizeof hd);
    hd.lk_point_levels = h_counters[0]; hd.lk_iterations = h_counters[1]; hd.n_tracks[0] = set0->n; hd.n_new = set1 ? set1->n : 0;
    FeDev* dev = B.up(&hd, 1);
    LkSet ls[2];
    for (int k = 0; k < n_sets && B.ok; ++k) {
        const lvk_fe_track_io* s = io[k];
        ls[k] = lk_set(B.up(s->h_src_pts, s->n), k ? &dev->n_new : &dev->n_tracks[0], B.filled<lvk_pt2f>(s->grid, fill_byte), B.filled<uint8_t>(s->grid, fill_byte),
                       s->is_new ? nullptr : (const unsigned long long*)B.up(s->h_stored_desc, (size_t)s->n * 4),
                       s->is_new ? B.filled<unsigned long long>((size_t)s->grid * 4, fill_byte) : nullptr, B.filled<lvk_pt2f>((size_t)s->grid * 2, fill_byte), s->is_new);
    }
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_track_stage: allocation or copy failed");
    const int grid0 = set0->grid, grid = grid0 + (set1 ? set1->grid : 0);
    f.stream = ctx->stream; f.pv = make_view(prev); f.cv = make_view(next); f.width = width; f.height = height; f.term = lvk_lk_term(max_iteration, track_precision); f.dev = dev;
    f.cur_ext = d_next_ext; f.cur_blur = d_next_blur; f.prv_ext = d_prev_ext; f.prv_blur = d_prev_blur;
    HMat Hm; memcpy(Hm.h, H, sizeof Hm.h);
    if (grid > 0) {                     // no slots, no launch
        lk_launch_window(patch_size, f, variant == 2, ls[0], ls[n_sets - 1], grid0, grid, Hm);
        LVK_LAUNCH_CHECK(ctx);
    }
    for (int k = 0; k < n_sets; ++k) {
        const lvk_fe_track_io* s = io[k];
        B.down(s->h_curr, ls[k].w_curr, s->grid); B.down(s->h_status, ls[k].w_status, s->grid); B.down(s->h_und, ls[k].w_und, (size_t)s->grid * 2);
        if (s->is_new) B.down((unsigned long long*)s->h_desc, ls[k].w_desc, (size_t)s->grid * 4);
    }
    B.down(&hd, dev, 1);
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_track_stage: copy failed");
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_counters[0] = hd.lk_point_levels; h_counters[1] = hd.lk_iterations;
    return LVK_OK;
}

lvk_status lvk_fe_commit_stage(lvk_context* ctx, int mode, int cap, int n, const lvk_pt2f* h_src_pts, const lvk_pt2f* h_curr, const uint8_t* h_status, const lvk_pt2f* h_und,
                               const uint64_t* h_src_id, const lvk_pt2f* h_src_init, const int* h_src_life, const uint64_t* h_src_desc,
                               const lvk_fe_track_arrays* h_dst, lvk_fe_commit_state* h_state)
{
    if (!ctx) return LVK_ERR_ARG;
    if (mode < 0 || mode > 2) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: mode must be 0, 1 or 2");
    if (cap < 1 || n < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: cap >= 1 and n >= 0 required");
    if (cap > FM_MAX_N) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_fe_commit_stage: cap %d beyond the %d points the kernel has LDS for", cap, FM_MAX_N);
    if (n > cap) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_fe_commit_stage: n %d beyond cap %d", n, cap);
    if (!h_dst || !h_state || !h_dst->id || !h_dst->pts || !h_dst->ppts || !h_dst->init || !h_dst->life || !h_dst->desc) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: null pointer");
    if (n > 0 && (!h_src_pts || !h_curr || !h_status || !h_und || !h_src_desc || (mode == 0 && (!h_src_id || !h_src_init || !h_src_life))))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: null input array");
    if (h_state->dst_n < 0 || h_state->dst_n > cap) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: dst_n %d outside [0, cap]", h_state->dst_n);
    if (mode != 0 && h_state->n_new != n) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: modes 1 and 2 commit the n_new new points: n_new must equal n");
    for (int i = 0; i < n; ++i) {
        if (h_status[i] > ST_ORB) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: status byte %d of point %d", (int)h_status[i], i);
        if (!pt_finite(h_und[2 * i]) || !pt_finite(h_und[2 * i + 1])) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_commit_stage: undistorted pair %d is not finite", i);
    }
    StageBufs B(ctx);
    FeDev hd; memset(&hd, 0, sizeof hd);
    hd.next_id = h_state->next_id; hd.n_new = h_state->n_new; hd.boot_ok = h_state->boot_ok;
    hd.n_tracks[0] = n; hd.n_tracks[1] = h_state->dst_n;                                     // as a frame has them: the source count in n_tracks[src] (mode 0) or n_new, the destination's in n_tracks[dst]
    FeDev* dev = B.up(&hd, 1);
    TrackSet dst;
    dst.id = (unsigned long long*)B.up(h_dst->id, cap); dst.pts = B.up(h_dst->pts, cap); dst.ppts = B.up(h_dst->ppts, cap); dst.init = B.up(h_dst->init, cap);
    dst.life = B.up(h_dst->life, cap); dst.desc = (unsigned long long*)B.up(h_dst->desc, (size_t)cap * 4);
    const lvk_pt2f* src_pts = B.up(h_src_pts, n); const lvk_pt2f* w_curr = B.up(h_curr, n); const uint8_t* w_status = B.up(h_status, n); const lvk_pt2f* w_und = B.up(h_und, (size_t)n * 2);
    const unsigned long long* src_desc = (const unsigned long long*)B.up(h_src_desc, (size_t)n * 4);
    const unsigned long long* src_id = mode == 0 ? (const unsigned long long*)B.up(h_src_id, n) : nullptr;
    const lvk_pt2f* src_init = mode == 0 ? B.up(h_src_init, n) : nullptr;
    const int* src_life = mode == 0 ? B.up(h_src_life, n) : nullptr;
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_commit_stage: allocation or copy failed");
    commit_launch(ctx->stream, mode, cap, src_pts, mode == 0 ? &dev->n_tracks[0] : &dev->n_new, w_curr, w_status, w_und, src_id, src_init, src_life, src_desc, dst, &dev->n_tracks[1], dev);
    LVK_LAUNCH_CHECK(ctx);
    B.down((unsigned long long*)h_dst->id, dst.id, cap); B.down(h_dst->pts, dst.pts, cap); B.down(h_dst->ppts, dst.ppts, cap); B.down(h_dst->init, dst.init, cap);
    B.down(h_dst->life, dst.life, cap); B.down((unsigned long long*)h_dst->desc, dst.desc, (size_t)cap * 4);
    B.down(&hd, dev, 1);
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_commit_stage: copy failed");
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_state->next_id = hd.next_id; h_state->dst_n = hd.n_tracks[1]; h_state->n_new = hd.n_new; h_state->boot_ok = hd.boot_ok;
    return LVK_OK;
}

lvk_status lvk_fe_msg_stage(lvk_context* ctx, const lvk_fe_track_arrays* h_set, int cap, int n, int model, const double intr[4], const double dist[4],
                            double dt_1, double dt_2, int prev_is_last, int fill_byte, lvk_feature_obs* h_out, lvk_fe_msg_state* h_state)
{
    if (!ctx) return LVK_ERR_ARG;
    if (cap < 1 || n < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_msg_stage: cap >= 1 and n >= 0 required");
    if (cap > FM_MAX_N) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_fe_msg_stage: cap %d beyond the %d slots a front-end can have", cap, FM_MAX_N);
    if (n > cap) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_fe_msg_stage: n %d beyond cap %d", n, cap);
    if (!h_set || !h_out || !h_state || !h_set->id || !h_set->pts || !h_set->ppts || !h_set->init) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_msg_stage: null pointer");
    if (prev_is_last != 0 && prev_is_last != 1) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_msg_stage: prev_is_last must be 0 or 1");
    if (!std::isfinite(dt_1) || !std::isfinite(dt_2)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_msg_stage: dt is not finite");
    CamParams cam;
    if (!stage_cam(&cam, model, intr, dist, 0, 0)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_fe_msg_stage: bad camera");
    StageBufs B(ctx);
    FeDev hd; memset(&hd, 0, sizeof hd);
    hd.n_tracks[0] = n; hd.n_msg = h_state->n_msg; hd.msg_features = h_state->msg_features; hd.msg_count = h_state->msg_count;
    FeDev* dev = B.up(&hd, 1);
    TrackSet ts; memset(&ts, 0, sizeof ts);                                                    // the message reads id, pts, ppts and init, and resets init
    ts.id = (unsigned long long*)B.up(h_set->id, cap); ts.pts = B.up(h_set->pts, cap); ts.ppts = B.up(h_set->ppts, cap); ts.init = B.up(h_set->init, cap);
    lvk_feature_obs* out = B.filled<lvk_feature_obs>(cap, fill_byte);
    int* n_host = B.up(&h_state->n_host, 1);
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_msg_stage: allocation or copy failed");
    msg_launch(ctx->stream, cap, ts, &dev->n_tracks[0], cam, dt_1, dt_2, prev_is_last, out, dev, n_host);
    LVK_LAUNCH_CHECK(ctx);
    B.down(h_out, out, cap); B.down(h_set->init, ts.init, cap); B.down(&h_state->n_host, n_host, 1); B.down(&hd, dev, 1);
    if (!B.ok) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_fe_msg_stage: copy failed");
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_state->n_msg = hd.n_msg; h_state->msg_features = hd.msg_features; h_state->msg_count = hd.msg_count;
    return LVK_OK;
}

}   // extern "C"

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
