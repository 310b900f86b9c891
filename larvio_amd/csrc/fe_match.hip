// fe_match.hip — guided ORB matching for gfx950 (wave64): which described corner of the current frame is map point q?  No reference
// counterpart: the reference tracks what it detected itself and never looks a known point up in a frame.
//   k_orb_match          one wavefront per query, four queries per workgroup.  The workgroup stages every candidate position in LDS once
//                        (8 bytes each, 32 KB at the 4096-candidate cap) and its four wavefronts sweep them 64 at a time; a lane reads the
//                        32-byte descriptor of its candidate from global memory only when the candidate is inside the query's window.
//                        Each lane keeps the smallest and the second smallest key (dist << 12 | index) it met; two wave-wide minima give the
//                        best and the runner-up.  A provisionally matched query claims its candidate with a 64-bit atomicMin of
//                        (dist << 32 | query) on the candidate's claim word.
//   k_orb_match_resolve  one thread per query: a provisional match whose claim word is not its own key lost the candidate.
// Everything but the in-window test is integer; the test is float32 as written (the library is built with -ffp-contract=off), so the
// result has exactly one right answer (include/lvk_c.h states it).
#include "lvk_internal.h"
#include "fe_track_dev.h"
#include "fe_frontend.h"

#define MATCH_MAX_CAND 4096
#define MATCH_MAX_Q    1024
#define MATCH_WAVES    4                    // queries per workgroup
#define MATCH_KEY_NONE 0x7fffffff           // larger than any key: 256 << 12 | 4095

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
    return v;
}

__global__ void __launch_bounds__(64 * MATCH_WAVES) k_orb_match(const lvk_pt2f* __restrict__ cand_pts, const unsigned long long* __restrict__ cand_desc, int n_cand,
                                                               const lvk_match_query* __restrict__ qs, const unsigned long long* __restrict__ q_desc, int n_q,
                                                               int max_dist, int ratio_pct, unsigned long long* __restrict__ claim, lvk_match_result* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    lvk_pt2f* s_pts = reinterpret_cast<lvk_pt2f*>(s_raw);
    for (int i = threadIdx.x; i < n_cand; i += 64 * MATCH_WAVES) s_pts[i] = cand_pts[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * MATCH_WAVES + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const lvk_match_query mq = qs[q];
    const float r2 = mq.radius * mq.radius;
    unsigned long long qd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) qd[k] = q_desc[(size_t)q * 4 + k];
    int k1 = MATCH_KEY_NONE, k2 = MATCH_KEY_NONE, cnt = 0;
    for (int c = lane; c < n_cand; c += 64) {
        const lvk_pt2f p = s_pts[c];
        const float dx = p.x - mq.x, dy = p.y - mq.y;
        if (dx * dx + dy * dy <= r2) {                       // false for a NaN anywhere
            const int key = (hamming256_u64(qd, cand_desc + (size_t)c * 4) << 12) | c;
            if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
            ++cnt;
        }
    }
    // keys are distinct (the index is part of them): the smallest is the best candidate, ties in distance to the lowest index; the smallest of
    // the others carries the runner-up distance
    const int best = wave_min_i32(k1);
    const int sec = wave_min_i32(k1 == best ? k2 : k1);
    const int n_window = wave_sum_i32(cnt);
    if (lane != 0) return;
    lvk_match_result r;
    r.n_window = n_window; r.pad = 0;
    if (n_window == 0) { r.cand = -1; r.dist = -1; r.second = -1; r.status = LVK_MATCH_NO_CANDIDATE; out[q] = r; return; }
    r.cand = best & 0xFFF; r.dist = best >> 12;
    r.second = sec == MATCH_KEY_NONE ? -1 : sec >> 12;
    if (r.dist > max_dist) r.status = LVK_MATCH_TOO_FAR;
    else if (r.second >= 0 && 100 * r.dist > ratio_pct * r.second) r.status = LVK_MATCH_AMBIGUOUS;
    else {
        r.status = LVK_MATCH_OK;                             // provisional until k_orb_match_resolve has looked at the claim
        atomicMin(&claim[r.cand], ((unsigned long long)r.dist << 32) | (unsigned)q);
    }
    out[q] = r;
}

__global__ void k_orb_match_resolve(const unsigned long long* __restrict__ claim, int n_q, lvk_match_result* __restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const lvk_match_result r = out[q];
    if (r.status != LVK_MATCH_OK) return;
    if (claim[r.cand] != (((unsigned long long)r.dist << 32) | (unsigned)q)) out[q].status = LVK_MATCH_CONFLICT;
}

// px[q] = the pixel of the query's candidate ((0, 0) when it has none: a point the undistortion accepts)
__global__ void k_match_pixels(const lvk_match_result* __restrict__ res, const lvk_pt2f* __restrict__ cand_pts, int n_q, lvk_pt2f* __restrict__ px)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const int c = res[q].cand;
    lvk_pt2f p; p.x = 0.f; p.y = 0.f;
    if (c >= 0) p = cand_pts[c];
    px[q] = p;
}
__global__ void k_match_pack(const lvk_match_result* __restrict__ res, const lvk_pt2f* __restrict__ px, const lvk_pt2f* __restrict__ und, int n_q,
                             lvk_landmark_match* __restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const lvk_match_result r = res[q];
    lvk_landmark_match m;
    m.status = r.status; m.dist = r.dist; m.second = r.second; m.n_window = r.n_window;
    m.px = px[q]; m.und = und[q];
    if (r.cand < 0) { m.und.x = 0.f; m.und.y = 0.f; }
    out[q] = m;
}

extern "C" lvk_status lvk_orb_match_guided(lvk_context* ctx, const lvk_pt2f* d_cand_pts, const uint8_t* d_cand_desc, int n_cand, const lvk_match_query* d_q,
                                           const uint8_t* d_q_desc, int n_q, int max_dist, int ratio_pct, lvk_match_result* d_out)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n_cand < 0 || n_q < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_guided: negative count (n_cand %d, n_q %d)", n_cand, n_q);
    if ((n_cand > 0 && (!d_cand_pts || !d_cand_desc)) || (n_q > 0 && (!d_q || !d_q_desc || !d_out))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_guided: null pointer");
    if (max_dist < 0 || max_dist > 256) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_guided: max_dist %d outside 0..256", max_dist);
    if (ratio_pct < 1 || ratio_pct > 100) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_guided: ratio_pct %d outside 1..100", ratio_pct);
    if ((((uintptr_t)d_cand_desc) | ((uintptr_t)d_q_desc)) & 7u) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_guided: descriptors must be 8-byte aligned");
    if (n_cand > MATCH_MAX_CAND) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_orb_match_guided: %d candidates, at most %d (their positions are staged in LDS)", n_cand, MATCH_MAX_CAND);
    if (n_q > MATCH_MAX_Q) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_orb_match_guided: %d queries, at most %d", n_q, MATCH_MAX_Q);
    if (n_q == 0) return LVK_OK;
    unsigned long long* claim = (unsigned long long*)lvk_ctx_scratch(ctx, LVK_SCR_MATCH_CLAIM, sizeof(unsigned long long) * MATCH_MAX_CAND);
    if (!claim) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_orb_match_guided: scratch allocation failed");
    if (n_cand > 0) LVK_HIP(ctx, hipMemsetAsync(claim, 0xFF, sizeof(unsigned long long) * (size_t)n_cand, ctx->stream));
    hipLaunchKernelGGL(k_orb_match, dim3((n_q + MATCH_WAVES - 1) / MATCH_WAVES), dim3(64 * MATCH_WAVES), sizeof(lvk_pt2f) * (size_t)n_cand, ctx->stream, d_cand_pts,
                       reinterpret_cast<const unsigned long long*>(d_cand_desc), n_cand, d_q, reinterpret_cast<const unsigned long long*>(d_q_desc), n_q, max_dist, ratio_pct,
                       claim, d_out);
    hipLaunchKernelGGL(k_orb_match_resolve, dim3((n_q + 255) / 256), dim3(256), 0, ctx->stream, (const unsigned long long*)claim, n_q, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// the tail of lvk_frontend_match_landmarks on the context's stream: the candidates' pixels of the n_q results, their normalised coordinates
// (lvk_undistort_points with unit intrinsics, as the feature message has them) and the records the host reads
lvk_status fe_match_finish(lvk_context* ctx, const CamParams& cam, const lvk_match_result* d_res, const lvk_pt2f* d_cand_pts, int n_q, lvk_pt2f* d_px, lvk_pt2f* d_und,
                           lvk_landmark_match* d_out)
{
    static const double unit[4] = {1., 1., 0., 0.};
    hipLaunchKernelGGL(k_match_pixels, dim3((n_q + 255) / 256), dim3(256), 0, ctx->stream, d_res, d_cand_pts, n_q, d_px);
    LVK_LAUNCH_CHECK(ctx);
    const lvk_status st = lvk_undistort_points(ctx, d_px, n_q, cam.intr, cam.model, cam.dist, unit, d_und);
    if (st != LVK_OK) return st;
    hipLaunchKernelGGL(k_match_pack, dim3((n_q + 255) / 256), dim3(256), 0, ctx->stream, d_res, (const lvk_pt2f*)d_px, (const lvk_pt2f*)d_und, n_q, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
