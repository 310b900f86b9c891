// fe_global.hip — global ORB search of a device-resident map for gfx950 (wave64): which map point is each described corner of the frame?
// The frame's corners are the queries (at most 4096), the map is the database (at most 1,048,576 points).  No reference counterpart.
// include/lvk_c.h states the definition (lvk_orb_match_global); everything is integer, so every field has one right value.
//   k_global_search   a workgroup owns a slice of GLB_SLICE map points and a tile of GLB_TILE corners, one corner per lane: the corner's
//                     descriptor sits in eight 32-bit registers, the slice's descriptors are wave-uniform and come in through scalar
//                     loads (32 bytes per map point and wavefront, no per-lane global read, no LDS).  Per pair: 8 XORs, 8 accumulating
//                     population counts, one shift-or for the key (dist << 20 | map index: 29 bits, distinct because the index is part
//                     of them) and a three-operation update of the lane's two smallest keys.  The pair of keys goes to row `slice` of
//                     the slices x corners table.
//   k_global_pick     64 corners per workgroup, four wavefronts that each merge a quarter of the slices (consecutive corners: coalesced
//                     rows), combined through LDS.  The two smallest keys over all slices are the best and the runner-up whatever the
//                     slice and tile sizes are: the minimum of distinct integers does not depend on the order it is taken in.  Status
//                     rules; a provisionally matched corner resets its map point's claim word with a plain store - so only the words
//                     that can be touched are cleared, never the 8 MB a million points would need, and no call relies on what an
//                     earlier one left behind.
//   k_global_claim    one lane per corner: 64-bit atomicMin of (dist << 32 | corner) on the claim word, as k_orb_match does.
//   k_global_select   ONE workgroup of 1024 lanes, four corners per lane.  Resolves the claims, counts the statuses, and orders the OK
//                     corners by (dist, corner): a count per (64-corner group, distance) from wave ballots - which also give a lane its
//                     rank inside its group -, a running sum down every distance's column, a scan of the 257 totals.  No LDS atomic
//                     decides a position; the integer adds of the status counters do not depend on their order.
//   k_reloc_*         the gather kernels of lvk_frontend_relocalise_map (frontend.hip).
#include "lvk_internal.h"
#include "fe_frontend.h"

#define GLB_MAX_CAND 4096
#define GLB_MAX_SEL  1024
#define GLB_SLICE    2048                   // map points per workgroup of the search
#define GLB_TILE     256                    // corners per workgroup of the search, one per lane
#define GLB_KEY_NONE 0x7fffffff             // larger than any key: 256 << 20 | 1048575
#define GLB_PICK_GROUPS 4                   // wavefronts of k_global_pick, each over a quarter of the slices
#define GLB_SEL_THREADS 1024
#define GLB_SEL_PER     (GLB_MAX_CAND / GLB_SEL_THREADS)
#define GLB_BINS     257                    // distances 0..256

static_assert(LVK_MAP_MAX_POINTS <= (1 << 20), "the key keeps 20 bits for the map index");

// the two smallest of {k1, k2, key}, k1 < k2 or both none
__device__ __forceinline__ void glb_keep2(int& k1, int& k2, int key)
{
    const int hi = k1 > key ? k1 : key;
    k1 = k1 < key ? k1 : key;
    k2 = k2 < hi ? k2 : hi;
}

__global__ void __launch_bounds__(GLB_TILE) k_global_search(const uint32_t* __restrict__ map_desc, int n_map, const uint32_t* __restrict__ cand_desc, int n_cand,
                                                           int2* __restrict__ part)
{
    const int c = blockIdx.y * GLB_TILE + threadIdx.x;
    if ((c & ~63) >= n_cand) return;                     // (the whole wavefront is beyond the corners)
    const int cc = c < n_cand ? c : n_cand - 1;          // a lane beyond the last corner repeats it and writes nothing
    uint32_t q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = cand_desc[8 * (size_t)cc + k];
    const int m0 = blockIdx.x * GLB_SLICE;
    const int m1 = m0 + GLB_SLICE < n_map ? m0 + GLB_SLICE : n_map;
    int k1 = GLB_KEY_NONE, k2 = GLB_KEY_NONE;
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
        const uint32_t* d = map_desc + 8 * (size_t)m;    // wave-uniform: scalar loads
        int dist = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) dist += __popc(q[k] ^ d[k]);
        glb_keep2(k1, k2, (dist << 20) | m);
    }
    if (c < n_cand) part[(size_t)blockIdx.x * n_cand + c] = make_int2(k1, k2);
}

__global__ void __launch_bounds__(64 * GLB_PICK_GROUPS) k_global_pick(const int2* __restrict__ part, int n_slices, int n_map, int n_cand, int max_dist, int ratio_pct,
                                                                     unsigned long long* __restrict__ claim, lvk_match_result* __restrict__ out)
{
    __shared__ int2 s_k[GLB_PICK_GROUPS][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    int k1 = GLB_KEY_NONE, k2 = GLB_KEY_NONE;
    if (c < n_cand)
        for (int s = grp; s < n_slices; s += GLB_PICK_GROUPS) {
            const int2 p = part[(size_t)s * n_cand + c];
            glb_keep2(k1, k2, p.x);
            glb_keep2(k1, k2, p.y);
        }
    s_k[grp][lane] = make_int2(k1, k2);
    __syncthreads();
    if (grp != 0 || c >= n_cand) return;
#pragma unroll
    for (int g = 1; g < GLB_PICK_GROUPS; ++g) { const int2 p = s_k[g][lane]; glb_keep2(k1, k2, p.x); glb_keep2(k1, k2, p.y); }
    lvk_match_result r;
    r.n_window = n_map; r.pad = 0;
    if (k1 == GLB_KEY_NONE) { r.cand = -1; r.dist = -1; r.second = -1; r.status = LVK_MATCH_NO_CANDIDATE; out[c] = r; return; }
    r.cand = k1 & 0xFFFFF; r.dist = k1 >> 20;
    r.second = k2 == GLB_KEY_NONE ? -1 : k2 >> 20;
    if (r.dist > max_dist) r.status = LVK_MATCH_TOO_FAR;
    else if (r.second >= 0 && 100 * r.dist > ratio_pct * r.second) r.status = LVK_MATCH_AMBIGUOUS;
    else {
        r.status = LVK_MATCH_OK;                             // provisional until k_global_select has looked at the claim
        claim[r.cand] = ~0ull;                               // (several corners may store the same value here; the claims come in the next launch)
    }
    out[c] = r;
}

__global__ void k_global_claim(const lvk_match_result* __restrict__ out, int n_cand, unsigned long long* __restrict__ claim)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const lvk_match_result r = out[c];
    if (r.status == LVK_MATCH_OK) atomicMin(&claim[r.cand], ((unsigned long long)r.dist << 32) | (unsigned)c);
}

__global__ void __launch_bounds__(GLB_SEL_THREADS) k_global_select(const unsigned long long* __restrict__ claim, int n_cand, int max_matches, lvk_match_result* __restrict__ out,
                                                                  lvk_global_match* __restrict__ sel, lvk_global_info* __restrict__ info)
{
    __shared__ unsigned short s_cnt[GLB_MAX_CAND / 64][GLB_BINS];     // OK corners per (group of 64 corners, distance), then the groups before
    __shared__ int s_base[GLB_BINS];                                  // OK corners per distance, then those at smaller distances
    __shared__ int s_stat[5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned short* flat = &s_cnt[0][0];
    for (int i = threadIdx.x; i < (GLB_MAX_CAND / 64) * GLB_BINS; i += GLB_SEL_THREADS) flat[i] = 0;
    if (threadIdx.x < 5) s_stat[threadIdx.x] = 0;
    __syncthreads();
    lvk_match_result r[GLB_SEL_PER];
    int rank[GLB_SEL_PER];
    bool ok[GLB_SEL_PER];
#pragma unroll
    for (int p = 0; p < GLB_SEL_PER; ++p) {
        const int c = p * GLB_SEL_THREADS + threadIdx.x;     // group p * 16 + wave holds corners 64 (p * 16 + wave) .. + 63, in lane order
        const int g = p * (GLB_SEL_THREADS / 64) + wave;
        ok[p] = false; rank[p] = 0; r[p].dist = 0;
        if (c < n_cand) {
            r[p] = out[c];
            if (r[p].status == LVK_MATCH_OK && claim[r[p].cand] != (((unsigned long long)r[p].dist << 32) | (unsigned)c)) {
                r[p].status = LVK_MATCH_CONFLICT;
                out[c].status = LVK_MATCH_CONFLICT;
            }
            ok[p] = r[p].status == LVK_MATCH_OK;
            atomicAdd(&s_stat[r[p].status], 1);
        }
        unsigned long long rem = __ballot(ok[p]);
        while (rem) {                                        // (rem is the same on every lane)
            const int d = __shfl(r[p].dist, __ffsll((long long)rem) - 1, 64);
            const bool mine = ok[p] && r[p].dist == d;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                rank[p] = __popcll(m & ((1ull << lane) - 1ull));
                if (rank[p] == 0) s_cnt[g][d] = (unsigned short)__popcll(m);
            }
            rem &= ~m;
        }
    }
    __syncthreads();
    if (threadIdx.x < GLB_BINS) {                            // one lane per distance: the count of every group -> the count of the groups before it
        int run = 0;
        for (int g = 0; g < GLB_MAX_CAND / 64; ++g) { const int v = s_cnt[g][threadIdx.x]; s_cnt[g][threadIdx.x] = (unsigned short)run; run += v; }
        s_base[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int d = 0; d < GLB_BINS; ++d) { const int v = s_base[d]; s_base[d] = run; run += v; }
        lvk_global_info o;
        o.n_ok = s_stat[LVK_MATCH_OK]; o.n_no_candidate = s_stat[LVK_MATCH_NO_CANDIDATE]; o.n_too_far = s_stat[LVK_MATCH_TOO_FAR];
        o.n_ambiguous = s_stat[LVK_MATCH_AMBIGUOUS]; o.n_conflict = s_stat[LVK_MATCH_CONFLICT];
        o.n_selected = run < max_matches ? run : max_matches; o.pad[0] = 0; o.pad[1] = 0;
        *info = o;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < GLB_SEL_PER; ++p) {
        if (!ok[p]) continue;
        const int g = p * (GLB_SEL_THREADS / 64) + wave;
        const int pos = s_base[r[p].dist] + (int)s_cnt[g][r[p].dist] + rank[p];
        if (pos < max_matches) {
            lvk_global_match m;
            m.cand = p * GLB_SEL_THREADS + threadIdx.x; m.index = r[p].cand; m.dist = r[p].dist; m.second = r[p].second;
            sel[pos] = m;
        }
    }
}

extern "C" lvk_status lvk_orb_match_global(lvk_context* ctx, const uint8_t* d_map_desc, int n_map, const uint8_t* d_cand_desc, int n_cand, int max_dist, int ratio_pct,
                                           int max_matches, lvk_match_result* d_best, lvk_global_match* d_sel, lvk_global_info* d_info)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n_map < 0 || n_cand < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: negative count (n_map %d, n_cand %d)", n_map, n_cand);
    if ((n_map > 0 && !d_map_desc) || (n_cand > 0 && (!d_cand_desc || !d_best || !d_sel || !d_info))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: null pointer");
    if (max_dist < 0 || max_dist > 256) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: max_dist %d outside 0..256", max_dist);
    if (ratio_pct < 1 || ratio_pct > 100) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: ratio_pct %d outside 1..100", ratio_pct);
    if (max_matches < 1 || max_matches > GLB_MAX_SEL) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: max_matches %d outside 1..%d", max_matches, GLB_MAX_SEL);
    if ((((uintptr_t)d_map_desc) | ((uintptr_t)d_cand_desc)) & 7u) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_orb_match_global: descriptors must be 8-byte aligned");
    if (n_cand > GLB_MAX_CAND) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_orb_match_global: %d corners, at most %d", n_cand, GLB_MAX_CAND);
    if (n_map > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_orb_match_global: %d map points, at most %d", n_map, LVK_MAP_MAX_POINTS);
    if (n_cand == 0) return LVK_OK;
    const int n_slices = (n_map + GLB_SLICE - 1) / GLB_SLICE, n_tiles = (n_cand + GLB_TILE - 1) / GLB_TILE;
    // the work buffer: the slices x corners table of key pairs, then one claim word per map point
    const size_t part_bytes = sizeof(int2) * (size_t)n_slices * n_cand;
    // (an empty map needs neither: no slice is read and no corner is provisionally matched, so nothing dereferences the null pointers)
    int2* part = nullptr; unsigned long long* claim = nullptr;
    if (n_map > 0) {
        uint8_t* work = (uint8_t*)lvk_ctx_scratch(ctx, LVK_SCR_GLOBAL_WORK, part_bytes + sizeof(unsigned long long) * (size_t)n_map);
        if (!work) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_orb_match_global: scratch allocation failed");
        part = (int2*)work; claim = (unsigned long long*)(work + part_bytes);
    }
    if (n_slices > 0)
        hipLaunchKernelGGL(k_global_search, dim3(n_slices, n_tiles), dim3(GLB_TILE), 0, ctx->stream, reinterpret_cast<const uint32_t*>(d_map_desc), n_map,
                           reinterpret_cast<const uint32_t*>(d_cand_desc), n_cand, part);
    hipLaunchKernelGGL(k_global_pick, dim3((n_cand + 63) / 64), dim3(64 * GLB_PICK_GROUPS), 0, ctx->stream, (const int2*)part, n_slices, n_map, n_cand, max_dist, ratio_pct, claim,
                       d_best);
    hipLaunchKernelGGL(k_global_claim, dim3((n_cand + 255) / 256), dim3(256), 0, ctx->stream, (const lvk_match_result*)d_best, n_cand, claim);
    hipLaunchKernelGGL(k_global_select, dim3(1), dim3(GLB_SEL_THREADS), 0, ctx->stream, (const unsigned long long*)claim, n_cand, max_matches, d_best, d_sel, d_info);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

// =========================================================================== lvk_frontend_relocalise_map's gather kernels
// px[k] = the pixel of selected corner k
__global__ void k_reloc_pixels(const lvk_global_match* __restrict__ sel, int n, const lvk_pt2f* __restrict__ cand_pts, lvk_pt2f* __restrict__ px)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    px[k] = cand_pts[sel[k].cand];
}
// the alignment's match records (X = the map point, u, v = the normalised corner) and the host's records, inlier still 0
__global__ void k_reloc_gather(const lvk_global_match* __restrict__ sel, int n, const double* __restrict__ X, const lvk_pt2f* __restrict__ px,
                               const lvk_pt2f* __restrict__ und, lvk_align_match* __restrict__ am, lvk_reloc_match* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const lvk_global_match s = sel[k];
    lvk_align_match a;
#pragma unroll
    for (int i = 0; i < 3; ++i) a.X[i] = X[3 * (size_t)s.index + i];
    a.u = (double)und[k].x; a.v = (double)und[k].y;
    am[k] = a;
    lvk_reloc_match m;
    m.cand = s.cand; m.index = s.index; m.dist = s.dist; m.second = s.second; m.px = px[k]; m.und = und[k]; m.inlier = 0; m.pad = 0;
    out[k] = m;
}
__global__ void k_reloc_inliers(const uint8_t* __restrict__ mask, int n, lvk_reloc_match* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k].inlier = mask[k];
}

// the n selected corners' pixels and normalised coordinates (lvk_undistort_points with unit intrinsics, as the feature message has them), then
// the two record arrays
lvk_status fe_reloc_gather(lvk_context* ctx, const CamParams& cam, const lvk_global_match* d_sel, int n, const lvk_pt2f* d_cand_pts, const double* d_X, lvk_pt2f* d_px,
                           lvk_pt2f* d_und, lvk_align_match* d_am, lvk_reloc_match* d_out)
{
    static const double unit[4] = {1., 1., 0., 0.};
    if (n <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_reloc_pixels, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_sel, n, d_cand_pts, d_px);
    LVK_LAUNCH_CHECK(ctx);
    const lvk_status st = lvk_undistort_points(ctx, d_px, n, cam.intr, cam.model, cam.dist, unit, d_und);
    if (st != LVK_OK) return st;
    hipLaunchKernelGGL(k_reloc_gather, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_sel, n, d_X, (const lvk_pt2f*)d_px, (const lvk_pt2f*)d_und, d_am, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
lvk_status fe_reloc_inliers(lvk_context* ctx, const uint8_t* d_mask, int n, lvk_reloc_match* d_out)
{
    if (n <= 0) return LVK_OK;
    hipLaunchKernelGGL(k_reloc_inliers, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_mask, n, d_out);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
