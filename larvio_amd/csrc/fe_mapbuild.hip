// fe_mapbuild.hip — a session's raw map-point exports into the resident prior map, for gfx950 (wave64): cull the bad points, drop the worse
// copy of every near-duplicate, order the rest best first and gather them in set_map's layout.  No reference counterpart.  include/lvk_c.h
// states the definition (lvk_map_build); every expression here is written in the order stated there, FP64, no contraction.  Chunks of 256
// points, one point per lane:
//   k_mb_classify   one lane per point: score (-0 canonicalised), BAD / UNCERTAIN / OUT_OF_RANGE, and for an eligible point the packed cell
//                   key (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20); every other point's key is ~0, larger than any cell's.
//   sort            a stable LSD radix sort of (64-bit key, index), eight passes of eight bits, three launches a pass:
//     k_mb_hist       the chunk's count per digit, LDS integer adds (the sums do not depend on their order), one column of the 256 x chunks
//                     table, stored row by row;
//     k_mb_rowscan    one workgroup per digit: its row -> the count of the chunks before each chunk, and the row's total;
//     k_mb_scatter    the digits' offsets from the 256 totals (a block scan), then the ordered scatter: eight ballots, one per bit of the
//                     digit, give every lane the set of lanes of its wavefront with the same digit - its rank is the set bits below it,
//                     the set's size goes to LDS for the wavefronts above.  No atomic decides a position.
//   k_mb_dedup      after the sort by cell key, one lane per SORTED position (the lanes of a wavefront sit in the same few cells): the three
//                     cells cx - 1 .. cx + 1 of a (cy, cz) row are one run of consecutive keys, so nine binary searches and nine walks visit
//                     the 27 neighbour cells.  A candidate is tested position, then Hamming, then priority; the first hit ends the walk.
//                     Quadratic inside one crowded cell, on purpose not capped.
//   k_mb_keys       the sort key of the order: the score's bits for a KEPT point (non-negative finite doubles order as their bits), ~0 for
//                     the rest; d_status; the chunk's count per status (LDS integer adds) into a 5 x chunks table.
//   k_mb_info       one workgroup adds the table's rows up: d_info.
//   sort            the same eight passes on the score keys: stable, so equal scores keep their index order.
//   k_mb_gather     one lane per sorted position whose key is not ~0: d_order and the three gathered arrays.  Nothing beyond n_kept is written.
// No kernel overwrites anything a sibling workgroup reads, and no result depends on an atomic's or a workgroup's order.
#include "lvk_internal.h"
#include "fe_frontend.h"
#include <cmath>
#include <limits>

#define MB_CHUNK   256                       // points per workgroup
#define MB_WAVES   (MB_CHUNK / 64)
#define MB_BINS    256                       // eight bits a pass
#define MB_PASSES  8
#define MB_NONE    (~0ull)                   // the key of a point that takes no part: behind every cell key (63 bits) and every finite score
#define MB_CELL_MAX 1048575.                 // 2^20 - 1
#define MB_STATES  5

static_assert(LVK_MAP_MAX_POINTS <= (1 << 20), "4096 chunks of 256 points: the row scan takes a row in 16 tiles");

struct MbArgs { double max_score, r_dup, r2; int dup_max_dist, dedupe; };

// the exclusive running sum of v over the workgroup's MB_CHUNK lanes; *total = the sum.  s_w: MB_WAVES words of LDS
__device__ __forceinline__ int mb_block_scan(int v, int* s_w, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    __syncthreads();                                     // (the previous use of s_w is over)
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MB_WAVES; ++w) { const int t = s_w[w]; if (w < wave) before += t; all += t; }
    *total = all;
    return before + (incl - v);
}

__device__ __forceinline__ bool mb_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

__global__ void __launch_bounds__(MB_CHUNK) k_mb_classify(const double* __restrict__ X, const double* __restrict__ cov, const double* __restrict__ score_in, int n, MbArgs a,
                                                          unsigned long long* __restrict__ score_bits, unsigned long long* __restrict__ cell_key, uint8_t* __restrict__ st)
{
    const int i = blockIdx.x * MB_CHUNK + threadIdx.x;
    if (i >= n) return;
    const double x[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
    bool bad = !(mb_finite(x[0]) && mb_finite(x[1]) && mb_finite(x[2]));
    double score = 0.;
    if (cov) {
        double c[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { c[k] = cov[9 * (size_t)i + k]; bad = bad || !mb_finite(c[k]); }
        bad = bad || c[0] < 0. || c[4] < 0. || c[8] < 0.;
        score = (c[0] + c[4]) + c[8];
    }
    if (score_in) score = score_in[i];
    bad = bad || !mb_finite(score) || score < 0.;
    if (score == 0.) score = 0.;                         // -0 -> +0: the bits then order as the values
    int status = LVK_MAPB_KEPT;                          // (provisional for an eligible point until k_mb_dedup has looked)
    unsigned long long key = MB_NONE;
    if (bad) status = LVK_MAPB_BAD;
    else if (score > a.max_score) status = LVK_MAPB_UNCERTAIN;
    else if (a.dedupe) {
        const double c0 = floor(x[0] / a.r_dup), c1 = floor(x[1] / a.r_dup), c2 = floor(x[2] / a.r_dup);
        if (fabs(c0) > MB_CELL_MAX || fabs(c1) > MB_CELL_MAX || fabs(c2) > MB_CELL_MAX) status = LVK_MAPB_OUT_OF_RANGE;
        else key = ((unsigned long long)((long long)c2 + 1048576) << 42) | ((unsigned long long)((long long)c1 + 1048576) << 21) | (unsigned long long)((long long)c0 + 1048576);
    }
    score_bits[i] = (unsigned long long)__double_as_longlong(score);
    st[i] = (uint8_t)status;
    if (a.dedupe) cell_key[i] = key;
}

// ------------------------------------------------------------------------------------------------ one pass of the radix sort
__global__ void __launch_bounds__(MB_CHUNK) k_mb_hist(const unsigned long long* __restrict__ key, int n, int shift, int n_chunks, int* __restrict__ table)
{
    __shared__ int s_cnt[MB_BINS];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * MB_CHUNK + threadIdx.x;
    if (i < n) atomicAdd(&s_cnt[(int)((key[i] >> shift) & 255ull)], 1);
    __syncthreads();
    table[(size_t)threadIdx.x * n_chunks + blockIdx.x] = s_cnt[threadIdx.x];
}

// row blockIdx.x of the table, in place: the count of every chunk -> the count of the chunks before it; tot[row] = the row's sum
__global__ void __launch_bounds__(MB_CHUNK) k_mb_rowscan(int* __restrict__ table, int n_chunks, int* __restrict__ tot)
{
    __shared__ int s_w[MB_WAVES];
    int* row = table + (size_t)blockIdx.x * n_chunks;
    int carry = 0;
    for (int base = 0; base < n_chunks; base += MB_CHUNK) {          // (the trip count is the same on every lane)
        const int ch = base + threadIdx.x;
        const int v = ch < n_chunks ? row[ch] : 0;
        int total;
        const int excl = mb_block_scan(v, s_w, &total);
        if (ch < n_chunks) row[ch] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// val_in == nullptr: the values are the positions themselves (the first pass)
__global__ void __launch_bounds__(MB_CHUNK) k_mb_scatter(const unsigned long long* __restrict__ key_in, const int* __restrict__ val_in, int n, int shift, int n_chunks,
                                                         const int* __restrict__ table, const int* __restrict__ tot, unsigned long long* __restrict__ key_out,
                                                         int* __restrict__ val_out)
{
    __shared__ int s_base[MB_BINS];
    __shared__ int s_cnt[MB_WAVES][MB_BINS];
    __shared__ int s_w[MB_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int total;
    s_base[threadIdx.x] = mb_block_scan(tot[threadIdx.x], s_w, &total);      // the keys with a smaller digit
#pragma unroll
    for (int w = 0; w < MB_WAVES; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * MB_CHUNK + threadIdx.x;
    const bool valid = i < n;
    const unsigned long long key = valid ? key_in[i] : 0ull;
    const int d = (int)((key >> shift) & 255ull);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) s_cnt[wave][d] = __popcll(peers);
    __syncthreads();
    if (!valid) return;
    int pos = s_base[d] + table[(size_t)d * n_chunks + blockIdx.x] + rank;
    for (int w = 0; w < wave; ++w) pos += s_cnt[w][d];
    key_out[pos] = key;                                  // pos < n: the offsets count exactly the n keys
    val_out[pos] = val_in ? val_in[i] : i;
}

// ------------------------------------------------------------------------------------------------ the duplicate rule
// the first position in key[0 .. n) that is not below k
__device__ __forceinline__ int mb_lower_bound(const unsigned long long* __restrict__ key, int n, unsigned long long k)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(MB_CHUNK) k_mb_dedup(const unsigned long long* __restrict__ skey, const int* __restrict__ sval, int n, MbArgs a, const double* __restrict__ X,
                                                       const unsigned long long* __restrict__ desc, const unsigned long long* __restrict__ score_bits, uint8_t* __restrict__ st)
{
    const int p = blockIdx.x * MB_CHUNK + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = skey[p];
    if (key == MB_NONE) return;                          // not eligible: its status stands
    const int i = sval[p];
    const double x[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
    unsigned long long di[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) di[k] = desc[4 * (size_t)i + k];
    const unsigned long long si = score_bits[i];
    const long long px = (long long)(key & 0x1FFFFFull), py = (long long)((key >> 21) & 0x1FFFFFull), pz = (long long)(key >> 42);   // 1 .. 2^21 - 1 each
    bool dup = false;
    for (int oz = -1; oz <= 1 && !dup; ++oz)
        for (int oy = -1; oy <= 1 && !dup; ++oy) {
            const long long qy = py + oy, qz = pz + oz;
            if (qy < 1 || qy > 0x1FFFFF || qz < 1 || qz > 0x1FFFFF) continue;          // no such cell
            // the cells px - 1 .. px + 1 of this row: px - 1 = 0 and px + 1 = 2^21 are cells nobody is in
            const unsigned long long row = ((unsigned long long)qz << 42) | ((unsigned long long)qy << 21);
            const unsigned long long first = row + (unsigned long long)(px - 1), end = row + (unsigned long long)(px + 2);
            for (int q = mb_lower_bound(skey, n, first); q < n && skey[q] < end; ++q) {
                const int j = sval[q];
                if (j == i) continue;
                const double dx = x[0] - X[3 * (size_t)j], dy = x[1] - X[3 * (size_t)j + 1], dz = x[2] - X[3 * (size_t)j + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= a.r2)) continue;
                int ham = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) ham += __popcll(di[k] ^ desc[4 * (size_t)j + k]);
                if (ham > a.dup_max_dist) continue;
                const unsigned long long sj = score_bits[j];
                if (sj < si || (sj == si && j < i)) { dup = true; break; }
            }
        }
    if (dup) st[i] = (uint8_t)LVK_MAPB_DUPLICATE;
}

// ------------------------------------------------------------------------------------------------ the order
__global__ void __launch_bounds__(MB_CHUNK) k_mb_keys(const unsigned long long* __restrict__ score_bits, const uint8_t* __restrict__ st, int n, int n_chunks,
                                                      unsigned long long* __restrict__ key, uint8_t* __restrict__ status, int* __restrict__ counts)
{
    __shared__ int s_cnt[MB_STATES];
    if (threadIdx.x < MB_STATES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * MB_CHUNK + threadIdx.x;
    if (i < n) {
        const int s = st[i];
        key[i] = s == LVK_MAPB_KEPT ? score_bits[i] : MB_NONE;
        if (status) status[i] = (uint8_t)s;
        atomicAdd(&s_cnt[s], 1);
    }
    __syncthreads();
    if (threadIdx.x < MB_STATES) counts[(size_t)threadIdx.x * n_chunks + blockIdx.x] = s_cnt[threadIdx.x];
}

__global__ void __launch_bounds__(MB_CHUNK) k_mb_info(const int* __restrict__ counts, int n_chunks, lvk_map_build_info* __restrict__ info)
{
    __shared__ int s_w[MB_WAVES];
    __shared__ int s_tot[MB_STATES];
    for (int s = 0; s < MB_STATES; ++s) {
        int v = 0;
        for (int ch = threadIdx.x; ch < n_chunks; ch += MB_CHUNK) v += counts[(size_t)s * n_chunks + ch];
        int total;
        (void)mb_block_scan(v, s_w, &total);
        if (threadIdx.x == 0) s_tot[s] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lvk_map_build_info o;
        o.n_kept = s_tot[LVK_MAPB_KEPT]; o.n_bad = s_tot[LVK_MAPB_BAD]; o.n_uncertain = s_tot[LVK_MAPB_UNCERTAIN]; o.n_out_of_range = s_tot[LVK_MAPB_OUT_OF_RANGE];
        o.n_duplicate = s_tot[LVK_MAPB_DUPLICATE]; o.pad[0] = 0; o.pad[1] = 0; o.pad[2] = 0;
        *info = o;
    }
}

__global__ void __launch_bounds__(MB_CHUNK) k_mb_gather(const unsigned long long* __restrict__ skey, const int* __restrict__ sval, int n, const double* __restrict__ X,
                                                        const double* __restrict__ cov, const unsigned long long* __restrict__ desc, int* __restrict__ order,
                                                        double* __restrict__ X_out, double* __restrict__ cov_out, unsigned long long* __restrict__ desc_out)
{
    const int p = blockIdx.x * MB_CHUNK + threadIdx.x;
    if (p >= n || skey[p] == MB_NONE) return;            // the kept points are the first n_kept positions
    const int i = sval[p];
    order[p] = i;
    if (X_out) {
#pragma unroll
        for (int k = 0; k < 3; ++k) X_out[3 * (size_t)p + k] = X[3 * (size_t)i + k];
    }
    if (cov_out) {
#pragma unroll
        for (int k = 0; k < 9; ++k) cov_out[9 * (size_t)p + k] = cov[9 * (size_t)i + k];
    }
    if (desc_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) desc_out[4 * (size_t)p + k] = desc[4 * (size_t)i + k];
    }
}

// the stable sort of (key[0], identity) by key: ping-pong between buffers 0 and 1, MB_PASSES is even, so the result is back in key[0], val[0]
static void mb_sort(hipStream_t stream, unsigned long long* const key[2], int* const val[2], int n, int n_chunks, int* table, int* tot)
{
    for (int pass = 0; pass < MB_PASSES; ++pass) {
        const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
        hipLaunchKernelGGL(k_mb_hist, dim3(n_chunks), dim3(MB_CHUNK), 0, stream, (const unsigned long long*)key[in], n, shift, n_chunks, table);
        hipLaunchKernelGGL(k_mb_rowscan, dim3(MB_BINS), dim3(MB_CHUNK), 0, stream, table, n_chunks, tot);
        hipLaunchKernelGGL(k_mb_scatter, dim3(n_chunks), dim3(MB_CHUNK), 0, stream, (const unsigned long long*)key[in], pass ? (const int*)val[in] : (const int*)nullptr, n, shift,
                           n_chunks, (const int*)table, (const int*)tot, key[out], val[out]);
    }
}

// the options with their defaults filled in and their ranges checked; false: *why names the field
static bool mb_options(const lvk_map_build_options* opt, lvk_map_build_options* o, const char** why)
{
    lvk_map_build_options a;
    memset(&a, 0, sizeof a);
    if (opt) a = *opt;
    if (std::isnan(a.max_score) || std::isnan(a.r_dup)) { *why = "an option is NaN"; return false; }
    if (a.max_score < 0. || a.r_dup < 0.) { *why = "an option is negative"; return false; }
    if (a.dup_max_dist < 0 || a.dup_max_dist > 256) { *why = "dup_max_dist outside 0..256"; return false; }
    if (a.max_score == 0.) a.max_score = std::numeric_limits<double>::infinity();
    if (a.dup_max_dist == 0) a.dup_max_dist = 32;
    a.pad = 0;
    *o = a;
    return true;
}
bool fe_map_build_options_ok(const lvk_map_build_options* opt, const char** why)
{
    lvk_map_build_options o;
    return mb_options(opt, &o, why);
}

extern "C" lvk_status lvk_map_build(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, const double* d_score, int n,
                                    const lvk_map_build_options* opt, int* d_order, double* d_X_out, double* d_cov_out, uint8_t* d_desc_out, uint8_t* d_status,
                                    lvk_map_build_info* d_info)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_build: negative count (n %d)", n);
    lvk_map_build_options o; const char* why = "";
    if (!mb_options(opt, &o, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_build: %s", why);
    const bool dedupe = o.r_dup > 0.;
    if (!d_info || (n > 0 && (!d_X || !d_order || !d_X_out || (d_cov && !d_cov_out) || (d_desc && !d_desc_out)))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_build: null pointer");
    if (n > 0 && dedupe && !d_desc) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_build: r_dup > 0 needs the descriptors");
    if (d_desc && ((((uintptr_t)d_desc) | ((uintptr_t)d_desc_out)) & 7u)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_build: descriptors must be 8-byte aligned");
    if (n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_map_build: %d points, at most %d", n, LVK_MAP_MAX_POINTS);
    if (n == 0) { LVK_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(lvk_map_build_info), ctx->stream)); return LVK_OK; }

    const int n_chunks = (n + MB_CHUNK - 1) / MB_CHUNK;
    // the work buffer: two key and two index arrays (the sort's ping-pong), the scores' bits, the digit x chunk table, the status x chunk
    // table, the digits' totals, the status bytes - the 8-byte arrays first
    const size_t n8 = sizeof(unsigned long long) * (size_t)n, n4 = sizeof(int) * (size_t)n;
    const size_t table_bytes = sizeof(int) * (size_t)MB_BINS * n_chunks, counts_bytes = sizeof(int) * (size_t)MB_STATES * n_chunks, tot_bytes = sizeof(int) * MB_BINS;
    uint8_t* work = (uint8_t*)lvk_ctx_scratch(ctx, LVK_SCR_MAPBUILD_WORK, 3 * n8 + 2 * n4 + table_bytes + counts_bytes + tot_bytes + (size_t)n);
    if (!work) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_map_build: scratch allocation failed");
    unsigned long long* const key[2] = {(unsigned long long*)work, (unsigned long long*)(work + n8)};
    unsigned long long* score_bits = (unsigned long long*)(work + 2 * n8);
    int* const val[2] = {(int*)(work + 3 * n8), (int*)(work + 3 * n8 + n4)};
    int* table = (int*)(work + 3 * n8 + 2 * n4);
    int* counts = (int*)((uint8_t*)table + table_bytes);
    int* tot = (int*)((uint8_t*)counts + counts_bytes);
    uint8_t* st = (uint8_t*)tot + tot_bytes;

    MbArgs a;
    a.max_score = o.max_score; a.r_dup = o.r_dup; a.r2 = o.r_dup * o.r_dup; a.dup_max_dist = o.dup_max_dist; a.dedupe = dedupe ? 1 : 0;
    const unsigned long long* desc = reinterpret_cast<const unsigned long long*>(d_desc);
    hipLaunchKernelGGL(k_mb_classify, dim3(n_chunks), dim3(MB_CHUNK), 0, ctx->stream, d_X, d_cov, d_score, n, a, score_bits, key[0], st);
    if (dedupe) {
        mb_sort(ctx->stream, key, val, n, n_chunks, table, tot);
        hipLaunchKernelGGL(k_mb_dedup, dim3(n_chunks), dim3(MB_CHUNK), 0, ctx->stream, (const unsigned long long*)key[0], (const int*)val[0], n, a, d_X, desc,
                           (const unsigned long long*)score_bits, st);
    }
    hipLaunchKernelGGL(k_mb_keys, dim3(n_chunks), dim3(MB_CHUNK), 0, ctx->stream, (const unsigned long long*)score_bits, (const uint8_t*)st, n, n_chunks, key[0], d_status, counts);
    hipLaunchKernelGGL(k_mb_info, dim3(1), dim3(MB_CHUNK), 0, ctx->stream, (const int*)counts, n_chunks, d_info);
    mb_sort(ctx->stream, key, val, n, n_chunks, table, tot);
    // an output whose input is NULL is not touched, whatever the caller passed for it: the gather reads what it writes from
    hipLaunchKernelGGL(k_mb_gather, dim3(n_chunks), dim3(MB_CHUNK), 0, ctx->stream, (const unsigned long long*)key[0], (const int*)val[0], n, d_X, d_cov, desc, d_order, d_X_out,
                       d_cov ? d_cov_out : (double*)nullptr, d_desc ? reinterpret_cast<unsigned long long*>(d_desc_out) : (unsigned long long*)nullptr);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
