// fe_map.hip — a device-resident prior map seen from a pose prediction, for gfx950 (wave64): where each point should appear, how far the
// matcher may look for it, and which at most 1024 points to ask it about.  No reference counterpart.  include/lvk_c.h states the definition
// (lvk_map_select_queries); every expression here is written in the order stated there, FP64, no contraction.  An ordered stream
// compaction in three launches, chunks of 256 points (one point per lane):
//   k_map_project   one lane per point: pose, forward model (fe_camera_dev.h), status and cell - 24 bytes read, 2 written (status | cell
//                   << 8).  The workgroup counts its points per cell and per other status in LDS (integer adds: the sums do not depend on
//                   their order) and writes one column of the (cells + 3) x chunks table, stored row by row.
//   k_map_scan      one workgroup.  A wavefront takes a row, 64 chunks at a time (consecutive words), and turns it into the exclusive running
//                   count by a shuffle scan plus a carry; the row totals give the cells' output offsets (each capped at the quota), the
//                   status counts and n_selected.
//   k_map_scatter   one lane per point again.  A point is live when it is VISIBLE and its cell had not filled its quota in earlier chunks
//                   (the others do nothing more).  Its rank inside the chunk comes from wave ballots: the wavefront walks the distinct
//                   cells of its live lanes, a ballot per cell gives every lane of that cell its rank in the wavefront (the set bits
//                   below it) and the wavefront's count, which goes to LDS for the wavefronts above.  rank < quota: the lane projects
//                   its point once more - the same device function on the same operands: the same bits -, now with the radius, which
//                   is the only place the 72-byte covariance is read, and writes record, query and descriptor at offset[cell] + rank.
// No kernel overwrites anything a sibling workgroup reads, and no result depends on an atomic's order.
#include "lvk_internal.h"
#include "fe_camera_dev.h"
#include <math.h>
#include <cmath>
#include <limits>

#define MAP_CHUNK     256                    // points per workgroup
#define MAP_WAVES     (MAP_CHUNK / 64)
#define MAP_MAX_CELLS 256                    // 16 x 16
#define MAP_OTHER     3                      // BEHIND, FAR, OUTSIDE: rows cells .. cells + 2 of the table

struct MapArgs {
    double c, s, t[3];                       // the alignment
    double Rwc[9], p[3];                     // R_wc row-major, p_wc
    double R[9];                             // Rz^T R_wc
    double C[36];                            // cov_cam
    CamParams cam;
    double min_depth, max_depth, max_r2, margin, hi_x, hi_y, k_sigma, sigma2, r_min, r_max;
    int rows, cols, quota, has_cov_cam;
};
struct MapPoint { int status, cell; double x, y, pc[3], px, py; };

// pose, forward model, status and cell of the point X
__device__ __forceinline__ void map_point(const MapArgs& a, const double* X, MapPoint& o)
{
    const double q0 = a.c * X[0] - a.s * X[1], q1 = a.s * X[0] + a.c * X[1];
    const double g0 = (q0 + a.t[0]) - a.p[0], g1 = (q1 + a.t[1]) - a.p[1], g2 = (X[2] + a.t[2]) - a.p[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.pc[i] = (a.Rwc[i] * g0 + a.Rwc[3 + i] * g1) + a.Rwc[6 + i] * g2;
    o.x = o.pc[0] / o.pc[2]; o.y = o.pc[1] / o.pc[2];
    const double r2 = o.x * o.x + o.y * o.y;
    cam_project(a.cam, o.x, o.y, r2, o.px, o.py);
    o.cell = 0;
    if (!(o.pc[2] > a.min_depth)) { o.status = LVK_MAP_BEHIND; return; }
    if (o.pc[2] > a.max_depth) { o.status = LVK_MAP_FAR; return; }
    if (!(r2 <= a.max_r2)) { o.status = LVK_MAP_OUTSIDE; return; }
    if (!(a.margin <= o.px && o.px <= a.hi_x && a.margin <= o.py && o.py <= a.hi_y)) { o.status = LVK_MAP_OUTSIDE; return; }
    o.status = LVK_MAP_VISIBLE;
    const int col = (int)((o.px * (double)a.cols) / (double)a.cam.width), row = (int)((o.py * (double)a.rows) / (double)a.cam.height);
    o.cell = (row < a.rows - 1 ? row : a.rows - 1) * a.cols + (col < a.cols - 1 ? col : a.cols - 1);
}

// the search radius of a projected point; S: its covariance (map frame, row-major) when has_cov
__device__ __forceinline__ double map_radius(const MapArgs& a, const MapPoint& o, const double (&S)[9], bool has_cov)
{
    double lam = 0.;
    if (has_cov || a.has_cov_cam) {
        double Sc[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        if (has_cov) {
            double M[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) M[3 * i + j] = (S[3 * i] * a.R[j] + S[3 * i + 1] * a.R[3 + j]) + S[3 * i + 2] * a.R[6 + j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Sc[3 * i + j] = (a.R[i] * M[j] + a.R[3 + i] * M[3 + j]) + a.R[6 + i] * M[6 + j];
        }
        if (a.has_cov_cam) {
            const double G[18] = {0., -o.pc[2], o.pc[1], -a.Rwc[0], -a.Rwc[3], -a.Rwc[6],
                                  o.pc[2], 0., -o.pc[0], -a.Rwc[1], -a.Rwc[4], -a.Rwc[7],
                                  -o.pc[1], o.pc[0], 0., -a.Rwc[2], -a.Rwc[5], -a.Rwc[8]};
            double T[18];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    double acc = G[6 * i] * a.C[k];
#pragma unroll
                    for (int m = 1; m < 6; ++m) acc = acc + G[6 * i + m] * a.C[6 * m + k];
                    T[6 * i + k] = acc;
                }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double acc = T[6 * i] * G[6 * j];
#pragma unroll
                    for (int k = 1; k < 6; ++k) acc = acc + T[6 * i + k] * G[6 * j + k];
                    Sc[3 * i + j] = has_cov ? Sc[3 * i + j] + acc : acc;
                }
        }
        const double u0 = Sc[0] - o.x * Sc[6], u1 = Sc[1] - o.x * Sc[7], u2 = Sc[2] - o.x * Sc[8];
        const double v0 = Sc[3] - o.y * Sc[6], v1 = Sc[4] - o.y * Sc[7], v2 = Sc[5] - o.y * Sc[8];
        const double e00 = u0 - u2 * o.x, e01 = u1 - u2 * o.y, e10 = v0 - v2 * o.x, e11 = v1 - v2 * o.y;
        const double sx = a.cam.intr[0] / o.pc[2], sy = a.cam.intr[1] / o.pc[2];
        const double pa = (sx * sx) * e00, pd = (sy * sy) * e11, pb = ((sx * sy) * e01 + (sx * sy) * e10) / 2.;
        const double hd = (pa - pd) / 2.;
        lam = (pa + pd) / 2. + sqrt(hd * hd + pb * pb);
    }
    if (!(lam >= 0.) || !(lam <= 1.7976931348623157e308)) return a.r_max;
    const double r = a.k_sigma * sqrt(lam + a.sigma2);
    return r < a.r_min ? a.r_min : r > a.r_max ? a.r_max : r;
}

__global__ void __launch_bounds__(MAP_CHUNK) k_map_project(const double* __restrict__ X, int n, MapArgs a, int n_chunks, unsigned short* __restrict__ code,
                                                          int* __restrict__ table)
{
    __shared__ int s_cnt[MAP_MAX_CELLS + MAP_OTHER];
    const int n_rows = a.rows * a.cols + MAP_OTHER;
    for (int r = threadIdx.x; r < n_rows; r += MAP_CHUNK) s_cnt[r] = 0;
    __syncthreads();
    const int i = blockIdx.x * MAP_CHUNK + threadIdx.x;
    if (i < n) {
        const double x[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
        MapPoint o;
        map_point(a, x, o);
        code[i] = (unsigned short)(o.status | (o.cell << 8));
        atomicAdd(&s_cnt[o.status == LVK_MAP_VISIBLE ? o.cell : n_rows - MAP_OTHER + (o.status - 1)], 1);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_rows; r += MAP_CHUNK) table[(size_t)r * n_chunks + blockIdx.x] = s_cnt[r];
}

// table row r, in place: the count of every chunk -> the count of the chunks before it.  cell_base[c] = the output offset of cell c
__global__ void __launch_bounds__(MAP_CHUNK) k_map_scan(int* __restrict__ table, int n_chunks, int n_cells, int quota, int* __restrict__ cell_base, lvk_map_info* __restrict__ info)
{
    __shared__ int s_tot[MAP_MAX_CELLS + MAP_OTHER];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < n_cells + MAP_OTHER; r += MAP_WAVES) {
        int* row = table + (size_t)r * n_chunks;
        int carry = 0;
        for (int base = 0; base < n_chunks; base += 64) {
            const int ch = base + lane;
            const int v = ch < n_chunks ? row[ch] : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
            if (ch < n_chunks) row[ch] = carry + (incl - v);
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) s_tot[r] = carry;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int base = 0, vis = 0;
        for (int c = 0; c < n_cells; ++c) { cell_base[c] = base; base += s_tot[c] < quota ? s_tot[c] : quota; vis += s_tot[c]; }
        lvk_map_info o;
        o.n_selected = base; o.n_visible = vis; o.n_behind = s_tot[n_cells]; o.n_far = s_tot[n_cells + 1]; o.n_outside = s_tot[n_cells + 2];
        o.n_candidates = 0; o.pad[0] = 0; o.pad[1] = 0;
        *info = o;
    }
}

__global__ void __launch_bounds__(MAP_CHUNK) k_map_scatter(const double* __restrict__ X, const double* __restrict__ cov, const unsigned long long* __restrict__ desc, int n,
                                                          MapArgs a, int n_chunks, const unsigned short* __restrict__ code, const int* __restrict__ table,
                                                          const int* __restrict__ cell_base, lvk_map_sel* __restrict__ sel, lvk_match_query* __restrict__ q,
                                                          unsigned long long* __restrict__ q_desc, uint8_t* __restrict__ status)
{
    __shared__ int s_w[MAP_WAVES][MAP_MAX_CELLS];
    const int n_cells = a.rows * a.cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = threadIdx.x; r < MAP_WAVES * MAP_MAX_CELLS; r += MAP_CHUNK) s_w[r / MAP_MAX_CELLS][r % MAP_MAX_CELLS] = 0;
    __syncthreads();
    const int i = blockIdx.x * MAP_CHUNK + threadIdx.x;
    const int cd = i < n ? (int)code[i] : LVK_MAP_BEHIND;
    const int st = cd & 0xFF, cell = cd >> 8;
    const bool vis = st == LVK_MAP_VISIBLE && cell < n_cells;
    const int start = vis ? table[(size_t)cell * n_chunks + blockIdx.x] : 0;
    const bool live = vis && start < a.quota;            // a cell that filled its quota in earlier chunks needs no further work
    int rank = 0;
    unsigned long long rem = __ballot(live);
    while (rem) {                                        // (rem is the same on every lane)
        const int c = __shfl(cell, __ffsll((long long)rem) - 1, 64);
        const bool mine = live && cell == c;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            rank = __popcll(m & ((1ull << lane) - 1ull));
            if (rank == 0) s_w[wave][c] = __popcll(m);
        }
        rem &= ~m;
    }
    __syncthreads();
    bool chosen = false;
    if (live) {
        rank += start;
        for (int w = 0; w < wave; ++w) rank += s_w[w][cell];
        if (rank < a.quota) {
            chosen = true;
            const int pos = cell_base[cell] + rank;
            const double x[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
            MapPoint o;
            map_point(a, x, o);
            double S[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            if (cov) {
#pragma unroll
                for (int k = 0; k < 9; ++k) S[k] = cov[9 * (size_t)i + k];
            }
            const double rad = map_radius(a, o, S, cov != nullptr);
            lvk_map_sel r;
            r.index = i; r.cell = cell; r.x = (float)o.px; r.y = (float)o.py; r.radius = (float)rad; r.depth = (float)o.pc[2];
            sel[pos] = r;
            lvk_match_query mq;
            mq.x = r.x; mq.y = r.y; mq.radius = r.radius; mq.pad = 0.f;
            q[pos] = mq;
            if (desc) {
#pragma unroll
                for (int k = 0; k < 4; ++k) q_desc[4 * (size_t)pos + k] = desc[4 * (size_t)i + k];
            }
        }
    }
    if (status && i < n) status[i] = (uint8_t)(st | (chosen ? LVK_MAP_SELECTED : 0));
}

static bool map_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// the options with their defaults filled in and their ranges checked; false: *why names the field
static bool map_options(const lvk_map_select_options* opt, lvk_map_select_options* o, const char** why)
{
    lvk_map_select_options a;
    memset(&a, 0, sizeof a);
    if (opt) a = *opt;
    const double* f = &a.min_depth;
    for (int k = 0; k < 8; ++k) if (std::isnan(f[k])) { *why = "an option is NaN"; return false; }
    if (a.min_depth == 0.) a.min_depth = 0.1;
    if (a.max_depth == 0.) a.max_depth = std::numeric_limits<double>::infinity();
    if (a.max_r2 == 0.) a.max_r2 = std::numeric_limits<double>::infinity();
    if (a.k_sigma == 0.) a.k_sigma = 3.;
    if (a.sigma_px == 0.) a.sigma_px = 1.;
    if (a.r_min == 0.) a.r_min = 4.;
    if (a.r_max == 0.) a.r_max = 40.;
    if (a.rows == 0) a.rows = 4;
    if (a.cols == 0) a.cols = 5;
    if (a.margin < 0.) { *why = "margin is negative"; return false; }
    if (a.r_min > a.r_max) { *why = "r_min > r_max"; return false; }
    if (a.rows < 1 || a.rows > 16 || a.cols < 1 || a.cols > 16) { *why = "rows and cols must be in 1..16"; return false; }
    if (a.quota == 0) a.quota = LVK_MAP_MAX_QUERIES / (a.rows * a.cols);
    if (a.quota < 1) { *why = "quota < 1"; return false; }
    if ((long long)a.rows * a.cols * a.quota > LVK_MAP_MAX_QUERIES) { *why = "rows * cols * quota > 1024"; return false; }
    a.pad = 0;
    *o = a;
    return true;
}

// rows * cols * quota of the options as lvk_map_select_queries reads them (-1: it refuses them): the records a caller must have room for
int fe_map_max_selected(const lvk_map_select_options* opt)
{
    lvk_map_select_options o; const char* why = "";
    return map_options(opt, &o, &why) ? o.rows * o.cols * o.quota : -1;
}

extern "C" lvk_status lvk_map_select_queries(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, int n, const lvk_map_camera* cam,
                                             const lvk_align_result* align, const double* R_wc, const double* p_wc, const double* cov_cam,
                                             const lvk_map_select_options* opt, lvk_map_sel* d_sel, lvk_match_query* d_q, uint8_t* d_q_desc, lvk_map_info* d_info,
                                             uint8_t* d_status)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: negative count (n %d)", n);
    if (!cam || !R_wc || !p_wc || !d_info || (n > 0 && (!d_X || !d_sel || !d_q || (d_desc && !d_q_desc)))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: null pointer");
    lvk_map_select_options o; const char* why = "";
    if (!map_options(opt, &o, &why)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: %s", why);
    if (!map_finite(R_wc, 9) || !map_finite(p_wc, 3)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: R_wc or p_wc is not finite");
    if (align && !(std::isfinite(align->c) && std::isfinite(align->s) && map_finite(align->t, 3))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: the alignment is not finite");
    if (!map_finite(cam->intr, 4) || !map_finite(cam->dist, 4)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: the camera is not finite");
    if (cam->model != 0 && cam->model != 1) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: model %d (0 radtan, 1 equidistant)", cam->model);
    if (cam->width < 1 || cam->height < 1) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: a %d x %d image", cam->width, cam->height);
    if (d_desc && ((((uintptr_t)d_desc) | ((uintptr_t)d_q_desc)) & 7u)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_select_queries: descriptors must be 8-byte aligned");
    if (n > LVK_MAP_MAX_POINTS) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_map_select_queries: %d points, at most %d", n, LVK_MAP_MAX_POINTS);
    if (n == 0) { LVK_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(lvk_map_info), ctx->stream)); return LVK_OK; }

    MapArgs a;
    memset(&a, 0, sizeof a);
    a.c = 1.;
    if (align) { a.c = align->c; a.s = align->s; memcpy(a.t, align->t, sizeof a.t); }
    memcpy(a.Rwc, R_wc, sizeof a.Rwc); memcpy(a.p, p_wc, sizeof a.p);
    for (int j = 0; j < 3; ++j) { a.R[j] = a.c * R_wc[j] + a.s * R_wc[3 + j]; a.R[3 + j] = a.c * R_wc[3 + j] - a.s * R_wc[j]; a.R[6 + j] = R_wc[6 + j]; }
    if (cov_cam) { memcpy(a.C, cov_cam, sizeof a.C); a.has_cov_cam = 1; }
    for (int k = 0; k < 4; ++k) { a.cam.intr[k] = cam->intr[k]; a.cam.dist[k] = cam->dist[k]; }
    a.cam.model = cam->model; a.cam.width = cam->width; a.cam.height = cam->height;
    a.min_depth = o.min_depth; a.max_depth = o.max_depth; a.max_r2 = o.max_r2; a.margin = o.margin;
    a.hi_x = (double)(cam->width - 1) - o.margin; a.hi_y = (double)(cam->height - 1) - o.margin;
    a.k_sigma = o.k_sigma; a.sigma2 = o.sigma_px * o.sigma_px; a.r_min = o.r_min; a.r_max = o.r_max;
    a.rows = o.rows; a.cols = o.cols; a.quota = o.quota;

    const int n_chunks = (n + MAP_CHUNK - 1) / MAP_CHUNK, n_cells = o.rows * o.cols;
    // the work buffer: the table, the cells' offsets, the points' codes
    const size_t table_bytes = sizeof(int) * (size_t)(n_cells + MAP_OTHER) * n_chunks, base_bytes = sizeof(int) * MAP_MAX_CELLS;
    uint8_t* work = (uint8_t*)lvk_ctx_scratch(ctx, LVK_SCR_MAP_WORK, table_bytes + base_bytes + sizeof(unsigned short) * (size_t)n);
    if (!work) return lvk_set_error(ctx, LVK_ERR_DEVICE, "lvk_map_select_queries: scratch allocation failed");
    int* table = (int*)work; int* cell_base = (int*)(work + table_bytes); unsigned short* code = (unsigned short*)(work + table_bytes + base_bytes);
    hipLaunchKernelGGL(k_map_project, dim3(n_chunks), dim3(MAP_CHUNK), 0, ctx->stream, d_X, n, a, n_chunks, code, table);
    hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(MAP_CHUNK), 0, ctx->stream, table, n_chunks, n_cells, o.quota, cell_base, d_info);
    hipLaunchKernelGGL(k_map_scatter, dim3(n_chunks), dim3(MAP_CHUNK), 0, ctx->stream, d_X, d_cov, reinterpret_cast<const unsigned long long*>(d_desc), n, a, n_chunks,
                       (const unsigned short*)code, (const int*)table, (const int*)cell_base, d_sel, d_q, reinterpret_cast<unsigned long long*>(d_q_desc), d_status);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
