// be_fix.hip — external position and pose fixes: the sparse measurement update (lvk_ekf_update_sparse, include/lvk_c.h: 3 or 6 rows,
// at most 12 columns, a full noise covariance, a chi-square gate decided on the device) with its two kernels, and the filter's fix
// queue (lvk_ekf_add_fix and what goes with it; lvk_ekf_apply_fixes is the stage backend.hip's ekf_process_impl runs).
#include "be_filter.h"
#include "be_host_math.h"
#include <math.h>

#define FX_ROWS 6
#define FX_COLS 12

// First launch, one wavefront per 64 columns of P.  Every workgroup gathers the ncols x ncols sub-block P_s of P and forms
//   T_s = H P_s (m x ncols),   S = T_s H^T + R (upper triangle, mirrored),   S = L L^T,   y = L^-1 r,   gamma = y^T y
// by itself - the same operands in the same order everywhere, so all workgroups hold the same bits and none reads what another
// writes - lane 0 factoring the 6 x 6 at most.  Then lane l takes column j = 64 blockIdx.x + l:
//   t_i = sum_k H[i][k] P[cols[k]][j] (k ascending),   w_i = (t_i - sum_{k<i} L[i][k] w_k) / L[i][i],   dx_j = sum_i w_i y_i,
// W (m x n, row stride n) going to the work space the second launch reads.  A status other than 0 writes dx = 0 and no W.
// info (4 doubles, written by workgroup 0): status, gamma, the smallest pivot, 0.
__global__ __launch_bounds__(64) void k_fix_gain(const double* __restrict__ P, int ld, int n, const lvk_sparse_update* __restrict__ u, double* __restrict__ W,
                                                 double* __restrict__ dx, double* __restrict__ info)
{
    __shared__ double Hs[FX_ROWS * FX_COLS], Ps[FX_COLS * FX_COLS], Ts[FX_ROWS * FX_COLS], S[FX_ROWS * FX_ROWS], Ls[FX_ROWS * FX_ROWS], y[FX_ROWS];
    __shared__ int cs[FX_COLS], status_s;
    const int lane = threadIdx.x, m = u->m, nc = u->ncols;
    if (lane < nc) cs[lane] = u->cols[lane];
    for (int t = lane; t < m * nc; t += 64) Hs[t] = u->H[t];
    __syncthreads();
    for (int t = lane; t < nc * nc; t += 64) Ps[t] = P[(size_t)cs[t / nc] * ld + cs[t % nc]];
    __syncthreads();
    for (int t = lane; t < m * nc; t += 64) {
        const int i = t / nc, l = t % nc;
        double s = 0.;
        for (int k = 0; k < nc; ++k) s += Hs[i * nc + k] * Ps[k * nc + l];
        Ts[t] = s;
    }
    __syncthreads();
    if (lane < m * m) {
        const int i = lane / m, j = lane % m;
        if (i <= j) {
            double s = 0.;
            for (int l = 0; l < nc; ++l) s += Ts[i * nc + l] * Hs[j * nc + l];
            s = s + u->R[i * m + j];
            S[i * m + j] = s; S[j * m + i] = s;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int status = 0;
        double pmin = 0., gamma = 0.;
        for (int j = 0; j < m; ++j) {
            double d = S[j * m + j];
            for (int k = 0; k < j; ++k) d -= Ls[j * m + k] * Ls[j * m + k];
            if (!(d > 0.)) { status = 2; pmin = d; break; }              // (a NaN lands here too)
            if (j == 0 || d < pmin) pmin = d;
            const double ljj = sqrt(d);
            Ls[j * m + j] = ljj;
            for (int i = j + 1; i < m; ++i) {
                double s = S[i * m + j];
                for (int k = 0; k < j; ++k) s -= Ls[i * m + k] * Ls[j * m + k];
                Ls[i * m + j] = s / ljj;
            }
        }
        if (status == 0) {
            for (int i = 0; i < m; ++i) {
                double s = u->r[i];
                for (int k = 0; k < i; ++k) s -= Ls[i * m + k] * y[k];
                y[i] = s / Ls[i * m + i];
            }
            for (int i = 0; i < m; ++i) gamma += y[i] * y[i];
            const double gate = u->gate;
            if (gate > 0. && !(gamma <= gate)) status = 1;
        }
        status_s = status;
        if (blockIdx.x == 0) { info[0] = (double)status; info[1] = gamma; info[2] = pmin; info[3] = 0.; }
    }
    __syncthreads();
    const int j = blockIdx.x * 64 + lane;
    if (j >= n) return;
    if (status_s != 0) { dx[j] = 0.; return; }
    double p[FX_COLS], w[FX_ROWS];
#pragma unroll
    for (int k = 0; k < FX_COLS; ++k) p[k] = k < nc ? P[(size_t)cs[k] * ld + j] : 0.;
    double d = 0.;
#pragma unroll
    for (int i = 0; i < FX_ROWS; ++i) {
        if (i < m) {
            double s = 0.;
#pragma unroll
            for (int k = 0; k < FX_COLS; ++k) if (k < nc) s += Hs[i * nc + k] * p[k];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= Ls[i * m + k] * w[k];
            w[i] = s / Ls[i * m + i];
            W[(size_t)i * n + j] = w[i];
            d += w[i] * y[i];
        }
    }
    dx[j] = d;
}

// Second launch: P[a][b] <- P[a][b] - sum_i W[i][a] W[i][b] (i ascending), one entry per thread and four rows per thread; (a, b) and
// (b, a) multiply the same pairs in the same order.  Nothing happens unless the first launch reported status 0.
__global__ __launch_bounds__(256) void k_fix_downdate(double* __restrict__ P, int ld, int n, int m, const double* __restrict__ W, const double* __restrict__ info)
{
    if (info[0] != 0.) return;                          // (uniform over the grid)
    const int b = blockIdx.x * 64 + threadIdx.x, a0 = (blockIdx.y * 4 + threadIdx.y) * 4;
    if (b >= n) return;
    double wb[FX_ROWS];
#pragma unroll
    for (int i = 0; i < FX_ROWS; ++i) wb[i] = i < m ? W[(size_t)i * n + b] : 0.;
    for (int q = 0; q < 4; ++q) {
        const int a = a0 + q;
        if (a >= n) return;
        double s = 0.;
#pragma unroll
        for (int i = 0; i < FX_ROWS; ++i) if (i < m) s += W[(size_t)i * n + a] * wb[i];
        P[(size_t)a * ld + b] = P[(size_t)a * ld + b] - s;
    }
}

// what the kernels assume of one record on an n x n covariance
static const char* sparse_update_flaw(const lvk_sparse_update* u, int n)
{
    if (u->m != 3 && u->m != 6) return "m is not 3 or 6";
    if (u->ncols < 1 || u->ncols > FX_COLS) return "ncols is outside 1..12";
    for (int k = 0; k < u->ncols; ++k) {
        if (u->cols[k] < 0 || u->cols[k] >= n) return "a column lies outside [0, n)";
        if (k > 0 && u->cols[k] <= u->cols[k - 1]) return "the columns do not ascend";
    }
    if (!std::isfinite(u->gate)) return "the gate is not finite";
    for (int i = 0; i < u->m * u->ncols; ++i) if (!std::isfinite(u->H[i])) return "an entry of H is not finite";
    for (int i = 0; i < u->m; ++i) {
        if (!std::isfinite(u->r[i])) return "an entry of r is not finite";
        for (int j = i; j < u->m; ++j) if (!std::isfinite(u->R[i * u->m + j])) return "an entry of R is not finite";
    }
    return nullptr;
}

// (C ABI) the record goes up in the stage's input blob, W lives in its work space, dx and the report come back through its output
// blob; both launches are queued at once and the call waits once
extern "C" lvk_status lvk_ekf_update_sparse(lvk_context* ctx, double* d_P, int ldp, int n, const lvk_sparse_update* h_u, double* h_dx, double* h_info4)
{
    if (!ctx || !d_P || !h_u || !h_dx || !h_info4 || n <= 0 || ldp < n) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_update_sparse: bad argument");
    if (const char* flaw = sparse_update_flaw(h_u, n)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_ekf_update_sparse: %s (m %d, ncols %d, n %d)", flaw, h_u->m, h_u->ncols, n);
    const int m = h_u->m;
    const size_t dxb = sizeof(double) * (size_t)n;
    Stage sg(ctx);
    const size_t o_u = sg.take(Stage::IN, sizeof *h_u), o_w = sg.take(Stage::MID, sizeof(double) * (size_t)m * n);
    const size_t o_dx = sg.take(Stage::OUT, dxb), o_info = sg.take(Stage::OUT, 4 * sizeof(double));
    LVK_TRY(sg.alloc());
    LVK_TRY(sg.put(Stage::IN, o_u, h_u, sizeof *h_u));
    double* W = sg.at<double>(Stage::MID, o_w); double* info = sg.at<double>(Stage::OUT, o_info);
    hipLaunchKernelGGL(k_fix_gain, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_P, ldp, n, sg.at<lvk_sparse_update>(Stage::IN, o_u), W, sg.at<double>(Stage::OUT, o_dx), info);
    LVK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_fix_downdate, dim3((n + 63) / 64, (n + 15) / 16), dim3(64, 4), 0, ctx->stream, d_P, ldp, n, m, W, info);
    LVK_LAUNCH_CHECK(ctx);
    LVK_TRY(sg.get(h_dx, Stage::OUT, o_dx, dxb));
    LVK_TRY(sg.get(h_info4, Stage::OUT, o_info, 4 * sizeof(double)));
    return sg.wait();
}

// ------------------------------------------------------------------------- the filter's fix queue
// lower Cholesky factor of the leading m x m block of a row-major matrix of row stride ld: does it exist, and is the block symmetric
static bool spd_block(const double* A, int ld, int m)
{
    double L[36];
    for (int i = 0; i < m; ++i) for (int j = 0; j < i; ++j) if (A[i * ld + j] != A[j * ld + i]) return false;
    for (int j = 0; j < m; ++j) {
        double d = A[j * ld + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.)) return false;
        L[j * 6 + j] = sqrt(d);
        for (int i = j + 1; i < m; ++i) { double s = A[i * ld + j]; for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k]; L[i * 6 + j] = s / L[j * 6 + j]; }
    }
    return true;
}
static void fix_report(lvk_ekf* e, const lvk_fix& f, int status, double gamma, long long ci, long long cj, double a)
{
    lvk_fix_report r; r.tag = f.tag; r.kind = f.kind; r.status = status; r.gamma = gamma; r.clone_i = ci; r.clone_j = cj; r.a = a;
    drain_append(e->fix_reports, r);
    e->fix_stats[1 + status]++;
}
// the rows of one fix on clone i (and, interpolated, its newer neighbour j with weight a): columns, H, r, R of the sparse update
static void fix_rows(const lvk_ekf* e, const lvk_fix& f, int i, int j, double a, lvk_sparse_update* u)
{
    const bool pose = f.kind == LVK_FIX_POSE;
    const int m = pose ? 6 : 3, nc = j >= 0 ? 12 : 6, row0 = pose ? 3 : 0;
    memset(u, 0, sizeof *u);
    u->m = m; u->ncols = nc;
    double pred[3] = {0, 0, 0};
    for (int s = 0; s < (j >= 0 ? 2 : 1); ++s) {
        const int rank = s ? j : i;
        const double wgt = j >= 0 ? (s ? a : 1.0 - a) : 1.0;
        const Clone& c = e->clones[(size_t)rank];
        double R[9], Rl[3], Sk[9];
        quat_to_rot(c.q, R); m3_v(R, f.lever, Rl); skew3(Rl, Sk);
        for (int k = 0; k < 6; ++k) u->cols[6 * s + k] = e->leg + 6 * rank + k;
        for (int x = 0; x < 3; ++x) {
            pred[x] += wgt * (c.p[x] + Rl[x]);
            for (int k = 0; k < 3; ++k) u->H[(row0 + x) * nc + 6 * s + k] = wgt * -Sk[x * 3 + k];      // H_theta = -[R l]x
            u->H[(row0 + x) * nc + 6 * s + 3 + x] = wgt;                                                 // H_p = I
        }
    }
    for (int x = 0; x < 3; ++x) u->r[row0 + x] = f.p[x] - pred[x];
    if (pose) {
        const Clone& c = e->clones[(size_t)i];
        const double qi[4] = {-c.q[0], -c.q[1], -c.q[2], c.q[3]};
        double dq[4]; quat_mul(f.q, qi, dq);
        const double sg = dq[3] < 0 ? -2.0 : 2.0;
        for (int x = 0; x < 3; ++x) { u->r[x] = sg * dq[x]; u->H[x * nc + x] = 1.0; }
    }
    for (int x = 0; x < m; ++x) for (int z = 0; z < m; ++z) u->R[x * m + z] = f.cov[x * 6 + z];
    u->gate = e->fix_gate_scale > 0 ? e->fix_gate_scale * lvk_chi2_005(m) : 0.0;
}
// The queue, in order: every fix whose clone can be named is consumed - applied through lvk_ekf_update_sparse and the injection, or
// reported with the reason it was not - and one that is newer than the newest clone waits for a later message.
lvk_status lvk_ekf_apply_fixes(lvk_ekf* e)
{
    std::vector<lvk_fix> waiting;
    std::vector<double> dx;
    for (const lvk_fix& f : e->fix_queue) {
        const int nc = (int)e->clones.size();
        int i = -1, j = -1; double a = 0.0; int miss = -1;
        if (nc == 0) { waiting.push_back(f); continue; }
        if (f.clone_id >= 0) { i = clone_rank(e, f.clone_id); if (i < 0) miss = LVK_FIX_STALE; }
        else if (f.time < e->clones.front().time) miss = LVK_FIX_STALE;
        else if (f.time > e->clones.back().time) { waiting.push_back(f); continue; }
        else {
            int k = 0;
            while (k + 1 < nc && e->clones[(size_t)k + 1].time <= f.time) ++k;        // the newest clone that is not newer than the fix
            const double ti = e->clones[(size_t)k].time;
            if (ti == f.time) i = k;
            else {
                const double tj = e->clones[(size_t)k + 1].time;
                if (f.kind == LVK_FIX_POSITION && tj - ti <= e->fix_max_gap) { i = k; j = k + 1; a = (f.time - ti) / (tj - ti); }
                else miss = LVK_FIX_NO_CLONE;
            }
        }
        if (miss >= 0) { fix_report(e, f, miss, 0.0, -1, -1, 0.0); continue; }
        lvk_sparse_update u; fix_rows(e, f, i, j, a, &u);
        double info[4] = {0, 0, 0, 0};
        dx.assign((size_t)e->N, 0.0);
        const lvk_status st = lvk_ekf_update_sparse(e->ctx, e->dP[e->cur], e->ld, e->N, &u, dx.data(), info);
        if (st != LVK_OK) return st;
        e->n_sync++;
        const int status = (int)info[0];
        if (status == LVK_FIX_APPLIED) { lvk_ekf_inject(e, dx.data()); e->p00_valid = false; if (j >= 0) e->fix_stats[7]++; }
        fix_report(e, f, status, status == LVK_FIX_NOT_PD ? 0.0 : info[1], e->clones[(size_t)i].id, j >= 0 ? e->clones[(size_t)j].id : -1, a);
    }
    e->fix_queue.swap(waiting);
    return LVK_OK;
}

extern "C" {

lvk_status lvk_ekf_add_fix(lvk_ekf* e, const lvk_fix* f)
{
    if (!e || !f) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_add_fix: bad argument");
    // "pending" = queued and not yet waited for, whether or not the worker has finished meanwhile (as lvk_ekf_set_cov): the update
    // consumes the queue as it was when it was issued
    if (e->async && e->async->unwaited) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: an update is in flight (lvk_ekf_wait first)");
    ekf_quiesce(e);
    if (e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_ekf_add_fix: the sharded update does not apply fixes (lvk_ekf_set_shard is set)");
    if (f->kind != LVK_FIX_POSITION && f->kind != LVK_FIX_POSE) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: kind %d is neither LVK_FIX_POSITION nor LVK_FIX_POSE", f->kind);
    if (f->clone_id < -1) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: clone_id %lld", (long long)f->clone_id);
    const int m = f->kind == LVK_FIX_POSE ? 6 : 3;
    bool finite = std::isfinite(f->time);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(f->p[k]) && std::isfinite(f->lever[k]);
    for (int x = 0; x < m; ++x) for (int z = 0; z < m; ++z) finite = finite && std::isfinite(f->cov[x * 6 + z]);
    if (m == 6) for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(f->q[k]);
    if (!finite) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: a value is not finite");
    if (m == 6 && !(fabs(sqrt(f->q[0] * f->q[0] + f->q[1] * f->q[1] + f->q[2] * f->q[2] + f->q[3] * f->q[3]) - 1.0) <= 1e-6))
        return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: q is not a unit quaternion");
    if (!spd_block(f->cov, 6, m)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_ekf_add_fix: the %d x %d block of cov is not symmetric positive definite", m, m);
    if (e->fix_queue.size() >= (size_t)lvk_ekf::FIX_CAP) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "lvk_ekf_add_fix: %d fixes wait already", (int)lvk_ekf::FIX_CAP);
    e->fix_queue.push_back(*f);
    e->fix_stats[0]++;
    return LVK_OK;
}
lvk_status lvk_ekf_set_fix_options(lvk_ekf* e, double gate_scale, double max_gap_s)
{
    if (!e || std::isnan(gate_scale) || !(max_gap_s >= 0.0)) return lvk_set_error(e ? e->ctx : nullptr, LVK_ERR_ARG, "lvk_ekf_set_fix_options: bad argument");
    ekf_quiesce(e);
    e->fix_gate_scale = gate_scale; e->fix_max_gap = max_gap_s;
    return LVK_OK;
}
int lvk_ekf_take_fix_reports(lvk_ekf* e, lvk_fix_report* out, int cap)
{
    if (!e || !out || cap <= 0) return 0;
    ekf_quiesce(e);
    const int n = std::min((int)e->fix_reports.size(), cap);
    std::copy(e->fix_reports.begin(), e->fix_reports.begin() + n, out);
    e->fix_reports.erase(e->fix_reports.begin(), e->fix_reports.begin() + n);
    return n;
}
void lvk_ekf_fix_stats(const lvk_ekf* e, long* out8)
{
    if (!e || !out8) return;
    ekf_quiesce(e);
    memcpy(out8, e->fix_stats, sizeof e->fix_stats);
    out8[6] = (long)e->fix_queue.size();
}

}  // extern "C"
