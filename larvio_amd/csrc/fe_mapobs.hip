// fe_mapobs.hip — from the matcher's records to the filter's observation rows, on the device, for gfx950 (wave64): the OK records of
// lvk_frontend_match_map gather their map point and its covariance from the resident map, take both into the world frame by the map's
// alignment and fill lvk_landmark_obs rows, in the records' order.  No reference counterpart.  include/lvk_c.h states the definition
// (lvk_map_gather_obs); every expression here is written in the order stated there, FP64, no contraction.
// One workgroup, one lane per record (at most 1024).  A lane keeps its record when the match is OK and the map index lies inside the
// map - an index is compared before it is followed, a record that fails is counted and reads nothing.  The output position comes from
// wave ballots (the kept lanes below this one in its wavefront) and a scan of the wavefronts' counts in LDS: the order is the records'
// own, nothing depends on the order in which anything ran, no atomics.
#include "lvk_internal.h"
#include "fe_frontend.h"
#include <cmath>

#define MO_MAX   LVK_MAP_MAX_QUERIES
#define MO_WAVES (MO_MAX / 64)

struct MapObsArgs { double c, s, t[3], sigma; int n_rec, n_map; };

__global__ void __launch_bounds__(MO_MAX) k_map_gather_obs(const char* __restrict__ idx_base, int idx_stride, const char* __restrict__ m_base, int m_stride, MapObsArgs a,
                                                          const double* __restrict__ X, const double* __restrict__ cov, lvk_landmark_obs* __restrict__ obs,
                                                          int* __restrict__ idx, lvk_map_obs_info* __restrict__ info)
{
    __shared__ int s_ok[MO_WAVES], s_bad[MO_WAVES];
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6, n_waves = blockDim.x >> 6;
    bool ok = false, bad = false;
    int index = 0;
    float und_x = 0.f, und_y = 0.f;
    if (k < a.n_rec) {
        const lvk_landmark_match* m = reinterpret_cast<const lvk_landmark_match*>(m_base + (size_t)k * m_stride);
        if (m->status == LVK_MATCH_OK) {
            index = *reinterpret_cast<const int*>(idx_base + (size_t)k * idx_stride);
            ok = index >= 0 && index < a.n_map;
            bad = !ok;
            und_x = m->und.x; und_y = m->und.y;
        }
    }
    const unsigned long long b_ok = __ballot(ok), b_bad = __ballot(bad);
    if (lane == 0) { s_ok[wave] = __popcll(b_ok); s_bad[wave] = __popcll(b_bad); }
    __syncthreads();
    if (ok) {
        int pos = __popcll(b_ok & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += s_ok[w];
        const double x0 = X[3 * (size_t)index], x1 = X[3 * (size_t)index + 1], x2 = X[3 * (size_t)index + 2];
        const double c = a.c, s = a.s;
        const double q0 = c * x0 - s * x1, q1 = s * x0 + c * x1;
        lvk_landmark_obs o;
        o.p_w[0] = q0 + a.t[0]; o.p_w[1] = q1 + a.t[1]; o.p_w[2] = x2 + a.t[2];
        if (cov) {
            const double* S = cov + 9 * (size_t)index;
            const double sa = S[0], sb = S[1], sd = S[4], se = S[2], sf = S[5], sg = S[8];      // the upper triangle
            const double m00 = c * sa - s * sb, m01 = c * sb - s * sd, m10 = s * sa + c * sb, m11 = s * sb + c * sd;
            const double w00 = m00 * c - m01 * s, w01 = m00 * s + m01 * c, w11 = m10 * s + m11 * c;
            const double w02 = c * se - s * sf, w12 = s * se + c * sf;
            o.cov_w[0] = w00; o.cov_w[1] = w01; o.cov_w[2] = w02;
            o.cov_w[3] = w01; o.cov_w[4] = w11; o.cov_w[5] = w12;
            o.cov_w[6] = w02; o.cov_w[7] = w12; o.cov_w[8] = sg;
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) o.cov_w[e] = 0.;
        }
        o.uv[0] = (double)und_x; o.uv[1] = (double)und_y;
        o.sigma = a.sigma;
        obs[pos] = o;
        idx[pos] = k;
    }
    if (k == 0) {
        lvk_map_obs_info r;
        r.n_ok = 0; r.n_bad = 0; r.pad[0] = 0; r.pad[1] = 0;
        for (int w = 0; w < n_waves; ++w) { r.n_ok += s_ok[w]; r.n_bad += s_bad[w]; }
        *info = r;
    }
}

// (everything is checked by the callers: lvk_map_gather_obs below, lvk_frontend_localise_obs behind lvk_map_select_queries' own checks)
lvk_status fe_map_gather_launch(lvk_context* ctx, const void* idx_base, int idx_stride, const void* m_base, int m_stride, int n_rec, const double* d_X, const double* d_cov,
                                int n_map, const lvk_align_result* align, double sigma, lvk_landmark_obs* d_obs, int* d_idx, lvk_map_obs_info* d_info)
{
    if (n_rec < 1 || n_rec > MO_MAX) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_map_gather_obs: %d records, at most %d", n_rec, MO_MAX);
    MapObsArgs a;
    a.c = align ? align->c : 1.0; a.s = align ? align->s : 0.0;
    for (int i = 0; i < 3; ++i) a.t[i] = align ? align->t[i] : 0.0;
    a.sigma = sigma; a.n_rec = n_rec; a.n_map = n_map;
    hipLaunchKernelGGL(k_map_gather_obs, dim3(1), dim3((n_rec + 63) / 64 * 64), 0, ctx->stream, (const char*)idx_base, idx_stride, (const char*)m_base, m_stride, a, d_X, d_cov,
                       d_obs, d_idx, d_info);
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}

extern "C" lvk_status lvk_map_gather_obs(lvk_context* ctx, const lvk_map_match* d_rec, int n_rec, const double* d_X, const double* d_cov, int n_map,
                                         const lvk_align_result* align, double sigma, lvk_landmark_obs* d_obs, int* d_idx, lvk_map_obs_info* d_info)
{
    if (!ctx) return LVK_ERR_ARG;
    if (n_rec < 0 || n_map < 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_gather_obs: negative count (n_rec %d, n_map %d)", n_rec, n_map);
    if (!d_info || (n_rec > 0 && (!d_rec || !d_obs || !d_idx || (n_map > 0 && !d_X)))) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_gather_obs: null pointer");
    if (align && !(std::isfinite(align->c) && std::isfinite(align->s) && std::isfinite(align->t[0]) && std::isfinite(align->t[1]) && std::isfinite(align->t[2])))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_gather_obs: the alignment is not finite");
    if (!std::isfinite(sigma) || !(sigma > 0.)) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_map_gather_obs: sigma is not a finite number > 0");
    if (n_rec > MO_MAX) return lvk_set_error(ctx, LVK_ERR_CAPACITY, "lvk_map_gather_obs: %d records, at most %d", n_rec, MO_MAX);
    if (n_rec == 0) { LVK_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(lvk_map_obs_info), ctx->stream)); return LVK_OK; }
    return fe_map_gather_launch(ctx, &d_rec->index, (int)sizeof(lvk_map_match), &d_rec->m, (int)sizeof(lvk_map_match), n_rec, d_X, d_cov, n_map, align, sigma, d_obs, d_idx, d_info);
}
