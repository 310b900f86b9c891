// lvk_internal.h — shared internals of liblvk_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/lvk_c.h"

// spin-wait hint of a host thread (x86 pause; nothing elsewhere)
#if defined(__x86_64__) || defined(__i386__)
#define LVK_CPU_RELAX() __builtin_ia32_pause()
#else
#define LVK_CPU_RELAX() do { } while (0)
#endif

// store fence after host writes that a kernel launched next must see (write-combined BAR mappings: sfence on x86)
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#define LVK_STORE_FENCE() _mm_sfence()
#else
#define LVK_STORE_FENCE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#endif

// May this process push host writes into device memory through the PCIe BAR on `device`?  lvk_context.hip: LVK_BAR_PUSH=0 says no; a
// device without a large BAR says no; otherwise a self-test decides, once per device and process - the host writes a pattern into a
// fine-grained device buffer, a kernel reads it, the host REWRITES the same addresses, a second kernel reads again: a stale second
// read (L2 lines of the first read surviving the kernel boundary under this driver's MTYPE / partition settings) says no.
bool lvk_bar_usable(int device);

// Device memory that the HOST writes through the PCIe BAR (the filter's upload arena, the blocking front-end's image buffers): a
// fine-grained device allocation when the device reports a large BAR AND the process really has a writable mapping of it (checked in
// /proc/self/maps: a container may hide what the attribute promises); nullptr otherwise - callers then keep their pinned-host path.
static inline void* lvk_bar_alloc(int device, size_t bytes)
{
    void* p = nullptr;
    if (!lvk_bar_usable(device)) return nullptr;
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
    bool writable = false;
    if (FILE* f = fopen("/proc/self/maps", "r")) {
        char line[512]; unsigned long lo = 0, hi = 0; char perm[8] = {0};
        while (fgets(line, sizeof line, f))
            if (sscanf(line, "%lx-%lx %7s", &lo, &hi, perm) == 3 && (unsigned long)p >= lo && (unsigned long)p < hi) { writable = perm[0] == 'r' && perm[1] == 'w'; break; }
        fclose(f);
    }
    if (!writable) { (void)hipFree(p); return nullptr; }
    return p;
}

#define LVK_MAX_LEVELS 8
#define LVK_ORB_BORDER 32

// Scratch slots of a context (lvk_ctx_scratch): one name per user, or per group of users that share a buffer on purpose.
// Sharing is safe under one rule: every user of a shared slot ends with a wait for the context's stream (or, where it returns with work
// still queued, is followed on that stream by whatever reuses the buffer), and lvk_ctx_scratch waits for the stream before it frees a
// buffer to grow it - so no two users ever have work in flight on one buffer.
enum lvk_scratch_slot {
    LVK_SCR_CLAHE_LUT,                  // front-end: CLAHE look-up tables
    LVK_SCR_GFTT_EIG,                   // corner selection, stage entry: response map
    LVK_SCR_GFTT_WORK,                  // corner selection: counters and bins
    LVK_SCR_GFTT_CANDS,                 // corner selection: candidate keys
    LVK_SCR_UPDATE_B,                   // measurement update: B = [H P | r]
    LVK_SCR_UPDATE_S,                   // measurement update: S
    LVK_SCR_UPDATE_SP,                  // measurement update: S as partial planes, one per block of state columns (k_hp_splanes)
    LVK_SCR_UPDATE_INFO,                // measurement update: the factorisation's report words
    LVK_SCR_QR_H, LVK_SCR_QR_R,         // shared by the grouped-QR stage entry (ping-pong copy of H, r) and CAQR (V, T): one runs after the other on the stream
    LVK_SCR_STAGE_IN, LVK_SCR_STAGE_MID, LVK_SCR_STAGE_OUT,   // shared by every stage entry (input blob, staging, output blob): each ends with a stream wait
    LVK_SCR_CHOL_WS,                    // fused Cholesky: diagonal-block inverses and the panel flag (lvk_context::chol_epoch)
    LVK_SCR_LDLT_WS,                    // LDL^T update: pivot-ordered copies of [HP | r] and X, D, the permutation, the counters
    LVK_SCR_MATCH_CLAIM,                // guided ORB matching: one claim word per candidate
    LVK_SCR_ALIGN_HYP,                  // two-point alignment: the hypothesis records when the caller keeps none
    LVK_SCR_MAP_WORK,                   // prior-map selection: the chunk x cell table, the cells' offsets, the points' status and cell
    LVK_SCR_GLOBAL_WORK,                // global ORB search: the slices x corners table of key pairs, then one claim word per map point.  Its own slot, shared with nobody:
                                        // the four launches of a call follow one another on the context's stream, and so does the next call
    LVK_SCR_MAPBUILD_WORK,              // map build: the sort's two key and index arrays, the scores' bits, the digit x chunk and status x chunk tables, the status bytes.
                                        // Its own slot: a call's launches follow one another on the context's stream, and so does the next call
    LVK_SCR_ALIGN3D_HYP,                // 3D-3D alignment: the hypothesis records when the caller keeps none
    LVK_SCRATCH_SLOTS
};
#define LVK_LDS_OPTIN_KERNELS 24        // kernels that ask for more dynamic LDS than the default (fewer than that today)
struct lvk_context {
    int device;
    hipStream_t stream;
    bool own_stream;
    char err[512];
    // grow-only scratch buffers for the stage-level entry points (no stream-ordered pool: a fresh
    // pool block handed out mid-stream was observed to corrupt an in-flight launch sequence)
    void* scratch[LVK_SCRATCH_SLOTS];
    size_t scratch_bytes[LVK_SCRATCH_SLOTS];
    // dynamic-LDS opt-ins (hipFuncAttributeMaxDynamicSharedMemorySize) already made through THIS context: function attributes are
    // per device, so the cache lives here and not in a process-wide static.  Keyed on the kernel's function pointer, filled in order
    // of first use, searched linearly: two kernels cannot share an entry
    struct { const void* fn; size_t bytes; } lds_optin[LVK_LDS_OPTIN_KERNELS];
    // fused Cholesky + solve (be_linalg.hip, k_chol_fused): the factor workgroup hands panels to the solver workgroups through a flag
    // that only ever grows; chol_epoch numbers the launches, chol_ws (LVK_SCR_CHOL_WS) holds the diagonal-block inverses and the flag
    int chol_epoch;
};
// the bytes this context has already opted `fn` in to (a fresh entry: 0); nullptr when the table is full - the caller then opts in uncached
static inline size_t* lvk_lds_optin_entry(lvk_context* ctx, const void* fn)
{
    for (int i = 0; i < LVK_LDS_OPTIN_KERNELS; ++i) {
        if (ctx->lds_optin[i].fn == fn) return &ctx->lds_optin[i].bytes;
        if (!ctx->lds_optin[i].fn) { ctx->lds_optin[i].fn = fn; return &ctx->lds_optin[i].bytes; }
    }
    return nullptr;
}
// opt in to `bytes` of dynamic LDS for `fn` if this context has not already asked for at least that much
#define LVK_LDS_OPTIN(ctx, fn, bytes)                                                                                   \
    do {                                                                                                                \
        size_t* have_ = lvk_lds_optin_entry((ctx), (const void*)(fn));                                                  \
        if (!have_ || *have_ < (size_t)(bytes)) {                                                                       \
            LVK_HIP(ctx, hipFuncSetAttribute((const void*)(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            if (have_) *have_ = (size_t)(bytes);                                                                        \
        }                                                                                                               \
    } while (0)
void* lvk_ctx_scratch(lvk_context* ctx, int slot, size_t bytes);
struct lvk_pyramid;
lvk_status lvk_pyramid_build_with_orb(lvk_context* ctx, lvk_pyramid* p, const uint8_t* d_img, int stride, int clahe, double clip_limit,
                                      int tiles_x, int tiles_y, uint8_t* d_ext, int* mosaic_done);
lvk_status lvk_orb_blur_only(lvk_context* ctx, const lvk_pyramid* p, const uint8_t* d_ext, uint8_t* d_blur);
// corner selection (fe_image.hip), as the front-end queues it
lvk_status lvk_gftt_run(lvk_context* ctx, const float* d_eig, const uint8_t* d_mask, int w, int h, int max_corners,
                        double quality, double min_distance, unsigned* d_scratch, unsigned long long* d_cands, int cand_cap,
                        lvk_pt2f* d_out, int cap, int* d_n_out, const int* d_sub, bool prepared, bool max_done);
lvk_status lvk_mask_and_max(lvk_context* ctx, const lvk_pt2f* d_pts, const int* d_n, int w, int h, int md, const float* d_eig, uint8_t* d_mask, unsigned* d_scratch);
lvk_status lvk_mask_and_max_user(lvk_context* ctx, const lvk_pt2f* d_pts, const int* d_n, int w, int h, int md, const float* d_eig, uint8_t* d_mask, unsigned* d_scratch,
                                 const uint8_t* d_user_mask);      // d_user_mask: packed w x h, 0 / 255 (lvk_frontend_set_mask)
lvk_status lvk_mask_normalise(lvk_context* ctx, const uint8_t* d_src, int stride, int w, int h, uint8_t* d_dst);
struct lvk_frontend;
lvk_context* lvk_frontend_context(lvk_frontend* fe);      // frontend.hip
extern "C" lvk_status lvk_frontend_begin(lvk_frontend* fe, const lvk_image* img, double ts);   // image stage only (internal)
// the pipelined driver's non-blocking processImage: *slot = ring entry of the feature message (when *has_msg), collected later
extern "C" lvk_status lvk_frontend_process_async(lvk_frontend* fe, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* has_msg, int* slot);
// the front-end's part of lvk_vio_localise_map (be_pipe.hip): lvk_frontend_match_map's device chain, lvk_map_gather_obs on its records
// where they lie, one copy back.  h_obs / h_idx: room for LVK_MAP_MAX_QUERIES entries each
extern "C" lvk_status lvk_frontend_localise_obs(lvk_frontend* fe, const lvk_align_result* align, const double* R_wc, const double* p_wc, const double* cov_cam36,
                                                const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, double sigma_px,
                                                lvk_landmark_obs* h_obs, int* h_idx, lvk_map_info* h_info, lvk_map_obs_info* h_oinfo);
extern "C" lvk_status lvk_frontend_fetch_msg(lvk_frontend* fe, int slot, lvk_feature_obs* h_out, int cap, int* n_out);

struct lvk_pyramid {
    lvk_context* ctx;
    int n_levels, pad, max_level;
    int w[LVK_MAX_LEVELS], h[LVK_MAX_LEVELS];
    int istride[LVK_MAX_LEVELS];   // bytes per padded image row
    int dstride[LVK_MAX_LEVELS];   // int16 per padded derivative row
    uint8_t* img[LVK_MAX_LEVELS];  // padded buffers
    int16_t* der[LVK_MAX_LEVELS];
    uint8_t* clahe_lut;            // tiles*256 scratch for the fused CLAHE path
    int clahe_lut_cap;
    hipEvent_t ev_level0;          // optional: recorded on the build stream once level 0 is complete (side streams fork here)
};

// plain-data view of a pyramid passed to kernels by value
struct PyrView {
    int n_levels, pad;
    int w[LVK_MAX_LEVELS], h[LVK_MAX_LEVELS], istride[LVK_MAX_LEVELS], dstride[LVK_MAX_LEVELS];
    const uint8_t* img[LVK_MAX_LEVELS];   // pointer to pixel (0,0) of the level (inside the padded buffer)
    const int16_t* der[LVK_MAX_LEVELS];   // pointer to (Ix,Iy) of pixel (0,0)
};

static inline PyrView make_view(const lvk_pyramid* p)
{
    PyrView v;
    memset(&v, 0, sizeof v);
    v.n_levels = p->n_levels; v.pad = p->pad;
    for (int l = 0; l < p->n_levels; ++l) {
        v.w[l] = p->w[l]; v.h[l] = p->h[l]; v.istride[l] = p->istride[l]; v.dstride[l] = p->dstride[l];
        v.img[l] = p->img[l] + (size_t)p->pad * p->istride[l] + p->pad;
        v.der[l] = p->der[l] + (size_t)p->pad * p->dstride[l] + 2 * p->pad;
    }
    return v;
}

lvk_status lvk_set_error(lvk_context* ctx, lvk_status code, const char* fmt, ...);

#define LVK_HIP(ctx, call)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return lvk_set_error((ctx), LVK_ERR_DEVICE, "%s:%d %s: %s", __FILE__, __LINE__, #call, \
                                 hipGetErrorString(e_));                                      \
    } while (0)

#define LVK_LAUNCH_CHECK(ctx) LVK_HIP(ctx, hipGetLastError())

// n elements of device memory (never an empty allocation)
template <typename T> static bool dalloc(T** p, size_t n) { return hipMalloc((void**)p, sizeof(T) * (n ? n : 1)) == hipSuccess; }

// ---- compile-time instrumentation (make CXXFLAGS+=-DLVK_BE_TIMING; tools/gpu/be_ticks.py): thread 0 of ONE chosen workgroup of a kernel
// stores the 100 MHz wall clock at its phase boundaries into a per-file device array; off, the macros vanish
#ifdef LVK_BE_TIMING
#define BE_TICK_DECL(name) static __device__ unsigned long long name[64]
#define BE_TICK(arr, cond, k) do { if (threadIdx.x == 0 && (cond)) arr[k] = wall_clock64(); } while (0)
#define BE_TICK_GETTER(fn, arr) extern "C" void fn(unsigned long long* out) { hipDeviceSynchronize(); hipMemcpyFromSymbol(out, HIP_SYMBOL(arr), sizeof(unsigned long long) * 64); }
#else
#define BE_TICK_DECL(name)
#define BE_TICK(arr, cond, k) do { } while (0)
#define BE_TICK_GETTER(fn, arr)
#endif

// LK kernel of the frame path (fe_track_dev.h): LVK_LK_VARIANT in the environment, read once per process.  1 = the two-wavefront kernel
// (k_fe_lk_both), 2 = the five-wavefront one (k_fe_lk_pipe), unset or anything else = -1 = the library chooses: the five-wavefront kernel
// up to LVK_LK_PIPE_MAX_TRACKS track slots, the two-wavefront one above - at 2000 tracks five wavefronts and 12 KB of LDS per track no
// longer fit the chip in one round: 100 us against 61, profiles/r6_h_lk_pipe_ab.json.  0 named the two-wavefront kernel with wave-wide
// DPP sums, which is gone: it selects 1, the kernel that replaced it (bench.py labels 0 and 1 alike), never the library's own choice.
#define LVK_LK_PIPE_MAX_TRACKS 600
inline int lvk_lk_variant()
{
    static const int v = [] { const char* e = getenv("LVK_LK_VARIANT"); const int x = e ? atoi(e) : -1; return x < -1 || x > 2 ? -1 : x == 0 ? 1 : x; }();
    return v;
}
#define LK_PIPE_MAX_LEVELS 4            // pyramid levels k_fe_lk_pipe keeps templates for in LDS (LkTplLevel, fe_track_dev.h)
// Which LK kernel the frames of a front-end launch (its patch size, its track slots, the levels of the two pyramids of a frame), and may
// the frame's two track sets share ONE launch.  pipe: k_fe_lk_pipe<21>, otherwise k_fe_lk_both<patch_size>.  merged is opt-in
// (LVK_LK_MERGED=1, read once per process): built and measured in round 6 - bit-exact, and SLOWER in the pipelined driver (10,260 against
// 10,640 frames/s, LK launch 28.2 against 25.9 us: the launch then waits for the previous frame's detection on the side stream, and
// carries twice the blocks), +0.5 % through the adapter's schedule; profiles/r6_o_lk_merged_launch_ab.json
struct LkChoice { bool pipe, merged; };
inline LkChoice lvk_lk_choice(int patch_size, int slots, int levels_prev, int levels_curr)
{
    static const bool merged_on = [] { const char* e = getenv("LVK_LK_MERGED"); return e && !strcmp(e, "1"); }();
    int var = lvk_lk_variant();
    if (var < 0) var = slots <= LVK_LK_PIPE_MAX_TRACKS ? 2 : 1;
    const bool pipe = patch_size == 21 && var == 2 && levels_prev <= LK_PIPE_MAX_LEVELS && levels_curr <= LK_PIPE_MAX_LEVELS;
    return LkChoice{pipe, pipe && merged_on};
}
// cv::calcOpticalFlowPyrLK's termination criteria as it clamps them: the count to [0, 100], epsilon to [0, 10] and squared
struct LkTerm { int max_count; double epsilon; };
inline LkTerm lvk_lk_term(int max_iter, double eps)
{
    const double e = eps < 0. ? 0. : eps > 10. ? 10. : eps;
    return LkTerm{max_iter < 0 ? 0 : max_iter > 100 ? 100 : max_iter, e * e};
}

// ---- device helpers shared by the kernels --------------------------------------------------
__device__ __forceinline__ int d_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) { p = p < 0 ? -p : 2 * len - 2 - p; }
    return p;
}
__device__ __forceinline__ int d_cv_round(float v) { return __float2int_rn(v); }   // half-to-even
__device__ __forceinline__ int d_cv_floor(float v) { return (int)floorf(v); }
__device__ __forceinline__ uint8_t d_sat_u8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// parameter block for the per-point kernels of the frame-level path (device memory, refreshed per frame)
struct CamParams {
    double intr[4];
    double dist[4];
    int model;
    int width, height;
};
