/*
 * lvk_c.h — C ABI of liblvk_hip.so: the MI355X (gfx950) implementation of LARVIO's per-frame
 * hot path (visual front-end + EKF measurement update), the drop-in boundary under the
 * reference's two C++ classes.
 *
 * The reference has no FFI layer; its boundary is larvio::ImageProcessor
 * (/root/reference/include/larvio/image_processor.h:36-68) and larvio::LarVio
 * (include/larvio/larvio.h:37-90), called from app/larvioMain.cpp:107,114.  Each entry point
 * below cites the reference function it replaces.  INTEGRATION.md shows the adapter classes a
 * maintainer compiles against this header so that larvioMain.cpp / System.cpp link unchanged.
 *
 * Conventions
 *  - plain C types only; every function returns lvk_status; no exceptions cross the ABI;
 *  - handle-scoped state, no process globals; lvk_last_error(ctx) gives a message;
 *  - pointers named d_* are DEVICE pointers (hipMalloc / torch data_ptr()); h_* are host;
 *  - stage-level functions are asynchronous on the context's stream unless stated;
 *  - there is NO CPU fallback: without a gfx950 device lvk_context_create fails.
 */
#ifndef LVK_C_H
#define LVK_C_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int lvk_status;
#define LVK_OK              0
#define LVK_ERR_ARG         1   /* bad argument */
#define LVK_ERR_DEVICE      2   /* HIP runtime error / no device */
#define LVK_ERR_CAPACITY    3   /* a fixed capacity was exceeded */
#define LVK_ERR_UNSUPPORTED 4   /* configuration outside what the kernels are built for */
#define LVK_ERR_NUMERIC     5   /* the measurement update met an innovation covariance that is not positive definite: the filter has diverged
                                   (the default; lvk_ekf_set_indefinite_policy(LVK_INDEFINITE_LDLT) goes on as the reference does instead) */

typedef struct lvk_context  lvk_context;
typedef struct lvk_pyramid  lvk_pyramid;
typedef struct lvk_frontend lvk_frontend;

typedef struct { float x, y; } lvk_pt2f;
/* One 8-bit grey image as the reference's ImageData carries it (include/sensors/ImageData.hpp: a cv::Mat knows its own size and
 * step).  stride = bytes between rows (cv::Mat::step); is_device: 0 = data is a host pointer (copied in through the front-end's
 * pinned staging, the caller may reuse the buffer as soon as the call returns), 1 = data is a device pointer.  A front-end switched
 * to another pixel format (lvk_frontend_set_input_format) takes the same struct: data = that format's bytes, stride still in bytes. */
typedef struct { const uint8_t* data; int width, height, stride; int is_device; } lvk_image;
/* include/sensors/ImuData.hpp:17-43 */
typedef struct { double t; double gyro[3]; double acc[3]; } lvk_imu;
/* include/larvio/feature_msg.h:15-44 (MonoFeatureMeasurement, 72 bytes) */
typedef struct {
    uint64_t id;
    double u, v, u_init, v_init, u_vel, v_vel, u_init_vel, v_init_vel;
} lvk_feature_obs;

/* ------------------------------------------------------------------ runtime environment
 * What a deployment should set before the HIP runtime initialises in its process, shipped with the library instead of living in a
 * launcher script: GPU_MAX_HW_QUEUES=8 (one hardware queue per stream of the library and of the application; HIP's default of 4 makes
 * streams share queues: -17 % frames/s), HIP_FORCE_DEV_KERNARG=1 (kernel arguments in device memory), and - opt-in - the calling
 * thread and every thread started after it bound to the physical cores of one L3 group of its socket (local_rank picks the group).
 * Variables already set by the user are respected, with one exception: an explicit call with LVK_RT_HW_QUEUES raises a preset
 * GPU_MAX_HW_QUEUES below 8 to 8 and reports the flag (8 or more is left alone; nothing above 8 is ever written) - the implicit call
 * of lvk_context_create never overrides a variable.  Call it FIRST in main(), before any HIP call of the process; returns the flags
 * that took effect (a variable the user had set, or a call after this library has already initialised the runtime, reports nothing
 * for that flag; the environment is process-wide state: call it before other threads exist).  lvk_context_create applies LVK_RT_DEFAULT by itself (unless LVK_RUNTIME_ENV=0), which suffices when the library
 * is what makes the process's first HIP call.  No reference counterpart: the reference has no device. */
#define LVK_RT_HW_QUEUES   1u
#define LVK_RT_DEV_KERNARG 2u
#define LVK_RT_BIND_L3     4u
#define LVK_RT_DEFAULT     (LVK_RT_HW_QUEUES | LVK_RT_DEV_KERNARG)
unsigned    lvk_runtime_env(unsigned flags, int local_rank);

/* ------------------------------------------------------------------ context / memory */
lvk_status  lvk_context_create(int device, lvk_context** out);
void        lvk_context_destroy(lvk_context* ctx);
/* use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
lvk_status  lvk_context_set_stream(lvk_context* ctx, void* hip_stream);
void*       lvk_context_get_stream(const lvk_context* ctx);   /* the hipStream_t every call on this context is ordered on */
lvk_status  lvk_sync(lvk_context* ctx);
const char* lvk_last_error(const lvk_context* ctx);
const char* lvk_version(void);
/* thin helpers so a host without torch can drive the stage-level API */
lvk_status  lvk_malloc(lvk_context* ctx, size_t bytes, void** d_out);
lvk_status  lvk_free(lvk_context* ctx, void* d_ptr);
lvk_status  lvk_memcpy_h2d(lvk_context* ctx, void* d_dst, const void* h_src, size_t bytes);  /* async */
lvk_status  lvk_memcpy_d2h(lvk_context* ctx, void* h_dst, const void* d_src, size_t bytes);  /* sync  */
lvk_status  lvk_memset(lvk_context* ctx, void* d_dst, int value, size_t bytes);

/* ------------------------------------------------------------------ image passes
 * replaces createImagePyramids (image_processor.cpp:318-334):
 *   cv::createCLAHE(3.0,(8,8))->apply  +  cv::buildOpticalFlowPyramid(win, levels, derivs)
 * and ORBdescriptor::initializeLayerAndPyramid level 0 (ORBDescriptor.cpp:418-484). */
lvk_status lvk_clahe_u8(lvk_context* ctx, const uint8_t* d_src, int w, int h, int sstride,
                        uint8_t* d_dst, int dstride, double clip, int tiles_x, int tiles_y);

lvk_status lvk_pyramid_create(lvk_context* ctx, int w, int h, int win, int max_level, lvk_pyramid** out);
void       lvk_pyramid_destroy(lvk_pyramid* p);
/* level-0 source is d_img (already equalised or raw); builds all levels, padding, Scharr planes */
lvk_status lvk_pyramid_build(lvk_context* ctx, lvk_pyramid* p, const uint8_t* d_img, int stride);
/* fused CLAHE + build (what the frame-level path runs) */
lvk_status lvk_pyramid_build_clahe(lvk_context* ctx, lvk_pyramid* p, const uint8_t* d_img, int stride,
                                   double clip, int tiles_x, int tiles_y);
int        lvk_pyramid_levels(const lvk_pyramid* p);
/* geometry of level l: interior w,h; padded buffers: image row stride (bytes), deriv row stride
 * (int16 units); device base pointers of the PADDED buffers; pad = win */
lvk_status lvk_pyramid_level(const lvk_pyramid* p, int level, int* w, int* h, int* pad,
                             int* istride, int* dstride, const uint8_t** d_img, const int16_t** d_der);
/* ORB level-0 mosaic (border 32) and its 7x7 sigma-2 blurred copy; both (h+64) x (w+64), stride w+64 */
lvk_status lvk_orb_prepare(lvk_context* ctx, const lvk_pyramid* p, uint8_t* d_ext, uint8_t* d_blur);

/* Stage entry: a camera's pixel format to the 8-bit grey plane everything above reads - what the reference's ROS caller gets from
 * cv_bridge::toCvShare(msg, MONO8) (ros_wrapper/src/larvio/src/System.cpp:129) before it calls processImage.  No counterpart in the
 * reference's library itself.  The formulas ARE the contract, in integers:
 *   MONO8          grey = the byte (a strided copy)
 *   BGR8 / RGB8    grey = (1868*B + 9617*G + 4899*R + 8192) >> 14      (the weights sum to 2^14: no saturation is needed)
 *   BGRA8 / RGBA8  the same on B, G, R; the fourth byte is ignored
 *   MONO16         grey = min(255, v >> shift), v a uint16 in host byte order, shift in 0..8
 *   YUYV / UYVY    grey = Y: byte 0 / byte 1 of each 2-byte pixel (Y0 U Y1 V / U Y0 V Y1)
 * The colour line is the scalar 8-bit form OpenCV's 3.4 series documents for cvtColor; later releases use 15-bit constants that differ
 * on rare pixels, and agreement with any OpenCV build is not claimed (PARITY.md).
 * Reads, of source row y (at d_src + y * src_stride_bytes), the bytes [0, w * bytes_per_pixel) and nothing else; writes
 * d_dst[y * dst_stride + x] for x < w and nothing else: padding keeps its bits.  d_src and d_dst may have any byte alignment and any
 * stride that holds a row, except that MONO16 needs an even d_src and src_stride_bytes.  One launch on the context's stream, not waited for.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer, w or h <= 0, an unknown format, src_stride_bytes
 * < w * bytes_per_pixel, dst_stride < w, shift outside 0..8 or non-zero for a format other than MONO16, an odd w for YUYV / UYVY, an
 * odd d_src or src_stride_bytes for MONO16. */
#define LVK_PIX_MONO8  0   /* the front-end's default input */
#define LVK_PIX_BGR8   1
#define LVK_PIX_RGB8   2
#define LVK_PIX_BGRA8  3
#define LVK_PIX_RGBA8  4
#define LVK_PIX_MONO16 5
#define LVK_PIX_YUYV   6
#define LVK_PIX_UYVY   7
lvk_status lvk_image_to_gray(lvk_context* ctx, const void* d_src, int src_stride_bytes, int w, int h,
                             int format, int shift, uint8_t* d_dst, int dst_stride);

/* replaces cv::goodFeaturesToTrack(img, maxCorners, quality, minDistance, mask, 3)
 * (image_processor.cpp:343, 1035-1036).  d_mask may be NULL; d_n_out = device int. */
lvk_status lvk_min_eigen_map(lvk_context* ctx, const lvk_pyramid* p, float* d_eig);
lvk_status lvk_good_features(lvk_context* ctx, const lvk_pyramid* p, const uint8_t* d_mask,
                             int max_corners, double quality, double min_distance,
                             lvk_pt2f* d_out, int cap, int* d_n_out);
/* Stage entry: the selection half of lvk_good_features (masked maximum, threshold at quality * max, 3x3 non-maximum suppression,
 * greedy minDistance pass) on a caller's response map; lvk_good_features is lvk_min_eigen_map followed by this call.
 * Reads d_eig: w * h packed floats (row stride w), and d_mask (may be NULL): w * h packed bytes, any non-zero byte = allowed; neither
 * needs more than its type's alignment.  Writes min(found, cap) corners to d_out, strongest first, and that count to d_n_out.
 * Refusals (the context stays usable): LVK_ERR_ARG for a null ctx / d_eig / d_out / d_n_out, w < 3 or h < 3 (no interior pixel), w * h
 * beyond 2^31 - 1 or cap < 0; LVK_ERR_UNSUPPORTED for a min_distance that is not in 1 .. 32767 (a NaN included) or max_corners outside 1..4096; LVK_ERR_CAPACITY, with nothing
 * launched, when the grid of rint(min_distance)-sized cells does not fit the selection kernel's LDS next to its survivor buffer
 * (8 bytes per cell: about 11,000 cells, e.g. 1000 x 1000 at min_distance 2). */
lvk_status lvk_good_features_from_map(lvk_context* ctx, const float* d_eig, const uint8_t* d_mask, int w, int h,
                                      int max_corners, double quality, double min_distance,
                                      lvk_pt2f* d_out, int cap, int* d_n_out);

/* ------------------------------------------------------------------ per-point stages
 * replaces cv::calcOpticalFlowPyrLK(..., OPTFLOW_USE_INITIAL_FLOW) at
 * image_processor.cpp:368,405,558,618,830,870.  d_next_pts in/out; d_iters optional (n*levels). */
lvk_status lvk_lk_track(lvk_context* ctx, const lvk_pyramid* prev, const lvk_pyramid* next,
                        const lvk_pt2f* d_prev_pts, lvk_pt2f* d_next_pts, uint8_t* d_status, int n,
                        int max_iter, double eps, int* d_iters);
/* replaces ORBdescriptor::computeDescriptors (ORBDescriptor.cpp:386-416); d_desc n*32 bytes */
lvk_status lvk_orb_describe(lvk_context* ctx, const uint8_t* d_ext, const uint8_t* d_blur, int w, int h,
                            const lvk_pt2f* d_pts, int n, uint8_t* d_desc, float* d_angle);
/* replaces ORBdescriptor::computeDescriptorDistance row-wise (ORBDescriptor.h:43-59) */
lvk_status lvk_hamming256_rows(lvk_context* ctx, const uint8_t* d_a, const uint8_t* d_b, int n, int* d_dist);
/* replaces ImageProcessor::undistortPoints (image_processor.cpp:1040-1072); model 0 radtan, 1 equidistant */
lvk_status lvk_undistort_points(lvk_context* ctx, const lvk_pt2f* d_in, int n, const double intr[4], int model,
                                const double dist[4], const double new_intr[4], lvk_pt2f* d_out);
/* replaces cv::findFundamentalMat(p1,p2,FM_RANSAC,thresh,conf,mask) (image_processor.cpp:498,755,968).
 * d_mask n bytes; d_info[0] = 1 if a mask was written (n>=7) else 0, d_info[1] = hypotheses drawn. */
lvk_status lvk_find_fundamental_mask(lvk_context* ctx, const lvk_pt2f* d_p1, const lvk_pt2f* d_p2, int n,
                                     double thresh, double conf, uint8_t* d_mask, int* d_info);
/* the same call where the reference also uses the MATRIX it returns (solve_5pts.cpp:206, the moving-start initialiser's relative pose):
 * d_F (9 doubles, row-major) = the registrator's best minimal-sample model - cv::findFundamentalMat does not refit on the inliers -,
 * all zeros when it has none (OpenCV's empty Mat); n == 7: the first of the solver's up to three models. */
lvk_status lvk_find_fundamental(lvk_context* ctx, const lvk_pt2f* d_p1, const lvk_pt2f* d_p2, int n,
                                double thresh, double conf, uint8_t* d_mask, int* d_info, double* d_F);
/* the RANSAC branch alone for any n >= 8 (stage parity) */
lvk_status lvk_ransac_fundamental(lvk_context* ctx, const lvk_pt2f* d_p1, const lvk_pt2f* d_p2, int n,
                                  double thresh, double conf, int max_iters, uint8_t* d_mask, int* d_info);
/* Stage entry: guided ORB matching - for each of n_q queries (a predicted pixel, a search radius and a 256-bit descriptor) the described
 * corner of the frame that is the query's map point, or the reason there is none.  No reference counterpart: the reference never looks a
 * known point up in a frame.  All integer except the window test, which is float32 exactly as written (no contraction), so every field
 * has one right value:
 *   window     candidate c is in the window of query q iff  dx = cx - qx; dy = cy - qy; dx*dx + dy*dy <= radius*radius.  A NaN anywhere
 *              makes the comparison false (an infinite x or y too: the query then has no candidate; an infinite radius holds every finite
 *              candidate).  n_window = candidates in the window.
 *   best       the in-window candidate with the smallest Hamming distance, ties to the lowest candidate index: cand, dist.
 *   second     the smallest distance over the in-window candidates other than best, -1 when there is none.
 *   status     the first rule that applies: NO_CANDIDATE when n_window == 0 (cand = dist = second = -1); TOO_FAR when dist > max_dist;
 *              AMBIGUOUS when second >= 0 and 100 * dist > ratio_pct * second (ratio_pct 100 switches the test off); otherwise the query
 *              is provisionally matched.  A candidate claimed by several provisionally matched queries goes to the smallest (dist, query
 *              index): that query is OK, the others are CONFLICT, keep their cand and dist and are NOT moved to their second choice.
 * d_cand_pts / d_cand_desc: n_cand points and 32-byte descriptors (lvk_orb_describe's layout); d_q / d_q_desc: n_q queries and their
 * descriptors; d_out: n_q results, pad written as 0.  Both descriptor pointers must be 8-byte aligned.  Two launches (match, then the
 * resolve pass of the claims) behind a clear of the claim words on the context's stream, not waited for.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer where its count is positive, a negative count, max_dist
 * outside 0..256, ratio_pct outside 1..100, a descriptor pointer that is not 8-byte aligned.  LVK_ERR_CAPACITY: n_cand > 4096 (the
 * positions are staged in LDS) or n_q > 1024.  n_q == 0: LVK_OK, nothing launched.  n_cand == 0: every query NO_CANDIDATE. */
#define LVK_MATCH_OK           0
#define LVK_MATCH_NO_CANDIDATE 1
#define LVK_MATCH_TOO_FAR      2
#define LVK_MATCH_AMBIGUOUS    3
#define LVK_MATCH_CONFLICT     4
typedef struct { float x, y, radius, pad; } lvk_match_query;   /* predicted pixel, search radius in pixels */
typedef struct { int cand, dist, second, n_window, status, pad; } lvk_match_result;
lvk_status lvk_orb_match_guided(lvk_context* ctx, const lvk_pt2f* d_cand_pts, const uint8_t* d_cand_desc, int n_cand,
                                const lvk_match_query* d_q, const uint8_t* d_q_desc, int n_q,
                                int max_dist, int ratio_pct, lvk_match_result* d_out);
/* Stage entry: relocalisation against a prior map - the yaw and translation that take a map's frame into the filter's world frame, from
 * n putative 2D-3D matches, many of them wrong, by two-point RANSAC over n_pairs given pairs.  No reference counterpart.  Both frames
 * have z along gravity (roll and pitch are observable in either session), so four numbers are sought: c = cos psi, s = sin psi and t, with
 * p_w = Rz(psi) X + t,  Rz X = (c X_x - s X_y, s X_x + c X_y, X_z).  Match k carries the map point X_k (map frame) and the normalised
 * undistorted observation (u_k, v_k) (lvk_landmark_match.und); R_wc (row-major, camera to world) and p_wc are the camera pose of that image
 * in the filter's world frame; d_k = R_wc (u_k, v_k, 1)^T.  FP64 throughout, no contraction, no atan2 / sin / cos.
 *   solver     pair (i, j): a = X_i - X_j, rho2 = a_x^2 + a_y^2; the constraint is Rz a = l_i d_i - l_j d_j.  p = i when |d_i,z| >= |d_j,z|,
 *              else j, q the other.  No model when i == j, when an index is outside 0..n-1 (nothing is read), when rho2 is not > 0, when
 *              |d_p,z| < min_dz.  The z row gives l_p = alpha + beta l_q:  p = i: alpha = a_z / d_i,z, beta = d_j,z / d_i,z,
 *              e = alpha d_i,xy, f = beta d_i,xy - d_j,xy;  p = j: alpha = -a_z / d_j,z, beta = d_i,z / d_j,z, e = -alpha d_j,xy,
 *              f = d_i,xy - beta d_j,xy.  With w = e + mu f (mu = l_q), |w|^2 = rho2 is A mu^2 + 2 B mu + C = 0, A = f.f, B = e.f,
 *              C = e.e - rho2, disc = B B - A C.  No model unless A > 0 and disc >= 0.  Root 0 is mu = (-B - sqrt(disc)) / A, root 1
 *              mu = (-B + sqrt(disc)) / A; a root is a model iff mu > 0 and l_p > 0.  Its dot = a_xy . w, crs = a_x w_y - a_y w_x,
 *              nrm = sqrt(dot^2 + crs^2), c = dot / nrm, s = crs / nrm, t = (p_wc + l_i d_i) - Rz X_i.  At most two models, root 0 first.
 *   score      match k is an inlier of a model iff p_c = R_wc^T ((Rz X_k + t) - p_wc) has p_c.z > min_depth and
 *              (p_c.x / p_c.z - u_k)^2 + (p_c.y / p_c.z - v_k)^2 <= thresh^2; count = the inliers, the pair's own two included or not as
 *              the test says.
 *   winner     the model with the largest count; ties to the lowest hypothesis index, then to the lower root.  d_mask[k] = 1 for its
 *              inliers, 0 otherwise; the mask is NOT scored again after the refinement (lvk_find_fundamental does not refit either).
 *   refinement Gauss-Newton on (dpsi, dt) over the winner's inliers, minimising sum |r_k|^2, r_k = (p_c.x / p_c.z - u_k, p_c.y / p_c.z - v_k),
 *              from the winner: A = sum J^T J (4 x 4, order psi, t_x, t_y, t_z), g = sum J^T r, A d = -g by Cholesky; t += dt and the yaw by the
 *              half-angle form h = dpsi / 2, (c, s) <- (c, s) rotated by ((1 - h^2) / (1 + h^2), 2 h / (1 + h^2)).  Stop rule: behind the
 *              first step with dpsi^2 + |dt|^2 <= 1e-20, or behind max_refine_iters steps.  A and rms = sqrt(sum |r_k|^2 / n_inliers) are
 *              evaluated at the model that is returned; the caller inverts A and scales by their variance in normalised units - the
 *              library invents no covariance.  A pivot at or below 1e-12 of its diagonal entry of A counts as non-positive (rounding
 *              leaves a rank-deficient A with pivots of either sign at 1e-16 of it).
 *   status     the first rule that applies: NO_MODEL no pair gave a model (hyp = root = pair_i = pair_j = -1, c = c0 = 1, all else 0, mask
 *              zeroed); FEW_INLIERS the best count is below min_inliers (c0, s0, t0 = c, s, t = the winner, the mask is the winner's,
 *              A = rms = iters = 0); SINGULAR the solve met a non-positive pivot (c, s, t = the winner again, A and rms those of the
 *              iterate whose solve failed); OK.
 * d_m: n matches; d_pairs: n_pairs pairs; d_hyp: NULL or n_pairs records - n_models, then the models in root order, slots beyond
 * n_models and both pads zero; d_mask: n bytes; d_out: one record.  Matches beyond n and records beyond n_pairs are not read.  Two
 * launches on the context's stream (hypotheses; arg-max, mask and refinement), not waited for.
 * opt may be NULL; a zero field takes its default: thresh 0.01 (normalised units), min_depth 0.1, min_dz 1e-6, min_inliers 6 (2..1024),
 * max_refine_iters 10 (1..100).  LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed, a
 * negative count, an option that is not finite, not positive or outside its range, a non-finite entry of R_wc or p_wc.
 * LVK_ERR_CAPACITY: n > 1024 (the matches are staged in LDS) or n_pairs > 4096.  n < 2 or n_pairs == 0: NO_MODEL, the mask zeroed,
 * the hypotheses kernel not launched. */
#define LVK_ALIGN_OK          0
#define LVK_ALIGN_NO_MODEL    1
#define LVK_ALIGN_FEW_INLIERS 2
#define LVK_ALIGN_SINGULAR    3
#define LVK_ALIGN_DEFAULT_SEED 0xFFFFFFFFu      /* what a seed of 0 means to lvk_align_draw_pairs */
typedef struct { double X[3]; double u, v; } lvk_align_match;
typedef struct { int i, j; } lvk_align_pair;
typedef struct { int count, root; double c, s, t[3]; } lvk_align_model;
typedef struct { int n_models, pad; lvk_align_model m[2]; } lvk_align_hyp;
typedef struct { double thresh, min_depth, min_dz; int min_inliers, max_refine_iters; } lvk_align_options;   /* zeros = defaults */
typedef struct { int status, n_inliers, hyp, root, pair_i, pair_j, iters, pad;
                 double c, s, t[3];        /* refined */
                 double c0, s0, t0[3];     /* the winner of the minimal solver */
                 double A[16], rms; } lvk_align_result;
lvk_status lvk_align_ransac_2pt(lvk_context* ctx, const lvk_align_match* d_m, int n, const lvk_align_pair* d_pairs, int n_pairs,
                                const double R_wc[9], const double p_wc[3], const lvk_align_options* opt, lvk_align_hyp* d_hyp,
                                uint8_t* d_mask, lvk_align_result* d_out);
/* The pairs lvk_frontend_align_landmarks tries (host only, so that a caller can reproduce them): when n (n - 1) / 2 <= max_hypotheses
 * (0 = the cap, 4096) every pair i < j in lexicographic order; otherwise hypothesis h takes i = r() % n, j = r() % (n - 1), j += (j >= i),
 * r() the low word of x <- (uint32) x * 4164903690 + (x >> 32) (the multiply-with-carry generator of the RANSAC stage), x starting at seed,
 * or at LVK_ALIGN_DEFAULT_SEED for a seed of 0.  Returns the number of pairs written (0 for n < 2; h_pairs holds min(n (n - 1) / 2,
 * max_hypotheses)), -1 for a negative n, max_hypotheses outside 0..4096 or a null pointer. */
int        lvk_align_draw_pairs(int n, int max_hypotheses, uint32_t seed, lvk_align_pair* h_pairs);
/* Stage entry: the per-frame link of that chain - where should each point of a device-resident prior map appear from a pose prediction, how
 * far may the matcher look for it, and which at most 1024 points are worth asking lvk_orb_match_guided about.  No reference counterpart.
 * d_X: n points (3 doubles each) in the map's own frame; d_cov: NULL or their covariances (9 doubles each, row-major, map frame); d_desc:
 * NULL or their 32-byte descriptors; cam: the camera (intr = fx fy cx cy; model 0 radtan k1 k2 p1 p2, 1 equidistant k1..k4, as
 * lvk_undistort_points; width, height in pixels); align: the map's alignment - only c, s, t of the record are read, NULL = identity
 * (c = 1, s = 0, t = 0 through the same expressions); R_wc (row-major, camera to world) and p_wc as lvk_align_ransac_2pt takes them;
 * cov_cam: NULL or the 6 x 6 covariance (row-major) of the camera pose in the order [dtheta dp]: the rotation error is on the camera side,
 * R_true = R_wc (I + [dtheta]x), dp is in the world frame.  lvk_ekf_camera_pose_cov forms all three from a clone of the filter's window, the
 * extrinsics and the covariance where it lies.  FP64 throughout, no contraction, every expression in the order written here (a product chain a b c is
 * (a b) c, a sum of products runs over its index upwards from the first product), so every field has one right value:
 *   pose       q = (c X_x - s X_y, s X_x + c X_y);  g = ((q_x + t_x) - p_wc,x, (q_y + t_y) - p_wc,y, (X_z + t_z) - p_wc,z);
 *              p_c,i = (R_wc[0][i] g_0 + R_wc[1][i] g_1) + R_wc[2][i] g_2 (= R_wc^T (Rz X + t - p_wc));  x = p_c,x / p_c,z, y = p_c,y / p_c,z,
 *              r2 = x x + y y.
 *   model      radtan: rad = 1 + (k2 r2 + k1) r2;  xd = x rad + 2 p1 x y + p2 (r2 + 2 x x);  yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y.
 *              equidistant: r = sqrt(r2), th = atan(r), t2 = th th, thd = th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))), s = thd / r when
 *              r > 1e-8, else 1;  xd = x s, yd = y s.  px = fx xd + cx, py = fy yd + cy.  (The library's first forward model; everything
 *              else undistorts.)
 *   status     the first rule that applies: BEHIND unless p_c,z > min_depth (a NaN lands here); FAR when p_c,z > max_depth; OUTSIDE unless
 *              r2 <= max_r2; OUTSIDE unless margin <= px <= (width - 1) - margin and margin <= py <= (height - 1) - margin (a NaN pixel lands
 *              here); otherwise VISIBLE.  A radtan model folds back beyond its range: max_r2 is the guard (larvio_amd.localize.view_limit).
 *   radius     S = 0.  With d_cov: R = Rz^T R_wc (R[0][j] = c R_wc[0][j] + s R_wc[1][j], R[1][j] = c R_wc[1][j] - s R_wc[0][j], R[2][j] =
 *              R_wc[2][j]), M = Sigma_X R, S = R^T M - the point's covariance in the camera frame.  With cov_cam: G = [ [p_c]x | -R_wc^T ]
 *              (3 x 6), T = G cov_cam, K = T G^T, and S = S + K (S = K without d_cov).  u_j = S[0][j] - x S[2][j], v_j = S[1][j] - y S[2][j];
 *              e00 = u_0 - u_2 x, e01 = u_1 - u_2 y, e10 = v_0 - v_2 x, e11 = v_1 - v_2 y (= z^2 J S J^T, J = (1 / p_c,z) [[1, 0, -x],
 *              [0, 1, -y]]);  sx = fx / p_c,z, sy = fy / p_c,z;  a = (sx sx) e00, d = (sy sy) e11, b = ((sx sy) e01 + (sx sy) e10) / 2;
 *              lambda = (a + d) / 2 + sqrt(((a - d) / 2)^2 + b^2), the larger eigenvalue of the pixel covariance; lambda = 0 with neither
 *              covariance.  radius = k_sigma sqrt(lambda + sigma_px^2), clamped to [r_min, r_max]; r_max when lambda is negative or not
 *              finite.  The distortion's own Jacobian is left out on purpose: the radius is a gate, not a measurement.
 *   cell       col = min(cols - 1, (int)((px cols) / width)), row = min(rows - 1, (int)((py rows) / height)), from the FP64 pixel;
 *              cell = row cols + col.
 *   selection  every cell keeps its `quota` VISIBLE points with the lowest map index; the output is ordered by (cell, map index), both
 *              ascending.  The map's order is its priority: sort it best-first once, at upload.  Nothing in the rule depends on the
 *              order in which anything ran: two runs on the same input give the same bytes.
 * px, py, radius and p_c,z are rounded to float32 once, at the end.  d_sel: the selected points' records; d_q: the same as lvk_match_query
 * (pad 0), ready for lvk_orb_match_guided; d_q_desc: their descriptors, gathered from d_desc (required when d_desc is given, not touched
 * otherwise) - all three with room for rows cols quota records; d_info: n_selected and the count per status (n_candidates 0, pad 0);
 * d_status: NULL or n bytes, the status with bit 7 set on a selected point.  Records beyond n_selected are not written.  Three launches on
 * the context's stream (project and count; scan the chunk x cell table; ordered scatter and gather), not waited for; the covariances are
 * read for the selected points only.
 * opt may be NULL; a zero field takes its default: min_depth 0.1, max_depth +inf, max_r2 +inf (no test), margin 0, k_sigma 3, sigma_px 1,
 * r_min 4, r_max 40, rows x cols 4 x 5 (1..16 each), quota 1024 / (rows cols) rounded down.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed, a negative count, a non-finite entry of
 * R_wc, p_wc, the alignment or the camera, width or height < 1, a model other than 0 or 1, an option that is NaN, a negative margin, r_min
 * > r_max, rows or cols outside 1..16, quota < 1, rows cols quota > 1024, a descriptor pointer that is not 8-byte aligned.
 * LVK_ERR_CAPACITY: n > 1,048,576.  n == 0: LVK_OK, d_info zeroed, nothing launched. */
#define LVK_MAP_VISIBLE  0
#define LVK_MAP_BEHIND   1
#define LVK_MAP_FAR      2
#define LVK_MAP_OUTSIDE  3
#define LVK_MAP_SELECTED 0x80                    /* bit 7 of a d_status byte */
#define LVK_MAP_MAX_POINTS  1048576
#define LVK_MAP_MAX_QUERIES 1024
typedef struct { double intr[4]; int model, width, height, pad; double dist[4]; } lvk_map_camera;
typedef struct { double min_depth, max_depth, max_r2, margin, k_sigma, sigma_px, r_min, r_max; int rows, cols, quota, pad; } lvk_map_select_options;   /* zeros = defaults */
typedef struct { int index, cell; float x, y, radius, depth; } lvk_map_sel;
typedef struct { int n_selected, n_visible, n_behind, n_far, n_outside, n_candidates, pad[2]; } lvk_map_info;
lvk_status lvk_map_select_queries(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, int n,
                                  const lvk_map_camera* cam, const lvk_align_result* align, const double R_wc[9], const double p_wc[3],
                                  const double cov_cam[36], const lvk_map_select_options* opt, lvk_map_sel* d_sel, lvk_match_query* d_q,
                                  uint8_t* d_q_desc, lvk_map_info* d_info, uint8_t* d_status);
/* Stage entry: the start of that chain - a session's raw exports (lvk_ekf_take_lost_features_cov, lvk_ekf_take_msckf_points, the first-seen
 * descriptors of lvk_frontend_tracks) into the map lvk_frontend_set_map expects: bad points culled, of near-duplicates the better copy
 * kept, the rest sorted best first.  No reference counterpart.  d_X: n points (3 doubles each); d_cov: NULL or their covariances (9 doubles
 * each, row-major); d_desc: their 32-byte descriptors, 8-byte aligned - required when r_dup > 0, otherwise NULL is allowed; d_score: NULL
 * or n doubles, smaller is better.  FP64 throughout, no contraction, every expression in the order written here, so every output has one
 * right value:
 *   score      d_score[i] when d_score is given; otherwise (c00 + c11) + c22 of the point's covariance; 0 with neither.  Scores compare by
 *              value: -0 equals +0 (it is canonicalised to +0 before anything orders by it).
 *   cell       only when r_dup > 0: c_a = floor(X_a / r_dup) per axis - an IEEE division, then floor, so a negative coordinate rounds down,
 *              not towards zero.
 *   status     the first rule that applies: BAD - a non-finite entry of X, of the covariance (when given, whether or not it is the score) or
 *              a non-finite score (a covariance trace that overflows included), a negative covariance diagonal, a score < 0; UNCERTAIN -
 *              score > max_score; OUT_OF_RANGE - r_dup > 0 and some |c_a| > 2^20 - 1; DUPLICATE - below; otherwise KEPT.
 *   duplicate  the points that are not BAD, UNCERTAIN or OUT_OF_RANGE are eligible.  An eligible i is DUPLICATE iff there is an eligible
 *              j != i with (score_j, j) < (score_i, i) lexicographically, |c_a(i) - c_a(j)| <= 1 on all three axes, d2 = ((dx dx + dy dy) +
 *              dz dz) <= r_dup r_dup with dx = X_i,x - X_j,x and so on, and a Hamming distance of the two descriptors <= dup_max_dist.  j
 *              counts whether or not j is itself a DUPLICATE: the rule is not greedy, so it depends on no processing order - the price is
 *              that a chain A-B-C (A suppresses B, B suppresses C, A and C apart) keeps only A.  The cell condition is part of the rule
 *              (it can only bite where a division rounds at a cell's edge), so the answer is exact there too.  Nothing is fused or
 *              averaged: the better copy stays as it is.
 *   order      the KEPT points by ascending (score, original index): a stable sort.
 * d_order: the original indices of the kept points, best first; d_X_out, d_cov_out, d_desc_out: the kept points gathered in that order, in
 * lvk_frontend_set_map's layout - each with room for n records, n_kept of them are written and nothing beyond; d_cov_out / d_desc_out may
 * be NULL when d_cov / d_desc is, and is neither read, written nor checked for alignment then, whatever it is.  No output may alias an input.  d_status: NULL or n bytes (LVK_MAPB_*); d_info: the count per status (they
 * sum to n) and pad 0, written by the kernels of every call that launches (no host clear).  On the context's stream, not waited for, work
 * buffers from the context's pool (37 bytes a point): classify; with r_dup > 0 a stable LSD radix sort by packed cell key (eight passes of
 * three launches: count, scan, ordered scatter from wave ballots) and the neighbour search - every point visits its 27 neighbour cells by
 * nine binary searches, candidates tested position, Hamming, priority; the cost is quadratic inside one crowded cell and is not capped -;
 * the order's keys and the counts; the same sort on the scores' bits (non-negative finite doubles order as their bit patterns); the gather.
 * opt may be NULL; a zero field takes its default: max_score +inf, r_dup 0 = no de-duplication (and no OUT_OF_RANGE), dup_max_dist 32.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed, n < 0, an option that is NaN or
 * negative, dup_max_dist outside 0..256, a descriptor pointer that is not 8-byte aligned, r_dup > 0 without descriptors.
 * LVK_ERR_CAPACITY: n > LVK_MAP_MAX_POINTS.  n == 0: LVK_OK, d_info zeroed, nothing launched. */
#define LVK_MAPB_KEPT         0
#define LVK_MAPB_BAD          1
#define LVK_MAPB_UNCERTAIN    2
#define LVK_MAPB_OUT_OF_RANGE 3
#define LVK_MAPB_DUPLICATE    4
typedef struct { double max_score, r_dup; int dup_max_dist, pad; } lvk_map_build_options;   /* zeros = defaults */
typedef struct { int n_kept, n_bad, n_uncertain, n_out_of_range, n_duplicate, pad[3]; } lvk_map_build_info;
lvk_status lvk_map_build(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, const double* d_score, int n,
                         const lvk_map_build_options* opt, int* d_order, double* d_X_out, double* d_cov_out, uint8_t* d_desc_out,
                         uint8_t* d_status, lvk_map_build_info* d_info);
/* Stage entry: global ORB search of a device-resident map - the first link of that chain at the map's full size.  The search runs the other
 * way round from lvk_orb_match_guided: the n_cand described corners of the frame are the queries (descriptor of corner c at d_cand_desc +
 * 32 c) and the n_map map points are the database; there is no window.  No reference counterpart.  Everything is integer, so every field
 * has one right value:
 *   best       for corner c, the map point with the smallest Hamming distance over all n_map points, ties to the lowest map index:
 *              d_best[c].cand = that MAP INDEX (the field keeps the name it has in lvk_match_result), dist = its distance,
 *              n_window = n_map, pad = 0.
 *   second     the smallest distance over the map points other than best, -1 when n_map == 1.
 *   status     the first rule of lvk_orb_match_guided that applies, unchanged: NO_CANDIDATE when n_map == 0 (cand = dist = second = -1);
 *              TOO_FAR when dist > max_dist; AMBIGUOUS when second >= 0 and 100 * dist > ratio_pct * second - two exact duplicates at
 *              distance 0 are therefore NOT ambiguous (0 > 0 is false), as in the guided matcher; otherwise the corner is provisionally
 *              matched.  A map point claimed by several provisionally matched corners goes to the smallest (dist, corner index): that
 *              corner is OK, the others are CONFLICT, keep their cand and dist and are NOT moved to their second choice.
 *   selection  the OK corners in ascending (dist, corner index) order; the first n_selected = min(n_ok, max_matches) of them are written to
 *              d_sel[0 .. n_selected) as (cand = the corner, index = the map point, dist, second).  Records beyond n_selected are not touched.
 *   info       n_ok, n_no_candidate, n_too_far, n_ambiguous, n_conflict: the corners per status (they sum to n_cand); n_selected; pad 0.
 * Nothing in the rule depends on how the work is cut into slices of the map or tiles of corners, nor on the order in which anything ran.
 * d_best: n_cand records; d_sel: max_matches records; d_info: one record, written by the kernels of every call that launches (no host
 * clear).  Both descriptor pointers must be 8-byte aligned.  Four launches on the context's stream (search: two smallest keys dist << 20 |
 * index per slice of the map and corner; pick: the two smallest over the slices, status, and a reset of the claim words that can be
 * touched - never of one word per map point; claim: a 64-bit atomicMin of dist << 32 | corner; select: resolve, count, order - one
 * workgroup), not waited for.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer where its count is positive (d_best, d_sel and d_info
 * go with n_cand), a negative count, max_dist outside 0..256, ratio_pct outside 1..100, max_matches outside 1..1024, a descriptor pointer
 * that is not 8-byte aligned.  LVK_ERR_CAPACITY: n_cand > 4096 or n_map > LVK_MAP_MAX_POINTS.  n_cand == 0: LVK_OK, nothing launched,
 * nothing written.  n_map == 0: every corner NO_CANDIDATE. */
typedef struct { int cand, index, dist, second; } lvk_global_match;
typedef struct { int n_ok, n_no_candidate, n_too_far, n_ambiguous, n_conflict, n_selected, pad[2]; } lvk_global_info;
lvk_status lvk_orb_match_global(lvk_context* ctx, const uint8_t* d_map_desc, int n_map, const uint8_t* d_cand_desc, int n_cand,
                                int max_dist, int ratio_pct, int max_matches, lvk_match_result* d_best, lvk_global_match* d_sel,
                                lvk_global_info* d_info);
/* Stage entry: a second session into the map of the first (3D-3D) - the yaw and translation that take session B's frame into the resident
 * map's frame A, from n putative point-to-point matches, many of them wrong, by two-point RANSAC over n_pairs given pairs.  No reference
 * counterpart.  Both frames have z along gravity, so the model is that of lvk_align_ransac_2pt: Y = Rz(psi) X + t, carried as c = cos psi,
 * s = sin psi and t, Rz X = (c X_x - s X_y, s X_x + c X_y, X_z).  Match k carries X_k (frame B) and Y_k (frame A).  The pairs, the result
 * record and the statuses are lvk_align_ransac_2pt's (lvk_align_pair, lvk_align_draw_pairs, lvk_align_result, LVK_ALIGN_*).  FP64
 * throughout, no contraction, no atan2 / sin / cos, every expression in the order written here (a sum of products runs from the first
 * product upwards):
 *   solver     pair (i, j): a = X_i - X_j, b = Y_i - Y_j (per component), ra2 = a_x a_x + a_y a_y, rb2 = b_x b_x + b_y b_y.  No model when
 *              i == j; when an index is outside 0..n-1 (nothing is read); when ra2 or rb2 is not > min_rho min_rho (a NaN lands here);
 *              when |a_z - b_z| > 2 thresh; when |sqrt(ra2) - sqrt(rb2)| > 2 thresh.  Otherwise dot = a_x b_x + a_y b_y,
 *              crs = a_x b_y - a_y b_x, nrm = sqrt(dot dot + crs crs) - no model either unless nrm > 0, which only an underflow of a
 *              min_rho below 1e-150 can bring about -, c = dot / nrm, s = crs / nrm.  With q_k = (c X_k,x - s X_k,y, s X_k,x + c X_k,y)
 *              (the expressions of lvk_map_select_queries): t_x = ((Y_i,x - q_i,x) + (Y_j,x - q_j,x)) / 2, t_y likewise,
 *              t_z = ((Y_i,z - X_i,z) + (Y_j,z - X_j,z)) / 2.  One model per pair.
 *   score      match k is an inlier iff d2 = (d_x d_x + d_y d_y) + d_z d_z <= thresh thresh with d = ((q_k,x + t_x) - Y_k,x,
 *              (q_k,y + t_y) - Y_k,y, (X_k,z + t_z) - Y_k,z); a NaN is not an inlier.  count = the inliers.
 *   winner     the model with the largest count; ties to the lowest hypothesis index.  d_mask[k] = 1 for its inliers, 0 otherwise; the mask
 *              is NOT scored again after the refinement.
 *   refinement closed form over the winner's m inliers, no iteration: mX = (sum X_k) / m, mY = (sum Y_k) / m; x' = X_k - mX, y' = Y_k - mY;
 *              D = sum (x'_x y'_x + x'_y y'_y), C = sum (x'_x y'_y - x'_y y'_x), W = sum ((x'_x x'_x + x'_y x'_y) + (y'_x y'_x + y'_y y'_y));
 *              nrm = sqrt(D D + C C), c = D / nrm, s = C / nrm, t = (mY_x - (c mX_x - s mX_y), mY_y - (s mX_x + c mX_y), mY_z - mX_z).
 *              At the model that is returned, with q_k as above and r_k = the d of the score: A = sum J^T J (4 x 4, order psi, t_x, t_y,
 *              t_z), J_k = [(-q_k,y, q_k,x, 0)^T | I3], that is A00 = sum (q_k,y q_k,y + q_k,x q_k,x), A01 = A10 = sum -q_k,y,
 *              A02 = A20 = sum q_k,x, A11 = A22 = A33 = m, every other entry 0; rms = sqrt((sum ((r_x r_x + r_y r_y) + r_z r_z)) / m).
 *              The sums over the inliers may be taken in any order (they are, across the lanes, in one fixed shape: two calls give the
 *              same bytes).  The caller inverts A and scales by the points' variance - the library invents no covariance.
 *   status     the first rule that applies: NO_MODEL no pair gave a model (fields as lvk_align_ransac_2pt sets them: hyp = root = pair_i =
 *              pair_j = -1, c = c0 = 1, all else 0, mask zeroed); FEW_INLIERS the best count is below min_inliers (c0, s0, t0 = c, s, t =
 *              the winner, the mask is the winner's, A = rms = 0); SINGULAR the refinement's nrm is not > 1e-12 (W / 2) - all inliers on
 *              one vertical line in either frame - (c, s, t = the winner again, A and rms at the winner); OK.  root is 0 whenever there is
 *              a winner, iters is always 0.
 * d_m: n matches; d_pairs: n_pairs pairs; d_hyp: NULL or n_pairs records - n_models (0 or 1), count, c, s, t, everything zero when there is
 * no model, the pads zero; d_mask: n bytes; d_out: one record.  Matches beyond n and records beyond n_pairs are not read or written.
 * Two launches on the context's stream, not waited for: the hypotheses (four wavefronts a workgroup, one pair each; the workgroup stages
 * the n matches in LDS once - 48 bytes each, 48 KB at the cap, inside the 64 KB that need no opt-in -, a wavefront scores its model across
 * its lanes, 64 matches a step, and counts with an integer ballot); then one workgroup for the arg-max (an integer key), the mask and the
 * refinement.  No atomics anywhere.
 * opt may be NULL; a zero field takes its default: thresh 0.10 (metres), min_rho 0.5 (metres), min_inliers 6 (2..1024).  The defaults
 * are design choices, not measurements: 10 cm is a few sigma of a good exported point, 0.5 m keeps a pair's yaw from being decided by
 * that noise.  LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed, a negative count, an option
 * that is not finite, not positive or outside its range.  LVK_ERR_CAPACITY: n > 1024 (the matches are staged in LDS) or n_pairs > 4096.
 * n < 2 or n_pairs == 0: NO_MODEL, the mask zeroed, the hypotheses kernel not launched. */
typedef struct { double X[3], Y[3]; } lvk_align3d_match;
typedef struct { int n_models, count, pad[2]; double c, s, t[3]; } lvk_align3d_hyp;
typedef struct { double thresh, min_rho; int min_inliers, pad; } lvk_align3d_options;   /* zeros = defaults */
lvk_status lvk_align_ransac_3d(lvk_context* ctx, const lvk_align3d_match* d_m, int n, const lvk_align_pair* d_pairs, int n_pairs,
                               const lvk_align3d_options* opt, lvk_align3d_hyp* d_hyp, uint8_t* d_mask, lvk_align_result* d_out);
/* The alignment the other way round (host only): in holds A -> B as Y = Rz X + t (its refined c, s, t are read), out takes B -> A:
 * c' = c, s' = -s, t' = (-(c t_x + s t_y), -(c t_y - s t_x), -t_z), every other field 0.  A session that was localised online holds the
 * map's alignment into its own world frame; lvk_frontend_merge_map wants the session's into the map.  in == out is allowed.
 * LVK_ERR_ARG: a null pointer. */
lvk_status lvk_align_invert(const lvk_align_result* in, lvk_align_result* out);
/* Stage entry: an alignment applied to a point set where it lies on the device.  No reference counterpart.  d_X: n points (3 doubles each);
 * d_cov: NULL or their covariances (9 doubles each, row-major; the upper triangle is read); d_desc: NULL or their 32-byte descriptors;
 * align: only c, s, t of the record are read, NULL = identity (c = 1, s = 0, t = 0 through the same expressions, so NULL and an explicit
 * identity record give the same bytes); cov_align16: NULL or the 4 x 4 covariance P (row-major; the upper triangle is read) of the
 * alignment's (psi, t_x, t_y, t_z).  FP64 throughout, no contraction, every expression in the order written here:
 *   p          q = (c X_x - s X_y, s X_x + c X_y), p = (q_x + t_x, q_y + t_y, X_z + t_z) - the expressions of lvk_map_select_queries.
 *   cov        w = Rz Sigma Rz^T by the expressions of lvk_map_gather_obs (w00, w01, w11, w02, w12, w22 from a, b, d, e, f, g).  With
 *              cov_align16: j = (-q_y, q_x, 0) and, for a <= b, k_ab = (((j_a j_b) P[0][0] + j_a P[0][1 + b]) + j_b P[0][1 + a]) +
 *              P[1 + a][1 + b] (= J P J^T, J = [j^T | I3]); the output is w_ab + k_ab, k_ab alone without d_cov.  The full matrix is
 *              written, entry (b, a) is a copy of entry (a, b).  This treats the alignment's error, which all points of the set share,
 *              as independent from point to point: right for any one point, too optimistic for what depends on several of them.
 *   desc       copied.
 * Non-finite points and covariances pass through (lvk_map_build classifies them).  d_X_out: n x 3; d_cov_out: n x 9, written when d_cov
 * or cov_align16 is given and required then, otherwise untouched; d_desc_out: n x 32, written and required when d_desc is given, otherwise
 * untouched.  Each may be the tail of a larger buffer.  No output may alias an input.  One launch on the context's stream, one lane per
 * point, chunks of 256, not waited for.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed, n < 0, a non-finite c, s or t of the
 * alignment, a non-finite entry of cov_align16, a descriptor pointer that is not 8-byte aligned.  LVK_ERR_CAPACITY: n >
 * LVK_MAP_MAX_POINTS.  n == 0: LVK_OK, nothing launched. */
lvk_status lvk_map_transform(lvk_context* ctx, const double* d_X, const double* d_cov, const uint8_t* d_desc, int n, const lvk_align_result* align,
                             const double cov_align16[16], double* d_X_out, double* d_cov_out, uint8_t* d_desc_out);
/* replaces integrateImuData + predictFeatureTracking's matrix (image_processor.cpp:222-293): host math */
lvk_status lvk_predict_homography(const lvk_imu* h_imu, int n_imu, double t_prev, double t_curr,
                                  const double R_cam_imu[9], const double intr[4], float H[9]);

/* ------------------------------------------------------------------ the front-end object
 * replaces larvio::ImageProcessor (image_processor.h:36-68): lvk_frontend_create = ctor+initialize()
 * (image_processor.cpp:28-126, parameters as loadParameters reads them), lvk_frontend_process =
 * processImage (image_processor.cpp:130-219). */
typedef struct {
    int width, height;
    int pyramid_levels;      /* config/euroc.yaml:43 */
    int patch_size;          /* :44 */
    int max_iteration;       /* :46 */
    double track_precision;  /* :47 */
    int max_features_num;    /* :49 */
    int min_distance;        /* :50 */
    int flag_equalize;       /* :51 */
    int pub_frequency;       /* :52 */
    int distortion_model;    /* 0 radtan, 1 equidistant (:14) */
    double intrinsics[4];    /* fx fy cx cy (:17-21) */
    double distortion[4];    /* (:22-26) */
    double R_cam_imu[9];     /* row-major, = (T_cam_imu rotation)^T as image_processor.cpp:93 */
} lvk_fe_config;

lvk_status lvk_frontend_create(lvk_context* ctx, const lvk_fe_config* cfg, lvk_frontend** out);
void       lvk_frontend_destroy(lvk_frontend* fe);
/* img->width/height must equal the configured resolution and img->stride >= width (LVK_ERR_ARG otherwise: the reference cannot
 * read past a cv::Mat, neither does this).  h_out receives up to cap features when *has_msg = 1 (the reference's
 * `return haveFeatures`). */
lvk_status lvk_frontend_process(lvk_frontend* fe, const lvk_image* img,
                                double ts, const lvk_imu* h_imu, int n_imu,
                                lvk_feature_obs* h_out, int cap, int* n_out, int* has_msg);
/* introspection (synchronises): live tracks after the last call = the reference's
 * pts_ids_/prev_pts_/pts_lifetime_/init_pts_/vOrbDescriptors after the rotation at :207-216 */
lvk_status lvk_frontend_tracks(lvk_frontend* fe, uint64_t* h_ids, lvk_pt2f* h_pts, int* h_lifetime,
                               lvk_pt2f* h_init, uint8_t* h_desc, int cap, int* n_out);
lvk_status lvk_frontend_new_pts(lvk_frontend* fe, lvk_pt2f* h_pts, int cap, int* n_out);
int        lvk_frontend_state(const lvk_frontend* fe);   /* 1 FIRST_IMAGE 2 SECOND_IMAGE 3 OTHER_IMAGES */
/* Region mask for corner detection - OpenCV's mask argument of goodFeaturesToTrack.  No reference counterpart: the reference's
 * ImageProcessor detects with its own keep-out mask only (image_processor.cpp:1005-1037) and with none on the first frame (:337-352).
 * nonzero = corners may be detected here; NULL clears.  mask->width/height must equal the configured resolution and mask->stride >=
 * width (LVK_ERR_ARG otherwise, as lvk_frontend_process; the mask in force stays); is_device 0 and 1 are both accepted.  The call waits
 * for the front-end's own streams, so a detection already queued keeps the mask it was queued with, then stores a packed 0/255 copy in
 * a device buffer the front-end owns (the caller's buffer is free on return).  The mask holds from the next processed frame on: it is
 * ANDed with the reference's keep-out mask on re-detection and takes the place of "no mask" on the first frame, and it governs the
 * maximum behind the quality threshold as well as the candidates.  It restricts detection only: a track that moves into a masked
 * area is kept.  Budget, quality level, min_distance and ordering are unchanged, and with no mask set the front-end launches exactly
 * the kernels it launches without this call.  With a lvk_vio_pipe attached, call it before the first lvk_vio_pipe_submit or after
 * lvk_vio_pipe_drain - never between a submit and the drain that follows. */
lvk_status lvk_frontend_set_mask(lvk_frontend* fe, const lvk_image* mask);
int        lvk_frontend_has_mask(const lvk_frontend* fe);
/* Input pixel format (LVK_PIX_*, shift as lvk_image_to_gray).  No reference counterpart: the reference's library takes MONO8 and its
 * ROS caller converts on the host.  After the call every lvk_image given to this front-end - lvk_frontend_process, lvk_vio_process,
 * lvk_vio_process_deferred, lvk_vio_pipe_submit - is in that format: data points at the format's bytes, width / height stay the
 * configured resolution in pixels, stride is in bytes and must be >= width * bytes_per_pixel (LVK_ERR_ARG otherwise, the handle stays
 * usable); a MONO16 device image also needs an even pointer and stride.  The raw bytes take the usual upload route and
 * lvk_image_to_gray turns them into a grey plane the front-end owns, on the image stream in front of the pyramid; everything after that
 * is the MONO8 path.  The call waits for the front-end's own streams, then resizes the upload buffers to the format's row bytes;
 * LVK_ERR_ARG for an unknown format, a bad shift, or YUYV / UYVY on an odd configured width, LVK_ERR_DEVICE when a buffer cannot be
 * had - either way the format in force stays.  LVK_PIX_MONO8 (the default) restores today's buffers and launches: no grey plane, no
 * conversion kernel.  With a lvk_vio_pipe attached, call it before the first lvk_vio_pipe_submit or after lvk_vio_pipe_drain. */
lvk_status lvk_frontend_set_input_format(lvk_frontend* fe, int format, int shift);
int        lvk_frontend_input_format(const lvk_frontend* fe);
/* Where in the last processed frame are these map points?  No reference counterpart.  h_q: n_q predicted pixels with their search radii,
 * h_desc: their 32-byte descriptors (e.g. the first-seen descriptor lvk_frontend_tracks returned for the point's feature id), at most 1024.
 * The call waits for the front-end's own streams, as lvk_frontend_tracks does, then runs on the main stream, on the pyramid and ORB planes
 * of the last processed frame: lvk_min_eigen_map into a buffer of its own (allocated on first use; nothing the detection owns is touched),
 * lvk_good_features_from_map with no mask at all (max_candidates, quality, min_distance), lvk_orb_describe of those corners,
 * lvk_orb_match_guided (max_dist, ratio_pct), lvk_undistort_points of the matched pixels with unit intrinsics - as the feature message does
 * it -, and one copy of the n_q records back.  Per query: status, dist, second and n_window as lvk_orb_match_guided states them; px = the
 * candidate's pixel, und = its normalised coordinate (what lvk_landmark_obs takes as uv); both (0, 0) for NO_CANDIDATE, and set for every
 * other status, OK or not.  *n_cand_out (may be NULL) = corners the selection found.  The call is off the per-frame path: it waits for the
 * GPU twice (the corner count, the records) and changes nothing a later frame reads - a run with these calls publishes the bits of a run
 * without them.
 * opt may be NULL; a zero field takes its default: max_candidates 4096 (1..4096), quality 0.01, min_distance the configured
 * min_distance - the spacing the map's own points were detected at -, max_dist 58 (the front-end's own descriptor gate; 1..256 here, 0
 * being the default's spelling), ratio_pct 100 = no ratio test (1..100).
 * LVK_ERR_ARG, with nothing launched: a null pointer that is needed, n_q < 0, a field of opt outside its range or not finite, a call
 * before the first processed frame, a call between lvk_frontend_begin and the lvk_frontend_process of the same frame.  LVK_ERR_CAPACITY:
 * n_q > 1024, max_candidates > 4096, and the selection's own refusal (its cell grid does not fit the LDS: lvk_good_features_from_map),
 * passed through unchanged; its LVK_ERR_UNSUPPORTED for a min_distance outside 1..32767 likewise.  None of these is sticky: the handle
 * goes on.  On a handle that has failed the call returns the failure, as lvk_frontend_process does.  n_q == 0 is legal and still reports
 * *n_cand_out.  With a lvk_vio_pipe attached, call it only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit - never between
 * a submit and the drain that follows. */
typedef struct { int max_candidates; double quality, min_distance; int max_dist, ratio_pct; } lvk_match_options;  /* zeros = defaults */
typedef struct { int status, dist, second, n_window; lvk_pt2f px, und; } lvk_landmark_match;
lvk_status lvk_frontend_match_landmarks(lvk_frontend* fe, const lvk_match_query* h_q, const uint8_t* h_desc, int n_q,
                                        const lvk_match_options* opt, lvk_landmark_match* h_out, int* n_cand_out);
/* The first link of that chain: a map from another session has its own origin and yaw, and lvk_frontend_match_landmarks can only be asked
 * once the map is in the filter's world frame.  Match the map's descriptors with an infinite radius and a ratio test, hand the OK
 * records here (h_m: X = the map point, u, v = lvk_landmark_match.und; n <= 1024) with the camera pose of that frame in the filter's world
 * frame, and the call returns the yaw and translation of the map (lvk_align_ransac_2pt states all of it).  It waits for the front-end's own
 * streams, as lvk_frontend_match_landmarks does, draws the pairs (lvk_align_draw_pairs with max_hypotheses - 0 = 4096, the cap - and seed),
 * uploads, runs the stage entry on the main stream in buffers of its own (allocated on first use) and copies the result and the n mask
 * bytes back (h_mask may be NULL).  Off the per-frame path; it changes nothing a later frame reads - a run with these calls publishes the
 * bits of a run without them.  LVK_ERR_ARG, with nothing launched: a null pointer that is needed, n < 0, max_hypotheses < 0, the
 * stage entry's own refusals, a call before the first processed frame or between lvk_frontend_begin and the lvk_frontend_process of
 * the same frame.  LVK_ERR_CAPACITY: n > 1024, max_hypotheses > 4096.  None is sticky.  With a lvk_vio_pipe attached, call it only
 * between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
lvk_status lvk_frontend_align_landmarks(lvk_frontend* fe, const lvk_align_match* h_m, int n, const double R_wc[9], const double p_wc[3],
                                        const lvk_align_options* opt, int max_hypotheses, uint32_t seed, lvk_align_result* h_out,
                                        uint8_t* h_mask);
/* The per-frame link of that chain with the map resident on the device.  lvk_frontend_set_map copies a prior map - n points h_X (3 doubles
 * each, the map's own frame), their covariances h_cov9 (9 doubles each, may be NULL) and their 32-byte descriptors h_desc (required) - into
 * device buffers the front-end owns; it replaces a previous map, n == 0 frees it (the pointers may then be NULL).  The map's order is its
 * priority (lvk_map_select_queries).  It waits for the front-end's own streams and for the copies.  LVK_ERR_ARG: a null pointer that is
 * needed, n < 0, a call between lvk_frontend_begin and the lvk_frontend_process of the same frame; LVK_ERR_CAPACITY: n > 1,048,576;
 * LVK_ERR_DEVICE when the buffers cannot be had - in each case the map in force stays.  lvk_frontend_map_size = the points of the map in
 * force (0: none).
 * lvk_frontend_match_map runs lvk_map_select_queries on that map with the configured camera (align, R_wc, p_wc, cov_cam36, select_opt as
 * the stage entry takes them), reads n_selected back, then runs exactly the device chain of lvk_frontend_match_landmarks (match_opt: its
 * options) on the selected queries and their gathered descriptors, and copies n_selected records back: index and cell of the map point,
 * the query q the matcher was given, the point's depth, and m, the record lvk_frontend_match_landmarks returns for that query.  cap: the
 * room in h_out, at least rows cols quota of select_opt (1020 with the defaults); *n_out = n_selected; h_info (may be NULL): the stage
 * entry's counts with n_candidates = the corners the frame offered.  The same preconditions, waits (three here: the selection's count,
 * the corner count, the records) and promise as lvk_frontend_match_landmarks: off the per-frame path, it changes nothing a later frame
 * reads - a run with these calls publishes the bits of a run without them - and a front-end that never calls them launches what it
 * launched before.  LVK_ERR_ARG, with nothing launched: no map is set, a null pointer that is needed, a call before the first processed
 * frame or between lvk_frontend_begin and the lvk_frontend_process of the same frame, and the refusals of the stage entry and of
 * lvk_frontend_match_landmarks; LVK_ERR_CAPACITY: cap < rows cols quota, and what lvk_frontend_match_landmarks passes through.  None is
 * sticky.  With a lvk_vio_pipe attached, call either only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
typedef struct { int index, cell; lvk_match_query q; float depth, pad; lvk_landmark_match m; } lvk_map_match;
lvk_status lvk_frontend_set_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, int n);
int        lvk_frontend_map_size(const lvk_frontend* fe);
lvk_status lvk_frontend_match_map(lvk_frontend* fe, const lvk_align_result* align, const double R_wc[9], const double p_wc[3],
                                  const double cov_cam36[36], const lvk_map_select_options* select_opt, const lvk_match_options* match_opt,
                                  lvk_map_match* h_out, int cap, int* n_out, lvk_map_info* h_info);
/* The start of that chain with the map resident on the device: a session's raw exports in, the map in force out.  h_X, h_cov9 (may be NULL),
 * h_desc (required: the resident map has descriptors) as lvk_frontend_set_map takes them, h_score (may be NULL) and opt as lvk_map_build
 * takes them.  The call uploads, runs lvk_map_build on the main stream in buffers of its own, waits, and makes the gathered arrays the map
 * in force exactly as if lvk_frontend_set_map had been called with them: lvk_frontend_map_size = n_kept afterwards, n_kept == 0 (n == 0
 * included) frees the map.  h_order (may be NULL; cap_order = its room in entries): the original indices of the kept points in the map's
 * order, so that the caller keeps its own ids and attributes in step; info (may be NULL): the stage entry's counts.  The same preconditions
 * and waits as lvk_frontend_set_map.  LVK_ERR_ARG: a null pointer that is needed, n < 0, cap_order < 0, the stage entry's refusals, a call
 * between lvk_frontend_begin and the lvk_frontend_process of the same frame; LVK_ERR_CAPACITY: n > LVK_MAP_MAX_POINTS, or h_order given
 * and cap_order < n_kept (cap_order >= n always suffices); LVK_ERR_DEVICE when the buffers cannot be had - in each case the map in force
 * stays, and none is sticky.  Off the per-frame path: a run that never calls it launches what it launched before.  With a lvk_vio_pipe
 * attached, call it only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
lvk_status lvk_frontend_build_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, const double* h_score, int n,
                                  const lvk_map_build_options* opt, int* h_order, int cap_order, lvk_map_build_info* info);
/* The first link of that chain with the map resident on the device: from "last processed frame + map in force + camera pose" to the map's
 * yaw and translation in one call, whatever the map's size.  It detects and describes the frame's corners exactly as
 * lvk_frontend_match_landmarks does (lvk_min_eigen_map, lvk_good_features_from_map with no mask, a wait for the count, lvk_orb_describe;
 * match_opt's max_candidates, quality, min_distance), runs lvk_orb_match_global of the map's descriptors against them (match_opt's
 * max_dist and ratio_pct - zero fields take lvk_frontend_match_landmarks' defaults, so ratio_pct stays 100: 80 is recommended here -;
 * max_matches, 0 = 1024), waits for n_selected, draws the pairs on the host (lvk_align_draw_pairs(n_selected, max_hypotheses, seed)),
 * gathers the lvk_align_match records on the device (X = map point `index`, (u, v) = the corner's pixel through lvk_undistort_points with
 * unit intrinsics), runs lvk_align_ransac_2pt (align_opt) and makes one copy back: h_out = the result, h_matches[0 .. n_selected) = the
 * selection's records in its order with the corner's pixel px, its normalised coordinate und, inlier = the mask byte and pad = 0,
 * h_info (may be NULL) = the search's counts.  *n_out = n_selected; cap = the room in h_matches, at least min(max_matches, 1024).
 * n_selected < 2 gives LVK_ALIGN_NO_MODEL through the stage entry's own rule and is no error.
 * The same preconditions, waits (three: the corner count, n_selected, the records) and promise as lvk_frontend_match_map: off the per-frame
 * path, it waits for the front-end's own streams, works in buffers of its own (allocated on first use) and the matcher's corner buffers,
 * changes nothing a later frame reads - a run with these calls publishes the bits of a run without them - and a front-end that never calls
 * it allocates and launches what it did before.  LVK_ERR_ARG: no map is set, a null pointer that is needed, max_matches outside 0..1024 (as
 * the stage entry refuses it), max_hypotheses negative, a call before the first processed frame or between lvk_frontend_begin and the lvk_frontend_process of the same frame, and the
 * refusals of lvk_frontend_match_landmarks' options and of the stage entries, passed through; LVK_ERR_CAPACITY: cap < min(max_matches,
 * 1024), max_hypotheses > 4096, and what the stage entries pass through.  None is sticky.  With a lvk_vio_pipe attached,
 * call it only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
typedef struct { int cand, index, dist, second; lvk_pt2f px, und; int inlier, pad; } lvk_reloc_match;
lvk_status lvk_frontend_relocalise_map(lvk_frontend* fe, const double R_wc[9], const double p_wc[3], const lvk_match_options* match_opt,
                                       const lvk_align_options* align_opt, int max_matches, int max_hypotheses, uint32_t seed,
                                       lvk_align_result* h_out, lvk_reloc_match* h_matches, int cap, int* n_out, lvk_global_info* h_info);
/* The way back into that chain: a second session's exports merged into the map in force (multi-session mapping).  h_X, h_cov9, h_desc: the
 * n points of session B in B's own world frame, as lvk_frontend_build_map takes them (covariances and descriptors are required here).
 * align: B -> A (Y = Rz X + t; lvk_align_invert turns the A -> B alignment of a session that was localised online), or NULL = find it;
 * cov_align16: NULL or the alignment's covariance as lvk_map_transform takes it.  On the main stream, in buffers of the call's own - the
 * small ones of the search and the alignment allocated by the first call and kept, the ones sized by the two maps for the call's duration:
 *   1  upload B; lvk_map_build on B alone with build_opt (cull, B's own duplicates, best first): order_B, n_kept_B.  One wait.
 *   2  only when align == NULL: the first min(n_kept_B, 4096) points of the sorted B are the queries of lvk_orb_match_global against the
 *      resident map's descriptors (match_opt's max_dist and ratio_pct, zero = 58 and 100 as elsewhere, the other fields are not read;
 *      max_matches 1024); a wait for n_selected; lvk_align_draw_pairs(n_selected, max_hypotheses, seed); a gather kernel writes the
 *      lvk_align3d_match records, X = sorted B's point `cand`, Y = the resident point `index`; lvk_align_ransac_3d (align_opt); a wait for
 *      the result.  A status other than LVK_ALIGN_OK ends the call with LVK_OK, *h_align_out carrying the status, the map in force
 *      untouched, *info zeroed and h_order not written: not finding an alignment is an answer, not an error.
 *   3  the resident arrays are copied device to device into [A | .], lvk_map_transform (the alignment, cov_align16) writes the sorted B
 *      behind them.
 *   4  lvk_map_build with build_opt on the concatenation, the covariance's trace the score on both sides.  On equal scores the resident
 *      copy wins - as a duplicate's better copy and in the order -, because its index is the lower.  One wait.
 *   5  the result becomes the map in force exactly as lvk_frontend_build_map installs it (n_kept == 0 frees the map).
 *   6  h_order (may be NULL; cap_order = its room in entries) in the caller's view: a value i < n_A is resident point i, any other is
 *      n_A + B's ORIGINAL index (composed through order_B), n_A the size of the map before the call - so the caller keeps its ids in step.
 * *h_align_out (required): the alignment that was used - the stage entry's record, or a copy of *align; *info (may be NULL): the counts of
 * step 4; *h_match_info (may be NULL): the search's counts, zero when align was given.
 * LVK_ERR_ARG: no map is set, the resident map has no covariances, h_X, h_cov9 or h_desc is NULL with n > 0, h_align_out is NULL, n < 0,
 * cap_order < 0, max_hypotheses < 0, with align == NULL a max_dist outside 0..256 or a ratio_pct outside 0..100 (with an alignment given
 * the search does not run and its options are not read), a non-finite c, s or t of align, a non-finite entry of cov_align16, the stage
 * entries' refusals of the options, a call between lvk_frontend_begin and the lvk_frontend_process of the same frame - each of these is
 * found before anything is uploaded or launched.  LVK_ERR_CAPACITY: n_A + n > LVK_MAP_MAX_POINTS, max_hypotheses >
 * 4096, h_order given and cap_order < n_kept (cap_order >= n_A + n always suffices).  LVK_ERR_DEVICE when the buffers cannot be had.  In
 * each case the map in force stays, and none is sticky.  Off the per-frame path: it waits for the front-end's own streams first, changes
 * nothing a later frame reads - a run with merges between frames publishes the bits of a run without them -, and a run that never calls it
 * launches and allocates what it did before.  With a lvk_vio_pipe attached, call it only between lvk_vio_pipe_drain and the next
 * lvk_vio_pipe_submit. */
lvk_status lvk_frontend_merge_map(lvk_frontend* fe, const double* h_X, const double* h_cov9, const uint8_t* h_desc, int n,
                                  const lvk_align_result* align, const double cov_align16[16], const lvk_match_options* match_opt,
                                  const lvk_align3d_options* align_opt, int max_hypotheses, uint32_t seed,
                                  const lvk_map_build_options* build_opt, lvk_align_result* h_align_out, int* h_order, int cap_order,
                                  lvk_map_build_info* info, lvk_global_info* h_match_info);
/* cumulative LK work: point-levels processed and iterations executed (SURVEY §8d byte model) */
lvk_status lvk_frontend_lk_stats(lvk_frontend* fe, uint64_t* point_levels, uint64_t* iterations);
/* feature messages published so far (getFeatureMsg, image_processor.cpp:1076-1128) and the features they carried in total:
   features / messages = the tracks the tracker holds per published frame (the "~150 tracks" of BASELINE.json's metric) */
lvk_status lvk_frontend_msg_stats(lvk_frontend* fe, uint64_t* messages, uint64_t* features);

/* Per-stage GPU time measured with HIP events on the context's stream (the reference only times the
 * whole call, app/larvioMain.cpp:106-109).  stage_mask bit i enables stage i; reading synchronises.
 * Stages: 0 pyramid(+CLAHE) 1 orb_prepare 2 lk_fwd 3 lk_rev 4 orb_gate 5 ransac_commit 6 min_eigen
 * 7 gftt_select(mask,max,candidates,select) 8 feature_msg.  LK/ORB/RANSAC stages sum old+new launches.
 * Bits 16..23 of stage_mask: bracket every n-th frame only (0 or 1: every frame) - an event record is a barrier packet on the frame's
 * dependent chain, so a measurement that must not slow what it measures samples (bench.py: every 5th frame). */
#define LVK_FE_STAGES 9
lvk_status lvk_frontend_profile_enable(lvk_frontend* fe, unsigned stage_mask);
lvk_status lvk_frontend_profile_read(lvk_frontend* fe, double ms_sum[LVK_FE_STAGES], uint64_t launches[LVK_FE_STAGES], int reset);
const char* lvk_frontend_stage_name(int stage);

/* ------------------------------------------------------------------ stage entries of the frame path
 * The three kinds of launch a steady-state frame queues, each on a caller's HOST arrays through the very launch code lvk_frontend_process
 * uses (stage parity; no reference counterpart beyond the functions cited).  Each call checks everything on the host before it queues
 * anything, allocates its device buffers for the call, and returns after a wait for the context's stream.  Refusals leave every output
 * array untouched and the context usable.  Status codes in the per-point status byte: 0 alive, 1 lost by the forward pass, 2 by the
 * reverse pass, 3 by the descriptor gate.
 *
 * lvk_fe_track_stage: forward LK from the H-predicted start, in-image test, reverse LK, <= 1 px round trip, descriptor gate (> 58 bits
 * fails) and the K -> K undistorted pair of every point (trackFeatures image_processor.cpp:558-712, trackNewFeatures :830-943) in ONE
 * launch: variant 1 = k_fe_lk_both<patch_size> (two wavefronts per point), variant 2 = k_fe_lk_pipe<21> (five).  The variant is the
 * caller's, LVK_LK_VARIANT is not read.  prev / next: built pyramids of width x height created with win = patch_size; d_*_ext / d_*_blur:
 * their lvk_orb_prepare planes.  A set is n points in `grid` slots (= blocks; the frame path launches one per track slot): blocks >= n
 * must write nothing, which a caller sees because every output array is filled with fill_byte before the launch.  is_new = 0: the gate
 * compares with h_stored_desc (n x 4 words); 1: with the previous-image descriptor, which is written to h_desc (grid x 4).  Per slot:
 * h_curr = the forward result whatever the status, h_und[2p] = the undistorted source point, h_und[2p + 1] = the undistorted forward
 * result - written only when the forward pass succeeded.  set1 (may be NULL, variant 2 only): a second set in the same launch, blocks
 * [grid0, grid0 + grid1) - the frame path's LVK_LK_MERGED launch.  h_counters[2]: lk_point_levels and lk_iterations, in / out.
 * LVK_ERR_ARG: a null pointer that is needed, n < 0 or n > grid, is_new not 0 / 1, pyramids not width x height or not built with win =
 * patch_size, a variant other than 1 / 2, a second set with variant 1, H or the camera not finite, a model other than 0 / 1, a source
 * point that is not finite or outside [0, width - 1] x [0, height - 1] (the descriptor wavefront reads the mosaic around it
 * unconditionally).  LVK_ERR_CAPACITY: grid > 4096.  LVK_ERR_UNSUPPORTED: patch_size not 15 / 21 / 31, variant 2 with another window
 * than 21 or with a pyramid of more than 4 levels (the templates it keeps in LDS). */
typedef struct {
    int n, grid, is_new;
    const lvk_pt2f* h_src_pts;          /* n */
    const uint64_t* h_stored_desc;      /* n x 4, is_new = 0 */
    lvk_pt2f* h_curr;                   /* out, grid */
    uint8_t*  h_status;                 /* out, grid */
    lvk_pt2f* h_und;                    /* out, grid x 2 */
    uint64_t* h_desc;                   /* out, grid x 4, is_new = 1 */
} lvk_fe_track_io;
lvk_status lvk_fe_track_stage(lvk_context* ctx, const lvk_pyramid* prev, const lvk_pyramid* next, const uint8_t* d_prev_ext, const uint8_t* d_prev_blur,
                              const uint8_t* d_next_ext, const uint8_t* d_next_blur, int width, int height, int patch_size, int variant, const float H[9],
                              int model, const double intr[4], const double dist[4], int max_iteration, double track_precision, int fill_byte,
                              const lvk_fe_track_io* set0, const lvk_fe_track_io* set1, uint64_t h_counters[2]);

/* lvk_fe_commit_stage: k_fe_ransac_commit - ordered compaction of the alive points, the modes' failure rules, the cv::findFundamentalMat
 * mask on their undistorted pairs (fewer than 7: none, everything is kept; 7: all ones; 8..14 LMedS; 15 and more RANSAC) and the ordered
 * write of the destination set.  mode 0 = old tracks (trackFeatures :701-808: the set is replaced, id and init carried, life + 1),
 * 1 = new points appended behind dst_n (trackNewFeatures :932-1001: fails - nothing changes - with fewer than 20 alive or none kept),
 * 2 = bootstrap (initializeFirstFeatures :464-536: needs 20 after the forward pass, after the reverse pass, after the gate and after the
 * mask; boot_ok says which way it went, failure leaves dst_n = 0).  One workgroup: 512 threads when cap > 512, otherwise 256 - by the
 * slot count cap, as the frame path chooses, not by n.  All source arrays hold n entries (h_und n x 2, h_src_desc n x 4; h_src_id,
 * h_src_init, h_src_life: mode 0 only), h_dst's arrays cap slots each, in / out.  h_state in / out; in modes 1 and 2 the kernel's count
 * IS n_new, as in a frame, so n_new must equal n on entry.
 * Mode 1 at a full set: slots >= cap are never written and dst_n stops at cap, but next_id advances by the UNCLIPPED count of kept points
 * - ids are consumed by points that found no slot.  (The frame path never gets there: detection asks for cap - dst_n corners at most.)
 * LVK_ERR_ARG: mode outside 0..2, cap < 1, n < 0, a null pointer that is needed, dst_n outside [0, cap], n_new != n in modes 1 / 2, a
 * status byte above 3, an undistorted point that is not finite.  LVK_ERR_CAPACITY: cap > 4096 (the kernel's LDS), n > cap. */
typedef struct {                        /* a track set in host arrays */
    uint64_t* id; lvk_pt2f* pts; lvk_pt2f* ppts; lvk_pt2f* init; int* life;
    uint64_t* desc;                     /* 4 words per slot */
} lvk_fe_track_arrays;
typedef struct { uint64_t next_id; int dst_n, n_new, boot_ok; } lvk_fe_commit_state;
lvk_status lvk_fe_commit_stage(lvk_context* ctx, int mode, int cap, int n, const lvk_pt2f* h_src_pts, const lvk_pt2f* h_curr, const uint8_t* h_status, const lvk_pt2f* h_und,
                               const uint64_t* h_src_id, const lvk_pt2f* h_src_init, const int* h_src_life, const uint64_t* h_src_desc,
                               const lvk_fe_track_arrays* h_dst, lvk_fe_commit_state* h_state);

/* lvk_fe_msg_stage: k_fe_msg - getFeatureMsg (:1076-1128) of the first n of a set's cap slots, ceil(cap / 64) blocks of 64 threads as the
 * frame path launches it.  Reads h_set's id, pts, ppts and init (cap entries each; life and desc may be NULL); writes h_out[i] for i < n
 * (h_out: cap entries, filled with fill_byte before the launch) and resets init[i] to (-1, -1) where it was a real point.  h_state in /
 * out: n_msg and n_host become n, msg_features grows by n, msg_count by one.
 * LVK_ERR_ARG: cap < 1, n < 0, a null pointer, prev_is_last not 0 / 1, a dt or the camera not finite, a model other than 0 / 1.
 * LVK_ERR_CAPACITY: cap > 4096, n > cap. */
typedef struct { int n_msg, n_host; uint64_t msg_features, msg_count; } lvk_fe_msg_state;
lvk_status lvk_fe_msg_stage(lvk_context* ctx, const lvk_fe_track_arrays* h_set, int cap, int n, int model, const double intr[4], const double dist[4],
                            double dt_1, double dt_2, int prev_is_last, int fill_byte, lvk_feature_obs* h_out, lvk_fe_msg_state* h_state);

/* ==================================================================== back-end: EKF measurement update
 * replaces larvio::LarVio (include/larvio/larvio.h:37-90).  feature_idp_dim = 1, use_schmidt = 0,
 * calib_imu_instrinsic = 0 or 1 (config/euroc.yaml:8-10,105,108) are implemented; other values are refused.
 * Matrices crossing the ABI are ROW-MAJOR doubles with an explicit leading dimension (P is symmetric, so the
 * reference's column-major Eigen::MatrixXd state_cov maps onto it unchanged). */
typedef struct lvk_ekf lvk_ekf;

/* stage level (device pointers): the dense algebra of measurementUpdate_msckf / _hybrid (larvio.cpp:1430-1460,1578-1594) */
/* [H | r] (rows x cols) -> top `cols` rows of Q^T [H | r], in place (SPQR replacement, larvio.cpp:1430-1445). */
lvk_status lvk_ekf_compress_qr(lvk_context* ctx, double* d_H, int ld, int rows, int cols, double* d_r, int* rows_out);
/* The same compression when the caller knows the block structure of H (as the filter does: a feature's rows touch the extrinsics / td
 * columns and the 6-column blocks of the clones that observed it - the sparsity SPQR exploits in the reference).  The rows come in
 * n_groups consecutive groups; group i has h_rows[i] rows that are zero outside the ascending columns
 * h_cols[h_col_off[i] .. h_col_off[i+1]).  A TSQR tree over consecutive groups whose column union fits one workgroup's LDS is planned on
 * the host and run level by level (work ~ 2 r c^2 with c = columns per node instead of 2 r cols^2).  Result in place at the top of
 * d_H / d_r, *rows_out rows (>= cols possible: finish with lvk_ekf_compress_qr).  lvk_ekf_qr_plan is the host-only planning step
 * (no device needed): blocks as 8 ints {in_start, in_rows, out_start, out_rows, ncols, col_off, copy, 0} level after level. */
lvk_status lvk_ekf_compress_qr_groups(lvk_context* ctx, double* d_H, int ld, int rows, int cols, double* d_r, int n_groups,
                                      const int* h_rows, const int* h_col_off, const int* h_cols, int* rows_out);
int        lvk_ekf_qr_plan(int N, int n_groups, const int* h_rows, const int* h_col_off, const int* h_cols, int* h_blocks, int cap_blocks,
                           int* h_block_cols, int cap_cols, int* h_level_blocks, int* h_level_cols, int cap_levels, int* final_rows);
/* S = H P H^T + sigma2 I ; dx = P H^T S^-1 r ; P <- (I - K H) P symmetrised.  H is m x n (ldh), P n x n (ldp).
 * Replaces larvio.cpp:1453-1460, 1578-1594.  Waits for the update: LVK_ERR_NUMERIC when S is not positive definite.  d_P and d_dx
 * are then exactly what they were before the call (the launch that would write them reads the factorisation's report first), so
 * the same arguments can go to lvk_ekf_update_ldlt, which goes on as the reference's pivoted LDLT does. */
lvk_status lvk_ekf_update(lvk_context* ctx, double* d_P, int ldp, int n, const double* d_H, int ldh, int m,
                          const double* d_r, double sigma2, double* d_dx);
/* The same update through an LDL^T factorisation of S with diagonal pivoting (at every step the remaining diagonal entry of largest
 * magnitude, the first one on a tie), for an S that need not be positive definite - S.ldlt().solve(H P) of larvio.cpp:1456:
 *     K = (S^-1 H P)^T ;  dx = K r ;  P <- (I - K H) P ;  P <- (P + P^T) / 2.
 * A D entry of magnitude <= DBL_MIN gives a zero component of the solution instead of a division.  Always the pivoted route, also for
 * a positive definite S.  h_info (host, 2 ints): [0] the number of negative, [1] of zero D entries.  Waits for its launch.
 * LVK_ERR_ARG for bad arguments, LVK_ERR_CAPACITY (nothing launched) when m rows do not fit the factor kernel's LDS (m > ~1100). */
lvk_status lvk_ekf_update_ldlt(lvk_context* ctx, double* d_P, int ldp, int n, const double* d_H, int ldh, int m,
                               const double* d_r, double sigma2, double* d_dx, int* h_info);
/* ... also returning the pivot order: h_perm (host, m ints), row i of the factor is row h_perm[i] of S (parity tests) */
lvk_status lvk_ekf_update_ldlt_perm(lvk_context* ctx, double* d_P, int ldp, int n, const double* d_H, int ldh, int m,
                                    const double* d_r, double sigma2, double* d_dx, int* h_info, int* h_perm);
/* C = alpha op(A) op(B) + beta C on the FP64 matrix cores (v_mfma_f64_16x16x4_f64) — the P H^T-class contraction.  Row-major; A is stored
 * M x K (K x M when transa), B K x N (N x K when transb), C M x N.  LVK_ERR_ARG (nothing launched) for a negative dimension or a leading
 * dimension below the stored row length of its operand.  K = 0 is legal and gives C = beta C; beta = 0 never reads C. */
lvk_status lvk_dgemm(lvk_context* ctx, int transa, int transb, int M, int N, int K, double alpha, const double* d_A, int lda,
                     const double* d_B, int ldb, double beta, double* d_C, int ldc);
/* ... with the riders the measurement update hangs on its products (nothing else differs from lvk_dgemm):
 *   diag_add          added to the entries with row == col;
 *   d_xin, xin_col    (optional) M doubles copied into column xin_col of C's buffer, 0 <= xin_col < ldc ([H P | r] in one launch; the
 *                     column may lie outside the N computed ones, and must when both are wanted);
 *   d_xout, xout_col  (optional) output column xout_col (0 <= xout_col < N) goes to d_xout (M doubles) as the plain sum - no alpha, beta
 *                     or diag_add - and that column of C is left as it was (dx = W^T w next to P -= W^T W);
 *   d_gate            (optional) two ints in device memory: when either is non-zero the products write neither C nor d_xout (the
 *                     d_xin column is still copied). */
lvk_status lvk_dgemm_ex(lvk_context* ctx, int transa, int transb, int M, int N, int K, double alpha, const double* d_A, int lda,
                        const double* d_B, int ldb, double beta, double* d_C, int ldc, double diag_add, const double* d_xin, int xin_col,
                        double* d_xout, int xout_col, const int* d_gate);
/* The factor-and-solve of lvk_ekf_update on caller-owned device buffers: S = L L^T (m x m, lds) and B <- W = L^-1 B (m x nbcols, ldb),
 * both in place, in 32-row panels inside 160-row super-blocks [S11 . ; . S22]: each super-block is one fused launch (factor S11, solve
 * its rows of B, and L21^T = L11^-1 S12), followed by S22 -= L21 L21^T and B2 -= L21 W1.  Waits for its launches.
 * READ of S: the super-block's diagonal part and everything to its RIGHT, never what lies below-left of a super-block.  Inside a
 *   super-block: the 32 x 32 blocks below the diagonal ones; of a diagonal 32 x 32 block its two 16 x 16 diagonal tiles' UPPER triangles
 *   (diagonal included; the kernel takes row j for column j) and the 16 x 16 tile below-left of them.  For an exactly symmetric S this
 *   is its lower triangle inside a super-block plus the blocks to the right.  Everything else - the rest of the diagonal blocks, the
 *   blocks above them inside a super-block, the part below-left of a super-block, columns >= m - may hold anything, NaN included.
 * DEFINED in S afterwards: the 32 x 32 blocks of L below the diagonal blocks of their super-block (rows < m), and L21^T in S12 (the
 *   rows of a super-block, the columns right of it).  The diagonal blocks of L are NOT stored (the solves multiply with their inverses,
 *   which stay in scratch memory); the rest of S holds intermediate values.  Columns >= m of S and >= nbcols of B are not written.
 * h_info (host, 2 ints): [0] = 1 + the first row whose pivot was not positive (it is replaced by 1 and the launch goes on), 0 for a
 *   positive definite S; [1] = non-zero when a solver workgroup gave up waiting for a panel (a broken device).  Neither is an error here.
 * LVK_ERR_ARG unless m >= 0, nbcols >= 0, lds >= m, ldb >= nbcols, lds is a multiple of 4 and d_S is 32-byte aligned: rows of S are
 *   read and written as 32-byte vectors of 4 doubles starting at columns that are multiples of 4, so every row must start 32-byte
 *   aligned, and a row length that is no multiple of 4 would cut the last vector of a row short.  B is accessed by scalars. */
lvk_status lvk_chol_solve(lvk_context* ctx, double* d_S, int lds, int m, double* d_B, int ldb, int nbcols, int* h_info);

/* The structural covariance operations the filter runs on its device-resident P between updates, one call each (parity tests;
 * callers that want a single stage).  P is row-major with an explicit leading dimension; Pin and Pout are different buffers.  Each
 * call waits for its launch.  LVK_ERR_CAPACITY (with a message, nothing launched, the context stays usable) for sizes the kernels'
 * LDS cannot hold: the propagation's strip above 160 KB, n + 256 doubles above 64 KB for the re-anchoring and the append.
 *
 * lvk_ekf_cov_propagate_augment: processModel's covariance part (larvio.cpp:553-571: P_II <- Phi P_II Phi^T + Q, P_IC <- Phi P_IC,
 *   symmetrised) followed by stateAugmentation (:752-798: the new clone's six rows and columns are copies of rows {0,1,2,6,7,8}),
 *   in one launch.  Pin is (n_out - 6) x (n_out - 6): the IMU block (L = 22, or 46 with IMU intrinsics), clones up to pose_rows,
 *   in-state features after them; the new clone is inserted at pose_rows of Pout (n_out x n_out).  h_phi, h_q: L x L, row-major, on
 *   the host.  For L = 22 Phi's rows 9..21 must be identity rows and Q zero outside its leading 15 x 15 (the composed transition
 *   always is; the kernel receives only what that leaves): anything else is LVK_ERR_ARG.
 * lvk_ekf_cov_gather: Pout[a][b] = Pin[idx[a]][idx[b]], a, b < n, 0 <= idx < ldin (clone augmentation without propagation,
 *   :752-798; clone deletion :2563-2638; deletion of lost in-state features :3311-3327).
 * lvk_ekf_cov_reanchor: an in-state feature moves to a new anchor (updateFeatureCov_1didp, :3125-3293): row and column fc of the
 *   n x n P become J P, entry (fc, fc) J P J^T; J (n doubles, host) has at most 64 non-zeros (LVK_ERR_ARG otherwise).
 * lvk_ekf_cov_append_features: delayed initialisation of nn new 1-D in-state features (:1821-1854).  HH = diag(H2)^-1 H1 (H1: nn x n,
 *   ldh; H2: nn doubles on the host); rows and columns n..n+nn-1 of P (ld >= n + nn) become -HH P and HH P HH^T + sigma2 / H2^2
 *   (diagonal); d_dx_new (nn) = -HH dx + r1 / H2.  The old n x n block is not touched. */
lvk_status lvk_ekf_cov_propagate_augment(lvk_context* ctx, const double* d_Pin, int ldin, double* d_Pout, int ldout, int n_out, int pose_rows,
                                         int L, const double* h_phi, const double* h_q);
lvk_status lvk_ekf_cov_gather(lvk_context* ctx, const double* d_Pin, int ldin, double* d_Pout, int ldout, const int* h_idx, int n);
lvk_status lvk_ekf_cov_reanchor(lvk_context* ctx, double* d_P, int ld, int n, const double* h_J, int fc);
lvk_status lvk_ekf_cov_append_features(lvk_context* ctx, double* d_P, int ld, int n, int nn, const double* d_H1, int ldh, const double* h_H2,
                                       const double* d_r1, const double* d_dx, double sigma2, double* d_dx_new);

/* Position covariance of anchored inverse-depth landmarks, one 3 x 3 matrix per job, read off a device-resident covariance (n x n,
 * row-major, leading dimension ldp) without moving it.  Sigma is the first-order covariance of the landmark's world position
 *   p_w = R_c2w [u/rho, v/rho, 1/rho] + p_cam,   R_c2w = R(q_anchor) R_b2c^T,   p_cam = p_anchor + R(q_anchor) t_c_b
 * (R_c2w goes through Eigen's matrix -> quaternion -> matrix conversions, as the filter keeps a clone's camera attitude: with an
 * R_b2c that is orthonormal to the digits of a configuration file only, that is the matrix Feature::position was formed with)
 * under an error state delta ~ N(0, P) applied exactly as the filter's state injection applies a correction (larvio.cpp:1476-1575):
 *   anchor clone attitude   q <- small_angle_quat(d_theta) * q          (Hamilton, [x y z w]; R(q) maps body to world)
 *   anchor clone position   p <- p + d_p
 *   extrinsic rotation      R_b2c <- R_b2c R(small_angle_quat(d_theta_e))^T
 *   extrinsic translation   t_c_b <- t_c_b + d_t
 *   inverse depth           rho <- rho + d_rho
 * Thirteen columns of P matter: the extrinsics' 15..20 (d_theta_e, d_t), the anchor clone's six from anchor_col (d_theta, d_p) and the
 * feature's feat_col; Sigma = J P[those, those] J^T with, for R = R(q_anchor), r_c = p_w - p_cam and r = p_w - p_anchor,
 *   J = [ -[r_c]x R | R | -[r]x | I | -r_c / rho ].
 * Nothing outside those 13 rows and columns of P is read; every sum runs in a fixed order (the same input gives the same bits) and
 * the lower triangle is a copy of the upper one.  h_cov9: 9 doubles per job, row-major.  The call waits for its launch.
 * LVK_ERR_ARG, with nothing launched and the context still usable, when a pointer is null, n_jobs < 0, ldp < n, a job's column range
 * (15..20, anchor_col..anchor_col+5, feat_col) leaves [0, n), or its inv_depth is 0.  n_jobs == 0 is LVK_OK. */
typedef struct { int anchor_col, feat_col, pad0, pad1;      /* first of the anchor clone's 6 columns; the feature's column */
                 double q_anchor[4], R_b2c[9], t_c_b[3];    /* the anchor clone's IMU attitude as lvk_clone.q; extrinsics as lvk_ekf_get_state */
                 double obs_anchor[2], inv_depth; } lvk_landmark_job;
lvk_status lvk_ekf_landmark_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_landmark_job* h_jobs, int n_jobs, double* h_cov9);

/* Covariance of one pose relative to another (and the absolute 6 x 6 block of one pose), one 6 x 6 matrix per job, read off a
 * device-resident covariance (n x n, row-major, leading dimension ldp) without moving it.  The error state is the one the filter's
 * state injection applies (larvio.cpp:1476-1575):
 *   attitude   q <- small_angle_quat(d_theta) * q     (Hamilton, [x y z w]; R(q) maps body to world), i.e. R <- (I + [d_theta]x) R
 *   position   p <- p + d_p
 * A clone's columns are leg_dim + 6 c (d_theta) and leg_dim + 6 c + 3 (d_p); the IMU state's are 0..2 and 6..8 (velocity sits between
 * them), which is why a job names the first d_theta column and the first d_p column of each pose separately.
 * For two poses a, b:  R_ab = R_a^T R_b,  p_ab = R_a^T (p_b - p_a),  d = p_b - p_a.  The error of the relative pose is defined by
 *   R_ab,true = (I + [d_phi]x) R_ab,   p_ab,true = p_ab + d_rho,
 * and to first order, under the injection above,
 *   d_phi = R_a^T (d_theta_b - d_theta_a),   d_rho = R_a^T [d]x d_theta_a + R_a^T (d_p_b - d_p_a).
 * With the column order [d_theta_a d_p_a d_theta_b d_p_b] and the output order [d_phi; d_rho], Sigma_rel = J P[those, those] J^T with
 *   J = [ -R_a^T       0      R_a^T  0
 *          R_a^T [d]x  -R_a^T  0      R_a^T ].
 * (The signs were confirmed against inject() by central differences of (log(R_ab' R_ab^T), p_ab' - p_ab) under that injection:
 * tests/pose_rel_ref.py; they agree with the form above.)  A rigid motion of the world (d_theta_a = d_theta_b = theta,
 * d_p_x = [theta]x p_x + t) gives d_phi = d_rho = 0: the four unobservable directions of a VIO, in which the absolute covariance
 * grows without bound, cancel in Sigma_rel.
 * An ABSOLUTE job (a_theta_col < 0; a_p_col, q_a, p_a, q_b, p_b unused) returns the 6 x 6 block of b in the order [d_theta_b d_p_b]: a
 * pure gather, bit for bit the entries of P (so as symmetric as P is).
 * Nothing outside the job's twelve (six) rows and columns of P is read; every sum runs in a fixed order (the same input gives the
 * same bits); for a relative job the lower triangle is a copy of the upper one.  q_b is not used by the covariance (it is part of
 * the job so that one record describes both poses).  h_cov36: 36 doubles per job, row-major.  The call waits for its launch.
 * LVK_ERR_ARG, with nothing launched and the context still usable, when a pointer is null, n_jobs < 0, ldp < n, or a column triple
 * a job names (c..c+2 for each of its four - absolute: two - columns) leaves [0, n).  n_jobs == 0 is LVK_OK. */
typedef struct { int a_theta_col, a_p_col, b_theta_col, b_p_col;   /* first of three columns each; a_theta_col < 0: absolute job */
                 double q_a[4], p_a[3], q_b[4], p_b[3]; } lvk_pose_rel_job;
lvk_status lvk_ekf_pose_rel_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_pose_rel_job* h_jobs, int n_jobs, double* h_cov36);

/* Anchored inverse-depth landmarks in the CAMERA frame of a target pose, with their 3 x 3 covariance there, one per job, read off a
 * device-resident covariance (n x n, row-major, leading dimension ldp) without moving it.  The world-frame Sigma of
 * lvk_ekf_landmark_cov contains the four directions a VIO cannot observe (global position and yaw), which grow without bound; the
 * point relative to a camera of the window does not: here they cancel, as they do in lvk_ekf_pose_rel_cov.
 * The point's world position p_w is exactly that of lvk_ekf_landmark_cov (the same anchored inverse-depth form, the same
 * R(q_anchor) R_b2c^T taken through a quaternion and back), with p_cam = p_anchor + R(q_anchor) t_c_b.  For a target pose b
 * (attitude q_b, position p_b, body to world) the point in b's camera frame is
 *   p_c = R_b2c ( R_b^T (p_w - p_b) - t_c_b ).
 * The error state is the one the filter's state injection applies (the conventions are stated at lvk_ekf_landmark_cov and
 * lvk_ekf_pose_rel_cov): clone and IMU attitude R <- (I + [d_theta]x) R, position p <- p + d_p, extrinsic rotation
 * R_b2c <- R_b2c R(small_angle_quat(d_theta_e))^T, extrinsic translation t_c_b <- t_c_b + d_t, inverse depth rho <- rho + d_rho.
 * Nineteen columns of P matter, in this order:
 *   [ d_theta_e d_t (15..20) | d_theta_a d_p_a (anchor_col..+5) | d_theta_b (b_theta_col..+2) | d_p_b (b_p_col..+2) | d_rho (feat_col) ].
 * The target's d_theta and d_p columns are named separately, as in lvk_pose_rel_job: the target may be the IMU state (0 and 6) or any
 * clone (leg_dim + 6 c and + 3).  Sigma = J P[those, those] J^T with, for R_a = R(q_anchor), M = R_b2c R_b^T, f_A = [u v 1] / rho,
 * x = R_b2c^T f_A, r_c = p_w - p_cam,anchor (= R_a x), r = p_w - p_anchor, g = p_w - p_b and y = R_b^T g - t_c_b,
 *   J = [ R_b2c [y]x - M R_a [x]x | M R_a - R_b2c | -M [r]x | M | M [g]x | -M | -M r_c / rho ].
 * (Confirmed against inject() by central differences of p_c under that injection: tests/landmark_rel_ref.py; they agree with the
 * form above.)  A rigid motion of the world (d_theta_a = d_theta_b = theta, d_p_x = [theta]x p_x + t) gives d p_c = 0.  With the target
 * equal to the anchor clone (the same columns named twice - legal) every block but the last cancels: Sigma = sigma_rho^2 f_A f_A^T / rho^2.
 * g is formed as r + (p_anchor - p_b): the two positions are subtracted first, so that the size of the world coordinates does not
 * enter the rounding of p_c.
 * Nothing outside those 19 rows and columns of P is read; every sum runs in a fixed order (the same input gives the same bits) and
 * the lower triangle is a copy of the upper one.  h_out12: 12 doubles per job - p_c (3), then Sigma (9, row-major).  The call waits
 * for its launch.
 * LVK_ERR_ARG, with nothing launched and the context still usable, when a pointer is null, n_jobs < 0, ldp < n, a job's column range
 * (15..20, anchor_col..anchor_col+5, b_theta_col..+2, b_p_col..+2, feat_col) leaves [0, n), or its inv_depth is 0.  n_jobs == 0 is
 * LVK_OK. */
typedef struct { int anchor_col, feat_col, pad0, pad1;      /* as lvk_landmark_job, field for field ... */
                 double q_anchor[4], R_b2c[9], t_c_b[3];
                 double obs_anchor[2], inv_depth;
                 int b_theta_col, b_p_col;                  /* ... then the target: first of its three d_theta columns, first of its three d_p columns */
                 double q_b[4], p_b[3], p_anchor[3]; } lvk_landmark_rel_job;   /* the target's pose; the anchor clone's position as lvk_clone.p */
lvk_status lvk_ekf_landmark_rel_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_landmark_rel_job* h_jobs, int n_jobs, double* h_out12);

/* lvk_ekf_update_sparse: one measurement of 3 or 6 rows that touches at most 12 columns of the state and carries a full noise
 * covariance, applied to a device-resident covariance (n x n, row-major, leading dimension ldp) without a dense H, a GEMM or a whitening
 * step - the update an external position or pose fix needs (lvk_ekf_add_fix).  No reference counterpart: the reference has no such input.
 *   S = H P[cols, cols] H^T + R = L L^T,   gamma = r^T S^-1 r,   W = L^-1 H P[cols, :],   dx = W^T L^-1 r,   P <- P - W^T W.
 * H is m x ncols, packed row-major (row stride ncols); R is m x m, packed row-major (row stride m), and only its upper triangle,
 * diagonal included, is read - S is formed as its upper triangle and mirrored.  Entries of cols and H beyond ncols, of r beyond m and
 * of R beyond m x m are never read and may hold anything.
 * Two launches and one wait.  The first forms, in every workgroup by itself and therefore with the same bits everywhere, S from the
 * ncols x ncols sub-block of P, its Cholesky factor, gamma and the status, then its own 64 columns of W (to a work space) and of dx.
 * The second subtracts W^T W, one entry of P per thread, and does nothing unless the status is 0: the gate is decided on the device.
 * No kernel writes what a sibling workgroup of the same launch reads.  Every sum runs in a fixed order (the same input gives the
 * same bits), and P[i][j] and P[j][i] are formed from the same operands in the same order: a symmetric P stays symmetric bit for bit.
 * Nothing of P outside [0, n) x [0, n) is read or written: the padding of a wider ldp keeps its bytes.
 * h_dx: n doubles.  h_info4: [0] status - 0 applied, 1 gated out (gate > 0 and not gamma <= gate), 2 S not positive definite (a
 * pivot that is not > 0); [1] gamma (0 with status 2); [2] the smallest pivot met (the diagonal entry of the reduced S whose square
 * root is L_ii; with status 2 the failing one); [3] 0.  With status 1 or 2 not one byte of P changes and dx is all zeros.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer, m not 3 or 6, ncols outside 1..12, columns that
 * do not ascend strictly or leave [0, n), ldp < n, or a value that is not finite among gate and the entries of H, r and R that are read. */
typedef struct { int m;            /* 3 or 6 rows */
                 int ncols;        /* 1..12 distinct columns, ascending */
                 int cols[12];
                 double H[6*12];   /* row-major m x ncols */
                 double r[6], R[36];  /* residual; full SPD noise covariance, m x m row-major */
                 double gate; }    /* accept iff r' S^-1 r <= gate; <= 0: no gate */
        lvk_sparse_update;
lvk_status lvk_ekf_update_sparse(lvk_context* ctx, double* d_P, int ldp, int n, const lvk_sparse_update* h_u,
                                 double* h_dx /* n */, double* h_info4);

/* lvk_ekf_update_landmarks: up to 1024 image observations, all made in ONE image - of one clone b of the window - of points whose world
 * position is known (surveyed fiducials, the points of an earlier session, a prior map), fused directly into a device-resident
 * covariance (n x n, row-major, leading dimension ldp) - the update behind lvk_ekf_add_landmark_obs.  No reference counterpart.
 * Conventions (those of lvk_ekf_landmark_rel_cov and lvk_ekf_pose_rel_cov): R(q) maps body to world, the injection is
 * R_b <- (I + [d_theta_b]x) R_b, p_b <- p_b + d_p_b, R_b2c <- R_b2c R(d_theta_e)^T, t_c_b <- t_c_b + d_t; the clone has columns
 * clone_col .. clone_col + 5 (d_theta_b, d_p_b), the extrinsics 15..20 (d_theta_e, d_t).  For a world point p_w with covariance
 * Sigma_w, a normalised image observation z = (u, v) and pixel noise sigma (in normalised units):
 *   g = p_w - p_b,   y = R_b^T g - t_c_b,   p_c = R_b2c y,   h = (p_c.x / p_c.z, p_c.y / p_c.z),   r = z - h
 * (g is that subtraction before anything else: the size of the world coordinates stays out of the rounding).  Twelve columns of P
 * matter, in ascending order: 15..20, then the clone's six.  With M = R_b2c R_b^T the derivative of p_c is that of
 * lvk_ekf_landmark_rel_cov with the anchor terms dropped,
 *   d p_c = [R_b2c [y]x | -R_b2c | M [g]x | -M] [d_theta_e; d_t; d_theta_b; d_p_b],   d p_c / d p_w = M,
 *   H = J (d p_c) (2 x 12),  J = [1/z 0 -x/z^2; 0 1/z -y/z^2],   R_k = sigma^2 I + J M Sigma_w M^T J^T
 * (Sigma_w may be all zeros; only its upper triangle, diagonal included, is read).  The extrinsics columns are always named: when
 * the extrinsics are not estimated their block of P is zero and they drop out.  (The signs were confirmed against the injection by
 * central differences: tests/landmark_fix_ref.py.)
 * On the covariance as it is before the batch, observation by observation: p_c.z <= min_depth: BEHIND, nothing else is computed for
 * it (no division, no NaN), gamma_k = 0.  Otherwise gamma_k = r^T (H P_s H^T + R_k)^-1 r (P_s: the 12 x 12 sub-block), and with
 * gate > 0 the observation is USED iff gamma_k <= gate, else GATED (a pivot of that 2 x 2 that is not > 0 - possible only with an
 * indefinite P - counts as GATED with gamma_k = 0, and so does a pivot of R_k that is not > 0: a Sigma_w so many orders above sigma^2
 * that rounding leaves R_k indefinite).  The rows of a used observation are whitened by the Cholesky factor of R_k (unit
 * noise) and stacked, in the batch's order, as 2 n_used x 12 with the residual as a thirteenth column.  More than 12 rows are
 * compressed by Householder reflections applied to [0 (12 x 13); A]: reflection j involves row j of the zero block and all of A
 * (so its arithmetic is a_j.a_k / |a_j| for the new row and a_k - (a_j.a_k / a_j.a_j) a_j for what remains: no Gram matrix is formed
 * or factored, PARITY.md records why not).  The twelve columns act through the camera's pose alone, so the rows have rank 6 at the
 * most, and the rank is decided on the device: a column of which the reflections before it have left no more than 2^-60 of its
 * squared norm depends on them and gives no row (what it keeps is rounding, 1e-30 of the squared norm; an independent direction keeps
 * 1e-6 and more).  The compressed system has as many rows as the stacked one has rank - 6 for points in general position - and none
 * of rounding noise.  The part of the residual outside the range of the rows is dropped, as in every compression of the filter: the
 * batch's gamma of a compressed batch is that of the part inside it.
 * Then, m <= 12 rows:  S = H P_s H^T + I = L L^T,  W = L^-1 H P[cols, :],  dx = W^T L^-1 r,  P <- P - W^T W.
 * Three launches and one wait.  The first, one workgroup with one lane per observation, forms rows, gates, whitens and compresses;
 * the second (one wavefront per 64 columns, every workgroup forming S, L and y by itself with the same bits) writes W and dx; the
 * third subtracts W^T W.  Every sum runs in a fixed order: the same input gives the same bits, the per-observation results do not
 * depend on where an observation stands in the batch, and the compressed system depends on the used observations and their order
 * only - a batch and the same batch without its gated and behind observations give the same dx and P bit for bit.  No floating-point
 * atomics.  P[i][j] and P[j][i] are formed from the same operands in the same order: a symmetric P stays symmetric bit for bit.  No
 * kernel writes what a sibling workgroup of the same launch reads.  "Nothing to apply" is decided on the device: with n_used = 0 or a
 * pivot of S that is not > 0 not one byte of P changes and dx is all zeros.  Before the second launch nothing of P outside the twelve
 * rows AND columns is read (and with nothing to apply nothing ever is); nothing outside [0, n) x [0, n) is read or written at all.
 * h_dx: n doubles.  h_info8: [0] batch status - 0 applied, 1 all rejected (n_used = 0), 2 S not positive definite; [1] the batch's
 * gamma = |L^-1 r|^2 of the system that was applied (0 unless applied); [2] the smallest pivot of S (with status 2 the failing one, 0
 * with status 1); [3] n_used [4] n_gated [5] n_behind [6] rows m after compression (2 n_used up to 6 used observations, else the rank) [7] 0.
 * h_status[n_obs]: 0 used, 1 gated, 2 behind.  h_gamma[n_obs]: gamma_k.
 * At most 1024 observations: LVK_ERR_CAPACITY beyond.  n_obs == 0 is LVK_OK, launches nothing and writes nothing (h_obs may be null).
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer, ldp < n, clone_col < 21 or clone_col + 6 > n, a
 * value that is read and is not finite, sigma <= 0, a cov_w whose upper triangle is not positive semi-definite (its principal minors,
 * on the host), |q_b| off 1 by more than 1e-6, min_depth < 0. */
#define LVK_LANDMARK_USED   0
#define LVK_LANDMARK_GATED  1
#define LVK_LANDMARK_BEHIND 2
typedef struct { int clone_col, pad0;            /* first of the clone's six columns */
                 double q_b[4], p_b[3];          /* the clone's pose */
                 double R_b2c[9], t_c_b[3];      /* the extrinsics, as lvk_ekf_get_state hands them out */
                 double gate;                    /* an observation is used iff gamma_k <= gate; <= 0: no gate */
                 double min_depth; }             /* p_c.z <= min_depth: behind */
        lvk_landmark_fix_job;
typedef struct { double p_w[3], cov_w[9];        /* world point and its covariance (row-major; the upper triangle is read) */
                 double uv[2], sigma; }          /* normalised image observation and its standard deviation */
        lvk_landmark_obs;
lvk_status lvk_ekf_update_landmarks(lvk_context* ctx, double* d_P, int ldp, int n, const lvk_landmark_fix_job* h_job,
                                    const lvk_landmark_obs* h_obs, int n_obs, double* h_dx /* n */, double* h_info8,
                                    int* h_status /* n_obs */, double* h_gamma /* n_obs */);

/* Stage entry: the camera pose of one clone of the window and its covariance in the form lvk_map_select_queries takes as cov_cam, read off
 * a device-resident covariance (n x n, row-major, leading dimension ldp) without moving it - the link between the filter and the prior-map
 * chain.  No reference counterpart.  The job is lvk_landmark_fix_job without the gate fields; the conventions are those of
 * lvk_ekf_update_landmarks: R(q) maps body to world, the injection is R_b <- (I + [d_theta_b]x) R_b, p_b <- p_b + d_p_b,
 * R_b2c <- R_b2c R(d_theta_e)^T, t_c_b <- t_c_b + d_t; twelve columns of P matter, in ascending order: 15..20 (d_theta_e, d_t), then the
 * clone's six (d_theta_b, d_p_b).  The pose is
 *   R_wc = R_b R_b2c^T,   p_wc = p_b + R_b t_c_b,
 * its error is defined as lvk_map_select_queries reads it - R_wc,true = R_wc (I + [dtheta]x), the rotation error on the camera side, and
 * p_wc,true = p_wc + dp in the world frame - and to first order, under the injection above,
 *   dtheta = R_b2c d_theta_e + R_wc^T d_theta_b,   dp = R_b d_t - [R_b t_c_b]x d_theta_b + d_p_b,
 * so cov_cam = J P_s J^T (order [dtheta dp]) with P_s the 12 x 12 sub-block and
 *   J = [ R_b2c  0    R_wc^T          0
 *         0      R_b  -[R_b t_c_b]x   I ].
 * (The signs were confirmed against the injection by central differences of (R_wc^T R_wc', p_wc' - p_wc): tests/camera_pose_ref.py; they
 * agree with the form above.)  FP64 throughout, no contraction, every expression in the order written here, so every output has one right
 * value:
 *   R_b      Eigen's Quaternion::toRotationMatrix of q_b = [x y z w] (as lvk_ekf_landmark_rel_cov takes it): tx = 2 x, ty = 2 y, tz = 2 z,
 *            twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x, txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z;
 *            R_b = [1 - (tyy + tzz), txy - twz, txz + twy; txy + twz, 1 - (txx + tzz), tyz - twx; txz - twy, tyz + twx, 1 - (txx + tyy)].
 *   pose     R_wc[i][j] = (R_b[i][0] R_b2c[j][0] + R_b[i][1] R_b2c[j][1]) + R_b[i][2] R_b2c[j][2];
 *            u_i = (R_b[i][0] t_c_b,0 + R_b[i][1] t_c_b,1) + R_b[i][2] t_c_b,2;   p_wc,i = p_b,i + u_i.
 *   J        6 x 12, all zeros but: J[i][c] = R_b2c[i][c], J[i][6 + c] = R_wc[c][i], J[3 + i][3 + c] = R_b[i][c],
 *            J[3 + i][6 + c] = (-[u]x)[i][c] (rows (0, u_2, -u_1), (-u_2, 0, u_0), (u_1, -u_0, 0)), J[3 + i][9 + c] = 1 when i == c.
 *   T        T[i][j] = sum over l = 0..11, upwards from 0.0, of J[i][l] P_s[l][j] - the zero entries of J are terms like any other.
 *   cov_cam  for i <= j: cov[i][j] = sum over l = 0..11, upwards from 0.0, of T[i][l] J[j][l]; cov[j][i] is a copy of it, so the
 *            result is symmetric bit for bit.
 * One launch of one workgroup (one wavefront; 2304 bytes of LDS: P_s, J, T) and one wait.  Nothing outside those twelve rows and columns
 * of P is read.  When the extrinsics are not estimated their block of P is zero and cov_cam is the clone block's own J_b P_bb J_b^T.
 * h_R_wc: 9 doubles, row-major; h_p_wc: 3; h_cov36: 36, row-major.  larvio_amd.localize.camera_pose_cov_ref is the numpy restatement.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer, ldp < n, clone_col < 21 or clone_col + 6 > n, a value
 * of the job that is not finite, |q_b| off 1 by more than 1e-6. */
typedef struct { int clone_col, pad0;            /* first of the clone's six columns */
                 double q_b[4], p_b[3];          /* the clone's pose */
                 double R_b2c[9], t_c_b[3]; }    /* the extrinsics, as lvk_ekf_get_state hands them out */
        lvk_camera_pose_job;
lvk_status lvk_ekf_camera_pose_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_camera_pose_job* h_job,
                                   double* h_R_wc /* 9 */, double* h_p_wc /* 3 */, double* h_cov36 /* 36 */);

/* Stage entry: the last link of the prior-map chain on the device - the records of lvk_frontend_match_map into the observation rows
 * lvk_ekf_add_landmark_obs takes, gathered from the resident map so that the host needs no copy of it.  No reference counterpart.
 * d_rec: n_rec lvk_map_match records (at most 1024); d_X: the map's n_map points (3 doubles each, the map's own frame); d_cov: NULL or
 * their covariances (9 doubles each, row-major; the upper triangle is read); align: the map's alignment - only c, s, t are read, NULL =
 * identity (c = 1, s = 0, t = 0 through the same expressions, so NULL and an explicit identity record give the same bytes); sigma: the
 * standard deviation of a matched corner in normalised units.  FP64 throughout, no contraction, every expression in the order written
 * here, so every output has one right value:
 *   kept      record k is kept iff m.status == LVK_MATCH_OK and 0 <= index < n_map.  An OK record whose index is outside the map is
 *             counted in n_bad, is not emitted, and nothing is read at its index: an index is compared before it is followed.  Records
 *             of any other status are skipped whatever their index.
 *   p_w       with X = d_X[index]: q = (c X_x - s X_y, s X_x + c X_y), p_w = (q_x + t_x, q_y + t_y, X_z + t_z) - the expressions of
 *             lvk_map_select_queries, so the point that is fused is bit for bit the point that was projected.
 *   cov_w     Rz Sigma Rz^T as (Rz Sigma) Rz^T on the upper triangle a = S00, b = S01, d = S11, e = S02, f = S12, g = S22 of the point's
 *             covariance: m00 = c a - s b, m01 = c b - s d, m10 = s a + c b, m11 = s b + c d;  w00 = m00 c - m01 s, w01 = m00 s + m01 c,
 *             w11 = m10 s + m11 c, w02 = c e - s f, w12 = s e + c f, w22 = g;  cov_w = [w00 w01 w02; w01 w11 w12; w02 w12 w22] - entry
 *             (i, j) and entry (j, i) are one value, so the result is symmetric bit for bit.  All zeros when d_cov is NULL.
 *   uv        (double) m.und, both coordinates;  sigma is copied.
 *   order     the kept records in the records' own order: d_obs[j] is the j-th kept record, d_idx[j] its row in d_rec.
 * d_obs, d_idx: room for n_rec entries each, n_ok of them are written and nothing beyond; d_info: n_ok (the count), n_bad and pad 0,
 * written by the kernel of every call that launches.  One launch of one workgroup on the context's stream (one lane per record; the
 * positions come from wave ballots and a scan of the wavefronts' counts in 128 bytes of LDS - no atomics, nothing depends on the order
 * in which anything ran: two runs on the same input give the same bytes), not waited for.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer that is needed (d_info always; d_rec, d_obs, d_idx with
 * n_rec > 0; d_X with n_rec > 0 and n_map > 0), a negative count, a non-finite c, s or t of the alignment, a sigma that is not a finite
 * number > 0.  LVK_ERR_CAPACITY: n_rec > 1024.  n_rec == 0: LVK_OK, d_info zeroed, nothing launched. */
typedef struct { int n_ok, n_bad, pad[2]; } lvk_map_obs_info;
lvk_status lvk_map_gather_obs(lvk_context* ctx, const lvk_map_match* d_rec, int n_rec, const double* d_X, const double* d_cov, int n_map,
                              const lvk_align_result* align, double sigma, lvk_landmark_obs* d_obs, int* d_idx, lvk_map_obs_info* d_info);

typedef struct {
    /* names and meaning as LarVio::loadParameters reads them (larvio.cpp:58-311, config/euroc.yaml) */
    int if_fej, estimate_extrin, estimate_td, if_zupt_valid;
    int sw_size, max_track_len, least_observation_number;
    int max_features_in_one_grid, aug_grid_rows, aug_grid_cols;
    int width, height;
    double intrinsics[4];
    double T_cam_imu[16];
    double td;
    double pub_frequency, imu_rate;   /* features_rate / imu_rate are doubles in the reference (larvio.h:256-259, larvio.cpp:65-67,224) */
    double noise_gyro, noise_acc, noise_gyro_bias, noise_acc_bias, noise_feature;      /* standard deviations */
    double initial_covariance_orientation, initial_covariance_velocity, initial_covariance_position,
           initial_covariance_gyro_bias, initial_covariance_acc_bias, initial_covariance_extrin_rot, initial_covariance_extrin_trans;
    double rotation_threshold, translation_threshold, tracking_rate_threshold, feature_translation_threshold;
    double zupt_max_feature_dis, zupt_noise_v, zupt_noise_p, zupt_noise_q;
    double static_duration;
    int feature_idp_dim, use_schmidt, calib_imu_instrinsic;   /* must be 1, 0, 0|1 (1: LEG_DIM 46, IMU intrinsics in the state) */
    int max_features;                                          /* capacity hint: features per message (0 = 1024) */
    int legacy_grid;                                           /* 0 (default): grid_map as the reference keeps it - a std::map (larvio.h:383), so a grid code
                                                                  beyond the rows x cols cells (undistorted coordinates outside the image bounds) gets a cell
                                                                  of its own that updateGridMap never clears (larvio.cpp:1969-1975, 3351-3370).
                                                                  1: such codes are not counted (what this library did before round 6; opt-out only,
                                                                  also LVK_GRID_REFERENCE=0 in the environment) */
    int reserved0;                                             /* must be 0 */
} lvk_ekf_config;

/* one sliding-window clone (IMUState_Aug, include/larvio/imu_state.h:72-117) */
typedef struct {
    int64_t id;
    double time, dt;
    double q[4], p[3], p_fej[3];
    double R_b2c[9], t_c_b[3];
    double q_cam[4], p_cam[3];
} lvk_clone;

/* ctor + initialize() (larvio.cpp:40-360) */
lvk_status lvk_ekf_create(lvk_context* ctx, const lvk_ekf_config* cfg, lvk_ekf** out);
void       lvk_ekf_destroy(lvk_ekf* e);
/* LarVio::processFeatures (larvio.cpp:363-461).  h_imu is the caller's buffer; *n_consumed = how many leading samples the
 * reference would erase from it (larvio.cpp:511-512, StaticInitializer.cpp:146-147); *updated = the bool it returns.
 * The call returns when the HOST state (lvk_ekf_get_state, clones, features) is final; the covariance's last launches (the pruning's
 * gather) may still be queued on the context's stream - every entry point that reads the covariance synchronises first, and a device
 * fault in those tail launches is reported by the next call on the handle. */
lvk_status lvk_ekf_process(lvk_ekf* e, double ts, const lvk_feature_obs* h_feats, int n_feats,
                           const lvk_imu* h_imu, int n_imu, int* n_consumed, int* updated);
/* The same update, deferred: the call returns as soon as what the caller needs from processFeatures is known - *n_consumed (the
 * samples to erase from the driver's buffer: a function of time stamps, the state time and td only) and *will_update (the bool
 * processFeatures will return: always true once the filter is initialized; the cold paths - first IMU sample, static initializer,
 * a failed filter - run synchronously inside this call and report their real result) - and the update itself runs on a worker
 * thread of the filter, on the filter's stream.  The buffers are copied before the call returns.  Every other entry point of the
 * filter (all getters, the next update, set_state, destroy) first waits for the queued update, so callers always see the state
 * AFTER it: results are identical to lvk_ekf_process.  This is what lets the reference's blocking drivers
 * (app/larvioMain.cpp:104-116: processImage; processFeatures; getters) overlap the next frame's front-end with this frame's update.
 * lvk_ekf_wait blocks until the queued update is done and returns ITS status (*updated as lvk_ekf_process would have set it). */
lvk_status lvk_ekf_process_async(lvk_ekf* e, double ts, const lvk_feature_obs* h_feats, int n_feats,
                                 const lvk_imu* h_imu, int n_imu, int* n_consumed, int* will_update);
lvk_status lvk_ekf_wait(lvk_ekf* e, int* updated);
/* bypass the initializer (tests, benchmarks): IMU state at time t, last IMU sample (m_gyro_old / m_acc_old) */
lvk_status lvk_ekf_set_state(lvk_ekf* e, double t, const double q[4], const double p[3], const double v[3],
                             const double bg[3], const double ba[3], const double gyro_old[3], const double acc_old[3]);
int        lvk_ekf_dim(const lvk_ekf* e);                      /* state_cov.rows() */
int        lvk_ekf_is_initialized(const lvk_ekf* e);
/* take_off_stamp (larvio.cpp:380): the state time at which the initializer succeeded; the state log's time origin (:446) */
double     lvk_ekf_take_off_stamp(const lvk_ekf* e);
/* 30 doubles: t, q[4] (x y z w), v[3], p[3], bg[3], ba[3], R_imu_cam0[9], t_cam0_imu[3], td  (getTbw/getVel, larvio.cpp:2644-2700) */
lvk_status lvk_ekf_get_state(const lvk_ekf* e, double* h_out30);
/* the 24 IMU-intrinsic parameters T1 T2 T3 A1 A2 A3 M1 M2 (larvio.cpp:129-154; state columns 22..45 when calibrated) */
lvk_status lvk_ekf_get_imu_intrinsics(const lvk_ekf* e, double* h_out24);
lvk_status lvk_ekf_set_imu_intrinsics(lvk_ekf* e, const double* h_in24);
lvk_status lvk_ekf_get_cov(lvk_ekf* e, double* h_P);           /* N*N row-major, synchronises (getPpose/getPvel read blocks of it) */
/* the counterpart: replace the covariance (n*n row-major, n == lvk_ekf_dim(); a prior, or a test's starting point).  Nothing is
 * checked about the matrix itself.  LVK_ERR_ARG when n is not the state's dimension, or when an update queued with
 * lvk_ekf_process_async has not been waited for yet - by lvk_ekf_wait or by any other call that waits for it (every getter does) -
 * whether or not it has finished meanwhile: the answer does not depend on timing. */
lvk_status lvk_ekf_set_cov(lvk_ekf* e, const double* h_P, int n);
/* What a measurement update does when the Cholesky factorisation of S = H P H^T + sigma2 I meets a non-positive pivot:
 *   LVK_INDEFINITE_FAIL (the default): the update fails with LVK_ERR_NUMERIC and the handle stays failed;
 *   LVK_INDEFINITE_LDLT: that one update (after lost features, pruning or a zero-velocity update; queued with lvk_ekf_process_async or
 *     not) runs again through the pivoted LDL^T of lvk_ekf_update_ldlt on the untouched covariance, as the reference does
 *     (larvio.cpp:1456), and the filter continues.  lvk_ekf_indefinite_fallbacks counts how often this has happened.
 *     If that update has more rows than the pivoted factor's LDS holds (m > ~1100) the call fails with LVK_ERR_CAPACITY instead of
 *     LVK_ERR_NUMERIC; if the state's dimension is not the one the failed update ran on (no caller does that today) the default applies.
 * The sharded update has no fallback yet: with a transport set (lvk_ekf_set_shard) LVK_INDEFINITE_LDLT is refused with
 * LVK_ERR_UNSUPPORTED, and so is a transport once the policy is set. */
#define LVK_INDEFINITE_FAIL 0
#define LVK_INDEFINITE_LDLT 1
lvk_status lvk_ekf_set_indefinite_policy(lvk_ekf* e, int policy);
long       lvk_ekf_indefinite_fallbacks(const lvk_ekf* e);
/* Test hook, meaningful ONLY directly after an update that failed with LVK_ERR_NUMERIC under LVK_INDEFINITE_FAIL (the one case in which
 * it also answers on a failed handle): the stacked system that update read, after compression - H (m x n row-major), r (m) - and the
 * covariance (n x n) and state (30 doubles, as lvk_ekf_get_state), which the failed update left exactly where it started.  In any other
 * situation the row buffers may already hold a later stage's rows and covariance and state are simply the present ones: do not
 * build on it.  Any output pointer may be null; with all four null only *m and *n are set. */
lvk_status lvk_ekf_last_update(lvk_ekf* e, int* m, int* n, double* h_H, double* h_r, double* h_P, double* h_state30);
/* the leading n x n block of the covariance (n <= 16: orientation 0..2, velocity 3..5, position 6..8, gyro bias 9..11, ...), row-major -
 * all that getPpose / getPvel read (larvio.cpp:2673-2690); served from a host-side mirror the update keeps, no transfer of the matrix */
lvk_status lvk_ekf_get_cov_imu(lvk_ekf* e, int n, double* h_out);
int        lvk_ekf_get_clones(const lvk_ekf* e, lvk_clone* h_out, int cap);       /* getSwPoses */
int        lvk_ekf_get_features(const lvk_ekf* e, int64_t* h_ids, double* h_inv_depth, double* h_pos_w, int cap);  /* getActiveeMapPointPositions */
/* getStableMapPointPositions (larvio.cpp:2717-2722): in-state features that were lost since the last call, with their last world
 * position; the entries handed out are removed, as the reference clears lost_slam_features on read.  Returns the count (<= cap). */
int        lvk_ekf_take_lost_features(lvk_ekf* e, int64_t* h_ids, double* h_pos_w, int cap);
/* How well each map point is known: the 3 x 3 position covariance of lvk_ekf_landmark_cov (the conventions are stated there), read
 * off the filter's device-resident covariance by one kernel launch - the matrix itself is not transferred.
 * lvk_ekf_get_feature_cov: the in-state features in the order of lvk_ekf_get_features - id, anchor clone id, world position and Sigma
 *   (9 doubles each, row-major, exactly symmetric) - up to cap of them; *n_out = how many.  The jobs are built from the host state
 *   (anchor clone attitude, current extrinsics, anchor observation, inverse depth), the kernel runs on the context's stream behind
 *   whatever the last update left queued, and the call waits for it.  Any output pointer except n_out may be null.  A feature whose
 *   anchor clone is not in the window gets nine NaNs (the state injection skips the same case).  A failed handle answers as
 *   lvk_ekf_get_cov does.
 * lvk_ekf_set_lost_feature_cov: off by default.  While on, an update that drops lost in-state features from the covariance first runs
 *   the same kernel for them, on the covariance as it is BEFORE their columns go (after this message's propagation and clone
 *   augmentation, which leave the 13 rows and columns involved untouched); the results land in the filter's pinned download
 *   buffer and are attached to the queued points once the update has waited for its stream.  An update that drops features and
 *   would otherwise return without any wait behind that launch makes one more stream wait - only while the switch is on.  With it
 *   off the filter launches exactly the kernels it launched before this entry point existed.  Under the sharded update
 *   (lvk_ekf_set_shard) every rank runs the kernel for all lost points on its own replica of the covariance: identical bits everywhere.
 * lvk_ekf_take_lost_features_cov: drains the same list as lvk_ekf_take_lost_features, with each point's Sigma (9 doubles; nine NaNs
 *   for a point queued while the switch was off, or whose anchor had left the window).  h_ids, h_pos_w, h_cov9 may each be null. */
lvk_status lvk_ekf_get_feature_cov(lvk_ekf* e, int64_t* h_ids, int64_t* h_anchor_ids, double* h_pos_w, double* h_cov9, int cap, int* n_out);
lvk_status lvk_ekf_set_lost_feature_cov(lvk_ekf* e, int on);
int        lvk_ekf_take_lost_features_cov(lvk_ekf* e, int64_t* h_ids, double* h_pos_w, double* h_cov9, int cap);
/* The same map points where a consumer that steers or renders needs them: in the camera frame of a pose of the window, with the
 * covariance of lvk_ekf_landmark_rel_cov (conventions there), in which the unobservable global position and yaw cancel - the depth
 * sigma is sqrt(Sigma[2][2]).  The in-state features in the order of lvk_ekf_get_features - id, anchor clone id, p_c (3 doubles) and
 * Sigma (9 doubles, row-major, exactly symmetric) - up to cap of them; *n_out = how many.  to_clone_id == -1: the current IMU state
 * is the target (state columns 0.. and 6..); otherwise the id of a clone of lvk_ekf_get_clones - an id that is not in the window is
 * LVK_ERR_ARG and the handle stays usable.  The jobs are built from the host state exactly as lvk_ekf_get_feature_cov builds them,
 * plus the target's pose and the anchor clone's position; one launch on the context's stream behind whatever the last update left
 * queued, and the call waits for it.  Any output pointer except n_out may be null.  A feature whose anchor clone is not in the window
 * gets NaNs in position and Sigma.  A failed handle answers as lvk_ekf_get_cov does.  Under the sharded update (lvk_ekf_set_shard)
 * the call runs on the rank's own replica of the covariance.  A getter only: no switch, no state, nothing added to lvk_ekf_process*. */
lvk_status lvk_ekf_get_feature_rel(lvk_ekf* e, int64_t to_clone_id, int64_t* h_ids, int64_t* h_anchor_ids, double* h_pos_c, double* h_cov9, int cap, int* n_out);
/* The MSCKF points: every lost-feature update triangulates the features that never enter the state (hundreds to thousands per message),
 * uses them once and forgets them.  lvk_ekf_set_msckf_points (off by default) keeps them, each with the covariance of
 * lvk_ekf_msckf_point_cov (conventions there): while on, the lost-feature update queues that kernel for its MSCKF jobs ahead of its
 * update, on the covariance the update starts from (after this message's propagation and augmentation - the one the gate reads), with
 * the results going to the filter's pinned download buffer.  Once the update has waited for its stream and the gate results are known,
 * every MSCKF feature that was used and erased - it triangulated, its gate accepted it, and the kernel reported ok - yields one record
 * {id, world position, Sigma, number of observations} on a list that lvk_ekf_take_msckf_points drains (up to cap records per call;
 * any output pointer may be null; returns the count).  The list holds at most 65536 records: the oldest half goes when it is full.
 * Sigma is CONSERVATIVE: it is stated against the covariance before the update that consumes the point has been applied.
 * One feature id can appear in SEVERAL records: a track that is still alive when it reaches max_track_len observations is used and
 * erased like a lost one, and the tracker's next message starts it again under the same id - a long track is consumed in pieces, each
 * piece a record of its own (its own observations, position and Sigma).  Do not key a map by id alone; only with max_track_len above
 * the window (sw_size + 2) is every id handed out once.
 * The kernel takes 2..64 observations per point, as the stage entry does: a feature seen from more than 64 clones (possible only with
 * sw_size > 62) takes part in the update as always but is not exported.  Every MSCKF job of an update has a result slot (the download
 * buffer holds as many as the update's batch may have jobs; a batch that broke that rule would fail the update with
 * LVK_ERR_CAPACITY, not lose points).
 * Gate-rejected points and the features of pruning updates (they stay in the map) are not exported.  The launch is queued ahead of the update,
 * whose gate results and correction the host always waits for on the same stream before it reads the export: by that order of calls
 * the export is meant to need no stream wait of its own (at most one more per update is its budget; the waits are not counted by a
 * test).  With the switch off the filter launches exactly the kernels it launched
 * before this entry point existed.  State, covariance and counters are the same bits with the switch on or off.
 * The sharded update does not export: with a transport set (lvk_ekf_set_shard) switching on is refused with LVK_ERR_UNSUPPORTED, and so
 * is a transport while the switch is on. */
lvk_status lvk_ekf_set_msckf_points(lvk_ekf* e, int on);
int        lvk_ekf_take_msckf_points(lvk_ekf* e, int64_t* h_ids, double* h_pos_w, double* h_cov9, int* h_n_obs, int cap);
/* The keyframe export: the pose side of the two exports above.  A clone that the pruning removes from the window is gone, and the only
 * pose uncertainty a caller can otherwise get is the absolute one (lvk_ekf_get_cov_imu), which grows without bound along the four
 * unobservable directions.  lvk_ekf_set_keyframe_export (off by default) keeps every pruned clone as a record with the covariances of
 * lvk_ekf_pose_rel_cov (conventions there): while on, the pruning - the two-clone case and the zero-velocity one-clone case - queues one
 * absolute and one relative job for each clone it removes, AFTER the pruning update's correction has been injected and BEFORE the
 * clone's rows and columns leave the covariance: the last covariance in which the clone exists, with the poses that belong to it.
 * b (to_id) is the nearest NEWER clone that survives this pruning; two adjacent removed clones share it.  Every record therefore points
 * forward in time to a clone that is exported later or is still in the window (lvk_ekf_get_window_cov): the records form a connected
 * chain.  The results go to the filter's pinned download buffer and are attached to the records by the time the update's call,
 * lvk_ekf_wait or any getter returns; a pruning update that would otherwise return without any wait behind that launch makes one
 * more stream wait - only while the switch is on.  With it off the filter launches exactly the kernels it launched before this entry
 * point existed.  State, covariance and counters are the same bits with the switch on or off; blocking, deferred and pipelined
 * (lvk_vio_pipe) runs give the same records.
 *   id, time        the removed clone (a);  to_id, to_time: b
 *   q, p            a's pose (body in world) as the filter last held it
 *   rel_q, rel_p    R_ab = R_a^T R_b as a quaternion [x y z w], p_ab = R_a^T (p_b - p_a), from the poses of that instant
 *   cov_abs         a's 6 x 6 block, order [d_theta d_p], row-major: bit for bit the entries of the covariance
 *   cov_rel         Sigma_rel of (a, b), order [d_phi d_rho], row-major, exactly symmetric
 * lvk_ekf_take_keyframes drains the list in pruning order (within one pruning: ascending id), up to cap records per call, and returns
 * the count.  The list holds at most 65536 records: the oldest half goes when it is full.
 * lvk_ekf_get_window_cov: for the clones of lvk_ekf_get_clones, in that order (up to cap; *n_out = how many), each clone's id, its
 * absolute block (36 doubles) and, for clone i < n - 1, Sigma_rel to clone i + 1 (36 doubles); the last clone gets 36 NaNs.  One
 * launch and one wait, on the context's stream behind whatever is queued.  h_ids, h_cov_abs36, h_cov_rel36 may each be null.  A failed
 * handle answers as lvk_ekf_get_cov does.
 * The edges are marginals of ONE joint distribution: consecutive relative poses share clones and are correlated.  Using them as
 * independent factors of a pose graph is the usual approximation, not an identity.
 * The sharded update does not export: with a transport set (lvk_ekf_set_shard) switching on is refused with LVK_ERR_UNSUPPORTED, and so
 * is a transport while the switch is on. */
typedef struct { int64_t id, to_id; double time, to_time;
                 double q[4], p[3];            /* the clone's pose as the filter last held it */
                 double rel_q[4], rel_p[3];    /* R_ab as a quaternion, p_ab; a = this clone, b = to_id */
                 double cov_abs[36], cov_rel[36]; } lvk_keyframe;
lvk_status lvk_ekf_set_keyframe_export(lvk_ekf* e, int on);
int        lvk_ekf_take_keyframes(lvk_ekf* e, lvk_keyframe* h_out, int cap);
lvk_status lvk_ekf_get_window_cov(lvk_ekf* e, int64_t* h_ids, double* h_cov_abs36, double* h_cov_rel36, int cap, int* n_out);
/* External fixes: the way back INTO the filter.  Global position and yaw are unobservable for a VIO and their block of the covariance
 * grows without bound (see lvk_ekf_pose_rel_cov); a caller that has GNSS, motion capture or a pose graph over lvk_ekf_take_keyframes
 * hands its result back as a measurement of a CLONE that is still in the window - a delayed measurement on a stochastic clone, so a
 * late result is fused correctly with no re-propagation.  No reference counterpart.
 * Conventions (those of lvk_ekf_pose_rel_cov): R(q) maps body to world, the injection is R <- (I + [d_theta]x) R, p <- p + d_p, clone
 * c has columns leg + 6 c (d_theta) and leg + 6 c + 3 (d_p), times are on the IMU clock as lvk_clone.time.  A fix is expressed in the
 * FILTER's world frame: aligning an external frame (yaw and translation) is the caller's job (for a map of points seen in a frame,
 * lvk_frontend_align_landmarks estimates exactly those four numbers; a frame that differs by more stays the caller's).
 *   LVK_FIX_POSITION   z = p_i + R_i lever + n,  n ~ N(0, cov[0:3, 0:3]) (cov is 6 x 6 row-major storage; the upper-left 3 x 3 is used);
 *                      r = z - (p_i + R_i lever),  H_theta = -[R_i lever]x,  H_p = I                                  (3 rows, 6 columns)
 *   ... between two adjacent clones i, j, a = (t - t_i) / (t_j - t_i): the prediction is (1 - a)(p_i + R_i lever) + a (p_j + R_j lever)
 *                      and the two clones' blocks are scaled by 1 - a and a                                           (3 rows, 12 columns)
 *   LVK_FIX_POSE       three more rows in front: r_theta = 2 vec(q_z * q_i^-1), the sign taken so that w >= 0, H_theta = I on clone i;
 *                      cov is the 6 x 6 covariance in the order [d_theta; p]                                          (6 rows, 6 columns)
 * (The signs were confirmed against the injection by central differences: tests/fix_ref.py.)
 * lvk_ekf_add_fix queues a fix (at most 64 wait at a time: LVK_ERR_CAPACITY beyond).  Every update (lvk_ekf_process and its deferred
 * and pipelined forms) applies the queue at one place: after the zero-velocity check and before the lost-feature update - the
 * message's own clone exists, no clone has been pruned yet - in queue order, each fix one lvk_ekf_update_sparse on the filter's
 * covariance followed by the state injection.  An empty queue costs nothing: the filter then launches exactly the kernels it
 * launched before these entry points existed.  Each applied fix costs two launches and one stream wait.  The target clone:
 *   clone_id >= 0                that clone; an id that is not in the window (pruned, or never handed out): LVK_FIX_STALE
 *   clone_id == -1, by time      a clone whose time equals (==) the fix's: that clone; older than the oldest clone: LVK_FIX_STALE; newer
 *                                than the newest clone: the fix stays queued; strictly between two adjacent clones: a POSITION fix
 *                                with t_j - t_i <= max_gap_s is interpolated, anything else is LVK_FIX_NO_CLONE.
 * max_gap_s defaults to 0 - no interpolation unless the caller asks for it and picks the gap: after pruning, adjacent clones can be far
 * apart, and the library invents no bound.  The chi-square gate of a fix is gate_scale times the filter's own table entry for 3 or 6
 * degrees of freedom - the table of the feature gate (larvio.cpp:353-357), the reference's 5 % quantiles: 0.3518 and 1.6354 - so the
 * default scale of 1 is as strict as the filter is with its features; a caller who wants the usual 99.9 % gate passes
 * 16.27 / 0.3518 = 46.2 (3 rows) or 22.46 / 1.6354 = 13.7 (6 rows).  A scale <= 0 disables the gate; a NaN is LVK_ERR_ARG.
 * One lvk_fix_report per consumed fix (lvk_ekf_take_fix_reports drains them in order, up to cap per call, and returns the count; the
 * list holds at most 65536 records: the oldest half goes when it is full): tag, kind, status, gamma = r^T S^-1 r (0 unless APPLIED or
 * GATED), the ids of the clones used (clone_j = -1 unless interpolated; both -1 for STALE and NO_CLONE) and a (0 unless interpolated).
 * lvk_ekf_fix_stats: [0] fixes queued so far [1] applied [2] gated [3] not positive definite [4] stale [5] no clone [6] waiting now
 * [7] of the applied ones, interpolated.  lvk_ekf_counters and lvk_ekf_last_update are unchanged by a fix, and lvk_ekf_config keeps its size.
 * A gated or not-positive-definite fix leaves state and covariance exactly as they were.
 * Refusals and limits:
 *   lvk_ekf_add_fix is LVK_ERR_UNSUPPORTED while a shard transport is set (lvk_ekf_set_shard), and a transport is refused while fixes
 *     wait: the sharded update does not apply fixes;
 *   LVK_ERR_ARG for a value that is not finite (time, p, lever, the part of cov that is used, q of a POSE fix), a cov block that is not
 *     symmetric positive definite (a Cholesky factorisation on the host), a POSE fix whose |q| differs from 1 by more than 1e-6, a kind
 *     other than the two, a clone_id below -1;
 *   a deferred update (lvk_ekf_process_async) consumes what was queued when it was issued; lvk_ekf_add_fix between the issue and
 *     lvk_ekf_wait (or any other call that waits for it: every getter does) is LVK_ERR_ARG, whether or not the update has finished
 *     meanwhile, as for lvk_ekf_set_cov;
 *   with a lvk_vio_pipe, fixes are legal only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
#define LVK_FIX_POSITION 0
#define LVK_FIX_POSE     1
#define LVK_FIX_APPLIED  0
#define LVK_FIX_GATED    1
#define LVK_FIX_NOT_PD   2
#define LVK_FIX_STALE    3
#define LVK_FIX_NO_CLONE 4
typedef struct { int64_t tag;       /* caller's, echoed in the report */
                 int kind;          /* LVK_FIX_POSITION 0, LVK_FIX_POSE 1 */
                 int64_t clone_id;  /* >= 0: this clone; -1: by time */
                 double time;       /* IMU clock, as lvk_clone.time */
                 double p[3], q[4], lever[3];
                 double cov[36]; }  /* POSITION: upper-left 3x3 used, order [p]; POSE: order [dtheta; p] */
        lvk_fix;
typedef struct { int64_t tag; int kind, status; double gamma; int64_t clone_i, clone_j; double a; } lvk_fix_report;
lvk_status lvk_ekf_add_fix(lvk_ekf* e, const lvk_fix* h_fix);              /* queue, cap 64: LVK_ERR_CAPACITY beyond */
lvk_status lvk_ekf_set_fix_options(lvk_ekf* e, double gate_scale, double max_gap_s);
int        lvk_ekf_take_fix_reports(lvk_ekf* e, lvk_fix_report* h_out, int cap);
void       lvk_ekf_fix_stats(const lvk_ekf* e, long* h_out8);
/* Observations of known landmarks: localising against a prior map.  Where lvk_ekf_add_fix takes a finished pose with a covariance, this
 * takes what a vision caller has before any PnP: image observations (normalised coordinates, as the filter's own features) of points
 * whose position in the FILTER's world frame is known, each with its own covariance - surveyed fiducial corners, the output of
 * lvk_ekf_take_msckf_points / lvk_ekf_take_lost_features_cov of an earlier lap, a prior map (one with its own origin and yaw is
 * brought into this frame by lvk_frontend_align_landmarks first).  The filter fuses them directly
 * (lvk_ekf_update_landmarks: measurement model, gate, compression), correlation with the extrinsics included, and five points or
 * fewer - where a PnP has no answer - still count.  No reference counterpart.
 * lvk_ekf_add_landmark_obs queues one BATCH: the observations made in one image, i.e. of one clone (at most 1024 observations per
 * batch and 16 batches waiting: LVK_ERR_CAPACITY beyond; n_obs = 0 is a legal, empty batch).  The target clone follows the rules of
 * lvk_ekf_add_fix without the interpolation: clone_id >= 0 names it (not in the window: LVK_LANDMARKS_STALE); clone_id == -1 goes by
 * time - equal (==) to a clone's time: that clone; older than the oldest clone: STALE; newer than the newest: the batch stays queued;
 * anything else, strictly between two clones included: LVK_LANDMARKS_NO_CLONE.
 * Every update applies the queue right behind the fix queue - after the zero-velocity check, before the lost-feature update - in queue
 * order, each batch one lvk_ekf_update_landmarks on the filter's covariance (three launches, one wait) plus the state injection.  An
 * empty queue costs nothing, an empty batch launches nothing, and a run that never queues a batch keeps its bits.
 * lvk_ekf_set_landmark_options: the gate of one observation is gate_scale times the filter's own table entry for 2 degrees of freedom
 * (the reference's 5 % quantile, 0.1026): the default scale of 1 is as strict as the filter is with its features; the usual 99.9 %
 * gate is 13.816 / 0.1026 = 134.7.  A scale <= 0 disables the gate; a NaN is LVK_ERR_ARG.  min_depth (default 0.1, >= 0) is the depth
 * in the camera frame at or below which an observation counts as behind the camera.
 * One lvk_landmark_report per consumed batch (lvk_ekf_take_landmark_reports drains them in order, up to cap per call, and returns the
 * count; the list is capped like the fix reports): tag, status, the clone's id (-1 for STALE and NO_CLONE), n_obs, n_used, n_gated,
 * n_behind and the batch's gamma (0 unless APPLIED).  ALL_REJECTED (no observation was used; an empty batch too) and NOT_PD leave state
 * and covariance exactly as they were.  lvk_ekf_landmark_stats: [0] batches queued so far [1] applied [2] all rejected [3] not positive
 * definite [4] stale [5] no clone [6] waiting now [7] observations in consumed batches [8] used [9] gated [10] behind [11] 0.
 * lvk_ekf_counters, lvk_ekf_last_update and lvk_ekf_config are unchanged.
 * Refusals: LVK_ERR_UNSUPPORTED while a shard transport is set, and a transport is refused while batches wait; LVK_ERR_ARG for what
 * lvk_ekf_update_landmarks refuses in an observation, a time that is not finite, a clone_id below -1; between lvk_ekf_process_async
 * and the call that waits for it an add is LVK_ERR_ARG, as for fixes; with a lvk_vio_pipe, adds are legal only between
 * lvk_vio_pipe_drain and the next lvk_vio_pipe_submit. */
#define LVK_LANDMARKS_APPLIED      0
#define LVK_LANDMARKS_ALL_REJECTED 1
#define LVK_LANDMARKS_NOT_PD       2
#define LVK_LANDMARKS_STALE        3
#define LVK_LANDMARKS_NO_CLONE     4
typedef struct { int64_t tag; int status, n_obs; int64_t clone_id; int n_used, n_gated, n_behind, pad0; double gamma; } lvk_landmark_report;
lvk_status lvk_ekf_add_landmark_obs(lvk_ekf* e, int64_t tag, int64_t clone_id, double time, const lvk_landmark_obs* h_obs, int n_obs);
lvk_status lvk_ekf_set_landmark_options(lvk_ekf* e, double gate_scale, double min_depth);
int        lvk_ekf_take_landmark_reports(lvk_ekf* e, lvk_landmark_report* h_out, int cap);
void       lvk_ekf_landmark_stats(const lvk_ekf* e, long* h_out12);
/* What the moving-start initialiser (FlexibleInitializer.cpp:11-25 -> DynamicInitializer.cpp) handed to the filter, with the intermediate
 * results of the successful attempt - for parity tests against an independent restatement fed the same messages:
 *   valid        1 once the dynamic initialiser has succeeded on this handle (0: never ran, or the static one fired)
 *   message      0-based index of the lvk_ekf_process call (counted from the first one the initialisers saw) that succeeded
 *   attempts     relative-pose attempts made up to and including the successful one (= calls of the RANSAC stage's window scan that found a frame)
 *   ransac_calls launches of the RANSAC kernel (cv::findFundamentalMat, solve_5pts.cpp:206) over all attempts
 *   l, rel_R/rel_T   relativePose's frame and pose (DynamicInitializer.cpp:331-360), n_points = landmarks the SfM triangulated (initial_sfm.cpp)
 *   sfm_R/sfm_T  the window's 11 structure-from-motion poses (camera-to-c0 rotation row-major, position)
 *   bg, g, scale solveGyroscopeBias / LinearAlignment + RefineGravity (initial_alignment.cpp:74-122 ...)
 *   state_time, q (x y z w), v, erase     the state the filter starts from and the IMU samples erased */
typedef struct lvk_init_report {
    int valid, message, attempts, ransac_calls, l, n_points, erase, pad;
    double state_time, scale, rel_R[9], rel_T[3], sfm_R[11 * 9], sfm_T[11 * 3], bg[3], g[3], q[4], v[3];
} lvk_init_report;
lvk_status lvk_ekf_init_report(const lvk_ekf* e, lvk_init_report* h_out);
/* [0] hybrid updates [1] msckf updates [2] rows of the last update [3] zupt updates [4] gated in [5] gated out [6] map size [7] triangulations */
void       lvk_ekf_counters(const lvk_ekf* e, long* h_out8);
/* HIP-event bracket around the H P GEMM (the P H^T contraction, FP64 MFMA) of every update: enable/disable; h_out3 (optional) receives
 * [milliseconds, flops = sum 2 m N^2, launches] accumulated since the previous call */
lvk_status lvk_ekf_profile(lvk_ekf* e, int enable, double* h_out3);
/* the same switch brackets every level of the structure-aware TSQR compression (k_qr_sparse; replaces the SPQR calls at
 * larvio.cpp:1430-1445, 2209-2229): h_out4 = [milliseconds, Householder flops on the structure actually factored (sum over nodes
 * and reflectors j of 4 (r - j)(c + 1 - j)), launches, rows entering the levels] since the previous call */
lvk_status lvk_ekf_profile_qr(lvk_ekf* e, double* h_out4);

/* ---- sharded measurement update (BASELINE.json configs[4]).  Every rank runs the same filter on the same messages; the
 * per-feature device work of an update (Jacobian rows, null-space projection, chi-square gate, stacking, first compression) is split
 * into `world` contiguous feature ranges in the reference's stacking order (larvio.cpp:2185-2201), rank `rank` doing its own; one
 * all-gather per update hands every rank all compressed blocks and all gate results, in rank order, and the rest of the update is
 * replicated - identical bits on every rank.  The collective is a callback so that the transport is the caller's choice:
 * lvk_shard_allgather_rccl (below) runs ncclAllGather on the filter's stream, device buffers in place; a test may move the bytes
 * through the host.  fn must deliver, in d_recv, the `world` send buffers of bytes_per_rank bytes each in rank order, ordered on
 * hip_stream.  fn = NULL (world 1) switches sharding off; with a transport the sharded path runs at any world size, world 1 included
 * (a loop-back through pack -> all-gather -> unpack -> second stage: validates a transport on one GPU).  The exchange buffers are
 * allocated by this call.  Every capacity test of the sharded update has the same outcome on all ranks (each rank plans every rank's
 * share), so a capacity error is raised everywhere before anybody enters the collective; a rank that fails locally (a launch error
 * while queueing its rows, or later) still enters it, with a poisoned block header, and its peers return LVK_ERR_DEVICE at their
 * next sync instead of waiting.  One case cannot post a block - an update that admits new in-state features sizes its exchange from
 * gate results the failing rank could not read - and calls fn(user, NULL, NULL, 0, stream) instead: bytes_per_rank == 0 means
 * ABORT, the transport must make the peers' pending exchange fail (lvk_shard_allgather_rccl: ncclCommAbort). */
typedef int /* lvk_status */ (*lvk_exchange_fn)(void* user, const void* d_send, void* d_recv, size_t bytes_per_rank, void* hip_stream);
lvk_status lvk_ekf_set_shard(lvk_ekf* e, int rank, int world, lvk_exchange_fn fn, void* user);
/* [0] exchanges [1] bytes sent by this rank [2] sharded updates [3] rows this rank stacked; [4] updates the structure-aware
 * compression ran in [5] its levels [6] rows in [7] rows out */
void       lvk_ekf_shard_stats(const lvk_ekf* e, long* h_out8);
/* RCCL transport: one communicator per rank (ncclCommInitRank with the 128-byte id rank 0 obtained from lvk_shard_unique_id and
 * distributed out of band, e.g. torch.distributed.broadcast); pass lvk_shard_allgather_rccl + the communicator to lvk_ekf_set_shard. */
typedef struct lvk_shard_comm lvk_shard_comm;
lvk_status lvk_shard_unique_id(char* h_out128);
lvk_status lvk_shard_comm_create(lvk_context* ctx, const char* h_uid128, int rank, int world, lvk_shard_comm** out);
void       lvk_shard_comm_destroy(lvk_shard_comm* c);
const char* lvk_shard_rccl_path(void);                        /* which librccl the transport bound (the one next to the HIP runtime in use) */
const char* lvk_shard_comm_error(const lvk_shard_comm* c);    /* text of the last RCCL error lvk_shard_allgather_rccl returned on it */
lvk_status lvk_shard_allgather_rccl(void* comm, const void* d_send, void* d_recv, size_t bytes_per_rank, void* hip_stream);

/* ---- per-feature stages of the update, one call each (parity tests; callers that want a single stage).  Host buffers.
 * lvk_triangulate: Feature::initializePosition (use_position 0) / the LM refinement from a given position (1), feature.hpp:383-890,
 *   n views = camera-to-world poses + normalised observations; *ok_out = the reference's return value.
 * lvk_ekf_gate_and_stack: for a batch of MSCKF features, featureJacobian_msckf (larvio.cpp:924-981: H_x blocks, null-space projection),
 *   gatingTest (:1865-1880) against P, and the stacking of the accepted features' rows (:2185-2201) into H (rows x N, row-major,
 *   ld = N) and r.  h_clone_rank / h_obs / h_obs_vel are indexed by obs_off + k.  gamma / accept are per feature. */
typedef struct { double R[9]; double t[3]; } lvk_cam_pose;
typedef struct { double p_w[3]; int n_obs, obs_off; } lvk_msckf_feature;
lvk_status lvk_triangulate(lvk_context* ctx, const lvk_cam_pose* h_poses, const double* h_obs, int n, int use_position,
                           const double* h_position_in, int* ok_out, double* h_position, double* h_solution, double* h_inv_depth,
                           double* h_obs_anchor);
lvk_status lvk_ekf_gate_and_stack(lvk_context* ctx, const lvk_clone* h_clones, int n_clones, const lvk_msckf_feature* h_feats, int n_feats,
                                  const int* h_clone_rank, const double* h_obs, const double* h_obs_vel, const double* h_P, int N,
                                  int if_fej, int estimate_td, double sigma2, double* h_H, double* h_r, int rows_cap, int* rows_out,
                                  double* h_gamma, int* h_accept);

/* lvk_ekf_feature_rows: the per-feature row stage of the filter's update, launched as the filter launches it (the triangulation of
 * tri_pending jobs, the feature-row kernel, the stacking kernel), for a batch of jobs of the three kinds the filter builds:
 *   LVK_FJ_MSCKF        featureJacobian_msckf (larvio.cpp:859-981): 2M rows, null-space projected, rows 3.. are the output;
 *   LVK_FJ_EKF_NEW      a new 1-D inverse-depth feature (:1117-1244), M observing clones other than the anchor: projected on the
 *                       left null space of its feature column, row 0 is the range row (h2 = its feature entry), rows 1.. the output;
 *   LVK_FJ_EKF_TRACKED  a tracked in-state feature: its 2M raw rows.
 * Clone ranks, z and zv (2 doubles each) are indexed by obs_off + k; P is N x N with leading dimension ldp.  gate > 0 gates the job
 * with dof = gate against lvk_chi2_005(dof) (gatingTest, :1865-1880); gate 0 accepts it.  tri_pending (MSCKF only): the landmark is
 * triangulated first from the camera poses h_cams[obs_off + k] (lvk_triangulate with use_position 0) and read by the row kernel
 * from the triangulation's result slot; a failed triangulation rejects the job.
 * Outputs: h_res[j]; the compact block [G | r] of every job (2M x (c + 1), row-major, jobs one after the other in h_blocks) and its
 * column map (c ints per job in h_ccols); and the dense rows: every MSCKF and EKF_TRACKED job owns rows (2M - 3, respectively 2M)
 * of h_H (ldh >= N, h_rows rows) and h_r in job order (EKF_NEW rows never reach it, as in the filter: their feature column is a new
 * state).  h_rows must hold every candidate row (the sum over those jobs), whichever the mode.  h_H and h_r are read first and only
 * the written rows change.  Without LVK_FR_DIRECT or LVK_FR_DEVICE_ZERO the host reads
 * the gate back and stacks only accepted jobs' rows, one after the other; otherwise a rejected job's rows are zero rows with a zero
 * residual.
 * *rows_out = dense rows written.  LVK_ERR_ARG / LVK_ERR_CAPACITY for input the kernels do not handle; nothing is launched then. */
enum { LVK_FJ_MSCKF = 0, LVK_FJ_EKF_NEW = 1, LVK_FJ_EKF_TRACKED = 2 };
enum {
    LVK_FR_GENERAL = 1,      /* force the general kernel (otherwise the filter's routing picks it) */
    LVK_FR_STRIDE = 2,       /* observations in fixed-stride slots (stride = the batch's largest M), as the filter stages short tracks */
    LVK_FR_DIRECT = 4,       /* the row kernel writes the dense rows itself (no stacking launch) */
    LVK_FR_DEVICE_ZERO = 8   /* the stacking kernel zeroes rejected jobs' rows on the device */
};
typedef struct {
    int type, n_obs, obs_off, anchor_rank, fcol, gate, tri_pending, pad;
    double p_w[3], p_fej[3], inv_depth, obs_anchor[3];
} lvk_feature_job;
typedef struct { double gamma, h2; int rows, first_row, c, accept; } lvk_feature_result;
lvk_status lvk_ekf_feature_rows(lvk_context* ctx, const lvk_clone* h_clones, int n_clones, const lvk_feature_job* h_jobs, int n_jobs,
                                const int* h_clone_rank, const double* h_obs, const double* h_obs_vel, const lvk_cam_pose* h_cams, int n_obs,
                                const double* h_P, int N, int ldp, int leg_dim, int if_fej, int estimate_td, double sigma2, int mode,
                                lvk_feature_result* h_res, double* h_blocks, int* h_ccols, double* h_H, int ldh, int h_rows, double* h_r,
                                int* rows_out);

/* lvk_ekf_msckf_point_cov: first-order 3 x 3 position covariance of least-squares (MSCKF) points, one per job, read off a
 * device-resident covariance (n x n, row-major, leading dimension ldp) without moving it.  A job is a point p_w with M = n_obs
 * observations from DISTINCT clones; clone ranks, z and zv (2 doubles each) are indexed by obs_off + k, as in lvk_ekf_gate_and_stack:
 * the three arrays carry no length, the caller supplies at least max(obs_off + n_obs) entries (2 doubles each for z and zv).
 * With Hx_t (2 x 6, the observing clone), He_t (2 x 6, the extrinsics) and Hf_t (2 x 3, the point) of measurementJacobian_msckf
 * (larvio.cpp:859-921, first-estimate form when if_fej) for observation t, and Hc (2M x c, c = 7 + 6M) the compact block the row stage
 * builds before its null-space projection - columns 0..5 He_t, column 6 the observation's zv when estimate_td and 0 otherwise, columns
 * 7+6t.. Hx_t; its column map cc is 15..21, then leg_dim + 6 rank_t + j -
 *   A = sum_t Hf_t^T Hf_t,   G_t = A^-1 Hf_t^T,   B = sum_t G_t Hc[2t:2t+2, :],   Sigma = sigma2 A^-1 + B P[cc, cc] B^T :
 * the covariance of the least-squares point under pixel noise sigma2 and a state error ~ N(0, P), cross terms between all observing
 * clones included.  A is solved with an unpivoted 3 x 3 LDL^T; if one of its pivots is not positive the point gets nine NaNs and
 * h_ok = 0 (h_ok = 1 otherwise) - a nearly singular A gives a correspondingly large Sigma, not a refusal.  Nothing of P outside rows and
 * columns cc is read; every sum runs in a fixed order (the same input gives the same bits); the lower triangle is a copy of the upper
 * one.  h_cov9: 9 doubles per job, row-major.  The call waits for its launch.
 * LVK_ERR_ARG, with nothing launched and the context still usable: a null pointer, n_jobs < 0, n <= 0, ldp < n, leg_dim other than 22 / 46,
 * n_obs outside 2..64, a negative obs_off, a rank outside [0, n_clones) or whose six columns leave [0, n), a rank that appears twice in
 * one job.  n_jobs == 0 is LVK_OK. */
typedef struct { int n_obs, obs_off; double p_w[3]; } lvk_msckf_point_job;
lvk_status lvk_ekf_msckf_point_cov(lvk_context* ctx, const double* d_P, int ldp, int n, const lvk_clone* h_clones, int n_clones,
                                   const lvk_msckf_point_job* h_jobs, int n_jobs, const int* h_clone_rank, const double* h_obs, const double* h_obs_vel,
                                   int leg_dim, int if_fej, int estimate_td, double sigma2, double* h_cov9, int* h_ok);

/* ---- the two kernels around the exchange of the sharded update (lvk_ekf_set_shard), one call each (parity tests).  Host
 * buffers; each call launches the production kernel through the launcher the filter uses, waits, and copies back.
 * Wire layout of one rank's block (bytes_per_rank bytes, the same on every rank of an update; d_recv holds `world` of them in rank
 * order):
 *   [0, LVK_SHARD_HDR)        header; only its first 16 bytes are defined: unsigned magic (LVK_SHARD_MAGIC), int rank, int k, int n_res
 *   [.., + res_bytes)         n_res lvk_feature_result records, the gate results of the rank's jobs (res_bytes: a multiple of 256,
 *                             >= 32 * the largest job count of any rank)
 *   [.., + k (ncols + 1) 8)   the rank's k compressed rows, ncols + 1 doubles each: the row of H, then its residual
 * Whatever follows (rows k.. of a rank with fewer rows than the largest block, padding) is undefined and never read.
 * The receiver accepts a block iff magic, rank, k and n_res are what ITS plan says about that rank (every rank plans every rank's
 * share).  A block that fails the test - a rank that failed locally posts 0xFF over its header - contributes k zero rows with zero
 * residuals, its results are not copied, and bit min(rank, 31) is raised in the peer-failure word.
 *
 * lvk_shard_pack_stage: k rows of h_X (row-major, ld >= ncols) and h_rX, n_res results -> the block of `rank`, in h_send.  The
 *   device send buffer holds `fill` in every byte before the launch: bytes the kernel does not write come back as fill.
 * lvk_shard_unpack_stage: h_recv (world * bytes_per_rank bytes) and the plan h_meta[world] -> rank g's rows to rows row_off.. of
 *   H (rows x ld, columns [0, ncols)) and r, its results to [job_lo, job_lo + job_n) of both result arrays (n_fout entries each).
 *   h_H, h_r, h_fout, h_fout_host are uploaded as given and read back after the kernel: what it does not write is unchanged.
 *   h_fout_host may be NULL (the kernel then gets no mirror array), h_peer_fail may be NULL (the kernel then gets no word to raise);
 *   otherwise *h_peer_fail is uploaded, OR-ed into by the kernel and read back.
 * LVK_ERR_ARG, nothing launched: a negative size, ld < ncols, res_bytes no multiple of 256 or < 32 n_res (32 job_n of any meta),
 * bytes_per_rank no multiple of 8 or < LVK_SHARD_HDR + res_bytes + 8 k (ncols + 1) (k_max for the unpack), a meta with k outside
 * [0, k_max], with rows outside [0, rows) or jobs outside [0, n_fout). */
#define LVK_SHARD_HDR   256
#define LVK_SHARD_MAGIC 0x4c564b58u      /* "LVKX" */
typedef struct { int job_lo, job_n, k, row_off; } lvk_shard_meta;
lvk_status lvk_shard_pack_stage(lvk_context* ctx, int rank, const double* h_X, int ld, const double* h_rX, int k, int ncols,
                                const lvk_feature_result* h_res, int n_res, size_t res_bytes, int fill,
                                void* h_send, size_t bytes_per_rank);
lvk_status lvk_shard_unpack_stage(lvk_context* ctx, const void* h_recv, size_t bytes_per_rank, const lvk_shard_meta* h_meta, int world,
                                  int ncols, int k_max, size_t res_bytes, double* h_H, int ld, int rows, double* h_r,
                                  lvk_feature_result* h_fout, lvk_feature_result* h_fout_host /* or NULL */, int n_fout,
                                  int* h_peer_fail /* or NULL */);

/* ==================================================================== the driver step
 * One camera frame through both halves, exactly the two calls the reference's drivers make per image
 * (app/larvioMain.cpp:104-116: processImage, then processFeatures when it returned true), with the driver's IMU buffer
 * semantics (samples with t < t_img + 0.05 are visible, processFeatures erases what it consumed, :98-102 and larvio.cpp:511-512).
 * h_imu[0..n_imu) is the CURRENT buffer; *n_consumed tells the caller how many leading samples to drop. */
lvk_status lvk_vio_process(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts,
                           const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* updated);
/* the same step with the update deferred (lvk_frontend_process, then lvk_ekf_process_async): returns when the front-end is done and
 * the update is queued; any getter of the filter (or the next step) waits for it.  This is the schedule the adapter classes
 * (adapter/: larvio::ImageProcessor / larvio::LarVio) give an unchanged blocking driver. */
lvk_status lvk_vio_process_deferred(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts,
                                    const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* will_update);

/* Localise in the loop: from the filter's pose of the last processed frame to queued observations of the resident prior map, in one call -
 * the per-frame link of the prior-map chain (lvk_frontend_set_map / lvk_frontend_build_map, lvk_frontend_relocalise_map for align).  No
 * reference counterpart.  The target clone: clone_id >= 0 names it; clone_id == -1 goes by time, equal (==) to a clone's time - the rule of
 * lvk_ekf_add_landmark_obs without its "newer than the newest stays queued" case.  A frame the filter has no clone for (not initialised,
 * an id that is not in the window, a time no clone has) gives h_info->status = LVK_LOCALISE_NO_CLONE and LVK_OK: nothing is launched,
 * nothing is queued, the rest of h_info is zero and clone_id -1.  Otherwise, in order:
 *   1  the filter's pending update is waited for, as every getter does;
 *   2  lvk_ekf_camera_pose_cov on the filter's covariance with that clone and the current extrinsics: R_wc, p_wc, cov_cam;
 *   3  the device chain of lvk_frontend_match_map with those three, align, select_opt and match_opt - the very code lvk_frontend_match_map
 *      runs, records left on the device;
 *   4  lvk_map_gather_obs' launch on those records where they lie, sigma = sigma_px / ((fx + fy) / 2) of the front-end's camera;
 *   5  one copy back of the count, the source rows and the observations;
 *   6  the observations are queued as ONE batch on that clone (by its id) with `tag`, through lvk_ekf_add_landmark_obs itself: its limits,
 *      refusals and reports are unchanged.  Zero observations (nothing selected, nothing matched) are queued as the legal empty batch, so
 *      there is one lvk_landmark_report per call that found its clone.
 * h_info: status, n_ok = the observations queued, n_bad (lvk_map_gather_obs), the clone's id, map = lvk_frontend_match_map's counts, and
 * the R_wc, p_wc, cov_cam of step 2 that steps 3 and 4 used.
 * Off the per-frame path, as its parts are: it waits for the GPU (once in step 2; the selection's count, the corner count and the copy in
 * 3 to 5), works in the matcher's buffers and one buffer of its own (allocated on first use), and changes nothing a later frame reads
 * except the queue it is meant to fill; a run that never calls it allocates and launches what it did before.  fe and ekf may share a
 * context or not.  With a lvk_vio_pipe attached to ekf it is legal only between lvk_vio_pipe_drain and the next lvk_vio_pipe_submit:
 * LVK_ERR_ARG while a submitted frame's update is queued or running.  LVK_ERR_UNSUPPORTED while a shard transport is set, as
 * lvk_ekf_add_landmark_obs.  LVK_ERR_ARG: a null fe, ekf or h_info, clone_id < -1, a time that is not finite with clone_id == -1, a sigma_px
 * that is not a finite number > 0.  (An update queued by lvk_ekf_process_async is no refusal: step 1 waits for it.)
 * Every refusal of the parts (no map is set, a call before the first processed frame or between lvk_frontend_begin and the
 * lvk_frontend_process of the same frame, the options' ranges, 16 batches waiting) passes through unchanged; none is sticky, and a call
 * refused after step 2 has queued nothing. */
#define LVK_LOCALISE_QUEUED   0
#define LVK_LOCALISE_NO_CLONE 1
typedef struct { int status, n_ok, n_bad, pad; int64_t clone_id; lvk_map_info map; double R_wc[9], p_wc[3], cov_cam[36]; } lvk_localise_info;
lvk_status lvk_vio_localise_map(lvk_frontend* fe, lvk_ekf* ekf, const lvk_align_result* align, int64_t clone_id, double time, double sigma_px,
                                const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, int64_t tag,
                                lvk_localise_info* h_info);

/* The same loop, pipelined across two HIP streams: the filter update of frame k (worker thread, ekf's context) overlaps the
 * front-end of frame k+1 (caller's thread, fe's context).  fe and ekf must have been created on DIFFERENT lvk_contexts.
 * The pipe owns the driver's IMU vector: push samples as larvioMain.cpp:98-102 does (t < t_img + 0.05) before each submit;
 * erasure happens inside, in the order the sequential loop would do it, so every result is identical to lvk_vio_process.
 * push/submit/drain are called from one thread.  Read the filter (lvk_ekf_get_*) only after lvk_vio_pipe_drain. */
typedef struct lvk_vio_pipe lvk_vio_pipe;
lvk_status lvk_vio_pipe_create(lvk_frontend* fe, lvk_ekf* ekf, lvk_vio_pipe** out);
void       lvk_vio_pipe_destroy(lvk_vio_pipe* p);
lvk_status lvk_vio_pipe_push_imu(lvk_vio_pipe* p, const lvk_imu* h_imu, int n);
lvk_status lvk_vio_pipe_submit(lvk_vio_pipe* p, const lvk_image* img, double ts, int* has_msg);
lvk_status lvk_vio_pipe_drain(lvk_vio_pipe* p, long* n_updates, long* n_msgs);
/* Called on the filter's thread after every update that processFeatures would have answered with true — the point at which the
 * reference's drivers publish odometry (app/larvioMain.cpp:117-, ros_wrapper System.cpp:177-193).  ts = the message's stamp,
 * state30 as lvk_ekf_get_state.  The filter is quiescent for the duration of the call: lvk_ekf_get_* are allowed inside it.
 * Set before the first submit (or after a drain); fn = NULL removes it. */
typedef void (*lvk_odometry_fn)(void* user, double ts, const double* state30);
lvk_status lvk_vio_pipe_on_update(lvk_vio_pipe* p, lvk_odometry_fn fn, void* user);
/* host wall time in microseconds since the last reset: [0] caller thread inside the front-end, [1] caller waiting for an erase
 * count, [2] worker inside filter updates, [3] worker waiting for a message */
lvk_status lvk_vio_pipe_stats(lvk_vio_pipe* p, double* h_out4, int reset);
/* image-in -> state-out latency (microseconds of host wall time, entry of lvk_vio_pipe_submit to the end of the update it triggered)
 * of every frame that produced a feature message since the last reset, in order; *n_out <= cap entries are written.  For a VIO this
 * is the latency that matters (the reference's timing window app/larvioMain.cpp:106-116 spans both calls). */
lvk_status lvk_vio_pipe_latency(lvk_vio_pipe* p, float* h_out_us, int cap, int* n_out, int reset);
/* Erase counts lvk_vio_pipe_submit took EARLY (from the last published camera-IMU time offset, because no IMU sample lies within
 * LVK_PIPE_TD_MARGIN [0.5 ms] of the bound the count depends on - the caller's thread then does not wait for the running update), and
 * how many of them the filter's thread found different when the update started (expected: 0; the reference's sequential schedule
 * - larvio.cpp:464-517 erasing before the next processImage reads the vector - is reproduced exactly whenever it is 0).
 * LVK_PIPE_EARLY_COUNT=0 switches the early count off (every frame after a message frame then waits for the running update). */
lvk_status lvk_vio_pipe_early_counts(lvk_vio_pipe* p, long* n_early, long* n_wrong);

#ifdef __cplusplus
}
#endif
#endif
