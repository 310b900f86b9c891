// fe_frontend.h — what the frame path's two files share (not part of the ABI): the device records of a frame (FeDev, TrackSet, HMat,
// the per-point stage codes), the front-end object with its stage profiler (ProfScope) and the calling thread's phase tracer (FeTrace,
// FT), and the launchers of fe_frame.hip that frontend.hip calls.
#pragma once
#include "lvk_internal.h"
#include <atomic>
#include <chrono>
#include <vector>

// =========================================================================== frame-level device state
struct FeDev {
    unsigned long long next_id;
    unsigned long long lk_point_levels, lk_iterations;
    int n_tracks[2];     // live tracks in set 0 / set 1
    int n_new;           // new_pts_ size
    int n_msg;           // features in the last message
    int boot_ok;         // result of the last bootstrap attempt
    int pad_;
    unsigned long long msg_features, msg_count;   // features in all published messages / messages published (mean tracks per message)
};

struct TrackSet {       // structure of arrays, capacity cap
    unsigned long long* id;
    lvk_pt2f* pts;       // curr_pts_ of the frame that wrote the set == prev_pts_ of the next frame
    lvk_pt2f* ppts;      // prev_pts_ of the frame that wrote the set (needed by getFeatureMsg)
    lvk_pt2f* init;
    int* life;
    unsigned long long* desc;   // 4 x u64 per track: first-seen descriptor
};

struct HMat { float h[9]; };

// stage codes in the per-point status byte
#define ST_ALIVE 0
#define ST_FWD   1
#define ST_REV   2
#define ST_ORB   3

struct FeMsgArgs { int publish, prev_is_last; double dt_1, dt_2; lvk_feature_obs* out; int* n_host; };

// =========================================================================== host object
#define LVK_MSG_SLOTS 4
struct lvk_frontend {
    lvk_context* ctx;
    lvk_fe_config cfg;
    int cap;
    int image_state;           // 1 FIRST_IMAGE, 2 SECOND_IMAGE, 3 OTHER_IMAGES
    bool b_first_img;
    long pub_counter;
    double last_pub_time, curr_img_time, prev_img_time;
    int cur;                   // track set holding prev_pts_ (written by the previous frame)
    lvk_pyramid* pyr[3];       // [0] = prev, [1] = curr, [2] = spare (rotated every frame: the image stage of frame k+1 fills its
    uint8_t *ext[3], *blur[3]; //  buffers on its own stream while frame k's tracking still reads [0] and [1])
    uint8_t* d_img;            // device copy of a host image
    // Host images (the reference's cv::Mat, pageable) are copied by the calling thread into a ring of pinned, device-mapped staging
    // slots; the GPU side is either one asynchronous H2D copy into d_img (default) or, with LVK_FE_ZEROCOPY=1, the first two image
    // kernels reading the slot in place over PCIe.  The caller's buffer is free as soon as the call returns (as in the reference).
    uint8_t* h_stage[3] = {nullptr, nullptr, nullptr};
    // Blocking calls (lvk_frontend_process without lvk_frontend_begin: the adapter's and the sequential driver's schedule) on a host with
    // a large BAR (every MI355X host; hipDeviceAttributeIsLargeBar): the calling thread copies the image straight into one of three
    // DEVICE buffers instead - the same ~10 us of CPU copy as into a pinned slot (tools/gpu/bar_probe.hip) and no copy command, whose
    // engine start-up + transfer (~20 us) stood in front of the frame's first kernel: sequential driver +5.6 %, adapter's schedule
    // +2.6 % (profiles/r4_al_image_bar_push_ab.txt).  The pipelined driver queues its image stage a frame ahead, where that latency
    // is hidden, and keeps the copy engine (the BAR copy measured -0.8 % there).  A buffer is reused three frames later, behind an
    // event recorded after the two kernels that read it (ev_img).
    uint8_t* d_ring[3] = {nullptr, nullptr, nullptr}; hipEvent_t ev_img[3] = {nullptr, nullptr, nullptr}; bool ev_img_set[3] = {false, false, false}; bool bar_push = false;

    int stage_next = 0;
    TrackSet set[2];
    lvk_pt2f *w_curr, *wn_curr, *new_pts;
    lvk_pt2f *w_und, *wn_und;  // undistorted (prev, curr) pair per point, written by the LK kernel next to w_curr / wn_curr
    uint8_t *w_status, *wn_status;
    unsigned long long* wn_desc;
    float* eig; uint8_t* mask; unsigned* gf_scratch; unsigned long long* gf_cands; int gf_cand_cap;
    // caller's region mask (lvk_frontend_set_mask; no reference counterpart): packed w x h, 0 / 255, allocated on first use and read-only to
    // every kernel; has_user_mask chooses k_mask_max<true> over k_mask_max<false> and hands the bootstrap detection a mask
    uint8_t* user_mask = nullptr; bool has_user_mask = false;
    // caller's pixel format (lvk_frontend_set_input_format; no reference counterpart).  MONO8: d_gray stays null and nothing below differs
    // from a front-end without the call.  Otherwise h_stage / d_ring / d_img hold RAW rows of width * bytes_per_pixel bytes and
    // lvk_image_to_gray writes the packed grey plane d_gray on the image stream.  ONE plane is enough although three frames can be in
    // flight: its only readers are the first kernels of the same frame's image stage, queued on that same stream right behind the
    // conversion, and the next frame's conversion is queued behind them - the stream's order is the lock (as for d_img itself).
    int pix_format = LVK_PIX_MONO8, pix_shift = 0; uint8_t* d_gray = nullptr;
    // The message buffer: pinned host memory (h_msg) and its device-mapped view (d_msg), and its length, same arrangement - a ring
    // of LVK_MSG_SLOTS messages so that a pipelined driver can let the GPU run ahead: processImage returns as soon as the frame is
    // queued and the filter's thread picks the message up when ev_msg[slot] has fired (lvk_frontend_fetch_msg).
    lvk_feature_obs* d_msg; lvk_feature_obs* h_msg;
    int* h_nmsg; int* d_nmsg;
    hipEvent_t ev_msg[LVK_MSG_SLOTS] = {};
    std::atomic<int> msg_pending[LVK_MSG_SLOTS];         // 1 from the publish until the message has been fetched
    int msg_next = 0;
    FeDev* dev; FeDev* h_dev;                            // device + pinned host mirror
    CamParams cam;
    // Side stream side[0] ("new points"): goodFeaturesToTrack after a publish, then the next frame's LK / descriptor gate of those
    // points.  The main stream keeps the old tracks and both commits.  With the filter's stream that makes four: HIP maps streams
    // onto 4 hardware queues by default, and two streams sharing a queue serialise (measured), so there is no fifth.
    // side[1] ("image"): upload, CLAHE, pyramid + Scharr planes and the ORB planes of a frame.  They depend on nothing but the image,
    // so with three buffer sets they run ahead of the tracking chain of the previous frame (~55 us per frame off the main chain).
    lvk_context* side[2];
    hipEvent_t ev_main[2] = {nullptr, nullptr}, ev_side[2] = {nullptr, nullptr};   // end of frame f's work on the main / side stream, by parity of f
    hipEvent_t ev_end[2] = {nullptr, nullptr};           // what stands for "frame f's main-stream work is done": ev_main[par], or the message's own event when the frame published (nothing follows it on that stream: one record, not two)
    bool frame_early = false;                            // the current frame's image stage was queued ahead of its tracking (lvk_frontend_begin: the pipelined driver)
    int last_msg_slot = -1;                              // ring entry of the message published by the current frame (-1: none)
    long n_img = 0;                                                                // image stages queued so far
    bool image_done; double image_done_ts;       // lvk_frontend_begin already queued this frame's image stage
    bool pyr_event = true;                       // this frame's image stage recorded ev_pyr (blocking API); false: ev_orb stands for the whole stage
    // fork/join events.  Each record or wait is a barrier packet on its stream (~5 us on the frame's chain), so there are as few as
    // the data flow allows: ev_pyr / ev_orb (image stream -> main and side: pyramid / ORB planes of this frame ready), ev_new (side
    // stream -> main), ev_commit (main -> side), ev_tail (bootstrap only), ev_main / ev_side (end of a frame on either stream)
    hipEvent_t ev_pyr, ev_orb, ev_new, ev_commit, ev_tail;
    bool ev_trim = true;                                 // LVK_FE_EVENT_TRIM=0: queue every event record / stream wait as rounds 1-4 did (A/B switch)
    // lvk_frontend_match_landmarks' own buffers, allocated by its first call (null in a front-end that never matches): response map, the
    // corners, their count and descriptors, then the queries, their descriptors, the matcher's results, the matched pixels, their
    // normalised coordinates and the records the host reads
    struct Match {
        float* eig; lvk_pt2f* cand_pts; int* n_cand; uint8_t* cand_desc;
        lvk_match_query* q; uint8_t* q_desc; lvk_match_result* res; lvk_pt2f *px, *und; lvk_landmark_match* out;
    } match = {};
    // lvk_frontend_align_landmarks' own buffers, allocated by its first call: the matches, the pairs, the mask and the result
    struct Align { lvk_align_match* m; lvk_align_pair* pairs; uint8_t* mask; lvk_align_result* out; } align = {};
    // the prior map of lvk_frontend_set_map (null in a front-end without one): its n points, their covariances (or null) and descriptors,
    // and lvk_frontend_match_map's own buffers, allocated with the map: the selected points' records and the counts
    struct Map { double *X, *cov; uint8_t* desc; int n; lvk_map_sel* sel; lvk_map_info* info; } map = {};
    // lvk_frontend_relocalise_map's own buffers, allocated by its first call: the search's records per corner and its selection, the selected
    // corners' pixels and normalised coordinates, and the blob that goes back in one copy (RelocBlob: result, counts, match records)
    struct RelocBlob { lvk_align_result res; lvk_global_info info; lvk_reloc_match m[1024]; };
    struct Reloc { lvk_match_result* best; lvk_global_match* sel; lvk_pt2f *px, *und; RelocBlob* blob; } reloc = {};
    // lvk_vio_localise_map's own buffer, allocated by its first call: the blob that goes back in one copy - the counts, then room for 1024
    // source rows and 1024 observations (lvk_frontend_localise_obs lays it out for the frame's n_selected)
    struct Loc { char* blob; } loc = {};
    // lvk_frontend_merge_map's own small buffers, allocated by its first call: the search's records per query and its selection, its counts,
    // the 3D alignment's matches, pairs, mask and result
    struct Merge { lvk_match_result* best; lvk_global_match* sel; lvk_global_info* ginfo; lvk_align3d_match* m; lvk_align_pair* pairs; uint8_t* mask; lvk_align_result* res; } merge = {};
    // sticky: a frame that failed AFTER its image stage was queued (device error, ring overrun) leaves the buffer-set rotation and the
    // end-of-frame events out of step with the frame count; the handle then refuses further frames instead of racing on its buffers
    lvk_status failed = LVK_OK; char failed_msg[200] = {0};
    // HIP-event profiling of stages
    unsigned prof_mask; unsigned prof_stride; bool prof_take;     // stride: bracket every n-th frame only (event records are barrier packets on the frame's critical chain)
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_free;
    double prof_ms[LVK_FE_STAGES];
    uint64_t prof_n[LVK_FE_STAGES];
};

inline hipEvent_t prof_event(lvk_frontend* fe)
{
    if (!fe->ev_free.empty()) { hipEvent_t e = fe->ev_free.back(); fe->ev_free.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
}
struct ProfScope {
    lvk_frontend* fe; int stage; hipEvent_t a; bool on;
    hipStream_t st;
    ProfScope(lvk_frontend* f, int s, hipStream_t stream = nullptr) : fe(f), stage(s), on(((f->prof_mask >> s) & 1u) && f->prof_take), st(stream ? stream : f->ctx->stream)
    { if (on) { a = prof_event(fe); hipEventRecord(a, st); } }
    ~ProfScope() { if (on) { hipEvent_t b = prof_event(fe); hipEventRecord(b, st); fe->pending.push_back({stage, a, b}); } }
};

// host-side phase tracer of the calling thread (LVK_FE_TRACE=1; printed by lvk_frontend_destroy): where the caller's time per frame goes
enum { FT_SLOT_WAIT, FT_STAGE_COPY, FT_UPLOAD, FT_IMAGE_LAUNCH, FT_OUTSIDE, FT_FRAME_WAITS, FT_PREDICT, FT_TRACK_LAUNCH, FT_COMMIT_LAUNCH, FT_PUBLISH, FT_DETECT, FT_END, FT_N };
struct FeTrace {
    bool on = false; double acc[FT_N] = {0}; long n = 0; std::chrono::steady_clock::time_point last;
    void start() { if (on) last = std::chrono::steady_clock::now(); }
    void mark(int k) { if (!on) return; auto t = std::chrono::steady_clock::now(); acc[k] += std::chrono::duration<double, std::micro>(t - last).count(); last = t; }
};
extern FeTrace g_ft;                                     // frontend.hip, with the names its report prints
#define FT(k) g_ft.mark(k)

// =========================================================================== what frontend.hip calls in fe_frame.hip
// The library is built without relocatable device code: a kernel is launched from the file that defines it, so the frame path's
// launches are these calls.
// one track set's LK + descriptor gate on `stream`
lvk_status track_chain(lvk_frontend* fe, hipStream_t stream, const lvk_pt2f* src_pts, const int* n_ptr, const HMat& H, lvk_pt2f* w_curr, uint8_t* w_status,
                       const unsigned long long* stored_desc, unsigned long long* w_desc, int is_new);
// both sets' in ONE launch (lvk_lk_choice(...).merged)
lvk_status track_chain_merged(lvk_frontend* fe, hipStream_t stream, int src, const HMat& H);
// RANSAC + write of the destination track set on the main stream; mode 0 old tracks, 1 new points appended, 2 bootstrap
lvk_status commit(lvk_frontend* fe, int mode, const lvk_pt2f* src_pts, const int* n_ptr, const lvk_pt2f* w_curr, const uint8_t* w_status,
                  const TrackSet* src, const unsigned long long* desc_src, int dst_set);
// the feature message of set `dst` on the main stream
lvk_status fe_msg_launch(lvk_frontend* fe, int dst, const FeMsgArgs& m);
// fe_match.hip: matched pixels, their normalised coordinates and the host's records behind lvk_orb_match_guided, on the context's stream
lvk_status fe_match_finish(lvk_context* ctx, const CamParams& cam, const lvk_match_result* d_res, const lvk_pt2f* d_cand_pts, int n_q, lvk_pt2f* d_px, lvk_pt2f* d_und,
                           lvk_landmark_match* d_out);
// fe_map.hip: rows * cols * quota of the options as lvk_map_select_queries reads them, -1 when it refuses them
int fe_map_max_selected(const lvk_map_select_options* opt);
// fe_mapobs.hip: the launch behind lvk_map_gather_obs on the context's stream, for records whose map index and whose lvk_landmark_match lie
// at idx_base + k idx_stride and m_base + k m_stride (bytes): one array of lvk_map_match, or the selection's and the matcher's own arrays
lvk_status fe_map_gather_launch(lvk_context* ctx, const void* idx_base, int idx_stride, const void* m_base, int m_stride, int n_rec, const double* d_X, const double* d_cov,
                                int n_map, const lvk_align_result* align, double sigma, lvk_landmark_obs* d_obs, int* d_idx, lvk_map_obs_info* d_info);
// fe_global.hip: behind lvk_orb_match_global on the context's stream - the n selected corners' pixels, their normalised coordinates, the
// alignment's match records and the host's records (inlier 0); then, behind lvk_align_ransac_2pt, inlier = the mask byte
lvk_status fe_reloc_gather(lvk_context* ctx, const CamParams& cam, const lvk_global_match* d_sel, int n, const lvk_pt2f* d_cand_pts, const double* d_X, lvk_pt2f* d_px,
                           lvk_pt2f* d_und, lvk_align_match* d_am, lvk_reloc_match* d_out);
lvk_status fe_reloc_inliers(lvk_context* ctx, const uint8_t* d_mask, int n, lvk_reloc_match* d_out);
// fe_mapbuild.hip: does lvk_map_build accept these options (false: *why names the field)?  lvk_frontend_build_map asks before it allocates
bool fe_map_build_options_ok(const lvk_map_build_options* opt, const char** why);
// fe_align3d.hip: does lvk_align_ransac_3d accept these options?  And, behind lvk_orb_match_global on the context's stream, the 3D alignment's
// match records of lvk_frontend_merge_map: X = point `cand` of the n_b sorted points of B, Y = point `index` of the n_a resident points
bool fe_align3d_options_ok(const lvk_align3d_options* opt, const char** why);
lvk_status fe_merge_gather(lvk_context* ctx, const lvk_global_match* d_sel, int n, const double* d_XB, int n_b, const double* d_XA, int n_a, lvk_align3d_match* d_out);
#ifdef LVK_LK_BOUNDS
void fe_lk_bounds_report();                             // prints what the frame path's kernels recorded in THEIR copy of g_lk_oob
#endif
