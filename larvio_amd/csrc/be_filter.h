// be_filter.h — the filter object as its own translation units see it (backend.hip and the stages it runs: be_propagate.hip,
// be_triangulate.hip, be_update.hip, be_prune.hip, be_initialize.hip; be_export.hip, be_pipe.hip): the host records, struct lvk_ekf
// with its deferred-update worker, the records the stages pass one another (row jobs, triangulation requests), the phase tracer, and
// the few inline helpers that more than one of those files needs.  Nothing here is visible outside liblvk_hip.so; what the files
// call in one another is declared in be_host.h.
#pragma once
#include "lvk_internal.h"
#include "be_dev.h"
#include "be_host.h"
#include "be_qr.h"
#include <vector>
#include <map>
#include <stdexcept>
#include <algorithm>
#include <iterator>
#include <atomic>
#include <functional>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <chrono>
namespace lvk_init { struct DynInit; }

#define LEG (e->leg)           // LEG_DIM: 22, or 46 with online IMU-intrinsics calibration (larvio.cpp:158-161)
#define LEG_MAX 46

// ------------------------------------------------------------------------- host records
struct Obs { long long sid; double z[2], zv[2]; };
struct Feature {
    long long id = 0;
    std::vector<Obs> obs;                  // ascending state id (std::map in the reference)
    double position[3] = {0, 0, 0}, position_fej[3] = {0, 0, 0};
    bool is_initialized = false;
    long long id_anchor = -1;
    double inv_depth = 0, obs_anchor[3] = {0, 0, 0};
    bool in_state = false, ekf_feature = false;
    int total_obs = 0;
    int find(long long sid) const
    {   // obs is sorted by state id and almost every query asks for the newest one or two: look there first, then bisect
        const int n = (int)obs.size();
        if (n == 0) return -1;
        if (obs[n - 1].sid == sid) return n - 1;
        if (obs[n - 1].sid < sid) return -1;
        if (n >= 2 && obs[n - 2].sid == sid) return n - 2;
        int lo = 0, hi = n - 2;                                   // first index with sid >= wanted, in [0, n-2)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (obs[mid].sid < sid) lo = mid + 1; else hi = mid; }
        return (lo < n && obs[lo].sid == sid) ? lo : -1;
    }
    void set(long long sid, double u, double v, double uv, double vv)
    {
        int i = find(sid);
        if (i < 0) {
            Obs o; o.sid = sid;
            auto it = obs.end(); while (it != obs.begin() && (it - 1)->sid > sid) --it;     // appended at the end in the normal case
            it = obs.insert(it, o); i = (int)(it - obs.begin());
        }
        obs[i].z[0] = u; obs[i].z[1] = v; obs[i].zv[0] = uv; obs[i].zv[1] = vv;
    }
    void erase(long long sid) { int i = find(sid); if (i >= 0) obs.erase(obs.begin() + i); }
    void reset(long long new_id)
    {   // the state of Feature() with this id; the observation list keeps its capacity (recycled objects: no allocation per new track)
        id = new_id; obs.clear();
        for (int k = 0; k < 3; ++k) { position[k] = 0; position_fej[k] = 0; obs_anchor[k] = 0; }
        is_initialized = false; id_anchor = -1; inv_depth = 0; in_state = false; ekf_feature = false; total_obs = 0;
    }
};

// map_server (std::map<FeatureIDType, Feature> in the reference, include/larvio/larvio.h:150): an id-ordered container with the slice
// of the std::map interface the filter uses.  Ids are handed out in increasing order and features die in bulk, so the order lives
// in ONE sorted array of (id, pointer) slots: lookups are a bisection over 16-byte entries that stay in cache, new tracks are appended,
// a walk in id order is a linear scan (the next features' records are prefetched on the way), and erase only marks the slot -
// the marks are swept once per message (purge()), after the message had its chance to re-create a feature that was used and erased
// while its track lived on (every track is, every max_track_len frames; larvio.cpp:2240-2246).  Feature objects come from a free
// list and keep their address while they are in the map (the update's row jobs hold pointers to them).
// At configs[4] (2000 tracks) the std::map's pointer chasing was ~130 us per message in add_observations alone and as much again in the
// scans of the update.
class FeatureMap {
  public:
    struct Slot { long long id; Feature* f; bool live; };
    struct Ref { const long long first; Feature& second; Ref* operator->() { return this; } };
    class iterator {
      public:
        typedef std::forward_iterator_tag iterator_category; typedef Ref value_type; typedef long difference_type; typedef Ref* pointer; typedef Ref reference;
        iterator() : m(nullptr), i(0) {}
        iterator(const FeatureMap* m_, size_t i_) : m(m_), i(i_) { skip(); }
        Ref operator*() const { const Slot& s = m->slots[i]; return Ref{s.id, *s.f}; }
        Ref operator->() const { return **this; }
        iterator& operator++() { ++i; skip(); return *this; }
        iterator operator++(int) { iterator t = *this; ++*this; return t; }
        bool operator==(const iterator& o) const { return i == o.i; }
        bool operator!=(const iterator& o) const { return i != o.i; }
        size_t index() const { return i; }
      private:
        void skip()
        {
            const size_t n = m->slots.size();
            while (i < n && !m->slots[i].live) ++i;
            if (i + 8 < n) {                                      // records a few features ahead: the object, then (one step later) its observations
                __builtin_prefetch(m->slots[i + 8].f);
                const Feature* g = m->slots[i + 4].f;
                __builtin_prefetch((const char*)g + 64); __builtin_prefetch(g->obs.data());
            }
        }
        const FeatureMap* m; size_t i;
        friend class FeatureMap;
    };
    FeatureMap() {}
    FeatureMap(const FeatureMap&) = delete;
    FeatureMap& operator=(const FeatureMap&) = delete;
    ~FeatureMap() { for (Slot& s : slots) delete s.f; for (Feature* f : spare) delete f; }
    size_t size() const { return n_live; }
    bool empty() const { return n_live == 0; }
    iterator begin() const { return iterator(this, 0); }
    iterator end() const { iterator it; it.m = this; it.i = slots.size(); return it; }
    iterator find(long long id) const { const size_t k = lower(id); return (k < slots.size() && slots[k].id == id && slots[k].live) ? at_index(k) : end(); }
    Feature& at(long long id) const { const size_t k = lower(id); if (!(k < slots.size() && slots[k].id == id && slots[k].live)) throw std::out_of_range("FeatureMap::at"); return *slots[k].f; }
    Feature& operator[](long long id) { return *slots[obtain(id)].f; }
    // both emplace forms: the feature value is always a fresh one in the callers (Feature()), so only the id is used
    std::pair<iterator, bool> emplace(long long id, const Feature&) { const size_t before = n_live; const size_t k = obtain(id); return std::make_pair(at_index(k), n_live != before); }
    iterator emplace_hint(const iterator&, long long id, const Feature&) { return at_index(obtain(id)); }
    size_t erase(long long id) { const size_t k = lower(id); if (!(k < slots.size() && slots[k].id == id && slots[k].live)) return 0; slots[k].live = false; --n_live; ++n_dead; return 1; }
    iterator erase(const iterator& it) { Slot& s = slots[it.i]; if (s.live) { s.live = false; --n_live; ++n_dead; } return iterator(this, it.i + 1); }
    // sweep the erased slots (their objects go back to the free list); invalidates iterators, keeps the addresses of live features
    void purge()
    {
        if (!n_dead) return;
        size_t w = 0;
        for (size_t r = 0; r < slots.size(); ++r) { if (slots[r].live) slots[w++] = slots[r]; else spare.push_back(slots[r].f); }
        slots.resize(w); n_dead = 0;
    }
  private:
    size_t lower(long long id) const
    {   // first slot with id >= wanted; the newest ids are asked for most
        const size_t n = slots.size();
        if (n == 0 || slots[n - 1].id < id) return n;
        size_t lo = 0, hi = n - 1;
        while (lo < hi) { const size_t mid = (lo + hi) >> 1; if (slots[mid].id < id) lo = mid + 1; else hi = mid; }
        return lo;
    }
    iterator at_index(size_t k) const { iterator it; it.m = this; it.i = k; return it; }
    Feature* fresh(long long id) { Feature* f; if (!spare.empty()) { f = spare.back(); spare.pop_back(); } else f = new Feature(); f->reset(id); return f; }
    size_t obtain(long long id)
    {   // index of the live slot of `id`, creating it (as a default feature) if there is none
        const size_t k = lower(id);
        if (k < slots.size() && slots[k].id == id) {
            if (!slots[k].live) { slots[k].f->reset(id); slots[k].live = true; ++n_live; --n_dead; }      // erased earlier in this message cycle: a new feature under the old id
            return k;
        }
        Slot s; s.id = id; s.f = fresh(id); s.live = true;
        slots.insert(slots.begin() + (long)k, s);               // k == size() for a new track (ids grow): an append
        ++n_live;
        return k;
    }
    std::vector<Slot> slots; std::vector<Feature*> spare; size_t n_live = 0, n_dead = 0;
};
struct Clone {
    long long id; double time, dt; double q[4], p[3], p_fej[3], R_b2c[9], t_c_b[3], q_cam[4], p_cam[3];
};
struct ImuS { double t; double q[4], p[3], v[3], bg[3], ba[3]; };

typedef lvk_status (*lvk_feats_fn)(void* user, const lvk_feature_obs** feats, int* n_feats);
struct lvk_ekf {
    lvk_context* ctx;
    lvk_ekf_config cfg;
    // state_server
    long long imu_id = 0; double imu_dt = 0;
    ImuS s, s_old, s_fej_now, s_fej_old;
    double R_b2c[9], t_c_b[3], td = 0;
    std::vector<Clone> clones;
    mutable std::vector<short> rank_tab; mutable long long rank_base = 0; mutable bool ranks_dirty = true;   // see clone_rank()
    mutable std::vector<double> rcam; mutable bool rcam_valid = false;      // camera-to-world rotation of every clone (clone_Rcam), rebuilt after poses change
    std::vector<long long> feature_states;
    FeatureMap map;                                    // map_server (ascending id)
    int leg = 22;
    int N = 22;
    double imx[24];                                     // T1 T2 T3 A1 A2 A3 M1 M2 (larvio.cpp:129-154)
    double Tg[9], As[9], Ma[9];                         // updateImuMx (:3803-3846)
    long long next_state_id = 0;
    bool is_gravity_set = false, b_first_features = false, if_fej = false, if_zupt = false;
    double m_gyro_old[3], m_acc_old[3];
    double take_off_stamp = 0, last_update_time = 0, last_zupt_time = 0, tracking_rate = 0;
    struct LostPoint { long long id; double p[3]; double cov[9]; };
    std::vector<LostPoint> lost_slam;                   // in-state features that were lost, with their last world position (drained on read)
    // lvk_ekf_set_lost_feature_cov: the position covariance of every lost point, computed (k_landmark_cov) before its column leaves P.
    // lost_cov_slot: for the last lost_cov_slot.size() entries of lost_slam, where in the download buffer (down_lm) the kernel puts
    // their Sigma (-1: no job, the anchor is outside the window); attached at the end of the call, behind a stream sync
    // (lost_cov_mark = n_sync when the launch was queued: one more sync only if none has followed)
    bool lost_cov_on = false; std::vector<int> lost_cov_slot; int lost_cov_mark = 0; size_t down_lm = 0; int lm_cap = 0;
    // lvk_ekf_set_msckf_points: the MSCKF features a lost-feature update used and erased, with the position covariance k_msckf_point_cov
    // computed for them ahead of that update (drained on read).  The kernel covers jobs [mp_lo, mp_lo + mp_n) of the update's batch and
    // writes job k's Sigma / ok word to slot k - mp_lo of the download buffer (down_mp / down_mpok)
    struct MsckfPoint { long long id; double p[3]; double cov[9]; int n_obs; };
    std::vector<MsckfPoint> msckf_points;
    bool msckf_points_on = false; size_t down_mp = 0, down_mpok = 0, mp_lo = 0; int mp_cap = 0, mp_n = 0;
    // lvk_ekf_set_keyframe_export: the clones the pruning removes, each with its absolute 6 x 6 block and the covariance of its pose
    // relative to the nearest newer surviving clone (k_pose_rel_cov), computed before its columns leave P (drained on read).
    // kf_pending: the last kf_pending entries of keyframes wait for their results - record i's absolute block in slot 2 i of the
    // download buffer (down_kf), its relative one in slot 2 i + 1 - attached like the lost-feature covariance (kf_mark as lost_cov_mark)
    std::vector<lvk_keyframe> keyframes;
    bool keyframes_on = false; size_t down_kf = 0; int kf_pending = 0, kf_mark = 0;
    // lvk_ekf_add_fix: external position / pose fixes waiting for their clone (at most FIX_CAP), applied by lvk_ekf_apply_fixes
    // (be_fix.hip) once per message; one report per consumed fix (drained on read).  fix_stats: [0] queued so far [1] applied [2] gated
    // [3] not positive definite [4] stale [5] no clone [7] interpolated among the applied ([6], waiting, is fix_queue.size())
    enum { FIX_CAP = 64 };
    std::vector<lvk_fix> fix_queue; std::vector<lvk_fix_report> fix_reports;
    double fix_gate_scale = 1.0, fix_max_gap = 0.0; long fix_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // lvk_ekf_add_landmark_obs: batches of observations of known landmarks waiting for their clone (at most LM_CAP), applied by
    // lvk_ekf_apply_landmarks (be_landmark_fix.hip) behind the fixes; one report per consumed batch (drained on read).  lm_stats: as
    // lvk_ekf_landmark_stats hands them out ([6], waiting, is lm_queue.size())
    enum { LM_CAP = 16 };
    struct LmBatch { long long tag, clone_id; double time; std::vector<lvk_landmark_obs> obs; };
    std::vector<LmBatch> lm_queue; std::vector<lvk_landmark_report> lm_reports;
    double lm_gate_scale = 1.0, lm_min_depth = 0.1; long lm_stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double sigma2, zupt_v2, zupt_p2, zupt_q2, imu_img_time_th, Qc[12];
    double x_min, y_min, grid_w, grid_h;
    std::vector<int> grid_count;
    // The reference's grid_map is a std::map<int, vector> (larvio.h:383): a feature whose code falls outside the rows x cols cells (undistorted
    // coordinates beyond the image bounds) gets a cell of its own, which updateGridMap never clears (larvio.cpp:3356-3366) - it only fills up
    // and, once it holds max_features_in_one_grid ids, diverts every later feature with that code to the MSCKF branch (:1969-1975).
    // reference_grid (the default) keeps that bookkeeping; lvk_ekf_config.legacy_grid = 1 or LVK_GRID_REFERENCE=0 selects what this
    // library did before round 6 (such codes not counted at all) - an opt-out for comparing old records, not the reference's filter.
    std::map<int, int> grid_phantom;
    bool reference_grid = true;
    std::vector<double> coarse_dis;
    int static_counter = 0, static_num = 0; double lower_time_bound = 0;
    lvk_status dyn_status = LVK_OK;
    lvk_init::DynInit* dyn = nullptr;                    // the moving-start initialiser (be_init.h); lives until the filter has a state
    char* d_dyn = nullptr; size_t dyn_cap = 0;           // device scratch of its RANSAC stage (dyn_ransac): grow-only
    lvk_init_report init_report = {};                    // what it handed over (lvk_ekf_init_report); valid = 0 until it has
    int init_calls = 0, init_ransac_calls = 0;
    std::map<long long, std::pair<double, double>> init_features;
    long counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    lvk_status failed = LVK_OK; char failed_msg[256] = {0};   // sticky: set by the first lvk_ekf_process that returned an error
    // per-frame composed transition (processModel): Phi_tot, Q_tot
    double Phi_tot[LEG_MAX * LEG_MAX], Q_tot[LEG_MAX * LEG_MAX]; bool have_prop = false;
    // device
    int ld = 0, nmax = 0, rows_cap = 0, hrows = 0, feat_cap = 0, obs_cap = 0;
    double* dP[2] = {nullptr, nullptr}; int cur = 0;
    int* d_idx = nullptr; double *d_phiq = nullptr, *d_J = nullptr, *d_dx = nullptr, *d_tmp = nullptr;
    TriJob* d_tri = nullptr; TriResult* d_triout = nullptr; FeatJob* d_fj = nullptr; FeatResult* d_fout = nullptr;
    TriResult* d_tridev = nullptr;                      // device copy of the triangulation results, indexed by the row job that consumes them (FJ_TRI_PENDING)
    int* d_rank = nullptr; double *d_z = nullptr, *d_zv = nullptr; CamPose* d_cams = nullptr; CloneDev* d_clones = nullptr;
    double* d_staging = nullptr; size_t staging_cap = 0; int* d_ccols = nullptr; size_t ccols_cap = 0; StackRow* d_map = nullptr;
    double *d_H = nullptr, *d_r = nullptr, *d_H1 = nullptr, *d_H2 = nullptr, *d_r1 = nullptr;
    double *d_Hb = nullptr, *d_rb = nullptr;            // ping-pong partner of d_H / d_r for the levels of the structure-aware compression
    int sparse_qr_min_rows = 480;
    std::vector<int> tri_ranks; std::vector<double> tri_z;       // view pools of the triangulation requests of the current batch
    struct ColCache { int type = -1, ncols = 0, anchor = 0, fcol = 0; std::vector<long long> sids; ColList cols; };
    mutable ColCache colcache;                          // job_dense_cols: the column list of the previous job, reused when the next one has the same observation set
    long qr_stats[4] = {0, 0, 0, 0};                    // [0] updates compressed [1] levels run [2] rows in [3] rows out
    // sharded measurement update: this rank builds the feature rows of its contiguous slice, one all-gather of the
    // compressed blocks (+ every feature's gate result), replicated update.  fn == nullptr = off; with a transport the sharded path
    // runs at any world size, world 1 included (a loop-back that exercises pack -> all-gather -> unpack -> second stage on one GPU).
    // The exchange buffers are allocated once, in lvk_ekf_set_shard, for xk_cap block rows per rank: nothing that can fail on one
    // rank only sits between the ranks and their collective.
    struct Shard { int rank = 0, world = 1; lvk_exchange_fn fn = nullptr; void* user = nullptr; char *d_send = nullptr, *d_recv = nullptr; size_t cap = 0; int xk_cap = 0;
                   long stats[4] = {0, 0, 0, 0}; } shard;     // stats: [0] exchanges [1] bytes sent per rank (sum) [2] sharded updates [3] rows this rank stacked
    size_t down_flag = 0;                               // offset in h_down of the word k_shard_unpack raises when a peer's block arrives poisoned
    size_t down_info = 0;                               // offset in h_down of the factorisation's report words (update_health)
    size_t down_p00 = 0; bool p00_valid = false;        // offset in h_down of the mirror of P[0:16, 0:16] (q v p bg ba[0]) the last update's final GEMM wrote; valid: nothing has touched that block since
    UpdateWs ws;
    // what to do when the Cholesky meets a non-positive pivot (lvk_ekf_set_indefinite_policy).  The update's last launch leaves P
    // and dx alone then (GemmRider::gate), so under LVK_INDEFINITE_LDLT update_health() runs that one update again through the
    // pivoted LDL^T: `last` is the stacked system the failed update read (still in place: nothing writes d_H / d_r before the sync
    // that looks at the report), `redo` what the caller had queued behind the update and has to be queued again behind the new one.
    int indefinite_policy = LVK_INDEFINITE_FAIL; long indefinite_fallbacks = 0;
    struct LastUpdate { const double* H = nullptr; const double* r = nullptr; int m = 0, n = 0; } last;
    std::function<lvk_status()> redo;
    bool fell_back = false;                             // set by update_health when it re-ran the update: d_dx has changed since the caller's copy was queued
    // pinned host arenas
    char* h_up = nullptr; size_t up_cap = 0, up_off = 0, up_flushed = 0;
    size_t up_lim = 0; int up_half = 0;                 // the arena is used in halves, alternating per call: kernels queued behind a call's last sync may still read its half while the next call stages into the other
    int n_sync = 0;                                     // stream syncs of the current call (a call without any ends with one: see ekf_process_impl)
    char* d_up = nullptr;                               // device mirror of the upload arena: ONE H2D copy per sync point
    bool zero_copy = false;                             // d_up aliases the pinned arena (device-mapped host memory): no H2D copies at all
    bool bar_push = false;                              // d_up is DEVICE memory that this thread writes through the PCIe BAR (flush_uploads): see lvk_ekf_create
    int defer = 0; std::vector<std::function<lvk_status()>> deferred;   // launches waiting for a shared flush (begin_defer/end_defer)
    CamPose* dv_cams = nullptr; CloneDev* dv_clones = nullptr;
    // results come back WITHOUT copies: the kernels that produce them (triangulation, per-feature rows, the dx column of W^T[W|w])
    // also write them into this device-mapped pinned buffer; the host reads it after the stream sync it needs anyway
    char* h_down = nullptr; size_t down_cap = 0; char* dh_down = nullptr; size_t down_feat = 0, down_dx = 0;
    // fired as soon as the number of IMU samples this call erases is final (before any GPU work): lets a pipelined driver
    // hand the next frame's front-end the right buffer view while this update is still running
    void (*on_consumed)(void*, int) = nullptr; void* on_consumed_user = nullptr;
    // one update with the sticky failure state kept (backend.hip's ekf_process_guarded, set by lvk_ekf_create; fetch, when given, delivers
    // the message once the IMU batch is counted).  be_pipe.hip calls it through the handle: no object calls a function of backend.o
    lvk_status (*process)(lvk_ekf* e, double ts, const lvk_feature_obs* feats, int n_feats, const lvk_imu* imu, int n_imu, int* n_consumed, int* updated, lvk_feats_fn fetch, void* fetch_user) = nullptr;
    // optional HIP-event bracket around the H P GEMM of every update (bench: MFMA utilisation of the P H^T contraction)
    bool prof_on = false; double prof_ms = 0, prof_flops = 0; long prof_n = 0;
    double prof_qr_ms = 0, prof_qr_flops = 0, prof_qr_rows = 0; long prof_qr_n = 0;     // the same bracket around every k_qr_sparse level (kind 1)
    struct ProfEv { hipEvent_t a, b; double flops; int kind = 0; double rows = 0; };
    struct Async;                                       // lvk_ekf_process_async: the worker that runs a queued update (created on first use)
    Async* async = nullptr;
    std::vector<ProfEv> prof_pending; std::vector<hipEvent_t> prof_free;
};

// ------------------------------------------------------------------------- deferred updates
// lvk_ekf_process_async hands an update to this worker and returns; the next call that looks at the filter (any getter, the next
// update, destroy) waits for it.  A blocking driver (app/larvioMain.cpp:104-116: processImage, processFeatures, getters) then gets
// the front-end of the next frame running while the update of this one is still in flight, as far as its own getter calls allow.
struct lvk_ekf::Async {
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::atomic<int> state{0};                          // 0 idle, 1 an update is queued or running
    std::atomic<bool> stop{false};
    double ts = 0; std::vector<lvk_feature_obs> feats; std::vector<lvk_imu> imu; int expect_used = 0;
    lvk_status st = LVK_OK; int updated = 0; long n_deferred = 0;
    bool unwaited = false;                              // an update was queued and no call has waited for it yet (caller's thread only)
};
// every entry point that reads or changes the filter first waits for the queued update
static void ekf_quiesce(const lvk_ekf* e)
{
    lvk_ekf::Async* a = e->async;
    if (a) a->unwaited = false;
    if (!a || a->state.load(std::memory_order_acquire) == 0) return;
    for (int spin = 0; spin < 40000; ++spin) { if (a->state.load(std::memory_order_acquire) == 0) return; LVK_CPU_RELAX(); }
    std::unique_lock<std::mutex> lk(a->mu);
    a->cv.wait(lk, [&] { return a->state.load(std::memory_order_acquire) == 0; });
}

// ------------------------------------------------------------------------- small helpers
// rank of a clone in the window by state id: direct-address table over [first id, last id] (ids only grow; the window spans a few
// dozen of them), rebuilt lazily after the clone list changes - the linear search ran thousands of times per update
static inline int clone_rank(const lvk_ekf* e, long long id)
{
    if (e->ranks_dirty) {
        e->rank_tab.clear();
        e->rank_base = e->clones.empty() ? 0 : e->clones.front().id;
        if (!e->clones.empty()) {
            e->rank_tab.assign((size_t)(e->clones.back().id - e->rank_base + 1), (short)-1);
            for (size_t i = 0; i < e->clones.size(); ++i) e->rank_tab[(size_t)(e->clones[i].id - e->rank_base)] = (short)i;
        }
        e->ranks_dirty = false;
    }
    const long long k = id - e->rank_base;
    return (k < 0 || k >= (long long)e->rank_tab.size()) ? -1 : e->rank_tab[(size_t)k];
}
static inline int fs_rank(const lvk_ekf* e, long long id) { for (size_t i = 0; i < e->feature_states.size(); ++i) if (e->feature_states[i] == id) return (int)i; return -1; }
template <typename T> static inline T* up_alloc(lvk_ekf* e, size_t n)
{   // bump allocation in the pinned upload arena (reset once per frame; copies are stream-ordered)
    size_t bytes = (sizeof(T) * n + 63) & ~(size_t)63;
    if (e->up_off + bytes > e->up_lim) return nullptr;
    T* p = (T*)(e->h_up + e->up_off); e->up_off += bytes; return p;
}
#define EKF_HIP(call) LVK_HIP(e->ctx, call)
template <typename T> static inline T* dev(lvk_ekf* e, T* host) { return (T*)(e->d_up + ((char*)host - e->h_up)); }
static inline lvk_status flush_uploads(lvk_ekf* e)
{   // everything staged in the pinned arena since the last flush goes up in one stream-ordered copy
    if (e->bar_push) {                                                   // the host pushes what it staged into the device-resident arena
        if (e->up_off > e->up_flushed) { memcpy(e->d_up + e->up_flushed, e->h_up + e->up_flushed, e->up_off - e->up_flushed); LVK_STORE_FENCE(); e->up_flushed = e->up_off; }
        return LVK_OK;
    }
    if (e->zero_copy) { e->up_flushed = e->up_off; return LVK_OK; }     // kernels read the pinned arena directly
    if (e->up_off > e->up_flushed) {
        EKF_HIP(hipMemcpyAsync(e->d_up + e->up_flushed, e->h_up + e->up_flushed, e->up_off - e->up_flushed, hipMemcpyHostToDevice, e->ctx->stream));
        e->up_flushed = e->up_off;
    }
    return LVK_OK;
}
// A launch that reads staged data.  Normally: flush what is staged, launch.  Between begin_defer and end_defer the launches are held
// back so that several of them share ONE host-to-device copy (each copy is ~4 us on the filter's dependent chain plus its barrier).
static inline lvk_status run_or_defer(lvk_ekf* e, std::function<lvk_status()> fn)
{
    if (e->defer > 0) { e->deferred.push_back(std::move(fn)); return LVK_OK; }
    lvk_status st = flush_uploads(e);
    return st == LVK_OK ? fn() : st;
}
static inline void ekf_state30(const lvk_ekf* e, double* o)
{   // the 30 values of lvk_ekf_get_state
    o[0] = e->s.t; memcpy(o + 1, e->s.q, 32); memcpy(o + 5, e->s.v, 24); memcpy(o + 8, e->s.p, 24); memcpy(o + 11, e->s.bg, 24); memcpy(o + 14, e->s.ba, 24);
    memcpy(o + 17, e->R_b2c, 72); memcpy(o + 26, e->t_c_b, 24); o[29] = e->td;
}
// how many samples batch_imu will erase, without touching the state: time stamps only - the state time t0, the bound (image time +
// td) and the threshold.  t_after = the state time batch_imu leaves behind.
static inline int imu_erase_count(double t0, double time_bound, double th, const lvk_imu* imu, int n_imu, double* t_after)
{
    int used = 0; double t = t0;
    for (int i = 0; i < n_imu; ++i) {
        if (imu[i].t <= t) { ++used; continue; }
        if (imu[i].t - time_bound > th) break;
        t = imu[i].t; ++used;
    }
    if (t_after) *t_after = t;
    return used;
}
static inline int batch_imu_count(const lvk_ekf* e, double time_bound, const lvk_imu* imu, int n_imu, double* t_after = nullptr)
{
    return imu_erase_count(e->s.t, time_bound, e->imu_img_time_th, imu, n_imu, t_after);
}
// a record joins a list that is drained on read: one nobody reads is capped - at 65,536 records the oldest 32,768 go
template <typename T> static inline void drain_append(std::vector<T>& list, const T& rec)
{
    if (list.size() >= (size_t)1 << 16) list.erase(list.begin(), list.begin() + (1 << 15));
    list.push_back(rec);
}
// hdev: the job's record in the upload arena (patched until the launch is flushed); tri >= 0: the triangulation request (index in the
// caller's batch) whose result the row kernel consumes on the device (FJ_TRI_PENDING) and the host reads after the update
struct RowJob { Feature* f; int type; std::vector<long long> sids; bool want_gate; int dof; FeatJob dev; FeatResult res; FeatJob* hdev = nullptr; int tri = -1; };
struct RowObs { const int* rank = nullptr; const double *z = nullptr, *zv = nullptr; };      // where a batch's observations lie on the device (FeatJob::obs_off indexes them)

// ------------------------------------------------------------------------- host-side phase tracer (LVK_EKF_TRACE=1)
// one instance for all the filter's files (backend.hip defines it, with the names its report prints)
enum { TR_IMU, TR_PROP, TR_FETCH, TR_ADDOBS, TR_ZUPT, TR_RLF_PRE, TR_RLF_TRI, TR_RLF_TRIAGE, TR_RLF_ROWS, TR_RLF_UPD, TR_RLF_DX, TR_RLF_INJ,
       TR_PR_PRE, TR_PR_TRI, TR_PR_ROWS, TR_PR_UPD, TR_PR_DX, TR_PR_END, TR_FINAL, TR_N };
struct EkfTrace {
    bool on = false; double acc[TR_N] = {0}; long n = 0;
    double sub_acc[8] = {0}; std::chrono::steady_clock::time_point last_sub; long cnt[4] = {0, 0, 0, 0};      // cnt: updates above 160 rows / plans drawn up / compressions taken / rows of those updates      // finer marks inside one phase (TRS): time since the previous mark of either kind
    double cur[TR_N] = {0};                              // this update's phases: an update above LVK_EKF_TRACE_SLOW_US is printed on its own
    std::chrono::steady_clock::time_point last;
    void start() { if (on) { last = last_sub = std::chrono::steady_clock::now(); for (int i = 0; i < TR_N; ++i) cur[i] = 0; } }
    void mark(int slot) { if (!on) return; auto t = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double, std::micro>(t - last).count(); acc[slot] += d; cur[slot] += d; last = t; last_sub = t; }
    void sub(int k) { if (!on) return; auto t = std::chrono::steady_clock::now(); sub_acc[k] += std::chrono::duration<double, std::micro>(t - last_sub).count(); last_sub = t; }
    void end_update(const char* const* names)
    {
        static const double slow = [] { const char* v = getenv("LVK_EKF_TRACE_SLOW_US"); return v ? atof(v) : 0.0; }();
        if (!on || slow <= 0) return;
        double tot = 0; for (int i = 0; i < TR_N; ++i) tot += cur[i];
        if (tot < slow) return;
        fprintf(stderr, "[lvk_ekf trace] slow update %ld: %.0f us:", n, tot);
        for (int i = 0; i < TR_N; ++i) if (cur[i] > 0.02 * tot) fprintf(stderr, " %s %.0f;", names[i], cur[i]);
        fprintf(stderr, "\n");
    }
};
extern EkfTrace g_tr;
#define TR(slot) g_tr.mark(slot)
#define TRS(k) g_tr.sub(k)

// ------------------------------------------------------------------------- helpers of more than one stage
static void update_imu_mx(lvk_ekf* e)
{   // larvio.cpp:3803-3846
    const double *T1 = e->imx, *T2 = e->imx + 3, *T3 = e->imx + 6, *A1 = e->imx + 9, *A2 = e->imx + 12, *A3 = e->imx + 15, *M1 = e->imx + 18, *M2 = e->imx + 21;
    double* Tg = e->Tg; double* As = e->As; double* Ma = e->Ma;
    Tg[0] = T2[0]; Tg[1] = T3[0]; Tg[2] = T3[1]; Tg[3] = T1[0]; Tg[4] = T2[1]; Tg[5] = T3[2]; Tg[6] = T1[1]; Tg[7] = T1[2]; Tg[8] = T2[2];
    As[0] = A2[0]; As[1] = A3[0]; As[2] = A3[1]; As[3] = A1[0]; As[4] = A2[1]; As[5] = A3[2]; As[6] = A1[1]; As[7] = A1[2]; As[8] = A2[2];
    Ma[0] = M2[0]; Ma[1] = 0; Ma[2] = 0; Ma[3] = M1[0]; Ma[4] = M2[1]; Ma[5] = 0; Ma[6] = M1[1]; Ma[7] = M1[2]; Ma[8] = M2[2];
}
// P <- P[idx, idx] (ping-pong)
static lvk_status cov_gather(lvk_ekf* e, const std::vector<int>& idx)
{
    int* h = up_alloc<int>(e, idx.size());
    if (!h) return lvk_set_error(e->ctx, LVK_ERR_CAPACITY, "upload arena exhausted");
    memcpy(h, idx.data(), sizeof(int) * idx.size());
    double* src = e->dP[e->cur]; double* dst = e->dP[e->cur ^ 1];
    const int* d_idx = dev(e, h); const int n = (int)idx.size();
    lvk_status st = run_or_defer(e, [=]() { return lvk_cov_gather(e->ctx, src, e->ld, dst, e->ld, d_idx, n); });
    if (st != LVK_OK) return st;
    e->cur ^= 1; e->N = n;
    return LVK_OK;
}
// P loses the rows / columns marked in drop (N flags)
static lvk_status cov_drop(lvk_ekf* e, const std::vector<char>& drop)
{
    std::vector<int> idx; idx.reserve(e->N);
    for (int i = 0; i < e->N; ++i) if (!drop[i]) idx.push_back(i);
    return cov_gather(e, idx);
}

// ------------------------------------------------------------------------- device job batches: the records and small helpers the stages share
// one triangulation request: its views live in the filter's request pools (tri_ranks / tri_z) at [off, off + n) - no per-request
// vectors (at configs[4] an update issues hundreds of requests)
struct TriReq { Feature* f; int mode; int off, n; long long last_id; bool use_pos; int slot = -1; };   // slot >= 0: the row job that takes the result on the device (lvk_ekf_launch_triangulation)
struct TriAns { bool ok; double position[3], inv_depth, obs_anchor[3]; long long id_anchor; };
static void apply_tri(Feature* f, int mode, const TriAns& a)
{   // feature.hpp:537-546 incl. the FEJ quirk (position_FEJ takes the OLD position of a first-time feature)
    if (!a.ok) return;
    if (!f->is_initialized) memcpy(f->position_fej, f->position, 24);
    f->is_initialized = true;
    memcpy(f->position, a.position, 24);
    f->id_anchor = a.id_anchor;
    f->inv_depth = a.inv_depth; memcpy(f->obs_anchor, a.obs_anchor, 24);
    if (mode == 2) f->ekf_feature = true;
}
static TriAns tri_answer(const lvk_ekf* e, const TriReq& rq, size_t slot)
{   // after a stream sync that covers the batch: d_triout IS the mapped view of h_down
    const TriResult& o = ((const TriResult*)e->h_down)[slot];
    TriAns a; a.ok = o.ok != 0; memcpy(a.position, o.position, 24); a.inv_depth = o.inv_depth; memcpy(a.obs_anchor, o.obs_anchor, 24); a.id_anchor = rq.last_id;
    return a;
}
// One feature-rows job (rows on the device) ------------------------------------------------------------
// the job of an MSCKF feature over the given observations, or over all it has
static RowJob msckf_job(Feature* f, std::vector<long long> sids, int tri = -1)
{
    RowJob r; r.f = f; r.type = JOB_MSCKF; r.want_gate = true; r.dof = 2 * (int)sids.size() - 3; r.tri = tri; r.sids = std::move(sids);
    return r;
}
static RowJob msckf_job(Feature* f, int tri = -1)
{
    std::vector<long long> sids; sids.reserve(f->obs.size()); for (const Obs& o : f->obs) sids.push_back(o.sid);
    return msckf_job(f, std::move(sids), tri);
}
// row layout of a job, known before it runs: MSCKF blocks lose the 3 rows of the null-space projection, a new in-state
// feature's block keeps its range row first, a tracked in-state feature contributes its 2 rows as they are
static int job_first_row(const RowJob& j) { return fj_first_row(j.type); }
static int job_rows(const RowJob& j) { return fj_rows(j.type, (int)j.sids.size()); }
static bool gate_ok(lvk_ekf* e, const RowJob& j)
{
    const bool ok = j.res.gamma < lvk_chi2_005(j.dof);
    e->counters[ok ? 4 : 5]++;
    return ok;
}
static void drop_observations(lvk_ekf* e, const long long* sids, int n) { for (auto kv : e->map) for (int k = 0; k < n; ++k) kv.second.erase(sids[k]); }
// ... and its effect on the host state, when any row passed its gate; counter: 0 feature update, 1 pruning update
static void gated_update_apply(lvk_ekf* e, const std::vector<double>& dx, int accepted, int counter)
{
    if (accepted <= 0) return;
    lvk_ekf_inject(e, dx.data());
    e->last_update_time = e->s.t;
    e->counters[counter]++;
    e->counters[2] = accepted;
}
// What a gated update leaves to the host, after its sync.  The MSCKF jobs [order[0]) in ascending order: a job whose triangulation
// was consumed on the device (RowJob::tri) has its answer read and applied in `mode`, and one whose triangulation failed is not used
// (its rows were zeroed on the device); the others pass through gate_ok and are recorded as MSCKF points.  retire(job, tri_ok) is
// the caller's bookkeeping for each of them.  Then the tracked in-state jobs [order[1]), two rows each.  Returns the accepted rows.
template <class Retire>
static int settle_update(lvk_ekf* e, const std::vector<RowJob>& jobs, const size_t (&order)[2][2], const std::vector<TriReq>& reqs, int mode, Retire retire)
{
    int accepted = 0;
    for (size_t k = order[0][0]; k < order[0][1]; ++k) {
        const RowJob& j = jobs[k];
        bool tri_ok = true;
        if (j.tri >= 0) { const TriAns a = tri_answer(e, reqs[(size_t)j.tri], k); apply_tri(j.f, mode, a); tri_ok = a.ok; }
        if (tri_ok && gate_ok(e, j)) { accepted += job_rows(j); lvk_ekf_msckf_point_record(e, j, k); }
        retire(j, tri_ok);
    }
    for (size_t k = order[1][0]; k < order[1][1]; ++k) if (gate_ok(e, jobs[k])) accepted += 2;
    return accepted;
}
