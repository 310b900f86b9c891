// be_host.h — what the back-end's translation units call in one another (host side): the records they pass by value and the
// prototype of every lvk_* function that one be_*.hip / backend.hip defines and another calls.  Definers include it as well, so
// the compiler checks each definition against the prototype its callers see.  (The structure-aware compression has be_qr.h; the
// filter object itself, which backend.hip shares with the exports of be_export.hip and the pipelined driver of be_pipe.hip, has
// be_filter.h.  backend.hip runs one message through the stages declared at the end of this file and defines the one phase tracer
// they all mark (g_tr, be_filter.h); no function of backend.o is called from another object - the pipelined driver reaches the
// update through lvk_ekf::process.)
#pragma once
#include "lvk_internal.h"
#include "be_dev.h"
#include <vector>

// Workspace of one measurement update, passed by value.  B: m x (n+1), S: m x m.  info: the factorisation's report words, in DEVICE
// memory (the final GEMM reads them: GemmRider::gate); info_host: their mirror in device-mapped host memory, written only when one
// is set; ev_*: optional bracket around the update's first launch (H P, with S's partial planes where lvk_update_fused_s); dx_host: host-mapped mirror of dx; p00_host: of the updated P's leading
// 16 x 16 block
struct UpdateWs { double* B; int ldb; double* S; int lds; int* info; hipEvent_t ev_a = nullptr, ev_b = nullptr; double* dx_host = nullptr; double* p00_host = nullptr; int* info_host = nullptr; };
// sharded update: rank g's jobs [job_lo, job_lo + job_n) and its k compressed rows, stacked from row_off (host writes, k_shard_unpack reads)
// LVK_SHARD_HDR, the bytes of the header every rank's block starts with, is part of the wire layout: include/lvk_c.h
struct ShardMeta { int job_lo, job_n, k, row_off; };

// Staging of a stage-level entry (host buffers in, launchers, host buffers out): up to three device blobs in the context's shared
// stage slots - IN (what the host composes and uploads in one copy, through the mirror this owns), MID (device-only work space), OUT
// (results; may be pre-filled from the caller's memory) - each laid out as regions aligned to 256 bytes.  Usage: take() every region,
// alloc(), fill host(), upload(), launch on at(), get() the results, wait().  The destructor waits for the stream too, so that no exit,
// failing or not, leaves an asynchronous copy behind that names the mirror or a caller's buffer.
struct Stage {
    enum { IN, MID, OUT };
    lvk_context* ctx; size_t bytes[3] = {0, 0, 0}; char* dev[3] = {nullptr, nullptr, nullptr}; std::vector<char> mirror; bool waited = false;
    explicit Stage(lvk_context* c) : ctx(c) {}
    Stage(const Stage&) = delete;
    ~Stage() { if (!waited) (void)hipStreamSynchronize(ctx->stream); }
    size_t take(int blob, size_t n) { const size_t at = bytes[blob]; bytes[blob] = (at + (n ? n : 1) + 255) & ~(size_t)255; return at; }      // offset of a new region (never empty: its pointer stays valid)
    lvk_status alloc()
    {
        const int slot[3] = {LVK_SCR_STAGE_IN, LVK_SCR_STAGE_MID, LVK_SCR_STAGE_OUT};
        for (int b = 0; b < 3; ++b)
            if (bytes[b] && !(dev[b] = (char*)lvk_ctx_scratch(ctx, slot[b], bytes[b]))) return lvk_set_error(ctx, LVK_ERR_DEVICE, "scratch allocation failed");
        mirror.assign(bytes[IN], 0);
        return LVK_OK;
    }
    template <class T> T* host(size_t off) { return (T*)(mirror.data() + off); }                    // a region of IN, in the mirror
    template <class T> T* at(int blob, size_t off) const { return (T*)(dev[blob] + off); }          // a region, on the device
    lvk_status upload() { return put(IN, 0, mirror.data(), bytes[IN]); }
    lvk_status put(int blob, size_t off, const void* h, size_t n)                                   // host memory that outlives the call -> region
    {
        if (n) LVK_HIP(ctx, hipMemcpyAsync(dev[blob] + off, h, n, hipMemcpyHostToDevice, ctx->stream));
        return LVK_OK;
    }
    lvk_status get(void* h, int blob, size_t off, size_t n)                                         // region -> host memory, queued
    {
        if (n) LVK_HIP(ctx, hipMemcpyAsync(h, dev[blob] + off, n, hipMemcpyDeviceToHost, ctx->stream));
        return LVK_OK;
    }
    lvk_status wait() { waited = true; LVK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return LVK_OK; }
};
// `call` returns lvk_status: pass a failure on
#define LVK_TRY(call) do { const lvk_status st_ = (call); if (st_ != LVK_OK) return st_; } while (0)

// be_linalg.hip
lvk_status lvk_stage_copy2(lvk_context* ctx, void* d_dst0, const void* d_src0, size_t bytes0, void* d_dst1, const void* d_src1, size_t bytes1);
lvk_status lvk_update_core(lvk_context* ctx, double* P, int ldp, int n, const double* H, int ldh, int m, const double* r, double sigma2, double* dx, UpdateWs ws);
bool lvk_update_fused_s(int m);                           // lvk_update_core forms S inside the H P launch for this m
double lvk_update_first_launch_flops(int m, int n);       // flops of what lvk_update_core brackets with UpdateWs::ev_a / ev_b
lvk_status lvk_update_ldlt_core(lvk_context* ctx, double* P, int ldp, int n, const double* H, int ldh, int m, const double* r, double sigma2, double* dx, UpdateWs ws, int** d_cnt_out, int** d_perm_out);
lvk_status lvk_cov_gather(lvk_context* ctx, const double* Pin, int ldin, double* Pout, int ldout, const int* d_idx, int n);
lvk_status lvk_cov_propagate_augment(lvk_context* ctx, const double* Pin, int ldin, double* Pout, int ldout, int n_out, int pose_rows, int L,
                                     const double* h_phi, const double* h_q, const double* d_phiq);
lvk_status lvk_cov_reanchor(lvk_context* ctx, double* P, int ld, int n, const double* d_J, int fc);
lvk_status lvk_cov_append_features(lvk_context* ctx, double* P, int ld, int n, int nn, const double* H1, int ldh, const double* H2, const double* r1,
                                   const double* dx, double sigma2, double* tmp, double* dx_new);
// be_ldlt.hip
size_t lvk_ldlt_lds_bytes(int m);
lvk_status lvk_ldlt_factor_solve(lvk_context* ctx, double* S, int ld, int m, const double* B, int ldb, int nbcols, double* Bp, double* X, double* Dg, int* perm, int* cnt);
void lvk_cov_symmetrize(lvk_context* ctx, double* P, int ld, int n);
// be_landmark.hip
bool lvk_landmark_job_ok(const lvk_landmark_job* j, int n);
lvk_status lvk_launch_landmark_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_landmark_job* d_jobs, int n_jobs, double* d_cov9);
// be_landmark_rel.hip
bool lvk_landmark_rel_job_ok(const lvk_landmark_rel_job* j, int n);
lvk_status lvk_launch_landmark_rel_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_landmark_rel_job* d_jobs, int n_jobs, double* d_out12);
// be_pose_rel.hip
bool lvk_pose_rel_job_ok(const lvk_pose_rel_job* j, int n);
lvk_status lvk_launch_pose_rel_cov(lvk_context* ctx, const double* d_P, int ldp, const lvk_pose_rel_job* d_jobs, int n_jobs, double* d_cov36);
// be_msckf_point.hip
lvk_status lvk_launch_msckf_point_cov(lvk_context* ctx, const double* d_P, int ldp, const PointJob* d_jobs, int n_jobs, const CloneDev* d_clones, const int* d_rank,
                                      const double* d_z, const double* d_zv, FilterFlags fl, const TriResult* d_tri, double* d_cov9, int* d_ok);
// be_feature.hip
int lvk_feature_rows_route(int max_rows, int gate_rows_max);
lvk_status lvk_launch_triangulate(lvk_context* ctx, const TriJob* d_jobs, int n_jobs, const CamPose* d_cams, const int* d_rank, const double* d_z, TriResult* d_out, TriResult* d_out_dev);
lvk_status lvk_launch_feature_rows(lvk_context* ctx, const FeatJob* d_jobs, int n_jobs, int max_rows, const CloneDev* d_clones, const int* d_rank,
                                   const double* d_z, const double* d_zv, const double* d_P, int ldp, FilterFlags fl, double* d_staging, int* d_ccols, FeatResult* d_out, FeatResult* d_out_host,
                                   double* d_Hout, int ldh, int ncols_out, double* d_rout, int obs_stride, int n_clones, const TriResult* d_tri);
lvk_status lvk_launch_stack_rows(lvk_context* ctx, const FeatResult* d_fout, const StackRow* d_map, int n_rows, const double* d_staging, const int* d_ccols, double* d_H, int ldh, int ncols, double* d_r);
// be_qr.hip, be_qr_dense.hip
double lvk_chi2_005(int dof);
lvk_status lvk_qr_compress_dev(lvk_context* ctx, double* d_H, int ldh, int rows, int cols, double* d_r, int* rows_out);
// be_shard.hip
lvk_status lvk_shard_pack(lvk_context* ctx, const FeatResult* d_res, int n_res, const double* d_X, int ld, const double* d_rX, int k, int ncols, char* d_send, size_t res_bytes, int rank);
lvk_status lvk_shard_unpack(lvk_context* ctx, const char* d_recv, size_t bytes_per_rank, size_t res_bytes, const ShardMeta* d_meta, int world, int ncols, int k_max,
                            FeatResult* d_fout, FeatResult* d_fout_host, double* d_H, int ld, double* d_r, int* d_peer_fail);
// be_export.hip: the drain lists' launches (queued before the columns they read leave P) and their read-back (be_filter.h has the records)
struct RowJob; struct RowObs;
lvk_status lvk_ekf_lost_cov_queue(lvk_ekf* e, const std::vector<long long>& ekf_lost);
lvk_status lvk_ekf_keyframes_queue(lvk_ekf* e, const long long* rm, int nrm);
lvk_status lvk_ekf_exports_attach(lvk_ekf* e);
lvk_status lvk_ekf_msckf_points_queue(lvk_ekf* e, const std::vector<RowJob>& jobs, size_t lo, size_t hi, const RowObs& obs);
void lvk_ekf_msckf_point_record(lvk_ekf* e, const RowJob& j, size_t k);
// The stages of one message (backend.hip's ekf_process_impl runs them; be_filter.h has their records)
// be_initialize.hip
bool lvk_ekf_static_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased);
bool lvk_ekf_dynamic_try_init(lvk_ekf* e, double ts, const lvk_feature_obs* f, int n, const lvk_imu* imu, int n_imu, int* n_erased);
// be_propagate.hip
int lvk_ekf_batch_imu(lvk_ekf* e, double time_bound, const lvk_imu* imu, int n_imu);
lvk_status lvk_ekf_state_augmentation(lvk_ekf* e);
void lvk_ekf_add_observations(lvk_ekf* e, const lvk_feature_obs* f, int n);
void lvk_ekf_inject(lvk_ekf* e, const double* dx);
// be_triangulate.hip
struct Feature; struct TriReq; struct TriAns;
lvk_status lvk_ekf_upload_clones(lvk_ekf* e);
void lvk_ekf_make_tri_req(lvk_ekf* e, Feature* f, int mode, TriReq* rq);
lvk_status lvk_ekf_launch_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs);
lvk_status lvk_ekf_run_triangulation(lvk_ekf* e, std::vector<TriReq>& reqs, std::vector<TriAns>& ans);
bool lvk_ekf_check_motion(const lvk_ekf* e, const Feature& f, bool if_tracked);
// be_update.hip
struct RowGroup;
lvk_status lvk_ekf_d2h_sync(lvk_ekf* e, void* dst, const void* src, size_t bytes);
lvk_status lvk_ekf_dense_update(lvk_ekf* e, int m, std::vector<double>& dx, int extra, const std::vector<RowGroup>* groups = nullptr);
lvk_status lvk_ekf_gated_update(lvk_ekf* e, std::vector<RowJob>& jobs, const size_t (&order)[2][2], const int (&tr)[3], std::vector<double>& dx,
                                const long long* retire = nullptr, int n_retire = 0, size_t mp_lo = 0, size_t mp_hi = 0);
lvk_status lvk_ekf_remove_lost_features(lvk_ekf* e);
// be_fix.hip
lvk_status lvk_ekf_apply_fixes(lvk_ekf* e);
// be_landmark_fix.hip
lvk_status lvk_ekf_apply_landmarks(lvk_ekf* e);
// be_prune.hip
lvk_status lvk_ekf_check_zupt(lvk_ekf* e, bool* out);
lvk_status lvk_ekf_prune_imu_state_buffer(lvk_ekf* e);
