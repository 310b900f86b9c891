// lvk_larvio.hpp — the C++ host side above the C ABI (include/lvk_c.h): the two classes LARVIO's drivers construct, with the
// reference's method names, argument meaning and error convention (bool returns; "false" from processImage = no message this
// frame), minus OpenCV / Eigen / Boost in the signatures (those libraries are not installed here; INTEGRATION.md shows the
// adapter with the reference's exact signatures for a tree that has them).  Header-only; link with liblvk_hip.so.
//
//   reference                                                   here
//   larvio::ImageProcessor (image_processor.h:36-68)            lvk::ImageProcessor
//   larvio::LarVio (larvio.h:39-90)                             lvk::LarVio
//   ImuData (sensors/ImuData.hpp:17-43)                         lvk::ImuData      (same three fields)
//   ImgData{timeStampToSec, cv::Mat} (sensors/ImageData.hpp)    lvk::ImageData    (plain 8-bit view instead of cv::Mat)
//   MonoFeatureMeasurement / MonoCameraMeasurement              lvk::MonoFeatureMeasurement (= lvk_feature_obs, the same 72-byte record) /
//   (feature_msg.h:15-56)                                       lvk::MonoCameraMeasurement
#ifndef LVK_LARVIO_HPP
#define LVK_LARVIO_HPP
#include "lvk_c.h"
#include "lvk_config.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace lvk {

struct ImuData { double timeStampToSec; double angular_velocity[3]; double linear_acceleration[3]; };
static_assert(sizeof(ImuData) == sizeof(lvk_imu), "ImuData is laid out as lvk_imu");
struct ImageData { double timeStampToSec; const uint8_t* data; int width, height, step; };
typedef lvk_feature_obs MonoFeatureMeasurement;
struct MonoCameraMeasurement { double timeStampToSec; std::vector<MonoFeatureMeasurement> features; };

// one context (= one HIP stream) shared by the two halves unless the caller passes its own
class Context {
public:
    explicit Context(int device = 0) : ctx_(nullptr) { status_ = lvk_context_create(device, &ctx_); }
    ~Context() { if (ctx_) lvk_context_destroy(ctx_); }
    bool ok() const { return status_ == LVK_OK; }
    lvk_context* get() const { return ctx_; }
    const char* error() const { return ctx_ ? lvk_last_error(ctx_) : "no usable gfx950 device (liblvk_hip has no CPU fallback)"; }
private:
    Context(const Context&); Context& operator=(const Context&);
    lvk_context* ctx_; lvk_status status_;
};

class ImageProcessor {
public:
    // the reference's constructor takes the YAML path and loadParameters() reads it (image_processor.cpp:44-113); here the caller
    // hands over the same parameters as a plain struct (field names = YAML keys)
    ImageProcessor(const lvk_fe_config& cfg, lvk_context* ctx) : cfg_(cfg), ctx_(ctx), fe_(nullptr) {}
    // the reference's own constructor (image_processor.cpp:28-33): the configuration file is read by initialize()
    ImageProcessor(const std::string& config_file, lvk_context* ctx) : cfg_(), config_file_(config_file), ctx_(ctx), fe_(nullptr) {}
    ~ImageProcessor() { if (fe_) lvk_frontend_destroy(fe_); }
    bool initialize()                                                                   // image_processor.cpp:116-126
    {
        if (!config_file_.empty()) {                                                    // loadParameters (:44-113)
            ConfigFile f; std::string err;
            if (!f.open(config_file_)) { std::fprintf(stderr, "config_file error: %s\n", f.error().c_str()); return false; }
            if (!load_fe_config(f, &cfg_, &err)) { std::fprintf(stderr, "config_file error: %s\n", err.c_str()); return false; }
        }
        if (!ctx_) { std::fprintf(stderr, "ImageProcessor: no device context\n"); return false; }
        if (lvk_frontend_create(ctx_, &cfg_, &fe_) != LVK_OK) { std::fprintf(stderr, "ImageProcessor: %s\n", lvk_last_error(ctx_)); return false; }
        out_.resize((size_t)cfg_.max_features_num);
        return true;
    }
    // image_processor.cpp:130-219.  true = `features` holds this frame's message.
    bool processImage(const ImageData& msg, const std::vector<ImuData>& imu_msg_buffer, MonoCameraMeasurement* features)
    {
        if (!fe_ || !features) return false;
        int n = 0, has = 0;
        const lvk_imu* imu = imu_msg_buffer.empty() ? nullptr : reinterpret_cast<const lvk_imu*>(imu_msg_buffer.data());
        const lvk_image im = {msg.data, msg.width, msg.height, msg.step, /*is_device=*/0};     // a cv::Mat's own size and step
        if (lvk_frontend_process(fe_, &im, msg.timeStampToSec, imu, (int)imu_msg_buffer.size(),
                                 out_.data(), (int)out_.size(), &n, &has) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::processImage: %s\n", lvk_last_error(ctx_));
            return false;
        }
        if (!has) return false;
        features->timeStampToSec = msg.timeStampToSec;
        features->features.assign(out_.begin(), out_.begin() + n);
        return true;
    }
    // region mask for corner detection (lvk_frontend_set_mask; the reference has no such call): non-zero = corners may be detected
    // there.  With a VioPipeline: before the first processImage or after drain().
    bool setMask(const uint8_t* data, int w, int h, int stride)
    {
        if (!fe_) return false;
        const lvk_image im = {data, w, h, stride, /*is_device=*/0};
        if (lvk_frontend_set_mask(fe_, &im) != LVK_OK) { std::fprintf(stderr, "ImageProcessor::setMask: %s\n", lvk_last_error(ctx_)); return false; }
        return true;
    }
    bool clearMask() { return fe_ && lvk_frontend_set_mask(fe_, nullptr) == LVK_OK; }
    // pixel format of every ImageData from now on (lvk_frontend_set_input_format; the reference's ROS caller converts on the host
    // instead): LVK_PIX_*; msg.data then points at that format's bytes and msg.step is in bytes.  shift: MONO16 only, grey =
    // min(255, v >> shift).  After initialize(); with a VioPipeline before the first processImage or after drain().  false = refused,
    // the previous format stays in force.
    bool setInputFormat(int format, int shift = 0)
    {
        if (!fe_) return false;
        if (lvk_frontend_set_input_format(fe_, format, shift) != LVK_OK) { std::fprintf(stderr, "ImageProcessor::setInputFormat: %s\n", lvk_last_error(ctx_)); return false; }
        return true;
    }
    // where in the last processed frame are these map points (lvk_frontend_match_landmarks; the reference has no such call)?  queries: the
    // predicted pixel and search radius of each, desc: 32 bytes per query; opt may be null (defaults).  out[i].status == LVK_MATCH_OK marks a
    // match, out[i].und is what lvk_landmark_obs takes as uv.  With a VioPipeline only after drain().  false = refused.
    bool matchLandmarks(const std::vector<lvk_match_query>& queries, const std::vector<uint8_t>& desc, std::vector<lvk_landmark_match>& out,
                        const lvk_match_options* opt = nullptr, int* n_candidates = nullptr)
    {
        if (!fe_ || desc.size() != queries.size() * 32) return false;
        out.resize(queries.size());
        if (lvk_frontend_match_landmarks(fe_, queries.data(), desc.data(), (int)queries.size(), opt, out.data(), n_candidates) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::matchLandmarks: %s\n", lvk_last_error(ctx_)); return false;
        }
        return true;
    }
    // the yaw and translation that take a prior map's frame into the filter's world frame (lvk_frontend_align_landmarks; the reference has no
    // such call): matches = (map point, normalised observation) pairs of the last processed frame, many of them possibly wrong; R_wc, p_wc =
    // that frame's camera pose in the filter's world frame; opt may be null (defaults).  out.status == LVK_ALIGN_OK marks success, mask[k]
    // the winner's inliers.  With a VioPipeline only after drain().  false = refused.
    bool alignLandmarks(const std::vector<lvk_align_match>& matches, const double R_wc[9], const double p_wc[3], lvk_align_result& out,
                        std::vector<uint8_t>* mask = nullptr, const lvk_align_options* opt = nullptr, int max_hypotheses = 0, uint32_t seed = 0)
    {
        if (!fe_) return false;
        if (mask) mask->assign(matches.size(), 0);
        if (lvk_frontend_align_landmarks(fe_, matches.data(), (int)matches.size(), R_wc, p_wc, opt, max_hypotheses, seed, &out,
                                         mask && !mask->empty() ? mask->data() : nullptr) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::alignLandmarks: %s\n", lvk_last_error(ctx_)); return false;
        }
        return true;
    }
    // keep a prior map on the device (lvk_frontend_set_map; the reference has no such call): X = 3 doubles per point in the map's own frame,
    // best first - the order is the priority matchMap selects by -, cov9 = 9 doubles per point or empty, desc = 32 bytes per point.  Replaces
    // a previous map, an empty X frees it.  With a VioPipeline only after drain().  false = refused.
    bool setMap(const std::vector<double>& X, const std::vector<double>& cov9, const std::vector<uint8_t>& desc)
    {
        const size_t n = X.size() / 3;
        if (!fe_ || X.size() != 3 * n || desc.size() != 32 * n || (!cov9.empty() && cov9.size() != 9 * n)) return false;
        if (lvk_frontend_set_map(fe_, n ? X.data() : nullptr, cov9.empty() ? nullptr : cov9.data(), n ? desc.data() : nullptr, (int)n) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::setMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        return true;
    }
    // a session's raw exports into the resident map (lvk_frontend_build_map): bad points culled, of near-duplicates the better copy kept,
    // the rest sorted best first and made the map in force as setMap would.  score: empty, or one per point (smaller is better; without
    // it the covariance's trace is the score).  order (may be null): the original indices of the kept points in the map's order.
    bool buildMap(const std::vector<double>& X, const std::vector<double>& cov9, const std::vector<uint8_t>& desc, const std::vector<double>& score = std::vector<double>(),
                  const lvk_map_build_options* opt = nullptr, std::vector<int>* order = nullptr, lvk_map_build_info* info = nullptr)
    {
        const size_t n = X.size() / 3;
        if (!fe_ || X.size() != 3 * n || desc.size() != 32 * n || (!cov9.empty() && cov9.size() != 9 * n) || (!score.empty() && score.size() != n)) return false;
        std::vector<int> ord(n ? n : 1);
        lvk_map_build_info got;
        if (lvk_frontend_build_map(fe_, n ? X.data() : nullptr, cov9.empty() ? nullptr : cov9.data(), n ? desc.data() : nullptr, score.empty() ? nullptr : score.data(), (int)n, opt,
                                   ord.data(), (int)n, &got) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::buildMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        ord.resize((size_t)got.n_kept);
        if (order) order->swap(ord);
        if (info) *info = got;
        return true;
    }
    // the resident map's points in the last processed frame (lvk_frontend_match_map): projected from the pose prediction R_wc, p_wc (align:
    // the map's alignment or null, cov_cam36: the pose covariance [dtheta dp] or null), culled, at most 1024 picked cell by cell and
    // matched.  out[i].index is the map point, out[i].m.status == LVK_MATCH_OK marks a match.  With a VioPipeline only after drain().
    bool matchMap(const double R_wc[9], const double p_wc[3], std::vector<lvk_map_match>& out, const lvk_align_result* align = nullptr,
                  const double* cov_cam36 = nullptr, const lvk_map_select_options* select_opt = nullptr, const lvk_match_options* match_opt = nullptr,
                  lvk_map_info* info = nullptr)
    {
        if (!fe_) return false;
        out.resize(LVK_MAP_MAX_QUERIES);
        int n = 0;
        if (lvk_frontend_match_map(fe_, align, R_wc, p_wc, cov_cam36, select_opt, match_opt, out.data(), (int)out.size(), &n, info) != LVK_OK) {
            out.clear();
            std::fprintf(stderr, "ImageProcessor::matchMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        out.resize((size_t)n);
        return true;
    }
    // the resident map's yaw and translation from the last processed frame in one call, whatever the map's size
    // (lvk_frontend_relocalise_map): the frame's corners searched in the whole map, the best max_matches (0 = 1024) matches into the
    // two-point RANSAC.  R_wc, p_wc = that frame's camera pose in the filter's world frame; the options may be null (ratio_pct 80 is
    // recommended in match_opt).  out.status == LVK_ALIGN_OK marks success; matches[k].inlier the winner's inliers; matchMap takes out as
    // align.  With a VioPipeline only after drain().  false = refused.
    bool relocaliseMap(const double R_wc[9], const double p_wc[3], lvk_align_result& out, std::vector<lvk_reloc_match>* matches = nullptr,
                       const lvk_match_options* match_opt = nullptr, const lvk_align_options* align_opt = nullptr, int max_matches = 0,
                       int max_hypotheses = 0, uint32_t seed = 0, lvk_global_info* info = nullptr)
    {
        if (!fe_) return false;
        std::vector<lvk_reloc_match> m(1024);
        int n = 0;
        if (lvk_frontend_relocalise_map(fe_, R_wc, p_wc, match_opt, align_opt, max_matches, max_hypotheses, seed, &out, m.data(), (int)m.size(), &n, info) != LVK_OK) {
            if (matches) matches->clear();
            std::fprintf(stderr, "ImageProcessor::relocaliseMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        m.resize((size_t)n);
        if (matches) matches->swap(m);
        return true;
    }
    // a second session's exports merged into the resident map (lvk_frontend_merge_map): X, cov9, desc = session B in its own world frame;
    // align = B -> the map's frame (lvk_align_invert turns the alignment of a session that was localised online) or null = find it from
    // the two maps; cov_align16 = the alignment's 4 x 4 covariance or null.  used.status == LVK_ALIGN_OK marks a merge - any other status
    // with a true return means no alignment was found and the map in force stands.  order (may be null): the merged map's points in the
    // caller's view, a value below the old mapSize that resident point, any other the old mapSize + B's original index.  With a
    // VioPipeline only after drain().  false = refused.
    bool mergeMap(const std::vector<double>& X, const std::vector<double>& cov9, const std::vector<uint8_t>& desc, lvk_align_result& used,
                  const lvk_align_result* align = nullptr, const double* cov_align16 = nullptr, const lvk_map_build_options* build_opt = nullptr,
                  const lvk_match_options* match_opt = nullptr, const lvk_align3d_options* align_opt = nullptr, int max_hypotheses = 0, uint32_t seed = 0,
                  std::vector<int>* order = nullptr, lvk_map_build_info* info = nullptr, lvk_global_info* match_info = nullptr)
    {
        const size_t n = X.size() / 3;
        if (!fe_ || X.size() != 3 * n || desc.size() != 32 * n || cov9.size() != 9 * n) return false;
        const int n_a = lvk_frontend_map_size(fe_);
        std::vector<int> ord((size_t)(n_a > 0 ? n_a : 0) + n + 1);
        lvk_map_build_info got;
        if (lvk_frontend_merge_map(fe_, n ? X.data() : nullptr, n ? cov9.data() : nullptr, n ? desc.data() : nullptr, (int)n, align, cov_align16, match_opt, align_opt,
                                   max_hypotheses, seed, build_opt, &used, ord.data(), (int)ord.size(), &got, match_info) != LVK_OK) {
            std::fprintf(stderr, "ImageProcessor::mergeMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        ord.resize((size_t)got.n_kept);
        if (order) order->swap(ord);
        if (info) *info = got;
        return true;
    }
    lvk_frontend* handle() const { return fe_; }
private:
    ImageProcessor(const ImageProcessor&); ImageProcessor& operator=(const ImageProcessor&);
    lvk_fe_config cfg_; std::string config_file_; lvk_context* ctx_; lvk_frontend* fe_;
    std::vector<MonoFeatureMeasurement> out_;
};

class LarVio {
public:
    LarVio(const lvk_ekf_config& cfg, lvk_context* ctx) : cfg_(cfg), ctx_(ctx), ekf_(nullptr), f_state_(nullptr), f_takeoff_(nullptr), takeoff_written_(false) {}
    // the reference's own constructor (larvio.cpp:40-44): initialize() reads the file and opens the two debug logs in output_dir
    LarVio(const std::string& config_file, lvk_context* ctx) : cfg_(), config_file_(config_file), ctx_(ctx), ekf_(nullptr), f_state_(nullptr), f_takeoff_(nullptr), takeoff_written_(false) {}
    ~LarVio() { if (ekf_) lvk_ekf_destroy(ekf_); if (f_state_) std::fclose(f_state_); if (f_takeoff_) std::fclose(f_takeoff_); }   // larvio.cpp:47-55
    bool initialize()                                                                   // larvio.cpp:314-360
    {
        if (!config_file_.empty()) {                                                    // loadParameters (:58-311)
            ConfigFile f; std::string err;
            if (!f.open(config_file_)) { std::fprintf(stderr, "config_file error: %s\n", f.error().c_str()); return false; }
            if (!load_ekf_config(f, &cfg_, &err)) { std::fprintf(stderr, "config_file error: %s\n", err.c_str()); return false; }
            const std::string dir = f.str("output_dir");                               // :220, :318-319; a directory that does not exist => no logs, as with ofstream
            if (!dir.empty()) { f_state_ = std::fopen((dir + "msckf_2_state.txt").c_str(), "w"); f_takeoff_ = std::fopen((dir + "msckf_2_takeoff.txt").c_str(), "w"); }
        }
        if (!ctx_) { std::fprintf(stderr, "LarVio: no device context\n"); return false; }
        if (lvk_ekf_create(ctx_, &cfg_, &ekf_) != LVK_OK) { std::fprintf(stderr, "LarVio: %s\n", lvk_last_error(ctx_)); return false; }
        return true;
    }
    // larvio.cpp:363-461.  Erases the IMU samples it consumed from the caller's vector (:511-512).  true = the filter was updated.
    bool processFeatures(MonoCameraMeasurement* msg, std::vector<ImuData>& imu_msg_buffer)
    {
        if (!ekf_ || !msg) return false;
        int used = 0, updated = 0;
        const lvk_imu* imu = imu_msg_buffer.empty() ? nullptr : reinterpret_cast<const lvk_imu*>(imu_msg_buffer.data());
        if (lvk_ekf_process(ekf_, msg->timeStampToSec, msg->features.empty() ? nullptr : msg->features.data(), (int)msg->features.size(),
                            imu, (int)imu_msg_buffer.size(), &used, &updated) != LVK_OK) {
            std::fprintf(stderr, "LarVio::processFeatures: %s\n", lvk_last_error(ctx_));
            return false;
        }
        imu_msg_buffer.erase(imu_msg_buffer.begin(), imu_msg_buffer.begin() + used);
        if (updated) write_logs();
        return updated != 0;
    }
    // What an update does with an innovation covariance that is not positive definite: LVK_INDEFINITE_FAIL (the default: the update
    // fails and the handle stays failed) or LVK_INDEFINITE_LDLT (that update runs again through the pivoted LDL^T, as the reference's
    // S.ldlt().solve does, and the filter goes on).  After initialize().
    bool setIndefinitePolicy(int policy) { return ekf_ && lvk_ekf_set_indefinite_policy(ekf_, policy) == LVK_OK; }
    // replace the covariance: n x n row-major, n == the state's dimension (lvk_ekf_dim); a prior to start from
    bool setCov(const double* P, int n) { return ekf_ && lvk_ekf_set_cov(ekf_, P, n) == LVK_OK; }
    // getTbw (larvio.cpp:2644-2655): body-to-world pose as a row-major 4x4
    void getTbw(double T[16]) const
    {
        double s[30]; lvk_ekf_get_state(ekf_, s);
        const double x = s[1], y = s[2], z = s[3], w = s[4];                            // stored [x y z w]
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                             2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                             2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j]; T[4 * i + 3] = s[8 + i]; }
        T[12] = T[13] = T[14] = 0; T[15] = 1;
    }
    void getVel(double v[3]) const { double s[30]; lvk_ekf_get_state(ekf_, s); std::memcpy(v, s + 5, 24); }        // :2658-2660
    // getPpose / getPvel (:2663-2700): covariance blocks of (theta, p) and v
    void getPpose(double P66[36]) const
    {
        const int N = 9; double P[81]; if (lvk_ekf_get_cov_imu(ekf_, N, P) != LVK_OK) std::memset(P, 0, sizeof P);
        static const int idx[6] = {0, 1, 2, 6, 7, 8};
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) P66[6 * a + b] = P[(size_t)idx[a] * N + idx[b]];
    }
    void getPvel(double P33[9]) const
    {
        const int N = 9; double P[81]; if (lvk_ekf_get_cov_imu(ekf_, N, P) != LVK_OK) std::memset(P, 0, sizeof P);
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) P33[3 * a + b] = P[(size_t)(3 + a) * N + 3 + b];
    }
    void getSwPoses(std::vector<lvk_clone>& out) const { out.resize(64); out.resize((size_t)lvk_ekf_get_clones(ekf_, out.data(), 64)); }     // :2703-2717
    void getActiveeMapPointPositions(std::vector<int64_t>& ids, std::vector<double>& xyz) const                                          // :2727-2735
    {
        ids.resize(1024); xyz.resize(3 * 1024); std::vector<double> idp(1024);
        const int n = lvk_ekf_get_features(ekf_, ids.data(), idp.data(), xyz.data(), 1024);
        ids.resize((size_t)n); xyz.resize((size_t)3 * n);
    }
    void getStableMapPointPositions(std::vector<int64_t>& ids, std::vector<double>& xyz)                                                 // :2717-2722
    {
        ids.resize(4096); xyz.resize(3 * 4096);
        const int n = lvk_ekf_take_lost_features(ekf_, ids.data(), xyz.data(), 4096);
        ids.resize((size_t)n); xyz.resize((size_t)3 * n);
    }
    // Position covariances of the map points (lvk_ekf_get_feature_cov / lvk_ekf_take_lost_features_cov; conventions in lvk_c.h):
    // cov holds 9 doubles per point, row-major, NaN where the filter has none.  setLostFeatureCov(true), after initialize(), makes
    // the filter compute a lost point's covariance before its column leaves the state.
    bool getFeatureCov(std::vector<int64_t>& ids, std::vector<int64_t>& anchor_ids, std::vector<double>& xyz, std::vector<double>& cov) const
    {
        ids.resize(1024); anchor_ids.resize(1024); xyz.resize(3 * 1024); cov.resize(9 * 1024);
        int n = 0;
        const bool ok = ekf_ && lvk_ekf_get_feature_cov(ekf_, ids.data(), anchor_ids.data(), xyz.data(), cov.data(), 1024, &n) == LVK_OK;
        if (!ok) n = 0;
        ids.resize((size_t)n); anchor_ids.resize((size_t)n); xyz.resize((size_t)3 * n); cov.resize((size_t)9 * n);
        return ok;
    }
    // The same map points in the camera frame of a pose of the window (lvk_ekf_get_feature_rel; conventions in lvk_c.h): xyz_c holds
    // 3 doubles per point, cov 9 (row-major; cov[9 k + 8] is the depth variance), NaN where the anchor clone has left the window.
    // to_clone_id -1: the current IMU state; otherwise a clone id of getSwPoses' window - false when it is not there.
    bool getFeaturesInCamera(std::vector<int64_t>& ids, std::vector<int64_t>& anchor_ids, std::vector<double>& xyz_c, std::vector<double>& cov, int64_t to_clone_id = -1) const
    {
        ids.resize(4096); anchor_ids.resize(4096); xyz_c.resize(3 * 4096); cov.resize(9 * 4096);
        int n = 0;
        const bool ok = ekf_ && lvk_ekf_get_feature_rel(ekf_, to_clone_id, ids.data(), anchor_ids.data(), xyz_c.data(), cov.data(), 4096, &n) == LVK_OK;
        if (!ok) n = 0;
        ids.resize((size_t)n); anchor_ids.resize((size_t)n); xyz_c.resize((size_t)3 * n); cov.resize((size_t)9 * n);
        return ok;
    }
    bool setLostFeatureCov(bool on) { return ekf_ && lvk_ekf_set_lost_feature_cov(ekf_, on ? 1 : 0) == LVK_OK; }
    void takeLostFeaturesCov(std::vector<int64_t>& ids, std::vector<double>& xyz, std::vector<double>& cov)
    {
        ids.resize(4096); xyz.resize(3 * 4096); cov.resize(9 * 4096);
        const int n = lvk_ekf_take_lost_features_cov(ekf_, ids.data(), xyz.data(), cov.data(), 4096);
        ids.resize((size_t)n); xyz.resize((size_t)3 * n); cov.resize((size_t)9 * n);
    }
    // The MSCKF points (lvk_ekf_set_msckf_points / lvk_ekf_take_msckf_points; conventions in lvk_c.h): setMsckfPoints(true), after
    // initialize(), makes every lost-feature update keep the features it triangulated, accepted and erased, each with its 3 x 3
    // position covariance (9 doubles, row-major) and observation count; takeMsckfPoints hands out up to 4096 of them per call.
    bool setMsckfPoints(bool on) { return ekf_ && lvk_ekf_set_msckf_points(ekf_, on ? 1 : 0) == LVK_OK; }
    void takeMsckfPoints(std::vector<int64_t>& ids, std::vector<double>& xyz, std::vector<double>& cov, std::vector<int>& n_obs)
    {
        ids.resize(4096); xyz.resize(3 * 4096); cov.resize(9 * 4096); n_obs.resize(4096);
        const int n = ekf_ ? lvk_ekf_take_msckf_points(ekf_, ids.data(), xyz.data(), cov.data(), n_obs.data(), 4096) : 0;
        ids.resize((size_t)n); xyz.resize((size_t)3 * n); cov.resize((size_t)9 * n); n_obs.resize((size_t)n);
    }
    // The keyframe export (lvk_ekf_set_keyframe_export / lvk_ekf_take_keyframes / lvk_ekf_get_window_cov; conventions in lvk_c.h):
    // setKeyframeExport(true), after initialize(), makes the pruning keep every clone it removes as an lvk_keyframe - pose, absolute
    // 6 x 6 covariance and the covariance of its pose relative to the nearest newer surviving clone; takeKeyframes hands out up to 1024
    // of them per call.  getWindowCov: the clones still in the window - ids, 36 doubles of absolute block each and 36 of Sigma_rel to
    // the next clone (NaN for the last).
    bool setKeyframeExport(bool on) { return ekf_ && lvk_ekf_set_keyframe_export(ekf_, on ? 1 : 0) == LVK_OK; }
    void takeKeyframes(std::vector<lvk_keyframe>& out)
    {
        out.resize(1024);
        const int n = ekf_ ? lvk_ekf_take_keyframes(ekf_, out.data(), 1024) : 0;
        out.resize((size_t)n);
    }
    bool getWindowCov(std::vector<int64_t>& ids, std::vector<double>& cov_abs, std::vector<double>& cov_rel) const
    {
        ids.resize(256); cov_abs.resize(36 * 256); cov_rel.resize(36 * 256);
        int n = 0;
        const bool ok = ekf_ && lvk_ekf_get_window_cov(ekf_, ids.data(), cov_abs.data(), cov_rel.data(), 256, &n) == LVK_OK;
        if (!ok) n = 0;
        ids.resize((size_t)n); cov_abs.resize((size_t)36 * n); cov_rel.resize((size_t)36 * n);
        return ok;
    }
    // External fixes (lvk_ekf_add_fix / lvk_ekf_set_fix_options / lvk_ekf_take_fix_reports; models, target clone, gate and refusals in
    // lvk_c.h): addFix queues a position or pose fix, expressed in the filter's world frame, on a clone of the window - by id or by
    // time - and the next processFeatures that holds the clone applies it; takeFixReports hands out what became of each (up to 256
    // per call).  With a VioPipeline call addFix only between drain() and the next processImage.
    bool addFix(const lvk_fix& fix) { return ekf_ && lvk_ekf_add_fix(ekf_, &fix) == LVK_OK; }
    bool setFixOptions(double gate_scale, double max_gap_s) { return ekf_ && lvk_ekf_set_fix_options(ekf_, gate_scale, max_gap_s) == LVK_OK; }
    void takeFixReports(std::vector<lvk_fix_report>& out)
    {
        out.resize(256);
        const int n = ekf_ ? lvk_ekf_take_fix_reports(ekf_, out.data(), 256) : 0;
        out.resize((size_t)n);
    }
    // Observations of known landmarks (lvk_ekf_add_landmark_obs / lvk_ekf_set_landmark_options / lvk_ekf_take_landmark_reports; the
    // measurement model, target clone, gate and refusals in lvk_c.h): addLandmarkObs queues the observations made in ONE image of
    // points whose position in the filter's world frame is known, on a clone of the window - by id or (clone_id -1) by time - and the
    // next processFeatures that holds the clone applies them; takeLandmarkReports hands out what became of each batch (up to 64 per
    // call).  With a VioPipeline call addLandmarkObs only between drain() and the next processImage.
    bool addLandmarkObs(long long tag, long long clone_id, double time, const std::vector<lvk_landmark_obs>& obs)
    {
        return ekf_ && lvk_ekf_add_landmark_obs(ekf_, tag, clone_id, time, obs.data(), (int)obs.size()) == LVK_OK;
    }
    bool setLandmarkOptions(double gate_scale, double min_depth) { return ekf_ && lvk_ekf_set_landmark_options(ekf_, gate_scale, min_depth) == LVK_OK; }
    void takeLandmarkReports(std::vector<lvk_landmark_report>& out)
    {
        out.resize(64);
        const int n = ekf_ ? lvk_ekf_take_landmark_reports(ekf_, out.data(), 64) : 0;
        out.resize((size_t)n);
    }
    void landmarkStats(long out12[12]) const { for (int i = 0; i < 12; ++i) out12[i] = 0; if (ekf_) lvk_ekf_landmark_stats(ekf_, out12); }
    // Localise in the loop (lvk_vio_localise_map; steps, target clone and refusals in lvk_c.h): from this filter's pose of the frame `fe`
    // processed last to ONE queued batch of observations of fe's resident map (ImageProcessor::setMap / buildMap) - the clone's camera
    // pose and covariance, matchMap's device chain, the gather of the matched points, addLandmarkObs, without a host copy of the map.
    // The clone goes by id, or (clone_id -1) by time.  info.status == LVK_LOCALISE_NO_CLONE: the filter has no clone for that frame,
    // nothing was queued.  With a VioPipeline call it only between drain() and the next processImage.
    bool localiseMap(ImageProcessor& fe, lvk_localise_info& info, const lvk_align_result* align = nullptr, long long clone_id = -1, double time = 0.0,
                     double sigma_px = 1.0, const lvk_map_select_options* select_opt = nullptr, const lvk_match_options* match_opt = nullptr, long long tag = 0)
    {
        if (!ekf_ || !fe.handle()) return false;
        if (lvk_vio_localise_map(fe.handle(), ekf_, align, clone_id, time, sigma_px, select_opt, match_opt, tag, &info) != LVK_OK) {
            std::fprintf(stderr, "LarVio::localiseMap: %s\n", lvk_last_error(ctx_)); return false;
        }
        return true;
    }
    lvk_ekf* handle() const { return ekf_; }
private:
    friend class VioPipeline;
    LarVio(const LarVio&); LarVio& operator=(const LarVio&);
    // the debug logs of larvio.cpp:388 and :446-453: take-off stamp once; then per update
    //   t-take_off  qw qx qy qz  vx vy vz  px py pz  bgx bgy bgz  bax bay baz  qbc(w x y z)  t_cam0_imu      ("%g" = the ostream default)
    void write_logs()
    {
        if (!f_state_ && !f_takeoff_) return;
        double s[30]; lvk_ekf_get_state(ekf_, s);
        const double t0 = lvk_ekf_take_off_stamp(ekf_);
        if (f_takeoff_ && !takeoff_written_) { std::fprintf(f_takeoff_, "%.9f\n", t0); std::fflush(f_takeoff_); takeoff_written_ = true; }
        if (!f_state_) return;
        double qbc[4]; rot_to_quat_wxyz(s + 17, qbc);
        std::fprintf(f_state_, "%g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g\n", s[0] - t0, s[4], s[1], s[2], s[3],
                     s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15], s[16], qbc[0], qbc[1], qbc[2], qbc[3], s[26], s[27], s[28]);
    }
    // Eigen::Quaterniond(Matrix3d) (larvio.cpp:436): Shepperd's branch on the trace, w >= 0 in the first branch only
    static void rot_to_quat_wxyz(const double* R, double q[4])
    {
        const double t = R[0] + R[4] + R[8];
        if (t > 0) {
            double r = std::sqrt(t + 1.0); q[0] = 0.5 * r; r = 0.5 / r;
            q[1] = (R[7] - R[5]) * r; q[2] = (R[2] - R[6]) * r; q[3] = (R[3] - R[1]) * r;
        } else {
            int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[4 * i]) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            double r = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
            q[1 + i] = 0.5 * r; r = 0.5 / r;
            q[0] = (R[3 * k + j] - R[3 * j + k]) * r; q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * r; q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * r;
        }
    }
    lvk_ekf_config cfg_; std::string config_file_; lvk_context* ctx_; lvk_ekf* ekf_;
    FILE* f_state_; FILE* f_takeoff_; bool takeoff_written_;
};

// The driver loop with the filter update of message k overlapping the front-end of the following frames (lvk_vio_pipe_*): same
// results as calling processImage / processFeatures in turn, but processFeatures' answer arrives through a callback on the filter's
// thread — the place to publish odometry.  The two halves must have been created on DIFFERENT Contexts (= HIP streams).
//     pipe.pushImu(...)            samples with t < t_img + 0.05, as larvioMain.cpp:98-102 fills imu_msg_buffer
//     pipe.processImage(img)       true = this frame produced a feature message (its update runs in the background)
//     pipe.drain()                 wait for the updates in flight before reading the estimator
class VioPipeline {
public:
    typedef void (*OdometryFn)(void* user, double ts, const LarVio& estimator);
    VioPipeline(ImageProcessor& fe, LarVio& be) : be_(be), pipe_(nullptr), fn_(nullptr), user_(nullptr)
    {
        if (lvk_vio_pipe_create(fe.handle(), be.handle(), &pipe_) != LVK_OK) pipe_ = nullptr;
        else lvk_vio_pipe_on_update(pipe_, &VioPipeline::trampoline, this);
    }
    ~VioPipeline() { if (pipe_) lvk_vio_pipe_destroy(pipe_); }
    bool ok() const { return pipe_ != nullptr; }
    void onOdometry(OdometryFn fn, void* user) { drain(); fn_ = fn; user_ = user; }
    bool pushImu(const ImuData* v, size_t n) { return pipe_ && lvk_vio_pipe_push_imu(pipe_, reinterpret_cast<const lvk_imu*>(v), (int)n) == LVK_OK; }
    bool processImage(const ImageData& msg)
    {
        int has = 0;
        const lvk_image im = {msg.data, msg.width, msg.height, msg.step, /*is_device=*/0};
        if (!pipe_ || lvk_vio_pipe_submit(pipe_, &im, msg.timeStampToSec, &has) != LVK_OK) return false;
        return has != 0;
    }
    bool drain(long* n_updates = nullptr, long* n_msgs = nullptr) { return pipe_ && lvk_vio_pipe_drain(pipe_, n_updates, n_msgs) == LVK_OK; }
    // erase counts submit() took early / how many of them the filter's thread found different (expected 0; lvk_c.h)
    bool earlyCounts(long* n_early, long* n_wrong) { return pipe_ && lvk_vio_pipe_early_counts(pipe_, n_early, n_wrong) == LVK_OK; }
    lvk_vio_pipe* handle() const { return pipe_; }
private:
    VioPipeline(const VioPipeline&); VioPipeline& operator=(const VioPipeline&);
    static void trampoline(void* self, double ts, const double*)
    {
        VioPipeline* p = static_cast<VioPipeline*>(self);
        p->be_.write_logs();                                      // the reference's state log, as processFeatures writes it
        if (p->fn_) p->fn_(p->user_, ts, p->be_);
    }
    LarVio& be_; lvk_vio_pipe* pipe_; OdometryFn fn_; void* user_;
};

}  // namespace lvk
#endif
