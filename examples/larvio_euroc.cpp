// larvio_euroc.cpp — the headless form of the reference's dataset driver (/root/reference/app/larvioMain.cpp:27-117, minus
// Pangolin): same command line, same loop, same log files (msckf_2_state.txt / msckf_2_takeoff.txt in the configuration's
// output_dir, written by lvk::LarVio as larvio.cpp:388,446-453 does), running on liblvk_hip.so.
//
//   larvio_euroc path_to_imu/data.csv path_to_cam0/data.csv path_to_cam0/data config_file_path [--tum traj.txt] [--max-frames N] [--pipelined] [--mask FILE.png] [--map-out FILE] [--msckf-out FILE] [--keyframes-out FILE] [--depth-out FILE] [--fixes FILE] [--fix-max-gap S] [--landmarks FILE]
//
// --mask restricts corner detection to the non-zero pixels of an 8-bit PNG of the configured resolution (ImageProcessor::setMask:
// a fisheye vignette, the vehicle's own body); a mask of another size is an error.
// --map-out turns the filter's lost-point covariances on (LarVio::setLostFeatureCov) and writes, at the end of the run, one line per
// stable map point: "id x y z sxx sxy sxz syy syz szz" - its last world position and the upper triangle of its 3 x 3 position covariance.
// --msckf-out turns the filter's MSCKF-point export on (LarVio::setMsckfPoints) and writes one line per point the lost-feature updates
// triangulated, accepted and erased: "id x y z" + the nine entries of its 3 x 3 position covariance, row-major + its observation count.
// The list is drained after every update; --pipelined drains it once, at the end (the filter keeps the newest 65536 points).
// --keyframes-out turns the filter's keyframe export on (LarVio::setKeyframeExport) and writes one line per clone the pruning removed:
// "id to_id time to_time q(4) p(3) rel_q(4) rel_p(3) cov_abs(36) cov_rel(36)" - its pose, the pose of clone to_id relative to it, its
// absolute 6 x 6 covariance and the covariance of that relative pose (lvk_c.h, lvk_ekf_pose_rel_cov).  Drained after every update;
// --pipelined drains once, at the end.
// --depth-out writes, after every pose, one line per in-state feature: "timestamp id x y z s00 s01 s02 s11 s12 s22" - the point in the
// camera frame of that pose and the upper triangle of its 3 x 3 covariance there (LarVio::getFeaturesInCamera; lvk_c.h,
// lvk_ekf_landmark_rel_cov): s22 is the depth variance.  A getter only: the filter's outputs do not notice it.
// --fixes reads external position / pose fixes (LarVio::addFix; lvk_c.h, lvk_ekf_add_fix) from a csv file with the columns
// "time,kind,px,py,pz,qx,qy,qz,qw,sigma_p,sigma_theta[,lx,ly,lz]" (kind 0 position / 1 pose; time on the IMU clock, ascending; the fix
// in the FILTER's world frame - aligning another frame is the caller's job; lines that do not parse are skipped) and queues each line
// before the first frame whose stamp reaches its time; the filter applies it on the clone with exactly that time, or - with
// --fix-max-gap S - between two adjacent clones at most S seconds apart.  A last line "fixes queued .. applied .." reports the outcome.
// Not with --pipelined (the pipeline takes fixes only between a drain and the next frame).
// --tum writes "t x y z qx qy qz qw" (body in world, absolute stamps, 17 significant digits) for tools/traj_rmse.py.
// --pipelined runs the same loop through lvk::VioPipeline: the filter update of a message overlaps the front-end of the next
// frames on a second HIP stream; the trajectory is the same, written from the filter thread's odometry callback.
// The filter starts with the static initializer (StaticInitializer.cpp); the dynamic (SfM) initializer is outside the hot path.
#include "lvk_dataset.hpp"
#include "lvk_euroc_args.hpp"
#include "lvk_png.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static void write_tum(FILE* tum, const lvk::LarVio& Estimator)
{
    double s[30]; lvk_ekf_get_state(Estimator.handle(), s);                                        // q stored [x y z w]; p = s[8..10]
    std::fprintf(tum, "%.9f %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", s[0], s[8], s[9], s[10], s[1], s[2], s[3], s[4]);
}

// --map-out: the stable points collected so far (the filter hands each one out once)
struct MapOut {
    FILE* f; long n;
    void drain(lvk::LarVio& Estimator)
    {
        if (!f) return;
        std::vector<int64_t> ids; std::vector<double> xyz, cov;
        do {
            Estimator.takeLostFeaturesCov(ids, xyz, cov);
            for (size_t i = 0; i < ids.size(); ++i, ++n) {
                const double* p = &xyz[3 * i]; const double* c = &cov[9 * i];
                std::fprintf(f, "%lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)ids[i], p[0], p[1], p[2], c[0], c[1], c[2], c[4], c[5], c[8]);
            }
        } while (!ids.empty());
    }
    void close() { if (f) { std::fclose(f); f = nullptr; } }
};

// --msckf-out: the MSCKF points collected so far (drained after every update, so the filter's list stays short)
struct MsckfOut {
    FILE* f; long n;
    void drain(lvk::LarVio& Estimator)
    {
        if (!f) return;
        std::vector<int64_t> ids; std::vector<double> xyz, cov; std::vector<int> n_obs;
        do {
            Estimator.takeMsckfPoints(ids, xyz, cov, n_obs);
            for (size_t i = 0; i < ids.size(); ++i, ++n) lvk::write_msckf_point(f, (long long)ids[i], &xyz[3 * i], &cov[9 * i], n_obs[i]);
        } while (!ids.empty());
    }
    void close() { if (f) { std::fclose(f); f = nullptr; } }
};

// --keyframes-out: the pruned clones collected so far (drained after every update)
struct KeyframesOut {
    FILE* f; long n;
    void drain(lvk::LarVio& Estimator)
    {
        if (!f) return;
        std::vector<lvk_keyframe> kf;
        do {
            Estimator.takeKeyframes(kf);
            for (size_t i = 0; i < kf.size(); ++i, ++n) lvk::write_keyframe(f, (long long)kf[i].id, (long long)kf[i].to_id, &kf[i].time);
        } while (!kf.empty());
    }
    void close() { if (f) { std::fclose(f); f = nullptr; } }
};

// --depth-out: the in-state features in the camera frame of the pose just published
struct DepthOut {
    FILE* f; long n;
    void write(const lvk::LarVio& Estimator)
    {
        if (!f) return;
        std::vector<int64_t> ids, anchors; std::vector<double> xyz, cov;
        double s[30];
        if (lvk_ekf_get_state(Estimator.handle(), s) != LVK_OK || !Estimator.getFeaturesInCamera(ids, anchors, xyz, cov)) return;
        for (size_t i = 0; i < ids.size(); ++i, ++n) lvk::write_depth_point(f, s[0], (long long)ids[i], &xyz[3 * i], &cov[9 * i]);
    }
    void close() { if (f) { std::fclose(f); f = nullptr; } }
};

// --landmarks reads image observations of points whose position in the filter's world frame is known (LarVio::addLandmarkObs; lvk_c.h,
// lvk_ekf_add_landmark_obs) from a csv file with the columns "time,px,py,pz,u,v,sigma[,sigma_w]" (time on the IMU clock, ascending;
// u, v normalised).  Consecutive lines with equal time form one batch, queued by time before the first frame whose stamp reaches it.  A
// last line "landmarks batches .. applied .." reports the outcome.  Not with --pipelined, as --fixes.
struct Landmarks {
    lvk::LandmarkFile file; size_t next; long refused;
    void queue_up_to(lvk::LarVio& Estimator, double stamp)
    {
        for (; next < file.batches() && file.rows[8 * file.first[next]] <= stamp; ++next) {
            std::vector<lvk_landmark_obs> obs;
            for (size_t k = file.first[next]; k < file.first[next + 1]; ++k) {
                const double* v = &file.rows[8 * k];
                lvk_landmark_obs o = lvk_landmark_obs();
                for (int i = 0; i < 3; ++i) { o.p_w[i] = v[1 + i]; o.cov_w[4 * i] = v[7] * v[7]; }
                o.uv[0] = v[4]; o.uv[1] = v[5]; o.sigma = v[6];
                obs.push_back(o);
            }
            if (!Estimator.addLandmarkObs((long long)next, -1, file.rows[8 * file.first[next]], obs)) ++refused;
        }
    }
};
// --fixes: the file's lines in order; next = the first one not queued yet
struct Fixes {
    std::vector<lvk_fix> all; size_t next; long refused;
    bool load(const std::string& path)
    {
        FILE* f = std::fopen(path.c_str(), "r");
        if (!f) return false;
        char line[1024];
        while (std::fgets(line, sizeof line, f)) {
            double v[14];
            if (!lvk::parse_fix_line(line, v)) continue;
            lvk_fix x = lvk_fix();
            x.tag = (int64_t)all.size(); x.kind = (int)v[1]; x.clone_id = -1; x.time = v[0];
            for (int i = 0; i < 3; ++i) { x.p[i] = v[2 + i]; x.lever[i] = v[11 + i]; }
            for (int i = 0; i < 4; ++i) x.q[i] = v[5 + i];
            if (x.kind == LVK_FIX_POSE) for (int i = 0; i < 3; ++i) { x.cov[7 * i] = v[10] * v[10]; x.cov[7 * (3 + i)] = v[9] * v[9]; }
            else for (int i = 0; i < 3; ++i) x.cov[7 * i] = v[9] * v[9];
            all.push_back(x);
        }
        std::fclose(f);
        return true;
    }
    void queue_up_to(lvk::LarVio& Estimator, double stamp) { for (; next < all.size() && all[next].time <= stamp; ++next) if (!Estimator.addFix(all[next])) ++refused; }
};

struct OdometrySink { FILE* tum; long n_odo; DepthOut* depth; };
static void on_odometry(void* user, double, const lvk::LarVio& Estimator)
{
    OdometrySink* o = static_cast<OdometrySink*>(user);
    ++o->n_odo;
    if (o->tum) write_tum(o->tum, Estimator);
    o->depth->write(Estimator);
}

static int run_pipelined(const char* image_dir, const std::vector<lvk::ImuData>& allImuData, const std::vector<lvk::ImgInfo>& allImgInfo, long max_frames,
                         lvk::ImageProcessor& ImgProcesser, lvk::LarVio& Estimator, FILE* tum, MapOut& map_out, MsckfOut& msckf_out, KeyframesOut& kf_out,
                         DepthOut& depth_out)
{
    typedef std::chrono::steady_clock Clock;
    lvk::VioPipeline pipe(ImgProcesser, Estimator);
    if (!pipe.ok()) { std::fprintf(stderr, "cannot create the pipeline\n"); return 1; }
    OdometrySink sink = {tum, 0, &depth_out};
    pipe.onOdometry(on_odometry, &sink);
    const size_t n_frames = max_frames >= 0 && (size_t)max_frames < allImgInfo.size() ? (size_t)max_frames : allImgInfo.size();
    size_t k = 0; double t_proc = 0, t_io = 0; long n_msgs = 0, n_upd = 0;
    for (size_t j = 0; j < n_frames; ++j) {
        const Clock::time_point t0 = Clock::now();
        const std::string fullPath = std::string(image_dir) + "/" + allImgInfo[j].imgName;
        lvk::GreyImage image; std::string err;
        if (!lvk::read_png_grey(fullPath, &image, &err)) { std::fprintf(stderr, "%s: %s\n", fullPath.c_str(), err.c_str()); return 1; }
        const double ts = allImgInfo[j].timeStampToSec;
        const size_t k0 = k;
        while (k < allImuData.size() && allImuData[k].timeStampToSec - ts < 0.05) ++k;
        const Clock::time_point t1 = Clock::now();
        if (k > k0) pipe.pushImu(&allImuData[k0], k - k0);
        lvk::ImageData msg = {ts, image.data.data(), image.width, image.height, image.width};
        pipe.processImage(msg);
        t_io += std::chrono::duration<double>(t1 - t0).count();
        t_proc += std::chrono::duration<double>(Clock::now() - t1).count();
    }
    const Clock::time_point t2 = Clock::now();
    if (!pipe.drain(&n_upd, &n_msgs)) { std::fprintf(stderr, "pipeline: %s\n", "an update failed"); return 1; }
    t_proc += std::chrono::duration<double>(Clock::now() - t2).count();
    if (tum) std::fclose(tum);
    map_out.drain(Estimator); map_out.close();
    msckf_out.drain(Estimator); msckf_out.close();
    kf_out.drain(Estimator); kf_out.close();
    depth_out.close();
    std::printf("frames %zu  feature messages %ld  odometry updates %ld  state dim %d\n", n_frames, n_msgs, sink.n_odo, lvk_ekf_dim(Estimator.handle()));
    std::printf("pipelined: %.3f ms/frame in the driver thread   image read+decode %.3f ms/frame\n", n_frames ? 1e3 * t_proc / n_frames : 0.0, n_frames ? 1e3 * t_io / n_frames : 0.0);
    if (t_proc > 0) std::printf("processing rate %.1f frames/s (pipelined, host buffers)\n", n_frames / t_proc);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "Usage: %s path_to_imu/data.csv path_to_cam0/data.csv path_to_cam0/data config_file_path [--tum traj.txt] [--max-frames N] [--pipelined] [--mask FILE.png] [--map-out FILE] [--msckf-out FILE] [--keyframes-out FILE] [--depth-out FILE] [--fixes FILE] [--fix-max-gap S] [--landmarks FILE]\n", argv[0]);
        return 1;
    }
    lvk::EurocArgs opt; std::string bad;
    if (!lvk::parse_euroc_args(argc, argv, 5, &opt, &bad)) { std::fprintf(stderr, "unknown option %s\n", bad.c_str()); return 1; }
    const std::string &tum_path = opt.tum, &mask_path = opt.mask, &map_path = opt.map_out; const long max_frames = opt.max_frames; const bool pipelined = opt.pipelined;

    // Read sensors (larvioMain.cpp:33-37)
    std::vector<lvk::ImuData> allImuData; std::vector<lvk::ImgInfo> allImgInfo;
    if (!lvk::loadImuFile(argv[1], allImuData) || allImuData.empty()) { std::fprintf(stderr, "cannot read IMU samples from %s\n", argv[1]); return 1; }
    if (!lvk::loadImageList(argv[2], allImgInfo) || allImgInfo.empty()) { std::fprintf(stderr, "cannot read the image list %s\n", argv[2]); return 1; }
    const std::string config_file(argv[4]);
    // the mask is checked against the configuration before any device is touched
    lvk::GreyImage mask;
    if (!mask_path.empty()) {
        std::string err; lvk::ConfigFile f; lvk_fe_config fcfg = lvk_fe_config();
        if (!lvk::read_png_grey(mask_path, &mask, &err)) { std::fprintf(stderr, "%s: %s\n", mask_path.c_str(), err.c_str()); return 1; }
        if (!f.open(config_file)) { std::fprintf(stderr, "config_file error: %s\n", f.error().c_str()); return 1; }
        if (!lvk::load_fe_config(f, &fcfg, &err)) { std::fprintf(stderr, "config_file error: %s\n", err.c_str()); return 1; }
        if (mask.width != fcfg.width || mask.height != fcfg.height) {
            std::fprintf(stderr, "%s: the mask is %dx%d, the configuration says %dx%d\n", mask_path.c_str(), mask.width, mask.height, fcfg.width, fcfg.height);
            return 1;
        }
    }

    lvk::Context ctx(0);
    if (!ctx.ok()) { std::fprintf(stderr, "larvio_euroc: %s\n", ctx.error()); return 3; }
    lvk::ImageProcessor ImgProcesser(config_file, ctx.get());                                      // :42-48
    if (!ImgProcesser.initialize()) { std::fprintf(stderr, "Image Processer initialization failed!\n"); return 1; }
    if (!mask_path.empty() && !ImgProcesser.setMask(mask.data.data(), mask.width, mask.height, mask.width)) return 1;
    lvk::Context ctx2(0);                                                                           // the filter's own stream when pipelined
    if (pipelined && !ctx2.ok()) { std::fprintf(stderr, "larvio_euroc: %s\n", ctx2.error()); return 3; }
    lvk::LarVio Estimator(config_file, pipelined ? ctx2.get() : ctx.get());                         // :50-56
    if (!Estimator.initialize()) { std::fprintf(stderr, "Estimator initialization failed!\n"); return 1; }

    FILE* tum = nullptr;
    if (!tum_path.empty() && !(tum = std::fopen(tum_path.c_str(), "w"))) { std::perror(tum_path.c_str()); return 1; }
    MapOut map_out = {nullptr, 0};
    if (!map_path.empty()) {
        if (!(map_out.f = std::fopen(map_path.c_str(), "w"))) { std::perror(map_path.c_str()); return 1; }
        if (!Estimator.setLostFeatureCov(true)) { std::fprintf(stderr, "larvio_euroc: %s\n", ctx.error()); return 1; }
    }
    MsckfOut msckf_out = {nullptr, 0};
    if (!opt.msckf_out.empty()) {
        if (!(msckf_out.f = std::fopen(opt.msckf_out.c_str(), "w"))) { std::perror(opt.msckf_out.c_str()); return 1; }
        if (!Estimator.setMsckfPoints(true)) { std::fprintf(stderr, "larvio_euroc: %s\n", (pipelined ? ctx2 : ctx).error()); return 1; }
    }
    KeyframesOut kf_out = {nullptr, 0};
    if (!opt.keyframes_out.empty()) {
        if (!(kf_out.f = std::fopen(opt.keyframes_out.c_str(), "w"))) { std::perror(opt.keyframes_out.c_str()); return 1; }
        if (!Estimator.setKeyframeExport(true)) { std::fprintf(stderr, "larvio_euroc: %s\n", (pipelined ? ctx2 : ctx).error()); return 1; }
    }
    DepthOut depth_out = {nullptr, 0};
    if (!opt.depth_out.empty() && !(depth_out.f = std::fopen(opt.depth_out.c_str(), "w"))) { std::perror(opt.depth_out.c_str()); return 1; }
    Landmarks landmarks = {lvk::LandmarkFile(), 0, 0};
    if (!opt.landmarks.empty()) {
        if (pipelined) { std::fprintf(stderr, "larvio_euroc: --landmarks is not available with --pipelined\n"); return 1; }
        if (!landmarks.file.load(opt.landmarks)) { std::perror(opt.landmarks.c_str()); return 1; }
    }
    Fixes fixes = {std::vector<lvk_fix>(), 0, 0};
    if (!opt.fixes.empty()) {
        if (pipelined) { std::fprintf(stderr, "larvio_euroc: --fixes is not available with --pipelined\n"); return 1; }
        if (!fixes.load(opt.fixes)) { std::perror(opt.fixes.c_str()); return 1; }
        if (!Estimator.setFixOptions(1.0, opt.fix_max_gap)) { std::fprintf(stderr, "larvio_euroc: %s\n", ctx.error()); return 1; }
    }
    if (pipelined) return run_pipelined(argv[3], allImuData, allImgInfo, max_frames, ImgProcesser, Estimator, tum, map_out, msckf_out, kf_out, depth_out);

    typedef std::chrono::steady_clock Clock;
    double t_fe = 0, t_be = 0, t_io = 0; long n_fe = 0, n_be = 0, n_odo = 0;
    size_t k = 0;
    std::vector<lvk::ImuData> imu_msg_buffer;
    const size_t n_frames = max_frames >= 0 && (size_t)max_frames < allImgInfo.size() ? (size_t)max_frames : allImgInfo.size();
    for (size_t j = 0; j < n_frames; ++j) {
        // get img (:88-95)
        const Clock::time_point t0 = Clock::now();
        const std::string fullPath = std::string(argv[3]) + "/" + allImgInfo[j].imgName;
        lvk::GreyImage image; std::string err;
        if (!lvk::read_png_grey(fullPath, &image, &err)) { std::fprintf(stderr, "%s: %s\n", fullPath.c_str(), err.c_str()); return 1; }
        const double ts = allImgInfo[j].timeStampToSec;
        // get imus (:98-103): everything up to 0.05 s past the image
        while (k < allImuData.size() && allImuData[k].timeStampToSec - ts < 0.05) imu_msg_buffer.push_back(allImuData[k++]);
        const Clock::time_point t1 = Clock::now();

        // process (:106-116)
        lvk::ImageData msg = {ts, image.data.data(), image.width, image.height, image.width};
        lvk::MonoCameraMeasurement features;
        const bool bProcess = ImgProcesser.processImage(msg, imu_msg_buffer, &features);
        const Clock::time_point t2 = Clock::now();
        bool bPubOdo = false;
        fixes.queue_up_to(Estimator, ts);
        landmarks.queue_up_to(Estimator, ts);
        if (bProcess) bPubOdo = Estimator.processFeatures(&features, imu_msg_buffer);
        const Clock::time_point t3 = Clock::now();
        t_io += std::chrono::duration<double>(t1 - t0).count();
        t_fe += std::chrono::duration<double>(t2 - t1).count(); ++n_fe;
        if (bProcess) { t_be += std::chrono::duration<double>(t3 - t2).count(); ++n_be; }
        if (bPubOdo) {
            ++n_odo;
            if (tum) write_tum(tum, Estimator);
            depth_out.write(Estimator);
        }
        msckf_out.drain(Estimator);
        kf_out.drain(Estimator);
    }
    if (tum) std::fclose(tum);
    map_out.drain(Estimator); map_out.close();
    msckf_out.drain(Estimator); msckf_out.close();
    kf_out.drain(Estimator); kf_out.close();
    depth_out.close();
    std::printf("frames %ld  feature messages %ld  odometry updates %ld  state dim %d\n", n_fe, n_be, n_odo, lvk_ekf_dim(Estimator.handle()));
    std::printf("front-end %.3f ms/frame   back-end %.3f ms/message   image read+decode %.3f ms/frame\n", n_fe ? 1e3 * t_fe / n_fe : 0.0,
                n_be ? 1e3 * t_be / n_be : 0.0, n_fe ? 1e3 * t_io / n_fe : 0.0);
    if (t_fe + t_be > 0) std::printf("processing rate %.1f frames/s (front-end + back-end, sequential, host buffers)\n", n_fe / (t_fe + t_be));
    if (!opt.landmarks.empty()) {
        long st[12]; Estimator.landmarkStats(st);
        std::printf("landmarks batches %zu refused %ld queued %ld applied %ld all_rejected %ld not_pd %ld stale %ld no_clone %ld waiting %ld obs %ld used %ld gated %ld behind %ld\n",
                    landmarks.file.batches(), landmarks.refused, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10]);
    }
    if (!opt.fixes.empty()) {
        long st[8]; lvk_ekf_fix_stats(Estimator.handle(), st);
        std::printf("fixes read %zu refused %ld queued %ld applied %ld gated %ld not_pd %ld stale %ld no_clone %ld waiting %ld interpolated %ld\n", fixes.all.size(), fixes.refused,
                    st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]);
    }
    return 0;
}
