// adapter/adapter_main.cpp — the loop of the reference's app/larvioMain.cpp:84-117 written against the ADAPTER classes
// (larvio::ImageProcessor / larvio::LarVio with the reference's own signatures), i.e. what larvioMain.cpp does once it is linked
// against lvk_adapter instead of the image_processor / estimator libraries, minus the Pangolin viewer (:57-82,118-202).
// Usage: adapter_main path_to_imu/data.csv path_to_cam0/data.csv path_to_cam0/data config_file_path [--tum traj.txt] [--bench N [--no-vis]] [--depth-out FILE]
// --depth-out FILE: after every odometry message, LarVio::getFeaturesInCamera and one line per active map point in the format of
// examples/larvio_euroc --depth-out (examples/lvk_euroc_args.hpp), stamped with the image's time.
// --bench N: the image files are decoded before the loop starts (the reference's player reads them inside it; a PNG decode is ten times
// a frame of this library) and the LAST N frames of the loop - processImage, processFeatures, every getter of larvioMain.cpp:117-170 -
// are timed with the steady clock; one line "bench frames N seconds S frames_per_s F" is printed (bench.py: adapter_cpp).  --no-vis
// leaves out getVisualImg (the viewer's picture: a device-to-host copy and a drawing pass per odometry message).
// --input-format NAME[:SHIFT] (bgr8 rgb8 bgra8 rgba8 mono16 yuyv uyvy): ImageProcessor::setInputFormat, and every decoded grey frame is
// handed over as a cv::Mat of that format whose grey IS the frame - (g, g, g[, 7]), g << SHIFT, (g, 128) / (128, g) - so that the run
// must print what the default run prints.
// The library's runtime settings (lvk_runtime_env: hardware queues, kernel arguments) need no call here: lvk_context_create applies
// them, and the adapter's initialize() is this process's first HIP call - larvioMain.cpp itself links unchanged.
#include <larvio/image_processor.h>
#include <larvio/larvio.h>

#include "../examples/lvk_dataset.hpp"
#include "../examples/lvk_euroc_args.hpp"
#include "../examples/lvk_png.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

using namespace larvio;

// a grey frame as a cv::Mat of pixel format `format` (LVK_PIX_*) whose conversion gives the frame back
static cv::Mat grey_as(const lvk::GreyImage& g, int format, int shift)
{
    if (format == LVK_PIX_MONO8) return cv::Mat(g.height, g.width, CV_8UC1, const_cast<unsigned char*>(g.data.data())).clone();
    const int type = format == LVK_PIX_BGR8 || format == LVK_PIX_RGB8 ? CV_8UC3 : format == LVK_PIX_BGRA8 || format == LVK_PIX_RGBA8 ? CV_8UC4 : format == LVK_PIX_MONO16 ? CV_16UC1 : CV_8UC2;
    cv::Mat m(g.height, g.width, type);
    for (int y = 0; y < g.height; ++y) {
        const unsigned char* s = g.data.data() + (size_t)y * g.width; unsigned char* d = m.ptr(y);
        for (int x = 0; x < g.width; ++x) {
            switch (format) {
            case LVK_PIX_BGR8: case LVK_PIX_RGB8: d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = s[x]; break;
            case LVK_PIX_BGRA8: case LVK_PIX_RGBA8: d[4 * x] = d[4 * x + 1] = d[4 * x + 2] = s[x]; d[4 * x + 3] = 7; break;
            case LVK_PIX_MONO16: { const unsigned short v = (unsigned short)(s[x] << shift); std::memcpy(d + 2 * x, &v, 2); break; }
            case LVK_PIX_YUYV: d[2 * x] = s[x]; d[2 * x + 1] = 128; break;
            default: d[2 * x] = 128; d[2 * x + 1] = s[x]; break;
            }
        }
    }
    return m;
}

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "Usage: %s path_to_imu/data.csv path_to_cam0/data.csv path_to_cam0/data config_file_path [--tum traj.txt]\n", argv[0]); return 1; }
    std::string tum_path, depth_path; long bench_n = 0; bool vis_on = true; int pix_format = LVK_PIX_MONO8, pix_shift = 0;
    for (int a = 5; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--tum") && a + 1 < argc) tum_path = argv[++a];
        else if (!std::strcmp(argv[a], "--depth-out") && a + 1 < argc) depth_path = argv[++a];
        else if (!std::strcmp(argv[a], "--bench") && a + 1 < argc) bench_n = std::atol(argv[++a]);
        else if (!std::strcmp(argv[a], "--no-vis")) vis_on = false;
        else if (!std::strcmp(argv[a], "--input-format") && a + 1 < argc) {
            static const char* const names[] = {"mono8", "bgr8", "rgb8", "bgra8", "rgba8", "mono16", "yuyv", "uyvy"};
            std::string v = argv[++a]; const size_t colon = v.find(':');
            if (colon != std::string::npos) { pix_shift = std::atoi(v.c_str() + colon + 1); v.resize(colon); }
            pix_format = -1;
            for (int f = 0; f < 8; ++f) if (v == names[f]) pix_format = f;
            if (pix_format < 0) { std::fprintf(stderr, "--input-format: unknown format %s\n", v.c_str()); return 1; }
        }
    }
    std::vector<lvk::ImuData> imu_rows; std::vector<lvk::ImgInfo> allImgInfo;
    if (!lvk::loadImuFile(argv[1], imu_rows) || !lvk::loadImageList(argv[2], allImgInfo)) { std::fprintf(stderr, "cannot read the sensor files\n"); return 1; }
    std::vector<ImuData> allImuData;
    for (const auto& m : imu_rows) allImuData.push_back(ImuData(m.timeStampToSec, m.angular_velocity[0], m.angular_velocity[1], m.angular_velocity[2],
                                                                m.linear_acceleration[0], m.linear_acceleration[1], m.linear_acceleration[2]));
    std::string config_file(argv[4]);

    ImageProcessorPtr ImgProcesser;                                   // larvioMain.cpp:42-48
    ImgProcesser.reset(new ImageProcessor(config_file));
    if (!ImgProcesser->initialize()) { std::fprintf(stderr, "Image Processer initialization failed!\n"); return 1; }
    if (pix_format != LVK_PIX_MONO8 && !ImgProcesser->setInputFormat(pix_format, pix_shift)) { std::fprintf(stderr, "the input format was refused\n"); return 1; }
    LarVioPtr Estimator;                                              // :50-55
    Estimator.reset(new LarVio(config_file));
    if (!Estimator->initialize()) { std::fprintf(stderr, "Estimator initialization failed!\n"); return 1; }

    FILE* tum = tum_path.empty() ? nullptr : std::fopen(tum_path.c_str(), "w");
    FILE* depth = depth_path.empty() ? nullptr : std::fopen(depth_path.c_str(), "w");
    if (!depth_path.empty() && !depth) { std::perror(depth_path.c_str()); return 1; }
    size_t k = 0; long n_msgs = 0, n_odo = 0, n_stable = 0, n_active = 0;
    std::vector<ImuData> imu_msg_buffer;
    std::vector<lvk::GreyImage> preloaded;
    if (bench_n > 0) {
        preloaded.resize(allImgInfo.size());
        for (size_t j = 0; j < allImgInfo.size(); ++j) { std::string err; if (!lvk::read_png_grey(std::string(argv[3]) + "/" + allImgInfo[j].imgName, &preloaded[j], &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; } }
        if ((size_t)bench_n > allImgInfo.size()) bench_n = (long)allImgInfo.size();
    }
    std::chrono::steady_clock::time_point t_bench;
    for (size_t j = 0; j < allImgInfo.size(); ++j) {
        if (bench_n > 0 && j + (size_t)bench_n == allImgInfo.size()) { (void)Estimator->getTbw(); t_bench = std::chrono::steady_clock::now(); }   // the getter waits for a deferred update: the timed part starts with an idle filter
        lvk::GreyImage image_file; std::string err;
        if (bench_n <= 0 && !lvk::read_png_grey(std::string(argv[3]) + "/" + allImgInfo[j].imgName, &image_file, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        lvk::GreyImage& image = bench_n > 0 ? preloaded[j] : image_file;
        ImageDataPtr imgPtr(new ImgData);                             // :88-95
        imgPtr->timeStampToSec = allImgInfo[j].timeStampToSec;
        imgPtr->image = grey_as(image, pix_format, pix_shift);
        while (k < allImuData.size() && allImuData[k].timeStampToSec - imgPtr->timeStampToSec < 0.05) imu_msg_buffer.push_back(allImuData[k++]);   // :98-103
        MonoCameraMeasurementPtr features = new MonoCameraMeasurement;                                                  // :105
        const bool bProcess = ImgProcesser->processImage(imgPtr, imu_msg_buffer, features);                             // :107
        bool bPubOdo = false;
        if (bProcess) { ++n_msgs; bPubOdo = Estimator->processFeatures(features, imu_msg_buffer); }                     // :114
        delete features;
        if (bPubOdo) {                                                                                                  // :117-170, without the viewer
            ++n_odo;
            const Eigen::Isometry3d T_b_w = Estimator->getTbw();
            const Eigen::Vector3d vel = Estimator->getVel();
            const Eigen::Matrix<double, 6, 6> P_pose = Estimator->getPpose();
            const Eigen::Matrix3d P_vel = Estimator->getPvel();
            std::vector<Eigen::Isometry3d> swPoses; Estimator->getSwPoses(swPoses);
            std::map<FeatureIDType, Eigen::Vector3d> stable, active;
            Estimator->getStableMapPointPositions(stable); Estimator->getActiveeMapPointPositions(active);
            n_stable += (long)stable.size(); n_active = (long)active.size();
            const cv::Mat vis = vis_on ? ImgProcesser->getVisualImg() : cv::Mat();
            if (tum) std::fprintf(tum, "%.9f %.17g %.17g %.17g  %.17g %.17g %.17g  %.6e %.6e  %zu %d\n", imgPtr->timeStampToSec, T_b_w.translation()(0), T_b_w.translation()(1),
                                  T_b_w.translation()(2), vel(0), vel(1), vel(2), P_pose(0, 0), P_vel(0, 0), swPoses.size(), vis.cols * vis.rows * vis.channels());
            if (depth) {
                std::vector<FeatureIDType> ids; std::vector<Eigen::Vector3d> pos_c; std::vector<double> cov9;
                if (!Estimator->getFeaturesInCamera(ids, pos_c, cov9)) { std::fprintf(stderr, "getFeaturesInCamera failed\n"); return 1; }
                for (size_t i = 0; i < ids.size(); ++i) {
                    const double p[3] = {pos_c[i](0), pos_c[i](1), pos_c[i](2)};
                    lvk::write_depth_point(depth, imgPtr->timeStampToSec, (long long)ids[i], p, &cov9[9 * i]);
                }
            }
        }
    }
    if (bench_n > 0) {
        (void)Estimator->getTbw();                                    // the last deferred update is part of the timed work
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_bench).count();
        std::printf("bench frames %ld seconds %.6f frames_per_s %.1f\n", bench_n, sec, (double)bench_n / sec);
    }
    if (tum) std::fclose(tum);
    if (depth) std::fclose(depth);
    std::printf("frames %zu  feature messages %ld  odometry updates %ld  stable map points handed out %ld  active at the end %ld\n", allImgInfo.size(), n_msgs, n_odo, n_stable, n_active);
    return 0;
}
