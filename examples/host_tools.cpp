// host_tools.cpp — exposes the host-only helpers of the dataset driver (configuration reader, PNG reader, CSV readers) on the
// command line so that tests/test_host_tools.py can check them on a machine without a GPU.  Not linked against liblvk_hip.so.
//   host_tools config <file.yaml>          the two C-ABI configuration structs, one "name value" line per field
//   host_tools png <in.png> <out.raw>      prints "width height", writes the 8-bit grey pixels
//   host_tools imu <data.csv>              one "%.17g x7" line per sample
//   host_tools images <data.csv>           one "stamp name" line per image
//   host_tools euroc-args [options...]     the dataset driver's options as it parses them, one "name value" line each (exit 1 + the
//                                          driver's message on an unknown option)
//   host_tools euroc-args-all [options...] the same with every field (euroc-args keeps the six lines it has always printed)
//   host_tools euroc-args-fields <f1,f2,...> [options...]   the fields named (tum mask map_out msckf_out keyframes_out depth_out max_frames
//                                          pipelined), in that order: a new option needs no listing of its own (the two above keep their lines)
//   host_tools depth-line <stamp> <id> <x y z> <9 covariance entries, row-major>      the --depth-out line of that point
//   host_tools keyframe-line <id> <to_id> <88 doubles: time to_time q p rel_q rel_p cov_abs cov_rel>      the --keyframes-out line of that record
//   host_tools msckf-line <id> <x y z> <9 covariance entries, row-major> <n_obs>      the --msckf-out line of that point
#include "lvk_config.hpp"
#include "lvk_dataset.hpp"
#include "lvk_euroc_args.hpp"
#include "lvk_png.hpp"
#include <cstdio>
#include <cstring>
#include <string>

static void show(const char* name, double v) { std::printf("%s %.17g\n", name, v); }
static void show(const char* name, const double* v, int n) { std::printf("%s", name); for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]); std::printf("\n"); }

int main(int argc, char** argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "config")) {
        lvk::ConfigFile f;
        if (!f.open(argv[2])) { std::fprintf(stderr, "config_file error: %s\n", f.error().c_str()); return 1; }
        lvk_fe_config a; lvk_ekf_config b; std::string err;
        if (!lvk::load_fe_config(f, &a, &err) || !lvk::load_ekf_config(f, &b, &err)) { std::fprintf(stderr, "config_file error: %s\n", err.c_str()); return 1; }
        std::printf("output_dir %s\n", f.str("output_dir").c_str());
#define FE(x) show("fe." #x, (double)a.x)
        FE(width); FE(height); FE(pyramid_levels); FE(patch_size); FE(max_iteration); FE(track_precision); FE(max_features_num);
        FE(min_distance); FE(flag_equalize); FE(pub_frequency); FE(distortion_model);
        show("fe.intrinsics", a.intrinsics, 4); show("fe.distortion", a.distortion, 4); show("fe.R_cam_imu", a.R_cam_imu, 9);
#define BE(x) show("ekf." #x, (double)b.x)
        BE(if_fej); BE(estimate_extrin); BE(estimate_td); BE(if_zupt_valid); BE(sw_size); BE(max_track_len); BE(least_observation_number);
        BE(max_features_in_one_grid); BE(aug_grid_rows); BE(aug_grid_cols); BE(pub_frequency); BE(imu_rate); BE(width); BE(height);
        show("ekf.intrinsics", b.intrinsics, 4); show("ekf.T_cam_imu", b.T_cam_imu, 16);
        BE(td); BE(noise_gyro); BE(noise_acc); BE(noise_gyro_bias); BE(noise_acc_bias); BE(noise_feature);
        BE(initial_covariance_orientation); BE(initial_covariance_velocity); BE(initial_covariance_position); BE(initial_covariance_gyro_bias);
        BE(initial_covariance_acc_bias); BE(initial_covariance_extrin_rot); BE(initial_covariance_extrin_trans);
        BE(rotation_threshold); BE(translation_threshold); BE(tracking_rate_threshold); BE(feature_translation_threshold);
        BE(zupt_max_feature_dis); BE(zupt_noise_v); BE(zupt_noise_p); BE(zupt_noise_q); BE(static_duration);
        BE(feature_idp_dim); BE(use_schmidt); BE(calib_imu_instrinsic); BE(max_features); BE(legacy_grid); BE(reserved0);
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "png")) {
        lvk::GreyImage img; std::string err;
        if (!lvk::read_png_grey(argv[2], &img, &err)) { std::fprintf(stderr, "%s: %s\n", argv[2], err.c_str()); return 1; }
        FILE* o = std::fopen(argv[3], "wb"); if (!o) { std::perror(argv[3]); return 1; }
        std::fwrite(img.data.data(), 1, img.data.size(), o); std::fclose(o);
        std::printf("%d %d\n", img.width, img.height);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "imu")) {
        std::vector<lvk::ImuData> v;
        if (!lvk::loadImuFile(argv[2], v)) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        for (size_t i = 0; i < v.size(); ++i)
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", v[i].timeStampToSec, v[i].angular_velocity[0], v[i].angular_velocity[1],
                        v[i].angular_velocity[2], v[i].linear_acceleration[0], v[i].linear_acceleration[1], v[i].linear_acceleration[2]);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "images")) {
        std::vector<lvk::ImgInfo> v;
        if (!lvk::loadImageList(argv[2], v)) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        for (size_t i = 0; i < v.size(); ++i) std::printf("%.17g %s\n", v[i].timeStampToSec, v[i].imgName.c_str());
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "euroc-args")) {
        lvk::EurocArgs o; std::string bad;
        if (!lvk::parse_euroc_args(argc, argv, 2, &o, &bad)) { std::fprintf(stderr, "unknown option %s\n", bad.c_str()); return 1; }
        std::printf("tum %s\nmask %s\nmap_out %s\nmsckf_out %s\nmax_frames %ld\npipelined %d\n", o.tum.c_str(), o.mask.c_str(), o.map_out.c_str(), o.msckf_out.c_str(),
                    o.max_frames, o.pipelined ? 1 : 0);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "euroc-args-all")) {
        lvk::EurocArgs o; std::string bad;
        if (!lvk::parse_euroc_args(argc, argv, 2, &o, &bad)) { std::fprintf(stderr, "unknown option %s\n", bad.c_str()); return 1; }
        std::printf("tum %s\nmask %s\nmap_out %s\nmsckf_out %s\nkeyframes_out %s\nmax_frames %ld\npipelined %d\n", o.tum.c_str(), o.mask.c_str(), o.map_out.c_str(),
                    o.msckf_out.c_str(), o.keyframes_out.c_str(), o.max_frames, o.pipelined ? 1 : 0);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "euroc-args-fields")) {
        lvk::EurocArgs o; std::string bad;
        if (!lvk::parse_euroc_args(argc, argv, 3, &o, &bad)) { std::fprintf(stderr, "unknown option %s\n", bad.c_str()); return 1; }
        const struct { const char* name; std::string value; } all[] = {{"tum", o.tum}, {"mask", o.mask}, {"map_out", o.map_out}, {"msckf_out", o.msckf_out},
            {"keyframes_out", o.keyframes_out}, {"depth_out", o.depth_out}, {"fixes", o.fixes}, {"fix_max_gap", std::to_string(o.fix_max_gap)}, {"landmarks", o.landmarks}, {"max_frames", std::to_string(o.max_frames)}, {"pipelined", o.pipelined ? "1" : "0"}};
        const std::string want = argv[2];
        for (size_t lo = 0; lo <= want.size();) {
            size_t hi = want.find(',', lo); if (hi == std::string::npos) hi = want.size();
            const std::string name = want.substr(lo, hi - lo); bool found = false;
            for (const auto& f : all) if (name == f.name) { std::printf("%s %s\n", f.name, f.value.c_str()); found = true; }
            if (!found) { std::fprintf(stderr, "unknown field %s\n", name.c_str()); return 2; }
            lo = hi + 1;
        }
        return 0;
    }
    if (argc == 16 && !std::strcmp(argv[1], "depth-line")) {
        double v[12]; for (int i = 0; i < 12; ++i) v[i] = std::strtod(argv[4 + i], nullptr);
        lvk::write_depth_point(stdout, std::strtod(argv[2], nullptr), std::atoll(argv[3]), v, v + 3);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "fix-line")) {
        double v[14];
        if (!lvk::parse_fix_line(argv[2], v)) { std::printf("no fix\n"); return 0; }
        for (int i = 0; i < 14; ++i) std::printf("%.17g%c", v[i], i == 13 ? '\n' : ' ');
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "landmark-batches")) {      // "batch b time t n k" per batch, then every line's 8 numbers
        lvk::LandmarkFile lf;
        if (!lf.load(argv[2])) { std::perror(argv[2]); return 1; }
        for (size_t b = 0; b < lf.batches(); ++b) {
            std::printf("batch %zu time %.17g n %zu\n", b, lf.rows[8 * lf.first[b]], lf.first[b + 1] - lf.first[b]);
            for (size_t k = lf.first[b]; k < lf.first[b + 1]; ++k) for (int i = 0; i < 8; ++i) std::printf("%.17g%c", lf.rows[8 * k + i], i == 7 ? '\n' : ' ');
        }
        return 0;
    }
    if (argc == 92 && !std::strcmp(argv[1], "keyframe-line")) {
        double v[88]; for (int i = 0; i < 88; ++i) v[i] = std::strtod(argv[4 + i], nullptr);
        lvk::write_keyframe(stdout, std::atoll(argv[2]), std::atoll(argv[3]), v);
        return 0;
    }
    if (argc == 16 && !std::strcmp(argv[1], "msckf-line")) {
        double v[12]; for (int i = 0; i < 12; ++i) v[i] = std::strtod(argv[3 + i], nullptr);
        lvk::write_msckf_point(stdout, std::atoll(argv[2]), v, v + 3, std::atoi(argv[15]));
        return 0;
    }
    std::fprintf(stderr, "usage: host_tools config|png|imu|images|euroc-args|euroc-args-all|euroc-args-fields|msckf-line|keyframe-line|depth-line|fix-line|landmark-batches ...\n");
    return 2;
}
