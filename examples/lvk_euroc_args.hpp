// lvk_euroc_args.hpp — the options of examples/larvio_euroc after its four positional arguments, and the line format of its
// --msckf-out, --keyframes-out and --depth-out files; host-only, so that examples/host_tools can show both on a machine without a GPU.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace lvk {

struct EurocArgs { std::string tum, mask, map_out, msckf_out, keyframes_out, depth_out, fixes, landmarks; long max_frames; bool pipelined; double fix_max_gap;
                   EurocArgs() : max_frames(-1), pipelined(false), fix_max_gap(0.0) {} };

// argv[first..]: false, with the offending word in *bad, on an unknown option or an option without its value
inline bool parse_euroc_args(int argc, char** argv, int first, EurocArgs* o, std::string* bad)
{
    for (int a = first; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--tum") && a + 1 < argc) o->tum = argv[++a];
        else if (!std::strcmp(argv[a], "--max-frames") && a + 1 < argc) o->max_frames = std::atol(argv[++a]);
        else if (!std::strcmp(argv[a], "--pipelined")) o->pipelined = true;
        else if (!std::strcmp(argv[a], "--mask") && a + 1 < argc) o->mask = argv[++a];
        else if (!std::strcmp(argv[a], "--map-out") && a + 1 < argc) o->map_out = argv[++a];
        else if (!std::strcmp(argv[a], "--msckf-out") && a + 1 < argc) o->msckf_out = argv[++a];
        else if (!std::strcmp(argv[a], "--keyframes-out") && a + 1 < argc) o->keyframes_out = argv[++a];
        else if (!std::strcmp(argv[a], "--depth-out") && a + 1 < argc) o->depth_out = argv[++a];
        else if (!std::strcmp(argv[a], "--fixes") && a + 1 < argc) o->fixes = argv[++a];
        else if (!std::strcmp(argv[a], "--fix-max-gap") && a + 1 < argc) o->fix_max_gap = std::atof(argv[++a]);
        else if (!std::strcmp(argv[a], "--landmarks") && a + 1 < argc) o->landmarks = argv[++a];
        else { if (bad) *bad = argv[a]; return false; }
    }
    return true;
}

// one --msckf-out line: "id x y z s00 s01 s02 s10 s11 s12 s20 s21 s22 n_obs" (17 significant digits: the doubles round-trip)
inline void write_msckf_point(FILE* f, long long id, const double* p, const double* c, int n_obs)
{
    std::fprintf(f, "%lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", id, p[0], p[1], p[2], c[0], c[1], c[2], c[3], c[4],
                 c[5], c[6], c[7], c[8], n_obs);
}

// one --keyframes-out line: "id to_id time to_time q(4) p(3) rel_q(4) rel_p(3) cov_abs(36) cov_rel(36)", the matrices row-major (17
// significant digits: the doubles round-trip); v: the 88 doubles from time on, in that order
inline void write_keyframe(FILE* f, long long id, long long to_id, const double* v)
{
    std::fprintf(f, "%lld %lld", id, to_id);
    for (int i = 0; i < 88; ++i) std::fprintf(f, " %.17g", v[i]);
    std::fprintf(f, "\n");
}

// one --depth-out line: "timestamp id x y z s00 s01 s02 s11 s12 s22" - the state time (9 decimals, as --tum writes it), the feature, its
// position in the camera frame of that state and the upper triangle of its 3 x 3 covariance there (17 significant digits: the doubles
// round-trip; s22 is the depth variance)
inline void write_depth_point(FILE* f, double t, long long id, const double* p, const double* c)
{
    std::fprintf(f, "%.9f %lld %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", t, id, p[0], p[1], p[2], c[0], c[1], c[2], c[4], c[5], c[8]);
}

// one --fixes line: "time,kind,px,py,pz,qx,qy,qz,qw,sigma_p,sigma_theta[,lx,ly,lz]" - kind 0 position / 1 pose, the fix in the filter's
// world frame at `time` on the IMU clock, isotropic standard deviations (m, rad), an optional lever arm in the body frame.  v: the 14
// numbers in that order (the lever arm zero when absent).  false: not such a line (a comment, a header, too few fields).
inline bool parse_fix_line(const char* line, double v[14])
{
    for (int i = 0; i < 14; ++i) v[i] = 0.0;
    int n = 0; const char* p = line;
    while (n < 14) {
        char* end = nullptr; const double x = std::strtod(p, &end);
        if (end == p) break;
        v[n++] = x; p = end;
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
        if (*p != ',') break;
        ++p;
    }
    return (n == 11 || n == 14) && (v[1] == 0.0 || v[1] == 1.0);
}

// one --landmarks line: "time,px,py,pz,u,v,sigma[,sigma_w]" - an observation (u, v, normalised image coordinates, standard deviation
// sigma) made in the image at `time` (IMU clock) of the point (px, py, pz) of the filter's world frame, known to an isotropic standard
// deviation sigma_w (0 when absent).  v: the 8 numbers in that order.  false: not such a line (a comment, a header, too few fields).
inline bool parse_landmark_line(const char* line, double v[8])
{
    for (int i = 0; i < 8; ++i) v[i] = 0.0;
    int n = 0; const char* p = line;
    while (n < 8) {
        char* end = nullptr; const double x = std::strtod(p, &end);
        if (end == p) break;
        v[n++] = x; p = end;
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
        if (*p != ',') break;
        ++p;
    }
    return n == 7 || n == 8;
}

// the batches of a --landmarks file: consecutive lines with equal time form one batch.  rows: 8 doubles per line as parse_landmark_line
// gives them, in file order; first[b] .. first[b + 1]: the lines of batch b
struct LandmarkFile {
    std::vector<double> rows; std::vector<size_t> first;
    size_t batches() const { return first.empty() ? 0 : first.size() - 1; }
    bool load(const std::string& path)
    {
        FILE* f = std::fopen(path.c_str(), "r");
        if (!f) return false;
        char line[1024]; size_t n = 0;
        while (std::fgets(line, sizeof line, f)) {
            double v[8];
            if (!parse_landmark_line(line, v)) continue;
            if (n == 0 || v[0] != rows[8 * (n - 1)]) first.push_back(n);
            rows.insert(rows.end(), v, v + 8); ++n;
        }
        std::fclose(f);
        if (n) first.push_back(n);
        return true;
    }
};

}   // namespace lvk
