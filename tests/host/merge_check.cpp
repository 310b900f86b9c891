// Compile-and-run check of lvk::ImageProcessor::mergeMap (include/lvk_larvio.hpp) against the C ABI: the member's signature, the layout of
// the 3D alignment's records as larvio_amd/_lib.py mirrors them, lvk_align_invert (host code) on one alignment, and the behaviour on a
// handle that was never initialised (no device is touched).
#include "lvk_larvio.hpp"
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    typedef bool (lvk::ImageProcessor::*Fn)(const std::vector<double>&, const std::vector<double>&, const std::vector<uint8_t>&, lvk_align_result&, const lvk_align_result*,
                                            const double*, const lvk_map_build_options*, const lvk_match_options*, const lvk_align3d_options*, int, uint32_t, std::vector<int>*,
                                            lvk_map_build_info*, lvk_global_info*);
    Fn fn = &lvk::ImageProcessor::mergeMap;
    lvk_fe_config fc; std::memset(&fc, 0, sizeof fc);
    lvk::ImageProcessor fe(fc, nullptr);
    std::vector<double> X(3, 0.0), cov(9, 0.0); std::vector<uint8_t> desc(32, 0);
    lvk_align_result used; std::memset(&used, 0x5A, sizeof used);
    const bool ok = (fe.*fn)(X, cov, desc, used, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);      // no handle: refused before the library is asked
    std::printf("mergeMap %d\n", ok ? 1 : 0);
    std::printf("match %zu X %zu Y %zu hyp %zu n_models %zu count %zu c %zu s %zu t %zu options %zu thresh %zu min_rho %zu min_inliers %zu\n", sizeof(lvk_align3d_match),
                offsetof(lvk_align3d_match, X), offsetof(lvk_align3d_match, Y), sizeof(lvk_align3d_hyp), offsetof(lvk_align3d_hyp, n_models), offsetof(lvk_align3d_hyp, count),
                offsetof(lvk_align3d_hyp, c), offsetof(lvk_align3d_hyp, s), offsetof(lvk_align3d_hyp, t), sizeof(lvk_align3d_options), offsetof(lvk_align3d_options, thresh),
                offsetof(lvk_align3d_options, min_rho), offsetof(lvk_align3d_options, min_inliers));
    lvk_align_result in, out; std::memset(&in, 0, sizeof in); std::memset(&out, 0x5A, sizeof out);
    in.c = 0.6; in.s = 0.8; in.t[0] = 3.0; in.t[1] = -2.0; in.t[2] = 0.5; in.status = 3; in.rms = 7.0;
    const int st = (int)lvk_align_invert(&in, &out);
    std::printf("invert %d %.17g %.17g %.17g %.17g %.17g status %d rms %g null %d\n", st, out.c, out.s, out.t[0], out.t[1], out.t[2], out.status, out.rms,
                (int)lvk_align_invert(nullptr, &out));
    return ok ? 1 : 0;
}
