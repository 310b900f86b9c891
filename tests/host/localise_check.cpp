// Compile-and-run check of lvk::LarVio::localiseMap (include/lvk_larvio.hpp) against the C ABI: the member's signature, the layout of
// lvk_localise_info as larvio_amd/_lib.py mirrors it, and the behaviour on handles that were never initialised (no device is touched).
#include "lvk_larvio.hpp"
#include <cstddef>
#include <cstdio>
#include <cstring>

int main()
{
    typedef bool (lvk::LarVio::*Fn)(lvk::ImageProcessor&, lvk_localise_info&, const lvk_align_result*, long long, double, double, const lvk_map_select_options*,
                                    const lvk_match_options*, long long);
    Fn fn = &lvk::LarVio::localiseMap;
    lvk_fe_config fc; std::memset(&fc, 0, sizeof fc);
    lvk_ekf_config ec; std::memset(&ec, 0, sizeof ec);
    lvk::ImageProcessor fe(fc, nullptr);
    lvk::LarVio be(ec, nullptr);
    lvk_localise_info info; std::memset(&info, 0x5A, sizeof info);
    const bool ok = (be.*fn)(fe, info, nullptr, -1, 0.0, 1.0, nullptr, nullptr, 0);       // neither handle exists: refused before the library is asked
    std::printf("localiseMap %d\n", ok ? 1 : 0);
    std::printf("sizeof %zu status %zu n_ok %zu n_bad %zu clone_id %zu map %zu R_wc %zu p_wc %zu cov_cam %zu\n", sizeof(lvk_localise_info), offsetof(lvk_localise_info, status),
                offsetof(lvk_localise_info, n_ok), offsetof(lvk_localise_info, n_bad), offsetof(lvk_localise_info, clone_id), offsetof(lvk_localise_info, map),
                offsetof(lvk_localise_info, R_wc), offsetof(lvk_localise_info, p_wc), offsetof(lvk_localise_info, cov_cam));
    std::printf("obs_info %zu camera_pose_job %zu codes %d %d\n", sizeof(lvk_map_obs_info), sizeof(lvk_camera_pose_job), LVK_LOCALISE_QUEUED, LVK_LOCALISE_NO_CLONE);
    return ok ? 1 : 0;
}
