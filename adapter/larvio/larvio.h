// adapter/larvio/larvio.h — drop-in replacement of the reference's include/larvio/larvio.h: the same class name, namespace, public
// members and typedefs (/root/reference/include/larvio/larvio.h:37-90,421), so that app/larvioMain.cpp (:50-55,114,139-155) and
// ros_wrapper System.cpp compile and link unchanged; everything private is a handle into liblvk_hip.so.
#ifndef LARVIO_H
#define LARVIO_H

#include <map>
#include <string>
#include <vector>
#include <cstdio>
#include <boost/shared_ptr.hpp>
#include <Eigen/Dense>
#include <Eigen/Geometry>

#include <larvio/feature_msg.h>
#include "sensors/ImuData.hpp"
#include "lvk_c.h"

namespace larvio {

typedef long long int FeatureIDType;      // include/larvio/imu_state.h:24

class LarVio {
  public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW

    LarVio(std::string& config_file_);                    // larvio.cpp:40-44
    LarVio(const LarVio&) = delete;
    LarVio operator=(const LarVio&) = delete;
    ~LarVio();                                            // larvio.cpp:47-55

    bool initialize();                                    // larvio.cpp:314-360
    void reset();                                         // declared by the reference (larvio.h:57), never defined there; here: start over
    // larvio.cpp:363-461: erases the IMU samples it consumed from imu_msg_buffer (:511-512); true = publish
    bool processFeatures(MonoCameraMeasurementPtr msg, std::vector<ImuData>& imu_msg_buffer);

    Eigen::Isometry3d getTbw();                           // larvio.cpp:2644-2658
    Eigen::Vector3d getVel();                             // :2661-2668
    Eigen::Matrix<double, 6, 6> getPpose();               // :2671-2688
    Eigen::Matrix3d getPvel();                            // :2691-2699
    void getSwPoses(std::vector<Eigen::Isometry3d>& swPoses);                                            // :2702-2716
    void getStableMapPointPositions(std::map<larvio::FeatureIDType, Eigen::Vector3d>& mMapPoints);       // :2719-2723 (clears on read)
    void getActiveeMapPointPositions(std::map<larvio::FeatureIDType, Eigen::Vector3d>& mMapPoints);      // :2726-2730 (clears on read)

    // not in the reference: the MSCKF points the lost-feature updates triangulate, accept and erase, each with its 3 x 3 position
    // covariance (lvk_ekf_set_msckf_points / lvk_ekf_take_msckf_points, lvk_c.h); cov9: 9 doubles per point, row-major (drained on read)
    bool setMsckfPoints(bool on);
    void takeMsckfPoints(std::vector<FeatureIDType>& ids, std::vector<Eigen::Vector3d>& positions, std::vector<double>& cov9, std::vector<int>& n_obs);

    // not in the reference: the clones the pruning removes, each with its absolute 6 x 6 covariance and the covariance of its pose
    // relative to the nearest newer surviving clone (lvk_ekf_set_keyframe_export / lvk_ekf_take_keyframes, lvk_c.h; drained on read),
    // and the same for the clones still in the window (lvk_ekf_get_window_cov: 36 doubles per clone each, row-major)
    bool setKeyframeExport(bool on);
    void takeKeyframes(std::vector<lvk_keyframe>& keyframes);
    bool getWindowCov(std::vector<long long>& ids, std::vector<double>& cov_abs36, std::vector<double>& cov_rel36);

    // not in the reference: the active map points in the camera frame of the current IMU state (to_clone_id -1) or of a clone of the
    // window, each with its 3 x 3 covariance there, in which the unobservable global position and yaw cancel (lvk_ekf_get_feature_rel,
    // lvk_c.h); cov9: 9 doubles per point, row-major, NaN where the anchor clone has left the window
    bool getFeaturesInCamera(std::vector<FeatureIDType>& ids, std::vector<Eigen::Vector3d>& positions_c, std::vector<double>& cov9, long long to_clone_id = -1);

    // not in the reference: external position / pose fixes on a clone of the window, expressed in the filter's world frame
    // (lvk_ekf_add_fix / lvk_ekf_set_fix_options / lvk_ekf_take_fix_reports, lvk_c.h: models, target clone, gate, refusals); the next
    // processFeatures that holds the clone applies a queued fix, takeFixReports says what became of each (drained on read)
    bool addFix(const lvk_fix& fix);
    bool setFixOptions(double gate_scale, double max_gap_s);
    void takeFixReports(std::vector<lvk_fix_report>& reports);
    // not in the reference: image observations of points whose world position is known, all made in one image, fused on that image's
    // clone (lvk_ekf_add_landmark_obs / lvk_ekf_set_landmark_options / lvk_ekf_take_landmark_reports / lvk_ekf_landmark_stats, lvk_c.h)
    bool addLandmarkObs(long long tag, long long clone_id, double time, const std::vector<lvk_landmark_obs>& obs);
    bool setLandmarkOptions(double gate_scale, double min_depth);
    void takeLandmarkReports(std::vector<lvk_landmark_report>& reports);
    void landmarkStats(long out12[12]);

    typedef boost::shared_ptr<LarVio> Ptr;
    typedef boost::shared_ptr<const LarVio> ConstPtr;

  private:
    void writeLogs();
    void finish();                                        // waits for a deferred update, then the logs / map points that follow it
    std::string config_file;
    lvk_ekf_config cfg;
    lvk_context* ctx;
    lvk_ekf* ekf;
    std::FILE *f_state, *f_takeoff;
    bool takeoff_written;
    bool failed; double good_state[30];                   // a (deferred) update failed: the filter is unusable, getters answer from the last good state
    bool blocking, pending;                               // LVK_ADAPTER_BLOCKING=1: processFeatures runs the update before it returns
    std::map<FeatureIDType, Eigen::Vector3d> active_slam_features;   // refreshed after every update (larvio.cpp:455-458), cleared on read
};

typedef LarVio::Ptr LarVioPtr;
typedef LarVio::ConstPtr LarVioConstPtr;

} // namespace larvio

#endif
