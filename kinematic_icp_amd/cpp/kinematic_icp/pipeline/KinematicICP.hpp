// kinematic_icp/pipeline/KinematicICP.hpp -- drop-in for the reference header of the same path
// (/root/reference/cpp/kinematic_icp/pipeline/KinematicICP.{hpp,cpp}): same Config fields and defaults, same class
// surface (RegisterFrame, SetPose, LocalMap, VoxelMap, pose), so ros/src/.../LidarOdometryServer.cpp compiles
// against it unchanged.  The ICP (registration_ + local_map_) and - unless KICP_HOST_PRESTEPS is defined - the
// pre-steps (deskew + crop + transform, two-level voxel downsample: kicp_pre_*) run on the MI355X; the registration
// source and the frame that goes into the map never leave HBM, and the map update itself (kiss-icp Update: ordered
// insertion + far-voxel removal) runs there too.  The threshold bookkeeping stays on the host
// (SURVEY.md section 8f rows 1, 2 and 4).
#pragma once
#include <Eigen/Core>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <kiss_icp/core/Preprocessing.hpp>
#include <kiss_icp/core/VoxelHashMap.hpp>
#include <kiss_icp/core/VoxelUtils.hpp>
#include <memory>
#include <sophus/se3.hpp>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "kinematic_icp/correspondence_threshold/CorrespondenceThreshold.hpp"
#include "kinematic_icp/registration/Registration.hpp"

namespace kinematic_icp::pipeline {

struct Config {
    // Preprocessing
    double max_range = 100.0;
    double min_range = 0.0;
    // Mapping parameters
    double voxel_size = 1.0;
    unsigned int max_points_per_voxel = 20;
    // Derived parameter
    double map_resolution() const { return voxel_size / std::sqrt(max_points_per_voxel); }
    // Correspondence threshold parameters
    bool use_adaptive_threshold = true;
    double fixed_threshold = 1.0;
    // Registration Parameters
    int max_num_iterations = 10;
    double convergence_criterion = 0.001;
    int max_num_threads = 1;
    bool use_adaptive_odometry_regularization = true;
    double fixed_regularization = 0.0;
    // Motion compensation
    bool deskew = false;
    // backend extension (last member, so aggregate initialisers of the reference's fields keep their meaning): false = localisation in a
    // prior map - RegisterFrame and its siblings do everything but the map update, and SetPose leaves the map alone
    bool update_map = true;
};

class KinematicICP {
public:
    using Vector3dVector = std::vector<Eigen::Vector3d>;
    using Vector3dVectorTuple = std::tuple<Vector3dVector, Vector3dVector>;

    explicit KinematicICP(const Config &config)
        : registration_(config.max_num_iterations, config.convergence_criterion, config.max_num_threads,
                        config.use_adaptive_odometry_regularization, config.fixed_regularization),
          correspondence_threshold_(config.map_resolution(), config.max_range, config.use_adaptive_threshold, config.fixed_threshold),
          config_(config),
          preprocessor_(config.max_range, config.min_range, config.deskew, config.max_num_threads),
          local_map_(config.voxel_size, config.max_range, config.max_points_per_voxel) {
#ifndef KICP_HOST_PRESTEPS
        kicp_bridge::check(kicp_pre_create(kicp_bridge::default_device(), &pre_), "KinematicICP");
#endif
    }
    ~KinematicICP() { kicp_pre_destroy(pre_); }
    // copyable and movable like the reference's class (every member is held by value there, KinematicICP.hpp:100-108): a copy owns
    // a deep copy of the map (and of the occupancy grid and the height columns, when enabled, and a depth view of the same configuration), a registration
    // handle of its own and its own pre-step workspace
    KinematicICP(const KinematicICP &o)
        : last_pose_(o.last_pose_),
          registration_(o.registration_),
          correspondence_threshold_(o.correspondence_threshold_),
          config_(o.config_),
          preprocessor_(o.preprocessor_),
          local_map_(o.local_map_),
          grid_(kicp_bridge::clone_grid(o.grid_.get())),
          transients_enabled_(o.transients_enabled_),
          transient_config_(o.transient_config_),
          grid_follow_(o.grid_follow_),
          elev_(kicp_bridge::clone_elevation(o.elev_.get())),
          elev_follow_(o.elev_follow_),
          last_elev_stats_(o.last_elev_stats_),
          elev_carving_(o.elev_carving_),
          elev_carve_(o.elev_carve_),
          last_elev_carve_stats_(o.last_elev_carve_stats_),
          view_(kicp_bridge::clone_view(o.view_.get())),
          last_removal_(o.last_removal_),
          sensor_in_base_(o.sensor_in_base_) {
#ifndef KICP_HOST_PRESTEPS
        kicp_bridge::check(kicp_pre_create(kicp_bridge::default_device(), &pre_), "KinematicICP");
#endif
    }
    KinematicICP(KinematicICP &&o) noexcept
        : last_pose_(o.last_pose_),
          registration_(std::move(o.registration_)),
          correspondence_threshold_(o.correspondence_threshold_),
          config_(o.config_),
          preprocessor_(o.preprocessor_),
          local_map_(std::move(o.local_map_)),
          pre_(o.pre_),
          grid_(std::move(o.grid_)),
          transients_enabled_(o.transients_enabled_),
          transient_config_(o.transient_config_),
          last_transients_(std::move(o.last_transients_)),
          grid_follow_(o.grid_follow_),
          elev_(std::move(o.elev_)),
          elev_follow_(o.elev_follow_),
          last_elev_stats_(o.last_elev_stats_),
          elev_carving_(o.elev_carving_),
          elev_carve_(o.elev_carve_),
          last_elev_carve_stats_(o.last_elev_carve_stats_),
          view_(std::move(o.view_)),
          last_removal_(o.last_removal_),
          sensor_in_base_(o.sensor_in_base_) {
        o.pre_ = nullptr;
    }
    KinematicICP &operator=(KinematicICP o) noexcept {  // copy / move and swap
        std::swap(last_pose_, o.last_pose_);
        registration_ = std::move(o.registration_);
        std::swap(correspondence_threshold_, o.correspondence_threshold_), std::swap(config_, o.config_), std::swap(preprocessor_, o.preprocessor_);
        local_map_ = std::move(o.local_map_);
        std::swap(pre_, o.pre_);
        std::swap(elev_carving_, o.elev_carving_), std::swap(elev_carve_, o.elev_carve_), std::swap(last_elev_carve_stats_, o.last_elev_carve_stats_);
        std::swap(transients_enabled_, o.transients_enabled_), std::swap(transient_config_, o.transient_config_), std::swap(last_transients_, o.last_transients_);
        std::swap(grid_follow_, o.grid_follow_), std::swap(elev_follow_, o.elev_follow_);
        std::swap(grid_, o.grid_), std::swap(elev_, o.elev_), std::swap(last_elev_stats_, o.last_elev_stats_), std::swap(view_, o.view_), std::swap(last_removal_, o.last_removal_), std::swap(sensor_in_base_, o.sensor_in_base_);
        return *this;
    }

    // pipeline/KinematicICP.cpp:48-85
    Vector3dVectorTuple RegisterFrame(const std::vector<Eigen::Vector3d> &frame, const std::vector<double> &timestamps,
                                      const Sophus::SE3d &lidar_to_base, const Sophus::SE3d &relative_odometry) {
        sensor_in_base_ = lidar_to_base.translation();
        const Sophus::SE3d relative_odometry_in_lidar = lidar_to_base.inverse() * relative_odometry * lidar_to_base;
#ifndef KICP_HOST_PRESTEPS
        double rel_lidar[7], ext[7];
        kicp_bridge::to_params(relative_odometry_in_lidar, rel_lidar);
        kicp_bridge::to_params(lidar_to_base, ext);
        // Preprocess + transform_points + the two VoxelDownsamples as ONE backend call behind one host synchronisation; the
        // preprocessed frame (a return value nothing on the device waits for) travels back while the downsamples run
        Vector3dVectorTuple result{Vector3dVector(frame.size()), Vector3dVector()};
        auto &out_frame = std::get<0>(result);
        DownloadGuard guard{pre_};
        size_t counts[3] = {0, 0, 0};
        const int order = kicp_bridge::check(
            kicp_pre_frame(pre_, kicp_bridge::xyz(frame), frame.size(), timestamps.data(), timestamps.size(), rel_lidar, ext, config_.max_range, config_.min_range,
                           config_.deskew ? 1 : 0, config_.voxel_size * 0.5, config_.voxel_size * 1.5, out_frame.empty() ? nullptr : out_frame.front().data(),
                           out_frame.size(), counts),
            "Preprocess + VoxelDownsample");
        if (order == KICP_WARN_TABLE_ORDER) kicp_bridge::warn_once(kicp_last_error());
        return RegisterChained(result, guard, counts, relative_odometry);
#else
        const auto preprocessed_frame = preprocessor_.Preprocess(frame, timestamps, relative_odometry_in_lidar);
        Vector3dVector preprocessed_frame_in_base(preprocessed_frame.size());
        for (size_t i = 0; i < preprocessed_frame.size(); ++i) preprocessed_frame_in_base[i] = lidar_to_base * preprocessed_frame[i];
        const auto frame_downsample = kiss_icp::VoxelDownsample(preprocessed_frame_in_base, config_.voxel_size * 0.5);
        const auto source = kiss_icp::VoxelDownsample(frame_downsample, config_.voxel_size * 1.5);
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto new_pose = registration_.ComputeRobotMotion(source, local_map_, last_pose_, relative_odometry, tau);
        const auto odometry_error = (last_pose_ * relative_odometry).inverse() * new_pose;
        correspondence_threshold_.UpdateOdometryError(odometry_error);
        if (view_ && config_.update_map) RemoveSeenThrough(kicp_bridge::xyz(preprocessed_frame_in_base), preprocessed_frame_in_base.size(), false, new_pose);
        if (config_.update_map) local_map_.Update(frame_downsample, new_pose);
        last_pose_ = new_pose;
        FollowPose();
        if (grid_ && transients_enabled_) DetectTransients(kicp_bridge::xyz(preprocessed_frame_in_base), preprocessed_frame_in_base.size(), false);
        if (grid_) IntegrateGrid(kicp_bridge::xyz(preprocessed_frame_in_base), preprocessed_frame_in_base.size(), false);
        if (elev_) IntegrateElevation(kicp_bridge::xyz(preprocessed_frame_in_base), preprocessed_frame_in_base.size(), false);
        return {preprocessed_frame_in_base, source};
#endif
    }

#ifndef KICP_HOST_PRESTEPS
    // ---- backend extension: feed the PointCloud2 bytes directly ----
    // IngestCloud replaces PointCloud2ToEigen(msg, {}) (RosUtils.cpp:30-39) and the per-point part of
    // TimeStampHandler::ProcessTimestamps (TimeStampHandler.cpp:57-106,121-128): it returns {cloud has stamps, min stamp,
    // max stamp} (seconds), which is all ProcessTimestamps' begin/end-stamp logic (:107-119) needs; the decoded points
    // and normalised stamps stay in HBM.  RegisterIngestedFrame is RegisterFrame on that cloud.
    std::tuple<bool, double, double> IngestCloud(const void *data, size_t n_points, const kicp_cloud_layout &layout) {
        double lo = 0.0, hi = 0.0;
        kicp_bridge::check(kicp_pre_ingest(pre_, data, n_points, &layout, nullptr, &lo, &hi), "IngestCloud");
        return {layout.stamp_datatype != 0 && n_points != 0, lo, hi};
    }
    // IngestScan is the 2-D LiDAR mode of the node (online_node.cpp:44-58): laser_geometry's projectLaser(*msg, cloud, range_cutoff,
    // channel_option::Timestamp) and then what IngestCloud does with that cloud, on the GPU from the raw ranges (kicp.h
    // kicp_pre_ingest_scan).  `ranges` = msg->ranges.data(), n = msg->ranges.size().  It returns {a beam was kept, min stamp, max
    // stamp} like IngestCloud; RegisterIngestedFrame then registers the projected scan.
    std::tuple<bool, double, double> IngestScan(const float *ranges, size_t n, const kicp_laser_scan &scan, double range_cutoff = -1.0) {
        double lo = 0.0, hi = 0.0;
        kicp_bridge::check(kicp_pre_ingest_scan(pre_, ranges, n, &scan, range_cutoff, &lo, &hi), "IngestScan");
        return {kicp_pre_ingested_count(pre_) != 0, lo, hi};
    }
    // Look-ahead for callers that already hold the NEXT message (a bag replay; ros/src/kinematic_icp_ros/nodes/offline_node.cpp reads
    // its messages in a loop): announce it before RegisterIngestedFrame of the current one - it is then uploaded and decoded while the
    // current frame's pre-steps run, and its IngestCloud call returns at once.  The bytes must stay valid until that IngestCloud call.
    void AnnounceNextCloud(const void *data, size_t n_points, const kicp_cloud_layout &layout) {
        kicp_bridge::check(kicp_pre_ingest_ahead(pre_, data, n_points, &layout, nullptr), "AnnounceNextCloud");
    }
    Vector3dVectorTuple RegisterIngestedFrame(const Sophus::SE3d &lidar_to_base, const Sophus::SE3d &relative_odometry) {
        sensor_in_base_ = lidar_to_base.translation();
        const Sophus::SE3d relative_odometry_in_lidar = lidar_to_base.inverse() * relative_odometry * lidar_to_base;
        double rel_lidar[7], ext[7];
        kicp_bridge::to_params(relative_odometry_in_lidar, rel_lidar);
        kicp_bridge::to_params(lidar_to_base, ext);
        Vector3dVectorTuple result{Vector3dVector(kicp_pre_ingested_count(pre_)), Vector3dVector()};
        auto &out_frame = std::get<0>(result);
        DownloadGuard guard{pre_};
        size_t counts[3] = {0, 0, 0};
        const int order = kicp_bridge::check(
            kicp_pre_frame_ingested(pre_, rel_lidar, ext, config_.max_range, config_.min_range, config_.deskew ? 1 : 0, config_.voxel_size * 0.5,
                                    config_.voxel_size * 1.5, out_frame.empty() ? nullptr : out_frame.front().data(), out_frame.size(), counts),
            "Preprocess + VoxelDownsample");
        if (order == KICP_WARN_TABLE_ORDER) kicp_bridge::warn_once(kicp_last_error());
        return RegisterChained(result, guard, counts, relative_odometry);
    }
    // ---- backend extension: the published clouds as PointCloud2 `data` (LidarOdometryServer.cpp:240-263 PublishClouds, which
    // converts each with EigenToPointCloud2, RosUtils.cpp:40-63) ----
    // RegisterFrameF32 / RegisterIngestedFrameF32 are RegisterFrame / RegisterIngestedFrame - the same pose, threshold and map update -
    // with the two returned clouds written as x y z FLOAT32 records (kicp_bridge::PointCloud2Xyz32) into the byte vectors a node hands
    // over as msg->data: the GPU narrows them, 12 bytes per point cross PCIe and the host makes no pass of its own over them.  A null
    // pointer means the cloud is not produced at all (a topic without subscriber): the frame is then not even pushed.
    void RegisterFrameF32(const std::vector<Eigen::Vector3d> &frame, const std::vector<double> &timestamps, const Sophus::SE3d &lidar_to_base,
                          const Sophus::SE3d &relative_odometry, std::vector<uint8_t> *frame_data, std::vector<uint8_t> *keypoints_data) {
        sensor_in_base_ = lidar_to_base.translation();
        const Sophus::SE3d relative_odometry_in_lidar = lidar_to_base.inverse() * relative_odometry * lidar_to_base;
        double rel_lidar[7], ext[7];
        kicp_bridge::to_params(relative_odometry_in_lidar, rel_lidar);
        kicp_bridge::to_params(lidar_to_base, ext);
        float *out = LandFrame(frame_data, frame.size());
        DownloadGuard guard{pre_, out != nullptr};
        size_t counts[3] = {0, 0, 0};
        const int order = kicp_bridge::check(
            kicp_pre_frame_f32(pre_, kicp_bridge::xyz(frame), frame.size(), timestamps.data(), timestamps.size(), rel_lidar, ext, config_.max_range,
                               config_.min_range, config_.deskew ? 1 : 0, config_.voxel_size * 0.5, config_.voxel_size * 1.5, out, frame.size(), counts),
            "Preprocess + VoxelDownsample");
        if (order == KICP_WARN_TABLE_ORDER) kicp_bridge::warn_once(kicp_last_error());
        RegisterChainedF32(guard, counts, relative_odometry, frame_data, keypoints_data);
    }
    void RegisterIngestedFrameF32(const Sophus::SE3d &lidar_to_base, const Sophus::SE3d &relative_odometry, std::vector<uint8_t> *frame_data,
                                  std::vector<uint8_t> *keypoints_data) {
        sensor_in_base_ = lidar_to_base.translation();
        const Sophus::SE3d relative_odometry_in_lidar = lidar_to_base.inverse() * relative_odometry * lidar_to_base;
        double rel_lidar[7], ext[7];
        kicp_bridge::to_params(relative_odometry_in_lidar, rel_lidar);
        kicp_bridge::to_params(lidar_to_base, ext);
        const size_t n_in = kicp_pre_ingested_count(pre_);
        float *out = LandFrame(frame_data, n_in);
        DownloadGuard guard{pre_, out != nullptr};
        size_t counts[3] = {0, 0, 0};
        const int order = kicp_bridge::check(
            kicp_pre_frame_ingested_f32(pre_, rel_lidar, ext, config_.max_range, config_.min_range, config_.deskew ? 1 : 0, config_.voxel_size * 0.5,
                                        config_.voxel_size * 1.5, out, n_in, counts),
            "Preprocess + VoxelDownsample");
        if (order == KICP_WARN_TABLE_ORDER) kicp_bridge::warn_once(kicp_last_error());
        RegisterChainedF32(guard, counts, relative_odometry, frame_data, keypoints_data);
    }
    // LocalMap() as the published map's msg->data (kiss_icp::VoxelHashMap::PointcloudF32)
    void LocalMapF32(std::vector<uint8_t> &data) const { local_map_.PointcloudF32(data); }
#endif

    // (with Config::update_map == false the map is a prior the caller loaded: SetPose then moves the robot, not the map)
    inline void SetPose(const Sophus::SE3d &pose) {
        last_pose_ = pose;
        if (config_.update_map) local_map_.Clear();
        correspondence_threshold_.Reset();
    }

    // ---- backend extension: localising in a saved map (INTEGRATION.md "Localising in a saved map") ----
    // SaveMap writes the local map as a PCD file; LoadMap replaces it by a file's map (its voxel size, range and points per voxel come
    // from the file's `# kicp_map` line when it has one, from this pipeline's Config otherwise).
    void SaveMap(const std::string &path) const { local_map_.SavePCD(path); }
    void LoadMap(const std::string &path) {
        try {
            local_map_ = kiss_icp::VoxelHashMap::LoadPCD(path);
        } catch (const std::runtime_error &) {  // (a foreign file without the parameter line; any other problem throws again)
            local_map_ = kiss_icp::VoxelHashMap::LoadPCD(path, config_.voxel_size, config_.max_range, config_.max_points_per_voxel);
        }
    }
    // Relocalize: which of `candidates` (kicp_bridge::planar_grid builds a grid) explains `keypoints` - a registration source in the
    // base frame, e.g. the second cloud RegisterFrame returns - best: all are scored against the map, the top_m cheapest refined and
    // scored again (kicp.h kicp_relocalize; tau = the threshold of a first frame).  The result becomes the pipeline's pose.  The
    // refinement moves along the kinematic model only: with this call the candidates' lateral spacing is the accuracy.
    KinematicRegistration::Relocalization Relocalize(const std::vector<Eigen::Vector3d> &keypoints, const std::vector<Sophus::SE3d> &candidates,
                                                     size_t top_m = 8) {
        correspondence_threshold_.Reset();
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto found = registration_.Relocalize(keypoints, local_map_, candidates, tau, top_m);
        last_pose_ = found.pose;
        return found;
    }
    // RelocalizePlanar: the same with the finalists refined in the plane - x, y and yaw - instead of along the kinematic model (kicp.h
    // kicp_relocalize_planar), so the result is not tied to the candidates' lateral spacing.  The result becomes the pipeline's pose.
    KinematicRegistration::Relocalization RelocalizePlanar(const std::vector<Eigen::Vector3d> &keypoints, const std::vector<Sophus::SE3d> &candidates,
                                                           size_t top_m = 8, int max_iterations = 100, double convergence = 1e-4) {
        correspondence_threshold_.Reset();
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto found = registration_.RelocalizePlanar(keypoints, local_map_, candidates, tau, top_m, max_iterations, convergence);
        last_pose_ = found.pose;
        return found;
    }
    // BuildOccupancy: the occupancy pyramid of the map as it is NOW (kicp.h kicp_occ_build; a snapshot - build it again after the map
    // changed), `cell` about the map's point spacing voxel_size / sqrt(max_points_per_voxel).  RelocalizeSearch then needs no
    // candidates: it searches a whole window (kicp_bridge::search_window_around(Occupancy(), ...); half extents <= 0: the whole map)
    // for the top_m nodes that explain `keypoints` best and refines them in the plane (kicp.h kicp_relocalize_search).  The result
    // becomes the pipeline's pose.
    void BuildOccupancy(double cell, int dilate = 1, int levels = 4) { occupancy_ = kicp_bridge::build_occupancy(local_map_.handle(), cell, dilate, levels); }
    const kicp_occ *Occupancy() const { return occupancy_.get(); }
    KinematicRegistration::Relocalization RelocalizeSearch(const std::vector<Eigen::Vector3d> &keypoints, const kicp_search_window &window,
                                                           size_t top_m = 8, int max_iterations = 100, double convergence = 1e-4) {
        if (!occupancy_) throw std::runtime_error("KinematicICP::RelocalizeSearch: call BuildOccupancy first");
        correspondence_threshold_.Reset();
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto found = registration_.RelocalizeSearch(keypoints, local_map_, occupancy_.get(), window, tau, top_m, max_iterations, convergence);
        last_pose_ = found.pose;
        return found;
    }

    // ---- backend extension: an occupancy grid for the planner (INTEGRATION.md "An occupancy grid for the planner") ----
    // With a grid enabled, RegisterFrame, RegisterIngestedFrame and their F32 variants integrate the frame they return - the deskewed,
    // cropped frame in the base frame, all of it - into a 2-D grid after the registration and before they return: at the new pose, with
    // the translation of lidar_to_base as the sensor's origin, every point in the band a hit and the cells its ray crosses free (kicp.h
    // kicp_grid_*).  Poses, thresholds, returned clouds and the map are what they are without the grid.  Config::update_map = false
    // does not stop it: localising in a saved map while drawing a grid of what is seen now is legitimate.  SetPose leaves it alone.
    // Grid() is the shared handle (null without a grid): a node may keep it for the kicp_grid_* calls of its map publisher.
    // (A new grid, or none, ends EnableTransients below - its plane and switch went with the old handle - and EnableGridFollow.)
    void EnableGrid(const kicp_bridge::GridConfig &config) {
        grid_ = kicp_bridge::make_grid(config), transients_enabled_ = false, last_transients_.clear(), grid_follow_ = {};
    }
    void DisableGrid() { grid_.reset(), transients_enabled_ = false, last_transients_.clear(), grid_follow_ = {}; }
    // FOLLOWING (off by default; a new grid starts with it off).  With it on, the grid follows the robot (kicp.h kicp_grid_follow): in
    // every frame, after the registration and before the transients and the integration, it scrolls - by multiples of step_cells per
    // axis - so that the cell of the new pose's translation lies at least margin_cells from every edge; cells that leave are forgotten,
    // cells that enter are unknown, the grid's origin moves (GridOccupancy and SaveGrid report it) and the plan is invalidated.  Most
    // frames do not scroll, which costs no launch.  LastGridScroll(): the (dx, dy) the last frame applied.  A pair the rule refuses -
    // margin_cells or step_cells 0, 2 * margin_cells + step_cells above the width or the height - is std::invalid_argument.  Poses,
    // thresholds, returned clouds and the voxel map are what they are without following: the grid never feeds the registration.
    void EnableGridFollow(unsigned int margin_cells, unsigned int step_cells) {
        kicp_grid_config config{};
        kicp_bridge::check(kicp_grid_info(RequireGrid("EnableGridFollow"), &config, nullptr, nullptr), "EnableGridFollow");
        grid_follow_ = kicp_bridge::make_follow(config.width, config.height, margin_cells, step_cells, "KinematicICP::EnableGridFollow");
    }
    void DisableGridFollow() { grid_follow_ = {}; }
    bool GridFollowEnabled() const { return grid_follow_.enabled; }
    std::array<int, 2> LastGridScroll() const { return grid_follow_.last; }
    std::shared_ptr<kicp_grid> Grid() const { return grid_; }
    // the readout, a nav_msgs/OccupancyGrid's `data`: width * height bytes, row-major from the origin, -1 unknown, else 0 .. 100
    void GridOccupancy(std::vector<int8_t> &data, unsigned int min_observations = 1) const {
        kicp_grid_config config{};
        kicp_bridge::check(kicp_grid_info(RequireGrid("GridOccupancy"), &config, nullptr, nullptr), "GridOccupancy");
        data.resize(static_cast<size_t>(config.width) * config.height);
        kicp_bridge::check(kicp_grid_occupancy(grid_.get(), min_observations, reinterpret_cast<signed char *>(data.data()), data.size()), "GridOccupancy");
    }
    // What a planner plans on (kicp.h kicp_grid_clearance .. kicp_grid_last_window), computed on the GPU from the counters where they
    // are.  GridClearance: per cell of `rect` (null: the full grid) the squared distance in cells to the nearest source within
    // config.radius_cells, radius_cells^2 + 1 where there is none.  GridCostmap: a nav2_msgs/Costmap's data, Nav2's inflation rule over
    // `table` (radius_cells^2 + 2 entries; kicp_grid_cost_table_nav2 fills Nav2's own).  The result for a rectangle equals the full
    // grid's restricted to it, and a frame changes nothing beyond GridLastWindow().grown(radius_cells, width, height): that is all a
    // node has to refresh after RegisterFrame.
    void GridClearance(std::vector<uint16_t> &data, const kicp_bridge::GridClearanceConfig &config, const kicp_bridge::GridRect *rect = nullptr) const {
        const kicp_bridge::GridRect r = GridRectOrAll(rect, "GridClearance");
        data.resize(static_cast<size_t>(r.w) * r.h);
        kicp_bridge::check(kicp_grid_clearance(grid_.get(), &config, r.x0, r.y0, r.w, r.h, data.data(), data.size()), "GridClearance");
    }
    void GridCostmap(std::vector<uint8_t> &data, const kicp_bridge::GridClearanceConfig &config, const std::vector<uint8_t> &table, bool inflate_unknown = false,
                     const kicp_bridge::GridRect *rect = nullptr) const {
        const kicp_bridge::GridRect r = GridRectOrAll(rect, "GridCostmap");
        data.resize(static_cast<size_t>(r.w) * r.h);
        kicp_bridge::check(kicp_grid_costmap(grid_.get(), &config, table.data(), table.size(), inflate_unknown ? 1 : 0, r.x0, r.y0, r.w, r.h, data.data(), data.size()),
                           "GridCostmap");
    }
    // From the costmap to a path (kicp.h kicp_plan_weights .. kicp_grid_potential): the cost-to-go field a planner spreads from its goals
    // - 0 on a passable goal, min(least sum of step weights, plan.max_potential) where a path reaches, 0xFFFFFFFF elsewhere - with
    // q = weight[cost] per cell, 0 for impassable (kicp_plan_weights fills NavFn's table).  GridPotential computes the full grid's
    // costmap as GridCostmap does and spreads the field over it on the GPU: the costmap never leaves HBM.  GridPotentialOfCostmap takes
    // a costmap the node holds (width * height bytes, e.g. the master grid after other layers wrote into it).  goals: (x, y) cells.
    // Returns goals used, cells below max_potential, cells at it, relaxation rounds.  PotentialPath walks down a potential from
    // `start` to a goal (host code; throws for an unreachable start and for one in the zone max_potential clamped) -> the cells as
    // (x, y), start and goal included; it needs the costmap the potential was made from, so a node that plans with GridPotential keeps
    // its costmap current as above.
    using GridCell = std::array<unsigned int, 2>;
    std::array<unsigned long long, 4> GridPotential(std::vector<uint32_t> &data, const kicp_bridge::GridClearanceConfig &config, const std::vector<uint8_t> &table,
                                                    bool inflate_unknown, const std::array<uint8_t, 256> &weight, const std::vector<GridCell> &goals,
                                                    const kicp_bridge::PlanConfig &plan = kicp_bridge::PlanConfig{0xFFFFFFFEu}) const {
        const kicp_bridge::GridRect r = GridRectOrAll(nullptr, "GridPotential");
        data.resize(static_cast<size_t>(r.w) * r.h);
        std::array<unsigned long long, 4> stats{};
        kicp_bridge::check(kicp_grid_potential(grid_.get(), &config, table.data(), table.size(), inflate_unknown ? 1 : 0, weight.data(), &plan,
                                               goals.empty() ? nullptr : goals.front().data(), goals.size(), data.data(), data.size(), stats.data()),
                           "GridPotential");
        return stats;
    }
    std::array<unsigned long long, 4> GridPotentialOfCostmap(std::vector<uint32_t> &data, const std::vector<uint8_t> &costmap, const std::array<uint8_t, 256> &weight,
                                                             const std::vector<GridCell> &goals,
                                                             const kicp_bridge::PlanConfig &plan = kicp_bridge::PlanConfig{0xFFFFFFFEu}) const {
        const kicp_bridge::GridRect r = GridRectOrAll(nullptr, "GridPotentialOfCostmap");
        if (costmap.size() != static_cast<size_t>(r.w) * r.h) throw std::runtime_error("KinematicICP::GridPotentialOfCostmap: the costmap must have the grid's width * height bytes");
        data.resize(costmap.size());
        std::array<unsigned long long, 4> stats{};
        kicp_bridge::check(kicp_grid_potential_of_costmap(grid_.get(), costmap.data(), weight.data(), &plan, goals.empty() ? nullptr : goals.front().data(), goals.size(),
                                                          data.data(), data.size(), stats.data()),
                           "GridPotentialOfCostmap");
        return stats;
    }
    std::vector<GridCell> PotentialPath(const std::vector<uint32_t> &potential, const std::vector<uint8_t> &costmap, const std::array<uint8_t, 256> &weight,
                                        const GridCell &start) const {
        const kicp_bridge::GridRect r = GridRectOrAll(nullptr, "PotentialPath");
        return kicp_bridge::potential_path(potential, costmap, r.w, r.h, weight, start);
    }
    // From the field to a command (kicp.h kicp_plan_q .. kicp_grid_score_arcs): a fan of arcs - one step (dx, dy, dc, ds) each, in the
    // robot's frame; ArcSteps makes them from commands (v, omega) held for dt with the odometry's own motion model - rolled n_steps
    // poses forward from `start` with the footprint's samples (base frame; FootprintBox makes a box's) laid on the plan at every pose.
    // The plan is what the last GridPotential or GridPotentialOfCostmap left on the GPU - q per cell and the potential - and is scored
    // there: nothing but the arcs and the results crosses PCIe.  Per arc: free_steps (poses before the first collision), cost_sum
    // and cost_max of the weights under the footprint along them, end_potential at the last free pose (0xFFFFFFFF outside the grid).
    // Throws without a grid and without a plan ("call GridPotential first").  BestArc ranks the results on the host: the admissible
    // arc (free_steps >= min_free_steps, end_potential != 0xFFFFFFFF) of least w_potential * end_potential + w_cost * cost_sum +
    // w_blocked * (n_steps - free_steps), the lowest index on a tie, results.size() when there is none.
    void ScoreArcs(std::vector<kicp_bridge::ArcResult> &results, const kicp_bridge::ArcStart &start, const std::vector<kicp_bridge::ArcStep> &arcs, unsigned int n_steps,
                   const std::vector<kicp_bridge::FootprintSample> &footprint) const {
        const kicp_grid *grid = RequireGrid("ScoreArcs");
        if (!kicp_grid_has_plan(grid)) throw std::runtime_error("KinematicICP::ScoreArcs: call GridPotential first (or GridPotentialOfCostmap): the grid holds no plan");
        results.resize(arcs.size());
        kicp_bridge::check(kicp_grid_score_arcs(grid, start.data(), arcs.empty() ? nullptr : arcs.front().data(), arcs.size(), n_steps,
                                                footprint.empty() ? nullptr : footprint.front().data(), footprint.size(), results.empty() ? nullptr : results.front().data(),
                                                4 * results.size()),
                           "ScoreArcs");
    }
    // the same from a pose - pose() for the robot as it stands: its x, y and the heading of its x axis in the plane
    void ScoreArcs(std::vector<kicp_bridge::ArcResult> &results, const Sophus::SE3d &pose, const std::vector<kicp_bridge::ArcStep> &arcs, unsigned int n_steps,
                   const std::vector<kicp_bridge::FootprintSample> &footprint) const {
        ScoreArcs(results, kicp_bridge::arc_start(pose), arcs, n_steps, footprint);
    }
    std::vector<kicp_bridge::ArcStep> ArcSteps(const std::vector<double> &v, const std::vector<double> &omega, double dt) const { return kicp_bridge::arc_steps(v, omega, dt); }
    std::vector<kicp_bridge::FootprintSample> FootprintBox(double x_min, double x_max, double y_min, double y_max, double spacing) const {
        return kicp_bridge::footprint_box(x_min, x_max, y_min, y_max, spacing);
    }
    size_t BestArc(const std::vector<kicp_bridge::ArcResult> &results, unsigned int n_steps, unsigned int w_potential = 1, unsigned int w_cost = 0, unsigned int w_blocked = 0,
                   unsigned int min_free_steps = 1) const {
        return kicp_bridge::best_arc(results, n_steps, w_potential, w_cost, w_blocked, min_free_steps);
    }
    // Commands that change along a trajectory (kicp.h kicp_arc_tree_nodes .. kicp_grid_score_arc_tree): a tree of arc segments on the
    // same plan.  Level d + 1 of `tree` offers branch[d] primitives (rows as ArcSteps makes them, level 1's first), each held for
    // steps[d] steps; a node's trajectory runs from `start` through the primitives of its path, and shared prefixes are rolled once on
    // the GPU, one launch per level.  results: one ArcResult per node, level by level (kicp_bridge::arc_tree_nodes gives the counts and
    // the row each level begins at); the child that takes primitive b under node j of a level is node j * branch + b of the next;
    // free_steps counts along the whole path, and a node under one that collided repeats its result.  Throws without a grid and
    // without a plan ("call GridPotential first").  BestArcTreeLeaf ranks the leaves by BestArc's rule with n_steps = the steps along
    // a path: found, the leaf's index in the last level and its path - path[0] is the command to execute now.
    void ScoreArcTree(std::vector<kicp_bridge::ArcResult> &results, const kicp_bridge::ArcStart &start, const kicp_bridge::ArcTree &tree,
                      const std::vector<kicp_bridge::FootprintSample> &footprint) const {
        const kicp_grid *grid = RequireGrid("ScoreArcTree");
        if (!kicp_grid_has_plan(grid)) throw std::runtime_error("KinematicICP::ScoreArcTree: call GridPotential first (or GridPotentialOfCostmap): the grid holds no plan");
        results.resize(kicp_bridge::arc_tree_nodes(tree).n_nodes);
        kicp_bridge::check(kicp_grid_score_arc_tree(grid, start.data(), static_cast<unsigned int>(tree.branch.size()), tree.branch.data(), tree.steps.data(),
                                                    tree.primitives.front().data(), footprint.empty() ? nullptr : footprint.front().data(), footprint.size(),
                                                    results.front().data(), 4 * results.size()),
                           "ScoreArcTree");
    }
    // the same from a pose - pose() for the robot as it stands
    void ScoreArcTree(std::vector<kicp_bridge::ArcResult> &results, const Sophus::SE3d &pose, const kicp_bridge::ArcTree &tree,
                      const std::vector<kicp_bridge::FootprintSample> &footprint) const {
        ScoreArcTree(results, kicp_bridge::arc_start(pose), tree, footprint);
    }
    kicp_bridge::ArcTreeLeaf BestArcTreeLeaf(const std::vector<kicp_bridge::ArcResult> &results, const kicp_bridge::ArcTree &tree, unsigned int w_potential = 1,
                                             unsigned int w_cost = 0, unsigned int w_blocked = 0, unsigned int min_free_steps = 1) const {
        return kicp_bridge::best_arc_tree_leaf(results, tree, w_potential, w_cost, w_blocked, min_free_steps);
    }
    // Where to go while mapping (kicp.h kicp_grid_frontiers): the frontiers of the grid as it stands - the clear cells with an unknown
    // edge neighbour, joined over their eight neighbours - found on the GPU from the counters, those of at least config.min_size cells
    // in ascending label order.  With use_plan, best_potential and best_cell come from the plan the last GridPotential or
    // GridPotentialOfCostmap left on the GPU: with the robot's cell as that call's one goal they are the cost of driving to the frontier
    // and the cell to drive to - PotentialPath from best_cell leads down to the robot; reverse it.  The plan is a snapshot, the
    // frontiers are the current counters'; neither is changed.  labels (nullable): width * height words, the label on every frontier
    // cell and 0xFFFFFFFF elsewhere.  Throws without a grid, and with use_plan without a plan ("call GridPotential first").
    void GridFrontiers(std::vector<kicp_bridge::Frontier> &frontiers, const kicp_bridge::FrontierConfig &config, bool use_plan = false,
                       std::vector<uint32_t> *labels = nullptr) const {
        const kicp_bridge::GridRect r = GridRectOrAll(nullptr, "GridFrontiers");
        if (use_plan && !kicp_grid_has_plan(grid_.get()))
            throw std::runtime_error("KinematicICP::GridFrontiers: call GridPotential first (or GridPotentialOfCostmap): the grid holds no plan");
        if (labels) labels->resize(static_cast<size_t>(r.w) * r.h);
        std::vector<unsigned long long> rows(256 * static_cast<size_t>(KICP_FRONTIER_WORDS));
        size_t n = 0;
        auto call = [&] {
            return kicp_grid_frontiers(grid_.get(), &config, use_plan ? 1 : 0, rows.data(), rows.size() / KICP_FRONTIER_WORDS, &n, labels ? labels->data() : nullptr,
                                       labels ? labels->size() : 0);
        };
        int rc = call();
        if (rc == KICP_ERR_CAPACITY && n > rows.size() / KICP_FRONTIER_WORDS) {  // more frontiers than that: their number came back
            rows.resize(n * KICP_FRONTIER_WORDS);
            rc = call();
        }
        kicp_bridge::check(rc, "GridFrontiers");
        frontiers.resize(n);
        for (size_t i = 0; i < n; ++i) frontiers[i] = kicp_bridge::frontier_of_row(rows.data() + i * KICP_FRONTIER_WORDS);
    }
    // What stands in known free space right now (kicp.h kicp_grid_transients): while enabled, RegisterFrame and its variants run the
    // detection on the frame they return, at the new pose, immediately before that frame is integrated into the grid - from HBM on the
    // chained path, from the host points on the other - so the counters it is judged by do not hold its own hits yet.  Transients() are
    // the last frame's, of at least config.min_size cells in ascending label order.  With as_sources the grid's switch is raised: the
    // cells of those transients are sources in GridClearance, GridCostmap and GridPotential until the next frame replaces them, while
    // GridOccupancy, GridFrontiers, GridGain and SaveGrid never see them.  Poses, clouds, the map and the grid's counters are what they
    // are without it.  A copied pipeline copies the switch and the configuration and starts with an empty plane.  Throws without a grid.
    void EnableTransients(const kicp_bridge::TransientConfig &config, bool as_sources = true) {
        kicp_grid *grid = MutableGrid("EnableTransients");
        size_t n = 0;
        const double pose[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, sensor[3] = {0.0, 0.0, 0.0};
        kicp_bridge::check(kicp_grid_transients(grid, nullptr, 0, pose, sensor, &config, nullptr, 0, &n, nullptr, 0, nullptr), "EnableTransients");  // (checks config)
        kicp_bridge::check(kicp_grid_use_transients(grid, as_sources ? 1 : 0), "EnableTransients");
        transient_config_ = config, transients_enabled_ = true, last_transients_.clear();
    }
    // empties the plane and lowers the switch; without a grid there is nothing to do
    void DisableTransients() {
        if (grid_ && transients_enabled_) {
            size_t n = 0;
            const double pose[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, sensor[3] = {0.0, 0.0, 0.0};
            kicp_bridge::check(kicp_grid_transients(grid_.get(), nullptr, 0, pose, sensor, &transient_config_, nullptr, 0, &n, nullptr, 0, nullptr), "DisableTransients");
            kicp_bridge::check(kicp_grid_use_transients(grid_.get(), 0), "DisableTransients");
        }
        transients_enabled_ = false, last_transients_.clear();
    }
    bool TransientsEnabled() const { return transients_enabled_; }
    const std::vector<kicp_bridge::Transient> &Transients() const { return last_transients_; }
    // the plane of the last frame's transients, a byte per cell: what GridCostmap treats as lethal while the switch is on
    void TransientPlane(std::vector<uint8_t> &plane) const {
        const kicp_bridge::GridRect r = GridRectOrAll(nullptr, "TransientPlane");
        plane.resize(static_cast<size_t>(r.w) * r.h);
        kicp_bridge::check(kicp_grid_transient_plane(grid_.get(), plane.data(), plane.size()), "TransientPlane");
    }
    // What the robot would see from there (kicp.h kicp_grid_gain): per candidate viewpoint - a cell index y * width + x, such as the
    // best_cell of GridFrontiers' frontiers under a plan - the distinct unknown cells a sensor of config.range_cells' range (1 .. 361)
    // would see, on the GPU from the counters: 8 R rays per viewpoint, cut to the disc, stopped by occupied cells and by the grid's
    // edge, not by unknown ones.  An exploration node ranks its frontiers by out[i].seen against best_potential, the cost of driving
    // there; the weighting is the caller's.  Neither the counters nor the plan are changed.  Throws without a grid, and for a cell
    // index outside it.
    void GridGain(const std::vector<unsigned int> &cells, const kicp_bridge::GainConfig &config, std::vector<kicp_bridge::Gain> &out) const {
        const kicp_grid *grid = RequireGrid("GridGain");
        std::vector<unsigned int> rows(cells.size() * static_cast<size_t>(KICP_GAIN_WORDS));
        kicp_bridge::check(kicp_grid_gain(grid, &config, cells.data(), cells.size(), rows.data(), rows.size()), "GridGain");
        out.resize(cells.size());
        for (size_t i = 0; i < cells.size(); ++i) out[i] = kicp_bridge::gain_of_row(rows.data() + i * KICP_GAIN_WORDS);
    }
    // the window of the last integrated frame clipped to the grid; empty() when it lies outside, and before any frame
    kicp_bridge::GridRect GridLastWindow() const {
        kicp_bridge::GridRect r;
        kicp_bridge::check(kicp_grid_last_window(RequireGrid("GridLastWindow"), &r.x0, &r.y0, &r.w, &r.h), "GridLastWindow");
        return r;
    }
    // <prefix>.pgm + <prefix>.yaml, the pair map_server and Nav2 read
    void SaveGrid(const std::string &prefix, unsigned int min_observations = 1, double occupied_thresh = 0.65, double free_thresh = 0.25) const {
        kicp_bridge::check(kicp_grid_save_map(RequireGrid("SaveGrid"), prefix.c_str(), min_observations, occupied_thresh, free_thresh), "SaveGrid");
    }

    // ---- backend extension: uneven ground (INTEGRATION.md "Uneven ground: height columns") ----
    // With the height columns enabled, RegisterFrame, RegisterIngestedFrame and their F32 variants integrate the frame they return into a
    // layer of one 64-bit column per cell - which world heights ever returned there - exactly where and as the occupancy grid gets it:
    // after the registration, at the new pose, with the translation of lidar_to_base as the sensor (kicp.h kicp_elev_*, which also states
    // the layer's known limitations).  Poses, thresholds, returned clouds, the map and the grid are what they are without it.
    // Elevation() is the shared handle (null without a layer): kicp_elev_to_grid(Elevation().get(), &config, planner_grid.get()) puts the
    // traversability into a grid a node dedicates to its planner, and kicp_elev_to_grid_slope(Elevation().get(), &config, &slope,
    // planner_grid.get()) the traversability with the slope limit.  LastElevationStats(): used, skipped, outside_grid, outside_column,
    // new_bits, new_cells of the last frame (zeros before the first).
    void EnableElevation(const kicp_bridge::ElevationConfig &config) {
        elev_ = kicp_bridge::make_elevation(config), last_elev_stats_ = {}, elev_follow_ = {}, DisableElevationCarving();
    }
    void DisableElevation() { elev_.reset(), last_elev_stats_ = {}, elev_follow_ = {}, DisableElevationCarving(); }
    // FOLLOWING for the layer, as EnableGridFollow for the grid (kicp.h kicp_elev_follow; off by default, a new layer starts with it
    // off).  A planner grid fed by kicp_elev_to_grid* is scrolled by its owner, by LastElevationScroll().
    void EnableElevationFollow(unsigned int margin_cells, unsigned int step_cells) {
        kicp_elev_config config{};
        kicp_bridge::check(kicp_elev_info(RequireElevation("EnableElevationFollow"), &config, nullptr, nullptr), "EnableElevationFollow");
        elev_follow_ = kicp_bridge::make_follow(config.width, config.height, margin_cells, step_cells, "KinematicICP::EnableElevationFollow");
    }
    void DisableElevationFollow() { elev_follow_ = {}; }
    bool ElevationFollowEnabled() const { return elev_follow_.enabled; }
    std::array<int, 2> LastElevationScroll() const { return elev_follow_.last; }
    std::shared_ptr<kicp_elev> Elevation() const { return elev_; }
    const kicp_bridge::ElevationStats &LastElevationStats() const { return last_elev_stats_; }
    // CARVING (off by default; a new layer starts with it off).  With it on, a frame goes into the layer as an UPDATE (kicp.h
    // kicp_elev_update): the bits its rays pass through are cleared, then the frame is marked, so what has left - a passer-by - leaves
    // the traversability too.  The configuration is checked here (std::invalid_argument).  LastElevationCarveStats(): the nine words of
    // the last update - LastElevationStats()'s six, counted on the carved columns, then carve_points, bits_cleared, cells_emptied
    // (zeros before the first, and while carving is off).
    void EnableElevationCarving(const kicp_bridge::ElevationCarveConfig &config) {
        RequireElevation("EnableElevationCarving");
        if (config.widen_slabs > 64u || config.keep_ground > 1u)
            throw std::invalid_argument("KinematicICP::EnableElevationCarving: widen_slabs must lie in 0 .. 64 and keep_ground must be 0 or 1");
        elev_carving_ = true, elev_carve_ = config, last_elev_carve_stats_ = {};
    }
    void DisableElevationCarving() { elev_carving_ = false, elev_carve_ = {}, last_elev_carve_stats_ = {}; }
    bool ElevationCarving() const { return elev_carving_; }
    const kicp_bridge::ElevationCarveStats &LastElevationCarveStats() const { return last_elev_carve_stats_; }
    // -1 unknown, 0 traversable, 100 obstacle per cell of `rect` (nullptr: the full layer), row-major; ground (nullable): the ground's
    // slab per cell, 255 unknown; counts (nullable): unknown, traversable, BODY, STEP only.  The result for a rectangle equals the full
    // layer's restricted to it; a frame changes it only inside ElevationLastWindow() grown by one cell.
    void ElevationTraversability(const kicp_bridge::ElevationTraversabilityConfig &config, std::vector<int8_t> &data, const kicp_bridge::GridRect *rect = nullptr,
                                 std::vector<uint8_t> *ground = nullptr, std::array<unsigned long long, 4> *counts = nullptr) const {
        kicp_bridge::GridRect r;
        if (rect) {
            r = *rect;
        } else {
            kicp_elev_config layer{};
            kicp_bridge::check(kicp_elev_info(RequireElevation("ElevationTraversability"), &layer, nullptr, nullptr), "ElevationTraversability");
            r.w = layer.width, r.h = layer.height;
        }
        data.resize(static_cast<size_t>(r.w) * r.h);
        if (ground) ground->resize(data.size());
        kicp_bridge::check(kicp_elev_traversability(RequireElevation("ElevationTraversability"), &config, r.x0, r.y0, r.w, r.h, reinterpret_cast<signed char *>(data.data()),
                                                    ground ? ground->data() : nullptr, counts ? counts->data() : nullptr, data.size()),
                           "ElevationTraversability");
    }
    // The same with the slope limit (kicp.h THE SLOPE LIMIT): a cell is also an obstacle when a least-squares plane through the known
    // grounds of its window is steeper than slope.rise_slabs slabs per slope.run_cells cells.  counts (nullable): unknown, traversable,
    // BODY, STEP only, SLOPE only; fit (nullable): D, Da, Db per cell, zeros without a fit.  A frame changes the result only inside
    // ElevationLastWindow() grown by max(1, slope.radius_cells) cells.  A bad configuration: std::runtime_error from the library's check.
    void ElevationTraversabilitySlope(const kicp_bridge::ElevationTraversabilityConfig &config, const kicp_bridge::ElevationSlopeConfig &slope, std::vector<int8_t> &data,
                                      const kicp_bridge::GridRect *rect = nullptr, std::vector<uint8_t> *ground = nullptr,
                                      std::array<unsigned long long, KICP_ELEV_SLOPE_COUNTS> *counts = nullptr, std::vector<long long> *fit = nullptr) const {
        const kicp_elev *elev = RequireElevation("ElevationTraversabilitySlope");
        kicp_bridge::GridRect r;
        if (rect) {
            r = *rect;
        } else {
            kicp_elev_config layer{};
            kicp_bridge::check(kicp_elev_info(elev, &layer, nullptr, nullptr), "ElevationTraversabilitySlope");
            r.w = layer.width, r.h = layer.height;
        }
        data.resize(static_cast<size_t>(r.w) * r.h);
        if (ground) ground->resize(data.size());
        if (fit) fit->resize(3 * data.size());
        kicp_bridge::check(kicp_elev_traversability_slope(elev, &config, &slope, r.x0, r.y0, r.w, r.h, reinterpret_cast<signed char *>(data.data()),
                                                          ground ? ground->data() : nullptr, fit ? fit->data() : nullptr, counts ? counts->data() : nullptr, data.size()),
                           "ElevationTraversabilitySlope");
    }
    // the slope limit of a tangent on this layer's cell and slab (kicp_elev_slope_limit): rise_slabs and run_cells of `slope` are set
    kicp_bridge::ElevationSlopeConfig ElevationSlopeLimit(double max_tangent, kicp_bridge::ElevationSlopeConfig slope = {4u, 6u, 12u, 0u, 1u}) const {
        kicp_elev_config layer{};
        kicp_bridge::check(kicp_elev_info(RequireElevation("ElevationSlopeLimit"), &layer, nullptr, nullptr), "ElevationSlopeLimit");
        kicp_bridge::check(kicp_elev_slope_limit(&layer, max_tangent, &slope.rise_slabs, &slope.run_cells), "ElevationSlopeLimit");
        return slope;
    }
    // The same with the class ROUGH (kicp.h ROUGH): a cell with a fit is also an obstacle when the mean squared residual of its fit set to
    // the fitted plane exceeds rough.num / rough.den slabs^2.  counts (nullable): unknown, traversable, BODY, STEP only, SLOPE only, ROUGH
    // only; fit (nullable): D, Da, Db, Q, n per cell, zeros without a fit.  The window rule and the errors are the slope entry's.
    void ElevationTraversabilityRough(const kicp_bridge::ElevationTraversabilityConfig &config, const kicp_bridge::ElevationSlopeConfig &slope,
                                      const kicp_bridge::ElevationRoughConfig &rough, std::vector<int8_t> &data, const kicp_bridge::GridRect *rect = nullptr,
                                      std::vector<uint8_t> *ground = nullptr, std::array<unsigned long long, KICP_ELEV_ROUGH_COUNTS> *counts = nullptr,
                                      std::vector<long long> *fit = nullptr) const {
        const kicp_elev *elev = RequireElevation("ElevationTraversabilityRough");
        kicp_bridge::GridRect r;
        if (rect) {
            r = *rect;
        } else {
            kicp_elev_config layer{};
            kicp_bridge::check(kicp_elev_info(elev, &layer, nullptr, nullptr), "ElevationTraversabilityRough");
            r.w = layer.width, r.h = layer.height;
        }
        data.resize(static_cast<size_t>(r.w) * r.h);
        if (ground) ground->resize(data.size());
        if (fit) fit->resize(5 * data.size());
        kicp_bridge::check(kicp_elev_traversability_rough(elev, &config, &slope, &rough, r.x0, r.y0, r.w, r.h, reinterpret_cast<signed char *>(data.data()),
                                                          ground ? ground->data() : nullptr, fit ? fit->data() : nullptr, counts ? counts->data() : nullptr, data.size()),
                           "ElevationTraversabilityRough");
    }
    // the ROUGH limit of an r.m.s. residual in metres on this layer's slab (kicp_elev_rough_limit)
    kicp_bridge::ElevationRoughConfig ElevationRoughLimit(double rms_metres) const {
        kicp_elev_config layer{};
        kicp_bridge::ElevationRoughConfig rough{};
        kicp_bridge::check(kicp_elev_info(RequireElevation("ElevationRoughLimit"), &layer, nullptr, nullptr), "ElevationRoughLimit");
        kicp_bridge::check(kicp_elev_rough_limit(&layer, rms_metres, &rough.num, &rough.den), "ElevationRoughLimit");
        return rough;
    }
    // A node's call after a frame: the layer's classes into the grid it dedicates to its planner (same cell, origin, width and height as
    // the layer, same device) - kicp_elev_to_grid without `slope`, kicp_elev_to_grid_slope with it, kicp_elev_to_grid_rough with `slope`
    // and `rough` (`rough` without `slope`: std::invalid_argument) -, and with `fill` the cells the layer does not know from the
    // pipeline's own occupancy grid (kicp_grid_fill_unknown; needs EnableGrid), whose seven words go to fill_counts (nullable).  Never
    // called inside RegisterFrame: the node decides when it plans.
    void ElevationIntoGrid(kicp_grid *planner_grid, const kicp_bridge::ElevationTraversabilityConfig &config, const kicp_bridge::ElevationSlopeConfig *slope = nullptr,
                           const kicp_bridge::ElevationRoughConfig *rough = nullptr, const kicp_bridge::GridFillConfig *fill = nullptr,
                           kicp_bridge::GridFillCounts *fill_counts = nullptr) const {
        const kicp_elev *elev = RequireElevation("ElevationIntoGrid");
        if (rough && !slope) throw std::invalid_argument("KinematicICP::ElevationIntoGrid: rough needs slope - ROUGH is the residual of the slope limit's fit");
        const kicp_grid *source = fill ? RequireGrid("ElevationIntoGrid") : nullptr;
        if (rough)
            kicp_bridge::check(kicp_elev_to_grid_rough(elev, &config, slope, rough, planner_grid), "ElevationIntoGrid");
        else if (slope)
            kicp_bridge::check(kicp_elev_to_grid_slope(elev, &config, slope, planner_grid), "ElevationIntoGrid");
        else
            kicp_bridge::check(kicp_elev_to_grid(elev, &config, planner_grid), "ElevationIntoGrid");
        if (fill) kicp_bridge::check(kicp_grid_fill_unknown(planner_grid, source, fill, fill_counts ? fill_counts->data() : nullptr), "ElevationIntoGrid");
    }
    // the window of the last integrated frame clipped to the layer; empty() when it lies outside, and before any frame
    kicp_bridge::GridRect ElevationLastWindow() const {
        kicp_bridge::GridRect r;
        kicp_bridge::check(kicp_elev_last_window(RequireElevation("ElevationLastWindow"), &r.x0, &r.y0, &r.w, &r.h), "ElevationLastWindow");
        return r;
    }

    // ---- backend extension: keeping moving things out of the map (INTEGRATION.md "Keeping moving things out of the map") ----
    // With see-through removal enabled, RegisterFrame, RegisterIngestedFrame and their F32 variants render the frame they return - the
    // deskewed, cropped frame in the base frame, all of it - into a depth view at the new pose, with the translation of lidar_to_base
    // as the sensor, and remove the map points that frame sees through (kicp.h kicp_view_*, kicp_map_remove_seen_through) - after the
    // pose is known and BEFORE the frame's own points go into the map.  The pose of THIS frame and the returned clouds are what they
    // are without it; the map, and with it later poses, differ by the removed points.  With Config::update_map == false the map is a
    // prior and nothing is removed.  LastRemoval(): points in range, points removed, voxels that lost at least one point, voxels
    // erased of the last frame (zeros before the first, and when the removal was skipped).
    void EnableSeeThroughRemoval(const kicp_bridge::ViewConfig &config) { view_ = kicp_bridge::make_view(config), last_removal_ = {}; }
    void DisableSeeThroughRemoval() { view_.reset(), last_removal_ = {}; }
    std::shared_ptr<kicp_view> View() const { return view_; }
    const std::array<unsigned long long, 4> &LastRemoval() const { return last_removal_; }

    std::vector<Eigen::Vector3d> LocalMap() const { return local_map_.Pointcloud(); }
    const kiss_icp::VoxelHashMap &VoxelMap() const { return local_map_; }
    kiss_icp::VoxelHashMap &VoxelMap() { return local_map_; }
    const Sophus::SE3d &pose() const { return last_pose_; }
    Sophus::SE3d &pose() { return last_pose_; }

protected:
    const kicp_grid *RequireGrid(const char *who) const {
        if (!grid_) throw std::runtime_error(std::string("KinematicICP::") + who + ": call EnableGrid first");
        return grid_.get();
    }
    kicp_grid *MutableGrid(const char *who) {
        if (!grid_) throw std::runtime_error(std::string("KinematicICP::") + who + ": call EnableGrid first");
        return grid_.get();
    }
    const kicp_elev *RequireElevation(const char *who) const {
        if (!elev_) throw std::runtime_error(std::string("KinematicICP::") + who + ": call EnableElevation first");
        return elev_.get();
    }
    kicp_bridge::GridRect GridRectOrAll(const kicp_bridge::GridRect *rect, const char *who) const {
        if (rect) return RequireGrid(who), *rect;
        kicp_grid_config config{};
        kicp_bridge::check(kicp_grid_info(RequireGrid(who), &config, nullptr, nullptr), who);
        kicp_bridge::GridRect all;
        all.w = config.width, all.h = config.height;
        return all;
    }
    // one frame into the grid at last_pose_ (already the new pose), from HBM or from host memory
    // the grid and the layer follow the new pose's translation, where following is on
    void FollowPose() {
        const Eigen::Vector3d at = last_pose_.translation();
        if (grid_ && grid_follow_.enabled)
            kicp_bridge::check(kicp_grid_follow(grid_.get(), at.x(), at.y(), grid_follow_.margin_cells, grid_follow_.step_cells, &grid_follow_.last[0], &grid_follow_.last[1]),
                               "KinematicICP: following with the grid");
        if (elev_ && elev_follow_.enabled)
            kicp_bridge::check(kicp_elev_follow(elev_.get(), at.x(), at.y(), elev_follow_.margin_cells, elev_follow_.step_cells, &elev_follow_.last[0], &elev_follow_.last[1]),
                               "KinematicICP: following with the height layer");
    }
    void IntegrateGrid(const double *xyz, size_t n, bool on_device) {
        double pose[7];
        kicp_bridge::to_params(last_pose_, pose);
        const double sensor[3] = {sensor_in_base_.x(), sensor_in_base_.y(), sensor_in_base_.z()};
        kicp_bridge::check(on_device ? kicp_grid_integrate_device(grid_.get(), xyz, n, pose, sensor, nullptr) : kicp_grid_integrate(grid_.get(), xyz, n, pose, sensor, nullptr),
                           "occupancy grid");
    }
    // the transients of one frame at last_pose_ (already the new pose) against the counters as they stand, from HBM or from host memory
    void DetectTransients(const double *xyz, size_t n_points, bool on_device) {
        double pose[7];
        kicp_bridge::to_params(last_pose_, pose);
        const double sensor[3] = {sensor_in_base_.x(), sensor_in_base_.y(), sensor_in_base_.z()};
        transient_rows_.resize(std::max<size_t>(transient_rows_.size(), 64 * static_cast<size_t>(KICP_TRANSIENT_WORDS)));
        size_t n = 0;
        auto call = [&] {
            const size_t cap = transient_rows_.size() / KICP_TRANSIENT_WORDS;
            return on_device ? kicp_grid_transients_device(grid_.get(), xyz, n_points, pose, sensor, &transient_config_, transient_rows_.data(), cap, &n, nullptr, 0, nullptr)
                             : kicp_grid_transients(grid_.get(), xyz, n_points, pose, sensor, &transient_config_, transient_rows_.data(), cap, &n, nullptr, 0, nullptr);
        };
        int rc = call();
        if (rc == KICP_ERR_CAPACITY && n > transient_rows_.size() / KICP_TRANSIENT_WORDS) {  // more transients than that: their number came back
            transient_rows_.resize(n * KICP_TRANSIENT_WORDS);
            rc = call();
        }
        kicp_bridge::check(rc, "transients");
        last_transients_.resize(n);
        for (size_t i = 0; i < n; ++i) last_transients_[i] = kicp_bridge::transient_of_row(transient_rows_.data() + i * KICP_TRANSIENT_WORDS);
    }
    // one frame into the height columns at last_pose_ (already the new pose), from HBM or from host memory
    void IntegrateElevation(const double *xyz, size_t n, bool on_device) {
        double pose[7];
        kicp_bridge::to_params(last_pose_, pose);
        const double sensor[3] = {sensor_in_base_.x(), sensor_in_base_.y(), sensor_in_base_.z()};
        if (elev_carving_) {
            unsigned long long *stats = last_elev_carve_stats_.data();
            kicp_bridge::check(on_device ? kicp_elev_update_device(elev_.get(), xyz, n, pose, sensor, &elev_carve_, stats)
                                         : kicp_elev_update(elev_.get(), xyz, n, pose, sensor, &elev_carve_, stats),
                               "height columns");
            std::copy(stats, stats + KICP_ELEV_STATS, last_elev_stats_.begin());
            return;
        }
        unsigned long long *stats = last_elev_stats_.data();
        kicp_bridge::check(on_device ? kicp_elev_integrate_device(elev_.get(), xyz, n, pose, sensor, stats) : kicp_elev_integrate(elev_.get(), xyz, n, pose, sensor, stats),
                           "height columns");
    }
    // the frame into the depth view at the new pose, from HBM or from host memory; then the sweep of the map
    void RemoveSeenThrough(const double *xyz, size_t n, bool on_device, const Sophus::SE3d &new_pose) {
        double pose[7];
        kicp_bridge::to_params(new_pose, pose);
        const double sensor[3] = {sensor_in_base_.x(), sensor_in_base_.y(), sensor_in_base_.z()};
        kicp_bridge::check(on_device ? kicp_view_render_device(view_.get(), xyz, n, pose, sensor, nullptr) : kicp_view_render(view_.get(), xyz, n, pose, sensor, nullptr),
                           "depth view");
        last_removal_ = local_map_.RemoveSeenThrough(view_.get());
    }
#ifndef KICP_HOST_PRESTEPS
    // From the moment the backend's helper thread holds a pointer into the result's frame vector: should any later step throw,
    // the download is collected (and dropped) before the vector is destroyed, so nothing is ever copied into freed memory.
    struct DownloadGuard {
        kicp_pre *pre;
        bool armed = true;  // (false: nothing was pushed)
        ~DownloadGuard() {
            if (armed) (void)kicp_pre_download_finish(pre, 0, nullptr, 0, nullptr);
        }
    };
    // pipeline/KinematicICP.cpp:65-84 from the pre-steps' three buffers on (0: preprocessed frame, 1: first downsample - what goes
    // into the map, 2: second downsample - the registration source): register, update the threshold and the map - all on the
    // device; only the two returned clouds come back to the host.
    // register, update the threshold, begin the map update (shared by the fp64 and the FLOAT32 entries)
    void RegisterOnDevice(kicp_bridge::Trace &trace, const size_t counts[3], const Sophus::SE3d &relative_odometry) {
        const size_t n_down = counts[1], n_source = counts[2];
        const double tau = correspondence_threshold_.ComputeThreshold();
        const auto new_pose = registration_.ComputeRobotMotionDevice(kicp_pre_device_ptr(pre_, 2, nullptr), n_source, local_map_, last_pose_,
                                                                     relative_odometry, tau);
        trace.lap("threshold + map update");
        correspondence_threshold_.UpdateOdometryError((last_pose_ * relative_odometry).inverse() * new_pose);
        // see-through removal, when enabled: the whole preprocessed frame (buffer 0, complete since the pre-steps returned) is rendered at
        // the new pose and the map swept against it, before the frame's own points go in
        if (view_ && config_.update_map) RemoveSeenThrough(kicp_pre_device_ptr(pre_, 0, nullptr), counts[0], true, new_pose);
        // (the map update's kernels run while this thread collects the two returned clouds: nothing below touches the map or buffer 1)
        if (config_.update_map) local_map_.UpdateDeviceBegin(kicp_pre_device_ptr(pre_, 1, nullptr), n_down, new_pose);
        last_pose_ = new_pose;
        // the occupancy grid, when enabled: the whole preprocessed frame (buffer 0, complete since the pre-steps returned) at the new pose
        // following, when enabled: the grid and the layer scroll towards the new pose before the frame goes into them
        FollowPose();
        // the transients, when enabled: the same frame against the counters as they stand, before its own hits go into them
        if (grid_ && transients_enabled_) DetectTransients(kicp_pre_device_ptr(pre_, 0, nullptr), counts[0], true);
        if (grid_) IntegrateGrid(kicp_pre_device_ptr(pre_, 0, nullptr), counts[0], true);
        // the height columns, when enabled: the same frame at the same pose
        if (elev_) IntegrateElevation(kicp_pre_device_ptr(pre_, 0, nullptr), counts[0], true);
    }
    Vector3dVectorTuple RegisterChained(Vector3dVectorTuple &result, DownloadGuard &guard, const size_t counts[3], const Sophus::SE3d &relative_odometry) {
        kicp_bridge::Trace trace("registration");
        auto &frame = std::get<0>(result);
        const size_t n_source = counts[2];
        RegisterOnDevice(trace, counts, relative_odometry);
        trace.lap("collect results");
        auto &source = std::get<1>(result);
        source.resize(n_source);
        kicp_bridge::check(kicp_pre_download(pre_, 2, source.empty() ? nullptr : source.front().data(), source.size(), nullptr), "download");
        guard.armed = false;
        if (!frame.empty()) kicp_bridge::check(kicp_pre_download_finish(pre_, 0, frame.front().data(), frame.size(), nullptr), "download");
        frame.resize(counts[0]);  // (the landing area held every input point; shrinking costs nothing)
        // The map update's kernels are still running: whatever touches the map next - the next frame's registration, LocalMap(),
        // VoxelMap() - collects them first (kicp.h: kicp_map_update_pose_device_begin), so they overlap the caller's own work and the
        // next frame's pre-steps instead of this thread's idle wait (round 6; the points they read stay in the pre-step workspace's
        // spare buffer meanwhile).  KICP_SYNC_MAP_UPDATE=1: wait here, as round 5 did.
        static const bool sync_update = [] { const char *e = std::getenv("KICP_SYNC_MAP_UPDATE"); return e && *e && *e != '0'; }();
        if (sync_update && config_.update_map) {
            trace.lap("map update: wait");
            local_map_.UpdateFinish();
        }
        return std::move(result);  // built in place: no copy of the clouds on the way out
    }
    // the frame's records land in `data` (room for every input point; shrunk to the frame afterwards); nullptr: no frame wanted
    static float *LandFrame(std::vector<uint8_t> *data, size_t n_in) {
        if (!data) return nullptr;
        data->resize(n_in * kicp_bridge::PointCloud2Xyz32::point_step);
        return n_in ? reinterpret_cast<float *>(data->data()) : nullptr;
    }
    void RegisterChainedF32(DownloadGuard &guard, const size_t counts[3], const Sophus::SE3d &relative_odometry, std::vector<uint8_t> *frame_data,
                            std::vector<uint8_t> *keypoints_data) {
        kicp_bridge::Trace trace("registration");
        RegisterOnDevice(trace, counts, relative_odometry);
        trace.lap("collect results");
        constexpr size_t step = kicp_bridge::PointCloud2Xyz32::point_step;
        if (keypoints_data) {
            keypoints_data->resize(counts[2] * step);
            kicp_bridge::check(kicp_pre_download_f32(pre_, 2, counts[2] ? reinterpret_cast<float *>(keypoints_data->data()) : nullptr, counts[2], nullptr),
                               "download");
        }
        if (guard.armed) {
            guard.armed = false;
            kicp_bridge::check(kicp_pre_download_finish(pre_, 0, nullptr, 0, nullptr), "download");
        }
        if (frame_data) frame_data->resize(counts[0] * step);
        static const bool sync_update = [] { const char *e = std::getenv("KICP_SYNC_MAP_UPDATE"); return e && *e && *e != '0'; }();
        if (sync_update && config_.update_map) {
            trace.lap("map update: wait");
            local_map_.UpdateFinish();
        }
    }
#endif
    Sophus::SE3d last_pose_;
    KinematicRegistration registration_;
    CorrespondenceThreshold correspondence_threshold_;
    Config config_;
    kiss_icp::Preprocessor preprocessor_;
    kiss_icp::VoxelHashMap local_map_;
    kicp_pre *pre_ = nullptr;  // device workspace of the pre-steps (backend detail)
    std::shared_ptr<kicp_occ> occupancy_;  // BuildOccupancy's snapshot of the map (backend detail)
    std::shared_ptr<kicp_grid> grid_;      // EnableGrid's occupancy grid (backend detail); null: no grid
    bool transients_enabled_ = false;      // EnableTransients: every frame is searched for transients before it goes into the grid
    kicp_bridge::TransientConfig transient_config_{};
    std::vector<kicp_bridge::Transient> last_transients_;  // the last frame's
    std::vector<unsigned long long> transient_rows_;       // where their rows land (scratch that keeps its size)
    kicp_bridge::Follow grid_follow_;      // EnableGridFollow: the grid scrolls after the robot
    std::shared_ptr<kicp_elev> elev_;      // EnableElevation's height columns (backend detail); null: no layer
    kicp_bridge::Follow elev_follow_;      // EnableElevationFollow: the layer does
    kicp_bridge::ElevationStats last_elev_stats_{};  // the last frame's statistics of that layer
    bool elev_carving_ = false;                      // EnableElevationCarving: frames go into the layer as updates
    kicp_bridge::ElevationCarveConfig elev_carve_{};
    kicp_bridge::ElevationCarveStats last_elev_carve_stats_{};  // the last update's nine words
    std::shared_ptr<kicp_view> view_;      // EnableSeeThroughRemoval's depth view (backend detail); null: nothing is removed
    std::array<unsigned long long, 4> last_removal_{};  // the last frame's sweep statistics
    Eigen::Vector3d sensor_in_base_ = Eigen::Vector3d(0.0, 0.0, 0.0);  // the translation of the last frame's lidar_to_base
};

}  // namespace kinematic_icp::pipeline
