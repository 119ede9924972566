// kinematic_icp/registration/Registration.hpp -- drop-in for the reference header of the same path
// (/root/reference/cpp/kinematic_icp/registration/Registration.hpp:23-51): same struct, constructor signature,
// ComputeRobotMotion signature and public fields; the body runs on the MI355X through include/kicp.h.
#pragma once
#include <Eigen/Core>
#include <kiss_icp/core/VoxelHashMap.hpp>
#include <sophus/se3.hpp>
#include <utility>
#include <vector>

#include "kicp_bridge.hpp"

namespace kinematic_icp {
struct KinematicRegistration {
    explicit KinematicRegistration(const int max_num_iteration, const double convergence_criterion, const int max_num_threads,
                                   const bool use_adaptive_odometry_regularization, const double fixed_regularization)
        : max_num_iterations_(max_num_iteration),
          convergence_criterion_(convergence_criterion),
          // Registration.cpp:141-142: "only manipulate the number of threads if the user specifies something greater than 0", else
          // tbb::this_task_arena::max_concurrency() = the hardware threads this process may use.  The field reads like the
          // reference's; the GPU path itself has no host thread pool to size with it.
          max_num_threads_(max_num_threads > 0 ? max_num_threads : kicp_bridge::hardware_threads()),
          use_adaptive_odometry_regularization_(use_adaptive_odometry_regularization),
          fixed_regularization_(fixed_regularization) {
        const kicp_reg_config c = config();
        kicp_bridge::check(kicp_reg_create(&c, device_, &handle_), "KinematicRegistration");
    }
    ~KinematicRegistration() { kicp_reg_destroy(handle_); }
    // copyable and movable like the reference's struct (a plain aggregate of five parameters, Registration.hpp:32-50): a copy has
    // the same parameters and backend options and device workspaces of its own (kicp_reg_clone)
    KinematicRegistration(const KinematicRegistration &o)
        : max_num_iterations_(o.max_num_iterations_),
          convergence_criterion_(o.convergence_criterion_),
          max_num_threads_(o.max_num_threads_),
          use_adaptive_odometry_regularization_(o.use_adaptive_odometry_regularization_),
          fixed_regularization_(o.fixed_regularization_),
          device_(o.device_),
          last_stats_(o.last_stats_) {
        kicp_bridge::check(kicp_reg_clone(o.handle_, &handle_), "KinematicRegistration(const KinematicRegistration&)");
    }
    KinematicRegistration(KinematicRegistration &&o) noexcept
        : max_num_iterations_(o.max_num_iterations_),
          convergence_criterion_(o.convergence_criterion_),
          max_num_threads_(o.max_num_threads_),
          use_adaptive_odometry_regularization_(o.use_adaptive_odometry_regularization_),
          fixed_regularization_(o.fixed_regularization_),
          device_(o.device_),
          handle_(o.handle_),
          last_stats_(o.last_stats_) {
        o.handle_ = nullptr;
    }
    KinematicRegistration &operator=(KinematicRegistration o) noexcept {  // copy / move and swap
        std::swap(max_num_iterations_, o.max_num_iterations_), std::swap(convergence_criterion_, o.convergence_criterion_);
        std::swap(max_num_threads_, o.max_num_threads_), std::swap(use_adaptive_odometry_regularization_, o.use_adaptive_odometry_regularization_);
        std::swap(fixed_regularization_, o.fixed_regularization_), std::swap(device_, o.device_), std::swap(handle_, o.handle_);
        std::swap(last_stats_, o.last_stats_);
        return *this;
    }

    Sophus::SE3d ComputeRobotMotion(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map,
                                    const Sophus::SE3d &last_robot_pose, const Sophus::SE3d &relative_wheel_odometry,
                                    const double max_correspondence_distance) {
        const kicp_reg_config c = config();  // the fields are public and mutable in the reference: honour edits
        kicp_bridge::check(kicp_reg_set_config(handle_, &c), "KinematicRegistration");
        double last[7], rel[7], out[7];
        kicp_bridge::to_params(last_robot_pose, last);
        kicp_bridge::to_params(relative_wheel_odometry, rel);
        kicp_bridge::check(kicp_register(handle_, voxel_map.handle(), kicp_bridge::xyz(frame), frame.size(), last, rel,
                                         max_correspondence_distance, out, &last_stats_),
                           "KinematicRegistration::ComputeRobotMotion");
        return kicp_bridge::from_params(out);
    }

    // backend extension: the frame as float32 xyz, the way a PointCloud2 carries it (RosUtils.cpp:30-39 widens it on the host);
    // half the bytes cross PCIe, the (exact) widening happens on the device
    Sophus::SE3d ComputeRobotMotion(const float *frame_xyz_f32, size_t n, const kiss_icp::VoxelHashMap &voxel_map, const Sophus::SE3d &last_robot_pose,
                                    const Sophus::SE3d &relative_wheel_odometry, const double max_correspondence_distance) {
        const kicp_reg_config c = config();
        kicp_bridge::check(kicp_reg_set_config(handle_, &c), "KinematicRegistration");
        double last[7], rel[7], out[7];
        kicp_bridge::to_params(last_robot_pose, last);
        kicp_bridge::to_params(relative_wheel_odometry, rel);
        kicp_bridge::check(kicp_register_f32(handle_, voxel_map.handle(), frame_xyz_f32, n, last, rel, max_correspondence_distance, out, &last_stats_),
                           "KinematicRegistration::ComputeRobotMotion(float)");
        return kicp_bridge::from_params(out);
    }

    // backend extension: the frame is already in HBM (output of the on-device pre-steps)
    Sophus::SE3d ComputeRobotMotionDevice(const double *d_frame_xyz, size_t n, const kiss_icp::VoxelHashMap &voxel_map,
                                          const Sophus::SE3d &last_robot_pose, const Sophus::SE3d &relative_wheel_odometry,
                                          const double max_correspondence_distance) {
        const kicp_reg_config c = config();
        kicp_bridge::check(kicp_reg_set_config(handle_, &c), "KinematicRegistration");
        double last[7], rel[7], out[7];
        kicp_bridge::to_params(last_robot_pose, last);
        kicp_bridge::to_params(relative_wheel_odometry, rel);
        kicp_bridge::check(kicp_register_device(handle_, voxel_map.handle(), d_frame_xyz, n, last, rel, max_correspondence_distance, out,
                                                &last_stats_),
                           "KinematicRegistration::ComputeRobotMotionDevice");
        return kicp_bridge::from_params(out);
    }

    // backend extension: DataAssociation (Registration.cpp:62-81) of ONE frame at many poses in one call (kicp.h kicp_score_poses):
    // per pose {number of correspondences, sum of their squared residuals}
    std::vector<std::pair<double, double>> ScorePoses(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map,
                                                      const std::vector<Sophus::SE3d> &poses, const double max_correspondence_distance) {
        const std::vector<double> flat = kicp_bridge::to_params(poses);
        std::vector<double> n_corr(poses.size()), ssr(poses.size());
        kicp_bridge::check(kicp_score_poses(handle_, voxel_map.handle(), kicp_bridge::xyz(frame), frame.size(), flat.data(), poses.size(),
                                            max_correspondence_distance, n_corr.data(), ssr.data()),
                           "KinematicRegistration::ScorePoses");
        std::vector<std::pair<double, double>> scores(poses.size());
        for (size_t k = 0; k < poses.size(); ++k) scores[k] = {n_corr[k], ssr[k]};
        return scores;
    }
    // backend extension: localise the frame among candidate poses (kicp.h kicp_relocalize): score all, refine the top_m cheapest, score
    // again.  `found` (nullable) tells whether a refinement kept correspondences; without one the cheapest unrefined candidate returns.
    struct Relocalization {
        Sophus::SE3d pose;
        size_t candidate = 0;
        double cost_before = 0.0, cost_after = 0.0;
        bool refined = false;
    };
    Relocalization Relocalize(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map, const std::vector<Sophus::SE3d> &candidates,
                              const double max_correspondence_distance, const size_t top_m = 8) {
        const kicp_reg_config c = config();
        kicp_bridge::check(kicp_reg_set_config(handle_, &c), "KinematicRegistration");
        const std::vector<double> flat = kicp_bridge::to_params(candidates);
        Relocalization r;
        double out[7];
        const int rc = kicp_bridge::check(kicp_relocalize(handle_, voxel_map.handle(), kicp_bridge::xyz(frame), frame.size(), flat.data(), candidates.size(),
                                                          max_correspondence_distance, top_m, out, &r.candidate, &r.cost_before, &r.cost_after),
                                          "KinematicRegistration::Relocalize");
        r.pose = kicp_bridge::from_params(out), r.refined = rc == KICP_OK;
        return r;
    }
    // backend extension: planar (x, y, yaw) Gauss-Newton refinement of many poses of ONE frame, all in lock step (kicp.h
    // kicp_refine_poses_planar); its own limits, not max_num_iterations_ / convergence_criterion_: a point-to-point step in the plane
    // needs tens of iterations.  status 0: converged, 1: max_iterations steps applied, 2: degenerate (the pose as it stood)
    struct PlanarRefinement {
        Sophus::SE3d pose;
        int iterations = 0, status = 0;
    };
    std::vector<PlanarRefinement> RefinePosesPlanar(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map,
                                                    const std::vector<Sophus::SE3d> &poses, const double max_correspondence_distance,
                                                    const int max_iterations = 100, const double convergence = 1e-4) {
        const std::vector<double> flat = kicp_bridge::to_params(poses);
        std::vector<double> out(flat.size());
        std::vector<int> iterations(poses.size()), status(poses.size());
        kicp_bridge::check(kicp_refine_poses_planar(handle_, voxel_map.handle(), kicp_bridge::xyz(frame), frame.size(), flat.data(), poses.size(),
                                                    max_correspondence_distance, max_iterations, convergence, out.data(), iterations.data(), status.data()),
                           "KinematicRegistration::RefinePosesPlanar");
        std::vector<PlanarRefinement> refined(poses.size());
        // (a degenerate pose comes back as it was given - a NaN pose included, which Sophus would refuse to rebuild)
        for (size_t k = 0; k < poses.size(); ++k) refined[k] = {status[k] == 2 ? poses[k] : kicp_bridge::from_params(&out[7 * k]), iterations[k], status[k]};
        return refined;
    }
    // backend extension: Relocalize with the finalists refined in the plane (kicp.h kicp_relocalize_planar): a candidate's lateral
    // offset is removed too, so a coarse grid only has to put one candidate into the basin of the truth
    Relocalization RelocalizePlanar(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map,
                                    const std::vector<Sophus::SE3d> &candidates, const double max_correspondence_distance, const size_t top_m = 8,
                                    const int max_iterations = 100, const double convergence = 1e-4) {
        const std::vector<double> flat = kicp_bridge::to_params(candidates);
        Relocalization r;
        double out[7];
        const int rc = kicp_bridge::check(kicp_relocalize_planar(handle_, voxel_map.handle(), kicp_bridge::xyz(frame), frame.size(), flat.data(), candidates.size(),
                                                                 max_correspondence_distance, top_m, max_iterations, convergence, out, &r.candidate,
                                                                 &r.cost_before, &r.cost_after),
                                          "KinematicRegistration::RelocalizePlanar");
        r.pose = kicp_bridge::from_params(out), r.refined = rc == KICP_OK;
        return r;
    }
    // backend extension: relocalisation over a whole search window without a candidate grid (kicp.h kicp_relocalize_search): the top_m
    // best nodes of the window by their hit count in the occupancy pyramid `occ` of voxel_map (kicp_bridge::build_occupancy), found by
    // branch and bound, then RelocalizePlanar with every one of them a finalist.  `candidate` is the node index the pose started from.
    Relocalization RelocalizeSearch(const std::vector<Eigen::Vector3d> &frame, const kiss_icp::VoxelHashMap &voxel_map, const kicp_occ *occ,
                                    const kicp_search_window &window, const double max_correspondence_distance, const size_t top_m = 8,
                                    const int max_iterations = 100, const double convergence = 1e-4) {
        Relocalization r;
        double out[7];
        unsigned long long node = 0;
        const int rc = kicp_bridge::check(kicp_relocalize_search(handle_, voxel_map.handle(), occ, kicp_bridge::xyz(frame), frame.size(), &window,
                                                                 max_correspondence_distance, top_m, max_iterations, convergence, out, &node, &r.cost_before,
                                                                 &r.cost_after),
                                          "KinematicRegistration::RelocalizeSearch");
        r.pose = kicp_bridge::from_params(out), r.candidate = static_cast<size_t>(node), r.refined = rc == KICP_OK;
        return r;
    }

    int max_num_iterations_;
    double convergence_criterion_;
    int max_num_threads_;
    bool use_adaptive_odometry_regularization_;
    double fixed_regularization_;

    // backend access (not part of the reference API)
    kicp_reg *handle() const { return handle_; }
    const kicp_stats &last_stats() const { return last_stats_; }

private:
    kicp_reg_config config() const {
        return kicp_reg_config{max_num_iterations_, convergence_criterion_, max_num_threads_, use_adaptive_odometry_regularization_ ? 1 : 0,
                               fixed_regularization_};
    }
    int device_ = kicp_bridge::default_device();  // KICP_DEVICE
    kicp_reg *handle_ = nullptr;
    kicp_stats last_stats_{};
};
}  // namespace kinematic_icp
