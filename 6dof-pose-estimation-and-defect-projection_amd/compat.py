"""Drop-in surface: `from pedp_hip.compat import *` where run.py says `from src import *`
(run.py:3, src/__init__.py:1-4), plus the `mycpp` slot (Utils.py:45-48, estimater.py:118).

The hot-path names, the global registration that precedes them under
`determine_pose(icp=True)`, the message format to the viewer thread (`update_dash_data`), and FoundationPose's
renderer (`nvdiffrast_render`, `make_mesh_tensors` and the `dr` stand-in for `nvdiffrast.torch`), and its crop batches
(`make_crop_data_batch`, `make_score_crop_data_batch` and the `kornia` stand-in with `warp_perspective`), and the pose
arithmetic of its refinement loop (`pose_update`, `max_pair_distance`), and the estimator with the two predictors'
loops (`FoundationPose`, `PoseRefinePredictor`, `ScorePredictor`, estimator.py), and the two networks with their
checkpoint loaders (`RefineNet`, `ScoreNetMultiPair`, `load_refiner`, `load_scorer`, networks.py), and the evaluation
metrics (`add_err`, `adds_err`, their batch forms, `compute_auc_sklearn`, `symmetry_tfs_from_info`, metrics.py), and the
exact cloud-to-mesh distance with the deviation heat map (`closest_points`, `compute_distance`, `align_to_mesh`,
`deviation_heatmap`, surface_distance.py), and the robust best fit of the scene to that surface, the pose the deviation
is measured in (`fit_to_surface`, `refit_pose`, `fit_frame_to_surface`, surface_fit.py), and the defect map on the model in the place of run.py:196-201's list of
hit clouds (`DefectMap`, defect_map.py), and the inspection coverage over its faces, which the reference has no
counterpart of (`CoverageMap`, coverage.py), and the next camera poses that coverage asks for (`ViewPlanner`,
`orbit_views`, view_plan.py), and the refinement that gives a coarse CAD model the resolution those per-face maps need
(`refine_mesh`, `RefinedMesh`, `edge_for_camera`, mesh_refine.py; the reference loads a separately prepared model file,
datareader.py:720-724), and the sampling that makes the model's cloud from the model's mesh (`mesh_to_pcd`,
`sample_points_uniformly`, `sample_points_poisson_disk`, `thin_to_spacing`, mesh_sample.py; pose_estimation.py:453-464); the Dash app, sensor
code and the networks' weights stay the reference's own.
"""
import numpy as np

from . import _lib
from .geometry import (KDTreeSearchParamHybrid, LineSet, PinholeCameraIntrinsic, PointCloud,  # noqa: F401
                       RegistrationResult, TriangleMesh)
from .icp_refine import (background_removal, compute_average_normal, determine_pose, estimate_normals,  # noqa: F401
                         execute_global_registration, filter_largest_cluster, run_icp,
                         flip_plane_normal_if_needed, improve_result, perform_plane_segmentation,
                         predict_z_axis_adjustment, preprocess_source, preprocess_target, refine_pose_with_icp,
                         refine_registration, remove_plane, remove_points_below_plane, remove_statistical_outliers,
                         transform_object)
from .ray_projection import (align_to_surface, calc_coordinates, compute_rays, create_intersection_pcd,  # noqa: F401
                             heatmap_to_point3d, heatmap_to_points, intersect_rays_with_mesh, load_extrinsics,
                             pcd_from_point3d, project_debug_rays, ray_tracing)
from .registration import (CorrespondenceCheckerBasedOnDistance, CorrespondenceCheckerBasedOnEdgeLength,  # noqa: F401
                           CorrespondenceCheckerBasedOnNormal, Feature, ICPConvergenceCriteria,
                           RANSACConvergenceCriteria, TransformationEstimationPointToPlane,
                           TransformationEstimationPointToPoint, compute_fpfh_feature, get_rotation_matrix_from_xyz,
                           registration_icp, registration_ransac_based_on_feature_matching)


def cluster_poses(angle_diff, dist_diff, poses_in, symmetry_tfs):
    """mycpp.cluster_poses(angle_diff_deg, dist_diff, poses[N,4,4], symmetry_tfs[S,4,4]) ->
    list of kept 4x4 float32 poses (mycpp/src/app/pybind_api.cpp:24-68).  Prints the two
    lines the C++ prints (:26, :66)."""
    poses = np.ascontiguousarray(poses_in, dtype=np.float32).reshape(-1, 4, 4)
    print(f"num original candidates = {len(poses)}")
    keep = _lib.cluster_poses(angle_diff, dist_diff, poses, symmetry_tfs)
    print(f"num of pose after clustering: {len(keep)}")
    return [poses[k].copy() for k in keep]


from .depth_filters import bilateral_filter_depth, depth2xyzmap, depth2xyzmap_batch, erode_depth  # noqa: E402
from .viewer_wire import update_dash_data  # noqa: E402  (web_vis.py:203-217: the message to the viewer thread)
from .render import (dr, glcam_in_cvcam, make_mesh_tensors, nvdiffrast_render,  # noqa: E402  (Utils.py:18, :68-220, :752-804)
                     projection_matrix_from_intrinsics)
from .crop import (BatchPoseData, compute_crop_window_tf_batch, kornia, make_crop_data_batch,  # noqa: E402,F401  (Utils.py:577-621)
                   make_score_crop_data_batch, warp_perspective)
from .pose import max_pair_distance, pose_update  # noqa: E402,F401  (predict_pose_refine.py:195-231, Utils.py:559-574)
from .estimator import (FoundationPose, PoseRefinePredictor, ScorePredictor, compute_mesh_diameter,  # noqa: E402,F401
                        euler_matrix, guess_translation, mask_depth_stats, sample_views_icosphere, set_seed)
from .metrics import (add_err, add_err_batch, adds_err, adds_err_batch, compute_auc_sklearn,  # noqa: E402,F401  (Utils.py:232-266, :806-834)
                      symmetry_tfs_from_info)
from .surface_distance import align_to_mesh, closest_points, compute_distance, deviation_heatmap  # noqa: E402,F401  (run.py:64's heat map)
from .surface_distance import (Solid, compute_occupancy, compute_signed_distance, signed_closest_points,  # noqa: E402,F401
                               signed_deviation, split_deviation)
from .surface_fit import fit_frame_to_surface, fit_to_surface, refit_pose  # noqa: E402,F401  (between refine_pose_with_icp and the heat map)
from .defect_map import DefectMap  # noqa: E402,F401  (run.py:61, :119, :196-201: the history of hits, kept per face)
from .coverage import CoverageMap  # noqa: E402,F401  (no counterpart: run.py never says what was not inspected)
from .view_plan import ViewPlanner, orbit_views  # noqa: E402,F401  (no counterpart: where to point the camera next)
from .deviation_map import DeviationMap  # noqa: E402,F401  (no counterpart: how far off each face is, over all frames)
from .mesh_refine import RefinedMesh, edge_for_camera, refine_mesh  # noqa: E402,F401  (datareader.py:720-724 loads an offline-refined model.ply)
from .mesh_sample import mesh_to_pcd, sample_points_poisson_disk, sample_points_uniformly, thin_to_spacing  # noqa: E402,F401  (pose_estimation.py:453-464)
from .raycasting_scene import RaycastingScene  # noqa: E402,F401  (defect_projection.py:245-256 builds one; here with all its queries)
from .networks import RefineNet, ScoreNetMultiPair, load_refiner, load_scorer  # noqa: E402,F401  (learning/models/*.py)


class _MyCpp:
    """`mycpp = pedp_hip.compat.mycpp` gives estimater.py its `mycpp.cluster_poses`."""
    cluster_poses = staticmethod(cluster_poses)


mycpp = _MyCpp()

__all__ = [
    "refine_registration", "improve_result", "predict_z_axis_adjustment", "refine_pose_with_icp", "determine_pose",
    "preprocess_source", "preprocess_target", "transform_object", "execute_global_registration", "run_icp",
    "perform_plane_segmentation", "flip_plane_normal_if_needed", "remove_plane", "remove_points_below_plane",
    "background_removal", "filter_largest_cluster", "remove_statistical_outliers", "estimate_normals",
    "compute_average_normal", "KDTreeSearchParamHybrid",
    "heatmap_to_points", "compute_rays", "intersect_rays_with_mesh", "create_intersection_pcd",
    "project_debug_rays", "load_extrinsics", "ray_tracing",
    "heatmap_to_point3d", "pcd_from_point3d", "calc_coordinates", "align_to_surface",
    "erode_depth", "bilateral_filter_depth", "depth2xyzmap", "depth2xyzmap_batch",
    "registration_icp", "TransformationEstimationPointToPlane", "TransformationEstimationPointToPoint",
    "ICPConvergenceCriteria", "get_rotation_matrix_from_xyz",
    "compute_fpfh_feature", "Feature", "registration_ransac_based_on_feature_matching", "RANSACConvergenceCriteria",
    "CorrespondenceCheckerBasedOnEdgeLength", "CorrespondenceCheckerBasedOnDistance", "CorrespondenceCheckerBasedOnNormal",
    "PointCloud", "TriangleMesh", "LineSet", "PinholeCameraIntrinsic", "RegistrationResult",
    "cluster_poses", "mycpp", "update_dash_data",
    "nvdiffrast_render", "make_mesh_tensors", "projection_matrix_from_intrinsics", "glcam_in_cvcam", "dr",
    "warp_perspective", "kornia", "compute_crop_window_tf_batch", "make_crop_data_batch", "make_score_crop_data_batch",
    "BatchPoseData", "pose_update", "max_pair_distance",
    "FoundationPose", "PoseRefinePredictor", "ScorePredictor", "guess_translation", "mask_depth_stats", "set_seed",
    "sample_views_icosphere", "euler_matrix", "compute_mesh_diameter",
    "RefineNet", "ScoreNetMultiPair", "load_refiner", "load_scorer",
    "add_err", "adds_err", "add_err_batch", "adds_err_batch", "compute_auc_sklearn", "symmetry_tfs_from_info",
    "closest_points", "compute_distance", "align_to_mesh", "deviation_heatmap",
    "Solid", "compute_signed_distance", "compute_occupancy", "signed_closest_points", "signed_deviation", "split_deviation",
    "fit_to_surface", "refit_pose", "fit_frame_to_surface",
    "DefectMap", "CoverageMap", "ViewPlanner", "orbit_views", "DeviationMap", "RaycastingScene",
    "refine_mesh", "RefinedMesh", "edge_for_camera",
    "mesh_to_pcd", "sample_points_uniformly", "sample_points_poisson_disk", "thin_to_spacing",
]
