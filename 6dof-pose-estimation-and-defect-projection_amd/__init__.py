"""pedp_hip -- MI355X-native ICP refinement and ray-mesh defect projection.

The directory name follows the repository convention
(`6dof-pose-estimation-and-defect-projection_amd`); it is not a valid Python identifier,
so import it as `pedp_hip` (the small alias package at the repository root).

Layout
  csrc/            HIP kernels + the C ABI (include/pedp.h) -> libpedp_hip.so
  _lib.py          ctypes binding; raises if the library or the GPU is missing
  _bridge.py       the wrappers' torch / numpy plumbing: arrays on the call's side, launches on torch's stream
  geometry.py      PointCloud / TriangleMesh / RegistrationResult / PinholeCameraIntrinsic
                   holders with the attribute names the reference uses (Open3D duck types)
  registration.py  registration_icp, estimation/criteria classes, get_rotation_matrix_from_xyz
  icp_refine.py    host mirror of src/pose_estimation.py's refinement functions
  ray_projection.py host mirror of src/defect_projection.py's projection functions
  defect_map.py    DefectMap: per-face accumulation of projected heat maps on the model, and the defect regions
  coverage.py      CoverageMap: which faces of the model the camera has seen, and how well, over a DefectMap's faces
  view_plan.py     ViewPlanner: next-best-view planning, the gain of candidate camera poses over a CoverageMap; orbit_views
  deviation_map.py DeviationMap: per-face statistics of the signed deviation over frames, regions with their volume
  mesh_refine.py   refine_mesh: the model's faces split to a maximum edge length, each with its CAD face; edge_for_camera
  mesh_sample.py   sample_points_uniformly / sample_points_poisson_disk: the model's cloud from its mesh; thin_to_spacing, mesh_to_pcd
  surface_fit.py   fit_to_surface: robust best fit of a scene cloud to the posed surface itself; refit_pose, fit_frame_to_surface
  raycasting_scene.py RaycastingScene: cast_rays, count / list_intersections, test_occlusions and the distance queries on one mesh
  compat.py        `from pedp_hip.compat import *` in place of `from src import *` (run.py:3)
  dist.py          one-process-per-GPU sharding over torch.distributed (RCCL)
  synth.py         deterministic synthetic inputs of the benchmark configurations
"""
from . import _lib
from ._lib import PedpError, LIB_PATH
from .defect_map import DefectMap
from .coverage import CoverageMap
from .view_plan import ViewPlanner, orbit_views
from .deviation_map import DeviationMap
from .mesh_refine import RefinedMesh, edge_for_camera, refine_mesh
from .mesh_sample import MeshSampler, mesh_to_pcd, sample_points_poisson_disk, sample_points_uniformly, thin_to_spacing

__all__ = ["_lib", "PedpError", "LIB_PATH", "DefectMap", "CoverageMap", "ViewPlanner", "orbit_views", "DeviationMap", "refine_mesh",
           "RefinedMesh", "edge_for_camera", "sample_points_uniformly", "sample_points_poisson_disk", "thin_to_spacing", "mesh_to_pcd",
           "MeshSampler"]
