// The cluster of a mesh handle's culling spheres (pedp_mesh_s::spheres): CL_TRIS consecutive triangle records share
// one bounding sphere, 64 clusters one super-cluster sphere.  Built by ray/mesh_records.h; read by the culled ray
// sweep (ray/sweep_culled.h) and by the closest-point search (pedp_closest.hip).
#pragma once

namespace {

constexpr int CL_TRIS = 16;  // triangles per cluster

}  // namespace
