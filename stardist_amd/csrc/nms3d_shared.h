// nms3d_shared.h -- what nms3d.hip offers to the other translation units of the library (raster3d.hip): the convex hulls of
// polyhedra and the cone map of a ray mesh, in buffers of the CURRENT arena pass (the caller has called Arena::begin()).
#pragma once
#include "common.h"
#include "geom3d.h"

namespace sd {

// Convex hulls of n polyhedra (the half-spaces Qhull gives the reference in halfspaces_convex, stardist3d_impl.cpp:767-795):
// planes[(i*cap + f)*4 .. +3] = (nz, ny, nx, offset) with inside <=> n.p + offset <= 0, count[i] facets (cap = 2*n_rays),
// count[i] == -2 if the hull could not be built; adj[(i*cap + f)*3 + e] = the facet across edge e of facet f (0xFFFF: unknown).
struct HullPlanes { double* planes; unsigned short* adj; int* count; int cap; };
int hull_planes(const float* d_dist, const float* d_points, const float* d_verts, int n, int R, HullPlanes* out, hipStream_t s);

struct SideJoin;     // nms_rounds.h
// Cone map of a ray mesh (geom3d.h); *out stays {nullptr, nullptr} when the map is switched off (sd_set_option("nms3d_cone_map", 0))
// or the mesh has too many faces for its 16-bit face ids.  fork != nullptr: built on the helper stream, next to what follows on s.
int cone_map(const float* d_verts, const int* d_faces, int F, sd3::ConeMap* out, hipStream_t s, SideJoin* fork = nullptr);

}  // namespace sd
