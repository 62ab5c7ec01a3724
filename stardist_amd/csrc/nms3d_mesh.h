// nms3d_mesh.h -- kernels over the ray mesh of the 3D NMS (nms3d.hip): edge adjacency of its faces (seeds of the exact volume
// routine), its validity as a star-shaped closed surface (precondition of the volume bounds, nms3d_hiv.h), and its refinement into the
// finer direction meshes of the bounds.  Device code of ONE translation unit (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// edge adjacency of the ray mesh: adj[3f + e] = face sharing edge e = (v_e, v_{e+1}) of face f (the lowest-numbered one), or -1.
// One wave per face, the lanes share the scan over the other faces (the meshes of the finer bounds have 4 F and 16 F faces).
__global__ void __launch_bounds__(64) k_face_adj(const int* __restrict__ faces, int F, int* __restrict__ adj) {
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f >= F) return;
  const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  int found[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
  for (int g = lane; g < F; g += 64) {
    if (g == f) continue;
    const int a = faces[3 * g], b = faces[3 * g + 1], c = faces[3 * g + 2];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int x = v[e], y = v[(e + 1) % 3];
      if ((a == x || b == x || c == x) && (a == y || b == y || c == y) && g < found[e]) found[e] = g;
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    int m = found[e];
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(m, o); m = t < m ? t : m; }
    if (lane == 0) adj[3 * f + e] = m == 0x7fffffff ? -1 : m;
  }
}

// Direction mesh for the volume bounds: the ray mesh with every triangle split in four at its edge midpoints (directions
// R + edge id).  The cones over the sub-triangles tile the cone of their parent, so the arguments above hold unchanged, and the
// gap between the two bounds shrinks ~4x: the exact volume (100x the cost) is needed for ~4x fewer pairs.
__global__ void k_refine_edges(const int* __restrict__ faces, const int* __restrict__ adj, int F, int* __restrict__ edgeId, int* counter) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * F) return;
  const int f = t / 3, g = adj[t];
  edgeId[t] = (g < 0 || f < g) ? atomicAdd(counter, 1) : -1;            // the face with the smaller index owns the shared edge
}
__global__ void k_refine_mesh(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ adj, int R, int F,
                              const int* __restrict__ edgeId, float* __restrict__ verts2, int* __restrict__ faces2) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < R) { verts2[3 * f] = verts[3 * f]; verts2[3 * f + 1] = verts[3 * f + 1]; verts2[3 * f + 2] = verts[3 * f + 2]; }
  if (f >= F) return;
  const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  int mid[3];
  for (int e = 0; e < 3; ++e) {
    const int x = v[e], y = v[(e + 1) % 3];
    int id = edgeId[3 * f + e];
    if (id < 0) {                                                       // owned by the neighbour: its edge with the same end points
      const int g = adj[3 * f + e];
      for (int e2 = 0; e2 < 3; ++e2) {
        const int a = faces[3 * g + e2], b = faces[3 * g + (e2 + 1) % 3];
        if ((a == x && b == y) || (a == y && b == x)) id = edgeId[3 * g + e2];
      }
    } else {
      const int m = R + id;
      verts2[3 * m] = 0.5f * (verts[3 * x] + verts[3 * y]); verts2[3 * m + 1] = 0.5f * (verts[3 * x + 1] + verts[3 * y + 1]);
      verts2[3 * m + 2] = 0.5f * (verts[3 * x + 2] + verts[3 * y + 2]);
    }
    mid[e] = R + id;
  }
  int* o = faces2 + 12 * f;                                             // same orientation as the parent
  o[0] = v[0]; o[1] = mid[0]; o[2] = mid[2];
  o[3] = mid[0]; o[4] = v[1]; o[5] = mid[1];
  o[6] = mid[2]; o[7] = mid[1]; o[8] = v[2];
  o[9] = mid[0]; o[10] = mid[1]; o[11] = mid[2];
}

// The volume bounds above need the ray mesh to be a closed surface that is star-shaped about the origin (cones over its
// triangles tile the sphere of directions exactly once).  mesh[0] |= 1: an edge without a partner, |= 2: degenerate or
// degenerate face; mesh_sa = sum of the absolute solid angles (Van Oosterom & Strackee): exactly 4 pi iff the radial
// projection of the closed mesh covers the sphere once without folds.
__global__ void k_mesh_check(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ adj, int F, int* mesh,
                             double* mesh_sa) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  double u[3][3];
  for (int y = 0; y < 3; ++y) {
    const int v = faces[3 * f + y];
    const double z = verts[3 * v], yy = verts[3 * v + 1], x = verts[3 * v + 2];
    const double nn = sqrt(z * z + yy * yy + x * x);
    u[y][0] = z / nn; u[y][1] = yy / nn; u[y][2] = x / nn;
  }
  const double det = u[0][0] * (u[1][1] * u[2][2] - u[1][2] * u[2][1]) + u[0][1] * (u[1][2] * u[2][0] - u[1][0] * u[2][2]) +
                     u[0][2] * (u[1][0] * u[2][1] - u[1][1] * u[2][0]);
  const double d01 = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
  const double d12 = u[1][0] * u[2][0] + u[1][1] * u[2][1] + u[1][2] * u[2][2];
  const double d20 = u[2][0] * u[0][0] + u[2][1] * u[0][1] + u[2][2] * u[0][2];
  const double sa = 2.0 * atan2(det, 1.0 + d01 + d12 + d20);
  int bad = 0;
  if (adj[3 * f] < 0 || adj[3 * f + 1] < 0 || adj[3 * f + 2] < 0) bad |= 1;
  if (!(fabs(det) > 1e-12)) bad |= 2;
  if (bad) atomicOr(&mesh[0], bad);
  atomicAdd(&mesh[det > 0 ? 1 : 2], 1);
  atomicAdd(mesh_sa, fabs(sa));
}

}  // namespace
