/* stardist_hip.h -- C ABI of libstardist_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the native layer of the StarDist prediction path.  Every entry point
 * replaces one function of the reference's native modules `stardist.lib.stardist2d` /
 * `stardist.lib.stardist3d` (CPython, positional args) or of its experimental plain-C ABI
 * `libstardist3d` (stardist/lib/stardist3d_lib.h:52-79) and keeps that function's argument
 * meaning, array layout (row-major, dense) and ownership rules:
 *
 *   - caller owns every buffer; inputs are never modified;
 *   - `*_host` entry points (and the two `_LIB_*` names kept verbatim from the reference ABI)
 *     take HOST pointers and do H2D/D2H themselves on the null stream;
 *   - `*_device` entry points take DEVICE pointers plus a `hipStream_t` (passed as void*) and
 *     enqueue all work on that stream; they synchronise the stream only where documented
 *     (the NMS entry points do, because the greedy scan is driven from the host);
 *   - return value: 0 on success, -1 on error (message via sd_last_error()); the two `_LIB_*`
 *     functions return void like the reference and report errors on stderr.
 *
 * No torch / numpy types appear here.  The reference-side bindings (CPython / ctypes / JNA)
 * are shown in INTEGRATION.md.
 */
#ifndef STARDIST_HIP_H
#define STARDIST_HIP_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------ */
const char* sd_last_error(void);          /* message of the calling thread's last failed call  */
int sd_version(void);                     /* ABI version, currently 1                          */
int sd_device_count(void);                /* number of visible HIP devices (0 without a GPU)   */
int sd_release_workspace(void);           /* free the cached device workspace                  */
/* Switches between EQUIVALENT formulations (same results; the parity suite runs both settings against the reference):
 *   "nms3d_volume_bounds" 1|0  decide 3D pairs from rigorous volume bounds where possible / always compute the exact volume
 *   "nms3d_cone_map"      1|0  stage-5 voxel tests through the cone map / over every face as the reference does
 *   "nms3d_refine_mesh"   2|1|0  direction meshes of the volume bounds: the ray mesh only (0); refined once for the pairs it leaves
 *                              undecided (1); refined twice for the pairs that reach the exact-volume kernels (2, default)
 *   "nms3d_tail_batch"    1|0  late greedy rounds of the 3D NMS (once at most max(N/32, 512) candidates are undecided) as one speculative
 *                              batch + replay on the device / as plain rounds; a value d >= 2 sets the threshold to N/d (tuning)
 *   "nms3d_split_exact"   3|2|1|0  exact volumes of the pairs the bounds leave undecided by four waves per pair in a second pass (3,
 *                              default: for every launch; 2: stage 4 only up to 16 384 pairs per launch; 1: both stages only for small
 *                              launches, full-size workspace in the bounds pass) / 0: by the wave that evaluated the bounds
 *                              (bit-identical volumes)
 *   "nms3d_bounds_reuse"  1|0  the once-refined direction mesh keeps the ray mesh's vertices in front: their boundary points are taken
 *                              from the coarse pass that has just run over the same planes (bit for bit what a second cast would store) /
 *                              every direction of the refined mesh is cast
 *   "nms3d_bounds_lean"   1|0  bounds-only launches of stages 3 / 4 (every launch in the two-pass form) are made without the adjacency-seed
 *                              table, and the cull's index tables lie in the ray-cast workspace: 21.9 instead of 25.6 KB of LDS per wave,
 *                              seven waves per CU instead of six / the layout of the one-pass kernels
 *   "nms3d_defer_exact"   r|0  from greedy round r on, the pairs the bounds of stages 3 / 4 leave undecided are not integrated in their
 *                              round (a launch of the exact-volume kernel costs one exact volume's latency however few pairs it holds):
 *                              they are queued, the suppressed-or-not candidate stays undecided, and the tail batch evaluates the queue
 *                              in its one pass (needs "nms3d_tail_batch" and "nms3d_split_exact"; same survivors; default 3: measured
 *                              on the 256^3 bench set 23.0 -> 21.3 ms, from round 1 or 2 on the pending candidates stall the rounds
 *                              behind them: 23.2 ms) / 0: every round integrates its own
 *   "nms2d_area_bounds"   1|0  2D pairs far from the threshold are decided from an enclosure of the intersection area (regular arithmetic,
 *                              area_bounds.h) / every pair runs the Clipper-exact sweep
 *   "nms2d_defer_undecided" r|0  (with "nms2d_area_bounds") from greedy round r on (default 2), a round that leaves at most 16 384 pairs undecided
 *                              does not sweep them itself: they are swept by the tail batch's one launch (a sweep launch costs one sweep's
 *                              latency however few pairs it holds) / 0: every round sweeps its own; "nms2d_defer_max" = that pair limit (16 384;
 *                              measured on the 2048^2 bench set: deferring round 1's 55 000 pairs as well stalls the rounds behind it -- 13.5 instead of 7.7 ms)
 *   "nms2d_strict"        0|1  1 = bit-exact BY CONSTRUCTION: every 2D pair runs the Clipper-exact sweep (overrides "nms2d_area_bounds"); the
 *                              default decides the pairs far from the threshold from an enclosure of Clipper's area whose band is validated
 *                              empirically and adversarially, not proven
 *   "nms2d_neighbours_single_pass", "nms3d_neighbours_single_pass" 1|0  neighbour lists of the NMS written in one pass into slots sized
 *                              from the cell table / counted, scanned and filled in two passes (same lists up to order)
 *   "probe_tier"          1|2  capacity tier sd_clip_pairs_device runs first;  "probe_no_general" 1: do not fall back to the general path
 *   "trace"               1    print per-round counters to stdout
 * Nothing in the library reads the process environment.  sd_get_option returns -1 for an unknown name. */
int sd_set_option(const char* name, int value);
int sd_get_option(const char* name);

/* ---- 2D non-maximum suppression ------------------------------------------------------------
 * replaces stardist.lib.stardist2d.c_non_max_suppression_inds
 *   (stardist/lib/stardist2d.cpp:390-615; caller stardist/nms.py:186-227)
 * dist   (n_polys, n_rays) float32, points (n_polys, 2) float32 (y, x), both sorted by score
 * descending.  use_kdtree / use_bbox / verbose / threshold as in the reference ("O!O!iiif").
 * keep   (n_polys,) bytes: 1 = survivor, 0 = suppressed (the reference returns NPY_BOOL).
 * stats  optional int64[16] (may be NULL): {0 pairs evaluated, 1 pairs re-run on the exact-join path,
 *        2 greedy rounds, 3 ordered neighbour relations (2 x the entries the lists store), 4 pair-kernel time ns (HIP events on `stream`),
 *        5 pair-kernel launches, 6 exact-join kernel ns, 7 build+bin+neighbour kernels ns, 8 capacity spills,
 *        9 pairs decided by the area enclosure (counted in 0 as well), 10 undecided pairs deferred to the tail batch,
 *        11 undecided pairs not swept because another pair had suppressed their j meanwhile (counted in 0 as well),
 *        12 slot total of the single-pass neighbour lists: the sum over the candidates of the population of the cells each list is built
 *           from, a true 64-bit sum, whichever form the lists took (0 for a call that ends before the lists),
 *        13 form of the neighbour lists: 1 = one pass into slots, 0 = two passes (asked for by "nms2d_neighbours_single_pass" = 0, or
 *           because the slot total is 2^31 - 1 or more or the slots do not fit the workspace), 14.. 0}.
 * Beyond 2^31 - 2 stored neighbour entries the call fails ("exceed the capacity of one call"); every total involved is summed in 64 bits.
 */
int sd_nms2d_host(const float* dist, const float* points, int n_polys, int n_rays,
                  int use_kdtree, int use_bbox, int verbose, float threshold,
                  uint8_t* keep, int64_t* stats);
int sd_nms2d_device(const float* d_dist, const float* d_points, int n_polys, int n_rays,
                    int use_kdtree, int use_bbox, int verbose, float threshold,
                    uint8_t* d_keep, int64_t* stats, void* stream);

/* Test probe of the 2D NMS's build step, exactly as sd_nms2d_device runs it (same kernel, same table of ray directions): integer
 * vertices d_vx / d_vy (n_polys, n_rays), d_bbox (n_polys, 4) [xmin, xmax, ymin, ymax], d_radius, d_area (n_polys) and d_gstats (5):
 * bits of the largest distance, min / max of floor(y) and of floor(x) over the centres. */
int sd_nms2d_build_device(const float* d_dist, const float* d_points, int n_polys, int n_rays, int32_t* d_vx, int32_t* d_vy,
                          int32_t* d_bbox, float* d_radius, float* d_area, int32_t* d_gstats, void* stream);

/* replaces stardist.lib.stardist2d.c_non_max_suppression_inds_old
 *   (stardist/lib/stardist2d.cpp:173-386, "O!O!fiiii"; caller stardist/nms.py:20-74 _non_maximum_suppression_old; the reference keeps
 *   it as a second statement of the NMS, tests/test_nms2D.py:78-110 "old == new")
 * polys   (n_polys, 2, n_rays) int32 vertex coordinates (row 0 = y, row 1 = x), sorted by score descending;
 * mapping (height, width) int32: id of the score-sorted polygon at that pixel of the prediction grid, -1 = none (only read with
 *         max_bbox_search != 0: polygon i is compared with the polygons j > i found in the window
 *         [(bbox - max bbox size) / grid, (bbox + max bbox size) / grid) of the map, :285-311; else with every j > i, :337);
 * keep    (n_polys,) bytes: 1 = survivor. */
int sd_nms2d_old_host(const int32_t* polys, int n_polys, int n_rays, const int32_t* mapping, int height, int width,
                      float threshold, int max_bbox_search, int grid_y, int grid_x, int verbose, uint8_t* keep);
int sd_nms2d_old_device(const int32_t* d_polys, int n_polys, int n_rays, const int32_t* d_mapping, int height, int width,
                        float threshold, int max_bbox_search, int grid_y, int grid_x, int verbose, uint8_t* d_keep, void* stream);

/* Test hook of the exclusive sum behind the neighbour lists of both NMS and the pair list of sd_nms2d_old_device: d_out[k] = the sum of
 * d_in[0 .. k) for k < n, int32 counts summed in 64 bits (a sum in the counts' own type would wrap at 2^32 whatever the type of d_out). */
int sd_exclusive_sum_i32_i64_device(const int32_t* d_in, int n, int64_t* d_out, void* stream);

/* Test probe: Clipper::AddPath (clipper.cpp:1045-1221) once per polygon -- the prepared-polygon records the 2D NMS
 * builds per candidate (stardist_amd/csrc/clip_beam.h, PolyPrep<MAXV>, MAXV = 32/64/128/256 for n_verts). */
int sd_prepare_polys_device(const int32_t* d_x, const int32_t* d_y, int n_polys, int n_verts, void* d_out,
                            int64_t out_bytes, void* stream);

/* pair-level probe used by the parity tests: intersection area of integer polygons exactly as
 * poly_intersection_area (stardist2d.cpp:152-165) computes it.  xa..yb are device int32
 * arrays of shape (n_pairs, n_verts); out_twice_area int64 (2*area), out_flags int32
 * (bit0.. see clip_sweep.h status bits, bit8 = pair needed the join path). */
int sd_clip_pairs_device(const int32_t* d_xa, const int32_t* d_ya, const int32_t* d_xb,
                         const int32_t* d_yb, int n_pairs, int n_verts,
                         int64_t* d_out_twice_area, int32_t* d_out_flags, void* stream);

/* Test probe of the decision shortcut of the 2D NMS (stardist_amd/csrc/area_bounds.h): for the same inputs as sd_clip_pairs_device
 * (n_verts 3..32) the exact area of the intersection by boundary integration (float32), the half-width of the band that encloses
 * the area ClipperLib returns for the pair, and info = bit 0: the enclosure may be used for a decision (both polygons simple, equally
 * oriented, small enough for exact float predicates), bits 8..17: number of boundary crossings, bits 18..28: number of edge pairs
 * closer than one lattice step. */
int sd_area_bounds_pairs_device(const int32_t* d_xa, const int32_t* d_ya, const int32_t* d_xb, const int32_t* d_yb, int n_pairs,
                                int n_verts, float* d_out_area, float* d_out_band, int32_t* d_out_info, void* stream);
/* The largest grid (blocks of four waves, two pairs per wave and trip) sd_area_bounds_pairs_device launches on the current device:
 * the number of blocks resident at once by the occupancy query; -1 when the query fails.  Tests size inputs with it so that a wave
 * takes several trips. */
int sd_area_bounds_pairs_grid(void);

/* Test probe of the 2D NMS's per-polygon pass for n_verts <= 32 (stardist_amd/csrc/poly_pass.h), exactly as the NMS launches it:
 * d_props (n_polys) records of 32 bytes (area_bounds.h PolyProps; n_verts 3..32) and / or d_prep (n_polys) PolyPrep<32> records, each
 * may be NULL.  Bytes of a PolyPrep record that the preparation does not define are left as they were. */
int sd_poly_pass_device(const int32_t* d_x, const int32_t* d_y, int n_polys, int n_verts, void* d_props, void* d_prep, void* stream);

/* ---- star-convex distances (training targets; same native module) --------------------------
 * replaces stardist.lib.stardist2d.c_star_dist (stardist2d.cpp:55-124)
 * src (H, W) uint16 labels; dst (ceil(H/gy), ceil(W/gx), n_rays) float32. */
int sd_star_dist2d_host(const uint16_t* src, int H, int W, int n_rays, int grid_y, int grid_x,
                        float* dst);
int sd_star_dist2d_device(const uint16_t* d_src, int H, int W, int n_rays, int grid_y,
                          int grid_x, float* d_dst, void* stream);
/* replaces stardist.lib.stardist3d.c_star_dist3d (stardist3d.cpp:245-346)
 * src (Z, Y, X) uint16; dz/dy/dx (n_rays,) float32 ray unit vectors;
 * dst (ceil(Z/gz), ceil(Y/gy), ceil(X/gx), n_rays) float32. */
int sd_star_dist3d_host(const uint16_t* src, int Z, int Y, int X, const float* dz,
                        const float* dy, const float* dx, int n_rays, int grid_z, int grid_y,
                        int grid_x, float* dst);
int sd_star_dist3d_device(const uint16_t* d_src, int Z, int Y, int X, const float* d_dz,
                          const float* d_dy, const float* d_dx, int n_rays, int grid_z,
                          int grid_y, int grid_x, float* d_dst, void* stream);

/* ---- training target: per-object normalised distance transform ----------------------------
 * replaces stardist.utils.edt_prob (stardist/utils.py:71-125; called by the data generators).
 * lbl (Z, Y, X) int32 label image (2D: Z = 1), labels 1..max_label are objects, everything else background;
 * (sz, sy, sx) axis spacing (the reference's `anisotropy`); prob (Z, Y, X) float32: for an object pixel the Euclidean distance
 * (float64) to the nearest pixel inside the image with another label, divided by (the object's maximum + 1e-10); else 0. */
int sd_edt_prob_device(const int32_t* d_lbl, int Z, int Y, int X, double sz, double sy, double sx, int max_label,
                       float* d_prob, void* stream);

/* ---- 2D label rasteriser --------------------------------------------------------------------
 * replaces the Python loop stardist.geometry.geom2d.polygons_to_label_coord
 *   (stardist/geometry/geom2d.py:149-166: skimage.draw.polygon per object, later objects
 *   overwrite earlier ones).
 * coord (n_polys, 2, n_rays) float32 (row 0 = y/r, row 1 = x/c), painted in array order;
 * labels (n_polys,) int32: value written is labels[i]+1 (geom2d.py:164);
 * result (H, W) int32, fully written (background 0). */
int sd_polygons_to_label_host(const float* coord, const int32_t* labels, int n_polys, int n_rays,
                              int H, int W, int32_t* result);
int sd_polygons_to_label_device(const float* d_coord, const int32_t* d_labels, int n_polys,
                                int n_rays, int H, int W, int32_t* d_result, void* stream);
/* ... only the window [y0, y0 + H) x [x0, x0 + W) of an HI x WI image (d_result (H, W)): the pixels are the ones the whole-image
 * call writes there -- each rank of a block-sharded prediction renders the write regions of its own blocks (stardist/big.py:319-326
 * block.write) from the global polygon list. */
int sd_polygons_to_label_window_device(const float* d_coord, const int32_t* d_labels, int n_polys, int n_rays, int HI, int WI,
                                       int y0, int x0, int H, int W, int32_t* d_result, void* stream);

/* polar -> cartesian for a list of polygons: replaces stardist.geometry.geom2d.dist_to_coord (geom2d.py:130-146) in numpy's own
 * arithmetic (products and the final sum in float64, rounded to float32 where numpy rounds): d_dist (n, R) float32, d_points (n, 2)
 * float64 (y, x), d_sincos (2, R) float64 = (sin, cos) of linspace(0, 2 pi, R, endpoint=False) computed by the caller's libm,
 * scale (y, x) = `scale_dist`; d_coord (n, 2, R) float32. */
int sd_dist_to_coord_device(const float* d_dist, const double* d_points, const double* d_sincos, long long n_polys, int n_rays,
                            double scale_y, double scale_x, float* d_coord, void* stream);

/* ---- behind the 2D NMS on predict_instances (stardist/models/model2d.py:536-561) --------------
 * positions of the non-zero keep flags, ascending (the `inds` of non_maximum_suppression_sparse, nms.py:175-183: boolean-mask indexing):
 * d_positions (n) int64 receives *d_count entries. */
int sd_survivor_positions_device(const unsigned char* d_keep, long long n, long long* d_positions, int32_t* d_count, void* stream);
/* for candidates in SCORE order (descending, as the NMS takes them): rows of the m survivors at d_positions -- prob (m), points (m, 2)
 * int64 -- their polygon coordinates d_out_coord (m, 2, R) = dist_to_coord (geom2d.py:130-146, arithmetic of sd_dist_to_coord_device,
 * scale 1), and the same coordinates in the order polygons_to_label paints them (ascending score, stable: geom2d.py:186-197) with
 * their label ids minus one, d_out_labels_paint (m) -- the inputs of sd_polygons_to_label_device.  d_out_coord_paint may be NULL. */
int sd_survivors2d_device(const long long* d_positions, int m, const float* d_prob, const long long* d_points, const float* d_dist,
                          int n_rays, const double* d_sincos, float* d_out_prob, long long* d_out_points, float* d_out_coord,
                          float* d_out_coord_paint, int32_t* d_out_labels_paint, void* stream);

/* ---- 3D non-maximum suppression -------------------------------------------------------------
 * name, signature and semantics of the reference's C ABI
 *   (stardist/lib/stardist3d_lib.h:52-66 -> _COMMON_non_maximum_suppression_sparse,
 *    stardist/lib/stardist3d_impl.cpp:956-1385; Python caller stardist/nms.py:327-384)
 * host pointers; result (n_polys,) bool: true = survivor. */
void _LIB_non_maximum_suppression_sparse(const float* scores, const float* dist,
                                         const float* points, const int n_polys,
                                         const int n_rays, const int n_faces, const float* verts,
                                         const int* faces, const float threshold,
                                         const int use_bbox, const int use_kdtree,
                                         const int verbose, bool* result);
/* stats: optional int64[16]: {0 upper-bound tests, 1 lower-bound tests, 2 kernel-volume calls, 3 render calls,
 * 4 greedy rounds, 5 neighbour entries, 6 suppressed by kernel stage, 7 suppressed by render stage,
 * 8 stage-3 kernel ns, 9 stage-4 ns, 10 stage-5 ns, 11 hull-volume calls, 12 kept by hull stage,
 * 13 exact-volume decisions (stages 3 / 4) whose ratio lies within 1e-6 of the threshold -- the volumes agree with Qhull's to 1e-9
 * relative, so only such a pair could be decided differently; the count makes that observable --, 14 faces that needed the
 * large-capacity fallback, 15 broad-phase ns}.  All sixteen entries are taken: the slot total and the form of the neighbour lists, which
 * sd_nms2d_device reports in stats[12] and [13], have no place here (same list builder, same 64-bit totals). */
int sd_nms3d_device(const float* d_scores, const float* d_dist, const float* d_points,
                    int n_polys, int n_rays, int n_faces, const float* d_verts,
                    const int* d_faces, float threshold, int use_bbox, int use_kdtree,
                    int verbose, uint8_t* d_keep, int64_t* stats, void* stream);

/* Test probe of the two volume stages of the 3D cascade: for every pair (i, j) of d_pairs (int32 [n_pairs][2], indices into the
 * n_polys candidates) the intersection volume of the two KERNELS (replaces qhull_overlap_kernel, stardist3d_impl.cpp:830-869,
 * 0 if the midpoint of the centres is not interior) and of the two CONVEX HULLS (replaces qhull_overlap_convex_hulls, :872-939,
 * 1e10 on failure), as float64.  Either output pointer may be NULL. */
int sd_hiv_pairs_device(const float* d_dist, const float* d_points, int n_polys, int n_rays, int n_faces,
                        const float* d_verts, const int* d_faces, const int32_t* d_pairs, int n_pairs,
                        double* d_vol_kernel, double* d_vol_hull, void* stream);

/* ---- 3D label rasteriser --------------------------------------------------------------------
 * name, signature and semantics of the reference's C ABI
 *   (stardist/lib/stardist3d_lib.h:69-77 -> _COMMON_polyhedron_to_label,
 *    stardist/lib/stardist3d_impl.cpp:1404-1525; Python caller geom3d.py:100-198)
 * result (nz, ny, nx) int32 must be zero-initialised by the caller (the reference only writes
 * inside polyhedra). Polyhedra are given in painting order (first writer keeps the voxel). */
void _LIB_polyhedron_to_label(const float* dist, const float* points, const float* verts,
                              const int* faces, const int n_polys, const int n_rays,
                              const int n_faces, const int* labels, const int nz, const int ny,
                              const int nx, const int render_mode, const int verbose,
                              const int use_overlap_label, const int overlap_label, int* result);
int sd_polyhedron_to_label_device(const float* d_dist, const float* d_points,
                                  const float* d_verts, const int* d_faces, int n_polys,
                                  int n_rays, int n_faces, const int* d_labels, int nz, int ny,
                                  int nx, int render_mode, int verbose, int use_overlap_label,
                                  int overlap_label, int* d_result, void* stream);
/* ... only the window [z0, z0 + nz) x [y0, y0 + ny) x [x0, x0 + nx) of an NZ x NY x NX volume; d_result (nz, ny, nx) must be
 * zero-initialised by the caller like the whole-volume result (the implementation only writes inside polyhedra). */
int sd_polyhedron_to_label_window_device(const float* d_dist, const float* d_points, const float* d_verts, const int* d_faces,
                                         int n_polys, int n_rays, int n_faces, const int* d_labels, int NZ, int NY, int NX,
                                         int z0, int y0, int x0, int nz, int ny, int nx, int render_mode, int verbose,
                                         int use_overlap_label, int overlap_label, int* d_result, void* stream);

/* ---- candidate selection --------------------------------------------------------------------
 * replaces the numpy glue stardist.nms._ind_prob_thresh + np.where + gather
 *   (stardist/nms.py:6-17, stardist/models/base.py:553-610) on device.
 * prob (n_pix,) float32 and dist (n_pix, n_rays) float32 are the network heads over a grid of
 * `ndim` (2 or 3) dims `shape`; selects pixels with prob > thresh that are at least b[2*d] /
 * b[2*d+1] grid cells from the low / high face of dim d, in C order (== np.where order).
 * Writes out_prob (cap,), out_dist (cap, n_rays) = max(dist, 1e-3f) (skipped when d_dist is NULL), out_points (cap, ndim)
 * int32 grid indices (NOT yet multiplied by the grid) and *d_count (int32) = number found
 * (may exceed cap: then only the first cap are written). */
int sd_select_candidates_device(const float* d_prob, const float* d_dist, int ndim,
                                const int* shape, const int* b, int n_rays, float thresh,
                                int cap, float* d_out_prob, float* d_out_dist,
                                int32_t* d_out_points, int32_t* d_count, void* stream);

/* np.argsort(scores)[::-1] of stardist/nms.py:114,167 on the device, stated as a stable ascending sort reversed (best score first, equal scores
 * in descending order of their position): d_scores (n,) float32 (finite) -> d_sorted (n,) float32 = the scores in that order, d_order (n,) int64 =
 * the position of the k-th best in d_scores. */
int sd_sort_scores_desc_device(const float* d_scores, int n, float* d_sorted, int64_t* d_order, void* stream);

/* Candidates in score order (the argsort of stardist/nms.py:167 applied to the selection above): d_points (n_sel, ndim) int32 grid indices as
 * written by sd_select_candidates_device, d_order (n,) int64 = index of the k-th best candidate (NULL: identity).  Writes, per k:
 * d_rows[k] = C-order linear index of (point + origin) in the grid `full_shape` (the row of the channels-last feature matrix the
 * distance head is evaluated on, sd_head_rows_device), d_points_f32[k] / d_points_i64[k] = point * grid (pixel coordinates: float32 as the
 * NMS natives take them, int64 as the result dict returns them).  Any output pointer may be NULL. */
int sd_sorted_rows_device(const int32_t* d_points, const int64_t* d_order, int n, int ndim, const int* full_shape, const int* origin,
                          const int* grid, int64_t* d_rows, float* d_points_f32, int64_t* d_points_i64, void* stream);

/* ---- reference-style C ABI for the natives that have none in the reference --------------------
 * (stardist/lib/stardist3d_lib.h:52-79 covers only the two 3D functions above).  Same conventions: host pointers, caller
 * owns all buffers, no return code (errors abort with a message on stderr).  Argument meaning as the CPython functions:
 *   _LIB_non_maximum_suppression_2d  <- c_non_max_suppression_inds      stardist2d.cpp:390-615  (dist, points sorted by score)
 *   _LIB_polygon_to_label            <- polygons_to_label_coord         geom2d.py:149-166       (coord (n,2,n_rays); result (ny,nx))
 *   _LIB_star_dist                   <- c_star_dist                     stardist2d.cpp:55-124
 *   _LIB_star_dist3d                 <- c_star_dist3d                   stardist3d.cpp:245-346 */
void _LIB_non_maximum_suppression_2d(const float* dist, const float* points, const int n_polys,
                                     const int n_rays, const float threshold, const int use_bbox,
                                     const int use_kdtree, const int verbose, bool* result);
void _LIB_polygon_to_label(const float* coord, const int* labels, const int n_polys,
                           const int n_rays, const int ny, const int nx, int* result);
void _LIB_star_dist(const unsigned short* src, const int ny, const int nx, const int n_rays,
                    const int grid_y, const int grid_x, float* dst);
void _LIB_star_dist3d(const unsigned short* src, const int nz, const int ny, const int nx,
                      const float* pdz, const float* pdy, const float* pdx, const int n_rays,
                      const int grid_z, const int grid_y, const int grid_x, float* dst);

/* ---- network epilogue ------------------------------------------------------------------------
 * bias + activation of a convolution output in one in-place pass (the reference's Keras Conv layers do both inside the
 * layer: csbdeep unet_block / resnet_block as called from stardist/models/model2d.py:310-349, model3d.py:360-447).
 * x is viewed as [n_outer][n_channels][inner] float32 (channels-last tensors: inner = 1, n_outer = pixels);
 * act: 0 = linear, 1 = relu. */
int sd_bias_act_device(float* d_x, const float* d_bias, long long n_outer, int n_channels,
                       long long inner, int act, void* stream);
/* x = act((x + addend) + bias): epilogue of a convolution over a channel concatenation that is evaluated as two
 * convolutions over the two sources (Concatenate + Conv of csbdeep's unet_block up path, blocks.py) -- the
 * concatenated tensor is never written. addend has the layout of x. */
int sd_add_bias_act_device(float* d_x, const float* d_addend, const float* d_bias, long long n_outer,
                           int n_channels, long long inner, int act, void* stream);

/* Keras MaxPooling2D / 3D(pool), 'valid', stride = pool, channels-last float32 (csbdeep unet_block between its levels; the grid > 1
 * stages of stardist/models/model2d.py:317-325): d_in [D][H][W][C] -> d_out [D/pz][H/py][W/px][C]; 2D: D = pz = 1.  C % 4 == 0.
 * Special values (one rule for both pooling forms, this one and sd_maxpool_split16_ndhwc_device): a window that holds a NaN, of either
 * sign, gives NaN -- pooling never hides a numerical failure, and the forward maximum is the element the adjoint
 * (sd_maxpool3d_adjoint_ndhwc_device) takes as the arg-max; otherwise the maximum in the total order -inf < .. < -0 < +0 < .. < +inf.
 * (The ReLU of the epilogues -- sd_bias_act_device and the convolutions' -- is max(v, 0) of the hardware: a NaN and -0 give +0.) */
int sd_maxpool_ndhwc_device(const float* d_in, int n_channels, int D, int H, int W, int pz, int py, int px, float* d_out, void* stream);

/* point-level probe of the reference's inside_polyhedron (stardist/lib/stardist3d_impl.cpp:153-191) for ONE polyhedron
 * (d_dist: n_rays, d_centre: 3, zyx) on n points (d_points: n x 3, zyx): d_out[t] = 1 if inside.  use_cone_map != 0 evaluates
 * the predicate only on the faces whose cone can contain the point's direction (csrc/geom3d.h), as stage 5 of the NMS does;
 * both settings give identical results. */
int sd_inside_polyhedron_device(const float* d_dist, const float* d_centre, int n_rays, int n_faces,
                                const float* d_verts, const int* d_faces, const float* d_points,
                                long long n, int use_cone_map, uint8_t* d_out, void* stream);

/* features epilogue + one-channel head: out = act(in + bias) over channels-last [n_pix][n_channels] float32 (in place when
 * d_out == d_in; n_channels 32, 64, 128 or 256) and, when d_w is given, d_dot[p] = sum_c out[p][c] * d_w[c] + d_wbias[0], through the
 * logistic function when sigmoid != 0: the object-probability head of the reference's models (Conv 1x1, sigmoid:
 * stardist/models/model2d.py:338-341, model3d.py:436-439) evaluated while the features are in registers.
 * d_bias == NULL: no bias; d_out == NULL (d_w given): the features are only read and just d_dot is written. */
int sd_bias_act_dot_device(const float* d_in, float* d_out, const float* d_bias, long long n_pix, int n_channels,
                           int act, const float* d_w, const float* d_wbias, int sigmoid, float* d_dot, void* stream);
/* distance head on selected pixels: d_out[i][r] = max(clamp_min, d_bias[r] + sum_k d_feat[d_rows[i]][k] * d_w[r][k]) for
 * i < n_rows, r < n_out (d_rows == NULL: row i itself, i.e. the dense head).  d_feat is channels-last [n_pix][n_channels],
 * d_w the Conv 1x1 kernel [n_out][n_channels] (model2d.py:342-343, model3d.py:440-441).  With d_rows = the candidate pixels
 * (prob > prob_thresh) this is what predict_sparse (stardist/models/base.py:553-610) keeps of the dense prediction.
 * fp32 MFMA, one fixed fma chain per output whatever rows are batched together. */
int sd_head_rows_device(const float* d_feat, int n_channels, const long long* d_rows, long long n_rows,
                        const float* d_w, const float* d_bias, int n_out, float clamp_min, float* d_out,
                        void* stream);

/* ---- network convolutions (hand-written, f32 matrix cores) --------------------------------------------------------------
 * One Keras Conv2D(3x3) / Conv3D(3x3x3), padding='same', stride 1, + bias + activation of the reference's U-Net (csbdeep unet_block as
 * built by stardist/models/model2d.py:310-349 and model3d.py:360-399), channels-last float32:
 *     out[z][y][x][co] = act(bias[co] + sum_{ci,kz,ky,kx} in[z+kz-1][y+ky-1][x+kx-1][ci] * w[co][ci][kz][ky][kx])   (zero padding)
 * kz = 1: 2D (D must be 1), kz = 3: 3D.  The input channels are the concatenation [source 0 (c0 channels), source 1 (c1 channels)]
 * -- Concatenate([up, skip]) of the up path without the concatenated tensor; d_src1 == NULL: one source.  `up` is a bit mask of the
 * axes (1: x, 2: y, 4: z) along which a source has half the output resolution and is read through nearest-neighbour 2x up-sampling
 * (UpSampling2D/3D folded into the operand fetch).  stride = floats per pixel of a source.
 * Supported: c0, c1 multiples of 32 with c0 + c1 <= 512 and c_out a multiple of 32; and the first layer c0 = 1 (c_out % 4 == 0).
 * d_wpacked: the kernel in the device layout written by sd_conv3_pack_weights_host (sd_conv3_packed_floats floats).
 * act: 0 linear, 1 relu.  Exact float32: each output is one fma chain in a fixed order (bias first), repeatable bit for bit. */
long long sd_conv3_packed_floats(int c_in, int c_out, int kz);
int sd_conv3_pack_weights_host(const float* w /* [c_out][c_in][kz][3][3] */, int c_in, int c_out, int kz, float* packed);
int sd_conv3_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1, int up1,
                          int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, int c_out, int act,
                          float* d_out, void* stream);
/* ... with a residual: out = act(conv + bias + res), res channels-last [D][H][W][res_stride] -- Add([shortcut, x]) + Activation that
 * closes a csbdeep resnet_block (stardist/models/model3d.py:417-422), folded into the convolution's epilogue.  d_res == NULL: none. */
int sd_conv3_res_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1, int up1,
                              int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, const float* d_res,
                              int res_stride, int c_out, int act, float* d_out, void* stream);

/* The same layer with every f32 product evaluated as six bf16 x bf16 products (operands split into three bf16 terms each, f32
 * accumulation) on the bf16 matrix cores: f32-level accuracy (the dropped cross terms are below 2^-24 of a product) at 6/16 of the
 * f32-MFMA time.  Same arguments; c0, c1 multiples of 32 only (the one-channel first layer stays on sd_conv3_ndhwc_device); the
 * weights are packed by sd_conv3_bf16x6_pack_weights_host.  Opt-in: the exact-f32 kernel above is the default network path. */
long long sd_conv3_bf16x6_packed_floats(int c_in, int c_out, int kz);
int sd_conv3_bf16x6_pack_weights_host(const float* w /* [c_out][c_in][kz][3][3] */, int c_in, int c_out, int kz, float* packed);
int sd_conv3_bf16x6_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1,
                                 int up1, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, int c_out,
                                 int act, float* d_out, void* stream);
int sd_conv3_bf16x6_res_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1,
                                     int up1, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias,
                                     const float* d_res, int res_stride, int c_out, int act, float* d_out, void* stream);

/* The same layer with every f32 product evaluated as three fp16 x fp16 products: each operand x = hi + lo' * 2^-11 (hi = fp16(x),
 * lo' = fp16((x - hi) * 2^11)), a * b ~ hi*hi + 2^-11 (hi*lo' + lo'*hi), f32 accumulation in two accumulators on the fp16 matrix cores:
 * f32-level accuracy (the dropped term is below 2^-22 of a product; networks within 3e-6 of a float64 evaluation like the two forms
 * above) with half the matrix instructions of the bf16 form -- the default network path since round 4.  Same arguments as
 * sd_conv3_bf16x6_*, plus d_range_flag (device int, may be NULL): OR-ed with 1 when an input value lies outside the fp16 range
 * (|x| > 65504, infinities included; a NaN is not flagged -- it propagates into the output as in any f32 evaluation), in which case the output is not valid and the caller must re-evaluate the layer with the bf16x6 form.
 * sd_conv3_f16x3_pack_weights_host returns -2 (weights still packed) when a weight is outside that range.
 * Option "conv_f16_workgroups_per_cu" (sd_set_option): 2 (default) or 1, an A/B probe of the launch geometry; same results. */
long long sd_conv3_f16x3_packed_floats(int c_in, int c_out, int kz);
int sd_conv3_f16x3_pack_weights_host(const float* w /* [c_out][c_in][kz][3][3] */, int c_in, int c_out, int kz, float* packed);
int sd_conv3_f16x3_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1,
                                int up1, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, int c_out,
                                int act, float* d_out, int* d_range_flag, void* stream);
int sd_conv3_f16x3_res_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1,
                                    int up1, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias,
                                    const float* d_res, int res_stride, int c_out, int act, float* d_out, int* d_range_flag,
                                    void* stream);

/* ... with the ONE-CHANNEL HEAD behind the layer fused into its epilogue (the object-probability head behind the features layer:
 * Conv 1x1 + sigmoid, stardist/models/model2d.py:338-341, model3d.py:436-439).  Besides d_out the kernel writes, per pixel and per group of
 * four consecutive output channels, the sum (in channel order) of their products (after bias + activation) with d_dot_w[c_out]:
 * d_dot_partial[D * H * W][c_out / 4] -- the per-lane term of sd_bias_act_dot_device, taken while the tile is in registers.
 * sd_dot_combine_device (groups = c_out / 32: 1, 2, 4 or 8) adds a pixel's terms in the order of that function's reduction, then the
 * head's bias d_wbias[0] (NULL: none), then the logistic function (sigmoid != 0): the result equals sd_bias_act_dot_device on the same
 * features BIT FOR BIT, without reading the features a second time. */
int sd_conv3_f16x3_dot_ndhwc_device(const float* d_src0, int c0, int stride0, int up0, const float* d_src1, int c1, int stride1,
                                    int up1, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, int c_out,
                                    int act, float* d_out, int* d_range_flag, const float* d_dot_w, float* d_dot_partial, void* stream);
int sd_dot_combine_device(const float* d_partial, int groups, long long n_pix, const float* d_wbias, int sigmoid, float* d_out, void* stream);

/* ---- split16 activation tensors (round 6) ---------------------------------------------------------------------------------------
 * What the split-fp16 kernel's consumer side derives from every f32 value it reads -- hi = fp16(x), lo' = fp16((x - hi) * 2^11) -- made
 * ONCE by the producing layer instead of once per consumer workgroup and unit.  A split16 tensor has the shape, strides and addresses
 * of the channels-last f32 tensor it stands for (C a multiple of 32, dense); per pixel and 32-channel chunk its 128 bytes hold 8
 * elements of 16 bytes: element p * 4 + o = the fp16 terms of plane p (0: hi, 1: lo') of channels o * 8 .. o * 8 + 7.
 * Value = hi + lo' * 2^-11 (exact in f32): the 22 bits the f32-tensor entry points keep of x, so every layer's result is bit-identical
 * whichever form carries the activations between the layers of the reference's U-Net (csbdeep unet_block, model2d.py:310-349,
 * model3d.py:360-399).
 *   sd_conv3_f16x3_fmt_ndhwc_device   the layer of sd_conv3_f16x3_ndhwc_device / _dot_ with either side in split16 form
 *                                     (in_split16: all sources; out_split16: no fused head then).  d_range_flag |= 1: an f32 INPUT was
 *                                     outside the fp16 range; |= 2: a value of the split16 OUTPUT was (the output is not valid).
 *   sd_conv3_c1x32_split16_device     the one-channel first layer (1 -> 32, weights packed by sd_conv3_pack_weights_host) writing split16
 *   sd_maxpool_split16_ndhwc_device   MaxPooling on a split16 tensor: == split16(maxpool(f32 tensor)) bit for bit (x -> (hi, lo') is monotone);
 *                                     the special-value rule of sd_maxpool_ndhwc_device: a pair whose value hi + lo' 2^-11 is NaN wins, so the result is NaN
 *                                     in both terms wherever the f32 form gives NaN; the pair of +-inf, (+-inf, NaN), is ordered by its hi
 *   sd_split16_pack_device / _unpack_device   f32 <-> split16 as their own passes (tests; consumers that only take f32 tensors);
 *                                     d_range_flag (may be NULL) |= 2 when a value is outside the fp16 range, infinities included.  A NaN
 *                                     is NOT a range error, here and in the flags of the convolutions alike: it is not flagged and stays
 *                                     a NaN in both terms */
int sd_conv3_f16x3_fmt_ndhwc_device(const float* d_src0, int c0, int up0, const float* d_src1, int c1, int up1, int D, int H, int W, int kz,
                                    const float* d_wpacked, const float* d_bias, int c_out, int act, float* d_out, int in_split16,
                                    int out_split16, int* d_range_flag, const float* d_dot_w, float* d_dot_partial, void* stream);
/* ... on SELECTED pixels: d_out[r][0 .. c_out) = act(bias + conv(src))[d_rows[r]] (d_rows: linear pixel indices into [D][H][W]), bit-identical to
 * what the dense entry points store there.  The sparse prediction path (stardist/models/base.py:553-610 predict_sparse keeps the candidates of
 * a dense prediction) runs the features layer densely WITHOUT its store -- sd_conv3_f16x3_fmt_ndhwc_device with d_out == NULL and the fused
 * probability head: only the head's partial sums leave the kernel -- and then evaluates the layer here for the candidate pixels only. */
int sd_conv3_f16x3_rows_device(const float* d_src, int c_in, int in_split16, int D, int H, int W, int kz, const float* d_wpacked,
                               const float* d_bias, int c_out, int act, const long long* d_rows, long long n_rows, float* d_out, void* stream);
int sd_conv3_c1x32_split16_device(const float* d_src, int D, int H, int W, int kz, const float* d_wpacked, const float* d_bias, int act,
                                  float* d_out, int* d_range_flag, void* stream);
int sd_maxpool_split16_ndhwc_device(const float* d_in, int n_channels, int D, int H, int W, int pz, int py, int px, float* d_out, void* stream);
int sd_split16_pack_device(const float* d_in, long long n_pix, int n_channels, float* d_out, int* d_range_flag, void* stream);
int sd_split16_unpack_device(const float* d_in, long long n_pix, int n_channels, float* d_out, void* stream);

/* UpSampling2D/3D (nearest, x2 along the axes of `up`: bit 0 x, 1 y, 2 z) + Concatenate([up-sampled a, b]) of a csbdeep unet_block up
 * level as one channels-last tensor [D][H][W][ca + cb] (a: [D >> z][H >> y][W >> x][ca]).  Only the coverage path needs it -- up
 * levels whose channel counts are not multiples of 32 (e.g. n_filter_base = 48) run this + sd_convg_ndhwc_device; the fused 3x3 kernels
 * above never materialise the concatenation.  ca, cb multiples of 4. */
int sd_upcat_ndhwc_device(const float* d_a, int ca, int up, const float* d_b, int cb, int D, int H, int W, float* d_out, void* stream);

/* ---- general convolution (any kernel size, stride, padding, channel counts) ------------------------------------------------
 * Every other convolution of the reference's networks, channels-last float32, exact f32 on the matrix cores with one fixed fma chain
 * per output (bias first, residual last): the 7x7x7 stem, the strided first convolution and the strided 1x1x1 shortcut projection of
 * csbdeep's resnet_block (stardist/models/model3d.py:400-447), first layers with n_channel_in = 3 (model2d.py:310-316), 1x1 heads
 * with few channels (prob_class, model2d.py:345-347).
 *     out[zo][yo][xo][co] = act(bias[co] + sum in[zo*sz - pz + dz][yo*sy - py + dy][xo*sx - px + dx][ci] * w[co][ci][dz][dy][dx] (+ res))
 * with zeros outside the input; (pz, py, px) = padding BEFORE the first element (TensorFlow 'same' with a stride pads asymmetrically,
 * so the caller states it); (Do, Ho, Wo) = output extent.  2D: kz = sz = 1, pz = 0, D = Do = 1.  c_in a multiple of 32, or
 * taps * c_in <= 6144 (small-channel form); any c_out.  src_stride / res_stride / out_stride = floats per pixel of those tensors.
 * d_wpacked: written by sd_convg_pack_weights_host (sd_convg_packed_floats floats; -1 = unsupported shape). */
long long sd_convg_packed_floats(int c_in, int c_out, int kz, int ky, int kx);
int sd_convg_pack_weights_host(const float* w /* [c_out][c_in][kz][ky][kx] */, int c_in, int c_out, int kz, int ky, int kx, float* packed);
int sd_convg_ndhwc_device(const float* d_src, int c_in, int src_stride, int D, int H, int W, int kz, int ky, int kx, int sz, int sy,
                          int sx, int pz, int py, int px, int Do, int Ho, int Wo, const float* d_wpacked, const float* d_bias,
                          const float* d_res, int res_stride, int c_out, int act, float* d_out, int out_stride, void* stream);

/* ---- evaluation: sparse overlap of two label images (stardist/matching.py:45-52 without the dense matrix) ------------------
 * d_true, d_pred: two int32 label images of n elements each (2D or 3D, flattened in the same order).  Result: every pair (t, p) != (0, 0)
 * of labels that share at least one pixel, ascending by (t, p), as d_keys[i] = t << 32 | p (original ids, no relabelling) and
 * d_counts[i] = its number of pixels.  Buffer protocol: capacity plus real count -- *h_count (host) receives the number of pairs, the
 * first min(*h_count, cap) of them are written; a caller whose cap was too small calls again with cap >= *h_count (cap = 0 with NULL
 * buffers is a pure count query).  h_minmax (host, 4 ints) receives {min, max} of d_true, then of d_pred ({0, 0, 0, 0} for n = 0); if
 * either minimum is negative nothing else is computed and *h_count = 0.  Integer arithmetic only: the list is bit-identical from call
 * to call.  Synchronises the stream (the number of runs sizes the sort).  At most 2^31 - 1 runs of equal (t, p). */
int sd_label_overlap_device(const int32_t* d_true, const int32_t* d_pred, long long n, long long cap, int64_t* d_keys, int64_t* d_counts,
                            long long* h_count, int32_t* h_minmax, void* stream);

/* The same list for every consecutive pair (k, k + 1) of the K >= 2 frames of the int32 stack d_ys (K, n), in one call: the K - 1 lists
 * sparse_overlap(ys[k], ys[k + 1]) are concatenated in d_keys / d_counts (format and capacity protocol as above, *h_count = entries of
 * all lists); h_offsets (host, K entries): list k is [h_offsets[k], h_offsets[k + 1]), h_offsets[K - 1] = *h_count (always filled in
 * full, whatever cap is).  h_minmax (host, 2 K ints): {min, max} of every frame; a negative minimum leaves everything else 0.  Every
 * frame is read twice (count pass, append pass); the pair index is sorted as the bits above the ids, and where pair index and ids need
 * more than 64 bits the pairs are worked off in groups inside the call (ids up to 2^31 - 1, any K).  Integer arithmetic only, bit-
 * identical from call to call.  Synchronises the stream once plus once per group. */
int sd_label_overlap_stack_device(const int32_t* d_ys, int K, long long n, long long cap, int64_t* d_keys, int64_t* d_counts,
                                  long long* h_offsets, long long* h_count, int32_t* h_minmax, void* stream);

/* Relabel a stack through one table per frame: d_out[k][i] = new id of d_ys[k][i] (both int32 (K, n)), 0 stays 0.  The table of frame k
 * is d_ids / d_new [h_offsets[k], h_offsets[k + 1]) (h_offsets: host, K + 1 entries): raw ids ascending, strictly positive, and the id
 * each becomes; h_max[k] (host) = the largest raw id of frame k.  An id that is not in its frame's table becomes 0.  Frames with
 * h_max[k] < 2^22 are looked up in a dense table built here (while the tables of a call stay below 2^26 entries), the others by a
 * binary search in the sorted ids.  One launch for the stack; every element of d_out is written.  Synchronises the stream once (the
 * upload of the frame descriptors). */
int sd_relabel_stack_device(const int32_t* d_ys, int K, long long n, const int32_t* d_ids, const int32_t* d_new,
                            const long long* h_offsets, const int32_t* h_max, int32_t* d_out, void* stream);

/* ---- training (2D): backward pass and losses (csrc/train2d.hip; the two pooling / up-sampling adjoints: csrc/train3d.hip) ------
 * The reference trains its Keras model with StarDist2D.train (stardist/models/model2d.py) on the losses of base.py:34-60, 315-325; these
 * entry points are the pieces of that step the forward kernels above do not cover.  Channels-last float32, batch B (2D: [B][H][W][C]).
 *
 * sd_conv_wgrad_ndhwc_device: weight and bias gradient of a 'same' k x k convolution (k = 3, or k = 1 with one full-resolution source)
 *     dW[co][ci][ky][kx] = sum_{b,y,x} g[b][y][x][co] * in[b][y+ky-1][x+kx-1][ci]      (k = 1: in[b][y][x][ci]; zero padding)
 *     db[co] = sum g[..][co]   (d_db may be NULL)
 * with in = [src0 (c0 channels) | src1 (c1 channels)] and the forward kernels' `up` bit masks (1: x, 2: y: the source has half the
 * resolution and is read through nearest up-sampling).  Any channel counts (c_in = 1 included).  Exact f32 products on the matrix cores;
 * the pixels are split into chunks that depend on the shape only, the chunk partials are added in chunk order in float64: repeatable bit
 * for bit.  d_dw is [c_out][c0 + c1][k][k] (the torch layout).
 * sd_relu_mask_device: out = y > 0 ? dy : 0 (the ReLU adjoint from the saved post-activation output y).
 * sd_maxpool_adjoint_ndhwc_device: adjoint of sd_maxpool_ndhwc_device (pool py x px, stride = pool, 'valid'): each window's gradient goes
 * to its first maximum in scan order (y, then x), everything else is zero.  d_in = the pooling's input [B][H][W][C], d_gout [B][H/py][W/px][C].
 * sd_upcat_adjoint_ndhwc_device: adjoint of [UpSampling(src0) | src1]: d_gcat [B][H][W][c0 + c1] -> d_g1 = its last c1 channels
 * [B][H][W][c1], d_g0 [B][H >> y][W >> x][c0] = the sum over each up-sampling window (order dy, then dx) of its first c0 channels.
 * These two check their own arguments and then are sd_maxpool3d_adjoint_ndhwc_device / sd_upcat3d_adjoint_ndhwc_device (below) with
 * D = 1, pz = 1 and up bit 4 clear: one kernel per operation serves both models.
 * sd_stardist_loss2d_device: the 2D model's losses and their gradients over n_pix pixels (batch and space flattened):
 *     prob_loss = mean over pixels with prob_true >= 0 of -(t log(pc + e) + (1 - t) log(1 - pc + e)),  pc = clip(prob, e, 1 - e), e = 1e-7
 *     dist_loss = mean over pixels of  mean_r(m * pen(t_r - d_r)) / (mean(m) + e) + reg * mean_r((1 - m) |d_r|)
 * (m = the last channel of d_dist_true_mask [n_pix][n_rays + 1]; pen = |.| for dist_loss 0 (mae), square for 1 (mse)); d_losses (device,
 * 3 doubles) = {prob_loss, dist_loss, w_prob * prob_loss + w_dist * dist_loss}; d_grad_logit [n_pix] = d total / d (logit of prob)
 * (zero where prob is clipped or masked), d_grad_dist [n_pix][n_rays] = d total / d dist; both NULL: the losses only (evaluation without
 * a backward pass).  float64 sums in a fixed order.
 * sd_stardist_loss2d_metrics_device: sd_stardist_loss2d_device (the same losses and gradients, bit for bit; gradient buffers both NULL:
 * the losses only) that also evaluates the metrics the reference compiles its model with (base.py kld, relevant_mae, relevant_mse,
 * dist_iou_metric) over the same pixels; d_metrics (device, 4 doubles) =
 *     kld             = mean over pixels with prob_true >= 0 of bce(tc, pc) - bce(tc, tc),  tc = clip(prob_true, e, 1), pc = clip(prob, e, 1)
 *     relevant_mae    = mean over pixels of m mean_r |t_r - d_r|   / (mean(m) + e)
 *     relevant_mse    = mean over pixels of m mean_r (t_r - d_r)^2 / (mean(m) + e)
 *     dist_iou_metric = mean over pixels of m inter / (union + e)   / (mean(m) + e)
 * with bce the cross entropy of prob_loss above, inter = mean_r min(t_r, d+_r)^2, union = mean_r max(t_r, d+_r)^2, d+ = max(0, d).  These
 * are the values of one batch; Keras averages kld over batches and the other three over pixels. */
int sd_conv_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src0, int c0, int up0, const float* d_src1, int c1, int up1,
                               int B, int H, int W, int k, float* d_dw, float* d_db, void* stream);
int sd_relu_mask_device(const float* d_dy, const float* d_y, long long n, float* d_out, void* stream);
int sd_maxpool_adjoint_ndhwc_device(const float* d_in, const float* d_gout, int n_channels, int B, int H, int W, int py, int px,
                                    float* d_gin, void* stream);
int sd_upcat_adjoint_ndhwc_device(const float* d_gcat, int c0, int up0, int c1, int B, int H, int W, float* d_g0, float* d_g1, void* stream);
int sd_stardist_loss2d_device(const float* d_prob, const float* d_dist, const float* d_prob_true, const float* d_dist_true_mask,
                              long long n_pix, int n_rays, int dist_loss, double w_prob, double w_dist, double background_reg,
                              double* d_losses, float* d_grad_logit, float* d_grad_dist, void* stream);
int sd_stardist_loss2d_metrics_device(const float* d_prob, const float* d_dist, const float* d_prob_true, const float* d_dist_true_mask,
                                      long long n_pix, int n_rays, int dist_loss, double w_prob, double w_dist, double background_reg,
                                      double* d_losses, float* d_grad_logit, float* d_grad_dist, double* d_metrics, void* stream);

/* ---- StarDist3D training (stardist/models/model3d.py train; csrc/train3d.hip) ------------------------------------------------
 * The pieces of the 3D U-Net / ResNet training step that neither the forward kernels nor the 2D entry points above cover, and the
 * max-pool / up-sampling adjoint kernels of both models (2D tensors are the D = 1 case).
 * Channels-last float32, batch B: [B][D][H][W][C].  The losses are sd_stardist_loss2d_device's with n_pix = B * d * h * w.
 *
 * sd_conv3_wgrad_ndhwc_device: weight and bias gradient of a 'same' 3x3x3 convolution with stride 1
 *     dW[co][ci][kz][ky][kx] = sum_{b,z,y,x} g[b][z][y][x][co] * in[b][z+kz-1][y+ky-1][x+kx-1][ci]      (zero padding)
 *     db[co] = sum g[..][co]   (d_db may be NULL)
 * with in = [src0 (c0 channels) | src1 (c1 channels)] and the forward kernels' `up` bit masks (1: x, 2: y, 4: z: that source has half
 * the resolution along the axis and is read through nearest up-sampling).  Any channel counts (c_in = 1 included).
 * sd_convg_wgrad_ndhwc_device: the same for any kernel (kz, ky, kx), stride (sz, sy, sx) and padding before the first element
 * (pz, py, px) -- the convention of sd_convg_ndhwc_device: g is the gradient of the output [B][Do][Ho][Wo][c_out], src the input
 * [B][D][H][W][c_in]:  dW[co][ci][dz][dy][dx] = sum g[b][zo][yo][xo][co] * src[b][zo*sz - pz + dz][yo*sy - py + dy][xo*sx - px + dx][ci].
 * Both: exact f32 products on the matrix cores; the output rows are split into chunks that depend on the shape only and the chunk
 * partials are added in chunk order in float64: repeatable bit for bit.  d_dw has the torch layout [c_out][c_in][kz][ky][kx].
 * sd_convg_dgrad_ndhwc_device: the data gradient of that convolution (a transposed convolution), d_gin [B][D][H][W][c_in]:
 *     gin[b][z][y][x][ci] = sum over (dz, dy, dx) with zo = (z + pz - dz) / sz integral and inside [0, Do) (likewise y, x),
 *                           over co ascending, of g[b][zo][yo][xo][co] * w[co][ci][dz][dy][dx]
 * one f32 fma chain in that order per element; d_wt is the kernel in the layout [kz][ky][kx][c_out][c_in].
 * sd_maxpool3d_adjoint_ndhwc_device: adjoint of sd_maxpool_ndhwc_device (pool pz x py x px, stride = pool, 'valid'): each window's
 * gradient goes to its first maximum in scan order (z, y, x), everything else is zero.  d_in = the pooling's input [B][D][H][W][C].
 * sd_upcat3d_adjoint_ndhwc_device: adjoint of [UpSampling3D(src0) | src1]: d_gcat [B][D][H][W][c0 + c1] -> d_g1 = its last c1
 * channels, d_g0 [B][D >> z][H >> y][W >> x][c0] = the sum over each up-sampling window (order dz, dy, dx) of its first c0 channels. */
int sd_conv3_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src0, int c0, int up0, const float* d_src1, int c1, int up1,
                                int B, int D, int H, int W, float* d_dw, float* d_db, void* stream);
int sd_convg_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src, int c_in, int B, int D, int H, int W, int kz, int ky,
                                int kx, int sz, int sy, int sx, int pz, int py, int px, int Do, int Ho, int Wo, float* d_dw, float* d_db,
                                void* stream);
int sd_convg_dgrad_ndhwc_device(const float* d_g, int c_out, const float* d_wt, int c_in, int B, int D, int H, int W, int kz, int ky,
                                int kx, int sz, int sy, int sx, int pz, int py, int px, int Do, int Ho, int Wo, float* d_gin, void* stream);
int sd_maxpool3d_adjoint_ndhwc_device(const float* d_in, const float* d_gout, int n_channels, int B, int D, int H, int W, int pz, int py,
                                      int px, float* d_gin, void* stream);
int sd_upcat3d_adjoint_ndhwc_device(const float* d_gcat, int c0, int up0, int c1, int B, int D, int H, int W, float* d_g0, float* d_g1,
                                    void* stream);

/* ---- training a multi-class model (the reference's StarDistData2D / 3D with n_classes and weighted_categorical_crossentropy,
 * stardist/models/model2d.py:106-119, base.py:108-126; csrc/train_classes.hip) ---------------------------------------------------
 * sd_class_targets_device: prob_class of a batch, d_out [B][d][h][w][n_channels] (n_channels = n_classes + 1), in one launch from the
 * batch's label patches d_labels [B][D][H][W] (int32, negative ids clipped to 0; images: D = d = 1).
 *   d_meta [B][4] per sample: {offset into d_keys / d_codes, entries, form, default code}.  Form 0: a dense table, the label id is the
 *   index; form 1: `entries` label ids sorted ascending in d_keys (d_keys may be NULL when every sample is dense), searched.  An id the
 *   table does not hold has the default code.  Codes: 0 ... n_classes = the class id, -1 = ignore the object, -2 = missing.
 *   d_tz [d], d_ty [h], d_tx [w]: the source index of each output position along the axis (the nearest-neighbour zoom the reference
 *   applies, tabulated by the caller), -1 = outside the array.  d_neg [B][d][h][w] (bytes, may be NULL): the negative-label mask.
 *   Per output pixel, with l its source label: every channel 0; class c >= 1 sets channel c to 1; code -1 sets every channel to -1;
 *   channel 0 = (l == 0); an outside pixel is all 0; a pixel of d_neg is all -1.
 *   The launch also looks up every label > 0 of d_labels: if one has code -2, *d_missing (device int32, cleared by the caller) is
 *   raised with an atomic or.  Nothing is synchronised.
 * sd_class_loss_device: the weighted categorical cross entropy of the class head over n_pix pixels, from its logits [n_pix][n_channels]
 * and the targets of sd_class_targets_device, e = 1e-7:
 *     p = softmax(z),  S = sum_c (p_c + e),  q = clip(p / S, e, 1 - e),  L = -sum_c w_c [t_c >= 0] t_c log q_c,  loss = sum L / n_pix
 * (every pixel counts in the mean, as in Keras).  d_class_weights: n_channels doubles on the device.  d_losses (device, 2 doubles) =
 * {loss, w_class * loss}.  d_grad_logits [n_pix][n_channels] = d (w_class * loss) / d z of this literal expression (zero through the
 * clip where p / S leaves [e, 1 - e]; through the division with every p_j free; through the softmax), or NULL: the loss only, the same
 * bits.  float64 per pixel, partial sums per fixed pixel range added in order: repeatable bit for bit.  Any n_channels >= 2. */
int sd_class_targets_device(const int32_t* d_labels, int B, int D, int H, int W, const int32_t* d_meta, const int32_t* d_keys,
                            const int32_t* d_codes, const int32_t* d_tz, const int32_t* d_ty, const int32_t* d_tx, int d, int h, int w,
                            const unsigned char* d_neg, int n_channels, float* d_out, int32_t* d_missing, void* stream);
int sd_class_loss_device(const float* d_logits, const float* d_target, const double* d_class_weights, long long n_pix, int n_channels,
                         double w_class, double* d_losses, float* d_grad_logits, void* stream);

/* ---- image normalisation (csbdeep.utils.normalize / normalize_mi_ma; csrc/normalize.hip) --------------------------------------
 * d_x: a contiguous array of n_seg interleaved segments of n elements each (element i belongs to segment i % n_seg: a channels-last image
 * whose statistics are taken over every axis but the last; n_seg = 1: over the whole array).  dtype: 0 = uint8, 1 = uint16, 2 = float32.
 *
 * sd_percentiles_device: d_out[seg * n_q + j] = float32(np.percentile(segment seg, h_q[j])) (method 'linear'), bit for bit: exact order
 *   statistics by radix selection on order-preserving keys (one histogram pass for uint8 / uint16, three for float32), then numpy's
 *   interpolation between the two neighbouring order statistics.  h_q: n_q percentiles in [0, 100] on the host, 2 <= n_q <= 3.
 *   interp_f32 (float32 data only): 1 = virtual index, weight and interpolation in float32 -- what numpy >= 2.0 does for float32 data
 *   and a Python-scalar q; 0 = in float64, rounded to float32 at the end (numpy < 2.0, or q given as float64 array).  Integer data
 *   always interpolate in float64.  A NaN anywhere in a float32 segment gives NaN for that segment.  1 <= n_seg <= 64, n >= 1.
 *   Integer counting only: the same bits from call to call.  Nothing is copied to the host and the stream is not synchronised.
 * sd_normalize_mi_ma_device: d_out[i] = (float32(x[i]) - mi) / (ma - mi + eps) with mi = d_mi[i % n_seg], ma = d_ma[i % n_seg] read from
 *   device memory, float32 operations in this order with a correctly rounded division; clip != 0: then limited to [0, 1] as np.clip does
 *   (NaN stays).  d_out may be d_x for float32 input. */
int sd_percentiles_device(const void* d_x, int dtype, long long n, int n_seg, const double* h_q, int n_q, int interp_f32, float* d_out,
                          void* stream);
int sd_normalize_mi_ma_device(const void* d_x, int dtype, long long n, int n_seg, const float* d_mi, const float* d_ma, float eps, int clip,
                              float* d_out, void* stream);

/* ---- linear resampling of an image (scipy.ndimage.zoom(x, zoom, order=1); csrc/zoom.hip, csrc/zoom_linear.h) ------------------
 * d_src: a contiguous array of shape h_in_shape[0 .. rank - 1], d_dst: one of shape h_out_shape (both shapes on the host, every extent
 * >= 1, 1 <= rank <= 4), of the same element type.  dtype: 0 = uint8, 1 = uint16, 2 = float32.  d_i0 / d_w0 / d_w1: the per-axis tables
 * on the device, axis after axis, h_out_shape[d] entries each: for output index k of the axis, i0 = the first source index (floor of the
 * source coordinate k * (n - 1) / (m - 1); -1 = the coordinate lies past the array, the output is 0) and the float64 weights of the
 * samples i0 and i0 + 1 (where i0 + 1 is the extent, the mirrored index is read instead, as scipy does; its weight is 0).  An i0 beyond
 * the source extent is clamped, so no table can make the kernel read outside d_src.  Float64 sum over the 2^rank samples in scipy's
 * order, each product and sum rounded on its own; float32 is rounded once at the end, integers are rounded half up and saturated.  With
 * the tables of stardist_amd.utils.zoom_linear the result equals scipy's bit for bit, non-finite pixels included (a NaN is a NaN: its
 * sign and payload are not defined).  One thread per output element, 64-bit offsets; nothing is copied to the host and the stream is
 * not synchronised.  d_dst must not be d_src. */
int sd_zoom_linear_device(const void* d_src, void* d_dst, int dtype, int rank, const int* h_in_shape, const int* h_out_shape,
                          const int32_t* d_i0, const double* d_w0, const double* d_w1, void* stream);

/* ---- label-image helpers: bounding boxes and hole filling (csrc/fill_holes.hip, csrc/fill_holes.h) ----------------------------
 * lbl (Z, Y, X) int32 label image (2D: Z = 1, and the z axis then takes no part), labels 1 .. max_label are objects, every other
 * value is background.  Bad arguments (a null pointer, a non-positive extent, a negative max_label) set the error string and return -1.
 * Nothing is copied to the host and the stream is not synchronised (the workspace grows on a first call of a larger size).
 *
 * Boxes, as scipy.ndimage.find_objects gives them: d_boxes is [max_label + 1][6] = z0, y0, x0, z1, y1, x1 with exclusive stops;
 * entry 0 and absent labels hold the sentinel INT_MAX, INT_MAX, INT_MAX, 0, 0, 0 (start > stop).  One pass over the image. */
int sd_label_boxes_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int32_t* d_boxes, void* stream);

/* replaces stardist.utils.fill_label_holes (stardist/utils.py:137-153, default structure): d_out = max(d_lbl, 0) (labels beyond
 * max_label: 0), and every pixel of a hole of label L = a 4- (6-) connected set of pixels != L inside L's bounding box that holds no
 * pixel of the box's outermost layer = gets max(d_out, L).  Integer arithmetic only, the same bits from call to call.  d_out must
 * not be d_lbl. */
int sd_fill_label_holes_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int32_t* d_out, void* stream);

/* ---- star representation of a label image's objects (csrc/relabel_star.hip, csrc/relabel_star.h): what relabel_image_stardist /
 * relabel_image_stardist3D (stardist/geometry/geom2d.py:200-211, geom3d.py:201-217) need besides the rasterisers ----------------
 * lbl (Z, Y, X) int32 label image as above (2D: Z = 1).
 *
 * Centroid sums: d_sums is [max_label + 1][4] int64 = pixel count, sum of z, sum of y, sum of x of every label 1 .. max_label; the
 * call zeroes it, entry 0 and absent labels stay 0 (every other value of lbl is background).  One pass over the image, 64-bit
 * integer arithmetic and 64-bit offsets: the same bits from call to call.  Bad arguments (a null pointer, a non-positive extent, a
 * negative max_label) set the error string and return -1.  Nothing is copied to the host and the stream is not synchronised. */
int sd_label_centroid_sums_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int64_t* d_sums, void* stream);

/* ---- intensity statistics of labelled objects (csrc/measure.hip, csrc/measure.h): the part of stardist_amd.utils.measure_labels that
 * reads the image; boxes, pixel counts and coordinate sums come from the two entry points above ------------------------------------
 * lbl (Z, Y, X) int32 label image as above (2D: Z = 1); d_boxes: the table sd_label_boxes_device wrote for this lbl and max_label (it
 * is read on the device; every box is clamped to the image, so no table can make the kernels read outside d_lbl or d_img).  d_img:
 * (Z, Y, X, C) contiguous, channels last, 1 <= C <= 64; dtype: 0 = uint8, 1 = uint16, 2 = float32.  Over the pixels p of label l, with
 * v = img[p][c]:
 *   integer images  d_isum2[l][c] = {sum v, sum v * v} in int64 (exact, also beyond 2^53); d_minmax[l][c] = {min, max} as int32;
 *                   d_fsum2 is not used and may be null
 *   float32 images  d_fsum2[l][c] = {sum double(v), sum double(v) * double(v)} in float64 (every square is exact); d_minmax[l][c] =
 *                   {min, max} as float32; d_isum2 is not used and may be null
 * Every table is [max_label + 1][C][2] and the call writes every row: row 0 and the rows of absent labels hold the sentinel, sums 0
 * and {min, max} = {INT32_MAX, INT32_MIN} or {+inf, -inf}.  A NaN pixel makes sum, sum of squares, min and max of its object and
 * channel NaN (as numpy's do); +-inf follow IEEE (+inf and -inf in one object: the sums are NaN, min and max the infinities).
 * The float64 sums are added in the fixed order csrc/measure.h states -- per-lane sums over the flattened (row, x) index of the box, a
 * fixed cross-lane tree, a box of more than 65536 pixels in chunks of whole rows whose results are added in chunk order -- with no
 * floating-point atomic anywhere: they depend on (extents, lbl, img) alone, the same bits from call to call, from process to
 * process and on any grid.  64-bit offsets.  Bad arguments set the error string and return -1 before anything is launched: a null
 * d_lbl, d_boxes, d_img or d_minmax, a null sum table of the dtype's kind, a non-positive extent, a negative max_label, a dtype outside
 * 0 .. 2, C outside 1 .. 64, more than 2^40 pixels or Z * Y beyond int.  Nothing is copied to the host and the stream is not
 * synchronised (the workspace grows on a first call of a larger size). */
int sd_label_intensity_stats_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const void* d_img,
                                    int dtype, int C, int64_t* d_isum2, double* d_fsum2, void* d_minmax, void* stream);

/* ---- exact intensity percentiles of labelled objects (csrc/measure_rank.hip, csrc/measure_rank.h): the columns of
 * stardist_amd.utils.measure_labels(percentiles=) -----------------------------------------------------------------------------------
 * lbl, d_boxes, d_img, dtype and C as for sd_label_intensity_stats_device (every box is clamped to the image, and the kernels count an
 * object's pixels themselves while they read its box: no table can make them read or write outside their buffers).  h_q: n_q
 * percentiles in [0, 100] on the host, 1 <= n_q <= 8.  d_out is [max_label + 1][C][n_q] float64 and the call writes every entry:
 *   d_out[l][c][j] = np.percentile(v, h_q[j]) (method 'linear') of the values v of label l in channel c, bit for bit: exact order
 *   statistics, then numpy's interpolation between the two neighbouring ones.  Integer images interpolate in float64.  float32 images:
 *   interp_f32 = 1: virtual index, weight and interpolation in float32 -- what numpy >= 2.0 does for float32 data and a Python-scalar q;
 *   0: in float64, rounded to float32 at the end; either way the entry is the float32 result widened to double.
 *   Row 0 and the rows of absent labels hold NaN.  A NaN among an object's values of a channel makes that object's entries of that
 *   channel NaN, and only those; +-inf follow numpy's interpolation (inf - inf = NaN).
 * Per object: a box of at most 1024 pixels has its keys compacted into LDS and sorted there by one wave; a larger box of at most 65536
 * pixels gets one radix-selection pass per 8-bit digit by one workgroup; the chunks of a larger box are spread over the grid, their
 * counts merged by 64-bit integer atomics in a workspace of 128 (object, channel) slots, beyond which an object falls back to the single
 * workgroup.  Counting is in integers only, without floating-point atomics: the result depends on (extents, lbl, img, q) alone, the
 * same bits from call to call and on any grid.  64-bit offsets.  Bad arguments set the error string and return -1 before anything is
 * launched: a null pointer, a non-positive extent, a negative max_label, a dtype outside 0 .. 2, C outside 1 .. 64, n_q outside 1 .. 8,
 * a q outside [0, 100] or not finite, more than 2^40 pixels or Z * Y beyond int.  The inputs are not written, nothing is copied to the
 * host and the stream is not synchronised (the workspace grows on a first call of a larger size). */
int sd_label_percentiles_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const void* d_img,
                                int dtype, int C, const double* h_q, int n_q, int interp_f32, double* d_out, void* stream);

/* ---- shape tables of labelled objects (csrc/measure_shape.hip, csrc/measure_shape.h): the integer sums behind the shape columns of
 * stardist_amd.utils.measure_labels(shape=True) -- inertia tensor, axis lengths, eccentricity, orientation, perimeter, Crofton perimeter,
 * Euler number ----------------------------------------------------------------------------------------------------------------------
 * lbl (Z, Y, X) int32 label image as above (2D: Z = 1): labels 1 .. max_label are objects, every other value is background.  Both calls
 * write every row of their table; row 0 and the rows of absent labels are 0.  The input is not written.  Integer arithmetic only
 * (64-bit integer atomics, no floating point anywhere), 64-bit offsets: the tables depend on the input alone, the same bits from call
 * to call.  Bad arguments (a null pointer, a non-positive extent, a negative max_label, more than 2^40 pixels) set the error string and
 * return -1 before anything is launched.  Nothing is copied to the host and the stream is not synchronised.
 *
 * Moment sums: d_boxes is the table sd_label_boxes_device wrote for this lbl and max_label (read on the device, every box clamped to
 * the image).  With u_d = coordinate_d - box start_d, d_m2 is [max_label + 1][6] = sum of u_z u_z, u_z u_y, u_z u_x, u_y u_y, u_y u_x,
 * u_x u_x over the pixels of the label (2D: the three z entries are 0).  The caller keeps numel * max(extent)^2 below 2^63. */
int sd_label_moment_sums_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, int64_t* d_m2, void* stream);

/* Contour counts of a 2D label image: d_counts is [max_label + 1][18] = n_1, n_r2, n_h, h_1 .. h_15.
 *   A border pixel of label l is a pixel of l with a 4-neighbour that is not l (outside the image and other labels are not l).  With
 *   a / d = the number of its 4- / diagonal neighbours that are border pixels of l, it counts into n_1 for (a, d) in {(2,0), (3,0), (2,1),
 *   (3,1), (2,2), (3,2)}, into n_r2 for {(0,2), (1,3)}, into n_h for {(1,1), (1,2)}, else into nothing: the three classes of
 *   skimage.measure.perimeter(mask, 4), whose value is n_1 + sqrt(2) n_r2 + (1 + sqrt(2)) / 2 n_h.
 *   h_code counts the 2 x 2 windows at the positions i in [0, Y], j in [0, X] in which l has the configuration code = 1 [L(i,j) = l] +
 *   2 [L(i-1,j) = l] + 4 [L(i,j-1) = l] + 8 [L(i-1,j-1) = l]: the histogram of skimage.measure.perimeter_crofton(mask, 4) and
 *   euler_number(mask, 2) (= h_8 - h_6 - h_14). */
int sd_label_contour_counts_device(const int32_t* d_lbl, int Y, int X, int max_label, int64_t* d_counts, void* stream);

/* ---- hull table of labelled objects (csrc/measure_hull.hip, csrc/measure_hull.h): the two integers behind the hull columns of
 * stardist_amd.utils.measure_labels(hull=True) -- convex_area, solidity, feret_diameter_max of scikit-image 0.18 ---------------------
 * lbl (Y, X) int32 label image of a 2D image: labels 1 .. max_label are objects, every other value is background; d_boxes is the table
 * sd_label_boxes_device wrote for this lbl and max_label (read on the device, every box clamped to the image; a row outside its
 * label's box is ignored).  d_hull is [max_label + 1][2] = convex_area, F2; every row is written, row 0 and absent labels are 0.
 *   In doubled coordinates pixel (r, c) has the centre (2 r, 2 c) and the diamond points (2 r +- 1, 2 c), (2 r, 2 c +- 1).  H = the
 *   convex hull of the diamond points of the pixels of l; the convex image = the pixels whose centre lies in H or on its boundary;
 *   convex_area = their number (pixels of other labels count); F2 = the largest squared distance between two diamond points of the
 *   convex image's pixels, so that feret_diameter_max = sqrt(F2 / 4).
 * Integer arithmetic only (int32 coordinates, int64 products, integer min / max atomics), 64-bit offsets: the table depends on the
 * input alone.  Bad arguments (a null pointer, a non-positive extent, an extent of 2^30 or more, a negative max_label, more than 2^40
 * pixels) set the error string and return -1 before anything is launched.  Two scalars, the summed heights of the boxes and the
 * workspace of the objects too tall for LDS, come to the host to size the row table: the stream is synchronised once. */
int sd_label_hull_device(const int32_t* d_lbl, int Y, int X, int max_label, const int32_t* d_boxes, int64_t* d_hull, void* stream);

/* ---- connected components (csrc/label_cc.hip, csrc/label_cc.h): what skimage.measure.label(img, background, connectivity) and, for a
 * mask, scipy.ndimage.label(mask, generate_binary_structure(ndim, connectivity)) compute ----------------------------------------------
 * d_img: (Z, Y, X) contiguous image (2D: Z = 1); dtype: 0 = uint8 (a bool mask travels as uint8), 1 = uint16, 3 = int32 (the codes above;
 * 2, float32, is not taken).  Two pixels are joined when they are neighbours, their values are equal and that value is not `background`
 * (a background that is no value of the dtype makes every pixel foreground).  Neighbours: the offsets (dz, dy, dx) in {-1, 0, 1}^3 with
 * at most `connectivity` (1 .. 3) non-zero coordinates, i.e. 6, 18 or 26 of them; with Z = 1 this is the 2D rule for connectivity 1
 * (4 neighbours) or 2 (8).  d_out (Z * Y * X int32, not d_img) serves as the parent array first and then holds the result: 0 for
 * background, ids 1 .. n in raster (C) order of each component's first pixel; d_count receives n.  A tiled union-find whose parent of a
 * pixel never exceeds the pixel's own linear index, so that every loop ends without an iteration cap, and whose roots are the
 * components' smallest indices: integer arithmetic only, the result depends on the input alone, the same bits from call to call.
 * d_img is not written.  Bad arguments set the error string and return -1 before anything is launched: a null pointer, a
 * non-positive extent, connectivity outside 1 .. 3, another dtype, more than 2^31 - 1 pixels.  Nothing is copied to the host and the
 * stream is not synchronised (the workspace, one int per pixel, grows on a first call of a larger size). */
int sd_label_components_device(const void* d_img, int dtype, int Z, int Y, int X, int connectivity, long long background, int* d_out,
                               int* d_count, void* stream);

/* ---- nearest-feature transform (csrc/edt_feature.hip, csrc/edt_feature.h): scipy.ndimage.distance_transform_edt with indices, exactly -
 * d_img: (Z, Y, X) contiguous image (2D: Z = 1, the z axis then takes no part); dtype: 0 = uint8, 1 = uint16, 3 = int32, as above.  The
 * features are the pixels != 0, or with feature_is_zero = 1 the pixels == 0 (distance_transform_edt's orientation).  For a pixel p and
 * a feature q, D(p, q) = ((sz dz)^2 + (sy dy)^2) + (sx dx)^2 in float64, every operation rounded on its own, each term t = s * d; t * t
 * -- scipy's floats.  nearest(p) is the feature of smallest D; among equal D the smallest x wins, then the smallest y, then the
 * smallest z (scipy's choice); a feature is its own nearest feature.  d_index[p] (int32, may be null) = the linear index of nearest(p),
 * d_dist[p] (float64, may be null) = sqrt(D(p, nearest(p))).  max_distance < 0 or inf: no bound; otherwise a pixel with
 * dist > max_distance, like every pixel of an image without features, gets index -1 and distance +inf, and no scan goes farther than
 * the bound.  A separable pass per axis in scipy's order, outward scans that stop when the axis term alone exceeds the best value:
 * no atomics, the result depends on the input alone, the same bits from call to call; the time follows the largest distance in the
 * result (or the bound).  d_img is not written.  Bad arguments set the error string and return -1 before anything is launched: a null
 * image, a non-positive extent, more than 2^31 - 1 pixels, a spacing that is not positive and finite, a NaN max_distance,
 * feature_is_zero outside 0 / 1, another dtype.  Nothing is copied to the host and the stream is not synchronised (the workspace, 12 B
 * per pixel, 24 B for a volume, grows on a first call of a larger size). */
int sd_nearest_feature_device(const void* d_img, int dtype, int Z, int Y, int X, int feature_is_zero, double sz, double sy, double sx,
                              double max_distance, int32_t* d_index, double* d_dist, void* stream);

/* skimage.segmentation.expand_labels(lbl, distance, spacing) on the transform above: d_out[p] (Z * Y * X int32, not d_lbl) =
 * d_lbl[nearest(p)] if sqrt(D) <= distance -- compared on the square root, as scikit-image does -- and 0 otherwise, the features being
 * the pixels with d_lbl != 0 (negative labels too).  distance = 0 copies; distance = inf has no bound.  d_lbl is not written.  -1
 * before any launch for a null pointer, d_out == d_lbl, a non-positive extent, more than 2^31 - 1 pixels, a spacing that is not
 * positive and finite, a distance that is negative or NaN.  Nothing is copied to the host, the stream is not synchronised. */
int sd_expand_labels_device(const int32_t* d_lbl, int Z, int Y, int X, double sz, double sy, double sx, double distance, int32_t* d_out,
                            void* stream);

/* ---- label clean-up (csrc/label_edit.hip, csrc/label_edit.h): the device halves of stardist_amd.utils.find_boundaries, clear_border and
 * remove_small_objects, i.e. of skimage.segmentation.find_boundaries / clear_border and skimage.morphology.remove_small_objects (0.18) --
 * Images are (Z, Y, X) contiguous int32 (2D: Z = 1, the z axis then takes no part).  Integer arithmetic only, 64-bit offsets, no
 * atomics: every result depends on the input alone, the same bits from call to call.  No input is written.  Bad arguments set the
 * error string and return -1 before anything is launched: a null pointer, a non-positive extent or table size, an output that is an
 * input, more than 2^31 - 1 pixels, and what each entry names.  Nothing is copied to the host and the stream is not synchronised.
 *
 * Boundaries: d_out[p] (uint8) = 1 where p is a boundary pixel, else 0.  With N_c(p) = the in-image neighbours of p whose offsets have at
 * most `connectivity` (1 .. 3; with Z = 1, 2 and 3 are the same) non-zero coordinates -- a neighbour outside the image does not exist --
 *   mode 0 (thick)  some q in N_c(p) has lbl[q] != lbl[p]
 *   mode 1 (inner)  thick and lbl[p] != background
 *   mode 2 (outer)  thick and (lbl[p] == background or the maximum of lbl over W(p) != the minimum of lbl' over W(p)), W(p) = p and all its
 *                   in-image neighbours (full connectivity whatever `connectivity` is), lbl' = lbl with every background pixel replaced
 *                   by `sentinel` (scikit-image takes the largest value of the image's dtype)
 * background and sentinel are compared as 64-bit values, so either may lie outside int32.  One workgroup per tile, the tile with a halo
 * of 1 in LDS: one read of the labels, one byte written per pixel.  Also -1 for a connectivity or a mode outside its range. */
int sd_find_boundaries_device(const int32_t* d_lbl, int Z, int Y, int X, int connectivity, int mode, long long background, long long sentinel,
                              uint8_t* d_out, void* stream);

/* Border flags: d_flags (n_flags bytes; the call zeroes it) gets d_flags[k] = 1 for every key k = d_key[p] in 0 .. n_flags - 1 -- the
 * component image of sd_label_components_device, 0 being the background -- of a pixel p that
 *   d_mask == NULL  lies within buffer_size + 1 (buffer_size >= 0) of an image edge along y or x, and with ndim = 3 along z too (ndim = 2
 *                   needs Z = 1); only these pixels are visited
 *   d_mask given    has d_mask[p] == 0 (uint8, (Z, Y, X)); one pass over the mask, buffer_size is ignored
 * A key outside the table is ignored.  Every writer stores the same 1 with a vector store, so the order of the stores does not matter.
 * Also -1 for ndim outside 2 / 3 and for a negative buffer_size. */
int sd_label_border_flags_device(const int32_t* d_key, int Z, int Y, int X, int ndim, int buffer_size, const uint8_t* d_mask, long long n_flags,
                                 uint8_t* d_flags, void* stream);

/* Clear what is flagged: d_out[p] = d_flags[d_key[p]] ? bgval : d_val[p] over n pixels (a key outside 0 .. n_flags - 1 counts as not
 * flagged).  d_key is the component image (clear_border) or d_val itself (remove_small_objects, whose flags say "fewer than min_size
 * pixels", from the counts of sd_label_centroid_sums_device).  One read of each image, one write; 16-byte accesses where the
 * pointers and n allow. */
int sd_label_clear_flagged_device(const int32_t* d_val, const int32_t* d_key, const uint8_t* d_flags, long long n_flags, long long n, int bgval,
                                  int32_t* d_out, void* stream);

/* ---- label contacts (stardist_amd.utils.label_contacts, measure_labels(neighbors=); csrc/label_contacts.hip) ----
 * d_lbl: an int32 label image of rank ndim = 2 (Z = 1) or 3 with extents Z, Y, X; connectivity in 1 .. ndim.  A contact is a pair of
 * pixels (p, p + o), o one of the lexicographically positive offsets with at most `connectivity` non-zero coordinates, both inside the
 * image, whose labels differ.  Result: every unordered pair {a, b}, a < b, of labels with at least one contact, ascending by (a, b), as
 * d_keys[i] = a << 32 | b and d_counts[i] = its number of contacts; the pairs with a = 0 (the background) only with
 * with_background != 0.  Buffer protocol of sd_label_overlap_device: *h_count (host) receives the number of pairs, the first
 * min(*h_count, cap) of them are written (cap = 0 with NULL buffers is a pure count query).  h_minmax (host, 2 ints) receives {min, max}
 * of d_lbl ({0, 0} for an extent <= 0, which is no error and gives no pair); if the minimum is negative nothing else is computed and
 * *h_count = 0.  h_runs (host, may be NULL) receives the number of (key, length) runs the append pass wrote, before they are reduced:
 * the sum of d_counts is the number of contacts, so runs < sum says that lanes were combined.  Integer arithmetic only: the table is
 * bit-identical from call to call.  Synchronises the stream, as sd_label_overlap_device does: once for the number of runs, which sizes
 * the sort, and once for the size of the table.  At most 2^31 - 1 runs; extents up to 2^31 - 1 - 128, their product is not bounded.
 * -1 also for a rank or connectivity outside its range. */
int sd_label_contacts_device(const int32_t* d_lbl, int ndim, int Z, int Y, int X, int connectivity, int with_background, long long cap,
                             int64_t* d_keys, int64_t* d_counts, long long* h_count, int32_t* h_minmax, long long* h_runs, void* stream);

/* ---- point neighbours (stardist_amd.utils.point_neighbors, measure_labels(nearest=, within=); DESIGN.md section 3v;
 * csrc/point_neighbors.hip) ----
 * d_points (n, nd) and d_queries (m, nd) float64, nd = 2 or 3, already scaled by the caller; d_queries = NULL (then m = n): the points
 * are their own queries and query i skips point i, and only that one.  d2(q, p) = ((q0 - p0)^2 + (q1 - p1)^2) + (q2 - p2)^2, every
 * operation rounded in float64, no fused multiply-add; candidates are ordered by (d2, index); with use_radius a candidate needs
 * d2 <= r2 (the caller forms r2 = fl(radius * radius)).  Results hold d2, not its root.
 *   mode 0   d_indices, d_d2 (m, k), k in 1 .. 64: the first k candidates of every query, -1 / +inf where there are fewer
 *   mode 1   d_offsets (m): the number of candidates of every query (needs use_radius); nothing else is written
 *   mode 2   d_offsets (m + 1): the exclusive sums of those numbers, *h_total (host) the last of them; if 0 < *h_total <= cap, d_indices
 *            and d_d2 (cap entries each) receive row i at d_offsets[i] .. d_offsets[i + 1], ascending by index; a caller that
 *            finds *h_total > cap comes again with room (cap = 0 with NULL lists is a pure size query)
 * cell_size: 0 lets the library choose the edge of the grid's cells from the points' box and n, about two points per cell; a value
 * in [2^-500, 2^500] is taken as given (-1 if that makes more than 2^21 cells along an axis or 2^27 in all).  *h_cell (host, may be
 * NULL) receives the edge used.  The result does not depend on the cell size.  Synchronises the stream once, to read the box of the
 * points (128 x 6 doubles), and in mode 2 once more for the total.  No atomics: the same bits from call to call.  n = 0 or m = 0 is no
 * error (mode 0 fills -1 / +inf, the others zeros).  -1 also for nd, mode or k outside their range, n or m beyond 2^31 - 2, a radius
 * mode without use_radius, r2 < 0 or NaN, a cell size outside its range, a point coordinate that is not finite or not below 2^500 in
 * magnitude (the queries are the caller's to check), a missing buffer.  Time grows with the fullest cells: one far outlier that
 * stretches the box can leave all other points in one cell (correct, but quadratic), and a query far from everything walks up to
 * every cell once. */
int sd_point_neighbors_device(const double* d_points, long long n, const double* d_queries, long long m, int nd, int mode, int k,
                              int use_radius, double r2, double cell_size, long long cap, int64_t* d_indices, double* d_d2,
                              int64_t* d_offsets, long long* h_total, double* h_cell, void* stream);

/* Spot detection (stardist_amd.spots; the per-element rules are csrc/spots.h's).  An image is nd = 2 or 3 axes of
 * extents n0, n1, n2 (n0 = 1 for nd = 2), at most 2^32 - 1 pixels, dtype 0 uint8, 1 uint16, 2 float32; it is never written.
 *
 * sd_gaussian_filter_device: scipy.ndimage.gaussian_filter(img, output=float32, mode="reflect") bit for bit (NaN positions; not their
 * payload).  h_radius (host, 3 ints, z y x): the window's radius per axis, < 0 for an axis that is skipped, at most 512.  d_weights:
 * the float64 tables of the axes that are not skipped, one after the other in axis order, 2 r + 1 entries each, w[r] the centre.  One
 * output element of a line: tmp = in[l] w[r]; for j = r .. 1: tmp += (in[l - j] + in[l + j]) w[r - j], in double, every operation
 * rounded, indices reflected with period 2 n; stored as float.  Axes in the order 0, 1, 2; between axes the image is float32.  d_out
 * receives the result, d_work (as large; needed for two or three passes) is scratch.  With every axis skipped d_out is the cast.
 * A pass along the last axis keeps its tile and halo in LDS always, a pass along another axis up to r = 80 and reads global memory
 * beyond.  No read-back, no synchronisation.
 *
 * sd_peak_local_max_device: the peaks of stardist_amd.spots.peak_local_max's definition.  h_distance (host, 3 ints): min_distance per
 * axis, 0 .. 2^20; h_border (host, 3 long long): the border width per axis, >= 0.  d_labels: int32 like the image, or NULL.  The
 * threshold is threshold_abs if has_abs else the least non-NaN value, raised to fl64(threshold_rel * greatest non-NaN value) if
 * has_rel; it is computed and read on the device.  per_label < 0: no per-label cap (it needs d_labels); num_peaks < 0: no cap.
 * d_keys (cap entries) receives the keys ((~value key) << 32 | raster index), ascending, which is (-value, index) ascending;
 * h_count[0] (host) the number of peaks found before the cuts, h_count[1] the number of keys that are the result, or -1 if
 * h_count[0] > cap: nothing is delivered then, and the caller comes again with room for all.  The halo of a tile lives in LDS while
 * (t0 + 2 d0) (t1 + 2 d1) (64 + 2 d2) floats fit in 48 KiB (tiles 1 x 16 x 64, 3D 4 x 4 x 64: d <= 36 for a 2D image and one d),
 * beyond that the window is read from global memory.  Synchronises the stream once for h_count[0] and, with a per-label cap, once
 * more.  Integer atomics only: the same keys from call to call.
 *
 * sd_peaks_emit_device: for the first `count` keys, d_coords (count x nd int64), d_values (count, the image's dtype, the pixel's own
 * bits) and d_out_labels (count int32; zeros without d_labels).  No synchronisation.
 *
 * All three return -1 before any launch for a null pointer, nd outside 2 .. 3, a dtype code outside 0 .. 2, an extent < 1, more
 * than 2^32 - 1 pixels, a radius beyond 512 / a distance beyond 2^20, a negative border or a NaN threshold. */
int sd_gaussian_filter_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int* h_radius,
                              const double* d_weights, float* d_out, float* d_work, void* stream);
int sd_peak_local_max_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int32_t* d_labels,
                             const int* h_distance, const long long* h_border, int has_abs, double threshold_abs, int has_rel,
                             double threshold_rel, long long per_label, long long num_peaks, long long cap, uint64_t* d_keys,
                             long long* h_count, void* stream);
int sd_peaks_emit_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int32_t* d_labels,
                         const uint64_t* d_keys, long long count, int64_t* d_coords, void* d_values, int32_t* d_out_labels, void* stream);

/* Rank filters and grey morphology (stardist_amd.rank_filters; the per-element rules are csrc/rank_filter.h's).
 * Images as for spot detection: nd = 2 or 3 axes of extents n0, n1, n2 (n0 = 1 for nd = 2), at most 2^32 - 1 pixels, dtype 0 uint8
 * (bool images travel as uint8), 1 uint16, 2 float32; never written.  The output has the image's dtype.  mode: 0 reflect, 1 nearest,
 * 2 mirror, 3 constant -- scipy.ndimage's index rules, for windows longer than the axis as well; cval (mode 3) must be a value of the
 * dtype and not NaN.  Along an axis a window of `size` elements starts size / 2 + origin elements before the output position
 * (scipy's origin; 0 <= size / 2 + origin < size).  A window that covers a NaN gives NaN; -0.0 sorts below +0.0.  Window lengths go
 * up to 1025 per axis, footprints up to 4096 elements.  No atomics, no read-back, no synchronisation: the same bits from call to call.
 *
 * sd_minmax_box_device: minimum_filter (is_max = 0) or maximum_filter (is_max = 1) under a box: h_size and h_origin (host, 3 ints,
 * z y x; a 2D image has size 1 on axis 0), one separable pass per axis whose size is not 1, in the order 0, 1, 2.  fuse_op applies to
 * what the last pass would store, x, and the pixel r of d_ref (an image like d_in): 0 x, 1 r - x, 2 x - r (both in the dtype; unsigned
 * types wrap), 3 x ^ r (uint8 only) -- the top-hats' last step.  d_out receives the result, d_work (as large; needed for two or three
 * passes) is scratch; d_in, d_ref, d_out and d_work are distinct.  A pass keeps its tile (1024 x 1 along the last axis, 32 x 64 along
 * another) with its halo in LDS while that fits in 48 KiB -- always along the last axis, along another up to size 737 / 353 / 161 for
 * uint8 / uint16 / float32 -- and reads global memory beyond.
 *
 * sd_rank_filter_device: the rank-th smallest (0-based, 0 <= rank < count) of the `count` pixels under a footprint of extents
 * h_extent (host, 3 ints) whose true elements are h_offsets (host, count x 3 ints (dz, dy, dx), each inside its extent; copied to the
 * device on the stream).  Selection is a bisection over the key's bits (8 / 16 / 32 walks over the window); rank 0 and count - 1 are
 * one walk.  The tile (1 x 16 x 64, 3D 4 x 4 x 64) with the footprint's halo lives in LDS while it fits in 48 KiB, else the window is
 * read from global memory.  d_out is not d_in.
 *
 * Both return -1 before any launch for a null pointer, nd outside 2 .. 3, a dtype, mode or fuse code outside its range, an extent < 1,
 * more than 2^32 - 1 pixels, a window length outside 1 .. 1025, an origin outside its window, a cval that is NaN or no value of the
 * dtype, count outside 1 .. 4096, a rank outside 0 .. count - 1, an offset outside its extent, buffers that are not distinct. */
int sd_minmax_box_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int* h_size,
                         const int* h_origin, int is_max, int mode, double cval, int fuse_op, const void* d_ref, void* d_out,
                         void* d_work, void* stream);
int sd_rank_filter_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int* h_extent,
                          const int* h_origin, const int* h_offsets, int count, int rank, int mode, double cval, void* d_out,
                          void* stream);

/* The augmentation chain of a training batch (stardist_amd.augment.Compose.apply_device; the rules are csrc/augment.h's) in ONE launch:
 * d_x (B, *shape) float32 and d_y (B, *shape) int32, nd = 2 or 3 extents in h_shape, give d_out_x and d_out_y of the same shapes
 * (not the inputs): per sample FlipRot90 (always, as an index map), then Warp (flags bit 0; bit 1: mode 'reflect', else 'constant'),
 * then on the image IntensityScaleShift (bit 2) and AdditiveNoise (bit 3).  The table holds one 168-byte row per sample (struct
 * augment::Sample): h_table on the host, read here to check that every index map stays inside its patch, d_table the same bytes on
 * the device, uploaded by the caller in one copy.  d_disp: (B, n_disp, *shape) float32 displacements added to the warp coordinates of
 * the axes a row names, or NULL with n_disp = 0.  Equal to the host route (numpy, scipy.ndimage.map_coordinates of order 1 / 0) bit
 * for bit, NaN for NaN; no atomics, the same bits from call to call.  -1 before the launch for a null pointer, an output that is an
 * input, nd outside 2 / 3, B outside 1 .. 65535, an extent < 1, more than 2^31 - 1 pixels per sample, unknown flags, a displacement
 * field without a Warp, a row whose map leaves the patch.  Nothing is copied to the host, the stream is not synchronised. */
int sd_augment_batch_device(const float* d_x, const int32_t* d_y, int B, int nd, const int* h_shape, int flags, const void* h_table,
                            const void* d_table, const float* d_disp, int n_disp, float* d_out_x, int32_t* d_out_y, void* stream);

/* Star distances at given pixels only: d_points (n, 2) [(n, 3)] int64 pixel coordinates (y, x) [(z, y, x)], d_dist (n, n_rays) float32.
 * Row p is the row of sd_star_dist2d_device [sd_star_dist3d_device] (grid 1) at that pixel, bit for bit -- 0 for a background pixel --
 * with one difference in what is read: the labels are int32 and are compared by their low 16 bits, the cast to unsigned short that the
 * reference and the dense entry points' callers apply, so ids that agree modulo 65536 are one object to a ray and an id that is a
 * multiple of 65536 is background.  3D: d_dz / d_dy / d_dx are the rays' components (n_rays floats each) and the result is
 * max(dist, floor) (relabel_image_stardist3D clamps at 1e-3f; 0 = no clamp).  n = 0 returns 0 without a launch.  A point outside the
 * image gets a row of zeros and the call returns -1; so do a non-positive extent, a negative n, n_rays outside 1 .. 4096, a null
 * pointer and, in 3D, a ray that is zero or NaN in every component (its march would not end; its column is zeros).  The device entries read one flag back (the stream is synchronised); the _host entries take host arrays and compute on
 * the host, with the same code for the march (no device is touched). */
int sd_star_dist2d_points_device(const int32_t* d_lbl, int H, int W, const int64_t* d_points, int n, int n_rays, float* d_dist,
                                 void* stream);
int sd_star_dist3d_points_device(const int32_t* d_lbl, int Z, int Y, int X, const int64_t* d_points, int n, const float* d_dz,
                                 const float* d_dy, const float* d_dx, int n_rays, float floor, float* d_dist, void* stream);
int sd_star_dist2d_points_host(const int32_t* lbl, int H, int W, const int64_t* points, int n, int n_rays, float* dist);
int sd_star_dist3d_points_host(const int32_t* lbl, int Z, int Y, int X, const int64_t* points, int n, const float* dz, const float* dy,
                               const float* dx, int n_rays, float floor, float* dist);

#ifdef __cplusplus
}
#endif
#endif /* STARDIST_HIP_H */
