/*
 * coma_hip.h -- C ABI of libcoma_hip.so, the MI355X (gfx950) implementation of ComA's dense hot path.
 *
 * The reference (snuvclab/coma) has no native layer: its boundary for this path is a set of Python
 * methods on torch tensors.  Each entry point below replaces the tensor-op chain of one such method;
 * the citation after "replaces:" is the reference file:line (relative to the reference repo root).
 * The Python host mirror in coma_amd/ binds these with ctypes (see INTEGRATION.md for the stub a
 * reference maintainer would add to utils/coma.py).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (COMA_E_*); coma_last_error() gives the text
 *     (thread-local).  Nothing throws, nothing allocates device memory: the caller owns every
 *     buffer (device pointers unless stated) and passes the hipStream_t to launch on (NULL = default).
 *   - row-major, innermost index last.  H = #human vertices, O = #object points, N = #orientation
 *     bins, S = #samples in this call, R = voxels per axis.
 *   - "in/out" accumulators are added to, never overwritten, so calls compose over sample batches
 *     and an all-reduce(SUM) over ranks gives the single-process result.
 */
#ifndef COMA_HIP_H
#define COMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped when an existing signature of coma_hip.h / sd_hip.h / seg_hip.h changes; coma_amd/_lib.py refuses a library that
 * reports another value (a stale build loaded through COMA_HIP_LIB would otherwise be called with mismatched argument lists) */
#define COMA_ABI_VERSION 11  /* 11: seg_conv_gemm_describe added; seg_conv_gemm_f32 refuses a forced split_k whose slabs the workspace does not hold (it ran with fewer slices); 10: sd_conv_gemm_describe added; sd_conv_gemm_f16 refuses a column bias with SD_EPI_PERM16_N / SD_EPI_PERM32_N and colstats in a phase launch with in_h * in_w % 32 != 0 */
/* The version counts CHANGES of existing signatures, not additions: a function that is only added (the text tower, the sample
 * elimination, the rasteriser, the mesh volume functions, the coma_vposer_* and coma_angle_prior_* functions) leaves it alone, because a library without it already fails to load
 * (coma_amd/_lib.py binds every declared name).  An argument check that is only added (coma_occupancy_fused's window, thres_sq_cut
 * and alignment checks, coma_contact_accumulate_f32's limit on N, coma_occupancy_reduce's limit on R3) leaves it alone as well: the
 * call was outside the documented contract before, and is told so now. */

#define COMA_OK 0
#define COMA_E_INVALID (-1) /* bad argument (null pointer, non-positive size, unsupported shape) */
#define COMA_E_LAUNCH (-2)  /* HIP reported an error at launch */
#define COMA_E_DEVICE (-3)  /* no usable gfx950 device / runtime failure */

int coma_abi_version(void);
const char* coma_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * K1+K2+K3  fused contact / relative-orientation accumulator.
 * replaces: utils/coma.py:279-323 (ComA.aggregate_single_sample_for_contact) looped over samples as
 *           in utils/coma.py:257-268, with canonicalize_a_wrt_b_to_p (utils/coma.py:123-172),
 *           geodesic_gaussian_scores (:102-112) and negative_exp (:116-119) fused in.
 * human_verts/human_normals : f32 [S,H,3]
 * obj_verts/obj_normals     : f32 [S,O,3], or [O,3] shared by all samples when obj_sample_stride == 0
 *                             (obj_sample_stride is in floats: O*3 for per-sample objects)
 * sphere_grid               : f32 [N,3]   (the f32 rounding of get_uniform_points_on_sphere, :18-26)
 * principle_vec/sub_vec     : HOST pointers, 3 floats each
 * prob_h_wrt_o, prob_o_wrt_h: f32 [H,O,N] in/out ;  nom, den, cnt : f32 [H,O] in/out
 * Numerics: distance/threshold test bit-exact w.r.t. the reference's f32 sequence (cnt and den are exact); the histogram is
 * evaluated in f32 (reference: f64 intermediates rounded into f32 sums), parity <= 1e-3 relative.  The weights of one call are
 * summed in f32 as 2^64 * w and rescaled once, so a bin the reference keeps as an f32 denormal is kept here too.
 * S = 0 is accepted and writes nothing.  N <= 65535 * 256 (the 256-bin chunks walk grid y); a larger N is refused.
 * ------------------------------------------------------------------------------------------- */
int coma_contact_accumulate_f32(const float* human_verts, const float* human_normals,
                                const float* obj_verts, const float* obj_normals,
                                int64_t obj_sample_stride, const float* sphere_grid,
                                int S, int H, int O, int N,
                                const float* principle_vec, const float* sub_principle_vec,
                                float spatial_grid_size, float spatial_grid_thres,
                                float normal_gaussian_sigma, float eps,
                                float* prob_h_wrt_o, float* prob_o_wrt_h,
                                float* nom, float* den, float* cnt, void* stream);

/* K4a+K4b  normalise a histogram in place and reduce it to the per-pair contact map.
 * replaces: utils/coma.py:328-330 (normalize_prob_grid_for_normals, one grid) fused with
 *           utils/coma.py:342-356 (compute_contact_map, one of "human"/"obj").
 * prob [M,N] in/out (M = H*O) becomes prob/(sum_k prob + eps);
 * contact[m] = (sum_k prob[m,k] * (1 - p.n_k)/2) * nom[m]/den[m].   contact may be NULL
 * (normalise only). */
int coma_contact_map_f32(float* prob, const float* sphere_grid, const float* principle_vec /*host*/,
                         const float* nom, const float* den, int64_t M, int N, float eps,
                         float* contact, void* stream);

/* K4b  significant pairs + masked max.
 * replaces: utils/coma.py:376-377 (significant_contact_pairs) and :402-427
 *           (aggregate_contact_for_significant_pairs).
 * pairs u8 [H,O] = cnt >= threshold (threshold = f32(ratio * used_count), formed by the caller);
 * col_any u8 [O], row_any u8 [H] = any over the other axis;
 * which = 0 ("human"): out f32 [H] = max over {o : col_any[o]} contact[h,o], zeros if none
 * which = 1 ("obj")  : out f32 [O] = max over {h : row_any[h]} contact[h,o], zeros if none.
 * The maximum propagates NaN (np.max); elements of contact outside the mask are not read.  Every pointer is required. */
int coma_significant_pairs_u8(const float* cnt, float threshold, int H, int O, uint8_t* pairs,
                              uint8_t* col_any, uint8_t* row_any, void* stream);
int coma_masked_max_f32(const float* contact, const uint8_t* col_any, const uint8_t* row_any, int H,
                        int O, int which, float* out, void* stream);

/* K4c  negated normalised Shannon entropy of the (normalised) histogram.
 * replaces: utils/coma.py:328-330 + :455-463 / :467-475 (compute_nonphysical_response_sphere).
 * prob [M,N] in/out is normalised in place first; score[m] = 1 + sum_k plogp(round(p*n_bin)/n_bin)/ln(n_bin). */
int coma_entropy_f32(float* prob, int64_t M, int N, float eps, float n_bin, float* score, void* stream);

/* Consumer of the accumulator state: the optimisation app's target selection.
 * replaces: src/application/optimize.py:190-192 (`np.argmax(prob_grid_canon_human_wrt_obj[:, o_ref, :], axis=1)` -> the
 *           bin whose direction becomes the per-vertex orientation target) and :195-196 (`np.nonzero(np.max(nom / denom,
 *           axis=1) > contact_threshold)`, `np.argmax(nom[selected], axis=1)`).
 * coma_row_argmax_i64: idx[m] = argmax_k x[m*row_stride + col_offset + k] (k < n) with NumPy's rules -- the FIRST
 *   maximum, NaN counts as the maximum; val (optional) = that element (= np.max of the row).  idx or val may be NULL.
 * coma_contact_select_u8: selected[h] = (max_o nom[h,o]/den[h,o]) > threshold, NaN-propagating max (false). */
int coma_row_argmax_i64(const float* x, int64_t rows, int n, int64_t row_stride, int64_t col_offset, int64_t* idx,
                        float* val, void* stream);
int coma_contact_select_u8(const float* nom, const float* den, int H, int O, float threshold, uint8_t* selected,
                           void* stream);

/* K5  occupancy splat.
 * replaces: utils/coma_occupancy.py:287-295 (dense [H,R,R,R] f64 distance test) by an equivalent
 *           sparse test over the voxels whose centres can lie inside the threshold sphere.
 * q       : f32 [S,H,3] = f32(human_verts - obj_vert0), subtraction in f64 by the caller (:288-289)
 * centers : f64 [3,R] device; centers[c][i] = spatial_grid[c] at index i along axis c, i.e. the
 *           per-axis voxel centres exactly as load_voxelgrid builds them (:171 -- note the product
 *           voxel_size * f32(index) is rounded to f32 there, so the table is NOT start+voxel*(i+.5))
 * voxel   : centre spacing (2.4/R), used only to bound the candidate box
 * thres   : voxel*scale_tolerance (:242), the f64 threshold of the test d < thres
 * counts  : f32 [H,R,R,R] in/out; integer-valued, bit-exact (f64 distance, (x+y)+z order) while a cell stays below 2^24.
 * A sample with a NaN or infinite coordinate hits no cell.  S = 0 is accepted and writes nothing. */
int coma_occupancy_splat(const float* q, int S, int H, int R, const double* centers, double voxel,
                         double thres, float* counts, void* stream);

/* K6  occupancy reducer.
 * replaces: utils/coma_occupancy.py:297-312 (normalize_prob_grid_for_spatials + max over humans).
 * counts [H,R3] in/out -> counts/rowsum (no eps: an empty row becomes NaN, as in the reference);
 * select u8 [H] or NULL (= all) picks the rows the max runs over; out f32 [R3];
 * rowsum f32 [H] is scratch/output.  NaN propagates like torch.max.  A select without any row set leaves out = -inf everywhere.
 * rowsum is an f32 sum of the cells in the kernel's own order: exact, hence equal to coma_occupancy_fused's, while the row's hit
 * total is below 2^24; above that it is one of several roundings and the quotients follow it.
 * With R3 % 4 == 0 and counts and out both 16-byte aligned the cells go four at a time; any other R3 or alignment is accepted
 * and takes the one-cell kernels, same bits.  R3 needing more than 2^31 - 1 workgroups is refused. */
int coma_occupancy_reduce(float* counts, const uint8_t* select, int H, int64_t R3, float* rowsum,
                          float* out, void* stream);

/* K5 + K6 fused (SURVEY.md 8d structure B): zero grid -> splat all S samples -> normalise -> max over humans, the per-vertex
 * grid written once.  replaces: utils/coma_occupancy.py:272-312 for the usual "register every sample, aggregate, reduce" order;
 * afterwards counts holds the normalised grid exactly as return_aggregated_spatial_grids leaves it (write_raw = 0) or the raw
 * counts the reference exports before reducing (write_raw = 1; the max is over the normalised values either way), rowsum the
 * hit totals.
 * thres_sq_cut : the smallest double x with sqrt(x) >= thres (host: step ulps from thres*thres), so that the kernel's
 *                (dx^2+dy^2)+dz^2 < thres_sq_cut is bit-for-bit the reference's sqrt(...) < thres;
 * window       : candidate cells per axis, >= the number of voxel centres an open interval of length 2*thres (+ the 0.01-voxel
 *                margins) can contain: ceil(2*scale_tolerance) + 2;
 * workspace    : coma_occupancy_fused_workspace_bytes(S, H, R, window) bytes of device scratch (16 bytes per (vertex, sample) + 4 bytes per
 *                (vertex, sample, window plane) + the per-group maxima).  R*R % 4 == 0, R*R <= 20480: the latter binds before the
 *                R <= 255 of the 8-bit cell indices, so R <= 142 in effect.
 * Refused (COMA_E_INVALID): a window whose power-of-two rounding is below ceil(2*thres/voxel - 1e-9) + 2 (hits past the first
 * `window` cells of a range would be dropped from the grid and the row sum alike); a thres_sq_cut that is not the cut of thres
 * (checked with two host sqrt); counts, out or workspace not 16-byte aligned (all three are accessed 16 bytes at a time).
 * counts is overwritten (every cell, every row), not added to.  A select without any row set leaves out = -inf everywhere, as in
 * coma_occupancy_reduce.  A sample with a NaN or infinite coordinate hits no cell.  rowsum[h] is the correctly rounded f32 of the
 * exact integer hit total (a 32-bit count: S * window^3 < 2^32) and every quotient the correctly rounded f32 division by it, also
 * above 2^24, where coma_occupancy_reduce's f32 row sum may round differently (reachable from about 11 700 samples at
 * scale_tolerance 7). */
size_t coma_occupancy_fused_workspace_bytes(int S, int H, int R, int window);
int coma_occupancy_fused(const float* q, int S, int H, int R, const double* centers, double voxel, double thres,
                         double thres_sq_cut, int window, const uint8_t* select, int write_raw, float* counts, float* rowsum,
                         float* out, void* workspace, size_t workspace_bytes, void* stream);

/* K7  nearest-vertex index map (first minimum wins ties).
 * replaces: utils/coma.py:87-91 (argmin over f64 squared distances).
 * points f64 [P,3], verts f64 [V,3] -> idx i64 [P]; bit-exact against np.argmin of ((dx^2 + dy^2) + dz^2), its NaN rule included:
 * a NaN distance counts as the minimum and the first one wins; a row of +inf distances gives 0.  P = 0 writes nothing. */
int coma_nearest_vertex_i64(const double* points, const double* verts, int P, int V, int64_t* idx,
                            void* stream);

/* Two-view DLT triangulation + candidate scoring.
 * replaces: src/generation/optimize_depth.py:202-237 (solve_DLT) and :291-295 (reprojection MSE in both views).
 * views f64 [n_views][28]: per camera {rot[9], trans[3]} of get_projection_matrix (:164-183), {mr[9] = R C, tmr[3] = t R C} of
 * get_view2joints_render (:185-200), scale, max(resolution), resolution/2 (x, y) -- built on the host with the reference's own
 * expressions.  ref_xy f64 [J,2] pixel joints of the reference view; cand_view i32 [P], cand_xy f64 [P,J,2] ->
 * tri f64 [P,J,3], ref_mse / other_mse f64 [P].  <= 1e-9 relative against np.linalg.pinv on well-conditioned pairs.
 * cand_view lives on the device and is followed as given: every entry must lie in [0, n_views), which is the caller's to validate
 * (coma_amd/triangulate.py does, on the host, before the launch).  P = 0 writes nothing. */
int coma_dlt_score_f64(const double* views, int n_views, int ref_view, const double* ref_xy, const int* cand_view,
                       const double* cand_xy, int P, int J, double* tri, double* ref_mse, double* other_mse, void* stream);

/* RANSAC reprojection matrix over the selected candidates sel i32 [C] (indices into the P candidates above):
 * mse[a][b] = mean_j |xy_b[j] - render_{view(b)}(tri_a[j])|^2, counts[a] = #{b : mse[a][b] < threshold}.
 * replaces: src/generation/optimize_depth.py:329-350 (the candidates^2 loop).
 * sel and cand_view are followed as given: the entry point is told neither P nor n_views, so sel[] in [0, P) and cand_view[sel[]] in
 * [0, n_views) are the caller's to validate (coma_amd/triangulate.py does).  C <= 65535 (one grid row per candidate); C = 0 writes nothing. */
int coma_ransac_mse_f64(const double* views, const double* tri, const int* cand_view, const double* cand_xy, const int* sel,
                        int C, int J, double threshold, double* mse, int* counts, void* stream);

/* Sample ingestion: area-weighted vertex normals of S posed meshes with one shared topology.
 * replaces: open3d TriangleMesh.compute_vertex_normals() + normalize_vectors_np in
 *           prepare_affordance_extraction_inputs (utils/coma.py:672-686).
 * verts f64 [S,V,3]; faces i32 [F,3]; vf_offsets i32 [V+1] / vf_faces i32 [3F]: vertex -> incident faces (CSR, ascending
 * face index: the order in which open3d accumulates); eps >= 0 applies the reference's second v/(|v|+eps); normals f64 [S,V,3].
 * A vertex without faces, or whose face normals cancel, gets (0, 0, 1).  faces, vf_offsets and vf_faces are followed as given: vertex
 * indices in [0, V), face indices in [0, F) and offsets ascending within [0, 3F] are the caller's to validate.  S <= 65535. */
int coma_vertex_normals_f64(const double* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces,
                            int S, int V, int F, double eps, double* normals, void* stream);

/* Weighted sample elimination (Yuksel 2015), the method behind open3d's sample_points_poisson_disk; opt-in sampler of the
 * down-sampling writers (coma_amd/downsample.py::sample_poisson_disk).  Parity with open3d's own point set is UNPINNED (another
 * RNG draws its candidates, and the constants the host passes are quoted from memory); what is pinned is this definition:
 * d_ij = sqrt(((xi-xj)^2 + (yi-yj)^2) + (zi-zj)^2); pairs with d_ij >= r_max contribute nothing; w_ij = ((t*t)^2)^2 with
 * t = 1 - max(d_ij, r_min)/r_max; w_i = sum over j != i in ascending j; until n_keep points are alive the alive point of largest
 * w is removed (lowest index on equal w) and every alive neighbour j gets one w_j -= w_ij.  All f64, no FMA: bit-identical to
 * tests/sample_elim_ref.py.
 * points f64 [M,3] -> keep_idx i64 [n_keep], the surviving indices in ascending order.  workspace: device buffer of
 * coma_sample_eliminate_workspace_bytes(M) bytes, 8-byte aligned.  Refused (COMA_E_INVALID, keep_idx untouched): M outside
 * [1, 65536], n_keep outside [1, M], alpha != 8, r_max <= 0, r_min outside [0, r_max).  n_keep == M returns 0..M-1 without
 * running the loop.  The loop runs in ONE workgroup (no waiting between workgroups). */
size_t coma_sample_eliminate_workspace_bytes(int M);
int coma_sample_eliminate_f64(const double* points, int M, int n_keep, double r_max, double r_min, double alpha, void* workspace,
                              int64_t* keep_idx, void* stream);

/* Depth initialisation's silhouette test: an orthographic nearest-depth map per mesh and one compare-and-count pass.
 * replaces: the Blender scene build and the 2*retrieval_range + 1 instance-segmentation renders of
 *           src/generation/initialize_depth.py:134-201 (select_human), and get_rendered_human_segmap / compute_IoU of
 *           src/generation/compute_metrics.py:39-112.  The candidates differ only by a shift along the viewing axis of an
 *           orthographic camera, so they share one screen footprint: two depth maps (human, asset) answer all K of them.
 * Blender's own render is UNPINNED (bpy is not available to this project); what is pinned, bit for bit against the NumPy
 * restatement tests/raster_ref.py, is this rule set (all f64, no FMA, sums in the order written):
 *   camera space   c = diag(1,-1,-1) R^T (p - t) as in utils/blenderproc.py:183-196: d = p - t; c.x = (R00 d0 + R10 d1) + R20 d2;
 *                  c.y = -((R01 d0 + R11 d1) + R21 d2); c.z = -((R02 d0 + R12 d1) + R22 d2) is the depth, larger is farther.
 *   pixel          u = c.x s + W/2, v = c.y s + H/2 (x to the right, y down), s = max(W, H) / scale: Blender's ortho scale spans
 *                  the LARGER side, the max(cam_resolution) of initialize_depth.py:312-314.  [3rd-party, unpinned] for W != H:
 *                  utils/blenderproc.py:196 scales x by W and y by H, which agrees only for the square images the pipeline uses.
 *   snapping       U = floor(u 256 + 0.5), V = floor(v 256 + 0.5) as integers (1/256-pixel grid).  A non-finite vertex (or depth)
 *                  or |U|, |V| > 2^25 refuses the call; below that every edge function is exact in int64 and in f64.
 *   coverage       pixel (i, j) is sampled at (256 i + 128, 256 j + 128); integer edge functions
 *                  e_PQ(x, y) = (Qx - Px)(y - Py) - (Qy - Py)(x - Px); area = e_AB(C); area < 0 swaps B and C (both windings are
 *                  drawn), area == 0 is skipped; with e0 = e_BC, e1 = e_CA, e2 = e_AB a sample is covered when every e > 0, or
 *                  e == 0 on an edge P->Q with Qy < Py, or Qy == Py and Qx > Px (top-left rule: a shared edge is hit exactly once).
 *   depth          z = ((e0 zA + e1 zB) + e2 zC) / area; a NaN (only when |z| 2^53 overflows) is not drawn.
 *   resolve        key(z) = bits ^ (sign ? all ones : 2^63), an order-preserving u64; 64-bit atomic minimum per pixel, so the map
 *                  does not depend on the order of arrival; the empty key is all ones.
 * verts f64 [V,3] world space, faces i32 [F,3] (device); R f64[9] row-major camera-to-world rotation and t f64[3] camera position
 * are HOST pointers read during the call; depth_key u64 [H,W]; workspace: coma_raster_workspace_bytes(V, F) bytes of device
 * scratch, 16-byte aligned.  W, H in [1, 8192].
 * Refusals.  Arguments the host can see (null pointer, sizes, scale, camera) return COMA_E_INVALID before anything is launched.
 * The vertex and face DATA live on the device and no entry point here synchronises with the host, so those refusals are taken on
 * the device: the first kernel records them in the workspace, every later kernel then does nothing (depth_key is left untouched),
 * and coma_raster_status(workspace, stream) -- the one call that waits for the stream -- returns COMA_E_INVALID with the text.
 * !! coma_raster_depth_f64 RETURNING COMA_OK DOES NOT MEAN THE MAP WAS DRAWN.  A C caller MUST call coma_raster_status on the same
 * !! workspace and stream before it reads depth_key or hands it to coma_silhouette_iou: after a refusal depth_key still holds
 * !! whatever it held before the call (uninitialised memory for a fresh buffer), and nothing else reports that. */
size_t coma_raster_workspace_bytes(int V, int F);
int coma_raster_depth_f64(const double* verts, int V, const int32_t* faces, int F, const double* R, const double* t, double scale,
                          int W, int H, void* workspace, uint64_t* depth_key, void* stream);
int coma_raster_status(const void* workspace, void* stream);

/* Compare and count.  human_key / asset_key u64 [H,W] from coma_raster_depth_f64 (asset_key NULL = no asset), offsets f64 [K]
 * (device; the shift of candidate k along the viewing axis, added to the decoded human depth), gt u8 [H,W] (non-zero = person).
 * A pixel belongs to candidate k when the human key is not empty and (the asset key is empty or zh + offsets[k] < za).  The test
 * is strict, so the asset wins an exact tie ([unpinned] against Blender, which has no defined order for coincident surfaces).
 * visible[k] = #pixels of candidate k, inter[k] = #(candidate and gt), uni[k] = #(candidate or gt): i64 [K], overwritten; integer
 * counts, so the order of the reduction cannot matter.  masks u8 [K,H,W] (0 / 255) is written when non-NULL.  K in [1, 64].
 * The host forms IoU = inter / uni (src/generation/initialize_depth.py:175-178).  No host synchronisation. */
int coma_silhouette_iou(const uint64_t* human_key, const uint64_t* asset_key, const double* offsets, int K, const uint8_t* gt,
                        int W, int H, int64_t* visible, int64_t* inter, int64_t* uni, uint8_t* masks, void* stream);

/* Signed volume of a triangle mesh: sum over the faces of det[a b c] / 6, what trimesh's `volume` gives for a closed mesh
 * (src/generation/compute_metrics.py:97, the denominator of the intersection ratio).  All f64, no FMA:
 * det = (ax (by cz - bz cy) - ay (bx cz - bz cx)) + az (bx cy - by cx); the sum has a FIXED shape (each thread adds its faces in
 * ascending order, a tree per workgroup, the partials in block order, a tree over them) and is divided by 6 once, so two calls
 * give the same bits; against a sum in another order it is within F 2^-52 sum|det| / 6.
 * verts f64 [V,3], faces i32 [F,3], out f64 [1] (device); workspace: coma_mesh_volume_workspace_bytes(F) bytes, 8-byte aligned.
 * A face index outside [0, V) is not followed and makes the result NaN.  No host synchronisation. */
size_t coma_mesh_volume_workspace_bytes(int F);
int coma_mesh_volume_f64(const double* verts, int V, const int32_t* faces, int F, double* out, void* workspace, void* stream);

/* Intersection volume of two meshes by columns: every crossing of a grid cell's column with either surface, then one sweep.
 * replaces: the Blender boolean of src/generation/compute_metrics.py:86-99 (trimesh.boolean.intersection(engine="blender").volume),
 *           the numerator of `interscetion_ratio`.  Blender's boolean is UNPINNED; what is pinned, bit for bit against the NumPy
 *           restatement tests/volume_ref.py, is this rule set:
 *   columns, grid  columns run along world +z over an axis-aligned xy grid of square cells: origin (x0, y0), s cells per world
 *                  unit, W x H cells, W, H in [1, 8192].  In the camera convention above this is R = diag(1,-1,-1),
 *                  t = (x0, y0, 0), W/2 = H/2 = 0: u = (x - x0) s, v = (y - y0) s, depth = z.
 *   snapping, coverage, depth   the rasteriser's rules above, unchanged (the same device functions): U = floor(u 256 + 0.5),
 *                  sample at (256 i + 128, 256 j + 128), int64 edge functions, area = e_AB(C), area < 0 swaps B and C, area == 0
 *                  is skipped, top-left rule, z = ((e0 zA + e1 zB) + e2 zC) / area in f64.
 *   crossing       every covered (column, triangle) pair yields one crossing (Z, sigma): Z = floor((z s) 256 + 0.5) as int64 -- the
 *                  quantum of the xy grid; sigma = +1 when the area BEFORE the swap was > 0, -1 when it was < 0.  A non-finite z or
 *                  |Z| > 2^40 refuses the call.
 *   sweep          per column the crossings of mesh A and of mesh B are sorted by Z.  Going up, n_A -= sigma at each crossing of A,
 *                  n_B likewise.  Between two consecutive events Z_k < Z_k+1 the column is inside A iff n_A != 0, inside B iff
 *                  n_B != 0, inside both iff both.  The order among equal Z cannot matter: the interval between them is empty.
 *   result         three int64 sums of interval lengths over all columns, sums = {L_AB, L_A, L_B}, accumulated with integer
 *                  atomics: independent of the order of arrival.  The host forms volume = L / (256 s^3).  col_ab i64 [H,W]
 *                  (optional) is each column's share of L_AB.
 * Validity: the rule set measures a volume for CLOSED, consistently oriented meshes (either orientation: n != 0, not n > 0).  For an
 * open or inconsistently oriented mesh the result is still deterministic but it is not a volume.
 * capacity is the number of crossings (A plus B) the workspace has room for, in [1, 2^31 - 1]: the total depends on the data, so
 * the caller chooses it.  workspace: coma_column_crossings_workspace_bytes(...) bytes of device scratch, 16-byte aligned (0 for
 * sizes the call would refuse).  sums i64 [3] (device).
 * Refusals follow coma_raster_depth_f64: what the host can see returns COMA_E_INVALID before any launch; what lives on the device
 * (non-finite vertex, coordinate beyond 2^25 sub-cell units, face index out of range, the Z range, capacity exceeded) is recorded in
 * the workspace, the later kernels idle, sums and col_ab are left untouched, and coma_intersection_status(workspace, stream,
 * needed) -- the one call that waits for the stream -- returns COMA_E_INVALID with the text.  *needed (HOST pointer, may be NULL)
 * receives the number of crossings counted (0 when the call was refused before they were counted): after a capacity refusal it is
 * the capacity to call again with.
 * !! coma_intersection_columns RETURNING COMA_OK DOES NOT MEAN THE SUMS WERE WRITTEN.  A C caller MUST call
 * !! coma_intersection_status on the same workspace and stream before it reads sums or col_ab: after a refusal they still hold
 * !! whatever they held before the call (uninitialised memory for a fresh buffer), and nothing else reports that. */
size_t coma_column_crossings_workspace_bytes(int VA, int FA, int VB, int FB, int W, int H, int64_t capacity);
int coma_intersection_columns(const double* vertsA, int VA, const int32_t* facesA, int FA, const double* vertsB, int VB,
                              const int32_t* facesB, int FB, double x0, double y0, double s, int W, int H, int64_t capacity,
                              void* workspace, int64_t* sums, int64_t* col_ab, void* stream);
int coma_intersection_status(const void* workspace, void* stream, int64_t* needed);

/* Depth optimisation: one scalar d, the displacement of the human along the camera's front vector, moved by Adam under a multiview
 * joint term and a collision term.
 * replaces: the optimisation loop of src/generation/optimize_depth.py:689-780.  Its optimiser holds the displacement alone (:695), so
 *           the body model's output is the same in every epoch: vertices V0 + d f, joints J0 + d f.
 * COAP's collision loss (a learned occupancy network, :752-753) is available through coma_depth_optimize_coap_f64 (the section
 * "COAP" below): its ARCHITECTURE is pinned against the code the reference vendors with seeded weights; its checkpoint is a download
 * that is not available to this project and has never been executed here.  The default collision term is geometric: the intersection
 * ratio L_AB / L_A of the column rule set above, in [0, 1], as a function of d; that is what --w_collision weights with
 * --collision columns.  What is pinned, bit for bit against the NumPy restatement tests/shift_ref.py, is this rule set:
 *   frame          the host rotates both meshes into the camera-aligned frame p' = p R (f64; R the camera's rotation, so the front
 *                  vector R[:, 2] becomes +z) and lays the grid over the xy overlap of the two bounding boxes; the z extent does not
 *                  enter, because the human slides along it and its footprint never changes.
 *   crossings      columns, grid, snapping, coverage, depth and crossing (Z, sigma) are those of coma_intersection_columns, from the
 *                  same kernels; mesh A is the human.  Per column the crossings are then sorted by (mesh, Z) and kept: A's list,
 *                  then B's.  L_A and L_B are the interval lengths inside A and inside B (the sweep's, for one mesh at a time).
 *   shift          Delta = floor((d s) 256 + 0.5) as int64, |Delta| clamped to 2^42 (nothing can overlap beyond; a NaN counts as
 *                  beyond).  L_AB(Delta) is the L_AB of the sweep above after Delta is added to every Z of A.  It is an integer,
 *                  piecewise-linear function whose breakpoints lie on integers.
 *   slope          S2(Delta) = L_AB(Delta + 1) - L_AB(Delta - 1): an exact central difference, no tie rule.
 *   collision      ratio(d) = L_AB(Delta) / L_A, d ratio / dd = (S2(Delta) (256 s)) / (2 L_A) in f64; both 0 when L_A == 0.
 *   multiview      joints = J0 + d f (x = J0x + d fx, ...).  Per inlier n with the view record w of coma_dlt_score_f64:
 *                  cx = ((x mr0 + y mr3) + z mr6) - tmr0, px = cx / scale max(res) + res_x / 2, rx = px - xy[n][j][0], likewise y;
 *                  ax = ((fx mr0 + fy mr3) + fz mr6) / scale max(res), likewise ay.  sq_n = sum_j (rx rx + ry ry) and
 *                  gr_n = sum_j (rx ax + ry ay), j ascending.  multiview_joint_loss (:371-400) sums over the joints and averages over
 *                  the two coordinates (torch.mean(torch.sum(., axis=1)) on [1, J, 2]; not a mean over joints): loss_n = 0.5 sq_n,
 *                  with the analytic gradient gr_n.  Over the views: 256 partial sums (partial t adds views t, t + 256, ... in
 *                  ascending order), a tree lds[t] + lds[t + h] for h = 128 ... 1, then / N.
 *   Adam           torch's form in f64, no FMA: g = w_multiview g_mv + w_collision (d ratio / dd); m = b1 m + (1 - b1) g;
 *                  v = b2 v + ((1 - b2) g) g; p1 = p1 b1, p2 = p2 b2 (running products from 1); d = d - ((lr / (1 - p1)) m) /
 *                  (sqrt(v) / sqrt(1 - p2) + 1e-8); b1 = 0.9, b2 = 0.999.  w_refview of the reference is not in its loss (:757).
 * coma_shift_columns_prepare: arguments, capacity and refusals exactly as coma_intersection_columns; workspace:
 *   coma_shift_columns_workspace_bytes(...) bytes, 16-byte aligned; it holds the sorted lists until the next prepare.  lengths i64 [2]
 *   (device, may be NULL) = {L_A, L_B}, each mesh's list walked alone: for closed meshes these are sums[1] and sums[2] of
 *   coma_intersection_columns; an OPEN mesh is still inside after its last crossing, which the joint sweep there counts up to the other
 *   mesh's next crossing and the walk here does not, so the two may differ.  Refusals are recorded on the device, the later kernels idle (lengths untouched), and
 *   coma_shift_columns_status(workspace, stream, needed) is the one call that waits.
 * coma_shift_profile: d f64 [K] (device), K in [1, 64] -> L i64 [K,3] = L_AB at Delta - 1, Delta, Delta + 1 (device), integer atomics.
 *   Left untouched when the workspace holds a refused call.  No host synchronisation.
 * coma_depth_optimize_f64: workspace (a prepared shift workspace, or NULL: no collision term; w_collision == 0 has the same
 *   effect), views f64 [n_views,28], joints0 f64 [J,3], cand_view i32 [N], cand_xy f64 [N,J,2] (device; N == 0: no multiview term),
 *   front f64 [3] (HOST pointer, read during the call), E epochs in [1, 4096].  Per epoch one profile kernel (K = 1, d read from traj)
 *   and one single-workgroup step kernel are enqueued; no host synchronisation.  traj f64 [E+1] = d before epoch 0 ... after epoch
 *   E - 1; Ltraj i64 [E,3] the profile at traj[e] (written when the collision term is on); losses f64 [E,2] = {multiview loss,
 *   ratio} at traj[e], unweighted.  state: coma_depth_optimize_state_bytes() bytes of device scratch, 8-byte aligned, where the step
 *   kernels keep m, v, p1, p2 between launches.  A d that is not finite is recorded there and the later epochs idle;
 *   coma_depth_optimize_status(state, stream, epoch) -- which waits -- then returns COMA_E_INVALID and the epoch (HOST pointer, may be
 *   NULL) after which it happened; so it does when the workspace holds a refused call (nothing is written then).
 *   What a stopped call leaves: traj up to and including the non-finite d, losses and Ltraj up to the epoch that produced it; every
 *   later slot of traj and losses keeps what it held.  Ltraj is zeroed as a whole before epoch 0 when the collision term is on.
 *   cand_view: every entry must lie in [0, n_views).  The entries live on the device, so the step kernel tests each one before it
 *   follows it; an entry outside the range is never followed.  The epoch that meets one (always epoch 0: cand_view does not change)
 *   writes NOTHING: losses[0], traj[1] and the Adam state keep what they held, traj[0] = d0 and -- with the collision term on --
 *   Ltraj[0], the profile at d0, which is taken before the step, are the only results; the later epochs idle, and
 *   coma_depth_optimize_status returns COMA_E_INVALID with epoch 0.  coma_depth_optimize_coap_f64 does the same (Ctraj[0] written).
 *   With L_A == 0 (the human off the grid) ratio and slope are both 0 and the collision term moves nothing.
 *   The clamp of the shift: "nothing can overlap beyond" holds for closed meshes.  An OPEN mesh stays inside to the end of its
 *   column, so L_AB at +2^42 and at -2^42 may be non-zero and differ; a NaN d takes +2^42.  Still deterministic, still restated. */
size_t coma_shift_columns_workspace_bytes(int VA, int FA, int VB, int FB, int W, int H, int64_t capacity);
int coma_shift_columns_prepare(const double* vertsA, int VA, const int32_t* facesA, int FA, const double* vertsB, int VB,
                               const int32_t* facesB, int FB, double x0, double y0, double s, int W, int H, int64_t capacity,
                               void* workspace, int64_t* lengths, void* stream);
int coma_shift_columns_status(const void* workspace, void* stream, int64_t* needed);
int coma_shift_profile(const void* workspace, const double* d, int K, int64_t* L, void* stream);
size_t coma_depth_optimize_state_bytes(void);
int coma_depth_optimize_f64(const void* workspace, const double* views, int n_views, const double* joints0, const double* front,
                            const int32_t* cand_view, const double* cand_xy, int N, int J, double d0, double lr, double w_multiview,
                            double w_collision, int E, double* traj, int64_t* Ltraj, double* losses, void* state, void* stream);
int coma_depth_optimize_status(const void* state, void* stream, int* epoch);

/* COAP: the learned occupancy body model behind the reference's collision loss -- encode a posed body once, query points against it.
 * replaces: imports/coap/coap.py (Partitioner :162-594 on the host, COAPBodyModel.encode_body / query / collision_loss :639-742) and
 *           imports/coap/modules.py (ResnetPointnet, ImplicitNet) as src/generation/optimize_depth.py:104-132, 671, 752-753 uses them.
 * PINNED against the reference's own COAPBodyModel executed on the CPU in f64 with a SEEDED state dict on a seeded SMPL-X-layout model
 * (tests/golden/coap_golden.npz), through the f64 restatement tests/coap_ref.py.  Only the architecture is pinned: the trained
 * checkpoint is a download and has never been executed here.  Rule set:
 *   partition      on the host (coma_amd/coap.py partition): a vertex's part is the arg-max of its skinning weights after the merges of
 *                  MERGE_BODY_PARTS, a face's the most frequent of its three vertices; K parts, joint_mapper picks their joints.
 *   transforms     R_k: the Rodrigues chain over the first mK joints (angle = |r + 1e-8|, axis r / angle), origin j_k: the posed joint.
 *                  Local coordinates are R_k^T (p - j_k), the analytic inverse of the rigid transform, in f64 on the f32 data (the
 *                  reference inverts the 4 x 4 numerically; its R is orthogonal to about 1e-8, far below the f32 bound).
 *   boxes          min and max of the part's own vertices (tight_vert_selector) in its frame; centre = (min + max) / 2, size =
 *                  |max - min| 1.125; inside: |q - centre| < size / 2 in every coordinate, strictly.
 *   samples        an INPUT: per part n_samples entries (the first n_samples / 2 on the tight faces, the rest on the extended ones)
 *                  of three vertex ids and three barycentric weights; the point is v0 + b1 (v1 - v0) + b2 (v2 - v0) -- the first
 *                  weight is implied, so that the weights sum to one exactly and the samples move rigidly with the body.  pytorch3d's
 *                  own sampler (which the reference calls every epoch) is not reproduced: its point set is unpinned.
 *   encoder        ResnetPointnet(out 128, hidden 128) without block_2 on the local samples: fc_pos 3 -> 256; four ResnetBlockFC
 *                  (256 -> 128, fc_1(relu(fc_0(relu(x)))) plus a bias-free shortcut), after each of the first three the output beside
 *                  its maximum over the part's samples; max-pool, relu, fc_c.  The pooled half of a block's input is constant per part
 *                  and enters as a per-part bias.
 *   query          input [q (3), inside (1), one-hot (K), latent (128)]; query_encoder = ImplicitNet(d_in 132 + K, 256 x 3, out 128,
 *                  skip_in [2]): lin1 has 124 - K outputs and lin2 reads cat(x, input) / sqrt 2; decoder = ImplicitNet(d_in 131 =
 *                  [q, z], 256 x 6, out 1, skip_in [3]); Softplus(beta 100, threshold 20); occ_k = sigmoid(-x) inside; occ = max over
 *                  the parts.  Pairs (part, point) outside the part's box contribute exactly zero and are not evaluated; for the
 *                  others inside = 1, so the one-hot, inside and latent inputs of lin0 and lin2 are per-part biases.
 *   shift          with d (a device scalar) and front f the body is taken as moved by d f: the query is x - d f, everything else is
 *                  unchanged (R_k^T (p - j_k) does not see a translation of the whole body).
 *   derivative     d occ / d d = the tangent pass of the winning part along -R_k^T f: y' = W x' at every layer, y' softplus'(y) at
 *                  every activation, -s (1 - s) x' at the sigmoid; 0 where no part holds the point.  Ties between parts of equal occ
 *                  go to the larger bit pattern of the derivative (the reference: to the first part).
 *   collision      a point counts if it lies in the closed box of the posed vertices (moved by d f) and occ > filter_threshold
 *                  (optimize_depth.py:104-120); loss = sum relu(occ - 0.5), d loss / d d = sum [occ > 0.5] d occ / d d, in f64: 256
 *                  points per partial in point order, the tree of block_sum; then partial t, t + 256, ... and the tree again.
 *                  DEVIATION: where more than 10 000 points survive the reference keeps a random 10 000 (:129-130); here all count.
 * Arithmetic: transforms, boxes, sample points and local coordinates in f64 on the f32 data; the networks in f32 on
 * v_mfma_f32_32x32x2_f32, every sum in a fixed k order; maxima by integer-keyed atomics; no floating-point atomics: two calls give
 * identical bits.
 * weights: coma_coap_weights_floats(K) floats (device, 16-byte aligned), packed by coma_amd/coap.py pack_weights, in this order (a
 *   "fragment" matrix [in, out] is stored [out / 32][in / 8][64 lanes][4]: lane l of step g holds W[k = 8 g + 4 (l / 32) + e][n = 32 nb
 *   + l % 32], zero beyond the matrix; a "plain" one row-major [in][out]): encoder fc_pos (fragment 8 x 256, bias); per block: fc_0,
 *   shortcut, fc_1 (fragments; of fc_0 and shortcut only the first 128 inputs in blocks 1 - 3), their two biases, and in blocks 1 - 3
 *   the pooled halves of fc_0 and shortcut (plain); fc_c (plain, bias); for lin0 and lin2 of the query encoder: the inside column, the
 *   one-hot columns [K][256], the latent columns (plain), the bias (lin2's columns divided by sqrt 2); then the ten layers as
 *   fragments, each followed by its bias padded to whole column blocks: lin0 (q only), lin1, lin2 (rows [x, q] / sqrt 2), lin3,
 *   decoder lin0 (rows [q, z]), lin1, lin2, lin3 (rows [x, q, z] / sqrt 2), lin4, lin5; decoder lin6 [256] and its bias.
 * coma_coap_encode_f32: full_pose f32 [>= 3 mK], joints f32 [>= mK,3], vertices f32 [V,3] (device); parents i32 [mK], joint_mapper
 *   u8 [mK] (HOST, read during the call; parents[i] in [0, i), joint_mapper selects K joints); selector i32 [K,S]; sample_ids i32
 *   [K,n_samples,3], sample_bary f32 [K,n_samples,3] (device).  K in [1, 32], mK in [K, 64], n_samples in [2, 4096] (no multiple of
 *   anything), S in [1, V].  code: coma_coap_code_bytes(K) bytes, 16-byte aligned: a 16-byte header {magic, K, status, 0}, then per
 *   part 24 doubles {R row-major (9), origin (3), centre (3), size / 2 (3), min (3), max (3)}, the posed vertices' box {min, max}
 *   (6 doubles), then f32: latent [K,128], the per-part biases of lin0 and lin2 [K,256] each (every field at a multiple of 16 bytes).
 *   workspace: coma_coap_encode_workspace_bytes(K, n_samples).  An id outside [0, V) or a non-finite input is recorded in the header
 *   (the id reads vertex 0); coma_coap_status(code, stream) -- which waits -- then returns COMA_E_INVALID, and queries against such
 *   a code block return zeros.
 * coma_coap_query_f32: points f32 [T,3], T in [1, 2^22]; d f64 (device, may be NULL: 0); front f32 [3] (HOST; read with d or the
 *   derivative); occ f32 [T]; docc f32 [T] (written with derivative != 0).  workspace: coma_coap_query_workspace_bytes(K, T); its first
 *   i32 is the length of the (part, point) list of the last call.  One fused launch runs all layers over the list.
 * coma_coap_collision_f32: the epoch's term; result f64 [2] = {loss, d loss / d d}, kept i64 (may be NULL) the number of points past
 *   the filter (device); filter_threshold in [0, 1).
 * coma_depth_optimize_coap_f64: coma_depth_optimize_f64 with the term above in place of the column profile: per epoch the collision
 *   launches (d read from traj) and one step kernel; multiview term, Adam, state block, stop rule and coma_depth_optimize_status are
 *   the same.  Ctraj f64 [E,2] = {loss, d loss / d d} at traj[e] (written when w_collision != 0); losses f64 [E,2] = {multiview loss,
 *   COAP loss}, unweighted.  With w_collision == 0 nothing of COAP is read. */
size_t coma_coap_weights_floats(int K);
size_t coma_coap_code_bytes(int K);
size_t coma_coap_encode_workspace_bytes(int K, int n_samples);
size_t coma_coap_query_workspace_bytes(int K, int T);
int coma_coap_encode_f32(const float* weights, size_t weights_floats, const float* full_pose, const float* joints, const float* vertices, int V,
                         const int32_t* parents, const uint8_t* joint_mapper, int mK, int K, const int32_t* selector, int S,
                         const int32_t* sample_ids, const float* sample_bary, int n_samples, void* code, void* workspace,
                         size_t workspace_bytes, void* stream);
int coma_coap_status(const void* code, void* stream);
int coma_coap_query_f32(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T, const double* d,
                        const float* front, int derivative, float* occ, float* docc, void* workspace, size_t workspace_bytes, void* stream);
int coma_coap_collision_f32(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T, const double* d,
                            const float* front, double filter_threshold, double* result, int64_t* kept, void* workspace,
                            size_t workspace_bytes, void* stream);
int coma_depth_optimize_coap_f64(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T,
                                 double filter_threshold, void* coap_workspace, size_t coap_workspace_bytes, const double* views, int n_views,
                                 const double* joints0, const double* front, const int32_t* cand_view, const double* cand_xy, int N, int J,
                                 double d0, double lr, double w_multiview, double w_collision, int E, double* traj, double* Ctraj,
                                 double* losses, void* state, void* stream);

/* The optimisation app's ComA objective: the orientation term and the contact term of one posed mesh, unweighted, and their
 * gradients with respect to the vertices, in one pass (the app never needs a loss without its gradient).
 * replaces: src/application/optimize.py:274-289 (compute_vertex_normals :118-152, normalize_vectors_torch, the column
 *           reference_object_vertex_index of canonicalize_a_wrt_b_to_p :69-115) and the loss lines :295-296 (chamfer_distance
 *           :155-164), forward and backward, inside the 2000-iteration loop of :252-307.  SMPL-X, VPoser, the angle prior and COAP
 *           stay with the caller: its autograd continues from the two gradients returned here.
 * PINNED against the reference's own functions and loss lines, executed on the CPU in f64 (tests/golden/app_objective_golden.npz),
 * through the f64 restatement tests/app_ref.py.  Rule set:
 *   normals        N_h = sum over the faces incident to h, ascending face index, of (v1 - v0) x (v2 - v0): the three index_add calls
 *                  of :124-150 add this same vector to each corner.  Three normalisations follow in the reference's order:
 *                  n1 = N / max(|N|, 1e-6) (F.normalize(eps=1e-6)), n2 = n1 / (|n1| + eps) (:277), a = n2 / (|n2| + eps) (:73).
 *   canonicalise   for the one column b the map a -> f is linear, f = M a, M built on the host in f64 from b^ = b / (|b| + eps) and
 *                  p^, s^ likewise: with c = B p^, B the b_cross of :92-98 as written (B[0][0] = b0 is set, B[2][1] = b0 is not),
 *                  M = c c^T / (1 + b^.p^) + (b^.p^) I + p^ b^^T - b^ p^^T; when 1 + b^.p^ < eps it is the replacer
 *                  M = 2 s^ s^^T - I instead.  Then f^ = f / |f|.  |p^.s^| > 1e-8 refuses the call (the reference asserts it).
 *                  With one eps in both places, 1 + b^.p^ >= about 2 eps even for b = -p, so the replacer needs eps > about 0.62.
 *   orientation    term = (1 / V) sum_h nan_to_num(1 - (GT_h . f^_h + 1) / 2).  A vertex whose share is NaN -- its normal sum is
 *                  zero (no incident face, or only degenerate ones), or f is -- contributes 0 to the term and nothing to the
 *                  gradient.  DEVIATION: the reference gives a zero gradient for a vertex without faces and NaN gradients around a
 *                  degenerate fan (0 * inf in the backward of its square roots).
 *   contact        A = verts[selected], B = targets (the object points obj_verts[corresponding_object_indices], duplicates kept):
 *                  term = mean_i min_j |A_i - B_j| + mean_j min_i |A_i - B_j|.  The argmin is taken over f32 distances
 *                  sqrt((dx^2 + dy^2) + dz^2) of coordinate differences, the FIRST minimum wins a tie; the winning distance is then
 *                  taken again in f64.  The gradient follows the argmin; a zero distance has zero gradient (as cdist's backward).
 *                  k == 0: the term is 0, its gradient zero, nothing of it is launched (the reference raises on an empty min).
 *                  `selected` must hold DISTINCT rows (np.nonzero gives them so): two equal entries write one gradient row twice.
 *   gradients      analytic.  g_h = d term / d N_h through f / |f| and the three normalisations; back to the vertices by a GATHER over
 *                  the CSR table: per incident face G = (g_f0 + g_f1) + g_f2, d/dv1 = (v2 - v0) x G, d/dv2 = G x (v1 - v0),
 *                  d/dv0 = -(d/dv1 + d/dv2), the slot of h taken, faces ascending.  The contact term's second direction is a scan
 *                  over j ascending for the rows whose argmin is i.  No floating-point atomics anywhere; the sums of the two terms
 *                  are per-workgroup trees whose partials one workgroup adds in block order: two calls give the same bits.
 *   precision      inputs and outputs are f32; everything per vertex and every sum is evaluated in f64 (the work is latency-bound),
 *                  so the outputs are the f32 rounding of the rule set.  Only the k x k argmin search is f32.
 * verts f32 [V,3]; faces i32 [F,3]; vf_offsets i32 [V+1] / vf_faces i32 [3F] as for coma_vertex_normals_f64; orientation_gt f32 [V,3];
 * obj_normal / principle_vec / sub_principle_vec: HOST pointers, 3 floats each, read during the call; selected i32 [k]; targets
 * f32 [k,3] (both may be NULL when k == 0); terms f32 [2] = {orientation, contact}; grad_orientation, grad_contact f32 [V,3],
 * overwritten; workspace: coma_app_objective_workspace_bytes(V, F, k) bytes of device scratch, 16-byte aligned (0 for sizes the call
 * would refuse).  Refused before any launch: a null pointer, V or F <= 0, k < 0 or k > V, eps < 0, a workspace too small.  A face,
 * table or selected index outside its range (device data the call cannot see) is not followed and makes the term it feeds NaN.
 * Seven kernel launches and one memset on the caller's stream; no host synchronisation. */
size_t coma_app_objective_workspace_bytes(int V, int F, int k);
int coma_app_objective_f32(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, int V, int F,
                           const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                           const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k,
                           float* terms, float* grad_orientation, float* grad_contact, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The same objective for N bodies in one call: N posed meshes of one topology against one set of constants (several starts of one
 * fit).  Rule set: the one above, per body -- body n of the batch has the BITS of coma_app_objective_f32 on body n's vertices: terms,
 * both gradients, NaN for NaN.  The kernels are the single-body call's (which is this call with N = 1): the body is the last grid
 * dimension and every workgroup works on one body, so no sum changes its shape.  The column split of the double minimum is chosen
 * from N k (N bodies fill the device N times sooner); the merge takes (min, first argmin) in ascending split order on exact f32
 * comparisons, so its result does not depend on the split.  A body's NaN stays in that body.
 * Shared by all bodies: faces, vf_offsets, vf_faces, orientation_gt, obj_normal / principle_vec / sub_principle_vec (M), eps, selected,
 * targets.  Per body: verts f32 [N][V,3]; terms f32 [N][2]; grad_orientation, grad_contact f32 [N][V,3], overwritten; every scratch
 * array.  N in [1, 1024].  workspace: coma_app_objective_batch_workspace_bytes(V, F, k, N) bytes, 16-byte aligned (0 for sizes the call
 * would refuse; at N = 1 the single-body size).  Refused before any launch, in the single-body call's order: what it refuses, then
 * (after eps) N outside [1, 1024], then the workspace.  Seven kernel launches and one memset (of N V 3 floats) whatever N; no host
 * synchronisation.  Per-body constants (other targets or another object normal per body) are not offered. */
size_t coma_app_objective_batch_workspace_bytes(int V, int F, int k, int N);
int coma_app_objective_batch_f32(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, int V, int F,
                                 const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                                 const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k, int N,
                                 float* terms, float* grad_orientation, float* grad_contact, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* The SMPL-X body model: linear blend skinning of a V-vertex template over a J-joint tree, forward and backward (one body per
 * call; the batched calls follow this block).
 * replaces: the third-party `smplx` package behind the `body_model` hook of src/application/optimize.py (every iteration, forward
 *           and backward) and src/generation/optimize_depth.py (once per item), i.e. lbs / batch_rodrigues / batch_rigid_transform and
 *           the assembly of SMPLX.forward (use_face_contour=False, no joint mapper).
 * PINNED against that package's own lbs and SMPLX class executed on the CPU in f64 (tests/golden/smplx_golden.npz), through the f64
 * restatement tests/smplx_ref.py.  Rule set:
 *   parameters     theta f32 [NT].  n_pca > 0: theta = [3 J - 2 hand_dim axis-angle entries | n_pca left | n_pca right] and the hands'
 *                  axis-angles are coefficients x hand_components (f32 [2, n_pca, hand_dim], left then right); n_pca == 0: theta is the
 *                  3 J axis-angle entries themselves.  SMPL-X: J = 55, hand_dim = 45, the leading 75 entries are global_orient 3 |
 *                  body_pose 63 | jaw 3 | leye 3 | reye 3.  pose = assembled theta + pose_mean (f32 [3J], may be NULL = zeros).
 *   Rodrigues      per joint r: angle = |r + 1e-8| (the epsilon added to EACH component before the norm), dir = r / angle,
 *                  K = skew(dir), R = I + sin(angle) K + (1 - cos(angle)) K K.  Finite, with a finite derivative, at r = 0.
 *   shape stage    v_shaped = v_template + shapedirs . coefficients (shapedirs f32 [V,3,NB], coefficients f32 [NB] = betas followed
 *                  by expression), J_rest = J_regressor (f32 [J,V]) v_shaped.  Kept in f64 in `shape_state`; re-run only when the
 *                  coefficients change.
 *   pose stage     feature = (R_i - I) for i = 1 .. J-1 flattened, P = 9 (J - 1).  G_0 = [R_0 | J_0], G_i = G_parent(i) [R_i | J_i -
 *                  J_parent(i)] in ascending i; joints_i = G_i.t (+ transl); A_i = [G_i.R | G_i.t - G_i.R J_i].  One workgroup.
 *   skinning       v_posed = v_shaped + sum_p feature_p posedirs[p, 3v + c] (posedirs f32 [P, 3V], the model's own layout; summed in
 *                  eight ascending runs of rows whose results are added in ascending order), T = sum_j weights[v, j] A_j (weights
 *                  f32 [V,J], j ascending), vertex = T [v_posed, 1] (+ transl).
 *   backward       from g = dL/dvertices f32 [V,3]: dL/dtransl = sum_v g_v; dL/dA_j = sum_v weights[v,j] g_v (x) [v_posed, 1];
 *                  g_vposed = T.R^T g_v; dL/dfeature_p = <posedirs[p, :], g_vposed>; the chain in descending i; the derivative of
 *                  the Rodrigues formula with the 1e-8 inside the norm; the hand components transposed.  coma_smplx_backward_f32 gives
 *                  NO gradient with respect to betas, expression, or through the joints output (coma_smplx_backward_full_f32
 *                  does: `full backward` below).  Sums over vertices: per workgroup of 128 vertices in
 *                  ascending order, then over the workgroups in ascending order; the P dot products as 256 strided partial sums and
 *                  a tree lds[t] + lds[t + h], h = 128 ... 1.  No floating-point atomics: two calls give the same bits.
 *   extra joints   out_e = sum_{i<3} vertex_weight[e,i] (vertex[vertex_index[e,i]] - transl) + transl: a vertex pick is index
 *                  (i, i, i) with weights (1, 0, 0), a static landmark a face's three vertices with its barycentric weights.  The
 *                  caller lays the result behind the J posed joints: [J | vertex picks | landmarks].  No gradient of its own: the
 *                  full backward takes the table and scatters.
 *   full backward  coma_smplx_backward_full_f32: from g = dL/dvertices [V,3], gJ = dL/djoints [J + E, 3] (posed joints first, then
 *                  the extra joints as the forward lays them out) and gP = dL/dfull_pose [3J], each of which may be NULL = zeros, to
 *                  dL/dtheta, dL/dtransl and dL/dcoefficients f32 [NB] (betas followed by expression).
 *                  extra joints: the effective vertex gradient g_eff[v] = g[v] + sum of w[e,i] gJ[J + e] over the table entries with
 *                    vertex_index[e,i] = v, added in ascending (e, i) (a gather per vertex over the whole table: repeated indices --
 *                    a vertex pick, landmark faces sharing a vertex -- need no atomics; an index outside [0, V) matches nothing);
 *                    g_eff takes g's place in every rule of `backward`; dL/dtransl += (1 - ((w[e,0] + w[e,1]) + w[e,2])) gJ[J + e],
 *                    e ascending.
 *                  posed joints: joints_i = G_i.t + transl, so dG_i.t += gJ[i] before the descending chain walk and dL/dtransl +=
 *                    sum_i gJ[i], i ascending; dL/dtransl = (vertex share + posed-joint share) + extra-joint share.
 *                  full pose: full_pose = assembled theta + pose_mean, so dpose += gP after the Rodrigues derivative and before the
 *                    transposed hand components.
 *                  rest joints: from A_i.t = G_i.t - G_i.R J_i, dJ_i = -G_i.R^T dA_i.t; in the chain walk, from G_i.t = G_p.R (J_i -
 *                    J_p) + G_p.t with u = G_p.R^T dG_i.t (dG_i.t complete: every child has a larger index), dJ_i += u and dJ_p -= u;
 *                    at the root dJ_0 += dG_0.t.
 *                  shape: dL/dv_shaped[v] = g_vposed[v] (of g_eff) + sum_j J_regressor[j,v] dJ_j, j ascending; dL/dcoefficient_l =
 *                    sum_{i < 3V} shapedirs[i,l] dL/dv_shaped[i]: per workgroup of 256 rows i in ascending order, then over the
 *                    workgroups in ascending order.
 *                  With grad_joints, grad_full_pose and grad_coefficients all NULL, grad_theta and grad_transl are the bits of
 *                  coma_smplx_backward_f32.  All in f64 on the f32 data; two calls give the same bits.  The 3 launches of the
 *                  backward, plus 1 when gJ reaches extra joints or g is NULL (the effective gradient), plus 2 for the coefficients.
 *   precision     inputs and outputs are f32; every stage is evaluated in f64 (the work is bandwidth- and latency-bound), so the
 *                  outputs are the f32 rounding of the rule set.
 * All pointers are device pointers except `parents` (HOST, i32 [J], read during the call; parents[0] is ignored, parents[i] must lie
 * in [0, i) for i > 0).  shape_state / saved / workspace: coma_smplx_{shape_state,saved,workspace}_bytes(V, J) bytes, 16-byte aligned
 * (0 for sizes the calls refuse).  `saved` is written by a forward and read by ITS backward (one per forward in flight); `workspace`
 * is scratch shared by all calls on one stream.  vertices f32 [V,3], joints f32 [J,3], full_pose f32 [3J] (may be NULL), grad_theta
 * f32 [NT], grad_transl f32 [3], transl f32 [3] (may be NULL).  Refused before any launch: a null pointer, V outside [1, 2^24], J
 * outside [1, 64], NB outside [1, 1024], n_pca outside [0, 64], hand_dim not a multiple of 3 or 2 hand_dim > 3 (J - 1), a bad parent, a
 * buffer too small or misaligned.  A vertex_index outside [0, V) is not followed and gives NaN.  Forward: 3 launches, backward: 3,
 * shape: 2, extra joints: 1; caller's stream, no allocation, no host synchronisation.
 * coma_smplx_backward_full_f32 takes what the backward takes plus grad_joints f32 [J + E, 3], grad_full_pose f32 [3J], the extra-joint
 * table (vertex_index i32 [E,3], vertex_weight f32 [E,3]; read only with grad_joints and E > 0), shapedirs, J_regressor, NB and
 * grad_coefficients f32 [NB] (the last three pointers read only when grad_coefficients is given).  grad_vertices, grad_joints,
 * grad_full_pose and grad_coefficients may each be NULL: a NULL input contributes nothing, a NULL output is not computed.  Its workspace
 * is its own: coma_smplx_grad_workspace_bytes(V, J, NB) bytes (0 for V, J the calls refuse or NB outside [0, 1024]).  Refused as well:
 * E outside [0, 4096], a NULL table with grad_joints and E > 0, with grad_coefficients NB outside [1, 1024] or a NULL shapedirs or
 * J_regressor (without it NB outside [0, 1024]).  Up to 6 launches (see `full backward`).  Still not built on top of it: COAP's own
 * backward, so src/application/optimize.py --use_collision stays refused. */
size_t coma_smplx_workspace_bytes(int V, int J);
size_t coma_smplx_shape_state_bytes(int V, int J);
size_t coma_smplx_saved_bytes(int V, int J);
int coma_smplx_shape_f32(const float* v_template, const float* shapedirs, const float* coefficients, const float* J_regressor, int V, int J,
                         int NB, void* shape_state, size_t shape_state_bytes, void* stream);
int coma_smplx_forward_f32(const float* theta, const float* transl, const float* posedirs, const float* weights, const int32_t* parents,
                           const float* hand_components, const float* pose_mean, int V, int J, int hand_dim, int n_pca,
                           const void* shape_state, float* vertices, float* joints, float* full_pose, void* saved, size_t saved_bytes,
                           void* workspace, size_t workspace_bytes, void* stream);
int coma_smplx_backward_f32(const float* grad_vertices, const float* posedirs, const float* weights, const int32_t* parents,
                            const float* hand_components, int V, int J, int hand_dim, int n_pca, const void* shape_state,
                            const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t coma_smplx_grad_workspace_bytes(int V, int J, int NB);
int coma_smplx_backward_full_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose, const float* posedirs,
                                 const float* weights, const int32_t* parents, const float* hand_components, const int32_t* extra_index,
                                 const float* extra_weight, int E, const float* shapedirs, const float* J_regressor, int NB, int V, int J,
                                 int hand_dim, int n_pca, const void* shape_state, const void* saved, size_t saved_bytes,
                                 float* grad_theta, float* grad_transl, float* grad_coefficients, void* workspace, size_t workspace_bytes,
                                 void* stream);
int coma_smplx_extra_joints_f32(const float* vertices, const float* transl, const int32_t* vertex_index, const float* vertex_weight, int V,
                                int E, float* out, void* stream);

/* The SMPL-X body model for a BATCH of N bodies in one call: the package's `batch_size=N`.
 * Rule set: the one above, applied to every body.  Body n of a batched call has THE BITS of the single-body call on the same inputs:
 * its pose offset is the eight ascending runs of rows added in ascending order, its sums over vertices are per workgroup of 128 in
 * ascending order and then over the workgroups in ascending order, its P dot products are 256 strided partial sums and the tree, all in
 * f64 on the f32 data without floating-point atomics.  What the batch changes is how often the operands move:
 *   posedirs       bodies are served in chunks of C = 8.  Forward: a workgroup holds the chunk's features of its run of rows in LDS
 *                  and eight f64 sums per thread, so an element of posedirs is loaded once per chunk; backward: the workgroup of row p
 *                  forms the chunk's eight dot products from one read of the row.  ceil(N / 8) sweeps per direction.
 *   weights        a skinning workgroup stages its 128 x J tile once and walks 2 bodies over it, each body's A in LDS in turn:
 *                  ceil(N / 2) reads of the table (2.3 MB at V = 10 475, J = 55) per direction.
 *   pose stage     one workgroup per body, forward and backward.
 * Launches: forward 3 (pose, offsets, skinning), extra joints 1, backward 3 (skinning, features, chain), plus 1 when grad_joints reaches
 * extra joints or grad_vertices is NULL (the effective gradient), whatever N is.
 * Arrays: theta f32 [N, NT], transl f32 [N, 3] or NULL, vertices f32 [N, V, 3], joints f32 [N, J, 3], full_pose f32 [N, 3J] (may be
 * NULL), grad_vertices f32 [N, V, 3], grad_joints f32 [N, J + E, 3], grad_full_pose f32 [N, 3J] (each gradient may be NULL = zeros),
 * grad_theta f32 [N, NT], grad_transl f32 [N, 3]; the extra joints read vertices [N, V, 3] and write out f32 [N, E, 3] from ONE table.
 * The model pointers are those of the single-body calls; `parents` stays a HOST pointer.
 * shape_state / shape_stride: shape_stride = 0 is one shape state shared by all bodies; otherwise body n's state lies at shape_state +
 * n shape_stride (bytes), each written by coma_smplx_shape_f32, which is unchanged.
 * saved: coma_smplx_batch_saved_bytes(V, J, N) bytes, written by a forward and read by ITS backward: body n's block is the single-body
 * layout at n coma_smplx_saved_bytes(V, J).  workspace: coma_smplx_batch_workspace_bytes(V, J, N) for the forward (features [N, P] and
 * the partial offsets [N, 8, 3V] in f64: 2.0 MB per body at V = 10 475) and coma_smplx_batch_grad_workspace_bytes(V, J, N) for the
 * backward, whichever gradients are given (g_vposed and the effective gradient [N, 3V], the workgroups' shares [N, tiles, 12 J + 3], the
 * feature gradients [N, P]).  All three return 0 for sizes the calls refuse; all buffers 16-byte aligned.
 * coma_smplx_backward_batch_f32: with grad_joints and grad_full_pose NULL body n has the bits of coma_smplx_backward_f32; otherwise those
 * of coma_smplx_backward_full_f32 with grad_coefficients NULL.  DEVIATION: the gradient to the shape coefficients is not part of the
 * batched call.
 * Refused before any launch: N outside [1, 1024]; a shape_stride that is neither 0 nor a multiple of 16 of at least
 * coma_smplx_shape_state_bytes(V, J); and everything the single-body calls refuse (a null pointer, V, J, n_pca, hand_dim, a bad
 * parent, a buffer too small or misaligned, E outside [0, 4096], a NULL table with grad_joints and E > 0).  Caller's stream, no
 * allocation, no host synchronisation. */
size_t coma_smplx_batch_workspace_bytes(int V, int J, int N);
size_t coma_smplx_batch_saved_bytes(int V, int J, int N);
size_t coma_smplx_batch_grad_workspace_bytes(int V, int J, int N);
int coma_smplx_forward_batch_f32(const float* theta, const float* transl, const float* posedirs, const float* weights, const int32_t* parents,
                                 const float* hand_components, const float* pose_mean, int V, int J, int hand_dim, int n_pca, int N,
                                 const void* shape_state, size_t shape_stride, float* vertices, float* joints, float* full_pose, void* saved,
                                 size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int coma_smplx_backward_batch_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose, const float* posedirs,
                                  const float* weights, const int32_t* parents, const float* hand_components, const int32_t* extra_index,
                                  const float* extra_weight, int E, int V, int J, int hand_dim, int n_pca, int N, const void* shape_state,
                                  size_t shape_stride, const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl,
                                  void* workspace, size_t workspace_bytes, void* stream);
int coma_smplx_extra_joints_batch_f32(const float* vertices, const float* transl, const int32_t* vertex_index, const float* vertex_weight,
                                      int V, int E, int N, float* out, void* stream);

/* VPoser's pose decoder (forward and backward), its encoder (forward), and the SMPLify angle prior.
 * replaces: the `pose_decoder` and `angle_prior` hooks of src/application/optimize.py, i.e. the reference's vendored VPoser
 *           (imports/vposer/vposer_smpl.py: decode(output_type="aa") and its autograd in every iteration, encode once per fit),
 *           rotation_matrix_to_angle_axis of utils/transformations.py:144-280 and SMPLifyAnglePrior of imports/vposer/prior.py:53-85.
 * PINNED against that code executed on the CPU in f64 with seeded weights (tests/golden/vposer_golden.npz), through the f64
 * restatement tests/vposer_ref.py.  N = batch, D = latent size, H = neurons, NJ = joints.  Weights in torch's Linear layout
 * [out, in], f32.  Rule set:
 *   layers         lrelu(x) = x where x > 0, else 0.2 x.  h1 = lrelu(W1 z + b1) [H], h2 = lrelu(W2 h1 + b2) [H], o = W3 h2 + b3 [6 NJ].
 *                  Summation order of one output row: lane l of a wave64 adds W[row, i] x[i] for i = l, l + 64, ... ascending; the 64
 *                  partial sums are folded by v = v + v[lane xor h] for h = 32, 16, 8, 4, 2, 1; the bias is added last.
 *   Gram-Schmidt   per joint j the six numbers o[6j ..] are a [3,2] matrix with columns c0 = (o0, o2, o4), c1 = (o1, o3, o5):
 *                  b1 = c0 / max(|c0|, 1e-12), u = c1 - (b1 . c1) b1, b2 = u / max(|u|, 1e-12), b3 = b1 x b2; the rotation R has the
 *                  COLUMNS b1, b2, b3 (`matrices` [N,NJ,9] is R row-major).  |v| = sqrt((v0^2 + v1^2) + v2^2).
 *   quaternion     on T = R^T (T[i] = b_{i+1}; the reference transposes first).  Branch id:
 *                    T22 < 1e-6:  0 when T00 > T11, else 1;        otherwise:  2 when T00 < -T11, else 3.
 *                    0: t = 1 + T00 - T11 - T22, cand = (T12 - T21, t, T01 + T10, T20 + T02)
 *                    1: t = 1 - T00 + T11 - T22, cand = (T20 - T02, T01 + T10, t, T12 + T21)
 *                    2: t = 1 - T00 - T11 + T22, cand = (T01 - T10, T20 + T02, T12 + T21, t)
 *                    3: t = 1 + T00 + T11 + T22, cand = (t, T12 - T21, T20 - T02, T01 - T10)
 *                  (t summed left to right), q = cand / sqrt(t) * 0.5.  Only the selected candidate is evaluated: the reference
 *                  multiplies the other three by zero before its square root.
 *   axis-angle     s2 = (q1^2 + q2^2) + q3^2, s = sqrt(s2), two_theta = 2 atan2(-s, -q0) when q0 < 0, else 2 atan2(s, q0);
 *                  k = two_theta / s where s2 > 0, else 2; aa = (q1, q2, q3) k.
 *   backward       from grad_aa [N, 3 NJ]: the analytic derivative of the three steps above for the branch the forward stored, then
 *                  g_h2 = lrelu'(h2) (W3^T g_o), g_h1 = lrelu'(h1) (W2^T g_h2), grad_z = W1^T g_h1, with lrelu' = 1 where the activation
 *                  is > 0 and 0.2 elsewhere.  Summation order of one input column: wave w of 16 adds W[o, i] g[o] for o = w, w + 16,
 *                  ... ascending; the 16 partial sums are added in ascending w.  NO gradient with respect to the weights.
 *                  The map is discontinuous where the angle reaches pi, and where s2 == 0 (the exact identity) k is the constant 2.
 *                  DEVIATION: at the exact identity the reference's autograd gives NaN (torch.where over 0 / 0 in its backward);
 *                  this backward returns the finite gradient of the k = 2 branch, d aa / d (q1, q2, q3) = 2.
 *   encoder        eval-mode BatchNorm1d, y = (x - running_mean) / sqrt(running_var + 1e-5) weight + bias (bn = f32 [4, C]: weight, bias,
 *                  running_mean, running_var): e = lrelu(W2 bn2(lrelu(W1 bn1(pose) + b1)) + b2); Wml f32 [2 D, H] holds the rows of
 *                  the mu layer, then those of the logvar layer (bml likewise): mean = first D outputs, scale = softplus of the last D,
 *                  softplus(x) = x where x > 20, else log1p(exp(x)).  Forward only, no dropout (eval mode).
 *   angle prior    out[n, i] = exp(sign[i] pose[n, index[i]])^2 for i < K; backward: grad_pose f32 [N, P], zero except
 *                  grad_pose[n, index[i]] = grad_out[n, i] 2 sign[i] out[n, i] (equal indices are added in ascending i).
 *   precision      inputs and outputs are f32; all arithmetic is f64 (the work is latency- and bandwidth-bound), so the outputs are the
 *                  f32 rounding of the rule set.  No floating-point atomics: two calls give the same bits.
 * Out of scope: training and dropout, the GMM and L2 priors, aa2matrot, the tanh decoder, gradients with respect to the weights.
 * All pointers are device pointers except `index` (i32 [K]) and `sign` (f32 [K]) of the angle prior: HOST, read during the call.
 * z f32 [N, D]; aa, grad_aa f32 [N, 3 NJ]; matrices f32 [N, NJ, 9] and branch i8 [N, NJ] may be NULL; pose f32 [N, 3 NJ] (encoder) or
 * [N, P] (prior); mean, scale f32 [N, D].  saved / workspace: coma_vposer_{saved,workspace}_bytes(N, H, NJ) bytes, 16-byte aligned (0
 * for sizes the calls refuse); `saved` (h1, h2, o in f64 and the branch ids) is written by a decode and read by ITS backward (one per
 * forward in flight), `workspace` is scratch shared by all calls on one stream.  Refused before any launch: a null pointer, N outside
 * [1, 64], D outside [1, 256], H outside [1, 2048], NJ outside [1, 64], P outside [1, 4096], K outside [1, 16], an index outside [0, P),
 * a buffer too small or misaligned.  Decode: 4 launches, its backward: 4, encode: 5, the prior and its backward: 1 each; caller's
 * stream, no allocation, no host synchronisation. */
size_t coma_vposer_saved_bytes(int N, int H, int NJ);
size_t coma_vposer_workspace_bytes(int N, int H, int NJ);
int coma_vposer_decode_f32(const float* z, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                           const float* b3, int N, int D, int H, int NJ, float* aa, float* matrices, int8_t* branch, void* saved,
                           size_t saved_bytes, void* stream);
int coma_vposer_decode_backward_f32(const float* grad_aa, const float* W1, const float* W2, const float* W3, int N, int D, int H, int NJ,
                                    const void* saved, size_t saved_bytes, float* grad_z, void* workspace, size_t workspace_bytes,
                                    void* stream);
int coma_vposer_encode_f32(const float* pose, const float* bn1, const float* W1, const float* b1, const float* bn2, const float* W2,
                           const float* b2, const float* Wml, const float* bml, int N, int D, int H, int NJ, float* mean, float* scale,
                           void* workspace, size_t workspace_bytes, void* stream);
int coma_angle_prior_f32(const float* pose, int N, int P, const int32_t* index, const float* sign, int K, float* out, void* stream);
int coma_angle_prior_backward_f32(const float* pose, const float* grad_out, int N, int P, const int32_t* index, const float* sign, int K,
                                  float* grad_pose, void* stream);

/* The fitting app's whole Adam loop: E iterations of decode -> skin -> objective -> backward -> Adam enqueued by one call (N = 1).
 * replaces: the loop of src/application/optimize.py:252-307 with the parameter set of :236-250 and torch.optim.Adam, i.e. what
 *           this repository's fit() drives from Python through four autograd Functions and torch's optimiser.
 * Every stage is the existing entry point in two halves (csrc/fit_stages.h): its argument checks, made ONCE per call on buffers
 * carved from ONE workspace, and its launches, enqueued per iteration on the caller's stream; the new kernels only move numbers
 * between the stages and take the step.  PINNED against the reference's own parts (its vendored SMPLX class and
 * VPoser class, SMPLifyAnglePrior, the objective's own lines, torch.optim.Adam) run on the CPU in f64
 * (tests/golden/app_fit_golden.npz), through the f64 restatement tests/fit_ref.py.
 *   parameters     p f64 [P] = [global_orient 3 | transl 3 | left hand hs | right hand hs | embedding D], hs = n_pca when n_pca > 0,
 *                  else hand_dim; P = 6 + 2 hs + D.  Kept in `state` with Adam's m, v, the running products p1, p2, the iteration
 *                  count and the status word.  coma_app_fit_init_f64 writes p0 (f64 [P], device), m = v = 0, p1 = p2 = 1, count 0;
 *                  a second coma_app_fit_f32 on the same state continues where the first stopped.
 *   launches       per iteration, in order, no host synchronisation, no floating-point atomics:
 *                   1 fit_assemble_kernel    theta f32 = [fl32(global_orient) | body_pose, left for 3 | lead_fixed 9 | fl32(hands)]
 *                                            (the layout of coma_smplx_forward_f32), z = fl32(embedding), transl = fl32(transl)
 *                   2 coma_vposer_decode_f32 z -> aa f32 [3 NJ]
 *                   3 fit_pose_kernel        aa into theta's body_pose slot; prior_i = exp(sign_i aa[index_i])^2 and their sum,
 *                                            i ascending through the workgroup tree, f64 (not rounded to f32)
 *                   4 coma_smplx_forward_f32 theta, transl -> raw vertices f32
 *                   5 fit_scale_kernel       vs = fl32(raw fl32(scale_factor)), written to `vertices`
 *                   6 coma_app_objective_f32 vs -> terms f32 [2], g_o, g_c
 *                   7 fit_seed_kernel        g = fl32(fl32(fl32(fl32(w_o) g_o) + fl32(fl32(w_c) g_c)) fl32(scale_factor)): f32, unfused, the
 *                                            order of torch's eager ops in the Python path, whose seed it therefore equals bit for bit
 *                   8 coma_smplx_backward_f32 g -> grad_theta, grad_transl
 *                   9 fit_prior_grad_kernel  grad_aa_j = fl32(grad_theta[3 + j] + bending_prior_weight (sum over i with index_i == j,
 *                                            ascending, of 2 sign_i prior_i)) in f64
 *                  10 coma_vposer_decode_backward_f32 grad_aa -> grad_z
 *                  11 fit_step_kernel        one workgroup, below
 *   gradient       g f64 [P] in p's order: grad_theta's global_orient and hand entries and grad_transl as they are (f32 values), and
 *                  grad_z + (2 z) (body_pose_weight^2 pprior_weight) with z the f64 embedding.
 *   Adam           torch's form in f64, no FMA, per component: m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g; p1 = p1 b1,
 *                  p2 = p2 b2; p = p - ((lr / (1 - p1)) m) / (sqrt(v) / sqrt(1 - p2) + 1e-8); b1 = 0.9, b2 = 0.999.
 *   records        losses f64 [E,5] = {total, pprior, weighted angle prior, orientation term, contact term} at the parameters BEFORE
 *                  the step: pprior = ((sum z^2) body_pose_weight^2) pprior_weight (tree sum over the f64 embedding), weighted
 *                  prior = bending_prior_weight sum prior, the two terms unweighted as coma_app_objective_f32 gives them, total =
 *                  ((pprior + weighted prior) + orientation_weight t_o) + contact_weight t_c in f64.  traj f64 [E+1, P] (may be
 *                  NULL): row 0 = p before the call's first iteration, row e + 1 = p after iteration e.  grad0 f64 [P] (may be
 *                  NULL) = g of the call's first iteration.  vertices f32 [V,3] = vs of the LAST iteration's forward -- the forward
 *                  before the last step, which is what the reference saves.
 *   non-finite     the step kernel looks at every g and every updated p; if one is not finite it applies NOTHING: p, m, v and the
 *                  products stay, the count still advances, and the first such iteration is recorded in `state`.  Later iterations
 *                  run on the frozen, finite parameters, so no kernel ever reads a non-finite parameter (the records of such
 *                  iterations are written all the same: traj repeats p, losses may hold non-finite numbers).
 *                  coma_app_fit_status(state, stream, iteration) is the ONE call that waits; it returns COMA_E_INVALID and the
 *                  iteration (HOST pointer, may be NULL), counted from the last init.  It also reports a state that no init has
 *                  written, or one of another P: such a call leaves the state's parameters and every record but `vertices` as
 *                  they were (`vertices` then holds no result).
 * Descriptor: model pointers as coma_smplx_forward_f32 takes them, decoder pointers as coma_vposer_decode_f32, objective pointers as
 * coma_app_objective_f32, the prior's as coma_angle_prior_f32 (index into the 3 NJ body pose).  HOST pointers, read during the call:
 * parents, obj_normal, principle_vec, sub_principle_vec, prior_index, prior_sign; everything else lives on the device.
 * state: coma_app_fit_state_bytes(P) bytes (0 for P outside [7, 512]), 16-byte aligned.  workspace:
 * coma_app_fit_workspace_bytes(V, F, J, k, H, NJ, n_theta) bytes, 16-byte aligned (0 where one of the called entry points would
 * refuse the sizes or n_theta = 3 NJ + 12 + 2 hs is outside [3 NJ + 12, 3 NJ + 12 + 192]: hs <= 96); it holds theta, z, aa, the raw vertices, both models' saved
 * blocks and workspaces, the objective's workspace, terms, g_o, g_c, g and every gradient: no allocation inside the call.
 * Refused before any launch (COMA_E_INVALID, nothing written): a NULL descriptor, state or workspace, or required pointer; E outside
 * [1, 4096]; D outside [1, 256]; more than 96 entries per hand; EVERYTHING the five called entry points refuse of their own arguments,
 * by their own checks and in their own words under this call's name (V, F, J, k, hand_dim, n_pca, a bad parent, H, NJ, a misaligned
 * f32 buffer or shape state, eps < 0, principle vectors that are not orthogonal, ...): those checks are made once, before the loop,
 * and not again per iteration; 3 NJ + 12 != 3 J - 2 hand_dim; P != 6 + 2 hs + D; the prior's K outside [1, 16] or an index outside
 * [0, 3 NJ); a non-finite lr, weight or scale_factor; a state or workspace too small or misaligned; traj, losses, grad0 not 8-byte or
 * vertices, lead_fixed not 4-byte aligned. */
typedef struct coma_app_fit_desc {
  /* body model: coma_smplx_forward_f32 / coma_smplx_backward_f32 */
  const float* posedirs;
  const float* weights;
  const int32_t* parents;          /* HOST i32 [J] */
  const float* hand_components;    /* may be NULL when n_pca == 0 or hand_dim == 0 */
  const float* pose_mean;          /* may be NULL */
  const void* shape_state;
  const float* lead_fixed;         /* f32 [9]: jaw, left eye, right eye; zeros in the app */
  int V, J, hand_dim, n_pca;
  /* pose decoder: coma_vposer_decode_f32 / coma_vposer_decode_backward_f32 */
  const float* W1;
  const float* b1;
  const float* W2;
  const float* b2;
  const float* W3;
  const float* b3;
  int D, H, NJ;
  /* angle prior: coma_angle_prior_f32, on the body pose (P = 3 NJ) */
  const int32_t* prior_index;      /* HOST i32 [prior_K] */
  const float* prior_sign;         /* HOST f32 [prior_K] */
  int prior_K;
  /* objective: coma_app_objective_f32 */
  const int32_t* faces;
  const int32_t* vf_offsets;
  const int32_t* vf_faces;
  const float* orientation_gt;
  const float* obj_normal;         /* HOST f32 [3] */
  const float* principle_vec;      /* HOST f32 [3] */
  const float* sub_principle_vec;  /* HOST f32 [3] */
  const int32_t* selected;         /* may be NULL when k == 0 */
  const float* targets;            /* may be NULL when k == 0 */
  int F, k;
  double eps;
  /* the fit */
  int P, E;
  double lr, body_pose_weight, bending_prior_weight, pprior_weight, orientation_weight, contact_weight, scale_factor;
  double* traj;                    /* f64 [E+1, P] or NULL */
  double* losses;                  /* f64 [E, 5] */
  double* grad0;                   /* f64 [P] or NULL */
  float* vertices;                 /* f32 [V, 3] */
} coma_app_fit_desc;
size_t coma_app_fit_state_bytes(int P);
size_t coma_app_fit_workspace_bytes(int V, int F, int J, int k, int H, int NJ, int n_theta);
int coma_app_fit_init_f64(const double* p0, int P, void* state, size_t state_bytes, void* stream);
int coma_app_fit_f32(const coma_app_fit_desc* d, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);
int coma_app_fit_status(const void* state, void* stream, int* iteration);

#ifdef __cplusplus
}
#endif
#endif /* COMA_HIP_H */
