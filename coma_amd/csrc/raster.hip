// Orthographic nearest-depth rasteriser and the silhouette compare-and-count pass of depth initialisation (gfx950).
// The rule set is stated in include/coma_hip.h and restated in NumPy by tests/raster_ref.py; every step is either exact integer
// arithmetic or one correctly rounded f64 operation in a fixed order (no FMA: -ffp-contract=off), so the two agree key for key.
//
// coma_raster_depth_f64, five launches on the caller's stream, no host synchronisation:
//   reset  -> zeroes the header of the workspace (status word, length of the work list)
//   setup  -> one thread per vertex: camera space, pixel, snap to the 1/256 grid; refusals (non-finite, beyond 2^25, face index out
//             of range) are OR-ed into the status word.  Every later kernel returns at once when the status word is set, so a
//             refused call leaves depth_key untouched; coma_raster_status() reports the word to the host.
//   fill   -> depth_key = empty (all ones).  A kernel, not a memset node: a captured memset node hung graph replays.
//   bin    -> one LANE per triangle.  A triangle whose clipped bounding box holds <= kSmallMax pixel centres is drawn by its lane
//             (SMPL-X at 512^2: ~16 centres per box); a larger one is appended to the device-side work list with its box.
//   tile   -> one workgroup per 16 x 16 screen tile (x gridDim.y slices of the list), one pixel per thread: 256 list entries at a
//             time are tested against the tile by the 256 threads, the thread that finds a hit sets the triangle up ONCE and
//             stores it compacted in LDS, and every thread evaluates each stored triangle for its own pixel.  The running minimum
//             stays in a register: ONE atomic per pixel per workgroup, however many large triangles cover it.  A handful of screen-filling triangles therefore cost ~tiles x triangles pixel tests,
//             not one lane looping over the whole screen.
// The resolve is a 64-bit unsigned atomic minimum on an order-preserving key, so the map does not depend on arrival order.
//
// coma_silhouette_iou: zero the 3K counters, then one pass over the pixels; a wave handles 64 consecutive pixels, each candidate's
// predicate is reduced by ballot + popcount, accumulated per workgroup in LDS and flushed with 3K integer atomics per workgroup.
#include "raster_common.h"

namespace coma {

constexpr int kIouMaxK = 64;
constexpr unsigned long long kEmptyKey = ~0ull;

__device__ __forceinline__ unsigned long long depth_key(double z) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(z);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_depth(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// key of the triangle at pixel (x, y), or the empty key when the centre is not covered
__device__ __forceinline__ unsigned long long raster_sample(const RasterTri& t, int x, int y) {
  double z;
  if (!raster_cover_depth(t, x, y, z)) return kEmptyKey;
  if (z != z) return kEmptyKey;   // only when |depth| * 2^53 overflows: such a sample is not drawn
  return depth_key(z);
}

__global__ void raster_reset_kernel(int* __restrict__ hdr) {
  if (threadIdx.x < kHeaderBytes / sizeof(int)) hdr[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void raster_setup_kernel(const double* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                           RasterCam cam, SnapVert* __restrict__ sv, int* __restrict__ hdr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int bad = 0;
  if (i < V) {
    const double p0 = verts[3 * (int64_t)i + 0], p1 = verts[3 * (int64_t)i + 1], p2 = verts[3 * (int64_t)i + 2];
    const double d0 = p0 - cam.t[0], d1 = p1 - cam.t[1], d2 = p2 - cam.t[2];
    // diag(1,-1,-1) R^T d: row k of R^T is column k of R
    const double cx = (cam.r[0] * d0 + cam.r[3] * d1) + cam.r[6] * d2;
    const double cy = -((cam.r[1] * d0 + cam.r[4] * d1) + cam.r[7] * d2);
    const double cz = -((cam.r[2] * d0 + cam.r[5] * d1) + cam.r[8] * d2);
    const double su = floor((cx * cam.s + cam.hw) * 256.0 + 0.5), sw = floor((cy * cam.s + cam.hh) * 256.0 + 0.5);
    if (!(__builtin_isfinite(p0) && __builtin_isfinite(p1) && __builtin_isfinite(p2) && __builtin_isfinite(cz))) bad |= kBadNonFinite;
    else if (!(fabs(su) <= kSnapLimit && fabs(sw) <= kSnapLimit)) bad |= kBadRange;
    else sv[i] = SnapVert{(int)su, (int)sw, cz};
  }
  if (i < F) {
    const int a = faces[3 * (int64_t)i + 0], b = faces[3 * (int64_t)i + 1], c = faces[3 * (int64_t)i + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) bad |= kBadFace;
  }
  if (bad) atomicOr(&hdr[0], bad);
}

__global__ __launch_bounds__(256) void raster_fill_kernel(unsigned long long* __restrict__ key, int64_t n, const int* __restrict__ hdr) {
  if (hdr[0]) return;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) key[i] = kEmptyKey;
}

__global__ __launch_bounds__(256) void raster_bin_kernel(const SnapVert* __restrict__ sv, const int* __restrict__ faces, int F, int W, int H,
                                                         unsigned long long* __restrict__ key, int4* __restrict__ big, int* __restrict__ hdr) {
  if (hdr[0]) return;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  RasterTri t;
  if (!raster_tri_load(sv, faces, f, W, H, t)) return;
  if ((t.x1 - t.x0 + 1) * (int64_t)(t.y1 - t.y0 + 1) > kSmallMax) {
    const int slot = atomicAdd(&hdr[1], 1);   // < F: a face is appended at most once
    big[slot] = make_int4(f, t.x0 | (t.y0 << 16), t.x1 | (t.y1 << 16), 0);
    return;
  }
  for (int y = t.y0; y <= t.y1; ++y)
    for (int x = t.x0; x <= t.x1; ++x) {
      const unsigned long long k = raster_sample(t, x, y);
      if (k != kEmptyKey) atomicMin(&key[(int64_t)y * W + x], k);
    }
}

__global__ __launch_bounds__(256) void raster_tile_kernel(const SnapVert* __restrict__ sv, const int* __restrict__ faces, int W, int H,
                                                          int tiles_x, unsigned long long* __restrict__ key, const int4* __restrict__ big,
                                                          const int* __restrict__ hdr) {
  __shared__ RasterTri hits[256];   // the set-up triangles of this step's hits: prepared once, by the thread that found the hit
  __shared__ int n_hits;
  if (hdr[0]) return;
  const int n = hdr[1];
  const int tid = threadIdx.x;
  const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
  const int x = tx0 + (tid & (kTile - 1)), y = ty0 + (tid >> 4);
  unsigned long long best = kEmptyKey;
  for (int base = blockIdx.y * 256; base < n; base += gridDim.y * 256) {   // n is uniform: so is the trip count
    if (tid == 0) n_hits = 0;
    __syncthreads();
    if (base + tid < n) {
      const int4 e = big[base + tid];
      const int bx0 = e.y & 0xffff, by0 = e.y >> 16, bx1 = e.z & 0xffff, by1 = e.z >> 16;
      if (bx0 < tx0 + kTile && bx1 >= tx0 && by0 < ty0 + kTile && by1 >= ty0) {
        RasterTri t;
        raster_tri_load(sv, faces, e.x, W, H, t);   // true for every listed face
        hits[atomicAdd(&n_hits, 1)] = t;
      }
    }
    __syncthreads();
    const int nh = n_hits;
    for (int h = 0; h < nh; ++h) {
      const RasterTri t = hits[h];   // the same address for every lane: an LDS broadcast
      if (x >= t.x0 && x <= t.x1 && y >= t.y0 && y <= t.y1) {
        const unsigned long long k = raster_sample(t, x, y);
        best = k < best ? k : best;
      }
    }
    __syncthreads();
  }
  if (best != kEmptyKey) atomicMin(&key[(int64_t)y * W + x], best);   // inside a clipped box, so inside the screen
}

__global__ void iou_zero_kernel(unsigned long long* __restrict__ a, unsigned long long* __restrict__ b, unsigned long long* __restrict__ c,
                                int K) {
  if ((int)threadIdx.x < K) a[threadIdx.x] = 0, b[threadIdx.x] = 0, c[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void iou_count_kernel(const unsigned long long* __restrict__ hk, const unsigned long long* __restrict__ ak,
                                                        const double* __restrict__ offsets, int K, const uint8_t* __restrict__ gt,
                                                        int64_t N, unsigned long long* __restrict__ visible,
                                                        unsigned long long* __restrict__ inter, unsigned long long* __restrict__ uni,
                                                        uint8_t* __restrict__ masks) {
  __shared__ int s_vis[kIouMaxK], s_int[kIouMaxK];
  __shared__ double s_off[kIouMaxK];
  __shared__ int s_gt;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  if (tid < K) s_vis[tid] = 0, s_int[tid] = 0, s_off[tid] = offsets[tid];
  if (tid == 0) s_gt = 0;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * 256 + (tid - lane); base < N; base += (int64_t)gridDim.x * 256) {   // uniform per wave
    const int64_t pix = base + lane;
    const bool valid = pix < N;
    const unsigned long long h = valid ? hk[pix] : kEmptyKey;
    const unsigned long long a = (valid && ak) ? ak[pix] : kEmptyKey;
    const bool g = valid && gt[pix] != 0;
    const bool human = h != kEmptyKey, bare = a == kEmptyKey;
    const double zh = key_depth(h), za = key_depth(a);
    const int ng = __popcll(__ballot(g));
    if (lane == 0 && ng) atomicAdd(&s_gt, ng);
    const bool any_human = __ballot(human) != 0;
    if (!any_human && !masks) continue;
    for (int k = 0; k < K; ++k) {
      const bool v = human && (bare || zh + s_off[k] < za);   // strict: the asset wins an exact tie
      if (any_human) {
        const int nv = __popcll(__ballot(v)), ni = __popcll(__ballot(v && g));
        if (lane == 0 && nv) atomicAdd(&s_vis[k], nv), atomicAdd(&s_int[k], ni);
      }
      if (masks && valid) masks[(int64_t)k * N + pix] = v ? 255 : 0;
    }
  }
  __syncthreads();
  if (tid < K) {
    const int nv = s_vis[tid], ni = s_int[tid];
    if (nv) atomicAdd(&visible[tid], (unsigned long long)nv);
    if (ni) atomicAdd(&inter[tid], (unsigned long long)ni);
    if (s_gt + nv - ni) atomicAdd(&uni[tid], (unsigned long long)(s_gt + nv - ni));   // |G or V| = |G| + |V| - |G and V|
  }
}

int raster_reset_launch(int* hdr, hipStream_t st) {
  hipLaunchKernelGGL(raster_reset_kernel, dim3(1), dim3(64), 0, st, hdr);
  return check_launch("raster_reset_kernel");
}

int raster_setup_launch(const double* verts, int V, const int* faces, int F, const RasterCam& cam, SnapVert* sv, int* hdr, hipStream_t st) {
  hipLaunchKernelGGL(raster_setup_kernel, dim3((unsigned)(((V > F ? V : F) + 255) / 256)), dim3(256), 0, st, verts, V, faces, F, cam, sv, hdr);
  return check_launch("raster_setup_kernel");
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_raster_workspace_bytes(int V, int F) {
  if (V < 1 || F < 1) return 0;
  return kHeaderBytes + (size_t)V * sizeof(SnapVert) + (size_t)F * sizeof(int4);
}

extern "C" int coma_raster_depth_f64(const double* verts, int V, const int32_t* faces, int F, const double* R, const double* t,
                                     double scale, int W, int H, void* workspace, uint64_t* depth_key, void* stream) {
  if (!verts || !faces || !R || !t || !workspace || !depth_key) return fail(COMA_E_INVALID, "coma_raster_depth_f64: null pointer");
  if (V < 1 || V > kRasterMaxPrims || F < 1 || F > kRasterMaxPrims)
    return fail(COMA_E_INVALID, "coma_raster_depth_f64: V=%d, F=%d outside [1, %d]", V, F, kRasterMaxPrims);
  if (W < 1 || W > kRasterMaxDim || H < 1 || H > kRasterMaxDim)
    return fail(COMA_E_INVALID, "coma_raster_depth_f64: W=%d, H=%d outside [1, %d]", W, H, kRasterMaxDim);
  if (!(scale > 0.0) || !(scale <= 1.7e308)) return fail(COMA_E_INVALID, "coma_raster_depth_f64: scale=%g must be positive and finite", scale);
  for (int k = 0; k < 12; ++k)
    if (!__builtin_isfinite(k < 9 ? R[k] : t[k - 9])) return fail(COMA_E_INVALID, "coma_raster_depth_f64: non-finite camera");
  if ((uintptr_t)workspace % 16) return fail(COMA_E_INVALID, "coma_raster_depth_f64: workspace must be 16-byte aligned");
  RasterCam cam;
  for (int k = 0; k < 9; ++k) cam.r[k] = R[k];
  for (int k = 0; k < 3; ++k) cam.t[k] = t[k];
  cam.s = (double)(W > H ? W : H) / scale, cam.hw = (double)W * 0.5, cam.hh = (double)H * 0.5;
  int* hdr = (int*)workspace;
  SnapVert* sv = (SnapVert*)((char*)workspace + kHeaderBytes);
  int4* big = (int4*)(sv + V);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)W * H;
  if (int rc = raster_reset_launch(hdr, st)) return rc;
  if (int rc = raster_setup_launch(verts, V, faces, F, cam, sv, hdr, st)) return rc;
  const unsigned fill_blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(raster_fill_kernel, dim3(fill_blocks), dim3(256), 0, st, (unsigned long long*)depth_key, n, hdr);
  if (int rc = check_launch("raster_fill_kernel")) return rc;
  hipLaunchKernelGGL(raster_bin_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, sv, faces, F, W, H,
                     (unsigned long long*)depth_key, big, hdr);
  if (int rc = check_launch("raster_bin_kernel")) return rc;
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const int tiles = tiles_x * tiles_y;
  const int slices = tiles >= 2048 ? 1 : (2048 / tiles > 32 ? 32 : 2048 / tiles);   // the list is short when the triangles are large
  hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, st, sv, faces, W, H, tiles_x,
                     (unsigned long long*)depth_key, big, hdr);
  return check_launch("raster_tile_kernel");
}

extern "C" int coma_raster_status(const void* workspace, void* stream) {
  if (!workspace) return fail(COMA_E_INVALID, "coma_raster_status: null pointer");
  int word = 0;
  if (int rc = read_back(&word, workspace, sizeof(int), stream, "coma_raster_status")) return rc;
  if (word & kBadNonFinite) return fail(COMA_E_INVALID, "coma_raster_depth_f64: non-finite vertex (depth map untouched)");
  if (word & kBadRange)
    return fail(COMA_E_INVALID, "coma_raster_depth_f64: a snapped coordinate exceeds +-2^25 (1/256-pixel units; depth map untouched)");
  if (word & kBadFace) return fail(COMA_E_INVALID, "coma_raster_depth_f64: face index outside [0, V) (depth map untouched)");
  return COMA_OK;
}

extern "C" int coma_silhouette_iou(const uint64_t* human_key, const uint64_t* asset_key, const double* offsets, int K,
                                   const uint8_t* gt, int W, int H, int64_t* visible, int64_t* inter, int64_t* uni, uint8_t* masks,
                                   void* stream) {
  if (!human_key || !offsets || !gt || !visible || !inter || !uni) return fail(COMA_E_INVALID, "coma_silhouette_iou: null pointer");
  if (K < 1 || K > kIouMaxK) return fail(COMA_E_INVALID, "coma_silhouette_iou: K=%d outside [1, %d]", K, kIouMaxK);
  if (W < 1 || W > kRasterMaxDim || H < 1 || H > kRasterMaxDim)
    return fail(COMA_E_INVALID, "coma_silhouette_iou: W=%d, H=%d outside [1, %d]", W, H, kRasterMaxDim);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)W * H;
  hipLaunchKernelGGL(iou_zero_kernel, dim3(1), dim3(kIouMaxK), 0, st, (unsigned long long*)visible, (unsigned long long*)inter,
                     (unsigned long long*)uni, K);
  if (int rc = check_launch("iou_zero_kernel")) return rc;
  const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(iou_count_kernel, dim3(blocks), dim3(256), 0, st, (const unsigned long long*)human_key,
                     (const unsigned long long*)asset_key, offsets, K, gt, n, (unsigned long long*)visible, (unsigned long long*)inter,
                     (unsigned long long*)uni, masks);
  return check_launch("iou_count_kernel");
}
