// Signed mesh volume and the column form of the intersection volume of two closed meshes (gfx950).
// The rule set is stated in include/coma_hip.h and restated in NumPy by tests/volume_ref.py.  Coverage and depth are the rasteriser's
// own device functions (raster_common.h); everything after the depth is integer arithmetic, so the three sums and the per-column
// map are bit-exact against the restatement whatever the order of arrival.
//
// coma_intersection_columns, on the caller's stream, no host synchronisation:
//   reset    -> zeroes the 64-byte header: status word, lengths of the two work lists, the number of crossings, the three sums
//   setup x2 -> the rasteriser's setup kernel with the camera R = diag(1,-1,-1), t = (x0, y0, 0), W/2 = H/2 = 0: u = (x - x0) s,
//               v = (y - y0) s, depth = z.  Refusals are OR-ed into the status word; every later kernel idles when it is set.
//   zero     -> per-column counts = 0 (a kernel, not a memset node: DESIGN 4)
//   count x2 -> per mesh: one LANE per triangle; a small box is walked by its lane (one atomic add per covered column), a large one
//               is appended to the mesh's work list, which the tile kernel drains per 16 x 16 tile (one atomic add per column per
//               workgroup).  A non-finite depth or |Z| > 2^40 is noted here and refused by the scan.
//   scan     -> exclusive prefix sum of the counts in place (1024 columns per workgroup: sums, one workgroup over the sums, offsets);
//               the total is kept in the header and compared with the caller's capacity
//   fill x2  -> the count pass again; each crossing takes the next slot of its column (atomic cursor = the offset array, which
//               ends up holding each column's END) and stores (Z << 2 | mesh << 1 | sigma > 0) as one int64
//   sweep    -> one lane per column: sort the column's entries (in LDS up to kSortMax of them, in place in the workspace beyond),
//               walk them upwards keeping n_A and n_B, add up the interval lengths; wave reduction, three integer atomics per wave
//   finish   -> sums = the header's three accumulators, unless the call was refused
//
// Everything up to the fill is columns_crossings_launch (declared in columns_common.h), which depth_opt.hip calls as well.
//
// coma_mesh_volume_f64: per-face determinants summed in a fixed shape (grid-stride per thread, LDS tree per workgroup, partials in
// block order, one workgroup over the partials), so two calls give the same bits.
#include "columns_common.h"

namespace coma {

constexpr int kVolumeBlocks = 256;

// Z of a covered sample; false (and the status word set) when the rule set refuses it
__device__ __forceinline__ bool crossing_z(double z, double s, long long& Z, int* __restrict__ hdr) {
  const double q = floor((z * s) * 256.0 + 0.5);
  if (!(fabs(q) <= (double)kZLimit)) {   // NaN and infinities fail the comparison too
    atomicOr(&hdr[3], 1);
    return false;
  }
  Z = (long long)q;
  return true;
}

__global__ __launch_bounds__(256) void columns_zero_kernel(unsigned* __restrict__ cnt, int64_t n, const int* __restrict__ hdr) {
  if (hdr[0]) return;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) cnt[i] = 0;
}

// kFill = false: count the crossings of every column, list the large triangles (entries and capacity are not used).
// kFill = true: store them.  The scan has already refused a total above capacity and the fill kernels idle after a refusal, so
// `slot < capacity` always holds there; the test stays as a safeguard only, because a store past the workspace is the one fault
// of this file that the host could not contain.
template <bool kFill>
__global__ __launch_bounds__(256) void columns_bin_kernel(const SnapVert* __restrict__ sv, const int* __restrict__ faces, int F, int W, int H,
                                                          double s, int mesh, unsigned* __restrict__ cnt, long long* __restrict__ entries,
                                                          long long capacity, int4* __restrict__ big, int* __restrict__ hdr) {
  if (hdr[0]) return;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  RasterTri t;
  if (!raster_tri_load(sv, faces, f, W, H, t)) return;
  if ((t.x1 - t.x0 + 1) * (int64_t)(t.y1 - t.y0 + 1) > kSmallMax) {
    if (!kFill) {
      const int slot = atomicAdd(&hdr[1 + mesh], 1);   // < F: a face is appended at most once
      big[slot] = make_int4(f, t.x0 | (t.y0 << 16), t.x1 | (t.y1 << 16), 0);
    }
    return;
  }
  for (int y = t.y0; y <= t.y1; ++y)
    for (int x = t.x0; x <= t.x1; ++x) {
      double z;
      long long Z;
      if (!raster_cover_depth(t, x, y, z)) continue;
      if (!crossing_z(z, s, Z, hdr)) continue;
      const unsigned slot = atomicAdd(&cnt[(int64_t)y * W + x], 1u);
      if (kFill && (long long)slot < capacity) entries[slot] = pack_crossing(Z, mesh, t.flipped);
    }
}

template <bool kFill>
__global__ __launch_bounds__(256) void columns_tile_kernel(const SnapVert* __restrict__ sv, const int* __restrict__ faces, int W, int H,
                                                           int tiles_x, double s, int mesh, unsigned* __restrict__ cnt,
                                                           long long* __restrict__ entries, long long capacity,
                                                           const int4* __restrict__ big, int* __restrict__ hdr) {
  __shared__ RasterTri hits[256];   // the set-up triangles of this step's hits: prepared once, by the thread that found the hit
  __shared__ int n_hits;
  if (hdr[0]) return;
  const int n = hdr[1 + mesh];
  const int tid = threadIdx.x;
  const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
  const int x = tx0 + (tid & (kTile - 1)), y = ty0 + (tid >> 4);
  unsigned mine = 0;
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
      if (x >= t.x0 && x <= t.x1 && y >= t.y0 && y <= t.y1) {   // inside a clipped box, so inside the grid
        double z;
        long long Z;
        if (!raster_cover_depth(t, x, y, z)) continue;
        if (!crossing_z(z, s, Z, hdr)) continue;
        if (kFill) {
          const unsigned slot = atomicAdd(&cnt[(int64_t)y * W + x], 1u);
          if ((long long)slot < capacity) entries[slot] = pack_crossing(Z, mesh, t.flipped);
        } else {
          ++mine;
        }
      }
    }
    __syncthreads();
  }
  if (!kFill && mine) atomicAdd(&cnt[(int64_t)y * W + x], mine);
}

// sum of v over the 256 threads (every thread gets it) and the exclusive prefix of this thread
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long* __restrict__ lds, unsigned long long& total) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned long long add = tid >= d ? lds[tid - d] : 0;
    __syncthreads();
    lds[tid] += add;
    __syncthreads();
  }
  const unsigned long long incl = lds[tid];
  total = lds[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void scan_sums_kernel(const unsigned* __restrict__ cnt, int64_t n, unsigned long long* __restrict__ block_sums,
                                                        const int* __restrict__ hdr) {
  __shared__ unsigned long long lds[256];
  if (hdr[0]) return;
  const int64_t base = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  unsigned long long v = 0;
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < n) v += cnt[base + k];
  unsigned long long total;
  block_scan(v, lds, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums -> their exclusive prefix; the grand total goes to the header and is held against the capacity
__global__ __launch_bounds__(256) void scan_top_kernel(unsigned long long* __restrict__ block_sums, int nb, long long capacity, int* __restrict__ hdr) {
  __shared__ unsigned long long lds[256];
  if (hdr[0]) return;
  if (hdr[3]) {   // uniform: the count kernels have finished
    if (threadIdx.x == 0) atomicOr(&hdr[0], kBadDepth);
    return;
  }
  const int chunk = (nb + 255) / 256;
  const int lo = threadIdx.x * chunk, hi = min(nb, lo + chunk);
  unsigned long long v = 0;
  for (int i = lo; i < hi; ++i) v += block_sums[i];
  unsigned long long total;
  unsigned long long run = block_scan(v, lds, total);
  for (int i = lo; i < hi; ++i) {
    const unsigned long long c = block_sums[i];
    block_sums[i] = run;
    run += c;
  }
  if (threadIdx.x == 0) {
    ((unsigned long long*)hdr)[kHdrNeeded] = total;
    if (total > (unsigned long long)capacity) atomicOr(&hdr[0], kBadCapacity);
  }
}

__global__ __launch_bounds__(256) void scan_offsets_kernel(unsigned* __restrict__ cnt, int64_t n, const unsigned long long* __restrict__ block_sums,
                                                           const int* __restrict__ hdr) {
  __shared__ unsigned long long lds[256];
  if (hdr[0]) return;
  const int64_t base = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  unsigned c[kScanItems];
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    c[k] = base + k < n ? cnt[base + k] : 0;
    v += c[k];
  }
  unsigned long long total;
  unsigned long long run = block_sums[blockIdx.x] + block_scan(v, lds, total);   // <= capacity < 2^31 from here on
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < n) cnt[base + k] = (unsigned)run;
    run += c[k];
  }
}

// insertion sort of p[0], p[stride], ..., then the walk upwards
__device__ __forceinline__ void sort_and_sweep(long long* p, int stride, int n, long long& lab, long long& la, long long& lb) {
  for (int i = 1; i < n; ++i) {
    const long long e = p[(int64_t)i * stride];
    int j = i - 1;
    while (j >= 0 && p[(int64_t)j * stride] > e) {
      p[(int64_t)(j + 1) * stride] = p[(int64_t)j * stride];
      --j;
    }
    p[(int64_t)(j + 1) * stride] = e;
  }
  int na = 0, nb = 0;
  long long prev = 0;
  for (int i = 0; i < n; ++i) {
    const long long e = p[(int64_t)i * stride];
    const long long Z = e >> 2;   // arithmetic: a floor
    if (i > 0) {
      const long long len = Z - prev;
      if (na != 0) la += len;
      if (nb != 0) lb += len;
      if (na != 0 && nb != 0) lab += len;
    }
    const int sigma = (e & 1) ? 1 : -1;
    if (e & 2) nb -= sigma;
    else na -= sigma;
    prev = Z;
  }
}

__global__ __launch_bounds__(256) void columns_sweep_kernel(const unsigned* __restrict__ ends, long long* __restrict__ entries, int64_t n,
                                                            long long* __restrict__ col_ab, int* __restrict__ hdr) {
  __shared__ long long lds[kSortMax * 256];   // entry k of lane t at [k * 256 + t]: consecutive lanes, consecutive banks
  if (hdr[0]) return;
  const int tid = threadIdx.x;
  const int64_t col = (int64_t)blockIdx.x * 256 + tid;
  long long lab = 0, la = 0, lb = 0;
  if (col < n) {
    const unsigned lo = col ? ends[col - 1] : 0u, hi = ends[col];
    const int m = (int)(hi - lo);
    if (m > 0 && m <= kSortMax) {
      for (int k = 0; k < m; ++k) lds[k * 256 + tid] = entries[lo + k];
      sort_and_sweep(&lds[tid], 256, m, lab, la, lb);
    } else if (m > kSortMax) {
      sort_and_sweep(entries + lo, 1, m, lab, la, lb);   // a long column: slow, in place, correct
    }
    if (col_ab) col_ab[col] = lab;
  }
  lab = wave_sum(lab), la = wave_sum(la), lb = wave_sum(lb);
  if ((tid & (kWave - 1)) == 0) {
    unsigned long long* acc = (unsigned long long*)hdr + kHdrSums;
    if (lab) atomicAdd(&acc[0], (unsigned long long)lab);
    if (la) atomicAdd(&acc[1], (unsigned long long)la);
    if (lb) atomicAdd(&acc[2], (unsigned long long)lb);
  }
}

__global__ void columns_finish_kernel(const int* __restrict__ hdr, long long* __restrict__ sums) {
  if (hdr[0]) return;
  if (threadIdx.x < 3) sums[threadIdx.x] = ((const long long*)hdr)[kHdrSums + threadIdx.x];
}

// ---- signed volume ----
__global__ __launch_bounds__(256) void volume_partial_kernel(const double* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                             double* __restrict__ partial) {
  __shared__ double lds[256];
  double acc = 0.0;
  for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
    const int ia = faces[3 * (int64_t)f + 0], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {
      acc = __builtin_nan("");   // nothing is read through a bad index; the result says so
      continue;
    }
    const D3 a = load3(verts, ia), b = load3(verts, ib), c = load3(verts, ic);
    // the cofactor expansion as written, not dot(a, cross(b, c)): the middle term is subtracted
    const double det = (a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x)) + a.z * (b.x * c.y - b.y * c.x);
    acc = acc + det;
  }
  const double s = block_sum<256>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void volume_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double lds[256];
  const double s = block_sum<256>((int)threadIdx.x < nb ? partial[threadIdx.x] : 0.0, lds);
  if (threadIdx.x == 0) out[0] = s / 6.0;
}

static int volume_blocks(int F) { return (F + 255) / 256 < kVolumeBlocks ? (F + 255) / 256 : kVolumeBlocks; }

int columns_crossings_launch(const double* const verts[2], const int V[2], const int* const faces[2], const int F[2], double x0, double y0,
                             double s, int W, int H, long long capacity, char* ws, const ColumnsLayout& l, hipStream_t st) {
  int* hdr = (int*)ws;
  SnapVert* sv[2] = {(SnapVert*)(ws + l.sv_a), (SnapVert*)(ws + l.sv_b)};
  int4* big[2] = {(int4*)(ws + l.big_a), (int4*)(ws + l.big_b)};
  unsigned* cnt = (unsigned*)(ws + l.cnt);
  unsigned long long* block_sums = (unsigned long long*)(ws + l.block_sums);
  long long* entries = (long long*)(ws + l.entries);
  RasterCam cam = {};
  cam.r[0] = 1.0, cam.r[4] = -1.0, cam.r[8] = -1.0;   // u = x - x0, v = y - y0, depth = z
  cam.t[0] = x0, cam.t[1] = y0, cam.t[2] = 0.0;
  cam.s = s, cam.hw = 0.0, cam.hh = 0.0;
  const int64_t n = (int64_t)W * H;
  const unsigned pix_blocks = (unsigned)((n + 255) / 256);
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const int tiles = tiles_x * tiles_y;
  const int slices = tiles >= 2048 ? 1 : (2048 / tiles > 32 ? 32 : 2048 / tiles);

  if (int rc = raster_reset_launch(hdr, st)) return rc;
  for (int m = 0; m < 2; ++m)
    if (int rc = raster_setup_launch(verts[m], V[m], faces[m], F[m], cam, sv[m], hdr, st)) return rc;
  hipLaunchKernelGGL(columns_zero_kernel, dim3(pix_blocks < 2048 ? pix_blocks : 2048), dim3(256), 0, st, cnt, n, hdr);
  if (int rc = check_launch("columns_zero_kernel")) return rc;
  for (int m = 0; m < 2; ++m) {
    hipLaunchKernelGGL(columns_bin_kernel<false>, dim3((unsigned)((F[m] + 255) / 256)), dim3(256), 0, st, sv[m], faces[m], F[m], W, H, s, m, cnt,
                       entries, capacity, big[m], hdr);
    if (int rc = check_launch("columns_bin_kernel<count>")) return rc;
    hipLaunchKernelGGL(columns_tile_kernel<false>, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, st, sv[m], faces[m], W, H, tiles_x, s, m, cnt,
                       entries, capacity, big[m], hdr);
    if (int rc = check_launch("columns_tile_kernel<count>")) return rc;
  }
  hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)l.scan_blocks), dim3(256), 0, st, cnt, n, block_sums, hdr);
  if (int rc = check_launch("scan_sums_kernel")) return rc;
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, st, block_sums, l.scan_blocks, capacity, hdr);
  if (int rc = check_launch("scan_top_kernel")) return rc;
  hipLaunchKernelGGL(scan_offsets_kernel, dim3((unsigned)l.scan_blocks), dim3(256), 0, st, cnt, n, block_sums, hdr);
  if (int rc = check_launch("scan_offsets_kernel")) return rc;
  for (int m = 0; m < 2; ++m) {
    hipLaunchKernelGGL(columns_bin_kernel<true>, dim3((unsigned)((F[m] + 255) / 256)), dim3(256), 0, st, sv[m], faces[m], F[m], W, H, s, m, cnt,
                       entries, capacity, big[m], hdr);
    if (int rc = check_launch("columns_bin_kernel<fill>")) return rc;
    hipLaunchKernelGGL(columns_tile_kernel<true>, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, st, sv[m], faces[m], W, H, tiles_x, s, m, cnt,
                       entries, capacity, big[m], hdr);
    if (int rc = check_launch("columns_tile_kernel<fill>")) return rc;
  }
  return COMA_OK;
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_mesh_volume_workspace_bytes(int F) { return F < 1 ? 0 : (size_t)volume_blocks(F) * sizeof(double); }

extern "C" int coma_mesh_volume_f64(const double* verts, int V, const int32_t* faces, int F, double* out, void* workspace, void* stream) {
  if (!verts || !faces || !out || !workspace) return fail(COMA_E_INVALID, "coma_mesh_volume_f64: null pointer");
  if (V < 1 || V > kRasterMaxPrims || F < 1 || F > kRasterMaxPrims)
    return fail(COMA_E_INVALID, "coma_mesh_volume_f64: V=%d, F=%d outside [1, %d]", V, F, kRasterMaxPrims);
  if ((uintptr_t)workspace % 8) return fail(COMA_E_INVALID, "coma_mesh_volume_f64: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = volume_blocks(F);
  hipLaunchKernelGGL(volume_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, verts, V, faces, F, (double*)workspace);
  if (int rc = check_launch("volume_partial_kernel")) return rc;
  hipLaunchKernelGGL(volume_final_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, out);
  return check_launch("volume_final_kernel");
}

extern "C" size_t coma_column_crossings_workspace_bytes(int VA, int FA, int VB, int FB, int W, int H, int64_t capacity) {
  if (!columns_sizes_ok(VA, FA, VB, FB, W, H, capacity)) return 0;
  return columns_layout(VA, FA, VB, FB, W, H, capacity).total;
}

extern "C" int coma_intersection_columns(const double* vertsA, int VA, const int32_t* facesA, int FA, const double* vertsB, int VB,
                                         const int32_t* facesB, int FB, double x0, double y0, double s, int W, int H, int64_t capacity,
                                         void* workspace, int64_t* sums, int64_t* col_ab, void* stream) {
  if (!vertsA || !facesA || !vertsB || !facesB || !workspace || !sums) return fail(COMA_E_INVALID, "coma_intersection_columns: null pointer");
  if (!columns_sizes_ok(VA, FA, VB, FB, W, H, capacity))
    return fail(COMA_E_INVALID, "coma_intersection_columns: V, F outside [1, %d], W, H outside [1, %d] or capacity outside [1, %lld]", kRasterMaxPrims,
                kRasterMaxDim, kMaxCapacity);
  if (!(s > 0.0) || !(s <= 1.7e308) || !__builtin_isfinite(x0) || !__builtin_isfinite(y0))
    return fail(COMA_E_INVALID, "coma_intersection_columns: s=%g must be positive and finite, the origin finite", s);
  if ((uintptr_t)workspace % 16) return fail(COMA_E_INVALID, "coma_intersection_columns: workspace must be 16-byte aligned");
  const ColumnsLayout l = columns_layout(VA, FA, VB, FB, W, H, capacity);
  char* ws = (char*)workspace;
  int* hdr = (int*)ws;
  const double* verts[2] = {vertsA, vertsB};
  const int* faces[2] = {facesA, facesB};
  const int V[2] = {VA, VB}, F[2] = {FA, FB};
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)W * H;
  const unsigned pix_blocks = (unsigned)((n + 255) / 256);
  unsigned* cnt = (unsigned*)(ws + l.cnt);
  long long* entries = (long long*)(ws + l.entries);
  if (int rc = columns_crossings_launch(verts, V, faces, F, x0, y0, s, W, H, (long long)capacity, ws, l, st)) return rc;
  hipLaunchKernelGGL(columns_sweep_kernel, dim3(pix_blocks), dim3(256), 0, st, cnt, entries, n, (long long*)col_ab, hdr);
  if (int rc = check_launch("columns_sweep_kernel")) return rc;
  hipLaunchKernelGGL(columns_finish_kernel, dim3(1), dim3(64), 0, st, hdr, (long long*)sums);
  return check_launch("columns_finish_kernel");
}

extern "C" int coma_intersection_status(const void* workspace, void* stream, int64_t* needed) {
  if (!workspace) return fail(COMA_E_INVALID, "coma_intersection_status: null pointer");
  long long head[3] = {0, 0, 0};   // status word + list length, list length + depth flag, crossings counted
  if (int rc = read_back(head, workspace, sizeof(head), stream, "coma_intersection_status")) return rc;
  const int word = (int)(head[0] & 0xffffffffll);
  if (needed) *needed = head[kHdrNeeded];
  if (word & kBadNonFinite) return fail(COMA_E_INVALID, "coma_intersection_columns: non-finite vertex (sums untouched)");
  if (word & kBadRange)
    return fail(COMA_E_INVALID, "coma_intersection_columns: a snapped coordinate exceeds +-2^25 (1/256-cell units; sums untouched)");
  if (word & kBadFace) return fail(COMA_E_INVALID, "coma_intersection_columns: face index outside [0, V) (sums untouched)");
  if (word & kBadDepth) return fail(COMA_E_INVALID, "coma_intersection_columns: a crossing's depth is non-finite or beyond +-2^40 (1/256-cell units; sums untouched)");
  if (word & kBadCapacity)
    return fail(COMA_E_INVALID, "coma_intersection_columns: capacity exceeded, %lld crossings needed (sums untouched)", head[kHdrNeeded]);
  return COMA_OK;
}
