// K7: nearest-vertex index map (gfx950).
// replaces: utils/coma.py:87-91 -- argmin_v sum((p_i - m_v)^2) over an f64 [V,P] table, first minimum
// wins ties (np.argmin).  One workgroup per query point, threads strided over the mesh vertices
// (coalesced 24-B records), f64 arithmetic in the reference's order ((dx^2+dy^2)+dz^2, no FMA), then a
// (distance, index) lexicographic min-reduction so the tie-break is identical.  np.argmin's NaN rule as well: a NaN distance
// counts as the minimum and the first one wins (nn_better, the mirror image of reduce.hip's np_better).
#include "common.h"

namespace coma {

// is (d, i) ahead of (bd, bi) in np.argmin's order?  A NaN beats any number, the lower index decides between equals.
__device__ __forceinline__ bool nn_better(double d, int i, double bd, int bi) {
  const bool dn = d != d, bn = bd != bd;
  if (dn != bn) return dn;
  if (dn) return i < bi;
  return d < bd || (d == bd && i < bi);
}

__global__ __launch_bounds__(256) void nearest_vertex_kernel(const double* __restrict__ pts,
                                                             const double* __restrict__ verts, int V,
                                                             int64_t* __restrict__ idx) {
  __shared__ double sd[4];
  __shared__ int si[4];
  const double px = pts[3 * (int64_t)blockIdx.x + 0], py = pts[3 * (int64_t)blockIdx.x + 1],
               pz = pts[3 * (int64_t)blockIdx.x + 2];
  double best = __builtin_inf();
  int bi = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += 256) {
    double dx = px - verts[3 * (int64_t)v + 0], dy = py - verts[3 * (int64_t)v + 1],
           dz = pz - verts[3 * (int64_t)v + 2];
    double d = (dx * dx + dy * dy) + dz * dz;
    if (nn_better(d, v, best, bi)) { best = d; bi = v; }   // (+inf, 0x7fffffff) loses to every vertex, a +inf distance included
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    double od = __shfl_xor(best, m);
    int oi = __shfl_xor(bi, m);
    if (nn_better(od, oi, best, bi)) { best = od; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (nn_better(sd[w], si[w], best, bi)) { best = sd[w]; bi = si[w]; }
    // V >= 1, so thread 0 has taken vertex 0 at the least and the start value is gone: a row of +inf distances gives 0, a row with
    // NaN distances its first NaN, every other row its first minimum -- np.argmin in all three
    idx[blockIdx.x] = (int64_t)bi;
  }
}

}  // namespace coma

using namespace coma;

extern "C" int coma_nearest_vertex_i64(const double* points, const double* verts, int P, int V,
                                       int64_t* idx, void* stream) {
  if (!points || !verts || !idx) return fail(COMA_E_INVALID, "coma_nearest_vertex_i64: null pointer");
  if (P < 0 || V <= 0) return fail(COMA_E_INVALID, "coma_nearest_vertex_i64: bad sizes P=%d V=%d", P, V);
  if (P == 0) return COMA_OK;
  hipLaunchKernelGGL(nearest_vertex_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, points,
                     verts, V, idx);
  return check_launch("nearest_vertex_kernel");
}
