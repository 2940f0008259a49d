// Weighted sample elimination (Yuksel 2015), the method behind open3d's sample_points_poisson_disk (gfx950).
// The serial definition is kept so that the result is bit-identical to the NumPy restatement in tests/sample_elim_ref.py:
//   d_ij = sqrt(((xi-xj)^2 + (yi-yj)^2) + (zi-zj)^2), pairs with d_ij >= r_max contribute nothing,
//   w_ij = ((t*t)^2)^2 with t = 1 - max(d_ij, r_min)/r_max (alpha = 8), w_i = sum of w_ij over j != i in ASCENDING j;
//   then, until n_keep points are alive: the alive point of largest w goes (lowest index on ties) and every alive neighbour j
//   of it gets one w_j -= w_ij.  All f64, no FMA (-ffp-contract=off), sqrt and / correctly rounded: nothing depends on scheduling.
// Phase 1 (grid-wide): initial weights, one thread per point, j tiled through LDS in ascending order; also writes an SoA copy
//   of the points so that phase 2 reads 512-B rows.
// Phase 2 (ONE workgroup of 1024 threads, no inter-workgroup waiting anywhere): thread t owns the strip j = t, t+1024, ... of the
//   weights for the whole loop (LDS when M <= 16384, the workspace otherwise), so a step needs one barrier: strip maximum ->
//   wave reduction -> 16 (weight, index) slots in LDS (double-buffered by step parity) -> every thread reduces the 16 slots
//   itself -> each thread updates the alive points of its strip against the removed point.  A dead point holds -inf.
// A pair is tested on its squared distance first (s > r_max^2 (1 + 1e-9) implies sqrt(s) > r_max, sqrt being monotonic), so the
// sqrt and the division run only for pairs near or inside the radius; the test skips no pair that contributes.
#include "common.h"

namespace coma {

constexpr int kElimThreads = 1024;
constexpr int kElimWaves = kElimThreads / kWave;
constexpr int kElimLdsMaxM = 16384;   // 128 KB of f64 weights + the static slots stay inside the 160 KB of a workgroup
constexpr int kElimMaxM = 65536;
constexpr int kInitThreads = 256;

__device__ __forceinline__ bool elim_pair_weight(double xi, double yi, double zi, double xj, double yj, double zj, double r_max,
                                                 double r_min, double r2hi, double& wij) {
  const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const double s = (dx * dx + dy * dy) + dz * dz;
  if (!(s <= r2hi)) return false;
  const double d = sqrt(s);
  if (!(d < r_max)) return false;
  const double dh = d < r_min ? r_min : d;
  const double t = 1.0 - dh / r_max;
  const double t2 = t * t, t4 = t2 * t2;
  wij = t4 * t4;
  return true;
}

__global__ __launch_bounds__(kInitThreads) void elim_init_kernel(const double* __restrict__ pts, int M, double r_max, double r_min,
                                                                 double r2hi, double* __restrict__ x, double* __restrict__ y,
                                                                 double* __restrict__ z, double* __restrict__ w) {
  __shared__ double tx[kInitThreads], ty[kInitThreads], tz[kInitThreads];
  const int i = blockIdx.x * kInitThreads + threadIdx.x;
  double xi = 0.0, yi = 0.0, zi = 0.0;
  if (i < M) {
    xi = pts[3 * (int64_t)i + 0], yi = pts[3 * (int64_t)i + 1], zi = pts[3 * (int64_t)i + 2];
    x[i] = xi, y[i] = yi, z[i] = zi;
  }
  double acc = 0.0;
  for (int j0 = 0; j0 < M; j0 += kInitThreads) {
    const int jl = j0 + threadIdx.x;
    if (jl < M) {
      tx[threadIdx.x] = pts[3 * (int64_t)jl + 0], ty[threadIdx.x] = pts[3 * (int64_t)jl + 1];
      tz[threadIdx.x] = pts[3 * (int64_t)jl + 2];
    }
    __syncthreads();
    const int n = min(kInitThreads, M - j0);
    if (i < M) {
      for (int k = 0; k < n; ++k) {   // ascending j: the order of the sum is part of the contract
        double wij;
        if (j0 + k != i && elim_pair_weight(xi, yi, zi, tx[k], ty[k], tz[k], r_max, r_min, r2hi, wij)) acc += wij;
      }
    }
    __syncthreads();
  }
  if (i < M) w[i] = acc;
}

__global__ __launch_bounds__(256) void elim_iota_kernel(int M, int64_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) keep[i] = i;
}

// (weight, index) order of the argmax: larger weight first, lower index on equal weight
__device__ __forceinline__ bool elim_before(double wa, int ia, double wb, int ib) { return wa > wb || (wa == wb && ia < ib); }

template <bool kLdsW>
__global__ __launch_bounds__(kElimThreads) void elim_loop_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                 const double* __restrict__ z, double* __restrict__ wg, int M,
                                                                 int n_keep, double r_max, double r_min, double r2hi,
                                                                 int64_t* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) double elim_w[];
  __shared__ double sbest[2][kElimWaves];
  __shared__ int sidx[2][kElimWaves];
  __shared__ int scount[kElimThreads];
  const int t = threadIdx.x;
  const double ninf = -__builtin_inf();
  double* w = kLdsW ? elim_w : wg;
  if (kLdsW)
    for (int j = t; j < M; j += kElimThreads) w[j] = wg[j];   // a thread only ever touches its own strip: no barrier needed

  const int steps = M - n_keep;
  for (int step = 0; step < steps; ++step) {
    const int p = step & 1;
    double best = ninf;
    int bi = 0x7fffffff;
    for (int j = t; j < M; j += kElimThreads) {
      double v = w[j];
      if (v != v) v = __builtin_inf();   // np.argmax takes the first NaN; only non-finite input gets here
      if (v > best) { best = v; bi = j; }   // ascending j per thread: strict > keeps the lowest index
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ow = __shfl_xor(best, m);
      const int oi = __shfl_xor(bi, m);
      if (elim_before(ow, oi, best, bi)) { best = ow; bi = oi; }
    }
    if ((t & 63) == 0) { sbest[p][t >> 6] = best; sidx[p][t >> 6] = bi; }
    __syncthreads();
    best = sbest[p][0], bi = sidx[p][0];
#pragma unroll
    for (int k = 1; k < kElimWaves; ++k)
      if (elim_before(sbest[p][k], sidx[p][k], best, bi)) { best = sbest[p][k]; bi = sidx[p][k]; }
    if (bi >= M) break;   // nothing selectable (non-finite input): uniform over the workgroup; the output below stays in bounds
    const double xi = x[bi], yi = y[bi], zi = z[bi];
    for (int j = t; j < M; j += kElimThreads) {
      const double v = w[j];
      if (j == bi) { w[j] = ninf; continue; }
      if (v == ninf) continue;
      double wij;
      if (elim_pair_weight(xi, yi, zi, x[j], y[j], z[j], r_max, r_min, r2hi, wij)) w[j] = v - wij;
    }
  }

  // surviving indices in ascending order: contiguous chunk per thread, counts scanned through LDS
  __syncthreads();
  const int chunk = (M + kElimThreads - 1) / kElimThreads;
  const int lo = min(M, t * chunk), hi = min(M, lo + chunk);
  int cnt = 0;
  for (int j = lo; j < hi; ++j) cnt += w[j] != ninf;
  scount[t] = cnt;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < kElimThreads; ++k) { const int c = scount[k]; scount[k] = run; run += c; }
  }
  __syncthreads();
  int pos = scount[t];
  for (int j = lo; j < hi; ++j)
    if (w[j] != ninf) {
      if (pos < n_keep) keep[pos] = j;
      ++pos;
    }
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_sample_eliminate_workspace_bytes(int M) {
  return M > 0 ? (size_t)M * 4 * sizeof(double) : 0;   // SoA copy of the points (x, y, z) + the weights
}

extern "C" int coma_sample_eliminate_f64(const double* points, int M, int n_keep, double r_max, double r_min, double alpha,
                                         void* workspace, int64_t* keep_idx, void* stream) {
  if (!points || !workspace || !keep_idx) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: null pointer");
  if (M < 1 || M > kElimMaxM) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: M=%d outside [1, %d]", M, kElimMaxM);
  if (n_keep < 1 || n_keep > M) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: n_keep=%d outside [1, M=%d]", n_keep, M);
  if (alpha != 8.0) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: alpha=%g is not supported (only 8)", alpha);
  if (!(r_max > 0.0) || r_max > 1.7e308) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: r_max=%g must be positive and finite", r_max);
  if (!(r_min >= 0.0 && r_min < r_max)) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: r_min=%g outside [0, r_max=%g)", r_min, r_max);
  if ((uintptr_t)workspace % sizeof(double)) return fail(COMA_E_INVALID, "coma_sample_eliminate_f64: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (n_keep == M) {
    hipLaunchKernelGGL(elim_iota_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, M, keep_idx);
    return check_launch("elim_iota_kernel");
  }
  double* x = (double*)workspace;
  double *y = x + M, *z = y + M, *w = z + M;
  const double r2hi = r_max * r_max * (1.0 + 1e-9);
  hipLaunchKernelGGL(elim_init_kernel, dim3((unsigned)((M + kInitThreads - 1) / kInitThreads)), dim3(kInitThreads), 0, st, points,
                     M, r_max, r_min, r2hi, x, y, z, w);
  if (int rc = check_launch("elim_init_kernel")) return rc;
  if (M <= kElimLdsMaxM) {
    static LdsOptIn slot;
    const size_t lds = (size_t)M * sizeof(double);
    if (lds > 48 * 1024)
      if (int rc = opt_in_lds(slot, (const void*)elim_loop_kernel<true>, lds, "coma_sample_eliminate_f64")) return rc;
    hipLaunchKernelGGL(elim_loop_kernel<true>, dim3(1), dim3(kElimThreads), lds, st, x, y, z, w, M, n_keep, r_max, r_min, r2hi,
                       keep_idx);
  } else {
    hipLaunchKernelGGL(elim_loop_kernel<false>, dim3(1), dim3(kElimThreads), 0, st, x, y, z, w, M, n_keep, r_max, r_min, r2hi,
                       keep_idx);
  }
  return check_launch("elim_loop_kernel");
}
