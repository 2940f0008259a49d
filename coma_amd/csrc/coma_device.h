// Internal: device primitives shared by the coma:: kernel files -- the wave sums, the fixed-shape f64 workgroup sum and the f64
// 3-vector.  Every user promises reproducible bits (fixed summation shapes, -ffp-contract=off), so the shapes and associations
// below are part of that promise: changing one changes the bits of every caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace coma {

// butterfly: every lane gets the sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// integer, so the order does not matter: the sum is valid in lane 0
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// Sum of v over the kThreads threads of the workgroup in a fixed shape: an LDS tree, lds[t] + lds[t + h] for h = kThreads / 2 ... 1;
// every thread gets it.  The leading barrier lets consecutive calls reuse one `lds` array; every thread of the workgroup must
// arrive (no early return ahead of a call).  triangulate.hip's block_sum_128 is a different shape (wave butterfly, then two
// partials) whose bits its tests pin: it stays there.
template <int kThreads>
__device__ __forceinline__ double block_sum(double v, double* lds) {
  const int t = threadIdx.x;
  __syncthreads();
  lds[t] = v;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) lds[t] = lds[t] + lds[t + h];
    __syncthreads();
  }
  return lds[0];
}

__device__ __forceinline__ double load(const float* p, int64_t i) { return (double)p[i]; }
__device__ __forceinline__ double load(const double* p, int64_t i) { return p[i]; }

// f64 3-vector; dot and norm associate as (x x + y y) + z z
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ D3 operator/(D3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double norm(D3 a) { return sqrt(dot(a, a)); }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
template <typename T>
__device__ __forceinline__ D3 load3(const T* p, int64_t i) { return {load(p, 3 * i), load(p, 3 * i + 1), load(p, 3 * i + 2)}; }

}  // namespace coma
