// The SMPL-X body model -- linear blend skinning of a template over a joint tree -- forward and backward, for gfx950.
// replaces: the third-party `smplx` package behind the `body_model` hook of src/application/optimize.py (called and differentiated
// in every one of its 2000 iterations, several dozen eager launches each way) and of src/generation/optimize_depth.py, by three
// launches forward and three backward on the caller's stream.  Rule set: include/coma_hip.h; restated in f64 in tests/smplx_ref.py.
//
// In the project's own words.  The packed parameters theta are axis-angle vectors for the leading joints followed by the
// coefficients of the two hands; the hands' axis-angles are the coefficients times the model's hand components, and the model's
// mean pose is added to all of it.  Every joint's axis-angle r becomes a rotation by Rodrigues' formula with the angle taken as the
// norm of (r + 1e-8), the epsilon added to each component: the formula and its derivative stay finite at r = 0, which is where the
// app starts.  The shape stage (once per betas) moves the template along the shape directions and regresses the rest joints from
// it.  The pose stage walks the tree from the root, G_i = G_parent [R_i | J_i - J_parent], and takes the rest pose out again:
// A_i = [G_i.R | G_i.t - G_i.R J_i].  The skinning stage adds the pose-dependent offsets (the entries of R_i - I for i >= 1 times
// `posedirs`) to the shaped template, blends the A_i with the vertex's weights and applies the blend.  The backward walks all of
// that in reverse from dL/dvertices to dL/dtheta and dL/dtransl; betas, expression and the joint outputs get NO gradient.
// The FULL backward (coma_smplx_backward_full_f32) is the same three launches with additions: dL/djoints of the extra joints is
// gathered into an effective vertex gradient first; dL/djoints of the posed joints and dL/dfull_pose are injected into the chain
// kernel, which also collects the gradient of the rest joints; J_regressor^T and shapedirs^T carry that and the skinning's dL/dv_posed
// back to the coefficients.  Up to three launches more; with none of its inputs given it is the backward, bit for bit.  COAP's own
// backward is not built on it yet: src/application/optimize.py --use_collision stays refused.
//
// Everything is evaluated in f64 on f32 inputs (as the rest of the per-vertex code of this library: V = 10 475 and a 55-joint
// chain are latency- and bandwidth-bound, the f64 rate does not show), so the outputs are the f32 rounding of the rule set.  The
// one large operand is posedirs [P, 3V] (61 MB): forward reads it with threads along the 3V axis and the P rows split over
// kPSplit workgroups per column block, so that about a thousand workgroups keep loads in flight; backward reads the same rows as
// P dot products, one workgroup each.  No transposed copy.  No floating-point atomics: every sum over vertices is per-workgroup
// (fixed order inside), then one fixed-order pass over the workgroups, so two calls give the same bits.
//
// There is ONE kernel per stage and it poses N bodies: body n is found from body 0's pointers through BatchStrides, and the
// single-body entry points are the batch of one (N = 1, the same launches with grids of one body), so body n of a batch has the
// bits of the single-body call.  N only changes how often the operands move: a sweep over posedirs serves C bodies (their features
// in LDS, one f64 sum per body in registers), a skinning workgroup stages its weights tile once and walks B bodies over it, the pose
// stage runs one workgroup per body.  C and B are template arguments: kChunk and kSkinChunk, and 1 at N = 1, where the compiler then
// gives the code of a kernel written for one body (Layout picks them and the grids that go with them).
#include "coma_device.h"
#include "fit_stages.h"

#include <cmath>

namespace coma {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 128;        // vertices (and threads) per skinning workgroup: weights tile 128 x 64 f32 = 32 KB of LDS
constexpr int kPSplit = 8;        // splits of the P rows of posedirs in the forward
constexpr int kMaxRows = (9 * (kMaxJ - 1) + kPSplit - 1) / kPSplit;
constexpr int kMaxPca = 64;
constexpr int kMaxBatch = 1024;   // N: bodies per call (coma_smplx_*_batch_f32; the single-body entry points are N = 1)
constexpr int kChunk = 8;         // C: bodies served by one sweep over posedirs (16 VGPRs of f64 sums per thread; forward LDS 71 x 8 f64)
constexpr int kSkinChunk = 2;     // bodies one skinning workgroup walks over its staged weights tile

// ---- shape stage ----
__global__ __launch_bounds__(kBlock) void smplx_shape_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                            const float* __restrict__ coef, int n3, int NB, double* __restrict__ v_shaped) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n3) return;
  double acc = 0.0;
  for (int l = 0; l < NB; ++l) acc = acc + (double)coef[l] * (double)shapedirs[(int64_t)i * NB + l];
  v_shaped[i] = (double)v_template[i] + acc;
}

// one workgroup per (joint, coordinate pair is folded: three sums in one pass)
__global__ __launch_bounds__(kBlock) void smplx_jrest_kernel(const float* __restrict__ J_regressor, const double* __restrict__ v_shaped, int V,
                                                            double* __restrict__ j_rest) {
  __shared__ double lds[kBlock];
  const int j = blockIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  for (int v = threadIdx.x; v < V; v += kBlock) {
    const double w = (double)J_regressor[(int64_t)j * V + v];
    s[0] = s[0] + w * v_shaped[3 * (int64_t)v];
    s[1] = s[1] + w * v_shaped[3 * (int64_t)v + 1];
    s[2] = s[2] + w * v_shaped[3 * (int64_t)v + 2];
  }
  for (int c = 0; c < 3; ++c) {
    const double r = block_sum<kBlock>(s[c], lds);
    if (threadIdx.x == 0) j_rest[3 * j + c] = r;
  }
}

// ---- pose stage ----
struct Rod { double a, x, y, z, s, c; };

__device__ __forceinline__ Rod rod_of(const double* r) {
  const double e = 1e-8;
  const double x0 = r[0] + e, y0 = r[1] + e, z0 = r[2] + e;
  Rod q;
  q.a = sqrt((x0 * x0 + y0 * y0) + z0 * z0);
  q.x = r[0] / q.a; q.y = r[1] / q.a; q.z = r[2] / q.a;
  q.s = sin(q.a); q.c = cos(q.a);
  return q;
}

// K = [[0,-z,y],[z,0,-x],[-y,x,0]] and K K of the unit-ish direction
__device__ __forceinline__ void skew(const Rod& q, double* K, double* K2) {
  K[0] = 0.0; K[1] = -q.z; K[2] = q.y; K[3] = q.z; K[4] = 0.0; K[5] = -q.x; K[6] = -q.y; K[7] = q.x; K[8] = 0.0;
  K2[0] = -(q.y * q.y + q.z * q.z); K2[1] = q.x * q.y; K2[2] = q.x * q.z;
  K2[3] = q.x * q.y; K2[4] = -(q.x * q.x + q.z * q.z); K2[5] = q.y * q.z;
  K2[6] = q.x * q.z; K2[7] = q.y * q.z; K2[8] = -(q.x * q.x + q.y * q.y);
}

__device__ __forceinline__ void rodrigues(const double* r, double* R) {
  const Rod q = rod_of(r);
  double K[9], K2[9];
  skew(q, K, K2);
  const double c1 = 1.0 - q.c;
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = ((e % 4 == 0) ? 1.0 : 0.0) + (q.s * K[e] + c1 * K2[e]);
}

// dL/dr from dL/dR, the +1e-8 inside the norm included
__device__ __forceinline__ void rodrigues_backward(const double* r, const double* dR, double* dr) {
  const Rod q = rod_of(r);
  double K[9], K2[9], dK[9];
  skew(q, K, K2);
  const double c1 = 1.0 - q.c;
  double da = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) da = da + dR[e] * (q.c * K[e] + q.s * K2[e]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double m = 0.0;                                     // (dR K^T + K^T dR)[i][j]
#pragma unroll
      for (int k = 0; k < 3; ++k) m = m + (dR[3 * i + k] * K[3 * j + k] + K[3 * k + i] * dR[3 * k + j]);
      dK[3 * i + j] = q.s * dR[3 * i + j] + c1 * m;
    }
  const double dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
  const double dat = da - ((dd[0] * r[0] + dd[1] * r[1]) + dd[2] * r[2]) / (q.a * q.a);
#pragma unroll
  for (int k = 0; k < 3; ++k) dr[k] = dd[k] / q.a + dat * ((r[k] + 1e-8) / q.a);
}

// R [J,9] and the chain G [J,3x4] in LDS from pose [3J] (LDS) and the rest joints; serial in the joint index (parent[i] < i)
__device__ __forceinline__ void pose_chain(const double* pose, const double* __restrict__ j_rest, const Tree& tree, int J, double* R, double* G) {
  const int t = threadIdx.x;
  if (t < J) rodrigues(pose + 3 * t, R + 9 * t);
  __syncthreads();
  if (t < 12) G[t] = (t % 4 < 3) ? R[3 * (t / 4) + t % 4] : j_rest[t / 4];
  __syncthreads();
  for (int i = 1; i < J; ++i) {
    const int p = tree.parent[i];
    if (t < 12) {
      const int r = t / 4, c = t % 4;
      const double* Gp = G + 12 * p + 4 * r;
      double v;
      if (c < 3) {
        v = (Gp[0] * R[9 * i + c] + Gp[1] * R[9 * i + 3 + c]) + Gp[2] * R[9 * i + 6 + c];
      } else {
        const double tx = j_rest[3 * i] - j_rest[3 * p], ty = j_rest[3 * i + 1] - j_rest[3 * p + 1], tz = j_rest[3 * i + 2] - j_rest[3 * p + 2];
        v = ((Gp[0] * tx + Gp[1] * ty) + Gp[2] * tz) + Gp[3];
      }
      G[12 * i + t] = v;
    }
    __syncthreads();
  }
}

template <typename T>
__device__ __forceinline__ T* at_bytes(T* p, size_t bytes) {
  return (T*)((char*)p + bytes);
}
template <typename T>
__device__ __forceinline__ const T* at_bytes(const T* p, size_t bytes) {
  return (const T*)((const char*)p + bytes);
}

// what differs from body to body
struct PoseBody {
  const float* theta;
  const float* transl;
  const double* j_rest;
  double* s_pose;
  double* s_A;
  double* feat;
  float* joints;
  float* full_pose;
};

__device__ __forceinline__ void pose_forward(const PoseArgs& a, const PoseBody& b) {
  __shared__ double pose[3 * kMaxJ], R[9 * kMaxJ], G[12 * kMaxJ];
  const int t = threadIdx.x, J = a.J;
  const int nb = a.n_pca > 0 ? 3 * J - 2 * a.hd : 3 * J;
  for (int k = t; k < 3 * J; k += kBlock) {
    double v;
    if (k < nb) {
      v = (double)b.theta[k];
    } else {
      const int h = (k - nb) / a.hd, kk = (k - nb) % a.hd;
      v = 0.0;
      for (int i = 0; i < a.n_pca; ++i) v = v + (double)b.theta[nb + h * a.n_pca + i] * (double)a.comps[(int64_t)(h * a.n_pca + i) * a.hd + kk];
    }
    if (a.mean) v = v + (double)a.mean[k];
    pose[k] = v;
    b.s_pose[k] = v;
    if (b.full_pose) b.full_pose[k] = (float)v;
  }
  __syncthreads();
  pose_chain(pose, b.j_rest, a.tree, J, R, G);
  for (int q = t; q < 12 * J; q += kBlock) {
    const int i = q / 12, r = (q % 12) / 4, c = q % 4;
    const double* Gi = G + 12 * i + 4 * r;
    double v = Gi[c];
    if (c == 3) {
      v = v - ((Gi[0] * b.j_rest[3 * i] + Gi[1] * b.j_rest[3 * i + 1]) + Gi[2] * b.j_rest[3 * i + 2]);
      b.joints[3 * i + r] = (float)(Gi[3] + (b.transl ? (double)b.transl[r] : 0.0));
    }
    b.s_A[q] = v;
  }
  for (int q = t; q < 9 * (J - 1); q += kBlock) b.feat[q] = R[9 + q] - ((q % 9) % 4 == 0 ? 1.0 : 0.0);
}

// one workgroup per body
__global__ __launch_bounds__(kBlock) void smplx_pose_kernel(PoseArgs a, BatchStrides st) {
  const size_t n = blockIdx.x;
  const int J = a.J;
  pose_forward(a, PoseBody{a.theta + n * st.NT, a.transl ? a.transl + 3 * n : nullptr, at_bytes(a.j_rest, n * st.shape), at_bytes(a.s_pose, n * st.saved),
                           at_bytes(a.s_A, n * st.saved), a.feat + n * (size_t)(9 * (J - 1)), a.joints + n * (size_t)(3 * J),
                           a.full_pose ? a.full_pose + n * (size_t)(3 * J) : nullptr});
}

// ---- skinning stage ----
// Partial pose offsets: part[n][s][i] = sum over the rows p of split s (ascending) of feat[n][p] posedirs[p][i].  Grid (column blocks,
// kPSplit, chunks of C bodies).  The chunk's features of this split sit in LDS as [row][body]; every posedirs element is loaded once
// and used for all bodies of the chunk, each body's sum in a register of its own.  With P = 0 (J = 1) it writes zeros.  C = 1 is the
// instantiation for one body: no f64 work for absent bodies.
template <int C>
__global__ __launch_bounds__(kBlock) void smplx_offsets_kernel(const float* __restrict__ posedirs, const double* __restrict__ feat, int P, int n3,
                                                              int rows, int N, double* __restrict__ part) {
  __shared__ double f[kMaxRows * C];
  const int s = blockIdx.y, n0 = blockIdx.z * C, nc = min(C, N - n0);
  const int p0 = s * rows, p1 = min(P, p0 + rows);
  for (int q = threadIdx.x; q < (p1 - p0) * C; q += kBlock) {
    const int r = q / C, c = q % C;
    f[q] = (C == 1 || c < nc) ? feat[(int64_t)(n0 + c) * P + p0 + r] : 0.0;
  }
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n3) return;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
  const float* col = posedirs + i;
#pragma unroll C == 1 ? 8 : 4
  for (int p = p0; p < p1; ++p) {
    const double x = (double)col[(int64_t)p * n3];
    const double* fp = f + (p - p0) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = acc[c] + fp[c] * x;
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (C == 1 || c < nc) part[((int64_t)(n0 + c) * kPSplit + s) * n3 + i] = acc[c];
}

// the weights of this workgroup's tile of vertices (one contiguous run of the [V,J] table) into LDS (no barrier: the first stage_A
// gives it) -> the vertices in the tile
__device__ __forceinline__ int stage_weights(const float* __restrict__ weights, int V, int J, float* Wt) {
  const int v0 = blockIdx.x * kTile, n = min(kTile, V - v0);
  const float* src = weights + (int64_t)v0 * J;
  for (int q = threadIdx.x; q < n * J; q += kTile) Wt[q] = src[q];
  return n;
}

// the next body's transforms into LDS, once every thread is done with the previous body's (the chunk's first body has none before it)
__device__ __forceinline__ void stage_A(const double* __restrict__ A, int J, double* Al, bool first) {
  if (!first) __syncthreads();
  for (int q = threadIdx.x; q < 12 * J; q += kTile) Al[q] = A[q];
  __syncthreads();
}

__device__ __forceinline__ void blend(const float* w, const double* Al, int J, double* T) {
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.0;
  for (int j = 0; j < J; ++j) {
    const double wj = (double)w[j];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = T[e] + wj * Al[12 * j + e];
  }
}

// vertex v of one body (thread t of its tile): the pose offset from the eight partial sums, the blend, the vertex
__device__ __forceinline__ void skin_vertex(const float* Wt, const double* Al, int V, int J, int64_t v, int t, const double* __restrict__ part,
                                            const double* __restrict__ v_shaped, const float* __restrict__ transl, double* __restrict__ v_posed,
                                            float* __restrict__ vertices) {
  const int64_t n3 = 3 * (int64_t)V;
  double vp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double off = 0.0;
    for (int s = 0; s < kPSplit; ++s) off = off + part[s * n3 + 3 * v + c];
    vp[c] = v_shaped[3 * v + c] + off;
    v_posed[3 * v + c] = vp[c];
  }
  double T[12];
  blend(Wt + t * J, Al, J, T);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double x = ((T[4 * c] * vp[0] + T[4 * c + 1] * vp[1]) + T[4 * c + 2] * vp[2]) + T[4 * c + 3];
    vertices[3 * v + c] = (float)(x + (transl ? (double)transl[c] : 0.0));
  }
}

// Grid (tiles, chunks of B bodies); part is [N][kPSplit][3V].  The weights tile is staged once and the chunk's bodies walk over it.
// B = 1 is the instantiation for one body: no body loop, so the compiler gives it the code of a kernel written for one body.
template <int B>
__global__ __launch_bounds__(kTile) void smplx_skin_kernel(SkinArgs a, BatchStrides st) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  const int n = stage_weights(a.weights, a.V, a.J, Wt);
  const int t = threadIdx.x;
  const size_t n3 = 3 * (size_t)a.V, b0 = (size_t)blockIdx.y * B;
#pragma unroll 1
  for (int i = 0; i < B; ++i) {
    const size_t b = b0 + i;
    if (B > 1 && b >= (size_t)st.N) break;
    stage_A(at_bytes(a.A, b * st.saved), a.J, Al, i == 0);
    if (t < n)
      skin_vertex(Wt, Al, a.V, a.J, (int64_t)blockIdx.x * kTile + t, t, a.part + b * kPSplit * n3, at_bytes(a.v_shaped, b * st.shape),
                  a.transl ? a.transl + 3 * b : nullptr, at_bytes(a.v_posed, b * st.saved), a.vertices + b * n3);
  }
}

// ---- backward ----
template <typename TG>
struct SkinBwdArgs {
  const float* weights;
  const double* A;
  const double* v_posed;
  const TG* grad;           // dL/dvertices [V,3]: the caller's f32, or the f64 effective gradient of the full backward
  int V, J;
  double* gvp;              // workspace [V,3]: T[:3,:3]^T g
  double* dA_part;          // workspace [blocks][12 J + 3]: the block's share of dL/dA, then of dL/dtransl
};

// one body's tile, weights and transforms staged: g_vposed of its vertices, then the tile's share of dL/dA and dL/dtransl
template <typename TG>
__device__ __forceinline__ void skin_bwd_tile(const float* Wt, const double* Al, double* gl, double* vl, int n, int J, const TG* __restrict__ grad,
                                              const double* __restrict__ v_posed, double* __restrict__ gvp, double* __restrict__ dA_part) {
  const int t = threadIdx.x;
  if (t < n) {
    const int64_t v = (int64_t)blockIdx.x * kTile + t;
    double T[12];
    blend(Wt + t * J, Al, J, T);
    const double g[3] = {load(grad, 3 * v), load(grad, 3 * v + 1), load(grad, 3 * v + 2)};     // after the blend: not live across its loop
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gvp[3 * v + c] = (T[c] * g[0] + T[4 + c] * g[1]) + T[8 + c] * g[2];
      gl[3 * t + c] = g[c];
      vl[4 * t + c] = v_posed[3 * v + c];
    }
    vl[4 * t + 3] = 1.0;
  }
  __syncthreads();
  const int nq = 12 * J + 3;
  double* out = dA_part + (int64_t)blockIdx.x * nq;
  for (int q = t; q < nq; q += kTile) {
    double acc = 0.0;
    if (q < 12 * J) {
      const int j = q / 12, r = (q % 12) / 4, c = q % 4;
#pragma unroll 8                                            // asked for: inside the body loop the compiler no longer unrolls these on its own
      for (int u = 0; u < n; ++u) acc = acc + ((double)Wt[u * J + j] * gl[3 * u + r]) * vl[4 * u + c];
    } else {
      const int r = q - 12 * J;
#pragma unroll 8
      for (int u = 0; u < n; ++u) acc = acc + gl[3 * u + r];
    }
    out[q] = acc;
  }
}

// Grid (tiles, chunks of B bodies); grad and gvp are [N][3V], dA_part is [N][tiles][12 J + 3].  stage_A's barrier between two bodies
// also keeps the first one's gl / vl until every thread has summed over them.  B = 1 as in smplx_skin_kernel.
template <typename TG, int B>
__global__ __launch_bounds__(kTile) void smplx_skin_bwd_kernel(SkinBwdArgs<TG> a, BatchStrides st) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  __shared__ double gl[3 * kTile], vl[4 * kTile];
  const int n = stage_weights(a.weights, a.V, a.J, Wt);
  const size_t n3 = 3 * (size_t)a.V, per_body = (size_t)gridDim.x * (12 * a.J + 3), b0 = (size_t)blockIdx.y * B;
#pragma unroll 1
  for (int i = 0; i < B; ++i) {
    const size_t b = b0 + i;
    if (B > 1 && b >= (size_t)st.N) break;
    stage_A(at_bytes(a.A, b * st.saved), a.J, Al, i == 0);
    skin_bwd_tile(Wt, Al, gl, vl, n, a.J, a.grad + b * n3, at_bytes(a.v_posed, b * st.saved), a.gvp + b * n3, a.dA_part + b * per_body);
  }
}

// dL/dfeature_p of body n = <posedirs[p, :], gvp[n]>.  Grid (P rows, chunks of C bodies); one read of the row serves the chunk's dot
// products, each with 256 strided partial sums and the tree.  gvp is [N][3V], dfeat [N][P].  C = 1 is the instantiation for one body.
template <int C>
__global__ __launch_bounds__(kBlock) void smplx_feature_bwd_kernel(const float* __restrict__ posedirs, const double* __restrict__ gvp, int n3,
                                                                  int P, int N, double* __restrict__ dfeat) {
  __shared__ double lds[kBlock];
  const int n0 = blockIdx.y * C, nc = min(C, N - n0);
  const float* row = posedirs + (int64_t)blockIdx.x * n3;
  const double* g0 = gvp + (int64_t)n0 * n3;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll C == 1 ? 4 : 2
  for (int i = threadIdx.x; i < n3; i += kBlock) {
    const double x = (double)row[i];
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (C == 1 || c < nc) acc[c] = acc[c] + x * g0[(int64_t)c * n3 + i];
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (C == 1 || c < nc) {                                 // nc is the workgroup's: every thread reaches the same barriers
      const double s = block_sum<kBlock>(acc[c], lds);
      if (threadIdx.x == 0) dfeat[(int64_t)(n0 + c) * P + blockIdx.x] = s;
    }
}

// what differs from body to body
struct PoseBwdBody {
  const double* s_pose;
  const double* j_rest;
  const double* dA_part;
  const double* dfeat;
  float* grad_theta;
  float* grad_transl;
  const float* gJ;
  const float* gP;
  double* dJ_out;
};

__device__ __forceinline__ void pose_backward(const PoseBwdArgs& a, const PoseBwdBody& b) {
  __shared__ double pose[3 * kMaxJ], R[9 * kMaxJ], G[12 * kMaxJ], dG[12 * kMaxJ], dR[9 * kMaxJ], dJ[3 * kMaxJ];
  const int t = threadIdx.x, J = a.J;
  for (int k = t; k < 3 * J; k += kBlock) pose[k] = b.s_pose[k];
  __syncthreads();
  pose_chain(pose, b.j_rest, a.tree, J, R, G);
  // dL/dA and dL/dtransl: the workgroups' shares in block order; dA into G's place is not possible (G is needed), so into dR/dG
  const int nq = 12 * J + 3;
  double* dA = dG;                                        // dG is built from dA in place below
  for (int q = t; q < nq; q += kBlock) {
    double acc = 0.0;
    for (int w = 0; w < a.nblk; ++w) acc = acc + b.dA_part[(int64_t)w * nq + q];
    if (q < 12 * J) {
      dA[q] = acc;
    } else {
      const int r = q - 12 * J;
      if (b.gJ) {                                           // joints_i = G_i.t + transl, and the extra joints' direct term
        double posed = 0.0, direct = 0.0;
        for (int i = 0; i < J; ++i) posed = posed + (double)b.gJ[3 * i + r];
        for (int e = 0; e < a.E; ++e) {
          const double w = ((double)a.extra_w[3 * e] + (double)a.extra_w[3 * e + 1]) + (double)a.extra_w[3 * e + 2];
          direct = direct + (1.0 - w) * (double)b.gJ[3 * (J + e) + r];
        }
        acc = (acc + posed) + direct;
      }
      b.grad_transl[r] = (float)acc;
    }
  }
  __syncthreads();
  // A = [G.R | G.t - G.R J]: dG.t = dA.t, dG.R = dA.R - dA.t J^T   (each entry reads its own row's dA.t, which is not rewritten)
  for (int q = t; q < 12 * J; q += kBlock) {
    const int i = q / 12, r = (q % 12) / 4, c = q % 4;
    if (c < 3) dG[q] = dA[q] - dA[12 * i + 4 * r + 3] * b.j_rest[3 * i + c];
  }
  if (b.dJ_out)                                           // ... and dJ_i = -G_i.R^T dA_i.t
    for (int q = t; q < 3 * J; q += kBlock) {
      const int i = q / 3, c = q % 3;
      dJ[q] = -((G[12 * i + c] * dA[12 * i + 3] + G[12 * i + 4 + c] * dA[12 * i + 7]) + G[12 * i + 8 + c] * dA[12 * i + 11]);
    }
  __syncthreads();
  if (b.gJ) {                                             // dG_i.t += dL/djoints_i, once dA.t has been read
    for (int q = t; q < 3 * J; q += kBlock) dG[12 * (q / 3) + 4 * (q % 3) + 3] = dG[12 * (q / 3) + 4 * (q % 3) + 3] + (double)b.gJ[q];
    __syncthreads();
  }
  for (int i = J - 1; i >= 1; --i) {
    const int p = a.tree.parent[i];
    if (t < 9) {                                          // dR_i = G_p.R^T dG_i.R + dL/dfeature
      const int r = t / 3, c = t % 3;
      double v = (G[12 * p + r] * dG[12 * i + c] + G[12 * p + 4 + r] * dG[12 * i + 4 + c]) + G[12 * p + 8 + r] * dG[12 * i + 8 + c];
      dR[9 * i + t] = v + b.dfeat[9 * (i - 1) + t];
    } else if (t >= 16 && t < 28) {                       // dG_p.R += dG_i.R R_i^T + dG_i.t t_i^T;  dG_p.t += dG_i.t
      const int e = t - 16, r = e / 4, c = e % 4;
      const double* di = dG + 12 * i + 4 * r;
      double add;
      if (c < 3) {
        const double tc = b.j_rest[3 * i + c] - b.j_rest[3 * p + c];
        add = ((di[0] * R[9 * i + 3 * c] + di[1] * R[9 * i + 3 * c + 1]) + di[2] * R[9 * i + 3 * c + 2]) + di[3] * tc;
      } else {
        add = di[3];
      }
      dG[12 * p + e] = dG[12 * p + e] + add;
    } else if (t >= 32 && t < 35 && b.dJ_out) {            // G_i.t = G_p.R (J_i - J_p) + G_p.t: u = G_p.R^T dG_i.t to J_i, -u to J_p
      const int c = t - 32;
      const double u = (G[12 * p + c] * dG[12 * i + 3] + G[12 * p + 4 + c] * dG[12 * i + 7]) + G[12 * p + 8 + c] * dG[12 * i + 11];
      dJ[3 * i + c] = dJ[3 * i + c] + u;
      dJ[3 * p + c] = dJ[3 * p + c] - u;
    }
    __syncthreads();
  }
  if (b.dJ_out) {                                         // the root: G_0.t = J_0
    if (t >= 32 && t < 35) dJ[t - 32] = dJ[t - 32] + dG[4 * (t - 32) + 3];
    __syncthreads();
    for (int q = t; q < 3 * J; q += kBlock) b.dJ_out[q] = dJ[q];
  }
  if (t < 9) dR[t] = dG[4 * (t / 3) + t % 3];
  __syncthreads();
  double* dpose = G;                                      // the chain is no longer needed
  if (t < J) {
    double dr[3];
    rodrigues_backward(pose + 3 * t, dR + 9 * t, dr);
    if (b.gP) {                                           // full_pose = assembled theta + pose_mean
      dr[0] = dr[0] + (double)b.gP[3 * t]; dr[1] = dr[1] + (double)b.gP[3 * t + 1]; dr[2] = dr[2] + (double)b.gP[3 * t + 2];
    }
    dpose[3 * t] = dr[0]; dpose[3 * t + 1] = dr[1]; dpose[3 * t + 2] = dr[2];
  }
  __syncthreads();
  const int nb = a.n_pca > 0 ? 3 * J - 2 * a.hd : 3 * J;
  for (int k = t; k < nb; k += kBlock) b.grad_theta[k] = (float)dpose[k];
  for (int q = t; q < 2 * a.n_pca; q += kBlock) {           // the hand components transposed
    const int h = q / a.n_pca;
    double acc = 0.0;
    for (int kk = 0; kk < a.hd; ++kk) acc = acc + (double)a.comps[(int64_t)q * a.hd + kk] * dpose[nb + h * a.hd + kk];
    b.grad_theta[nb + q] = (float)acc;
  }
}

// one workgroup per body; gJ is [N][J + E, 3]; the gradient to the rest joints is collected for a single body only
__global__ __launch_bounds__(kBlock) void smplx_pose_bwd_kernel(PoseBwdArgs a, BatchStrides st) {
  const size_t n = blockIdx.x;
  const int J = a.J;
  pose_backward(a, PoseBwdBody{at_bytes(a.s_pose, n * st.saved), at_bytes(a.j_rest, n * st.shape), a.dA_part + n * a.nblk * (size_t)(12 * J + 3),
                               a.dfeat + n * (size_t)(9 * (J - 1)), a.grad_theta + n * st.NT, a.grad_transl + 3 * n,
                               a.gJ ? a.gJ + n * (size_t)(3 * (J + a.E)) : nullptr, a.gP ? a.gP + n * (size_t)(3 * J) : nullptr,
                               st.N == 1 ? a.dJ_out : nullptr});
}

// ---- extra joints ----
// grid (blocks of 3E, N): vertices [N][V,3], transl [N][3] or null, out [N][E,3]; one table for all bodies
__global__ __launch_bounds__(kBlock) void smplx_gather_kernel(const float* __restrict__ vertices, const float* __restrict__ transl,
                                                             const int32_t* __restrict__ idx, const float* __restrict__ w, int V, int E,
                                                             float* __restrict__ out) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= 3 * E) return;
  const size_t n = blockIdx.y;
  vertices += n * 3 * (size_t)V;
  out += n * 3 * (size_t)E;
  if (transl) transl += 3 * n;
  const int e = q / 3, c = q % 3;
  const double tr = transl ? (double)transl[c] : 0.0;
  double acc = 0.0;
  for (int i = 0; i < 3; ++i) {
    const int v = idx[3 * e + i];
    const double x = (v >= 0 && v < V) ? (double)vertices[3 * (int64_t)v + c] - tr : (double)NAN;   // an index outside the mesh is not followed
    acc = acc + (double)w[3 * e + i] * x;
  }
  out[q] = (float)(acc + tr);
}

// ---- the full backward's own passes ----
constexpr int kMaxE = 4096;       // extra joints whose gradient is scattered back
constexpr int kEffChunk = 768;    // table entries in LDS per pass

// The effective vertex gradient: g_eff[v] = g[v] (zeros without g) + the sum over the table entries (e, i) with index v, in ascending
// (e, i), of w[e,i] gJ_extra[e].  Written as a gather -- every vertex scans the whole table from LDS -- so repeated indices (a vertex
// pick is (i, i, i), landmark faces share vertices) add in the table's order without atomics; an index outside [0, V) matches nothing.
// Grid (blocks of V, N): g [N][V,3] or null, g_eff [N][V,3]; gJ_extra is body 0's first extra-joint row of dL/djoints (or null), body
// n's is gJ_stride = 3 (J + E) floats on.
__global__ __launch_bounds__(kBlock) void smplx_effective_grad_kernel(const float* __restrict__ g, const float* __restrict__ gJ_extra,
                                                                     size_t gJ_stride, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ w, int V, int E, double* __restrict__ g_eff) {
  __shared__ int32_t li[kEffChunk];
  __shared__ double lw[3 * kEffChunk];
  const size_t n = blockIdx.y;
  if (g) g += n * 3 * (size_t)V;
  if (gJ_extra) gJ_extra += n * gJ_stride;
  g_eff += n * 3 * (size_t)V;
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  D3 acc = {0.0, 0.0, 0.0};
  if (g && v < V) acc = load3(g, v);
  for (int n0 = 0; n0 < 3 * E; n0 += kEffChunk) {
    const int m = min(kEffChunk, 3 * E - n0);
    __syncthreads();
    for (int q = threadIdx.x; q < m; q += kBlock) {
      const int k = n0 + q;
      const D3 c = load3(gJ_extra, k / 3) * (double)w[k];
      li[q] = idx[k];
      lw[3 * q] = c.x; lw[3 * q + 1] = c.y; lw[3 * q + 2] = c.z;
    }
    __syncthreads();
    if (v < V)
      for (int q = 0; q < m; ++q)
        if (li[q] == (int32_t)v) acc = acc + D3{lw[3 * q], lw[3 * q + 1], lw[3 * q + 2]};
  }
  if (v < V) { g_eff[3 * v] = acc.x; g_eff[3 * v + 1] = acc.y; g_eff[3 * v + 2] = acc.z; }
}

// kBlock rows i = 3 v + c of the [3V] axis per workgroup.  dL/dv_shaped[i] = gvp[i] + sum_j J_regressor[j, v] dJ[j][c] (j ascending)
// stays in LDS; then one thread per coefficient l sums shapedirs[i, l] dv_shaped[i] over the workgroup's rows in ascending order
// (threads along l read the [3V, NB] table contiguously) into part[workgroup][l].
__global__ __launch_bounds__(kBlock) void smplx_shape_bwd_kernel(const float* __restrict__ shapedirs, const float* __restrict__ J_regressor,
                                                                const double* __restrict__ gvp, const double* __restrict__ dJ, int V, int J, int NB,
                                                                double* __restrict__ part) {
  __shared__ double dJl[3 * kMaxJ], dv[kBlock];
  const int t = threadIdx.x;
  const int64_t n3 = 3 * (int64_t)V, i0 = (int64_t)blockIdx.x * kBlock, i = i0 + t;
  for (int q = t; q < 3 * J; q += kBlock) dJl[q] = dJ[q];
  __syncthreads();
  double x = 0.0;
  if (i < n3) {
    const int64_t v = i / 3;
    const int c = (int)(i % 3);
    double reg = 0.0;
    for (int j = 0; j < J; ++j) reg = reg + (double)J_regressor[(int64_t)j * V + v] * dJl[3 * j + c];
    x = gvp[i] + reg;
  }
  dv[t] = x;
  __syncthreads();
  const int rows = (int)min((int64_t)kBlock, n3 - i0);
  for (int l = t; l < NB; l += kBlock) {
    const float* col = shapedirs + i0 * NB + l;
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) acc = acc + (double)col[(int64_t)r * NB] * dv[r];
    part[(int64_t)blockIdx.x * NB + l] = acc;
  }
}

// dL/dcoefficient_l: the workgroups' shares in ascending order
__global__ __launch_bounds__(kBlock) void smplx_coef_sum_kernel(const double* __restrict__ part, int nblk, int NB, float* __restrict__ out) {
  const int l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= NB) return;
  double acc = 0.0;
  for (int b = 0; b < nblk; ++b) acc = acc + part[(int64_t)b * NB + l];
  out[l] = (float)acc;
}

// ---- the host half ----
constexpr int kMaxV = 1 << 24;
constexpr int kMaxNB = 1024;

// Every buffer of N bodies.  The forward workspace is feat [N][P], part [N][kPSplit][3V]; the backward workspace is gvp [N][3V],
// dA_part [N][tiles][12 J + 3], dfeat [N][P], g_eff [N][3V] (the batched backward's ends here), then dJ and coef_part of the full
// backward.  The single-body forward and vertices-only backward share ONE workspace: the forward blocks, then the backward blocks up
// to dfeat, which therefore sit `fwd_total` further on.  Body n's saved block is the single-body one at n x saved_stride.
struct Layout : SmplxGrids {
  size_t feat, part, fwd_total;                                                   // forward workspace
  size_t gvp, dA_part, dfeat, g_eff, dJ, coef_part, grad_total;                   // backward workspace
  size_t v_shaped, j_rest, shape_total;                                           // shape state
  size_t s_pose, s_A, s_vposed, saved_stride;                                     // saved by a forward for its backward
  size_t batch_grad_total() const { return dJ; }
  size_t single_total() const { return fwd_total + g_eff; }
};

Layout layout(int V, int J, int N = 1, int NB = 0) {
  Layout L = {};
  const size_t n3 = (size_t)3 * V, d = sizeof(double), n = (size_t)N;
  L.P = 9 * (J - 1);
  L.rows = (L.P + kPSplit - 1) / kPSplit;
  L.nblk = (V + kTile - 1) / kTile;
  L.nb3 = (int)((n3 + kBlock - 1) / kBlock);
  L.C = N == 1 ? 1 : kChunk;          // one body: the instantiations that do no work for absent bodies
  L.B = N == 1 ? 1 : kSkinChunk;
  L.chunks = (N + L.C - 1) / L.C;
  L.skin_chunks = (N + L.B - 1) / L.B;
  const size_t P = (size_t)(L.P > 0 ? L.P : 1);
  Carve fwd, bwd, shape, saved;
  L.feat = fwd.take(n * P * d);
  L.part = fwd.take(n * kPSplit * n3 * d);
  L.fwd_total = fwd.at;
  L.gvp = bwd.take(n * n3 * d);
  L.dA_part = bwd.take(n * L.nblk * (12 * J + 3) * d);
  L.dfeat = bwd.take(n * P * d);
  L.g_eff = bwd.take(n * n3 * d);
  L.dJ = bwd.take((size_t)3 * J * d);
  L.coef_part = bwd.take((size_t)L.nb3 * (NB > 0 ? NB : 1) * d);
  L.grad_total = bwd.at;
  L.v_shaped = shape.take(n3 * d);
  L.j_rest = shape.take((size_t)3 * J * d);
  L.shape_total = shape.at;
  L.s_pose = saved.take((size_t)3 * J * d);
  L.s_A = saved.take((size_t)12 * J * d);
  L.s_vposed = saved.take(n3 * d);
  L.saved_stride = saved.at;
  return L;
}

bool sizes_ok(int V, int J, int N = 1) { return V >= 1 && V <= kMaxV && J >= 1 && J <= kMaxJ && N >= 1 && N <= kMaxBatch; }

// what every forward and backward refuses after its null pointers; fills the tree and builds the call's layout (NB is only carved
// with, its own refusal comes later)
int check_common(const char* who, int V, int J, int hand_dim, int n_pca, const int32_t* parents, Tree& tree, int N, int NB,
                 const void* shape_state, size_t shape_stride, Layout& L) {
  if (!sizes_ok(V, J)) return fail(COMA_E_INVALID, "%s: V=%d must lie in [1, %d] and J=%d in [1, %d]", who, V, kMaxV, J, kMaxJ);
  if (n_pca < 0 || n_pca > kMaxPca) return fail(COMA_E_INVALID, "%s: n_pca=%d outside [0, %d]", who, n_pca, kMaxPca);
  if (hand_dim < 0 || hand_dim % 3 != 0 || 2 * hand_dim > 3 * (J - 1))
    return fail(COMA_E_INVALID, "%s: hand_dim=%d must be a multiple of 3 with 2 hand_dim <= 3 (J - 1) = %d", who, hand_dim, 3 * (J - 1));
  for (int i = 0; i < kMaxJ; ++i) tree.parent[i] = 0;
  for (int i = 1; i < J; ++i) {
    if (parents[i] < 0 || parents[i] >= i) return fail(COMA_E_INVALID, "%s: parent %d of joint %d outside [0, %d)", who, parents[i], i, i);
    tree.parent[i] = parents[i];
  }
  if (N < 1 || N > kMaxBatch) return fail(COMA_E_INVALID, "%s: N=%d outside [1, %d]", who, N, kMaxBatch);
  L = layout(V, J, N, NB);
  if (shape_stride != 0 && (shape_stride < L.shape_total || (shape_stride & 15) != 0))
    return fail(COMA_E_INVALID, "%s: shape_stride=%zu must be 0 (one shape state for all bodies) or a multiple of 16 of at least %zu", who,
                shape_stride, L.shape_total);
  if (((uintptr_t)shape_state & 15) != 0) return fail(COMA_E_INVALID, "%s: shape state must be 16-byte aligned", who);
  return COMA_OK;
}

int extra_joints_impl(const char* who, int N, const float* vertices, const float* transl, const int32_t* vertex_index, const float* vertex_weight,
                      int V, int E, float* out, void* stream) {
  if (N < 1 || N > kMaxBatch) return fail(COMA_E_INVALID, "%s: N=%d outside [1, %d]", who, N, kMaxBatch);
  if (E == 0) return COMA_OK;
  if (!vertices || !vertex_index || !vertex_weight || !out) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (V < 1 || V > kMaxV || E < 0 || E > kMaxV) return fail(COMA_E_INVALID, "%s: bad sizes V=%d E=%d", who, V, E);
  hipLaunchKernelGGL(smplx_gather_kernel, dim3((3 * E + kBlock - 1) / kBlock, N), dim3(kBlock), 0, (hipStream_t)stream, vertices, transl,
                     vertex_index, vertex_weight, V, E, out);
  return check_launch(who);
}

// the skinning backward on the caller's f32 gradient or on the f64 effective one
template <typename TG>
void launch_skin_bwd(const SmplxBackwardPlan& p, const TG* grad, hipStream_t s) {
  SkinBwdArgs<TG> sb = {};
  sb.weights = p.weights; sb.A = p.s_A; sb.v_posed = p.s_vposed; sb.grad = grad;
  sb.V = p.V; sb.J = p.pose.J; sb.gvp = p.gvp; sb.dA_part = p.dA_part;
  const auto skin_bwd = p.g.B == 1 ? smplx_skin_bwd_kernel<TG, 1> : smplx_skin_bwd_kernel<TG, kSkinChunk>;
  hipLaunchKernelGGL(skin_bwd, dim3(p.g.nblk, p.g.skin_chunks), dim3(kTile), 0, s, sb, p.strides);
}

}  // namespace

int smplx_forward_plan(const char* who, bool batched, int N, size_t shape_stride, const float* theta, const float* transl, const float* posedirs,
                       const float* weights, const int32_t* parents, const float* hand_components, const float* pose_mean, int V, int J,
                       int hand_dim, int n_pca, const void* shape_state, float* vertices, float* joints, float* full_pose, void* saved,
                       size_t saved_bytes, void* workspace, size_t workspace_bytes, SmplxForwardPlan& p) {
  if (!theta || !posedirs || !weights || !parents || !shape_state || !vertices || !joints || !saved || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  p = {};
  PoseArgs& pa = p.pose;
  Layout L;
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pa.tree, N, 0, shape_state, shape_stride, L)) return rc;
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, N * L.saved_stride)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, batched ? L.fwd_total : L.single_total())) return rc;
  const char* st = (const char*)shape_state;
  char* sv = (char*)saved;
  char* ws = (char*)workspace;
  p.who = who; p.g = L; p.posedirs = posedirs; p.part = (double*)(ws + L.part);
  p.strides = {N, n_pca > 0 ? 3 * J - 2 * hand_dim + 2 * n_pca : 3 * J, shape_stride, L.saved_stride};
  pa.theta = theta; pa.comps = hand_components; pa.mean = pose_mean; pa.transl = transl; pa.j_rest = (const double*)(st + L.j_rest);
  pa.J = J; pa.hd = hand_dim; pa.n_pca = n_pca; pa.s_pose = (double*)(sv + L.s_pose); pa.s_A = (double*)(sv + L.s_A);
  pa.feat = (double*)(ws + L.feat); pa.joints = joints; pa.full_pose = full_pose;
  SkinArgs& sa = p.skin;
  sa.weights = weights; sa.A = pa.s_A; sa.v_shaped = (const double*)(st + L.v_shaped); sa.part = p.part; sa.transl = transl;
  sa.V = V; sa.J = J; sa.v_posed = (double*)(sv + L.s_vposed); sa.vertices = vertices;
  return COMA_OK;
}

int smplx_forward_enqueue(const SmplxForwardPlan& p, hipStream_t s) {
  const SmplxGrids& L = p.g;
  const int N = p.strides.N;
  hipLaunchKernelGGL(smplx_pose_kernel, dim3(N), dim3(kBlock), 0, s, p.pose, p.strides);
  const auto offsets = L.C == 1 ? smplx_offsets_kernel<1> : smplx_offsets_kernel<kChunk>;       // one body: no sums for absent ones
  hipLaunchKernelGGL(offsets, dim3(L.nb3, kPSplit, L.chunks), dim3(kBlock), 0, s, p.posedirs, (const double*)p.pose.feat, L.P, 3 * p.skin.V, L.rows, N,
                     p.part);
  const auto skin = L.B == 1 ? smplx_skin_kernel<1> : smplx_skin_kernel<kSkinChunk>;
  hipLaunchKernelGGL(skin, dim3(L.nblk, L.skin_chunks), dim3(kTile), 0, s, p.skin, p.strides);
  return check_launch(p.who);
}

int smplx_backward_plan(const char* who, bool batched, int N, size_t shape_stride, const float* grad_vertices, const float* posedirs,
                        const float* weights, const int32_t* parents, const float* hand_components, int V, int J, int hand_dim, int n_pca,
                        const void* shape_state, const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace,
                        size_t workspace_bytes, const FullBwd* full, SmplxBackwardPlan& p) {
  if ((!full && !grad_vertices) || !posedirs || !weights || !parents || !shape_state || !saved || !grad_theta || !grad_transl || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  p = {};
  PoseBwdArgs& pb = p.pose;
  Layout L;
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pb.tree, N, full ? full->NB : 0, shape_state, shape_stride, L)) return rc;
  bool scatter = false, want_coef = false;
  if (full) {
    if (full->E < 0 || full->E > kMaxE) return fail(COMA_E_INVALID, "%s: E=%d outside [0, %d]", who, full->E, kMaxE);
    scatter = full->grad_joints && full->E > 0;
    if (scatter && (!full->extra_index || !full->extra_weight))
      return fail(COMA_E_INVALID, "%s: null pointer (the extra-joint tables with grad_joints and E > 0)", who);
    want_coef = full->grad_coefficients != nullptr;
    if (full->NB < (want_coef ? 1 : 0) || full->NB > kMaxNB) return fail(COMA_E_INVALID, "%s: NB=%d outside [%d, %d]", who, full->NB, want_coef ? 1 : 0, kMaxNB);
    if (want_coef && !full->shapedirs) return fail(COMA_E_INVALID, "%s: null pointer (shapedirs with grad_coefficients)", who);
    if (want_coef && !full->J_regressor) return fail(COMA_E_INVALID, "%s: null pointer (J_regressor with grad_coefficients)", who);
  }
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, N * L.saved_stride)) return rc;
  const size_t need = !full ? L.single_total() : batched ? L.batch_grad_total() : L.grad_total;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, need)) return rc;
  const char* st = (const char*)shape_state;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace + (full ? 0 : L.fwd_total);
  p.who = who; p.g = L; p.V = V; p.posedirs = posedirs; p.weights = weights;
  p.strides = {N, n_pca > 0 ? 3 * J - 2 * hand_dim + 2 * n_pca : 3 * J, shape_stride, L.saved_stride};
  p.s_A = (const double*)(sv + L.s_A); p.s_vposed = (const double*)(sv + L.s_vposed); p.grad_vertices = grad_vertices;
  p.gvp = (double*)(ws + L.gvp); p.dA_part = (double*)(ws + L.dA_part); p.dfeat = (double*)(ws + L.dfeat);
  if (scatter || !grad_vertices) {                          // only then does the gradient at the vertices differ from the caller's
    p.g_eff = (double*)(ws + L.g_eff);
    p.gJ_extra = scatter ? full->grad_joints + 3 * (size_t)J : nullptr; p.gJ_stride = 3 * (size_t)(J + full->E);
    p.extra_index = full->extra_index; p.extra_weight = full->extra_weight; p.E = scatter ? full->E : 0;
  }
  pb.s_pose = (const double*)(sv + L.s_pose); pb.j_rest = (const double*)(st + L.j_rest); pb.comps = hand_components;
  pb.dA_part = p.dA_part; pb.dfeat = p.dfeat; pb.J = J; pb.hd = hand_dim; pb.n_pca = n_pca; pb.nblk = L.nblk;
  pb.grad_theta = grad_theta; pb.grad_transl = grad_transl;
  if (full) {
    pb.gJ = full->grad_joints; pb.gP = full->grad_full_pose; pb.extra_w = full->extra_weight; pb.E = scatter ? full->E : 0;
    pb.dJ_out = want_coef ? (double*)(ws + L.dJ) : nullptr;
  }
  if (want_coef) {
    p.shapedirs = full->shapedirs; p.J_regressor = full->J_regressor; p.NB = full->NB;
    p.coef_part = (double*)(ws + L.coef_part); p.grad_coefficients = full->grad_coefficients;
  }
  return COMA_OK;
}

int smplx_backward_enqueue(const SmplxBackwardPlan& p, hipStream_t s) {
  const SmplxGrids& L = p.g;
  const int N = p.strides.N, V = p.V, J = p.pose.J;
  if (p.g_eff) {
    hipLaunchKernelGGL(smplx_effective_grad_kernel, dim3((V + kBlock - 1) / kBlock, N), dim3(kBlock), 0, s, p.grad_vertices, p.gJ_extra, p.gJ_stride,
                       p.extra_index, p.extra_weight, V, p.E, p.g_eff);
    launch_skin_bwd<double>(p, p.g_eff, s);
  } else {
    launch_skin_bwd<float>(p, p.grad_vertices, s);
  }
  const auto feature_bwd = L.C == 1 ? smplx_feature_bwd_kernel<1> : smplx_feature_bwd_kernel<kChunk>;
  if (L.P > 0) hipLaunchKernelGGL(feature_bwd, dim3(L.P, L.chunks), dim3(kBlock), 0, s, p.posedirs, (const double*)p.gvp, 3 * V, L.P, N, p.dfeat);
  hipLaunchKernelGGL(smplx_pose_bwd_kernel, dim3(N), dim3(kBlock), 0, s, p.pose, p.strides);
  if (p.grad_coefficients) {
    hipLaunchKernelGGL(smplx_shape_bwd_kernel, dim3(L.nb3), dim3(kBlock), 0, s, p.shapedirs, p.J_regressor, (const double*)p.gvp,
                       (const double*)p.pose.dJ_out, V, J, p.NB, p.coef_part);
    hipLaunchKernelGGL(smplx_coef_sum_kernel, dim3((p.NB + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double*)p.coef_part, L.nb3, p.NB,
                       p.grad_coefficients);
  }
  return check_launch(p.who);
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_smplx_workspace_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).single_total() : 0; }
extern "C" size_t coma_smplx_shape_state_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).shape_total : 0; }
extern "C" size_t coma_smplx_saved_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).saved_stride : 0; }
extern "C" size_t coma_smplx_grad_workspace_bytes(int V, int J, int NB) {
  return sizes_ok(V, J) && NB >= 0 && NB <= kMaxNB ? layout(V, J, 1, NB).grad_total : 0;
}
extern "C" size_t coma_smplx_batch_workspace_bytes(int V, int J, int N) { return sizes_ok(V, J, N) ? layout(V, J, N).fwd_total : 0; }
extern "C" size_t coma_smplx_batch_saved_bytes(int V, int J, int N) { return sizes_ok(V, J, N) ? N * layout(V, J, N).saved_stride : 0; }
extern "C" size_t coma_smplx_batch_grad_workspace_bytes(int V, int J, int N) { return sizes_ok(V, J, N) ? layout(V, J, N).batch_grad_total() : 0; }

extern "C" int coma_smplx_shape_f32(const float* v_template, const float* shapedirs, const float* coefficients, const float* J_regressor, int V,
                                    int J, int NB, void* shape_state, size_t shape_state_bytes, void* stream) {
  const char* who = "coma_smplx_shape_f32";
  if (!v_template || !shapedirs || !coefficients || !J_regressor || !shape_state) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!sizes_ok(V, J)) return fail(COMA_E_INVALID, "%s: V=%d must lie in [1, %d] and J=%d in [1, %d]", who, V, kMaxV, J, kMaxJ);
  if (NB < 1 || NB > kMaxNB) return fail(COMA_E_INVALID, "%s: NB=%d outside [1, %d]", who, NB, kMaxNB);
  const Layout L = layout(V, J);
  if (int rc = check_buffer(who, "shape state", shape_state, shape_state_bytes, L.shape_total)) return rc;
  char* st = (char*)shape_state;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(smplx_shape_kernel, dim3(L.nb3), dim3(kBlock), 0, s, v_template, shapedirs, coefficients, 3 * V, NB, (double*)(st + L.v_shaped));
  hipLaunchKernelGGL(smplx_jrest_kernel, dim3(J), dim3(kBlock), 0, s, J_regressor, (const double*)(st + L.v_shaped), V, (double*)(st + L.j_rest));
  return check_launch(who);
}

extern "C" int coma_smplx_forward_f32(const float* theta, const float* transl, const float* posedirs, const float* weights, const int32_t* parents,
                                      const float* hand_components, const float* pose_mean, int V, int J, int hand_dim, int n_pca,
                                      const void* shape_state, float* vertices, float* joints, float* full_pose, void* saved, size_t saved_bytes,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  SmplxForwardPlan p;
  if (int rc = smplx_forward_plan("coma_smplx_forward_f32", false, 1, 0, theta, transl, posedirs, weights, parents, hand_components, pose_mean, V, J,
                                  hand_dim, n_pca, shape_state, vertices, joints, full_pose, saved, saved_bytes, workspace, workspace_bytes, p))
    return rc;
  return smplx_forward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_smplx_forward_batch_f32(const float* theta, const float* transl, const float* posedirs, const float* weights,
                                            const int32_t* parents, const float* hand_components, const float* pose_mean, int V, int J,
                                            int hand_dim, int n_pca, int N, const void* shape_state, size_t shape_stride, float* vertices,
                                            float* joints, float* full_pose, void* saved, size_t saved_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  SmplxForwardPlan p;
  if (int rc = smplx_forward_plan("coma_smplx_forward_batch_f32", true, N, shape_stride, theta, transl, posedirs, weights, parents, hand_components,
                                  pose_mean, V, J, hand_dim, n_pca, shape_state, vertices, joints, full_pose, saved, saved_bytes, workspace,
                                  workspace_bytes, p))
    return rc;
  return smplx_forward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_smplx_backward_f32(const float* grad_vertices, const float* posedirs, const float* weights, const int32_t* parents,
                                       const float* hand_components, int V, int J, int hand_dim, int n_pca, const void* shape_state,
                                       const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  SmplxBackwardPlan p;
  if (int rc = smplx_backward_plan("coma_smplx_backward_f32", false, 1, 0, grad_vertices, posedirs, weights, parents, hand_components, V, J, hand_dim,
                                   n_pca, shape_state, saved, saved_bytes, grad_theta, grad_transl, workspace, workspace_bytes, nullptr, p))
    return rc;
  return smplx_backward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_smplx_backward_full_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose,
                                            const float* posedirs, const float* weights, const int32_t* parents, const float* hand_components,
                                            const int32_t* extra_index, const float* extra_weight, int E, const float* shapedirs,
                                            const float* J_regressor, int NB, int V, int J, int hand_dim, int n_pca, const void* shape_state,
                                            const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl,
                                            float* grad_coefficients, void* workspace, size_t workspace_bytes, void* stream) {
  const FullBwd full = {grad_joints, grad_full_pose, extra_index, extra_weight, E, shapedirs, J_regressor, NB, grad_coefficients};
  SmplxBackwardPlan p;
  if (int rc = smplx_backward_plan("coma_smplx_backward_full_f32", false, 1, 0, grad_vertices, posedirs, weights, parents, hand_components, V, J,
                                   hand_dim, n_pca, shape_state, saved, saved_bytes, grad_theta, grad_transl, workspace, workspace_bytes, &full, p))
    return rc;
  return smplx_backward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_smplx_backward_batch_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose,
                                             const float* posedirs, const float* weights, const int32_t* parents, const float* hand_components,
                                             const int32_t* extra_index, const float* extra_weight, int E, int V, int J, int hand_dim, int n_pca,
                                             int N, const void* shape_state, size_t shape_stride, const void* saved, size_t saved_bytes,
                                             float* grad_theta, float* grad_transl, void* workspace, size_t workspace_bytes, void* stream) {
  const FullBwd full = {grad_joints, grad_full_pose, extra_index, extra_weight, E, nullptr, nullptr, 0, nullptr};
  SmplxBackwardPlan p;
  if (int rc = smplx_backward_plan("coma_smplx_backward_batch_f32", true, N, shape_stride, grad_vertices, posedirs, weights, parents, hand_components,
                                   V, J, hand_dim, n_pca, shape_state, saved, saved_bytes, grad_theta, grad_transl, workspace, workspace_bytes, &full,
                                   p))
    return rc;
  return smplx_backward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_smplx_extra_joints_f32(const float* vertices, const float* transl, const int32_t* vertex_index, const float* vertex_weight,
                                           int V, int E, float* out, void* stream) {
  return extra_joints_impl("coma_smplx_extra_joints_f32", 1, vertices, transl, vertex_index, vertex_weight, V, E, out, stream);
}

extern "C" int coma_smplx_extra_joints_batch_f32(const float* vertices, const float* transl, const int32_t* vertex_index,
                                                 const float* vertex_weight, int V, int E, int N, float* out, void* stream) {
  return extra_joints_impl("coma_smplx_extra_joints_batch_f32", N, vertices, transl, vertex_index, vertex_weight, V, E, out, stream);
}

