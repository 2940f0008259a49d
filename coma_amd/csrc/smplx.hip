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
// The BATCHED forms (coma_smplx_*_batch_f32: N bodies in the launches of one) share the arithmetic of every stage with the
// single-body kernels as device functions, so body n of a batch has the bits of the single-body call.  What changes is how often
// the operands move: a sweep over posedirs serves kChunk bodies (their features in LDS, one f64 sum per body in registers), a
// skinning workgroup stages its weights tile once and walks kSkinChunk bodies over it, the pose stage runs one workgroup per body.
#include "common.h"
#include "coma_device.h"

#include <cmath>

namespace coma {
namespace {

constexpr int kMaxJ = 64;         // joints (the chain kernels keep the whole tree in LDS)
constexpr int kBlock = 256;
constexpr int kTile = 128;        // vertices (and threads) per skinning workgroup: weights tile 128 x 64 f32 = 32 KB of LDS
constexpr int kPSplit = 8;        // splits of the P rows of posedirs in the forward
constexpr int kMaxRows = (9 * (kMaxJ - 1) + kPSplit - 1) / kPSplit;
constexpr int kMaxPca = 64;
// the batched forms (coma_smplx_*_batch_f32)
constexpr int kMaxBatch = 1024;
constexpr int kChunk = 8;         // C: bodies served by one sweep over posedirs (16 VGPRs of f64 sums per thread; forward LDS 71 x 8 f64)
constexpr int kSkinChunk = 2;     // bodies one skinning workgroup walks over its staged weights tile

struct Tree { int32_t parent[kMaxJ]; };

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

struct PoseArgs {
  const float* theta;
  const float* comps;     // [2, n_pca, hd]
  const float* mean;      // [3J] or null
  const float* transl;    // [3] or null
  const double* j_rest;
  int J, hd, n_pca;
  Tree tree;
  double* s_pose;         // saved [3J]
  double* s_A;            // saved [J,12]
  double* feat;           // workspace [9 (J - 1)]
  float* joints;          // [J,3]
  float* full_pose;       // [3J] or null
};

// what differs from body to body of a batch; the single-body kernel passes PoseArgs' own pointers
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

__global__ __launch_bounds__(kBlock) void smplx_pose_kernel(PoseArgs a) {
  pose_forward(a, PoseBody{a.theta, a.transl, a.j_rest, a.s_pose, a.s_A, a.feat, a.joints, a.full_pose});
}

// How a batched call finds body n: the f32 arrays are dense [N, ...]; the shape states and saved blocks are `stride` bytes apart.
struct BatchStrides {
  int N, NT;
  size_t shape, saved;      // bytes; shape = 0: one shape state for all bodies
};

template <typename T>
__device__ __forceinline__ T* at_bytes(T* p, size_t bytes) {
  return (T*)((char*)p + bytes);
}
template <typename T>
__device__ __forceinline__ const T* at_bytes(const T* p, size_t bytes) {
  return (const T*)((const char*)p + bytes);
}

// one workgroup per body; PoseArgs holds body 0's pointers
__global__ __launch_bounds__(kBlock) void smplx_pose_batch_kernel(PoseArgs a, BatchStrides st) {
  const size_t n = blockIdx.x;
  const int J = a.J;
  pose_forward(a, PoseBody{a.theta + n * st.NT, a.transl ? a.transl + 3 * n : nullptr, at_bytes(a.j_rest, n * st.shape), at_bytes(a.s_pose, n * st.saved),
                           at_bytes(a.s_A, n * st.saved), a.feat + n * (size_t)(9 * (J - 1)), a.joints + n * (size_t)(3 * J),
                           a.full_pose ? a.full_pose + n * (size_t)(3 * J) : nullptr});
}

// ---- skinning stage ----
// partial pose offsets: part[s][i] = sum over the rows p of split s (ascending) of feat[p] posedirs[p][i]
__global__ __launch_bounds__(kBlock) void smplx_offsets_kernel(const float* __restrict__ posedirs, const double* __restrict__ feat, int P, int n3,
                                                              int rows, double* __restrict__ part) {
  __shared__ double f[kMaxRows];
  const int s = blockIdx.y;
  const int p0 = s * rows, p1 = min(P, p0 + rows);
  for (int p = p0 + threadIdx.x; p < p1; p += kBlock) f[p - p0] = feat[p];
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n3) return;
  double acc = 0.0;
  const float* col = posedirs + i;
#pragma unroll 8
  for (int p = p0; p < p1; ++p) acc = acc + f[p - p0] * (double)col[(int64_t)p * n3];
  part[(int64_t)s * n3 + i] = acc;
}

// The batched form: grid (column blocks, kPSplit, chunks of kChunk bodies).  The chunk's features of this split sit in LDS as
// [row][body]; every posedirs element is loaded once and used for all bodies of the chunk, each body's sum in a register of its own
// and in the single-body kernel's order.  part is [N][kPSplit][3V].  With P = 0 it writes the zeros the single-body call memsets.
__global__ __launch_bounds__(kBlock) void smplx_offsets_batch_kernel(const float* __restrict__ posedirs, const double* __restrict__ feat, int P,
                                                                    int n3, int rows, int N, double* __restrict__ part) {
  __shared__ double f[kMaxRows * kChunk];
  const int s = blockIdx.y, n0 = blockIdx.z * kChunk, nc = min(kChunk, N - n0);
  const int p0 = s * rows, p1 = min(P, p0 + rows);
  for (int q = threadIdx.x; q < (p1 - p0) * kChunk; q += kBlock) {
    const int r = q / kChunk, c = q % kChunk;
    f[q] = c < nc ? feat[(int64_t)(n0 + c) * P + p0 + r] : 0.0;
  }
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n3) return;
  double acc[kChunk];
#pragma unroll
  for (int c = 0; c < kChunk; ++c) acc[c] = 0.0;
  const float* col = posedirs + i;
#pragma unroll 4
  for (int p = p0; p < p1; ++p) {
    const double x = (double)col[(int64_t)p * n3];
    const double* fp = f + (p - p0) * kChunk;
#pragma unroll
    for (int c = 0; c < kChunk; ++c) acc[c] = acc[c] + fp[c] * x;
  }
#pragma unroll
  for (int c = 0; c < kChunk; ++c)
    if (c < nc) part[((int64_t)(n0 + c) * kPSplit + s) * n3 + i] = acc[c];
}

struct SkinArgs {
  const float* weights;     // [V,J]
  const double* A;          // [J,12]
  const double* v_shaped;   // [V,3]
  const double* part;       // [kPSplit][3V]
  const float* transl;      // [3] or null
  int V, J;
  double* v_posed;          // saved [V,3]
  float* vertices;          // [V,3]
};

// the weights of a tile of vertices (one contiguous run of the [V,J] table) and the J transforms into LDS
__device__ __forceinline__ int stage_tile(const float* __restrict__ weights, const double* __restrict__ A, int V, int J, float* Wt, double* Al) {
  const int v0 = blockIdx.x * kTile, n = min(kTile, V - v0);
  const float* src = weights + (int64_t)v0 * J;
  for (int q = threadIdx.x; q < n * J; q += kTile) Wt[q] = src[q];
  for (int q = threadIdx.x; q < 12 * J; q += kTile) Al[q] = A[q];
  __syncthreads();
  return n;
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

__global__ __launch_bounds__(kTile) void smplx_skin_kernel(SkinArgs a) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  const int n = stage_tile(a.weights, a.A, a.V, a.J, Wt, Al);
  const int t = threadIdx.x;
  if (t >= n) return;
  skin_vertex(Wt, Al, a.V, a.J, (int64_t)blockIdx.x * kTile + t, t, a.part, a.v_shaped, a.transl, a.v_posed, a.vertices);
}

// the weights of this workgroup's tile of vertices into LDS (no barrier: the first stage_A gives it) -> the vertices in the tile
__device__ __forceinline__ int stage_weights(const float* __restrict__ weights, int V, int J, float* Wt) {
  const int v0 = blockIdx.x * kTile, n = min(kTile, V - v0);
  const float* src = weights + (int64_t)v0 * J;
  for (int q = threadIdx.x; q < n * J; q += kTile) Wt[q] = src[q];
  return n;
}

// the next body's transforms into LDS, once every thread is done with the previous body's
__device__ __forceinline__ void stage_A(const double* __restrict__ A, int J, double* Al) {
  __syncthreads();
  for (int q = threadIdx.x; q < 12 * J; q += kTile) Al[q] = A[q];
  __syncthreads();
}

// The batched form: grid (tiles, chunks of kSkinChunk bodies); SkinArgs holds body 0's pointers, part is [N][kPSplit][3V].  The
// weights tile is staged once and the chunk's bodies walk over it.
__global__ __launch_bounds__(kTile) void smplx_skin_batch_kernel(SkinArgs a, BatchStrides st) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  const int n = stage_weights(a.weights, a.V, a.J, Wt);
  const int t = threadIdx.x, b0 = blockIdx.y * kSkinChunk, b1 = min(st.N, b0 + kSkinChunk);
  const size_t n3 = 3 * (size_t)a.V;
  for (size_t b = b0; b < (size_t)b1; ++b) {
    stage_A(at_bytes(a.A, b * st.saved), a.J, Al);
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
    const double g[3] = {load(grad, 3 * v), load(grad, 3 * v + 1), load(grad, 3 * v + 2)};
    double T[12];
    blend(Wt + t * J, Al, J, T);
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
      for (int u = 0; u < n; ++u) acc = acc + ((double)Wt[u * J + j] * gl[3 * u + r]) * vl[4 * u + c];
    } else {
      const int r = q - 12 * J;
      for (int u = 0; u < n; ++u) acc = acc + gl[3 * u + r];
    }
    out[q] = acc;
  }
}

template <typename TG>
__global__ __launch_bounds__(kTile) void smplx_skin_bwd_kernel(SkinBwdArgs<TG> a) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  __shared__ double gl[3 * kTile], vl[4 * kTile];
  const int n = stage_tile(a.weights, a.A, a.V, a.J, Wt, Al);
  skin_bwd_tile(Wt, Al, gl, vl, n, a.J, a.grad, a.v_posed, a.gvp, a.dA_part);
}

// The batched form: grid (tiles, chunks of kSkinChunk bodies); the args hold body 0's pointers, grad and gvp are [N][3V], dA_part is
// [N][tiles][12 J + 3].  stage_A's first barrier also keeps a body's gl / vl until every thread has summed over them.
template <typename TG>
__global__ __launch_bounds__(kTile) void smplx_skin_bwd_batch_kernel(SkinBwdArgs<TG> a, BatchStrides st) {
  __shared__ float Wt[kTile * kMaxJ];
  __shared__ double Al[12 * kMaxJ];
  __shared__ double gl[3 * kTile], vl[4 * kTile];
  const int n = stage_weights(a.weights, a.V, a.J, Wt);
  const int b0 = blockIdx.y * kSkinChunk, b1 = min(st.N, b0 + kSkinChunk);
  const size_t n3 = 3 * (size_t)a.V, per_body = (size_t)gridDim.x * (12 * a.J + 3);
  for (size_t b = b0; b < (size_t)b1; ++b) {
    stage_A(at_bytes(a.A, b * st.saved), a.J, Al);
    skin_bwd_tile(Wt, Al, gl, vl, n, a.J, a.grad + b * n3, at_bytes(a.v_posed, b * st.saved), a.gvp + b * n3, a.dA_part + b * per_body);
  }
}

// dL/dfeature_p = <posedirs[p, :], gvp>: one workgroup per row
__global__ __launch_bounds__(kBlock) void smplx_feature_bwd_kernel(const float* __restrict__ posedirs, const double* __restrict__ gvp, int n3,
                                                                  double* __restrict__ dfeat) {
  __shared__ double lds[kBlock];
  const float* row = posedirs + (int64_t)blockIdx.x * n3;
  double acc = 0.0;
#pragma unroll 4
  for (int i = threadIdx.x; i < n3; i += kBlock) acc = acc + (double)row[i] * gvp[i];
  const double s = block_sum<kBlock>(acc, lds);
  if (threadIdx.x == 0) dfeat[blockIdx.x] = s;
}

// The batched form: grid (P rows, chunks of kChunk bodies); one read of the row serves the chunk's dot products, each with the
// single-body kernel's 256 strided partial sums and tree.  gvp is [N][3V], dfeat [N][P].
__global__ __launch_bounds__(kBlock) void smplx_feature_bwd_batch_kernel(const float* __restrict__ posedirs, const double* __restrict__ gvp, int n3,
                                                                        int P, int N, double* __restrict__ dfeat) {
  __shared__ double lds[kBlock];
  const int n0 = blockIdx.y * kChunk, nc = min(kChunk, N - n0);
  const float* row = posedirs + (int64_t)blockIdx.x * n3;
  const double* g0 = gvp + (int64_t)n0 * n3;
  double acc[kChunk];
#pragma unroll
  for (int c = 0; c < kChunk; ++c) acc[c] = 0.0;
#pragma unroll 2
  for (int i = threadIdx.x; i < n3; i += kBlock) {
    const double x = (double)row[i];
#pragma unroll
    for (int c = 0; c < kChunk; ++c)
      if (c < nc) acc[c] = acc[c] + x * g0[(int64_t)c * n3 + i];
  }
#pragma unroll
  for (int c = 0; c < kChunk; ++c)
    if (c < nc) {                                           // nc is the workgroup's: every thread reaches the same barriers
      const double s = block_sum<kBlock>(acc[c], lds);
      if (threadIdx.x == 0) dfeat[(int64_t)(n0 + c) * P + blockIdx.x] = s;
    }
}

struct PoseBwdArgs {
  const double* s_pose;
  const double* j_rest;
  const float* comps;
  const double* dA_part;
  const double* dfeat;
  int J, hd, n_pca, nblk;
  Tree tree;
  float* grad_theta;
  float* grad_transl;
  // the full backward's additions; each pointer may be null and then changes nothing
  const float* gJ;          // dL/djoints [J + E, 3]
  const float* gP;          // dL/dfull_pose [3J]
  const float* extra_w;     // [E,3]: the extra joints' weights, for the direct transl term (read only with gJ)
  int E;
  double* dJ_out;           // dL/dJ_rest [J,3]
};

// what differs from body to body of a batch; the single-body kernel passes PoseBwdArgs' own pointers
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

__global__ __launch_bounds__(kBlock) void smplx_pose_bwd_kernel(PoseBwdArgs a) {
  pose_backward(a, PoseBwdBody{a.s_pose, a.j_rest, a.dA_part, a.dfeat, a.grad_theta, a.grad_transl, a.gJ, a.gP, a.dJ_out});
}

// one workgroup per body; PoseBwdArgs holds body 0's pointers, gJ is [N][J + E, 3]; no gradient to the rest joints
__global__ __launch_bounds__(kBlock) void smplx_pose_bwd_batch_kernel(PoseBwdArgs a, BatchStrides st) {
  const size_t n = blockIdx.x;
  const int J = a.J;
  pose_backward(a, PoseBwdBody{at_bytes(a.s_pose, n * st.saved), at_bytes(a.j_rest, n * st.shape), a.dA_part + n * a.nblk * (size_t)(12 * J + 3),
                               a.dfeat + n * (size_t)(9 * (J - 1)), a.grad_theta + n * st.NT, a.grad_transl + 3 * n,
                               a.gJ ? a.gJ + n * (size_t)(3 * (J + a.E)) : nullptr, a.gP ? a.gP + n * (size_t)(3 * J) : nullptr, nullptr});
}

// ---- extra joints ----
__device__ __forceinline__ void gather_extra(const float* __restrict__ vertices, const float* __restrict__ transl, const int32_t* __restrict__ idx,
                                             const float* __restrict__ w, int V, int E, float* __restrict__ out) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= 3 * E) return;
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

__global__ __launch_bounds__(kBlock) void smplx_gather_kernel(const float* __restrict__ vertices, const float* __restrict__ transl,
                                                             const int32_t* __restrict__ idx, const float* __restrict__ w, int V, int E,
                                                             float* __restrict__ out) {
  gather_extra(vertices, transl, idx, w, V, E, out);
}

// grid (blocks of 3E, N): vertices [N][V,3], transl [N][3] or null, out [N][E,3]; one table for all bodies
__global__ __launch_bounds__(kBlock) void smplx_gather_batch_kernel(const float* __restrict__ vertices, const float* __restrict__ transl,
                                                                   const int32_t* __restrict__ idx, const float* __restrict__ w, int V, int E,
                                                                   float* __restrict__ out) {
  const size_t n = blockIdx.y;
  gather_extra(vertices + n * 3 * (size_t)V, transl ? transl + 3 * n : nullptr, idx, w, V, E, out + n * 3 * (size_t)E);
}

// ---- the full backward's own passes ----
constexpr int kMaxE = 4096;       // extra joints whose gradient is scattered back
constexpr int kEffChunk = 768;    // table entries in LDS per pass

// The effective vertex gradient: g_eff[v] = g[v] (zeros without g) + the sum over the table entries (e, i) with index v, in ascending
// (e, i), of w[e,i] gJ_extra[e].  Written as a gather -- every vertex scans the whole table from LDS -- so repeated indices (a vertex
// pick is (i, i, i), landmark faces share vertices) add in the table's order without atomics; an index outside [0, V) matches nothing.
__device__ __forceinline__ void effective_grad(const float* __restrict__ g, const float* __restrict__ gJ_extra, const int32_t* __restrict__ idx,
                                               const float* __restrict__ w, int V, int E, double* __restrict__ g_eff) {
  __shared__ int32_t li[kEffChunk];
  __shared__ double lw[3 * kEffChunk];
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

__global__ __launch_bounds__(kBlock) void smplx_effective_grad_kernel(const float* __restrict__ g, const float* __restrict__ gJ_extra,
                                                                     const int32_t* __restrict__ idx, const float* __restrict__ w, int V, int E,
                                                                     double* __restrict__ g_eff) {
  effective_grad(g, gJ_extra, idx, w, V, E, g_eff);
}

// grid (blocks of V, N): g [N][V,3] or null, gJ [N][J + E, 3] or null (the extra joints' rows are read), g_eff [N][V,3]
__global__ __launch_bounds__(kBlock) void smplx_effective_grad_batch_kernel(const float* __restrict__ g, const float* __restrict__ gJ, int J,
                                                                           const int32_t* __restrict__ idx, const float* __restrict__ w, int V,
                                                                           int E, int E_all, double* __restrict__ g_eff) {
  const size_t n = blockIdx.y, n3 = 3 * (size_t)V;
  effective_grad(g ? g + n * n3 : nullptr, gJ ? gJ + n * 3 * (size_t)(J + E_all) + 3 * (size_t)J : nullptr, idx, w, V, E, g_eff + n * n3);
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

struct Layout {
  size_t feat, part, gvp, dA_part, dfeat, total;      // workspace
  size_t v_shaped, j_rest, shape_total;               // shape state
  size_t s_pose, s_A, s_vposed, saved_total;          // saved by a forward for its backward
  int P, rows, nblk, nb3;
};

Layout layout(int V, int J) {
  Layout L = {};
  const size_t n3 = (size_t)3 * V, d = sizeof(double);
  L.P = 9 * (J - 1);
  L.rows = (L.P + kPSplit - 1) / kPSplit;
  L.nblk = (V + kTile - 1) / kTile;
  L.nb3 = (int)((n3 + kBlock - 1) / kBlock);
  Carve ws, shape, saved;
  L.feat = ws.take((size_t)(L.P > 0 ? L.P : 1) * d);
  L.part = ws.take((size_t)kPSplit * n3 * d);
  L.gvp = ws.take(n3 * d);
  L.dA_part = ws.take((size_t)L.nblk * (12 * J + 3) * d);
  L.dfeat = ws.take((size_t)(L.P > 0 ? L.P : 1) * d);
  L.total = ws.at;
  L.v_shaped = shape.take(n3 * d);
  L.j_rest = shape.take((size_t)3 * J * d);
  L.shape_total = shape.at;
  L.s_pose = saved.take((size_t)3 * J * d);
  L.s_A = saved.take((size_t)12 * J * d);
  L.s_vposed = saved.take(n3 * d);
  L.saved_total = saved.at;
  return L;
}

constexpr int kMaxV = 1 << 24;
constexpr int kMaxNB = 1024;

bool sizes_ok(int V, int J) { return V >= 1 && V <= kMaxV && J >= 1 && J <= kMaxJ; }

// the full backward's workspace: what the backward needs of the one above (at offsets of its own), then its additions
struct GradLayout {
  size_t gvp, dA_part, dfeat, g_eff, dJ, coef_part, total;
};

GradLayout grad_layout(int V, int J, int NB) {
  const Layout L = layout(V, J);
  GradLayout G = {};
  const size_t n3 = (size_t)3 * V, d = sizeof(double);
  Carve ws;
  G.gvp = ws.take(n3 * d);
  G.dA_part = ws.take((size_t)L.nblk * (12 * J + 3) * d);
  G.dfeat = ws.take((size_t)(L.P > 0 ? L.P : 1) * d);
  G.g_eff = ws.take(n3 * d);
  G.dJ = ws.take((size_t)3 * J * d);
  G.coef_part = ws.take((size_t)L.nb3 * (NB > 0 ? NB : 1) * d);
  G.total = ws.at;
  return G;
}

int check_common(const char* who, int V, int J, int hand_dim, int n_pca, const int32_t* parents, Tree& tree) {
  if (!sizes_ok(V, J)) return fail(COMA_E_INVALID, "%s: V=%d must lie in [1, %d] and J=%d in [1, %d]", who, V, kMaxV, J, kMaxJ);
  if (n_pca < 0 || n_pca > kMaxPca) return fail(COMA_E_INVALID, "%s: n_pca=%d outside [0, %d]", who, n_pca, kMaxPca);
  if (hand_dim < 0 || hand_dim % 3 != 0 || 2 * hand_dim > 3 * (J - 1))
    return fail(COMA_E_INVALID, "%s: hand_dim=%d must be a multiple of 3 with 2 hand_dim <= 3 (J - 1) = %d", who, hand_dim, 3 * (J - 1));
  for (int i = 0; i < kMaxJ; ++i) tree.parent[i] = 0;
  for (int i = 1; i < J; ++i) {
    if (parents[i] < 0 || parents[i] >= i) return fail(COMA_E_INVALID, "%s: parent %d of joint %d outside [0, %d)", who, parents[i], i, i);
    tree.parent[i] = parents[i];
  }
  return COMA_OK;
}

}  // namespace
}  // namespace coma

using namespace coma;

extern "C" size_t coma_smplx_workspace_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).total : 0; }
extern "C" size_t coma_smplx_shape_state_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).shape_total : 0; }
extern "C" size_t coma_smplx_saved_bytes(int V, int J) { return sizes_ok(V, J) ? layout(V, J).saved_total : 0; }

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
  const char* who = "coma_smplx_forward_f32";
  if (!theta || !posedirs || !weights || !parents || !shape_state || !vertices || !joints || !saved || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  PoseArgs pa = {};
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pa.tree)) return rc;
  const Layout L = layout(V, J);
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, L.saved_total)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
  if (((uintptr_t)shape_state & 15) != 0) return fail(COMA_E_INVALID, "%s: shape state must be 16-byte aligned", who);
  const char* st = (const char*)shape_state;
  char* sv = (char*)saved;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  pa.theta = theta; pa.comps = hand_components; pa.mean = pose_mean; pa.transl = transl; pa.j_rest = (const double*)(st + L.j_rest);
  pa.J = J; pa.hd = hand_dim; pa.n_pca = n_pca; pa.s_pose = (double*)(sv + L.s_pose); pa.s_A = (double*)(sv + L.s_A);
  pa.feat = (double*)(ws + L.feat); pa.joints = joints; pa.full_pose = full_pose;
  hipLaunchKernelGGL(smplx_pose_kernel, dim3(1), dim3(kBlock), 0, s, pa);
  if (L.P > 0)
    hipLaunchKernelGGL(smplx_offsets_kernel, dim3(L.nb3, kPSplit), dim3(kBlock), 0, s, posedirs, (const double*)(ws + L.feat), L.P, 3 * V, L.rows,
                       (double*)(ws + L.part));
  else if (hipMemsetAsync(ws + L.part, 0, (size_t)kPSplit * 3 * V * sizeof(double), s) != hipSuccess)
    return fail(COMA_E_LAUNCH, "%s: memset failed", who);
  SkinArgs sa = {};
  sa.weights = weights; sa.A = pa.s_A; sa.v_shaped = (const double*)(st + L.v_shaped); sa.part = (const double*)(ws + L.part); sa.transl = transl;
  sa.V = V; sa.J = J; sa.v_posed = (double*)(sv + L.s_vposed); sa.vertices = vertices;
  hipLaunchKernelGGL(smplx_skin_kernel, dim3(L.nblk), dim3(kTile), 0, s, sa);
  return check_launch(who);
}

namespace coma {
namespace {

// what coma_smplx_backward_full_f32 adds to coma_smplx_backward_f32; every pointer may be null
struct FullBwd {
  const float* grad_joints;
  const float* grad_full_pose;
  const int32_t* extra_index;
  const float* extra_weight;
  int E;
  const float* shapedirs;
  const float* J_regressor;
  int NB;
  float* grad_coefficients;
};

// Both backward entry points: `full` null is the vertices-only backward on the forward's workspace layout (its launches and bits are
// those of the first release); otherwise the full backward on its own layout.
int backward_impl(const char* who, const float* grad_vertices, const float* posedirs, const float* weights, const int32_t* parents,
                  const float* hand_components, int V, int J, int hand_dim, int n_pca, const void* shape_state, const void* saved,
                  size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace, size_t workspace_bytes, void* stream,
                  const FullBwd* full) {
  if ((!full && !grad_vertices) || !posedirs || !weights || !parents || !shape_state || !saved || !grad_theta || !grad_transl || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  PoseBwdArgs pb = {};
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pb.tree)) return rc;
  const Layout L = layout(V, J);
  size_t o_gvp = L.gvp, o_dA = L.dA_part, o_dfeat = L.dfeat, need = L.total;
  GradLayout GL = {};
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
    GL = grad_layout(V, J, full->NB);
    o_gvp = GL.gvp; o_dA = GL.dA_part; o_dfeat = GL.dfeat; need = GL.total;
  }
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, L.saved_total)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, need)) return rc;
  if (((uintptr_t)shape_state & 15) != 0) return fail(COMA_E_INVALID, "%s: shape state must be 16-byte aligned", who);
  const char* st = (const char*)shape_state;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  double* gvp = (double*)(ws + o_gvp);
  double* dA_part = (double*)(ws + o_dA);
  if (scatter || !grad_vertices) {                          // only then does the gradient at the vertices differ from the caller's
    double* g_eff = (double*)(ws + GL.g_eff);
    const int E = scatter ? full->E : 0;
    hipLaunchKernelGGL(smplx_effective_grad_kernel, dim3((V + kBlock - 1) / kBlock), dim3(kBlock), 0, s, grad_vertices,
                       scatter ? full->grad_joints + 3 * (size_t)J : nullptr, full->extra_index, full->extra_weight, V, E, g_eff);
    SkinBwdArgs<double> sb = {};
    sb.weights = weights; sb.A = (const double*)(sv + L.s_A); sb.v_posed = (const double*)(sv + L.s_vposed); sb.grad = g_eff;
    sb.V = V; sb.J = J; sb.gvp = gvp; sb.dA_part = dA_part;
    hipLaunchKernelGGL(smplx_skin_bwd_kernel<double>, dim3(L.nblk), dim3(kTile), 0, s, sb);
  } else {
    SkinBwdArgs<float> sb = {};
    sb.weights = weights; sb.A = (const double*)(sv + L.s_A); sb.v_posed = (const double*)(sv + L.s_vposed); sb.grad = grad_vertices;
    sb.V = V; sb.J = J; sb.gvp = gvp; sb.dA_part = dA_part;
    hipLaunchKernelGGL(smplx_skin_bwd_kernel<float>, dim3(L.nblk), dim3(kTile), 0, s, sb);
  }
  if (L.P > 0)
    hipLaunchKernelGGL(smplx_feature_bwd_kernel, dim3(L.P), dim3(kBlock), 0, s, posedirs, (const double*)gvp, 3 * V, (double*)(ws + o_dfeat));
  pb.s_pose = (const double*)(sv + L.s_pose); pb.j_rest = (const double*)(st + L.j_rest); pb.comps = hand_components;
  pb.dA_part = dA_part; pb.dfeat = (const double*)(ws + o_dfeat); pb.J = J; pb.hd = hand_dim; pb.n_pca = n_pca; pb.nblk = L.nblk;
  pb.grad_theta = grad_theta; pb.grad_transl = grad_transl;
  if (full) {
    pb.gJ = full->grad_joints; pb.gP = full->grad_full_pose; pb.extra_w = full->extra_weight; pb.E = scatter ? full->E : 0;
    pb.dJ_out = want_coef ? (double*)(ws + GL.dJ) : nullptr;
  }
  hipLaunchKernelGGL(smplx_pose_bwd_kernel, dim3(1), dim3(kBlock), 0, s, pb);
  if (want_coef) {
    double* part = (double*)(ws + GL.coef_part);
    hipLaunchKernelGGL(smplx_shape_bwd_kernel, dim3(L.nb3), dim3(kBlock), 0, s, full->shapedirs, full->J_regressor, (const double*)gvp,
                       (const double*)(ws + GL.dJ), V, J, full->NB, part);
    hipLaunchKernelGGL(smplx_coef_sum_kernel, dim3((full->NB + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double*)part, L.nb3, full->NB,
                       full->grad_coefficients);
  }
  return check_launch(who);
}

}  // namespace
}  // namespace coma

extern "C" int coma_smplx_backward_f32(const float* grad_vertices, const float* posedirs, const float* weights, const int32_t* parents,
                                       const float* hand_components, int V, int J, int hand_dim, int n_pca, const void* shape_state,
                                       const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return backward_impl("coma_smplx_backward_f32", grad_vertices, posedirs, weights, parents, hand_components, V, J, hand_dim, n_pca, shape_state,
                       saved, saved_bytes, grad_theta, grad_transl, workspace, workspace_bytes, stream, nullptr);
}

extern "C" size_t coma_smplx_grad_workspace_bytes(int V, int J, int NB) {
  return sizes_ok(V, J) && NB >= 0 && NB <= kMaxNB ? grad_layout(V, J, NB).total : 0;
}

extern "C" int coma_smplx_backward_full_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose,
                                            const float* posedirs, const float* weights, const int32_t* parents, const float* hand_components,
                                            const int32_t* extra_index, const float* extra_weight, int E, const float* shapedirs,
                                            const float* J_regressor, int NB, int V, int J, int hand_dim, int n_pca, const void* shape_state,
                                            const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl,
                                            float* grad_coefficients, void* workspace, size_t workspace_bytes, void* stream) {
  const FullBwd full = {grad_joints, grad_full_pose, extra_index, extra_weight, E, shapedirs, J_regressor, NB, grad_coefficients};
  return backward_impl("coma_smplx_backward_full_f32", grad_vertices, posedirs, weights, parents, hand_components, V, J, hand_dim, n_pca,
                       shape_state, saved, saved_bytes, grad_theta, grad_transl, workspace, workspace_bytes, stream, &full);
}

extern "C" int coma_smplx_extra_joints_f32(const float* vertices, const float* transl, const int32_t* vertex_index, const float* vertex_weight,
                                           int V, int E, float* out, void* stream) {
  const char* who = "coma_smplx_extra_joints_f32";
  if (E == 0) return COMA_OK;
  if (!vertices || !vertex_index || !vertex_weight || !out) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (V < 1 || V > kMaxV || E < 0 || E > kMaxV) return fail(COMA_E_INVALID, "%s: bad sizes V=%d E=%d", who, V, E);
  hipLaunchKernelGGL(smplx_gather_kernel, dim3((3 * E + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, vertices, transl, vertex_index,
                     vertex_weight, V, E, out);
  return check_launch(who);
}

// ---- the batched entry points ----
namespace coma {
namespace {

// Body n's saved block is the single-body layout at n x saved_stride.  Forward workspace: feat [N][P], part [N][kPSplit][3V].
// Backward workspace (one layout for both forms): gvp [N][3V], dA_part [N][tiles][12 J + 3], dfeat [N][P], g_eff [N][3V].
struct BatchLayout {
  Layout one;
  size_t feat, part, total;
  size_t gvp, dA_part, dfeat, g_eff, grad_total;
  size_t saved_stride, saved_total;
  int NT, chunks, skin_chunks;
};

bool batch_ok(int V, int J, int N) { return sizes_ok(V, J) && N >= 1 && N <= kMaxBatch; }

BatchLayout batch_layout(int V, int J, int N) {
  BatchLayout B = {};
  B.one = layout(V, J);
  const size_t n3 = (size_t)3 * V, d = sizeof(double), n = (size_t)N, P = (size_t)(B.one.P > 0 ? B.one.P : 1);
  Carve ws, grad;
  B.feat = ws.take(n * P * d);
  B.part = ws.take(n * kPSplit * n3 * d);
  B.total = ws.at;
  B.gvp = grad.take(n * n3 * d);
  B.dA_part = grad.take(n * B.one.nblk * (12 * J + 3) * d);
  B.dfeat = grad.take(n * P * d);
  B.g_eff = grad.take(n * n3 * d);
  B.grad_total = grad.at;
  B.saved_stride = B.one.saved_total;
  B.saved_total = n * B.saved_stride;
  B.chunks = (N + kChunk - 1) / kChunk;
  B.skin_chunks = (N + kSkinChunk - 1) / kSkinChunk;
  return B;
}

int check_batch(const char* who, int V, int J, int N, const void* shape_state, size_t shape_stride) {
  if (N < 1 || N > kMaxBatch) return fail(COMA_E_INVALID, "%s: N=%d outside [1, %d]", who, N, kMaxBatch);
  const size_t need = layout(V, J).shape_total;
  if (shape_stride != 0 && (shape_stride < need || (shape_stride & 15) != 0))
    return fail(COMA_E_INVALID, "%s: shape_stride=%zu must be 0 (one shape state for all bodies) or a multiple of 16 of at least %zu", who,
                shape_stride, need);
  if (((uintptr_t)shape_state & 15) != 0) return fail(COMA_E_INVALID, "%s: shape state must be 16-byte aligned", who);
  return COMA_OK;
}

}  // namespace
}  // namespace coma

extern "C" size_t coma_smplx_batch_workspace_bytes(int V, int J, int N) { return batch_ok(V, J, N) ? batch_layout(V, J, N).total : 0; }
extern "C" size_t coma_smplx_batch_saved_bytes(int V, int J, int N) { return batch_ok(V, J, N) ? batch_layout(V, J, N).saved_total : 0; }
extern "C" size_t coma_smplx_batch_grad_workspace_bytes(int V, int J, int N) { return batch_ok(V, J, N) ? batch_layout(V, J, N).grad_total : 0; }

extern "C" int coma_smplx_forward_batch_f32(const float* theta, const float* transl, const float* posedirs, const float* weights,
                                            const int32_t* parents, const float* hand_components, const float* pose_mean, int V, int J,
                                            int hand_dim, int n_pca, int N, const void* shape_state, size_t shape_stride, float* vertices,
                                            float* joints, float* full_pose, void* saved, size_t saved_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  const char* who = "coma_smplx_forward_batch_f32";
  if (!theta || !posedirs || !weights || !parents || !shape_state || !vertices || !joints || !saved || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  PoseArgs pa = {};
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pa.tree)) return rc;
  if (int rc = check_batch(who, V, J, N, shape_state, shape_stride)) return rc;
  const BatchLayout B = batch_layout(V, J, N);
  const Layout& L = B.one;
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, B.saved_total)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, B.total)) return rc;
  const char* st = (const char*)shape_state;
  char* sv = (char*)saved;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const BatchStrides bs = {N, n_pca > 0 ? 3 * J - 2 * hand_dim + 2 * n_pca : 3 * J, shape_stride, B.saved_stride};
  pa.theta = theta; pa.comps = hand_components; pa.mean = pose_mean; pa.transl = transl; pa.j_rest = (const double*)(st + L.j_rest);
  pa.J = J; pa.hd = hand_dim; pa.n_pca = n_pca; pa.s_pose = (double*)(sv + L.s_pose); pa.s_A = (double*)(sv + L.s_A);
  pa.feat = (double*)(ws + B.feat); pa.joints = joints; pa.full_pose = full_pose;
  hipLaunchKernelGGL(smplx_pose_batch_kernel, dim3(N), dim3(kBlock), 0, s, pa, bs);
  hipLaunchKernelGGL(smplx_offsets_batch_kernel, dim3(L.nb3, kPSplit, B.chunks), dim3(kBlock), 0, s, posedirs, (const double*)(ws + B.feat), L.P,
                     3 * V, L.rows, N, (double*)(ws + B.part));
  SkinArgs sa = {};
  sa.weights = weights; sa.A = pa.s_A; sa.v_shaped = (const double*)(st + L.v_shaped); sa.part = (const double*)(ws + B.part); sa.transl = transl;
  sa.V = V; sa.J = J; sa.v_posed = (double*)(sv + L.s_vposed); sa.vertices = vertices;
  hipLaunchKernelGGL(smplx_skin_batch_kernel, dim3(L.nblk, B.skin_chunks), dim3(kTile), 0, s, sa, bs);
  return check_launch(who);
}

extern "C" int coma_smplx_backward_batch_f32(const float* grad_vertices, const float* grad_joints, const float* grad_full_pose,
                                             const float* posedirs, const float* weights, const int32_t* parents, const float* hand_components,
                                             const int32_t* extra_index, const float* extra_weight, int E, int V, int J, int hand_dim, int n_pca,
                                             int N, const void* shape_state, size_t shape_stride, const void* saved, size_t saved_bytes,
                                             float* grad_theta, float* grad_transl, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "coma_smplx_backward_batch_f32";
  if (!posedirs || !weights || !parents || !shape_state || !saved || !grad_theta || !grad_transl || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (n_pca > 0 && hand_dim > 0 && !hand_components) return fail(COMA_E_INVALID, "%s: null pointer (hand_components with n_pca > 0)", who);
  PoseBwdArgs pb = {};
  if (int rc = check_common(who, V, J, hand_dim, n_pca, parents, pb.tree)) return rc;
  if (int rc = check_batch(who, V, J, N, shape_state, shape_stride)) return rc;
  if (E < 0 || E > kMaxE) return fail(COMA_E_INVALID, "%s: E=%d outside [0, %d]", who, E, kMaxE);
  const bool scatter = grad_joints && E > 0;
  if (scatter && (!extra_index || !extra_weight))
    return fail(COMA_E_INVALID, "%s: null pointer (the extra-joint tables with grad_joints and E > 0)", who);
  const BatchLayout B = batch_layout(V, J, N);
  const Layout& L = B.one;
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, B.saved_total)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, B.grad_total)) return rc;
  const char* st = (const char*)shape_state;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const BatchStrides bs = {N, n_pca > 0 ? 3 * J - 2 * hand_dim + 2 * n_pca : 3 * J, shape_stride, B.saved_stride};
  double* gvp = (double*)(ws + B.gvp);
  double* dA_part = (double*)(ws + B.dA_part);
  double* dfeat = (double*)(ws + B.dfeat);
  if (scatter || !grad_vertices) {                          // as the single-body full backward: only then is an effective gradient built
    double* g_eff = (double*)(ws + B.g_eff);
    hipLaunchKernelGGL(smplx_effective_grad_batch_kernel, dim3((V + kBlock - 1) / kBlock, N), dim3(kBlock), 0, s, grad_vertices,
                       scatter ? grad_joints : nullptr, J, extra_index, extra_weight, V, scatter ? E : 0, E, g_eff);
    SkinBwdArgs<double> sb = {};
    sb.weights = weights; sb.A = (const double*)(sv + L.s_A); sb.v_posed = (const double*)(sv + L.s_vposed); sb.grad = g_eff;
    sb.V = V; sb.J = J; sb.gvp = gvp; sb.dA_part = dA_part;
    hipLaunchKernelGGL(smplx_skin_bwd_batch_kernel<double>, dim3(L.nblk, B.skin_chunks), dim3(kTile), 0, s, sb, bs);
  } else {
    SkinBwdArgs<float> sb = {};
    sb.weights = weights; sb.A = (const double*)(sv + L.s_A); sb.v_posed = (const double*)(sv + L.s_vposed); sb.grad = grad_vertices;
    sb.V = V; sb.J = J; sb.gvp = gvp; sb.dA_part = dA_part;
    hipLaunchKernelGGL(smplx_skin_bwd_batch_kernel<float>, dim3(L.nblk, B.skin_chunks), dim3(kTile), 0, s, sb, bs);
  }
  if (L.P > 0)
    hipLaunchKernelGGL(smplx_feature_bwd_batch_kernel, dim3(L.P, B.chunks), dim3(kBlock), 0, s, posedirs, (const double*)gvp, 3 * V, L.P, N, dfeat);
  pb.s_pose = (const double*)(sv + L.s_pose); pb.j_rest = (const double*)(st + L.j_rest); pb.comps = hand_components;
  pb.dA_part = dA_part; pb.dfeat = dfeat; pb.J = J; pb.hd = hand_dim; pb.n_pca = n_pca; pb.nblk = L.nblk;
  pb.grad_theta = grad_theta; pb.grad_transl = grad_transl;
  pb.gJ = grad_joints; pb.gP = grad_full_pose; pb.extra_w = extra_weight; pb.E = scatter ? E : 0;
  hipLaunchKernelGGL(smplx_pose_bwd_batch_kernel, dim3(N), dim3(kBlock), 0, s, pb, bs);
  return check_launch(who);
}

extern "C" int coma_smplx_extra_joints_batch_f32(const float* vertices, const float* transl, const int32_t* vertex_index,
                                                 const float* vertex_weight, int V, int E, int N, float* out, void* stream) {
  const char* who = "coma_smplx_extra_joints_batch_f32";
  if (N < 1 || N > kMaxBatch) return fail(COMA_E_INVALID, "%s: N=%d outside [1, %d]", who, N, kMaxBatch);
  if (E == 0) return COMA_OK;
  if (!vertices || !vertex_index || !vertex_weight || !out) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (V < 1 || V > kMaxV || E < 0 || E > kMaxV) return fail(COMA_E_INVALID, "%s: bad sizes V=%d E=%d", who, V, E);
  hipLaunchKernelGGL(smplx_gather_batch_kernel, dim3((3 * E + kBlock - 1) / kBlock, N), dim3(kBlock), 0, (hipStream_t)stream, vertices, transl,
                     vertex_index, vertex_weight, V, E, out);
  return check_launch(who);
}
