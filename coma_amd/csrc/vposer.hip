// VPoser's pose decoder (forward and backward), its encoder (forward) and the SMPLify angle prior, for gfx950.
// replaces: the `pose_decoder` and `angle_prior` hooks of src/application/optimize.py (the reference's imports/vposer/vposer_smpl.py,
// imports/vposer/prior.py and the matrix -> quaternion -> axis-angle chain of its utils/transformations.py), called and differentiated
// in every iteration of the fit, by four launches forward and four backward on the caller's stream.  Rule set: include/coma_hip.h;
// restated in f64 in tests/vposer_ref.py.
//
// In the project's own words.  The decoder is a three-layer perceptron (leaky ReLU, slope 0.2) whose 6 NJ outputs are read, per
// joint, as two 3-vectors; Gram-Schmidt turns them into an orthonormal frame whose vectors are the COLUMNS of the joint's rotation.
// The rotation becomes a quaternion by the four-candidate rule (the candidate is chosen from the signs and sizes of the diagonal of
// the transposed matrix; only the chosen one is evaluated, the others are multiplied by zero in the reference and never reach its
// square root), and the quaternion becomes an axis-angle vector through 2 atan2(|v|, w) with both arguments negated when w < 0.
// The backward applies the analytic derivative of that tail for the branch the forward took (the forward stores it), then walks
// the three layers transposed.  At N = 1 the layers are GEMVs over 1.4 MB of weights: latency- and bandwidth-bound, so the
// arithmetic is f64 on f32 inputs and the outputs are the f32 rounding of the rule set.
//
// Forward layer: one wave per output row; lane l adds the products of columns l, l + 64, ... in ascending order (coalesced reads of
// the weight row), then the 64 partial sums are folded by v = v + v[lane ^ h], h = 32, 16, 8, 4, 2, 1.  Transposed layer: 64 columns
// per workgroup, one per lane; wave w of the 16 adds the rows o = w, w + 16, ... of its column in ascending order (a row's 64 columns
// are consecutive in memory), and the 16 partial sums are added in ascending w through LDS.  No floating-point atomics: two calls
// give the same bits.
#include "coma_device.h"
#include "fit_stages.h"

#include <cmath>

namespace coma {
namespace {

constexpr int kMaxN = 64, kMaxD = 256, kMaxH = 2048, kMaxNJ = 64;
constexpr int kMaxP = 4096, kMaxK = 16;      // angle prior: pose width and number of selected entries
constexpr int kFwdWaves = 4;                 // output rows per forward workgroup
constexpr int kBwdWaves = 16;                // row splits per transposed workgroup
constexpr double kSlope = 0.2;
constexpr double kNormEps = 1e-12;           // F.normalize's eps
constexpr double kDiagEps = 1e-6;            // the test on the (2,2) entry
constexpr double kBnEps = 1e-5;

// y[n, o] = epilogue(b[o] + sum_i W[o, i] x[n, i]); grid (ceil(Out / kFwdWaves), N).
// act: 0 none, 1 leaky ReLU.  y64 (f64 [N, Out]) or, when y64 is NULL, two f32 outputs of `split` columns each: rows o < split go to
// lo[n, o], rows o >= split to hi[n, o - split] after softplus (threshold 20) -- the encoder's mean and scale.
template <typename TX>
__global__ __launch_bounds__(kFwdWaves * kWave) void vposer_linear_kernel(const TX* __restrict__ x, const float* __restrict__ W,
                                                                          const float* __restrict__ b, int In, int Out, int act,
                                                                          double* __restrict__ y64, float* __restrict__ lo,
                                                                          float* __restrict__ hi, int split) {
  const int lane = threadIdx.x & (kWave - 1);
  const int o = blockIdx.x * kFwdWaves + (threadIdx.x >> 6);     // wave-uniform
  const int n = blockIdx.y;
  if (o >= Out) return;
  const float* row = W + (int64_t)o * In;
  double acc = 0.0;
  for (int i = lane; i < In; i += kWave) acc = acc + (double)row[i] * load(x, (int64_t)n * In + i);
#pragma unroll
  for (int h = kWave / 2; h >= 1; h >>= 1) acc = acc + __shfl_xor(acc, h, kWave);
  if (lane != 0) return;
  double v = acc + (double)b[o];
  if (act == 1) v = v > 0.0 ? v : v * kSlope;
  if (y64) {
    y64[(int64_t)n * Out + o] = v;
  } else if (o < split) {
    lo[(int64_t)n * split + o] = (float)v;
  } else {
    hi[(int64_t)n * split + (o - split)] = (float)(v > 20.0 ? v : log1p(exp(v)));
  }
}

// gx[n, i] = mask(h[n, i]) * sum_o W[o, i] gy[n, o]; grid (ceil(In / 64), N), kBwdWaves waves.
// h (f64 [N, In], the layer's activated input) may be NULL: no mask; else the factor is 1 where h > 0 and the slope elsewhere
// (the leaky ReLU keeps the sign of its argument).  Output f64 gx64 or f32 gx32.
__global__ __launch_bounds__(kBwdWaves * kWave) void vposer_linear_t_kernel(const double* __restrict__ gy, const float* __restrict__ W,
                                                                            const double* __restrict__ h, int In, int Out,
                                                                            double* __restrict__ gx64, float* __restrict__ gx32) {
  __shared__ double part[kBwdWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int i = blockIdx.x * kWave + lane;
  const int n = blockIdx.y;
  double acc = 0.0;
  if (i < In)
    for (int o = w; o < Out; o += kBwdWaves) acc = acc + (double)W[(int64_t)o * In + i] * gy[(int64_t)n * Out + o];
  part[w][lane] = acc;
  __syncthreads();
  if (w != 0 || i >= In) return;
  double s = part[0][lane];
#pragma unroll
  for (int k = 1; k < kBwdWaves; ++k) s = s + part[k][lane];
  if (h) s = h[(int64_t)n * In + i] > 0.0 ? s : s * kSlope;
  if (gx64) gx64[(int64_t)n * In + i] = s;
  else gx32[(int64_t)n * In + i] = (float)s;
}

// eval-mode BatchNorm1d over the columns: y = (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias; bn = [4, C] f32
template <typename TX>
__global__ __launch_bounds__(256) void vposer_bn_kernel(const TX* __restrict__ x, const float* __restrict__ bn, int C, int total,
                                                        double* __restrict__ y) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c = t % C;
  const double g = (double)bn[c], beta = (double)bn[C + c], m = (double)bn[2 * C + c], var = (double)bn[3 * C + c];
  y[t] = (load(x, t) - m) / sqrt(var + kBnEps) * g + beta;
}

// ---- the tail: 6 numbers -> rotation -> quaternion -> axis-angle ----
struct Tail {
  double n0, n1, dot;           // max(|c0|, eps), max(|u|, eps), b1 . c1
  bool free0, free1;            // the norm, not eps, divided
  D3 T[3];                      // T[i] = b_{i+1}: the TRANSPOSED rotation, the matrix the selection rule reads
  int branch;
  double t, q[4];               // the selected t and 0.5 cand / sqrt(t)
  double s2, s, tt, k;          // sin^2, sin, two_theta, the factor
};

__device__ __forceinline__ void candidate(const D3* T, int branch, double* t, double* c) {
  if (branch == 0) {
    *t = ((1.0 + T[0].x) - T[1].y) - T[2].z;
    c[0] = T[1].z - T[2].y; c[1] = *t; c[2] = T[0].y + T[1].x; c[3] = T[2].x + T[0].z;
  } else if (branch == 1) {
    *t = ((1.0 - T[0].x) + T[1].y) - T[2].z;
    c[0] = T[2].x - T[0].z; c[1] = T[0].y + T[1].x; c[2] = *t; c[3] = T[1].z + T[2].y;
  } else if (branch == 2) {
    *t = ((1.0 - T[0].x) - T[1].y) + T[2].z;
    c[0] = T[0].y - T[1].x; c[1] = T[2].x + T[0].z; c[2] = T[1].z + T[2].y; c[3] = *t;
  } else {
    *t = ((1.0 + T[0].x) + T[1].y) + T[2].z;
    c[0] = *t; c[1] = T[1].z - T[2].y; c[2] = T[2].x - T[0].z; c[3] = T[0].y - T[1].x;
  }
}

// forced >= 0: the branch the forward stored; < 0: select
__device__ __forceinline__ void tail_forward(const double* o, int forced, Tail& f, double* aa) {
  const D3 c0 = {o[0], o[2], o[4]}, c1 = {o[1], o[3], o[5]};
  const double l0 = norm(c0);
  f.free0 = l0 >= kNormEps; f.n0 = f.free0 ? l0 : kNormEps;
  f.T[0] = c0 / f.n0;
  f.dot = dot(f.T[0], c1);
  const D3 u = c1 - f.T[0] * f.dot;
  const double l1 = norm(u);
  f.free1 = l1 >= kNormEps; f.n1 = f.free1 ? l1 : kNormEps;
  f.T[1] = u / f.n1;
  f.T[2] = cross(f.T[0], f.T[1]);
  if (forced >= 0) f.branch = forced;
  else if (f.T[2].z < kDiagEps) f.branch = f.T[0].x > f.T[1].y ? 0 : 1;
  else f.branch = f.T[0].x < -f.T[1].y ? 2 : 3;
  double c[4];
  candidate(f.T, f.branch, &f.t, c);
  const double root = sqrt(f.t);
  for (int e = 0; e < 4; ++e) f.q[e] = c[e] / root * 0.5;
  f.s2 = (f.q[1] * f.q[1] + f.q[2] * f.q[2]) + f.q[3] * f.q[3];
  f.s = sqrt(f.s2);
  f.tt = 2.0 * (f.q[0] < 0.0 ? atan2(-f.s, -f.q[0]) : atan2(f.s, f.q[0]));
  f.k = f.s2 > 0.0 ? f.tt / f.s : 2.0;
  for (int e = 0; e < 3; ++e) aa[e] = f.q[e + 1] * f.k;
}

// dL/do [6] from dL/daa [3]
__device__ __forceinline__ void tail_backward(const double* o, const Tail& f, const double* ga, double* go) {
  // axis-angle <- quaternion
  double gq[4];
  const double gk = (ga[0] * f.q[1] + ga[1] * f.q[2]) + ga[2] * f.q[3];
  for (int e = 0; e < 3; ++e) gq[e + 1] = ga[e] * f.k;
  gq[0] = 0.0;
  if (f.s2 > 0.0) {                       // else k = 2 is a constant: the finite gradient at the identity
    const double gtt = gk / f.s;
    const double r2 = f.s2 + f.q[0] * f.q[0];
    const double gs = -gk * f.tt / f.s2 + 2.0 * gtt * f.q[0] / r2;
    gq[0] = -2.0 * gtt * f.s / r2;
    const double gs2 = gs / (2.0 * f.s);
    for (int e = 1; e < 4; ++e) gq[e] = gq[e] + 2.0 * f.q[e] * gs2;
  }
  // quaternion <- the selected candidate: q = 0.5 c / sqrt(t)
  const double root = sqrt(f.t);
  double gc[4];
  for (int e = 0; e < 4; ++e) gc[e] = 0.5 * gq[e] / root;
  double gt = -0.5 * (((gq[0] * f.q[0] + gq[1] * f.q[1]) + gq[2] * f.q[2]) + gq[3] * f.q[3]) / f.t;
  D3 g[3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};       // dL/dT, row by row
  if (f.branch == 0) {
    gt = gt + gc[1];
    g[0].x = gt; g[1].y = -gt; g[2].z = -gt;
    g[1].z = gc[0]; g[2].y = -gc[0]; g[0].y = gc[2]; g[1].x = gc[2]; g[2].x = gc[3]; g[0].z = gc[3];
  } else if (f.branch == 1) {
    gt = gt + gc[2];
    g[0].x = -gt; g[1].y = gt; g[2].z = -gt;
    g[2].x = gc[0]; g[0].z = -gc[0]; g[0].y = gc[1]; g[1].x = gc[1]; g[1].z = gc[3]; g[2].y = gc[3];
  } else if (f.branch == 2) {
    gt = gt + gc[3];
    g[0].x = -gt; g[1].y = -gt; g[2].z = gt;
    g[0].y = gc[0]; g[1].x = -gc[0]; g[2].x = gc[1]; g[0].z = gc[1]; g[1].z = gc[2]; g[2].y = gc[2];
  } else {
    gt = gt + gc[0];
    g[0].x = gt; g[1].y = gt; g[2].z = gt;
    g[1].z = gc[1]; g[2].y = -gc[1]; g[2].x = gc[2]; g[0].z = -gc[2]; g[0].y = gc[3]; g[1].x = -gc[3];
  }
  // Gram-Schmidt: b3 = b1 x b2, b2 = u / n1, u = c1 - (b1 . c1) b1, b1 = c0 / n0
  D3 gb1 = g[0] + cross(f.T[1], g[2]);
  const D3 gb2 = g[1] + cross(g[2], f.T[0]);
  const double p2 = f.free1 ? dot(f.T[1], gb2) : 0.0;
  const D3 gu = (gb2 - f.T[1] * p2) / f.n1;
  const D3 c1 = {o[1], o[3], o[5]};
  const double pu = dot(gu, f.T[0]);
  const D3 gc1 = gu - f.T[0] * pu;
  gb1 = gb1 - (gu * f.dot + c1 * pu);
  const double p1 = f.free0 ? dot(f.T[0], gb1) : 0.0;
  const D3 gc0 = (gb1 - f.T[0] * p1) / f.n0;
  go[0] = gc0.x; go[1] = gc1.x; go[2] = gc0.y; go[3] = gc1.y; go[4] = gc0.z; go[5] = gc1.z;
}

// one thread per (n, joint)
__global__ __launch_bounds__(256) void vposer_tail_kernel(const double* __restrict__ o, int total, float* __restrict__ aa,
                                                          float* __restrict__ matrices, int8_t* __restrict__ branch,
                                                          int8_t* __restrict__ saved_branch) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  double in[6], out[3];
  for (int e = 0; e < 6; ++e) in[e] = o[(int64_t)t * 6 + e];
  Tail f;
  tail_forward(in, -1, f, out);
  for (int e = 0; e < 3; ++e) aa[(int64_t)t * 3 + e] = (float)out[e];
  saved_branch[t] = (int8_t)f.branch;
  if (branch) branch[t] = (int8_t)f.branch;
  if (matrices)
    for (int c = 0; c < 3; ++c) {                       // the rotation's column c is T[c]
      float* m = matrices + (int64_t)t * 9 + c;
      m[0] = (float)f.T[c].x; m[3] = (float)f.T[c].y; m[6] = (float)f.T[c].z;
    }
}

__global__ __launch_bounds__(256) void vposer_tail_bwd_kernel(const double* __restrict__ o, const int8_t* __restrict__ saved_branch,
                                                              const float* __restrict__ grad_aa, int total, double* __restrict__ go) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  double in[6], out[3], ga[3], g[6];
  for (int e = 0; e < 6; ++e) in[e] = o[(int64_t)t * 6 + e];
  for (int e = 0; e < 3; ++e) ga[e] = (double)grad_aa[(int64_t)t * 3 + e];
  Tail f;
  tail_forward(in, (int)saved_branch[t] & 3, f, out);
  tail_backward(in, f, ga, g);
  for (int e = 0; e < 6; ++e) go[(int64_t)t * 6 + e] = g[e];
}

// ---- the angle prior ----
struct PriorArgs { int32_t index[kMaxK]; float sign[kMaxK]; int K; };

__global__ __launch_bounds__(256) void angle_prior_kernel(const float* __restrict__ pose, int N, int P, PriorArgs a, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N * a.K) return;
  const int n = t / a.K, k = t % a.K;
  const double e = exp((double)a.sign[k] * (double)pose[(int64_t)n * P + a.index[k]]);
  out[t] = (float)(e * e);
}

// grad_pose[n, p] = sum over k with index[k] == p, ascending, of grad_out[n, k] 2 sign[k] exp(sign[k] pose[n, p])^2; zero elsewhere
__global__ __launch_bounds__(256) void angle_prior_bwd_kernel(const float* __restrict__ pose, const float* __restrict__ grad_out, int N, int P,
                                                              PriorArgs a, float* __restrict__ grad_pose) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N * P) return;
  const int n = t / P, p = t % P;
  double g = 0.0;
  for (int k = 0; k < a.K; ++k)
    if (a.index[k] == p) {
      const double s = (double)a.sign[k];
      const double e = exp(s * (double)pose[t]);
      g = g + (double)grad_out[(int64_t)n * a.K + k] * (2.0 * s * (e * e));
    }
  grad_pose[t] = (float)g;
}

// ---- host side ----
struct Layout {
  size_t h1, h2, o, branch, saved_total;     // saved: h1, h2 f64 [N,H]; o f64 [N,6NJ]; branch i8 [N,NJ]
  size_t a, b, c, total;                     // workspace: three f64 [N, max(H, 6 NJ)]
};

Layout layout(int N, int H, int NJ) {
  Layout L;
  const size_t d = sizeof(double);
  Carve saved, ws;
  L.h1 = saved.take((size_t)N * H * d);
  L.h2 = saved.take((size_t)N * H * d);
  L.o = saved.take((size_t)N * 6 * NJ * d);
  L.branch = saved.take((size_t)N * NJ);
  L.saved_total = saved.at;
  const size_t wide = (size_t)N * (H > 6 * NJ ? H : 6 * NJ) * d;
  L.a = ws.take(wide);
  L.b = ws.take(wide);
  L.c = ws.take(wide);
  L.total = ws.at;
  return L;
}

bool sizes_ok(int N, int H, int NJ) { return N >= 1 && N <= kMaxN && H >= 1 && H <= kMaxH && NJ >= 1 && NJ <= kMaxNJ; }

int check_sizes(const char* who, int N, int D, int H, int NJ) {
  if (!sizes_ok(N, H, NJ) || D < 1 || D > kMaxD)
    return fail(COMA_E_INVALID, "%s: N=%d must lie in [1, %d], D=%d in [1, %d], H=%d in [1, %d] and NJ=%d in [1, %d]", who, N, kMaxN, D, kMaxD, H,
                kMaxH, NJ, kMaxNJ);
  return COMA_OK;
}

template <typename TX>
void linear(hipStream_t s, const TX* x, const float* W, const float* b, int N, int In, int Out, int act, double* y64, float* lo = nullptr,
            float* hi = nullptr, int split = 0) {
  hipLaunchKernelGGL(vposer_linear_kernel<TX>, dim3((Out + kFwdWaves - 1) / kFwdWaves, N), dim3(kFwdWaves * kWave), 0, s, x, W, b, In, Out, act, y64,
                     lo, hi, split);
}

void linear_t(hipStream_t s, const double* gy, const float* W, const double* h, int N, int In, int Out, double* gx64, float* gx32) {
  hipLaunchKernelGGL(vposer_linear_t_kernel, dim3((In + kWave - 1) / kWave, N), dim3(kBwdWaves * kWave), 0, s, gy, W, h, In, Out, gx64, gx32);
}

int prior_args(const char* who, int N, int P, const int32_t* index, const float* sign, int K, PriorArgs& a) {
  if (N < 1 || N > kMaxN || P < 1 || P > kMaxP || K < 1 || K > kMaxK)
    return fail(COMA_E_INVALID, "%s: N=%d must lie in [1, %d], P=%d in [1, %d] and K=%d in [1, %d]", who, N, kMaxN, P, kMaxP, K, kMaxK);
  a = PriorArgs{};
  a.K = K;
  for (int k = 0; k < K; ++k) {
    if (index[k] < 0 || index[k] >= P) return fail(COMA_E_INVALID, "%s: index[%d]=%d outside [0, %d)", who, k, index[k], P);
    a.index[k] = index[k];
    a.sign[k] = sign[k];
  }
  return COMA_OK;
}

}  // namespace

int vposer_decode_plan(const char* who, const float* z, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                       const float* b3, int N, int D, int H, int NJ, float* aa, float* matrices, int8_t* branch, void* saved, size_t saved_bytes,
                       VposerDecodePlan& p) {
  if (!z || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !aa || !saved) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (int rc = check_sizes(who, N, D, H, NJ)) return rc;
  if (!f32_aligned({z, W1, b1, W2, b2, W3, b3, aa, matrices})) return fail(COMA_E_INVALID, "%s: an f32 buffer is not 4-byte aligned", who);
  const Layout L = layout(N, H, NJ);
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, L.saved_total)) return rc;
  char* sv = (char*)saved;
  p = {who, z, W1, b1, W2, b2, W3, b3, N, D, H, NJ, (double*)(sv + L.h1), (double*)(sv + L.h2), (double*)(sv + L.o), (int8_t*)(sv + L.branch),
       aa, matrices, branch};
  return COMA_OK;
}

int vposer_decode_enqueue(const VposerDecodePlan& p, hipStream_t s) {
  linear(s, p.z, p.W1, p.b1, p.N, p.D, p.H, 1, p.h1);
  linear(s, (const double*)p.h1, p.W2, p.b2, p.N, p.H, p.H, 1, p.h2);
  linear(s, (const double*)p.h2, p.W3, p.b3, p.N, p.H, 6 * p.NJ, 0, p.o);
  const int total = p.N * p.NJ;
  hipLaunchKernelGGL(vposer_tail_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const double*)p.o, total, p.aa, p.matrices, p.branch,
                     p.saved_branch);
  return check_launch(p.who);
}

int vposer_decode_backward_plan(const char* who, const float* grad_aa, const float* W1, const float* W2, const float* W3, int N, int D, int H,
                                int NJ, const void* saved, size_t saved_bytes, float* grad_z, void* workspace, size_t workspace_bytes,
                                VposerDecodeBackwardPlan& p) {
  if (!grad_aa || !W1 || !W2 || !W3 || !saved || !grad_z || !workspace) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (int rc = check_sizes(who, N, D, H, NJ)) return rc;
  if (!f32_aligned({grad_aa, W1, W2, W3, grad_z})) return fail(COMA_E_INVALID, "%s: an f32 buffer is not 4-byte aligned", who);
  const Layout L = layout(N, H, NJ);
  if (int rc = check_buffer(who, "saved state", saved, saved_bytes, L.saved_total)) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  p = {who, grad_aa, W1, W2, W3, N, D, H, NJ, (const double*)(sv + L.h1), (const double*)(sv + L.h2), (const double*)(sv + L.o),
       (const int8_t*)(sv + L.branch), (double*)(ws + L.a), (double*)(ws + L.b), (double*)(ws + L.c), grad_z};
  return COMA_OK;
}

int vposer_decode_backward_enqueue(const VposerDecodeBackwardPlan& p, hipStream_t s) {
  const int total = p.N * p.NJ;
  hipLaunchKernelGGL(vposer_tail_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, s, p.o, p.saved_branch, p.grad_aa, total, p.go);
  linear_t(s, p.go, p.W3, p.h2, p.N, p.H, 6 * p.NJ, p.gh2, nullptr);
  linear_t(s, p.gh2, p.W2, p.h1, p.N, p.H, p.H, p.gh1, nullptr);
  linear_t(s, p.gh1, p.W1, nullptr, p.N, p.D, p.H, nullptr, p.grad_z);
  return check_launch(p.who);
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_vposer_saved_bytes(int N, int H, int NJ) { return sizes_ok(N, H, NJ) ? layout(N, H, NJ).saved_total : 0; }
extern "C" size_t coma_vposer_workspace_bytes(int N, int H, int NJ) { return sizes_ok(N, H, NJ) ? layout(N, H, NJ).total : 0; }

extern "C" int coma_vposer_decode_f32(const float* z, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                                      const float* b3, int N, int D, int H, int NJ, float* aa, float* matrices, int8_t* branch, void* saved,
                                      size_t saved_bytes, void* stream) {
  VposerDecodePlan p;
  if (int rc = vposer_decode_plan("coma_vposer_decode_f32", z, W1, b1, W2, b2, W3, b3, N, D, H, NJ, aa, matrices, branch, saved, saved_bytes, p)) return rc;
  return vposer_decode_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_vposer_decode_backward_f32(const float* grad_aa, const float* W1, const float* W2, const float* W3, int N, int D, int H,
                                               int NJ, const void* saved, size_t saved_bytes, float* grad_z, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  VposerDecodeBackwardPlan p;
  if (int rc = vposer_decode_backward_plan("coma_vposer_decode_backward_f32", grad_aa, W1, W2, W3, N, D, H, NJ, saved, saved_bytes, grad_z, workspace,
                                           workspace_bytes, p))
    return rc;
  return vposer_decode_backward_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_vposer_encode_f32(const float* pose, const float* bn1, const float* W1, const float* b1, const float* bn2, const float* W2,
                                      const float* b2, const float* Wml, const float* bml, int N, int D, int H, int NJ, float* mean,
                                      float* scale, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "coma_vposer_encode_f32";
  if (!pose || !bn1 || !W1 || !b1 || !bn2 || !W2 || !b2 || !Wml || !bml || !mean || !scale || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (int rc = check_sizes(who, N, D, H, NJ)) return rc;
  if (!f32_aligned({pose, bn1, W1, b1, bn2, W2, b2, Wml, bml, mean, scale})) return fail(COMA_E_INVALID, "%s: an f32 buffer is not 4-byte aligned", who);
  const Layout L = layout(N, H, NJ);
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  double *a = (double*)(ws + L.a), *b = (double*)(ws + L.b);
  const int F = 3 * NJ;
  hipLaunchKernelGGL(vposer_bn_kernel<float>, dim3((N * F + 255) / 256), dim3(256), 0, s, pose, bn1, F, N * F, a);
  linear(s, (const double*)a, W1, b1, N, F, H, 1, b);
  hipLaunchKernelGGL(vposer_bn_kernel<double>, dim3((N * H + 255) / 256), dim3(256), 0, s, (const double*)b, bn2, H, N * H, a);
  linear(s, (const double*)a, W2, b2, N, H, H, 1, b);
  linear(s, (const double*)b, Wml, bml, N, H, 2 * D, 0, (double*)nullptr, mean, scale, D);
  return check_launch(who);
}

extern "C" int coma_angle_prior_f32(const float* pose, int N, int P, const int32_t* index, const float* sign, int K, float* out, void* stream) {
  const char* who = "coma_angle_prior_f32";
  if (!pose || !index || !sign || !out) return fail(COMA_E_INVALID, "%s: null pointer", who);
  PriorArgs a;
  if (int rc = prior_args(who, N, P, index, sign, K, a)) return rc;
  hipLaunchKernelGGL(angle_prior_kernel, dim3((N * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, pose, N, P, a, out);
  return check_launch(who);
}

extern "C" int coma_angle_prior_backward_f32(const float* pose, const float* grad_out, int N, int P, const int32_t* index, const float* sign,
                                             int K, float* grad_pose, void* stream) {
  const char* who = "coma_angle_prior_backward_f32";
  if (!pose || !grad_out || !index || !sign || !grad_pose) return fail(COMA_E_INVALID, "%s: null pointer", who);
  PriorArgs a;
  if (int rc = prior_args(who, N, P, index, sign, K, a)) return rc;
  hipLaunchKernelGGL(angle_prior_bwd_kernel, dim3((N * P + 255) / 256), dim3(256), 0, (hipStream_t)stream, pose, grad_out, N, P, a, grad_pose);
  return check_launch(who);
}
