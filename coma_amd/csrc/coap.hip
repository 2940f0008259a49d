// COAP (gfx950): the learned occupancy body model behind the collision loss -- encode a posed body once, then query points against
// it, values and the derivative along the camera's front vector.  The rule set is stated in include/coma_hip.h ("COAP") and restated
// in NumPy by tests/coap_ref.py.
//
// All matrix work runs on the fp32 matrix unit (v_mfma_f32_32x32x2_f32) through ONE tile routine, gemm(): a workgroup of four waves
// owns 64 rows whose activations stay in LDS (row stride 260 floats: a lane's 16-byte fragment reads are conflict-free), every wave
// computes both 32-row halves for its own 32-column blocks, and the weights -- packed on the host in fragment order, so that a wave's
// read of one (column block, 8 k) step is one contiguous KB -- stream from L2 straight into registers, one step ahead of the MFMAs.
// Operand reads follow seg_gemm.hip: ONE 16-byte read per operand tile and 8 k, lanes 0-31 taking k = 8g .. 8g+3 and lanes 32-63
// k = 8g+4 .. 8g+7, MFMA step e consuming element e of both.  Every sum therefore runs in a fixed k order.
//
// coma_coap_encode_f32: reset -> geometry (Rodrigues chain, per-part boxes, the posed vertices' box; f64) -> PointNet stage 0
//   (fc_pos, block_0) -> [fold (the pooled half of the next block's input as per-part biases) -> stage i] x 3 -> latent (fc_c, and
//   the per-part biases of the query encoder's layers 0 and 2: one-hot, inside = 1 and latent inputs folded).  The per-part maximum
//   between the stages is an integer-keyed atomic maximum, which does not depend on the order of arrival.
// coma_coap_query_f32: reset -> list ((part, point) pairs whose point lies in the part's box; wave-aggregated append, count on the
//   device) -> mlp: ONE launch for all ten 256-wide layers and the last dot, persistent workgroups over tiles of the list (bounded by
//   the list's capacity); with the derivative a tile is 32 pairs, value rows 0-31 and their tangent rows 32-63 through the same weight
//   fragments (y' = W x', then y' softplus'(y)); the skip concatenations are formed in place in LDS; the per-point maximum over the
//   parts is an integer-keyed atomic maximum of (occ, docc) -> finalize (keys to occ, docc).
// coma_coap_collision_f32: the same with the bounding-box prefilter in `list` and, for finalize, the fixed-shape f64 sum: block
//   partials in block order, then one workgroup.
#include "coap_internal.h"
#include "coma_device.h"

namespace coma {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCoapMaxParts = 32, kCoapMaxJoints = 64, kCoapMaxSamples = 4096, kCoapMaxPoints = 1 << 22, kCoapMaxVerts = 1 << 24;
constexpr int kLatent = 128, kLd = 260, kSd = 132, kRows = 64;
constexpr int kCoapMagic = 0x434f4150;
constexpr int kGeoDoubles = 24;   // per part: R (9, row-major, world from local), origin (3), box centre (3), half size (3), min (3), max (3)
constexpr int kMlpMaxBlocks = 2048;
constexpr float kBeta = 100.0f, kThreshold = 20.0f;
enum { kCoapBadIndex = 1, kCoapNonFinite = 2 };

struct CodeLayout {
  size_t geo, vbox, latent, bias0, bias2, total;
};

static CodeLayout code_layout(int K) {
  Carve c;
  c.take(16);   // header: magic, K, status, pad
  CodeLayout l;
  l.geo = c.take((size_t)K * kGeoDoubles * sizeof(double));
  l.vbox = c.take(6 * sizeof(double));
  l.latent = c.take((size_t)K * kLatent * sizeof(float));
  l.bias0 = c.take((size_t)K * 256 * sizeof(float));
  l.bias2 = c.take((size_t)K * 256 * sizeof(float));
  l.total = c.at;
  return l;
}

// offsets into the packed weights, in floats; the order and the sizes are those of coma_amd/coap.py's pack_weights
struct CoapLayout {
  int K, n1, nb1, g2;   // n1 = 124 - K outputs of the query encoder's lin1, in nb1 column blocks; layer 2 reads g2 steps of 8 k
  long long e_pos_w, e_pos_b, e_fc0[4], e_sc[4], e_fc1[4], e_b0[4], e_b1[4], e_fc0p[4], e_scp[4], e_fcc_w, e_fcc_b;
  long long q_in[2], q_hot[2], q_lat[2], q_b[2];
  long long w[10], b[10], w6, b6, total;
};

static CoapLayout coap_layout(int K) {
  CoapLayout l = {};
  long long at = 0;
  auto take = [&](long long n) { const long long o = at; at += n; return o; };
  auto frag = [&](int nb, int g) { return take((long long)nb * g * 256); };
  l.K = K, l.n1 = 124 - K, l.nb1 = (l.n1 + 31) / 32, l.g2 = (l.n1 + 3 + 7) / 8;
  l.e_pos_w = frag(8, 1), l.e_pos_b = take(256);
  for (int i = 0; i < 4; ++i) {
    const int g = i == 0 ? 32 : 16;
    l.e_fc0[i] = frag(4, g), l.e_sc[i] = frag(4, g), l.e_fc1[i] = frag(4, 16), l.e_b0[i] = take(128), l.e_b1[i] = take(128);
    if (i) l.e_fc0p[i] = take(128 * 128), l.e_scp[i] = take(128 * 128);
  }
  l.e_fcc_w = take(128 * 128), l.e_fcc_b = take(128);
  for (int i = 0; i < 2; ++i) l.q_in[i] = take(256), l.q_hot[i] = take((long long)K * 256), l.q_lat[i] = take(128 * 256), l.q_b[i] = take(256);
  const int nb[10] = {8, l.nb1, 8, 4, 8, 8, 4, 8, 8, 8}, g[10] = {1, 32, l.g2, 32, 17, 32, 32, 32, 32, 32};
  for (int i = 0; i < 10; ++i) l.w[i] = frag(nb[i], g[i]), l.b[i] = take(nb[i] * 32);
  l.w6 = take(256), l.b6 = take(4);
  l.total = at;
  return l;
}

// ---- the tile routine ----
// acc[h][j] (+)= X[32 h .. 32 h + 31][0 .. 8 G) . W for the column blocks nb = wave + 4 j < NB of this wave.  X: LDS, row stride kLd.
// Wf: fragments [NB][G][64 lanes][4]: lane l of step g holds W[k = 8 g + 4 (l >> 5) + e][n = 32 nb + (l & 31)], e = 0 .. 3.
template <int NBW>
__device__ __forceinline__ void gemm(const float* X, const float* __restrict__ Wf, int G, int NB, f32x16 (&acc)[2][NBW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NBW; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[h][j][i] = 0.0f;
  if (wave >= NB) return;
  const float* a0 = X + (lane & 31) * kLd + 4 * (lane >> 5);
  const float* a1 = a0 + 32 * kLd;
  const f32x4* wp[NBW];
  f32x4 next[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    const int nb = wave + 4 * j < NB ? wave + 4 * j : wave;
    wp[j] = (const f32x4*)Wf + (size_t)nb * G * 64 + lane;
    next[j] = wp[j][0];
  }
  for (int g = 0; g < G; ++g) {
    f32x4 w[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      w[j] = next[j];
      if (g + 1 < G) next[j] = wp[j][(size_t)(g + 1) * 64];
    }
    const f32x4 x0 = *(const f32x4*)(a0 + 8 * g), x1 = *(const f32x4*)(a1 + 8 * g);
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      if (wave + 4 * j >= NB) continue;
      acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, w[j].x, acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, w[j].x, acc[1][j], 0, 0, 0);
      acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, w[j].y, acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, w[j].y, acc[1][j], 0, 0, 0);
      acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, w[j].z, acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, w[j].z, acc[1][j], 0, 0, 0);
      acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, w[j].w, acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, w[j].w, acc[1][j], 0, 0, 0);
    }
  }
}

// f(row in [0, 32), col, value of row, value of row + 32) over this wave's accumulator elements: D[row = 8 (i / 4) + 4 (lane / 32) + i % 4][col = lane % 32]
template <int NBW, typename F>
__device__ __forceinline__ void each_pair(const f32x16 (&acc)[2][NBW], int NB, F&& f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    if (wave + 4 * j >= NB) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) f(8 * (i >> 2) + 4 * (lane >> 5) + (i & 3), 32 * (wave + 4 * j) + (lane & 31), acc[0][j][i], acc[1][j][i]);
  }
}

// Softplus(beta = 100) with torch's threshold of 20, and its slope
__device__ __forceinline__ float softplus(float y, float* slope) {
  const float z = kBeta * y;
  if (z > kThreshold) {
    *slope = 1.0f;
    return y;
  }
  const float e = expf(z);
  *slope = e / (e + 1.0f);
  return log1pf(e) / kBeta;
}

__device__ __forceinline__ unsigned max_key(float v) {   // monotone in v
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float max_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- encode ----
struct CoapTree {
  int mK, K;
  int parents[kCoapMaxJoints];
  int mapped[kCoapMaxParts];
};

__global__ __launch_bounds__(256) void coap_reset_encode_kernel(int* __restrict__ hdr, int K, unsigned* __restrict__ pooled, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) pooled[i] = 0u;
  if (i == 0) hdr[0] = kCoapMagic, hdr[1] = K, hdr[2] = 0, hdr[3] = 0;
}

// Workgroups 0 .. K - 1: a part's transform and the box of its own vertices in its frame; workgroup K: the posed vertices' box.
__global__ __launch_bounds__(256) void coap_geometry_kernel(CoapTree tree, const float* __restrict__ full_pose, const float* __restrict__ joints,
                                                            const float* __restrict__ vertices, int V, const int* __restrict__ selector, int S,
                                                            char* __restrict__ code, CodeLayout cl) {
  __shared__ double rot[kCoapMaxJoints][9], chain[kCoapMaxJoints][9], lo[256][3], hi[256][3];
  const int tid = threadIdx.x, b = blockIdx.x;
  int* hdr = (int*)code;
  if (tid < tree.mK) {   // batch_rodrigues: the angle is the norm of r + 1e-8, the axis r / angle
    const D3 r = load3(full_pose, tid);
    const D3 e = {r.x + 1e-8, r.y + 1e-8, r.z + 1e-8};
    const double a = norm(e);
    const D3 u = r / a;
    const double s = sin(a), c = 1.0 - cos(a);
    const double k[9] = {0.0, -u.z, u.y, u.z, 0.0, -u.x, -u.y, u.x, 0.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double kk = (k[3 * i] * k[j] + k[3 * i + 1] * k[3 + j]) + k[3 * i + 2] * k[6 + j];
        rot[tid][3 * i + j] = ((i == j ? 1.0 : 0.0) + s * k[3 * i + j]) + c * kk;
      }
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 0; j < 9; ++j) chain[0][j] = rot[0][j];
    for (int n = 1; n < tree.mK; ++n) {
      const double* p = chain[tree.parents[n]];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) chain[n][3 * i + j] = (p[3 * i] * rot[n][j] + p[3 * i + 1] * rot[n][3 + j]) + p[3 * i + 2] * rot[n][6 + j];
    }
  }
  __syncthreads();
  const bool whole = b == tree.K;
  const int joint = whole ? 0 : tree.mapped[b];
  const double* R = chain[joint];
  const D3 o = load3(joints, joint);
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  const int count = whole ? V : S;
  for (int s = tid; s < count; s += 256) {
    int v = whole ? s : selector[(int64_t)b * S + s];
    if (v < 0 || v >= V) bad |= kCoapBadIndex, v = 0;
    const D3 p = load3(vertices, v);
    if (!(__builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z))) bad |= kCoapNonFinite;
    double q[3] = {p.x, p.y, p.z};
    if (!whole) {
      const D3 w = p - o;   // R^T (v - j): the analytic inverse of the rigid transform
      for (int c = 0; c < 3; ++c) q[c] = (R[c] * w.x + R[3 + c] * w.y) + R[6 + c] * w.z;
    }
    for (int c = 0; c < 3; ++c) mn[c] = fmin(mn[c], q[c]), mx[c] = fmax(mx[c], q[c]);
  }
  for (int c = 0; c < 3; ++c) lo[tid][c] = mn[c], hi[tid][c] = mx[c];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h)
      for (int c = 0; c < 3; ++c) lo[tid][c] = fmin(lo[tid][c], lo[tid + h][c]), hi[tid][c] = fmax(hi[tid][c], hi[tid + h][c]);
    __syncthreads();
  }
  if (bad) atomicOr(&hdr[2], bad);
  if (tid != 0) return;
  if (whole) {
    double* out = (double*)(code + cl.vbox);
    for (int c = 0; c < 3; ++c) out[c] = lo[0][c], out[3 + c] = hi[0][c];
    return;
  }
  double* g = (double*)(code + cl.geo) + (int64_t)b * kGeoDoubles;
  for (int j = 0; j < 9; ++j) g[j] = R[j];
  g[9] = o.x, g[10] = o.y, g[11] = o.z;
  for (int c = 0; c < 3; ++c) {
    g[12 + c] = (lo[0][c] + hi[0][c]) * 0.5;
    g[15 + c] = (fabs(hi[0][c] - lo[0][c]) * 1.125) * 0.5;
    g[18 + c] = lo[0][c], g[21 + c] = hi[0][c];
  }
  if (!(__builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) && __builtin_isfinite(R[0]))) atomicOr(&hdr[2], (int)kCoapNonFinite);
}

// One ResnetBlockFC over a tile of 64 samples of one part (grid: tiles x K).  FIRST: the local sample points through fc_pos, then
// block_0 on the 256-wide result; otherwise a block on net [128] | pooled [128], the pooled half folded into c0 / cs per part.
// net (in place), [K][n][128]; pooled_out [K][128] keys.  Rows past n repeat sample n - 1: the maximum does not see them.
template <bool FIRST>
__global__ __launch_bounds__(256) void coap_block_kernel(CoapLayout L, int blk, const float* __restrict__ W, const float* __restrict__ vertices, int V,
                                                         const int* __restrict__ ids, const float* __restrict__ bary, int n, char* __restrict__ code,
                                                         CodeLayout cl, const float* __restrict__ c0, const float* __restrict__ cs,
                                                         float* __restrict__ net, unsigned* __restrict__ pooled_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XR = lds;                 // the block's input
  float* XA = lds + kRows * kLd;   // relu of it, then the hidden layer
  const int tid = threadIdx.x, k = blockIdx.y, row0 = blockIdx.x * kRows;
  if (FIRST) {
    if (tid < kRows) {
      const int s = min(row0 + tid, n - 1);
      const double* g = (const double*)(code + cl.geo) + (int64_t)k * kGeoDoubles;
      const int64_t at = ((int64_t)k * n + s) * 3;
      int id[3] = {ids[at], ids[at + 1], ids[at + 2]};
      for (int c = 0; c < 3; ++c)
        if (id[c] < 0 || id[c] >= V) atomicOr((int*)code + 2, (int)kCoapBadIndex), id[c] = 0;
      const D3 v0 = load3(vertices, id[0]), v1 = load3(vertices, id[1]), v2 = load3(vertices, id[2]);
      const double b1 = (double)bary[at + 1], b2 = (double)bary[at + 2];   // the first weight is implied: the three sum to one exactly
      const D3 p = (v0 + (v1 - v0) * b1) + (v2 - v0) * b2;
      const D3 w = p - D3{g[9], g[10], g[11]};
      float* x = XR + tid * kLd;
      for (int c = 0; c < 3; ++c) x[c] = (float)((g[c] * w.x + g[3 + c] * w.y) + g[6 + c] * w.z);
      for (int c = 3; c < 8; ++c) x[c] = 0.0f;
    }
    __syncthreads();
    f32x16 acc[2][2];
    gemm<2>(XR, W + L.e_pos_w, 1, 8, acc);
    __syncthreads();
    const float* bias = W + L.e_pos_b;
    each_pair<2>(acc, 8, [&](int r, int c, float a, float b) {
      const float y0 = a + bias[c], y1 = b + bias[c];
      XR[r * kLd + c] = y0, XR[(r + 32) * kLd + c] = y1;
      XA[r * kLd + c] = fmaxf(y0, 0.0f), XA[(r + 32) * kLd + c] = fmaxf(y1, 0.0f);
    });
  } else {
    for (int i = tid; i < kRows * 128; i += 256) {
      const int r = i >> 7, c = i & 127;
      const float v = net[((int64_t)k * n + min(row0 + r, n - 1)) * 128 + c];
      XR[r * kLd + c] = v, XA[r * kLd + c] = fmaxf(v, 0.0f);
    }
  }
  __syncthreads();
  const int G = FIRST ? 32 : 16;
  f32x16 sc[2][1], hid[2][1];
  gemm<1>(XR, W + L.e_sc[blk], G, 4, sc);
  gemm<1>(XA, W + L.e_fc0[blk], G, 4, hid);
  __syncthreads();
  const float* b0 = FIRST ? W + L.e_b0[blk] : c0 + k * 128;
  each_pair<1>(hid, 4, [&](int r, int c, float a, float b) {
    XA[r * kLd + c] = fmaxf(a + b0[c], 0.0f), XA[(r + 32) * kLd + c] = fmaxf(b + b0[c], 0.0f);
  });
  __syncthreads();
  gemm<1>(XA, W + L.e_fc1[blk], 16, 4, hid);
  const float* b1 = W + L.e_b1[blk];
  const int lane = tid & 63;
  float top = -INFINITY;
  int col = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3), c = 32 * (tid >> 6) + (lane & 31);
    const float fold = FIRST ? 0.0f : cs[k * 128 + c];
    const float y0 = (sc[0][0][i] + fold) + (hid[0][0][i] + b1[c]), y1 = (sc[1][0][i] + fold) + (hid[1][0][i] + b1[c]);
    if (row0 + r < n) net[((int64_t)k * n + row0 + r) * 128 + c] = y0;
    if (row0 + r + 32 < n) net[((int64_t)k * n + row0 + r + 32) * 128 + c] = y1;
    top = fmaxf(top, fmaxf(y0, y1));   // a repeated row repeats a value
    col = c;
  }
  top = fmaxf(top, __shfl_xor(top, 32));
  if (lane < 32) atomicMax(&pooled_out[k * 128 + col], max_key(top));
}

// the pooled half of block `blk`'s input as per-part biases: c0 = b0 + W0[:, 128:] relu(pooled), cs = Ws[:, 128:] pooled (grid K, 128 threads)
__global__ __launch_bounds__(128) void coap_fold_kernel(CoapLayout L, int blk, const float* __restrict__ W, const unsigned* __restrict__ pooled,
                                                        float* __restrict__ c0, float* __restrict__ cs) {
  __shared__ float p[128];
  const int k = blockIdx.x, c = threadIdx.x;
  p[c] = max_value(pooled[k * 128 + c]);
  __syncthreads();
  const float* w0 = W + L.e_fc0p[blk];   // [in][out]
  const float* ws = W + L.e_scp[blk];
  float a = W[L.e_b0[blk] + c], s = 0.0f;
  for (int i = 0; i < 128; ++i) a = fmaf(w0[i * 128 + c], fmaxf(p[i], 0.0f), a), s = fmaf(ws[i * 128 + c], p[i], s);
  c0[k * 128 + c] = a, cs[k * 128 + c] = s;
}

// latent = fc_c(relu(pooled)); then the query encoder's per-part biases of layers 0 and 2 (grid K, 256 threads)
__global__ __launch_bounds__(256) void coap_latent_kernel(CoapLayout L, const float* __restrict__ W, const unsigned* __restrict__ pooled,
                                                          char* __restrict__ code, CodeLayout cl) {
  __shared__ float p[128], lat[128];
  const int k = blockIdx.x, c = threadIdx.x;
  if (c < 128) p[c] = fmaxf(max_value(pooled[k * 128 + c]), 0.0f);
  __syncthreads();
  if (c < 128) {
    const float* w = W + L.e_fcc_w;   // [in][out]
    float a = W[L.e_fcc_b + c];
    for (int i = 0; i < 128; ++i) a = fmaf(w[i * 128 + c], p[i], a);
    lat[c] = a;
    ((float*)(code + cl.latent))[k * 128 + c] = a;
    if (!__builtin_isfinite(a)) atomicOr((int*)code + 2, (int)kCoapNonFinite);
  }
  __syncthreads();
  for (int i = 0; i < 2; ++i) {
    const float* w = W + L.q_lat[i];   // [128][256]
    float a = (W[L.q_b[i] + c] + W[L.q_in[i] + c]) + W[L.q_hot[i] + k * 256 + c];
    for (int j = 0; j < 128; ++j) a = fmaf(w[j * 256 + c], lat[j], a);
    ((float*)(code + (i ? cl.bias2 : cl.bias0)))[k * 256 + c] = a;
  }
}

// ---- query ----
struct QueryLayout {
  size_t keys, list, partial, total;   // after a 16-byte header: the list's count, the kept count (8 bytes)
  int blocks;
};

static QueryLayout query_layout(int K, int T) {
  Carve c;
  c.take(16);
  QueryLayout l;
  l.keys = c.take((size_t)T * 8);
  l.list = c.take((size_t)T * K * 4);
  l.blocks = (T + 255) / 256;
  l.partial = c.take((size_t)l.blocks * 2 * sizeof(double));
  l.total = c.at;
  return l;
}

__global__ void coap_reset_query_kernel(int* __restrict__ hdr) {
  if (threadIdx.x < 4) hdr[threadIdx.x] = 0;
}

// One thread per point: zero its key; with `prefilter` drop it unless it lies in the closed box of the posed vertices (shifted by
// d f); append (point, part) for every part whose box holds x - d f.  A wave appends with one atomic per part.
__global__ __launch_bounds__(256) void coap_list_kernel(const char* __restrict__ code, CodeLayout cl, int K, const float* __restrict__ points, int T,
                                                        const double* __restrict__ dptr, D3 f, int prefilter, int* __restrict__ list,
                                                        int* __restrict__ count, unsigned long long* __restrict__ keys,
                                                        const long long* __restrict__ stop) {
  if (stop && stop[4]) return;
  const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int* hdr = (const int*)code;
  const bool good = hdr[0] == kCoapMagic && hdr[1] == K && hdr[2] == 0;
  bool live = t < T && good;
  if (t < T) keys[t] = 0ull;
  D3 x = {0.0, 0.0, 0.0};
  if (live) {
    const double d = dptr ? *dptr : 0.0;
    const D3 p = load3(points, t), s = f * d;
    if (prefilter) {
      const double* vb = (const double*)(code + cl.vbox);
      live = p.x >= vb[0] + s.x && p.y >= vb[1] + s.y && p.z >= vb[2] + s.z && p.x <= vb[3] + s.x && p.y <= vb[4] + s.y && p.z <= vb[5] + s.z;
    }
    x = p - s;
  }
  for (int k = 0; k < K; ++k) {
    bool in = false;
    if (live) {
      const double* g = (const double*)(code + cl.geo) + (int64_t)k * kGeoDoubles;
      const D3 w = x - D3{g[9], g[10], g[11]};
      in = true;
      for (int c = 0; c < 3; ++c) {
        const double q = (g[c] * w.x + g[3 + c] * w.y) + g[6 + c] * w.z;
        in = in && fabs(q - g[12 + c]) < g[15 + c];
      }
    }
    const unsigned long long mask = __ballot(in);
    if (mask == 0ull) continue;
    int base = 0;
    if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(count, __popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1);
    if (in) list[(int64_t)base + __popcll(mask & ((1ull << lane) - 1ull))] = (t << 5) | k;   // base + rank < K T: every pair is appended once
  }
}

template <bool TAN>
__global__ __launch_bounds__(256) void coap_mlp_kernel(CoapLayout L, const float* __restrict__ W, const char* __restrict__ code, CodeLayout cl,
                                                       const float* __restrict__ points, const double* __restrict__ dptr, D3 f,
                                                       const int* __restrict__ list, const int* __restrict__ count, int capacity,
                                                       unsigned long long* __restrict__ keys, const long long* __restrict__ stop) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* X = lds;                      // [64][kLd] the activations
  float* S = X + kRows * kLd;          // [64][kSd] q (3) | z (128): the decoder's input, kept for its skip connection
  int* part = (int*)(S + kRows * kSd); // [64]
  int* point = part + kRows;           // [64]
  float* fin = (float*)(point + kRows);   // [64]
  constexpr int kEnt = TAN ? 32 : 64;
  if (stop && stop[4]) return;
  const int tid = threadIdx.x;
  const int n = min(max(*count, 0), capacity);
  const double d = dptr ? *dptr : 0.0;
  const float* bias0 = (const float*)(code + cl.bias0);
  const float* bias2 = (const float*)(code + cl.bias2);
  f32x16 acc[2][2], one[2][1];

  // bias(row, col) added to value rows; softplus; tangent rows times the slope of their value row
  auto activate = [&](float a, float b, float bias_a, float bias_b, float* ha, float* hb) {
    float slope;
    *ha = softplus(a + bias_a, &slope);
    if (TAN) {
      *hb = b * slope;
    } else {
      *hb = softplus(b + bias_b, &slope);
    }
  };

  for (int tile = blockIdx.x; (long long)tile * kEnt < n; tile += gridDim.x) {
    if (tid < kRows) {
      const int e = TAN ? (tid & 31) : tid;
      const int idx = tile * kEnt + e;
      const bool live = idx < n;
      const int pk = live ? list[idx] : 0;
      const int k = pk & 31, t = pk >> 5;
      const double* g = (const double*)(code + cl.geo) + (int64_t)k * kGeoDoubles;
      D3 w = {0.0, 0.0, 0.0};
      if (TAN && tid >= 32) {
        w = D3{-f.x, -f.y, -f.z};
      } else if (live) {
        w = (load3(points, t) - f * d) - D3{g[9], g[10], g[11]};
      }
      part[tid] = k, point[tid] = live ? t : -1;
      for (int c = 0; c < 3; ++c) {
        const float q = (float)((g[c] * w.x + g[3 + c] * w.y) + g[6 + c] * w.z);
        S[tid * kSd + c] = q, X[tid * kLd + c] = q;
      }
      S[tid * kSd + 131] = 0.0f;
      for (int c = 3; c < 8; ++c) X[tid * kLd + c] = 0.0f;
    }
    __syncthreads();
    // query_encoder.lin0: q -> 256 (one-hot, inside and latent inputs are the per-part bias)
    gemm<2>(X, W + L.w[0], 1, 8, acc);
    __syncthreads();
    each_pair<2>(acc, 8, [&](int r, int c, float a, float b) {
      float ha, hb;
      activate(a, b, bias0[part[r] * 256 + c], bias0[part[r + 32] * 256 + c], &ha, &hb);
      X[r * kLd + c] = ha, X[(r + 32) * kLd + c] = hb;
    });
    __syncthreads();
    // lin1: 256 -> n1 = 124 - K; then q beside it: the skip input of lin2 (whose other columns are its per-part bias)
    gemm<1>(X, W + L.w[1], 32, L.nb1, one);
    __syncthreads();
    {
      const float* bias = W + L.b[1];
      each_pair<1>(one, L.nb1, [&](int r, int c, float a, float b) {
        float ha, hb;
        activate(a, b, bias[c], bias[c], &ha, &hb);
        if (c < L.n1) X[r * kLd + c] = ha, X[(r + 32) * kLd + c] = hb;
      });
      if (tid < kRows)
        for (int c = 0; c < 8 * L.g2 - L.n1; ++c) X[tid * kLd + L.n1 + c] = c < 3 ? S[tid * kSd + c] : 0.0f;
    }
    __syncthreads();
    gemm<2>(X, W + L.w[2], L.g2, 8, acc);
    __syncthreads();
    each_pair<2>(acc, 8, [&](int r, int c, float a, float b) {
      float ha, hb;
      activate(a, b, bias2[part[r] * 256 + c], bias2[part[r + 32] * 256 + c], &ha, &hb);
      X[r * kLd + c] = ha, X[(r + 32) * kLd + c] = hb;
    });
    __syncthreads();
    // lin3: 256 -> z (128), no activation; the decoder's input is q | z
    gemm<1>(X, W + L.w[3], 32, 4, one);
    __syncthreads();
    {
      const float* bias = W + L.b[3];
      each_pair<1>(one, 4, [&](int r, int c, float a, float b) {
        const float za = a + bias[c], zb = TAN ? b : b + bias[c];
        X[r * kLd + 3 + c] = za, X[(r + 32) * kLd + 3 + c] = zb;
        S[r * kSd + 3 + c] = za, S[(r + 32) * kSd + 3 + c] = zb;
      });
      if (tid < kRows)
        for (int c = 0; c < 8; ++c) X[tid * kLd + (c < 3 ? c : 128 + c)] = c < 3 ? S[tid * kSd + c] : 0.0f;   // q in 0 .. 2, zeros in 131 .. 135
    }
    __syncthreads();
    // decoder.lin0 .. lin5
#pragma unroll 1
    for (int layer = 4; layer < 10; ++layer) {
      const float* bias = W + L.b[layer];
      if (layer == 6) {   // 256 -> 125, then the skip input q | z beside it
        gemm<1>(X, W + L.w[6], 32, 4, one);
        __syncthreads();
        each_pair<1>(one, 4, [&](int r, int c, float a, float b) {
          float ha, hb;
          activate(a, b, bias[c], bias[c], &ha, &hb);
          if (c < 125) X[r * kLd + c] = ha, X[(r + 32) * kLd + c] = hb;
        });
        for (int i = tid; i < kRows * 131; i += 256) {
          const int r = i / 131, c = i - r * 131;
          X[r * kLd + 125 + c] = S[r * kSd + c];
        }
      } else {
        gemm<2>(X, W + L.w[layer], layer == 4 ? 17 : 32, 8, acc);
        __syncthreads();
        each_pair<2>(acc, 8, [&](int r, int c, float a, float b) {
          float ha, hb;
          activate(a, b, bias[c], bias[c], &ha, &hb);
          X[r * kLd + c] = ha, X[(r + 32) * kLd + c] = hb;
        });
      }
      __syncthreads();
    }
    // decoder.lin6: one dot per row, four threads a row over the columns 4 c + quarter, then ((p0 + p1) + (p2 + p3))
    {
      const int r = tid >> 2, quarter = tid & 3;
      const float* w6 = W + L.w6;
      float p = 0.0f;
      for (int c = 0; c < 64; ++c) p = fmaf(X[r * kLd + 4 * c + quarter], w6[4 * c + quarter], p);
      p += __shfl_xor(p, 1);
      p += __shfl_xor(p, 2);
      if (quarter == 0) fin[r] = p;
    }
    __syncthreads();
    if (tid < kEnt && point[tid] >= 0) {
      const float x = fin[tid] + W[L.b6];
      const float s = 1.0f / (1.0f + expf(x));   // sigmoid(-x)
      const float ds = TAN ? -(s * (1.0f - s)) * fin[tid + 32] : 0.0f;
      if (s > 0.0f)
        atomicMax(&keys[point[tid]], ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)__float_as_uint(ds));
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void coap_finalize_kernel(const unsigned long long* __restrict__ keys, int T, float* __restrict__ occ,
                                                            float* __restrict__ docc) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const unsigned long long key = keys[t];
  occ[t] = __uint_as_float((unsigned)(key >> 32));
  if (docc) docc[t] = __uint_as_float((unsigned)(key & 0xffffffffull));
}

// kept = occ > filter_threshold (a point the prefilter dropped has occ = 0); loss = sum relu(occ - 0.5), dloss = sum [occ > 0.5] docc
__global__ __launch_bounds__(256) void coap_partial_kernel(const unsigned long long* __restrict__ keys, int T, double filter_threshold,
                                                           double* __restrict__ partial, unsigned long long* __restrict__ kept,
                                                           const long long* __restrict__ stop) {
  __shared__ double lds[256];
  const long long stopped = stop ? stop[4] : 0;
  if (stopped) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  double loss = 0.0, grad = 0.0;
  long long keep = 0;
  if (t < T) {
    const unsigned long long key = keys[t];
    const double occ = (double)__uint_as_float((unsigned)(key >> 32));
    if (occ > filter_threshold) {
      keep = 1;
      if (occ > 0.5) loss = occ - 0.5, grad = (double)__uint_as_float((unsigned)(key & 0xffffffffull));
    }
  }
  loss = block_sum<256>(loss, lds);
  grad = block_sum<256>(grad, lds);
  keep = wave_sum(keep);
  if ((threadIdx.x & 63) == 0 && keep) atomicAdd(kept, (unsigned long long)keep);
  if (threadIdx.x == 0) partial[2 * blockIdx.x] = loss, partial[2 * blockIdx.x + 1] = grad;
}

// thread t adds the partials t, t + 256, ... in ascending order; the tree follows
__global__ __launch_bounds__(256) void coap_sum_kernel(const double* __restrict__ partial, int blocks, const unsigned long long* __restrict__ kept,
                                                       double* __restrict__ result, long long* __restrict__ kept_out,
                                                       const long long* __restrict__ stop) {
  __shared__ double lds[256];
  const long long stopped = stop ? stop[4] : 0;
  if (stopped) return;
  double loss = 0.0, grad = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) loss = loss + partial[2 * b], grad = grad + partial[2 * b + 1];
  loss = block_sum<256>(loss, lds);
  grad = block_sum<256>(grad, lds);
  if (threadIdx.x == 0) {
    result[0] = loss, result[1] = grad;
    if (kept_out) *kept_out = (long long)*kept;
  }
}

static LdsOptIn opt_block[2], opt_mlp[2];
constexpr size_t kBlockLds = (size_t)2 * kRows * kLd * sizeof(float);
constexpr size_t kMlpLds = ((size_t)kRows * kLd + (size_t)kRows * kSd + 3 * kRows) * sizeof(float);

static int domain_ok(int K) { return K >= 1 && K <= kCoapMaxParts; }

static int query_launches(const float* weights, const char* code, int K, const float* points, int T, const double* d, D3 f, int derivative,
                          int prefilter, char* ws, const QueryLayout& ql, const long long* stop, hipStream_t st) {
  const CoapLayout L = coap_layout(K);
  const CodeLayout cl = code_layout(K);
  int* hdr = (int*)ws;
  int* list = (int*)(ws + ql.list);
  unsigned long long* keys = (unsigned long long*)(ws + ql.keys);
  hipLaunchKernelGGL(coap_reset_query_kernel, dim3(1), dim3(64), 0, st, hdr);
  if (int rc = check_launch("coap_reset_query_kernel")) return rc;
  hipLaunchKernelGGL(coap_list_kernel, dim3((unsigned)ql.blocks), dim3(256), 0, st, code, cl, K, points, T, d, f, prefilter, list, hdr, keys, stop);
  if (int rc = check_launch("coap_list_kernel")) return rc;
  const int capacity = K * T;
  const int ent = derivative ? 32 : 64;
  const int tiles = (capacity + ent - 1) / ent;
  const unsigned grid = (unsigned)(tiles < kMlpMaxBlocks ? tiles : kMlpMaxBlocks);
  if (derivative) {
    if (int rc = opt_in_lds(opt_mlp[1], (const void*)coap_mlp_kernel<true>, kMlpLds, "coma_coap_query_f32")) return rc;
    hipLaunchKernelGGL(coap_mlp_kernel<true>, dim3(grid), dim3(256), kMlpLds, st, L, weights, code, cl, points, d, f, (const int*)list, (const int*)hdr,
                       capacity, keys, stop);
  } else {
    if (int rc = opt_in_lds(opt_mlp[0], (const void*)coap_mlp_kernel<false>, kMlpLds, "coma_coap_query_f32")) return rc;
    hipLaunchKernelGGL(coap_mlp_kernel<false>, dim3(grid), dim3(256), kMlpLds, st, L, weights, code, cl, points, d, f, (const int*)list, (const int*)hdr,
                       capacity, keys, stop);
  }
  return check_launch("coap_mlp_kernel");
}

static int front_ok(const float* front) {
  return front && __builtin_isfinite(front[0]) && __builtin_isfinite(front[1]) && __builtin_isfinite(front[2]);
}

size_t coap_weights_floats(int K) { return (size_t)coap_layout(K).total; }

int coap_collision_check(const char* who, const float* weights, const void* code, int K, const float* points, int T, const double* front,
                         double filter_threshold, const void* workspace, size_t workspace_bytes) {
  if (!weights || !code || !points || !workspace) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!domain_ok(K) || T < 1 || T > kCoapMaxPoints) return fail(COMA_E_INVALID, "%s: K=%d outside [1, %d] or T=%d outside [1, %d]", who, K, kCoapMaxParts, T, kCoapMaxPoints);
  if (!front || !__builtin_isfinite(front[0]) || !__builtin_isfinite(front[1]) || !__builtin_isfinite(front[2]))
    return fail(COMA_E_INVALID, "%s: front must be three finite numbers", who);
  if (!(filter_threshold >= 0.0) || !(filter_threshold < 1.0)) return fail(COMA_E_INVALID, "%s: filter_threshold=%g outside [0, 1)", who, filter_threshold);
  if (!f32_aligned({weights, points}) || ((uintptr_t)code & 15)) return fail(COMA_E_INVALID, "%s: weights and points 4-byte, the code block 16-byte aligned", who);
  return check_buffer(who, "workspace", workspace, workspace_bytes, query_layout(K, T).total);
}

int coap_collision_launch(const float* weights, const void* code, int K, const float* points, int T, const double* d, const double* front,
                          double filter_threshold, double* result, long long* kept, void* workspace, const long long* stop, hipStream_t st) {
  const QueryLayout ql = query_layout(K, T);
  char* ws = (char*)workspace;
  const D3 f = {front[0], front[1], front[2]};
  if (int rc = query_launches(weights, (const char*)code, K, points, T, d, f, 1, 1, ws, ql, stop, st)) return rc;
  unsigned long long* keep = (unsigned long long*)(ws + 8);
  hipLaunchKernelGGL(coap_partial_kernel, dim3((unsigned)ql.blocks), dim3(256), 0, st, (const unsigned long long*)(ws + ql.keys), T, filter_threshold,
                     (double*)(ws + ql.partial), keep, stop);
  if (int rc = check_launch("coap_partial_kernel")) return rc;
  hipLaunchKernelGGL(coap_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)(ws + ql.partial), ql.blocks, (const unsigned long long*)keep, result, kept,
                     stop);
  return check_launch("coap_sum_kernel");
}

struct EncodeLayout {
  size_t pooled, c0, cs, net, total;
};

static EncodeLayout encode_layout(int K, int n) {
  Carve c;
  EncodeLayout l;
  l.pooled = c.take((size_t)4 * K * 128 * sizeof(unsigned));
  l.c0 = c.take((size_t)K * 128 * sizeof(float));
  l.cs = c.take((size_t)K * 128 * sizeof(float));
  l.net = c.take((size_t)K * n * 128 * sizeof(float));
  l.total = c.at;
  return l;
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_coap_weights_floats(int K) { return domain_ok(K) ? (size_t)coap_layout(K).total : 0; }

extern "C" size_t coma_coap_code_bytes(int K) { return domain_ok(K) ? code_layout(K).total : 0; }

extern "C" size_t coma_coap_encode_workspace_bytes(int K, int n_samples) {
  if (!domain_ok(K) || n_samples < 2 || n_samples > kCoapMaxSamples) return 0;
  return encode_layout(K, n_samples).total;
}

extern "C" size_t coma_coap_query_workspace_bytes(int K, int T) {
  if (!domain_ok(K) || T < 1 || T > kCoapMaxPoints) return 0;
  return query_layout(K, T).total;
}

extern "C" int coma_coap_encode_f32(const float* weights, size_t weights_floats, const float* full_pose, const float* joints, const float* vertices,
                                    int V, const int32_t* parents, const uint8_t* joint_mapper, int mK, int K, const int32_t* selector, int S,
                                    const int32_t* sample_ids, const float* sample_bary, int n_samples, void* code, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "coma_coap_encode_f32";
  if (!weights || !full_pose || !joints || !vertices || !parents || !joint_mapper || !selector || !sample_ids || !sample_bary || !code || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!domain_ok(K) || mK < K || mK > kCoapMaxJoints) return fail(COMA_E_INVALID, "%s: K=%d outside [1, %d] or mK=%d outside [K, %d]", who, K, kCoapMaxParts, mK, kCoapMaxJoints);
  if (n_samples < 2 || n_samples > kCoapMaxSamples) return fail(COMA_E_INVALID, "%s: n_samples=%d outside [2, %d]", who, n_samples, kCoapMaxSamples);
  if (V < 1 || V > kCoapMaxVerts || S < 1 || S > V) return fail(COMA_E_INVALID, "%s: V=%d outside [1, %d] or S=%d outside [1, V]", who, V, kCoapMaxVerts, S);
  if (weights_floats < (size_t)coap_layout(K).total)
    return fail(COMA_E_INVALID, "%s: weights of %zu floats, %lld needed", who, weights_floats, coap_layout(K).total);
  CoapTree tree = {};
  tree.mK = mK, tree.K = K;
  int parts = 0;
  for (int i = 0; i < mK; ++i) {
    if (i > 0 && (parents[i] < 0 || parents[i] >= i)) return fail(COMA_E_INVALID, "%s: parents[%d]=%d outside [0, %d)", who, i, parents[i], i);
    tree.parents[i] = i ? parents[i] : 0;
    if (joint_mapper[i]) {
      if (parts < K) tree.mapped[parts] = i;
      ++parts;
    }
  }
  if (parts != K) return fail(COMA_E_INVALID, "%s: joint_mapper selects %d joints, K=%d", who, parts, K);
  if (!f32_aligned({weights, full_pose, joints, vertices, selector, sample_ids, sample_bary}) || ((uintptr_t)weights & 15))
    return fail(COMA_E_INVALID, "%s: arrays 4-byte, the weights 16-byte aligned", who);
  if (((uintptr_t)code & 15)) return fail(COMA_E_INVALID, "%s: the code block must be 16-byte aligned", who);
  const EncodeLayout el = encode_layout(K, n_samples);
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, el.total)) return rc;
  const CoapLayout L = coap_layout(K);
  const CodeLayout cl = code_layout(K);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  char* cd = (char*)code;
  unsigned* pooled = (unsigned*)(ws + el.pooled);
  float* c0 = (float*)(ws + el.c0);
  float* cs = (float*)(ws + el.cs);
  float* net = (float*)(ws + el.net);
  const int cells = 4 * K * 128;
  hipLaunchKernelGGL(coap_reset_encode_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (int*)cd, K, pooled, cells);
  if (int rc = check_launch("coap_reset_encode_kernel")) return rc;
  hipLaunchKernelGGL(coap_geometry_kernel, dim3((unsigned)(K + 1)), dim3(256), 0, st, tree, full_pose, joints, vertices, V, (const int*)selector, S, cd, cl);
  if (int rc = check_launch("coap_geometry_kernel")) return rc;
  if (int rc = opt_in_lds(opt_block[0], (const void*)coap_block_kernel<true>, kBlockLds, who)) return rc;
  if (int rc = opt_in_lds(opt_block[1], (const void*)coap_block_kernel<false>, kBlockLds, who)) return rc;
  const dim3 grid((unsigned)((n_samples + kRows - 1) / kRows), (unsigned)K);
  hipLaunchKernelGGL(coap_block_kernel<true>, grid, dim3(256), kBlockLds, st, L, 0, weights, vertices, V, (const int*)sample_ids, sample_bary, n_samples, cd,
                     cl, (const float*)c0, (const float*)cs, net, pooled);
  if (int rc = check_launch("coap_block_kernel")) return rc;
  for (int blk = 1; blk < 4; ++blk) {
    hipLaunchKernelGGL(coap_fold_kernel, dim3((unsigned)K), dim3(128), 0, st, L, blk, weights, (const unsigned*)(pooled + (size_t)(blk - 1) * K * 128), c0, cs);
    if (int rc = check_launch("coap_fold_kernel")) return rc;
    hipLaunchKernelGGL(coap_block_kernel<false>, grid, dim3(256), kBlockLds, st, L, blk, weights, vertices, V, (const int*)sample_ids, sample_bary, n_samples,
                       cd, cl, (const float*)c0, (const float*)cs, net, pooled + (size_t)blk * K * 128);
    if (int rc = check_launch("coap_block_kernel")) return rc;
  }
  hipLaunchKernelGGL(coap_latent_kernel, dim3((unsigned)K), dim3(256), 0, st, L, weights, (const unsigned*)(pooled + (size_t)3 * K * 128), cd, cl);
  return check_launch("coap_latent_kernel");
}

extern "C" int coma_coap_status(const void* code, void* stream) {
  if (!code) return fail(COMA_E_INVALID, "coma_coap_status: null pointer");
  int hdr[4] = {0, 0, 0, 0};
  if (int rc = read_back(hdr, code, sizeof(hdr), stream, "coma_coap_status")) return rc;
  if (hdr[0] != kCoapMagic) return fail(COMA_E_INVALID, "coma_coap_status: not a code block of coma_coap_encode_f32");
  if (hdr[2] & kCoapBadIndex) return fail(COMA_E_INVALID, "coma_coap_encode_f32: a vertex id of the selector or of the sample table lies outside [0, V)");
  if (hdr[2] & kCoapNonFinite) return fail(COMA_E_INVALID, "coma_coap_encode_f32: non-finite vertex, joint, pose or latent code");
  return COMA_OK;
}

extern "C" int coma_coap_query_f32(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T, const double* d,
                                   const float* front, int derivative, float* occ, float* docc, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* who = "coma_coap_query_f32";
  if (!weights || !code || !points || !occ || !workspace) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!domain_ok(K) || T < 1 || T > kCoapMaxPoints) return fail(COMA_E_INVALID, "%s: K=%d outside [1, %d] or T=%d outside [1, %d]", who, K, kCoapMaxParts, T, kCoapMaxPoints);
  if ((d || derivative) && !front_ok(front)) return fail(COMA_E_INVALID, "%s: front (three finite numbers) is read with d or with the derivative", who);
  if (derivative && !docc) return fail(COMA_E_INVALID, "%s: docc is written with the derivative", who);
  if (weights_floats < (size_t)coap_layout(K).total)
    return fail(COMA_E_INVALID, "%s: weights of %zu floats, %lld needed", who, weights_floats, coap_layout(K).total);
  if (!f32_aligned({weights, points, occ, docc}) || ((uintptr_t)weights & 15) || ((uintptr_t)code & 15) || ((uintptr_t)d & 7))
    return fail(COMA_E_INVALID, "%s: arrays 4-byte, d 8-byte, the weights and the code block 16-byte aligned", who);
  const QueryLayout ql = query_layout(K, T);
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, ql.total)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const D3 f = front ? D3{(double)front[0], (double)front[1], (double)front[2]} : D3{0.0, 0.0, 0.0};
  if (int rc = query_launches(weights, (const char*)code, K, points, T, d, f, derivative ? 1 : 0, 0, (char*)workspace, ql, nullptr, st)) return rc;
  hipLaunchKernelGGL(coap_finalize_kernel, dim3((unsigned)ql.blocks), dim3(256), 0, st, (const unsigned long long*)((char*)workspace + ql.keys), T, occ,
                     derivative ? docc : nullptr);
  return check_launch("coap_finalize_kernel");
}

extern "C" int coma_coap_collision_f32(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T, const double* d,
                                       const float* front, double filter_threshold, double* result, int64_t* kept, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  const char* who = "coma_coap_collision_f32";
  if (!result || !front) return fail(COMA_E_INVALID, "%s: null pointer", who);
  const double f[3] = {(double)front[0], (double)front[1], (double)front[2]};
  if (int rc = coap_collision_check(who, weights, code, K, points, T, f, filter_threshold, workspace, workspace_bytes)) return rc;
  if (weights_floats < (size_t)coap_layout(K).total)
    return fail(COMA_E_INVALID, "%s: weights of %zu floats, %lld needed", who, weights_floats, coap_layout(K).total);
  if (((uintptr_t)weights & 15) || ((uintptr_t)d & 7) || ((uintptr_t)result & 7) || ((uintptr_t)kept & 7))
    return fail(COMA_E_INVALID, "%s: d, result and kept 8-byte, the weights 16-byte aligned", who);
  return coap_collision_launch(weights, code, K, points, T, d, f, filter_threshold, result, (long long*)kept, workspace, nullptr, (hipStream_t)stream);
}
