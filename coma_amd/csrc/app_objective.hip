// The optimisation app's ComA objective (orientation term + contact term) and its analytic gradient with respect to the posed
// vertices, for gfx950.  replaces: src/application/optimize.py:274-289 and :295-296 of the reference -- about sixty eager torch
// launches per iteration (forward and backward), a [V,O,3] canonicalisation of which one column is used, and two k x k cdist
// matrices -- by seven small launches and one memset on the caller's stream.  Rule set: include/coma_hip.h; restated in f64 in
// tests/app_ref.py.
//
// Everything per vertex runs in f64 on f32 inputs (V = 10 475: the work is latency-bound, the f64 rate does not show), so the
// results are the f32 rounding of the rule set.  The only part with real arithmetic, the k x k double minimum, is f32 and tiled
// through LDS: one wave owns 64 rows, a split of the columns is staged 64 points at a time, and the per-split (min, argmin) pairs
// are merged in ascending split order, so the first minimum wins whatever the split.  No floating-point atomics: the normal
// gradient returns to the vertices by a gather over the vertex->face CSR table, the contact term's second direction by a scan in
// ascending j, and the two term sums by per-workgroup trees whose partials a single workgroup adds in block order.
//
// One kernel set for N bodies (coma_app_objective_batch_f32; coma_app_objective_f32 is N = 1): the last grid dimension is the body,
// a workgroup moves its per-body pointers (vertices, gradients, every scratch array) to its body once and then runs the single
// body's code, so body n has the single call's bits.  Topology, orientation targets, M, the selection and the targets are shared.
#include "coma_device.h"
#include "fit_stages.h"

#include <cmath>

namespace coma {
namespace {

constexpr int kRowTile = 64;      // rows per workgroup (one wave) and points per LDS stage of the double minimum
constexpr int kBlock = 256;       // every other kernel
constexpr int kMinGrid = 1024;    // workgroups the double minimum aims for (256 CUs x 4 SIMDs, one wave each)

// the per-body arrays of a workgroup whose body is n (the vertex kernels: blockIdx.y, gridDim.x = ceil(V / 256))
__device__ __forceinline__ void to_body(AppArgs& A, int n) {
  A.verts += (int64_t)n * A.V * 3;
  A.gN += (int64_t)n * A.V * 3;
  A.part_o += (int64_t)n * gridDim.x;
}

// one incident face of a vertex: its three indices, or false when the table points outside the mesh
__device__ __forceinline__ bool face_of(const AppArgs& A, int e, int& i0, int& i1, int& i2) {
  const int f = A.vf[e];
  if (f < 0 || f >= A.F) return false;
  i0 = A.faces[3 * f]; i1 = A.faces[3 * f + 1]; i2 = A.faces[3 * f + 2];
  return i0 >= 0 && i0 < A.V && i1 >= 0 && i1 < A.V && i2 >= 0 && i2 < A.V;
}

// K1: per vertex the normal sum, the three normalisations, f = M a, the vertex's share of the orientation term and g_h = d term / d N_h
__global__ __launch_bounds__(kBlock) void app_vertex_kernel(AppArgs A) {
  __shared__ double lds[kBlock];
  to_body(A, blockIdx.y);
  const int h = blockIdx.x * kBlock + threadIdx.x;
  double t = 0.0;
  if (h < A.V) {
    D3 N = {0.0, 0.0, 0.0}, g = {0.0, 0.0, 0.0};
    bool ok = true;
    const int e0 = max(A.off[h], 0), e1 = min(A.off[h + 1], 3 * A.F);
    for (int e = e0; e < e1; ++e) {
      int i0, i1, i2;
      if (!face_of(A, e, i0, i1, i2)) { ok = false; break; }
      const D3 v0 = load3(A.verts, i0);
      N = N + cross(load3(A.verts, i1) - v0, load3(A.verts, i2) - v0);
    }
    const double n0 = norm(N);
    if (!ok) {
      t = NAN;                                         // a table that leaves the mesh poisons the term, it is not followed
    } else if (n0 > 0.0) {
      const double m = fmax(n0, 1e-6);                 // F.normalize(eps=1e-6)
      const D3 n1 = N * (1.0 / m);
      const double r1 = norm(n1), s1 = r1 + A.eps;
      const D3 n2 = n1 / s1;
      const double r2 = norm(n2), s2 = r2 + A.eps;
      const D3 a = n2 / s2;
      const D3 f = {(A.M[0] * a.x + A.M[1] * a.y) + A.M[2] * a.z, (A.M[3] * a.x + A.M[4] * a.y) + A.M[5] * a.z,
                    (A.M[6] * a.x + A.M[7] * a.y) + A.M[8] * a.z};
      const double rf = norm(f);
      const D3 fh = f / rf;
      const D3 gt = load3(A.gt, h);
      t = 1.0 - (dot(gt, fh) + 1.0) / 2.0;
      if (t != t) {
        t = 0.0;                                       // nan_to_num; no gradient either
      } else {
        const D3 gfh = gt * (-0.5 / (double)A.V);
        const D3 gf = (gfh - fh * dot(gfh, fh)) * (1.0 / rf);
        const D3 ga = {(A.M[0] * gf.x + A.M[3] * gf.y) + A.M[6] * gf.z, (A.M[1] * gf.x + A.M[4] * gf.y) + A.M[7] * gf.z,
                       (A.M[2] * gf.x + A.M[5] * gf.y) + A.M[8] * gf.z};
        const D3 gn2 = ga * (1.0 / s2) - n2 * (dot(ga, n2) / (r2 * s2 * s2));
        const D3 gn1 = gn2 * (1.0 / s1) - n1 * (dot(gn2, n1) / (r1 * s1 * s1));
        if (n0 >= 1e-6) {
          const D3 nh = N * (1.0 / n0);
          g = (gn1 - nh * dot(gn1, nh)) * (1.0 / n0);
        } else {
          g = gn1 * 1e6;
        }
      }
    }
    A.gN[3 * (int64_t)h] = g.x; A.gN[3 * (int64_t)h + 1] = g.y; A.gN[3 * (int64_t)h + 2] = g.z;
  }
  const double s = block_sum<kBlock>(t, lds);
  if (threadIdx.x == 0) A.part_o[blockIdx.x] = s;
}

// K2: the normal gradient back to the vertices, a gather: per incident face G = g_f0 + g_f1 + g_f2, then the derivative of
// (v1 - v0) x (v2 - v0) with respect to the slot this vertex holds in the face
__global__ __launch_bounds__(kBlock) void app_face_gather_kernel(AppArgs A, float* __restrict__ grad) {
  const int h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= A.V) return;
  to_body(A, blockIdx.y);
  grad += (int64_t)blockIdx.y * A.V * 3;
  D3 acc = {0.0, 0.0, 0.0};
  const int e0 = max(A.off[h], 0), e1 = min(A.off[h + 1], 3 * A.F);
  for (int e = e0; e < e1; ++e) {
    if (e > e0 && A.vf[e] == A.vf[e - 1]) continue;     // a face that names this vertex twice is listed twice: taken once
    int i0, i1, i2;
    if (!face_of(A, e, i0, i1, i2)) { acc = {NAN, NAN, NAN}; break; }
    const D3 G = (load3(A.gN, i0) + load3(A.gN, i1)) + load3(A.gN, i2);
    const D3 v0 = load3(A.verts, i0);
    const D3 d1 = cross(load3(A.verts, i2) - v0, G);     // d / d v1
    const D3 d2 = cross(G, load3(A.verts, i1) - v0);     // d / d v2
    if (h == i0) acc = acc - (d1 + d2);
    if (h == i1) acc = acc + d1;
    if (h == i2) acc = acc + d2;
  }
  grad[3 * (int64_t)h] = (float)acc.x; grad[3 * (int64_t)h + 1] = (float)acc.y; grad[3 * (int64_t)h + 2] = (float)acc.z;
}

// a point of one side of the contact term: row t of `base`, or row idx[t] when the side is a selection; a row outside [0, rows)
// is not followed and reads as NaN (it then never wins a minimum)
__device__ __forceinline__ bool point_row(const int32_t* idx, int t, int rows, int& r) {
  r = idx ? idx[t] : t;
  return r >= 0 && r < rows;
}

// K3 (run twice, sides swapped): for 64 rows of P the minimum and first argmin of sqrt((dx^2 + dy^2) + dz^2) over one split of Q.
// Body blockIdx.z: the side that is the vertices moves by its stride (the targets' stride is 0), the results by out_stride.
__global__ __launch_bounds__(kRowTile) void app_rowmin_kernel(const float* __restrict__ P, const int32_t* __restrict__ idxP, int rowsP,
                                                             int64_t strideP, const float* __restrict__ Q, const int32_t* __restrict__ idxQ,
                                                             int rowsQ, int64_t strideQ, int k, int chunk, float* __restrict__ pmin,
                                                             int32_t* __restrict__ parg, int64_t out_stride) {
  __shared__ float4 tile[kRowTile];
  const int lane = threadIdx.x;
  P += blockIdx.z * strideP; Q += blockIdx.z * strideQ;
  pmin += blockIdx.z * out_stride; parg += blockIdx.z * out_stride;
  const int i = blockIdx.x * kRowTile + lane;
  const int split = blockIdx.y;
  float px = NAN, py = NAN, pz = NAN;
  int r;
  if (i < k && point_row(idxP, i, rowsP, r)) { px = P[3 * (int64_t)r]; py = P[3 * (int64_t)r + 1]; pz = P[3 * (int64_t)r + 2]; }
  float best = INFINITY;
  int arg = -1;
  const int jbeg = split * chunk * kRowTile, jend = min(k, jbeg + chunk * kRowTile);
  for (int j0 = jbeg; j0 < jend; j0 += kRowTile) {
    const int j = j0 + lane;
    float4 q = {NAN, NAN, NAN, 0.0f};
    if (j < jend && point_row(idxQ, j, rowsQ, r)) q = {Q[3 * (int64_t)r], Q[3 * (int64_t)r + 1], Q[3 * (int64_t)r + 2], 0.0f};
    __syncthreads();
    tile[lane] = q;
    __syncthreads();
    const int n = min(kRowTile, jend - j0);
    for (int jj = 0; jj < n; ++jj) {
      const float4 c = tile[jj];
      const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      if (d < best) { best = d; arg = j0 + jj; }
    }
  }
  if (i < k) {
    pmin[(int64_t)split * k + i] = best;
    parg[(int64_t)split * k + i] = arg;
  }
}

// the per-body arrays of a workgroup whose body is n (the contact kernels: blockIdx.y, gridDim.x = ceil(k / 256))
__device__ __forceinline__ void to_body(ContactArgs& C, int n) {
  C.verts += (int64_t)n * C.V * 3;
  C.pmin += (int64_t)n * 2 * C.nsplit * C.k;
  C.parg += (int64_t)n * 2 * C.nsplit * C.k;
  C.dist += (int64_t)n * 2 * C.k;
  C.arg += (int64_t)n * 2 * C.k;
  C.part_c += (int64_t)n * 2 * gridDim.x;
}

__device__ __forceinline__ D3 point_a(const ContactArgs& C, int i) {
  int r;
  return point_row(C.sel, i, C.V, r) ? load3(C.verts, r) : D3{NAN, NAN, NAN};
}

// K4: merge the splits in ascending order (first minimum wins), take the winning distance again in f64, partial sums of both directions
__global__ __launch_bounds__(kBlock) void app_contact_merge_kernel(ContactArgs C) {
  __shared__ double lds[kBlock];
  to_body(C, blockIdx.y);
  const int t = blockIdx.x * kBlock + threadIdx.x;
  double d[2] = {0.0, 0.0};
  if (t < C.k) {
    for (int dir = 0; dir < 2; ++dir) {
      float best = INFINITY;
      int arg = -1;
      for (int s = 0; s < C.nsplit; ++s) {
        const int64_t at = ((int64_t)dir * C.nsplit + s) * C.k + t;
        if (C.pmin[at] < best) { best = C.pmin[at]; arg = C.parg[at]; }
      }
      double dd = NAN;                                  // no finite distance in the row: the term is NaN
      if (arg >= 0) {
        const D3 a = point_a(C, dir == 0 ? t : arg), b = load3(C.targets, dir == 0 ? arg : t);
        const D3 df = a - b;
        dd = norm(df);
      }
      d[dir] = dd;
      C.dist[(int64_t)dir * C.k + t] = dd;
      C.arg[(int64_t)dir * C.k + t] = arg;
    }
  }
  const int nb = gridDim.x;
  const double s0 = block_sum<kBlock>(d[0], lds);
  const double s1 = block_sum<kBlock>(d[1], lds);
  if (threadIdx.x == 0) { C.part_c[blockIdx.x] = s0; C.part_c[nb + blockIdx.x] = s1; }
}

// K5: contact gradient of selected row i: its own nearest target, then every target j (ascending) whose nearest selected row is i
__global__ __launch_bounds__(kBlock) void app_contact_grad_kernel(ContactArgs C, float* __restrict__ grad) {
  __shared__ int32_t owner[kBlock];
  to_body(C, blockIdx.y);
  grad += (int64_t)blockIdx.y * C.V * 3;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < C.k;
  D3 a = {0.0, 0.0, 0.0}, g = {0.0, 0.0, 0.0};
  if (live) {
    a = point_a(C, i);
    const int j = C.arg[i];
    const double d = C.dist[i];
    if (j < 0) g = {NAN, NAN, NAN};
    else if (d > 0.0) g = (a - load3(C.targets, j)) * (1.0 / d);      // a zero distance has zero gradient
  }
  for (int j0 = 0; j0 < C.k; j0 += kBlock) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    owner[threadIdx.x] = j < C.k ? C.arg[C.k + j] : -1;
    __syncthreads();
    if (!live) continue;
    const int n = min(kBlock, C.k - j0);
    for (int jj = 0; jj < n; ++jj) {
      if (owner[jj] != i) continue;
      const double d = C.dist[C.k + j0 + jj];
      if (d > 0.0) g = g + (a - load3(C.targets, j0 + jj)) * (1.0 / d);
    }
  }
  int r;
  if (live && point_row(C.sel, i, C.V, r)) {
    const double s = 1.0 / (double)C.k;
    grad[3 * (int64_t)r] = (float)(g.x * s); grad[3 * (int64_t)r + 1] = (float)(g.y * s); grad[3 * (int64_t)r + 2] = (float)(g.z * s);
  }
}

// K6, one workgroup per body: the partials in block order (thread t adds t, t + 256, ...; then the tree), the means, the two terms
__global__ __launch_bounds__(kBlock) void app_finalize_kernel(const double* __restrict__ part_o, int nb_o, int V,
                                                             const double* __restrict__ part_c, int nb_c, int k, float* __restrict__ terms) {
  __shared__ double lds[kBlock];
  part_o += (int64_t)blockIdx.x * nb_o; part_c += (int64_t)blockIdx.x * 2 * nb_c; terms += (int64_t)blockIdx.x * 2;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb_o; b += kBlock) s[0] = s[0] + part_o[b];
  for (int b = threadIdx.x; b < nb_c; b += kBlock) { s[1] = s[1] + part_c[b]; s[2] = s[2] + part_c[nb_c + b]; }
  double r[3];
  for (int q = 0; q < 3; ++q) r[q] = block_sum<kBlock>(s[q], lds);
  if (threadIdx.x == 0) {
    terms[0] = (float)(r[0] / (double)V);
    terms[1] = k > 0 ? (float)(r[1] / (double)k + r[2] / (double)k) : 0.0f;
  }
}

struct Layout {
  size_t gN, part_o, part_c, dist, arg, pmin, parg, total;
  int nb_v, nb_k, row_blocks, chunk, nsplit;
};

// the scratch of N bodies: every array is [N] of the single body's, so N = 1 is the single-body layout
Layout layout(int V, int k, int N = 1) {
  Layout L = {};
  L.nb_v = (V + kBlock - 1) / kBlock;
  L.nb_k = (k + kBlock - 1) / kBlock;
  L.row_blocks = (k + kRowTile - 1) / kRowTile;
  if (k > 0) {
    int want = kMinGrid / (L.row_blocks * N);           // splits of the columns, so that small k still fills the device; N bodies
                                                        // fill it N times sooner (the merge does not depend on the split)
    if (want < 1) want = 1;
    if (want > L.row_blocks) want = L.row_blocks;
    L.chunk = (L.row_blocks + want - 1) / want;         // column tiles per split
    L.nsplit = (L.row_blocks + L.chunk - 1) / L.chunk;  // no split is empty
  }
  Carve ws;
  L.gN = ws.take((size_t)N * V * 3 * sizeof(double));
  L.part_o = ws.take((size_t)N * L.nb_v * sizeof(double));
  L.part_c = ws.take((size_t)N * 2 * L.nb_k * sizeof(double));
  L.dist = ws.take((size_t)N * 2 * k * sizeof(double));
  L.arg = ws.take((size_t)N * 2 * k * sizeof(int32_t));
  L.pmin = ws.take((size_t)N * 2 * L.nsplit * k * sizeof(float));
  L.parg = ws.take((size_t)N * 2 * L.nsplit * k * sizeof(int32_t));
  L.total = ws.at;
  return L;
}

void unit_host(const float* v, double eps, double* out) {   // utils/transformations.py:14-17, in f64 on the f32 inputs
  const double x = v[0], y = v[1], z = v[2];
  const double n = std::sqrt((x * x + y * y) + z * z) + eps;
  out[0] = x / n; out[1] = y / n; out[2] = z / n;
}

constexpr int kMaxBatch = 1024;   // N: bodies per call, the body model's bound

bool sizes_ok(int V, int F, int k, int N) { return V > 0 && F > 0 && k >= 0 && k <= V && N >= 1 && N <= kMaxBatch; }

}  // namespace

// both entry points: the refusals in one order, M, and the arguments of one body's launches
int app_objective_plan(const char* who, bool batched, int N, const float* verts, const int32_t* faces, const int32_t* vf_offsets,
                       const int32_t* vf_faces, int V, int F, const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                       const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k, float* terms,
                       float* grad_orientation, float* grad_contact, void* workspace, size_t workspace_bytes, AppObjectivePlan& p) {
  if (!verts || !faces || !vf_offsets || !vf_faces || !orientation_gt || !obj_normal || !principle_vec || !sub_principle_vec || !terms ||
      !grad_orientation || !grad_contact || !workspace)
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (V <= 0 || F <= 0 || F > INT32_MAX / 3) return fail(COMA_E_INVALID, "%s: bad sizes V=%d F=%d", who, V, F);
  if (k < 0 || k > V) return fail(COMA_E_INVALID, "%s: k=%d outside [0, V=%d]", who, k, V);
  if (k > 0 && (!selected || !targets)) return fail(COMA_E_INVALID, "%s: null pointer (selected / targets with k > 0)", who);
  if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(COMA_E_INVALID, "%s: eps must be finite and >= 0", who);
  if (batched && (N < 1 || N > kMaxBatch)) return fail(COMA_E_INVALID, "%s: N=%d outside [1, %d]", who, N, kMaxBatch);
  const Layout L = layout(V, k, N);
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;

  // the canonicalisation of one column b is linear in the normalised vertex normal: f = M a
  double b[3], pv[3], s[3];
  unit_host(obj_normal, eps, b);
  unit_host(principle_vec, eps, pv);
  unit_host(sub_principle_vec, eps, s);
  const double ps = (pv[0] * s[0] + pv[1] * s[1]) + pv[2] * s[2];
  if (!(std::fabs(ps) <= 1e-8)) return fail(COMA_E_INVALID, "%s: principle_vec and sub_principle_vec are not orthogonal", who);
  const double bp = (b[0] * pv[0] + b[1] * pv[1]) + b[2] * pv[2];
  p = {};
  AppArgs& A = p.vertex;
  if (1.0 + bp < eps) {                                 // b opposite to p: 2 (a.s) s - a
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A.M[3 * i + j] = 2.0 * s[i] * s[j] - (i == j ? 1.0 : 0.0);
  } else {
    // the reference's b_cross as written: [0][0] = b0 is set and [2][1] = b0 is not
    const double c[3] = {(b[0] * pv[0] - b[2] * pv[1]) + b[1] * pv[2], b[2] * pv[0] - b[0] * pv[2], -b[1] * pv[0]};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        A.M[3 * i + j] = c[i] * c[j] / (1.0 + bp) + (i == j ? bp : 0.0) + pv[i] * b[j] - b[i] * pv[j];
  }
  char* ws = (char*)workspace;
  A.verts = verts; A.faces = faces; A.off = vf_offsets; A.vf = vf_faces; A.gt = orientation_gt; A.V = V; A.F = F; A.eps = eps;
  A.gN = (double*)(ws + L.gN); A.part_o = (double*)(ws + L.part_o);
  p.who = who; p.N = N; p.nb_v = L.nb_v; p.nb_k = L.nb_k; p.row_blocks = L.row_blocks; p.chunk = L.chunk;
  p.pmin = (float*)(ws + L.pmin); p.parg = (int32_t*)(ws + L.parg);
  p.terms = terms; p.grad_orientation = grad_orientation; p.grad_contact = grad_contact;
  ContactArgs& C = p.contact;
  C.verts = verts; C.sel = selected; C.targets = targets; C.V = V; C.k = k; C.nsplit = L.nsplit;
  C.pmin = p.pmin; C.parg = p.parg; C.dist = (double*)(ws + L.dist); C.arg = (int32_t*)(ws + L.arg); C.part_c = (double*)(ws + L.part_c);
  return COMA_OK;
}

// the launches of one body over a grid that has the bodies as its last dimension
int app_objective_enqueue(const AppObjectivePlan& p, hipStream_t st) {
  const AppArgs& A = p.vertex;
  const ContactArgs& C = p.contact;
  const int N = p.N, V = A.V, k = C.k;
  if (hipMemsetAsync(p.grad_contact, 0, (size_t)N * V * 3 * sizeof(float), st) != hipSuccess) return fail(COMA_E_LAUNCH, "%s: memset failed", p.who);
  hipLaunchKernelGGL(app_vertex_kernel, dim3(p.nb_v, N), dim3(kBlock), 0, st, A);
  hipLaunchKernelGGL(app_face_gather_kernel, dim3(p.nb_v, N), dim3(kBlock), 0, st, A, p.grad_orientation);
  if (k > 0) {
    const dim3 grid(p.row_blocks, C.nsplit, N);
    const int64_t half = (int64_t)C.nsplit * k, body = (int64_t)V * 3;
    hipLaunchKernelGGL(app_rowmin_kernel, grid, dim3(kRowTile), 0, st, C.verts, C.sel, V, body, C.targets, (const int32_t*)nullptr, k, (int64_t)0,
                       k, p.chunk, p.pmin, p.parg, 2 * half);
    hipLaunchKernelGGL(app_rowmin_kernel, grid, dim3(kRowTile), 0, st, C.targets, (const int32_t*)nullptr, k, (int64_t)0, C.verts, C.sel, V, body,
                       k, p.chunk, p.pmin + half, p.parg + half, 2 * half);
    hipLaunchKernelGGL(app_contact_merge_kernel, dim3(p.nb_k, N), dim3(kBlock), 0, st, C);
    hipLaunchKernelGGL(app_contact_grad_kernel, dim3(p.nb_k, N), dim3(kBlock), 0, st, C, p.grad_contact);
  }
  hipLaunchKernelGGL(app_finalize_kernel, dim3(N), dim3(kBlock), 0, st, (const double*)A.part_o, p.nb_v, V, (const double*)C.part_c, p.nb_k, k, p.terms);
  return check_launch(p.who);
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_app_objective_workspace_bytes(int V, int F, int k) { return sizes_ok(V, F, k, 1) ? layout(V, k).total : 0; }
extern "C" size_t coma_app_objective_batch_workspace_bytes(int V, int F, int k, int N) {
  return sizes_ok(V, F, k, N) ? layout(V, k, N).total : 0;
}

extern "C" int coma_app_objective_f32(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, int V,
                                      int F, const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                                      const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k,
                                      float* terms, float* grad_orientation, float* grad_contact, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  AppObjectivePlan p;
  if (int rc = app_objective_plan("coma_app_objective_f32", false, 1, verts, faces, vf_offsets, vf_faces, V, F, orientation_gt, obj_normal, principle_vec,
                                  sub_principle_vec, eps, selected, targets, k, terms, grad_orientation, grad_contact, workspace, workspace_bytes, p))
    return rc;
  return app_objective_enqueue(p, (hipStream_t)stream);
}

extern "C" int coma_app_objective_batch_f32(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces,
                                            int V, int F, const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                                            const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k,
                                            int N, float* terms, float* grad_orientation, float* grad_contact, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  AppObjectivePlan p;
  if (int rc = app_objective_plan("coma_app_objective_batch_f32", true, N, verts, faces, vf_offsets, vf_faces, V, F, orientation_gt, obj_normal,
                                  principle_vec, sub_principle_vec, eps, selected, targets, k, terms, grad_orientation, grad_contact, workspace,
                                  workspace_bytes, p))
    return rc;
  return app_objective_enqueue(p, (hipStream_t)stream);
}
