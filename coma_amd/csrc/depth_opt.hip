// Depth optimisation (gfx950): the shift profile of the column crossings as the collision term, the multiview joint term and the
// Adam update of the one parameter d, the displacement along the camera's front vector.  The rule set is stated in
// include/coma_hip.h and restated in NumPy by tests/shift_ref.py.  The crossings come from the kernels of mesh_volume.hip
// (columns_common.h); everything the profile does with them is integer arithmetic, so L is bit-exact whatever the order of arrival.
// The step kernel's sums have a fixed shape and no FMA, so the trajectory is bit-exact too.
//
// coma_shift_columns_prepare, on the caller's stream, no host synchronisation:
//   crossings -> reset ... fill of columns_crossings_launch: per-column lists, unsorted
//   params    -> grid size, scale and the offsets of the arrays, for the profile kernels (which receive the workspace only)
//   sort      -> one lane per column: sort by (mesh, Z) (in LDS up to kSortMax entries, in place in the workspace beyond), write the
//                list back, note where B's part starts, walk A's part and B's part for L_A and L_B; wave reduction, integer atomics
// coma_shift_profile: zero (L = 0, a kernel) -> profile: one lane per column merge-walks its two lists once per shift; a wave covers
//   64 neighbouring columns, whose lists are adjacent in memory; wave reduction, one integer atomic per wave and non-zero sum.
// coma_depth_optimize_f64: init (traj[0] = d0, Adam state, Ltraj = 0) -> per epoch: profile (K = 1, d read from traj) -> step (one
//   workgroup: multiview loss and gradient, collision ratio and slope from Ltraj, Adam, traj[e + 1]).
#include "coap_internal.h"
#include "columns_common.h"
#include "coma_device.h"

namespace coma {

constexpr long long kShiftLimit = 1ll << 42;
constexpr size_t kParamBytes = 64;
constexpr long long kShiftMagic = 0x5348494654434f4cll;
constexpr int kProfileBlocks = 1024;   // the profile's grid is fixed (the host does not know W x H there): grid-stride over the columns
constexpr int kViewDoubles = 28;
constexpr int kMaxShifts = 64, kMaxEpochs = 4096, kMaxJoints = 1024, kMaxInliers = 65536;
enum { kStM = 0, kStV = 1, kStP1 = 2, kStP2 = 3, kStStatus = 4, kStEpoch = 5 };   // state block, in units of 8 bytes

// first 64 bytes of a shift workspace; the columns workspace (header first) follows
struct ShiftParams {
  long long magic, n;
  long long off_cnt, off_entries, off_split;   // byte offsets from the start of the shift workspace
  double s;
  long long pad[2];
};
static_assert(sizeof(ShiftParams) == kParamBytes, "parameter block");

struct ShiftLayout {
  ColumnsLayout c;
  size_t split, total;
};

static ShiftLayout shift_layout(int VA, int FA, int VB, int FB, int W, int H, long long capacity) {
  ShiftLayout l;
  l.c = columns_layout(VA, FA, VB, FB, W, H, capacity);
  l.split = kParamBytes + (l.c.total + 15) / 16 * 16;
  l.total = l.split + (size_t)W * H * sizeof(unsigned);
  return l;
}

__global__ void shift_params_kernel(ShiftParams* __restrict__ out, ShiftParams p) {
  if (threadIdx.x == 0) *out = p;
}

// order of the stored lists: mesh A before mesh B, then by Z (the packed word is monotone in Z within one mesh)
__device__ __forceinline__ bool crossing_before(long long a, long long b) {
  const long long ma = a & 2, mb = b & 2;
  return ma != mb ? ma < mb : a < b;
}

// sum of the interval lengths inside ONE mesh along p[0], p[stride], ...: n != 0 between two consecutive crossings
__device__ __forceinline__ long long inside_length(const long long* p, int stride, int n) {
  int w = 0;
  long long prev = 0, len = 0;
  for (int i = 0; i < n; ++i) {
    const long long e = p[(int64_t)i * stride];
    const long long Z = e >> 2;   // arithmetic: a floor
    if (i > 0 && w != 0) len += Z - prev;
    w -= (e & 1) ? 1 : -1;
    prev = Z;
  }
  return len;
}

// insertion sort of p[0], p[stride], ... by (mesh, Z); returns the number of crossings of mesh A
__device__ __forceinline__ int sort_by_mesh(long long* p, int stride, int n) {
  for (int i = 1; i < n; ++i) {
    const long long e = p[(int64_t)i * stride];
    int j = i - 1;
    while (j >= 0 && crossing_before(e, p[(int64_t)j * stride])) {
      p[(int64_t)(j + 1) * stride] = p[(int64_t)j * stride];
      --j;
    }
    p[(int64_t)(j + 1) * stride] = e;
  }
  int na = 0;
  while (na < n && !(p[(int64_t)na * stride] & 2)) ++na;
  return na;
}

__global__ __launch_bounds__(256) void shift_sort_kernel(const unsigned* __restrict__ ends, long long* __restrict__ entries, int64_t n,
                                                         unsigned* __restrict__ split, int* __restrict__ hdr) {
  __shared__ long long lds[kSortMax * 256];   // entry k of lane t at [k * 256 + t]: consecutive lanes, consecutive banks
  if (hdr[0]) return;
  const int tid = threadIdx.x;
  const int64_t col = (int64_t)blockIdx.x * 256 + tid;
  long long la = 0, lb = 0;
  if (col < n) {
    const unsigned lo = col ? ends[col - 1] : 0u, hi = ends[col];
    const int m = (int)(hi - lo);
    int na = 0;
    if (m > 0 && m <= kSortMax) {
      for (int k = 0; k < m; ++k) lds[k * 256 + tid] = entries[lo + k];
      na = sort_by_mesh(&lds[tid], 256, m);
      la = inside_length(&lds[tid], 256, na), lb = inside_length(&lds[na * 256 + tid], 256, m - na);
      for (int k = 0; k < m; ++k) entries[lo + k] = lds[k * 256 + tid];
    } else if (m > kSortMax) {
      na = sort_by_mesh(entries + lo, 1, m);   // a long column: slow, in place, correct
      la = inside_length(entries + lo, 1, na), lb = inside_length(entries + lo + na, 1, m - na);
    }
    split[col] = lo + (unsigned)na;
  }
  la = wave_sum(la), lb = wave_sum(lb);
  if ((tid & (kWave - 1)) == 0) {
    unsigned long long* acc = (unsigned long long*)hdr + kHdrSums;
    if (la) atomicAdd(&acc[1], (unsigned long long)la);
    if (lb) atomicAdd(&acc[2], (unsigned long long)lb);
  }
}

__global__ void shift_lengths_kernel(const int* __restrict__ hdr, long long* __restrict__ lengths) {
  if (hdr[0]) return;
  if (threadIdx.x < 2) lengths[threadIdx.x] = ((const long long*)hdr)[kHdrSums + 1 + threadIdx.x];
}

// the shift of a displacement d in 1/256-cell units, clamped; a NaN counts as beyond the clamp
__device__ __forceinline__ long long shift_of(double d, double s) {
  const double q = floor((d * s) * 256.0 + 0.5);
  if (!(fabs(q) <= (double)kShiftLimit)) return q < 0.0 ? -kShiftLimit : kShiftLimit;
  return (long long)q;
}

// L_AB of one column with `delta` added to every Z of A: the merge of the two sorted lists, walked upwards
__device__ __forceinline__ long long merge_length(const long long* __restrict__ pa, int na, const long long* __restrict__ pb, int nb,
                                                  long long delta) {
  int ia = 0, ib = 0, wa = 0, wb = 0;
  long long prev = 0, len = 0;
  long long ea = pa[0], eb = pb[0];   // na, nb >= 1
  while (ia < na || ib < nb) {
    const bool take_a = ib >= nb || (ia < na && (ea >> 2) + delta <= (eb >> 2));
    const long long Z = take_a ? (ea >> 2) + delta : (eb >> 2);
    if (wa != 0 && wb != 0) len += Z - prev;   // both are 0 before the first event
    if (take_a) {
      wa -= (ea & 1) ? 1 : -1;
      if (++ia < na) ea = pa[ia];
    } else {
      wb -= (eb & 1) ? 1 : -1;
      if (++ib < nb) eb = pb[ib];
    }
    prev = Z;
  }
  return len;
}

__global__ __launch_bounds__(256) void shift_zero_kernel(const char* __restrict__ ws, long long* __restrict__ L, int count) {
  const ShiftParams* p = (const ShiftParams*)ws;
  if (p->magic != kShiftMagic || ((const int*)(ws + kParamBytes))[0]) return;
  for (int i = threadIdx.x; i < count; i += 256) L[i] = 0;
}

// stop (may be NULL): the optimiser's state block; nothing is added once its status is set
__global__ __launch_bounds__(256) void shift_profile_kernel(const char* __restrict__ ws, const double* __restrict__ d, int K,
                                                            long long* __restrict__ L, const long long* __restrict__ stop) {
  const ShiftParams* p = (const ShiftParams*)ws;
  if (p->magic != kShiftMagic || ((const int*)(ws + kParamBytes))[0]) return;
  if (stop && stop[kStStatus]) return;
  const int64_t n = p->n;
  const double s = p->s;
  const unsigned* ends = (const unsigned*)(ws + p->off_cnt);
  const unsigned* split = (const unsigned*)(ws + p->off_split);
  const long long* entries = (const long long*)(ws + p->off_entries);
  const int tid = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {   // uniform per workgroup
    const int64_t col = base + tid;
    unsigned lo = 0, mid = 0, hi = 0;
    if (col < n) lo = col ? ends[col - 1] : 0u, mid = split[col], hi = ends[col];
    const int na = (int)(mid - lo), nb = (int)(hi - mid);
    const bool both = na > 0 && nb > 0;
    if (!__any(both)) continue;   // a wave over columns that one of the meshes does not reach
    for (int k = 0; k < K; ++k) {
      const long long delta = shift_of(d[k], s);
      long long l[3] = {0, 0, 0};
      if (both) {
#pragma unroll
        for (int j = 0; j < 3; ++j) l[j] = merge_length(entries + lo, na, entries + mid, nb, delta + (j - 1));
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long long sum = wave_sum(l[j]);
        if ((tid & (kWave - 1)) == 0 && sum) atomicAdd((unsigned long long*)&L[3 * k + j], (unsigned long long)sum);
      }
    }
  }
}

// ---- the optimiser ----
__global__ __launch_bounds__(256) void depth_init_kernel(const char* __restrict__ ws, double d0, double* __restrict__ traj,
                                                         long long* __restrict__ Ltraj, int E, double* __restrict__ state) {
  if (ws && (((const ShiftParams*)ws)->magic != kShiftMagic || ((const int*)(ws + kParamBytes))[0])) {
    if (threadIdx.x == 0) ((long long*)state)[kStStatus] = 2, ((long long*)state)[kStEpoch] = 0;   // the columns were refused
    return;
  }
  if (ws)
    for (int i = threadIdx.x; i < 3 * E; i += 256) Ltraj[i] = 0;
  if (threadIdx.x == 0) {
    traj[0] = d0;
    state[kStM] = 0.0, state[kStV] = 0.0, state[kStP1] = 1.0, state[kStP2] = 1.0;
    ((long long*)state)[kStStatus] = __builtin_isfinite(d0) ? 0 : 1;
    ((long long*)state)[kStEpoch] = 0;
  }
}

// The multiview term of one epoch, by one workgroup: thread t adds up the views t, t + 256, ... in ascending order, each view its
// joints in ascending order; the tree follows.  joints = J0 + d f; per view q = joints (R C) - t (R C), xy = q / scale max(res) +
// res / 2 (view_record layout).  Every thread returns the mean loss and its derivative.  A cand_view entry outside [0, n_views) is not
// followed: status 3 and the epoch are recorded, and every thread returns true -- the caller then writes nothing for this epoch.
__device__ __forceinline__ bool multiview_term(const double* __restrict__ views, const double* __restrict__ joints0, double f0, double f1, double f2,
                                               const int* __restrict__ cand_view, int n_views, const double* __restrict__ cand_xy, int N, int J, int e,
                                               double d, double* __restrict__ state, double* lds, double* loss_out, double* grad_out) {
  const double ox = d * f0, oy = d * f1, oz = d * f2;
  double loss = 0.0, grad = 0.0;
  int bad = 0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const int view = cand_view[n];
    if (view < 0 || view >= n_views) {   // not followed; recorded, and the later epochs idle
      ((long long*)state)[kStStatus] = 3, ((long long*)state)[kStEpoch] = e;   // every writer stores the same two values
      bad = 1;
      continue;
    }
    const double* w = views + (int64_t)view * kViewDoubles;
    const double* mr = w + 12;
    const double* tmr = w + 21;
    const double scale = w[24], maxres = w[25], hx = w[26], hy = w[27];
    const double ax = ((f0 * mr[0] + f1 * mr[3]) + f2 * mr[6]) / scale * maxres;   // d xy / d d
    const double ay = ((f0 * mr[1] + f1 * mr[4]) + f2 * mr[7]) / scale * maxres;
    double sq = 0.0, gr = 0.0;
    for (int j = 0; j < J; ++j) {
      const double x = joints0[3 * j] + ox, y = joints0[3 * j + 1] + oy, z = joints0[3 * j + 2] + oz;
      const double cx = ((x * mr[0] + y * mr[3]) + z * mr[6]) - tmr[0];
      const double cy = ((x * mr[1] + y * mr[4]) + z * mr[7]) - tmr[1];
      const double rx = (cx / scale * maxres + hx) - cand_xy[((int64_t)n * J + j) * 2];
      const double ry = (cy / scale * maxres + hy) - cand_xy[((int64_t)n * J + j) * 2 + 1];
      sq = sq + (rx * rx + ry * ry);
      gr = gr + (rx * ax + ry * ay);
    }
    loss = loss + 0.5 * sq;   // the sum over the joints, the mean over the two coordinates
    grad = grad + gr;
  }
  loss = block_sum<256>(loss, lds);
  grad = block_sum<256>(grad, lds);
  if (N > 0) loss = loss / (double)N, grad = grad / (double)N;
  *loss_out = loss, *grad_out = grad;
  return __syncthreads_or(bad) != 0;   // uniform: one bad entry anywhere stops the whole step
}

// Adam on the one parameter (thread 0): g = the objective's derivative at traj[e]; writes traj[e + 1] and the state block
__device__ __forceinline__ void adam_step(double g, double d, double lr, int e, double* __restrict__ traj, double* __restrict__ state) {
  const double b1 = 0.9, b2 = 0.999;
  const double m = b1 * state[kStM] + (1.0 - b1) * g;
  const double v = b2 * state[kStV] + (1.0 - b2) * g * g;
  const double p1 = state[kStP1] * b1, p2 = state[kStP2] * b2;
  const double next = d - (lr / (1.0 - p1)) * m / (sqrt(v) / sqrt(1.0 - p2) + 1e-8);
  state[kStM] = m, state[kStV] = v, state[kStP1] = p1, state[kStP2] = p2;
  traj[e + 1] = next;
  if (!__builtin_isfinite(next) && !((long long*)state)[kStStatus]) ((long long*)state)[kStStatus] = 1, ((long long*)state)[kStEpoch] = e + 1;
}

// Where an epoch's collision term {value, d value / d d} comes from; each source's arithmetic is its own.
// The shift profile: Ltraj[e] = the three lengths of this epoch, written by the profile launch; L_A and the scale from the workspace
struct ShiftSource {
  const char* ws;            // null: no collision term
  const long long* Ltraj;
  __device__ __forceinline__ void term(int e, double w_collision, double* value, double* slope) const {
    double ratio = 0.0, sl = 0.0;
    if (ws && w_collision != 0.0) {
      const long long la = ((const long long*)(ws + kParamBytes))[kHdrSums + 1];
      if (la != 0) {
        const long long* l = Ltraj + 3 * (int64_t)e;
        ratio = (double)l[1] / (double)la;
        sl = ((double)(l[2] - l[0]) * (256.0 * ((const ShiftParams*)ws)->s)) / (2.0 * (double)la);
      }
    }
    *value = ratio, *slope = sl;
  }
};

// COAP: Ctraj[e] = {loss, d loss / d d} of this epoch, written by the collision launches
struct CoapSource {
  const double* Ctraj;
  __device__ __forceinline__ void term(int e, double w_collision, double* value, double* slope) const {
    *value = w_collision != 0.0 ? Ctraj[2 * e] : 0.0, *slope = w_collision != 0.0 ? Ctraj[2 * e + 1] : 0.0;
  }
};

template <typename Source>
__global__ __launch_bounds__(256) void depth_step_kernel(Source source, const double* __restrict__ views, const double* __restrict__ joints0, double f0,
                                                         double f1, double f2, const int* __restrict__ cand_view, int n_views,
                                                         const double* __restrict__ cand_xy, int N, int J, double lr, double w_multiview,
                                                         double w_collision, int e, double* __restrict__ traj, double* __restrict__ losses,
                                                         double* __restrict__ state) {
  __shared__ double lds[256];
  const long long stopped = ((const long long*)state)[kStStatus];
  __syncthreads();   // every thread has read the word before any thread may set it below: the branch is uniform
  if (stopped) return;
  const double d = traj[e];
  double loss, grad;
  if (multiview_term(views, joints0, f0, f1, f2, cand_view, n_views, cand_xy, N, J, e, d, state, lds, &loss, &grad)) return;   // status 3: losses, traj, Adam untouched
  if (threadIdx.x != 0) return;
  double value, slope;
  source.term(e, w_collision, &value, &slope);
  losses[2 * e] = loss, losses[2 * e + 1] = value;
  adam_step(w_multiview * grad + w_collision * slope, d, lr, e, traj, state);
}

// what both optimisers refuse of the arguments they share (no launch)
static int depth_optimize_check(const char* who, const double* views, int n_views, const double* joints0, const double* front, const int32_t* cand_view,
                                const double* cand_xy, int N, int J, double d0, double lr, double w_multiview, double w_collision, int E,
                                const double* traj, const double* losses, const void* state) {
  if (!front || !traj || !losses || !state) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (E < 1 || E > kMaxEpochs) return fail(COMA_E_INVALID, "%s: E=%d outside [1, %d]", who, E, kMaxEpochs);
  if (N < 0 || N > kMaxInliers || J < 1 || J > kMaxJoints || n_views < 0)
    return fail(COMA_E_INVALID, "%s: N=%d outside [0, %d], J=%d outside [1, %d] or n_views=%d < 0", who, N, kMaxInliers, J, kMaxJoints, n_views);
  if (N > 0 && (!views || !joints0 || !cand_view || !cand_xy || n_views < 1))
    return fail(COMA_E_INVALID, "%s: null pointer (views, joints0, cand_view, cand_xy are read when N > 0)", who);
  if (!__builtin_isfinite(d0) || !__builtin_isfinite(lr) || !__builtin_isfinite(w_multiview) || !__builtin_isfinite(w_collision) ||
      !__builtin_isfinite(front[0]) || !__builtin_isfinite(front[1]) || !__builtin_isfinite(front[2]))
    return fail(COMA_E_INVALID, "%s: d0, lr, the weights and front must be finite", who);
  return COMA_OK;
}

static int read_status(const void* hdr, void* stream, int64_t* needed, const char* who) {
  long long head[3] = {0, 0, 0};   // status word + list length, list length + depth flag, crossings counted
  if (int rc = read_back(head, hdr, sizeof(head), stream, who)) return rc;
  const int word = (int)(head[0] & 0xffffffffll);
  if (needed) *needed = head[kHdrNeeded];
  const char* of = "coma_shift_columns_prepare";   // the call whose refusal the workspace holds
  if (word & kBadNonFinite) return fail(COMA_E_INVALID, "%s: non-finite vertex (nothing written)", of);
  if (word & kBadRange) return fail(COMA_E_INVALID, "%s: a snapped coordinate exceeds +-2^25 (1/256-cell units; nothing written)", of);
  if (word & kBadFace) return fail(COMA_E_INVALID, "%s: face index outside [0, V) (nothing written)", of);
  if (word & kBadDepth)
    return fail(COMA_E_INVALID, "%s: a crossing's depth is non-finite or beyond +-2^40 (1/256-cell units; nothing written)", of);
  if (word & kBadCapacity) return fail(COMA_E_INVALID, "%s: capacity exceeded, %lld crossings needed (nothing written)", of, head[kHdrNeeded]);
  return COMA_OK;
}

static int profile_launch(const char* ws, const double* d, int K, long long* L, const long long* stop, hipStream_t st) {
  hipLaunchKernelGGL(shift_profile_kernel, dim3(kProfileBlocks), dim3(256), 0, st, ws, d, K, L, stop);
  return check_launch("shift_profile_kernel");
}

}  // namespace coma

using namespace coma;

extern "C" size_t coma_shift_columns_workspace_bytes(int VA, int FA, int VB, int FB, int W, int H, int64_t capacity) {
  if (!columns_sizes_ok(VA, FA, VB, FB, W, H, capacity)) return 0;
  return shift_layout(VA, FA, VB, FB, W, H, capacity).total;
}

extern "C" int coma_shift_columns_prepare(const double* vertsA, int VA, const int32_t* facesA, int FA, const double* vertsB, int VB,
                                          const int32_t* facesB, int FB, double x0, double y0, double s, int W, int H, int64_t capacity,
                                          void* workspace, int64_t* lengths, void* stream) {
  if (!vertsA || !facesA || !vertsB || !facesB || !workspace) return fail(COMA_E_INVALID, "coma_shift_columns_prepare: null pointer");
  if (!columns_sizes_ok(VA, FA, VB, FB, W, H, capacity))
    return fail(COMA_E_INVALID, "coma_shift_columns_prepare: V, F outside [1, %d], W, H outside [1, %d] or capacity outside [1, %lld]", kRasterMaxPrims,
                kRasterMaxDim, kMaxCapacity);
  if (!(s > 0.0) || !(s <= 1.7e308) || !__builtin_isfinite(x0) || !__builtin_isfinite(y0))
    return fail(COMA_E_INVALID, "coma_shift_columns_prepare: s=%g must be positive and finite, the origin finite", s);
  if ((uintptr_t)workspace % 16) return fail(COMA_E_INVALID, "coma_shift_columns_prepare: workspace must be 16-byte aligned");
  const ShiftLayout l = shift_layout(VA, FA, VB, FB, W, H, capacity);
  char* ws = (char*)workspace;
  char* cws = ws + kParamBytes;
  int* hdr = (int*)cws;
  const double* verts[2] = {vertsA, vertsB};
  const int* faces[2] = {facesA, facesB};
  const int V[2] = {VA, VB}, F[2] = {FA, FB};
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)W * H;
  ShiftParams p = {};
  p.magic = kShiftMagic, p.n = n, p.s = s;
  p.off_cnt = (long long)(kParamBytes + l.c.cnt), p.off_entries = (long long)(kParamBytes + l.c.entries), p.off_split = (long long)l.split;
  if (int rc = columns_crossings_launch(verts, V, faces, F, x0, y0, s, W, H, (long long)capacity, cws, l.c, st)) return rc;
  hipLaunchKernelGGL(shift_params_kernel, dim3(1), dim3(64), 0, st, (ShiftParams*)ws, p);
  if (int rc = check_launch("shift_params_kernel")) return rc;
  hipLaunchKernelGGL(shift_sort_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned*)(cws + l.c.cnt),
                     (long long*)(cws + l.c.entries), n, (unsigned*)(ws + l.split), hdr);
  if (int rc = check_launch("shift_sort_kernel")) return rc;
  if (lengths) {
    hipLaunchKernelGGL(shift_lengths_kernel, dim3(1), dim3(64), 0, st, hdr, (long long*)lengths);
    if (int rc = check_launch("shift_lengths_kernel")) return rc;
  }
  return COMA_OK;
}

extern "C" int coma_shift_columns_status(const void* workspace, void* stream, int64_t* needed) {
  if (!workspace) return fail(COMA_E_INVALID, "coma_shift_columns_status: null pointer");
  return read_status((const char*)workspace + kParamBytes, stream, needed, "coma_shift_columns_status");
}

extern "C" int coma_shift_profile(const void* workspace, const double* d, int K, int64_t* L, void* stream) {
  if (!workspace || !d || !L) return fail(COMA_E_INVALID, "coma_shift_profile: null pointer");
  if (K < 1 || K > kMaxShifts) return fail(COMA_E_INVALID, "coma_shift_profile: K=%d outside [1, %d]", K, kMaxShifts);
  if ((uintptr_t)workspace % 16) return fail(COMA_E_INVALID, "coma_shift_profile: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(shift_zero_kernel, dim3(1), dim3(256), 0, st, (const char*)workspace, (long long*)L, 3 * K);
  if (int rc = check_launch("shift_zero_kernel")) return rc;
  return profile_launch((const char*)workspace, d, K, (long long*)L, nullptr, st);
}

extern "C" size_t coma_depth_optimize_state_bytes(void) { return 64; }

extern "C" int coma_depth_optimize_f64(const void* workspace, const double* views, int n_views, const double* joints0, const double* front,
                                       const int32_t* cand_view, const double* cand_xy, int N, int J, double d0, double lr, double w_multiview,
                                       double w_collision, int E, double* traj, int64_t* Ltraj, double* losses, void* state, void* stream) {
  const char* who = "coma_depth_optimize_f64";
  if (int rc = depth_optimize_check(who, views, n_views, joints0, front, cand_view, cand_xy, N, J, d0, lr, w_multiview, w_collision, E, traj, losses, state))
    return rc;
  const char* ws = (workspace && w_collision != 0.0) ? (const char*)workspace : nullptr;
  if (ws && !Ltraj) return fail(COMA_E_INVALID, "%s: Ltraj is written when the collision term is on", who);
  if (((uintptr_t)workspace % 16) || ((uintptr_t)state % 8)) return fail(COMA_E_INVALID, "%s: workspace 16-byte, state 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_init_kernel, dim3(1), dim3(256), 0, st, ws, d0, traj, (long long*)Ltraj, E, (double*)state);
  if (int rc = check_launch("depth_init_kernel")) return rc;
  for (int e = 0; e < E; ++e) {
    if (ws)
      if (int rc = profile_launch(ws, traj + e, 1, (long long*)Ltraj + 3 * (int64_t)e, (const long long*)state, st)) return rc;
    hipLaunchKernelGGL(depth_step_kernel<ShiftSource>, dim3(1), dim3(256), 0, st, ShiftSource{ws, (const long long*)Ltraj}, views, joints0, front[0], front[1],
                       front[2], cand_view, n_views, cand_xy, N, J, lr, w_multiview, w_collision, e, traj, losses, (double*)state);
    if (int rc = check_launch("depth_step_kernel")) return rc;
  }
  return COMA_OK;
}

extern "C" int coma_depth_optimize_coap_f64(const float* weights, size_t weights_floats, const void* code, int K, const float* points, int T,
                                            double filter_threshold, void* coap_workspace, size_t coap_workspace_bytes, const double* views, int n_views,
                                            const double* joints0, const double* front, const int32_t* cand_view, const double* cand_xy, int N, int J,
                                            double d0, double lr, double w_multiview, double w_collision, int E, double* traj, double* Ctraj,
                                            double* losses, void* state, void* stream) {
  const char* who = "coma_depth_optimize_coap_f64";
  if (int rc = depth_optimize_check(who, views, n_views, joints0, front, cand_view, cand_xy, N, J, d0, lr, w_multiview, w_collision, E, traj, losses, state))
    return rc;
  const bool collide = w_collision != 0.0;
  if (collide) {
    if (!Ctraj) return fail(COMA_E_INVALID, "%s: Ctraj is written when the collision term is on", who);
    if (int rc = coap_collision_check(who, weights, code, K, points, T, front, filter_threshold, coap_workspace, coap_workspace_bytes)) return rc;
    if (weights_floats < coap_weights_floats(K)) return fail(COMA_E_INVALID, "%s: weights of %zu floats, %zu needed", who, weights_floats, coap_weights_floats(K));
    if (((uintptr_t)weights & 15) || ((uintptr_t)Ctraj & 7)) return fail(COMA_E_INVALID, "%s: Ctraj 8-byte, the weights 16-byte aligned", who);
  }
  if ((uintptr_t)state % 8) return fail(COMA_E_INVALID, "%s: state must be 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_init_kernel, dim3(1), dim3(256), 0, st, (const char*)nullptr, d0, traj, (long long*)nullptr, E, (double*)state);
  if (int rc = check_launch("depth_init_kernel")) return rc;
  for (int e = 0; e < E; ++e) {
    if (collide)
      if (int rc = coap_collision_launch(weights, code, K, points, T, traj + e, front, filter_threshold, Ctraj + 2 * (int64_t)e, nullptr, coap_workspace,
                                         (const long long*)state, st))
        return rc;
    hipLaunchKernelGGL(depth_step_kernel<CoapSource>, dim3(1), dim3(256), 0, st, CoapSource{Ctraj}, views, joints0, front[0], front[1], front[2], cand_view,
                       n_views, cand_xy, N, J, lr, w_multiview, w_collision, e, traj, losses, (double*)state);
    if (int rc = check_launch("depth_step_kernel")) return rc;
  }
  return COMA_OK;
}

extern "C" int coma_depth_optimize_status(const void* state, void* stream, int* epoch) {
  if (!state) return fail(COMA_E_INVALID, "coma_depth_optimize_status: null pointer");
  long long tail[2] = {0, 0};
  if (int rc = read_back(tail, (const long long*)state + kStStatus, sizeof(tail), stream, "coma_depth_optimize_status")) return rc;
  if (epoch) *epoch = (int)tail[1];
  if (tail[0] == 3) return fail(COMA_E_INVALID, "coma_depth_optimize_f64: cand_view holds an index outside [0, n_views) (met in epoch %d; nothing written for it, later epochs not run)", (int)tail[1]);
  if (tail[0] == 2) return fail(COMA_E_INVALID, "coma_depth_optimize_f64: the columns workspace holds a refused call (nothing written)");
  if (tail[0]) return fail(COMA_E_INVALID, "coma_depth_optimize_f64: d is not finite after epoch %d (later epochs not run)", (int)tail[1]);
  return COMA_OK;
}
