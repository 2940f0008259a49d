// The fitting app's Adam loop (gfx950): E iterations of decode -> skin -> objective -> backward -> Adam enqueued by ONE call.  The rule
// set is stated in include/coma_hip.h ("The fitting app's whole Adam loop") and restated in NumPy by tests/fit_ref.py.  Every stage
// is the existing entry point's two halves (fit_stages.h: vposer.hip, smplx.hip, app_objective.hip): its plan is made ONCE per call, on
// buffers carved from one workspace -- the plans make the stages' refusals, under this call's name, so every refusal comes before the
// first launch and none of them is written out again here -- and the loop only enqueues, on the caller's stream.  The kernels of this
// file move numbers between the stages and take the step:
//   assemble   p (f64, state) -> theta, z, transl (f32)                       one workgroup
//   pose       aa -> theta's body_pose slot; the angle prior and its sum (f64)  one workgroup
//   scale      vs = raw vertices * scale_factor (f32)                          3V elements
//   seed       g = (w_o g_o + w_c g_c) * scale_factor (f32, unfused)            3V elements
//   prior_grad grad_aa = grad_theta[body] + w_bend d prior                      3 NJ elements
//   step       g[P], the non-finite test, Adam, the records                     one workgroup
// All are latency-bound launches; sums have a fixed shape (block_sum) and nothing is contracted into FMAs (-ffp-contract=off), so two
// calls give the same bits.
#include "coma_device.h"
#include "fit_stages.h"

#include <cmath>

namespace coma {
namespace {

constexpr int kFitBlock = 256;
constexpr int kFitMaxP = 2 * kFitBlock;      // the step kernel keeps two components per thread
constexpr int kFitMaxD = 256, kFitMaxHand = 96, kFitMaxK = 16, kFitMaxEpochs = 4096;
constexpr int kLeadFixed = 9;                // jaw, left eye, right eye
constexpr long long kFitMagic = 0x434f4d41464954ll;   // "COMAFIT"; the header keeps magic + P
// state block in units of 8 bytes: header, then p, m, v (P each)
enum { kFsStatus = 0, kFsIteration = 1, kFsCount = 2, kFsMagic = 3, kFsP1 = 4, kFsP2 = 5, kFsHeader = 8 };
enum { kFitOk = 0, kFitNonFinite = 1, kFitOtherP = 2 };

struct PriorVec { int32_t index[kFitMaxK]; float sign[kFitMaxK]; int K; };

__device__ __forceinline__ bool state_ok(const double* state, int P) { return ((const long long*)state)[kFsMagic] == kFitMagic + P; }

__global__ __launch_bounds__(kFitBlock) void fit_init_kernel(const double* __restrict__ p0, int P, double* __restrict__ state) {
  const int t = threadIdx.x;
  for (int i = t; i < P; i += kFitBlock) {
    state[kFsHeader + i] = p0[i];
    state[kFsHeader + P + i] = 0.0;
    state[kFsHeader + 2 * P + i] = 0.0;
  }
  if (t == 0) {
    long long* w = (long long*)state;
    w[kFsStatus] = kFitOk, w[kFsIteration] = 0, w[kFsCount] = 0, w[kFsMagic] = kFitMagic + P;
    state[kFsP1] = 1.0, state[kFsP2] = 1.0, state[6] = 0.0, state[7] = 0.0;
  }
}

// p = [global_orient 3 | transl 3 | left hs | right hs | z D] -> theta = [global_orient | body 3 NJ (not written) | fixed 9 | left | right]
__global__ __launch_bounds__(kFitBlock) void fit_assemble_kernel(double* __restrict__ state, int P, int hs, int D, int n_body,
                                                                 const float* __restrict__ lead_fixed, float* __restrict__ theta,
                                                                 float* __restrict__ z, float* __restrict__ transl) {
  if (!state_ok(state, P)) {   // an init of another P is recorded in its own header; anything else is not ours to write to
    const long long other = ((const long long*)state)[kFsMagic] - kFitMagic;
    if (threadIdx.x == 0 && other >= 7 && other <= kFitMaxP) ((long long*)state)[kFsStatus] = kFitOtherP;
    return;
  }
  const double* p = state + kFsHeader;
  const int hands = 3 + n_body + kLeadFixed;
  for (int i = threadIdx.x; i < P; i += kFitBlock) {
    const float x = (float)p[i];
    if (i < 3) theta[i] = x;
    else if (i < 6) transl[i - 3] = x;
    else if (i < 6 + 2 * hs) theta[hands + (i - 6)] = x;
    else z[i - 6 - 2 * hs] = x;
  }
  if (threadIdx.x < kLeadFixed) theta[3 + n_body + threadIdx.x] = lead_fixed[threadIdx.x];
}

__global__ __launch_bounds__(kFitBlock) void fit_pose_kernel(const float* __restrict__ aa, int n_body, PriorVec a, float* __restrict__ theta,
                                                             double* __restrict__ prior_sum) {
  __shared__ double lds[kFitBlock];
  const int t = threadIdx.x;
  for (int i = t; i < n_body; i += kFitBlock) theta[3 + i] = aa[i];
  double v = 0.0;
  if (t < a.K) {
    const double e = exp((double)a.sign[t] * (double)aa[a.index[t]]);
    v = e * e;
  }
  v = block_sum<kFitBlock>(v, lds);
  if (t == 0) prior_sum[0] = v;
}

__global__ __launch_bounds__(kFitBlock) void fit_scale_kernel(const float* __restrict__ raw, int n, float scale, float* __restrict__ vs) {
  const int i = blockIdx.x * kFitBlock + threadIdx.x;
  if (i < n) vs[i] = raw[i] * scale;
}

__global__ __launch_bounds__(kFitBlock) void fit_seed_kernel(const float* __restrict__ g_o, const float* __restrict__ g_c, int n, float w_o, float w_c,
                                                             float scale, float* __restrict__ g) {
  const int i = blockIdx.x * kFitBlock + threadIdx.x;
  if (i >= n) return;
  const float a = w_o * g_o[i], b = w_c * g_c[i];
  const float s = a + b;
  g[i] = s * scale;
}

__global__ __launch_bounds__(kFitBlock) void fit_prior_grad_kernel(const float* __restrict__ aa, const float* __restrict__ grad_theta, int n_body,
                                                                   PriorVec a, double w_bend, float* __restrict__ grad_aa) {
  const int j = blockIdx.x * kFitBlock + threadIdx.x;
  if (j >= n_body) return;
  double d = 0.0;
  for (int i = 0; i < a.K; ++i)
    if (a.index[i] == j) {
      const double s = (double)a.sign[i];
      const double e = exp(s * (double)aa[j]);
      d = d + 2.0 * s * (e * e);
    }
  grad_aa[j] = (float)((double)grad_theta[3 + j] + w_bend * d);
}

struct StepArgs {
  const float* grad_theta;
  const float* grad_transl;
  const float* grad_z;
  const float* terms;
  const double* prior_sum;
  int P, hs, D, n_body, e;
  double lr, w_body, w_bend, w_prior, w_o, w_c;
  double* traj;
  double* losses;
  double* grad0;
  double* state;
};

__global__ __launch_bounds__(kFitBlock) void fit_step_kernel(StepArgs a) {
  __shared__ double lds[kFitBlock];
  if (!state_ok(a.state, a.P)) return;
  const int t = threadIdx.x, P = a.P;
  double* p = a.state + kFsHeader;
  double* m = p + P;
  double* v = m + P;
  const int z0 = 6 + 2 * a.hs, hands = 3 + a.n_body + kLeadFixed;
  const double b1 = 0.9, b2 = 0.999;
  const double p1 = a.state[kFsP1] * b1, p2 = a.state[kFsP2] * b2;
  const double step = a.lr / (1.0 - p1), root2 = sqrt(1.0 - p2);
  const double w_pp = a.w_body * a.w_body * a.w_prior;

  double zz = 0.0, bad = 0.0;
  double old_[2], g_[2], m_[2], v_[2], new_[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = t + r * kFitBlock;
    old_[r] = g_[r] = m_[r] = v_[r] = new_[r] = 0.0;
    if (i >= P) continue;
    const double x = p[i];
    double g;
    if (i < 3) g = (double)a.grad_theta[i];
    else if (i < 6) g = (double)a.grad_transl[i - 3];
    else if (i < z0) g = (double)a.grad_theta[hands + (i - 6)];
    else {
      g = (double)a.grad_z[i - z0] + (2.0 * x) * w_pp;
      zz = zz + x * x;
    }
    const double mi = b1 * m[i] + (1.0 - b1) * g;
    const double vi = b2 * v[i] + ((1.0 - b2) * g) * g;
    const double xi = x - (step * mi) / (sqrt(vi) / root2 + 1e-8);
    old_[r] = x, g_[r] = g, m_[r] = mi, v_[r] = vi, new_[r] = xi;
    if (!__builtin_isfinite(g) || !__builtin_isfinite(xi)) bad = 1.0;
  }
  zz = block_sum<kFitBlock>(zz, lds);
  bad = block_sum<kFitBlock>(bad, lds);    // every thread gets the same sum: the branch below is uniform
  const bool apply = bad == 0.0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = t + r * kFitBlock;
    if (i >= P) continue;
    if (apply) p[i] = new_[r], m[i] = m_[r], v[i] = v_[r];
    if (a.traj) {
      if (a.e == 0) a.traj[i] = old_[r];
      a.traj[(int64_t)(a.e + 1) * P + i] = apply ? new_[r] : old_[r];
    }
    if (a.grad0 && a.e == 0) a.grad0[i] = g_[r];
  }
  if (t == 0) {
    long long* w = (long long*)a.state;
    const long long count = w[kFsCount];
    if (apply) a.state[kFsP1] = p1, a.state[kFsP2] = p2;
    else if (w[kFsStatus] == kFitOk) w[kFsStatus] = kFitNonFinite, w[kFsIteration] = count;
    w[kFsCount] = count + 1;
    const double pprior = (zz * (a.w_body * a.w_body)) * a.w_prior;
    const double bend = a.w_bend * a.prior_sum[0];
    const double t_o = (double)a.terms[0], t_c = (double)a.terms[1];
    double* l = a.losses + (int64_t)a.e * 5;
    l[0] = ((pprior + bend) + a.w_o * t_o) + a.w_c * t_c;
    l[1] = pprior, l[2] = bend, l[3] = t_o, l[4] = t_c;
  }
}

// what one call lays into its workspace; every field at a multiple of 16
struct FitLayout {
  size_t theta, z, transl, aa, raw, joints, sx_saved, sx_ws, vp_saved, vp_ws, obj_ws, terms, g_o, g_c, g, g_theta, g_transl, g_aa, g_z, prior, total;
  size_t sx_saved_bytes, sx_ws_bytes, vp_saved_bytes, vp_ws_bytes, obj_ws_bytes;
};

bool fit_layout(int V, int F, int J, int k, int H, int NJ, long long n_theta, FitLayout& L) {
  L = FitLayout{};
  L.sx_saved_bytes = coma_smplx_saved_bytes(V, J), L.sx_ws_bytes = coma_smplx_workspace_bytes(V, J);
  L.vp_saved_bytes = coma_vposer_saved_bytes(1, H, NJ), L.vp_ws_bytes = coma_vposer_workspace_bytes(1, H, NJ);
  L.obj_ws_bytes = coma_app_objective_workspace_bytes(V, F, k);
  if (!L.sx_saved_bytes || !L.sx_ws_bytes || !L.vp_saved_bytes || !L.vp_ws_bytes || !L.obj_ws_bytes) return false;
  if (n_theta < 3 * NJ + 3 + kLeadFixed || n_theta > 3 * NJ + 3 + kLeadFixed + 2 * kFitMaxHand) return false;   // NJ <= 64 by now
  const size_t f = sizeof(float), n3 = (size_t)3 * V;
  Carve ws;
  L.theta = ws.take((size_t)n_theta * f);
  L.z = ws.take((size_t)kFitMaxD * f);
  L.transl = ws.take(3 * f);
  L.aa = ws.take((size_t)3 * NJ * f);
  L.raw = ws.take(n3 * f);
  L.joints = ws.take((size_t)3 * J * f);
  L.sx_saved = ws.take(L.sx_saved_bytes);
  L.sx_ws = ws.take(L.sx_ws_bytes);
  L.vp_saved = ws.take(L.vp_saved_bytes);
  L.vp_ws = ws.take(L.vp_ws_bytes);
  L.obj_ws = ws.take(L.obj_ws_bytes);
  L.terms = ws.take(2 * f);
  L.g_o = ws.take(n3 * f);
  L.g_c = ws.take(n3 * f);
  L.g = ws.take(n3 * f);
  L.g_theta = ws.take((size_t)n_theta * f);
  L.g_transl = ws.take(3 * f);
  L.g_aa = ws.take((size_t)3 * NJ * f);
  L.g_z = ws.take((size_t)kFitMaxD * f);
  L.prior = ws.take(sizeof(double));
  L.total = ws.at;
  return true;
}

size_t state_bytes(int P) { return P >= 7 && P <= kFitMaxP ? align16((size_t)(kFsHeader + 3 * P) * sizeof(double)) : 0; }

}  // namespace
}  // namespace coma

using namespace coma;

extern "C" size_t coma_app_fit_state_bytes(int P) { return state_bytes(P); }

extern "C" size_t coma_app_fit_workspace_bytes(int V, int F, int J, int k, int H, int NJ, int n_theta) {
  FitLayout L;
  return fit_layout(V, F, J, k, H, NJ, n_theta, L) ? L.total : 0;
}

extern "C" int coma_app_fit_init_f64(const double* p0, int P, void* state, size_t state_bytes_, void* stream) {
  const char* who = "coma_app_fit_init_f64";
  if (!p0 || !state) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!state_bytes(P)) return fail(COMA_E_INVALID, "%s: P=%d outside [7, %d]", who, P, kFitMaxP);
  if (int rc = check_buffer(who, "state", state, state_bytes_, state_bytes(P))) return rc;
  if ((uintptr_t)p0 & 7) return fail(COMA_E_INVALID, "%s: p0 must be 8-byte aligned", who);
  hipLaunchKernelGGL(fit_init_kernel, dim3(1), dim3(kFitBlock), 0, (hipStream_t)stream, p0, P, (double*)state);
  return check_launch(who);
}

extern "C" int coma_app_fit_f32(const coma_app_fit_desc* d, void* state, size_t state_bytes_, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const char* who = "coma_app_fit_f32";
  if (!d || !state || !workspace) return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (!d->lead_fixed || !d->prior_index || !d->prior_sign || !d->losses)     // the fit's own; the stages' pointers are refused by their plans
    return fail(COMA_E_INVALID, "%s: null pointer", who);
  if (d->E < 1 || d->E > kFitMaxEpochs) return fail(COMA_E_INVALID, "%s: E=%d outside [1, %d]", who, d->E, kFitMaxEpochs);
  const int V = d->V, J = d->J, hd = d->hand_dim, n_pca = d->n_pca, D = d->D, H = d->H, NJ = d->NJ, K = d->prior_K, k = d->k, P = d->P;
  if (D < 1 || D > kFitMaxD) return fail(COMA_E_INVALID, "%s: D=%d outside [1, %d]", who, D, kFitMaxD);
  const int hs = (n_pca > 0 && hd > 0) ? n_pca : hd;
  if (hs < 0 || hs > kFitMaxHand) return fail(COMA_E_INVALID, "%s: %d entries per hand, outside [0, %d]", who, hs, kFitMaxHand);
  // every carved field has the alignment of the block it is carved from: said of the caller's two blocks, not of a field
  if (((uintptr_t)state & 15) != 0) return fail(COMA_E_INVALID, "%s: state must be 16-byte aligned", who);
  if (((uintptr_t)workspace & 15) != 0) return fail(COMA_E_INVALID, "%s: workspace must be 16-byte aligned", who);
  FitLayout L;
  if (!fit_layout(V, d->F, J, k, H, NJ, 3 * (long long)NJ + 3 + kLeadFixed + 2 * hs, L))
    return fail(COMA_E_INVALID, "%s: sizes V=%d F=%d J=%d k=%d H=%d NJ=%d outside what the body model, the decoder or the objective accept", who, V,
                d->F, J, k, H, NJ);
  const int n_body = 3 * NJ;

  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float *theta = (float*)(ws + L.theta), *z = (float*)(ws + L.z), *transl = (float*)(ws + L.transl), *aa = (float*)(ws + L.aa);
  float *raw = (float*)(ws + L.raw), *joints = (float*)(ws + L.joints), *terms = (float*)(ws + L.terms);
  float *g_o = (float*)(ws + L.g_o), *g_c = (float*)(ws + L.g_c), *g = (float*)(ws + L.g);
  float *g_theta = (float*)(ws + L.g_theta), *g_transl = (float*)(ws + L.g_transl), *g_aa = (float*)(ws + L.g_aa), *g_z = (float*)(ws + L.g_z);
  double* prior = (double*)(ws + L.prior);

  // the stages' plans, once: each makes its entry point's refusals; nothing is launched, no address is followed on the device
  VposerDecodePlan decode;
  SmplxForwardPlan forward;
  AppObjectivePlan objective;
  SmplxBackwardPlan backward;
  VposerDecodeBackwardPlan decode_bwd;
  if (int rc = vposer_decode_plan(who, z, d->W1, d->b1, d->W2, d->b2, d->W3, d->b3, 1, D, H, NJ, aa, nullptr, nullptr, ws + L.vp_saved, L.vp_saved_bytes,
                                  decode))
    return rc;
  if (int rc = smplx_forward_plan(who, false, 1, 0, theta, transl, d->posedirs, d->weights, d->parents, d->hand_components, d->pose_mean, V, J, hd,
                                  n_pca, d->shape_state, raw, joints, nullptr, ws + L.sx_saved, L.sx_saved_bytes, ws + L.sx_ws, L.sx_ws_bytes, forward))
    return rc;
  if (int rc = app_objective_plan(who, false, 1, d->vertices, d->faces, d->vf_offsets, d->vf_faces, V, d->F, d->orientation_gt, d->obj_normal,
                                  d->principle_vec, d->sub_principle_vec, d->eps, d->selected, d->targets, k, terms, g_o, g_c, ws + L.obj_ws,
                                  L.obj_ws_bytes, objective))
    return rc;
  if (int rc = smplx_backward_plan(who, false, 1, 0, g, d->posedirs, d->weights, d->parents, d->hand_components, V, J, hd, n_pca, d->shape_state,
                                   ws + L.sx_saved, L.sx_saved_bytes, g_theta, g_transl, ws + L.sx_ws, L.sx_ws_bytes, nullptr, backward))
    return rc;
  if (int rc = vposer_decode_backward_plan(who, g_aa, d->W1, d->W2, d->W3, 1, D, H, NJ, ws + L.vp_saved, L.vp_saved_bytes, g_z, ws + L.vp_ws,
                                           L.vp_ws_bytes, decode_bwd))
    return rc;

  // what ties the stages together, and the fit's own arguments
  if (3 * (long long)NJ + 3 + kLeadFixed != 3 * (long long)J - 2 * (long long)hd)
    return fail(COMA_E_INVALID, "%s: the decoder's 3 NJ = %d body-pose entries do not fill the model's 3 J - 2 hand_dim - 12 = %d", who, 3 * NJ,
                3 * J - 2 * hd - 3 - kLeadFixed);
  if (P != 6 + 2 * hs + D) return fail(COMA_E_INVALID, "%s: P=%d, but 6 + 2 hs + D = %d (hs=%d, D=%d)", who, P, 6 + 2 * hs + D, hs, D);
  PriorVec pv = {};
  if (K < 1 || K > kFitMaxK) return fail(COMA_E_INVALID, "%s: prior_K=%d outside [1, %d]", who, K, kFitMaxK);
  pv.K = K;
  for (int i = 0; i < K; ++i) {
    if (d->prior_index[i] < 0 || d->prior_index[i] >= n_body)
      return fail(COMA_E_INVALID, "%s: prior_index[%d]=%d outside [0, %d)", who, i, d->prior_index[i], n_body);
    pv.index[i] = d->prior_index[i], pv.sign[i] = d->prior_sign[i];
  }
  for (double x : {d->lr, d->body_pose_weight, d->bending_prior_weight, d->pprior_weight, d->orientation_weight, d->contact_weight, d->scale_factor})
    if (!std::isfinite(x)) return fail(COMA_E_INVALID, "%s: lr, the weights and scale_factor must be finite", who);
  if (int rc = check_buffer(who, "state", state, state_bytes_, state_bytes(P))) return rc;
  if (int rc = check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
  if (((uintptr_t)d->traj & 7) || ((uintptr_t)d->losses & 7) || ((uintptr_t)d->grad0 & 7) || !f32_aligned({d->vertices, d->lead_fixed}))
    return fail(COMA_E_INVALID, "%s: traj, losses, grad0 must be 8-byte and vertices, lead_fixed 4-byte aligned", who);

  const int n3 = 3 * V;
  const dim3 grid3((unsigned)((n3 + kFitBlock - 1) / kFitBlock)), block(kFitBlock);
  const float scale = (float)d->scale_factor, w_o = (float)d->orientation_weight, w_c = (float)d->contact_weight;
  StepArgs sa = {};
  sa.grad_theta = g_theta, sa.grad_transl = g_transl, sa.grad_z = g_z, sa.terms = terms, sa.prior_sum = prior;
  sa.P = P, sa.hs = hs, sa.D = D, sa.n_body = n_body;
  sa.lr = d->lr, sa.w_body = d->body_pose_weight, sa.w_bend = d->bending_prior_weight, sa.w_prior = d->pprior_weight;
  sa.w_o = d->orientation_weight, sa.w_c = d->contact_weight;
  sa.traj = d->traj, sa.losses = d->losses, sa.grad0 = d->grad0, sa.state = (double*)state;

  for (int e = 0; e < d->E; ++e) {
    hipLaunchKernelGGL(fit_assemble_kernel, dim3(1), block, 0, st, (double*)state, P, hs, D, n_body, d->lead_fixed, theta, z, transl);
    if (int rc = check_launch("fit_assemble_kernel")) return rc;
    if (int rc = vposer_decode_enqueue(decode, st)) return rc;
    hipLaunchKernelGGL(fit_pose_kernel, dim3(1), block, 0, st, (const float*)aa, n_body, pv, theta, prior);
    if (int rc = check_launch("fit_pose_kernel")) return rc;
    if (int rc = smplx_forward_enqueue(forward, st)) return rc;
    hipLaunchKernelGGL(fit_scale_kernel, grid3, block, 0, st, (const float*)raw, n3, scale, d->vertices);
    if (int rc = check_launch("fit_scale_kernel")) return rc;
    if (int rc = app_objective_enqueue(objective, st)) return rc;
    hipLaunchKernelGGL(fit_seed_kernel, grid3, block, 0, st, (const float*)g_o, (const float*)g_c, n3, w_o, w_c, scale, g);
    if (int rc = check_launch("fit_seed_kernel")) return rc;
    if (int rc = smplx_backward_enqueue(backward, st)) return rc;
    hipLaunchKernelGGL(fit_prior_grad_kernel, dim3((unsigned)((n_body + kFitBlock - 1) / kFitBlock)), block, 0, st, (const float*)aa,
                       (const float*)g_theta, n_body, pv, d->bending_prior_weight, g_aa);
    if (int rc = check_launch("fit_prior_grad_kernel")) return rc;
    if (int rc = vposer_decode_backward_enqueue(decode_bwd, st)) return rc;
    sa.e = e;
    hipLaunchKernelGGL(fit_step_kernel, dim3(1), block, 0, st, sa);
    if (int rc = check_launch("fit_step_kernel")) return rc;
  }
  return COMA_OK;
}

extern "C" int coma_app_fit_status(const void* state, void* stream, int* iteration) {
  const char* who = "coma_app_fit_status";
  if (!state) return fail(COMA_E_INVALID, "%s: null pointer", who);
  long long head[4] = {0, 0, 0, 0};
  if (int rc = read_back(head, state, sizeof(head), stream, who)) return rc;
  if (iteration) *iteration = (int)head[kFsIteration];
  const long long P = head[kFsMagic] - kFitMagic;
  if (P < 7 || P > kFitMaxP) {
    if (iteration) *iteration = 0;
    return fail(COMA_E_INVALID, "coma_app_fit_f32: the state was not written by coma_app_fit_init_f64 (nothing written)");
  }
  if (head[kFsStatus] == kFitOtherP)
    return fail(COMA_E_INVALID, "coma_app_fit_f32: the state was initialised for P=%d, not for the call's P (nothing written)", (int)P);
  if (head[kFsStatus] != kFitOk)
    return fail(COMA_E_INVALID, "coma_app_fit_f32: a gradient or an updated parameter is not finite in iteration %d (no step applied from there on)",
                (int)head[kFsIteration]);
  return COMA_OK;
}
