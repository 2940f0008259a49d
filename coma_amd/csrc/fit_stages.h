// Internal: what app_fit.hip needs of vposer.hip, smplx.hip and app_objective.hip -- every stage of a fit iteration as a PLAN, made once,
// and an ENQUEUE, made per iteration.  X_plan(who, the entry point's arguments, plan) gives every refusal of the stage's entry point in
// its words and order, under the caller's name, fills the plan and launches nothing; X_enqueue(plan, stream) does the launches (a
// memset included) and nothing else.  A plan is a value on the caller's stack: the kernel-argument structs, the grids and the few
// scalars its launches need; the pointers in it are the caller's.  The public entry points are plan, then enqueue.
#pragma once
#include "common.h"

namespace coma {

// ---- vposer.hip: the pose decoder, any N ----
struct VposerDecodePlan {
  const char* who;
  const float *z, *W1, *b1, *W2, *b2, *W3, *b3;
  int N, D, H, NJ;
  double *h1, *h2, *o;          // the saved block's fields
  int8_t* saved_branch;
  float* aa;
  float* matrices;              // may be null
  int8_t* branch;               // may be null
};
int vposer_decode_plan(const char* who, const float* z, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                       const float* b3, int N, int D, int H, int NJ, float* aa, float* matrices, int8_t* branch, void* saved, size_t saved_bytes,
                       VposerDecodePlan& p);
int vposer_decode_enqueue(const VposerDecodePlan& p, hipStream_t s);

struct VposerDecodeBackwardPlan {
  const char* who;
  const float *grad_aa, *W1, *W2, *W3;
  int N, D, H, NJ;
  const double *h1, *h2, *o;    // the saved block's fields
  const int8_t* saved_branch;
  double *go, *gh2, *gh1;       // the workspace's
  float* grad_z;
};
int vposer_decode_backward_plan(const char* who, const float* grad_aa, const float* W1, const float* W2, const float* W3, int N, int D, int H,
                                int NJ, const void* saved, size_t saved_bytes, float* grad_z, void* workspace, size_t workspace_bytes,
                                VposerDecodeBackwardPlan& p);
int vposer_decode_backward_enqueue(const VposerDecodeBackwardPlan& p, hipStream_t s);

// ---- smplx.hip: the body model, N bodies; the single-body, full and batched entry points all go through these ----
constexpr int kMaxJ = 64;         // joints (the chain kernels keep the whole tree in LDS)

struct Tree { int32_t parent[kMaxJ]; };

// How a kernel finds body n of N from body 0's pointers: the f32 arrays and the workspace blocks are dense [N, ...]; the shape
// states and saved blocks are `shape` / `saved` bytes apart.
struct BatchStrides {
  int N, NT;                // bodies; entries of one body's theta
  size_t shape, saved;      // bytes; shape = 0: one shape state for all bodies
};

struct PoseArgs {           // the pointers are body 0's
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

struct SkinArgs {           // the pointers are body 0's
  const float* weights;     // [V,J]
  const double* A;          // [J,12]
  const double* v_shaped;   // [V,3]
  const double* part;       // [kPSplit][3V]
  const float* transl;      // [3] or null
  int V, J;
  double* v_posed;          // saved [V,3]
  float* vertices;          // [V,3]
};

struct PoseBwdArgs {        // the pointers are body 0's
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

// the grids of a call's launches and the instantiation that goes with them
struct SmplxGrids {
  int P, rows, nblk, nb3;
  int C, chunks, B, skin_chunks;                  // bodies per sweep over posedirs and per skinning workgroup (the instantiation), and their chunks
};

struct SmplxForwardPlan {
  const char* who;
  SmplxGrids g;
  BatchStrides strides;
  PoseArgs pose;
  const float* posedirs;
  double* part;               // workspace [N][kPSplit][3V]: written by the offsets launch, read as skin.part
  SkinArgs skin;
};
// `batched` only says which workspace the ABI gives the call: the single-body one also holds the vertices-only backward's blocks.
int smplx_forward_plan(const char* who, bool batched, int N, size_t shape_stride, const float* theta, const float* transl, const float* posedirs,
                       const float* weights, const int32_t* parents, const float* hand_components, const float* pose_mean, int V, int J,
                       int hand_dim, int n_pca, const void* shape_state, float* vertices, float* joints, float* full_pose, void* saved,
                       size_t saved_bytes, void* workspace, size_t workspace_bytes, SmplxForwardPlan& p);
int smplx_forward_enqueue(const SmplxForwardPlan& p, hipStream_t s);

// what the full and the batched backward take besides dL/dvertices; every pointer may be null
struct FullBwd {
  const float* grad_joints;
  const float* grad_full_pose;
  const int32_t* extra_index;
  const float* extra_weight;
  int E;
  // the gradient to the coefficients, which the batched ABI does not have
  const float* shapedirs;
  const float* J_regressor;
  int NB;
  float* grad_coefficients;
};

struct SmplxBackwardPlan {
  const char* who;
  SmplxGrids g;
  BatchStrides strides;
  int V;
  const float* posedirs;
  const float* weights;
  const double *s_A, *s_vposed;       // of the saved block
  const float* grad_vertices;         // the caller's; may be null in the full backward
  // only when the gradient at the vertices differs from the caller's (g_eff non-null): the extra joints' rows scattered into it
  double* g_eff;
  const float* gJ_extra;
  size_t gJ_stride;
  const int32_t* extra_index;
  const float* extra_weight;
  int E;
  double *gvp, *dA_part, *dfeat;      // workspace; pose reads the last two
  PoseBwdArgs pose;
  // the gradient to the coefficients (grad_coefficients non-null): pose.dJ_out, then these
  const float* shapedirs;
  const float* J_regressor;
  int NB;
  double* coef_part;
  float* grad_coefficients;
};
// `full` null is the vertices-only backward on the single-body workspace (its blocks behind the forward's); otherwise the backward
// workspace from its start, up to g_eff for the batched ABI and whole for the full backward.
int smplx_backward_plan(const char* who, bool batched, int N, size_t shape_stride, const float* grad_vertices, const float* posedirs,
                        const float* weights, const int32_t* parents, const float* hand_components, int V, int J, int hand_dim, int n_pca,
                        const void* shape_state, const void* saved, size_t saved_bytes, float* grad_theta, float* grad_transl, void* workspace,
                        size_t workspace_bytes, const FullBwd* full, SmplxBackwardPlan& p);
int smplx_backward_enqueue(const SmplxBackwardPlan& p, hipStream_t s);

// ---- app_objective.hip: the ComA objective, N bodies ----
struct AppArgs {
  const float* verts;
  const int32_t* faces;
  const int32_t* off;
  const int32_t* vf;
  const float* gt;
  int V, F;
  double M[9];     // f = M a (row-major), built on the host
  double eps;
  double* gN;      // [N][V,3] d term / d N_h
  double* part_o;  // [N][ceil(V / 256)]
};

struct ContactArgs {
  const float* verts;
  const int32_t* sel;
  const float* targets;
  int V, k, nsplit;
  const float* pmin;     // [N][2][nsplit][k]
  const int32_t* parg;   // [N][2][nsplit][k]
  double* dist;          // [N][2][k]  |A_i - B_argmin| and |A_argmin - B_j| in f64
  int32_t* arg;          // [N][2][k]
  double* part_c;        // [N][2][ceil(k / 256)]
};

struct AppObjectivePlan {
  const char* who;
  int N, nb_v, nb_k, row_blocks, chunk;
  AppArgs vertex;             // M computed by the plan
  ContactArgs contact;        // launched with contact.k > 0
  float* pmin;                // workspace: written by the two row-minimum launches, read as contact.pmin / contact.parg
  int32_t* parg;
  float *terms, *grad_orientation, *grad_contact;
};
int app_objective_plan(const char* who, bool batched, int N, const float* verts, const int32_t* faces, const int32_t* vf_offsets,
                       const int32_t* vf_faces, int V, int F, const float* orientation_gt, const float* obj_normal, const float* principle_vec,
                       const float* sub_principle_vec, double eps, const int32_t* selected, const float* targets, int k, float* terms,
                       float* grad_orientation, float* grad_contact, void* workspace, size_t workspace_bytes, AppObjectivePlan& p);
int app_objective_enqueue(const AppObjectivePlan& p, hipStream_t s);

}  // namespace coma
