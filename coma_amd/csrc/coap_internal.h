// Internal: what depth_opt.hip needs of coap.hip -- the epoch's COAP collision term as launches on a stream, arguments already checked.
#pragma once
#include "common.h"

namespace coma {

size_t coap_weights_floats(int K);   // K in [1, 32]

// the argument checks shared (front: three doubles on the host) by coma_coap_collision_f32 and coma_depth_optimize_coap_f64 (no launch)
int coap_collision_check(const char* who, const float* weights, const void* code, int K, const float* points, int T, const double* front,
                         double filter_threshold, const void* workspace, size_t workspace_bytes);

// reset, list (bounding-box prefilter, per-part boxes), the fused query with the derivative, the fixed-shape sum: result[0] = loss,
// result[1] = d loss / d d, *kept (may be NULL) = the number of points past the filter.  `stop` (may be NULL): an optimiser's state
// block; nothing is computed once its status word (index 4, in units of 8 bytes) is set.
int coap_collision_launch(const float* weights, const void* code, int K, const float* points, int T, const double* d, const double* front,
                          double filter_threshold, double* result, long long* kept, void* workspace, const long long* stop, hipStream_t st);

}  // namespace coma
