// Internal: recording hook shared by the sd_* / seg_* launch entry points, and the replay table (see sd_plan.hip).
#pragma once
#include <array>
#include <cstdint>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../../include/sd_hip.h"
#include "../../include/seg_hip.h"

namespace sd {

enum PlanKind : int { PK_CONV = 1, PK_GN, PK_GN_COLSTATS, PK_LN, PK_ATTN, PK_SOFTMAX, PK_TEMB, PK_COPY, PK_ATTN_WIDE, PK_XCHAIN, PK_XFRONT, PK_GN_TABLE, PK_XTAIL, PK_CONV_SMALL_N, PK_WINO_IN, PK_WINO_OUT, PK_GN_WINO_IN, PK_IM2COL_C3, PK_GN_TABLE_CAT, PK_CONV_HALO, PK_CONV_C3, PK_SEG,
                     PK_TEXT_EMBED, PK_ATTN_CAUSAL,   // appended (CLIP text tower): kinds are stored in model files, new ones go last
                     PK_COUNT_ };

// One recorded launch: every pointer argument in p[], every integer in i[], every float in f[].  Pointers are kept apart so that a
// saved model can be relocated.  The layout is part of the model file format (tests/test_plan_records.py pins it): a kind stores its
// entry point's arguments, the trailing stream dropped, each array filled in argument order -- PK_SEG from i[1] on, i[0] holding the
// SEG_OP_* code of include/seg_hip.h.  record<>() packs and replay<>() unpacks by the parameter types of the kind's entry<> below, so
// the two cannot disagree.  The records that do not follow argument order are written by hand, pack and unpack side by side in sd_plan.hip.
struct PlanRec {
  int kind;
  int reserved;
  void* p[16];
  int64_t i[24];
  double f[4];
};

bool plan_recording();                 // is this thread recording into a model?
int plan_record(const PlanRec& r);     // append; returns COMA_OK

// hand-written records (sd_plan.hip): a descriptor, host arrays of levels
int record_conv(const sd_conv_gemm_desc* d);
int record_seg_conv(const seg_conv_desc* d);
int record_rpn_select_levels(const void* const* preds, const void* const* cell_anchors, const int* fh, const int* fw, int n_levels, int first_stride,
                             int ld, int batch, int pre_topk, float img_h, float img_w, int cap, void* cand_keys, void* cand_boxes,
                             void* cand_group, void* key_scratch);
// entry points with their arguments in the order their records store them (sd_plan.hip)
int winograd_input_stored(const void* x0, const void* x1, void* v, const float* gn_affine, int c0, int c1, int batch, int h, int w, int upsample,
                          int silu, float vscale, void* stream);
int xattn_chain_stored(const void* attn1_out, const void* h, const void* wo1, const void* bo1, const void* gamma2, const void* beta2,
                       const void* wq2, const void* k2, const void* vt2, const void* wo2, const void* bo2, const void* gamma3, const void* beta3,
                       void* h2, void* n3, int64_t rows, int rows_per_sample, int lk, int ldv2, float eps, void* stream);

// ---- the replay table: the entry point a record of kind Kind (PK_SEG: of operator Op) replays.  launch() in sd_plan.hip dispatches
// on the same kinds; PK_CONV, SEG_OP_CONV and SEG_OP_RPN_SELECT_LEVELS are the hand-written records above.
template <int Kind, int Op = 0> inline constexpr auto entry = nullptr;
template <> inline constexpr auto entry<PK_GN> = sd_groupnorm_f16;
template <> inline constexpr auto entry<PK_GN_COLSTATS> = sd_groupnorm_colstats_f16;
template <> inline constexpr auto entry<PK_LN> = sd_layernorm_f16;
template <> inline constexpr auto entry<PK_ATTN> = sd_attention_f16;
template <> inline constexpr auto entry<PK_SOFTMAX> = sd_softmax_f16;
template <> inline constexpr auto entry<PK_TEMB> = sd_timestep_embedding_f16;
template <> inline constexpr auto entry<PK_COPY> = sd_copy_d2d;
template <> inline constexpr auto entry<PK_ATTN_WIDE> = sd_attention_wide_f16;
template <> inline constexpr auto entry<PK_XCHAIN> = xattn_chain_stored;
template <> inline constexpr auto entry<PK_XFRONT> = sd_xfront_f16;
template <> inline constexpr auto entry<PK_GN_TABLE> = sd_groupnorm_table_f16;
template <> inline constexpr auto entry<PK_XTAIL> = sd_xtail_f16;
template <> inline constexpr auto entry<PK_CONV_SMALL_N> = sd_conv3x3_small_n_f16;
template <> inline constexpr auto entry<PK_WINO_IN> = winograd_input_stored;
template <> inline constexpr auto entry<PK_WINO_OUT> = sd_winograd_output_f16;
template <> inline constexpr auto entry<PK_GN_WINO_IN> = sd_gn_winograd_input_f16;
template <> inline constexpr auto entry<PK_IM2COL_C3> = sd_im2col3x3_c3_f16;
template <> inline constexpr auto entry<PK_GN_TABLE_CAT> = sd_groupnorm_table_cat_f16;
template <> inline constexpr auto entry<PK_CONV_HALO> = sd_conv3x3_halo_f16;
template <> inline constexpr auto entry<PK_CONV_C3> = sd_conv3x3_c3_f16;
template <> inline constexpr auto entry<PK_TEXT_EMBED> = sd_text_embed_f16;
template <> inline constexpr auto entry<PK_ATTN_CAUSAL> = sd_attention_causal_f16;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_RESIZE> = seg_resize_normalize_u8;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_MAXPOOL> = seg_maxpool3x3s2_f32;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_SUBSAMPLE> = seg_subsample2_f32;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_MEMSET> = seg_memset;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_RPN_SELECT> = seg_rpn_select;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_SORT> = seg_sort_candidates;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_NMS> = seg_nms;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_ROI_ALIGN> = seg_roi_align_f32;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_BOX_PREDICT> = seg_box_predict;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_FINALIZE> = seg_finalize_detections;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_POINT_SAMPLE> = seg_point_sample_f32;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_UPSAMPLE2X> = seg_upsample2x_f32;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_TOPK_POINTS> = seg_topk_points;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_POINT_LOGIT> = seg_point_logit_scatter;
template <> inline constexpr auto entry<PK_SEG, SEG_OP_PASTE> = seg_paste_masks;

// ---- signature-driven packing
namespace rec {
enum Slot { P, I, F };
template <class T> constexpr Slot slot_of() {
  if constexpr (std::is_pointer_v<T>) return P;
  else if constexpr (std::is_integral_v<T>) return I;
  else { static_assert(std::is_floating_point_v<T>, "a recorded argument is a pointer, an integer or a float"); return F; }
}
// where each of the arguments T... goes in its array (i[] starting at i0), and how many of each there are
template <int i0, class... T> struct Layout {
  static constexpr std::array<Slot, sizeof...(T)> slot{slot_of<T>()...};
  static constexpr std::array<int, 3> count = [] { std::array<int, 3> n{0, i0, 0}; for (Slot s : slot) ++n[s]; return n; }();
  static constexpr std::array<int, sizeof...(T)> index = [] {
    std::array<int, 3> n{0, i0, 0};
    std::array<int, sizeof...(T)> at{};
    for (size_t k = 0; k < sizeof...(T); ++k) at[k] = n[slot[k]]++;
    return at;
  }();
};
template <class T> void put(PlanRec& r, int k, T v) {
  if constexpr (slot_of<T>() == P) r.p[k] = const_cast<void*>(static_cast<const void*>(v));
  else if constexpr (slot_of<T>() == I) r.i[k] = static_cast<int64_t>(v);
  else r.f[k] = static_cast<double>(v);
}
template <class T> T get(const PlanRec& r, int k) {
  if constexpr (slot_of<T>() == P) return static_cast<T>(r.p[k]);
  else if constexpr (slot_of<T>() == I) return static_cast<T>(r.i[k]);
  else return static_cast<T>(r.f[k]);
}
template <int i0, class... P> int call(int (*fn)(P...), const PlanRec& r, void* stream) {      // the last of P... is the stream
  using L = Layout<i0, P...>;
  return [&]<size_t... K>(std::index_sequence<K...>) {
    return fn(get<std::tuple_element_t<K, std::tuple<P...>>>(r, L::index[K])..., stream);
  }(std::make_index_sequence<sizeof...(P) - 1>{});
}
}  // namespace rec

// Record a launch of entry<Kind, Op> with the arguments `a` (the stream left out): `if (plan_recording()) return record<PK_LN>(x, rows, ...);`
template <int Kind, int Op = 0, class... A> int record(A... a) {
  static_assert(std::is_same_v<int (*)(A..., void*), std::remove_const_t<decltype(entry<Kind, Op>)>>,
                "record<Kind, Op>(args): the argument types must be the parameters of entry<Kind, Op>, the stream left out");
  constexpr int i0 = Kind == PK_SEG ? 1 : 0;
  using L = rec::Layout<i0, A...>;
  static_assert(L::count[rec::P] <= 16 && L::count[rec::I] <= 24 && L::count[rec::F] <= 4, "the arguments do not fit a PlanRec");
  PlanRec r{};
  r.kind = Kind;
  if constexpr (i0) r.i[0] = Op;
  [&]<size_t... K>(std::index_sequence<K...>) { (rec::put(r, L::index[K], a), ...); }(std::index_sequence_for<A...>{});
  return plan_record(r);
}

// Replay a record of kind Kind (operator Op): entry<Kind, Op> called with the arguments record<Kind, Op> stored.
template <int Kind, int Op = 0> int replay(const PlanRec& r, void* stream) {
  return rec::call<Kind == PK_SEG ? 1 : 0>(entry<Kind, Op>, r, stream);
}

}  // namespace sd
