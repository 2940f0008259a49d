// sd_text.hip -- the two kernels of the CLIP text tower that the UNet / VAE operators do not already cover (gfx950, fp16 storage,
// fp32 accumulate): token + position embedding, and causal multi-head self-attention over short sequences.
//
// The SD-1.x text encoder is transformers' CLIPTextModel (hidden 768, 12 pre-LayerNorm layers, 12 heads of 64, quick_gelu MLP, 77
// positions), which the reference runs in eager fp16 (utils/adaptive_mask_inpainting.py:459-482 `self.text_encoder(...)`).  Everything
// else of the tower is sd_layernorm_f16 and sd_conv_gemm_f16 (fused q|k|v product, out_proj / fc2 with the residual epilogue, fc1 with
// SD_EPI_QUICK_GELU); coma_amd/sd/text.py records the launch list.
#include <hip/hip_fp16.h>

#include "common.h"
#include "sd_plan.h"
#include "../../include/sd_hip.h"

namespace sd {

using coma::check_launch;
using coma::fail;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// out[row, :] = tok[clamp(ids[row])] + pos[row % len]: one wave per row, 8 channels per lane and step.  The sum is formed in fp32 and
// rounded once (what torch's fp16 `tok[ids] + pos` computes).
__global__ __launch_bounds__(64) void text_embed_kernel(const int32_t* __restrict__ ids, int len, const _Float16* __restrict__ tok, int vocab,
                                                        const _Float16* __restrict__ pos, int width, _Float16* __restrict__ out) {
  const long long row = blockIdx.x;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);          // a bad id never reads outside the table
  const int p = (int)(row % len);
  const half8* t = reinterpret_cast<const half8*>(tok + (long long)id * width);
  const half8* q = reinterpret_cast<const half8*>(pos + (long long)p * width);
  half8* o = reinterpret_cast<half8*>(out + row * width);
  for (int c = threadIdx.x; c < width / 8; c += 64) {
    const half8 a = t[c], b = q[c];
    half8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (_Float16)((float)a[e] + (float)b[e]);
    o[c] = r;
  }
}

// Causal attention, d = 64, len <= 128: one workgroup (4 waves) per (sequence, head).  Q, K and V of the pair are staged in LDS (K rows
// padded to 72 halves: the 16 lanes of a ds_read_b128 group read 16 distinct 16-byte slots); a wave owns query i: lane j holds the
// fp32 scores of keys j and j + 64, the masked row max / sum are wave reductions (the whole row is in registers: an exact softmax, no
// online rescale), the probabilities go through LDS, and lane c accumulates output channel c over keys 0..i only -- keys after i are
// never read, so they cannot change the result.
constexpr int CA_MAXL = 128, CA_D = 64, CA_KST = CA_D + 8;

__global__ __launch_bounds__(256) void attention_causal_kernel(const _Float16* __restrict__ q, const _Float16* __restrict__ k,
                                                               const _Float16* __restrict__ v, _Float16* __restrict__ out, int len, int ldq,
                                                               int ldk, int ldv, int ldo, float scale) {
  __shared__ __attribute__((aligned(16))) _Float16 qs[CA_MAXL * CA_D];
  __shared__ __attribute__((aligned(16))) _Float16 ks[CA_MAXL * CA_KST];
  __shared__ __attribute__((aligned(16))) _Float16 vs[CA_MAXL * CA_D];
  __shared__ __attribute__((aligned(16))) float ps[4][CA_MAXL];
  const int h = blockIdx.x, s = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long row0 = (long long)s * len;
  for (int c = tid; c < len * (CA_D / 8); c += 256) {
    const int r = c >> 3, e = (c & 7) * 8;
    const long long g = row0 + r;
    *reinterpret_cast<half8*>(qs + r * CA_D + e) = *reinterpret_cast<const half8*>(q + g * ldq + h * CA_D + e);
    *reinterpret_cast<half8*>(ks + r * CA_KST + e) = *reinterpret_cast<const half8*>(k + g * ldk + h * CA_D + e);
    *reinterpret_cast<half8*>(vs + r * CA_D + e) = *reinterpret_cast<const half8*>(v + g * ldv + h * CA_D + e);
  }
  __syncthreads();
  for (int i0 = 0; i0 < len; i0 += 4) {          // uniform trip count: every wave reaches the barriers below
    const int i = i0 + wave;
    if (i < len) {
      const int j0 = lane, j1 = lane + 64;
      float s0 = 0.0f, s1 = 0.0f;
      const _Float16* k0 = ks + j0 * CA_KST;
      const _Float16* k1 = ks + j1 * CA_KST;
#pragma unroll
      for (int e = 0; e < CA_D; e += 8) {
        const half8 qv = *reinterpret_cast<const half8*>(qs + i * CA_D + e);     // broadcast
        const half8 a = *reinterpret_cast<const half8*>(k0 + e);
        const half8 b = *reinterpret_cast<const half8*>(k1 + e);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          s0 = fmaf((float)qv[t], (float)a[t], s0);
          s1 = fmaf((float)qv[t], (float)b[t], s1);
        }
      }
      const bool v0 = j0 <= i, v1 = j1 <= i;
      s0 *= scale;
      s1 *= scale;
      float m = fmaxf(v0 ? s0 : -__builtin_inff(), v1 ? s1 : -__builtin_inff());
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      const float e0 = v0 ? __expf(s0 - m) : 0.0f, e1 = v1 ? __expf(s1 - m) : 0.0f;
      float sum = e0 + e1;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
      const float inv = 1.0f / sum;
      ps[wave][j0] = e0 * inv;
      ps[wave][j1] = e1 * inv;
    }
    __syncthreads();
    if (i < len) {
      float acc = 0.0f;
      const float* p = ps[wave];
      int j = 0;
      for (; j + 4 <= i + 1; j += 4) {
        const float4 pv = *reinterpret_cast<const float4*>(p + j);           // broadcast
        acc = fmaf(pv.x, (float)vs[(j + 0) * CA_D + lane], acc);
        acc = fmaf(pv.y, (float)vs[(j + 1) * CA_D + lane], acc);
        acc = fmaf(pv.z, (float)vs[(j + 2) * CA_D + lane], acc);
        acc = fmaf(pv.w, (float)vs[(j + 3) * CA_D + lane], acc);
      }
      for (; j <= i; ++j) acc = fmaf(p[j], (float)vs[j * CA_D + lane], acc);
      out[(row0 + i) * ldo + h * CA_D + lane] = (_Float16)acc;
    }
    __syncthreads();                             // ps[wave] is rewritten by the next query
  }
}

}  // namespace sd

using namespace sd;

// PK_TEXT_EMBED / PK_ATTN_CAUSAL are appended to the record kinds: the kinds of existing model files keep their values
static_assert(PK_TEXT_EMBED == PK_SEG + 1 && PK_ATTN_CAUSAL == PK_SEG + 2 && PK_COUNT_ == PK_ATTN_CAUSAL + 1,
              "new plan record kinds go just before PK_COUNT_");

extern "C" int sd_text_embed_f16(const int32_t* ids, int seqs, int len, const void* tok_emb, int vocab, const void* pos_emb, int n_pos,
                                 int width, void* out, void* stream) {
  if (plan_recording()) return record<PK_TEXT_EMBED>(ids, seqs, len, tok_emb, vocab, pos_emb, n_pos, width, out);
  if (!ids || !tok_emb || !pos_emb || !out) return fail(COMA_E_INVALID, "sd_text_embed_f16: null pointer");
  if (seqs <= 0 || len <= 0 || vocab <= 0 || n_pos < len || width <= 0 || width % 8)
    return fail(COMA_E_INVALID, "sd_text_embed_f16: bad sizes (seqs=%d len=%d vocab=%d n_pos=%d width=%d; n_pos >= len, width %% 8 == 0)", seqs, len,
                vocab, n_pos, width);
  if ((long long)seqs * len > 0x7fffffffLL) return fail(COMA_E_INVALID, "sd_text_embed_f16: too many rows");
  if (((uintptr_t)tok_emb | (uintptr_t)pos_emb | (uintptr_t)out) & 15) return fail(COMA_E_INVALID, "sd_text_embed_f16: tables and output must be 16-byte aligned");
  hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)(seqs * len)), dim3(64), 0, (hipStream_t)stream, ids, len, (const _Float16*)tok_emb,
                     vocab, (const _Float16*)pos_emb, width, (_Float16*)out);
  return check_launch("text_embed_kernel");
}

extern "C" int sd_attention_causal_f16(const void* q, const void* k, const void* v, void* out, int seqs, int heads, int len, int d, int ldq,
                                       int ldk, int ldv, int ldo, float scale, void* stream) {
  if (plan_recording()) return record<PK_ATTN_CAUSAL>(q, k, v, out, seqs, heads, len, d, ldq, ldk, ldv, ldo, scale);
  if (!q || !k || !v || !out) return fail(COMA_E_INVALID, "sd_attention_causal_f16: null pointer");
  if (d != CA_D) return fail(COMA_E_INVALID, "sd_attention_causal_f16: head dim must be %d (got %d)", CA_D, d);
  if (len < 1 || len > CA_MAXL) return fail(COMA_E_INVALID, "sd_attention_causal_f16: sequence length must be 1..%d (got %d)", CA_MAXL, len);
  if (seqs <= 0 || heads <= 0 || seqs > 65535 || heads > 65535) return fail(COMA_E_INVALID, "sd_attention_causal_f16: bad seqs / heads");
  const int w = heads * d;
  if (ldq < w || ldk < w || ldv < w || ldo < w || ldq % 8 || ldk % 8 || ldv % 8)
    return fail(COMA_E_INVALID, "sd_attention_causal_f16: leading dimensions must cover heads * d and q / k / v ones be multiples of 8");
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return fail(COMA_E_INVALID, "sd_attention_causal_f16: q / k / v must be 16-byte aligned");
  if (((uintptr_t)out) & 1) return fail(COMA_E_INVALID, "sd_attention_causal_f16: out must be 2-byte aligned");
  hipLaunchKernelGGL(attention_causal_kernel, dim3((unsigned)heads, (unsigned)seqs), dim3(256), 0, (hipStream_t)stream, (const _Float16*)q,
                     (const _Float16*)k, (const _Float16*)v, (_Float16*)out, len, ldq, ldk, ldv, ldo, scale);
  return check_launch("attention_causal_kernel");
}
