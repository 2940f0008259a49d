// Internal: the tile machinery shared by the C = 320 row-tile kernels (xfront_kernel and xchain_kernel in sd_xchain.hip, xtail_kernel
// in sd_xtail.hip).  A workgroup of NW waves keeps TM token rows on the chip:
//   T  : LDS tile [TM][320] fp16, rows of 640 B with the 16-byte chunks swizzled (tswz) -- the activation operand of the products
//   WB : LDS stages of a weight K-slice [320][32] (rows of 64 B, wswz), filled by LDS-DMA, one barrier per slice
//   MFMA v_mfma_f32_32x32x16_f16 as D = W_frag . A_frag^T: a lane owns one output row of a 32-row tile and, per 32-column tile, four
//   quads of 4 consecutive columns.  Wave (wr, wc) owns RT 32-row tiles and the columns 160 wc .. + 159 (5 tiles).
// Free function templates with every value passed explicitly: carrying the tile state in an object costs xchain_kernel the two
// registers it has left (254 of 256 with two workgroups per CU) and makes it spill.
#pragma once
#include "common.h"
#include "sd_device.h"

namespace sd {
namespace rowtile {

constexpr int C = 320, BK = 32;
constexpr int WB_STAGE = C * BK;                      // halves per [320][32] weight slice
constexpr unsigned OOB = 0x80000000u;                 // buffer offset that fails every range check: the DMA writes zeros

// 16-byte chunk slot of logical chunk c (0..39) in row `row` of T: the 8 chunks of a 128-byte group are permuted with the row,
// rows alternate between the two halves of the 256-byte bank window (640 = 512 + 128) -> conflict-free fragment reads
__device__ __forceinline__ int tswz(int row, int c) { return (c & ~7) | ((c ^ (row >> 1)) & 7); }
// weight slice rows are 64 bytes (4 chunks)
__device__ __forceinline__ int wswz(int row, int c) { return c ^ ((row >> 2) & 3); }

// ---- tile DMA: rows m0 .. m0 + TM - 1 of the [M][320] tensor `src` -> T.  TM rows x 40 chunks = pieces of 1 KiB, 10 per wave;
// lane -> (row, slot) of the piece, source chunk un-swizzled (tswz is an involution); rows at or beyond M arrive as zeros.
template <int TM, int NW>
__device__ __forceinline__ void load_tile(_Float16* T, const _Float16* src, unsigned tensor_bytes, int m0, int M, int wave, int lane) {
  constexpr int PPW = TM * 40 / 64 / NW;
  static_assert(PPW * NW * 64 == TM * 40, "DMA piece counts");
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(src, tensor_bytes);
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int q = (wave * PPW + j) * 64 + lane;
    const int row = q / 40, slot = q - row * 40;
    const unsigned off = (m0 + row) < M ? (unsigned)(((long long)(m0 + row) * C + tswz(row, slot) * 8) * 2) : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)(T + (wave * PPW + j) * 512), 16, off, 0, 0, 0);
  }
#endif
}

// ---- weight slice DMA: a [320 rows][32 k] slice of a row-major [320][320] matrix = 20 pieces of 16 rows, 20 / NW per wave.  The
// lane offsets of slice 0 are computed once per kernel (w_off); slice s is 64 s bytes further along every row.
template <int NW>
__device__ __forceinline__ void slice_offsets(unsigned (&w_off)[20 / NW], int wave, int lane) {
  static_assert(20 % NW == 0, "DMA piece counts");
#pragma unroll
  for (int j = 0; j < 20 / NW; ++j) {
    const int p = wave + NW * j;
    const int row = p * 16 + (lane >> 2), slot = lane & 3;
    w_off[j] = (unsigned)((row * C + wswz(row, slot) * 8) * 2);
  }
}
template <int NW>
__device__ __forceinline__ void issue_w(const __amdgpu_buffer_rsrc_t& rs, _Float16* stage, const unsigned (&w_off)[20 / NW], int s,
                                        int wave) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int j = 0; j < 20 / NW; ++j)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)(stage + (wave + NW * j) * 512), 16, w_off[j] + s * (BK * 2), 0, 0, 0);
#endif
}

// ---- the MFMAs of K-slice s (two steps of 16): acc[i][j] += A[row0 + 32 i][32 s .. + 31] . Wb[n0 + 32 j + l31][0 .. 31]^T.  A is a swizzled
// tile with rows of LDA halves and chunk swizzle SWZ, Wb a landed weight slice.  SWAPPED exchanges the operand roles: a lane then owns
// weight row n0 + 32 j + l31 and 4 consecutive rows of A per quad.
template <int LDA, int (*SWZ)(int, int), bool SWAPPED, int RT, int NT>
__device__ __forceinline__ void slice_mfma(float16v (&acc)[RT][NT], const _Float16* A, const int (&rows)[RT], const _Float16* Wb, int n0,
                                           int s, int l31, int hh) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int ks = 2 * s + kk;
    half8 af[RT], wf[NT];
#pragma unroll
    for (int i = 0; i < RT; ++i) af[i] = *reinterpret_cast<const half8*>(&A[rows[i] * LDA + SWZ(rows[i], 2 * ks + hh) * 8]);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + j * 32 + l31;
      wf[j] = *reinterpret_cast<const half8*>(&Wb[n * BK + wswz(n, 2 * kk + hh) * 8]);
    }
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[i][j] = SWAPPED ? __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], wf[j], acc[i][j], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], af[i], acc[i][j], 0, 0, 0);
  }
}

// ---- acc = T[rows of this wave][320] . W[320][320]^T for the wave's 32 x 160 patch: 10 slices through two stages of WB, one barrier
// per slice.  Entry: T complete and visible (a barrier has passed).  Exit: every wave is done reading T and WB.
template <int NW, bool SWAPPED>
__device__ __forceinline__ void product320(float16v (&acc)[1][5], const _Float16* T, _Float16* WB, const _Float16* w,
                                           const unsigned (&w_off)[20 / NW], const int (&rows)[1], int wave, int wc, int l31, int hh) {
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(w, (unsigned)(C * C * 2));
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.0f;
  issue_w<NW>(rs, WB, w_off, 0, wave);
#pragma unroll 1
  for (int s = 0; s < C / BK; ++s) {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                    // slice s landed everywhere; every wave is done with the other stage
    if (s + 1 < C / BK) issue_w<NW>(rs, WB + ((s + 1) & 1) * WB_STAGE, w_off, s + 1, wave);
    slice_mfma<C, tswz, SWAPPED>(acc, T, rows, WB + (s & 1) * WB_STAGE, wc * 160, s, l31, hh);
  }
  __builtin_amdgcn_s_barrier();
}

// ---- accumulators -> tile.  Register quad (j, rg) of a lane = the 4 consecutive columns from quad_col(j, rg) of the lane's row in each
// of the wave's RT row tiles (rows row0, row0 + 32, ...).
__device__ __forceinline__ int quad_col(int wc, int hh, int j, int rg) { return wc * 160 + j * 32 + 8 * rg + 4 * hh; }
__device__ __forceinline__ _Float16* quad_ptr(_Float16* tile, int row, int col) { return &tile[row * C + tswz(row, col >> 3) * 8 + (col & 7)]; }
// dst <- fp16(acc (+ bias if BIAS) (+ dst if ADD)) for the wave's RT x 5 tiles; each quad is read and written by the lane that owns it
template <int RT, bool BIAS, bool ADD>
__device__ __forceinline__ void write_acc(const float16v (&acc)[RT][5], const int (&rows)[RT], const _Float16* bias, _Float16* dst, int wc,
                                          int hh) {
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        _Float16* p = quad_ptr(dst, rows[i], quad_col(wc, hh, j, rg));
        float v[4] = {acc[i][j][rg * 4 + 0], acc[i][j][rg * 4 + 1], acc[i][j][rg * 4 + 2], acc[i][j][rg * 4 + 3]};
        if constexpr (BIAS) {
          const half4 bv = *reinterpret_cast<const half4*>(bias + quad_col(wc, hh, j, rg));
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)bv[e];
        }
        if constexpr (ADD) {
          const half4 tv = *reinterpret_cast<const half4*>(p);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)tv[e];
        }
        *reinterpret_cast<half4*>(p) = half4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      }
}

// ---- row passes over a swizzled [TM][320] tile: 4 lanes per row, 10 chunks of 16 bytes each.
// store_rows: the rows -> global [M][ld] at column offset col0, coalesced 16-byte stores
template <int TM, int NW>
__device__ __forceinline__ void store_rows(const _Float16* tile, _Float16* out, int ld, int col0, int m0, int M, int tid) {
  const int qtr = tid & 3;
#pragma unroll
  for (int row = tid >> 2; row < TM; row += NW * 16)
    if (m0 + row < M)
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        const int c = qtr * 10 + i;
        *reinterpret_cast<half8*>(out + (long long)(m0 + row) * ld + col0 + c * 8) = *reinterpret_cast<const half8*>(&tile[row * C + tswz(row, c) * 8]);
      }
}
// layernorm_rows (TM = 16 NW): stores the row as it stands in T to res_out (unless null), LayerNorms it (mean / variance with two lane
// exchanges) and either writes the normalised row back into T (ln_out == nullptr) or stores it to ln_out.  The row stays in 40
// registers between the two sweeps (xfront_kernel, which cannot afford them, keeps a re-reading form of its own).
__device__ __forceinline__ void layernorm_rows(_Float16* T, _Float16* res_out, const _Float16* gamma, const _Float16* beta,
                                               _Float16* ln_out, float eps, int m0, int M, int tid) {
  const int row = tid >> 2, qtr = tid & 3;
  const bool ok = m0 + row < M;
  half8 x[10];
  float sum = 0.0f, sq = 0.0f;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int c = qtr * 10 + i;
    x[i] = *reinterpret_cast<const half8*>(&T[row * C + tswz(row, c) * 8]);
    if (ok && res_out) *reinterpret_cast<half8*>(res_out + (long long)(m0 + row) * C + c * 8) = x[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float f = (float)x[i][e]; sum += f; sq += f * f; }
  }
  sum += __shfl_xor(sum, 1); sq += __shfl_xor(sq, 1);
  sum += __shfl_xor(sum, 2); sq += __shfl_xor(sq, 2);
  const float mean = sum * (1.0f / C);
  const float var = fmaxf(sq * (1.0f / C) - mean * mean, 0.0f);
  const float rstd = rsqrtf(var + eps);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int c = qtr * 10 + i;
    const half8 gm = *reinterpret_cast<const half8*>(gamma + c * 8), bt = *reinterpret_cast<const half8*>(beta + c * 8);
    half8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (_Float16)(((float)x[i][e] - mean) * rstd * (float)gm[e] + (float)bt[e]);
    if (ln_out) { if (ok) *reinterpret_cast<half8*>(ln_out + (long long)(m0 + row) * C + c * 8) = y; }
    else *reinterpret_cast<half8*>(&T[row * C + tswz(row, c) * 8]) = y;
  }
}

// ---- host: the tail of an entry point -- opt the kernel into its LDS (once per device), launch one workgroup per TM rows, report
template <auto KERNEL, class Args>
int launch(const Args& g, int64_t rows, int tm, int nw, int lds_bytes, const char* entry, const char* kernel_name, void* stream) {
  static coma::LdsOptIn lds_opt;
  if (int rc = coma::opt_in_lds(lds_opt, reinterpret_cast<const void*>(KERNEL), lds_bytes, entry)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)(rows / tm)), dim3(nw * 64), lds_bytes, (hipStream_t)stream, g);
  return coma::check_launch(kernel_name);
}

}  // namespace rowtile
}  // namespace sd
