// The column crossings of two meshes as a shared stage (include/coma_hip.h states the rule set): workspace header and layout, the
// limits, and the launcher of everything up to the filled, unsorted per-column lists.  Shared by mesh_volume.hip (one sweep per
// column: the intersection volume) and depth_opt.hip (the lists sorted once and kept: the shift profile of the depth optimisation),
// so that the two cannot drift apart.  The kernels themselves live in mesh_volume.hip.
#pragma once
#include "coma_device.h"
#include "raster_common.h"

namespace coma {

constexpr int kSortMax = 16;                       // crossings per column sorted in LDS: 256 lanes x 16 x 8 B = 32 KiB
constexpr int kScanItems = 4;                      // columns per thread of the scan kernels
constexpr int kScanBlock = 256 * kScanItems;
constexpr long long kZLimit = 1ll << 40;
constexpr long long kMaxCapacity = 0x7fffffffll;   // offsets are 32-bit
enum { kBadDepth = 8, kBadCapacity = 16 };
// header, as 16 ints: [0] status, [1] / [2] length of the work list of A / B, [3] a refused depth was met, then int64 at byte 16:
// crossings counted, 24 / 32 / 40: L_AB, L_A, L_B.  The count kernels test hdr[0] before their barriers, so nothing may change it
// while they run: they raise hdr[3], and the scan folds it into the status word.
enum { kHdrNeeded = 2, kHdrSums = 3 };             // in units of int64

// a crossing as stored: Z << 2 | mesh << 1 | (sigma > 0)
__device__ __forceinline__ long long pack_crossing(long long Z, int mesh, bool flipped) {
  return Z * 4 + (mesh << 1) + (flipped ? 0 : 1);
}

struct ColumnsLayout {
  size_t sv_a, sv_b, big_a, big_b, cnt, block_sums, entries, total;
  int scan_blocks;
};

inline ColumnsLayout columns_layout(int VA, int FA, int VB, int FB, int W, int H, long long capacity) {
  ColumnsLayout l;
  const size_t n = (size_t)W * H;
  auto up = [](size_t x) { return (x + 15) / 16 * 16; };
  l.scan_blocks = (int)((n + kScanBlock - 1) / kScanBlock);
  l.sv_a = kHeaderBytes;
  l.sv_b = l.sv_a + (size_t)VA * sizeof(SnapVert);
  l.big_a = l.sv_b + (size_t)VB * sizeof(SnapVert);
  l.big_b = l.big_a + (size_t)FA * sizeof(int4);
  l.cnt = l.big_b + (size_t)FB * sizeof(int4);
  l.block_sums = up(l.cnt + n * sizeof(unsigned));
  l.entries = up(l.block_sums + (size_t)l.scan_blocks * sizeof(unsigned long long));
  l.total = l.entries + (size_t)capacity * sizeof(long long);
  return l;
}

inline bool columns_sizes_ok(int VA, int FA, int VB, int FB, int W, int H, long long capacity) {
  return VA >= 1 && VA <= kRasterMaxPrims && FA >= 1 && FA <= kRasterMaxPrims && VB >= 1 && VB <= kRasterMaxPrims && FB >= 1 &&
         FB <= kRasterMaxPrims && W >= 1 && W <= kRasterMaxDim && H >= 1 && H <= kRasterMaxDim && capacity >= 1 && capacity <= kMaxCapacity;
}

// mesh_volume.hip: reset, setup x2, zero, count x2, scan, fill x2 on `st`.  Afterwards (unless the header's status word is set) the
// array at l.cnt holds each column's END in the array at l.entries, and the crossings of a column lie between the previous
// column's end and its own, in no particular order.  Arguments are the caller's to validate (columns_sizes_ok, s, the origin).
int columns_crossings_launch(const double* const verts[2], const int V[2], const int* const faces[2], const int F[2], double x0, double y0,
                             double s, int W, int H, long long capacity, char* ws, const ColumnsLayout& l, hipStream_t st);

}  // namespace coma
