// The rasteriser's rule set as device functions (include/coma_hip.h states it): snapped vertices, exact int64 edge functions, the
// top-left rule, the f64 depth of a covered sample.  Shared by raster.hip (nearest-depth map) and mesh_volume.hip (every crossing of
// a pixel's column), so that the two cannot drift apart.
#pragma once
#include "common.h"

namespace coma {

constexpr int kSmallMax = 256;          // pixel centres in a bounding box that one lane still walks by itself
constexpr int kTile = 16;               // screen tile of the work-list kernel: 16 x 16 pixels = 256 threads
constexpr int kRasterMaxDim = 8192;     // W, H: box corners are packed into 16 bits each
constexpr int kRasterMaxPrims = 1 << 24;
constexpr double kSnapLimit = 33554432.0;   // 2^25 in 1/256-pixel units: every edge function stays below 2^53
constexpr size_t kHeaderBytes = 64;
enum { kBadNonFinite = 1, kBadRange = 2, kBadFace = 4 };

struct RasterCam {
  double r[9], t[3];   // camera-to-world rotation (row-major) and position
  double s, hw, hh;    // pixels per world unit, W/2, H/2
};

struct SnapVert {
  int x, y;            // 1/256-pixel units
  double z;            // camera-space depth, larger is farther
};

// edge function of P -> Q at (px, py): exact in int64 below the snap limit
__device__ __forceinline__ long long edge_fn(int Px, int Py, int Qx, int Qy, int px, int py) {
  return (long long)(Qx - Px) * (long long)(py - Py) - (long long)(Qy - Py) * (long long)(px - Px);
}

// a sample ON the edge P -> Q belongs to the triangle only when the edge is a left edge (runs upwards, y is down) or a top edge
__device__ __forceinline__ bool edge_owns_ties(int Px, int Py, int Qx, int Qy) {
  const int dx = Qx - Px, dy = Qy - Py;
  return dy < 0 || (dy == 0 && dx > 0);
}

struct RasterTri {
  int ax, ay, bx, by, cx, cy;
  double za, zb, zc, area;
  bool t0, t1, t2;
  bool flipped;         // area < 0 as given: B and C were swapped
  int x0, y0, x1, y1;   // inclusive pixel box, clipped to the screen; empty when x0 > x1 or y0 > y1
};

// false: nothing to draw (zero area, or no pixel centre of the screen inside the bounding box)
__device__ __forceinline__ bool raster_tri_load(const SnapVert* __restrict__ sv, const int* __restrict__ faces, int f, int W, int H,
                                                RasterTri& t) {
  const int ia = faces[3 * (int64_t)f + 0];
  int ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
  SnapVert A = sv[ia], B = sv[ib], C = sv[ic];
  long long area = edge_fn(A.x, A.y, B.x, B.y, C.x, C.y);
  if (area == 0) return false;
  t.flipped = area < 0;
  if (area < 0) {   // the other winding: swap two vertices
    const SnapVert T = B;
    B = C, C = T, area = -area;
  }
  t.ax = A.x, t.ay = A.y, t.bx = B.x, t.by = B.y, t.cx = C.x, t.cy = C.y;
  t.za = A.z, t.zb = B.z, t.zc = C.z, t.area = (double)area;
  t.t0 = edge_owns_ties(B.x, B.y, C.x, C.y), t.t1 = edge_owns_ties(C.x, C.y, A.x, A.y), t.t2 = edge_owns_ties(A.x, A.y, B.x, B.y);
  const int mnx = min(A.x, min(B.x, C.x)), mxx = max(A.x, max(B.x, C.x));
  const int mny = min(A.y, min(B.y, C.y)), mxy = max(A.y, max(B.y, C.y));
  // pixel i is sampled at 256 i + 128: first i with 256 i + 128 >= mn, last i with 256 i + 128 <= mx (>> is a floor)
  t.x0 = max(0, (mnx + 127) >> 8), t.x1 = min(W - 1, (mxx - 128) >> 8);
  t.y0 = max(0, (mny + 127) >> 8), t.y1 = min(H - 1, (mxy - 128) >> 8);
  return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// true when the centre of pixel (x, y) is covered; z is then the depth there
__device__ __forceinline__ bool raster_cover_depth(const RasterTri& t, int x, int y, double& z) {
  const int px = 256 * x + 128, py = 256 * y + 128;
  const long long e0 = edge_fn(t.bx, t.by, t.cx, t.cy, px, py);
  const long long e1 = edge_fn(t.cx, t.cy, t.ax, t.ay, px, py);
  const long long e2 = edge_fn(t.ax, t.ay, t.bx, t.by, px, py);
  const bool in = (e0 > 0 || (e0 == 0 && t.t0)) && (e1 > 0 || (e1 == 0 && t.t1)) && (e2 > 0 || (e2 == 0 && t.t2));
  if (!in) return false;
  z = (((double)e0 * t.za + (double)e1 * t.zb) + (double)e2 * t.zc) / t.area;
  return true;
}

// raster.hip: zeroes the header of a workspace (64 bytes) / snaps the vertices into sv and ORs the refusals (kBad*) into hdr[0]
int raster_reset_launch(int* hdr, hipStream_t st);
int raster_setup_launch(const double* verts, int V, const int* faces, int F, const RasterCam& cam, SnapVert* sv, int* hdr, hipStream_t st);

}  // namespace coma
