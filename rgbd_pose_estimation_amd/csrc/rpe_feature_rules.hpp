// The RULES of the feature stage (include/rgbd_pose_hip.h Part 3, "Features and relocalisation", "Scale levels") beside their tables,
// stated once for the one-level route (rpe_feature.hip, rpe_feature_oriented.hip) and the levels' route (rpe_feature_scale.hip);
// integers and comparisons throughout.  Kept as a kernel's OWN TEXT, because calling a shared function changed the kernel's
// instructions (profiles/rules_ab.json): the 5 x 5 box sum in D1 and D1s; the tests in D6 and D6s; the word store in D6, D6o and
// (store_words) rpe_feature_scale.hip; moments, angle bin and steered tests in D6o and D6os.  A change to one goes to each text.
#pragma once
#include "rpe_brief_table.h"
#include "rpe_feature_disc.h"

namespace rpe {
namespace {

// D1 / D1s: a workgroup owns a 32 x 8 tile and keeps its pixels with a halo of 3 in LDS, a pixel as Y | K << 8 (K: known)
constexpr int kTileX = 32, kTileY = 8, kHalo = 3, kBorder = 16;
constexpr int kLdsX = kTileX + 2 * kHalo, kLdsY = kTileY + 2 * kHalo;
using FeatTile = unsigned short[kLdsY][kLdsX + 2];
// the luma of an RGBA8 pixel (the caller decides what A = 0 means)
__device__ __forceinline__ unsigned luma(unsigned px) { return (77u * (px & 0xffu) + 150u * ((px >> 8) & 0xffu) + 29u * ((px >> 16) & 0xffu) + 128u) >> 8; }

// The segment-test score of pixel (u, v) of a w x h image, at (cx, cy) in the tile: 0 unless the pixel lies kBorder inside the image,
// it and the 16 ring pixels are known, nine contiguous ring pixels are all brighter than Y + thr or all darker than Y - thr, and
// finite() holds (asked last: the view's geometry there; it captures BY VALUE, by reference the whole unit compiles differently).
template <class Finite>
__device__ __forceinline__ int segment_score(const FeatTile& t, int cx, int cy, int u, int v, int w, int h, int thr, Finite finite) {
  int sc = 0;
  const int c = t[cy][cx];
  if (u >= kBorder && u < w - kBorder && v >= kBorder && v < h - kBorder && (c & 0x100)) {
    constexpr int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int RY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    const int Y = c & 0xff;
    unsigned hi = 0, lo = 0, known = 0x100;
    int sum = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int r = t[cy + RY[k]][cx + RX[k]], yr = r & 0xff;
      known &= (unsigned)r;
      hi |= (unsigned)(yr > Y + thr) << k;
      lo |= (unsigned)(yr < Y - thr) << k;
      const int d = yr > Y ? yr - Y : Y - yr;
      sum += d > thr ? d - thr : 0;
    }
    // nine contiguous ring pixels: bit i of run9(m) is set iff bits i .. i + 8 of the doubled 16-bit mask are
    auto run9 = [](unsigned m16) { unsigned m = m16 | m16 << 16; unsigned r = m & (m >> 1); r &= r >> 2; r &= r >> 4; return r & (m >> 8) & 0xffffu; };
    if (known && (run9(hi) | run9(lo))) sc = finite() ? sum : 0;
  }
  return sc;
}

// D2 / D4: 3 x 3 non-maximum suppression at index i, row width w (a positive score lies kBorder inside its image: 8 neighbours exist)
__device__ __forceinline__ bool survives(const int* __restrict__ score, int i, int w) {
  const int s = score[i];
  if (s <= 0) return false;
  bool ok = true;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      if (dx == 0 && dy == 0) continue;
      const int nb = score[i + dy * w + dx];
      ok = ok && ((dy < 0 || (dy == 0 && dx < 0)) ? s > nb : s >= nb);   // a tie goes to the lower pixel index
    }
  return ok;
}

}  // namespace
}  // namespace rpe
