// ofdis_lr.h -- device helpers of the stereo left-right step (ofdis_stereo_lr.hip, compiled under the exact contract only, so
// every kernel that uses them computes the same bits): the left-right consistency test of include/ofdis.h (ofdis_lr_check) and
// the row scan of ofdis_disparity_fill.  Each is written once here for the standalone kernels and for the fused finish
// (upsample_lr_kernel); the one-channel level disparity to full resolution is upsample_at<float> of ofdis_upsample.h.
#pragma once
#include "ofdis_upsample.h"

namespace ofdis {

// The left-right test for the pixel at column x with displacement d towards the other view; `R(xx)` returns the other view's
// displacement at an integer column of the same row.  fb_code (ofdis_upsample.h) with v = 0 and the vertical blend dropped.
template <class Other>
__device__ __forceinline__ uint8_t lr_code(float d, int x, int W, float alpha, float beta, Other R) {
  const float xb = (float)x + d;
  if (!(xb >= 0.0f && xb <= (float)(W - 1))) return FB_OUTSIDE;  // (NaN lands here)
  int x0 = 0;
  float ax = 0.0f;
  if (W > 1) { x0 = min((int)floorf(xb), W - 2); ax = xb - (float)x0; }
  const int x1 = min(x0 + 1, W - 1);
  const float bx = 1.0f - ax;
  const float r = R(x0) * bx + R(x1) * ax;
  const float s = d + r;
  const float lhs = s * s;
  const float rhs = alpha * (d * d + r * r) + beta;
  return lhs <= rhs ? FB_CONSISTENT : FB_INCONSISTENT;
}

// ------------------------------------------------------------------------------------ nearest consistent neighbour of a row
// A wavefront walks a row in chunks of 64 columns, lane i at column base + i.  `m` is the chunk's ballot of "consistent".  Inside
// the chunk the inclusive max-scan of (consistent ? x : -1) from the left -- and the min-scan of (consistent ? x : W) from the
// right -- is a bit search in m; across chunks it is one wavefront-uniform carry: the nearest consistent column of the chunks
// already walked (-1: none).
__device__ __forceinline__ int scan_left(unsigned long long m, int lane, int base, int carry) {  // largest consistent x' < x
  const unsigned long long low = m & ((1ull << lane) - 1ull);
  return low ? base + 63 - __builtin_clzll(low) : carry;
}
__device__ __forceinline__ int scan_right(unsigned long long m, int lane, int base, int carry) {  // smallest consistent x' > x
  const unsigned long long high = (m >> lane) >> 1;
  return high ? base + lane + 1 + __builtin_ctzll(high) : carry;
}
__device__ __forceinline__ int carry_left(unsigned long long m, int base, int carry) {
  return m ? base + 63 - __builtin_clzll(m) : carry;
}
__device__ __forceinline__ int carry_right(unsigned long long m, int base, int carry) {
  return m ? base + __builtin_ctzll(m) : carry;
}
// OFDIS_FILL_BACKGROUND for a flagged pixel with value d: l / r = its nearest consistent columns (-1: none), D(x) the row
__device__ __forceinline__ float fill_pick(float dl, float dr) { return fabsf(dl) <= fabsf(dr) ? dl : dr; }
template <class Row>
__device__ __forceinline__ float fill_background(float d, int l, int r, Row D) {
  if (l >= 0 && r >= 0) return fill_pick(D(l), D(r));
  if (l >= 0) return D(l);
  if (r >= 0) return D(r);
  return d;
}

}  // namespace ofdis
