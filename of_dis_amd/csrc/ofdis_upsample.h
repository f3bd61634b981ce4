// ofdis_upsample.h -- device helpers of the full-resolution finish, shared by the exact-only units ofdis_upsample.hip,
// ofdis_interp.hip, ofdis_stereo_lr.hip, ofdis_track.hip, ofdis_dense_tracks.hip, ofdis_tfilter.hip and ofdis_trajfilter.hip: the arithmetic of the level flow to full resolution (run_dense.cpp:406-414, UpGeom
// in ofdis_kernels.h), the forward-backward consistency test and the compact output encodings (include/ofdis.h:
// ofdis_encoding).  These units are compiled with -ffp-contract=off only and every finish kernel takes its values from the
// helpers below -- upsample_h, up_row / up_group, up_mix -- so every one of them computes the same bits.  How the quad kernels
// among them map lanes to pixels, walk the frames and store their bytes is ofdis_quad.h, included here.
#pragma once
#include <algorithm>

#include "ofdis_kernels.h"
#include "ofdis_quad.h"

namespace ofdis {

// ------------------------------------------------------------------------------------ level flow to full resolution
// flowout *= 2^lv_l; cv::resize(flowout, x 2^lv_l, INTER_LINEAR); crop the padding.  cv::resize bilinear for CV_32FC1 / C2:
// half-pixel centres, source index clamped with the fraction forced to 0 at the borders, horizontal interpolation first.
// 2^lv_l is a power of two, so (X + 0.5) / s - 0.5 is exact in fp32.  T is float2 (flow) or float (stereo disparity).
__device__ __forceinline__ float up_scaled(float v, float s) { return v * s; }
__device__ __forceinline__ float2 up_scaled(float2 v, float s) { return make_float2(v.x * s, v.y * s); }
// a * (1 - f) + b * f, each product and the sum separately rounded
__device__ __forceinline__ float up_mix(float a, float b, float f) { return a * (1.0f - f) + b * f; }
__device__ __forceinline__ float2 up_mix(float2 a, float2 b, float f) {
  const float e = 1.0f - f;
  return make_float2(a.x * e + b.x * f, a.y * e + b.y * f);
}

// Horizontal step: the two source rows sy, sy1 of the level flow `fl` interpolated at padded full-resolution column X, times
// 2^sc_l.
template <class T>
__device__ __forceinline__ void upsample_h(const T* __restrict__ fl, const UpGeom& g, int sy, int sy1, int X, T& r0, T& r1) {
  const int sw = g.sw;
  float fx = ((float)X + 0.5f) * g.inv() - 0.5f;
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.0f; }
  if (sx >= sw - 1) { sx = sw - 1; fx = 0.0f; }
  const int sx1 = min(sx + 1, sw - 1);
  T v00 = fl[sy * sw + sx], v01 = fl[sy * sw + sx1], v10 = fl[sy1 * sw + sx], v11 = fl[sy1 * sw + sx1];
  if (g.scale()) {
    const float scf = g.scf();
    v00 = up_scaled(v00, scf); v01 = up_scaled(v01, scf); v10 = up_scaled(v10, scf); v11 = up_scaled(v11, scf);
  }
  r0 = up_mix(v00, v01, fx);
  r1 = up_mix(v10, v11, fx);
}

// Vertical step for one padded full-resolution row Y: its two source rows and weight.
struct UpRow {
  int sy, sy1;
  float fy;
};
__device__ __forceinline__ UpRow up_row(int Y, const UpGeom& g) {
  UpRow r;
  const float fy = ((float)Y + 0.5f) * g.inv() - 0.5f;
  r.sy = (int)floorf(fy);
  const bool clamp = r.sy < 0 || r.sy >= g.sh - 1;
  r.fy = clamp ? 0.0f : fy - floorf(fy);
  r.sy = r.sy < 0 ? 0 : (r.sy >= g.sh - 1 ? g.sh - 1 : r.sy);
  r.sy1 = min(r.sy + 1, g.sh - 1);
  return r;
}
// One pixel of the full-resolution result: the level flow at padded column X of a row / at padded pixel (X, Y).
template <class T>
__device__ __forceinline__ T upsample_at(const T* __restrict__ fl, const UpGeom& g, int X, const UpRow& r) {
  T a0, a1;
  upsample_h(fl, g, r.sy, r.sy1, X, a0, a1);
  return up_mix(a0, a1, r.fy);
}
template <class T>
__device__ __forceinline__ T upsample_at(const T* __restrict__ fl, const UpGeom& g, int X, int Y) {
  return upsample_at(fl, g, X, up_row(Y, g));
}

// The same vertical step for a row group: the s = 2^sc_l padded rows with floor((Y + 0.5) / s - 0.5) = k are
// [k*s + s/2, k*s + s/2 + s) and share their source rows, so a kernel interpolates horizontally once per group.  Groups are
// numbered grp = 0 .. sh: k = -1 .. sh-1 (k = 0 .. sh for s = 1, the last one empty); k = -1 and k = sh-1 are the half groups
// at the borders, where the source row is clamped and the weight forced to 0.  [Y0, Y1) are the group's rows inside the crop
// (empty: nothing to do); floor((Y + 0.5) / s - 0.5) is exact, so fy(Y) is up_row's value.
struct UpGroup {
  int Y0, Y1, sy, sy1;
  bool clamp;
  float inv;
  __device__ __forceinline__ float fy(int Y) const {
    const float f = ((float)Y + 0.5f) * inv - 0.5f;
    return clamp ? 0.0f : f - floorf(f);
  }
};
__device__ __forceinline__ UpGroup up_group(int grp, const UpGeom& g) {
  UpGroup r;
  const int s = 1 << g.sc_l;
  const int k = grp - (s > 1 ? 1 : 0);
  r.Y0 = max(k * s + s / 2, g.top);
  r.Y1 = min(k * s + s / 2 + s, g.top + g.ho);
  r.inv = g.inv();
  const int sy = (int)floorf(((float)r.Y0 + 0.5f) * r.inv - 0.5f);
  r.clamp = sy < 0 || sy >= g.sh - 1;
  r.sy = sy < 0 ? 0 : (sy >= g.sh - 1 ? g.sh - 1 : sy);
  r.sy1 = min(r.sy + 1, g.sh - 1);
  return r;
}

// ------------------------------------------------------------------------------------ forward-backward consistency
// The test of include/ofdis.h (ofdis_fb_check), written once for every kernel that evaluates it.  The units that include this
// header are compiled under the exact contract only (-ffp-contract=off): every operation is separately rounded, so the mask is
// a fixed function of the two flows.
// The pieces are stated once -- fb_inside, fb_bilinear, fb_consistent -- and shared by the mask kernels (fb_code), frame
// interpolation (ofdis_interp.hip) and the point trajectories of ofdis_track.hip, which walk a REAL position through them.
enum : uint8_t { FB_CONSISTENT = 0, FB_INCONSISTENT = 1, FB_OUTSIDE = 2 };
// 0 <= px <= W-1 and 0 <= py <= H-1 (NaN: false)
__device__ __forceinline__ bool fb_inside(float px, float py, int W, int H) {
  return px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1);
}
// A full-resolution flow sampled bilinearly at the real position (px, py) inside the image.  `R(x0, x1, y0, y1, r00, r01, r10,
// r11)` returns that flow at the four integer pixels around it.
template <class Taps>
__device__ __forceinline__ float2 fb_bilinear(float px, float py, int W, int H, Taps R) {
  int x0 = 0, y0 = 0;
  float ax = 0.0f, ay = 0.0f;
  if (W > 1) { x0 = min((int)floorf(px), W - 2); ax = px - (float)x0; }
  if (H > 1) { y0 = min((int)floorf(py), H - 2); ay = py - (float)y0; }
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  float2 r00, r01, r10, r11;
  R(x0, x1, y0, y1, r00, r01, r10, r11);
  const float bx = 1.0f - ax, by = 1.0f - ay;
  return make_float2((r00.x * bx + r01.x * ax) * by + (r10.x * bx + r11.x * ax) * ay,
                     (r00.y * bx + r01.y * ax) * by + (r10.y * bx + r11.y * ax) * ay);
}
// the inequality on a flow (u, v) and the other direction's flow (ru, rv) at its target (a NaN on either side: false)
__device__ __forceinline__ bool fb_consistent(float u, float v, float ru, float rv, float alpha, float beta) {
  const float du = u + ru, dv = v + rv;
  const float lhs = du * du + dv * dv;
  const float rhs = alpha * ((u * u + v * v) + (ru * ru + rv * rv)) + beta;
  return lhs <= rhs;
}
// One step of a trajectory (include/ofdis.h: ofdis_track_points, steps 1 and 2) from the position p in frame k: q = p + the
// forward flow of pair k at p.  False where the track ends: q outside the image or, with FB, the inequality on the reverse flow
// at q.  `taps(k, d)` gives pair k's flow of direction d (0: frame k -> k + 1, 1: the reverse) at four integer pixels
// (fb_bilinear's R).  Stated once for the walks of ofdis_track.hip and ofdis_dense_tracks.hip.
template <bool FB, class Taps>
__device__ __forceinline__ bool fb_track_step(float2 p, int k, int W, int H, float alpha, float beta, Taps taps, float2& q) {
  const float2 uv = fb_bilinear(p.x, p.y, W, H, taps(k, 0));
  q = make_float2(p.x + uv.x, p.y + uv.y);
  bool live = fb_inside(q.x, q.y, W, H);
  if (FB && live) {
    const float2 r = fb_bilinear(q.x, q.y, W, H, taps(k, 1));
    live = fb_consistent(uv.x, uv.y, r.x, r.y, alpha, beta);
  }
  return live;
}
// The code of integer pixel (x, y) with flow (u, v); `R` gives the other direction's flow (fb_bilinear).
template <class Other>
__device__ __forceinline__ uint8_t fb_code(float u, float v, int x, int y, int W, int H, float alpha, float beta, Other R) {
  const float xb = (float)x + u, yb = (float)y + v;
  if (!fb_inside(xb, yb, W, H)) return FB_OUTSIDE;  // (NaN lands here)
  const float2 r = fb_bilinear(xb, yb, W, H, R);
  return fb_consistent(u, v, r.x, r.y, alpha, beta) ? FB_CONSISTENT : FB_INCONSISTENT;
}
// `R` for a materialised full-resolution flow F [H][W][2]
struct FlowTaps {
  const float2* F;
  int W;
  __device__ __forceinline__ void operator()(int x0, int x1, int y0, int y1, float2& r00, float2& r01, float2& r10,
                                             float2& r11) const {
    r00 = F[(size_t)y0 * W + x0]; r01 = F[(size_t)y0 * W + x1];
    r10 = F[(size_t)y1 * W + x0]; r11 = F[(size_t)y1 * W + x1];
  }
};

// `R` for a direction whose full-resolution flow is not materialised: the four neighbours recomputed from its level flow
// `fl`, the bits ofdis_batch_upsample_frames writes.  Neighbour rows y0 and y1 usually share their source rows (for s > 1): then
// the two horizontal interpolations are reused.
struct UpNeighbours {
  const float2* fl;
  const UpGeom& g;
  __device__ __forceinline__ void operator()(int x0, int x1, int y0, int y1, float2& r00, float2& r01, float2& r10,
                                             float2& r11) const {
    const UpRow q0 = up_row(y0 + g.top, g), q1 = up_row(y1 + g.top, g);
    float2 p0, p1, n0, n1;  // row pair of y0 at columns x0 and x1
    upsample_h(fl, g, q0.sy, q0.sy1, x0 + g.left, p0, p1);
    upsample_h(fl, g, q0.sy, q0.sy1, x1 + g.left, n0, n1);
    r00 = up_mix(p0, p1, q0.fy);
    r01 = up_mix(n0, n1, q0.fy);
    if (q1.sy != q0.sy) {  // (sy1 is a function of sy)
      upsample_h(fl, g, q1.sy, q1.sy1, x0 + g.left, p0, p1);
      upsample_h(fl, g, q1.sy, q1.sy1, x1 + g.left, n0, n1);
    }
    r10 = up_mix(p0, p1, q1.fy);
    r11 = up_mix(n0, n1, q1.fy);
  }
};

// ------------------------------------------------------------------------------------ 8-bit frames at a real position
// frame I (W x H x noc bytes) sampled bilinearly at p, clamped into the frame: c[0 .. noc-1]
__device__ __forceinline__ void interp_sample(const uint8_t* __restrict__ I, int W, int H, int noc, float pxc, float pyc,
                                              float (&c)[3]) {
  int x0 = 0, y0 = 0;
  float ax = 0.0f, ay = 0.0f;
  if (W > 1) { x0 = min((int)floorf(pxc), W - 2); ax = pxc - (float)x0; }
  if (H > 1) { y0 = min((int)floorf(pyc), H - 2); ay = pyc - (float)y0; }
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const uint8_t* r0 = I + (size_t)y0 * W * noc;
  const uint8_t* r1 = I + (size_t)y1 * W * noc;
#pragma unroll
  for (int ch = 0; ch < noc; ++ch) {
    const float i00 = (float)r0[x0 * noc + ch], i01 = (float)r0[x1 * noc + ch];
    const float i10 = (float)r1[x0 * noc + ch], i11 = (float)r1[x1 * noc + ch];
    c[ch] = (i00 * bx + i01 * ax) * by + (i10 * bx + i11 * ax) * ay;
  }
}

// ------------------------------------------------------------------------------------ compact output encodings
// The arithmetic of include/ofdis.h (ofdis_encoding), written once for ofdis_encode and the encoding upsample kernels.  TYPE is
// an OFDIS_ENC_* value.  enc_bits returns one encoded element in the low bits of a word.
enum { ENC_F32 = 0, ENC_F16 = 1, ENC_U16 = 2, ENC_U8 = 3 };
template <int TYPE>
struct EncTraits {
  static constexpr int bytes = TYPE == ENC_F32 ? 4 : (TYPE == ENC_U8 ? 1 : 2);
  static constexpr int per16 = 16 / bytes;  // elements of one 16-byte store
};
template <int TYPE>
__device__ __forceinline__ unsigned enc_bits(float v, float scale, float offset) {
  if constexpr (TYPE == ENC_F32) {
    return __float_as_uint(v);
  } else if constexpr (TYPE == ENC_F16) {
    // fptrunc: v_cvt_f16_f32 under the kernel's default mode, round to nearest even, binary16 subnormals kept
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
  } else {
    constexpr float M = TYPE == ENC_U16 ? 65535.0f : 255.0f;
    float t = v * scale + offset;  // two roundings (this header's units are compiled with -ffp-contract=off)
    t = fminf(fmaxf(t, 0.0f), M);  // (IEEE maxNum: a NaN becomes 0)
    return (unsigned)(int)floorf(t + 0.5f);
  }
}
// NV = per16 values in memory order into the four words of a 16-byte store
template <int TYPE>
__device__ __forceinline__ void enc_pack16(const float (&v)[EncTraits<TYPE>::per16], float scale, float offset, unsigned (&w)[4]) {
  constexpr int per_word = EncTraits<TYPE>::per16 / 4, bits = 8 * EncTraits<TYPE>::bytes;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < per_word; ++j) word |= enc_bits<TYPE>(v[i * per_word + j], scale, offset) << ((bits * j) & 31);
    w[i] = word;
  }
}

}  // namespace ofdis
