// ofdis_upsample.h -- device helpers shared by the exact-only units ofdis_pyr.hip and ofdis_interp.hip: the arithmetic of
// the level flow to full resolution (upsample_crop_kernel, run_dense.cpp:406-414), the forward-backward consistency test and
// the compact output encodings (include/ofdis.h: ofdis_encoding).
// Both units are compiled with -ffp-contract=off only, so every kernel that uses these computes the same bits.
#pragma once
#include "ofdis_kernels.h"

namespace ofdis {

// cv::resize INTER_LINEAR, horizontal step: the two source rows sy, sy1 of the level flow `fl` (sw columns) interpolated at
// padded full-resolution column X, times 2^sc_l when `scale`.
__device__ __forceinline__ void upsample_h(const float2* __restrict__ fl, int sw, int sy, int sy1, int X, float inv,
                                           float scf, bool scale, float2& r0, float2& r1) {
  float fx = ((float)X + 0.5f) * inv - 0.5f;
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.0f; }
  if (sx >= sw - 1) { sx = sw - 1; fx = 0.0f; }
  const int sx1 = min(sx + 1, sw - 1);
  float2 v00 = fl[sy * sw + sx], v01 = fl[sy * sw + sx1], v10 = fl[sy1 * sw + sx], v11 = fl[sy1 * sw + sx1];
  if (scale) {
    v00.x *= scf; v00.y *= scf; v01.x *= scf; v01.y *= scf;
    v10.x *= scf; v10.y *= scf; v11.x *= scf; v11.y *= scf;
  }
  const float ax = 1.0f - fx;
  r0 = make_float2(v00.x * ax + v01.x * fx, v00.y * ax + v01.y * fx);
  r1 = make_float2(v10.x * ax + v11.x * fx, v10.y * ax + v11.y * fx);
}

// The same step for the one-channel result of the stereo-depth mode: the expressions of upsample_crop1_kernel.
__device__ __forceinline__ void upsample_h1(const float* __restrict__ fl, int sw, int sy, int sy1, int X, float inv, float scf,
                                            bool scale, float& r0, float& r1) {
  float fx = ((float)X + 0.5f) * inv - 0.5f;
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.0f; }
  if (sx >= sw - 1) { sx = sw - 1; fx = 0.0f; }
  const int sx1 = min(sx + 1, sw - 1);
  float v00 = fl[sy * sw + sx], v01 = fl[sy * sw + sx1], v10 = fl[sy1 * sw + sx], v11 = fl[sy1 * sw + sx1];
  if (scale) { v00 *= scf; v01 *= scf; v10 *= scf; v11 *= scf; }
  const float ax = 1.0f - fx;
  r0 = v00 * ax + v01 * fx;
  r1 = v10 * ax + v11 * fx;
}

// ------------------------------------------------------------------------------------ forward-backward consistency
// The test of include/ofdis.h (ofdis_fb_check), written once for every kernel that evaluates it.  The units that include this
// header are compiled under the exact contract only (-ffp-contract=off): every operation is separately rounded, so the mask is
// a fixed function of the two flows.
// `R(xx, yy)` returns the other direction's flow at an integer pixel of the full-resolution image.
enum : uint8_t { FB_CONSISTENT = 0, FB_INCONSISTENT = 1, FB_OUTSIDE = 2 };
template <class Other>
__device__ __forceinline__ uint8_t fb_code(float u, float v, int x, int y, int W, int H, float alpha, float beta, Other R) {
  const float xb = (float)x + u, yb = (float)y + v;
  if (!(xb >= 0.0f && xb <= (float)(W - 1) && yb >= 0.0f && yb <= (float)(H - 1))) return FB_OUTSIDE;  // (NaN lands here)
  int x0 = 0, y0 = 0;
  float ax = 0.0f, ay = 0.0f;
  if (W > 1) { x0 = min((int)floorf(xb), W - 2); ax = xb - (float)x0; }
  if (H > 1) { y0 = min((int)floorf(yb), H - 2); ay = yb - (float)y0; }
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  float2 r00, r01, r10, r11;
  R(x0, x1, y0, y1, r00, r01, r10, r11);
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float ru = (r00.x * bx + r01.x * ax) * by + (r10.x * bx + r11.x * ax) * ay;
  const float rv = (r00.y * bx + r01.y * ax) * by + (r10.y * bx + r11.y * ax) * ay;
  const float du = u + ru, dv = v + rv;
  const float lhs = du * du + dv * dv;
  const float rhs = alpha * ((u * u + v * v) + (ru * ru + rv * rv)) + beta;
  return lhs <= rhs ? FB_CONSISTENT : FB_INCONSISTENT;
}

// Vertical source rows and weight of padded full-resolution row Y: the vertical step of upsample_crop_kernel for one row.
// (There the rows of a group share sy; floor((Y + 0.5) / s - 0.5) is exact, so per row it is the same value.)
struct UpRow {
  int sy, sy1;
  float fy;
};
__device__ __forceinline__ UpRow up_row(int Y, int sh, float inv) {
  UpRow r;
  const float fy = ((float)Y + 0.5f) * inv - 0.5f;
  r.sy = (int)floorf(fy);
  const bool clamp = r.sy < 0 || r.sy >= sh - 1;
  r.fy = clamp ? 0.0f : fy - floorf(fy);
  r.sy = r.sy < 0 ? 0 : (r.sy >= sh - 1 ? sh - 1 : r.sy);
  r.sy1 = min(r.sy + 1, sh - 1);
  return r;
}
__device__ __forceinline__ float2 up_mix(float2 a0, float2 a1, float fy) {
  const float ay = 1.0f - fy;
  return make_float2(a0.x * ay + a1.x * fy, a0.y * ay + a1.y * fy);
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
