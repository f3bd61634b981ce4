// ofdis_stabilize.hip -- video stabilisation (include/ofdis.h: ofdis_camera_path, ofdis_warp_frames and, through both,
// ofdis_batch_stabilize): the per-pair camera models of ofdis_global_motion turned into one correcting warp per frame by a
// windowed average of the motions relative to that frame, and the frames resampled by their warps.
//
// Compiled under the exact contract only (-ffp-contract=off).  The camera path is a fixed sequence of separately rounded fp64
// operations (the divisions are the compiler's correctly rounded expansion), the frame warp a fixed sequence of fp32 ones;
// of_dis_amd/stabilize.py states both in numpy and the tests compare bit for bit.
//
// camera_path_kernel: one lane per frame.  The lane walks its window outwards -- pair f + j - 1 forward, pair f - j backward --
// and stops at the clip's end, at `radius` or at the first unusable pair on either side, which is the header's reach r_f.  The
// two running maps and the accumulator are named scalars (StabMap): nothing is indexed dynamically, nothing goes to scratch.
// At most 2 * radius models of 48 bytes per lane: the cost is negligible next to one frame of the warp.
//
// camera_path_projective_kernel (ofdis_camera_path_projective): the same walk on homographies (StabMap8, eight named scalars
// with an implicit 1 in the corner).  A composition is the 3 x 3 product divided by its corner entry, the inverse the adjugate
// divided by the determinant of the linear part: 24 fp64 divisions per step of the walk, still nothing next to a frame.
//
// warp_frames_kernel<NOC, NP>: the quad mapping of ofdis_quad.h, one body for the affine warp (NP = 6) and the projective one
// (NP = 8, ofdis_warp_frames_projective).  The frame's NP coefficients are uniform per workgroup (scalar loads).  Four taps per
// pixel through interp_sample; an affine warp keeps the lanes of a wavefront on neighbouring source bytes, a usable projective
// one (denominator >= 0.5) nearly so.  NP = 8 adds the perspective terms and ONE correctly rounded fp32 division per pixel to
// the same expressions; NP = 6 compiles to what it was before the projective warp existed.  4 * NOC output bytes and 4
// `inside` bytes per lane (quad_store).  No LDS.
#include "ofdis_upsample.h"

namespace ofdis {

// ------------------------------------------------------------------------------------ camera path
// x' = a*x + b*y + tx, y' = c*x + d*y + ty in centred coordinates
struct StabMap {
  double a, b, c, d, tx, ty;
};
// OFDIS_STAB_MIN_DET <= det <= OFDIS_STAB_MAX_DET (NaN: false)
__device__ __forceinline__ bool stab_det_ok(double det) { return det >= 0.25 && det <= 4.0; }
__device__ __forceinline__ bool stab_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (NaN: false)
__device__ __forceinline__ bool stab_finite(const StabMap& m) {
  return stab_finite(m.a) && stab_finite(m.b) && stab_finite(m.c) && stab_finite(m.d) && stab_finite(m.tx) && stab_finite(m.ty);
}
__device__ __forceinline__ double stab_det(const StabMap& m) { return m.a * m.d - m.b * m.c; }
// T_k of the model of pair k; false: the pair is unusable
__device__ __forceinline__ bool stab_pair_map(const double* __restrict__ models, int k, StabMap& t) {
  const double* m = models + (size_t)k * 6;
  const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5];
  if (!(stab_finite(a0) && stab_finite(a1) && stab_finite(a2) && stab_finite(a3) && stab_finite(a4) && stab_finite(a5))) return false;
  t = StabMap{1.0 + a1, a2, a4, 1.0 + a5, a0, a3};
  return stab_det_ok(stab_det(t));
}
// t o m: m first, then t
__device__ __forceinline__ StabMap stab_compose(const StabMap& t, const StabMap& m) {
  StabMap r;
  r.a = t.a * m.a + t.b * m.c;
  r.b = t.a * m.b + t.b * m.d;
  r.c = t.c * m.a + t.d * m.c;
  r.d = t.c * m.b + t.d * m.d;
  r.tx = (t.a * m.tx + t.b * m.ty) + t.tx;
  r.ty = (t.c * m.tx + t.d * m.ty) + t.ty;
  return r;
}
__device__ __forceinline__ StabMap stab_invert(const StabMap& t, double det) {
  StabMap r;
  r.a = t.d / det;
  r.b = (0.0 - t.b) / det;
  r.c = (0.0 - t.c) / det;
  r.d = t.a / det;
  r.tx = 0.0 - (r.a * t.tx + r.b * t.ty);
  r.ty = 0.0 - (r.c * t.tx + r.d * t.ty);
  return r;
}

__global__ __launch_bounds__(256) void camera_path_kernel(const double* __restrict__ models, int npairs, StabWindow win,
                                                          double* __restrict__ warps) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f > npairs) return;
  const double w0 = win.w[0];
  StabMap acc{w0, 0.0, 0.0, w0, 0.0, 0.0};
  double sw = w0;
  StabMap mf{1.0, 0.0, 0.0, 1.0, 0.0, 0.0}, mb = mf;
  for (int j = 1; j <= win.radius; ++j) {
    if (f + j - 1 >= npairs || f - j < 0) break;
    StabMap tf, tb;
    const bool okf = stab_pair_map(models, f + j - 1, tf);
    const bool okb = stab_pair_map(models, f - j, tb);
    if (!(okf && okb)) break;
    mf = stab_compose(tf, mf);
    mb = stab_compose(stab_invert(tb, stab_det(tb)), mb);
    const double wj = win.w[j];
    acc.a = acc.a + (wj * mf.a + wj * mb.a);
    acc.b = acc.b + (wj * mf.b + wj * mb.b);
    acc.c = acc.c + (wj * mf.c + wj * mb.c);
    acc.d = acc.d + (wj * mf.d + wj * mb.d);
    acc.tx = acc.tx + (wj * mf.tx + wj * mb.tx);
    acc.ty = acc.ty + (wj * mf.ty + wj * mb.ty);
    sw = sw + (wj + wj);
  }
  const StabMap q{acc.a / sw, acc.b / sw, acc.c / sw, acc.d / sw, acc.tx / sw, acc.ty / sw};
  const double det = stab_det(q);
  StabMap w{1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  if (stab_det_ok(det)) {
    const StabMap inv = stab_invert(q, det);
    if (stab_finite(inv)) w = inv;
  }
  const double s = 1.0 / win.zoom;
  double* o = warps + (size_t)f * 6;
  o[0] = w.tx;
  o[1] = w.a * s - 1.0;
  o[2] = w.b * s;
  o[3] = w.ty;
  o[4] = w.c * s;
  o[5] = w.d * s - 1.0;
}

hipError_t launch_camera_path(const double* models, int npairs, const StabWindow& win, double* warps, hipStream_t s) {
  hipLaunchKernelGGL(camera_path_kernel, dim3((unsigned)(npairs + 1 + 255) / 256), dim3(256), 0, s, models, npairs, win, warps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ projective camera path
// x' = (a*x + b*y + tx) / (1 + gx*x + gy*y), y' = (c*x + d*y + ty) / (1 + gx*x + gy*y) in centred coordinates
struct StabMap8 {
  double a, b, c, d, tx, ty, gx, gy;
};
__device__ __forceinline__ StabMap8 stab_identity8() { return StabMap8{1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0}; }
// finite, ok(det of the linear part), and the denominator at least 0.5 (the header's STAB_MIN_DENOM) over the frame of half
// sides hx, hy (NaN: false)
__device__ __forceinline__ bool stab_usable(const StabMap8& m, double hx, double hy) {
  if (!(stab_finite(m.a) && stab_finite(m.b) && stab_finite(m.c) && stab_finite(m.d) && stab_finite(m.tx) && stab_finite(m.ty) &&
        stab_finite(m.gx) && stab_finite(m.gy)))
    return false;
  return stab_det_ok(m.a * m.d - m.b * m.c) && (1.0 - fabs(m.gx) * hx) - fabs(m.gy) * hy >= 0.5;
}
// T_k of the 8-parameter model of pair k; false: the pair is unusable
__device__ __forceinline__ bool stab_pair_map8(const double* __restrict__ models, int k, double hx, double hy, StabMap8& t) {
  const double* m = models + (size_t)k * 8;
  const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5], a6 = m[6], a7 = m[7];
  if (!(stab_finite(a0) && stab_finite(a1) && stab_finite(a2) && stab_finite(a3) && stab_finite(a4) && stab_finite(a5) &&
        stab_finite(a6) && stab_finite(a7)))
    return false;
  t = StabMap8{1.0 + a1, a2, a4, 1.0 + a5, a0, a3, 0.0 - a6, 0.0 - a7};
  return stab_usable(t, hx, hy);
}
// t o m: m first, then t
__device__ __forceinline__ StabMap8 stab_compose(const StabMap8& t, const StabMap8& m) {
  const double a = (t.a * m.a + t.b * m.c) + t.tx * m.gx;
  const double b = (t.a * m.b + t.b * m.d) + t.tx * m.gy;
  const double c = (t.c * m.a + t.d * m.c) + t.ty * m.gx;
  const double d = (t.c * m.b + t.d * m.d) + t.ty * m.gy;
  const double tx = (t.a * m.tx + t.b * m.ty) + t.tx;
  const double ty = (t.c * m.tx + t.d * m.ty) + t.ty;
  const double gx = (t.gx * m.a + t.gy * m.c) + m.gx;
  const double gy = (t.gx * m.b + t.gy * m.d) + m.gy;
  const double n = (t.gx * m.tx + t.gy * m.ty) + 1.0;
  return StabMap8{a / n, b / n, c / n, d / n, tx / n, ty / n, gx / n, gy / n};
}
__device__ __forceinline__ StabMap8 stab_invert(const StabMap8& t) {
  const double D = t.a * t.d - t.b * t.c;
  StabMap8 r;
  r.a = (t.d - t.ty * t.gy) / D;
  r.b = (t.tx * t.gy - t.b) / D;
  r.c = (t.ty * t.gx - t.c) / D;
  r.d = (t.a - t.tx * t.gx) / D;
  r.tx = (t.b * t.ty - t.tx * t.d) / D;
  r.ty = (t.tx * t.c - t.a * t.ty) / D;
  r.gx = (t.c * t.gy - t.d * t.gx) / D;
  r.gy = (t.b * t.gx - t.a * t.gy) / D;
  return r;
}

__global__ __launch_bounds__(256) void camera_path_projective_kernel(const double* __restrict__ models, int npairs, double hx,
                                                                     double hy, StabWindow win, double* __restrict__ warps) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f > npairs) return;
  const double w0 = win.w[0];
  StabMap8 acc{w0, 0.0, 0.0, w0, 0.0, 0.0, 0.0, 0.0};
  double sw = w0;
  StabMap8 mf = stab_identity8(), mb = mf;
  for (int j = 1; j <= win.radius; ++j) {
    if (f + j - 1 >= npairs || f - j < 0) break;
    StabMap8 tf, tb;
    const bool okf = stab_pair_map8(models, f + j - 1, hx, hy, tf);
    const bool okb = stab_pair_map8(models, f - j, hx, hy, tb);
    if (!(okf && okb)) break;
    mf = stab_compose(tf, mf);
    mb = stab_compose(stab_invert(tb), mb);
    const double wj = win.w[j];
    acc.a = acc.a + (wj * mf.a + wj * mb.a);
    acc.b = acc.b + (wj * mf.b + wj * mb.b);
    acc.c = acc.c + (wj * mf.c + wj * mb.c);
    acc.d = acc.d + (wj * mf.d + wj * mb.d);
    acc.tx = acc.tx + (wj * mf.tx + wj * mb.tx);
    acc.ty = acc.ty + (wj * mf.ty + wj * mb.ty);
    acc.gx = acc.gx + (wj * mf.gx + wj * mb.gx);
    acc.gy = acc.gy + (wj * mf.gy + wj * mb.gy);
    sw = sw + (wj + wj);
  }
  const StabMap8 q{acc.a / sw, acc.b / sw, acc.c / sw, acc.d / sw, acc.tx / sw, acc.ty / sw, acc.gx / sw, acc.gy / sw};
  StabMap8 w = stab_identity8();
  if (stab_usable(q, hx, hy)) {
    const StabMap8 inv = stab_invert(q);
    if (stab_usable(inv, hx, hy)) w = inv;
  }
  const double s = 1.0 / win.zoom;
  double* o = warps + (size_t)f * 8;
  o[0] = w.tx;
  o[1] = w.a * s - 1.0;
  o[2] = w.b * s;
  o[3] = w.ty;
  o[4] = w.c * s;
  o[5] = w.d * s - 1.0;
  o[6] = 0.0 - w.gx * s;
  o[7] = 0.0 - w.gy * s;
}

hipError_t launch_camera_path_projective(const double* models, int npairs, int w, int h, const StabWindow& win, double* warps,
                                         hipStream_t s) {
  hipLaunchKernelGGL(camera_path_projective_kernel, dim3((unsigned)(npairs + 1 + 255) / 256), dim3(256), 0, s, models, npairs,
                     (double)(w - 1) * 0.5, (double)(h - 1) * 0.5, win, warps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ frame warp
// what the kernel is launched with: the frames of this launch
struct StabWarpArgs {
  const uint8_t* frames;  // [nframes][H][W][NOC]
  const double* warps;    // [nframes][NP]
  uint8_t* out;           // [nframes][H][W][NOC]
  uint8_t* inside;        // [nframes][H][W] or null
  QuadLaunch q;
  bool replicate;         // OFDIS_BORDER_REPLICATE
  bool vec_out, vec_ins;  // quad_vec of out and inside
};

template <int NOC, int NP>
__global__ __launch_bounds__(256) void warp_frames_kernel(int W, int H, StabWarpArgs a) {
  static_assert(NP == 6 || NP == 8, "an affine warp b0 .. b5 or a projective one g0 .. g7");
  QuadLane l;
  if (!quad_lane(a.q, W, H, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const int np = min(4, W - x);
  const size_t plane = (size_t)W * H;
  const uint8_t* I = a.frames + f * plane * NOC;
  const double* wp = a.warps + (size_t)f * NP;  // (uniform over the workgroup)
  const float b0 = (float)wp[0], b1 = (float)wp[1], b2 = (float)wp[2], b3 = (float)wp[3], b4 = (float)wp[4], b5 = (float)wp[5];
  float g6 = 0.0f, g7 = 0.0f;
  if constexpr (NP == 8) g6 = (float)wp[6], g7 = (float)wp[7];
  const float yc = (float)(2 * y - (H - 1)) * 0.5f;
  uint8_t q[4 * NOC], ins[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float c[3] = {0.0f, 0.0f, 0.0f};
    ins[i] = 0;
    if (i < np) {
      const int xx = x + i;
      const float xc = (float)(2 * xx - (W - 1)) * 0.5f;
      float mu = (b0 + b1 * xc) + b2 * yc;
      float mv = (b3 + b4 * xc) + b5 * yc;
      bool front = true;
      if constexpr (NP == 8) {  // the displacement of the homography: the quadratic model over the denominator
        const float e = g6 * xc + g7 * yc;
        const float D = 1.0f - e;
        const float r = 1.0f / D;  // (the compiler's correctly rounded expansion)
        mu = (mu + e * xc) * r;
        mv = (mv + e * yc) * r;
        front = D > 0.0f;  // (NaN: false)
      }
      const float px = (float)xx + mu, py = (float)y + mv;
      const bool in = front && fb_inside(px, py, W, H);
      ins[i] = in ? 1 : 0;
      if (in || a.replicate)  // (fmaxf / fminf return the other operand for a NaN: a NaN position samples pixel 0)
        interp_sample(I, W, H, NOC, fminf(fmaxf(px, 0.0f), (float)(W - 1)), fminf(fmaxf(py, 0.0f), (float)(H - 1)), c);
    }
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) q[i * NOC + ch] = quad_u8(c[ch]);
  }
  const size_t px0 = f * plane + (size_t)y * W + x;  // the quad's first pixel in a [frames][H][W] array
  quad_store<NOC>(a.out + px0 * NOC, q, np, a.vec_out);
  if (a.inside) quad_store<1>(a.inside + px0, ins, np, a.vec_ins);
}

template <int NP>
static hipError_t launch_warp(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w, int h,
                              int noc, bool replicate, hipStream_t s) {
  StabWarpArgs a{frames, warps, out, inside, QuadLaunch{}, replicate, quad_vec(w, out), quad_vec(w, inside)};
  return quad_chunks(nframes, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL((warp_frames_kernel<3, NP>), blocks, dim3(256), 0, s, w, h, a);
    else
      hipLaunchKernelGGL((warp_frames_kernel<1, NP>), blocks, dim3(256), 0, s, w, h, a);
    return hipGetLastError();
  });
}
hipError_t launch_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w,
                              int h, int noc, bool replicate, hipStream_t s) {
  return launch_warp<6>(frames, warps, out, inside, nframes, w, h, noc, replicate, s);
}
hipError_t launch_warp_frames_projective(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes,
                                         int w, int h, int noc, bool replicate, hipStream_t s) {
  return launch_warp<8>(frames, warps, out, inside, nframes, w, h, noc, replicate, s);
}

}  // namespace ofdis
