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
// warp_frames_kernel<NOC>: the quad mapping of ofdis_quad.h.  The frame's six coefficients are uniform per workgroup (scalar
// loads).  Four taps per pixel through interp_sample; an affine warp keeps the lanes of a wavefront on neighbouring source
// bytes.  4 * NOC output bytes and 4 `inside` bytes per lane (quad_store).  No LDS.
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

// ------------------------------------------------------------------------------------ frame warp
// what the kernel is launched with: the frames of this launch
struct StabWarpArgs {
  const uint8_t* frames;  // [nframes][H][W][NOC]
  const double* warps;    // [nframes][6]
  uint8_t* out;           // [nframes][H][W][NOC]
  uint8_t* inside;        // [nframes][H][W] or null
  QuadLaunch q;
  bool replicate;         // OFDIS_BORDER_REPLICATE
  bool vec_out, vec_ins;  // quad_vec of out and inside
};

template <int NOC>
__global__ __launch_bounds__(256) void warp_frames_kernel(int W, int H, StabWarpArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, W, H, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const int np = min(4, W - x);
  const size_t plane = (size_t)W * H;
  const uint8_t* I = a.frames + f * plane * NOC;
  const double* wp = a.warps + (size_t)f * 6;  // (uniform over the workgroup)
  const float b0 = (float)wp[0], b1 = (float)wp[1], b2 = (float)wp[2], b3 = (float)wp[3], b4 = (float)wp[4], b5 = (float)wp[5];
  const float yc = (float)(2 * y - (H - 1)) * 0.5f;
  uint8_t q[4 * NOC], ins[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float c[3] = {0.0f, 0.0f, 0.0f};
    ins[i] = 0;
    if (i < np) {
      const int xx = x + i;
      const float xc = (float)(2 * xx - (W - 1)) * 0.5f;
      const float mu = (b0 + b1 * xc) + b2 * yc;
      const float mv = (b3 + b4 * xc) + b5 * yc;
      const float px = (float)xx + mu, py = (float)y + mv;
      const bool in = fb_inside(px, py, W, H);
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

hipError_t launch_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w,
                              int h, int noc, bool replicate, hipStream_t s) {
  StabWarpArgs a{frames, warps, out, inside, QuadLaunch{}, replicate, quad_vec(w, out), quad_vec(w, inside)};
  return quad_chunks(nframes, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL(warp_frames_kernel<3>, blocks, dim3(256), 0, s, w, h, a);
    else
      hipLaunchKernelGGL(warp_frames_kernel<1>, blocks, dim3(256), 0, s, w, h, a);
    return hipGetLastError();
  });
}

}  // namespace ofdis
