// ofdis_interp.hip -- frame interpolation from bidirectional flow with occlusion masks (include/ofdis.h: ofdis_interpolate,
// ofdis_batch_interpolate).  Backward warping of both frames to time t with the flows of Jiang et al., "Super SloMo"
// (CVPR 2018, eq. 4), blended by t where both warps are consistent and taken from the one consistent side elsewhere.
//
// Compiled under the exact contract only (-ffp-contract=off): every operation of the header's definition is a separately
// rounded fp32 operation, so the output is a fixed function of the inputs and the fused kernel below -- which recomputes
// the full-resolution flows and the masks from the level flows with the helpers of ofdis_batch_upsample_bidir
// (ofdis_upsample.h) -- writes the bits the standalone kernel writes on that function's materialised outputs.
//
// Mapping (both kernels): the quad mapping of ofdis_quad.h.  A lane evaluates the two flows at its pixels once and then loops
// over all times, writing the quad's 4 * noc bytes per time (quad_store); a frame's flows and u8 frames are read into one L2.
#include "ofdis_upsample.h"

namespace ofdis {

// The header's definition for the quad of pixels x .. x+3 of row y (those < W).  `flow(d, xx)` gives direction d's flow at
// pixel (xx, y) of the frame; `consistent(d, nx, ny)` whether direction d's mask at (nx, ny) is OFDIS_FB_CONSISTENT.
// `out_row` points at pixel (0, y) of time 0's output frame, `tstride` is the size of one output frame in bytes, `vec` is
// quad_vec of the output.
template <int NOC, class Flow, class Consistent>
__device__ __forceinline__ void interp_quad(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, uint8_t* out_row,
                                            size_t tstride, int x, int y, int W, int H, const InterpTimes& ts, bool vec,
                                            Flow flow, Consistent consistent) {
  const int np = min(4, W - x);
  float2 f01[4], f10[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < np) { f01[i] = flow(0, x + i); f10[i] = flow(1, x + i); }
    else { f01[i] = make_float2(0.0f, 0.0f); f10[i] = f01[i]; }
  }
  for (int k = 0; k < ts.n; ++k) {
    const float t = ts.t[k];
    const float s = 1.0f - t, a = s * t, tt = t * t, ss = s * s;
    // at t = 0 and t = 1 the weights are (1, 0) and (0, 1) whatever the masks say
    const bool need_masks = t > 0.0f && t < 1.0f;
    uint8_t q[4 * NOC];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float u0 = f01[i].x, v0 = f01[i].y, u1 = f10[i].x, v1 = f10[i].y;
      const float ft0x = tt * u1 - a * u0, ft0y = tt * v1 - a * v0;
      const float ft1x = ss * u0 - a * u1, ft1y = ss * v0 - a * v1;
      const float p0x = (float)(x + i) + ft0x, p0y = (float)y + ft0y;
      const float p1x = (float)(x + i) + ft1x, p1y = (float)y + ft1y;
      const float p0xc = fminf(fmaxf(p0x, 0.0f), (float)(W - 1)), p0yc = fminf(fmaxf(p0y, 0.0f), (float)(H - 1));
      const float p1xc = fminf(fmaxf(p1x, 0.0f), (float)(W - 1)), p1yc = fminf(fmaxf(p1y, 0.0f), (float)(H - 1));
      float c0[3], c1[3];
      interp_sample(A, W, H, NOC, p0xc, p0yc, c0);
      interp_sample(B, W, H, NOC, p1xc, p1yc, c1);
      float w0 = s, w1 = t;
      if (need_masks) {
        const bool m0 = fb_inside(p0x, p0y, W, H) &&
                        consistent(0, min((int)floorf(p0xc + 0.5f), W - 1), min((int)floorf(p0yc + 0.5f), H - 1));
        const bool m1 = fb_inside(p1x, p1y, W, H) &&
                        consistent(1, min((int)floorf(p1xc + 0.5f), W - 1), min((int)floorf(p1yc + 0.5f), H - 1));
        if (m0 != m1) {  // t is inside (0, 1) here: the consistent side alone
          w0 = m0 ? 1.0f : 0.0f;
          w1 = m0 ? 0.0f : 1.0f;
        }
      } else if (t >= 1.0f) {
        w0 = 0.0f; w1 = 1.0f;
      } else {
        w0 = 1.0f; w1 = 0.0f;
      }
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) q[i * NOC + ch] = quad_u8(w0 * c0[ch] + w1 * c1[ch]);
    }
    quad_store<NOC>(out_row + k * tstride + (size_t)x * NOC, q, np, vec);
  }
}

// Materialised arrays: flows [n][H][W][2], masks [n][H][W] or null, frames [n][H][W][NOC], out [n][nt][H][W][NOC].
template <int NOC>
__global__ __launch_bounds__(256) void interp_frames_kernel(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b,
                                                            const float2* __restrict__ ffw, const float2* __restrict__ frev,
                                                            const uint8_t* __restrict__ mfw, const uint8_t* __restrict__ mrev,
                                                            uint8_t* __restrict__ out, QuadLaunch ql, int W, int H,
                                                            InterpTimes ts, bool vec) {
  QuadLane l;
  if (!quad_lane(ql, W, H, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const size_t plane = (size_t)W * H;
  const float2* fl[2] = {ffw + f * plane + (size_t)y * W, frev + f * plane + (size_t)y * W};
  const uint8_t* mk[2] = {mfw ? mfw + f * plane : nullptr, mrev ? mrev + f * plane : nullptr};
  uint8_t* out_row = out + ((size_t)f * ts.n * H + y) * W * NOC;
  interp_quad<NOC>(img_a + f * plane * NOC, img_b + f * plane * NOC, out_row, plane * NOC, x, y, W, H, ts, vec,
                   [&](int d, int xx) { return fl[d][xx]; },
                   [&](int d, int nx, int ny) { return !mk[d] || mk[d][(size_t)ny * W + nx] == FB_CONSISTENT; });
}

// An OFDIS_BATCH_REVERSE context's level flows (UpGeom): the flows at the quad's pixels and the fb codes at the sampled pixels
// recomputed with the helpers upsample_bidir_kernel (ofdis_upsample.hip) uses -- upsample_at, fb_code on UpNeighbours -- the
// codes per time at the two pixels the warps land nearest to.
template <int NOC>
__global__ __launch_bounds__(256) void interp_bidir_kernel(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b,
                                                           const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                           uint8_t* __restrict__ out, QuadLaunch ql, UpGeom g,
                                                           InterpTimes ts, float alpha, float beta, bool vec) {
  const int wo = g.wo, ho = g.ho;
  QuadLane l;
  if (!quad_lane(ql, wo, ho, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const float2* flw[2] = {fw + (size_t)f * g.plane(), rev + (size_t)f * g.plane()};
  const UpRow ry = up_row(y + g.top, g);
  const size_t plane = (size_t)wo * ho;
  uint8_t* out_row = out + ((size_t)f * ts.n * ho + y) * wo * NOC;
  interp_quad<NOC>(img_a + f * plane * NOC, img_b + f * plane * NOC, out_row, plane * NOC, x, y, wo, ho, ts, vec,
                   [&](int d, int xx) { return upsample_at(flw[d], g, xx + g.left, ry); },
                   [&](int d, int nx, int ny) {
                     const float2 val = upsample_at(flw[d], g, nx + g.left, ny + g.top);
                     return fb_code(val.x, val.y, nx, ny, wo, ho, alpha, beta, UpNeighbours{flw[1 - d], g}) == FB_CONSISTENT;
                   });
}

hipError_t launch_interp_frames(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                                const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int w, int h,
                                int noc, const InterpTimes& ts, hipStream_t s) {
  const float2 *ff = (const float2*)flow_fw, *fr = (const float2*)flow_rev;
  const bool vec = quad_vec(w, out);
  return quad_chunks(nframes, w, h, [&](const QuadLaunch& ql, dim3 blocks) {
    if (noc == 3)
      hipLaunchKernelGGL(interp_frames_kernel<3>, blocks, dim3(256), 0, s, img_a, img_b, ff, fr, mask_fw, mask_rev, out, ql, w, h,
                         ts, vec);
    else
      hipLaunchKernelGGL(interp_frames_kernel<1>, blocks, dim3(256), 0, s, img_a, img_b, ff, fr, mask_fw, mask_rev, out, ql, w, h,
                         ts, vec);
    return hipGetLastError();
  });
}

hipError_t launch_interp_bidir(const uint8_t* img_a, const uint8_t* img_b, const float* fw, const float* rev, uint8_t* out,
                               int nframes, UpGeom ug, int noc, const InterpTimes& ts, float alpha, float beta, hipStream_t s) {
  const float2 *ff = (const float2*)fw, *fr = (const float2*)rev;
  const bool vec = quad_vec(ug.wo, out);
  return quad_chunks(nframes, ug.wo, ug.ho, [&](const QuadLaunch& ql, dim3 blocks) {
    if (noc == 3)
      hipLaunchKernelGGL(interp_bidir_kernel<3>, blocks, dim3(256), 0, s, img_a, img_b, ff, fr, out, ql, ug, ts, alpha, beta, vec);
    else
      hipLaunchKernelGGL(interp_bidir_kernel<1>, blocks, dim3(256), 0, s, img_a, img_b, ff, fr, out, ql, ug, ts, alpha, beta, vec);
    return hipGetLastError();
  });
}

}  // namespace ofdis
