// ofdis_interp.hip -- frame interpolation from bidirectional flow with occlusion masks (include/ofdis.h: ofdis_interpolate,
// ofdis_batch_interpolate).  Backward warping of both frames to time t with the flows of Jiang et al., "Super SloMo"
// (CVPR 2018, eq. 4), blended by t where both warps are consistent and taken from the one consistent side elsewhere.
//
// Compiled under the exact contract only (-ffp-contract=off): every operation of the header's definition is a separately
// rounded fp32 operation, so the output is a fixed function of the inputs and the fused kernel below -- which recomputes
// the full-resolution flows and the masks from the level flows with the helpers of ofdis_batch_upsample_bidir
// (ofdis_upsample.h) -- writes the bits the standalone kernel writes on that function's materialised outputs.
//
// Mapping (both kernels): one lane owns a quad of 4 adjacent output pixels of one row; it evaluates the two flows at its
// pixels once and then loops over all times, writing the quad's 4 * noc bytes per time (one dword for gray, three for RGB,
// non-temporal: the output is never read by this library).  The workgroups of a frame stay on one XCD (xcd_frame_map), so a
// frame's flows and u8 frames are read into one L2.
#include "ofdis_upsample.h"

namespace ofdis {

// The header's definition for the quad of pixels x .. x+3 of row y (those < W).  `flow(d, xx)` gives direction d's flow at
// pixel (xx, y) of the frame; `consistent(d, nx, ny)` whether direction d's mask at (nx, ny) is OFDIS_FB_CONSISTENT.
// `out_row` points at pixel (0, y) of time 0's output frame, `tstride` is the size of one output frame in bytes.
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
      for (int ch = 0; ch < NOC; ++ch) {
        const int v = (int)floorf((w0 * c0[ch] + w1 * c1[ch]) + 0.5f);
        q[i * NOC + ch] = (uint8_t)min(max(v, 0), 255);
      }
    }
    uint8_t* o = out_row + k * tstride + (size_t)x * NOC;
    if (vec) {  // whole quad inside the row, rows 4-byte aligned
      unsigned wd[NOC];
#pragma unroll
      for (int j = 0; j < NOC; ++j)
        wd[j] = (unsigned)q[4 * j] | ((unsigned)q[4 * j + 1] << 8) | ((unsigned)q[4 * j + 2] << 16) | ((unsigned)q[4 * j + 3] << 24);
#pragma unroll
      for (int j = 0; j < NOC; ++j) __builtin_nontemporal_store(wd[j], reinterpret_cast<unsigned*>(o) + j);
    } else {
#pragma unroll
      for (int j = 0; j < 4 * NOC; ++j)
        if (j < np * NOC) o[j] = q[j];
    }
  }
}

// Materialised arrays: flows [n][H][W][2], masks [n][H][W] or null, frames [n][H][W][NOC], out [n][nt][H][W][NOC].
template <int NOC>
__global__ __launch_bounds__(256) void interp_frames_kernel(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b,
                                                            const float2* __restrict__ ffw, const float2* __restrict__ frev,
                                                            const uint8_t* __restrict__ mfw, const uint8_t* __restrict__ mrev,
                                                            uint8_t* __restrict__ out, int nframes, int W, int H, int bpf,
                                                            InterpTimes ts, bool vec_ok) {
  int f, blk;
  xcd_frame_map(blockIdx.x, bpf, nframes, f, blk);
  const int qpr = (W + 3) >> 2;
  const int qi = blk * 256 + threadIdx.x;
  if (f >= nframes || qi >= qpr * H) return;
  const int y = qi / qpr, x = (qi - y * qpr) * 4;
  const size_t plane = (size_t)W * H;
  const float2* fl[2] = {ffw + f * plane + (size_t)y * W, frev + f * plane + (size_t)y * W};
  const uint8_t* mk[2] = {mfw ? mfw + f * plane : nullptr, mrev ? mrev + f * plane : nullptr};
  uint8_t* out_row = out + ((size_t)f * ts.n * H + y) * W * NOC;
  interp_quad<NOC>(img_a + f * plane * NOC, img_b + f * plane * NOC, out_row, plane * NOC, x, y, W, H, ts,
                   vec_ok && x + 4 <= W, [&](int d, int xx) { return fl[d][xx]; },
                   [&](int d, int nx, int ny) { return !mk[d] || mk[d][(size_t)ny * W + nx] == FB_CONSISTENT; });
}

// An OFDIS_BATCH_REVERSE context's level flows (UpGeom): the flows at the quad's pixels and the fb codes at the sampled pixels
// recomputed with the helpers upsample_bidir_kernel (ofdis_upsample.hip) uses -- upsample_at, fb_code on UpNeighbours -- the
// codes per time at the two pixels the warps land nearest to.
template <int NOC>
__global__ __launch_bounds__(256) void interp_bidir_kernel(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b,
                                                           const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                           uint8_t* __restrict__ out, int nframes, UpGeom g, int bpf,
                                                           InterpTimes ts, float alpha, float beta, bool vec_ok) {
  int f, blk;
  xcd_frame_map(blockIdx.x, bpf, nframes, f, blk);
  const int wo = g.wo, ho = g.ho;
  const int qpr = (wo + 3) >> 2;
  const int qi = blk * 256 + threadIdx.x;
  if (f >= nframes || qi >= qpr * ho) return;
  const int y = qi / qpr, x = (qi - y * qpr) * 4;
  const float2* flw[2] = {fw + (size_t)f * g.plane(), rev + (size_t)f * g.plane()};
  const UpRow ry = up_row(y + g.top, g);
  const size_t plane = (size_t)wo * ho;
  uint8_t* out_row = out + ((size_t)f * ts.n * ho + y) * wo * NOC;
  interp_quad<NOC>(img_a + f * plane * NOC, img_b + f * plane * NOC, out_row, plane * NOC, x, y, wo, ho, ts,
                   vec_ok && x + 4 <= wo, [&](int d, int xx) { return upsample_at(flw[d], g, xx + g.left, ry); },
                   [&](int d, int nx, int ny) {
                     const float2 val = upsample_at(flw[d], g, nx + g.left, ny + g.top);
                     return fb_code(val.x, val.y, nx, ny, wo, ho, alpha, beta, UpNeighbours{flw[1 - d], g}) == FB_CONSISTENT;
                   });
}

hipError_t launch_interp_frames(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                                const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int w, int h,
                                int noc, const InterpTimes& ts, hipStream_t s) {
  const QuadGrid g = quad_grid(nframes, w, h);
  const bool vec = (w & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t plane = (size_t)w * h;
  for (int f0 = 0; f0 < nframes; f0 += g.chunk) {
    const int n = std::min(g.chunk, nframes - f0);
    const size_t fo = (size_t)f0 * plane;
    const uint8_t* mf = mask_fw ? mask_fw + fo : nullptr;
    const uint8_t* mr = mask_rev ? mask_rev + fo : nullptr;
    const float2* ff = (const float2*)flow_fw + fo;
    const float2* fr = (const float2*)flow_rev + fo;
    uint8_t* o = out + fo * noc * ts.n;
    if (noc == 3)
      hipLaunchKernelGGL(interp_frames_kernel<3>, dim3(quad_blocks(n, g.bpf)), dim3(256), 0, s, img_a + fo * 3, img_b + fo * 3,
                         ff, fr, mf, mr, o, n, w, h, g.bpf, ts, vec);
    else
      hipLaunchKernelGGL(interp_frames_kernel<1>, dim3(quad_blocks(n, g.bpf)), dim3(256), 0, s, img_a + fo, img_b + fo, ff,
                         fr, mf, mr, o, n, w, h, g.bpf, ts, vec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_interp_bidir(const uint8_t* img_a, const uint8_t* img_b, const float* fw, const float* rev, uint8_t* out,
                               int nframes, UpGeom ug, int noc, const InterpTimes& ts, float alpha, float beta, hipStream_t s) {
  const QuadGrid g = quad_grid(nframes, ug.wo, ug.ho);
  const bool vec = (ug.wo & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const size_t plane = (size_t)ug.wo * ug.ho, lplane = ug.plane();
  for (int f0 = 0; f0 < nframes; f0 += g.chunk) {
    const int n = std::min(g.chunk, nframes - f0);
    const float2* ff = (const float2*)fw + (size_t)f0 * lplane;
    const float2* fr = (const float2*)rev + (size_t)f0 * lplane;
    uint8_t* o = out + (size_t)f0 * plane * noc * ts.n;
    if (noc == 3)
      hipLaunchKernelGGL(interp_bidir_kernel<3>, dim3(quad_blocks(n, g.bpf)), dim3(256), 0, s, img_a + (size_t)f0 * plane * 3,
                         img_b + (size_t)f0 * plane * 3, ff, fr, o, n, ug, g.bpf, ts, alpha, beta, vec);
    else
      hipLaunchKernelGGL(interp_bidir_kernel<1>, dim3(quad_blocks(n, g.bpf)), dim3(256), 0, s, img_a + (size_t)f0 * plane,
                         img_b + (size_t)f0 * plane, ff, fr, o, n, ug, g.bpf, ts, alpha, beta, vec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ofdis
