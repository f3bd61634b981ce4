// ofdis_trajfilter.hip -- temporal filtering of a clip along flow trajectories over 2R + 1 frames (include/ofdis.h:
// ofdis_trajectory_filter on materialised flows, ofdis_batch_trajectory_filter straight from the level flows of an
// OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context): every output pixel walks R steps forward and R steps back through the
// flows of consecutive pairs (the walk of ofdis_track.hip), samples the frame at every stop, and a direction ends where the
// path leaves the image or fails the forward-backward test.
//
// Compiled under the exact contract only (-ffp-contract=off): every operation of the header's definition is a separately
// rounded fp32 operation, stated once in ofdis_upsample.h (fb_inside, fb_bilinear, fb_consistent, interp_sample), so the
// output is a fixed function of the inputs and the fused kernel -- which takes a flow at a pixel with upsample_at and the four
// taps around a real position with UpNeighbours, as every other finish kernel does -- writes the bits the standalone kernel
// writes on the materialised outputs of ofdis_batch_upsample_bidir.
//
// Mapping (both kernels): the quad mapping of ofdis_quad.h over the OUTPUT frames.  A step of a walk is a chain of dependent
// gathers (the flow at p, the other direction's flow at q, the frame at q); the lane's four walks of one direction take each
// link of that chain together and without a branch -- a walk that has ended goes on gathering at its last position, which is
// inside the image, and its results are discarded -- so four independent gathers are in flight per lane and link, and the
// wavefronts of a CU hide the rest.  A frame is read by the 2R + 1 output frames around it, which one launch works on at
// about the same time.  No LDS; the weights and the radius travel in the launch arguments.
#include "ofdis_upsample.h"

namespace ofdis {

// what both kernels are launched with: the clip, the outputs, the output frames of this launch
struct TrajArgs {
  const uint8_t* frames;  // [npairs + 1][H][W][NOC]
  uint8_t* out;           // [npairs + 1][H][W][NOC]
  uint8_t* support;       // [npairs + 1][H][W] or null
  QuadLaunch q;
  int npairs;
  TrajWeights w;
  float tau, alpha, beta;
  bool fb;                // with the consistency test
  bool vec_out, vec_sup;  // quad_vec of out and support
};

// The header's definition for the quad of pixels x .. x+3 of row y (those < W) of output frame f.  `first(k, r, xx)` gives
// pair k's flow at integer pixel (xx, y) -- r = 0: frame k -> k + 1, r = 1: the reverse -- and `taps(k, r)` that flow at four
// integer pixels (fb_bilinear's R).  Direction d = 0 walks back, d = 1 forward: the order in which the sums take them.
template <int NOC, class First, class Taps>
__device__ __forceinline__ void traj_quad(const TrajArgs& a, int f, int x, int y, int W, int H, First first, Taps taps) {
  const int np = min(4, W - x);
  const size_t plane = (size_t)W * H;
  const uint8_t* crow = a.frames + (f * plane + (size_t)y * W + x) * NOC;
  float c[4][3], num[4][3], den[4];
  float2 p[2][4];    // where each walk stands: always inside the image
  bool live[2][4];
  unsigned reach[4];  // nf | nb << 4
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) num[i][ch] = c[i][ch] = ch < NOC && i < np ? (float)crow[i * NOC + ch] : 0.0f;
    den[i] = 1.0f;
    reach[i] = 0;
    p[0][i] = p[1][i] = make_float2((float)min(x + i, W - 1), (float)y);
    live[0][i] = live[1][i] = i < np;
  }
  for (int j = 1; j <= a.w.radius; ++j) {
    const float wj = a.w.w[j - 1];
    float wd[2][4], s[2][4][3];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wd[d][i] = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[d][i][ch] = 0.0f;
      }
      const int k = d ? f + j - 1 : f - j;  // the pair this step crosses
      if (k < 0 || k >= a.npairs || !(live[d][0] || live[d][1] || live[d][2] || live[d][3])) {
#pragma unroll
        for (int i = 0; i < 4; ++i) live[d][i] = false;
        continue;
      }
      const uint8_t* J = a.frames + (size_t)(d ? f + j : f - j) * plane * NOC;
      const int r = d ? 0 : 1;  // the flow that leads on; 1 - r leads back
      float2 uv[4], q[4];
      bool ok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uv[i] = j == 1 ? first(k, r, min(x + i, W - 1)) : fb_bilinear(p[d][i].x, p[d][i].y, W, H, taps(k, r));
        q[i] = make_float2(p[d][i].x + uv[i].x, p[d][i].y + uv[i].y);
        ok[i] = live[d][i] && fb_inside(q[i].x, q[i].y, W, H);
        if (!ok[i]) q[i] = p[d][i];  // an ended walk stays where it is: the gathers below stay inside, their results are dropped
      }
      if (a.fb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float2 o = fb_bilinear(q[i].x, q[i].y, W, H, taps(k, 1 - r));
          ok[i] = ok[i] && fb_consistent(uv[i].x, uv[i].y, o.x, o.y, a.alpha, a.beta);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float sv[3] = {0.0f, 0.0f, 0.0f};
        interp_sample(J, W, H, NOC, q[i].x, q[i].y, sv);
        float dm = fabsf(sv[0] - c[i][0]);
#pragma unroll
        for (int ch = 1; ch < NOC; ++ch) dm = fmaxf(dm, fabsf(sv[ch] - c[i][ch]));
        const float g = fmaxf(1.0f - dm / a.tau, 0.0f);
        if (ok[i]) {
          wd[d][i] = wj * g;
#pragma unroll
          for (int ch = 0; ch < NOC; ++ch) s[d][i][ch] = sv[ch];
        }
        p[d][i] = q[i];
        live[d][i] = ok[i];
        reach[i] += wd[d][i] > 0.0f ? (d ? 1u : 16u) : 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) num[i][ch] = (num[i][ch] + wd[0][i] * s[0][i][ch]) + wd[1][i] * s[1][i][ch];
      den[i] = (den[i] + wd[0][i]) + wd[1][i];
    }
  }
  uint8_t o8[4 * NOC], sup[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) o8[i * NOC + ch] = quad_u8(num[i][ch] / den[i]);
    sup[i] = (uint8_t)reach[i];
  }
  const size_t px0 = f * plane + (size_t)y * W + x;  // the quad's first pixel in a [frames][H][W] array
  quad_store<NOC>(a.out + px0 * NOC, o8, np, a.vec_out);
  if (a.support) quad_store<1>(a.support + px0, sup, np, a.vec_sup);
}

// materialised flows [npairs][H][W][2]: step 1 reads the pixel's flow directly, later steps its four taps (FlowTaps)
template <int NOC>
__global__ __launch_bounds__(256) void trajfilter_frames_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                                int W, int H, TrajArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, W, H, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const size_t plane = (size_t)W * H;
  traj_quad<NOC>(a, f, x, y, W, H, [&](int k, int r, int xx) { return ((r ? rev : fw) + k * plane)[(size_t)y * W + xx]; },
                 [&](int k, int r) { return FlowTaps{(r ? rev : fw) + k * plane, W}; });
}

// level flows [npairs][sh][sw][2] of a context (UpGeom): the full-resolution values recomputed, at the pixel with upsample_at
// and at the taps with UpNeighbours -- the bits ofdis_batch_upsample_bidir writes
template <int NOC>
__global__ __launch_bounds__(256) void trajfilter_level_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                               UpGeom g, TrajArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, g.wo, g.ho, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const UpRow ry = up_row(y + g.top, g);
  traj_quad<NOC>(a, f, x, y, g.wo, g.ho,
                 [&](int k, int r, int xx) { return upsample_at((r ? rev : fw) + k * g.plane(), g, xx + g.left, ry); },
                 [&](int k, int r) { return UpNeighbours{(r ? rev : fw) + k * g.plane(), g}; });
}

static TrajArgs traj_args(const uint8_t* frames, uint8_t* out, uint8_t* support, int npairs, int w, const TrajWeights& tw,
                          float tau, bool fb, float alpha, float beta) {
  return TrajArgs{frames, out, support, QuadLaunch{}, npairs, tw, tau, alpha, beta, fb, quad_vec(w, out), quad_vec(w, support)};
}

hipError_t launch_trajfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out,
                                    uint8_t* support, int npairs, int w, int h, int noc, const TrajWeights& tw, float tau,
                                    bool fb, float alpha, float beta, hipStream_t s) {
  const float2 *ff = (const float2*)flow_fw, *fr = (const float2*)flow_rev;
  TrajArgs a = traj_args(frames, out, support, npairs, w, tw, tau, fb, alpha, beta);
  return quad_chunks(npairs + 1, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL(trajfilter_frames_kernel<3>, blocks, dim3(256), 0, s, ff, fr, w, h, a);
    else
      hipLaunchKernelGGL(trajfilter_frames_kernel<1>, blocks, dim3(256), 0, s, ff, fr, w, h, a);
    return hipGetLastError();
  });
}

hipError_t launch_trajfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                   int npairs, UpGeom ug, int noc, const TrajWeights& tw, float tau, bool fb, float alpha,
                                   float beta, hipStream_t s) {
  const float2 *ff = (const float2*)fw, *fr = (const float2*)rev;
  TrajArgs a = traj_args(frames, out, support, npairs, ug.wo, tw, tau, fb, alpha, beta);
  return quad_chunks(npairs + 1, ug.wo, ug.ho, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL(trajfilter_level_kernel<3>, blocks, dim3(256), 0, s, ff, fr, ug, a);
    else
      hipLaunchKernelGGL(trajfilter_level_kernel<1>, blocks, dim3(256), 0, s, ff, fr, ug, a);
    return hipGetLastError();
  });
}

}  // namespace ofdis
