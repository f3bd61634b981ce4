// ofdis_tfilter.hip -- motion-compensated temporal filtering of a clip (include/ofdis.h: ofdis_temporal_filter on materialised
// arrays, ofdis_batch_temporal_filter straight from the level flows of an OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context):
// frame f averaged with frames f-1 and f+1 warped onto it, a neighbour left out where the forward-backward test flags the
// pixel or its sample falls outside, and faded out by the photometric gate tau.
//
// Compiled under the exact contract only (-ffp-contract=off): every operation of the header's definition is a separately
// rounded fp32 operation (the two divisions are the compiler's correctly rounded expansion), so the output is a fixed function
// of the inputs and the fused kernel below -- which recomputes the full-resolution flows and the codes from the level flows
// with the helpers of ofdis_batch_upsample_bidir (ofdis_upsample.h: upsample_at, fb_code on UpNeighbours) -- writes the bits
// the standalone kernel writes on that function's materialised outputs.
//
// Mapping (both kernels): the quad mapping of ofdis_quad.h over the OUTPUT frames.  A lane reads the quad of frame f, takes up
// to two flows per pixel, gathers the four taps of each valid sample and writes the quad's 4 * noc bytes and its 4 support
// bytes (quad_store).  A frame is read three times -- as the centre of its own output and as a neighbour of the two next to
// it, which the same launch works on at about the same time.
#include "ofdis_upsample.h"

namespace ofdis {

// what both kernels are launched with: the clip, the outputs, the output frames of this launch
struct TfArgs {
  const uint8_t* frames;  // [npairs + 1][H][W][NOC]
  uint8_t* out;           // [npairs + 1][H][W][NOC]
  uint8_t* support;       // [npairs + 1][H][W] or null
  QuadLaunch q;
  int npairs;
  float wn, tau;
  bool vec_out, vec_sup;  // quad_vec of out and support
};

// The header's definition for the quad of pixels x .. x+3 of row y (those < W) of output frame f.  Candidate d = 0 is the next
// frame (the forward flow of pair f), d = 1 the previous one (the reverse flow of pair f-1): `flow(d, xx)` gives that flow at
// pixel (xx, y), `consistent(d, xx, uv)` whether its code there is OFDIS_FB_CONSISTENT (asked only where the target is inside).
template <int NOC, class Flow, class Consistent>
__device__ __forceinline__ void tfilter_quad(const TfArgs& a, int f, int x, int y, int W, int H, Flow flow, Consistent consistent) {
  const int np = min(4, W - x);
  const size_t plane = (size_t)W * H;
  const uint8_t* cur = a.frames + f * plane * NOC;
  const bool has[2] = {f < a.npairs, f > 0};
  const uint8_t* nb[2] = {has[0] ? cur + plane * NOC : cur, has[1] ? cur - plane * NOC : cur};
  const uint8_t* crow = cur + ((size_t)y * W + x) * NOC;
  uint8_t q[4 * NOC], sup[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float c[3] = {0.0f, 0.0f, 0.0f}, s[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}, w[2] = {0.0f, 0.0f};
    if (i < np) {
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) c[ch] = (float)crow[i * NOC + ch];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        if (!has[d]) continue;
        const float2 uv = flow(d, x + i);
        const float px = (float)(x + i) + uv.x, py = (float)y + uv.y;
        if (!fb_inside(px, py, W, H) || !consistent(d, x + i, uv)) continue;
        interp_sample(nb[d], W, H, NOC, px, py, s[d]);
        float dm = fabsf(s[d][0] - c[0]);
#pragma unroll
        for (int ch = 1; ch < NOC; ++ch) dm = fmaxf(dm, fabsf(s[d][ch] - c[ch]));
        w[d] = a.wn * fmaxf(1.0f - dm / a.tau, 0.0f);
      }
    }
    const float den = (1.0f + w[1]) + w[0];
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) {
      const float num = (c[ch] + w[1] * s[1][ch]) + w[0] * s[0][ch];
      q[i * NOC + ch] = quad_u8(num / den);
    }
    sup[i] = (uint8_t)((w[1] > 0.0f ? 1 : 0) | (w[0] > 0.0f ? 2 : 0));
  }
  const size_t px0 = f * plane + (size_t)y * W + x;  // the quad's first pixel in a [frames][H][W] array
  quad_store<NOC>(a.out + px0 * NOC, q, np, a.vec_out);
  if (a.support) quad_store<1>(a.support + px0, sup, np, a.vec_sup);
}

// Materialised arrays: flows [npairs][H][W][2], masks [npairs][H][W] or null.
template <int NOC>
__global__ __launch_bounds__(256) void tfilter_frames_kernel(const float2* __restrict__ ffw, const float2* __restrict__ frev,
                                                             const uint8_t* __restrict__ mfw, const uint8_t* __restrict__ mrev,
                                                             int W, int H, TfArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, W, H, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const size_t plane = (size_t)W * H;
  // candidate 0 belongs to pair f, candidate 1 to pair f - 1 (a pair that does not exist is never read: tfilter_quad)
  const size_t row[2] = {min(f, a.npairs - 1) * plane + (size_t)y * W, max(f - 1, 0) * plane + (size_t)y * W};
  const float2* fl[2] = {ffw + row[0], frev + row[1]};
  const uint8_t* mk[2] = {mfw ? mfw + row[0] : nullptr, mrev ? mrev + row[1] : nullptr};
  tfilter_quad<NOC>(a, f, x, y, W, H, [&](int d, int xx) { return fl[d][xx]; },
                    [&](int d, int xx, float2) { return !mk[d] || mk[d][xx] == FB_CONSISTENT; });
}

// An OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE context's level flows (UpGeom): the flows at the quad's pixels and their codes
// recomputed with the helpers upsample_bidir_kernel (ofdis_upsample.hip) uses -- upsample_at, fb_code on the UpNeighbours of
// the same pair's other direction.
template <int NOC>
__global__ __launch_bounds__(256) void tfilter_level_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                            UpGeom g, float alpha, float beta, TfArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, g.wo, g.ho, l) || !l.active) return;
  const int f = l.f, x = l.x, y = l.y;
  const size_t pair[2] = {(size_t)min(f, a.npairs - 1) * g.plane(), (size_t)max(f - 1, 0) * g.plane()};
  const float2* fl[2] = {fw + pair[0], rev + pair[1]};     // the flow from frame f to the neighbour ...
  const float2* other[2] = {rev + pair[0], fw + pair[1]};  // ... and the same pair's flow back
  const UpRow ry = up_row(y + g.top, g);
  tfilter_quad<NOC>(a, f, x, y, g.wo, g.ho, [&](int d, int xx) { return upsample_at(fl[d], g, xx + g.left, ry); },
                    [&](int d, int xx, float2 uv) {
                      return fb_code(uv.x, uv.y, xx, y, g.wo, g.ho, alpha, beta, UpNeighbours{other[d], g}) == FB_CONSISTENT;
                    });
}

static TfArgs tfilter_args(const uint8_t* frames, uint8_t* out, uint8_t* support, int npairs, int w, float wn, float tau) {
  return TfArgs{frames, out, support, QuadLaunch{}, npairs, wn, tau, quad_vec(w, out), quad_vec(w, support)};
}

hipError_t launch_tfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                                 const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int w, int h, int noc,
                                 float wn, float tau, hipStream_t s) {
  const float2 *ff = (const float2*)flow_fw, *fr = (const float2*)flow_rev;
  TfArgs a = tfilter_args(frames, out, support, npairs, w, wn, tau);
  return quad_chunks(npairs + 1, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL(tfilter_frames_kernel<3>, blocks, dim3(256), 0, s, ff, fr, mask_fw, mask_rev, w, h, a);
    else
      hipLaunchKernelGGL(tfilter_frames_kernel<1>, blocks, dim3(256), 0, s, ff, fr, mask_fw, mask_rev, w, h, a);
    return hipGetLastError();
  });
}

hipError_t launch_tfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                int npairs, UpGeom ug, int noc, float wn, float tau, float alpha, float beta, hipStream_t s) {
  const float2 *ff = (const float2*)fw, *fr = (const float2*)rev;
  TfArgs a = tfilter_args(frames, out, support, npairs, ug.wo, wn, tau);
  return quad_chunks(npairs + 1, ug.wo, ug.ho, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    if (noc == 3)
      hipLaunchKernelGGL(tfilter_level_kernel<3>, blocks, dim3(256), 0, s, ff, fr, ug, alpha, beta, a);
    else
      hipLaunchKernelGGL(tfilter_level_kernel<1>, blocks, dim3(256), 0, s, ff, fr, ug, alpha, beta, a);
    return hipGetLastError();
  });
}

}  // namespace ofdis
