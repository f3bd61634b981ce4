// ofdis_track.hip -- dense point trajectories through a clip (include/ofdis.h: ofdis_track_points on materialised flows,
// ofdis_batch_track_points straight from the level flows of an OFDIS_BATCH_SEQUENCE context): the flows of consecutive pairs
// chained from a seed, each track ended where it leaves the image or fails the forward-backward test (Sundaram, Brox and
// Keutzer, "Dense point trajectories by GPU-accelerated large displacement optical flow", ECCV 2010).
//
// Compiled under the exact contract only (-ffp-contract=off): every operation of the header's definition is a separately
// rounded fp32 operation, stated once in ofdis_upsample.h (fb_track_step: fb_inside, fb_bilinear, fb_consistent), so the
// tracks are a fixed function of the flows and the fused kernel -- which takes the four neighbours of a sample from the pair's
// level flow with the helpers of every other finish kernel (UpNeighbours) -- writes the bits the standalone kernel writes on
// the materialised flows.
//
// Mapping (both kernels): one lane per point, one wavefront per workgroup -- a wavefront marches in lock step and shares
// nothing with its neighbours, so a few thousand points already spread over every compute unit.  The loop over the frames is
// wave-uniform: every lane writes its entry of frame f (the position, or the NaN of a track that has not started or has
// ended: no memset) as one 8-byte store next to its neighbours', and the step to frame f + 1 is predicated on the lanes whose
// track is alive -- before the wavefront's smallest seed frame and after its last live step the loop is its store.  A step is
// a dependent chain of two gathers (forward flow at p, reverse flow at q) of four taps each; the tracks are written once and
// never read by this library: non-temporal stores.
#include "ofdis_kernels.h"
#include "ofdis_upsample.h"

namespace ofdis {

typedef unsigned u2v __attribute__((ext_vector_type(2)));

constexpr unsigned kTrackEnded = 0x7FC00000u;  // both components of an entry outside a track
constexpr int kTrackLanes = 64;

struct TrackArgs {
  const float2* seeds;    // [npoints]
  const int* seed_frame;  // [npoints] or null (0)
  int npoints, npairs, max_steps;
  int W, H;               // full-resolution frame
  float alpha, beta;
  u2v* tracks;            // [npairs + 1][npoints]
  int* counts;            // [npoints] or null
};

// The header's definition for the lane's point.  `taps(k, d)` gives pair k's flow of direction d (0: frame k -> k + 1, 1: the
// reverse) at four integer pixels (fb_bilinear's R).  FB: with the consistency test.
template <bool FB, class Taps>
__device__ __forceinline__ void track_walk(const TrackArgs& a, Taps taps) {
  const int i = blockIdx.x * kTrackLanes + threadIdx.x;
  if (i >= a.npoints) return;
  float2 p = a.seeds[i];
  const int s = a.seed_frame ? a.seed_frame[i] : 0;
  const bool seeded = s >= 0 && s <= a.npairs && fb_inside(p.x, p.y, a.W, a.H);
  // the last frame the track may reach (0 <= s <= npairs where it matters: nothing overflows)
  const int last = seeded && a.max_steps && a.max_steps < a.npairs - s ? s + a.max_steps : a.npairs;
  bool live = false;
  int count = 0;
  for (int f = 0; f <= a.npairs; ++f) {
    if (f == s) live = seeded;
    const u2v entry = live ? (u2v){__float_as_uint(p.x), __float_as_uint(p.y)} : (u2v){kTrackEnded, kTrackEnded};
    __builtin_nontemporal_store(entry, a.tracks + (size_t)f * a.npoints + i);
    if (!live) continue;
    ++count;
    live = f < last;
    if (!live) continue;
    float2 q;
    live = fb_track_step<FB>(p, f, a.W, a.H, a.alpha, a.beta, taps, q);
    p = q;
  }
  if (a.counts) a.counts[i] = count;
}

// materialised flows [npairs][H][W][2]
template <bool FB>
__global__ __launch_bounds__(kTrackLanes) void track_points_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                                   TrackArgs a) {
  const size_t plane = (size_t)a.W * a.H;
  track_walk<FB>(a, [&](int k, int d) { return FlowTaps{(d ? rev : fw) + k * plane, a.W}; });
}

// level flows [npairs][sh][sw][2] of a context (UpGeom): the full-resolution values recomputed at the taps
template <bool FB>
__global__ __launch_bounds__(kTrackLanes) void track_level_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                                  UpGeom g, TrackArgs a) {
  track_walk<FB>(a, [&](int k, int d) { return UpNeighbours{(d ? rev : fw) + k * g.plane(), g}; });
}

static TrackArgs track_args(int npairs, int w, int h, const float* seeds, const int* seed_frame, int npoints, int max_steps,
                            float alpha, float beta, float* tracks, int* counts) {
  return TrackArgs{(const float2*)seeds, seed_frame, npoints, npairs, max_steps, w, h, alpha, beta, (u2v*)tracks, counts};
}
static dim3 track_grid(int npoints) { return dim3((unsigned)((npoints + kTrackLanes - 1) / kTrackLanes)); }

hipError_t launch_track_points(const float* fw, const float* rev, int npairs, int w, int h, const float* seeds,
                               const int* seed_frame, int npoints, int max_steps, float alpha, float beta, float* tracks,
                               int* counts, hipStream_t s) {
  const TrackArgs a = track_args(npairs, w, h, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks, counts);
  if (rev)
    hipLaunchKernelGGL(track_points_kernel<true>, track_grid(npoints), dim3(kTrackLanes), 0, s, (const float2*)fw,
                       (const float2*)rev, a);
  else
    hipLaunchKernelGGL(track_points_kernel<false>, track_grid(npoints), dim3(kTrackLanes), 0, s, (const float2*)fw,
                       (const float2*)nullptr, a);
  return hipGetLastError();
}

hipError_t launch_track_level(const float* fw, const float* rev, int npairs, UpGeom g, const float* seeds, const int* seed_frame,
                              int npoints, int max_steps, float alpha, float beta, float* tracks, int* counts, hipStream_t s) {
  const TrackArgs a = track_args(npairs, g.wo, g.ho, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks, counts);
  if (rev)
    hipLaunchKernelGGL(track_level_kernel<true>, track_grid(npoints), dim3(kTrackLanes), 0, s, (const float2*)fw,
                       (const float2*)rev, g, a);
  else
    hipLaunchKernelGGL(track_level_kernel<false>, track_grid(npoints), dim3(kTrackLanes), 0, s, (const float2*)fw,
                       (const float2*)nullptr, g, a);
  return hipGetLastError();
}

}  // namespace ofdis
