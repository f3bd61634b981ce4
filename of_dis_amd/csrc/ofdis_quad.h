// ofdis_quad.h -- the quad mapping of ofdis_interp.hip, ofdis_tfilter.hip, ofdis_trajfilter.hip, ofdis_gmotion.hip and
// ofdis_stabilize.hip, stated once: one lane owns a quad of 4 adjacent pixels of one row of one frame, a workgroup holds 256
// quads, the workgroups of a frame stay on one XCD (xcd_frame_map), and the launcher walks the frames in chunks below
// QUAD_MAX_BLOCKS.  Here are the geometry (quad_grid, quad_blocks), the chunk walk (quad_chunks), what a lane makes of its
// workgroup index (quad_lane) and how it writes its quad of 8-bit values (quad_u8, quad_store, quad_vec).
#pragma once
#include <algorithm>

#include "ofdis_kernels.h"

namespace ofdis {

// ------------------------------------------------------------------------------------ host: geometry and the chunk walk
// Blocks of 256 quads per frame, and the frames of one launch: a launch covers at most QUAD_MAX_BLOCKS = 2^22 blocks (2^30
// lanes; ofdis_kernels.h), a multiple of 8 frames where it can (xcd_frame_map), and the launcher walks the frames in such chunks.
struct QuadGrid {
  int bpf, chunk;
};
inline QuadGrid quad_grid(int nframes, int w, int h) {
  QuadGrid g;
  g.bpf = (int)(((long long)((w + 3) >> 2) * h + 255) / 256);
  long long c = quad_max_blocks() / g.bpf;
  if (c >= 8) c &= ~7ll;
  g.chunk = (int)std::max(1ll, std::min(c, (long long)nframes));
  return g;
}
inline unsigned quad_blocks(int frames, int bpf) {
  const long long fr = frames < 8 ? frames : (frames + 7) / 8 * 8;
  return (unsigned)(fr * bpf);
}

// what a kernel knows of its launch: it works on the frames [f0, f0 + n) of the call, with bpf blocks per frame
struct QuadLaunch {
  int f0, n, bpf;
};
// The launches of one call over `nframes` frames of w x h: `launch(const QuadLaunch&, dim3 blocks)` once per chunk.  It returns
// the launch's error (hipGetLastError()); the walk ends at the first one and returns it.  The runtime is asked by the callback
// and not here, so that the host test of this loop, whose callback records and launches nothing, needs no device.
template <class Launch>
inline hipError_t quad_chunks(int nframes, int w, int h, Launch launch) {
  const QuadGrid g = quad_grid(nframes, w, h);
  for (int f0 = 0; f0 < nframes; f0 += g.chunk) {
    const int n = std::min(g.chunk, nframes - f0);
    const hipError_t e = launch(QuadLaunch{f0, n, g.bpf}, dim3(quad_blocks(n, g.bpf)));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// whether an array of rows of w pixels can take quad_store's 4-byte stores: rows a multiple of 4 pixels, the array 4-byte aligned
inline bool quad_vec(int w, const void* p) { return (w & 3) == 0 && ((uintptr_t)p & 3) == 0; }

// ------------------------------------------------------------------------------------ device: the lane and its stores
// The lane's frame of the call, the block of that frame and the quad's first pixel (x, y).  False: the whole workgroup has
// nothing to do (xcd_frame_map's padding frames).  `active` is false for a lane past the last quad of the frame (x = y = 0,
// nothing is read): a kernel with a workgroup barrier keeps such lanes, every other returns on !active.
struct QuadLane {
  int f, blk, x, y;
  bool active;
};
__device__ __forceinline__ bool quad_lane(const QuadLaunch& q, int W, int H, QuadLane& l) {
  int lf;
  xcd_frame_map(blockIdx.x, q.bpf, q.n, lf, l.blk);
  if (lf >= q.n) return false;
  l.f = q.f0 + lf;
  const int qpr = (W + 3) >> 2;
  const int qi = l.blk * 256 + threadIdx.x;
  l.active = qi < qpr * H;
  l.y = l.active ? qi / qpr : 0;
  l.x = l.active ? (qi - l.y * qpr) * 4 : 0;
  return true;
}

// a float to an 8-bit pixel: round half up, saturate (a NaN becomes 0)
__device__ __forceinline__ uint8_t quad_u8(float v) { return (uint8_t)min(max((int)floorf(v + 0.5f), 0), 255); }

// The quad's 4 * N bytes q to o, its first pixel in an array of N bytes per pixel; np <= 4 pixels of it are inside the row.
// `vec` (quad_vec) and a whole quad: N 4-byte non-temporal stores (no array written here is read again by this library);
// otherwise exactly np * N single bytes.
template <int N>
__device__ __forceinline__ void quad_store(uint8_t* o, const uint8_t (&q)[4 * N], int np, bool vec) {
  if (vec && np == 4) {
    unsigned wd[N];
#pragma unroll
    for (int j = 0; j < N; ++j)
      wd[j] = (unsigned)q[4 * j] | ((unsigned)q[4 * j + 1] << 8) | ((unsigned)q[4 * j + 2] << 16) | ((unsigned)q[4 * j + 3] << 24);
#pragma unroll
    for (int j = 0; j < N; ++j) __builtin_nontemporal_store(wd[j], reinterpret_cast<unsigned*>(o) + j);
  } else {
#pragma unroll
    for (int j = 0; j < 4 * N; ++j)
      if (j < np * N) o[j] = q[j];
  }
}

}  // namespace ofdis
