// ofdis_dense_tracks.hip -- dense trajectories through a clip (include/ofdis.h: ofdis_seed_texture, ofdis_dense_tracks on
// materialised flows, ofdis_batch_dense_tracks straight from the level flows of an OFDIS_BATCH_SEQUENCE context): the walk of
// ofdis_track.hip from seeds the library places itself -- the textured centres of a grid, and in every frame again the centres
// of the cells that hold no live track (Sundaram, Brox and Keutzer 2010; Wang et al., "Dense trajectories") -- with the tracks
// capped at Lmax + 1 frames.
//
// Compiled under the exact contract only (-ffp-contract=off).  The step of a track is fb_track_step of ofdis_upsample.h, the
// code ofdis_track.hip walks with, so a slot replays bit for bit through ofdis_track_points; the texture test is integer
// arithmetic.
//
// Mapping.  Whether a cell seeds in frame f depends on where every live track stands in frame f, and where the tracks seeded in
// frame f stand decides frame f + 1: the frames are sequential, and between them stands a dependency of every cell on every
// track.  One workgroup walking the whole clip with __syncthreads would keep that dependency inside a compute unit, but a clip
// holds up to Lmax x cells live tracks (a quarter of a million at 1024 x 436, stride 5, Lmax 15), each step two dependent
// four-tap gathers: one compute unit of 256 would carry all of it.  So the dependency is a launch boundary, and every launch
// spreads over the device:
//   texture   ONE launch for the clip, one lane per (frame, cell): textured(f, centre) does not depend on the tracks
//   per frame f = 0 .. npairs, in stream order and without a host synchronisation:
//     advance (f >= 1)     one lane per slot of the live window: the step with pair f - 1, the entry of frame f, the cell stamp
//     count   (f < npairs) one lane per cell: seeds = textured and not stamped; one count per workgroup
//     assign  (f < npairs) the same lanes: slot = base[f] + the counts of the workgroups before + the rank inside the workgroup
// Slot numbers are a prefix sum over the cell numbers: no atomic, no grid-wide barrier and no wait on another workgroup takes
// part.  ntracks never reaches the host: every grid is sized by a bound the host knows -- the tracks alive in frame f were
// seeded in frames f - Lmax .. f - 1, i.e. they are the slots [base[max(f - Lmax, 0)], base[f]), at most min(Lmax, f) x cells
// and at most max_tracks of them.
//
// State.  The tracks are written once and never read (non-temporal stores, as in ofdis_track.hip); the position and the start
// frame of a slot live in a ring of `cap` = min(Lmax x cells, max_tracks) entries at slot % cap: the live window is never wider
// than the ring, so a new slot only ever takes the entry of a track that has ended.  Occupancy is a frame stamp, occ[cell] =
// f + 1: plain stores of one value need no atomic and no clearing between the frames.
#include "ofdis_kernels.h"
#include "ofdis_upsample.h"

namespace ofdis {

typedef unsigned u2v __attribute__((ext_vector_type(2)));

constexpr unsigned kDenseEnded = 0x7FC00000u;  // both components of an entry outside a track
constexpr int kDenseLanes = 64;                // advance: one wavefront per workgroup, as ofdis_track.hip
constexpr int kDenseCells = 256;               // texture, count, assign: cells per workgroup

// the grid of include/ofdis.h
struct DenseGrid {
  int W, H, stride, ncx, ncy;
  __host__ __device__ int cells() const { return ncx * ncy; }
  __device__ __forceinline__ int cell_of(float px, float py) const {  // a position inside the image
    return min((int)floorf(py) / stride, ncy - 1) * ncx + min((int)floorf(px) / stride, ncx - 1);
  }
};
static DenseGrid dense_grid(int w, int h, int stride) {
  const int off = stride / 2;
  return DenseGrid{w, h, stride, (w - 1 - off) / stride + 1, (h - 1 - off) / stride + 1};
}

// ------------------------------------------------------------------------------------ the texture test
// textured(f, centre of cell c) of include/ofdis.h for the lane's (frame, cell): exact integer arithmetic
template <int NOC>
__global__ __launch_bounds__(kDenseCells) void seed_texture_kernel(const uint8_t* __restrict__ frames, DenseGrid g, int wr, int T,
                                                                   uint8_t* __restrict__ out) {
  const int c = blockIdx.x * kDenseCells + threadIdx.x;
  if (c >= g.cells()) return;
  const int f = blockIdx.y;
  const uint8_t* I = frames + (size_t)f * g.W * g.H * NOC;
  const int off = g.stride / 2;
  const int sx = off + (c % g.ncx) * g.stride, sy = off + (c / g.ncx) * g.stride;
  int sa = 0, sb = 0, sc = 0;  // |sums| <= 255^2 * 3 * 15^2 < 2^26
  for (int j = -wr; j <= wr; ++j) {
    const int y = min(max(sy + j, 0), g.H - 1);
    const uint8_t* row = I + (size_t)y * g.W * NOC;
    const uint8_t* up = I + (size_t)max(y - 1, 0) * g.W * NOC;
    const uint8_t* down = I + (size_t)min(y + 1, g.H - 1) * g.W * NOC;
    for (int i = -wr; i <= wr; ++i) {
      const int x = min(max(sx + i, 0), g.W - 1);
      const int xl = max(x - 1, 0) * NOC, xr = min(x + 1, g.W - 1) * NOC;
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) {
        const int gx = (int)row[xr + ch] - (int)row[xl + ch];
        const int gy = (int)down[x * NOC + ch] - (int)up[x * NOC + ch];
        sa += gx * gx;
        sb += gx * gy;
        sc += gy * gy;
      }
    }
  }
  const long long a = sa, b = sb, cc = sc, t = T;
  out[(size_t)f * g.cells() + c] = a >= t && cc >= t && (a - t) * (cc - t) >= b * b;
}

static hipError_t launch_texture(const uint8_t* frames, int nframes, const DenseGrid& g, int noc, int window, int min_eig,
                                 uint8_t* out, hipStream_t s) {
  const unsigned bx = (unsigned)((g.cells() + kDenseCells - 1) / kDenseCells);
  const size_t frame = (size_t)g.W * g.H * noc;
  for (int f0 = 0; f0 < nframes; f0 += 32768) {  // (the y extent of a grid)
    const dim3 grid(bx, (unsigned)std::min(32768, nframes - f0));
    if (noc == 1)
      hipLaunchKernelGGL(seed_texture_kernel<1>, grid, dim3(kDenseCells), 0, s, frames + f0 * frame, g, window, min_eig,
                         out + (size_t)f0 * g.cells());
    else
      hipLaunchKernelGGL(seed_texture_kernel<3>, grid, dim3(kDenseCells), 0, s, frames + f0 * frame, g, window, min_eig,
                         out + (size_t)f0 * g.cells());
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ the frame loop
struct DenseArgs {
  DenseGrid g;
  int npairs, lmax, max_tracks;
  unsigned cap;    // entries of the ring
  float alpha, beta;
  u2v* tracks;     // [lmax + 1][max_tracks]
  int* start;      // [max_tracks]
  int* len;        // [max_tracks] or null
  long long* info; // {ntracks, dropped}
  // work
  int* base;           // [npairs + 1]: the slots taken before frame f seeds
  long long* dropped;  // seeds without a slot so far
  int* occ;            // [cells]: f + 1 where a live track stands in the cell in frame f
  int* cnt;            // [workgroups of cells]: the seeds of each in the current frame
  const uint8_t* tex;  // [npairs][cells]
  float2* pos;         // [cap]: where the slot's track stands
  int* born;           // [cap]: its start frame, -1 once it has ended
};

struct DenseLayout {
  size_t base, dropped, occ, cnt, tex, pos, born, bytes;
};
static size_t dense_cap(long long generations, int cells, long long max_tracks) {
  return (size_t)std::min(generations * cells, max_tracks);
}
// every array on an 8-byte boundary
static DenseLayout dense_layout(int npairs, int cells, size_t cap) {
  DenseLayout l;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 7) & ~(size_t)7; return here; };
  l.dropped = take(8);
  l.pos = take(cap * sizeof(float2));
  l.base = take(((size_t)npairs + 1) * sizeof(int));
  l.occ = take((size_t)cells * sizeof(int));
  l.cnt = take((size_t)((cells + kDenseCells - 1) / kDenseCells) * sizeof(int));
  l.born = take(cap * sizeof(int));
  l.tex = take((size_t)npairs * cells);
  l.bytes = at;
  return l;
}

// The lane's slot of the live window takes the step to frame f >= 1 (the header's "advance"); `taps` as fb_track_step's.
template <bool FB, class Taps>
__device__ __forceinline__ void dense_advance(const DenseArgs& a, int f, Taps taps) {
  const int w0 = a.base[max(f - a.lmax, 0)], w1 = a.base[f];
  const long long i = (long long)blockIdx.x * kDenseLanes + threadIdx.x;
  if (i >= w1 - w0) return;
  const int slot = w0 + (int)i;
  const unsigned r = (unsigned)slot % a.cap;
  const int s = a.born[r];
  if (s < 0) return;
  int n = f - s;  // the entries the track has
  float2 q;
  bool live = fb_track_step<FB>(a.pos[r], f - 1, a.g.W, a.g.H, a.alpha, a.beta, taps, q);
  if (live) {
    __builtin_nontemporal_store((u2v){__float_as_uint(q.x), __float_as_uint(q.y)}, a.tracks + (size_t)n * a.max_tracks + slot);
    ++n;
    live = n <= a.lmax && f < a.npairs;  // complete, or the clip is over
  }
  if (live) {
    a.pos[r] = q;
    a.occ[a.g.cell_of(q.x, q.y)] = f + 1;
    return;
  }
  a.born[r] = -1;
  for (int j = n; j <= a.lmax; ++j)
    __builtin_nontemporal_store((u2v){kDenseEnded, kDenseEnded}, a.tracks + (size_t)j * a.max_tracks + slot);
  if (a.len) a.len[slot] = n;
}

template <bool FB>
__global__ __launch_bounds__(kDenseLanes) void dense_advance_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                                    DenseArgs a, int f) {
  const size_t plane = (size_t)a.g.W * a.g.H;
  dense_advance<FB>(a, f, [&](int k, int d) { return FlowTaps{(d ? rev : fw) + k * plane, a.g.W}; });
}
template <bool FB>
__global__ __launch_bounds__(kDenseLanes) void dense_advance_level_kernel(const float2* __restrict__ fw,
                                                                          const float2* __restrict__ rev, UpGeom ug, DenseArgs a,
                                                                          int f) {
  dense_advance<FB>(a, f, [&](int k, int d) { return UpNeighbours{(d ? rev : fw) + k * ug.plane(), ug}; });
}

// does cell c seed in frame f?  (Frame 0 has no live track, and the stamps are whatever the work buffer held.)
__device__ __forceinline__ bool dense_seeds(const DenseArgs& a, int f, int c) {
  return c < a.g.cells() && (f == 0 || a.occ[c] != f + 1) && a.tex[(size_t)f * a.g.cells() + c];
}
// the sum of v over the workgroup's kDenseCells lanes, in every lane
__device__ __forceinline__ int dense_block_sum(int v, int* lds) {
  __syncthreads();  // (lds may still be read from the previous call)
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int k = kDenseCells / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) lds[threadIdx.x] += lds[threadIdx.x + k];
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(kDenseCells) void dense_count_kernel(DenseArgs a, int f) {
  __shared__ int lds[kDenseCells];
  const int c = blockIdx.x * kDenseCells + threadIdx.x;
  const int n = dense_block_sum(dense_seeds(a, f, c), lds);
  if (threadIdx.x == 0) {
    a.cnt[blockIdx.x] = n;
    if (f == 0 && blockIdx.x == 0) a.base[0] = 0;
  }
}

__global__ __launch_bounds__(kDenseCells) void dense_assign_kernel(DenseArgs a, int f) {
  __shared__ int lds[kDenseCells];
  const int c = blockIdx.x * kDenseCells + threadIdx.x;
  const bool seeds = dense_seeds(a, f, c);
  if (f == 0 && c < a.g.cells()) a.occ[c] = 0;  // from here on the stamps are this call's
  // the seeds of the workgroups before this one
  int before = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += kDenseCells) before += a.cnt[k];
  before = dense_block_sum(before, lds);
  // ... and of the lanes before this one: an inclusive scan over the workgroup
  __syncthreads();
  lds[threadIdx.x] = seeds;
  __syncthreads();
  for (int k = 1; k < kDenseCells; k <<= 1) {
    const int v = (int)threadIdx.x >= k ? lds[threadIdx.x - k] : 0;
    __syncthreads();
    lds[threadIdx.x] += v;
    __syncthreads();
  }
  const int rank = lds[threadIdx.x] - seeds, mine = lds[kDenseCells - 1];
  const long long taken = a.base[f];
  const long long slot = taken + before + rank;
  if (seeds && slot < a.max_tracks) {  // (else: dropped)
    const int off = a.g.stride / 2;
    const float2 p = make_float2((float)(off + (c % a.g.ncx) * a.g.stride), (float)(off + (c / a.g.ncx) * a.g.stride));
    __builtin_nontemporal_store((u2v){__float_as_uint(p.x), __float_as_uint(p.y)}, a.tracks + slot);
    a.start[slot] = f;
    const unsigned r = (unsigned)slot % a.cap;
    a.pos[r] = p;
    a.born[r] = f;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {  // the one writer of base[f + 1], which nobody reads in this launch
    const long long all = taken + before + mine, kept = min(all, (long long)a.max_tracks);
    const long long dropped = (f ? *a.dropped : 0) + (all - kept);
    a.base[f + 1] = (int)kept;
    *a.dropped = dropped;
    if (f == a.npairs - 1) {
      a.info[0] = kept;
      a.info[1] = dropped;
    }
  }
}

static DenseArgs dense_args(const DenseGrid& g, int npairs, int max_len, float alpha, float beta, int max_tracks, float* tracks,
                            int* start, int* len, long long* info, void* work) {
  DenseArgs a;
  a.g = g;
  a.npairs = npairs;
  a.lmax = max_len ? std::min(max_len, npairs) : npairs;
  a.max_tracks = max_tracks;
  a.cap = (unsigned)dense_cap(a.lmax, g.cells(), max_tracks);
  a.alpha = alpha;
  a.beta = beta;
  a.tracks = (u2v*)tracks;
  a.start = start;
  a.len = len;
  a.info = info;
  const DenseLayout l = dense_layout(npairs, g.cells(), a.cap);
  char* w = (char*)work;
  a.base = (int*)(w + l.base);
  a.dropped = (long long*)(w + l.dropped);
  a.occ = (int*)(w + l.occ);
  a.cnt = (int*)(w + l.cnt);
  a.tex = (const uint8_t*)(w + l.tex);
  a.pos = (float2*)(w + l.pos);
  a.born = (int*)(w + l.born);
  return a;
}

// the frame loop; `advance(a, f, grid)` launches the advance kernel of frame f
template <class Advance>
static hipError_t dense_frames(const uint8_t* frames, int noc, int window, int min_eig, const DenseArgs& a, Advance advance,
                               hipStream_t s) {
  const int cells = a.g.cells();
  if (hipError_t e = launch_texture(frames, a.npairs, a.g, noc, window, min_eig, const_cast<uint8_t*>(a.tex), s)) return e;
  const dim3 cell_grid((unsigned)((cells + kDenseCells - 1) / kDenseCells));
  for (int f = 0; f <= a.npairs; ++f) {
    if (f >= 1) {
      const long long window_slots = std::min((long long)std::min(a.lmax, f) * cells, (long long)a.max_tracks);
      advance(a, f, dim3((unsigned)((window_slots + kDenseLanes - 1) / kDenseLanes)));
    }
    if (f < a.npairs) {
      hipLaunchKernelGGL(dense_count_kernel, cell_grid, dim3(kDenseCells), 0, s, a, f);
      hipLaunchKernelGGL(dense_assign_kernel, cell_grid, dim3(kDenseCells), 0, s, a, f);
    }
  }
  return hipGetLastError();
}

int dense_tracks_cells(int w, int h, int stride, int* ncx, int* ncy) {
  const DenseGrid g = dense_grid(w, h, stride);
  if (ncx) *ncx = g.ncx;
  if (ncy) *ncy = g.ncy;
  return g.cells();
}

size_t dense_tracks_work_bytes(int npairs, int w, int h, int stride, int max_len, int max_tracks) {
  const int cells = dense_grid(w, h, stride).cells();
  const int lmax = max_len ? std::min(max_len, npairs) : npairs;
  return dense_layout(npairs, cells, dense_cap(lmax, cells, max_tracks)).bytes;
}

hipError_t launch_seed_texture(const uint8_t* frames, int nframes, int w, int h, int noc, int stride, int window, int min_eig,
                               uint8_t* out, hipStream_t s) {
  return launch_texture(frames, nframes, dense_grid(w, h, stride), noc, window, min_eig, out, s);
}

hipError_t launch_dense_tracks(const uint8_t* frames, const float* fw, const float* rev, int npairs, int w, int h, int noc,
                               int stride, int window, int min_eig, int max_len, float alpha, float beta, int max_tracks,
                               float* tracks, int* start, int* len, long long* info, void* work, hipStream_t s) {
  const DenseArgs a = dense_args(dense_grid(w, h, stride), npairs, max_len, alpha, beta, max_tracks, tracks, start, len, info, work);
  return dense_frames(frames, noc, window, min_eig, a, [&](const DenseArgs& d, int f, dim3 grid) {
    if (rev)
      hipLaunchKernelGGL(dense_advance_kernel<true>, grid, dim3(kDenseLanes), 0, s, (const float2*)fw, (const float2*)rev, d, f);
    else
      hipLaunchKernelGGL(dense_advance_kernel<false>, grid, dim3(kDenseLanes), 0, s, (const float2*)fw, (const float2*)nullptr, d, f);
  }, s);
}

hipError_t launch_dense_tracks_level(const uint8_t* frames, const float* fw, const float* rev, int npairs, UpGeom g, int noc,
                                     int stride, int window, int min_eig, int max_len, float alpha, float beta, int max_tracks,
                                     float* tracks, int* start, int* len, long long* info, void* work, hipStream_t s) {
  const DenseArgs a = dense_args(dense_grid(g.wo, g.ho, stride), npairs, max_len, alpha, beta, max_tracks, tracks, start, len, info,
                                 work);
  return dense_frames(frames, noc, window, min_eig, a, [&](const DenseArgs& d, int f, dim3 grid) {
    if (rev)
      hipLaunchKernelGGL(dense_advance_level_kernel<true>, grid, dim3(kDenseLanes), 0, s, (const float2*)fw, (const float2*)rev, g,
                         d, f);
    else
      hipLaunchKernelGGL(dense_advance_level_kernel<false>, grid, dim3(kDenseLanes), 0, s, (const float2*)fw,
                         (const float2*)nullptr, g, d, f);
  }, s);
}

}  // namespace ofdis
