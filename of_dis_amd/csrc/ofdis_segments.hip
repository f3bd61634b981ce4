// ofdis_segments.hip -- segments of a label map (include/ofdis.h: ofdis_label_segments): the connected components of the
// foreground of [nmaps][H][W] byte maps under 4- or 8-connectivity, the small ones removed, the kept ones numbered in the order
// of their smallest raster index, and one record of integer sums per kept segment.
//
// Everything is an integer: the result is a pure function of the inputs whatever the order of the unions and of the atomics
// (min, max and add are associative and commutative, the root of a component is a minimum).  Compiled under the exact contract
// only (-ffp-contract=off): the one floating-point step, qu = (int)rintf(u * 256.0f), is that of ofdis_gmotion.hip.
//
// Mapping.  A wavefront takes 64 consecutive pixels of a row (a CHUNK); __ballot of the foreground predicate is that piece of
// the row as one 64-bit word, and a lane's row run inside the chunk -- its first and last lane -- follows from two bit
// operations on the word.  The pixels of a run are connected by construction, so only a run's first lane (its HEAD) owns an
// entry of the union-find forest that matters; the other lanes point at it and never change.
//
// Seven launches on the stream, no host synchronisation, no workgroup ever waits for another (no flags, no tickets, no spinning):
//   init     parent[p] = the head of p's run (foreground) or -1 (background); area[head] = 0.  Plain stores only.
//   merge    the unions no run gives for free.  With cur / up the words of rows y and y - 1 (one bit from either neighbouring
//            chunk shifted in), a lane unites its pixel with
//              the pixel above        where cur & up            and not both at x - 1   (the first column of an overlap)
//              the pixel up-left      where cur & up(x-1)       and neither up(x) nor cur(x-1)          (conn 8)
//              the pixel up-right     where cur & up(x+1)       and neither up(x) nor cur(x+1)          (conn 8)
//              the pixel to the left  at lane 0 where the run continues from the chunk before.
//            The excluded cases are covered by the vertical union one column further.  A union follows the parents of both
//            pixels to their roots and links the larger root below the smaller one with atomicMin.
//   flatten  every head finds its root and stores it as its parent; a wavefront adds, per distinct root among its lanes, the
//            number of its pixels of that root to area[root] (one popcount of a ballot, one atomic).
//   count    per block of 256 raster indices: the roots, the roots with area >= min_area, the foreground pixels -> one record of
//            counts per block, plain stores.
//   scan     one workgroup per map: the exclusive prefix sum of the kept roots over the blocks, in raster order, and info.
//   number   per block again: a kept root's number = the blocks before + its rank in the block + 1, stored in place of its area;
//            the numbers <= max_segments initialise their record: area, root, the root's own x and y as the box, zeros.
//   relabel  every pixel takes the number at its root -> segments; per distinct segment among a wavefront's lanes one lane
//            issues the record's atomics -- the box from the first and last set bit of the segment's ballot, sx from six
//            popcounts, sy and nflow from one -- and per run its head adds squ and sqv (a wavefront prefix sum, two differences).
//
// The forest.  parent is int32 [nmaps][H * W]; an entry only ever DECREASES and only ever holds indices of its own component, so
// every walk follows strictly decreasing indices and ends, and the last root standing is the component's smallest index.
// Cross-XCD visibility: an XCD's L2 does not see another XCD's atomicMin within a launch.  The walks of merge and flatten read
// parents with agent-scope atomic loads; even so a walk may end at an index that has just stopped being a root.  That is
// harmless: the closing atomicMin on the supposed root returns what the entry really held, and when that is not the index
// itself the union goes on from there with a strictly smaller index.  Flatten runs in a launch of its own after every union,
// where the forest no longer changes except for heads being pointed at their own root -- a walk through such a head arrives at
// the same root either way.  The box fields of a record are read plainly before their atomic (a stale value is an earlier,
// looser bound: the atomic is then issued where it was not needed, never skipped where it was).
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kSegLanes = 256;    // a workgroup: four wavefronts (four chunks) or one block of 256 raster indices
constexpr int kSegRecord = 12;    // int64 fields of a record
constexpr float kSegMaxFlow = 4096.0f;  // OFDIS_GM_MAX_FLOW

struct SegGeom {
  int w, h, n;      // n = w * h < 2^26
  int cpr;          // chunks per row
  int nblk;         // blocks of 256 raster indices per map
  int nmaps;
  long long units;  // nmaps * h * cpr chunks
  __host__ __device__ long long blocks() const { return (long long)nmaps * nblk; }
};

__device__ __forceinline__ bool seg_fg(const uint8_t* map, const SegGeom& g, int x, int y, unsigned codes) {
  if ((unsigned)x >= (unsigned)g.w || (unsigned)y >= (unsigned)g.h) return false;
  const unsigned b = map[(size_t)y * g.w + x];
  return b < 8u && ((codes >> b) & 1u);
}
// first and last lane of the run of set bits around `lane` (whose bit is set)
__device__ __forceinline__ int seg_run_start(unsigned long long cur, int lane) {
  const unsigned long long below = ~cur & ((1ull << lane) - 1ull);
  return below ? 64 - __clzll((long long)below) : 0;
}
__device__ __forceinline__ int seg_run_end(unsigned long long cur, int lane) {
  const unsigned long long above = ~cur & ~((2ull << lane) - 1ull);
  return above ? __ffsll((long long)above) - 2 : 63;
}

// a wavefront's chunk: map, row, first column
struct SegChunk {
  int map, y, x0;
};
__device__ __forceinline__ SegChunk seg_chunk(const SegGeom& g, long long u) {
  const int per_map = g.h * g.cpr;
  const int map = (int)(u / per_map), r = (int)(u - (long long)map * per_map);
  return SegChunk{map, r / g.cpr, (r % g.cpr) * 64};
}
#define SEG_FOR_CHUNKS(g, u) \
  for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < (g).units; u += (long long)gridDim.x * 4)

// ------------------------------------------------------------------------------------ init
__global__ __launch_bounds__(kSegLanes) void seg_init_kernel(const uint8_t* __restrict__ label, SegGeom g, unsigned codes,
                                                             int* __restrict__ parent, int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  SEG_FOR_CHUNKS(g, u) {
    const SegChunk c = seg_chunk(g, u);
    const int x = c.x0 + lane;
    const bool f = seg_fg(label + (size_t)c.map * g.n, g, x, c.y, codes);
    const unsigned long long cur = __ballot(f);
    if (x < g.w) {
      const int start = f ? seg_run_start(cur, lane) : lane;
      const size_t o = (size_t)c.map * g.n + (size_t)c.y * g.w + x;
      parent[o] = f ? c.y * g.w + c.x0 + start : -1;
      if (f && start == lane) area[o] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------ merge
__device__ __forceinline__ int seg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int seg_find(const int* parent, int x) {
  for (int p = seg_load(parent + x); p != x; p = seg_load(parent + x)) x = p;   // p < x: strictly decreasing
  return x;
}
__device__ __forceinline__ void seg_union(int* parent, int a, int b) {
  for (;;) {
    a = seg_find(parent, a);
    b = seg_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);   // parent[a] = min(what it held, b)
    if (old == a) return;                       // a was a root and now hangs below b
    a = old;                                    // it was not: old < a is of a's component and b's; go on with the two
  }
}

template <bool CONN8>
__global__ __launch_bounds__(kSegLanes) void seg_merge_kernel(const uint8_t* __restrict__ label, SegGeom g, unsigned codes,
                                                              int* parent) {
  const int lane = threadIdx.x & 63;
  SEG_FOR_CHUNKS(g, u) {
    const SegChunk c = seg_chunk(g, u);
    const uint8_t* map = label + (size_t)c.map * g.n;
    const int x = c.x0 + lane;
    const unsigned long long cur = __ballot(seg_fg(map, g, x, c.y, codes));
    const unsigned long long up = __ballot(seg_fg(map, g, x, c.y - 1, codes));
    // the four pixels beside the chunk: lane 0 left of row y, 1 right of it, 2 left of row y - 1, 3 right of it
    const unsigned long long edge =
        __ballot(lane < 4 && seg_fg(map, g, (lane & 1) ? c.x0 + 64 : c.x0 - 1, c.y - (lane >> 1), codes));
    const unsigned long long cur_l = (cur << 1) | (edge & 1), cur_r = (cur >> 1) | (((edge >> 1) & 1) << 63);
    const unsigned long long up_l = (up << 1) | ((edge >> 2) & 1), up_r = (up >> 1) | (((edge >> 3) & 1) << 63);
    const unsigned long long vert = cur & up & ~(cur_l & up_l);
    const unsigned long long nw = CONN8 ? cur & up_l & ~up & ~cur_l : 0ull;
    const unsigned long long ne = CONN8 ? cur & up_r & ~up & ~cur_r : 0ull;
    const unsigned long long me = 1ull << lane;
    int* pm = parent + (size_t)c.map * g.n;
    const int idx = c.y * g.w + x;
    if (lane == 0 && (cur & cur_l & 1)) seg_union(pm, idx, idx - 1);
    if (vert & me) seg_union(pm, idx, idx - g.w);
    if (nw & me) seg_union(pm, idx, idx - g.w - 1);
    if (ne & me) seg_union(pm, idx, idx - g.w + 1);
  }
}

// ------------------------------------------------------------------------------------ flatten, area
__global__ __launch_bounds__(kSegLanes) void seg_flatten_kernel(const uint8_t* __restrict__ label, SegGeom g, unsigned codes,
                                                                int* parent, int* area) {
  const int lane = threadIdx.x & 63;
  SEG_FOR_CHUNKS(g, u) {
    const SegChunk c = seg_chunk(g, u);
    const int x = c.x0 + lane;
    const bool f = seg_fg(label + (size_t)c.map * g.n, g, x, c.y, codes);
    const unsigned long long cur = __ballot(f);
    const int start = f ? seg_run_start(cur, lane) : lane;
    int* pm = parent + (size_t)c.map * g.n;
    const int idx = c.y * g.w + x;
    int root = -1;
    if (f && start == lane) {
      root = seg_find(pm, idx);
      if (root != idx) pm[idx] = root;
    }
    root = __shfl(root, start);   // (a background lane reads itself: -1)
    for (unsigned long long todo = cur; todo;) {
      const int r0 = __shfl(root, __ffsll((long long)todo) - 1);
      const unsigned long long m = __ballot(f && root == r0);
      todo &= ~m;
      if (lane == 0) atomicAdd(area + (size_t)c.map * g.n + r0, __popcll(m));
    }
  }
}

// ------------------------------------------------------------------------------------ count, scan, number
// per block of 256 raster indices of a map, four int32: roots, kept roots, foreground pixels, then (scan) the kept roots of
// the blocks before
struct SegFlags {
  bool root, kept, fg;
};
__device__ __forceinline__ SegFlags seg_flags(const int* pm, const int* am, int n, int p, int min_area) {
  SegFlags s{false, false, false};
  if (p < n) {
    const int q = pm[p];
    s.fg = q >= 0;
    s.root = q == p;
    s.kept = s.root && am[p] >= min_area;
  }
  return s;
}

__global__ __launch_bounds__(kSegLanes) void seg_count_kernel(SegGeom g, const int* __restrict__ parent, const int* __restrict__ area,
                                                              int min_area, int* __restrict__ counts) {
  __shared__ int part[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = blockIdx.x; b < g.blocks(); b += gridDim.x) {
    const int map = (int)(b / g.nblk), blk = (int)(b % g.nblk);
    const SegFlags s = seg_flags(parent + (size_t)map * g.n, area + (size_t)map * g.n, g.n, blk * kSegLanes + (int)threadIdx.x, min_area);
    const int nr = __popcll(__ballot(s.root)), nk = __popcll(__ballot(s.kept)), nf = __popcll(__ballot(s.fg));
    if (lane == 0) part[wave][0] = nr, part[wave][1] = nk, part[wave][2] = nf;
    __syncthreads();
    if (threadIdx.x < 3)
      counts[b * 4 + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSegLanes) void seg_scan_kernel(SegGeom g, int max_segments, int* counts, long long* __restrict__ info) {
  __shared__ int wsum[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int map = blockIdx.x; map < g.nmaps; map += gridDim.x) {
    int* cm = counts + (size_t)map * g.nblk * 4;
    int carry = 0, roots = 0, fgs = 0;   // (each below 2^26)
    for (int b0 = 0; b0 < g.nblk; b0 += kSegLanes) {
      const int b = b0 + (int)threadIdx.x;
      const int nr = b < g.nblk ? cm[b * 4 + 0] : 0, nk = b < g.nblk ? cm[b * 4 + 1] : 0, nf = b < g.nblk ? cm[b * 4 + 2] : 0;
      int incl = nk, sr = nr, sf = nf;   // inclusive prefix of nk, sums of the other two, over the wavefront
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
        sr += __shfl_xor(sr, d);
        sf += __shfl_xor(sf, d);
      }
      if (lane == 63) wsum[wave][0] = incl, wsum[wave][1] = sr, wsum[wave][2] = sf;
      __syncthreads();
      int before = carry;
      for (int v = 0; v < wave; ++v) before += wsum[v][0];
      if (b < g.nblk) cm[b * 4 + 3] = before + incl - nk;
      carry += wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
      roots += wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
      fgs += wsum[0][2] + wsum[1][2] + wsum[2][2] + wsum[3][2];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      long long* im = info + (size_t)map * 4;
      im[0] = roots, im[1] = carry, im[2] = carry < max_segments ? carry : max_segments, im[3] = fgs;
    }
  }
}

__global__ __launch_bounds__(kSegLanes) void seg_number_kernel(SegGeom g, const int* __restrict__ parent, int* area,
                                                               const int* __restrict__ counts, int min_area, int max_segments,
                                                               long long* __restrict__ records) {
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = blockIdx.x; b < g.blocks(); b += gridDim.x) {
    const int map = (int)(b / g.nblk), blk = (int)(b % g.nblk);
    const int p = blk * kSegLanes + (int)threadIdx.x;
    int* am = area + (size_t)map * g.n;
    const SegFlags s = seg_flags(parent + (size_t)map * g.n, am, g.n, p, min_area);
    const unsigned long long kept = __ballot(s.kept);
    if (lane == 0) part[wave] = __popcll(kept);
    __syncthreads();
    if (s.root) {
      int k = 0;
      if (s.kept) {
        k = counts[b * 4 + 3] + __popcll(kept & ((1ull << lane) - 1ull)) + 1;
        for (int v = 0; v < wave; ++v) k += part[v];
        if (records && k <= max_segments) {
          long long* r = records + ((size_t)map * max_segments + (k - 1)) * kSegRecord;
          const int x = p % g.w, y = p / g.w;
          r[0] = am[p], r[1] = p, r[2] = x, r[3] = y, r[4] = x, r[5] = y;
          for (int i = 6; i < kSegRecord; ++i) r[i] = 0;
        }
      }
      am[p] = k;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ relabel, records
__global__ __launch_bounds__(kSegLanes) void seg_relabel_kernel(const uint8_t* __restrict__ label, const float2* __restrict__ flow,
                                                                SegGeom g, unsigned codes, const int* __restrict__ parent,
                                                                const int* __restrict__ number, int max_segments,
                                                                int* __restrict__ segments, long long* records) {
  typedef unsigned long long u64;
  const int lane = threadIdx.x & 63;
  SEG_FOR_CHUNKS(g, u) {
    const SegChunk c = seg_chunk(g, u);
    const int x = c.x0 + lane;
    const bool f = seg_fg(label + (size_t)c.map * g.n, g, x, c.y, codes);
    const unsigned long long cur = __ballot(f);
    const int start = f ? seg_run_start(cur, lane) : lane;
    const bool head = f && start == lane;
    const size_t o = (size_t)c.map * g.n + (size_t)c.y * g.w + x;
    int k = 0;
    if (head) k = number[(size_t)c.map * g.n + parent[o]];   // a head's parent is its root (flatten)
    k = __shfl(k, start);
    if (segments && x < g.w) segments[o] = k;
    if (!records) continue;
    const bool rec = k >= 1 && k <= max_segments;
    bool usable = false;
    int qu = 0, qv = 0;
    if (flow && rec) {
      const float2 uv = flow[o];
      usable = fabsf(uv.x) <= kSegMaxFlow && fabsf(uv.y) <= kSegMaxFlow;
      if (usable) qu = (int)rintf(uv.x * 256.0f), qv = (int)rintf(uv.y * 256.0f);
    }
    const unsigned long long use = __ballot(usable);
    long long* rm = records + (size_t)c.map * max_segments * kSegRecord;
    for (unsigned long long todo = __ballot(rec); todo;) {
      const int l0 = __ffsll((long long)todo) - 1;
      const int k0 = __shfl(k, l0);
      const unsigned long long m = __ballot(rec && k == k0);
      todo &= ~m;
      if (lane == l0) {
        long long* r = rm + (size_t)(k0 - 1) * kSegRecord;
        const long long xmin = c.x0 + __ffsll((long long)m) - 1, xmax = c.x0 + 63 - __clzll((long long)m);
        const int cnt = __popcll(m);
        if (xmin < r[2]) atomicMin((u64*)(r + 2), (u64)xmin);
        if (xmax > r[4]) atomicMax((u64*)(r + 4), (u64)xmax);
        if (c.y > r[5]) atomicMax((u64*)(r + 5), (u64)c.y);
        // the sum of the set bits' positions, one popcount per bit of a lane number
        const int pos = __popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(m & 0xCCCCCCCCCCCCCCCCull) +
                        4 * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(m & 0xFF00FF00FF00FF00ull) +
                        16 * __popcll(m & 0xFFFF0000FFFF0000ull) + 32 * __popcll(m & 0xFFFFFFFF00000000ull);
        atomicAdd((u64*)(r + 6), (u64)((long long)c.x0 * cnt + pos));
        if (c.y) atomicAdd((u64*)(r + 7), (u64)((long long)c.y * cnt));
        if (m & use) atomicAdd((u64*)(r + 8), (u64)__popcll(m & use));
      }
    }
    if (flow) {   // squ, sqv per run: an inclusive prefix sum over the wavefront (at most 64 * 2^20), then end minus start
      int su = qu, sv = qv;
      for (int d = 1; d < 64; d <<= 1) {
        const int tu = __shfl_up(su, d), tv = __shfl_up(sv, d);
        if (lane >= d) su += tu, sv += tv;
      }
      const int end = f ? seg_run_end(cur, lane) : lane;
      const int ru = __shfl(su, end) - su + qu, rv = __shfl(sv, end) - sv + qv;
      if (head && rec) {
        long long* r = rm + (size_t)(k - 1) * kSegRecord;
        if (ru) atomicAdd((u64*)(r + 9), (u64)(long long)ru);
        if (rv) atomicAdd((u64*)(r + 10), (u64)(long long)rv);
      }
    }
  }
}

// ------------------------------------------------------------------------------------ the launcher
static SegGeom seg_geom(int nmaps, int w, int h) {
  SegGeom g;
  g.w = w, g.h = h, g.n = w * h, g.cpr = (w + 63) / 64, g.nblk = (g.n + kSegLanes - 1) / kSegLanes, g.nmaps = nmaps;
  g.units = (long long)nmaps * h * g.cpr;
  return g;
}

// parent and area (later: number), int32 [nmaps][h * w] each, then the counts, int32 [nmaps][ceil(h * w / 256)][4]
size_t segments_work_bytes(int nmaps, int w, int h) {
  const SegGeom g = seg_geom(nmaps, w, h);
  return (size_t)nmaps * (8 * (size_t)g.n + 16 * (size_t)g.nblk);
}

hipError_t launch_label_segments(const uint8_t* label, const float* flow, int nmaps, int w, int h, unsigned codes, int conn,
                                 int min_area, int max_segments, int* segments, long long* records, long long* info, void* work,
                                 hipStream_t s) {
  const SegGeom g = seg_geom(nmaps, w, h);
  int* parent = (int*)work;
  int* area = parent + (size_t)nmaps * g.n;
  int* counts = area + (size_t)nmaps * g.n;
  if (min_area < 1) min_area = 1;
  const dim3 chunks(grid_for(g.units * 64)), blocks(grid_for(g.blocks() * kSegLanes)), maps(grid_for((long long)nmaps * kSegLanes));
  seg_init_kernel<<<chunks, kSegLanes, 0, s>>>(label, g, codes, parent, area);
  if (conn == 8) seg_merge_kernel<true><<<chunks, kSegLanes, 0, s>>>(label, g, codes, parent);
  else seg_merge_kernel<false><<<chunks, kSegLanes, 0, s>>>(label, g, codes, parent);
  seg_flatten_kernel<<<chunks, kSegLanes, 0, s>>>(label, g, codes, parent, area);
  seg_count_kernel<<<blocks, kSegLanes, 0, s>>>(g, parent, area, min_area, counts);
  seg_scan_kernel<<<maps, kSegLanes, 0, s>>>(g, max_segments, counts, info);
  seg_number_kernel<<<blocks, kSegLanes, 0, s>>>(g, parent, area, counts, min_area, max_segments, records);
  seg_relabel_kernel<<<chunks, kSegLanes, 0, s>>>(label, (const float2*)flow, g, codes, parent, area, max_segments, segments, records);
  return hipGetLastError();
}

}  // namespace ofdis
