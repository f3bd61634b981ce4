// ofdis_segment_tracks.hip -- object tracks (include/ofdis.h: ofdis_segment_overlap, _link, _chain, _relabel, _tracks): the
// segments of consecutive maps of a clip (ofdis_segments.hip) associated through the forward flow, linked by mutual best
// match, chained into numbered tracks with one record of integer sums each, and the maps relabelled by track.
//
// Everything is an integer; the one floating-point step is xt = x + (int)rintf(u).  Integer adds, minima and maxima are
// associative and commutative, so every output is a pure function of the inputs whatever the order of the atomics.  Compiled
// under the exact contract only, like ofdis_segments.hip.
//
// Five launches on the stream, no host synchronisation, no workgroup ever waits for another:
//   clear    overlap[k][i][j] = 0 for i < n_k, j < n_{k+1}: a wavefront per row, plain stores.
//   overlap  the per-pixel pass.  A wavefront takes 64 consecutive pixels of a row of map k (a chunk, as in ofdis_segments.hip);
//            a lane whose value a is recorded follows its flow to (xt, yt) of map k + 1 and, where the value b there is
//            recorded, holds the key (a - 1) * S + (b - 1).  Per distinct key among the lanes ONE lane adds the popcount of the
//            key's ballot.  Two routes, same bits (the choice: st_lds_route, below):
//              global  the add is an integer atomicAdd on overlap itself; any S.
//              lds     S <= kStLdsMaxSegments: a workgroup owns a band of kStBandRows rows of one pair and adds into an S x S
//                      histogram in dynamic LDS (S * S * 4 <= 64 KiB); at the end of the band its non-zero entries go to
//                      overlap with one atomicAdd each.
//   link     one workgroup per pair: the arg-maximum of every row (a wavefront per row, ties to the smallest b) and of every
//            column (a lane per column, ties to the smallest a) in LDS, then one lane per a applies the four conditions.
//   chain    ONE workgroup walks the maps in order: the predecessor of every segment of map k from link[k - 1] (an LDS
//            atomicMin: the smallest a, which is the only one for the injective links of the link step), a prefix sum over the
//            born segments in the order of s, ids, and the track records.  A track is extended by at most one segment per map
//            (link[k - 1][a - 1] is ONE value), so its record has one writer per map and the barrier between two maps orders them.
//            The ids and lengths of the previous map stay in LDS.
//   relabel  every pixel takes the id of its segment, a chunk per wavefront.
//
// The grid of the per-pixel kernels (overlap, relabel) and of clear is capped by a number of workgroups of its own,
// kStGridBlocks = kStBlocksPerCu workgroups for each of the kStCus compute units of the MI355X (of_dis_amd/capi.py mirrors it as
// SEGTRACK_GRID_BLOCKS, so that a test at small frames can count the maps that reach the second trip); the lds route holds
// 64 KiB per workgroup at S = 128, of which a compute unit's 160 KiB take two: kStLdsGridBlocks.
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kStLanes = 256;            // a workgroup: four wavefronts
constexpr int kStCus = 256;              // compute units of the MI355X
constexpr int kStBlocksPerCu = 8;        // workgroups per compute unit of a grid-stride launch: 32 wavefronts, a full CU
constexpr int kStGridBlocks = kStCus * kStBlocksPerCu;       // SEGTRACK_GRID_BLOCKS
constexpr int kStLdsLanes = 1024;        // a workgroup of the lds route: sixteen wavefronts
constexpr int kStLdsBlocksPerCu = 2;     // 160 KiB / 64 KiB, and 2 x 16 wavefronts fill a CU
constexpr int kStLdsGridBlocks = kStCus * kStLdsBlocksPerCu; // SEGTRACK_LDS_GRID_BLOCKS
constexpr int kStLdsMaxSegments = 128;   // SEGTRACK_LDS_MAX_SEGMENTS: S * S * 4 <= 64 KiB
constexpr int kStBandRows = 32;          // SEGTRACK_BAND_ROWS: rows of a pair one workgroup of the lds route owns at a time
constexpr int kStMaxSegments = 1024;     // SEGTRACK_MAX_SEGMENTS
constexpr int kStRecord = 12;            // int64 fields of a segment record and of a track record
constexpr float kStMaxFlow = 4096.0f;    // OFDIS_GM_MAX_FLOW
constexpr long long kStMaxArea = 1ll << 26;
static_assert(kStLdsMaxSegments * kStLdsMaxSegments * 4 <= 64 * 1024, "the histogram of the lds route fits 64 KiB");
static_assert(kStLdsBlocksPerCu * kStLdsMaxSegments * kStLdsMaxSegments * 4 <= 160 * 1024, "and a CU holds kStLdsBlocksPerCu of them");

// the choice of the overlap route, stated once
static bool st_lds_route(int max_segments) { return max_segments <= kStLdsMaxSegments; }
static unsigned st_grid(long long workgroups, int cap) {
  return (unsigned)(workgroups < 1 ? 1 : workgroups > cap ? cap : workgroups);
}

struct StGeom {
  int w, h, n;      // n = w * h < 2^26
  int cpr;          // chunks per row
  int bands;        // bands of kStBandRows rows per map
  int S;            // max_segments
};
static StGeom st_geom(int w, int h, int max_segments) {
  StGeom g;
  g.w = w, g.h = h, g.n = w * h, g.cpr = (w + 63) / 64, g.bands = (h + kStBandRows - 1) / kStBandRows, g.S = max_segments;
  return g;
}

// n_k = min(max(info[k][2], 0), S): the recorded segments of map k
__device__ __forceinline__ int st_count(const long long* __restrict__ info, int k, int S) {
  const long long v = info[(size_t)k * 4 + 2];
  return v < 0 ? 0 : v > S ? S : (int)v;
}

// ------------------------------------------------------------------------------------ clear
__global__ __launch_bounds__(kStLanes) void strk_clear_kernel(const long long* __restrict__ info, int npairs, int S,
                                                              int* __restrict__ overlap) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)npairs * S;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * 4) {
    const int k = (int)(r / S), i = (int)(r - (long long)k * S);
    if (i >= st_count(info, k, S)) continue;
    const int n1 = st_count(info, k + 1, S);
    int* row = overlap + (size_t)r * S;
    for (int j = lane; j < n1; j += 64) row[j] = 0;
  }
}

// ------------------------------------------------------------------------------------ overlap
// the key of the pixel (x, y) of map k, or -1.  n0, n1: the recorded segments of maps k and k + 1
__device__ __forceinline__ int st_key(const int* __restrict__ seg0, const int* __restrict__ seg1, const float2* __restrict__ flow,
                                      const StGeom& g, int x, int y, int n0, int n1) {
  if (x >= g.w) return -1;
  const size_t o = (size_t)y * g.w + x;
  const int a = seg0[o];
  if (a < 1 || a > n0) return -1;
  const float2 uv = flow[o];
  if (!(fabsf(uv.x) <= kStMaxFlow && fabsf(uv.y) <= kStMaxFlow)) return -1;   // (a NaN fails)
  const int xt = x + (int)rintf(uv.x), yt = y + (int)rintf(uv.y);
  if ((unsigned)xt >= (unsigned)g.w || (unsigned)yt >= (unsigned)g.h) return -1;
  const int b = seg1[(size_t)yt * g.w + xt];
  if (b < 1 || b > n1) return -1;
  return (a - 1) * g.S + (b - 1);
}
// per distinct key among the wavefront's lanes, one lane adds the number of lanes that hold it
template <class Add>
__device__ __forceinline__ void st_aggregate(int key, int lane, Add add) {
  for (unsigned long long todo = __ballot(key >= 0); todo;) {
    const int l0 = __ffsll((long long)todo) - 1;
    const int k0 = __shfl(key, l0);
    const unsigned long long m = __ballot(key == k0);
    todo &= ~m;
    if (lane == l0) add(k0, __popcll(m));
  }
}

__global__ __launch_bounds__(kStLanes) void strk_overlap_global_kernel(const int* __restrict__ segments, const float2* __restrict__ flow,
                                                                       const long long* __restrict__ info, StGeom g, int npairs,
                                                                       int* overlap) {
  const int lane = threadIdx.x & 63;
  const int per_map = g.h * g.cpr;
  const long long units = (long long)npairs * per_map;
  for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (long long)gridDim.x * 4) {
    const int k = (int)(u / per_map), r = (int)(u - (long long)k * per_map);
    const int y = r / g.cpr, x = (r % g.cpr) * 64 + lane;
    const int n0 = st_count(info, k, g.S), n1 = st_count(info, k + 1, g.S);
    const int* seg0 = segments + (size_t)k * g.n;
    const int key = st_key(seg0, seg0 + g.n, flow + (size_t)k * g.n, g, x, y, n0, n1);
    int* ov = overlap + (size_t)k * g.S * g.S;
    st_aggregate(key, lane, [&](int k0, int cnt) { atomicAdd(ov + k0, cnt); });
  }
}

// (kStLdsLanes lanes: the histogram allows two workgroups on a compute unit, which sixteen wavefronts each fill.  Only the n0 x n1
// cells a pair can touch are cleared and flushed, in the layout [i][j] at i * S + j of overlap itself.)
__global__ __launch_bounds__(kStLdsLanes) void strk_overlap_lds_kernel(const int* __restrict__ segments, const float2* __restrict__ flow,
                                                                       const long long* __restrict__ info, StGeom g, int npairs,
                                                                       int* overlap) {
  extern __shared__ int st_hist[];   // [S][S]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long units = (long long)npairs * g.bands;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const int k = (int)(u / g.bands), y0 = (int)(u - (long long)k * g.bands) * kStBandRows;
    const int rows = g.h - y0 < kStBandRows ? g.h - y0 : kStBandRows;
    const int n0 = st_count(info, k, g.S), n1 = st_count(info, k + 1, g.S);
    const int cells = n0 * n1;
    for (int e = threadIdx.x; e < cells; e += kStLdsLanes) st_hist[(e / n1) * g.S + e % n1] = 0;
    __syncthreads();
    const int* seg0 = segments + (size_t)k * g.n;
    for (int c = wave; c < rows * g.cpr; c += kStLdsLanes / 64) {
      const int y = y0 + c / g.cpr, x = (c % g.cpr) * 64 + lane;
      const int key = st_key(seg0, seg0 + g.n, flow + (size_t)k * g.n, g, x, y, n0, n1);
      st_aggregate(key, lane, [&](int k0, int cnt) { atomicAdd(st_hist + k0, cnt); });
    }
    __syncthreads();
    int* ov = overlap + (size_t)k * g.S * g.S;
    for (int e = threadIdx.x; e < cells; e += kStLdsLanes) {
      const int at = (e / n1) * g.S + e % n1;
      const int v = st_hist[at];
      if (v) atomicAdd(ov + at, v);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ link
__device__ __forceinline__ long long st_area(const long long* __restrict__ records, size_t slot) {
  const long long a = records[slot * kStRecord];
  return a < 0 ? 0 : a > kStMaxArea ? kStMaxArea : a;
}

__global__ __launch_bounds__(kStLanes) void strk_link_kernel(const int* __restrict__ overlap, const long long* __restrict__ records,
                                                             const long long* __restrict__ info, int npairs, int S, int min_share,
                                                             int* __restrict__ link) {
  __shared__ int fbest[kStMaxSegments], fcount[kStMaxSegments], bbest[kStMaxSegments];   // b (1-based) or 0, c(a, b), a or 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = blockIdx.x; k < npairs; k += gridDim.x) {
    const int n0 = st_count(info, k, S), n1 = st_count(info, k + 1, S);
    const int* ov = overlap + (size_t)k * S * S;
    for (int a = wave; a < n0; a += 4) {   // rows: the largest count, among equals the smallest b
      int c = 0, b = 0;
      for (int j = lane; j < n1; j += 64) {
        const int v = ov[(size_t)a * S + j];
        if (v > c) c = v, b = j + 1;
      }
      for (int d = 1; d < 64; d <<= 1) {
        const int oc = __shfl_xor(c, d), ob = __shfl_xor(b, d);
        if (oc > c || (oc == c && ob < b)) c = oc, b = ob;   // (c == 0 on both sides: b == 0 on both)
      }
      if (lane == 0) fbest[a] = b, fcount[a] = c;
    }
    for (int j = threadIdx.x; j < n1; j += kStLanes) {   // columns: the smallest a of the largest count
      int c = 0, a = 0;
      for (int i = 0; i < n0; ++i) {
        const int v = ov[(size_t)i * S + j];
        if (v > c) c = v, a = i + 1;
      }
      bbest[j] = a;
    }
    __syncthreads();
    for (int a = threadIdx.x; a < n0; a += kStLanes) {
      const int b = fbest[a];
      int out = 0;
      if (b && bbest[b - 1] == a + 1) {
        const long long a0 = st_area(records, (size_t)k * S + a), a1 = st_area(records, (size_t)(k + 1) * S + (b - 1));
        if ((long long)fcount[a] * 100 >= (long long)min_share * (a0 < a1 ? a0 : a1)) out = b;
      }
      link[(size_t)k * S + a] = out;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ chain
__global__ __launch_bounds__(kStLanes) void strk_chain_kernel(const int* __restrict__ link, const long long* __restrict__ records,
                                                              const long long* __restrict__ info, int nmaps, int S, int max_tracks,
                                                              int* __restrict__ ids, long long* tracks, long long* __restrict__ tinfo) {
  typedef unsigned long long u64;
  constexpr int kNone = 0x7FFFFFFF;
  __shared__ int pred[kStMaxSegments];           // the predecessor's slot in map k - 1, or kNone
  __shared__ int id_of[2][kStMaxSegments], len_of[2][kStMaxSegments];   // of maps k and k - 1, by k & 1
  __shared__ int wsum[4];
  __shared__ int part[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ntracks = 0;              // the same in every lane: below 2^26
  int links = 0, longest = 0;   // this lane's share
  int n_prev = 0;
  for (int k = 0; k < nmaps; ++k) {
    const int n = st_count(info, k, S);
    int *idc = id_of[k & 1], *lenc = len_of[k & 1];
    const int *idp = id_of[(k & 1) ^ 1], *lenp = len_of[(k & 1) ^ 1];
    for (int s = tid; s < n; s += kStLanes) pred[s] = kNone;
    __syncthreads();
    if (k > 0)
      for (int a = tid; a < n_prev; a += kStLanes) {
        const int b = link[(size_t)(k - 1) * S + a];
        if (b >= 1 && b <= n) atomicMin(pred + (b - 1), a);
      }
    __syncthreads();
    for (int s0 = 0; s0 < n; s0 += kStLanes) {   // (the same trips in every lane: the barriers are workgroup-wide)
      const int s = s0 + tid;
      const bool in = s < n;
      const int p = in ? pred[s] : 0;
      const bool born = in && p == kNone;
      const u64 bm = __ballot(born);
      if (lane == 0) wsum[wave] = __popcll(bm);
      __syncthreads();
      int before = 0, total = 0;
      for (int v = 0; v < 4; ++v) {
        if (v < wave) before += wsum[v];
        total += wsum[v];
      }
      if (in) {
        const long long* r = records + ((size_t)k * S + s) * kStRecord;
        const long long area = r[0];
        int id, len;
        if (born) {
          id = ntracks + before + __popcll(bm & ((1ull << lane) - 1ull)) + 1, len = 1;
          if (id <= max_tracks) {
            long long* t = tracks + (size_t)(id - 1) * kStRecord;
            t[0] = k, t[1] = s + 1, t[2] = 1, t[3] = s + 1, t[4] = area, t[5] = r[6], t[6] = r[7], t[7] = r[8], t[8] = r[9];
            t[9] = r[10], t[10] = area, t[11] = area;
          }
        } else {
          id = idp[p], len = lenp[p] + 1, ++links;
          if (id <= max_tracks) {   // this track's only writer in map k; the barriers since map k - 1 order the two
            long long* t = tracks + (size_t)(id - 1) * kStRecord;
            t[2] = len, t[3] = s + 1;
            t[4] = (long long)((u64)t[4] + (u64)area);   // two's complement: garbage records wrap
            t[5] = (long long)((u64)t[5] + (u64)r[6]), t[6] = (long long)((u64)t[6] + (u64)r[7]);
            t[7] = (long long)((u64)t[7] + (u64)r[8]), t[8] = (long long)((u64)t[8] + (u64)r[9]);
            t[9] = (long long)((u64)t[9] + (u64)r[10]);
            if (area < t[10]) t[10] = area;
            if (area > t[11]) t[11] = area;
          }
        }
        idc[s] = id, lenc[s] = len;
        ids[(size_t)k * S + s] = id;
        if (len > longest) longest = len;
      }
      ntracks += total;
      __syncthreads();
    }
    n_prev = n;
  }
  for (int d = 1; d < 64; d <<= 1) {
    links += __shfl_xor(links, d);
    const int o = __shfl_xor(longest, d);
    if (o > longest) longest = o;
  }
  if (lane == 0) part[wave][0] = links, part[wave][1] = longest;
  __syncthreads();
  if (tid == 0) {
    int l = 0, m = 0;
    for (int v = 0; v < 4; ++v) {
      l += part[v][0];
      if (part[v][1] > m) m = part[v][1];
    }
    tinfo[0] = ntracks, tinfo[1] = ntracks < max_tracks ? ntracks : max_tracks, tinfo[2] = l, tinfo[3] = m;
  }
}

// ------------------------------------------------------------------------------------ relabel
__global__ __launch_bounds__(kStLanes) void strk_relabel_kernel(const int* __restrict__ segments, const int* __restrict__ ids,
                                                                const long long* __restrict__ info, StGeom g, int nmaps,
                                                                int* __restrict__ track_map) {
  const int lane = threadIdx.x & 63;
  const int per_map = g.h * g.cpr;
  const long long units = (long long)nmaps * per_map;
  for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (long long)gridDim.x * 4) {
    const int k = (int)(u / per_map), r = (int)(u - (long long)k * per_map);
    const int y = r / g.cpr, x = (r % g.cpr) * 64 + lane;
    if (x >= g.w) continue;
    const int n = st_count(info, k, g.S);
    const size_t o = (size_t)k * g.n + (size_t)y * g.w + x;
    const int s = segments[o];
    track_map[o] = s >= 1 && s <= n ? ids[(size_t)k * g.S + (s - 1)] : 0;
  }
}

// ------------------------------------------------------------------------------------ the launchers
size_t segment_tracks_work_bytes(int nmaps, int max_segments) {
  const size_t b = (size_t)(nmaps - 1) * max_segments * ((size_t)max_segments + 1) * 4;
  return b ? (b + 7) / 8 * 8 : 8;
}

hipError_t launch_segment_overlap(const int* segments, const float* flow, const long long* info, int nmaps, int w, int h,
                                  int max_segments, int* overlap, hipStream_t s) {
  const int npairs = nmaps - 1;
  if (npairs < 1) return hipSuccess;
  const StGeom g = st_geom(w, h, max_segments);
  strk_clear_kernel<<<st_grid(((long long)npairs * max_segments + 3) / 4, kStGridBlocks), kStLanes, 0, s>>>(info, npairs, max_segments,
                                                                                                           overlap);
  if (st_lds_route(max_segments))
    strk_overlap_lds_kernel<<<st_grid((long long)npairs * g.bands, kStLdsGridBlocks), kStLdsLanes,
                              (size_t)max_segments * max_segments * sizeof(int), s>>>(segments, (const float2*)flow, info, g, npairs,
                                                                                      overlap);
  else
    strk_overlap_global_kernel<<<st_grid(((long long)npairs * h * g.cpr + 3) / 4, kStGridBlocks), kStLanes, 0, s>>>(
        segments, (const float2*)flow, info, g, npairs, overlap);
  return hipGetLastError();
}

hipError_t launch_segment_link(const int* overlap, const long long* records, const long long* info, int nmaps, int max_segments,
                               int min_share, int* link, hipStream_t s) {
  const int npairs = nmaps - 1;
  if (npairs < 1) return hipSuccess;
  strk_link_kernel<<<st_grid(npairs, kStGridBlocks), kStLanes, 0, s>>>(overlap, records, info, npairs, max_segments, min_share, link);
  return hipGetLastError();
}

hipError_t launch_segment_chain(const int* link, const long long* records, const long long* info, int nmaps, int max_segments,
                                int max_tracks, int* ids, long long* tracks, long long* tinfo, hipStream_t s) {
  strk_chain_kernel<<<1, kStLanes, 0, s>>>(link, records, info, nmaps, max_segments, max_tracks, ids, tracks, tinfo);
  return hipGetLastError();
}

hipError_t launch_segment_relabel(const int* segments, const int* ids, const long long* info, int nmaps, int w, int h,
                                  int max_segments, int* track_map, hipStream_t s) {
  const StGeom g = st_geom(w, h, max_segments);
  strk_relabel_kernel<<<st_grid(((long long)nmaps * h * g.cpr + 3) / 4, kStGridBlocks), kStLanes, 0, s>>>(segments, ids, info, g, nmaps,
                                                                                                         track_map);
  return hipGetLastError();
}

}  // namespace ofdis
