// ofdis_kmeans.hip -- k-means training of the bag-of-features codebook (include/ofdis.h: ofdis_codebook_seed,
// ofdis_codebook_update, ofdis_codebook_train): Lloyd's algorithm on the 8-bit descriptors of ofdis_descriptor_normalize, four
// independent clusterings (one per channel) in one pass.  The assignment is ofdis_bof.hip's kernel through its launcher; new here
// are the seeding and the centre update: per channel and word the mean of the member rows, rounded half up.
//
// Everything is integer arithmetic: a sum of bytes is exact in uint32 whatever order it is taken in, so the bits depend neither
// on the mapping below, nor on the order the atomics of the count arrive in, nor on the arithmetic contract; compiled once.
//
// The update buckets, then sums (desc is read once, by the sum alone):
//   clear    counts [4][nwords] and the stats row of this iteration := 0
//   count    per slot and channel: rank = counts[c][word]++ (a returning atomic: the member's place inside its word, arbitrary
//            and not part of any result), ~0 for a slot that belongs to no word; with stats, the members whose word changed and
//            the sum of their distances, reduced per workgroup, then one 64-bit atomic each; prev := words
//   scan     one workgroup per channel: off[c][k] = the exclusive sum of counts[c], off[c][nwords] = the members with a word
//   scatter  order[c][off[c][word] + rank] = slot: every word's members in one segment
//   sum      a wavefront per chunk of kKmChunk = 256 positions of order[c]: the runs of one word inside the chunk in turn, the
//            lanes split over the dwords of the channel's segment of a row (EL lanes) and over 64 / EL members at a time; two
//            16-bit sums per register (256 x 255 < 2^16).  A run that is its word's whole segment is divided and stored as
//            bytes; a run that is a part of a longer segment -- at most one at the head and one at the tail of a chunk -- goes
//            to the chunk's slab row with plain stores
//   finish   a workgroup per (channel, word): a segment that spans several chunks is summed from their slab rows, the threads
//            split over entries and chunks, then divided and stored.  A word that owns everything is 1/256 of the rows again
// Nothing synchronises with the host; every kernel is sized by max_tracks and reads ntracks from info.
//
// The work buffer (kmeans_layout; M = max_tracks, K = nwords, every section a multiple of 8 bytes):
//   prev  int32 [M][4]   the words of the iteration before (train with stats)
//   dist  int32 [M][4]   the distances of the assignment (train with stats)
//   rank  uint32 [M][4]
//   off   uint32 [4][K + 1]
//   order uint32 [4][M]
//   slab  uint32 [4][ceil(M / 256)][2][RL]   head and tail sums of every chunk, RL = the padded entries of the longest channel
#include "../../include/ofdis.h"
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kKmThreads = 256;
constexpr int kKmChunk = 256;          // positions of order[c] per wavefront of the sum: 256 x 255 fits 16 bits
constexpr int kKmCountBlocks = 1024;   // the count's grid at most: a workgroup adds its stats with 8 atomics
constexpr unsigned kKmNoRank = 0xffffffffu;
typedef unsigned km_u32_any __attribute__((aligned(1)));   // a dword of a row: rows of 33 C bytes are not aligned
typedef unsigned long long km_u64;

__device__ __forceinline__ int km_ch_off(int c, int C) { return c == 0 ? 0 : c == 1 ? 8 * C : c == 2 ? 17 * C : 25 * C; }
__device__ __forceinline__ int km_ch_len(int c, int C) { return c == 1 ? 9 * C : 8 * C; }
__device__ __forceinline__ km_u64 km_xor_u64(km_u64 v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((km_u64)hi << 32) | lo;
}

// how the lanes of the sum are split (KmGeom, ofdis_kernels.h): NP passes of EL lanes over the dwords of a channel (at most
// ceil(9 C / 4))
KmGeom km_geom(int C) {
  const int nd = (9 * C + 3) / 4;
  KmGeom g;
  g.np = nd <= 64 ? 1 : 5;  // (nd <= 288)
  g.log2el = 2;
  while ((1 << g.log2el) < nd && g.log2el < 6) ++g.log2el;
  g.el = 1 << g.log2el;
  g.rl = 4 * g.el * g.np;
  return g;
}

struct KmLayout {
  size_t prev, dist, rank, off, order, slab, bytes;
};
static KmLayout kmeans_layout(int max_tracks, int C, int nwords) {
  const size_t M = (size_t)max_tracks, K = (size_t)nwords, nch = (M + kKmChunk - 1) / kKmChunk;
  const auto up8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
  KmLayout l;
  l.prev = 0;
  l.dist = l.prev + 16 * M;
  l.rank = l.dist + 16 * M;
  l.off = l.rank + 16 * M;
  l.order = l.off + up8(16 * (K + 1));
  l.slab = l.order + 16 * M;
  l.bytes = l.slab + 4 * nch * 2 * (size_t)km_geom(C).rl * 4;
  return l;
}

size_t codebook_train_work_bytes(int max_tracks, int nxy, int nt, int nwords) {
  return kmeans_layout(max_tracks, nxy * nxy * nt, nwords).bytes;
}

struct KmArgs {
  const uint8_t* desc;  // [max_tracks][D]
  const int* words;     // [max_tracks][4]
  const int* len;       // [max_tracks] or null: every slot a member
  const long long* info;
  int max_tracks, C, nwords, min_len, first;  // first: iteration 0, every member counts as changed
  uint8_t* codebook;                          // [nwords][D]
  unsigned* counts;                           // [4][nwords]
  long long* stats;                           // [4][2] of this iteration or null
  int* prev;                                  // the work buffer's sections
  const int* dist;
  unsigned *rank, *off, *order, *slab;
  int el, log2el, rl, nch;
};

// ------------------------------------------------------------------------------------ ofdis_codebook_seed
// one wavefront per word: the first member at or after s_k, 64 slots per step, then its row byte by byte
__global__ __launch_bounds__(64) void km_seed_kernel(const uint8_t* desc, const int* len, const long long* info, int max_tracks,
                                                     int D, int nwords, int min_len, uint8_t* codebook) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const long long n = min(info[0], (long long)max_tracks);
  uint8_t* row = codebook + (size_t)k * D;
  long long src = -1;
  if (n > 0) {
    const long long s = (long long)(2 * k + 1) * n / (2 * nwords);  // (< 2^15 2^24)
    if (!len) src = s;
    for (long long t = 0; t < n && src < 0; t += 64) {
      long long i = s + t + lane;
      i -= i >= n ? n : 0;
      const bool member = t + lane < n && len[i] >= min_len;  // (t + lane < n: i < n, and no slot is looked at twice)
      const km_u64 m = __ballot(member);
      if (m) src = s + t + (__ffsll((long long)m) - 1);
    }
    if (src >= n) src -= n;
  }
  for (int e = lane; e < D; e += 64) row[e] = src >= 0 ? desc[(size_t)src * D + e] : (uint8_t)0;
}

// ------------------------------------------------------------------------------------ ofdis_codebook_update
__global__ __launch_bounds__(kKmThreads) void km_clear_kernel(unsigned* counts, int n, long long* stats) {
  const int i = blockIdx.x * kKmThreads + threadIdx.x;
  if (i < n) counts[i] = 0;
  if (stats && i < 8) stats[i] = 0;
}

template <bool STATS>
__global__ __launch_bounds__(kKmThreads) void km_count_kernel(KmArgs a) {
  __shared__ km_u64 red[kKmThreads / 64][8];
  const int tid = threadIdx.x;
  const long long n = min(a.info[0], (long long)a.max_tracks);
  km_u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // per channel: the changes, the distances
  for (long long i = (long long)blockIdx.x * kKmThreads + tid; i < n; i += (long long)gridDim.x * kKmThreads) {
    const bool member = !a.len || a.len[i] >= a.min_len;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t at = (size_t)i * 4 + c;
      const int w = a.words[at];
      const bool in = member && (unsigned)w < (unsigned)a.nwords;  // (a word outside the codebook: the slot belongs to none)
      a.rank[at] = in ? atomicAdd(a.counts + (size_t)c * a.nwords + w, 1u) : kKmNoRank;
      if (STATS) {
        const int before = a.prev[at];
        a.prev[at] = w;
        acc[2 * c] += member && (a.first || before != w) ? 1 : 0;
        acc[2 * c + 1] += member ? (km_u64)(long long)a.dist[at] : 0;
      }
    }
  }
  if (STATS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      km_u64 v = acc[j];
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) v += km_xor_u64(v, m);
      if ((tid & 63) == 0) red[tid >> 6][j] = v;
    }
    __syncthreads();
    if (tid < 8) {
      km_u64 v = 0;
      for (int w = 0; w < kKmThreads / 64; ++w) v += red[w][tid];
      if (v) atomicAdd((km_u64*)a.stats + tid, v);
    }
  }
}

// one workgroup per channel: thread t owns the words [t per, (t + 1) per)
__global__ __launch_bounds__(kKmThreads) void km_scan_kernel(const unsigned* counts, int nwords, unsigned* off) {
  __shared__ unsigned part[kKmThreads];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int per = (nwords + kKmThreads - 1) / kKmThreads;
  const int k0 = min(tid * per, nwords), k1 = min(k0 + per, nwords);
  const unsigned* cnt = counts + (size_t)c * nwords;
  unsigned* o = off + (size_t)c * (nwords + 1);
  unsigned sum = 0;
  for (int k = k0; k < k1; ++k) sum += cnt[k];
  part[tid] = sum;
  __syncthreads();
  for (int m = 1; m < kKmThreads; m <<= 1) {  // inclusive scan over the threads
    const unsigned add = tid >= m ? part[tid - m] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  unsigned at = part[tid] - sum;
  for (int k = k0; k < k1; ++k) {
    o[k] = at;
    at += cnt[k];
  }
  if (tid == kKmThreads - 1) o[nwords] = part[tid];
}

__global__ __launch_bounds__(kKmThreads) void km_scatter_kernel(KmArgs a) {
  const long long i = (long long)blockIdx.x * kKmThreads + threadIdx.x;
  if (i >= min(a.info[0], (long long)a.max_tracks)) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned r = a.rank[(size_t)i * 4 + c];
    if (r == kKmNoRank) continue;
    const int w = a.words[(size_t)i * 4 + c];  // (inside the codebook: the count said so)
    a.order[(size_t)c * a.max_tracks + a.off[(size_t)c * (a.nwords + 1) + w] + r] = (unsigned)i;
  }
}

// the rounded mean floor((2 S + M) / (2 M)) = floor(S / M) + (2 (S mod M) >= M) without leaving 32 bits (S < 2^32, M <= 2^24)
__device__ __forceinline__ unsigned km_mean(unsigned S, unsigned M) {
  const unsigned q = S / M, r = S - q * M;
  return q + (2 * r >= M ? 1 : 0);
}

template <int NP>
__global__ __launch_bounds__(kKmThreads) void km_sum_kernel(KmArgs a) {
  constexpr int U = NP == 1 ? 4 : 2;  // members in flight per lane group
  __shared__ unsigned slots[kKmThreads / 64][kKmChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y, C = a.C, K = a.nwords;
  const unsigned* off = a.off + (size_t)c * (K + 1);
  const unsigned total = off[K];
  const unsigned chunk = blockIdx.x * (kKmThreads / 64) + wave;
  const unsigned p0 = chunk * kKmChunk, p1 = min(p0 + kKmChunk, total);
#pragma unroll
  for (int j = 0; j < kKmChunk / 64; ++j) {
    const unsigned p = p0 + 64 * j + lane;
    slots[wave][64 * j + lane] = p < p1 ? a.order[(size_t)c * a.max_tracks + p] : 0;
  }
  __syncthreads();
  if (p0 >= total) return;
  const int el = lane & (a.el - 1), g = lane >> a.log2el, ml = 64 >> a.log2el;
  const int offc = km_ch_off(c, C), n_c = km_ch_len(c, C), nd = (n_c + 3) >> 2;
  const size_t D = (size_t)33 * C;
  unsigned r = 0;
  const unsigned rend = p1 - p0;
  while (r < rend) {
    const int k = __builtin_amdgcn_readfirstlane(a.words[(size_t)slots[wave][r] * 4 + c]);  // the word of this run
    const unsigned a0 = off[k], b0 = off[k + 1];
    const unsigned rr = min(b0, p1) - p0;  // (> r: position p0 + r lies in [a0, b0))
    unsigned lo[NP], hi[NP];  // bytes 0 and 2, bytes 1 and 3 of the lane's dwords, 16 bits each
#pragma unroll
    for (int p = 0; p < NP; ++p) lo[p] = hi[p] = 0;
    for (; r < rr; r += ml * U) {
      unsigned v[U][NP];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned m = r + u * ml + g;
        const bool ok = m < rr;
        const uint8_t* row = a.desc + (size_t)slots[wave][ok ? m : 0] * D + offc;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int d = el + 64 * p;  // (NP > 1: EL = 64)
          // a whole dword never leaves the row: the one channel whose length may be no multiple of 4 has a channel behind it
          v[u][p] = ok && d < nd ? *(const km_u32_any*)(row + 4 * d) : 0u;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          lo[p] += v[u][p] & 0x00ff00ffu;
          hi[p] += (v[u][p] >> 8) & 0x00ff00ffu;
        }
    }
    r = rr;
    if (NP == 1) {  // the lane groups held different members
#pragma unroll
      for (int m = 32; m >= 4; m >>= 1)
        if (m >= a.el) {  // (uniform)
          lo[0] += __shfl_xor(lo[0], m);
          hi[0] += __shfl_xor(hi[0], m);
        }
    }
    const bool whole = a0 >= p0 && b0 <= p1;
    const unsigned cnt = b0 - a0;
    if (g == 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int d = el + 64 * p, e = 4 * d;
        const unsigned S[4] = {lo[p] & 0xffffu, hi[p] & 0xffffu, lo[p] >> 16, hi[p] >> 16};
        if (whole) {
          if (d < nd) {
            uint8_t* to = a.codebook + (size_t)k * D + offc + e;
            const unsigned q[4] = {km_mean(S[0], cnt), km_mean(S[1], cnt), km_mean(S[2], cnt), km_mean(S[3], cnt)};
            if (e + 3 < n_c) {
              *(km_u32_any*)to = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
            } else {  // the bytes behind the channel belong to the next one
#pragma unroll
              for (int b = 0; b < 3; ++b)
                if (e + b < n_c) to[b] = (uint8_t)q[b];
            }
          }
        } else {  // a part of a longer segment: the chunk's head (the segment began before it) or tail row
          unsigned* to = a.slab + (((size_t)c * a.nch + chunk) * 2 + (a0 < p0 ? 0 : 1)) * a.rl + e;
          *(uint2*)to = make_uint2(S[0], S[1]);
          *(uint2*)(to + 2) = make_uint2(S[2], S[3]);
        }
      }
    }
  }
}

// a workgroup per (word, channel): nothing to do unless the word's segment spans chunks
__global__ __launch_bounds__(kKmThreads) void km_finish_kernel(KmArgs a) {
  __shared__ unsigned red[kKmThreads];
  const int tid = threadIdx.x, k = blockIdx.x, c = blockIdx.y, C = a.C;
  const unsigned* off = a.off + (size_t)c * (a.nwords + 1);
  const unsigned a0 = off[k], b0 = off[k + 1];
  if (a0 == b0) return;  // an empty word keeps its bytes (uniform, like the next)
  const unsigned j0 = a0 / kKmChunk, j1 = (b0 - 1) / kKmChunk, cnt = b0 - a0;
  if (j0 == j1) return;
  const int offc = km_ch_off(c, C), n_c = km_ch_len(c, C);
  const int log2te = OFDIS_KM_FINISH_LOG2TE(n_c), te = 1 << log2te, jg = kKmThreads >> log2te;  // entries x chunk groups
  const int e0 = tid & (te - 1), gj = tid >> log2te;
  const unsigned* slab = a.slab + (size_t)c * a.nch * 2 * a.rl;
  for (int eb = 0; eb < n_c; eb += te) {
    const int e = eb + e0;
    unsigned s = 0;
    if (e < n_c)
      for (unsigned j = j0 + gj; j <= j1; j += jg) s += slab[((size_t)j * 2 + (j == j0 ? 1 : 0)) * a.rl + e];
    red[tid] = s;
    __syncthreads();
    if (gj == 0 && e < n_c) {
      for (int q = 1; q < jg; ++q) s += red[q * te + e0];
      a.codebook[(size_t)k * 33 * C + offc + e] = (uint8_t)km_mean(s, cnt);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_codebook_seed(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                                int min_len, uint8_t* codebook, hipStream_t s) {
  hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)nwords), dim3(64), 0, s, desc, len, info, max_tracks, 33 * nxy * nxy * nt, nwords,
                     min_len, codebook);
  return hipGetLastError();
}

// one update; prev and dist are used with stats alone
static hipError_t km_update(const uint8_t* desc, const int* words, const int* len, const long long* info, int max_tracks, int C,
                            int nwords, int min_len, int first, uint8_t* codebook, uint32_t* counts, long long* stats, void* work,
                            hipStream_t s) {
  const KmLayout l = kmeans_layout(max_tracks, C, nwords);
  const KmGeom g = km_geom(C);
  uint8_t* w = (uint8_t*)work;
  const int nch = (max_tracks + kKmChunk - 1) / kKmChunk;
  const KmArgs a{desc, words, len, info, max_tracks, C, nwords, min_len, first, codebook, counts, stats, (int*)(w + l.prev),
                 (const int*)(w + l.dist), (unsigned*)(w + l.rank), (unsigned*)(w + l.off), (unsigned*)(w + l.order),
                 (unsigned*)(w + l.slab), g.el, g.log2el, g.rl, nch};
  const dim3 threads(kKmThreads);
  const unsigned slot_blocks = (unsigned)((max_tracks + kKmThreads - 1) / kKmThreads);
  hipLaunchKernelGGL(km_clear_kernel, dim3((unsigned)((4 * nwords + kKmThreads - 1) / kKmThreads)), threads, 0, s, counts, 4 * nwords,
                     stats);
  const dim3 count_grid(slot_blocks < (unsigned)kKmCountBlocks ? slot_blocks : (unsigned)kKmCountBlocks);
  if (stats)
    hipLaunchKernelGGL(km_count_kernel<true>, count_grid, threads, 0, s, a);
  else
    hipLaunchKernelGGL(km_count_kernel<false>, count_grid, threads, 0, s, a);
  hipLaunchKernelGGL(km_scan_kernel, dim3(4), threads, 0, s, counts, nwords, a.off);
  hipLaunchKernelGGL(km_scatter_kernel, dim3(slot_blocks), threads, 0, s, a);
  const dim3 sum_grid((unsigned)((nch + kKmThreads / 64 - 1) / (kKmThreads / 64)), 4);
  if (g.np == 1)
    hipLaunchKernelGGL(km_sum_kernel<1>, sum_grid, threads, 0, s, a);
  else
    hipLaunchKernelGGL(km_sum_kernel<5>, sum_grid, threads, 0, s, a);
  hipLaunchKernelGGL(km_finish_kernel, dim3((unsigned)nwords, 4), threads, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_codebook_update(const uint8_t* desc, const int* words, const int* len, const long long* info, int max_tracks, int nxy,
                                  int nt, int nwords, int min_len, uint8_t* codebook, uint32_t* counts, void* work, hipStream_t s) {
  return km_update(desc, words, len, info, max_tracks, nxy * nxy * nt, nwords, min_len, 0, codebook, counts, nullptr, work, s);
}

hipError_t launch_codebook_train(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                                 int min_len, int iters, uint8_t* codebook, int* words, uint32_t* counts, long long* stats, void* work,
                                 hipStream_t s) {
  const int C = nxy * nxy * nt;
  int* dist = stats ? (int*)((uint8_t*)work + kmeans_layout(max_tracks, C, nwords).dist) : nullptr;
  for (int t = 0; t < iters; ++t) {
    if (hipError_t e = launch_codebook_assign(desc, info, max_tracks, nxy, nt, codebook, nwords, words, dist, s)) return e;
    if (hipError_t e = km_update(desc, words, len, info, max_tracks, C, nwords, min_len, t == 0, codebook, counts,
                                 stats ? stats + (size_t)t * 8 : nullptr, work, s))
      return e;
  }
  return hipSuccess;
}

}  // namespace ofdis
