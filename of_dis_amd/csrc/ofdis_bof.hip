// ofdis_bof.hip -- bag-of-features encoding of the dense-track descriptors (include/ofdis.h: ofdis_descriptor_normalize,
// ofdis_codebook_assign, ofdis_bof_histogram, ofdis_track_bof): the four histogram channels of a hist row as 8-bit RootSIFT
// descriptors, every channel matched against the words of a codebook by exact squared distance, and the per-clip count of the
// words (Wang, Klaeser, Schmid and Liu, "Dense trajectories and motion boundary descriptors", 2013, section 4).
//
// Everything here is integer arithmetic: a descriptor entry is the largest q with q*q*S <= 510*510*h in uint64, a distance is an
// int32 the matrix cores compute exactly, the nearest word is the lowest index that attains the minimum, the counts are integer
// atomics.  The bits depend neither on the mapping below nor on the arithmetic contract; compiled once.
//
// Distances.  With x' = x - 128 and c' = c - 128 (the bytes x ^ 0x80, c ^ 0x80 read as int8) the difference x - c is unchanged
// and d = |x'|^2 + |c'|^2 - 2 x'.c'; the dot products of 16 words with 16 tracks over 64 entries are one
// v_mfma_i32_16x16x64_i8.  A = the words (the staged tile), B = the tracks (registers): lane l supplies 16 consecutive bytes of
// row l & 15 of either operand, the bytes [64 s + 16 (l >> 4), + 16) of k-step s -- the same pattern on both sides, so the sum
// over k is the same whatever order the instruction takes the 64 products in.  The result has its track on the lane
// (col = l & 15) and its words in the registers (row = 4 (l >> 4) + reg): every lane keeps the running minimum of its track
// over the words it sees in ascending order (replace on strictly smaller), and the four lanes of a track are merged at the end
// with the lower index winning a tie.  Entries past the channel's length are the byte 0 on both sides and add nothing; words
// past nwords never win, tracks past ntracks are never stored.
//
// Mapping.  A workgroup of four wavefronts owns 64 TG consecutive slots of one channel (blockIdx.y); a wavefront holds the
// fragments of its 16 TG tracks in registers for the whole kernel, NK k-steps each.  (NK, TG) is (2, 8), (6, 3) or (18, 1) by
// the longest channel, 9 C <= 128, 384, 1152 bytes: 16 to 18 fragments of four registers.  The codebook goes through LDS in
// tiles of 16 TG words, signed, padded and with |c'|^2 summed on the way (LDS atomics); a row is NK 64 + 16 bytes, an odd number
// of 16-byte chunks, so the 16 rows a ds_read_b128 touches fall into different banks.  A tile is staged once per workgroup and
// used by TG x TG x nk MFMAs in every wavefront.  No wavefront hands anything to another.
//
// The fused route (FUSED) differs in where a track's bytes come from: the channel's uint64 sum over the hist row first, then
// the entries again (the wavefront's own 16 TG rows, an L2 hit) through bof_root into the fragments; desc is never written.
#include "../../include/ofdis.h"
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kBofThreads = 256;  // four wavefronts
constexpr int kBofNoWord = 0x3ffffffc;  // the key of a word past nwords: above 4 (|c'|^2 - 2 x'.c') + 3 of any real word (< 2^28)
typedef int bof_v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long bof_u64;

// where channel c (HOG, HOF, MBHx, MBHy) starts in a row and how long it is, C = nxy^2 nt
__device__ __forceinline__ int bof_ch_off(int c, int C) { return c == 0 ? 0 : c == 1 ? 8 * C : c == 2 ? 17 * C : 25 * C; }
__device__ __forceinline__ int bof_ch_len(int c, int C) { return c == 1 ? 9 * C : 8 * C; }

__device__ __forceinline__ bof_u64 bof_xor_u64(bof_u64 v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((bof_u64)hi << 32) | lo;
}

// desc_e of include/ofdis.h: min(255, max{q >= 0 : q q S <= 510^2 h}) for an entry h of a channel with the sum S >= h.  The
// float quotient only proposes a q: T < 2^50 and S < 2^43 convert, divide and take the root with a relative error below 2^-21,
// which is below 2^-13 on a q <= 254, so the truncated root is the answer or one off; the exact products (below 2^62) settle
// it, two steps either way and without a branch.
__device__ __forceinline__ unsigned bof_root(unsigned h, bof_u64 S) {
  const bof_u64 T = (bof_u64)(OFDIS_BOF_SCALE * OFDIS_BOF_SCALE) * h;
  int q = min(max((int)sqrtf((float)T / (float)max(S, (bof_u64)1)), 0), 254);
#pragma unroll
  for (int i = 0; i < 2; ++i) q -= (bof_u64)(q * q) * S > T ? 1 : 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) q += (bof_u64)((q + 1) * (q + 1)) * S <= T ? 1 : 0;  // (from 254 up to 256 where the clamp acts)
  return h ? (unsigned)min(q, 255) : 0u;  // (S == 0 included)
}

// ------------------------------------------------------------------------------------ ofdis_descriptor_normalize
// one wavefront per slot, the channels in turn: the sum over the lanes, then every lane its entries
__global__ __launch_bounds__(64) void bof_normalize_kernel(const unsigned* hist, const long long* info, int max_tracks, int C,
                                                           uint8_t* desc) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= min(info[0], (long long)max_tracks)) return;  // (uniform over the workgroup)
  const size_t D = (size_t)33 * C;
  const unsigned* h = hist + (size_t)slot * D;
  uint8_t* d = desc + (size_t)slot * D;
  for (int c = 0; c < 4; ++c) {
    const int off = bof_ch_off(c, C), n = bof_ch_len(c, C);
    bof_u64 S = 0;
    for (int e = lane; e < n; e += 64) S += h[off + e];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) S += bof_xor_u64(S, m);
    for (int e = lane; e < n; e += 64) d[off + e] = (uint8_t)bof_root(h[off + e], S);
  }
}

// ------------------------------------------------------------------------------------ ofdis_codebook_assign, ofdis_track_bof
struct BofArgs {
  const uint8_t* desc;   // [max_tracks][D] (assignment)
  const unsigned* hist;  // [max_tracks][D] (fused)
  const int* len;        // [max_tracks] (fused)
  const long long* info;
  const uint8_t* codebook;  // [nwords][D]
  int max_tracks, C, nwords, min_len;
  int* words;     // [max_tracks][4] or null
  int* dist;      // [max_tracks][4] or null
  unsigned* bof;  // [4][nwords] (fused)
};

template <int NK, int TG, bool FUSED>
__global__ __launch_bounds__(kBofThreads) void bof_assign_kernel(BofArgs a) {
  constexpr int kRow = NK * 64 + 16;  // bytes of a staged word
  constexpr int kTile = 16 * TG;      // words of a tile
  __shared__ __attribute__((aligned(16))) uint8_t cw[kTile * kRow];
  // per word of the tile, by the tile's parity: the key 4 |c'|^2 + (w & 3), or kBofNoWord + (w & 3) for a word past nwords.
  // (w & 3) is the register the word's result lands in, so key - 8 x'.c' = 4 (|c'|^2 - 2 x'.c') + reg orders a lane's four
  // results by (distance, word) in one integer, and one past nwords loses against every real one
  __shared__ __attribute__((aligned(16))) int cn[2][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int c = blockIdx.y, C = a.C;
  const long long ntracks = min(a.info[0], (long long)a.max_tracks);
  const long long base = (long long)blockIdx.x * (64 * TG);
  if (base >= ntracks) return;  // (uniform over the workgroup)
  const int off = bof_ch_off(c, C), n = bof_ch_len(c, C), nk = (n + 63) >> 6;
  const size_t D = (size_t)33 * C;

  // the tracks' fragments: lane (col, g) holds the bytes [64 s + 16 g, + 16) of track col of group t
  bof_v4i b[TG][NK];
  int xn[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    const long long i = base + (wave * TG + t) * 16 + col;
    const bool live = i < ntracks;
    bof_u64 S = 0;
    if (FUSED) {
      if (live)
        for (int s = 0; s < nk; ++s)
          for (int j = 0; j < 16; ++j) {
            const int e = 64 * s + 16 * g + j;
            if (e < n) S += a.hist[(size_t)i * D + off + e];
          }
      S += bof_xor_u64(S, 16);
      S += bof_xor_u64(S, 32);
    }
    int sq = 0;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      bof_v4i f = {0, 0, 0, 0};
      if (s < nk && live) {
        const int e0 = 64 * s + 16 * g;
        const size_t at = (size_t)i * D + off + e0;
        if (FUSED) {
          // one copy of the root per fragment: the 16 entries in a loop, a word of four into its register by selects
          unsigned w = 0;
#pragma unroll 1
          for (int j = 0; j < 16; ++j) {
            if (e0 + j < n) {
              const int sx = (int)bof_root(a.hist[at + j], S) - 128;
              sq += sx * sx;
              w |= (unsigned)(sx & 255) << (8 * (j & 3));
            }
            if ((j & 3) == 3) {
              const int jw = j >> 2;
              f.x = jw == 0 ? (int)w : f.x;
              f.y = jw == 1 ? (int)w : f.y;
              f.z = jw == 2 ? (int)w : f.z;
              f.w = jw == 3 ? (int)w : f.w;
              w = 0;
            }
          }
        } else {
#pragma unroll
          for (int jw = 0; jw < 4; ++jw) {
            unsigned w = 0;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb)
              if (e0 + 4 * jw + jb < n) {
                const int sx = (int)a.desc[at + 4 * jw + jb] - 128;
                sq += sx * sx;
                w |= (unsigned)(sx & 255) << (8 * jb);
              }
            f[jw] = (int)w;
          }
        }
      }
      b[t][s] = f;
    }
    sq += __shfl_xor(sq, 16);
    sq += __shfl_xor(sq, 32);
    xn[t] = sq;
  }

  int best[TG], bk[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) best[t] = kBofNoWord >> 2, bk[t] = 0;  // (best: |c'|^2 - 2 x'.c' of word bk)

  const unsigned nk16 = (unsigned)nk * 16;                                // dwords of a staged word that are read
  const unsigned by_nk16 = (unsigned)((0x100000000ull + nk16 - 1) / nk16);  // u / nk16 == umulhi(u, by_nk16) for u < 2^16
  if (tid < kTile) cn[0][tid] = (tid < a.nwords ? 0 : kBofNoWord) + (tid & 3);
  int par = 0;
  for (int tile0 = 0; tile0 < a.nwords; tile0 += kTile, par ^= 1) {
    __syncthreads();  // the tile before this one is used up
    if (tid < kTile) cn[par ^ 1][tid] = (tile0 + kTile + tid < a.nwords ? 0 : kBofNoWord) + (tid & 3);  // the next tile's
    for (unsigned u = tid; u < kTile * nk16; u += kBofThreads) {
      const unsigned w = __umulhi(u, by_nk16), dw = u - w * nk16;
      const int k = tile0 + (int)w, e0 = 4 * (int)dw;
      unsigned pack = 0;
      int sq = 0;
      if (k < a.nwords && e0 < n) {
        const uint8_t* p = a.codebook + (size_t)k * D + off + e0;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          if (e0 + jb < n) {
            const int sx = (int)p[jb] - 128;
            sq += sx * sx;
            pack |= (unsigned)(sx & 255) << (8 * jb);
          }
      }
      *(unsigned*)(cw + w * kRow + 4 * dw) = pack;
      if (sq) atomicAdd(&cn[par][w], 4 * sq);
    }
    __syncthreads();
#pragma unroll 1
    for (int ws = 0; ws < TG; ++ws) {
      const int k0 = tile0 + ws * 16;
      if (k0 >= a.nwords) break;  // (uniform)
      bof_v4i acc[TG];
#pragma unroll
      for (int t = 0; t < TG; ++t) acc[t] = bof_v4i{0, 0, 0, 0};
      const uint8_t* row = cw + (ws * 16 + col) * kRow + g * 16;
#pragma unroll
      for (int s = 0; s < NK; ++s) {
        if (s < nk) {  // (uniform)
          const bof_v4i av = *(const bof_v4i*)(row + s * 64);
#pragma unroll
          for (int t = 0; t < TG; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b[t][s], acc[t], 0, 0, 0);
        }
      }
      // register r of lane (col, g): word k0 + 4 g + r against track col.  The least key of the four, then strictly smaller
      // than what the earlier words gave: the lowest word at the minimum
      const bof_v4i c4 = *(const bof_v4i*)&cn[par][ws * 16 + g * 4];
      const int kg = k0 + g * 4;
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        const int m = min(min(c4[0] - 8 * acc[t][0], c4[1] - 8 * acc[t][1]), min(c4[2] - 8 * acc[t][2], c4[3] - 8 * acc[t][3]));
        const int v = m >> 2;
        const bool take = v < best[t];
        best[t] = take ? v : best[t];
        bk[t] = take ? kg + (m & 3) : bk[t];
      }
    }
  }

#pragma unroll
  for (int t = 0; t < TG; ++t) {
    int v = best[t], k = bk[t];
#pragma unroll
    for (int m = 16; m < 64; m <<= 1) {
      const int ov = __shfl_xor(v, m), ok = __shfl_xor(k, m);
      const bool take = (ov < v) | ((ov == v) & (ok < k));
      v = take ? ov : v;
      k = take ? ok : k;
    }
    const long long i = base + (wave * TG + t) * 16 + col;
    if (g == 0 && i < ntracks) {
      if (a.words) a.words[(size_t)i * 4 + c] = k;
      if (a.dist) a.dist[(size_t)i * 4 + c] = v + xn[t];
      if (FUSED && a.len[i] >= a.min_len) atomicAdd(a.bof + (size_t)c * a.nwords + k, 1u);
    }
  }
}

BofShape bof_assign_shape(int C) {
  const int nk = (9 * C + 63) / 64;  // the k-steps of the longest channel
  return nk <= 2 ? BofShape{nk, 2, 8} : nk <= 6 ? BofShape{nk, 6, 3} : BofShape{nk, 18, 1};
}

template <bool FUSED>
static hipError_t bof_assign_launch(const BofArgs& a, hipStream_t s) {
  const BofShape sh = bof_assign_shape(a.C);
  const dim3 grid((unsigned)((a.max_tracks + 64 * sh.TG - 1) / (64 * sh.TG)), 4);
  if (sh.NK == 2)
    hipLaunchKernelGGL((bof_assign_kernel<2, 8, FUSED>), grid, dim3(kBofThreads), 0, s, a);
  else if (sh.NK == 6)
    hipLaunchKernelGGL((bof_assign_kernel<6, 3, FUSED>), grid, dim3(kBofThreads), 0, s, a);
  else
    hipLaunchKernelGGL((bof_assign_kernel<18, 1, FUSED>), grid, dim3(kBofThreads), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ ofdis_bof_histogram
__global__ __launch_bounds__(kBofThreads) void bof_clear_kernel(unsigned* bof, int n) {
  const int i = blockIdx.x * kBofThreads + threadIdx.x;
  if (i < n) bof[i] = 0;
}

__global__ __launch_bounds__(kBofThreads) void bof_count_kernel(const int* words, const int* len, const long long* info,
                                                                int max_tracks, int nwords, int min_len, unsigned* bof) {
  const long long i = (long long)blockIdx.x * kBofThreads + threadIdx.x;
  if (i >= min(info[0], (long long)max_tracks) || len[i] < min_len) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = words[(size_t)i * 4 + c];
    if ((unsigned)k < (unsigned)nwords) atomicAdd(bof + (size_t)c * nwords + k, 1u);  // (a word outside the codebook: not counted)
  }
}

static hipError_t bof_clear(uint32_t* bof, int nwords, hipStream_t s) {
  hipLaunchKernelGGL(bof_clear_kernel, dim3((unsigned)((4 * nwords + kBofThreads - 1) / kBofThreads)), dim3(kBofThreads), 0, s, bof,
                     4 * nwords);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_descriptor_normalize(const uint32_t* hist, const long long* info, int max_tracks, int nxy, int nt, uint8_t* desc,
                                       hipStream_t s) {
  hipLaunchKernelGGL(bof_normalize_kernel, dim3((unsigned)max_tracks), dim3(64), 0, s, hist, info, max_tracks, nxy * nxy * nt, desc);
  return hipGetLastError();
}

hipError_t launch_codebook_assign(const uint8_t* desc, const long long* info, int max_tracks, int nxy, int nt, const uint8_t* codebook,
                                  int nwords, int* words, int* dist, hipStream_t s) {
  const BofArgs a{desc, nullptr, nullptr, info, codebook, max_tracks, nxy * nxy * nt, nwords, 1, words, dist, nullptr};
  return bof_assign_launch<false>(a, s);
}

hipError_t launch_bof_histogram(const int* words, const int* len, const long long* info, int max_tracks, int nwords, int min_len,
                                uint32_t* bof, hipStream_t s) {
  if (hipError_t e = bof_clear(bof, nwords, s)) return e;
  hipLaunchKernelGGL(bof_count_kernel, dim3((unsigned)((max_tracks + kBofThreads - 1) / kBofThreads)), dim3(kBofThreads), 0, s, words,
                     len, info, max_tracks, nwords, min_len, bof);
  return hipGetLastError();
}

hipError_t launch_track_bof(const uint32_t* hist, const int* len, const long long* info, int max_tracks, int nxy, int nt,
                            const uint8_t* codebook, int nwords, int min_len, uint32_t* bof, int* words, hipStream_t s) {
  if (hipError_t e = bof_clear(bof, nwords, s)) return e;
  const BofArgs a{nullptr, hist, len, info, codebook, max_tracks, nxy * nxy * nt, nwords, min_len, words, nullptr, bof};
  return bof_assign_launch<true>(a, s);
}

}  // namespace ofdis
