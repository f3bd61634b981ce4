// ofdis_track_select.hip -- track selection for (improved) dense trajectories (include/ofdis.h: ofdis_track_select): every slot
// of ofdis_dense_tracks is classified -- too short, not finite, static, erratic, one dominating jump, or (given the camera
// models of ofdis_global_motion) moving only as the camera does -- and the kept slots are compacted, in their order, into a
// fresh set of the same layout (Wang, Klaeser, Schmid and Liu 2013; Wang and Schmid, "Action recognition with improved
// trajectories", 2013).
//
// Compiled under the exact contract only (-ffp-contract=off): every fp32 operation of the header is separately rounded and
// every sum runs over ascending j inside one lane, so the bits depend on nothing below.
//
// Mapping.  Three launches on the caller's stream; output slot numbers are a prefix sum over the input slot numbers, as the
// seed numbers of ofdis_dense_tracks.hip are: no atomic, no grid-wide barrier, no wait on another workgroup.
//   classify  one lane per slot, kTsLanes slots per workgroup.  The tracks are step-major, so step j of 64 neighbouring slots
//             is 512 contiguous bytes: every load of a wavefront is one coalesced access.  Two walks over the L positions (sums,
//             steps and residuals; then the spreads around the means) -- the second hits in L2.  It writes `code`, and into the
//             workgroup's record of `work` the seven counts per code and, per wavefront, the 64-bit ballot of the kept lanes.
//   scan      ONE workgroup: the exclusive prefix sum of the kept counts over the workgroups, kTsLanes records per trip (a
//             wave scan by lane shifts, the four wave totals through LDS); the totals per code; info_out and counts.
//   scatter   the same lanes as classify.  A kept lane reads its rank from the ballots (popcounts of the wavefronts before it
//             and of the lanes before it in its own), adds the workgroup's offset, copies the lmax + 1 positions, start and
//             len, writes index and computes shape_out.  The destinations of a wavefront are monotone and, where the kept
//             lanes are neighbours, contiguous.  What the shape needs (S or Sr) is recomputed from the positions the lane
//             copies anyway: cheaper than a float per slot through the work buffer.
// The record of a workgroup: int32 [8] = the counts of the codes 0 .. 6 and (written by the scan) the kept slots of the
// workgroups before it, then u64 [4] ballots: 64 bytes per kTsLanes slots.
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kTsLanes = 256;             // slots per workgroup (capi.py: TRACK_SELECT_LANES)
constexpr int kTsWaves = kTsLanes / 64;
constexpr int kTsCodes = 7;               // kept + the six OFDIS_TS_* codes
constexpr unsigned kTsIdle = 0xFFu;       // the code of a lane without a slot (never stored)
// every grid below is one launch: no chunk walk is needed
static_assert((OFDIS_DT_MAX_TRACKS + kTsLanes - 1) / kTsLanes < GRID_MAX_BLOCKS, "one launch covers OFDIS_DT_MAX_TRACKS slots");

struct TsRecord {
  int count[kTsCodes];
  int before;  // kept slots of the workgroups before this one (the scan)
  unsigned long long kept[kTsWaves];
};
static_assert(sizeof(TsRecord) == 64, "the work record is 64 bytes");

struct TsArgs {
  const float2* tracks;   // [lmax + 1][max_tracks]
  const int* start;       // [max_tracks]
  const int* len;         // [max_tracks]
  const long long* info;  // {ntracks, dropped}
  int lmax, max_tracks;
  const double* models;   // [npairs][nparam] or null
  int npairs, nparam;     // nparam: 6, or 8 for the projective models (ofdis_track_select_projective)
  float cx, cy;           // (float)(W - 1) * 0.5f, (float)(H - 1) * 0.5f
  ofdis_track_select_params p;
  uint8_t* code;          // [max_tracks] or null
  long long* counts;      // [7] or null
  int max_out;
  float2* tracks_out;     // [lmax + 1][max_out]
  int* start_out;         // [max_out]
  int* len_out;           // [max_out]
  long long* info_out;    // {nkept_written, dropped_out}
  int* index;             // [max_out] or null
  float2* shape_out;      // [max_out][lmax] or null
  TsRecord* work;         // [workgroups]
};

__device__ __forceinline__ int ts_slots(const TsArgs& a) { return (int)min(max(a.info[0], 0ll), (long long)a.max_tracks); }
__device__ __forceinline__ bool ts_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }  // (NaN: false)
__device__ __forceinline__ bool ts_on(const TsArgs& a, int code) { return (a.p.tests >> (code - 1)) & 1u; }

// The step of slot i from p (step j) to q: d = q - p and, with models, the residual under the model of pair k = first + j.
// Returns false where k lies outside the models (then r = d).
__device__ __forceinline__ bool ts_step(const TsArgs& a, int k, float2 p, float2 q, float2& d, float2& r) {
  d = make_float2(q.x - p.x, q.y - p.y);
  r = d;
  if (!a.models) return true;
  if (k < 0 || k >= a.npairs) return false;
  const double* m = a.models + (size_t)k * a.nparam;
  const float a0 = (float)m[0], a1 = (float)m[1], a2 = (float)m[2], a3 = (float)m[3], a4 = (float)m[4], a5 = (float)m[5];
  const float xc = p.x - a.cx, yc = p.y - a.cy;
  float mu = (a0 + a1 * xc) + a2 * yc, mv = (a3 + a4 * xc) + a5 * yc;
  if (a.nparam == 8) {  // (uniform) the quadratic terms of the projective model
    const float pq = (float)m[6] * xc + (float)m[7] * yc;
    mu = mu + pq * xc;
    mv = mv + pq * yc;
  }
  r = make_float2(d.x - mu, d.y - mv);
  return true;
}

// the code of slot i (include/ofdis.h: the first test that holds)
__device__ __forceinline__ unsigned ts_classify(const TsArgs& a, int i) {
  const int L = min(max(a.len[i], 0), a.lmax + 1), first = a.start[i];
  const float fl = (float)L;
  bool finite = true, pairs = true;
  float sumx = 0.f, sumy = 0.f, S = 0.f, mmax = 0.f, rmax = 0.f;
  float2 p = make_float2(0.f, 0.f);
  for (int j = 0; j < L; ++j) {
    const float2 q = a.tracks[(size_t)j * a.max_tracks + i];
    finite &= ts_finite(q.x) & ts_finite(q.y);
    sumx += q.x;
    sumy += q.y;
    if (j) {
      float2 d, r;
      pairs &= ts_step(a, first + j - 1, p, q, d, r);
      const float m = sqrtf(d.x * d.x + d.y * d.y), rm = sqrtf(r.x * r.x + r.y * r.y);
      S += m;
      mmax = m > mmax ? m : mmax;
      rmax = rm > rmax ? rm : rmax;
    }
    p = q;
  }
  const float mx = sumx / fl, my = sumy / fl;
  float vx = 0.f, vy = 0.f;
  for (int j = 0; j < L; ++j) {
    const float2 q = a.tracks[(size_t)j * a.max_tracks + i];
    const float ex = q.x - mx, ey = q.y - my;
    vx += ex * ex;
    vy += ey * ey;
  }
  const float sx = sqrtf(vx / fl), sy = sqrtf(vy / fl);
  const ofdis_track_select_params& t = a.p;
  if (ts_on(a, 1) && L < max(t.min_len, 1)) return 1;
  if (ts_on(a, 2) && !(finite && pairs)) return 2;
  if (ts_on(a, 3) && sx < t.min_std && sy < t.min_std) return 3;
  if (ts_on(a, 4) && (sx > t.max_std || sy > t.max_std)) return 4;
  if (ts_on(a, 5) && L >= 2 && mmax > t.max_step && mmax > S * t.max_step_share) return 5;
  if (ts_on(a, 6) && a.models && L >= 2 && rmax <= t.min_camera) return 6;
  return 0;
}

__global__ __launch_bounds__(kTsLanes) void track_select_classify_kernel(TsArgs a) {
  __shared__ int lds[kTsWaves][kTsCodes];
  const int i = blockIdx.x * kTsLanes + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned code = i < ts_slots(a) ? ts_classify(a, i) : kTsIdle;
  if (code != kTsIdle && a.code) a.code[i] = (uint8_t)code;
  TsRecord& rec = a.work[blockIdx.x];
#pragma unroll
  for (int c = 0; c < kTsCodes; ++c) {
    const unsigned long long has = __ballot(code == (unsigned)c);
    if (lane == 0) {
      lds[wave][c] = __popcll(has);
      if (c == 0) rec.kept[wave] = has;
    }
  }
  __syncthreads();
  if (threadIdx.x < kTsCodes) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < kTsWaves; ++w) n += lds[w][threadIdx.x];
    rec.count[threadIdx.x] = n;
  }
}

// the sum of v over the workgroup's kTsLanes lanes, in every lane
template <class T>
__device__ __forceinline__ T ts_block_sum(T v, T* lds) {
  for (int k = 32; k > 0; k >>= 1) v += __shfl_xor(v, k);
  __syncthreads();  // (lds may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T sum = 0;
#pragma unroll
  for (int w = 0; w < kTsWaves; ++w) sum += lds[w];
  return sum;
}

__global__ __launch_bounds__(kTsLanes) void track_select_scan_kernel(TsArgs a, int workgroups) {
  __shared__ int lds[kTsWaves];
  __shared__ long long lds64[kTsWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;  // the kept slots of the records before this trip
  long long per_code[kTsCodes] = {};
  for (int b0 = 0; b0 < workgroups; b0 += kTsLanes) {  // (uniform)
    const int b = b0 + threadIdx.x;
    int kept = 0;
    if (b < workgroups) {
      kept = a.work[b].count[0];
#pragma unroll
      for (int c = 0; c < kTsCodes; ++c) per_code[c] += a.work[b].count[c];
    }
    int incl = kept;  // the inclusive scan over the wavefront, then the totals of the wavefronts before
    for (int k = 1; k < 64; k <<= 1) {
      const int up = __shfl_up(incl, k);
      if (lane >= k) incl += up;
    }
    __syncthreads();  // (lds may still be read from the previous trip)
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int before = carry, trip = 0;
#pragma unroll
    for (int w = 0; w < kTsWaves; ++w) {
      if (w < wave) before += lds[w];
      trip += lds[w];
    }
    if (b < workgroups) a.work[b].before = before + incl - kept;
    carry += trip;
  }
#pragma unroll
  for (int c = 0; c < kTsCodes; ++c) per_code[c] = ts_block_sum(per_code[c], lds64);
  if (threadIdx.x == 0) {
    const long long written = min((long long)carry, (long long)a.max_out);
    a.info_out[0] = written;
    a.info_out[1] = carry - written;
  }
  if (a.counts && threadIdx.x < kTsCodes) {
    long long n = 0;
#pragma unroll
    for (int c = 0; c < kTsCodes; ++c) n = (int)threadIdx.x == c ? per_code[c] : n;
    a.counts[threadIdx.x] = n;
  }
}

__global__ __launch_bounds__(kTsLanes) void track_select_scatter_kernel(TsArgs a) {
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const int i = blockIdx.x * kTsLanes + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.x * kTsLanes >= ts_slots(a)) return;  // (uniform: a workgroup without a slot keeps nothing)
  const TsRecord& rec = a.work[blockIdx.x];
  int rank = rec.before;
  unsigned long long mine = 0;
#pragma unroll
  for (int w = 0; w < kTsWaves; ++w) {
    const unsigned long long m = rec.kept[w];
    if (w < wave) rank += __popcll(m);
    if (w == wave) mine = m;
  }
  if (!((mine >> lane) & 1ull)) return;  // (a lane without a slot has no bit either)
  rank += __popcll(mine & ((1ull << lane) - 1ull));
  if (rank >= a.max_out) return;  // dropped_out counts it
  const int L = min(max(a.len[i], 0), a.lmax + 1), first = a.start[i];
  a.start_out[rank] = first;
  a.len_out[rank] = a.len[i];
  if (a.index) a.index[rank] = i;
  // the copy, bit for bit, and on the way the sum the shape is divided by: S without models, Sr with them
  const u2v* src = (const u2v*)a.tracks + i;
  u2v* dst = (u2v*)a.tracks_out + rank;
  float sum = 0.f;
  float2 p = make_float2(0.f, 0.f);
  for (int j = 0; j <= a.lmax; ++j) {
    const u2v bits = src[(size_t)j * a.max_tracks];
    __builtin_nontemporal_store(bits, dst + (size_t)j * a.max_out);
    const float2 q = make_float2(__uint_as_float(bits.x), __uint_as_float(bits.y));
    if (j && j < L) {
      float2 d, r;
      ts_step(a, first + j - 1, p, q, d, r);
      sum += sqrtf(r.x * r.x + r.y * r.y);
    }
    p = q;
  }
  if (!a.shape_out) return;
  for (int j = 0; j < a.lmax; ++j) {
    float2 s = make_float2(0.f, 0.f);
    if (j < L - 1 && sum != 0.f) {
      float2 d, r;
      ts_step(a, first + j, a.tracks[(size_t)j * a.max_tracks + i], a.tracks[(size_t)(j + 1) * a.max_tracks + i], d, r);
      s = make_float2(r.x / sum, r.y / sum);
    }
    __builtin_nontemporal_store((u2v){__float_as_uint(s.x), __float_as_uint(s.y)}, (u2v*)a.shape_out + (size_t)rank * a.lmax + j);
  }
}

size_t track_select_work_bytes(int max_tracks) { return (size_t)((max_tracks + kTsLanes - 1) / kTsLanes) * sizeof(TsRecord); }

hipError_t launch_track_select(const float* tracks, const int* start, const int* len, const long long* info, int lmax, int max_tracks,
                               const double* models, int npairs, int w, int h, const ofdis_track_select_params& p, uint8_t* code,
                               long long* counts, int max_tracks_out, float* tracks_out, int* start_out, int* len_out,
                               long long* info_out, int* index, float* shape_out, void* work, hipStream_t s, int nparam) {
  const TsArgs a{(const float2*)tracks, start, len, info, lmax, max_tracks, models, npairs, nparam, (float)(w - 1) * 0.5f,
                 (float)(h - 1) * 0.5f, p, code, counts, max_tracks_out, (float2*)tracks_out, start_out, len_out, info_out, index,
                 (float2*)shape_out, (TsRecord*)work};
  const int workgroups = (max_tracks + kTsLanes - 1) / kTsLanes;
  hipLaunchKernelGGL(track_select_classify_kernel, dim3((unsigned)workgroups), dim3(kTsLanes), 0, s, a);
  hipLaunchKernelGGL(track_select_scan_kernel, dim3(1), dim3(kTsLanes), 0, s, a, workgroups);
  hipLaunchKernelGGL(track_select_scatter_kernel, dim3((unsigned)workgroups), dim3(kTsLanes), 0, s, a);
  return hipGetLastError();
}

}  // namespace ofdis
