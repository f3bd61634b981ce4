// ofdis_gmotion.hip -- per-pair global (camera) motion models of a flow field and the motion-compensated flow (include/ofdis.h:
// ofdis_global_motion / ofdis_motion_compensate on materialised arrays, ofdis_batch_global_motion /
// ofdis_batch_motion_compensate straight from the level flows of a context): a translation or 6-parameter affine model per
// pair by trimmed least squares, then the residual flow and an inlier / outlier / invalid label per pixel.
//
// Compiled under the exact contract only (-ffp-contract=off).  The twelve sums of a fit are exact 64-bit integers -- integer
// addition is associative, so the mapping of pixels to lanes, workgroups and slab records cannot change them -- the solve is a
// fixed sequence of separately rounded fp64 operations (the divisions are the compiler's correctly rounded expansion) and the
// residual a fixed sequence of fp32 ones.  The level-flow kernels take flows and codes only from the helpers of
// ofdis_batch_upsample_bidir / _upsample_frames (ofdis_upsample.h: upsample_at, fb_code on UpNeighbours), so they see the
// bits the standalone kernels read from that function's materialised outputs: both routes give the same models and labels.
//
// Accumulate (one launch per round, all pairs): the quad mapping of ofdis_quad.h over the pairs; the lanes past a pair's last
// quad stay for the workgroup's reduction.  A lane's partial sums are reduced over its wavefront by shuffles (64-bit values as
// two halves), over the workgroup's four wavefronts through LDS, and the workgroup writes ONE 96-byte record into its own slab
// slot [pair][block] with plain stores.  No atomics, no flags, no waiting between workgroups: the solve kernel, behind it on
// the stream, sums a pair's records with one wavefront and one lane solves.  The next round's accumulate launch reads that
// model from device memory.
//
// Widths of the partial sums, with |X|, |Y| <= 8191 < 2^13 (OFDIS_GM_MAX_SIDE) and |qu|, |qv| <= 2^20 (OFDIS_GM_MAX_FLOW * 256):
//   per lane (4 pixels)       n <= 4, |SX|, |SY| < 2^15, SXX, |SXY|, SYY < 2^28, |Squ|, |Sqv| <= 2^22: int32;
//                             |SXqu| ... < 2^35: int64 (one product alone needs 34 bits)
//   per workgroup (256 lanes) n <= 2^10, |SX|, |SY| < 2^23, |Squ|, |Sqv| <= 2^30: these five stay int32 through the wavefront
//                             reduction and are widened in LDS; SXX, SXY, SYY < 2^36: widened before the wavefront reduction
//   per pair                  every sum < W^2 * H * 2^20 <= 2^59 (include/ofdis.h): int64 never overflows
//
// The 8-parameter projective models (ofdis_projective_motion, ofdis_projective_compensate and their ofdis_batch_* twins) are the
// same kernels with NP = 8: the record grows to 23 sums (padded to 24) -- the third moments XXX .. YYY, the fourth moments
// XXXX .. YYYY and the right-hand sides R6, R7 of the two quadratic parameters -- and the residual gains the term p*xc, p*yc.
//   per pixel                 |XXX| < 2^39, XXXX < 2^52, |R6|, |R7| < 2^47: int64 per lane
//   per workgroup (1024 px)   fourth moments < 2^62, third < 2^49, |R6|, |R7| < 2^57: int64.  The 23 sums of a lane are reduced
//                             over the wavefront TOGETHER (gm_block_sums: a lane keeps half of its sums and hands the other half
//                             to its partner at every step), 64 lane exchanges where 23 separate reductions take 234
//   per pair                  a fourth moment reaches 2^78 at 8192 x 8192: the solve kernel adds the records of the eleven new
//                             sums in 128 bits (two 64-bit limbs, Wide) and converts each to fp64 correctly rounded
#include "ofdis_upsample.h"

namespace ofdis {

typedef float gm_f4 __attribute__((ext_vector_type(4)));

enum { GM_INLIER = 0, GM_OUTLIER = 1, GM_INVALID = 2 };
enum { GM_NSUMS = 12 };  // n, SX, SY, SXX, SXY, SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv: one slab record
// the projective record: the twelve, XXX, XXY, XYY, YYY, XXXX, XXXY, XXYY, XYYY, YYYY, R6, R7 and one word of padding
enum { PM_NSUMS = 23, PM_RECORD = 24 };
// NP, the parameters of a model, selects the kernels: 6 (translation / affine) or 8 (projective)
template <int NP>
struct GmRecord {
  static constexpr int sums = NP == 8 ? (int)PM_NSUMS : (int)GM_NSUMS, stride = NP == 8 ? (int)PM_RECORD : (int)GM_NSUMS;
};

// what the accumulate and compensate kernels are launched with: the pairs of this launch
struct GmArgs {
  const double* models;  // [npairs][NP]: the previous round's models (gated accumulate), the models to subtract (compensate)
  long long* slab;       // [npairs][bpf][GmRecord<NP>::stride] (accumulate)
  float2* residual;      // [npairs][H][W] or null (compensate)
  uint8_t* label;        // [npairs][H][W] or null (compensate)
  QuadLaunch q;
  float t2;              // thresh * thresh
  int res_align;         // compensate: 16 / 8 / 4-byte stores of the residual
  bool vec_label;        // ... and quad_vec of the labels
};

// the model of a pair in fp32 and the header's residual
template <int NP>
struct GmModel {
  float a[NP];
};
template <int NP>
__device__ __forceinline__ GmModel<NP> gm_model(const double* models, int pair) {
  GmModel<NP> m;
#pragma unroll
  for (int k = 0; k < NP; ++k) m.a[k] = (float)models[(size_t)pair * NP + k];
  return m;
}
template <int NP>
__device__ __forceinline__ float2 gm_residual(const GmModel<NP>& m, int X, int Y, float2 uv) {
  const float xc = (float)X * 0.5f, yc = (float)Y * 0.5f;
  float mu = (m.a[0] + m.a[1] * xc) + m.a[2] * yc;
  float mv = (m.a[3] + m.a[4] * xc) + m.a[5] * yc;
  if constexpr (NP == 8) {
    const float p = m.a[6] * xc + m.a[7] * yc;
    mu = mu + p * xc;
    mv = mv + p * yc;
  }
  return make_float2(uv.x - mu, uv.y - mv);
}
__device__ __forceinline__ bool gm_near(float2 r, float t2) { return r.x * r.x + r.y * r.y <= t2; }  // (NaN: false)
// u and v finite and within OFDIS_GM_MAX_FLOW (NaN: false)
__device__ __forceinline__ bool gm_in_range(float2 uv) { return fabsf(uv.x) <= 4096.0f && fabsf(uv.y) <= 4096.0f; }

__device__ __forceinline__ int gm_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long gm_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), o);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// One round's sums of a workgroup's 256 quads into its slab record.  `flow(xx)` gives the flow at pixel (xx, y) of the lane's
// row, `consistent(xx, uv)` whether the mask there is OFDIS_FB_CONSISTENT (asked only where the flow is in range and, GATED,
// near).  GATED: the set is `near` under the model of the previous round.  Every lane of the workgroup gets here.
template <int NP, bool GATED, class Flow, class Consistent>
__device__ __forceinline__ void gm_block_sums(const GmArgs& a, const QuadLane& l, int W, int H, Flow flow, Consistent consistent) {
  constexpr int NS = GmRecord<NP>::stride;
  __shared__ long long part[4][NS];
  GmModel<NP> m;
  if constexpr (GATED) m = gm_model<NP>(a.models, l.f);
  const int np = l.active ? min(4, W - l.x) : 0;
  const int Y = 2 * l.y - (H - 1);
  int n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0, su = 0, sv = 0;
  long long sxu = 0, syu = 0, sxv = 0, syv = 0;
  long long hi[NP == 8 ? 11 : 1] = {};  // (NP == 8) XXX, XXY, XYY, YYY, XXXX, XXXY, XXYY, XYYY, YYYY, R6, R7
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= np) continue;
    const int xx = l.x + i;
    const float2 uv = flow(xx);
    const int X = 2 * xx - (W - 1);
    bool in = gm_in_range(uv);
    if constexpr (GATED) in = in && gm_near(gm_residual(m, X, Y, uv), a.t2);
    if (!in || !consistent(xx, uv)) continue;  // (the code last: the level-flow kernel computes it only for pixels still in)
    const int qu = (int)rintf(uv.x * 256.0f), qv = (int)rintf(uv.y * 256.0f);
    n += 1; sx += X; sy += Y; sxx += X * X; sxy += X * Y; syy += Y * Y;
    su += qu; sv += qv;
    sxu += (long long)X * qu; syu += (long long)Y * qu;
    sxv += (long long)X * qv; syv += (long long)Y * qv;
    if constexpr (NP == 8) {
      const long long xx = X * X, xy = X * Y, yy = Y * Y;  // (below 2^26: the products below stay inside int64)
      hi[0] += xx * X; hi[1] += xx * Y; hi[2] += yy * X; hi[3] += yy * Y;
      hi[4] += xx * xx; hi[5] += xx * xy; hi[6] += xx * yy; hi[7] += xy * yy; hi[8] += yy * yy;
      hi[9] += xx * qu + xy * qv; hi[10] += xy * qu + yy * qv;
    }
  }
  const int wave = threadIdx.x >> 6;
  if constexpr (NP == 8) {
    // 23 separate wavefront sums would take 23 x 6 exchange steps (this kernel is bound by them, not by HBM).  Here the sums are
    // reduced together, the lanes sharing the work: at every step a lane keeps one half of its sums, hands the other half to
    // its partner and adds what the partner hands over, so 16 + 8 + 4 + 2 + 1 values cross instead of 32 x 5; after five steps
    // lane L holds sum number L >> 1 over its 32 partners and the last step adds the neighbour's.  Integer addition: the same
    // numbers whatever the order.
    long long u[32] = {n, sx, sy, sxx, sxy, syy, su, sxu, syu, sv, sxv, syv, hi[0], hi[1], hi[2], hi[3], hi[4], hi[5], hi[6],
                       hi[7], hi[8], hi[9], hi[10]};  // (24 .. 31: zero)
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 32, half = 16; half >= 1; o >>= 1, half >>= 1) {
      const bool upper = (lane & o) != 0;
#pragma unroll
      for (int j = 0; j < half; ++j) {
        const long long keep = upper ? u[j + half] : u[j], send = upper ? u[j] : u[j + half];
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)send, o);
        const unsigned hi32 = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)send >> 32), o);
        u[j] = keep + (long long)(((unsigned long long)hi32 << 32) | lo);
      }
    }
    {
      const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)u[0], 1);
      const unsigned hi32 = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)u[0] >> 32), 1);
      u[0] += (long long)(((unsigned long long)hi32 << 32) | lo);
    }
    if ((lane & 1) == 0 && (lane >> 1) < NS) part[wave][lane >> 1] = u[0];  // (sum 23, the padding word, is zero)
  } else {
    long long s[NS];
    s[0] = gm_wave_sum(n); s[1] = gm_wave_sum(sx); s[2] = gm_wave_sum(sy);
    s[3] = gm_wave_sum((long long)sxx); s[4] = gm_wave_sum((long long)sxy); s[5] = gm_wave_sum((long long)syy);
    s[6] = gm_wave_sum(su); s[7] = gm_wave_sum(sxu); s[8] = gm_wave_sum(syu);
    s[9] = gm_wave_sum(sv); s[10] = gm_wave_sum(sxv); s[11] = gm_wave_sum(syv);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) part[wave][k] = s[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    a.slab[((size_t)l.f * a.q.bpf + l.blk) * NS + k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
  }
}

// Materialised arrays: flow [npairs][H][W][2], mask [npairs][H][W] or null.
template <int NP, bool GATED>
__global__ __launch_bounds__(256) void gm_sums_frames_kernel(const float2* __restrict__ flow, const uint8_t* __restrict__ mask,
                                                             int W, int H, GmArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, W, H, l)) return;
  const size_t row = ((size_t)l.f * H + l.y) * W;
  const float2* fl = flow + row;
  const uint8_t* mk = mask ? mask + row : nullptr;
  gm_block_sums<NP, GATED>(a, l, W, H, [&](int xx) { return fl[xx]; },
                       [&](int xx, float2) { return !mk || mk[xx] == FB_CONSISTENT; });
}

// A context's level flows (UpGeom): the flow at the quad's pixels as ofdis_batch_upsample_frames writes it and, with `rev`
// (fb_check = 1), the forward code of ofdis_batch_upsample_bidir recomputed as tfilter_level_kernel does.
template <int NP, bool GATED>
__global__ __launch_bounds__(256) void gm_sums_level_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                            UpGeom g, float alpha, float beta, GmArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, g.wo, g.ho, l)) return;
  const float2* fl = fw + (size_t)l.f * g.plane();
  const float2* other = rev ? rev + (size_t)l.f * g.plane() : nullptr;
  const UpRow ry = up_row(l.y + g.top, g);
  gm_block_sums<NP, GATED>(a, l, g.wo, g.ho, [&](int xx) { return upsample_at(fl, g, xx + g.left, ry); },
                       [&](int xx, float2 uv) {
                         return !other ||
                                fb_code(uv.x, uv.y, xx, l.y, g.wo, g.ho, alpha, beta, UpNeighbours{other, g}) == FB_CONSISTENT;
                       });
}

// The header's solve on the twelve sums `s`: the model a[6] and the status.
__device__ __forceinline__ int gm_solve(const long long (&s)[GM_NSUMS], int model, double (&a)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = 0.0;
  if (s[0] == 0) return 2;  // OFDIS_GM_EMPTY
  const double n = (double)s[0], Sx = (double)s[1], Sy = (double)s[2], Sxx = (double)s[3], Sxy = (double)s[4], Syy = (double)s[5];
  const double Su[2] = {(double)s[6], (double)s[9]}, Sxu[2] = {(double)s[7], (double)s[10]}, Syu[2] = {(double)s[8], (double)s[11]};
  if (model == 1 && s[0] >= 3) {
    const double c00 = Sxx * Syy - Sxy * Sxy;
    const double c01 = Sxy * Sy - Sx * Syy;
    const double c02 = Sx * Sxy - Sxx * Sy;
    const double c11 = n * Syy - Sy * Sy;
    const double c12 = Sx * Sy - n * Sxy;
    const double c22 = n * Sxx - Sx * Sx;
    const double det = (n * c00 + Sx * c01) + Sy * c02;
    if (det > 0.0) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const double b0 = ((c00 * Su[c] + c01 * Sxu[c]) + c02 * Syu[c]) / det;
        const double b1 = ((c01 * Su[c] + c11 * Sxu[c]) + c12 * Syu[c]) / det;
        const double b2 = ((c02 * Su[c] + c12 * Sxu[c]) + c22 * Syu[c]) / det;
        a[3 * c] = b0 / 256.0;
        a[3 * c + 1] = b1 / 128.0;
        a[3 * c + 2] = b2 / 128.0;
      }
      return 0;  // OFDIS_GM_OK_AFFINE
    }
  }
  a[0] = (Su[0] / n) / 256.0;
  a[3] = (Su[1] / n) / 256.0;
  return 1;  // OFDIS_GM_TRANSLATION
}

// One wavefront per pair: the pair's slab records summed (lanes stride over the records, then the wavefront reduction), lane 0
// solves and writes.  ROUND0 writes always (an empty set: the zero model, OFDIS_GM_EMPTY); a later round with an empty set
// leaves the previous round's model, set size and status as they are.
template <bool ROUND0>
__global__ __launch_bounds__(64) void gm_solve_kernel(const long long* __restrict__ slab, int bpf, int model,
                                                      double* __restrict__ models, long long* __restrict__ stats) {
  const int pair = blockIdx.x;
  const long long* rec = slab + (size_t)pair * bpf * GM_NSUMS;
  long long s[GM_NSUMS];
#pragma unroll
  for (int k = 0; k < GM_NSUMS; ++k) s[k] = 0;
  for (int r = threadIdx.x; r < bpf; r += 64) {
#pragma unroll
    for (int k = 0; k < GM_NSUMS; ++k) s[k] += rec[(size_t)r * GM_NSUMS + k];
  }
#pragma unroll
  for (int k = 0; k < GM_NSUMS; ++k) s[k] = gm_wave_sum(s[k]);
  if (threadIdx.x != 0) return;
  if (!ROUND0 && s[0] == 0) return;
  double a[6];
  const int status = gm_solve(s, model, a);
#pragma unroll
  for (int k = 0; k < 6; ++k) models[(size_t)pair * 6 + k] = a[k];
  if (!stats) return;
  if (ROUND0) stats[(size_t)pair * 3] = s[0];
  stats[(size_t)pair * 3 + 1] = s[0];
  stats[(size_t)pair * 3 + 2] = status;
}

// ------------------------------------------------------------------------------------ projective solve
// A signed 128-bit sum in two limbs (two's complement): a pair's third and fourth moments and R6, R7 do not fit 64 bits.
struct Wide {
  unsigned long long lo;
  long long hi;
};
__device__ __forceinline__ Wide wide_add(Wide a, Wide b) {
  Wide r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (long long)(r.lo < a.lo);
  return r;
}
__device__ __forceinline__ Wide wide_of(long long v) { return Wide{(unsigned long long)v, v < 0 ? -1ll : 0ll}; }
__device__ __forceinline__ Wide gm_wave_sum(Wide v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Wide w;
    const unsigned l0 = (unsigned)__shfl_xor((int)(unsigned)v.lo, o), l1 = (unsigned)__shfl_xor((int)(unsigned)(v.lo >> 32), o);
    const unsigned h0 = (unsigned)__shfl_xor((int)(unsigned)v.hi, o);
    const unsigned h1 = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v.hi >> 32), o);
    w.lo = ((unsigned long long)l1 << 32) | l0;
    w.hi = (long long)(((unsigned long long)h1 << 32) | h0);
    v = wide_add(v, w);
  }
  return v;
}
// The nearest double (ties to even) of a sum below 2^127 in magnitude: the magnitude shifted right until 64 bits remain, what
// was shifted out kept as a sticky bit 0 (far below the rounding position of a 64-bit value whose top bit is set), one
// u64 -> f64 conversion -- the only rounding -- and an exact scaling by the power of two.
__device__ __forceinline__ double wide_to_double(Wide v) {
  const bool neg = v.hi < 0;
  unsigned long long lo = v.lo, hi = (unsigned long long)v.hi;
  if (neg) {
    lo = ~lo + 1ull;
    hi = ~hi + (unsigned long long)(lo == 0ull);
  }
  double d;
  if (hi == 0ull) {
    d = (double)lo;
  } else {
    const int sh = 64 - __clzll((long long)hi);  // 1 .. 63
    unsigned long long m = (hi << (64 - sh)) | (lo >> sh);
    if (lo & ((1ull << sh) - 1ull)) m |= 1ull;
    d = (double)m * __longlong_as_double((long long)(1023 + sh) << 52);
  }
  return neg ? -d : d;
}

// The header's 8-parameter solve: `s` the twelve sums, `w` the eleven wide ones as doubles (XXX, XXY, XYY, YYY, XXXX, XXXY,
// XXYY, XYYY, YYYY, R6, R7).  Returns the number of parameters solved, 8, 6, 2 or 0.  LDL^T, column by column; every index
// below is a constant after unrolling, so that the factor stays in registers.
__device__ __forceinline__ int pm_solve(const long long (&s)[GM_NSUMS], const double (&w)[11], double (&a)[8]) {
  double N[8][8], t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) N[i][j] = 0.0;
  const double M[3][3] = {{(double)s[0], (double)s[1], (double)s[2]},
                          {(double)s[1], (double)s[3], (double)s[4]},
                          {(double)s[2], (double)s[4], (double)s[5]}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) N[i][j] = N[3 + i][3 + j] = M[i][j];
  const double col6[6] = {M[1][1], w[0], w[1], M[1][2], w[1], w[2]}, col7[6] = {M[1][2], w[1], w[2], M[2][2], w[2], w[3]};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    N[6][i] = col6[i];  // (the factorisation reads the lower triangle only)
    N[7][i] = col7[i];
  }
  N[6][6] = w[4] + w[6];
  N[7][6] = w[5] + w[7];
  N[7][7] = w[6] + w[8];
#pragma unroll
  for (int k = 0; k < 6; ++k) t[k] = (double)s[6 + k];
  t[6] = w[9];
  t[7] = w[10];
  double C[8][8], L[8][8], d[8];
  bool ok = s[0] >= 4;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int i = k; i < 8; ++i) {
      double acc = N[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) acc = acc - C[i][j] * L[k][j];
      C[i][k] = acc;
    }
    d[k] = C[k][k];
    ok = ok && d[k] > N[k][k] * 0x1p-40;
#pragma unroll
    for (int i = k + 1; i < 8; ++i) L[i][k] = C[i][k] / d[k];
  }
  // both branches are computed and the result selected (a failed factorisation holds infinities or NaNs that nothing reads):
  // the eight results stay in registers
  double z[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    z[i] = t[i];
#pragma unroll
    for (int j = 0; j < i; ++j) z[i] = z[i] - L[i][j] * z[j];
  }
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    b[i] = z[i] / d[i];
#pragma unroll
    for (int j = i + 1; j < 8; ++j) b[i] = b[i] - L[j][i] * b[j];
  }
  const double scale[8] = {256.0, 128.0, 128.0, 256.0, 128.0, 128.0, 64.0, 64.0};
  double a6[6];
  const int status = gm_solve(s, 1, a6);  // OFDIS_GM_AFFINE: affine, translation or empty
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p = b[k] / scale[k];
    a[k] = ok ? p : (k < 6 ? a6[k] : 0.0);
  }
  return ok ? 8 : (status == 0 ? 6 : (status == 1 ? 2 : 0));
}

// gm_solve_kernel for the projective record: the twelve sums in 64 bits, the eleven new ones in 128.
template <bool ROUND0>
__global__ __launch_bounds__(64) void pm_solve_kernel(const long long* __restrict__ slab, int bpf, double* __restrict__ models,
                                                      long long* __restrict__ stats) {
  const int pair = blockIdx.x;
  const long long* rec = slab + (size_t)pair * bpf * PM_RECORD;
  long long s[GM_NSUMS];
  Wide ws[11];
#pragma unroll
  for (int k = 0; k < GM_NSUMS; ++k) s[k] = 0;
#pragma unroll
  for (int k = 0; k < 11; ++k) ws[k] = Wide{0ull, 0ll};
  for (int r = threadIdx.x; r < bpf; r += 64) {
#pragma unroll
    for (int k = 0; k < GM_NSUMS; ++k) s[k] += rec[(size_t)r * PM_RECORD + k];
#pragma unroll
    for (int k = 0; k < 11; ++k) ws[k] = wide_add(ws[k], wide_of(rec[(size_t)r * PM_RECORD + GM_NSUMS + k]));
  }
#pragma unroll
  for (int k = 0; k < GM_NSUMS; ++k) s[k] = gm_wave_sum(s[k]);
#pragma unroll
  for (int k = 0; k < 11; ++k) ws[k] = gm_wave_sum(ws[k]);
  if (threadIdx.x != 0) return;
  if (!ROUND0 && s[0] == 0) return;
  double w[11], a[8];
#pragma unroll
  for (int k = 0; k < 11; ++k) w[k] = wide_to_double(ws[k]);
  const int count = pm_solve(s, w, a);
#pragma unroll
  for (int k = 0; k < 8; ++k) models[(size_t)pair * 8 + k] = a[k];
  if (!stats) return;
  if (ROUND0) stats[(size_t)pair * 3] = s[0];
  stats[(size_t)pair * 3 + 1] = s[0];
  stats[(size_t)pair * 3 + 2] = count;
}

// ------------------------------------------------------------------------------------ compensate
// The quad's residuals and labels.  The residual may alias the flow: a lane reads its own four pixels before it writes them.
template <int NP, class Flow, class Consistent>
__device__ __forceinline__ void gm_compensate_quad(const GmArgs& a, const QuadLane& l, int W, int H, Flow flow, Consistent consistent) {
  const GmModel<NP> m = gm_model<NP>(a.models, l.f);
  const int np = min(4, W - l.x);
  const int Y = 2 * l.y - (H - 1);
  float2 r[4];
  uint8_t lab[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = make_float2(0.0f, 0.0f);
    lab[i] = GM_INVALID;
    if (i >= np) continue;
    const int xx = l.x + i;
    const float2 uv = flow(xx);
    r[i] = gm_residual(m, 2 * xx - (W - 1), Y, uv);
    if (gm_in_range(uv) && consistent(xx, uv)) lab[i] = gm_near(r[i], a.t2) ? GM_INLIER : GM_OUTLIER;
  }
  const size_t px0 = ((size_t)l.f * H + l.y) * W + l.x;  // the quad's first pixel in a [pairs][H][W] array
  if (a.residual) {
    float2* o = a.residual + px0;
    if (a.res_align >= 16) {  // (W even and the array 16-byte aligned: pixels px0, px0 + 2 start a 16-byte unit)
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        if (i + 1 < np) __builtin_nontemporal_store((gm_f4){r[i].x, r[i].y, r[i + 1].x, r[i + 1].y}, reinterpret_cast<gm_f4*>(o + i));
        else if (i < np) o[i] = r[i];
      }
    } else if (a.res_align >= 8) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < np) o[i] = r[i];
    } else {
      float* of = reinterpret_cast<float*>(o);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < np) { of[2 * i] = r[i].x; of[2 * i + 1] = r[i].y; }
    }
  }
  if (a.label) quad_store<1>(a.label + px0, lab, np, a.vec_label);
}

// (no __restrict__ on the flow: the residual may be the same array)
template <int NP>
__global__ __launch_bounds__(256) void gm_compensate_frames_kernel(const float2* flow, const uint8_t* __restrict__ mask, int W, int H,
                                                                   GmArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, W, H, l) || !l.active) return;
  const size_t row = ((size_t)l.f * H + l.y) * W;
  const float2* fl = flow + row;
  const uint8_t* mk = mask ? mask + row : nullptr;
  gm_compensate_quad<NP>(a, l, W, H, [&](int xx) { return fl[xx]; }, [&](int xx, float2) { return !mk || mk[xx] == FB_CONSISTENT; });
}

template <int NP>
__global__ __launch_bounds__(256) void gm_compensate_level_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                                  UpGeom g, float alpha, float beta, GmArgs a) {
  QuadLane l;
  if (!quad_lane(a.q, g.wo, g.ho, l) || !l.active) return;
  const float2* fl = fw + (size_t)l.f * g.plane();
  const float2* other = rev ? rev + (size_t)l.f * g.plane() : nullptr;
  const UpRow ry = up_row(l.y + g.top, g);
  gm_compensate_quad<NP>(a, l, g.wo, g.ho, [&](int xx) { return upsample_at(fl, g, xx + g.left, ry); },
                     [&](int xx, float2 uv) {
                       return !other ||
                              fb_code(uv.x, uv.y, xx, l.y, g.wo, g.ho, alpha, beta, UpNeighbours{other, g}) == FB_CONSISTENT;
                     });
}

// ------------------------------------------------------------------------------------ launchers
size_t gmotion_work_bytes(int npairs, int w, int h) {
  return (size_t)npairs * quad_grid(npairs, w, h).bpf * GM_NSUMS * sizeof(long long);
}
size_t projective_work_bytes(int npairs, int w, int h) {
  return (size_t)npairs * quad_grid(npairs, w, h).bpf * PM_RECORD * sizeof(long long);
}

// the launches of one pass over all pairs: `launch(GmArgs, blocks)` once per chunk of pairs
template <class Launch>
static hipError_t gm_chunks(GmArgs a, int npairs, int w, int h, Launch launch) {
  return quad_chunks(npairs, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    a.q = q;
    launch(a, blocks);
    return hipGetLastError();
  });
}

// `rounds` times (accumulate, solve) on the stream; `sums(gated, GmArgs, blocks)` launches one accumulate kernel.  NP = 8: the
// projective solve (`model` is not looked at)
template <int NP, class Sums>
static hipError_t gm_rounds(int npairs, int w, int h, int model, int rounds, float thresh, double* models, long long* stats,
                            void* work, hipStream_t s, Sums sums) {
  GmArgs a{};
  a.models = models;
  a.slab = (long long*)work;
  a.t2 = thresh * thresh;
  const int bpf = quad_grid(npairs, w, h).bpf;
  for (int r = 0; r < rounds; ++r) {
    const bool gated = r > 0;
    hipError_t e = gm_chunks(a, npairs, w, h, [&](const GmArgs& c, dim3 blocks) { sums(gated, c, blocks); });
    if (e != hipSuccess) return e;
    if constexpr (NP == 8) {
      if (gated)
        hipLaunchKernelGGL(pm_solve_kernel<false>, dim3(npairs), dim3(64), 0, s, (const long long*)work, bpf, models, stats);
      else
        hipLaunchKernelGGL(pm_solve_kernel<true>, dim3(npairs), dim3(64), 0, s, (const long long*)work, bpf, models, stats);
    } else {
      if (gated)
        hipLaunchKernelGGL(gm_solve_kernel<false>, dim3(npairs), dim3(64), 0, s, (const long long*)work, bpf, model, models, stats);
      else
        hipLaunchKernelGGL(gm_solve_kernel<true>, dim3(npairs), dim3(64), 0, s, (const long long*)work, bpf, model, models, stats);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int NP>
static hipError_t gm_fit_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int model, int rounds,
                                float thresh, double* models, long long* stats, void* work, hipStream_t s) {
  const float2* fl = (const float2*)flow;
  return gm_rounds<NP>(npairs, w, h, model, rounds, thresh, models, stats, work, s, [&](bool gated, const GmArgs& a, dim3 blocks) {
    if (gated)
      hipLaunchKernelGGL((gm_sums_frames_kernel<NP, true>), blocks, dim3(256), 0, s, fl, mask, w, h, a);
    else
      hipLaunchKernelGGL((gm_sums_frames_kernel<NP, false>), blocks, dim3(256), 0, s, fl, mask, w, h, a);
  });
}
hipError_t launch_gmotion_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int model, int rounds,
                                 float thresh, double* models, long long* stats, void* work, hipStream_t s) {
  return gm_fit_frames<6>(flow, mask, npairs, w, h, model, rounds, thresh, models, stats, work, s);
}
hipError_t launch_projective_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int rounds, float thresh,
                                    double* models, long long* stats, void* work, hipStream_t s) {
  return gm_fit_frames<8>(flow, mask, npairs, w, h, 1, rounds, thresh, models, stats, work, s);
}

template <int NP>
static hipError_t gm_fit_level(const float* fw, const float* rev, int npairs, UpGeom ug, int model, int rounds, float thresh,
                               float alpha, float beta, double* models, long long* stats, void* work, hipStream_t s) {
  const float2 *ff = (const float2*)fw, *fr = (const float2*)rev;
  return gm_rounds<NP>(npairs, ug.wo, ug.ho, model, rounds, thresh, models, stats, work, s,
                       [&](bool gated, const GmArgs& a, dim3 blocks) {
                         if (gated)
                           hipLaunchKernelGGL((gm_sums_level_kernel<NP, true>), blocks, dim3(256), 0, s, ff, fr, ug, alpha, beta, a);
                         else
                           hipLaunchKernelGGL((gm_sums_level_kernel<NP, false>), blocks, dim3(256), 0, s, ff, fr, ug, alpha, beta, a);
                       });
}
hipError_t launch_gmotion_level(const float* fw, const float* rev, int npairs, UpGeom ug, int model, int rounds, float thresh,
                                float alpha, float beta, double* models, long long* stats, void* work, hipStream_t s) {
  return gm_fit_level<6>(fw, rev, npairs, ug, model, rounds, thresh, alpha, beta, models, stats, work, s);
}
hipError_t launch_projective_level(const float* fw, const float* rev, int npairs, UpGeom ug, int rounds, float thresh, float alpha,
                                   float beta, double* models, long long* stats, void* work, hipStream_t s) {
  return gm_fit_level<8>(fw, rev, npairs, ug, 1, rounds, thresh, alpha, beta, models, stats, work, s);
}

// the compensate kernels' store widths: see GmArgs
static GmArgs gm_compensate_args(const double* models, float thresh, float* residual, uint8_t* label, int w) {
  GmArgs a{};
  a.models = models;
  a.residual = (float2*)residual;
  a.label = label;
  a.t2 = thresh * thresh;
  const uintptr_t ra = (uintptr_t)residual;
  a.res_align = (w & 1) == 0 && (ra & 15) == 0 ? 16 : ((ra & 7) == 0 ? 8 : 4);
  a.vec_label = quad_vec(w, label);
  return a;
}

template <int NP>
static hipError_t gm_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w, int h,
                                       float thresh, float* residual, uint8_t* label, hipStream_t s) {
  return gm_chunks(gm_compensate_args(models, thresh, residual, label, w), npairs, w, h, [&](const GmArgs& a, dim3 blocks) {
    hipLaunchKernelGGL(gm_compensate_frames_kernel<NP>, blocks, dim3(256), 0, s, (const float2*)flow, mask, w, h, a);
  });
}
hipError_t launch_gmotion_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w, int h,
                                            float thresh, float* residual, uint8_t* label, hipStream_t s) {
  return gm_compensate_frames<6>(flow, mask, models, npairs, w, h, thresh, residual, label, s);
}
hipError_t launch_projective_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w,
                                               int h, float thresh, float* residual, uint8_t* label, hipStream_t s) {
  return gm_compensate_frames<8>(flow, mask, models, npairs, w, h, thresh, residual, label, s);
}

template <int NP>
static hipError_t gm_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UpGeom ug, float thresh,
                                      float alpha, float beta, float* residual, uint8_t* label, hipStream_t s) {
  return gm_chunks(gm_compensate_args(models, thresh, residual, label, ug.wo), npairs, ug.wo, ug.ho,
                   [&](const GmArgs& a, dim3 blocks) {
                     hipLaunchKernelGGL(gm_compensate_level_kernel<NP>, blocks, dim3(256), 0, s, (const float2*)fw,
                                        (const float2*)rev, ug, alpha, beta, a);
                   });
}
hipError_t launch_gmotion_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UpGeom ug,
                                           float thresh, float alpha, float beta, float* residual, uint8_t* label, hipStream_t s) {
  return gm_compensate_level<6>(fw, rev, models, npairs, ug, thresh, alpha, beta, residual, label, s);
}
hipError_t launch_projective_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UpGeom ug,
                                              float thresh, float alpha, float beta, float* residual, uint8_t* label, hipStream_t s) {
  return gm_compensate_level<8>(fw, rev, models, npairs, ug, thresh, alpha, beta, residual, label, s);
}

}  // namespace ofdis
