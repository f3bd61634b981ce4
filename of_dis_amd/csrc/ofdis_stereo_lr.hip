// ofdis_stereo_lr.hip -- the stereo left-right step of include/ofdis.h: the 8-bit mirror that feeds the mirror pass's pyramid,
// the left-right consistency test (ofdis_lr_check), the occlusion fill (ofdis_disparity_fill) and the fused finish of an
// OFDIS_BATCH_STEREO_LR context (ofdis_batch_upsample_lr).  Compiled under the exact contract only (-ffp-contract=off), like
// ofdis_upsample.hip and ofdis_interp.hip: masks and filled disparities are fixed functions of their inputs.
//
// In stereo everything is row-local: the consistency test of a pixel reads the other view along its own row, and the fill takes
// the nearest consistent pixels of the row.  Every row kernel here gives a row to ONE wavefront, which walks it in chunks of 64
// columns (lane i at column 64 c + i); the nearest-consistent-neighbour search is a bit search in the chunk's ballot plus a
// wavefront-uniform carry from chunk to chunk (ofdis_lr.h).
#include <algorithm>

#include "ofdis_kernels.h"
#include "ofdis_lr.h"

namespace ofdis {

// mir(I)[y][x] = I[y][W-1-x], all channels of a pixel together, for [n][h][w][noc] 8-bit frames
__global__ __launch_bounds__(256) void mirror_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long total,
                                                        int w, int noc) {
  const int rowb = w * noc;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(i % rowb);
    const int x = e / noc, c = e - x * noc;
    dst[i] = src[i - e + (w - 1 - x) * noc + c];
  }
}
hipError_t launch_mirror_u8(const uint8_t* src, uint8_t* dst, int nframes, int w, int h, int noc, hipStream_t s) {
  const long long total = (long long)nframes * h * w * noc;
  hipLaunchKernelGGL(mirror_u8_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, dst, total, w, noc);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ ofdis_lr_check
__global__ __launch_bounds__(256) void lr_check_kernel(const float* __restrict__ disp, const float* __restrict__ other,
                                                       uint8_t* __restrict__ mask, long long total, int w, float alpha,
                                                       float beta) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    const float* R = other + (i - x);  // the row's first pixel
    mask[i] = lr_code(disp[i], x, w, alpha, beta, [&](int xx) { return R[xx]; });
  }
}
hipError_t launch_lr_check(const float* disp, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                           float beta, hipStream_t s) {
  const long long total = (long long)nframes * w * h;
  hipLaunchKernelGGL(lr_check_kernel, dim3(grid_for(total)), dim3(256), 0, s, disp, other, mask, total, w, alpha, beta);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ ofdis_disparity_fill
// OFDIS_FILL_NONE / OFDIS_FILL_INVALIDATE: one pixel per thread
__global__ __launch_bounds__(256) void fill_pixelwise_kernel(const float* disp, const uint8_t* __restrict__ mask, float* out,
                                                             long long total, int invalidate) {  // (out may be disp)
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float d = disp[i];
    out[i] = (invalidate && mask[i] != FB_CONSISTENT) ? INFINITY : d;
  }
}
// OFDIS_FILL_BACKGROUND on materialised arrays of any width: one wavefront per row, two walks.  Left to right, a flagged pixel
// takes the value of its nearest consistent pixel on the left (its own where there is none); right to left, it compares that
// with the nearest consistent pixel on the right.  Only flagged pixels are ever changed and only consistent ones are looked up,
// and a lane re-reads only what it wrote itself, so `out` may be `disp`.  (Not __restrict__: they may alias.)
__global__ __launch_bounds__(256) void fill_background_kernel(const float* disp, const uint8_t* __restrict__ mask, float* out,
                                                              long long rows, int w) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (whole wavefronts: a row belongs to one)
  const float* d = disp + row * w;
  const uint8_t* mk = mask + row * w;
  float* o = out + row * w;
  const int nchunks = (w + 63) / 64;
  int carry = -1, first = -1;
  for (int c = 0; c < nchunks; ++c) {
    const int base = c * 64, x = base + lane;
    const bool in = x < w;
    const bool cons = in && mk[x] == FB_CONSISTENT;
    const unsigned long long m = __ballot(cons);
    if (in) {
      const float v = d[x];
      const int l = cons ? x : scan_left(m, lane, base, carry);
      o[x] = l >= 0 ? d[l] : v;
    }
    if (first < 0 && m) first = base + __builtin_ctzll(m);
    carry = carry_left(m, base, carry);
  }
  if (first < 0) return;  // no consistent pixel in the row: out = disp, written above
  carry = -1;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int base = c * 64, x = base + lane;
    const bool in = x < w;
    const bool cons = in && mk[x] == FB_CONSISTENT;
    const unsigned long long m = __ballot(cons);
    if (in && !cons) {
      const int r = scan_right(m, lane, base, carry);
      if (r >= 0) {
        const float dr = d[r];
        o[x] = first < x ? fill_pick(o[x], dr) : dr;  // (o[x]: the left candidate, this lane's own write)
      }
    }
    carry = carry_right(m, base, carry);
  }
}
hipError_t launch_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int w, int h, int mode,
                                 hipStream_t s) {
  const long long total = (long long)nframes * w * h, rows = (long long)nframes * h;
  if (mode == OFDIS_FILL_BACKGROUND) {
    if ((rows + 3) / 4 > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_background_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, disp, mask, out, rows, w);
  } else {
    if (mode == OFDIS_FILL_NONE && out == disp) return hipSuccess;
    hipLaunchKernelGGL(fill_pixelwise_kernel, dim3(grid_for(total)), dim3(256), 0, s, disp, mask, out, total,
                       mode == OFDIS_FILL_INVALIDATE ? 1 : 0);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ ofdis_batch_upsample_lr
// The fused finish.  A workgroup of `rows` wavefronts (1 .. 4) takes `rows` output rows of one frame, a wavefront per row.  Per
// row in LDS: U (the forward disparity at full resolution, what ofdis_batch_upsample_frames writes), DR (the mirror pass's, negated
// and un-mirrored), the 64-bit ballots of "consistent" per chunk and view, and the left carries per chunk and view:
//     8 wo + 1536 bytes per row  (LR_ROW_EXTRA floats beside the two rows), dynamic; at most 64 KB per workgroup.
//   1  both rows from the level disparities (four cached loads per value)
//   2  left to right: both views' codes from LDS, masks out; without OFDIS_FILL_BACKGROUND the disparities go out here too
//   3  OFDIS_FILL_BACKGROUND, right to left: nearest consistent neighbours from the ballots and carries, disparities out
// Every output byte is written once; nothing is read back from HBM.
constexpr int LR_MAX_CHUNKS = 64;                      // 64 columns each: widths up to LR_FUSED_MAX_WIDTH
constexpr int LR_ROW_EXTRA = 2 * LR_MAX_CHUNKS * 3;    // floats: ballots (two floats each) and carries of two views
constexpr int LR_FUSED_MAX_WIDTH = 64 * LR_MAX_CHUNKS;
static_assert(LR_FUSED_MAX_WIDTH == OFDIS_LR_FUSED_MAX_WIDTH, "the limit include/ofdis.h states");
typedef unsigned long long u64;

__global__ __launch_bounds__(256) void upsample_lr_kernel(const float* __restrict__ fw, const float* __restrict__ mir,
                                                          float* __restrict__ out_l, float* __restrict__ out_r,
                                                          uint8_t* __restrict__ mask_l, uint8_t* __restrict__ mask_r, UpGeom g,
                                                          int fill_mode, float alpha, float beta) {
  const int wo = g.wo, ho = g.ho;
  extern __shared__ __attribute__((aligned(16))) float lr_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int f = blockIdx.y;
  const int yrow = blockIdx.x * (blockDim.x >> 6) + wv;
  const bool live = yrow < ho;       // (a dead wavefront keeps walking -- the barriers are workgroup-wide -- and stores nothing)
  const int y = live ? yrow : ho - 1;
  float* row[2];
  row[0] = lr_lds + (size_t)wv * (2 * wo + LR_ROW_EXTRA);
  row[1] = row[0] + wo;
  u64* mb = reinterpret_cast<u64*>(row[1] + wo);  // [2][LR_MAX_CHUNKS]   (wo floats twice: 8-byte aligned)
  int* cl = reinterpret_cast<int*>(mb + 2 * LR_MAX_CHUNKS);  // [2][LR_MAX_CHUNKS]
  const float* flw = fw + (size_t)f * g.plane();
  const float* flm = mir + (size_t)f * g.plane();
  const UpRow ry = up_row(y + g.top, g);
  for (int x = lane; x < wo; x += 64) {
    row[0][x] = upsample_at(flw, g, x + g.left, ry);
    row[1][x] = -upsample_at(flm, g, (wo - 1 - x) + g.left, ry);
  }
  __syncthreads();
  float* outs[2] = {out_l, out_r};
  uint8_t* masks[2] = {mask_l, mask_r};
  const size_t o0 = ((size_t)f * ho + y) * wo;
  const int nchunks = (wo + 63) / 64;
  const bool background = fill_mode == OFDIS_FILL_BACKGROUND;
  int carry[2] = {-1, -1};
  for (int c = 0; c < nchunks; ++c) {
    const int base = c * 64, x = base + lane;
    const bool in = x < wo;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const float* oth = row[1 - v];
      const float d = in ? row[v][x] : 0.0f;
      const uint8_t code = in ? lr_code(d, x, wo, alpha, beta, [&](int xx) { return oth[xx]; }) : (uint8_t)FB_INCONSISTENT;
      if (live && in) {
        if (masks[v]) masks[v][o0 + x] = code;
        if (!background && outs[v])
          __builtin_nontemporal_store((fill_mode == OFDIS_FILL_INVALIDATE && code != FB_CONSISTENT) ? INFINITY : d,
                                      outs[v] + o0 + x);
      }
      if (background) {
        const u64 m = __ballot(in && code == FB_CONSISTENT);
        if (lane == 0) { mb[v * LR_MAX_CHUNKS + c] = m; cl[v * LR_MAX_CHUNKS + c] = carry[v]; }
        carry[v] = carry_left(m, base, carry[v]);
      }
    }
  }
  if (!background) return;
  __syncthreads();
  carry[0] = carry[1] = -1;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int base = c * 64, x = base + lane;
    const bool in = x < wo;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const u64 m = mb[v * LR_MAX_CHUNKS + c];
      if (in && live && outs[v]) {
        const float* r = row[v];
        float d = r[x];
        if (!((m >> lane) & 1ull))
          d = fill_background(d, scan_left(m, lane, base, cl[v * LR_MAX_CHUNKS + c]), scan_right(m, lane, base, carry[v]),
                              [&](int xx) { return r[xx]; });
        __builtin_nontemporal_store(d, outs[v] + o0 + x);
      }
      carry[v] = carry_right(m, base, carry[v]);
    }
  }
}

bool upsample_lr_fuses(int wo) { return wo <= LR_FUSED_MAX_WIDTH; }
size_t upsample_lr_row_bytes(int wo) { return ((size_t)2 * wo + LR_ROW_EXTRA) * sizeof(float); }
hipError_t launch_upsample_lr(const float* fw, const float* mir, float* out_l, float* out_r, uint8_t* mask_l, uint8_t* mask_r,
                              int nframes, UpGeom g, int fill_mode, float alpha, float beta, hipStream_t s) {
  if (!upsample_lr_fuses(g.wo) || nframes > 65535) return hipErrorInvalidValue;
  const size_t per_row = upsample_lr_row_bytes(g.wo);
  const int rows = (int)std::min<size_t>(4, (64 * 1024) / per_row);  // >= 1 up to LR_FUSED_MAX_WIDTH
  hipLaunchKernelGGL(upsample_lr_kernel, dim3((g.ho + rows - 1) / rows, nframes), dim3(64 * rows), rows * per_row, s, fw, mir,
                     out_l, out_r, mask_l, mask_r, g, fill_mode, alpha, beta);
  return hipGetLastError();
}

// The composition's first step for widths above LR_FUSED_MAX_WIDTH: U and DR materialised, one pixel per thread
__global__ __launch_bounds__(256) void lr_materialise_kernel(const float* __restrict__ fw, const float* __restrict__ mir,
                                                             float* __restrict__ u, float* __restrict__ dr, UpGeom g) {
  const int f = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= g.wo) return;
  const size_t o = ((size_t)f * g.ho + y) * g.wo + x;
  u[o] = upsample_at(fw + (size_t)f * g.plane(), g, x + g.left, y + g.top);
  dr[o] = -upsample_at(mir + (size_t)f * g.plane(), g, (g.wo - 1 - x) + g.left, y + g.top);
}
hipError_t launch_lr_materialise(const float* fw, const float* mir, float* u, float* dr, int nframes, UpGeom g, hipStream_t s) {
  if (g.ho > 65535 || nframes > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lr_materialise_kernel, dim3((g.wo + 255) / 256, g.ho, nframes), dim3(256), 0, s, fw, mir, u, dr, g);
  return hipGetLastError();
}

}  // namespace ofdis
