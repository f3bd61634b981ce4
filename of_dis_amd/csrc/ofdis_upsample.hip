// ofdis_upsample.hip -- the full-resolution finish on the level result (run_dense.cpp:406-414): the flow (or stereo
// disparity) x 2^lv_l, cv::resize(INTER_LINEAR) by 2^lv_l, cropped to the original size -- as fp32 or in a compact output
// encoding (include/ofdis.h: ofdis_encoding, ofdis_encode) -- and the forward-backward consistency masks (ofdis_fb_check,
// ofdis_batch_upsample_bidir).  Compiled under the exact contract only (-ffp-contract=off); geometry (UpGeom) and arithmetic
// are those of ofdis_upsample.h, shared with ofdis_interp.hip and ofdis_stereo_lr.hip.
#include "ofdis_kernels.h"
#include "ofdis_upsample.h"

namespace ofdis {

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------ result to full resolution
// ofdis_batch_upsample_frames (<ENC_F32, C>: the bits unchanged) and ofdis_batch_upsample_frames_enc: the values encoded in
// registers (include/ofdis.h: ofdis_encoding) and written once.  The level result (57 KB per frame at op-point 2) is L2
// resident; the output is written once and never read by this library: non-temporal stores.  The kernel is its stores, so a lane
// issues ONE 16-byte store per output row: it owns the NV = 16 / element size adjacent values of a row -- NV / C columns (C = 2:
// 2 / 4 / 8 columns of 4- / 2- / 1-byte elements, C = 1 twice as many) -- interpolates them horizontally on the two source rows
// of a row group (up_group) ONCE and then writes the <= 2^sc_l rows of the group, which differ only in the vertical weight.
// Lanes are numbered over (row group, 16-byte chunk of the row) so that rows shorter than a workgroup's 4 KB leave no lanes
// idle.  `align` = the largest power of two <= 16 that divides both the row's byte length and the address of `out`: below 16
// (odd widths and the like) a lane writes its chunk in pieces of that size.
__device__ __forceinline__ void store_chunk16(uint8_t* o, const unsigned (&w)[4], int nb, int align) {
  if (align >= 16) {  // (then every chunk of a row is whole: nb == 16)
    __builtin_nontemporal_store((u4){w[0], w[1], w[2], w[3]}, reinterpret_cast<u4*>(o));
  } else if (align >= 8) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (8 * i < nb) *reinterpret_cast<uint2*>(o + 8 * i) = make_uint2(w[2 * i], w[2 * i + 1]);
  } else if (align >= 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * i < nb) *reinterpret_cast<unsigned*>(o + 4 * i) = w[i];
  } else if (align >= 2) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (2 * i < nb) *reinterpret_cast<unsigned short*>(o + 2 * i) = (unsigned short)(w[i >> 1] >> (16 * (i & 1)));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < nb) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

template <int TYPE, int C>
__global__ __launch_bounds__(256) void upsample_crop_enc_kernel(const float* __restrict__ flow, uint8_t* __restrict__ out,
                                                                UpGeom g, int chunks, int align, float scale, float offset) {
  constexpr int NV = EncTraits<TYPE>::per16, NCOL = NV / C;
  const int f = blockIdx.y;
  const unsigned id = blockIdx.x * 256u + threadIdx.x;
  const int gi = (int)(id / (unsigned)chunks), ch = (int)(id - (unsigned)gi * (unsigned)chunks);
  if (gi > g.sh) return;
  const int x = ch * NCOL;  // first column of the lane (< wo: chunks = ceil(wo / NCOL))
  const UpGroup grp = up_group(gi, g);
  if (grp.Y0 >= grp.Y1) return;
  const float* fl = flow + (size_t)f * g.plane() * C;
  float r0[NV], r1[NV];  // the lane's values on the two source rows, in memory order
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    const int X = min(x + c, g.wo - 1) + g.left;  // (columns past the row's end repeat the last one; they are not stored)
    if constexpr (C == 2) {
      float2 a0, a1;
      upsample_h(reinterpret_cast<const float2*>(fl), g, grp.sy, grp.sy1, X, a0, a1);
      r0[2 * c] = a0.x; r0[2 * c + 1] = a0.y;
      r1[2 * c] = a1.x; r1[2 * c + 1] = a1.y;
    } else {
      upsample_h(fl, g, grp.sy, grp.sy1, X, r0[c], r1[c]);
    }
  }
  const int row_bytes = g.wo * C * EncTraits<TYPE>::bytes;
  const int nb = min(16, row_bytes - ch * 16);
  for (int Y = grp.Y0; Y < grp.Y1; ++Y) {
    const float fy = grp.fy(Y);
    float v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = up_mix(r0[i], r1[i], fy);
    unsigned w[4];
    enc_pack16<TYPE>(v, scale, offset, w);
    store_chunk16(out + ((size_t)f * g.ho + (Y - g.top)) * row_bytes + (size_t)ch * 16, w, nb, align);
  }
}

// largest power of two <= 16 dividing the address and the byte length of a row
static int store_align(const void* p, size_t row_bytes) {
  const size_t v = (size_t)(uintptr_t)p | row_bytes | 16;
  return (int)(v & (~v + 1));
}

template <int TYPE>
static hipError_t launch_upsample_crop_enc_t(const float* flow, void* out, int nframes, UpGeom g, int channels, float scale,
                                             float offset, hipStream_t s) {
  const int ncol = EncTraits<TYPE>::per16 / channels;
  const int chunks = (g.wo + ncol - 1) / ncol;
  const long long lanes = (long long)chunks * (g.sh + 1);
  const long long row_bytes = (long long)g.wo * channels * EncTraits<TYPE>::bytes;
  if (nframes > 65535 || lanes >= (1ll << 31) || row_bytes >= (1ll << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)nframes);
  const int align = store_align(out, (size_t)row_bytes);
  if (channels == 1)
    hipLaunchKernelGGL((upsample_crop_enc_kernel<TYPE, 1>), grid, dim3(256), 0, s, flow, (uint8_t*)out, g, chunks, align, scale,
                       offset);
  else
    hipLaunchKernelGGL((upsample_crop_enc_kernel<TYPE, 2>), grid, dim3(256), 0, s, flow, (uint8_t*)out, g, chunks, align, scale,
                       offset);
  return hipGetLastError();
}

hipError_t launch_upsample_crop(const float* flow, float* out, int nframes, UpGeom g, int channels, hipStream_t s) {
  if (g.ho > 65535 || nframes > 65535) return hipErrorInvalidValue;
  return launch_upsample_crop_enc_t<ENC_F32>(flow, out, nframes, g, channels, 1.0f, 0.0f, s);
}

hipError_t launch_upsample_crop_enc(const float* flow, void* out, int nframes, UpGeom g, int channels, int type, float scale,
                                    float offset, hipStream_t s) {
  switch (type) {
    case ENC_F32:  // the bits unchanged; two channels: within the limits of ofdis_batch_upsample_frames, as before
      if (channels == 1) return launch_upsample_crop_enc_t<ENC_F32>(flow, out, nframes, g, channels, scale, offset, s);
      return launch_upsample_crop(flow, (float*)out, nframes, g, channels, s);
    case ENC_F16: return launch_upsample_crop_enc_t<ENC_F16>(flow, out, nframes, g, channels, scale, offset, s);
    case ENC_U16: return launch_upsample_crop_enc_t<ENC_U16>(flow, out, nframes, g, channels, scale, offset, s);
    case ENC_U8: return launch_upsample_crop_enc_t<ENC_U8>(flow, out, nframes, g, channels, scale, offset, s);
  }
  return hipErrorInvalidValue;
}

// ofdis_encode on a materialised array: a lane converts the 16 / element size values of one 16-byte store per step (16-byte
// loads), grid-stride; the values past the last whole store -- every value when src or dst is not 16-byte aligned -- one by one.
template <int TYPE>
__global__ __launch_bounds__(256) void encode_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t n,
                                                     size_t nvec, float scale, float offset) {
  constexpr int NV = EncTraits<TYPE>::per16, EB = EncTraits<TYPE>::bytes;
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = t0; i < nvec; i += stride) {
    float v[NV];
#pragma unroll
    for (int q = 0; q < NV / 4; ++q) {
      const f4v t = reinterpret_cast<const f4v*>(src)[i * (NV / 4) + q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    unsigned w[4];
    enc_pack16<TYPE>(v, scale, offset, w);
    reinterpret_cast<u4*>(dst)[i] = (u4){w[0], w[1], w[2], w[3]};
  }
  for (size_t i = nvec * NV + t0; i < n; i += stride) {
    const unsigned q = enc_bits<TYPE>(src[i], scale, offset);
    if constexpr (EB == 4) reinterpret_cast<unsigned*>(dst)[i] = q;
    else if constexpr (EB == 2) reinterpret_cast<unsigned short*>(dst)[i] = (unsigned short)q;
    else dst[i] = (uint8_t)q;
  }
}

template <int TYPE>
static hipError_t launch_encode_t(const float* src, void* dst, size_t n, float scale, float offset, hipStream_t s) {
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const size_t nvec = aligned ? n / EncTraits<TYPE>::per16 : 0;
  const size_t work = nvec > n - nvec * EncTraits<TYPE>::per16 ? nvec : n - nvec * EncTraits<TYPE>::per16;
  hipLaunchKernelGGL(encode_kernel<TYPE>, dim3(grid_for((long long)work)), dim3(256), 0, s, src, (uint8_t*)dst, n, nvec, scale,
                     offset);
  return hipGetLastError();
}

hipError_t launch_encode(const float* src, void* dst, size_t n, int type, float scale, float offset, hipStream_t s) {
  switch (type) {
    case ENC_F32: return launch_encode_t<ENC_F32>(src, dst, n, scale, offset, s);
    case ENC_F16: return launch_encode_t<ENC_F16>(src, dst, n, scale, offset, s);
    case ENC_U16: return launch_encode_t<ENC_U16>(src, dst, n, scale, offset, s);
    case ENC_U8: return launch_encode_t<ENC_U8>(src, dst, n, scale, offset, s);
  }
  return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------ forward-backward consistency
// materialised flows: one pixel per thread, grid-stride over all frames
__global__ __launch_bounds__(256) void fb_check_kernel(const float2* __restrict__ flow, const float2* __restrict__ other,
                                                       uint8_t* __restrict__ mask, long long total, int w, int h,
                                                       float alpha, float beta) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    const long long r = i / w;
    const int y = (int)(r % h);
    const float2* R = other + (i - (long long)y * w - x);  // the frame's first pixel
    const float2 uv = flow[i];
    mask[i] = fb_code(uv.x, uv.y, x, y, w, h, alpha, beta, FlowTaps{R, w});
  }
}

hipError_t launch_fb_check(const float* flow, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                           float beta, hipStream_t s) {
  const long long total = (long long)nframes * w * h;
  hipLaunchKernelGGL(fb_check_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const float2*)flow, (const float2*)other, mask,
                     total, w, h, alpha, beta);
  return hipGetLastError();
}

// Both directions to full resolution and both masks, one pixel per thread (grid = (x chunks of 256, output rows, frames)).
// The masks need the OTHER direction's upsampled flow at the four integer neighbours of a non-integer target: recomputed
// from the level flow (UpNeighbours), so the values are the bits ofdis_batch_upsample_frames writes, instead of read back
// from HBM.  The level flows (57 KB per frame and direction at operating point 2, 2 MB at 1080p) are gathered through the
// caches.
__global__ __launch_bounds__(256) void upsample_bidir_kernel(const float2* __restrict__ fw, const float2* __restrict__ rev,
                                                             float2* __restrict__ out_fw, float2* __restrict__ out_rev,
                                                             uint8_t* __restrict__ mask_fw, uint8_t* __restrict__ mask_rev,
                                                             UpGeom g, float alpha, float beta) {
  const int f = blockIdx.z, y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= g.wo) return;
  const float2* flw[2] = {fw + (size_t)f * g.plane(), rev + (size_t)f * g.plane()};
  const UpRow ry = up_row(y + g.top, g);
  float2 val[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) val[d] = upsample_at(flw[d], g, x + g.left, ry);
  const size_t o = ((size_t)f * g.ho + y) * g.wo + x;
  if (out_fw) __builtin_nontemporal_store((f2v){val[0].x, val[0].y}, reinterpret_cast<f2v*>(out_fw + o));
  if (out_rev) __builtin_nontemporal_store((f2v){val[1].x, val[1].y}, reinterpret_cast<f2v*>(out_rev + o));
  uint8_t* masks[2] = {mask_fw, mask_rev};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    if (!masks[d]) continue;
    masks[d][o] = fb_code(val[d].x, val[d].y, x, y, g.wo, g.ho, alpha, beta, UpNeighbours{flw[1 - d], g});
  }
}

hipError_t launch_upsample_bidir(const float* fw, const float* rev, float* out_fw, float* out_rev, uint8_t* mask_fw,
                                 uint8_t* mask_rev, int nframes, UpGeom g, float alpha, float beta, hipStream_t s) {
  if (g.ho > 65535 || nframes > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(upsample_bidir_kernel, dim3((g.wo + 255) / 256, g.ho, nframes), dim3(256), 0, s, (const float2*)fw,
                     (const float2*)rev, (float2*)out_fw, (float2*)out_rev, mask_fw, mask_rev, g, alpha, beta);
  return hipGetLastError();
}

}  // namespace ofdis
