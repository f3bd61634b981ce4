// ofdis_descriptors.hip -- trajectory-aligned descriptors of dense tracks (include/ofdis.h: ofdis_track_descriptors): the
// histograms of gradient orientation (HOG), flow orientation (HOF) and motion boundaries (MBHx, MBHy) in the space-time tube
// around every track, and the track's normalised displacements (Wang, Klaeser, Schmid and Liu, "Dense trajectories and motion
// boundary descriptors", 2013).
//
// Compiled under the exact contract only (-ffp-contract=off): every fp32 operation of a feature is separately rounded, and a
// histogram entry is a sum of integers, so the bits depend neither on the mapping below nor on the order of the sums.
//
// Mapping.  One wavefront (one workgroup) per slot walks the steps of its track in order.  The lanes are tied to the spatial
// cells: with nxy^2 cells, cell c owns the lanes [c L, (c + 1) L), L = 64 / nxy^2 (64, 16, 7, 4; with nxy = 3 one lane idles),
// and lane s of a cell takes the cell's pixels s, s + L, s + 2 L, ... in row order -- for the cells of 16 pixels a side of
// N 32, nxy 2 a row of a cell per 16 lanes.  Every lane accumulates into a histogram of its own in LDS, laid out [bin][lane]:
// 33 bins (8 HOG, 9 HOF, 8 MBHx, 8 MBHy) x 64 lanes x 4 bytes = 8448 bytes, lane l only ever touches bank l % 32 with the
// other half of the wavefront in the other group of 32 -- no atomic, no bank conflict.  At the end of a temporal cell the
// lanes of each spatial cell are summed and the 33 nxy^2 entries go to `hist` once, with non-temporal stores; temporal cells
// the track never reaches are written as the zeros the private histograms hold.  A lane's sum is at most N^2 lmax x 65535
// < 2^32 (the header's size condition).
//
// The features are recomputed from the frames and the flow for every window pixel (five flow values and four grey values);
// the windows of neighbouring tracks overlap and hit in L2.  A per-frame feature map staged in a work buffer is a later,
// measured decision (tools/descriptors_probe.py).
#include "ofdis_kernels.h"

namespace ofdis {

constexpr int kDescLanes = 64;  // one wavefront per workgroup, as ofdis_track.hip
constexpr int kDescBins = 33;   // 8 HOG + 9 HOF + 8 MBHx + 8 MBHy
constexpr float kDescQMax = 65535.f;

struct DescArgs {
  const uint8_t* frames;  // [npairs + 1][H][W][noc]
  const float2* flow;     // [npairs][H][W]
  const float2* tracks;   // [lmax + 1][max_tracks]
  const int* start;       // [max_tracks]
  const int* len;         // [max_tracks]
  const long long* info;  // {ntracks, dropped}
  int npairs, W, H, lmax, max_tracks;
  int N, nxy, nt;
  float min_flow;
  unsigned* hist;  // [max_tracks][33 nxy^2 nt]
  float2* shape;   // [max_tracks][lmax] or null
};

// oct(a, b) of include/ofdis.h: the octant of a vector by comparisons only, -1 where no case holds (zero vector, NaN).  The
// four cases exclude each other, so they are selects and not branches: the window loop is bound by instruction issue.
template <class T>
__device__ __forceinline__ int desc_oct(T a, T b) {
  const T z = (T)0;
  const bool c0 = (a > z) & (b >= z), c1 = (a <= z) & (b > z), c2 = (a < z) & (b <= z), c3 = (a >= z) & (b < z);
  const T p = c0 ? a : c1 ? b : c2 ? -a : -b;
  const T q = c0 ? b : c1 ? -a : c2 ? -b : a;
  const int bin = (c0 ? 0 : c1 ? 2 : c2 ? 4 : 6) + (q >= p ? 1 : 0);
  return (c0 | c1 | c2 | c3) ? bin : -1;
}
// quant(m, s) of include/ofdis.h; a finite result for every m (fminf drops a NaN), used only where m is finite
__device__ __forceinline__ unsigned desc_quant(float m, float s) { return (unsigned)(int)floorf(fminf(m * s, kDescQMax) + 0.5f); }
__device__ __forceinline__ bool desc_finite(float m) { return fabsf(m) <= 3.4028234663852886e38f; }  // (NaN: false)
// q into bin `bin` of the bins at h (the lane's column of the LDS histogram) where `on`; nothing (zero into the first bin)
// where not
__device__ __forceinline__ void desc_add(unsigned* h, bool on, int bin, unsigned q) { h[(on ? bin : 0) * kDescLanes] += on ? q : 0u; }

// a vote of a gradient (gx, gy) with scale s into the 8 bins at h
__device__ __forceinline__ void desc_vote(unsigned* h, float gx, float gy, float s) {
  const float m = sqrtf(gx * gx + gy * gy);
  const int bin = desc_oct(gx, gy);
  desc_add(h, desc_finite(m) & (bin >= 0), bin, desc_quant(m, s));
}

template <int NOC>
__device__ __forceinline__ int desc_gray(const uint8_t* I, unsigned at) {
  if (NOC == 1) return I[at];
  return (int)I[at * 3] + (int)I[at * 3 + 1] + (int)I[at * 3 + 2];
}

template <int NOC>
__global__ __launch_bounds__(kDescLanes) void track_descriptors_kernel(DescArgs a) {
  __shared__ unsigned lds[kDescBins * kDescLanes];
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= a.info[0]) return;  // (uniform over the workgroup)
  const int ncells = a.nxy * a.nxy, cs = a.N / a.nxy, L = kDescLanes / ncells;
  const int cell = lane / L, sub = lane % L;  // cell >= ncells: an idle lane
  const int cell_x0 = (cell % a.nxy) * cs - a.N / 2, cell_y0 = (cell / a.nxy) * cs - a.N / 2;
  const int steps = min(max(a.len[slot], 1), a.lmax + 1) - 1;  // the pairs the track crossed
  const int first = a.start[slot];
  const size_t plane = (size_t)a.W * a.H;
  const size_t D = (size_t)kDescBins * ncells * a.nt;
  const unsigned by_cs = (unsigned)((0x100000000ull + cs - 1) / cs);  // q / cs == umulhi(q, by_cs) for q < 4096, cs <= 64
  unsigned* mine = lds + lane;
#pragma unroll
  for (int e = 0; e < kDescBins; ++e) mine[e * kDescLanes] = 0;

  for (int j = 0; j < a.lmax; ++j) {
    const int k = first + j;
    if (j < steps && cell < ncells && k >= 0 && k < a.npairs) {
      const float2 p = a.tracks[(size_t)j * a.max_tracks + slot];
      const float fx = floorf(p.x + 0.5f), fy = floorf(p.y + 0.5f);
      // a centre further than N outside the image has no window pixel inside it (and a NaN has no window)
      if (fx >= -64.f && fx <= (float)(a.W + 64) && fy >= -64.f && fy <= (float)(a.H + 64)) {
        const int x0 = (int)fx + cell_x0, y0 = (int)fy + cell_y0;
        const uint8_t* I = a.frames + (size_t)k * plane * NOC;
        const float2* F = a.flow + (size_t)k * plane;
        for (int q = sub; q < cs * cs; q += L) {
          const int qy = (int)__umulhi((unsigned)q, by_cs);
          const int x = x0 + (q - qy * cs), y = y0 + qy;
          if (x < 0 || x >= a.W || y < 0 || y >= a.H) continue;
          const int xl = max(x - 1, 0), xr = min(x + 1, a.W - 1), yu = max(y - 1, 0), yd = min(y + 1, a.H - 1);
          const unsigned row = (unsigned)(y * a.W);  // pixel numbers inside a frame are below 2^30
          const unsigned l = row + xl, r = row + xr, u = (unsigned)(yu * a.W + x), d = (unsigned)(yd * a.W + x);
          {  // HOG: doubled central differences of the grey value, exact integers
            const int gx = desc_gray<NOC>(I, r) - desc_gray<NOC>(I, l), gy = desc_gray<NOC>(I, d) - desc_gray<NOC>(I, u);
            const int bin = desc_oct(gx, gy);
            desc_add(mine, bin >= 0, bin, desc_quant(sqrtf((float)(gx * gx + gy * gy)), 16.f));
          }
          {  // HOF: bin 8 below min_flow
            const float2 f = F[row + x];
            const float m = sqrtf(f.x * f.x + f.y * f.y);
            const bool still = m < a.min_flow;
            const int bin = still ? 8 : desc_oct(f.x, f.y);
            desc_add(mine + 8 * kDescLanes, desc_finite(m) & (bin >= 0), bin, still ? 256u : desc_quant(m, 256.f));
          }
          const float2 fl = F[l], fr = F[r], fu = F[u], fd = F[d];
          desc_vote(mine + 17 * kDescLanes, fr.x - fl.x, fd.x - fu.x, 4096.f);  // MBHx
          desc_vote(mine + 25 * kDescLanes, fr.y - fl.y, fd.y - fu.y, 4096.f);  // MBHy
        }
      }
    }
    const int t = j * a.nt / a.lmax;
    if (j + 1 < a.lmax && (j + 1) * a.nt / a.lmax == t) continue;  // (uniform)
    // the end of temporal cell t: entry (cell c, bin e) is the sum over the L lanes of c
    __syncthreads();
    for (int o = lane; o < kDescBins * ncells; o += kDescLanes) {
      const int c = o / kDescBins, e = o % kDescBins;
      unsigned sum = 0;
      for (int s = 0; s < L; ++s) sum += lds[e * kDescLanes + c * L + s];
      const int ch0 = e < 8 ? 0 : e < 17 ? 8 : e < 25 ? 17 : 25, nb = ch0 == 8 ? 9 : 8;  // the channel's first bin and bins
      const size_t at = (size_t)ch0 * ncells * a.nt + (size_t)(t * ncells + c) * nb + (e - ch0);
      __builtin_nontemporal_store(sum, a.hist + (size_t)slot * D + at);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kDescBins; ++e) mine[e * kDescLanes] = 0;
  }

  if (!a.shape) return;
  // the sequential sum of the step lengths in every lane, then the lanes share the steps
  float S = 0.f;
  for (int j = 0; j < steps; ++j) {
    const float2 p = a.tracks[(size_t)j * a.max_tracks + slot], q = a.tracks[(size_t)(j + 1) * a.max_tracks + slot];
    const float dx = q.x - p.x, dy = q.y - p.y;
    S += sqrtf(dx * dx + dy * dy);
  }
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  for (int j = lane; j < a.lmax; j += kDescLanes) {
    float sx = 0.f, sy = 0.f;
    if (j < steps && S != 0.f) {
      const float2 p = a.tracks[(size_t)j * a.max_tracks + slot], q = a.tracks[(size_t)(j + 1) * a.max_tracks + slot];
      sx = (q.x - p.x) / S;
      sy = (q.y - p.y) / S;
    }
    __builtin_nontemporal_store((u2v){__float_as_uint(sx), __float_as_uint(sy)}, (u2v*)a.shape + (size_t)slot * a.lmax + j);
  }
}

hipError_t launch_track_descriptors(const uint8_t* frames, const float* flow, int npairs, int w, int h, int noc, const float* tracks,
                                    const int* start, const int* len, const long long* info, int lmax, int max_tracks, int patch,
                                    int nxy, int nt, float min_flow, uint32_t* hist, float* shape, hipStream_t s) {
  const DescArgs a{frames, (const float2*)flow, (const float2*)tracks, start, len, info, npairs, w, h, lmax, max_tracks,
                   patch, nxy, nt, min_flow, hist, (float2*)shape};
  const dim3 grid((unsigned)max_tracks);
  if (noc == 1)
    hipLaunchKernelGGL(track_descriptors_kernel<1>, grid, dim3(kDescLanes), 0, s, a);
  else
    hipLaunchKernelGGL(track_descriptors_kernel<3>, grid, dim3(kDescLanes), 0, s, a);
  return hipGetLastError();
}

}  // namespace ofdis
