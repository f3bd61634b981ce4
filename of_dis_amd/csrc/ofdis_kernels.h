// ofdis_kernels.h -- argument blocks and launchers of the gfx950 kernels (internal C++ API; the public ABI is
// include/ofdis.h).  The argument blocks are shared; the launchers exist once per arithmetic contract (ofdis_dev.h):
// ofdis_launchers.inc is included into ofdis::exact and ofdis::fused, every kernel file defines its launchers in the
// namespace of the contract it is being compiled for (OFDIS_KNS), and ofdis_capi.hip picks a set per context.
#pragma once
#include <type_traits>
#include <utility>

#include "ofdis_dev.h"

namespace ofdis {

// Runtime value -> template argument, written once per launcher: calls f with the std::integral_constant out of V0, V... that
// equals v; a value that is not in the list takes the LAST one, as the `default:` arm of a switch would.  Nested calls handle
// several arguments:  with_constant<1, 2, 3>(a.iterations, [&](auto NS) { ... kernel<decltype(NS)::value> ... });
template <auto V0, auto... V, class T, class F>
inline auto with_constant(T v, F&& f) {
  if constexpr (sizeof...(V) == 0) return f(std::integral_constant<decltype(V0), V0>{});
  else return v == V0 ? f(std::integral_constant<decltype(V0), V0>{}) : with_constant<V...>(v, f);
}
// ... and for a row 0 .. N-1 of a constexpr table of instantiations
template <class F, int... I>
inline auto with_index(int i, F&& f, std::integer_sequence<int, I...>) { return with_constant<I...>(i, f); }
template <int N, class F>
inline auto with_index(int i, F&& f) { return with_index(i, f, std::make_integer_sequence<int, N>{}); }

// Rows per frame slot of a wavefront in the kernels that put several frames of a low level side by side in one wavefront
// (64 / R frames: wavefront SOR, fused TV and their stereo twins).  The kernels take R as an argument and trust it.
inline int slot_rows(int h) { return h <= 16 ? 16 : (h <= 32 ? 32 : 64); }

// flow-plane layouts used between kernels
//   AoS   : [frame][h][w][2]   -- the reference's dense-flow format (DIS init / output)
//   planar: [frame][h][w] x2   -- TV stage
struct DisArgs {
  LevelGeom g;
  int nframes;
  // solver parameters (oflow.cpp:76-108)
  int max_iter, min_iter, costfct, patnorm;
  int stereo, camlr;  // SELECTMODE=2: one horizontal displacement per patch; camlr 0 -> p <= 0, 1 -> p >= 0 (patch.cpp:188-193)
  int reload_window;  // set by launch_patch_optimize (!ofdis_tuning::patch_window_reuse): the gray 8x8 kernel fetches its tap
                      // window in every evaluation, also where it has not moved
  float dp_thresh_sq, dr_thresh, res_thresh;
  float outlier_sq_max;  // largest x with sqrtf(x) <= outlierthresh (= P/2, oflow.cpp:82): outlier_sq_threshold()
  const float* im_a;     // [B][tmp_h][tmp_w][noc]
  const float* im_a_dx;
  const float* im_a_dy;
  const float* im_b;
  const float* flow_prev;  // AoS [B][h/2][w/2][2] or nullptr
  float* p_out;            // [B][nop][2]       both in the internal grid-row-major layout (ofdis_dev.h: patch_slot,
  float* pweight;          // [B][nop][novals]  pweight_row): the densify kernels read them, nobody else
  float* pixw;             // [B][nop][P*P] or nullptr: RGB 12x12 only (patch_pixel_weights_supported): patches whose weights
                           // the densification reads unshifted store one float per pixel here INSTEAD of pweight (ofdis_dev.h)
};
// snapshot of the kernel-selection knobs (include/ofdis.h: ofdis_tuning; ofdis_capi.hip); *epoch counts the changes
ofdis_tuning tuning(unsigned* epoch = nullptr);

// Which patch kernel launch_patch_optimize runs, decided once: a pure host function of the level, the mode, the knobs and the
// arithmetic contract.  The launcher launches what it says, patch_pixel_weights_supported is its `pixw`.
struct PatchKernel {
  // NONE: refused | LANES16: patch_optimize_rgb12_kernel (fused contract) / patch_optimize_rgb12x_kernel (exact), 16 lanes per
  // patch | GRAY8: patch_optimize_gray8_kernel | GENERIC: patch_optimize_kernel
  enum Family { NONE, LANES16, GRAY8, GENERIC };
  int row;               // the instantiation: its row of kPatchKernels, -1 = no kernel
  int contract;          // as given
  int lpp;               // lanes per patch
  int threads;           // workgroup size
  int blocks_per_frame;  // (the grid: xcd_grid of them)
  bool pixw;             // that kernel honours DisArgs::pixw: the compact per-pixel weights of RGB 12x12 flow patches
};
// every instantiation of the three kernels that exists: t = its template arguments in the order of its parameter list --
// LANES16 <L1, NOC, STEREO, BS>, GRAY8 <COST, STEREO>, GENERIC <M, LPP, NV, COST>
struct PatchInstance {
  PatchKernel::Family family;
  int t[4];
};
inline constexpr PatchInstance kPatchKernels[] = {
    // RGB 8x8 | gray 12x12 | RGB 12x12, each flow / stereo with the L2 / L1 cost
    {PatchKernel::LANES16, {0, 3, 0, 2}}, {PatchKernel::LANES16, {1, 3, 0, 2}}, {PatchKernel::LANES16, {0, 3, 1, 2}},
    {PatchKernel::LANES16, {1, 3, 1, 2}}, {PatchKernel::LANES16, {0, 1, 0, 3}}, {PatchKernel::LANES16, {1, 1, 0, 3}},
    {PatchKernel::LANES16, {0, 1, 1, 3}}, {PatchKernel::LANES16, {1, 1, 1, 3}}, {PatchKernel::LANES16, {0, 3, 0, 3}},
    {PatchKernel::LANES16, {1, 3, 0, 3}}, {PatchKernel::LANES16, {0, 3, 1, 3}}, {PatchKernel::LANES16, {1, 3, 1, 3}},
    {PatchKernel::GRAY8, {-1, 1}},        {PatchKernel::GRAY8, {0, 0}},         {PatchKernel::GRAY8, {-1, 0}},
    {PatchKernel::GENERIC, {1, 8, 64, 0}},    {PatchKernel::GENERIC, {1, 8, 64, -1}},   {PatchKernel::GENERIC, {1, 8, 0, -1}},
    {PatchKernel::GENERIC, {3, 64, 0, -1}},   {PatchKernel::GENERIC, {7, 32, 432, 0}},  {PatchKernel::GENERIC, {7, 32, 432, 1}},
    {PatchKernel::GENERIC, {7, 64, 432, 0}},  {PatchKernel::GENERIC, {7, 64, 432, 1}},  {PatchKernel::GENERIC, {7, 64, 0, -1}},
    {PatchKernel::GENERIC, {12, 64, 0, -1}},
};
constexpr int kNumPatchKernels = (int)(sizeof(kPatchKernels) / sizeof(kPatchKernels[0]));

inline PatchKernel choose_patch_kernel(const LevelGeom& g, bool stereo, int costfct, bool pixw_asked, const ofdis_tuning& tn,
                                       int contract) {
  PatchKernel k{-1, contract, 0, 0, 0, false};
  auto pick = [&](PatchKernel::Family family, int t0, int t1, int t2 = 0, int t3 = 0) {
    for (int r = 0; r < kNumPatchKernels && k.row < 0; ++r) {
      const PatchInstance& i = kPatchKernels[r];
      if (i.family == family && i.t[0] == t0 && i.t[1] == t1 && i.t[2] == t2 && i.t[3] == t3) k.row = r;
    }
    const int wpf = (g.nop + 64 / k.lpp - 1) / (64 / k.lpp);                 // wavefronts per frame
    const int wpb = (family == PatchKernel::GRAY8 && wpf < 4) ? wpf : 4;     // ... per block (the other kernels assume 4)
    k.threads = 64 * wpb;
    k.blocks_per_frame = (wpf + wpb - 1) / wpb;
    return k;
  };
  const int M = (g.novals + 63) / 64;
  const bool l2l1 = costfct == 0 || costfct == 1;
  // 12x12 patches, RGB or gray, and RGB 8x8 patches, flow or stereo, have their own mapping (16 lanes per patch, four
  // patches per wavefront: ofdis_tuning::rgb12 with rgb12_lpp = 16, the default)
  const int rgb12_lpp = tn.rgb12_lpp == 0 ? 16 : tn.rgb12_lpp;
  if (((g.P == 12 && (g.noc == 1 || g.noc == 3)) || (g.P == 8 && g.noc == 3)) && l2l1 && tn.rgb12 && rgb12_lpp == 16) {
    k.lpp = 16;
    k.pixw = g.novals == 432 && g.P == 12 && !stereo;
    return pick(PatchKernel::LANES16, costfct != 0, g.P == 8 ? 3 : g.noc, stereo, g.P == 8 ? 2 : 3);
  }
  if (pixw_asked || M > 12) return k;  // (only the kernels above write the compact weights)
  if (M <= 1 && g.noc == 1 && g.P == 8 && tn.gray8) {
    k.lpp = 4;
    return pick(PatchKernel::GRAY8, (!stereo && costfct == 0) ? 0 : -1, stereo);
  }
  // RGB 12x12 (operating points 3 and 4, BASELINE configs[3]): 432 entries, 6 full groups of 64 + 48.  ofdis_tuning::rgb12_lpp = 32:
  // two patches per wavefront (the scalar solve, predicates and every reduction instruction shared by two patches:
  // 929 -> 705 instructions per patch and iteration, 82 -> 127 VGPRs).  Measured on configs[3] the same 19.6 +- 0.4 ms per
  // 16-pair level-1 launch either way -- patches that reset early leave their wavefront's other half running alone
  // (PMC: 18 % fewer VALU instructions, same time) -- so one patch per wavefront stayed the default until the
  // 16-lanes-per-patch kernels (round 4) took it over.
  const bool rgb12 = g.novals == 432 && !stereo && l2l1 && tn.rgb12;
  k.lpp = M <= 1 ? 8 : ((rgb12 && rgb12_lpp == 32) ? 32 : 64);
  if (M <= 1 && g.novals == 64) return pick(PatchKernel::GENERIC, 1, 8, 64, costfct == 0 ? 0 : -1);
  if (M <= 1) return pick(PatchKernel::GENERIC, 1, 8, 0, -1);
  if (M <= 3) return pick(PatchKernel::GENERIC, 3, 64, 0, -1);
  if (rgb12) return pick(PatchKernel::GENERIC, 7, k.lpp, 432, costfct);
  return pick(PatchKernel::GENERIC, M <= 7 ? 7 : 12, 64, 0, -1);
}

// The geometry of densify_quad_kernel and of the densification inside tv_prep_kernel (PrepArgs::dens_*), which must agree: gray
// 8x8 patches on a step-4 grid (operating point 2), at most 2 x 2 patches per pixel
inline bool densify_quad_geometry(const LevelGeom& g) { return g.noc == 1 && g.P == 8 && g.steps == 4 && g.offw < 4 && g.offh < 4; }

struct DensifyArgs {
  LevelGeom g;
  int nframes;
  const float* p;        // [B][nop][2]       (internal layout, as the patch kernels write them)
  const float* pweight;  // [B][nop][novals]
  const float* pixw;     // [B][nop][P*P] or nullptr: what the patch kernel was given as DisArgs::pixw
  float* flow_aos;       // if non-null: AoS output
  float* wx;             // else planar outputs (row-major)
  float* wy;
  // forward-backward merging (usefbcon, patchgrid.cpp:277-375): the complementary grid's results, or null
  int stereo;               // one flow channel: flow_aos is [B][h][w], wy is not written
  unsigned idx_magic;       // set by launch_densify: ceil(2^32 / w) for the pixel-index split
  const float* cg_p;        // [B][nop][2]
  const float* cg_pweight;  // [B][nop][novals]
};

struct TvGeom {
  int w, h, noc, nframes;
};

// The full-resolution finish (ofdis_upsample.h): the level flow, sw x sh and a factor 2^sc_l below the padded size, goes to
// the crop of wo x ho pixels at (left, top) of the padded full-resolution image.
struct UpGeom {
  int sw, sh, sc_l, left, top, wo, ho;
  __host__ __device__ float scf() const { return (float)(1 << sc_l); }
  __host__ __device__ float inv() const { return 1.0f / scf(); }  // (a power of two: exact)
  __host__ __device__ bool scale() const { return sc_l > 0; }
  __host__ __device__ size_t plane() const { return (size_t)sw * sh; }  // pixels of one frame's level flow
};

// The two launch limits, in workgroups of 256 lanes.  QUAD_MAX_BLOCKS: one launch of a kernel in which a lane owns a quad of
// one frame (quad_chunks, ofdis_quad.h); the launcher walks the frames in chunks that stay below it.  GRID_MAX_BLOCKS: the
// grid of a grid-stride kernel (grid_for); the kernel loops over what is beyond it.  Both are read in host code only.  The
// product is built with the constants; the test library (tests/csrc/ofdis_launch_hooks.hip) compiles the same units with
// OFDIS_TEST_LAUNCH_LIMITS, where they are two host variables of that library which a test lowers to reach the second chunk
// and the second trip at test sizes.
constexpr long long QUAD_MAX_BLOCKS = 1ll << 22;
constexpr long long GRID_MAX_BLOCKS = 1ll << 20;
#ifdef OFDIS_TEST_LAUNCH_LIMITS
extern long long test_quad_max_blocks, test_grid_max_blocks;
inline long long quad_max_blocks() { return test_quad_max_blocks; }
inline long long grid_max_blocks() { return test_grid_max_blocks; }
#else
constexpr long long quad_max_blocks() { return QUAD_MAX_BLOCKS; }
constexpr long long grid_max_blocks() { return GRID_MAX_BLOCKS; }
#endif

// blocks of 256 threads for a grid-stride loop over `total` elements
inline unsigned grid_for(long long total) {
  long long b = (total + 255) / 256;
  if (b > grid_max_blocks()) b = grid_max_blocks();
  if (b < 1) b = 1;
  return (unsigned)b;
}

// image_warp.  src: either the padded interleaved pyramid plane (src_padded=1: [B][tmp_h][tmp_w][noc],
// pad/tmp_w given) or packed planar [B][noc][h][w] (src_padded=0).  dst: [B][noc][h][w], mask [B][h][w].
struct WarpArgs {
  TvGeom t;
  const float* src;
  int src_padded, pad, tmp_w, tmp_h;
  const float* wx;
  const float* wy;
  float* dst;
  float* mask;
};
// get_derivatives.  im1 as for WarpArgs.src; im2w packed planar [B][noc][h][w].
// out [B][8][noc][h][w]
struct DerivArgs {
  TvGeom t;
  const float* im1;
  int im1_padded, pad, tmp_w, tmp_h;
  const float* im2w;
  float* out;  // [B][8][noc][h][w] row-major
  // record form (the RGB fused TV path; ofdis_tv.hip): with rec_d8 the planes are not written; [noc][B][w*h][8] derivative
  // records and [B][w*h][2] (wx, wy) records in the diag layout instead, zeroed by the warp's mask
  float* rec_d8 = nullptr;
  float* rec_w = nullptr;
  const float* mask = nullptr;  // row-major [B][h][w]
  const float* wx = nullptr;    // row-major
  const float* wy = nullptr;
};

// image_warp + get_derivatives of the fused TV path in one row-marching kernel (ofdis_prep.hip): densified AoS flow and the
// two padded gray planes in, the sdiag records of the fused TV kernel out (ofdis_dev.h: sdiag_index)
struct PrepArgs {
  TvGeom t;           // noc = 1
  const float* im1;   // padded plane of the first image  [B][tmp_h][tmp_w]
  const float* im2;   // padded plane of the second image
  int pad, tmp_w, tmp_h;
  const float* flow;  // AoS [B][h][w][2], row-major: the flow to warp with (wx, wy)
  float* d8;          // [records][8] = Ix, Iz, Ixx, Ixz, Iy, Ixy, Iyz, Iyy; all zero where the warp's mask is zero
  float* wrec;        // [records][2] = wx, wy
  int S;              // frames per strip
  int band_rows;      // output rows per wavefront (0 = chosen by the launcher from the batch size)
  // round 6, optional: densification inside this kernel (tv_prep_densifies).  With dens_p the dense flow is computed from the
  // patch results -- [B][nop][2] displacements and [B][nop][64] weights in the internal grid-row-major layout (ofdis_dev.h:
  // patch_slot, pweight_row), exactly what launch_densify would read -- and `flow` is not read.
  const float* dens_p = nullptr;
  const float* dens_pweight = nullptr;
  int dens_nopw = 0, dens_noph = 0, dens_offw = 0, dens_offh = 0;
};

// compute_smoothness + compute_data + sub_laplacian x2 -> sys [B][7][w*h] in DIAG layout (ofdis_dev.h)
struct SystemArgs {
  TvGeom t;
  const float* mask;   // row-major [B][h][w]
  const float* wx;     // row-major
  const float* wy;
  const float* du;     // DIAG layout [B][w*h]
  const float* dv;
  const float* derivs;
  float quarter_alpha, half_delta_over3, half_gamma_over3;
  float* sys;
};

// sor_coupled; every operand in DIAG layout
struct SorArgs {
  TvGeom t;
  const float* sys;  // [B][7][w*h]: a11,a12,a22,b1,b2,sh,sv
  float* du;         // [B][w*h]
  float* dv;
  int iterations;
  float omega;
};

// All fixed-point iterations of a level fused: compute_smoothness + compute_data + 2x sub_laplacian produce each
// anti-diagonal's system coefficients in registers, immediately consumed by the wavefront SOR of
// ofdis_sor.hip (h <= 64, gray).  Operands = the sdiag records of ofdis_prep.hip.
struct FusedArgs {
  TvGeom t;
  const float* d8;    // [records][8] derivatives (all zero where the warp's mask is zero)
  const float* wrec;  // [records][2] wx, wy
  float* uv;          // [records][2] du, dv (in/out; never read during the first iteration)
  int S;              // frames per strip (divides t.nframes)
  float quarter_alpha, half_delta_over3, half_gamma_over3;
  int iterations;  // SOR sweeps per fixed-point iteration (tv_solverit)
  float omega;
  int n_inner;     // fixed-point iterations run back to back inside one launch
  int total_frames;  // frames of the whole batch this launch is a part of (pipelined sub-batches); 0 = t.nframes
  // optional: AoS flow [B][h][w][2].  When the launcher picks a multi-wave variant it writes uu = wx + du, vv = wy + dv
  // of the last fixed-point iteration there itself (refine_variational.cpp:209-221, 92-99) instead of storing du, dv --
  // tv_finish is then not needed; launch_tv_fused reports that through *wrote_flow.
  float* flow_out;
  int mw_max_groups;  // frame groups (workgroups) up to which the multi-wave variants are launched (0 = never)
  int split;          // 0 = never the split (producer / solver wavefronts) variant of the multi-wave kernel
  int tp_pipe;        // 1: THROUGHPUT regime on the iteration-pipelined mapping (MODE 1) with strips of S frames: a workgroup of
                      // n_inner wavefronts per strip group, du / dv from iteration to iteration through LDS, the derivative
                      // records of a row read by n_inner wavefronts of ONE compute unit within a few steps (one HBM read, the
                      // others hit the L2) -- 48 instead of 56 n_inner bytes of HBM traffic per pixel and level
  int tall_group = 0; // levels of 65 ... 96 rows: 1 = several strips per workgroup, their rows beyond 64 in ONE shared wavefront
                      // (ofdis_fused_tall.hip: GROUPED), 0 = two wavefronts per strip
};
// cross-CU variant (one workgroup per fixed-point iteration of a frame group), kept out of FusedArgs so that the other
// variants' kernel arguments -- and register allocation -- stay what they were
struct FusedXcu {
  float* xbuf = nullptr;   // [n_inner - 1][nframes][w*h] granules of 4 floats {du, tag, dv, tag}; null: never
  int max_groups = 0;      // frame groups up to which the variant is launched (0 = never)
  int* err = nullptr;      // device-visible word, set to 1 when a hand-over row never arrived (results invalid); the variant
                           // is only launched with one
  unsigned wait_us = 0;    // microseconds a workgroup waits for one row before it gives up; 0 = the default (50 ms), 1 = not at all
  int drop = 0;            // test hook: the first iteration withholds its hand-over rows (ofdis_tuning::fused_xcu_drop)
};




// on-device pyramid (ofdis_pyr.hip; run_dense.cpp:130-178,298-311 restated)
// row y of frame f starts at src + f * stride + y * pitch (bytes; packed frames: pitch = wo * noc, stride = pitch * ho)
hipError_t launch_pyr_base(const uint8_t* src, float* dst, int nframes, int wo, int ho, int W, int H, int noc, int l,
                           size_t pitch, size_t stride, hipStream_t s);
hipError_t launch_pyr_down(const float* src, float* dst, int nframes, int w, int h, int noc, hipStream_t s);
// `down` (optional): also the next coarser level's unpadded image [B][h/2][w/2][noc] (what launch_pyr_down computes), in the
// same launch where the geometry allows (pyr_planes_fuses_down), else by a launch of its own
hipError_t launch_pyr_planes(const float* src, float* img, float* dx, float* dy, int nframes, int w, int h, int noc,
                             int pad, hipStream_t s, float* down = nullptr);
bool pyr_planes_fuses_down(int w, int h, int noc, int pad);
// which kernels the three launchers above run, stated once (host only; the launchers call these and nothing else decides):
// the base level's generic kernel or the 16-byte streaming kernel for blocks of 4, 8 or 16 pixels (the value is the block size)
enum PyrBaseVariant { PYR_BASE_GENERIC = 0, PYR_BASE_STREAM4 = 4, PYR_BASE_STREAM8 = 8, PYR_BASE_STREAM16 = 16 };
PyrBaseVariant pyr_base_variant(const uint8_t* src, int wo, int W, int noc, int l, size_t pitch, size_t stride);
// the planes' generic kernel (a separate pyr_down launch where `down` is wanted), the gray quad kernel, or the quad kernel
// writing `down` as well
enum PyrPlanesVariant { PYR_PLANES_GENERIC = 0, PYR_PLANES_GRAY4 = 1, PYR_PLANES_GRAY4_DOWN = 2 };
PyrPlanesVariant pyr_planes_variant(int w, int h, int noc, int pad, bool want_down);

// result to full resolution (ofdis_upsample.hip).  x 2^sc_l, bilinear upsample (cv::resize INTER_LINEAR) and crop of the AoS
// result (run_dense.cpp:406-414): the OFDIS_ENC_F32 kernel of launch_upsample_crop_enc
hipError_t launch_upsample_crop(const float* flow, float* out, int nframes, UpGeom g, int channels, hipStream_t s);
// the same, written in an output encoding (include/ofdis.h: ofdis_encoding; `type` already validated): out = [nframes][ho][wo]
// [channels] elements.  OFDIS_ENC_F32 with two channels is launch_upsample_crop.
hipError_t launch_upsample_crop_enc(const float* flow, void* out, int nframes, UpGeom g, int channels, int type, float scale,
                                    float offset, hipStream_t s);
// n fp32 values of a materialised array into that encoding (ofdis_encode)
hipError_t launch_encode(const float* src, void* dst, size_t n, int type, float scale, float offset, hipStream_t s);
// forward-backward consistency test (include/ofdis.h: ofdis_fb_check) on full-resolution AoS flows
hipError_t launch_fb_check(const float* flow, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                           float beta, hipStream_t s);
// both directions' level flows to full resolution plus both masks in one launch (ofdis_batch_upsample_bidir); outputs may be null
hipError_t launch_upsample_bidir(const float* fw, const float* rev, float* out_fw, float* out_rev, uint8_t* mask_fw,
                                 uint8_t* mask_rev, int nframes, UpGeom g, float alpha, float beta, hipStream_t s);
// stereo left-right step (include/ofdis.h; ofdis_stereo_lr.hip).  mir(I)[y][x] = I[y][w-1-x] on [n][h][w][noc] 8-bit frames:
hipError_t launch_mirror_u8(const uint8_t* src, uint8_t* dst, int nframes, int w, int h, int noc, hipStream_t s);
hipError_t launch_lr_check(const float* disp, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                           float beta, hipStream_t s);
hipError_t launch_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int w, int h, int mode,
                                 hipStream_t s);
// forward and mirror level disparities to both views' full-resolution disparities and masks in one launch
// (ofdis_batch_upsample_lr; outputs may be null), for original widths upsample_lr_fuses() accepts ...
bool upsample_lr_fuses(int wo);
size_t upsample_lr_row_bytes(int wo);  // LDS per output row
hipError_t launch_upsample_lr(const float* fw, const float* mir, float* out_l, float* out_r, uint8_t* mask_l, uint8_t* mask_r,
                              int nframes, UpGeom g, int fill_mode, float alpha, float beta, hipStream_t s);
// ... and, above them, the first step of the composition: U and DR = -Dm un-mirrored, materialised
hipError_t launch_lr_materialise(const float* fw, const float* mir, float* u, float* dr, int nframes, UpGeom g, hipStream_t s);
// frame interpolation (include/ofdis.h: ofdis_interpolate; ofdis_interp.hip).  The times travel by value in the launch.
struct InterpTimes {
  float t[16];  // OFDIS_INTERP_MAX_TIMES
  int n;
};
// on materialised arrays: frames [n][h][w][noc] u8, AoS flows [n][h][w][2], masks [n][h][w] or null, out [n][ts.n][h][w][noc]
hipError_t launch_interp_frames(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                                const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int w, int h,
                                int noc, const InterpTimes& ts, hipStream_t s);
// straight from both directions' level flows (ofdis_batch_interpolate): flows and masks as launch_upsample_bidir computes them
hipError_t launch_interp_bidir(const uint8_t* img_a, const uint8_t* img_b, const float* fw, const float* rev, uint8_t* out,
                               int nframes, UpGeom g, int noc, const InterpTimes& ts, float alpha, float beta, hipStream_t s);
// point trajectories (include/ofdis.h: ofdis_track_points; ofdis_track.hip).  On materialised full-resolution flows
// [npairs][h][w][2] (rev null: no consistency test); seeds [npoints][2], seed_frame [npoints] or null, tracks
// [npairs + 1][npoints][2], counts [npoints] or null
hipError_t launch_track_points(const float* fw, const float* rev, int npairs, int w, int h, const float* seeds,
                               const int* seed_frame, int npoints, int max_steps, float alpha, float beta, float* tracks,
                               int* counts, hipStream_t s);
// straight from the level flows of npairs consecutive pairs (ofdis_batch_track_points): the flows as launch_upsample_bidir /
// launch_upsample_crop compute them
hipError_t launch_track_level(const float* fw, const float* rev, int npairs, UpGeom g, const float* seeds, const int* seed_frame,
                              int npoints, int max_steps, float alpha, float beta, float* tracks, int* counts, hipStream_t s);
// dense trajectories (include/ofdis.h: ofdis_dense_tracks; ofdis_dense_tracks.hip).  The grid of a w x h frame (returns its
// cells), and the bytes of the work buffer of a call (max_len 0 and max_tracks OFDIS_DT_MAX_TRACKS: of any call on that clip)
int dense_tracks_cells(int w, int h, int stride, int* ncx, int* ncy);
size_t dense_tracks_work_bytes(int npairs, int w, int h, int stride, int max_len, int max_tracks);
// frames [nframes][h][w][noc] u8 -> out [nframes][ncy][ncx] u8
hipError_t launch_seed_texture(const uint8_t* frames, int nframes, int w, int h, int noc, int stride, int window, int min_eig,
                               uint8_t* out, hipStream_t s);
// on materialised flows [npairs][h][w][2] (rev null: no consistency test): the texture launch, then per frame advance, count and
// assign, all on the stream; tracks [Lmax + 1][max_tracks][2], start, len (or null) [max_tracks], info [2]
hipError_t launch_dense_tracks(const uint8_t* frames, const float* fw, const float* rev, int npairs, int w, int h, int noc,
                               int stride, int window, int min_eig, int max_len, float alpha, float beta, int max_tracks,
                               float* tracks, int* start, int* len, long long* info, void* work, hipStream_t s);
// straight from the level flows of npairs consecutive pairs (ofdis_batch_dense_tracks), as launch_track_level
hipError_t launch_dense_tracks_level(const uint8_t* frames, const float* fw, const float* rev, int npairs, UpGeom g, int noc,
                                     int stride, int window, int min_eig, int max_len, float alpha, float beta, int max_tracks,
                                     float* tracks, int* start, int* len, long long* info, void* work, hipStream_t s);
// track selection (include/ofdis.h: ofdis_track_select; ofdis_track_select.hip): the arrays of launch_dense_tracks in, code
// [max_tracks] u8 and counts [7] (either may be null) and the compacted set of max_tracks_out slots out -- tracks_out, start_out,
// len_out, info_out [2], index [max_tracks_out] and shape_out [max_tracks_out][lmax][2] (either may be null); models [npairs][6]
// of launch_gmotion_frames for a w x h frame, or null.  Three launches (classify, scan, scatter); work holds
// track_select_work_bytes(max_tracks): one 64-byte record per workgroup, 8-byte aligned.  nparam: the doubles per model, 6, or
// 8 for those of launch_projective_frames (ofdis_track_select_projective)
size_t track_select_work_bytes(int max_tracks);
hipError_t launch_track_select(const float* tracks, const int* start, const int* len, const long long* info, int lmax, int max_tracks,
                               const double* models, int npairs, int w, int h, const ofdis_track_select_params& p, uint8_t* code,
                               long long* counts, int max_tracks_out, float* tracks_out, int* start_out, int* len_out,
                               long long* info_out, int* index, float* shape_out, void* work, hipStream_t s, int nparam = 6);
// trajectory-aligned descriptors (include/ofdis.h: ofdis_track_descriptors; ofdis_descriptors.hip): the arrays of
// launch_dense_tracks in, hist [max_tracks][33 nxy^2 nt] u32 and shape [max_tracks][lmax][2] (or null) out; one wavefront per
// slot, the slots >= info[0] return at once
hipError_t launch_track_descriptors(const uint8_t* frames, const float* flow, int npairs, int w, int h, int noc, const float* tracks,
                                    const int* start, const int* len, const long long* info, int lmax, int max_tracks, int patch,
                                    int nxy, int nt, float min_flow, uint32_t* hist, float* shape, hipStream_t s);
// bag-of-features encoding of those descriptors (include/ofdis.h: ofdis_descriptor_normalize ... ofdis_track_bof;
// ofdis_bof.hip): hist -> desc u8 per slot and channel; desc against codebook [nwords][33 nxy^2 nt] u8 on the matrix cores ->
// words, dist [max_tracks][4] (either may be null); words -> bof [4][nwords], cleared by a launch of its own; and the three in
// one pass that never writes desc.  All sized by max_tracks, the slots >= info[0] neither read nor written
hipError_t launch_descriptor_normalize(const uint32_t* hist, const long long* info, int max_tracks, int nxy, int nt, uint8_t* desc,
                                       hipStream_t s);
hipError_t launch_codebook_assign(const uint8_t* desc, const long long* info, int max_tracks, int nxy, int nt, const uint8_t* codebook,
                                  int nwords, int* words, int* dist, hipStream_t s);
hipError_t launch_bof_histogram(const int* words, const int* len, const long long* info, int max_tracks, int nwords, int min_len,
                                uint32_t* bof, hipStream_t s);
hipError_t launch_track_bof(const uint32_t* hist, const int* len, const long long* info, int max_tracks, int nxy, int nt,
                            const uint8_t* codebook, int nwords, int min_len, uint32_t* bof, int* words, hipStream_t s);
// which bof_assign_kernel<NK, TG, .> serves C = nxy^2 nt, by the k-steps nk = ceil(9 C / 64) of the longest channel: a
// workgroup owns 64 TG slots and stages tiles of 16 TG words.  Host only; the launcher and the tests' layout classes read it
struct BofShape {
  int nk, NK, TG;
};
BofShape bof_assign_shape(int C);
// k-means training of that codebook (include/ofdis.h: ofdis_codebook_seed ... ofdis_codebook_train; ofdis_kmeans.hip): the seed
// rows; one centre update (six launches: clear, count, scan, scatter, sum, finish) from words -> codebook, counts [4][nwords];
// and iters x (launch_codebook_assign + update) with stats [iters][4][2] or null.  len may be null (every slot a member); work
// holds codebook_train_work_bytes (the layout: ofdis_kmeans.hip), 8-byte aligned
size_t codebook_train_work_bytes(int max_tracks, int nxy, int nt, int nwords);
// how the lanes of the update's sum are split for C = nxy^2 nt: np passes (1 or 5) of el lanes over the dwords of a channel;
// rl = 4 el np, the uint32 entries of a slab row.  Host only
struct KmGeom {
  int np, el, log2el, rl;
};
KmGeom km_geom(int C);
// km_finish_kernel's threads over a channel of n_c entries: 2^log2te entries x 256 >> log2te groups of chunks.  One statement
// for the kernel and the host; a macro, since the kernel compiles to the same code only from the expression itself (through
// an inlined function one scalar compare of it comes out unsigned)
#define OFDIS_KM_FINISH_LOG2TE(n_c) ((n_c) <= 16 ? 4 : (n_c) <= 128 ? 7 : 8)
inline int km_finish_log2te(int n_c) { return OFDIS_KM_FINISH_LOG2TE(n_c); }
hipError_t launch_codebook_seed(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                                int min_len, uint8_t* codebook, hipStream_t s);
hipError_t launch_codebook_update(const uint8_t* desc, const int* words, const int* len, const long long* info, int max_tracks, int nxy,
                                  int nt, int nwords, int min_len, uint8_t* codebook, uint32_t* counts, void* work, hipStream_t s);
hipError_t launch_codebook_train(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                                 int min_len, int iters, uint8_t* codebook, int* words, uint32_t* counts, long long* stats, void* work,
                                 hipStream_t s);
// motion-compensated temporal filter (include/ofdis.h: ofdis_temporal_filter; ofdis_tfilter.hip).  On materialised arrays:
// frames, out [npairs + 1][h][w][noc] u8, AoS flows [npairs][h][w][2], masks [npairs][h][w] or null, support
// [npairs + 1][h][w] or null
hipError_t launch_tfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                                 const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int w, int h, int noc,
                                 float wn, float tau, hipStream_t s);
// straight from the level flows of npairs consecutive pairs (ofdis_batch_temporal_filter): flows and masks as
// launch_upsample_bidir computes them
hipError_t launch_tfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                int npairs, UpGeom g, int noc, float wn, float tau, float alpha, float beta, hipStream_t s);
// temporal filter along flow trajectories (include/ofdis.h: ofdis_trajectory_filter; ofdis_trajfilter.hip).  The weights travel
// by value in the launch, as InterpTimes does: w[0 .. radius), the rest zero
struct TrajWeights {
  float w[8];  // OFDIS_TRAJ_MAX_RADIUS
  int radius;
};
// on materialised arrays: frames, out [npairs + 1][h][w][noc] u8, AoS flows [npairs][h][w][2], support [npairs + 1][h][w] or
// null; fb: with the consistency test
hipError_t launch_trajfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out,
                                    uint8_t* support, int npairs, int w, int h, int noc, const TrajWeights& tw, float tau,
                                    bool fb, float alpha, float beta, hipStream_t s);
// straight from the level flows of npairs consecutive pairs (ofdis_batch_trajectory_filter): the flows as
// launch_upsample_bidir computes them
hipError_t launch_trajfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                   int npairs, UpGeom g, int noc, const TrajWeights& tw, float tau, bool fb, float alpha,
                                   float beta, hipStream_t s);
// global motion models and motion-compensated flow (include/ofdis.h: ofdis_global_motion; ofdis_gmotion.hip).  `work`: one
// record of sums per workgroup and pair, gmotion_work_bytes(npairs, w, h) bytes; `rounds` x (accumulate, solve) on the stream.
// On materialised arrays: flow [npairs][h][w][2], mask [npairs][h][w] or null, models [npairs][6], stats [npairs][3] or null
size_t gmotion_work_bytes(int npairs, int w, int h);
hipError_t launch_gmotion_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int model, int rounds,
                                 float thresh, double* models, long long* stats, void* work, hipStream_t s);
hipError_t launch_gmotion_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w, int h,
                                            float thresh, float* residual, uint8_t* label, hipStream_t s);
// straight from the level flows of npairs pairs: the flow as launch_upsample_crop computes it; with `rev` the forward mask of
// launch_upsample_bidir, without (null) no mask
hipError_t launch_gmotion_level(const float* fw, const float* rev, int npairs, UpGeom g, int model, int rounds, float thresh,
                                float alpha, float beta, double* models, long long* stats, void* work, hipStream_t s);
hipError_t launch_gmotion_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UpGeom g,
                                           float thresh, float alpha, float beta, float* residual, uint8_t* label, hipStream_t s);
// the 8-parameter projective twins (include/ofdis.h: ofdis_projective_motion): the same kernels with models [npairs][8], records
// of 24 sums (projective_work_bytes) and, as the third value of stats, the number of parameters solved
size_t projective_work_bytes(int npairs, int w, int h);
hipError_t launch_projective_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int rounds, float thresh,
                                    double* models, long long* stats, void* work, hipStream_t s);
hipError_t launch_projective_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w,
                                               int h, float thresh, float* residual, uint8_t* label, hipStream_t s);
hipError_t launch_projective_level(const float* fw, const float* rev, int npairs, UpGeom g, int rounds, float thresh, float alpha,
                                   float beta, double* models, long long* stats, void* work, hipStream_t s);
hipError_t launch_projective_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UpGeom g,
                                              float thresh, float alpha, float beta, float* residual, uint8_t* label, hipStream_t s);
// segments of label maps (include/ofdis.h: ofdis_label_segments; ofdis_segments.hip): label [nmaps][h][w] u8, flow
// [nmaps][h][w][2] or null -> segments [nmaps][h][w] int32 and records [nmaps][max_segments][12] int64 (either may be null), info
// [nmaps][4] int64.  Seven launches on the stream (init, merge, flatten, count, scan, number, relabel), all grid-stride; work
// holds segments_work_bytes: parent and area, int32 [nmaps][h * w] each, and four int32 per block of 256 pixels
size_t segments_work_bytes(int nmaps, int w, int h);
hipError_t launch_label_segments(const uint8_t* label, const float* flow, int nmaps, int w, int h, unsigned codes, int conn,
                                 int min_area, int max_segments, int* segments, long long* records, long long* info, void* work,
                                 hipStream_t s);
// object tracks (include/ofdis.h: ofdis_segment_overlap, _link, _chain, _relabel, _tracks; ofdis_segment_tracks.hip): segments
// [nmaps][h][w] int32, records [nmaps][S][12] int64 and info [nmaps][4] int64 of launch_label_segments, flow [nmaps][h][w][2]
// -> overlap [nmaps - 1][S][S] int32 (two launches: clear, accumulate), link [nmaps - 1][S] int32, ids [nmaps][S] int32, tracks
// [max_tracks][12] and tinfo [4] int64 (one workgroup), track_map [nmaps][h][w] int32.  One map: overlap and link launch nothing.
// segment_tracks_work_bytes: overlap and link, rounded up to 8 bytes, at least 8
size_t segment_tracks_work_bytes(int nmaps, int max_segments);
hipError_t launch_segment_overlap(const int* segments, const float* flow, const long long* info, int nmaps, int w, int h,
                                  int max_segments, int* overlap, hipStream_t s);
hipError_t launch_segment_link(const int* overlap, const long long* records, const long long* info, int nmaps, int max_segments,
                               int min_share, int* link, hipStream_t s);
hipError_t launch_segment_chain(const int* link, const long long* records, const long long* info, int nmaps, int max_segments,
                                int max_tracks, int* ids, long long* tracks, long long* tinfo, hipStream_t s);
hipError_t launch_segment_relabel(const int* segments, const int* ids, const long long* info, int nmaps, int w, int h,
                                  int max_segments, int* track_map, hipStream_t s);
// video stabilisation (include/ofdis.h: ofdis_camera_path, ofdis_warp_frames; ofdis_stabilize.hip).  The window travels in
// the launch, as InterpTimes does: w[0 .. radius], the rest zero
struct StabWindow {
  double w[65];  // OFDIS_STAB_MAX_RADIUS + 1
  double zoom;
  int radius;
};
// models [npairs][6] -> warps [npairs + 1][6], one lane per frame, one launch
hipError_t launch_camera_path(const double* models, int npairs, const StabWindow& win, double* warps, hipStream_t s);
// frames, out [nframes][h][w][noc] u8, warps [nframes][6], inside [nframes][h][w] u8 or null; replicate: OFDIS_BORDER_REPLICATE
hipError_t launch_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w,
                              int h, int noc, bool replicate, hipStream_t s);
// the projective twins (include/ofdis.h: ofdis_camera_path_projective, ofdis_warp_frames_projective): models [npairs][8] of a
// w x h clip -> warps [npairs + 1][8], and the frames under warps [nframes][8]
hipError_t launch_camera_path_projective(const double* models, int npairs, int w, int h, const StabWindow& win, double* warps,
                                         hipStream_t s);
hipError_t launch_warp_frames_projective(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes,
                                         int w, int h, int noc, bool replicate, hipStream_t s);

// ---- stereo-depth mode (SELECTMODE=2; ofdis_de.hip)
struct DeSystemArgs {
  TvGeom t;
  const float* mask;   // row-major [B][h][w]
  const float* wx;     // row-major: the flow before the increment
  const float* du;     // diag: the increment of the previous fixed-point iterations
  int clamp;           // uu = wx (< 0: before the first solve), min(wx + du, 0) (0: left camera), max(., 0) (1: right)
  const float* derivs; // row-major [B][8*noc][h][w]
  float quarter_alpha, half_delta_over3, half_gamma_over3;
  float* sys;          // [B][4][w*h] diag: a11, b1, smooth_horiz, smooth_vert
};
struct DeSorArgs {
  TvGeom t;
  const float* sys;
  float* du;  // diag, in/out
  int iterations;
  float omega;
};
// All fixed-point iterations of a stereo level in one launch (de_fused_kernel, ofdis_de.hip: levels of <= 64 rows): the record
// arrays of the derivatives kernel in, du out (diag plane; never read during the first iteration)
struct DeFusedArgs {
  TvGeom t;
  const float* d8;    // [noc][B][w*h][8] derivative records (zero where the warp's mask is zero)
  const float* wrec;  // [B][w*h][2]: wx (and wy = 0)
  float* du;          // [B][w*h] diag
  float quarter_alpha, half_delta_over3, half_gamma_over3;
  int iterations;     // solver sweeps per fixed-point iteration
  float omega;
  int n_inner;
  int camlr;          // 0: left camera (uu = min(wx + du, 0)), 1: right (max)
};

namespace exact {
#include "ofdis_launchers.inc"
}  // namespace exact
namespace fused {
#include "ofdis_launchers.inc"
}  // namespace fused

}  // namespace ofdis
