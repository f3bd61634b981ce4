// ofdis_launch_hooks.hip -- TEST LIBRARY (libofdis_testhooks.so), not part of the product: thin C wrappers around the
// ofdis::launch_* functions of of_dis_amd/csrc/ofdis_kernels.h, and the two launch limits as variables a test can lower.
//
// The test library links the PRODUCT'S OWN units (TESTHOOK_UNITS of of_dis_amd/build.py has the list), compiled with the
// product's flags plus -DOFDIS_TEST_LAUNCH_LIMITS.  Under that
// define quad_max_blocks() and grid_max_blocks() (ofdis_kernels.h) read the two variables below instead of returning the
// product's constants.  Both are read in host code only (quad_grid, grid_for), so the kernels here are the product's kernels;
// what changes is how many launches (quad_grid's chunks) or grid-stride trips (grid_for) cover the work.  With the limits at
// their product values the launches are the product's.
//
// Every hook is declared in ofdis_test_hooks.h, which also has HOOK, UPG_PARAMS and UPG (UpGeom travels as seven ints).
#include <hip/hip_runtime.h>

#include "../../of_dis_amd/csrc/ofdis_upsample.h"
#include "ofdis_test_hooks.h"

#ifndef OFDIS_TEST_LAUNCH_LIMITS
#error "the test library is compiled with -DOFDIS_TEST_LAUNCH_LIMITS"
#endif

namespace ofdis {
long long test_quad_max_blocks = QUAD_MAX_BLOCKS;
long long test_grid_max_blocks = GRID_MAX_BLOCKS;
}  // namespace ofdis

using namespace ofdis;

static InterpTimes interp_times(const float* times, int ntimes) {
  InterpTimes ts{};
  for (int k = 0; k < ntimes && k < 16; ++k) ts.t[k] = times[k];
  ts.n = ntimes;
  return ts;
}
static TrajWeights traj_weights(const float* weights, int radius) {
  TrajWeights tw{};
  for (int k = 0; k < radius && k < 8; ++k) tw.w[k] = weights[k];
  tw.radius = radius;
  return tw;
}

// ------------------------------------------------------------------------------------ the limits and the host-only geometry
// 0 = the product's value
HOOK void ofdis_test_set_launch_limits(long long quad_max_blocks, long long grid_max_blocks) {
  test_quad_max_blocks = quad_max_blocks > 0 ? quad_max_blocks : QUAD_MAX_BLOCKS;
  test_grid_max_blocks = grid_max_blocks > 0 ? grid_max_blocks : GRID_MAX_BLOCKS;
}
// host only, needs no GPU: quad_grid, quad_blocks, quad_chunks, grid_for and xcd_frame_map for workgroups [n0, n0 + count)
HOOK void ofdis_test_quad_grid(int nframes, int w, int h, int* bpf, int* chunk) {
  const QuadGrid g = quad_grid(nframes, w, h);
  *bpf = g.bpf;
  *chunk = g.chunk;
}
HOOK unsigned ofdis_test_quad_blocks(int frames, int bpf) { return quad_blocks(frames, bpf); }
// quad_chunks with a callback that records instead of launching: (f0, n, workgroups) of the first `cap` launches into
// walk[cap][3]; returns the number of launches, -1 for an error
HOOK int ofdis_test_quad_chunks(int nframes, int w, int h, int cap, int* walk) {
  int count = 0;
  const hipError_t e = quad_chunks(nframes, w, h, [&](const QuadLaunch& q, dim3 blocks) {
    if (count < cap) {
      walk[3 * count] = q.f0;
      walk[3 * count + 1] = q.n;
      walk[3 * count + 2] = (int)blocks.x;
    }
    ++count;
    return hipSuccess;
  });
  return e == hipSuccess ? count : -1;
}
HOOK unsigned ofdis_test_grid_for(long long total) { return grid_for(total); }
HOOK void ofdis_test_xcd_frame_map(int n0, int count, int blocks_per_frame, int nframes, int* frame, int* blk) {
  for (int i = 0; i < count; ++i) xcd_frame_map(n0 + i, blocks_per_frame, nframes, frame[i], blk[i]);
}
// host only, needs no GPU: the core launchers' geometry -- the padded grid xcd_frame_map expects (-1: refused) and the rows per
// frame slot of the kernels that pack frames into a wavefront
HOOK long long ofdis_test_xcd_grid(int nframes, long long blocks_per_frame) {
  dim3 g;
  return xcd_grid(nframes, blocks_per_frame, g) == hipSuccess ? (long long)g.x : -1;
}
HOOK int ofdis_test_slot_rows(int h) { return slot_rows(h); }
// host only, needs no GPU: the patch kernel launch_patch_optimize runs (choose_patch_kernel) for a level of nop patches of
// P x P pixels and noc channels -- out = family (PatchKernel::Family), its four template arguments, lanes per patch, workgroup
// size, workgroups per frame, and whether it honours DisArgs::pixw (what patch_pixel_weights_supported returns)
HOOK void ofdis_test_patch_kernel_choice(int P, int noc, int nop, int stereo, int costfct, int pixw_asked, int gray8, int rgb12,
                                         int rgb12_lpp, int contract, int* out) {
  LevelGeom g{};
  g.P = P;
  g.noc = noc;
  g.nop = nop;
  g.novals = noc * P * P;
  ofdis_tuning tn{};
  tn.gray8 = gray8;
  tn.rgb12 = rgb12;
  tn.rgb12_lpp = rgb12_lpp;
  const PatchKernel k = choose_patch_kernel(g, stereo != 0, costfct, pixw_asked != 0, tn, contract);
  out[0] = k.row < 0 ? (int)PatchKernel::NONE : (int)kPatchKernels[k.row].family;
  for (int q = 0; q < 4; ++q) out[1 + q] = k.row < 0 ? 0 : kPatchKernels[k.row].t[q];
  out[5] = k.lpp;
  out[6] = k.threads;
  out[7] = k.blocks_per_frame;
  out[8] = k.pixw;
}
HOOK size_t ofdis_test_gmotion_work_bytes(int npairs, int w, int h) { return gmotion_work_bytes(npairs, w, h); }
// host only, needs no GPU: the layout classes of the track-description chain for C = nxy^2 nt, as the launchers choose them
// (bof_assign_shape, km_geom) and as km_finish_kernel splits its threads over a channel of n_c entries (km_finish_log2te)
HOOK void ofdis_test_bof_shape(int C, int* nk, int* NK, int* TG) {
  const BofShape s = bof_assign_shape(C);
  *nk = s.nk;
  *NK = s.NK;
  *TG = s.TG;
}
HOOK void ofdis_test_km_geom(int C, int* np, int* el, int* rl) {
  const KmGeom g = km_geom(C);
  *np = g.np;
  *el = g.el;
  *rl = g.rl;
}
HOOK int ofdis_test_km_finish_split(int n_c) { return 1 << km_finish_log2te(n_c); }
// host only, needs no GPU: the kernels the pyramid's launchers pick (ofdis_pyr.hip).  Base level: 0 generic, 4 / 8 / 16 the
// streaming kernel of that block size (`src` is only looked at as an address); planes: 0 generic, 1 gray quads, 2 gray quads
// that write `down` as well
HOOK int ofdis_test_pyr_base_variant(const uint8_t* src, int wo, int W, int noc, int l, size_t pitch, size_t stride) {
  return (int)pyr_base_variant(src, wo, W, noc, l, pitch, stride);
}
HOOK int ofdis_test_pyr_planes_variant(int w, int h, int noc, int pad, int want_down) {
  return (int)pyr_planes_variant(w, h, noc, pad, want_down != 0);
}

// ------------------------------------------------------------------------------------ launchers that walk quad_grid's chunks
HOOK int ofdis_test_launch_interp_frames(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                                         const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int w, int h,
                                         int noc, const float* times, int ntimes, void* stream) {
  return (int)launch_interp_frames(img_a, img_b, flow_fw, flow_rev, mask_fw, mask_rev, out, nframes, w, h, noc,
                                   interp_times(times, ntimes), (hipStream_t)stream);
}
HOOK int ofdis_test_launch_interp_bidir(const uint8_t* img_a, const uint8_t* img_b, const float* fw, const float* rev, uint8_t* out,
                                        int nframes, UPG_PARAMS, int noc, const float* times, int ntimes, float alpha, float beta,
                                        void* stream) {
  return (int)launch_interp_bidir(img_a, img_b, fw, rev, out, nframes, UPG, noc, interp_times(times, ntimes), alpha, beta,
                                  (hipStream_t)stream);
}
HOOK int ofdis_test_launch_tfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                                          const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int w, int h, int noc,
                                          float wn, float tau, void* stream) {
  return (int)launch_tfilter_frames(frames, flow_fw, flow_rev, mask_fw, mask_rev, out, support, npairs, w, h, noc, wn, tau,
                                    (hipStream_t)stream);
}
HOOK int ofdis_test_launch_tfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                         int npairs, UPG_PARAMS, int noc, float wn, float tau, float alpha, float beta,
                                         void* stream) {
  return (int)launch_tfilter_level(frames, fw, rev, out, support, npairs, UPG, noc, wn, tau, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_trajfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out,
                                             uint8_t* support, int npairs, int w, int h, int noc, const float* weights, int radius,
                                             float tau, int fb, float alpha, float beta, void* stream) {
  return (int)launch_trajfilter_frames(frames, flow_fw, flow_rev, out, support, npairs, w, h, noc, traj_weights(weights, radius),
                                       tau, fb != 0, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_trajfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out,
                                            uint8_t* support, int npairs, UPG_PARAMS, int noc, const float* weights, int radius,
                                            float tau, int fb, float alpha, float beta, void* stream) {
  return (int)launch_trajfilter_level(frames, fw, rev, out, support, npairs, UPG, noc, traj_weights(weights, radius), tau, fb != 0,
                                      alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_gmotion_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int model, int rounds,
                                          float thresh, double* models, long long* stats, void* work, void* stream) {
  return (int)launch_gmotion_frames(flow, mask, npairs, w, h, model, rounds, thresh, models, stats, work, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_gmotion_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w,
                                                     int h, float thresh, float* residual, uint8_t* label, void* stream) {
  return (int)launch_gmotion_compensate_frames(flow, mask, models, npairs, w, h, thresh, residual, label, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_gmotion_level(const float* fw, const float* rev, int npairs, UPG_PARAMS, int model, int rounds,
                                         float thresh, float alpha, float beta, double* models, long long* stats, void* work,
                                         void* stream) {
  return (int)launch_gmotion_level(fw, rev, npairs, UPG, model, rounds, thresh, alpha, beta, models, stats, work,
                                   (hipStream_t)stream);
}
HOOK int ofdis_test_launch_gmotion_compensate_level(const float* fw, const float* rev, const double* models, int npairs, UPG_PARAMS,
                                                    float thresh, float alpha, float beta, float* residual, uint8_t* label,
                                                    void* stream) {
  return (int)launch_gmotion_compensate_level(fw, rev, models, npairs, UPG, thresh, alpha, beta, residual, label,
                                              (hipStream_t)stream);
}
HOOK int ofdis_test_launch_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w,
                                       int h, int noc, int replicate, void* stream) {
  return (int)launch_warp_frames(frames, warps, out, inside, nframes, w, h, noc, replicate != 0, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ launchers behind grid_for
HOOK int ofdis_test_launch_pyr_base(const uint8_t* src, float* dst, int nframes, int wo, int ho, int W, int H, int noc, int l,
                                    size_t pitch, size_t stride, void* stream) {
  return (int)launch_pyr_base(src, dst, nframes, wo, ho, W, H, noc, l, pitch, stride, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_pyr_down(const float* src, float* dst, int nframes, int w, int h, int noc, void* stream) {
  return (int)launch_pyr_down(src, dst, nframes, w, h, noc, (hipStream_t)stream);
}
// (grid = (chunks of a frame, frames), no grid_for: here for the comparison with tests/pyr_ref.py, tests/test_gpu_pyramid.py)
HOOK int ofdis_test_launch_pyr_planes(const float* src, float* img, float* dx, float* dy, float* down, int nframes, int w, int h,
                                      int noc, int pad, void* stream) {
  return (int)launch_pyr_planes(src, img, dx, dy, nframes, w, h, noc, pad, (hipStream_t)stream, down);
}
HOOK int ofdis_test_launch_encode(const float* src, void* dst, size_t n, int type, float scale, float offset, void* stream) {
  return (int)launch_encode(src, dst, n, type, scale, offset, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_fb_check(const float* flow, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                                    float beta, void* stream) {
  return (int)launch_fb_check(flow, other, mask, nframes, w, h, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_mirror_u8(const uint8_t* src, uint8_t* dst, int nframes, int w, int h, int noc, void* stream) {
  return (int)launch_mirror_u8(src, dst, nframes, w, h, noc, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_lr_check(const float* disp, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                                    float beta, void* stream) {
  return (int)launch_lr_check(disp, other, mask, nframes, w, h, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int w, int h, int mode,
                                          void* stream) {
  return (int)launch_disparity_fill(disp, mask, out, nframes, w, h, mode, (hipStream_t)stream);
}
