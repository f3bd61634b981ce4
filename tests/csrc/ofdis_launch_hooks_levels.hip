// ofdis_launch_hooks_levels.hip -- the launch hooks of the level-flow finish launchers that ofdis_launch_hooks.hip does not
// have (of_dis_amd/csrc/ofdis_kernels.h: the upsample, the projective camera models, the point and dense trajectories and the
// stereo left-right finish), linked into the TEST library beside ofdis_launch_hooks.hip, which owns the two launch limits.
// tests/test_gpu_level_routes.py calls every level route through these and the five level hooks there with a free UpGeom.
#include <hip/hip_runtime.h>

#include "../../of_dis_amd/csrc/ofdis_kernels.h"
#include "ofdis_test_hooks.h"

#ifndef OFDIS_TEST_LAUNCH_LIMITS
#error "the test library is compiled with -DOFDIS_TEST_LAUNCH_LIMITS"
#endif

using namespace ofdis;

// (OFDIS_ENC_F32 with two channels is launch_upsample_crop)
HOOK int ofdis_test_launch_upsample_crop_enc(const float* flow, void* out, int nframes, UPG_PARAMS, int channels, int type,
                                             float scale, float offset, void* stream) {
  return (int)launch_upsample_crop_enc(flow, out, nframes, UPG, channels, type, scale, offset, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_upsample_bidir(const float* fw, const float* rev, float* out_fw, float* out_rev, uint8_t* mask_fw,
                                          uint8_t* mask_rev, int nframes, UPG_PARAMS, float alpha, float beta, void* stream) {
  return (int)launch_upsample_bidir(fw, rev, out_fw, out_rev, mask_fw, mask_rev, nframes, UPG, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_projective_level(const float* fw, const float* rev, int npairs, UPG_PARAMS, int rounds, float thresh,
                                            float alpha, float beta, double* models, long long* stats, void* work, void* stream) {
  return (int)launch_projective_level(fw, rev, npairs, UPG, rounds, thresh, alpha, beta, models, stats, work, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_projective_compensate_level(const float* fw, const float* rev, const double* models, int npairs,
                                                       UPG_PARAMS, float thresh, float alpha, float beta, float* residual,
                                                       uint8_t* label, void* stream) {
  return (int)launch_projective_compensate_level(fw, rev, models, npairs, UPG, thresh, alpha, beta, residual, label,
                                                 (hipStream_t)stream);
}
HOOK int ofdis_test_launch_track_level(const float* fw, const float* rev, int npairs, UPG_PARAMS, const float* seeds,
                                       const int* seed_frame, int npoints, int max_steps, float alpha, float beta, float* tracks,
                                       int* counts, void* stream) {
  return (int)launch_track_level(fw, rev, npairs, UPG, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks, counts,
                                 (hipStream_t)stream);
}
HOOK int ofdis_test_launch_dense_tracks_level(const uint8_t* frames, const float* fw, const float* rev, int npairs, UPG_PARAMS,
                                              int noc, int stride, int window, int min_eig, int max_len, float alpha, float beta,
                                              int max_tracks, float* tracks, int* start, int* len, long long* info, void* work,
                                              void* stream) {
  return (int)launch_dense_tracks_level(frames, fw, rev, npairs, UPG, noc, stride, window, min_eig, max_len, alpha, beta, max_tracks,
                                        tracks, start, len, info, work, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_upsample_lr(const float* fw, const float* mir, float* out_l, float* out_r, uint8_t* mask_l,
                                       uint8_t* mask_r, int nframes, UPG_PARAMS, int fill_mode, float alpha, float beta,
                                       void* stream) {
  return (int)launch_upsample_lr(fw, mir, out_l, out_r, mask_l, mask_r, nframes, UPG, fill_mode, alpha, beta, (hipStream_t)stream);
}
HOOK int ofdis_test_launch_lr_materialise(const float* fw, const float* mir, float* u, float* dr, int nframes, UPG_PARAMS,
                                          void* stream) {
  return (int)launch_lr_materialise(fw, mir, u, dr, nframes, UPG, (hipStream_t)stream);
}
// host only, needs no GPU: which form ofdis_batch_upsample_lr takes at original width wo
HOOK int ofdis_test_upsample_lr_fuses(int wo) { return upsample_lr_fuses(wo) ? 1 : 0; }
