/* ofdis_test_hooks.h -- TEST LIBRARY (libofdis_testhooks.so), not part of the product: every function the library exports,
 * declared once as plain C.
 *
 * The five hook files beside this header (ofdis_testhooks.hip, ofdis_launch_hooks*.hip) include it and define their functions
 * as extern "C" (HOOK): a definition whose parameter list disagrees with its declaration here does not compile.  The Python
 * side (tests/common.py: testhooks) reads its ctypes prototypes from this text with the parser that binds the product
 * (of_dis_amd/abi.py), and tests/test_testhooks_abi.py holds the declarations to the library's symbol table, so a definition
 * that is not extern "C", or has no declaration here, fails there.
 *
 * The declarations stay free of macros and attributes, for that parser: the pragma exports them under -fvisibility=hidden, and
 * UpGeom travels as seven ints written out in the order of its members. */
#ifndef OFDIS_TEST_HOOKS_H_
#define OFDIS_TEST_HOOKS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
/* for the definitions: the linkage of the declarations below, and UpGeom's seven ints as parameters and as the struct */
#define HOOK extern "C"
#define UPG_PARAMS int sw, int sh, int sc_l, int left, int top, int wo, int ho
#define UPG (UpGeom{sw, sh, sc_l, left, top, wo, ho})
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- ofdis_testhooks.hip: device kernels around the header-only helpers of ofdis_dev.h, and the host-side outlier threshold */
int ofdis_test_wave_sum(const float* in, float* out, int n, void* stream);
int ofdis_test_div_sqrt(const float* a, const float* b, float* out, int n, void* stream);
float ofdis_test_outlier_sq(float t);

/* ---- ofdis_launch_hooks.hip: the two launch limits (0 = the product's value) and the host-only geometry */
void ofdis_test_set_launch_limits(long long quad_max_blocks, long long grid_max_blocks);
void ofdis_test_quad_grid(int nframes, int w, int h, int* bpf, int* chunk);
unsigned ofdis_test_quad_blocks(int frames, int bpf);
int ofdis_test_quad_chunks(int nframes, int w, int h, int cap, int* walk);
unsigned ofdis_test_grid_for(long long total);
void ofdis_test_xcd_frame_map(int n0, int count, int blocks_per_frame, int nframes, int* frame, int* blk);
long long ofdis_test_xcd_grid(int nframes, long long blocks_per_frame);
int ofdis_test_slot_rows(int h);
void ofdis_test_patch_kernel_choice(int P, int noc, int nop, int stereo, int costfct, int pixw_asked, int gray8, int rgb12,
                                    int rgb12_lpp, int contract, int* out);
size_t ofdis_test_gmotion_work_bytes(int npairs, int w, int h);
void ofdis_test_bof_shape(int C, int* nk, int* NK, int* TG);
void ofdis_test_km_geom(int C, int* np, int* el, int* rl);
int ofdis_test_km_finish_split(int n_c);
int ofdis_test_pyr_base_variant(const uint8_t* src, int wo, int W, int noc, int l, size_t pitch, size_t stride);
int ofdis_test_pyr_planes_variant(int w, int h, int noc, int pad, int want_down);

/* ---- ofdis_launch_hooks.hip: launchers that walk quad_grid's chunks; every ofdis_test_launch_* returns a hipError_t */
int ofdis_test_launch_interp_frames(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                                    const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int w, int h,
                                    int noc, const float* times, int ntimes, void* stream);
int ofdis_test_launch_interp_bidir(const uint8_t* img_a, const uint8_t* img_b, const float* fw, const float* rev, uint8_t* out,
                                   int nframes, int sw, int sh, int sc_l, int left, int top, int wo, int ho, int noc,
                                   const float* times, int ntimes, float alpha, float beta, void* stream);
int ofdis_test_launch_tfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                                     const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int w, int h, int noc,
                                     float wn, float tau, void* stream);
int ofdis_test_launch_tfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                    int npairs, int sw, int sh, int sc_l, int left, int top, int wo, int ho, int noc, float wn,
                                    float tau, float alpha, float beta, void* stream);
int ofdis_test_launch_trajfilter_frames(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out,
                                        uint8_t* support, int npairs, int w, int h, int noc, const float* weights, int radius,
                                        float tau, int fb, float alpha, float beta, void* stream);
int ofdis_test_launch_trajfilter_level(const uint8_t* frames, const float* fw, const float* rev, uint8_t* out, uint8_t* support,
                                       int npairs, int sw, int sh, int sc_l, int left, int top, int wo, int ho, int noc,
                                       const float* weights, int radius, float tau, int fb, float alpha, float beta,
                                       void* stream);
int ofdis_test_launch_gmotion_frames(const float* flow, const uint8_t* mask, int npairs, int w, int h, int model, int rounds,
                                     float thresh, double* models, long long* stats, void* work, void* stream);
int ofdis_test_launch_gmotion_compensate_frames(const float* flow, const uint8_t* mask, const double* models, int npairs, int w,
                                                int h, float thresh, float* residual, uint8_t* label, void* stream);
int ofdis_test_launch_gmotion_level(const float* fw, const float* rev, int npairs, int sw, int sh, int sc_l, int left, int top,
                                    int wo, int ho, int model, int rounds, float thresh, float alpha, float beta, double* models,
                                    long long* stats, void* work, void* stream);
int ofdis_test_launch_gmotion_compensate_level(const float* fw, const float* rev, const double* models, int npairs, int sw, int sh,
                                               int sc_l, int left, int top, int wo, int ho, float thresh, float alpha, float beta,
                                               float* residual, uint8_t* label, void* stream);
int ofdis_test_launch_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w,
                                  int h, int noc, int replicate, void* stream);

/* ---- ofdis_launch_hooks.hip: launchers behind grid_for (pyr_planes: grid = (chunks of a frame, frames), no grid_for) */
int ofdis_test_launch_pyr_base(const uint8_t* src, float* dst, int nframes, int wo, int ho, int W, int H, int noc, int l,
                               size_t pitch, size_t stride, void* stream);
int ofdis_test_launch_pyr_down(const float* src, float* dst, int nframes, int w, int h, int noc, void* stream);
int ofdis_test_launch_pyr_planes(const float* src, float* img, float* dx, float* dy, float* down, int nframes, int w, int h,
                                 int noc, int pad, void* stream);
int ofdis_test_launch_encode(const float* src, void* dst, size_t n, int type, float scale, float offset, void* stream);
int ofdis_test_launch_fb_check(const float* flow, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                               float beta, void* stream);
int ofdis_test_launch_mirror_u8(const uint8_t* src, uint8_t* dst, int nframes, int w, int h, int noc, void* stream);
int ofdis_test_launch_lr_check(const float* disp, const float* other, uint8_t* mask, int nframes, int w, int h, float alpha,
                               float beta, void* stream);
int ofdis_test_launch_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int w, int h, int mode,
                                     void* stream);

/* ---- ofdis_launch_hooks_levels.hip: the level-flow finish launchers with a free UpGeom */
int ofdis_test_launch_upsample_crop_enc(const float* flow, void* out, int nframes, int sw, int sh, int sc_l, int left, int top,
                                        int wo, int ho, int channels, int type, float scale, float offset, void* stream);
int ofdis_test_launch_upsample_bidir(const float* fw, const float* rev, float* out_fw, float* out_rev, uint8_t* mask_fw,
                                     uint8_t* mask_rev, int nframes, int sw, int sh, int sc_l, int left, int top, int wo, int ho,
                                     float alpha, float beta, void* stream);
int ofdis_test_launch_projective_level(const float* fw, const float* rev, int npairs, int sw, int sh, int sc_l, int left, int top,
                                       int wo, int ho, int rounds, float thresh, float alpha, float beta, double* models,
                                       long long* stats, void* work, void* stream);
int ofdis_test_launch_projective_compensate_level(const float* fw, const float* rev, const double* models, int npairs, int sw,
                                                  int sh, int sc_l, int left, int top, int wo, int ho, float thresh, float alpha,
                                                  float beta, float* residual, uint8_t* label, void* stream);
int ofdis_test_launch_track_level(const float* fw, const float* rev, int npairs, int sw, int sh, int sc_l, int left, int top,
                                  int wo, int ho, const float* seeds, const int* seed_frame, int npoints, int max_steps,
                                  float alpha, float beta, float* tracks, int* counts, void* stream);
int ofdis_test_launch_dense_tracks_level(const uint8_t* frames, const float* fw, const float* rev, int npairs, int sw, int sh,
                                         int sc_l, int left, int top, int wo, int ho, int noc, int stride, int window, int min_eig,
                                         int max_len, float alpha, float beta, int max_tracks, float* tracks, int* start, int* len,
                                         long long* info, void* work, void* stream);
int ofdis_test_launch_upsample_lr(const float* fw, const float* mir, float* out_l, float* out_r, uint8_t* mask_l, uint8_t* mask_r,
                                  int nframes, int sw, int sh, int sc_l, int left, int top, int wo, int ho, int fill_mode,
                                  float alpha, float beta, void* stream);
int ofdis_test_launch_lr_materialise(const float* fw, const float* mir, float* u, float* dr, int nframes, int sw, int sh, int sc_l,
                                     int left, int top, int wo, int ho, void* stream);
int ofdis_test_upsample_lr_fuses(int wo);

/* ---- ofdis_launch_hooks_projective.hip */
int ofdis_test_launch_warp_frames_projective(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside,
                                             int nframes, int w, int h, int noc, int replicate, void* stream);

/* ---- ofdis_launch_hooks_segments.hip */
size_t ofdis_test_segments_work_bytes(int nmaps, int w, int h);
int ofdis_test_launch_label_segments(const uint8_t* label, const float* flow, int nmaps, int w, int h, unsigned codes, int conn,
                                     int min_area, int max_segments, int* segments, long long* records, long long* info,
                                     void* work, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* OFDIS_TEST_HOOKS_H_ */
