/* ofdis.h -- C ABI of the MI355X-native OF_DIS hot path (libofdis_hip.so).
 *
 * The reference has exactly one API: the constructor of OFC::OFClass
 * (reference oflow.h:84-111, definition oflow.cpp:32-363, sole call site run_dense.cpp:391-400).
 * Everything happens inside that constructor; nothing is retained afterwards.  ofdis_flow() below
 * is that constructor as a C function (same argument meaning, same buffers, same output), and
 * ofdis_batch_* is the same computation over many independent frame pairs resident in HBM, which
 * is how a GPU reaches throughput on problems this small.
 *
 * Plain pointers and sizes only; no C++/torch types.  Device pointers are HIP device pointers,
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *
 * TWO arithmetic contracts, one source.  A context fixes its contract at creation (ofdis_tuning::contract,
 * OFDIS_CONTRACT=fused in the environment); everything else in this header holds for both.
 *   exact (0, the LIBRARY default; run_OF_* / ofdis_flow use it unless told otherwise): fp32 throughout, every operation
 *     separately rounded (no FMA contraction), IEEE divide/sqrt, same operation order as the reference's SSE path; vector
 *     reductions (the only place the reference leaves the order to Eigen) use the order documented in DESIGN.md
 *     ("Reduction order": <= 64 entries: 8 stride-8 partials, then distance 4, 1, 2; more: 64 strided partials, then a
 *     butterfly at distance 1..32).  The result is bit-identical to the reference sources compiled against
 *     oracle/eigen_shim with -DOFDIS_SHIM_WAVE64, whatever kernel mapping the batch size selects.
 *   fused (1, what `python bench.py` TIMES by default, after its gate passed in that run): the tolerance contract of
 *     BASELINE.json's north star.  Same algorithm, taps, control flow and reduction shapes; multiply-adds contract to
 *     v_fma_f32 and quotients / roots are the hardware's 1-ulp v_rcp_f32 / v_rsq_f32 / v_sqrt_f32.  Bound (asserted in
 *     tests/test_gpu_contract.py against the PLAIN reference build, sequential sums): mean EPE < 1e-4 px and max EPE <
 *     1e-3 px on the full-resolution flow.  Results then depend on the kernel mapping (i.e. on the batch size) by up to
 *     3e-4 px; they stay deterministic and independent of a frame's slot and neighbours.
 */
#ifndef OFDIS_H_
#define OFDIS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  2 (round 5): ofdis_tuning grew to 16 ints (fused_tp_pipe, fused_xcu_spin, contract were appended in round 4
 * without a bump), ofdis_batch_status and ofdis_batch_upsample_frames were added.  3 (round 6): streams, pinned host memory
 * asynchronous copies and events (ofdis_stream_create, ofdis_host_alloc, ofdis_memcpy_h2d_async / _d2h_async,
 * ofdis_event_*), ofdis_build_id; ofdis_tuning grew to
 * 20 ints (fused_xcu_drop, prep_densify, fused_tall_group, fused_rgb_min) and fused_xcu_spin became a time in microseconds
 * (round 8 appended patch_window_reuse, 21 ints, without a bump: a caller compiled against the 20-int struct must be rebuilt).  A caller checks ofdis_version() ==
 * OFDIS_VERSION before passing structs (of_dis_amd/capi.py does at load). */
#define OFDIS_VERSION 3

/* status codes (the reference reports nothing and has UB on bad input; we return a status) */
enum {
  OFDIS_OK = 0,
  OFDIS_ERR_INVALID = -1,      /* bad argument / unsupported parameter combination */
  OFDIS_ERR_UNSUPPORTED = -2,  /* valid in the reference but outside this path */
  OFDIS_ERR_DEVICE = -3,       /* HIP runtime error (ofdis_last_error() has the text) */
  OFDIS_ERR_NOMEM = -4
};

/* The run-time parameters of OFC::OFClass::OFClass, in the constructor's order
 * (oflow.h:91-111; parsed at oflow.cpp:76-108).  `noc` is a run-time value here instead of the
 * reference's per-binary SELECTCHANNEL. */
typedef struct ofdis_params {
  int   width, height;      /* size of level 0 (already padded to a multiple of 2^sc_f), oflow.h:92 */
  int   imgpadding;         /* border of every pyramid plane, == p_samp_s at the call site (run_dense.cpp:393) */
  int   sc_f, sc_l;         /* coarsest / finest pyramid level used */
  int   max_iter, min_iter;
  float dp_thresh, dr_thresh, res_thresh;
  int   p_samp_s;           /* patch edge length P */
  float patove;             /* patch overlap in [0,1) */
  int   usefbcon;           /* forward-backward merging (oflow.cpp:162-170, patchgrid.cpp:277-375) */
  int   costfct;            /* 0 L2, 1 L1, 2 pseudo-Huber (patch.cpp:230-261) */
  int   noc;                /* channels: 1 (run_OF_INT) or 3 (run_OF_RGB) */
  int   patnorm;            /* subtract patch mean */
  int   usetvref;           /* TV-L1 variational refinement on/off */
  float tv_alpha, tv_gamma, tv_delta;
  int   tv_innerit, tv_solverit;
  float tv_sor;
  int   verbosity;          /* 0 silent, 1 total time, 2 per-level TIME lines (oflow.cpp:179,303,359) */
  int   selectmode;         /* the reference's compile-time SELECTMODE: 0 or 1 = optical flow (run_OF_*, two flow
                             * channels), 2 = stereo depth (run_DE_*: ONE channel = horizontal displacement <= 0,
                             * patch.cpp:188-193, refine_variational.cpp:245-336).  Every flow array below then has
                             * one float per pixel instead of two. */
} ofdis_params;

/* Fill `p` with the reference's operating point 1..4 for an image of `width_org` columns
 * (run_dense.cpp:225-265, AutoFirstScaleSelect run_dense.cpp:180-183).  width/height/imgpadding are
 * set by the caller after padding.  Returns OFDIS_OK or OFDIS_ERR_INVALID. */
int ofdis_params_oppoint(ofdis_params* p, int op_point, int width_org, int noc);

const char* ofdis_last_error(void);
int ofdis_version(void);
/* Identity of the kernels in this library: a hash over the kernel sources and compiler flags it was built from
 * (of_dis_amd/build.py: source_id).  Counter-derived measurements (profiles/traffic_*.json) carry the id of the library
 * they were collected on; bench.py attaches them only to a library with the same id. */
const char* ofdis_build_id(void);
/* number of HIP devices visible / select one (one process per GPU: call once at start) */
int ofdis_device_count(void);
int ofdis_set_device(int device);
/* PCI bus id ("0000:c1:00.0") of a visible device into buf (at least 16 bytes): a multi-rank launcher can check that the
 * ranks really sit on different GPUs */
int ofdis_device_pci_bus_id(int device, char* buf, int len);

/* ---------------------------------------------------------------------------------------------
 * Drop-in for the constructor: host pointers in, host flow out, synchronous.
 * Replaces: OFC::OFClass::OFClass(...) oflow.h:84-111 / run_dense.cpp:391-400.
 * im_*: arrays of sc_f+1 host pointers; entries sc_l..sc_f must be valid (oflow.h:85-87).  Each
 * plane is row-major fp32, (w/2^l + 2*imgpadding) x (h/2^l + 2*imgpadding) x noc, channel
 * interleaved, images replicate-padded, gradients zero-padded (run_dense.cpp:166-175).
 * im_b_dx / im_b_dy may be NULL when usefbcon == 0 (never read then).
 * outflow: 2*(w>>sc_l)*(h>>sc_l) floats, AoS (u,v), fully overwritten.
 * initflow: optional (w>>(sc_f+1))*(h>>(sc_f+1))*2 floats or NULL (oflow.cpp:217-220).
 * ------------------------------------------------------------------------------------------- */
int ofdis_flow(const ofdis_params* p,
               const float* const* im_a, const float* const* im_a_dx, const float* const* im_a_dy,
               const float* const* im_b, const float* const* im_b_dx, const float* const* im_b_dy,
               float* outflow, const float* initflow);
/* ofdis_flow keeps the device contexts of the last few parameter sets (buffers, a stream, pinned staging) so that a loop over frame pairs -- the reference's usage, one constructor per pair -- pays for them
 * once; calls are serialised internally.  ofdis_flow_cache_clear() releases them (e.g. before hipDeviceReset or at
 * shutdown); the next ofdis_flow() builds a fresh one. */
void ofdis_flow_cache_clear(void);

/* ---------------------------------------------------------------------------------------------
 * Batched, device-resident form (the throughput path).
 * A batch context owns every intermediate buffer for `nframes` frame pairs of one geometry.
 * Pyramid layout in HBM, per level l in [sc_l, sc_f], one array per plane kind:
 *     float plane[nframes][tmp_h_l][tmp_w_l][noc]    tmp_* = level size + 2*imgpadding
 * i.e. the reference's per-level plane, frame-major.  Output: float flow[nframes][h_l][w_l][2]
 * at l = sc_l.
 * ------------------------------------------------------------------------------------------- */
typedef struct ofdis_batch ofdis_batch;

/* nframes: 1..65535.  All device memory of the context is one allocation.  Same as ofdis_batch_create_ex(out, p, nframes, 0). */
int ofdis_batch_create(ofdis_batch** out, const ofdis_params* p, int nframes);
void ofdis_batch_destroy(ofdis_batch* b);

/* ---------------------------------------------------------------------------------------------
 * Bidirectional flow and forward-backward occlusion masks (the consistency check of Sundaram, Brox and Keutzer, 2010).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_BATCH_REVERSE 1u          /* flag of ofdis_batch_create_ex */
#define OFDIS_FB_ALPHA 0.01f            /* defaults of the consistency test */
#define OFDIS_FB_BETA  0.5f
enum { OFDIS_FB_CONSISTENT = 0, OFDIS_FB_INCONSISTENT = 1, OFDIS_FB_OUTSIDE = 2 };

/* flags = 0 is ofdis_batch_create.  Unknown flag bits: OFDIS_ERR_INVALID.
 * OFDIS_BATCH_REVERSE: the context also computes the REVERSE flow B -> A of every pair.  It allocates B's gradient planes
 * (input kinds 4 and 5, filled by ofdis_batch_build_pyramids_u8 or ofdis_batch_upload_b_gradients) whatever usefbcon says, and
 * per-level reverse flow buffers; all other scratch is shared.  ofdis_batch_run then runs the coarse-to-fine pass twice on
 * `stream`: first forward, exactly as a plain context, then on the swapped pair.  Frame k's reverse flow (every level) is
 * bit-identical to the forward flow that a plain context of the same nframes, params, contract and pipelining computes for
 * the pair (B_k, A_k); the forward flow is bit-identical to a plain context's.  Pipelining, graph replay, kernel timing and
 * ofdis_batch_status cover both passes (a lost hand-over of the cross-CU TV variant in either fails the pass).
 * Stereo depth (selectmode 2) with OFDIS_BATCH_REVERSE: OFDIS_ERR_UNSUPPORTED, whatever other bits are set -- the second view
 * of a stereo pair is OFDIS_BATCH_STEREO_LR (below: "Stereo depth: right-view disparity ..."). */
int ofdis_batch_create_ex(ofdis_batch** out, const ofdis_params* p, int nframes, unsigned flags);
/* The reverse results of an OFDIS_BATCH_REVERSE context, laid out as ofdis_batch_flow / ofdis_batch_level_flow /
 * ofdis_batch_download; NULL or OFDIS_ERR_INVALID on a context created without the flag. */
const float* ofdis_batch_flow_reverse(const ofdis_batch* b);
const float* ofdis_batch_level_flow_reverse(const ofdis_batch* b, int level);
int ofdis_batch_download_reverse(ofdis_batch* b, int frame, float* outflow_host, void* stream);
/* Warm start of the reverse direction: borrows a device array laid out as for ofdis_batch_set_initflow (which stays
 * forward-only); NULL = zero flow.  OFDIS_ERR_INVALID on a context created without OFDIS_BATCH_REVERSE. */
int ofdis_batch_set_initflow_reverse(ofdis_batch* b, const float* initflow_dev);
/* One launch over the frames [first_frame, first_frame + count) of an OFDIS_BATCH_REVERSE context: out_fw / out_rev =
 * device [count][height_org][width_org][2], bit-identical to what ofdis_batch_upsample_frames makes of the forward flow
 * (and a plain context on the swapped pairs of the reverse flow); mask_fw / mask_rev = device [count][height_org][width_org]
 * bytes, bit-identical to ofdis_fb_check(fw, rev) and ofdis_fb_check(rev, fw) on those materialised flows.  Any of the four
 * outputs may be NULL (not written).  alpha, beta: as for ofdis_fb_check.  Joins a pipelined pass by itself. */
int ofdis_batch_upsample_bidir(ofdis_batch* b, int first_frame, int count, float* out_fw, float* out_rev,
                               uint8_t* mask_fw, uint8_t* mask_rev, int width_org, int height_org,
                               float alpha, float beta, void* stream);
/* The forward-backward consistency test on device arrays of AoS flows [nframes][height][width][2]: one byte per pixel of
 * `flow` (the image `flow` starts in) into `mask` [nframes][height][width].  For pixel (x, y) with (u, v) = flow, every
 * operation a separately rounded fp32 operation in this order:
 *   xb = x + u, yb = y + v; not (0 <= xb <= W-1 and 0 <= yb <= H-1) (NaN included): OFDIS_FB_OUTSIDE
 *   x0 = floor(xb) clamped to W-2 (x0 = 0, ax = 0 when W == 1), ax = xb - x0, x1 = min(x0+1, W-1); the same for y
 *   r = (R[y0][x0]*(1-ax) + R[y0][x1]*ax) * (1-ay) + (R[y1][x0]*(1-ax) + R[y1][x1]*ax) * ay   (R = flow_other, per component)
 *   du = u + ru, dv = v + rv; lhs = du*du + dv*dv; rhs = alpha * ((u*u + v*v) + (ru*ru + rv*rv)) + beta
 *   lhs <= rhs: OFDIS_FB_CONSISTENT, else OFDIS_FB_INCONSISTENT
 * Independent of the arithmetic contract.  Invalid sizes, or alpha / beta negative or not finite: OFDIS_ERR_INVALID. */
int ofdis_fb_check(const float* flow, const float* flow_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stereo depth: right-view disparity, left-right check and occlusion fill.
 *
 * Let mir(I)[y][x] = I[y][W-1-x] on the original 8-bit W x H frames (all channels of a pixel together).  For a pair (L, R) the
 * MIRROR PASS is the ordinary stereo pass (left camera, displacement <= 0) on the pair (A', B') = (mir(R), mir(L)); Dm is its
 * full-resolution result.  The right-view disparity is DR[y][x] = -Dm[y][W-1-x] (>= 0): pixel (x, y) of R shows what L shows
 * at x + DR.  The left-view result DL (<= 0) is what a plain stereo context computes.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_BATCH_STEREO_LR 2u        /* flag of ofdis_batch_create_ex */
enum { OFDIS_FILL_NONE = 0, OFDIS_FILL_INVALIDATE = 1, OFDIS_FILL_BACKGROUND = 2 };
#define OFDIS_LR_FUSED_MAX_WIDTH 4096   /* ofdis_batch_upsample_lr: widest original frame the one-launch kernel takes */
/* OFDIS_BATCH_STEREO_LR is valid with selectmode 2 only (any other selectmode: OFDIS_ERR_INVALID).  The context allocates a
 * second set of input planes for (A', B') -- ofdis_batch_input kinds 6 = A', 7 = A'_dx, 8 = A'_dy, 9 = B' (with usefbcon also
 * 10 = B'_dx, 11 = B'_dy) -- and per-level mirror disparity buffers; all other scratch is shared.
 * ofdis_batch_build_pyramids_u8 also builds the mirror planes, from mir(img_b) and mir(img_a): the pyramid of a mirrored frame
 * is not the mirror of the pyramid (one-sided padding, the sign of dx, the downsampling phase), so they hold the bits the same
 * call on a plain context given host-mirrored, swapped frames produces.  ofdis_batch_run runs the forward pass exactly as a
 * plain context does, then the mirror pass on `stream`: every level of it is bit-identical to what a plain stereo context of
 * the same nframes, params, contract and pipelining computes from the mirrored, swapped frames.  Pipelining, graph replay,
 * kernel timing and ofdis_batch_status cover both passes.  The warm start stays forward-only: ofdis_batch_set_initflow /
 * ofdis_batch_upload_initflow warm-start the forward pass, the mirror pass always starts from zero.
 *
 * The raw mirror-pass disparities (MIRRORED coordinates, <= 0), laid out as ofdis_batch_flow / ofdis_batch_level_flow.  They
 * exist for the parity tests; applications take ofdis_batch_upsample_lr.  NULL on a context created without the flag. */
const float* ofdis_batch_flow_mirror(const ofdis_batch* b);
const float* ofdis_batch_level_flow_mirror(const ofdis_batch* b, int level);
/* The left-right consistency test on device arrays [nframes][height][width], one float per pixel: the displacement in x
 * towards the other view (left view <= 0, right view >= 0).  One byte per pixel of `disp` into `mask`, codes OFDIS_FB_*.  For
 * pixel (x, y) with d = disp, every operation a separately rounded fp32 operation in this order:
 *   xb = x + d;  not (0 <= xb <= W-1) (NaN included): OFDIS_FB_OUTSIDE
 *   x0 = min(floor(xb), W-2), ax = xb - x0  (x0 = 0, ax = 0 when W == 1);  x1 = min(x0+1, W-1)
 *   r = R[y][x0]*(1-ax) + R[y][x1]*ax                    (R = disp_other, same row)
 *   s = d + r;  lhs = s*s;  rhs = alpha*(d*d + r*r) + beta;  lhs <= rhs: OFDIS_FB_CONSISTENT, else OFDIS_FB_INCONSISTENT
 * i.e. the test of ofdis_fb_check with v = 0 and the vertical blend dropped: for finite inputs the same codes as ofdis_fb_check
 * on the flows (d, 0).  Independent of the arithmetic contract.  Argument errors as ofdis_fb_check. */
int ofdis_lr_check(const float* disp, const float* disp_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream);
/* What to do with the pixels a mask flags (mask != OFDIS_FB_CONSISTENT); device arrays as above, `out` may be `disp`.
 *   OFDIS_FILL_NONE        out = disp
 *   OFDIS_FILL_INVALIDATE  out = +inf where flagged (the "unknown" of Middlebury .pfm files), else disp bit for bit
 *   OFDIS_FILL_BACKGROUND  a flagged pixel x takes its value from the nearest consistent pixels of its row: l the largest
 *                          x' < x and r the smallest x' > x with mask == OFDIS_FB_CONSISTENT.  Both exist:
 *                          out = fabsf(d[l]) <= fabsf(d[r]) ? d[l] : d[r] (the farther surface; the left one on a tie); one
 *                          exists: that one; the row has none: out = disp.  Consistent pixels are copied bit for bit.
 * No arithmetic is involved: the result is a pure function of the inputs.  Any other mode, NULL pointers or bad sizes:
 * OFDIS_ERR_INVALID before any device work. */
int ofdis_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int width, int height, int mode,
                         void* stream);
/* The fused finish of an OFDIS_BATCH_STEREO_LR context, one launch over the frames [first_frame, first_frame + count):
 * out_left / out_right = device [count][height_org][width_org] floats, mask_left / mask_right = the same shape in bytes; any
 * of the four may be NULL (not written).  Bit-identical to the materialised composition
 *   U = ofdis_batch_upsample_frames of the forward disparity; Dm = the same upsample of the mirror disparity;
 *   DR[y][x] = -Dm[y][width_org-1-x];
 *   mask_left = ofdis_lr_check(U, DR), mask_right = ofdis_lr_check(DR, U)     (always of the UNFILLED disparities)
 *   out_left = ofdis_disparity_fill(U, mask_left, fill_mode), out_right = ofdis_disparity_fill(DR, mask_right, fill_mode)
 * A wavefront builds a row of U and DR in LDS from the level disparities, checks both against each other there, fills and
 * writes each output once.  Original widths above OFDIS_LR_FUSED_MAX_WIDTH take the composition itself (several launches,
 * staging buffers owned by the context).  Joins a pipelined pass by itself.  OFDIS_ERR_INVALID: a context created without
 * OFDIS_BATCH_STEREO_LR, a frame range outside the batch, an original size above the padded size, a fill mode that does not
 * exist, alpha / beta as ofdis_fb_check rejects them. */
int ofdis_batch_upsample_lr(ofdis_batch* b, int first_frame, int count, float* out_left, float* out_right,
                            uint8_t* mask_left, uint8_t* mask_right, int fill_mode, int width_org, int height_org,
                            float alpha, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame interpolation from bidirectional flow with occlusion masks.
 *
 * Inputs per frame pair k: 8-bit frames A, B of size W x H x noc (noc 1 or 3, channels interleaved, BGR as the binaries use
 * it); full-resolution flows F01 (A -> B) and F10 (B -> A), each [H][W][2] fp32; optionally the masks M01 and M10
 * (OFDIS_FB_* codes); times t_0 ... t_{n-1}.  For every output pixel (x, y) and time t, every operation is a separately
 * rounded fp32 operation in this order:
 *   (u0,v0) = F01[y][x]      (u1,v1) = F10[y][x]
 *   s = 1 - t;  a = s * t;  tt = t * t;  ss = s * s
 *   ft0x = tt*u1 - a*u0;  ft0y = tt*v1 - a*v0          (flow t -> 0, Jiang et al., "Super SloMo", CVPR 2018, eq. 4)
 *   ft1x = ss*u0 - a*u1;  ft1y = ss*v0 - a*v1          (flow t -> 1)
 *   p0 = ((float)x + ft0x, (float)y + ft0y);  p1 = ((float)x + ft1x, (float)y + ft1y)
 *   sample(I, p): pxc = fminf(fmaxf(px, 0), W-1), pyc likewise (IEEE fmin/fmax: NaN -> the other operand)
 *       x0 = min((int)floorf(pxc), W-2), ax = pxc - x0   (x0 = 0, ax = 0 when W == 1); y0, ay likewise; x1 = min(x0+1, W-1)
 *       c = (I[y0][x0]*(1-ax) + I[y0][x1]*ax) * (1-ay) + (I[y1][x0]*(1-ax) + I[y1][x1]*ax) * ay      per channel, taps as float
 *       (fb_code's expression in of_dis_amd/csrc/ofdis_upsample.h, with bx = 1-ax, by = 1-ay computed once)
 *   c0 = sample(A, p0);  c1 = sample(B, p1)
 *   inside(p) = 0 <= px <= W-1 and 0 <= py <= H-1, on the unclamped p (NaN: false)
 *   near(p)   = (min((int)floorf(pxc + 0.5f), W-1), min((int)floorf(pyc + 0.5f), H-1))
 *   v0 = inside(p0) and M01[near(p0)] == OFDIS_FB_CONSISTENT;  v1 = inside(p1) and M10[near(p1)] == OFDIS_FB_CONSISTENT
 *        (a NULL mask counts as all consistent)
 *   (w0, w1) = (s, t) if v0 == v1;  (1, 0) if v0 only and t < 1, else (0, 1);  (0, 1) if v1 only and t > 0, else (1, 0)
 *   out = (uint8) clamp((int)floorf((w0*c0 + w1*c1) + 0.5f), 0, 255)
 * For finite flows, t = 0 returns A and t = 1 returns B bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_INTERP_MAX_TIMES 16
/* device arrays: img_a, img_b [nframes][height][width][noc] u8; flow_fw, flow_rev [nframes][height][width][2] f32;
 * mask_fw, mask_rev [nframes][height][width] u8 or NULL; out [nframes][ntimes][height][width][noc] u8.
 * times: HOST array of ntimes values (copied into the launch).  Independent of the arithmetic contract.
 * OFDIS_ERR_INVALID before any device work: a NULL frame, flow, out or times pointer; ntimes outside
 * 1..OFDIS_INTERP_MAX_TIMES; a time that is not finite or lies outside [0, 1]; noc not 1 or 3; sizes as ofdis_fb_check. */
int ofdis_interpolate(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                      const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int width, int height,
                      int noc, const float* times, int ntimes, void* stream);
/* OFDIS_BATCH_REVERSE contexts: frames [first_frame, first_frame+count) of the context, straight from its level flows.
 * img_a / img_b are the whole [nframes][height_org][width_org][noc] arrays given to ofdis_batch_build_pyramids_u8.
 * out = [count][ntimes][height_org][width_org][noc].  Bit-identical to ofdis_interpolate applied to the four outputs
 * of ofdis_batch_upsample_bidir(b, first_frame, count, ..., alpha, beta).  Joins a pipelined pass by itself.
 * OFDIS_ERR_INVALID as ofdis_interpolate, and for a context created without OFDIS_BATCH_REVERSE, a frame range outside the
 * batch, an original size above the padded size, and alpha / beta as ofdis_fb_check rejects them. */
int ofdis_batch_interpolate(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int first_frame, int count,
                            const float* times, int ntimes, uint8_t* out, int width_org, int height_org,
                            float alpha, float beta, void* stream);

/* device pointers to the context-owned input planes of level l: kind 0 = image A, 1 = A_dx,
 * 2 = A_dy, 3 = image B (with usefbcon also 4 = B_dx, 5 = B_dy; OFDIS_BATCH_STEREO_LR: 6 .. 11, the same of the mirrored pair).  The caller fills them (hipMemcpy, its own kernels, ofdis_batch_upload
 * or ofdis_batch_build_pyramids_u8). */
float* ofdis_batch_input(ofdis_batch* b, int level, int kind);
size_t ofdis_batch_input_elems(const ofdis_batch* b, int level); /* floats per frame per plane */
/* copy one frame's host pyramid (the ofdis_flow() layout) into slot `frame`.  Like every upload below this ENQUEUES
 * copies on `stream`: the host arrays must stay valid and unchanged until the stream has been synchronised
 * (ofdis_sync). */
int ofdis_batch_upload(ofdis_batch* b, int frame, const float* const* im_a, const float* const* im_a_dx,
                       const float* const* im_a_dy, const float* const* im_b, void* stream);
/* build all input planes of levels sc_l..sc_f on the device from raw 8-bit frames
 * (run_dense.cpp:130-178,298-311,326-344 restated on device): img_a/img_b are device pointers to
 * [nframes][height_org][width_org][noc] uint8; padding to params.width x params.height is applied
 * as the reference does (replicate, floor/ceil split).  Exact (bit-identical to the fp32 OpenCV arithmetic of the
 * reference for 8-bit input) for sc_f <= 7; larger sc_f returns OFDIS_ERR_UNSUPPORTED. */
int ofdis_batch_build_pyramids_u8(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int width_org,
                                  int height_org, void* stream);

/* usefbcon = 1 only: the gradient pyramids of the second image (the backward grid's templates; never read otherwise) */
int ofdis_batch_upload_b_gradients(ofdis_batch* b, int frame, const float* const* im_b_dx, const float* const* im_b_dy,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Video sequences: nframes + 1 consecutive frames give nframes pairs, and every frame's planes are built and held once.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_BATCH_SEQUENCE 16u        /* flag of ofdis_batch_create_ex */
/* An OFDIS_BATCH_SEQUENCE context of `nframes` (still the number of PAIRS, 1..65534; more: OFDIS_ERR_UNSUPPORTED) holds
 * nframes + 1 frame slots; pair k is (frame k, frame k + 1).  Per level it allocates three input arrays of nframes + 1 frames
 * -- image, dx, dy -- and nothing for B: ofdis_batch_input kinds 3, 4, 5 are kinds 0, 1, 2 one frame further on
 * (ofdis_batch_input(b, l, 3 + j) == ofdis_batch_input(b, l, j) + ofdis_batch_input_elems(b, l)), and all six kinds are
 * returned whatever usefbcon says.  Everything downstream sees ordinary A and B planes: ofdis_batch_run (pipelined
 * sub-batches, graph replay, the warm start, ofdis_batch_status) and every result call work as on a plain context and give the
 * bits a plain context gives for img_a = frames[0 .. nframes), img_b = frames[1 .. nframes].  ofdis_batch_interpolate takes
 * `frames` and `frames + one frame` as img_a and img_b.
 * Valid with OFDIS_BATCH_REVERSE (the reverse flow of pair k is frame k + 1 -> frame k; B's gradient planes cost nothing
 * here) and with usefbcon.  OFDIS_ERR_INVALID with OFDIS_BATCH_STEREO_LR and with selectmode 2: a stereo pair is no sequence.
 * The pair-wise entry points would write a shared slot twice: ofdis_batch_build_pyramids_u8, ofdis_batch_upload and
 * ofdis_batch_upload_b_gradients return OFDIS_ERR_INVALID on a sequence context; the two calls below return it on any other. */
/* frame slots of the input arrays: nframes + 1 for a sequence context, nframes for every other, 0 for NULL */
int ofdis_batch_input_frames(const ofdis_batch* b);
/* one frame's host pyramid (image, dx, dy in the ofdis_flow() layout) into frame slot 0 .. nframes; enqueues as
 * ofdis_batch_upload does */
int ofdis_batch_upload_frame(ofdis_batch* b, int slot, const float* const* im, const float* const* im_dx,
                             const float* const* im_dy, void* stream);
/* ofdis_batch_build_pyramids_u8 for the nframes + 1 frames of a sequence, each through the pyramid once, read as a decoder
 * delivers them: `frames` is a device pointer, row y of frame f starts at frames + f * frame_stride + y * row_pitch and holds
 * width_org pixels of noc interleaved bytes.  row_pitch = 0 means width_org * noc, frame_stride = 0 means row_pitch *
 * height_org (both 0: the packed layout of ofdis_batch_build_pyramids_u8).  The luma plane of an NV12 surface is
 * row_pitch = the surface pitch, frame_stride = pitch * surface height * 3 / 2.  Only the width_org * noc bytes of a row are
 * ever read: the padding may be uninitialised or belong to another surface.  Gray frames whose width_org, left padding,
 * `frames`, row_pitch and frame_stride are all multiples of 16 take the 16-byte streaming kernel, as packed frames do.
 * Same bits as the packed call on the same pixels.  OFDIS_ERR_INVALID: row_pitch < width_org * noc, frame_stride <
 * row_pitch * height_org, sizes as ofdis_batch_build_pyramids_u8; OFDIS_ERR_UNSUPPORTED: sc_f > 7. */
int ofdis_batch_build_pyramids_u8_seq(ofdis_batch* b, const uint8_t* frames, size_t row_pitch, size_t frame_stride,
                                      int width_org, int height_org, void* stream);
/* Bytes of device memory in the arrays the context holds right now (any context; lazily allocated scratch counts once it
 * exists; the up to 255 bytes of alignment after each array do not).  0 for NULL. */
size_t ofdis_batch_device_bytes(const ofdis_batch* b);

/* ---------------------------------------------------------------------------------------------
 * Point trajectories through a clip: the flows of consecutive pairs chained from a seed, each track ended where it leaves the
 * image or fails the forward-backward test (Sundaram, Brox and Keutzer, 2010: the use that test was made for).
 *
 * W x H is the frame size; npairs consecutive pairs cover frames 0 .. npairs.  Ffw[k] and Frev[k] are the full-resolution
 * flows of pair k, frame k -> k+1 and frame k+1 -> k, each [H][W][2] fp32.  Point i has the seed (sx, sy) = seeds[i] and the
 * seed frame s = seed_frame[i] (0 when seed_frame is NULL).  Every operation is a separately rounded fp32 operation in this
 * order, independent of the arithmetic contract:
 *   inside(p) = 0 <= px <= W-1 and 0 <= py <= H-1                                                        (NaN: false)
 *   bil(F, p):  x0 = min((int)floorf(px), W-2), ax = px - x0   (x0 = 0, ax = 0 when W == 1); y0, ay likewise;
 *       x1 = min(x0+1, W-1), y1 = min(y0+1, H-1);  bx = 1-ax, by = 1-ay
 *       (F[y0][x0]*bx + F[y0][x1]*ax) * by + (F[y1][x0]*bx + F[y1][x1]*ax) * ay                        per component
 *       (the expression of ofdis_fb_check, of_dis_amd/csrc/ofdis_upsample.h: fb_bilinear, at a real position)
 *   s < 0, s > npairs or not inside(seed): count = 0.  Otherwise p_s = seed, copied bit for bit, count = 1, and for
 *   k = s, s+1, ... while k < npairs and (max_steps == 0 or k - s < max_steps):
 *     1. (u, v) = bil(Ffw[k], p_k);  q = (px + u, py + v);  not inside(q): the track ends
 *     2. with Frev:  (ru, rv) = bil(Frev[k], q);  du = u + ru, dv = v + rv;  lhs = du*du + dv*dv;
 *        rhs = alpha * ((u*u + v*v) + (ru*ru + rv*rv)) + beta;  the track ends unless lhs <= rhs        (NaN ends it)
 *     3. p_{k+1} = q, count += 1
 * tracks = [npairs+1][npoints][2] fp32, frame-major (the lanes of a wavefront store adjacent 8-byte values):
 * tracks[f][i] = p_f for s <= f < s + count; every other entry holds the NaN with the bits 0x7FC00000 in both components.  The
 * call writes every entry exactly once and relies on no memset.  counts = [npoints] int32, may be NULL.
 * of_dis_amd/tracking.py states the same arithmetic in numpy.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_TRACK_MAX_POINTS (1 << 24)
/* device arrays: flow_fw, flow_rev [npairs][height][width][2] (flow_rev NULL: no consistency test); seeds [npoints][2];
 * seed_frame [npoints] int32 or NULL; tracks, counts as above.  One lane per point; enqueues on `stream`.
 * OFDIS_ERR_INVALID before any device work: a NULL flow_fw, seeds or tracks; npoints outside 1..OFDIS_TRACK_MAX_POINTS;
 * max_steps < 0; npairs < 1; sizes, alpha and beta as ofdis_fb_check rejects them. */
int ofdis_track_points(const float* flow_fw, const float* flow_rev /* NULL: no consistency test */, int npairs,
                       int width, int height, const float* seeds /* [npoints][2] */, const int* seed_frame /* or NULL */,
                       int npoints, int max_steps, float alpha, float beta, float* tracks, int* counts, void* stream);
/* OFDIS_BATCH_SEQUENCE contexts: the pairs [first_frame, first_frame+count) of the context, straight from its level flows
 * (the full-resolution flows are never written); seed_frame is relative to first_frame, tracks = [count+1][npoints][2].
 * fb_check = 1: bit-identical to ofdis_track_points applied to out_fw and out_rev of ofdis_batch_upsample_bidir(b,
 * first_frame, count, ...); fb_check = 0: to ofdis_track_points applied to what ofdis_batch_upsample_frames writes, with
 * flow_rev = NULL -- under both contracts (the kernel is contract-independent, the level flows are not).  Joins a pipelined
 * pass by itself.  OFDIS_ERR_INVALID as ofdis_track_points, and for a NULL context, a context created without
 * OFDIS_BATCH_SEQUENCE (the pairs of any other context are no chain), fb_check not 0 or 1, fb_check = 1 on a context created
 * without OFDIS_BATCH_REVERSE, a pair range outside the batch, an original size above the padded size. */
int ofdis_batch_track_points(ofdis_batch* b, int first_frame, int count, const float* seeds, const int* seed_frame,
                             int npoints, int max_steps, int fb_check, float alpha, float beta, float* tracks,
                             int* counts, int width_org, int height_org, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense trajectories: the walk of ofdis_track_points from seeds the library places itself -- the textured centres of a grid,
 * and in every frame again the centres of the cells that hold no live track -- with every track capped at a length (Sundaram,
 * Brox and Keutzer, 2010; Wang, Klaeser, Schmid and Liu, "Dense trajectories and motion boundary descriptors", 2013).  One
 * call runs a clip end to end: everything is enqueued on `stream`, nothing synchronises with the host.
 *
 * A clip has npairs + 1 frames I_0 .. I_npairs, 8-bit, W x H x noc (noc 1 or 3, channels interleaved); Ffw[k], Frev[k] as for
 * ofdis_track_points.  stride s: 2 .. OFDIS_DT_MAX_STRIDE, W >= s and H >= s; window wr: 0 .. OFDIS_DT_MAX_WINDOW; min_eig T >= 0;
 * max_len >= 0; max_tracks: 1 .. OFDIS_DT_MAX_TRACKS; alpha, beta as for ofdis_fb_check.
 *
 * Grid.  off = s / 2, ncx = (W-1-off)/s + 1, ncy = (H-1-off)/s + 1 (integer divisions).  Cell (cx, cy) has the centre pixel
 * (off + cx*s, off + cy*s), always inside the image; cells are numbered row by row, c = cy*ncx + cx.  A position p inside the
 * image lies in cell (min((int)floorf(px) / s, ncx-1), min((int)floorf(py) / s, ncy-1)).
 *
 * Texture test.  textured(f, sx, sy) is exact integer arithmetic on frame f.  The window pixels are (x', y') = (clamp(sx+i, 0,
 * W-1), clamp(sy+j, 0, H-1)) for i, j = -wr .. wr, a clamped pixel counted once per (i, j).  Per channel
 *     gx = I[y'][min(x'+1, W-1)] - I[y'][max(x'-1, 0)],   gy = I[min(y'+1, H-1)][x'] - I[max(y'-1, 0)][x']
 * a = sum gx*gx, b = sum gx*gy, c = sum gy*gy over the window and the channels (a, c <= 255^2 * 3 * 15^2 < 2^26), and
 *     textured = a >= T and c >= T and (a-T)*(c-T) >= b*b                                   (int64; products below 2^52)
 * which is exactly lambda_min([[a, b], [b, c]]) >= T: T = 0 holds for every pixel, a constant window fails every T >= 1.
 * Scale: the tensor is a SUM of DOUBLED central differences, so the mean structure tensor of true gradients has the
 * eigenvalues lambda / (4 * (2wr+1)^2 * noc).  A threshold relative to the frame's largest (Wang) or mean (Sundaram) eigenvalue
 * is not provided: that is a choice of T on the host.
 *
 * Process.  Lmax = max_len ? min(max_len, npairs) : npairs; a track is complete once it covers Lmax + 1 frames.  For
 * f = 0 .. npairs, in this order:
 *   1. advance (f >= 1): every live track takes steps 1 - 3 of the ofdis_track_points loop with pair f-1 (the consistency test
 *      with Frev only).  A track that fails ends and has no entry for frame f; one that passes records its position, len += 1;
 *      a track that is now complete stops being live.
 *   2. occupancy (f < npairs): a cell is occupied if a live track has its frame-f position in it.
 *   3. seed (f < npairs): the unoccupied cells in ascending cell number; each with textured(f, centre) starts a track at
 *      ((float)sx, (float)sy) with start = f, len = 1, live, in slot ntracks++.  With ntracks == max_tracks the seed is dropped
 *      instead: dropped++, no track starts, the cell stays unoccupied.  The last frame seeds nothing.
 *
 * Outputs.  tracks = [Lmax+1][max_tracks][2] fp32, step-major (adjacent slots are adjacent 8-byte values): tracks[j][i] is track
 * i in frame start[i] + j for j < len[i]; for len[i] <= j <= Lmax both components hold the NaN 0x7FC00000.  start, len =
 * [max_tracks] int32 (len may be NULL); info = {ntracks, dropped}.  The call writes every entry of the slots < ntracks and both
 * info values, reads and writes nothing of the slots >= ntracks and relies on no memset.
 *
 * Consequences.
 *   Replay: for every slot i, ofdis_track_points(Ffw, Frev, ..., seeds = tracks[0][i], seed_frame = start[i], max_steps = Lmax)
 *     gives the same len[i] positions bit for bit, and counts == len[i].
 *   Coverage: with dropped == 0, after step 3 of every frame f < npairs every textured cell holds the position of a live track.
 *   Slot order: the slots are ordered by (start, cell of the seed).
 *   Known count: with T = 0, zero flows and Frev zero, ntracks = ncx*ncy*ceil(npairs/Lmax); every track is complete except
 *     those of the last generation when Lmax does not divide npairs.
 * of_dis_amd/tracking.py states the same process in numpy (dense_tracks_ref, seed_texture_ref).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_DT_MAX_TRACKS (1 << 24)
#define OFDIS_DT_MAX_STRIDE 64
#define OFDIS_DT_MAX_WINDOW 7
/* the grid of a width x height frame: returns ncx * ncy and writes ncx, ncy (either may be NULL); 0, and zeros, for a stride
 * outside its range, a side smaller than the stride and sizes ofdis_fb_check rejects */
int ofdis_dense_tracks_cells(int width, int height, int stride, int* ncx, int* ncy);
/* bytes of the work buffer ofdis_dense_tracks needs for any max_len and max_tracks: the texture bits of every frame and cell,
 * per-frame counts, and position and start frame of min(npairs * cells, OFDIS_DT_MAX_TRACKS) slots; 0 for rejected sizes */
size_t ofdis_dense_tracks_work_bytes(int npairs, int width, int height, int stride);
/* the texture test on its own, at every cell centre of every frame: device arrays frames [nframes][height][width][noc], out
 * [nframes][ncy][ncx] u8, 1 / 0.  OFDIS_ERR_INVALID as ofdis_dense_tracks, and for nframes < 1 */
int ofdis_seed_texture(const uint8_t* frames, int nframes, int width, int height, int noc, int stride, int window,
                       int min_eig, uint8_t* out, void* stream);
/* device arrays: frames [npairs+1][height][width][noc]; flow_fw, flow_rev [npairs][height][width][2] (flow_rev NULL: no
 * consistency test); tracks, start, len, info as above; work: 8-byte aligned, at least ofdis_dense_tracks_work_bytes.  One
 * launch tests the texture of every frame; then per frame one launch advances the tracks (one lane per slot of the live
 * window) and two number the seeds (a prefix sum over the cells: slot numbers involve no atomic).  OFDIS_ERR_INVALID before
 * any device work: a NULL frames, flow_fw, tracks, start, info or work; noc not 1 or 3; stride, window or max_tracks outside
 * their ranges; min_eig < 0 or max_len < 0; a side smaller than stride; sizes, alpha and beta as ofdis_fb_check rejects them;
 * npairs < 1; a work buffer that is too small or not 8-byte aligned. */
int ofdis_dense_tracks(const uint8_t* frames, const float* flow_fw, const float* flow_rev /* NULL: no test */, int npairs,
                       int width, int height, int noc, int stride, int window, int min_eig, int max_len, float alpha,
                       float beta, int max_tracks, float* tracks, int* start, int* len /* or NULL */, long long* info,
                       void* work, size_t work_bytes, void* stream);
/* OFDIS_BATCH_SEQUENCE contexts: the pairs [first_frame, first_frame+count) of the context, straight from its level flows (the
 * full-resolution flows are never written); `frames` is the packed clip given to ofdis_batch_build_pyramids_u8_seq, `start` is
 * relative to first_frame, Lmax = max_len ? min(max_len, count) : count.  fb_check = 1: bit-identical to ofdis_dense_tracks
 * applied to frames + first_frame frames and to out_fw and out_rev of ofdis_batch_upsample_bidir(b, first_frame, count, ...);
 * fb_check = 0: to what ofdis_batch_upsample_frames writes, with flow_rev = NULL -- under both contracts.  The work buffer
 * belongs to the context: allocated at the first call for what that call needs (a later call that needs more allocates
 * again) and counted by ofdis_batch_device_bytes.  Joins a pipelined pass by itself.  OFDIS_ERR_INVALID as ofdis_dense_tracks,
 * and for a NULL context, a context created without OFDIS_BATCH_SEQUENCE, fb_check not 0 or 1, fb_check = 1 on a context
 * created without OFDIS_BATCH_REVERSE, a pair range outside the batch, an original size above the padded size. */
int ofdis_batch_dense_tracks(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int stride, int window,
                             int min_eig, int max_len, int fb_check, float alpha, float beta, int max_tracks,
                             float* tracks, int* start, int* len, long long* info, int width_org, int height_org,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Track selection: the stage of Wang et al.'s pipeline between tracking and description.  Every slot of ofdis_dense_tracks is
 * classified -- too short, not finite, static, erratic, one dominating jump and, for the "improved" trajectories (Wang and
 * Schmid, "Action recognition with improved trajectories", 2013), moving only as the camera does -- and the kept slots are
 * compacted, in their order, into a fresh (tracks, start, len, info) set of the same layout.  Every later stage
 * (ofdis_track_descriptors, ofdis_track_bof, ofdis_codebook_*) reads ntracks from the device `info` array and pays per slot, so
 * it takes the selected set unchanged and is cheaper in proportion.  Everything is enqueued on `stream`; nothing synchronises
 * with the host, and nkept never reaches it.
 *
 * Inputs: the arrays of ofdis_dense_tracks.  tracks [lmax+1][max_tracks][2] fp32, start, len [max_tracks] int32, info = the
 * device array {ntracks, dropped}; n = min(info[0], max_tracks) slots are looked at.  Optionally models [npairs][6] fp64 exactly
 * as ofdis_global_motion writes them, with the frame size W x H they refer to; pair k of the models is pair k of the clip the
 * tracks were made on (start counts from the same frame).
 *
 * Quantities, per slot i < n with L = clamp(len[i], 0, lmax+1) and (x_j, y_j) = tracks[j][i].  Every float operation is a
 * separately rounded fp32 operation, every sum is sequential over ascending j starting from 0.0f, sqrtf and / are IEEE.  A
 * "maximum" starts from 0.0f and takes m_j where m_j > maximum, so it passes over a NaN.
 *   mean    mx = (sum over j < L of x_j) / (float)L;  my likewise
 *   spread  sx = sqrtf((sum over j < L of (x_j - mx)*(x_j - mx)) / (float)L);  sy likewise
 *   step    for j < L-1: d_j = tracks[j+1][i] - tracks[j][i] = (dx, dy), m_j = sqrtf(dx*dx + dy*dy);
 *           S = the sum of the m_j, mmax = their maximum
 *   residual step (models given), under the model a_0 .. a_5 of pair k = start[i] + j:
 *           af_n = (float)a_n;  xc = x_j - (float)(W-1)*0.5f;  yc = y_j - (float)(H-1)*0.5f
 *           mu = (af0 + af1*xc) + af2*yc;  mv = (af3 + af4*xc) + af5*yc;  r_j = (dx - mu, dy - mv) = (rx, ry)
 *           rm_j = sqrtf(rx*rx + ry*ry);  Sr = the sum of the rm_j, rmax = their maximum
 *           A k outside 0 .. npairs-1 makes the slot OFDIS_TS_INVALID; where that test is switched off such a step has r_j = d_j.
 *           Without models r_j = d_j, Sr = S.
 * The code of a slot is the FIRST test that holds, in this order; 0 (OFDIS_TS_KEPT) where none does.  A NaN in a comparison
 * gives false, as elsewhere in this header.
 *   1 OFDIS_TS_SHORT    L < max(min_len, 1)
 *   2 OFDIS_TS_INVALID  one of the L positions has a component that is not finite, or a step has no model (above)
 *   3 OFDIS_TS_STATIC   sx < min_std && sy < min_std
 *   4 OFDIS_TS_ERRATIC  sx > max_std || sy > max_std
 *   5 OFDIS_TS_JUMP     L >= 2 && mmax > max_step && mmax > S * max_step_share
 *   6 OFDIS_TS_CAMERA   models != NULL && L >= 2 && rmax <= min_camera
 * Bit (code - 1) of `tests` switches a test on; a cleared bit skips it, and the slot goes on to the next test.
 *
 * Outputs.  code [max_tracks] u8 or NULL: the code of every slot < n.  counts [7] int64 or NULL: the slots per code, kept ones
 * (counts[0]) included.  The compacted set, with its own stride max_tracks_out and the same lmax: tracks_out
 * [lmax+1][max_tracks_out][2], start_out, len_out [max_tracks_out], info_out = {nkept_written, dropped_out}, index
 * [max_tracks_out] int32 or NULL, shape_out [max_tracks_out][lmax][2] fp32 or NULL.
 *   Output slot r is the r-th kept input slot (the order is kept), index[r] its input slot.  All lmax+1 entries of the track
 *   are copied bit for bit, the NaN tail beyond len included; start and len are copied.
 *   nkept_written = min(nkept, max_tracks_out), dropped_out = nkept - nkept_written: kept slots beyond max_tracks_out are not
 *   written.
 *   shape_out[r][j] = (rx / Sr, ry / Sr) of r_j for j < L-1; (0, 0) when Sr == 0 and for j >= L-1.  With models this is the
 *   camera-compensated trajectory shape; without, it is d_j / S, bit-identical to what ofdis_track_descriptors writes as
 *   `shape` for the same track.  Where a non-finite position was kept (OFDIS_TS_INVALID switched off) a NaN entry has no defined
 *   payload.
 *   Only output slots < nkept_written are written, every entry of them exactly once; only code entries < n are written; counts
 *   and info_out are written whole.  The call relies on no memset and reads nothing of the input slots >= n.  The outputs must not
 *   overlap the inputs or each other: nothing checks it.
 *
 * Consequences.
 *   Drop-in: ofdis_track_descriptors and ofdis_track_bof on the selected set give rows index[r] of the same calls on the
 *     original set.
 *   Identity: with tests == 0 and max_tracks_out >= n the selected set equals the first n slots of the input, index[r] == r.
 *   Sums: counts sums to n; counts[0] == nkept_written + dropped_out.
 *   Known values: a track that stands still is OFDIS_TS_STATIC; L positions one pixel apart along an axis have the
 *     spread sqrt((L*L - 1) / 12), above sqrt(3) from L = 7 on; a track whose steps equal a translation model has every rm_j == 0 and
 *     is OFDIS_TS_CAMERA with the model, kept without it.
 *   Contract independence: one unit, compiled once with every operation separately rounded, serves both contracts.
 * Improved trajectories on an OFDIS_BATCH_SEQUENCE context: ofdis_batch_dense_tracks -> ofdis_batch_global_motion -> this call
 * -> ofdis_batch_upsample_bidir and, for the residual flow HOF and MBH are made of, ofdis_batch_motion_compensate ->
 * ofdis_track_descriptors on the selected set -> ofdis_track_bof.  The tracks follow the full flow; the camera models change
 * what is selected and what the descriptors see.  No context form is needed: no argument here belongs to a context.
 * ofdis_track_select_projective takes the 8-parameter models of ofdis_projective_motion instead (section "Projective camera
 * models", which states the residual step under them).
 * Not provided: RANSAC (the models are those of ofdis_global_motion or ofdis_projective_motion); a bag-of-features channel for
 * the shape.  of_dis_amd/tracking.py states the same definition in numpy (track_select_ref).
 * ------------------------------------------------------------------------------------------- */
enum { OFDIS_TS_KEPT = 0, OFDIS_TS_SHORT = 1, OFDIS_TS_INVALID = 2, OFDIS_TS_STATIC = 3, OFDIS_TS_ERRATIC = 4, OFDIS_TS_JUMP = 5,
       OFDIS_TS_CAMERA = 6 };
#define OFDIS_TS_ALL_TESTS 0x3Fu
typedef struct ofdis_track_select_params {
  int min_len;           /* 0 */
  float min_std;         /* 1.7320508f = sqrtf(3), Wang's value */
  float max_std;         /* 50 */
  float max_step;        /* 20 */
  float max_step_share;  /* 0.7f */
  float min_camera;      /* 1 */
  unsigned tests;        /* OFDIS_TS_ALL_TESTS */
} ofdis_track_select_params;
/* the values above; a NULL p is ignored */
void ofdis_track_select_defaults(ofdis_track_select_params* p);
/* bytes of the work buffer: one 64-byte record (the counts per code, the kept slots before it, the kept lanes) per 256 slots;
 * 0 for max_tracks outside 1 .. OFDIS_DT_MAX_TRACKS */
size_t ofdis_track_select_work_bytes(int max_tracks);
/* device arrays as above; p is read on the host.  Three launches: classify (one lane per slot; one record per workgroup into
 * `work`, plain stores), scan (one workgroup: the offsets of the workgroups, info_out, counts), scatter (the kept lanes copy).
 * No atomics, no waiting between workgroups.  OFDIS_ERR_INVALID before any device work: a NULL tracks, start, len, info, p,
 * tracks_out, start_out, len_out, info_out or work; lmax < 1; max_tracks or max_tracks_out outside 1 .. OFDIS_DT_MAX_TRACKS;
 * models given with npairs < 1, with sizes ofdis_fb_check rejects or a side above OFDIS_GM_MAX_SIDE; min_std, max_std, max_step
 * or min_camera NaN or negative (+infinity is accepted for max_std and max_step only); max_step_share outside [0, 1];
 * min_len < 0; bits of tests outside OFDIS_TS_ALL_TESTS; a work buffer smaller than ofdis_track_select_work_bytes(max_tracks) or
 * not 8-byte aligned. */
int ofdis_track_select(const float* tracks, const int* start, const int* len, const long long* info, int lmax, int max_tracks,
                       const double* models /* or NULL */, int npairs, int width, int height,
                       const ofdis_track_select_params* p, uint8_t* code /* or NULL */, long long* counts /* or NULL */,
                       int max_tracks_out, float* tracks_out, int* start_out, int* len_out, long long* info_out,
                       int* index /* or NULL */, float* shape_out /* or NULL */, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory-aligned descriptors of dense tracks: in the space-time tube around every track of ofdis_dense_tracks the histograms
 * of gradient orientation (HOG), of flow orientation (HOF) and of the motion boundaries (MBHx, MBHy: the orientation of the
 * gradient of each flow component), and the track's normalised displacements (trajectory shape) -- the second half of Wang,
 * Klaeser, Schmid and Liu, "Dense trajectories and motion boundary descriptors", 2013.  Every histogram entry is a sum of
 * integers, so its bits depend neither on the order of the sum nor on the kernel's mapping nor on the arithmetic contract.
 *
 * Inputs: the arrays of ofdis_dense_tracks.  frames [npairs+1][H][W][noc] u8, noc 1 or 3; Ffw = flow_fw [npairs][H][W][2] fp32
 * -- or equally the residual flow of ofdis_motion_compensate, the camera-compensated flow "improved trajectories" feed into HOF
 * and MBH; tracks [lmax+1][max_tracks][2], start, len [max_tracks]; info = the device array {ntracks, dropped} exactly as
 * ofdis_dense_tracks wrote it (ntracks never reaches the host).  Parameters: lmax >= 1, the Lmax the tracks array was made
 * with; patch N: even, 2 .. OFDIS_DESC_MAX_PATCH; nxy: 1 .. 4 with N % nxy == 0; nt: 1 .. 8 with nt <= lmax; min_flow finite and
 * >= 0; and N*N*lmax <= 65536, so that no sum of addends <= 65535 reaches 2^32.
 *
 * Features, per pixel (x, y) of frame k / pair k.  "Clamped": neighbour indices clamp to the image, as in the texture test.
 * Every float operation is a separately rounded fp32 operation, sqrtf is IEEE.
 *   oct(a, b), the octant of a vector by comparisons only:
 *     Q = 0 if a > 0 && b >= 0, (p, q) = (a, b);     Q = 1 if a <= 0 && b > 0, (p, q) = (b, -a);
 *     Q = 2 if a < 0 && b <= 0, (p, q) = (-a, -b);   Q = 3 if a >= 0 && b < 0, (p, q) = (-b, a);
 *     bin = 2*Q + (q >= p ? 1 : 0).  No case holds (zero vector, NaN): the pixel contributes nothing to that channel.
 *   quant(m, s): m not finite: the pixel contributes nothing; else (int)floorf(fminf(m*s, 65535.f) + 0.5f).
 *   HOG  (8 bins): g = the pixel value (noc 1) or the integer sum of the three channels (noc 3);
 *        gx = g[y][x+1] - g[y][x-1], gy = g[y+1][x] - g[y-1][x] (clamped, doubled central differences, integers);
 *        m = sqrtf((float)(gx*gx + gy*gy)) (the argument is below 2^24: exact); bin = oct(gx, gy), q = quant(m, 16).
 *   HOF  (9 bins): (u, v) = Ffw[k][y][x], m = sqrtf(u*u + v*v).  m not finite: nothing.  m < min_flow: bin 8 with q = 256, the
 *        "no motion" bin, counted as one pixel of motion as Wang's implementation does (this takes precedence over the
 *        zero-vector rule).  Otherwise bin = oct(u, v), q = quant(m, 256).  With min_flow = 0 bin 8 stays empty.
 *   MBHx (8 bins): gx = u[y][x+1] - u[y][x-1], gy = u[y+1][x] - u[y-1][x] (clamped); m = sqrtf(gx*gx + gy*gy);
 *        bin = oct(gx, gy), q = quant(m, 4096).
 *   MBHy (8 bins): the same on v.
 *
 * Tube.  For slot i < ntracks and step j = 0 .. len[i]-2, the pairs the track crossed (a track of length 1 has all-zero
 * histograms; j < lmax always): k = start[i] + j, (px, py) = tracks[j][i], cx = (int)floorf(px + 0.5f), cy likewise.  The
 * window pixels are x = cx - N/2 + a, y = cy - N/2 + b for a, b = 0 .. N-1; pixels outside the image contribute nothing.  The
 * spatial cell of a pixel is (a / (N/nxy), b / (N/nxy)) (column, row), its temporal cell t = j*nt / lmax (integer division).
 *
 * Outputs.  hist = [max_tracks][D] u32, D = 33*nxy*nxy*nt, in the index order channel (HOG, HOF, MBHx, MBHy), t, cell row,
 * cell column, bin: the channels start at 0, 8*C, 17*C and 25*C with C = nxy*nxy*nt.  Each entry is the sum of the q of its
 * cell and bin.  shape = [max_tracks][lmax][2] fp32 or NULL: d_j = tracks[j+1][i] - tracks[j][i] for j < len[i]-1, S = the
 * sequential sum over ascending j of sqrtf(dx*dx + dy*dy), shape[i][j] = (dx/S, dy/S) (IEEE division); (0, 0) when S == 0 and
 * for j >= len[i]-1.  The call writes every entry of the slots < ntracks exactly once, reads and writes nothing of the slots
 * >= ntracks, relies on no memset and does not synchronise with the host.
 *
 * Consequences.
 *   Known value: zero flows and min_flow > 0 put all of HOF in bin 8: each cell holds 256 x (its pixels inside the image) x
 *     (the steps of its temporal cell); MBHx and MBHy are all zero.  A constant frame has HOG all zero.
 *   Translation: adding a constant vector to Ffw leaves MBHx and MBHy unchanged wherever the sums stay finite and no rounding
 *     occurs -- stated for integer-valued test flows only.
 *   Contract independence: integer sums of separately rounded values; one unit, compiled once, serves both contracts.
 * Not provided: interpolation of a vote between neighbouring bins; normalisation in floating point (of_dis_amd/tracking.py:
 * normalize_descriptors, on the host -- the 8-bit RootSIFT form on the device and the bag of features made of it are the next
 * section, ofdis_descriptor_normalize .. ofdis_track_bof); a form that reads a sequence context's level
 * flows directly -- every window pixel needs five flow values and is visited by about 40 overlapping windows, and rebuilding
 * flow values from level flows already loses when each is used a handful of times (README: trajectory filter, global motion).
 * The route is ofdis_batch_upsample_bidir -> ofdis_dense_tracks -> this call.
 * of_dis_amd/tracking.py states the same definition in numpy (track_descriptors_ref).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_DESC_MAX_PATCH 64
/* D = 33 * nxy * nxy * nt, or 0 for a patch, nxy or nt outside its range or a patch nxy does not divide */
int ofdis_track_descriptor_dims(int patch, int nxy, int nt);
/* device arrays as above; shape may be NULL.  One launch: one wavefront per slot, sized by max_tracks, the slots >= ntracks
 * return at once.  OFDIS_ERR_INVALID before any device work: a NULL frames, flow_fw, tracks, start, len, info or hist; noc not 1
 * or 3; sizes as ofdis_fb_check rejects them; npairs < 1; lmax < 1 or lmax > npairs; max_tracks outside
 * 1 .. OFDIS_DT_MAX_TRACKS; patch, nxy or nt outside their ranges, patch odd or not a multiple of nxy, nt > lmax,
 * patch*patch*lmax > 65536; min_flow negative or not finite. */
int ofdis_track_descriptors(const uint8_t* frames, const float* flow_fw, int npairs, int width, int height, int noc,
                            const float* tracks, const int* start, const int* len, const long long* info,
                            int lmax, int max_tracks, int patch, int nxy, int nt, float min_flow,
                            uint32_t* hist, float* shape /* or NULL */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bag-of-features encoding of those descriptors, the last stage of Wang et al.'s pipeline: every histogram channel of a hist
 * row becomes an 8-bit RootSIFT descriptor, each is matched against the words of a codebook by squared Euclidean distance, and
 * the clip is described by how often every word was the nearest one.  Everything is integer arithmetic: a result is a pure
 * function of its inputs, independent of the order of any sum, of the kernels' mapping and of the arithmetic contract.
 *
 * Notation of the section above: C = nxy*nxy*nt, D = 33*C; channel c = 0 .. 3 (HOG, HOF, MBHx, MBHy) is the segment of a row
 * that starts at 0, 8*C, 17*C, 25*C and has n_c = 8*C, 9*C, 8*C, 8*C entries; nxy: 1 .. 4, nt: 1 .. 8 (the patch is no
 * argument).  info = the device array {ntracks, dropped} of ofdis_dense_tracks; ntracks never reaches the host, and every call
 * neither reads nor writes anything of the slots >= ntracks.  max_tracks: 1 .. OFDIS_DT_MAX_TRACKS.
 *
 * Normalisation (ofdis_descriptor_normalize): hist [max_tracks][D] u32 -> desc [max_tracks][D] u8, same index order.  Per slot
 * and channel, with S the uint64 sum of the channel's entries h_e:
 *   S == 0: desc_e = 0 for the whole channel.
 *   otherwise desc_e = min(255, max{ q >= 0 : q*q*S <= 510*510*h_e }), division-free uint64 arithmetic, every product < 2^62.
 * Identity: max{ q : q*q*S <= T } = floor(sqrt(floor(T / S))) for integers T >= 0, S > 0 (q*q*S <= T <=> q*q <= T/S <=>
 * q*q <= floor(T/S), q*q being an integer), so without the clamp desc_e = floor(sqrt(floor(510*510*h_e / S))): RootSIFT
 * (divide by the L1 norm, take the square root; Arandjelovic and Zisserman 2012) in units of 1/OFDIS_BOF_SCALE, clamped at
 * 255 -- the convention of 8-bit SIFT (x 512, clamp 255).  An entry reaches 255 where it holds a quarter of its channel's sum
 * or more.
 *
 * Assignment (ofdis_codebook_assign): codebook [nwords][D] u8, row k holds word k of every channel in the index order of a
 * hist row; nwords: 1 .. OFDIS_BOF_MAX_WORDS.  For slot i and channel c, d(k) = sum over the channel's entries e of
 * (desc[i][e] - codebook[k][e])^2, at most 1152*255*255 < 2^31; words[i][c] = the smallest k that attains the minimum of d,
 * dist[i][c] = that minimum.  words, dist = [max_tracks][4] int32; dist may be NULL.  An all-zero channel is assigned like any
 * other.
 *
 * Counting (ofdis_bof_histogram): bof [4][nwords] u32, bof[c][k] = the number of slots i < ntracks with len[i] >= min_len and
 * words[i][c] == k; min_len >= 1, and min_len = lmax + 1 counts complete tracks only, as Wang et al. do.  The call clears bof
 * itself with a launch of its own and relies on no memset; it counts with integer atomics.  A words entry outside
 * 0 .. nwords-1 (an array the caller filled) is not counted.
 *
 * Fused (ofdis_track_bof): hist -> bof in one pass, bit-identical to the three calls above in a row: it reads hist, normalises
 * in registers, never writes desc, assigns, counts, and writes words where it is not NULL.
 *
 * Consequences.
 *   Known value: a channel with one nonzero entry has that entry 255 and the rest 0; a channel of n equal nonzero entries has
 *     every entry min(255, floor(sqrt(floor(260100 / n)))), e.g. 180 for n = 8.
 *   Scale invariance: multiplying a channel's entries by a common factor leaves desc unchanged where no product overflows.
 *   Ties: equal distances go to the lowest index, so a codebook with a duplicated row never uses the later copy; a codebook
 *     drawn from the descriptors themselves gives dist 0 and the first copy.
 *   Sums: every row of bof sums to the number of counted tracks; the four rows have the same sum.
 *   Contract independence: integers only; one unit, compiled once, serves both contracts.
 * Not provided: Fisher vectors; the shape channel (floats: it is not encoded).  Taking out static tracks, and erratic and
 * camera-only ones, comes before this stage: ofdis_track_select.  The codebook itself comes from the k-means training of the next section (ofdis_codebook_seed, ofdis_codebook_train) or from the caller.
 * The route is ofdis_dense_tracks -> ofdis_track_descriptors -> ofdis_track_bof.  None of the calls
 * synchronises with the host.  of_dis_amd/tracking.py states the same definitions in numpy (normalize_descriptors_u8,
 * codebook_assign_ref, bof_ref).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_BOF_SCALE 510
#define OFDIS_BOF_MAX_WORDS 16384
/* One launch, one wavefront per slot.  OFDIS_ERR_INVALID before any device work (this and the three calls below): a NULL
 * required pointer (all but dist, and words of ofdis_track_bof); max_tracks outside 1 .. OFDIS_DT_MAX_TRACKS; nxy or nt
 * outside its range; nwords outside 1 .. OFDIS_BOF_MAX_WORDS; min_len < 1. */
int ofdis_descriptor_normalize(const uint32_t* hist, const long long* info, int max_tracks, int nxy, int nt, uint8_t* desc,
                               void* stream);
/* One launch: v_mfma_i32_16x16x64_i8 on the bytes ^ 0x80 (both sides minus 128: differences unchanged), 64 to 512 slots of one
 * channel per workgroup, the codebook through LDS in tiles. */
int ofdis_codebook_assign(const uint8_t* desc, const long long* info, int max_tracks, int nxy, int nt, const uint8_t* codebook,
                          int nwords, int* words, int* dist /* or NULL */, void* stream);
/* Two launches: the clear, the count. */
int ofdis_bof_histogram(const int* words, const int* len, const long long* info, int max_tracks, int nwords, int min_len,
                        uint32_t* bof, void* stream);
/* Two launches: the clear, then the assignment kernel reading hist. */
int ofdis_track_bof(const uint32_t* hist, const int* len, const long long* info, int max_tracks, int nxy, int nt,
                    const uint8_t* codebook, int nwords, int min_len, uint32_t* bof, int* words /* or NULL */,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * K-means training of the bag-of-features codebook: Lloyd's algorithm on the desc rows of ofdis_descriptor_normalize, all
 * integers, four independent clusterings in one pass (row k of a codebook holds word k of every channel).  The assignment step
 * is ofdis_codebook_assign; the centre update is exact integer arithmetic, so a trained codebook is a pure function of its
 * inputs: independent of the order of the slots, of any order of summation, of the kernels' mapping and of the arithmetic
 * contract.
 *
 * Notation of the section above: C, D = 33*C, channel c with its offset off_c and its length n_c; desc [max_tracks][D] u8,
 * codebook [nwords][D] u8, words [max_tracks][4] int32, info = {ntracks, dropped} on the device.  n = min(info[0], max_tracks);
 * no call reads or writes anything of the slots >= n.
 *
 * Members.  Slot i < n is a member iff len == NULL or len[i] >= min_len (len [max_tracks] int32 of ofdis_dense_tracks);
 * min_len >= 1 is checked either way, and min_len = lmax + 1 trains on complete tracks, the population ofdis_bof_histogram
 * counts.
 *
 * Seeding (ofdis_codebook_seed).  For word k, s_k = floor((2k+1)*n / (2*nwords)).  Row k of codebook is the whole desc row, all
 * four channels, of the first member at or after s_k, cyclically: of slot (s_k + t) mod n for the smallest t >= 0 that makes it
 * a member.  With no member, which includes n == 0, every row is all zero.  With len == NULL and n >= nwords the rows come from
 * nwords distinct, evenly spread slots.  Repeated rows are harmless: by the tie rule of the assignment a later copy is never
 * used, and it stays an empty word.
 *
 * Update (ofdis_codebook_update).  For each channel c and word k, with M = {members i : words[i][c] == k}:
 *   counts[c][k] = |M|                                                      counts [4][nwords] u32
 *   |M| > 0:  codebook[k][off_c + e] = floor((2*S_e + |M|) / (2*|M|)),  S_e = sum over M of desc[i][off_c + e]
 *             -- the mean rounded half up; S_e <= 2^24 * 255 < 2^32, and the result is <= 255 by construction
 *   |M| == 0: the word keeps its bytes.
 * A words entry outside 0 .. nwords-1 (an array the caller filled) belongs to no word.  The call writes every entry of counts
 * itself and relies on no memset.
 *
 * Training (ofdis_codebook_train).  codebook is in/out: any uint8 array, from ofdis_codebook_seed or of the caller's own seeding
 * (k-means++, say).  For t = 0 .. iters-1:
 *   words, dist := ofdis_codebook_assign(desc, codebook): every slot < n is written, members or not, exactly as that call would
 *   stats[t][c][0] := the number of members whose words[i][c] differs from iteration t-1; at t = 0 the number of members
 *   stats[t][c][1] := the sum over the members of dist[i][c], in int64 (< 2^55)
 *   codebook, counts := the update above
 * stats = [iters][4][2] int64 on the device, or NULL.  On return words and counts belong to the last assignment, taken against
 * the codebook before the last update; codebook is the result of the last update -- a caller who wants the words of the
 * returned codebook calls ofdis_codebook_assign.  iters: 1 .. OFDIS_KMEANS_MAX_ITERS.
 *
 * Consequences.
 *   Monotone: per channel, stats[t+1][c][1] <= stats[t][c][1].  The nearest integer to a mean minimises a sum of squares over
 *     the integers, the previous centre was an integer, an empty word does not move, and the assignment cannot increase any
 *     member's distance.
 *   Fixed point: once stats[t][c][0] == 0, the channel's words, counts and codebook bytes stay the same in every later
 *     iteration.
 *   Order: the update depends neither on the order of the slots nor on any order of summation (integer sums).
 *   Route: ofdis_codebook_train with iters = T is bit-identical to T rounds of ofdis_codebook_assign + ofdis_codebook_update.
 *   Contract independence: integers only; one unit, compiled once, serves both contracts.
 *   Known values: members {0, 1} give 1; members {0, 0, 1} give 0; members {254, 255} give 255; nwords = 1 gives the rounded
 *     mean of the members after one iteration.
 * Not provided: re-seeding of empty words (counts shows them); k-means++ seeding; subsampling (train on a desc array the caller
 * thinned); an early exit (all iters are enqueued); Fisher vectors and the shape channel, as before.  None of the calls
 * synchronises with the host.  of_dis_amd/tracking.py states the same definitions in numpy (codebook_seed_ref,
 * codebook_update_ref, codebook_train_ref).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_KMEANS_MAX_ITERS 1000
/* Bytes of the work buffer of ofdis_codebook_update and ofdis_codebook_train; 0 for rejected sizes.  With M = max_tracks and
 * K = nwords it holds, in this order: the previous words and dist of the assignment, int32 [M][4] each (training with stats);
 * every member's rank inside its word, u32 [M][4]; the offsets of the words' segments, u32 [4][K+1]; the slots ordered by word,
 * u32 [4][M]; and two rows of partial sums per 256 ordered slots and channel, u32 [4][ceil(M/256)][2][RL], RL = the entries of
 * the longest channel padded to the lanes that sum them (16 .. 1280).  About 64 + RL/8 bytes per slot. */
size_t ofdis_codebook_train_work_bytes(int max_tracks, int nxy, int nt, int nwords);
/* One launch, one wavefront per word: len is walked 64 slots per step.  OFDIS_ERR_INVALID before any device work (this and the
 * two calls below): a NULL required pointer (all but len and stats); max_tracks outside 1 .. OFDIS_DT_MAX_TRACKS; nxy outside
 * 1 .. 4; nt outside 1 .. 8; nwords outside 1 .. OFDIS_BOF_MAX_WORDS; min_len < 1; iters outside its range; a work buffer that
 * is NULL, smaller than ofdis_codebook_train_work_bytes or not 8-byte aligned. */
int ofdis_codebook_seed(const uint8_t* desc, const int* len /* or NULL */, const long long* info, int max_tracks, int nxy, int nt,
                        int nwords, int min_len, uint8_t* codebook, void* stream);
/* Six launches: bucket, then sum.  The members are counted per word (integer atomics whose arrival order reaches no result),
 * the counts scanned, the slots scattered into their word's segment, the rows of every segment summed in registers (desc is
 * read once) and divided; a segment longer than 256 members is summed in parts, by a last launch. */
int ofdis_codebook_update(const uint8_t* desc, const int* words, const int* len /* or NULL */, const long long* info,
                          int max_tracks, int nxy, int nt, int nwords, int min_len, uint8_t* codebook, uint32_t* counts,
                          void* work, size_t work_bytes, void* stream);
/* iters x (the assignment kernel + the six launches above), enqueued at once. */
int ofdis_codebook_train(const uint8_t* desc, const int* len /* or NULL */, const long long* info, int max_tracks, int nxy, int nt,
                         int nwords, int min_len, int iters, uint8_t* codebook, int* words, uint32_t* counts,
                         long long* stats /* or NULL */, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Motion-compensated temporal filtering of a clip: every frame averaged with its two neighbours warped onto it by the flow
 * (motion compensation), a neighbour left out where the forward-backward test flags the pixel, where its sample falls outside
 * the image and -- with a finite tau -- faded out as it differs from the pixel it would be averaged with.  The classical use
 * is video denoising (three frames with independent noise: the noise drops towards 1 / sqrt(3)).
 *
 * A clip has npairs + 1 frames I_0 .. I_npairs, 8-bit, W x H x noc (noc 1 or 3, channels interleaved).  Ffw[k] is the flow
 * from frame k to k+1 and Frev[k] the flow from frame k+1 to k, each [H][W][2] fp32; the optional masks Mfw[k], Mrev[k] hold
 * OFDIS_FB_* codes as ofdis_batch_upsample_bidir writes them.  wn is the neighbour strength, 0 <= wn <= 1; tau the
 * photometric gate in grey levels, +inf (no gate) or a positive float that is not subnormal.  For output frame f and pixel
 * (x, y), every operation is a separately rounded fp32 operation in this order, independent of the arithmetic contract:
 *   c[ch] = (float) I_f[y][x][ch]
 *   candidate(J, F, M):                    J = the neighbouring frame, F = the flow from frame f to J, M = its mask or NULL
 *       (u, v) = F[y][x];  p = ((float)x + u, (float)y + v)
 *       valid  = inside(p) and (M == NULL or M[y][x] == OFDIS_FB_CONSISTENT)      inside: 0 <= px <= W-1 and 0 <= py <= H-1,
 *                                                                                 as in ofdis_fb_check (NaN: false)
 *       not valid: w = 0, s[ch] = 0
 *       valid:  s[ch] = sample(J, p)[ch]   the bilinear expression of ofdis_interpolate above, at p itself (p is inside:
 *                                          the clamp changes nothing)
 *               d = max over ch of fabsf(s[ch] - c[ch])
 *               g = fmaxf(1 - d / tau, 0)  IEEE division; tau = +inf gives g = 1
 *               w = wn * g
 *   next = candidate(I_{f+1}, Ffw[f],    Mfw[f])      when f < npairs, else w_n = 0, s_n = 0
 *   prev = candidate(I_{f-1}, Frev[f-1], Mrev[f-1])   when f > 0,      else w_p = 0, s_p = 0
 *   num[ch] = (c[ch] + w_p * s_p[ch]) + w_n * s_n[ch];   den = (1 + w_p) + w_n
 *   out[ch] = (uint8) clamp((int)floorf(num[ch] / den + 0.5f), 0, 255)
 *   support = (w_p > 0 ? 1 : 0) | (w_n > 0 ? 2 : 0)
 * Consequences: wn = 0 returns the clip bit for bit (num = c, den = 1), and a clip of identical frames with zero flows returns
 * itself (every sample is the pixel, d = 0, and (c + w_p*c + w_n*c) / (1 + w_p + w_n) lies within a few ulp of the integer c).
 * The first frame has support & 1 == 0 and the last support & 2 == 0 everywhere.
 * of_dis_amd/temporal.py states the same arithmetic in numpy.
 * ------------------------------------------------------------------------------------------- */
/* device arrays: frames, out [npairs+1][height][width][noc] u8; flow_fw, flow_rev [npairs][height][width][2] f32; mask_fw,
 * mask_rev [npairs][height][width] u8 or NULL (all consistent); support [npairs+1][height][width] u8 or NULL (not written).
 * One lane per quad of four adjacent pixels; 4-byte stores where width is a multiple of 4 and the array is 4-byte aligned, byte
 * stores of the same bytes otherwise; nothing outside `out` and `support` is written.  Enqueues on `stream`.
 * OFDIS_ERR_INVALID before any device work: a NULL frames, flow or out pointer; out == frames; noc not 1 or 3; npairs < 1;
 * sizes as ofdis_fb_check rejects them; wn outside [0, 1] or NaN; tau not positive, subnormal or NaN. */
int ofdis_temporal_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                          const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int width, int height, int noc,
                          float wn, float tau, void* stream);
/* OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE contexts: frames first_frame .. first_frame + count of the context (count + 1
 * output frames), straight from its level flows.  `frames` is the whole packed clip [nframes+1][height_org][width_org][noc]
 * given to ofdis_batch_build_pyramids_u8_seq (pitched surfaces: copy them, as for ofdis_batch_interpolate); out =
 * [count+1][height_org][width_org][noc], support = [count+1][height_org][width_org] or NULL.  Only the pairs [first_frame,
 * first_frame + count) are used: the first and the last frame of the range have ONE neighbour, even where the context holds
 * more pairs.  Bit-identical to ofdis_temporal_filter applied to the four outputs of ofdis_batch_upsample_bidir(b,
 * first_frame, count, ..., alpha, beta) and to frames + first_frame frames, under both contracts (the kernel is
 * contract-independent, the level flows are not); the flows and masks are never written.  Joins a pipelined pass by itself.
 * OFDIS_ERR_INVALID as ofdis_temporal_filter, and for a NULL context, a context created without OFDIS_BATCH_SEQUENCE or
 * without OFDIS_BATCH_REVERSE, a pair range outside the batch, an original size above the padded size, alpha / beta as
 * ofdis_fb_check rejects them. */
int ofdis_batch_temporal_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                uint8_t* support, int width_org, int height_org, float wn, float tau,
                                float alpha, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal filtering along flow trajectories over 2R + 1 frames: the filter above averages a frame with its two neighbours
 * only, which caps the noise gain at 1 / sqrt(3).  Here every output pixel walks `radius` steps forward and `radius` steps
 * back through the flows of consecutive pairs -- the walk of ofdis_track_points -- and samples the frame at every stop; a
 * direction ends where the path leaves the image or fails the forward-backward test.
 *
 * A clip has npairs + 1 frames I_0 .. I_npairs, 8-bit, W x H x noc (noc 1 or 3, channels interleaved).  Ffw[k] is the flow
 * from frame k to k+1 and Frev[k] the flow from frame k+1 to k, each [H][W][2] fp32; both are required.  `weights` is a HOST
 * array of `radius` floats w_1 .. w_R, 1 <= radius <= OFDIS_TRAJ_MAX_RADIUS, each inside [0, 1]; it is copied into the launch
 * as the times of ofdis_interpolate are.  tau is the photometric gate of ofdis_temporal_filter; fb_check is 0 or 1; alpha and
 * beta are those of ofdis_fb_check.  Every operation is a separately rounded fp32 operation in this order, independent of the
 * arithmetic contract; inside, bil and the inequality are those of ofdis_track_points, sample that of ofdis_temporal_filter
 * (of_dis_amd/csrc/ofdis_upsample.h: fb_inside, fb_bilinear, fb_consistent, interp_sample).  For output frame f, pixel (x, y)
 * and c[ch] = (float) I_f[y][x][ch]:
 *   walk(dir):  p_0 = ((float)x, (float)y), alive; for j = 1 .. R while alive:
 *       forward:  k = f + j - 1, F = Ffw[k],  O = Frev[k], J = I_{f+j};  the direction ends when k >= npairs
 *       backward: k = f - j,     F = Frev[k], O = Ffw[k],  J = I_{f-j};  the direction ends when k < 0
 *       (u, v) = F[y][x] when j == 1 (read directly, as ofdis_temporal_filter does), else bil(F, p_{j-1})
 *       q = (p.x + u, p.y + v);  not inside(q): the direction ends                                      (NaN lands here)
 *       fb_check: (ru, rv) = bil(O, q);  du = u + ru, dv = v + rv;  lhs = du*du + dv*dv;
 *                 rhs = alpha * ((u*u + v*v) + (ru*ru + rv*rv)) + beta;  the direction ends unless lhs <= rhs
 *       p_j = q;  s_j[ch] = sample(J, q)[ch];  d = max over ch of fabsf(s_j[ch] - c[ch])
 *       g = fmaxf(1 - d / tau, 0);  w_j^dir = w_j * g
 *     every step not reached: w_j^dir = 0, s_j = 0
 *   num[ch] = c[ch]; den = 1; for j = 1 .. R:
 *       num[ch] = (num[ch] + w_j^back * s_j^back[ch]) + w_j^fwd * s_j^fwd[ch]
 *       den     = (den + w_j^back) + w_j^fwd
 *   out[ch] = (uint8) clamp((int)floorf(num[ch] / den + 0.5f), 0, 255)
 *   support = nf | (nb << 4),  nf / nb = how many forward / backward steps have w_j^dir > 0
 * A photometric gate of 0 does not end a direction: only leaving the image or failing the inequality does.
 * Consequences:
 *   - Radius 1 matches the existing filter.  With radius 1 and w_1 = wn, `out` holds the bytes of ofdis_temporal_filter on the
 *     same frames and flows -- with fb_check = 1 for mask_fw = ofdis_fb_check(Ffw, Frev) and mask_rev = ofdis_fb_check(Frev,
 *     Ffw), with fb_check = 0 for NULL masks -- for any flows, non-finite ones included, because step 1 reads the flow
 *     directly.  `support` differs only in format: bit 0 here is the old bit 1, bit 4 the old bit 0.
 *   - Zero weights return the clip.  All weights 0 returns the clip bit for bit (num = c, den = 1) with support 0.
 *   - Identical frames with zero flows return themselves (every sample is the pixel, d = 0, and the quotient lies within a few
 *     ulp of the integer c).
 *   - Reach matches a track.  For finite flows, the forward reach nf of pixel (x, y) of frame f with tau = +inf and all
 *     weights > 0 is count - 1 of the track that ofdis_track_points gives the seed (x, y) at seed frame f with max_steps = R
 *     (with flow_rev = Frev for fb_check = 1, NULL for 0).
 * The first frame has nb = 0 and the last nf = 0 everywhere.  of_dis_amd/temporal.py states the same arithmetic in numpy
 * (trajectory_filter_ref).
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_TRAJ_MAX_RADIUS 8
/* device arrays: frames, out [npairs+1][height][width][noc] u8; flow_fw, flow_rev [npairs][height][width][2] f32; support
 * [npairs+1][height][width] u8 or NULL (not written).  weights: HOST, [radius].  One lane per quad of four adjacent pixels;
 * 4-byte stores where width is a multiple of 4 and the array is 4-byte aligned, byte stores of the same bytes otherwise;
 * nothing outside `out` and `support` is written, and no device memory is allocated.  Enqueues on `stream`.
 * OFDIS_ERR_INVALID before any device work: a NULL frames, flow, out or weights pointer; out == frames; noc not 1 or 3; radius
 * outside 1..OFDIS_TRAJ_MAX_RADIUS; a weight outside [0, 1] or NaN; tau not positive, subnormal or NaN; fb_check not 0 or 1;
 * alpha or beta as ofdis_fb_check rejects them; npairs < 1; sizes as ofdis_fb_check rejects them. */
int ofdis_trajectory_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out,
                            uint8_t* support /* or NULL */, int npairs, int width, int height, int noc,
                            const float* weights /* host */, int radius, float tau, int fb_check, float alpha, float beta,
                            void* stream);
/* OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE contexts (both flags whatever fb_check is: walking back takes the reverse flows):
 * frames first_frame .. first_frame + count of the context (count + 1 output frames), straight from its level flows.
 * `frames`, out and support as for ofdis_batch_temporal_filter.  Only the pairs [first_frame, first_frame + count) are used:
 * a walk ends at the range's first and last frame even where the context holds more pairs, so a caller who filters a long
 * clip in ranges overlaps them by `radius` pairs on either side and keeps the frames in between.  Bit-identical to
 * ofdis_trajectory_filter applied to out_fw and out_rev of ofdis_batch_upsample_bidir(b, first_frame, count, ...) and to
 * frames + first_frame frames, under both contracts (the kernel is contract-independent, the level flows are not); the
 * full-resolution flows are never written.  Joins a pipelined pass by itself.
 * OFDIS_ERR_INVALID as ofdis_trajectory_filter, and for a NULL context, a context created without OFDIS_BATCH_SEQUENCE or
 * without OFDIS_BATCH_REVERSE, a pair range outside the batch, an original size above the padded size. */
int ofdis_batch_trajectory_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                  uint8_t* support, int width_org, int height_org, const float* weights /* host */,
                                  int radius, float tau, int fb_check, float alpha, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Global (camera) motion models and motion-compensated flow: per pair, a translation or a 6-parameter affine model of the flow
 * field fitted by trimmed least squares -- a least-squares fit, then rounds - 1 re-fits on the pixels whose residual under the
 * previous model is within thresh pixels -- and, given the models, the residual flow (flow minus model) with a label per pixel:
 * inlier (background, moves with the camera), outlier (moves on its own) or invalid.  The uses: subtracting the camera motion
 * before a two-stream quantisation, the input of a stabiliser, foreground / background segmentation, scene-change statistics.
 * Warping frames along a smoothed camera path -- stabilisation itself -- is the next section, "Video stabilisation".
 * The 8-parameter projective model, the first-order flow of a homography, is the section after this one ("Projective camera
 * models").
 * Not provided: similarity models, models of the reverse direction, the C++ sequence driver.
 *
 * The frame is W x H with both sides <= OFDIS_GM_MAX_SIDE.  F is the flow [H][W][2] fp32 of one pair, M its mask of OFDIS_FB_*
 * codes or NULL.  Centred, doubled coordinates are integers: X = 2x - (W-1), Y = 2y - (H-1).
 *   valid(x, y) = (M == NULL or M[y][x] == OFDIS_FB_CONSISTENT) and fabsf(u) <= OFDIS_GM_MAX_FLOW and fabsf(v) <= OFDIS_GM_MAX_FLOW
 *                                                           ((u, v) = F[y][x]; a NaN or an infinity fails the comparison)
 *   qu = (int)rintf(u * 256.0f), qv likewise                the product is exact, rintf rounds to nearest even; |q| <= 2^20
 * Sums over a pixel set S, twelve exact 64-bit integers:
 *   n = |S|, SX, SY, SXX, SXY, SYY,  Squ, SXqu, SYqu,  Sqv, SXqv, SYqv          (SXqu = sum of X * qu, and so on)
 * Bounds: a set has at most W * H pixels, |X| < W, |Y| < H and |q| <= 2^20, so |SXqu| < W * 2^20 * W * H = W^2 * H * 2^20 and,
 * with W, H <= 8192 = 2^13, every one of the twelve is below 2^13 * 2^13 * 2^13 * 2^20 = 2^59 (the second moments below
 * 2^52): int64 never overflows.
 * Integer addition is associative, so any mapping of pixels to lanes and any order of summation gives the same twelve numbers:
 * this is what lets the fused kernel use a different mapping from the standalone one and still return the same bits.
 * Solve, in fp64, every operation separately rounded (no contraction), int64 -> double the ordinary round-to-nearest
 * conversion; n, Sx ... are the sums as doubles, Su / Sxu / Syu those of qu, Sv / Sxv / Syv those of qv:
 *   c00 = Sxx*Syy - Sxy*Sxy   c01 = Sxy*Sy - Sx*Syy   c02 = Sx*Sxy - Sxx*Sy
 *   c11 = n*Syy - Sy*Sy       c12 = Sx*Sy - n*Sxy     c22 = n*Sxx - Sx*Sx
 *   det = (n*c00 + Sx*c01) + Sy*c02
 *   affine (model == OFDIS_GM_AFFINE and n >= 3 and det > 0):
 *       b0 = ((c00*Su + c01*Sxu) + c02*Syu) / det      a0 = b0 / 256
 *       b1 = ((c01*Su + c11*Sxu) + c12*Syu) / det      a1 = b1 / 128
 *       b2 = ((c02*Su + c12*Sxu) + c22*Syu) / det      a2 = b2 / 128
 *       and the same with Sv, Sxv, Syv for a3, a4, a5                          status OFDIS_GM_OK_AFFINE
 *   translation (asked for, or the fallback from affine, n >= 1):
 *       a0 = (Su / n) / 256, a3 = (Sv / n) / 256, the rest 0                   status OFDIS_GM_TRANSLATION
 *   n == 0: the model is all zeros                                             status OFDIS_GM_EMPTY
 * The model means u(x, y) = a0 + a1*(x - cx) + a2*(y - cy), v(x, y) = a3 + a4*(x - cx) + a5*(y - cy), cx = (W-1)/2, cy = (H-1)/2.
 * Caveat: on small sets every product above is exact, so a collinear set (one row, one diagonal) gives det == 0 exactly and
 * falls back to the translation; on very large collinear sets the products round and det is only approximately 0.
 * Residual, in fp32, every operation separately rounded:
 *   af_k = (float) a_k;  xc = (float)X * 0.5f;  yc = (float)Y * 0.5f
 *   mu = (af0 + af1*xc) + af2*yc;  mv = (af3 + af4*xc) + af5*yc;  ru = u - mu;  rv = v - mv
 *   r2 = ru*ru + rv*rv;  t2 = thresh*thresh (computed once);  near = valid and r2 <= t2      (a NaN gives false)
 * Rounds: S_0 = valid; for r >= 1, S_r = near under the model of round r-1.  Each round sums over its set and solves.  An empty
 * S_r with r >= 1 ends the process: the model and status of round r-1 stay.
 * of_dis_amd/gmotion.py states the same arithmetic in numpy.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_GM_MAX_SIDE   8192
#define OFDIS_GM_MAX_FLOW   4096.0f
#define OFDIS_GM_MAX_ROUNDS 8
enum { OFDIS_GM_TRANSLATION_ONLY = 0, OFDIS_GM_AFFINE = 1 };                    /* model */
enum { OFDIS_GM_OK_AFFINE = 0, OFDIS_GM_TRANSLATION = 1, OFDIS_GM_EMPTY = 2 };  /* status */
enum { OFDIS_GM_INLIER = 0, OFDIS_GM_OUTLIER = 1, OFDIS_GM_INVALID = 2 };       /* label */
/* bytes of the work buffer ofdis_global_motion needs (one 96-byte record of sums per workgroup and pair); 0 for sizes that
 * function rejects */
size_t ofdis_global_motion_work_bytes(int npairs, int width, int height);
/* device arrays: flow [npairs][height][width][2] f32; mask [npairs][height][width] u8 or NULL (all consistent); models
 * [npairs][6] f64; stats [npairs][3] int64 or NULL: |S_0|, the size of the last set used, the status; work: 8-byte aligned,
 * at least ofdis_global_motion_work_bytes.  All rounds are enqueued on `stream` without a host synchronisation: per round one
 * launch that sums all pairs (a workgroup writes one record into its own slot of `work` with plain stores; no atomics, no
 * waiting between workgroups) and one that solves (one wavefront per pair).  OFDIS_ERR_INVALID before any device work: a NULL
 * flow, models or work pointer; model not OFDIS_GM_TRANSLATION_ONLY or OFDIS_GM_AFFINE; rounds outside 1 ..
 * OFDIS_GM_MAX_ROUNDS; thresh not finite or <= 0; sizes as ofdis_fb_check rejects them or a side above OFDIS_GM_MAX_SIDE; a
 * work buffer that is too small or not 8-byte aligned. */
int ofdis_global_motion(const float* flow, const uint8_t* mask, int npairs, int width, int height, int model, int rounds,
                        float thresh, double* models, long long* stats, void* work, size_t work_bytes, void* stream);
/* One pass: residual[y][x] = (ru, rv) under the pair's model (NaN and infinities propagate), label[y][x] = OFDIS_GM_INLIER for
 * near, OFDIS_GM_OUTLIER for valid but not near, OFDIS_GM_INVALID otherwise.  residual [npairs][height][width][2] f32 and label
 * [npairs][height][width] u8: either may be NULL (not written), not both; residual may be `flow` itself.  16-byte stores of the
 * residual where width is even and the array 16-byte aligned, 4-byte stores of the labels where width is a multiple of 4 and
 * the array 4-byte aligned, narrower stores of the same bytes otherwise; nothing outside the two outputs is written.
 * OFDIS_ERR_INVALID before any device work: a NULL flow or models pointer, both outputs NULL, thresh and sizes as above. */
int ofdis_motion_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                            float thresh, float* residual, uint8_t* label, void* stream);
/* The same straight from the level flows of the pairs [first_frame, first_frame + count) of an optical-flow context (any kind:
 * plain, OFDIS_BATCH_REVERSE, OFDIS_BATCH_SEQUENCE); the full-resolution flow and the masks are never written.  models
 * [count][6], stats [count][3] or NULL, residual / label [count][height_org][width_org]([2]).
 * fb_check = 0: bit-identical to the standalone calls on what ofdis_batch_upsample_frames writes, with mask = NULL.
 * fb_check = 1 (needs OFDIS_BATCH_REVERSE): bit-identical to the standalone calls on out_fw and mask_fw of
 * ofdis_batch_upsample_bidir(b, first_frame, count, ..., alpha, beta).  Both under both contracts (the kernels are
 * contract-independent, the level flows are not).  The work buffer belongs to the context: allocated at the first call,
 * counted by ofdis_batch_device_bytes from then on.  Joins a pipelined pass by itself.  OFDIS_ERR_INVALID as the standalone
 * calls, and for a NULL context, a stereo-depth context, fb_check not 0 or 1, fb_check = 1 on a context created without
 * OFDIS_BATCH_REVERSE, alpha / beta as ofdis_fb_check rejects them, a pair range outside the batch, an original size above the
 * padded size or above OFDIS_GM_MAX_SIDE. */
int ofdis_batch_global_motion(ofdis_batch* b, int first_frame, int count, int model, int rounds, float thresh, int fb_check,
                              float alpha, float beta, double* models, long long* stats, int width_org, int height_org,
                              void* stream);
int ofdis_batch_motion_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh, int fb_check,
                                  float alpha, float beta, float* residual, uint8_t* label, int width_org, int height_org,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Projective camera models: the 8-parameter twins of the section above -- fit, compensate, and track selection under them.
 * An affine map cannot represent a pan or a tilt with perspective; the model here can, to first order.  It is the 8-parameter
 * QUADRATIC flow model, the instantaneous flow of a planar scene or of a rotating camera, with xc = x - (W-1)/2, yc = y - (H-1)/2:
 *   p = a6*xc + a7*yc
 *   u = a0 + a1*xc + a2*yc + p*xc
 *   v = a3 + a4*xc + a5*yc + p*yc
 * It is linear in a0 .. a7; a6 = a7 = 0 is the affine model of ofdis_global_motion in the same parametrisation; to first order it
 * is the flow of the homography [[1+a1, a2, a0], [a4, 1+a5, a3], [-a6, -a7, 1]] in centred coordinates.  It is THIS model and not
 * a DLT homography fit: being linear in its parameters it is fitted from exact integer sums like the affine one, whereas the
 * DLT needs moments of order x^2 * x'^2, which overflow 64 bits for a single pixel.
 * Stabilisation: ofdis_camera_path, ofdis_warp_frames and ofdis_batch_stabilize stay affine (the quadratic model is not closed
 * under composition).  The homography above is: the section "Projective video stabilisation" chains, averages and inverts the
 * camera path on it and resamples the frames by a perspective warp, from the models fitted here.
 * Not provided (out of scope): a DLT fit; similarity models; RANSAC; the C++ sequence driver.
 *
 * Everything that is not the model is word for word the section above: valid, qu = (int)rintf(u * 256.0f), X = 2x - (W-1),
 * Y = 2y - (H-1), near, the rounds (S_0 = valid, S_r = near under the model of round r-1, an empty later set leaves the previous
 * result), the labels, the store widths, the residual that may alias the flow.  Models are [npairs][8] fp64, a0 .. a7.
 * Sums over a pixel set S, 23 exact integers: the twelve of the section above, then
 *   XXX, XXY, XYY, YYY            (XXY = sum of X*X*Y, and so on)
 *   XXXX, XXXY, XXYY, XYYY, YYYY
 *   R6 = sum of (X*X*qu + X*Y*qv),  R7 = sum of (X*Y*qu + Y*Y*qv)
 * Bounds: |X|, |Y| < 2^13 and |q| <= 2^20, so per pixel a fourth moment is below 2^52 and |R6|, |R7| below 2^47; a workgroup
 * covers at most 1024 pixels, so every sum of its record fits int64 (a fourth moment at most 2^62).  A PAIR's sums do not: the
 * sum of X^4 over 8192 x 2 pixels already needs more than 63 bits, a full 8192 x 8192 frame reaches 2^78.  The records of a pair
 * are therefore added in 128 bits for these eleven sums, and each of them is converted to fp64 CORRECTLY ROUNDED (to nearest,
 * ties to even -- Python's float(int)).  The twelve old sums stay below 2^59 and convert as before.
 * Solve, in fp64, every operation separately rounded (no contraction).  In integer units b (u_q = b0 + b1 X + b2 Y + b6 X^2 + b7 XY,
 * v_q = b3 + b4 X + b5 Y + b6 XY + b7 Y^2) the symmetric normal matrix N and the right-hand side t are, all sums as doubles:
 *   rows and columns 0..2 and again 3..5: [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]]; zero between the two blocks
 *   column 6 (rows 0..5): Sxx, XXX, XXY, Sxy, XXY, XYY        column 7 (rows 0..5): Sxy, XXY, XYY, Syy, XYY, YYY
 *   N66 = XXXX + XXYY    N67 = XXXY + XYYY    N77 = XXYY + YYYY           (one fp64 addition each)
 *   t = (Su, Sxu, Syu, Sv, Sxv, Syv, R6, R7)
 * factored as L D L^T without a square root, column by column, every inner sum over ascending j:
 *   for k = 0 .. 7:   for i = k .. 7:  C_ik = N_ik;  for j = 0 .. k-1:  C_ik = C_ik - C_ij * L_kj
 *                     d_k = C_kk;  the pivot PASSES when d_k > N_kk * 2^-40;  for i = k+1 .. 7:  L_ik = C_ik / d_k
 *   for i = 0 .. 7:   z_i = t_i;  for j = 0 .. i-1:  z_i = z_i - L_ij * z_j
 *   for i = 7 .. 0:   b_i = z_i / d_i;  for j = i+1 .. 7:  b_i = b_i - L_ji * b_j
 *   a0 = b0/256, a1 = b1/128, a2 = b2/128, a3 = b3/256, a4 = b4/128, a5 = b5/128, a6 = b6/64, a7 = b7/64
 * Rank test: the projective branch is taken when n >= 4 and all eight pivots pass.  On exactly degenerate sets (one row, one
 * diagonal, H = 1, W = 1) a pivot is 0 or below 2.2e-16 of its diagonal entry; a 2 x 2 block in the corner of a 300 x 70 frame
 * has 1.2e-10, four random pixels 4e-3, a full frame 0.4: 2^-40 (9.1e-13) separates them.  Otherwise the solve of the section
 * above runs unchanged on the twelve sums with model = OFDIS_GM_AFFINE: a0 .. a5 are the bits ofdis_global_motion gives on the
 * same set, a6 = a7 = 0.
 * stats[k] = { |S_0|, the size of the last set used, the number of parameters of the model that was solved: 8, 6 (affine), 2
 * (translation) or 0 (empty) }.
 * Residual, in fp32, every operation separately rounded; xc, yc as in the section above ((float)X * 0.5f):
 *   p = af6*xc + af7*yc
 *   mu = ((af0 + af1*xc) + af2*yc) + p*xc;  mv = ((af3 + af4*xc) + af5*yc) + p*yc;  ru = u - mu;  rv = v - mv
 * Consequence: with a6 = a7 = 0 every output equals that of the 6-parameter function under == (only the sign of a zero may
 * differ).  of_dis_amd/gmotion.py states the same arithmetic in numpy (projective_motion_ref, projective_compensate_ref).
 * ------------------------------------------------------------------------------------------- */
/* bytes of the work buffer ofdis_projective_motion needs (one record of 24 x 8 bytes per workgroup and pair: the 23 sums and a
 * word of padding); 0 for sizes that function rejects */
size_t ofdis_projective_motion_work_bytes(int npairs, int width, int height);
/* ofdis_global_motion without `model`: models [npairs][8] f64, stats [npairs][3] int64 or NULL as stated above; the same
 * launches (per round one that sums all pairs -- one record per workgroup, plain stores, no atomics -- and one that solves, one
 * wavefront per pair, which adds the pair's records in 128 bits), no host synchronisation, the same OFDIS_ERR_INVALID cases
 * before any device work. */
int ofdis_projective_motion(const float* flow, const uint8_t* mask, int npairs, int width, int height, int rounds, float thresh,
                            double* models, long long* stats /* or NULL */, void* work, size_t work_bytes, void* stream);
/* ofdis_motion_compensate under models [npairs][8]: the same outputs, store widths, aliasing rule and rejections. */
int ofdis_projective_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                                float thresh, float* residual, uint8_t* label, void* stream);
/* ofdis_batch_global_motion / ofdis_batch_motion_compensate under the 8-parameter model: straight from the level flows, fb_check
 * as there, bit-identical to the two standalone calls above on what ofdis_batch_upsample_frames / ofdis_batch_upsample_bidir
 * write, under both contracts.  The work buffer is a slab of its own that belongs to the context: allocated at the first call,
 * counted by ofdis_batch_device_bytes from then on.  Joins a pipelined pass by itself.  OFDIS_ERR_INVALID as the 6-parameter calls. */
int ofdis_batch_projective_motion(ofdis_batch* b, int first_frame, int count, int rounds, float thresh, int fb_check, float alpha,
                                  float beta, double* models, long long* stats, int width_org, int height_org, void* stream);
int ofdis_batch_projective_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh,
                                      int fb_check, float alpha, float beta, float* residual, uint8_t* label, int width_org,
                                      int height_org, void* stream);
/* ofdis_track_select with models [npairs][8] of ofdis_projective_motion: the residual step of a slot becomes
 *   pq = af6*xc + af7*yc;  mu = ((af0 + af1*xc) + af2*yc) + pq*xc;  mv = ((af3 + af4*xc) + af5*yc) + pq*yc
 * with xc = x_j - (float)(W-1)*0.5f, yc = y_j - (float)(H-1)*0.5f as there; everything else, the rejections included, is that
 * function's.  A track that follows an 8-parameter model exactly is OFDIS_TS_CAMERA with it and kept without. */
int ofdis_track_select_projective(const float* tracks, const int* start, const int* len, const long long* info, int lmax,
                                  int max_tracks, const double* models /* or NULL */, int npairs, int width, int height,
                                  const ofdis_track_select_params* p, uint8_t* code /* or NULL */,
                                  long long* counts /* or NULL */, int max_tracks_out, float* tracks_out, int* start_out,
                                  int* len_out, long long* info_out, int* index /* or NULL */, float* shape_out /* or NULL */,
                                  void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Segments: connected components of a label map, small ones removed, one record per segment.  The step from the byte per pixel
 * that ofdis_motion_compensate and ofdis_projective_compensate write to objects: the things that move against the camera are the
 * components of the OFDIS_GM_OUTLIER pixels; the occlusion regions of a pair are those of an OFDIS_FB_* mask.
 * Not provided: morphological opening or closing before labelling; hole filling; association of segments across frames by this
 * call (the section "Object tracks" below does it: ofdis_segment_tracks); a form
 * that reads a context's level flows directly (composing from materialised arrays wins, as the measurements of the fused
 * global-motion, trajectory-filter and projective routes in README.md show: the labels come from either compensate call); the
 * C++ sequence driver.
 *
 * label is [nmaps][H][W] u8, any byte map: OFDIS_GM_* labels, OFDIS_FB_* masks, or the caller's own.
 * Foreground: codes is a bit set; pixel p is foreground iff label[p] < 8 and ((codes >> label[p]) & 1).  A byte of 8 or more is
 * never foreground, so no shift by 8 or more is ever made.  Moving objects: codes = 1u << OFDIS_GM_OUTLIER.
 * Connectivity: conn = 4 (edge neighbours) or 8 (edge and corner neighbours).  A component is a maximal connected set of
 * foreground pixels within one map; maps never interact.
 * Canonical numbering: the root of a component is its smallest raster index y*W + x; the components are ordered by ascending
 * root, ncomp is their number; a component is kept iff area >= max(min_area, 1); the kept ones are numbered 1 .. nkept in the same
 * order.  With min_area <= 1 this is what scipy.ndimage.label returns for the 4- or 8-structure.
 * segments [nmaps][H][W] int32: 0 for background and for removed components, k for the k-th kept component.  Every entry is
 * written once; nothing relies on a memset.  Segments beyond max_segments are still numbered here.
 * records [nmaps][max_segments][12] int64: record k-1 of a map belongs to kept segment k, for k <= min(nkept, max_segments):
 *   { area, root, xmin, ymin, xmax, ymax, sx, sy, nflow, squ, sqv, 0 }
 * The box is inclusive; sx and sy are the sums of x and of y over the segment (the centroid is sx/area, sy/area).  flow is
 * [nmaps][H][W][2] f32 or NULL -- the residual of the compensate call, or any other flow.  A pixel of the segment is usable iff
 * fabsf(u) <= OFDIS_GM_MAX_FLOW and fabsf(v) <= OFDIS_GM_MAX_FLOW (a NaN fails this); nflow counts the usable pixels, squ is the
 * sum of (int)rintf(u * 256.0f) over them and sqv that of v: the quantisation of "Global (camera) motion models" (the mean
 * residual of the segment is squ / (256 nflow)).  Without flow the three are 0.  The slots at or beyond min(nkept, max_segments)
 * are neither read nor written.
 * info [nmaps][4] int64: { ncomp, nkept, min(nkept, max_segments), the number of foreground pixels }.
 * Limits (in prose: the section adds no macro; of_dis_amd/capi.py and of_dis_amd/segments.py carry them as SEG_MAX_SEGMENTS = 2^24,
 * SEG_RECORD_FIELDS = 12, SEG_INFO_FIELDS = 4): max_segments is 1 .. 16777216; both sides are at most OFDIS_GM_MAX_SIDE.
 * Bounds: W, H <= 8192 = 2^13, so a raster index is below 2^26 and fits int32, as do area, ncomp and every number; sx < 2^26 *
 * 2^13 = 2^39 and sy likewise; |q| <= 2^20, so |squ| <= 2^26 * 2^20 = 2^46: int64 never overflows.
 * Order independence: integer min, max and add are associative and commutative, and the root of a component is a minimum, so
 * every output is a pure function of the inputs whatever the order in which the unions are made and the atomics arrive: two
 * calls give the same bits.  of_dis_amd/segments.py states the definition in numpy (label_segments_ref).
 * ------------------------------------------------------------------------------------------- */
/* bytes of the work buffer ofdis_label_segments needs: nmaps * (8 * W*H + 16 * ceil(W*H / 256)) -- the parent and the area /
 * number of every pixel (int32 [nmaps][H*W] each) and four int32 of counts per block of 256 pixels; 0 for sizes that function
 * rejects */
size_t ofdis_segments_work_bytes(int nmaps, int width, int height);
/* device arrays as stated above; work: 8-byte aligned, at least ofdis_segments_work_bytes.  label is read by several of the
 * launches, which rely on finding the same bytes each time: whatever writes it must be ordered before the call on `stream`,
 * and it must not change until the call's work has completed.  Seven launches are enqueued on
 * `stream` without a host synchronisation: row runs from a wavefront ballot, unions by integer atomicMin on the parent array (no
 * workgroup waits for another), a flattening pass, the areas, a two-level prefix sum over the kept roots in raster order, the
 * records' initial values, and the relabelling pass that also accumulates the records with integer atomics (no floating-point
 * atomic anywhere).  OFDIS_ERR_INVALID before any device work: a NULL label, info or work pointer; segments and records both
 * NULL; codes 0 or with a bit above bit 7; conn not 4 or 8; min_area < 0; max_segments outside 1 .. 16777216; sizes as
 * ofdis_fb_check rejects them or a side above OFDIS_GM_MAX_SIDE; a work buffer that is too small or not 8-byte aligned. */
int ofdis_label_segments(const uint8_t* label, const float* flow /* or NULL */, int nmaps, int width, int height, unsigned codes,
                         int conn, int min_area, int max_segments, int* segments /* or NULL */, long long* records /* or NULL */,
                         long long* info, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Object tracks: the segments of consecutive maps of a clip linked across frames.  ofdis_label_segments numbers the moving
 * objects of every frame pair on its own; here segment a of map k and segment b of map k + 1 become the same object where the
 * forward flow carries most of one onto the other, the links are chained into numbered tracks with one record each, and the
 * maps are relabelled by track.  Four steps, each a call of its own, and ofdis_segment_tracks, which enqueues all four.
 * Not provided: split and merge events (a split or a merge ends tracks and starts new ones; the caller has `overlap` to find
 * them); tracks across a gap (an object that is not recorded in one map comes back as a new track); a sparse overlap for more
 * than 1024 segments per map; a form that reads a context's level flows directly (any full-resolution forward flow will do:
 * that of ofdis_batch_upsample_bidir, for example); the C++ sequence driver.
 *
 * Notation: N = nmaps, the maps of a clip in frame order, map k in the coordinates of frame k; S = max_segments, the value
 * ofdis_label_segments was called with.  segments [N][H][W] int32, records [N][S][12] int64 and info [N][4] int64 are as that
 * call wrote them; flow is [N][H][W][2] f32, flow k taking frame k to frame k + 1 (the flow of the last map is never read).
 * n_k = min(max(info[k][2], 0), S), read on the device, never by the host.  A value s in map k is RECORDED iff 1 <= s <= n_k;
 * every other value (0, negative, above n_k) is background here, so arbitrary int32 maps never index out of range.
 * Integers throughout; the one floating-point step is (int)rintf(u), round to nearest even.
 *
 * 1. Overlap.  For k = 0 .. N-2 and every pixel (x, y) of map k whose value a is recorded in map k: (u, v) = flow[k][y][x] is
 * usable iff fabsf(u) <= 4096 && fabsf(v) <= 4096 (a NaN fails this); xt = x + (int)rintf(u), yt = y + (int)rintf(v); if
 * (xt, yt) is inside the frame and b = segments[k+1][yt][xt] is recorded in map k + 1, overlap[k][a-1][b-1] += 1.
 * overlap is [N-1][S][S] int32.  Only the entries (i, j) with i < n_k and j < n_{k+1} are defined, zeros included: the call
 * clears them itself (a launch of its own before the accumulating one); the rest is neither read nor written.
 * Two routes give the same bits: wavefront-aggregated integer atomics on global memory for every S, and for S <= 128 a
 * histogram in LDS per workgroup and band of rows (S * S * 4 <= 64 KiB), whose non-zero entries are then added to global memory.
 *
 * 2. Link: mutual best match.  Within pair k, c(a, b) = overlap[k][a-1][b-1]; fbest(a) is the recorded b with the largest
 * c(a, b), among equals the smallest b, none if every c(a, b) is 0; bbest(b) is the same over a.  link[k][a-1] = b iff
 * c(a, b) > 0 and fbest(a) = b and bbest(b) = a and c * 100 >= min_share * min(area_k(a), area_{k+1}(b)), compared in int64,
 * and 0 otherwise; area is records[..][0] clamped to 0 .. 2^26; min_share is 0 .. 100 (per cent of the smaller segment).
 * link is [N-1][S] int32; the entries a-1 < n_k are defined, the rest is neither read nor written.  Links are injective by
 * construction: no two a share a b.  A split or a merge therefore ends tracks and starts new ones.
 *
 * 3. Chain.  (k, s) is BORN iff k = 0 or no a has link[k-1][a-1] = s (only a <= n_{k-1} and values 1 .. n_k count).  The born
 * (k, s) are ordered by k, then by s, and numbered 1 .. ntracks.  ids[k][s-1] is its own number if born, otherwise the id of
 * its predecessor a (for a link array that is not injective -- not one of step 2 -- the smallest such a).  ids is [N][S] int32,
 * defined for s <= n_k.  tracks is [max_tracks][12] int64; record t-1 is written for t <= min(ntracks, max_tracks):
 *   { first_map, first_segment, length, last_segment, sum area, sum sx, sum sy, sum nflow, sum squ, sum sqv, min area, max area }
 * the sums over the member segments' record fields 0, 6, 7, 8, 9 and 10, in two's-complement arithmetic (garbage records wrap
 * instead of being undefined); min and max of field 0 as it stands.  The slots beyond min(ntracks, max_tracks) are neither
 * read nor written.  tinfo [4] int64: { ntracks, min(ntracks, max_tracks), the number of links followed (segments that are
 * not born), the longest length }.  N = 1 is valid: every recorded segment is a track of length 1.
 *
 * 4. Relabel.  track_map[k][y][x] = ids[k][s-1] if s = segments[k][y][x] is recorded, else 0; every entry is written once.
 *
 * Limits (in prose: the section adds no macro; of_dis_amd/capi.py and of_dis_amd/segments.py carry them as SEGTRACK_MAX_SEGMENTS
 * = 1024, SEGTRACK_MAX_MAPS = 65536, SEGTRACK_MAX_TRACKS = 2^24, SEGTRACK_FIELDS = 12, SEGTRACK_INFO_FIELDS = 4,
 * SEGTRACK_LDS_MAX_SEGMENTS = 128): nmaps is 1 .. 65536, max_segments 1 .. 1024, max_tracks 1 .. 16777216, both sides at most
 * OFDIS_GM_MAX_SIDE.
 * Bounds: a count is at most W*H < 2^26 and fits int32; c * 100 < 2^33 and min_share * area <= 100 * 2^26 < 2^33.  With N <=
 * 65536 = 2^16 and S <= 1024 = 2^10, ntracks <= N*S <= 2^26 fits int32, as does a length (<= N).  Over a track of at most 2^16
 * segments of label_segments' records: sum area <= 2^26 * 2^16 = 2^42, sum sx < 2^39 * 2^16 = 2^55 and sum sy likewise,
 * |sum squ| <= 2^46 * 2^16 = 2^62: int64 never overflows on records that call wrote.
 * Order independence: integer adds and minima are associative and commutative, so every output is a pure function of the
 * inputs whatever the order in which the atomics arrive: two calls give the same bits.  of_dis_amd/segments.py states the
 * definitions in numpy (segment_overlap_ref, segment_link_ref, segment_chain_ref, segment_relabel_ref, segment_tracks_ref).
 * Every call below enqueues on `stream` without a host synchronisation; no workgroup waits for another; there is no
 * floating-point atomic.  OFDIS_ERR_INVALID before any device work: a NULL required pointer; nmaps outside 1 .. 65536;
 * max_segments outside 1 .. 1024; min_share outside 0 .. 100; max_tracks outside 1 .. 16777216; sizes as ofdis_label_segments
 * rejects them; a work buffer that is too small or not 8-byte aligned.
 * ------------------------------------------------------------------------------------------- */
/* bytes of the work buffer ofdis_segment_tracks needs: 8 * ceil((N-1) * S * (S+1) * 4 / 8), at least 8 -- overlap
 * [N-1][S][S] and link [N-1][S], int32 each; 0 for arguments that function rejects */
size_t ofdis_segment_tracks_work_bytes(int nmaps, int max_segments);
/* step 1: two launches (clear, accumulate); with nmaps = 1 nothing is launched */
int ofdis_segment_overlap(const int* segments, const float* flow, const long long* info, int nmaps, int width, int height,
                          int max_segments, int* overlap, void* stream);
/* step 2: one workgroup per pair computes the row and column arg-maxima; with nmaps = 1 nothing is launched */
int ofdis_segment_link(const int* overlap, const long long* records, const long long* info, int nmaps, int max_segments,
                       int min_share, int* link, void* stream);
/* step 3: one workgroup walks the maps in order, a few barriers per map */
int ofdis_segment_chain(const int* link, const long long* records, const long long* info, int nmaps, int max_segments,
                        int max_tracks, int* ids, long long* tracks, long long* tinfo, void* stream);
/* step 4 */
int ofdis_segment_relabel(const int* segments, const int* ids, const long long* info, int nmaps, int width, int height,
                          int max_segments, int* track_map, void* stream);
/* steps 1 to 4 (4 only with a track_map) on `stream`, overlap and link in `work` (8-byte aligned, at least
 * ofdis_segment_tracks_work_bytes): the same bits as the four calls */
int ofdis_segment_tracks(const int* segments, const float* flow, const long long* records, const long long* info, int nmaps,
                         int width, int height, int max_segments, int min_share, int max_tracks, int* ids, long long* tracks,
                         long long* tinfo, int* track_map /* or NULL */, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Video stabilisation: the per-pair camera models of a clip turned into one correcting warp per frame -- the classical
 * Gaussian motion filter: the motions relative to a frame averaged over a window around it -- and the frames resampled by their
 * warps.  Two operations, each stated below one step at a time, both independent of the arithmetic contract.
 * The 8-parameter models of ofdis_projective_motion take the same route on 3 x 3 maps in the section after this one,
 * "Projective video stabilisation"; the three functions here stay affine.
 * Not provided: a DLT homography fit (the projective path takes the quadratic-flow models as they are), similarity models,
 * rolling-shutter correction, automatic crop or zoom selection, inpainting of the exposed border, the C++ sequence driver,
 * stereo contexts.
 *
 * Conventions.  A warp is six doubles b0 .. b5 in the parametrisation of a model of ofdis_global_motion: the displacement field
 * (b0 + b1*xc + b2*yc, b3 + b4*xc + b5*yc) in centred coordinates xc = x - (W-1)/2, yc = y - (H-1)/2; all zeros is the
 * identity.  A map M = (a, b, c, d, tx, ty) means x' = a*xc + b*yc + tx, y' = c*xc + d*yc + ty.  The model a0 .. a5 of pair k
 * is read as the map T_k = (1 + a1, a2, a4, 1 + a5, a0, a3): it takes a position in frame k to the same scene point in frame
 * k+1.
 *
 * Camera path: models [npairs][6] fp64 and the window w_0 .. w_radius -> warps [npairs+1][6] fp64, one per frame.  Every
 * operation is a separately rounded fp64 operation (no contraction) in this order:
 *   det(M) = M.a*M.d - M.b*M.c
 *   ok(det) = OFDIS_STAB_MIN_DET <= det <= OFDIS_STAB_MAX_DET                                       (a NaN fails the test)
 *   usable(k) = all six numbers of the model finite and ok(det(T_k)).  An unusable pair is a break -- a scene cut, a failed
 *       fit -- and no window reaches across it.
 *   T o M (M first):  a = T.a*M.a + T.b*M.c   b = T.a*M.b + T.b*M.d   c = T.c*M.a + T.d*M.c   d = T.c*M.b + T.d*M.d
 *                     tx = (T.a*M.tx + T.b*M.ty) + T.tx               ty = (T.c*M.tx + T.d*M.ty) + T.ty
 *   inv(T), D = det(T):  a = T.d / D   b = (0 - T.b) / D   c = (0 - T.c) / D   d = T.a / D       (0 - x: a zero stays +0)
 *                     tx = 0 - (a*T.tx + b*T.ty)   ty = 0 - (c*T.tx + d*T.ty)                   (a, b, c, d: the new ones)
 *   For frame f:  acc = (w_0, 0, 0, w_0, 0, 0) (w_0 times the identity), sw = w_0, Mf = Mb = identity, and for j = 1, 2, ...
 *   while j <= radius and f + j - 1 < npairs and f - j >= 0 and usable(f + j - 1) and usable(f - j):
 *       Mf = T_{f+j-1} o Mf;   Mb = inv(T_{f-j}) o Mb                      the motions from frame f to frames f + j and f - j
 *       acc.e = acc.e + (w_j*Mf.e + w_j*Mb.e)  for each of the six numbers e;   sw = sw + (w_j + w_j)
 *   The walk stops at the first j that fails: the reach is r_f = min(radius, fwd_f, back_f) with fwd_f / back_f the numbers
 *   of consecutive usable pairs f, f+1, ... / f-1, f-2, ...; the window is truncated symmetrically, so a uniform pan is left
 *   alone wherever the window is truncated, and the first frame, the last frame and the frames at a break get Q = identity.
 *   Motions are relative to frame f, not a path accumulated from frame 0: rounding error does not grow with the length of the
 *   clip and every frame is an independent piece of work.
 *       Q = acc / sw  (six divisions);   D = det(Q)
 *       W = inv(Q) where ok(D) and all six numbers of inv(Q) are finite, else the identity          the backward map:
 *                                                                                                   out_f(x) = I_f(W x)
 *       s = 1 / zoom;  the zoom about the centre, W o scale(s), hides the border a correction exposes:
 *       b0 = W.tx   b1 = W.a*s - 1   b2 = W.b*s   b3 = W.ty   b4 = W.c*s   b5 = W.d*s - 1
 *   The weights are a HOST array of radius + 1 doubles, copied into the launch as the times of ofdis_interpolate are: finite,
 *   w_0 > 0, the others >= 0, 0 <= radius <= OFDIS_STAB_MAX_RADIUS.  Their shape is the caller's (a Gaussian:
 *   of_dis_amd/stabilize.py: gaussian_weights); no transcendental function runs on the device.  1 <= zoom <= OFDIS_STAB_MAX_ZOOM.
 *
 * Frame warp: frames [n][H][W][noc] u8 and warps [n][6] fp64 -> out, the same shape, and inside [n][H][W] u8 (optional).  For
 * pixel (x, y) of frame f, every operation is a separately rounded fp32 operation in this order; positions are built as the
 * residual of ofdis_motion_compensate is, every pixel from its own expression and never by an increment from its neighbour:
 *   bf_k = (float) b_k;   X = 2x - (W-1), Y = 2y - (H-1);   xc = (float)X * 0.5f, yc = (float)Y * 0.5f
 *   mu = (bf0 + bf1*xc) + bf2*yc;   mv = (bf3 + bf4*xc) + bf5*yc;   p = ((float)x + mu, (float)y + mv)
 *   ins = inside(p)       0 <= px <= W-1 and 0 <= py <= H-1, as in ofdis_fb_check (a NaN gives false)
 *   c[ch] = sample(I_f, pc)[ch], pc = (fminf(fmaxf(px, 0), W-1), fminf(fmaxf(py, 0), H-1)): the clamped bilinear expression of
 *       ofdis_interpolate above (a NaN coordinate clamps to 0)
 *   OFDIS_BORDER_CONSTANT: where not ins, c[ch] = 0.   OFDIS_BORDER_REPLICATE: c as sampled, everywhere.
 *   out[ch] = (uint8) clamp((int)floorf(c[ch] + 0.5f), 0, 255);   inside = ins ? 1 : 0
 * Consequences: a zero warp returns the frame bit for bit (p = (x, y), the sample is the pixel), and a warp that is an integer
 * translation (b0, b3 integers, the rest 0) returns the frame shifted by it bit for bit (p is an integer position: the
 * bilinear weights are 0 and 1), under OFDIS_BORDER_CONSTANT with zeros on the uncovered border.
 * of_dis_amd/stabilize.py states the same arithmetic in numpy.
 * ------------------------------------------------------------------------------------------- */
#define OFDIS_STAB_MAX_RADIUS 64
#define OFDIS_STAB_MIN_DET    0.25
#define OFDIS_STAB_MAX_DET    4.0
#define OFDIS_STAB_MAX_ZOOM   16.0
enum { OFDIS_BORDER_CONSTANT = 0, OFDIS_BORDER_REPLICATE = 1 };                 /* border */
/* device arrays: models [npairs][6] f64, warps [npairs+1][6] f64; weights: HOST, radius + 1 doubles.  One lane per frame, one
 * launch on `stream`, no host synchronisation.  OFDIS_ERR_INVALID before any device work: a NULL models, weights or warps
 * pointer; radius, the weights or zoom outside the ranges above; npairs < 1. */
int ofdis_camera_path(const double* models, int npairs, const double* weights /* host */, int radius, double zoom,
                      double* warps, void* stream);
/* device arrays: frames, out [nframes][height][width][noc] u8; warps [nframes][6] f64; inside [nframes][height][width] u8 or
 * NULL (not written).  One lane per quad of four adjacent pixels; 4-byte stores where width is a multiple of 4 and the array is
 * 4-byte aligned, byte stores of the same bytes otherwise; nothing outside `out` and `inside` is written.  Enqueues on
 * `stream`.  OFDIS_ERR_INVALID before any device work: a NULL frames, warps or out pointer; out == frames; noc not 1 or 3; a
 * border that is not OFDIS_BORDER_CONSTANT or OFDIS_BORDER_REPLICATE; nframes < 1; sizes as ofdis_fb_check rejects them or a
 * side above OFDIS_GM_MAX_SIDE. */
int ofdis_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside /* or NULL */, int nframes,
                      int width, int height, int noc, int border, void* stream);
/* OFDIS_BATCH_SEQUENCE contexts: frames first_frame .. first_frame + count of the context (count + 1 output frames)
 * stabilised over the pairs [first_frame, first_frame + count).  `frames` is the whole packed clip
 * [nframes+1][height_org][width_org][noc] given to ofdis_batch_build_pyramids_u8_seq; out = [count+1][height_org][width_org]
 * [noc], inside = [count+1][height_org][width_org] or NULL, warps = device [count+1][6] or NULL.  The composition, all enqueued
 * on `stream`: ofdis_batch_global_motion(b, first_frame, count, model, rounds, thresh, fb_check, alpha, beta, ...), then
 * ofdis_camera_path on its models, then ofdis_warp_frames on frames + first_frame frames -- bit-identical to those three calls
 * made separately, under both contracts (the kernels are contract-independent, the level flows are not).  Models and warps
 * live in an array of the context: allocated at the first call, counted by ofdis_batch_device_bytes from then on; the warps are
 * copied to `warps` when one is given.  Joins a pipelined pass by itself.  OFDIS_ERR_INVALID as the two calls above and as
 * ofdis_batch_global_motion (fb_check = 1 needs OFDIS_BATCH_REVERSE), and for a NULL context or a context created without
 * OFDIS_BATCH_SEQUENCE (the pairs of any other context are no chain). */
int ofdis_batch_stabilize(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int model, int rounds,
                          float thresh, int fb_check, float alpha, float beta, const double* weights /* host */, int radius,
                          double zoom, int border, uint8_t* out, uint8_t* inside /* or NULL */,
                          double* warps /* device [count+1][6] or NULL */, int width_org, int height_org, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Projective video stabilisation: the section above for the 8-parameter models of ofdis_projective_motion.  The quadratic flow
 * model does not compose, but the map it is the first-order flow of does: the path is chained, averaged and inverted on 3 x 3
 * maps, and the frames are resampled by a true perspective warp -- a pan or a tilt leaves no keystone wobble at the corners.
 * Both operations are independent of the arithmetic contract.  The affine functions are unchanged.
 * Not provided: a DLT fit, similarity models, rolling-shutter correction, automatic crop or zoom selection, inpainting of the
 * exposed border, the C++ sequence driver, stereo contexts.
 *
 * Conventions.  A warp is eight doubles g0 .. g7, the map [[1+g1, g2, g0], [g4, 1+g5, g3], [-g6, -g7, 1]] in centred
 * coordinates xc = x - (W-1)/2, yc = y - (H-1)/2: all zeros is the identity, g6 = g7 = 0 is the affine warp b0 .. b5 of
 * ofdis_warp_frames.  A map M = (a, b, c, d, tx, ty, gx, gy), with an implicit 1 in the corner, means
 *   x' = (a*xc + b*yc + tx) / (1 + gx*xc + gy*yc),   y' = (c*xc + d*yc + ty) / (1 + gx*xc + gy*yc).
 * The model a0 .. a7 of pair k is read as T_k = (1 + a1, a2, a4, 1 + a5, a0, a3, 0 - a6, 0 - a7).
 *
 * Camera path: models [npairs][8] fp64, the frame size W x H and the window w_0 .. w_radius -> warps [npairs+1][8] fp64.
 * Every operation is a separately rounded fp64 operation (no contraction) in this order; det and ok are the section above's:
 *   hx = (W-1)/2, hy = (H-1)/2                                                                       (exact in fp64)
 *   usable(M) = all eight numbers finite, and ok(M.a*M.d - M.b*M.c), and
 *               (1 - |M.gx|*hx) - |M.gy|*hy >= 0.5                                                   (a NaN fails each test)
 *       The last test keeps the denominator at or above 0.5 on every pixel of the frame, which is why the path takes the
 *       frame size.  usable(k) = usable(T_k); an unusable pair is a break.
 *   T o M (M first), the 3 x 3 product in this order, then all eight divided by n:
 *       a = (T.a*M.a + T.b*M.c) + T.tx*M.gx     b = (T.a*M.b + T.b*M.d) + T.tx*M.gy
 *       c = (T.c*M.a + T.d*M.c) + T.ty*M.gx     d = (T.c*M.b + T.d*M.d) + T.ty*M.gy
 *       tx = (T.a*M.tx + T.b*M.ty) + T.tx       ty = (T.c*M.tx + T.d*M.ty) + T.ty
 *       gx = (T.gx*M.a + T.gy*M.c) + M.gx       gy = (T.gx*M.b + T.gy*M.d) + M.gy
 *       n = (T.gx*M.tx + T.gy*M.ty) + 1
 *   inv(T): the adjugate divided by its corner entry D = T.a*T.d - T.b*T.c, the determinant the usable test guards:
 *       a = (T.d - T.ty*T.gy) / D        b = (T.tx*T.gy - T.b) / D        c = (T.ty*T.gx - T.c) / D        d = (T.a - T.tx*T.gx) / D
 *       tx = (T.b*T.ty - T.tx*T.d) / D   ty = (T.tx*T.c - T.a*T.ty) / D   gx = (T.c*T.gy - T.d*T.gx) / D   gy = (T.b*T.gx - T.a*T.gy) / D
 *   The walk, the window, its symmetric truncation and the breaks are word for word those of ofdis_camera_path, on eight
 *   numbers: acc = w_0 times the identity (w_0, 0, 0, w_0, 0, 0, 0, 0), sw = w_0, Mf = Mb = identity, and for j = 1, 2, ...
 *   while j <= radius and f + j - 1 < npairs and f - j >= 0 and usable(f + j - 1) and usable(f - j):
 *       Mf = T_{f+j-1} o Mf;   Mb = inv(T_{f-j}) o Mb
 *       acc.e = acc.e + (w_j*Mf.e + w_j*Mb.e)  for each of the eight numbers e;   sw = sw + (w_j + w_j)
 *       Q = acc / sw  (eight divisions)
 *       W = inv(Q) where usable(Q) and usable(inv(Q)) (so all eight numbers of inv(Q) are finite), else the identity
 *       s = 1 / zoom:   g0 = W.tx   g1 = W.a*s - 1   g2 = W.b*s   g3 = W.ty   g4 = W.c*s   g5 = W.d*s - 1
 *                       g6 = 0 - W.gx*s   g7 = 0 - W.gy*s
 *   Weights, radius and zoom as in the section above.
 *
 * Frame warp: frames [n][H][W][noc] u8 and warps [n][8] fp64 -> out and inside as ofdis_warp_frames writes them.  fp32, every
 * operation separately rounded, in DISPLACEMENT form, so that it degenerates exactly to the affine warp; gf_k = (float) g_k,
 * xc and yc as there:
 *   e = gf6*xc + gf7*yc;   D = 1.0f - e;   r = 1.0f / D                  (one correctly rounded division per pixel)
 *   mu = ((gf0 + gf1*xc) + gf2*yc) + e*xc;   mv = ((gf3 + gf4*xc) + gf5*yc) + e*yc
 *   p = ((float)x + mu*r, (float)y + mv*r)
 *   ins = D > 0 and inside(p)                                            (a NaN fails the test)
 * Clamping, sampling, border, rounding, out and inside are exactly those of ofdis_warp_frames.  (mu, mv) / D is the exact
 * displacement of the map above, and its numerator is the quadratic model of "Projective camera models".
 * Consequences.  With g6 = g7 = 0 every byte of out and inside equals ofdis_warp_frames on g0 .. g5 (e = +-0, D = 1, r = 1).  A
 * zero warp returns the frame bit for bit, an integer translation (g0, g3 integers, the rest 0) the shifted frame bit for bit.
 * With a6 = a7 = 0 models the path has g6 = g7 = 0 exactly and g0 .. g5 agree with ofdis_camera_path to rounding, not to the
 * bit: the translation of the inverse is rounded differently (here from the adjugate, there from the inverted linear part).
 * of_dis_amd/stabilize.py states the same arithmetic in numpy (camera_path_projective_ref, warp_frames_projective_ref;
 * STAB_MIN_DENOM there and in of_dis_amd/capi.py is the 0.5 of usable).
 * ------------------------------------------------------------------------------------------- */
/* device arrays: models [npairs][8] f64, warps [npairs+1][8] f64; weights: HOST, radius + 1 doubles; width, height: the frame
 * size of the clip the models were fitted on.  One lane per frame, one launch on `stream`, no host synchronisation.
 * OFDIS_ERR_INVALID before any device work: a NULL models, weights or warps pointer; radius, the weights or zoom outside their
 * ranges; npairs < 1; a side outside 1 .. OFDIS_GM_MAX_SIDE. */
int ofdis_camera_path_projective(const double* models, int npairs, int width, int height, const double* weights /* host */,
                                 int radius, double zoom, double* warps, void* stream);
/* ofdis_warp_frames under warps [nframes][8]: the same arrays, store widths and rejections. */
int ofdis_warp_frames_projective(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside /* or NULL */,
                                 int nframes, int width, int height, int noc, int border, void* stream);
/* ofdis_batch_stabilize without `model`: the composition, all enqueued on `stream`, of ofdis_batch_projective_motion(b,
 * first_frame, count, rounds, thresh, fb_check, alpha, beta, ...), ofdis_camera_path_projective on its models at width_org x
 * height_org and ofdis_warp_frames_projective on frames + first_frame frames -- bit-identical to those three calls made
 * separately, under both contracts.  warps = device [count+1][8] or NULL.  Models and warps live in an array of the context of
 * its own: allocated at the first call, counted by ofdis_batch_device_bytes from then on.  Joins a pipelined pass by itself.
 * OFDIS_ERR_INVALID as ofdis_batch_stabilize, each before any allocation or device work. */
int ofdis_batch_stabilize_projective(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int rounds,
                                     float thresh, int fb_check, float alpha, float beta, const double* weights /* host */,
                                     int radius, double zoom, int border, uint8_t* out, uint8_t* inside /* or NULL */,
                                     double* warps /* device [count+1][8] or NULL */, int width_org, int height_org,
                                     void* stream);

/* Warm start (the reference's `initflow`, oflow.cpp:217-220; e.g. the previous frame pair's flow of a video):
 * per frame (w >> (sc_f+1)) x (h >> (sc_f+1)) x 2 floats, AoS.  set_initflow borrows a device array
 * [nframes][ofdis_batch_initflow_elems] (NULL switches the warm start off again); upload_initflow copies one
 * frame's host array into a buffer owned by the batch (frames never uploaded start from zero flow). */
size_t ofdis_batch_initflow_elems(const ofdis_batch* b);
int ofdis_batch_set_initflow(ofdis_batch* b, const float* initflow_dev);
int ofdis_batch_upload_initflow(ofdis_batch* b, int frame, const float* initflow_host, void* stream);

/* enqueue the whole hot path (all levels, DIS + densify + TV) for all frames on `stream` */
int ofdis_batch_run(ofdis_batch* b, void* stream);
/* Throughput option: cut the batch into `sub_batches` (2..4; 0 or 1 = off, the default) parts that run on internal
 * streams forked from the caller's stream and NOT joined at the end of ofdis_batch_run, so that consecutive passes
 * overlap (coarse-level kernels of one part fill the issue slots left by another part's kernels).  Results are then
 * complete on a stream only after ofdis_batch_join(b, stream); ofdis_batch_download / _upsample join themselves.
 * Do not modify the inputs of a pass before joining it.  Results are identical in either mode. */
int ofdis_batch_set_pipeline(ofdis_batch* b, int sub_batches);
int ofdis_batch_join(ofdis_batch* b, void* stream);
/* Launch-graph replay: the schedule of a context never changes, so an un-pipelined ofdis_batch_run can replay it as one
 * hipGraph launch instead of ~15 kernel launches.  mode 0 = direct launches (the default: measured, the asynchronous
 * launches already overlap the execution and the replay is not faster), 1 = captured at the next pass, -1 = captured at
 * the second pass of the context.  Results are identical; timing mode, verbosity > 0 and pipelined mode always launch
 * directly. */
int ofdis_batch_set_graph(ofdis_batch* b, int mode);
/* device pointer to the result, [nframes][h>>sc_l][w>>sc_l][2] ([..][1] in stereo-depth mode); in pipelined mode valid on
 * a stream after ofdis_batch_join(b, stream) */
const float* ofdis_batch_flow(const ofdis_batch* b);
/* After the caller has synchronised the stream(s) of the context's last pass by its own means: OFDIS_OK, or
 * OFDIS_ERR_DEVICE when that pass's results are invalid.  The one kernel that can report this is the cross-CU variant of the
 * fused TV kernel (contexts of <= 768 frames; ofdis_tuning::fused_xcu_max): its workgroups hand rows to each other through
 * memory and wait, bounded (ofdis_tuning::fused_xcu_spin: 50 ms), for workgroups the dispatcher started earlier; a wait that
 * expires marks the pass as failed.
 * The failure stays with the context until its next ofdis_batch_run, which no longer uses the variant: run again.
 * ofdis_batch_download, ofdis_flow (which repeats the pass itself) and ofdis_sync on the stream of the pass report the same
 * condition; callers that synchronise through HIP directly call this. */
int ofdis_batch_status(ofdis_batch* b);
/* device pointer to the dense flow of an intermediate level (for per-level parity tests) */
const float* ofdis_batch_level_flow(const ofdis_batch* b, int level);
int ofdis_batch_download(ofdis_batch* b, int frame, float* outflow_host, void* stream);
/* The step after the path (run_dense.cpp:406-414): values x 2^sc_l, bilinear upsample by 2^sc_l (cv::resize
 * INTER_LINEAR semantics: half-pixel centres, clamped borders) and crop of the 2^sc_f padding, for all frames:
 * out_dev = device [nframes][height_org][width_org][2] ([..][1] in stereo-depth mode).  Enqueues on `stream`. */
int ofdis_batch_upsample(ofdis_batch* b, float* out_dev, int width_org, int height_org, void* stream);
/* The same for the frames [first_frame, first_frame + count) only: out_dev = device [count][height_org][width_org][2].
 * (A host driver that streams a long sequence through one context writes its .flo files chunk by chunk; bench.py takes
 * its sample of the timed context's result this way.) */
int ofdis_batch_upsample_frames(ofdis_batch* b, int first_frame, int count, float* out_dev, int width_org,
                                int height_org, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Compact output encodings.  The full-resolution fp32 result is four times the bytes most bulk consumers keep (fp16 in
 * memory, 16-bit fixed point in KITTI-style files, clipped 8-bit planes in two-stream datasets), and over a PCIe link the
 * download of that result is what bounds a host loop.  An encoding is applied per value v (each component of a flow vector
 * on its own); the output keeps the AoS order of the fp32 result, [..][2] or [..][1] in stereo-depth mode.  Every operation is
 * a separately rounded fp32 operation, independent of the arithmetic contract:
 *   OFDIS_ENC_F32  the bits of v unchanged (accepted everywhere, so that a caller has one code path)
 *   OFDIS_ENC_F16  IEEE binary16 of v, round to nearest even; gradual underflow (subnormal halves are produced, not flushed);
 *                  |v| >= 65520 gives +-inf; NaN gives some NaN.  scale and offset are ignored
 *   OFDIS_ENC_U16 (M = 65535), OFDIS_ENC_U8 (M = 255):
 *                  t = v * scale + offset   (two operations);  t = fminf(fmaxf(t, 0), M)   (IEEE: a NaN becomes 0);
 *                  q = (int)floorf(t + 0.5f)                   (a tie x.5 rounds up)
 *                  A consumer decodes v ~ (q - offset) / scale.  KITTI flow .png is {U16, 64, 32768}, KITTI disparity of the
 *                  left view {U16, -256, 0} (the left-view result is <= 0), the two-stream "bound 20" format {U8, 255/40, 127.5}
 * OFDIS_ERR_INVALID before any device work: a NULL encoding, an unknown type; for the integer types a scale that is zero or
 * not finite, an offset that is not finite.  of_dis_amd/encoding.py states the same arithmetic in numpy.
 * ------------------------------------------------------------------------------------------- */
enum { OFDIS_ENC_F32 = 0, OFDIS_ENC_F16 = 1, OFDIS_ENC_U16 = 2, OFDIS_ENC_U8 = 3 };
typedef struct ofdis_encoding {
  int   type;            /* OFDIS_ENC_* */
  float scale, offset;   /* integer types only */
} ofdis_encoding;
size_t ofdis_encoding_bytes(int type);   /* bytes per element: 4, 2, 2, 1; 0 for an unknown type */
/* Materialised: n fp32 values of the device array `src` into the device array `dst` (ofdis_encoding_bytes(type) bytes each).
 * Not in place: src == dst is OFDIS_ERR_INVALID, like NULL pointers.  16-byte loads and stores where both arrays are 16-byte
 * aligned (what ofdis_dev_alloc returns), element by element otherwise.  Enqueues on `stream`. */
int ofdis_encode(const float* src, void* dst, size_t n, const ofdis_encoding* enc, void* stream);
/* ofdis_batch_upsample_frames writing the encoded result directly: out = device [count][height_org][width_org][C] elements
 * (C = 2, or 1 in stereo-depth mode).  Bit-identical to ofdis_encode applied to what ofdis_batch_upsample_frames writes for
 * the same arguments, for both contracts and every kind of context (of an OFDIS_BATCH_REVERSE or OFDIS_BATCH_STEREO_LR
 * context: the forward result); the fp32 array is never written.  A lane encodes in registers and issues one 16-byte store per
 * output row where the rows' byte length and `out` are multiples of 16 bytes; other sizes take narrower stores, same bytes.
 * `out` is aligned to its element size; nothing outside it is written.  Joins a pipelined pass by itself.  Argument errors:
 * those of ofdis_batch_upsample_frames and of the encoding. */
int ofdis_batch_upsample_frames_enc(ofdis_batch* b, int first_frame, int count, void* out, int width_org, int height_org,
                                    const ofdis_encoding* enc, void* stream);

/* Kernel timing for the roofline report: when enabled, ofdis_batch_run brackets every launch of
 * the named kernel class with hipEvents on `stream`; ofdis_batch_kernel_time returns the summed
 * milliseconds and launch count since the last reset (synchronises the events). */
enum { OFDIS_K_WARP = 0, OFDIS_K_DERIV = 1, OFDIS_K_SYSTEM = 2, OFDIS_K_SOR = 3, OFDIS_K_PATCH = 4,
       OFDIS_K_DENSIFY = 5, OFDIS_K_UPDATE = 6, OFDIS_K_FUSED = 7, OFDIS_K_COUNT = 8 };
int ofdis_batch_timing(ofdis_batch* b, int enable);
int ofdis_batch_kernel_time(ofdis_batch* b, int kernel_class, double* ms_sum, long* launches);
/* the same launch by launch, in launch order (a pass launches a class once per level, coarsest level first): fills
 * ms_out[0 .. min(capacity, *launches) - 1] */
int ofdis_batch_kernel_times(ofdis_batch* b, int kernel_class, double* ms_out, int capacity, int* launches);

/* ---------------------------------------------------------------------------------------------
 * Kernel-selection knobs.  Several stages exist in more than one mapping of the SAME arithmetic (every setting but
 * `contract` gives bit-identical results); the library picks by geometry and batch size.  The knobs are process-wide, are initialised
 * ONCE from the environment variables named below at the first call into the library and can be changed at run time
 * (the parity tests run every mapping; a maintainer can pin one).  A change takes effect at the next ofdis_batch_run /
 * ofdis_flow, except fused_tv and contract, which a context fixes at creation (it allocates the scratch of the path it will take:
 * ofdis_flow_cache_clear() before ofdis_flow picks up a change).  A captured launch graph (ofdis_batch_set_graph) is
 * re-captured after a change.
 * ------------------------------------------------------------------------------------------- */
typedef struct ofdis_tuning {
  int gray8;          /* 1: gray 8x8 patches use the 4-lanes-per-patch kernel; 0: generic kernel     OFDIS_NO_GRAY8 -> 0 */
  int rgb12;          /* 1: RGB 12x12, gray 12x12 and RGB 8x8 patches (flow or stereo, cost function 0 / 1) use the
                       * 16-lanes-per-patch kernels / the compile-time instantiations; 0: generic kernel   OFDIS_NO_RGB12 -> 0 */
  int rgb12_lpp;      /* lanes per RGB 12x12 patch: 0 = the library's choice (16), 64 = one patch per wavefront, 32 = two,
                       * 16 = four (a 3x3 pixel block per lane for the taps; the exact contract moves the interpolated
                       * values through LDS into the entry order its documented summation needs, the fused contract sums
                       * block-wise)                                                                  OFDIS_RGB12_LPP */
  int fused_tv;       /* 1: gray levels of <= 256 rows and <= 256 columns take the fused TV path (warp + derivatives kernel,
                       * fused system + SOR kernel), RGB levels of <= 256 rows the fused system + SOR kernels (fused_rgb_min)
                       *                                                                              OFDIS_NO_FUSED -> 0 */
  int fused_mw_max;   /* frame groups up to which the multi-wave fused TV kernels are launched       OFDIS_FUSED_MW_MAX
                       * (default 512 and at most 1024 frames per batch; 0 = never; >= 2^30 = always) */
  int fused_split;    /* 1: multi-wave kernel with producer + solver wavefronts per iteration  OFDIS_FUSED_NO_SPLIT -> 0 */
  int finish_fusion;  /* 1: the multi-wave kernels write the refined flow themselves        OFDIS_NO_FINISH_FUSION -> 0 */
  int fused_strip;    /* frames per strip of the throughput fused TV kernel; 0 = chosen by the library  OFDIS_FUSED_STRIP */
  int prep_band_rows; /* output rows per wavefront of the warp + derivatives kernel; 0 = by batch size  OFDIS_PREP_BAND_ROWS */
  int graph;          /* 1: ofdis_batch_set_graph may replay a captured launch graph                 OFDIS_NO_GRAPH -> 0 */
  int flow_dma;       /* 1: ofdis_flow stages through hipMemcpyAsync instead of copy kernels               OFDIS_FLOW_DMA */
  int flow_whole;     /* 1: ofdis_flow uploads the whole pyramid before the first launch                OFDIS_FLOW_WHOLE */
  int fused_xcu_max;  /* frame groups up to which the fused TV kernel runs every fixed-point iteration of a group as its
                       * own workgroup on its own CU (contexts of <= 768 frames; 0 = never)        OFDIS_FUSED_XCU_MAX */
  int fused_tp_pipe;  /* large batches: the fused TV kernel with one wavefront per fixed-point iteration and strip (the
                       * iterations of a strip on one compute unit share the derivative records through the L2) instead of
                       * one wavefront per strip walking all iterations.  0 = never, 1 = where it is faster (gray levels of
                       * more than 32 rows under the fused contract; RGB levels of <= 64 rows under the fused contract in
                       * batches of up to 2048 frames), 2 = always                                  OFDIS_FUSED_TP_PIPE */
  int fused_xcu_spin; /* microseconds a workgroup of that variant waits for a hand-over row (device wall clock) before it
                       * reports the pass as failed and carries on without waiting; 0 = the default, 50 000 (50 ms: a
                       * thousand times the longest healthy wait, and the most a drop-in call can lose before its pass is
                       * repeated on the other mapping); 1 forces the failure                     OFDIS_FUSED_XCU_SPIN */
  int contract;       /* ARITHMETIC CONTRACT -- the one knob that changes bits.  0 = exact (default) and 1 = fused, both
                       * stated at the top of this file: exact is bit-identical to the reference build, fused the tolerance contract of the
                       * north star (flow within 1e-3 px of the reference): every kernel compiled a second time with
                       * multiply-adds contracted to v_fma_f32 and the hardware's 1-ulp reciprocal / square root in place
                       * of the correctly rounded ones -- same algorithm, same control flow, fewer instructions.  A context
                       * fixes it at creation, like fused_tv.                                OFDIS_CONTRACT=fused -> 1 */
  int fused_xcu_drop; /* TEST HOOK, 0 in production: 1 = the first fixed-point iteration of the cross-CU variant withholds its
                       * hand-over rows, so that the iteration behind it really waits out fused_xcu_spin (what a dispatcher
                       * that broke the variant's ordering assumption would cause): tests/test_gpu_xcu.py measures what
                       * the failure protocol costs at the DEFAULT bound with it                  OFDIS_FUSED_XCU_DROP */
  int prep_densify;   /* 1: on the fused TV path (gray 8x8 patches, step-4 grid) the warp + derivatives kernel densifies the
                       * flow from the patch results itself (PatGridClass::AggregateFlowDense inside tv_prep_kernel): no
                       * densification launch, no round trip of the dense flow; 0: separate kernel  OFDIS_NO_PREP_DENSIFY -> 0 */
  int fused_tall_group; /* levels of 65 ... 96 rows (the finest level of a 1080p / 4K gray pair is 120 x 68): 1 = the fused TV
                       * kernel takes up to three strips per workgroup, their rows beyond the 64th sharing ONE wavefront
                       * (2 .. 7: at most that many); 0 = two wavefronts per strip   OFDIS_TALL_GROUP, OFDIS_NO_TALL_GROUP -> 0 */
  int fused_rgb_min;  /* RGB levels of <= 256 rows (three derivative record arrays) and gray levels of > 256 columns and <= 256
                       * rows take the fused system + SOR kernels behind the TILED warp and derivatives kernels (the latter
                       * writing records; with fused_tv and finish_fusion) in contexts of at least this many frames: 0 = the
                       * library's choice (16 under the fused contract, 512 under the exact one: below it the
                       * one-launch-per-stage kernels are as fast or faster), 1 = always, 2^30 = never.  The stereo-depth
                       * mode's levels of <= 64 rows take their fused kernel (de_fused_kernel) by the same knob; its own
                       * defaults: always under the fused contract, from 256 frames under the exact one
                       *                                                                            OFDIS_FUSED_RGB_MIN */
  int patch_window_reuse; /* 1: the gray 8x8 patch kernel keeps the 9 x 3 tap window of an evaluation in registers and loads it
                       * again only when its integer position has moved (a converged search fetches the same bytes in every
                       * evaluation); 0: nine loads per lane in every evaluation.  Same values either way
                       *                                                            OFDIS_NO_PATCH_WINDOW_REUSE -> 0 */
} ofdis_tuning;
int ofdis_get_tuning(ofdis_tuning* out);
int ofdis_set_tuning(const ofdis_tuning* in);

/* ---------------------------------------------------------------------------------------------
 * Per-function entry points (device pointers, batched over `nframes` frames, packed planes
 * [nframes][h][w]).  Each replaces one FDF1.0.1 / PatGrid function; used by the parity tests and
 * available to a maintainer who wants to swap a single stage.
 * ------------------------------------------------------------------------------------------- */
/* image_warp, opticalflow_aux.c:18-60.  src/dst: [nframes][noc][h][w]; wx, wy, mask: [nframes][h][w] */
int ofdis_image_warp(float* dst, float* mask, const float* src, const float* wx, const float* wy,
                     int w, int h, int noc, int nframes, void* stream);
/* get_derivatives, opticalflow_aux.c:65-116.  out: [nframes][8][noc][h][w] in the order
 * Ix,Iy,Iz,Ixx,Ixy,Iyy,Ixz,Iyz */
int ofdis_get_derivatives(float* out, const float* im1, const float* im2w, int w, int h, int noc,
                          int nframes, void* stream);
/* compute_smoothness + compute_data + 2x sub_laplacian fused (opticalflow_aux.c:123-199,310-438):
 * out: [nframes][7][h][w] = a11,a12,a22,b1,b2,smooth_horiz,smooth_vert */
int ofdis_tv_system(float* out, const float* mask, const float* wx, const float* wy, const float* du,
                    const float* dv, const float* derivs, float tv_alpha, float tv_gamma, float tv_delta,
                    int w, int h, int noc, int nframes, void* stream);
/* sor_coupled, solver.c:77-421: `iterations` lexicographic block-SOR sweeps; du, dv in place.
 * sys: the [nframes][7][h][w] array of ofdis_tv_system (not modified; the reference's in-place
 * block inverse, solver.c:113-120, lives in registers). */
int ofdis_sor_coupled(float* du, float* dv, const float* sys, int iterations, float omega, int w, int h,
                      int nframes, void* stream);
/* one pyramid level of PatGridClass::{InitializeGrid,SetTargetImage,InitializeFromCoarserOF,
 * Optimize} + AggregateFlowDense (patchgrid.cpp:98-141,195-275,377-397).
 * im_*: [nframes][tmp_h][tmp_w][noc]; flow_prev: [nframes][h/2][w/2][2] or NULL;
 * p_out: [nframes][nopatches][2] or NULL; flow_out: [nframes][h][w][2] */
int ofdis_patchgrid_level(const ofdis_params* p, int level, const float* im_a, const float* im_a_dx,
                          const float* im_a_dy, const float* im_b, const float* flow_prev, float* p_out,
                          float* flow_out, int nframes, void* stream);
/* one pyramid level of VarRefClass (refine_variational.cpp:25-241); flow [nframes][h][w][2] in place */
int ofdis_varref_level(const ofdis_params* p, int level, const float* im_a, const float* im_b, float* flow,
                       int nframes, void* stream);

/* plain device memory helpers so that C callers need no HIP headers */
void* ofdis_dev_alloc(size_t bytes);
void ofdis_dev_free(void* p);
int ofdis_memcpy_h2d(void* dst, const void* src, size_t bytes);
int ofdis_memcpy_d2h(void* dst, const void* src, size_t bytes);
int ofdis_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
/* Waits for `stream` (NULL = the calling thread's current device's default stream).  Also reports -- once, as
 * OFDIS_ERR_DEVICE -- a lost hand-over of the cross-CU fused TV variant (ofdis_batch_status) of every context whose last
 * pass was enqueued on that stream; for the NULL stream, which exists once per device, only the contexts of the calling
 * thread's current device. */
int ofdis_sync(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Streams, pinned host memory and asynchronous copies (version 3): what a host loop needs to keep the link and the GPU
 * busy at the same time -- the reference's per-pair upload / download (run_dense.cpp:326-344 convertTo + pyramid on the
 * host, :406-421 resize + crop + .flo) becomes: pinned 8-bit frames -> ofdis_memcpy_h2d_async -> ofdis_batch_build_pyramids_u8
 * -> ofdis_batch_run -> ofdis_batch_upsample_frames -> ofdis_memcpy_d2h_async, all enqueued on ONE stream per slot, with
 * two or more slots (context + stream + buffers) in flight so that one slot's download overlaps the next slot's upload
 * and kernels (host/run_seq_main.cpp).  Several small passes in flight on several streams is also how a share of a few
 * dozen pairs per GPU (BASELINE configs[4] at 8 GPUs) keeps the chip busy: DESIGN.md 6, bench.py `small_batch.depth`.
 * ------------------------------------------------------------------------------------------- */
/* a non-blocking stream on the calling thread's current device; NULL on failure (ofdis_last_error) */
void* ofdis_stream_create(void);
void ofdis_stream_destroy(void* stream);
/* page-locked host memory, usable with every visible device (hipHostMallocPortable); NULL on failure */
void* ofdis_host_alloc(size_t bytes);
void ofdis_host_free(void* p);
/* enqueue a copy on `stream`; the host buffer must stay valid until the stream has been synchronised.  With memory from
 * ofdis_host_alloc the copy is a DMA that overlaps kernels and copies of other streams; with pageable memory it still
 * works, staged and partly synchronous, like hipMemcpyAsync */
int ofdis_memcpy_h2d_async(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int ofdis_memcpy_d2h_async(void* dst_host, const void* src_dev, size_t bytes, void* stream);
/* Events order work across streams without the host.  Why a host loop wants them: uploads share the link's one direction
 * and downloads the other, so the copies of consecutive chunks belong on ONE upload stream and ONE download stream (each
 * in order) beside the compute stream(s) -- two chunks that each run upload, kernels, download on a stream of their own fall
 * into lock step (both upload, then both download) and the two directions never overlap (tools/link_probe.py: 12.2 k
 * against 15 k pairs/s).  ofdis_event_record marks a point of `stream`; ofdis_stream_wait_event makes `stream` wait for
 * the last recorded point (a never-recorded event is complete); ofdis_event_sync blocks the host until it is reached. */
void* ofdis_event_create(void);
void ofdis_event_destroy(void* event);
int ofdis_event_record(void* event, void* stream);
int ofdis_stream_wait_event(void* stream, void* event);
int ofdis_event_sync(void* event);

#ifdef __cplusplus
}
#endif
#endif /* OFDIS_H_ */
