// ofdis_schedule.hip -- what one pass of a batch context launches: the plan of a level (its TV refinement route and every
// knob-dependent choice along it), the route bodies, the coarse-to-fine launch schedule of OFC::OFClass::OFClass
// (oflow.cpp:184-337) with its pipelined and graph-replayed forms, and the pass state of the cross-CU fused TV variant.
#include <sys/time.h>

#include "ofdis_context.h"

using namespace ofdis;

namespace ofdis {

static double now_ms() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return tv.tv_sec * 1000.0 + tv.tv_usec / 1000.0;
}

// Contexts of up to this many frames own the hand-over granule array of the cross-CU fused TV variant
constexpr int XCU_MAX_CONTEXT_FRAMES = 768;

// After a synchronisation that covers the context's last pass: OFDIS_ERR_DEVICE when that pass's results are invalid.
// The failure stays attached to the context until its next pass starts (xcu_begin_pass), which runs without the variant.
int xcu_poll(ofdis_batch* b) {
  XcuState* x = b ? b->xcu : nullptr;
  if (!x) return OFDIS_OK;
  if (*(volatile int*)x->host) {
    *(volatile int*)x->host = 0;
    x->failed = true;
    x->off = true;
    x->rezero = true;
  }
  if (x->failed)
    return fail(OFDIS_ERR_DEVICE, "fused TV kernel (cross-CU variant): a hand-over row never arrived; the results of this pass are "
                                  "invalid -- run the context again (it no longer uses the variant)");
  if (x->missed.exchange(false))  // said once: whoever consumed the earlier pass's results without asking learns it here
    return fail(OFDIS_ERR_DEVICE, "fused TV kernel (cross-CU variant): an EARLIER pass of this context lost a hand-over row and "
                                  "was never polled; its results were invalid (the pass since then ran without the variant)");
  return OFDIS_OK;
}
int xcu_begin_pass(ofdis_batch* b, hipStream_t s) {
  XcuState* x = b->xcu;
  if (!x) return OFDIS_OK;
  if (*(volatile int*)x->host) {  // a failure nobody has polled yet: the variant goes off all the same, and the failure
    (void)xcu_poll(b);            // stays latched (`missed`) until one synchronising route has reported it
    x->missed = true;
  }
  x->failed = false;
  x->told_sync = false;
  x->last_stream = s;
  {
    int dev = -1;
    (void)hipGetDevice(&dev);
    x->last_device = dev;
  }
  x->ran = true;
  if (x->rezero && b->xbuf) {  // stale tags of the pass that failed
    // (a previous pipelined pass leaves its sub-streams unjoined on purpose; they may still be using the granules)
    if (b->join_pending) {
      for (hipEvent_t ev : b->sub_done) HIPCHK(hipStreamWaitEvent(s, ev, 0));
      b->join_pending = false;
    }
    HIPCHK(hipMemsetAsync(b->xbuf, 0, frame_elems(*b, b->xbuf) * b->total_frames * sizeof(float), s));
    x->rezero = false;
  }
  return OFDIS_OK;
}

DisArgs dis_args(const ofdis_params& p, const LevelGeom& g, int nframes) {
  DisArgs a;
  memset(&a, 0, sizeof(a));
  a.g = g;
  a.nframes = nframes;
  a.max_iter = p.max_iter;
  a.min_iter = p.min_iter;
  a.costfct = p.costfct;
  a.patnorm = p.patnorm;
  a.dp_thresh_sq = p.dp_thresh * p.dp_thresh;  // oflow.cpp:88
  a.dr_thresh = p.dr_thresh;
  a.res_thresh = p.res_thresh;
  a.outlier_sq_max = outlier_sq_threshold((float)p.p_samp_s / 2);  // outlierthresh, oflow.cpp:82
  a.stereo = p.selectmode == 2;
  a.camlr = 0;  // the forward grid is the left camera (oflow.cpp:153-156)
  return a;
}

// Frames per strip of the throughput fused TV kernel.  A strip pays the fill / drain of the skewed sweep (h steps) once
// instead of once per frame, but its wavefront runs S times as long, and a launch of few, long wavefronts ends with idle
// SIMDs: measured at 16384 pairs (level 3, ms per 4096 pairs): S = 1 / 2 / 4 / 8 -> 2.30 / 2.18 / 2.21 / 2.24
// (profiles/README.md r03_b).  Rule: the largest S in {4, 2} that divides the frame count and leaves >= 4096 wavefronts in
// the launch, else 1; ofdis_tuning::fused_strip overrides.
// `pipe`: the iteration-pipelined mapping (a workgroup of n_inner wavefronts per strip group): every wavefront pays the
// fill / drain and the lag behind its predecessor per strip, so longer strips pay off more -- the largest S in {8, 4, 2}
// that leaves >= 1024 workgroups (two rounds of what the chip holds).
static int strip_length(const ofdis_batch& b, const LevelGeom& g, const ofdis_tuning& tn, bool pipe) {
  const int n = b.nframes;
  if (tn.fused_strip > 0) return (n % tn.fused_strip == 0) ? tn.fused_strip : 1;
  const int R = slot_rows(g.h);
  for (int S = pipe ? 8 : 4; S > 1; S >>= 1)
    if (n % S == 0 && (n / S) / (64 / R) >= (pipe ? 1024 : 4096)) return S;
  return 1;
}

// The one-launch route a level's geometry and the context's parameters allow, whatever the knobs and the scratch say
// (PerStage / StereoPerStage: none).  The scratch sizing at creation and the plan of every pass both start from it.
static Route fusable_route(const ofdis_params& p, const Launchers& K, const LevelGeom& g, int nframes) {
  const TvConsts c = tv_consts(p.tv_alpha, p.tv_gamma, p.tv_delta);
  const TvGeom t{g.w, g.h, g.noc, nframes};
  const int n_inner = p.tv_innerit * (g.level + 1);  // :36
  const bool params_ok = K.tv_fused_params_ok(c.quarter_alpha, c.half_delta_over3, c.half_gamma_over3);
  if (p.selectmode == 2)
    return params_ok && n_inner >= 1 && K.de_fused_supported(t, p.tv_solverit) ? Route::StereoFused : Route::StereoPerStage;
  if (!params_ok || !K.tv_fused_supported(t, p.tv_solverit)) return Route::PerStage;
  if (K.tv_prep_supported(t)) return Route::GrayFused;  // (gray only)
  return g.h >= 4 && n_inner >= 1 ? Route::Records : Route::PerStage;
}

Scratch size_scratch(const ofdis_batch& b, const ofdis_tuning& tn) {
  const ofdis_params& p = b.p;
  const LevelGeom& g0 = b.geom[0];  // finest level: largest of everything
  Scratch sc;
  // compact per-pixel weights: only the 16-lane RGB 12x12 patch kernels write them (forward-backward merging reads the weights
  // by another shifted rule) -- other geometries do not pay.  Sized for any knob setting that may pick those kernels later.
  ofdis_tuning rgb16 = tn;
  rgb16.rgb12 = 1;
  rgb16.rgb12_lpp = 16;
  sc.pixw = !p.usefbcon && b.k->patch_pixel_weights_supported(dis_args(p, g0, b.nframes), &rgb16);
  // TV scratch.  The per-stage planes (13 of the 25 floats per pixel: a third of the context) only when some level can take a
  // route that reads them; records for the levels that can take a one-launch route; the cross-CU variant's {du, tag, dv, tag}
  // per pixel and iteration boundary (ofdis_fused_xcu.hip) only while the knob is on, for contexts of at most
  // XCU_MAX_CONTEXT_FRAMES frames: 16 B x (n_inner - 1) per pixel of the largest gray fused level that can take the variant
  // (>= 2 fixed-point iterations; levels of more than 64 rows never do: two wavefronts per strip, ofdis_fused_tall.hip),
  // 344 KB per frame at operating point 2
  const bool xcu = tn.fused_tv && b.nframes <= XCU_MAX_CONTEXT_FRAMES && tn.fused_xcu_max > 0;
  bool all_gray_fused = true;
  size_t fused_px = 0;
  for (const LevelGeom& g : b.geom) {
    const Route r = fusable_route(p, *b.k, g, b.nframes);
    const size_t px = (size_t)g.w * g.h, n_inner = (size_t)std::max(1, p.tv_innerit * (g.level + 1));
    all_gray_fused = all_gray_fused && r == Route::GrayFused;
    if (r == Route::GrayFused || r == Route::Records || r == Route::StereoFused) fused_px = std::max(fused_px, px);
    if (xcu && r == Route::GrayFused && n_inner >= 2 && g.h <= 64)
      sc.xbuf_per_frame = std::max(sc.xbuf_per_frame, (n_inner - 1) * px * 4);
  }
  sc.planes = !(tn.fused_tv && all_gray_fused);
  if (tn.fused_tv && fused_px) {  // gray: the finest level's size, RGB and stereo: the largest level that can fuse
    sc.rec_px = (p.noc == 1 && p.selectmode != 2) ? (size_t)g0.w * g0.h : fused_px;
    sc.uv = p.selectmode != 2;
  }
  return sc;
}

static FusedArgs fused_args(const ofdis_batch& b, const LevelGeom& g, const LevelPlan& pl, float* flow_out) {
  const ofdis_params& p = b.p;
  const TvConsts c = tv_consts(p.tv_alpha, p.tv_gamma, p.tv_delta);
  FusedArgs fa{TvGeom{g.w, g.h, g.noc, b.nframes}, b.derivs, b.wrec, b.uv, pl.S, c.quarter_alpha, c.half_delta_over3,
               c.half_gamma_over3, p.tv_solverit, p.tv_sor, p.tv_innerit * (g.level + 1), b.total_frames,
               pl.fused_writes_flow ? flow_out : nullptr, pl.mw_max_groups, pl.split, pl.tp_pipe};
  fa.tall_group = pl.tall_group;
  return fa;
}

// The fused TV path BY RECORDS (round 6).  RGB levels of at most 256 rows (one wavefront per frame up to 64 rows, two to four
// beyond): the unfused path's tiled warp kernel, the derivatives kernel in its record form and the fused system + SOR
// kernel with three derivative record arrays -- every fixed-point iteration of the level in one launch
// instead of n_inner x (tv_system + SOR), the derivative records read once per iteration instead of planes + system planes.
// One wavefront walks a frame's n_inner * w + h steps whatever the batch: measured at 1024x436, operating point 2 (ms per
// step, fused / per-stage kernels): 1 pair 0.91 / 0.90, 16 pairs 0.93 / 0.97, 256 pairs 1.33 / 1.58, 1024 pairs 3.08-3.23 /
// 3.90, 4096 pairs 11.4-11.6 / 14.5 under the FUSED contract; under the EXACT contract its steps are half as long again
// (1.33 instead of 0.81 ms per pass whatever the batch): 16 pairs 1.47 / 1.11, 64 pairs 1.53 / 1.20, 256 pairs 1.87 / 1.71,
// 512 pairs 2.34 / 2.45, 1024 pairs 3.4 / 3.9 -- so contexts of fewer than 16 (fused contract) / 512 (exact contract) frames
// keep the per-stage kernels (ofdis_tuning::fused_rgb_min).
// Gray levels the row-marching warp + derivatives kernel does not take (more than 256 columns: the finest level of operating
// points 3 / 4) but the fused system + SOR kernels do (<= 256 rows) go the same way.
// Needs the unfused scratch (wx, wy, mask, w_im2) AND the record arrays.
constexpr int FUSED_RGB_MIN_FRAMES = 16, FUSED_RGB_MIN_FRAMES_EXACT = 512;
// Stereo levels of at most 64 rows: every fixed-point iteration in ONE launch of de_fused_kernel, fed by the derivatives
// kernel's record form.  Measured at 1242x375, operating point 2 (ms per step, fused kernel / per-stage kernels): fused
// contract 1 pair 0.58 / 0.69, 64 pairs 0.63 / 0.75, 1024 pairs 1.40 / 1.84, 4096 pairs 4.04 / 5.94 -- always; exact contract
// 1 pair 0.76 / 0.72, 64 pairs 0.80 / 0.78, 256 pairs 0.93 / 0.95, 1024 pairs 1.65 / 2.04, 4096 pairs 4.37 / 6.08 -- from 256
// frames on (ofdis_tuning::fused_rgb_min overrides both).
constexpr int FUSED_DE_MIN_FRAMES = 1, FUSED_DE_MIN_FRAMES_EXACT = 256;

// The plan of level `g` of context `b` (a frame view: its own nframes, its parent's total_frames) under the snapshot `tn`.
LevelPlan plan_level(const ofdis_batch& b, const LevelGeom& g, const ofdis_tuning& tn) {
  const ofdis_params& p = b.p;
  const Launchers& K = *b.k;
  LevelPlan pl;
  // RGB 12x12 without forward-backward merging: the patches the densification reads unshifted store one float per pixel (the
  // denominator of its weight) instead of three |r|
  pl.pixw = b.pixw && !p.usefbcon && K.patch_pixel_weights_supported(dis_args(p, g, b.nframes), &tn);
  if (!p.usetvref) return pl;
  const Route can = fusable_route(p, K, g, b.nframes);
  const int n_inner = p.tv_innerit * (g.level + 1);
  const int total = b.total_frames > 0 ? b.total_frames : b.nframes;
  const size_t px = (size_t)g.w * g.h;
  if (p.selectmode == 2) {
    const int min_frames = tn.fused_rgb_min > 0 ? tn.fused_rgb_min : (b.contract == 1 ? FUSED_DE_MIN_FRAMES : FUSED_DE_MIN_FRAMES_EXACT);
    const bool fz = can == Route::StereoFused && b.wrec && tn.fused_tv && px <= b.rec_px && total >= min_frames;
    pl.route = fz ? Route::StereoFused : Route::StereoPerStage;
    return pl;
  }
  // (a context created with every level on the gray fused route owns no per-stage scratch: b.wx == nullptr keeps it there)
  if (can == Route::GrayFused && b.wrec && (tn.fused_tv || !b.wx)) {
    if (n_inner <= 0) return pl;  // du = dv = 0: the densified flow is the refined one
    pl.route = Route::GrayFused;
    // The densification inside tv_prep needs: a fused kernel that writes the refined flow itself (nobody else then reads the
    // densified flow: tv_finish_records would), the geometry of the quad densification, no forward-backward merging, and the
    // context's own patch results (ofdis_varref_level has none: its flow comes densified).
    pl.dens_in_prep = b.pvec && tn.prep_densify && tn.finish_fusion && !p.usefbcon && K.tv_prep_densifies(g);
    pl.prep_band_rows = tn.prep_band_rows;
    pl.mw_max_groups = tn.fused_mw_max;
    pl.split = tn.fused_split;
    pl.tall_group = tn.fused_tall_group;
    pl.fused_writes_flow = tn.finish_fusion;
    // (no error word, or a context that has seen a lost hand-over: never the cross-CU variant)
    const bool xcu_ok = b.xbuf && b.xcu && !b.xcu->off;
    pl.fx = FusedXcu{xcu_ok ? b.xbuf : nullptr, xcu_ok ? tn.fused_xcu_max : 0, xcu_ok ? b.xcu->dev : nullptr,
                     tn.fused_xcu_spin > 0 ? (unsigned)tn.fused_xcu_spin : 0u, tn.fused_xcu_drop};
    FusedArgs fa = fused_args(b, g, pl, nullptr);
    if (K.tv_fused_mode(fa, &pl.fx) == 0) {  // not the small-batch regime: strips, on one of the two throughput mappings
      // which of the two: measured per 16384 pairs (profiles/README.md round 4), levels 3 / 4 / 5 of operating point 2:
      //   fused contract  one wavefront per strip 5.47 / 1.75 / 0.44 ms (HBM-bound: 56 B per pixel and iteration),
      //                   a wavefront per iteration, S = 8: 4.41 / 2.04 / 0.57 (issue-bound, 1/5 of the traffic)
      //   exact contract  9.06 against 11.9 ms in total (370 instead of 220 instructions per step: issue-bound either way,
      //                   and the pipelined form executes more wavefront-steps)
      // so: levels of more than 32 rows (one strip per wavefront) under the fused contract; fused_tp_pipe = 2 forces it
      pl.tp_pipe = fa.tp_pipe = tn.fused_tp_pipe >= 2 || (tn.fused_tp_pipe == 1 && b.contract == 1 && g.h > 32);
      pl.S = strip_length(b, g, tn, K.tv_fused_mode(fa, &pl.fx) == 1);
    }
    return pl;
  }
  const int min_frames = tn.fused_rgb_min > 0 ? tn.fused_rgb_min : (b.contract == 1 ? FUSED_RGB_MIN_FRAMES : FUSED_RGB_MIN_FRAMES_EXACT);
  if (can == Route::Records && b.wrec && b.uv && b.wx && b.mask && b.w_im2 && tn.fused_tv && tn.finish_fusion &&
      px <= b.rec_px && total >= min_frames) {
    pl.route = Route::Records;
    pl.tall_group = tn.fused_tall_group;
    // RGB levels of <= 64 rows: a wavefront per fixed-point iteration (the iteration-pipelined mapping) instead of one per
    // frame while the batch leaves SIMDs idle -- measured under the fused contract at 1024x436, operating point 2, k frames/s:
    // 256 pairs 193 -> 247, 1024 pairs 318-324 -> 359, 4096 pairs 351-361 -> 350; under the exact contract it is slower
    // (1024 pairs: 293 -> 271: more instructions per pixel and iteration, as for gray) -- fused_tp_pipe = 2 forces it
    if (g.noc == 3 && g.h <= 64)
      pl.tp_pipe = tn.fused_tp_pipe >= 2 || (tn.fused_tp_pipe == 1 && b.contract == 1 && total <= 2048);
    return pl;
  }
  pl.route = Route::PerStage;
  return pl;
}

// image_warp + get_derivatives (refine_variational.cpp:189-190) by the per-stage kernels from the planes wx, wy: derivative
// planes out, or -- `records` -- the records the one-launch kernels walk
static int warp_derivatives(ofdis_batch* b, const LevelGeom& g, const float* im_a, const float* im_b, bool records, hipStream_t s) {
  const Launchers& K = *b->k;
  const TvGeom t{g.w, g.h, g.noc, b->nframes};
  {
    KTimer kt(b, OFDIS_K_WARP, s);
    WarpArgs wa{t, im_b, 1, g.pad, g.tmp_w, g.tmp_h, b->wx, b->wy, b->w_im2, b->mask};
    HIPCHK(K.warp(wa, s));
  }
  KTimer kt(b, OFDIS_K_DERIV, s);
  DerivArgs da{t, im_a, 1, g.pad, g.tmp_w, g.tmp_h, b->w_im2, b->derivs};
  if (records) {
    da.rec_d8 = b->derivs; da.rec_w = b->wrec; da.mask = b->mask; da.wx = b->wx; da.wy = b->wy;
  }
  HIPCHK(K.derivatives(da, s));
  return OFDIS_OK;
}

// GrayFused: `flow` (AoS) holds the densified flow on entry -- unless the plan densifies inside tv_prep -- and the refined one
// on return
static int tv_gray_fused(ofdis_batch* b, const LevelGeom& g, const LevelPlan& pl, const float* im_a, const float* im_b, float* flow,
                  hipStream_t s) {
  const Launchers& K = *b->k;
  const FusedArgs fa = fused_args(*b, g, pl, flow);
  {  // image_warp + get_derivatives (refine_variational.cpp:189-190): one kernel, records out
    KTimer kt(b, OFDIS_K_DERIV, s);
    PrepArgs pa{fa.t, im_a, im_b, g.pad, g.tmp_w, g.tmp_h, flow, b->derivs, b->wrec, pl.S, pl.prep_band_rows};
    if (pl.dens_in_prep) {  // AggregateFlowDense inside this kernel: patch results in, the dense flow never reaches memory
      pa.dens_p = b->pvec; pa.dens_pweight = b->pweight;
      pa.dens_nopw = g.nopw; pa.dens_noph = g.noph; pa.dens_offw = g.offw; pa.dens_offh = g.offh;
    }
    HIPCHK(K.tv_prep(pa, s));
  }
  bool flow_written = false;  // the multi-wave variants of the fused kernel write the refined AoS flow themselves
  {  // every fixed-point iteration of this level in one launch (du = dv = 0 on its first pass: no memset)
    KTimer kt(b, OFDIS_K_FUSED, s);
    HIPCHK(K.tv_fused(fa, s, &flow_written, &pl.fx));
  }
  if (!flow_written) {
    KTimer kt(b, OFDIS_K_UPDATE, s);
    HIPCHK(K.tv_finish_records(fa.t, flow, b->uv, pl.S, s));
  }
  return OFDIS_OK;
}

// Records: wx / wy hold the dense flow (planar, row-major) on entry; every fixed-point iteration in one launch, which writes
// the refined AoS flow itself
static int tv_records(ofdis_batch* b, const LevelGeom& g, const LevelPlan& pl, const float* im_a, const float* im_b, float* flow,
               hipStream_t s) {
  if (int rc = warp_derivatives(b, g, im_a, im_b, true, s)) return rc;
  bool flow_written = false;
  {
    KTimer kt(b, OFDIS_K_FUSED, s);
    HIPCHK(b->k->tv_fused(fused_args(*b, g, pl, flow), s, &flow_written, nullptr));
  }
  if (!flow_written) return fail(OFDIS_ERR_DEVICE, "the RGB fused TV kernel did not write the flow");
  return OFDIS_OK;
}

// PerStage: wx / wy hold the dense flow on entry, the refined AoS flow goes to `flow`
static int tv_per_stage(ofdis_batch* b, const LevelGeom& g, const float* im_a, const float* im_b, float* flow, hipStream_t s) {
  const ofdis_params& p = b->p;
  const Launchers& K = *b->k;
  const TvGeom t{g.w, g.h, g.noc, b->nframes};
  const size_t npx = (size_t)g.w * g.h;
  const int n_inner = p.tv_innerit * (g.level + 1);
  const TvConsts c = tv_consts(p.tv_alpha, p.tv_gamma, p.tv_delta);
  if (int rc = warp_derivatives(b, g, im_a, im_b, false, s)) return rc;
  HIPCHK(hipMemsetAsync(b->du, 0, npx * b->nframes * sizeof(float), s));  // image_erase :186-187
  HIPCHK(hipMemsetAsync(b->dv, 0, npx * b->nframes * sizeof(float), s));
  for (int it = 0; it < n_inner; ++it) {
    {
      KTimer kt(b, OFDIS_K_SYSTEM, s);
      SystemArgs sa{t, b->mask, b->wx, b->wy, b->du, b->dv, b->derivs, c.quarter_alpha, c.half_delta_over3,
                    c.half_gamma_over3, b->sys};
      HIPCHK(K.tv_system(sa, s));
    }
    {
      KTimer kt(b, OFDIS_K_SOR, s);
      SorArgs so{t, b->sys, b->du, b->dv, p.tv_solverit, p.tv_sor};
      HIPCHK(K.sor(so, s));
    }
  }
  KTimer kt(b, OFDIS_K_UPDATE, s);
  HIPCHK(K.tv_finish(t, b->wx, b->wy, b->du, b->dv, flow, s));
  return OFDIS_OK;
}

// VarRefClass::RefLevelDE (refine_variational.cpp:245-336), stereo-depth mode: b->wx holds the densified horizontal
// displacement (row-major), b->wy zeros; the refined plane goes to `flow` ([B][h][w], one channel).  StereoFused: every
// fixed-point iteration in one launch (du is never read during the first iteration and every pixel of it is written by every
// iteration).
static int de_fused(ofdis_batch* b, const LevelGeom& g, const float* im_a, const float* im_b, float* flow, int camlr, hipStream_t s) {
  const ofdis_params& p = b->p;
  const Launchers& K = *b->k;
  const TvGeom t{g.w, g.h, g.noc, b->nframes};
  const TvConsts c = tv_consts(p.tv_alpha, p.tv_gamma, p.tv_delta);
  if (int rc = warp_derivatives(b, g, im_a, im_b, true, s)) return rc;
  {
    KTimer kt(b, OFDIS_K_FUSED, s);
    DeFusedArgs fa{t, b->derivs, b->wrec, b->du, c.quarter_alpha, c.half_delta_over3, c.half_gamma_over3, p.tv_solverit,
                   p.tv_sor, p.tv_innerit * (g.level + 1), camlr};
    HIPCHK(K.de_fused(fa, s));
  }
  KTimer kt(b, OFDIS_K_UPDATE, s);
  HIPCHK(K.de_update(t, b->wx, b->du, nullptr, flow, camlr, s));  // wx = uu (:318)
  return OFDIS_OK;
}
static int de_per_stage(ofdis_batch* b, const LevelGeom& g, const float* im_a, const float* im_b, float* flow, int camlr,
                 hipStream_t s) {
  const ofdis_params& p = b->p;
  const Launchers& K = *b->k;
  const TvGeom t{g.w, g.h, g.noc, b->nframes};
  const size_t n = (size_t)g.w * g.h * b->nframes;
  const int n_inner = p.tv_innerit * (g.level + 1);
  const TvConsts c = tv_consts(p.tv_alpha, p.tv_gamma, p.tv_delta);
  if (int rc = warp_derivatives(b, g, im_a, im_b, false, s)) return rc;
  HIPCHK(hipMemsetAsync(b->du, 0, n * sizeof(float), s));                                    // image_erase(du)
  if (n_inner <= 0) {
    HIPCHK(hipMemcpyAsync(flow, b->wx, n * sizeof(float), hipMemcpyDeviceToDevice, s));  // uu = wx (:283), wx = uu (:318)
    return OFDIS_OK;
  }
  for (int it = 0; it < n_inner; ++it) {
    {
      KTimer kt(b, OFDIS_K_SYSTEM, s);
      // uu = wx before the first solve (:283), min / max (wx + du, 0) by camera side after it (:299-316): formed by the kernel
      DeSystemArgs sa{t, b->mask, b->wx, b->du, it == 0 ? -1 : camlr, b->derivs, c.quarter_alpha, c.half_delta_over3,
                      c.half_gamma_over3, b->sys};
      HIPCHK(K.de_system(sa, s));
    }
    {
      KTimer kt(b, OFDIS_K_SOR, s);
      DeSorArgs so{t, b->sys, b->du, p.tv_solverit, p.tv_sor};
      HIPCHK(K.de_sor(so, s));
    }
  }
  KTimer kt(b, OFDIS_K_UPDATE, s);
  HIPCHK(K.de_update(t, b->wx, b->du, nullptr, flow, camlr, s));  // wx = uu (:318)
  return OFDIS_OK;
}

// VarRefClass for one level, all frames, on the plan's route.  On entry the densified flow is where pl.planar() says (the
// planes wx / wy, or `flow` itself); the refined flow is in `flow` on return.  camlr: the camera side of a stereo level.
int refine_level(ofdis_batch* b, const LevelGeom& g, const LevelPlan& pl, const float* im_a, const float* im_b, float* flow,
                 hipStream_t s, int camlr) {
  switch (pl.route) {
    case Route::None: return OFDIS_OK;
    case Route::GrayFused: return tv_gray_fused(b, g, pl, im_a, im_b, flow, s);
    case Route::Records: return tv_records(b, g, pl, im_a, im_b, flow, s);
    case Route::PerStage: return tv_per_stage(b, g, im_a, im_b, flow, s);
    case Route::StereoFused: return de_fused(b, g, im_a, im_b, flow, camlr, s);
    case Route::StereoPerStage: return de_per_stage(b, g, im_a, im_b, flow, camlr, s);
  }
  return OFDIS_OK;
}

// The second direction of a context, described by a plane set and a result set:
//   OFDIS_BATCH_REVERSE    planes: A's and B's exchanged; results: flow_rev, from the reverse warm start
//   OFDIS_BATCH_STEREO_LR  planes: the mirrored, swapped pair's own (in_mir); results: flow_rev, never warm-started
//                          (initflow_rev stays null on such a context)
// Everything else -- frame count, scratch, contract, kernel selection, the level plan -- stays, so the pass computes what a
// plain context computes for that pair.  Done in place (applying it twice restores the context), so that kernel timing records
// both directions.
static bool has_second_direction(const ofdis_batch& b) { return b.reverse || b.stereo_lr; }
static void swap_direction(ofdis_batch* b) {
  if (b->stereo_lr)
    for (int k = 0; k < 6; ++k) std::swap(b->in[k], b->in_mir[k]);
  else
    for (int k = 0; k < 3; ++k) std::swap(b->in[k], b->in[3 + k]);
  std::swap(b->flow, b->flow_rev);
  std::swap(b->initflow, b->initflow_rev);
}

// one pyramid level of the loop (the body of oflow.cpp:184-337)
int run_one_level(ofdis_batch* b, int sl, hipStream_t s) {
  const ofdis_params& p = b->p;
  const int verbose = p.verbosity;
  const int ii = sl - p.sc_l;
  const LevelGeom& g = b->geom[ii];
  double tt[5] = {0, 0, 0, 0, 0};
  double t0 = 0;
  if (verbose > 1) { (void)hipStreamSynchronize(s); t0 = now_ms(); }
  // steps 1-3: patch grid construction, initialisation from the coarser flow and the inverse
  // search run as ONE kernel (pconst/pinit are reported as 0, poptim carries the time)
  const bool fb = p.usefbcon != 0;
  const bool bw_flow = fb && sl > p.sc_l;  // the backward flow is not needed at the last scale (oflow.cpp:269,291)
  const ofdis_tuning tn = tuning();  // ONE snapshot per level (another thread may change the knobs between the stages)
  const LevelPlan pl = plan_level(*b, g, tn);
  {
    KTimer kt(b, OFDIS_K_PATCH, s);
    DisArgs a = dis_args(p, g, b->nframes);
    a.im_a = b->in[0][ii];
    a.im_a_dx = b->in[1][ii];
    a.im_a_dy = b->in[2][ii];
    a.im_b = b->in[3][ii];
    a.flow_prev = (sl < p.sc_f) ? b->flow[ii + 1] : b->initflow;  // oflow.cpp:209-220
    a.p_out = b->pvec;
    a.pweight = b->pweight;
    a.pixw = pl.pixw ? b->pixw : nullptr;
    HIPCHK(b->k->patch_optimize(a, s, &tn));
    a.pixw = nullptr;
    if (fb) {  // the backward grid: images swapped (oflow.cpp:193-197,214-215,234-235)
      a.im_a = b->in[3][ii];
      a.im_a_dx = b->in[4][ii];
      a.im_a_dy = b->in[5][ii];
      a.im_b = b->in[0][ii];
      a.flow_prev = (sl < p.sc_f) ? b->flow_bw[ii + 1] : nullptr;
      a.p_out = b->pvec_bw;
      a.pweight = b->pweight_bw;
      a.camlr = 1;  // the backward grid is the right camera: displacement >= 0 (oflow.cpp:155-156, patch.cpp:191-192)
      HIPCHK(b->k->patch_optimize(a, s, &tn));
    }
  }
  if (verbose > 1) { (void)hipStreamSynchronize(s); tt[2] = now_ms() - t0; t0 = now_ms(); }
  // step 4: densification (with usefbcon each direction also merges the other grid's negated flow).
  // (Doing it inside the warp kernel -- one launch and one flow round trip less -- was measured: same time, 2.4x
  // the HBM traffic because a 32x32 pixel tile re-fetches the weight lines of the patches it shares with its
  // neighbours; not kept.)
  for (int dir = 0; dir < (bw_flow ? 2 : 1); ++dir) {
    if (pl.dens_in_prep) break;  // (never with usefbcon) the warp + derivatives kernel densifies from p / pweight itself
    DensifyArgs d;
    memset(&d, 0, sizeof(d));
    d.g = g;
    d.nframes = b->nframes;
    d.p = dir ? b->pvec_bw : b->pvec;
    d.pweight = dir ? b->pweight_bw : b->pweight;
    d.pixw = (pl.pixw && !dir) ? b->pixw : nullptr;
    d.stereo = p.selectmode == 2;
    if (fb) {
      d.cg_p = dir ? b->pvec : b->pvec_bw;
      d.cg_pweight = dir ? b->pweight : b->pweight_bw;
    }
    if (dir == 0 && pl.planar()) {  // (the gray fused route refines the AoS flow in place)
      d.wx = b->wx;
      d.wy = b->wy;
    } else {  // (the backward flow is parked as AoS until the forward refinement has used the planes)
      d.flow_aos = dir ? b->flow_bw[ii] : b->flow[ii];
    }
    KTimer kt(b, OFDIS_K_DENSIFY, s);
    HIPCHK(b->k->densify(d, s));
  }
  if (verbose > 1) { (void)hipStreamSynchronize(s); tt[3] = now_ms() - t0; t0 = now_ms(); }
  // step 5: variational refinement
  if (int rc = refine_level(b, g, pl, b->in[0][ii], b->in[3][ii], b->flow[ii], s)) return rc;
  if (bw_flow && pl.route != Route::None) {  // VarRefClass on the swapped pair (oflow.cpp:291-294), the right camera
    // (its densified flow waits in flow_bw: two channels, AoS; stereo: one)
    const size_t n = (size_t)g.w * g.h * b->nframes;
    if (p.selectmode == 2) {
      HIPCHK(hipMemcpyAsync(b->wx, b->flow_bw[ii], n * sizeof(float), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemsetAsync(b->wy, 0, n * sizeof(float), s));
    } else if (pl.planar()) {
      HIPCHK(b->k->flow_split(TvGeom{g.w, g.h, g.noc, b->nframes}, b->flow_bw[ii], b->wx, b->wy, s));
    }
    if (int rc = refine_level(b, g, pl, b->in[3][ii], b->in[0][ii], b->flow_bw[ii], s, 1)) return rc;
  }
  if (verbose > 1) {
    (void)hipStreamSynchronize(s);
    tt[4] = now_ms() - t0;
    printf("TIME (Sc: %i, #p:%6i, pconst, pinit, poptim, cflow, tvopt, total): %8.2f %8.2f %8.2f %8.2f %8.2f -> %8.2f ms.\n",
           sl, g.nop, tt[0], tt[1], tt[2], tt[3], tt[4], tt[0] + tt[1] + tt[2] + tt[3] + tt[4]);
  }
  return OFDIS_OK;
}

// The coarse-to-fine loop of OFClass::OFClass (oflow.cpp:184-337), every stage batched over frames.
static int run_levels(ofdis_batch* b, hipStream_t s) {
  const ofdis_params& p = b->p;
  const int verbose = p.verbosity;
  double t_all0 = 0;
  if (verbose > 0) {
    (void)hipStreamSynchronize(s);
    t_all0 = now_ms();
  }
  if (verbose > 1) printf("TIME (Grid Memo. Alloc. ) (ms): %3g\n", 0.0);  // buffers live in the batch context
  for (int sl = p.sc_f; sl >= p.sc_l; --sl)
    if (int rc = run_one_level(b, sl, s)) return rc;
  if (has_second_direction(*b)) {  // the same levels on the second direction's pairs, one direction after the other on `s`
    swap_direction(b);
    int rc = OFDIS_OK;
    for (int sl = p.sc_f; sl >= p.sc_l && !rc; --sl) rc = run_one_level(b, sl, s);
    swap_direction(b);
    if (rc) return rc;
  }
  if (verbose > 0) {
    (void)hipStreamSynchronize(s);
    printf("TIME (O.Flow Run-Time   ) (ms): %3g\n", now_ms() - t_all0);
    fflush(stdout);
  }
  return OFDIS_OK;
}

// The launch schedule of a context is fixed (same kernels, same pointers every pass), so it can be replayed as ONE
// hipGraph launch instead of ~15 kernel launches (ofdis_batch_set_graph).  Measured on this stack it buys nothing: the
// direct launches are asynchronous and overlap the execution of the first kernels (64 pairs per pass: 0.491 ms replayed,
// 0.486 ms direct; one pair: 0.459 both), so the default is off.  Never used when timing or TIME lines are requested
// (they synchronise between stages), in pipelined mode (the sub-batches are deliberately not joined), with
// OFDIS_NO_GRAPH, or after a capture failure -- the direct launches are always the fallback.
static int run_graph_or_levels(ofdis_batch* b, hipStream_t s) {
  unsigned epoch = 0;
  const bool env_off = !tuning(&epoch).graph;
  const bool want = b->graph_mode != 0 && !env_off && !b->timing && b->p.verbosity == 0 && (b->graph_mode == 1 || b->runs >= 1);
  b->runs++;
  if (!want) return run_levels(b, s);
  // the kernel selection is baked into the capture: the knobs (epoch), the warm-start pointer, and -- per context -- whether
  // the cross-CU fused TV variant is still allowed (a context that has seen a lost hand-over must not replay a graph that
  // still contains tv_fused_xcu_kernel: "run again" has to run the other kernel)
  const bool xcu_off = b->xcu && b->xcu->off;
  if (b->graph_exec && (b->graph_initflow != b->initflow || b->graph_initflow_rev != b->initflow_rev || b->graph_epoch != epoch ||
                        b->graph_xcu_off != xcu_off)) {
    (void)hipGraphExecDestroy(b->graph_exec);
    b->graph_exec = nullptr;
  }
  if (!b->graph_exec) {
    if (!b->cap_stream && hipStreamCreateWithFlags(&b->cap_stream, hipStreamNonBlocking) != hipSuccess) {
      b->graph_mode = 0;
      return run_levels(b, s);
    }
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(b->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const int rc = run_levels(b, b->cap_stream);
      const hipError_t e = hipStreamEndCapture(b->cap_stream, &g);
      ok = rc == OFDIS_OK && e == hipSuccess && g != nullptr;
    }
    if (ok) ok = hipGraphInstantiate(&b->graph_exec, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok) {
      (void)hipGetLastError();
      b->graph_exec = nullptr;
      b->graph_mode = 0;
      return run_levels(b, s);
    }
    b->graph_initflow = b->initflow;
    b->graph_initflow_rev = b->initflow_rev;
    b->graph_epoch = epoch;
    b->graph_xcu_off = xcu_off;
  }
  HIPCHK(hipGraphLaunch(b->graph_exec, s));
  return OFDIS_OK;
}

}  // namespace ofdis

extern "C" {

// Pipelined mode (ofdis_batch_set_pipeline(b, S), S = 2..4): the batch is cut into S sub-batches; sub-batch 0 runs on
// the caller's stream, the others on internal streams that are forked from the caller's stream by an event but NOT
// joined back at the end of the call.  Consecutive calls then drift apart by up to one pass, so the coarse levels of
// one sub-batch (one or two wavefronts per SIMD, latency bound) overlap with the fine levels of another instead of
// leaving issue slots idle: +6 % at 4096 frames.  (Joining inside every call keeps the sub-batches in lock step and
// loses the effect -- measured.)  The price is an explicit join: results are complete on `stream` only after
// ofdis_batch_join(b, stream); download / upsample join by themselves.  Frames are independent, results unaffected.
int ofdis_batch_set_pipeline(ofdis_batch* b, int sub_batches) {
  if (!b || sub_batches < 0 || sub_batches > 4) return fail(OFDIS_ERR_INVALID, "sub_batches must be 0..4");
  if (b->join_pending) HIPCHK(hipDeviceSynchronize());
  b->join_pending = false;
  b->pipeline = sub_batches < 1 ? 1 : sub_batches;
  return OFDIS_OK;
}

int ofdis_batch_join(ofdis_batch* b, void* stream) {
  if (!b) return fail(OFDIS_ERR_INVALID, "batch is NULL");
  if (!b->join_pending) return OFDIS_OK;
  for (hipEvent_t ev : b->sub_done) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, ev, 0));  // never-recorded events are complete
  b->join_pending = false;
  return OFDIS_OK;
}

int ofdis_batch_set_graph(ofdis_batch* b, int mode) {
  if (!b || mode < -1 || mode > 1) return fail(OFDIS_ERR_INVALID, "mode must be -1 (auto), 0 (off) or 1 (on)");
  b->graph_mode = mode;
  return OFDIS_OK;
}

int ofdis_batch_run(ofdis_batch* b, void* stream) {
  if (!b) return fail(OFDIS_ERR_INVALID, "batch is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = xcu_begin_pass(b, s)) return rc;
  int S = (b->timing || b->p.verbosity != 0) ? 1 : b->pipeline;
  if (b->nframes < 2 * S) S = 1;
  if (S == 1) {
    int rc = ofdis_batch_join(b, stream);  // a previous pipelined pass may still be running
    if (rc) return rc;
    return run_graph_or_levels(b, s);
  }
  if (!b->sub_start) HIPCHK(hipEventCreateWithFlags(&b->sub_start, hipEventDisableTiming));
  while ((int)b->sub_streams.size() < S - 1) {
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    b->sub_streams.push_back(st);
  }
  while ((int)b->sub_done.size() < S) {  // one per sub-batch, the caller's stream included: a join may happen on
    hipEvent_t ev;                        // another stream than the run
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    b->sub_done.push_back(ev);
  }
  HIPCHK(hipEventRecord(b->sub_start, s));  // fork: the internal streams see everything enqueued on `s` so far
  b->join_pending = true;                   // from here on sub-streams may carry work, whatever happens below
  const int per = (b->nframes + S - 1) / S;
  int rc = OFDIS_OK;
  for (int k = S - 1; k >= 0 && !rc; --k) {  // sub-batch 0 last, on the caller's stream
    const int f0 = k * per, n = std::min(per, b->nframes - f0);
    hipStream_t sk = k ? b->sub_streams[k - 1] : s;
    if (n > 0) {
      ofdis_batch v = frame_view(*b, f0, n);
      if (k) HIPCHK(hipStreamWaitEvent(sk, b->sub_start, 0));
      rc = run_levels(&v, sk);
    }
    if (!rc) HIPCHK(hipEventRecord(b->sub_done[k], sk));
  }
  return rc;
}

}  // extern "C"
