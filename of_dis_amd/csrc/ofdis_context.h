// ofdis_context.h -- the batch context of include/ofdis.h (struct ofdis_batch: every HBM buffer of the hot path) and what the
// host units share: ofdis_context.hip (memory, creation, inputs, result accessors), ofdis_schedule.hip (the level plan and the
// launch schedule), ofdis_products.hip (what is made from a context's flows: the finish, checks, interpolation, trajectories,
// filters, global motion, stabilisation) and ofdis_capi.hip (ofdis_flow, per-function entry points, runtime wrappers).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

// the library is compiled with -fvisibility=hidden: what include/ofdis.h declares is the whole export list
#pragma GCC visibility push(default)
#include "../../include/ofdis.h"
#pragma GCC visibility pop
#include "ofdis_kernels.h"

namespace ofdis {

// The launchers of one arithmetic contract (ofdis_kernels.h / ofdis_launchers.inc): every kernel file is compiled once per
// contract into ofdis::exact and ofdis::fused; a context fixes its contract at creation (ofdis_tuning::contract) and
// launches through its table.
// The list is stated once, as X(member, function of ofdis_launchers.inc): the struct and both tables (ofdis_context.hip) are
// made from it, every entry bound by name.
#define OFDIS_LAUNCHERS(X)                                                     \
  X(patch_optimize, launch_patch_optimize)                                     \
  X(patch_pixel_weights_supported, patch_pixel_weights_supported)              \
  X(densify, launch_densify)                                                   \
  X(patch_p_reference_order, launch_patch_p_reference_order)                   \
  X(warp, launch_warp)                                                         \
  X(derivatives, launch_derivatives)                                           \
  X(tv_prep_supported, tv_prep_supported)                                      \
  X(tv_prep_densifies, tv_prep_densifies)                                      \
  X(tv_prep, launch_tv_prep)                                                   \
  X(tv_system, launch_tv_system)                                               \
  X(sor, launch_sor)                                                           \
  X(tv_fused_supported, tv_fused_supported)                                    \
  X(tv_fused_params_ok, tv_fused_params_ok)                                    \
  X(tv_fused_mode, tv_fused_mode)                                              \
  X(tv_fused, launch_tv_fused)                                                 \
  X(tv_finish_records, launch_tv_finish_records)                               \
  X(to_diag, launch_to_diag)                                                   \
  X(from_diag, launch_from_diag)                                               \
  X(tv_finish, launch_tv_finish)                                               \
  X(flow_split, launch_flow_split)                                             \
  X(de_system, launch_de_system)                                               \
  X(de_sor, launch_de_sor)                                                     \
  X(de_update, launch_de_update)                                               \
  X(de_fused_supported, de_fused_supported)                                    \
  X(de_fused, launch_de_fused)
struct Launchers {
#define OFDIS_LAUNCHER_MEMBER(member, function) decltype(&exact::function) member;
  OFDIS_LAUNCHERS(OFDIS_LAUNCHER_MEMBER)
#undef OFDIS_LAUNCHER_MEMBER
};
const Launchers& launchers(int contract);

int fail(int code, const std::string& msg);  // sets ofdis_last_error, returns `code`
int hipfail(hipError_t e, const char* what);
#define HIPCHK(expr)                                  \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return hipfail(_e, #expr);  \
  } while (0)

struct EventPair {
  hipEvent_t a, b;
};

struct TvConsts {
  float quarter_alpha, half_delta_over3, half_gamma_over3;
};
inline TvConsts tv_consts(float alpha, float gamma, float delta) {  // refine_variational.cpp:40-42
  return {0.25f * alpha, delta * 0.5f / 3.0f, gamma * 0.5f / 3.0f};
}

// The routes of a level's TV refinement (VarRefClass, refine_variational.cpp:25-336):
//   GrayFused       gray levels of 16 ... 256 columns and <= 256 rows: tv_prep (warp + derivatives in one kernel, records out,
//                   optionally the densification too) and tv_fused (every fixed-point iteration in one launch), on the AoS flow
//   Records         RGB levels of <= 256 rows and gray levels wider than 256 columns: the per-stage warp, the derivatives
//                   kernel in its record form and tv_fused
//   PerStage        warp, derivatives, n_inner x (tv_system + sor), tv_finish
//   StereoFused     stereo-depth levels of <= 64 rows: warp, derivatives in record form, de_fused, de_update
//   StereoPerStage  warp, derivatives, n_inner x (de_system + de_sor), de_update
//   None            no refinement (usetvref off, or the gray fused route with no fixed-point iteration: du = dv = 0)
// Every route gives the same bits under the exact contract; they differ in speed (the measurements are with the rules below).
enum class Route { None, GrayFused, Records, PerStage, StereoFused, StereoPerStage };

// What a context allocates besides its inputs, flows and patch results, decided at creation under ONE snapshot of the knobs
struct Scratch {
  bool pixw = false;          // compact per-pixel weights of the RGB 12x12 patch kernels
  bool planes = false;        // wx, wy, du, dv, mask, w_im2, sys: the planes of the per-stage kernels
  size_t rec_px = 0;          // pixels per frame of the (wx, wy) records wrec (0: none) ...
  bool uv = false;            // ... and of the (du, dv) records uv
  size_t xbuf_per_frame = 0;  // floats: hand-over granules of the cross-CU variant of tv_fused
};

// What one pass does on one level: the refinement route and every knob-dependent choice along it.  Decided ONCE per level and
// pass from one snapshot of the knobs (plan_level), so that the patch kernel, the densification and the refinement agree even
// if another thread changes the knobs in between.
struct LevelPlan {
  Route route = Route::None;
  bool pixw = false;          // the patch kernel writes the compact per-pixel weights (DisArgs::pixw), the densification reads them
  bool dens_in_prep = false;  // GrayFused: tv_prep densifies from the patch results itself (no densify launch)
  int prep_band_rows = 0;     // GrayFused: PrepArgs::band_rows
  // FusedArgs choices (GrayFused, Records)
  int S = 1, tp_pipe = 0, mw_max_groups = 0, split = 0, tall_group = 0;
  bool fused_writes_flow = true;  // FusedArgs::flow_out given; else tv_finish_records forms the refined flow
  FusedXcu fx;                    // GrayFused: the cross-CU variant's arguments (xbuf null: never)
  // does the refinement start from the planes wx, wy (which the densification then writes) rather than from the AoS flow?
  bool planar() const { return route != Route::None && route != Route::GrayFused; }
};

}  // namespace ofdis

// Cross-CU variant of the fused TV kernel (ofdis_fused_xcu.hip): a workgroup whose hand-over row never arrives (bounded
// wait) sets a word in mapped host memory.  The word belongs to the CONTEXT that launched the kernel: it is allocated with
// the context (never on a launch path), polled by every synchronising entry point on behalf of that context only, and a
// context that has seen it once never launches the variant again (its granule array is re-zeroed before the next pass).
struct XcuState {
  int* host = nullptr;             // mapped, device-visible
  int* dev = nullptr;
  // (atomics: ofdis_sync polls the contexts of its stream from whichever thread synchronises, possibly while the context's
  // own thread starts its next pass)
  std::atomic<bool> off{false};        // the variant is off for this context
  std::atomic<bool> failed{false};     // the results of the last pass are invalid (until the next pass starts)
  std::atomic<bool> told_sync{false};  // ofdis_sync has reported the failure (it does so once; status / download keep saying it)
  std::atomic<bool> missed{false};     // a pass failed and the NEXT pass was started before anybody polled: reported once, late
  std::atomic<bool> rezero{false};     // the granule array may hold stale tags
  std::atomic<hipStream_t> last_stream{nullptr};  // where the last pass was enqueued (ofdis_sync polls the contexts of its stream)
  std::atomic<int> last_device{-1};               // ... and on which device (the null stream is "the same" stream on every device)
  std::atomic<bool> ran{false};
};

struct ofdis_batch {
  static constexpr int MAX_LEVELS = 21;  // check_params: 0 <= sc_l <= sc_f <= 20
  ofdis_params p;
  int contract = 0;                  // arithmetic contract, fixed at creation (ofdis_tuning::contract)
  const ofdis::Launchers* k = &ofdis::launchers(0);  // ... and its launchers
  int nframes = 0;
  int total_frames = 0;              // nframes of the owning context (a frame_view keeps it)
  int nlevels = 0;
  std::vector<ofdis::LevelGeom> geom;  // index = level - sc_l
  // Device arrays.  Every one is a float* MEMBER of this struct (per-level ones: fixed arrays, index = level - sc_l) and is
  // described once, where it is requested (dalloc): its size per frame.  Frame views and per-frame addresses derive from that.
  float* in[6][MAX_LEVELS] = {};     // A, A_dx, A_dy, B per level (+ B_dx, B_dy when usefbcon)
  bool sequence = false;             // OFDIS_BATCH_SEQUENCE: in[0..2] hold nframes + 1 frames (pair k = frames k, k + 1) and
                                     // in[3 + j] = in[j] + one frame: B's planes are A's, one frame further on (never allocated)
  float* flow_bw[MAX_LEVELS] = {};   // usefbcon: backward dense flow per level (oflow.cpp:162)
  float* pvec_bw = nullptr;          // usefbcon: backward grid results
  float* pweight_bw = nullptr;
  float* flow[MAX_LEVELS] = {};      // AoS dense flow per level
  int nop = 2;                       // flow channels (1 in stereo-depth mode)
  const float* initflow = nullptr;   // borrowed device pointer (ofdis_batch_set_initflow) or null
  bool reverse = false;              // OFDIS_BATCH_REVERSE: every pass also runs on the swapped pair (swap_direction)
  bool stereo_lr = false;            // OFDIS_BATCH_STEREO_LR: ... on the mirrored, swapped pair, whose planes are
  float* in_mir[6][MAX_LEVELS] = {}; //     A', A'_dx, A'_dy, B' per level (+ B'_dx, B'_dy when usefbcon)
  float* flow_rev[MAX_LEVELS] = {};  // the second direction's per-level results (reverse flow / mirror disparity)
  const float* initflow_rev = nullptr;  // ... from this warm start (ofdis_batch_set_initflow_reverse)
  float* initflow_own = nullptr;     // staging buffer of ofdis_batch_upload_initflow
  // scratch, sized for the finest level
  float *pvec = nullptr, *pweight = nullptr;
  float* pixw = nullptr;             // RGB: compact per-pixel weight denominators (ofdis_dev.h: pixw_row), [B][nop][P*P]
  float *wx = nullptr, *wy = nullptr, *du = nullptr, *dv = nullptr, *mask = nullptr;
  float *w_im2 = nullptr, *derivs = nullptr, *sys = nullptr;
  size_t rec_px = 0;                     // pixels per frame wrec / uv are sized for (RGB contexts: the largest level that can fuse)
  float *wrec = nullptr, *uv = nullptr;  // fused TV path: the (wx, wy) and (du, dv) records; `derivs` holds the
                                         // derivative records there (ofdis_dev.h: sdiag_index)
  float* xbuf = nullptr;                 // ... and the hand-over granules of its cross-CU variant (small contexts only)
  struct XcuState* xcu = nullptr;        // ... with the variant's error word (owned by the context; frame views share it)
  float* pyr_tmp[MAX_LEVELS] = {};   // unpadded level images (ofdis_batch_build_pyramids_u8), lazily allocated
  float* mir_u8 = nullptr;           // ... and, OFDIS_BATCH_STEREO_LR, one mirrored 8-bit frame set (bytes, held as floats)
  float *lr_u = nullptr, *lr_dr = nullptr, *lr_mask = nullptr;  // staging of ofdis_batch_upsample_lr above its fused width, lazy
  float* gm_slab = nullptr;          // records of sums of ofdis_batch_global_motion (ofdis_gmotion.hip; int64, held as floats), lazy
  float* pm_slab = nullptr;          // ... and the 24-sum records of ofdis_batch_projective_motion (int64, held as floats), lazy
  float* stab_path = nullptr;        // models [nframes][6] then warps [nframes + 1][6] of ofdis_batch_stabilize (fp64, held as floats), lazy
  float* stab_path8 = nullptr;       // ... and models [nframes][8] then warps [nframes + 1][8] of ofdis_batch_stabilize_projective, lazy
  float* dt_slab = nullptr;          // work buffer of ofdis_batch_dense_tracks (ofdis_dense_tracks.hip; held as floats), lazy: a
                                     // call that needs more than it holds requests a larger one (dstage)
  float* retired = nullptr;          // always null: where the descriptions of outgrown staging buffers point (dstage)
  // device memory: requests are collected (dalloc) and served from ONE hipMalloc per commit (dcommit) -- a context is
  // one allocation (two with the u8 pyramid scratch), and the input planes form one contiguous region [in_base,
  // in_base + in_bytes) in (level, kind) order so that a single-frame context is uploaded with one copy (ofdis_flow)
  struct Array { size_t slot, per_frame; bool view; int extra; };  // the member's byte offset in this struct; floats per frame
                                                         // (the array holds nframes + extra times as many: the frame slots of
                                                         // a sequence context are one more than its pairs); does a frame view
                                                         // get its share?
  std::vector<Array> arrays;  // in request order; [0, committed) are served
  size_t committed = 0;
  std::vector<void*> allocs;
  char* in_base = nullptr;
  size_t in_bytes = 0;
  // hipGraph replay of the launch schedule (ofdis_batch_set_graph)
  int graph_mode = 0;                    // 0 off (default), 1 on, -1 captured at the second pass
  long runs = 0;                         // un-pipelined passes so far
  hipGraphExec_t graph_exec = nullptr;
  const float* graph_initflow = nullptr; // the warm-start pointer the captured graph was built with
  const float* graph_initflow_rev = nullptr;  // ... and the reverse direction's
  unsigned graph_epoch = 0;              // ... and the state of the kernel-selection knobs (ofdis_set_tuning)
  bool graph_xcu_off = false;            // ... and whether the cross-CU fused TV variant was already off for this context
  hipStream_t cap_stream = nullptr;      // capture stream
  // sub-batches on internal streams (ofdis_batch_run)
  std::vector<hipStream_t> sub_streams;  // streams of sub-batches 1..S-1 (sub-batch 0 runs on the caller's stream)
  std::vector<hipEvent_t> sub_done;
  hipEvent_t sub_start = nullptr;
  int pipeline = 1;                      // ofdis_batch_set_pipeline: number of sub-batches (1 = none)
  bool join_pending = false;             // sub-batches may still be running on the internal streams
  // timing
  bool timing = false;
  std::vector<ofdis::EventPair> ev[OFDIS_K_COUNT];
  size_t ev_used[OFDIS_K_COUNT] = {0};

  const ofdis::LevelGeom& g(int level) const { return geom[level - p.sc_l]; }
};

namespace ofdis {

struct KTimer {  // brackets one launch with events when timing is on
  ofdis_batch* b;
  int k;
  hipStream_t s;
  EventPair* ep = nullptr;
  KTimer(ofdis_batch* b_, int k_, hipStream_t s_) : b(b_), k(k_), s(s_) {
    if (!b || !b->timing) return;
    auto& v = b->ev[k];
    if (b->ev_used[k] == v.size()) {
      EventPair e;
      (void)hipEventCreate(&e.a);
      (void)hipEventCreate(&e.b);
      v.push_back(e);
    }
    ep = &v[b->ev_used[k]++];
    (void)hipEventRecord(ep->a, s);
  }
  ~KTimer() {
    if (ep) (void)hipEventRecord(ep->b, s);
  }
};

// ofdis_context.hip
LevelGeom make_geom(const ofdis_params& p, int sl);
int check_params(const ofdis_params* p);
void context_init(ofdis_batch* b, const ofdis_params& p, int nframes, const ofdis_tuning& tn, int first_level, int last_level);
void context_release(ofdis_batch* b);  // everything the context owns; not the struct itself
void dalloc(ofdis_batch* b, float** member, size_t per_frame, bool view = true, int extra_frames = 0);  // request; served by dcommit()
int dcommit(ofdis_batch* b);
struct Stage { float** member; size_t per_frame; int extra_frames = 0; };
int dstage(ofdis_batch* b, const std::vector<Stage>& wants);  // staging made on first use: dalloc + dcommit of what is missing or too small
constexpr unsigned kOpticalFlow = 1u << 31;                   // beside the OFDIS_BATCH_* flags: not a stereo-depth context
int context_check(const ofdis_batch* b, unsigned needs);      // what a call needs of its context; fails naming what is missing
void dalloc_tv_scratch(ofdis_batch* b, const Scratch& sc);
int xcu_arm(ofdis_batch* b, hipStream_t s);
size_t frame_elems(const ofdis_batch& b, float* const& member);       // floats per frame of a context array, e.g. b.flow[0]
float* frame_at(const ofdis_batch& b, float* const& member, int f);  // ... and where its frame `f` starts
ofdis_batch frame_view(const ofdis_batch& b, int f0, int n);
extern std::mutex g_xcu_mutex;  // live contexts that own a cross-CU error word (ofdis_sync has only a stream to go by)
extern std::vector<ofdis_batch*> g_xcu_contexts;
// ofdis_schedule.hip
int xcu_poll(ofdis_batch* b);
int xcu_begin_pass(ofdis_batch* b, hipStream_t s);
DisArgs dis_args(const ofdis_params& p, const LevelGeom& g, int nframes);
Scratch size_scratch(const ofdis_batch& b, const ofdis_tuning& tn);
LevelPlan plan_level(const ofdis_batch& b, const LevelGeom& g, const ofdis_tuning& tn);
int refine_level(ofdis_batch* b, const LevelGeom& g, const LevelPlan& pl, const float* im_a, const float* im_b, float* flow,
                 hipStream_t s, int camlr = 0);
int run_one_level(ofdis_batch* b, int sl, hipStream_t s);

}  // namespace ofdis
