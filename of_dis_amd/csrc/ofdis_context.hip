// ofdis_context.hip -- the batch context's own half of the C ABI of include/ofdis.h: kernel-selection knobs, parameter
// handling, the context's device memory (array descriptions, frame views), creation, inputs and result accessors.
#include <cfloat>
#include <cmath>

#include "ofdis_context.h"

using namespace ofdis;

namespace ofdis {

#define OFDIS_LAUNCHER_TABLE(ns)                                                                                        \
  {ns::launch_patch_optimize, ns::patch_pixel_weights_supported, ns::launch_densify, ns::launch_patch_p_reference_order, ns::launch_warp, ns::launch_derivatives, ns::tv_prep_supported, ns::tv_prep_densifies,      \
   ns::launch_tv_prep, ns::launch_tv_system, ns::launch_sor, ns::tv_fused_supported, ns::tv_fused_params_ok,            \
   ns::tv_fused_mode, ns::launch_tv_fused, ns::launch_tv_finish_records, ns::launch_to_diag, ns::launch_from_diag,      \
   ns::launch_tv_finish, ns::launch_flow_split, ns::launch_de_system, ns::launch_de_sor, ns::launch_de_update,          \
   ns::de_fused_supported, ns::launch_de_fused}
const Launchers kExactLaunchers = OFDIS_LAUNCHER_TABLE(exact);
const Launchers kFusedLaunchers = OFDIS_LAUNCHER_TABLE(fused);
#undef OFDIS_LAUNCHER_TABLE
const Launchers& launchers(int contract) { return contract ? kFusedLaunchers : kExactLaunchers; }

// Kernel-selection knobs (include/ofdis.h: ofdis_tuning): read ONCE from the environment, changed only through
// ofdis_set_tuning; every launch path takes a snapshot (no getenv on the dispatch path).
static std::mutex g_tuning_mutex;
static ofdis_tuning g_tuning;
static bool g_tuning_init = false;
static unsigned g_tuning_epoch = 0;
static void tuning_init_locked() {
  if (g_tuning_init) return;
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  g_tuning.gray8 = !on("OFDIS_NO_GRAY8");
  g_tuning.rgb12 = !on("OFDIS_NO_RGB12");
  {
    const int l = num("OFDIS_RGB12_LPP", 0);
    g_tuning.rgb12_lpp = (l == 16 || l == 32 || l == 64) ? l : 0;
  }
  g_tuning.fused_tv = !on("OFDIS_NO_FUSED");
  g_tuning.fused_mw_max = std::max(0, num("OFDIS_FUSED_MW_MAX", 512));
  g_tuning.fused_split = !on("OFDIS_FUSED_NO_SPLIT");
  g_tuning.finish_fusion = !on("OFDIS_NO_FINISH_FUSION");
  g_tuning.fused_strip = std::max(0, num("OFDIS_FUSED_STRIP", 0));
  g_tuning.prep_band_rows = std::max(0, num("OFDIS_PREP_BAND_ROWS", 0));
  g_tuning.graph = !on("OFDIS_NO_GRAPH");
  g_tuning.flow_dma = on("OFDIS_FLOW_DMA");
  g_tuning.flow_whole = on("OFDIS_FLOW_WHOLE");
  g_tuning.fused_xcu_max = std::max(0, num("OFDIS_FUSED_XCU_MAX", 768));
  g_tuning.fused_tp_pipe = std::max(0, std::min(2, num("OFDIS_FUSED_TP_PIPE", 1)));
  g_tuning.fused_xcu_spin = std::max(0, num("OFDIS_FUSED_XCU_SPIN", 0));
  g_tuning.fused_xcu_drop = num("OFDIS_FUSED_XCU_DROP", 0) != 0;  // test hook
  g_tuning.prep_densify = !on("OFDIS_NO_PREP_DENSIFY");
  g_tuning.fused_tall_group = on("OFDIS_NO_TALL_GROUP") ? 0 : std::max(1, std::min(7, num("OFDIS_TALL_GROUP", 1)));
  g_tuning.fused_rgb_min = std::max(0, num("OFDIS_FUSED_RGB_MIN", 0));
  {  // arithmetic contract: "fused" / "1" = the tolerance contract, anything else (or unset) = exact
    const char* e = getenv("OFDIS_CONTRACT");
    g_tuning.contract = (e && (!strcmp(e, "fused") || !strcmp(e, "1"))) ? 1 : 0;
  }
  g_tuning_init = true;
}

ofdis_tuning tuning(unsigned* epoch) {
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  tuning_init_locked();
  if (epoch) *epoch = g_tuning_epoch;
  return g_tuning;
}

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hipfail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return OFDIS_ERR_DEVICE;
}

// Level geometry exactly as the reference derives it (oflow.cpp:91-92,138-151; patchgrid.cpp:42-48).
LevelGeom make_geom(const ofdis_params& p, int sl) {
  LevelGeom g;
  memset(&g, 0, sizeof(g));
  const float sc_fct = (float)pow(2, -sl);
  g.level = sl;
  g.h = (int)(p.height * sc_fct);
  g.w = (int)(p.width * sc_fct);
  g.pad = p.imgpadding;
  g.noc = p.noc;
  g.P = p.p_samp_s;
  g.lb = -(float)p.p_samp_s / 2;
  g.ubw = (float)(g.w + p.p_samp_s / 2 - 2);
  g.ubh = (float)(g.h + p.p_samp_s / 2 - 2);
  g.tmp_w = g.w + 2 * g.pad;
  g.tmp_h = g.h + 2 * g.pad;
  int steps = (int)floor(p.p_samp_s * (1 - p.patove));
  g.steps = steps < 1 ? 1 : steps;
  g.steps_magic = g.steps > 1 ? (unsigned)((0x100000000ull + (unsigned)g.steps - 1) / (unsigned)g.steps) : 0u;
  g.novals = p.noc * p.p_samp_s * p.p_samp_s;
  g.nopw = (int)ceil((float)g.w / (float)g.steps);
  g.noph = (int)ceil((float)g.h / (float)g.steps);
  g.offw = (int)floor((g.w - (g.nopw - 1) * g.steps) / 2);
  g.offh = (int)floor((g.h - (g.noph - 1) * g.steps) / 2);
  g.nop = g.nopw * g.noph;
  g.plane_elems = (size_t)g.tmp_w * g.tmp_h * g.noc;
  return g;
}

int check_params(const ofdis_params* p) {
  if (!p) return fail(OFDIS_ERR_INVALID, "params is NULL");
  if (p->noc != 1 && p->noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (p->sc_l < 0 || p->sc_f < p->sc_l || p->sc_f > 20) return fail(OFDIS_ERR_INVALID, "need 0 <= sc_l <= sc_f");
  if (p->width <= 0 || p->height <= 0 || (p->width % (1 << p->sc_f)) || (p->height % (1 << p->sc_f)))
    return fail(OFDIS_ERR_INVALID, "width/height must be positive multiples of 2^sc_f (oflow.h:87)");
  if ((p->width >> p->sc_l) > 32768 || (p->height >> p->sc_l) > 32768)
    return fail(OFDIS_ERR_UNSUPPORTED, "finest level larger than 32768 pixels in one dimension");
  if (p->p_samp_s < 2 || (p->p_samp_s & 1)) return fail(OFDIS_ERR_INVALID, "p_samp_s must be even and >= 2");
  if (p->imgpadding < p->p_samp_s) return fail(OFDIS_ERR_INVALID, "imgpadding must be >= p_samp_s (oflow.cpp:147-149)");
  if (p->noc * p->p_samp_s * p->p_samp_s > 64 * 12) return fail(OFDIS_ERR_UNSUPPORTED, "patch too large (novals > 768)");
  if (p->costfct < 0 || p->costfct > 2) return fail(OFDIS_ERR_UNSUPPORTED, "costfct must be 0, 1 or 2");
  if (!(p->patove >= 0.0f && p->patove < 1.0f)) return fail(OFDIS_ERR_INVALID, "patove must be in [0,1)");
  if (p->usetvref && ((p->height >> p->sc_f) < 4))
    return fail(OFDIS_ERR_INVALID, "coarsest level must have >= 4 rows for the TV derivative filter (image.c:401-434)");
  if (p->max_iter < 0 || p->tv_innerit < 0 || p->tv_solverit < 0) return fail(OFDIS_ERR_INVALID, "negative iteration count");
  if (p->selectmode < 0 || p->selectmode > 2) return fail(OFDIS_ERR_INVALID, "selectmode must be 0/1 (optical flow) or 2 (stereo depth)");
  return OFDIS_OK;
}

// What create turns (params, frame count, knob snapshot) into before any memory is requested: contract, launchers, frame
// counts, flow channels and the geometry of levels first_level .. last_level (a whole context: sc_l .. sc_f).
void context_init(ofdis_batch* b, const ofdis_params& p, int nframes, const ofdis_tuning& tn, int first_level, int last_level) {
  b->p = p;
  b->contract = tn.contract ? 1 : 0;
  b->k = &launchers(b->contract);
  b->nframes = b->total_frames = nframes;
  b->nlevels = last_level - first_level + 1;
  b->nop = p.selectmode == 2 ? 1 : 2;
  for (int l = first_level; l <= last_level; ++l) b->geom.push_back(make_geom(p, l));
}

static float*& member(const ofdis_batch& b, const ofdis_batch::Array& a) { return *(float**)((char*)&b + a.slot); }
static size_t array_elems(const ofdis_batch& b, const ofdis_batch::Array& a) { return a.per_frame * ((size_t)b.nframes + a.extra); }
static size_t array_bytes(const ofdis_batch& b, const ofdis_batch::Array& a) {  // (every array starts on a 256-byte boundary)
  const size_t elems = array_elems(b, a);
  return ((elems ? elems : 1) * sizeof(float) + 255) & ~(size_t)255;
}

// THE description of a device array: `per_frame` floats for each of the context's frames (and `extra_frames` more), at `slot`
// (a float* member of *b).
void dalloc(ofdis_batch* b, float** slot, size_t per_frame, bool view, int extra_frames) {
  *slot = nullptr;
  b->arrays.push_back({(size_t)((char*)slot - (char*)b), per_frame, view, extra_frames});
}
// Test hook OFDIS_POISON_SCRATCH=1: fresh device memory holds NaN patterns instead of zeros.  Read at every allocation (never
// on a launch path): the tests switch it while the library is loaded.
static int scratch_fill_byte() {
  const char* poison = getenv("OFDIS_POISON_SCRATCH");
  return (poison && poison[0] == '1') ? 0xFF : 0;
}
int dcommit(ofdis_batch* b) {
  size_t total = 0;
  for (size_t i = b->committed; i < b->arrays.size(); ++i) total += array_bytes(*b, b->arrays[i]);
  if (!total) return OFDIS_OK;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, total);
  if (e == hipSuccess) {
    b->allocs.push_back(d);
    // Every context starts from zeroed scratch: no result may depend on what an allocation held before.  (Poisoned: the GPU
    // tests run whole flows and single levels that way and expect the same bits, i.e. nothing is read before it is written
    // except where zero is the defined initial value.)
    e = hipMemsetAsync(d, scratch_fill_byte(), total, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  if (e != hipSuccess) {
    b->arrays.resize(b->committed);  // (their members are null)
    return hipfail(e, d ? "hipMemset" : "hipMalloc");
  }
  char* c = (char*)d;
  for (; b->committed < b->arrays.size(); ++b->committed) {
    member(*b, b->arrays[b->committed]) = (float*)c;
    c += array_bytes(*b, b->arrays[b->committed]);
  }
  return OFDIS_OK;
}
// the TV scratch of `sc`: requests, which dcommit serves (or fails)
void dalloc_tv_scratch(ofdis_batch* b, const Scratch& sc) {
  const size_t npx = (size_t)b->geom[0].w * b->geom[0].h, noc = b->p.noc;
  if (sc.planes) {
    dalloc(b, &b->wx, npx); dalloc(b, &b->wy, npx); dalloc(b, &b->du, npx); dalloc(b, &b->dv, npx);
    dalloc(b, &b->mask, npx); dalloc(b, &b->w_im2, npx * noc); dalloc(b, &b->sys, npx * 7);
  }
  dalloc(b, &b->derivs, npx * 8 * noc);
  b->rec_px = sc.rec_px;
  if (sc.rec_px) dalloc(b, &b->wrec, sc.rec_px * 2);
  if (sc.rec_px && sc.uv) dalloc(b, &b->uv, sc.rec_px * 2);
  if (sc.xbuf_per_frame) dalloc(b, &b->xbuf, sc.xbuf_per_frame);
}

size_t frame_elems(const ofdis_batch& b, float* const& slot) {
  const size_t off = (size_t)((const char*)&slot - (const char*)&b);
  for (const ofdis_batch::Array& a : b.arrays)
    if (a.slot == off) return a.per_frame;
  return 0;  // (never requested: the member is null)
}
float* frame_at(const ofdis_batch& b, float* const& slot, int f) {
  return slot ? slot + (size_t)f * frame_elems(b, slot) : nullptr;
}

// A contiguous range of a batch's frames as a batch of its own: every array a view sees is advanced to frame f0 by its own
// description, so a sub-batch gets exactly its share of every input, output and scratch array and the shares never overlap.
// The view owns nothing.
ofdis_batch frame_view(const ofdis_batch& b, int f0, int n) {
  ofdis_batch v = b;
  v.allocs.clear(); v.sub_streams.clear(); v.sub_done.clear();
  v.timing = false;
  v.nframes = n;
  for (const ofdis_batch::Array& a : b.arrays) {
    float*& ptr = member(v, a);
    if (!a.view) ptr = nullptr;
    else if (ptr) ptr += (size_t)f0 * a.per_frame;
  }
  if (b.sequence)  // kinds 3..5 are no arrays of their own (the same planes one frame further on): they move with the others
    for (int i = 0; i < b.nlevels; ++i)
      for (int k = 3; k < 6; ++k)
        if (v.in[k][i]) v.in[k][i] += (size_t)f0 * b.geom[i].plane_elems;
  if (v.initflow) v.initflow += (size_t)f0 * ofdis_batch_initflow_elems(&b);
  if (v.initflow_rev) v.initflow_rev += (size_t)f0 * ofdis_batch_initflow_elems(&b);
  return v;
}

std::mutex g_xcu_mutex;
std::vector<ofdis_batch*> g_xcu_contexts;

// The cross-CU variant's state of a context that owns granules (with the context, never on a launch path): their tags zeroed
// on `s` (0 = not yet written; the kernel restores the zeros itself) and the error word.
int xcu_arm(ofdis_batch* b, hipStream_t s) {
  if (!b->xbuf) return OFDIS_OK;
  HIPCHK(hipMemsetAsync(b->xbuf, 0, frame_elems(*b, b->xbuf) * b->nframes * sizeof(float), s));
  void* h = nullptr;
  void* d = nullptr;
  HIPCHK(hipHostMalloc(&h, sizeof(int), hipHostMallocMapped | hipHostMallocPortable));
  *(volatile int*)h = 0;
  hipError_t e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) { (void)hipHostFree(h); return hipfail(e, "hipHostGetDevicePointer"); }
  b->xcu = new XcuState();
  b->xcu->host = (int*)h;
  b->xcu->dev = (int*)d;
  return OFDIS_OK;
}

void context_release(ofdis_batch* b) {
  if (b->xcu) {
    {
      std::lock_guard<std::mutex> lock(g_xcu_mutex);
      g_xcu_contexts.erase(std::remove(g_xcu_contexts.begin(), g_xcu_contexts.end(), b), g_xcu_contexts.end());
    }
    (void)hipHostFree(b->xcu->host);
    delete b->xcu;
    b->xcu = nullptr;
  }
  for (hipStream_t st : b->sub_streams) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  for (hipEvent_t ev : b->sub_done) (void)hipEventDestroy(ev);
  if (b->sub_start) (void)hipEventDestroy(b->sub_start);
  if (b->graph_exec) (void)hipGraphExecDestroy(b->graph_exec);
  if (b->cap_stream) (void)hipStreamDestroy(b->cap_stream);
  for (void* d : b->allocs) (void)hipFree(d);
  for (int k = 0; k < OFDIS_K_COUNT; ++k)
    for (auto& e : b->ev[k]) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
}

// host pyramids src[0 .. nkinds) into frame `frame` of the input planes in[first_kind ..] (a sequence context: frame slot)
static int upload_planes(ofdis_batch* b, int frame, int first_kind, int nkinds, const float* const* const* src, hipStream_t s) {
  for (int l = b->p.sc_l; l <= b->p.sc_f; ++l)
    for (int k = 0; k < nkinds; ++k) {
      float* const& plane = b->in[first_kind + k][l - b->p.sc_l];
      if (!src[k][l]) return fail(OFDIS_ERR_INVALID, "pyramid level pointer is NULL");
      HIPCHK(hipMemcpyAsync(frame_at(*b, plane, frame), src[k][l], frame_elems(*b, plane) * sizeof(float), hipMemcpyHostToDevice, s));
    }
  return OFDIS_OK;
}

static const char* const kSeqOnly = "not a context created with OFDIS_BATCH_SEQUENCE";
static int seq_refuses(const char* what, const char* instead) {
  return fail(OFDIS_ERR_INVALID, std::string(what) + " takes frame pairs; an OFDIS_BATCH_SEQUENCE context shares its frame slots "
                                                     "between pairs and is filled through " + instead);
}

// the forward / reverse halves of the result accessors
static const float* level_flow(const ofdis_batch& b, int level, bool reverse) {
  if (level < b.p.sc_l || level > b.p.sc_f) return nullptr;
  return (reverse ? b.flow_rev : b.flow)[level - b.p.sc_l];  // (flow_rev: null without OFDIS_BATCH_REVERSE)
}
static int download(ofdis_batch* b, int frame, float* outflow_host, hipStream_t s, bool reverse) {
  float* const& flow = reverse ? b->flow_rev[0] : b->flow[0];
  if (int rc = ofdis_batch_join(b, s)) return rc;
  HIPCHK(hipMemcpyAsync(outflow_host, frame_at(*b, flow, frame), frame_elems(*b, flow) * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return xcu_poll(b);
}

static bool fb_constants_ok(float alpha, float beta) {
  return std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f;
}

static_assert(sizeof(InterpTimes::t) / sizeof(float) == OFDIS_INTERP_MAX_TIMES, "InterpTimes holds OFDIS_INTERP_MAX_TIMES");
static int interp_times(const float* times, int ntimes, InterpTimes& ts) {
  if (!times) return fail(OFDIS_ERR_INVALID, "times is NULL");
  if (ntimes < 1 || ntimes > OFDIS_INTERP_MAX_TIMES) return fail(OFDIS_ERR_INVALID, "ntimes must be 1..OFDIS_INTERP_MAX_TIMES");
  memset(&ts, 0, sizeof(ts));
  for (int k = 0; k < ntimes; ++k) {
    if (!(std::isfinite(times[k]) && times[k] >= 0.0f && times[k] <= 1.0f))
      return fail(OFDIS_ERR_INVALID, "every time must be finite and inside [0, 1]");
    ts.t[k] = times[k];
  }
  ts.n = ntimes;
  return OFDIS_OK;
}

}  // namespace ofdis

extern "C" {

const char* ofdis_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------ kernel-selection knobs
int ofdis_get_tuning(ofdis_tuning* out) {
  if (!out) return fail(OFDIS_ERR_INVALID, "out is NULL");
  *out = ofdis::tuning();
  return OFDIS_OK;
}
int ofdis_set_tuning(const ofdis_tuning* in) {
  if (!in) return fail(OFDIS_ERR_INVALID, "tuning is NULL");
  if (in->rgb12_lpp != 0 && in->rgb12_lpp != 16 && in->rgb12_lpp != 32 && in->rgb12_lpp != 64)
    return fail(OFDIS_ERR_INVALID, "rgb12_lpp must be 0 (library's choice), 16, 32 or 64");
  if (in->fused_mw_max < 0 || in->fused_strip < 0 || in->prep_band_rows < 0 || in->fused_xcu_max < 0 || in->fused_xcu_spin < 0)
    return fail(OFDIS_ERR_INVALID, "negative knob");
  if (in->fused_strip > 64 || in->prep_band_rows > 64)  // (strips index their records with 32-bit byte offsets)
    return fail(OFDIS_ERR_INVALID, "fused_strip / prep_band_rows must be <= 64");
  if (in->fused_tp_pipe < 0 || in->fused_tp_pipe > 2) return fail(OFDIS_ERR_INVALID, "fused_tp_pipe must be 0, 1 or 2");
  if (in->contract != 0 && in->contract != 1) return fail(OFDIS_ERR_INVALID, "contract must be 0 (exact) or 1 (fused)");
  if (in->fused_xcu_spin > 30000000) return fail(OFDIS_ERR_INVALID, "fused_xcu_spin is a wait in microseconds, at most 30 s");
  if (in->fused_xcu_drop != 0 && in->fused_xcu_drop != 1) return fail(OFDIS_ERR_INVALID, "fused_xcu_drop (test hook) must be 0 or 1");
  if (in->prep_densify != 0 && in->prep_densify != 1) return fail(OFDIS_ERR_INVALID, "prep_densify must be 0 or 1");
  if (in->fused_tall_group < 0 || in->fused_tall_group > 7) return fail(OFDIS_ERR_INVALID, "fused_tall_group must be 0 .. 7");
  if (in->fused_rgb_min < 0) return fail(OFDIS_ERR_INVALID, "negative knob");
  ofdis::tuning();  // initialise from the environment first
  std::lock_guard<std::mutex> lock(ofdis::g_tuning_mutex);
  ofdis::g_tuning = *in;
  ++ofdis::g_tuning_epoch;
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ batch context
int ofdis_batch_create(ofdis_batch** out, const ofdis_params* p, int nframes) { return ofdis_batch_create_ex(out, p, nframes, 0); }

int ofdis_batch_create_ex(ofdis_batch** out, const ofdis_params* p, int nframes, unsigned flags) {
  if (!out) return fail(OFDIS_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int rc = check_params(p);
  if (rc) return rc;
  if (nframes < 1) return fail(OFDIS_ERR_INVALID, "nframes must be >= 1");
  if (flags & ~(OFDIS_BATCH_REVERSE | OFDIS_BATCH_STEREO_LR | OFDIS_BATCH_SEQUENCE)) return fail(OFDIS_ERR_INVALID, "unknown flag bits");
  const bool reverse = (flags & OFDIS_BATCH_REVERSE) != 0, stereo_lr = (flags & OFDIS_BATCH_STEREO_LR) != 0;
  const bool sequence = (flags & OFDIS_BATCH_SEQUENCE) != 0;
  if (reverse && p->selectmode == 2)
    return fail(OFDIS_ERR_UNSUPPORTED, "OFDIS_BATCH_REVERSE: no reverse direction in stereo-depth mode (selectmode 2); the "
                                       "right view is OFDIS_BATCH_STEREO_LR");
  if (stereo_lr && p->selectmode != 2) return fail(OFDIS_ERR_INVALID, "OFDIS_BATCH_STEREO_LR needs stereo-depth mode (selectmode 2)");
  if (sequence && (stereo_lr || p->selectmode == 2))
    return fail(OFDIS_ERR_INVALID, "OFDIS_BATCH_SEQUENCE: a stereo pair is not a sequence (selectmode 2, OFDIS_BATCH_STEREO_LR)");
  if (nframes > 65535)  // launch_warp / launch_upsample_crop carry the frame in grid.z
    return fail(OFDIS_ERR_UNSUPPORTED, "at most 65535 frames per batch context");
  if (sequence && nframes > 65534)  // launch_pyr_planes carries the nframes + 1 frame slots in grid.y
    return fail(OFDIS_ERR_UNSUPPORTED, "at most 65534 pairs (65535 frames) per OFDIS_BATCH_SEQUENCE context");
  ofdis_batch* b = new ofdis_batch();
  const ofdis_tuning tn = tuning();  // ONE snapshot decides the contract and the scratch
  context_init(b, *p, nframes, tn, p->sc_l, p->sc_f);
  b->reverse = reverse;
  b->stereo_lr = stereo_lr;
  b->sequence = sequence;
  // (the reverse pass reads B's gradients as its A's.)  A sequence: image, dx, dy of nframes + 1 frame slots; kinds 3..5 derive
  const int nin = sequence ? 3 : (p->usefbcon || reverse) ? 6 : 4;
  for (int i = 0; i < b->nlevels; ++i)  // the input planes first: one contiguous region in (level, kind) order
    for (int k = 0; k < nin; ++k) dalloc(b, &b->in[k][i], b->geom[i].plane_elems, true, sequence ? 1 : 0);
  for (const ofdis_batch::Array& a : b->arrays) b->in_bytes += array_bytes(*b, a);
  if (stereo_lr)  // the mirrored pair's planes: the same sizes, stated by the same expression
    for (int i = 0; i < b->nlevels; ++i)
      for (int k = 0; k < nin; ++k) dalloc(b, &b->in_mir[k][i], b->geom[i].plane_elems);
  for (int i = 0; i < b->nlevels; ++i) {
    const size_t flow_elems = (size_t)b->geom[i].w * b->geom[i].h * b->nop;
    dalloc(b, &b->flow[i], flow_elems);
    if (reverse || stereo_lr) dalloc(b, &b->flow_rev[i], flow_elems);
    if (p->usefbcon && i > 0) dalloc(b, &b->flow_bw[i], flow_elems);
  }
  const LevelGeom& g0 = b->geom[0];  // finest level: largest of everything
  size_t nop_max = 0;
  for (auto& g : b->geom) nop_max = std::max(nop_max, (size_t)g.nop);
  const Scratch sc = size_scratch(*b, tn);
  dalloc(b, &b->pvec, nop_max * 2);
  dalloc(b, &b->pweight, nop_max * g0.novals);
  if (sc.pixw) dalloc(b, &b->pixw, nop_max * (size_t)g0.P * g0.P);
  if (p->usefbcon) dalloc(b, &b->pvec_bw, nop_max * 2);
  if (p->usefbcon) dalloc(b, &b->pweight_bw, nop_max * g0.novals);
  if (p->usetvref) dalloc_tv_scratch(b, sc);
  rc = dcommit(b);
  if (!rc) b->in_base = (char*)b->in[0][0];
  if (!rc && sequence)  // B of pair k is frame k + 1: the same arrays, one frame further on
    for (int i = 0; i < b->nlevels; ++i)
      for (int k = 0; k < 3; ++k) b->in[3 + k][i] = b->in[k][i] + b->geom[i].plane_elems;
  if (!rc) rc = xcu_arm(b, nullptr);
  if (!rc && b->xcu) {
    const hipError_t e = hipStreamSynchronize(nullptr);  // (the zeroing)
    if (e != hipSuccess) rc = hipfail(e, "hipMemset");
  }
  if (!rc && b->xcu) {
    std::lock_guard<std::mutex> lock(g_xcu_mutex);
    g_xcu_contexts.push_back(b);
  }
  if (rc) {
    ofdis_batch_destroy(b);
    return rc == OFDIS_ERR_DEVICE ? OFDIS_ERR_NOMEM : rc;
  }
  *out = b;
  return OFDIS_OK;
}

void ofdis_batch_destroy(ofdis_batch* b) {
  if (b) context_release(b);
  delete b;
}

float* ofdis_batch_input(ofdis_batch* b, int level, int kind) {
  if (!b || level < b->p.sc_l || level > b->p.sc_f || kind < 0) return nullptr;
  const int nin = (b->p.usefbcon || b->reverse || b->sequence) ? 6 : 4;
  if (kind < nin) return b->in[kind][level - b->p.sc_l];
  if (b->stereo_lr && kind >= 6 && kind < 6 + nin) return b->in_mir[kind - 6][level - b->p.sc_l];  // the mirrored pair's
  return nullptr;
}
size_t ofdis_batch_input_elems(const ofdis_batch* b, int level) {
  if (!b || level < b->p.sc_l || level > b->p.sc_f) return 0;
  return b->g(level).plane_elems;
}
int ofdis_batch_input_frames(const ofdis_batch* b) { return b ? b->nframes + (b->sequence ? 1 : 0) : 0; }
size_t ofdis_batch_device_bytes(const ofdis_batch* b) {
  size_t total = 0;
  if (b)
    for (size_t i = 0; i < b->committed; ++i) total += array_elems(*b, b->arrays[i]) * sizeof(float);
  return total;
}

int ofdis_batch_upload(ofdis_batch* b, int frame, const float* const* im_a, const float* const* im_a_dx,
                       const float* const* im_a_dy, const float* const* im_b, void* stream) {
  if (!b || frame < 0 || frame >= b->nframes || !im_a || !im_a_dx || !im_a_dy || !im_b)
    return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (b->sequence) return seq_refuses("ofdis_batch_upload", "ofdis_batch_upload_frame");
  const float* const* src[4] = {im_a, im_a_dx, im_a_dy, im_b};
  return upload_planes(b, frame, 0, 4, src, (hipStream_t)stream);
}

int ofdis_batch_upload_b_gradients(ofdis_batch* b, int frame, const float* const* im_b_dx, const float* const* im_b_dy,
                                   void* stream) {
  if (!b || frame < 0 || frame >= b->nframes || !im_b_dx || !im_b_dy) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (b->sequence) return seq_refuses("ofdis_batch_upload_b_gradients", "ofdis_batch_upload_frame");
  if (!b->p.usefbcon && !b->reverse) return OFDIS_OK;  // never read (patch.cpp:90-97)
  const float* const* src[2] = {im_b_dx, im_b_dy};
  return upload_planes(b, frame, 4, 2, src, (hipStream_t)stream);
}

int ofdis_batch_upload_frame(ofdis_batch* b, int slot, const float* const* im, const float* const* im_dx,
                             const float* const* im_dy, void* stream) {
  if (!b || !b->sequence) return fail(OFDIS_ERR_INVALID, kSeqOnly);
  if (slot < 0 || slot > b->nframes || !im || !im_dx || !im_dy) return fail(OFDIS_ERR_INVALID, "bad arguments");
  const float* const* src[3] = {im, im_dx, im_dy};
  return upload_planes(b, slot, 0, 3, src, (hipStream_t)stream);
}

// One frame set of `count` 8-bit frames (row y of frame f at src + f * stride + y * pitch) through the pyramid schedule: the
// base level, then per level the planes -- image, and the gradients where the set has them (non-null) -- plus the next
// level's unpadded image.
static int build_frame_set(ofdis_batch* b, const uint8_t* src, size_t pitch, size_t stride, int count,
                           float* (*planes)[ofdis_batch::MAX_LEVELS], int width_org, int height_org, hipStream_t s) {
  const ofdis_params& p = b->p;
  HIPCHK(launch_pyr_base(src, b->pyr_tmp[0], count, width_org, height_org, p.width, p.height, p.noc, p.sc_l, pitch, stride, s));
  for (int i = 0; i < b->nlevels; ++i) {
    const LevelGeom& g = b->geom[i];
    // the planes of level i and, in the same launch where the geometry allows, the unpadded image of level i + 1
    // (2x2 means: cv::resize(.5,.5), run_dense.cpp:150)
    float* down = i + 1 < b->nlevels ? b->pyr_tmp[i + 1] : nullptr;
    HIPCHK(launch_pyr_planes(b->pyr_tmp[i], planes[0][i], planes[1][i], planes[2][i], count, g.w, g.h, p.noc, g.pad, s, down));
  }
  return OFDIS_OK;
}
// the checks both 8-bit entry points share, and the unpadded level images (lazily; a frame view never sees them)
static int build_prepare(ofdis_batch* b, int width_org, int height_org) {
  const ofdis_params& p = b->p;
  // the padded size must be what run_dense.cpp:298-305 derives from the original size
  const int sc = 1 << p.sc_f;
  if (width_org < 1 || height_org < 1 || width_org > p.width || height_org > p.height || p.width - width_org >= sc ||
      p.height - height_org >= sc)
    return fail(OFDIS_ERR_INVALID, "params.width/height are not the 2^sc_f padding of the original size");
  // level l images need 8+2l bits, the Sobel partial sums 10+2l: exact in fp32 up to l = 7 (ofdis_pyr.hip)
  if (p.sc_f > 7) return fail(OFDIS_ERR_UNSUPPORTED, "exact fp32 pyramid needs sc_f <= 7");
  if (!b->pyr_tmp[0]) {
    for (int i = 0; i < b->nlevels; ++i)
      dalloc(b, &b->pyr_tmp[i], (size_t)b->geom[i].w * b->geom[i].h * b->geom[i].noc, false, b->sequence ? 1 : 0);
    if (b->stereo_lr) dalloc(b, &b->mir_u8, ((size_t)p.width * p.height * p.noc + 3) / 4, false);
    if (int rc = dcommit(b)) return rc;
  }
  return OFDIS_OK;
}

int ofdis_batch_build_pyramids_u8_seq(ofdis_batch* b, const uint8_t* frames, size_t row_pitch, size_t frame_stride,
                                      int width_org, int height_org, void* stream) {
  if (!b || !b->sequence) return fail(OFDIS_ERR_INVALID, kSeqOnly);
  if (!frames) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (width_org < 1 || height_org < 1) return fail(OFDIS_ERR_INVALID, "params.width/height are not the 2^sc_f padding of the original size");
  const size_t row_bytes = (size_t)width_org * b->p.noc;
  if (!row_pitch) row_pitch = row_bytes;
  if (row_pitch < row_bytes) return fail(OFDIS_ERR_INVALID, "row_pitch is shorter than a row (width_org * noc bytes)");
  if (!frame_stride) frame_stride = row_pitch * height_org;
  if (frame_stride < row_pitch * height_org) return fail(OFDIS_ERR_INVALID, "frame_stride is shorter than a frame (row_pitch * height_org bytes)");
  if (int rc = build_prepare(b, width_org, height_org)) return rc;
  // every frame once: its planes are B's of the pair before it and A's of the pair after it
  return build_frame_set(b, frames, row_pitch, frame_stride, b->nframes + 1, &b->in[0], width_org, height_org, (hipStream_t)stream);
}

int ofdis_batch_build_pyramids_u8(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int width_org,
                                  int height_org, void* stream) {
  if (!b || !img_a || !img_b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (b->sequence) return seq_refuses("ofdis_batch_build_pyramids_u8", "ofdis_batch_build_pyramids_u8_seq");
  const ofdis_params& p = b->p;
  if (int rc = build_prepare(b, width_org, height_org)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t pitch = (size_t)width_org * p.noc, stride = pitch * height_org;  // packed frames
  // (B's gradients only exist, non-null, with usefbcon or OFDIS_BATCH_REVERSE)
  auto build = [&](const uint8_t* src, float* (*planes)[ofdis_batch::MAX_LEVELS]) -> int {
    return build_frame_set(b, src, pitch, stride, b->nframes, planes, width_org, height_org, s);
  };
  if (int rc = build(img_a, &b->in[0])) return rc;
  if (int rc = build(img_b, &b->in[3])) return rc;
  if (b->stereo_lr) {  // (A', B') = (mir(B), mir(A)): mirrored as 8-bit frames into scratch, then the same kernels
    uint8_t* m = reinterpret_cast<uint8_t*>(b->mir_u8);
    HIPCHK(launch_mirror_u8(img_b, m, b->nframes, width_org, height_org, p.noc, s));
    if (int rc = build(m, &b->in_mir[0])) return rc;
    HIPCHK(launch_mirror_u8(img_a, m, b->nframes, width_org, height_org, p.noc, s));
    if (int rc = build(m, &b->in_mir[3])) return rc;
  }
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ results
const float* ofdis_batch_flow(const ofdis_batch* b) { return b ? b->flow[0] : nullptr; }
const float* ofdis_batch_level_flow(const ofdis_batch* b, int level) { return b ? level_flow(*b, level, false) : nullptr; }

int ofdis_batch_download(ofdis_batch* b, int frame, float* outflow_host, void* stream) {
  if (!b || frame < 0 || frame >= b->nframes || !outflow_host) return fail(OFDIS_ERR_INVALID, "bad arguments");
  return download(b, frame, outflow_host, (hipStream_t)stream, false);
}

// Warm start (oflow.cpp:217-220): the coarsest level initialises its patches from this flow exactly as finer levels
// do from the level above, i.e. it is indexed as a (w >> (sc_f+1)) x (h >> (sc_f+1)) AoS plane per frame.
size_t ofdis_batch_initflow_elems(const ofdis_batch* b) {
  if (!b) return 0;
  const LevelGeom& g = b->geom[b->nlevels - 1];
  return (size_t)(g.w / 2) * (g.h / 2) * b->nop;
}

int ofdis_batch_set_initflow(ofdis_batch* b, const float* initflow_dev) {
  if (!b) return fail(OFDIS_ERR_INVALID, "batch is NULL");
  b->initflow = initflow_dev;
  return OFDIS_OK;
}

int ofdis_batch_upload_initflow(ofdis_batch* b, int frame, const float* initflow_host, void* stream) {
  if (!b || frame < 0 || frame >= b->nframes || !initflow_host) return fail(OFDIS_ERR_INVALID, "bad arguments");
  const size_t n = ofdis_batch_initflow_elems(b);
  if (!b->initflow_own) {
    dalloc(b, &b->initflow_own, n);
    if (int rc = dcommit(b)) return rc;
    HIPCHK(hipMemsetAsync(b->initflow_own, 0, n * b->nframes * sizeof(float), (hipStream_t)stream));
  }
  HIPCHK(hipMemcpyAsync(frame_at(*b, b->initflow_own, frame), initflow_host, n * sizeof(float), hipMemcpyHostToDevice,
                        (hipStream_t)stream));
  b->initflow = b->initflow_own;
  return OFDIS_OK;
}

// What every full-resolution finish of a context starts with: the frame range and the original size checked, the pass joined
// (ofdis_batch_join), then the finish's geometry and where frames [first_frame, ...) start in a finest-level result array
// (flow[0], flow_rev[0]).
struct Finish {
  UpGeom g;
  size_t off;
};
static int finish_begin(ofdis_batch* b, int first_frame, int count, int width_org, int height_org, void* stream, Finish& fin) {
  if (first_frame < 0 || count < 1 || first_frame > b->nframes - count) return fail(OFDIS_ERR_INVALID, "frame range outside the batch");
  const ofdis_params& p = b->p;
  if (width_org < 1 || height_org < 1 || width_org > p.width || height_org > p.height)
    return fail(OFDIS_ERR_INVALID, "original size exceeds the padded size");
  if (int rc = ofdis_batch_join(b, stream)) return rc;
  const LevelGeom& g = b->geom[0];
  fin.g = UpGeom{g.w, g.h, p.sc_l, (p.width - width_org) / 2, (p.height - height_org) / 2, width_org, height_org};
  fin.off = (size_t)first_frame * frame_elems(*b, b->flow[0]);
  return OFDIS_OK;
}

int ofdis_batch_upsample_frames(ofdis_batch* b, int first_frame, int count, float* out_dev, int width_org,
                                int height_org, void* stream) {
  if (!b || !out_dev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_upsample_crop(b->flow[0] + fin.off, out_dev, count, fin.g, b->nop, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_upsample(ofdis_batch* b, float* out_dev, int width_org, int height_org, void* stream) {
  if (!b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  return ofdis_batch_upsample_frames(b, 0, b->nframes, out_dev, width_org, height_org, stream);
}

// ------------------------------------------------------------------------------------ compact output encodings
size_t ofdis_encoding_bytes(int type) {
  switch (type) {
    case OFDIS_ENC_F32: return 4;
    case OFDIS_ENC_F16: case OFDIS_ENC_U16: return 2;
    case OFDIS_ENC_U8: return 1;
  }
  return 0;
}

static int encoding_check(const ofdis_encoding* enc) {
  if (!enc) return fail(OFDIS_ERR_INVALID, "encoding is NULL");
  if (!ofdis_encoding_bytes(enc->type)) return fail(OFDIS_ERR_INVALID, "unknown encoding type");
  if (enc->type == OFDIS_ENC_U16 || enc->type == OFDIS_ENC_U8) {
    if (!std::isfinite(enc->scale) || enc->scale == 0.0f) return fail(OFDIS_ERR_INVALID, "encoding scale must be finite and not zero");
    if (!std::isfinite(enc->offset)) return fail(OFDIS_ERR_INVALID, "encoding offset must be finite");
  }
  return OFDIS_OK;
}

int ofdis_encode(const float* src, void* dst, size_t n, const ofdis_encoding* enc, void* stream) {
  if (!src || !dst) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if ((const void*)src == dst) return fail(OFDIS_ERR_INVALID, "ofdis_encode does not work in place");
  if (int rc = encoding_check(enc)) return rc;
  if (n == 0) return OFDIS_OK;
  HIPCHK(launch_encode(src, dst, n, enc->type, enc->scale, enc->offset, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_upsample_frames_enc(ofdis_batch* b, int first_frame, int count, void* out, int width_org, int height_org,
                                    const ofdis_encoding* enc, void* stream) {
  if (!b || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = encoding_check(enc)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_upsample_crop_enc(b->flow[0] + fin.off, out, count, fin.g, b->nop, enc->type, enc->scale, enc->offset,
                                  (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ reverse direction (OFDIS_BATCH_REVERSE)
const float* ofdis_batch_flow_reverse(const ofdis_batch* b) { return b && b->reverse ? b->flow_rev[0] : nullptr; }
const float* ofdis_batch_level_flow_reverse(const ofdis_batch* b, int level) {
  return b && b->reverse ? level_flow(*b, level, true) : nullptr;
}

int ofdis_batch_set_initflow_reverse(ofdis_batch* b, const float* initflow_dev) {
  if (!b || !b->reverse) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  b->initflow_rev = initflow_dev;
  return OFDIS_OK;
}

int ofdis_batch_download_reverse(ofdis_batch* b, int frame, float* outflow_host, void* stream) {
  if (!b || !b->reverse) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  if (frame < 0 || frame >= b->nframes || !outflow_host) return fail(OFDIS_ERR_INVALID, "bad arguments");
  return download(b, frame, outflow_host, (hipStream_t)stream, true);
}

int ofdis_batch_upsample_bidir(ofdis_batch* b, int first_frame, int count, float* out_fw, float* out_rev,
                               uint8_t* mask_fw, uint8_t* mask_rev, int width_org, int height_org,
                               float alpha, float beta, void* stream) {
  if (!b || !b->reverse) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!out_fw && !out_rev && !mask_fw && !mask_rev) return OFDIS_OK;
  HIPCHK(launch_upsample_bidir(b->flow[0] + fin.off, b->flow_rev[0] + fin.off, out_fw, out_rev, mask_fw, mask_rev, count, fin.g,
                               alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_fb_check(const float* flow, const float* flow_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream) {
  if (!flow || !flow_other || !mask) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (nframes < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  HIPCHK(launch_fb_check(flow, flow_other, mask, nframes, width, height, alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ stereo left-right (OFDIS_BATCH_STEREO_LR)
const float* ofdis_batch_flow_mirror(const ofdis_batch* b) { return b && b->stereo_lr ? b->flow_rev[0] : nullptr; }
const float* ofdis_batch_level_flow_mirror(const ofdis_batch* b, int level) {
  return b && b->stereo_lr ? level_flow(*b, level, true) : nullptr;
}

int ofdis_lr_check(const float* disp, const float* disp_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream) {
  if (!disp || !disp_other || !mask) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (nframes < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  HIPCHK(launch_lr_check(disp, disp_other, mask, nframes, width, height, alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

static bool fill_mode_ok(int mode) { return mode == OFDIS_FILL_NONE || mode == OFDIS_FILL_INVALIDATE || mode == OFDIS_FILL_BACKGROUND; }

int ofdis_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int width, int height, int mode,
                         void* stream) {
  if (!fill_mode_ok(mode)) return fail(OFDIS_ERR_INVALID, "fill mode must be OFDIS_FILL_NONE, _INVALIDATE or _BACKGROUND");
  if (!disp || !mask || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (nframes < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  HIPCHK(launch_disparity_fill(disp, mask, out, nframes, width, height, mode, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_upsample_lr(ofdis_batch* b, int first_frame, int count, float* out_left, float* out_right,
                            uint8_t* mask_left, uint8_t* mask_right, int fill_mode, int width_org, int height_org,
                            float alpha, float beta, void* stream) {
  if (!b || !b->stereo_lr) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_STEREO_LR");
  if (!fill_mode_ok(fill_mode)) return fail(OFDIS_ERR_INVALID, "fill mode must be OFDIS_FILL_NONE, _INVALIDATE or _BACKGROUND");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  hipStream_t s = (hipStream_t)stream;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!out_left && !out_right && !mask_left && !mask_right) return OFDIS_OK;
  const ofdis_params& p = b->p;
  const float* fw = b->flow[0] + fin.off;
  const float* mir = b->flow_rev[0] + fin.off;
  if (upsample_lr_fuses(width_org)) {
    HIPCHK(launch_upsample_lr(fw, mir, out_left, out_right, mask_left, mask_right, count, fin.g, fill_mode, alpha, beta, s));
    return OFDIS_OK;
  }
  // wider than the fused kernel's rows: the composition itself, through staging owned by the context
  const size_t px = (size_t)p.width * p.height;
  if (!b->lr_u) {
    dalloc(b, &b->lr_u, px, false);
    dalloc(b, &b->lr_dr, px, false);
    dalloc(b, &b->lr_mask, (2 * px + 3) / 4, false);
    if (int rc = dcommit(b)) return rc;
  }
  const size_t n = (size_t)count * width_org * height_org;  // (count <= nframes, original size <= padded size)
  uint8_t* ml = mask_left ? mask_left : reinterpret_cast<uint8_t*>(b->lr_mask);
  uint8_t* mr = mask_right ? mask_right : reinterpret_cast<uint8_t*>(b->lr_mask) + n;
  HIPCHK(launch_lr_materialise(fw, mir, b->lr_u, b->lr_dr, count, fin.g, s));
  if (mask_left || out_left) HIPCHK(launch_lr_check(b->lr_u, b->lr_dr, ml, count, width_org, height_org, alpha, beta, s));
  if (mask_right || out_right) HIPCHK(launch_lr_check(b->lr_dr, b->lr_u, mr, count, width_org, height_org, alpha, beta, s));
  if (out_left) HIPCHK(launch_disparity_fill(b->lr_u, ml, out_left, count, width_org, height_org, fill_mode, s));
  if (out_right) HIPCHK(launch_disparity_fill(b->lr_dr, mr, out_right, count, width_org, height_org, fill_mode, s));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ frame interpolation (ofdis_interp.hip)
int ofdis_interpolate(const uint8_t* img_a, const uint8_t* img_b, const float* flow_fw, const float* flow_rev,
                      const uint8_t* mask_fw, const uint8_t* mask_rev, uint8_t* out, int nframes, int width, int height,
                      int noc, const float* times, int ntimes, void* stream) {
  if (!img_a || !img_b || !flow_fw || !flow_rev || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  InterpTimes ts;
  if (int rc = interp_times(times, ntimes, ts)) return rc;
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (nframes < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  HIPCHK(launch_interp_frames(img_a, img_b, flow_fw, flow_rev, mask_fw, mask_rev, out, nframes, width, height, noc, ts,
                              (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_interpolate(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int first_frame, int count,
                            const float* times, int ntimes, uint8_t* out, int width_org, int height_org,
                            float alpha, float beta, void* stream) {
  if (!b || !b->reverse) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  if (!img_a || !img_b || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  InterpTimes ts;
  if (int rc = interp_times(times, ntimes, ts)) return rc;
  const ofdis_params& p = b->p;
  if (p.noc != 1 && p.noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  const size_t img_off = (size_t)first_frame * width_org * height_org * p.noc;
  HIPCHK(launch_interp_bidir(img_a + img_off, img_b + img_off, b->flow[0] + fin.off, b->flow_rev[0] + fin.off, out, count, fin.g,
                             p.noc, ts, alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ point trajectories (ofdis_track.hip)
static int track_args_check(const float* seeds, int npoints, int max_steps, float alpha, float beta, const float* tracks) {
  if (!seeds || !tracks) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (npoints < 1 || npoints > OFDIS_TRACK_MAX_POINTS) return fail(OFDIS_ERR_INVALID, "npoints outside 1..OFDIS_TRACK_MAX_POINTS");
  if (max_steps < 0) return fail(OFDIS_ERR_INVALID, "max_steps is negative");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  return OFDIS_OK;
}

int ofdis_track_points(const float* flow_fw, const float* flow_rev, int npairs, int width, int height, const float* seeds,
                       const int* seed_frame, int npoints, int max_steps, float alpha, float beta, float* tracks, int* counts,
                       void* stream) {
  if (!flow_fw) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = track_args_check(seeds, npoints, max_steps, alpha, beta, tracks)) return rc;
  if (npairs < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  HIPCHK(launch_track_points(flow_fw, flow_rev, npairs, width, height, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks,
                             counts, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_track_points(ofdis_batch* b, int first_frame, int count, const float* seeds, const int* seed_frame, int npoints,
                             int max_steps, int fb_check, float alpha, float beta, float* tracks, int* counts, int width_org,
                             int height_org, void* stream) {
  if (!b || !b->sequence)  // (the pairs of any other context are no chain)
    return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_SEQUENCE");
  if (fb_check != 0 && fb_check != 1) return fail(OFDIS_ERR_INVALID, "fb_check must be 0 or 1");
  if (fb_check && !b->reverse) return fail(OFDIS_ERR_INVALID, "fb_check needs a context created with OFDIS_BATCH_REVERSE");
  if (int rc = track_args_check(seeds, npoints, max_steps, alpha, beta, tracks)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_track_level(b->flow[0] + fin.off, fb_check ? b->flow_rev[0] + fin.off : nullptr, count, fin.g, seeds, seed_frame,
                            npoints, max_steps, alpha, beta, tracks, counts, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ dense trajectories (ofdis_dense_tracks.hip)
static int dense_grid_check(int width, int height, int stride) {
  if (stride < 2 || stride > OFDIS_DT_MAX_STRIDE) return fail(OFDIS_ERR_INVALID, "stride outside 2..OFDIS_DT_MAX_STRIDE");
  if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail(OFDIS_ERR_INVALID, "bad sizes");
  if (width < stride || height < stride) return fail(OFDIS_ERR_INVALID, "bad sizes (a side smaller than the stride)");
  return OFDIS_OK;
}
static int dense_texture_check(const uint8_t* frames, int noc, int window, int min_eig) {
  if (!frames) return fail(OFDIS_ERR_INVALID, "frames is NULL");
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (window < 0 || window > OFDIS_DT_MAX_WINDOW) return fail(OFDIS_ERR_INVALID, "window outside 0..OFDIS_DT_MAX_WINDOW");
  if (min_eig < 0) return fail(OFDIS_ERR_INVALID, "min_eig is negative");
  return OFDIS_OK;
}
static int dense_args_check(const uint8_t* frames, int noc, int window, int min_eig, int max_len, float alpha, float beta,
                            int max_tracks, const float* tracks, const int* start, const long long* info) {
  if (int rc = dense_texture_check(frames, noc, window, min_eig)) return rc;
  if (!tracks || !start || !info) return fail(OFDIS_ERR_INVALID, "tracks, start or info is NULL");
  if (max_len < 0) return fail(OFDIS_ERR_INVALID, "max_len is negative");
  if (max_tracks < 1 || max_tracks > OFDIS_DT_MAX_TRACKS) return fail(OFDIS_ERR_INVALID, "max_tracks outside 1..OFDIS_DT_MAX_TRACKS");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  return OFDIS_OK;
}

int ofdis_dense_tracks_cells(int width, int height, int stride, int* ncx, int* ncy) {
  if (ncx) *ncx = 0;
  if (ncy) *ncy = 0;
  if (dense_grid_check(width, height, stride)) return 0;
  return dense_tracks_cells(width, height, stride, ncx, ncy);
}

size_t ofdis_dense_tracks_work_bytes(int npairs, int width, int height, int stride) {
  if (npairs < 1 || dense_grid_check(width, height, stride)) return 0;
  return dense_tracks_work_bytes(npairs, width, height, stride, 0, OFDIS_DT_MAX_TRACKS);
}

int ofdis_seed_texture(const uint8_t* frames, int nframes, int width, int height, int noc, int stride, int window, int min_eig,
                       uint8_t* out, void* stream) {
  if (int rc = dense_texture_check(frames, noc, window, min_eig)) return rc;
  if (!out) return fail(OFDIS_ERR_INVALID, "out is NULL");
  if (int rc = dense_grid_check(width, height, stride)) return rc;
  if (nframes < 1) return fail(OFDIS_ERR_INVALID, "bad sizes (nframes < 1)");
  HIPCHK(launch_seed_texture(frames, nframes, width, height, noc, stride, window, min_eig, out, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_dense_tracks(const uint8_t* frames, const float* flow_fw, const float* flow_rev, int npairs, int width, int height,
                       int noc, int stride, int window, int min_eig, int max_len, float alpha, float beta, int max_tracks,
                       float* tracks, int* start, int* len, long long* info, void* work, size_t work_bytes, void* stream) {
  if (!flow_fw) return fail(OFDIS_ERR_INVALID, "flow_fw is NULL");
  if (int rc = dense_args_check(frames, noc, window, min_eig, max_len, alpha, beta, max_tracks, tracks, start, info)) return rc;
  if (int rc = dense_grid_check(width, height, stride)) return rc;
  if (npairs < 1) return fail(OFDIS_ERR_INVALID, "bad sizes (npairs < 1)");
  if (!work || ((uintptr_t)work & 7) || work_bytes < ofdis_dense_tracks_work_bytes(npairs, width, height, stride))
    return fail(OFDIS_ERR_INVALID, "work buffer is NULL, not 8-byte aligned or smaller than ofdis_dense_tracks_work_bytes");
  HIPCHK(launch_dense_tracks(frames, flow_fw, flow_rev, npairs, width, height, noc, stride, window, min_eig, max_len, alpha, beta,
                             max_tracks, tracks, start, len, info, work, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_dense_tracks(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int stride, int window,
                             int min_eig, int max_len, int fb_check, float alpha, float beta, int max_tracks, float* tracks,
                             int* start, int* len, long long* info, int width_org, int height_org, void* stream) {
  if (!b || !b->sequence)  // (the pairs of any other context are no chain)
    return fail(OFDIS_ERR_INVALID, kSeqOnly);
  if (fb_check != 0 && fb_check != 1) return fail(OFDIS_ERR_INVALID, "fb_check must be 0 or 1");
  if (fb_check && !b->reverse) return fail(OFDIS_ERR_INVALID, "fb_check needs a context created with OFDIS_BATCH_REVERSE");
  const ofdis_params& p = b->p;
  if (int rc = dense_args_check(frames, p.noc, window, min_eig, max_len, alpha, beta, max_tracks, tracks, start, info)) return rc;
  if (int rc = dense_grid_check(width_org, height_org, stride)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  const size_t need = dense_tracks_work_bytes(count, width_org, height_org, stride, max_len, max_tracks);
  if (need > b->dt_slab_bytes) {  // what this call needs; an earlier, smaller buffer stays with the context until it is destroyed
    const size_t per_frame = (need + sizeof(float) * b->nframes - 1) / (sizeof(float) * b->nframes);
    b->dt_slab_bytes = 0;
    dalloc(b, &b->dt_slab, per_frame, false);
    if (int rc = dcommit(b)) return rc;
    b->dt_slab_bytes = per_frame * b->nframes * sizeof(float);
  }
  HIPCHK(launch_dense_tracks_level(frames + (size_t)first_frame * width_org * height_org * p.noc, b->flow[0] + fin.off,
                                   fb_check ? b->flow_rev[0] + fin.off : nullptr, count, fin.g, p.noc, stride, window, min_eig,
                                   max_len, alpha, beta, max_tracks, tracks, start, len, info, b->dt_slab, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ track descriptors (ofdis_descriptors.hip)
static int desc_params_check(int patch, int nxy, int nt) {
  if (patch < 2 || patch > OFDIS_DESC_MAX_PATCH || patch % 2) return fail(OFDIS_ERR_INVALID, "patch must be even, 2..OFDIS_DESC_MAX_PATCH");
  if (nxy < 1 || nxy > 4 || patch % nxy) return fail(OFDIS_ERR_INVALID, "nxy must be 1..4 and divide patch");
  if (nt < 1 || nt > 8) return fail(OFDIS_ERR_INVALID, "nt outside 1..8");
  return OFDIS_OK;
}

int ofdis_track_descriptor_dims(int patch, int nxy, int nt) { return desc_params_check(patch, nxy, nt) ? 0 : 33 * nxy * nxy * nt; }

int ofdis_track_descriptors(const uint8_t* frames, const float* flow_fw, int npairs, int width, int height, int noc,
                            const float* tracks, const int* start, const int* len, const long long* info, int lmax,
                            int max_tracks, int patch, int nxy, int nt, float min_flow, uint32_t* hist, float* shape,
                            void* stream) {
  if (!frames) return fail(OFDIS_ERR_INVALID, "frames is NULL");
  if (!flow_fw) return fail(OFDIS_ERR_INVALID, "flow_fw is NULL");
  if (!tracks || !start || !len || !info) return fail(OFDIS_ERR_INVALID, "tracks, start, len or info is NULL");
  if (!hist) return fail(OFDIS_ERR_INVALID, "hist is NULL");
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail(OFDIS_ERR_INVALID, "bad sizes");
  if (npairs < 1) return fail(OFDIS_ERR_INVALID, "bad sizes (npairs < 1)");
  if (lmax < 1 || lmax > npairs) return fail(OFDIS_ERR_INVALID, "lmax outside 1..npairs");
  if (max_tracks < 1 || max_tracks > OFDIS_DT_MAX_TRACKS) return fail(OFDIS_ERR_INVALID, "max_tracks outside 1..OFDIS_DT_MAX_TRACKS");
  if (int rc = desc_params_check(patch, nxy, nt)) return rc;
  if (nt > lmax) return fail(OFDIS_ERR_INVALID, "nt above lmax");
  if ((long long)patch * patch * lmax > 65536) return fail(OFDIS_ERR_INVALID, "patch * patch * lmax above 65536");
  if (!(min_flow >= 0.f) || std::isinf(min_flow)) return fail(OFDIS_ERR_INVALID, "min_flow must be finite and >= 0");
  HIPCHK(launch_track_descriptors(frames, flow_fw, npairs, width, height, noc, tracks, start, len, info, lmax, max_tracks, patch,
                                  nxy, nt, min_flow, hist, shape, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ temporal filter (ofdis_tfilter.hip)
static int tfilter_args_check(const uint8_t* frames, const uint8_t* out, int noc, float wn, float tau) {
  if (!frames || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (out == frames) return fail(OFDIS_ERR_INVALID, "the temporal filter does not work in place");
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (!(wn >= 0.0f && wn <= 1.0f)) return fail(OFDIS_ERR_INVALID, "wn must be inside [0, 1]");
  if (!(tau >= FLT_MIN)) return fail(OFDIS_ERR_INVALID, "tau must be +inf or a positive float that is not subnormal");
  return OFDIS_OK;
}

int ofdis_temporal_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                          const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int width, int height, int noc,
                          float wn, float tau, void* stream) {
  if (!flow_fw || !flow_rev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = tfilter_args_check(frames, out, noc, wn, tau)) return rc;
  if (npairs < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  HIPCHK(launch_tfilter_frames(frames, flow_fw, flow_rev, mask_fw, mask_rev, out, support, npairs, width, height, noc, wn, tau,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_temporal_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                uint8_t* support, int width_org, int height_org, float wn, float tau, float alpha, float beta,
                                void* stream) {
  if (!b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (!b->sequence)  // (the pairs of any other context share no frames)
    return fail(OFDIS_ERR_INVALID, b->reverse ? "not a context created with OFDIS_BATCH_SEQUENCE"
                                              : "not a context created with OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE");
  if (!b->reverse) return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  const ofdis_params& p = b->p;
  if (int rc = tfilter_args_check(frames, out, p.noc, wn, tau)) return rc;
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_tfilter_level(frames + (size_t)first_frame * width_org * height_org * p.noc, b->flow[0] + fin.off,
                              b->flow_rev[0] + fin.off, out, support, count, fin.g, p.noc, wn, tau, alpha, beta,
                              (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ trajectory filter (ofdis_trajfilter.hip)
static_assert(sizeof(TrajWeights::w) / sizeof(float) == OFDIS_TRAJ_MAX_RADIUS, "TrajWeights holds OFDIS_TRAJ_MAX_RADIUS");
static int trajfilter_args_check(const uint8_t* frames, const uint8_t* out, int noc, const float* weights, int radius, float tau,
                                 int fb_check, float alpha, float beta, TrajWeights& tw) {
  if (!frames || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (out == frames) return fail(OFDIS_ERR_INVALID, "the trajectory filter does not work in place");
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (!weights) return fail(OFDIS_ERR_INVALID, "weights is NULL");
  if (radius < 1 || radius > OFDIS_TRAJ_MAX_RADIUS) return fail(OFDIS_ERR_INVALID, "radius must be 1..OFDIS_TRAJ_MAX_RADIUS");
  memset(&tw, 0, sizeof(tw));
  for (int j = 0; j < radius; ++j) {
    if (!(weights[j] >= 0.0f && weights[j] <= 1.0f)) return fail(OFDIS_ERR_INVALID, "every weight must be inside [0, 1]");
    tw.w[j] = weights[j];
  }
  tw.radius = radius;
  if (!(tau >= FLT_MIN)) return fail(OFDIS_ERR_INVALID, "tau must be +inf or a positive float that is not subnormal");
  if (fb_check != 0 && fb_check != 1) return fail(OFDIS_ERR_INVALID, "fb_check must be 0 or 1");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  return OFDIS_OK;
}

int ofdis_trajectory_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out, uint8_t* support,
                            int npairs, int width, int height, int noc, const float* weights, int radius, float tau,
                            int fb_check, float alpha, float beta, void* stream) {
  if (!flow_fw || !flow_rev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  TrajWeights tw;
  if (int rc = trajfilter_args_check(frames, out, noc, weights, radius, tau, fb_check, alpha, beta, tw)) return rc;
  if (npairs < 1 || width < 1 || height < 1 || (long long)width * height > (1ll << 30))
    return fail(OFDIS_ERR_INVALID, "bad sizes");
  HIPCHK(launch_trajfilter_frames(frames, flow_fw, flow_rev, out, support, npairs, width, height, noc, tw, tau, fb_check != 0,
                                  alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_trajectory_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                  uint8_t* support, int width_org, int height_org, const float* weights, int radius, float tau,
                                  int fb_check, float alpha, float beta, void* stream) {
  if (!b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (!b->sequence)  // (the pairs of any other context share no frames)
    return fail(OFDIS_ERR_INVALID, b->reverse ? "not a context created with OFDIS_BATCH_SEQUENCE"
                                              : "not a context created with OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE");
  if (!b->reverse)  // (whatever fb_check is: walking back takes the reverse flows)
    return fail(OFDIS_ERR_INVALID, "not a context created with OFDIS_BATCH_REVERSE");
  const ofdis_params& p = b->p;
  TrajWeights tw;
  if (int rc = trajfilter_args_check(frames, out, p.noc, weights, radius, tau, fb_check, alpha, beta, tw)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_trajfilter_level(frames + (size_t)first_frame * width_org * height_org * p.noc, b->flow[0] + fin.off,
                                 b->flow_rev[0] + fin.off, out, support, count, fin.g, p.noc, tw, tau, fb_check != 0, alpha, beta,
                                 (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ global motion (ofdis_gmotion.hip)
static bool gm_sizes_ok(int npairs, int width, int height) {
  return npairs >= 1 && width >= 1 && height >= 1 && width <= OFDIS_GM_MAX_SIDE && height <= OFDIS_GM_MAX_SIDE;
}
static int gm_thresh_check(float thresh) {
  if (!(std::isfinite(thresh) && thresh > 0.0f)) return fail(OFDIS_ERR_INVALID, "thresh must be finite and > 0");
  return OFDIS_OK;
}
static int gm_fit_check(int model, int rounds, float thresh) {
  if (model != OFDIS_GM_TRANSLATION_ONLY && model != OFDIS_GM_AFFINE)
    return fail(OFDIS_ERR_INVALID, "model must be OFDIS_GM_TRANSLATION_ONLY or OFDIS_GM_AFFINE");
  if (rounds < 1 || rounds > OFDIS_GM_MAX_ROUNDS) return fail(OFDIS_ERR_INVALID, "rounds outside 1..OFDIS_GM_MAX_ROUNDS");
  return gm_thresh_check(thresh);
}
static const char* const kGmSizes = "bad sizes (a side above OFDIS_GM_MAX_SIDE?)";
// what both batch calls check about the context and the mask they are asked for
static int gm_batch_check(const ofdis_batch* b, int fb_check, float alpha, float beta, int width_org, int height_org) {
  if (!b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (b->p.selectmode == 2) return fail(OFDIS_ERR_INVALID, "not an optical-flow context (stereo-depth mode has no flow field)");
  if (fb_check != 0 && fb_check != 1) return fail(OFDIS_ERR_INVALID, "fb_check must be 0 or 1");
  if (fb_check && !b->reverse) return fail(OFDIS_ERR_INVALID, "fb_check needs a context created with OFDIS_BATCH_REVERSE");
  if (!fb_constants_ok(alpha, beta)) return fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
  if (width_org > OFDIS_GM_MAX_SIDE || height_org > OFDIS_GM_MAX_SIDE) return fail(OFDIS_ERR_INVALID, kGmSizes);
  return OFDIS_OK;
}

size_t ofdis_global_motion_work_bytes(int npairs, int width, int height) {
  return gm_sizes_ok(npairs, width, height) ? gmotion_work_bytes(npairs, width, height) : 0;
}

int ofdis_global_motion(const float* flow, const uint8_t* mask, int npairs, int width, int height, int model, int rounds,
                        float thresh, double* models, long long* stats, void* work, size_t work_bytes, void* stream) {
  if (!flow || !models) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  if (!gm_sizes_ok(npairs, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  if (!work || ((uintptr_t)work & 7) || work_bytes < gmotion_work_bytes(npairs, width, height))
    return fail(OFDIS_ERR_INVALID, "work buffer is NULL, not 8-byte aligned or smaller than ofdis_global_motion_work_bytes");
  HIPCHK(launch_gmotion_frames(flow, mask, npairs, width, height, model, rounds, thresh, models, stats, work,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_motion_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                            float thresh, float* residual, uint8_t* label, void* stream) {
  if (!flow || !models || (!residual && !label)) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_thresh_check(thresh)) return rc;
  if (!gm_sizes_ok(npairs, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  HIPCHK(launch_gmotion_compensate_frames(flow, mask, models, npairs, width, height, thresh, residual, label,
                                          (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_global_motion(ofdis_batch* b, int first_frame, int count, int model, int rounds, float thresh, int fb_check,
                              float alpha, float beta, double* models, long long* stats, int width_org, int height_org,
                              void* stream) {
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org)) return rc;
  if (!models) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!b->gm_slab) {  // records for every pair at the padded size (no original size needs more), held as floats
    dalloc(b, &b->gm_slab, gmotion_work_bytes(1, std::min(b->p.width, OFDIS_GM_MAX_SIDE), std::min(b->p.height, OFDIS_GM_MAX_SIDE)) /
                               sizeof(float), false);
    if (int rc = dcommit(b)) return rc;
  }
  HIPCHK(launch_gmotion_level(b->flow[0] + fin.off, fb_check ? b->flow_rev[0] + fin.off : nullptr, count, fin.g, model, rounds,
                              thresh, alpha, beta, models, stats, b->gm_slab, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_motion_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh, int fb_check,
                                  float alpha, float beta, float* residual, uint8_t* label, int width_org, int height_org,
                                  void* stream) {
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org)) return rc;
  if (!models || (!residual && !label)) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_thresh_check(thresh)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_gmotion_compensate_level(b->flow[0] + fin.off, fb_check ? b->flow_rev[0] + fin.off : nullptr, models, count, fin.g,
                                         thresh, alpha, beta, residual, label, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ video stabilisation (ofdis_stabilize.hip)
static_assert(sizeof(StabWindow::w) / sizeof(double) == OFDIS_STAB_MAX_RADIUS + 1, "StabWindow holds OFDIS_STAB_MAX_RADIUS + 1 weights");
static int stab_window(const double* weights, int radius, double zoom, StabWindow& win) {
  if (!weights) return fail(OFDIS_ERR_INVALID, "weights is NULL");
  if (radius < 0 || radius > OFDIS_STAB_MAX_RADIUS) return fail(OFDIS_ERR_INVALID, "radius outside 0..OFDIS_STAB_MAX_RADIUS");
  memset(&win, 0, sizeof(win));
  for (int j = 0; j <= radius; ++j) {
    if (!(std::isfinite(weights[j]) && weights[j] >= 0.0 && (j > 0 || weights[j] > 0.0)))
      return fail(OFDIS_ERR_INVALID, "weights must be finite, w_0 > 0 and the others >= 0");
    win.w[j] = weights[j];
  }
  if (!(std::isfinite(zoom) && zoom >= 1.0 && zoom <= OFDIS_STAB_MAX_ZOOM))
    return fail(OFDIS_ERR_INVALID, "zoom must be inside [1, OFDIS_STAB_MAX_ZOOM]");
  win.zoom = zoom;
  win.radius = radius;
  return OFDIS_OK;
}
static int stab_warp_check(const uint8_t* frames, const uint8_t* out, int noc, int border) {
  if (!frames || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (out == frames) return fail(OFDIS_ERR_INVALID, "the frame warp does not work in place");
  if (noc != 1 && noc != 3) return fail(OFDIS_ERR_INVALID, "noc must be 1 or 3");
  if (border != OFDIS_BORDER_CONSTANT && border != OFDIS_BORDER_REPLICATE)
    return fail(OFDIS_ERR_INVALID, "border must be OFDIS_BORDER_CONSTANT or OFDIS_BORDER_REPLICATE");
  return OFDIS_OK;
}

int ofdis_camera_path(const double* models, int npairs, const double* weights, int radius, double zoom, double* warps,
                      void* stream) {
  if (!models || !warps) return fail(OFDIS_ERR_INVALID, "bad arguments");
  StabWindow win;
  if (int rc = stab_window(weights, radius, zoom, win)) return rc;
  if (npairs < 1) return fail(OFDIS_ERR_INVALID, "bad sizes (npairs < 1)");
  HIPCHK(launch_camera_path(models, npairs, win, warps, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_warp_frames(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int width,
                      int height, int noc, int border, void* stream) {
  if (!warps) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = stab_warp_check(frames, out, noc, border)) return rc;
  if (!gm_sizes_ok(nframes, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  HIPCHK(launch_warp_frames(frames, warps, out, inside, nframes, width, height, noc, border == OFDIS_BORDER_REPLICATE,
                            (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_stabilize(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int model, int rounds, float thresh,
                          int fb_check, float alpha, float beta, const double* weights, int radius, double zoom, int border,
                          uint8_t* out, uint8_t* inside, double* warps, int width_org, int height_org, void* stream) {
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org)) return rc;
  if (!b->sequence) return fail(OFDIS_ERR_INVALID, kSeqOnly);  // (the pairs of any other context are no chain)
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  StabWindow win;
  if (int rc = stab_window(weights, radius, zoom, win)) return rc;
  const ofdis_params& p = b->p;
  if (int rc = stab_warp_check(frames, out, p.noc, border)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!b->stab_path) {  // 6 + 6 doubles per pair and 6 more for the last frame, held as floats
    dalloc(b, &b->stab_path, 24, false, 1);
    if (int rc = dcommit(b)) return rc;
  }
  double* models = reinterpret_cast<double*>(b->stab_path);
  double* path = models + (size_t)b->nframes * 6;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = ofdis_batch_global_motion(b, first_frame, count, model, rounds, thresh, fb_check, alpha, beta, models, nullptr,
                                         width_org, height_org, stream))
    return rc;
  HIPCHK(launch_camera_path(models, count, win, path, s));
  HIPCHK(launch_warp_frames(frames + (size_t)first_frame * width_org * height_org * p.noc, path, out, inside, count + 1, width_org,
                            height_org, p.noc, border == OFDIS_BORDER_REPLICATE, s));
  if (warps) HIPCHK(hipMemcpyAsync(warps, path, (size_t)(count + 1) * 6 * sizeof(double), hipMemcpyDeviceToDevice, s));
  return OFDIS_OK;
}

}  // extern "C"
