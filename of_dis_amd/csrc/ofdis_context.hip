// ofdis_context.hip -- the batch context's own half of the C ABI of include/ofdis.h: kernel-selection knobs, parameter
// handling, the context's device memory (array descriptions, frame views, staging made on first use), creation, inputs and the
// result accessors of all three directions.  What is made from the results is ofdis_products.hip.
#include "ofdis_context.h"

using namespace ofdis;

namespace ofdis {

template <int CONTRACT>
static constexpr Launchers launcher_table() {
  Launchers t{};
#define OFDIS_LAUNCHER_ENTRY(member, function)                         \
  if constexpr (CONTRACT) t.member = fused::function;                  \
  else t.member = exact::function;
  OFDIS_LAUNCHERS(OFDIS_LAUNCHER_ENTRY)
#undef OFDIS_LAUNCHER_ENTRY
  return t;
}
constexpr Launchers kExactLaunchers = launcher_table<0>();
constexpr Launchers kFusedLaunchers = launcher_table<1>();
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
  g_tuning.patch_window_reuse = !on("OFDIS_NO_PATCH_WINDOW_REUSE");
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
// Staging the context makes on first use (never seen by a frame view): every member of `wants` holds at least its floats per
// frame afterwards.  One that is null or smaller is requested anew and the requests are served together (one allocation).
// The buffer a member outgrows stays with the context until destroy, and in ofdis_batch_device_bytes: its description
// moves to `retired`, so that the member keeps exactly one.
int dstage(ofdis_batch* b, const std::vector<Stage>& wants) {
  for (const Stage& w : wants) {
    const size_t slot = (size_t)((char*)w.member - (char*)b);
    auto have = std::find_if(b->arrays.begin(), b->arrays.end(), [&](const ofdis_batch::Array& a) { return a.slot == slot; });
    if (have != b->arrays.end() && have->per_frame >= w.per_frame) continue;
    if (have != b->arrays.end()) have->slot = (size_t)((char*)&b->retired - (char*)b);
    dalloc(b, w.member, w.per_frame, false, w.extra_frames);
  }
  return dcommit(b);
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

// What a call needs of its context: creation flags (OFDIS_BATCH_*) and / or kOpticalFlow.  The message names what is missing; a
// NULL context has none of it.
int context_check(const ofdis_batch* b, unsigned needs) {
  if ((needs & kOpticalFlow) && (!b || b->p.selectmode == 2))
    return fail(OFDIS_ERR_INVALID, "not an optical-flow context (stereo-depth mode has no flow field)");
  std::string missing;
  auto need = [&](unsigned flag, bool has, const char* name) {
    if ((needs & flag) && !has) missing += (missing.empty() ? "" : " | ") + std::string(name);
  };
  need(OFDIS_BATCH_SEQUENCE, b && b->sequence, "OFDIS_BATCH_SEQUENCE");
  need(OFDIS_BATCH_REVERSE, b && b->reverse, "OFDIS_BATCH_REVERSE");
  need(OFDIS_BATCH_STEREO_LR, b && b->stereo_lr, "OFDIS_BATCH_STEREO_LR");
  return missing.empty() ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "not a context created with " + missing);
}
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
  if (in->patch_window_reuse != 0 && in->patch_window_reuse != 1) return fail(OFDIS_ERR_INVALID, "patch_window_reuse must be 0 or 1");
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
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE)) return rc;
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
  std::vector<Stage> tmp;
  for (int i = 0; i < b->nlevels; ++i)
    tmp.push_back({&b->pyr_tmp[i], (size_t)b->geom[i].w * b->geom[i].h * b->geom[i].noc, b->sequence ? 1 : 0});
  if (b->stereo_lr) tmp.push_back({&b->mir_u8, ((size_t)p.width * p.height * p.noc + 3) / 4});
  return dstage(b, tmp);
}

int ofdis_batch_build_pyramids_u8_seq(ofdis_batch* b, const uint8_t* frames, size_t row_pitch, size_t frame_stride,
                                      int width_org, int height_org, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE)) return rc;
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

// the reverse direction (OFDIS_BATCH_REVERSE)
const float* ofdis_batch_flow_reverse(const ofdis_batch* b) { return b && b->reverse ? b->flow_rev[0] : nullptr; }
const float* ofdis_batch_level_flow_reverse(const ofdis_batch* b, int level) {
  return b && b->reverse ? level_flow(*b, level, true) : nullptr;
}

int ofdis_batch_download_reverse(ofdis_batch* b, int frame, float* outflow_host, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_REVERSE)) return rc;
  if (frame < 0 || frame >= b->nframes || !outflow_host) return fail(OFDIS_ERR_INVALID, "bad arguments");
  return download(b, frame, outflow_host, (hipStream_t)stream, true);
}

// the mirror pass (OFDIS_BATCH_STEREO_LR)
const float* ofdis_batch_flow_mirror(const ofdis_batch* b) { return b && b->stereo_lr ? b->flow_rev[0] : nullptr; }
const float* ofdis_batch_level_flow_mirror(const ofdis_batch* b, int level) {
  return b && b->stereo_lr ? level_flow(*b, level, true) : nullptr;
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
int ofdis_batch_set_initflow_reverse(ofdis_batch* b, const float* initflow_dev) {
  if (int rc = context_check(b, OFDIS_BATCH_REVERSE)) return rc;
  b->initflow_rev = initflow_dev;
  return OFDIS_OK;
}

int ofdis_batch_upload_initflow(ofdis_batch* b, int frame, const float* initflow_host, void* stream) {
  if (!b || frame < 0 || frame >= b->nframes || !initflow_host) return fail(OFDIS_ERR_INVALID, "bad arguments");
  const size_t n = ofdis_batch_initflow_elems(b);
  const bool first_use = !b->initflow_own;
  if (int rc = dstage(b, {{&b->initflow_own, n}})) return rc;
  if (first_use) HIPCHK(hipMemsetAsync(b->initflow_own, 0, n * b->nframes * sizeof(float), (hipStream_t)stream));
  HIPCHK(hipMemcpyAsync(frame_at(*b, b->initflow_own, frame), initflow_host, n * sizeof(float), hipMemcpyHostToDevice,
                        (hipStream_t)stream));
  b->initflow = b->initflow_own;
  return OFDIS_OK;
}

}  // extern "C"
