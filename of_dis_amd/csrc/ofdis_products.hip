// ofdis_products.hip -- what is made from a context's flows, and the same steps on caller-supplied arrays: the full-resolution
// finish and its encodings, forward-backward and left-right checks, interpolation, point and dense trajectories, their selection, descriptors,
// their bag-of-features encoding and the training of its codebook, the temporal filters, global motion, the segments of its label maps, their tracks and stabilisation.
// Every entry point validates its arguments, joins the pass (finish_begin) and launches; the checks they share are stated once, below.  Reads no environment.
#include <cfloat>
#include <cmath>

#include "ofdis_context.h"

using namespace ofdis;

namespace ofdis {

// ------------------------------------------------------------------------------------ the shared checks
static int sizes_check(int n, int width, int height) {
  const bool ok = n >= 1 && width >= 1 && height >= 1 && (long long)width * height <= (1ll << 30);
  return ok ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "bad sizes");
}
static int noc_check(int noc) { return noc == 1 || noc == 3 ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "noc must be 1 or 3"); }
static int fb_constants_check(float alpha, float beta) {
  const bool ok = std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f;
  return ok ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "alpha and beta must be finite and >= 0");
}
static int fb_flag_check(int fb_check) {
  return fb_check == 0 || fb_check == 1 ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "fb_check must be 0 or 1");
}
// A caller-supplied work buffer of at least `need` bytes, which the caller learns from the function named `bytes_fn`
static int work_check(const void* work, size_t work_bytes, size_t need, const char* bytes_fn) {
  if (work && !((uintptr_t)work & 7) && work_bytes >= need) return OFDIS_OK;
  return fail(OFDIS_ERR_INVALID, std::string("work buffer is NULL, not 8-byte aligned or smaller than ") + bytes_fn);
}

// A full-resolution finish of a context.  finish_begin: the frame range and the original size checked, the pass joined
// (ofdis_batch_join), then the finish's geometry and its operands: where frames [first_frame, ...) start in the finest-level
// results and in a packed 8-bit clip of the original size and the context's channel count.
struct Finish {
  bool fb = false;  // the call asked for the consistency test (fb_check_arg, before finish_begin)
  UpGeom g;
  const float *fw, *rev;  // flow[0], flow_rev[0] (null on a context without a second direction) ...
  const float* fb_rev;    // ... and the reverse flow to test against: rev if asked for, else null
  size_t clip_off;
  const uint8_t* clip(const uint8_t* frames) const { return frames + clip_off; }
};
// the fb_check argument of the batch forms: 0 or 1, and 1 needs the reverse flows
static int fb_check_arg(const ofdis_batch* b, int fb_check, Finish& fin) {
  if (int rc = fb_flag_check(fb_check)) return rc;
  if (fb_check && !b->reverse) return fail(OFDIS_ERR_INVALID, "fb_check needs a context created with OFDIS_BATCH_REVERSE");
  fin.fb = fb_check != 0;
  return OFDIS_OK;
}
static int finish_begin(ofdis_batch* b, int first_frame, int count, int width_org, int height_org, void* stream, Finish& fin) {
  if (first_frame < 0 || count < 1 || first_frame > b->nframes - count) return fail(OFDIS_ERR_INVALID, "frame range outside the batch");
  const ofdis_params& p = b->p;
  if (width_org < 1 || height_org < 1 || width_org > p.width || height_org > p.height)
    return fail(OFDIS_ERR_INVALID, "original size exceeds the padded size");
  if (int rc = ofdis_batch_join(b, stream)) return rc;
  const LevelGeom& g = b->geom[0];
  fin.g = UpGeom{g.w, g.h, p.sc_l, (p.width - width_org) / 2, (p.height - height_org) / 2, width_org, height_org};
  fin.fw = frame_at(*b, b->flow[0], first_frame);
  fin.rev = frame_at(*b, b->flow_rev[0], first_frame);
  fin.fb_rev = fin.fb ? fin.rev : nullptr;
  fin.clip_off = (size_t)first_frame * width_org * height_org * p.noc;
  return OFDIS_OK;
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

int ofdis_batch_upsample_frames(ofdis_batch* b, int first_frame, int count, float* out_dev, int width_org,
                                int height_org, void* stream) {
  if (!b || !out_dev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_upsample_crop(fin.fw, out_dev, count, fin.g, b->nop, (hipStream_t)stream));
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
  HIPCHK(launch_upsample_crop_enc(fin.fw, out, count, fin.g, b->nop, enc->type, enc->scale, enc->offset, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ reverse direction (OFDIS_BATCH_REVERSE)
int ofdis_batch_upsample_bidir(ofdis_batch* b, int first_frame, int count, float* out_fw, float* out_rev,
                               uint8_t* mask_fw, uint8_t* mask_rev, int width_org, int height_org,
                               float alpha, float beta, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_REVERSE)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!out_fw && !out_rev && !mask_fw && !mask_rev) return OFDIS_OK;
  HIPCHK(launch_upsample_bidir(fin.fw, fin.rev, out_fw, out_rev, mask_fw, mask_rev, count, fin.g, alpha, beta,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_fb_check(const float* flow, const float* flow_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream) {
  if (!flow || !flow_other || !mask) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = sizes_check(nframes, width, height)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  HIPCHK(launch_fb_check(flow, flow_other, mask, nframes, width, height, alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ stereo left-right (OFDIS_BATCH_STEREO_LR)
int ofdis_lr_check(const float* disp, const float* disp_other, uint8_t* mask, int nframes, int width, int height,
                   float alpha, float beta, void* stream) {
  if (!disp || !disp_other || !mask) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = sizes_check(nframes, width, height)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  HIPCHK(launch_lr_check(disp, disp_other, mask, nframes, width, height, alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

static int fill_mode_check(int mode) {
  if (mode != OFDIS_FILL_NONE && mode != OFDIS_FILL_INVALIDATE && mode != OFDIS_FILL_BACKGROUND)
    return fail(OFDIS_ERR_INVALID, "fill mode must be OFDIS_FILL_NONE, _INVALIDATE or _BACKGROUND");
  return OFDIS_OK;
}

int ofdis_disparity_fill(const float* disp, const uint8_t* mask, float* out, int nframes, int width, int height, int mode,
                         void* stream) {
  if (int rc = fill_mode_check(mode)) return rc;
  if (!disp || !mask || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = sizes_check(nframes, width, height)) return rc;
  HIPCHK(launch_disparity_fill(disp, mask, out, nframes, width, height, mode, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_upsample_lr(ofdis_batch* b, int first_frame, int count, float* out_left, float* out_right,
                            uint8_t* mask_left, uint8_t* mask_right, int fill_mode, int width_org, int height_org,
                            float alpha, float beta, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_STEREO_LR)) return rc;
  if (int rc = fill_mode_check(fill_mode)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  if (!out_left && !out_right && !mask_left && !mask_right) return OFDIS_OK;
  if (upsample_lr_fuses(width_org)) {
    HIPCHK(launch_upsample_lr(fin.fw, fin.rev, out_left, out_right, mask_left, mask_right, count, fin.g, fill_mode, alpha, beta, s));
    return OFDIS_OK;
  }
  // wider than the fused kernel's rows: the composition itself, through staging owned by the context
  const size_t px = (size_t)b->p.width * b->p.height;
  if (int rc = dstage(b, {{&b->lr_u, px}, {&b->lr_dr, px}, {&b->lr_mask, (2 * px + 3) / 4}})) return rc;
  const size_t n = (size_t)count * width_org * height_org;  // (count <= nframes, original size <= padded size)
  uint8_t* ml = mask_left ? mask_left : reinterpret_cast<uint8_t*>(b->lr_mask);
  uint8_t* mr = mask_right ? mask_right : reinterpret_cast<uint8_t*>(b->lr_mask) + n;
  HIPCHK(launch_lr_materialise(fin.fw, fin.rev, b->lr_u, b->lr_dr, count, fin.g, s));
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
  if (int rc = noc_check(noc)) return rc;
  if (int rc = sizes_check(nframes, width, height)) return rc;
  HIPCHK(launch_interp_frames(img_a, img_b, flow_fw, flow_rev, mask_fw, mask_rev, out, nframes, width, height, noc, ts,
                              (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_interpolate(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int first_frame, int count,
                            const float* times, int ntimes, uint8_t* out, int width_org, int height_org,
                            float alpha, float beta, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_REVERSE)) return rc;
  if (!img_a || !img_b || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  InterpTimes ts;
  if (int rc = interp_times(times, ntimes, ts)) return rc;
  if (int rc = noc_check(b->p.noc)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_interp_bidir(fin.clip(img_a), fin.clip(img_b), fin.fw, fin.rev, out, count, fin.g, b->p.noc, ts, alpha, beta,
                             (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ point trajectories (ofdis_track.hip)
static int track_args_check(const float* seeds, int npoints, int max_steps, float alpha, float beta, const float* tracks) {
  if (!seeds || !tracks) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (npoints < 1 || npoints > OFDIS_TRACK_MAX_POINTS) return fail(OFDIS_ERR_INVALID, "npoints outside 1..OFDIS_TRACK_MAX_POINTS");
  if (max_steps < 0) return fail(OFDIS_ERR_INVALID, "max_steps is negative");
  return fb_constants_check(alpha, beta);
}

int ofdis_track_points(const float* flow_fw, const float* flow_rev, int npairs, int width, int height, const float* seeds,
                       const int* seed_frame, int npoints, int max_steps, float alpha, float beta, float* tracks, int* counts,
                       void* stream) {
  if (!flow_fw) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = track_args_check(seeds, npoints, max_steps, alpha, beta, tracks)) return rc;
  if (int rc = sizes_check(npairs, width, height)) return rc;
  HIPCHK(launch_track_points(flow_fw, flow_rev, npairs, width, height, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks,
                             counts, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_track_points(ofdis_batch* b, int first_frame, int count, const float* seeds, const int* seed_frame, int npoints,
                             int max_steps, int fb_check, float alpha, float beta, float* tracks, int* counts, int width_org,
                             int height_org, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE)) return rc;  // (the pairs of any other context are no chain)
  Finish fin;
  if (int rc = fb_check_arg(b, fb_check, fin)) return rc;
  if (int rc = track_args_check(seeds, npoints, max_steps, alpha, beta, tracks)) return rc;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_track_level(fin.fw, fin.fb_rev, count, fin.g, seeds, seed_frame, npoints, max_steps, alpha, beta, tracks, counts,
                            (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ dense trajectories (ofdis_dense_tracks.hip)
static int dense_grid_check(int width, int height, int stride) {
  if (stride < 2 || stride > OFDIS_DT_MAX_STRIDE) return fail(OFDIS_ERR_INVALID, "stride outside 2..OFDIS_DT_MAX_STRIDE");
  if (int rc = sizes_check(1, width, height)) return rc;
  if (width < stride || height < stride) return fail(OFDIS_ERR_INVALID, "bad sizes (a side smaller than the stride)");
  return OFDIS_OK;
}
static int dense_texture_check(const uint8_t* frames, int noc, int window, int min_eig) {
  if (!frames) return fail(OFDIS_ERR_INVALID, "frames is NULL");
  if (int rc = noc_check(noc)) return rc;
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
  return fb_constants_check(alpha, beta);
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
  if (int rc = work_check(work, work_bytes, ofdis_dense_tracks_work_bytes(npairs, width, height, stride), "ofdis_dense_tracks_work_bytes"))
    return rc;
  HIPCHK(launch_dense_tracks(frames, flow_fw, flow_rev, npairs, width, height, noc, stride, window, min_eig, max_len, alpha, beta,
                             max_tracks, tracks, start, len, info, work, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_dense_tracks(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int stride, int window,
                             int min_eig, int max_len, int fb_check, float alpha, float beta, int max_tracks, float* tracks,
                             int* start, int* len, long long* info, int width_org, int height_org, void* stream) {
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE)) return rc;  // (the pairs of any other context are no chain)
  Finish fin;
  if (int rc = fb_check_arg(b, fb_check, fin)) return rc;
  if (int rc = dense_args_check(frames, b->p.noc, window, min_eig, max_len, alpha, beta, max_tracks, tracks, start, info)) return rc;
  if (int rc = dense_grid_check(width_org, height_org, stride)) return rc;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  // what this call needs; an earlier, smaller buffer stays with the context until it is destroyed
  const size_t need = dense_tracks_work_bytes(count, width_org, height_org, stride, max_len, max_tracks);
  if (int rc = dstage(b, {{&b->dt_slab, (need + sizeof(float) * b->nframes - 1) / (sizeof(float) * b->nframes)}})) return rc;
  HIPCHK(launch_dense_tracks_level(fin.clip(frames), fin.fw, fin.fb_rev, count, fin.g, b->p.noc, stride, window, min_eig, max_len,
                                   alpha, beta, max_tracks, tracks, start, len, info, b->dt_slab, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ track selection (ofdis_track_select.hip)
void ofdis_track_select_defaults(ofdis_track_select_params* p) {
  if (p) *p = ofdis_track_select_params{0, 1.7320508f, 50.0f, 20.0f, 0.7f, 1.0f, OFDIS_TS_ALL_TESTS};
}

size_t ofdis_track_select_work_bytes(int max_tracks) {
  return max_tracks >= 1 && max_tracks <= OFDIS_DT_MAX_TRACKS ? track_select_work_bytes(max_tracks) : 0;
}

// ofdis_track_select and ofdis_track_select_projective: nparam doubles per model
static int track_select_call(const float* tracks, const int* start, const int* len, const long long* info, int lmax, int max_tracks,
                             const double* models, int npairs, int width, int height, const ofdis_track_select_params* p,
                             uint8_t* code, long long* counts, int max_tracks_out, float* tracks_out, int* start_out, int* len_out,
                             long long* info_out, int* index, float* shape_out, void* work, size_t work_bytes, void* stream,
                             int nparam) {
  if (!tracks || !start || !len || !info) return fail(OFDIS_ERR_INVALID, "tracks, start, len or info is NULL");
  if (!p) return fail(OFDIS_ERR_INVALID, "params is NULL");
  if (!tracks_out || !start_out || !len_out || !info_out) return fail(OFDIS_ERR_INVALID, "tracks_out, start_out, len_out or info_out is NULL");
  if (lmax < 1) return fail(OFDIS_ERR_INVALID, "lmax below 1");
  if (max_tracks < 1 || max_tracks > OFDIS_DT_MAX_TRACKS) return fail(OFDIS_ERR_INVALID, "max_tracks outside 1..OFDIS_DT_MAX_TRACKS");
  if (max_tracks_out < 1 || max_tracks_out > OFDIS_DT_MAX_TRACKS)
    return fail(OFDIS_ERR_INVALID, "max_tracks_out outside 1..OFDIS_DT_MAX_TRACKS");
  if (models && (npairs < 1 || width < 1 || height < 1 || width > OFDIS_GM_MAX_SIDE || height > OFDIS_GM_MAX_SIDE))
    return fail(OFDIS_ERR_INVALID, "models with bad sizes (npairs < 1, a side above OFDIS_GM_MAX_SIDE?)");
  if (p->min_len < 0) return fail(OFDIS_ERR_INVALID, "min_len is negative");
  if (!(p->min_std >= 0.0f) || std::isinf(p->min_std)) return fail(OFDIS_ERR_INVALID, "min_std must be finite and >= 0");
  if (!(p->max_std >= 0.0f)) return fail(OFDIS_ERR_INVALID, "max_std must be >= 0");
  if (!(p->max_step >= 0.0f)) return fail(OFDIS_ERR_INVALID, "max_step must be >= 0");
  if (!(p->max_step_share >= 0.0f && p->max_step_share <= 1.0f)) return fail(OFDIS_ERR_INVALID, "max_step_share outside [0, 1]");
  if (!(p->min_camera >= 0.0f) || std::isinf(p->min_camera)) return fail(OFDIS_ERR_INVALID, "min_camera must be finite and >= 0");
  if (p->tests & ~OFDIS_TS_ALL_TESTS) return fail(OFDIS_ERR_INVALID, "tests has bits outside OFDIS_TS_ALL_TESTS");
  if (int rc = work_check(work, work_bytes, track_select_work_bytes(max_tracks), "ofdis_track_select_work_bytes")) return rc;
  HIPCHK(launch_track_select(tracks, start, len, info, lmax, max_tracks, models, npairs, width, height, *p, code, counts,
                             max_tracks_out, tracks_out, start_out, len_out, info_out, index, shape_out, work, (hipStream_t)stream,
                             nparam));
  return OFDIS_OK;
}

int ofdis_track_select(const float* tracks, const int* start, const int* len, const long long* info, int lmax, int max_tracks,
                       const double* models, int npairs, int width, int height, const ofdis_track_select_params* p, uint8_t* code,
                       long long* counts, int max_tracks_out, float* tracks_out, int* start_out, int* len_out, long long* info_out,
                       int* index, float* shape_out, void* work, size_t work_bytes, void* stream) {
  return track_select_call(tracks, start, len, info, lmax, max_tracks, models, npairs, width, height, p, code, counts,
                           max_tracks_out, tracks_out, start_out, len_out, info_out, index, shape_out, work, work_bytes, stream, 6);
}

int ofdis_track_select_projective(const float* tracks, const int* start, const int* len, const long long* info, int lmax,
                                  int max_tracks, const double* models, int npairs, int width, int height,
                                  const ofdis_track_select_params* p, uint8_t* code, long long* counts, int max_tracks_out,
                                  float* tracks_out, int* start_out, int* len_out, long long* info_out, int* index,
                                  float* shape_out, void* work, size_t work_bytes, void* stream) {
  return track_select_call(tracks, start, len, info, lmax, max_tracks, models, npairs, width, height, p, code, counts,
                           max_tracks_out, tracks_out, start_out, len_out, info_out, index, shape_out, work, work_bytes, stream, 8);
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
  if (int rc = noc_check(noc)) return rc;
  if (int rc = sizes_check(1, width, height)) return rc;
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

// ------------------------------------------------------------------------------------ bag of features (ofdis_bof.hip)
// what the four calls (and the three of the codebook training below) share: the slots, the cells of the descriptor and, where asked for (0: not an argument), the codebook's
// size and the shortest track counted
static int bof_check(const long long* info, int max_tracks, int nxy, int nt, bool codebook, int nwords, bool counts, int min_len) {
  if (!info) return fail(OFDIS_ERR_INVALID, "info is NULL");
  if (max_tracks < 1 || max_tracks > OFDIS_DT_MAX_TRACKS) return fail(OFDIS_ERR_INVALID, "max_tracks outside 1..OFDIS_DT_MAX_TRACKS");
  if (nxy < 1 || nxy > 4) return fail(OFDIS_ERR_INVALID, "nxy outside 1..4");
  if (nt < 1 || nt > 8) return fail(OFDIS_ERR_INVALID, "nt outside 1..8");
  if (codebook && (nwords < 1 || nwords > OFDIS_BOF_MAX_WORDS)) return fail(OFDIS_ERR_INVALID, "nwords outside 1..OFDIS_BOF_MAX_WORDS");
  if (counts && min_len < 1) return fail(OFDIS_ERR_INVALID, "min_len below 1");
  return OFDIS_OK;
}

int ofdis_descriptor_normalize(const uint32_t* hist, const long long* info, int max_tracks, int nxy, int nt, uint8_t* desc,
                               void* stream) {
  if (!hist) return fail(OFDIS_ERR_INVALID, "hist is NULL");
  if (!desc) return fail(OFDIS_ERR_INVALID, "desc is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, false, 0, false, 0)) return rc;
  HIPCHK(launch_descriptor_normalize(hist, info, max_tracks, nxy, nt, desc, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_codebook_assign(const uint8_t* desc, const long long* info, int max_tracks, int nxy, int nt, const uint8_t* codebook,
                          int nwords, int* words, int* dist, void* stream) {
  if (!desc) return fail(OFDIS_ERR_INVALID, "desc is NULL");
  if (!codebook) return fail(OFDIS_ERR_INVALID, "codebook is NULL");
  if (!words) return fail(OFDIS_ERR_INVALID, "words is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, true, nwords, false, 0)) return rc;
  HIPCHK(launch_codebook_assign(desc, info, max_tracks, nxy, nt, codebook, nwords, words, dist, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_bof_histogram(const int* words, const int* len, const long long* info, int max_tracks, int nwords, int min_len,
                        uint32_t* bof, void* stream) {
  if (!words) return fail(OFDIS_ERR_INVALID, "words is NULL");
  if (!len) return fail(OFDIS_ERR_INVALID, "len is NULL");
  if (!bof) return fail(OFDIS_ERR_INVALID, "bof is NULL");
  if (int rc = bof_check(info, max_tracks, 1, 1, true, nwords, true, min_len)) return rc;
  HIPCHK(launch_bof_histogram(words, len, info, max_tracks, nwords, min_len, bof, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_track_bof(const uint32_t* hist, const int* len, const long long* info, int max_tracks, int nxy, int nt,
                    const uint8_t* codebook, int nwords, int min_len, uint32_t* bof, int* words, void* stream) {
  if (!hist) return fail(OFDIS_ERR_INVALID, "hist is NULL");
  if (!len) return fail(OFDIS_ERR_INVALID, "len is NULL");
  if (!codebook) return fail(OFDIS_ERR_INVALID, "codebook is NULL");
  if (!bof) return fail(OFDIS_ERR_INVALID, "bof is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, true, nwords, true, min_len)) return rc;
  HIPCHK(launch_track_bof(hist, len, info, max_tracks, nxy, nt, codebook, nwords, min_len, bof, words, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ codebook training (ofdis_kmeans.hip)
size_t ofdis_codebook_train_work_bytes(int max_tracks, int nxy, int nt, int nwords) {
  const bool ok = max_tracks >= 1 && max_tracks <= OFDIS_DT_MAX_TRACKS && nxy >= 1 && nxy <= 4 && nt >= 1 && nt <= 8 && nwords >= 1 &&
                  nwords <= OFDIS_BOF_MAX_WORDS;
  return ok ? codebook_train_work_bytes(max_tracks, nxy, nt, nwords) : 0;
}

int ofdis_codebook_seed(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                        int min_len, uint8_t* codebook, void* stream) {
  if (!desc) return fail(OFDIS_ERR_INVALID, "desc is NULL");
  if (!codebook) return fail(OFDIS_ERR_INVALID, "codebook is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, true, nwords, true, min_len)) return rc;
  HIPCHK(launch_codebook_seed(desc, len, info, max_tracks, nxy, nt, nwords, min_len, codebook, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_codebook_update(const uint8_t* desc, const int* words, const int* len, const long long* info, int max_tracks, int nxy,
                          int nt, int nwords, int min_len, uint8_t* codebook, uint32_t* counts, void* work, size_t work_bytes,
                          void* stream) {
  if (!desc) return fail(OFDIS_ERR_INVALID, "desc is NULL");
  if (!words) return fail(OFDIS_ERR_INVALID, "words is NULL");
  if (!codebook) return fail(OFDIS_ERR_INVALID, "codebook is NULL");
  if (!counts) return fail(OFDIS_ERR_INVALID, "counts is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, true, nwords, true, min_len)) return rc;
  if (int rc = work_check(work, work_bytes, codebook_train_work_bytes(max_tracks, nxy, nt, nwords), "ofdis_codebook_train_work_bytes"))
    return rc;
  HIPCHK(launch_codebook_update(desc, words, len, info, max_tracks, nxy, nt, nwords, min_len, codebook, counts, work,
                                (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_codebook_train(const uint8_t* desc, const int* len, const long long* info, int max_tracks, int nxy, int nt, int nwords,
                         int min_len, int iters, uint8_t* codebook, int* words, uint32_t* counts, long long* stats, void* work,
                         size_t work_bytes, void* stream) {
  if (!desc) return fail(OFDIS_ERR_INVALID, "desc is NULL");
  if (!codebook) return fail(OFDIS_ERR_INVALID, "codebook is NULL");
  if (!words) return fail(OFDIS_ERR_INVALID, "words is NULL");
  if (!counts) return fail(OFDIS_ERR_INVALID, "counts is NULL");
  if (int rc = bof_check(info, max_tracks, nxy, nt, true, nwords, true, min_len)) return rc;
  if (iters < 1 || iters > OFDIS_KMEANS_MAX_ITERS) return fail(OFDIS_ERR_INVALID, "iters outside 1..OFDIS_KMEANS_MAX_ITERS");
  if (int rc = work_check(work, work_bytes, codebook_train_work_bytes(max_tracks, nxy, nt, nwords), "ofdis_codebook_train_work_bytes"))
    return rc;
  HIPCHK(launch_codebook_train(desc, len, info, max_tracks, nxy, nt, nwords, min_len, iters, codebook, words, counts, stats, work,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ temporal filter (ofdis_tfilter.hip)
static int tfilter_args_check(const uint8_t* frames, const uint8_t* out, int noc, float wn, float tau) {
  if (!frames || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (out == frames) return fail(OFDIS_ERR_INVALID, "the temporal filter does not work in place");
  if (int rc = noc_check(noc)) return rc;
  if (!(wn >= 0.0f && wn <= 1.0f)) return fail(OFDIS_ERR_INVALID, "wn must be inside [0, 1]");
  if (!(tau >= FLT_MIN)) return fail(OFDIS_ERR_INVALID, "tau must be +inf or a positive float that is not subnormal");
  return OFDIS_OK;
}

int ofdis_temporal_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, const uint8_t* mask_fw,
                          const uint8_t* mask_rev, uint8_t* out, uint8_t* support, int npairs, int width, int height, int noc,
                          float wn, float tau, void* stream) {
  if (!flow_fw || !flow_rev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = tfilter_args_check(frames, out, noc, wn, tau)) return rc;
  if (int rc = sizes_check(npairs, width, height)) return rc;
  HIPCHK(launch_tfilter_frames(frames, flow_fw, flow_rev, mask_fw, mask_rev, out, support, npairs, width, height, noc, wn, tau,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_temporal_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                uint8_t* support, int width_org, int height_org, float wn, float tau, float alpha, float beta,
                                void* stream) {
  // (the pairs of any other context share no frames)
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE)) return rc;
  if (int rc = tfilter_args_check(frames, out, b->p.noc, wn, tau)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_tfilter_level(fin.clip(frames), fin.fw, fin.rev, out, support, count, fin.g, b->p.noc, wn, tau, alpha, beta,
                              (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ trajectory filter (ofdis_trajfilter.hip)
static_assert(sizeof(TrajWeights::w) / sizeof(float) == OFDIS_TRAJ_MAX_RADIUS, "TrajWeights holds OFDIS_TRAJ_MAX_RADIUS");
static int trajfilter_args_check(const uint8_t* frames, const uint8_t* out, int noc, const float* weights, int radius, float tau,
                                 int fb_check, float alpha, float beta, TrajWeights& tw) {
  if (!frames || !out) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (out == frames) return fail(OFDIS_ERR_INVALID, "the trajectory filter does not work in place");
  if (int rc = noc_check(noc)) return rc;
  if (!weights) return fail(OFDIS_ERR_INVALID, "weights is NULL");
  if (radius < 1 || radius > OFDIS_TRAJ_MAX_RADIUS) return fail(OFDIS_ERR_INVALID, "radius must be 1..OFDIS_TRAJ_MAX_RADIUS");
  memset(&tw, 0, sizeof(tw));
  for (int j = 0; j < radius; ++j) {
    if (!(weights[j] >= 0.0f && weights[j] <= 1.0f)) return fail(OFDIS_ERR_INVALID, "every weight must be inside [0, 1]");
    tw.w[j] = weights[j];
  }
  tw.radius = radius;
  if (!(tau >= FLT_MIN)) return fail(OFDIS_ERR_INVALID, "tau must be +inf or a positive float that is not subnormal");
  if (int rc = fb_flag_check(fb_check)) return rc;
  return fb_constants_check(alpha, beta);
}

int ofdis_trajectory_filter(const uint8_t* frames, const float* flow_fw, const float* flow_rev, uint8_t* out, uint8_t* support,
                            int npairs, int width, int height, int noc, const float* weights, int radius, float tau,
                            int fb_check, float alpha, float beta, void* stream) {
  if (!flow_fw || !flow_rev) return fail(OFDIS_ERR_INVALID, "bad arguments");
  TrajWeights tw;
  if (int rc = trajfilter_args_check(frames, out, noc, weights, radius, tau, fb_check, alpha, beta, tw)) return rc;
  if (int rc = sizes_check(npairs, width, height)) return rc;
  HIPCHK(launch_trajfilter_frames(frames, flow_fw, flow_rev, out, support, npairs, width, height, noc, tw, tau, fb_check != 0,
                                  alpha, beta, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_trajectory_filter(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, uint8_t* out,
                                  uint8_t* support, int width_org, int height_org, const float* weights, int radius, float tau,
                                  int fb_check, float alpha, float beta, void* stream) {
  // (the pairs of any other context share no frames; REVERSE whatever fb_check is: walking back takes the reverse flows)
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE | OFDIS_BATCH_REVERSE)) return rc;
  TrajWeights tw;
  if (int rc = trajfilter_args_check(frames, out, b->p.noc, weights, radius, tau, fb_check, alpha, beta, tw)) return rc;
  Finish fin;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  HIPCHK(launch_trajfilter_level(fin.clip(frames), fin.fw, fin.rev, out, support, count, fin.g, b->p.noc, tw, tau, fb_check != 0, alpha,
                                 beta, (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ global motion (ofdis_gmotion.hip)
static const char* const kGmSizes = "bad sizes (a side above OFDIS_GM_MAX_SIDE?)";
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
// what both batch calls check about the context and the mask they are asked for
static int gm_batch_check(const ofdis_batch* b, int fb_check, float alpha, float beta, int width_org, int height_org, Finish& fin) {
  if (int rc = context_check(b, kOpticalFlow)) return rc;
  if (int rc = fb_check_arg(b, fb_check, fin)) return rc;
  if (int rc = fb_constants_check(alpha, beta)) return rc;
  if (width_org > OFDIS_GM_MAX_SIDE || height_org > OFDIS_GM_MAX_SIDE) return fail(OFDIS_ERR_INVALID, kGmSizes);
  return OFDIS_OK;
}

static size_t camera_work_bytes(int npairs, int width, int height, int nparam) {
  return nparam == 8 ? projective_work_bytes(npairs, width, height) : gmotion_work_bytes(npairs, width, height);
}

// The four entry points of a family, nparam = 6 (ofdis_global_motion ...) or 8 (ofdis_projective_motion ...: no `model`
// argument, the callers pass OFDIS_GM_AFFINE): the checks and the launch; the extern "C" functions below forward.
static int camera_fit(const float* flow, const uint8_t* mask, int npairs, int width, int height, int model, int rounds,
                      float thresh, double* models, long long* stats, void* work, size_t work_bytes, void* stream, int nparam) {
  if (!flow || !models) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  if (!gm_sizes_ok(npairs, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  if (int rc = work_check(work, work_bytes, camera_work_bytes(npairs, width, height, nparam),
                          nparam == 8 ? "ofdis_projective_motion_work_bytes" : "ofdis_global_motion_work_bytes"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(nparam == 8 ? launch_projective_frames(flow, mask, npairs, width, height, rounds, thresh, models, stats, work, s)
                     : launch_gmotion_frames(flow, mask, npairs, width, height, model, rounds, thresh, models, stats, work, s));
  return OFDIS_OK;
}

static int camera_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                             float thresh, float* residual, uint8_t* label, void* stream, int nparam) {
  if (!flow || !models || (!residual && !label)) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_thresh_check(thresh)) return rc;
  if (!gm_sizes_ok(npairs, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(nparam == 8 ? launch_projective_compensate_frames(flow, mask, models, npairs, width, height, thresh, residual, label, s)
                     : launch_gmotion_compensate_frames(flow, mask, models, npairs, width, height, thresh, residual, label, s));
  return OFDIS_OK;
}

static int camera_batch_fit(ofdis_batch* b, int first_frame, int count, int model, int rounds, float thresh, int fb_check,
                            float alpha, float beta, double* models, long long* stats, int width_org, int height_org, void* stream,
                            int nparam) {
  Finish fin;
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org, fin)) return rc;
  if (!models) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  // records for every pair at the padded size (no original size needs more), held as floats; one slab per family
  const size_t slab =
      camera_work_bytes(1, std::min(b->p.width, OFDIS_GM_MAX_SIDE), std::min(b->p.height, OFDIS_GM_MAX_SIDE), nparam);
  float*& held = nparam == 8 ? b->pm_slab : b->gm_slab;
  if (int rc = dstage(b, {{&held, slab / sizeof(float)}})) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(nparam == 8
             ? launch_projective_level(fin.fw, fin.fb_rev, count, fin.g, rounds, thresh, alpha, beta, models, stats, held, s)
             : launch_gmotion_level(fin.fw, fin.fb_rev, count, fin.g, model, rounds, thresh, alpha, beta, models, stats, held, s));
  return OFDIS_OK;
}

static int camera_batch_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh, int fb_check,
                                   float alpha, float beta, float* residual, uint8_t* label, int width_org, int height_org,
                                   void* stream, int nparam) {
  Finish fin;
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org, fin)) return rc;
  if (!models || (!residual && !label)) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = gm_thresh_check(thresh)) return rc;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(nparam == 8
             ? launch_projective_compensate_level(fin.fw, fin.fb_rev, models, count, fin.g, thresh, alpha, beta, residual, label, s)
             : launch_gmotion_compensate_level(fin.fw, fin.fb_rev, models, count, fin.g, thresh, alpha, beta, residual, label, s));
  return OFDIS_OK;
}

size_t ofdis_global_motion_work_bytes(int npairs, int width, int height) {
  return gm_sizes_ok(npairs, width, height) ? camera_work_bytes(npairs, width, height, 6) : 0;
}
size_t ofdis_projective_motion_work_bytes(int npairs, int width, int height) {
  return gm_sizes_ok(npairs, width, height) ? camera_work_bytes(npairs, width, height, 8) : 0;
}

int ofdis_global_motion(const float* flow, const uint8_t* mask, int npairs, int width, int height, int model, int rounds,
                        float thresh, double* models, long long* stats, void* work, size_t work_bytes, void* stream) {
  return camera_fit(flow, mask, npairs, width, height, model, rounds, thresh, models, stats, work, work_bytes, stream, 6);
}
int ofdis_projective_motion(const float* flow, const uint8_t* mask, int npairs, int width, int height, int rounds, float thresh,
                            double* models, long long* stats, void* work, size_t work_bytes, void* stream) {
  return camera_fit(flow, mask, npairs, width, height, OFDIS_GM_AFFINE, rounds, thresh, models, stats, work, work_bytes, stream, 8);
}

int ofdis_motion_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                            float thresh, float* residual, uint8_t* label, void* stream) {
  return camera_compensate(flow, mask, models, npairs, width, height, thresh, residual, label, stream, 6);
}
int ofdis_projective_compensate(const float* flow, const uint8_t* mask, const double* models, int npairs, int width, int height,
                                float thresh, float* residual, uint8_t* label, void* stream) {
  return camera_compensate(flow, mask, models, npairs, width, height, thresh, residual, label, stream, 8);
}

int ofdis_batch_global_motion(ofdis_batch* b, int first_frame, int count, int model, int rounds, float thresh, int fb_check,
                              float alpha, float beta, double* models, long long* stats, int width_org, int height_org,
                              void* stream) {
  return camera_batch_fit(b, first_frame, count, model, rounds, thresh, fb_check, alpha, beta, models, stats, width_org,
                          height_org, stream, 6);
}
int ofdis_batch_projective_motion(ofdis_batch* b, int first_frame, int count, int rounds, float thresh, int fb_check, float alpha,
                                  float beta, double* models, long long* stats, int width_org, int height_org, void* stream) {
  return camera_batch_fit(b, first_frame, count, OFDIS_GM_AFFINE, rounds, thresh, fb_check, alpha, beta, models, stats, width_org,
                          height_org, stream, 8);
}

int ofdis_batch_motion_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh, int fb_check,
                                  float alpha, float beta, float* residual, uint8_t* label, int width_org, int height_org,
                                  void* stream) {
  return camera_batch_compensate(b, first_frame, count, models, thresh, fb_check, alpha, beta, residual, label, width_org,
                                 height_org, stream, 6);
}
int ofdis_batch_projective_compensate(ofdis_batch* b, int first_frame, int count, const double* models, float thresh, int fb_check,
                                      float alpha, float beta, float* residual, uint8_t* label, int width_org, int height_org,
                                      void* stream) {
  return camera_batch_compensate(b, first_frame, count, models, thresh, fb_check, alpha, beta, residual, label, width_org,
                                 height_org, stream, 8);
}

// ------------------------------------------------------------------------------------ segments (ofdis_segments.hip)
// The limits of the section "Segments" of include/ofdis.h, which states them in prose
static const int kSegMaxSegments = 1 << 24;

size_t ofdis_segments_work_bytes(int nmaps, int width, int height) {
  return sizes_check(nmaps, width, height) == OFDIS_OK && gm_sizes_ok(nmaps, width, height) ? segments_work_bytes(nmaps, width, height)
                                                                                           : 0;
}

int ofdis_label_segments(const uint8_t* label, const float* flow, int nmaps, int width, int height, unsigned codes, int conn,
                         int min_area, int max_segments, int* segments, long long* records, long long* info, void* work,
                         size_t work_bytes, void* stream) {
  if (!label) return fail(OFDIS_ERR_INVALID, "label is NULL");
  if (!info) return fail(OFDIS_ERR_INVALID, "info is NULL");
  if (!segments && !records) return fail(OFDIS_ERR_INVALID, "segments and records are both NULL");
  if (codes == 0 || codes > 0xFFu) return fail(OFDIS_ERR_INVALID, "codes must have a bit set and none above bit 7");
  if (conn != 4 && conn != 8) return fail(OFDIS_ERR_INVALID, "conn must be 4 or 8");
  if (min_area < 0) return fail(OFDIS_ERR_INVALID, "min_area must be >= 0");
  if (max_segments < 1 || max_segments > kSegMaxSegments) return fail(OFDIS_ERR_INVALID, "max_segments outside 1..16777216");
  if (int rc = sizes_check(nmaps, width, height)) return rc;
  if (!gm_sizes_ok(nmaps, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  if (int rc = work_check(work, work_bytes, segments_work_bytes(nmaps, width, height), "ofdis_segments_work_bytes")) return rc;
  HIPCHK(launch_label_segments(label, flow, nmaps, width, height, codes, conn, min_area, max_segments, segments, records, info, work,
                               (hipStream_t)stream));
  return OFDIS_OK;
}

// ------------------------------------------------------------------------------------ object tracks (ofdis_segment_tracks.hip)
// The limits of the section "Object tracks" of include/ofdis.h, which states them in prose
static const int kSegTrackMaxSegments = 1024, kSegTrackMaxMaps = 65536, kSegTrackMaxTracks = 1 << 24;

// the checks the five calls share: the clip (nmaps, max_segments) and, for the calls that read pixels, the frame
static int segtrack_clip_check(int nmaps, int max_segments) {
  if (nmaps < 1 || nmaps > kSegTrackMaxMaps) return fail(OFDIS_ERR_INVALID, "nmaps outside 1..65536");
  if (max_segments < 1 || max_segments > kSegTrackMaxSegments) return fail(OFDIS_ERR_INVALID, "max_segments outside 1..1024");
  return OFDIS_OK;
}
static int segtrack_frame_check(int nmaps, int width, int height) {
  if (int rc = sizes_check(nmaps, width, height)) return rc;
  return gm_sizes_ok(nmaps, width, height) ? OFDIS_OK : fail(OFDIS_ERR_INVALID, kGmSizes);
}
static int segtrack_share_check(int min_share) {
  return min_share >= 0 && min_share <= 100 ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "min_share outside 0..100");
}
static int segtrack_tracks_check(int max_tracks) {
  return max_tracks >= 1 && max_tracks <= kSegTrackMaxTracks ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "max_tracks outside 1..16777216");
}
#define SEGTRACK_NEED(p) \
  if (!(p)) return fail(OFDIS_ERR_INVALID, #p " is NULL")

size_t ofdis_segment_tracks_work_bytes(int nmaps, int max_segments) {
  const bool ok = nmaps >= 1 && nmaps <= kSegTrackMaxMaps && max_segments >= 1 && max_segments <= kSegTrackMaxSegments;
  return ok ? segment_tracks_work_bytes(nmaps, max_segments) : 0;
}

int ofdis_segment_overlap(const int* segments, const float* flow, const long long* info, int nmaps, int width, int height,
                          int max_segments, int* overlap, void* stream) {
  SEGTRACK_NEED(segments);
  SEGTRACK_NEED(flow);
  SEGTRACK_NEED(info);
  SEGTRACK_NEED(overlap);
  if (int rc = segtrack_clip_check(nmaps, max_segments)) return rc;
  if (int rc = segtrack_frame_check(nmaps, width, height)) return rc;
  HIPCHK(launch_segment_overlap(segments, flow, info, nmaps, width, height, max_segments, overlap, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_segment_link(const int* overlap, const long long* records, const long long* info, int nmaps, int max_segments,
                       int min_share, int* link, void* stream) {
  SEGTRACK_NEED(overlap);
  SEGTRACK_NEED(records);
  SEGTRACK_NEED(info);
  SEGTRACK_NEED(link);
  if (int rc = segtrack_clip_check(nmaps, max_segments)) return rc;
  if (int rc = segtrack_share_check(min_share)) return rc;
  HIPCHK(launch_segment_link(overlap, records, info, nmaps, max_segments, min_share, link, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_segment_chain(const int* link, const long long* records, const long long* info, int nmaps, int max_segments,
                        int max_tracks, int* ids, long long* tracks, long long* tinfo, void* stream) {
  SEGTRACK_NEED(link);
  SEGTRACK_NEED(records);
  SEGTRACK_NEED(info);
  SEGTRACK_NEED(ids);
  SEGTRACK_NEED(tracks);
  SEGTRACK_NEED(tinfo);
  if (int rc = segtrack_clip_check(nmaps, max_segments)) return rc;
  if (int rc = segtrack_tracks_check(max_tracks)) return rc;
  HIPCHK(launch_segment_chain(link, records, info, nmaps, max_segments, max_tracks, ids, tracks, tinfo, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_segment_relabel(const int* segments, const int* ids, const long long* info, int nmaps, int width, int height,
                          int max_segments, int* track_map, void* stream) {
  SEGTRACK_NEED(segments);
  SEGTRACK_NEED(ids);
  SEGTRACK_NEED(info);
  SEGTRACK_NEED(track_map);
  if (int rc = segtrack_clip_check(nmaps, max_segments)) return rc;
  if (int rc = segtrack_frame_check(nmaps, width, height)) return rc;
  HIPCHK(launch_segment_relabel(segments, ids, info, nmaps, width, height, max_segments, track_map, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_segment_tracks(const int* segments, const float* flow, const long long* records, const long long* info, int nmaps,
                         int width, int height, int max_segments, int min_share, int max_tracks, int* ids, long long* tracks,
                         long long* tinfo, int* track_map, void* work, size_t work_bytes, void* stream) {
  SEGTRACK_NEED(segments);
  SEGTRACK_NEED(flow);
  SEGTRACK_NEED(records);
  SEGTRACK_NEED(info);
  SEGTRACK_NEED(ids);
  SEGTRACK_NEED(tracks);
  SEGTRACK_NEED(tinfo);
  if (int rc = segtrack_clip_check(nmaps, max_segments)) return rc;
  if (int rc = segtrack_frame_check(nmaps, width, height)) return rc;
  if (int rc = segtrack_share_check(min_share)) return rc;
  if (int rc = segtrack_tracks_check(max_tracks)) return rc;
  if (int rc = work_check(work, work_bytes, segment_tracks_work_bytes(nmaps, max_segments), "ofdis_segment_tracks_work_bytes")) return rc;
  int* overlap = (int*)work;   // [nmaps - 1][S][S], then link [nmaps - 1][S]
  int* link = overlap + (size_t)(nmaps - 1) * max_segments * max_segments;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(launch_segment_overlap(segments, flow, info, nmaps, width, height, max_segments, overlap, s));
  HIPCHK(launch_segment_link(overlap, records, info, nmaps, max_segments, min_share, link, s));
  HIPCHK(launch_segment_chain(link, records, info, nmaps, max_segments, max_tracks, ids, tracks, tinfo, s));
  if (track_map) HIPCHK(launch_segment_relabel(segments, ids, info, nmaps, width, height, max_segments, track_map, s));
  return OFDIS_OK;
}
#undef SEGTRACK_NEED

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
  if (int rc = noc_check(noc)) return rc;
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

// ofdis_batch_stabilize (nparam = 6) and ofdis_batch_stabilize_projective (nparam = 8: no `model` argument, the caller passes
// OFDIS_GM_AFFINE): the checks, the context's array of models and warps, and the three stages on one stream
static int camera_batch_stabilize(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int model, int rounds,
                                  float thresh, int fb_check, float alpha, float beta, const double* weights, int radius,
                                  double zoom, int border, uint8_t* out, uint8_t* inside, double* warps, int width_org,
                                  int height_org, void* stream, int nparam) {
  Finish fin;
  if (int rc = gm_batch_check(b, fb_check, alpha, beta, width_org, height_org, fin)) return rc;
  if (int rc = context_check(b, OFDIS_BATCH_SEQUENCE)) return rc;  // (the pairs of any other context are no chain)
  if (int rc = gm_fit_check(model, rounds, thresh)) return rc;
  StabWindow win;
  if (int rc = stab_window(weights, radius, zoom, win)) return rc;
  if (int rc = stab_warp_check(frames, out, b->p.noc, border)) return rc;
  if (int rc = finish_begin(b, first_frame, count, width_org, height_org, stream, fin)) return rc;
  // nparam + nparam doubles per pair and nparam more for the last frame, held as floats
  float*& held = nparam == 8 ? b->stab_path8 : b->stab_path;
  if (int rc = dstage(b, {{&held, (size_t)4 * nparam, 1}})) return rc;
  double* models = reinterpret_cast<double*>(held);
  double* path = models + (size_t)b->nframes * nparam;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = camera_batch_fit(b, first_frame, count, model, rounds, thresh, fb_check, alpha, beta, models, nullptr, width_org,
                                height_org, stream, nparam))
    return rc;
  const uint8_t* clip = fin.clip(frames);
  const bool replicate = border == OFDIS_BORDER_REPLICATE;
  if (nparam == 8) {
    HIPCHK(launch_camera_path_projective(models, count, width_org, height_org, win, path, s));
    HIPCHK(launch_warp_frames_projective(clip, path, out, inside, count + 1, width_org, height_org, b->p.noc, replicate, s));
  } else {
    HIPCHK(launch_camera_path(models, count, win, path, s));
    HIPCHK(launch_warp_frames(clip, path, out, inside, count + 1, width_org, height_org, b->p.noc, replicate, s));
  }
  if (warps) HIPCHK(hipMemcpyAsync(warps, path, (size_t)(count + 1) * nparam * sizeof(double), hipMemcpyDeviceToDevice, s));
  return OFDIS_OK;
}

int ofdis_batch_stabilize(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int model, int rounds, float thresh,
                          int fb_check, float alpha, float beta, const double* weights, int radius, double zoom, int border,
                          uint8_t* out, uint8_t* inside, double* warps, int width_org, int height_org, void* stream) {
  return camera_batch_stabilize(b, frames, first_frame, count, model, rounds, thresh, fb_check, alpha, beta, weights, radius, zoom,
                                border, out, inside, warps, width_org, height_org, stream, 6);
}

int ofdis_camera_path_projective(const double* models, int npairs, int width, int height, const double* weights, int radius,
                                 double zoom, double* warps, void* stream) {
  if (!models || !warps) return fail(OFDIS_ERR_INVALID, "bad arguments");
  StabWindow win;
  if (int rc = stab_window(weights, radius, zoom, win)) return rc;
  if (npairs < 1) return fail(OFDIS_ERR_INVALID, "bad sizes (npairs < 1)");
  if (!gm_sizes_ok(npairs, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  HIPCHK(launch_camera_path_projective(models, npairs, width, height, win, warps, (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_warp_frames_projective(const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int width,
                                 int height, int noc, int border, void* stream) {
  if (!warps) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (int rc = stab_warp_check(frames, out, noc, border)) return rc;
  if (!gm_sizes_ok(nframes, width, height)) return fail(OFDIS_ERR_INVALID, kGmSizes);
  HIPCHK(launch_warp_frames_projective(frames, warps, out, inside, nframes, width, height, noc, border == OFDIS_BORDER_REPLICATE,
                                       (hipStream_t)stream));
  return OFDIS_OK;
}

int ofdis_batch_stabilize_projective(ofdis_batch* b, const uint8_t* frames, int first_frame, int count, int rounds, float thresh,
                                     int fb_check, float alpha, float beta, const double* weights, int radius, double zoom,
                                     int border, uint8_t* out, uint8_t* inside, double* warps, int width_org, int height_org,
                                     void* stream) {
  return camera_batch_stabilize(b, frames, first_frame, count, OFDIS_GM_AFFINE, rounds, thresh, fb_check, alpha, beta, weights,
                                radius, zoom, border, out, inside, warps, width_org, height_org, stream, 8);
}

}  // extern "C"
