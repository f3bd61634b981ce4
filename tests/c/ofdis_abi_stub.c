/* ofdis_abi_stub.c -- a host-only stand-in for the part of the C ABI (include/ofdis.h) that the two host mains
 * (of_dis_amd/csrc/host/run_dense_main.cpp, run_seq_main.cpp) and cli_params.h call, so that the sequence driver links and
 * runs as it is on a machine without a GPU (of_dis_amd/build.py: seq_stub_command; tests/test_seq_driver_stub.py).  It
 * includes the header: a signature that drifts no longer compiles.
 *
 * Everything is synchronous: "device" memory is malloc, the *_async copies are memcpy, streams and events are one-byte
 * allocations (so that a handle that is never destroyed is a leak a sanitizer sees).  A context keeps a copy of the frames it
 * was built from, and its "flow" is an element-wise function of the two frames of a pair
 * (tests/test_seq_driver_stub.py: stub_flow states it in numpy):
 *     a = first byte, a2 = last byte of the pixel of frame A; b, b2 of frame B
 *     channel 0:  0.25 a - 0.125 b2          channel 1 (optical flow only):  0.03125 b - 0.5 a2 + 1
 * (every value and every partial result is exact in fp32, not in half precision), written in the requested encoding with the
 * header's arithmetic.
 * A wrong frame, slot, carried frame or stale buffer therefore changes the bytes of a result.
 *
 * Failures by ordinal, from the environment (counted over the whole process, 1-based, atomically):
 *     OFDIS_STUB_FAIL_RUN=N         the N-th ofdis_batch_run returns OFDIS_ERR_INVALID
 *     OFDIS_STUB_FAIL_STATUS=N      the N-th ofdis_batch_status returns OFDIS_ERR_DEVICE (only that one)
 *     OFDIS_STUB_FAIL_HOST_ALLOC=N  the N-th ofdis_host_alloc returns NULL
 *     OFDIS_STUB_DEVICES=N          what ofdis_device_count reports (default 2) */
#include <math.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ofdis.h"

struct ofdis_batch {
  int nframes, noc, nch, sequence;
  int width, height;      /* of the frames held, 0 before the first build */
  uint8_t *frames_a, *frames_b; /* sequence: frames_a holds nframes + 1 frames and frames_b stays NULL */
};

static _Thread_local char g_error[160] = "";
static atomic_int g_runs, g_statuses, g_host_allocs;

static int fail(int rc, const char* what) {
  snprintf(g_error, sizeof(g_error), "stub: %s", what);
  return rc;
}
/* does this call, the n-th of its kind, fail? */
static int nth_fails(atomic_int* counter, const char* knob) {
  const int n = atomic_fetch_add(counter, 1) + 1;
  const char* v = getenv(knob);
  return v && atoi(v) == n;
}

const char* ofdis_last_error(void) { return g_error; }

int ofdis_params_oppoint(ofdis_params* p, int op_point, int width_org, int noc) {
  if (!p || width_org <= 0 || (noc != 1 && noc != 3) || op_point < 1 || op_point > 4) return fail(OFDIS_ERR_INVALID, "bad arguments");
  memset(p, 0, sizeof(*p));
  p->sc_f = 3;
  p->sc_l = 1;
  p->p_samp_s = p->imgpadding = 8;
  p->noc = noc;
  p->verbosity = 2;
  return OFDIS_OK;
}

int ofdis_device_count(void) {
  const char* v = getenv("OFDIS_STUB_DEVICES");
  return v ? atoi(v) : 2;
}
int ofdis_set_device(int device) {
  return device >= 0 && device < ofdis_device_count() ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "no such device");
}
int ofdis_device_pci_bus_id(int device, char* buf, int len) {
  if (!buf || len < 16 || device < 0 || device >= ofdis_device_count()) return fail(OFDIS_ERR_INVALID, "bad arguments");
  snprintf(buf, (size_t)len, "0000:%02x:00.0", device);
  return OFDIS_OK;
}

int ofdis_batch_create_ex(ofdis_batch** out, const ofdis_params* p, int nframes, unsigned flags) {
  if (!out || !p || nframes < 1 || (flags & ~OFDIS_BATCH_SEQUENCE)) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if ((flags & OFDIS_BATCH_SEQUENCE) && p->selectmode == 2) return fail(OFDIS_ERR_INVALID, "a stereo pair is no sequence");
  ofdis_batch* b = (ofdis_batch*)calloc(1, sizeof(*b));
  if (!b) return fail(OFDIS_ERR_NOMEM, "out of memory");
  b->nframes = nframes;
  b->noc = p->noc;
  b->nch = p->selectmode == 2 ? 1 : 2;
  b->sequence = (flags & OFDIS_BATCH_SEQUENCE) != 0;
  *out = b;
  return OFDIS_OK;
}
int ofdis_batch_create(ofdis_batch** out, const ofdis_params* p, int nframes) { return ofdis_batch_create_ex(out, p, nframes, 0u); }
void ofdis_batch_destroy(ofdis_batch* b) {
  if (!b) return;
  free(b->frames_a);
  free(b->frames_b);
  free(b);
}

/* the context's own copy of `count` frames */
static int keep_frames(ofdis_batch* b, uint8_t** held, const uint8_t* frames, int count, int width_org, int height_org) {
  const size_t bytes = (size_t)count * width_org * height_org * b->noc;
  free(*held);
  *held = (uint8_t*)malloc(bytes);
  if (!*held) return fail(OFDIS_ERR_NOMEM, "out of memory");
  memcpy(*held, frames, bytes);
  b->width = width_org;
  b->height = height_org;
  return OFDIS_OK;
}
int ofdis_batch_build_pyramids_u8(ofdis_batch* b, const uint8_t* img_a, const uint8_t* img_b, int width_org, int height_org,
                                  void* stream) {
  (void)stream;
  if (!b || b->sequence || !img_a || !img_b || width_org < 1 || height_org < 1) return fail(OFDIS_ERR_INVALID, "bad arguments");
  const int rc = keep_frames(b, &b->frames_a, img_a, b->nframes, width_org, height_org);
  return rc ? rc : keep_frames(b, &b->frames_b, img_b, b->nframes, width_org, height_org);
}
int ofdis_batch_build_pyramids_u8_seq(ofdis_batch* b, const uint8_t* frames, size_t row_pitch, size_t frame_stride, int width_org,
                                      int height_org, void* stream) {
  (void)stream;
  if (!b || !b->sequence || !frames || row_pitch || frame_stride || width_org < 1 || height_org < 1)
    return fail(OFDIS_ERR_INVALID, "bad arguments (the stub takes packed frames only)");
  return keep_frames(b, &b->frames_a, frames, b->nframes + 1, width_org, height_org);
}

int ofdis_batch_run(ofdis_batch* b, void* stream) {
  (void)stream;
  if (!b || !b->frames_a) return fail(OFDIS_ERR_INVALID, "no frames in the context");
  if (nth_fails(&g_runs, "OFDIS_STUB_FAIL_RUN")) return fail(OFDIS_ERR_INVALID, "injected failure of ofdis_batch_run");
  return OFDIS_OK;
}
int ofdis_batch_status(ofdis_batch* b) {
  if (!b) return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (nth_fails(&g_statuses, "OFDIS_STUB_FAIL_STATUS")) return fail(OFDIS_ERR_DEVICE, "injected lost pass");
  return OFDIS_OK;
}

size_t ofdis_encoding_bytes(int type) {
  switch (type) {
    case OFDIS_ENC_F32: return 4;
    case OFDIS_ENC_F16: case OFDIS_ENC_U16: return 2;
    case OFDIS_ENC_U8: return 1;
  }
  return 0;
}
/* IEEE binary16 of v, round to nearest even (finite |v| < 65520 only: all the stub produces) */
static uint16_t to_half(float v) {
  uint32_t x;
  memcpy(&x, &v, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  const int e = (int)((x >> 23) & 0xff) - 127 + 15;
  uint32_t m = x & 0x7fffffu;
  if (e >= 31) return (uint16_t)(sign | 0x7c00u);
  if (e <= 0) {  /* subnormal half or zero */
    if (e < -10) return sign;
    m |= 0x800000u;
    const int shift = 14 - e;
    const uint32_t q = m >> shift, rest = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    return (uint16_t)(sign | (q + (rest > half || (rest == half && (q & 1)))));
  }
  const uint32_t q = ((uint32_t)e << 10) | (m >> 13), rest = m & 0x1fffu;
  return (uint16_t)(sign | (q + (rest > 0x1000u || (rest == 0x1000u && (q & 1)))));  /* (a carry runs into the exponent) */
}
int ofdis_batch_upsample_frames_enc(ofdis_batch* b, int first_frame, int count, void* out, int width_org, int height_org,
                                    const ofdis_encoding* enc, void* stream) {
  (void)stream;
  if (!b || !out || !enc || !ofdis_encoding_bytes(enc->type) || first_frame < 0 || count < 1 || first_frame + count > b->nframes)
    return fail(OFDIS_ERR_INVALID, "bad arguments");
  if (!b->frames_a || width_org != b->width || height_org != b->height) return fail(OFDIS_ERR_INVALID, "not the size of the frames held");
  const int integer = enc->type == OFDIS_ENC_U16 || enc->type == OFDIS_ENC_U8;
  if (integer && (!isfinite(enc->scale) || enc->scale == 0.0f || !isfinite(enc->offset))) return fail(OFDIS_ERR_INVALID, "bad encoding");
  const size_t npix = (size_t)width_org * height_org, noc = (size_t)b->noc;
  const float top = enc->type == OFDIS_ENC_U8 ? 255.0f : 65535.0f;
  size_t o = 0;
  for (int k = first_frame; k < first_frame + count; ++k) {
    const uint8_t* fa = b->frames_a + (size_t)k * npix * noc;
    const uint8_t* fb = b->sequence ? fa + npix * noc : b->frames_b + (size_t)k * npix * noc;
    for (size_t i = 0; i < npix; ++i)
      for (int c = 0; c < b->nch; ++c, ++o) {
        const float v = c == 0 ? 0.25f * fa[i * noc] - 0.125f * fb[i * noc + noc - 1]
                               : 0.03125f * fb[i * noc] - 0.5f * fa[i * noc + noc - 1] + 1.0f;
        if (enc->type == OFDIS_ENC_F32) {
          ((float*)out)[o] = v;
        } else if (enc->type == OFDIS_ENC_F16) {
          ((uint16_t*)out)[o] = to_half(v);
        } else {
          volatile float t = v * enc->scale;  /* (volatile: two separately rounded operations, whatever the flags) */
          t = t + enc->offset;
          const float q = floorf(fminf(fmaxf(t, 0.0f), top) + 0.5f);
          if (enc->type == OFDIS_ENC_U8) ((uint8_t*)out)[o] = (uint8_t)q;
          else ((uint16_t*)out)[o] = (uint16_t)q;
        }
      }
  }
  return OFDIS_OK;
}
int ofdis_batch_upsample(ofdis_batch* b, float* out_dev, int width_org, int height_org, void* stream) {
  const ofdis_encoding f32 = {OFDIS_ENC_F32, 1.0f, 0.0f};
  return ofdis_batch_upsample_frames_enc(b, 0, b ? b->nframes : 0, out_dev, width_org, height_org, &f32, stream);
}

void* ofdis_dev_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void ofdis_dev_free(void* p) { free(p); }
void* ofdis_host_alloc(size_t bytes) {
  if (nth_fails(&g_host_allocs, "OFDIS_STUB_FAIL_HOST_ALLOC")) {
    fail(OFDIS_ERR_NOMEM, "injected failure of ofdis_host_alloc");
    return NULL;
  }
  return malloc(bytes ? bytes : 1);
}
void ofdis_host_free(void* p) { free(p); }
static int copy(void* dst, const void* src, size_t bytes) {
  if (!dst || !src) return fail(OFDIS_ERR_INVALID, "NULL in a copy");
  memcpy(dst, src, bytes);
  return OFDIS_OK;
}
int ofdis_memcpy_h2d(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes); }
int ofdis_memcpy_d2h(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes); }
int ofdis_memcpy_h2d_async(void* dst_dev, const void* src_host, size_t bytes, void* stream) {
  return stream ? copy(dst_dev, src_host, bytes) : fail(OFDIS_ERR_INVALID, "NULL stream");
}
int ofdis_memcpy_d2h_async(void* dst_host, const void* src_dev, size_t bytes, void* stream) {
  return stream ? copy(dst_host, src_dev, bytes) : fail(OFDIS_ERR_INVALID, "NULL stream");
}
int ofdis_sync(void* stream) {
  (void)stream;
  return OFDIS_OK;
}

void* ofdis_stream_create(void) { return malloc(1); }
void ofdis_stream_destroy(void* stream) { free(stream); }
void* ofdis_event_create(void) { return malloc(1); }
void ofdis_event_destroy(void* event) { free(event); }
int ofdis_event_record(void* event, void* stream) { return event && stream ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "NULL event or stream"); }
int ofdis_stream_wait_event(void* stream, void* event) { return event && stream ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "NULL event or stream"); }
int ofdis_event_sync(void* event) { return event ? OFDIS_OK : fail(OFDIS_ERR_INVALID, "NULL event"); }
