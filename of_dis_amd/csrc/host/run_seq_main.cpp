// run_OF_INT_seq / run_OF_RGB_seq -- the reference's run_OF_* main (run_dense.cpp:185-431) over MANY frame pairs and
// several GPUs of one node, in the host language of the reference, on top of the C ABI (include/ofdis.h).
// With -DOFDIS_MODE=2: run_DE_INT_seq / run_DE_RGB_seq, the stereo-depth binaries' counterpart (one displacement channel,
// "img1 img2 out.pfm" per line).
//
//   run_OF_INT_seq pairs.txt [--gpus N | --devices d0,d1,..] [--chunk C] [--depth D] [--link FORMAT] [--dry-run 1]
//                  [--sequence 1] [oppoint 1-4 | p1 .. p20]
//
// pairs.txt: one pair per line, "img1 img2 out.flo" (blank lines and lines starting with # are skipped); all images of one
// size.  The parameter block after the options is the single-pair binaries' (README.md:48-88).
//
// The reference has no such tool: its main handles one pair per process.  Frame pairs are independent problems (`initflow`
// is always null, run_dense.cpp:395), so the list is cut into contiguous shares (sizes differ by at most one, earlier
// shares take the remainder -- the partition of of_dis_amd/shard.py: frame_range), one host thread per share, each bound to
// its GPU (ofdis_set_device), with nothing shared on the data path.  A thread streams its share through resident batch
// contexts of C pairs (default 64), three stages on three threads (decode | device | .flo files) over rotating PINNED chunk
// buffers; the device stage keeps --depth D (default 2) chunks in flight, each on its own slot = context + stream + device
// buffers (round 6: include/ofdis.h version 3), so that one chunk's download (the full-resolution flow is 3.6 MB per
// 1024x436 pair: the link is the bottleneck of this stage) overlaps the next chunk's upload and kernels:
// read C pairs -> upload the 8-bit frames (ofdis_memcpy_h2d_async) -> padding, pyramid, Sobel on the device
// (ofdis_batch_build_pyramids_u8: run_dense.cpp:130-178,298-344) -> the hot path (ofdis_batch_run: OFClass::OFClass,
// oflow.cpp:184-337) -> x 2^lv_l, bilinear upsample, crop on the device (ofdis_batch_upsample_frames: run_dense.cpp:406-414)
// -> download (ofdis_memcpy_d2h_async) -> one Middlebury .flo per pair (run_dense.cpp:16-57).  Under the library's default (exact) arithmetic
// contract every .flo is byte-identical to what the single-pair binary writes for that pair, whatever the chunk size and
// the number of GPUs (tests/test_cli.py::test_sequence_driver_*).
//
// --link f32|f16|u8:BOUND|u16:SCALE:OFFSET|kitti: the format the result takes over the link (include/ofdis.h: ofdis_encoding;
// ofdis_batch_upsample_frames_enc writes it directly).  The full-resolution fp32 flow is four times the 8-bit frames that went
// up, so the download bounds the device stage; the device buffer, the pinned chunk buffer and the download shrink to the
// encoded size.  f32 (the default): as above.  f16: half precision over the link, widened on the host, the usual .flo / .pfm
// with values rounded to half precision.  u8:BOUND = {U8, 255 / (2 BOUND), 127.5}, u16:SCALE:OFFSET, kitti = {U16, 64, 32768}
// (run_DE_*_seq: {U16, -256, 0}, the KITTI disparity of the left view): binary PGM planes <out>.u.pgm and <out>.v.pgm (stereo
// depth: <out>.pgm), maxval 255 or 65535, 16-bit samples big-endian; of_dis_amd/encoding.py decodes them.
//
// --sequence 1 (run_OF_*_seq only): the list is a video, one line per FRAME, "img out.flo" -- out.flo is the flow from this
// frame to the next -- and the last line "img" alone: N + 1 lines are the N pairs (line k, line k + 1).  Shares are cut over
// pairs as above.  A chunk of C pairs then decodes and uploads its C + 1 frames once each (pinned buffer and device buffer of
// C + 1 frames, no second set) into an OFDIS_BATCH_SEQUENCE context, which builds every frame's planes once
// (ofdis_batch_build_pyramids_u8_seq); the frame two consecutive chunks of a share have in common is copied on the host from
// the previous chunk's pinned buffer instead of being decoded again.  Same bits, so the same files as the pairs list of the
// same pairs.
//
// --devices 0,0 puts two shares on one device (how the two-GPU split is tested on a one-GPU box).
// --dry-run 1 prints the partition ("share r: device d pairs lo..hi") and exits without touching a device or a file
// (tests/test_cli.py checks it against of_dis_amd.shard.frame_range on the CPU).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "cli_common.h"
#include "cli_params.h"
#include "image_io.h"
#include "ofdis.h"

using ofdis_host::now_ms;

namespace {

struct Pair {
  std::string a, b, out;
};

struct Options {  // the command line before the parameter block
  bool sequence = false, dry_run = false;
  int chunk = 16;  // (measured, round 6: with the copies on their own streams the device stage is link-bound from 16-pair
                   // chunks on -- 13.7 k pairs/s against 11.5 k with 64-pair chunks over a run of 8192 pairs, whose
                   // four 285 MB chunk buffers take 0.3 s to page-lock; small chunks also start the three stages sooner)
  int depth = 2;   // chunks in flight on the device (slots): 2 = one chunk's download overlaps the next one's upload + kernels
  int width = 0, height = 0;  // --size W H: the geometry of the run (default: the first readable pair's)
  int device_bench = 0;       // --device-bench N: measurement mode (Plan)
  int io_threads = 0;         // --io-threads T: decoder / writer workers per share (0 = hardware threads / (2 x shares), 1..16)
  ofdis_encoding link = {OFDIS_ENC_F32, 1.0f, 0.0f};  // --link
  std::string link_name = "f32";
  std::vector<int> devices;
  int first_param = 2;  // argv index of the parameter block
};

struct Share {      // one host thread = one contiguous block of the list on one device
  int device = 0;
  int lo = 0, hi = 0;
  int failed = 0;   // pairs of this share whose .flo was NOT written (unreadable, failed on the device, or unwritable)
  double ms_compute = 0;  // the device stage's busy time: first upload .. last download of its chunks (device work + PCIe,
                          // chunks overlapping), without the time it waited for the decoder / the writer
  std::string pci;        // PCI bus id of the device the share ran on
  int chunks_done = 0, chunk_pairs = 0;
  std::string error;      // a failure that ended the share early
};

void frame_range(int total, int rank, int world, int* lo, int* hi) {  // of_dis_amd/shard.py: frame_range
  const int base = total / world, rem = total % world;
  *lo = rank * base + std::min(rank, rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}

// read_image with a catch of last resort: whatever a decoder throws is that image's error line -- an exception that left a
// decode worker would be std::terminate for every share on every GPU, with passes in flight
bool read_frame(const std::string& path, ofdis_host::Image8* im, std::string* err) {
  try {
    return ofdis_host::read_image(path, OFDIS_NOC, im, err);
  } catch (const std::exception& e) {
    *err = path + ": " + e.what();
  } catch (...) {
    *err = path + ": cannot decode";
  }
  return false;
}

// The pairs of a chunk are decoded / written by `threads` workers side by side (--io-threads: the file system and the PNM / PNG
// decoder, not the device, set the pace of a run -- one worker writes ~0.7 k .flo files of 1024x436 per second).
template <typename F>
void parallel_for(int n, int threads, F&& f) {
  threads = std::max(1, std::min(threads, n));
  if (threads == 1) {
    for (int k = 0; k < n; ++k) f(k);
    return;
  }
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&] {
      for (int k = next++; k < n; k = next++) f(k);
    });
  for (auto& t : pool) t.join();
}

// Every resource of the ABI is held by a move-only handle that releases it: who owns a handle frees what it names.
template <auto Release>
struct Releaser {
  template <typename T>
  void operator()(T* p) const { Release(p); }
};
using Stream = std::unique_ptr<void, Releaser<ofdis_stream_destroy>>;
using Event = std::unique_ptr<void, Releaser<ofdis_event_destroy>>;
using DeviceMem = std::unique_ptr<void, Releaser<ofdis_dev_free>>;
using Pinned = std::unique_ptr<uint8_t, Releaser<ofdis_host_free>>;  // ofdis_host_alloc: the asynchronous copies are DMAs only
                                                                     // from / to page-locked memory
using Context = std::unique_ptr<ofdis_batch, Releaser<ofdis_batch_destroy>>;

// What a share is computed from, once: the options of the run (by now with the geometry and the workers filled in) and what
// follows from them for this share.  Nothing in it changes while the share runs.
// device_bench > 0 (--device-bench N, a measurement mode): the first chunk of the share is decoded once and pushed through the
// device stage N times, no .flo is written -- what the device stage (link + kernels) sustains when neither the decoder nor
// the file system holds it back (tools/seq_probe.py).
struct Plan : Options {
  Plan(const std::vector<Pair>& list, const Options& o, const ofdis_params& p, const Share& sh)
      : Options(o), pairs(list), params(p), device(sh.device), lo(sh.lo), hi(sh.hi), C(std::min(chunk, hi - lo)),
        F(sequence ? C + 1 : C), n_chunks(device_bench > 0 ? device_bench : (hi - lo + C - 1) / C),
        D(std::max(1, std::min(depth, n_chunks))), bench_skip(device_bench > D + 2 ? D + 2 : 0),
        img_bytes((size_t)width * height * OFDIS_NOC), flo_floats((size_t)OFDIS_NCH * width * height),
        flo_bytes(flo_floats * ofdis_encoding_bytes(link.type)) {
    params.verbosity = 0;  // (the per-level TIME lines synchronise between stages; the driver prints its own summary)
  }
  const std::vector<Pair>& pairs;
  ofdis_params params;
  int device, lo, hi;  // the share: pairs lo .. hi - 1 of the list
  int C;               // pairs of a chunk
  int F;               // frames of a chunk's first (--sequence: only) frame buffer
  int n_chunks;
  int D;               // slots in flight on the device
  int bench_skip;      // (measurement mode: the first D + 2 chunks page-lock and fill the chunk buffers -- not counted)
  size_t img_bytes, flo_floats;
  size_t flo_bytes;    // one pair's result as it crosses the link
};

// One chunk of a share on its way through the three stages: decode (reader thread) -> device (the share's thread) -> .flo
// files (writer thread).  Three buffers rotate, so that a chunk is being decoded and another written while the device works
// on a third: the device stage never waits for the file system unless the file system is the slower side (it is: DESIGN.md 6).
struct Chunk {
  int c0 = 0, m = 0;                // first pair of the chunk (index into the list), pairs in it; m = 0: end of the share
  // [C][h][w][noc] 8-bit frames; slots of unreadable pairs / of a short last chunk keep what the buffer held before (valid
  // images, results never used).  The buffers are not zero-filled up front -- a gigabyte of page faults for nothing -- only the
  // slots that would otherwise go to the device undefined are (init_upto: slots below it have been written at least once)
  // --sequence: ha holds the chunk's C + 1 frames (pair k = frames k, k + 1; fok: which were readable) and hb stays null
  Pinned ha, hb;
  int init_upto = 0;
  std::vector<char> fok;
  Pinned full;                      // [C][h][w][2] full-resolution flows, in the encoding of the link
  std::vector<char> ok;
};
// One slot of the device stage: a resident context with its own compute stream and device buffers.  The copies do NOT run on
// the slot's stream: all uploads of a share go, in order, to one upload stream and all downloads to one download stream (the
// link has one direction each; two slots that each ran upload - kernels - download on a stream of their own would fall into
// lock step -- both uploading, then both downloading -- and the directions would never overlap: tools/link_probe.py), tied
// to the slot's kernels by events.
struct Slot {
  Stream stream;                    // pyramids, the hot path, upsample (declared before the context: released after it)
  Context b;
  DeviceMem da, db;
  DeviceMem dfull;                  // the chunk's result in the encoding of the link
  Event ev_up, ev_done, ev_down;    // upload complete / kernels complete / download complete
  Chunk* chunk = nullptr;           // the chunk in flight on this slot, or null
};
class ChunkQueue {  // a FIFO of chunk pointers
 public:
  void push(Chunk* c) {
    { std::lock_guard<std::mutex> l(m_); q_.push_back(c); }
    cv_.notify_one();
  }
  Chunk* pop(bool wait = true) {  // blocks until there is one; wait = false: null when the queue is empty
    std::unique_lock<std::mutex> l(m_);
    if (wait) cv_.wait(l, [&] { return !q_.empty(); });
    if (q_.empty()) return nullptr;
    Chunk* c = q_.front();
    q_.pop_front();
    return c;
  }
 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<Chunk*> q_;
};

// A share at work: its device resources, its chunk buffers and the three stages that pass the buffers round.
class Pipeline {
 public:
  Pipeline(const Plan& plan, Share* share) : pl(plan), sh(share), slots(plan.D), bufs(plan.D + 2) {}
  // No copy may still read or write a pinned buffer when it is released: the one rule of the teardown that the order of the
  // members does not state (then the chunk buffers go first, the slots next, the copy streams last).
  ~Pipeline() {
    if (s_in) (void)ofdis_sync(s_in.get());
    if (s_out) (void)ofdis_sync(s_out.get());
    for (Slot& sl : slots)
      if (sl.stream) (void)ofdis_sync(sl.stream.get());
  }

  // the streams and slots: null, or what failed (ofdis_last_error has the reason)
  const char* setup() {
    s_in.reset(ofdis_stream_create());
    s_out.reset(ofdis_stream_create());
    if (!s_in || !s_out) return "ofdis_stream_create";
    for (Slot& sl : slots) {
      ofdis_batch* b = nullptr;
      if (ofdis_batch_create_ex(&b, &pl.params, pl.C, pl.sequence ? OFDIS_BATCH_SEQUENCE : 0u) != OFDIS_OK) return "ofdis_batch_create";
      sl.b.reset(b);
      sl.stream.reset(ofdis_stream_create());
      sl.ev_up.reset(ofdis_event_create());
      sl.ev_done.reset(ofdis_event_create());
      sl.ev_down.reset(ofdis_event_create());
      if (!sl.ev_up || !sl.ev_done || !sl.ev_down) return "ofdis_event_create";
      sl.da.reset(ofdis_dev_alloc(pl.img_bytes * pl.F));
      if (!pl.sequence) sl.db.reset(ofdis_dev_alloc(pl.img_bytes * pl.C));
      sl.dfull.reset(ofdis_dev_alloc(pl.flo_bytes * pl.C));
      if (!sl.stream || !sl.da || (!pl.sequence && !sl.db) || !sl.dfull) return "slot allocation";
    }
    return nullptr;
  }

  // the three stages, to the end of the share: the device stage on the calling thread (the one bound to the GPU)
  void run() {
    for (Chunk& c : bufs) free_q.push(&c);
    std::thread rd(&Pipeline::reader, this), wr(&Pipeline::writer, this);
    device_stage();
    rd.join();
    wr.join();
    sh->failed = pl.device_bench > 0 ? 0 : pl.hi - pl.lo - written;  // as a set: the pairs of this share without a .flo (never more than the share)
    if (alloc_failed && sh->error.empty()) sh->error = "pinned host memory";
    sh->chunks_done = pl.n_chunks - pl.bench_skip;
  }

 private:
  // ---- stage 1: decode (cv::imread in the reference, run_dense.cpp:208-209)
  void reader() {
    (void)ofdis_set_device(pl.device);  // (this thread page-locks the chunk buffers: on the share's device, not on device 0)
    for (int ci = 0; ci < pl.n_chunks && !stop; ++ci) {
      Chunk* c = free_q.pop();
      if (!chunk_alloc(*c)) {
        fprintf(stderr, "ofdis_host_alloc: %s\n", ofdis_last_error());
        alloc_failed = true;
        free_q.push(c);
        break;
      }
      c->c0 = pl.device_bench > 0 ? pl.lo : pl.lo + ci * pl.C;
      c->m = std::min(pl.C, pl.hi - c->c0);
      if (!(pl.device_bench > 0 && c->init_upto >= pl.F)) {  // (measurement mode: the buffer may hold the decoded first chunk already)
        if (pl.sequence) decode_frames(c);
        else decode_pairs(c);
        fill_tail(c);
      }
      ready_q.push(c);
    }
    Chunk* end = free_q.pop();
    end->m = 0;
    ready_q.push(end);
  }

  // (page-locking memory costs ~0.25 ms per MB, a 64-pair chunk of 1024x436 frames is 285 MB: the buffers are allocated by the
  // reader thread when it first needs them, beside the device work on the chunks before)
  bool chunk_alloc(Chunk& c) {
    if (c.ha) return true;
    c.ha.reset((uint8_t*)ofdis_host_alloc(pl.img_bytes * pl.F));
    if (!pl.sequence) c.hb.reset((uint8_t*)ofdis_host_alloc(pl.img_bytes * pl.C));
    c.full.reset((uint8_t*)ofdis_host_alloc(pl.flo_bytes * pl.C));
    c.ok.assign(pl.C, 0);
    c.fok.assign(pl.F, 0);
    return c.ha && (pl.sequence || c.hb) && c.full;
  }

  // a slot that was never written gets a defined (black) frame; any other keeps its previous content
  void blank_if_new(const Chunk& c, uint8_t* buf, int k) const {
    if (k >= c.init_upto) memset(buf + k * pl.img_bytes, 0, pl.img_bytes);
  }

  // One image into slot k of a frame buffer of the chunk.  An image that cannot be read, or is not of the run's size (reported
  // as `label`, not like the first readable `like`), is *err and leaves the slot to blank_if_new.
  bool decode_frame(const Chunk& c, uint8_t* buf, int k, const std::string& path, const std::string& label, const char* like,
                    std::string* err) const {
    ofdis_host::Image8 im;
    bool ok = read_frame(path, &im, err);
    if (ok && (im.width != pl.width || im.height != pl.height)) {
      ok = false;
      *err = label + ": not " + std::to_string(pl.width) + "x" + std::to_string(pl.height) + " like the first readable " + like;
    }
    if (ok) memcpy(buf + k * pl.img_bytes, im.data.data(), pl.img_bytes);
    else blank_if_new(c, buf, k);
    return ok;
  }

  // pairs c0 .. c0 + m - 1, both images of each; the second image of a pair is not read when the first has failed
  void decode_pairs(Chunk* c) {
    parallel_for(c->m, pl.io_threads, [&](int k) {
      const Pair& pr = pl.pairs[c->c0 + k];
      const std::string label = pr.a + " / " + pr.b;
      std::string err;
      const bool ok_a = decode_frame(*c, c->ha.get(), k, pr.a, label, "pair", &err);
      c->ok[k] = ok_a && decode_frame(*c, c->hb.get(), k, pr.b, label, "pair", &err);
      if (!ok_a) blank_if_new(*c, c->hb.get(), k);
      if (!c->ok[k]) fprintf(stderr, "%s\n", err.c_str());
    });
  }

  // frames c0 .. c0 + m, each once: frame k is pairs[c0 + k].a (the last one: the last pair's b); the first is taken over
  // from the chunk before where that chunk ended with it
  void decode_frames(Chunk* c) {
    int first = 0;
    if (carry.frame && carry.index == c->c0) {
      memmove(c->ha.get(), carry.frame, pl.img_bytes);
      c->fok[0] = carry.ok;
      first = 1;
    }
    parallel_for(c->m + 1 - first, pl.io_threads, [&](int j) {
      const int k = first + j;
      const std::string& name = k < c->m ? pl.pairs[c->c0 + k].a : pl.pairs[c->c0 + k - 1].b;
      std::string err;
      c->fok[k] = decode_frame(*c, c->ha.get(), k, name, name, "frame", &err);
      if (!c->fok[k]) fprintf(stderr, "%s\n", err.c_str());
    });
    for (int k = 0; k < c->m; ++k) c->ok[k] = c->fok[k] && c->fok[k + 1];
    carry.frame = c->ha.get() + c->m * pl.img_bytes;
    carry.index = c->c0 + c->m;
    carry.ok = c->fok[c->m];
  }

  // the slots of a short chunk that were never written
  void fill_tail(Chunk* c) const {
    if (c->init_upto >= pl.F) return;
    const int from = std::max(c->init_upto, c->m + (pl.sequence ? 1 : 0));
    if (from < pl.F) {
      memset(c->ha.get() + from * pl.img_bytes, 0, (pl.F - from) * pl.img_bytes);
      if (!pl.sequence) memset(c->hb.get() + from * pl.img_bytes, 0, (pl.F - from) * pl.img_bytes);
    }
    c->init_upto = pl.F;
  }

  // ---- stage 2: the device
  // upload (upload stream) -> pyramids, the hot path, upsample (the slot's stream) -> download (download stream)
  int enqueue(Slot& sl, Chunk* c, bool with_upload) {
    void *const in = s_in.get(), *const out = s_out.get(), *const st = sl.stream.get();
    int rc = OFDIS_OK;
    if (with_upload) {
      // (the slot's device buffers are free: retire() waited for the download that followed the kernels that last read them)
      rc = ofdis_memcpy_h2d_async(sl.da.get(), c->ha.get(), pl.img_bytes * pl.F, in);
      if (!rc && !pl.sequence) rc = ofdis_memcpy_h2d_async(sl.db.get(), c->hb.get(), pl.img_bytes * pl.C, in);
      if (!rc) rc = ofdis_event_record(sl.ev_up.get(), in);
      if (!rc) rc = ofdis_stream_wait_event(st, sl.ev_up.get());
      if (!rc && pl.sequence) rc = ofdis_batch_build_pyramids_u8_seq(sl.b.get(), (const uint8_t*)sl.da.get(), 0, 0, pl.width, pl.height, st);
      if (!rc && !pl.sequence)
        rc = ofdis_batch_build_pyramids_u8(sl.b.get(), (const uint8_t*)sl.da.get(), (const uint8_t*)sl.db.get(), pl.width, pl.height, st);
    }
    if (!rc) rc = ofdis_batch_run(sl.b.get(), st);
    if (!rc) rc = ofdis_batch_upsample_frames_enc(sl.b.get(), 0, c->m, sl.dfull.get(), pl.width, pl.height, &pl.link, st);
    if (!rc) rc = ofdis_event_record(sl.ev_done.get(), st);
    if (!rc) rc = ofdis_stream_wait_event(out, sl.ev_done.get());
    if (!rc) rc = ofdis_memcpy_d2h_async(c->full.get(), sl.dfull.get(), pl.flo_bytes * c->m, out);
    if (!rc) rc = ofdis_event_record(sl.ev_down.get(), out);
    return rc;
  }

  // wait for the slot's chunk (its download) and hand it to the writer.  A pass that reports itself as failed (a lost
  // hand-over of the cross-CU fused TV variant, small contexts only: ofdis_batch_status of THIS slot's context, whose pass
  // the download followed) is repeated once -- the pyramids are still resident and the context no longer uses that variant.
  int retire(Slot& sl) {
    Chunk* c = sl.chunk;
    if (!c) return OFDIS_OK;
    int rc = ofdis_event_sync(sl.ev_down.get());
    if (!rc) rc = ofdis_batch_status(sl.b.get());
    if (rc == OFDIS_ERR_DEVICE) {
      fprintf(stderr, "%s\n", ofdis_last_error());
      rc = enqueue(sl, c, false);
      if (!rc) rc = ofdis_event_sync(sl.ev_down.get());
      if (!rc) rc = ofdis_batch_status(sl.b.get());
    }
    sl.chunk = nullptr;
    if (rc) {
      (void)ofdis_sync(s_out.get());  // (a download may still be writing the chunk's buffer: drain before it is reused)
      (void)ofdis_sync(sl.stream.get());
      free_q.push(c);
      return rc;
    }
    done_q.push(c);
    return OFDIS_OK;
  }

  // slots are used round-robin: the oldest chunk in flight is the first occupied slot from `from` on
  Slot* oldest_in_flight(int from) {
    for (int k = 0; k < pl.D; ++k)
      if (slots[(from + k) % pl.D].chunk) return &slots[(from + k) % pl.D];
    return nullptr;
  }

  void device_stage() {
    double busy_since = 0;  // start of the current busy interval (some slot has a chunk), 0 = idle
    auto idle = [&] { if (busy_since != 0) { sh->ms_compute += now_ms() - busy_since; busy_since = 0; } };
    auto note_error = [&] { if (sh->error.empty()) sh->error = std::string("chunk: ") + ofdis_last_error(); };
    int chunks_seen = 0, next = 0;  // next: the slot the next chunk takes
    for (;;) {
      // nothing decoded yet: rather than sitting on finished chunks, hand the oldest one in flight to the writer
      Chunk* c = ready_q.pop(false);
      if (!c) {
        if (Slot* o = oldest_in_flight(next)) {
          if (retire(*o)) { note_error(); stop = true; }
          if (!oldest_in_flight(next)) idle();
          continue;
        }
        c = ready_q.pop();  // (the device is idle: this wait is the decoder's time, not the device stage's)
      }
      if (c->m == 0) {  // end of the share: retire what is in flight, oldest first
        while (Slot* o = oldest_in_flight(next))
          if (retire(*o)) note_error();
        idle();
        done_q.push(c);
        return;
      }
      if (stop) {  // (drain what the reader had already queued)
        free_q.push(c);
        continue;
      }
      Slot& sl = slots[next];
      next = (next + 1) % pl.D;
      int rc = retire(sl);  // the slot's previous chunk (the D - 1 younger chunks stay in flight meanwhile)
      if (++chunks_seen == pl.bench_skip + 1 && pl.bench_skip) { sh->ms_compute = 0; busy_since = 0; }  // the measured part starts here
      if (busy_since == 0) busy_since = now_ms();
      if (!rc) {
        rc = enqueue(sl, c, true);
        if (!rc) sl.chunk = c;
      }
      if (rc) {  // this chunk and everything after it stay unwritten; what is in flight finishes and is written
        note_error();
        stop = true;
        if (!sl.chunk) {
          (void)ofdis_sync(s_in.get());  // (copies of a half-enqueued chunk may still be reading its buffers)
          (void)ofdis_sync(s_out.get());
          free_q.push(c);
        }
      }
    }
  }

  // ---- stage 3: one result per pair: Middlebury .flo (run_dense.cpp:16-57) / .pfm, or the PGM planes of an integer encoding
  bool write_pair(const std::string& out, const uint8_t* q, std::string* err) const {
    if (pl.link.type == OFDIS_ENC_F32) return ofdis_host::write_float_result(out, (const float*)q, pl.width, pl.height, err);
    if (pl.link.type == OFDIS_ENC_F16) {
      std::vector<float> wide(pl.flo_floats);
      ofdis_host::half_to_float((const uint16_t*)q, wide.data(), pl.flo_floats);
      return ofdis_host::write_float_result(out, wide.data(), pl.width, pl.height, err);
    }
    static const char* const plane[] = {OFDIS_MODE == 2 ? ".pgm" : ".u.pgm", ".v.pgm"};
    for (int ch = 0; ch < OFDIS_NCH; ++ch)
      if (!ofdis_host::write_pgm_plane(out + plane[ch], q, pl.width, pl.height, OFDIS_NCH, ch, (int)ofdis_encoding_bytes(pl.link.type), err))
        return false;
    return true;
  }

  void writer() {
    (void)ofdis_set_device(pl.device);
    for (;;) {
      Chunk* c = done_q.pop();
      if (c->m == 0) break;
      parallel_for(pl.device_bench > 0 ? 0 : c->m, pl.io_threads, [&](int k) {
        if (!c->ok[k]) return;
        std::string err;
        if (!write_pair(pl.pairs[c->c0 + k].out, c->full.get() + k * pl.flo_bytes, &err))
          fprintf(stderr, "%s\n", err.c_str());
        else
          ++written;
      });
      free_q.push(c);
    }
  }

  const Plan& pl;
  Share* const sh;
  Stream s_in;   // every upload of this share, in order
  Stream s_out;  // every download of this share, in order
  std::vector<Slot> slots;
  std::vector<Chunk> bufs;  // one being decoded, D on the device, one being written
  ChunkQueue free_q, ready_q, done_q;
  std::atomic<int> written{0};            // .flo files of this share that exist now
  std::atomic<bool> stop{false};          // the device stage gave up: the reader stops feeding it
  std::atomic<bool> alloc_failed{false};  // the reader could not page-lock a chunk buffer
  // --sequence: the last frame of the chunk decoded before (only the reader writes frame buffers, one chunk at a time, so it
  // is still there -- even when the buffer has come round and is the one being filled now)
  struct { const uint8_t* frame = nullptr; int index = -1; char ok = 0; } carry;
};

void run_share(const std::vector<Pair>& pairs, const Options& opt, const ofdis_params& params, Share* sh) {
  const int n_share = sh->hi - sh->lo;
  if (n_share < 1) return;
  auto bail = [&](const char* what) { sh->error = std::string(what) + ": " + ofdis_last_error(); sh->failed = n_share; };
  if (ofdis_set_device(sh->device) != OFDIS_OK) return bail("ofdis_set_device");
  char id[32] = {0};
  if (ofdis_device_pci_bus_id(sh->device, id, sizeof(id)) == OFDIS_OK) sh->pci = id;
  const Plan plan(pairs, opt, params, *sh);
  sh->chunk_pairs = plan.C;
  Pipeline pipe(plan, sh);
  if (const char* what = pipe.setup()) return bail(what);
  pipe.run();
}


int usage(const char* argv0) {
  fprintf(stderr, "usage: %s pairs.txt [--gpus N | --devices d0,d1,..] [--chunk C] [--depth D] [--size W H] [--device-bench N] [--io-threads T] "
                  "[--link f32|f16|u8:BOUND|u16:SCALE:OFFSET|kitti] [--dry-run 1] [--sequence 1] [oppoint 1-4 | lv_f lv_l maxiter miniter "
                  "mindprate mindrrate minimgerr patchsz poverl usefbcon patnorm costfct usetvref tv_alpha tv_gamma tv_delta "
                  "tv_innerit tv_solverit tv_sor verbosity]\n  pairs.txt: one \"img1 img2 out.flo\" per line (--sequence 1, optical flow only: "
                  "one \"img out.flo\" per frame, the last line \"img\" alone)\n", argv0);
  return 2;
}

// one number, nothing after it, finite
bool parse_float(const std::string& t, float* out) {
  if (t.empty()) return false;
  char* end = nullptr;
  const float v = strtof(t.c_str(), &end);
  if (end != t.c_str() + t.size() || !std::isfinite(v)) return false;
  *out = v;
  return true;
}

// --link FORMAT (the top of this file) into the library's encoding
bool parse_link(const std::string& v, ofdis_encoding* enc) {
  enc->scale = 1.0f;
  enc->offset = 0.0f;
  if (v == "f32") { enc->type = OFDIS_ENC_F32; return true; }
  if (v == "f16") { enc->type = OFDIS_ENC_F16; return true; }
  if (v == "kitti") {
    enc->type = OFDIS_ENC_U16;
    enc->scale = OFDIS_MODE == 2 ? -256.0f : 64.0f;
    enc->offset = OFDIS_MODE == 2 ? 0.0f : 32768.0f;
    return true;
  }
  if (v.compare(0, 3, "u8:") == 0) {
    float bound;
    if (!parse_float(v.substr(3), &bound) || !(bound > 0.0f)) return false;
    enc->type = OFDIS_ENC_U8;
    enc->scale = 255.0f / (2.0f * bound);
    enc->offset = 127.5f;
    return std::isfinite(enc->scale) && enc->scale != 0.0f;
  }
  if (v.compare(0, 4, "u16:") == 0) {
    const size_t colon = v.find(':', 4);
    if (colon == std::string::npos) return false;
    enc->type = OFDIS_ENC_U16;
    return parse_float(v.substr(4, colon - 4), &enc->scale) && parse_float(v.substr(colon + 1), &enc->offset) && enc->scale != 0.0f;
  }
  return false;
}

// argv[2 ..] up to the parameter block into *o.  Returns 0, or the exit status.
int parse_options(int argc, char** argv, Options* o) {
  int k = 2;
  while (k < argc && argv[k][0] == '-' && argv[k][1] == '-') {
    const std::string opt = argv[k];
    if (k + 1 >= argc) {
      fprintf(stderr, "%s needs a value\n", opt.c_str());
      return 2;
    }
    const char* val = argv[k + 1];
    if (opt == "--gpus") {
      o->devices.clear();
      for (int d = 0; d < atoi(val); ++d) o->devices.push_back(d);
    } else if (opt == "--devices") {
      o->devices.clear();
      std::istringstream ss(val);
      std::string tok;
      while (std::getline(ss, tok, ',')) o->devices.push_back(atoi(tok.c_str()));
    } else if (opt == "--chunk") {
      o->chunk = atoi(val);
    } else if (opt == "--depth") {
      o->depth = atoi(val);
    } else if (opt == "--device-bench") {
      o->device_bench = atoi(val);
    } else if (opt == "--io-threads") {
      o->io_threads = atoi(val);
    } else if (opt == "--size") {
      if (k + 2 >= argc) {
        fprintf(stderr, "--size needs W H\n");
        return 2;
      }
      o->width = atoi(val);
      o->height = atoi(argv[k + 2]);
      ++k;
    } else if (opt == "--link") {
      if (!parse_link(val, &o->link)) {
        fprintf(stderr, "--link %s: not a link format\n", val);
        return usage(argv[0]);
      }
      o->link_name = val;
    } else if (opt == "--dry-run") {
      o->dry_run = atoi(val) != 0;
    } else if (opt == "--sequence") {
      o->sequence = atoi(val) != 0;
    } else {
      fprintf(stderr, "unknown option %s\n", opt.c_str());
      return 2;
    }
    k += 2;
  }
  o->first_param = k;
  if (o->devices.empty()) o->devices.push_back(0);
  if (o->sequence && OFDIS_MODE == 2) {
    fprintf(stderr, "--sequence: a list of stereo pairs is not a sequence\n");
    return 2;
  }
  return 0;
}

// The list into *pairs: one pair per line, or (sequence) one frame per line.  Returns 0, or the exit status.
int read_list(const char* path, bool sequence, std::vector<Pair>* pairs) {
  std::ifstream f(path);
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    return 1;
  }
  std::string line;
  std::vector<Pair> frames;  // --sequence: a = the frame, out = the flow to the next frame (the last frame: empty)
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    Pair pr;
    if (!(ss >> pr.a) || pr.a[0] == '#') continue;
    if (sequence) {
      ss >> pr.out;
      frames.push_back(pr);
      continue;
    }
    if (!(ss >> pr.b >> pr.out)) {
      fprintf(stderr, "%s: expected \"img1 img2 out.flo\", got \"%s\"\n", path, line.c_str());
      return 2;
    }
    pairs->push_back(pr);
  }
  for (size_t i = 0; i < frames.size(); ++i) {
    const bool last = i + 1 == frames.size();
    if (frames[i].out.empty() != last) {
      fprintf(stderr, "%s: --sequence expects \"img out.flo\" per frame and the last line \"img\" alone, got \"%s %s\"%s\n", path,
              frames[i].a.c_str(), frames[i].out.c_str(), last ? " as the last line" : "");
      return 2;
    }
    if (!last) pairs->push_back({frames[i].a, frames[i + 1].a, frames[i].out});
  }
  if (pairs->empty()) {
    fprintf(stderr, "%s lists no pairs\n", path);
    return 1;
  }
  return 0;
}

// What stands between the options and the first device work, in this order: the devices exist, --chunk, --depth, and the
// geometry of the run: --size, else the size of the first READABLE first image (an unreadable pair is reported by its share
// like any other and does not stop the pairs after it); every pair is checked against it.  Returns 0, or the exit status.
int validate(const char* list, const std::vector<Pair>& pairs, Options* o) {
  const int ndev = ofdis_device_count();
  for (int d : o->devices)
    if (d < 0 || d >= ndev) {
      fprintf(stderr, "device %d requested, %d HIP device(s) visible\n", d, ndev);
      return 1;
    }
  if (o->chunk < 1 || o->chunk > 65535) {
    fprintf(stderr, "--chunk must be 1..65535\n");
    return 2;
  }
  if (o->depth < 1 || o->depth > 8) {
    fprintf(stderr, "--depth must be 1..8\n");
    return 2;
  }
  if (o->width >= 1 && o->height >= 1) return 0;
  std::string err;
  for (size_t i = 0; i < pairs.size() && o->width < 1; ++i) {
    ofdis_host::Image8 first;
    if (read_frame(pairs[i].a, &first, &err)) {
      o->width = first.width;
      o->height = first.height;
    }
  }
  if (o->width < 1) {
    fprintf(stderr, "no readable image in %s (last error: %s)\n", list, err.c_str());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const double t_start = now_ms();
  if (argc < 2) return usage(argv[0]);
  Options opt;
  if (int st = parse_options(argc, argv, &opt)) return st;
  std::vector<Pair> pairs;
  if (int st = read_list(argv[1], opt.sequence, &pairs)) return st;
  const int R = (int)opt.devices.size();
  std::vector<Share> shares(R);
  for (int r = 0; r < R; ++r) {
    shares[r].device = opt.devices[r];
    frame_range((int)pairs.size(), r, R, &shares[r].lo, &shares[r].hi);
    if (opt.dry_run) printf("share %d: device %d pairs %d..%d\n", r, shares[r].device, shares[r].lo, shares[r].hi - 1);  // the partition only
  }
  if (opt.dry_run) return 0;
  if (int st = validate(argv[1], pairs, &opt)) return st;
  ofdis_params p;
  if (int st = ofdis_host::parse_params(argc, argv, opt.first_param, opt.width, OFDIS_NOC, OFDIS_MODE, &p)) return st;
  ofdis_host::pad_size(&p, opt.width, opt.height);
  if (opt.io_threads < 1) opt.io_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency() / (2 * R)));

  std::vector<std::thread> threads;
  const double t0 = now_ms();
  for (int r = 0; r < R; ++r) threads.emplace_back(run_share, std::cref(pairs), std::cref(opt), std::cref(p), &shares[r]);
  for (auto& t : threads) t.join();
  const double t_all = now_ms() - t0;
  int failed = 0;
  for (int r = 0; r < R; ++r) {
    const Share& s = shares[r];
    failed += s.failed;
    if (!s.error.empty()) fprintf(stderr, "share %d (device %d, pairs %d..%d): %s\n", r, s.device, s.lo, s.hi - 1, s.error.c_str());
    if (p.verbosity > 1)
      printf("TIME (share %d: device %d [%s], pairs %d..%d, upload+pyramid+flow+upsample+download, %d chunk(s) in flight) (ms): %3g\n", r,
             s.device, s.pci.c_str(), s.lo, s.hi - 1, opt.depth, s.ms_compute);
  }
  const bool f32 = opt.link.type == OFDIS_ENC_F32;
  for (int r = 0; r < R && opt.device_bench > 0; ++r)
    printf("DEVICE STAGE (share %d: %d chunks of %d pairs, %d in flight): %.1f pairs/s (upload of the 8-bit frames, pyramids, flow, upsample, "
           "download of the full-resolution flow%s%s; no decoding, no .flo)\n", r, shares[r].chunks_done, shares[r].chunk_pairs, opt.depth,
           shares[r].ms_compute > 0 ? shares[r].chunks_done * (double)shares[r].chunk_pairs / (shares[r].ms_compute * 1e-3) : 0.0,
           f32 ? "" : " as ", f32 ? "" : opt.link_name.c_str());
  if (p.verbosity > 0)
    printf("TIME (%d pairs on %d device share(s), chunk %d, incl. image decoding and .flo writing by %d worker(s) each per share) (ms): %3g  (%.1f pairs/s; start-up %3g ms)\n",
           (int)pairs.size(), R, opt.chunk, opt.io_threads, t_all, pairs.size() / (t_all * 1e-3), t0 - t_start);
  return failed ? 1 : 0;
}
