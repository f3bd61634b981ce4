// image_io_probe.cpp -- the host image readers and writers (of_dis_amd/csrc/host/image_io.cpp) behind a program of their own,
// so that tests/test_image_io.py can hand them files no well-behaved encoder writes.  Links image_io.cpp and zlib, nothing
// else: no device, no libofdis_hip, so it also builds and runs under the host sanitizers (tools/host_sanitize.sh).
//
//   image_io_probe read  MANIFEST OUTDIR    each line "path channels": read_image(path, channels); prints "OK w h c" and
//                                           writes the decoded bytes of line k (0-based) to OUTDIR/k.raw, or prints "ERR message"
//   image_io_probe write MANIFEST           each line one writer call on an array read from a raw file:
//                                             flo  in.raw w h out                (float32 [h][w][2])
//                                             pfm  in.raw w h out                (float32 [h][w])
//                                             pgm  in.raw w h channels channel sample_bytes out
//                                             half in.raw n out                  (uint16 [n] -> float32 [n], raw)
//                                           prints "OK" or "ERR message"
// One answer line per manifest line, in order; a whole manifest is one process.  Exit status 0 whatever the files hold, 2
// for a command line or manifest it cannot use.  Test infrastructure: Python owns the inputs and the expected bytes.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "image_io.h"

namespace {

bool slurp_raw(const std::string& path, size_t bytes, std::vector<uint8_t>* buf) {
  buf->resize(bytes);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  const bool ok = fread(buf->data(), 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}

bool dump_raw(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok;
}

int bad_line(const char* manifest, int k, const std::string& line) {
  fprintf(stderr, "%s line %d: cannot use \"%s\"\n", manifest, k, line.c_str());
  return 2;
}

void answer(bool ok, const std::string& err) {
  if (ok) printf("OK\n");
  else printf("ERR %s\n", err.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  const bool reads = argc == 4 && !strcmp(argv[1], "read"), writes = argc == 3 && !strcmp(argv[1], "write");
  if (!reads && !writes) {
    fprintf(stderr, "usage: %s read MANIFEST OUTDIR | %s write MANIFEST\n", argv[0], argv[0]);
    return 2;
  }
  std::ifstream mf(argv[2]);
  if (!mf) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  std::string line;
  for (int k = 0; std::getline(mf, line); ++k) {
    std::istringstream ss(line);
    std::string err;
    if (reads) {
      std::string path;
      int channels = 0;
      if (!(ss >> path >> channels) || (channels != 1 && channels != 3)) return bad_line(argv[2], k, line);
      ofdis_host::Image8 im;
      if (!ofdis_host::read_image(path, channels, &im, &err)) {
        printf("ERR %s\n", err.c_str());
        continue;
      }
      // (the bytes the reader returned, not width * height * channels of them: the test compares the two)
      if (!dump_raw(std::string(argv[3]) + "/" + std::to_string(k) + ".raw", im.data.data(), im.data.size())) {
        fprintf(stderr, "cannot write under %s\n", argv[3]);
        return 2;
      }
      printf("OK %d %d %d\n", im.width, im.height, im.channels);
      continue;
    }
    std::string verb, in, out;
    std::vector<uint8_t> raw;
    int w = 0, h = 0;
    if (!(ss >> verb >> in)) return bad_line(argv[2], k, line);
    if (verb == "half") {
      size_t n = 0;
      if (!(ss >> n >> out) || !slurp_raw(in, 2 * n, &raw)) return bad_line(argv[2], k, line);
      std::vector<float> wide(n);
      ofdis_host::half_to_float((const uint16_t*)raw.data(), wide.data(), n);
      answer(dump_raw(out, wide.data(), 4 * n), "cannot write " + out);
    } else if (verb == "flo" || verb == "pfm") {
      const size_t per_pixel = verb == "flo" ? 8 : 4;
      if (!(ss >> w >> h >> out) || w < 1 || h < 1 || !slurp_raw(in, per_pixel * w * h, &raw)) return bad_line(argv[2], k, line);
      const bool ok = verb == "flo" ? ofdis_host::write_flo(out, (const float*)raw.data(), w, h, &err)
                                    : ofdis_host::write_pfm(out, (const float*)raw.data(), w, h, &err);
      answer(ok, err);
    } else if (verb == "pgm") {
      int channels = 0, channel = 0, sample_bytes = 0;
      if (!(ss >> w >> h >> channels >> channel >> sample_bytes >> out) || w < 1 || h < 1 || channels < 1 || channel < 0 ||
          channel >= channels || (sample_bytes != 1 && sample_bytes != 2) || !slurp_raw(in, (size_t)sample_bytes * channels * w * h, &raw))
        return bad_line(argv[2], k, line);
      answer(ofdis_host::write_pgm_plane(out, raw.data(), w, h, channels, channel, sample_bytes, &err), err);
    } else {
      return bad_line(argv[2], k, line);
    }
  }
  fflush(stdout);
  return 0;
}
