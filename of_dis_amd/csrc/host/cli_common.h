// cli_common.h -- what the single-pair binaries (run_dense_main.cpp) and the sequence driver (run_seq_main.cpp) state in the
// same words: which of the reference's per-binary choices a program is compiled for, the clock of the TIME lines, and the file
// a floating-point result goes to.
#pragma once
#include <sys/time.h>

#include <string>

#include "image_io.h"

#ifndef OFDIS_NOC  // the reference's SELECTCHANNEL: 1 gray (run_*_INT*), 3 colour (run_*_RGB*)
#define OFDIS_NOC 1
#endif
#ifndef OFDIS_MODE  // the reference's SELECTMODE: 1 optical flow (run_OF_*, .flo), 2 stereo depth (run_DE_*, .pfm)
#define OFDIS_MODE 1
#endif
#define OFDIS_NCH (OFDIS_MODE == 2 ? 1 : 2)  // values per pixel of a result

namespace ofdis_host {

inline double now_ms() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return tv.tv_sec * 1000.0 + tv.tv_usec / 1000.0;
}

// one fp32 result [height][width][OFDIS_NCH]: Middlebury .flo (run_dense.cpp:16-57), or .pfm in stereo-depth mode
inline bool write_float_result(const std::string& out, const float* v, int width, int height, std::string* err) {
#if OFDIS_MODE == 2
  return write_pfm(out, v, width, height, err);
#else
  return write_flo(out, v, width, height, err);
#endif
}

}  // namespace ofdis_host
