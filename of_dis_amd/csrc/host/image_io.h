// image_io.h -- minimal 8-bit image reading (PGM/PPM binary, PNG via zlib) and Middlebury .flo writing for
// the run_OF_* executables.  The reference uses cv::imread (run_dense.cpp:208-209); OpenCV is not a
// dependency here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace ofdis_host {

struct Image8 {
  int width = 0, height = 0, channels = 0;  // channels: 1 (gray) or 3 (B,G,R interleaved like cv::imread)
  std::vector<uint8_t> data;
};

// Reads P5/P6 PNM or PNG (8-bit gray / gray+alpha / RGB / RGBA / palette, non-interlaced).
// want_channels = 1: colour input is converted with OpenCV's fixed-point BGR2GRAY
// (Y = (4899 R + 9617 G + 1868 B + 8192) >> 14); = 3: gray input is replicated.
// Anything else -- not a regular file, another format, maxval other than 255, a header that promises more than the file
// holds -- is `false` and one line in *err that names the path: never an exception, never a read outside the file
// (INTEGRATION.md 6 lists what is refused; tests/test_image_io.py).
bool read_image(const std::string& path, int want_channels, Image8* out, std::string* err);

// SaveFlowFile (run_dense.cpp:16-57): "PIEH", int32 width, int32 height, then rows of (float u, float v).
bool write_flo(const std::string& path, const float* flow_uv, int width, int height, std::string* err);
// stereo-depth result (run_dense.cpp:60-81): one channel, PFM
bool write_pfm(const std::string& path, const float* disp, int width, int height, std::string* err);
// Integer-encoded results (run_*_seq --link u8 / u16): component `channel` of the interleaved array
// samples[height][width][channels] (sample_bytes 1 or 2, host byte order) as a binary PGM (P5), maxval 255 or 65535; 16-bit
// samples are written most significant byte first, as PNM defines.
bool write_pgm_plane(const std::string& path, const void* samples, int width, int height, int channels, int channel,
                     int sample_bytes, std::string* err);
// IEEE binary16 values to float, exactly (run_*_seq --link f16 widens on the host before it writes .flo / .pfm)
void half_to_float(const uint16_t* src, float* dst, size_t n);

}  // namespace ofdis_host
