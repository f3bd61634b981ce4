#include "image_io.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <zlib.h>

#include <exception>
#include <utility>

namespace ofdis_host {
namespace {

// A reader's answer to a malformed file is `false` and a message: every index below is checked against the file's length, and
// every size a header states against what the file could hold, before anything is allocated for it.

// the whole of a REGULAR file (a directory opens as a stream as well, and then has no length to speak of)
bool slurp(const std::string& path, std::vector<uint8_t>* buf) {
  struct stat st;
  if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 0) return false;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  buf->resize((size_t)st.st_size);
  const bool ok = fread(buf->data(), 1, buf->size(), f) == buf->size();
  fclose(f);
  return ok;
}

// the next decimal number of a PNM header, after white space and comments; -1 if there is none, INT_MAX if it is larger
int pnm_int(const std::vector<uint8_t>& b, size_t* pos) {
  size_t p = *pos;
  for (;;) {
    while (p < b.size() && (b[p] == ' ' || b[p] == '\n' || b[p] == '\r' || b[p] == '\t')) ++p;
    if (p < b.size() && b[p] == '#') {
      while (p < b.size() && b[p] != '\n') ++p;
      continue;
    }
    break;
  }
  int v = 0;
  bool any = false;
  while (p < b.size() && b[p] >= '0' && b[p] <= '9') {
    const int d = b[p] - '0';
    v = v > (INT_MAX - d) / 10 ? INT_MAX : v * 10 + d;  // saturates
    ++p;
    any = true;
  }
  *pos = p;
  return any ? v : -1;
}

// the shortest P5 file: "P5 1 1 255", one white space, one sample
const size_t kPnmMinBytes = 12;

bool read_pnm(const std::vector<uint8_t>& b, Image8* im, std::string* err) {
  if (b.size() < kPnmMinBytes) { *err = "PNM file is truncated"; return false; }
  const int ch = (b[1] == '5') ? 1 : 3;
  size_t pos = 2;
  const int w = pnm_int(b, &pos), h = pnm_int(b, &pos), maxv = pnm_int(b, &pos);
  // (a maxval below 255 would need the samples scaled by 255 / maxval, as every other reader does: not an 8-bit file)
  if (w <= 0 || h <= 0 || maxv != 255) { *err = "unsupported PNM header (need 8-bit P5/P6, maxval 255)"; return false; }
  ++pos;  // single whitespace after maxval
  if (pos >= b.size() || (uint64_t)w > (uint64_t)(b.size() - pos) / ((uint64_t)h * ch)) { *err = "PNM file is truncated"; return false; }
  const size_t n = (size_t)w * h * ch;  // (at most the file's length)
  im->width = w; im->height = h; im->channels = ch;
  im->data.assign(b.begin() + pos, b.begin() + pos + n);
  if (ch == 3)  // stored R,G,B -> B,G,R (cv::imread order)
    for (size_t i = 0; i < (size_t)w * h; ++i) std::swap(im->data[3 * i], im->data[3 * i + 2]);
  return true;
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// the shortest PNG that can decode: signature, IHDR (12 + 13), one IDAT (12 + data); IEND is not insisted on
const size_t kPngMinBytes = 8 + 25 + 12;
// No deflate stream inflates to more than 1032 times its length (zlib's technical notes, "Maximum Compression Factor": a
// length-258 match costs at least two bits): an image whose scanlines would take more than that is refused unallocated.
const uint64_t kInflateMaxRatio = 1032;

bool read_png(const std::vector<uint8_t>& b, Image8* im, std::string* err) {
  if (b.size() < kPngMinBytes) { *err = "PNG file is truncated"; return false; }
  size_t pos = 8;
  bool have_ihdr = false, have_plte = false;
  uint32_t w = 0, h = 0;
  int depth = 0, ctype = 0, compression = 0, filter = 0, interlace = 0;
  std::vector<uint8_t> idat, plte;
  while (b.size() - pos >= 12) {  // length, type, data, CRC (not checked)
    const uint32_t len = be32(&b[pos]);
    const char* type = (const char*)&b[pos + 4];
    const uint8_t* d = &b[pos + 8];
    if (len > b.size() - pos - 12) { *err = "PNG chunk overruns file"; return false; }
    const bool ihdr = !memcmp(type, "IHDR", 4);
    if (!ihdr && !have_ihdr) { *err = "PNG does not start with IHDR"; return false; }
    if (ihdr && have_ihdr) { *err = "PNG has two IHDR chunks"; return false; }
    if (ihdr) {
      if (len != 13) { *err = "PNG IHDR chunk is not 13 bytes long"; return false; }
      w = be32(d); h = be32(d + 4); depth = d[8]; ctype = d[9]; compression = d[10]; filter = d[11]; interlace = d[12];
      have_ihdr = true;
    } else if (!memcmp(type, "PLTE", 4)) {
      if (have_plte || len == 0 || len % 3 != 0 || len > 768) { *err = "PNG PLTE chunk is not 1..256 entries of 3 bytes, once"; return false; }
      plte.assign(d, d + len);
      have_plte = true;
    } else if (!memcmp(type, "IDAT", 4)) {
      idat.insert(idat.end(), d, d + len);
    } else if (!memcmp(type, "IEND", 4)) {
      break;
    }
    pos += 12 + (size_t)len;
  }
  if (!have_ihdr) { *err = "PNG does not start with IHDR"; return false; }
  if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) { *err = "PNG size is not 1..2^31-1"; return false; }
  if (depth != 8 || interlace != 0 || compression != 0 || filter != 0) { *err = "unsupported PNG (need 8-bit, non-interlaced)"; return false; }
  int spp;
  switch (ctype) {
    case 0: spp = 1; break;
    case 2: spp = 3; break;
    case 3: spp = 1; break;
    case 4: spp = 2; break;
    case 6: spp = 4; break;
    default: *err = "unsupported PNG colour type"; return false;
  }
  if (ctype == 3 && !have_plte) { *err = "PNG palette image without PLTE chunk"; return false; }
  // filter byte + samples per scanline: below 2^33 each, below 2^64 together; against what the IDAT bytes could inflate to
  const uint64_t raw_bytes = ((uint64_t)w * spp + 1) * h;
  if (raw_bytes > kInflateMaxRatio * idat.size()) { *err = "PNG image data is too short for its size"; return false; }
  const size_t stride = (size_t)w * spp;
  std::vector<uint8_t> raw((size_t)raw_bytes);
  uLongf rawlen = (uLongf)raw.size();
  if (uncompress(raw.data(), &rawlen, idat.data(), (uLong)idat.size()) != Z_OK || rawlen != raw.size()) {
    *err = "PNG inflate failed";
    return false;
  }
  std::vector<uint8_t> pix(stride * h);
  for (size_t y = 0; y < h; ++y) {  // undo the scanline filters
    const int ft = raw[(stride + 1) * y];
    if (ft > 4) { *err = "PNG scanline has an unknown filter type"; return false; }
    const uint8_t* in = &raw[(stride + 1) * y + 1];
    uint8_t* cur = &pix[stride * y];
    const uint8_t* up = y ? &pix[stride * (y - 1)] : nullptr;
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= (size_t)spp ? cur[i - spp] : 0, bb = up ? up[i] : 0, c = (up && i >= (size_t)spp) ? up[i - spp] : 0;
      int v = in[i];
      switch (ft) {
        case 1: v += a; break;
        case 2: v += bb; break;
        case 3: v += (a + bb) >> 1; break;
        case 4: {
          const int p = a + bb - c, pa = abs(p - a), pb = abs(p - bb), pc = abs(p - c);
          v += (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
          break;
        }
        default: break;
      }
      cur[i] = (uint8_t)v;
    }
  }
  const bool color = (ctype == 2 || ctype == 6 || ctype == 3);
  const size_t n = (size_t)w * h;
  im->width = (int)w; im->height = (int)h; im->channels = color ? 3 : 1;
  im->data.resize(n * im->channels);
  for (size_t i = 0; i < n; ++i) {
    if (ctype == 0 || ctype == 4) {
      im->data[i] = pix[i * spp];
    } else {
      uint8_t r, g, bl;
      if (ctype == 3) {
        const size_t k = (size_t)pix[i] * 3;
        if (k + 2 >= plte.size()) { r = g = bl = 0; }  // an index beyond the palette: black
        else { r = plte[k]; g = plte[k + 1]; bl = plte[k + 2]; }
      } else {
        r = pix[i * spp]; g = pix[i * spp + 1]; bl = pix[i * spp + 2];
      }
      im->data[3 * i] = bl; im->data[3 * i + 1] = g; im->data[3 * i + 2] = r;
    }
  }
  return true;
}

bool read_any(const std::string& path, int want_channels, Image8* out, std::string* err) {
  std::vector<uint8_t> b;
  if (!slurp(path, &b)) { *err = "cannot read " + path; return false; }
  Image8 im;
  static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  bool ok;
  if (b.size() >= 2 && b[0] == 'P' && (b[1] == '5' || b[1] == '6')) ok = read_pnm(b, &im, err);
  else if (b.size() >= 8 && !memcmp(b.data(), png_sig, 8)) ok = read_png(b, &im, err);
  else { *err = path + ": unsupported format (PGM/PPM binary or PNG)"; return false; }
  if (!ok) { *err = path + ": " + *err; return false; }
  if (im.channels == want_channels) { *out = std::move(im); return true; }
  Image8 cv;
  cv.width = im.width; cv.height = im.height; cv.channels = want_channels;
  const size_t n = (size_t)im.width * im.height;
  cv.data.resize(n * want_channels);
  if (want_channels == 1) {
    for (size_t i = 0; i < n; ++i) {
      const int bl = im.data[3 * i], g = im.data[3 * i + 1], r = im.data[3 * i + 2];
      cv.data[i] = (uint8_t)((r * 4899 + g * 9617 + bl * 1868 + 8192) >> 14);
    }
  } else {
    for (size_t i = 0; i < n; ++i) cv.data[3 * i] = cv.data[3 * i + 1] = cv.data[3 * i + 2] = im.data[i];
  }
  *out = std::move(cv);
  return true;
}

}  // namespace

// (never throws: a well-formed file too large for this machine's memory is an unreadable file like any other)
bool read_image(const std::string& path, int want_channels, Image8* out, std::string* err) {
  try {
    return read_any(path, want_channels, out, err);
  } catch (const std::exception& e) {
    try { *err = path + ": " + e.what(); } catch (...) { err->clear(); }
    return false;
  }
}

bool write_flo(const std::string& path, const float* flow_uv, int width, int height, std::string* err) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { *err = "WriteFile: could not open file " + path; return false; }
  bool ok = fwrite("PIEH", 1, 4, f) == 4;
  const int32_t w = width, h = height;
  ok = ok && fwrite(&w, sizeof(w), 1, f) == 1 && fwrite(&h, sizeof(h), 1, f) == 1;
  ok = ok && fwrite(flow_uv, sizeof(float), (size_t)2 * width * height, f) == (size_t)2 * width * height;
  fclose(f);
  if (!ok) *err = "WriteFile: problem writing data to " + path;
  return ok;
}

// SavePFMFile (run_dense.cpp:60-81): "Pf", size, scale -1.000000 (little endian), rows bottom-up, values negated
bool write_pfm(const std::string& path, const float* disp, int width, int height, std::string* err) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { *err = "WriteFile: could not open file " + path; return false; }
  fprintf(f, "Pf\n%d %d\n%f\n", width, height, (float)-1.0f);
  bool ok = true;
  for (int y = height - 1; y >= 0 && ok; --y)
    for (int x = 0; x < width; ++x) {
      const float t = -disp[(size_t)y * width + x];
      if (fwrite(&t, sizeof(float), 1, f) != 1) { ok = false; break; }
    }
  fclose(f);
  if (!ok) *err = "WriteFile: problem writing data to " + path;
  return ok;
}

// binary PGM of one component of an interleaved integer array; 16-bit samples most significant byte first (the PNM rule)
bool write_pgm_plane(const std::string& path, const void* samples, int width, int height, int channels, int channel,
                     int sample_bytes, std::string* err) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { *err = "WriteFile: could not open file " + path; return false; }
  fprintf(f, "P5\n%d %d\n%d\n", width, height, sample_bytes == 2 ? 65535 : 255);
  const size_t n = (size_t)width * height;
  std::vector<uint8_t> plane(n * sample_bytes);
  if (sample_bytes == 2) {
    const uint16_t* q = (const uint16_t*)samples;
    for (size_t i = 0; i < n; ++i) {
      const uint16_t v = q[i * channels + channel];
      plane[2 * i] = (uint8_t)(v >> 8);
      plane[2 * i + 1] = (uint8_t)(v & 255);
    }
  } else {
    const uint8_t* q = (const uint8_t*)samples;
    for (size_t i = 0; i < n; ++i) plane[i] = q[i * channels + channel];
  }
  const bool ok = fwrite(plane.data(), 1, plane.size(), f) == plane.size();
  fclose(f);
  if (!ok) *err = "WriteFile: problem writing data to " + path;
  return ok;
}

// IEEE binary16 -> binary32, exact (subnormals, infinities and NaNs included)
void half_to_float(const uint16_t* src, float* dst, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t h = src[i], sign = (h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31, m = h & 1023, bits;
    if (e == 31) {
      bits = sign | 0x7f800000u | (m << 13);
    } else if (e != 0) {
      bits = sign | ((e + 112) << 23) | (m << 13);
    } else if (m == 0) {
      bits = sign;
    } else {  // subnormal half: normalise
      e = 113;
      while (!(m & 1024)) { m <<= 1; --e; }
      bits = sign | (e << 23) | ((m & 1023) << 13);
    }
    memcpy(dst + i, &bits, sizeof(bits));
  }
}

}  // namespace ofdis_host
