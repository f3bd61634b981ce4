// ofdis_launch_hooks_segments.hip -- the launch hook of the segment labelling (of_dis_amd/csrc/ofdis_segments.hip:
// launch_label_segments), linked into the TEST library beside ofdis_launch_hooks.hip, which owns the two launch limits:
// tests/test_gpu_segments.py lowers GRID_MAX_BLOCKS through tests/segments_hooks.py and expects the same bits from the second
// and later trips of every one of the seven grid-stride kernels.
#include <hip/hip_runtime.h>

#include "../../of_dis_amd/csrc/ofdis_kernels.h"
#include "ofdis_test_hooks.h"

#ifndef OFDIS_TEST_LAUNCH_LIMITS
#error "the test library is compiled with -DOFDIS_TEST_LAUNCH_LIMITS"
#endif

using namespace ofdis;

HOOK size_t ofdis_test_segments_work_bytes(int nmaps, int w, int h) {
  return segments_work_bytes(nmaps, w, h);
}

HOOK int ofdis_test_launch_label_segments(
    const uint8_t* label, const float* flow, int nmaps, int w, int h, unsigned codes, int conn, int min_area, int max_segments,
    int* segments, long long* records, long long* info, void* work, void* stream) {
  return (int)launch_label_segments(label, flow, nmaps, w, h, codes, conn, min_area, max_segments, segments, records, info, work,
                                    (hipStream_t)stream);
}
