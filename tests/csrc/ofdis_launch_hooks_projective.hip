// ofdis_launch_hooks_projective.hip -- the launch hook of the projective frame warp (of_dis_amd/csrc/ofdis_stabilize.hip:
// launch_warp_frames_projective), linked into the TEST library beside ofdis_launch_hooks.hip, which owns the two launch limits:
// tests/test_gpu_stabilize_projective.py lowers QUAD_MAX_BLOCKS through tests/launch_hooks.py and expects the same bytes from
// the launcher's second chunk.
#include <hip/hip_runtime.h>

#include "../../of_dis_amd/csrc/ofdis_kernels.h"
#include "ofdis_test_hooks.h"

#ifndef OFDIS_TEST_LAUNCH_LIMITS
#error "the test library is compiled with -DOFDIS_TEST_LAUNCH_LIMITS"
#endif

using namespace ofdis;

HOOK int ofdis_test_launch_warp_frames_projective(
    const uint8_t* frames, const double* warps, uint8_t* out, uint8_t* inside, int nframes, int w, int h, int noc, int replicate,
    void* stream) {
  return (int)launch_warp_frames_projective(frames, warps, out, inside, nframes, w, h, noc, replicate != 0, (hipStream_t)stream);
}
