#!/bin/sh
# host_sanitize.sh -- the host code that runs without a device, under the host sanitizers.
#
#   tools/host_sanitize.sh [pytest arguments]
#
# 1. The image readers and writers: tests/c/image_io_probe.cpp + of_dis_amd/csrc/host/image_io.cpp built a second time with
#    AddressSanitizer and UndefinedBehaviorSanitizer (the command line of of_dis_amd/build.py: io_probe_command, plus the flags
#    below) into a temporary directory; tests/test_image_io.py runs with OFDIS_IMAGE_IO_PROBE naming that program.
# 2. The sequence driver on the host-only stand-in for the library (tests/c/ofdis_abi_stub.c; build.py: seq_stub_commands):
#    one pair of programs with AddressSanitizer + UBSan, a second pair with ThreadSanitizer; tests/test_seq_driver_stub.py runs
#    once against each, with OFDIS_SEQ_STUB_DIR naming the directory.
#    What ThreadSanitizer shows on a synchronous stub: the hand-over of chunk buffers between the reader, the device stage and
#    the writer of a share through the three queues, the decode / write workers, and the flags the threads share.  What it
#    does not show: the lifetime of a buffer under an asynchronous copy -- in the stub a copy has finished when the call
#    returns, on a device it runs until its stream is drained.  That order is kept by the driver's drain before release and
#    by the byte-for-byte GPU tests (tests/test_gpu_seq_cli.py), not by this script.
#
# A report ends a program with a non-zero status (-fno-sanitize-recover=all; ThreadSanitizer: its own exit status 66), which
# the tests take for a failure and print.  The runtimes are linked statically: the programs depend on no load order and
# nothing is preloaded.  Host code only, on a machine without a GPU: no program here links the HIP runtime, and this script
# is neither part of a GPU job nor called from a test.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
dir=$(mktemp -d "${TMPDIR:-/tmp}/ofdis_sanitize.XXXXXX")
trap 'rm -rf "$dir"' EXIT
cd "$root"
mkdir "$dir/asan" "$dir/tsan"
python3 - "$dir" <<'EOF'
import subprocess
import sys

from of_dis_amd import build

ASAN = ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
        "-static-libubsan"]
TSAN = ["-O1", "-fno-omit-frame-pointer", "-fsanitize=thread", "-static-libtsan"]
subprocess.check_call(build.io_probe_command(sys.argv[1] + "/image_io_probe", ASAN))
for sub, flags in (("asan", ASAN), ("tsan", TSAN)):
    for name in build.SEQ_STUB_PROGRAMS:
        for cmd in build.seq_stub_commands(f"{sys.argv[1]}/{sub}/{name}", name, flags):
            subprocess.check_call(cmd)
EOF
OFDIS_IMAGE_IO_PROBE="$dir/image_io_probe" python3 -m pytest tests/test_image_io.py "$@"
OFDIS_SEQ_STUB_DIR="$dir/asan" python3 -m pytest tests/test_seq_driver_stub.py "$@"
OFDIS_SEQ_STUB_DIR="$dir/tsan" python3 -m pytest tests/test_seq_driver_stub.py "$@"
