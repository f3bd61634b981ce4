#!/bin/sh
# host_sanitize.sh -- the host image readers and writers under AddressSanitizer and UndefinedBehaviorSanitizer.
#
#   tools/host_sanitize.sh [pytest arguments]
#
# Builds tests/c/image_io_probe.cpp + of_dis_amd/csrc/host/image_io.cpp a second time with the sanitizers (the command line of
# of_dis_amd/build.py: io_probe_command, plus the flags below) into a temporary directory and runs tests/test_image_io.py with
# OFDIS_IMAGE_IO_PROBE naming that program.  A report ends the probe with a non-zero status (-fno-sanitize-recover=all), which
# the tests take for a failure and print.  The runtimes are linked statically: the program depends on no load order and
# nothing is preloaded.  Host code only, on a machine without a GPU: the probe links no HIP runtime, and this script is
# neither part of a GPU job nor called from a test.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
dir=$(mktemp -d "${TMPDIR:-/tmp}/ofdis_sanitize.XXXXXX")
trap 'rm -rf "$dir"' EXIT
cd "$root"
python3 - "$dir/image_io_probe" -O1 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
    -static-libasan -static-libubsan <<'EOF'
import subprocess
import sys

from of_dis_amd import build

subprocess.check_call(build.io_probe_command(sys.argv[1], sys.argv[2:]))
EOF
OFDIS_IMAGE_IO_PROBE="$dir/image_io_probe" python3 -m pytest tests/test_image_io.py "$@"
