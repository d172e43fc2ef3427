"""Every header under csrc/hip/ includes what it uses: each one passes a device-side syntax check for gfx950 on its own, so no
header compiles only because of the order in which p264hip.hip happens to include the others (kernel_intra.h did for a long
time: it took its residual arithmetic and buffer helpers from kernel_mc.h without including it).  No GPU needed."""
import glob
import os
import subprocess

import pytest

from p264decoder_amd import build

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.HIP_DIR, "*.h")))


@pytest.fixture(scope="module")
def hipcc():
    try:
        return build._hipcc()
    except RuntimeError as e:                         # no ROCm compiler on this machine
        pytest.skip(str(e))


def test_there_are_headers():
    assert "kernel_mc.h" in HEADERS and "device_common.h" in HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(hipcc, header):
    r = subprocess.run([hipcc, "--offload-arch=" + build.HIP_ARCH, "-std=c++17", "-I", build.INC, "-I", build.HIP_DIR,
                        "--cuda-device-only", "-fsyntax-only", "-x", "hip", os.path.join(build.HIP_DIR, header)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, "%s does not compile on its own:\n%s" % (header, r.stdout[-4000:])
