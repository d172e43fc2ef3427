"""The host drivers under the sanitizers, as a stand-alone program (tests/tools/host_drivers_main.c: a two-rank fan-out over
TCP inside one process and the parse-only pipeline on three threads, the HIP layer stubbed out).  Built twice with gcc - once
with AddressSanitizer and UBSan, once with ThreadSanitizer - and run as a plain child process: exit status 0 (the frames of the
stream that travelled equal those of the one that stayed, every picture count is right) and no sanitizer report."""
import os
import subprocess

import pytest

from tests import synth_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "p264decoder_amd", "csrc", "host")
HOST_SRCS = ["parser.c", "vlc.c", "cabac.c", "dropin.c", "pipeline.c", "fanout.c", "input_layout.c", "export_layout.c", "compact.c", "cpu_check.c"]
REPORTS = ("AddressSanitizer", "runtime error:", "ThreadSanitizer")


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_host_drivers_under_sanitizer(lib, tmp_path, sanitize):
    if lib.p264hip_device_count() > 0:
        pytest.skip("a HIP device is present: sanitizer runs belong on the CPU machine")
    exe = str(tmp_path / "host_drivers_main")
    srcs = [os.path.join(HOST_DIR, s) for s in HOST_SRCS] + [os.path.join(ROOT, "tests", "tools", s) for s in ("hip_stub.c", "host_drivers_main.c")]
    subprocess.run(["gcc", "-O0", "-g", "-std=gnu11", "-fsanitize=" + sanitize, "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                    "-I" + HOST_DIR] + srcs + ["-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe, "-n", "12", os.path.join(ROOT, "tests", "golden", "f26.264"), synth_cases.generate("cif_ip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert not any(word in r.stdout for word in REPORTS), r.stdout
    assert "fan-out: 48 pictures in 12 rounds, 24 through the worker" in r.stdout and "pipeline: 48 pictures" in r.stdout, r.stdout
