"""A plain `bench.py` run (no --full) as every pull request's measurement runs it: exactly --steps timed steps, the contract's
fields in the one JSON line, and with --dump-outputs the frames the last timed step decoded.  With 4 streams every stream is
dumped, and stream 0 is the golden all-P stream: its frame must hash to what the real reference decoder produced for that
picture (tests/golden/synth_cfg3_1080p_allp.sha256)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import synth_cases
from tests.conftest import frame_sha256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_what_the_last_step_decoded(lib, tmp_path):
    S, K, W = 4, 3, 1
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(S), "--steps", str(K), "--warmup", str(W),
                          "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["metric"] == "1080p decoded frames/sec" and r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "int16"
    assert r["steps"] == K and r["warmup"] == W and r["ranks"][0]["frames"] == S * K
    assert abs(r["value"] - S * K / (r["ms_per_step"] * K * 1e-3)) < 0.01 * r["value"]
    assert not {"extras", "cpu_baseline", "kernels", "roofline", "golden_check"} & set(r)        # --full only
    planes = [np.load(str(tmp_path / (n + ".npy"))) for n in ("frame_y", "frame_u", "frame_v")]
    assert [p.dtype for p in planes] == [np.float32] * 3
    assert [p.shape for p in planes] == [(S, 1088, 1920), (S, 544, 960), (S, 544, 960)]
    hashes = synth_cases.golden("cfg3_1080p_allp")[1]
    assert frame_sha256(*(p[0].astype(np.uint8) for p in planes)) == hashes[1 + W + K - 1]
