#!/usr/bin/env python3
"""tests/golden/high_pool.json: per source of the High-profile pools of tests/distinct_pool.py (POOL_HIGH, POOL_SCALED, POOL_SCALED_PLAIN) the SHA-256
of the stream and the per-picture SHA-256 of what H.264 says the pictures are, by tests/scaling_checker.py (SpecRecon: 8x8
transform, Intra 8x8, scaling lists - the oracle and the reference decode none of them).  The hashes let the GPU tests compare
without running the checker, which takes seconds per source.

H.264 defines no result for a macroblock with an intermediate value outside 16 bits: a source with one such macroblock in any
picture is refused (pick another seed, a lower --qp, --qp-delta or --maxlevel), so that no macroblock is ever left out of a
comparison."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from p264decoder_amd import Parser                      # noqa: E402
from tests import distinct_pool, scaling_checker        # noqa: E402
from tests.conftest import frame_sha256                # noqa: E402

N_PICTURES = 7
out = {}
for spec in distinct_pool.HIGH_SPECS:
    data = distinct_pool.read_stream(spec)
    parser = Parser(quiet=True, intra8x8=True, scaling=True)
    pics, slots = parser.parse_stream(data), parser.slots
    parser.close()
    assert len(pics) == N_PICTURES, "%s: %d pictures" % (spec, len(pics))
    for i, p in enumerate(pics):
        bad = scaling_checker.census(p)[1]
        if bad:
            sys.exit("%s: picture %d has %d level blocks that feed a value out of range, first %s" % (spec, i, len(bad), sorted(bad, key=str)[:3]))
    frames = distinct_pool.spec_frames(pics, slots)
    out[spec] = {"stream": hashlib.sha256(data).hexdigest(), "frames": [frame_sha256(*f) for f in frames]}
    print("%d pictures, %d with lists: %s" % (len(pics), sum(bool(int(p.desc.scaling_lists)) for p in pics), spec))
with open(distinct_pool.HIGH_GOLDEN, "w") as f:
    json.dump({"checker": "tests/scaling_checker.py: SpecRecon", "sources": out}, f, indent=1)
    f.write("\n")
