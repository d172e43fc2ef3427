#!/usr/bin/env python3
"""Records tests/golden/parse_corpus.json: the outcomes of tests/parse_corpus.py from the library of the tree this runs in.  The
file pins a parser that must not change what it computes, so it is recorded from the commit BEFORE such a change: in a worktree of
that commit, with tests/parse_corpus.py, tests/test_parse_corpus_cpu.py and this file copied in,

    python tests/golden/make_parse_corpus.py && python -m pytest tests/test_parse_corpus_cpu.py -q

and the JSON copied back."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from p264decoder_amd import _native, build      # noqa: E402
from tests import parse_corpus                  # noqa: E402

build.build()
rec = parse_corpus.record(_native.load())
with open(parse_corpus.GOLDEN, "w") as f:
    json.dump(rec, f, indent=0, separators=(",", ":"))
    f.write("\n")
clean = [o for v in rec["clean"].values() for o in v]
print("%d streams, %d NALs, %d pictures; %d damaged copies -> %s" % (len(rec["clean"]), len(clean), sum(len(o) == 16 for o in clean),
                                                                      sum(len(v) for v in rec["damaged"].values()), parse_corpus.GOLDEN))
