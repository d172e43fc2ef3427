#!/usr/bin/env python3
"""Records what tests/test_abi.py holds the drop-in's binary contract to, from the REAL reference (build container only:
needs the reference tree and oracle/_ref/libp264ref_kat.so, `make -C oracle ref`):

    python tests/golden/make_ref_abi.py <reference tree>

  ref_dropin_layout.txt    sizes and offsets of p264_param_t / p264_picture_t / p264_image_t / p264_nal_t through its p264.h
  ref_param_default.json   every field its p264_param_default fills in (core/core.c:41-137), on a struct pre-filled with 0x55
  ref_cli_symbols.txt      the p264_* symbols its command-line caller (p264decoder.c) leaves undefined when linked against
                           libp264amd.so

Only these values are written, nothing of the reference's text."""
import ctypes as C
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from p264decoder_amd import _native as N          # noqa: E402
from p264decoder_amd import build                 # noqa: E402
from p264decoder_amd import decoder as D          # noqa: E402
from tests import test_abi as T                   # noqa: E402

ref = sys.argv[1]
build.build()
N.load()

with open(os.path.join(HERE, "ref_dropin_layout.txt"), "w") as f:
    f.write(T.dropin_layout(ref, "p264.h"))

kat = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libp264ref_kat.so"))
p = D.Param()
C.memset(C.byref(p), 0x55, C.sizeof(p))
kat.p264_param_default(C.byref(p))
with open(os.path.join(HERE, "ref_param_default.json"), "w") as f:
    json.dump(T.param_values_json(p), f, indent=0, sort_keys=True)
    f.write("\n")

with tempfile.TemporaryDirectory() as td:
    exe, cc = T.compile_reference_cli(ref, td)
    if cc.returncode != 0:
        raise SystemExit(cc.stdout)
    with open(os.path.join(HERE, "ref_cli_symbols.txt"), "w") as f:
        f.write("".join(s + "\n" for s in sorted(T.undefined_p264_symbols(exe))))
print("ref_dropin_layout.txt, ref_param_default.json, ref_cli_symbols.txt written")
