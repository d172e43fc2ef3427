#!/usr/bin/env python3
"""tests/golden/limit_geometry.json: per picture of tests/limit_geometry.py whose expectation is too slow for a GPU test
(golden_pictures(): pictures with explicit weights above IN_TEST_MB macroblocks by tests/wp_checker.py, High-profile pictures by
tests/scaling_checker.py's SpecRecon, those with a Cr offset by cr_offset_checker.TwoChains over it) seam_fuzz.picture_digest of the drawn picture and the SHA-256 of every plane of what H.264 says
it is.  A High-profile picture with a level block that feeds a value outside 16 bits is refused, as tests/golden/make_high_pool.py
refuses such a source: no macroblock is ever left out of a comparison."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import cr_offset_checker, hip_harness, limit_geometry as L, oracle_bind, scaling_checker, seam_fuzz        # noqa: E402

oracle = oracle_bind.load()
out = {}
for key, st, checker in L.golden_pictures():
    t = time.time()
    if checker in ("SpecRecon", "TwoChains"):
        for cr in ((False, True) if checker == "TwoChains" else (False,)):
            with cr_offset_checker.variant(st.pic, cr):
                bad = scaling_checker.census(st.pic)[1]
            if bad:
                sys.exit("%s: %d level blocks feed a value out of range, first %s" % (key, len(bad), sorted(bad, key=str)[:3]))
        if checker == "TwoChains":
            two = cr_offset_checker.TwoChains(scaling_checker.SpecRecon, st.pic.mb_w, st.pic.mb_h, L.SLOTS)
            for slot, f in st.frames.items():
                two.store.write(slot, f)
            planes = two.reconstruct(st.pic)
            assert two.v_differs, "%s: Cr's offset changes nothing" % key
        else:
            planes = hip_harness.expect(st, scaling_checker.SpecRecon, L.SLOTS)
    else:
        planes = L.expected(oracle, st)
    out[key] = {"checker": checker, "digest": seam_fuzz.picture_digest(st.pic), "planes": L.plane_hashes(planes)}
    print("%-60s %5d macroblocks %6.1f s" % (key, st.pic.n_mb, time.time() - t))
with open(L.GOLDEN, "w") as f:
    json.dump({"pictures": out}, f, indent=1, sort_keys=True)
    f.write("\n")
