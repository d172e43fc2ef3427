"""Records tests/golden/launch_shapes.json: p264hip_last_launch() of every case of tests/test_gpu_launch_shapes.py, on an MI355X.
Run it in a worktree of the commit whose launch shapes are to be pinned (with this script and the test copied in):
    python tests/golden/make_launch_shapes.py [output.json]
The table is only written if it covers what the test is there for (asserted below)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from p264decoder_amd import _native  # noqa: E402
from tests import test_gpu_launch_shapes as T  # noqa: E402


def main():
    lib = _native.load()
    for name in list(os.environ):
        if name.startswith(T.K):
            del os.environ[name]
    cases, units = {}, None
    for case in T.CASES:
        li = T.run_case(lib, case, os.environ.__setitem__)
        for k in case[3]:
            del os.environ[k]
        units = units or li["compute_units"]
        assert li["compute_units"] == units
        cases[T.case_id(case)] = li
        print(T.case_id(case), li, flush=True)
    assert len(cases) == len(T.CASES), "two cases share an id"
    rows = list(zip(T.CASES, cases.values()))
    plain = [(c, li) for c, li in rows if not c[3]]                      # no knob: the built-in choices
    assert {c[1] for c, _ in plain} == set(T.SIZES)
    assert {li["deblock_pics_per_wg"] for _, li in plain} >= {1, 2, 3, 4, 5, 6}
    assert len({li["intra_waves"] for _, li in plain}) == 3
    assert {li["deblock_rb_log2"] for _, li in rows} >= {2, 3}
    assert {li["deblock_odd_single"] for _, li in rows} == {0, 1}
    assert {li["deblock_odd_single"] for _, li in plain} == {0, 1}      # (chosen by the cost comparison, not only by the knob)
    assert any(li["edge_info_fused"] == 0 for _, li in rows) and any(li["edge_info_fused"] > 0 for _, li in rows)
    # motion-compensation workgroups per picture: compute units * 48 / pictures, at least 48, at most what the geometry's work
    # lists can hold in chunks - 48 in a batch that would get fewer is the floor, anything below 48 is the max_chunks cap
    assert any(li["mc_wgs_per_picture"] == 48 and (units * 48 + c[1] - 1) // c[1] < 48 for c, li in plain), "no case at the floor"
    assert any(0 < li["mc_wgs_per_picture"] < 48 for _, li in plain), "no case at the max_chunks cap"
    assert any(li["mc_wgs_per_picture"] == 0 for _, li in rows)          # (I pictures only: no inter launch)
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with open(out, "w") as f:
        json.dump({"compute_units": units, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases on %d compute units" % (out, len(cases), units))


if __name__ == "__main__":
    main()
