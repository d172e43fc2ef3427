"""Intra prediction under every neighbour availability on the MI355X, against tests/intra_checker.py (written from H.264 8.3, not
from the oracle or the kernels): pictures of seam_fuzz.make_picture(avail_mode="free") - the four `avail` flags of a macroblock
drawn independently, as constrained intra prediction produces them in a picture's interior (LEFT off with TOPLEFT on, TOPRIGHT
off with everything else on ...) - and the directed slice construction seam_fuzz.make_directed (LEFT, TOP, no TOPLEFT: where the
reference's DC fall-back, SURVEY A-Q7, and the standard's differ).  P, B, weighted-B pictures and pictures with I_PCM through
p264hip_reconstruct in batches of three streams; every family once as a batch of P / B pictures only (k_intra_sparse) and once
with an I picture in the batch (dense k_intra); the streams of a batch go into their input slots by the plain, the packed and
the compact upload.  Bytes of all three planes, every picture, nothing filtered.  The coverage figures come from the drawn
pictures (`draw`), so the CPU twin (test_intra_avail_cpu.py) asserts the same without a device."""
import pytest

from p264decoder_amd import _native as N
from tests import intra_checker
from tests.hip_harness import compare, put, reconstructor
from tests.intra_avail_stim import DST, FAMILIES, ROADS, S, SLOTS, check_coverage, check_directed, draw_1080p, prepare, survey_all


@pytest.mark.gpu
@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_intra_availability(lib, oracle, name, with_i):
    mb_w, mb_h = FAMILIES[name][:2]
    batch, log = prepare(oracle, name, with_i)
    with reconstructor(lib, mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S) as hip:
        first = list(FAMILIES).index(name) + with_i
        for s, (pic, f, want) in enumerate(batch):
            for slot in range(DST):
                hip.write_frame(s, slot, *f)
            put(hip, lib, s, pic, ROADS[(first + s) % 3])
        hip.reconstruct(list(range(S)), list(range(S)))
        for s, (pic, f, want) in enumerate(batch):
            compare(hip.read_frame(s, DST), want, "%s stream %d by %s" % (name, s, ROADS[(first + s) % 3]), pic)
    if "directed" in name:
        check_directed(name, with_i, batch, log)


@pytest.mark.gpu
def test_coverage_behind_the_gpu_comparison():
    check_coverage(survey_all())


@pytest.mark.gpu
def test_intra_availability_1080p_batch(lib, oracle):
    mb_w, mb_h = 120, 68
    with reconstructor(lib, mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S) as hip:
        batch = []
        for s, (pic, f, _) in enumerate(draw_1080p()):
            chk = intra_checker.IntraChecker(oracle, mb_w, mb_h, SLOTS)
            for slot in range(DST):
                for dst, src in zip(chk.store[slot], f):
                    dst[:] = src
                hip.write_frame(s, slot, *f)
            assert len({int(a) for a in pic.rec["avail"][pic.rec["mb_type"] <= N.MB_IPCM]}) == 16
            batch.append((pic, [a.copy() for a in chk.reconstruct(pic)]))
            put(hip, lib, s, pic, ROADS[s])
        hip.reconstruct(list(range(S)), list(range(S)))
        for s, (pic, want) in enumerate(batch):
            compare(hip.read_frame(s, DST), want, "1080p stream %d" % s, pic)
