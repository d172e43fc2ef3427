"""Batches of distinct pictures (TEST INFRASTRUCTURE).

p264hip_reconstruct sets its launch shapes and kernel instances from the whole batch, and inside the kernels a workgroup or
wavefront finds its picture by index arithmetic.  In a batch whose streams all decode the same picture every store holds the same
bytes, so a kernel that takes picture j's offsets, edge info, references or work lists for picture i still writes the right
frame.  A Pool is K synthetic streams of one geometry that differ in what a picture carries (chroma QP offset, loop-filter
offsets and on / off, per-macroblock QP, reference counts, B-picture modes, explicit weights).  Each source is parsed by its own
Parser and its expected frames are computed once: the committed reference (or oracle) hashes where they exist, else the oracle,
the weighted checker for explicit-weight sources.  High-profile sources (8x8 transform, Intra 8x8, scaling matrices), which neither
the oracle nor the reference decodes, are pinned to the standard as tests/scaling_checker.py states it: the committed hashes of
tests/golden/high_pool.json; that checker runs again only to say where a picture that differs does so.

Batch entry j decodes source j % K into stream order[j], a shuffled permutation of the streams: any K consecutive entries (every
k_deblock workgroup of up to K pictures) hold K different sources, and an entry's index is not its stream."""
import hashlib
import json
import os

import numpy as np

from p264decoder_amd import Parser, _native as N
from tests import scaling_checker, synth_cases, wp_checker
from tests.conftest import frame_sha256


def cif(seed, extra="", frames=8, gop=0):
    return "--mbw 22 --mbh 18 --frames %d --gop %d --seed %d --coded 20 --maxlevel 12 %s" % (frames, gop, seed, extra)


def cif_main(seed, extra="", bframes=2):
    return "--mbw 22 --mbh 18 --frames 7 --seed %d --refs 2 --bframes %d --coded 20 --maxlevel 12 %s" % (seed, bframes, extra)


def hd(seed, extra=""):
    return "--mbw 120 --mbh 68 --frames 4 --gop 0 --seed %d --coded 12 --maxlevel 12 --crop-bottom 4 %s" % (seed, extra)


def hd_main(seed, extra="", bframes=2):
    return "--mbw 120 --mbh 68 --frames 7 --seed %d --refs 2 --bframes %d --coded 12 --maxlevel 12 --crop-bottom 4 %s" % (seed, bframes, extra)


def main_11x9(seed, extra="", bframes=2, refs=2, coded=20, maxlevel=2):
    """11 x 9 macroblocks: 5, 3 and 2 loop-filter bands of 2, 4 and 8 rows, the last part-filled at every height; 99 macroblocks = 13
    workgroups of k_t8x8 / k_scaled_inter, the last with 3 macroblocks; an odd width"""
    return "--mbw 11 --mbh 9 --frames 7 --seed %d --refs %d --bframes %d --coded %d --maxlevel %d %s" % (seed, refs, bframes, coded, maxlevel, extra)


def high(seed, extra="", **kw):
    return main_11x9(seed, "--t8x8 70 --i8x8 50 " + extra, **kw)


# A source is a case name of synth_cases (reference- or oracle-pinned) or synth264 arguments (checked by the oracle / checker;
# those of HIGH_SPECS: pinned to scaling_checker.SpecRecon).
# (a) CIF, Baseline, IDR + P pictures (one source has a second IDR at picture 5): k_mc_sort, the fused edge info,
# k_deblock_bs<false>.  Sources 0, 1, 2 and 3 share slice QP 26 with four different pairs of loop-filter offsets.
POOL_P = [
    "cif_ip",
    cif(301, "--qp 26 --deblock-offsets 3 2"),
    cif(302, "--qp 26 --deblock-offsets -4 -3"),
    cif(303, "--qp 26 --deblock-offsets 6 -6"),
    cif(304, "--qp 30 --cqo -7"),
    cif(305, "--qp 32 --cqo 6 --deblock-offsets 2 -2"),
    cif(306, "--nodeblock"),
    cif(307, "--qp 28 --qp-delta 6"),
    cif(308, "--qp 30 --qp-delta 10 --deblock-offsets -2 4 --cqo 3"),
    cif(309, "--refs 2 --qp 24"),
    cif(310, "--refs 3 --mmco --qp 34 --deblock-offsets 5 5"),
    cif(311, "--qp 22", gop=5),
    cif(312, "--qp 38 --deblock-offsets -6 -5 --cqo -3"),
    cif(313, "--qp 29 --qp-delta 4 --refs 2 --sub8x8"),
    cif(314, "--qp 36 --cqo 10 --deblock-offsets 1 3"),
    cif(315, "--qp 18 --deblock-offsets -1 -1"),
    cif(316, "--qp 33 --qp-delta 8 --refs 2 --cqo -5 --deblock-offsets 4 -3"),
]
# (b) CIF, Main, I P B B P B B (two sources with one B picture between reference pictures: steps that mix P and B pictures),
# CAVLC and CABAC, spatial and temporal direct, implicit weights on and off: k_mc_sort_b, k_mc_second, k_deblock_bs<true>.
# Sources 0 and 1 share slice QP 26 with different offsets.
POOL_B = [
    cif_main(401, "--qp 26 --deblock-offsets 3 2 --implicit --d8inf"),
    cif_main(402, "--qp 26 --deblock-offsets -4 -3 --cabac --implicit"),
    cif_main(403, "--temporal"),
    cif_main(404, "--cabac --temporal --implicit"),
    cif_main(405, "--qp 30 --cqo -6 --implicit"),
    cif_main(406, "--qp 32 --cqo 5 --cabac --temporal --deblock-offsets 2 -2"),
    cif_main(407, "--nodeblock --implicit"),
    cif_main(408, "--qp 28 --qp-delta 6 --cabac"),
    cif_main(409, "--refs 3 --qp-delta 8 --deblock-offsets -2 4 --cqo 3"),
    cif_main(410, "--implicit", bframes=1),
    cif_main(411, "--cabac --temporal --qp 34", bframes=1),
    cif_main(412, "--d8inf --temporal --cqo 2 --qp 24"),
    cif_main(413, "--cabac --d8inf --deblock-offsets -6 5 --qp 36"),
    cif_main(414, "--qp 20 --implicit --cabac --refs 3"),
    cif_main(415, "--qp 38 --deblock-offsets 6 6 --temporal --implicit"),
    cif_main(416, "--cabac --qp-delta 4 --cqo -4 --deblock-offsets -1 1"),
    cif_main(417, "--sub8x8 --implicit --qp 29"),
]
# (c) pool (b) plus one source with explicit weights in P and B slices: every step takes k_mc_sort_b_wp / k_mc_sort_wp and k_mc_wp
POOL_WP = POOL_B + [cif_main(418, "--cabac --wp --wp-bi --qp 27")]

# the bench's own batch: 1080p IDR + 3 P pictures; four reference-pinned cases, the others new seeds, offsets, chroma QP offsets,
# no loop filter (hd(501) shares slice QP 26 with cfg3_1080p_allp / cfg3_1080p_ip, other offsets)
POOL_BENCH = [
    "cfg3_1080p_allp", "cfg3_1080p_ip", "cfg3_1080p_ip_l32", "qpd_1080p",
    hd(501, "--qp 26 --deblock-offsets 3 2"),
    hd(502, "--qp 30 --cqo -6 --deblock-offsets -3 -2"),
    hd(503, "--qp 24 --cqo 5 --refs 2"),
    hd(504, "--nodeblock --qp 28"),
    hd(505, "--qp 31 --qp-delta 6 --deblock-offsets -2 4 --cqo 3"),
    hd(506, "--qp 26 --deblock-offsets -5 -4"),
]
# config 4's batch: 1080p Main, I P B B P B B, no explicit weights (main_1080p_cabac_ipb is the case of BASELINE config 4:
# oracle-pinned; its seed-91 stream shares slice QP 26 with hd_main(601))
POOL_CFG4 = [
    "main_1080p_cabac_ipb",
    hd_main(601, "--qp 26 --deblock-offsets 3 2 --implicit --d8inf"),
    hd_main(602, "--cabac --temporal"),
    hd_main(603, "--temporal --implicit --cqo -5"),
    hd_main(604, "--cabac --cqo 4 --deblock-offsets -3 -2 --implicit"),
    hd_main(605, "--nodeblock --cabac --implicit"),
    hd_main(606, "--qp-delta 6 --refs 3 --qp 28"),
    hd_main(607, "--cabac --qp 30 --deblock-offsets 2 -3 --d8inf"),
    hd_main(608, "--cabac --implicit --qp 24", bframes=1),
]

# (d) 11 x 9 macroblocks, High profile without matrices, I P B B P B B: macroblocks with the 8x8 transform (P264_MB_T8X8) and Intra
# 8x8 macroblocks in every P and B picture - k_t8x8, k_intra_i8 / k_intra_sparse_i8, and the loop filter's edge mask for the 8x8
# transform.  Slice QP, --qp-delta and --maxlevel stay where no macroblock leaves 16 bits (tests/golden/make_high_pool.py refuses
# a source that does); most loop-filter offsets are positive so that the filter still has work at these QPs - in most pictures it
# would change hundreds of lines of the inner luma edges that the 8x8 transform takes out (tests/test_distinct_pool_cpu.py counts
# them); source 12 has the filter on with thresholds of 0.  Sources 0 and 1 share slice QP 20 with different offsets.
POOL_HIGH = [
    high(801, "--qp 20 --deblock-offsets 3 2 --implicit --d8inf"),
    high(802, "--qp 20 --deblock-offsets -4 -3 --cabac --implicit"),
    high(803, "--qp 18 --temporal --deblock-offsets 6 6"),
    high(804, "--qp 16 --cabac --temporal --implicit --deblock-offsets 5 4"),
    high(805, "--qp 20 --cqo -6 --implicit --deblock-offsets 6 3"),
    high(806, "--qp 19 --cqo 5 --cabac --temporal --deblock-offsets 2 -2"),
    high(807, "--qp 18 --nodeblock --implicit"),
    high(187, "--qp 20 --qp-delta 3 --deblock-offsets 3 2 --cqo -4"),
    high(822, "--qp 14 --qp-delta 2 --deblock-offsets -2 4 --cqo 3", refs=3),
    high(810, "--qp 17 --implicit --deblock-offsets 4 6", bframes=1),
    high(811, "--cabac --temporal --qp 20 --deblock-offsets 6 5", bframes=1),
    high(812, "--d8inf --temporal --cqo 2 --qp 12 --deblock-offsets 6 6"),
    high(813, "--cabac --d8inf --deblock-offsets -6 5 --qp 20"),
    high(814, "--qp 10 --implicit --cabac --deblock-offsets 6 6", refs=3, maxlevel=3),
    high(815, "--qp 20 --deblock-offsets 6 6 --temporal --implicit", coded=30),
    high(816, "--cabac --qp 16 --qp-delta 3 --cqo -4 --deblock-offsets -1 1"),
    high(817, "--sub8x8 --implicit --qp 19 --deblock-offsets 5 5"),
]
# (e) pictures with scaling matrices beside flat ones, alternating: nine sources whose SPS, PPS or both carry the default (JVT) or
# random lists - one of them with explicit weights in P and B slices -, eight flat sources of pool (d), which a batch with a scaled
# picture gives the all-16 table and whose 8x8 blocks k_scaled_inter then owns, and one Main source without any 8x8 block:
# k_mc_sort_scaled and k_mc_wp (every step behind the IDR holds a picture with explicit weights), k_scaled_inter, k_intra_scaled /
# k_intra_sparse_scaled.  Sources 0 and 12 share slice QP 12 with different offsets.
POOL_SCALED = [
    high(701, "--cabac --qp 12 --cqm jvt --cqm-where sps --deblock-offsets 6 4", coded=30, maxlevel=3),
    POOL_HIGH[0],
    high(702, "--qp 13 --cqm rand:5 --cqm-where pps --cqo -4 --deblock-offsets 6 6", coded=30),
    POOL_HIGH[1],
    high(703, "--cabac --qp 16 --cqm rand:6 --cqm-where both --wp --wp-bi --deblock-offsets 5 6", coded=30),
    POOL_HIGH[3],
    high(704, "--qp 8 --qp-delta 2 --cqm jvt --cqm-where pps --temporal --implicit --cqo 5 --deblock-offsets 6 6", coded=30),
    POOL_HIGH[5],
    high(705, "--cabac --qp 20 --cqm rand:8 --cqm-where sps --nodeblock --d8inf", coded=30, maxlevel=1),
    main_11x9(901, "--qp 20 --implicit --deblock-offsets 4 3"),
    high(706, "--cabac --qp 14 --cqm jvt --cqm-where both --implicit --deblock-offsets 6 3", bframes=1, coded=30),
    POOL_HIGH[8],
    high(707, "--qp 12 --cqm rand:9 --cqm-where sps --deblock-offsets 6 6 --temporal", refs=3, coded=30),
    POOL_HIGH[10],
    high(708, "--cabac --qp 18 --cqm rand:11 --cqm-where pps --deblock-offsets 5 4 --implicit", coded=30, maxlevel=1),
    POOL_HIGH[12],
    high(709, "--qp 16 --cqm rand:12 --cqm-where both --cqo -3 --deblock-offsets 6 2", coded=25),
    POOL_HIGH[14],
]
# (f) pool (e) with its explicit-weight source replaced by the same arguments without weights: no batch of pool (e) is without an
# explicit-weight picture behind the IDR, so it always takes k_mc_sort_scaled and k_mc_wp; here the step of P pictures takes
# k_mc_sort_scaled_p and k_mc, the steps with B pictures k_mc_sort_scaled, k_mc and k_mc_second
POOL_SCALED_PLAIN = [s.replace("--wp --wp-bi ", "") for s in POOL_SCALED]
assert sum(a != b for a, b in zip(POOL_SCALED, POOL_SCALED_PLAIN)) == 1
# four streams of one size and one frame-store depth for the pipeline (tests/test_gpu_pipeline.py, tests/test_pipeline_cpu.py)
PIPELINE_HIGH = {"scaled cabac b": POOL_SCALED[0], "scaled weighted": POOL_SCALED[4], "flat high": POOL_HIGH[0], "main": POOL_SCALED[9]}
# the sources whose expectation is the standard's (tests/scaling_checker.py: SpecRecon), committed in tests/golden/high_pool.json -
# the oracle and the reference know neither the 8x8 transform nor scaling lists
HIGH_SPECS = list(dict.fromkeys(POOL_HIGH + POOL_SCALED + POOL_SCALED_PLAIN))


HIGH_GOLDEN = os.path.join(synth_cases.GOLDEN, "high_pool.json")
_high_golden = {}


def high_golden(spec):
    """(stream sha256, [per-picture sha256 of SpecRecon's output]) of a source of HIGH_SPECS, from tests/golden/high_pool.json"""
    if not _high_golden:
        with open(HIGH_GOLDEN) as f:
            _high_golden.update(json.load(f)["sources"])
    return _high_golden[spec]["stream"], _high_golden[spec]["frames"]


def read_stream(args):
    with open(synth_cases.generate(args), "rb") as f:
        return f.read()


def stream_of(spec):
    """(stream bytes, committed per-picture hashes or None)"""
    if spec in synth_cases.CASES:
        digest, hashes = synth_cases.golden(spec)
        data = synth_cases.stream_bytes(spec)
    elif spec in synth_cases.ORACLE_CASES:
        digest, hashes = synth_cases.oracle_golden(spec)
        data = read_stream(synth_cases.ORACLE_CASES[spec])
    elif spec in HIGH_SPECS:
        digest, hashes = high_golden(spec)
        data = read_stream(spec)
    else:
        return read_stream(spec), None
    assert hashlib.sha256(data).hexdigest() == digest, "%s: the stream writer no longer writes the pinned stream" % spec
    return data, hashes


def spec_frames(pics, slots, tells=None):
    """[[y, u, v]] of the pictures by the standard (scaling_checker.SpecRecon: 8x8 transform, Intra 8x8, scaling lists); OutOfRange
    where a macroblock has no defined result.  tells: a list that gets, per picture, how many lines of the inner luma edges 1 and 3
    of macroblocks with the 8x8 transform the loop filter would have changed had it not left them alone (t8x8_checker.deblock)"""
    chk = scaling_checker.SpecRecon(pics[0].mb_w, pics[0].mb_h, slots)
    out = []
    for p in pics:
        before = sum(chk.tells.values())
        out.append([a.copy() for a in chk.reconstruct(p)])
        if tells is not None:
            tells.append(sum(chk.tells.values()) - before)
    return out


class Source:
    def __init__(self, lib, spec, n_pictures):
        self.spec = spec
        self.high = spec in HIGH_SPECS                  # parsed for a backend that knows Intra 8x8 records and reads the lists
        data, self.pinned = stream_of(spec)
        parser = Parser(quiet=True, lib=lib, intra8x8=self.high, scaling=self.high)
        self.pics = parser.parse_stream(data, limit=n_pictures)
        self.slots = parser.slots
        parser.close()
        assert len(self.pics) == n_pictures, "%s: %d pictures" % (spec, len(self.pics))
        self.hashes, self.frames = None, None

    def expect(self, oracle=None):
        """the expected frame of every picture: committed hashes, else the oracle / weighted checker (frames kept for messages)"""
        if self.pinned is not None:
            self.hashes = self.pinned[:len(self.pics)]
            return
        p0 = self.pics[0]
        chk = wp_checker.WeightedChecker(oracle, p0.mb_w, p0.mb_h, self.slots)
        self.frames = [[a.copy() for a in chk.reconstruct(p)] for p in self.pics]
        self.hashes = [frame_sha256(*f) for f in self.frames]

    def check(self, step, got, what):
        if frame_sha256(*got) == self.hashes[step]:
            return
        msg = "%s: source %s picture %d (slice type %d) differs" % (what, self.spec, step, self.pics[step].desc.slice_type)
        if self.frames is None and self.high:           # (only now: the checker takes seconds per source)
            self.frames = spec_frames(self.pics, self.slots)
            if frame_sha256(*self.frames[step]) != self.hashes[step]:
                msg += " (from the committed hash too: the checker's picture is not the one of tests/golden/high_pool.json)"
        if self.frames is not None:
            for plane, (a, b) in enumerate(zip(got, self.frames[step])):
                if not np.array_equal(a, b):
                    ys, xs = np.nonzero(a != b)
                    msg += "; plane %d: %d samples, first (y=%d,x=%d) got %d want %d" % (plane, len(ys), ys[0], xs[0], a[ys[0], xs[0]], b[ys[0], xs[0]])
                    break
        raise AssertionError(msg)


class Pool:
    def __init__(self, lib, specs, n_pictures, oracle=None):
        self.sources = [Source(lib, s, n_pictures) for s in specs]
        self.K = len(specs)
        self.n_pictures = n_pictures
        p0 = self.sources[0].pics[0]
        self.mb_w, self.mb_h = p0.mb_w, p0.mb_h
        assert all((s.pics[0].mb_w, s.pics[0].mb_h) == (self.mb_w, self.mb_h) for s in self.sources)
        self.slots = max(s.slots for s in self.sources)
        if oracle is not None:
            for s in self.sources:
                s.expect(oracle)

    def order(self, S, seed):
        """order[j] = the stream of batch entry j (which decodes source j % K); shuffled"""
        return [int(x) for x in np.random.default_rng(seed).permutation(S)]

    def step_pictures(self, step):
        return [s.pics[step] for s in self.sources]

    def workgroups(self, S, per_wg):
        """the sources of each k_deblock workgroup of a batch of S entries, per_wg pictures per workgroup"""
        return [[j % self.K for j in range(w, min(w + per_wg, S))] for w in range(0, S, per_wg)]

    def run(self, hip, S, seed, on_step=None):
        """every picture of every source through `hip` (S streams, K input slots), entry j = source j % K on stream order[j];
        on_step(step, launch info, pictures of the step) after each call; every stream of every step checked"""
        order = self.order(S, seed)
        ids = [j % self.K for j in range(S)]
        for t in range(self.n_pictures):
            pics = self.step_pictures(t)
            hip.upload(0, pics)
            hip.reconstruct(ids, order)
            hip.sync()
            if on_step:                                      # (the launch shapes, and what the batch's content launched)
                on_step(t, dict(hip.last_launch(), t8x8_wgs=hip.last_t8x8_wgs(), intra_i8=hip.last_intra_i8(), scaled_pictures=hip.last_scaled_pictures()), pics)
            for j, s in enumerate(order):
                k = j % self.K
                self.sources[k].check(t, hip.read_frame(s, pics[k].desc.dst_slot), "entry %d (source %d) stream %d" % (j, k, s))


def expected_edge_info_fused(pics, knob=None):
    """edge_info_fused of a batch: 0 with any I, B or explicit-weight picture, a P picture whose list holds one frame at several
    indices, or a picture with the 8x8 transform or scaling lists - the fused role has no edge mask - (own k_deblock_bs launch), else
    the knob or 1"""
    if any(p.desc.slice_type != N.SLICE_P or p.desc.explicit_wp or len(set(p.desc.ref_slot[:p.desc.n_ref])) < p.desc.n_ref or
           p.desc.transform_8x8 or p.desc.scaling_lists for p in pics):
        return 0
    return 1 if knob is None else int(knob)


def expected_inter_instances(pics):
    """the kernels of a batch's inter stage by launch_inter's rule (p264hip.hip): the sort by what the batch holds (scaling lists, B
    pictures, explicit weights), k_mc_wp with explicit weights, k_mc_second with B pictures; none for I pictures only.  The launch
    info does not name these kernels: this says what a batch of these pictures selects, not what was observed"""
    d = [p.desc for p in pics]
    if all(x.slice_type == N.SLICE_I for x in d):
        return ()
    b, wp = any(x.slice_type == N.SLICE_B for x in d), any(x.explicit_wp for x in d)
    if any(int(x.scaling_lists) for x in d):
        sort = "k_mc_sort_scaled" if b or wp else "k_mc_sort_scaled_p"
    else:
        sort = ("k_mc_sort_b" if b else "k_mc_sort") + ("_wp" if wp else "")
    return (sort, "k_mc_wp" if wp else "k_mc") + (("k_mc_second",) if b else ())
