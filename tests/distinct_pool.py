"""Batches of distinct pictures (TEST INFRASTRUCTURE).

p264hip_reconstruct sets its launch shapes and kernel instances from the whole batch, and inside the kernels a workgroup or
wavefront finds its picture by index arithmetic.  In a batch whose streams all decode the same picture every store holds the same
bytes, so a kernel that takes picture j's offsets, edge info, references or work lists for picture i still writes the right
frame.  A Pool is K synthetic streams of one geometry that differ in what a picture carries (chroma QP offset, loop-filter
offsets and on / off, per-macroblock QP, reference counts, B-picture modes, explicit weights).  Each source is parsed by its own
Parser and its expected frames are computed once: the committed reference (or oracle) hashes where they exist, else the oracle,
the weighted checker for explicit-weight sources.

Batch entry j decodes source j % K into stream order[j], a shuffled permutation of the streams: any K consecutive entries (every
k_deblock workgroup of up to K pictures) hold K different sources, and an entry's index is not its stream."""
import hashlib

import numpy as np

from p264decoder_amd import Parser, _native as N
from tests import synth_cases, wp_checker
from tests.conftest import frame_sha256


def cif(seed, extra="", frames=8, gop=0):
    return "--mbw 22 --mbh 18 --frames %d --gop %d --seed %d --coded 20 --maxlevel 12 %s" % (frames, gop, seed, extra)


def cif_main(seed, extra="", bframes=2):
    return "--mbw 22 --mbh 18 --frames 7 --seed %d --refs 2 --bframes %d --coded 20 --maxlevel 12 %s" % (seed, bframes, extra)


def hd(seed, extra=""):
    return "--mbw 120 --mbh 68 --frames 4 --gop 0 --seed %d --coded 12 --maxlevel 12 --crop-bottom 4 %s" % (seed, extra)


def hd_main(seed, extra="", bframes=2):
    return "--mbw 120 --mbh 68 --frames 7 --seed %d --refs 2 --bframes %d --coded 12 --maxlevel 12 --crop-bottom 4 %s" % (seed, bframes, extra)


# A source is a case name of synth_cases (reference- or oracle-pinned) or synth264 arguments (checked by the oracle / checker).
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


def stream_of(spec):
    """(stream bytes, committed per-picture hashes or None)"""
    if spec in synth_cases.CASES:
        digest, hashes = synth_cases.golden(spec)
        data = synth_cases.stream_bytes(spec)
    elif spec in synth_cases.ORACLE_CASES:
        digest, hashes = synth_cases.oracle_golden(spec)
        data = open(synth_cases.generate(synth_cases.ORACLE_CASES[spec]), "rb").read()
    else:
        return open(synth_cases.generate(spec), "rb").read(), None
    assert hashlib.sha256(data).hexdigest() == digest, "%s: the stream writer no longer writes the pinned stream" % spec
    return data, hashes


class Source:
    def __init__(self, lib, spec, n_pictures):
        self.spec = spec
        data, self.pinned = stream_of(spec)
        parser = Parser(quiet=True, lib=lib)
        self.pics = parser.parse_stream(data, limit=n_pictures)
        self.slots = parser.slots
        parser.close()
        assert len(self.pics) == n_pictures, "%s: %d pictures" % (spec, len(self.pics))
        self.hashes, self.frames = None, None

    def expect(self, oracle):
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
            if on_step:
                on_step(t, hip.last_launch(), pics)
            for j, s in enumerate(order):
                k = j % self.K
                self.sources[k].check(t, hip.read_frame(s, pics[k].desc.dst_slot), "entry %d (source %d) stream %d" % (j, k, s))


def expected_edge_info_fused(pics, knob=None):
    """edge_info_fused of a batch: 0 with any I, B or explicit-weight picture, or a P picture whose list holds one frame at several
    indices (own k_deblock_bs launch), else the knob or 1"""
    if any(p.desc.slice_type != N.SLICE_P or p.desc.explicit_wp or len(set(p.desc.ref_slot[:p.desc.n_ref])) < p.desc.n_ref for p in pics):
        return 0
    return 1 if knob is None else int(knob)
