"""The parse of every stream the suite has, NAL by NAL, and of damaged copies of them (TEST INFRASTRUCTURE): what
tests/test_parse_corpus_cpu.py compares with tests/golden/parse_corpus.json, recorded by tests/golden/make_parse_corpus.py from the
library of the commit BEFORE the parser's state was regrouped.  The streams are the synth264 argument strings of the other test
modules, imported; a damaged copy has a few bytes overwritten and is fed to the end, past every refusal: its outcomes pin what a
refused NAL leaves behind in the parser."""
import hashlib
import os
import random

from p264decoder_amd import Parser, _native as N
from p264decoder_amd.recon import P264Error
from tests import slice_streams, synth_cases
from tests import stream_args as A

GOLDEN = os.path.join(synth_cases.GOLDEN, "parse_corpus.json")
DAMAGE_BELOW = 40000            # bytes: longer streams are parsed as they are only
COPIES = 8


def arguments():
    """[(name, synth264 arguments)]"""
    out = [("synth:" + k, v[0]) for k, v in synth_cases.CASES.items() if k not in synth_cases.BIG]
    out += [("ipcm:" + k, v) for k, v in A.IPCM_STREAMS.items()]
    out += [("wp:" + k, v) for k, v in A.WP_STREAMS.items()]
    out += [("cip:" + k, v + A.CI) for k, v in A.CI_STREAMS.items()]
    out += [("slices:" + k, v) for k, v in slice_streams.STREAMS.items()]
    out += [("agreeing:" + k, v) for k, v in slice_streams.AGREEING.items()]
    for i, v in enumerate(A.CABAC_STREAMS):
        out += [("cabac:%d:cavlc" % i, v), ("cabac:%d:cabac" % i, v + " --cabac")]
    out += [("b:%d" % i, v) for i, v in enumerate(A.B_STREAMS)]
    for tag, group in (("mmco", A.MMCO), ("sliced", A.SLICED), ("sub8x8", A.SUB8X8), ("reorder", [A.REORDER])):
        out += [("multiref:%s:%d" % (tag, i), v) for i, v in enumerate(group)]
    out += [("long_lists:" + k, v) for k, v in A.LONG_LISTS.items()]       # (behind everything recorded before them: the damage drawn for those stays)
    return out


_streams = []


def streams():
    """[(name, Annex-B bytes)]: the synthetic streams, then tests/golden/f26.264"""
    if not _streams:
        _streams.extend((name, open(synth_cases.generate(args), "rb").read()) for name, args in arguments())
        _streams.append(("f26", open(os.path.join(synth_cases.GOLDEN, "f26.264"), "rb").read()))
    return _streams


def damaged():
    """[(name, [COPIES damaged copies])] of every stream below DAMAGE_BELOW bytes: 1 - 5 bytes at offsets >= 30 (behind the parameter
    sets' first bytes) overwritten with random ones"""
    rng = random.Random(5)
    out = []
    for name, data in streams():
        if len(data) >= DAMAGE_BELOW:
            continue
        copies = []
        for _ in range(COPIES):
            b = bytearray(data)
            for _ in range(rng.randint(1, 5)):
                b[rng.randrange(30, len(b))] = rng.randrange(256)
            copies.append(bytes(b))
        out.append((name, copies))
    return out


def outcomes(lib, data):
    """one entry per NAL of the stream, all fed to ONE parser: "-" no picture, the picture's parse digest, "E" refused"""
    parser = Parser(quiet=True, lib=lib)
    out = []
    for typ, idc, rbsp in N.split_annexb(lib, data):
        try:
            pic = parser.feed(typ, idc, rbsp)
        except P264Error:
            out.append("E")
            continue
        out.append("-" if pic is None else slice_streams.parse_digest([pic])[0])
    parser.close()
    return out


def damaged_digest(outs):
    return hashlib.sha256(" ".join(outs).encode()).hexdigest()


def record(lib):
    """what the golden file holds: {"clean": {name: [outcome per NAL]}, "damaged": {name: [SHA-256 of a copy's joined outcomes]}}"""
    return {"clean": {name: outcomes(lib, data) for name, data in streams()},
            "damaged": {name: [damaged_digest(outcomes(lib, c)) for c in copies] for name, copies in damaged()}}
