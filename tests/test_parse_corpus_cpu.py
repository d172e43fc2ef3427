"""The host parser on every stream of the suite and on damaged copies of them, NAL by NAL, against what the library of the commit
before the parser's state was regrouped gave (tests/golden/parse_corpus.json, tests/golden/make_parse_corpus.py): the pictures byte
for byte, every refusal, and - by feeding on after one - the state a refusal leaves behind."""
import json

import pytest

from tests import parse_corpus as pc


@pytest.fixture(scope="module")
def want():
    return json.load(open(pc.GOLDEN))


def test_the_corpus_is_the_recorded_one(want):
    assert list(want["clean"]) == [name for name, _ in pc.streams()]
    assert list(want["damaged"]) == [name for name, _ in pc.damaged()]
    assert all(len(v) == pc.COPIES for v in want["damaged"].values())


def test_streams_parse_to_what_they_did(lib, want):
    pictures = 0
    for name, data in pc.streams():
        got = pc.outcomes(lib, data)
        assert got == want["clean"][name], name
        assert "E" not in got, name
        pictures += sum(len(o) == 16 for o in got)
    assert pictures > 900


def test_damaged_streams_parse_to_what_they_did(lib, want):
    """the damage must keep reaching both halves: pictures that still come out, and NALs that are refused"""
    pictures = refused = 0
    for name, copies in pc.damaged():
        for k, data in enumerate(copies):
            got = pc.outcomes(lib, data)
            pictures += sum(len(o) == 16 for o in got)
            refused += got.count("E")
            assert pc.damaged_digest(got) == want["damaged"][name][k], "%s, damaged copy %d: %s" % (name, k, " ".join(got))
    print("damaged streams: %d pictures delivered, %d NALs refused" % (pictures, refused))
    assert pictures >= 2000 and refused >= 2000, (pictures, refused)
