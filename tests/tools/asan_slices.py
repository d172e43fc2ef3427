"""Driver for tests/tools/asan_slices.sh: the streams whose slices differ in reference lists and loop-filter offsets
(tests/slice_streams.py) through the host parser built with AddressSanitizer + UBSan - whole, against the writer's record, and
damaged; the packers on the parsed pictures; the parse-only pipeline.  Host code only: the HIP layer is a stub."""
import os
import pathlib
import random
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from p264decoder_amd import HipReconstructor, Parser, Pipeline, _native as N     # noqa: E402

lib = N.load(sys.argv[1])
from tests import slice_streams as ss                                            # noqa: E402

random.seed(5)
MANY = "--mbw 6 --mbh 5 --frames 9 --seed 123 --refs 4 --bframes 1 --slices 3 --wp --coded 10 --maxlevel 6 --slice-lists-many"
WP = "--mbw 8 --mbh 6 --frames 13 --seed 122 --refs 3 --bframes 2 --slices 3 --wp --wp-bi --cabac --coded 10 --maxlevel 6 --slice-lists --slice-deblock"
streams = []
with tempfile.TemporaryDirectory() as t:
    for name, args in list(ss.STREAMS.items()) + [("wp", WP), ("many", MANY)]:
        data, dump = ss.make(pathlib.Path(t), args)
        streams.append(data)
        try:
            pics = Parser(quiet=True, lib=lib).parse_stream(data)
        except Exception as e:
            assert name == "many", (name, e)                    # more than sixteen entries: refused, cleanly
            print(name, "refused")
            continue
        ss.check_against_dump(pics, dump)
        for p in pics:
            HipReconstructor.expand_compact(p, HipReconstructor.pack_compact(p, lib), lib)
            HipReconstructor.pack(p, lib)
        print(name, len(pics))
for data in streams:
    for trial in range(40):
        d = bytearray(data)
        for _ in range(random.randrange(1, 20)):
            d[random.randrange(30, len(d))] = random.randrange(256)
        d = bytes(d[:random.randrange(100, len(d))])
        try:
            Parser(quiet=True, lib=lib).parse_stream(d)
        except Exception:
            pass
print("damaged streams ok")
same_size = [s for s, a in zip(streams, ss.STREAMS.values()) if "--mbw 8 --mbh 6" in a]
pipe = Pipeline(same_size * 2, threads=3, device=-1, lib=lib)
print("pipeline", pipe.run()["pictures"])
pipe.close()
