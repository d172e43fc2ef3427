"""The C-ABI library loads without a GPU and exports every symbol include/*.h declares;
struct layouts seen by ctypes equal what a C compiler sees.  No compute calls here."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import pytest

from p264decoder_amd import _native as N
from p264decoder_amd import decoder as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def declared_functions():
    names = set()
    for h in os.listdir(INC):
        if not h.endswith(".h"):
            continue
        text = open(os.path.join(INC, h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(p264\w*)\s*\(", text):
            pre = text[:m.start()].rstrip()
            if pre.endswith(("*", "int", "void", "char", "int64_t", "p264parse", "p264_t")) or pre.endswith("const"):
                names.add(m.group(1))
    return names


def test_library_exports_every_declared_symbol(lib):
    names = declared_functions()
    assert {"p264_decoder_open", "p264_decoder_decode", "p264_decoder_close", "p264_nal_decode", "p264_param_default",
            "p264hip_create", "p264hip_reconstruct", "p264hip_submit", "p264parse_nal", "p264_annexb_next"} <= names
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, "declared in include/*.h but not exported: %s" % missing


def test_library_is_not_a_timing_build(lib):
    """Bit 0 of p264hip_build_info() marked a library with pieces of its kernels compiled out (wrong pictures).  No such build
    exists any more; the bit is reserved and stays clear in the library under test and the one that travels to the GPU box."""
    assert lib.p264hip_build_info() & N.BUILD_TIMING == 0


def test_struct_layouts_match_the_headers(lib):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "p264hip.h"
#include "p264_dropin.h"
int main(void) {
  printf("mb %zu\n", sizeof(p264hip_mb_t));
  printf("pic %zu %zu %zu %zu\n", sizeof(p264hip_picture_t), offsetof(p264hip_picture_t, ref_slot), offsetof(p264hip_picture_t, mb), offsetof(p264hip_picture_t, coefs));
  printf("param %zu %zu %zu %zu\n", sizeof(p264_param_t), offsetof(p264_param_t, analyse), offsetof(p264_param_t, rc), offsetof(p264_param_t, b_repeat_headers));
  printf("picture %zu %zu\n", sizeof(p264_picture_t), offsetof(p264_picture_t, img));
  printf("nal %zu %zu\n", sizeof(p264_nal_t), offsetof(p264_nal_t, p_payload));
  printf("launch %zu %zu\n", sizeof(p264hip_launch_info_t), offsetof(p264hip_launch_info_t, deblock_wgs));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I" + INC, c, "-o", exe], check=True)
        out = dict((l.split()[0], [int(x) for x in l.split()[1:]]) for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert out["mb"] == [C.sizeof(N.MbInfo)] == [16]
    assert out["pic"] == [C.sizeof(N.Picture), N.Picture.ref_slot.offset, N.Picture.mb.offset, N.Picture.coefs.offset]
    assert out["param"] == [C.sizeof(D.Param), D.Param.analyse.offset, D.Param.rc.offset, D.Param.b_repeat_headers.offset]
    assert out["picture"] == [C.sizeof(D.PictureOut), D.PictureOut.img.offset]
    assert out["nal"] == [C.sizeof(D.Nal), D.Nal.p_payload.offset]
    assert out["launch"] == [C.sizeof(N.LaunchInfo), N.LaunchInfo.deblock_wgs.offset]


GOLDEN = os.path.join(ROOT, "tests", "golden")
DROPIN_LAYOUT = r'''
int main(void) {
  printf("%zu %zu %zu %zu %zu ", sizeof(p264_param_t), offsetof(p264_param_t, vui), offsetof(p264_param_t, cqm_4iy), offsetof(p264_param_t, analyse), offsetof(p264_param_t, rc));
  printf("%zu %zu %zu ", offsetof(p264_param_t, pf_log), offsetof(p264_param_t, b_aud), offsetof(p264_param_t, b_repeat_headers));
  printf("%zu %zu %zu %zu ", sizeof(p264_picture_t), offsetof(p264_picture_t, i_width), offsetof(p264_picture_t, img), sizeof(p264_image_t));
  printf("%zu %zu %zu\n", sizeof(p264_nal_t), offsetof(p264_nal_t, i_payload), offsetof(p264_nal_t, p_payload));
  return 0; }
'''


def dropin_layout(inc, hdr):
    """Sizes and offsets of the drop-in structs as a C compiler sees them through header `hdr` of directory `inc`."""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write("#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\n#include \"%s\"\n%s" % (hdr, DROPIN_LAYOUT))
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-w", "-I" + inc, c, "-o", exe], check=True)
        return subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_dropin_structs_match_the_reference_header():
    """Binary contract of the drop-in: same sizes/offsets as the reference's own p264.h (what a compiler sees through it,
    recorded by tests/golden/make_ref_abi.py in tests/golden/ref_dropin_layout.txt)."""
    want = open(os.path.join(GOLDEN, "ref_dropin_layout.txt")).read()
    assert dropin_layout(INC, "p264_dropin.h") == want


def test_open_fails_loudly_without_a_gpu(lib):
    """No silent CPU fallback: on a box without a HIP device the product refuses to open."""
    if lib.p264hip_device_count() > 0:
        pytest.skip("a GPU is present")
    p = D.param_default(lib)
    D._bind(lib)
    assert not lib.p264_decoder_open(C.byref(p))
    h = C.c_void_p()
    assert lib.p264hip_create(C.byref(h), 0, 22, 18, 1, 2, 1) == -2      # P264HIP_ENODEV
    assert b"no HIP device" in lib.p264hip_last_error()


def test_cli_builds_and_prints_usage():
    """tools/p264decoder_amd (the `p264decoder -d` equivalent) is built with the library; without arguments it
    prints the reference's usage line and fails, before touching any device (p264decoder.c:83-89,115-122)."""
    import subprocess
    from p264decoder_amd import build as _build
    _build.build_tools()
    cli = os.path.join(os.path.dirname(_build.__file__), "tools", "p264decoder_amd")
    assert os.path.exists(cli)
    r = subprocess.run([cli], stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "-d <test.264> [recon.yuv] [origin.yuv]" in r.stderr


def _param_values(p):
    """Every field of a p264_param_t as comparable Python values (strings by content; `cpu` and `pf_log` left out: the
    reference detects x86 features and installs its own logger function)."""
    out = {}

    def walk(prefix, obj):
        for name, typ in obj._fields_:
            v = getattr(obj, name)
            key = prefix + name
            if key in ("cpu", "pf_log"):
                continue
            if hasattr(v, "_fields_"):
                walk(key + ".", v)
            elif isinstance(v, C.Array):
                out[key] = [list(x) if isinstance(x, C.Array) else x for x in v]
            elif typ is C.c_char_p:
                out[key] = v
            elif typ is C.c_void_p or (isinstance(typ, type) and issubclass(typ, C._Pointer)):
                out[key] = bool(v)
            else:
                out[key] = v
    walk("", p)
    return out


def param_values_json(p):
    """_param_values in the form tests/golden/ref_param_default.json keeps them (strings by content as latin-1 text)."""
    return json.loads(json.dumps({k: {"bytes": v.decode("latin-1")} if isinstance(v, bytes) else v for k, v in _param_values(p).items()}))


def test_param_default_values_match_the_reference(lib):
    """p264_param_default fills every field with the reference's value (core/core.c:41-137): compared against what the REAL
    function filled in, recorded by tests/golden/make_ref_abi.py from oracle/_ref/libp264ref_kat.so (the reference's own
    objects) in tests/golden/ref_param_default.json."""
    a = D.Param()
    C.memset(C.byref(a), 0xAA, C.sizeof(a))
    D._bind(lib)
    lib.p264_param_default(C.byref(a))
    va, vb = param_values_json(a), json.load(open(os.path.join(GOLDEN, "ref_param_default.json")))
    assert va.keys() == vb.keys() and len(va) > 60
    diff = {k: (va[k], vb[k]) for k in va if va[k] != vb[k]}
    assert not diff, diff
    assert bool(a.pf_log) and a.cpu == 0


def test_picture_alloc_and_clean(lib):
    """p264_picture_alloc / p264_picture_clean (p264.h:300-305, core/core.c:181-272): plane pointers and strides."""
    D._bind(lib)
    pic = D.PictureOut()
    lib.p264_picture_alloc.argtypes = [C.POINTER(D.PictureOut), C.c_int, C.c_int, C.c_int]
    lib.p264_picture_clean.argtypes = [C.POINTER(D.PictureOut)]
    lib.p264_picture_alloc(C.byref(pic), 0x0001, 64, 32)
    assert pic.i_width == 64 and pic.i_height == 32 and pic.img.i_plane == 3 and list(pic.img.i_stride)[:3] == [64, 32, 32]
    base = C.cast(pic.img.plane[0], C.c_void_p).value
    assert C.cast(pic.img.plane[1], C.c_void_p).value == base + 64 * 32 and C.cast(pic.img.plane[2], C.c_void_p).value == base + 64 * 32 * 5 // 4
    lib.p264_picture_clean(C.byref(pic))
    assert pic.img.i_plane == 0 and not pic.img.plane[0]


REF = "/root/reference"


CLI_NEEDS = {"p264_param_default", "p264_decoder_open", "p264_decoder_decode", "p264_decoder_close", "p264_nal_decode", "p264_mdate"}


def compile_reference_cli(ref, tmp):
    """The reference's own caller (p264decoder.c), compiled from where it lies and linked against libp264amd.so; the empty
    config.h its line 44 includes is written to `tmp` (upstream's configure writes it, SURVEY App. C uses an empty one)."""
    open(os.path.join(tmp, "config.h"), "w").write("")
    exe = os.path.join(tmp, "p264decoder_ref_cli")
    cc = subprocess.run(["gcc", "-O1", "-std=gnu99", "-w", "-D__P264__", "-DHAVE_STDINT_H", "-I" + tmp, "-I" + ref, os.path.join(ref, "p264decoder.c"),
                         "-L" + os.path.dirname(N.LIB_PATH), "-lp264amd", "-Wl,-rpath," + os.path.dirname(N.LIB_PATH), "-Wl,--no-undefined", "-lm", "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return exe, cc


def undefined_p264_symbols(exe):
    undefined = {l.split()[-1] for l in subprocess.run(["nm", "-u", exe], stdout=subprocess.PIPE, text=True).stdout.splitlines() if " p264_" in l or l.strip().startswith("U p264_")}
    return {u.split("@")[0] for u in undefined}


def test_the_reference_cli_links_unchanged_against_the_library(lib, tmp_path):
    """the reference's own caller (p264decoder.c:69-381: main, Decode, write_frame) compiled from
    where it lies, UNCHANGED, with the reference's headers, and linked against libp264amd.so instead of the reference's core/ and
    decoder/ objects - every symbol it needs (p264_param_default, p264_decoder_open / _decode / _close, p264_nal_decode,
    p264_mdate) must resolve to the library.  The symbols it leaves undefined are recorded in tests/golden/ref_cli_symbols.txt
    (tests/golden/make_ref_abi.py) and checked against the library everywhere.  Where the reference's source is at hand the
    caller itself is compiled as well - with the empty `config.h` its line 44 includes (upstream's configure writes it, this tree
    has no configure, SURVEY App. C uses an empty one; in tmp, nothing enters the repo) - and must leave exactly those symbols
    undefined.  Run there without a GPU the binary must get as far as the reference would with a decoder that cannot open:
    Help() on no arguments, and "p264_decoder_open failed" on `-d` (p264decoder.c:203-207) - through OUR p264_decoder_open."""
    recorded = set(open(os.path.join(GOLDEN, "ref_cli_symbols.txt")).read().split())
    assert CLI_NEEDS <= recorded
    assert all(hasattr(lib, u) for u in recorded), sorted(u for u in recorded if not hasattr(lib, u))
    if not os.path.exists(os.path.join(REF, "p264decoder.c")):
        return                                                        # the reference's source does not travel: the recorded list is the check
    exe, cc = compile_reference_cli(REF, str(tmp_path))
    assert cc.returncode == 0, cc.stdout[-3000:]
    # every p264_* symbol the caller leaves undefined is one the library defines
    undefined = undefined_p264_symbols(exe)
    assert CLI_NEEDS <= undefined and undefined == recorded
    assert all(hasattr(lib, u) for u in undefined), undefined
    ldd = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "libp264amd.so" in ldd and "not found" not in ldd
    import torch
    if not torch.cuda.is_available():
        stream = os.path.join(ROOT, "tests", "golden", "f26.264")
        run = subprocess.run([exe, "-d", stream, str(tmp_path / "out.yuv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                             env=dict(os.environ, P264AMD_QUIET="1"))
        assert "p264_decoder_open failed" in run.stderr             # no HIP device: the drop-in refuses to open (no CPU fallback)
