"""normalizer_spec edits through include/spmx_reference_binding.h: tests/cpp/ref_override_test.cc edits the spec through a
``sentencepiece::SentencePieceProcessor*`` that points at the subclass -- ``mutable_normalizer_spec()`` is not virtual, the
subclass only sees the edit because it looks at the proto at the top of every call -- and compares every line with an
unmodified base-class processor given the same edit.  Built like tests/test_ref_binding.py: ``__graft_entry__.build()``
compiles the driver where the reference tree is and joins it with the reference's objects under oracle/_ref/."""
import glob
import os
import subprocess

import pytest

from tests import fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
BIN = os.path.join(ROOT, "tests", "cpp", "ref_override_test")
OBJ = os.path.join(ROOT, "oracle", "_ref", "ref_override_test.o")    # the driver and the reference's objects, linked with -r


def build(emu):
    """-> path of the binary, or None where neither the reference tree and its compiled objects nor OBJ are there."""
    if os.path.isdir(os.path.join(REF, "src")):
        objs = sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True))
        if not objs:
            return None
        deps = [os.path.join(ROOT, "tests", "cpp", "ref_override_test.cc"), os.path.join(ROOT, "include", "spmx_reference_binding.h"),
                os.path.join(ROOT, "include", "spmx.h")] + objs
        if not os.path.exists(OBJ) or os.path.getmtime(OBJ) < max(os.path.getmtime(p) for p in deps):
            inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle", "_ref"), "-I" + REF, "-I" + REF + "/src",
                   "-I" + REF + "/src/builtin_pb", "-I" + REF + "/third_party", "-I" + REF + "/third_party/protobuf-lite"]
            drv = OBJ + ".driver.o"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-pthread", "-DHAVE_PTHREAD=1", "-D_USE_INTERNAL_STRING_VIEW"] + inc +
                                  ["-c", "-o", drv, deps[0]])
            subprocess.check_call(["g++", "-r", "-nostdlib", "-o", OBJ, drv] + objs)
            os.remove(drv)
    if not os.path.exists(OBJ):
        return None
    out = BIN + ("_emu" if emu else "")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    if emu:
        from tests import emulib
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    if not os.path.exists(so):
        return None
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in (OBJ, so)):
        subprocess.check_call(["g++", "-pthread", "-o", out, OBJ, "-L" + lib, "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib,
                               "-lpthread"])
    return out


# the loaded specs differ: bpe1k_noesc starts from escape_whitespaces off, bpe1k_llama from add_dummy_prefix on without
# remove_extra_whitespaces
MODELS = ["test_model", "bpe1k", "uni1k_bf", "bpe1k_noesc", "bpe1k_llama"]


@pytest.mark.parametrize("model", MODELS)
def test_reference_binding_override_emulated(model, tmp_path):
    b = build(emu=True)
    if b is None:
        pytest.skip("no reference tree / compiled reference objects here")
    text = os.path.join(str(tmp_path), "lines.txt")
    with open(os.path.join(fixtures.GOLDEN, "botchan.txt"), "rb") as f:
        lines = f.read().split(b"\n")[:400]
    with open(text, "wb") as f:
        f.write(b"\n".join(lines) + b"\n")
    out = subprocess.run([b, os.path.join(fixtures.GOLDEN, model + ".model"), text], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK 400 ")


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_reference_binding_override_gpu(model):
    """Every line of botchan under every edit."""
    b = build(emu=False)
    if b is None:
        pytest.skip("no compiled reference objects here (oracle/_ref is made by __graft_entry__.build() where the reference is)")
    out = subprocess.run([b, os.path.join(fixtures.GOLDEN, model + ".model"), os.path.join(fixtures.GOLDEN, "botchan.txt")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK 4288 ")
