"""The CalculateEntropy / SampleEncodeAndScore overrides of include/spmx_reference_binding.h against the C ABI with a
fixed seed (tests/cpp/ref_lattice_score_test.cc), built the way tests/test_ref_binding.py builds its driver: compiled
against the reference's header where the reference tree is (``__graft_entry__.build()`` does it) and joined with the
reference's objects into one relocatable object under oracle/_ref/, which is all the link needs wherever the test runs."""
import glob
import os
import subprocess

import pytest

from tests import fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
BIN = os.path.join(ROOT, "tests", "cpp", "ref_lattice_score_test")
OBJ = os.path.join(ROOT, "oracle", "_ref", "ref_lattice_score_test.o")


def build(emu):
    """-> path of the binary, or None where neither the reference tree and its compiled objects nor OBJ are there."""
    if os.path.isdir(os.path.join(REF, "src")):
        objs = sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "obj", "**", "*.o"), recursive=True))
        if not objs:
            return None
        deps = [os.path.join(ROOT, "tests", "cpp", "ref_lattice_score_test.cc"), os.path.join(ROOT, "include", "spmx_reference_binding.h"),
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


@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_binding_agrees_with_the_c_abi_emulated(model):
    b = build(emu=True)
    if b is None:
        pytest.skip("no reference tree / compiled reference objects here")
    out = subprocess.run([b, os.path.join(fixtures.GOLDEN, model + ".model")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK ")


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_binding_agrees_with_the_c_abi_gpu(model):
    b = build(emu=False)
    if b is None:
        pytest.skip("no compiled reference objects here (oracle/_ref is made by __graft_entry__.build() where the reference is)")
    out = subprocess.run([b, os.path.join(fixtures.GOLDEN, model + ".model")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK ")
