"""The C++ facade's ExpectedCounts (include/spmx_processor.h) against the Python call's numbers: the test writes them into a
file, tests/cpp/expected_counts_test.cc reads it, makes the same calls and compares bit for bit.  Built the way
tests/test_cpp_facade.py builds its programs, emulated and on the GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import fixtures
from tests.test_sampling import _Eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "expected_counts_test")
SENTENCES = ["hello world", "in the end it was a test", ""]
FREQ = [3, 1, 5]


def _build(emu):
    src = os.path.join(ROOT, "tests", "cpp", "expected_counts_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    out = BIN + ("_emu" if emu else "")
    if emu:
        from tests import emulib
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(ROOT, "include", "spmx_processor.h"),
                                               os.path.join(ROOT, "include", "spmx.h"), so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-L" + lib,
                               "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("kind", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_facade_expected_counts_equal_the_python_call(kind, tmp_path):
    sp = _Eng(kind).load(fixtures.model_blob("test_model"))
    lines = ["S %d" % len(SENTENCES)] + [s.encode().hex() or "-" for s in SENTENCES]
    for freq in (FREQ, None):
        e, z, v = sp.ExpectedCounts(SENTENCES, freq)
        assert e.sum() > 0 and v[2] == 0 and z[2] == 0
        nz = np.flatnonzero(e)
        lines.append(" ".join(["F", str(len(freq or []))] + [str(f) for f in freq or []]))
        lines.append(" ".join(["Z"] + ["%08x" % b for b in z.view(np.uint32)]))
        lines.append(" ".join(["V"] + [str(int(x)) for x in v]))
        lines.append("E %d" % len(nz))
        lines += ["%d %016x" % (i, b) for i, b in zip(nz.tolist(), e[nz].view(np.uint64).tolist())]
    numbers = tmp_path / "numbers.txt"
    numbers.write_text("\n".join(lines) + "\n")
    out = subprocess.run([_build(kind == "emu"), os.path.join(fixtures.GOLDEN, "test_model.model"), str(numbers)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK ")
