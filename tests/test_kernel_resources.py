"""The compiler's resource report of the word-per-lane kernels (sentencepiece_amd/libspmx.resources.txt, written by the
kernels.o rule of csrc/Makefile from -Rpass-analysis=kernel-resource-usage): no scratch memory and no spilled vector
register in any of them.  Scratch in these kernels is how a pipeline stage that the compiler could not keep in registers
shows: the probes of a batch are then waited for where they are issued."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "sentencepiece_amd", "libspmx.resources.txt")

# (mangled: <length><name>ILb<0|1>EE -- the H16 template argument)
KERNELS = ["%d%sILb%dEE" % (len(n), n, b) for n in ("EncodeWordWaveKernel", "EncodeWordWaveCollectKernel", "EncodeWordWaveAgainKernel")
           for b in (1, 0)]


def _report():
    """{function name: {field: value}} of the report's remarks."""
    out, cur = {}, None
    with open(REPORT) as f:
        for line in f:
            m = re.search(r"remark:\s+(.*?)\s*$", line)
            if not m:
                continue
            key, _, val = m.group(1).partition(":")
            if key == "Function Name":
                cur = out.setdefault(val.strip(), {})
            elif cur is not None:
                cur[key.strip()] = val.strip()
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_word_per_lane_kernels_use_no_scratch(kernel):
    if not os.path.exists(REPORT):
        pytest.skip("no resource report next to the library (csrc/Makefile writes it with kernels.o)")
    rep = _report()
    names = [n for n in rep if kernel in n]
    assert len(names) == 1, (kernel, names)
    r = rep[names[0]]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
