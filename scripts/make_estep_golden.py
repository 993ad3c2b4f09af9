#!/usr/bin/env python3
"""Writes tests/golden/expected_counts.npz: the compiled reference's E-step -- Lattice::PopulateMarginal's float marginals per
piece, log Z and the node count of Lattice::Viterbi() -- for the sentences recorded in tests/golden/lattice_scores.json
(referred to by index), each at freq 1 and the 64- and 300-byte ones at freq 3 and 2^20 too (tests/estep.py ``cases``).

Needs the reference tree (REF, /root/reference by default) and oracle/_ref/libspm_ref.so (`make -C oracle ref`): the driver
tests/cpp/estep_golden.cc is compiled against the reference's headers and linked with that library; the binary goes to
oracle/_ref/ and is never committed.  The numpy re-statement (tests/estep.py) is compared as it goes: log Z and the node
counts must agree exactly, the counts within the bound of tests/test_expected_counts.py.

The file is sparse and compressed: per case the non-zero (id, float bits) of ``expected``.  It must stay below the largest
file under tests/golden/; the 6000-byte cases are the first to go where it does not.

    python scripts/make_estep_golden.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests import estep, fixtures, latticeref, latticescore as ls, oraclelib  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(OUT, "estep_golden")


def build_driver():
    inc = ["-I" + os.path.join(OUT), "-I" + REF, "-I" + REF + "/src", "-I" + REF + "/src/builtin_pb", "-I" + REF + "/third_party",
           "-I" + REF + "/third_party/protobuf-lite"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-pthread", "-DHAVE_PTHREAD=1", "-D_USE_INTERNAL_STRING_VIEW"] + inc +
                          ["-o", BIN, os.path.join(ROOT, "tests", "cpp", "estep_golden.cc"), "-L" + OUT, "-lspm_ref",
                           "-Wl,-rpath," + OUT, "-lpthread"])


def run_driver(model, lines):
    with tempfile.NamedTemporaryFile("w", suffix=".cases", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.run([BIN, os.path.join(fixtures.GOLDEN, model + ".model"), f.name], capture_output=True, text=True)
    finally:
        os.remove(f.name)
    if out.returncode != 0:
        raise SystemExit("driver failed: " + out.stderr)
    return out.stdout.splitlines()


def main():
    build_driver()
    oracle = oraclelib.OracleLib()
    sents = ls.golden()["sentences"]
    cases = estep.cases()
    limit = max(os.path.getsize(os.path.join(fixtures.GOLDEN, f)) for f in os.listdir(fixtures.GOLDEN)
                if os.path.join(fixtures.GOLDEN, f) != estep.GOLDEN)
    rec = {}
    for model in sorted({s["model"] for s in sents}):
        mine = [(i, f) for i, f in cases if sents[i]["model"] == model]
        got = run_driver(model, ["M %d %s" % (f, sents[i]["raw"].encode().hex() or "-") for i, f in mine])
        assert len(got) == len(mine)
        o = oracle.load(fixtures.model_blob(model))
        lm = latticeref.Model(fixtures.model_blob(model))
        z_equal = 0
        for (i, f), line in zip(mine, got):
            w = line.split()
            k = int(w[3])
            pairs = [x.split(":") for x in w[4:4 + k]]
            ids = np.array([int(a) for a, _ in pairs], dtype=np.int32)
            vals = np.array([int(b, 16) for _, b in pairs], dtype=np.uint32)
            rec[(i, f)] = (int(w[1], 16), int(w[2]), ids, vals)
            if f == 1:                                            # the re-statement, as it goes
                lat = latticeref.Lattice(lm, o.normalize(sents[i]["raw"].encode()))
                _, _, Z = estep.marginal_q(lat, 1)
                z_equal += ls.bits(Z) == int(w[1], 16)
                assert estep.viterbi_nodes32(lat) == int(w[2]), (model, sents[i]["name"])
        print("%s: %d cases, log Z of the re-statement bit-equal in %d of %d" % (model, len(mine), z_equal, sum(f == 1 for _, f in mine)),
              flush=True)
    keep = list(cases)
    while True:
        offs = np.zeros(len(keep) + 1, dtype=np.int64)
        np.cumsum([len(rec[c][2]) for c in keep], out=offs[1:])
        np.savez_compressed(estep.GOLDEN,
                            sentence=np.array([i for i, _ in keep], dtype=np.int32), freq=np.array([f for _, f in keep], dtype=np.uint32),
                            z_bits=np.array([rec[c][0] for c in keep], dtype=np.uint32),
                            viterbi_nodes=np.array([rec[c][1] for c in keep], dtype=np.uint32), offsets=offs,
                            ids=np.concatenate([rec[c][2] for c in keep]), value_bits=np.concatenate([rec[c][3] for c in keep]))
        size = os.path.getsize(estep.GOLDEN)
        if size <= limit:
            break
        longest = max(sents[i]["dev_len"] for i, _ in keep)
        print("%d bytes is more than the largest golden file (%d): dropping the cases of %d device bytes" % (size, limit, longest))
        keep = [(i, f) for i, f in keep if sents[i]["dev_len"] < longest]
    print("wrote %s: %d cases, %d bytes" % (estep.GOLDEN, len(keep), size))


if __name__ == "__main__":
    main()
