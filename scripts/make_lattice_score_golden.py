#!/usr/bin/env python3
"""Writes tests/golden/lattice_scores.json: the compiled reference's CalculateEntropy (float bits) and the float64 exact
entropy for the sentences of tests/latticescore.py, and the result counts of its SampleEncodeAndScore without
replacement.

Needs the reference tree (REF, /root/reference by default) and oracle/_ref/libspm_ref.so (`make -C oracle ref`): the
driver tests/cpp/lattice_score_golden.cc is compiled against the reference's header and linked with that library; the
binary goes to oracle/_ref/ and is never committed.  Where ``import sentencepiece`` works the wheel must return the same
bits and counts -- except for a sentence whose lattice holds a USER_DEFINED piece: a later upstream release scores those
otherwise than the 0.2.1 sources this project follows (seen with 0.2.2: "Botchan" under uni1k_uds, theta 0.2, gives 0.26505
there and 0.29696 here), so those cases are compared with the compiled reference alone and counted.  The numpy re-statement (tests/latticescore.py) is compared as well and the bit-equal cases counted.

    python scripts/make_lattice_score_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests import fixtures, latticeref, latticescore as ls, oraclelib  # noqa: E402
from tests import test_sampling_marginals as tm  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(OUT, "lattice_score_golden")


def build_driver():
    inc = ["-I" + os.path.join(OUT), "-I" + REF, "-I" + REF + "/src", "-I" + REF + "/src/builtin_pb", "-I" + REF + "/third_party",
           "-I" + REF + "/third_party/protobuf-lite"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-pthread", "-DHAVE_PTHREAD=1", "-D_USE_INTERNAL_STRING_VIEW"] + inc +
                          ["-o", BIN, os.path.join(ROOT, "tests", "cpp", "lattice_score_golden.cc"), "-L" + OUT, "-lspm_ref",
                           "-Wl,-rpath," + OUT, "-lpthread"])


def run_driver(model, lines, may_crash=False):
    with tempfile.NamedTemporaryFile("w", suffix=".cases", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.run([BIN, os.path.join(fixtures.GOLDEN, model + ".model"), f.name], capture_output=True, text=True)
    finally:
        os.remove(f.name)
    if out.returncode != 0:
        if may_crash and out.returncode < 0:
            return None
        raise SystemExit("driver failed: " + out.stderr)
    return out.stdout.splitlines()


def japanese_sentence(o, corpora, target):
    """A prefix of the Japanese sample, ASCII letters and digits mixed in after every line (so that every length can be
    hit, not one in three), whose device form has exactly ``target`` bytes."""
    lines = tm._lines(corpora, "ja", 0, len(corpora["ja"][1]) - 1)
    extra = [b"abc", b"x7", b"Tokyo2020", b"k", b"spm", b"42"]
    src = b"".join(ln + extra[i % len(extra)] for i, ln in enumerate(lines)).replace(b" ", b"")
    while ls.dev_len(o.normalize(src)) < target + 64:
        src += src
    text = src.decode("utf-8")
    for start in range(0, 60):
        part = text[start:]
        lo, hi = 1, len(part)
        while lo < hi:                                            # the device length grows with the prefix
            mid = (lo + hi) // 2
            if ls.dev_len(o.normalize(part[:mid].encode())) >= target:
                hi = mid
            else:
                lo = mid + 1
        if ls.dev_len(o.normalize(part[:lo].encode())) == target:
            return part[:lo].encode()
    raise SystemExit("no Japanese prefix of %d device bytes" % target)


def hexs(raw):
    return raw.hex() if raw else "-"


def main():
    build_driver()
    try:
        import sentencepiece
    except ImportError:
        sentencepiece = None
    corpora, oracle = fixtures.Corpora(), oraclelib.OracleLib()
    sentences, entropy, counts = [], [], []
    equal = total = wheel_skipped = 0
    worst = 0.0
    for model, kind, lengths in ls.SENTENCES:
        o = oracle.load(fixtures.model_blob(model))
        lm = latticeref.Model(fixtures.model_blob(model))
        wheel = sentencepiece.SentencePieceProcessor(model_proto=fixtures.model_blob(model)) if sentencepiece else None
        sents = []
        for L in lengths:
            if L == 1:                                            # one character
                raw = "東".encode() if kind == "ja" else b"a"
            elif kind == "ja":
                raw = japanese_sentence(o, corpora, L)
            else:
                raw = tm.sentence((model, kind, L), corpora, oracle)[0]
            if L > 1 and (L in tm.EXACT or kind == "ja"):
                assert ls.dev_len(o.normalize(raw)) == L, (model, kind, L, ls.dev_len(o.normalize(raw)))
            sents.append(("%s%d" % (kind, L), raw))
        sents += [(name, text.encode()) for name, text in ls.FIXED]
        lines = ["E %r %s" % (th, hexs(raw)) for _, raw in sents for th in ls.THETAS]
        got = run_driver(model, lines)
        assert len(got) == len(lines)
        k = 0
        for name, raw in sents:
            norm = o.normalize(raw)
            lat = latticeref.Lattice(lm, norm)
            has_uds = any(lm.pieces[int(t)][2] == latticeref.USER_DEFINED for t in lat.id)
            sid = len(sentences)
            sentences.append({"model": model, "name": name, "raw": raw.decode("utf-8"), "dev_len": ls.dev_len(norm)})
            for th in ls.THETAS:
                b = int(got[k].split()[1], 16)
                k += 1
                if wheel is not None and not has_uds:
                    assert ls.bits(wheel.CalculateEntropy(raw.decode("utf-8"), th)) == b, (model, name, th)
                wheel_skipped += wheel is not None and has_uds
                mine = ls.entropy32(lat, th)
                ref = float(ls.from_bits(b))
                total += 1
                equal += ls.bits(mine) == b
                worst = max(worst, abs(float(mine) - ref) / max(abs(ref), 1e-30) if ref != 0.0 else abs(float(mine)))
                entropy.append({"sentence": sid, "theta": th, "ref_bits": b, "exact": ls.exact_entropy(lat, th)})
        print("%s: %d sentences" % (model, len(sents)), flush=True)
    print("numpy re-statement: %d of %d cases bit-equal to the compiled reference, largest relative difference %.3g" % (equal, total, worst))
    if wheel_skipped:
        print("%d cases not compared with the wheel: a USER_DEFINED piece in the lattice" % wheel_skipped)
    model = "test_model"
    lines = ["C %d %d %r %s" % (k, best, 1.0, hexs(s.encode())) for s in ls.COUNT_SENTENCES for k in ls.COUNT_SAMPLES for best in (0, 1)]
    # one process per case: where the lattice has ONE path and include_best is set the reference erases the best path from
    # the samples and then reads and pops the back of an empty vector (unigram_model.cc:788-798) -- undefined behaviour,
    # which ends the process here; recorded as results = null, and the wheel is not asked
    got = [run_driver(model, [ln], may_crash=True) for ln in lines]
    wheel = sentencepiece.SentencePieceProcessor(model_proto=fixtures.model_blob(model)) if sentencepiece else None
    lm = latticeref.Model(fixtures.model_blob(model))
    o = oracle.load(fixtures.model_blob(model))
    k = 0
    for s in ls.COUNT_SENTENCES:
        lat = latticeref.Lattice(lm, o.normalize(s.encode()))
        paths = len(lat.paths()) if lat.n_chars else 0
        for num in ls.COUNT_SAMPLES:
            for best in (0, 1):
                n = int(got[k][0].split()[1]) if got[k] is not None else None
                k += 1
                if wheel is not None and n is not None:
                    try:
                        w = len(wheel.SampleEncodeAndScore(s, num_samples=num, alpha=1.0, wor=True, include_best=bool(best)))
                    except RuntimeError:
                        w = -1
                    assert w == n, (s, num, best, w, n)
                counts.append({"model": model, "raw": s, "paths": paths, "num_samples": num, "include_best": best, "results": n})
    with open(ls.GOLDEN, "w", encoding="utf-8") as f:
        json.dump({"sentences": sentences, "entropy": entropy, "wor_counts": counts}, f, ensure_ascii=False, indent=0)
    print("wrote %s: %d sentences, %d entropy cases, %d count cases" % (ls.GOLDEN, len(sentences), len(entropy), len(counts)))


if __name__ == "__main__":
    main()
