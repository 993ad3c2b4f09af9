"""The hosts of CalculateEntropy / SampleEncodeAndScore: the C++ facade against the C ABI (tests/cpp/lattice_score_test.cc,
built the way tests/test_cpp_facade.py builds its programs) and the Python entry points of processor.py."""
import os
import pickle
import subprocess

import numpy as np
import pytest

from sentencepiece_amd.processor import SentencePieceProcessor
from tests import emulib, fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "lattice_score_test")


class EmuProcessor(SentencePieceProcessor):
    """The product's class bound to the emulated library (what unpickling needs on a machine without a GPU)."""

    def __init__(self, *args, **kw):
        kw.setdefault("_lib", emulib.lib())
        super().__init__(*args, **kw)


def _build(emu):
    src = os.path.join(ROOT, "tests", "cpp", "lattice_score_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    out = BIN + ("_emu" if emu else "")
    if emu:
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(ROOT, "include", "spmx_processor.h"),
                                               os.path.join(ROOT, "include", "spmx.h"), so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-L" + lib,
                               "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("kind", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_facade_agrees_with_the_c_abi(kind):
    out = subprocess.run([_build(kind == "emu"), os.path.join(fixtures.GOLDEN, "test_model.model")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK ")


def _fields(buf):
    """(field number, wire type, value) of a protobuf message: varints as int, length-delimited and fixed32 as bytes."""
    i = 0
    while i < len(buf):
        key = shift = 0
        while True:
            key |= (buf[i] & 0x7F) << shift
            shift += 7
            i += 1
            if not buf[i - 1] & 0x80:
                break
        num, wt = key >> 3, key & 7
        if wt == 0:
            v = shift = 0
            while True:
                v |= (buf[i] & 0x7F) << shift
                shift += 7
                i += 1
                if not buf[i - 1] & 0x80:
                    break
            yield num, wt, v
        elif wt == 2:
            n = shift = 0
            while True:
                n |= (buf[i] & 0x7F) << shift
                shift += 7
                i += 1
                if not buf[i - 1] & 0x80:
                    break
            yield num, wt, buf[i:i + n]
            i += n
        else:
            assert wt == 5
            yield num, wt, buf[i:i + 4]
            i += 4


def nbest_of(blob):
    """A serialized NBestSentencePieceText (src/sentencepiece.proto) -> [(ids, pieces, score)]."""
    res = []
    for num, wt, spt in _fields(blob):
        assert (num, wt) == (1, 2)
        ids, pieces, score = [], [], None
        for n2, w2, v in _fields(spt):
            if n2 == 2:
                f = {n3: v3 for n3, _, v3 in _fields(v)}
                ids.append(f[2])
                pieces.append(bytes(f[1]))
            elif n2 == 3:
                score = float(np.frombuffer(v, dtype=np.float32)[0])
        res.append((ids, pieces, score))
    return res


@pytest.mark.parametrize("kind", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_python_entry_points(kind):
    sp = (EmuProcessor if kind == "emu" else SentencePieceProcessor)(model_proto=fixtures.model_blob("test_model"))
    sents = ["hello world", "in the end it was a test", "a"]
    # entropy: a list equals the per-sentence calls
    one = [sp.CalculateEntropy(s, 0.5) for s in sents]
    assert all(isinstance(x, float) for x in one) and sp.calculate_entropy(sents, 0.5, num_threads=4) == one
    assert np.array_equal(sp.CalculateEntropyPacked(np.frombuffer("".join(sents).encode(), dtype=np.uint8),
                                                    np.cumsum([0] + [len(s) for s in sents]), 0.5), np.asarray(one, dtype=np.float32))
    for kw in (dict(), dict(wor=True), dict(wor=True, include_best=True)):
        as_ids = sp.SampleEncodeAndScore(sents, num_samples=3, alpha=0.5, seed=42, out_type=int, **kw)
        as_str = sp.sample_encode_and_score(sents, num_samples=3, alpha=0.5, seed=42, out_type=str, **kw)
        as_ser = sp.SampleEncodeAndScore(sents, num_samples=3, alpha=0.5, seed=42, out_type="serialized_proto", **kw)
        as_imm = sp.SampleEncodeAndScore(sents, num_samples=3, alpha=0.5, seed=42, out_type="immutable_proto", **kw)
        assert len(as_ids) == len(as_str) == len(as_ser) == len(as_imm) == 3
        for s, ids_rows, str_rows, ser, imm in zip(sents, as_ids, as_str, as_ser, as_imm):
            assert len(ids_rows) == (3 if s != "a" or not kw else 1)           # "a" has two paths: one result without replacement
            assert [sc for _, sc in ids_rows] == [sc for _, sc in str_rows]
            assert [[sp.PieceToId(p) for p in row] for row, _ in str_rows] == [row for row, _ in ids_rows]
            dec = nbest_of(ser)
            assert [(i, np.float32(sc)) for i, _, sc in dec] == [(row, np.float32(sc)) for row, sc in ids_rows]
            assert [p for _, p, _ in dec] == [[q.encode() for q in row] for row, _ in str_rows]
            assert imm.SerializeAsString() == ser and [x.score for x in imm.nbests] == [sc for _, sc in ids_rows]
        # sentence 0 of the list is the single call with that seed (the key is (seed, sentence index, draw))
        assert sp.SampleEncodeAndScore(sents[0], num_samples=3, alpha=0.5, seed=42, **kw) == as_ids[0]
        assert sp.SampleEncodeAndScoreAsIds(sents[0], num_samples=3, alpha=0.5, seed=42, **kw) == as_ids[0]
        assert sp.SampleEncodeAndScoreAsPieces(sents[0], num_samples=3, alpha=0.5, seed=42, **kw) == as_str[0]
        # the extra options apply as they do to NBestEncode
        with_eos = sp.SampleEncodeAndScore(sents[0], num_samples=3, alpha=0.5, seed=42, add_bos=True, add_eos=True, **kw)
        assert with_eos == [([sp.bos_id()] + row + [sp.eos_id()], sc) for row, sc in as_ids[0]]
        rev = sp.SampleEncodeAndScore(sents[0], num_samples=3, alpha=0.5, seed=42, reverse=True, **kw)
        assert rev == [(row[::-1], sc) for row, sc in as_ids[0]]
    # without a seed every call draws afresh
    draws = {tuple(map(tuple, (r for r, _ in sp.SampleEncodeAndScore(sents[1], num_samples=4, alpha=0.1)))) for _ in range(6)}
    assert len(draws) > 1
    # SetVocabulary restricts the lattice as it does for NBestEncode
    sp.SetVocabulary(["▁he", "ll", "o", "▁", "h", "e", "l", "w", "r", "d"])
    try:
        allowed = {sp.PieceToId(p) for p in ["▁he", "ll", "o", "▁", "h", "e", "l", "w", "r", "d"]}
        rows_ = sp.SampleEncodeAndScore("hello world", num_samples=8, alpha=0.1, seed=3)
        nb = sp.NBestEncodeAsIds("hello world", 64)
        assert all(tuple(r) in {tuple(x) for x in nb} for r, _ in rows_)
        restricted = sp.CalculateEntropy("hello world", 0.5)
    finally:
        sp.ResetVocabulary()
    assert restricted != one[0] and sp.CalculateEntropy("hello world", 0.5) == one[0]
    assert allowed
    # pickle round-trips a processor that then still answers both calls
    clone = pickle.loads(pickle.dumps(sp))
    assert clone.CalculateEntropy(sents, 0.5) == one
    assert clone.SampleEncodeAndScore(sents, num_samples=3, alpha=0.5, seed=42, wor=True) == \
        sp.SampleEncodeAndScore(sents, num_samples=3, alpha=0.5, seed=42, wor=True)
