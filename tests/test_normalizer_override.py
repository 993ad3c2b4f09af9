"""Live normalizer_spec overrides (spmx_override_normalizer_spec, OverrideNormalizerSpec, mutable_normalizer_spec) and
pickling of the processor.

The invariant under test: after any sequence of overrides a handle behaves like one newly created from its own
serialized_model_proto() -- the loaded ModelProto with only the overridden normalizer_spec fields changed.  Every
expected value comes from the C oracle (and, where it is built, the compiled reference) loaded from the ModelProto edited
the same way through ``sentencepiece_model_pb2``; never from another handle of the product.  Each test runs on the CPU
with the device emulated (tests/emulib.py) and, with ``-m gpu``, on the product library."""
import copy
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys
import threading

import numpy as np
import pytest

from sentencepiece_amd.processor import SentencePieceProcessor
from tests import emulib, fixtures, refshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("add_dummy_prefix", "remove_extra_whitespaces", "escape_whitespaces")


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.param, emulib.backend(request.param)


def pb():
    from sentencepiece import sentencepiece_model_pb2
    return sentencepiece_model_pb2


def edited(blob, **fields):
    """The ModelProto `blob` with normalizer_spec fields set through the protobuf classes."""
    m = pb().ModelProto()
    m.ParseFromString(blob)
    for k, v in fields.items():
        setattr(m.normalizer_spec, k, v)
    return m.SerializeToString()


def loaded_flags(blob):
    m = pb().ModelProto()
    m.ParseFromString(blob)
    return tuple(bool(getattr(m.normalizer_spec, f)) for f in FLAGS)


@functools.lru_cache(maxsize=None)
def inputs(model):
    """One packed batch that reaches every launch shape at the smallest size that does: the whole edge corpus, 300 lines
    of botchan, one document of about 20 KB and -- for the 32k vocabularies, so that the word rounds have words to take
    -- 2,000 synthetic sentences."""
    corp = fixtures.Corpora()
    parts = [corp["edge"], fixtures.head(*corp["botchan"], 300)]
    bt, bo = corp["botchan"]
    k = int(np.searchsorted(bo, 20000))
    doc = np.asarray(bt[:int(bo[k])])
    parts.append((doc, np.array([0, len(doc)], dtype=np.uint64)))
    if model in ("uni32k", "bpe32k"):
        parts.append(fixtures.head(*corp["synth20k"], 2000))
    text = np.concatenate([np.asarray(t, dtype=np.uint8) for t, _ in parts])
    offs, base = [np.zeros(1, dtype=np.uint64)], 0
    for t, o in parts:
        offs.append(np.asarray(o[1:], dtype=np.uint64) + np.uint64(base))
        base += len(t)
    return text, np.concatenate(offs)


_ORACLE = []


def oracle_lib():
    if not _ORACLE:
        from tests import oraclelib
        _ORACLE.append(oraclelib.OracleLib())
    return _ORACLE[0]


@functools.lru_cache(maxsize=None)
def expected(model, flags):
    """(ids, id_offsets, decoded text, text offsets, spans, normalized) of inputs(model) from the oracle on the edited blob;
    where the compiled reference is built its ids and decoded text must say the same."""
    blob = edited(fixtures.model_blob(model), **dict(zip(FLAGS, flags)))
    o = oracle_lib().load(blob)
    text, offs = inputs(model)
    ids, io = o.encode_batch(text, offs)
    dt, do = o.decode_batch(ids, io)
    if refshim.available():
        r = refshim.RefLib().load(blob)
        rids, rio = r.encode_batch(text, offs)
        np.testing.assert_array_equal(rio, io)
        np.testing.assert_array_equal(rids, ids)
        rt, ro = r.decode_batch(ids, io)
        np.testing.assert_array_equal(ro, do)
        np.testing.assert_array_equal(rt, dt)
    return ids, io, dt, do, o.encode_spans(text, offs), o.normalize_batch(text, offs)


def same(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64), err_msg=str(what))


def check_step(h, model, flags):
    text, offs = inputs(model)
    ids, io, dt, do, spans, norm = expected(model, flags)
    assert tuple(h.sp.NormalizerSpec()[f] for f in FLAGS) == flags
    got = h.sp.EncodePacked(text, offs)
    same(got, (ids, io), (model, flags, "ids"))
    same(h.sp.DecodePacked(*got), (dt, do), (model, flags, "decode"))
    same(h.sp.EncodeSpansPacked(text, offs), spans, (model, flags, "spans"))
    same(h.sp.NormalizePacked(text, offs, with_offsets=True), norm, (model, flags, "normalize"))


def gray_walk(start):
    """The other seven flag combinations and then `start` again, each one switch away from the one before."""
    bits = sum(1 << i for i, f in enumerate(start) if f)
    for i in range(1, 9):
        g = (i % 8) ^ ((i % 8) >> 1)
        yield tuple(bool((bits ^ g) >> k & 1) for k in range(3))


WALK_MODELS = ["test_model", "bpe1k", "uni1k_uds", "uni1k_suffix", "uni1k_bf", "bpe1k_llama", "bpe1k_noesc", "uni32k", "bpe32k"]


@pytest.mark.parametrize("model", WALK_MODELS)
def test_walk_all_flag_combinations(model, backend, golden_arrays):
    """One handle through all eight combinations in Gray-code order, ending on the loaded spec: every step equals the
    oracle on the equally edited blob, the last one also the stored ids of the model."""
    blob = fixtures.model_blob(model)
    h = backend[1].load(blob)
    start = loaded_flags(blob)
    prev, seen = start, set()
    for flags in gray_walk(start):
        (changed,) = [i for i in range(3) if flags[i] != prev[i]]
        h.sp.OverrideNormalizerSpec(**{FLAGS[changed]: flags[changed]})
        check_step(h, model, flags)
        seen.add(flags)
        prev = flags
    assert len(seen) == 8 and prev == start
    text, offs = inputs(model)
    ids, io = h.sp.EncodePacked(text, offs)
    n_edge = len(fixtures.Corpora()["edge"][1]) - 1
    np.testing.assert_array_equal(ids[:int(io[n_edge])], golden_arrays[model + "__edge__ids"])
    cnt = golden_arrays[model + "__botchan__cnt"][:300].astype(np.int64)
    np.testing.assert_array_equal(np.diff(io[n_edge:n_edge + 301].astype(np.int64)), cnt)
    np.testing.assert_array_equal(ids[int(io[n_edge]):int(io[n_edge + 300])], golden_arrays[model + "__botchan__ids"][:int(cnt.sum())])
    m = pb().ModelProto()
    m.ParseFromString(h.sp.serialized_model_proto())
    assert tuple(getattr(m.normalizer_spec, f) for f in FLAGS) == start


@pytest.mark.gpu
def test_single_override_of_the_250k_vocabulary(oracle, corpora):
    """c5_250k (the largest tables: the rebuild's upload replaces hundreds of megabytes) with one switch changed."""
    blob = fixtures.model_blob("c5_250k")
    sp = SentencePieceProcessor(model_proto=blob)
    before = sp.HandleInfo()["table_bytes"]
    sp.OverrideNormalizerSpec(add_dummy_prefix=False)
    o = oracle.load(edited(blob, add_dummy_prefix=False))
    for name, k in (("edge", 10 ** 6), ("botchan", 300), ("synth20k", 2000)):
        text, offs = fixtures.head(*corpora[name], k)
        same(sp.EncodePacked(text, offs), o.encode_batch(text, offs), name)
    # spmx_handle_info reports the NEW tables: what a handle newly created from the edited proto reports (that handle is
    # asked for nothing else)
    fresh = SentencePieceProcessor(model_proto=sp.serialized_model_proto())
    assert sp.HandleInfo()["table_bytes"] == fresh.HandleInfo()["table_bytes"] > 0
    assert before > 0


def test_reference_known_answers(backend):
    """python/test/sentencepiece_test.py:912-927 (test_override_normalize_spec) and :896-903 on the bundled model."""
    h = backend[1].load(fixtures.model_blob("test_model"))
    sp = h.sp
    assert sp.Encode(" hello  world ", out_type=str) == ["▁he", "ll", "o", "▁world"]
    sp.override_normalizer_spec(add_dummy_prefix=False)
    sp.override_normalizer_spec(remove_extra_whitespaces=False)
    sp.override_normalizer_spec(escape_whitespaces=False)
    assert sp.Encode(" hello  world ", out_type=str) == [" ", "he", "ll", "o", "  ", "w", "or", "l", "d", " "]
    h = backend[1].load(fixtures.model_blob("test_model"))
    assert h.sp.Normalize("  hello  world  ") == "▁hello▁world"
    h.sp.override_normalizer_spec(add_dummy_prefix=False, escape_whitespaces=False)      # the spec of :897-902
    assert h.sp.Normalize("  hello  world  ") == "hello world"


@pytest.mark.parametrize("model", ["test_model", "bpe1k"])
def test_state_survives_an_override(model, backend, oracle, corpora):
    """Encode extra options, a vocabulary restriction and decode extra options set BEFORE an override hold after it; a
    restriction set and lifted AFTER one works on the rebuilt tables."""
    blob = fixtures.model_blob(model)
    text, offs = fixtures.head(*corpora["botchan"], 300)
    m = pb().ModelProto()
    m.ParseFromString(blob)
    subset = [p.piece for i, p in enumerate(m.pieces) if i % 3 == 0]

    def reversed_rows(ids, io):          # Decode under `reverse` = Decode of the reversed pieces (sentencepiece_processor.cc:819)
        return np.concatenate([ids[int(io[i]):int(io[i + 1])][::-1] for i in range(len(io) - 1)] + [np.zeros(0, np.int32)])

    h = backend[1].load(blob)
    h.sp.SetEncodeExtraOptions("bos:eos")
    h.sp.SetVocabulary(subset)
    h.sp.SetDecodeExtraOptions("reverse")
    h.sp.SetProfiling(True)
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=False, remove_extra_whitespaces=False)
    eblob = edited(blob, add_dummy_prefix=False, remove_extra_whitespaces=False)
    o = oracle.load(eblob)
    o.set_encode_extra_options("bos:eos")
    o.set_vocabulary(subset)
    want = o.encode_batch(text, offs)
    got = h.sp.EncodePacked(text, offs)
    same(got, want, "first order: ids")
    assert sum(c["sentences"] for c in h.sp.LastProfile()["classes"]) == len(offs) - 1           # the profiling switch held
    same(h.sp.DecodePacked(*got), o.decode_batch(reversed_rows(*want), want[1]), "first order: decode")
    if refshim.available():
        r = refshim.RefLib().load(eblob)
        r.set_decode_extra_options("reverse")
        same(h.sp.DecodePacked(*got), r.decode_batch(*want), "first order: decode, compiled reference")
    assert not np.array_equal(want[0], oracle.load(eblob).encode_batch(text, offs)[0])           # the restriction matters here

    h = backend[1].load(blob)
    h.sp.OverrideNormalizerSpec(escape_whitespaces=False)
    o = oracle.load(edited(blob, escape_whitespaces=False))
    h.sp.SetVocabulary(subset)
    o.set_vocabulary(subset)
    same(h.sp.EncodePacked(text, offs), o.encode_batch(text, offs), "second order: restricted")
    h.sp.ResetVocabulary()
    o.reset_vocabulary()
    same(h.sp.EncodePacked(text, offs), o.encode_batch(text, offs), "second order: reset")


def _spec_variants():
    """name -> ModelProto bytes of test_model whose normalizer_spec lacks the three switches / is missing / carries an
    unknown field (number 77, a varint, behind the known ones)."""
    m = pb().ModelProto()
    m.ParseFromString(fixtures.model_blob("test_model"))
    out = {"full": m.SerializeToString()}
    for f in FLAGS:
        m.normalizer_spec.ClearField(f)
    out["no_switches"] = m.SerializeToString()
    spec = m.normalizer_spec.SerializeToString() + bytes([(77 << 3) & 0x7F | 0x80, (77 << 3) >> 7, 5])
    m2 = pb().ModelProto()
    m2.ParseFromString(out["full"])
    m2.ClearField("normalizer_spec")
    out["no_spec"] = m2.SerializeToString()
    body = m2.SerializeToString()
    n = len(spec)
    assert n >= 128
    varint = bytes([n & 0x7F | 0x80, n >> 7]) if n < 16384 else bytes([n & 0x7F | 0x80, (n >> 7) & 0x7F | 0x80, n >> 14])
    out["unknown_field"] = body + bytes([3 << 3 | 2]) + varint + spec
    return out


@pytest.mark.parametrize("variant", ["full", "no_switches", "no_spec", "unknown_field"])
def test_serialized_proto_is_the_edited_proto(variant, backend, oracle, corpora):
    blob = _spec_variants()[variant]
    text, offs = fixtures.head(*corpora["botchan"], 300)
    h = backend[1].load(blob)
    assert h.sp.serialized_model_proto() == blob
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=False, escape_whitespaces=True)       # (the second at its default: written all the same)
    want = pb().ModelProto()
    want.ParseFromString(blob)
    want.normalizer_spec.add_dummy_prefix = False
    want.normalizer_spec.escape_whitespaces = True
    got_bytes = h.sp.serialized_model_proto()
    got = pb().ModelProto()
    got.ParseFromString(got_bytes)
    assert got == want
    assert got.normalizer_spec.HasField("escape_whitespaces") and got.normalizer_spec.HasField("add_dummy_prefix")
    assert got.SerializeToString() == want.SerializeToString()         # unknown fields included
    if variant == "unknown_field":
        assert bytes([(77 << 3) & 0x7F | 0x80, (77 << 3) >> 7, 5]) in got.normalizer_spec.SerializeToString()
    ids = h.sp.EncodePacked(text, offs)
    same(ids, oracle.load(want.SerializeToString()).encode_batch(text, offs), variant)
    same(backend[1].load(got_bytes).sp.EncodePacked(text, offs), ids, "a fresh handle from the bytes")
    # name / normalization_rule_tsv: the proto changes, the ids do not
    h.sp.OverrideNormalizerSpec(name="identity", normalization_rule_tsv="rules.tsv")
    want.normalizer_spec.name = "identity"
    want.normalizer_spec.normalization_rule_tsv = "rules.tsv"
    got.ParseFromString(h.sp.serialized_model_proto())
    assert got == want and got.normalizer_spec.name == "identity"
    same(h.sp.EncodePacked(text, offs), ids, "name")


def test_empty_charsmap_override(backend, oracle, corpora):
    """precompiled_charsmap="" (no rules at all): the oracle on the equally edited blob, full-width forms left alone."""
    blob = fixtures.model_blob("test_model")
    h = backend[1].load(blob)
    h.sp.OverrideNormalizerSpec(precompiled_charsmap="")
    eblob = edited(blob, precompiled_charsmap=b"")
    o = oracle.load(eblob)
    got = pb().ModelProto()
    got.ParseFromString(h.sp.serialized_model_proto())
    want = pb().ModelProto()
    want.ParseFromString(eblob)
    assert got == want and got.normalizer_spec.HasField("precompiled_charsmap")
    lines = ["ＡＢＣ㍿ full width".encode(), "ｶﾞ half".encode()]
    for name, k in (("edge", 10 ** 6), ("botchan", 200)):
        text, offs = fixtures.head(*corpora[name], k)
        same(h.sp.EncodePacked(text, offs), o.encode_batch(text, offs), name)
        same(h.sp.NormalizePacked(text, offs, with_offsets=True), o.normalize_batch(text, offs), name)
    for line in lines:
        assert h.sp.EncodeAsIds(line.decode()) == list(o.encode(line))
    assert h.sp.EncodeAsIds(lines[0].decode()) != list(oracle.load(blob).encode(lines[0]))    # the rules mattered


class EmuProcessor(SentencePieceProcessor):
    """The product's class bound to the emulated library: what ``self.__init__()`` inside ``__setstate__`` needs on a
    machine without a GPU.  Nothing else differs."""

    def __init__(self, *args, **kw):
        kw.setdefault("_lib", emulib.lib())
        super().__init__(*args, **kw)


def _processor_class(kind):
    return SentencePieceProcessor if kind == "gpu" else EmuProcessor


def test_pickle_and_deepcopy(backend, oracle, corpora, tmp_path):
    cls = _processor_class(backend[0])
    blob = fixtures.model_blob("test_model")
    text, offs = fixtures.head(*corpora["botchan"], 200)
    sp = cls(model_proto=blob)
    assert sp.__getstate__() == sp.serialized_model_proto() == blob
    assert sp["▁the"] == sp.PieceToId("▁the") != sp.unk_id()
    same(pickle.loads(pickle.dumps(sp)).EncodePacked(text, offs), oracle.load(blob).encode_batch(text, offs), "plain")
    sp.OverrideNormalizerSpec(add_dummy_prefix=False, remove_extra_whitespaces=False)
    want = oracle.load(edited(blob, add_dummy_prefix=False, remove_extra_whitespaces=False)).encode_batch(text, offs)
    assert sp.__getstate__() == sp.serialized_model_proto() != blob
    for clone in (pickle.loads(pickle.dumps(sp)), copy.deepcopy(sp), copy.copy(sp)):
        assert clone._h and clone._h.value != sp._h.value
        assert clone.NormalizerSpec() == sp.NormalizerSpec() == dict(zip(FLAGS, (False, False, True)))
        same(clone.EncodePacked(text, offs), want, "clone")
    same(sp.EncodePacked(text, offs), want, "the original")
    # pickled here, loaded in a fresh child process
    state = tmp_path / "sp.pickle"
    state.write_bytes(pickle.dumps(sp))
    child = ("import pickle, sys\n"
             "sys.path.insert(0, %r)\n"
             "sp = pickle.load(open(%r, 'rb'))\n"
             "print(type(sp).__name__, sp.NormalizerSpec()['add_dummy_prefix'])\n"
             "print(' '.join(str(i) for i in sp.EncodeAsIds(' hello  world ')))\n") % (ROOT, str(state))
    out = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.strip().split("\n")
    assert rows[0] == "%s False" % cls.__name__
    o = oracle.load(edited(blob, add_dummy_prefix=False, remove_extra_whitespaces=False))
    assert [int(x) for x in rows[1].split()] == list(o.encode(" hello  world "))


def _raw_override(lib, handle, pairs):
    n = len(pairs)
    names = (C.c_char_p * n)(*[k.encode() for k, _ in pairs])
    vals = (C.c_char_p * n)(*[v for _, v in pairs])
    lens = (C.c_uint64 * n)(*[len(v) for _, v in pairs])
    rc = lib.spmx_override_normalizer_spec(handle, names, vals, lens, n)
    return rc, lib.spmx_last_error(handle).decode()


def test_errors(backend, oracle, corpora):
    blob = fixtures.model_blob("test_model")
    text, offs = fixtures.head(*corpora["botchan"], 200)
    h = backend[1].load(blob)
    base = oracle.load(blob).encode_batch(text, offs)
    # the C ABI: codes and texts
    assert _raw_override(h.lib, h.sp._h, [("no_such_field", b"1")]) == (5, 'unknown field name "no_such_field" in NormalizerSpec.')
    assert _raw_override(h.lib, h.sp._h, [("add_dummy_prefix", b"perhaps")]) == (3, 'cannot parse "perhaps" as bool.')
    same(h.sp.EncodePacked(text, offs), base, "after an error")
    assert h.sp.serialized_model_proto() == blob
    # Python: the SWIG layer's exception types (sentencepiece.i:70-82)
    with pytest.raises(OSError, match="unknown field name"):
        h.sp.OverrideNormalizerSpec(no_such_field=1)
    with pytest.raises(SyntaxError, match='cannot parse "2" as bool'):
        h.sp.OverrideNormalizerSpec(escape_whitespaces=2)
    same(h.sp.EncodePacked(text, offs), base, "after an exception")
    # the pairs before the failing one are applied, that one and the ones behind it are not
    with pytest.raises(SyntaxError):
        h.sp.OverrideNormalizerSpec(add_dummy_prefix="F", remove_extra_whitespaces="nope", escape_whitespaces="false")
    assert h.sp.NormalizerSpec() == dict(zip(FLAGS, (False, True, True)))
    eblob = edited(blob, add_dummy_prefix=False)
    same(h.sp.EncodePacked(text, offs), oracle.load(eblob).encode_batch(text, offs), "the pair before the failing one")
    got, want = pb().ModelProto(), pb().ModelProto()
    got.ParseFromString(h.sp.serialized_model_proto())
    want.ParseFromString(eblob)
    assert got == want
    # every spelling lexical_cast<bool> takes (src/util.h:60-77); an empty value is true (PARSE_BOOL)
    for v, want_flag in (("1", True), ("t", True), ("TRUE", True), ("y", True), ("Yes", True), ("", True),
                         ("0", False), ("f", False), ("False", False), ("n", False), ("NO", False)):
        h.sp.OverrideNormalizerSpec(add_dummy_prefix=v)
        assert h.sp.NormalizerSpec()["add_dummy_prefix"] is want_flag, v
    # a charsmap blob that a load refuses: load's error, a RuntimeError in Python, and the handle works on
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=True)
    bad = b"\xff\xff\xff\x7f" + b"x" * 40
    with pytest.raises(RuntimeError, match="Trie data size exceeds the input blob size."):
        h.sp.OverrideNormalizerSpec(escape_whitespaces=False, precompiled_charsmap=bad)
    with pytest.raises(RuntimeError, match="Trie data size exceeds the input blob size."):
        backend[1].load(edited(blob, precompiled_charsmap=bad))
    assert h.sp.NormalizerSpec() == dict(zip(FLAGS, (True, True, True)))
    same(h.sp.EncodePacked(text, offs), base, "after a refused charsmap")
    m = pb().ModelProto()
    m.ParseFromString(h.sp.serialized_model_proto())
    assert m.normalizer_spec.precompiled_charsmap == pb().ModelProto.FromString(blob).normalizer_spec.precompiled_charsmap


def test_an_override_that_changes_nothing(backend):
    """Every field at its current value: the proto gets the fields written explicitly, everything else stays -- the table
    bytes spmx_handle_info reports, the ids.  Then three switches in one call."""
    blob = fixtures.model_blob("test_model")
    h = backend[1].load(blob)
    before = h.sp.HandleInfo()["table_bytes"]
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=True, escape_whitespaces="yes", name="nfkc")
    assert h.sp.HandleInfo()["table_bytes"] == before
    got = pb().ModelProto()
    got.ParseFromString(h.sp.serialized_model_proto())
    assert got == pb().ModelProto.FromString(edited(blob, add_dummy_prefix=True, escape_whitespaces=True, name="nfkc"))
    assert h.sp.Encode(" hello  world ", out_type=str) == ["▁he", "ll", "o", "▁world"]
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=False, remove_extra_whitespaces=False, escape_whitespaces=False)
    fresh = backend[1].load(h.sp.serialized_model_proto())        # (asked for its table bytes only)
    assert h.sp.HandleInfo()["table_bytes"] == fresh.sp.HandleInfo()["table_bytes"] > 0
    assert h.sp.Encode(" hello  world ", out_type=str) == [" ", "he", "ll", "o", "  ", "w", "or", "l", "d", " "]


def test_concurrent_callers_around_an_override(backend, oracle, corpora):
    """tests/test_host.py::test_emu_concurrent_callers with an override between two rounds: four threads, three calls
    each, joined; the override; the same threads again against the new expectation."""
    blob = fixtures.model_blob("test_model")
    h = backend[1].load(blob)
    parts = [fixtures.head(*corpora[name], k) for name, k in (("botchan", 400), ("edge", 10 ** 6), ("synth20k", 500), ("mixed2k", 60))]

    def round_(o):
        want = [o.encode_batch(t, of) for t, of in parts]
        got = [None] * len(parts)

        def run(i):
            for _ in range(3):
                got[i] = h.sp.EncodePacked(*parts[i])
        threads = [threading.Thread(target=run, args=(i,)) for i in range(len(parts))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for g, w in zip(got, want):
            assert g is not None
            same(g, w, "threads")

    round_(oracle.load(blob))
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=False, remove_extra_whitespaces=False)
    round_(oracle.load(edited(blob, add_dummy_prefix=False, remove_extra_whitespaces=False)))
    h.sp.OverrideNormalizerSpec(escape_whitespaces=False)
    round_(oracle.load(edited(blob, add_dummy_prefix=False, remove_extra_whitespaces=False, escape_whitespaces=False)))


def _build_facade_driver(emu):
    src = os.path.join(ROOT, "tests", "cpp", "override_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    out = os.path.join(ROOT, "tests", "cpp", "override_test" + ("_emu" if emu else ""))
    if emu:
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(ROOT, "include", "spmx_processor.h"),
                                               os.path.join(ROOT, "include", "spmx.h"), so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-I" + os.path.join(ROOT, "include"), "-L" + lib,
                               "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("model", ["test_model", "bpe1k_llama"])
def test_cpp_facade(model, backend, oracle, tmp_path):
    """tests/cpp/override_test.cc: mutable_normalizer_spec()->set_*() and OverrideNormalizerSpec(map) of
    include/spmx_processor.h; every section of its output against the oracle on the equally edited blob."""
    exe = _build_facade_driver(emu=backend[0] == "emu")
    blob = fixtures.model_blob(model)
    with open(os.path.join(fixtures.GOLDEN, "botchan.txt"), "rb") as f:
        lines = f.read().split(b"\n")[:120] + [b" hello  world ", b"", "ＡＢＣ  x".encode()]
    tp, pp = tmp_path / "in.txt", tmp_path / "out.model"
    tp.write_bytes(b"\n".join(lines) + b"\n")
    env = dict(os.environ)
    if backend[0] == "emu":
        env.update(SPMX_EMU_CUS="2")
    out = subprocess.run([exe, os.path.join(fixtures.GOLDEN, model + ".model"), str(tp), str(pp)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    a, r, e = loaded_flags(blob)
    want_sections = [("loaded", (a, r, e)), ("set_add_dummy_prefix", (not a, r, e)), ("set_escape_and_remove", (not a, not r, not e)),
                     ("override_all_true", (True, True, True)), ("name_and_tsv", (True, True, True)), ("after_errors", (True, True, True))]
    rows = out.stdout.split("\n")
    errors = [x for x in rows if x.startswith("E ")]
    assert errors == ['E 5|unknown field name "no_such_field" in NormalizerSpec.', 'E 3|cannot parse "perhaps" as bool.']
    rows = [x for x in rows if not x.startswith("E ")]
    text = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.zeros(len(lines) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lines])
    k = 0
    for label, flags in want_sections:
        assert rows[k] == "== %s %d %d %d" % ((label,) + tuple(int(x) for x in flags)), rows[k]
        ids, io = oracle.load(edited(blob, **dict(zip(FLAGS, flags)))).encode_batch(text, offs)
        for i in range(len(lines)):
            assert [int(x) for x in rows[k + 1 + i].split()] == ids[int(io[i]):int(io[i + 1])].tolist(), (label, i)
        k += 1 + len(lines)
    got, want = pb().ModelProto(), pb().ModelProto()
    got.ParseFromString(pp.read_bytes())
    want.ParseFromString(edited(blob, add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True, name="identity",
                                normalization_rule_tsv="rules.tsv"))
    assert got == want
