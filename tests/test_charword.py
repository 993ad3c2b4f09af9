"""Character and word models (model_type CHAR / WORD) on the device path: csrc/kernels_charword.h inside the streaming
launch, their tables (csrc/tables.cc), and everything around them that had only seen unigram and BPE models.

Expected values: tests/golden/charword_golden.npz / .json -- the compiled reference (oracle/_ref) on
scripts/make_charword_fixtures.py inputs(model) -- and, where oracle/_ref is built, the live reference as well.  Every
test runs with the device emulated and, with -m gpu, on the product library.

On the parent of the commit that added these models every test here fails at load: kUnimplemented, "only unigram and
bpe models are on the device path"."""
import ctypes as C
import functools
import hashlib
import json
import os
import pickle
import subprocess
import threading

import numpy as np
import pytest

from scripts import make_charword_fixtures as cw
from sentencepiece_amd import synth
from sentencepiece_amd.processor import SentencePieceProcessor
from tests import emulib, fixtures, refshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = list(cw.MODELS)
INTERNAL = 13


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.param, emulib.backend(request.param)


class EmuProcessor(SentencePieceProcessor):
    """The product's class bound to the emulated library (what unpickling needs on a machine without a GPU)."""

    def __init__(self, *args, **kw):
        kw.setdefault("_lib", emulib.lib())
        super().__init__(*args, **kw)


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(fixtures.GOLDEN, "charword_golden.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(fixtures.GOLDEN, "charword_golden.npz"))


@functools.lru_cache(maxsize=None)
def expected(model):
    """(ids int32, id offsets uint64) of inputs(model)."""
    _, g = golden()
    return g[model + "__ids"].astype(np.int32), g[model + "__io"].astype(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(model):
    return refshim.RefLib().load(fixtures.model_blob(model)) if refshim.available() else None


def same(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64), err_msg=str(what))


def sentences(text, offs, idx):
    tb = np.asarray(text).tobytes()
    return [tb[int(offs[i]):int(offs[i + 1])] for i in idx]


def batch(model, kind):
    """inputs(model) and its expected ids; the emulated tests leave out the two 1 MiB sentences that close it (their
    class table ends at 64 KiB: 65537 bytes is already beyond its last class)."""
    text, offs = cw.inputs(model)
    ids, io = expected(model)
    n = len(offs) - 1 - (cw.N_TAIL if kind == "emu" else 0)
    return (text[:int(offs[n])], offs[:n + 1]), (ids[:int(io[n])], io[:n + 1])


def small(model):
    """The edge corpus and 300 lines: the head of inputs(model), with its expected ids."""
    text, offs = cw.inputs(model)
    ids, io = expected(model)
    n = len(fixtures.mf.edge_sentences()) + 300
    return (text[:int(offs[n])], offs[:n + 1]), (ids[:int(io[n])], io[:n + 1])


@pytest.mark.parametrize("model", MODELS)
def test_parity(model, backend):
    """One batch -- edge cases, text, a document, a sentence at every length class's capacity and one byte beyond, an
    empty and an all-space sentence -- through the host entry, the device-resident entry, the spans entry and Decode."""
    import torch
    kind, lib = backend
    meta, g = golden()
    (text, offs), (ids, io) = batch(model, kind)
    h = lib.load(fixtures.model_blob(model))
    assert h.sp.model_type() == (4 if model.startswith("char") else 3)
    # ---- the host entry (spmx_encode_batch_ex) ----
    got = h.encode_batch(text, offs)
    same(got, (ids, io), (model, "host entry"))
    assert h.status == 0 and not h.sent_status.any()
    wave = "CharWordWaveKernel" in [c["kernel"] for c in h.sp.LastProfile()["classes"]]
    if model == "char_uds":                                 # (a cut's start depends on the cut before it: the lane form only)
        assert not wave and h.path()["overflow"] >= 1       # (a sentence beyond the last class: the exact-capacity launch ran)
    else:
        assert wave                                         # the documents took the wave-cooperative form (kernels_charwave.h)
    if model in ("char1k", "word1k"):
        assert h.path()["overflow"] >= 1                    # ... and so did what fits no text column: the overflow list
    r = reference(model)
    if r is not None:
        same(r.encode_batch(text, offs, threads=4), (ids, io), (model, "the golden file is stale"))
    # ---- the device-resident entry (spmx_encode_batch_device) ----
    dev = "cuda" if kind == "gpu" else "cpu"
    d_ids, d_io, total = h.sp.EncodeDevice(torch.from_numpy(np.asarray(text)).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev))
    assert total == len(ids)
    same((d_ids[:total].cpu().numpy(), d_io.cpu().numpy()), (ids, io), (model, "device entry"))
    # ---- Decode of the ids ----
    want_of = meta[model] if kind == "gpu" else meta[model]["head"]   # (digests of the whole batch / without its 1 MiB tail)
    dt, do = h.sp.DecodePacked(ids, io)
    assert len(dt) == want_of["decode_bytes"]
    assert hashlib.sha256(dt.tobytes() + do.astype("<u8").tobytes()).hexdigest() == want_of["decode_sha256"]
    if r is not None and kind == "emu":
        same((dt, do), r.decode_batch(ids, io), (model, "decode"))
    # ---- the spans entry: ids + the byte range of every piece ----
    sids, sb, se, sio = h.sp.EncodeSpansPacked(text, offs)
    same((sids, sio), (ids, io), (model, "spans entry"))
    assert hashlib.sha256(sb.astype("<u4").tobytes() + se.astype("<u4").tobytes()).hexdigest() == want_of["spans_sha256"]
    if r is not None:
        same((sids, sb, se, sio), r.encode_spans(text, offs), (model, "spans"))
    # ---- SentencePieceText, byte for byte; spmx_encode, a sentence at a time ----
    idx = cw.proto_sample(offs)
    lines = sentences(text, offs, idx)
    po = g[model + "__proto_offs"].astype(np.int64)
    pblob = g[model + "__protos"].tobytes()
    want = [pblob[po[k]:po[k + 1]] for k in range(len(idx))]
    assert h.sp.EncodeAsSerializedProto(lines) == want
    if r is not None:
        assert cw.ref_serialized(r, *synth.pack(lines)) == want
    out = np.zeros(4 * cw.PROTO_MAX_RAW + 64, dtype=np.int32)
    for i, line in zip(idx, lines):
        n_ids = C.c_uint64(0)
        assert h.lib.spmx_encode(h.sp._h, line, len(line), out.ctypes.data, len(out), C.byref(n_ids)) == 0
        assert out[:n_ids.value].tolist() == ids[int(io[i]):int(io[i + 1])].tolist(), (model, i)


def apply_options(ids, io, opts, bos=1, eos=2):
    """ApplyExtraOptions (sentencepiece_processor.cc:1019-1064) on every row of a CSR of ids."""
    io = io.astype(np.int64)
    rows = []
    for i in range(len(io) - 1):
        row = ids[io[i]:io[i + 1]].tolist()
        for o in opts.split(":"):
            if o == "reverse":
                row.reverse()
            elif o == "bos":
                row.insert(0, bos)
            elif o == "eos":
                row.append(eos)
        rows.append(row)
    flat = np.array([t for r in rows for t in r], dtype=np.int32)
    return flat, np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)


@pytest.mark.parametrize("model", ["char_uds", "char_bf", "word_suffix", "word_bf"])
def test_extra_options_and_pieces(model, backend):
    """bos / eos / reverse / unk_piece in several orders: the ids are the golden rows with ApplyExtraOptions applied; the
    spans and the piece strings (the merged unknown piece is the concatenation of its cuts; byte pieces under byte
    fallback) against the live reference where it is built."""
    r = reference(model)
    (text, offs), (ids, io) = small(model)
    h = backend[1].load(fixtures.model_blob(model))
    assert (h.sp.bos_id(), h.sp.eos_id()) == (1, 2)
    lines = sentences(text, offs, range(0, len(offs) - 1, 5))
    try:
        for opts in ("bos:eos", "reverse", "eos:reverse:bos", "reverse:unk_piece:bos"):
            h.set_encode_extra_options(opts)
            same(h.encode_batch(text, offs), apply_options(ids, io, opts), (model, opts))
            sids, sb, se, sio = h.sp.EncodeSpansPacked(text, offs)
            same((sids, sio), apply_options(ids, io, opts), (model, opts, "spans entry"))
            if r is not None:
                r.set_encode_extra_options(opts)
                same(r.encode_batch(text, offs), apply_options(ids, io, opts), (model, opts, "reference"))
                same((sids, sb, se, sio), r.encode_spans(text, offs), (model, opts, "spans"))
                assert h.sp.EncodeAsSerializedProto(lines) == cw.ref_serialized(r, *synth.pack(lines)), (model, opts)
    finally:
        if r is not None:
            r.set_encode_extra_options("")


def _message(status_text):
    """'Internal: file(line) [condition] message' -> (code name, message)."""
    code, rest = status_text.split(": ", 1)
    return code, rest.split("] ", 1)[1]


@pytest.mark.parametrize("model", ["char_ident", "word_ident"])
def test_refusals(model, backend):
    """The calls the reference refuses for these models are refused with its status code and message, and the handle
    keeps working."""
    (text, offs), want = small(model)
    h = backend[1].load(fixtures.model_blob(model))
    lib, hh = h.lib, h.sp._h
    t1, o1 = synth.pack([b"hello world"])
    outs = [C.c_void_p() for _ in range(4)]
    refs = [C.byref(p) for p in outs]
    calls = {
        "nbest": lambda: lib.spmx_nbest_encode_batch(hh, t1.ctypes.data, o1.ctypes.data, 1, 3, *refs),
        "sample": lambda: lib.spmx_sample_encode_batch(hh, t1.ctypes.data, o1.ctypes.data, 1, -1, C.c_float(0.1), 0, refs[0], refs[1]),
        "sample_nbest": lambda: lib.spmx_sample_encode_batch(hh, t1.ctypes.data, o1.ctypes.data, 1, 1, C.c_float(0.1), 0, refs[0], refs[1]),
        "original": lambda: lib.spmx_encode_batch_original(hh, t1.ctypes.data, o1.ctypes.data, 1, refs[0], refs[1]),
        "set_vocabulary": lambda: lib.spmx_set_vocabulary(hh, (C.c_char_p * 1)(b"a"), (C.c_uint64 * 1)(1), 1),
    }
    messages = {"nbest": "NBestEncode is not available for the current model.",
                "sample": "SampleEncode is not available for the current model.",
                "sample_nbest": "SampleEncode is not available for the current model.",
                # (the kOriginal entry has no counterpart in the reference's processor -- there it is a switch on a unigram
                # model -- so this string is the product's own: its lattice entries share one refusal)
                "original": "SampleEncode is not available for the current model.",
                "set_vocabulary": "Vocabulary constraint is only enabled in subword units."}
    r = reference(model)
    if r is not None:                                       # the table above is the reference's
        ids = np.zeros(64, np.int32)
        fn = r.lib.spmref_nbest_encode
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        assert fn(r.h, b"hello world", 11, 3, ids.ctypes.data, 64, np.zeros(8, np.uint64).ctypes.data, np.zeros(8, np.float32).ctypes.data) == -1
        assert _message(r.lib.spmref_last_error(r.h).decode()) == ("Internal", messages["nbest"])
        for k in (-1, 1):
            with pytest.raises(RuntimeError):
                r.sample_encode(b"hello world", k, 0.1)
            assert _message(r.lib.spmref_last_error(r.h).decode()) == ("Internal", messages["sample"])
        with pytest.raises(RuntimeError) as e:
            r.set_vocabulary(["a"])
        assert _message(str(e.value)) == ("Internal", messages["set_vocabulary"])
    for name, call in calls.items():
        assert call() == INTERNAL, name
        assert lib.spmx_last_error(hh).decode() == messages[name], name
        assert all(p.value is None for p in outs), name
        same(h.encode_batch(text, offs), want, (model, "after", name))
    with pytest.raises(RuntimeError, match="SampleEncode is not available"):
        h.sp.EncodeOriginalPacked(t1, o1)
    with pytest.raises(RuntimeError, match="NBestEncode is not available"):
        h.sp.NBestEncodeAsIds("hello world", 3)
    same(h.encode_batch(text, offs), want, (model, "after the Python forms"))


def _edited(blob, **fields):
    from sentencepiece import sentencepiece_model_pb2 as pb
    m = pb.ModelProto()
    m.ParseFromString(blob)
    for k, v in fields.items():
        setattr(m.normalizer_spec, k, v)
    return m.SerializeToString()


def test_override_normalizer_spec(backend):
    """OverrideNormalizerSpec(add_dummy_prefix=False) on word1k: as a handle loaded from the equally edited blob -- whose
    expected ids come from the compiled reference where it is built."""
    blob = fixtures.model_blob("word1k")
    (text, offs), before = small("word1k")
    h = backend[1].load(blob)
    same(h.encode_batch(text, offs), before, "before")
    h.sp.OverrideNormalizerSpec(add_dummy_prefix=False)
    eblob = _edited(blob, add_dummy_prefix=False)
    fresh = backend[1].load(eblob)
    got = h.encode_batch(text, offs)
    same(got, fresh.encode_batch(text, offs), "override against a fresh handle")
    assert len(got[0]) != len(before[0])                    # (it mattered: the first word of a sentence is another word now)
    same(h.sp.EncodeSpansPacked(text, offs), fresh.sp.EncodeSpansPacked(text, offs), "spans")
    same(h.sp.NormalizePacked(text, offs, with_offsets=True), fresh.sp.NormalizePacked(text, offs, with_offsets=True), "normalize")
    assert h.sp.serialized_model_proto() == fresh.sp.serialized_model_proto()
    if refshim.available():
        r = refshim.RefLib().load(eblob)
        same(got, r.encode_batch(text, offs), "override against the reference")
        same(h.sp.DecodePacked(*got), r.decode_batch(*got), "decode")


@pytest.mark.parametrize("model", ["char_uds", "word_keepws"])
def test_pickle_round_trip(model, backend):
    cls = SentencePieceProcessor if backend[0] == "gpu" else EmuProcessor
    blob = fixtures.model_blob(model)
    (text, offs), want = small(model)
    sp = cls(model_proto=blob)
    assert sp.serialized_model_proto() == blob
    clone = pickle.loads(pickle.dumps(sp))
    assert clone._h and clone._h.value != sp._h.value and clone.model_type() == sp.model_type()
    same(clone.EncodePacked(text, offs), want, "clone")
    same(sp.EncodePacked(text, offs), want, "original")
    assert clone.GetScore(5) == sp.GetScore(5)
    assert clone.Decode(clone.EncodeAsIds("the cat sat"), out_type=str) == sp.Decode(sp.EncodeAsIds("the cat sat"), out_type=str)


def test_set_vocabulary_refused_then_reset(backend):
    """SetVocabulary (and so LoadVocabulary, which ends in it: sentencepiece_processor.cc:329-352) is refused and changes
    nothing; ResetVocabulary is harmless."""
    (text, offs), want = small("word_ident")
    h = backend[1].load(fixtures.model_blob("word_ident"))
    with pytest.raises(RuntimeError, match="only enabled in subword units"):
        h.sp.SetVocabulary(["▁the"])
    same(h.encode_batch(text, offs), want, "after SetVocabulary")
    h.sp.ResetVocabulary()
    same(h.encode_batch(text, offs), want, "after ResetVocabulary")


def test_encode_file(backend, tmp_path):
    """EncodeFile on a character model: the bytes `spm_encode --output_format=id` of the compiled reference writes."""
    model = "char_bf"
    (text, offs), (ids, io) = small(model)
    lines = [ln for ln in sentences(text, offs, range(len(offs) - 1)) if b"\n" not in ln and b"\r" not in ln and b"\x00" not in ln]
    src, out = tmp_path / "in.txt", tmp_path / "out.ids"
    src.write_bytes(b"\n".join(lines) + b"\n")
    h = backend[1].load(fixtures.model_blob(model))
    ns, ni = h.sp.EncodeFile(str(src), str(out), "id")
    rows = h.sp.EncodePacked(*synth.pack(lines))
    rio = rows[1].astype(np.int64)
    want = "".join(" ".join(str(t) for t in rows[0][rio[i]:rio[i + 1]]) + "\n" for i in range(len(lines))).encode()
    assert (ns, ni) == (len(lines), len(rows[0]))
    assert out.read_bytes() == want
    tool = os.path.join(ROOT, "oracle", "_ref", "spm_encode")
    if os.path.exists(tool):
        mp = tmp_path / "m.model"
        mp.write_bytes(fixtures.model_blob(model))
        ref_out = subprocess.run([tool, "--model=" + str(mp), "--output_format=id", "--input=" + str(src)], capture_output=True)
        assert ref_out.returncode == 0, ref_out.stderr
        assert out.read_bytes() == ref_out.stdout


def test_two_host_threads_on_one_handle(backend):
    h = backend[1].load(fixtures.model_blob("char1k"))
    (text, offs), want = small("char1k")
    n = len(offs) - 1
    cut = n // 2
    parts = [((text[:int(offs[cut])], offs[:cut + 1]), (want[0][:int(want[1][cut])], want[1][:cut + 1])), ((text, offs), want)]
    got = [None, None]

    def run(i):
        for _ in range(3):
            got[i] = h.sp.EncodePacked(*parts[i][0])
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(2):
        assert got[i] is not None
        same(got[i], parts[i][1], ("thread", i))


def test_list_form_and_pieces(backend):
    """The list form (spmx_encode_batch_views through Encode(list)) and the piece strings on a word model: the pieces of
    a sentence tile its normalized text (a merged unknown piece is the concatenation of its cuts)."""
    model = "word_nodummy"
    (text, offs), (ids, io) = small(model)
    h = backend[1].load(fixtures.model_blob(model))
    lines = [ln.decode("utf-8") for ln in sentences(text, offs, range(60, 160))]
    io64 = io.astype(np.int64)
    assert h.sp.Encode(lines, out_type=int) == [ids[io64[i]:io64[i + 1]].tolist() for i in range(60, 160)]
    for ln, pieces in zip(lines, h.sp.Encode(lines, out_type=str)):
        assert "".join(pieces) == h.sp.Normalize(ln), ln


def _build_cpp_driver(emu):
    src = os.path.join(ROOT, "tests", "cpp", "charword_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    out = os.path.join(ROOT, "tests", "cpp", "charword_test" + ("_emu" if emu else ""))
    if emu:
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(ROOT, "include", "spmx_processor.h"),
                                               os.path.join(ROOT, "include", "spmx.h"), so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-L" + lib,
                               "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("model", ["char_uds", "word_suffix"])
def test_cpp_facade(model, backend, tmp_path):
    """The header-only C++ SentencePieceProcessor (include/spmx_processor.h) on these models: tests/cpp/charword_test.cc
    -- Load, Encode per line, EncodeBatch over all lines, the refused calls (LoadVocabulary among them) -- prints the golden ids and the reference's
    Status codes and messages."""
    binary = _build_cpp_driver(backend[0] == "emu")
    (text, offs), (ids, io) = small(model)
    io64 = io.astype(np.int64)
    keep = [i for i, ln in enumerate(sentences(text, offs, range(len(offs) - 1))) if b"\n" not in ln]
    src = tmp_path / "in.txt"
    src.write_bytes(b"\n".join(sentences(text, offs, keep)) + b"\n")
    vocab = tmp_path / "vocab.tsv"
    vocab.write_text("▁the\t10\na\t5\n", encoding="utf-8")
    out = subprocess.run([binary, os.path.join(fixtures.GOLDEN, model + ".model"), str(src), str(vocab)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.split("\n")
    got = [int(x) for line in rows if not line.startswith("R ") for x in line.split()]
    assert got == [int(t) for i in keep for t in ids[io64[i]:io64[i + 1]]]
    assert [line for line in rows if line.startswith("R ")] == [
        "R nbest 13|NBestEncode is not available for the current model.",
        "R sample 13|SampleEncode is not available for the current model.",
        "R set_vocabulary 13|Vocabulary constraint is only enabled in subword units.",
        "R load_vocabulary 13|Vocabulary constraint is only enabled in subword units."]
