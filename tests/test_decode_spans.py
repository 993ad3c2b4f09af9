"""Decode to SentencePieceText (src/sentencepiece_processor.cc:766-925): the spans form of the decode kernels
(csrc/kernels_decode.h decode_body<true, true>), spmx_decode_batch_spans*, the Python out_types and the C++ facade.

Golden bytes: tests/golden/decode_protos.json (scripts/make_decode_proto_golden.py: the reference's serialized protos per
row of ids / of piece strings, no extra options).  The decode extra options are checked through what ApplyExtraOptions
(:1019-1064) does to the piece list: the proto under an option equals the no-option proto of the transformed row.
One checker, an emulator twin (CPU) and a -m gpu twin per model."""
import base64
import hashlib
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

from tests import fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["test_model", "uni1k_bf", "bpe1k_bf_uds", "uni1k_suffix", "bpe1k_llama", "test_ja_model", "uni1k_ident", "uni1k_ident_dn"]
DENORMALIZED = {"uni1k_ident_dn"}
OPTIONS = ["reverse", "bos:eos", "eos:reverse:bos"]

_golden = None


def golden(model):
    """{"ids" | "pieces": {"groups", "rows", "protos"}} of one model, unpacked once per session."""
    global _golden
    if _golden is None:
        with open(os.path.join(fixtures.GOLDEN, "decode_protos.json"), encoding="utf-8") as f:
            packed = json.load(f)["models"]
        _golden = {m: {form: json.loads(lzma.decompress(base64.b64decode(v[form])).decode("utf-8")) for form in ("ids", "pieces")}
                   for m, v in packed.items()}
    return _golden[model]


def same(blob, want):
    """want: the proto in hex, or "sha256:" + its digest (the random rows)."""
    if want.startswith("sha256:"):
        return hashlib.sha256(blob).hexdigest() == want[7:]
    return blob.hex() == want


# ---- a reader of the wire format, for the invariants (the product's writer is pinned by the golden bytes) ----
def _varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, i


def _fields(b):
    i, out = 0, []
    while i < len(b):
        key, i = _varint(b, i)
        if key & 7 == 2:
            n, i = _varint(b, i)
            out.append((key >> 3, b[i:i + n]))
            i += n
        elif key & 7 == 0:
            v, i = _varint(b, i)
            out.append((key >> 3, v))
        else:
            raise AssertionError("unexpected wire type in a Decode proto")
    return out


def parse(blob):
    """-> (text bytes | None, [(piece, id, surface | None, begin | None, end | None)])"""
    text, pieces = None, []
    for num, v in _fields(blob):
        if num == 1:
            text = v
        elif num == 2:
            d = dict(_fields(v))
            pieces.append((d.get(1), d.get(2), d.get(3), d.get(4), d.get(5)))
    return text, pieces


def check_invariants(blob, plain_text, raw_text, where):
    """Every piece has surface / begin / end; the surfaces tile the text before the denormalizer; `text` is what plain
    Decode gives.  raw_text: that text where the caller has it, else None.  Returns the concatenated surfaces."""
    text, pieces = parse(blob)
    assert text is not None and text == plain_text, where
    pos = 0
    for k, (piece, pid, surface, begin, end) in enumerate(pieces):
        assert piece is not None and pid is not None and surface is not None and begin is not None and end is not None, (where, k)
        assert begin == pos and end == begin + len(surface), (where, k)
        pos = end
    cat = b"".join(p[2] for p in pieces)
    assert pos == len(cat), where
    if raw_text is not None:
        assert cat == raw_text, where
    return cat


def apply_options(row, opts, bos, eos):
    """ApplyExtraOptions (:1019-1064) on a row of ids or of piece strings."""
    row = list(row)
    for o in opts.split(":"):
        if o == "reverse":
            row.reverse()
        elif o == "eos":
            row.append(eos)
        elif o == "bos":
            row.insert(0, bos)
    return row


def check_model(sp, model):
    g = golden(model)
    n = sp.GetPieceSize()
    dn = model in DENORMALIZED
    differs = 0
    for form in ("ids", "pieces"):
        rows, protos = g[form]["rows"], g[form]["protos"]
        assert len(rows) == len(protos) and len(rows) >= 40
        one = sp.DecodeIdsAsSerializedProto if form == "ids" else sp.DecodePiecesAsSerializedProto
        many = sp.Decode if form == "ids" else sp.DecodePieces
        by_row = {json.dumps(r, ensure_ascii=False): p for r, p in zip(rows, protos)}
        # ---- goldens: one call per row, then all rows in one batch ----
        for i, (row, want) in enumerate(zip(rows, protos)):
            got = one(row)
            assert isinstance(got, bytes) and same(got, want), (model, form, i, row[:8], parse(got))
        base = many(rows, out_type="serialized_proto")
        assert len(base) == len(rows)
        for i, (got, want) in enumerate(zip(base, protos)):
            assert same(got, want), (model, form, i, "batched")
        # ---- invariants of the no-option protos ----
        plain = many(rows, out_type=bytes)
        raws = [None] * len(rows)
        if form == "ids":
            offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
            flat = np.array([t for r in rows for t in r], dtype=np.int32)
            text, to, pid, b, e, po, raw, ro = sp.DecodeSpansPacked(flat, offs)
            np.testing.assert_array_equal(po, offs)
            np.testing.assert_array_equal(pid, flat)
            assert b.dtype == np.uint32 and e.dtype == np.uint32
            rawb = raw.tobytes()
            raws = [rawb[int(ro[i]):int(ro[i + 1])] for i in range(len(rows))]
            assert text.tobytes() == b"".join(plain)
        for i, blob in enumerate(base):
            cat = check_invariants(blob, plain[i], raws[i], (model, form, i))
            if not dn:
                assert cat == plain[i], (model, form, i)
            differs += cat != plain[i]
        # ---- the immutable form: str fields, spans in characters ----
        if not dn:
            for i in list(range(0, len(rows), 7)) + [len(rows) - 1]:
                view = many(rows[i], out_type="immutable_proto")
                text, pieces = parse(base[i])
                assert isinstance(view.text, str) and view.text == text.decode("utf-8")
                assert view.SerializeAsString() == base[i]
                assert len(view.pieces) == len(pieces)
                for p, (piece, pid_, surface, begin, end) in zip(view.pieces, pieces):
                    assert (p.piece, p.id, p.surface) == (piece.decode("utf-8"), pid_, surface.decode("utf-8")), (model, form, i)
                    assert p.begin == len(text[:begin].decode("utf-8")) and p.end == len(text[:end].decode("utf-8")), (model, form, i)
            views = many(rows[:3], out_type="immutable_proto")
            assert [v.SerializeAsString() for v in views] == base[:3]
        # ---- decode extra options ----
        bos, eos = sp.bos_id(), sp.eos_id()
        try:
            for opts in OPTIONS:
                if ("bos" in opts and bos < 0) or ("eos" in opts and eos < 0):
                    continue
                b_, e_ = (bos, eos) if form == "ids" else (sp.IdToPiece(bos) if bos >= 0 else None, sp.IdToPiece(eos) if eos >= 0 else None)
                moved = [apply_options(r, opts, b_, e_) for r in rows]
                sp.SetDecodeExtraOptions("")
                want = many(moved, out_type="serialized_proto")
                want_plain = many(moved, out_type=bytes)
                sp.SetDecodeExtraOptions(opts)
                got = many(rows, out_type="serialized_proto")
                got_plain = many(rows, out_type=bytes)
                hits = 0
                for i in range(len(rows)):
                    assert got[i] == want[i], (model, form, opts, i)
                    assert got_plain[i] == want_plain[i], (model, form, opts, i)
                    check_invariants(got[i], got_plain[i], None, (model, form, opts, i))
                    ref = by_row.get(json.dumps(moved[i], ensure_ascii=False))
                    if ref is not None:
                        hits += 1
                        assert same(got[i], ref), (model, form, opts, i, "golden of the transformed row")
                if opts == "reverse":
                    assert hits >= 2          # the empty and the one-piece rows at least
            if form == "pieces":              # unk: a piece outside the vocabulary becomes the unknown piece (:1050-1058)
                unk = sp.unk_id()
                unk_name = sp.IdToPiece(unk)
                moved = [[unk_name if sp.PieceToId(p) == unk else p for p in r] for r in rows]
                sp.SetDecodeExtraOptions("")
                want = many(moved, out_type="serialized_proto")
                sp.SetDecodeExtraOptions("unk")
                got = many(rows, out_type="serialized_proto")
                assert got == want, (model, "unk")
                assert any(m != r for m, r in zip(moved, rows))
        finally:
            sp.SetDecodeExtraOptions("")
        # ---- errors ----
        if form == "ids":
            for bad in (n, -1):
                for call in (lambda: sp.DecodeIdsAsSerializedProto([1, bad, 2]),
                             lambda: sp.Decode([[1], [2, bad]], out_type="immutable_proto")):
                    with pytest.raises(Exception, match="Invalid id"):
                        call()
            out = sp.DecodeSpansPacked(np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.uint64))
            assert [len(x) for x in out[:6]] == [0, 1, 0, 0, 0, 1] and int(out[5][0]) == 0
        assert parse(one([])) == (b"", [])
        assert many([[], rows[1], []], out_type="serialized_proto") == [base[rows.index([])], base[1], base[rows.index([])]]
    if dn:
        assert differs > 0, "no row of the denormalizer model has a text that differs from its surfaces"
    else:
        assert differs == 0


@pytest.mark.parametrize("model", MODELS)
def test_emu_decode_protos(model):
    from tests import emulib
    check_model(emulib.EmuLib().load(fixtures.model_blob(model), cus=2).sp, model)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_gpu_decode_protos(model):
    from sentencepiece_amd.processor import SentencePieceProcessor
    check_model(SentencePieceProcessor(model_proto=fixtures.model_blob(model)), model)


def check_issue_examples(sp):
    """The spans the reference gives for the named rows, as numbers (uni1k_bf)."""
    def spans(pieces):
        return [(p[3], p[4]) for p in parse(sp.DecodePiecesAsSerializedProto(pieces))[1]]
    filler = "a"
    assert spans([filler] * 62 + ["<0xF0>", "<0x9F>", "<0x98>", "<0x80>"])[-4:] == [(62, 62), (62, 62), (62, 62), (62, 66)]
    text, pieces = parse(sp.DecodePiecesAsSerializedProto(["▁", "▁the", "▁"]))
    assert text == b"the " and [(p[3], p[4]) for p in pieces] == [(0, 0), (0, 3), (3, 4)]
    text, pieces = parse(sp.DecodePiecesAsSerializedProto(["<0xFF>", "<0x80>", "▁the"]))
    assert pieces[-1][2:] == (b" the", 6, 10)
    text, pieces = parse(sp.DecodePiecesAsSerializedProto(["<0xE3>", "<0x81>", "zz", "<0x82>"]))
    assert [p[2] for p in pieces] == [b"\xef\xbf\xbd", b"\xef\xbf\xbd", b"zz", b"\xef\xbf\xbd"]
    text, pieces = parse(sp.DecodePiecesAsSerializedProto(["<s>", "</s>", "<s>"]))
    assert text == b"" and [(p[2], p[3], p[4]) for p in pieces] == [(b"", 0, 0)] * 3


def test_emu_decode_proto_examples():
    from tests import emulib
    check_issue_examples(emulib.EmuLib().load(fixtures.model_blob("uni1k_bf")).sp)


@pytest.mark.gpu
def test_gpu_decode_proto_examples():
    from sentencepiece_amd.processor import SentencePieceProcessor
    check_issue_examples(SentencePieceProcessor(model_proto=fixtures.model_blob("uni1k_bf")))


# ---- the C++ facade: tests/cpp/decode_spans_test.cc, built the way tests/test_cpp_facade.py builds its driver ----
def _build_driver(emu):
    src = os.path.join(ROOT, "tests", "cpp", "decode_spans_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu else os.path.join(ROOT, "sentencepiece_amd")
    out = os.path.join(ROOT, "tests", "cpp", "decode_spans_test" + ("_emu" if emu else ""))
    if emu:
        from tests import emulib
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu else "libspmx.so")
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "include", "spmx_processor.h")),
                 os.path.getmtime(os.path.join(ROOT, "include", "spmx.h")), os.path.getmtime(so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-L" + lib,
                               "-lspmx_emu" if emu else "-lspmx", "-Wl,-rpath," + lib])
    return out


def _facade_case(binary, model, tmp_path):
    """The driver reads `I <hex proto> <ids...>` / `P <hex proto> <hex piece>...` lines, calls DecodeIdsAsSerializedProto /
    DecodePiecesAsSerializedProto (through a base-class pointer) and Decode(..., SentencePieceText*), and compares."""
    g = golden(model)
    lines = []
    for form, tag in (("ids", "I"), ("pieces", "P")):
        for row, want in zip(g[form]["rows"], g[form]["protos"]):
            if want.startswith("sha256:"):
                continue
            cells = [str(t) for t in row] if form == "ids" else [p.encode("utf-8").hex() or "-" for p in row]
            lines.append(" ".join([tag, want or "-"] + cells))
    assert len(lines) > 50
    path = tmp_path / "rows.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([binary, os.path.join(fixtures.GOLDEN, model + ".model"), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("ok %d" % len(lines)), out.stdout[-500:]


@pytest.mark.parametrize("model", ["uni1k_bf", "uni1k_ident_dn"])
def test_emu_facade_decode_protos(model, tmp_path):
    _facade_case(_build_driver(emu=True), model, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["uni1k_bf", "uni1k_ident_dn"])
def test_gpu_facade_decode_protos(model, tmp_path):
    _facade_case(_build_driver(emu=False), model, tmp_path)


# ---- a batch larger than the grid ----
@pytest.mark.gpu
def test_gpu_decode_spans_large_batch():
    """200,000 sentences (more than n_cu * 32 wavefronts: the grid-stride loop runs): DecodeSpansDevice gives DecodeDevice's
    text, and the spans tile every sentence's text."""
    import torch
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    sp = SentencePieceProcessor(model_proto=fixtures.model_blob("uni32k"))
    n = 200_000
    text, offs = synth.mixed_corpus(n, seed=20250307)
    dev = torch.device("cuda", 0)
    d_ids, d_io, total = sp.EncodeDevice(torch.from_numpy(text).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
    d_ids = d_ids[:total].clone()
    d_text, d_to, nbytes = sp.DecodeDevice(d_ids, d_io)
    r = sp.DecodeSpansDevice(d_ids, d_io)
    assert r["total_bytes"] == nbytes and r["total_pieces"] == total and r["raw_bytes"] == nbytes
    assert torch.equal(r["text_offsets"], d_to)
    assert torch.equal(r["text"][:nbytes], d_text[:nbytes])
    assert torch.equal(r["piece_offsets"], d_io - d_io[0])
    assert torch.equal(r["piece_ids"][:total], d_ids)
    b = r["begin"][:total].cpu().numpy().view(np.uint32).astype(np.int64)
    e = r["end"][:total].cpu().numpy().view(np.uint32).astype(np.int64)
    po = r["piece_offsets"].cpu().numpy()
    to = d_to.cpu().numpy()
    lens = np.diff(po)
    assert (lens > 0).sum() > n // 2
    first, last = po[:-1][lens > 0], po[1:][lens > 0] - 1
    assert (b[first] == 0).all()                                   # begin[0] == 0
    assert (e[last] == np.diff(to)[lens > 0]).all()                # end[-1] == the sentence's bytes
    assert (np.diff(to)[lens == 0] == 0).all()
    inner = np.ones(total, dtype=bool)
    inner[first] = False
    assert (b[inner] == e[np.flatnonzero(inner) - 1]).all()        # begin[k] == end[k - 1]
    assert (e >= b).all()
    # the host form on the first 2,000 sentences
    k = 2000
    ids_h = d_ids[:int(po[k])].cpu().numpy()
    text_h, to_h, pid_h, b_h, e_h, po_h, raw_h, ro_h = sp.DecodeSpansPacked(ids_h, po[:k + 1].astype(np.uint64))
    np.testing.assert_array_equal(to_h.astype(np.int64), to[:k + 1])
    np.testing.assert_array_equal(text_h, d_text[:int(to[k])].cpu().numpy())
    np.testing.assert_array_equal(pid_h, ids_h)
    np.testing.assert_array_equal(b_h.astype(np.int64), b[:int(po[k])])
    np.testing.assert_array_equal(e_h.astype(np.int64), e[:int(po[k])])
    np.testing.assert_array_equal(po_h.astype(np.int64), po[:k + 1])
