"""Golden vectors for Decode to SentencePieceText (tests/golden/decode_protos.json): the serialized SentencePieceText the
REFERENCE produces for rows of ids and rows of piece strings (the `sentencepiece` Python module, v0.2.2, installed in the build environment --
DecodeIdsAsSerializedProto / DecodePiecesAsSerializedProto take the sentencepiece_processor.cc:766-925 path), no extra
options (the module has no SetDecodeExtraOptions; tests/test_decode_spans.py derives those cases from these rows).  Also
writes tests/golden/uni1k_ident_dn.model: uni1k_ident plus test_model's charsmap as denormalizer_spec.
Run where that module is installed; the tests only read the JSON.

The rows and the protos of a model are stored packed -- base64(lzma(json)) of {"groups": [[name, first, count], ...],
"rows": [...], "protos": [hex, ...]} for the ids form and for the pieces form -- because the rows around the 64-piece
sweep boundary are long and repetitive: 3 MB as plain hex.  The protos of the random rows (group "fuzz") do not compress;
of those the file holds "sha256:" + the digest of the serialized proto, which pins the same bytes.
tests/test_decode_spans.py unpacks and compares."""
import base64
import hashlib
import json
import lzma
import os
import sys

import sentencepiece as spm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")

from scripts.make_nbest_golden import SENTENCES  # noqa: E402

MODELS = ["test_model", "uni1k_bf", "bpe1k_bf_uds", "uni1k_suffix", "bpe1k_llama", "test_ja_model", "uni1k_ident", "uni1k_ident_dn"]
SMILE = ["<0xF0>", "<0x9F>", "<0x98>", "<0x80>"]       # U+1F600
BOUNDARY = list(range(59, 67)) + list(range(123, 131))


def make_dn_model():
    """tests/test_decode.py::_with_denormalizer("uni1k_ident", (False, False, False)), committed so that the GPU test
    needs no protobuf module."""
    from sentencepiece import sentencepiece_model_pb2 as pb
    m, src = pb.ModelProto(), pb.ModelProto()
    m.ParseFromString(open(os.path.join(G, "uni1k_ident.model"), "rb").read())
    src.ParseFromString(open(os.path.join(G, "test_model.model"), "rb").read())
    m.denormalizer_spec.precompiled_charsmap = src.normalizer_spec.precompiled_charsmap
    m.denormalizer_spec.add_dummy_prefix = False
    m.denormalizer_spec.remove_extra_whitespaces = False
    m.denormalizer_spec.escape_whitespaces = False
    with open(os.path.join(G, "uni1k_ident_dn.model"), "wb") as f:
        f.write(m.SerializeToString())


def pack(obj):
    raw = json.dumps(obj, ensure_ascii=False, separators=(",", ":")).encode("utf-8")
    return base64.b64encode(lzma.compress(raw, preset=9 | lzma.PRESET_EXTREME)).decode("ascii")


def piece_rows(sp):
    """[(group, row of piece strings)]: the shapes at which the sweep can go wrong."""
    n = sp.GetPieceSize()
    normal = [i for i in range(n) if not (sp.IsControl(i) or sp.IsUnknown(i) or sp.IsByte(i) or sp.IsUnused(i))]
    plain = [sp.IdToPiece(i) for i in normal if not sp.IdToPiece(i).startswith("▁")]
    filler = plain[0]
    ctrl = sp.IdToPiece(sp.bos_id()) if sp.bos_id() >= 0 else "<s>"
    ctrl2 = sp.IdToPiece(sp.eos_id()) if sp.eos_id() >= 0 else "</s>"
    unk = sp.IdToPiece(sp.unk_id())
    has_bytes = any(sp.IsByte(i) for i in range(min(n, 300)))
    rows = []
    for s in SENTENCES:
        rows.append(("encodings", sp.EncodeAsPieces(s)))
    if has_bytes:
        for k in BOUNDARY:       # the character the sweep defers across its 64-piece boundary, whole and truncated
            for keep in (4, 1, 2, 3):
                rows.append(("boundary", [filler] * k + SMILE[:keep]))
    cyc = [sp.IdToPiece(normal[(7 * j) % len(normal)]) for j in range(128)]
    for ln in (0, 1, 64, 65, 128):
        rows.append(("lengths", cyc[:ln]))
    rows.append(("cut", ["<0xE3>", "<0x81>", ctrl, "<0x82>"]))
    rows.append(("cut", ["<0xE3>", "<0x81>", unk, "<0x82>"]))
    rows.append(("cut", ["<0xE3>", "<0x81>", "zz", "<0x82>"]))
    rows.append(("cut", ["<0xE3>", "<0x81>", "<0x82>", ctrl, "<0xE3>", "<0x81>", "<0x82>", filler]))
    rows.append(("invalid", ["<0xFF>"]))
    rows.append(("invalid", ["<0x80>"]))
    rows.append(("invalid", ["<0xC0>", "<0x80>", "<0xED>", "<0xA0>", "<0x80>", "<0xF4>", "<0x90>", "<0x80>", "<0x80>", "<0x41>"]))
    rows.append(("whitespace", ["▁", "▁the", "▁"]))
    rows.append(("whitespace", ["▁", "▁", "▁▁a", "▁"]))
    rows.append(("whitespace", [ctrl, "▁the", "▁the"]))
    rows.append(("bytes_then_word", ["<0xFF>", "<0x80>", "▁the"]))
    rows.append(("bytes_then_word", ["<0x41>", "▁the"]))
    rows.append(("control_only", [ctrl, ctrl2, ctrl]))
    rows.append(("literals", ["zzzqqq"]))
    rows.append(("literals", ["▁notapiece"]))
    rows.append(("literals", [""]))
    rows.append(("literals", ["q" * 300]))
    rows.append(("literals", [unk]))
    rows.append(("literals", ["▁notapiece", filler, "", unk, "zzzqqq", "<0xE3>", "q" * 300, "▁the"]))
    return rows


def grouped(tagged):
    groups = []
    for i, (g, _) in enumerate(tagged):
        if groups and groups[-1][0] == g:
            groups[-1][2] += 1
        else:
            groups.append([g, i, 1])
    return groups


def main():
    make_dn_model()
    from scripts.make_fixtures import decode_fuzz_ids
    out = {"_what": "serialized SentencePieceText of Decode(ids) / Decode(pieces) per (model, row), no extra options; per model and "
                    "form base64(lzma(json {groups: [[name, first, count]], rows, protos: [hex | sha256:digest]})); made by "
                    "scripts/make_decode_proto_golden.py with sentencepiece " + spm.__version__, "models": {}}
    for model in MODELS:
        sp = spm.SentencePieceProcessor(model_file=os.path.join(G, model + ".model"))
        unk, unk_name = sp.unk_id(), sp.IdToPiece(sp.unk_id())
        pieces = piece_rows(sp)
        # the ids form of every row whose pieces are all in the vocabulary, then the fuzz rows
        ids = []
        for g, row in pieces:
            t = [sp.PieceToId(p) for p in row]
            if all(i != unk or p == unk_name for i, p in zip(t, row)):
                ids.append((g, t))
        fi, fo = decode_fuzz_ids(sp.GetPieceSize())
        for r in range(40):
            ids.append(("fuzz", [int(x) for x in fi[int(fo[r]):int(fo[r + 1])]]))
        # one call per row; an empty row goes through the batch form (the wrapper's single form takes [] for an empty batch)
        pp = [sp.DecodePiecesAsSerializedProto([row])[0].hex() for _, row in pieces]
        ip = [sp.DecodeIdsAsSerializedProto([row])[0] for _, row in ids]
        ip = ["sha256:" + hashlib.sha256(b).hexdigest() if g == "fuzz" else b.hex() for (g, _), b in zip(ids, ip)]
        out["models"][model] = {
            "pieces": pack({"groups": grouped(pieces), "rows": [r for _, r in pieces], "protos": pp}),
            "ids": pack({"groups": grouped(ids), "rows": [r for _, r in ids], "protos": ip}),
        }
        print(model, len(pieces), "piece rows", len(ids), "id rows", len(out["models"][model]["pieces"]) + len(out["models"][model]["ids"]), "bytes packed")
    path = os.path.join(G, "decode_protos.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=False, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
