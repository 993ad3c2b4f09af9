#!/usr/bin/env python3
"""Fixtures of the character and word models (model_type CHAR / WORD): tests/golden/<name>.model for the names in
MODELS, and tests/golden/charword_golden.npz / .json -- what the compiled reference (oracle/_ref/libspm_ref.so) gives
for inputs(model): ids, id offsets, Decode(ids) and, for a sample of the sentences, the serialized SentencePieceText.

    python scripts/make_charword_fixtures.py --only models   # train (needs the `sentencepiece` wheel; training only)
    python scripts/make_charword_fixtures.py --only golden   # needs oracle/_ref (the build makes it where the reference is)

tests/test_charword.py reads inputs() and the golden files; it needs neither the wheel nor oracle/_ref."""
import argparse
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")

IDENT = dict(normalization_rule_name="identity")
# name -> (corpus file, trainer arguments)
MODELS = {
    "char_ident": ("botchan.txt", dict(model_type="char", vocab_size=120, **IDENT)),
    "char_uds": ("botchan.txt", dict(model_type="char", vocab_size=120, user_defined_symbols=["<sep>", "ab"], **IDENT)),
    "char_bf": ("botchan.txt", dict(model_type="char", vocab_size=330, byte_fallback=True, character_coverage=0.98, **IDENT)),
    "char_ja": ("ja_sample.txt", dict(model_type="char", vocab_size=600, character_coverage=0.98, **IDENT)),
    "word_ident": ("botchan.txt", dict(model_type="word", vocab_size=400, **IDENT)),
    "word_nodummy": ("botchan.txt", dict(model_type="word", vocab_size=400, add_dummy_prefix=False, **IDENT)),
    "word_suffix": ("botchan.txt", dict(model_type="word", vocab_size=400, treat_whitespace_as_suffix=True, **IDENT)),
    "word_keepws": ("botchan.txt", dict(model_type="word", vocab_size=400, remove_extra_whitespaces=False, **IDENT)),
    "word_bf": ("botchan.txt", dict(model_type="word", vocab_size=660, byte_fallback=True, **IDENT)),
    "char1k": ("botchan.txt", dict(model_type="char", vocab_size=1000)),          # nmt_nfkc: the charsmap is most of the file
    "word1k": ("botchan.txt", dict(model_type="word", vocab_size=1000)),
}
# sentence lengths at which the launch sequence changes its path: the capacity of every length class (the product's table
# and the small first class the emulated tests add) and one byte more -- the last one is longer than any class, so the
# overflow list and its exact-capacity launch run too
CAPACITIES = [24, 192, 576, 1536, 4096, 16384, 65536, 1048576]
N_TAIL = 2               # the two sentences of the product's last class (1 MiB, and a byte more) close the batch: the emulated
                         # tests, whose class table ends at 64 KiB, leave them out (a lane of the CPU model takes seconds for each)
PROTO_SAMPLE = 60        # sentences (spread over the batch, none above PROTO_MAX_RAW bytes) whose SentencePieceText is stored
PROTO_MAX_RAW = 600


def make_models():
    import sentencepiece as spm
    for name, (corpus, kw) in MODELS.items():
        out = os.path.join(G, name)
        spm.SentencePieceTrainer.train(input=os.path.join(G, corpus), model_prefix=out, num_threads=4, minloglevel=2,
                                       hard_vocab_limit=False, **kw)
        os.remove(out + ".vocab")
        print("trained", name, os.path.getsize(out + ".model"), "bytes")


def _lines(name):
    with open(os.path.join(G, name), "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


@functools.lru_cache(maxsize=None)
def inputs(model):
    """One packed batch (text uint8, offsets uint64): the edge corpus; 300 lines of botchan (char_ja: all of ja_sample);
    a document of about 20 KB; a sentence at every length class's capacity and one byte beyond; an empty sentence and
    one of spaces only; three short sentences that grow elevenfold under NFKC; last, the N_TAIL sentences of the product's largest class.  The long sentences repeat an 8 KB stretch of botchan (the stored ids stay compressible)."""
    from scripts import make_fixtures as mf
    from sentencepiece_amd import synth
    bot = _lines("botchan.txt")
    sents = list(mf.edge_sentences())
    sents += _lines("ja_sample.txt") if model == "char_ja" else bot[:300]
    flat = b" ".join(bot)
    sents.append(flat[:20000])
    unit = flat[40000:48192]
    caps = [(unit * (n // len(unit) + 1))[:n] for cap in CAPACITIES for n in (cap, cap + 1)]
    # (under nmt_nfkc U+FDFA grows elevenfold: short sentences whose normalized form fits no text column of their class --
    # the overflow list, whatever the class table)
    grow = ["ﷺ".encode() * 7, "ﷺ".encode() * 60, ("ab ﷺ zz " * 40).encode()]
    sents += caps[:-N_TAIL] + [b"", b" " * 37] + grow + caps[-N_TAIL:]
    return synth.pack(sents)


def proto_sample(offs):
    """Indices of the sentences whose serialized SentencePieceText the golden holds byte for byte: a stride over the
    sentences of up to PROTO_MAX_RAW bytes.  (Of ALL sentences it holds the digest of the pieces' byte ranges.)"""
    short = [i for i in range(len(offs) - 1) if int(offs[i + 1]) - int(offs[i]) <= PROTO_MAX_RAW]
    return short[::max(1, len(short) // PROTO_SAMPLE)]


def ref_serialized(r, text, offs):
    import ctypes as C
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    cap = int(len(text)) * 120 + 64 * n + 256
    out = np.empty(cap, dtype=np.uint8)
    oo = np.zeros(n + 1, dtype=np.uint64)
    fn = r.lib.spmref_encode_serialized_batch
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    tot = fn(r.h, text.ctypes.data if len(text) else None, offs.ctypes.data, n, out.ctypes.data, cap, oo.ctypes.data)
    assert tot >= 0
    b = out[:tot].tobytes()
    return [b[int(oo[i]):int(oo[i + 1])] for i in range(n)]


def make_golden():
    from sentencepiece_amd import synth
    from tests import refshim
    ref = refshim.RefLib()
    arrays, meta = {}, {"_what": "compiled reference (oracle/_ref) on scripts/make_charword_fixtures.py inputs(model): ids as int16 "
                                 "where they fit, id offsets, sha256 of Decode(ids) text + offsets, sha256 of pieces.begin + pieces.end (uint32) of "
                                 "Encode(input, SentencePieceText*), and that message serialized for the sentences proto_sample() names"}
    for name in MODELS:
        with open(os.path.join(G, name + ".model"), "rb") as f:
            h = ref.load(f.read())
        text, offs = inputs(name)
        ids, io = h.encode_batch(text, offs, threads=8)
        dt, do = h.decode_batch(ids, io)
        arrays[name + "__ids"] = ids.astype(np.int16 if h.piece_size() < 32768 else np.int32)
        arrays[name + "__io"] = io.astype(np.uint32)
        idx = proto_sample(offs)
        tb = np.asarray(text).tobytes()
        protos = ref_serialized(h, *synth.pack([tb[int(offs[i]):int(offs[i + 1])] for i in idx]))
        sids, sb, se, sio = h.encode_spans(text, offs)
        assert np.array_equal(sids, ids) and np.array_equal(sio, io)
        arrays[name + "__protos"] = np.frombuffer(b"".join(protos), dtype=np.uint8)
        arrays[name + "__proto_offs"] = np.concatenate([[0], np.cumsum([len(p) for p in protos])]).astype(np.uint32)
        # ... and of the batch without its N_TAIL last sentences (what the emulated tests run)
        nh = len(offs) - 1 - N_TAIL
        ih, th = int(io[nh]), int(do[nh])
        head = dict(decode_bytes=th,
                    decode_sha256=hashlib.sha256(dt[:th].tobytes() + do[:nh + 1].astype("<u8").tobytes()).hexdigest(),
                    spans_sha256=hashlib.sha256(sb[:ih].astype("<u4").tobytes() + se[:ih].astype("<u4").tobytes()).hexdigest())
        meta[name] = dict(n=int(len(offs) - 1), tokens=int(len(ids)), decode_bytes=int(len(dt)), head=head,
                          spans_sha256=hashlib.sha256(sb.astype("<u4").tobytes() + se.astype("<u4").tobytes()).hexdigest(),
                          decode_sha256=hashlib.sha256(dt.tobytes() + do.astype("<u8").tobytes()).hexdigest())
        print(name, meta[name]["tokens"], "ids", len(protos), "protos")
    np.savez_compressed(os.path.join(G, "charword_golden.npz"), **arrays)
    with open(os.path.join(G, "charword_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("charword_golden.npz", os.path.getsize(os.path.join(G, "charword_golden.npz")), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["models", "golden"], default=None)
    a = ap.parse_args()
    if a.only in (None, "models"):
        make_models()
    if a.only in (None, "golden"):
        make_golden()
