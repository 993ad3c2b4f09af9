"""Known answers for the character and word models (model_type CHAR / WORD; csrc/kernels_charword.h).

The cases of the reference's own unit tests -- src/char_model_test.cc:51-107, src/word_model_test.cc:52-81 -- rebuilt as
tiny ModelProtos, and on top of them the corners of PieceToId (src/model_interface.cc:51-61: the pieces map, then the
reserved map, else unk) and of what PopulateSentencePieceText does with the cuts (src/sentencepiece_processor.cc:581-613:
a run of unknown pieces is one id; byte fallback; the extra options).  Every expected row is written down here as
piece NAMES, by hand; where the compiled reference is built it must give the same rows (that pins the transcription).
Each test runs with the device emulated and, with -m gpu, on the product library.

On the parent of the commit that added these models every test here fails at load: kUnimplemented, "only unigram and
bpe models are on the device path"."""
import numpy as np
import pytest

from sentencepiece_amd import synth
from tests import emulib, refshim

WS = "▁"
UNK, CONTROL, USER_DEFINED, UNUSED, BYTE = 2, 3, 4, 5, 6
WORD, CHAR = 3, 4
FAILS = "the reference's Encode fails this sentence"
NOT_CONSUMED = "all normalized characters are not consumed."


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return emulib.backend(request.param)


def build_model(model_type, pieces, dummy=False, rm_ws=False, byte_fallback=False):
    """pieces: [(string, type)] after <unk>, <s>, </s> (MakeBaseModelProto); identity normalizer, whitespace escaped."""
    names = ["<unk>", "<s>", "</s>"]
    out = bytearray()
    for p, t in [("<unk>", UNK), ("<s>", CONTROL), ("</s>", CONTROL)]:
        out += synth._piece_msg(p.encode(), 0.0, t)
    if byte_fallback:
        for b in range(256):
            names.append("<0x%02X>" % b)
            out += synth._piece_msg(names[-1].encode(), 0.0, BYTE)
    for k, (p, t) in enumerate(pieces):
        names.append(p)
        out += synth._piece_msg(p.encode("utf-8"), -0.1 * k, t)
    trainer = b"\x18" + synth._varint(model_type)                       # trainer_spec.model_type
    if byte_fallback:
        trainer += synth._varint(35 << 3) + b"\x01"                     # trainer_spec.byte_fallback
    out += b"\x12" + synth._varint(len(trainer)) + trainer
    norm = b"\x0a\x08identity" + b"\x18" + bytes([dummy]) + b"\x20" + bytes([rm_ws]) + b"\x28\x01"
    out += b"\x1a" + synth._varint(len(norm)) + norm
    return bytes(out), names


LONG = WS + "x" * 150                                                    # a word piece of 153 bytes
CHAR_PIECES = [(WS, 1), ("a", 1), ("b", 1), ("c", 1), ("d", 1), ("ABC", USER_DEFINED)]
WORD_PIECES = [(WS + "ab", 1), (WS + "cd", 1), (WS + "abc", 1), (WS + "a", 1), (WS + "b", 1), (WS + "c", 1), (WS + "d", 1)]

# (name, model bytes + names, encode extra options, [(input, expected piece names; "<unk>" for an unknown run)])
CASES = [
    # ---- src/char_model_test.cc:51-107 ----
    ("char_encode", build_model(CHAR, CHAR_PIECES), "", [
        ("", []),
        (WS + "a" + WS + "b" + WS + "c", [WS, "a", WS, "b", WS, "c"]),
        (WS + "ab" + WS + "cd" + WS + "abc", [WS, "a", "b", WS, "c", "d", WS, "a", "b", "c"]),
        ("あ".encode()[:1], ["<unk>"]),                                   # (the normalizer makes U+FFFD of it: one unknown character)
        (WS + "abABCcd", [WS, "a", "b", "ABC", "c", "d"]),               # "ABC" is USER_DEFINED: cut out whole
        ("a b", ["a", WS, "b"]),                                         # an escaped space is a character of its own
    ]),
    # ---- src/word_model_test.cc:52-81 ----
    ("word_encode", build_model(WORD, WORD_PIECES), "", [
        ("", []),
        (WS + "a" + WS + "b" + WS + "c", [WS + "a", WS + "b", WS + "c"]),
        (WS + "ab" + WS + "cd" + WS + "abc", [WS + "ab", WS + "cd", WS + "abc"]),
        (" ab cd", [WS + "ab", WS + "cd"]),
        ("ab cd", ["<unk>", WS + "cd"]),                                 # no dummy prefix: the first word is "ab", not a piece
    ]),
    # ---- PieceToId: the reserved map is searched too ----
    # A cut equal to a CONTROL piece's string gets that piece's id from PieceToId -- and PopulateSentencePieceText then
    # consumes no text for it (:561-567), so the reference's Encode FAILS the sentence: kInternal, "all normalized
    # characters are not consumed." (:628).  (Later releases of the reference's Python module return the bos id here; the
    # compiled reference this project is checked against, and so the product, do not.)
    ("word_bos_word", build_model(WORD, [(WS + "the", 1), (WS + "<s>", 1)]), "", [
        ("<s> the", FAILS),                                              # the word "<s>" without a dummy prefix
        ("the <s>", ["<unk>", WS + "<s>"]),                              # "▁<s>" is an ordinary piece
        ("</s>", FAILS),
        (" the", [WS + "the"]),
    ]),
    ("char_control_char", build_model(CHAR, [("a", 1), ("☃", CONTROL)]), "", [("a☃a", FAILS), ("aa", ["a", "a"])]),
    ("word_unk_string", build_model(WORD, [(WS + "the", 1), (WS + "<unk>", 1)]), "", [
        ("<unk> the", ["<unk>", WS + "the"]),                            # a word equal to the unk piece's string: unk_id
        ("<unk> zz the", ["<unk>", WS + "the"]),                         # ... and it merges with the unknown word behind it
        (" the <unk>", [WS + "the", WS + "<unk>"]),
    ]),
    ("char_unk_string", build_model(CHAR, [("a", 1), ("<", 1), (">", 1)]), "", [
        ("<unk>", ["<", "<unk>", ">"]),                                  # characters: u, n, k are unknown, one run
    ]),
    ("word_byte_piece_word", build_model(WORD, [(WS + "the", 1)], byte_fallback=True), "", [
        ("<0x41> the", ["<0x41>", WS + "the"]),                          # the word "<0x41>" finds the BYTE piece
        ("A the", ["<0x41>", WS + "the"]),                               # ... as the unknown word "A" does by byte fallback
        (" the Zé", [WS + "the", "<0xE2>", "<0x96>", "<0x81>", "<0x5A>", "<0xC3>", "<0xA9>"]),
    ]),
    ("char_byte_fallback", build_model(CHAR, [("a", 1), (WS, 1)], byte_fallback=True), "", [
        ("a é", ["a", WS, "<0xC3>", "<0xA9>"]),
        ("中a", ["<0xE4>", "<0xB8>", "<0xAD>", "a"]),
    ]),
    ("word_unused_found", build_model(WORD, [(WS + "the", UNUSED), (WS + "cat", 1)]), "", [
        (" the cat", [WS + "the", WS + "cat"]),                          # an UNUSED piece is found like any other
    ]),
    ("char_unused_found", build_model(CHAR, [("a", UNUSED), ("b", 1)]), "", [("ab", ["a", "b"])]),
    # ---- user-defined pieces ----
    ("word_uds_not_cut", build_model(WORD, [(WS + "the", 1), ("<sep>", USER_DEFINED), (WS + "a<sep>b", 1)]), "", [
        (" the a<sep>b", [WS + "the", WS + "a<sep>b"]),                  # inside a word it is part of the word
        (" the<sep> the", ["<unk>", WS + "the"]),
        ("<sep>", ["<sep>"]),                                            # the whole word IS the piece: PieceToId finds it
    ]),
    ("char_uds_longest", build_model(CHAR, [("a", 1), ("b", 1), ("c", 1), ("ab", USER_DEFINED), ("abc", USER_DEFINED),
                                            ("<sep>", USER_DEFINED), ("bcx", USER_DEFINED)]), "", [
        ("abcab", ["abc", "ab"]),                                        # longest match first
        ("abx", ["ab", "<unk>"]),
        ("a<sep>bcb", ["a", "<sep>", "b", "c", "b"]),                    # "bc" + not-x: the walk went on and found nothing
        ("<sepab", ["<unk>", "ab"]),                                     # "<sep" is four unknown characters, one run
        ("bcx", ["bcx"]),
    ]),
    # ---- runs of unknowns ----
    ("word_unknown_runs", build_model(WORD, [(WS + "cat", 1), (WS + "q", 1)], dummy=True, rm_ws=True), "", [
        ("cat <sep>abc Zé中文 q", [WS + "cat", "<unk>", WS + "q"]),        # across words: one id
        ("zz", ["<unk>"]),
        ("q zz zz", [WS + "q", "<unk>"]),
        ("  ", []),                                                      # nothing but spaces: no ids
    ]),
    ("char_unknown_runs", build_model(CHAR, [("a", 1)]), "", [("xyaz中a", ["<unk>", "a", "<unk>", "a"]), ("xyz", ["<unk>"])]),
    # ---- whitespace the normalizer leaves ----
    ("word_keep_whitespace", build_model(WORD, [(WS + "the", 1), (WS, 1), (WS + "cat", 1)], dummy=True), "", [
        ("the   cat", [WS + "the", WS, WS, WS + "cat"]),                 # every space symbol of a run starts a word
        ("the cat ", [WS + "the", WS + "cat", WS]),
    ]),
    # ---- a piece longer than the unigram path's 120 bytes ----
    ("word_long_piece", build_model(WORD, [(LONG, 1), (WS + "a", 1)]), "", [
        (" " + "x" * 150 + " a", [LONG, WS + "a"]),
        (" " + "x" * 149 + " a", ["<unk>", WS + "a"]),
        (" " + "x" * 151, ["<unk>"]),
    ]),
    # ---- more cuts than a wavefront has lanes, cuts longer than a sweep of 64 bytes (the wave-cooperative form's rounds) ----
    ("char_runs_across_rounds", build_model(CHAR, [("a", 1), (WS, 1)]), "", [
        ("x" * 200, ["<unk>"]),                                          # one run over four rounds of cuts: one id
        ("a" + "x" * 63 + "y" * 64 + "a", ["a", "<unk>", "a"]),          # the run begins in one round and ends in the third
        ("a" * 64 + "x", ["a"] * 64 + ["<unk>"]),
        ("a" * 63 + "xx" + "a", ["a"] * 63 + ["<unk>", "a"]),            # ... across the boundary between two rounds
        ("中" * 70 + "a", ["<unk>", "a"]),
    ]),
    ("char_bf_across_rounds", build_model(CHAR, [("a", 1)], byte_fallback=True), "", [
        ("a" * 62 + "中中" + "a", ["a"] * 62 + ["<0xE4>", "<0xB8>", "<0xAD>"] * 2 + ["a"]),
    ]),
    ("word_across_rounds", build_model(WORD, [(WS + "a", 1), (LONG, 1), (WS + "y" * 64, 1)], dummy=True, rm_ws=True), "", [
        (" ".join(["zz"] * 70 + ["a"]), ["<unk>", WS + "a"]),            # seventy unknown words: one id
        (" ".join(["a"] * 64 + ["zz", "zz", "a"]), [WS + "a"] * 64 + ["<unk>", WS + "a"]),
        ("a " + "x" * 150 + " a", [WS + "a", LONG, WS + "a"]),           # a word of three sweeps, carried over
        ("x" * 300 + " a " + "y" * 64, ["<unk>", WS + "a", WS + "y" * 64]),
        ("a " + "x" * 1000, [WS + "a", "<unk>"]),                        # the text ends inside a carried-over word
    ]),
    ("word_bf_across_rounds", build_model(WORD, [(WS + "a", 1)], dummy=True, rm_ws=True, byte_fallback=True), "", [
        ("a " + "q" * 70 + " a", [WS + "a", "<0xE2>", "<0x96>", "<0x81>"] + ["<0x71>"] * 70 + [WS + "a"]),
    ]),
    # ---- the extra options, in several orders ----
    ("word_bos_eos", build_model(WORD, WORD_PIECES), "bos:eos", [(" ab zz cd", ["<s>", WS + "ab", "<unk>", WS + "cd", "</s>"]), ("", ["<s>", "</s>"])]),
    ("word_eos_reverse_bos", build_model(WORD, WORD_PIECES), "eos:reverse:bos", [(" ab zz cd", ["<s>", "</s>", WS + "cd", "<unk>", WS + "ab"])]),
    ("char_reverse_unk", build_model(CHAR, CHAR_PIECES), "reverse:unk", [(WS + "axyABC", ["ABC", "<unk>", "a", WS])]),
    ("char_bos_eos_reverse_unk", build_model(CHAR, CHAR_PIECES), "bos:eos:reverse:unk", [("abcd", ["</s>", "d", "c", "b", "a", "<s>"])]),
    ("char_reverse_many", build_model(CHAR, CHAR_PIECES), "reverse", [("abcdabcda", list("adcbadcba"))]),    # (more than two stores of four)
]


def as_bytes(k):
    return k if isinstance(k, bytes) else k.encode("utf-8")


# form: "lane" -- the class table's own routing (these short sentences take the lane-per-sentence form,
# csrc/kernels_charword.h); "wave" -- every class goes to the wave-cooperative form (csrc/kernels_charwave.h: a lane per
# cut, ids placed by a prefix sum), which a character model with USER_DEFINED pieces does not have (it stays as it is)
@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kats(case, form, backend):
    import ctypes as C
    name, (blob, names), opts, kats = case
    want = [None if exp is FAILS else [names.index(p) for p in exp] for _, exp in kats]
    if refshim.available():                              # the table itself, sentence by sentence
        r = refshim.RefLib().load(blob)
        r.set_encode_extra_options(opts)
        for (s, _), row in zip(kats, want):
            if row is None:
                with pytest.raises(RuntimeError):
                    r.encode(as_bytes(s))
                assert r.lib.spmref_last_error(r.h).decode().startswith("Internal:")
                assert r.lib.spmref_last_error(r.h).decode().endswith(NOT_CONSUMED)
            else:
                assert r.encode(as_bytes(s)).tolist() == row, (name, s, "the table itself is wrong")
    h = backend.load(blob, env={"SPMX_UNI_WAVE_MAX": "1000000"} if form == "wave" else None)
    h.set_encode_extra_options(opts)
    text, offs = synth.pack([as_bytes(k) for k, _ in kats])
    ids, io = h.encode_batch(text, offs)
    if form == "wave" and any(len(as_bytes(k)) for k, _ in kats):
        has_uds = h.sp.model_type() == CHAR and (h.flags() & 0x80) != 0          # (csrc/dev.h kNfHasUserDefined)
        assert ("CharWordWaveKernel" in [c["kernel"] for c in h.sp.LastProfile()["classes"]]) == (not has_uds)
    io = io.astype(np.int64)
    assert [ids[io[i]:io[i + 1]].tolist() for i in range(len(kats))] == [row or [] for row in want]
    assert h.sent_status.tolist() == [13 if row is None else 0 for row in want]
    assert h.status == sum(row is None for row in want)
    # one sentence at a time through spmx_encode: the same rows, the reference's Status for a sentence it fails
    out = np.zeros(512, dtype=np.int32)
    for (s, _), row in zip(kats, want):
        n_ids, b = C.c_uint64(0), as_bytes(s)
        rc = h.lib.spmx_encode(h.sp._h, b, len(b), out.ctypes.data, len(out), C.byref(n_ids))
        if row is None:
            assert rc == 13 and h.lib.spmx_last_error(None).decode() == NOT_CONSUMED
        else:
            assert rc == 0 and out[:n_ids.value].tolist() == row, (name, s)


def test_model_type_and_scores(backend):
    for mt, pieces in ((WORD, WORD_PIECES), (CHAR, CHAR_PIECES)):
        blob, names = build_model(mt, pieces)
        h = backend.load(blob)
        assert h.sp.model_type() == mt
        assert h.sp.GetPieceSize() == len(names)
        for i in range(3, len(names)):
            assert h.sp.IdToPiece(i) == names[i] and h.sp.PieceToId(names[i]) == i
            assert h.sp.GetScore(i) == pytest.approx(-0.1 * (i - 3), abs=1e-7)
