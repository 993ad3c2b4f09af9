"""Every key of every built-in rule set's charsmap through the normalizer's device forms.

The kernels decide from tables derived in csrc/tables.cc (ascii_safe, the two-byte prefix bitmap, the code-point bitmaps,
the one-character rule table) that they need not look at the charsmap at all; one wrong bit there changes the ids of
exactly the sentences that hold one code point or one two-character key.  So the inputs here are built from the keys
themselves (tests/charsmapkeys.py reads them from the ModelProto, independently of the product and of the oracle;
tests/sweepcorpus.py puts each into nine sentence contexts, into documents at every phase of the 64-byte sweeps, and adds
every code point and every two-byte pair), for models of all four rule sets: nmt_nfkc, nfkc, nmt_nfkc_cf, nfkc_cf.

Legs: the helper against the oracle; the oracle against the compiled reference (where it is built); the emulator against
the oracle (CPU); the device against the oracle (-m gpu), whole corpus, four calls, four forms.

What the emulator leg runs, and what it leaves to the GPU leg.  Measured under the emulator: encode of the 2 M key
sentences of a model 3.6 s, of its 10 MB of documents 53 s (the long form, 5 us a byte), of the code point corpus 14 s;
the wave-cooperative form (SPMX_UNI_WAVE_MAX) 420 us a sentence (128 s for the thinned keys' 304 k sentences);
normalize_batch 340 us and encode_spans 170 us a sentence (wave-per-sentence kernels, 64 emulated lanes).  Per model:
  * `{}`, small class table (the deep case): encode_batch over the WHOLE corpus -- every key sentence, every document
    (so every phase 0..63 for every separator), the text above 256 KB in a call of its own (the two-wavefront form), every
    code point sentence -- and normalize_batch / encode_spans over every thinned key (sweepcorpus.thin: the keys that are
    not Hangul compositions plus every 16th Hangul one, 34 k of 226 k) in one of the nine contexts each, in turn, plus one
    document per separator and every 64th code point sentence;
  * `{}` with the default class table and SPMX_NO_WORD_KERNEL=1 with both: encode_batch over every key sentence, every
    code point alone, every two-byte pair, every 32nd document and every 64th packed code point sentence;
  * SPMX_CHAR_NORM_ALWAYS, SPMX_NO_CHAR_NORM, SPMX_NO_FAST, SPMX_NO_LANE_GENERAL (alone, and with the word kernels off, where
    it acts on every model: see EMU_SETTINGS): encode_batch over all nine contexts of
    every thinned key (304 k sentences), every 64th document, every 64th code point sentence;
  * SPMX_UNI_WAVE_MAX raised: every 64th thinned key (at 420 us a sentence the thinned list would take two minutes a case);
  * normalize_batch and encode_spans outside the deep case: every 300th thinned key in all nine contexts, one document,
    every 512th code point sentence.
bpe1k_noesc (split_by_whitespace off: a sentence per wavefront, 47 us a sentence emulated, 97 s for its key sentences)
runs every key sentence in its deep case only; elsewhere every 16th thinned key where the others run all of them (the lane
switches do not reach its kernel), and every 16th key where they run all keys.  Each case starts its strides at an offset of its own.  SPMX_SWEEP_FULL=1 in the
environment runs every case over everything; that has never been run to its end (hours).  The GPU leg thins nothing.

What it costs: the CPU cases of this file (160: the helper, the oracle against the reference, the emulator leg) took
27 minutes of wall time in one process on an 8-core machine, 43 minutes of CPU time; nine tenths of it are the deep
cases, 1.5 minutes a model and 3.6 for bpe1k_noesc.  The 80 GPU cases take two to five seconds each.

No counter tells char_norm_stream's tiles from fast_norm_stream's, so SPMX_CHAR_NORM_ALWAYS / SPMX_NO_CHAR_NORM have no
path assertion: that they reach the kernel is pinned only by api.cc passing the mode on (a.no_char_norm)."""
import functools
import os

import numpy as np
import pytest

from tests import charsmapkeys, fixtures, refshim, sweepcorpus
from tests.emulib import SMALL_CLASSES

RULESETS = {"nmt_nfkc": "uni1k", "nfkc": "uni1k_nfkc", "nmt_nfkc_cf": "uni1k_cf", "nfkc_cf": "uni1k_nfkc_cf"}
KEY_COUNTS = {"nmt_nfkc": 225275, "nfkc": 225232, "nmt_nfkc_cf": 226683, "nfkc_cf": 226640}
NEW_MODELS = ["uni1k_nfkc", "uni1k_cf", "bpe1k_cf", "uni1k_nfkc_cf"]
EMU_MODELS = NEW_MODELS + ["test_model", "uni1k_uds", "uni1k_suffix", "bpe1k_noesc", "test_ja_model"]
GPU_MODELS = NEW_MODELS + ["test_model", "uni1k_uds", "bpe1k_noesc", "uni32k", "bpe1k_llama"]
CHARWORD_MODELS = ["char1k", "word1k"]
WAVE_PER_SENTENCE = ["bpe1k_noesc"]     # (see the module docstring: thinned under the emulator in every setting)
SWEEP_FULL = os.environ.get("SPMX_SWEEP_FULL") == "1"


@functools.lru_cache(maxsize=1)
def model_keys(model):
    """The model's own rule keys; for a model without a charsmap (identity) those of nmt_nfkc_cf, the largest set."""
    keys, _ = charsmapkeys.model_rules(fixtures.model_blob(model))
    if not keys:
        keys, _ = charsmapkeys.model_rules(fixtures.model_blob("uni1k_cf"))
    return keys


@functools.lru_cache(maxsize=1)
def thin_keys(model):
    return sweepcorpus.thin(model_keys(model))


@functools.lru_cache(maxsize=1)
def full_parts(model):
    """The whole corpus of a model: [(name, part)]."""
    keys = model_keys(model)
    return [("sentences", sweepcorpus.Sentences(keys)), ("documents", sweepcorpus.Documents(keys)),
            ("code points", sweepcorpus.code_points())]


def is_whole(model, name, part):
    return any(n == name and p is part for n, p in full_parts(model))


class _Pick:
    """Chosen sentences of a corpus part; describes them as the part does."""

    def __init__(self, part, pick):
        from sentencepiece_amd import synth
        self.part, self.pick = part, np.asarray(pick, dtype=np.int64)
        self.text, self.offs = synth.gather_packed(part.text, part.offs, self.pick)

    def describe(self, i):
        return self.part.describe(int(self.pick[i]))


BIG = "text above 256 KB"


def emu_parts(model, setting, classes, case):
    """-> (parts for encode_batch, parts for normalize_batch / encode_spans) of one emulator case: the module docstring
    says what is taken; `case` (the case's number within its model) moves the start of every stride."""
    sents, docs, cp = (p for _, p in full_parts(model))
    nd, ncp, npk = len(docs.offs) - 2, len(cp.offs) - 1, cp.n_packed          # (nd: without the text above 256 KB)
    kt = thin_keys(model)
    slow = model in WAVE_PER_SENTENCE
    deep = setting == "default" and classes == "small"
    sparse_norm = [("sentences", sweepcorpus.Sentences(kt[case * 7 % 300::300])), ("documents", _Pick(docs, [case * 5 % nd])),
                   ("code points", _Pick(cp, np.arange(case * 37 % 512, ncp, 512)))]
    if deep or SWEEP_FULL:
        enc = [("sentences", sents), ("documents", _Pick(docs, np.arange(nd))), (BIG, _Pick(docs, [nd])), ("code points", cp)]
        if SWEEP_FULL:
            return enc, enc
        per_sep = nd // len(sweepcorpus.SEPARATORS)
        return enc, [("sentences", sweepcorpus.Sentences(kt, one_context=True)),
                     ("documents", _Pick(docs, [i * per_sep + (case + 3 * i) % per_sep for i in range(len(sweepcorpus.SEPARATORS))])),
                     ("code points", _Pick(cp, np.arange(case % 64, ncp, 64)))]
    if setting in EXHAUSTIVE:
        enc = [("sentences", sweepcorpus.Sentences(model_keys(model)[case % 16::16]) if slow else sents),
               ("documents", _Pick(docs, np.arange(case % 32, nd, 32))),
               ("code points", _Pick(cp, np.arange(case % 64, ncp, 64) if slow else
                                     np.concatenate([np.arange(case % 64, npk, 64), np.arange(npk, ncp)])))]
    else:
        step = 64 if setting == "uni_wave" else 16 if slow else 1
        enc = [("sentences", sweepcorpus.Sentences(kt[case % step::step])), ("documents", _Pick(docs, np.arange(case % 64, nd, 64))),
               ("code points", _Pick(cp, np.arange(case % 64, ncp, 64)))]
    return enc, sparse_norm


class _Want:
    """The oracle's results for one model; those on a whole corpus part (`keep`: the part's name) are kept for the model's
    other cases, the rest are computed each time."""

    def __init__(self, oracle, model):
        self.o = oracle.load(fixtures.model_blob(model))
        self.memo = {}

    def __call__(self, call, part, keep=None):
        if keep is not None and (call, keep) in self.memo:
            return self.memo[call, keep]
        if call == "decode":
            got = self.o.decode_batch(*self("encode", part, keep))
        else:
            fn = {"encode": self.o.encode_batch, "normalize": self.o.normalize_batch, "spans": self.o.encode_spans}[call]
            got = fn(part.text, part.offs)
        if keep is not None:
            self.memo[call, keep] = got
        return got


_want_cache = {}


def want(oracle, model):
    if model not in _want_cache:
        _want_cache.clear()                          # one model's results at a time
        _want_cache[model] = _Want(oracle, model)
    return _want_cache[model]


def normalizer_spec(model):
    return [v for f, wt, v in charsmapkeys._fields(fixtures.model_blob(model)) if f == 3 and wt == 2]


WS = "\u2581".encode()


def charword_vocab(model):
    """(model_type, {piece bytes: id}, unk id) of a fixture model, from its serialized proto: ModelProto.pieces (1) with
    piece (1) and type (3; 2 is UNKNOWN), trainer_spec (2) with model_type (3; 3 WORD, 4 CHAR)."""
    vocab, unk, model_type = {}, -1, None
    for f, wt, v in charsmapkeys._fields(fixtures.model_blob(model)):
        if f == 1 and wt == 2:
            d = {g: x for g, _, x in charsmapkeys._fields(v)}
            if d.get(3, 1) == 2:
                unk = len(vocab)
            vocab.setdefault(bytes(d[1]), len(vocab))
        elif f == 2 and wt == 2:
            t = {g: x for g, _, x in charsmapkeys._fields(v)}
            model_type = t.get(3, 1)
            # (the cuts below are the plain ones: whitespace in front of a word, no whitespace-only pieces)
            assert not t.get(24, 0) and not t.get(26, 0)
    assert unk >= 0 and model_type in (3, 4)
    return model_type, vocab, unk


def charword_ids(model, norm, norm_offs):
    """Encode of a character or word model restated over normalized text (the oracle's, which restates neither model type):
    a character model's pieces are the characters, a word model's the stretches that begin at the sentence's start and at
    every U+2581; a piece's id is its vocabulary entry or the unknown id, and a run of unknown pieces counts once.
    -> (ids int32, id offsets uint64)"""
    model_type, vocab, unk = charword_vocab(model)
    norm = np.asarray(norm, dtype=np.uint8)
    no = np.asarray(norm_offs).astype(np.int64)
    if model_type == 4:
        starts = np.flatnonzero((norm & 0xC0) != 0x80)          # (normalized text is well-formed UTF-8)
    else:
        sym = np.flatnonzero((norm[:-2] == WS[0]) & (norm[1:-1] == WS[1]) & (norm[2:] == WS[2])) if len(norm) > 2 else no[:0]
        starts = np.union1d(sym, no[:-1][no[1:] > no[:-1]])
    # a piece ends where the next begins or where its sentence ends
    sent = np.searchsorted(no, starts, side="right") - 1
    ends = np.minimum(np.append(starts[1:], len(norm)), no[sent + 1])
    nb = norm.tobytes()
    get = vocab.get
    ids = np.fromiter((get(nb[a:b], unk) for a, b in zip(starts.tolist(), ends.tolist())), dtype=np.int32, count=len(starts))
    # the processor merges a run of unknown pieces within a sentence into one (PopulateSentencePieceText)
    keep = np.ones(len(ids), dtype=bool)
    keep[1:] = ~((ids[1:] == unk) & (ids[:-1] == unk) & (sent[1:] == sent[:-1]))
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    return ids[keep], kept_before[np.searchsorted(starts, no, side="left")].astype(np.uint64)


class _CharWordWant:
    """The oracle restates unigram and BPE models only.  For char1k and word1k it gives the normalized text (through uni1k,
    whose normalizer_spec is byte for byte theirs), charword_ids cuts that text into the expected ids, and where the
    compiled reference is built its ids are compared as well."""

    def __init__(self, oracle, model):
        assert normalizer_spec(model) == normalizer_spec("uni1k")
        self.model = model
        self.norm = _Want(oracle, "uni1k")
        self.ref = refshim.RefLib().load(fixtures.model_blob(model)) if refshim.available() else None
        self.memo = {}

    def normalize(self, part, keep=None):
        return self.norm("normalize", part, keep)

    def encode(self, part, keep=None):
        """-> (ids, id offsets) by charword_ids; checked against the compiled reference where there is one."""
        if keep is not None and keep in self.memo:
            return self.memo[keep]
        text, offs, _ = self.normalize(part, keep)
        got = charword_ids(self.model, text, offs)
        if self.ref is not None:
            assert_same("%s: the restated cuts against the compiled reference" % self.model, part, "encode",
                        self.ref.encode_batch(part.text, part.offs, threads=8), got)
        if keep is not None:
            self.memo[keep] = got
        return got


def charword_want(oracle, model):
    if ("cw", model) not in _want_cache:
        _want_cache.clear()
        _want_cache["cw", model] = _CharWordWant(oracle, model)
    return _want_cache["cw", model]


def check_charword(tag, sp, part, w, keep=None):
    """Char and word models: Normalize with offsets against the oracle, ids against the cuts restated over its text."""
    assert_same(tag, part, "normalize", sp.NormalizePacked(part.text, part.offs, with_offsets=True), w.normalize(part, keep))
    ids, io, st, failed = sp.EncodePackedEx(part.text, part.offs)
    assert failed == 0 and not np.asarray(st).any()
    assert_same(tag, part, "encode", (ids, io), w.encode(part, keep))


def assert_same(tag, part, call, got, wanted):
    """Array for array; the message names the first differing sentence's bytes and the key it was built from."""
    fd = sweepcorpus.first_difference
    if call == "encode" or call == "decode":
        (g, go), (w, wo) = got, wanted
        bad = [fd(g, w, go, wo)]
    elif call == "spans":
        g, gb, ge, go = got[:4]
        w, wb, we, wo = wanted
        bad = [fd(g, w, go, wo), fd(gb, wb, go, wo), fd(ge, we, go, wo)]
    else:                       # normalize: text, offsets, norm_to_orig (one entry per byte + one closing each sentence)
        (g, go, gn), (w, wo, wn) = got, wanted
        k = np.arange(len(wo), dtype=np.int64)
        bad = [fd(g, w, go, wo), fd(gn, wn, np.asarray(go).astype(np.int64) + k, np.asarray(wo).astype(np.int64) + k)]
    bad = [x for x in bad if x is not None]
    if bad:
        pytest.fail("%s, %s differs from the oracle first at %s" % (tag, call, part.describe(min(bad))), pytrace=False)


# ------------------------------------------------------------------------------------------------ the key helper (CPU)

@pytest.mark.parametrize("rule", sorted(RULESETS))
def test_key_helper_counts_and_replacements(rule, oracle):
    """The four key counts, and for every key: the oracle's Normalize(key), dummy prefix off (set in the serialized proto
    by charsmapkeys.with_normalizer_flag: no protobuf classes needed), is the replacement with its spaces escaped.  Left out: the keys whose replacement is, begins or ends with a space
    (remove_extra_whitespaces eats those): at most 81."""
    blob = fixtures.model_blob(RULESETS[rule])
    keys, repls = charsmapkeys.model_rules(blob)
    assert len(keys) == KEY_COUNTS[rule] == len(set(keys))
    assert max(map(len, keys)) <= 12 and max(len(k.decode("utf-8")) for k in keys) <= 4
    empty = sum(r == b"" for r in repls)
    if rule == "nmt_nfkc":
        assert sum(k[0] < 0x80 for k in keys) == 621 and sum(b" " in r for r in repls) == 81
        assert empty == 30 and sum(ord(k.decode("utf-8")[0]) >= 0x20000 for k in keys) == 542
        assert max(map(len, repls)) == 33
    # only the nmt_ rules delete characters (30 of them, with or without case folding); nfkc and nfkc_cf replace by nothing never
    assert empty == (30 if rule.startswith("nmt_") else 0)
    ws = "▁".encode()
    skipped, parts, expect = 0, [], []
    for k, r in zip(keys, repls):
        if r[:1] == b" " or r[-1:] == b" ":
            skipped += 1
            continue
        parts.append(k)
        expect.append(r.replace(b" ", ws))
    assert skipped <= 81
    text, offs = sweepcorpus.pack(parts)
    o = oracle.load(charsmapkeys.with_normalizer_flag(blob, 3, False))         # (3: add_dummy_prefix)
    assert o.normalize(b"a") == b"a" and oracle.load(blob).normalize(b"a") == ws + b"a"
    got, go, _ = o.normalize_batch(text, offs)
    wt, wo = sweepcorpus.pack(expect)
    bad = sweepcorpus.first_difference(got, wt, go, wo)
    assert bad is None, "key %r: oracle %r, charsmap %r" % (parts[bad], got[int(go[bad]):int(go[bad + 1])].tobytes(),
                                                            expect[bad])


# ----------------------------------------------------------------------------- the oracle against the reference (CPU)

@pytest.mark.parametrize("rule", sorted(RULESETS))
def test_oracle_matches_reference_on_the_sweep(rule, oracle):
    """Encode ids and Normalize with offsets over the whole sweep corpus: pins the oracle on the keys themselves."""
    if not refshim.available():
        pytest.skip("the compiled reference is not built here")
    model = RULESETS[rule]
    r = refshim.RefLib().load(fixtures.model_blob(model))
    w = want(oracle, model)
    for name, part in full_parts(model):
        got = r.encode_batch(part.text, part.offs, threads=8)
        assert_same("%s %s: reference" % (model, name), part, "encode", got, w("encode", part, name))
        got = r.normalize_batch(part.text, part.offs)
        assert_same("%s %s: reference" % (model, name), part, "normalize", got, w("normalize", part, name))


# --------------------------------------------------------------------------------------------------- the emulator (CPU)

NOWORD = {"SPMX_NO_WORD_KERNEL": "1"}
EMU_SETTINGS = {
    "default": {},
    "noword": NOWORD,
    "charnorm_always": dict(NOWORD, SPMX_CHAR_NORM_ALWAYS="1"),
    "no_charnorm": dict(NOWORD, SPMX_NO_CHAR_NORM="1"),
    "no_fast": {"SPMX_NO_FAST": "1"},
    "no_lane_general": {"SPMX_NO_LANE_GENERAL": "1"},
    # (where the word form takes the key sentences -- the rule sets without case folding -- the switch above has nothing to
    # set aside; with the word kernels off it acts on every model that has fast forms)
    "no_lane_general_noword": dict(NOWORD, SPMX_NO_LANE_GENERAL="1"),
    "uni_wave": dict(NOWORD, SPMX_UNI_WAVE_MAX="1000000"),       # the wave-cooperative form takes the staged classes
}
EXHAUSTIVE = ("default", "noword")
# StreamFastEligible (kernels_normlane.h): user-defined symbols, or a dummy prefix that is a suffix, leave norm_lane_any alone
NO_FAST_FORMS = ("uni1k_uds", "uni1k_suffix")
# ... and BPE without whitespace splitting is not word-wise: a sentence per wavefront (EncodeKernel, normalize_wave), no lane
# tiles, no backlog, and the lane switches do not reach it
NO_LANE_TILES = tuple(WAVE_PER_SENTENCE)
# rule sets without case folding: with the word kernels on, the word form takes the key sentences before any tile could set
# them aside (measured: backlog 0); the case-folding models must show a backlog under SPMX_NO_LANE_GENERAL alone too
WORD_FORM_TAKES_KEYS = ("uni1k_nfkc", "test_model")


def _emu_cases():
    for model in EMU_MODELS + CHARWORD_MODELS:
        case = 0
        for setting in EMU_SETTINGS:
            if model in CHARWORD_MODELS and setting not in EXHAUSTIVE:
                continue                  # (kernels_charword.h has one normalizer: the lane switches do not reach it)
            for classes in ("small", "default"):
                yield pytest.param(model, setting, classes, case, id="%s-%s-%s" % (model, setting, classes))
                case += 1


def long_kernel(h):
    """Name of the kernel the last encode's long form ran (LastProfile's slot 4), "" where it did not run."""
    return h.sp.LastProfile()["classes"][4]["kernel"]


def _check_path(model, setting, name, h, n):
    """The form a setting is meant to force took the sentences: a silent fallback would sweep the wrong kernel.  (The module
    docstring says why SPMX_CHAR_NORM_ALWAYS / SPMX_NO_CHAR_NORM have no assertion here.)"""
    p = h.path()
    taken = [c["sentences"] for c in h.sp.LastProfile()["classes"]]
    bpe = model.startswith("bpe")
    assert p["failed"] == 0
    if setting == "no_fast" and name in ("sentences", "code points"):
        assert p["backlog"] == 0, "SPMX_NO_FAST: every lane runs norm_lane_any, none waits in a backlog"
    if model in NO_FAST_FORMS + NO_LANE_TILES and name in ("sentences", "code points"):
        assert p["backlog"] == 0, "no fast form for this model: nothing is ever set aside, in any setting"
    if "SPMX_NO_WORD_KERNEL" in EMU_SETTINGS[setting]:
        assert sum(taken[5:7]) == 0, "SPMX_NO_WORD_KERNEL: no sentence may take the word form"
    if name in ("documents", BIG):
        # few long texts (up to four a CU; emulib loads with 2 CUs): a workgroup of two wavefronts each, HBM normalize;
        # many: a wavefront each.  (BPE has the one long form; it reports its launch and its kernel, not a sentence count.)
        few = n <= 4 * 2
        assert name != BIG or few
        if not (bpe and name == BIG):      # (a word-wise BPE model takes a text of short words through its streaming kernel)
            assert p["long_launches"] > 0
            assert long_kernel(h) == ("BpeLongKernel" if bpe else "UniLongPipeKernel" if few else "UniLongKernel")
    if setting == "uni_wave" and name == "sentences" and not bpe:
        assert taken[4] > 0, "SPMX_UNI_WAVE_MAX: the wave-cooperative form must take staged sentences"


@pytest.mark.parametrize("model,setting,classes,case", list(_emu_cases()))
def test_emu_sweep(model, setting, classes, case, oracle):
    from tests import emulib
    enc, norm = emu_parts(model, setting, classes, case)
    h = emulib.EmuLib().load(fixtures.model_blob(model), env=dict(EMU_SETTINGS[setting]),
                             classes=SMALL_CLASSES if classes == "small" else "")
    tag = "%s %s %s classes" % (model, setting, classes)
    if model in CHARWORD_MODELS:
        w = charword_want(oracle, model)
        name, part = enc[0]
        ids, io = h.encode_batch(part.text, part.offs)
        assert h.status == 0 and not np.asarray(h.sent_status).any()
        assert_same(tag, part, "encode", (ids, io), w.encode(part, name if is_whole(model, name, part) else None))
        check_charword(tag, h.sp, norm[0][1], w)
        return
    w = want(oracle, model)
    if setting.startswith("no_lane_general") and model not in NO_FAST_FORMS + NO_LANE_TILES:
        # (the profile counts a call's last chunk of sentences, so the switch is pinned on a call of one chunk)
        probe = sweepcorpus.Sentences(thin_keys(model)[case % 16::16])
        h.encode_batch(probe.text, probe.offs)
        word_form = sum(c["sentences"] for c in h.sp.LastProfile()["classes"][5:7])
        assert h.path()["backlog"] > 0 or (setting == "no_lane_general" and model in WORD_FORM_TAKES_KEYS and word_form > 0), \
            "SPMX_NO_LANE_GENERAL: what the fast forms give up must wait in the backlog"
    for name, part in enc:
        got = h.encode_batch(part.text, part.offs)
        assert h.status == 0 and not np.asarray(h.sent_status).any()
        _check_path(model, setting, name, h, len(part.offs) - 1)
        assert_same("%s, %s" % (tag, name), part, "encode", got, w("encode", part, name if is_whole(model, name, part) else None))
    for name, part in norm:
        assert_same("%s, %s" % (tag, name), part, "normalize", h.normalize_batch(part.text, part.offs), w("normalize", part))
        assert_same("%s, %s" % (tag, name), part, "spans", h.encode_spans(part.text, part.offs), w("spans", part))


# ---------------------------------------------------------------------------------------------------------- the device

GPU_FORMS = {"default": {}, "noword": {"SPMX_NO_WORD_KERNEL": "1"}, "charnorm_always": {"SPMX_CHAR_NORM_ALWAYS": "1"},
             "small_classes": {"SPMX_CLASSES": SMALL_CLASSES}}
# ... and the lane normalizers forced one by one, as under the emulator (unigram and BPE models; milliseconds on the device)
GPU_LANE_FORMS = {k: EMU_SETTINGS[k] for k in ("charnorm_always", "no_charnorm", "no_fast", "no_lane_general")}


def _gpu_cases():
    for m in GPU_MODELS + CHARWORD_MODELS:
        for f in GPU_FORMS:
            yield pytest.param(m, f, id="%s-%s" % (m, f))
        if m not in CHARWORD_MODELS:
            for f in GPU_LANE_FORMS:
                yield pytest.param(m, "lane_" + f, id="%s-lane_%s" % (m, f))


@pytest.mark.gpu
@pytest.mark.parametrize("model,form", list(_gpu_cases()))
def test_gpu_sweep(model, form, oracle):
    """The whole corpus, nothing thinned: EncodePackedEx, NormalizePacked with offsets, EncodeSpansPacked, DecodePacked of
    the ids; the handle's defaults, the three forms the sweep was asked for, and the four lane-normalizer settings.
    char1k and word1k: the sentence corpus, NormalizePacked against the oracle, and the ids against the cuts restated over
    the oracle's normalized text (charword_ids; the oracle restates neither model type)."""
    from tests.test_gpu_parity import _load_with_env
    sp = _load_with_env(model, dict(GPU_LANE_FORMS[form[5:]] if form.startswith("lane_") else GPU_FORMS[form]))
    tag = "%s %s" % (model, form)
    if model in CHARWORD_MODELS:
        check_charword(tag, sp, full_parts(model)[0][1], charword_want(oracle, model), keep="sentences")
        return
    w = want(oracle, model)
    for name, part in full_parts(model):
        sp.SetProfiling(name == "documents")
        ids, io, st, failed = sp.EncodePackedEx(part.text, part.offs)
        assert failed == 0 and not np.asarray(st).any()
        if name == "documents":
            # 257 texts of 40 KB and more are few for a whole device (up to four a CU): the two-wavefront form takes them
            assert sp.LastProfile()["classes"][4]["kernel"] == ("BpeLongKernel" if model.startswith("bpe") else "UniLongPipeKernel")
            sp.SetProfiling(False)
        assert_same("%s, %s" % (tag, name), part, "encode", (ids, io), w("encode", part, name))
        assert_same("%s, %s" % (tag, name), part, "normalize", sp.NormalizePacked(part.text, part.offs, with_offsets=True),
                    w("normalize", part, name))
        assert_same("%s, %s" % (tag, name), part, "spans", sp.EncodeSpansPacked(part.text, part.offs), w("spans", part, name))
        assert_same("%s, %s" % (tag, name), part, "decode", sp.DecodePacked(ids, io), w("decode", part, name))
