"""CalculateEntropy on the device (kernels_nbest.h mode 3) against the COMPILED REFERENCE's number.

The reference's float32 entropy is far from the exact value on long text (alpha grows, ``alpha[l] - alpha[r]`` loses its
digits), so parity with the reference is the contract: tests/golden/lattice_scores.json holds its result bit for bit
(scripts/make_lattice_score_golden.py) beside the float64 exact entropy.

    emulated   bit-equal to the golden reference: the emulator's libm is the reference's, a difference is an
               order-of-operations bug
    MI355X     |dev - ref| <= 2e-4 |ref| + 1e-6: 3.5 times the worst case (5.7e-5) of a variant with the same order but an
               all-float32 libm; the device's double exp / log rounded to float are expected far inside

Teeth: the exact entropy lies OUTSIDE that bound of the reference for most sentences of 3000 device bytes and more, so a
kernel that computes the "right" entropy in another order or precision fails.

Lengths are in device form (U+2581 one byte): 1023 / 1024 run in the first lattice launch, 1025, 3000 and 6000 in the wide
one, and "㍿" * 40 among short sentences outgrows the batch's guess and is set aside.

Seen (fixed inputs): emulated, all 260 golden cases bit-equal.  MI355X: 258 of 260 bit-equal, the other two (test_model
3000 bytes and uni1k_uds 6000 bytes at theta 0.2) off by 5.64e-7 and 5.44e-7 relative: the last bit of expf, which the device
replaces by the double exp rounded to float.
"""
import collections

import numpy as np
import pytest

from tests import fixtures, latticeref, latticescore as ls
from tests.test_sampling import _Eng

RTOL, ATOL = 2e-4, 1e-6
MODELS = [m for m, _, _ in ls.SENTENCES]


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def emu(request):
    return _Eng(request.param)


@pytest.fixture(scope="module")
def procs(emu):
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = emu.load(fixtures.model_blob(model))
        return cache[model]
    return get


def cases_of(model):
    """[(sentence record, {theta: (reference float32, exact float64)})] of a model, in the golden file's order."""
    g = ls.golden()
    by = collections.defaultdict(dict)
    for c in g["entropy"]:
        by[c["sentence"]][c["theta"]] = (ls.from_bits(c["ref_bits"]), c["exact"])
    return [(s, by[i]) for i, s in enumerate(g["sentences"]) if s["model"] == model]


def within(dev, ref):
    return abs(float(dev) - float(ref)) <= RTOL * abs(float(ref)) + ATOL


def check(kind, got, want, what):
    """Emulated: the reference's bits.  Device: the bound.  -> (bit-equal?, relative difference)."""
    same = ls.bits(got) == ls.bits(want)
    rel = abs(float(got) - float(want)) / abs(float(want)) if float(want) != 0.0 else abs(float(got))
    if kind == "emu":
        assert same, (what, float(got), float(want))
    else:
        assert within(got, want), (what, float(got), float(want), rel)
    return same, rel


# ----------------------------------------------------------------------------------------------- 1. the instruments ----
def test_golden_lengths():
    """The golden sentences sit where the file says: the capacity boundary is hit exactly."""
    for model, kind, lengths in ls.SENTENCES:
        got = {s["name"]: s["dev_len"] for s, _ in cases_of(model)}
        for L in lengths:
            if model in ls.EXACT_MODELS and L in (63, 64, 65, 1023, 1024, 1025):
                assert got["%s%d" % (kind, L)] == L
            elif L > 1:
                assert L <= got["%s%d" % (kind, L)] <= L + 8
        assert got["empty"] == 0 and got["spaces"] == 0


@pytest.mark.parametrize("model", MODELS)
def test_helper_matches_reference(model, oracle):
    """tests/latticescore.py's same-order float32 entropy against the compiled reference's bits: equality is expected
    (the double exp rounded to float is what glibc's expf gives but for a rare last bit), 1e-6 relative is asserted."""
    lm = latticeref.Model(fixtures.model_blob(model))
    o = oracle.load(fixtures.model_blob(model))
    equal = total = 0
    for s, per in cases_of(model):
        norm = o.normalize(s["raw"].encode())
        assert ls.dev_len(norm) == s["dev_len"]
        lat = latticeref.Lattice(lm, norm)
        for theta, (ref, _) in per.items():
            mine = ls.entropy32(lat, theta)
            total += 1
            equal += ls.bits(mine) == ls.bits(ref)
            assert abs(float(mine) - float(ref)) <= 1e-6 * abs(float(ref)), (model, s["name"], theta, float(mine), float(ref))
    print("helper %s: %d of %d cases bit-equal to the reference" % (model, equal, total))


def test_exact_entropy_is_outside_the_bound():
    """The teeth: at 3000 device bytes and more the float64 exact entropy misses the reference by more than the device
    bound in at least half of the cases -- computing the true entropy is not what passes this file."""
    out = total = 0
    for model in MODELS:
        for s, per in cases_of(model):
            if s["dev_len"] < 3000:
                continue
            for theta, (ref, exact) in per.items():
                total += 1
                out += not within(exact, ref)
    print("exact entropy outside the device bound: %d of %d cases at >= 3000 bytes" % (out, total))
    assert total >= 16 and 2 * out >= total


@pytest.mark.parametrize("model", MODELS)
def test_logsumexp_cut_is_reached_at_theta_8(model, oracle):
    """At theta = 8 the terms into some position lie more than 50 apart from 64 bytes on: LogSumExp's early return runs."""
    lm = latticeref.Model(fixtures.model_blob(model))
    o = oracle.load(fixtures.model_blob(model))
    for s, _ in cases_of(model):
        if not 64 <= s["dev_len"] <= 1100 or s["name"] in dict(ls.FIXED):     # (the corpus sentences)
            continue
        lat = latticeref.Lattice(lm, o.normalize(s["raw"].encode()))
        al = lat.forward_backward(8.0)[0]
        v = al[lat.cb] + 8.0 * lat.score
        assert max(float(np.ptp(v[lat.ce == q])) for q in range(1, lat.n_chars + 1)) > 50.0, (model, s["name"])


# --------------------------------------------------------------------------------------------------- 2. the device ----
@pytest.mark.parametrize("theta", ls.THETAS)
@pytest.mark.parametrize("model", MODELS)
def test_entropy_matches_reference(model, theta, emu, procs):
    """Every golden sentence of the model once, in one batch: one character, 63 / 64 / 65, 300, the capacity boundary,
    the wide launch's 3000 and 6000, an empty and an all-space sentence."""
    from sentencepiece_amd import synth
    h = procs(model)
    cs = cases_of(model)
    text, offs = synth.pack([s["raw"].encode() for s, _ in cs])
    nt, no, _ = h.NormalizePacked(text, offs)
    for i, (s, _) in enumerate(cs):                               # the device's normalized text has the golden lengths
        assert ls.dev_len(nt[int(no[i]):int(no[i + 1])].tobytes()) == s["dev_len"]
    assert max(s["dev_len"] for s, _ in cs) > 1024                # ... so the wide launch runs too
    got = h.CalculateEntropyPacked(text, offs, theta)
    assert got.dtype == np.float32 and len(got) == len(cs)
    stats = [check(emu.kind, got[i], per[theta][0], (model, s["name"], theta)) for i, (s, per) in enumerate(cs)]
    print("entropy %s %s theta %g: %d of %d bit-equal, largest relative difference %.3g"
          % (emu.kind, model, theta, sum(a for a, _ in stats), len(stats), max(r for _, r in stats)))
    empty = [i for i, (s, _) in enumerate(cs) if s["dev_len"] == 0]
    assert empty and all(ls.bits(got[i]) == 0x80000000 for i in empty)   # -0.0, as the reference


@pytest.mark.parametrize("model", ["test_ja_model", "test_model"])
def test_entropy_of_a_sentence_that_outgrows_the_guess(model, emu, procs):
    """"㍿" * 40 (120 raw bytes) among short sentences: the batch's guess for the first launch (1.25 * longest raw + 16,
    rounded up to 64) is below its normalized length, it is set aside and runs in the wide launch."""
    from sentencepiece_amd import synth
    h = procs(model)
    (s, per), = [(s, per) for s, per in cases_of(model) if s["name"] == "expand"]
    raw = s["raw"].encode()
    assert (len(raw) + len(raw) // 4 + 16 + 63) & ~63 < s["dev_len"] <= 1024
    for theta in ls.THETAS:
        got = h.CalculateEntropyPacked(*synth.pack([b"hello", raw, b"a b", raw]), theta)
        check(emu.kind, got[1], per[theta][0], (model, "expand", theta))
        assert ls.bits(got[1]) == ls.bits(got[3])


def test_entropy_ignores_batch_composition(emu, procs):
    """A sentence's entropy depends on nothing else in the batch, nor on its index: the same sentence at indices 0, 63,
    64 and 199, among short ones and among sentences that are set aside (beyond 1024 bytes, or outgrowing the guess)."""
    from sentencepiece_amd import synth
    model, theta = "test_model", 0.2
    h = procs(model)
    rec = {s["name"]: (s["raw"].encode(), per[theta][0]) for s, per in cases_of(model)}
    at = {0: "en300", 63: "en300", 64: "en300", 199: "en300", 1: "en1025", 65: "en1025", 130: "en3000", 131: "expand",
          7: "empty", 8: "spaces", 62: "en1024", 66: "en1023", 198: "en1025"}
    sents = [b"hello world"] * 200
    for i, name in at.items():
        sents[i] = rec[name][0]
    got = h.CalculateEntropyPacked(*synth.pack(sents), theta)
    for i, name in at.items():
        check(emu.kind, got[i], rec[name][1], (name, i))
    for name in ("en300", "en1025"):
        assert len({ls.bits(got[i]) for i, n in at.items() if n == name}) == 1      # (bit for bit on the device too)
    plain = h.CalculateEntropyPacked(*synth.pack([b"hello world"]), theta)
    assert all(ls.bits(got[i]) == ls.bits(plain[0]) for i in range(200) if i not in at)
    # the processor's entry: a str gives a float, a list a list
    sp_one = h.CalculateEntropy("hello world", theta)
    assert isinstance(sp_one, float) and ls.bits(sp_one) == ls.bits(plain[0])
    assert h.calculate_entropy(["hello world", ""], theta) == [sp_one, -0.0]


@pytest.mark.parametrize("model", ["bpe1k", "char1k", "word1k"])
def test_entropy_is_not_available_for_other_models(model, emu):
    h = emu.load(fixtures.model_blob(model))
    with pytest.raises(RuntimeError, match="CalculateEntropy is not available for the current model."):
        h.CalculateEntropy("hello", 0.5)
