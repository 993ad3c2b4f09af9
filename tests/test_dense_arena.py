"""The word-per-lane rounds' dense id stream (kernels_wordwave.h): a tile's sentences' ids back to back in its arena region,
the direct call's first-round regions placed from the input offsets (no arena_head atomic), the second round's own region
with the ids in front of its resume point copied over; and the compaction's list of document blocks starting empty at
every compaction (api.cc scan_compact).  Every case against the oracle on the CPU emulator."""
import numpy as np
import pytest

from sentencepiece_amd import synth
from tests import fixtures, wordfuzz


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.EmuLib()


def _check(h, o, sents, what):
    text, offs = synth.pack(sents)
    ids, io = h.encode_batch(text, offs)
    assert h.status == 0, what
    oids, oio = o.encode_batch(text, offs)
    k = wordfuzz.first_difference(ids, io, oids, oio)
    if k >= 0:
        a, b = np.asarray(io).astype(np.int64), np.asarray(oio).astype(np.int64)
        raise AssertionError("%s: sentence %d %r -> %s, reference %s" % (
            what, k, sents[k][:80], ids[a[k]:a[k + 1]].tolist()[:24], oids[b[k]:b[k + 1]].tolist()[:24]))


def _ran_word_wave(h):
    prof = {c["kernel"]: c["sentences"] for c in h.sp.LastProfile()["classes"] if c["kernel"]}
    return any(k.startswith("EncodeWordWaveCollect") for k in prof) and any(k.startswith("EncodeWordWaveAgain") for k in prof), prof


def _deferring_batch(words, seed, n=700):
    """Sentences of memo words with words the load-time memo lacks (made-up letter strings: the first round defers their
    sentences to the second) at the first, a middle and the last word, in runs of consecutive sentences, beside plain
    sentences, empty and all-space ones."""
    rng = np.random.default_rng(seed)
    odd = [bytes(rng.choice(list(b"bcdfghjklmnpqrstvwxz"), size=int(rng.integers(5, 12))).tolist()) for _ in range(60)]
    out = []
    for i in range(n):
        ws = [words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(1, 30)))]
        kind = (i // 3) % 6                                   # runs of three sentences of a kind: consecutive deferrals
        o = odd[int(rng.integers(0, len(odd)))]
        if kind == 1:
            ws[0] = o
        elif kind == 2:
            ws[len(ws) // 2] = o
        elif kind == 3:
            ws[-1] = o
        elif kind == 4:
            ws = [o if rng.random() < 0.3 else w for w in ws]
        out.append(b" ".join(ws))
        if i % 97 == 0:
            out += [b"", b" ", b"   "]
    return out


@pytest.mark.parametrize("variant", [{}, {"SPMX_NO_IDS16": "1"}, {"SPMX_NO_DIRECT": "1"}, {"SPMX_WORD_WAVE": "1"},
                                     {"SPMX_WORD_WAVE": "2"}])
@pytest.mark.parametrize("model", ["uni32k", "bpe32k"])
def test_emu_deferred_sentences_in_the_dense_stream(model, variant, emu, oracle):
    blob = fixtures.model_blob(model)
    words = wordfuzz.whole_words(blob, limit=500)
    h, o = emu.load(blob, classes=None, env=variant), oracle.load(blob)
    _check(h, o, _deferring_batch(words, 11), "%s %r" % (model, variant))
    if not variant:
        ok, prof = _ran_word_wave(h)
        assert ok, prof


@pytest.mark.parametrize("opts", ["bos", "eos", "bos:eos", "reverse", "bos:eos:reverse"])
def test_emu_extra_options_in_the_dense_stream(opts, emu, oracle):
    """The extra ids take their places in the stream; an empty or all-space sentence still takes them."""
    blob = fixtures.model_blob("uni32k")
    words = wordfuzz.whole_words(blob, limit=500)
    h, o = emu.load(blob, classes=None), oracle.load(blob)
    h.set_encode_extra_options(opts)
    o.set_encode_extra_options(opts)
    sents = _deferring_batch(words, 12, n=400) + [b"", b" ", b"  ", b"a"] * 5
    _check(h, o, sents, opts)


@pytest.mark.parametrize("variant", [{}, {"SPMX_NO_IDS16": "1"}, {"SPMX_NO_DIRECT": "1"}])
def test_emu_dense_stream_arena_overflow_and_retry(variant, emu, oracle):
    """SPMX_ARENA_FIRST: the direct call's first-round regions (and the second round's) do not fit the first attempt's
    arena; the overflow is flagged and the retry, with the arena arena_head asks for, gives the same ids."""
    blob = fixtures.model_blob("uni32k")
    words = wordfuzz.whole_words(blob, limit=500)
    h, o = emu.load(blob, classes=None, env=dict(variant, SPMX_ARENA_FIRST="600")), oracle.load(blob)
    _check(h, o, _deferring_batch(words, 13, n=500), "arena_first %r" % variant)
    assert h.path()["arena_retries"] >= 1


def test_emu_compaction_twice_with_document_blocks_listed(emu, oracle):
    """A call that compacts twice (an overflow sentence takes the exact-capacity launch behind the first compaction) with
    every block listed for CompactBigKernel: the list starts empty at each compaction -- it used to grow past d_big_list."""
    from tests import emulib
    blob = fixtures.model_blob("bpe1k")
    h = emu.load(blob, classes=emulib.SMALL_CLASSES, env={"SPMX_COMPACT_BIG": "1", "SPMX_NO_WORD_NORM": "1"})
    o = oracle.load(blob)
    words = wordfuzz.whole_words(blob, limit=300)
    rng = np.random.default_rng(14)
    sents = [b" ".join(words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(1, 4)))) for _ in range(19200)]
    sents[9000] = ("ﷺ" * 40).encode()                     # NFKC: each of them 18 characters -- beyond every column
    _check(h, o, sents, "compact twice")
    assert h.path()["overflow"] >= 1
