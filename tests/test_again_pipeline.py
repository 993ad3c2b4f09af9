"""The second word round's probe pipeline (kernels_wordwave.h, kWmDyn): the call-local memo's first slot tested straight
from the stage's registers, other slots walked to (dyn_walk), the ids' second row asked for where it is stored, and the
round's own launch bound (at most kWwAgainMaxWaves wavefronts a workgroup).  Every sentence against the oracle, on the CPU
emulator (test_emu_*) and on the GPU (test_gpu_*); both word-per-lane rounds must have run and nothing may have failed."""
import numpy as np
import pytest

from sentencepiece_amd import synth
from tests import fixtures, wordfuzz


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.EmuLib()


@pytest.fixture(scope="module")
def gpu():
    from tests import emulib
    return emulib.GpuLib()


def _check(lib, oracle, model, sents, env=None, what=""):
    """sents through `model` on `lib`: the oracle's ids for every sentence, both word-per-lane rounds ran, none failed."""
    assert len(sents) <= 2100
    blob = fixtures.model_blob(model)
    h, o = lib.load(blob, classes=None, env=dict(env or {})), oracle.load(blob)
    text, offs = synth.pack(sents)
    ids, io = h.encode_batch(text, offs)
    assert h.status == 0, what
    oids, oio = o.encode_batch(text, offs)
    k = wordfuzz.first_difference(ids, io, oids, oio)
    if k >= 0:
        a, b = np.asarray(io).astype(np.int64), np.asarray(oio).astype(np.int64)
        raise AssertionError("%s %s %r: sentence %d %r -> %s, reference %s" % (
            model, what, env, k, sents[k][:80], ids[a[k]:a[k + 1]].tolist()[:24], oids[b[k]:b[k + 1]].tolist()[:24]))
    prof = {c["kernel"]: c["sentences"] for c in h.sp.LastProfile()["classes"] if c["kernel"]}
    assert any(k.startswith("EncodeWordWaveCollect") for k in prof) and any(k.startswith("EncodeWordWaveAgain") for k in prof), prof
    assert h.path()["failed"] == 0
    return prof


def _again(prof):
    return sum(v for k, v in prof.items() if k.startswith("EncodeWordWaveAgain"))


def _made_up(n, seed, lo=5, hi=12):
    """n distinct letter strings no vocabulary holds as a word: the first round defers their sentences to the second."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        w = bytes(rng.choice(list(b"bcdfghjklmnpqrstvwxz"), size=int(rng.integers(lo, hi))).tolist())
        if w not in out:
            out.append(w)
    return out


def _deferring_batch(words, odd, seed, n=700):
    """tests/test_dense_arena.py's recipe: sentences of memo words with made-up words at the first, a middle and the last
    word, in runs of consecutive sentences, beside plain sentences, empty and all-space ones."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ws = [words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(1, 30)))]
        kind = (i // 3) % 6
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


_shared = {}


def _words(model, limit=500):
    key = ("words", model, limit)
    if key not in _shared:
        _shared[key] = wordfuzz.whole_words(fixtures.model_blob(model), limit=limit)
    return _shared[key]


def _by_pieces(model, cands):
    """{pieces: [word, ...]} of the candidates the reference segments without an unknown piece."""
    import sentencepiece as spm
    key = ("pieces", model, tuple(cands[:4]), len(cands))
    if key not in _shared:
        ref = spm.SentencePieceProcessor(model_proto=fixtures.model_blob(model))
        unk, out = ref.unk_id(), {}
        for w in cands:
            ids = ref.encode(w.decode("utf-8"))
            if unk not in ids:
                out.setdefault(len(ids), []).append(w)
        _shared[key] = out
    return _shared[key]


# ---- first slot against walked slot ----

SLOTS = [{"SPMX_DYN_SLOTS_LOG2": "4"}, {"SPMX_DYN_SLOTS_LOG2": "5"}, {"SPMX_DYN_SLOTS_LOG2": "6"}, {}]


def _case_slots(lib, oracle, env):
    """50 distinct made-up words in a table of 16, 32 and 64 slots: collisions, walks towards kDynProbes, a full table whose
    words go on to the general kernels; the default table (2^20 slots) is the first-slot-only control."""
    sents = _deferring_batch(_words("uni32k"), _made_up(50, 71), 72)
    prof = _check(lib, oracle, "uni32k", sents, env, "slots")
    assert _again(prof) > 0
    if env.get("SPMX_DYN_SLOTS_LOG2") == "6":
        # 50 words fit 64 slots, nearly all of them away from the slot their hash names: the second round finishes what it
        # finishes with the default table (every word in its first slot) unless a word sits more than kDynProbes slots from
        # its own -- without the walk it finishes 261 of these 458 sentences
        key = ("slots control", type(lib).__name__)
        if key not in _shared:
            _shared[key] = _again(_check(lib, oracle, "uni32k", sents, {}, "slots control"))
        assert _again(prof) >= 0.9 * _shared[key], (prof, _shared[key])


@pytest.mark.parametrize("env", SLOTS)
def test_emu_first_slot_against_walked_slot(env, emu, oracle):
    _case_slots(emu, oracle, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", SLOTS)
def test_gpu_first_slot_against_walked_slot(env, gpu, oracle):
    _case_slots(gpu, oracle, env)


# ---- entry shapes ----

def _fullwidth(w):
    return "".join(chr(0xFF00 + c - 0x20) for c in w).encode("utf-8")


def _sentences_with(words, special, seed, n=600):
    """n sentences of memo words with one to three of `special` anywhere, every special word used many times."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ws = [words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(0, 14)))]
        for _ in range(int(rng.integers(1, 4))):
            ws.insert(int(rng.integers(0, len(ws) + 1)), special[(i + int(rng.integers(0, 3))) % len(special)])
        out.append(b" ".join(ws))
    return out


def _case_pieces_1_to_8(lib, oracle):
    """Words of the call-local memo with 1 .. 4 ids (the first row of ids) and 5 .. 8 (the second row, asked for at the
    store).  One piece: a vocabulary word in fullwidth letters, which Normalize folds (not a key of the load-time memo)."""
    words = _words("uni32k")
    one = [_fullwidth(w) for w in words if 2 <= len(w) <= 5 and w.isalpha()][:12]
    rng = np.random.default_rng(73)
    src = b"etaoinshrdlucmfwypvbgkqjxz"
    cands = one + [bytes(src[int(i)] for i in rng.integers(0, len(src), size=int(rng.integers(3, 16)))) for _ in range(3000)]
    by = _by_pieces("uni32k", cands)
    assert all(len(by.get(k, [])) >= 1 for k in range(1, 9)), {k: len(v) for k, v in by.items()}
    assert any(w in by[1] for w in one)
    special = [w for k in range(1, 9) for w in by[k][:6]]
    prof = _check(lib, oracle, "uni32k", _sentences_with(words, special, 74), None, "1..8 pieces")
    assert _again(prof) > 300
    for env in ({"SPMX_NO_IDS16": "1"},):
        _check(lib, oracle, "uni32k", _sentences_with(words, special, 75, n=300), env, "1..8 pieces")


def test_emu_words_of_one_to_eight_pieces(emu, oracle):
    _case_pieces_1_to_8(emu, oracle)


@pytest.mark.gpu
def test_gpu_words_of_one_to_eight_pieces(gpu, oracle):
    _case_pieces_1_to_8(gpu, oracle)


WIDE_MODELS = ["uni1k_bf", "bpe1k"]


def _case_wide(lib, oracle, model):
    """Words of 9 .. 16 pieces (wide entries: 16-bit ids, two to a dword, both rows) beside words of 5 .. 8."""
    rng = np.random.default_rng(76)
    src = b"etaoinshrdlucmfwypvbgkqjxz0123456789QZ"
    cands = [bytes(src[int(i)] for i in rng.integers(0, len(src), size=int(rng.integers(6, 17)))) for _ in range(3000)]
    by = _by_pieces(model, cands)
    wide = [w for k in range(9, 17) for w in by.get(k, [])[:8]]
    mid = [w for k in range(5, 9) for w in by.get(k, [])[:4]]
    assert len(wide) >= 24 and len({len(w) for w in wide}) > 2 and len(mid) >= 4, (len(wide), len(mid))
    prof = _check(lib, oracle, model, _sentences_with(_words(model, 300), wide + mid, 77), None, "9..16 pieces")
    assert _again(prof) > 300


@pytest.mark.parametrize("model", WIDE_MODELS)
def test_emu_words_of_nine_to_sixteen_pieces_in_the_pipeline(model, emu, oracle):
    _case_wide(emu, oracle, model)


@pytest.mark.gpu
@pytest.mark.parametrize("model", WIDE_MODELS)
def test_gpu_words_of_nine_to_sixteen_pieces_in_the_pipeline(model, gpu, oracle):
    _case_wide(gpu, oracle, model)


def _case_unknown_runs(lib, oracle):
    """uni1k (no byte fallback): an unknown-piece run that continues across two words of the call-local memo (kDynLastUnk of
    the one, kDynFirstUnk of the next), and a word Normalize drops altogether (no ids) next to such runs."""
    words = _words("uni1k", 300)
    unk = ["日本", "語", "東京x", "x東京", "ab日", "日ab", "本"]
    gone = ["\u200b", "\ufeff"]                                # normalize to nothing
    pool = [w.encode("utf-8") for w in unk + gone]
    rng = np.random.default_rng(78)
    sents = []
    for i in range(600):
        ws = [words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(0, 8)))]
        at = int(rng.integers(0, len(ws) + 1))
        run = [pool[int(j)] for j in rng.integers(0, len(pool), size=int(rng.integers(1, 5)))]
        sents.append(b" ".join(ws[:at] + run + ws[at:]))
    # the shapes by name: unknown | unknown, unknown | dropped | unknown, dropped | unknown, unknown | dropped
    for a in (["日本", "語"], ["ab日", "日ab"], ["日本", "\u200b", "語"], ["\u200b", "語"], ["日本", "\u200b"], ["\u200b"]):
        for lead in ([], [words[0]], [words[1], words[2]]):
            sents.append(b" ".join(lead + [w.encode("utf-8") for w in a] + lead))
    prof = _check(lib, oracle, "uni1k", sents, None, "unknown runs")
    assert _again(prof) > 100


def test_emu_unknown_runs_and_dropped_words(emu, oracle):
    _case_unknown_runs(emu, oracle)


@pytest.mark.gpu
def test_gpu_unknown_runs_and_dropped_words(gpu, oracle):
    _case_unknown_runs(gpu, oracle)


# ---- batch edges ----

def _case_batch_edges(lib, oracle, env):
    """Sentences of exactly 63 .. 129 words with their made-up word first, last and at words 63 / 64 (a batch is 64 words);
    a tile whose batches hit the call-local memo in every lane, one with batches in which no lane does, sentences that
    continue across three batches."""
    words = _words("uni32k")
    odd = _made_up(40, 79)
    rng = np.random.default_rng(80)
    sents = []
    for W in (63, 64, 65, 127, 128, 129):
        for at in (0, W - 1, 62, 63, 64):
            if at >= W:
                continue
            ws = [words[int(j)] for j in rng.integers(0, len(words), size=W)]
            ws[at] = odd[(W + at) % len(odd)]
            sents.append(b" ".join(ws))
            sents.append(b" ".join(ws[:at] + [odd[(W + at + 1) % len(odd)]] + ws[at + 1:] + [odd[3]]))   # ... and a second one behind it
    for k in range(24):                                        # every lane of every batch hits the call-local memo
        sents.append(b" ".join(odd[int(j)] for j in rng.integers(0, len(odd), size=(64, 128, 200, 70)[k % 4])))
    for k in range(24):                                        # the made-up word, then three batches in which no lane does
        sents.append(b" ".join([odd[k % len(odd)]] + [words[int(j)] for j in rng.integers(0, len(words), size=(63, 127, 191, 250)[k % 4])]))
    sents += _deferring_batch(words, odd, 81, n=150)
    prof = _check(lib, oracle, "uni32k", sents, env, "batch edges")
    assert _again(prof) > 100


EDGE_VARIANTS = [{}, {"SPMX_NO_IDS16": "1"}, {"SPMX_WORDWAVE_WAVES": "1"}]


@pytest.mark.parametrize("env", EDGE_VARIANTS)
def test_emu_batch_edges(env, emu, oracle):
    _case_batch_edges(emu, oracle, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", EDGE_VARIANTS)
def test_gpu_batch_edges(env, gpu, oracle):
    _case_batch_edges(gpu, oracle, env)


# ---- variants ----

VARIANTS = [{}, {"SPMX_NO_IDS16": "1"}, {"SPMX_NO_DIRECT": "1"}, {"SPMX_WORDWAVE_WAVES": "1"}, {"SPMX_WORDWAVE_WAVES": "12"},
            {"SPMX_WORDWAVE_WAVES": "14"}, {"SPMX_WORDWAVE_WAVES": "16"}]


def _case_variants(lib, oracle, env, model):
    """SPMX_WORDWAVE_WAVES beyond the second round's launch bound still runs: that round's launch is clamped (api.cc)."""
    n = 2000 if model == "uni32k" else 700
    prof = _check(lib, oracle, model, _deferring_batch(_words(model), _made_up(60, 82), 83, n=n)[:2100], env, "variants")
    assert _again(prof) > 0


@pytest.mark.parametrize("env", VARIANTS)
@pytest.mark.parametrize("model", ["uni32k", "bpe32k"])
def test_emu_variants(model, env, emu, oracle):
    _case_variants(emu, oracle, env, model)


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS)
@pytest.mark.parametrize("model", ["uni32k", "bpe32k"])
def test_gpu_variants(model, env, gpu, oracle):
    _case_variants(gpu, oracle, env, model)
