"""The word-per-lane rounds' LDS layout by mode (kernels_wordwave.h kWwShared / kWwPerWave): the first round carries
neither the table of likely words nor s_n0 / s_x0 and runs 16 wavefronts a workgroup, the second round keeps its own layout
and its bound of kWwAgainMaxWaves = 12.  LastProfile()["path"] reports what each round was launched with.  Every sentence
against the oracle, on the CPU emulator (test_emu_*) and on the GPU (test_gpu_*)."""
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


N_SHORT = 4096
AGAIN_MAX_WAVES = 12          # kernels_wordwave.h kWwAgainMaxWaves

_shared = {}


def _batch(model):
    """4,096 sentences of 8 - 40 bytes (64 tiles: four workgroups of 16 wavefronts, all of them on tiles), one in eight with a
    word round 1 cannot finish or take: made-up words of 5 - 11, of 16 and of 17 bytes (no load-time memo holds them: their
    sentences go to round 2 through the call-local memo, the 17-byte ones to the tail), words that are not plain ASCII; an
    empty sentence; one sentence beyond 64 KB (kWwMaxLen: not the word form's)."""
    if ("batch", model) in _shared:
        return _shared[("batch", model)]
    words = [w for w in wordfuzz.whole_words(fixtures.model_blob(model), limit=500) if 1 <= len(w) <= 10]
    rng = np.random.default_rng(1501)
    letters = list(b"bcdfghjklmnpqrstvwxz")

    def made_up(k):
        return bytes(rng.choice(letters, size=k).tolist())
    special = [made_up(int(k)) for k in rng.integers(5, 12, size=24)]
    special += [made_up(16) for _ in range(6)] + [made_up(17) for _ in range(6)]
    special += [w.encode("utf-8") for w in ("naïve", "日本", "語", "café", "ＡＢ", "über")]
    sents = []
    while len(sents) < N_SHORT:
        i = len(sents)
        room = int(rng.integers(8, 41))
        ws = []
        if i % 8 == 3:
            ws.append(special[(i // 8) % len(special)])
        while True:
            w = words[int(rng.integers(0, len(words)))]
            if len(b" ".join(ws + [w])) > room:
                break
            ws.append(w)
        if i % 8 == 3 and len(ws) > 1 and (i // 8) % 3:          # the special word last, or in the middle
            ws = ws[1:] + ws[:1] if (i // 8) % 3 == 1 else ws[1:2] + ws[:1] + ws[2:]
        s = b" ".join(ws)
        if 8 <= len(s) <= 40:
            sents.append(s)
    sents[1000] = b""
    long_words = []
    size = 0
    while size <= 65536 + 300:
        w = words[int(rng.integers(0, len(words)))]
        long_words.append(w)
        size += len(w) + 1
    sents.append(b" ".join(long_words))
    assert len(sents[-1]) > 65536
    _shared[("batch", model)] = synth.pack(sents) + (sents,)
    return _shared[("batch", model)]


def _reference(oracle, model):
    if ("ref", model) not in _shared:
        text, offs, _ = _batch(model)
        _shared[("ref", model)] = oracle.load(fixtures.model_blob(model)).encode_batch(text, offs)
    return _shared[("ref", model)]


VARIANTS = [{}, {"SPMX_NO_IDS16": "1"}, {"SPMX_NO_DIRECT": "1"}, {"SPMX_WORDWAVE_WAVES": "1"}, {"SPMX_WORDWAVE_WAVES": "15"},
            {"SPMX_WORDWAVE_WAVES": "16"}]
MODELS = ["uni32k", "bpe32k"]


def _case(lib, oracle, model, env):
    text, offs, sents = _batch(model)
    oids, oio = _reference(oracle, model)
    h = lib.load(fixtures.model_blob(model), classes=None, env=dict(env))
    ids, io = h.encode_batch(text, offs)
    assert h.status == 0
    k = wordfuzz.first_difference(ids, io, oids, oio)
    if k >= 0:
        a, b = np.asarray(io).astype(np.int64), np.asarray(oio).astype(np.int64)
        raise AssertionError("%s %r: sentence %d %r -> %s, reference %s" % (
            model, env, k, sents[k][:80], ids[a[k]:a[k + 1]].tolist()[:24], oids[b[k]:b[k + 1]].tolist()[:24]))
    prof = h.sp.LastProfile()
    kernels = {c["kernel"]: c["sentences"] for c in prof["classes"] if c["kernel"]}
    assert any(k.startswith("EncodeWordWaveCollect") for k in kernels), kernels
    again = sum(v for k, v in kernels.items() if k.startswith("EncodeWordWaveAgain"))
    assert again > 100, kernels                      # round 2 ran over sentences a round 1 without s_n0 / s_x0 left it
    assert prof["path"]["failed"] == 0
    want = int(env.get("SPMX_WORDWAVE_WAVES", "16"))
    assert prof["path"]["word_waves_first"] == want, prof["path"]
    assert prof["path"]["word_waves_second"] == min(want, AGAIN_MAX_WAVES), prof["path"]


@pytest.mark.parametrize("env", VARIANTS)
@pytest.mark.parametrize("model", MODELS)
def test_emu_layout_by_mode(model, env, emu, oracle):
    _case(emu, oracle, model, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS)
@pytest.mark.parametrize("model", MODELS)
def test_gpu_layout_by_mode(model, env, gpu, oracle):
    _case(gpu, oracle, model, env)
