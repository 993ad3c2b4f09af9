"""How the tail behind the word rounds is launched (api.cc general_pass / long_launch): when the tail takes the
sentence-per-wavefront form, every length class that qualifies goes into ONE launch -- the classes' lists are copied behind
one another into one list; one kernel, one pool, one retry list, one read-back -- where there was a launch with a host
round trip per class.  Every sentence against the oracle, on the CPU emulator (test_emu_*) and on the GPU (test_gpu_*);
LastProfile()'s path counts the launches of the long form."""
import numpy as np
import pytest

from sentencepiece_amd import synth
from tests import fixtures, wordfuzz
from tests.test_again_pipeline import _made_up, _words


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.EmuLib()


@pytest.fixture(scope="module")
def gpu():
    from tests import emulib
    return emulib.GpuLib()


LONG_WORDS = [b"internationalisation", b"counterrevolutionaries", b"abcdefghijklmnopqrstuvwxyz", b"electroencephalography"]


def _mixed(n, seed, every=3):
    """n sentences of memo words; every `every`-th holds a made-up word (the first round defers it to the second), some
    are empty or all spaces."""
    words, odd = _words("uni32k"), _made_up(30, 91)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ws = [words[int(j)] for j in rng.integers(0, len(words), size=int(rng.integers(1, 20)))]
        if i % every == 0:
            ws[int(rng.integers(0, len(ws)))] = odd[int(rng.integers(0, len(odd)))]
        out.append(b" ".join(ws) if i % 41 != 7 else (b"", b" ", b"    ")[i % 3])
    return out


def _handed_on(targets, seed):
    """_mixed(300) with one sentence of about t bytes for every t of `targets` among them, each with a word of more than 16
    bytes: the word rounds hand those on, each to the list of its length class (192 / 576 / 1536 bytes ...)."""
    words = _words("uni32k")
    rng = np.random.default_rng(seed)
    sents = _mixed(300, seed + 1)
    for k, target in enumerate(targets):
        ws = []
        while sum(len(x) + 1 for x in ws) < target:
            ws.append(words[int(rng.integers(0, len(words)))])
        ws[(k * 7) % len(ws)] = LONG_WORDS[k % len(LONG_WORDS)]
        sents.insert(17 + 31 * k, b" ".join(ws))
    return sents


def _check(lib, oracle, sents, env, opts=""):
    blob = fixtures.model_blob("uni32k")
    h, o = lib.load(blob, classes=None, env=dict(env)), oracle.load(blob)
    if opts:
        h.set_encode_extra_options(opts)
        o.set_encode_extra_options(opts)
    text, offs = synth.pack(sents)
    ids, io = h.encode_batch(text, offs)
    assert h.status == 0
    oids, oio = o.encode_batch(text, offs)
    k = wordfuzz.first_difference(ids, io, oids, oio)
    if k >= 0:
        a, b = np.asarray(io).astype(np.int64), np.asarray(oio).astype(np.int64)
        raise AssertionError("%r %r: sentence %d %r -> %s, reference %s" % (
            env, opts, k, sents[k][:80], ids[a[k]:a[k + 1]].tolist()[:24], oids[b[k]:b[k + 1]].tolist()[:24]))
    assert h.path()["failed"] == 0
    prof = {c["kernel"]: c["sentences"] for c in h.sp.LastProfile()["classes"] if c["kernel"]}
    assert any(k.startswith("EncodeWordWaveCollect") for k in prof) and any(k.startswith("EncodeWordWaveAgain") for k in prof), prof
    return h, prof


def _long_form(prof):
    return sum(v for k, v in prof.items() if k.startswith("UniLong"))


TAIL_ENVS = [{}, {"SPMX_WORDWAVE_WAVES": "1"}, {"SPMX_NO_IDS16": "1"}, {"SPMX_NO_DIRECT": "1"}]


def _case_three_classes(lib, oracle, env):
    """A short, a middle and a long sentence (and more of each) with a word of more than 16 bytes: three length classes,
    one launch of the long form, which takes every one of them."""
    targets = (60, 400, 1200, 50, 420, 1000, 70, 1300)
    h, prof = _check(lib, oracle, _handed_on(targets, 100), env)
    assert _long_form(prof) >= len(targets), prof
    assert h.path()["long_launches"] == 1, h.path()


@pytest.mark.parametrize("env", TAIL_ENVS)
def test_emu_tail_of_three_classes_is_one_launch(env, emu, oracle):
    _case_three_classes(emu, oracle, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", TAIL_ENVS)
def test_gpu_tail_of_three_classes_is_one_launch(env, gpu, oracle):
    _case_three_classes(gpu, oracle, env)


def _case_class_counts(lib, oracle):
    """One class alone (its own list, no copy), two classes, five (up to 5,000 bytes: a document class among them), and a
    batch without such a sentence (no launch of the long form unless the word rounds hand something else on)."""
    for targets in ((300, 350, 320), (60, 1200), (60, 400, 1200, 3000, 5000, 80), ()):
        h, prof = _check(lib, oracle, _handed_on(targets, 102 + len(targets)), {})
        assert _long_form(prof) >= len(targets), (targets, prof)
        assert h.path()["long_launches"] == (1 if targets or _long_form(prof) else 0), (targets, h.path())


def test_emu_one_two_and_five_classes(emu, oracle):
    _case_class_counts(emu, oracle)


@pytest.mark.gpu
def test_gpu_one_two_and_five_classes(gpu, oracle):
    _case_class_counts(gpu, oracle)


def _case_extra_ids(lib, oracle, opts):
    h, prof = _check(lib, oracle, _handed_on((60, 400, 1200, 90), 110), {}, opts)
    assert h.path()["long_launches"] == 1, h.path()


@pytest.mark.parametrize("opts", ["bos", "bos:eos"])
def test_emu_extra_ids_in_the_merged_tail(opts, emu, oracle):
    _case_extra_ids(emu, oracle, opts)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["bos", "bos:eos"])
def test_gpu_extra_ids_in_the_merged_tail(opts, gpu, oracle):
    _case_extra_ids(gpu, oracle, opts)
