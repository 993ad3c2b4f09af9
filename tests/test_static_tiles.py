"""The direct first word round's tile order (kernels_wordwave.h ww_next_tile): the launch's first tiles by the wavefront's
own index, the rest from the queue's cursor (SPMX_STATIC_TILES = the share taken by index).  A tile taken twice or never
shows as a sentence whose ids differ from the oracle's.  W = the wavefronts of a full first-round launch (wavefronts per
workgroup, from the profile, x compute units): batches of 1 .. 64 (2 W) + 65 sentences put the boundary between the two
orders in front of, at and behind a whole round of the launch.  On the CPU emulator (test_emu_*) and on the GPU (test_gpu_*)."""
import numpy as np
import pytest

from sentencepiece_amd import synth
from tests import fixtures, wordfuzz

MODEL = "uni32k"
FRACTIONS = ["0", "0.5", "0.875"]
EMU_CUS = 2


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.EmuLib()


@pytest.fixture(scope="module")
def gpu():
    from tests import emulib
    return emulib.GpuLib()


_shared = {}


def _pool():
    """2,048 sentences of 8 - 24 bytes, words of the load-time memo."""
    if "pool" not in _shared:
        words = [w for w in wordfuzz.whole_words(fixtures.model_blob(MODEL), limit=500) if 1 <= len(w) <= 9]
        rng = np.random.default_rng(1502)
        pool = []
        while len(pool) < 2048:
            room = int(rng.integers(8, 25))
            ws = []
            while True:
                w = words[int(rng.integers(0, len(words)))]
                if len(b" ".join(ws + [w])) > room:
                    break
                ws.append(w)
            s = b" ".join(ws)
            if 8 <= len(s) <= 24:
                pool.append(s)
        _shared["pool"] = pool
    return _shared["pool"]


def _waves(lib, cus):
    """W: wavefronts per workgroup of the first round (profile) x compute units."""
    h = lib.load(fixtures.model_blob(MODEL), classes=None, env={})
    text, offs = synth.pack(_pool()[:256])
    h.encode_batch(text, offs)
    per_wg = h.path()["word_waves_first"]
    assert per_wg >= 1, h.path()
    return per_wg * cus


def _corpus(oracle, n):
    """n sentences drawn from the pool, with the oracle's ids: made once per size, every smaller batch is a prefix."""
    if ("corpus", n) not in _shared:
        pool = _pool()
        pick = np.random.default_rng(1503).integers(0, len(pool), size=n)
        text, offs = synth.pack([pool[int(k)] for k in pick])
        oids, oio = oracle.load(fixtures.model_blob(MODEL)).encode_batch(text, offs)
        _shared[("corpus", n)] = (text, offs, np.asarray(oids), np.asarray(oio).astype(np.int64))
    return _shared[("corpus", n)]


def _case(lib, oracle, frac, cus):
    key = ("W", type(lib).__name__)
    if key not in _shared:
        _shared[key] = _waves(lib, cus)
    W = _shared[key]
    counts = [1, 63, 64, 65, 64 * W - 1, 64 * W, 64 * W + 1, 64 * (2 * W) + 65]
    text, offs, oids, oio = _corpus(oracle, counts[-1])
    h = lib.load(fixtures.model_blob(MODEL), classes=None, env={"SPMX_STATIC_TILES": frac})
    for n in counts:
        t, o = text[:int(offs[n])], offs[:n + 1]
        ids, io = h.encode_batch(t, o)
        assert h.status == 0, (frac, n)
        io = np.asarray(io).astype(np.int64)
        assert int(io[-1]) == len(ids) == int(oio[n]), (frac, n, int(io[-1]), len(ids), int(oio[n]))   # counts sum to the ids written
        k = wordfuzz.first_difference(ids, io, oids[:int(oio[n])], oio[:n + 1])
        assert k < 0, "f = %s, %d sentences (W = %d): sentence %d -> %s, reference %s" % (
            frac, n, W, k, np.asarray(ids)[io[k]:io[k + 1]].tolist()[:16], oids[oio[k]:oio[k + 1]].tolist()[:16])
        kernels = [c["kernel"] for c in h.sp.LastProfile()["classes"] if c["kernel"]]
        assert any(x.startswith("EncodeWordWaveCollect") for x in kernels), (frac, n, kernels)


@pytest.mark.parametrize("frac", FRACTIONS)
def test_emu_static_tiles(frac, emu, oracle):
    _case(emu, oracle, frac, EMU_CUS)


@pytest.mark.gpu
@pytest.mark.parametrize("frac", FRACTIONS)
def test_gpu_static_tiles(frac, gpu, oracle):
    import torch
    _case(gpu, oracle, frac, torch.cuda.get_device_properties(0).multi_processor_count)
