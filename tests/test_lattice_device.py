"""The lattice calls on device buffers: spmx_nbest_encode_batch_device, spmx_sample_encode_batch_device and
spmx_sample_encode_and_score_batch_device, which leave the CSR of their results on the device
(sentencepiece_amd/csrc/kernels_latticecsr.h: rows pass, the project's scan, gather by aligned blocks of the output, the
pick of SampleEncode's n-best branch).

The expectation is the host-buffer form of the same call -- spmx_nbest_encode_batch and its siblings, which
tests/test_nbest.py, tests/test_sampling*.py and tests/test_sample_score.py pin to the oracle and the compiled reference --
and equality is exact: ids, offsets, and the scores bit for bit.  The one exception is SampleEncode with nbest_size > 1,
where the device draws with its own exp(); see test_sample_nbest_pick.

CPU: the device bodies under the wavefront emulator through the C ABI, host pointers standing in for device pointers.
GPU: the torch-tensor methods of processor.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import fixtures
from tests.emulib import EmuLib
from tests.test_decode_file import getline_split, packed
from tests.test_nbest import sentences

BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")
UNIGRAM = ["test_model", "uni1k_bf", "uni1k_uds", "test_ja_model"]
BPE = ["bpe1k", "bpe1k_llama"]
LONG = (b"zqxj vkqz 1907 xqzv " * 300)[:6000]                                # 6,000 bytes, results of more ids than a gather chunk holds
WIDE = (b"this is a test of the emergency broadcast system " * 6)[:280]      # an A* that outgrows the first hypothesis slice


@pytest.fixture(scope="module")
def emu():
    return EmuLib()


@pytest.fixture(scope="module")
def botchan():
    return getline_split(open(BOTCHAN, "rb").read())


def pad(text):
    return np.concatenate([np.ascontiguousarray(text, dtype=np.uint8), np.zeros(32, dtype=np.uint8)])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Placed:
    """A destination of `count` elements of `dtype`, `shift` bytes off a 16-byte boundary inside a 0xCD-filled block."""

    def __init__(self, count, dtype, shift):
        self.count, self.dtype = count, np.dtype(dtype)
        self.nbytes = count * self.dtype.itemsize
        self.raw = np.full(self.nbytes + 96, 0xCD, dtype=np.uint8)
        self.at = 32 + ((shift - self.raw.ctypes.data - 32) & 15)
        assert (self.raw.ctypes.data + self.at) % 16 == shift
        self.ptr = self.raw.ctypes.data + self.at

    def intact(self):
        return bool((self.raw[:self.at] == 0xCD).all() and (self.raw[self.at + self.nbytes:] == 0xCD).all())

    def untouched(self):
        return bool((self.raw == 0xCD).all())

    def array(self):
        return self.raw[self.at:self.at + self.nbytes].view(self.dtype).copy()


def scored_call(h, fn, text, offs, mid, ids, icap, io, sc, sent, rcap, ro):
    """One call of an n-best-shaped device form; buffers are Placed or None.  -> (rc, total_results, total_ids)"""
    n = len(offs) - 1
    tr, ti = C.c_uint64(0), C.c_uint64(0)
    p = [b.ptr if b is not None else None for b in (ids, io, sc, sent, ro)]
    rc = getattr(h.lib, fn)(h.sp._h, text.ctypes.data, int(offs[n]), offs.ctypes.data, n, *mid, p[0], icap, p[1], p[2], p[3], rcap,
                            p[4], None, C.byref(tr), C.byref(ti))
    return rc, tr.value, ti.value


def device_form(h, fn, text, offs, mid, shift=0, short=True):
    """The capacity protocol -- a query with null buffers, every capacity one short, the exact needs -- on destinations
    `shift` bytes (the uint64 arrays: 2 * shift, they need 8) off a 16-byte boundary; short=False leaves the two calls that are
    one short out (every call runs the search again).  -> (ids, io, sc, ro, sent)"""
    text, offs = pad(text), np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    rc, R, T = scored_call(h, fn, text, offs, mid, None, 0, None, None, None, 0, None)
    assert rc == (8 if n else 0), (rc, h.lib.spmx_last_error(None))

    def fresh():
        return (Placed(T, np.int32, shift), Placed(R + 1, np.uint64, 2 * shift), Placed(R, np.float32, shift),
                Placed(R, np.uint32, shift), Placed(n + 1, np.uint64, 2 * shift))
    if R and short:                                                   # one result short: nothing but result_offsets is written
        ids, io, sc, sent, ro = fresh()
        assert scored_call(h, fn, text, offs, mid, ids, T, io, sc, sent, R - 1, ro) == (8, R, T)
        assert ids.untouched() and io.untouched() and sc.untouched() and sent.untouched() and ro.intact()
    if T and short:                                                   # one id short: the rows are written, no id is
        ids, io, sc, sent, ro = fresh()
        assert scored_call(h, fn, text, offs, mid, ids, T - 1, io, sc, sent, R, ro) == (8, R, T)
        assert ids.untouched() and io.intact() and sc.intact() and sent.intact() and ro.intact()
    ids, io, sc, sent, ro = fresh()
    got = scored_call(h, fn, text, offs, mid, ids, T, io, sc, sent, R, ro)
    assert got == (0, R, T), (got, h.lib.spmx_last_error(None))
    for b in (ids, io, sc, sent, ro):
        assert b.intact(), "write outside a buffer"
    ids, io, sc, sent, ro = ids.array(), io.array(), sc.array(), sent.array(), ro.array()
    # sent_of_result agrees with result_offsets
    assert ro[0] == 0 and ro[n] == R and (np.diff(ro.astype(np.int64)) >= 0).all()
    assert np.array_equal(sent, np.repeat(np.arange(n, dtype=np.uint32), np.diff(ro.astype(np.int64))))
    assert io[0] == 0 and io[R] == T
    return ids, io, sc, ro, sent


def same(got, want, what):
    ids, io, sc, ro = got[:4]
    assert np.array_equal(ro, want[3]), what
    assert np.array_equal(io, want[1]), what
    assert np.array_equal(ids, want[0]), what
    assert np.array_equal(bits(sc), bits(want[2])), what


# ------------------------------------------------------------------------------------- 1. device form == host form ----
_HOST = {}


def host_nbest(emu, model, corp, k):
    key = (model, k)
    if key not in _HOST:
        sp = emu.load(fixtures.model_blob(model)).sp
        _HOST[key] = sp.NBestPacked(*corp, k)
    return _HOST[key]


@pytest.fixture(scope="module")
def corpus(botchan, corpora):
    return packed(botchan[:300] + sentences(corpora))


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("model", UNIGRAM)
def test_nbest_device_equals_host(model, cus, emu, corpus):
    h = emu.load(fixtures.model_blob(model), cus=cus)
    for k in (1, 2, 5, 64):
        got = device_form(h, "spmx_nbest_encode_batch_device", *corpus, (k,), shift=4 if k == 5 else 0, short=k == 2)
        same(got, host_nbest(emu, model, corpus, k), (model, cus, k))
        assert k > 1 or np.array_equal(got[3], np.arange(len(corpus[1]), dtype=np.uint64))


@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_nbest_device_extra_options(model, emu, corpus):
    h = emu.load(fixtures.model_blob(model), cus=3)
    try:
        for opts in ("bos:eos", "reverse:bos:eos"):
            h.set_encode_extra_options(opts)
            for k in (1, 5):
                got = device_form(h, "spmx_nbest_encode_batch_device", *corpus, (k,))
                same(got, h.sp.NBestPacked(*corpus, k), (model, opts, k))
    finally:
        h.set_encode_extra_options("")


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("model", UNIGRAM)
def test_sample_and_score_device_equals_host(model, cus, emu, botchan, corpora):
    """Modes 4 and 5 against spmx_sample_encode_and_score_batch with the same seed; an empty sentence owns no result (the
    sentence of a single path: test_one_path_sentence_owns_no_result)."""
    sents = botchan[:120] + [b"a", b"", b" "] + [s for s in sentences(corpora) if len(s) <= 250][:60]
    text, offs = packed(sents)
    h = emu.load(fixtures.model_blob(model), cus=cus)
    for wor, best, num, seed in ((0, 0, 1, 3), (0, 0, 4, 11), (1, 0, 3, 7), (1, 1, 3, 7), (1, 1, 1, 2 ** 63 + 5)):
        want = h.sp.SampleEncodeAndScorePacked(text, offs, num, 0.5, bool(wor), bool(best), seed)
        got = device_form(h, "spmx_sample_encode_and_score_batch_device", text, offs, (num, C.c_float(0.5), wor, best, seed),
                          shift=4 * wor)
        same(got, want, (model, cus, wor, best, num))
        ro = got[3].astype(np.int64)
        assert ro[122] == ro[121]                                     # the empty sentence


def test_one_path_sentence_owns_no_result(emu):
    """A sentence whose lattice has a single path: nothing without replacement, num_samples copies with replacement."""
    h = emu.load(fixtures.model_blob("uni1k_ident"), cus=1)
    text, offs = packed([b"hello world", b"\xe3\x81", b"hello"])       # (an invalid byte: one unknown node, one path)
    want = h.sp.SampleEncodeAndScorePacked(text, offs, 2, 0.5, True, True, 1)
    got = device_form(h, "spmx_sample_encode_and_score_batch_device", text, offs, (2, C.c_float(0.5), 1, 1, 1))
    same(got, want, "wor")
    counts = np.diff(got[3].astype(np.int64)).tolist()
    assert min(counts) == 0 and max(counts) > 0, counts


# ------------------------------------------------------------------------------- 2. where the CSR stage can go wrong ----
def shape_cases():
    one_word = [(b"w%d" % (i * 7919 % 1000)) for i in range(2000)]
    return [
        ("n0", [], 5),
        ("one_empty", [b""], 5),
        ("all_empty", [b""] * 700 + [b"hello world"] + [b""] * 700, 2),
        ("65", [b"hello world"] * 13, 5),
        ("129", [b"hello world"] * 43, 3),
        ("long", [b"a b", LONG, b"", b"hello world", b"x"], 2),
        ("one_word", one_word, 2),
        ("wide", [WIDE, b"hello world", b""], 400),                  # the id arena outgrows its first size: the regrow path
    ]


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("name,sents,k", shape_cases(), ids=[c[0] for c in shape_cases()])
def test_csr_shapes(name, sents, k, cus, emu):
    h = emu.load(fixtures.model_blob("test_model"), cus=cus)
    text, offs = packed(sents)
    # (the expectation from a handle of its own: this one's workspace is fresh, so the device form meets the first sizes)
    want = emu.load(fixtures.model_blob("test_model"), cus=cus).sp.NBestPacked(text, offs, k)
    for shift in (0, 4):
        got = device_form(h, "spmx_nbest_encode_batch_device", text, offs, (k,), shift=shift)
        same(got, want, (name, cus, shift))
    R = int(want[3][-1])
    if name in ("65", "129"):
        assert R == int(name)
    if name == "all_empty":
        assert R == 1400 + 2 and int(want[1][-1]) == int(want[1][702]) > 0 and int(want[1][700]) == 0
    if name == "long":
        assert int(np.diff(want[1].astype(np.int64)).max()) > 4096     # one result longer than a gather chunk


def test_csr_shapes_with_extras_on_empty_results(emu):
    """bos:eos gives the results of empty sentences two ids each: a flood of equal short rows."""
    h = emu.load(fixtures.model_blob("test_model"), cus=3)
    text, offs = packed([b""] * 300 + [b"hello world"] + [b""] * 300)
    try:
        h.set_encode_extra_options("bos:eos")
        got = device_form(h, "spmx_nbest_encode_batch_device", text, offs, (3,), shift=4)
        same(got, h.sp.NBestPacked(text, offs, 3), "bos:eos")
        assert int(got[1][-1]) > 2 * 600
    finally:
        h.set_encode_extra_options("")


def test_retry_rounds_and_small_budget(emu):
    """The handle's lattice seams: a first hypothesis slice of 1024 sends WIDE through the wide launches (the slice grows
    round by round), beside rows of the first launch."""
    h = emu.load(fixtures.model_blob("test_model"), cus=3, env={"SPMX_NBEST_HYPS_MIN": "1024", "SPMX_NBEST_BUDGET_GB": "1"})
    text, offs = packed([b"hello world", WIDE, b"", b"the cat", WIDE[:200], b"a"])
    for k in (8, 40):
        want = h.sp.NBestPacked(text, offs, k)
        same(device_form(h, "spmx_nbest_encode_batch_device", text, offs, (k,), shift=4), want, k)


def test_refusals(emu):
    text, offs = packed([b"hello"])
    text = pad(text)
    tr, ti = C.c_uint64(0), C.c_uint64(0)
    io = np.zeros(8, dtype=np.uint64)
    b = emu.load(fixtures.model_blob("bpe1k"))
    assert b.lib.spmx_nbest_encode_batch_device(b.sp._h, text.ctypes.data, 5, offs.ctypes.data, 1, 3, None, 0, None, None, None, 0, None,
                                                None, C.byref(tr), C.byref(ti)) == 13
    assert b"NBestEncode is not available for the current model." in b.lib.spmx_last_error(None)
    assert b.lib.spmx_sample_encode_and_score_batch_device(b.sp._h, text.ctypes.data, 5, offs.ctypes.data, 1, 2, C.c_float(0.5), 0, 0, 0,
                                                           None, 0, None, None, None, 0, None, None, C.byref(tr), C.byref(ti)) == 13
    assert b"SampleEncodeAndScore is not available for the current model." in b.lib.spmx_last_error(None)
    u = emu.load(fixtures.model_blob("test_model"))
    for args, msg in (((2, C.c_float(0.5), 0, 1, 0), b"returns empty result"), ((0, C.c_float(0.5), 1, 0, 0), b"returns empty result"),
                      ((513, C.c_float(0.5), 1, 0, 0), b"num_samples <= 512")):
        assert u.lib.spmx_sample_encode_and_score_batch_device(u.sp._h, text.ctypes.data, 5, offs.ctypes.data, 1, *args, None, 0, None, None,
                                                               None, 0, None, None, C.byref(tr), C.byref(ti)) == 13
        assert msg in u.lib.spmx_last_error(None)
    assert u.lib.spmx_sample_encode_batch_device(u.sp._h, text.ctypes.data, 5, offs.ctypes.data, 1, 513, C.c_float(0.5), 0, 0, None, 0,
                                                 io.ctypes.data, None, C.byref(ti)) == 13
    assert b"nbest_size <= 512" in u.lib.spmx_last_error(None)
    for m in ("char1k", "word1k"):
        c = emu.load(fixtures.model_blob(m), classes=None)
        assert c.lib.spmx_sample_encode_batch_device(c.sp._h, text.ctypes.data, 5, offs.ctypes.data, 1, -1, C.c_float(0.5), 0, 0, None, 0,
                                                     io.ctypes.data, None, C.byref(ti)) == 13
        assert b"SampleEncode is not available for the current model." in c.lib.spmx_last_error(None)


# ------------------------------------------------------------------------------------------------------ 3. sampling ----
def sample_device(h, text, offs, nbest_size, alpha, seed, index_base=0, shift=0, probe=True):
    """probe: the capacity protocol first (a query, one id short); else one call with room to spare."""
    text, offs = pad(text), np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    base = int(offs[0])
    text_ptr = text.ctypes.data                                       # (offsets are used as given: text + offs[i])
    ti = C.c_uint64(0)

    def call(ids, icap, io):
        rc = h.lib.spmx_sample_encode_batch_device(h.sp._h, text_ptr, int(offs[n]) - base, offs.ctypes.data, n, nbest_size, C.c_float(alpha),
                                                   seed, index_base, ids.ptr if ids is not None else None, icap,
                                                   io.ptr if io is not None else None, None, C.byref(ti))
        return rc, ti.value
    if not probe:
        ids, io = Placed(len(text) + 4 * n, np.int32, shift), Placed(n + 1, np.uint64, 2 * shift)
        rc, T = call(ids, ids.count, io)
        assert rc == 0 and ids.intact() and io.intact(), h.lib.spmx_last_error(None)
        return ids.array()[:T], io.array()
    rc, T = call(None, 0, None)
    assert rc == (8 if n else 0), (rc, h.lib.spmx_last_error(None))
    if T:
        ids, io = Placed(T, np.int32, shift), Placed(n + 1, np.uint64, 2 * shift)
        assert call(ids, T - 1, io) == (8, T) and ids.untouched() and io.intact()
    ids, io = Placed(T, np.int32, shift), Placed(n + 1, np.uint64, 2 * shift)
    assert call(ids, T, io) == (0, T), h.lib.spmx_last_error(None)
    assert ids.intact() and io.intact()
    return ids.array(), io.array()


def rows(ids, io):
    io = np.asarray(io).astype(np.int64)
    return [ids[io[i]:io[i + 1]].tolist() for i in range(len(io) - 1)]


@pytest.mark.parametrize("model", UNIGRAM)
def test_sample_device_equals_host_unigram(model, emu, botchan, corpora):
    sents = botchan[:300] + [s for s in sentences(corpora) if len(s) <= 250]
    text, offs = packed(sents)
    h = emu.load(fixtures.model_blob(model), cus=3)
    for nbest_size, alpha, seed in ((-1, 0.1, 0), (-1, 0.5, 12345), (0, 0.1, 1), (1, 0.1, 1)):
        want = h.sp.SampleEncodePacked(text, offs, nbest_size, alpha, seed)
        got = sample_device(h, text, offs, nbest_size, alpha, seed, shift=4 if seed else 0)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (model, nbest_size, alpha, seed)


@pytest.mark.parametrize("model", BPE)
def test_sample_device_equals_host_bpe(model, emu, botchan):
    text, offs = packed(botchan[:200] + [b"", b"hello world", "吾輩は猫である".encode()])
    h = emu.load(fixtures.model_blob(model), cus=3)
    for alpha in (0.0, 0.1, 1.0):
        for nbest_size in (-1, 3):
            want = h.sp.SampleEncodePacked(text, offs, nbest_size, alpha, 9)
            got = sample_device(h, text, offs, nbest_size, alpha, 9)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (model, alpha, nbest_size)
    assert rows(*h.sp.SampleEncodePacked(text, offs, -1, 0.0, 9)) == rows(*h.sp.EncodePacked(text, offs))


@pytest.mark.parametrize("model,nbest_size,alpha", [("test_model", -1, 0.3), ("test_model", 5, 0.5), ("uni1k_bf", -1, 0.1),
                                                     ("bpe1k", -1, 0.2), ("bpe1k_llama", -1, 0.5)])
def test_index_base(model, nbest_size, alpha, emu, botchan):
    """Sentences [k, n) run with index_base = k are the rows k..n of the whole batch."""
    sents = botchan[:150]
    h = emu.load(fixtures.model_blob(model), cus=3)
    whole = rows(*sample_device(h, *packed(sents), nbest_size, alpha, 77))
    assert whole != rows(*sample_device(h, *packed(sents), nbest_size, alpha, 78))       # (the seed matters)
    for k in (1, 64, 149):
        part = rows(*sample_device(h, *packed(sents[k:]), nbest_size, alpha, 77, index_base=k))
        assert part == whole[k:], (model, k)
        if k == 64:
            assert rows(*sample_device(h, *packed(sents[k:]), nbest_size, alpha, 77)) != whole[k:]


def splitmix_uniform(seed, index):
    m = (1 << 64) - 1
    x = (seed * 0x9E3779B97F4A7C15 + (index + 1) * 0xD1B54A32D192ED03) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    x ^= x >> 31
    return float(x >> 11) * (1.0 / 9007199254740992.0)


def check_sample_nbest_pick(nbest_packed, sample_rows, sents):
    """SampleEncode with nbest_size > 1 draws result c of a sentence where the uniform u * Z falls into the c-th interval of
    the cumulative weights exp(alpha * score - max).  The device computes exp in double with its own library, the host
    with glibc's: the two may differ in the last place, so only a draw within 1e-9 * Z of a boundary may differ.  Those
    sentences are set aside; with a 53-bit uniform the expected number over 2,000 sentences x 5 results is about 2e-5, so
    none is set aside here (the condition: at most 1 in 1,000)."""
    text, offs = packed(sents)
    ids, io, sc, ro = nbest_packed(text, offs, 5)
    res = rows(ids, io)
    ro = ro.astype(np.int64)
    alpha = np.float32(0.5)
    for seed in (0, 1, 2 ** 40 + 3):
        got = sample_rows(text, offs, 5, float(alpha), seed)
        aside = 0
        for s in range(len(sents)):
            w = np.float64(alpha) * sc[ro[s]:ro[s + 1]].astype(np.float64)
            e = np.exp(w - w.max())
            cum = np.cumsum(e)
            z = cum[-1]
            u = splitmix_uniform(seed, s) * z
            if np.abs(cum[:-1] - u).min(initial=np.inf) <= 1e-9 * z:
                aside += 1
                continue
            c = int(np.searchsorted(cum, u, side="right"))
            c = min(c, len(cum) - 1)
            assert got[s] == res[ro[s] + c], (seed, s, c)
        print("seed %d: %d of %d sentences set aside" % (seed, aside, len(sents)))
        assert aside * 1000 <= len(sents)
        assert aside == 0


def test_sample_nbest_pick(emu, botchan):
    h = emu.load(fixtures.model_blob("test_model"), cus=3)
    sents = botchan[:2000]
    check_sample_nbest_pick(h.sp.NBestPacked, lambda t, o, k, a, seed: rows(*sample_device(h, t, o, k, a, seed, probe=False)), sents)
    # and the host loop draws the same rows
    text, offs = packed(sents[:500])
    assert rows(*sample_device(h, text, offs, 5, 0.5, 4, shift=4)) == rows(*h.sp.SampleEncodePacked(text, offs, 5, 0.5, 4))


@pytest.mark.parametrize("kernel", ["LatticeCsrRowsKernel", "LatticeCsrGatherKernel", "LatticePickKernel", "LatticeIotaKernel",
                                    "LatticeMaxLenKernel", "LatticeSpFlagKernel", "LatticeRefSpanKernel"])
def test_new_kernels_use_no_scratch(kernel):
    """The compiler's resource report of the product library, which csrc/Makefile writes beside it with kernels.o: no
    scratch, no spilled register, no LDS in the kernels of kernels_latticecsr.h.  The report is part of every build, so its
    absence is a failure, not a reason to skip."""
    from tests.test_kernel_resources import REPORT, _report
    assert os.path.exists(REPORT), "no resource report next to the library: build it (make -C sentencepiece_amd/csrc)"
    rep = _report()
    names = [n for n in rep if kernel in n]
    assert len(names) == 1, (kernel, names)
    r = rep[names[0]]
    print(kernel, {k: r[k] for k in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")})
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == 0, r


# ----------------------------------------------------------------------------------------------------------- GPU half ----
def _dev(text, offs):
    import torch
    t = torch.from_numpy(pad(text)).cuda()[:len(text)]
    o = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).cuda()
    return t, o


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.fixture(scope="module")
def gpu_sp():
    from sentencepiece_amd.processor import SentencePieceProcessor
    return {m: SentencePieceProcessor(model_proto=fixtures.model_blob(m)) for m in ("test_model", "uni1k_bf", "bpe1k")}


def gpu_same(got, want, what):
    ids, io, sc, ro, sent = _host(*got)
    same((ids, io.view(np.uint64), sc, ro.view(np.uint64)), want, what)
    assert np.array_equal(sent.view(np.uint32), np.repeat(np.arange(len(ro) - 1, dtype=np.uint32), np.diff(ro))), what


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_gpu_nbest_device(model, gpu_sp, corpus):
    sp = gpu_sp[model]
    d = _dev(*corpus)
    for k in (1, 2, 5, 64):
        gpu_same(sp.NBestEncodeDevice(*d, k), sp.NBestPacked(*corpus, k), (model, k))


@pytest.mark.gpu
def test_gpu_csr_shapes(gpu_sp):
    """A few hundred sentences with every shape of section 2 at once: floods of empty results around a non-empty one, a
    6,000-byte sentence (the wide launch; a result longer than a gather chunk), one-word sentences, and the wide A*."""
    sp = gpu_sp["test_model"]
    sents = ([b""] * 150 + [b"hello world"] + [b""] * 150 + [LONG] +
             [(b"w%d" % i) for i in range(300)] + [WIDE, b"a"])
    text, offs = packed(sents)
    d = _dev(text, offs)
    for k in (2, 65):
        gpu_same(sp.NBestEncodeDevice(*d, k), sp.NBestPacked(text, offs, k), k)
    e = _dev(*packed([]))
    got = _host(*sp.NBestEncodeDevice(*e, 5))
    assert [len(x) for x in got] == [0, 1, 0, 1, 0] and got[1][0] == 0 and got[3][0] == 0


@pytest.mark.gpu
def test_gpu_sample_and_score_device(gpu_sp, botchan):
    sp = gpu_sp["test_model"]
    text, offs = packed(botchan[:300] + [b"a", b"", b" "])
    d = _dev(text, offs)
    for wor, best, num, seed in ((False, False, 4, 11), (True, False, 3, 7), (True, True, 3, 7)):
        want = sp.SampleEncodeAndScorePacked(text, offs, num, 0.5, wor, best, seed)
        gpu_same(sp.SampleEncodeAndScoreDevice(*d, num, 0.5, wor, best, seed), want, (wor, best, num))


@pytest.mark.gpu
def test_gpu_sample_device(gpu_sp, botchan):
    sents = botchan[:300] + [b"", b"hello world"]
    text, offs = packed(sents)
    d = _dev(text, offs)

    def dev_rows(sp, *a, **kw):
        ids, io, total = sp.SampleEncodeDevice(*d, *a, **kw)
        ids, io = _host(ids, io)
        assert int(io[-1]) == total
        return rows(ids, io)
    for model, cases in (("test_model", ((-1, 0.1, 0), (-1, 0.5, 5), (0, 0.1, 1), (1, 0.1, 1))), ("uni1k_bf", ((-1, 0.2, 3),)),
                         ("bpe1k", ((-1, 0.0, 2), (-1, 0.1, 2), (-1, 1.0, 2)))):
        sp = gpu_sp[model]
        for nbest_size, alpha, seed in cases:
            assert dev_rows(sp, nbest_size, alpha, seed) == rows(*sp.SampleEncodePacked(text, offs, nbest_size, alpha, seed)), \
                (model, nbest_size, alpha)
    # index_base, through the tensors: rows [k, n) on their own
    sp = gpu_sp["test_model"]
    whole = dev_rows(sp, -1, 0.3, 77)
    k = 100
    t2, o2 = _dev(*packed(sents[k:]))
    ids, io, _ = sp.SampleEncodeDevice(t2, o2, -1, 0.3, 77, index_base=k)
    assert rows(*_host(ids, io)) == whole[k:]


@pytest.mark.gpu
def test_gpu_sample_nbest_pick(gpu_sp, botchan):
    sp = gpu_sp["test_model"]

    def sample_rows(text, offs, k, alpha, seed):
        ids, io, _ = sp.SampleEncodeDevice(*_dev(text, offs), k, alpha, seed)
        return rows(*_host(ids, io))
    check_sample_nbest_pick(sp.NBestPacked, sample_rows, botchan[:2000])
