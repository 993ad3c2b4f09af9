"""Piece frequency counts on the device (sentencepiece_amd/csrc/kernels_piececount.h) and what stands on them: the id
histogram of the C ABI, spmx_count_file / spmx_write_vocabulary / spmx_load_vocabulary, the processor's LoadVocabulary,
CountIdsDevice, PieceCounts and GenerateVocabulary, and the spmx_encode flags --generate_vocabulary, --vocabulary and
--vocabulary_threshold.

The expected file is built here from ids an already verified path gives (the oracle; for character and word models the
library's own EncodePacked): a Counter over the ids without the UNKNOWN and CONTROL types, sorted by descending count and
then by piece in unsigned byte order.  It must equal tests/golden/vocab_counts.json -- recorded from the compiled
reference's `spm_encode --generate_vocabulary` by scripts/make_vocab_golden.py -- byte for byte, and a live run of that
binary where it is built.  CPU: the device bodies under the wavefront emulator through the C ABI; GPU: the torch-tensor
methods, the file call and the binary."""
import collections
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fixtures
from tests.emulib import EmuLib
from tests.test_decode_file import getline_split, image, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")
JA = os.path.join(fixtures.GOLDEN, "ja_sample.txt")
SPM_ENCODE = os.path.join(ROOT, "oracle", "_ref", "spm_encode")
MODELS = ["test_model", "uni1k_bf", "bpe1k_bf_uds", "bpe1k_llama", "test_ja_model", "char1k", "word1k"]
ORACLE_MODELS = [m for m in MODELS if m not in ("char1k", "word1k")]
GOLDEN = json.load(open(os.path.join(fixtures.GOLDEN, "vocab_counts.json"), encoding="utf-8"))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
# what the kernel strides by (kernels_piececount.h): a wavefront's tile, a full workgroup's step; (api.cc CountIds) the
# least share of a workgroup: the grid grows at its multiples
TILE, GROUP, SHARE = 1024, 16 * 1024, 8192


@pytest.fixture(scope="module")
def emu():
    return EmuLib()


def corpus_lines(model):
    if model == "test_ja_model":
        return getline_split(open(JA, "rb").read())
    return getline_split(open(BOTCHAN, "rb").read())[:600]


def golden_key(model):
    return "ja" if model == "test_ja_model" else "botchan600"


def piece_bytes(sp, i):
    n = sp._lib.spmx_id_to_piece(sp._h, i, None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    sp._lib.spmx_id_to_piece(sp._h, i, buf, n)
    return buf.raw[:n]


def vocab_image(sp, ids):
    """The file of spm_encode --generate_vocabulary for these ids (the specification, restated)."""
    cnt = collections.Counter(np.asarray(ids).tolist())
    rows = [(c, piece_bytes(sp, i)) for i, c in cnt.items() if sp._type(i) not in (2, 3)]
    rows.sort(key=lambda r: (-r[0], r[1]))               # (bytes compare as unsigned bytes)
    return b"".join(p + b"\t%d\n" % c for c, p in rows)


def golden_image(model, key):
    g = GOLDEN[model][key]
    data = "".join(x + "\n" for x in g["lines"]).encode("utf-8", "surrogateescape")
    assert hashlib.md5(data).hexdigest() == g["md5"]
    return data


_IDS = {}


def verified_ids(oracle, sp, model, lines, opts=""):
    """The ids of the lines from a path other tests verify: the oracle, or EncodePacked for a character or word model."""
    key = (model, len(lines), hashlib.md5(b"\n".join(lines)).hexdigest(), opts)
    if key not in _IDS:
        text, offs = packed(lines)
        if model in ORACLE_MODELS:
            o = oracle.load(fixtures.model_blob(model))
            o.set_encode_extra_options(opts)
            _IDS[key] = o.encode_batch(text, offs)[0]
        else:
            _IDS[key] = sp.EncodePacked(text, offs)[0]
    return _IDS[key]


def ref_run(model, paths, extra=()):
    res = subprocess.run([SPM_ENCODE, "--model=" + os.path.join(fixtures.GOLDEN, model + ".model"), "--generate_vocabulary=true",
                          *extra, *paths], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, timeout=300)
    assert res.returncode == 0, res.stderr
    return res.stdout


# --------------------------------------------------------------------------------------- the kernel, emulated ----
def count_cases(V, B):
    """(name, ids): V pieces, B LDS bins (B < V: both the LDS path and the direct path)."""
    rng = np.random.RandomState(5)
    sizes = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257]
    for s in (TILE, SHARE, GROUP, 2 * GROUP, 3 * GROUP):
        sizes += [s - 2, s - 1, s, s + 1, s + 2]
    out = [("T=%d" % t, rng.randint(0, V, size=t)) for t in sizes]
    out.append(("hot7", np.full(5000, 7)))
    out.append(("hotB", np.full(5000, min(B, V - 1))))
    out.append(("edges", np.tile([B - 1, min(B, V - 1), V - 1], 50)))
    out.append(("outside", np.asarray([-1, V, INT_MIN, INT_MAX, 0, V - 1, -1, INT_MAX] * 33)))
    z = rng.zipf(1.3, size=20000) - 1
    out.append(("zipf", np.where(z < V, z, rng.randint(0, V, size=20000))))
    return [(n, np.asarray(a, dtype=np.int32)) for n, a in out]


def bincount(ids, V):
    ids = np.asarray(ids, dtype=np.int64)
    return np.bincount(np.where((ids >= 0) & (ids < V), ids, V), minlength=V + 1).astype(np.uint64)


def emu_count(h, ids, shift, pre):
    """spmx_count_ids_device on ids placed `shift` bytes off a 16-byte boundary, the counts inside a 0xCD-filled buffer
    (pre-filled with `pre`): returns the counts; the neighbours must stay intact."""
    V = len(pre) - 1
    raw = np.zeros(len(ids) + 16, dtype=np.int32)
    at = ((shift - raw.ctypes.data) & 15) // 4
    assert (raw.ctypes.data + 4 * at) % 16 == shift
    raw[at:at + len(ids)] = ids
    dst = np.full(V + 1 + 16, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
    dst[8:8 + V + 1] = pre
    rc = h.lib.spmx_count_ids_device(h.sp._h, raw.ctypes.data + 4 * at, len(ids), dst.ctypes.data + 64, V + 1, None)
    assert rc == 0, h.lib.spmx_last_error(None)
    assert (dst[:8] == 0xCDCDCDCDCDCDCDCD).all() and (dst[8 + V + 1:] == 0xCDCDCDCDCDCDCDCD).all(), "write outside the counts"
    return dst[8:8 + V + 1].copy()


@pytest.mark.parametrize("cus", [1, 3])
@pytest.mark.parametrize("bins", [None, 256])
def test_count_kernel_emulated(emu, cus, bins, monkeypatch):
    if bins:
        monkeypatch.setenv("SPMX_COUNT_LDS_BINS", str(bins))
    h = emu.load(fixtures.model_blob("test_model"), cus=cus)
    V = h.sp.GetPieceSize()
    assert V == 1000
    B = min(bins or 32768, V)
    pre = (np.arange(V + 1, dtype=np.uint64) * 3 + 1)
    for name, ids in count_cases(V, B):
        want = bincount(ids, V)
        for shift in (0, 4, 8, 12):
            got = emu_count(h, ids, shift, pre)
            assert np.array_equal(got, pre + want), (name, shift)
    # a second call adds to the first
    ids = count_cases(V, B)[-1][1]
    once = emu_count(h, ids, 4, np.zeros(V + 1, dtype=np.uint64))
    twice = emu_count(h, ids[:777], 12, once)
    assert np.array_equal(twice, bincount(ids, V) + bincount(ids[:777], V))


def test_count_kernel_capacity(emu):
    h = emu.load(fixtures.model_blob("test_model"))
    V = h.sp.GetPieceSize()
    ids = np.arange(100, dtype=np.int32)
    dst = np.full(V + 8, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
    assert h.lib.spmx_count_ids_device(h.sp._h, ids.ctypes.data, len(ids), dst.ctypes.data, V, None) == 8
    assert (dst == 0xCDCDCDCDCDCDCDCD).all()
    assert h.lib.spmx_count_ids_device(h.sp._h, ids.ctypes.data, 0, dst.ctypes.data, V + 1, None) == 0
    assert (dst == 0xCDCDCDCDCDCDCDCD).all()


# ---------------------------------------------------------------------------------------------- the file call ----
def write_lines(path, lines, last_newline=True):
    data = image(lines)
    with open(path, "wb") as f:
        f.write(data if last_newline else data[:-1])
    return str(path)


@pytest.mark.parametrize("model", MODELS)
def test_generate_vocabulary_emulated(model, emu, oracle, tmp_path, monkeypatch):
    sp = emu.load(fixtures.model_blob(model), cus=3, classes=None).sp
    lines = corpus_lines(model)
    src, out = write_lines(tmp_path / "in.txt", lines), str(tmp_path / "vocab.tsv")
    ids = verified_ids(oracle, sp, model, lines)
    want = vocab_image(sp, ids)
    assert want == golden_image(model, golden_key(model)), "the restated specification against the compiled reference"
    ns, ni, nl = sp.GenerateVocabulary(src, out)
    assert (ns, ni, nl) == (len(lines), len(ids), want.count(b"\n"))
    assert open(out, "rb").read() == want
    if os.path.exists(SPM_ENCODE):
        assert ref_run(model, [src]) == want
    # bos / eos are control pieces: the same file
    sp.SetEncodeExtraOptions("bos:eos")
    try:
        assert sp.GenerateVocabulary(src, out) == (len(lines), len(ids) + 2 * len(lines), nl)
        assert open(out, "rb").read() == want
    finally:
        sp.SetEncodeExtraOptions("")
    # many chunks, four workers, one shared histogram
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    assert sp.GenerateVocabulary(src, out) == (len(lines), len(ids), nl)
    assert open(out, "rb").read() == want
    monkeypatch.delenv("SPMX_FILE_CHUNK")
    # the raw histogram of the file call, unknown and control ids included
    counts = np.zeros(sp.GetPieceSize() + 1, dtype=np.uint64)
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert sp._lib.spmx_count_file(sp._h, src.encode(), counts.ctypes.data, C.byref(a), C.byref(b)) == 0
    assert np.array_equal(counts, bincount(ids, sp.GetPieceSize())) and counts[-1] == 0


def test_generate_vocabulary_variations(emu, oracle, tmp_path):
    sp = emu.load(fixtures.model_blob("test_model"), cus=3, classes=None).sp
    out = str(tmp_path / "vocab.tsv")
    bot, ja = corpus_lines("test_model"), getline_split(open(JA, "rb").read())
    # two input files: the counts of their concatenation
    a, b = write_lines(tmp_path / "a.txt", bot[:250]), write_lines(tmp_path / "b.txt", bot[250:] + ja[:40])
    both = bot + ja[:40]
    ids = verified_ids(oracle, sp, "test_model", both)
    ns, ni, nl = sp.GenerateVocabulary([a, b], out)
    assert (ns, ni) == (len(both), len(ids))
    assert open(out, "rb").read() == vocab_image(sp, ids)
    if os.path.exists(SPM_ENCODE):
        assert ref_run("test_model", [a, b]) == open(out, "rb").read()
    # an empty file: an empty output
    empty = str(tmp_path / "empty.txt")
    open(empty, "wb").close()
    assert sp.GenerateVocabulary(empty, out) == (0, 0, 0)
    assert open(out, "rb").read() == b""
    # almost everything unknown: nothing unknown in the file
    ids = verified_ids(oracle, sp, "test_model", ja)
    assert (ids == sp.unk_id()).sum() > len(ids) // 4
    assert sp.GenerateVocabulary(JA, out)[:2] == (len(ja), len(ids))
    got = open(out, "rb").read()
    assert got == vocab_image(sp, ids) == golden_image("test_model", "ja")
    assert piece_bytes(sp, sp.unk_id()) + b"\t" not in got
    # a last line without '\n'
    src = write_lines(tmp_path / "nonl.txt", bot[:50], last_newline=False)
    assert sp.GenerateVocabulary(src, out)[0] == 50
    assert open(out, "rb").read() == vocab_image(sp, verified_ids(oracle, sp, "test_model", bot[:50]))
    # a missing input: as spmx_encode_file
    counts = np.zeros(sp.GetPieceSize() + 1, dtype=np.uint64)
    x, y = C.c_uint64(0), C.c_uint64(0)
    assert sp._lib.spmx_count_file(sp._h, str(tmp_path / "nothing").encode(), counts.ctypes.data, C.byref(x), C.byref(y)) == 5
    assert "No such file or directory" in sp._lib.spmx_last_error(sp._h).decode()


def test_tie_order_is_by_unsigned_bytes(emu, tmp_path):
    """Equal counts: pieces that differ first at a byte >= 0x80 against an ASCII byte come out in unsigned-byte order (a
    signed char comparison would put the UTF-8 piece first)."""
    sp = emu.load(fixtures.model_blob("test_model")).sp
    V = sp.GetPieceSize()
    pieces = {i: piece_bytes(sp, i) for i in range(V) if sp._type(i) == 1}
    hi = [i for i, p in pieces.items() if p[0] >= 0x80][:6]
    lo = [i for i, p in pieces.items() if p[0] < 0x80][:6]
    assert len(hi) == 6 and len(lo) == 6
    counts = np.zeros(V + 1, dtype=np.uint64)
    counts[hi + lo] = 9
    counts[lo[0]] = 10
    counts[sp.unk_id()] = 99                               # not written
    counts[V] = 5
    out = str(tmp_path / "v.tsv")
    nl = C.c_uint64(0)
    assert sp._lib.spmx_write_vocabulary(sp._h, counts.ctypes.data, out.encode(), C.byref(nl)) == 0
    rows = [r.split(b"\t") for r in open(out, "rb").read().split(b"\n")[:-1]]
    assert nl.value == len(rows) == 12
    assert rows[0] == [pieces[lo[0]], b"10"]
    tied = [r[0] for r in rows[1:]]
    assert tied == sorted(pieces[i] for i in hi + lo[1:])
    assert tied[0][0] < 0x80 <= tied[-1][0]


# ------------------------------------------------------------------------------------------------ round trip ----
def vocab_rows(path):
    return [(r.split(b"\t")[0], int(r.split(b"\t")[1])) for r in open(path, "rb").read().split(b"\n")[:-1]]


@pytest.mark.parametrize("model", ["test_model", "bpe1k_bf_uds"])
def test_load_vocabulary_round_trip(model, emu, tmp_path):
    sp = emu.load(fixtures.model_blob(model), cus=3, classes=None).sp
    lines = corpus_lines(model)[:200]
    src, voc = write_lines(tmp_path / "in.txt", lines), str(tmp_path / "vocab.tsv")
    sp.GenerateVocabulary(src, voc)
    text, offs = packed(lines)
    plain = sp.EncodePacked(text, offs)[0]
    try:
        for k in (1, 2, 50):
            sp.LoadVocabulary(voc, k)
            got = sp.EncodePacked(text, offs)[0]
            sp.SetVocabulary([p for p, c in vocab_rows(voc) if c >= k])
            assert np.array_equal(got, sp.EncodePacked(text, offs)[0]), k
            if k == 50:
                assert not np.array_equal(got, plain)
            if os.path.exists(SPM_ENCODE):
                res = subprocess.run([SPM_ENCODE, "--model=" + os.path.join(fixtures.GOLDEN, model + ".model"), "--vocabulary=" + voc,
                                      "--vocabulary_threshold=%d" % k, "--output_format=id", src], stdout=subprocess.PIPE,
                                     stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, timeout=300)
                assert res.returncode == 0, res.stderr
                assert [int(t) for t in res.stdout.split()] == got.tolist(), k
        sp.ResetVocabulary()
        assert np.array_equal(sp.EncodePacked(text, offs)[0], plain)
    finally:
        sp.ResetVocabulary()


def test_load_vocabulary_errors(emu, tmp_path):
    sp = emu.load(fixtures.model_blob("test_model")).sp
    lib = sp._lib
    missing = str(tmp_path / "nothing.tsv")
    assert lib.spmx_load_vocabulary(sp._h, missing.encode(), 1) == 5
    assert lib.spmx_last_error(sp._h).decode() == '"%s": No such file or directory' % missing
    bad = str(tmp_path / "bad.tsv")
    with open(bad, "wb") as f:
        f.write(b"a\t3\n\t4\n")
    assert lib.spmx_load_vocabulary(sp._h, bad.encode(), 1) == 13
    assert lib.spmx_last_error(sp._h).decode() == "LoadVocabulary: an empty token"
    with open(bad, "wb") as f:
        f.write(b"a\tx\n")
    assert lib.spmx_load_vocabulary(sp._h, bad.encode(), 1) == 13
    assert lib.spmx_last_error(sp._h).decode() == "Could not parse the frequency"
    with open(bad, "wb") as f:
        f.write(b"a\n\xe2\x96\x81the\t7\r\nb\t2")                    # no second column counts as 1
    assert lib.spmx_load_vocabulary(sp._h, bad.encode(), 2) == 0
    assert sp.IsUnused(sp.PieceToId("▁of")) and not sp.IsUnused(sp.PieceToId("▁the"))
    sp.ResetVocabulary()
    for model in ("char1k", "word1k"):                               # the reference's status for SetVocabulary
        cw = emu.load(fixtures.model_blob(model)).sp
        with pytest.raises(RuntimeError, match="Vocabulary constraint is only enabled in subword units"):
            cw.LoadVocabulary(bad, 1)


def test_count_kernel_uses_no_scratch():
    from tests.test_kernel_resources import REPORT, _report
    if not os.path.exists(REPORT):
        pytest.skip("no resource report next to the library (csrc/Makefile writes it with kernels.o)")
    rep = _report()
    names = [n for n in rep if "CountIdsKernel" in n]
    assert len(names) == 1, names
    r = rep[names[0]]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r


# -------------------------------------------------------------------------------------------------------- GPU ----
def _gpu_sp(model):
    from sentencepiece_amd.processor import SentencePieceProcessor
    return SentencePieceProcessor(model_proto=fixtures.model_blob(model), device=0)


def _gpu_count_checks(sp):
    """CountIdsDevice against torch.bincount: the cases of the issue, on the processor's model."""
    import torch
    V = sp.GetPieceSize()
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(9)

    def want(t):
        t = t.to(torch.int64)
        return torch.bincount(torch.where((t >= 0) & (t < V), t, torch.full_like(t, V)), minlength=V + 1)

    z = rng.zipf(1.3, size=1000003) - 1
    zipf = torch.from_numpy(np.where(z < V, z, rng.randint(0, V, size=len(z))).astype(np.int32)).to(dev)
    cases = {"empty": torch.zeros(0, dtype=torch.int32, device=dev),
             "one": torch.full((1,), V - 1, dtype=torch.int32, device=dev),
             "zipf": zipf,
             "hot": torch.full((1000000,), 7, dtype=torch.int32, device=dev),
             "off_by_one": zipf[1:200000],
             "outside": torch.tensor([-1, V, INT_MIN, INT_MAX, 0, V - 1] * 1000, dtype=torch.int32, device=dev)}
    for name, t in cases.items():
        got = sp.CountIdsDevice(t)
        assert got.dtype == torch.int64 and got.numel() == V + 1
        assert torch.equal(got, want(t)), name
    assert cases["off_by_one"].data_ptr() % 16 == 4
    acc = sp.CountIdsDevice(cases["zipf"])
    assert sp.CountIdsDevice(cases["hot"], acc) is acc                      # two calls accumulate
    assert torch.equal(acc, want(cases["zipf"]) + want(cases["hot"]))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = sp.CountIdsDevice(cases["zipf"])
    s.synchronize()
    assert torch.equal(got, want(cases["zipf"]))
    with pytest.raises(RuntimeError, match="counts_capacity"):
        sp.CountIdsDevice(cases["one"], torch.zeros(V, dtype=torch.int64, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["test_model", "uni32k"])
def test_count_ids_device_gpu(model):
    _gpu_count_checks(_gpu_sp(model))


@pytest.mark.gpu
def test_count_ids_device_gpu_small_bins():
    """SPMX_COUNT_LDS_BINS=256 in a fresh process: the LDS path and the direct path on a 1k-piece model."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_generate_vocabulary as t\n"
            "t._gpu_count_checks(t._gpu_sp('test_model'))\nprint('counted')\n" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPMX_COUNT_LDS_BINS="256"), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0 and b"counted" in res.stdout, res.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_generate_vocabulary_gpu(model, oracle, tmp_path):
    sp = _gpu_sp(model)
    lines = getline_split(open(BOTCHAN, "rb").read())[:600]
    src, out = write_lines(tmp_path / "in.txt", lines), str(tmp_path / "vocab.tsv")
    ids = verified_ids(oracle, sp, model, lines)
    want = vocab_image(sp, ids)
    assert want == golden_image(model, "botchan600")
    V = sp.GetPieceSize()
    counts = sp.PieceCounts(lines)
    assert counts.dtype == np.int64 and np.array_equal(counts.astype(np.uint64), bincount(ids, V))
    assert sp.GenerateVocabulary(src, out) == (len(lines), len(ids), want.count(b"\n"))
    assert open(out, "rb").read() == want
    if os.path.exists(SPM_ENCODE):
        assert ref_run(model, [src]) == want


@pytest.mark.gpu
def test_spmx_encode_vocabulary_flags_gpu(oracle, tmp_path):
    exe = os.path.join(ROOT, "sentencepiece_amd", "spmx_encode")
    mdl = "--model=" + os.path.join(fixtures.GOLDEN, "test_model.model")
    sp = _gpu_sp("test_model")
    lines = getline_split(open(BOTCHAN, "rb").read())[:600]
    src = write_lines(tmp_path / "in.txt", lines)
    a, b = write_lines(tmp_path / "a.txt", lines[:250]), write_lines(tmp_path / "b.txt", lines[250:])
    want = vocab_image(sp, verified_ids(oracle, sp, "test_model", lines))
    assert want == golden_image("test_model", "botchan600")

    def run(*args):
        return subprocess.run([exe, mdl, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, timeout=120)
    for args in (["--generate_vocabulary", "--input=" + src], ["--generate_vocabulary=true", a, b],
                 ["--generate_vocabulary", "--extra_options=bos:eos", "--output_format=piece", src]):
        res = run(*args)
        assert res.returncode == 0, res.stderr
        assert res.stdout == want, args
    # --vocabulary / --vocabulary_threshold against the Python path
    voc = str(tmp_path / "vocab.tsv")
    with open(voc, "wb") as f:
        f.write(want)
    res = run("--vocabulary=" + voc, "--vocabulary_threshold=50", "--output_format=id", "--generate_vocabulary=false", src)
    assert res.returncode == 0, res.stderr
    sp.LoadVocabulary(voc, 50)
    ids_out = str(tmp_path / "ids.txt")
    sp.EncodeFile(src, ids_out, "id")
    assert res.stdout == open(ids_out, "rb").read()
    sp.ResetVocabulary()
    sp.EncodeFile(src, ids_out, "id")
    assert res.stdout != open(ids_out, "rb").read()
    # an unknown flag, and a second positional input outside generate mode: the usage status
    assert run("--no_such_flag=1", src).returncode == 2
    assert run("--output_format=id", a, b).returncode == 2
