"""The output side of spm_encode on the device (sentencepiece_amd/csrc/kernels_tokentext.h): the id-line formatter, the
piece writer in its packed and its lines form, and what stands on them -- spmx_encode_file's "piece" and "id" formats,
EncodePiecesPacked / EncodeAsPieces, the spmx_encode command line.

Expected pieces come from the oracle's pieces form (tests/pieceslib.encode_pieces); where the compiled reference is built
it is asserted equal.  The oracle does not restate character and word models: their expectation is
tests/golden/piece_lines.json, recorded from the compiled reference's spm_encode by scripts/make_piece_lines_golden.py.
CPU: the device bodies under the wavefront emulator through the C ABI; GPU: the torch-tensor methods and the binary."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import fixtures, refshim
from tests.emulib import EmuLib
from tests.test_decode_file import emu_parse, getline_split, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")
MODELS = ["test_model", "uni1k_bf", "bpe1k_bf_uds", "bpe1k_llama", "test_ja_model", "char1k", "word1k"]
ORACLE_MODELS = [m for m in MODELS if m not in ("char1k", "word1k")]
OPTS = ["", "bos:eos", "reverse", "reverse:bos:eos", "unk_piece"]
# md5 of what the compiled reference's `spm_encode --model=test_model.model botchan.txt` writes with no format flag (the
# piece format, src/spm_encode_main.cc:32): recorded by scripts/make_piece_lines_golden.py, also in piece_lines.json
BOTCHAN_PIECES_MD5 = "da4b2c136bc7875bfaa260611b600ab2"
BOTCHAN_IDS_MD5 = "ff197d02d69c7695fccfec3bac27bf7a"
GOLDEN = json.load(open(os.path.join(fixtures.GOLDEN, "piece_lines.json"), encoding="utf-8"))
INT_MIN = -2 ** 31


@pytest.fixture(scope="module")
def emu():
    return EmuLib()


# ------------------------------------------------------------------------------------------------- id formatter ----
def id_cases():
    edge = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
            100000000, 999999999, 1000000000, 2 ** 31 - 1]
    edge = edge + [-v for v in edge if v] + [INT_MIN]
    rng = np.random.RandomState(11)
    out = [[], [[]], [[]] * 5, [[]] * 2000, [[7]], [edge], [[v] for v in edge], [[v, v] for v in edge]]
    out.append([list(range(5000))])                                         # one line that crosses chunks
    out.append([[1, 2], [], [3]])
    out.append([[1, 2], [3], []])                                           # a last line that is empty
    out.append([[]] * 700 + [[5]] + [[]] * 700)
    out.append([rng.randint(INT_MIN, 2 ** 31 - 1, size=rng.choice((0, 0, 1, 2, 7, 40))).tolist() for _ in range(600)])
    out.append([rng.randint(0, 32000, size=rng.choice((0, 1, 30, 300))).tolist() for _ in range(400)])
    return out


def csr(rows):
    ids = np.asarray([t for r in rows for t in r], dtype=np.int32)
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        offs[1:] = np.cumsum([len(r) for r in rows])
    return ids, offs


def id_image(rows):
    return b"".join(b" ".join(b"%d" % t for t in r) + b"\n" for r in rows)


def placed(call, want_len, shift):
    """Runs call(ptr, capacity) -> (rc, need) on a destination `shift` bytes off a 16-byte boundary inside a 0xCD-filled
    buffer; the neighbours must stay intact."""
    raw = np.full(want_len + 96, 0xCD, dtype=np.uint8)
    at = 32 + ((shift - raw.ctypes.data - 32) & 15)
    assert (raw.ctypes.data + at) % 16 == shift
    rc, need = call(raw.ctypes.data + at, want_len)
    assert rc == 0 and need == want_len, (rc, need, want_len)
    assert (raw[:at] == 0xCD).all() and (raw[at + want_len:] == 0xCD).all(), "write outside the image"
    return raw[at:at + want_len].tobytes()


def emu_format_ids(h, rows, shift=0):
    ids, offs = csr(rows)
    ids = np.concatenate([ids, np.zeros(1, dtype=np.int32)])         # (a valid pointer for no ids)
    need = C.c_uint64(0)

    def call(ptr, cap):
        rc = h.lib.spmx_format_id_lines_device(h.sp._h, ids.ctypes.data, offs.ctypes.data, len(rows), ptr, cap, None, C.byref(need))
        return rc, need.value
    want = len(id_image(rows))
    rc, got = call(None, 0)                                          # the capacity protocol: the exact need
    assert got == want and rc == (8 if want else 0)
    if want:
        scratch = np.full(want + 16, 0xCD, dtype=np.uint8)
        assert call(scratch.ctypes.data, want - 1) == (8, want)      # one byte short
        assert (scratch == 0xCD).all()
    return placed(call, want, shift)


@pytest.mark.parametrize("cus", [1, 3])
def test_id_formatter_emulated(emu, cus):
    h = emu.load(fixtures.model_blob("test_model"), cus=cus)
    for rows in id_cases():
        for shift in (0, 5):
            assert emu_format_ids(h, rows, shift) == id_image(rows), (len(rows), shift)


def test_id_formatter_round_trip(emu):
    """parse(format(csr)) == csr: the formatter is the parser's inverse on every int32."""
    h = emu.load(fixtures.model_blob("test_model"), cus=3)
    for rows in id_cases():
        if not rows:
            continue
        ids, offs = emu_parse(h, emu_format_ids(h, rows))
        want_ids, want_offs = csr(rows)
        assert np.array_equal(ids, want_ids) and np.array_equal(offs, want_offs), len(rows)


# ------------------------------------------------------------------------------------------------------- pieces ----
def crafted():
    return [b"", b"   ", "abc กขฃxyz ก".encode(), "กข \U0001F600\U0001F601 tail".encode(),
            b"ab\xff\xfecd \xe3\x81 x\x80", b"the quick brown fox " * 2048, "㎿㌖ ﷺ ﬃ".encode(), b"Hello world."]


def sources(model):
    """[(name, lines)]: botchan (its first 300 lines but for test_model), ja_sample.txt, the crafted sentences."""
    bot = getline_split(open(BOTCHAN, "rb").read())
    ja = getline_split(open(os.path.join(fixtures.GOLDEN, "ja_sample.txt"), "rb").read())
    return [("botchan", bot if model == "test_model" else bot[:300]), ("ja", ja), ("crafted", crafted())]


def rows_of(blob, poffs, io):
    poffs, io = np.asarray(poffs).astype(np.int64), np.asarray(io).astype(np.int64)
    return [[blob[poffs[k]:poffs[k + 1]] for k in range(io[i], io[i + 1])] for i in range(len(io) - 1)]


def piece_image(rows):
    return b"".join(b" ".join(r) + b"\n" for r in rows)


def emu_piece_lines(h, text, offs, shift=0, want_len=None):
    """want_len: the image's size where the caller knows it (no call to ask for it: every call encodes the batch)."""
    text = np.concatenate([np.ascontiguousarray(text, dtype=np.uint8), np.zeros(32, dtype=np.uint8)])
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(offs) - 1
    ni, need = C.c_uint64(0), C.c_uint64(0)

    def call(ptr, cap):
        rc = h.lib.spmx_encode_piece_lines_device(h.sp._h, text.ctypes.data, int(offs[n]), offs.ctypes.data, n, ptr, cap, None,
                                                  C.byref(ni), C.byref(need))
        return rc, need.value
    if want_len is None:
        rc, want_len = call(None, 0)
        assert rc == (8 if want_len else 0), h.lib.spmx_last_error(None)
        if want_len:
            assert call(np.zeros(want_len, dtype=np.uint8).ctypes.data, want_len - 1) == (8, want_len)
    return placed(call, want_len, shift), ni.value


class Expect:
    """Per (model, options, source): (ids, id_offsets, piece blob, piece offsets) from the oracle, equal to the compiled
    reference's where that is built; a character or word model: the compiled reference's, or None without it."""

    def __init__(self, oracle):
        self.oracle, self.made = oracle, {}
        self.ref = refshim.RefLib() if refshim.available() else None

    def get(self, model, opts, name, lines):
        key = (model, opts, name)
        if key not in self.made:
            blob = fixtures.model_blob(model)
            text, offs = packed(lines)
            want = None
            if model in ORACLE_MODELS:
                o = self.oracle.load(blob)
                o.set_encode_extra_options(opts)
                ids, _, _, io, pblob, poffs = o.encode_pieces(text, offs)
                want = (ids, io, pblob, poffs)
            if self.ref is not None:
                r = self.ref.load(blob)
                r.set_encode_extra_options(opts)
                ids, _, _, io, pblob, poffs = r.encode_pieces(text, offs)
                if want is not None:
                    assert np.array_equal(want[0], ids) and want[2] == pblob and np.array_equal(want[3], poffs), key
                want = (ids, io, pblob, poffs)
            self.made[key] = want
        return self.made[key]


@pytest.fixture(scope="module")
def expect(oracle):
    return Expect(oracle)


@pytest.mark.parametrize("model", MODELS)
def test_pieces_packed_and_lines_emulated(model, emu, expect):
    h = emu.load(fixtures.model_blob(model), cus=3, classes=None)
    try:
        for opts in OPTS:
            h.set_encode_extra_options(opts)
            for name, lines in sources(model):
                text, offs = packed(lines)
                ids, io, pb, po = h.sp.EncodePiecesPacked(text, offs)
                rows = rows_of(pb.tobytes(), po, io)
                want = expect.get(model, opts, name + str(len(lines)), lines)
                what = (model, opts, name)
                if want is not None:
                    assert np.array_equal(ids, want[0]) and np.array_equal(io, want[1]), what
                    assert pb.tobytes() == want[2], what
                    assert np.array_equal(po, want[3]), what
                probe = name == "crafted" and not opts           # the capacity protocol once per model: every call encodes
                image, n_ids = emu_piece_lines(h, text, offs, shift=5 if name == "crafted" else 0,
                                               want_len=None if probe else len(piece_image(rows)))
                assert n_ids == len(ids), what
                assert image == piece_image(rows), what
                if not opts and name == "botchan" and len(lines) == 300:
                    assert hashlib.md5(image).hexdigest() == GOLDEN["models"][model]["botchan300_md5"], what
    finally:
        h.set_encode_extra_options("")


@pytest.mark.parametrize("model", MODELS)
def test_piece_lines_literal_golden(model, emu):
    """The recorded lines of the compiled reference's spm_encode, every model (char1k and word1k have no other oracle)."""
    sp = emu.load(fixtures.model_blob(model), classes=None).sp
    lines = [x.encode("utf-8") for x in GOLDEN["lines"]]
    got = sp.EncodeAsPieces(lines)
    assert [" ".join(r) for r in got] == GOLDEN["models"][model]["pieces"]
    ids, io, pb, po = sp.EncodePiecesPacked(*packed(lines))
    assert piece_image(rows_of(pb.tobytes(), po, io)).decode("utf-8") == "".join(x + "\n" for x in GOLDEN["models"][model]["pieces"])


def test_pieces_capacity_protocol(emu):
    h = emu.load(fixtures.model_blob("test_model"))
    text, offs = packed([b"Hello world.", b"", b"I saw a girl with a telescope."])
    text = np.concatenate([text, np.zeros(32, dtype=np.uint8)])
    n = len(offs) - 1
    ti, tb = C.c_uint64(0), C.c_uint64(0)
    io = np.zeros(n + 1, dtype=np.uint64)

    def call(ids, icap, pb, pcap, po):
        return h.lib.spmx_encode_batch_pieces_device(h.sp._h, text.ctypes.data, int(offs[n]), offs.ctypes.data, n,
                                                     ids.ctypes.data if ids is not None else None, icap, io.ctypes.data,
                                                     pb.ctypes.data if pb is not None else None, pcap,
                                                     po.ctypes.data if po is not None else None, None, C.byref(ti), C.byref(tb))
    assert call(None, 0, None, 0, None) == 8 and ti.value > 0
    total = ti.value
    ids = np.zeros(total, dtype=np.int32)
    po = np.full(total + 2, 0xCDCDCDCD, dtype=np.uint64)
    assert call(ids, total, None, 0, po) == 8 and ti.value == total and tb.value > 0
    nbytes = tb.value
    pb = np.full(nbytes + 16, 0xCD, dtype=np.uint8)
    assert call(ids, total, pb, nbytes - 1, po) == 8 and tb.value == nbytes and (pb == 0xCD).all()
    assert call(ids, total, pb, nbytes, po) == 0, h.lib.spmx_last_error(None)
    assert (pb[nbytes:] == 0xCD).all() and po[total] == nbytes and po[total + 1] == 0xCDCDCDCD
    want = h.sp.EncodePiecesPacked(text[:int(offs[n])], offs)
    assert np.array_equal(ids, want[0]) and pb[:nbytes].tobytes() == want[2].tobytes() and np.array_equal(po[:total + 1], want[3])
    # one id short: the exact need again, and at that need the same result
    ids2 = np.zeros(total, dtype=np.int32)
    assert call(ids2, total - 1, pb, nbytes, po) == 8 and ti.value == total
    assert call(ids2, total, pb, nbytes, po) == 0 and np.array_equal(ids2, want[0]) and pb[:nbytes].tobytes() == want[2].tobytes()
    # the way back, spmx_decode_batch_device: one byte short, then at the reported need
    dids = np.concatenate([ids, np.zeros(16, dtype=np.int32)])
    text_want, toffs_want = h.sp.DecodePacked(ids, io)
    assert text_want.tobytes() == b"Hello world.I saw a girl with a telescope." and toffs_want.tolist() == [0, 12, 12, 42]
    need, to = C.c_uint64(0), np.zeros(n + 1, dtype=np.uint64)
    buf = np.full(len(text_want) + 16, 0xCD, dtype=np.uint8)

    def decode(cap):
        return h.lib.spmx_decode_batch_device(h.sp._h, dids.ctypes.data, io.ctypes.data, n, buf.ctypes.data, cap, to.ctypes.data, None,
                                              C.byref(need))
    assert decode(len(text_want) - 1) == 8 and need.value == len(text_want)
    assert decode(need.value) == 0, h.lib.spmx_last_error(None)
    assert buf[:need.value].tobytes() == text_want.tobytes() and (buf[need.value:] == 0xCD).all() and np.array_equal(to, toffs_want)
    # n == 0: an empty result
    assert h.lib.spmx_encode_batch_pieces_device(h.sp._h, None, 0, offs.ctypes.data, 0, None, 0, io.ctypes.data, None, 0, po.ctypes.data,
                                                 None, C.byref(ti), C.byref(tb)) == 0
    assert (ti.value, tb.value, po[0]) == (0, 0, 0)
    e = h.sp.EncodePiecesPacked(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert [len(x) for x in e] == [0, 1, 0, 1]


# ---------------------------------------------------------------------------------------------------- file call ----
@pytest.fixture(scope="module")
def botchan_pieces(oracle):
    """The piece-line image of botchan under test_model from the oracle."""
    o = oracle.load(fixtures.model_blob("test_model"))
    ids, _, _, io, pblob, poffs = o.encode_pieces(*packed(getline_split(open(BOTCHAN, "rb").read())))
    return piece_image(rows_of(pblob, poffs, io)), len(ids)


def test_encode_file_piece(emu, botchan_pieces, tmp_path, monkeypatch):
    """EncodeFile(botchan, out, "piece") is the oracle's image; its md5 is BOTCHAN_PIECES_MD5, the digest of the compiled
    reference's `spm_encode --model=tests/golden/test_model.model tests/golden/botchan.txt` (no format flag), obtained
    with scripts/make_piece_lines_golden.py."""
    want, n_ids = botchan_pieces
    assert hashlib.md5(want).hexdigest() == BOTCHAN_PIECES_MD5 == GOLDEN["models"]["test_model"]["botchan_md5"]
    sp = emu.load(fixtures.model_blob("test_model"), classes=None).sp
    out = str(tmp_path / "pieces.txt")
    for chunk in (None, "4096"):
        if chunk:
            monkeypatch.setenv("SPMX_FILE_CHUNK", chunk)
        assert sp.EncodeFile(BOTCHAN, out, "piece") == (4288, n_ids)
        got = open(out, "rb").read()
        assert got == want, chunk
        assert hashlib.md5(got).hexdigest() == BOTCHAN_PIECES_MD5
    # format "id": the bytes tests/test_host.py pins, now written on the device, and on the host loop
    ids_out = str(tmp_path / "ids.txt")
    for host in (False, True):
        if host:
            monkeypatch.setenv("SPMX_ID_HOST_FORMAT", "1")
        assert sp.EncodeFile(BOTCHAN, ids_out, "id") == (4288, n_ids)
        assert hashlib.md5(open(ids_out, "rb").read()).hexdigest() == BOTCHAN_IDS_MD5, host
    monkeypatch.delenv("SPMX_ID_HOST_FORMAT")
    # the round trip through DecodeFile: the piece file decodes to what the id file decodes to.  An unknown token's piece
    # shows its characters, and Decode(pieces) gives a piece outside the vocabulary back as it is where Decode(ids) writes
    # the unknown surface (spmx_decode_batch_pieces; the reference does the same): the files agree on every line without
    # an unknown id, and on every line under the decode option `unk`, which maps such pieces to the unknown piece first.
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    assert sp.DecodeFile(out, a, "piece") == sp.DecodeFile(ids_out, b, "id") == (4288, n_ids)
    unk = b"%d" % sp.unk_id()
    known = [unk not in row.split(b" ") for row in open(ids_out, "rb").read().split(b"\n")[:-1]]
    la, lb = open(a, "rb").read().split(b"\n"), open(b, "rb").read().split(b"\n")
    assert len(la) == len(lb) == 4289 and 4000 < sum(known) < 4288
    assert all(x == y for x, y, k in zip(la, lb, known) if k)
    sp.SetDecodeExtraOptions("unk")
    try:
        assert sp.DecodeFile(out, a, "piece") == sp.DecodeFile(ids_out, b, "id") == (4288, n_ids)
        assert open(a, "rb").read() == open(b, "rb").read()
    finally:
        sp.SetDecodeExtraOptions("")


def test_encode_file_piece_edges(emu, tmp_path):
    sp = emu.load(fixtures.model_blob("test_model")).sp
    src, out = str(tmp_path / "empty.txt"), str(tmp_path / "out.txt")
    open(src, "wb").close()
    for fmt in ("piece", "id"):
        assert sp.EncodeFile(src, out, fmt) == (0, 0)
        assert open(out, "rb").read() == b""
    ns, ni = C.c_uint64(0), C.c_uint64(0)
    rc = sp._lib.spmx_encode_file(sp._h, str(tmp_path / "nothing").encode(), out.encode(), b"piece", C.byref(ns), C.byref(ni))
    assert rc == 5 and "No such file or directory" in sp._lib.spmx_last_error(sp._h).decode()
    assert sp._lib.spmx_encode_file(sp._h, src.encode(), out.encode(), b"proto", C.byref(ns), C.byref(ni)) == 3
    msg = sp._lib.spmx_last_error(sp._h).decode()
    assert all(f in msg for f in ('"id"', '"piece"', '"bin"')), msg
    with open(src, "wb") as f:
        f.write(b"\n   \nHello world.\n\n")
    assert sp.EncodeFile(src, out, "piece")[0] == 4
    assert open(out, "rb").read() == ("\n\n" + GOLDEN["models"]["test_model"]["pieces"][0] + "\n\n").encode("utf-8")
    with open(src, "wb") as f:
        f.write(b"Hello world.")                                    # a last line without its '\n'
    sp.EncodeFile(src, out, "piece")
    assert open(out, "rb").read() == (GOLDEN["models"]["test_model"]["pieces"][0] + "\n").encode("utf-8")


# ---------------------------------------------------------------------------------------------- EncodeAsPieces ----
@pytest.mark.parametrize("model", ["test_model", "uni1k_bf", "bpe1k_bf_uds"])
def test_encode_as_pieces(model, emu, expect):
    sp = emu.load(fixtures.model_blob(model), classes=None).sp
    lines = crafted()
    try:
        for opts in OPTS:
            sp.SetEncodeExtraOptions(opts)
            ids, io, pblob, poffs = expect.get(model, opts, "crafted%d" % len(lines), lines)
            want = [[p.decode("utf-8", "surrogateescape") for p in r] for r in rows_of(pblob, poffs, io)]
            assert sp.EncodeAsPieces(lines) == want, opts
            assert sp.EncodeAsPieces(lines[-1]) == want[-1]
            assert sp.encode(lines[-1].decode(), out_type=str) == want[-1]
    finally:
        sp.SetEncodeExtraOptions("")


def test_encode_as_pieces_after_override(emu):
    """OverrideNormalizerSpec rebuilds the tables, the piece names among them: the pieces follow the new spec."""
    sp = emu.load(fixtures.model_blob("uni1k_bf"), classes=None).sp
    lines = [b"Hello world.", "café ก".encode(), b""]
    before = sp.EncodeAsPieces(lines)
    assert before[0][0].startswith("▁")
    sp.OverrideNormalizerSpec(add_dummy_prefix=False)
    after = sp.EncodeAsPieces(lines)
    assert after == [[p.decode("utf-8", "surrogateescape") for p, *_ in row] for row in sp.EncodeAsSentencePieceText(lines)]
    assert after != before and not after[0][0].startswith("▁")
    assert any(p.startswith("<0x") for p in after[1])


# ------------------------------------------------------------------------------------------------------ C++ facade ----
def _build_pieces_test(emu_build):
    src = os.path.join(ROOT, "tests", "cpp", "pieces_test.cc")
    lib = os.path.join(ROOT, "tests", "emu") if emu_build else os.path.join(ROOT, "sentencepiece_amd")
    out = os.path.join(ROOT, "tests", "cpp", "pieces_test" + ("_emu" if emu_build else ""))
    if emu_build:
        from tests import emulib
        emulib.lib()
    so = os.path.join(lib, "libspmx_emu.so" if emu_build else "libspmx.so")
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "include", "spmx_processor.h")),
                 os.path.getmtime(os.path.join(ROOT, "include", "spmx.h")), os.path.getmtime(so))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, src, "-L" + lib,
                               "-lspmx_emu" if emu_build else "-lspmx", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("opts", ["", "reverse:bos:eos"])
def test_facade_pieces_emulated(opts, expect, tmp_path):
    """EncodeAsPieces, Encode(input, vector<string>*) and EncodeAsPiecesBatch of include/spmx_processor.h, device emulated."""
    exe = _build_pieces_test(True)
    lines = getline_split(open(BOTCHAN, "rb").read())[:120]
    src = str(tmp_path / "in.txt")
    with open(src, "wb") as f:
        f.write(b"".join(x + b"\n" for x in lines))
    _, io, pblob, poffs = expect.get("test_model", opts, "botchan120", lines)
    args = [exe, os.path.join(fixtures.GOLDEN, "test_model.model"), src] + ([opts] if opts else [])
    env = dict(os.environ, SPMX_EMU_CUS="2")
    res = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr
    assert res.stdout == piece_image(rows_of(pblob, poffs, io))


# ------------------------------------------------------------------------------------------------- kernel resources ----
@pytest.mark.parametrize("kernel", ["IdLinesLenKernel", "IdLinesWriteKernel", "PieceLinesLenKernel", "PieceLinesWriteKernel",
                                    "PiecePackedLenKernel", "PiecePackedWriteKernel"])
def test_new_kernels_use_no_scratch(kernel):
    from tests.test_kernel_resources import REPORT, _report
    if not os.path.exists(REPORT):
        pytest.skip("no resource report next to the library (csrc/Makefile writes it with kernels.o)")
    rep = _report()
    names = [n for n in rep if kernel in n]
    assert len(names) == 1, (kernel, names)
    r = rep[names[0]]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r


# ------------------------------------------------------------------------------------------------------------ GPU ----
def _to_device(arr, pad=16):
    import torch
    arr = np.ascontiguousarray(arr)
    d = torch.zeros(arr.nbytes + pad, dtype=torch.uint8, device="cuda:0")
    if arr.nbytes:
        d[:arr.nbytes].copy_(torch.frombuffer(bytearray(arr.tobytes()), dtype=torch.uint8))
    return d


@pytest.fixture(scope="module")
def gpu_sp():
    from sentencepiece_amd.processor import SentencePieceProcessor
    return SentencePieceProcessor(model_proto=fixtures.model_blob("test_model"), device=0)


@pytest.mark.gpu
def test_id_formatter_gpu(gpu_sp):
    import torch
    for rows in id_cases():
        ids, offs = csr(rows)
        d_ids = _to_device(ids).view(torch.int32)[:len(ids)]
        d_offs = _to_device(offs.astype(np.int64), pad=0).view(torch.int64)
        assert gpu_sp.FormatIdLinesDevice(d_ids, d_offs).cpu().numpy().tobytes() == id_image(rows), len(rows)
    # a destination 5 bytes off a 16-byte boundary: the neighbours stay intact
    rows = id_cases()[-2]
    want = id_image(rows)
    ids, offs = csr(rows)
    d_ids = _to_device(ids).view(torch.int32)[:len(ids)]
    d_offs = _to_device(offs.astype(np.int64), pad=0).view(torch.int64)
    buf = torch.full((len(want) + 96,), 0xCD, dtype=torch.uint8, device="cuda:0")
    at = 32 + ((5 - buf.data_ptr() - 32) & 15)
    need = C.c_uint64(0)
    stream = torch.cuda.current_stream().cuda_stream
    rc = gpu_sp._lib.spmx_format_id_lines_device(gpu_sp._h, d_ids.data_ptr(), d_offs.data_ptr(), len(rows), buf.data_ptr() + at,
                                                 len(want) - 1, stream, C.byref(need))
    assert rc == 8 and need.value == len(want)
    rc = gpu_sp._lib.spmx_format_id_lines_device(gpu_sp._h, d_ids.data_ptr(), d_offs.data_ptr(), len(rows), buf.data_ptr() + at,
                                                 len(want), stream, C.byref(need))
    assert rc == 0 and need.value == len(want)
    got = buf.cpu().numpy()
    assert (got[:at] == 0xCD).all() and (got[at + len(want):] == 0xCD).all(), "write outside the image"
    assert got[at:at + len(want)].tobytes() == want


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_pieces_gpu(model, expect):
    import torch
    from sentencepiece_amd.processor import SentencePieceProcessor
    sp = SentencePieceProcessor(model_proto=fixtures.model_blob(model), device=0)
    lines = crafted()
    text, offs = packed(lines)
    d_text = _to_device(text, pad=32)[:len(text)]
    d_offs = _to_device(offs.astype(np.int64), pad=0).view(torch.int64)
    for opts in OPTS:
        sp.SetEncodeExtraOptions(opts)
        want = expect.get(model, opts, "crafted%d" % len(lines), lines)
        ids, io, pb, po = sp.EncodePiecesPacked(text, offs)
        assert np.array_equal(ids, want[0]) and np.array_equal(io, want[1]), opts
        assert pb.tobytes() == want[2] and np.array_equal(po, want[3]), opts
        d_ids, d_io, d_pb, d_po, total = sp.EncodePiecesDevice(d_text, d_offs)
        assert total == len(want[0]) and np.array_equal(d_ids.cpu().numpy(), want[0]), opts
        assert d_pb.cpu().numpy().tobytes() == want[2], opts
        assert np.array_equal(d_po.cpu().numpy().astype(np.uint64), want[3]), opts
        d_img, n_ids = sp.EncodePieceLinesDevice(d_text, d_offs)
        assert n_ids == len(want[0])
        assert d_img.cpu().numpy().tobytes() == piece_image(rows_of(want[2], want[3], want[1])), opts


@pytest.mark.gpu
def test_encode_file_piece_gpu(gpu_sp, tmp_path, monkeypatch):
    import torch
    out = str(tmp_path / "pieces.txt")
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    assert gpu_sp.EncodeFile(BOTCHAN, out, "piece")[0] == 4288
    got = open(out, "rb").read()
    assert hashlib.md5(got).hexdigest() == BOTCHAN_PIECES_MD5
    ids_out = str(tmp_path / "ids.txt")
    gpu_sp.EncodeFile(BOTCHAN, ids_out, "id")
    assert hashlib.md5(open(ids_out, "rb").read()).hexdigest() == BOTCHAN_IDS_MD5
    monkeypatch.delenv("SPMX_FILE_CHUNK")
    # the command line writes the same bytes
    exe = os.path.join(ROOT, "sentencepiece_amd", "spmx_encode")
    res = subprocess.run([exe, "--model=" + os.path.join(fixtures.GOLDEN, "test_model.model"), "--output_format=piece", BOTCHAN],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout == got
    # a device chain on one stream: file image -> lines -> piece lines, nothing copied to the host in between
    data = open(BOTCHAN, "rb").read()
    d_file = _to_device(np.frombuffer(data, dtype=np.uint8))[:len(data)]
    d_text, d_offs, n = gpu_sp.SplitLinesDevice(d_file)
    d_img, n_ids = gpu_sp.EncodePieceLinesDevice(d_text, d_offs)
    assert n == 4288 and d_img.cpu().numpy().tobytes() == got
