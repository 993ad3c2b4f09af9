"""The file side of Decode: the id-line parser and the line joiner (sentencepiece_amd/csrc/kernels_idtext.h), and
spmx_decode_file / DecodeFile / the spmx_decode command line around them -- the loop of the reference's spm_decode
(src/spm_decode_main.cc: std::getline, StrSplit(line, " ") without empty tokens, atoi per token, Decode, WriteLine).

The parser's oracle lives here: getline_split as in tests/test_split.py, line.split(b" ") without its empty tokens, libc's
atoi through ctypes.  The text's oracle is oracle.decode_batch on those ids, every line followed by b"\\n"; where the compiled
reference is present its decode_batch / decode_pieces are compared as well.
CPU: the device bodies under the wavefront emulator through the C ABI; GPU: the torch-tensor methods and the binary."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from tests import fixtures, refshim
from tests.emulib import EmuLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")
FILE_MODELS = ["test_model", "bpe1k_bf_uds", "char1k", "word1k"]
# md5 of botchan.txt encoded and decoded again by the compiled reference under test_model.model, every line with its '\n'
BOTCHAN_DECODED_MD5 = "58027be27acf20eac1315eefecd471fb"

_libc = C.CDLL(None)
_libc.atoi.restype = C.c_int
_libc.atoi.argtypes = [C.c_char_p]


def getline_split(data):
    """What a std::getline loop yields: '\\n' ends a line, a trailing line without it counts, "a\\n" is one line."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def want_csr(data):
    """(ids int32, id_offsets uint64) of a file image: getline, split at ' ' without empty tokens, libc atoi."""
    ids, offs = [], [0]
    for line in getline_split(data):
        ids.extend(_libc.atoi(tok) for tok in line.split(b" ") if tok)
        offs.append(len(ids))
    return np.asarray(ids, dtype=np.int32), np.asarray(offs, dtype=np.uint64)


ATOI_TABLE = [(b"\t\r+12x", 12), (b"\r", 0), (b"+-5", 0), (b"12\x003", 12), (b"2147483648", -2147483648), (b"4294967301", 5),
              (b"9223372036854775808", -1), (b"99999999999999999999", -1), (b"-9223372036854775809", 0),
              (b"0" * 24 + b"12", 12), (b"\xc2\xa05", 0)]


def _fill(n):
    """n bytes of short tokens and single spaces, ending in a space."""
    return (b"31 7 205 " * (n // 9 + 1))[:n - 1] + b" " if n else b""


def parser_cases():
    rng = random.Random(9)
    out = [b"", b"\n", b"7", b"7\n", b" 7  8 \n", b"\n\n\n", b"1 2\r\n3\r\n", b"1 2 \r\n"]
    out += [tok for tok, _ in ATOI_TABLE]
    out.append(b" ".join(tok for tok, _ in ATOI_TABLE) + b"\n")
    for p in (15, 16, 1023, 1024, 16383, 16384):
        out.append(_fill(p) + b"4711 12\n")                       # a delimiter before the token's first byte at p
        out.append(_fill(p - 3) + b"1234567 12\n")                # ... a token from before going on through p
        for d in (b" ", b"\n"):                                   # a delimiter at p between two digit runs
            out.append(_fill(p - 5) + b"98765" + d + b"43210 1" + d)
    out.append(_fill(16384 - 20) + b"0" * 30 + b"1234567890" + b" 5\n")      # a 40-byte token over a chunk end
    out.append(_fill(16384 - 20) + b"\t" * 30 + b"-123456789x" + b" 5")       # ... its value behind the chunk end
    out.append(b"\n" * 1025 + b"5")
    out.append(b" ".join(b"%d" % (k * 37) for k in range(70)) + b"\n")        # more tokens on a line than a wavefront has lanes
    out.append(b"1 2\n3 4")
    out.append(b"1 2\n3 4 ")
    out.append(b"9" * 3000 + b" 1\n")                                         # a digit string much longer than a step
    for n in (1000, 5000, 2 * 16384 + 5, 70001):
        for p_nl in (0.01, 0.1, 0.6):
            out.append(bytes(0x0A if rng.random() < p_nl else rng.choice(b"0123456789 \n\r\t+-x") for _ in range(n)))
    return out


def joiner_cases():
    rng = random.Random(10)
    out = [[], [b""], [b""] * 1025, [b"a"]]
    out += [[b"x" * n] for n in (15, 16, 17, 1023, 1024, 16385)]
    out.append([b"ab" * 8, b"", b"c" * 15, b"d" * 16, b"", b"", b"e" * 17])
    out.append([bytes(rng.choice(b"abc \r\xe3\x81\x82") for _ in range(rng.choice((0, 0, 1, 3, 15, 16, 17, 40, 300, 2000))))
                for _ in range(400)])
    out.append([b"q" * 20000, b"", b"r" * 16384, b"s"])
    return out


def packed(lines):
    offs = np.zeros(len(lines) + 1, dtype=np.uint64)
    if lines:
        offs[1:] = np.cumsum([len(x) for x in lines])
    return np.frombuffer(b"".join(lines), dtype=np.uint8), offs


def image(lines):
    return b"".join(x + b"\n" for x in lines)


def test_atoi_table():
    """The issue's table is what this machine's libc says (the oracle the other tests lean on)."""
    for tok, want in ATOI_TABLE:
        assert _libc.atoi(tok) == want, tok


# ---------------------------------------------------------------------------------------------- emulator, C ABI ----
def emu_parse(h, data):
    """bytes -> (ids, id_offsets) through spmx_parse_id_lines_device on host memory; checks the capacity protocol."""
    n = len(data)
    raw = np.zeros(n + 64, dtype=np.uint8)
    shift = (-raw.ctypes.data) & 15
    buf = raw[shift:shift + n + 16]
    buf[:n] = np.frombuffer(data, dtype=np.uint8)
    buf[n:] = 0x31            # padding must not count
    nl, nt = C.c_uint64(0), C.c_uint64(0)
    small = np.full(1, 0xCDCDCDCD, dtype=np.uint64)
    rc = h.lib.spmx_parse_id_lines_device(h.sp._h, buf.ctypes.data, n, None, 0, small.ctypes.data, 1, None, C.byref(nl), C.byref(nt))
    if n == 0:
        assert rc == 0 and small[0] == 0 and (nl.value, nt.value) == (0, 0)
    elif rc != 0:
        assert rc == 8, h.lib.spmx_last_error(None)
    ids = np.full(nt.value + 3, -0x32323233, dtype=np.int32)
    offs = np.full(nl.value + 4, 0xCDCDCDCD, dtype=np.uint64)
    lines, total = nl.value, nt.value
    rc = h.lib.spmx_parse_id_lines_device(h.sp._h, buf.ctypes.data, n, ids.ctypes.data, total, offs.ctypes.data, lines + 1, None,
                                          C.byref(nl), C.byref(nt))
    assert rc == 0, h.lib.spmx_last_error(None)
    assert (nl.value, nt.value) == (lines, total)
    assert (ids[total:] == -0x32323233).all(), "write past the ids"
    assert (offs[lines + 1:] == 0xCDCDCDCD).all(), "write past the offsets"
    return ids[:total].copy(), offs[:lines + 1].copy()


def emu_join(h, lines, shift):
    """lines -> the file image through spmx_join_lines_device, the destination `shift` bytes off a 16-byte boundary."""
    text, offs = packed(lines)
    text = np.concatenate([text, np.zeros(1, dtype=np.uint8)])     # (a valid pointer for an empty text)
    need = C.c_uint64(0)
    rc = h.lib.spmx_join_lines_device(h.sp._h, text.ctypes.data, offs.ctypes.data, len(lines), None, 0, None, C.byref(need))
    want = len(text) - 1 + len(lines)
    assert need.value == want and rc == (8 if want else 0)
    raw = np.full(want + 96, 0xCD, dtype=np.uint8)
    at = 32 + ((shift - raw.ctypes.data - 32) & 15)
    assert (raw.ctypes.data + at) % 16 == shift
    rc = h.lib.spmx_join_lines_device(h.sp._h, text.ctypes.data, offs.ctypes.data, len(lines), raw.ctypes.data + at, want, None,
                                      C.byref(need))
    assert rc == 0 and need.value == want, h.lib.spmx_last_error(None)
    assert (raw[:at] == 0xCD).all() and (raw[at + want:] == 0xCD).all(), "write outside the image"
    return raw[at:at + want].tobytes()


@pytest.fixture(scope="module")
def emu():
    return EmuLib()


@pytest.mark.parametrize("cus", [1, 3])
def test_parser_emulated(emu, cus):
    """SPMX_EMU_CUS 1: a grid of one block for every image; 3: several blocks from 3 chunks on."""
    h = emu.load(fixtures.model_blob("test_model"), cus=cus)
    for data in parser_cases():
        ids, offs = emu_parse(h, data)
        want_ids, want_offs = want_csr(data)
        assert np.array_equal(offs, want_offs), (len(data), data[:40])
        assert np.array_equal(ids, want_ids), (len(data), data[:40])


def test_parser_rejects_a_misaligned_image(emu):
    h = emu.load(fixtures.model_blob("test_model"))
    raw = np.zeros(64, dtype=np.uint8)
    at = raw.ctypes.data + ((1 - raw.ctypes.data) & 15)
    nl, nt = C.c_uint64(0), C.c_uint64(0)
    assert h.lib.spmx_parse_id_lines_device(h.sp._h, at, 4, None, 0, None, 0, None, C.byref(nl), C.byref(nt)) == 3


@pytest.mark.parametrize("cus", [1, 3])
def test_joiner_emulated(emu, cus):
    h = emu.load(fixtures.model_blob("test_model"), cus=cus)
    for lines in joiner_cases():
        for shift in (0, 5):
            assert emu_join(h, lines, shift) == image(lines), (len(lines), shift)


# ------------------------------------------------------------------------------------------- the file call (emulated) ----
@pytest.fixture(scope="module")
def botchan_ids(emu, oracle, tmp_path_factory):
    """{model: (sp, path of EncodeFile(botchan, "id")'s output, ids, id_offsets)}: encoded once for the module.
    bpe1k_bf_uds: the emulated BPE encode of botchan takes 13 s, so its id file is written here in EncodeFile's format
    (tests/test_host.py pins that format) from the oracle's ids."""
    made = {}

    def get(model):
        if model not in made:
            sp = emu.load(fixtures.model_blob(model), classes=None).sp
            path = str(tmp_path_factory.mktemp("ids") / (model + ".ids"))
            if model == "bpe1k_bf_uds":
                ids, io = oracle.load(fixtures.model_blob(model)).encode_batch(*packed(getline_split(open(BOTCHAN, "rb").read())))
                io = io.astype(np.int64)
                with open(path, "wb") as f:
                    f.write(image([b" ".join(b"%d" % t for t in ids[io[i]:io[i + 1]]) for i in range(len(io) - 1)]))
            else:
                sp.EncodeFile(BOTCHAN, path, "id")
            made[model] = (sp, path) + want_csr(open(path, "rb").read())
        return made[model]
    return get


def _lines_of(text, offs):
    offs = offs.astype(np.int64)
    text = text.tobytes()
    return b"".join(text[offs[i]:offs[i + 1]] + b"\n" for i in range(len(offs) - 1))


def want_text(oracle, model, sp, ids, io):
    """The oracle's Decode of every line with its '\\n', equal to the compiled reference's where that is built.  The oracle
    restates unigram and BPE only: a character or word model is decoded by the compiled reference, or failing that by the
    engine's own batch Decode (tests/test_charword.py pins it to the reference's digests)."""
    r = refshim.RefLib().load(fixtures.model_blob(model)) if refshim.available() else None
    if model in ("char1k", "word1k"):
        return _lines_of(*(r.decode_batch(ids, io) if r is not None else sp.DecodePacked(ids, io)))
    want = _lines_of(*oracle.load(fixtures.model_blob(model)).decode_batch(ids, io))
    if r is not None:
        assert want == _lines_of(*r.decode_batch(ids, io))
    return want


@pytest.mark.parametrize("model", FILE_MODELS)
def test_decode_file_round_trip(model, botchan_ids, oracle, tmp_path, monkeypatch):
    sp, path, ids, io = botchan_ids(model)
    want = want_text(oracle, model, sp, ids, io)
    out = str(tmp_path / "text.txt")
    for chunk in ("4096", None):
        if chunk:
            monkeypatch.setenv("SPMX_FILE_CHUNK", chunk)
        else:
            monkeypatch.delenv("SPMX_FILE_CHUNK")
        assert sp.DecodeFile(path, out, "id") == (len(io) - 1, len(ids))
        assert open(out, "rb").read() == want, chunk
    # "bin": the ids EncodeFile writes flat (bpe1k_bf_uds: the same layout written here), chunked by their offsets
    binp = str(tmp_path / "ids.bin")
    if model == "bpe1k_bf_uds":
        ids.astype("<i4").tofile(binp)
        io.astype("<u8").tofile(binp + ".idx")
    else:
        sp.EncodeFile(BOTCHAN, binp, "bin")
    for chunk in ("4096", None):
        if chunk:
            monkeypatch.setenv("SPMX_FILE_CHUNK", chunk)
        else:
            monkeypatch.delenv("SPMX_FILE_CHUNK")
        assert sp.DecodeFile(binp, out, "bin") == (len(io) - 1, len(ids))
        assert open(out, "rb").read() == want, chunk


def test_decode_file_botchan_md5(botchan_ids, tmp_path):
    """The decoded botchan under test_model.model against the digest of the compiled reference's text:
    ids, io = RefLib().load(blob).encode_batch(*packed(getline_split(botchan))); t, o = r.decode_batch(ids, io);
    md5(b"".join(t[o[i]:o[i + 1]] + b"\\n" for i in range(4288)))."""
    sp, path, ids, io = botchan_ids("test_model")
    out = str(tmp_path / "text.txt")
    assert sp.DecodeFile(path, out) == (4288, 95515)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == BOTCHAN_DECODED_MD5


@pytest.mark.parametrize("model", FILE_MODELS)
def test_decode_file_pieces(model, emu, tmp_path, monkeypatch):
    sp = emu.load(fixtures.model_blob(model), classes=None).sp
    r = refshim.RefLib().load(fixtures.model_blob(model)) if refshim.available() else None
    src = getline_split(open(BOTCHAN, "rb").read())[:300]
    rows = [[p.encode() for p in row] for row in sp.EncodeAsPieces([x.decode() for x in src])]
    rows.insert(7, [rows[0][0], b"\xe2\x96\x81zzqqzz", b"<unk>", b"not-a-piece"] if rows[0] else [b"\xe2\x96\x81zzqqzz"])
    rows.insert(9, [])
    path, out = str(tmp_path / "pieces.txt"), str(tmp_path / "text.txt")
    with open(path, "wb") as f:
        f.write(b"".join(b"  ".join(row) + b" \n" if i == 3 else b" ".join(row) + b"\n" for i, row in enumerate(rows)))
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    try:
        for opts in ("", "unk", "reverse:bos:eos"):
            sp.SetDecodeExtraOptions(opts)
            want = [sp.DecodePieces(row, out_type=bytes) if row else sp.DecodePieces([row], out_type=bytes)[0] for row in rows]
            if r is not None:
                r.set_decode_extra_options(opts)
                assert want == [r.decode_pieces(row) for row in rows], opts
            assert sp.DecodeFile(path, out, "piece") == (len(rows), sum(len(row) for row in rows))
            assert open(out, "rb").read() == image(want), opts
    finally:
        sp.SetDecodeExtraOptions("")


def test_decode_file_invalid_id(botchan_ids, tmp_path, monkeypatch):
    sp, path, ids, io = botchan_ids("test_model")
    lines = open(path, "rb").read().split(b"\n")[:-1]
    size = sp.GetPieceSize()
    bad, out = str(tmp_path / "bad.ids"), str(tmp_path / "text.txt")
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    nl, ni = C.c_uint64(0), C.c_uint64(0)
    for token, later in ((b"%d" % size, b"%d" % (size + 7)), (b"-1", b"%d" % size)):
        for second in (False, True):
            rows = list(lines)
            rows[2999] = rows[2999] + b" " + token          # line 3000
            if second:
                rows[4100] = later + b" " + rows[4100]      # ... and another one chunks later
            with open(bad, "wb") as f:
                f.write(image(rows))
            assert os.path.getsize(bad) > 50 * 4096
            rc = sp._lib.spmx_decode_file(sp._h, bad.encode(), out.encode(), b"id", C.byref(nl), C.byref(ni))
            assert rc == 11
            assert sp._lib.spmx_last_error(sp._h).decode() == "Invalid id: " + token.decode()
            with pytest.raises(RuntimeError, match="Invalid id: " + token.decode() + "$"):
                sp.DecodeFile(bad, out, "id")


def test_decode_file_empty_and_missing(emu, tmp_path):
    sp = emu.load(fixtures.model_blob("test_model")).sp
    src, out = str(tmp_path / "empty.ids"), str(tmp_path / "text.txt")
    open(src, "wb").close()
    for fmt in ("id", "piece"):
        assert sp.DecodeFile(src, out, fmt) == (0, 0)
        assert open(out, "rb").read() == b""
    nl, ni = C.c_uint64(0), C.c_uint64(0)
    for fmt in (b"id", b"bin", b"piece"):
        rc = sp._lib.spmx_decode_file(sp._h, str(tmp_path / "nothing").encode(), out.encode(), fmt, C.byref(nl), C.byref(ni))
        assert rc == 5 and "No such file or directory" in sp._lib.spmx_last_error(sp._h).decode()
    assert sp._lib.spmx_decode_file(sp._h, src.encode(), out.encode(), b"proto", C.byref(nl), C.byref(ni)) == 3
    # lines without ids still write their '\n'
    with open(src, "wb") as f:
        f.write(b"\n   \n\n")
    assert sp.DecodeFile(src, out, "id") == (3, 0)
    assert open(out, "rb").read() == b"\n\n\n"


def test_decode_file_denormalizer(emu, tmp_path, monkeypatch):
    """uni1k_ident_dn carries a denormalizer_spec: the file holds the denormalized text, as Decode returns it."""
    blob = fixtures.model_blob("uni1k_ident_dn")
    sp = emu.load(blob, classes=None).sp
    src = [x for x in getline_split(open(BOTCHAN, "rb").read())[:200]] + ["ｆｕｌｌ　ｗｉｄｔｈ ①② ﬁ".encode()]
    text, offs = packed(src)
    ids, io = sp.EncodePacked(text, offs)
    dt, do = sp.DecodePacked(ids, io)
    do = do.astype(np.int64)
    want = b"".join(dt.tobytes()[do[i]:do[i + 1]] + b"\n" for i in range(len(src)))
    if refshim.available():
        rt, ro = refshim.RefLib().load(blob).decode_batch(ids, io)
        ro = ro.astype(np.int64)
        assert want == b"".join(rt.tobytes()[ro[i]:ro[i + 1]] + b"\n" for i in range(len(src)))
    io = io.astype(np.int64)
    path, out = str(tmp_path / "in.ids"), str(tmp_path / "text.txt")
    with open(path, "wb") as f:
        f.write(image([b" ".join(b"%d" % t for t in ids[io[i]:io[i + 1]]) for i in range(len(src))]))
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    assert sp.DecodeFile(path, out, "id") == (len(src), len(ids))
    assert open(out, "rb").read() == want


# ------------------------------------------------------------------------------------------------- kernel resources ----
@pytest.mark.parametrize("kernel", ["ParseIdsCountKernel", "ParseIdsWriteKernel", "JoinLinesKernel"])
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
def _to_device(data):
    import torch
    d = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda:0")[:len(data)]
    if data:
        d.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return d


@pytest.fixture(scope="module")
def gpu_sp():
    from sentencepiece_amd.processor import SentencePieceProcessor
    return SentencePieceProcessor(model_proto=fixtures.model_blob("test_model"), device=0)


@pytest.mark.gpu
def test_parser_gpu(gpu_sp):
    for data in parser_cases():
        d_ids, d_offs, n, t = gpu_sp.ParseIdLinesDevice(_to_device(data))
        want_ids, want_offs = want_csr(data)
        assert (n, t) == (len(want_offs) - 1, len(want_ids)), (len(data), data[:40])
        assert np.array_equal(d_offs.cpu().numpy().astype(np.uint64), want_offs), (len(data), data[:40])
        assert np.array_equal(d_ids.cpu().numpy(), want_ids), (len(data), data[:40])


@pytest.mark.gpu
def test_joiner_gpu(gpu_sp):
    import torch
    for lines in joiner_cases():
        text, offs = packed(lines)
        d_text = _to_device(text.tobytes())
        d_offs = torch.from_numpy(offs.astype(np.int64)).to("cuda:0")
        assert gpu_sp.JoinLinesDevice(d_text, d_offs).cpu().numpy().tobytes() == image(lines), len(lines)
        # a destination 5 bytes off a 16-byte boundary, through the C ABI
        want = len(text) + len(lines)
        d_out = torch.full((want + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
        at = (5 - d_out.data_ptr()) & 15
        need = C.c_uint64(0)
        rc = gpu_sp._lib.spmx_join_lines_device(gpu_sp._h, d_text.data_ptr(), d_offs.data_ptr(), len(lines), d_out.data_ptr() + at,
                                                want, torch.cuda.current_stream().cuda_stream, C.byref(need))
        assert rc == 0 and need.value == want
        got = d_out.cpu().numpy()
        assert got[at:at + want].tobytes() == image(lines), len(lines)
        assert (got[:at] == 0xCD).all() and (got[at + want:] == 0xCD).all()


@pytest.fixture(scope="module")
def gpu_botchan(gpu_sp, oracle, tmp_path_factory):
    """(path of the id file, the text the oracle decodes from it)"""
    path = str(tmp_path_factory.mktemp("gpu_ids") / "botchan.ids")
    assert gpu_sp.EncodeFile(BOTCHAN, path, "id") == (4288, 95515)
    ids, io = want_csr(open(path, "rb").read())
    return path, want_text(oracle, "test_model", gpu_sp, ids, io)


@pytest.mark.gpu
def test_decode_file_gpu(gpu_sp, gpu_botchan, tmp_path, monkeypatch):
    path, want = gpu_botchan
    out = str(tmp_path / "text.txt")
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    assert gpu_sp.DecodeFile(path, out, "id") == (4288, 95515)
    got = open(out, "rb").read()
    assert got == want and hashlib.md5(got).hexdigest() == BOTCHAN_DECODED_MD5


@pytest.mark.gpu
def test_spmx_decode_binary_gpu(gpu_sp, gpu_botchan, tmp_path):
    path, want = gpu_botchan
    exe = os.path.join(ROOT, "sentencepiece_amd", "spmx_decode")
    model = os.path.join(fixtures.GOLDEN, "test_model.model")
    with open(path, "rb") as f:
        r = subprocess.run([exe, "--model=" + model, "--input_format=id"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    bad = str(tmp_path / "bad.ids")
    with open(bad, "wb") as f:
        f.write(b"5 6\n7 %d\n" % gpu_sp.GetPieceSize())
    r = subprocess.run([exe, "--model=" + model, "--input_format=id", "--input=" + bad], capture_output=True)
    assert r.returncode == 1 and b"Invalid id: %d" % gpu_sp.GetPieceSize() in r.stderr and r.stdout == b""


@pytest.mark.gpu
def test_device_chain_gpu(gpu_sp, gpu_botchan, tmp_path):
    """ParseIdLinesDevice -> DecodeDevice -> JoinLinesDevice on one stream, nothing copied to the host in between."""
    import torch
    path, want = gpu_botchan
    stream = torch.cuda.Stream(device="cuda:0")
    d_file = _to_device(open(path, "rb").read())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        d_ids, d_io, n, t = gpu_sp.ParseIdLinesDevice(d_file, stream=stream.cuda_stream)
        d_text, d_to, total = gpu_sp.DecodeDevice(d_ids, d_io, stream=stream.cuda_stream)
        d_image = gpu_sp.JoinLinesDevice(d_text[:total], d_to, stream=stream.cuda_stream)
    stream.synchronize()
    assert (n, t) == (4288, 95515)
    out = str(tmp_path / "text.txt")
    gpu_sp.DecodeFile(path, out, "id")
    assert d_image.cpu().numpy().tobytes() == open(out, "rb").read() == want
