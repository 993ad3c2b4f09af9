"""spmx_encode_file_ex: the lattice formats of spm_encode (src/spm_encode_main.cc:120-153) through the chunk pipeline, the
lattice calls' device forms and the id-line writer.

nbest_id / nbest_piece / sample_id / sample_piece: the file equals the Python formatting of the host calls' results
(NBestPacked / NBestEncodeAsPieces / SampleEncodePacked / SampleEncodeAsPieces with the same seed) over getline-split lines;
the sample files do not depend on SPMX_FILE_CHUNK; nbest_id and nbest_piece are pinned to the compiled reference's
`spm_encode --output_format=nbest_id | nbest_piece` by md5 (tests/golden/nbest_lines.json, recorded by
scripts/make_nbest_lines_golden.py).  The reference's sample formats draw from a thread-local mt19937 and cannot be pinned
byte for byte: their distribution is pinned through the host calls by tests/test_sampling_marginals.py.  id / piece / bin
give spmx_encode_file's bytes; the three proto formats give an empty file.

CPU: the emulated library's C ABI.  GPU: the spmx_encode binary and EncodeFile."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import fixtures
from tests.emulib import EmuLib
from tests.test_decode_file import getline_split, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")
GOLDEN = json.load(open(os.path.join(fixtures.GOLDEN, "nbest_lines.json"), encoding="utf-8"))
OPTS = ["", "bos:eos", "reverse", "unk_piece"]


@pytest.fixture(scope="module")
def emu():
    return EmuLib()


@pytest.fixture(scope="module")
def botchan():
    return open(BOTCHAN, "rb").read().splitlines(True)


def id_lines(ids, io):
    io = np.asarray(io).astype(np.int64)
    return b"".join(b" ".join(b"%d" % t for t in ids[io[r]:io[r + 1]]) + b"\n" for r in range(len(io) - 1))


def want_nbest(sp, data, k):
    ids, io, _, ro = sp.NBestPacked(*packed(getline_split(data)), k)
    return id_lines(ids, io), int(ro[-1]), len(ids)


def want_sample(sp, data, k, alpha, seed):
    ids, io = sp.SampleEncodePacked(*packed(getline_split(data)), k, alpha, seed)
    return id_lines(ids, io), len(io) - 1, len(ids)


def piece_lines(results):
    return b"".join(" ".join(r).encode("utf-8", "surrogateescape") + b"\n" for r in results)


def want_nbest_pieces(sp, data, k):
    per_line = sp.NBestEncodeAsPieces(getline_split(data), k)
    return piece_lines([r for line in per_line for r in line])


def want_sample_pieces(sp, data, k, alpha, seed):
    lines = getline_split(data)
    return piece_lines(sp.SampleEncodeAsPieces(lines, k, alpha, seed=seed)) if lines else b""


def datas(botchan):
    body = b"".join(botchan[:60])
    return [("lf", body), ("no_last_lf", body + b"a last line"), ("crlf", body.replace(b"\n", b"\r\n")), ("empty", b""),
            ("blank_lines", b"\n\nhello world\n\n"), ("one", b"x"),
            ("unknown", "abc กขฃxyz ก\nกข 😀😁 tail\n㎿㌖ ﷺ ﬃ  two  spaces\n".encode("utf-8"))]


@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
def test_nbest_id_file(model, emu, botchan, tmp_path):
    sp = emu.load(fixtures.model_blob(model), cus=3).sp
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    try:
        for opts in OPTS:
            sp.SetEncodeExtraOptions(opts)
            for name, data in datas(botchan):
                open(src, "wb").write(data)
                for k in (3, 1):
                    image, lines, n_ids = want_nbest(sp, data, k)
                    assert sp.EncodeFile(src, out, "nbest_id", nbest_size=k) == (len(getline_split(data)), lines, n_ids), (opts, name, k)
                    assert open(out, "rb").read() == image, (opts, name, k)
                    assert sp.EncodeFile(src, out, "nbest_piece", nbest_size=k) == (len(getline_split(data)), lines, n_ids), (opts, name, k)
                    assert open(out, "rb").read() == want_nbest_pieces(sp, data, k), (opts, name, k)
    finally:
        sp.SetEncodeExtraOptions("")


@pytest.mark.parametrize("model,cases", [("test_model", ((-1, 0.3), (5, 0.5), (1, 0.5))), ("uni1k_bf", ((-1, 0.1),)),
                                         ("bpe1k", ((-1, 0.1), (-1, 0.0))), ("bpe1k_llama", ((3, 0.2),))])
def test_sample_id_file(model, cases, emu, botchan, tmp_path, monkeypatch):
    sp = emu.load(fixtures.model_blob(model), cus=3).sp
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    try:
        for opts in OPTS:
            sp.SetEncodeExtraOptions(opts)
            for name, data in datas(botchan):
                open(src, "wb").write(data)
                for k, alpha in cases if not opts else cases[:1]:
                    image, lines, n_ids = want_sample(sp, data, k, alpha, 41)
                    assert sp.EncodeFile(src, out, "sample_id", nbest_size=k, alpha=alpha, seed=41) == (lines, lines, n_ids), (opts, name, k)
                    assert open(out, "rb").read() == image, (opts, name, k, alpha)
                    assert sp.EncodeFile(src, out, "sample_piece", nbest_size=k, alpha=alpha, seed=41) == (lines, lines, n_ids), (opts, name, k)
                    assert open(out, "rb").read() == want_sample_pieces(sp, data, k, alpha, 41), (opts, name, k, alpha)
        # the draws depend on (seed, line number) alone: a file cut into many chunks gives the same bytes
        sp.SetEncodeExtraOptions("")
        data = b"".join(botchan[:400])
        open(src, "wb").write(data)
        k, alpha = cases[0]
        sp.EncodeFile(src, out, "sample_id", nbest_size=k, alpha=alpha, seed=7)
        whole = open(out, "rb").read()
        assert whole == want_sample(sp, data, k, alpha, 7)[0]
        monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
        assert len(data) > 4 * 4096
        sp.EncodeFile(src, out, "sample_id", nbest_size=k, alpha=alpha, seed=7)
        assert open(out, "rb").read() == whole
        if alpha > 0:
            sp.EncodeFile(src, out, "sample_id", nbest_size=k, alpha=alpha, seed=8)
            assert open(out, "rb").read() != whole
        sp.EncodeFile(src, out, "sample_piece", nbest_size=k, alpha=alpha, seed=7)           # (still at 4096 bytes a chunk)
        chunked = open(out, "rb").read()
        monkeypatch.delenv("SPMX_FILE_CHUNK")
        sp.EncodeFile(src, out, "sample_piece", nbest_size=k, alpha=alpha, seed=7)
        assert open(out, "rb").read() == chunked == want_sample_pieces(sp, data, k, alpha, 7)
    finally:
        sp.SetEncodeExtraOptions("")


def test_nbest_id_chunked(emu, botchan, tmp_path, monkeypatch):
    sp = emu.load(fixtures.model_blob("test_model"), cus=3).sp
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    data = b"".join(botchan[:300])
    open(src, "wb").write(data)
    image, lines, n_ids = want_nbest(sp, data, 3)
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    assert sp.EncodeFile(src, out, "nbest_id", nbest_size=3) == (300, lines, n_ids)
    assert open(out, "rb").read() == image
    assert sp.EncodeFile(src, out, "nbest_piece", nbest_size=3) == (300, lines, n_ids)
    assert open(out, "rb").read() == want_nbest_pieces(sp, data, 3)


@pytest.mark.parametrize("model", ["test_model", "uni1k_bf"])
@pytest.mark.parametrize("fmt", ["nbest_id", "nbest_piece"])
def test_nbest_against_the_reference(model, fmt, emu, botchan, tmp_path):
    """md5 of the whole image against what the compiled reference's spm_encode --output_format=nbest_id | nbest_piece
    --nbest_size=3 wrote for botchan's first 200 lines."""
    sp = emu.load(fixtures.model_blob(model), cus=3).sp
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(src, "wb").write(b"".join(botchan[:GOLDEN["lines"]]))
    sp.EncodeFile(src, out, fmt, nbest_size=GOLDEN["nbest_size"])
    got = open(out, "rb").read()
    want = GOLDEN["models"][model][fmt]
    assert got.decode("utf-8").split("\n")[:20] == want["head"]
    assert len(got) == want["bytes"] and hashlib.md5(got).hexdigest() == want["md5"]


@pytest.mark.parametrize("model", ["test_model", "bpe1k"])
def test_existing_formats_through_ex(model, emu, botchan, tmp_path):
    sp = emu.load(fixtures.model_blob(model), cus=3).sp
    src = str(tmp_path / "in.txt")
    open(src, "wb").write(b"".join(botchan[:200]) + b"no newline")
    import ctypes as C
    for fmt in ("id", "piece", "bin"):
        a, b = str(tmp_path / ("a." + fmt)), str(tmp_path / ("b." + fmt))
        want = sp.EncodeFile(src, a, fmt)
        ns, nl, ni = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert sp._lib.spmx_encode_file_ex(sp._h, src.encode(), b.encode(), fmt.encode(), 10, C.c_float(0.5), 0, C.byref(ns), C.byref(nl),
                                           C.byref(ni)) == 0
        assert (ns.value, ni.value) == want and nl.value == ns.value
        assert open(a, "rb").read() == open(b, "rb").read()
        if fmt == "bin":
            assert open(a + ".idx", "rb").read() == open(b + ".idx", "rb").read()


def test_proto_formats_and_refusals(emu, botchan, tmp_path):
    sp = emu.load(fixtures.model_blob("test_model")).sp
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(src, "wb").write(b"".join(botchan[:50]))
    for fmt in ("proto", "sample_proto", "nbest_proto"):
        open(out, "wb").write(b"stale")
        assert sp.EncodeFile(src, out, fmt) == (0, 0, 0)
        assert open(out, "rb").read() == b""
    with pytest.raises(Exception, match="format must be"):
        sp.EncodeFile(src, out, "nonsense")
    with pytest.raises(Exception, match="nbest_size <= 512"):
        sp.EncodeFile(src, out, "sample_id", nbest_size=513)
    with pytest.raises(Exception):
        sp.EncodeFile(str(tmp_path / "missing.txt"), out, "nbest_id")
    bpe = emu.load(fixtures.model_blob("bpe1k")).sp
    for fmt in ("nbest_id", "nbest_piece"):
        with pytest.raises(Exception, match="NBestEncode is not available for the current model."):
            bpe.EncodeFile(src, out, fmt)
    char = emu.load(fixtures.model_blob("char1k"), classes=None).sp
    for fmt in ("sample_id", "sample_piece"):
        with pytest.raises(Exception, match="SampleEncode is not available for the current model."):
            char.EncodeFile(src, out, fmt)
    # a seed of None counts up per call: two files of draws differ
    sp.EncodeFile(src, out, "sample_id", nbest_size=-1, alpha=0.5)
    first = open(out, "rb").read()
    sp.EncodeFile(src, out, "sample_id", nbest_size=-1, alpha=0.5)
    assert open(out, "rb").read() != first


# ----------------------------------------------------------------------------------------------------------- GPU half ----
EXE = os.path.join(ROOT, "sentencepiece_amd", "spmx_encode")
MODEL = os.path.join(fixtures.GOLDEN, "test_model.model")


@pytest.fixture(scope="module")
def gpu(botchan, tmp_path_factory):
    """(processor, botchan's first 300 lines, their file, an output path, run(fmt, *flags) -> what the binary wrote)"""
    from sentencepiece_amd.processor import SentencePieceProcessor
    sp = SentencePieceProcessor(model_file=MODEL)
    d = tmp_path_factory.mktemp("lattice_files")
    data = b"".join(botchan[:300])
    src, out = str(d / "in.txt"), str(d / "out.txt")
    open(src, "wb").write(data)

    def run(fmt, *flags, input=src):
        subprocess.run([EXE, "--model=" + MODEL, "--input=" + input, "--output=" + out, "--output_format=" + fmt, *flags], check=True,
                       stderr=subprocess.PIPE)
        return open(out, "rb").read()
    return sp, data, src, out, run


@pytest.mark.gpu
def test_gpu_binary_nbest_formats(gpu, botchan, tmp_path):
    sp, data, src, out, run = gpu
    assert run("nbest_id") == want_nbest(sp, data, 10)[0]                   # (--nbest_size defaults to 10)
    assert run("nbest_id", "--nbest_size=3") == want_nbest(sp, data, 3)[0]
    assert run("nbest_piece", "--nbest_size=3") == want_nbest_pieces(sp, data, 3)
    head = str(tmp_path / "head.txt")
    open(head, "wb").write(b"".join(botchan[:GOLDEN["lines"]]))
    for fmt in ("nbest_id", "nbest_piece"):
        assert hashlib.md5(run(fmt, "--nbest_size=3", input=head)).hexdigest() == GOLDEN["models"]["test_model"][fmt]["md5"]
    sp.SetEncodeExtraOptions("bos:eos")
    try:
        assert run("nbest_piece", "--nbest_size=3", "--extra_options=bos:eos") == want_nbest_pieces(sp, data, 3)
    finally:
        sp.SetEncodeExtraOptions("")


@pytest.mark.gpu
def test_gpu_binary_sample_and_proto_formats(gpu):
    sp, data, src, out, run = gpu
    assert run("sample_id", "--nbest_size=-1", "--alpha=0.3", "--random_seed=9") == want_sample(sp, data, -1, 0.3, 9)[0]
    assert run("sample_id", "--random_seed=9") == want_sample(sp, data, 10, 0.5, 9)[0]     # (n-best sampling: the defaults)
    assert run("sample_piece", "--nbest_size=-1", "--alpha=0.3", "--random_seed=9") == want_sample_pieces(sp, data, -1, 0.3, 9)
    assert run("sample_piece", "--random_seed=9") == want_sample_pieces(sp, data, 10, 0.5, 9)
    for fmt in ("proto", "sample_proto", "nbest_proto"):
        assert run(fmt) == b""
    assert subprocess.run([EXE, "--model=" + MODEL, "--input=" + src, "--output=" + out, "--output_format=nonsense"],
                          stderr=subprocess.PIPE).returncode == 1


@pytest.mark.gpu
def test_gpu_encode_file_chunk_independence(gpu, monkeypatch):
    """EncodeFile, and the draws' independence of the chunk size on the device."""
    sp, data, src, out, _ = gpu
    assert sp.EncodeFile(src, out, "sample_id", nbest_size=-1, alpha=0.3, seed=9)[0] == 300
    whole = open(out, "rb").read()
    assert whole == want_sample(sp, data, -1, 0.3, 9)[0]
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    sp.EncodeFile(src, out, "sample_id", nbest_size=-1, alpha=0.3, seed=9)
    assert open(out, "rb").read() == whole
    sp.EncodeFile(src, out, "nbest_id", nbest_size=3)
    assert open(out, "rb").read() == want_nbest(sp, data, 3)[0]
    sp.EncodeFile(src, out, "sample_piece", nbest_size=-1, alpha=0.3, seed=9)
    assert open(out, "rb").read() == want_sample_pieces(sp, data, -1, 0.3, 9)
    sp.EncodeFile(src, out, "nbest_piece", nbest_size=3)
    assert open(out, "rb").read() == want_nbest_pieces(sp, data, 3)
