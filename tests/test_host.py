"""The host-buffer side of the boundary: the chunk pipeline of spmx_encode_batch, the
(pointer, length) form behind EncodeBatch(vector<string_view>), concurrent callers on one handle, and the corpus file
tool -- on the CPU with the device emulated (tests/emulib.py), on the GPU with -m gpu."""
import ctypes as C
import hashlib
import os
import threading

import numpy as np
import pytest

from tests import fixtures

# the survey's known answer: `spm_encode --model=test_model.model --output_format=id < botchan.txt | md5sum`
BOTCHAN_ID_MD5 = "ff197d02d69c7695fccfec3bac27bf7a"


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.EmuLib()


def views_call(lib, handle, bufs):
    class V(C.Structure):
        _fields_ = [("data", C.c_char_p), ("len", C.c_uint64)]
    arr = (V * len(bufs))(*[V(b, len(b)) for b in bufs])
    p_ids, p_off, p_st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nf = C.c_uint64(0)
    rc = lib.spmx_encode_batch_views(handle, arr, len(bufs), C.byref(p_ids), C.byref(p_off), C.byref(p_st), C.byref(nf))
    assert rc == 0, lib.spmx_last_error(None)
    n = len(bufs)
    io = np.ctypeslib.as_array(C.cast(p_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    ids = (np.ctypeslib.as_array(C.cast(p_ids, C.POINTER(C.c_int32)), shape=(int(io[n]),)).copy() if io[n] else np.zeros(0, np.int32))
    for p in (p_ids, p_off, p_st):
        lib.spmx_free(p)
    return ids, io


@pytest.mark.parametrize("model", ["uni32k", "bpe32k", "uni1k_bf"])
def test_emu_chunk_pipeline_and_views(model, emu, oracle, corpora):
    """A batch big enough for the chunk pipeline (chunks of 1024 sentences here, 3 workers): the same CSR as the oracle's,
    through the packed form and through the (pointer, length) form."""
    blob = fixtures.model_blob(model)
    h = emu.load(blob, classes=None, env={"SPMX_HOST_CHUNK": "1024", "SPMX_HOST_THREADS": "3"})
    o = oracle.load(blob)
    text, offs = fixtures.head(*corpora["synth20k"], 6500)
    ids, io = h.encode_batch(text, offs)
    oids, oio = o.encode_batch(text, offs)
    np.testing.assert_array_equal(io, oio)
    np.testing.assert_array_equal(ids, oids)
    assert not h.sent_status.any()
    tb = np.asarray(text).tobytes()
    bufs = [tb[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
    vids, vio = views_call(h.lib, h.sp._h, bufs)
    np.testing.assert_array_equal(vio, oio)
    np.testing.assert_array_equal(vids, oids)


def test_emu_concurrent_callers(emu, oracle, corpora):
    """Encode is const in the reference and may be called from several threads at once: here every call leases its own
    workspace and stream."""
    blob = fixtures.model_blob("test_model")
    h, o = emu.load(blob), oracle.load(blob)
    parts = [fixtures.head(*corpora[name], k) for name, k in (("botchan", 400), ("edge", 10 ** 6), ("synth20k", 500), ("mixed2k", 60))]
    want = [o.encode_batch(t, of) for t, of in parts]
    got = [None] * len(parts)

    def run(i):
        for _ in range(3):
            got[i] = h.sp.EncodePacked(*parts[i])
    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(parts))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for (ids, io), (oids, oio) in zip(got, want):
        np.testing.assert_array_equal(io, oio)
        np.testing.assert_array_equal(ids, oids)


def test_emu_encode_file(emu, tmp_path):
    """spmx_encode_file, format "id": the bytes `spm_encode --output_format=id` writes for botchan.txt with the bundled
    model (95,515 tokens, md5 ff197d02...); format "bin": the same ids, flat."""
    h = emu.load(fixtures.model_blob("test_model"), classes=None)
    src = os.path.join(fixtures.GOLDEN, "botchan.txt")
    out = str(tmp_path / "ids.txt")
    ns, ni = h.sp.EncodeFile(src, out, "id")
    assert (ns, ni) == (4288, 95515)
    data = open(out, "rb").read()
    assert hashlib.md5(data).hexdigest() == BOTCHAN_ID_MD5
    outb = str(tmp_path / "ids.bin")
    assert h.sp.EncodeFile(src, outb, "bin") == (4288, 95515)
    ids = np.fromfile(outb, dtype=np.int32)
    io = np.fromfile(outb + ".idx", dtype=np.uint64)
    assert len(io) == 4289 and int(io[-1]) == 95515 == len(ids)
    lines = data.decode().split("\n")[:-1]
    assert [int(x) for x in lines[7].split()] == ids[int(io[7]):int(io[8])].tolist()


BOTCHAN = os.path.join(fixtures.GOLDEN, "botchan.txt")


def read_bin(path):
    return np.fromfile(path, dtype=np.int32), np.fromfile(path + ".idx", dtype=np.uint64)


def count_file(sp, path):
    """spmx_count_file -> (status, counts, n_sentences, n_ids)."""
    counts = np.zeros(sp.GetPieceSize() + 1, dtype=np.uint64)
    ns, ni = C.c_uint64(0), C.c_uint64(0)
    rc = sp._lib.spmx_count_file(sp._h, path.encode(), counts.ctypes.data, C.byref(ns), C.byref(ni))
    return rc, counts, ns.value, ni.value


@pytest.fixture(scope="module")
def botchan_one_chunk(emu, tmp_path_factory):
    """botchan.txt as one chunk: (ids, offsets) of format "bin" and the histogram of spmx_count_file."""
    sp = emu.load(fixtures.model_blob("test_model"), classes=None).sp
    out = str(tmp_path_factory.mktemp("one_chunk") / "ids.bin")
    assert "SPMX_FILE_CHUNK" not in os.environ
    assert sp.EncodeFile(BOTCHAN, out, "bin") == (4288, 95515)
    rc, counts, ns, ni = count_file(sp, BOTCHAN)
    assert (rc, ns, ni) == (0, 4288, 95515) and int(counts.sum()) == 95515
    return read_bin(out) + (counts,)


def check_chunked_file_calls(sp, want, tmp_path):
    """Formats "id" and "bin" and the histogram, SPMX_FILE_CHUNK set by the caller: what one chunk gives."""
    ids, io, counts = want
    out, outb = str(tmp_path / "ids.txt"), str(tmp_path / "ids.bin")
    assert sp.EncodeFile(BOTCHAN, out, "id") == (4288, 95515)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == BOTCHAN_ID_MD5
    assert sp.EncodeFile(BOTCHAN, outb, "bin") == (4288, 95515)
    got_ids, got_io = read_bin(outb)
    np.testing.assert_array_equal(got_io, io)
    np.testing.assert_array_equal(got_ids, ids)
    rc, got, ns, ni = count_file(sp, BOTCHAN)
    assert (rc, ns, ni) == (0, 4288, 95515)
    np.testing.assert_array_equal(got, counts)


@pytest.mark.parametrize("threads", ["1", "4"])
def test_emu_file_calls_chunked(threads, emu, botchan_one_chunk, tmp_path, monkeypatch):
    """More than 50 chunks of 4 KiB through one worker and through four: spmx_encode_file's "id" (on the device and on the
    host's formatting loop) and "bin" and spmx_count_file give what one chunk gives."""
    sp = emu.load(fixtures.model_blob("test_model"), classes=None, env={"SPMX_HOST_THREADS": threads}).sp
    assert os.path.getsize(BOTCHAN) > 50 * 4096
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    check_chunked_file_calls(sp, botchan_one_chunk, tmp_path)
    monkeypatch.setenv("SPMX_ID_HOST_FORMAT", "1")
    out = str(tmp_path / "ids_host.txt")
    assert sp.EncodeFile(BOTCHAN, out, "id") == (4288, 95515)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == BOTCHAN_ID_MD5


def test_emu_file_calls_second_attempt(emu, oracle, tmp_path):
    """The grow-and-retry helper's second attempt inside the file calls, made certain: lines of punctuation give about
    one id per byte, more than the id arena holds after its first reservation (the guess of one id per two bytes and 4 per
    line + 64, a quarter and 79 on top at the most), so the encode runs again at the reported need.  A fresh handle per
    call: a workspace keeps what it has grown to."""
    blob = fixtures.model_blob("test_model")
    lines = [b";.,!" * 60, b",;" * 300, b"Hello world.", b"!.;," * 150]
    text = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
    oids, oio = oracle.load(blob).encode_batch(text, offs)
    guess = len(text) // 2 + 4 * len(lines) + 64
    assert len(oids) > guess + guess // 4 + 79
    sp = emu.load(blob, classes=None).sp
    src, out = str(tmp_path / "punct.txt"), str(tmp_path / "punct.bin")
    with open(src, "wb") as f:
        f.write(b"\n".join(lines) + b"\n")
    assert sp.EncodeFile(src, out, "bin") == (len(lines), len(oids))
    ids, io = read_bin(out)
    np.testing.assert_array_equal(io, oio)
    np.testing.assert_array_equal(ids, oids)
    rc, counts, ns, ni = count_file(emu.load(blob, classes=None).sp, src)
    assert (rc, ns, ni) == (0, len(lines), len(oids))
    np.testing.assert_array_equal(counts[:-1], np.bincount(oids, minlength=sp.GetPieceSize()))


def test_emu_file_call_failures(emu, tmp_path):
    """A missing input and an output that cannot be opened, ten times each: the status and text, no descriptor left open,
    and the handle encodes the file afterwards (nothing left locked or leased)."""
    sp = emu.load(fixtures.model_blob("test_model"), classes=None, env={"SPMX_HOST_THREADS": "4"}).sp
    lib, missing, nodir = sp._lib, str(tmp_path / "nothing"), str(tmp_path / "no_such_dir" / "out")
    ns, ni = C.c_uint64(0), C.c_uint64(0)
    counts = np.ones(sp.GetPieceSize() + 1, dtype=np.uint64)
    head, head_out = str(tmp_path / "head.txt"), str(tmp_path / "head.ids")
    with open(head, "wb") as f:
        f.write(b"".join(open(BOTCHAN, "rb").readlines()[:40]))
    assert sp.EncodeFile(head, head_out, "id")[0] == 40
    head_want = open(head_out, "rb").read()
    assert head_want.count(b"\n") == 40

    def works():
        assert sp.EncodeFile(head, head_out, "id")[0] == 40 and open(head_out, "rb").read() == head_want

    def failing_calls():
        for fmt in (b"id", b"piece", b"bin"):
            assert lib.spmx_encode_file(sp._h, missing.encode(), str(tmp_path / "o").encode(), fmt, C.byref(ns), C.byref(ni)) == 5
            assert lib.spmx_last_error(sp._h).decode() == '"%s": No such file or directory' % missing
            works()
            assert lib.spmx_encode_file(sp._h, BOTCHAN.encode(), nodir.encode(), fmt, C.byref(ns), C.byref(ni)) == 7
            assert lib.spmx_last_error(sp._h).decode() == 'cannot write "%s"' % nodir
            works()
        assert count_file(sp, missing)[0] == 5
        assert lib.spmx_last_error(sp._h).decode() == '"%s": No such file or directory' % missing
        works()
        assert lib.spmx_write_vocabulary(sp._h, counts.ctypes.data, nodir.encode(), C.byref(ns)) == 7
        assert lib.spmx_last_error(sp._h).decode() == 'cannot write "%s"' % nodir
        works()
    failing_calls()                               # (whatever the first calls open for good is open now)
    fds = len(os.listdir("/proc/self/fd")) if os.path.isdir("/proc/self/fd") else None
    for _ in range(10):
        failing_calls()
    if fds is not None:
        assert len(os.listdir("/proc/self/fd")) == fds
    out = str(tmp_path / "ids.txt")
    assert sp.EncodeFile(BOTCHAN, out, "id") == (4288, 95515)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == BOTCHAN_ID_MD5
    rc, got, n_sent, n_ids = count_file(sp, BOTCHAN)
    assert (rc, n_sent, n_ids, int(got.sum())) == (0, 4288, 95515, 95515)


@pytest.mark.gpu
def test_gpu_file_calls_chunked(tmp_path, monkeypatch):
    """test_emu_file_calls_chunked on the device, four workers on four streams: the order of the chunks in the output."""
    from sentencepiece_amd.processor import SentencePieceProcessor
    model = os.path.join(fixtures.GOLDEN, "test_model.model")
    monkeypatch.setenv("SPMX_HOST_THREADS", "4")
    sp = SentencePieceProcessor(model_file=model)
    outb = str(tmp_path / "one.bin")
    assert sp.EncodeFile(BOTCHAN, outb, "bin") == (4288, 95515)
    rc, counts, ns, ni = count_file(sp, BOTCHAN)
    assert (rc, ns, ni) == (0, 4288, 95515)
    monkeypatch.setenv("SPMX_FILE_CHUNK", "4096")
    check_chunked_file_calls(sp, read_bin(outb) + (counts,), tmp_path)


@pytest.mark.gpu
def test_gpu_encode_file_and_cli(tmp_path):
    """The same known answer on the GPU, through the Python wrapper and through the spmx_encode command line."""
    import subprocess
    from sentencepiece_amd.processor import SentencePieceProcessor
    model = os.path.join(fixtures.GOLDEN, "test_model.model")
    src = os.path.join(fixtures.GOLDEN, "botchan.txt")
    sp = SentencePieceProcessor(model_file=model)
    out = str(tmp_path / "ids.txt")
    assert sp.EncodeFile(src, out, "id") == (4288, 95515)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == BOTCHAN_ID_MD5
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sentencepiece_amd", "spmx_encode")
    r = subprocess.run([exe, "--model=" + model, "--output_format=id", src], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert hashlib.md5(r.stdout).hexdigest() == BOTCHAN_ID_MD5


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["uni32k", "bpe32k"])
def test_gpu_chunk_pipeline(model, oracle):
    """2.2 M sentences through the host-buffer form (chunk pipeline: 8 workers) and the (pointer, length) form: a strided
    sample equals the oracle's ids, and both forms agree everywhere."""
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    blob = fixtures.model_blob(model)
    sp = SentencePieceProcessor(model_proto=blob)
    text, offs = synth.ascii_corpus(2_200_000, seed=5)
    ids, io, st, failed = sp.EncodePackedEx(text, offs)
    assert failed == 0 and not st.any()
    pick = np.arange(0, len(offs) - 1, 997)
    pt, po = synth.gather_packed(text, offs, pick)
    oids, oio = oracle.load(blob).encode_batch(pt, po)
    cnt = np.diff(io.astype(np.int64))
    np.testing.assert_array_equal(cnt[pick], np.diff(oio.astype(np.int64)))
    got = np.concatenate([ids[int(io[i]):int(io[i + 1])] for i in pick])
    np.testing.assert_array_equal(got, oids)
    d_ids, d_io, total = None, None, None
    import torch
    d_text = torch.from_numpy(text).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_ids, d_io, total = sp.EncodeDevice(d_text, d_offs)
    np.testing.assert_array_equal(d_io.cpu().numpy().astype(np.uint64), io)
    np.testing.assert_array_equal(d_ids[:total].cpu().numpy(), ids)


def test_emu_encode_batch_multi(emu, oracle, corpora):
    """spmx_encode_batch_multi: three handles (three GPUs of a node; here three emulated devices) share the chunks of one
    batch and fill one CSR."""
    blob = fixtures.model_blob("uni32k")
    env = {"SPMX_HOST_CHUNK": "1024", "SPMX_HOST_THREADS": "2"}
    hs = [emu.load(blob, classes=None, env=env) for _ in range(3)]
    text, offs = fixtures.head(*corpora["synth20k"], 9000)
    text, offs = np.ascontiguousarray(text), np.ascontiguousarray(offs, dtype=np.uint64)
    arr = (C.c_void_p * 3)(*[h.sp._h for h in hs])
    p_ids, p_off, p_st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nf = C.c_uint64(0)
    n = len(offs) - 1
    lib = hs[0].lib
    rc = lib.spmx_encode_batch_multi(arr, 3, text.ctypes.data, offs.ctypes.data, n, C.byref(p_ids), C.byref(p_off), C.byref(p_st), C.byref(nf))
    assert rc == 0, lib.spmx_last_error(None)
    io = np.ctypeslib.as_array(C.cast(p_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    ids = np.ctypeslib.as_array(C.cast(p_ids, C.POINTER(C.c_int32)), shape=(int(io[n]),)).copy()
    for p in (p_ids, p_off, p_st):
        lib.spmx_free(p)
    oids, oio = oracle.load(blob).encode_batch(text, offs)
    np.testing.assert_array_equal(io, oio)
    np.testing.assert_array_equal(ids, oids)


def test_emu_degenerate_batches(emu, oracle):
    """Empty batches, empty sentences and null pointers through every host form: the reference's batch is a loop of
    Encode calls, so n = 0 gives an empty CSR and an empty sentence an empty id range (bos / eos when asked for)."""
    blob = fixtures.model_blob("test_model")
    h, o = emu.load(blob), oracle.load(blob)
    lib = h.lib
    # n = 0 through the packed form
    p_ids, p_off = C.c_void_p(), C.c_void_p()
    offs0 = np.zeros(1, dtype=np.uint64)
    assert lib.spmx_encode_batch(h.sp._h, None, offs0.ctypes.data, 0, C.byref(p_ids), C.byref(p_off)) == 0
    assert np.ctypeslib.as_array(C.cast(p_off, C.POINTER(C.c_uint64)), shape=(1,))[0] == 0
    lib.spmx_free(p_ids); lib.spmx_free(p_off)
    # n = 0 and empty views
    ids, io = views_call(lib, h.sp._h, [])
    assert len(ids) == 0 and io.tolist() == [0]
    ids, io = views_call(lib, h.sp._h, [b"", b"a", b"", b""])
    want, wio = o.encode_batch(*__import__("sentencepiece_amd.synth", fromlist=["pack"]).pack([b"", b"a", b"", b""]))
    np.testing.assert_array_equal(io, wio)
    np.testing.assert_array_equal(ids, want)
    # empty sentences keep their bos / eos
    h.set_encode_extra_options("bos:eos")
    o.set_encode_extra_options("bos:eos")
    ids, io = views_call(lib, h.sp._h, [b"", b" ", b"x"])
    want, wio = o.encode_batch(*__import__("sentencepiece_amd.synth", fromlist=["pack"]).pack([b"", b" ", b"x"]))
    np.testing.assert_array_equal(io, wio)
    np.testing.assert_array_equal(ids, want)
    # null output containers are an error, not a crash
    assert lib.spmx_encode_batch(h.sp._h, None, offs0.ctypes.data, 0, None, None) != 0
    # the lattice entry points on an empty batch
    h.set_encode_extra_options("")
    for fn in (lambda: h.sp.SampleEncodePacked(np.zeros(0, np.uint8), offs0, -1, 0.1), lambda: h.sp.EncodeOriginalPacked(np.zeros(0, np.uint8), offs0)):
        ids, io = fn()
        assert len(ids) == 0 and io.tolist() == [0]
