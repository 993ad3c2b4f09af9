#!/usr/bin/env python3
"""Rates of the file side of Encode -- never the headline metric (bench.py times the device-resident encode) -- on the C2
corpus (synth.ascii_corpus) at a reduced size:

  file_id      EncodeFile(corpus -> id lines): sentences/s, MB/s in and out (PCIe and the disk included); the image is
               written by the device formatter (csrc/kernels_tokentext.h)
  file_id_host the same with SPMX_ID_HOST_FORMAT=1: ids + offsets copied back, the host's formatting loop per worker
  file_piece   EncodeFile(corpus -> piece lines)
  pieces_packed / encode_as_pieces / encode_as_pieces_spt
               EncodePiecesPacked (arrays), EncodeAsPieces (Python lists of str) and the composition EncodeAsPieces had
               before the device piece writer (EncodeAsSentencePieceText's loop) on a list of sentences

Every figure is (min, median, max) over `reps` timed runs behind one warm-up run.  A tree without the piece format (an
earlier commit, for the A/B of format "id") reports what it has.

    python scripts/encode_file_rate.py [sentences] [model] [list sentences] [golden dir]
    (one JSON line, also written to profiles/r11_encode_file_rate.json)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sentencepiece_amd import synth  # noqa: E402
from sentencepiece_amd.processor import SentencePieceProcessor  # noqa: E402


def timed(fn, reps=5):
    """(min, median, max) wall seconds of `reps` runs behind a warm-up run, and the last result."""
    r = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return (ts[0], ts[len(ts) // 2], ts[-1]), r


def rate(ts, count):
    return {"ms_min_med_max": [round(t * 1e3, 3) for t in ts], "per_s_med": count / ts[1], "per_s_min_max": [count / ts[2], count / ts[0]]}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    model = sys.argv[2] if len(sys.argv) > 2 else "uni32k"
    n_list = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
    golden = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "tests", "golden")
    sp = SentencePieceProcessor(model_file=os.path.join(golden, model + ".model"))
    text, offs = synth.ascii_corpus(n, seed=20250227)
    out = {"sentences": n, "model": model, "list_sentences": n_list, "file_chunk": int(os.environ.get("SPMX_FILE_CHUNK", "0"))}
    with tempfile.TemporaryDirectory() as td:
        corpus, idp, idh, pcp = (os.path.join(td, x) for x in ("corpus.txt", "corpus.ids", "corpus.ids.host", "corpus.pieces"))
        lens = np.diff(offs.astype(np.int64))
        buf = np.full(len(text) + n, 0x0A, dtype=np.uint8)
        buf[np.repeat(np.arange(n), lens) + np.arange(len(text))] = text
        buf.tofile(corpus)
        in_mb = len(buf) / 1e6

        def file_rate(path, fmt):
            ts, (ns, ni) = timed(lambda: sp.EncodeFile(corpus, path, fmt))
            assert ns == n
            r = rate(ts, n)
            r.update(ids=ni, mb_in_per_s_med=in_mb / ts[1], mb_out_per_s_med=os.path.getsize(path) / 1e6 / ts[1])
            return r
        out["file_id"] = file_rate(idp, "id")
        os.environ["SPMX_ID_HOST_FORMAT"] = "1"
        try:
            out["file_id_host"] = file_rate(idh, "id")
        finally:
            del os.environ["SPMX_ID_HOST_FORMAT"]
        with open(idp, "rb") as a, open(idh, "rb") as b:
            assert a.read() == b.read()
        try:
            out["file_piece"] = file_rate(pcp, "piece")
        except RuntimeError as e:
            out["file_piece"] = {"unavailable": str(e)}

    lt, lo = text[:int(offs[n_list])], offs[:n_list + 1]
    blob = lt.tobytes()
    lo64 = lo.astype(np.int64)
    items = [blob[lo64[i]:lo64[i + 1]] for i in range(n_list)]        # (bytes: the corpus has sentences that are not UTF-8)
    if hasattr(sp, "EncodePiecesPacked"):
        ts, r = timed(lambda: sp.EncodePiecesPacked(lt, lo), reps=3)
        out["pieces_packed"] = rate(ts, n_list)
        out["pieces_packed"].update(pieces=len(r[0]), piece_bytes=len(r[2]))
    ts, rows = timed(lambda: sp.EncodeAsPieces(items), reps=3)
    out["encode_as_pieces"] = rate(ts, n_list)

    def spt_route():
        return [[p.decode("utf-8", "surrogateescape") for p, *_ in row] for row in sp.EncodeAsSentencePieceText(items)]
    ts, old_rows = timed(spt_route, reps=2)
    assert old_rows == rows
    out["encode_as_pieces_spt"] = rate(ts, n_list)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r11_encode_file_rate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
