#!/usr/bin/env python3
"""Rates of the file side of Decode -- never the headline metric (bench.py times the device-resident encode) -- on an id
file that EncodeFile made from the C2 corpus (synth.ascii_corpus):

  file      DecodeFile(ids file -> text file), "id" and "bin": MB/s of input and output, lines/s (PCIe and the disk included)
  parser    ParseIdLinesDevice on the whole image in HBM, between two events on its stream (count pass, two scans, the
            read-back of the totals, write pass) against its byte model: the image read twice + 4 T + 8 n written
  joiner    JoinLinesDevice on the decoded text, likewise: text and offsets read once, text + n written
  host      the route a user had before DecodeFile: Python line split + int() + DecodePacked + join + write

    python scripts/decode_file_rate.py [sentences] [model]     (one JSON line, also written to profiles/r10_decode_file_rate.json)
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


def best_of(fn, reps=3):
    """Best wall time of reps - 1 runs behind a warm-up run."""
    best, r = None, None
    for it in range(reps):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        if it > 0 and (best is None or dt < best):
            best = dt
    return best, r


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    model = sys.argv[2] if len(sys.argv) > 2 else "uni32k"
    sp = SentencePieceProcessor(model_file=os.path.join(ROOT, "tests", "golden", model + ".model"))
    text, offs = synth.ascii_corpus(n, seed=20250227)
    out = {"sentences": n, "model": model, "file_chunk": int(os.environ.get("SPMX_FILE_CHUNK", "0"))}
    with tempfile.TemporaryDirectory() as td:
        corpus, idp, binp, txt = (os.path.join(td, x) for x in ("corpus.txt", "corpus.ids", "corpus.bin", "decoded.txt"))
        lens = np.diff(offs.astype(np.int64))
        buf = np.full(len(text) + n, 0x0A, dtype=np.uint8)
        buf[np.repeat(np.arange(n), lens) + np.arange(len(text))] = text
        buf.tofile(corpus)
        assert sp.EncodeFile(corpus, idp, "id")[0] == n
        sp.EncodeFile(corpus, binp, "bin")
        id_bytes = os.path.getsize(idp)

        dt, (lines, ids) = best_of(lambda: sp.DecodeFile(idp, txt, "id"))
        txt_bytes = os.path.getsize(txt)
        out.update(ids=ids, id_file_mb=id_bytes / 1e6, text_file_mb=txt_bytes / 1e6)
        out["file_id"] = {"ms": dt * 1e3, "lines_per_s": lines / dt, "mb_in_per_s": id_bytes / dt / 1e6, "mb_out_per_s": txt_bytes / dt / 1e6}
        with open(txt, "rb") as f:
            decoded = f.read()
        dt, _ = best_of(lambda: sp.DecodeFile(binp, txt, "bin"))
        with open(txt, "rb") as f:
            assert f.read() == decoded
        out["file_bin"] = {"ms": dt * 1e3, "lines_per_s": lines / dt, "mb_in_per_s": (4 * ids + 8 * (n + 1)) / dt / 1e6,
                           "mb_out_per_s": txt_bytes / dt / 1e6}

        # the two kernels by themselves, device-resident
        image = np.fromfile(idp, dtype=np.uint8)
        d_file = torch.zeros(len(image) + 16, dtype=torch.uint8, device="cuda:0")[:len(image)]
        d_file.copy_(torch.from_numpy(image))
        stream = torch.cuda.current_stream()

        def timed_ms(fn, reps=5):
            best, r = None, None
            for it in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r = fn()
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if it > 0 and (best is None or ms < best):
                    best = ms
            return best, r
        ms, (d_ids, d_io, nl, nt) = timed_ms(lambda: sp.ParseIdLinesDevice(d_file))
        assert (nl, nt) == (n, ids)
        model_bytes = 2 * id_bytes + 4 * nt + 8 * nl
        out["parser"] = {"ms": ms, "model_bytes": model_bytes, "gb_per_s_of_model": model_bytes / ms / 1e6,
                         "image_gb_per_s": id_bytes / ms / 1e6}
        d_text, d_to, total = sp.DecodeDevice(d_ids, d_io)
        ms, d_image = timed_ms(lambda: sp.JoinLinesDevice(d_text[:total], d_to))
        assert d_image.numel() == txt_bytes and d_image.cpu().numpy().tobytes() == decoded
        model_bytes = total + 8 * (nl + 1) + total + nl
        out["joiner"] = {"ms": ms, "model_bytes": model_bytes, "gb_per_s_of_model": model_bytes / ms / 1e6}

        # what a user did before: every step of the file workflow in Python around DecodePacked
        def host_route():
            with open(idp, "rb") as f:
                rows = f.read().split(b"\n")
            if rows and rows[-1] == b"":
                rows.pop()
            flat, io = [], np.zeros(len(rows) + 1, dtype=np.uint64)
            for i, row in enumerate(rows):
                flat.extend(int(t) for t in row.split(b" ") if t)
                io[i + 1] = len(flat)
            t, to = sp.DecodePacked(np.asarray(flat, dtype=np.int32), io)
            t, to = t.tobytes(), to.astype(np.int64)
            with open(txt, "wb") as f:
                f.write(b"".join(t[to[i]:to[i + 1]] + b"\n" for i in range(len(rows))))
        dt, _ = best_of(host_route, reps=2)
        with open(txt, "rb") as f:
            assert f.read() == decoded
        out["host_route"] = {"ms": dt * 1e3, "lines_per_s": n / dt, "mb_in_per_s": id_bytes / dt / 1e6}
        out["file_id_over_host_route"] = out["host_route"]["ms"] / out["file_id"]["ms"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r10_decode_file_rate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
