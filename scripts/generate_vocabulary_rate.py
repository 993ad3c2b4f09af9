#!/usr/bin/env python3
"""Rates of the piece counts (csrc/kernels_piececount.h) -- never the headline metric (bench.py times the device-resident
encode):

  count_kernel   CountIdsDevice on a device-resident id array (the ids of the C2 corpus, synth.ascii_corpus, encoded once):
                 ids/s and GB/s of ids read, timed with events around `inner` back-to-back calls
  bincount       torch.bincount on the same tensor (as int64, the conversion not timed): the yardstick
  count_file     spmx_count_file of the corpus file (what GenerateVocabulary runs per input): sentences/s, MB/s in
  file_bin       EncodeFile(corpus, "bin") of the same file: what counting adds to -- or saves against -- encoding to a
                 file can be read off the two

Every figure is (min, median, max) over `reps` timed runs behind one warm-up run.

    python scripts/generate_vocabulary_rate.py [sentences] [model] [golden dir]
    (one JSON line, also written to profiles/r12_generate_vocabulary_rate.json)
"""
import ctypes as C
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


def device_timed(fn, inner=10, reps=5):
    """(min, median, max) seconds per call: events around `inner` calls enqueued back to back."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3 / inner)
    ts.sort()
    return ts[0], ts[len(ts) // 2], ts[-1]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    model = sys.argv[2] if len(sys.argv) > 2 else "uni32k"
    golden = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden")
    sp = SentencePieceProcessor(model_file=os.path.join(golden, model + ".model"))
    V = sp.GetPieceSize()
    text, offs = synth.ascii_corpus(n, seed=20250227)
    out = {"sentences": n, "model": model, "pieces": V, "lds_bins": int(os.environ.get("SPMX_COUNT_LDS_BINS", "0")),
           "file_chunk": int(os.environ.get("SPMX_FILE_CHUNK", "0"))}

    ids, _ = sp.EncodePacked(text, offs)
    d_ids = torch.from_numpy(ids).to("cuda:0")
    d_counts = torch.zeros(V + 1, dtype=torch.int64, device="cuda:0")
    ts = device_timed(lambda: sp.CountIdsDevice(d_ids, d_counts))
    out["count_kernel"] = rate(ts, len(ids))
    out["count_kernel"].update(ids=len(ids), gb_per_s_med=4 * len(ids) / 1e9 / ts[1])
    d_wide = d_ids.to(torch.int64)
    ts = device_timed(lambda: torch.bincount(d_wide, minlength=V + 1))
    out["bincount"] = rate(ts, len(ids))
    assert torch.equal(sp.CountIdsDevice(d_ids), torch.bincount(d_wide, minlength=V + 1))

    with tempfile.TemporaryDirectory() as td:
        corpus, binp = os.path.join(td, "corpus.txt"), os.path.join(td, "corpus.bin")
        lens = np.diff(offs.astype(np.int64))
        buf = np.full(len(text) + n, 0x0A, dtype=np.uint8)
        buf[np.repeat(np.arange(n), lens) + np.arange(len(text))] = text
        buf.tofile(corpus)
        in_mb = len(buf) / 1e6

        def count_file():
            counts = np.zeros(V + 1, dtype=np.uint64)
            ns, ni = C.c_uint64(0), C.c_uint64(0)
            sp._check(sp._lib.spmx_count_file(sp._h, os.fsencode(corpus), counts.ctypes.data, C.byref(ns), C.byref(ni)))
            return counts, int(ns.value), int(ni.value)
        ts, (counts, ns, ni) = timed(count_file)
        assert ns == n and ni == len(ids) and np.array_equal(counts, np.bincount(ids, minlength=V + 1).astype(np.uint64))
        out["count_file"] = rate(ts, n)
        out["count_file"].update(ids=ni, mb_in_per_s_med=in_mb / ts[1])
        ts, (ns, ni) = timed(lambda: sp.EncodeFile(corpus, binp, "bin"))
        assert ns == n
        out["file_bin"] = rate(ts, n)
        out["file_bin"].update(ids=ni, mb_in_per_s_med=in_mb / ts[1])
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r12_generate_vocabulary_rate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
