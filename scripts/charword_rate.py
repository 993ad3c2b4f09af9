#!/usr/bin/env python3
"""One-GPU rates of the character and word models (csrc/kernels_charword.h), run by hand on a machine with an MI355X:

    python scripts/charword_rate.py [--sentences 10000000] [--steps 5] [--warmup 2] [--out profiles/r09_charword_rate.json]

For tests/golden/char1k.model and word1k.model, on the benchmark's synthetic ASCII batch (sentencepiece_amd/synth.py
ascii_corpus, the seed bench.py uses) and on one document shape (2048 documents of 16 KiB):
  * sentences/s and GB of text/s of the device-resident encode (device events around `steps` calls after `warmup`);
  * EVERY sentence's ids compared with the compiled reference (oracle/_ref): the count of differing sentences, which must
    be 0 for the figures to mean anything;
  * the compiled reference on this machine's host at one thread and at its best thread count of 1 .. 16;
  * the bytes the algorithm needs per sentence, L + 4 T + 16 (text read once, ids written once, two offsets), over the
    step time, as a share of what a streaming kernel reaches on this chip -- an END-TO-END figure, not a kernel's;
  * which kernel dominates: the per-launch times of the product's own profile of one more step.
  * a `rocprofv3 --kernel-trace --stats` summary of one step per model (a run of its own, the profiler off everywhere
    else): profiles/r09_charword_kernel_stats_<model>.csv.
Every GPU step is a child process of its own under `timeout`; after a step that fails nothing else is started.  Without
the compiled reference nothing is written: a rate without the 0-differ comparison is not a result.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS = 6300.0     # what a streaming kernel reaches on an MI355X (of 8 TB/s nominal)
SEED = 20250227
MODELS = ("char1k", "word1k")
SHAPES = ("synthetic", "docs_16k")


def make_batch(shape, sentences):
    from sentencepiece_amd import synth
    if shape == "synthetic":
        return synth.ascii_corpus(sentences, seed=SEED)
    text, offs = synth.ascii_corpus(400_000, seed=SEED + 1)
    flat = np.frombuffer(b" ".join(synth.unpack(text, offs)), dtype=np.uint8)
    n_docs, size = 2048, 16384
    body = np.tile(flat, -(-n_docs * size // len(flat)))[:n_docs * size].copy()
    return body, np.arange(0, (n_docs + 1) * size, size, dtype=np.uint64)


def child(model, shape, sentences, steps, warmup, compare=True):
    """One (model, shape) on the GPU -> one JSON line."""
    import torch
    from sentencepiece_amd.processor import SentencePieceProcessor
    from tests import refshim
    with open(os.path.join(ROOT, "tests", "golden", model + ".model"), "rb") as f:
        blob = f.read()
    text, offs = make_batch(shape, sentences)
    n = len(offs) - 1
    sp = SentencePieceProcessor(model_proto=blob, device=0)
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.asarray(text)).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_ids, d_io, total = sp.EncodeDevice(d_text, d_offs)
    for _ in range(warmup):
        d_ids, d_io, total = sp.EncodeDevice(d_text, d_offs, d_ids=d_ids, d_id_offsets=d_io)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d_ids, d_io, total = sp.EncodeDevice(d_text, d_offs, d_ids=d_ids, d_id_offsets=d_io)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    sp.SetProfiling(True)
    sp.EncodeDevice(d_text, d_offs, d_ids=d_ids, d_id_offsets=d_io)
    prof = sp.LastProfile()
    sp.SetProfiling(False)
    ids = d_ids[:total].cpu().numpy()
    io = d_io.cpu().numpy().astype(np.uint64)
    out = {"model": model, "shape": shape, "sentences": int(n), "text_bytes": int(len(text)), "ids": int(total), "step_ms": ms}
    best = min(ms)
    out["sentences_per_s"] = n / best * 1e3
    out["text_gb_per_s"] = len(text) / best / 1e6
    alg = len(text) + 4 * int(total) + 16 * n
    out["algorithmic_bytes_per_sentence"] = alg / n
    out["share_of_streaming_peak_end_to_end"] = alg / best / 1e6 / HBM_ACHIEVABLE_GBS
    out["launches_ms"] = {c["kernel"]: c["kernel_ms"] for c in prof["classes"] if c["kernel"]}
    if not compare:
        print(json.dumps(out))
        return 0
    if refshim.available():
        r = refshim.RefLib().load(blob)
        host = {}
        sub = min(n, 200_000)                                # (the host legs on a prefix: the reference is ~10^4 times slower)
        st, so = text[:int(offs[sub])], offs[:sub + 1]
        for threads in (1, 2, 4, 8, 16):
            t0 = time.perf_counter()
            r.encode_count(st, so, threads=threads)
            host[threads] = sub / (time.perf_counter() - t0)
        out["reference_host_sentences_per_s"] = {"one_thread": host[1], "best": max(host.values()),
                                                 "best_threads": max(host, key=host.get), "on_sentences": sub}
        rids, rio = r.encode_batch(text, offs, threads=16)
        differ = int(n) if len(rio) != len(io) else int(np.count_nonzero(np.diff(rio.astype(np.int64)) != np.diff(io.astype(np.int64))))
        if differ == 0 and not np.array_equal(rids, ids):
            bad = np.flatnonzero(rids != ids)
            differ = int(len(np.unique(np.searchsorted(io, bad, side="right"))))
        out["sentences_differing_from_the_reference"] = differ
    print(json.dumps(out))
    return 0 if out.get("sentences_differing_from_the_reference") == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_charword_rate.json"))
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a (model, shape) child may take")
    ap.add_argument("--child", nargs=2, metavar=("MODEL", "SHAPE"), default=None)
    ap.add_argument("--no-compare", action="store_true", help="(child, under the profiler) time only")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.sentences, a.steps, a.warmup, compare=not a.no_compare)
    from tests import refshim
    if not refshim.available():
        print("charword_rate: oracle/_ref is not built; without the comparison with the compiled reference no rate is recorded", file=sys.stderr)
        return 1
    records = []
    for model in MODELS:
        for shape in SHAPES:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", model, shape,
                   "--sentences", str(a.sentences), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = [ln for ln in p.stdout.split("\n") if ln.startswith("{")]
            if p.returncode != 0 or not line:
                print("charword_rate: %s / %s ended with status %d; nothing more is started\n%s" % (model, shape, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return 1
            records.append(json.loads(line[-1]))
            print(line[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    # one step per model under the kernel trace, each a run of its own (--no-compare: the trace is of the encode, the
    # comparison was made above)
    import glob
    import shutil
    import tempfile
    for model in MODELS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--child", model, "synthetic", "--sentences", str(min(a.sentences, 2_000_000)),
                   "--steps", "1", "--warmup", "1", "--no-compare"]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
            if p.returncode != 0 or not stats:
                print("charword_rate: the kernel trace of %s ended with status %d; nothing more is started\n%s" % (model, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return 1
            shutil.copy(stats[0], os.path.join(os.path.dirname(a.out), "r09_charword_kernel_stats_%s.csv" % model))
    with open(a.out, "w") as f:
        json.dump({"what": "scripts/charword_rate.py on one MI355X; rates from the fastest of step_ms", "records": records}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
