#!/usr/bin/env python3
"""Rate of the E-step on the device: ExpectedCountsDevice (device buffers in, the accumulator left on the device: Normalize
kernels + lattice kernel mode 6 with one 64-bit atomic add per node) on

    words        the word list of bench.py's corpus builder (synth.WordList), every word one "sentence" whose weight is its
                 Zipf frequency scaled to a corpus of 10^9 words -- the shape of the unigram trainer's input
    sentences    sentences of that corpus builder (synth.ascii_corpus), weight 1

What one run of it gave is in DESIGN.md 4.4; whole calls by the host clock around a device synchronise, no kernel times.

    python scripts/estep_rate.py [sentences] [model]

One JSON line per shape."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    model = sys.argv[2] if len(sys.argv) > 2 else "uni32k"
    with open(os.path.join(ROOT, "tests", "golden", model + ".model"), "rb") as f:
        blob = f.read()
    sp = SentencePieceProcessor(model_proto=blob, device=0)
    dev = torch.device("cuda", 0)
    words = synth.WordList()
    p = np.diff(np.concatenate([[0.0], words.cdf]))
    w_offs = np.concatenate([words.offs, [len(words.blob)]]).astype(np.int64)
    w_freq = np.maximum(1, np.rint(p * 1e9)).astype(np.int64)
    s_text, s_offs = synth.ascii_corpus(n, seed=20250227)
    shapes = [("words (Zipf weights)", words.blob, w_offs, w_freq),
              ("sentences", s_text, np.asarray(s_offs).astype(np.int64), None)]
    for name, text, offs, freq in shapes:
        buf = torch.zeros(len(text) + 32, dtype=torch.uint8)
        buf[:len(text)] = torch.from_numpy(np.ascontiguousarray(text))
        d_text = buf.to(dev)[:len(text)]
        d_offs = torch.from_numpy(offs).to(dev)
        d_freq = None if freq is None else torch.from_numpy(freq.astype(np.uint32).view(np.int32)).to(dev)
        count = len(offs) - 1
        sp.ExpectedCountsDevice(d_text, d_offs, d_freq)              # warm: workspace, scratch
        torch.cuda.synchronize(dev)
        best, d_acc = None, None
        for _ in range(3):
            t0 = time.perf_counter()
            d_acc, d_z, d_v = sp.ExpectedCountsDevice(d_text, d_offs, d_freq)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        nodes = float(d_v.sum().item())
        print(json.dumps({"metric": "sentences/sec ExpectedCountsDevice, %s, %s, MI355X, device form" % (name, model),
                          "value": count / best, "unit": "sentences/s", "ms": best * 1e3, "sentences": count,
                          "bytes": int(len(text)), "MB/s": len(text) / best / 1e6,
                          "expected_tokens": float(d_acc.double().sum().item()) / 2.0 ** 24, "viterbi_nodes": nodes,
                          "objective": sp.EStepObjective(d_z.cpu().numpy(), freq)}))


if __name__ == "__main__":
    main()
