#!/usr/bin/env python3
"""Rates of the device lattice scoring calls (host-buffer form: H2D + Normalize kernels + lattice kernel + D2H + host
CSR): CalculateEntropyPacked and SampleEncodeAndScorePacked with and without replacement, on the corpus builder of
bench.py.  Nothing has been measured with it yet: no rate is stated anywhere in the documents.

    python scripts/lattice_score_rate.py [sentences] [num_samples] [model]

One JSON line per call."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    model = sys.argv[3] if len(sys.argv) > 3 else "uni32k"
    with open(os.path.join(ROOT, "tests", "golden", model + ".model"), "rb") as f:
        blob = f.read()
    sp = SentencePieceProcessor(model_proto=blob, device=0)
    text, offs = synth.ascii_corpus(n, seed=20250227)
    warm = synth.gather_packed(text, offs, np.arange(0, n, max(1, n // 1000)))
    calls = [("CalculateEntropy", lambda t, o: sp.CalculateEntropyPacked(t, o, 0.2)),
             ("SampleEncodeAndScore (num_samples %d, with replacement)" % k, lambda t, o: sp.SampleEncodeAndScorePacked(t, o, k, 0.2, seed=1)),
             ("SampleEncodeAndScore (num_samples %d, without replacement)" % k,
              lambda t, o: sp.SampleEncodeAndScorePacked(t, o, k, 0.2, wor=True, seed=1))]
    for name, fn in calls:
        fn(*warm)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            res = fn(text, offs)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        results = len(res) if isinstance(res, np.ndarray) else int(res[3][-1])
        print(json.dumps({"metric": "sentences/sec %s, theta 0.2, %s, MI355X, host-buffer form" % (name, model), "value": n / best,
                          "unit": "sentences/s", "ms": best * 1e3, "sentences": n, "results": results}))


if __name__ == "__main__":
    main()
