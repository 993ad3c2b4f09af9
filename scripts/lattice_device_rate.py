#!/usr/bin/env python3
"""Host form against device form of the lattice calls: NBestEncode (5) and lattice SampleEncode on the corpus builder of
bench.py.  The host form is H2D + Normalize + lattice kernel + D2H of the sparse result arena + host CSR assembly; the
device form takes torch tensors already on the GPU and leaves the CSR there (kernels_latticecsr.h), synchronised before
the clock stops.  Nothing has been measured with it yet: no rate is stated anywhere in the documents.

    python scripts/lattice_device_rate.py [sentences] [nbest_size] [model]

One JSON line per call and form."""
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
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    model = sys.argv[3] if len(sys.argv) > 3 else "uni32k"
    with open(os.path.join(ROOT, "tests", "golden", model + ".model"), "rb") as f:
        blob = f.read()
    sp = SentencePieceProcessor(model_proto=blob, device=0)
    text, offs = synth.ascii_corpus(n, seed=20250227)
    warm = synth.gather_packed(text, offs, np.arange(0, n, max(1, n // 1000)))

    def on_device(t, o):
        padded = np.concatenate([np.ascontiguousarray(t, dtype=np.uint8), np.zeros(32, dtype=np.uint8)])
        return (torch.from_numpy(padded).cuda()[:len(t)],
                torch.from_numpy(np.ascontiguousarray(o, dtype=np.uint64).view(np.int64)).cuda())
    d_all, d_warm = on_device(text, offs), on_device(*warm)

    def timed(fn, args):
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*args)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, res
    calls = [("NBestEncode (%d)" % k, lambda t, o: sp.NBestPacked(t, o, k), lambda t, o: sp.NBestEncodeDevice(t, o, k),
              lambda r: int(r[3][-1])),
             ("SampleEncode (lattice, alpha 0.2)", lambda t, o: sp.SampleEncodePacked(t, o, -1, 0.2, 1),
              lambda t, o: sp.SampleEncodeDevice(t, o, -1, 0.2, 1), lambda r: n)]
    for name, host, dev, results in calls:
        for form, fn, args, w in (("host-buffer form", host, (text, offs), warm), ("device form", dev, d_all, d_warm)):
            fn(*w)
            best, res = timed(fn, args)
            print(json.dumps({"metric": "sentences/sec %s, %s, MI355X, %s" % (name, model, form), "value": n / best,
                              "unit": "sentences/s", "ms": best * 1e3, "sentences": n, "results": results(res)}))


if __name__ == "__main__":
    main()
