#!/usr/bin/env python3
"""Device-resident batch Decode rate (ids -> text), SURVEY.md section 8f row 2.

    python scripts/decode_rate.py [sentences] [model] [--spans] [--repeats R]

Encodes a synthetic corpus on the GPU, then times K decode calls over the resident CSR ids (count pass, scan, write
pass and the two host read-backs included).  Algorithmic bytes per sentence: 4 T' ids + 8 (id offset) read,
L' text bytes + 8 (text offset) written.

--spans: also times DecodeSpansDevice (the SentencePieceText form: per piece its id and the byte range of its surface) over
the same resident ids; its algorithmic bytes add 4 + 8 written per piece and 8 (piece offset) per sentence.
--repeats R: R timed windows of the plain call (each of K steps with a synchronise inside), all listed -- for comparing two
builds of the library run alternately (SPMX_LIB selects the library)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, steps):
    """Seconds per call: warm-up, then `steps` calls and a synchronise inside the window."""
    import torch
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    import torch
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    spans = "--spans" in sys.argv
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 1
    if "--repeats" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--repeats") + 1])
    n = int(args[0]) if len(args) > 0 else 10_000_000
    model = args[1] if len(args) > 1 else "uni32k"
    with open(os.path.join(ROOT, "tests", "golden", model + ".model"), "rb") as f:
        sp = SentencePieceProcessor(model_proto=f.read(), device=0)
    text, offs = synth.ascii_corpus(n, seed=20250227)
    dev = torch.device("cuda", 0)
    d_ids, d_io, total = sp.EncodeDevice(torch.from_numpy(text).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
    d_ids = d_ids[:total].clone()
    d_text, d_to, nbytes = sp.DecodeDevice(d_ids, d_io)
    steps = 30          # 13 ms a call at 10 M sentences: a window of some 400 ms
    windows = [timed(lambda: sp.DecodeDevice(d_ids, d_io, d_text, d_to), steps) for _ in range(repeats)]
    dt = float(np.median(windows))
    alg = 4 * total + 8 * n + nbytes + 8 * n
    res = {"metric": "sentences/sec DecodeBatch, %s, MI355X" % model, "value": n / dt, "unit": "sentences/s",
           "ms_per_step": dt * 1e3, "gb_text_per_s": nbytes / dt / 1e9,
           "roofline": {"bound": "hbm", "achieved": alg / dt / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": alg / dt / 8e12, "algorithmic_bytes_per_call": alg},
           "config": {"workload": "%d sentences, %d ids, %d text bytes, device-resident" % (n, total, nbytes)}}
    if repeats > 1:
        res["ms_per_step_windows"] = [w * 1e3 for w in windows]
    if spans:
        r = sp.DecodeSpansDevice(d_ids, d_io)
        assert r["total_bytes"] == nbytes and r["total_pieces"] == total
        ds = timed(lambda: sp.DecodeSpansDevice(d_ids, d_io, out=r), steps)
        alg_s = alg + 12 * total + 8 * n
        res["spans"] = {"value": n / ds, "unit": "sentences/s", "ms_per_step": ds * 1e3, "slowdown_vs_plain": ds / dt,
                        "roofline": {"bound": "hbm", "achieved": alg_s / ds / 1e9, "peak": 8000.0, "unit": "GB/s",
                                     "frac": alg_s / ds / 8e12, "algorithmic_bytes_per_call": alg_s}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
