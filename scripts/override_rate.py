#!/usr/bin/env python3
"""What a normalizer_spec override costs next to loading the model.

    python scripts/override_rate.py [--out profiles/r08_override_ms.json] [--reps 5] [model ...]

Per model (default uni32k, bpe32k, c5_250k): `reps` times, in one process, the wall clock of
  - spmx_create of the model's bytes (parse, table compile, upload, self-test), and
  - ONE single-flag spmx_override_normalizer_spec on the handle just made (table compile and upload beside the old
    tables, swap, release of the old set): add_dummy_prefix goes off on a handle loaded with it on.
spmx_create is the yardstick: an override does the same compile and upload without the parse and the self-test, but it holds
two table sets for a moment and frees one.  One short encode follows every override and is checked to run (not timed)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sentencepiece_amd import _capi
    from sentencepiece_amd.processor import SentencePieceProcessor
    from tests import fixtures
    argv = sys.argv[1:]
    out = None
    reps = 5
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
        del argv[argv.index("--reps"):argv.index("--reps") + 2]
    models = argv or ["uni32k", "bpe32k", "c5_250k"]
    _capi.lib()
    import torch
    device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU visible to torch"
    res = {"metric": "milliseconds per call", "device": device, "reps": reps, "models": {}}
    for model in models:
        blob = fixtures.model_blob(model)
        SentencePieceProcessor(model_proto=blob).Encode("warm up: the first handle of a process pays for the runtime")
        create_ms, override_ms = [], []
        sp = SentencePieceProcessor()
        for _ in range(reps):
            sp._close()                      # (the previous handle's release is not part of a load)
            t0 = time.perf_counter()
            sp.Load(model_proto=blob)
            create_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            sp.OverrideNormalizerSpec(add_dummy_prefix=False)
            override_ms.append((time.perf_counter() - t0) * 1e3)
            assert sp.NormalizerSpec()["add_dummy_prefix"] is False and len(sp.Encode("hello world")) > 0
        info = sp.HandleInfo()
        res["models"][model] = {"create_ms": create_ms, "override_ms": override_ms,
                                "create_ms_median": float(np.median(create_ms)), "override_ms_median": float(np.median(override_ms)),
                                "override_over_create": float(np.median(override_ms) / np.median(create_ms)),
                                "table_bytes": info["table_bytes"], "model_bytes": len(blob), "pieces": sp.GetPieceSize()}
    line = json.dumps(res)
    print(line)
    if out:
        with open(os.path.join(ROOT, out) if not os.path.isabs(out) else out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
