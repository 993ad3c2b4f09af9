#!/usr/bin/env python3
"""One-GPU measurements of the packed gather (include/spmx.h: spmx_pack_ids / spmx_unpack_ids /
spmx_all_gather_ids_packed).  Nothing here runs on two GPUs: world 8 is SIMULATED on one device, and the 8-GPU figures
this prints are a MODEL.

    python scripts/gather_packed_rate.py rate  [--sentences 10000000] [--world 8] [--rounds 12] [--out FILE.json]
        The headline's shape: the 32k unigram model's ids of `sentences` sentences of the synthetic bench corpus, from the
        product's own encode, as ONE rank's shard; the world's other ranks carry the same shard (the kernels do not care
        whose ids they move).  Timed with device events, one call per measurement, the variants alternated round by
        round:  pack (one rank's block), unpack (world blocks -> the job's CSR), a hipMemcpyAsync device to device of the
        same byte count as each (read + written) as the yardstick, and the torch-op chain the two kernels replace
        (sharding.IdGatherer._call_exact's narrowing copy and counts conversion; result()'s widening, cumsum and cat;
        encode_sharded's concatenation into one CSR).  Prints and writes one JSON document.
    python scripts/gather_packed_rate.py steady [--sentences 1000000] [--calls 24]
        For a HIP API trace: world 1 over the real librccl, `calls` steady-state calls of spmx_all_gather_ids_packed and
        then of spmx_all_gather_ids, each loop between two hipRuntimeGetVersion calls (markers nothing else makes).
    python scripts/gather_packed_rate.py summarize HIP_API_TRACE.csv
        Counts the HIP API calls between the markers of a `steady` run's trace.
"""
import argparse
import ctypes as C
import csv
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS = 6300.0     # what a streaming kernel reaches on an MI355X (of 8 TB/s nominal)
XGMI_LINK_GBS = 76.5            # one direction of one xGMI link
ENCODE_MS = 4.47                # the project's one-GPU encode of the headline batch (BENCH round 6)


def link_model(world, payload_bytes, encode_ms, device_ms):
    """The formula of the benchmark's gather bound, restated: every rank's payload crosses one link per peer per step at
    the link's one-direction peak, overlapped with the next batch's device work (the encode plus the gather's own
    kernels); the step is the longer of the two."""
    link_ms = payload_bytes / (XGMI_LINK_GBS * 1e9) * 1e3
    step_ms = max(encode_ms + device_ms, link_ms)
    return {"world": world, "payload_bytes_per_rank": int(payload_bytes), "link_ms": link_ms, "device_ms_per_step": encode_ms + device_ms,
            "step_ms": step_ms, "scaling_vs_one_gpu": world * encode_ms / step_ms, "what": "MODEL, not a measurement"}


def encode_corpus(sentences):
    import torch
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    with open(os.path.join(ROOT, "tests", "golden", "uni32k.model"), "rb") as f:
        sp = SentencePieceProcessor(model_proto=f.read())
    text, offs = synth.ascii_corpus(sentences, seed=20250227)
    dev = torch.device("cuda", 0)
    d_ids, d_io, total = sp.EncodeDevice(torch.from_numpy(text).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
    return sp, d_ids[:total].clone(), d_io, int(total)


def rate(args):
    import torch
    from sentencepiece_amd import sharding
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    sp, ids, io, total = encode_corpus(args.sentences)
    dev, n, world = ids.device, args.sentences, args.world
    piece_size = sp.GetPieceSize()
    longest = int((io[1:] - io[:-1]).max())
    idw, cw = (2 if piece_size <= 65536 else 4), (1 if longest <= 255 else (2 if longest <= 65535 else 4))
    bb = sharding.packed_block_bytes(piece_size, n, total, longest)
    blocks = torch.empty(bb * world, dtype=torch.uint8, device=dev)
    all_ids = torch.empty(total * world, dtype=torch.int32, device=dev)
    all_offs = torch.empty(n * world + 1, dtype=torch.int64, device=dev)
    rs = torch.zeros(world + 1, dtype=torch.int64, device=dev)
    ri = torch.zeros(world + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    for r in range(world):
        sharding.pack_ids(ids, io, piece_size, n, total, longest, out=blocks[bb * r:bb * (r + 1)])
    sharding.packed_status(sharding.unpack_ids(blocks, world, piece_size, n, total, longest, all_ids, all_offs, rs, ri, status))
    # the result once against the torch chain's (the timing below compares like with like)
    assert torch.equal(all_ids[total:2 * total], ids) and torch.equal(all_offs[n:2 * n], io[:-1] + total)
    tiles = (n + 255) // 256
    pack_read, pack_written = 4 * total + 8 * (n + 1), idw * total + cw * n + 8 * tiles + 128
    unpack_read, unpack_written = world * pack_written, world * (4 * total + 8 * n) + 8
    copy_a = torch.empty(max(pack_read + pack_written, unpack_read + unpack_written) // 2, dtype=torch.uint8, device=dev)
    copy_b = torch.empty_like(copy_a)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def memcpy(nbytes):
        assert hip.hipMemcpyAsync(copy_b.data_ptr(), copy_a.data_ptr(), nbytes, 3, stream) == 0

    wire = torch.int16 if idw == 2 else torch.int32
    sent = {}

    def torch_send():                      # IdGatherer._call_exact: staged narrowing copy, counts in their wire width
        xs = torch.empty(total, dtype=wire, device=dev)
        xs.copy_(ids)
        c64 = io[1:] - io[:-1]
        sent["ids"], sent["counts"] = xs, (c64.to(torch.uint8) if cw == 1 else c64.to(torch.int32))

    def torch_receive():                   # IdGatherer.result() per rank, then encode_sharded's concatenation
        parts, offs = [], []
        for _ in range(world):
            parts.append(sent["ids"].to(torch.int32))
            c = sent["counts"].to(torch.int64)
            offs.append(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(c, 0)]))
        full_ids = torch.cat(parts)
        bases = np.concatenate([[0], np.cumsum([p.numel() for p in parts])])
        full_off = torch.cat([offs[r][:-1] + int(bases[r]) for r in range(world)] + [torch.tensor([int(bases[-1])], dtype=torch.int64, device=dev)])
        return full_ids, full_off

    torch_send()
    t_ids, t_off = torch_receive()
    assert torch.equal(t_ids, all_ids) and torch.equal(t_off, all_offs)
    del t_ids, t_off
    variants = {
        "pack": lambda: sharding.pack_ids(ids, io, piece_size, n, total, longest, out=blocks[:bb]),
        "memcpy_as_pack": lambda: memcpy((pack_read + pack_written) // 2),
        "unpack": lambda: sharding.unpack_ids(blocks, world, piece_size, n, total, longest, all_ids, all_offs, rs, ri, status),
        "memcpy_as_unpack": lambda: memcpy((unpack_read + unpack_written) // 2),
        "torch_send": torch_send,
        "torch_receive": torch_receive,
    }
    times = {k: [] for k in variants}
    for rnd in range(args.warmup + args.rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rnd >= args.warmup:
                times[name].append(a.elapsed_time(b))
    moved = {"pack": pack_read + pack_written, "memcpy_as_pack": pack_read + pack_written, "unpack": unpack_read + unpack_written,
             "memcpy_as_unpack": unpack_read + unpack_written}
    res = {}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_pct": 100.0 * (max(t) - min(t)) / med, "calls": len(t)}
        if name in moved:
            res[name].update(bytes_read_plus_written=moved[name], gb_per_s=moved[name] / med / 1e6,
                             share_of_achievable_hbm=moved[name] / med / 1e6 / HBM_ACHIEVABLE_GBS)
    fused = res["pack"]["median_ms"] + res["unpack"]["median_ms"]
    chain = res["torch_send"]["median_ms"] + res["torch_receive"]["median_ms"]
    worst_spread = max(res[k]["spread_pct"] for k in ("pack", "unpack", "torch_send", "torch_receive"))
    wide_payload = 4 * total + 8 * n
    out = {
        "what": "one MI355X; world %d SIMULATED on one device (every rank carries the same shard); nothing here ran on two GPUs" % world,
        "sentences_per_rank": n, "ids_per_rank": total, "ids_per_sentence": total / n, "piece_size": piece_size, "longest_sentence_ids": longest,
        "id_width": idw, "count_width": cw, "block_bytes": bb, "wide_payload_bytes": wide_payload, "block_over_wide": bb / wide_payload,
        "timing": "device events around single calls, variants alternated round by round, %d rounds after %d warm-up" % (args.rounds, args.warmup),
        "variants": res,
        "gate": {"pack_plus_unpack_ms": fused, "torch_chain_ms": chain, "holds": fused <= chain, "speedup": chain / fused,
                 "largest_spread_pct_of_the_four": worst_spread},
        "link_model": {"encode_ms": ENCODE_MS, "link_gb_per_s_one_direction": XGMI_LINK_GBS,
                       "wide": link_model(8, wide_payload, ENCODE_MS, 0.0),
                       "packed": link_model(8, bb, ENCODE_MS, res["pack"]["median_ms"] + res["unpack"]["median_ms"]),
                       "packed_transfer_only": link_model(8, bb, ENCODE_MS, 0.0)},
    }
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if out["gate"]["holds"] else 1


def steady(args):
    import torch
    from sentencepiece_amd import _capi, sharding
    lib = _capi.lib()
    hip = C.CDLL("libamdhip64.so")
    sp, ids, io, total = encode_corpus(args.sentences)
    dev, n = ids.device, args.sentences
    longest = int((io[1:] - io[:-1]).max())
    uid = (C.c_char * 128)()
    comm = C.c_void_p()
    assert lib.spmx_rccl_unique_id(uid) == 0 and lib.spmx_rccl_comm_init(C.byref(comm), 1, 0, uid) == 0, lib.spmx_gather_last_error()
    g = sharding.PackedGatherer(comm, 0, 1, sp.GetPieceSize(), n, total, longest)
    all_ids = torch.empty(total, dtype=torch.int32, device=dev)
    all_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rs = torch.zeros(2, dtype=torch.int64, device=dev)
    ri = torch.zeros(2, dtype=torch.int64, device=dev)
    scratch = torch.zeros(int(lib.spmx_gather_scratch_words(1)), dtype=torch.int64, device=dev)
    h_rs, h_ri = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    stream = torch.cuda.current_stream(dev).cuda_stream
    version = C.c_int(0)

    def packed():
        g(ids, io, all_ids, all_offs, rs, ri)

    def wide():
        assert lib.spmx_all_gather_ids(comm, 0, 1, ids.data_ptr(), total, io.data_ptr(), n, all_ids.data_ptr(), total, all_offs.data_ptr(),
                                       n + 1, scratch.data_ptr(), h_rs.ctypes.data, h_ri.ctypes.data, stream) == 0

    for fn in (packed, wide):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        hip.hipRuntimeGetVersion(C.byref(version))        # marker: the steady-state calls begin
        for _ in range(args.calls):
            fn()
        hip.hipRuntimeGetVersion(C.byref(version))        # marker: ... and end (nothing has waited for them yet)
        torch.cuda.synchronize()
    g.status()
    assert torch.equal(all_ids, ids) and torch.equal(all_offs, io)
    g.close()
    lib.spmx_rccl_comm_destroy(comm)
    print("steady: %d calls of each form, %d sentences, %d ids" % (args.calls, n, total))
    return 0


def summarize(args):
    rows = []
    with open(args.trace, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), row["Function"]))
    rows.sort()
    marks = [i for i, (_, fn) in enumerate(rows) if fn == "hipRuntimeGetVersion"]
    assert len(marks) >= 4, "expected the four markers of a `steady` run, found %d" % len(marks)
    marks = marks[-4:]
    for label, (a, b) in (("spmx_all_gather_ids_packed", marks[:2]), ("spmx_all_gather_ids (the wide call, for contrast)", marks[2:])):
        counts = {}
        for _, fn in rows[a + 1:b]:
            counts[fn] = counts.get(fn, 0) + 1
        print("HIP API calls between the markers of the steady-state loop of %s:" % label)
        for fn in sorted(counts):
            print("  %-28s %6d" % (fn, counts[fn]))
        waits = sum(v for k, v in counts.items() if "Synchronize" in k)
        print("  -> host waits (hip*Synchronize): %d; hipMemcpy* calls (any direction): %d" %
              (waits, sum(v for k, v in counts.items() if k.startswith("hipMemcpy"))))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("rate")
    p.add_argument("--sentences", type=int, default=10_000_000)
    p.add_argument("--world", type=int, default=8)
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=None)
    p = sub.add_parser("steady")
    p.add_argument("--sentences", type=int, default=1_000_000)
    p.add_argument("--calls", type=int, default=24)
    p = sub.add_parser("summarize")
    p.add_argument("trace")
    args = ap.parse_args()
    return {"rate": rate, "steady": steady, "summarize": summarize}[args.mode](args)


if __name__ == "__main__":
    sys.exit(main())
