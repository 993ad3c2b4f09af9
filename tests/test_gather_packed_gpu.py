"""The packed gather (include/spmx.h: spmx_gather_plan_*, spmx_all_gather_ids_packed, spmx_pack_ids / spmx_unpack_ids)
on the GPU, through the Python wrappers of sentencepiece_amd/sharding.py: libspmx.so's pack and unpack kernels, the real
librccl at world 1, and world 8 simulated on the one device.  The CPU legs are in tests/test_gather_packed.py."""
import ctypes as C

import numpy as np
import pytest

from sentencepiece_amd import sharding
from tests import fixtures

pytestmark = pytest.mark.gpu

ID_PAT, OFF_PAT, SUM_PAT = -7, 0xCDCD, 0xABAB


def _device_csr(n, max_count, id_top, seed, dev):
    """A generated CSR on the device: counts 0 .. 26 (a fifth of the sentences empty), one sentence of max_count ids (the
    4-byte width: 70 000), an odd total, ids over the whole id width with 0 and id_top among them."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    counts = torch.randint(0, 27, (n,), generator=g, dtype=torch.int64)
    counts[torch.rand(n, generator=g) < 0.2] = 0
    counts[n // 3] = max_count
    if int(counts.sum()) % 2 == 0:
        counts[n // 3 + 1] += 1
    total = int(counts.sum())
    ids = torch.randint(0, id_top + 1, (total,), generator=g, dtype=torch.int64).to(torch.int32)
    ids[0], ids[total // 2], ids[total - 1] = id_top, id_top, 0
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    return ids.to(dev), offs.to(dev)


@pytest.mark.parametrize("id_width,count_width", [(2, 1), (2, 2), (4, 4), (4, 1)])
def test_pack_unpack_round_trip_many_workgroups(id_width, count_width):
    """Four ranks of 400 001 / 0 / 380 000 / 399 872 sentences, about 12 M ids: every workgroup of the two kernels has work,
    the outputs are moved off their 16-byte alignment, guard words surround them."""
    import torch
    dev = torch.device("cuda", 0)
    piece_size, id_top = {2: (65536, 65535), 4: (65537, 2 ** 31 - 1)}[id_width]
    max_count = {1: 255, 2: 65535, 4: 70000}[count_width]
    sizes = [400_001, 0, 380_000, 399_872]
    shards = [_device_csr(n, max_count, id_top, 11 * r + id_width + count_width, dev) if n else
              (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)) for r, n in enumerate(sizes)]
    world = len(shards)
    cap_s, cap_i = max(sizes), max(int(i.numel()) for i, _ in shards)
    bb = sharding.packed_block_bytes(piece_size, cap_s, cap_i, max_count)
    assert bb <= id_width * cap_i + count_width * cap_s + cap_s // 16 + 1024
    blocks = torch.empty(bb * world, dtype=torch.uint8, device=dev)
    assert blocks.data_ptr() % 128 == 0
    for r, (ids, offs) in enumerate(shards):
        sharding.pack_ids(ids, offs, piece_size, cap_s, cap_i, max_count, out=blocks[bb * r:bb * (r + 1)])
    want_ids = torch.cat([i for i, _ in shards])
    bases = np.concatenate([[0], np.cumsum([int(i.numel()) for i, _ in shards])])
    want_offs = torch.cat([o[:-1] + int(bases[r]) for r, (_, o) in enumerate(shards)] +
                          [torch.tensor([int(bases[-1])], dtype=torch.int64, device=dev)])
    assert int(want_ids.numel()) >= 10_000_000 and any(int(b) % 2 for b in bases[1:-1])
    n_i, n_s = int(want_ids.numel()), int(want_offs.numel())
    ids_buf = torch.full((n_i + 40,), ID_PAT, dtype=torch.int32, device=dev)
    offs_buf = torch.full((n_s + 40,), OFF_PAT, dtype=torch.int64, device=dev)
    rs = torch.full((world + 1,), SUM_PAT, dtype=torch.int64, device=dev)
    ri = torch.full((world + 1,), SUM_PAT, dtype=torch.int64, device=dev)
    all_ids, all_offs = ids_buf[17:17 + n_i], offs_buf[9:9 + n_s]        # (4 and 8 bytes past a 16-byte boundary)
    st = sharding.unpack_ids(blocks, world, piece_size, cap_s, cap_i, max_count, all_ids, all_offs, rs, ri)
    sharding.packed_status(st)
    assert torch.equal(all_offs, want_offs) and torch.equal(all_ids, want_ids)
    assert bool((ids_buf[:17] == ID_PAT).all()) and bool((ids_buf[17 + n_i:] == ID_PAT).all())
    assert bool((offs_buf[:9] == OFF_PAT).all()) and bool((offs_buf[9 + n_s:] == OFF_PAT).all())
    assert rs.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and ri.tolist() == bases.tolist()


def test_all_gather_ids_packed_on_the_gpu_world_1(oracle, corpora):
    """libspmx.so + the real librccl on the one GPU of the box: communicator through the spmx_rccl_* helpers, the plan's
    agreement over it, pack -> unpack; the product encode feeds it.  Twice on one plan."""
    import torch
    from sentencepiece_amd import _capi
    from sentencepiece_amd.processor import SentencePieceProcessor
    lib = _capi.lib()
    blob = fixtures.model_blob("uni32k")
    text, offs = fixtures.head(*corpora["synth20k"], 5000)
    sp = SentencePieceProcessor(model_proto=blob)
    dev = torch.device("cuda", 0)
    d_ids, d_io, total = sp.EncodeDevice(torch.from_numpy(text).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
    n = len(offs) - 1
    longest = int((d_io[1:] - d_io[:-1]).max())
    uid = (C.c_char * 128)()
    assert lib.spmx_rccl_unique_id(uid) == 0, lib.spmx_gather_last_error()
    comm = C.c_void_p()
    assert lib.spmx_rccl_comm_init(C.byref(comm), 1, 0, uid) == 0, lib.spmx_gather_last_error()
    g = sharding.PackedGatherer(comm, 0, 1, sp.GetPieceSize(), n, total, longest)
    assert g.block_bytes == sharding.packed_block_bytes(sp.GetPieceSize(), n, total, longest) < 4 * total + 8 * n
    oids, oio = oracle.load(blob).encode_batch(text, offs)
    for _ in range(2):
        all_ids = torch.full((total + 8,), ID_PAT, dtype=torch.int32, device=dev)
        all_offs = torch.full((n + 3,), OFF_PAT, dtype=torch.int64, device=dev)
        rs = torch.full((2,), SUM_PAT, dtype=torch.int64, device=dev)
        ri = torch.full((2,), SUM_PAT, dtype=torch.int64, device=dev)
        g(d_ids, d_io, all_ids, all_offs, rs, ri)
        g.status()
        np.testing.assert_array_equal(all_offs[:n + 1].cpu().numpy().astype(np.uint64), np.asarray(oio))
        np.testing.assert_array_equal(all_ids[:total].cpu().numpy(), np.asarray(oids))
        assert bool((all_ids[total:] == ID_PAT).all()) and bool((all_offs[n + 1:] == OFF_PAT).all())     # guard words untouched
        assert rs.tolist() == [0, n] and ri.tolist() == [0, total]
    g.close()
    assert lib.spmx_rccl_comm_destroy(comm) == 0


def test_world_8_on_one_device_equals_the_single_encode():
    """8 byte-balanced shards of a generated corpus of 1.2 M sentences, each encoded on its own, packed, and all unpacked
    together: the CSR is bit-equal to the single encode of the whole corpus."""
    import torch
    from sentencepiece_amd import synth
    from sentencepiece_amd.processor import SentencePieceProcessor
    world, n = 8, 1_200_000
    text, offs = synth.ascii_corpus(n, seed=20261016)
    sp = SentencePieceProcessor(model_proto=fixtures.model_blob("uni32k"))
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(text).to(dev)
    w_ids, w_io, w_total = sp.EncodeDevice(d_text, torch.from_numpy(offs.view(np.int64)).to(dev))
    w_ids, w_io = w_ids[:w_total].clone(), w_io.clone()
    b = sharding.shard_bounds(offs, world)
    shards = []
    for r in range(world):
        lo, hi = int(b[r]), int(b[r + 1])
        o = torch.from_numpy((offs[lo:hi + 1] - offs[lo]).astype(np.int64)).to(dev)
        ids, io, total = sp.EncodeDevice(d_text[int(offs[lo]):int(offs[hi])].clone(), o)
        shards.append((ids[:total].clone(), io.clone()))
    cap_s = max(int(io.numel()) - 1 for _, io in shards)
    cap_i = max(int(i.numel()) for i, _ in shards)
    longest = max(int((io[1:] - io[:-1]).max()) for _, io in shards)
    piece_size = sp.GetPieceSize()
    bb = sharding.packed_block_bytes(piece_size, cap_s, cap_i, longest)
    assert piece_size <= 65536 and longest <= 255 and bb < (4 * cap_i + 8 * cap_s) // 2
    blocks = torch.empty(bb * world, dtype=torch.uint8, device=dev)
    for r, (ids, io) in enumerate(shards):
        sharding.pack_ids(ids, io, piece_size, cap_s, cap_i, longest, out=blocks[bb * r:bb * (r + 1)])
    all_ids = torch.full((w_total + 16,), ID_PAT, dtype=torch.int32, device=dev)
    all_offs = torch.full((n + 9,), OFF_PAT, dtype=torch.int64, device=dev)
    rs = torch.zeros(world + 1, dtype=torch.int64, device=dev)
    ri = torch.zeros(world + 1, dtype=torch.int64, device=dev)
    sharding.packed_status(sharding.unpack_ids(blocks, world, piece_size, cap_s, cap_i, longest, all_ids[:w_total], all_offs[:n + 1], rs, ri))
    assert torch.equal(all_offs[:n + 1], w_io) and torch.equal(all_ids[:w_total], w_ids)
    assert bool((all_ids[w_total:] == ID_PAT).all()) and bool((all_offs[n + 1:] == OFF_PAT).all())
    assert rs.tolist() == [int(v) for v in b] and ri.tolist() == [int(w_io[int(v)]) for v in b]


@pytest.mark.parametrize("case", ["sentences over the agreed capacity", "ids over the agreed capacity", "a count of 256 under width 1",
                                  "an id of 65536 under width 2", "an output buffer one id short"])
def test_violations_on_the_gpu(case):
    """What needs no second rank: three blocks on the device, the middle one breaks the agreement; the unpack reports it,
    writes nothing, and the same buffers then carry a valid job."""
    import torch
    from sentencepiece_amd import _capi
    from tests.test_gather_packed import _violation_cases, expected
    lib = _capi.lib()
    dev = torch.device("cuda", 0)
    cases = _violation_cases()
    piece_size, max_count, maker, (cap_s, cap_i), code = cases.get(case, (65536, 255, cases["valid"][2], (8, 1000), 8))
    world = 3
    bb = sharding.packed_block_bytes(piece_size, cap_s, cap_i, max_count)
    blocks = torch.empty(bb * world, dtype=torch.uint8, device=dev)
    for shard_of in (maker, cases["valid"][2]):
        host = [shard_of(r) for r in range(world)]
        want = expected(host)
        for r, (ids, o) in enumerate(host):
            sharding.pack_ids(torch.from_numpy(ids).to(dev), torch.from_numpy(o.view(np.int64)).to(dev), piece_size, cap_s, cap_i, max_count,
                              out=blocks[bb * r:bb * (r + 1)])
        short = 1 if case not in cases and shard_of is maker else 0
        all_ids = torch.full((len(want[0]) - short if case not in cases else 2000,), ID_PAT, dtype=torch.int32, device=dev)
        all_offs = torch.full((64,), OFF_PAT, dtype=torch.int64, device=dev)
        rs = torch.full((world + 1,), SUM_PAT, dtype=torch.int64, device=dev)
        st = sharding.unpack_ids(blocks, world, piece_size, cap_s, cap_i, max_count, all_ids, all_offs, rs, None)
        if shard_of is maker:
            words = st.cpu().tolist()
            assert words[0] == code and words[1] == (1 if case in cases else 0xFFFFFFFF), words
            with pytest.raises(RuntimeError, match="status %d" % code):
                sharding.packed_status(st)
            assert (b"rank 1" if case in cases else b"this caller") in lib.spmx_gather_last_error()
            assert bool((all_ids == ID_PAT).all()) and bool((all_offs == OFF_PAT).all()) and bool((rs == SUM_PAT).all())
        else:
            sharding.packed_status(st)
            np.testing.assert_array_equal(all_ids[:len(want[0])].cpu().numpy(), want[0])
            np.testing.assert_array_equal(all_offs[:len(want[1])].cpu().numpy().astype(np.uint64), want[1])
            assert rs.tolist() == want[2].tolist()
