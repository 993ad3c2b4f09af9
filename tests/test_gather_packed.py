"""The packed gather of the C ABI (include/spmx.h: spmx_gather_plan_*, spmx_all_gather_ids_packed, spmx_pack_ids /
spmx_unpack_ids; csrc/gather.cc, csrc/kernels_gather.h pack_block / unpack_block) on the CPU: the device bodies run under
the emulator (tests/emulib.py), ranks are threads of this process over tests/emu/libfake_rccl.so, "device" memory is host
memory.  The -m gpu twins are in tests/test_gather_packed_gpu.py."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from sentencepiece_amd import sharding
from tests import fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256
U64_MAX = 2 ** 64 - 1
ID_PAT, OFF_PAT, SUM_PAT = -7, 0xCDCD, 0xABAB


@pytest.fixture(scope="module")
def emu_lib():
    os.environ["SPMX_RCCL_LIB"] = os.path.join(ROOT, "tests", "emu", "libfake_rccl.so")    # (read at the first gather call)
    from tests import emulib
    return emulib.EmuLib()


def aligned(nbytes, fill=0xA5, align=128):
    """uint8 view of nbytes whose address is a multiple of `align`."""
    raw = np.full(nbytes + align, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def make_csr(n, max_count, id_top, seed, offset_base=0):
    """A generated CSR of n sentences: empty sentences, a sentence of exactly max_count ids (kept small for the 4-byte
    width's 70 000), ids at 0 and at id_top.  -> (ids int32 [offset_base + total], offsets uint64 [n + 1] starting at
    offset_base)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 9, size=n).astype(np.int64)
    counts[rng.random(n) < 0.2] = 0
    if n > 2:
        counts[0] = 0
        counts[n - 1] = 0
    if n:
        top = int(rng.integers(1, n - 1)) if n > 2 else 0
        counts[top] = max_count
        if n > 3 and int(counts.sum()) % 2 == 0:          # an odd number of ids: the next rank's ids start at an odd element
            counts[1 if top != 1 else 2] += 1
    total = int(counts.sum())
    ids = rng.integers(0, id_top + 1, size=total, dtype=np.int64)
    if total:
        ids[0] = id_top
        ids[total - 1] = 0
        ids[total // 2] = id_top
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64) + np.uint64(offset_base)
    full = np.concatenate([np.full(offset_base, 12345, dtype=np.int64), ids]).astype(np.int32)
    return full, offs


def expected(shards):
    """The job's CSR of per-rank (ids, offsets) shards -> (all_ids, all_offsets, rank_sentences, rank_ids)."""
    parts, offs, rs, ri = [], [], [0], [0]
    for ids, o in shards:
        lo, hi = int(o[0]), int(o[-1])
        offs.append(o[:-1].astype(np.int64) - lo + ri[-1])
        parts.append(ids[lo:hi])
        rs.append(rs[-1] + len(o) - 1)
        ri.append(ri[-1] + hi - lo)
    all_ids = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    all_offs = np.concatenate(offs + [np.array([ri[-1]], dtype=np.int64)])
    return all_ids.astype(np.int32), all_offs.astype(np.uint64), np.array(rs, np.uint64), np.array(ri, np.uint64)


# what the agreed numbers select: (piece_size, top id) per id width, (max ids per sentence) per count width
ID_WIDTHS = {2: (65536, 65535), 4: (65537, 2 ** 31 - 1)}
COUNT_WIDTHS = {1: 255, 2: 65535, 4: 70000}
# sentences per rank: n = 0, one below / at / one above a tile boundary, several tiles; empty ranks among the others
WORLDS = {1: [TILE + 1], 2: [TILE - 1, TILE], 5: [0, TILE + 1, 0, 3, 2 * TILE + 5], 64: [(7 * r) % 23 if r % 5 else 0 for r in range(64)]}


def roundtrip_host(lib, shards, piece_size, max_count, slack=(0, 0), skew=(1, 1)):
    """pack every shard, unpack all, in host memory.  skew: elements by which the output arrays are moved off their 16-byte
    alignment.  -> (status words, all_ids with guards, all_offs with guards, rank_sentences, rank_ids, expectation)."""
    world = len(shards)
    cap_s = max(len(o) - 1 for _, o in shards)
    cap_i = max(int(o[-1]) - int(o[0]) for _, o in shards)
    bb = int(lib.spmx_packed_block_bytes(piece_size, cap_s, cap_i, max_count))
    blocks = aligned(bb * world)
    for r, (ids, o) in enumerate(shards):
        rc = lib.spmx_pack_ids(ids.ctypes.data, o.ctypes.data, len(o) - 1, piece_size, cap_s, cap_i, max_count, U64_MAX, U64_MAX,
                               blocks[bb * r:].ctypes.data, None)
        assert rc == 0, lib.spmx_gather_last_error()
    want = expected(shards)
    n_i, n_s = len(want[0]) + slack[0], len(want[1]) + slack[1]
    ids_buf = aligned(4 * (n_i + 24)).view(np.int32)
    ids_buf[:] = ID_PAT
    offs_buf = aligned(8 * (n_s + 24)).view(np.uint64)
    offs_buf[:] = OFF_PAT
    rs = np.full(world + 3, SUM_PAT, dtype=np.uint64)
    ri = np.full(world + 3, SUM_PAT, dtype=np.uint64)
    st = np.full(4, 77, dtype=np.uint64)
    all_ids, all_offs = ids_buf[skew[0]:], offs_buf[skew[1]:]
    rc = lib.spmx_unpack_ids(blocks.ctypes.data, world, piece_size, cap_s, cap_i, max_count, all_ids.ctypes.data, n_i,
                             all_offs.ctypes.data, n_s, rs.ctypes.data, ri.ctypes.data, st.ctypes.data, None)
    assert rc == 0, lib.spmx_gather_last_error()
    return st, ids_buf, offs_buf, rs, ri, want, bb


@pytest.mark.parametrize("world", sorted(WORLDS))
@pytest.mark.parametrize("count_width", sorted(COUNT_WIDTHS))
@pytest.mark.parametrize("id_width", sorted(ID_WIDTHS))
def test_pack_unpack_round_trip(emu_lib, id_width, count_width, world):
    lib = emu_lib.lib
    piece_size, id_top = ID_WIDTHS[id_width]
    max_count = COUNT_WIDTHS[count_width]
    # (rank 1's CSR does not start at offset 0: the ids of a shard are d_ids[offsets[0] .. offsets[n]))
    shards = [make_csr(n, max_count, id_top, 100 * world + r, offset_base=3 if r == 1 else 0) for r, n in enumerate(WORLDS[world])]
    skew = (1, 1)
    st, ids_buf, offs_buf, rs, ri, want, bb = roundtrip_host(lib, shards, piece_size, max_count, skew=skew)
    assert st.tolist()[:3] == [0, 0, 0], (st.tolist(), lib.spmx_packed_status(st.ctypes.data), lib.spmx_gather_last_error())
    w_ids, w_offs, w_rs, w_ri = want
    assert world == 1 or any(int(v) % 2 for v in w_ri[1:world])     # an odd id base: source and destination aligned differently
    np.testing.assert_array_equal(offs_buf[skew[1]:skew[1] + len(w_offs)], w_offs)
    np.testing.assert_array_equal(ids_buf[skew[0]:skew[0] + len(w_ids)], w_ids)
    np.testing.assert_array_equal(rs[:world + 1], w_rs)
    np.testing.assert_array_equal(ri[:world + 1], w_ri)
    # nothing outside the CSR and the prefix sums is written
    assert (ids_buf[:skew[0]] == ID_PAT).all() and (ids_buf[skew[0] + len(w_ids):] == ID_PAT).all()
    assert (offs_buf[:skew[1]] == OFF_PAT).all() and (offs_buf[skew[1] + len(w_offs):] == OFF_PAT).all()
    assert (rs[world + 1:] == SUM_PAT).all() and (ri[world + 1:] == SUM_PAT).all()
    # the block has the width the agreed numbers ask for
    cap_s = max(len(o) - 1 for _, o in shards)
    cap_i = max(int(o[-1]) - int(o[0]) for _, o in shards)
    assert id_width * cap_i + count_width * cap_s <= bb <= id_width * cap_i + count_width * cap_s + cap_s // 16 + 1024


def test_pack_unpack_aligned_outputs_and_no_sentences(emu_lib):
    """Outputs ON their 16-byte alignment (the paired offset stores), and a job without any sentence."""
    lib = emu_lib.lib
    shards = [make_csr(n, 40, 65535, 7 + r) for r, n in enumerate([TILE + 3, 2 * TILE])]
    st, ids_buf, offs_buf, rs, ri, want, _ = roundtrip_host(lib, shards, 65536, 255, skew=(0, 0))
    assert st.tolist()[:3] == [0, 0, 0]
    np.testing.assert_array_equal(offs_buf[:len(want[1])], want[1])
    np.testing.assert_array_equal(ids_buf[:len(want[0])], want[0])
    assert (ids_buf[len(want[0]):] == ID_PAT).all() and (offs_buf[len(want[1]):] == OFF_PAT).all()
    empty = [(np.zeros(0, np.int32), np.zeros(1, np.uint64)) for _ in range(3)]
    st, ids_buf, offs_buf, rs, ri, want, _ = roundtrip_host(lib, empty, 65536, 255)
    assert st.tolist()[:3] == [0, 0, 0] and offs_buf[1] == 0 and (offs_buf[2:] == OFF_PAT).all() and (ids_buf == ID_PAT).all()
    assert rs[:4].tolist() == [0, 0, 0, 0] and ri[:4].tolist() == [0, 0, 0, 0]


def _violation_cases():
    """name -> (piece_size, agreed max_count, shards maker, capacities override or None, status code, slack of the outputs)"""
    ok = lambda r: make_csr(5 + r, 9, 65535, 40 + r)

    def too_many_sentences(r):
        return make_csr(9, 9, 65535, 50) if r == 1 else make_csr(3, 9, 65535, 51 + r)

    def too_many_ids(r):
        return make_csr(4, 200, 65535, 60) if r == 1 else make_csr(4, 9, 65535, 61 + r)

    def wide_count(r):
        return make_csr(6, 256 if r == 1 else 255, 65535, 70 + r)

    def wide_id(r):
        ids, o = make_csr(6, 9, 65535, 80 + r)
        if r == 1:
            ids = ids.copy()
            ids[len(ids) // 3] = 65536
        return ids, o

    return {
        "sentences over the agreed capacity": (65536, 255, too_many_sentences, (8, 1000), 8),
        "ids over the agreed capacity": (65536, 255, too_many_ids, (8, 100), 8),
        "a count of 256 under width 1": (65536, 255, wide_count, (8, 1000), 11),
        "an id of 65536 under width 2": (65536, 255, wide_id, (8, 1000), 11),
        "valid": (65536, 255, ok, (8, 1000), 0),
    }


@pytest.mark.parametrize("case", [k for k in _violation_cases() if k != "valid"])
def test_pack_unpack_reports_violations(emu_lib, case):
    """No second rank needed: three blocks packed and unpacked in one thread; rank 1's shard breaks the agreement."""
    lib = emu_lib.lib
    piece_size, max_count, maker, (cap_s, cap_i), code = _violation_cases()[case]
    world = 3
    bb = int(lib.spmx_packed_block_bytes(piece_size, cap_s, cap_i, max_count))
    blocks = aligned(bb * world)
    for shard_of in (maker, _violation_cases()["valid"][2]):            # the violation, then a valid job through the same buffers
        shards = [shard_of(r) for r in range(world)]
        for r, (ids, o) in enumerate(shards):
            assert lib.spmx_pack_ids(ids.ctypes.data, o.ctypes.data, len(o) - 1, piece_size, cap_s, cap_i, max_count, U64_MAX, U64_MAX,
                                     blocks[bb * r:].ctypes.data, None) == 0
        all_ids = np.full(2000, ID_PAT, dtype=np.int32)
        all_offs = np.full(64, OFF_PAT, dtype=np.uint64)
        rs = np.full(world + 1, SUM_PAT, dtype=np.uint64)
        ri = np.full(world + 1, SUM_PAT, dtype=np.uint64)
        st = np.zeros(4, dtype=np.uint64)
        assert lib.spmx_unpack_ids(blocks.ctypes.data, world, piece_size, cap_s, cap_i, max_count, all_ids.ctypes.data, len(all_ids),
                                   all_offs.ctypes.data, len(all_offs), rs.ctypes.data, ri.ctypes.data, st.ctypes.data, None) == 0
        if shard_of is maker:
            assert int(st[0]) == code and int(st[1]) == 1, st.tolist()
            assert lib.spmx_packed_status(st.ctypes.data) == code and b"rank 1" in lib.spmx_gather_last_error()
            assert (all_ids == ID_PAT).all() and (all_offs == OFF_PAT).all() and (rs == SUM_PAT).all() and (ri == SUM_PAT).all()
        else:
            want = expected(shards)
            assert int(st[0]) == 0 and lib.spmx_packed_status(st.ctypes.data) == 0
            np.testing.assert_array_equal(all_ids[:len(want[0])], want[0])
            np.testing.assert_array_equal(all_offs[:len(want[1])], want[1])


def test_unpack_output_one_id_short_and_foreign_blocks(emu_lib):
    lib = emu_lib.lib
    shards = [make_csr(5 + r, 9, 65535, 90 + r) for r in range(2)]
    st, ids_buf, offs_buf, rs, ri, want, bb = roundtrip_host(lib, shards, 65536, 255, slack=(-1, 0))
    assert st.tolist()[:3] == [8, 0xFFFFFFFF, 32] and int(st[3]) == len(want[0])       # the caller's own buffer: no rank to name
    assert (ids_buf == ID_PAT).all() and (offs_buf == OFF_PAT).all() and (rs == SUM_PAT).all()
    st, ids_buf, offs_buf, rs, ri, want, bb = roundtrip_host(lib, shards, 65536, 255, slack=(0, -1))
    assert st.tolist()[:3] == [8, 0xFFFFFFFF, 32] and (ids_buf == ID_PAT).all() and (offs_buf == OFF_PAT).all()
    # bytes that are no block of these capacities are refused, not interpreted
    junk = aligned(2 * bb, fill=0x5A)
    out_i, out_o, st = np.full(64, ID_PAT, np.int32), np.full(64, OFF_PAT, np.uint64), np.zeros(4, np.uint64)
    assert lib.spmx_unpack_ids(junk.ctypes.data, 2, 65536, 6, 100, 255, out_i.ctypes.data, 64, out_o.ctypes.data, 64, None, None,
                               st.ctypes.data, None) == 0
    assert st.tolist()[:3] == [13, 0, 64] and (out_i == ID_PAT).all() and (out_o == OFF_PAT).all()
    assert lib.spmx_unpack_ids(junk.ctypes.data, 65, 65536, 6, 100, 255, None, 0, None, 0, None, None, st.ctypes.data, None) == 3
    assert lib.spmx_pack_ids(None, None, 0, 65536, 6, 100, 255, 0, 0, junk[1:].ctypes.data, None) == 3      # not 128-byte aligned


def test_block_size_is_within_the_cap_and_below_half_of_the_wide_form(emu_lib):
    lib = emu_lib.lib
    for piece_size, idw in ((32000, 2), (65536, 2), (65537, 4), (250000, 4)):
        for max_count, cw in ((1, 1), (255, 1), (256, 2), (65535, 2), (65536, 4)):
            for s, i in ((0, 0), (1, 1), (255, 3), (256, 7000), (257, 1), (12345, 345678), (10_000_000, 280_800_000)):
                bb = int(lib.spmx_packed_block_bytes(piece_size, s, i, max_count))
                assert bb % 128 == 0 and idw * i + cw * s <= bb <= idw * i + cw * s + s // 16 + 1024, (piece_size, max_count, s, i, bb)
    # the headline shape: 10 M sentences of 28.08 ids, a 32k vocabulary, at most 255 ids per sentence
    s, i = 10_000_000, 280_800_000
    assert int(lib.spmx_packed_block_bytes(32000, s, i, 255)) * 2 < 4 * i + 8 * s


class _Rank:
    """One rank of a threaded job: communicator, plan, and gathers into pattern-filled host arrays."""

    def __init__(self, lib, uid, world, rank):
        self.lib, self.world, self.rank = lib, world, rank
        self.comm = C.c_void_p()
        assert lib.spmx_rccl_comm_init(C.byref(self.comm), world, rank, uid) == 0, lib.spmx_gather_last_error()
        self.plan = C.c_void_p()

    def create(self, piece_size, max_s, max_i, max_count):
        rc = self.lib.spmx_gather_plan_create(self.comm, self.rank, self.world, piece_size, max_s, max_i, max_count, C.byref(self.plan))
        assert rc == 0, self.lib.spmx_gather_last_error()

    def gather(self, ids, io, cap_ids, cap_offs):
        lib = self.lib
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        io = np.ascontiguousarray(io, dtype=np.uint64)
        all_ids = np.full(cap_ids + 4, ID_PAT, dtype=np.int32)
        all_offs = np.full(cap_offs + 4, OFF_PAT, dtype=np.uint64)
        rs = np.full(self.world + 1, SUM_PAT, dtype=np.uint64)
        ri = np.full(self.world + 1, SUM_PAT, dtype=np.uint64)
        rc = lib.spmx_all_gather_ids_packed(self.plan, ids.ctypes.data, io.ctypes.data, len(io) - 1, all_ids.ctypes.data, cap_ids,
                                            all_offs.ctypes.data, cap_offs, rs.ctypes.data, ri.ctypes.data, None)
        assert rc == 0, lib.spmx_gather_last_error()
        code = lib.spmx_gather_plan_status(self.plan, None)
        return code, lib.spmx_gather_last_error(), all_ids, all_offs, rs, ri

    def close(self):
        self.lib.spmx_gather_plan_destroy(self.plan)
        self.lib.spmx_rccl_comm_destroy(self.comm)


def _run_ranks(world, body, timeout=120):
    errors = []

    def guarded(rank):
        try:
            body(rank)
        except BaseException as e:           # noqa: B902 -- reported below, in the test's own thread
            errors.append((rank, e))

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
        assert not t.is_alive(), "a rank hangs"
    assert not errors, errors


@pytest.mark.parametrize("world,cuts", [(2, None), (3, None), (3, [0, 0, 700]), (4, [0, 100, 100, 450])])
@pytest.mark.parametrize("model", ["uni32k", "bpe1k"])
def test_all_gather_ids_packed_over_threads(model, world, cuts, emu_lib, oracle, corpora):
    blob = fixtures.model_blob(model)
    text, offs = fixtures.head(*corpora["synth20k"], 900)
    oids, oio = oracle.load(blob).encode_batch(text, offs)
    n = len(offs) - 1
    if cuts is None:
        sb = sharding.shard_bounds(offs, world)                         # byte-balanced contiguous shards
        bounds = [(int(sb[r]), int(sb[r + 1])) for r in range(world)]
    else:
        bounds = [(cuts[r], cuts[r + 1] if r + 1 < world else n) for r in range(world)]   # uneven, with empty shards
    lib = emu_lib.lib
    uid = (C.c_char * 128)()
    assert lib.spmx_rccl_unique_id(uid) == 0, lib.spmx_gather_last_error()
    handles = [emu_lib.load(blob, classes=None) for _ in range(world)]
    out, wide, sizes = [None] * world, [None] * world, [None] * world

    def run(rank):
        me = _Rank(lib, uid, world, rank)
        a, b = bounds[rank]
        t = text[int(offs[a]):int(offs[b])]
        o = (offs[a:b + 1] - offs[a]).astype(np.uint64)
        ids, io = handles[rank].encode_batch(t, o) if b > a else (np.zeros(0, np.int32), np.zeros(1, np.uint64))
        # every rank passes what IT needs: the plan agrees the maximum
        me.create(int(lib.spmx_piece_size(handles[rank].sp._h)), b - a, len(ids), int(np.diff(io.astype(np.int64)).max()) if b > a else 0)
        sizes[rank] = int(lib.spmx_gather_plan_block_bytes(me.plan))
        out[rank] = me.gather(ids, io, len(oids) + 5, n + 3)
        # the wide call on the same shards
        all_ids = np.full(len(oids), ID_PAT, dtype=np.int32)
        all_offs = np.full(n + 1, OFF_PAT, dtype=np.uint64)
        scratch = np.zeros(int(lib.spmx_gather_scratch_words(world)), dtype=np.uint64)
        ids32, io64 = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(io, dtype=np.uint64)
        assert lib.spmx_all_gather_ids(me.comm, rank, world, ids32.ctypes.data, len(ids32), io64.ctypes.data, b - a, all_ids.ctypes.data,
                                       len(all_ids), all_offs.ctypes.data, len(all_offs), scratch.ctypes.data, None, None, None) == 0
        wide[rank] = (all_ids, all_offs)
        me.close()

    _run_ranks(world, run)
    assert len(set(sizes)) == 1                       # one block size on every rank
    for rank in range(world):
        code, msg, all_ids, all_offs, rs, ri = out[rank]
        assert code == 0, msg
        np.testing.assert_array_equal(all_offs[:n + 1], np.asarray(oio))
        np.testing.assert_array_equal(all_ids[:len(oids)], np.asarray(oids))
        np.testing.assert_array_equal(all_offs[:n + 1], wide[rank][1])
        np.testing.assert_array_equal(all_ids[:len(oids)], wide[rank][0])
        assert (all_ids[len(oids):] == ID_PAT).all() and (all_offs[n + 1:] == OFF_PAT).all()      # nothing written past the CSR
        assert rs.tolist() == [bounds[0][0]] + [b for _, b in bounds]
        assert ri.tolist() == [int(oio[bounds[0][0]])] + [int(oio[b]) for _, b in bounds]


@pytest.mark.parametrize("case", [k for k in _violation_cases() if k != "valid"] + ["an output buffer one id short on one rank"])
def test_all_gather_ids_packed_violation_every_rank_returns_the_same(emu_lib, case):
    """Rank 1 breaks the agreement (or, last case, sizes its output one id short): every rank returns the same status
    naming rank 1, none hangs, nothing is written, and a valid gather on the same plan succeeds afterwards."""
    lib = emu_lib.lib
    world = 3
    cases = _violation_cases()
    valid = cases["valid"][2]
    if case in cases:
        piece_size, max_count, maker, (cap_s, cap_i), code = cases[case]
    else:
        piece_size, max_count, maker, (cap_s, cap_i), code = 65536, 255, valid, (8, 1000), 8
    bad_total = sum(int(valid(r)[1][-1]) for r in range(world))
    uid = (C.c_char * 128)()
    assert lib.spmx_rccl_unique_id(uid) == 0
    first, second = [None] * world, [None] * world

    def run(rank):
        me = _Rank(lib, uid, world, rank)
        me.create(piece_size, cap_s, cap_i, max_count)
        short = 1 if case not in cases and rank == 1 else 0
        first[rank] = me.gather(*maker(rank), (bad_total if case not in cases else 2000) - short, 64)
        second[rank] = me.gather(*valid(rank), 2000, 64)
        me.close()

    _run_ranks(world, run, timeout=60)
    want = expected([valid(r) for r in range(world)])
    for rank in range(world):
        got, msg, all_ids, all_offs, rs, ri = first[rank]
        assert got == code and b"rank 1" in msg, (rank, got, msg)
        assert (all_ids == ID_PAT).all() and (all_offs == OFF_PAT).all() and (rs == SUM_PAT).all() and (ri == SUM_PAT).all()
        got, msg, all_ids, all_offs, rs, ri = second[rank]
        assert got == 0, msg
        np.testing.assert_array_equal(all_ids[:len(want[0])], want[0])
        np.testing.assert_array_equal(all_offs[:len(want[1])], want[1])
        np.testing.assert_array_equal(rs, want[2])
        np.testing.assert_array_equal(ri, want[3])


def test_python_wrappers_over_the_emulated_library(emu_lib):
    """sharding.PackedGatherer / pack_ids / unpack_ids / packed_status with CPU tensors: the same code path a GPU caller takes."""
    import torch
    lib = emu_lib.lib
    shards = [make_csr(300 + 7 * r, 30, 65535, 200 + r) for r in range(2)]
    want = expected(shards)
    cap_s, cap_i = 320, int(max(len(i) for i, _ in shards))
    bb = sharding.packed_block_bytes(65536, cap_s, cap_i, 255, _lib=lib)
    blocks = torch.from_numpy(aligned(2 * bb))
    for r, (ids, o) in enumerate(shards):
        sharding.pack_ids(torch.from_numpy(ids), torch.from_numpy(o.view(np.int64)), 65536, cap_s, cap_i, 255, out=blocks[bb * r:bb * (r + 1)], _lib=lib)
    all_ids = torch.full((len(want[0]),), ID_PAT, dtype=torch.int32)
    all_offs = torch.full((len(want[1]),), OFF_PAT, dtype=torch.int64)
    rs, ri = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    sharding.packed_status(sharding.unpack_ids(blocks, 2, 65536, cap_s, cap_i, 255, all_ids, all_offs, rs, ri, _lib=lib), _lib=lib)
    np.testing.assert_array_equal(all_ids.numpy(), want[0])
    np.testing.assert_array_equal(all_offs.numpy().astype(np.uint64), want[1])
    assert rs.tolist() == want[2].tolist() and ri.tolist() == want[3].tolist()
    with pytest.raises(RuntimeError, match="status 8"):
        sharding.packed_status(sharding.unpack_ids(blocks, 2, 65536, cap_s, cap_i, 255, all_ids[:-1], all_offs, _lib=lib), _lib=lib)
    # the plan at world 1
    uid = (C.c_char * 128)()
    comm = C.c_void_p()
    assert lib.spmx_rccl_unique_id(uid) == 0 and lib.spmx_rccl_comm_init(C.byref(comm), 1, 0, uid) == 0
    ids, o = shards[0]
    g = sharding.PackedGatherer(comm, 0, 1, 65536, len(o) - 1, len(ids), 255, _lib=lib)
    assert g.block_bytes == sharding.packed_block_bytes(65536, len(o) - 1, len(ids), 255, _lib=lib)
    out_ids = torch.full((len(ids),), ID_PAT, dtype=torch.int32)
    out_offs = torch.full((len(o),), OFF_PAT, dtype=torch.int64)
    g(torch.from_numpy(ids), torch.from_numpy(o.view(np.int64)), out_ids, out_offs)
    g.status()
    np.testing.assert_array_equal(out_ids.numpy(), ids)
    np.testing.assert_array_equal(out_offs.numpy().astype(np.uint64), o)
    g(torch.from_numpy(ids), torch.from_numpy(o.view(np.int64)), out_ids[:-1], out_offs)
    with pytest.raises(RuntimeError, match="status 8: rank 0"):
        g.status()
    g.close()
    lib.spmx_rccl_comm_destroy(comm)


def test_plan_rejects_bad_arguments(emu_lib):
    lib = emu_lib.lib
    plan = C.c_void_p()
    assert lib.spmx_gather_plan_create(None, 0, 1, 1000, 1, 1, 1, C.byref(plan)) == 3
    assert lib.spmx_gather_plan_create(C.c_void_p(1), 2, 2, 1000, 1, 1, 1, C.byref(plan)) == 3
    assert lib.spmx_all_gather_ids_packed(None, None, None, 0, None, 0, None, 0, None, None, None) == 3
    assert lib.spmx_gather_plan_status(None, None) == 3 and lib.spmx_gather_plan_block_bytes(None) == 0
    lib.spmx_gather_plan_destroy(None)


@pytest.mark.parametrize("world", [1, 3])
def test_cpp_host_gathers_packed_over_threads(world, emu_lib):
    """tests/cpp/gather_packed_test.cc: the facade's PackedGatherPlan from a C++ host, ranks = threads."""
    src = os.path.join(ROOT, "tests", "cpp", "gather_packed_test.cc")
    out = os.path.join(ROOT, "tests", "cpp", "gather_packed_test_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-o", out, src, "-L" + emu_dir, "-lspmx_emu",
                           "-Wl,-rpath," + emu_dir])
    env = dict(os.environ, SPMX_RCCL_LIB=os.path.join(emu_dir, "libfake_rccl.so"), SPMX_EMU_CUS="2")
    r = subprocess.run([out, os.path.join(fixtures.GOLDEN, "test_model.model"), os.path.join(fixtures.GOLDEN, "botchan.txt"), str(world)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok 600 "), (r.stdout, r.stderr)
