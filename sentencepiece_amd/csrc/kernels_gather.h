// Multi-GPU gather of the token ids (spmx_all_gather_ids, gather.cc): after the ids and the per-sentence offsets of
// every rank have arrived, the offsets of rank r's sentences are moved from "ids before me on rank r" to "ids before
// me in the whole job" -- + the ids of the ranks before r.  One launch over all sentences; the rank of a sentence by a
// search over the (at most kMaxRanks + 1) sentence prefix sums held in the kernel's arguments.
#ifndef SPMX_KERNELS_GATHER_H_
#define SPMX_KERNELS_GATHER_H_

namespace spmx {

constexpr int kMaxRanks = 64;

struct RebaseArgs {
  uint64_t *offs;                      // [total_sentences + 1]: every rank's LOCAL offsets back to back; [total] gets the total
  uint32_t world;
  uint64_t sent_before[kMaxRanks + 1]; // sentences on the ranks before r (prefix sums, [world] = total)
  uint64_t ids_before[kMaxRanks + 1];  // ids on the ranks before r ([world] = total)
};

SPMX_DEVICE void rebase_block(const RebaseArgs &a) {
  const uint64_t total = a.sent_before[a.world];
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  for (uint64_t i = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(wv::lane()); i <= total; i += stride) {
    if (i == total) { a.offs[i] = a.ids_before[a.world]; continue; }
    uint32_t lo = 0, hi = a.world;                 // sent_before[lo] <= i < sent_before[hi]
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.sent_before[mid] <= i) lo = mid; else hi = mid;
    }
    a.offs[i] += a.ids_before[lo];
  }
}

// ---- packed gather (spmx_all_gather_ids_packed / spmx_pack_ids / spmx_unpack_ids, gather.cc) -------------------------
// The wire block of one rank (include/spmx.h documents it for hosts; version kPackedVersion).  Every section starts at a
// multiple of 128 bytes that follows from the AGREED capacities alone, so every rank's block has the same layout:
//   header   16 uint64 (PackedHeader below)
//   bases    per tile of kPackedTile sentences the rank-local id offset at the tile's start, uint64
//   counts   ids per sentence, count_width bytes each
//   ids      id_width bytes each
// Side information: 128 + 8 * ceil(cap_s / 256) + three paddings below 128 <= cap_s / 32 + 520 bytes.
constexpr uint32_t kPackedVersion = 1;
constexpr uint32_t kPackedMagic = 0x58504B31u;   // "1KPX": what the upper half of header word 0 holds
constexpr uint32_t kPackedTile = 256;            // sentences per tile: four per lane
constexpr uint32_t kPackedUnit = 8;              // ids per lane per access: 32 bytes of int32, 16 bytes of 16-bit ids
// header words (uint64 each)
enum : uint32_t {
  kPhVersion = 0,     // kPackedVersion | kPackedMagic << 32
  kPhSentences = 1,   // what the sender packed (status != 0: what it was asked to pack; the block then carries NO sentences)
  kPhIds = 2,
  kPhWidths = 3,      // id width | count width << 8
  kPhStatus = 4,      // kPs* bits, 0 = a valid block (the low 32 bits are written with atomics)
  kPhCapIds = 5,      // capacity of the sender's own d_all_ids
  kPhCapOffsets = 6,  // ... of its d_all_id_offsets
  kPhAgreedSentences = 7,
  kPhAgreedIds = 8,
  kPhWords = 16,
};
// status bits: of a block (the pack kernel sets them) and of a gather (the unpack kernel adds the last two)
enum : uint32_t {
  kPsSentences = 1u << 0,   // more sentences than agreed                     -> 8
  kPsIds = 1u << 1,         // more ids than agreed                           -> 8
  kPsCount = 1u << 2,       // a sentence's id count outside the count width  -> 11
  kPsId = 1u << 3,          // an id outside the id width                     -> 11
  kPsArgs = 1u << 4,        // a null buffer with a non-zero size             -> 3
  kPsOutput = 1u << 5,      // the gathered CSR does not fit a rank's output  -> 8
  kPsFormat = 1u << 6,      // not a block of this version / these capacities -> 13
};
SPMX_HD inline int PackedStatusCode(uint32_t bits) {
  if (bits & kPsFormat) return 13;
  if (bits & kPsArgs) return 3;
  if (bits & (kPsSentences | kPsIds | kPsOutput)) return 8;
  if (bits & (kPsCount | kPsId)) return 11;
  return 0;
}

struct PackedLayout {
  uint64_t cap_s, cap_i;        // agreed capacities: sentences, ids
  uint32_t idw, cw;             // bytes per id (2, 4), per count (1, 2, 4)
  uint64_t off_bases, off_counts, off_ids, bytes;
};
SPMX_HD inline uint64_t PackedAlign(uint64_t v) { return (v + 127u) & ~static_cast<uint64_t>(127u); }
SPMX_HD inline PackedLayout MakePackedLayout(uint32_t piece_size, uint64_t cap_s, uint64_t cap_i, uint64_t max_count) {
  PackedLayout l;
  l.cap_s = cap_s;
  l.cap_i = cap_i;
  l.idw = piece_size <= 65536u ? 2u : 4u;
  l.cw = max_count <= 255u ? 1u : (max_count <= 65535u ? 2u : 4u);
  l.off_bases = kPhWords * 8u;
  l.off_counts = l.off_bases + PackedAlign(8u * ((cap_s + kPackedTile - 1u) / kPackedTile));
  l.off_ids = l.off_counts + PackedAlign(cap_s * l.cw);
  l.bytes = l.off_ids + PackedAlign(cap_i * l.idw);
  return l;
}

struct PackArgs {
  const int32_t *ids;
  const uint64_t *offs;        // [n + 1] (null when n == 0)
  uint64_t n;
  uint8_t *block;              // 128-byte aligned, lay.bytes; header word kPhStatus is zero at the launch
  PackedLayout lay;
  uint64_t out_cap_ids, out_cap_offs;   // of the sender's gather outputs: they travel in the header
  uint32_t bad_args;
};

struct UnpackArgs {
  const uint8_t *blocks;       // world blocks, block_stride bytes apart
  uint64_t block_stride;
  uint32_t world;
  PackedLayout lay;
  int32_t *all_ids;
  uint64_t *all_offs;
  uint64_t cap_ids, cap_offs;  // of this rank's outputs
  uint64_t *rank_sentences, *rank_ids;   // [world + 1] each, nullable
  uint64_t *status;            // [4]: StatusCode number, offending rank (0xFFFFFFFF: the caller's own outputs), status bits, ids in the valid blocks
};

// 16 bytes to / from an address that is only 2- or 4-byte aligned (the narrow side of a stream whose wide side is aligned):
// one global_load / store_dwordx4 on gfx950 (unaligned access is on under HSA), a memcpy on the CPU model
struct PackedU4 { uint32_t x, y, z, w; };
SPMX_DEVICE PackedU4 packed_load16(const void *p) { PackedU4 v; __builtin_memcpy(&v, p, 16); return v; }
SPMX_DEVICE void packed_store16(void *p, const PackedU4 &v) { __builtin_memcpy(p, &v, 16); }

// the items b, b + grid, ... of [0, n) rotated by `done` items already dealt out, so that consecutive ranges (the ranks of
// an unpack) keep every workgroup busy: first item of workgroup b
SPMX_DEVICE uint64_t packed_first(uint64_t done, uint32_t b, uint32_t grid) {
  const uint32_t r = static_cast<uint32_t>(done % grid);
  return b >= r ? b - r : b + grid - r;
}

// inclusive prefix sum over the lanes of values below 2^40 (four counts of 32 bits are below 2^34): wv::scan_add is a
// 32-bit scan, so the value travels as 24 + 16 bits -- 64 lanes of 24 bits stay below 2^30
SPMX_DEVICE uint64_t packed_scan64(uint64_t v) {
  const uint32_t lo = wv::scan_add(static_cast<uint32_t>(v) & 0xFFFFFFu);
  const uint32_t hi = wv::scan_add(static_cast<uint32_t>(v >> 24));
  return (static_cast<uint64_t>(hi) << 24) + lo;
}

SPMX_DEVICE void pack_block(const PackArgs &a) {
  const uint32_t b = static_cast<uint32_t>(wv::block_id()), grid = static_cast<uint32_t>(wv::grid_size());
  const uint32_t lane = static_cast<uint32_t>(wv::lane());
  uint64_t *hdr = reinterpret_cast<uint64_t *>(a.block);
  uint32_t *status = reinterpret_cast<uint32_t *>(hdr + kPhStatus);
  const PackedLayout &L = a.lay;
  // ---- what every workgroup decides alike before any payload is written ----
  const uint64_t base = a.n && !a.bad_args ? a.offs[0] : 0u;
  const uint64_t n_ids = a.n && !a.bad_args ? a.offs[a.n] - base : 0u;      // (offsets that run backwards wrap to a huge count: flagged)
  uint32_t bad = a.bad_args || (n_ids && !a.ids) ? kPsArgs : 0u;
  if (a.n > L.cap_s) bad |= kPsSentences;
  if (n_ids > L.cap_i) bad |= kPsIds;
  if (b == 0 && lane == 0) {
    hdr[kPhVersion] = kPackedVersion | static_cast<uint64_t>(kPackedMagic) << 32;
    hdr[kPhSentences] = a.n;
    hdr[kPhIds] = n_ids;
    hdr[kPhWidths] = L.idw | L.cw << 8;
    hdr[kPhCapIds] = a.out_cap_ids;
    hdr[kPhCapOffsets] = a.out_cap_offs;
    hdr[kPhAgreedSentences] = L.cap_s;
    hdr[kPhAgreedIds] = L.cap_i;
    if (bad) wv::atomic_or(status, bad);
  }
  if (bad) return;
  uint32_t found = 0;
  // ---- counts and tile bases: a tile of 256 sentences per step, four sentences per lane ----
  uint64_t *bases = reinterpret_cast<uint64_t *>(a.block + L.off_bases);
  uint8_t *counts = a.block + L.off_counts;
  const uint64_t tiles = (a.n + kPackedTile - 1u) / kPackedTile;
  const uint64_t cmax = L.cw == 1u ? 0xFFu : (L.cw == 2u ? 0xFFFFu : 0xFFFFFFFFu);
  for (uint64_t t = b; t < tiles; t += grid) {
    const uint64_t s0 = t * kPackedTile + 4u * lane;
    if (lane == 0) bases[t] = a.offs[s0] - base;
    if (s0 >= a.n) continue;
    const uint32_t m = a.n - s0 >= 4u ? 4u : static_cast<uint32_t>(a.n - s0);
    uint64_t o[5];
    o[0] = a.offs[s0];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) o[k + 1] = k < m ? a.offs[s0 + k + 1] : o[k];
    uint32_t c[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint64_t d = o[k + 1] - o[k];
      if (d > cmax) found |= kPsCount;
      c[k] = static_cast<uint32_t>(d);
    }
    if (m == 4u) {          // one aligned store of four counts (the section and the tile are 128-byte aligned)
      if (L.cw == 1u) *reinterpret_cast<uint32_t *>(counts + s0) = c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24;
      else if (L.cw == 2u) *reinterpret_cast<D2 *>(counts + 2u * s0) = D2{c[0] | c[1] << 16, c[2] | c[3] << 16};
      else *reinterpret_cast<Q4 *>(counts + 4u * s0) = Q4{c[0], c[1], c[2], c[3]};
    } else {
      for (uint32_t k = 0; k < m; ++k) {
        if (L.cw == 1u) counts[s0 + k] = static_cast<uint8_t>(c[k]);
        else if (L.cw == 2u) reinterpret_cast<uint16_t *>(counts)[s0 + k] = static_cast<uint16_t>(c[k]);
        else reinterpret_cast<uint32_t *>(counts)[s0 + k] = c[k];
      }
    }
  }
  // ---- ids: aligned on the int32 side; eight ids per lane per step, the head and the tail one id per lane ----
  const int32_t *src = a.ids + base;
  uint8_t *dst = a.block + L.off_ids;
  uint64_t head = ((16u - (reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) / 4u;
  if (head > n_ids) head = n_ids;
  const uint64_t units = (n_ids - head) / kPackedUnit;
  const uint64_t tail0 = head + units * kPackedUnit;
  if (b == 0 && lane < kPackedUnit) {
    for (uint32_t pass = 0; pass < 2u; ++pass) {
      const uint64_t i = pass == 0 ? lane : tail0 + lane;
      if (i >= (pass == 0 ? head : n_ids)) continue;
      const uint32_t v = static_cast<uint32_t>(src[i]);
      if (L.idw == 2u) {
        if (v > 0xFFFFu) found |= kPsId;
        reinterpret_cast<uint16_t *>(dst)[i] = static_cast<uint16_t>(v);
      } else {
        reinterpret_cast<uint32_t *>(dst)[i] = v;
      }
    }
  }
  const Q4 *wide = reinterpret_cast<const Q4 *>(src + head);
  const uint64_t stride = static_cast<uint64_t>(grid) * 64u;
  if (L.idw == 2u) {
    uint8_t *out = dst + 2u * head;
    for (uint64_t u = static_cast<uint64_t>(b) * 64u + lane; u < units; u += stride) {
      const Q4 p = wide[2u * u], q = wide[2u * u + 1u];
      if ((p.x | p.y | p.z | p.w | q.x | q.y | q.z | q.w) > 0xFFFFu) found |= kPsId;
      packed_store16(out + 16u * u, PackedU4{(p.x & 0xFFFFu) | p.y << 16, (p.z & 0xFFFFu) | p.w << 16,
                                             (q.x & 0xFFFFu) | q.y << 16, (q.z & 0xFFFFu) | q.w << 16});
    }
  } else {
    uint8_t *out = dst + 4u * head;
    for (uint64_t u = static_cast<uint64_t>(b) * 64u + lane; u < units; u += stride) {
      const Q4 p = wide[2u * u], q = wide[2u * u + 1u];
      packed_store16(out + 32u * u, PackedU4{p.x, p.y, p.z, p.w});
      packed_store16(out + 32u * u + 16u, PackedU4{q.x, q.y, q.z, q.w});
    }
  }
  if (found) wv::atomic_or(status, found);
}

SPMX_DEVICE void unpack_block(const UnpackArgs &a) {
  const uint32_t b = static_cast<uint32_t>(wv::block_id()), grid = static_cast<uint32_t>(wv::grid_size());
  const uint32_t lane = static_cast<uint32_t>(wv::lane());
  const PackedLayout &L = a.lay;
  // ---- every workgroup reads the world's headers itself: totals, the first rank in trouble ----
  uint64_t total_s = 0, total_i = 0;
  uint32_t bits = 0, bad_rank = 0;
  uint64_t min_cap_i = ~0ull, min_cap_o = ~0ull;
  uint32_t cap_rank_i = 0xFFFFFFFFu, cap_rank_o = 0xFFFFFFFFu;     // the first ranks that hold those minima (none: only this caller's are smaller)
  for (uint32_t r = 0; r < a.world; ++r) {
    const uint64_t *h = reinterpret_cast<const uint64_t *>(a.blocks + r * a.block_stride);
    uint32_t s = static_cast<uint32_t>(h[kPhStatus]);
    if (h[kPhVersion] != (kPackedVersion | static_cast<uint64_t>(kPackedMagic) << 32) || h[kPhWidths] != (L.idw | L.cw << 8) ||
        h[kPhAgreedSentences] != L.cap_s || h[kPhAgreedIds] != L.cap_i)
      s = kPsFormat;
    else if (!s && (h[kPhSentences] > L.cap_s || h[kPhIds] > L.cap_i))
      s = kPsFormat;
    if (s && !bits) { bits = s; bad_rank = r; }
    if (s) continue;
    total_s += h[kPhSentences];
    total_i += h[kPhIds];
    if (h[kPhCapIds] < min_cap_i) { min_cap_i = h[kPhCapIds]; cap_rank_i = r; }
    if (h[kPhCapOffsets] < min_cap_o) { min_cap_o = h[kPhCapOffsets]; cap_rank_o = r; }
  }
  const uint64_t my_cap_i = a.all_ids ? a.cap_ids : 0u, my_cap_o = a.all_offs ? a.cap_offs : 0u;
  if (my_cap_i < min_cap_i) { min_cap_i = my_cap_i; cap_rank_i = 0xFFFFFFFFu; }
  if (my_cap_o < min_cap_o) { min_cap_o = my_cap_o; cap_rank_o = 0xFFFFFFFFu; }
  if (!bits && (total_i > min_cap_i || total_s + 1u > min_cap_o)) {
    bits = kPsOutput;
    bad_rank = total_i > min_cap_i ? cap_rank_i : cap_rank_o;
  }
  if (b == 0 && lane == 0) {
    a.status[0] = static_cast<uint64_t>(PackedStatusCode(bits));
    a.status[1] = bad_rank;
    a.status[2] = bits;
    a.status[3] = total_i;
  }
  if (bits) return;
  if (b == 0 && lane == 0) {
    a.all_offs[total_s] = total_i;
    if (a.rank_sentences) a.rank_sentences[a.world] = total_s;
    if (a.rank_ids) a.rank_ids[a.world] = total_i;
  }
  uint64_t sbase = 0, ibase = 0, done_t = 0, done_u = 0;
  for (uint32_t r = 0; r < a.world; ++r) {
    const uint8_t *blk = a.blocks + r * a.block_stride;
    const uint64_t *h = reinterpret_cast<const uint64_t *>(blk);
    const uint64_t n = h[kPhSentences], n_ids = h[kPhIds];
    if (b == 0 && lane == 0) {
      if (a.rank_sentences) a.rank_sentences[r] = sbase;
      if (a.rank_ids) a.rank_ids[r] = ibase;
    }
    // ---- offsets: a tile per step; its base from the block, inside it a wave-local scan of the counts ----
    const uint64_t *bases = reinterpret_cast<const uint64_t *>(blk + L.off_bases);
    const uint8_t *counts = blk + L.off_counts;
    const uint64_t tiles = (n + kPackedTile - 1u) / kPackedTile;
    for (uint64_t t = packed_first(done_t, b, grid); t < tiles; t += grid) {
      const uint64_t s0 = t * kPackedTile + 4u * lane;
      const uint32_t m = s0 >= n ? 0u : (n - s0 >= 4u ? 4u : static_cast<uint32_t>(n - s0));
      uint32_t c[4] = {0, 0, 0, 0};
      if (m == 4u) {
        if (L.cw == 1u) {
          const uint32_t w = *reinterpret_cast<const uint32_t *>(counts + s0);
          c[0] = w & 0xFFu; c[1] = (w >> 8) & 0xFFu; c[2] = (w >> 16) & 0xFFu; c[3] = w >> 24;
        } else if (L.cw == 2u) {
          const D2 w = *reinterpret_cast<const D2 *>(counts + 2u * s0);
          c[0] = w.x & 0xFFFFu; c[1] = w.x >> 16; c[2] = w.y & 0xFFFFu; c[3] = w.y >> 16;
        } else {
          const Q4 w = *reinterpret_cast<const Q4 *>(counts + 4u * s0);
          c[0] = w.x; c[1] = w.y; c[2] = w.z; c[3] = w.w;
        }
      } else {
        for (uint32_t k = 0; k < m; ++k)
          c[k] = L.cw == 1u ? counts[s0 + k] : (L.cw == 2u ? reinterpret_cast<const uint16_t *>(counts)[s0 + k] : reinterpret_cast<const uint32_t *>(counts)[s0 + k]);
      }
      const uint64_t mine = static_cast<uint64_t>(c[0]) + c[1] + c[2] + c[3];
      // (one or two bytes per count: a tile's sum is below 2^24, one 32-bit scan; four bytes: kept in 64 bits)
      const uint64_t incl = L.cw == 4u ? packed_scan64(mine) : static_cast<uint64_t>(wv::scan_add(static_cast<uint32_t>(mine)));
      uint64_t v = ibase + bases[t] + (incl - mine);
      uint64_t *out = a.all_offs + sbase + s0;
      if (m == 4u) {
        const uint64_t v1 = v + c[0], v2 = v1 + c[1], v3 = v2 + c[2];
        if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
          *reinterpret_cast<L2 *>(out) = L2{v, v1};
          *reinterpret_cast<L2 *>(out + 2) = L2{v2, v3};
        } else {
          out[0] = v;
          *reinterpret_cast<L2 *>(out + 1) = L2{v1, v2};
          out[3] = v3;
        }
      } else {
        for (uint32_t k = 0; k < m; ++k) { out[k] = v; v += c[k]; }
      }
    }
    done_t += tiles;
    // ---- ids: aligned on the int32 side (the destination, at an arbitrary element of the job's array) ----
    int32_t *dst = a.all_ids + ibase;
    const uint8_t *src = blk + L.off_ids;
    uint64_t head = ((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u;
    if (head > n_ids) head = n_ids;
    const uint64_t units = (n_ids - head) / kPackedUnit;
    const uint64_t tail0 = head + units * kPackedUnit;
    if (packed_first(done_u, b, grid) == 0u && lane < kPackedUnit) {     // (the workgroup that also takes this rank's first unit)
      for (uint32_t pass = 0; pass < 2u; ++pass) {
        const uint64_t i = pass == 0 ? lane : tail0 + lane;
        if (i >= (pass == 0 ? head : n_ids)) continue;
        dst[i] = L.idw == 2u ? static_cast<int32_t>(reinterpret_cast<const uint16_t *>(src)[i])
                             : static_cast<int32_t>(reinterpret_cast<const uint32_t *>(src)[i]);
      }
    }
    Q4 *wide = reinterpret_cast<Q4 *>(dst + head);
    const uint64_t groups = (units + 63u) / 64u;
    if (L.idw == 2u) {
      const uint8_t *in = src + 2u * head;
      for (uint64_t g = packed_first(done_u, b, grid); g < groups; g += grid) {
        const uint64_t u = g * 64u + lane;
        if (u >= units) continue;
        const PackedU4 p = packed_load16(in + 16u * u);
        wide[2u * u] = Q4{p.x & 0xFFFFu, p.x >> 16, p.y & 0xFFFFu, p.y >> 16};
        wide[2u * u + 1u] = Q4{p.z & 0xFFFFu, p.z >> 16, p.w & 0xFFFFu, p.w >> 16};
      }
    } else {
      const uint8_t *in = src + 4u * head;
      for (uint64_t g = packed_first(done_u, b, grid); g < groups; g += grid) {
        const uint64_t u = g * 64u + lane;
        if (u >= units) continue;
        const PackedU4 p = packed_load16(in + 32u * u), q = packed_load16(in + 32u * u + 16u);
        wide[2u * u] = Q4{p.x, p.y, p.z, p.w};
        wide[2u * u + 1u] = Q4{q.x, q.y, q.z, q.w};
      }
    }
    done_u += groups;
    sbase += n;
    ibase += n_ids;
  }
}

}  // namespace spmx
#endif
