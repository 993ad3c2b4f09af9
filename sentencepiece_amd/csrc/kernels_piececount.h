// The counting side of the reference's `spm_encode --generate_vocabulary` (src/spm_encode_main.cc:102-109): a histogram of
// ids.  The reference counts piece STRINGS in a map; piece strings are unique in a loaded model, so that map is a histogram
// over ids, filtered by piece type when it is written out (api.cc spmx_write_vocabulary).  ids[T] (int32) -> counts[V + 1]
// (uint64), ADDED to what is there: counts[id] for 0 <= id < V, counts[V] for every other value.  The reference counts in
// `int`; the counts here are 64-bit, and the two agree while every count is below 2^31.
//
// The distribution is Zipf-shaped -- one piece can be several per cent of all tokens -- so a global atomic per id would
// serialise on a handful of addresses.  A workgroup therefore owns B = min(V, kCountLdsBins) 32-bit bins in LDS (128 KiB of
// the CU's 160 KiB at the default: one workgroup per CU) and runs three phases with a workgroup barrier between them:
//   zero    the bins
//   sweep   its waves' grid-strided tiles of `ids`, counting into the bins with LDS atomics; an id in [B, V) and an
//           out-of-range value go to HBM directly with one 64-bit atomic
//   flush   every non-zero bin to `counts` with one 64-bit atomic
// The bins hold ids [0, B) -- ASSUMPTION: the low ids are the frequent ones.  Trained models list their pieces by descending
// score (unigram) or in merge order (BPE), so what misses the bins is the rare, spread-out tail.  A synthesised vocabulary
// whose ids are not ordered by frequency still counts correctly: it only loses the privatisation for its tail.
//
// Sweep: a tile is kCountTile ids = kCountLoads 16-byte loads per lane, all issued before the first count, so a wavefront
// keeps 4 KiB in flight; `ids` need only be 4-byte aligned -- the up to 3 ids before the first 16-byte boundary and the up
// to 3 behind the last whole 16 bytes are counted one by one by the grid's first wavefront.  Lanes that hit the same bin in
// one LDS atomic are serialised by the LDS (the worst case, every id equal, is 64 LDS cycles per 64 ids; the HBM side then
// waits for the LDS, which is still one address per CU and not one per chip).
// Traffic per id: 4 bytes read; per workgroup 4 B of LDS zeroed and read back and at most 8 min(B, share) bytes of atomics.
// The host sizes the grid from T (api.cc CountIdsDevice): a small batch runs few workgroups and does not pay a flush of
// 32k bins on each of 256 CUs.  The bins are 32-bit: a workgroup's share stays below 2^32 ids, the host splits a larger
// call into several launches.
#ifndef SPMX_KERNELS_PIECECOUNT_H_
#define SPMX_KERNELS_PIECECOUNT_H_

namespace spmx {

constexpr uint32_t kCountLdsBins = 32768;            // 128 KiB of bins
constexpr uint32_t kCountLdsBinsMin = 64;            // (the floor of the SPMX_COUNT_LDS_BINS test seam)
constexpr uint32_t kCountLoads = 4;                  // 16-byte loads per lane and tile
constexpr uint32_t kCountTile = 64 * 4 * kCountLoads;    // ids per tile: one wavefront, one step
constexpr uint32_t kCountMaxWaves = 16;              // wavefronts per workgroup: four per SIMD hide the loads' latency
constexpr uint64_t kCountMaxLaunch = 1ull << 31;     // ids per launch: no workgroup's share reaches 2^32

struct CountArgs {
  const int32_t *ids;           // T, 4-byte aligned
  uint64_t T;
  unsigned long long *counts;   // V + 1, added to
  uint32_t vocab;               // V
  uint32_t bins;                // B <= V: ids [0, B) are counted in LDS
};

SPMX_DEVICE void count_one(const CountArgs &a, uint32_t *bins, uint32_t id) {
  if (id < a.bins) wv::lds_atomic_add(bins + id, 1u);
  else wv::atomic_add(a.counts + (id < a.vocab ? id : a.vocab), 1ull);      // (a negative id is >= 2^31 here)
}

SPMX_DEVICE void count_zero_phase(const CountArgs &a, uint32_t *bins) {
  const uint32_t stride = static_cast<uint32_t>(wv::waves_per_block()) * 64u;
  for (uint32_t i = static_cast<uint32_t>(wv::wave_in_block()) * 64u + static_cast<uint32_t>(wv::lane()); i < a.bins; i += stride)
    bins[i] = 0u;
}

SPMX_DEVICE void count_sweep_phase(const CountArgs &a, uint32_t *bins) {
  const uint32_t lane = static_cast<uint32_t>(wv::lane());
  // ids [0, head) lie before the first 16-byte boundary, [head + 4 nq, T) behind the last whole 16 bytes
  uint64_t head = ((16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a.ids) & 15u)) & 15u) / 4u;
  if (head > a.T) head = a.T;
  const uint64_t nq = (a.T - head) / 4u;
  const uint64_t tail0 = head + nq * 4u;
  const uint64_t wave = static_cast<uint64_t>(wv::block_id()) * static_cast<uint64_t>(wv::waves_per_block()) + static_cast<uint64_t>(wv::wave_in_block());
  const uint64_t waves = static_cast<uint64_t>(wv::grid_size()) * static_cast<uint64_t>(wv::waves_per_block());
  if (wave == 0) {
    if (lane < head) count_one(a, bins, static_cast<uint32_t>(a.ids[lane]));
    if (tail0 + lane < a.T) count_one(a, bins, static_cast<uint32_t>(a.ids[tail0 + lane]));
  }
  const Q4 *q = reinterpret_cast<const Q4 *>(a.ids + head);
  constexpr uint64_t kTileQ = kCountTile / 4u;       // 16-byte units per tile
  const uint64_t tiles = (nq + kTileQ - 1) / kTileQ;
  for (uint64_t t = wave; t < tiles; t += waves) {
    const uint64_t q0 = t * kTileQ + lane;
    Q4 v[kCountLoads];
    if (q0 - lane + kTileQ <= nq) {                   // a whole tile: every load leaves before the first count
#pragma unroll
      for (uint32_t k = 0; k < kCountLoads; ++k) v[k] = wv::load_stream(q + q0 + k * 64u);
#pragma unroll
      for (uint32_t k = 0; k < kCountLoads; ++k) {
        count_one(a, bins, v[k].x);
        count_one(a, bins, v[k].y);
        count_one(a, bins, v[k].z);
        count_one(a, bins, v[k].w);
      }
    } else {                                          // the last tile
#pragma unroll
      for (uint32_t k = 0; k < kCountLoads; ++k) {
        if (q0 + k * 64u < nq) {
          const Q4 w = wv::load_stream(q + q0 + k * 64u);
          count_one(a, bins, w.x);
          count_one(a, bins, w.y);
          count_one(a, bins, w.z);
          count_one(a, bins, w.w);
        }
      }
    }
  }
}

SPMX_DEVICE void count_flush_phase(const CountArgs &a, const uint32_t *bins) {
  const uint32_t stride = static_cast<uint32_t>(wv::waves_per_block()) * 64u;
  for (uint32_t i = static_cast<uint32_t>(wv::wave_in_block()) * 64u + static_cast<uint32_t>(wv::lane()); i < a.bins; i += stride) {
    const uint32_t c = bins[i];
    if (c) wv::atomic_add(a.counts + i, static_cast<unsigned long long>(c));
  }
}

// the kernel: a workgroup of 1 .. kCountMaxWaves wavefronts (the emulator's launcher runs the phases one after another
// for every wavefront of the workgroup over one LDS image: what the barrier means)
SPMX_DEVICE void count_ids_block(const CountArgs &a, unsigned char *smem) {
  uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
  count_zero_phase(a, bins);
  wv::block_sync();
  count_sweep_phase(a, bins);
  wv::block_sync();
  count_flush_phase(a, bins);
}

}  // namespace spmx
#endif
