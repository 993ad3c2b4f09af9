// The lattice kernel's sparse results -> the dense CSR every other device call speaks.
//
// kernels_nbest.h leaves, after all its launches (the wide launches over the sentences set aside included), per sentence
// s a count res_count[s] and per slot (s, k < res_count[s]) of its K = NBestArgs::nbest slots where the result's ids sit
// in the id arena (res_off), how many they are (res_len) and the result's score.  Arena order is the order in which the
// lanes happened to allocate.  From that:
//   (scan)  kernels.h LaunchScan over res_count                       -> result_offsets[n + 1]
//   rows    a lane per RESULT r (1024 results per chunk; its sentence by binary search over result_offsets within the
//           chunk's range, as the token-text length pass finds an item's sentence)
//                                      -> row_len[r], row_src[r] (its place in the arena), scores[r], sent_of_result[r]
//   (scan)  LaunchScan over row_len                                   -> id_offsets[R + 1]
//   gather  by 16-byte blocks of the OUTPUT ids[T], aligned on the destination's address: a lane owns one block (4
//           ids), finds the result of its first id by binary search over id_offsets within the chunk's range and
//           searches again, from there on, only where a block crosses into another result -- results without ids are
//           stepped over by the search, not walked -- reads the arena at whatever alignment the source has (neighbouring
//           lanes read neighbouring words) and stores the block whole.  The image's first and last block go out by
//           elements.
// No lane walks a sentence or a result: a result of 5,000 ids spreads over 1,250 lanes and 5,000 results of one id over
// 1,250 as well.  The same gather runs once more per span arena (arena_nb / arena_ne) where the caller asks for the dense
// nbegin[T] / nend[T]: the token ranges in the DEVICE form of the normalized text, the negative bos / eos markers as they are.
//
// refspan  what the piece writer (kernels_tokentext.h) needs from those: ranges in the REFERENCE form of the normalized text,
//          where U+2581 is three bytes and not the one byte kSpByte.  A flag per byte of the device-form text (is it kSpByte),
//          the project's scan over the flags, then a lane per TOKEN: its result by binary search over id_offsets, the
//          result's sentence through sent_of_result, and position p of that sentence becomes p + 2 * (stand-ins before p).
//          A marker (bos / eos) becomes the empty range at 0: such a token's piece is its name.  A lane per RESULT gathers
//          the result's normalized base, norm_offs[sent_of_result[r]]: the writer's "sentence" is a result.
//
// pick    SampleEncode with nbest_size > 1 (src/sentencepiece_processor.cc:700-716): a lane per sentence draws one of
//         its results with probability exp(alpha * score) / Z -- the rule of api.cc SampleEncodeImpl's host loop, in
//         double, keyed by (seed, index_base + sentence) -- and moves the chosen row into the sentence's slot 0.  The
//         rows pass then runs with the identity for result_offsets (row s = slot (s, 0)).
//
// HBM-bound, no LDS.  Per result 24 bytes read + 16 (+ 8) written by the rows pass and 4 + 8 by its scan; per id 4 read
// and 4 written, plus the searches' reads of id_offsets (log2 of the results a chunk covers, from L2).
#ifndef SPMX_KERNELS_LATTICECSR_H_
#define SPMX_KERNELS_LATTICECSR_H_

namespace spmx {

constexpr uint32_t kLcRowChunk = 1024;       // results per chunk of the rows pass: 64 lanes x 16 steps
constexpr uint32_t kLcOutChunk = 4096;       // ids per chunk of the gather: 64 lanes x 4 ids (16 bytes) x 16 steps

struct LatticeCsrArgs {
  // what the lattice kernel left
  const unsigned long long *res_off;    // [n][K]
  const uint32_t *res_len;              // [n][K]
  const float *res_score;               // [n][K]
  uint32_t K;
  uint64_t n;
  // rows pass
  const uint64_t *result_offs;          // n + 1; null: the identity (the picked form: row s is slot (s, 0))
  uint64_t R;                           // result_offs[n]
  uint32_t *row_len;                    // R
  unsigned long long *row_src;          // R
  float *scores;                        // R, nullable
  uint32_t *sent_of_result;             // R, nullable
  // gather pass
  const uint64_t *id_offs;              // R + 1
  const int32_t *arena;                 // the id arena, or one of the span arenas
  int32_t *out;                         // T
  uint64_t T;                           // id_offs[R]
};

SPMX_DEVICE void latticecsr_rows_block(const LatticeCsrArgs &a) {
  if (a.R == 0 || a.n == 0) return;
  const int lane = wv::lane();
  const uint64_t chunks = (a.R + kLcRowChunk - 1) / kLcRowChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t r0 = ch * kLcRowChunk;
    const uint64_t r1 = r0 + kLcRowChunk < a.R ? r0 + kLcRowChunk : a.R;
    // the sentences of the chunk's first and last result (the same in every lane)
    uint64_t lo = 0, hi = 0;
    if (a.result_offs) {
      lo = tt_item_of(a.result_offs, 0, a.n - 1, r0);
      hi = tt_item_of(a.result_offs, lo, a.n - 1, r1 - 1);
    }
    for (uint32_t step = 0; step < kLcRowChunk / 64u; ++step) {
      const uint64_t r = r0 + step * 64u + static_cast<uint64_t>(lane);
      if (r >= r1) break;
      // (a sentence without results shares its offset with the next one: the largest s with result_offs[s] <= r owns r)
      const uint64_t s = a.result_offs ? tt_item_of(a.result_offs, lo, hi, r) : r;
      const uint64_t slot = s * a.K + (a.result_offs ? r - a.result_offs[s] : 0);
      a.row_len[r] = a.res_len[slot];
      a.row_src[r] = a.res_off[slot];
      if (a.scores) a.scores[r] = a.res_score[slot];
      if (a.sent_of_result) a.sent_of_result[r] = static_cast<uint32_t>(s);
    }
  }
}

SPMX_DEVICE void latticecsr_gather_block(const LatticeCsrArgs &a) {
  if (a.T == 0 || a.R == 0) return;
  const int lane = wv::lane();
  // blocks are aligned on the destination ADDRESS: block b holds the ids [4 b - mis, 4 b - mis + 4)
  const uint64_t mis = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(a.out) & 15u) >> 2;
  const uint64_t span = a.T + mis;
  const uint64_t chunks = (span + kLcOutChunk - 1) / kLcOutChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t c0 = ch * kLcOutChunk;
    const uint64_t c1 = c0 + kLcOutChunk < span ? c0 + kLcOutChunk : span;
    // the results of the chunk's first and last id (the same in every lane)
    const uint64_t lo = tt_item_of(a.id_offs, 0, a.R - 1, c0 > mis ? c0 - mis : 0);
    const uint64_t hi = tt_item_of(a.id_offs, lo, a.R - 1, c1 - mis - 1);
    for (uint32_t step = 0; step < kLcOutChunk / 256u; ++step) {
      const uint64_t b0 = c0 + step * 256u + static_cast<uint64_t>(lane) * 4u;     // in address units: id b0 - mis
      if (b0 >= c1) break;
      const uint64_t t0 = b0 > mis ? b0 - mis : 0;
      const uint64_t t1 = b0 + 4 - mis < a.T ? b0 + 4 - mis : a.T;
      uint64_t r = tt_item_of(a.id_offs, lo, hi, t0);
      uint64_t st = a.id_offs[r], en = a.id_offs[r + 1];
      int32_t v[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint64_t t = t0 + static_cast<uint64_t>(k);
        if (t >= t1) continue;
        if (t >= en) {                                  // into another result: the one that holds t, whatever lies between
          r = tt_item_of(a.id_offs, r + 1, hi, t);
          st = a.id_offs[r];
          en = a.id_offs[r + 1];
        }
        v[k] = a.arena[a.row_src[r] + (t - st)];
      }
      if (t1 - t0 == 4) {
        *reinterpret_cast<Q4 *>(a.out + t0) = Q4{static_cast<uint32_t>(v[0]), static_cast<uint32_t>(v[1]),
                                                  static_cast<uint32_t>(v[2]), static_cast<uint32_t>(v[3])};
      } else {                                          // the image's first or last block
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (t0 + static_cast<uint64_t>(k) < t1) a.out[t0 + static_cast<uint64_t>(k)] = v[k];
      }
    }
  }
}

// result_offsets, sent_of_result and scores of a call that went to the plain encoder: one result per sentence, score 0
struct LatticeIotaArgs {
  uint64_t n;
  uint64_t *result_offs;                // n + 1, nullable
  uint32_t *sent_of_result;             // n, nullable
  float *scores;                        // n, nullable
};
SPMX_DEVICE void latticecsr_iota_block(const LatticeIotaArgs &a) {
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  for (uint64_t s = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(wv::lane()); s <= a.n; s += stride) {
    if (a.result_offs) a.result_offs[s] = s;
    if (s < a.n && a.sent_of_result) a.sent_of_result[s] = static_cast<uint32_t>(s);
    if (s < a.n && a.scores) a.scores[s] = 0.f;
  }
}

// The longest sentence of a batch in raw bytes (the first lattice launch sizes its slices by it): a lane per sentence,
// grid-strided, the wave's maximum by a DPP scan, one atomic per wave.  Lengths saturate at 2^32 - 1.
struct LatticeMaxLenArgs {
  const uint64_t *offs;                 // n + 1
  uint64_t n;
  unsigned long long *max_len;          // zeroed by the caller
};
SPMX_DEVICE void latticecsr_maxlen_block(const LatticeMaxLenArgs &a) {
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  uint32_t mine = 0;
  for (uint64_t s = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(wv::lane()); s < a.n; s += stride) {
    const uint64_t b = a.offs[s], e = a.offs[s + 1];
    const uint64_t len = e > b ? e - b : 0;
    const uint32_t l32 = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(len);
    mine = l32 > mine ? l32 : mine;
  }
  const uint32_t top = wv::scan_max(mine);
  if (wv::lane() == 63 && top) wv::atomic_max(a.max_len, static_cast<unsigned long long>(top));
}

// ---- device-form token ranges -> what the piece writer reads (see the head of this file)
struct LatticeRefSpanArgs {
  const uint8_t *dnorm;                 // the device-form normalized text, dnorm_bytes
  uint64_t dnorm_bytes;
  uint32_t *flag;                       // dnorm_bytes (flags pass out)
  const uint64_t *pre;                  // dnorm_bytes + 1: stand-ins before a byte (scan out)
  const uint64_t *id_offs;              // R + 1
  uint64_t R, T;
  const uint32_t *sent;                 // R: sent_of_result
  const uint64_t *dnoffs;               // n + 1: the sentences in dnorm
  const uint64_t *rnoffs;               // n + 1: the sentences in the reference-form text
  int32_t *nbegin, *nend;               // T: in the device form, out the reference form (as uint32)
  uint64_t *res_noffs;                  // R (out): rnoffs[sent[r]]
};
SPMX_DEVICE void latticecsr_spflag_block(const LatticeRefSpanArgs &a) {
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  for (uint64_t i = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(wv::lane()); i < a.dnorm_bytes; i += stride)
    a.flag[i] = a.dnorm[i] == kSpByte ? 1u : 0u;
}
SPMX_DEVICE void latticecsr_refspan_block(const LatticeRefSpanArgs &a) {
  const int lane = wv::lane();
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  for (uint64_t r = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(lane); r < a.R; r += stride)
    a.res_noffs[r] = a.rnoffs[a.sent[r]];
  if (a.T == 0 || a.R == 0) return;
  const uint64_t chunks = (a.T + kLcRowChunk - 1) / kLcRowChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t t0 = ch * kLcRowChunk;
    const uint64_t t1 = t0 + kLcRowChunk < a.T ? t0 + kLcRowChunk : a.T;
    const uint64_t lo = tt_item_of(a.id_offs, 0, a.R - 1, t0);
    const uint64_t hi = tt_item_of(a.id_offs, lo, a.R - 1, t1 - 1);
    for (uint32_t step = 0; step < kLcRowChunk / 64u; ++step) {
      const uint64_t t = t0 + step * 64u + static_cast<uint64_t>(lane);
      if (t >= t1) break;
      const int32_t nb = a.nbegin[t], ne = a.nend[t];
      if (nb < 0 || ne < nb) { a.nbegin[t] = 0; a.nend[t] = 0; continue; }
      const uint64_t base = a.dnoffs[a.sent[tt_item_of(a.id_offs, lo, hi, t)]];
      const uint64_t p0 = a.pre[base];
      a.nbegin[t] = static_cast<int32_t>(static_cast<uint64_t>(nb) + 2u * (a.pre[base + static_cast<uint64_t>(nb)] - p0));
      a.nend[t] = static_cast<int32_t>(static_cast<uint64_t>(ne) + 2u * (a.pre[base + static_cast<uint64_t>(ne)] - p0));
    }
  }
}

struct LatticePickArgs {
  const uint32_t *res_count;            // [n]
  unsigned long long *res_off;          // [n][K]: slot 0 receives the chosen row
  uint32_t *res_len;
  float *res_score;
  uint32_t K;
  uint64_t n;
  float alpha;
  uint64_t seed, index_base;            // the draw of sentence s is keyed by (seed, index_base + s)
};

// api.cc SampleEncodeImpl's host loop, a lane per sentence: max-shifted exp(alpha * score) weights in double, a
// splitmix64-style hash of (seed, sentence) as a 53-bit uniform, a walk over the cumulative weights with the last
// result as the fallback.  exp is the device's here and glibc's there: a draw within an ulp of a boundary may differ.
SPMX_DEVICE void latticecsr_pick_block(const LatticePickArgs &a) {
#pragma clang fp contract(off)
  const uint64_t stride = static_cast<uint64_t>(wv::grid_size()) * 64u;
  for (uint64_t s = static_cast<uint64_t>(wv::block_id()) * 64u + static_cast<uint64_t>(wv::lane()); s < a.n; s += stride) {
    const uint32_t cnt = a.res_count[s];
    const uint64_t row = s * a.K;
    if (cnt == 0) { a.res_len[row] = 0; a.res_off[row] = 0; continue; }
    const float *sc = a.res_score + row;
    const double alpha = static_cast<double>(a.alpha);
    double mx = -1e300, z = 0.0;
    for (uint32_t k = 0; k < cnt; ++k) { const double w = alpha * sc[k]; mx = w > mx ? w : mx; }
    for (uint32_t k = 0; k < cnt; ++k) z += exp(alpha * sc[k] - mx);
    unsigned long long x = a.seed * 0x9E3779B97F4A7C15ull + (a.index_base + s + 1ull) * 0xD1B54A32D192ED03ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    double u = static_cast<double>(x >> 11) * (1.0 / 9007199254740992.0) * z;
    uint32_t c = cnt - 1u;
    for (uint32_t k = 0; k < cnt; ++k) { u -= exp(alpha * sc[k] - mx); if (u < 0.0) { c = k; break; } }
    if (c != 0u) {
      a.res_off[row] = a.res_off[row + c];
      a.res_len[row] = a.res_len[row + c];
      a.res_score[row] = a.res_score[row + c];
    }
  }
}

}  // namespace spmx
#endif
