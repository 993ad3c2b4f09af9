// The device side of the reference's spm_encode output loop (src/spm_encode_main.cc:110-119): an encoded batch -> token
// text.  The inverse of kernels_idtext.h.  A token's text is either its decimal id (--output_format=id) or its piece
// (--output_format=piece, the default); the output is either a file image of lines -- absl::StrJoin(tokens, " ") + '\n' per
// sentence, an empty sentence a single '\n' -- or, for pieces, the bytes back to back with piece_offsets[T + 1] (the
// EncodeAsPieces form).
//
// A piece's bytes follow PopulateSentencePieceText / ApplyExtraOptions (src/sentencepiece_processor.cc:566-620, :1029-1058):
// the name of a byte-fallback or control piece, trainer_spec.unk_piece for an unknown token under the `unk` / `unk_piece`
// extra option, otherwise normalized[nbegin, nend) of the token's own sentence (an unknown token shows its characters).
// The names come from tables.cc (HostTables::nm_*): per id a kind word and an offset, entry V is unk_piece.
//
// The output is a sequence of ITEMS.  Packed form: item i is token i.  Lines form: the tokens of sentence s followed by one
// line-end item, so token t of sentence s is item t + s and the line end of s is item id_offs[s + 1] + s; a token item
// holds its text and the byte behind it (' ', or '\n' for the sentence's last token), a line-end item the '\n' of an
// empty sentence and nothing otherwise.  Three launches, the shape of the parser:
//   length  a lane per item (1024 items per chunk, the sentence by binary search over id_offs[s] + s within the chunk's
//           range)                                                        -> len[item] (bytes), rec[item] (where they come from)
//   (scan)  exclusive prefix, kernels.h LaunchScan                        -> start[items + 1]: the exact size, the piece offsets
//   write   by 16-byte blocks of the OUTPUT, aligned on the destination's address, as the joiner: the block's first item
//           by binary search over start[], then every item that reaches into the block is shifted into a 128-bit
//           register pair -- one unaligned 16-byte load per piece, the digits of an id computed in registers -- and the
//           block leaves with one aligned 16-byte store.
// No lane walks a sentence: a one-line document and a flood of empty lines spread over the grid like any other batch.
// The 16-byte loads may reach up to 15 bytes behind a piece: `norm` and the name bytes carry 16 bytes of slack.
// HBM-bound.  Per token of L bytes, lines form of pieces: length pass 12 read (id, nbegin, nend) + 12 written, scan 4 + 8,
// write pass 16 read (start, rec) + L read + L + 1 written: 52 + 2 L + 1.  Ids: 4 + 12, 4 + 8, 16 + L + 1: 44 + L + 1.
#ifndef SPMX_KERNELS_TOKENTEXT_H_
#define SPMX_KERNELS_TOKENTEXT_H_

namespace spmx {

constexpr uint32_t kTtItemChunk = 1024;      // items per chunk of the length pass: 64 lanes x 16 steps
constexpr uint32_t kTtOutChunk = 16384;      // output bytes per chunk of the write pass: 64 lanes x 16 bytes x 16 steps

// rec word per item: the low bits hold the id (ids) or the byte offset of the text in `norm` / the name bytes (pieces)
constexpr uint64_t kTrName = 1ull << 63;     // the text is in the name bytes
constexpr uint64_t kTrLast = 1ull << 62;     // '\n' follows, not ' '
constexpr uint64_t kTrEnd = 1ull << 61;      // a line-end item: no token, only the '\n' of an empty sentence
constexpr uint64_t kTrOffMask = (1ull << 56) - 1;
// kind of an id (the low bits of nm_info; the length of the name from bit 8)
constexpr uint32_t kNkText = 0u;             // normalized[nbegin, nend)
constexpr uint32_t kNkName = 1u;             // byte-fallback and control pieces: IdToPiece
constexpr uint32_t kNkUnknown = 2u;          // the unknown piece: its characters, or entry V under the unk option

struct TokenTextArgs {
  const int32_t *ids;           // T
  const uint64_t *id_offs;      // n + 1
  uint64_t n;
  uint64_t items;               // lines form: T + n; packed form: T
  // pieces only
  const uint32_t *nbegin, *nend;    // T: the token's range of its normalized sentence
  const uint8_t *norm;              // norm_offs[n] bytes + 16 of slack
  const uint64_t *norm_offs;        // n + 1
  const uint32_t *nm_info;          // V + 1
  const uint32_t *nm_off;           // V + 1
  const uint8_t *nm_bytes;          // + 16 of slack
  uint32_t vocab;                   // V
  uint32_t unk_name;                // the unk / unk_piece extra option is set
  // between the passes
  uint32_t *len;                // items (length pass out)
  uint64_t *rec;                // items (length pass out)
  const uint64_t *start;        // items + 1 (scan out)
  uint8_t *out;                 // start[items] bytes
  uint64_t out_bytes;
};

// The sentence of item i: the largest s in [lo, hi] with id_offs[s] + s * LINES <= i (lo qualifies)
template <bool LINES>
SPMX_DEVICE uint64_t tt_sentence_of(const uint64_t *id_offs, uint64_t lo, uint64_t hi, uint64_t i) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (id_offs[mid] + (LINES ? mid : 0) <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

SPMX_DEVICE uint32_t tt_digits(uint32_t v) {
  uint32_t d = 1;
  if (v >= 10u) d = 2;
  if (v >= 100u) d = 3;
  if (v >= 1000u) d = 4;
  if (v >= 10000u) d = 5;
  if (v >= 100000u) d = 6;
  if (v >= 1000000u) d = 7;
  if (v >= 10000000u) d = 8;
  if (v >= 100000000u) d = 9;
  if (v >= 1000000000u) d = 10;
  return d;
}

// FMT 0: decimal ids (always lines), 1: pieces
template <int FMT, bool LINES>
SPMX_DEVICE void token_len_block(const TokenTextArgs &a) {
  if (a.items == 0 || a.n == 0) return;
  const int lane = wv::lane();
  const uint64_t chunks = (a.items + kTtItemChunk - 1) / kTtItemChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t i0 = ch * kTtItemChunk;
    const uint64_t i1 = i0 + kTtItemChunk < a.items ? i0 + kTtItemChunk : a.items;
    // the sentences of the chunk's first and last item (the same in every lane)
    const uint64_t lo = tt_sentence_of<LINES>(a.id_offs, 0, a.n - 1, i0);
    const uint64_t hi = tt_sentence_of<LINES>(a.id_offs, lo, a.n - 1, i1 - 1);
    for (uint32_t step = 0; step < kTtItemChunk / 64u; ++step) {
      const uint64_t i = i0 + step * 64u + static_cast<uint64_t>(lane);
      if (i >= i1) break;
      const uint64_t s = tt_sentence_of<LINES>(a.id_offs, lo, hi, i);
      const uint64_t t_end = a.id_offs[s + 1];
      if (LINES && i == t_end + s) {                   // the line-end item: the '\n' of a sentence without tokens
        a.len[i] = a.id_offs[s] == t_end ? 1u : 0u;
        a.rec[i] = kTrLast | kTrEnd;
        continue;
      }
      const uint64_t t = LINES ? i - s : i;
      const uint64_t last = LINES && t + 1 == t_end ? kTrLast : 0;
      const int32_t id = a.ids[t];
      if (FMT == 0) {
        const uint32_t neg = id < 0 ? 1u : 0u;
        const uint32_t mag = neg ? 0u - static_cast<uint32_t>(id) : static_cast<uint32_t>(id);
        a.len[i] = tt_digits(mag) + neg + 1u;
        a.rec[i] = static_cast<uint64_t>(static_cast<uint32_t>(id)) | last;
      } else {
        const uint32_t info = static_cast<uint32_t>(id) < a.vocab ? a.nm_info[id] : 0u;
        const uint32_t kind = info & 3u;
        uint32_t body;
        uint64_t rec;
        if (kind == kNkName || (kind == kNkUnknown && a.unk_name)) {
          const uint32_t e = kind == kNkName ? static_cast<uint32_t>(id) : a.vocab;
          body = a.nm_info[e] >> 8;
          rec = kTrName | a.nm_off[e];
        } else {
          const uint32_t b = a.nbegin[t], e = a.nend[t];
          body = e > b ? e - b : 0u;
          rec = a.norm_offs[s] + b;
        }
        a.len[i] = body + (LINES ? 1u : 0u);
        a.rec[i] = rec | last;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------ write pass --
// 16 bytes in two registers; byte k is bits [8 k, 8 k + 8) of lo (k < 8) or hi
struct B16 { uint64_t lo, hi; };
SPMX_DEVICE B16 b16_shl(B16 v, uint32_t bytes) {        // towards higher bytes; bytes < 16
  const uint32_t sh = 8u * bytes;
  if (sh == 0) return v;
  if (sh < 64u) return B16{v.lo << sh, (v.hi << sh) | (v.lo >> (64u - sh))};
  return B16{0, v.lo << (sh - 64u)};
}
SPMX_DEVICE B16 b16_shr(B16 v, uint32_t bytes) {        // bytes < 16
  const uint32_t sh = 8u * bytes;
  if (sh == 0) return v;
  if (sh < 64u) return B16{(v.lo >> sh) | (v.hi << (64u - sh)), v.hi >> sh};
  return B16{v.hi >> (sh - 64u), 0};
}
SPMX_DEVICE B16 b16_low(B16 v, uint32_t bytes) {        // the low `bytes` bytes; bytes <= 16
  if (bytes >= 16u) return v;
  if (bytes >= 8u) return B16{v.lo, bytes == 8u ? 0 : v.hi & ((1ull << (8u * (bytes - 8u))) - 1u)};
  return B16{bytes == 0 ? 0 : v.lo & ((1ull << (8u * bytes)) - 1u), 0};
}
SPMX_DEVICE B16 b16_put(B16 v, uint32_t at, uint32_t c) {   // ORs byte c in at position `at` < 16
  if (at < 8u) v.lo |= static_cast<uint64_t>(c) << (8u * at);
  else v.hi |= static_cast<uint64_t>(c) << (8u * (at - 8u));
  return v;
}

// The bytes of an item of `ilen` bytes from its byte `from` < ilen on (what lies behind the item's end is not defined)
template <int FMT, bool LINES>
SPMX_DEVICE B16 tt_item_bytes(const TokenTextArgs &a, uint64_t rec, uint32_t ilen, uint32_t from) {
  const uint32_t sep = (rec & kTrLast) ? 0x0Au : 0x20u;
  const uint32_t body = ilen - (LINES ? 1u : 0u);
  if (rec & kTrEnd) return B16{sep, 0};
  if (FMT == 0) {
    const int32_t id = static_cast<int32_t>(static_cast<uint32_t>(rec));
    uint32_t mag = id < 0 ? 0u - static_cast<uint32_t>(id) : static_cast<uint32_t>(id);
    B16 s = b16_put(B16{0, 0}, body, sep);              // (body <= 11)
    uint32_t p = body;
    do {
      --p;
      s = b16_put(s, p, 0x30u + mag % 10u);
      mag /= 10u;
    } while (mag != 0 && p != 0);
    if (id < 0) s = b16_put(s, 0, 0x2Du);
    return b16_shr(s, from);
  }
  B16 s{0, 0};
  if (from < body) {
    const uint8_t *src = ((rec & kTrName) ? a.nm_bytes : a.norm) + (rec & kTrOffMask) + from;
    const PackedU4 v = packed_load16(src);
    s = B16{static_cast<uint64_t>(v.x) | static_cast<uint64_t>(v.y) << 32, static_cast<uint64_t>(v.z) | static_cast<uint64_t>(v.w) << 32};
  }
  if (LINES) {
    const uint32_t rel = body - from;                   // where the separator falls
    if (rel < 16u) s = b16_put(b16_low(s, rel), rel, sep);
  }
  return s;
}

// The item of output byte o: the largest i in [lo, hi] with start[i] <= o (lo qualifies); it is not empty where o < start[hi + 1]
SPMX_DEVICE uint64_t tt_item_of(const uint64_t *start, uint64_t lo, uint64_t hi, uint64_t o) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (start[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <int FMT, bool LINES>
SPMX_DEVICE void token_write_block(const TokenTextArgs &a) {
  if (a.items == 0 || a.out_bytes == 0) return;
  const int lane = wv::lane();
  // blocks are aligned on the destination ADDRESS: block b holds the output bytes [16 b - mis, 16 b - mis + 16)
  const uint64_t mis = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(a.out) & 15u);
  const uint64_t span = a.out_bytes + mis;
  const uint64_t chunks = (span + kTtOutChunk - 1) / kTtOutChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t c0 = ch * kTtOutChunk;
    const uint64_t c1 = c0 + kTtOutChunk < span ? c0 + kTtOutChunk : span;
    // the items of the chunk's first and last byte (the same in every lane)
    const uint64_t lo = tt_item_of(a.start, 0, a.items - 1, c0 > mis ? c0 - mis : 0);
    const uint64_t hi = tt_item_of(a.start, lo, a.items - 1, c1 - mis - 1);
    for (uint32_t step = 0; step < kTtOutChunk / 1024u; ++step) {
      const uint64_t b0 = c0 + step * 1024u + static_cast<uint64_t>(lane) * 16u;   // in address units: output byte b0 - mis
      if (b0 >= c1) break;
      const uint64_t o0 = b0 > mis ? b0 - mis : 0;
      const uint64_t o1 = b0 + 16 - mis < a.out_bytes ? b0 + 16 - mis : a.out_bytes;
      uint64_t i = tt_item_of(a.start, lo, hi, o0);
      uint64_t st = a.start[i];
      uint64_t o = o0;
      B16 acc{0, 0};
      while (o < o1 && i < a.items) {
        const uint64_t en = a.start[i + 1];
        if (en > o) {
          const uint64_t stop = en < o1 ? en : o1;
          const uint32_t cnt = static_cast<uint32_t>(stop - o);
          const B16 s = b16_low(tt_item_bytes<FMT, LINES>(a, a.rec[i], static_cast<uint32_t>(en - st), static_cast<uint32_t>(o - st)), cnt);
          const B16 placed = b16_shl(s, static_cast<uint32_t>(o - o0));
          acc.lo |= placed.lo;
          acc.hi |= placed.hi;
          o = stop;
        }
        st = en;
        ++i;
      }
      if (o1 - o0 == 16) {
        *reinterpret_cast<Q4 *>(a.out + o0) = Q4{static_cast<uint32_t>(acc.lo), static_cast<uint32_t>(acc.lo >> 32),
                                                 static_cast<uint32_t>(acc.hi), static_cast<uint32_t>(acc.hi >> 32)};
      } else {                                          // the image's first or last block
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (o0 + static_cast<uint64_t>(k) < o1)
            a.out[o0 + static_cast<uint64_t>(k)] = static_cast<uint8_t>((k < 8 ? acc.lo : acc.hi) >> (8 * (k & 7)));
      }
    }
  }
}

}  // namespace spmx
#endif
