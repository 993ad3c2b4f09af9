// The device side of the reference's spm_decode loop (src/spm_decode_main.cc): std::getline over the input, StrSplit(line,
// " ") without empty tokens, atoi per token, Decode, WriteLine.  Two kernels around the batch Decode of kernels_decode.h:
//
//   parser   a file image of id lines                 -> ids[T] (int32) + id_offsets[n_lines + 1]   (parse_ids_block)
//   joiner   packed text + text_offsets[n + 1]        -> a file image, every line followed by '\n'  (join_lines_block)
//
// Lines are std::getline's, as in kernels_split.h.  A token is a maximal run of bytes other than ' ' and '\n'; its FIRST byte
// is the one whose predecessor is ' ', '\n' or the start of the image.  The value is glibc's atoi, (int) strtol(s, 0, 10):
// leading \t \v \f \r, one sign, digits up to the first other byte, saturation at LONG_MAX / LONG_MIN, the low 32 bits.
//
// Parser: two passes over chunks of kSplitChunk bytes around two scans (kernels.h LaunchScan), the shape of split_block:
//   count   newlines and token starts per chunk                       -> nl_counts[chunk], tok_counts[chunk]
//   (scan)  exclusive prefixes                                        -> nl_base[chunk], tok_base[chunk] (64 bit)
//   write   a token start of global rank t                            -> ids[t] = atoi(token)
//           a '\n' of line rank r with t token starts before it       -> id_offsets[r + 1] = t
// The lane that holds a token's first byte computes its value: from its own 16 bytes in registers, and -- only while the
// token is still in its digits at the end of the block -- byte by byte through global memory (never at or past `bytes`).
// HBM-bound: the image read twice, 4 T + 8 n written.
//
// Joiner: organised by 16-byte blocks of the OUTPUT image (aligned on the destination's address): line s occupies the
// output bytes [offsets[s] + s, offsets[s + 1] + s] (the last one is its '\n'), a strictly increasing function of s, so the
// line of an output byte is a binary search -- one per chunk for its first and last line, one per lane within that range.
// A lane builds its 16 bytes in registers (one unaligned 16-byte load where the block lies inside one line) and stores them
// with one aligned 16-byte store.  No lane walks a line, and a flood of empty lines spreads over the grid like any text.
// HBM-bound: text and offsets read once, text + n written.
#ifndef SPMX_KERNELS_IDTEXT_H_
#define SPMX_KERNELS_IDTEXT_H_

namespace spmx {

struct ParseIdsArgs {
  const uint8_t *file;       // 16-byte aligned, the allocation padded to 16 bytes
  uint64_t bytes;
  uint32_t *nl_counts;       // per chunk (count pass out)
  uint32_t *tok_counts;
  const uint64_t *nl_base;   // per chunk + 1 (scan out): newlines before the chunk; [n_chunks] = total
  const uint64_t *tok_base;  // ... token starts before the chunk
  int32_t *ids;              // T
  uint64_t *id_offsets;      // lines + 1
};

// glibc atoi, a byte at a time
struct AtoiState {
  uint32_t phase;            // 0 leading white space, 1 digits (behind the optional sign), 2 done
  uint32_t neg, sat;
  uint64_t acc;
};
SPMX_DEVICE void atoi_step(AtoiState &st, uint32_t c) {
  const uint32_t d = c - 0x30u;
  if (st.phase == 0) {
    if (c == 0x09u || (c >= 0x0Bu && c <= 0x0Du)) return;
    st.phase = 1;
    if (c == 0x2Bu) return;
    if (c == 0x2Du) { st.neg = 1; return; }
  }
  if (st.phase == 1) {
    if (d > 9u) { st.phase = 2; return; }
    // LONG_MAX = 922337203685477580 * 10 + 7, -LONG_MIN = ... + 8
    constexpr uint64_t kCut = 922337203685477580ull;
    if (st.acc > kCut || (st.acc == kCut && d > 7u + st.neg)) st.sat = 1;
    else st.acc = st.acc * 10u + d;
  }
}
SPMX_DEVICE int32_t atoi_value(const AtoiState &st) {
  if (st.sat) return st.neg ? 0 : -1;                       // the low words of LONG_MIN / LONG_MAX
  const uint32_t lo = static_cast<uint32_t>(st.acc);
  return static_cast<int32_t>(st.neg ? 0u - lo : lo);
}

template <bool WRITE>
SPMX_DEVICE void parse_ids_block(const ParseIdsArgs &a) {
  const int lane = wv::lane();
  const uint64_t chunks = (a.bytes + kSplitChunk - 1) / kSplitChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t c0 = ch * kSplitChunk;
    uint64_t nl_run = WRITE ? a.nl_base[ch] : 0;       // newlines / token starts before the current step
    uint64_t tok_run = WRITE ? a.tok_base[ch] : 0;
    uint32_t my_nl = 0, my_tok = 0;                      // count pass: this lane's share of the chunk
    for (uint32_t step = 0; step < kSplitChunk / kSplitStep; ++step) {
      const uint64_t s0 = c0 + step * kSplitStep;
      if (s0 >= a.bytes) break;
      const uint64_t pos = s0 + static_cast<uint64_t>(lane) * 16u;
      Q4 q{0, 0, 0, 0};
      if (pos < a.bytes) q = *reinterpret_cast<const Q4 *>(a.file + pos);   // (the allocation is padded to 16 bytes)
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
      const uint64_t left = pos < a.bytes ? a.bytes - pos : 0;
      const uint32_t vmask = left >= 16 ? 0xFFFFu : (1u << static_cast<uint32_t>(left)) - 1u;
      uint32_t nlm = 0, dm = 0;                          // byte k is '\n' / is a delimiter (' ', '\n', past the end)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        if (c == 0x0Au) nlm |= 1u << k;
        if (c == 0x0Au || c == 0x20u) dm |= 1u << k;
      }
      nlm &= vmask;
      dm |= ~vmask & 0xFFFFu;
      // the byte before this lane's block: the lane below's last one; lane 0 reads it (the start of the image counts as a delimiter)
      uint32_t before0 = 1;
      if (lane == 0 && s0 > 0) { const uint32_t c = a.file[s0 - 1]; before0 = (c == 0x0Au || c == 0x20u) ? 1u : 0u; }
      const uint32_t prev = wv::lane_up1(dm >> 15, before0);
      const uint32_t start = ~dm & ((dm << 1) | prev) & 0xFFFFu;
      const uint32_t n_nl = static_cast<uint32_t>(wv::popc64(nlm)), n_tok = static_cast<uint32_t>(wv::popc64(start));
      if (!WRITE) {
        my_nl += n_nl;
        my_tok += n_tok;
      } else {
        // one scan for both: at most 1024 newlines and 512 token starts in a step
        int both_total = 0;
        const int both = wave_excl_scan(static_cast<int>(n_nl | (n_tok << 16)), lane, &both_total);
        uint64_t r = nl_run + (static_cast<uint32_t>(both) & 0xFFFFu);
        uint64_t t = tok_run + (static_cast<uint32_t>(both) >> 16);
        nl_run += static_cast<uint32_t>(both_total) & 0xFFFFu;
        tok_run += static_cast<uint32_t>(both_total) >> 16;
        if ((nlm | start) != 0) {
          bool open = false;                             // a token that started in this block is being read
          uint64_t open_rank = 0;
          AtoiState st{0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint32_t bit = 1u << k;
            if (dm & bit) {
              if (open) { a.ids[open_rank] = atoi_value(st); open = false; }
              if (nlm & bit) { a.id_offsets[r + 1] = t; ++r; }
            } else {
              if (start & bit) { open = true; open_rank = t++; st = AtoiState{0, 0, 0, 0}; }
              if (open) atoi_step(st, (w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
            }
          }
          if (open) {
            // the token goes on behind the block: only digits (or leading white space) still change its value
            for (uint64_t p = pos + 16; st.phase != 2 && p < a.bytes; ++p) {
              const uint32_t c = a.file[p];
              if (c == 0x0Au || c == 0x20u) break;
              atoi_step(st, c);
            }
            a.ids[open_rank] = atoi_value(st);
          }
        }
      }
    }
    if (!WRITE) {
      int both_total = 0;                                // at most 16384 newlines and 8192 token starts in a chunk
      wave_excl_scan(static_cast<int>(my_tok), lane, &both_total);
      const int tok_total = both_total;
      wave_excl_scan(static_cast<int>(my_nl), lane, &both_total);
      if (lane == 0) { a.nl_counts[ch] = static_cast<uint32_t>(both_total); a.tok_counts[ch] = static_cast<uint32_t>(tok_total); }
    }
  }
  if (WRITE && wv::block_id() == 0 && lane == 0) {
    const uint64_t nl = a.nl_base[chunks];
    a.id_offsets[0] = 0;
    // a last line without its '\n' (std::getline returns it) closes with every token
    if (a.bytes > 0 && a.file[a.bytes - 1] != 0x0Au) a.id_offsets[nl + 1] = a.tok_base[chunks];
  }
}

// ------------------------------------------------------------------------------------------------------- joiner --
constexpr uint32_t kJoinChunk = 16384;    // output bytes per chunk: 64 lanes x 16 bytes x 16 steps

struct JoinLinesArgs {
  const uint8_t *text;          // text_offsets[n] bytes
  const uint64_t *offsets;      // n + 1
  uint64_t n;
  uint8_t *out;                 // out_bytes = offsets[n] + n
  uint64_t out_bytes;
};

// The line of output byte o: the largest s in [lo, hi] with offsets[s] + s <= o (lo qualifies)
SPMX_DEVICE uint64_t join_line_of(const uint64_t *offsets, uint64_t lo, uint64_t hi, uint64_t o) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] + mid <= o) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

SPMX_DEVICE void join_lines_block(const JoinLinesArgs &a) {
  if (a.n == 0 || a.out_bytes == 0) return;
  const int lane = wv::lane();
  // blocks are aligned on the destination ADDRESS: block b holds the output bytes [16 b - mis, 16 b - mis + 16)
  const uint64_t mis = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(a.out) & 15u);
  const uint64_t span = a.out_bytes + mis;
  const uint64_t chunks = (span + kJoinChunk - 1) / kJoinChunk;
  for (uint64_t ch = static_cast<uint64_t>(wv::block_id()); ch < chunks; ch += static_cast<uint64_t>(wv::grid_size())) {
    const uint64_t c0 = ch * kJoinChunk;
    const uint64_t c1 = c0 + kJoinChunk < span ? c0 + kJoinChunk : span;
    // the lines of the chunk's first and last byte (the same in every lane)
    const uint64_t first_o = c0 > mis ? c0 - mis : 0;
    const uint64_t lo = join_line_of(a.offsets, 0, a.n - 1, first_o);
    const uint64_t hi = join_line_of(a.offsets, lo, a.n - 1, c1 - mis - 1);
    for (uint32_t step = 0; step < kJoinChunk / 1024u; ++step) {
      const uint64_t b0 = c0 + step * 1024u + static_cast<uint64_t>(lane) * 16u;   // in address units: output byte b0 - mis
      if (b0 >= c1) break;
      const uint64_t o0 = b0 > mis ? b0 - mis : 0;
      const uint64_t o1 = b0 + 16 - mis < a.out_bytes ? b0 + 16 - mis : a.out_bytes;
      uint64_t s = join_line_of(a.offsets, lo, hi, o0);
      uint64_t end = a.offsets[s + 1] + s;             // where line s's '\n' goes
      if (o1 - o0 == 16 && o1 <= end) {                // a whole block inside one line
        const PackedU4 v = packed_load16(a.text + (o0 - s));
        *reinterpret_cast<Q4 *>(a.out + o0) = Q4{v.x, v.y, v.z, v.w};
        continue;
      }
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint64_t o = o0 + static_cast<uint64_t>(k);
        if (o < o1) {
          uint32_t c = 0x0Au;
          if (o == end) { ++s; if (s < a.n) end = a.offsets[s + 1] + s; }
          else c = a.text[o - s];
          w[k >> 2] |= c << (8 * (k & 3));
        }
      }
      if (o1 - o0 == 16) {
        *reinterpret_cast<Q4 *>(a.out + o0) = Q4{w[0], w[1], w[2], w[3]};
      } else {                                          // the image's first or last block
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (o0 + static_cast<uint64_t>(k) < o1) a.out[o0 + static_cast<uint64_t>(k)] = static_cast<uint8_t>(w[k >> 2] >> (8 * (k & 3)));
      }
    }
  }
}

}  // namespace spmx
#endif
