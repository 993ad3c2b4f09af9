// Character and word models (model_type CHAR / WORD), streaming form: one SENTENCE PER LANE inside the persistent
// streaming launch (kernels_stream.h encode_stream_block), beside unigram_stream_lane and bpe_stream_lane.
// Reference: character::Model::Encode (src/char_model.cc:28-43), word::Model::Encode (src/word_model.cc:28-39),
// SplitIntoWords and PieceToId (src/model_interface.cc), PopulateSentencePieceText (src/sentencepiece_processor.cc:547-636).
//
// Both models CUT the normalized text in text order and look every cut up with PieceToId:
//   char   the longest USER_DEFINED piece that starts at the position (PrefixMatcher::PrefixMatch), else one character;
//   word   a cut starts at byte 0 and at every space symbol (SplitIntoWords with both flags false, whatever the
//          trainer_spec says); the user-defined matcher is not consulted.
// PieceToId is one exact-match walk of the piece trie (tables.cc: pieces map, then reserved map; dev.h ptrie units,
// y = id | kPtUserDefined, or kPtControlCut), a byte at a time.  A walk dies at the first byte no piece continues -- the child-label
// summary in the unit usually proves that without a probe -- and the cut is unk_id from there on: an out-of-vocabulary
// word of any length costs as many probes as its known prefix.
//
// No scores, no recurrence, no backtrack: nothing is kept per position.  A lane holds two dwords of its text column
// in registers (the bytes at its position and the next four), the unit of its walk, and four ids on their way out;
// its only LDS is the workgroup's shared first trie level (StreamLds::roottab -- a one-byte character is cut and looked
// up without touching memory at all; a two- or three-byte character of a model without USER_DEFINED pieces by ONE load from
// the direct table, dev.h cfirst).  Ids leave FORWARD, in text order, as aligned 16-byte stores of four; the
// unknown-run merge / byte fallback of sentencepiece_processor.cc:581-613 is applied as the cuts come.
#ifndef SPMX_KERNELS_CHARWORD_H_
#define SPMX_KERNELS_CHARWORD_H_

namespace spmx {

// A lane's read position in its text column: bytes [pos, pos + 4) in one register whatever pos is.
struct CwText {
  const TextCol &gt;
  uint32_t cur = 0, nxt = 0;    // dwords k and k + 1 of the column, k = pos >> 2
  int k = -2;                   // (no dword yet)
  SPMX_DEVICE explicit CwText(const TextCol &g) : gt(g) {}
  SPMX_DEVICE void seek(int pos) {
    const int want = pos >> 2;
    if (want == k) return;
    if (want == k + 1) { cur = nxt; nxt = gt.dw(want + 1); }
    else { cur = gt.dw(want); nxt = gt.dw(want + 1); }
    k = want;
  }
  SPMX_DEVICE uint32_t peek4(int pos) {
    seek(pos);
    const uint32_t sh = 8u * (static_cast<uint32_t>(pos) & 3u);
    return sh ? (cur >> sh) | (nxt << (32u - sh)) : cur;
  }
};

// The ids of a lane's sentence on their way into its arena slot (and, spans form, every piece's begin into tslot).
// Forward order fills slot[0, cap) from its START, `reverse` from its end; the caller aligns the end that is filled
// first to 16 bytes (encode_stream_block), so four ids leave as one store.
struct CwOut {
  const SpmxDev &d;
  const TextCol &gt;
  int32_t *slot, *tslot;
  int cap;
  bool bf, reverse;
  uint32_t spb;
  int n = 0;
  bool right_unk = false, ok = true;
  uint32_t q0 = 0, q1 = 0, q2 = 0;
  SPMX_DEVICE CwOut(const SpmxDev &dev, const TextCol &g, int32_t *s, int32_t *ts, int c)
      : d(dev), gt(g), slot(s), tslot(ts), cap(c), bf((dev.flags & kNfByteFallback) != 0),
        reverse((dev.flags & kNfReverse) != 0), spb(SpByteOf(dev)) {}
  SPMX_DEVICE void put(uint32_t id, int off) {
    if (n >= cap) { ok = false; return; }
    if (tslot) {                                    // the spans form keeps the simple path
      slot[reverse ? cap - 1 - n : n] = static_cast<int32_t>(id);
      tslot[reverse ? cap - 1 - n : n] = off;
      ++n;
      return;
    }
    const int r = n & 3;
    if (r == 0) q0 = id; else if (r == 1) q1 = id; else if (r == 2) q2 = id;
    ++n;
    if (r == 3) {
      if (reverse) *reinterpret_cast<Q4 *>(slot + (cap - n)) = Q4{id, q2, q1, q0};
      else *reinterpret_cast<Q4 *>(slot + (n - 4)) = Q4{q0, q1, q2, id};
    }
  }
  // one cut of the text, [off, off + len), with PieceToId's answer
  SPMX_DEVICE void piece(uint32_t id, int off, int len) {
    if (id == kPtControlCut) {                      // a CONTROL piece's string: the reference fails the sentence (:561-567, :628)
      ok = false;
    } else if (static_cast<int32_t>(id) == d.unk_id) {
      if (bf) {                                     // one BYTE id per byte of the unknown piece (:581-603)
        for (int x = 0; x < len && ok; ++x) {
          const uint32_t b = col_byte(gt, off + x);
          if (b == spb) { put(static_cast<uint32_t>(d.byte_ids[0xE2]), off); put(static_cast<uint32_t>(d.byte_ids[0x96]), off); put(static_cast<uint32_t>(d.byte_ids[0x81]), off); }
          else put(static_cast<uint32_t>(d.byte_ids[b]), off);
        }
      } else if (!right_unk) {                      // a run of unknown pieces yields one id (:609-613)
        put(id, off);
      }
      right_unk = true;
    } else {
      put(id, off);
      right_unk = false;
    }
  }
  SPMX_DEVICE int finish() {                        // the last, incomplete group
    if (!ok) return -1;
    if (!tslot) {
      const int r = n & 3, g = n & ~3;
      for (int x = 0; x < r; ++x) {
        const uint32_t id = x == 0 ? q0 : (x == 1 ? q1 : q2);
        slot[reverse ? cap - 1 - (g + x) : g + x] = static_cast<int32_t>(id);
      }
    }
    return n;
  }
};

// word::Model::Encode of this lane's sentence (text column gt, nlen bytes): ids into slot[0, cap).  Returns their
// number, -1 when the reference fails the sentence (a word that is a CONTROL piece's string).  One text byte per iteration while the walk of the current word is alive (one
// probe in flight: it is issued at the end of an iteration and judged at the top of the next); a word whose walk has
// died is skipped four bytes at a time.
SPMX_DEVICE int word_stream_lane(const SpmxDev &d, const TextCol &gt, int nlen, int32_t *slot, int32_t *tslot, int cap,
                                 const U4 *roottab, bool active_in) {
  const bool one = (d.flags & kNfCompressSp) != 0;
  const U4 *__restrict__ ptrie = d.ptrie;
  bool active = active_in && nlen > 0;
  if (!active) nlen = 0;
  CwOut out(d, gt, slot, tslot, cap);
  CwText tx(gt);
  int pos = 0, pstart = 0;
  bool alive = true, probing = false;
  uint32_t pc = 0;
  U4 u{0, 0, 0, 0};
  while (wv::any(active)) {
    if (!active) continue;
    if (probing) { alive = (u.x & 0x1FFu) == (0x100u | pc); probing = false; }
    const bool at_end = pos >= nlen;
    uint32_t w4 = 0;
    bool sp = false;
    if (!at_end) {
      w4 = tx.peek4(pos);
      sp = one ? (w4 & 0xFFu) == kSpByte : ((w4 & 0xFFFFFFu) == 0x8196E2u && pos + 3 <= nlen);
    }
    if (at_end || (sp && pos > pstart)) {           // the word [pstart, pos) is complete
      const uint32_t id = alive && (u.x & kDatTerminalDev) ? (u.y & kPtIdMask) : static_cast<uint32_t>(d.unk_id);
      out.piece(id, pstart, pos - pstart);
      pstart = pos;
      alive = true;
      if (at_end || !out.ok) { active = false; continue; }
    }
    const uint32_t c = w4 & 0xFFu;
    if (pos == pstart) {                            // first byte: the shared first level
      u = roottab[c];
      alive = (u.x & 0x100u) != 0u;
      ++pos;
    } else if (alive) {
      if ((u.w >> ChildBit(c)) & 1u) { u = ptrie[(u.x >> kDatBaseShiftDev) ^ c]; pc = c; probing = true; }
      else alive = false;
      ++pos;
    } else {                                        // out of vocabulary: on to the next space symbol
      int step = 1;
      if (one) {
        const uint32_t m = sp_mask4(w4);
        step = m ? wv::ffs64(static_cast<uint64_t>(m)) - 1 : 4;
      }
      if (step > nlen - pos) step = nlen - pos;
      pos += step;                                  // (step 0: the byte at pos is a space symbol; the next iteration cuts)
    }
  }
  return out.finish();
}

// character::Model::Encode of this lane's sentence.  UDS: the model has USER_DEFINED pieces (the walk then goes on
// past the character for the longest of them; without, a cut is one character and up to four one-byte characters are
// cut per iteration from the LDS table alone).
template <bool UDS>
SPMX_DEVICE int char_stream_lane(const SpmxDev &d, const TextCol &gt, int nlen, int32_t *slot, int32_t *tslot, int cap,
                                 const U4 *roottab, bool active_in) {
  const U4 *__restrict__ ptrie = d.ptrie;
  const uint32_t unk = static_cast<uint32_t>(d.unk_id);
  const U4 *__restrict__ cfirst = UDS ? nullptr : d.cfirst;
  bool active = active_in && nlen > 0;
  if (!active) nlen = 0;
  CwOut out(d, gt, slot, tslot, cap);
  CwText tx(gt);
  int pos = 0, pstart = 0, mb = 1;
  int best_len = 0;
  uint32_t best_id = 0, char_id = unk;
  bool alive = false, probing = false;
  uint32_t pc = 0;
  U4 u{0, 0, 0, 0};
  while (wv::any(active)) {
    if (!active) continue;
    if (probing) { alive = (u.x & 0x1FFu) == (0x100u | pc); probing = false; }
    if (pos > pstart) {
      // what the walk has reached after the bytes [pstart, pos)
      const int dep = pos - pstart;
      const bool term = alive && (u.x & kDatTerminalDev);
      if (dep == mb) char_id = term ? (u.y & kPtIdMask) : unk;
      if (UDS && term && (u.y & kPtUserDefined)) { best_len = dep; best_id = u.y & kPtIdMask; }
      const bool more = alive && pos < nlen && (UDS || dep < mb);
      bool go = false;
      uint32_t c = 0;
      if (more) {
        c = tx.peek4(pos) & 0xFFu;
        go = ((u.w >> ChildBit(c)) & 1u) != 0u;
      }
      if (go) {
        u = ptrie[(u.x >> kDatBaseShiftDev) ^ c]; pc = c; probing = true;
        ++pos;
        continue;
      }
      // the cut is decided (a walk that died inside the character leaves char_id = unk)
      if (UDS && best_len > 0) { out.piece(best_id, pstart, best_len); pstart += best_len; }
      else { out.piece(dep >= mb ? char_id : unk, pstart, mb); pstart += mb; }
      pos = pstart;
      best_len = 0;
      char_id = unk;
      if (pos >= nlen || !out.ok) { active = false; continue; }
    }
    // a cut begins at pos == pstart
    uint32_t w4 = tx.peek4(pos);
    if (!UDS) {
      // one-byte characters straight from the first-level table
      int k = 0;
#pragma unroll
      for (; k < 4; ++k) {
        const U4 r = roottab[w4 & 0xFFu];
        if ((r.x & 7u) != 1u || pos >= nlen || !out.ok) break;
        out.piece((r.x & 0x100u) && (r.x & kDatTerminalDev) ? (r.y & kPtIdMask) : unk, pos, 1);
        ++pos;
        w4 >>= 8;
      }
      pstart = pos;
      if (pos >= nlen || !out.ok) { active = false; continue; }
      if (k == 4) continue;                         // (the register ran dry: the next iteration reads on)
      // a two- or three-byte character through the direct table (dev.h cfirst; tables.cc BuildFirstCharTable): the unit the
      // trie reaches behind the character's bytes, by code point -- one load, no chain
      const uint32_t c0 = w4 & 0xFFu;
      if (cfirst != nullptr && c0 >= 0xC2u && c0 < 0xF0u) {
        const uint32_t b1 = (w4 >> 8) & 0xFFu, b2 = (w4 >> 16) & 0xFFu;
        const bool three = c0 >= 0xE0u;
        const uint32_t cp = three ? ((c0 & 0x0Fu) << 12) | ((b1 & 0x3Fu) << 6) | (b2 & 0x3Fu) : ((c0 & 0x1Fu) << 6) | (b1 & 0x3Fu);
        const bool wf = (b1 & 0xC0u) == 0x80u && (!three || ((b2 & 0xC0u) == 0x80u && cp >= 0x800u));   // the canonical bytes of cp
        const int dch = three ? 3 : 2;
        if (wf && pos + dch <= nlen) {
          const U4 r = cfirst[cp];
          out.piece((r.x & 0x100u) && (r.x & kDatTerminalDev) ? (r.y & kPtIdMask) : unk, pos, dch);
          pos += dch;
          pstart = pos;
          if (pos >= nlen || !out.ok) active = false;
          continue;
        }
      }
    }
    u = roottab[w4 & 0xFFu];
    mb = static_cast<int>(u.x & 7u);
    if (mb > nlen - pos) mb = nlen - pos;
    alive = (u.x & 0x100u) != 0u;
    ++pos;
  }
  return out.finish();
}

}  // namespace spmx
#endif
