// Character and word models, wave-cooperative form: one SENTENCE PER WAVEFRONT, one CUT PER LANE -- for the sentences the
// lane-per-sentence form (kernels_charword.h) is the wrong tool for: documents (a lane would walk them alone) and what
// fits no text column of its launch.  Word models and character models without USER_DEFINED pieces (with them a cut's
// start depends on the cut before it: those keep the lane form).
//
// The normalized text comes from the position-parallel normalizer into a slice of the long form's pool, exactly as in
// kernels_uniwave.h (uni_long_block).  Then, in ROUNDS of up to 64 cuts:
//   starts   64 bytes a sweep, a lane per byte: a cut starts at byte 0 and at every character lead (char) / every space
//            symbol (word); the ballot's set bits go, in order, to a queue of start positions in LDS.  A cut is taken
//            once the NEXT start is in the queue (its end) -- so a word longer than a sweep, or than many, simply waits
//            at the queue's head while the sweeps go on, and the last cut ends at the end of the text;
//   walk     lane k walks PieceToId's trie (tables.cc) over the bytes of cut k, one probe per lane per iteration;
//   place    a cut's id count -- 1; 0 for an unknown cut behind an unknown cut (the run is one id; the neighbour is lane
//            k - 1, or the previous round's last cut, carried); its bytes' count under byte fallback -- goes through a
//            wave prefix sum.
// Two passes over the rounds: the first walks, keeps every cut's id at its start position in the slice and adds the
// counts up; then the sentence's ids are allocated in the arena in one piece (`reverse` needs the total) and the second
// pass places them (and, spans form, every id's token begin).
#ifndef SPMX_KERNELS_CHARWAVE_H_
#define SPMX_KERNELS_CHARWAVE_H_

namespace spmx {

constexpr uint32_t kCwQueue = 136;                      // start positions: fewer than 65 when a sweep begins, at most 64 more behind it
constexpr uint32_t kCwWaveLdsBytes = kCwQueue * 4u + ((kRawWinBytes + 15u) & ~15u);

// Calls body(s, e, have) for the cuts [s, e) of norm[0, nlen) in text order, up to 64 per call (lane k: cut k of the round;
// have: this lane has one).  body is wave-uniform code (it may use collectives).  WORD: a word model's cuts, else characters.
template <bool WORD, typename Body>
SPMX_DEVICE void cw_for_each_round(const SpmxDev &d, const uint8_t *norm, int nlen, uint32_t *q, int lane, Body body) {
  const bool one = (d.flags & kNfCompressSp) != 0;
  int base = 0, qn = 0;
  for (;;) {
    while (qn < 65 && base < nlen) {                    // (wave-uniform: qn and base are)
      const int p = base + lane;
      bool st = false;
      if (p < nlen) {
        const uint32_t b0 = norm[p];
        if (WORD) st = p == 0 || (one ? b0 == kSpByte : (b0 == 0xE2u && p + 3 <= nlen && norm[p + 1] == 0x96u && norm[p + 2] == 0x81u));
        else st = p == 0 || (b0 & 0xC0u) != 0x80u;
      }
      const uint64_t m = wv::ballot(st);
      if (st) q[qn + wv::popc64(m & ((1ull << lane) - 1ull))] = static_cast<uint32_t>(p);
      qn += wv::popc64(m);
      base += 64;
      wv::sync();
    }
    const bool last = base >= nlen;
    if (last) { if (lane == 0) q[qn] = static_cast<uint32_t>(nlen); wv::sync(); }
    int r = last ? qn : qn - 1;                         // cuts whose end is known
    if (r > 64) r = 64;
    if (r > 0) {
      const bool have = lane < r;
      const int s = have ? static_cast<int>(q[lane]) : 0, e = have ? static_cast<int>(q[lane + 1]) : 0;
      // the queue moves up by r (read, then written)
      uint32_t mv[3];
      const int left = qn - r + (last ? 1 : 0);
      for (int k = 0; k < 3; ++k) mv[k] = lane + 64 * k < left ? q[r + lane + 64 * k] : 0u;
      wv::sync();
      for (int k = 0; k < 3; ++k) if (lane + 64 * k < left) q[lane + 64 * k] = mv[k];
      wv::sync();
      qn -= r;
      body(s, e, have);
    }
    if (last && qn == 0) break;
  }
}

// PieceToId of the cut norm[s, e) by this lane (all lanes together: one probe each per iteration)
SPMX_DEVICE uint32_t cw_walk(const SpmxDev &d, const uint8_t *norm, int s, int e, bool have) {
  const U4 *__restrict__ ptrie = d.ptrie;
  const uint32_t root = ptrie[0].x >> kDatBaseShiftDev;
  U4 u{0, 0, 0, 0};
  int dep = 0;
  const int len = e - s;
  bool alive = have;
  while (wv::any(alive && dep < len)) {
    if (alive && dep < len) {
      const uint32_t c = norm[s + dep];
      if (dep == 0 || ((u.w >> ChildBit(c)) & 1u)) {
        u = ptrie[(dep == 0 ? root : (u.x >> kDatBaseShiftDev)) ^ c];
        alive = (u.x & 0x1FFu) == (0x100u | c);
      } else {
        alive = false;
      }
      ++dep;
    }
  }
  return alive && (u.x & kDatTerminalDev) ? (u.y & kPtIdMask) : static_cast<uint32_t>(d.unk_id);
}

template <bool WORD>
SPMX_DEVICE void charword_long_block(const LongArgs &a, unsigned char *smem) {
  const int lane = wv::lane();
  const SpmxDev &d = a.dev;
  uint32_t *q = reinterpret_cast<uint32_t *>(smem);
  uint8_t *rawwin = smem + kCwQueue * 4u;
  const uint32_t wave_id = static_cast<uint32_t>(wv::block_id() * wv::waves_per_block() + wv::wave_in_block());
  const uint32_t n_waves = static_cast<uint32_t>(wv::grid_size() * wv::waves_per_block());
  const uint32_t count = *a.list_count;
  const int n_extra = d.n_prefix + d.n_suffix;
  const bool bf = (d.flags & kNfByteFallback) != 0;
  const bool reverse = (d.flags & kNfReverse) != 0;
  const uint32_t spb = SpByteOf(d);
  unsigned long long st_sent = 0, st_raw = 0, st_ids = 0;
  for (uint32_t i = wave_id; i < count; i += n_waves) {
    const uint32_t sid = a.list[i];
    const uint64_t beg = a.offs[sid];
    const uint64_t L64 = a.offs[sid + 1] - beg;
    auto fail = [&](uint32_t code) {
      if (lane == 0) {
        a.counts[sid] = 0; a.tmp_off[sid] = 0; a.sent_status[sid] = static_cast<uint8_t>(code);
        wv::atomic_add(&a.side->n_failed, 1ull);
      }
    };
    if (L64 > 0x7FFFFFF0ull / (d.expand_max ? d.expand_max : 1u)) { fail(kSsOutOfRange); continue; }   // its normalized form could pass 2^31 bytes
    const int L = static_cast<int>(L64);
    // a slice for a normalized form of up to `cap` bytes and an id per byte position (as uni_long_block's)
    uint8_t *norm = nullptr;
    int32_t *bid = nullptr;
    auto take_slice = [&](uint64_t cap) -> bool {
      const uint64_t b_text = Align16(cap + 64 + 16);
      const uint64_t need = b_text + Align16((cap + 2) * 4);
      unsigned long long at = 0;
      if (lane == 0) at = wv::atomic_add(a.pool_head, static_cast<unsigned long long>(need));
      at = (static_cast<unsigned long long>(wv::shfl(static_cast<uint32_t>(at >> 32), 0)) << 32) | wv::shfl(static_cast<uint32_t>(at), 0);
      if (at + need > a.pool_cap) {                                   // the host grows the pool and launches again
        if (lane == 0) { a.retry_list[wv::atomic_add(a.retry_count, 1u)] = sid; a.counts[sid] = 0u; }
        return false;
      }
      norm = a.pool + at;
      bid = reinterpret_cast<int32_t *>(norm + b_text);
      return true;
    };
    int nlen = 0;
    if (L > 0) {
      const bool esc3 = (d.flags & kNfEscapeWs) && !(d.flags & kNfCompressSp);
      uint64_t cap1 = esc3 ? 3ull * static_cast<uint64_t>(L) + 64u : static_cast<uint64_t>(L) + static_cast<uint64_t>(L) / 2u + 64u;
      const uint64_t bound = static_cast<uint64_t>(L) * d.expand_max + 16u;
      if (cap1 > bound) cap1 = bound;
      if (!take_slice(cap1)) continue;
      nlen = normalize_wave<true>(d, a.text + beg, L, norm, static_cast<int>(cap1), lane);
      if (nlen < 0) {                                                 // it outgrew the slice: count, a slice of that size, write
        int n2 = 0;
        if (lane == 0) {
          int nsp = 0;
          FlatSink cs{nullptr, nullptr, 0};
          n2 = norm_lane_any(d, a.text, beg, L, cs, rawwin, &nsp);
        }
        n2 = wv::shfl(n2, 0);
        if (n2 > 0) {
          if (!take_slice(static_cast<uint64_t>(n2))) continue;
          if (lane == 0) {
            FlatSink ws{norm, nullptr, n2};
            int nsp2 = 0;
            norm_lane_any(d, a.text, beg, L, ws, rawwin, &nsp2);
          }
        }
        nlen = n2;
      }
    }
    wv::sync_global();
    // ids of one cut; `prev_unk`: the cut before it is unknown
    auto count_of = [&](uint32_t id, int s, int e, bool have, bool prev_unk) -> int {
      if (!have) return 0;
      if (static_cast<int32_t>(id) != d.unk_id) return 1;
      if (bf) return (e - s) + (norm[s] == spb ? 2 : 0);              // (only a cut's first byte can be the one-byte space symbol)
      return prev_unk ? 0 : 1;
    };
    // ---- pass 1: walk, keep the ids, count ----
    int total = 0;
    bool control = false;
    uint32_t carry_unk = 0;                                           // the previous round's last cut is unknown
    if (nlen > 0)
      cw_for_each_round<WORD>(d, norm, nlen, q, lane, [&](int s, int e, bool have) {
        const uint32_t id = cw_walk(d, norm, s, e, have);
        if (have) bid[s] = static_cast<int32_t>(id);
        control = control || wv::any(have && id == kPtControlCut);
        const uint32_t unk = have && static_cast<int32_t>(id) == d.unk_id ? 1u : 0u;
        const uint32_t left = wv::lane_up1(unk, carry_unk);
        int t = 0;
        wave_excl_scan(count_of(id, s, e, have, left != 0u), lane, &t);
        total += t;
        const int r = wv::popc64(wv::ballot(have));
        carry_unk = wv::shfl(unk, r - 1);
      });
    if (control) { fail(kSsInternal); continue; }                     // "all normalized characters are not consumed."
    // ---- the sentence's ids in the arena ----
    const int n_out = total + n_extra;
    unsigned long long off = 0;
    if (lane == 0) off = wv::atomic_add(a.arena_head, static_cast<unsigned long long>(n_out));
    off = (static_cast<unsigned long long>(wv::shfl(static_cast<uint32_t>(off >> 32), 0)) << 32) | wv::shfl(static_cast<uint32_t>(off), 0);
    if (lane == 0) { a.counts[sid] = static_cast<uint32_t>(n_out); a.tmp_off[sid] = off; }
    if (off + static_cast<unsigned long long>(n_out) > a.arena_cap) {
      if (lane == 0) wv::atomic_or(a.status, kStArenaOverflow);
      continue;
    }
    int32_t *dst = a.arena + off;
    int32_t *dtb = a.arena_tb ? a.arena_tb + off : nullptr;
    if (lane < d.n_prefix) dst[lane] = d.prefix_ids[lane];
    if (lane < d.n_suffix) dst[d.n_prefix + total + lane] = d.suffix_ids[lane];
    // ---- pass 2: place ----
    wv::sync_global();                                                // (pass 1's ids are read by the lanes of other rounds' cuts)
    int done = 0;
    carry_unk = 0;
    if (nlen > 0)
      cw_for_each_round<WORD>(d, norm, nlen, q, lane, [&](int s, int e, bool have) {
        const uint32_t id = have ? static_cast<uint32_t>(bid[s]) : 0u;
        const uint32_t unk = have && static_cast<int32_t>(id) == d.unk_id ? 1u : 0u;
        const uint32_t left = wv::lane_up1(unk, carry_unk);
        const int cnt = count_of(id, s, e, have, left != 0u);
        int t = 0;
        const int pos = done + wave_excl_scan(cnt, lane, &t);
        done += t;
        if (unk && bf) {                                              // one BYTE id per byte of the unknown cut (:581-603)
          int j = pos;
          for (int x = s; x < e; ++x) {
            const uint32_t b = norm[x];
            const int nb = b == spb ? 3 : 1;
            for (int y = 0; y < nb; ++y, ++j) {
              const uint32_t byte = b == spb ? (y == 0 ? 0xE2u : (y == 1 ? 0x96u : 0x81u)) : b;
              dst[d.n_prefix + (reverse ? total - 1 - j : j)] = d.byte_ids[byte];
              if (dtb) dtb[d.n_prefix + (reverse ? total - 1 - j : j)] = s;
            }
          }
        } else if (cnt == 1) {
          dst[d.n_prefix + (reverse ? total - 1 - pos : pos)] = static_cast<int32_t>(id);
          if (dtb) dtb[d.n_prefix + (reverse ? total - 1 - pos : pos)] = s;
        }
        const int r = wv::popc64(wv::ballot(have));
        carry_unk = wv::shfl(unk, r - 1);
      });
    ++st_sent; st_raw += static_cast<unsigned long long>(L); st_ids += static_cast<unsigned long long>(n_out);
  }
  if (a.stats && lane == 0 && st_sent) {
    wv::atomic_add(&a.stats[0], st_sent);
    wv::atomic_add(&a.stats[1], st_raw);
    wv::atomic_add(&a.stats[2], st_ids);
  }
}

}  // namespace spmx
#endif
