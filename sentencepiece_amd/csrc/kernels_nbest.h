// NBestEncode on the device: unigram::Model::NBestEncode
// (src/unigram_model.cc:686-717) = Lattice::SetSentence (:114-152) + Model::PopulateNodes (:547-596) +
// Lattice::NBest (:345-515: float Viterbi for the exact heuristic, then A* from EOS), followed per result by the id
// rules of PopulateSentencePieceText (src/sentencepiece_processor.cc:547-636) and the extra options (:1019-1064).
//
// One SENTENCE PER LANE, everything in the lane's own slice of an HBM scratch buffer: the lattice (character starts,
// nodes, the nodes ending at every position), the hypotheses and the agenda.  The agenda is a binary heap that
// performs exactly the element moves of libstdc++'s push_heap / pop_heap (bits/stl_heap.h __push_heap /
// __adjust_heap): std::priority_queue's order among equal keys is part of the reference's output.  A cold path --
// no LDS, no cross-lane step, the lanes of a wave simply diverge; its input is the normalized text in device form
// (U+2581 as one byte under kNfCompressSp) written by the Normalize kernels.
#ifndef SPMX_KERNELS_NBEST_H_
#define SPMX_KERNELS_NBEST_H_

namespace spmx {

// The first launch runs every sentence with 16-bit lattice indices under these capacities; what exceeds them is set
// aside (NBestArgs::retry_list) and runs in a second launch with 32-bit indices and capacities sized for the longest
// of them (api.cc LatticeBatchHost): no length limit.
constexpr uint32_t kNbMaxLen = 1024;        // normalized (device) bytes per sentence, first launch
constexpr uint32_t kNbMaxNodes = 16384;     // lattice nodes per sentence, first launch
constexpr uint32_t kNbAgendaCap = 10000 + 512;   // :487 kMaxAgendaSize + the largest fan-in handled
constexpr uint32_t kStNbestOverflow = 1u << 5;   // status: a per-sentence capacity was exceeded
constexpr int kNbExpectedFracBits = 24;          // mode 6: a node adds llrint(freq * p * 2^24) to its piece (SPMX_EXPECTED_FRAC_BITS)

template <typename IX>
struct NbNodeT { IX pos, length, byte_begin, byte_len; int32_t id; float score, backtrace; uint32_t prev; };   // 24 / 32 bytes
struct NbHyp { uint32_t next; uint32_t node; float fx, gx; };                                      // 16 bytes

SPMX_HD inline uint64_t NbAlign16(uint64_t x) { return (x + 15u) & ~static_cast<uint64_t>(15); }
// bytes of one lane's slice; ix = sizeof(IX)
SPMX_HD inline uint64_t NbestLaneBytes(uint64_t max_len, uint64_t max_nodes, uint64_t max_hyps, uint32_t ix) {
  return NbAlign16((max_len + 2) * ix)                       // surf: character starts
       + NbAlign16(max_nodes * (4ull * ix + 16))             // nodes
       + NbAlign16((max_len + 3) * 4ull)                     // end_off: CSR offsets of the nodes ending at a position
       + NbAlign16(max_nodes * ix)                           // end_idx
       + NbAlign16((max_len + 2) * ix)                       // cursor per position
       + NbAlign16(max_hyps * sizeof(NbHyp))                 // hypotheses (modes 1 and 4: alpha, one float per position; mode 3: alpha and H; mode 6: alpha and beta)
       + kNbAgendaCap * 4ull + 64;
}

struct NBestArgs {
  SpmxDev dev;
  const uint8_t *norm;          // packed normalized text, device form
  const uint64_t *norm_offs;    // n + 1
  uint32_t n;
  uint32_t nbest;               // 2 .. 1024 (mode 0); the draws per sentence, 1 .. 512 (mode 4); the rows a sentence may fill,
                                // num_samples + 2 (mode 5: the best path and the num_samples + 1 results of the search); 1 otherwise
  uint32_t mode;                // 0 Lattice::NBest (:345-515); 1 Lattice::Sample(inv_theta) (:511-542); 2 Lattice::Viterbi
                                // (:161-198), the kOriginal encoder (:674-692); 3 Lattice::CalculateEntropy(inv_theta)
                                // (:263-291): one result without ids, its score the entropy; 4 SampleEncodeAndScore with
                                // replacement (:828-843): `nbest` draws of mode 1's sampler, each with its log probability;
                                // 5 SampleEncodeAndScore without replacement (:771-827): mode 0's A* with Gumbel keys;
                                // 6 the unigram trainer's E-step of one sentence (Lattice::PopulateMarginal :235-261 and
                                // the node count of Lattice::Viterbi): no result rows, the outputs below
  uint32_t include_best;        // mode 5: the Viterbi path first, with score 0, and out of the samples
  float inv_theta;              // modes 1, 3, 4, 5
  uint64_t seed;                // mode 1: the lanes' generators are keyed by (seed, sentence index); mode 4: draw j of
                                // sentence i by (hash of the seed, i, j); mode 5: (hash of the seed, sentence index)
  uint64_t index_base;          // the sentence index of those keys is index_base + s: a batch that is rows [k, n) of a larger
                                // one draws what the larger one draws for them (0: the batch's own numbering)
  uint8_t *scratch;             // [lanes of the launch][lane_bytes]
  uint64_t lane_bytes;
  uint32_t max_hyps;
  uint32_t max_len, max_nodes;  // this launch's capacities (normalized bytes, lattice nodes)
  const uint32_t *list;         // the sentences of this launch (null: 0 .. n - 1)
  uint32_t n_list;
  uint32_t live_lanes;          // lanes of the launch that own a slice (0: all)
  uint32_t *retry_list;         // sentences beyond the capacities go here (null: they fail with kStNbestOverflow)
  uint32_t *retry_count;
  unsigned long long *retry_max_len;   // the longest of them (normalized bytes)
  int32_t *arena;               // ids of all results, allocated by atomics
  int32_t *arena_nb, *arena_ne; // spans form, else null: next to every id in `arena` the byte range [nb, ne) of the normalized
                                // DEVICE text its token covers (PopulateSentencePieceText :566-617: a run of unknown
                                // characters is one token; of a character's byte-fallback pieces the last one carries
                                // the range, the others are empty at its begin); an eos is -1, -1 (the end of the INPUT, :1033-1034), a bos -2, -2 (0)
  unsigned long long *arena_head;
  uint64_t arena_cap;
  unsigned long long *res_off;  // [n][nbest] where result k of sentence s sits in the arena
  uint32_t *res_len;            // [n][nbest]
  float *res_score;             // [n][nbest]
  uint32_t *res_count;          // [n]
  uint32_t *status;
  // mode 6
  const uint32_t *freq;         // [n] the sentences' weights (null: all 1)
  unsigned long long *acc;      // [piece_size] expected counts in fixed point, kNbExpectedFracBits fraction bits: ADDED to
  float *log_z;                 // [n] log Z of the sentence, not weighted (null: not asked for)
  uint32_t *viterbi_nodes;      // [n] nodes on the best path (null: not asked for)
};

// std::push_heap with comp(a, b) = a->fx < b->fx
SPMX_DEVICE void nb_heap_push(uint32_t *heap, uint32_t *hn, const NbHyp *hy, uint32_t value) {
  int hole = static_cast<int>((*hn)++);
  const float fx = hy[value].fx;
  while (hole > 0) {
    const int parent = (hole - 1) / 2;
    if (!(hy[heap[parent]].fx < fx)) break;
    heap[hole] = heap[parent];
    hole = parent;
  }
  heap[hole] = value;
}
// top(), then std::pop_heap + pop_back
SPMX_DEVICE uint32_t nb_heap_pop(uint32_t *heap, uint32_t *hn, const NbHyp *hy) {
  const uint32_t top = heap[0];
  const uint32_t value = heap[*hn - 1];
  const int len = static_cast<int>(--(*hn));
  if (len == 0) return top;
  int hole = 0, child = 0;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (hy[heap[child]].fx < hy[heap[child - 1]].fx) --child;
    heap[hole] = heap[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    heap[hole] = heap[child - 1];
    hole = child - 1;
  }
  const float fx = hy[value].fx;
  while (hole > 0) {
    const int parent = (hole - 1) / 2;
    if (!(hy[heap[parent]].fx < fx)) break;
    heap[hole] = heap[parent];
    hole = parent;
  }
  heap[hole] = value;
  return top;
}

// std::exp(float) as the reference's build has it: glibc's expf.  The emulated body (tests/emu) runs on the host and calls
// it, which is what makes its entropies the reference's bit for bit; the device takes the double exp rounded to float --
// the same number but for a rare last bit (over the golden sentences the two forms differ in 2 results of 260, by
// 5.6e-7 relative at most).
SPMX_DEVICE float nb_exp_float(float x) {
#ifdef SPMX_EMULATED
  return expf(x);
#else
  return static_cast<float>(exp(static_cast<double>(x)));
#endif
}

template <typename IX>
SPMX_DEVICE void nbest_lane(const NBestArgs &a, uint32_t s, uint8_t *mine) {
  typedef NbNodeT<IX> NbNode;
  const SpmxDev &d = a.dev;
  const uint8_t *norm = a.norm + a.norm_offs[s];
  const int size = static_cast<int>(a.norm_offs[s + 1] - a.norm_offs[s]);
  const bool bf = (d.flags & kNfByteFallback) != 0;
  const bool reverse = (d.flags & kNfReverse) != 0;
  const uint32_t spb = SpByteOf(d);
  const int n_extra = d.n_prefix + d.n_suffix;
  unsigned long long *res_off = a.res_off + static_cast<uint64_t>(s) * a.nbest;
  uint32_t *res_len = a.res_len + static_cast<uint64_t>(s) * a.nbest;
  float *res_score = a.res_score + static_cast<uint64_t>(s) * a.nbest;
  a.res_count[s] = 0;
  // one result = the extra ids around `body` ids produced by `emit`
  auto alloc = [&](int n_ids) -> int32_t * {
    const unsigned long long at = wv::atomic_add(a.arena_head, static_cast<unsigned long long>(n_ids));
    const uint32_t k = a.res_count[s];
    res_off[k] = at;
    res_len[k] = static_cast<uint32_t>(n_ids);
    if (at + static_cast<unsigned long long>(n_ids) > a.arena_cap) { wv::atomic_or(a.status, kStArenaOverflow); return nullptr; }
    return a.arena + at;
  };
  // the extra ids around a result's `body` ids (ApplyExtraOptions, sentencepiece_processor.cc:1019-1064); returns
  // where the body goes
  auto put_extras = [&](int32_t *dst, int body) -> int32_t * {
    for (int x = 0; x < d.n_prefix; ++x) dst[x] = d.prefix_ids[x];
    for (int x = 0; x < d.n_suffix; ++x) dst[d.n_prefix + body + x] = d.suffix_ids[x];
    if (a.arena_nb) {
      int32_t *nb = a.arena_nb + (dst - a.arena), *ne = a.arena_ne + (dst - a.arena);
      for (int x = 0; x < d.n_prefix; ++x) nb[x] = ne[x] = ((d.extra_eos >> x) & 1u) ? -1 : -2;                       // (reverse after eos puts an eos in front)
      for (int x = 0; x < d.n_suffix; ++x) nb[d.n_prefix + body + x] = ne[d.n_prefix + body + x] = ((d.extra_eos >> (kMaxExtra + x)) & 1u) ? -1 : -2;
    }
    return dst + d.n_prefix;
  };
  if (size == 0 && a.mode == 3u) {               // BOS and EOS alone: H[eos] = 0 + exp(0) * (0 + 0), returned negated (:263-291)
    res_off[0] = 0;
    res_len[0] = 0;
    res_score[0] = -0.f;
    a.res_count[s] = 1;
    return;
  }
  if (size == 0 && (a.mode == 4u || a.mode == 5u)) return;         // :745-747 no result (the caller's "returns empty result.")
  if (size == 0 && a.mode == 6u) {               // no node: Z = 0, nothing expected, an empty best path
    if (a.log_z) a.log_z[s] = 0.f;
    if (a.viterbi_nodes) a.viterbi_nodes[s] = 0u;
    return;
  }
  if (size == 0) {                               // unigram_model.cc:688-690: one empty result, score 0
    int32_t *dst = alloc(n_extra);
    if (dst) put_extras(dst, 0);
    res_score[0] = 0.f;
    a.res_count[s] = 1;
    return;
  }
  // beyond this launch's capacities: to the second launch, or a failure when this is it
  auto set_aside = [&]() {
    if (a.retry_list) {
      a.retry_list[wv::atomic_add(a.retry_count, 1u)] = s;
      wv::atomic_max(a.retry_max_len, static_cast<unsigned long long>(size));
    } else {
      wv::atomic_or(a.status, kStNbestOverflow);
    }
  };
  if (static_cast<uint32_t>(size) > a.max_len) { set_aside(); return; }
  const uint64_t ML = a.max_len, MN = a.max_nodes;
  IX *surf = reinterpret_cast<IX *>(mine);
  NbNode *nodes = reinterpret_cast<NbNode *>(mine + NbAlign16((ML + 2) * sizeof(IX)));
  uint32_t *end_off = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(nodes) + NbAlign16(MN * sizeof(NbNode)));
  IX *end_idx = reinterpret_cast<IX *>(reinterpret_cast<uint8_t *>(end_off) + NbAlign16((ML + 3) * 4));
  IX *cursor = reinterpret_cast<IX *>(reinterpret_cast<uint8_t *>(end_idx) + NbAlign16(MN * sizeof(IX)));
  NbHyp *hy = reinterpret_cast<NbHyp *>(reinterpret_cast<uint8_t *>(cursor) + NbAlign16((ML + 2) * sizeof(IX)));
  uint32_t *heap = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(hy) + NbAlign16(static_cast<uint64_t>(a.max_hyps) * sizeof(NbHyp)));
  // ---- SetSentence (:114-152): character starts ----
  int len = 0;
  for (int p = 0; p < size;) {
    surf[len++] = static_cast<IX>(p);
    const uint32_t c = norm[p];
    int mb = c == spb ? 1 : OneCharLenDev(c);
    if (mb > size - p) mb = size - p;
    p += mb;
  }
  surf[len] = static_cast<IX>(size);
  // ---- PopulateNodes (:547-596).  Nodes 0 = BOS, 1 = EOS, then in insertion order (begin position, then length):
  // the order of end_nodes(pos) that Viterbi's "first best wins" and the A* expansion follow ----
  uint32_t n_nodes = 2;
  nodes[0] = NbNode{0, 0, 0, 0, -1, 0.f, 0.f, 0u};
  nodes[1] = NbNode{static_cast<IX>(len), 0, 0, 0, -1, 0.f, 0.f, 0u};
  const float unk_score = d.unk_score;                         // :555 min_score() - kUnkPenalty
  const uint32_t root = d.ptrie[0].x >> kDatBaseShiftDev;
  bool over = false;
  for (int bp = 0; bp < len && !over; ++bp) {
    const int b0 = surf[bp];
    bool single = false;
    uint32_t nb = root;
    int pos_c = bp;                                            // get_chars_length (:548-552), monotone in the key length
    for (int kp = b0; kp < size;) {                            // commonPrefixSearch: matches in increasing length
      const uint32_t c = norm[kp];
      const U4 u = d.ptrie[nb ^ c];
      if ((u.x & 0x1FFu) != (0x100u | c)) break;
      ++kp;
      nb = u.x >> kDatBaseShiftDev;
      if (!(u.x & kDatTerminalDev)) continue;
      while (surf[pos_c] < kp) ++pos_c;
      const int length = pos_c - bp;
      if (u.y & kPtUnused) continue;                           // :576
      if (n_nodes >= a.max_nodes) { over = true; break; }
      float sc = wv::bits_to_float(u.z);
      if (u.y & kPtUserDefined) sc = static_cast<float>(static_cast<double>(static_cast<float>(length) * d.max_score) - 0.1);   // :580
      nodes[n_nodes++] = NbNode{static_cast<IX>(bp), static_cast<IX>(length), static_cast<IX>(b0),
                                static_cast<IX>(surf[bp + length] - b0), static_cast<int32_t>(u.y & kPtIdMask), sc, 0.f, 0u};
      if (length == 1) single = true;
    }
    if (!single && !over) {                                    // :589-593 the UNK node
      if (n_nodes >= a.max_nodes) { over = true; break; }
      nodes[n_nodes++] = NbNode{static_cast<IX>(bp), 1, static_cast<IX>(b0), static_cast<IX>(surf[bp + 1] - b0),
                                d.unk_id, unk_score, 0.f, 0u};
    }
  }
  if (over) { set_aside(); return; }
  // end_nodes as CSR over positions (insertion order within a position): BOS ends at 0
  for (int p = 0; p <= len + 1; ++p) end_off[p] = 0;
  end_off[0 + 1] = 1;
  for (uint32_t i = 2; i < n_nodes; ++i) ++end_off[nodes[i].pos + nodes[i].length + 1];
  for (int p = 0; p <= len; ++p) end_off[p + 1] += end_off[p];
  for (int p = 0; p <= len; ++p) cursor[p] = 0;
  end_idx[end_off[0] + cursor[0]++] = 0;
  for (uint32_t i = 2; i < n_nodes; ++i) {
    const int e = nodes[i].pos + nodes[i].length;
    end_idx[end_off[e] + cursor[e]++] = static_cast<IX>(i);
  }
  // ---- Viterbi (:167-198): backtrace_score of every node, begin positions in order (nodes are sorted by pos) ----
  auto best_into = [&](int pos, float score, uint32_t *prev) -> float {      // first best left node wins (:171)
    float best = 0.f;
    bool have = false;
    for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
      const float sc = nodes[end_idx[l]].backtrace + score;
      if (!have || sc > best) { best = sc; have = true; *prev = end_idx[l]; }
    }
    return best;
  };
  if (a.mode == 0u || a.mode == 2u || a.mode == 6u || (a.mode == 5u && a.include_best)) {
    for (uint32_t i = 2; i < n_nodes; ++i) nodes[i].backtrace = best_into(nodes[i].pos, nodes[i].score, &nodes[i].prev);
    nodes[1].backtrace = best_into(len, 0.f, &nodes[1].prev);
  }
  // ids of a path given as a chain of node indices, left to right through `next_of` (PopulateSentencePieceText
  // :581-613: a run of unknown pieces yields one id, byte fallback one id per byte), twice: count, then write
  // the ids of ONE lattice node of a path (dst null: count only).  k: ids so far; last: where the latest token that
  // is not a byte-fallback piece went (a run of unknown pieces extends it)
  auto put_node = [&](const NbNode &x, int32_t *dst, int body, int &k, bool &prev_unk, int &last) {
    const bool unk = x.id == d.unk_id;
    const int32_t nb0 = static_cast<int32_t>(x.byte_begin), ne0 = static_cast<int32_t>(x.byte_begin) + static_cast<int32_t>(x.byte_len);
    int32_t *snb = dst && a.arena_nb ? a.arena_nb + (dst - a.arena) : nullptr;
    int32_t *sne = dst && a.arena_nb ? a.arena_ne + (dst - a.arena) : nullptr;
    if (unk && bf) {
      int total = 0, j = 0;
      for (uint32_t t = 0; t < x.byte_len; ++t) total += norm[x.byte_begin + t] == spb ? 3 : 1;
      for (uint32_t t = 0; t < x.byte_len; ++t) {
        const uint32_t b = norm[x.byte_begin + t];
        const int nbt = b == spb ? 3 : 1;
        for (int y = 0; y < nbt; ++y, ++j) {
          const int at = reverse ? body - 1 - k : k;
          if (dst) dst[at] = d.byte_ids[b == spb ? (y == 0 ? 0xE2u : (y == 1 ? 0x96u : 0x81u)) : b];
          if (snb) { snb[at] = nb0; sne[at] = j == total - 1 ? ne0 : nb0; }       // :595-606
          ++k;
        }
      }
    } else if (!(unk && prev_unk)) {
      const int at = reverse ? body - 1 - k : k;
      if (dst) dst[at] = x.id;
      if (snb) { snb[at] = nb0; sne[at] = ne0; }
      last = at;
      ++k;
    } else if (sne) {
      sne[last] = ne0;                                                             // :612-616 the run's token grows
    }
    prev_unk = unk;
  };
  // ids of a path given as a chain of node indices, left to right through `next_of` (PopulateSentencePieceText
  // :581-613: a run of unknown pieces yields one id, byte fallback one id per byte), twice: count, then write
  auto emit_path = [&](auto first_of, auto next_of, auto done_of, float score) -> bool {
    int body = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int32_t *dst = nullptr;
      if (pass == 1) {
        dst = alloc(body + n_extra);
        if (!dst) return false;
        dst = put_extras(dst, body);
      }
      int k = 0, last = 0;
      bool prev_unk = false;
      for (uint32_t h = first_of(); !done_of(h); h = next_of(h)) put_node(nodes[h], dst, body, k, prev_unk, last);
      body = k;
    }
    res_score[a.res_count[s]] = score;
    a.res_count[s] = a.res_count[s] + 1;
    return true;
  };
  if (a.mode == 2u) {
    // ---- Lattice::Viterbi (:161-198): the path is the prev chain from EOS; emitted left to right by reversing it in
    // place (prev -> next) ----
    uint32_t nxt = 1u, cur = nodes[1].prev;             // walk from EOS's prev towards BOS, turning the links around
    while (cur != 0u) {
      const uint32_t pv = nodes[cur].prev;
      nodes[cur].prev = nxt;
      nxt = cur;
      cur = pv;
    }
    emit_path([&] { return nxt; }, [&](uint32_t h) { return nodes[h].prev; }, [&](uint32_t h) { return h == 1u; }, nodes[1].backtrace);
    return;
  }
  auto lse = [](float x, float y, bool init) -> float {                     // LogSumExp (:47-59)
    if (init) return y;
    const float vmin = x < y ? x : y, vmax = x < y ? y : x;
    if (vmax > vmin + 50.f) return vmax;
    return static_cast<float>(static_cast<double>(vmax) + log(exp(static_cast<double>(vmin - vmax)) + 1.0));
  };
  // a generator per sentence (mode 1) or per draw (mode 4), its state set by the mode: splitmix64, 53 random bits per draw
  unsigned long long st = 0;
  auto uniform = [&]() -> double {
    st += 0x9E3779B97F4A7C15ull;
    unsigned long long z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
  };
  // The scored modes (4, 5) put the caller's seed through splitmix64's finalizer before it enters the key: calls without a
  // seed of their own count one up per call, and the multiplier mode 1 gives the seed is the generator's own step, so
  // under mode 1's key the stream of seed + 1 is that of seed moved on by one draw.  Mode 1 keeps its key: its draws
  // are pinned.
  auto hashed_seed = [&]() -> unsigned long long {
    unsigned long long z = a.seed + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  // Lattice::Sample's backward pass (:520-542) over the forward scores `alpha` (per begin position): one left node after
  // another from EOS, each drawn with probability exp(alpha[l] + inv_theta * score[l] - Z) (std::discrete_distribution's
  // weights).  Returns the path's first node; the chain runs left to right through `prev`, up to EOS (node 1).
  auto draw_path = [&](const float *alpha) -> uint32_t {
    float Z = alpha[len];
    uint32_t nxt = 1u;                                  // the chain is built right to left: prev = the node to the right
    int pos = len;
    for (;;) {
      double sum = 0.0;
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const NbNode &ln = nodes[end_idx[l]];
        sum += exp(static_cast<double>(alpha[ln.pos] + a.inv_theta * ln.score - Z));
      }
      double r = uniform() * sum;
      uint32_t pick = end_idx[end_off[pos + 1] - 1];
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const NbNode &ln = nodes[end_idx[l]];
        r -= exp(static_cast<double>(alpha[ln.pos] + a.inv_theta * ln.score - Z));
        if (r < 0.0) { pick = end_idx[l]; break; }
      }
      if (pick == 0u) break;                            // reached BOS
      nodes[pick].prev = nxt;
      nxt = pick;
      pos = nodes[pick].pos;
      Z = alpha[pos];
    }
    return nxt;
  };
  if (a.mode == 1u) {
    // ---- Lattice::Sample(inv_theta) (:511-542): ForwardAlgorithm (:200-216) -- alpha of a node depends on its begin
    // position only: kept per position in the (idle) hypothesis slice -- then the backward pass ----
    float *alpha = reinterpret_cast<float *>(hy);
    alpha[0] = 0.f;
    for (int pos = 1; pos <= len; ++pos) {
      float acc = 0.f;
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const NbNode &ln = nodes[end_idx[l]];
        acc = lse(acc, a.inv_theta * ln.score + alpha[ln.pos], l == end_off[pos]);
      }
      alpha[pos] = acc;
    }
    // keyed by (seed, sentence)
    st = a.seed * 0x9E3779B97F4A7C15ull + (a.index_base + static_cast<unsigned long long>(s) + 1ull) * 0xD1B54A32D192ED03ull;
    const uint32_t first = draw_path(alpha);
    emit_path([&] { return first; }, [&](uint32_t h) { return nodes[h].prev; }, [&](uint32_t h) { return h == 1u; }, 0.f);
    return;
  }
  if (a.mode == 6u) {
    // ---- The E-step of one sentence (unigram::Trainer::RunEStep, src/unigram_model_trainer.cc:318-367):
    // Lattice::PopulateMarginal(freq, &expected) (:235-261) and the size of Lattice::Viterbi()'s path.  alpha of a node
    // depends on its begin position, beta (BackwardAlgorithm :218-233) on its end position: A and B, one float per
    // position.  The reference's number is the contract, as in modes 3 and 4: its order, float, nothing contracted.
    // Every capacity is checked BEFORE the first add to `acc`: a sentence that is set aside has added nothing, the wide
    // launch counts it once. ----
#pragma clang fp contract(off)
    float *A = reinterpret_cast<float *>(hy);
    float *B = A + (len + 1);
    const uint64_t room = static_cast<uint64_t>(a.max_hyps) * (sizeof(NbHyp) / sizeof(float));
    if (2ull * (static_cast<uint64_t>(len) + 1ull) > room) { set_aside(); return; }
    A[0] = 0.f;                                         // ForwardAlgorithm(1.0) (:200-216)
    for (int pos = 1; pos <= len; ++pos) {
      float acc = 0.f;
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const NbNode &ln = nodes[end_idx[l]];
        acc = lse(acc, ln.score + A[ln.pos], l == end_off[pos]);
      }
      A[pos] = acc;
    }
    // BackwardAlgorithm: the nodes beginning at a position are a run of `nodes` (sorted by position, in insertion order
    // -- the trie's matches by increasing length, the unknown node last); positions from the right
    B[len] = 0.f;
    for (uint32_t hi = n_nodes; hi > 2u;) {
      uint32_t lo = hi - 1u;
      const int pos = nodes[lo].pos;
      while (lo > 2u && static_cast<int>(nodes[lo - 1u].pos) == pos) --lo;
      float acc = 0.f;
      for (uint32_t i = lo; i < hi; ++i) acc = lse(acc, nodes[i].score + B[static_cast<int>(nodes[i].pos) + static_cast<int>(nodes[i].length)], i == lo);
      B[pos] = acc;
      hi = lo;
    }
    const float Z = A[len];
    const double weight = static_cast<double>(a.freq ? a.freq[s] : 1u);
    for (uint32_t i = 2; i < n_nodes; ++i) {
      const NbNode &x = nodes[i];
      if (x.id < 0) continue;                           // :250
      const float u = A[x.pos] + x.score;
      const float v = u + B[static_cast<int>(x.pos) + static_cast<int>(x.length)];
      const float t = v - Z;
      const double p = exp(static_cast<double>(t));
      const long long q = llrint(weight * p * static_cast<double>(1ll << kNbExpectedFracBits));   // to nearest, ties to even
      if (q > 0) wv::atomic_add(a.acc + x.id, static_cast<unsigned long long>(q));
    }
    if (a.log_z) a.log_z[s] = Z;
    if (a.viterbi_nodes) {                              // lattice.Viterbi().first.size(): nodes, before any id rule
      uint32_t cnt = 0;
      for (uint32_t cur = nodes[1].prev; cur != 0u; cur = nodes[cur].prev) ++cnt;
      a.viterbi_nodes[s] = cnt;
    }
    return;
  }
  if (a.mode == 3u || a.mode == 4u) {
    // ---- The scoring entry points.  Their results are compared with the reference's NUMBER, which on long text is far
    // from the exact one: the reference's recurrences in its order, in float, every product and sum
    // rounded on its own as its x86-64 build rounds them -- the library is built with -ffp-contract=off throughout (csrc/
    // Makefile), and the pragma in the scored blocks says so again where the result depends on it -- LogSumExp in
    // double as written there, and std::exp(float) as nb_exp_float has it. ----
#pragma clang fp contract(off)
    float *alpha = reinterpret_cast<float *>(hy);
    float *H = alpha + (len + 1);                       // mode 3 only
    const uint64_t room = static_cast<uint64_t>(a.max_hyps) * (sizeof(NbHyp) / sizeof(float));
    if ((a.mode == 3u ? 2ull : 1ull) * (static_cast<uint64_t>(len) + 1ull) > room) { set_aside(); return; }
    alpha[0] = 0.f;                                     // ForwardAlgorithm (:200-216)
    for (int pos = 1; pos <= len; ++pos) {
      float acc = 0.f;
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const NbNode &ln = nodes[end_idx[l]];
        const float w = a.inv_theta * ln.score;
        acc = lse(acc, w + alpha[ln.pos], l == end_off[pos]);
      }
      alpha[pos] = acc;
    }
    if (a.mode == 3u) {
      // Lattice::CalculateEntropy (:263-291): H of a node depends on its begin position only, as alpha does
      H[0] = 0.f;
      for (int pos = 1; pos <= len; ++pos) {
        const float ar = alpha[pos];
        float hsum = 0.f;
        for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
          const NbNode &ln = nodes[end_idx[l]];
          const float w = a.inv_theta * ln.score;
          const float t = w + alpha[ln.pos];
          const float lp = t - ar;                      // log of the transition probability
          const float e = nb_exp_float(lp);
          const float g = H[ln.pos] + lp;
          const float c = e * g;
          hsum = hsum + c;
        }
        H[pos] = hsum;
      }
      res_off[0] = 0;
      res_len[0] = 0;
      res_score[0] = -H[len];
      a.res_count[s] = 1;
      return;
    }
    // with replacement (:828-843): the lattice and alpha once, then `nbest` draws, draw j from the generator keyed by
    // (hashed seed, sentence, j) -- a third multiplier beside mode 1's, so the draws of (i, j) and (i + 1, j - 1) are unrelated
    const float marginal = alpha[len];
    const unsigned long long hs = hashed_seed();
    for (uint32_t j = 0; j < a.nbest; ++j) {
      st = hs + (a.index_base + static_cast<unsigned long long>(s) + 1ull) * 0xD1B54A32D192ED03ull +
           (static_cast<unsigned long long>(j) + 1ull) * 0xA0761D6478BD642Full;
      const uint32_t first = draw_path(alpha);
      float score = 0.f;
      for (uint32_t h = first; h != 1u; h = nodes[h].prev) {
        const float w = a.inv_theta * nodes[h].score;
        score = score + w;
      }
      if (!emit_path([&] { return first; }, [&](uint32_t h) { return nodes[h].prev; }, [&](uint32_t h) { return h == 1u; }, score - marginal)) return;
    }
    return;
  }
  // ---- A* (:375-515).  Mode 5 is the same search with stochastic keys (NBest(samples + 1, true, inv_theta), :391-450):
  // f(eos) is a Gumbel variate, a child's g is its log probability and its f a truncated Gumbel below its parent's ----
  const bool wor = a.mode == 5u;
  const uint32_t base = wor && a.include_best ? 1u : 0u;       // mode 5: row 0 is the best path (:756-769)
  const uint32_t want = wor ? a.nbest - 1u : a.nbest;          // results of the search (mode 5: samples + 1; nbest = samples + 2 rows)
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  uint32_t n_hyp = 0, hn = 0, n_res = 0;
  // ids of the complete path below hypothesis `top`, left to right (PopulateSentencePieceText :581-613), as row n_res
  auto emit_hyp = [&](uint32_t top) -> bool {
    int body = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int32_t *dst = nullptr;
      if (pass == 1) {
        dst = alloc(body + n_extra);
        if (!dst) return false;
        dst = put_extras(dst, body);
      }
      int k = 0, last = 0;
      bool prev_unk = false;
      for (uint32_t h = hy[top].next; hy[h].next != kNone; h = hy[h].next) put_node(nodes[hy[h].node], dst, body, k, prev_unk, last);
      body = k;
    }
    return true;
  };
  float fx_last = 0.f, fx_prev = 0.f, marginal = 0.f;          // mode 5: the perturbed scores of the last two results
  uint32_t best_at = kNone;                                    // mode 5: the row of the search that is the best path
  if (wor) {
#pragma clang fp contract(off)
    if (base) {
      // the Viterbi path as a chain of hypotheses, EOS first, so that it is emitted like a result; its prev links
      // stay as they are: a result is the best path when its nodes are (:782-786 compares the node vectors)
      hy[0] = NbHyp{kNone, 1u, 0.f, 0.f};
      n_hyp = 1;
      for (uint32_t cur = nodes[1].prev;; cur = nodes[cur].prev) {
        if (n_hyp >= a.max_hyps) { set_aside(); return; }
        hy[n_hyp] = NbHyp{n_hyp - 1u, cur, 0.f, 0.f};
        ++n_hyp;
        if (cur == 0u) break;
      }
      if (!emit_hyp(n_hyp - 1u)) return;
      res_score[0] = 0.f;                                      // "inclusion probability if we always include the best is 1"
      a.res_count[s] = n_res = 1;
    }
    // ForwardAlgorithm (:200-216) in the reference's order and float arithmetic, as modes 3 and 4 run it: alpha of a node
    // is that of its begin position, kept in the node's backtrace (Viterbi is done with it); nodes are sorted by position
    int at = -1;
    float acc = 0.f;
    for (uint32_t i = 2; i <= n_nodes; ++i) {
      const uint32_t nd = i < n_nodes ? i : 1u;                // EOS last
      const int pos = nodes[nd].pos;
      if (pos != at) {
        at = pos;
        for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
          const NbNode &ln = nodes[end_idx[l]];
          const float w = a.inv_theta * ln.score;
          acc = lse(acc, w + ln.backtrace, l == end_off[pos]);
        }
      }
      nodes[nd].backtrace = acc;
    }
    marginal = nodes[1].backtrace;
    st = hashed_seed() + (a.index_base + static_cast<unsigned long long>(s) + 1ull) * 0xD1B54A32D192ED03ull + 0x8EBC6AF09C88C6E3ull;
  }
  // Gumbel() (:61-70): -log(-log(u + 1e-7f)) in float, u uniform over the 2^24 floats k / 2^24.  Where u + 1e-7f rounds to
  // 1 the reference returns +inf (two values of u); those are drawn again here.
  auto gumbel = [&]() -> float {
    for (;;) {
      const float u = static_cast<float>(static_cast<uint32_t>(uniform() * 16777216.0)) * (1.f / 16777216.f);
      const float t = u + 1e-7f;
      if (t < 1.f) return -logf(-logf(t));
    }
  };
  if (n_hyp >= a.max_hyps) { a.res_count[s] = 0; set_aside(); return; }
  const uint32_t eos_hyp = n_hyp;
  hy[n_hyp] = NbHyp{kNone, 1u, wor ? gumbel() : nodes[1].backtrace, 0.f};
  ++n_hyp;
  nb_heap_push(heap, &hn, hy, eos_hyp);
  while (hn > 0) {
    const uint32_t top = nb_heap_pop(heap, &hn, hy);
    const uint32_t node = hy[top].node;
    if (node == 0) {                                           // reached BOS: a complete path
      if (!emit_hyp(top)) return;
      if (wor) {
#pragma clang fp contract(off)
        // its log probability (:799-809): the float sum of inv_theta * score, left to right, minus the marginal
        float score = 0.f;
        bool is_best = base != 0u;
        uint32_t left = 0u;
        for (uint32_t h = hy[top].next;; h = hy[h].next) {
          const uint32_t nd = hy[h].node;
          if (nodes[nd].prev != left) is_best = false;
          if (hy[h].next == kNone) break;
          const float w = a.inv_theta * nodes[nd].score;
          score = score + w;
          left = nd;
        }
        if (is_best) best_at = n_res;
        res_score[n_res] = score - marginal;
        fx_prev = fx_last;
        fx_last = hy[top].fx;
      } else {
        res_score[n_res] = hy[top].fx;
      }
      a.res_count[s] = ++n_res;
      if (n_res - base == want) break;
      continue;
    }
    const int pos = nodes[node].pos;
    const uint32_t fan = end_off[pos + 1] - end_off[pos];
    if (hn + fan > kNbAgendaCap) { wv::atomic_or(a.status, kStNbestOverflow); return; }
    if (n_hyp + fan > a.max_hyps) { a.res_count[s] = 0; set_aside(); return; }      // again, with a larger hypothesis slice
    const float gx = hy[top].gx;
    if (wor) {
#pragma clang fp contract(off)
      // :428-450, float and double where the reference has them: everything here is float there (std::exp, std::log1p
      // and std::abs of a float), adjusted_probs holds the float result widened
      const float fx = hy[top].fx, Z = nodes[node].backtrace;
      float max_score = -1e8f;
      for (uint32_t l = end_off[pos], i = n_hyp; l < end_off[pos + 1]; ++l, ++i) {
        const uint32_t ln = end_idx[l];
        const float w = a.inv_theta * nodes[ln].score;
        const float prob = gx + nodes[ln].backtrace + w - Z;
        const float perturbed = prob + gumbel();
        if (perturbed > max_score) max_score = perturbed;
        hy[i] = NbHyp{top, ln, perturbed, prob};
      }
      for (uint32_t i = n_hyp; i < n_hyp + fan; ++i) {        // truncated Gumbel, arXiv 1903.06059 appendix B.3
        const float perturbed = hy[i].fx;
        const float v = fx - perturbed + log1pf(-expf(perturbed - max_score));
        hy[i].fx = fx - fmaxf(0.f, v) - log1pf(expf(-fabsf(v)));
        nb_heap_push(heap, &hn, hy, i);
      }
      n_hyp += fan;
    } else {
      for (uint32_t l = end_off[pos]; l < end_off[pos + 1]; ++l) {
        const uint32_t ln = end_idx[l];
        hy[n_hyp] = NbHyp{top, ln, nodes[ln].backtrace + gx, nodes[ln].score + gx};
        nb_heap_push(heap, &hn, hy, n_hyp);
        ++n_hyp;
      }
    }
    if (hn >= 10000u) {                                        // :487-514 keep the best min(512, 10 nbest)
      const uint32_t keep = want * 10u < 512u ? want * 10u : 512u;
      // pop the best `keep` into the (free) tail of the hypothesis slice, then rebuild the heap from them in that order
      if (n_hyp + keep > a.max_hyps) { a.res_count[s] = 0; set_aside(); return; }
      uint32_t *tmp = reinterpret_cast<uint32_t *>(hy + n_hyp);
      for (uint32_t i = 0; i < keep; ++i) tmp[i] = nb_heap_pop(heap, &hn, hy);
      hn = 0;
      for (uint32_t i = 0; i < keep; ++i) nb_heap_push(heap, &hn, hy, tmp[i]);
    }
  }
  if (!wor) return;
  // ---- :775-827.  kappa is the perturbed score of the last result once the best path is out of the samples (erased where
  // it occurs, else the last sample goes); that last result is dropped, and every other score becomes the log of its
  // inclusion probability.  A lattice with no more paths than samples therefore returns one result fewer than it has
  // paths; where nothing is left the sentence owns no result (with include_best and ONE path the reference erases the
  // best path and then reads the back of an empty vector: no result here either). ----
  uint32_t m = n_res - base;
  float kappa_f = fx_last;
  if (base) {
    if (best_at != kNone) {
      if (best_at == n_res - 1u) kappa_f = fx_prev;
      for (uint32_t k = best_at; k + 1u < n_res; ++k) { res_off[k] = res_off[k + 1]; res_len[k] = res_len[k + 1]; res_score[k] = res_score[k + 1]; }
    } else {
      kappa_f = fx_prev;
    }
    if (m > 0u) --m;
  }
  if (m == 0u) { a.res_count[s] = 0; return; }
  --m;
  const double kappa = static_cast<double>(kappa_f);
  for (uint32_t k = base; k < base + m; ++k) {
    if (res_score[k] != 0.f) {                                 // :814 "only modify non best sample inclusion probabilities"
      const double x = static_cast<double>(res_score[k]) - kappa;
      const double y = exp(x);
      const double inc = x <= -10.0 ? x - (y / 2) + (y * y / 24) - ((y * y) * (y * y)) / 2880    // the log Gumbel survival function's series
                                    : log(-expm1(-y));
      res_score[k] = static_cast<float>(inc);
    }
  }
  a.res_count[s] = base + m;
}

// Persistent body: lane l of wave w takes sentences w * 64 + l, + lanes of the launch, ...
template <typename IX>
SPMX_DEVICE void nbest_block(const NBestArgs &a) {
  const uint32_t lane_id = static_cast<uint32_t>(wv::block_id() * wv::waves_per_block() + wv::wave_in_block()) * 64u +
                           static_cast<uint32_t>(wv::lane());
  const uint32_t lanes_all = static_cast<uint32_t>(wv::grid_size() * wv::waves_per_block()) * 64u;
  uint8_t *mine = a.scratch + static_cast<uint64_t>(lane_id) * a.lane_bytes;
  const uint32_t count = a.list ? a.n_list : a.n;
  if (a.live_lanes) { if (lane_id >= a.live_lanes) return; }
  const uint32_t lanes = a.live_lanes ? a.live_lanes : lanes_all;
  for (uint32_t i = lane_id; i < count; i += lanes) nbest_lane<IX>(a, a.list ? a.list[i] : i, mine);
}

}  // namespace spmx
#endif
