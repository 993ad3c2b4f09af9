// The reference-side binding of the encode path: what a maintainer of google/sentencepiece would add to the reference
// tree -- a subclass of sentencepiece::SentencePieceProcessor that forwards the virtuals the
// text -> ids path goes through (src/sentencepiece_processor.h:245-312) to the C ABI of libspmx (include/spmx.h), plus
// the batch entry point the Python wrapper's _EncodeAsIdsBatch (python/src/sentencepiece/sentencepiece.i:439-446) would
// call instead of its thread pool.  Compiled only INSIDE the reference tree (it includes the reference's own header);
// tests/cpp/ref_binding_test.cc builds it against /root/reference where that exists and drives it through a
// base-class pointer with spm_encode's loop (src/spm_encode_main.cc:115-119).
#ifndef SPMX_REFERENCE_BINDING_H_
#define SPMX_REFERENCE_BINDING_H_
#include <atomic>
#include <mutex>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "sentencepiece.pb.h"           // the reference's: NBestSentencePieceText (the proto form of SampleEncodeAndScore)
#include "sentencepiece_model.pb.h"     // the reference's: -I<reference>/src/builtin_pb (NormalizerSpec, for the live spec edits)
#include "sentencepiece_processor.h"   // the reference's: -I<reference>/src
#include "spmx.h"

namespace sentencepiece {

class AmdSentencePieceProcessor : public SentencePieceProcessor {
 public:
  explicit AmdSentencePieceProcessor(int device = 0) : device_(device) {}
  ~AmdSentencePieceProcessor() override { spmx_destroy(h_); }

  // Load(filename) (:245) reads the file and ends here too (sentencepiece_processor.cc:201-206 -> :242)
  util::Status LoadFromSerializedProto(absl::string_view serialized) override {                     // :261
    const util::Status st = SentencePieceProcessor::LoadFromSerializedProto(serialized);            // (keeps every other method working)
    if (!st.ok()) return st;
    return Create(serialized.data(), serialized.size());
  }
  util::Status Load(absl::string_view filename) override {                                           // :245
    const util::Status st = SentencePieceProcessor::Load(filename);
    if (!st.ok()) return st;
    const std::string blob = serialized_model_proto();                                               // :694
    return Create(blob.data(), blob.size());
  }
  util::Status SetEncodeExtraOptions(absl::string_view o) override {                                 // :267
    const util::Status st = SentencePieceProcessor::SetEncodeExtraOptions(o);
    if (!st.ok()) return st;
    const std::string opts(o.data(), o.size());
    unk_piece_option_ = reverse_option_ = false;           // what the piece strings of the scored forms below depend on
    for (size_t at = 0; at <= opts.size();) {
      size_t colon = opts.find(':', at);
      if (colon == std::string::npos) colon = opts.size();
      const std::string f = opts.substr(at, colon - at);
      if (f == "unk" || f == "unk_piece") unk_piece_option_ = true;
      if (f == "reverse") reverse_option_ = !reverse_option_;
      at = colon + 1;
    }
    return ToStatus(spmx_set_encode_extra_options(h_, opts.c_str()), h_);
  }
  util::Status SetDecodeExtraOptions(absl::string_view o) override {                                 // :270
    const util::Status st = SentencePieceProcessor::SetDecodeExtraOptions(o);
    if (!st.ok()) return st;
    return ToStatus(spmx_set_decode_extra_options(h_, std::string(o.data(), o.size()).c_str()), h_);
  }
  util::Status SetVocabulary(const std::vector<absl::string_view> &valid_vocab) override {           // :279
    const util::Status st = SentencePieceProcessor::SetVocabulary(valid_vocab);
    if (!st.ok()) return st;
    std::vector<const char *> p;
    std::vector<uint64_t> l;
    for (const auto &v : valid_vocab) { p.push_back(v.data()); l.push_back(v.size()); }
    return ToStatus(spmx_set_vocabulary(h_, p.data(), l.data(), p.size()), h_);
  }
  util::Status ResetVocabulary() override {                                                          // :283
    const util::Status st = SentencePieceProcessor::ResetVocabulary();
    if (!st.ok()) return st;
    return ToStatus(spmx_reset_vocabulary(h_), h_);
  }
  // the path itself: Encode(input, vector<int>*) (:299-300, .cc:392-403) on the device
  util::Status Encode(absl::string_view input, std::vector<int> *ids) const override {
    util::Status st = status();                            // CHECK_OR_RETURN_STATUS_STL (.cc:364-370)
    if (st.ok()) st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    if (!ids) return util::Status(util::StatusCode::kInternal, "output container is null");
    ids->clear();
    uint64_t n = 0;
    ids->resize(input.size() + 8);
    int rc = spmx_encode(h_, input.data(), input.size(), ids->data(), ids->size(), &n);
    if (rc == 8 /* RESOURCE_EXHAUSTED: n says what it takes */) {
      ids->resize(n);
      rc = spmx_encode(h_, input.data(), input.size(), ids->data(), ids->size(), &n);
    }
    ids->resize(rc == 0 ? n : 0);
    return ToStatus(rc, h_);
  }
  // CalculateEntropy (:385-386, .cc:748-759) and the three virtual forms of SampleEncodeAndScore (ids :375-378, pieces
  // :369-372, NBestSentencePieceText* :410-412; .cc:497-546, :724-746) on the device.  The non-virtual wrappers of the base
  // class (SampleEncodeAndScoreAsIds / AsPieces / AsSerializedProto / AsImmutableProto, :489-501, :545-550, :590-595) call
  // these, so every form of the two calls runs on the device through a SentencePieceProcessor*.  A call takes the next
  // value of a per-process counter as its seed; the overloads with a seed make a draw reproducible.
  util::Status CalculateEntropy(absl::string_view input, float alpha, float *entropy) const override {
    util::Status st = status();
    if (st.ok()) st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    if (!entropy) return util::Status(util::StatusCode::kInternal, "output container is null");
    const uint64_t offs[2] = {0, input.size()};
    float *e = nullptr;
    const int rc = spmx_calculate_entropy_batch(h_, input.data() ? input.data() : "", offs, 1, alpha, &e);
    if (rc == 0) *entropy = e[0];
    spmx_free(e);
    return ToStatus(rc, h_);
  }
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best,
                                    std::vector<std::pair<std::vector<int>, float>> *ids) const override {
    return SampleEncodeAndScore(input, num_samples, alpha, wor, include_best, NextScoreSeed(), ids);
  }
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best, uint64_t seed,
                                    std::vector<std::pair<std::vector<int>, float>> *ids) const {
    util::Status st = status();
    if (st.ok()) st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    if (!ids) return util::Status(util::StatusCode::kInternal, "output container is null");
    ids->clear();
    const uint64_t offs[2] = {0, input.size()};
    int32_t *i = nullptr;
    uint64_t *io = nullptr, *ro = nullptr;
    float *sc = nullptr;
    const int rc = spmx_sample_encode_and_score_batch(h_, input.data() ? input.data() : "", offs, 1, num_samples, alpha, wor, include_best,
                                                      seed, &i, &io, &sc, &ro);
    if (rc == 0)
      for (uint64_t r = ro[0]; r < ro[1]; ++r) ids->emplace_back(std::vector<int>(i + io[r], i + io[r + 1]), sc[r]);
    spmx_free(i); spmx_free(io); spmx_free(sc); spmx_free(ro);
    if (rc == 0 && ids->empty()) return util::Status(util::StatusCode::kInternal, "SampleEncodeAndScore returns empty result.");   // .cc:735
    return ToStatus(rc, h_);
  }
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best,
                                    NBestSentencePieceText *samples_spt) const override {
    return SampleEncodeAndScore(input, num_samples, alpha, wor, include_best, NextScoreSeed(), samples_spt);
  }
  // every result with its score and the pieces / surfaces / byte ranges PopulateSentencePieceText gives it (.cc:547-636): a
  // piece is its normalized text, the piece name for a byte-fallback piece and a bos / eos, unk_piece for an unknown token
  // under the `unk_piece` extra option (:1050-1058)
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best, uint64_t seed,
                                    NBestSentencePieceText *samples_spt) const {
    util::Status st = status();
    if (st.ok()) st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    if (!samples_spt) return util::Status(util::StatusCode::kInternal, "output proto is null");
    samples_spt->Clear();
    const uint64_t offs[2] = {0, input.size()};
    int32_t *ids = nullptr;
    uint64_t *io = nullptr, *ro = nullptr, *no = nullptr;
    float *sc = nullptr;
    uint32_t *b = nullptr, *e = nullptr, *nb = nullptr, *ne = nullptr;
    char *norm = nullptr;
    const char *txt = input.data() ? input.data() : "";
    int rc = spmx_sample_encode_and_score_batch_spans(h_, txt, offs, 1, num_samples, alpha, wor, include_best, seed, &ids, &io, &sc,
                                                      &ro, &b, &e, &nb, &ne);
    if (rc == 0) rc = spmx_normalize_batch(h_, txt, offs, 1, &norm, &no, nullptr);
    if (rc == 0) {
      for (uint64_t r = ro[0]; r < ro[1]; ++r) {
        SentencePieceText *spt = samples_spt->add_nbests();
        spt->set_score(sc[r]);
        spt->set_text(txt, input.size());
        for (uint64_t k = io[r]; k < io[r + 1]; ++k) {
          auto *p = spt->add_pieces();
          p->set_id(static_cast<uint32_t>(ids[k]));
          p->set_begin(b[k]);
          p->set_end(e[k]);
          const int type = spmx_piece_type(h_, ids[k]);
          if (type == 2 && unk_piece_option_) p->set_piece(IdToPiece(unk_id()));
          else if (type == 6 || type == 3) p->set_piece(IdToPiece(ids[k]));
          else p->set_piece(norm + nb[k], ne[k] - nb[k]);
          // `surface`: not on a bos / eos; of the byte pieces of one unknown character only on the last in text order
          bool has_surface = type != 3;
          if (type == 6) {
            const bool has_next = reverse_option_ ? k > io[r] : k + 1 < io[r + 1];
            const uint64_t nx = reverse_option_ ? k - 1 : k + 1;
            if (has_next && spmx_piece_type(h_, ids[nx]) == 6 && nb[nx] == nb[k]) has_surface = false;
          }
          if (has_surface) p->set_surface(txt + b[k], e[k] - b[k]);
        }
      }
    }
    const bool empty = rc == 0 && ro[1] == ro[0];
    spmx_free(ids); spmx_free(io); spmx_free(sc); spmx_free(ro); spmx_free(b); spmx_free(e); spmx_free(nb); spmx_free(ne);
    spmx_free(norm); spmx_free(no);
    if (empty) return util::Status(util::StatusCode::kInternal, "SampleEncodeAndScore returns empty result.");
    return ToStatus(rc, h_);
  }
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best,
                                    std::vector<std::pair<std::vector<std::string>, float>> *pieces) const override {
    return SampleEncodeAndScore(input, num_samples, alpha, wor, include_best, NextScoreSeed(), pieces);
  }
  util::Status SampleEncodeAndScore(absl::string_view input, int num_samples, float alpha, bool wor, bool include_best, uint64_t seed,
                                    std::vector<std::pair<std::vector<std::string>, float>> *pieces) const {
    if (!pieces) return util::Status(util::StatusCode::kInternal, "output container is null");
    pieces->clear();
    NBestSentencePieceText nb;
    const util::Status st = SampleEncodeAndScore(input, num_samples, alpha, wor, include_best, seed, &nb);
    if (!st.ok()) return st;
    for (const auto &spt : nb.nbests()) {
      pieces->emplace_back(std::vector<std::string>(), spt.score());
      for (const auto &p : spt.pieces()) pieces->back().first.push_back(p.piece());
    }
    return util::Status();
  }
  util::Status Decode(const std::vector<int> &ids, std::string *detokenized) const override {       // :311-312
    util::Status st = status();
    if (st.ok()) st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    if (!detokenized) return util::Status(util::StatusCode::kInternal, "output container is null");
    uint64_t n = 0;
    detokenized->resize(ids.size() * 8 + 16);
    int rc = spmx_decode(h_, ids.data(), ids.size(), &(*detokenized)[0], detokenized->size(), &n);
    if (rc == 8) {
      detokenized->resize(n);
      rc = spmx_decode(h_, ids.data(), ids.size(), &(*detokenized)[0], detokenized->size(), &n);
    }
    detokenized->resize(rc == 0 ? n : 0);
    return ToStatus(rc, h_);
  }
  // NEW: the batch form, element-wise Encode (sentencepiece.i:245-267): packed sentences in, CSR out (spmx_free)
  util::Status EncodeBatch(const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids, uint64_t **id_offsets) const {
    const util::Status st = SyncNormalizerSpec();
    if (!st.ok()) return st;
    return ToStatus(spmx_encode_batch(h_, text, offsets, n, ids, id_offsets), h_);
  }

 private:
  util::Status Create(const char *blob, size_t n) {
    spmx_destroy(h_);
    h_ = nullptr;
    const util::Status st = ToStatus(spmx_create(blob, n, device_, &h_), nullptr);
    if (st.ok()) pushed_.store(SpecBits(model_proto().normalizer_spec()), std::memory_order_release);
    return st;
  }
  // mutable_normalizer_spec() (:699) is not virtual and hands out the base class's own proto: an edit through it -- also
  // through a SentencePieceProcessor* -- is invisible here until the next call looks.  So every call on the path compares
  // the three switches with what the handle was last given and pushes a difference as ONE override: the edit is live at
  // the next Encode / Decode, as it is in the reference.  The edit itself (the header's "use at your own risk") is not to be
  // made while calls are in flight; the calls AFTER it may come from any number of threads at once, as the const methods
  // always may: the fast path is one acquire load and a compare, a thread that sees a difference takes the mutex, the first
  // one in pushes the override, and pushed_ changes only once the handle's new tables are in place -- so every other thread
  // either waits on the mutex and finds nothing left to do, or arrives later and reads tables that are complete.  No thread
  // encodes while the handle is being rebuilt.
  static int SpecBits(const NormalizerSpec &spec) {
    return (spec.add_dummy_prefix() ? 1 : 0) | (spec.remove_extra_whitespaces() ? 2 : 0) | (spec.escape_whitespaces() ? 4 : 0);
  }
  util::Status SyncNormalizerSpec() const {
    if (!h_) return util::Status();
    const int now = SpecBits(model_proto().normalizer_spec());
    if (now == pushed_.load(std::memory_order_acquire)) return util::Status();
    std::lock_guard<std::mutex> lock(push_mu_);
    if (now == pushed_.load(std::memory_order_relaxed)) return util::Status();      // another thread pushed it meanwhile
    static const char *const kFields[3] = {"add_dummy_prefix", "remove_extra_whitespaces", "escape_whitespaces"};
    const char *values[3] = {now & 1 ? "1" : "0", now & 2 ? "1" : "0", now & 4 ? "1" : "0"};
    const int rc = spmx_override_normalizer_spec(h_, kFields, values, nullptr, 3);
    if (rc != 0) return ToStatus(rc, h_);
    pushed_.store(now, std::memory_order_release);
    return util::Status();
  }
  static uint64_t NextScoreSeed() {
    static std::atomic<uint64_t> calls{std::random_device{}()};   // (the reference seeds from std::random_device, src/util.cc:202-204)
    return ++calls;
  }
  static util::Status ToStatus(int rc, const spmx_handle *h) {
    if (rc == 0) return util::Status();
    return util::Status(static_cast<util::StatusCode>(rc), spmx_last_error(h));
  }
  int device_ = 0;
  bool unk_piece_option_ = false;   // the `unk` / `unk_piece` encode extra option: piece strings only
  bool reverse_option_ = false;     // an odd number of `reverse` options: the pieces come out last first
  spmx_handle *h_ = nullptr;
  mutable std::atomic<int> pushed_{7};            // the switches last pushed to the handle (SpecBits)
  mutable std::mutex push_mu_;                    // one thread pushes a difference, the others wait for it
};

}  // namespace sentencepiece
#endif
