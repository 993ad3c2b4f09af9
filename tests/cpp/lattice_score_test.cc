// The facade's CalculateEntropy / SampleEncodeAndScore overloads (include/spmx_processor.h) against the C ABI
// (include/spmx.h) on one small batch: the same floats bit for bit, the same ids, the pieces and the serialized proto of
// the same results.  Prints "OK <checks>" or the first disagreement.
//
//   lattice_score_test MODEL
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spmx_processor.h"

namespace sp = sentencepiece_amd;

static int g_checks = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static uint32_t Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: lattice_score_test MODEL\n"); return 2; }
  struct Sub : sp::SentencePieceProcessor {};                    // through a base-class pointer: the methods are virtual
  Sub sub;
  sp::SentencePieceProcessor *p = &sub;
  if (!p->Load(argv[1]).ok()) { fprintf(stderr, "cannot load %s\n", argv[1]); return 1; }
  spmx_handle *h = nullptr;
  if (spmx_create_from_file(argv[1], 0, &h) != 0) { fprintf(stderr, "spmx_create_from_file failed\n"); return 1; }
  const std::vector<std::string> sents = {"hello world", "in the end it was a test", "a", ""};
  std::string text;
  std::vector<uint64_t> offs{0};
  for (const std::string &s : sents) { text += s; offs.push_back(text.size()); }
  const uint64_t n = sents.size();
  const uint64_t seed = 12345;

  // ---- CalculateEntropy ----
  for (float alpha : {0.f, 0.5f, 2.f}) {
    float *want = nullptr;
    CHECK(spmx_calculate_entropy_batch(h, text.data(), offs.data(), n, alpha, &want) == 0);
    std::vector<float> flat;
    CHECK(p->CalculateEntropyBatchFlat(text.data(), offs.data(), n, alpha, &flat).ok() && flat.size() == n);
    for (uint64_t i = 0; i < n; ++i) {
      float e = 7.f;
      CHECK(p->CalculateEntropy(sents[i], alpha, &e).ok());
      CHECK(Bits(e) == Bits(want[i]) && Bits(flat[i]) == Bits(want[i]) && Bits(p->CalculateEntropy(sents[i], alpha)) == Bits(want[i]));
    }
    CHECK(Bits(want[3]) == 0x80000000u);                         // the empty sentence: -0.0
    spmx_free(want);
  }

  // ---- SampleEncodeAndScore: with replacement, without, with the best path ----
  const int modes[3][2] = {{0, 0}, {1, 0}, {1, 1}};
  for (const auto &m : modes) {
    const bool wor = m[0] != 0, best = m[1] != 0;
    // the batch form
    int32_t *ids = nullptr;
    uint64_t *io = nullptr, *ro = nullptr;
    float *sc = nullptr;
    CHECK(spmx_sample_encode_and_score_batch(h, text.data(), offs.data(), n, 3, 0.5f, wor, best, seed, &ids, &io, &sc, &ro) == 0);
    std::vector<int32_t> f_ids;
    std::vector<uint64_t> f_io, f_ro;
    std::vector<float> f_sc;
    CHECK(p->SampleEncodeAndScoreBatchFlat(text.data(), offs.data(), n, 3, 0.5f, wor, best, seed, &f_ids, &f_io, &f_sc, &f_ro).ok());
    CHECK(f_ro == std::vector<uint64_t>(ro, ro + n + 1) && f_io == std::vector<uint64_t>(io, io + ro[n] + 1));
    CHECK(f_ids == std::vector<int32_t>(ids, ids + io[ro[n]]));
    for (uint64_t r = 0; r < ro[n]; ++r) CHECK(Bits(f_sc[r]) == Bits(sc[r]));
    CHECK(ro[4] == ro[3]);                                       // the empty sentence owns no result
    CHECK(ro[1] - ro[0] == 3);
    spmx_free(ids); spmx_free(io); spmx_free(sc); spmx_free(ro);
    // one sentence at a time: the C ABI on that sentence alone, the same seed
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t o1[2] = {0, sents[i].size()};
      CHECK(spmx_sample_encode_and_score_batch(h, sents[i].data(), o1, 1, 3, 0.5f, wor, best, seed, &ids, &io, &sc, &ro) == 0);
      std::vector<std::pair<std::vector<int>, float>> got;
      const sp::util::Status st = p->SampleEncodeAndScore(sents[i], 3, 0.5f, wor, best, seed, &got);
      sp::NBestSentencePieceText spt;
      const sp::util::Status st2 = p->SampleEncodeAndScore(sents[i], 3, 0.5f, wor, best, seed, &spt);
      if (ro[1] == 0) {                                          // sentencepiece_processor.cc:735
        CHECK(!st.ok() && st.code() == sp::util::StatusCode::kInternal && got.empty() && !st2.ok() && spt.nbests.empty());
        CHECK(std::string(st.error_message()).find("SampleEncodeAndScore returns empty result.") != std::string::npos);
      } else {
        CHECK(st.ok() && st2.ok() && got.size() == ro[1] && spt.nbests.size() == ro[1]);
        for (uint64_t r = 0; r < ro[1]; ++r) {
          CHECK(got[r].first == std::vector<int>(ids + io[r], ids + io[r + 1]) && Bits(got[r].second) == Bits(sc[r]));
          CHECK(spt.nbests[r].has_score && Bits(spt.nbests[r].score) == Bits(sc[r]) && spt.nbests[r].text == sents[i]);
          CHECK(spt.nbests[r].pieces.size() == got[r].first.size());
          for (size_t k = 0; k < got[r].first.size(); ++k) {
            CHECK(static_cast<int>(spt.nbests[r].pieces[k].id) == got[r].first[k]);
            CHECK(spt.nbests[r].pieces[k].piece == p->IdToPiece(got[r].first[k]));
          }
        }
        if (best) CHECK(got[0].second == 0.f && got[0].first == p->EncodeAsIds(sents[i]));
        CHECK(!spt.SerializeAsString().empty());
      }
      spmx_free(ids); spmx_free(io); spmx_free(sc); spmx_free(ro);
    }
    // the overloads without a seed draw afresh and return the same number of results
    std::vector<std::pair<std::vector<int>, float>> a;
    std::vector<std::pair<std::vector<std::string>, float>> b;
    CHECK(p->SampleEncodeAndScore(sents[1], 3, 0.5f, wor, best, &a).ok() && p->SampleEncodeAndScore(sents[1], 3, 0.5f, wor, best, &b).ok());
    CHECK(a.size() == 3 && b.size() == 3 && !b[0].first.empty());
    CHECK(p->SampleEncodeAndScoreAsIds(sents[1], 3, 0.5f, wor, best).size() == 3 && p->SampleEncodeAndScoreAsPieces(sents[1], 3, 0.5f, wor, best).size() == 3);
    CHECK(!p->SampleEncodeAndScoreAsSerializedProto(sents[1], 3, 0.5f, wor, best).empty());
  }
  std::vector<std::pair<std::vector<int>, float>> none;
  CHECK(!p->SampleEncodeAndScore("hello", 3, 0.5f, false, true, &none).ok());           // include_best without wor
  CHECK(!p->SampleEncodeAndScore("hello", 0, 0.5f, false, false, &none).ok());
  CHECK(!p->SampleEncodeAndScore("hello", 513, 0.5f, true, false, &none).ok());
  spmx_destroy(h);
  printf("OK %d\n", g_checks);
  return 0;
}
