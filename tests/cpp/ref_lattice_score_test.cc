// TEST: the CalculateEntropy / SampleEncodeAndScore overrides of include/spmx_reference_binding.h, compiled against the
// reference's own header and objects and driven through a sentencepiece::SentencePieceProcessor*, against the C ABI
// (spmx_calculate_entropy_batch, spmx_sample_encode_and_score_batch) with a fixed seed: the same floats bit for bit, the
// same ids, the pieces and the proto of the same results -- and the base class's non-virtual wrappers land on the device.
//   ref_lattice_score_test <model>
// exit 0 and "OK <checks>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "spmx_reference_binding.h"

static int g_checks = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static uint32_t Bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model\n", argv[0]); return 2; }
  namespace spm = sentencepiece;
  spm::SentencePieceProcessor base;
  std::unique_ptr<spm::SentencePieceProcessor> owner(new spm::AmdSentencePieceProcessor(0));
  spm::SentencePieceProcessor *sp = owner.get();                  // the virtual calls below go through the base-class pointer
  const auto *amd = static_cast<const spm::AmdSentencePieceProcessor *>(sp);   // (its overloads with a seed)
  CHECK(base.Load(argv[1]).ok() && sp->Load(argv[1]).ok());
  spmx_handle *h = nullptr;
  CHECK(spmx_create_from_file(argv[1], 0, &h) == 0);
  const std::vector<std::string> sents = {"hello world", "in the end it was a test", "a", ""};
  const uint64_t seed = 987654321;

  for (const std::string &s : sents) {
    const uint64_t offs[2] = {0, s.size()};
    // ---- CalculateEntropy: the C ABI's bits, and the reference's number from the host cores within the device bound ----
    for (float alpha : {0.f, 0.5f, 2.f}) {
      float *want = nullptr, got = 7.f, ref = 7.f;
      CHECK(spmx_calculate_entropy_batch(h, s.data(), offs, 1, alpha, &want) == 0);
      CHECK(sp->CalculateEntropy(s, alpha, &got).ok() && Bits(got) == Bits(want[0]));
      CHECK(Bits(sp->CalculateEntropy(s, alpha)) == Bits(want[0]));                     // the non-virtual wrapper (:519-521)
      CHECK(base.CalculateEntropy(s, alpha, &ref).ok() && std::fabs(got - ref) <= 2e-4f * std::fabs(ref) + 1e-6f);   // (tests/test_entropy.py's bound)
      spmx_free(want);
    }
    // ---- SampleEncodeAndScore: with replacement, without, with the best path ----
    const int modes[3][2] = {{0, 0}, {1, 0}, {1, 1}};
    for (const auto &m : modes) {
      const bool wor = m[0] != 0, best = m[1] != 0;
      int32_t *ids = nullptr;
      uint64_t *io = nullptr, *ro = nullptr;
      float *sc = nullptr;
      CHECK(spmx_sample_encode_and_score_batch(h, s.data(), offs, 1, 3, 0.5f, wor, best, seed, &ids, &io, &sc, &ro) == 0);
      std::vector<std::pair<std::vector<int>, float>> got;
      std::vector<std::pair<std::vector<std::string>, float>> pcs;
      spm::NBestSentencePieceText spt;
      const auto st = amd->SampleEncodeAndScore(s, 3, 0.5f, wor, best, seed, &got);
      const auto st2 = amd->SampleEncodeAndScore(s, 3, 0.5f, wor, best, seed, &pcs);
      const auto st3 = amd->SampleEncodeAndScore(s, 3, 0.5f, wor, best, seed, &spt);
      // the virtuals (a seed of their own): the same status and number of results
      std::vector<std::pair<std::vector<int>, float>> v_ids;
      std::vector<std::pair<std::vector<std::string>, float>> v_pcs;
      spm::NBestSentencePieceText v_spt;
      const auto v1 = sp->SampleEncodeAndScore(s, 3, 0.5f, wor, best, &v_ids);
      const auto v2 = sp->SampleEncodeAndScore(s, 3, 0.5f, wor, best, &v_pcs);
      const auto v3 = sp->SampleEncodeAndScore(s, 3, 0.5f, wor, best, &v_spt);
      if (ro[1] == 0) {                                          // sentencepiece_processor.cc:735
        CHECK(!st.ok() && !st2.ok() && !st3.ok() && !v1.ok() && !v2.ok() && !v3.ok());
        CHECK(st.code() == spm::util::StatusCode::kInternal && got.empty() && pcs.empty() && spt.nbests_size() == 0);
        CHECK(std::string(st.error_message()).find("SampleEncodeAndScore returns empty result.") != std::string::npos);
      } else {
        CHECK(st.ok() && st2.ok() && st3.ok() && v1.ok() && v2.ok() && v3.ok());
        CHECK(got.size() == ro[1] && pcs.size() == ro[1] && static_cast<uint64_t>(spt.nbests_size()) == ro[1]);
        CHECK(v_ids.size() == ro[1] && v_pcs.size() == ro[1] && static_cast<uint64_t>(v_spt.nbests_size()) == ro[1]);
        for (uint64_t r = 0; r < ro[1]; ++r) {
          CHECK(got[r].first == std::vector<int>(ids + io[r], ids + io[r + 1]) && Bits(got[r].second) == Bits(sc[r]));
          CHECK(Bits(pcs[r].second) == Bits(sc[r]) && pcs[r].first.size() == got[r].first.size());
          const auto &t = spt.nbests(static_cast<int>(r));
          CHECK(Bits(t.score()) == Bits(sc[r]) && t.text() == s && static_cast<size_t>(t.pieces_size()) == got[r].first.size());
          std::string joined;
          for (size_t k = 0; k < got[r].first.size(); ++k) {
            const auto &p = t.pieces(static_cast<int>(k));
            CHECK(static_cast<int>(p.id()) == got[r].first[k] && p.piece() == pcs[r].first[k] && p.piece() == sp->IdToPiece(got[r].first[k]));
            CHECK(p.surface() == s.substr(p.begin(), p.end() - p.begin()));
            joined += p.surface();
          }
          CHECK(joined == s);
          // the path is one of the reference's own segmentations: its pieces decode to the sentence
          std::string back;
          CHECK(base.Decode(got[r].first, &back).ok() && back == s);
        }
        if (best) {
          std::vector<int> enc;
          CHECK(base.Encode(s, &enc).ok() && got[0].first == enc && got[0].second == 0.f);
        }
        // the base class's non-virtual wrappers (:489-501, :545-550) run the overrides
        CHECK(sp->SampleEncodeAndScoreAsIds(s, 3, 0.5f, wor, best).size() == ro[1]);
        CHECK(sp->SampleEncodeAndScoreAsPieces(s, 3, 0.5f, wor, best).size() == ro[1]);
        spm::NBestSentencePieceText parsed;
        CHECK(parsed.ParseFromString(sp->SampleEncodeAndScoreAsSerializedProto(s, 3, 0.5f, wor, best)));
        CHECK(static_cast<uint64_t>(parsed.nbests_size()) == ro[1]);
      }
      spmx_free(ids); spmx_free(io); spmx_free(sc); spmx_free(ro);
    }
  }
  // "a" has two paths: three samples without replacement are ONE result here, which no run of the host reference's call
  // with its own generator can tell from the device's -- but two calls with one seed draw the same, and the extra options
  // reach the device: bos / eos around every result
  std::vector<std::pair<std::vector<int>, float>> plain, extra;
  CHECK(amd->SampleEncodeAndScore(sents[1], 3, 0.5f, true, false, seed, &plain).ok());
  CHECK(sp->SetEncodeExtraOptions("bos:eos").ok());
  CHECK(amd->SampleEncodeAndScore(sents[1], 3, 0.5f, true, false, seed, &extra).ok() && extra.size() == plain.size());
  for (size_t r = 0; r < plain.size(); ++r) {
    std::vector<int> want = plain[r].first;
    want.insert(want.begin(), sp->bos_id());
    want.push_back(sp->eos_id());
    CHECK(extra[r].first == want && Bits(extra[r].second) == Bits(plain[r].second));
  }
  std::vector<std::pair<std::vector<int>, float>> none;
  CHECK(!sp->SampleEncodeAndScore("hello", 3, 0.5f, false, true, &none).ok());          // include_best without wor
  CHECK(!sp->SampleEncodeAndScore("hello", 0, 0.5f, false, false, &none).ok());
  spmx_destroy(h);
  printf("OK %d\n", g_checks);
  return 0;
}
