// Driver of scripts/make_estep_golden.py: the compiled reference's E-step of one sentence -- Lattice::PopulateMarginal and the
// size of Lattice::Viterbi()'s path over the lattice of Model::PopulateNodes -- for tests/golden/expected_counts.npz.  Built
// against the reference's headers and oracle/_ref/libspm_ref.so where the reference tree is; nothing of it is committed.
//
//   estep_golden <model file> <case file>
//
// A case is one line, the sentence in hex (empty sentence: "-"):
//   M <freq> <hex>   ->  M <Z as float bits, hex (of freq 1)> <nodes on the Viterbi path> <k> then k times " <id>:<float bits, hex>",
//                        the non-zero entries of `expected` after PopulateMarginal(freq, &expected) on zeros
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sentencepiece_processor.h"
#include "unigram_model.h"

static std::string Unhex(const std::string &h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
  return out;
}

static uint32_t Bits(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s model cases\n", argv[0]); return 2; }
  sentencepiece::SentencePieceProcessor sp;
  const auto st = sp.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  const sentencepiece::unigram::Model model(sp.model_proto());
  const size_t V = static_cast<size_t>(sp.GetPieceSize());
  std::ifstream in(argv[2]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string kind, hex;
    ls >> kind;
    if (kind == "M") {
      double freq = 1.0;
      ls >> freq >> hex;
      std::string norm;
      const auto s = sp.Normalize(Unhex(hex), &norm);
      if (!s.ok()) { fprintf(stderr, "%s\n", s.ToString().c_str()); return 1; }
      sentencepiece::unigram::Lattice lattice;
      lattice.SetSentence(norm);
      model.PopulateNodes(&lattice);
      std::vector<float> one(V, 0.f), e(V, 0.f);
      const float Z = lattice.PopulateMarginal(1.0f, &one);
      lattice.PopulateMarginal(static_cast<float>(freq), &e);
      const size_t nodes = lattice.Viterbi().first.size();
      size_t k = 0;
      for (size_t i = 0; i < V; ++i) k += e[i] != 0.f;
      printf("M %08x %zu %zu", Bits(Z), nodes, k);
      for (size_t i = 0; i < V; ++i)
        if (e[i] != 0.f) printf(" %zu:%08x", i, Bits(e[i]));
      printf("\n");
    } else if (!kind.empty()) {
      fprintf(stderr, "bad case line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
