// Driver of scripts/make_lattice_score_golden.py: the compiled reference's CalculateEntropy and the result counts of its
// SampleEncodeAndScore without replacement, for tests/golden/lattice_scores.json.  Built against the reference's header
// and oracle/_ref/libspm_ref.so where the reference tree is; nothing of it is committed.
//
//   lattice_score_golden <model file> <case file>
//
// A case is one line, the sentence in hex (empty sentence: "-"):
//   E <theta> <hex>                              ->  E <entropy as float bits, hex>
//   C <num_samples> <include_best> <theta> <hex> ->  C <results, or -1 where the call fails> <status message>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sentencepiece_processor.h"

static std::string Unhex(const std::string &h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
  return out;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s model cases\n", argv[0]); return 2; }
  sentencepiece::SentencePieceProcessor sp;
  const auto st = sp.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  std::ifstream in(argv[2]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string kind, hex;
    ls >> kind;
    if (kind == "E") {
      float theta = 0.f;
      ls >> theta >> hex;
      float e = 0.f;
      const auto s = sp.CalculateEntropy(Unhex(hex), theta, &e);
      if (!s.ok()) { fprintf(stderr, "%s\n", s.ToString().c_str()); return 1; }
      uint32_t bits;
      memcpy(&bits, &e, 4);
      printf("E %08x\n", bits);
    } else if (kind == "C") {
      int num = 0, best = 0;
      float theta = 0.f;
      ls >> num >> best >> theta >> hex;
      std::vector<std::pair<std::vector<int>, float>> res;
      const auto s = sp.SampleEncodeAndScore(Unhex(hex), num, theta, true, best != 0, &res);
      if (s.ok()) printf("C %d ok\n", static_cast<int>(res.size()));
      else printf("C -1 %s\n", s.error_message());
    } else if (!kind.empty()) {
      fprintf(stderr, "bad case line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
