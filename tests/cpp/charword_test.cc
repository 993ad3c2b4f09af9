// A C++ caller of include/spmx_processor.h on a character or word model: Load, Encode per line and EncodeBatch over
// all lines (ids printed one line per sentence, Decode of them checked against Decode of the batch's), then the calls
// the reference refuses for these models (LoadVocabulary too, when a vocabulary file is given), one line each:
// "R <name> <code>|<message>".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/spmx_processor.h"

namespace sentencepiece = sentencepiece_amd;

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: charword_test MODEL TEXTFILE [VOCABFILE]\n"); return 2; }
  sentencepiece::SentencePieceProcessor sp;
  const sentencepiece::util::Status st = sp.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  std::ifstream f(argv[2], std::ios::binary);
  std::vector<std::string> lines;
  for (std::string line; std::getline(f, line);) lines.push_back(line);
  std::vector<std::string_view> views(lines.begin(), lines.end());
  std::vector<std::vector<int>> batch;
  if (!sp.EncodeBatch(views, &batch).ok() || batch.size() != lines.size()) { fprintf(stderr, "EncodeBatch failed\n"); return 1; }
  for (size_t i = 0; i < lines.size(); ++i) {
    if (i % 7 == 0) {
      std::vector<int> one;
      std::string t1, t2;
      if (!sp.Encode(lines[i], &one).ok() || one != batch[i]) { fprintf(stderr, "Encode != EncodeBatch at line %zu\n", i); return 1; }
      if (!sp.Decode(one, &t1).ok() || !sp.Decode(batch[i], &t2).ok() || t1 != t2) { fprintf(stderr, "Decode at line %zu\n", i); return 1; }
    }
    for (size_t k = 0; k < batch[i].size(); ++k) std::cout << (k ? " " : "") << batch[i][k];
    std::cout << "\n";
  }
  auto report = [](const char *name, const sentencepiece::util::Status &s) {
    std::cout << "R " << name << " " << static_cast<int>(s.code()) << "|" << s.error_message() << "\n";
  };
  std::vector<std::vector<int>> nbest;
  std::vector<int> drawn;
  report("nbest", sp.NBestEncode("hello world", 3, &nbest));
  report("sample", sp.SampleEncode("hello world", -1, 0.1f, &drawn));
  report("set_vocabulary", sp.SetVocabulary({"a", "b"}));
  if (argc > 3) report("load_vocabulary", sp.LoadVocabulary(argv[3], 1));   // ("<token> TAB <freq>" lines; it ends in SetVocabulary)
  std::vector<int> after;
  if (!lines.empty() && (!sp.Encode(lines[0], &after).ok() || after != batch[0])) { fprintf(stderr, "the handle after the refusals\n"); return 1; }
  return 0;
}
