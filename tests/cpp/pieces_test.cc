// TEST ONLY: EncodeAsPieces / Encode(input, std::vector<std::string>*) / EncodeAsPiecesBatch of include/spmx_processor.h.
//   pieces_test MODEL INPUT [extra options]
// Prints the pieces of every line of INPUT joined with ' ' (the batch form); the single-sentence forms must agree with it
// on the first 40 lines and on a few inputs of their own.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/spmx_processor.h"

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: pieces_test MODEL INPUT [extra options]\n"); return 2; }
  sentencepiece_amd::SentencePieceProcessor sp;
  auto st = sp.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  if (argc > 3) {
    st = sp.SetEncodeExtraOptions(argv[3]);
    if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  }
  std::vector<std::string> lines;
  std::ifstream in(argv[2]);
  for (std::string line; std::getline(in, line);) lines.push_back(line);
  std::vector<std::string_view> views(lines.begin(), lines.end());
  std::vector<std::vector<std::string>> rows;
  st = sp.EncodeAsPiecesBatch(views, &rows);
  if (!st.ok() || rows.size() != lines.size()) { fprintf(stderr, "EncodeAsPiecesBatch: %s\n", st.ToString().c_str()); return 1; }
  for (size_t i = 0; i < lines.size() && i < 40; ++i) {
    std::vector<std::string> one;
    st = sp.Encode(lines[i], &one);
    if (!st.ok() || one != rows[i] || sp.EncodeAsPieces(lines[i]) != rows[i]) { fprintf(stderr, "line %zu differs\n", i); return 1; }
  }
  if (argc <= 3 && (!sp.EncodeAsPieces("").empty() || !sp.EncodeAsPieces("   ").empty())) { fprintf(stderr, "empty input\n"); return 1; }
  if (sp.Encode("x", static_cast<std::vector<std::string> *>(nullptr)).ok()) { fprintf(stderr, "null container\n"); return 1; }
  st = sp.EncodeAsPiecesBatch({}, &rows);
  if (!st.ok() || !rows.empty()) { fprintf(stderr, "empty batch\n"); return 1; }
  st = sp.EncodeAsPiecesBatch(views, &rows);
  for (const auto &row : rows) {
    for (size_t k = 0; k < row.size(); ++k) printf("%s%s", k ? " " : "", row[k].c_str());
    printf("\n");
  }
  return 0;
}
