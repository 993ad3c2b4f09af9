// Decode to SentencePieceText through include/spmx_processor.h, the way a C++ caller of the reference would:
// DecodeIdsAsSerializedProto / DecodePiecesAsSerializedProto through a base-class pointer (the methods are virtual, as the
// reference's are) and Decode(ids | pieces, SentencePieceText*), against the expected bytes of a rows file:
//   I <hex proto> <id>...          P <hex proto> <hex piece | ->...
// Prints "ok N" after N matching rows.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/spmx_processor.h"

namespace sentencepiece = sentencepiece_amd;

static std::string Hex(const std::string &b) {
  static const char *d = "0123456789abcdef";
  std::string o;
  for (unsigned char c : b) { o.push_back(d[c >> 4]); o.push_back(d[c & 15]); }
  return o;
}
static std::string Unhex(const std::string &h) {
  std::string o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
  return o;
}

struct Derived : sentencepiece::SentencePieceProcessor {};

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: decode_spans_test MODEL ROWS\n"); return 2; }
  Derived derived;
  sentencepiece::SentencePieceProcessor *sp = &derived;
  const sentencepiece::util::Status st = sp->Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "%s\n", st.ToString().c_str()); return 1; }
  std::ifstream f(argv[2], std::ios::binary);
  int n = 0;
  for (std::string line; std::getline(f, line);) {
    std::istringstream ss(line);
    std::string tag, want, cell;
    ss >> tag >> want;
    std::string got;
    sentencepiece::SentencePieceText spt;
    if (tag == "I") {
      std::vector<int> ids;
      while (ss >> cell) ids.push_back(std::stoi(cell));
      got = sp->DecodeIdsAsSerializedProto(ids);
      if (!sp->Decode(ids, &spt).ok()) { fprintf(stderr, "row %d: Decode(ids, spt) failed\n", n); return 1; }
      std::string text;
      if (!sp->Decode(ids, &text).ok() || text != spt.text) { fprintf(stderr, "row %d: text differs from Decode(ids, &string)\n", n); return 1; }
    } else {
      std::vector<std::string> pieces;
      while (ss >> cell) pieces.push_back(Unhex(cell));
      got = sp->DecodePiecesAsSerializedProto(pieces);
      std::vector<std::string_view> views(pieces.begin(), pieces.end());
      if (sp->DecodePiecesAsSerializedProto(views) != got) { fprintf(stderr, "row %d: the string_view form differs\n", n); return 1; }
      if (!sp->Decode(pieces, &spt).ok()) { fprintf(stderr, "row %d: Decode(pieces, spt) failed\n", n); return 1; }
    }
    if (Hex(got) != want) { fprintf(stderr, "row %d (%s): got %s\nwant %s\n", n, tag.c_str(), Hex(got).c_str(), want.c_str()); return 1; }
    if (spt.SerializeAsString() != got) { fprintf(stderr, "row %d: Decode(..., spt) differs from the serialized form\n", n); return 1; }
    uint32_t pos = 0;
    for (const auto &p : spt.pieces) {
      if (p.begin != pos || p.end != p.begin + p.surface.size()) { fprintf(stderr, "row %d: spans do not tile the text\n", n); return 1; }
      pos = p.end;
    }
    ++n;
  }
  // an id out of range: kOutOfRange "Invalid id: N", and the serialized form swallows it
  sentencepiece::SentencePieceText spt;
  const sentencepiece::util::Status bad = sp->Decode(std::vector<int>{1, sp->GetPieceSize()}, &spt);
  if (bad.ok() || bad.code() != sentencepiece::util::StatusCode::kOutOfRange || bad.ToString().find("Invalid id") == std::string::npos) {
    fprintf(stderr, "expected kOutOfRange Invalid id, got %s\n", bad.ToString().c_str());
    return 1;
  }
  if (!sp->DecodeIdsAsSerializedProto(std::vector<int>{-1}).empty()) { fprintf(stderr, "a bad id must give an empty string\n"); return 1; }
  printf("ok %d\n", n);
  return 0;
}
