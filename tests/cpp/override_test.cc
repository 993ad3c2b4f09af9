// TEST: the normalizer_spec mutators of include/spmx_processor.h -- mutable_normalizer_spec()->set_*() and
// OverrideNormalizerSpec(map) -- on one loaded processor.
//   override_test <model> <text file> <proto out>
// Prints sections: a line "== <label> <add_dummy_prefix> <remove_extra_whitespaces> <escape_whitespaces>" followed by
// the ids of every line of the text file under the spec of that moment, one line each; "E <code>|<message>" after a
// failing call.  <proto out> receives serialized_model_proto() as it is at the end.  tests/test_normalizer_override.py
// compares every section with the oracle loaded from the equally edited ModelProto.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "spmx_processor.h"

namespace spm = sentencepiece_amd;

static std::vector<std::string> g_lines;

static void Section(spm::SentencePieceProcessor *sp, const char *label) {
  const spm::NormalizerSpec *spec = sp->mutable_normalizer_spec();
  printf("== %s %d %d %d\n", label, spec->add_dummy_prefix(), spec->remove_extra_whitespaces(), spec->escape_whitespaces());
  for (const std::string &line : g_lines) {
    std::vector<int> ids;
    const auto st = sp->Encode(line, &ids);
    if (!st.ok()) { fprintf(stderr, "Encode: %s\n", st.ToString().c_str()); exit(1); }
    for (size_t k = 0; k < ids.size(); ++k) printf(k ? " %d" : "%d", ids[k]);
    printf("\n");
  }
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s model text proto-out\n", argv[0]); return 2; }
  spm::SentencePieceProcessor sp;
  if (sp.mutable_normalizer_spec() != nullptr) { fprintf(stderr, "a spec before Load\n"); return 1; }   // as the reference
  auto st = sp.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "Load: %s\n", st.ToString().c_str()); return 1; }
  std::ifstream in(argv[2]);
  for (std::string line; std::getline(in, line);) g_lines.push_back(line);
  spm::NormalizerSpec *spec = sp.mutable_normalizer_spec();
  if (!spec) { fprintf(stderr, "no spec after Load\n"); return 1; }
  Section(&sp, "loaded");
  spec->set_add_dummy_prefix(!spec->add_dummy_prefix());
  if (spec->last_code() != 0) { fprintf(stderr, "set_add_dummy_prefix: %d\n", spec->last_code()); return 1; }
  Section(&sp, "set_add_dummy_prefix");
  spec->set_escape_whitespaces(!spec->escape_whitespaces());
  spec->set_remove_extra_whitespaces(!spec->remove_extra_whitespaces());
  Section(&sp, "set_escape_and_remove");
  st = sp.OverrideNormalizerSpec({{"add_dummy_prefix", "TRUE"}, {"escape_whitespaces", "y"}, {"remove_extra_whitespaces", ""}});
  if (!st.ok()) { fprintf(stderr, "OverrideNormalizerSpec: %s\n", st.ToString().c_str()); return 1; }
  Section(&sp, "override_all_true");
  spec->set_name("identity");
  spec->set_normalization_rule_tsv("rules.tsv");
  Section(&sp, "name_and_tsv");
  st = sp.OverrideNormalizerSpec({{"no_such_field", "1"}});
  printf("E %d|%s\n", static_cast<int>(st.code()), st.error_message());
  st = sp.OverrideNormalizerSpec({{"escape_whitespaces", "perhaps"}});
  printf("E %d|%s\n", static_cast<int>(st.code()), st.error_message());
  Section(&sp, "after_errors");
  const std::string blob = sp.serialized_model_proto();
  std::ofstream out(argv[3], std::ios::binary);
  out.write(blob.data(), static_cast<std::streamsize>(blob.size()));
  return out.good() ? 0 : 1;
}
