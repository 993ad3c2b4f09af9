// TEST: normalizer_spec edits through include/spmx_reference_binding.h.  mutable_normalizer_spec() is not virtual in the
// reference (src/sentencepiece_processor.h:699), so the edit is made on the base class's own proto, through a
// sentencepiece::SentencePieceProcessor* that points at the subclass; the subclass has to notice it at its next call.
// An unmodified base-class processor gets the same edit and is the expectation, line by line.
//   ref_override_test <model> <text file>
// exit 0 and "OK <lines> <ids>" when every line's ids, Decode of them and the batch form agree under every edit, also
// when the first calls after an edit come from four threads at once.
#include <atomic>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "spmx_reference_binding.h"

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s model text\n", argv[0]); return 2; }
  sentencepiece::SentencePieceProcessor base;
  std::unique_ptr<sentencepiece::SentencePieceProcessor> amd(new sentencepiece::AmdSentencePieceProcessor(0));
  sentencepiece::SentencePieceProcessor *sp = amd.get();
  if (sp->mutable_normalizer_spec() != nullptr) { fprintf(stderr, "a spec before Load\n"); return 1; }
  auto st = base.Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "base.Load: %s\n", st.ToString().c_str()); return 1; }
  st = sp->Load(argv[1]);
  if (!st.ok()) { fprintf(stderr, "amd.Load: %s\n", st.ToString().c_str()); return 1; }
  std::ifstream in(argv[2]);
  std::vector<std::string> lines;
  std::string packed;
  std::vector<uint64_t> offs{0};
  for (std::string line; std::getline(in, line);) {
    lines.push_back(line);
    packed += line;
    offs.push_back(packed.size());
  }
  const bool a0 = base.mutable_normalizer_spec()->add_dummy_prefix(), r0 = base.mutable_normalizer_spec()->remove_extra_whitespaces(),
             e0 = base.mutable_normalizer_spec()->escape_whitespaces();
  // one switch, then the other two at once, then back to the loaded spec
  const bool steps[3][3] = {{!a0, r0, e0}, {!a0, !r0, !e0}, {a0, r0, e0}};
  size_t total = 0;
  for (const auto &s : steps) {
    for (sentencepiece::SentencePieceProcessor *p : {&base, sp}) {
      sentencepiece::NormalizerSpec *spec = p->mutable_normalizer_spec();
      spec->set_add_dummy_prefix(s[0]);
      spec->set_remove_extra_whitespaces(s[1]);
      spec->set_escape_whitespaces(s[2]);
    }
    std::vector<std::vector<int>> want;
    for (size_t i = 0; i < lines.size(); ++i) {
      std::vector<int> a, b;
      const auto s1 = base.Encode(lines[i], &a), s2 = sp->Encode(lines[i], &b);
      if (s1.ok() != s2.ok() || a != b) { fprintf(stderr, "spec %d%d%d line %zu: ids differ (%zu vs %zu)\n", s[0], s[1], s[2], i, a.size(), b.size()); return 1; }
      std::string t1, t2;
      if (!base.Decode(a, &t1).ok() || !sp->Decode(b, &t2).ok() || t1 != t2) { fprintf(stderr, "spec %d%d%d line %zu: Decode differs\n", s[0], s[1], s[2], i); return 1; }
      total += b.size();
      want.push_back(std::move(a));
    }
    int32_t *ids = nullptr;
    uint64_t *io = nullptr;
    st = static_cast<sentencepiece::AmdSentencePieceProcessor *>(sp)->EncodeBatch(packed.data(), offs.data(), lines.size(), &ids, &io);
    if (!st.ok()) { fprintf(stderr, "EncodeBatch: %s\n", st.ToString().c_str()); return 1; }
    for (size_t i = 0; i < lines.size(); ++i) {
      if (io[i + 1] - io[i] != want[i].size()) { fprintf(stderr, "EncodeBatch: line %zu has %llu ids, not %zu\n", i, (unsigned long long)(io[i + 1] - io[i]), want[i].size()); return 1; }
      for (size_t k = 0; k < want[i].size(); ++k)
        if (ids[io[i] + k] != want[i][k]) { fprintf(stderr, "EncodeBatch: line %zu id %zu differs\n", i, k); return 1; }
    }
    spmx_free(ids);
    spmx_free(io);
  }
  // an edit seen first by the batch form, and first by Decode
  base.mutable_normalizer_spec()->set_add_dummy_prefix(!a0);
  sp->mutable_normalizer_spec()->set_add_dummy_prefix(!a0);
  {
    int32_t *ids = nullptr;
    uint64_t *io = nullptr;
    st = static_cast<sentencepiece::AmdSentencePieceProcessor *>(sp)->EncodeBatch(packed.data(), offs.data(), lines.size(), &ids, &io);
    if (!st.ok()) { fprintf(stderr, "EncodeBatch: %s\n", st.ToString().c_str()); return 1; }
    for (size_t i = 0; i < lines.size(); ++i) {
      std::vector<int> a;
      (void)base.Encode(lines[i], &a);
      if (io[i + 1] - io[i] != a.size()) { fprintf(stderr, "EncodeBatch after an edit: line %zu differs\n", i); return 1; }
      for (size_t k = 0; k < a.size(); ++k)
        if (ids[io[i] + k] != a[k]) { fprintf(stderr, "EncodeBatch after an edit: line %zu id %zu differs\n", i, k); return 1; }
    }
    spmx_free(ids);
    spmx_free(io);
  }
  base.mutable_normalizer_spec()->set_add_dummy_prefix(a0);
  sp->mutable_normalizer_spec()->set_add_dummy_prefix(a0);
  if (!lines.empty()) {
    std::vector<int> a;
    (void)base.Encode(" " + lines[0], &a);
    std::string t1, t2;
    if (!base.Decode(a, &t1).ok() || !sp->Decode(a, &t2).ok() || t1 != t2) { fprintf(stderr, "Decode after an edit differs\n"); return 1; }
  }
  // the first calls after an edit, from four threads at once: the edit is made while nothing is in flight, then every
  // thread's first Encode finds it.  One of them pushes it to the handle, none encodes on half-swapped tables.
  for (int round = 0; round < 2; ++round) {
    const bool a = round == 0 ? !a0 : a0, e = round == 0 ? !e0 : e0;
    for (sentencepiece::SentencePieceProcessor *p : {&base, sp}) {
      p->mutable_normalizer_spec()->set_add_dummy_prefix(a);
      p->mutable_normalizer_spec()->set_escape_whitespaces(e);
    }
    std::vector<std::vector<int>> want(lines.size());
    for (size_t i = 0; i < lines.size(); ++i) (void)base.Encode(lines[i], &want[i]);
    std::atomic<int> ready{0}, bad{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < 4; ++t)
      threads.emplace_back([&, t]() {
        ready.fetch_add(1);
        while (ready.load() < 4) std::this_thread::yield();
        for (size_t i = t; i < lines.size(); i += 4) {
          std::vector<int> b;
          if (!sp->Encode(lines[i], &b).ok() || b != want[i]) bad.fetch_add(1);
        }
      });
    for (auto &th : threads) th.join();
    if (bad.load()) { fprintf(stderr, "threads, round %d: %d lines differ\n", round, bad.load()); return 1; }
  }
  printf("OK %zu %zu\n", lines.size(), total);
  return 0;
}
