// spmx_encode: the command line of the reference's spm_encode (src/spm_encode_main.cc) over the C ABI of include/spmx.h:
// file (or stdin) in; out one line of space-separated ids per input line (--output_format=id, the reference's bytes), one
// line of space-separated pieces (--output_format=piece, the reference's bytes for its default format), or flat binary
// ids (--output_format=bin).  The default here is id; the reference's is piece.  --output_format also takes the reference's
// other names: nbest_id / nbest_piece (one line per result of NBestEncode(line, --nbest_size)), sample_id / sample_piece
// (SampleEncode(line, --nbest_size, --alpha), the draws keyed by --random_seed and the line number), proto / sample_proto /
// nbest_proto (nothing is written, as in the reference).
//   spmx_encode --model=M [--input=F] [--output=F] [--output_format=id|piece|bin|nbest_id|nbest_piece|sample_id|sample_piece|...] [--nbest_size=10]
//               [--alpha=0.5] [--random_seed=N] [--extra_options=bos:eos] [--device=N]
//               [--vocabulary=F --vocabulary_threshold=N] [--generate_vocabulary [FILE ...]]
// --vocabulary / --vocabulary_threshold restrict the pieces before any mode (LoadVocabulary, :80-83).
// --generate_vocabulary (bare or =true|false) writes `piece TAB count` lines instead of a segmentation (:102-109,
// :167-172); --output_format is ignored then, and the inputs are --input=F or, without it, EVERY positional argument, the
// counts accumulating over the files.  The encoding modes take one input: --input=F or the first positional argument
// (further positional inputs are not supported there).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>
#include <unistd.h>

#include "../include/spmx.h"

int main(int argc, char **argv) {
  std::string model, input, output, format = "id", extra, vocabulary;
  std::vector<std::string> rest;
  int device = 0, vocabulary_threshold = 0, nbest_size = 10;     // (--nbest_size 10, --alpha 0.5: src/spm_encode_main.cc:50-52)
  float alpha = 0.5f;
  unsigned long long random_seed = ~0ull;                       // (the reference: "~0u" means the seed is not set)
  bool seed_set = false;
  bool generate = false;
  const char *usage = "usage: spmx_encode --model=M [--input=F] [--output=F] [--extra_options=..] [--device=N]\n"
                      "       [--output_format=id|piece|bin|nbest_id|nbest_piece|sample_id|sample_piece|proto|nbest_proto|sample_proto]\n"
                      "       [--nbest_size=10] [--alpha=0.5] [--random_seed=N]\n       "
                      "[--vocabulary=F --vocabulary_threshold=N] [--generate_vocabulary [FILE ...]]\n"
                      "       (several positional inputs only with --generate_vocabulary)\n";
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&](const char *name, std::string *dst) {
      const std::string k = std::string("--") + name + "=";
      if (a.compare(0, k.size(), k) == 0) { *dst = a.substr(k.size()); return true; }
      return false;
    };
    std::string dev, flag;
    if (a == "--generate_vocabulary") { generate = true; continue; }
    if (val("generate_vocabulary", &flag)) {
      if (flag == "true" || flag == "1") generate = true;
      else if (flag == "false" || flag == "0") generate = false;
      else { fprintf(stderr, "--generate_vocabulary takes true or false\n%s", usage); return 2; }
      continue;
    }
    if (val("vocabulary", &vocabulary)) continue;
    if (val("vocabulary_threshold", &flag)) { vocabulary_threshold = atoi(flag.c_str()); continue; }
    if (val("nbest_size", &flag)) { nbest_size = atoi(flag.c_str()); continue; }
    if (val("alpha", &flag)) { alpha = static_cast<float>(atof(flag.c_str())); continue; }
    if (val("random_seed", &flag)) { random_seed = strtoull(flag.c_str(), nullptr, 10); seed_set = true; continue; }
    if (val("model", &model) || val("input", &input) || val("output", &output) || val("output_format", &format) ||
        val("extra_options", &extra)) continue;
    if (val("device", &dev)) { device = atoi(dev.c_str()); continue; }
    if (!a.empty() && a[0] != '-') { rest.push_back(a); continue; }
    fprintf(stderr, "unknown argument: %s\n", a.c_str());
    return 2;
  }
  if (model.empty()) { fprintf(stderr, "%s", usage); return 2; }
  if (!generate) {                                     // one input: --input, else the first positional argument
    const size_t used = input.empty() ? 1 : 0;
    if (rest.size() > used) { fprintf(stderr, "unknown argument: %s\n", rest[used].c_str()); return 2; }
    if (input.empty() && !rest.empty()) input = rest[0];
  }
  spmx_handle *h = nullptr;
  if (spmx_create_from_file(model.c_str(), device, &h) != 0) { fprintf(stderr, "%s\n", spmx_last_error(nullptr)); return 1; }
  if (!extra.empty() && spmx_set_encode_extra_options(h, extra.c_str()) != 0) { fprintf(stderr, "%s\n", spmx_last_error(h)); return 1; }
  if (!vocabulary.empty() && spmx_load_vocabulary(h, vocabulary.c_str(), vocabulary_threshold) != 0) { fprintf(stderr, "%s\n", spmx_last_error(h)); return 1; }
  // stdin / stdout go through temporary files: the library maps its input
  std::string in_path = input, out_path = output;
  char tin[] = "/tmp/spmx_encode_in_XXXXXX", tout[] = "/tmp/spmx_encode_out_XXXXXX";
  if (generate && !input.empty()) rest.assign(1, input);      // (the reference: --input wins over the positional arguments)
  const bool from_stdin = generate ? rest.empty() : in_path.empty();
  if (from_stdin) {
    const int fd = mkstemp(tin);
    if (fd < 0) { perror("mkstemp"); return 1; }
    FILE *f = fdopen(fd, "wb");
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), stdin)) > 0) fwrite(buf, 1, n, f);
    fclose(f);
    in_path = tin;
  }
  if (out_path.empty()) { const int fd = mkstemp(tout); if (fd < 0) { perror("mkstemp"); return 1; } close(fd); out_path = tout; }
  uint64_t ns = 0, ni = 0;
  int rc = 0;
  if (generate) {
    if (rest.empty()) rest.push_back(in_path);
    std::vector<uint64_t> counts(static_cast<size_t>(spmx_piece_size(h)) + 1, 0);
    for (size_t k = 0; k < rest.size() && rc == 0; ++k) {
      uint64_t s1 = 0, i1 = 0;
      rc = spmx_count_file(h, rest[k].c_str(), counts.data(), &s1, &i1);
      ns += s1;
      ni += i1;
    }
    if (rc == 0) rc = spmx_write_vocabulary(h, counts.data(), out_path.c_str(), nullptr);
  } else {
    if (!seed_set) random_seed = static_cast<unsigned long long>(getpid()) * 0x9E3779B97F4A7C15ull ^ static_cast<unsigned long long>(time(nullptr));
    rc = spmx_encode_file_ex(h, in_path.c_str(), out_path.c_str(), format.c_str(), nbest_size, alpha, random_seed, &ns, nullptr, &ni);
  }
  if (rc != 0) fprintf(stderr, "%s\n", spmx_last_error(h));
  if (rc == 0 && output.empty()) {
    FILE *f = fopen(out_path.c_str(), "rb");
    char buf[1 << 16];
    size_t n;
    while (f && (n = fread(buf, 1, sizeof(buf), f)) > 0) fwrite(buf, 1, n, stdout);
    if (f) fclose(f);
  }
  if (from_stdin) remove(tin);
  if (output.empty()) remove(tout);
  spmx_destroy(h);
  if (rc == 0) fprintf(stderr, "spmx_encode: %llu sentences, %llu ids\n", static_cast<unsigned long long>(ns), static_cast<unsigned long long>(ni));
  return rc == 0 ? 0 : 1;
}
