// spmx_decode: the command line of the reference's spm_decode (src/spm_decode_main.cc) over the C ABI of include/spmx.h:
// a file (or stdin) of id lines, of piece lines or of flat binary ids in, one decoded line of text per input line out.
//   spmx_decode --model=M [--input=F] [--output=F] [--input_format=piece|id|bin] [--extra_options=reverse] [--device=N]
// --input_format=bin reads F and F.idx (what spmx_encode --output_format=bin writes) and needs --input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>

#include "../include/spmx.h"

int main(int argc, char **argv) {
  std::string model, input, output, format = "piece", extra;
  int device = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&](const char *name, std::string *dst) {
      const std::string k = std::string("--") + name + "=";
      if (a.compare(0, k.size(), k) == 0) { *dst = a.substr(k.size()); return true; }
      return false;
    };
    std::string dev;
    if (val("model", &model) || val("input", &input) || val("output", &output) || val("input_format", &format) ||
        val("extra_options", &extra)) continue;
    if (val("device", &dev)) { device = atoi(dev.c_str()); continue; }
    if (!a.empty() && a[0] != '-' && input.empty()) { input = a; continue; }
    fprintf(stderr, "unknown argument: %s\n", a.c_str());
    return 2;
  }
  if (model.empty()) { fprintf(stderr, "usage: spmx_decode --model=M [--input=F] [--output=F] [--input_format=piece|id|bin] [--extra_options=..]\n"); return 2; }
  if (format == "bin" && input.empty()) { fprintf(stderr, "--input_format=bin needs --input=F (F and F.idx are read)\n"); return 2; }
  spmx_handle *h = nullptr;
  if (spmx_create_from_file(model.c_str(), device, &h) != 0) { fprintf(stderr, "%s\n", spmx_last_error(nullptr)); return 1; }
  if (!extra.empty() && spmx_set_decode_extra_options(h, extra.c_str()) != 0) { fprintf(stderr, "%s\n", spmx_last_error(h)); return 1; }
  // stdin / stdout go through temporary files: the library maps its input
  std::string in_path = input, out_path = output;
  char tin[] = "/tmp/spmx_decode_in_XXXXXX", tout[] = "/tmp/spmx_decode_out_XXXXXX";
  if (in_path.empty()) {
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
  uint64_t nl = 0, ni = 0;
  const int rc = spmx_decode_file(h, in_path.c_str(), out_path.c_str(), format.c_str(), &nl, &ni);
  if (rc != 0) fprintf(stderr, "%s\n", spmx_last_error(h));
  if (rc == 0 && output.empty()) {
    FILE *f = fopen(out_path.c_str(), "rb");
    char buf[1 << 16];
    size_t n;
    while (f && (n = fread(buf, 1, sizeof(buf), f)) > 0) fwrite(buf, 1, n, stdout);
    if (f) fclose(f);
  }
  if (input.empty()) remove(tin);
  if (output.empty()) remove(tout);
  spmx_destroy(h);
  if (rc == 0) fprintf(stderr, "spmx_decode: %llu lines, %llu ids\n", static_cast<unsigned long long>(nl), static_cast<unsigned long long>(ni));
  return rc == 0 ? 0 : 1;
}
