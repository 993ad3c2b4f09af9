// TEST INFRASTRUCTURE ONLY (see wave_emu.h, emu_launch.cc): the launcher of the token-text kernels
// (csrc/kernels_tokentext.h) on the lock-step wave model.  Included by csrc/api.cc where it is built for the emulator
// (SPMX_WAVE_API), so that libspmx_emu.so holds it beside emu_launch.cc's.
#ifndef SPMX_EMU_LAUNCH_TOKENTEXT_H_
#define SPMX_EMU_LAUNCH_TOKENTEXT_H_

namespace spmx {
namespace {
template <int FMT, bool LINES>
void RunTokenText(bool write, const TokenTextArgs &a, int grid) {
  for (int b = 0; b < grid; ++b) {
    if (write) emu::RunWave(b, grid, nullptr, [&] { token_write_block<FMT, LINES>(a); });
    else emu::RunWave(b, grid, nullptr, [&] { token_len_block<FMT, LINES>(a); });
  }
}
}  // namespace
hipError_t LaunchTokenText(int fmt, bool lines, bool write, const TokenTextArgs &a, int grid, hipStream_t) {
  if (fmt == 0) RunTokenText<0, true>(write, a, grid);
  else if (lines) RunTokenText<1, true>(write, a, grid);
  else RunTokenText<1, false>(write, a, grid);
  return hipSuccess;
}
}  // namespace spmx
#endif
