// TEST INFRASTRUCTURE ONLY (see wave_emu.h, emu_launch.cc): the launchers of the word / character kernels
// (csrc/kernels_charword.h, kernels_charwave.h) on the lock-step wave model.  Included by csrc/api.cc where it is built
// for the emulator (SPMX_WAVE_API), so that libspmx_emu.so holds them beside emu_launch.cc's.
#ifndef SPMX_EMU_LAUNCH_CHARWORD_H_
#define SPMX_EMU_LAUNCH_CHARWORD_H_
#include <vector>

namespace spmx {
namespace {
template <typename F>
void RunCharWordGrid(int grid, int waves, uint32_t lds_bytes, F body) {
  std::vector<unsigned char> raw(lds_bytes + 128);
  unsigned char *smem = raw.data() + ((64 - (reinterpret_cast<uintptr_t>(raw.data()) & 63)) & 63);
  for (int b = 0; b < grid; ++b) {
    memset(smem, 0xCD, lds_bytes + 32);
    for (int w = 0; w < waves; ++w) {
      emu::g_wave.wib = w;
      emu::g_wave.wpb = waves;
      emu::RunWave(b, grid, smem, [&] { body(smem); });
    }
  }
  emu::g_wave.wib = 0;
  emu::g_wave.wpb = 1;
}
}  // namespace

hipError_t LaunchEncodeCharWord(int model_type, bool uds, const EncodeArgs &a, int grid, int waves, uint32_t lds_bytes, hipStream_t) {
  if (model_type == 3) RunCharWordGrid(grid, waves, lds_bytes, [&](unsigned char *s) { encode_stream_block<3, 0, false>(a, s); });
  else if (uds) RunCharWordGrid(grid, waves, lds_bytes, [&](unsigned char *s) { encode_stream_block<4, 0, true>(a, s); });
  else RunCharWordGrid(grid, waves, lds_bytes, [&](unsigned char *s) { encode_stream_block<4, 0, false>(a, s); });
  return hipSuccess;
}
hipError_t LaunchCharWordLong(bool word, const LongArgs &a, int grid, hipStream_t) {
  if (word) RunCharWordGrid(grid, 1, kCwWaveLdsBytes, [&](unsigned char *s) { charword_long_block<true>(a, s); });
  else RunCharWordGrid(grid, 1, kCwWaveLdsBytes, [&](unsigned char *s) { charword_long_block<false>(a, s); });
  return hipSuccess;
}
}  // namespace spmx
#endif
