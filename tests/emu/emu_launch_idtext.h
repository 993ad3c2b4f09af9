// TEST INFRASTRUCTURE ONLY (see wave_emu.h, emu_launch.cc): the launchers of the id-line parser and the line joiner
// (csrc/kernels_idtext.h) on the lock-step wave model.  Included by csrc/api.cc where it is built for the emulator
// (SPMX_WAVE_API), so that libspmx_emu.so holds them beside emu_launch.cc's.
#ifndef SPMX_EMU_LAUNCH_IDTEXT_H_
#define SPMX_EMU_LAUNCH_IDTEXT_H_

namespace spmx {
hipError_t LaunchParseIdLines(bool write, const ParseIdsArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) {
    if (write) emu::RunWave(b, grid, nullptr, [&] { parse_ids_block<true>(a); });
    else emu::RunWave(b, grid, nullptr, [&] { parse_ids_block<false>(a); });
  }
  return hipSuccess;
}
hipError_t LaunchJoinLines(const JoinLinesArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { join_lines_block(a); });
  return hipSuccess;
}
}  // namespace spmx
#endif
