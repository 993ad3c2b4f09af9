// TEST INFRASTRUCTURE ONLY (see wave_emu.h, emu_launch.cc): the launchers of the lattice-results-to-CSR kernels
// (csrc/kernels_latticecsr.h) on the lock-step wave model.  Included by csrc/api.cc where it is built for the emulator
// (SPMX_WAVE_API), so that libspmx_emu.so holds them beside emu_launch.cc's.
#ifndef SPMX_EMU_LAUNCH_LATTICECSR_H_
#define SPMX_EMU_LAUNCH_LATTICECSR_H_

namespace spmx {
hipError_t LaunchLatticeCsr(bool gather, const LatticeCsrArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) {
    if (gather) emu::RunWave(b, grid, nullptr, [&] { latticecsr_gather_block(a); });
    else emu::RunWave(b, grid, nullptr, [&] { latticecsr_rows_block(a); });
  }
  return hipSuccess;
}
hipError_t LaunchLatticePick(const LatticePickArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { latticecsr_pick_block(a); });
  return hipSuccess;
}
hipError_t LaunchLatticeMaxLen(const LatticeMaxLenArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { latticecsr_maxlen_block(a); });
  return hipSuccess;
}
hipError_t LaunchLatticeRefSpan(bool flags, const LatticeRefSpanArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) {
    if (flags) emu::RunWave(b, grid, nullptr, [&] { latticecsr_spflag_block(a); });
    else emu::RunWave(b, grid, nullptr, [&] { latticecsr_refspan_block(a); });
  }
  return hipSuccess;
}
hipError_t LaunchLatticeIota(const LatticeIotaArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { latticecsr_iota_block(a); });
  return hipSuccess;
}
}  // namespace spmx
#endif
