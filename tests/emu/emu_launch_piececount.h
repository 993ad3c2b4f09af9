// TEST INFRASTRUCTURE ONLY (see wave_emu.h, emu_launch.cc): the launcher of the id histogram (csrc/kernels_piececount.h) on
// the lock-step wave model.  Included by csrc/api.cc where it is built for the emulator (SPMX_WAVE_API).
// The kernel's three phases are separated by workgroup barriers.  The wavefronts of a workgroup run one after another here,
// so each phase is run for EVERY wavefront of the workgroup, over one LDS image, before the next phase starts: exactly what
// the barrier guarantees on the device.
#ifndef SPMX_EMU_LAUNCH_PIECECOUNT_H_
#define SPMX_EMU_LAUNCH_PIECECOUNT_H_

#include <mutex>
#include <vector>

namespace spmx {
// The workers of spmx_count_file share one histogram and rely on the device's atomics.  wv::atomic_add of the wave model is
// a plain read-modify-write (one wavefront at a time per host thread), so launches from different host threads take turns.
static std::mutex &g_count_launch = *new std::mutex;
hipError_t LaunchCountIds(const CountArgs &a, int grid, int waves, hipStream_t) {
  std::lock_guard<std::mutex> turn(g_count_launch);
  std::vector<uint32_t> lds(a.bins + 16u);
  uint32_t *bins = lds.data();
  unsigned char *smem = reinterpret_cast<unsigned char *>(bins);
  for (int b = 0; b < grid; ++b) {
    memset(smem, 0xCD, lds.size() * sizeof(uint32_t));
    for (int phase = 0; phase < 3; ++phase) {
      for (int w = 0; w < waves; ++w) {
        emu::g_wave.wib = w;
        emu::g_wave.wpb = waves;
        emu::RunWave(b, grid, smem, [&] {
          if (phase == 0) count_zero_phase(a, bins);
          else if (phase == 1) count_sweep_phase(a, bins);
          else count_flush_phase(a, bins);
        });
      }
    }
    for (uint32_t i = a.bins; i < a.bins + 16u; ++i)
      if (bins[i] != 0xCDCDCDCDu) { fprintf(stderr, "CountIds: a write behind the LDS bins\n"); abort(); }
  }
  emu::g_wave.wib = 0;
  emu::g_wave.wpb = 1;
  return hipSuccess;
}
}  // namespace spmx
#endif
