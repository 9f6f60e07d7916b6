// tick2.hip - second translation unit of libdust_amd.so: the owner-computes persistent tick kernel (tick2.hpp) and its launcher.
// Kept apart from dust_amd.hip so that the two compile in parallel (build() in __graft_entry__.py) and a change to this kernel does
// not rebuild the rest of the library.
#include "tick2.hpp"

namespace dust {

// the kernel's instance for a model (Pendulum, else Particle) and a pairwise mode (IMQ, else K1)
static auto tick2_instance(int model, int mode) {
  if (model == DUST_MODEL_PENDULUM) return mode == PAIR_IMQ ? svmpc_tick2_kernel<DUST_MODEL_PENDULUM, PAIR_IMQ> : svmpc_tick2_kernel<DUST_MODEL_PENDULUM, PAIR_K1>;
  return mode == PAIR_IMQ ? svmpc_tick2_kernel<DUST_MODEL_PARTICLE, PAIR_IMQ> : svmpc_tick2_kernel<DUST_MODEL_PARTICLE, PAIR_K1>;
}

// (the attribute is set here, before the first launch: the occupancy query needs it, and launch_tick2 asks once per LDS size)
static int occ_of(const void *kernel, size_t lds, int *occ) {
  hipError_t e = hipSuccess;
  if (lds > 64 * 1024) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kernel, T2_NT, lds);
  return (int)e;
}

int tick2_occupancy(int model, int mode, size_t lds, int *occ) {
  *occ = 0;
  return occ_of((const void *)tick2_instance(model, mode), lds, occ);
}

int tick2_launch(const Tick2Args &f, int model, int mode, int grid, size_t lds, hipStream_t stream) {
  const auto kernel = tick2_instance(model, mode);
  kernel<<<grid, T2_NT, lds, stream>>>(f);
  return (int)hipGetLastError();
}

}  // namespace dust
