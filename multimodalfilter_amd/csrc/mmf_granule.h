// Tagged granules: the hand-off unit of the persistent loops (pf_persistent.inc, ekf_persistent.inc, lstm.hip).
//
// A value another workgroup of the SAME launch wrote or will read travels as an 8-byte GRANULE {fp32 value, u32 tag}
// moved by ONE agent-scope relaxed atomic (global_load / global_store_dwordx2 ... sc1: served by / written through to
// L2, never a stale per-CU L1 line; MI355X_MICROARCH.md, inter-workgroup visibility; cdna_hip_programming.md Guideline
// 16, R2: the data IS the flag).  The tag names the step the value belongs to (tag = step + 1); a reader spins on its
// own granules until the tag is the step's, so no separate flag, fence or store drain sits on the chain.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mmf.h"

namespace mmf {

// ---- granules: {fp32 value, u32 tag} in one naturally aligned 8-byte word, written and read by ONE instruction
using Granule = unsigned long long;
__device__ __forceinline__ Granule make_granule(float v, unsigned tag) {
  return (static_cast<Granule>(tag) << 32) | static_cast<Granule>(__float_as_uint(v));
}
__device__ __forceinline__ float granule_value(Granule g) { return __uint_as_float(static_cast<unsigned>(g)); }
__device__ __forceinline__ unsigned granule_tag(Granule g) { return static_cast<unsigned>(g >> 32); }
__device__ __forceinline__ Granule ld_granule(const Granule* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_granule(Granule* p, float v, unsigned tag) {
  __hip_atomic_store(p, make_granule(v, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr unsigned kGranuleSpinLimit = 1u << 13;  // polls (>= ~0.5 us each: 4-8 ms) before a reader gives up and the
                                                   // host re-runs the loop as launches (a healthy hand-off takes microseconds)

// ---- the bounded spin of a wave that polls granules, and what it does when the bound is reached.
// One failed poll: true (wave-uniform) when the wave must stop -- every 64 polls lane 0 looks at the spin budget and at
// the launch's abort word, which another wave raises when IT gave up.  The pause between polls is the caller's.
__device__ __forceinline__ bool spin_stop(const unsigned* abort_word, unsigned& spins, int lane) {
  if ((++spins & 63u) != 0) return false;
  int stop = 0;
  if (lane == 0) stop = (spins > kGranuleSpinLimit || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? 1 : 0;
  return __builtin_amdgcn_readfirstlane(stop) != 0;
}
// One lane of a wave or workgroup that stopped: every other wave of the launch follows at its next poll, and the host
// discards this loop and re-runs it as launches (engine.run_persistent reads MMF_FLAG_GAVE_UP from the status word).
__device__ __forceinline__ void give_up(unsigned* abort_word, int* status_word) {
  __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (status_word != nullptr) atomicOr(status_word, MMF_FLAG_GAVE_UP);
}

}  // namespace mmf
