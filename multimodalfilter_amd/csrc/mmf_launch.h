// The host side of a launch: kernels that ask for dynamic LDS, the co-residency test of the persistent grids, and the
// run-time value -> template argument steps of the dispatchers.  Launches without dynamic LDS keep <<<>>> + MMF_CHECK_LAUNCH.
#pragma once
#include <type_traits>
#include <utility>

#include "mmf_common.h"

namespace mmf {

constexpr size_t kLdsPerCu = 160u << 10;      // LDS of a gfx950 CU: the most one workgroup can ask for
constexpr size_t kLdsHalfCu = kLdsPerCu / 2;  // what a workgroup may take while two of them share a CU
constexpr size_t kLdsOptIn = 64u << 10;       // dynamic LDS above this has to be allowed per kernel before the launch

// the opt-in of a kernel that asks for more than kLdsOptIn of dynamic LDS; 0 or the hipError_t
template <class... P>
int allow_lds(void (*kernel)(P...), size_t lds_bytes) {
  if (lds_bytes <= kLdsOptIn) return 0;
  return static_cast<int>(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              static_cast<int>(lds_bytes)));
}

// kernel<<<grid, block, lds_bytes, stream>>>(args...): 0 or the hipError_t of the opt-in / the launch.  No other host call:
// the launch path of the small problems is host-bound.
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, A&&... args) {
  if (const int rc = allow_lds(kernel, lds_bytes)) return rc;
  kernel<<<grid, block, lds_bytes, stream>>>(std::forward<A>(args)...);
  return static_cast<int>(hipGetLastError());
}

// The ONE co-residency test of the persistent kernels, whose workgroups spin on each other's output: a grid that is not
// wholly resident hangs.  0: `blocks` workgroups of `threads` threads and `lds_bytes` of dynamic LDS are resident together
// on this device, by what the runtime says about THIS kernel; MMF_INTERNAL_NOT_RESIDENT: they are not (the caller takes its
// loop of launches); a hipError_t: a query failed.
template <class... P>
int resident(void (*kernel)(P...), int blocks, int threads, size_t lds_bytes) {
  if (const int rc = allow_lds(kernel, lds_bytes)) return rc;
  int per_cu = 0, dev = 0, cus = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), threads, lds_bytes);
  if (e == hipSuccess) e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return static_cast<int>(e);
  return per_cu >= 1 && blocks <= per_cu * cus ? 0 : MMF_INTERNAL_NOT_RESIDENT;
}

// a run-time flag / state dimension as a type, for `decltype(x)::value` template arguments: f(std::bool_constant<b>{}),
// f(std::integral_constant<int, d>{}) with d in 1 .. MMF_MAX_STATE_DIM (the callers have checked it)
template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
auto with_state_dim(int d, F&& f) {
  static_assert(MMF_MAX_STATE_DIM == 4, "one case per state dimension");
  switch (d) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

}  // namespace mmf
