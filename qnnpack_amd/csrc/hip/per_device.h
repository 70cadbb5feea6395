/*
 * per_device.h -- launch-side helpers (HIP-internal, C++ only): the "once per device" guard for launch-side set-up,
 * the dynamic-LDS opt-in built on it, the launch status and the compute-unit count.
 * hipFuncSetAttribute (the > 64 KiB dynamic-LDS opt-in) is a PER-DEVICE property of a kernel: a process that drives
 * several GPUs (runtime.hip) must set it on each of them, and several threads may reach the same launch helper.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "qnnp_hip.h"

namespace qnnp {

struct PerDeviceOnce {
  std::atomic<uint32_t> done{0};
  /* `if (auto once = guard.begin()) { hipFuncSetAttribute(...); }` -- the body runs until ONE caller has finished it on
   * the active device: the done bit is published by the scope's destructor, i.e. AFTER the attribute call returned, so a
   * second thread launching the same kernel at the same moment either sees the bit (the opt-in exists) or makes the
   * idempotent call itself -- never a launch with > 64 KiB of dynamic LDS ahead of the opt-in. */
  struct Scope {
    std::atomic<uint32_t>* word;
    uint32_t bit;
    explicit operator bool() const { return word != nullptr; }
    ~Scope() { if (word != nullptr) word->fetch_or(bit, std::memory_order_release); }
  };
  Scope begin()
  {
    const int device = qnnp_hip_device();
    const uint32_t bit = 1u << (static_cast<uint32_t>(device < 0 ? 0 : device) & 31u);
    if ((done.load(std::memory_order_acquire) & bit) != 0) return Scope{nullptr, 0u};
    return Scope{&done, bit};
  }
};

/* Opt Kernel in to `bytes` of dynamic LDS on the active device, once per (kernel, device). A refusal is cleared from
 * the error state: the launch that needed the opt-in then fails on its own, and launch_status() reports it. */
template <auto Kernel>
void allow_dynamic_lds(int bytes)
{
  static PerDeviceOnce once;
  if (auto scope = once.begin()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
      (void) hipGetLastError();
  }
}

/* the result of the launch just made */
inline int launch_status() { return hipGetLastError() == hipSuccess ? QNNP_HIP_OK : QNNP_HIP_ELAUNCH; }

/* compute units of the active device, 256 when no device context is bound */
inline uint32_t active_cu_count()
{
  const int cus = qnnp_hip_compute_units();
  return cus > 0 ? static_cast<uint32_t>(cus) : 256u;
}

}  // namespace qnnp
