// Host side of every entry point that takes caller-owned device memory (the alignment stages through align_common.h, the training
// seams of rnn_grad.hip and cnn_grad.hip, chiron_ctc_loss): the error text, the device to run on, the operands' residence and the
// status of the launches.  The text of chiron_last_error() is part of what the tests pin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chiron_amd.h"

namespace chiron {

chiron_status set_error(chiron_status st, const char* fmt, ...);   // engine.hip

// Makes device_id current.  who = nullptr: the alignment stages' texts, which carry no entry-point prefix.
inline chiron_status enter_device(const char* who, int32_t device_id) {
  const char* sep = who ? ": " : "";
  if (!who) who = "";
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    (void)hipGetLastError();
    return set_error(CHIRON_ERR_DEVICE, "%s%sno HIP device %d: libchiron_amd has no CPU fallback", who, sep, device_id);
  }
  if (hipSetDevice(device_id) != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "%s%shipSetDevice(%d) failed", who, sep, device_id);
  return CHIRON_OK;
}

inline bool on_device(const void* p) {
  hipPointerAttribute_t a;
  const bool ok = p && hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice;
  if (!ok) (void)hipGetLastError();
  return ok;
}

inline chiron_status launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
  return CHIRON_OK;
}

}  // namespace chiron
