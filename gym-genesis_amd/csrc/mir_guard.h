// mir_guard.h — the device guard every host entry point of the library takes before it launches or allocates: the calling thread's
// current device is switched to the scene's for the guard's lifetime and restored after it.
#pragma once
#include <hip/hip_runtime.h>

struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
