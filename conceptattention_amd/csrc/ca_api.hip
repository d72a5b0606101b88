// Host-side plumbing of libconceptattn: version, thread-local error text, device check, launch helpers.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ca_common.h"

static thread_local char g_err[512] = "";

void ca_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// CU count of the current device (cached per device; a race only repeats the query); -1 if the query fails
int ca_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int n = cus[dev & 63].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = -1;
    cus[dev & 63].store(n, std::memory_order_relaxed);
  }
  return n;
}

int ca_raise_lds_limit(std::initializer_list<const void *> kernels, int bytes, std::atomic<unsigned long long> &done,
                       const char *FN) {
  const unsigned long long dev_bit = ca_device_bit();
  if (done.load(std::memory_order_acquire) & dev_bit) return CA_OK;
  for (const void *k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
      ca_set_error("%s: hipFuncSetAttribute(%d bytes LDS): %s", FN, bytes, hipGetErrorString(e));
      return CA_ERR_LAUNCH;
    }
  }
  done.fetch_or(dev_bit, std::memory_order_release);
  return CA_OK;
}

int ca_check_launch(const char *FN) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ca_set_error("%s: launch failed: %s", FN, hipGetErrorString(e));
    return CA_ERR_LAUNCH;
  }
  return CA_OK;
}

extern "C" int ca_version(void) { return CA_VERSION; }

extern "C" const char *ca_last_error(void) { return g_err; }

extern "C" int ca_check_device(void) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) {
    ca_set_error("ca_check_device: hipGetDevice: %s", hipGetErrorString(e));
    return CA_ERR_ARCH;
  }
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, dev);
  if (e != hipSuccess) {
    ca_set_error("ca_check_device: hipGetDeviceProperties: %s", hipGetErrorString(e));
    return CA_ERR_ARCH;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    ca_set_error("ca_check_device: device %d is %s; libconceptattn is built for gfx950 only", dev, prop.gcnArchName);
    return CA_ERR_ARCH;
  }
  return CA_OK;
}
