// Device copies of small host-assembled tables (the zMobius ZCoef, the fused
// domain-wall W blocks), cached by (device, content). Operators reuse a
// handful of tables for their whole life, so a steady-state launch does no
// host-to-device transfer; a cached copy is never rewritten, so launches on
// any stream may read it concurrently. Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>

// The table's device copy on the current device, or nullptr when the
// allocation or the copy failed. A miss copies synchronously.
inline const void *device_table(const void *host, size_t bytes) {
  static std::map<std::string, void *> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::string key((const char *)&dev, sizeof(dev));
  key.append((const char *)host, bytes);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  if (cache.size() >= 256) {  // hipFree waits for in-flight kernels
    for (auto &kv : cache) (void)hipFree(kv.second);
    cache.clear();
  }
  void *dptr = nullptr;
  if (hipMalloc(&dptr, bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(dptr, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dptr);
    return nullptr;
  }
  cache.emplace(std::move(key), dptr);
  return dptr;
}
