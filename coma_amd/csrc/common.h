// Shared host-side helpers for libcoma_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../include/coma_hip.h"

namespace coma {

char* err_buf();  // thread-local, defined in abi.hip

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(COMA_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return COMA_OK;
}

constexpr int kWave = 64;  // CDNA wavefront

// ---- caller-owned buffers: workspaces, saved state ----
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// Lays fields out one after the other, each at a multiple of 16: take() gives the field's offset, `at` ends as the total.
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t offset = at;
    at = align16(at + bytes);
    return offset;
  }
};

inline int check_buffer(const char* who, const char* what, const void* p, size_t have, size_t need) {
  if (have < need) return fail(COMA_E_INVALID, "%s: %s of %zu bytes, %zu needed", who, what, have, need);
  if (((uintptr_t)p & 15) != 0) return fail(COMA_E_INVALID, "%s: %s must be 16-byte aligned", who, what);
  return COMA_OK;
}

inline bool f32_aligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (((uintptr_t)p & 3) != 0) return false;
  return true;
}

// The status reads: a small header copied back on the caller's stream, which is then waited for.
inline int read_back(void* dst, const void* src_dev, size_t bytes, void* stream, const char* who) {
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return fail(COMA_E_DEVICE, "%s: %s", who, hipGetErrorString(hipGetLastError()));
  return COMA_OK;
}

// Opt a kernel into more than 64 KB of dynamic LDS.  The attribute belongs to the function object of the CURRENT DEVICE, so the
// "already done" state is kept per device (a process that drives a second GPU must opt that device in as well) and in atomics
// (two threads may race to set it: the call is idempotent).  One LdsOptIn per call site / kernel instantiation.
struct LdsOptIn {
  static constexpr int kMaxDevices = 64;
  std::atomic<size_t> bytes[kMaxDevices] = {};
};

inline int opt_in_lds(LdsOptIn& slot, const void* fn, size_t bytes, const char* who) {
  int dev = -1;
  const bool tracked = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < LdsOptIn::kMaxDevices;
  if (tracked && slot.bytes[dev].load(std::memory_order_acquire) >= bytes) return COMA_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return fail(COMA_E_LAUNCH, "%s: cannot reserve %zu bytes of LDS", who, bytes);
  if (tracked) {
    size_t cur = slot.bytes[dev].load(std::memory_order_relaxed);
    while (cur < bytes && !slot.bytes[dev].compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
  }
  return COMA_OK;
}

}  // namespace coma
