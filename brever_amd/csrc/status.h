// Host-side status helpers shared by every translation unit of the library: the one error contract of
// include/brever_hip.h (0 ok, < 0 refused argument / unsupported configuration, > 0 a hipError_t, and
// brv_last_error() says why). No kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

namespace brv {

// Stores msg in the library's thread-local message (BRV_DEFINE_STATUS) and returns code.
__attribute__((visibility("hidden"))) int fail(int code, const char* msg);
// (hidden as well: next to the definition the compiler may emit this overload out of line, and as a weak default
// symbol one library's copy could be bound to another's, whose message it would then set)
__attribute__((visibility("hidden"))) inline int fail(int code, const std::string& msg) {
  return fail(code, msg.c_str());
}

// The library's last-error message and its two status exports: one thread-local string, written through brv::fail
// only (hidden: every library has its own, non-interposable copy) and read through last_error_fn. Goes into exactly
// ONE translation unit per shared library, at file scope, after the library's header has declared the two names.
#define BRV_DEFINE_STATUS(version_fn, last_error_fn)                                                    \
  namespace {                                                                                           \
  thread_local std::string g_err;                                                                       \
  }                                                                                                     \
  int brv::fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }                     \
  extern "C" {                                                                                          \
  int version_fn(void) { return 100; }                                                                  \
  const char* last_error_fn(void) { return g_err.c_str(); }                                             \
  }

// a failing HIP call ends the entry point with its hipError_t
#define BRV_HIP_OK(expr)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::brv::fail((int)e_, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// an argument the entry point does not take (-1) / a configuration it does not support (-2)
#define BRV_REFUSE(cond, msg) do { if (cond) return ::brv::fail(-1, msg); } while (0)
#define BRV_UNSUPPORTED(cond, msg) do { if (cond) return ::brv::fail(-2, msg); } while (0)

// grid of 256-thread workgroups for a GRID_STRIDE loop (common.cuh) over n elements
inline dim3 flat_grid(long long n, long long cap = 8192) {
  long long g = (n + 255)/256;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return dim3((unsigned)g);
}

}  // namespace brv
