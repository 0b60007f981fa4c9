// Status codes and the last-error plumbing of a kernel library (libbvhip, libbvdistill, libbveval): every entry
// point returns BV_OK or a negative code and leaves a message behind bv_set_error.  The public headers spell the
// same values as BV_* / BVD_* / BVE_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#define BV_OK 0
#define BV_ERR_INVALID_ARG (-1)
#define BV_ERR_UNSUPPORTED (-2)
#define BV_ERR_HIP (-3)

// A library that is ONE translation unit defines BV_STATUS_LINKAGE as `static` before its first include, so that the
// two helpers add no dynamic symbol; libbvhip's other translation units call the pair that c_api.cpp defines.
#ifndef BV_STATUS_LINKAGE
#define BV_STATUS_LINKAGE
#endif
BV_STATUS_LINKAGE void bv_set_error(const char* fmt, ...);
BV_STATUS_LINKAGE int bv_check_launch(const char* what);

#define BV_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) {                            \
      bv_set_error(__VA_ARGS__);              \
      return BV_ERR_INVALID_ARG;              \
    }                                         \
  } while (0)

// Expanded once per library, at namespace scope of one translation unit: the library's own thread-local message
// buffer (internal linkage: no two libraries can share it), the two helpers above and the two exported entry points
// `const char* last_error_fn(void)` / `int version_fn(void)`.
#define BV_DEFINE_STATUS(last_error_fn, version_fn, version)                       \
static thread_local char g_err[512] = "";                                          \
BV_STATUS_LINKAGE void bv_set_error(const char* fmt, ...) {                        \
  va_list ap;                                                                      \
  va_start(ap, fmt);                                                               \
  vsnprintf(g_err, sizeof(g_err), fmt, ap);                                        \
  va_end(ap);                                                                      \
}                                                                                  \
BV_STATUS_LINKAGE int bv_check_launch(const char* what) {                          \
  hipError_t e = hipGetLastError();                                                \
  if (e != hipSuccess) {                                                           \
    bv_set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));         \
    return BV_ERR_HIP;                                                             \
  }                                                                                \
  return BV_OK;                                                                    \
}                                                                                  \
extern "C" const char* last_error_fn(void) { return g_err; }                       \
extern "C" int version_fn(void) { return version; }
