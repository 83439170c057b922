// What a library of its own beside libtad_mi355x.so (simple_tad_amd/build.py: SIDE_LIBS) defines for itself: the error text and the
// launch check that common.h declares (capi.hip's are the first library's and are neither used nor shadowed).  Included by the ONE
// source of such a library, which is built with -fvisibility=hidden and exports its entry points alone; its *_last_error_string returns
// tad::side_last_error().
#pragma once
#include <stdarg.h>
#include "common.h"

namespace tad {

static thread_local char g_side_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_side_err, sizeof(g_side_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return TAD_ELAUNCH;
  }
  return TAD_OK;
}

static inline const char* side_last_error() { return g_side_err; }

}  // namespace tad
