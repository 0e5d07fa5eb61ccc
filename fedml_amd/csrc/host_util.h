// host_util.h — the host-side error reporting that every translation unit of
// libfedagg.so beside fedagg.hip shares.  fedagg.hip owns the thread's last
// error message and defines fedagg_set_error_internal; the other units report
// through it.  Everything here is internal to the including unit.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fedagg.h"

extern "C" int fedagg_set_error_internal(int code, const char* msg);

namespace {

[[maybe_unused]] int set_error(int code, const std::string& msg) {
  return fedagg_set_error_internal(code, msg.c_str());
}

// the launches before it, as `what`: FEDAGG_OK, or the HIP error recorded
[[maybe_unused]] int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(static_cast<int>(e), std::string(what) + ": " + hipGetErrorString(e));
  return FEDAGG_OK;
}

}  // namespace
