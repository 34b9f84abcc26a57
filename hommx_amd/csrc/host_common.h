// host_common.h -- host plumbing every translation unit shares: the one error message behind hommx_last_error() and the packed upload of
// host tables into one device block.  Defined in api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>

#include "../../include/hommx_hip.h"

namespace hommx {

// Sets the calling thread's message (hommx_last_error()) and returns `code`.  A layer that reports a lower layer's failure under its own
// name puts the name in front on the way out: prefix_error(rc, "mesh route: ").
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int prefix_error(int code, const char* prefix);

// the blocked family words a failed HIP call "<call>: <error>" (it defines HOMMX_HIP_TRY_FMT so), everyone else "<call> failed: <error>"
#ifndef HOMMX_HIP_TRY_FMT
#define HOMMX_HIP_TRY_FMT "%s failed: %s"
#endif
// HIP_TRY_OR: `cleanup` runs before the failing function returns
#define HIP_TRY_OR(cleanup, expr) HOMMX_HIP_TRY_(cleanup, expr, #expr)
#define HIP_TRY(expr) HOMMX_HIP_TRY_((void)0, expr, #expr)
#define HOMMX_HIP_TRY_(cleanup, expr, text)                                                                                       \
  do {                                                                                                                            \
    hipError_t e__ = (expr);                                                                                                      \
    if (e__ != hipSuccess) {                                                                                                      \
      cleanup;                                                                                                                    \
      return ::hommx::fail(e__ == hipErrorOutOfMemory ? HOMMX_ENOMEM : HOMMX_EHIP, HOMMX_HIP_TRY_FMT, text, hipGetErrorString(e__)); \
    }                                                                                                                             \
  } while (0)

// The layout of every packed block: pieces of bytes[k] bytes end to end, each 256-byte aligned (so a piece of 0 bytes takes no room).
// off[k]: where piece k starts; returns the size of the block.
inline size_t pack_offsets(size_t n, const size_t* bytes, size_t* off) {
  size_t total = 0;
  for (size_t k = 0; k < n; ++k) {
    off[k] = total;
    total += (bytes[k] + 255) / 256 * 256;
  }
  return total;
}

// One device allocation (*block, the caller's to hipFree) that holds a copy of every host array, laid out by pack_offsets; *dst of a
// piece is where it starts on the device.
struct HostPiece {
  const void* src;
  size_t bytes;
  const void** dst;
};
int upload_packed(void** block, std::initializer_list<HostPiece> pieces);

}  // namespace hommx
