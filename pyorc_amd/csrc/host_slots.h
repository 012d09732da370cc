// The slot layout of a host twin's staged call (api_internal.h, HostCall).  Pure host arithmetic, no HIP: tests/native/slot_layout_host.cpp
// checks it without a device.
#pragma once

#include <cstddef>

namespace lspiv_api {

constexpr size_t kSlotAlign = 256;   // every slot starts on a multiple of this: enough for any element type; nothing reads the gaps

// n slots laid out one after another: offset[i] of slot i, the total as the return value (what the workspace is sized to).  A slot
// that is not `present` (an optional argument that was not given) takes no room.
inline size_t slot_layout(const size_t* bytes, const bool* present, int n, size_t* offset) {
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    offset[i] = at;
    if (present[i]) at += (bytes[i] + kSlotAlign - 1) & ~(kSlotAlign - 1);
  }
  return at;
}

}  // namespace lspiv_api
