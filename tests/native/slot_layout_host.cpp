// The slot layout of the host twins' staged call (pyorc_amd/csrc/host_slots.h) on the CPU: tests/test_host_slots_host.py builds this with
// -fsanitize=address,undefined and runs it.  Every case lays its slots out, then writes each present slot from end to end into a heap
// block of exactly the returned total -- so a slot that reaches past the total is an AddressSanitizer report, not only a failed check.
//
//   slot_layout_host        exit status 0 and "ok: <cases> cases", or 1 and the first failed check
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_slots.h"

using lspiv_api::kSlotAlign;
using lspiv_api::slot_layout;

struct Slot { size_t bytes; bool present; };

static int check_case(const char* name, const std::vector<Slot>& slots) {
  const int n = (int)slots.size();
  std::vector<size_t> bytes(n), off(n, (size_t)-1);
  bool flags[16];
  for (int i = 0; i < n; ++i) { bytes[i] = slots[i].bytes; flags[i] = slots[i].present; }
  const size_t total = slot_layout(bytes.data(), flags, n, off.data());
  size_t end = 0, room = 0;   // the end of the last present slot; the room all present slots need
  for (int i = 0; i < n; ++i) {
    if (off[i] % kSlotAlign) return std::printf("%s: slot %d at %zu is not aligned to %zu\n", name, i, off[i], kSlotAlign), 1;
    if (off[i] != end) return std::printf("%s: slot %d at %zu, the slots before it end at %zu\n", name, i, off[i], end), 1;   // a NULL entry took room
    if (!flags[i]) continue;
    for (int k = 0; k < i; ++k)
      if (flags[k] && bytes[k] && bytes[i] && off[k] + bytes[k] > off[i]) return std::printf("%s: slots %d and %d overlap\n", name, k, i), 1;
    end = off[i] + ((bytes[i] + kSlotAlign - 1) / kSlotAlign) * kSlotAlign;
    room += ((bytes[i] + kSlotAlign - 1) / kSlotAlign) * kSlotAlign;
  }
  if (total != end || total != room) return std::printf("%s: total %zu, the slots end at %zu and need %zu\n", name, total, end, room), 1;
  // the workspace is sized to `total`: every byte of every present slot lies inside it, and no two slots share one
  char* ws = new char[total ? total : 1];
  std::memset(ws, 0, total ? total : 1);
  for (int i = 0; i < n; ++i) {
    if (!flags[i]) continue;
    for (size_t b = 0; b < bytes[i]; ++b) {
      if (ws[off[i] + b]) { delete[] ws; return std::printf("%s: byte %zu of slot %d belongs to slot %d as well\n", name, b, i, ws[off[i] + b] - 1), 1; }
      ws[off[i] + b] = (char)(i + 1);
    }
  }
  delete[] ws;
  return 0;
}

int main() {
  const struct { const char* name; std::vector<Slot> slots; } cases[] = {
    {"empty", {}},
    {"one byte", {{1, true}}},
    {"zero bytes", {{0, true}}},
    {"all absent", {{100, false}, {0, false}, {4096, false}}},
    {"exact multiples", {{256, true}, {512, true}, {1024, true}}},
    {"mixed", {{96, true}, {96, true}, {0, true}, {144, false}, {12, true}, {257, true}, {255, true}, {1, true}}},
    {"absent first and last", {{48, false}, {1000003, true}, {48, false}}},
    {"zero between", {{300, true}, {0, true}, {0, false}, {300, true}}},
    {"validate: u v peak2 flag", {{31892, true}, {31892, true}, {127568, false}, {7973, true}}},
    {"eight slots", {{7, true}, {8, true}, {9, true}, {0, false}, {511, true}, {513, true}, {1, false}, {65537, true}}},
  };
  int n = 0;
  for (const auto& c : cases) {
    if (check_case(c.name, c.slots)) return 1;
    ++n;
  }
  // the totals the entry points ask `ensure` for, worked out by hand
  const size_t b1[3] = {96, 0, 12};
  const bool p1[3] = {true, true, true};
  size_t o1[3];
  if (slot_layout(b1, p1, 3, o1) != 512 || o1[0] != 0 || o1[1] != 256 || o1[2] != 256) return std::printf("by hand: 96 | 0 | 12\n"), 1;
  const size_t b2[3] = {1000, 48, 257};
  const bool p2[3] = {true, false, true};
  size_t o2[3];
  if (slot_layout(b2, p2, 3, o2) != 1024 + 512 || o2[0] != 0 || o2[1] != 1024 || o2[2] != 1024) return std::printf("by hand: 1000 | NULL | 257\n"), 1;
  std::printf("ok: %d cases\n", n + 2);
  return 0;
}
