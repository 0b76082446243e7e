// Workspace layout: every region of a caller-provided workspace starts on a 256-byte boundary.
#pragma once
#include <cstddef>

namespace cfm {

inline size_t align_up(size_t x) { return (x + 255) / 256 * 256; }

// hands out consecutive aligned regions of `base`; with a null base it only counts (off = the bytes needed)
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename U> U* take(size_t n) {
    U* p = (U*)(base ? base + off : nullptr);
    off += align_up(n * sizeof(U));
    return p;
  }
};

}  // namespace cfm
