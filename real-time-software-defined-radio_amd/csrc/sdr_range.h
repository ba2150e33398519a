// The split of a contiguous range of elements into what 16-B loads can take and what they cannot:
// plain C++ for host and device alike (tests/pass_range_main.cpp builds it with the host compiler).
// Not part of the public ABI (include/sdr.h).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SDR_HD __host__ __device__
#else
#define SDR_HD
#endif

namespace sdrint {

struct RangeSplit {
  int head, tail;   // elements before the first 16-B boundary (< 16 / ES) and after the last whole vector
  int64_t nv;       // whole 16-B vectors between them
};

// len elements of ES bytes (2, 4 or 8) from address addr, a multiple of ES, on: no part leaves the range
template <int ES>
SDR_HD constexpr RangeSplit split_range(uintptr_t addr, int64_t len) {
  static_assert(ES == 2 || ES == 4 || ES == 8, "an element divides a 16-B vector");
  constexpr int V = 16 / ES;
  const int mis = (int)(addr & 15);
  const int64_t h = mis ? (16 - mis) / ES : 0;
  const int head = (int)(h < len ? h : len);
  const int64_t nv = (len - head) / V;
  return RangeSplit{head, (int)(len - head - nv * V), nv};
}

}  // namespace sdrint
