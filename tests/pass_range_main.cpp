// Prints what csrc/sdr_range.h makes of a range, for tests/test_pass_range.py: the header is plain
// C++, built by the host compiler with the address and undefined-behaviour sanitizers.  For every
// element size 2, 4, 8, every start that is a multiple of it in [0, 16) and every length
// 0 .. 3 * 16 / ES + 3:
//   range ES start len head nv tail
// The range lies in a heap block that ends with it, and the program reads it as a pass does -- the
// head elements, the 16-B vectors, the tail elements -- so an access outside it stops the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../real-time-software-defined-radio_amd/csrc/sdr_range.h"

template <int ES>
static unsigned read_as_split(const unsigned char* p, const sdrint::RangeSplit& r) {
  unsigned sum = 0;
  unsigned char v[16];
  auto take = [&](const unsigned char* q, int bytes) {
    std::memcpy(v, q, (size_t)bytes);
    for (int k = 0; k < bytes; ++k) sum += v[k];
  };
  for (int t = 0; t < r.head; ++t) take(p + t * ES, ES);
  for (int64_t i = 0; i < r.nv; ++i) take(p + r.head * ES + 16 * i, 16);
  for (int t = 0; t < r.tail; ++t) take(p + (r.head + r.nv * (16 / ES) + t) * ES, ES);
  return sum;
}

template <int ES>
static int ranges() {
  for (int start = 0; start < 16; start += ES)
    for (int len = 0; len <= 3 * 16 / ES + 3; ++len) {
      // a heap block that ends with the range: `start` zero bytes, then the range's bytes, all 1
      const size_t bytes = (size_t)start + (size_t)len * ES;
      unsigned char* block = static_cast<unsigned char*>(std::malloc(bytes ? bytes : 1));
      if (block == nullptr) return 1;
      std::memset(block, 0, (size_t)start);
      std::memset(block + start, 1, (size_t)len * ES);
      // the split looks at the address's low four bits only: they are `start`
      const sdrint::RangeSplit r = sdrint::split_range<ES>((uintptr_t)(4096 + start), len);
      if (read_as_split<ES>(block + start, r) != (unsigned)len * ES) return 2;   // every byte of the range once
      std::printf("range %d %d %d %d %lld %d\n", ES, start, len, r.head, (long long)r.nv, r.tail);
      std::free(block);
    }
  return 0;
}

int main() {
  static_assert(sdrint::split_range<4>(4, 9).head == 3 && sdrint::split_range<4>(4, 9).nv == 1 && sdrint::split_range<4>(4, 9).tail == 2,
                "usable in a constant expression");
  if (int rc = ranges<2>()) return rc;
  if (int rc = ranges<4>()) return rc;
  return ranges<8>();
}
