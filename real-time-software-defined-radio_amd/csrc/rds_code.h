// The RDS (26, 16) block code, once: the parity matrix, the offset syndromes, the burst table of
// the error corrector, and the window tile of the kernels that scan a bit row (rds.hip's link
// layer, rds_sync.hip's block sync; capi.hip's host link layer takes the host half).  Plain C++17;
// the device functions are under __HIPCC__.  rdssync.py holds the same table as the specification,
// and tests/test_rds_code.py holds this header against it on the host.
//
// Two words name a block's 26 bits.  A *pattern* has the block's first bit as bit 25 (rdssync.py's
// integers, and the burst table's).  A *window* has it as bit 0: what a ballot over the lanes of a
// row gives.  Syndromes are ten bits, column 0 of H the most significant, in both.
#pragma once
#include <cstdint>

namespace sdrint {

// parity matrix H: row j belongs to the block's bit j (rdssync.py _H)
constexpr uint16_t RDS_H[26] = {0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001, 0x2DC, 0x16E, 0x0B7,
                                0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B};
// offset syndromes by type: A, B, C, D, C'
constexpr uint32_t SYN_A = 0x3D8, SYN_B = 0x3D4, SYN_C = 0x25C, SYN_D = 0x258, SYN_CP = 0x3CC;
constexpr int TYPE_NONE = 7, TYPE_CP = 4;

constexpr int type_of(uint32_t s) {
  return s == SYN_A ? 0 : s == SYN_B ? 1 : s == SYN_C ? 2 : s == SYN_D ? 3 : s == SYN_CP ? TYPE_CP : TYPE_NONE;
}
constexpr uint32_t syn_of_type(int t) { return t == 0 ? SYN_A : t == 1 ? SYN_B : t == 2 ? SYN_C : t == 3 ? SYN_D : SYN_CP; }
constexpr int slot_of_type(int t) { return t == TYPE_CP ? 2 : t; }

// column c of H as a mask over a window
constexpr uint32_t col_mask(int c) {
  uint32_t m = 0;
  for (int j = 0; j < 26; ++j) m |= (uint32_t)((RDS_H[j] >> (9 - c)) & 1) << j;
  return m;
}

// the syndrome of a pattern
constexpr uint32_t syndrome(uint32_t pat) {
  uint32_t s = 0;
  for (int j = 0; j < 26; ++j)
    if ((pat >> (25 - j)) & 1u) s ^= RDS_H[j];
  return s;
}

// The burst table, by error syndrome: 1 << 16 | the information bits to flip, 0 = not correctable.
// Every error pattern inside the block whose first and last flipped bits are at most
// max_burst - 1 apart (26 / 51 / 99 / 191 / 367 patterns for 1 .. 5): their syndromes are
// distinct and non-zero, so the table by syndrome is the whole decoder.  Returns whether two
// syndromes collided (they do not for max_burst <= 5; the table is then unusable).
inline bool burst_table(int max_burst, uint32_t (&table)[1024]) {
  for (uint32_t& t : table) t = 0u;
  for (int len = 1; len <= max_burst; ++len) {
    const int inner = len > 2 ? len - 2 : 0;
    for (int first = 0; first + len <= 26; ++first)
      for (uint32_t mid = 0; mid < (1u << inner); ++mid) {
        uint32_t pat = 1u << (25 - first);
        if (len > 1) pat |= 1u << (25 - first - (len - 1));
        for (int k = 0; k < inner; ++k) pat |= ((mid >> k) & 1u) << (25 - first - 1 - k);
        const uint32_t s = syndrome(pat);
        if (s == 0u || table[s] != 0u) return true;
        table[s] = (1u << 16) | (pat >> 10);
      }
  }
  return false;
}

#ifdef __HIPCC__
template <int C>
__device__ __forceinline__ uint32_t parity_col(uint32_t v) {
  constexpr uint32_t m = col_mask(C);
  return (uint32_t)(__popc(v & m) & 1) << (9 - C);
}
// the syndrome of a window
__device__ __forceinline__ uint32_t syndrome_of(uint32_t v) {
  return parity_col<0>(v) | parity_col<1>(v) | parity_col<2>(v) | parity_col<3>(v) | parity_col<4>(v) | parity_col<5>(v) |
         parity_col<6>(v) | parity_col<7>(v) | parity_col<8>(v) | parity_col<9>(v);
}
// The window tile: a workgroup's waves ballot their bits of the row into the 32-bit words dw[]
// (how many words lie in front of the tile, and behind it, is the kernel's), and a thread takes
// the window that starts at bit o of dw[] by a funnel shift.
__device__ __forceinline__ uint32_t window_at(const uint32_t* dw, int o) {
  const int q = o >> 5, sh = o & 31;
  const unsigned long long pair = ((unsigned long long)dw[q + 1] << 32) | dw[q];
  return (uint32_t)(pair >> sh) & 0x3ffffffu;
}
// information word: the window's first 16 bits, the first one most significant
__device__ __forceinline__ uint32_t info_word(uint32_t v) { return __brev(v) >> 16; }
#endif

}  // namespace sdrint
