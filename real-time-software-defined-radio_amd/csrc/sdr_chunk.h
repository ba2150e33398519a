// What the passes over a whole capture block share (iqc.hip, ingest.hip): the block cut into
// chunks of whole 16-B vectors, one workgroup each, and the wave sum of their lane partials.
// Not part of the public ABI (include/sdr.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace sdrint {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

template <class T>
__device__ __forceinline__ T wave_sum64(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // the same order in every lane
  return v;
}

// the chunk [s0, s0 + len) of workgroup blockIdx.x as head samples, 16-B vectors and tail samples;
// ES: bytes of a complex sample
template <int ES>
struct Chunk {
  const char* p;       // the chunk's first sample
  int64_t len, nv;     // samples; whole 16-B vectors
  int head, tail;      // samples before the first vector (< 16 / ES) and after the last
  __device__ __forceinline__ Chunk(const void* iq, int64_t n, int64_t chunk) {
    constexpr int V = 16 / ES;
    const int64_t s0 = (int64_t)blockIdx.x * chunk;
    len = n - s0 < chunk ? n - s0 : chunk;
    p = reinterpret_cast<const char*>(iq) + s0 * ES;
    const int mis = (int)((uintptr_t)p & 15);                      // a multiple of ES: iq is aligned to one sample
    const int64_t h = mis ? (16 - mis) / ES : 0;
    head = (int)(h < len ? h : len);
    nv = (len - head) / V;
    tail = (int)(len - head - nv * V);
  }
  __device__ __forceinline__ const u4* vec() const { return reinterpret_cast<const u4*>(p + (int64_t)head * ES); }
  // the sample this thread takes alone, if any: k = 0 head, k = 1 tail
  __device__ __forceinline__ const char* single(int k) const {
    const int t = threadIdx.x;
    if (k == 0) return t < head ? p + (int64_t)t * ES : nullptr;
    return t < tail ? p + (head + nv * (16 / ES) + t) * ES : nullptr;
  }
};

// a block of n samples as at most max_wg chunks of whole 16-B vectors of any sample type, none
// shorter than min_chunk but the last; returns the number of chunks
inline int chunks_of(int64_t n, int64_t min_chunk, int max_wg, int64_t* chunk) {
  const int64_t per = ((n + max_wg - 1) / max_wg + 7) / 8 * 8;
  *chunk = std::max<int64_t>(per, min_chunk);
  return (int)((n + *chunk - 1) / *chunk);
}

}  // namespace sdrint
