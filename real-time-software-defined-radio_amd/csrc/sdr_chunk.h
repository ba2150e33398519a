// What the passes that read a whole contiguous range once share (iqc.hip, ingest.hip, rmeter.hip):
// the range as head elements, 16-B vectors and tail elements (sdr_range.h), the rounds of
// non-temporal loads over it, the lane records' way to one record per workgroup, the one-wave fold
// of those records, and the store of a sample pair.  Every order is fixed: the same calls give the
// same bits.  Not part of the public ABI (include/sdr.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdr_common.h"
#include "sdr_range.h"

namespace sdrint {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// One pass of NL lanes, this one lane t, over the split r of the ES-byte elements at p.  The whole
// vectors go in rounds of U non-temporal loads in flight per lane: vec(x, i) per loaded vector i,
// then round(x, i0) for the round's U vectors from vector i0 on (zeros where the range has ended;
// every lane reaches it, so a wave may exchange its vectors there).  After the rounds one(q) takes
// the head or tail element at q that lane t reads alone.
template <int ES, int NL, int U, class FV, class FR, class F1>
__device__ __forceinline__ void scan_range(const char* p, const RangeSplit& r, int t, FV&& vec, FR&& round, F1&& one) {
  const u4* v = reinterpret_cast<const u4*>(p + (int64_t)r.head * ES);
  for (int64_t i0 = 0; i0 < r.nv; i0 += NL * U) {
    u4 x[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + NL * u + t;
      in[u] = i < r.nv;
      x[u] = in[u] ? __builtin_nontemporal_load(v + i) : u4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (in[u]) vec(x[u], i0 + NL * u + t);
    round(x, i0);
  }
  if (t < r.head) one(p + (int64_t)t * ES);
  if (t < r.tail) one(p + (r.head + r.nv * (16 / ES) + t) * ES);
}
template <int ES, int NL, int U, class FV, class F1>
__device__ __forceinline__ void scan_range(const char* p, const RangeSplit& r, int t, FV&& vec, F1&& one) {
  scan_range<ES, NL, U>(p, r, t, vec, [](const u4 (&)[U], int64_t) {}, one);
}

// the chunk [s0, s0 + len) of workgroup blockIdx.x of a block of n samples of ES bytes, split
template <int ES>
struct Chunk : RangeSplit {
  const char* p;       // the chunk's first sample
  int64_t len;
  __device__ __forceinline__ Chunk(const void* iq, int64_t n, int64_t chunk) {
    const int64_t s0 = (int64_t)blockIdx.x * chunk;
    len = n - s0 < chunk ? n - s0 : chunk;
    p = reinterpret_cast<const char*>(iq) + s0 * ES;
    static_cast<RangeSplit&>(*this) = split_range<ES>((uintptr_t)p, len);   // iq is aligned to one sample
  }
};

// A record of lane partials says how two of it combine: void combine(const R&).  wave_record
// sends it through the butterfly, every field by the same steps as wave_reduce.
template <class R>
__device__ __forceinline__ R wave_record(R r) {
  struct Words {
    uint32_t w[sizeof(R) / 4];
  };
  static_assert(sizeof(R) % 4 == 0 && sizeof(Words) == sizeof(R), "a record is whole dwords");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Words o = __builtin_bit_cast(Words, r);
#pragma unroll
    for (size_t k = 0; k < sizeof(R) / 4; ++k) o.w[k] = __shfl_xor(o.w[k], off, 64);
    r.combine(__builtin_bit_cast(R, o));
  }
  return r;
}

// lane records -> butterfly -> lane 0 of each of the WAVES waves to LDS -> combined in wave order
// 0, 1, .. by thread 0, which hands the workgroup's record to store(r).  No atomics.
template <int WAVES, class R, class S>
__device__ __forceinline__ void block_record(R r, S&& store) {
  __shared__ R wp[WAVES];
  r = wave_record(r);
  if ((threadIdx.x & 63) == 0) wp[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    r = wp[0];
#pragma unroll
    for (int j = 1; j < WAVES; ++j) r.combine(wp[j]);
    store(r);
  }
}

// One wave folds nrec records: the lane takes records lane, lane + 64, .. in ascending order onto
// `id`, the record that changes nothing, U loads (load(b): record b) in flight; then the butterfly.
template <int U, class R, class L>
__device__ __forceinline__ R fold_records(int nrec, int lane, R id, L&& load) {
  R s = id;
  int b = lane;
  for (; b + 64 * (U - 1) < nrec; b += 64 * U) {
    R x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = load(b + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) s.combine(x[u]);
  }
  for (; b < nrec; b += 64) s.combine(load(b));
  return wave_record(s);
}

// two samples = 16 B of output, contiguous across the wave: one 16-B store, or two 8-B halves
// where out's 16-B phase differs from the pairs'
__device__ __forceinline__ void store_pair(float* q, bool out16, const f4 v) {
  if (out16) {
    *reinterpret_cast<f4*>(q) = v;
  } else {
    *reinterpret_cast<f2*>(q) = f2{v.x, v.y};
    *reinterpret_cast<f2*>(q + 2) = f2{v.z, v.w};
  }
}

// ---- the cut of a capture block (at most CAPTURE_MAX_N samples) into chunks, host ---------------
constexpr int64_t CAPTURE_MAX_N = INT32_MAX;
// the chunk of a block of n samples: whole 16-B vectors of any sample type, at most max_wg of them,
// none shorter than min_chunk but the last
constexpr int64_t chunk_len(int64_t n, int64_t min_chunk, int max_wg) {
  const int64_t per = ((n + max_wg - 1) / max_wg + 7) / 8 * 8;
  return per > min_chunk ? per : min_chunk;
}
inline int chunks_of(int64_t n, int64_t min_chunk, int max_wg, int64_t* chunk) {
  *chunk = chunk_len(n, min_chunk, max_wg);
  return (int)((n + *chunk - 1) / *chunk);
}
// the largest chunk chunks_of can return
constexpr int64_t max_chunk(int64_t min_chunk, int max_wg) { return chunk_len(CAPTURE_MAX_N, min_chunk, max_wg); }
// the most samples one of NL lanes takes of a chunk, V samples a vector: its vectors', a head and
// a tail sample -- what an exact 32-bit lane partial must hold
constexpr int64_t lane_share(int64_t chunk, int V, int NL) { return (chunk / V + NL - 1) / NL * V + 2; }

}  // namespace sdrint
