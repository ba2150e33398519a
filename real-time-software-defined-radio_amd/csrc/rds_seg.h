// What the RDS stages that work by segments share (rds_clock.hip, rds_carrier.hip).  A stream is
// cut into segments of 32 symbols, 768 samples; a call's row of a stream is the carried samples of
// the unfinished segment (and the few a stage keeps in front of it) followed by the caller's.
// Every stream of a call brings the same n, so the host alone keeps the cursor -- segments done,
// the carried tail, which of two slots the carried arrays are read from -- and the kernels get the
// call's geometry by value.  Here: that cursor and the call-time checks; on the device the row
// accessor across the seam, a segment's samples for the f64 sums, the window of per-segment
// records that reaches back into the carried ones, the split of a call's segments into one chunk
// per thread, and the workgroup scan that joins the chunks.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "sdr_ctx.h"

namespace sdrint {

constexpr int SPS = 24, SEG_SYM = 32, SEG = SPS * SEG_SYM;

// a call's geometry, the same for every stream: what the kernels read
struct SegCall {
  int64_t n, stride;
  int64_t seg0;                 // complete segments before this call
  int G, tail;                  // the call's complete segments; the carried samples of the unfinished one
};

// the host's place in the streams
struct SegCursor {
  int64_t seg0 = 0;
  int tail = 0, cur = 0;        // cur: the slot of the two-slot arrays the next call reads; it fills the other
  SegCall begin(int64_t n, int64_t stride) const { return SegCall{n, stride, seg0, (int)((tail + n) / SEG), tail}; }
  // after the call's launches
  void commit(const SegCall& c) {
    cur ^= 1;
    tail = (int)(c.tail + c.n - (int64_t)c.G * SEG);
    seg0 += c.G;
  }
};

// the call-time rules of both stages; rows: {rrc_i} or {rrc_i, rrc_q}
template <class Obj>
int seg_check_call(const Obj* k, std::initializer_list<const float*> rows, int64_t n, int64_t stride, const char* what) {
  if (k == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  const bool two = rows.size() > 1;
  uintptr_t bits = 0;
  for (const float* r : rows) {
    if (r == nullptr) return fail(SDR_EINVAL, "%s: %s is NULL", what, two ? "rrc_i or rrc_q" : "rrc_i");
    bits |= (uintptr_t)r;
  }
  if (n < 0 || n > k->max_n) return fail(SDR_EINVAL, "%s: n=%lld outside [0, max_n=%lld]", what, (long long)n, (long long)k->max_n);
  if (stride < n) return fail(SDR_EINVAL, "%s: stride=%lld < n=%lld", what, (long long)stride, (long long)n);
  if ((bits & 3) != 0) return fail(SDR_EINVAL, "%s: %s must be aligned to 4 B", what, two ? "rrc_i and rrc_q" : "rrc_i");
  return SDR_OK;
}

// sample v of a call's row, -FRONT <= v < tail + n: `carry` holds the FRONT samples a stage keeps
// in front of the unfinished segment, then that segment's
template <int FRONT>
struct SegRow {
  const float* x;
  const float* carry;
  int tail;
  __device__ __forceinline__ float operator()(int64_t v) const { return v < tail ? carry[FRONT + v] : x[v - tail]; }
};

// The samples p, p + 24, ... of segment g, j ascending: f(the sample of each row given).  The
// fast loop where the whole segment lies in the caller's rows, the accessor across the seam.
template <class F, class... Row>
__device__ __forceinline__ void seg_samples(int g, int p, int tail, F&& f, const Row&... row) {
  const int64_t v0 = (int64_t)g * SEG + p;
  if (v0 - p >= tail) {
    const int64_t i0 = v0 - tail;
#pragma unroll 8
    for (int j = 0; j < SEG_SYM; ++j) f(row.x[i0 + SPS * j]...);
  } else {
    for (int j = 0; j < SEG_SYM; ++j) f(row(v0 + SPS * j)...);
  }
}

// A stream's per-segment records, K values of T each: those of the call's segments in `cur`, the
// KEEP before the call carried (zero after a reset).
template <class T, int K, int KEEP>
struct SegWindow {
  const T* cur;
  const T* carried;
  // segment gl of the call, -KEEP <= gl
  __device__ __forceinline__ const T* at(int gl) const { return gl >= 0 ? cur + (int64_t)gl * K : carried + (KEEP + gl) * K; }
  // value i of the next call's carried records, after a call of G segments
  __device__ __forceinline__ T roll(int G, int i) const { return at(G - KEEP + i / K)[i % K]; }
};

// thread tid's chunk [lo, hi) of `count` segments split over nthreads, C to a chunk; the first
// nact threads have one that is not empty
struct SegChunk {
  int C, lo, hi, nact;
};
__device__ __forceinline__ SegChunk chunk_of(int tid, int count, int nthreads) {
  SegChunk c;
  c.C = (count + nthreads - 1) / nthreads;
  c.lo = tid * c.C < count ? tid * c.C : count;
  c.hi = c.lo + c.C < count ? c.lo + c.C : count;
  c.nact = c.C > 0 ? (count + c.C - 1) / c.C : 0;
  return c;
}

// inclusive scan of one value per thread across the first nact threads of the workgroup (two LDS
// slots, log2(nact) rounds); returns the slot that holds the result
template <class T, int NT, class Op>
__device__ __forceinline__ int block_scan(T (*buf)[NT], int tid, int nact, Op op) {
  int cur = 0;
  for (int off = 1; off < nact; off <<= 1) {
    __syncthreads();
    const T mine = buf[cur][tid];
    buf[cur ^ 1][tid] = tid >= off ? op(buf[cur][tid - off], mine) : mine;
    cur ^= 1;
  }
  __syncthreads();
  return cur;
}

}  // namespace sdrint
