// Wideband spectrum / waterfall (include/sdr.h sdr_spec_*): Welch periodogram rows of one
// interleaved-IQ capture in device memory, read in place.  With segment s starting at sample
// s hop, window w and N = nfft,
//   X_s[k]    = sum_{i < N} w[i] x[s hop + i] exp(-2 pi i k i / N)
//   out[r][j] = (1 / (navg (sum w)^2)) sum_{s in row r} |X_s[k]|^2,   k = (j + N / 2) mod N
// in f32, bin j centred on (j - N / 2) fs / N.
//
// The transform is a Stockham autosort FFT in f32 with the butterflies in registers: passes of
// radix 16 and 8 (and one of 4 at 8 192 points), two or three LDS round trips per transform (four
// at 8 192) instead of log2 N.  In a pass of radix R after passes whose radices multiply to Ns,
// butterfly j < N / R takes the points j + r N / R, turns point r by exp(-2 pi i r k / (Ns R)),
// k = j mod Ns, and writes its outputs to (j - k) R + k + r Ns.  The turns come from the table
// exp(-2 pi i t / N), t < N, computed on the host in f64: the entries for r = 1, 2, 3 and 4, 8, 12
// are read and the other nine are one complex product of two of them.  The radix-16 butterfly is
// four radix-4 ones, the constant turns exp(-2 pi i m / 16), and four more.
//
// Work: a workgroup of 256 threads (512 at 8 192 points) takes one chunk of one row: up to
// `chunk` consecutive segments (a row of more than SDR_SPEC_SPLIT_SEGS segments may be cut into
// several chunks, see sdr_spec_process_dev).  It transforms SPEC_TILE / N segments at a time
// ("slots"; one segment of fewer than 4 096 points would leave most threads idle), so that every
// thread holds 16 points -- one radix-16 butterfly, or two of radix 8:
//   pass 1  reads the samples from global memory straight into the butterfly's registers and
//           applies the window.  f32: 16 bytes per lane -- the lanes 2 t, 2 t + 1 hold butterflies
//           j, j + 1 of one slot, each loads two neighbouring samples of every other point and
//           the pair exchanges halves across lanes; the load is one instruction at either
//           alignment of the pair's address (8 or 16 bytes).  u8: the slot's 2 N bytes are
//           first copied into LDS in 16-byte pieces (the ends in 2-byte ones), and the pass
//           reads 2 bytes per point from there.  No access leaves the segment's own samples.
//   others  read the points from LDS, turn, transform, write them back (row index i kept at
//           i + (i >> 4) complex samples: the first pass's stride-R writes then spread over all
//           banks).  One buffer: a barrier between a pass's reads and its writes.
//   last    does not write: every thread adds |X|^2 of the bins it holds to its registers (the
//           same bins in every round, since the thread-to-butterfly map is fixed).
// After the chunk's last round the registers go to LDS and bin k is summed over the slots in
// slot order -- a fixed order, no atomics -- scaled and stored at j = (k + N / 2) mod N of the
// output row, or unscaled into the chunk's row of the partial sums where the row has several
// chunks; a second launch then adds a row's chunks in chunk order.  Segments that overlap
// (hop < N) are fetched by the same workgroup in the same or the next round, so the second fetch
// is served by the caches, not by HBM; nothing is kept in LDS between rounds.
//
// Rows of real samples (include/sdr.h sdr_rspec_*; a receiver's demodulated rows): rspec_kernel
// below, the same passes with two real segments per complex transform and a one-sided store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "sdr_ctx.h"
#include "sdr_launch.h"

using namespace sdrint;

namespace {

constexpr int SPEC_TILE = 4096;                    // points a workgroup transforms at a time (N if larger)
constexpr int64_t SPEC_TARGET_CHUNKS = 2048;       // chunks a call is cut into at most, beyond one per row
constexpr int SPEC_RED_BINS = 16, SPEC_RED_GROUPS = 16;   // the second launch: bins and chunk groups of a workgroup
// threads of a workgroup: one radix-16 butterfly each (256; 512 at 8 192 points)
constexpr int spec_threads(int N) { return (N > SPEC_TILE ? N : SPEC_TILE) / 16; }

// radices of the passes for N = 2^(6 + i)
constexpr int kSpecPasses[8] = {2, 2, 2, 3, 3, 3, 3, 4};
constexpr int kSpecRadix[8][4] = {{8, 8, 1, 1},   {16, 8, 1, 1},  {16, 16, 1, 1},  {8, 8, 8, 1},
                                  {16, 8, 8, 1},  {16, 16, 8, 1}, {16, 16, 16, 1}, {16, 16, 8, 4}};

struct SpecArgs {
  const void* iq;
  const float* win;        // [N]
  const float2* tw;        // [N]: exp(-2 pi i t / N)
  float* dst;              // the output rows, or the partial sums [rows cpr][N]
  int64_t dst_stride;      // floats between rows of dst
  int64_t hop;
  int64_t navg;            // segments per row
  int64_t chunk;           // segments per chunk
  int64_t cpr;             // chunks per row
  float scale;             // 1 / (navg (sum w)^2), or 1 for partial sums
};

static __device__ __forceinline__ float2 cadd(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
static __device__ __forceinline__ float2 csub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
static __device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return float2{fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y)};
}
// v exp(-2 pi i m / 16); m is a constant wherever this is called (unrolled loops)
static __device__ __forceinline__ float2 cmul_w16(float2 v, int m) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
  constexpr float cs[16] = {1.f, C1, H, S1, 0.f, -S1, -H, -C1, -1.f, -C1, -H, -S1, 0.f, S1, H, C1};
  constexpr float sn[16] = {0.f, S1, H, C1, 1.f, C1, H, S1, 0.f, -S1, -H, -C1, -1.f, -C1, -H, -S1};
  m &= 15;
  if (m == 0) return v;
  if (m == 4) return float2{v.y, -v.x};
  if (m == 8) return float2{-v.x, -v.y};
  if (m == 12) return float2{-v.y, v.x};
  return cmul(v, float2{cs[m], -sn[m]});
}

template <int R>
static __device__ __forceinline__ void fft_r(float2* v);
template <>
__device__ __forceinline__ void fft_r<1>(float2*) {}
template <>
__device__ __forceinline__ void fft_r<2>(float2* v) {
  const float2 a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}
template <>
__device__ __forceinline__ void fft_r<4>(float2* v) {
  const float2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), d = csub(v[1], v[3]);
  const float2 t3 = float2{d.y, -d.x};   // -i d
  v[0] = cadd(t0, t2);
  v[1] = cadd(t1, t3);
  v[2] = csub(t0, t2);
  v[3] = csub(t1, t3);
}
// R = 4 R2: point r = R2 a + b, output q = q1 + 4 q2:  exp(-2 pi i r q / R) =
// exp(-2 pi i a q1 / 4) exp(-2 pi i b q1 / R) exp(-2 pi i b q2 / R2)
template <int R>
static __device__ __forceinline__ void fft_r(float2* v) {
  constexpr int R2 = R / 4;
  float2 u[R];
#pragma unroll
  for (int b = 0; b < R2; ++b) {
    float2 t[4] = {v[b], v[R2 + b], v[2 * R2 + b], v[3 * R2 + b]};
    fft_r<4>(t);
#pragma unroll
    for (int q1 = 0; q1 < 4; ++q1) u[q1 * R2 + b] = cmul_w16(t[q1], b * q1 * (16 / R));
  }
#pragma unroll
  for (int q1 = 0; q1 < 4; ++q1) {
    fft_r<R2>(u + q1 * R2);
#pragma unroll
    for (int q2 = 0; q2 < R2; ++q2) v[q1 + 4 * q2] = u[q1 * R2 + q2];
  }
}

static __device__ __forceinline__ int spec_pad(int i) { return i + (i >> 4); }

// One pass of radix R after passes of total radix NS, for the workgroup's B slots of N points.
// FIRST: the points come from `ld(slot, j, v)` (window applied); LAST: |X|^2 is added to acc and
// nothing is written.
template <int N, int B, int SPEC_THREADS, int R, int NS, bool FIRST, bool LAST, class Load>
static __device__ __forceinline__ void spec_pass(float2* data, const float2* __restrict__ tw, float* acc, Load ld) {
  constexpr int S = N / R;                               // butterflies per slot = the points' stride
  constexpr int IT = B * S / SPEC_THREADS;               // butterflies per thread (one of radix 16)
  static_assert(IT >= 1 && IT * SPEC_THREADS == B * S, "every thread holds the same number of butterflies");
  const int tid = threadIdx.x;
  float2 v[IT][R];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int b = tid + it * SPEC_THREADS;
    const int slot = b / S, j = b % S;
    if constexpr (FIRST) {
      ld(slot, j, v[it]);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) v[it][r] = data[spec_pad(slot * N + j + r * S)];
      // the turns exp(-2 pi i r k / (NS R)) = tw[r kb], kb = k N / (NS R) < N / R
      const int kb = (j & (NS - 1)) * (N / (NS * R));
      float2 w[R];
#pragma unroll
      for (int r = 1; r < R; ++r)
        if (r < 4 || (r & 3) == 0) w[r] = tw[r * kb];
#pragma unroll
      for (int r = 5; r < R; ++r)
        if ((r & 3) != 0) w[r] = cmul(w[r & ~3], w[r & 3]);
#pragma unroll
      for (int r = 1; r < R; ++r) v[it][r] = cmul(v[it][r], w[r]);
    }
    fft_r<R>(v[it]);
  }
  if constexpr (LAST) {
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[it * R + r] = fmaf(v[it][r].x, v[it][r].x, fmaf(v[it][r].y, v[it][r].y, acc[it * R + r]));
  } else {
    __syncthreads();                                     // every read of the previous contents is done
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int b = tid + it * SPEC_THREADS;
      const int slot = b / S, j = b % S;
        const int k = j & (NS - 1);
      const int j0 = (j - k) * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) data[spec_pad(slot * N + j0 + r * NS)] = v[it][r];
    }
    __syncthreads();
  }
}

// The passes of one round: the workgroup's B slots, the points from `ld` (see spec_pass), |X|^2
// added to acc.  (The first pass's barrier between its loads and its writes: the previous round's
// last pass has read `data`.)
template <int LOGN, class Load>
static __device__ __forceinline__ void spec_passes(float2* data, const float2* __restrict__ tw, float* acc, Load load) {
  constexpr int N = 1 << LOGN;
  constexpr int SPEC_THREADS = spec_threads(N);
  constexpr int B = N >= SPEC_TILE ? 1 : SPEC_TILE / N;
  constexpr int NP = kSpecPasses[LOGN - 6];
  constexpr int R0 = kSpecRadix[LOGN - 6][0], R1 = kSpecRadix[LOGN - 6][1], R2 = kSpecRadix[LOGN - 6][2],
                R3 = kSpecRadix[LOGN - 6][3];
  auto none = [](int, int, float2*) {};
  spec_pass<N, B, SPEC_THREADS, R0, 1, true, false>(data, tw, acc, load);
  if constexpr (NP == 2) {
    spec_pass<N, B, SPEC_THREADS, R1, R0, false, true>(data, tw, acc, none);
  } else if constexpr (NP == 3) {
    spec_pass<N, B, SPEC_THREADS, R1, R0, false, false>(data, tw, acc, none);
    spec_pass<N, B, SPEC_THREADS, R2, R0 * R1, false, true>(data, tw, acc, none);
  } else {
    spec_pass<N, B, SPEC_THREADS, R1, R0, false, false>(data, tw, acc, none);
    spec_pass<N, B, SPEC_THREADS, R2, R0 * R1, false, false>(data, tw, acc, none);
    spec_pass<N, B, SPEC_THREADS, R3, R0 * R1 * R2, false, true>(data, tw, acc, none);
  }
}

// After a chunk's last round: acc[it RL + r] is bin j + r N / RL of slot b / (N / RL),
// b = tid + 256 it; all of them to LDS as sums[slot N + k]
template <int LOGN>
static __device__ __forceinline__ const float* spec_sums(float2* data, const float* acc) {
  constexpr int N = 1 << LOGN;
  constexpr int SPEC_THREADS = spec_threads(N);
  constexpr int B = N >= SPEC_TILE ? 1 : SPEC_TILE / N;
  constexpr int RL = kSpecRadix[LOGN - 6][kSpecPasses[LOGN - 6] - 1];   // the last pass's radix
  constexpr int SL = N / RL;
  constexpr int ITL = B * SL / SPEC_THREADS;
  const int tid = threadIdx.x;
  float* sums = reinterpret_cast<float*>(data);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITL; ++it) {
    const int b = tid + it * SPEC_THREADS;
    const int slot = b / SL, j = b % SL;
#pragma unroll
    for (int r = 0; r < RL; ++r) sums[slot * N + j + r * SL] = acc[it * RL + r];
  }
  __syncthreads();
  return sums;
}

template <int LOGN, bool U8>
__global__ __launch_bounds__(spec_threads(1 << LOGN)) void spec_kernel(const SpecArgs P) {
  constexpr int N = 1 << LOGN;
  constexpr int SPEC_THREADS = spec_threads(N);
  constexpr int B = N >= SPEC_TILE ? 1 : SPEC_TILE / N;   // slots
  constexpr int R0 = kSpecRadix[LOGN - 6][0];
  constexpr int NACC = B * N / SPEC_THREADS;             // bins a thread accumulates (16)
  constexpr int DATA = B * N + B * N / 16;               // complex samples of the padded buffer
  constexpr int RAWS = N + 16;                           // u8: 2-byte samples per slot of the raw copy (2 N + 32 bytes)
  extern __shared__ __attribute__((aligned(16))) unsigned char spec_lds[];   // spec_lds_bytes(): one array
  float2* data = reinterpret_cast<float2*>(spec_lds);
  [[maybe_unused]] uint16_t* raw = reinterpret_cast<uint16_t*>(spec_lds + (size_t)DATA * sizeof(float2));

  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / P.cpr, ch = (int64_t)blockIdx.x % P.cpr;
  const int64_t c0 = row * P.navg + ch * P.chunk;                                 // first segment
  const int64_t c1 = std::min<int64_t>(c0 + P.chunk, (row + 1) * P.navg);         // one past the last
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;

  for (int64_t sb = c0; sb < c1; sb += B) {
    if constexpr (U8) {
      // the raw copy: slot s's bytes [A - a, A - a + 2 N + 32) -> raw, A the segment's address
      // and a = A mod 16; only bytes [A, A + 2 N) are read
      constexpr int CH = RAWS / 8;                       // 16-byte pieces per slot
      for (int i = tid; i < B * CH; i += SPEC_THREADS) {
        const int slot = i / CH, c = i % CH;
        if (sb + slot >= c1) continue;
        const unsigned char* A = reinterpret_cast<const unsigned char*>(P.iq) + 2 * ((sb + slot) * P.hop);
        const int a = (int)((uintptr_t)A & 15);
        const unsigned char* g = A - a + 16 * c;
        uint16_t* l = raw + slot * RAWS + 8 * c;
        if (16 * c >= a && 16 * c + 16 <= a + 2 * N) {
          *reinterpret_cast<uint4*>(l) = *reinterpret_cast<const uint4*>(g);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int off = 16 * c + 2 * e;
            if (off >= a && off < a + 2 * N) l[e] = *reinterpret_cast<const uint16_t*>(g + 2 * e);
          }
        }
      }
      __syncthreads();                                   // (also: the previous round's last pass has read `data`)
    }
    auto load = [&](int slot, int j, float2* v) {
      constexpr int S = N / R0;
      const int64_t seg = sb + slot;
      const bool on = seg < c1;
      if constexpr (U8) {
        const unsigned char* A = reinterpret_cast<const unsigned char*>(P.iq) + 2 * (seg * P.hop);
        const uint16_t* l = raw + slot * RAWS + (int)(((uintptr_t)A & 15) >> 1) + j;
#pragma unroll
        for (int r = 0; r < R0; ++r) {
          const uint32_t q = on ? l[r * S] : 0x8080u;
          const float w = P.win[j + r * S];
          v[r] = float2{((float)(q & 255u) - 128.f) * (1.f / 128.f) * w, ((float)(q >> 8) - 128.f) * (1.f / 128.f) * w};
        }
      } else {
        // lanes 2 t, 2 t + 1 (butterflies je, je + 1 of one slot): the lane of parity p loads the
        // samples je, je + 1 of the points r = 2 i + p, keeps its own and hands over the other
        const int p = j & 1, je = j & ~1;
        const float2* x = reinterpret_cast<const float2*>(P.iq) + seg * P.hop + je;
#pragma unroll
        for (int i = 0; i < R0 / 2; ++i) {
          // two neighbouring samples: one 16-byte load (global_load_dwordx4), which the hardware
          // takes at the samples' 8-byte alignment too -- no second path for odd addresses
          const float2* src = x + (2 * i + p) * S;
          float4 q = float4{0.f, 0.f, 0.f, 0.f};
          if (on) {
            const float2 s0 = src[0], s1 = src[1];
            q = float4{s0.x, s0.y, s1.x, s1.y};
          }
          const float2 keep = p ? float2{q.z, q.w} : float2{q.x, q.y};
          const float2 send = p ? float2{q.x, q.y} : float2{q.z, q.w};
          const float2 recv = float2{__shfl_xor(send.x, 1), __shfl_xor(send.y, 1)};
          v[2 * i] = p ? recv : keep;
          v[2 * i + 1] = p ? keep : recv;
        }
#pragma unroll
        for (int r = 0; r < R0; ++r) {
          const float w = P.win[j + r * S];
          v[r] = float2{v[r].x * w, v[r].y * w};
        }
      }
    };
    spec_passes<LOGN>(data, P.tw, acc, load);
  }

  // bin k summed over the slots in slot order
  const float* sums = spec_sums<LOGN>(data, acc);
  float* drow = P.dst + (P.cpr > 1 ? (int64_t)blockIdx.x : row) * P.dst_stride;
  for (int k = tid; k < N; k += SPEC_THREADS) {
    float s = sums[k];
#pragma unroll
    for (int slot = 1; slot < B; ++slot) s += sums[slot * N + k];
    drow[(k + N / 2) & (N - 1)] = s * P.scale;
  }
}

// ---- rows of real samples (sdr_rspec) ----------------------------------------------------------
// The same transform for `nrows` rows of real f32 samples, one-sided:
//   out[q][r][k] = (c_k / (navg (sum w)^2)) sum_{s in row r} |X_{q,s}[k]|^2,  k = 0 .. N / 2,
//   c_0 = c_{N/2} = 1, otherwise 2.
// Two segments a, b of one row go through one complex transform, Z = FFT(w (a + i b)): for real a
// and b, |A[k]|^2 + |B[k]|^2 = (|Z[k]|^2 + |Z[N - k]|^2) / 2, so the passes and the accumulation
// are spec_kernel's and only the final store differs: it folds bin k with N - k (and stores the
// N / 2 + 1 sums where they are, not rotated).  A chunk's segments are paired in order, c0 + 2 p
// with c0 + 2 p + 1: a pair never leaves its chunk, and an odd chunk's last segment is paired with
// zeros.  A slot is one pair, so a round takes 2 B segments.
struct RSpecArgs {
  const float* x;          // row q starts q in_stride floats in
  const float* win;        // [N]
  const float2* tw;        // [N]: exp(-2 pi i t / N)
  float* dst;              // the output rows, or the partial sums [nrows rows cpr][dst_stride]
  int64_t dst_stride;      // floats between rows of dst
  int64_t in_stride;
  int64_t hop;
  int64_t rows;            // output rows per input row
  int64_t navg;            // segments per output row
  int64_t chunk;           // segments per chunk
  int64_t cpr;             // chunks per output row
  float scale;             // 1 / (navg (sum w)^2), or 1 for partial sums
};

// two neighbouring samples of a row at the row's own 4-byte alignment: one 8-byte load
// (global_load_dwordx2), which the hardware takes at any dword address
struct __attribute__((packed, aligned(4))) RSpecPair {
  float a, b;
};

template <int LOGN>
__global__ __launch_bounds__(spec_threads(1 << LOGN)) void rspec_kernel(const RSpecArgs P) {
  constexpr int N = 1 << LOGN;
  constexpr int SPEC_THREADS = spec_threads(N);
  constexpr int B = N >= SPEC_TILE ? 1 : SPEC_TILE / N;   // slots: pairs of segments
  constexpr int R0 = kSpecRadix[LOGN - 6][0];
  constexpr int NACC = B * N / SPEC_THREADS;
  extern __shared__ __attribute__((aligned(16))) unsigned char spec_lds[];
  float2* data = reinterpret_cast<float2*>(spec_lds);

  const int tid = threadIdx.x;
  const int64_t orow = (int64_t)blockIdx.x / P.cpr, ch = (int64_t)blockIdx.x % P.cpr;   // orow = q rows + r
  const int64_t q = orow / P.rows, row = orow % P.rows;
  const float* xq = P.x + q * P.in_stride;
  const int64_t c0 = row * P.navg + ch * P.chunk;                                 // first segment
  const int64_t c1 = std::min<int64_t>(c0 + P.chunk, (row + 1) * P.navg);         // one past the last
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  // The window values of the thread's points, read once: every butterfly of a thread has the same
  // j (the workgroup's size is a multiple of N / R0).  With the 8-byte sample loads a round has
  // twice spec_kernel's sample load instructions, and vector memory instructions, not bytes, are
  // what a round waits for; this takes R0 of them out of every round.
  constexpr int S0 = N / R0;
  static_assert(SPEC_THREADS % S0 == 0, "j = tid mod S0 in every butterfly of a thread");
  float wv[R0];
#pragma unroll
  for (int r = 0; r < R0; ++r) wv[r] = P.win[tid % S0 + r * S0];

  for (int64_t sb = c0; sb < c1; sb += 2 * B) {
    // lanes 2 t, 2 t + 1 (butterflies je, je + 1 of one slot): the even lane loads the samples
    // je, je + 1 of every point of segment a, the odd lane those of segment b; each keeps its own
    // butterfly's sample and hands over the other.  A segment at or past c1 reads nothing and
    // counts as zeros.
    auto load = [&](int slot, int j, float2* v) {
      constexpr int S = N / R0;
      const int p = j & 1, je = j & ~1;
      const int64_t seg = sb + 2 * slot + p;
      const bool on = seg < c1;
      const float* src = xq + seg * P.hop + je;
      RSpecPair s[R0];
#pragma unroll
      for (int r = 0; r < R0; ++r) s[r] = RSpecPair{0.f, 0.f};
      if (on) {
#pragma unroll
        for (int r = 0; r < R0; ++r) s[r] = *reinterpret_cast<const RSpecPair*>(src + r * S);
      }
#pragma unroll
      for (int r = 0; r < R0; ++r) {
        const float keep = p ? s[r].b : s[r].a;
        const float recv = __shfl_xor(p ? s[r].a : s[r].b, 1);
        v[r] = p ? float2{recv * wv[r], keep * wv[r]} : float2{keep * wv[r], recv * wv[r]};
      }
    };
    spec_passes<LOGN>(data, P.tw, acc, load);
  }

  // bins k and N - k summed over the slots in slot order, then added
  const float* sums = spec_sums<LOGN>(data, acc);
  float* drow = P.dst + (int64_t)blockIdx.x * P.dst_stride;   // the chunk's row of the partial sums; cpr == 1: row orow of out
  for (int k = tid; k <= N / 2; k += SPEC_THREADS) {
    const int km = (N - k) & (N - 1);
    float s = sums[k], sm = sums[km];
#pragma unroll
    for (int slot = 1; slot < B; ++slot) {
      s += sums[slot * N + k];
      sm += sums[slot * N + km];
    }
    drow[k] = (km == k ? s : s + sm) * P.scale;
  }
}

// out[row][j] = scale sum_c part[row cpr + c][j], j < nbins, in a fixed order: thread (g, j) of a
// workgroup adds the chunks g, g + 16, ... of one of its 16 bins in chunk order, then the 16
// groups' sums are added in group order.  N: the floats between the chunks' rows of part, a
// multiple of 16
__global__ __launch_bounds__(SPEC_RED_BINS * SPEC_RED_GROUPS) void spec_reduce_kernel(const float* __restrict__ part, float* out,
                                                                                      int N, int nbins, int64_t cpr,
                                                                                      int64_t out_stride, float scale) {
  __shared__ float sums[SPEC_RED_GROUPS][SPEC_RED_BINS];
  const int64_t row = blockIdx.y;
  const int b = threadIdx.x % SPEC_RED_BINS, g = threadIdx.x / SPEC_RED_BINS;
  const int j = blockIdx.x * SPEC_RED_BINS + b;            // < N
  const float* p = part + row * cpr * N + j;
  float s = 0.f;
  if (j < nbins) {
#pragma unroll 8
    for (int64_t c = g; c < cpr; c += SPEC_RED_GROUPS) s += p[c * N];
  }
  sums[g][b] = s;
  __syncthreads();
  if (g == 0 && j < nbins) {
#pragma unroll
    for (int q = 1; q < SPEC_RED_GROUPS; ++q) s += sums[q][b];
    out[row * out_stride + j] = s * scale;
  }
}

// the LDS of a launch: the padded points, then (u8) the raw copy of every slot
size_t spec_lds_bytes(int N, bool u8) {
  const int tile = std::max(N, SPEC_TILE);
  return (size_t)(tile + tile / 16) * sizeof(float2) + (u8 ? (size_t)(tile / N) * (2 * N + 32) : 0);
}

template <class Args>
void spec_launch1(void (*kern)(Args), int N, bool u8, unsigned grid, const Args& P, hipStream_t st) {
  const size_t lds = spec_lds_bytes(N, u8);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<grid, spec_threads(N), lds, st>>>(P);
}

template <bool U8>
void spec_launch(int logn, unsigned grid, const SpecArgs& P, hipStream_t st) {
  switch (logn) {
    case 6: spec_launch1(&spec_kernel<6, U8>, 1 << 6, U8, grid, P, st); break;
    case 7: spec_launch1(&spec_kernel<7, U8>, 1 << 7, U8, grid, P, st); break;
    case 8: spec_launch1(&spec_kernel<8, U8>, 1 << 8, U8, grid, P, st); break;
    case 9: spec_launch1(&spec_kernel<9, U8>, 1 << 9, U8, grid, P, st); break;
    case 10: spec_launch1(&spec_kernel<10, U8>, 1 << 10, U8, grid, P, st); break;
    case 11: spec_launch1(&spec_kernel<11, U8>, 1 << 11, U8, grid, P, st); break;
    case 12: spec_launch1(&spec_kernel<12, U8>, 1 << 12, U8, grid, P, st); break;
    default: spec_launch1(&spec_kernel<13, U8>, 1 << 13, U8, grid, P, st); break;
  }
}

void rspec_launch(int logn, unsigned grid, const RSpecArgs& P, hipStream_t st) {
  switch (logn) {
    case 6: spec_launch1(&rspec_kernel<6>, 1 << 6, false, grid, P, st); break;
    case 7: spec_launch1(&rspec_kernel<7>, 1 << 7, false, grid, P, st); break;
    case 8: spec_launch1(&rspec_kernel<8>, 1 << 8, false, grid, P, st); break;
    case 9: spec_launch1(&rspec_kernel<9>, 1 << 9, false, grid, P, st); break;
    case 10: spec_launch1(&rspec_kernel<10>, 1 << 10, false, grid, P, st); break;
    case 11: spec_launch1(&rspec_kernel<11>, 1 << 11, false, grid, P, st); break;
    case 12: spec_launch1(&rspec_kernel<12>, 1 << 12, false, grid, P, st); break;
    default: spec_launch1(&rspec_kernel<13>, 1 << 13, false, grid, P, st); break;
  }
}

// what sdr_spec and sdr_rspec share: the transform's size, the segments' geometry, the tables
struct SpecBase {
  sdr_ctx* ctx = nullptr;
  int N = 0, logn = 0;
  int64_t hop = 0, navg = 0;
  double wsum = 0.0;
  float* win = nullptr;
  float2* tw = nullptr;
};

// a create's argument rules (before the context is looked at): w = the window in f64
int spec_check_create(int nfft, const double* window, int64_t hop, int64_t navg, std::vector<double>& w, double* wsum,
                      const char* what) {
  if (nfft < SDR_SPEC_MIN_NFFT || nfft > SDR_SPEC_MAX_NFFT || (nfft & (nfft - 1)) != 0)
    return fail(SDR_EINVAL, "%s: nfft=%d must be a power of two in [%d, %d]", what, nfft, SDR_SPEC_MIN_NFFT, SDR_SPEC_MAX_NFFT);
  if (hop < 1 || hop > SDR_SPEC_MAX_HOP) return fail(SDR_EINVAL, "%s: hop=%lld outside [1, %d]", what, (long long)hop, SDR_SPEC_MAX_HOP);
  if (navg < 0) return fail(SDR_EINVAL, "%s: navg=%lld must be 0 (one row) or >= 1", what, (long long)navg);
  w.resize(nfft);
  *wsum = 0.0;
  for (int i = 0; i < nfft; ++i) {
    w[i] = window != nullptr ? window[i] : 0.5 - 0.5 * std::cos(two_pi * (double)i / (double)nfft);   // periodic Hann
    if (!std::isfinite(w[i])) return fail(SDR_EINVAL, "%s: window[%d] is not finite", what, i);
    *wsum += w[i];
  }
  if (*wsum == 0.0 || !std::isfinite(*wsum * *wsum)) return fail(SDR_EINVAL, "%s: the window sums to %g", what, *wsum);
  return SDR_OK;
}

// fills the object and uploads its tables (the f32 window, the turns computed in f64)
hipError_t spec_init(SpecBase* d, sdr_ctx* c, const std::vector<double>& w, double wsum, int64_t hop, int64_t navg) {
  const int nfft = (int)w.size();
  d->ctx = c;
  d->N = nfft;
  while ((1 << d->logn) < nfft) ++d->logn;
  d->hop = hop;
  d->navg = navg;
  d->wsum = wsum;
  std::vector<float> w32(nfft);
  std::vector<float2> tw(nfft);
  for (int i = 0; i < nfft; ++i) {
    w32[i] = (float)w[i];
    const double th = two_pi * (double)i / (double)nfft;
    tw[i] = float2{(float)std::cos(th), (float)-std::sin(th)};
  }
  hipError_t e = upload(&d->win, w32.data(), w32.size(), c->stream);
  if (e == hipSuccess) e = upload(&d->tw, tw.data(), tw.size(), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host vectors are read until here)
  return e;
}

void spec_free(SpecBase* d) {
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  (void)hipFree(d->win);
  (void)hipFree(d->tw);
}

// the rows of a call of n samples (per input row); navg_eff: the segments of an output row
int spec_geom(const SpecBase* d, int64_t n, int64_t* nseg, int64_t* rows, int64_t* navg_eff, const char* what) {
  if (n < d->N) return fail(SDR_EINVAL, "%s: n=%lld < nfft=%d", what, (long long)n, d->N);
  *nseg = (n - d->N) / d->hop + 1;
  *navg_eff = d->navg > 0 ? d->navg : *nseg;
  *rows = *nseg / *navg_eff;
  if (*rows < 1)
    return fail(SDR_EINVAL, "%s: n=%lld yields %lld segments, no complete row of navg=%lld", what, (long long)n, (long long)*nseg,
                (long long)d->navg);
  return SDR_OK;
}

// An output row of up to SDR_SPEC_SPLIT_SEGS segments is one chunk.  A longer one is cut so that
// the call -- `segs` segments in all its rows -- has about SPEC_TARGET_CHUNKS chunks (enough
// workgroups for one row of a long capture) of at least SDR_SPEC_SPLIT_SEGS segments (the partial
// sums stay below an eighth of the capture's bytes), the chunks of a row equal in length to
// within one segment.  The rule uses nothing of the device: the same call sums in the same order
// everywhere.  (cpr > 1: navg > lmin >= segs / SPEC_TARGET_CHUNKS, so the call has fewer than
// SPEC_TARGET_CHUNKS output rows: they fit the second launch's grid y.)
void spec_chunks(int64_t segs, int64_t navg, int64_t* cpr, int64_t* chunk) {
  const int64_t lmin = std::max<int64_t>(SDR_SPEC_SPLIT_SEGS, ceil_div(segs, SPEC_TARGET_CHUNKS));
  *cpr = ceil_div(navg, lmin);
  *chunk = ceil_div(navg, *cpr);
}

}  // namespace

struct sdr_spec : SpecBase {
  int dtype = 0;
};

struct sdr_rspec : SpecBase {
  int nrows = 0;
};

static int spec_check_call(sdr_spec* d, const void* iq, int64_t n, const float* out, int64_t out_stride, const char* what) {
  if (d == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (iq == nullptr || out == nullptr) return fail(SDR_EINVAL, "%s: iq or out is NULL", what);
  int64_t nseg, rows, na;
  TRY(spec_geom(d, n, &nseg, &rows, &na, what));
  if (out_stride < d->N) return fail(SDR_EINVAL, "%s: out_stride=%lld < nfft=%d", what, (long long)out_stride, d->N);
  return SDR_OK;
}

static int rspec_check_call(sdr_rspec* d, const float* x, int64_t n, int64_t in_stride, const float* out, int64_t out_stride,
                            const char* what) {
  if (d == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (x == nullptr || out == nullptr) return fail(SDR_EINVAL, "%s: x or out is NULL", what);
  int64_t nseg, rows, na;
  TRY(spec_geom(d, n, &nseg, &rows, &na, what));
  if (in_stride < n) return fail(SDR_EINVAL, "%s: in_stride=%lld < n=%lld", what, (long long)in_stride, (long long)n);
  if (out_stride < d->N / 2 + 1)
    return fail(SDR_EINVAL, "%s: out_stride=%lld < nfft/2+1=%d", what, (long long)out_stride, d->N / 2 + 1);
  if (((uintptr_t)x & 3) != 0 || ((uintptr_t)out & 3) != 0) return fail(SDR_EINVAL, "%s: x and out must be aligned to 4 B", what);
  return SDR_OK;
}

extern "C" {

int sdr_spec_create(sdr_ctx* c, int nfft, const double* window, int64_t hop, int64_t navg, int iq_dtype, sdr_spec** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_spec_create: out is NULL");
  *out = nullptr;
  std::vector<double> w;
  double wsum = 0.0;
  TRY(spec_check_create(nfft, window, hop, navg, w, &wsum, "sdr_spec_create"));
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8) return fail(SDR_EINVAL, "sdr_spec_create: bad iq_dtype %d", iq_dtype);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_spec* d = new (std::nothrow) sdr_spec;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_spec_create: out of host memory");
  d->dtype = iq_dtype;
  const hipError_t e = spec_init(d, c, w, wsum, hop, navg);
  if (e != hipSuccess) {
    sdr_spec_destroy(d);
    return create_failed(e, "sdr_spec_create");
  }
  *out = d;
  return SDR_OK;
}

void sdr_spec_destroy(sdr_spec* d) {
  if (d == nullptr) return;
  spec_free(d);
  delete d;
}

int sdr_spec_rows(sdr_spec* d, int64_t n, int64_t* nseg, int64_t* rows) {
  if (d == nullptr || nseg == nullptr || rows == nullptr) return fail(SDR_EINVAL, "sdr_spec_rows: NULL argument");
  int64_t na;
  return spec_geom(d, n, nseg, rows, &na, "sdr_spec_rows");
}

int sdr_spec_process_dev(sdr_spec* d, const void* iq, int64_t n, float* out, int64_t out_stride) {
  TRY(spec_check_call(d, iq, n, out, out_stride, "sdr_spec_process_dev"));
  const bool u8 = d->dtype == SDR_IQ_U8;
  if (((uintptr_t)iq & (u8 ? 1 : 7)) != 0 || ((uintptr_t)out & 3) != 0)
    return fail(SDR_EINVAL, "sdr_spec_process_dev: iq must be aligned to one complex sample (%d B) and out to 4 B", u8 ? 2 : 8);
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  int64_t nseg, rows, navg, cpr, chunk;
  TRY(spec_geom(d, n, &nseg, &rows, &navg, "sdr_spec_process_dev"));
  spec_chunks(rows * navg, navg, &cpr, &chunk);
  if (rows * cpr > 0x7fffffff)                     // (one workgroup each; such an output does not fit a device)
    return fail(SDR_EINVAL, "sdr_spec_process_dev: n=%lld yields %lld rows, above 2^31 - 1", (long long)n, (long long)rows);
  const double scale = 1.0 / ((double)navg * d->wsum * d->wsum);
  SpecArgs P;
  P.iq = iq;
  P.win = d->win;
  P.tw = d->tw;
  P.hop = d->hop;
  P.navg = navg;
  P.chunk = chunk;
  P.cpr = cpr;
  float* part = nullptr;
  if (cpr > 1) {
    TRY(scratch(c, S_SPEC, (size_t)(rows * cpr) * d->N * sizeof(float), (void**)&part));
    P.dst = part;
    P.dst_stride = d->N;
    P.scale = 1.f;
  } else {
    P.dst = out;
    P.dst_stride = out_stride;
    P.scale = (float)scale;
  }
  if (u8) spec_launch<true>(d->logn, (unsigned)(rows * cpr), P, c->stream);
  else spec_launch<false>(d->logn, (unsigned)(rows * cpr), P, c->stream);
  HIP_TRY(hipGetLastError());
  if (cpr > 1) {
    spec_reduce_kernel<<<dim3((unsigned)(d->N / SPEC_RED_BINS), (unsigned)rows), SPEC_RED_BINS * SPEC_RED_GROUPS, 0, c->stream>>>(
        part, out, d->N, d->N, cpr, out_stride, (float)scale);
    HIP_TRY(hipGetLastError());
  }
  return SDR_OK;
}

int sdr_spec_run(sdr_spec* d, const void* iq_host, int64_t n, float* out_host, int64_t out_stride) {
  TRY(spec_check_call(d, iq_host, n, out_host, out_stride, "sdr_spec_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  int64_t nseg, rows, navg;
  TRY(spec_geom(d, n, &nseg, &rows, &navg, "sdr_spec_run"));
  const size_t es = d->dtype == SDR_IQ_U8 ? 2 : 8, N = (size_t)d->N;
  return run_staged(c, iq_host, {1, (size_t)n * es, 0}, out_host, {(size_t)rows, N * 4, (size_t)out_stride * 4},
                    [&](void* din, void* dout) { return sdr_spec_process_dev(d, din, n, (float*)dout, d->N); });
}

int sdr_rspec_create(sdr_ctx* c, int nrows, int nfft, const double* window, int64_t hop, int64_t navg, sdr_rspec** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rspec_create: out is NULL");
  *out = nullptr;
  if (nrows < 1 || nrows > SDR_RSPEC_MAX_ROWS)
    return fail(SDR_EINVAL, "sdr_rspec_create: nrows=%d outside [1, %d]", nrows, SDR_RSPEC_MAX_ROWS);
  std::vector<double> w;
  double wsum = 0.0;
  TRY(spec_check_create(nfft, window, hop, navg, w, &wsum, "sdr_rspec_create"));
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rspec* d = new (std::nothrow) sdr_rspec;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_rspec_create: out of host memory");
  d->nrows = nrows;
  const hipError_t e = spec_init(d, c, w, wsum, hop, navg);
  if (e != hipSuccess) {
    sdr_rspec_destroy(d);
    return create_failed(e, "sdr_rspec_create");
  }
  *out = d;
  return SDR_OK;
}

void sdr_rspec_destroy(sdr_rspec* d) {
  if (d == nullptr) return;
  spec_free(d);
  delete d;
}

int sdr_rspec_rows(sdr_rspec* d, int64_t n, int64_t* nseg, int64_t* rows) {
  if (d == nullptr || nseg == nullptr || rows == nullptr) return fail(SDR_EINVAL, "sdr_rspec_rows: NULL argument");
  int64_t na;
  return spec_geom(d, n, nseg, rows, &na, "sdr_rspec_rows");
}

int sdr_rspec_process_dev(sdr_rspec* d, const float* x, int64_t n, int64_t in_stride, float* out, int64_t out_stride) {
  TRY(rspec_check_call(d, x, n, in_stride, out, out_stride, "sdr_rspec_process_dev"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  int64_t nseg, rows, navg, cpr, chunk;
  TRY(spec_geom(d, n, &nseg, &rows, &navg, "sdr_rspec_process_dev"));
  const int64_t orows = d->nrows * rows;           // output rows of the call
  spec_chunks(orows * navg, navg, &cpr, &chunk);
  if (orows * cpr > 0x7fffffff)                    // (one workgroup each)
    return fail(SDR_EINVAL, "sdr_rspec_process_dev: n=%lld yields %lld rows, above 2^31 - 1", (long long)n, (long long)orows);
  const int nbins = d->N / 2 + 1;
  const int pstride = d->N / 2 + SPEC_RED_BINS;    // floats between the chunks' partial sums: a multiple of 16
  const double scale = 1.0 / ((double)navg * d->wsum * d->wsum);
  RSpecArgs P;
  P.x = x;
  P.win = d->win;
  P.tw = d->tw;
  P.in_stride = in_stride;
  P.hop = d->hop;
  P.rows = rows;
  P.navg = navg;
  P.chunk = chunk;
  P.cpr = cpr;
  float* part = nullptr;
  if (cpr > 1) {
    TRY(scratch(c, S_SPEC, (size_t)(orows * cpr) * pstride * sizeof(float), (void**)&part));
    P.dst = part;
    P.dst_stride = pstride;
    P.scale = 1.f;
  } else {
    P.dst = out;
    P.dst_stride = out_stride;
    P.scale = (float)scale;
  }
  rspec_launch(d->logn, (unsigned)(orows * cpr), P, c->stream);
  HIP_TRY(hipGetLastError());
  if (cpr > 1) {
    spec_reduce_kernel<<<dim3((unsigned)(pstride / SPEC_RED_BINS), (unsigned)orows), SPEC_RED_BINS * SPEC_RED_GROUPS, 0, c->stream>>>(
        part, out, pstride, nbins, cpr, out_stride, (float)scale);
    HIP_TRY(hipGetLastError());
  }
  return SDR_OK;
}

int sdr_rspec_run(sdr_rspec* d, const float* x_host, int64_t n, int64_t in_stride, float* out_host, int64_t out_stride) {
  TRY(rspec_check_call(d, x_host, n, in_stride, out_host, out_stride, "sdr_rspec_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  int64_t nseg, rows, navg;
  TRY(spec_geom(d, n, &nseg, &rows, &navg, "sdr_rspec_run"));
  const size_t nb = (size_t)d->N / 2 + 1;
  return run_staged(c, x_host, {(size_t)d->nrows, (size_t)n * 4, (size_t)in_stride * 4}, out_host,
                    {(size_t)d->nrows * (size_t)rows, nb * 4, (size_t)out_stride * 4},
                    [&](void* din, void* dout) { return sdr_rspec_process_dev(d, (const float*)din, n, n, (float*)dout, (int64_t)nb); });
}

}  // extern "C"

