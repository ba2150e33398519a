// RDS symbol clock recovery on the device (include/sdr.h sdr_rds_clock_*): every stream's in-phase
// RRC row -> differential bits, byte per bit, with an int32 count per stream -- the rows
// sdr_rds_sync_process_dev takes.  The host model rdsclock.py RdsSymbolClock is the specification;
// this file restates it so that bits, counts and state are the same after every call, whatever the
// split of a stream into calls.
//
// A call's row of a stream is its carried samples (the 24 before the first unfinished segment and
// that segment's < 768 samples) followed by the new ones; every stream of a call has the same
// length, so the host knows the segment count G and the tail, and the streams differ only in what
// the device keeps: phi, pi, the symbol and bit counts.  Six launches per call, whatever nstreams
// and n are; no atomics, no workgroup waits for another:
//   energy  24 lanes per segment: E_g[p] in f64, j ascending, each row read once, coalesced.
//   track   a workgroup per stream.  A thread per segment sums the window (the carried vectors in
//           front of the call's first segment) and takes the first maximum; the phi recurrence is
//           a scan of maps {0..23} -> {0..23}: a thread composes the maps of its chunk of
//           segments, the chunk maps are scanned in LDS, and the thread walks its chunk from the
//           phi the scan gives it.  j0, the symbol counts and the parity of every segment's first
//           symbol follow from a prefix sum.
//   counts  a wave per segment, a lane per symbol pair: the sign changes by the parity of the
//           pair's first symbol, by ballot.
//   pair    a workgroup per stream: the windowed counts, the pi recurrence as a scan of 2-state
//           maps, the bits every segment gives and their prefix sum.
//   bits    a wave per segment, a lane per pair: the emitted pairs compare their two samples and
//           store a byte at the pair's bit index.
//   finish  diff = bit xor the bit before it; the counts; the carried samples, energy vectors and
//           sign-change counts into the other of two slots (a call reads one and fills the other).
// The segment geometry, the host's cursor, the row across the seam, the windows that reach into the
// carried vectors and counts, the chunks and their scan are rds_seg.h's, shared with rds_carrier.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "rds_seg.h"

using namespace sdrint;

namespace {

constexpr int CK_T = 256, CK_NW = CK_T / 64;
constexpr int CK_ESEG = CK_T / SPS;            // segments of an energy workgroup: 10 (240 lanes)
constexpr int CK_KEEP = SDR_RDS_CLOCK_MAX_WINDOW - 1;      // carried vectors in front of a call
constexpr int CK_CARRY = SPS + SEG;            // a carried row: 24 + < 768 samples (792 floats apart)

// a segment's word: phi, j0 + 1, the parity of its first symbol's index, pi, the first pair
// barred (its first symbol used, or none before it), the pi map (from pi 0, from pi 1)
constexpr int I_J0 = 8, I_PAR = 16, I_PI = 18, I_EXCL = 19, I_MAP = 20;

// a stream's carried state; all zero = reset
struct ClockState {
  int64_t symbols, bits;
  int64_t fwd, back, wraps, changes;
  int phi, pi;
};
// what a call's later launches need of the state before it
struct ClockCall {
  int phi_prev, nbits, first, pad;
};

struct ClockArgs {
  const float* x; SegCall c;    // c.tail: the carried samples behind the 24
  int window, hysteresis;
  int64_t gstride;              // segments per stream of the per-call arrays
  int64_t max_bits, bit_stride, diff_stride;
  const float* carry_in; float* carry_out;
  const double* ecar_in; double* ecar_out;      // [stream][CK_KEEP][24]
  const int* ccar_in; int* ccar_out;            // [stream][CK_KEEP][2]
  ClockState* state; ClockCall* call;
  double* E;                    // [stream][gstride][24]
  int* info; int* cc; int* bit0;                // [stream][gstride], [..][2], [..]
  uint8_t* bits;                // [stream][bit_stride]: the bit before the call, then the call's
  uint8_t* diff; int* counts;
};

// the call's row of stream s, from the 24 samples before its first segment on; its energy vectors
// and sign-change counts, the carried ones in front
using ClockRow = SegRow<SPS>;
using EnergyWindow = SegWindow<double, SPS, CK_KEEP>;
using CountWindow = SegWindow<int, 2, CK_KEEP>;
__device__ __forceinline__ ClockRow row_of(const ClockArgs& a, int s) {
  return ClockRow{a.x + (int64_t)s * a.c.stride, a.carry_in + (int64_t)s * CK_CARRY, a.c.tail};
}
__device__ __forceinline__ EnergyWindow energy_of(const ClockArgs& a, int s) {
  return EnergyWindow{a.E + (int64_t)s * a.gstride * SPS, a.ecar_in + (int64_t)s * CK_KEEP * SPS};
}
__device__ __forceinline__ CountWindow counts_of(const ClockArgs& a, int s) {
  return CountWindow{a.cc + (int64_t)s * a.gstride * 2, a.ccar_in + (int64_t)s * CK_KEEP * 2};
}

__device__ __forceinline__ int step_phi(int phi, int phat) {
  int d = phat - phi;                           // ((phat - phi + 12) mod 24) - 12, in -12 .. 11
  d = d > 11 ? d - 24 : d < -12 ? d + 24 : d;
  return d >= 2 ? (phi == 23 ? 0 : phi + 1) : d <= -2 ? (phi == 0 ? 23 : phi - 1) : phi;
}

__global__ __launch_bounds__(CK_T) void rds_clock_energy_kernel(const ClockArgs a) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const int g = blockIdx.x * CK_ESEG + tid / SPS, p = tid % SPS;
  if (tid >= CK_ESEG * SPS || g >= a.c.G) return;
  double e = 0.0;
  seg_samples(g, p, a.c.tail, [&e](float f) {
    const double d = __builtin_isfinite(f) ? (double)f : 0.0;
    e += d * d;
  }, row_of(a, s));
  a.E[((int64_t)s * a.gstride + g) * SPS + p] = e;
}

struct Sum4 {
  int x, y, z, w;
};

__global__ __launch_bounds__(CK_T) void rds_clock_track_kernel(const ClockArgs a) {
  __shared__ uint8_t maps[2][CK_T][SPS];
  __shared__ Sum4 sums[2][CK_T];
  const int s = blockIdx.x, tid = threadIdx.x, G = a.c.G;
  ClockState* st = a.state + s;
  const int phi_seed = st->phi;
  const int64_t sym_seed = st->symbols;
  int* __restrict__ info = a.info + (int64_t)s * a.gstride;
  const EnergyWindow energy = energy_of(a, s);

  // phat of every segment: the window's vectors, oldest first
  for (int g = tid; g < G; g += CK_T) {
    const int64_t gabs = a.c.seg0 + g;
    const int w = gabs + 1 < a.window ? (int)(gabs + 1) : a.window;
    double A[SPS];
#pragma unroll
    for (int p = 0; p < SPS; ++p) A[p] = 0.0;
    for (int k = w - 1; k >= 0; --k) {
      const int gl = g - k;                     // >= -CK_KEEP
      const double* __restrict__ e = energy.at(gl);
#pragma unroll
      for (int p = 0; p < SPS; ++p) A[p] += e[p];
    }
    double best = A[0];
    int phat = 0;
#pragma unroll
    for (int p = 1; p < SPS; ++p)
      if (A[p] > best) {
        best = A[p];
        phat = p;
      }
    info[g] = phat;
  }
  __syncthreads();

  // the map of this thread's chunk of segments
  const SegChunk ch = chunk_of(tid, G, CK_T);
  const int g_lo = ch.lo, g_hi = ch.hi, nact = ch.nact;
  {
    int m[SPS];
#pragma unroll
    for (int v = 0; v < SPS; ++v) m[v] = v;
    for (int g = g_lo; g < g_hi; ++g) {
      const int phat = info[g];
      const bool first = a.c.seg0 + g == 0;
#pragma unroll
      for (int v = 0; v < SPS; ++v) m[v] = first ? phat : step_phi(m[v], phat);
    }
#pragma unroll
    for (int v = 0; v < SPS; ++v) maps[0][tid][v] = (uint8_t)m[v];
  }
  int cur = 0;
  for (int off = 1; off < nact; off <<= 1) {    // inclusive scan: chunks 0 .. tid in order
    __syncthreads();
    // all the loads of a round, then its stores: a store between them would make every load wait
    const int from = tid >= off ? tid - off : tid;
    int before[SPS], next[SPS];
#pragma unroll
    for (int v = 0; v < SPS; ++v) before[v] = tid >= off ? maps[cur][from][v] : v;
#pragma unroll
    for (int v = 0; v < SPS; ++v) next[v] = maps[cur][tid][before[v]];
#pragma unroll
    for (int v = 0; v < SPS; ++v) maps[cur ^ 1][tid][v] = (uint8_t)next[v];
    cur ^= 1;
  }
  __syncthreads();
  const int phi_lo = tid == 0 ? phi_seed : maps[cur][tid - 1][phi_seed];

  // the chunk from its phi: j0 and the counters
  Sum4 c = {0, 0, 0, 0};
  int phi = phi_lo;
  for (int g = g_lo; g < g_hi; ++g) {
    const int phat = info[g];
    const bool first = a.c.seg0 + g == 0;
    const int nphi = first ? phat : step_phi(phi, phat);
    int j0 = 0;
    if (!first && nphi != phi) {
      const bool up = nphi == (phi == 23 ? 0 : phi + 1);
      c.y += up;
      c.z += !up;
      if (up && nphi == 0) j0 = 1;
      else if (!up && nphi == 23) j0 = -1;
      c.w += j0 != 0;
    }
    info[g] = nphi | ((j0 + 1) << I_J0);
    c.x += SEG_SYM - j0;
    phi = nphi;
  }
  sums[0][tid] = c;
  const int sc = block_scan(sums, tid, nact, [](const Sum4& p, const Sum4& q) { return Sum4{p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w}; });
  // the parity of every segment's first symbol
  int64_t msym = sym_seed + (tid == 0 ? 0 : sums[sc][tid - 1].x);
  for (int g = g_lo; g < g_hi; ++g) {
    const int w = info[g];
    info[g] = w | ((int)(msym & 1) << I_PAR);
    msym += SEG_SYM - (((w >> I_J0) & 3) - 1);
  }
  __syncthreads();
  if (tid == 0) {
    const Sum4 t = sums[sc][nact > 0 ? nact - 1 : 0];
    a.call[s].phi_prev = phi_seed;
    st->symbols = sym_seed + t.x;
    st->fwd += t.y;
    st->back += t.z;
    st->wraps += t.w;
    if (G > 0) st->phi = info[G - 1] & 0xff;
  }
}

// the pair whose second symbol is number k of segment g: its two samples
struct ClockPair {
  float prev, cur;
};
__device__ __forceinline__ ClockPair pair_of(const ClockRow& row, int g, int k, int w, int phi_before) {
  const int phi = w & 0xff, j0 = ((w >> I_J0) & 3) - 1;
  const int64_t v = (int64_t)g * SEG + SPS * (j0 + k) + phi;
  ClockPair r;
  r.cur = row(v);
  r.prev = k == 0 ? row((int64_t)g * SEG - SPS + phi_before) : row(v - SPS);
  return r;
}

__global__ __launch_bounds__(CK_T) void rds_clock_counts_kernel(const ClockArgs a) {
  const int s = blockIdx.y, lane = threadIdx.x & 63, g = blockIdx.x * CK_NW + (threadIdx.x >> 6);
  if (g >= a.c.G) return;                       // the whole wave
  const int* __restrict__ info = a.info + (int64_t)s * a.gstride;
  const int w = info[g];
  const int phi_before = g > 0 ? info[g - 1] & 0xff : a.call[s].phi_prev;
  const int cnt = SEG_SYM - (((w >> I_J0) & 3) - 1);
  const bool act = lane < cnt && !(lane == 0 && a.c.seg0 + g == 0);
  bool change = false;
  if (act) {
    const ClockPair pr = pair_of(row_of(a, s), g, lane, w, phi_before);
    change = (pr.prev > 0.0f) != (pr.cur > 0.0f);
  }
  // the pair's first symbol is number M_g + lane - 1
  const int par = (((w >> I_PAR) & 1) + lane + 1) & 1;
  const unsigned long long c0 = __ballot(change && par == 0), c1 = __ballot(change && par == 1);
  if (lane == 0) {
    int* cc = a.cc + ((int64_t)s * a.gstride + g) * 2;
    cc[0] = __popcll(c0);
    cc[1] = __popcll(c1);
  }
}

__device__ __forceinline__ int map2_apply(int m, int pi) { return (m >> pi) & 1; }
// first p, then q
__device__ __forceinline__ int map2_compose(int p, int q) { return map2_apply(q, map2_apply(p, 0)) | (map2_apply(q, map2_apply(p, 1)) << 1); }

struct Sum2 {
  int x, y;
};

__global__ __launch_bounds__(CK_T) void rds_clock_pair_kernel(const ClockArgs a) {
  __shared__ int maps[2][CK_T];
  __shared__ Sum2 sums[2][CK_T];
  const int s = blockIdx.x, tid = threadIdx.x, G = a.c.G;
  ClockState* st = a.state + s;
  const int pi_seed = st->pi;
  const int64_t bits_seed = st->bits;
  int* __restrict__ info = a.info + (int64_t)s * a.gstride;
  const CountWindow counts = counts_of(a, s);

  // every segment's map of pi from the windowed counts
  for (int g = tid; g < G; g += CK_T) {
    const int64_t gabs = a.c.seg0 + g;
    const int w = gabs + 1 < a.window ? (int)(gabs + 1) : a.window;
    int c0 = 0, c1 = 0;
    for (int k = w - 1; k >= 0; --k) {
      const int gl = g - k;
      const int* __restrict__ c = counts.at(gl);
      c0 += c[0];
      c1 += c[1];
    }
    int m;
    if (gabs == 0) m = c0 >= c1 ? 0 : 3;
    else m = (c1 - c0 > a.hysteresis ? 1 : 0) | (c0 - c1 > a.hysteresis ? 0 : 2);
    info[g] |= m << I_MAP;
  }
  __syncthreads();

  const SegChunk ch = chunk_of(tid, G, CK_T);
  const int g_lo = ch.lo, g_hi = ch.hi, nact = ch.nact;
  int cm = 2;                                   // the identity
  for (int g = g_lo; g < g_hi; ++g) cm = map2_compose(cm, (info[g] >> I_MAP) & 3);
  maps[0][tid] = cm;
  const int mc = block_scan(maps, tid, nact, [](int p, int q) { return map2_compose(p, q); });
  int pi = tid == 0 ? pi_seed : map2_apply(maps[mc][tid - 1], pi_seed);

  Sum2 c = {0, 0};
  for (int g = g_lo; g < g_hi; ++g) {
    const int w = info[g];
    const bool first = a.c.seg0 + g == 0;
    const int npi = map2_apply((w >> I_MAP) & 3, pi);
    const bool moved = !first && npi != pi;
    const bool excl = first || moved;
    const int cnt = SEG_SYM - (((w >> I_J0) & 3) - 1);
    const int r = (npi + ((w >> I_PAR) & 1) + 1) & 1;           // the emitted pairs: k = r, r + 2, ...
    c.x += (cnt - r + 1) / 2 - (r == 0 && excl ? 1 : 0);
    c.y += moved;
    info[g] = w | (npi << I_PI) | ((int)excl << I_EXCL);
    pi = npi;
  }
  sums[0][tid] = c;
  const int sc = block_scan(sums, tid, nact, [](const Sum2& p, const Sum2& q) { return Sum2{p.x + q.x, p.y + q.y}; });
  int nb = tid == 0 ? 0 : sums[sc][tid - 1].x;
  int* __restrict__ bit0 = a.bit0 + (int64_t)s * a.gstride;
  for (int g = g_lo; g < g_hi; ++g) {
    const int w = info[g];
    const int cnt = SEG_SYM - (((w >> I_J0) & 3) - 1);
    const int r = (((w >> I_PI) & 1) + ((w >> I_PAR) & 1) + 1) & 1;
    bit0[g] = nb;
    nb += (cnt - r + 1) / 2 - (r == 0 && ((w >> I_EXCL) & 1) ? 1 : 0);
  }
  __syncthreads();
  if (tid == 0) {
    const Sum2 t = sums[sc][nact > 0 ? nact - 1 : 0];
    a.call[s].nbits = t.x;
    a.call[s].first = bits_seed == 0;
    st->bits = bits_seed + t.x;
    st->changes += t.y;
    if (G > 0) st->pi = (info[G - 1] >> I_PI) & 1;
  }
}

__global__ __launch_bounds__(CK_T) void rds_clock_bits_kernel(const ClockArgs a) {
  const int s = blockIdx.y, lane = threadIdx.x & 63, g = blockIdx.x * CK_NW + (threadIdx.x >> 6);
  if (g >= a.c.G) return;
  const int* __restrict__ info = a.info + (int64_t)s * a.gstride;
  const int w = info[g];
  const int cnt = SEG_SYM - (((w >> I_J0) & 3) - 1);
  const int r = (((w >> I_PI) & 1) + ((w >> I_PAR) & 1) + 1) & 1;
  const int excl = r == 0 && ((w >> I_EXCL) & 1) ? 1 : 0;
  if (lane >= cnt || ((lane ^ r) & 1) != 0 || (lane == 0 && excl)) return;
  const int phi_before = g > 0 ? info[g - 1] & 0xff : a.call[s].phi_prev;
  const ClockPair pr = pair_of(row_of(a, s), g, lane, w, phi_before);
  const int64_t idx = (int64_t)a.bit0[(int64_t)s * a.gstride + g] + (lane - r) / 2 - excl;
  if (idx < a.max_bits) a.bits[(int64_t)s * a.bit_stride + 1 + idx] = pr.prev > pr.cur ? 1 : 0;
}

__global__ __launch_bounds__(CK_T) void rds_clock_finish_kernel(const ClockArgs a) {
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * CK_T + threadIdx.x;
  const ClockCall call = a.call[s];
  uint8_t* __restrict__ b = a.bits + (int64_t)s * a.bit_stride;
  // bits 1 .. nbits of b are the call's, b[0] the one before them unless these are the first
  const int64_t nd = call.nbits > 0 ? call.nbits - call.first : 0;
  if (i < nd) a.diff[(int64_t)s * a.diff_stride + i] = b[i + call.first] ^ b[i + call.first + 1];
  if (i == 0) {                                 // the only thread that reads b[0]
    a.counts[s] = (int)nd;
    if (call.nbits > 0) b[0] = b[call.nbits];
  }
  // the next call's carried samples: the 24 before its first segment, and the tail
  const int G = a.c.G;
  const int64_t L = a.c.tail + a.c.n - (int64_t)G * SEG;         // < 768
  if (i < SPS + L) a.carry_out[(int64_t)s * CK_CARRY + i] = row_of(a, s)((int64_t)G * SEG - SPS + i);
  // ... and the last CK_KEEP energy vectors and counts of (the carried ones, the call's)
  if (i < CK_KEEP * SPS) a.ecar_out[(int64_t)s * CK_KEEP * SPS + i] = energy_of(a, s).roll(G, (int)i);
  if (i < CK_KEEP * 2) a.ccar_out[(int64_t)s * CK_KEEP * 2 + i] = counts_of(a, s).roll(G, (int)i);
}

}  // namespace

struct sdr_rds_clock {
  sdr_ctx* ctx = nullptr;
  int S = 0, window = 4, hysteresis = 8;
  int64_t max_n = 0, gstride = 0, max_bits = 0, bit_stride = 0, diff_stride = 0;
  SegCursor seg;
  DevMem mem;
  float* carry[2] = {nullptr, nullptr};
  double* ecar[2] = {nullptr, nullptr};
  int* ccar[2] = {nullptr, nullptr};
  ClockState* state = nullptr;
  ClockCall* call = nullptr;
  double* E = nullptr;
  int* info = nullptr;
  int* cc = nullptr;
  int* bit0 = nullptr;
  uint8_t* bits = nullptr;
  uint8_t* diff = nullptr;
  int* counts = nullptr;
};

extern "C" {

int sdr_rds_clock_create(sdr_ctx* c, int nstreams, int64_t max_n, sdr_rds_clock** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_create: out is NULL");
  *out = nullptr;
  if (nstreams < 1 || nstreams > SDR_RDS_CLOCK_MAX_STREAMS)
    return fail(SDR_EINVAL, "sdr_rds_clock_create: nstreams=%d outside [1, %d]", nstreams, SDR_RDS_CLOCK_MAX_STREAMS);
  if (max_n < 1 || max_n > SDR_RDS_CLOCK_MAX_N)
    return fail(SDR_EINVAL, "sdr_rds_clock_create: max_n=%lld outside [1, %d]", (long long)max_n, SDR_RDS_CLOCK_MAX_N);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rds_clock* k = new (std::nothrow) sdr_rds_clock;
  if (k == nullptr) return fail(SDR_ENOMEM, "sdr_rds_clock_create: out of host memory");
  k->ctx = c;
  k->S = nstreams;
  k->max_n = max_n;
  k->gstride = (max_n + SEG - 1) / SEG;         // the segments of max_n samples behind a tail of < 768
  k->max_bits = 17 * k->gstride + 1;            // <= 33 symbols a segment and one carried
  k->bit_stride = ceil_div(k->max_bits + 2, 64) * 64;
  k->diff_stride = ceil_div(k->max_bits, 64) * 64;
  const size_t S = (size_t)nstreams, GS = S * (size_t)k->gstride;
  DevMem& m = k->mem;             // `true`: what a reset clears
  m.get2(k->carry, CK_CARRY * S, true);
  m.get2(k->ecar, CK_KEEP * SPS * S, true);
  m.get2(k->ccar, CK_KEEP * 2 * S, true);
  m.get(&k->state, S, true);
  m.get(&k->call, S, true);
  m.get(&k->E, SPS * GS);
  m.get(&k->info, GS);
  m.get(&k->cc, 2 * GS);
  m.get(&k->bit0, GS);
  m.get(&k->bits, S * (size_t)k->bit_stride, true);
  m.get(&k->diff, S * (size_t)k->diff_stride);
  m.get(&k->counts, S, true);
  if (m.err == hipSuccess) m.err = hipMemsetAsync(k->diff, 0, S * (size_t)k->diff_stride, c->stream);
  if (m.err == hipSuccess) m.err = m.zero(c->stream);
  if (m.err != hipSuccess) {
    const hipError_t e = m.err;
    sdr_rds_clock_destroy(k);
    return create_failed(e, "sdr_rds_clock_create");
  }
  *out = k;
  return SDR_OK;
}

void sdr_rds_clock_destroy(sdr_rds_clock* k) {
  if (k == nullptr) return;
  if (k->ctx != nullptr && set_dev(k->ctx) == SDR_OK) (void)hipStreamSynchronize(k->ctx->stream);
  k->mem.release();
  delete k;
}

int sdr_rds_clock_reset(sdr_rds_clock* k) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_reset: object is NULL");
  TRY(set_dev(k->ctx));
  HIP_TRY(k->mem.zero(k->ctx->stream));
  k->seg = SegCursor{};
  return SDR_OK;
}

int sdr_rds_clock_set_params(sdr_rds_clock* k, int window, int hysteresis) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_set_params: object is NULL");
  if (window < 1 || window > SDR_RDS_CLOCK_MAX_WINDOW)
    return fail(SDR_EINVAL, "sdr_rds_clock_set_params: window=%d outside [1, %d]", window, SDR_RDS_CLOCK_MAX_WINDOW);
  if (hysteresis < 0 || hysteresis > SDR_RDS_CLOCK_MAX_HYSTERESIS)
    return fail(SDR_EINVAL, "sdr_rds_clock_set_params: hysteresis=%d outside [0, %d]", hysteresis, SDR_RDS_CLOCK_MAX_HYSTERESIS);
  k->window = window;
  k->hysteresis = hysteresis;
  return SDR_OK;
}

int sdr_rds_clock_process_dev(sdr_rds_clock* k, const float* rrc_i, int64_t n, int64_t stride) {
  TRY(seg_check_call(k, {rrc_i}, n, stride, "sdr_rds_clock_process_dev"));
  sdr_ctx* c = k->ctx;
  TRY(set_dev(c));
  ClockArgs a;
  a.x = rrc_i;
  a.c = k->seg.begin(n, stride);
  const int64_t G = a.c.G;                      // <= gstride: tail <= 767
  a.window = k->window;
  a.hysteresis = k->hysteresis;
  a.gstride = k->gstride;
  a.max_bits = k->max_bits;
  a.bit_stride = k->bit_stride;
  a.diff_stride = k->diff_stride;
  a.carry_in = k->carry[k->seg.cur];
  a.carry_out = k->carry[k->seg.cur ^ 1];
  a.ecar_in = k->ecar[k->seg.cur];
  a.ecar_out = k->ecar[k->seg.cur ^ 1];
  a.ccar_in = k->ccar[k->seg.cur];
  a.ccar_out = k->ccar[k->seg.cur ^ 1];
  a.state = k->state;
  a.call = k->call;
  a.E = k->E;
  a.info = k->info;
  a.cc = k->cc;
  a.bit0 = k->bit0;
  a.bits = k->bits;
  a.diff = k->diff;
  a.counts = k->counts;
  const unsigned S = (unsigned)k->S;
  const unsigned gseg = (unsigned)std::max<int64_t>(1, ceil_div(G, CK_NW));
  const int64_t fin = std::max<int64_t>(17 * G + 1, CK_CARRY);    // the call's bits; the carried row; 15 x 24 vectors
  hipLaunchKernelGGL(rds_clock_energy_kernel, dim3((unsigned)std::max<int64_t>(1, ceil_div(G, CK_ESEG)), S), dim3(CK_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_clock_track_kernel, dim3(S), dim3(CK_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_clock_counts_kernel, dim3(gseg, S), dim3(CK_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_clock_pair_kernel, dim3(S), dim3(CK_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_clock_bits_kernel, dim3(gseg, S), dim3(CK_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_clock_finish_kernel, dim3((unsigned)ceil_div(fin, CK_T), S), dim3(CK_T), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  k->seg.commit(a.c);
  return SDR_OK;
}

int sdr_rds_clock_bits(sdr_rds_clock* k, uint8_t** dev, int64_t* stride, int32_t** counts_dev, int64_t* max_bits) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_bits: object is NULL");
  if (dev) *dev = k->diff;
  if (stride) *stride = k->diff_stride;
  if (counts_dev) *counts_dev = k->counts;
  if (max_bits) *max_bits = k->max_bits;
  return SDR_OK;
}

int sdr_rds_clock_fetch(sdr_rds_clock* k, uint8_t* bits, int32_t* counts) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_fetch: object is NULL");
  sdr_ctx* c = k->ctx;
  TRY(set_dev(c));
  if (bits)
    HIP_TRY(hipMemcpy2DAsync(bits, (size_t)k->max_bits, k->diff, (size_t)k->diff_stride, (size_t)k->max_bits, (size_t)k->S,
                             hipMemcpyDeviceToHost, c->stream));
  if (counts) HIP_TRY(hipMemcpyAsync(counts, k->counts, sizeof(int) * k->S, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_rds_clock_state(sdr_rds_clock* k, int64_t* state) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_state: object is NULL");
  if (state == nullptr) return fail(SDR_EINVAL, "sdr_rds_clock_state: state is NULL");
  std::vector<ClockState> st;
  TRY(fetch_states(k->ctx, k->state, k->S, &st));
  for (int s = 0; s < k->S; ++s) {
    int64_t* o = state + (size_t)SDR_RDS_CLOCK_NSTATE * s;
    o[0] = k->seg.seg0 * SEG;
    o[1] = k->seg.seg0;
    o[2] = st[s].phi;
    o[3] = st[s].pi;
    o[4] = st[s].symbols;
    o[5] = st[s].bits;
    o[6] = st[s].fwd;
    o[7] = st[s].back;
    o[8] = st[s].wraps;
    o[9] = st[s].changes;
  }
  return SDR_OK;
}

}  // extern "C"
