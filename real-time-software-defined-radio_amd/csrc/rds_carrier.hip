// RDS carrier phase recovery on the device (include/sdr.h sdr_rds_carrier_*): every stream's
// rrc_i and rrc_q rows -> one row per stream, the samples projected onto the axis the data lie on
// -- the rows sdr_rds_clock_process_dev and sdr_rds_links_process_dev take.  The host model
// rdscarrier.py RdsCarrierPhase is the specification; this file restates it so that rows, state and
// moments are the same after every call, whatever the split of a stream into calls.
//
// A call's rows of a stream are its carried samples (those of the unfinished segment, < 768 of
// each row; the stage needs none before them) followed by the new ones; every stream of a call has
// the same length, so the host knows the segment count G and the tail, and the streams differ only
// in what the device keeps: kappa, the counters and the last 16 moment triples.  The call's
// segments are its G complete ones and the one its last samples begin, whose axis depends on
// complete segments only and is found again, and counted, by the call that completes it.  Four
// launches per call, whatever nstreams and n are; no atomics, no workgroup waits for another:
//   moments 24 lanes per complete segment: the three sums over j in f64, each row read once,
//           coalesced; then a thread per segment and sum adds the 24 values, p ascending.
//   track   a workgroup of 1 024 per stream.  A thread per segment sums the window (the carried
//           triples in front of the call's first segment) and takes the sector; the kappa
//           recurrence is a scan of maps {0..63} -> {0..63}, which commute with half a turn and so
//           are 32 bytes each: 32 lanes walk a chunk of segments from the 32 values of kappa and
//           leave the chunk's map up to every segment, the 32 chunk maps are scanned in LDS, a byte
//           a thread and round, and a thread per segment looks its kappa up from the one in front
//           of its chunk, counting steps, holds and wraps.
//   rotate  every sample: y = float(f64(c) f64(i) + f64(s) f64(q)), both products exact, one
//           rounding fused or not.  Four samples a thread, a 16-byte store into the bank's own
//           rows, 16-byte loads from the rows whose address allows them and 4-byte loads from the
//           others; the last n mod 4 samples of a row one by one.
//   finish  the carried samples and the last 16 moment triples of (the carried ones, the call's)
//           into the other of two slots (a call reads one and fills the other).
// The segment geometry, the host's cursor, the rows across the seam, the window that reaches into
// the carried triples and the chunks are rds_seg.h's, shared with rds_clock.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "rds_seg.h"

using namespace sdrint;

namespace {

constexpr int CR_T = 256;
constexpr int CR_MSEG = CR_T / SPS;            // segments of a moments workgroup: 10 (240 lanes)
constexpr int CR_KEEP = SDR_RDS_CARRIER_MAX_WINDOW;        // carried moment triples in front of a call
constexpr int CR_NK = 64;                      // axis indices
constexpr int TR_T = 1024, TR_CH = TR_T / 32;  // the track workgroup: 32 chunks of segments, 32 lanes each

// tan(pi/32), tan(3 pi/32), tan(5 pi/32), tan(7 pi/32): the literals of rdscarrier.py THRESHOLDS
constexpr double CR_T0 = 0.098491403357164248, CR_T1 = 0.3033466836073424, CR_T2 = 0.53451113595079158,
                 CR_T3 = 0.82067879082866024;

// a segment's code: khat, or no direction (kappa holds), or segment 1's (kappa = khat); a hold that counts
constexpr int C_NONE = 32, C_SET = 64, C_COUNT = 128;

// a stream's carried state; all zero = reset
struct CarrierState {
  int64_t fwd, back, holds, wraps;
  double A, B, C;
  int kappa, pad;
};

struct CarrierArgs {
  const float* xi; const float* xq; SegCall c;
  int window;
  int64_t gstride, kstride;     // complete segments / segments per stream of the per-call arrays
  int64_t ystride;
  const float* carry_in; float* carry_out;      // [stream][2][SEG]
  const double* mcar_in; double* mcar_out;      // [stream][CR_KEEP][3]
  CarrierState* state;
  double* M;                    // [stream][gstride][3]
  int* info;                    // [stream][kstride]: the code, then kappa
  uint8_t* ptab;                // [stream][kstride][32]: a chunk's maps up to each of its segments
  const float2* axes;           // [64]
  float* y;                     // [stream][ystride]
};

// the call's row q (0: i, 1: q) of stream s; its moment triples, the carried ones in front
using CarrierRow = SegRow<0>;
using MomentWindow = SegWindow<double, 3, CR_KEEP>;
__device__ __forceinline__ CarrierRow row_of(const CarrierArgs& a, int s, int q) {
  return CarrierRow{(q ? a.xq : a.xi) + (int64_t)s * a.c.stride, a.carry_in + ((int64_t)s * 2 + q) * SEG, a.c.tail};
}
__device__ __forceinline__ MomentWindow moments_of(const CarrierArgs& a, int s) {
  return MomentWindow{a.M + (int64_t)s * a.gstride * 3, a.mcar_in + (int64_t)s * CR_KEEP * 3};
}

__global__ __launch_bounds__(CR_T) void rds_carrier_moments_kernel(const CarrierArgs a) {
  __shared__ double part[3][CR_MSEG * SPS];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int g = blockIdx.x * CR_MSEG + tid / SPS, p = tid % SPS;
  if (tid < CR_MSEG * SPS) {
    double eii = 0.0, eqq = 0.0, eiq = 0.0;
    if (g < a.c.G)
      seg_samples(g, p, a.c.tail, [&](float fi, float fq) {
        const bool ok = __builtin_isfinite(fi) && __builtin_isfinite(fq);
        const double di = ok ? (double)fi : 0.0, dq = ok ? (double)fq : 0.0;
        eii += di * di;
        eqq += dq * dq;
        eiq += di * dq;
      }, row_of(a, s, 0), row_of(a, s, 1));
    part[0][tid] = eii;
    part[1][tid] = eqq;
    part[2][tid] = eiq;
  }
  __syncthreads();
  if (tid < 3 * CR_MSEG) {
    const int gl = tid / 3, k = tid % 3, gs = blockIdx.x * CR_MSEG + gl;
    if (gs < a.c.G) {
      double t = 0.0;
      for (int q = 0; q < SPS; ++q) t += part[k][gl * SPS + q];
      a.M[((int64_t)s * a.gstride + gs) * 3 + k] = t;
    }
  }
}

// the sector 0 .. 31 of atan2(Q, P), or -1: no direction
__device__ __forceinline__ int sector_of(double P, double Q) {
  double hi = fabs(P), lo = fabs(Q);
  const bool swapped = lo > hi;
  if (swapped) {
    const double t = hi;
    hi = lo;
    lo = t;
  }
  if (!(hi > 0.0)) return -1;
  int m = (lo > hi * CR_T0 ? 1 : 0) + (lo > hi * CR_T1 ? 1 : 0) + (lo > hi * CR_T2 ? 1 : 0) + (lo > hi * CR_T3 ? 1 : 0);
  if (swapped) m = 8 - m;
  if (P < 0.0) m = 16 - m;
  if (Q < 0.0) m = (32 - m) & 31;
  return m;
}

// A segment's map of kappa commutes with half a turn, f(kappa + 32) = f(kappa) + 32 (mod 64): the
// step looks at kappa mod 32 only.  Segment 1's constant map does not, but the kappa in front of it
// is always 0, so khat + (kappa & 32) stands for it.  A map is therefore 32 bytes, f(0) .. f(31).
__device__ __forceinline__ int step_kappa(int kappa, int code) {
  if (code & C_NONE) return kappa;
  const int khat = code & 31;
  if (code & C_SET) return khat | (kappa & 32);
  const int d = ((khat - kappa + 16) & 31) - 16;                  // in -16 .. 15
  return d >= 2 ? (kappa + 1) & 63 : d <= -2 ? (kappa - 1) & 63 : kappa;
}
__device__ __forceinline__ int map_apply(const uint8_t* f, int kappa) { return f[kappa & 31] ^ (kappa & 32); }

__global__ __launch_bounds__(TR_T) void rds_carrier_track_kernel(const CarrierArgs a) {
  __shared__ uint8_t maps[2][TR_CH][32];
  __shared__ int red[2][TR_T / 64];
  const int s = blockIdx.x, tid = threadIdx.x, G = a.c.G, N = G + 1;
  CarrierState* st = a.state + s;
  const int seed = st->kappa;
  int* info = a.info + (int64_t)s * a.kstride;       // both are read where other threads have written
  uint8_t* tab = a.ptab + (int64_t)s * a.kstride * 32;
  const MomentWindow moments = moments_of(a, s);

  // the code of every segment: the window's triples, oldest first
  for (int g = tid; g < N; g += TR_T) {
    const int64_t gabs = a.c.seg0 + g;
    int code = C_NONE;                          // segment 0
    if (gabs >= 1) {
      const int w = gabs < a.window ? (int)gabs : a.window;
      double A = 0.0, B = 0.0, C = 0.0;
      // every one of the CR_KEEP triples in front of g exists (the carried ones are zero after a
      // reset), so the loads do not wait for w: eight triples in flight, the window's added
#pragma unroll 8
      for (int k = CR_KEEP; k >= 1; --k) {
        const int gl = g - k;                   // >= -CR_KEEP
        const double* __restrict__ m = moments.at(gl);
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        if (k <= w) {
          A += m0;
          B += m1;
          C += m2;
        }
      }
      const int khat = sector_of(A - B, 2.0 * C);
      code = khat < 0 ? (C_NONE | C_COUNT) : gabs == 1 ? (C_SET | khat) : khat;
      if (g == G - 1) {                         // the last complete segment's window
        st->A = A;
        st->B = B;
        st->C = C;
      }
    }
    info[g] = code;
  }
  __syncthreads();

  // 32 lanes walk a chunk of segments, lane v from kappa = v: tab[g][v] = where the chunk's segments
  // up to g take v, and the last of them is the chunk's map
  const int c = tid >> 5, v = tid & 31;
  const SegChunk ch = chunk_of(c, N, TR_CH);
  const int C = ch.C, g_lo = ch.lo, g_hi = ch.hi, nact = ch.nact;
  {
    int m = v;
    for (int g = g_lo; g < g_hi; g += 8) {      // eight codes in flight: a store may not pass a load
      int code[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) code[k] = g + k < g_hi ? info[g + k] : C_NONE;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        m = step_kappa(m, code[k]);
        if (g + k < g_hi) tab[(int64_t)(g + k) * 32 + v] = (uint8_t)m;
      }
    }
    maps[0][c][v] = (uint8_t)m;
  }
  int cur = 0;
  for (int off = 1; off < nact; off <<= 1) {    // inclusive scan: chunks 0 .. c in order
    __syncthreads();
    const int before = c >= off ? maps[cur][c - off][v] : v;
    maps[cur ^ 1][c][v] = (uint8_t)map_apply(maps[cur][c], before);
    cur ^= 1;
  }
  __syncthreads();

  // a thread per segment: kappa from the one in front of its chunk; the counters are those of the
  // complete segments
  int updown = 0, holdwrap = 0;                 // steps up | down << 16, holds | wraps << 16: each <= G < 2^16
  for (int g = tid; g < N; g += TR_T) {
    const int cg = g / C;
    const int k0 = cg == 0 ? seed : map_apply(maps[cur][cg - 1], seed);
    const int kappa = g == cg * C ? k0 : map_apply(tab + (int64_t)(g - 1) * 32, k0);
    const int nk = map_apply(tab + (int64_t)g * 32, k0);
    const int code = info[g];
    if (g < G) {
      if (!(code & (C_NONE | C_SET)) && nk != kappa) {
        const bool up = nk == ((kappa + 1) & 63);
        updown += up ? 1 : 1 << 16;
        holdwrap += ((up && nk == 0) || (!up && nk == 63)) ? 1 << 16 : 0;
      }
      holdwrap += (code & C_COUNT) ? 1 : 0;
      if (g == G - 1) st->kappa = nk;           // every thread has read the seed
    }
    info[g] = nk;
  }
  for (int off = 32; off > 0; off >>= 1) {
    updown += __shfl_xor(updown, off);
    holdwrap += __shfl_xor(holdwrap, off);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = updown;
    red[1][tid >> 6] = holdwrap;
  }
  __syncthreads();
  if (tid == 0) {
    int ud = 0, hw = 0;
    for (int w = 0; w < TR_T / 64; ++w) {
      ud += red[0][w];
      hw += red[1][w];
    }
    st->fwd += ud & 0xffff;
    st->back += ud >> 16;
    st->holds += hw & 0xffff;
    st->wraps += hw >> 16;
  }
}

__device__ __forceinline__ float project(float c, float sn, float fi, float fq) {
  return (float)((double)c * (double)fi + (double)sn * (double)fq);
}

typedef float vec4f __attribute__((ext_vector_type(4)));

// p[0 .. 3]: one 16-byte load where the address allows it
__device__ __forceinline__ vec4f load4(const float* __restrict__ p) {
  vec4f r;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    r = *reinterpret_cast<const vec4f*>(p);
  } else {
    r.x = p[0];
    r.y = p[1];
    r.z = p[2];
    r.w = p[3];
  }
  return r;
}

__global__ __launch_bounds__(CR_T) void rds_carrier_rotate_kernel(const CarrierArgs a) {
  const int s = blockIdx.y;
  const int64_t v = ((int64_t)blockIdx.x * CR_T + threadIdx.x) * 4;
  if (v >= a.c.n) return;
  const float* __restrict__ xi = a.xi + (int64_t)s * a.c.stride + v;
  const float* __restrict__ xq = a.xq + (int64_t)s * a.c.stride + v;
  float* __restrict__ y = a.y + (int64_t)s * a.ystride + v;
  const int* __restrict__ info = a.info + (int64_t)s * a.kstride;
  const int64_t r = a.c.tail + v;               // the sample's place in the call's row
  const int g0 = (int)(r / SEG);                // <= G
  const float2 ax0 = a.axes[info[g0] & 63];
  const float c0 = ax0.x, s0 = ax0.y;
  if (v + 4 <= a.c.n) {
    const int64_t edge = (int64_t)(g0 + 1) * SEG - r;             // the samples of this thread in g0
    float c1 = c0, s1 = s0;
    if (edge < 4) {
      const float2 ax1 = a.axes[info[g0 + 1] & 63];
      c1 = ax1.x;
      s1 = ax1.y;
    }
    const vec4f fi = load4(xi), fq = load4(xq);
    vec4f o;
    o.x = project(c0, s0, fi.x, fq.x);
    o.y = project(edge > 1 ? c0 : c1, edge > 1 ? s0 : s1, fi.y, fq.y);
    o.z = project(edge > 2 ? c0 : c1, edge > 2 ? s0 : s1, fi.z, fq.z);
    o.w = project(edge > 3 ? c0 : c1, edge > 3 ? s0 : s1, fi.w, fq.w);
    *reinterpret_cast<vec4f*>(y) = o;           // the bank's rows: 16-byte aligned, v a multiple of 4
  } else {
    const int left = (int)(a.c.n - v);          // 1 .. 3
    for (int k = 0; k < left; ++k) {
      float c1 = c0, s1 = s0;
      if ((r + k) / SEG != g0) {
        const float2 ax1 = a.axes[info[g0 + 1] & 63];
        c1 = ax1.x;
        s1 = ax1.y;
      }
      y[k] = project(c1, s1, xi[k], xq[k]);
    }
  }
}

__global__ __launch_bounds__(CR_T) void rds_carrier_finish_kernel(const CarrierArgs a) {
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * CR_T + threadIdx.x;
  // the next call's carried samples: those of the unfinished segment
  const int G = a.c.G;
  const int64_t L = a.c.tail + a.c.n - (int64_t)G * SEG;          // < 768
  if (i < L) {
    a.carry_out[((int64_t)s * 2 + 0) * SEG + i] = row_of(a, s, 0)((int64_t)G * SEG + i);
    a.carry_out[((int64_t)s * 2 + 1) * SEG + i] = row_of(a, s, 1)((int64_t)G * SEG + i);
  }
  // ... and the last CR_KEEP moment triples of (the carried ones, the call's)
  if (i < CR_KEEP * 3) a.mcar_out[(int64_t)s * CR_KEEP * 3 + i] = moments_of(a, s).roll(G, (int)i);
}

// the axis table: entries 0 .. 8 rounded from f64, the rest by symmetry; no negative zeros
void build_axes(float* out) {
  const double pi = 3.14159265358979323846;
  float first[9][2];
  for (int k = 0; k < 9; ++k) {
    first[k][0] = (float)std::cos(pi * k / 32);
    first[k][1] = (float)std::sin(pi * k / 32);
  }
  first[0][0] = 1.0f;
  first[0][1] = 0.0f;
  first[8][0] = first[8][1] = (float)std::sqrt(0.5);
  for (int k = 0; k < CR_NK; ++k) {
    const int r = k % 16, quarter = k / 16;
    float c = r <= 8 ? first[r][0] : first[16 - r][1], sn = r <= 8 ? first[r][1] : first[16 - r][0];
    for (int t = 0; t < quarter; ++t) {         // a quarter turn: (c, s) -> (-s, c)
      const float o = c;
      c = -sn;
      sn = o;
    }
    out[2 * k] = c + 0.0f;
    out[2 * k + 1] = sn + 0.0f;
  }
}

}  // namespace

struct sdr_rds_carrier {
  sdr_ctx* ctx = nullptr;
  int S = 0, window = 8;
  int64_t max_n = 0, gstride = 0, kstride = 0, ystride = 0;
  SegCursor seg;
  DevMem mem;
  float axes_host[2 * CR_NK] = {};
  float* carry[2] = {nullptr, nullptr};
  double* mcar[2] = {nullptr, nullptr};
  CarrierState* state = nullptr;
  double* M = nullptr;
  int* info = nullptr;
  uint8_t* ptab = nullptr;
  float2* axes = nullptr;
  float* y = nullptr;
};

extern "C" {

int sdr_rds_carrier_create(sdr_ctx* c, int nstreams, int64_t max_n, sdr_rds_carrier** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_create: out is NULL");
  *out = nullptr;
  if (nstreams < 1 || nstreams > SDR_RDS_CLOCK_MAX_STREAMS)
    return fail(SDR_EINVAL, "sdr_rds_carrier_create: nstreams=%d outside [1, %d]", nstreams, SDR_RDS_CLOCK_MAX_STREAMS);
  if (max_n < 1 || max_n > SDR_RDS_CLOCK_MAX_N)
    return fail(SDR_EINVAL, "sdr_rds_carrier_create: max_n=%lld outside [1, %d]", (long long)max_n, SDR_RDS_CLOCK_MAX_N);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rds_carrier* k = new (std::nothrow) sdr_rds_carrier;
  if (k == nullptr) return fail(SDR_ENOMEM, "sdr_rds_carrier_create: out of host memory");
  k->ctx = c;
  k->S = nstreams;
  k->max_n = max_n;
  k->gstride = (max_n + SEG - 1) / SEG;         // the segments of max_n samples behind a tail of < 768
  k->kstride = k->gstride + 1;                  // ... and the one the last samples begin
  k->ystride = ceil_div(max_n, 64) * 64;
  build_axes(k->axes_host);
  const size_t S = (size_t)nstreams;
  DevMem& m = k->mem;             // `true`: what a reset clears
  m.get2(k->carry, 2 * SEG * S, true);
  m.get2(k->mcar, CR_KEEP * 3 * S, true);
  m.get(&k->state, S, true);
  m.get(&k->M, 3 * S * (size_t)k->gstride);
  m.get(&k->info, S * (size_t)k->kstride);
  m.get(&k->ptab, 32 * S * (size_t)k->kstride);
  m.get(&k->y, S * (size_t)k->ystride);
  m.get(&k->axes, CR_NK);
  hipError_t e = m.err;
  if (e == hipSuccess) e = hipMemcpyAsync(k->axes, k->axes_host, sizeof(float) * 2 * CR_NK, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(k->info, 0, sizeof(int) * S * (size_t)k->kstride, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(k->y, 0, sizeof(float) * S * (size_t)k->ystride, c->stream);
  if (e == hipSuccess) e = m.zero(c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // axes_host has been read
  if (e != hipSuccess) {
    sdr_rds_carrier_destroy(k);
    return create_failed(e, "sdr_rds_carrier_create");
  }
  *out = k;
  return SDR_OK;
}

void sdr_rds_carrier_destroy(sdr_rds_carrier* k) {
  if (k == nullptr) return;
  if (k->ctx != nullptr && set_dev(k->ctx) == SDR_OK) (void)hipStreamSynchronize(k->ctx->stream);
  k->mem.release();
  delete k;
}

int sdr_rds_carrier_reset(sdr_rds_carrier* k) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_reset: object is NULL");
  TRY(set_dev(k->ctx));
  HIP_TRY(k->mem.zero(k->ctx->stream));
  k->seg = SegCursor{};
  return SDR_OK;
}

int sdr_rds_carrier_set_params(sdr_rds_carrier* k, int window) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_set_params: object is NULL");
  if (window < 1 || window > SDR_RDS_CARRIER_MAX_WINDOW)
    return fail(SDR_EINVAL, "sdr_rds_carrier_set_params: window=%d outside [1, %d]", window, SDR_RDS_CARRIER_MAX_WINDOW);
  k->window = window;
  return SDR_OK;
}

int sdr_rds_carrier_process_dev(sdr_rds_carrier* k, const float* rrc_i, const float* rrc_q, int64_t n, int64_t stride) {
  TRY(seg_check_call(k, {rrc_i, rrc_q}, n, stride, "sdr_rds_carrier_process_dev"));
  sdr_ctx* c = k->ctx;
  TRY(set_dev(c));
  CarrierArgs a;
  a.xi = rrc_i;
  a.xq = rrc_q;
  a.c = k->seg.begin(n, stride);
  const int64_t G = a.c.G;                      // <= gstride: tail <= 767
  a.window = k->window;
  a.gstride = k->gstride;
  a.kstride = k->kstride;
  a.ystride = k->ystride;
  a.carry_in = k->carry[k->seg.cur];
  a.carry_out = k->carry[k->seg.cur ^ 1];
  a.mcar_in = k->mcar[k->seg.cur];
  a.mcar_out = k->mcar[k->seg.cur ^ 1];
  a.state = k->state;
  a.M = k->M;
  a.info = k->info;
  a.ptab = k->ptab;
  a.axes = k->axes;
  a.y = k->y;
  const unsigned S = (unsigned)k->S;
  hipLaunchKernelGGL(rds_carrier_moments_kernel, dim3((unsigned)std::max<int64_t>(1, ceil_div(G, CR_MSEG)), S), dim3(CR_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_carrier_track_kernel, dim3(S), dim3(TR_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_carrier_rotate_kernel, dim3((unsigned)std::max<int64_t>(1, ceil_div(n, 4 * CR_T)), S), dim3(CR_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_carrier_finish_kernel, dim3((unsigned)ceil_div(SEG, CR_T), S), dim3(CR_T), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  k->seg.commit(a.c);
  return SDR_OK;
}

int sdr_rds_carrier_rows(sdr_rds_carrier* k, float** dev, int64_t* stride) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_rows: object is NULL");
  if (dev) *dev = k->y;
  if (stride) *stride = k->ystride;
  return SDR_OK;
}

int sdr_rds_carrier_fetch(sdr_rds_carrier* k, float* rows, int64_t n) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_fetch: object is NULL");
  if (n < 0 || n > k->max_n)
    return fail(SDR_EINVAL, "sdr_rds_carrier_fetch: n=%lld outside [0, max_n=%lld]", (long long)n, (long long)k->max_n);
  if (rows == nullptr && n > 0) return fail(SDR_EINVAL, "sdr_rds_carrier_fetch: rows is NULL");
  sdr_ctx* c = k->ctx;
  TRY(set_dev(c));
  if (n > 0)
    HIP_TRY(hipMemcpy2DAsync(rows, sizeof(float) * (size_t)n, k->y, sizeof(float) * (size_t)k->ystride, sizeof(float) * (size_t)n,
                             (size_t)k->S, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_rds_carrier_state(sdr_rds_carrier* k, int64_t* state) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_state: object is NULL");
  if (state == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_state: state is NULL");
  std::vector<CarrierState> st;
  TRY(fetch_states(k->ctx, k->state, k->S, &st));
  for (int s = 0; s < k->S; ++s) {
    int64_t* o = state + (size_t)SDR_RDS_CARRIER_NSTATE * s;
    o[0] = k->seg.seg0 * SEG + k->seg.tail;
    o[1] = k->seg.seg0;
    o[2] = st[s].kappa;
    o[3] = st[s].fwd;
    o[4] = st[s].back;
    o[5] = st[s].holds;
    o[6] = st[s].wraps;
  }
  return SDR_OK;
}

int sdr_rds_carrier_moments(sdr_rds_carrier* k, double* abc) {
  if (k == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_moments: object is NULL");
  if (abc == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_moments: abc is NULL");
  std::vector<CarrierState> st;
  TRY(fetch_states(k->ctx, k->state, k->S, &st));
  for (int s = 0; s < k->S; ++s) {
    abc[3 * s] = st[s].A;
    abc[3 * s + 1] = st[s].B;
    abc[3 * s + 2] = st[s].C;
  }
  return SDR_OK;
}

int sdr_rds_carrier_axes(float* out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rds_carrier_axes: out is NULL");
  build_axes(out);
  return SDR_OK;
}

}  // extern "C"
