// Capture ingest (include/sdr.h sdr_ingest_*): the stage in front of sdr_iqc.  The raw bytes of a
// capture block in device memory -- interleaved u8, s8, s16 or f32 IQ -- become the interleaved f32
// block every stage behind it reads, and, while the ADC's codes are still there, the block's level
// meter: samples on a rail, the peak, the sum of squares.  The reference has no such stage; the
// definition is rtsdr.ingest_model (capture.py).  Two launches, nothing returns to the host:
//
//   ingest_kernel<FMT, SWAP, METER>  workgroup b takes the samples [b chunk, (b + 1) chunk) by
//       sdr_chunk.h's range pass (eight 8-bit samples, four s16 samples or two f32 samples a 16-B
//       load).  Each input byte is read once.  The meter is taken on the lane's own vector; at the
//       end of a round of loads the integer formats pass their vectors through a 1-KiB LDS tile per
//       wave and load, so that lane l of store j holds the tile's sample pair 64 j + l: every wave
//       store covers 1 KiB of contiguous output (one 16-B store a lane, or two 8-B halves where
//       out's 16-B phase differs from the pairs').  The tile is the wave's own: no workgroup
//       barrier in the loop.  f32 is two samples a lane and needs no tile; it moves as bits, so
//       NaN payloads pass, and every lane loads before it stores, so it runs in place.
//       out = f32(code) 2^-(bits - 1): the conversion and the power-of-two product are exact.
//       METER: the lane partials become one record (clipped, nonfinite, peak, sumsq) per workgroup
//       by sdr_chunk.h's block record.  No atomics.
//   ingest_fold_kernel  one wave: sdr_chunk.h's fold of the records, then lane 0 stores the call's
//       meter and adds to the carried totals.
//
// With the meter off the stage is the first launch alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <type_traits>

#include "sdr_chunk.h"
#include "sdr_ctx.h"

using namespace sdrint;

namespace {

constexpr int ING_THREADS = 256;
constexpr int ING_WAVES = ING_THREADS / 64;
constexpr int ING_MAX_WG = 2048;                  // partial records per call
constexpr int ING_U = 4;                          // loads in flight per lane and round
constexpr int ING_NREC = 4;                       // clipped, nonfinite, peak, sumsq
constexpr int ING_FOLD_U = 8;                     // the fold's record loads in flight per lane
static_assert(SDR_INGEST_CHUNK % 8 == 0, "whole 16-B vectors of every type");
// The 8-bit lane partial of the sum of squares is 32 bits wide: a lane's samples of the largest
// chunk, each at most 2 x 128^2.
static_assert((uint64_t)lane_share(max_chunk(SDR_INGEST_CHUNK, ING_MAX_WG), 8, ING_THREADS) * 2 * 128 * 128 <= 0xffffffffull,
              "the 32-bit lane partial cannot overflow within a chunk");
// One s16 sample adds up to 2 x 32768^2 = 2^31: it fits 32 bits, two do not.  The s16 lane partial
// is 64 bits wide from the first sample on; a chunk of at most 2^31 samples stays below 2^62.
static_assert((uint64_t)2 * 32768 * 32768 <= 0xffffffffull, "one s16 sample's squares fit the 32-bit term");

constexpr bool is_f32(int fmt) { return fmt == SDR_IQ_F32; }
constexpr int es_of(int fmt) { return fmt == SDR_IQ_F32 ? 8 : fmt == SDR_IQ_S16 ? 4 : 2; }

// the lane's share of the meter, integer formats: exact
template <bool WIDE>
struct MeterInt {
  uint32_t clipped = 0, nonfinite = 0, peak = 0;
  std::conditional_t<WIDE, uint64_t, uint32_t> sq = 0;
  int hi, lo;                                     // the rails: 2^(bits - 1) - 1 and -2^(bits - 1)
  __device__ __forceinline__ void add(int ci, int cq) {
    const int mx = ci > cq ? ci : cq, mn = ci < cq ? ci : cq;
    clipped += (mx >= hi || mn <= lo) ? 1u : 0u;
    const uint32_t a = (uint32_t)(mx > -mn ? mx : -mn);            // max(|ci|, |cq|); -lo counts with its magnitude
    peak = a > peak ? a : peak;
    sq += (uint32_t)(ci * ci) + (uint32_t)(cq * cq);
  }
  __device__ __forceinline__ unsigned long long sumsq() const { return sq; }
};

// f32: a sample with a non-finite I or Q counts there and nowhere else; |x| of a finite float
// orders as its bits do, so the peak is an integer maximum; the squares are exact in f64
struct MeterF32 {
  uint32_t clipped = 0, nonfinite = 0, peak = 0;
  double S = 0.0;
  __device__ __forceinline__ void add(uint32_t bi, uint32_t bq) {
    const uint32_t ai = bi & 0x7fffffffu, aq = bq & 0x7fffffffu, a = ai > aq ? ai : aq;
    const bool fin = a < 0x7f800000u;
    nonfinite += fin ? 0u : 1u;
    clipped += (fin && a >= 0x3f800000u) ? 1u : 0u;
    peak = (fin && a > peak) ? a : peak;
    const double di = fin ? (double)__builtin_bit_cast(float, bi) : 0.0, dq = fin ? (double)__builtin_bit_cast(float, bq) : 0.0;
    S = __builtin_fma(dq, dq, __builtin_fma(di, di, S));
  }
  __device__ __forceinline__ double sumsq() const { return S; }
};

// the meter's record: the sum of squares -- u64, exact, or f64 --, the counts (a call has fewer than
// 2^31 samples) and the peak (an integer maximum); value k of workgroup b is the 8-byte word
// part[k ING_MAX_WG + b], so the fold's lane-strided loads are contiguous
template <class ST>
struct IngRec {
  ST sumsq;
  uint32_t clipped, nonfinite, peak, pad;
  __device__ __forceinline__ void combine(const IngRec& o) {
    clipped += o.clipped;
    nonfinite += o.nonfinite;
    peak = o.peak > peak ? o.peak : peak;
    sumsq += o.sumsq;
  }
};

template <int FMT>
using Meter = std::conditional_t<is_f32(FMT), MeterF32, MeterInt<FMT == SDR_IQ_S16>>;

// the codes of the 8-bit dword I0 Q0 I1 Q1 (u8: x - 128 is the byte with its top bit flipped)
template <int FMT>
__device__ __forceinline__ void codes8(uint32_t d, int (&c)[4]) {
  if constexpr (FMT == SDR_IQ_U8) d ^= 0x80808080u;
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = (int)(d << (24 - 8 * k)) >> 24;
}
__device__ __forceinline__ void codes16(uint32_t d, int& ci, int& cq) {
  ci = (int)(d << 16) >> 16;
  cq = (int)d >> 16;
}

// the meter of a lane's 16-B vector
template <int FMT>
__device__ __forceinline__ void meter_vec(Meter<FMT>& m, const u4 x) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (FMT == SDR_IQ_F32) {
      if (e & 1) m.add(x[e - 1], x[e]);
    } else if constexpr (FMT == SDR_IQ_S16) {
      int ci, cq;
      codes16(x[e], ci, cq);
      m.add(ci, cq);
    } else {
      int c[4];
      codes8<FMT>(x[e], c);
      m.add(c[0], c[1]);
      m.add(c[2], c[3]);
    }
  }
}

template <bool SWAP>
__device__ __forceinline__ f2 out_pair(int ci, int cq, float scale) {
  const float fi = (float)ci * scale, fq = (float)cq * scale;
  return SWAP ? f2{fq, fi} : f2{fi, fq};
}

// One sample taken alone: loaded, metered, stored at out[2 s].  raw and out are aligned to one
// sample, so the accesses are whole.
template <int FMT, bool SWAP, bool METER>
__device__ __forceinline__ void ingest_one(const char* q, float* o, float scale, Meter<FMT>& m) {
  if constexpr (FMT == SDR_IQ_F32) {
    const uint2 b = *reinterpret_cast<const uint2*>(q);
    if constexpr (METER) m.add(b.x, b.y);
    *reinterpret_cast<uint2*>(o) = SWAP ? uint2{b.y, b.x} : b;
  } else {
    int ci, cq;
    if constexpr (FMT == SDR_IQ_S16) {
      codes16(*reinterpret_cast<const uint32_t*>(q), ci, cq);
    } else {
      int c[4];
      codes8<FMT>((uint32_t)*reinterpret_cast<const uint16_t*>(q), c);
      ci = c[0];
      cq = c[1];
    }
    if constexpr (METER) m.add(ci, cq);
    *reinterpret_cast<f2*>(o) = out_pair<SWAP>(ci, cq, scale);
  }
}

// raw and out may be the same f32 block: neither is __restrict__
template <int FMT, bool SWAP, bool METER>
__global__ __launch_bounds__(ING_THREADS) void ingest_kernel(const void* raw, int64_t n, int64_t chunk, float scale, int hi, int lo,
                                                             float* out, unsigned long long* __restrict__ part) {
  constexpr int ES = es_of(FMT);
  constexpr int NST = 16 / ES / 2;                                  // sample pairs = 16-B stores of a 16-B load
  const Chunk<ES> c(raw, n, chunk);
  float* oc = out + 2 * (int64_t)blockIdx.x * chunk;                // the chunk's output
  float* ov = oc + 2 * c.head;                                      // and that of its vectors
  const bool out16 = ((uintptr_t)ov & 15) == 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Meter<FMT> m;
  if constexpr (!is_f32(FMT)) {
    m.hi = hi;
    m.lo = lo;
  }
  scan_range<ES, ING_THREADS, ING_U>(
      c.p, c, threadIdx.x,
      [&](const u4 x, int64_t i) {
        if constexpr (METER) meter_vec<FMT>(m, x);
        if constexpr (is_f32(FMT)) {
          const u4 y = SWAP ? u4{x.y, x.x, x.w, x.z} : x;
          store_pair(ov + 4 * i, out16, __builtin_bit_cast(f4, y));
        }
      },
      [&](const u4(&x)[ING_U], int64_t i0) {
        if constexpr (!is_f32(FMT)) {
          // the wave's own tiles: lane l's vector at 16 l, pair p of the tile read back at 16 p / NST
          using PT = std::conditional_t<NST == 4, uint32_t, uint2>;
          __shared__ u4 tile[ING_WAVES][ING_U][64];
#pragma unroll
          for (int u = 0; u < ING_U; ++u) tile[w][u][lane] = x[u];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int u = 0; u < ING_U; ++u) {
            const int64_t vb = i0 + ING_THREADS * u + 64 * w;             // the wave's first vector of this load
            const PT* t = reinterpret_cast<const PT*>(&tile[w][u][0]);
#pragma unroll
            for (int j = 0; j < NST; ++j) {
              const int p = 64 * j + lane;
              if (vb + p / NST < c.nv) {
                f2 a, b;
                if constexpr (NST == 4) {
                  int k[4];
                  codes8<FMT>(t[p], k);
                  a = out_pair<SWAP>(k[0], k[1], scale);
                  b = out_pair<SWAP>(k[2], k[3], scale);
                } else {
                  const uint2 d = t[p];
                  int ci, cq;
                  codes16(d.x, ci, cq);
                  a = out_pair<SWAP>(ci, cq, scale);
                  codes16(d.y, ci, cq);
                  b = out_pair<SWAP>(ci, cq, scale);
                }
                store_pair(ov + 4 * (vb * NST + p), out16, f4{a.x, a.y, b.x, b.y});
              }
            }
          }
          // the next round's tile writes come after this round's reads
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      },
      // the single samples: no vector holds them, so no other thread reads or writes them
      [&](const char* q) { ingest_one<FMT, SWAP, METER>(q, oc + 2 * ((q - c.p) / ES), scale, m); });
  if constexpr (METER) {
    using ST = decltype(m.sumsq());
    block_record<ING_WAVES>(IngRec<ST>{m.sumsq(), m.clipped, m.nonfinite, m.peak, 0}, [&](const IngRec<ST>& r) {
      part[0 * ING_MAX_WG + blockIdx.x] = r.clipped;
      part[1 * ING_MAX_WG + blockIdx.x] = r.nonfinite;
      part[2 * ING_MAX_WG + blockIdx.x] = r.peak;
      part[3 * ING_MAX_WG + blockIdx.x] = __builtin_bit_cast(unsigned long long, r.sumsq);
    });
  }
}

struct IngFold {
  const unsigned long long* part;   // [ING_NREC][ING_MAX_WG], nwg records in use
  sdr_ingest_meter* m;
  int64_t n;
  int nwg, f32, bits;
};

template <class ST>
__device__ __forceinline__ IngRec<ST> fold_meter(const unsigned long long* __restrict__ p, int nwg, int lane) {
  return fold_records<ING_FOLD_U>(nwg, lane, IngRec<ST>{ST(0), 0, 0, 0, 0}, [&](int b) {
    return IngRec<ST>{__builtin_bit_cast(ST, p[3 * ING_MAX_WG + b]), (uint32_t)p[0 * ING_MAX_WG + b], (uint32_t)p[1 * ING_MAX_WG + b],
                      (uint32_t)p[2 * ING_MAX_WG + b], 0};
  });
}

__global__ __launch_bounds__(64) void ingest_fold_kernel(const IngFold a) {
  const int lane = threadIdx.x;
  uint32_t clipped, nonfinite, peak;
  unsigned long long S = 0;
  double D = 0.0;
  if (a.f32) {
    const IngRec<double> r = fold_meter<double>(a.part, a.nwg, lane);
    clipped = r.clipped; nonfinite = r.nonfinite; peak = r.peak; D = r.sumsq;
  } else {
    const IngRec<unsigned long long> r = fold_meter<unsigned long long>(a.part, a.nwg, lane);
    clipped = r.clipped; nonfinite = r.nonfinite; peak = r.peak; S = r.sumsq;
  }
  if (lane != 0) return;
  sdr_ingest_meter* __restrict__ m = a.m;
  m->n = a.n;
  m->clipped = (int64_t)clipped;
  m->nonfinite = (int64_t)nonfinite;
  if (a.f32) {
    m->peak_code = 0;
    m->sumsq_code = 0;
    m->peak = (double)__builtin_bit_cast(float, peak);
    m->sumsq = D;
  } else {
    m->peak_code = (int64_t)peak;
    m->sumsq_code = S;
    m->peak = __builtin_ldexp((double)peak, -(a.bits - 1));
    m->sumsq = __builtin_ldexp((double)S, -2 * (a.bits - 1));
  }
  m->calls += 1;
  m->total_n += a.n;
  m->total_clipped += (int64_t)clipped;
}

constexpr int container_bits(int dtype) { return dtype == SDR_IQ_F32 ? 32 : dtype == SDR_IQ_S16 ? 16 : 8; }

}  // namespace

struct sdr_ingest {
  sdr_ctx* ctx = nullptr;
  int dtype = 0, bits = 0, swap = 0, meter = 1;
  DevMem mem;
  sdr_ingest_meter* st = nullptr;      // the meter: all-zero bits (0 and 0.0) after a reset
  unsigned long long* part = nullptr;  // [ING_NREC][ING_MAX_WG] partial records
};

extern "C" {

int sdr_ingest_create(sdr_ctx* c, int iq_dtype, const sdr_ingest_params* params, sdr_ingest** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_ingest_create: out is NULL");
  *out = nullptr;
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8 && iq_dtype != SDR_IQ_S8 && iq_dtype != SDR_IQ_S16)
    return fail(SDR_EINVAL, "sdr_ingest_create: bad iq_dtype %d", iq_dtype);
  const int width = container_bits(iq_dtype);
  const int bits = params != nullptr && params->bits != 0 ? params->bits : width;
  if (iq_dtype == SDR_IQ_S16 ? (bits < 2 || bits > 16) : bits != width)
    return fail(SDR_EINVAL, "sdr_ingest_create: bits=%d outside %s for iq_dtype %d", bits, iq_dtype == SDR_IQ_S16 ? "[2, 16]" : "the container's width",
                iq_dtype);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_ingest* d = new (std::nothrow) sdr_ingest;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_ingest_create: out of host memory");
  d->ctx = c;
  d->dtype = iq_dtype;
  d->bits = bits;
  d->swap = params != nullptr ? (params->swap != 0) : 0;
  d->meter = params != nullptr ? (params->meter != 0) : 1;
  d->mem.get(&d->st, 1, true);
  d->mem.get(&d->part, (size_t)ING_MAX_WG * ING_NREC);
  const int rc = d->mem.err != hipSuccess ? create_failed(d->mem.err, "sdr_ingest_create") : sdr_ingest_reset(d);
  if (rc != SDR_OK) {
    sdr_ingest_destroy(d);
    return rc;
  }
  *out = d;
  return SDR_OK;
}

void sdr_ingest_destroy(sdr_ingest* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  d->mem.release();
  delete d;
}

int sdr_ingest_reset(sdr_ingest* d) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_ingest_reset: object is NULL");
  TRY(set_dev(d->ctx));
  HIP_TRY(d->mem.zero(d->ctx->stream));
  return SDR_OK;
}

int sdr_ingest_process_dev(sdr_ingest* d, const void* raw, int64_t n, float* out) {
  const bool f32 = d != nullptr && d->dtype == SDR_IQ_F32;
  TRY(capture_check_call("sdr_ingest_process_dev", d, "raw", raw, d != nullptr ? es_of(d->dtype) : 0, n, out, f32));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  int64_t chunk;
  const int nwg = chunks_of(n, SDR_INGEST_CHUNK, ING_MAX_WG, &chunk);
  // the integer formats' scale 2^-(bits - 1) and rails; f32 uses none of them
  const float scale = f32 ? 1.0f : std::ldexp(1.0f, -(d->bits - 1));
  const int hi = f32 ? 0 : (1 << (d->bits - 1)) - 1, lo = -hi - 1;
#define ING_LAUNCH(FMT, SW, ME) \
  hipLaunchKernelGGL((ingest_kernel<FMT, SW, ME>), dim3(nwg), dim3(ING_THREADS), 0, c->stream, raw, n, chunk, scale, hi, lo, out, d->part)
#define ING_FMT(FMT)                      \
  do {                                    \
    if (d->swap) {                        \
      if (d->meter) ING_LAUNCH(FMT, true, true);   \
      else ING_LAUNCH(FMT, true, false);  \
    } else {                              \
      if (d->meter) ING_LAUNCH(FMT, false, true);  \
      else ING_LAUNCH(FMT, false, false); \
    }                                     \
  } while (0)
  switch (d->dtype) {
    case SDR_IQ_F32: ING_FMT(SDR_IQ_F32); break;
    case SDR_IQ_U8: ING_FMT(SDR_IQ_U8); break;
    case SDR_IQ_S8: ING_FMT(SDR_IQ_S8); break;
    default: ING_FMT(SDR_IQ_S16); break;
  }
#undef ING_FMT
#undef ING_LAUNCH
  HIP_TRY(hipGetLastError());
  if (d->meter) {
    const IngFold fold{d->part, d->st, n, nwg, f32 ? 1 : 0, d->bits};
    hipLaunchKernelGGL(ingest_fold_kernel, dim3(1), dim3(64), 0, c->stream, fold);
    HIP_TRY(hipGetLastError());
  }
  return SDR_OK;
}

int sdr_ingest_run(sdr_ingest* d, const void* raw_host, int64_t n, float* out_host) {
  TRY(capture_check_call("sdr_ingest_run", d, "raw", raw_host, 0, n, out_host, false));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const size_t es = (size_t)es_of(d->dtype);
  return run_staged(c, raw_host, {1, (size_t)n * es, 0}, out_host, {1, (size_t)n * 8, (size_t)n * 8},
                    [&](void* din, void* dout) { return sdr_ingest_process_dev(d, din, n, (float*)dout); });
}

int sdr_ingest_meter_get(sdr_ingest* d, sdr_ingest_meter* host) {
  if (d == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_ingest_meter_get: NULL argument");
  return fetch(d->ctx, d->st, 1, host);
}

int sdr_ingest_meter_dev(sdr_ingest* d, const sdr_ingest_meter** dev) {
  if (d == nullptr || dev == nullptr) return fail(SDR_EINVAL, "sdr_ingest_meter_dev: NULL argument");
  *dev = d->st;
  return SDR_OK;
}

}  // extern "C"
