// IQ imbalance and DC offset correction of a capture block (include/sdr.h sdr_iqc_*): the stage in
// front of sdr_spec / sdr_ddc / sdr_pfb.  The reference has no such stage; the definition is
// rtsdr.IqBalance (iqbalance.py).  A block of n complex samples (interleaved f32, or u8 as
// (x - 128) / 128) goes through three launches, nothing returns to the host:
//
//   iqc_moments_kernel<U8>  the block's five raw sums (I, Q, I^2, Q^2, I Q).  Workgroup b takes the
//       samples [b chunk, (b + 1) chunk) by sdr_chunk.h's range pass (two f32 samples or eight u8
//       samples a 16-B load).  f32: five f64 accumulators a lane (a product of two f32 values is
//       exact in f64).  u8: integer sums of the raw bytes, four samples' I and four samples' Q
//       gathered into a dword each (v_perm_b32) and summed by v_dot4_u32_u8, exact; the lane
//       partials are 32 bits wide, which a lane's share of the largest chunk fits.  The lane sums
//       become one record per workgroup by sdr_chunk.h's block record.
//   iqc_update_kernel       one wave: sdr_chunk.h's fold of the records, then lane 0 runs the
//       rule's steps 2 and 3 in f64 (u8: the integer sums first become the moments of
//       (x - 128) / 128, exactly) and stores the state and the four coefficients.
//   iqc_apply_kernel<U8>    I' = f32(I - dI), Q' = f32(c1 (I - dI) + c2 (Q - dQ)) in f64, the
//       coefficients read from the state.  A lane takes two samples: one 16-B (f32) or 4-B (u8)
//       load and one 16-B store, so every wave instruction covers contiguous bytes.  (Eight u8
//       samples a lane would leave each lane 64 B of output at a 64-B lane stride; the stores are 8
//       of this pass's 10 bytes a sample and get the contiguous form.)  The first sample is taken
//       alone where iq does not start on a load boundary, the last where one is left over; where
//       out's 16-B phase then differs from the pairs', a pair is stored as two 8-B halves.  Every
//       lane loads its samples before it stores them, so f32 runs in place.
//
// Floating-point contraction is off in this file: the rule's expressions are evaluated as written
// (m + rate (r - m); c1 x + c2 y as two products and a sum), as numpy evaluates them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>

#include "sdr_chunk.h"
#include "sdr_ctx.h"

#pragma clang fp contract(off)

using namespace sdrint;

namespace {

constexpr int IQC_THREADS = 256;
constexpr int IQC_WAVES = IQC_THREADS / 64;
constexpr int IQC_MAX_WG = 2048;                  // partial records per call
constexpr int IQC_U = 4;                          // loads in flight per lane and round
constexpr int IQC_UPD_U = 8;                      // the update's record loads in flight per lane
static_assert(SDR_IQC_CHUNK % 8 == 0, "whole 16-B vectors of either type");
static_assert(SDR_IQC_NSTATE == 12, "mI mQ pII pQQ pIQ dI dQ c1 c2 updates skipped holds");
// the u8 lane partials are 32 bits wide: a lane's samples of the largest chunk, each at most 255^2
static_assert((uint64_t)lane_share(max_chunk(SDR_IQC_CHUNK, IQC_MAX_WG), 8, IQC_THREADS) * 255 * 255 <= 0xffffffffull,
              "the 32-bit lane partials cannot overflow within a chunk");

__device__ __forceinline__ float u8f(uint32_t b) { return ((float)b - 128.f) * (1.f / 128.f); }

// the five raw sums I, Q, I^2, Q^2, I Q: f64 (f32 samples) or u64 (u8 samples, exact)
template <class T>
struct Sum5 {
  T a[5];
  __device__ __forceinline__ void combine(const Sum5& o) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] += o.a[k];
  }
};

// value k of workgroup b is part[k IQC_MAX_WG + b], so the update's lane-strided loads are contiguous
template <bool U8>
__global__ __launch_bounds__(IQC_THREADS) void iqc_moments_kernel(const void* __restrict__ iq, int64_t n, int64_t chunk,
                                                                  void* __restrict__ part) {
  using T = std::conditional_t<U8, unsigned long long, double>;
  const Chunk<U8 ? 2 : 8> c(iq, n, chunk);
  Sum5<T> r;
  if constexpr (U8) {
    uint32_t s[5] = {0, 0, 0, 0, 0};
    scan_range<2, IQC_THREADS, IQC_U>(
        c.p, c, threadIdx.x,
        [&](const u4 x, int64_t) {
#pragma unroll
          for (int e = 0; e < 4; e += 2) {                  // two dwords I0 Q0 I1 Q1, I2 Q2 I3 Q3 -> I0 I1 I2 I3, Q0 Q1 Q2 Q3
            const uint32_t wi = __builtin_amdgcn_perm(x[e + 1], x[e], 0x06040200u);
            const uint32_t wq = __builtin_amdgcn_perm(x[e + 1], x[e], 0x07050301u);
            s[0] = __builtin_amdgcn_udot4(wi, 0x01010101u, s[0], false);
            s[1] = __builtin_amdgcn_udot4(wq, 0x01010101u, s[1], false);
            s[2] = __builtin_amdgcn_udot4(wi, wi, s[2], false);
            s[3] = __builtin_amdgcn_udot4(wq, wq, s[3], false);
            s[4] = __builtin_amdgcn_udot4(wi, wq, s[4], false);
          }
        },
        [&](const char* q) {
          const uint32_t h = *reinterpret_cast<const uint16_t*>(q), bi = h & 255u, bq = h >> 8;
          s[0] += bi; s[1] += bq; s[2] += bi * bi; s[3] += bq * bq; s[4] += bi * bq;
        });
#pragma unroll
    for (int k = 0; k < 5; ++k) r.a[k] = s[k];
  } else {
    double(&a)[5] = r.a;
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] = 0.0;
    auto add = [&](float fi, float fq) {
      const double di = (double)fi, dq = (double)fq;
      a[0] += di; a[1] += dq;
      // (the products are exact in f64: the fused form rounds as a product and a sum do)
      a[2] = __builtin_fma(di, di, a[2]); a[3] = __builtin_fma(dq, dq, a[3]); a[4] = __builtin_fma(di, dq, a[4]);
    };
    scan_range<8, IQC_THREADS, IQC_U>(
        c.p, c, threadIdx.x,
        [&](const u4 x, int64_t) {
          const f4 f = __builtin_bit_cast(f4, x);
          add(f.x, f.y);
          add(f.z, f.w);
        },
        [&](const char* q) {
          const f2 f = *reinterpret_cast<const f2*>(q);
          add(f.x, f.y);
        });
  }
  block_record<IQC_WAVES>(r, [&](const Sum5<T>& w) {
#pragma unroll
    for (int k = 0; k < 5; ++k) reinterpret_cast<T*>(part)[k * IQC_MAX_WG + blockIdx.x] = w.a[k];
  });
}

struct IqcUpdate {
  const void* part;    // [5][IQC_MAX_WG], nwg records in use: f64 sums, or u64 sums of the raw bytes
  double* st;          // [SDR_IQC_NSTATE]
  int64_t n;
  int nwg, u8, dc, balance;
  double rate;
};

// the sums of the call's workgroups
template <class T>
__device__ __forceinline__ Sum5<T> sum_records(const void* part, int nwg, int lane) {
  const T* __restrict__ p = reinterpret_cast<const T*>(part);
  return fold_records<IQC_UPD_U>(nwg, lane, Sum5<T>{{T(0), T(0), T(0), T(0), T(0)}}, [&](int b) {
    Sum5<T> x;
#pragma unroll
    for (int k = 0; k < 5; ++k) x.a[k] = p[k * IQC_MAX_WG + b];
    return x;
  });
}

__global__ __launch_bounds__(64) void iqc_update_kernel(const IqcUpdate a) {
  const int lane = threadIdx.x;
  const double n = (double)a.n;
  double r[5];
  if (a.u8) {
    const Sum5<unsigned long long> S = sum_records<unsigned long long>(a.part, a.nwg, lane);
    // sums of (x - 128) / 128 and of their products from the sums of the bytes: integers below 2^53,
    // a division by a power of two, then the one division by n
    const long long sx = (long long)S.a[0], sy = (long long)S.a[1], sxx = (long long)S.a[2], syy = (long long)S.a[3], sxy = (long long)S.a[4];
    r[0] = (double)(sx - 128 * a.n) / 128.0 / n;
    r[1] = (double)(sy - 128 * a.n) / 128.0 / n;
    r[2] = (double)(sxx - 256 * sx + 16384 * a.n) / 16384.0 / n;
    r[3] = (double)(syy - 256 * sy + 16384 * a.n) / 16384.0 / n;
    r[4] = (double)(sxy - 128 * sx - 128 * sy + 16384 * a.n) / 16384.0 / n;
  } else {
    const Sum5<double> s = sum_records<double>(a.part, a.nwg, lane);
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = s.a[k] / n;
  }
  if (lane != 0) return;
  double* __restrict__ st = a.st;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 5; ++k) finite = finite && __builtin_isfinite(r[k]);
  if (!finite) {
    st[10] += 1.0;
    return;
  }
  double m[5];
  const bool first = st[9] == 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    m[k] = first ? r[k] : st[k] + a.rate * (r[k] - st[k]);
    st[k] = m[k];
  }
  st[9] += 1.0;
  const double A = m[2] - m[0] * m[0], B = m[3] - m[1] * m[1], C = m[4] - m[0] * m[1];
  const double q = C / A, t = B - q * C;
  if (A > 0.0 && t > 0.0 && __builtin_isfinite(A) && __builtin_isfinite(t)) {
    const double c2 = sqrt(A / t), c1 = -q * c2;
    st[5] = a.dc ? m[0] : 0.0;
    st[6] = a.dc ? m[1] : 0.0;
    st[7] = a.balance ? c1 : 0.0;
    st[8] = a.balance ? c2 : 1.0;
  } else {
    st[11] += 1.0;
  }
}

// the state after creation (all = 1), or four installed coefficients (all = 0)
__global__ __launch_bounds__(64) void iqc_set_kernel(double* __restrict__ st, double dI, double dQ, double c1, double c2, int all) {
  const int k = threadIdx.x;
  if (k >= SDR_IQC_NSTATE) return;
  const double v = k == 5 ? dI : k == 6 ? dQ : k == 7 ? c1 : k == 8 ? c2 : 0.0;
  if (all || (k >= 5 && k <= 8)) st[k] = v;
}

__device__ __forceinline__ f2 iqc_map(double I, double Q, const double (&c)[4]) {
  const double x = I - c[0], y = Q - c[1];
  return f2{(float)x, (float)(c[2] * x + c[3] * y)};
}

template <bool U8>
__device__ __forceinline__ f2 iqc_map_one(const void* iq, int64_t s, const double (&c)[4]) {
  if constexpr (U8) {
    const uint32_t h = reinterpret_cast<const uint16_t*>(iq)[s];
    return iqc_map((double)u8f(h & 255u), (double)u8f(h >> 8), c);
  } else {
    const f2 f = reinterpret_cast<const f2*>(iq)[s];
    return iqc_map((double)f.x, (double)f.y, c);
  }
}

// samples [0, head) alone (head is 0 or 1), then npairs pairs, then at most one sample
template <bool U8, bool OUT16>
__global__ __launch_bounds__(IQC_THREADS) void iqc_apply_kernel(const void* iq, int64_t n, int head, int64_t npairs,
                                                                const double* __restrict__ coeff, float* out) {
  using LT = std::conditional_t<U8, uint32_t, u4>;
  double c[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = coeff[k];
  const LT* v = reinterpret_cast<const LT*>(reinterpret_cast<const char*>(iq) + (U8 ? 2 : 8) * head);
  float* o = out + 2 * head;
  const int64_t step = (int64_t)gridDim.x * IQC_THREADS * IQC_U;
  const int64_t gt = (int64_t)blockIdx.x * IQC_THREADS + threadIdx.x;
  // the single samples: no pair holds them, so no other thread reads or writes them
  const bool one_head = gt == 0 && head == 1, one_tail = gt == 1 && head + 2 * npairs < n;
  f2 single = f2{0.f, 0.f};
  if (one_head) single = iqc_map_one<U8>(iq, 0, c);
  if (one_tail) single = iqc_map_one<U8>(iq, n - 1, c);
  if (one_head) *reinterpret_cast<f2*>(out) = single;
  if (one_tail) *reinterpret_cast<f2*>(out + 2 * (n - 1)) = single;
  for (int64_t i0 = (int64_t)blockIdx.x * IQC_THREADS * IQC_U + threadIdx.x; i0 < npairs; i0 += step) {
    LT x[IQC_U];
#pragma unroll
    for (int u = 0; u < IQC_U; ++u)
      if (i0 + IQC_THREADS * u < npairs) x[u] = __builtin_nontemporal_load(v + i0 + IQC_THREADS * u);
#pragma unroll
    for (int u = 0; u < IQC_U; ++u)
      if (i0 + IQC_THREADS * u < npairs) {
        f2 a, b;
        if constexpr (U8) {
          const uint32_t w = x[u];
          a = iqc_map((double)u8f(w & 255u), (double)u8f((w >> 8) & 255u), c);
          b = iqc_map((double)u8f((w >> 16) & 255u), (double)u8f(w >> 24), c);
        } else {
          const f4 f = __builtin_bit_cast(f4, x[u]);
          a = iqc_map((double)f.x, (double)f.y, c);
          b = iqc_map((double)f.z, (double)f.w, c);
        }
        store_pair(o + 4 * (i0 + IQC_THREADS * u), OUT16, f4{a.x, a.y, b.x, b.y});
      }
  }
}

}  // namespace

struct sdr_iqc {
  sdr_ctx* ctx = nullptr;
  int dtype = 0, dc = 1, balance = 1;
  double rate = 0.125;
  DevMem mem;
  double* st = nullptr;      // [SDR_IQC_NSTATE]
  char* part = nullptr;      // [5][IQC_MAX_WG] partial sums of 8 bytes
  StageTimer<3> tm;          // around the launches of a call with an estimate (sdr_iqc_set_timing)
};

extern "C" {

int sdr_iqc_create(sdr_ctx* c, int iq_dtype, const sdr_iqc_params* params, sdr_iqc** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_iqc_create: out is NULL");
  *out = nullptr;
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8) return fail(SDR_EINVAL, "sdr_iqc_create: bad iq_dtype %d", iq_dtype);
  const double rate = params != nullptr ? params->rate : 0.125;
  if (!(std::isfinite(rate) && rate > 0.0 && rate <= 1.0)) return fail(SDR_EINVAL, "sdr_iqc_create: rate=%g outside (0, 1]", rate);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_iqc* d = new (std::nothrow) sdr_iqc;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_iqc_create: out of host memory");
  d->ctx = c;
  d->dtype = iq_dtype;
  d->rate = rate;
  d->dc = params != nullptr ? (params->dc != 0) : 1;
  d->balance = params != nullptr ? (params->balance != 0) : 1;
  d->mem.get(&d->st, SDR_IQC_NSTATE);
  d->mem.get(&d->part, (size_t)IQC_MAX_WG * 5 * 8);
  const int rc = d->mem.err != hipSuccess ? create_failed(d->mem.err, "sdr_iqc_create") : sdr_iqc_reset(d);
  if (rc != SDR_OK) {
    sdr_iqc_destroy(d);
    return rc;
  }
  *out = d;
  return SDR_OK;
}

void sdr_iqc_destroy(sdr_iqc* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  d->mem.release();
  delete d;
}

int sdr_iqc_reset(sdr_iqc* d) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_iqc_reset: object is NULL");
  TRY(set_dev(d->ctx));
  hipLaunchKernelGGL(iqc_set_kernel, dim3(1), dim3(64), 0, d->ctx->stream, d->st, 0.0, 0.0, 0.0, 1.0, 1);
  HIP_TRY(hipGetLastError());
  return SDR_OK;
}

int sdr_iqc_set(sdr_iqc* d, const double coeff[4]) {
  if (d == nullptr || coeff == nullptr) return fail(SDR_EINVAL, "sdr_iqc_set: NULL argument");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(coeff[k])) return fail(SDR_EINVAL, "sdr_iqc_set: coefficient %d is not finite", k);
  TRY(set_dev(d->ctx));
  hipLaunchKernelGGL(iqc_set_kernel, dim3(1), dim3(64), 0, d->ctx->stream, d->st, coeff[0], coeff[1], coeff[2], coeff[3], 0);
  HIP_TRY(hipGetLastError());
  return SDR_OK;
}

int sdr_iqc_process_dev(sdr_iqc* d, const void* iq, int64_t n, float* out, int estimate) {
  const bool u8 = d != nullptr && d->dtype == SDR_IQ_U8;
  TRY(capture_check_call("sdr_iqc_process_dev", d, "iq", iq, u8 ? 2 : 8, n, out, !u8));
  const uintptr_t a0 = (uintptr_t)iq, o0 = (uintptr_t)out;
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  auto mark = [&](int k) { return estimate ? d->tm.mark(k, c->stream) : hipSuccess; };   // only calls with all three launches are timed
  HIP_TRY(mark(0));
  if (estimate) {
    // at most IQC_MAX_WG chunks of whole 16-B vectors, none shorter than SDR_IQC_CHUNK but the last
    int64_t chunk;
    const int nwg = chunks_of(n, SDR_IQC_CHUNK, IQC_MAX_WG, &chunk);
    if (u8) hipLaunchKernelGGL(iqc_moments_kernel<true>, dim3(nwg), dim3(IQC_THREADS), 0, c->stream, iq, n, chunk, d->part);
    else hipLaunchKernelGGL(iqc_moments_kernel<false>, dim3(nwg), dim3(IQC_THREADS), 0, c->stream, iq, n, chunk, d->part);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(1));
    const IqcUpdate up{d->part, d->st, n, nwg, u8 ? 1 : 0, d->dc, d->balance, d->rate};
    hipLaunchKernelGGL(iqc_update_kernel, dim3(1), dim3(64), 0, c->stream, up);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(2));
  }
  const int head = (int)std::min<int64_t>(n, (a0 & (u8 ? 3 : 15)) != 0 ? 1 : 0);
  const int64_t npairs = (n - head) / 2;
  const bool out16 = ((o0 + 8 * (uintptr_t)head) & 15) == 0;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, ceil_div(npairs, IQC_THREADS * IQC_U)));
  const double* coeff = d->st + 5;
#define IQC_APPLY(U8V, O16V) \
  hipLaunchKernelGGL((iqc_apply_kernel<U8V, O16V>), dim3(blocks), dim3(IQC_THREADS), 0, c->stream, iq, n, head, npairs, coeff, out)
  if (u8) {
    if (out16) IQC_APPLY(true, true);
    else IQC_APPLY(true, false);
  } else {
    if (out16) IQC_APPLY(false, true);
    else IQC_APPLY(false, false);
  }
#undef IQC_APPLY
  HIP_TRY(hipGetLastError());
  HIP_TRY(mark(3));
  return SDR_OK;
}

int sdr_iqc_run(sdr_iqc* d, const void* iq_host, int64_t n, float* out_host, int estimate) {
  TRY(capture_check_call("sdr_iqc_run", d, "iq", iq_host, 0, n, out_host, false));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const size_t es = d->dtype == SDR_IQ_U8 ? 2 : 8;
  return run_staged(c, iq_host, {1, (size_t)n * es, 0}, out_host, {1, (size_t)n * 8, (size_t)n * 8},
                    [&](void* din, void* dout) { return sdr_iqc_process_dev(d, din, n, (float*)dout, estimate); });
}

int sdr_iqc_state(sdr_iqc* d, double* host) {
  if (d == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_iqc_state: NULL argument");
  return fetch(d->ctx, d->st, SDR_IQC_NSTATE, host);
}

int sdr_iqc_set_timing(sdr_iqc* d, int on) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_iqc_set_timing: object is NULL");
  TRY(set_dev(d->ctx));
  HIP_TRY(d->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_iqc_stage_ms(sdr_iqc* d, float* ms) {
  if (d == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_iqc_stage_ms: NULL argument");
  return d->tm.elapsed(ms, "sdr_iqc_stage_ms: no timed call with an estimate (sdr_iqc_set_timing)");
}

int sdr_iqc_coeffs_dev(sdr_iqc* d, const double** dev) {
  if (d == nullptr || dev == nullptr) return fail(SDR_EINVAL, "sdr_iqc_coeffs_dev: NULL argument");
  *dev = d->st + 5;
  return SDR_OK;
}

}  // extern "C"
