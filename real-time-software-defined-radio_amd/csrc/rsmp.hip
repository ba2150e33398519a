// Rational resampler for device rows (include/sdr.h sdr_rsmp_*): nrows rows of f32 samples, real
// or interleaved complex, resampled by U / D through one real filter h of T taps designed at U
// times the input rate.  The definition, per row and component (x zero before the stream start),
//   y[m] = U sum_j h[j] xu[m D - j],   xu[i] = x[i / U] if U divides i, else 0
// is computed in polyphase form (P = ceil(T / U), h zero-padded to P U, m D = s U + r, 0 <= r < U)
//   y[m] = sum_{q < P} g[r + q U] x[s - q],   g = f32(U h)
// as one f32 FMA chain over q = 0 .. P - 1 per output and component, the first term a product
// (one tap of 1.0 copies the sample's bits, -0 included).  An output's bits depend only on g and
// on the P samples of its window -- not on where a call or a tile begins.
//
// Work: a workgroup takes tiles of To = C U R outputs of one row (R = 4 outputs per item, 2 where
// U > 512; C whole chunks of U R outputs, as many as SDR_RSMP_TILE and 64 KB of LDS hold, at least
// one).  To is a multiple of U, so every tile starts at phase 0, on input sample S0 = tile To D / U
// (64-bit), and everything inside the tile is 32-bit arithmetic relative to it.  Per tile:
//   stage  the tile's input span, samples S0 - (P - 1) .. S0 + To D / U - 1, into LDS.  Where the
//          span lies inside the caller's row: 16-byte buffer loads from the 16-byte boundary at or
//          below its first sample (the LDS copy starts `sh` samples early).  At the row's two ends:
//          sample by sample across the seam between the object's history (the P - 1 samples before
//          the call) and the caller's row (sdr_stream.h).  No access leaves the row's n samples or
//          the history: the gaps between rows are never read;
//   FMA    item (c, p), p < U, owns the R outputs m' = (c R + k) U + p, k < R, of the tile: they
//          share the phase r = (p D) mod U, so one tap read per q serves R outputs and both
//          components; their samples are D apart.  The taps sit in LDS as g[q U + r]: neighbouring
//          lanes read neighbouring taps where D mod U = 1, and samples about D / U apart.  Complex
//          samples are 8-byte LDS reads.  (No skew of the staging: where 2 D / U dwords is a
//          multiple of 64 the lanes' sample reads share a bank -- DESIGN.md §10.)
// The history update is a second launch (sdr_stream.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

#include "sdr_ctx.h"
#include "sdr_mma.h"
#include "sdr_stream.h"

using namespace sdrint;

namespace {

constexpr int RSMP_THREADS = 256;
constexpr size_t RSMP_LDS = 64 * 1024;             // taps + staging of a workgroup: two per compute unit at the least
constexpr int RSMP_MAX_GRID = 1 << 20;             // tiles per row beyond this are looped over

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct RsmpArgs {
  const float* in;         // row r: n samples from in + r in_stride samples
  const float* hist;       // [nrows][P - 1] samples: what preceded the call
  const float* taps;       // [P U]: g[q U + r] = f32(U h[q U + r])
  float* out;
  int64_t n, Mo;           // samples in, out per row
  int64_t in_stride, out_stride;
  int64_t tiles;           // per row
  int U, D, P;
  int To;                  // outputs per tile (a multiple of U R)
  int Sd;                  // input samples a tile advances by: To D / U
  int items;               // To / R
  int o_xs;                // LDS offset of the staging, bytes
};

template <int E, int R>
__global__ __launch_bounds__(RSMP_THREADS) void rsmp_kernel(const RsmpArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsmp_lds[];
  using ST = std::conditional_t<E == 2, float2, float>;
  constexpr int ES = 4 * E;                         // bytes per sample
  const int tid = threadIdx.x;
  const int U = A.U, D = A.D, P = A.P, HL = A.P - 1;
  const int L = A.Sd + HL;                          // samples of a tile's span
  const float* g_s = reinterpret_cast<const float*>(rsmp_lds);
  ST* x_s = reinterpret_cast<ST*>(rsmp_lds + A.o_xs);

  for (int i = tid; i < P * U; i += RSMP_THREADS) reinterpret_cast<float*>(rsmp_lds)[i] = A.taps[i];

  const int64_t row = blockIdx.y;
  const char* rowb = reinterpret_cast<const char*>(A.in) + row * A.in_stride * ES;
  const char* hb = reinterpret_cast<const char*>(A.hist) + row * (int64_t)HL * ES;
  ST* orow = reinterpret_cast<ST*>(A.out) + row * A.out_stride;

  for (int64_t t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    if (t != (int64_t)blockIdx.x) __syncthreads();  // the previous tile's reads are done
    // ---- stage: x_s[sh + i] = sample sb + i of the call's row, 0 <= i < L
    const int64_t S0 = t * A.Sd;                    // < n: the tile has an output
    const int64_t sb = S0 - HL;
    const int sh = (int)((((uintptr_t)rowb + (uintptr_t)(sb * ES)) & 15) / ES);
    const int64_t e0 = sb - sh;                     // the sample on the 16-byte boundary
    const int nq = ((L + sh) * ES + 15) / 16;       // 16-byte pieces from there
    if (e0 >= 0 && e0 * ES + (int64_t)16 * nq <= A.n * ES) {   // (uniform) inside the caller's row
      const __amdgpu_buffer_rsrc_t r = mm_rsrc(rowb + e0 * ES, (int64_t)16 * nq);
#pragma unroll 4
      for (int j = tid; j < nq; j += RSMP_THREADS)
        reinterpret_cast<u4v*>(x_s)[j] = __builtin_amdgcn_raw_buffer_load_b128(r, 16 * j, 0, 0);
    } else {
      // the seam load of sdr_stream.h, in samples
      const int64_t be = sb > 0 ? sb : 0;
      const int64_t left = A.n - be;                // >= 1
      const Seam<ES> seam{mm_rsrc(rowb + be * ES, (left < L ? left : L) * ES), mm_rsrc(hb, (int64_t)HL * ES),
                        (int)(sb - be),             // <= 0
                        S0 < HL ? (int)S0 : HL};    // the history's index of x_s[sh]: sb + HL; from HL on outside it
      for (int i = tid; i < L; i += RSMP_THREADS) x_s[sh + i] = __builtin_bit_cast(ST, seam.template load<ES>(i));
    }
    __syncthreads();                                // x_s (and, the first time, the taps) complete

    // ---- FMA chains: item (c, p) -> outputs m' = (c R + k) U + p, k < R, all of phase (p D) mod U
    const int64_t m0 = t * A.To;
    const int64_t mleft = A.Mo - m0;                // >= 1
    for (int it = tid; it < A.items; it += RSMP_THREADS) {
      const int c = (int)((unsigned)it / (unsigned)U), p = it - c * U;
      const int pd = p * D, sq = (int)((unsigned)pd / (unsigned)U), r = pd - sq * U;
      const float* gp = g_s + r;
      const ST* xp = x_s + (sh + HL + c * R * D + sq);   // the newest sample of output k = 0; k's are D on
      float ar[R], ai[R];
      {
        const float g = gp[0];
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const ST x = xp[k * D];
          if constexpr (E == 2) {
            ar[k] = g * x.x;
            ai[k] = g * x.y;
          } else {
            ar[k] = g * x;
          }
        }
      }
#pragma unroll 2
      for (int q = 1; q < P; ++q) {
        const float g = gp[q * U];
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const ST x = xp[k * D - q];
          if constexpr (E == 2) {
            ar[k] = fmaf(g, x.x, ar[k]);
            ai[k] = fmaf(g, x.y, ai[k]);
          } else {
            ar[k] = fmaf(g, x, ar[k]);
          }
        }
      }
      const int mb = c * R * U + p;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int m = mb + k * U;
        if (m < mleft) {
          if constexpr (E == 2) orow[m0 + m] = float2{ar[k], ai[k]};
          else orow[m0 + m] = ar[k];
        }
      }
    }
  }
}

}  // namespace

struct sdr_rsmp {
  sdr_ctx* ctx = nullptr;
  int nrows = 0, E = 0, T = 0, U = 0, D = 0, P = 0, R = 0, To = 0;
  int64_t step = 0;                     // a call's n is a multiple of this: D / gcd(U, D)
  size_t o_xs = 0, lds = 0;
  float* taps = nullptr;
  StreamHist hist;                      // the P - 1 samples before the next call, per row
  int64_t pos = 0;
};

extern "C" {

int sdr_rsmp_create(sdr_ctx* c, int nrows, int elems, const double* b, int taps, int up, int down, sdr_rsmp** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rsmp_create: out is NULL");
  *out = nullptr;
  if (nrows < 1 || nrows > SDR_RSMP_MAX_ROWS)
    return fail(SDR_EINVAL, "sdr_rsmp_create: nrows=%d outside [1, %d]", nrows, SDR_RSMP_MAX_ROWS);
  if (elems != SDR_RSMP_REAL && elems != SDR_RSMP_COMPLEX)
    return fail(SDR_EINVAL, "sdr_rsmp_create: elems=%d is neither SDR_RSMP_REAL nor SDR_RSMP_COMPLEX", elems);
  if (up < 1 || up > SDR_RSMP_MAX_FACTOR) return fail(SDR_EINVAL, "sdr_rsmp_create: up=%d outside [1, %d]", up, SDR_RSMP_MAX_FACTOR);
  if (down < 1 || down > SDR_RSMP_MAX_FACTOR)
    return fail(SDR_EINVAL, "sdr_rsmp_create: down=%d outside [1, %d]", down, SDR_RSMP_MAX_FACTOR);
  if (taps < 1 || taps > SDR_RSMP_MAX_TAPS)
    return fail(SDR_EINVAL, "sdr_rsmp_create: taps=%d outside [1, %d]", taps, SDR_RSMP_MAX_TAPS);
  if ((taps + up - 1) / up > SDR_RSMP_MAX_PHASE_TAPS)
    return fail(SDR_EINVAL, "sdr_rsmp_create: taps=%d at up=%d is more than %d taps per phase", taps, up, SDR_RSMP_MAX_PHASE_TAPS);
  if (b == nullptr) return fail(SDR_EINVAL, "sdr_rsmp_create: taps pointer is NULL");
  TRY(taps_finite(b, taps, "sdr_rsmp_create"));
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rsmp* d = new (std::nothrow) sdr_rsmp;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_rsmp_create: out of host memory");
  d->ctx = c;
  d->nrows = nrows;
  d->E = elems;
  d->T = taps;
  d->U = up;
  d->D = down;
  d->P = (taps + up - 1) / up;
  int g = up, r = down;
  while (r != 0) {
    const int t = g % r;
    g = r;
    r = t;
  }
  d->step = down / g;
  // the tile: whole chunks of U R outputs (R D input samples each), as many as SDR_RSMP_TILE and
  // the LDS hold; one chunk always fits (<= 4096 + 255 + 6 samples of 8 B beside <= 5119 taps)
  d->R = up <= SDR_RSMP_TILE / 4 ? 4 : 2;
  const int es = 4 * elems, chunk = up * d->R;
  d->o_xs = up16((size_t)d->P * up * sizeof(float));
  auto xs_bytes = [&](int nc) { return up16(((size_t)nc * d->R * down + d->P - 1 + 6) * es); };
  int nc = SDR_RSMP_TILE / chunk;
  while (nc > 1 && d->o_xs + xs_bytes(nc) > RSMP_LDS) --nc;
  d->To = nc * chunk;
  d->lds = d->o_xs + xs_bytes(nc);
  if (d->lds > RSMP_LDS) {                                     // (not inside the limits)
    const size_t lds = d->lds;
    delete d;
    return fail(SDR_EHIP, "sdr_rsmp_create: %zu B of LDS", lds);
  }
  std::vector<float> g32((size_t)d->P * up, 0.f);
  for (int j = 0; j < taps; ++j) g32[j] = (float)((double)up * b[j]);
  hipError_t e = upload(&d->taps, g32.data(), g32.size(), c->stream);
  if (e == hipSuccess) e = d->hist.alloc((size_t)nrows * (d->P - 1) * es, 0, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host vector is read until here)
  if (e != hipSuccess) {
    sdr_rsmp_destroy(d);
    return create_failed(e, "sdr_rsmp_create");
  }
  *out = d;
  return SDR_OK;
}

void sdr_rsmp_destroy(sdr_rsmp* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  (void)hipFree(d->taps);
  d->hist.free();
  delete d;
}

int sdr_rsmp_reset(sdr_rsmp* d) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_rsmp_reset: object is NULL");
  TRY(set_dev(d->ctx));
  HIP_TRY(d->hist.reset(d->ctx->stream));
  d->pos = 0;
  return SDR_OK;
}

int sdr_rsmp_position(sdr_rsmp* d, int64_t* in_samples) {
  if (d == nullptr || in_samples == nullptr) return fail(SDR_EINVAL, "sdr_rsmp_position: NULL argument");
  *in_samples = d->pos;
  return SDR_OK;
}

// the call-time rules that hold for host and device buffers alike
static int rsmp_check_call(sdr_rsmp* d, const float* in, int64_t n, int64_t in_stride, const float* out, int64_t out_stride,
                           const char* what) {
  if (d == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (in == nullptr || out == nullptr) return fail(SDR_EINVAL, "%s: in or out is NULL", what);
  if (n < 1 || n % d->step != 0)
    return fail(SDR_EINVAL, "%s: n=%lld must be >= 1 and a multiple of down/gcd(up, down)=%lld", what, (long long)n, (long long)d->step);
  const int64_t Mo = n / d->step * (d->U / (d->D / d->step));
  if (n > INT32_MAX || Mo > INT32_MAX)
    return fail(SDR_EINVAL, "%s: n=%lld or its %lld outputs per row reach 2^31", what, (long long)n, (long long)Mo);
  if (in_stride < n) return fail(SDR_EINVAL, "%s: in_stride=%lld < n=%lld", what, (long long)in_stride, (long long)n);
  if (out_stride < Mo)
    return fail(SDR_EINVAL, "%s: out_stride=%lld < n up/down=%lld", what, (long long)out_stride, (long long)Mo);
  const uintptr_t mask = 4 * d->E - 1;
  if (((uintptr_t)in & mask) != 0 || ((uintptr_t)out & mask) != 0)
    return fail(SDR_EINVAL, "%s: in and out must be aligned to one sample (%d B)", what, 4 * d->E);
  const uintptr_t es = 4 * d->E;
  const uintptr_t i0 = (uintptr_t)in, i1 = i0 + ((uintptr_t)(d->nrows - 1) * in_stride + n) * es;
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((uintptr_t)(d->nrows - 1) * out_stride + Mo) * es;
  if (o0 < i1 && i0 < o1) return fail(SDR_EINVAL, "%s: out's extent overlaps in's", what);
  return SDR_OK;
}

int sdr_rsmp_process_dev(sdr_rsmp* d, const float* in, int64_t n, int64_t in_stride, float* out, int64_t out_stride) {
  TRY(rsmp_check_call(d, in, n, in_stride, out, out_stride, "sdr_rsmp_process_dev"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  RsmpArgs A;
  A.in = in;
  A.hist = static_cast<const float*>(d->hist.current());
  A.taps = d->taps;
  A.out = out;
  A.n = n;
  A.Mo = n / d->step * (d->U / (d->D / d->step));
  A.in_stride = in_stride;
  A.out_stride = out_stride;
  A.tiles = ceil_div(A.Mo, d->To);
  A.U = d->U;
  A.D = d->D;
  A.P = d->P;
  A.To = d->To;
  A.Sd = d->To / d->U * d->D;
  A.items = d->To / d->R;
  A.o_xs = (int)d->o_xs;
  const dim3 grid((unsigned)std::min<int64_t>(A.tiles, RSMP_MAX_GRID), (unsigned)d->nrows), blk(RSMP_THREADS);
  if (d->E == 2) {
    if (d->R == 4) rsmp_kernel<2, 4><<<grid, blk, d->lds, c->stream>>>(A);
    else rsmp_kernel<2, 2><<<grid, blk, d->lds, c->stream>>>(A);
  } else {
    if (d->R == 4) rsmp_kernel<1, 4><<<grid, blk, d->lds, c->stream>>>(A);
    else rsmp_kernel<1, 2><<<grid, blk, d->lds, c->stream>>>(A);
  }
  HIP_TRY(hipGetLastError());
  if (d->E == 2) HIP_TRY(d->hist.advance<float2>(c->stream, in, n, in_stride, d->nrows, d->P - 1));
  else HIP_TRY(d->hist.advance<float>(c->stream, in, n, in_stride, d->nrows, d->P - 1));
  d->pos += n;
  return SDR_OK;
}

int sdr_rsmp_run(sdr_rsmp* d, const float* in_host, int64_t n, int64_t in_stride, float* out_host, int64_t out_stride) {
  TRY(rsmp_check_call(d, in_host, n, in_stride, out_host, out_stride, "sdr_rsmp_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const size_t es = 4 * (size_t)d->E, rows = (size_t)d->nrows;
  const int64_t Mo = n / d->step * (d->U / (d->D / d->step));
  return run_staged(c, in_host, {rows, (size_t)n * es, (size_t)in_stride * es}, out_host, {rows, (size_t)Mo * es, (size_t)out_stride * es},
                    [&](void* din, void* dout) { return sdr_rsmp_process_dev(d, (const float*)din, n, n, (float*)dout, Mo); });
}

}  // extern "C"
