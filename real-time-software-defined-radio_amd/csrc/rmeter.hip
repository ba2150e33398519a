// Modulation meter of rows of real samples (include/sdr.h sdr_rmeter_*): what a modulation monitor
// shows of every stream -- peaks, the sums behind the carrier offset and the multiplex power, the
// share of samples beyond the deviation limit and the histogram of the half-spans of consecutive
// windows -- taken from a receiver's rows where it left them.  The reference has no such stage; the
// definition is rtsdr.RowMeterModel (rowmeter.py).  Two launches, nothing returns to the host:
//
//   rmeter_reduce_kernel<SEG>  one workgroup per (row, chunk), the row on blockIdx.y.  A lane knows
//       its samples' window because every chunk is cut at the window boundaries; the host carries
//       the stream position, so the cut needs nothing from the device.
//       SEG = false (window >= SDR_RMETER_SEG): window k of the call is P = ceil(window /
//       SDR_RMETER_CHUNK) slots of L = ceil(window / P) samples, one workgroup each; a slot the
//       call has no sample of (before the carried count of the first window, behind the call's end
//       in the last) gives the empty record.  The workgroup's minimum and maximum are the window's
//       piece: no work beyond the call sums.
//       SEG = true: a chunk is G = SDR_RMETER_CHUNK / window whole windows, wave w takes windows w,
//       w + 4, .. of it: the lanes' sums run on over the chunk, the minimum and maximum go through
//       the butterfly once a window and lane 0 stores the piece.
//       Either way a contiguous range is read by sdr_chunk.h's range pass, RM_U loads in flight a
//       lane: no access leaves the range (sdr_range.h).  Per lane: f32 max and min, the finite,
//       non-finite and over counts, two f64 accumulators (the square of an f32 value is exact in
//       f64).  The lane partials become one record per chunk by sdr_chunk.h's block record.  No
//       atomics.
//   rmeter_fold_kernel  one wave per stream.  sdr_chunk.h's fold of the records gives the call's
//       sums.  The pieces go a lane each, 64 at a time: a segmented scan
//       keyed by the window (piece c belongs to window c / P, so a lane knows its segment's first
//       lane by arithmetic), started from the carried window, the pieces of four rounds loaded
//       ahead; the lane that holds a window's last piece stores its (min, max) and bins it.  Lanes of one round that hit the same bin find
//       each other by ballots over the bin's bits; the lowest adds their number to the call's
//       histogram in LDS, which goes to the stream's histogram with ordinary stores at the end.
//
// Floating-point contraction is off in this file: the bin is one subtraction and two products, as
// numpy evaluates them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "sdr_chunk.h"
#include "sdr_ctx.h"

#pragma clang fp contract(off)

using namespace sdrint;

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_WAVES = RM_THREADS / 64;
constexpr int RM_U = 4;                           // loads in flight per lane and round
constexpr int RM_FOLD_U = 8;                      // the fold's record loads in flight per lane
constexpr int RM_FOLD_PU = 4;                     // and the rounds of 64 pieces it loads ahead
constexpr int RM_BIN_BITS = 10;
static_assert(SDR_RMETER_MAX_BINS == 1 << RM_BIN_BITS, "the match looks at every bit of a bin");
static_assert(SDR_RMETER_CHUNK % 4 == 0 && SDR_RMETER_SEG <= SDR_RMETER_CHUNK, "a chunk holds at least one window below SDR_RMETER_SEG");
static_assert(SDR_RMETER_MIN_WINDOW >= 64, "a window is at least a wave's lanes");

__device__ __forceinline__ float vmax(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float vmin(float a, float b) { return b < a ? b : a; }

// a chunk's record, and a call's per row; the u32 counts hold a call's samples (fewer than 2^31)
struct RmRec {
  double sum, sumsq;
  uint32_t nfin, nonfinite, over;
  float mx, mn;
  uint32_t pad;
  __device__ __forceinline__ void combine(const RmRec& o) {
    nfin += o.nfin;
    nonfinite += o.nonfinite;
    over += o.over;
    mx = vmax(mx, o.mx);
    mn = vmin(mn, o.mn);
    sum += o.sum;
    sumsq += o.sumsq;
  }
};
static_assert(sizeof(RmRec) == 40, "five 8-byte words");

struct RmGeom {
  int64_t n, stride, W, w0;   // w0: samples of the call's first window that earlier calls took
  int64_t L;                  // !SEG: samples of a slot
  int P, G;                   // !SEG: slots per window (SEG: 1); SEG: windows per chunk
  int K, nrec, npiece;        // windows the call touches; records and pieces per row
  float limit;
};

// a lane's share of a range
struct Acc {
  uint32_t nfin = 0, nonfinite = 0, over = 0;
  float mx = -INFINITY, mn = INFINITY;
  double s = 0.0, q = 0.0;
  __device__ __forceinline__ void add(float x, float limit) {
    const uint32_t a = __builtin_bit_cast(uint32_t, x) & 0x7fffffffu;
    const bool fin = a < 0x7f800000u;
    nfin += fin ? 1u : 0u;
    nonfinite += fin ? 0u : 1u;
    over += (fin && __builtin_bit_cast(float, a) > limit) ? 1u : 0u;
    mx = (fin && x > mx) ? x : mx;
    mn = (fin && x < mn) ? x : mn;
    const double d = fin ? (double)x : 0.0;
    s += d;
    q = __builtin_fma(d, d, q);                   // (the square is exact: the fused form rounds as a product and a sum do)
  }
};

// the samples p[0 .. len) among NL lanes, this one lane t of them (rows are aligned to one float)
template <int NL>
__device__ __forceinline__ void scan_row(const float* __restrict__ p, int64_t len, int t, float limit, Acc& a) {
  scan_range<4, NL, RM_U>(
      reinterpret_cast<const char*>(p), split_range<4>((uintptr_t)p, len), t,
      [&](const u4 x, int64_t) {
        const f4 f = __builtin_bit_cast(f4, x);
        a.add(f.x, limit);
        a.add(f.y, limit);
        a.add(f.z, limit);
        a.add(f.w, limit);
      },
      [&](const char* q) { a.add(*reinterpret_cast<const float*>(q), limit); });
}

template <bool SEG>
__global__ __launch_bounds__(RM_THREADS) void rmeter_reduce_kernel(const float* __restrict__ rows, const RmGeom g, RmRec* __restrict__ rec,
                                                                   f2* __restrict__ piece) {
  const float* __restrict__ row = rows + (int64_t)blockIdx.y * g.stride;
  f2* __restrict__ pc = piece + (int64_t)blockIdx.y * g.npiece;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Acc a;
  if constexpr (SEG) {
    float cmx = -INFINITY, cmn = INFINITY;
    const int k0 = (int)blockIdx.x * g.G, k1 = k0 + g.G < g.K ? k0 + g.G : g.K;
    for (int k = k0 + w; k < k1; k += RM_WAVES) {
      int64_t lo = (int64_t)k * g.W - g.w0, hi = lo + g.W;           // window k of the call: never empty
      lo = lo > 0 ? lo : 0;
      hi = hi < g.n ? hi : g.n;
      a.mx = -INFINITY;
      a.mn = INFINITY;
      scan_row<64>(row + lo, hi - lo, lane, g.limit, a);
      const float mx = wave_max(a.mx), mn = wave_min(a.mn);
      if (lane == 0) pc[k] = f2{mn, mx};
      cmx = vmax(cmx, mx);
      cmn = vmin(cmn, mn);
    }
    a.mx = cmx;
    a.mn = cmn;
  } else {
    const int k = (int)blockIdx.x / g.P, p = (int)blockIdx.x % g.P;
    const int64_t base = (int64_t)k * g.W - g.w0;
    const int64_t o0 = (int64_t)p * g.L < g.W ? (int64_t)p * g.L : g.W, o1 = o0 + g.L < g.W ? o0 + g.L : g.W;
    const int64_t lo = base + o0 > 0 ? base + o0 : 0, hi = base + o1 < g.n ? base + o1 : g.n;
    if (hi > lo) scan_row<RM_THREADS>(row + lo, hi - lo, (int)threadIdx.x, g.limit, a);
  }
  block_record<RM_WAVES>(RmRec{a.s, a.q, a.nfin, a.nonfinite, a.over, a.mx, a.mn, 0}, [&](const RmRec& r) {
    rec[(int64_t)blockIdx.y * g.nrec + blockIdx.x] = r;
    if constexpr (!SEG) pc[blockIdx.x] = f2{r.mn, r.mx};
  });
}

struct RmFold {
  const RmRec* rec;          // [nstreams][nrec]
  const f2* piece;           // [nstreams][npiece] (min, max); piece c belongs to window c / P
  sdr_rmeter_record* st;     // [nstreams]
  unsigned long long* hist;  // [nstreams][nbins]
  f2* win;                   // [nstreams][wstride] (min, max) of the windows the call completes
  int64_t wstride, wcount;   // wcount: samples of the unfinished window behind the call
  int nrec, npiece, P, Kc, nbins;   // Kc: windows the call completes
  float scale;
};

__global__ __launch_bounds__(64) void rmeter_fold_kernel(const RmFold a) {
  __shared__ uint32_t lh[SDR_RMETER_MAX_BINS];     // the call's share of the histogram
  const int lane = threadIdx.x, s = blockIdx.x;
  sdr_rmeter_record* st = a.st + s;
  // the call's sums
  const RmRec* __restrict__ r = a.rec + (int64_t)s * a.nrec;
  const RmRec sum = fold_records<RM_FOLD_U>(a.nrec, lane, RmRec{0.0, 0.0, 0, 0, 0, -INFINITY, INFINITY, 0}, [&](int b) { return r[b]; });

  for (int b = lane; b < a.nbins; b += 64) lh[b] = 0;
  __syncthreads();
  // the windows: a piece a lane, a segmented scan keyed by the window, started from the carried one
  const f2* __restrict__ pc = a.piece + (int64_t)s * a.npiece;
  f2* __restrict__ win = a.win + (int64_t)s * a.wstride;
  float cmn = st->wmin, cmx = st->wmax;
  uint32_t empty = 0;
  for (int base0 = 0; base0 < a.npiece; base0 += 64 * RM_FOLD_PU) {
    f2 pv[RM_FOLD_PU];                                                // the pieces of RM_FOLD_PU rounds, loaded ahead of them
#pragma unroll
    for (int u = 0; u < RM_FOLD_PU; ++u) pv[u] = pc[base0 + 64 * u + lane < a.npiece ? base0 + 64 * u + lane : a.npiece - 1];
#pragma unroll
    for (int u = 0; u < RM_FOLD_PU; ++u) {
      const int base = base0 + 64 * u;
      if (base >= a.npiece) break;
      const int c = base + lane;
      const bool valid = c < a.npiece;
      const f2 v = valid ? pv[u] : f2{INFINITY, -INFINITY};
      float pmn = v.x, pmx = v.y;
      const int k = c / a.P;
      const int first = (k * a.P > base ? k * a.P : base) - base;       // the first lane of this round that holds window k
      if (lane == 0 && (base == 0 || base % a.P != 0)) {                // what came before belongs to lane 0's window
        pmn = vmin(pmn, cmn);
        pmx = vmax(pmx, cmx);
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float omn = __shfl_up(pmn, d, 64), omx = __shfl_up(pmx, d, 64);
        if (lane - d >= first) {
          pmn = vmin(pmn, omn);
          pmx = vmax(pmx, omx);
        }
      }
      const bool last = valid && (c + 1) % a.P == 0;                    // the window's last piece: its whole span so far
      bool hasbin = false;
      int bin = 0;
      if (last) {
        if (k < a.Kc) {
          win[k] = f2{pmn, pmx};
          if (pmx >= pmn) {                                             // a finite sample in it
            const float h = (pmx - pmn) * 0.5f;
            const float hb = h * a.scale;
            bin = hb < (float)a.nbins ? (int)hb : a.nbins - 1;
            hasbin = true;
          } else {
            empty += 1;
          }
        } else {                                                        // the call ends inside it
          st->wmin = pmn;
          st->wmax = pmx;
        }
      }
      // lanes with the same bin: the lowest adds their number
      unsigned long long peers = __ballot(hasbin);
      if (peers != 0) {
#pragma unroll
        for (int bit = 0; bit < RM_BIN_BITS; ++bit) {
          const bool one = ((bin >> bit) & 1) != 0;
          const unsigned long long m = __ballot(hasbin && one);
          peers &= one ? m : ~m;
        }
        if (hasbin && lane == __ffsll((long long)peers) - 1) lh[bin] += (uint32_t)__popcll(peers);
      }
      cmn = __shfl(pmn, 63, 64);
      cmx = __shfl(pmx, 63, 64);
      __syncthreads();                                                  // the next round's lanes see this round's counts
    }
  }
  unsigned long long* __restrict__ hist = a.hist + (int64_t)s * a.nbins;
  for (int b = lane; b < a.nbins; b += 64) {
    const uint32_t add = lh[b];
    if (add != 0) hist[b] += add;
  }
  empty = wave_sum(empty);
  if (lane != 0) return;
  st->n = sum.nfin;
  st->nonfinite = sum.nonfinite;
  st->over = sum.over;
  st->windows = a.Kc;
  st->sum = sum.sum;
  st->sumsq = sum.sumsq;
  st->max = sum.mx;
  st->min = sum.mn;
  st->calls += 1;
  st->total_n += sum.nfin;
  st->total_nonfinite += sum.nonfinite;
  st->total_over += sum.over;
  st->total_windows += a.Kc;
  st->empty_windows += empty;
  st->total_sum += sum.sum;
  st->total_sumsq += sum.sumsq;
  st->total_max = vmax(st->total_max, sum.mx);
  st->total_min = vmin(st->total_min, sum.mn);
  st->wcount = a.wcount;
  if (a.wcount == 0) {                                                // the call ended on a boundary
    st->wmin = INFINITY;
    st->wmax = -INFINITY;
  }
}

// the state after creation: zeros, the peaks at their identities
__global__ __launch_bounds__(64) void rmeter_reset_kernel(sdr_rmeter_record* __restrict__ st, unsigned long long* __restrict__ hist, int nbins) {
  const int s = blockIdx.x;
  for (int b = threadIdx.x; b < nbins; b += 64) hist[(int64_t)s * nbins + b] = 0;
  if (threadIdx.x != 0) return;
  sdr_rmeter_record z = {};
  z.max = z.total_max = z.wmax = -INFINITY;
  z.min = z.total_min = z.wmin = INFINITY;
  st[s] = z;
}

}  // namespace

struct sdr_rmeter {
  sdr_ctx* ctx = nullptr;
  int S = 0;
  sdr_rmeter_params prm = {};
  int64_t pos = 0;                     // samples per stream since the last reset
  int64_t last_windows = 0, wstride = 1;   // of the latest call
  DevMem mem;
  sdr_rmeter_record* st = nullptr;     // [S]
  unsigned long long* hist = nullptr;  // [S][nbins]
  GrowMem<RmRec> rec;                  // the work arrays, grown to the largest call
  GrowMem<f2> piece, win;
  StageTimer<2> tm;                    // around the two launches of a call (sdr_rmeter_set_timing)
};

namespace {

// the call-time rules, for host and device rows alike
int rm_check_call(const sdr_rmeter* d, const float* rows, int64_t stride, int64_t n, const char* what) {
  if (d == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (rows == nullptr) return fail(SDR_EINVAL, "%s: rows is NULL", what);
  if (n < 1 || n > INT32_MAX) return fail(SDR_EINVAL, "%s: n=%lld outside [1, 2^31 - 1]", what, (long long)n);
  if (d->S > 1 && stride < n) return fail(SDR_EINVAL, "%s: stride=%lld < n=%lld", what, (long long)stride, (long long)n);
  if (((uintptr_t)rows & 3) != 0) return fail(SDR_EINVAL, "%s: rows must be aligned to 4 B", what);
  return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_rmeter_create(sdr_ctx* c, int nstreams, const sdr_rmeter_params* params, sdr_rmeter** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_create: out is NULL");
  *out = nullptr;
  if (params == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_create: params is NULL");
  if (nstreams < 1 || nstreams > SDR_RMETER_MAX_STREAMS)
    return fail(SDR_EINVAL, "sdr_rmeter_create: nstreams=%d outside [1, %d]", nstreams, SDR_RMETER_MAX_STREAMS);
  if (params->window < SDR_RMETER_MIN_WINDOW || params->window > SDR_RMETER_MAX_WINDOW)
    return fail(SDR_EINVAL, "sdr_rmeter_create: window=%lld outside [%d, %d]", (long long)params->window, SDR_RMETER_MIN_WINDOW, SDR_RMETER_MAX_WINDOW);
  if (params->nbins < 1 || params->nbins > SDR_RMETER_MAX_BINS)
    return fail(SDR_EINVAL, "sdr_rmeter_create: nbins=%d outside [1, %d]", params->nbins, SDR_RMETER_MAX_BINS);
  if (!(std::isfinite(params->scale) && params->scale > 0.0f)) return fail(SDR_EINVAL, "sdr_rmeter_create: scale=%g is not finite and positive", (double)params->scale);
  if (std::isnan(params->limit)) return fail(SDR_EINVAL, "sdr_rmeter_create: limit is NaN");
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rmeter* d = new (std::nothrow) sdr_rmeter;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_rmeter_create: out of host memory");
  d->ctx = c;
  d->S = nstreams;
  d->prm = *params;
  d->mem.get(&d->st, (size_t)nstreams);
  d->mem.get(&d->hist, (size_t)nstreams * params->nbins);
  const int rc = d->mem.err != hipSuccess ? create_failed(d->mem.err, "sdr_rmeter_create") : sdr_rmeter_reset(d);
  if (rc != SDR_OK) {
    sdr_rmeter_destroy(d);
    return rc;
  }
  *out = d;
  return SDR_OK;
}

void sdr_rmeter_destroy(sdr_rmeter* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  d->mem.release();
  d->rec.release();
  d->piece.release();
  d->win.release();
  delete d;
}

int sdr_rmeter_reset(sdr_rmeter* d) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_reset: object is NULL");
  TRY(set_dev(d->ctx));
  hipLaunchKernelGGL(rmeter_reset_kernel, dim3(d->S), dim3(64), 0, d->ctx->stream, d->st, d->hist, d->prm.nbins);
  HIP_TRY(hipGetLastError());
  d->pos = 0;
  d->last_windows = 0;
  return SDR_OK;
}

int sdr_rmeter_process_dev(sdr_rmeter* d, const float* rows, int64_t stride, int64_t n) {
  TRY(rm_check_call(d, rows, stride, n, "sdr_rmeter_process_dev"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  // the cut of the call's samples at the window boundaries
  const int64_t W = d->prm.window, w0 = d->pos % W;
  const int64_t K = (w0 + n + W - 1) / W, Kc = (w0 + n) / W;
  const bool seg = W < SDR_RMETER_SEG;
  RmGeom g = {};
  g.n = n;
  g.stride = stride;
  g.W = W;
  g.w0 = w0;
  g.K = (int)K;
  g.limit = d->prm.limit;
  if (seg) {
    g.G = (int)(SDR_RMETER_CHUNK / W);
    g.P = 1;
    g.nrec = (int)ceil_div(K, g.G);
    g.npiece = (int)K;
  } else {
    g.P = (int)ceil_div(W, SDR_RMETER_CHUNK);
    g.L = ceil_div(W, g.P);
    g.nrec = g.npiece = (int)(K * g.P);
  }
  const int64_t wstride = std::max<int64_t>(Kc, 1);
  TRY(d->rec.fit((size_t)d->S * g.nrec, c->stream, "sdr_rmeter_process_dev"));
  TRY(d->piece.fit((size_t)d->S * g.npiece, c->stream, "sdr_rmeter_process_dev"));
  TRY(d->win.fit((size_t)d->S * wstride, c->stream, "sdr_rmeter_process_dev"));
  HIP_TRY(d->tm.mark(0, c->stream));
  const dim3 grid((unsigned)g.nrec, (unsigned)d->S);
  if (seg) hipLaunchKernelGGL(rmeter_reduce_kernel<true>, grid, dim3(RM_THREADS), 0, c->stream, rows, g, d->rec.p, d->piece.p);
  else hipLaunchKernelGGL(rmeter_reduce_kernel<false>, grid, dim3(RM_THREADS), 0, c->stream, rows, g, d->rec.p, d->piece.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(d->tm.mark(1, c->stream));
  const RmFold f{d->rec.p, d->piece.p, d->st, d->hist, d->win.p, wstride, (w0 + n) % W, g.nrec, g.npiece, g.P, (int)Kc, d->prm.nbins, d->prm.scale};
  hipLaunchKernelGGL(rmeter_fold_kernel, dim3(d->S), dim3(64), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  HIP_TRY(d->tm.mark(2, c->stream));
  d->pos += n;
  d->last_windows = Kc;
  d->wstride = wstride;
  return SDR_OK;
}

int sdr_rmeter_run(sdr_rmeter* d, const float* rows_host, int64_t stride, int64_t n) {
  TRY(rm_check_call(d, rows_host, stride, n, "sdr_rmeter_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  return run_staged(c, rows_host, {(size_t)d->S, (size_t)n * 4, (size_t)stride * 4}, nullptr, {},
                    [&](void* din, void*) { return sdr_rmeter_process_dev(d, (const float*)din, n, n); });
}

int sdr_rmeter_records(sdr_rmeter* d, sdr_rmeter_record* host) {
  if (d == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_records: NULL argument");
  return fetch(d->ctx, d->st, (size_t)d->S, host);
}

int sdr_rmeter_hist(sdr_rmeter* d, uint64_t* host) {
  if (d == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_hist: NULL argument");
  return fetch(d->ctx, reinterpret_cast<const uint64_t*>(d->hist), (size_t)d->S * d->prm.nbins, host);
}

int sdr_rmeter_windows(sdr_rmeter* d, float* host, int64_t cap, int64_t* counts) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_windows: object is NULL");
  if (cap < 0 || (host == nullptr && cap > 0)) return fail(SDR_EINVAL, "sdr_rmeter_windows: cap=%lld pairs without a place for them", (long long)cap);
  TRY(set_dev(d->ctx));
  const int64_t take = std::min(cap, d->last_windows);
  if (take > 0)
    HIP_TRY(hipMemcpy2DAsync(host, (size_t)cap * 8, d->win.p, (size_t)d->wstride * 8, (size_t)take * 8, d->S, hipMemcpyDeviceToHost, d->ctx->stream));
  HIP_TRY(hipStreamSynchronize(d->ctx->stream));
  if (counts != nullptr)
    for (int s = 0; s < d->S; ++s) counts[s] = d->last_windows;      // the streams share the position
  return SDR_OK;
}

int sdr_rmeter_state_dev(sdr_rmeter* d, const sdr_rmeter_record** dev, const uint64_t** hist_dev) {
  if (d == nullptr || (dev == nullptr && hist_dev == nullptr)) return fail(SDR_EINVAL, "sdr_rmeter_state_dev: NULL argument");
  if (dev != nullptr) *dev = d->st;
  if (hist_dev != nullptr) *hist_dev = reinterpret_cast<const uint64_t*>(d->hist);
  return SDR_OK;
}

int sdr_rmeter_set_timing(sdr_rmeter* d, int on) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_set_timing: object is NULL");
  TRY(set_dev(d->ctx));
  HIP_TRY(d->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_rmeter_stage_ms(sdr_rmeter* d, float* ms) {
  if (d == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_rmeter_stage_ms: NULL argument");
  return d->tm.elapsed(ms, "sdr_rmeter_stage_ms: no timed call (sdr_rmeter_set_timing)");
}

}  // extern "C"
