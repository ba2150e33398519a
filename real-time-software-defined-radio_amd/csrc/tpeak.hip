// True peak of rows of audio samples (include/sdr.h sdr_tpeak_*): the polyphase interpolator of
// ITU-R BS.1770-4 annex 2 -- or any table of up to 8 phases of up to 32 taps -- of which only maxima
// are kept, per segment of stream position, beside the sample peak.  The reference has no such
// stage; the definition is rtsdr.TruePeakModel (truepeak.py), which the device equals bit for bit:
//   y[t][p] = sum_k f64(h[p][k]) f64(x[t - k]),  f64 from 0.0, k ascending; an f32 x f32 product is
//   exact in f64, so the fused multiply-adds here round as numpy's products and sums do.
// Two launches per call, nothing returns to the host:
//
//   tpeak_reduce_kernel<UP, TAPS>  one workgroup per (row, piece), row = stream x channel on
//       blockIdx.y.  Segment k of the call is P = ceil(segment / TP_CHUNK) pieces of L = ceil(segment
//       / P) samples: the cut needs only the stream position, which the host carries, and a piece's
//       maxima belong to one segment.  A piece the call has no sample of gives the empty record.
//       The piece is walked in tiles of 256 lanes x TP_R = 8 samples whose origin is the 16-B
//       boundary at or below the piece's first sample: a lane whose 8 samples lie inside the piece
//       reads them, and the vectors that hold the taps - 1 samples in front of them, as 16-B
//       vectors whatever the row's alignment.  The lanes at either end of a piece and at the start
//       of a call read element by element through the seam load (sdr_stream.h), from the row or,
//       in front of the call's first sample, from the carried history; both descriptors cover
//       exactly what may be read.  A lane forms its 8 x UP values as f64 chains in registers, phase
//       by phase: one coefficient -- wave-uniform, a scalar load -- feeds the 8 samples' chains.  A
//       value is finite exactly when the taps samples under it are (no sum of taps f32 x f32
//       products leaves f64's range), so a wave whose samples are all finite takes the form without
//       a test per value: a sample's maximum over the phases, taken where the sample belongs to the
//       piece; any other wave tests every value.  <4, 12> is BS.1770's shape at compile time;
//       <0, 32> takes up and taps at run time (the taps loop unrolled to 32 behind a uniform test).
//       The lane records become the piece's by sdr_chunk.h's block record.  No atomics.
//   tpeak_fold_kernel  one wave per (stream, channel): sdr_chunk.h's fold of the records gives
//       the call's maxima and count; the segments go a lane each, 64 at a time (their P pieces one
//       after the other), or where P > 64 one after the other with the pieces a lane each, into
//       the carried open segment and the rings of the latest `cap` completed ones; lane 0 writes
//       the record; the lanes then store the row's new history, the last taps - 1 samples of (old
//       history, the call).  Maxima do not depend on the order they are taken in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>
#include <vector>

#include "sdr_chunk.h"
#include "sdr_ctx.h"
#include "sdr_stream.h"

using namespace sdrint;

namespace {

constexpr int TP_T = 256, TP_R = 8, TP_TILE = TP_T * TP_R, TP_WAVES = TP_T / 64;
constexpr int64_t TP_CHUNK = 4096;               // the longest piece of a segment
constexpr int TP_FOLD_U = 4;                      // the fold's record loads in flight per lane
static_assert(TP_R == 8, "a whole lane's samples are two 16-B vectors");
static_assert(SDR_TPEAK_MAX_TAPS == 32 && SDR_TPEAK_MAX_UP == 8, "the run-time kernel's unrolled taps loop; include/sdr.h");

// a piece's record, and a call's per row
struct TpRec {
  double pk, sp;
  uint32_t nonfinite, pad;
  __device__ __forceinline__ void combine(const TpRec& o) {
    pk = o.pk > pk ? o.pk : pk;
    sp = o.sp > sp ? o.sp : sp;
    nonfinite += o.nonfinite;
  }
};
static_assert(sizeof(TpRec) == 24, "three 8-byte words");
// (a call's count: fewer than 2^31 samples of at most 8 values would overflow 32 bits)
struct TpSum {
  double pk, sp;
  unsigned long long nonfinite;
  __device__ __forceinline__ void combine(const TpSum& o) {
    pk = o.pk > pk ? o.pk : pk;
    sp = o.sp > sp ? o.sp : sp;
    nonfinite += o.nonfinite;
  }
};

struct TpArgs {
  const float* x[2];       // a channel's rows; row (s, ch) is x[ch] + s stride
  const float* hist;       // [rows][taps - 1]: the samples in front of the call
  const double* tab;       // [up][taps]
  TpRec* piece;            // [rows][npiece]
  int64_t n, stride, seg, pos0, L;   // pos0: samples of the call's first segment that earlier calls took
  int P, nch, up, taps, npiece;
};

// a lane's share of a piece
struct TpLane {
  double pk = 0.0;
  float sp = 0.f;
  uint32_t nonfinite = 0;
};

// the UP x TP_R values over the window w: w[TM1 + i] is the lane's sample i, w[TM1 + i - k] the one
// k in front of it.  FAST: every value is finite -- a sample's maximum over the phases is formed
// without a test and taken where the sample belongs to the piece.  valid: bit i set where sample i does.
template <int UPC, int TAPSC, bool FAST>
__device__ __forceinline__ void tp_values(const float (&w)[TP_R + TAPSC - 1], const double* __restrict__ tab, int up, int taps, uint32_t valid,
                                          TpLane& l) {
  constexpr int TM1 = TAPSC - 1, W = TP_R + TM1;
  double xd[W], mi[TP_R];
#pragma unroll
  for (int j = 0; j < W; ++j) xd[j] = (double)w[j];
#pragma unroll
  for (int i = 0; i < TP_R; ++i) {
    const float q = __builtin_fabsf(w[TM1 + i]);
    l.sp = (((valid >> i) & 1u) != 0 && (FAST || q <= FLT_MAX) && q > l.sp) ? q : l.sp;
    mi[i] = 0.0;
  }
  auto phase = [&](int p) {
    double acc[TP_R];
#pragma unroll
    for (int i = 0; i < TP_R; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < TAPSC; ++k)
      if (UPC != 0 || k < taps) {
        const double hk = tab[p * taps + k];
#pragma unroll
        for (int i = 0; i < TP_R; ++i) acc[i] = __builtin_fma(hk, xd[TM1 + i - k], acc[i]);
      }
#pragma unroll
    for (int i = 0; i < TP_R; ++i) {
      const double v = __builtin_fabs(acc[i]);
      if constexpr (FAST) {
        mi[i] = __builtin_fmax(mi[i], v);
      } else if (((valid >> i) & 1u) != 0) {
        if (v <= DBL_MAX) l.pk = v > l.pk ? v : l.pk;
        else l.nonfinite += 1;
      }
    }
  };
  if constexpr (UPC != 0) {
    static_for<0, UPC>([&](auto p) { phase(p); });
  } else {
#pragma unroll 1
    for (int p = 0; p < up; ++p) phase(p);
  }
  if constexpr (FAST) {
#pragma unroll
    for (int i = 0; i < TP_R; ++i) l.pk = (((valid >> i) & 1u) != 0 && mi[i] > l.pk) ? mi[i] : l.pk;
  }
}

template <int UPC, int TAPSC>
__global__ __launch_bounds__(TP_T) void tpeak_reduce_kernel(const TpArgs a) {
  constexpr int TM1 = TAPSC - 1, W = TP_R + TM1, NP = (TM1 + 3) / 4;   // NP: the 16-B vectors that hold TM1 samples
  const int up = UPC != 0 ? UPC : a.up, taps = UPC != 0 ? TAPSC : a.taps;
  const int tid = threadIdx.x, hl = taps - 1;
  const int64_t rowi = blockIdx.y;
  const float* __restrict__ row = a.x[rowi % a.nch] + (rowi / a.nch) * a.stride;
  // the piece, in samples of the call
  const int64_t k = blockIdx.x / a.P, p = blockIdx.x % a.P, base = k * a.seg - a.pos0;
  const int64_t o0 = p * a.L < a.seg ? p * a.L : a.seg, o1 = o0 + a.L < a.seg ? o0 + a.L : a.seg;
  const int64_t lo = base + o0 > 0 ? base + o0 : 0, hi = base + o1 < a.n ? base + o1 : a.n;
  TpLane l;
  if (hi > lo) {
    const int64_t org = lo - (int64_t)(((uintptr_t)(row + lo) >> 2) & 3);   // row + org is on a 16-B boundary
    const bool need_hist = org - TM1 < 0;                                    // (the same in every lane)
    const int64_t a0 = need_hist ? 0 : org - TM1;                            // nothing below row + a0 is read
    Seam<4> sm;
    sm.in = mm_rsrc(row + a0, (hi - a0) * 4);
    sm.hist = mm_rsrc(a.hist + rowi * hl, (int64_t)hl * 4);
    for (int64_t t0 = org; t0 < hi; t0 += TP_TILE) {
      if (t0 + (int64_t)(tid & ~63) * TP_R >= hi) break;                     // nothing left for this wave
      const int64_t i0 = t0 + (int64_t)tid * TP_R;
      const bool full = i0 >= lo && i0 + TP_R <= hi;
      // the window's element j is sample i0 - TM1 + j of the call: element e of the descriptor over the
      // row from a0 on, element i0 - TM1 + hl + j of the history (which ends in front of sample 0)
      sm.d0 = (int)(i0 - TM1 - a0);
      sm.h0 = need_hist ? (int)(i0 - TM1 + hl) : 0;
      float w[W];
      auto from_seam = [&](auto j) {
        constexpr int J = decltype(j)::value;
        w[J] = __builtin_bit_cast(float, need_hist ? sm.template load<4, J>(0) : sm.template load_in<4, J>(0));
      };
      if (full && i0 >= 4 * NP) {
        // the NP vectors in front of the lane's own hold its TM1 samples in front: inside the row, like them
        static_for<0, NP>([&](auto q) {
          constexpr int J = 4 * decltype(q)::value - (4 * NP - TM1);        // the window's element of the vector's first
          const f4 v = *reinterpret_cast<const f4*>(row + i0 - TM1 + J);
          if constexpr (J >= 0) w[J] = v.x;
          if constexpr (J + 1 >= 0) w[J + 1] = v.y;
          if constexpr (J + 2 >= 0) w[J + 2] = v.z;
          w[J + 3] = v.w;
        });
      } else {
        static_for<0, TM1>(from_seam);
      }
      if (full) {
        const f4 u = *reinterpret_cast<const f4*>(row + i0), v = *reinterpret_cast<const f4*>(row + i0 + 4);
        w[TM1 + 0] = u.x; w[TM1 + 1] = u.y; w[TM1 + 2] = u.z; w[TM1 + 3] = u.w;
        w[TM1 + 4] = v.x; w[TM1 + 5] = v.y; w[TM1 + 6] = v.z; w[TM1 + 7] = v.w;
      } else {
        static_for<TM1, W>(from_seam);
      }
      bool fin = true;
#pragma unroll
      for (int j = 0; j < W; ++j) fin = fin && __builtin_isfinite(w[j]);
      // the lane's samples [v0, v1) belong to the piece
      const int v0 = lo - i0 > 0 ? (int)(lo - i0 < TP_R ? lo - i0 : TP_R) : 0, v1 = hi - i0 < TP_R ? (int)(hi - i0 > 0 ? hi - i0 : 0) : TP_R;
      const uint32_t valid = ((1u << v1) - 1u) & ~((1u << v0) - 1u);
      if (__ballot(!fin) == 0) tp_values<UPC, TAPSC, true>(w, a.tab, up, taps, valid, l);
      else tp_values<UPC, TAPSC, false>(w, a.tab, up, taps, valid, l);
    }
  }
  block_record<TP_WAVES>(TpRec{l.pk, (double)l.sp, l.nonfinite, 0}, [&](const TpRec& r) { a.piece[rowi * a.npiece + blockIdx.x] = r; });
}

struct TpFold {
  const TpRec* piece;      // [rows][npiece], piece c of segment c / P of the call
  double* ring_pk;         // [rows][cap]: completed segment g at g % cap
  double* ring_sp;
  sdr_tpeak_record* st;    // [rows]
  float* hist;             // [rows][hl]
  const float* x[2];
  int64_t stride, n, seg, pos0, done0;   // done0: segments completed before the call
  int nch, P, npiece, cap, hl;
};

__global__ __launch_bounds__(64) void tpeak_fold_kernel(const TpFold a) {
  const int lane = threadIdx.x;
  const int64_t rowi = blockIdx.x;
  const TpRec* __restrict__ pc = a.piece + rowi * a.npiece;
  sdr_tpeak_record* st = a.st + rowi;
  double* __restrict__ ring_pk = a.ring_pk + rowi * a.cap;
  double* __restrict__ ring_sp = a.ring_sp + rowi * a.cap;
  const TpSum sum = fold_records<TP_FOLD_U>(a.npiece, lane, TpSum{0.0, 0.0, 0}, [&](int b) {
    const TpRec r = pc[b];
    return TpSum{r.pk, r.sp, r.nonfinite};
  });
  // the segments: segment j of the call takes the carried open maxima (j = 0) and its P pieces
  const int64_t nseg = (a.pos0 + a.n + a.seg - 1) / a.seg, ndone = (a.pos0 + a.n) / a.seg;
  const double open_pk = st->open_peak, open_sp = st->open_sample_peak;
  const bool by_lane = a.P <= 64;
  for (int64_t j0 = 0; j0 < nseg; j0 += by_lane ? 64 : 1) {
    const int64_t j = by_lane ? j0 + lane : j0;
    double pk = 0.0, sp = 0.0;
    if (by_lane) {
      if (j < nseg)
        for (int q = 0; q < a.P; ++q) {
          const TpRec r = pc[j * a.P + q];
          pk = r.pk > pk ? r.pk : pk;
          sp = r.sp > sp ? r.sp : sp;
        }
    } else {
      for (int q = lane; q < a.P; q += 64) {
        const TpRec r = pc[j * a.P + q];
        pk = r.pk > pk ? r.pk : pk;
        sp = r.sp > sp ? r.sp : sp;
      }
      pk = wave_max(pk);
      sp = wave_max(sp);
    }
    if (j == 0) {
      pk = open_pk > pk ? open_pk : pk;
      sp = open_sp > sp ? open_sp : sp;
    }
    if (j < nseg && (by_lane || lane == 0)) {
      if (j >= ndone) {                                                  // the call ends inside it
        st->open_peak = pk;
        st->open_sample_peak = sp;
      } else if (j + a.cap >= ndone) {                                   // among the latest cap: no two lanes store to one slot
        ring_pk[(a.done0 + j) % a.cap] = pk;
        ring_sp[(a.done0 + j) % a.cap] = sp;
      }
    }
  }
  if (lane == 0) {
    if (ndone == nseg) st->open_peak = st->open_sample_peak = 0.0;       // the call ended on a boundary
    st->n = a.n;
    st->nonfinite = (int64_t)sum.nonfinite;
    st->peak = sum.pk;
    st->sample_peak = sum.sp;
    st->calls += 1;
    st->total_n += a.n;
    st->total_nonfinite += (int64_t)sum.nonfinite;
    st->total_peak = sum.pk > st->total_peak ? sum.pk : st->total_peak;
    st->total_sample_peak = sum.sp > st->total_sample_peak ? sum.sp : st->total_sample_peak;
    st->segments = a.done0 + ndone;
  }
  // the new history: the last hl samples of (old history, the call); every lane reads in front of
  // the one store instruction of the wave
  if (lane < a.hl) {
    const float* __restrict__ row = a.x[rowi % a.nch] + (rowi / a.nch) * a.stride;
    float* h = a.hist + rowi * a.hl;
    const int64_t i = a.n - a.hl + lane;
    const float v = i >= 0 ? row[i] : h[a.hl + i];
    h[lane] = v;
  }
}

// BS.1770-4 annex 2, phases 0 and 1 (x 8192); phases 2 and 3 are phases 1 and 0 reversed
const int TP_BS1770[2][12] = {{14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68},
                              {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155}};

int tp_check_rows(const char* what, const char* name, const float* p, int64_t stride, int64_t n) {
  if (n < 1 || n > INT32_MAX) return fail(SDR_EINVAL, "%s: n=%lld outside [1, 2^31 - 1]", what, (long long)n);
  if (stride < n) return fail(SDR_EINVAL, "%s: stride=%lld < n=%lld", what, (long long)stride, (long long)n);
  if (((uintptr_t)p & 3) != 0) return fail(SDR_EINVAL, "%s: %s must be aligned to 4 B", what, name);
  return SDR_OK;
}

}  // namespace

struct sdr_tpeak {
  sdr_ctx* ctx = nullptr;
  int S = 0, nch = 1, up = 0, taps = 0, cap = 0;
  int64_t seg = 0;
  int64_t pos = 0;                     // samples per stream since the last reset
  DevMem mem;
  double* tab = nullptr;               // [up][taps]
  float* hist = nullptr;               // [S nch][taps - 1]
  double* ring_pk = nullptr;           // [S nch][cap]
  double* ring_sp = nullptr;
  sdr_tpeak_record* st = nullptr;      // [S nch]
  GrowMem<TpRec> piece;                // the work array, grown to the largest call
  StageTimer<2> tm;                    // around the two launches of a call (sdr_tpeak_set_timing)
};

extern "C" {

int sdr_tpeak_create(sdr_ctx* c, int nstreams, int channels, const sdr_tpeak_params* params, sdr_tpeak** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_create: out is NULL");
  *out = nullptr;
  if (params == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_create: params is NULL");
  if (nstreams < 1 || nstreams > SDR_SOS_MAX_ROWS) return fail(SDR_EINVAL, "sdr_tpeak_create: nstreams=%d outside [1, %d]", nstreams, SDR_SOS_MAX_ROWS);
  if (channels != 1 && channels != 2) return fail(SDR_EINVAL, "sdr_tpeak_create: channels=%d is not 1 or 2", channels);
  int up = params->up, taps = params->taps;
  if (params->h == nullptr) {
    if (!((up == 4 && taps == 12) || (up == 0 && taps == 0)))
      return fail(SDR_EINVAL, "sdr_tpeak_create: up=%d, taps=%d without a table (h is NULL: 4 and 12, or both 0)", up, taps);
    up = 4;
    taps = 12;
  }
  if (up < 1 || up > SDR_TPEAK_MAX_UP) return fail(SDR_EINVAL, "sdr_tpeak_create: up=%d outside [1, %d]", up, SDR_TPEAK_MAX_UP);
  if (taps < 1 || taps > SDR_TPEAK_MAX_TAPS) return fail(SDR_EINVAL, "sdr_tpeak_create: taps=%d outside [1, %d]", taps, SDR_TPEAK_MAX_TAPS);
  std::vector<double> tab((size_t)up * taps);
  for (int p = 0; p < up; ++p)
    for (int k = 0; k < taps; ++k) {
      const int q = p < 2 ? p : 3 - p;
      const float v = params->h != nullptr ? params->h[p * taps + k] : (float)TP_BS1770[q][p < 2 ? k : 11 - k] / 8192.f;
      if (!std::isfinite(v)) return fail(SDR_EINVAL, "sdr_tpeak_create: h[%d][%d] is not finite", p, k);
      tab[(size_t)p * taps + k] = (double)v;
    }
  if (params->segment < SDR_LOUD_MIN_SEGMENT || params->segment > SDR_LOUD_MAX_SEGMENT)
    return fail(SDR_EINVAL, "sdr_tpeak_create: segment=%lld outside [%d, %d]", (long long)params->segment, SDR_LOUD_MIN_SEGMENT, SDR_LOUD_MAX_SEGMENT);
  if (params->cap < 4 || params->cap > SDR_LOUD_MAX_CAP) return fail(SDR_EINVAL, "sdr_tpeak_create: cap=%d outside [4, %d]", params->cap, SDR_LOUD_MAX_CAP);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_tpeak* t = new (std::nothrow) sdr_tpeak;
  if (t == nullptr) return fail(SDR_ENOMEM, "sdr_tpeak_create: out of host memory");
  t->ctx = c;
  t->S = nstreams;
  t->nch = channels;
  t->up = up;
  t->taps = taps;
  t->seg = params->segment;
  t->cap = params->cap;
  const size_t rows = (size_t)nstreams * channels;
  t->mem.get(&t->tab, tab.size());
  t->mem.get(&t->hist, rows * (size_t)std::max(taps - 1, 1), true);
  t->mem.get(&t->ring_pk, rows * (size_t)t->cap, true);
  t->mem.get(&t->ring_sp, rows * (size_t)t->cap, true);
  t->mem.get(&t->st, rows, true);
  hipError_t e = t->mem.err;
  if (e == hipSuccess) e = hipMemcpy(t->tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
  const int rc = e != hipSuccess ? create_failed(e, "sdr_tpeak_create") : sdr_tpeak_reset(t);
  if (rc != SDR_OK) {
    sdr_tpeak_destroy(t);
    return rc;
  }
  *out = t;
  return SDR_OK;
}

void sdr_tpeak_destroy(sdr_tpeak* t) {
  if (t == nullptr) return;
  if (t->ctx != nullptr && set_dev(t->ctx) == SDR_OK) (void)hipStreamSynchronize(t->ctx->stream);
  t->mem.release();
  t->piece.release();
  delete t;
}

// every maximum's identity is 0.0 and the history of a fresh stream is silence: zeros throughout
int sdr_tpeak_reset(sdr_tpeak* t) {
  if (t == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_reset: object is NULL");
  TRY(set_dev(t->ctx));
  HIP_TRY(t->mem.zero(t->ctx->stream));
  t->pos = 0;
  return SDR_OK;
}

int sdr_tpeak_process_dev(sdr_tpeak* t, const float* ch0, const float* ch1, int64_t stride, int64_t n) {
  if (t == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_process_dev: object is NULL");
  if (ch0 == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_process_dev: ch0 is NULL");
  if ((ch1 != nullptr) != (t->nch == 2)) return fail(SDR_EINVAL, "sdr_tpeak_process_dev: ch1 must be given with two channels and NULL with one");
  TRY(tp_check_rows("sdr_tpeak_process_dev", "ch0", ch0, stride, n));
  if (ch1 != nullptr) TRY(tp_check_rows("sdr_tpeak_process_dev", "ch1", ch1, stride, n));
  sdr_ctx* c = t->ctx;
  TRY(set_dev(c));
  // the cut of the call's samples at the segment boundaries, a segment in P pieces of L samples
  const int64_t seg = t->seg, pos0 = t->pos % seg, nseg = ceil_div(pos0 + n, seg);
  const int rows = t->S * t->nch;
  TpArgs a = {};
  a.x[0] = ch0;
  a.x[1] = ch1;
  a.hist = t->hist;
  a.tab = t->tab;
  a.n = n;
  a.stride = stride;
  a.seg = seg;
  a.pos0 = pos0;
  a.P = (int)ceil_div(seg, TP_CHUNK);
  a.L = ceil_div(seg, a.P);
  a.nch = t->nch;
  a.up = t->up;
  a.taps = t->taps;
  a.npiece = (int)(nseg * a.P);
  TRY(t->piece.fit((size_t)rows * a.npiece, c->stream, "sdr_tpeak_process_dev"));
  a.piece = t->piece.p;
  HIP_TRY(t->tm.mark(0, c->stream));
  const dim3 grid((unsigned)a.npiece, (unsigned)rows);
  if (t->up == 4 && t->taps == 12) hipLaunchKernelGGL((tpeak_reduce_kernel<4, 12>), grid, dim3(TP_T), 0, c->stream, a);
  else hipLaunchKernelGGL((tpeak_reduce_kernel<0, SDR_TPEAK_MAX_TAPS>), grid, dim3(TP_T), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(t->tm.mark(1, c->stream));
  const TpFold f{t->piece.p, t->ring_pk, t->ring_sp, t->st, t->hist, {ch0, ch1}, stride, n, seg, pos0, t->pos / seg, t->nch, a.P, a.npiece, t->cap, t->taps - 1};
  hipLaunchKernelGGL(tpeak_fold_kernel, dim3((unsigned)rows), dim3(64), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  HIP_TRY(t->tm.mark(2, c->stream));
  t->pos += n;
  return SDR_OK;
}

int sdr_tpeak_run(sdr_tpeak* t, const float* ch0_host, const float* ch1_host, int64_t stride, int64_t n) {
  if (t == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_run: object is NULL");
  if (ch0_host == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_run: ch0_host is NULL");
  if ((ch1_host != nullptr) != (t->nch == 2)) return fail(SDR_EINVAL, "sdr_tpeak_run: ch1_host must be given with two channels and NULL with one");
  TRY(tp_check_rows("sdr_tpeak_run", "ch0", nullptr, stride, n));
  sdr_ctx* c = t->ctx;
  TRY(set_dev(c));
  const size_t S = (size_t)t->S, rb = (size_t)n * 4;
  void *d0 = nullptr, *d1 = nullptr;
  TRY(scratch(c, S_IN, S * rb, &d0));
  HIP_TRY(hipMemcpy2DAsync(d0, rb, ch0_host, (size_t)stride * 4, rb, S, hipMemcpyHostToDevice, c->stream));
  if (ch1_host != nullptr) {
    TRY(scratch(c, S_IN2, S * rb, &d1));
    HIP_TRY(hipMemcpy2DAsync(d1, rb, ch1_host, (size_t)stride * 4, rb, S, hipMemcpyHostToDevice, c->stream));
  }
  TRY(sdr_tpeak_process_dev(t, (const float*)d0, (const float*)d1, n, n));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_tpeak_records(sdr_tpeak* t, sdr_tpeak_record* host) {
  if (t == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_records: NULL argument");
  return fetch(t->ctx, t->st, (size_t)t->S * t->nch, host);
}

int sdr_tpeak_segments(sdr_tpeak* t, double* peaks_host, double* sample_peaks_host, int64_t* first, int64_t* count) {
  if (t == nullptr || peaks_host == nullptr || sample_peaks_host == nullptr || first == nullptr || count == nullptr)
    return fail(SDR_EINVAL, "sdr_tpeak_segments: NULL argument");
  const size_t rows = (size_t)t->S * t->nch, cap = (size_t)t->cap;
  std::vector<double> ring(rows * cap);
  const int64_t done = t->pos / t->seg, cnt = std::min<int64_t>(done, (int64_t)cap);
  *first = done - cnt;
  *count = cnt;
  const double* dev[2] = {t->ring_pk, t->ring_sp};
  double* host[2] = {peaks_host, sample_peaks_host};
  for (int w = 0; w < 2; ++w) {
    TRY(fetch(t->ctx, dev[w], ring.size(), ring.data()));
    for (size_t r = 0; r < rows; ++r)
      for (int64_t i = 0; i < cnt; ++i) host[w][r * cap + i] = ring[r * cap + (size_t)((*first + i) % (int64_t)cap)];
  }
  return SDR_OK;
}

int sdr_tpeak_state_dev(sdr_tpeak* t, const double** peaks_dev, const double** sample_peaks_dev, const sdr_tpeak_record** records_dev) {
  if (t == nullptr || (peaks_dev == nullptr && sample_peaks_dev == nullptr && records_dev == nullptr))
    return fail(SDR_EINVAL, "sdr_tpeak_state_dev: NULL argument");
  if (peaks_dev != nullptr) *peaks_dev = t->ring_pk;
  if (sample_peaks_dev != nullptr) *sample_peaks_dev = t->ring_sp;
  if (records_dev != nullptr) *records_dev = t->st;
  return SDR_OK;
}

int sdr_tpeak_set_timing(sdr_tpeak* t, int on) {
  if (t == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_set_timing: object is NULL");
  TRY(set_dev(t->ctx));
  HIP_TRY(t->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_tpeak_stage_ms(sdr_tpeak* t, float* ms) {
  if (t == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_tpeak_stage_ms: NULL argument");
  return t->tm.elapsed(ms, "sdr_tpeak_stage_ms: no timed call (sdr_tpeak_set_timing)");
}

}  // extern "C"
