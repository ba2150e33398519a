// Wideband channelizer (multi-channel digital down-converter): one interleaved-IQ capture in,
// nch rows of interleaved complex f32 at Fs / D out, each centred on its own frequency
// (include/sdr.h sdr_ddc_*).  The reference has no channelizer; the definition is
//   y_c[m] = sum_j h[j] x[mD - j] exp(-i 2 pi phi_c(mD - j)),   phi_c(k) = ((inc_c k) mod 2^32) / 2^32
// ("mix down, lfilter(h, 1, .), [::D]") with an integer phase accumulator, computed in the
// frequency-translating form
//   y_c[m] = exp(-i 2 pi phi_c(mD)) sum_j g_c[j] x[mD - j],     g_c[j] = h[j] exp(+i 2 pi phi_c(j))
// as one dense GEMM Y = A X on the matrix cores, the interleaved IQ never de-interleaved: with
// xf[2k] = I_k, xf[2k + 1] = Q_k and K = 2T padded to 32 KS,
//   X[kap][n] = xf[2D (m0 + n) - 2 (T - 1) + kap]                      (columns 2D floats apart)
//   A_re[kap] = g_r[j] (kap even), -g_i[j] (odd);  A_im[kap] = g_i[j] (even), g_r[j] (odd);  j = T - 1 - kap / 2
// so a 16-row tile is 8 channels (row 2 c' = Re, 2 c' + 1 = Im), and lane l of a
// v_mfma_f32_16x16x32_f16 ends with both parts of channels 2 (l >> 4), 2 (l >> 4) + 1 at column
// l & 15: the rotation by the 32-bit phase of (absolute index) x inc_c and one 8-byte store.
// f32 accuracy from the hi / lo f16 split of sdr_mma.h (three MFMAs per K step; a u8 sample is
// exact in f16: no lo plane, two MFMAs).
//
// Work: a wave works alone and is persistent.  Its unit is a window of 16 CB outputs of ALL
// channels (CB = 4 column blocks; 1 where 2 D 63 + K floats do not fit the wave's LDS slice):
// it stages the window's 2 D (16 CB - 1) + 32 KS input floats once into its own LDS slice (f16
// hi and lo planes), then for every row tile and K step reads the tile's A fragment (pre-split
// in fragment order, 2 KB per step: from the workgroup's LDS copy where all of them fit beside
// the staging, ALDS; else from L2) and runs the CB column blocks.  So the input is read from HBM
// once, whatever nch is;
// neighbouring windows' 2 (T - 1) + pad floats of overlap come from L2.  The next window's loads
// are issued before this window's MFMAs.  Interior windows load 16 B (f32) / 4 B (u8) per lane
// from a descriptor that covers exactly the window; the windows that touch the call's first
// 2 (T - 1) floats or its end load complex samples one by one across the seam between the
// object's history (the T - 1 samples before the call) and the caller's buffer (sdr_stream.h), so
// the input is read in place and no access leaves either buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "sdr_ctx.h"
#include "sdr_mma.h"
#include "sdr_stream.h"

using namespace sdrint;

namespace {

constexpr int DDC_WAVES = 4;                       // per workgroup
constexpr int DDC_NQ_MAX = 15;                     // 4-element chunks per lane of a staged window
constexpr int DDC_LP_MAX = DDC_NQ_MAX * 256;       // staged elements per window (60 KB of LDS per workgroup in f32)
constexpr int DDC_INC_HALFS = SDR_DDC_MAX_CH * 2;   // the increments' place in LDS (a uint32 per channel), in halfs
constexpr int DDC_CB = 4;                          // column blocks per window (SDR_DDC_WINDOW = 16 DDC_CB)
static_assert(16 * DDC_CB == SDR_DDC_WINDOW, "the window the header names");
static_assert(DDC_WAVES * DDC_LP_MAX * 2 * sizeof(_Float16) + DDC_INC_HALFS * 2 <= 64 * 1024, "hi and lo planes of every wave in 64 KB of LDS");

typedef _Float16 h8a4 __attribute__((ext_vector_type(8), aligned(4)));   // a fragment at a 4-B aligned LDS address

struct DdcArgs {
  const void* iq;          // the call's n complex samples (f32 pairs or u8 pairs)
  const void* hist;        // the T - 1 complex samples before them, same type
  const _Float16* afrag;   // [NT KS][hi, lo][64 lanes][8]: the A fragments
  const uint32_t* inc;     // [8 NT]: the channels' phase increments (0 beyond nch)
  float* out;
  int64_t n2;              // input elements (2 n)
  int64_t M;               // outputs per channel (n / D)
  int64_t out_stride;      // complex samples between rows
  int64_t passes;          // windows of the call
  uint32_t pos_lo;         // the call's first sample's absolute index mod 2^32
  int nch, T, D, KS, NT, nq, lp;
  int a_lds;               // bytes of A fragments the workgroup keeps in LDS (0: read from afrag each K step)
};

template <int CB, bool U8, bool ALDS>
__global__ __launch_bounds__(64 * DDC_WAVES) void ddc_mma_kernel(const DdcArgs P) {
  extern __shared__ __attribute__((aligned(16))) _Float16 ddc_lds[];
  using VT = std::conditional_t<U8, uint32_t, u4v>;
  constexpr int ES = U8 ? 1 : 4;                    // bytes per element
  constexpr int W = 16 * CB;                        // outputs per window
  // the wave id, provably uniform (readfirstlane): everything derived from it is scalar
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int l = threadIdx.x & 63, b = l & 15, g = l >> 4;
  const int lp = P.lp, nq = P.nq, D = P.D, KS = P.KS;
  // the phase increments and the A fragments, once per workgroup (the only barrier: the waves
  // work alone after it).  Both are read from LDS in the window loop: a global load there makes
  // the compiler wait for every memory operation in flight -- the next window's loads and this
  // window's stores -- before each use, the counter being in order.
  uint32_t* inc_s = reinterpret_cast<uint32_t*>(ddc_lds);
  const _Float16* a_s = ddc_lds + DDC_INC_HALFS;
  for (int i = threadIdx.x; i < 8 * P.NT; i += 64 * DDC_WAVES) inc_s[i] = P.inc[i];
  for (int i = threadIdx.x; i < P.a_lds / 16; i += 64 * DDC_WAVES)
    reinterpret_cast<u4v*>(ddc_lds + DDC_INC_HALFS)[i] = reinterpret_cast<const u4v*>(P.afrag)[i];
  __syncthreads();
  _Float16* xh = ddc_lds + DDC_INC_HALFS + P.a_lds / 2 + (size_t)w * (U8 ? 1 : 2) * lp;
  _Float16* xl = xh + lp;                           // (f32 only)
  const int64_t gw = (int64_t)blockIdx.x * DDC_WAVES + w, nw = (int64_t)gridDim.x * DDC_WAVES;
  const int hl2 = 2 * (P.T - 1);                    // history elements
  const char* iqb = reinterpret_cast<const char*>(P.iq);

  // window p stages elements [e0, e0 + lp) of the stream (0 = the call's first element):
  // e0 = 2 D W p - 2 (T - 1) - sh, sh the elements (u8: 0 or 2) that make its address 4-B aligned
  auto origin = [&](int64_t p, int* sh) {
    const int64_t s0 = 2 * (int64_t)D * W * p - hl2;
    *sh = U8 ? (int)(((uintptr_t)P.iq + (uintptr_t)s0) & 3) : 0;
    return s0 - *sh;
  };
  auto load = [&](int64_t p, VT* v) {
    int sh;
    const int64_t e0 = origin(p, &sh);
    if (e0 >= 0 && e0 + lp <= P.n2) {               // interior (uniform): every chunk inside the caller's buffer
      const __amdgpu_buffer_rsrc_t r = mm_rsrc(iqb + e0 * ES, (int64_t)lp * ES);
#pragma unroll
      for (int j = 0; j < DDC_NQ_MAX; ++j)
        if (j < nq) {
          if constexpr (U8) v[j] = __builtin_amdgcn_raw_buffer_load_b32(r, 4 * (l + 64 * j), 0, 0);
          else v[j] = __builtin_amdgcn_raw_buffer_load_b128(r, 16 * (l + 64 * j), 0, 0);
        }
    } else {
      // the seam and the call's end: complex samples one by one, each from the history
      // (elements -hl2 .. -1) or the buffer (0 .. n2 - 1): the seam load of sdr_stream.h, in
      // element units
      const int64_t be = e0 > 0 ? e0 : 0;
      const int64_t left = P.n2 - be;
      const Seam<ES> seam{mm_rsrc(iqb + be * ES, (left < (1 << 22) ? left : (1 << 22)) * ES), mm_rsrc(P.hist, (int64_t)hl2 * ES),
                        (int)(e0 - be),                                 // <= 0
                        e0 > 0 ? (1 << 28) : (int)(e0 + hl2)};          // >= -2; past the seam: outside the history's range
#pragma unroll
      for (int j = 0; j < DDC_NQ_MAX; ++j)
        if (j < nq) {
          const int c = 4 * (l + 64 * j);
          if constexpr (U8) {
            const uint32_t a0 = seam.template load<2>(c), a1 = seam.template load<2, 2>(c);
            v[j] = (a0 & 0xffffu) | (a1 << 16);
          } else {
            const u2v a0 = seam.template load<8>(c), a1 = seam.template load<8, 2>(c);
            v[j] = u4v{a0.x, a0.y, a1.x, a1.y};
          }
        }
    }
  };

  VT v[DDC_NQ_MAX];
  if (gw < P.passes) load(gw, v);
  for (int64_t p = gw; p < P.passes; p += nw) {
    // stage: the wave's own LDS slice (its previous window's fragment reads retired in order)
#pragma unroll
    for (int j = 0; j < DDC_NQ_MAX; ++j)
      if (j < nq) {
        const int q = l + 64 * j;
        if constexpr (U8) {
          const uint32_t u = v[j];
          h4v hv;
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[e] = (_Float16)(((float)((u >> (8 * e)) & 255u) - 128.f) * (1.f / 128.f));
          *reinterpret_cast<h4v*>(xh + 4 * q) = hv;
        } else {
          h4v hv, lv;
          mm_split4(__builtin_bit_cast(float4, v[j]), &hv, &lv);
          *reinterpret_cast<h4v*>(xh + 4 * q) = hv;
          *reinterpret_cast<h4v*>(xl + 4 * q) = lv;
        }
      }
    if (p + nw < P.passes) load(p + nw, v);         // in flight while this window's MFMAs run
    int sh;
    (void)origin(p, &sh);
    const int64_t m0 = p * W;
    const int ub = sh + 2 * D * b + 8 * g;          // this lane's fragment origin in column block 0
    for (int t = 0; t < P.NT; ++t) {
      f4v acc_h[CB], acc_c[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) acc_h[cb] = acc_c[cb] = f4v{0.f, 0.f, 0.f, 0.f};
      for (int st = 0; st < KS; ++st) {
        // from LDS: the next window's loads stay in flight (a global load here would wait for
        // them first, the counter being in order)
        const int ao = (t * KS + st) * 1024 + 8 * l;
        h8v ah, al;
        if constexpr (ALDS) {                      // (compile time: the other path's loads must not be in this code)
          ah = *reinterpret_cast<const h8v*>(a_s + ao);
          al = *reinterpret_cast<const h8v*>(a_s + ao + 512);
        } else {
          ah = *reinterpret_cast<const h8v*>(P.afrag + ao);
          al = *reinterpret_cast<const h8v*>(P.afrag + ao + 512);
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const int u = ub + 32 * D * cb + 32 * st;
          const h8v bh = *reinterpret_cast<const h8a4*>(xh + u);
          acc_h[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc_h[cb], 0, 0, 0);
          if constexpr (!U8) {
            const h8v bl = *reinterpret_cast<const h8a4*>(xl + u);
            acc_c[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc_c[cb], 0, 0, 0);
          }
          acc_c[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc_c[cb], 0, 0, 0);
        }
      }
      // rows 4 g + 0..3 of the tile at column b: channels 8 t + 2 g (+ 1), Re and Im
      const int c0 = 8 * t + 2 * g;
      const uint32_t inc0 = inc_s[c0], inc1 = inc_s[c0 + 1];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int64_t m = m0 + 16 * cb + b;
        if (m < P.M) {
          const uint32_t k = P.pos_lo + (uint32_t)m * (uint32_t)D;   // the absolute index mod 2^32
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int c = c0 + h;
            if (c < P.nch) {
              const float re = fmaf(acc_c[cb][2 * h], 1.f / MM_LO, acc_h[cb][2 * h]);
              const float im = fmaf(acc_c[cb][2 * h + 1], 1.f / MM_LO, acc_h[cb][2 * h + 1]);
              // the phase as signed turns (24 bits of it survive the f32), in half turns for sincospi
              const float ht = (float)(int32_t)((h ? inc1 : inc0) * k) * 0x1p-31f;
              float sn, cs;
              sincospif(ht, &sn, &cs);
              float2 o;
              o.x = fmaf(im, sn, re * cs);
              o.y = fmaf(-re, sn, im * cs);
              *reinterpret_cast<float2*>(P.out + 2 * ((int64_t)c * P.out_stride + m)) = o;
            }
          }
        }
      }
    }
  }
}

// staged elements of a CB-block window: the alignment shift, the columns, the K steps
int ddc_nq(int D, int KS, int CB) { return (2 + 2 * D * (16 * CB - 1) + 32 * KS + 255) / 256; }

}  // namespace

struct sdr_ddc {
  sdr_ctx* ctx = nullptr;
  int nch = 0, T = 0, D = 0, dtype = 0, KS = 0, NT = 0, CB = 0, nq = 0;
  std::vector<uint32_t> inc;
  _Float16* afrag = nullptr;
  uint32_t* dinc = nullptr;
  StreamHist hist;                      // the T - 1 samples before the next call
  int64_t pos = 0;
};

extern "C" {

int sdr_ddc_create(sdr_ctx* c, int nch, const double* freq, const double* b, int taps, int decim, int iq_dtype,
                   sdr_ddc** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_ddc_create: out is NULL");
  *out = nullptr;
  if (nch < 1 || nch > SDR_DDC_MAX_CH) return fail(SDR_EINVAL, "sdr_ddc_create: nch=%d outside [1, %d]", nch, SDR_DDC_MAX_CH);
  if (taps < 1 || taps > SDR_DDC_MAX_TAPS)
    return fail(SDR_EINVAL, "sdr_ddc_create: taps=%d outside [1, %d]", taps, SDR_DDC_MAX_TAPS);
  if (decim < 1 || decim > SDR_DDC_MAX_DECIM)
    return fail(SDR_EINVAL, "sdr_ddc_create: decim=%d outside [1, %d]", decim, SDR_DDC_MAX_DECIM);
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8) return fail(SDR_EINVAL, "sdr_ddc_create: bad iq_dtype %d", iq_dtype);
  if (freq == nullptr || b == nullptr) return fail(SDR_EINVAL, "sdr_ddc_create: freq or taps pointer is NULL");
  TRY(taps_finite(b, taps, "sdr_ddc_create"));
  for (int ch = 0; ch < nch; ++ch)
    if (!std::isfinite(freq[ch]) || std::fabs(freq[ch]) > 0.5)
      return fail(SDR_EINVAL, "sdr_ddc_create: freq[%d]=%g is not a finite value in [-0.5, 0.5] cycles/sample", ch, freq[ch]);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_ddc* d = new (std::nothrow) sdr_ddc;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_ddc_create: out of host memory");
  d->ctx = c;
  d->nch = nch;
  d->T = taps;
  d->D = decim;
  d->dtype = iq_dtype;
  d->KS = (2 * taps + 31) / 32;
  d->NT = (nch + 7) / 8;
  d->CB = ddc_nq(decim, d->KS, DDC_CB) <= DDC_NQ_MAX ? DDC_CB : 1;
  d->nq = ddc_nq(decim, d->KS, d->CB);
  const int Kp = 32 * d->KS, rows = 16 * d->NT;
  // inc = rint(nu 2^32) mod 2^32; the complex taps g_c[j] = h[j] exp(+i 2 pi phi_c(j)) in f64
  d->inc.assign(8 * d->NT, 0u);
  std::vector<float> A((size_t)rows * Kp, 0.f);
  for (int ch = 0; ch < nch; ++ch) {
    const uint32_t inc = (uint32_t)(uint64_t)(int64_t)std::nearbyint(freq[ch] * 4294967296.0);
    d->inc[ch] = inc;
    float* are = A.data() + (size_t)(2 * ch) * Kp;   // row 16 t + 2 c' = 2 ch
    float* aim = are + Kp;
    for (int j = 0; j < taps; ++j) {
      const double ph = two_pi * ((double)(uint32_t)(inc * (uint32_t)j) / 4294967296.0);
      const double gr = b[j] * std::cos(ph), gi = b[j] * std::sin(ph);
      const int k = 2 * (taps - 1 - j);
      are[k] = (float)gr;
      are[k + 1] = (float)-gi;
      aim[k] = (float)gi;
      aim[k + 1] = (float)gr;
    }
  }
  const bool u8 = iq_dtype == SDR_IQ_U8;
  float* dA = nullptr;
  hipError_t e = upload(&dA, A.data(), A.size(), c->stream);
  if (e == hipSuccess) e = upload(&d->dinc, d->inc.data(), d->inc.size(), c->stream);
  if (e == hipSuccess) e = hipMalloc(&d->afrag, (size_t)d->NT * d->KS * 2 * 512 * sizeof(_Float16));
  if (e == hipSuccess) e = mm_prep(dA, d->afrag, d->NT, d->KS, c->stream);
  if (e == hipSuccess) e = d->hist.alloc((size_t)2 * (taps - 1) * (u8 ? 1 : 4), u8 ? 128 : 0, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host vectors are read until here)
  (void)hipFree(dA);
  if (e != hipSuccess) {
    sdr_ddc_destroy(d);
    return create_failed(e, "sdr_ddc_create");
  }
  *out = d;
  return SDR_OK;
}

void sdr_ddc_destroy(sdr_ddc* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  (void)hipFree(d->afrag);
  (void)hipFree(d->dinc);
  d->hist.free();
  delete d;
}

int sdr_ddc_freq(sdr_ddc* d, double* actual) {
  if (d == nullptr || actual == nullptr) return fail(SDR_EINVAL, "sdr_ddc_freq: NULL argument");
  for (int ch = 0; ch < d->nch; ++ch) actual[ch] = (double)(int32_t)d->inc[ch] / 4294967296.0;
  return SDR_OK;
}

int sdr_ddc_reset(sdr_ddc* d, int64_t position) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_ddc_reset: object is NULL");
  if (position < 0 || position % d->D != 0)
    return fail(SDR_EINVAL, "sdr_ddc_reset: position=%lld must be >= 0 and a multiple of decim=%d", (long long)position, d->D);
  TRY(set_dev(d->ctx));
  HIP_TRY(d->hist.reset(d->ctx->stream));
  d->pos = position;
  return SDR_OK;
}

int sdr_ddc_position(sdr_ddc* d, int64_t* position) {
  if (d == nullptr || position == nullptr) return fail(SDR_EINVAL, "sdr_ddc_position: NULL argument");
  *position = d->pos;
  return SDR_OK;
}

int sdr_ddc_process_dev(sdr_ddc* d, const void* iq, int64_t n, float* out, int64_t out_stride) {
  TRY(decim_check_call(d, iq, n, out, out_stride, "sdr_ddc_process_dev"));
  const bool u8 = d->dtype == SDR_IQ_U8;
  if (((uintptr_t)iq & (u8 ? 1 : 7)) != 0 || ((uintptr_t)out & 7) != 0)
    return fail(SDR_EINVAL, "sdr_ddc_process_dev: iq must be aligned to one complex sample (%d B) and out to 8 B", u8 ? 2 : 8);
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  DdcArgs P;
  P.iq = iq;
  P.hist = d->hist.current();
  P.afrag = d->afrag;
  P.inc = d->dinc;
  P.out = out;
  P.n2 = 2 * n;
  P.M = n / d->D;
  P.out_stride = out_stride;
  const int W = 16 * d->CB;
  P.passes = ceil_div(P.M, W);
  P.pos_lo = (uint32_t)(uint64_t)d->pos;
  P.nch = d->nch;
  P.T = d->T;
  P.D = d->D;
  P.KS = d->KS;
  P.NT = d->NT;
  P.nq = d->nq;
  P.lp = d->nq * 256;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(P.passes, DDC_WAVES), 2048);
  const size_t stage = (size_t)DDC_WAVES * P.lp * (u8 ? 1 : 2) * sizeof(_Float16);
  const size_t abytes = (size_t)d->NT * d->KS * 2048;
  const size_t incb = DDC_INC_HALFS * sizeof(_Float16);
  P.a_lds = incb + stage + abytes <= 64 * 1024 ? (int)abytes : 0;
  const size_t lds = incb + stage + P.a_lds;
  const dim3 blk(64 * DDC_WAVES);
#define DDC_LAUNCH(CBV, U8V)                                                                    \
  do {                                                                                          \
    if (P.a_lds != 0) ddc_mma_kernel<CBV, U8V, true><<<blocks, blk, lds, c->stream>>>(P);       \
    else ddc_mma_kernel<CBV, U8V, false><<<blocks, blk, lds, c->stream>>>(P);                   \
  } while (0)
  if (d->CB == DDC_CB) {
    if (u8) DDC_LAUNCH(DDC_CB, true);
    else DDC_LAUNCH(DDC_CB, false);
  } else {
    if (u8) DDC_LAUNCH(1, true);
    else DDC_LAUNCH(1, false);
  }
#undef DDC_LAUNCH
  HIP_TRY(hipGetLastError());
  if (u8) HIP_TRY(d->hist.advance<uint16_t>(c->stream, iq, n, 0, 1, d->T - 1));
  else HIP_TRY(d->hist.advance<float2>(c->stream, iq, n, 0, 1, d->T - 1));
  d->pos += n;
  return SDR_OK;
}

int sdr_ddc_run(sdr_ddc* d, const void* iq_host, int64_t n, float* out_host, int64_t out_stride) {
  TRY(decim_check_call(d, iq_host, n, out_host, out_stride, "sdr_ddc_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const size_t es = d->dtype == SDR_IQ_U8 ? 2 : 8, M = (size_t)(n / d->D);
  return run_staged(c, iq_host, {1, (size_t)n * es, 0}, out_host, {(size_t)d->nch, M * 8, (size_t)out_stride * 8},
                    [&](void* din, void* dout) { return sdr_ddc_process_dev(d, din, n, (float*)dout, (int64_t)M); });
}

}  // extern "C"
