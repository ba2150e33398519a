// Polyphase filter bank (include/sdr.h sdr_pfb_*): one interleaved-IQ capture in, nch rows of
// interleaved complex f32 at Fs / D out, row c centred on bin_c / M cycles per sample of a uniform
// grid of M bins.  The definition, with T real prototype taps h and k the absolute sample index,
//   y_c[m] = sum_j h[j] x[mD - j] exp(-2 pi i ((bin_c (k mod M)) mod M) / M),   k = pos + mD - j
// is computed in the polyphase form (P = ceil(T / M), h zero-padded to P M)
//   u_m[p] = sum_{q < P} h[p + q M] x[mD - p - q M]                                  (the fold)
//   y_c[m] = exp(-2 pi i (bin_c ((pos + mD) mod M) mod M) / M) sum_{p < M} exp(+2 pi i (bin_c p mod M) / M) u_m[p]
// so the filter's MACs are shared by all channels (T real-by-complex MACs per output time) and
// only the M-point DFT is per channel: a dense GEMM Y = A U on the matrix cores for the selected
// bins, A two rows (Re, Im) per channel over K = 2M (u's Re, Im interleaved) padded to 32 KS,
//   A_re[2p] = cos th, A_re[2p + 1] = -sin th;  A_im[2p] = sin th, A_im[2p + 1] = cos th;  th = 2 pi (bin_c p mod M) / M
// with ddc.hip's row order: a 16-row tile is 8 channels, and lane l of a v_mfma_f32_16x16x32_f16
// ends with both parts of channels 2 (l >> 4), 2 (l >> 4) + 1 at column l & 15.  f32 accuracy
// from the hi / lo f16 split of sdr_mma.h, three MFMAs per K step (the fold's output is not exact
// in f16, so a u8 capture takes the same three).
//
// Work: a workgroup of 4 waves is persistent and owns windows of W = 16 CB output times (CB = 4;
// 1 where the window's buffers take more than half a compute unit's LDS).  Per window:
//   stage  the (W - 1) D + P M complex inputs into LDS as f32 pairs, one buffer load each -- the
//          input is read from HBM once per call, whatever nch is.  Windows that reach below the
//          call's first sample read across the seam to the object's history (the T - 1 samples
//          before the call; sdr_stream.h); no access leaves either buffer;
//   fold   in f32 on the vector units: a thread runs the FMA chain over q for four (n, p) pairs
//          at a time, the taps and the samples from LDS, and writes u as f16 hi / lo planes, one
//          row of 32 KS (+ 8) halfs per output time -- u never goes to HBM;
//   GEMM   wave w takes the row tiles t = w, w + 4, ...: per K step the tile's A fragment
//          (pre-split in fragment order, 2 KB per step: from the workgroup's LDS copy where it
//          fits beside the rest in 64 KB, ALDS; else from L2, as its own instantiation, two K
//          steps requested ahead of the two being multiplied) against the CB column blocks of
//          u, then the rotation -- the M-entry table exp(-2 pi i t / M) in LDS, t = (bin_c s)
//          mod M in integers -- and one 8-byte store per channel and output.
// Two barriers per window (after stage, after fold): a wave that has finished its row tiles
// stages the next window while the others still multiply.  The grid is the workgroups the
// device holds at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "sdr_ctx.h"
#include "sdr_launch.h"
#include "sdr_mma.h"
#include "sdr_stream.h"

using namespace sdrint;

namespace {

constexpr int PFB_WAVES = 4;                       // per workgroup (8 measured: -5 % at 64 bins, +1..3 % at 96)
constexpr int PFB_THREADS = 64 * PFB_WAVES;
constexpr int PFB_CB = 4;                          // column blocks per window (SDR_PFB_WINDOW = 16 PFB_CB)
constexpr size_t PFB_LDS_ALDS = 64 * 1024;         // A fragments stay in LDS while everything fits this
constexpr size_t PFB_LDS_WINDOW = 80 * 1024;       // the full window while its buffers fit this: two workgroups per CU
constexpr size_t PFB_LDS_MAX = 160 * 1024;         // LDS of a gfx950 compute unit
static_assert(16 * PFB_CB == SDR_PFB_WINDOW, "the window the header names");

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// the LDS of a launch, in bytes from its start (all multiples of 16)
struct PfbLayout {
  size_t rot, bin, taps, xs, uh, ul, a, total;
};

PfbLayout pfb_layout(int M, int NT, int PM, int D, int KS, int CB, size_t abytes) {
  const int W = 16 * CB, US = 32 * KS + 8;
  PfbLayout o;
  o.rot = 0;
  o.bin = o.rot + up16((size_t)M * sizeof(float2));
  o.taps = o.bin + up16((size_t)8 * NT * sizeof(int));
  o.xs = o.taps + up16((size_t)PM * sizeof(float));
  o.uh = o.xs + up16(((size_t)(W - 1) * D + PM) * sizeof(float2));
  o.ul = o.uh + (size_t)W * US * sizeof(_Float16);
  o.a = o.ul + (size_t)W * US * sizeof(_Float16);
  o.total = o.a + abytes;
  return o;
}

struct PfbArgs {
  const void* iq;          // the call's n complex samples (f32 pairs or u8 pairs)
  const void* hist;        // the T - 1 complex samples before them, same type
  const float* taps;       // [P M]: the prototype, zero-padded
  const _Float16* afrag;   // [NT KS][hi, lo][64 lanes][8]: the DFT rows' fragments
  const float2* rot;       // [M]: exp(-2 pi i t / M)
  const int* bin;          // [8 NT]: the channels' bins (0 beyond nch)
  float* out;
  int64_t n;               // input samples
  int64_t Mo;              // outputs per channel (n / D)
  int64_t out_stride;      // complex samples between rows
  int64_t passes;          // windows of the call
  int s0;                  // the call's first sample's absolute index mod M
  int nch, M, T, D, PM, KS, NT, L;
  int o_bin, o_taps, o_xs, o_uh, o_ul, o_a;   // LDS offsets in bytes
  int a_lds;               // bytes of A fragments the workgroup keeps in LDS
  float invM;
};

// v mod M (and v / M) for 0 <= v < 2^24: v is exact in f32 and the quotient estimate is off by
// one at most
static __device__ __forceinline__ int pfb_divmod(int v, int M, float invM, int* quot) {
  int q = (int)((float)v * invM);
  int r = v - q * M;
  q -= r < 0 ? 1 : 0;
  r += r < 0 ? M : 0;
  q += r >= M ? 1 : 0;
  r -= r >= M ? M : 0;
  *quot = q;
  return r;
}
static __device__ __forceinline__ int pfb_mod(int v, int M, float invM) {
  int q;
  return pfb_divmod(v, M, invM, &q);
}

template <int CB, bool U8, bool ALDS>
__global__ __launch_bounds__(PFB_THREADS) void pfb_mma_kernel(const PfbArgs P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pfb_lds[];
  constexpr int ES = U8 ? 2 : 8;                    // bytes per complex sample
  constexpr int W = 16 * CB;                        // outputs per window
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63, b = l & 15, g = l >> 4;
  const int M = P.M, D = P.D, PM = P.PM, KS = P.KS, L = P.L, US = 32 * KS + 8;
  const float invM = P.invM;
  float2* rot_s = reinterpret_cast<float2*>(pfb_lds);
  int* bin_s = reinterpret_cast<int*>(pfb_lds + P.o_bin);
  float* h_s = reinterpret_cast<float*>(pfb_lds + P.o_taps);
  float2* x_s = reinterpret_cast<float2*>(pfb_lds + P.o_xs);
  _Float16* uh = reinterpret_cast<_Float16*>(pfb_lds + P.o_uh);
  _Float16* ul = reinterpret_cast<_Float16*>(pfb_lds + P.o_ul);
  const _Float16* a_s = reinterpret_cast<const _Float16*>(pfb_lds + P.o_a);

  // once per workgroup: the tables, the taps, the A fragments; u zeroed (its K padding stays 0)
  for (int i = tid; i < M; i += PFB_THREADS) rot_s[i] = P.rot[i];
  for (int i = tid; i < 8 * P.NT; i += PFB_THREADS) bin_s[i] = P.bin[i];
  for (int i = tid; i < PM; i += PFB_THREADS) h_s[i] = P.taps[i];
  for (int i = tid; i < W * US / 2; i += PFB_THREADS) reinterpret_cast<uint32_t*>(uh)[i] = reinterpret_cast<uint32_t*>(ul)[i] = 0u;
  if constexpr (ALDS)
    for (int i = tid; i < P.a_lds / 16; i += PFB_THREADS)
      reinterpret_cast<u4v*>(pfb_lds + P.o_a)[i] = reinterpret_cast<const u4v*>(P.afrag)[i];

  const int hl = P.T - 1;                           // history samples
  const char* iqb = reinterpret_cast<const char*>(P.iq);
  // (pos + m0 D) mod M of this workgroup's window, stepped from window to window
  int sm = (int)(((uint32_t)P.s0 + (uint32_t)blockIdx.x * (uint32_t)(W * D)) % (uint32_t)M);
  const int sstep = (int)(((uint32_t)gridDim.x * (uint32_t)(W * D)) % (uint32_t)M);

  const int qs = PFB_THREADS / M, rs = PFB_THREADS - qs * M;   // the fold's stride PFB_THREADS = qs M + rs
  // A from L2: K steps st, st + 1 of row tile t (the second clamped to the tile's last: then unused)
  [[maybe_unused]] auto load_a = [&](int t, int st, h8v* f) {
    const _Float16* a0 = P.afrag + ((size_t)(t * KS + st) * 1024 + 8 * l);
    const _Float16* a1 = P.afrag + ((size_t)(t * KS + (st + 1 < KS ? st + 1 : st)) * 1024 + 8 * l);
    f[0] = *reinterpret_cast<const h8v*>(a0);
    f[1] = *reinterpret_cast<const h8v*>(a0 + 512);
    f[2] = *reinterpret_cast<const h8v*>(a1);
    f[3] = *reinterpret_cast<const h8v*>(a1 + 512);
  };
  [[maybe_unused]] auto next_chunk = [&](int& t, int& st) {
    st += 2;
    if (st >= KS) {
      st = 0;
      t += PFB_WAVES;
    }
  };

  for (int64_t p = blockIdx.x; p < P.passes; p += gridDim.x) {
    // ---- stage: x_s[i] = sample sb + i of the call (0 = its first), sb = m0 D - (P M - 1): the
    // seam load of sdr_stream.h, in samples
    const int64_t m0 = p * W;
    const int64_t sb = m0 * D - (PM - 1);
    const int64_t be = sb > 0 ? sb : 0;
    const int64_t left = P.n - be;                  // >= 1: m0 D < n
    Seam<ES> seam;
    seam.in = mm_rsrc(iqb + be * ES, (left < L ? left : L) * ES);
    seam.d0 = (int)(sb - be);                         // <= 0
    auto conv = [](uint32_t v) {
      return float2{((float)(v & 255u) - 128.f) * (1.f / 128.f), ((float)((v >> 8) & 255u) - 128.f) * (1.f / 128.f)};
    };
    if (sb < 0 && hl > 0) {                         // (uniform) the window reaches into the history
      seam.hist = mm_rsrc(P.hist, (int64_t)hl * ES);
      seam.h0 = (int)(sb + hl);                       // the history's index of x_s[0]; below 0 where P M > T
      for (int i = tid; i < L; i += PFB_THREADS) {
        if constexpr (U8) x_s[i] = conv(seam.template load<ES>(i) & 0xffffu);
        else x_s[i] = __builtin_bit_cast(float2, seam.template load<ES>(i));
      }
    } else {
#pragma unroll 4
      for (int i = tid; i < L; i += PFB_THREADS) {
        if constexpr (U8) x_s[i] = conv(seam.template load_in<ES>(i) & 0xffffu);
        else x_s[i] = __builtin_bit_cast(float2, seam.template load_in<ES>(i));
      }
    }
    __syncthreads();                                // x_s complete; every wave is done with the previous u

    // (A from L2: this wave's first two K steps, in flight during the fold)
    [[maybe_unused]] h8v fa[4], fb[4];
    [[maybe_unused]] int tl = w, sl = 0;             // the row tile and K step the next fragment load takes
    if constexpr (!ALDS) {
      if (tl < P.NT) {
        load_a(tl, sl, fa);
        next_chunk(tl, sl);
      }
    }

    // ---- fold: u[n][p] = sum_q h[p + q M] x[(m0 + n) D - p - q M], f32 FMA chain over q; four
    // (n, p) pairs per thread at a time, PFB_THREADS apart in n M + p, so that eight LDS reads
    // are in flight per step of q
    for (int base = tid; base < W * M; base += 4 * PFB_THREADS) {
      int n0;
      int p0 = pfb_divmod(base, M, invM, &n0);
      int pp[4], xo[4], uo[4];
      bool ok[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = n0 < W;
        const int nc = ok[r] ? n0 : W - 1;          // (beyond the window: computed on valid memory, not stored)
        pp[r] = p0;
        xo[r] = nc * D + (PM - 1) - p0;
        uo[r] = nc * US + 2 * p0;
        p0 += rs;
        n0 += qs;
        if (p0 >= M) {
          p0 -= M;
          ++n0;
        }
      }
      float ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < PM; q += M) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float h = h_s[pp[r] + q];
          const float2 x = x_s[xo[r] - q];
          ar[r] = fmaf(h, x.x, ar[r]);
          ai[r] = fmaf(h, x.y, ai[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        h4v hv, lv;
        mm_split4(float4{ar[r], ai[r], ar[r + 1], ai[r + 1]}, &hv, &lv);
        if (ok[r]) {
          *reinterpret_cast<h2v*>(uh + uo[r]) = h2v{hv.x, hv.y};
          *reinterpret_cast<h2v*>(ul + uo[r]) = h2v{lv.x, lv.y};
        }
        if (ok[r + 1]) {
          *reinterpret_cast<h2v*>(uh + uo[r + 1]) = h2v{hv.z, hv.w};
          *reinterpret_cast<h2v*>(ul + uo[r + 1]) = h2v{lv.z, lv.w};
        }
      }
    }
    __syncthreads();                                // u complete

    // ---- GEMM + rotation + stores: this wave's row tiles against every column block
    f4v acc_h[CB], acc_c[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc_h[cb] = acc_c[cb] = f4v{0.f, 0.f, 0.f, 0.f};
    // one K step: the A fragment against the CB column blocks of u
    auto kstep = [&](const h8v ah, const h8v al, int st) {
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int u = (16 * cb + b) * US + 32 * st + 8 * g;
        const h8v bh = *reinterpret_cast<const h8v*>(uh + u);
        const h8v bl = *reinterpret_cast<const h8v*>(ul + u);
        acc_h[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc_h[cb], 0, 0, 0);
        acc_c[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc_c[cb], 0, 0, 0);
        acc_c[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc_c[cb], 0, 0, 0);
      }
    };
    // the end of row tile t: rows 4 g + 0..3 at column b are channels 8 t + 2 g (+ 1), Re and
    // Im; rotate, store, clear the accumulators
    auto finish = [&](int t) {
      const int c0 = 8 * t + 2 * g;
      const int bin0 = bin_s[c0], bin1 = bin_s[c0 + 1];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int64_t m = m0 + 16 * cb + b;
        if (m < P.Mo) {
          const int s = pfb_mod(sm + (16 * cb + b) * D, M, invM);   // (pos + m D) mod M
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int c = c0 + h;
            if (c < P.nch) {
              const float re = fmaf(acc_c[cb][2 * h], 1.f / MM_LO, acc_h[cb][2 * h]);
              const float im = fmaf(acc_c[cb][2 * h + 1], 1.f / MM_LO, acc_h[cb][2 * h + 1]);
              const float2 r = rot_s[pfb_mod((h ? bin1 : bin0) * s, M, invM)];
              float2 o;
              o.x = fmaf(-im, r.y, re * r.x);
              o.y = fmaf(re, r.y, im * r.x);
              *reinterpret_cast<float2*>(P.out + 2 * ((int64_t)c * P.out_stride + m)) = o;
            }
          }
        }
        acc_h[cb] = acc_c[cb] = f4v{0.f, 0.f, 0.f, 0.f};
      }
    };
    if constexpr (ALDS) {
      for (int t = w; t < P.NT; t += PFB_WAVES) {
        for (int st = 0; st < KS; ++st) {
          const int ao = (t * KS + st) * 1024 + 8 * l;
          kstep(*reinterpret_cast<const h8v*>(a_s + ao), *reinterpret_cast<const h8v*>(a_s + ao + 512), st);
        }
        finish(t);
      }
    } else {
      // (compile time: these loads must not be in the other path's code.)  Two K steps per
      // chunk, two register sets: the next chunk's fragments are requested before this
      // chunk's MFMAs, across the row tiles' ends too, so that one L2 round trip is hidden
      // behind each chunk and none waits for the stores in between
      auto chunk = [&](const h8v* f, int& t, int& st) {
        kstep(f[0], f[1], st);
        if (st + 1 < KS) kstep(f[2], f[3], st + 1);
        st += 2;
        if (st >= KS) {
          finish(t);
          st = 0;
          t += PFB_WAVES;
        }
      };
      int t = w, st = 0;
      while (t < P.NT) {
        if (tl < P.NT) {
          load_a(tl, sl, fb);
          next_chunk(tl, sl);
        }
        chunk(fa, t, st);
        if (t >= P.NT) break;
        if (tl < P.NT) {
          load_a(tl, sl, fa);
          next_chunk(tl, sl);
        }
        chunk(fb, t, st);
      }
    }
    sm += sstep;
    sm -= sm >= M ? M : 0;
  }
}

}  // namespace

struct sdr_pfb {
  sdr_ctx* ctx = nullptr;
  int M = 0, nch = 0, T = 0, D = 0, dtype = 0, KS = 0, NT = 0, PM = 0, CB = 0;
  size_t abytes = 0;
  float* taps = nullptr;
  _Float16* afrag = nullptr;
  float2* rot = nullptr;
  int* dbin = nullptr;
  StreamHist hist;                      // the T - 1 samples before the next call
  int64_t pos = 0;
  int grid = 0;                         // resident workgroups of its launch (from the first call on)
};

extern "C" {

int sdr_pfb_create(sdr_ctx* c, int nbins, int nch, const int* bin, const double* b, int taps, int decim, int iq_dtype,
                   sdr_pfb** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_pfb_create: out is NULL");
  *out = nullptr;
  if (nbins < 1 || nbins > SDR_PFB_MAX_BINS)
    return fail(SDR_EINVAL, "sdr_pfb_create: nbins=%d outside [1, %d]", nbins, SDR_PFB_MAX_BINS);
  if (nch < 1 || nch > SDR_PFB_MAX_CH) return fail(SDR_EINVAL, "sdr_pfb_create: nch=%d outside [1, %d]", nch, SDR_PFB_MAX_CH);
  if (taps < 1 || taps > SDR_PFB_MAX_TAPS)
    return fail(SDR_EINVAL, "sdr_pfb_create: taps=%d outside [1, %d]", taps, SDR_PFB_MAX_TAPS);
  if (decim < 1 || decim > SDR_PFB_MAX_DECIM)
    return fail(SDR_EINVAL, "sdr_pfb_create: decim=%d outside [1, %d]", decim, SDR_PFB_MAX_DECIM);
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8) return fail(SDR_EINVAL, "sdr_pfb_create: bad iq_dtype %d", iq_dtype);
  if (bin == nullptr || b == nullptr) return fail(SDR_EINVAL, "sdr_pfb_create: bin or taps pointer is NULL");
  TRY(taps_finite(b, taps, "sdr_pfb_create"));
  for (int ch = 0; ch < nch; ++ch)
    if (bin[ch] < 0 || bin[ch] >= nbins)
      return fail(SDR_EINVAL, "sdr_pfb_create: bin[%d]=%d outside [0, nbins=%d)", ch, bin[ch], nbins);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_pfb* d = new (std::nothrow) sdr_pfb;
  if (d == nullptr) return fail(SDR_ENOMEM, "sdr_pfb_create: out of host memory");
  const int M = nbins;
  d->ctx = c;
  d->M = M;
  d->nch = nch;
  d->T = taps;
  d->D = decim;
  d->dtype = iq_dtype;
  d->KS = (2 * M + 31) / 32;
  d->NT = (nch + 7) / 8;
  d->PM = (taps + M - 1) / M * M;
  d->abytes = (size_t)d->NT * d->KS * 2048;
  // the full window where its buffers fit the LDS without the A fragments, else one column block
  d->CB = pfb_layout(M, d->NT, d->PM, decim, d->KS, PFB_CB, 0).total <= PFB_LDS_WINDOW ? PFB_CB : 1;
  const int Kp = 32 * d->KS, rows = 16 * d->NT;
  // the DFT rows exp(+2 pi i (bin p mod M) / M) and the rotations exp(-2 pi i t / M), in f64
  std::vector<float> A((size_t)rows * Kp, 0.f);
  for (int ch = 0; ch < nch; ++ch) {
    float* are = A.data() + (size_t)(2 * ch) * Kp;   // row 16 t + 2 c' = 2 ch
    float* aim = are + Kp;
    for (int p = 0; p < M; ++p) {
      const double th = two_pi * (double)((bin[ch] * p) % M) / (double)M;
      const double cs = std::cos(th), sn = std::sin(th);
      are[2 * p] = (float)cs;
      are[2 * p + 1] = (float)-sn;
      aim[2 * p] = (float)sn;
      aim[2 * p + 1] = (float)cs;
    }
  }
  std::vector<float2> rot(M);
  for (int t = 0; t < M; ++t) {
    const double th = two_pi * (double)t / (double)M;
    rot[t] = float2{(float)std::cos(th), (float)-std::sin(th)};
  }
  std::vector<float> h32(d->PM, 0.f);
  for (int j = 0; j < taps; ++j) h32[j] = (float)b[j];
  std::vector<int> bins(8 * d->NT, 0);
  for (int ch = 0; ch < nch; ++ch) bins[ch] = bin[ch];
  const bool u8 = iq_dtype == SDR_IQ_U8;
  float* dA = nullptr;
  hipError_t e = upload(&dA, A.data(), A.size(), c->stream);
  if (e == hipSuccess) e = upload(&d->rot, rot.data(), rot.size(), c->stream);
  if (e == hipSuccess) e = upload(&d->taps, h32.data(), h32.size(), c->stream);
  if (e == hipSuccess) e = upload(&d->dbin, bins.data(), bins.size(), c->stream);
  if (e == hipSuccess) e = hipMalloc(&d->afrag, d->abytes);
  if (e == hipSuccess) e = mm_prep(dA, d->afrag, d->NT, d->KS, c->stream);
  if (e == hipSuccess) e = d->hist.alloc((size_t)(taps - 1) * (u8 ? 2 : 8), u8 ? 128 : 0, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host vectors are read until here)
  (void)hipFree(dA);
  if (e != hipSuccess) {
    sdr_pfb_destroy(d);
    return create_failed(e, "sdr_pfb_create");
  }
  *out = d;
  return SDR_OK;
}

void sdr_pfb_destroy(sdr_pfb* d) {
  if (d == nullptr) return;
  if (d->ctx != nullptr && set_dev(d->ctx) == SDR_OK) (void)hipStreamSynchronize(d->ctx->stream);
  (void)hipFree(d->afrag);
  (void)hipFree(d->rot);
  (void)hipFree(d->taps);
  (void)hipFree(d->dbin);
  d->hist.free();
  delete d;
}

int sdr_pfb_reset(sdr_pfb* d, int64_t position) {
  if (d == nullptr) return fail(SDR_EINVAL, "sdr_pfb_reset: object is NULL");
  if (position < 0 || position % d->D != 0)
    return fail(SDR_EINVAL, "sdr_pfb_reset: position=%lld must be >= 0 and a multiple of decim=%d", (long long)position, d->D);
  TRY(set_dev(d->ctx));
  HIP_TRY(d->hist.reset(d->ctx->stream));
  d->pos = position;
  return SDR_OK;
}

int sdr_pfb_position(sdr_pfb* d, int64_t* position) {
  if (d == nullptr || position == nullptr) return fail(SDR_EINVAL, "sdr_pfb_position: NULL argument");
  *position = d->pos;
  return SDR_OK;
}

int sdr_pfb_process_dev(sdr_pfb* d, const void* iq, int64_t n, float* out, int64_t out_stride) {
  TRY(decim_check_call(d, iq, n, out, out_stride, "sdr_pfb_process_dev"));
  const bool u8 = d->dtype == SDR_IQ_U8;
  if (((uintptr_t)iq & (u8 ? 1 : 7)) != 0 || ((uintptr_t)out & 7) != 0)
    return fail(SDR_EINVAL, "sdr_pfb_process_dev: iq must be aligned to one complex sample (%d B) and out to 8 B", u8 ? 2 : 8);
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const int W = 16 * d->CB;
  PfbLayout lay = pfb_layout(d->M, d->NT, d->PM, d->D, d->KS, d->CB, d->abytes);
  const bool alds = lay.total <= PFB_LDS_ALDS;
  if (!alds) lay.total = lay.a;
  if (lay.total > PFB_LDS_MAX) return fail(SDR_EHIP, "sdr_pfb_process_dev: %zu B of LDS", lay.total);   // (not inside the limits)
  PfbArgs P;
  P.iq = iq;
  P.hist = d->hist.current();
  P.taps = d->taps;
  P.afrag = d->afrag;
  P.rot = d->rot;
  P.bin = d->dbin;
  P.out = out;
  P.n = n;
  P.Mo = n / d->D;
  P.out_stride = out_stride;
  P.passes = ceil_div(P.Mo, W);
  P.s0 = (int)(d->pos % d->M);
  P.nch = d->nch;
  P.M = d->M;
  P.T = d->T;
  P.D = d->D;
  P.PM = d->PM;
  P.KS = d->KS;
  P.NT = d->NT;
  P.L = (W - 1) * d->D + d->PM;
  P.o_bin = (int)lay.bin;
  P.o_taps = (int)lay.taps;
  P.o_xs = (int)lay.xs;
  P.o_uh = (int)lay.uh;
  P.o_ul = (int)lay.ul;
  P.o_a = (int)lay.a;
  P.a_lds = alds ? (int)d->abytes : 0;
  P.invM = 1.f / (float)d->M;
  const size_t lds = lay.total;
  const dim3 blk(PFB_THREADS);
  // (beyond 64 KB only without the A fragments)
#define PFB_LAUNCH(CBV, U8V) \
  do {                       \
    if (alds) PFB_LAUNCH1(CBV, U8V, true); \
    else PFB_LAUNCH1(CBV, U8V, false);     \
  } while (0)
  // the grid: as many workgroups as the device holds at once (they are persistent: a second
  // round of them would run at a fraction of the occupancy), fewer for a short call
#define PFB_LAUNCH1(CBV, U8V, AV)                                                                        \
  do {                                                                                                   \
    auto kern = &pfb_mma_kernel<CBV, U8V, AV>;                                                           \
    if (lds > PFB_LDS_ALDS)                                                                              \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (d->grid == 0) {                                                                                  \
      int per = 0;                                                                                       \
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, PFB_THREADS, lds) != hipSuccess || per <= 0) per = 1; \
      d->grid = device_cus() * per;                                                                      \
    }                                                                                                    \
    kern<<<(unsigned)std::min<int64_t>(P.passes, d->grid), blk, lds, c->stream>>>(P);                    \
  } while (0)
  if (d->CB == PFB_CB) {
    if (u8) PFB_LAUNCH(PFB_CB, true);
    else PFB_LAUNCH(PFB_CB, false);
  } else {
    if (u8) PFB_LAUNCH(1, true);
    else PFB_LAUNCH(1, false);
  }
#undef PFB_LAUNCH
#undef PFB_LAUNCH1
  HIP_TRY(hipGetLastError());
  if (u8) HIP_TRY(d->hist.advance<uint16_t>(c->stream, iq, n, 0, 1, d->T - 1));
  else HIP_TRY(d->hist.advance<float2>(c->stream, iq, n, 0, 1, d->T - 1));
  d->pos += n;
  return SDR_OK;
}

int sdr_pfb_run(sdr_pfb* d, const void* iq_host, int64_t n, float* out_host, int64_t out_stride) {
  TRY(decim_check_call(d, iq_host, n, out_host, out_stride, "sdr_pfb_run"));
  sdr_ctx* c = d->ctx;
  TRY(set_dev(c));
  const size_t es = d->dtype == SDR_IQ_U8 ? 2 : 8, M = (size_t)(n / d->D);
  return run_staged(c, iq_host, {1, (size_t)n * es, 0}, out_host, {(size_t)d->nch, M * 8, (size_t)out_stride * 8},
                    [&](void* din, void* dout) { return sdr_pfb_process_dev(d, din, n, (float*)dout, (int64_t)M); });
}

}  // extern "C"
