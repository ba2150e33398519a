// Cascade of second-order sections on rows of real samples (include/sdr.h sdr_sos_*), and the
// programme loudness meter built on it (sdr_loud_*).  The reference has no such stage; the
// definitions are rtsdr.sos_model and rtsdr.LoudnessModel (sosfilter.py).
//
// A section is scipy.signal.sosfilt's (direct form II transposed), per row in f64:
//   y[n] = b0 x[n] + z1,   z1' = b1 x[n] - a1 y[n] + z2,   z2' = b2 x[n] - a2 y[n]
// i.e. s' = P s + c x with s = (z1, z2), P = [[-a1, 1], [-a2, 0]]: linear in the state, so the lanes'
// zero-state end states are combined by a scan with powers of P, as audio.hip does with its scalar
// pole.  The structure is the first-order section's (DESIGN §4 iir1_*):
//
//   a lane runs SOS_ITEMS = 8 consecutive samples of a section from zero state; the lanes' end
//   states go through an inclusive wave scan, v += P^(8 o) u, and over the workgroup's four waves
//   through LDS; the lane then reruns its 8 samples from its true entering state, and those
//   outputs, still f64 in registers, are the next section's input.  A tile is 2 048 samples.
//   Across tiles the cascade of K sections is one linear system with the 2K-vector of all
//   sections' states and M = A^2048, A the cascade's one-sample matrix: lower block-triangular,
//   and every product with M or a power of it skips the structural zeros, so a later section's
//   value never multiplies into an earlier one.
//   sos_tile_kernel<K, false>   (reduce) every tile but a row's last from zero state -> end state
//   sos_carry_kernel<K>         one wave per row: lane l chains 2^lg tiles, the lanes are scanned
//                               with M^(2^(lg + k)), a second pass stores each tile's entering state
//   sos_tile_kernel<K, true>    (apply) every tile from its true state: the f32 rows, the row's new
//                               state, and for the loudness meter the tile's sums of squares on
//                               either side of the one segment boundary a tile can hold
//   loud_fold_kernel            one wave per stream: the tiles' sums in a fixed order into the
//                               carried open segment and the ring of completed segments
// Rows of one tile take the apply launch alone.  No atomics, no waiting between workgroups.
//
// The powers decide the accuracy.  A K-weighting or rumble high-pass has its pole pair at about
// 0.995 e^(+-j 2e-4): P is far from normal (max |P^k| ~ 170) and powers formed in f64 by repeated
// squaring leave errors 300-700 times scipy's own rounding noise in the rows.  So every power --
// P^(8 m) for the lane, wave and workgroup strides, M, and M^(2^i) for the carry launch's lane
// strides (a lane chains a power of two of tiles so that these are all it needs) -- is formed on
// the host in long double (64-bit mantissa) and rounded once to f64: sos_table below, cached per
// coefficient set on the context.  No product tree runs on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sdr_common.h"
#include "sdr_ctx.h"

using namespace sdrint;

namespace {

constexpr int SOS_T = 256, SOS_ITEMS = 8, SOS_TILE = SOS_T * SOS_ITEMS, SOS_NW = SOS_T / 64;
constexpr int SOS_MAXK = SDR_SOS_MAX_SECTIONS;
constexpr int SOS_NPOW = 20;   // M^(2^i), i < 20: rows of up to 2^20 tiles, 2^14 a carry lane, scanned over 2^5 lanes
static_assert(SOS_TILE == SDR_SOS_TILE, "include/sdr.h names the tile");
static_assert(SOS_ITEMS == 8, "the row accesses below are two 16-B vectors per lane");
static_assert(SDR_LOUD_MIN_SEGMENT >= SOS_TILE, "a tile holds at most one segment boundary");

// the table of a cascade of K sections, in doubles:
//   [8 k + 0 .. 4]                 b0, b1, b2, a1, a2 of section k
//   pp_off(K) + 4 (65 k + m)       P_k^(8 m) row-major, m = 0 .. 64
//   mp_off(K) + 4 K K i            M^(2^i) row-major [2K][2K], i < SOS_NPOW
__host__ __device__ constexpr int pp_off(int K) { return 8 * K; }
__host__ __device__ constexpr int mp_off(int K) { return 8 * K + 4 * 65 * K; }
__host__ __device__ constexpr int tab_len(int K) { return mp_off(K) + 4 * K * K * SOS_NPOW; }

// ---- the host's powers, in long double ---------------------------------------------------------
typedef long double ld;

void mat_mul(const ld* a, const ld* b, ld* c, int d) {
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      ld s = 0;
      for (int k = 0; k < d; ++k) s += a[i * d + k] * b[k * d + j];
      c[i * d + j] = s;
    }
}

// out = a^e by binary powering (d <= 8)
void mat_pow(const ld* a, unsigned e, ld* out, int d) {
  ld base[64], acc[64], t[64];
  std::copy(a, a + d * d, base);
  for (int i = 0; i < d * d; ++i) acc[i] = (i / d == i % d) ? 1 : 0;
  for (; e != 0; e >>= 1) {
    if (e & 1) {
      mat_mul(acc, base, t, d);
      std::copy(t, t + d * d, acc);
    }
    mat_mul(base, base, t, d);
    std::copy(t, t + d * d, base);
  }
  std::copy(acc, acc + d * d, out);
}

void sos_table(const double* sos, int K, std::vector<double>* out) {
  const int D = 2 * K;
  std::vector<double>& h = *out;
  h.assign((size_t)tab_len(K), 0.0);
  ld A[64] = {};
  for (int k = 0; k < K; ++k) {
    const double* s = sos + 6 * k;
    const double c[5] = {s[0], s[1], s[2], s[4], s[5]};
    std::copy(c, c + 5, &h[8 * k]);
    const ld P[4] = {-(ld)s[4], 1, -(ld)s[5], 0};
    for (int m = 0; m <= 64; ++m) {
      ld pw[4];
      mat_pow(P, (unsigned)(SOS_ITEMS * m), pw, 2);
      for (int e = 0; e < 4; ++e) h[pp_off(K) + 4 * (65 * k + m) + e] = (double)pw[e];
    }
    // the cascade's one-sample matrix: section k's input is sum_j (prod_{j < m < k} b0_m) z1_j + (..) x
    const ld c1 = (ld)s[1] - (ld)s[4] * (ld)s[0], c2 = (ld)s[2] - (ld)s[5] * (ld)s[0];
    for (int e = 0; e < 4; ++e) A[(2 * k + e / 2) * D + 2 * k + e % 2] = P[e];
    ld g = 1;
    for (int j = k - 1; j >= 0; --j) {
      A[(2 * k) * D + 2 * j] = c1 * g;
      A[(2 * k + 1) * D + 2 * j] = c2 * g;
      g *= (ld)sos[6 * j];
    }
  }
  ld M[64], t[64];
  mat_pow(A, SOS_TILE, M, D);
  for (int i = 0; i < SOS_NPOW; ++i) {
    for (int e = 0; e < D * D; ++e) h[mp_off(K) + D * D * i + e] = (double)M[e];
    mat_mul(M, M, t, D);
    std::copy(t, t + D * D, M);
  }
}

int get_sos_tab(sdr_ctx* c, const double* sos, int K, const double** out) {
  for (const SosTab& t : c->sos)
    if (t.K == K && std::memcmp(t.sos, sos, sizeof(double) * 6 * K) == 0) {
      *out = t.dev;
      return SDR_OK;
    }
  std::vector<double> h;
  sos_table(sos, K, &h);
  SosTab t;
  t.K = K;
  std::copy(sos, sos + 6 * K, t.sos);
  hipError_t e = hipMalloc(&t.dev, sizeof(double) * h.size());
  if (e == hipSuccess) e = hipMemcpy(t.dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    return create_failed(e, "cascade table upload");
  }
  c->sos.push_back(t);
  *out = t.dev;
  return SDR_OK;
}

// ---- the kernels ---------------------------------------------------------------------------------
struct SosArgs {
  const float* x[2];       // a channel's rows; row (s, ch) is x[ch] + s x_stride
  float* y[2];             // NULL: nothing is stored
  int64_t x_stride, y_stride, n;
  int nch, ntiles, lg;     // lg: a carry lane chains 2^lg tiles
  const double* tab;
  double* state;           // [rows][2K], row = s nch + ch
  double* agg;             // [rows][ntiles][2K]: the tiles' zero-state end states (a row's last: unused)
  double* carry;           // [rows][ntiles][2K]: the state entering each tile
  // the loudness meter (METER)
  double* part;            // [rows][ntiles][2]: sums of squares before / from the tile's segment boundary
  int64_t pos0, seg;       // stream position of the call's first sample within its segment; segment length
  double inv_ref;
};

// one section of one tile: v[0 .. len) in, the section's output out; sin: the section's state entering
// the tile (the same in every lane); *e1, *e2: the lane's state after its last sample.  wagg: LDS,
// free again when the call returns.
__device__ __forceinline__ void section_tile(const double* __restrict__ coef, const double* __restrict__ pp, double (&v)[SOS_ITEMS],
                                             int len, double sin1, double sin2, double (*wagg)[2], int tid, double* e1, double* e2) {
  const int lane = tid & 63, wv = tid >> 6;
  const double b0 = coef[0], b1 = coef[1], b2 = coef[2], a1 = coef[3], a2 = coef[4];
  double z1 = 0.0, z2 = 0.0;
#pragma unroll
  for (int j = 0; j < SOS_ITEMS; ++j)
    if (j < len) {
      const double y = b0 * v[j] + z1;
      z1 = b1 * v[j] - a1 * y + z2;
      z2 = b2 * v[j] - a2 * y;
    }
  double v1 = z1, v2 = z2;              // inclusive: the state after lanes [.., lane] from zero
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int o = 1 << k;
    const double u1 = __shfl_up(v1, o, 64), u2 = __shfl_up(v2, o, 64);
    const double* __restrict__ p = pp + 4 * o;
    if (lane >= o) {
      v1 = p[0] * u1 + p[1] * u2 + v1;
      v2 = p[2] * u1 + p[3] * u2 + v2;
    }
  }
  if (lane == 63) {
    wagg[wv][0] = v1;
    wagg[wv][1] = v2;
  }
  __syncthreads();
  double c1 = sin1, c2 = sin2;          // the state entering this wave
  const double* __restrict__ pw = pp + 4 * 64;
#pragma unroll
  for (int w = 0; w < SOS_NW - 1; ++w)
    if (w < wv) {
      const double t1 = pw[0] * c1 + pw[1] * c2 + wagg[w][0], t2 = pw[2] * c1 + pw[3] * c2 + wagg[w][1];
      c1 = t1;
      c2 = t2;
    }
  __syncthreads();
  double x1 = __shfl_up(v1, 1, 64), x2 = __shfl_up(v2, 1, 64);
  if (lane == 0) x1 = x2 = 0.0;
  const double* __restrict__ pl = pp + 4 * lane;
  z1 = x1 + pl[0] * c1 + pl[1] * c2;
  z2 = x2 + pl[2] * c1 + pl[3] * c2;
#pragma unroll
  for (int j = 0; j < SOS_ITEMS; ++j)
    if (j < len) {
      const double y = b0 * v[j] + z1;
      z1 = b1 * v[j] - a1 * y + z2;
      z2 = b2 * v[j] - a2 * y;
      v[j] = y;
    }
  *e1 = z1;
  *e2 = z2;
}

// APPLY = false: the zero-state end state of every tile but each row's last -> agg
// APPLY = true: every tile from its entering state -> the rows, the state; METER: the tile's sums
template <int K, bool APPLY, bool METER>
__global__ __launch_bounds__(SOS_T) void sos_tile_kernel(const SosArgs a) {
  constexpr int D = 2 * K;
  __shared__ double wagg[SOS_NW][2];
  const int tid = threadIdx.x, s = blockIdx.y, ch = blockIdx.z;
  const int64_t row = (int64_t)s * a.nch + ch, tile = blockIdx.x;
  const int64_t i0 = tile * SOS_TILE + (int64_t)tid * SOS_ITEMS, left = a.n - i0;
  const int len = !APPLY || left >= SOS_ITEMS ? SOS_ITEMS : left > 0 ? (int)left : 0;
  const float* __restrict__ xr = a.x[ch] + (int64_t)s * a.x_stride + i0;
  double v[SOS_ITEMS];
  if (len == SOS_ITEMS && ((uintptr_t)xr & 15) == 0) {
    const f4v p = *reinterpret_cast<const f4v*>(xr), q = *reinterpret_cast<const f4v*>(xr + 4);
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w;
    v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < SOS_ITEMS; ++j) v[j] = j < len ? (double)xr[j] : 0.0;
  }
  // the state entering the tile: the carry launch's, or the row's own for rows of one tile
  const double* sin = a.ntiles > 1 ? a.carry + (row * a.ntiles + tile) * D : a.state + row * D;
  double se[D], e[D];
#pragma unroll
  for (int d = 0; d < D; ++d) se[d] = APPLY ? sin[d] : 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k)
    section_tile(a.tab + 8 * k, a.tab + pp_off(K) + 4 * 65 * k, v, len, se[2 * k], se[2 * k + 1], wagg, tid, &e[2 * k], &e[2 * k + 1]);
  if constexpr (!APPLY) {
    if (tid == SOS_T - 1) {
      double* __restrict__ g = a.agg + (row * a.ntiles + tile) * D;
#pragma unroll
      for (int d = 0; d < D; ++d) g[d] = e[d];
    }
  } else {
    // (every lane has read the entering state in front of the sections' barriers)
    if (len > 0 && i0 + len == a.n) {
      double* st = a.state + row * D;
#pragma unroll
      for (int d = 0; d < D; ++d) st[d] = e[d];
    }
    if (a.y[ch] != nullptr) {
      float* __restrict__ yr = a.y[ch] + (int64_t)s * a.y_stride + i0;
      if (len == SOS_ITEMS && ((uintptr_t)yr & 15) == 0) {
        *reinterpret_cast<f4v*>(yr) = f4v{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        *reinterpret_cast<f4v*>(yr + 4) = f4v{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
      } else {
#pragma unroll
        for (int j = 0; j < SOS_ITEMS; ++j)
          if (j < len) yr[j] = (float)v[j];
      }
    }
    if constexpr (METER) {
      __shared__ double red[SOS_NW][2];
      // the call's first sample of the segment behind the one the tile starts in
      const int64_t bnd = ((a.pos0 + tile * SOS_TILE) / a.seg + 1) * a.seg - a.pos0;
      double qa = 0.0, qb = 0.0;
#pragma unroll
      for (int j = 0; j < SOS_ITEMS; ++j)
        if (j < len) {
          const double w = v[j] * a.inv_ref;
          if (i0 + j < bnd) qa = __builtin_fma(w, w, qa);
          else qb = __builtin_fma(w, w, qb);
        }
      qa = wave_sum(qa);
      qb = wave_sum(qb);
      if ((tid & 63) == 0) {
        red[tid >> 6][0] = qa;
        red[tid >> 6][1] = qb;
      }
      __syncthreads();
      if (tid == 0) {
        double* __restrict__ p = a.part + (row * a.ntiles + tile) * 2;
        p[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        p[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
      }
    }
  }
}

// v += m u for a lower block-triangular m (2 x 2 blocks, row-major [2K][2K]): the zeros are skipped
template <int K>
__device__ __forceinline__ void tri_mul_add(const double* __restrict__ m, const double (&u)[2 * K], double (&v)[2 * K]) {
  constexpr int D = 2 * K;
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c)
      if (c / 2 <= r / 2) v[r] = m[r * D + c] * u[c] + v[r];
}

// carry: one wave per row; lane l chains the tiles [l 2^lg, (l + 1) 2^lg) from zero (lane 0: from
// the row's state), the lanes are scanned with M^(2^(lg + k)), and a second pass over the lane's
// tiles stores the state entering each.  agg of a row's last tile does not exist and is not read.
template <int K>
__global__ __launch_bounds__(64) void sos_carry_kernel(const SosArgs a) {
  constexpr int D = 2 * K;
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const double* __restrict__ m = a.tab + mp_off(K);
  const double* __restrict__ agg = a.agg + row * a.ntiles * D;
  double* __restrict__ carry = a.carry + row * a.ntiles * D;
  const int64_t k0 = (int64_t)lane << a.lg, kn = k0 + ((int64_t)1 << a.lg), k1 = kn < a.ntiles ? kn : a.ntiles;
  double zi[D], z[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    zi[d] = a.state[row * D + d];
    z[d] = lane == 0 ? zi[d] : 0.0;
  }
  for (int64_t k = k0; k < k1; ++k)
    if (k < a.ntiles - 1) {
      double t[D];
#pragma unroll
      for (int d = 0; d < D; ++d) t[d] = agg[k * D + d];
      tri_mul_add<K>(m, z, t);
#pragma unroll
      for (int d = 0; d < D; ++d) z[d] = t[d];
    }
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int o = 1 << s;
    double u[D];
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = __shfl_up(z[d], o, 64);
    if (lane >= o) tri_mul_add<K>(m + D * D * (a.lg + s), u, z);
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double up = __shfl_up(z[d], 1, 64);
    z[d] = lane == 0 ? zi[d] : up;
  }
  for (int64_t k = k0; k < k1; ++k) {
#pragma unroll
    for (int d = 0; d < D; ++d) carry[k * D + d] = z[d];
    if (k < a.ntiles - 1) {
      double t[D];
#pragma unroll
      for (int d = 0; d < D; ++d) t[d] = agg[k * D + d];
      tri_mul_add<K>(m, z, t);
#pragma unroll
      for (int d = 0; d < D; ++d) z[d] = t[d];
    }
  }
}

struct LoudFold {
  const double* part;      // [rows][ntiles][2]
  double* open;            // [rows]: the open segment's sum
  double* ring;            // [rows][cap]: completed segment g at g % cap
  int nch, ntiles, cap;
  int64_t pos0, n, seg, done0;   // done0: segments completed before the call
};

// one wave per stream.  Segment j of the call gets, in this order: the carried open sum (j = 0), the
// part behind the boundary of the tile that straddles into it, and the parts of the tiles that start
// in it.  Segments of up to 64 tiles (the 100 ms of a loudness meter: three) go a lane each, 64 at
// a time, the lane adding its tiles one after the other; longer ones one after the other, their
// tiles a lane each and then the wave's butterfly.  A completed segment is stored only if it is among
// the latest `cap`: no two lanes store to one slot of the ring.
__global__ __launch_bounds__(64) void loud_fold_kernel(const LoudFold a) {
  const int lane = threadIdx.x;
  const int64_t nseg = (a.pos0 + a.n + a.seg - 1) / a.seg, ndone = (a.pos0 + a.n) / a.seg;
  const bool by_lane = a.seg <= 64 * SOS_TILE;
  for (int ch = 0; ch < a.nch; ++ch) {
    const int64_t row = (int64_t)blockIdx.x * a.nch + ch;
    const double* __restrict__ part = a.part + row * a.ntiles * 2;
    double* __restrict__ ring = a.ring + row * a.cap;
    const double open = a.open[row];
    for (int64_t j0 = 0; j0 < nseg; j0 += by_lane ? 64 : 1) {
      const int64_t j = by_lane ? j0 + lane : j0;
      const int64_t lo = j * a.seg - a.pos0, hi = lo + a.seg;          // the segment, in samples of the call
      const int64_t t_lo = lo > 0 ? (lo + SOS_TILE - 1) / SOS_TILE : 0;
      const int64_t t_up = (hi + SOS_TILE - 1) / SOS_TILE, t_hi = t_up < a.ntiles ? t_up : a.ntiles;
      double total = j == 0 ? open : 0.0;
      if (j < nseg && t_lo > 0) total += part[2 * (t_lo - 1) + 1];
      if (by_lane) {
        if (j < nseg)
          for (int64_t t = t_lo; t < t_hi; ++t) total += part[2 * t];
      } else {
        double acc = 0.0;
        for (int64_t t = t_lo + lane; t < t_hi; t += 64) acc += part[2 * t];
        total += wave_sum(acc);
      }
      if (j < nseg && (by_lane || lane == 0)) {
        if (j >= ndone) a.open[row] = total;                             // the call ends inside it
        else if (j + a.cap >= ndone) ring[(a.done0 + j) % a.cap] = total;
      }
    }
    if (lane == 0 && ndone == nseg) a.open[row] = 0.0;                   // the call ended on a boundary
  }
}

template <int K>
void sos_launch_k(const SosArgs& a, int rows_s, bool meter, hipStream_t st, hipEvent_t* ev) {
  const dim3 blk(SOS_T);
  if (ev) (void)hipEventRecord(ev[0], st);
  if (a.ntiles > 1) hipLaunchKernelGGL((sos_tile_kernel<K, false, false>), dim3((unsigned)(a.ntiles - 1), (unsigned)rows_s, (unsigned)a.nch), blk, 0, st, a);
  if (ev) (void)hipEventRecord(ev[1], st);
  if (a.ntiles > 1) hipLaunchKernelGGL(sos_carry_kernel<K>, dim3((unsigned)(rows_s * a.nch)), dim3(64), 0, st, a);
  if (ev) (void)hipEventRecord(ev[2], st);
  const dim3 grid((unsigned)a.ntiles, (unsigned)rows_s, (unsigned)a.nch);
  if constexpr (K == 2) {
    if (meter) hipLaunchKernelGGL((sos_tile_kernel<K, true, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((sos_tile_kernel<K, true, false>), grid, blk, 0, st, a);
  } else {
    hipLaunchKernelGGL((sos_tile_kernel<K, true, false>), grid, blk, 0, st, a);
  }
  if (ev) (void)hipEventRecord(ev[3], st);
}

// what a cascade on `S` streams of `nch` rows owns
struct SosCore {
  sdr_ctx* ctx = nullptr;
  int K = 0, S = 0, nch = 1;
  const double* tab = nullptr;
  double* state = nullptr;              // [S nch][2K]
  GrowMem<double> agg, carry, part;
  void release() {
    agg.release();
    carry.release();
    part.release();
  }
};

// the launches of a call: a.x / y / strides / n (and the meter's fields) come filled in
int sos_launch(SosCore& k, SosArgs a, bool meter, hipEvent_t* ev, const char* what) {
  sdr_ctx* c = k.ctx;
  const int64_t nt = ceil_div(a.n, SOS_TILE);
  a.nch = k.nch;
  a.ntiles = (int)nt;
  a.lg = 0;
  while (((int64_t)64 << a.lg) < nt) ++a.lg;
  a.tab = k.tab;
  a.state = k.state;
  const size_t rows = (size_t)k.S * k.nch;
  if (nt > 1) {
    TRY(k.agg.fit(rows * nt * 2 * k.K, c->stream, what));
    TRY(k.carry.fit(rows * nt * 2 * k.K, c->stream, what));
  }
  if (meter) TRY(k.part.fit(rows * nt * 2, c->stream, what));
  a.agg = k.agg.p;
  a.carry = k.carry.p;
  a.part = k.part.p;
  switch (k.K) {
    case 1: sos_launch_k<1>(a, k.S, meter, c->stream, ev); break;
    case 2: sos_launch_k<2>(a, k.S, meter, c->stream, ev); break;
    case 3: sos_launch_k<3>(a, k.S, meter, c->stream, ev); break;
    default: sos_launch_k<4>(a, k.S, meter, c->stream, ev); break;
  }
  HIP_TRY(hipGetLastError());
  return SDR_OK;
}

int sos_check_coeffs(const double* sos, int K, const char* what) {
  if (sos == nullptr) return fail(SDR_EINVAL, "%s: sos is NULL", what);
  if (K < 1 || K > SOS_MAXK) return fail(SDR_EINVAL, "%s: K=%d outside [1, %d]", what, K, SOS_MAXK);
  for (int k = 0; k < K; ++k) {
    const double* s = sos + 6 * k;
    for (int j = 0; j < 6; ++j)
      if (!std::isfinite(s[j])) return fail(SDR_EINVAL, "%s: sos[%d][%d] is not finite", what, k, j);
    if (s[3] != 1.0) return fail(SDR_EINVAL, "%s: a0=%g of section %d is not 1", what, s[3], k);
    if (std::fabs(s[5]) >= 1.0 || std::fabs(s[4]) >= 1.0 + s[5])
      return fail(SDR_EINVAL, "%s: section %d (a1=%g, a2=%g) has a pole on or outside the unit circle", what, k, s[4], s[5]);
  }
  return SDR_OK;
}

int sos_check_rows(const char* what, const char* name, const float* p, int64_t stride, int64_t n) {
  if (n < 1 || n > INT32_MAX) return fail(SDR_EINVAL, "%s: n=%lld outside [1, 2^31 - 1]", what, (long long)n);
  if (stride < n) return fail(SDR_EINVAL, "%s: %s_stride=%lld < n=%lld", what, name, (long long)stride, (long long)n);
  if (((uintptr_t)p & 3) != 0) return fail(SDR_EINVAL, "%s: %s must be aligned to 4 B", what, name);
  return SDR_OK;
}

// a timer's events while it is on, for sos_launch
template <int N>
hipEvent_t* events_of(StageTimer<N>& tm) {
  return tm.on ? tm.ev : nullptr;
}

}  // namespace

struct sdr_sos {
  SosCore k;
  StageTimer<3> tm;                    // around the three launches of a call (sdr_sos_set_timing)
};

struct sdr_loud {
  SosCore k;
  sdr_loud_params prm = {};
  int64_t pos = 0;                     // samples per stream since the last reset
  double* ring = nullptr;              // [S][channels][cap]
  double* open = nullptr;              // [S][channels]
  StageTimer<4> tm;
};

extern "C" {

int sdr_sos_create(sdr_ctx* c, int nrows, const double* sos, int K, sdr_sos** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_sos_create: out is NULL");
  *out = nullptr;
  if (nrows < 1 || nrows > SDR_SOS_MAX_ROWS) return fail(SDR_EINVAL, "sdr_sos_create: nrows=%d outside [1, %d]", nrows, SDR_SOS_MAX_ROWS);
  TRY(sos_check_coeffs(sos, K, "sdr_sos_create"));
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_sos* f = new (std::nothrow) sdr_sos;
  if (f == nullptr) return fail(SDR_ENOMEM, "sdr_sos_create: out of host memory");
  f->k.ctx = c;
  f->k.K = K;
  f->k.S = nrows;
  int rc = get_sos_tab(c, sos, K, &f->k.tab);
  if (rc == SDR_OK) {
    const hipError_t e = hipMalloc(&f->k.state, sizeof(double) * 2 * K * nrows);
    rc = e != hipSuccess ? create_failed(e, "sdr_sos_create") : sdr_sos_reset(f);
  }
  if (rc != SDR_OK) {
    sdr_sos_destroy(f);
    return rc;
  }
  *out = f;
  return SDR_OK;
}

void sdr_sos_destroy(sdr_sos* f) {
  if (f == nullptr) return;
  if (f->k.ctx != nullptr && set_dev(f->k.ctx) == SDR_OK) (void)hipStreamSynchronize(f->k.ctx->stream);
  (void)hipFree(f->k.state);
  f->k.release();
  delete f;
}

int sdr_sos_reset(sdr_sos* f) {
  if (f == nullptr) return fail(SDR_EINVAL, "sdr_sos_reset: object is NULL");
  TRY(set_dev(f->k.ctx));
  HIP_TRY(hipMemsetAsync(f->k.state, 0, sizeof(double) * 2 * f->k.K * f->k.S, f->k.ctx->stream));
  return SDR_OK;
}

int sdr_sos_process_dev(sdr_sos* f, const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t n) {
  if (f == nullptr) return fail(SDR_EINVAL, "sdr_sos_process_dev: object is NULL");
  if (x == nullptr) return fail(SDR_EINVAL, "sdr_sos_process_dev: x is NULL");
  TRY(sos_check_rows("sdr_sos_process_dev", "x", x, x_stride, n));
  if (y != nullptr) {
    TRY(sos_check_rows("sdr_sos_process_dev", "y", y, y_stride, n));
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + 4 * ((uintptr_t)(f->k.S - 1) * x_stride + n);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + 4 * ((uintptr_t)(f->k.S - 1) * y_stride + n);
    if (x0 < y1 && y0 < x1 && !(x0 == y0 && x_stride == y_stride))
      return fail(SDR_EINVAL, "sdr_sos_process_dev: x and y overlap (only y == x with equal strides may)");
  }
  TRY(set_dev(f->k.ctx));
  SosArgs a = {};
  a.x[0] = x;
  a.y[0] = y;
  a.x_stride = x_stride;
  a.y_stride = y_stride;
  a.n = n;
  TRY(sos_launch(f->k, a, false, events_of(f->tm), "sdr_sos_process_dev"));
  if (f->tm.on) f->tm.timed = true;
  return SDR_OK;
}

int sdr_sos_run(sdr_sos* f, const float* x_host, float* y_host, int64_t stride, int64_t n) {
  if (f == nullptr) return fail(SDR_EINVAL, "sdr_sos_run: object is NULL");
  if (x_host == nullptr) return fail(SDR_EINVAL, "sdr_sos_run: x_host is NULL");
  TRY(sos_check_rows("sdr_sos_run", "x", nullptr, stride, n));
  sdr_ctx* c = f->k.ctx;
  TRY(set_dev(c));
  const HostRows r{(size_t)f->k.S, (size_t)n * 4, (size_t)stride * 4};
  return run_staged(c, x_host, r, y_host, r, [&](void* din, void* dout) { return sdr_sos_process_dev(f, (const float*)din, n, (float*)dout, n, n); });
}

int sdr_sos_state(sdr_sos* f, double* host) {
  if (f == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_sos_state: NULL argument");
  return fetch(f->k.ctx, f->k.state, (size_t)f->k.S * 2 * f->k.K, host);
}

int sdr_sos_set_state(sdr_sos* f, const double* host) {
  if (f == nullptr || host == nullptr) return fail(SDR_EINVAL, "sdr_sos_set_state: NULL argument");
  TRY(set_dev(f->k.ctx));
  HIP_TRY(hipMemcpyAsync(f->k.state, host, sizeof(double) * 2 * f->k.K * f->k.S, hipMemcpyHostToDevice, f->k.ctx->stream));
  HIP_TRY(hipStreamSynchronize(f->k.ctx->stream));
  return SDR_OK;
}

int sdr_sos_set_timing(sdr_sos* f, int on) {
  if (f == nullptr) return fail(SDR_EINVAL, "sdr_sos_set_timing: object is NULL");
  TRY(set_dev(f->k.ctx));
  HIP_TRY(f->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_sos_stage_ms(sdr_sos* f, float* ms) {
  if (f == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_sos_stage_ms: NULL argument");
  return f->tm.elapsed(ms, "sdr_sos_stage_ms: no timed call (sdr_sos_set_timing)");
}

// ---- the loudness meter --------------------------------------------------------------------------
int sdr_loud_create(sdr_ctx* c, int nstreams, int channels, const sdr_loud_params* params, sdr_loud** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_loud_create: out is NULL");
  *out = nullptr;
  if (params == nullptr) return fail(SDR_EINVAL, "sdr_loud_create: params is NULL");
  if (nstreams < 1 || nstreams > SDR_SOS_MAX_ROWS) return fail(SDR_EINVAL, "sdr_loud_create: nstreams=%d outside [1, %d]", nstreams, SDR_SOS_MAX_ROWS);
  if (channels != 1 && channels != 2) return fail(SDR_EINVAL, "sdr_loud_create: channels=%d is not 1 or 2", channels);
  if (params->segment < SDR_LOUD_MIN_SEGMENT || params->segment > SDR_LOUD_MAX_SEGMENT)
    return fail(SDR_EINVAL, "sdr_loud_create: segment=%lld outside [%d, %d]", (long long)params->segment, SDR_LOUD_MIN_SEGMENT, SDR_LOUD_MAX_SEGMENT);
  if (params->cap < 4 || params->cap > SDR_LOUD_MAX_CAP) return fail(SDR_EINVAL, "sdr_loud_create: cap=%d outside [4, %d]", params->cap, SDR_LOUD_MAX_CAP);
  if (!(std::isfinite(params->reference) && params->reference > 0.0))
    return fail(SDR_EINVAL, "sdr_loud_create: reference=%g is not finite and positive", params->reference);
  CHECK_CTX(c);
  TRY(set_dev(c));
  // ITU-R BS.1770-4 table 1 and 2: the pre-filter (shelf) and the RLB high-pass at 48 kHz
  static const double kw[12] = {1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585,
                                1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621};
  sdr_loud* l = new (std::nothrow) sdr_loud;
  if (l == nullptr) return fail(SDR_ENOMEM, "sdr_loud_create: out of host memory");
  l->k.ctx = c;
  l->k.K = 2;
  l->k.S = nstreams;
  l->k.nch = channels;
  l->prm = *params;
  const size_t rows = (size_t)nstreams * channels;
  int rc = get_sos_tab(c, kw, 2, &l->k.tab);
  if (rc == SDR_OK) {
    hipError_t e = hipMalloc(&l->k.state, sizeof(double) * 4 * rows);
    if (e == hipSuccess) e = hipMalloc(&l->ring, sizeof(double) * rows * params->cap);
    if (e == hipSuccess) e = hipMalloc(&l->open, sizeof(double) * rows);
    rc = e != hipSuccess ? create_failed(e, "sdr_loud_create") : sdr_loud_reset(l);
  }
  if (rc != SDR_OK) {
    sdr_loud_destroy(l);
    return rc;
  }
  *out = l;
  return SDR_OK;
}

void sdr_loud_destroy(sdr_loud* l) {
  if (l == nullptr) return;
  if (l->k.ctx != nullptr && set_dev(l->k.ctx) == SDR_OK) (void)hipStreamSynchronize(l->k.ctx->stream);
  (void)hipFree(l->k.state);
  (void)hipFree(l->ring);
  (void)hipFree(l->open);
  l->k.release();
  delete l;
}

int sdr_loud_reset(sdr_loud* l) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_loud_reset: object is NULL");
  sdr_ctx* c = l->k.ctx;
  TRY(set_dev(c));
  const size_t rows = (size_t)l->k.S * l->k.nch;
  HIP_TRY(hipMemsetAsync(l->k.state, 0, sizeof(double) * 4 * rows, c->stream));
  HIP_TRY(hipMemsetAsync(l->ring, 0, sizeof(double) * rows * l->prm.cap, c->stream));
  HIP_TRY(hipMemsetAsync(l->open, 0, sizeof(double) * rows, c->stream));
  l->pos = 0;
  return SDR_OK;
}

int sdr_loud_process_dev(sdr_loud* l, const float* ch0, const float* ch1, int64_t stride, int64_t n) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_loud_process_dev: object is NULL");
  if (ch0 == nullptr) return fail(SDR_EINVAL, "sdr_loud_process_dev: ch0 is NULL");
  if ((ch1 != nullptr) != (l->k.nch == 2)) return fail(SDR_EINVAL, "sdr_loud_process_dev: ch1 must be given with two channels and NULL with one");
  TRY(sos_check_rows("sdr_loud_process_dev", "ch0", ch0, stride, n));
  if (ch1 != nullptr) TRY(sos_check_rows("sdr_loud_process_dev", "ch1", ch1, stride, n));
  sdr_ctx* c = l->k.ctx;
  TRY(set_dev(c));
  const int64_t seg = l->prm.segment;
  SosArgs a = {};
  a.x[0] = ch0;
  a.x[1] = ch1;
  a.x_stride = stride;
  a.n = n;
  a.pos0 = l->pos % seg;
  a.seg = seg;
  a.inv_ref = 1.0 / l->prm.reference;
  TRY(sos_launch(l->k, a, true, events_of(l->tm), "sdr_loud_process_dev"));
  const LoudFold f{l->k.part.p, l->open, l->ring, l->k.nch, (int)ceil_div(n, SOS_TILE), l->prm.cap, a.pos0, n, seg, l->pos / seg};
  hipLaunchKernelGGL(loud_fold_kernel, dim3((unsigned)l->k.S), dim3(64), 0, c->stream, f);
  HIP_TRY(hipGetLastError());
  HIP_TRY(l->tm.mark(4, c->stream));
  l->pos += n;
  return SDR_OK;
}

int sdr_loud_run(sdr_loud* l, const float* ch0_host, const float* ch1_host, int64_t stride, int64_t n) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_loud_run: object is NULL");
  if (ch0_host == nullptr) return fail(SDR_EINVAL, "sdr_loud_run: ch0_host is NULL");
  if ((ch1_host != nullptr) != (l->k.nch == 2)) return fail(SDR_EINVAL, "sdr_loud_run: ch1_host must be given with two channels and NULL with one");
  TRY(sos_check_rows("sdr_loud_run", "ch0", nullptr, stride, n));
  sdr_ctx* c = l->k.ctx;
  TRY(set_dev(c));
  const size_t S = (size_t)l->k.S, rb = (size_t)n * 4;
  void *d0 = nullptr, *d1 = nullptr;
  TRY(scratch(c, S_IN, S * rb, &d0));
  HIP_TRY(hipMemcpy2DAsync(d0, rb, ch0_host, (size_t)stride * 4, rb, S, hipMemcpyHostToDevice, c->stream));
  if (ch1_host != nullptr) {
    TRY(scratch(c, S_IN2, S * rb, &d1));
    HIP_TRY(hipMemcpy2DAsync(d1, rb, ch1_host, (size_t)stride * 4, rb, S, hipMemcpyHostToDevice, c->stream));
  }
  TRY(sdr_loud_process_dev(l, (const float*)d0, (const float*)d1, n, n));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_loud_segments(sdr_loud* l, double* host, int64_t* first, int64_t* count) {
  if (l == nullptr || host == nullptr || first == nullptr || count == nullptr) return fail(SDR_EINVAL, "sdr_loud_segments: NULL argument");
  const size_t rows = (size_t)l->k.S * l->k.nch, cap = (size_t)l->prm.cap;
  std::vector<double> ring(rows * cap);
  TRY(fetch(l->k.ctx, l->ring, ring.size(), ring.data()));
  const int64_t done = l->pos / l->prm.segment, cnt = std::min<int64_t>(done, (int64_t)cap);
  *first = done - cnt;
  *count = cnt;
  for (size_t r = 0; r < rows; ++r)
    for (int64_t i = 0; i < cnt; ++i) host[r * cap + i] = ring[r * cap + (size_t)((*first + i) % (int64_t)cap)];
  return SDR_OK;
}

int sdr_loud_state_dev(sdr_loud* l, const double** ring_dev, const double** open_dev) {
  if (l == nullptr || (ring_dev == nullptr && open_dev == nullptr)) return fail(SDR_EINVAL, "sdr_loud_state_dev: NULL argument");
  if (ring_dev != nullptr) *ring_dev = l->ring;
  if (open_dev != nullptr) *open_dev = l->open;
  return SDR_OK;
}

int sdr_loud_set_timing(sdr_loud* l, int on) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_loud_set_timing: object is NULL");
  TRY(set_dev(l->k.ctx));
  HIP_TRY(l->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_loud_stage_ms(sdr_loud* l, float* ms) {
  if (l == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_loud_stage_ms: NULL argument");
  return l->tm.elapsed(ms, "sdr_loud_stage_ms: no timed call (sdr_loud_set_timing)");
}

}  // extern "C"
