// Audio output stage: a first-order IIR section (FM de-emphasis) as a parallel scan, and the
// float -> int16 PCM conversion of the audio rows.
//
// The section is scipy.signal.lfilter([b0, b1], [1, a1], x, zi) per row:
//   y[n] = b0 x[n] + z[n-1],   z[n] = b1 x[n] - a1 y[n]      (state z: one f64, scipy's zi / zf)
// i.e. z[n] = p z[n-1] + c x[n] with the pole p = -a1: linear in the state, so the response to
// the state entering a run of samples is added to the run's zero-state response afterwards,
//   y[n0 + j] = y0[j] + p^j z_in,    z_end = z0_end + p^len z_in.
// A lane runs IIR_ITEMS consecutive samples from zero state (f64), the lanes' end states are
// combined by an inclusive wave scan and a chain over the workgroup's waves, and the state
// entering each tile of IIR_TILE samples comes from two launches before the apply launch: the
// tiles' zero-state end states (reduce), then one wave per row that chains them from zi (carry).
// There is no waiting between workgroups inside a launch.  Rows of one tile skip both.
//
// Pole powers: p^j inside a lane by repeated multiplication; every stride power (lanes, waves,
// tiles, the carry scan's lane strides) is pow() of the host in f64 -- the table
// sdr_iir1_table() and IirLaunch::q -- so each is correctly rounded to within the host libm's
// error instead of carrying the roundings of a product tree.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sdr_launch.h"

namespace {

constexpr int IIR_T = SDR_IIR_THREADS, IIR_ITEMS = SDR_IIR_ITEMS, IIR_TILE = SDR_IIR_TILE, IIR_NW = IIR_T / 64;
static_assert(IIR_ITEMS == 8, "the row accesses below are two 16-B vectors per lane");
typedef float f4v __attribute__((ext_vector_type(4)));

// the PCM rule of the audio stage (include/sdr.h sdr_audio_out_dev)
__device__ __forceinline__ int pcm16(float x) {
  const float v = x * 16384.0f;
  if (v != v) return 0;
  if (v >= 32767.0f) return 32767;
  if (v <= -32768.0f) return -32768;
  return (int)v;
}

// a lane's samples [i0, i0 + 8) of a row of n; 0 beyond the row.  vec: the row is 16-B aligned
__device__ __forceinline__ void load8(const float* __restrict__ row, int64_t i0, int len, bool vec, float (&v)[IIR_ITEMS]) {
  if (vec && len == IIR_ITEMS) {
    const f4v a = *reinterpret_cast<const f4v*>(row + i0), b = *reinterpret_cast<const f4v*>(row + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < IIR_ITEMS; ++j) v[j] = j < len ? row[i0 + j] : 0.f;
  }
}
__device__ __forceinline__ void store8(float* __restrict__ row, int64_t i0, int len, bool vec, const float (&v)[IIR_ITEMS]) {
  if (vec && len == IIR_ITEMS) {
    *reinterpret_cast<f4v*>(row + i0) = f4v{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f4v*>(row + i0 + 4) = f4v{v[4], v[5], v[6], v[7]};
  } else {
#pragma unroll
    for (int j = 0; j < IIR_ITEMS; ++j)
      if (j < len) row[i0 + j] = v[j];
  }
}

// One tile of one row.  The lane's zero-state run (y0, end state z), then the state entering
// the lane: the exclusive scan of the lanes' end states with the tile's entering state
// *cin folded in (LDS, written by one lane before the call and read after the barrier here: a
// zf that aliases zi is stored only after zi has been read; NULL: 0).  tab[k] = p^(8 k).  Lanes past the row's end hold values nothing reads
// (the scan only moves state towards later samples).  Returns the lane's entering state.
__device__ __forceinline__ double tile_scan(const float (&x)[IIR_ITEMS], int len, double b0, double b1, double a1,
                                            const double* __restrict__ tab, const double* cin, double* wagg, int tid,
                                            double (&y0)[IIR_ITEMS], double* z_end, double* tile_end) {
  const int lane = tid & 63, wv = tid >> 6;
  double z = 0.0;
#pragma unroll
  for (int j = 0; j < IIR_ITEMS; ++j)
    if (j < len) {
      const double y = b0 * (double)x[j] + z;
      z = b1 * (double)x[j] - a1 * y;
      y0[j] = y;
    }
  *z_end = z;
  double v = z;                         // inclusive: the state after lanes [.., lane] from zero
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int o = 1 << k;
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v = tab[o] * u + v;
  }
  if (lane == 63) wagg[wv] = v;
  __syncthreads();
  double c = cin != nullptr ? *cin : 0.0;   // the state entering this wave
#pragma unroll
  for (int w = 0; w < IIR_NW; ++w)
    if (w < wv) c = tab[64] * c + wagg[w];
  if (tile_end != nullptr && tid == IIR_T - 1) *tile_end = tab[64] * c + v;
  double e = __shfl_up(v, 1, 64);
  if (lane == 0) e = 0.0;
  return e + tab[lane] * c;
}

struct RowSel {
  const float* x; float* y; int64_t si;   // the row's input, output (nullable) and state index
};
__device__ __forceinline__ RowSel row_of(const IirLaunch& a, int s, int ch) {
  RowSel r;
  r.x = a.x[ch] + (int64_t)s * a.x_stride;
  r.y = a.y[ch] != nullptr ? a.y[ch] + (int64_t)s * a.y_stride : nullptr;
  r.si = (int64_t)s * a.st_stride + ch;
  return r;
}

// BLEND: a lane's 8 samples of both channels (right unused with nch == 1) through the stream's
// gain ramp gn = {g0, g1, m0, m1} (IirLaunch::gains), in f64 and rounded once.  reduce and apply
// both form their samples here, so both see the same f32 values.
__device__ __forceinline__ void blend8(const double* __restrict__ gn, int64_t i0, int64_t n, int nch, float (&l)[IIR_ITEMS],
                                       float (&r)[IIR_ITEMS]) {
  const double g0 = gn[0], dg = gn[1] - g0, m0 = gn[2], dm = gn[3] - m0, dn = (double)n;
  double g[IIR_ITEMS], m[IIR_ITEMS];
#pragma unroll
  for (int j = 0; j < IIR_ITEMS; ++j) {
    const double t = (double)(i0 + j + 1) / dn;
    g[j] = g0 + dg * t;
    m[j] = m0 + dm * t;
  }
  if (nch == 2) {
#pragma unroll
    for (int j = 0; j < IIR_ITEMS; ++j) {
      const double mid = ((double)l[j] + (double)r[j]) / 2.0, side = ((double)l[j] - (double)r[j]) / 2.0;
      l[j] = (float)(m[j] * (mid + g[j] * side));
      r[j] = (float)(m[j] * (mid - g[j] * side));
    }
  } else {
#pragma unroll
    for (int j = 0; j < IIR_ITEMS; ++j) l[j] = (float)(m[j] * (double)l[j]);
  }
}

// reduce: the zero-state end state of every tile but each row's last -> agg[row][tile]
template <bool BLEND>
__global__ __launch_bounds__(IIR_T) void iir1_reduce_kernel(const IirLaunch a) {
  __shared__ double wagg[2][IIR_NW];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int64_t tile = blockIdx.x, i0 = tile * IIR_TILE + (int64_t)tid * IIR_ITEMS;   // full tiles only
  float xs[2][IIR_ITEMS];               // both channels' loads in flight before the first scan
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
    if (ch < a.nch) load8(row_of(a, s, ch).x, i0, IIR_ITEMS, a.vec_x != 0, xs[ch]);
  if (BLEND) blend8(a.gains + 4 * (int64_t)s, i0, a.n, a.nch, xs[0], xs[1]);
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    if (ch >= a.nch) break;
    const float (&x)[IIR_ITEMS] = xs[ch];
    double y0[IIR_ITEMS], z_end, t_end = 0.0;
    (void)tile_scan(x, IIR_ITEMS, a.b0, a.b1, a.a1, a.tab, nullptr, wagg[ch], tid, y0, &z_end, &t_end);
    if (tid == IIR_T - 1) a.agg[((int64_t)s * a.nch + ch) * a.ntiles + tile] = t_end;
  }
}

// carry: per row one wave; lane l chains the tiles [l K, (l + 1) K) from zero (lane 0: from zi),
// the lanes are scanned with q[k] = p^(TILE K 2^k), and a second pass over the lane's tiles
// stores the state entering each.  agg of a row's last tile does not exist and is not read.
// (The two passes instead of a stored prefix: the scan needs each lane's end state first.)
__global__ __launch_bounds__(64) void iir1_carry_kernel(const IirLaunch a) {
  const int lane = threadIdx.x, row = blockIdx.x;
  const int s = row / a.nch, ch = row - s * a.nch;
  const double zi = a.zi != nullptr ? a.zi[(int64_t)s * a.st_stride + ch] : 0.0;
  const double pt = a.tab[IIR_T];
  const double* __restrict__ agg = a.agg + (int64_t)row * a.ntiles;
  double* __restrict__ carry = a.carry + (int64_t)row * a.ntiles;
  const int64_t k0 = (int64_t)lane * a.K, k1 = k0 + a.K < a.ntiles ? k0 + a.K : a.ntiles;
  // up to CARRY_R tiles per lane (rows of up to 64 CARRY_R tiles): their end states in registers,
  // the loads in flight together; longer rows read them in both passes
  constexpr int CARRY_R = 8;
  const bool regs = a.K <= CARRY_R;
  double ag[CARRY_R];
  bool on[CARRY_R];
#pragma unroll
  for (int j = 0; j < CARRY_R; ++j) {
    on[j] = regs && k0 + j < k1 && k0 + j < a.ntiles - 1;
    ag[j] = on[j] ? agg[k0 + j] : 0.0;
  }
  double z = lane == 0 ? zi : 0.0;
  if (regs) {
#pragma unroll
    for (int j = 0; j < CARRY_R; ++j)
      if (on[j]) z = pt * z + ag[j];
  } else {
    for (int64_t k = k0; k < k1; ++k)
      if (k < a.ntiles - 1) z = pt * z + agg[k];
  }
  double v = z;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int o = 1 << k;
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v = a.q[k] * u + v;
  }
  z = __shfl_up(v, 1, 64);
  if (lane == 0) z = zi;
  if (regs) {
#pragma unroll
    for (int j = 0; j < CARRY_R; ++j) {
      if (k0 + j < k1) carry[k0 + j] = z;
      if (on[j]) z = pt * z + ag[j];
    }
  } else {
    for (int64_t k = k0; k < k1; ++k) {
      carry[k] = z;
      if (k < a.ntiles - 1) z = pt * z + agg[k];
    }
  }
}

// apply: every tile from its entering state -> the f32 rows, the interleaved PCM, the end states
template <bool BLEND>
__global__ __launch_bounds__(IIR_T) void iir1_apply_kernel(const IirLaunch a) {
  __shared__ double wagg[2][IIR_NW], cin[2];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int64_t tile = blockIdx.x, i0 = tile * IIR_TILE + (int64_t)tid * IIR_ITEMS;
  const int64_t left = a.n - i0;
  const int len = left >= IIR_ITEMS ? IIR_ITEMS : left > 0 ? (int)left : 0;
  unsigned pc[IIR_ITEMS];               // PCM: left in the low half, right in the high half
#pragma unroll
  for (int j = 0; j < IIR_ITEMS; ++j) pc[j] = 0u;
  float xs[2][IIR_ITEMS];               // both channels' loads in flight before the first scan
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
    if (ch < a.nch) load8(row_of(a, s, ch).x, i0, len, a.vec_x != 0, xs[ch]);
  if (BLEND) blend8(a.gains + 4 * (int64_t)s, i0, a.n, a.nch, xs[0], xs[1]);
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    if (ch >= a.nch) break;
    const RowSel r = row_of(a, s, ch);
    const float (&x)[IIR_ITEMS] = xs[ch];
    float yf[IIR_ITEMS];
    if (a.filter) {
      // the state entering the tile: the carry launch's, or zi itself for rows of one tile
      if (tid == 0) {
        double c = 0.0;
        if (a.ntiles > 1) c = a.carry[((int64_t)s * a.nch + ch) * a.ntiles + tile];
        else if (a.zi != nullptr) c = a.zi[r.si];
        cin[ch] = c;
      }
      double y0[IIR_ITEMS], z_end;
      const double z_in = tile_scan(x, len, a.b0, a.b1, a.a1, a.tab, &cin[ch], wagg[ch], tid, y0, &z_end, nullptr);
      const double p = -a.a1;
      double pw = 1.0;
#pragma unroll
      for (int j = 0; j < IIR_ITEMS; ++j)
        if (j < len) {
          yf[j] = (float)(y0[j] + pw * z_in);
          pw *= p;
        }
      if (a.zf != nullptr && len > 0 && i0 + len == a.n) a.zf[r.si] = z_end + pw * z_in;
    } else {
#pragma unroll
      for (int j = 0; j < IIR_ITEMS; ++j) yf[j] = x[j];
    }
    if (r.y != nullptr) store8(r.y, i0, len, a.vec_y != 0, yf);
    if (a.pcm != nullptr) {
#pragma unroll
      for (int j = 0; j < IIR_ITEMS; ++j) {
        const unsigned v = (unsigned)pcm16(yf[j]) & 0xffffu;
        pc[j] |= a.nch == 1 ? (v | (v << 16)) : (v << (16 * ch));
      }
    }
  }
  if (a.pcm != nullptr) {
    int16_t* __restrict__ prow = a.pcm + (int64_t)s * a.pcm_stride;
    if (a.vec_pcm && len == IIR_ITEMS) {
      unsigned* q = reinterpret_cast<unsigned*>(prow + 2 * i0);
      *reinterpret_cast<uint4*>(q) = uint4{pc[0], pc[1], pc[2], pc[3]};
      *reinterpret_cast<uint4*>(q + 4) = uint4{pc[4], pc[5], pc[6], pc[7]};
    } else {
#pragma unroll
      for (int j = 0; j < IIR_ITEMS; ++j)
        if (j < len) {
          prow[2 * (i0 + j)] = (int16_t)(pc[j] & 0xffffu);
          prow[2 * (i0 + j) + 1] = (int16_t)(pc[j] >> 16);
        }
    }
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void sdr_iir1_table(double a1, double* tab) {
  const double p = -a1;
  for (int k = 0; k <= SDR_IIR_THREADS; ++k) tab[k] = std::pow(p, (double)(SDR_IIR_ITEMS * k));
}

int64_t sdr_iir1_tiles(int64_t n) { return (n + IIR_TILE - 1) / IIR_TILE; }

hipError_t sdr_launch_iir1(const IirLaunch& in, hipStream_t st) {
  IirLaunch a = in;
  if (a.n < 1 || a.nstreams < 1 || a.nstreams > 65535 || a.nch < 1 || a.nch > 2 || a.x[0] == nullptr ||
      (a.nch == 2 && a.x[1] == nullptr) || (a.filter && a.tab == nullptr))
    return hipErrorInvalidValue;
  a.ntiles = sdr_iir1_tiles(a.n);
  if (a.ntiles > 0x7fffffff) return hipErrorInvalidValue;
  a.vec_x = a.x_stride % 4 == 0 && al16(a.x[0]) && (a.nch == 1 || al16(a.x[1]));
  a.vec_y = a.y_stride % 4 == 0 && (a.y[0] == nullptr || al16(a.y[0])) && (a.y[1] == nullptr || al16(a.y[1]));
  a.vec_pcm = a.pcm != nullptr && al16(a.pcm) && a.pcm_stride % 8 == 0;
  const dim3 blk(IIR_T);
  const bool blend = a.gains != nullptr;
  if (a.filter && a.ntiles > 1) {
    if (a.agg == nullptr || a.carry == nullptr) return hipErrorInvalidValue;
    a.K = (a.ntiles + 63) / 64;
    const double p = -a.a1;
    for (int k = 0; k < 6; ++k) a.q[k] = std::pow(p, (double)IIR_TILE * (double)a.K * (double)(1 << k));
    hipLaunchKernelGGL(blend ? iir1_reduce_kernel<true> : iir1_reduce_kernel<false>,
                       dim3((unsigned)(a.ntiles - 1), (unsigned)a.nstreams), blk, 0, st, a);
    hipLaunchKernelGGL(iir1_carry_kernel, dim3((unsigned)(a.nstreams * a.nch)), dim3(64), 0, st, a);
  }
  hipLaunchKernelGGL(blend ? iir1_apply_kernel<true> : iir1_apply_kernel<false>, dim3((unsigned)a.ntiles, (unsigned)a.nstreams),
                     blk, 0, st, a);
  return hipGetLastError();
}
