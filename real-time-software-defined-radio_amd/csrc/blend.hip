// Quality and gain control: every stream's MPX quality (blocks.py mpx_quality's definition, in
// f64) from its one-sided power spectrum, and from it the stereo-blend and mute gains the audio
// output stage (audio.hip, BLEND) ramps over the next block.  One launch per update, one wave per
// stream; nothing leaves the device.
//
// A subcarrier's ratio is sum(band) / (median(guard) x bins in band) in dB.  The median is numpy's:
// the middle value of the sorted guard, or the mean of the two middle values.  It is found by rank
// counting: the guard (at most SDR_BLEND_MAX_GUARD bins, a few hundred in practice) is staged in
// LDS, every lane counts for its bins how many others sort before them (ties broken by index, so
// the ranks are a permutation), and the lanes that hold the middle ranks publish their values.  A
// NaN in the guard gives a NaN floor, as np.median does; everything else is what IEEE arithmetic
// gives (a zero floor: +inf dB, 0 / 0: NaN).
#include <hip/hip_runtime.h>

#include <cmath>

#include "sdr_launch.h"

namespace {

constexpr int MAXG = SDR_BLEND_MAX_GUARD;

// sum of row[b0 .. b1) in f64: lane-strided partial sums, then the butterfly
__device__ __forceinline__ double band_sum(const float* __restrict__ row, int b0, int b1, int lane) {
  double acc = 0.0;
  for (int k = b0 + lane; k < b1; k += 64) acc += (double)row[k];
  return wave_sum(acc);
}

// np.median of the bins of up to two ranges of row (count = n0 + n1 <= MAXG, >= 1)
__device__ __forceinline__ double guard_median(const float* __restrict__ row, const int (&rg)[2][2], float* g, double* mid,
                                               int lane) {
  const int n0 = rg[0][1] - rg[0][0], n = n0 + rg[1][1] - rg[1][0];
  bool nan = false;
  for (int i = lane; i < n; i += 64) {
    const float v = i < n0 ? row[rg[0][0] + i] : row[rg[1][0] + (i - n0)];
    g[i] = v;
    nan |= v != v;
  }
  __syncthreads();
  const int lo = (n - 1) / 2, hi = n / 2;
  for (int i = lane; i < n; i += 64) {
    const float v = g[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float u = g[j];
      rank += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    if (rank == lo) mid[0] = (double)v;
    if (rank == hi) mid[1] = (double)v;
  }
  __syncthreads();
  const double m = lo == hi ? mid[0] : (mid[0] + mid[1]) / 2.0;
  const bool any_nan = __any(nan ? 1 : 0) != 0;
  __syncthreads();                        // g and mid are reused by the next band
  return any_nan ? __builtin_nan("") : m;
}

__device__ __forceinline__ double clip01(double x) { return x != x ? 0.0 : x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x; }
__device__ __forceinline__ double smooth(double cur, double target, double attack, double release) {
  return cur + (target < cur ? attack : release) * (target - cur);
}

__global__ __launch_bounds__(64) void blend_update_kernel(const BlendLaunch a) {
  __shared__ float g[MAXG];
  __shared__ double mid[2];
  const int lane = threadIdx.x, s = blockIdx.x;
  const float* __restrict__ row = a.power + (int64_t)s * a.stride;
  double db[2], floor0 = 0.0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {            // 0: pilot, 1: RDS
    const double sum = band_sum(row, a.bd.band[b][0], a.bd.band[b][1], lane);
    const double fl = guard_median(row, a.bd.guard[b], g, mid, lane);
    if (b == 0) floor0 = fl;
    db[b] = 10.0 * log10(sum / (fl * (double)(a.bd.band[b][1] - a.bd.band[b][0])));
  }
  if (lane != 0) return;
  double* __restrict__ st = a.state + (int64_t)s * SDR_BLEND_NSTATE;
  double* __restrict__ gn = a.gains + (int64_t)s * 4;
  const double tg = clip01((db[0] - a.blend_lo) / (a.blend_hi - a.blend_lo));
  const double tm = a.mute ? clip01((a.mute_hi - 10.0 * log10(floor0)) / (a.mute_hi - a.mute_lo)) : 1.0;
  const double g0 = st[4], m0 = st[6];
  const double g1 = smooth(g0, tg, a.attack, a.release);
  const double m1 = a.mute ? smooth(m0, tm, a.attack, a.release) : 1.0;
  st[0] = db[0]; st[1] = db[1]; st[2] = floor0;
  st[3] = g0; st[4] = g1; st[5] = m0; st[6] = m1;
  st[7] += 1.0;
  gn[0] = g0; gn[1] = g1; gn[2] = m0; gn[3] = m1;
}

// the state after a reset: mono until a pilot has been seen, silent until the floor has been (mute on)
__global__ __launch_bounds__(64) void blend_reset_kernel(double* __restrict__ state, double* __restrict__ gains, int nstreams,
                                                         int mute) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nstreams) return;
  const double m = mute ? 0.0 : 1.0;
  double* st = state + (int64_t)s * SDR_BLEND_NSTATE;
#pragma unroll
  for (int k = 0; k < SDR_BLEND_NSTATE; ++k) st[k] = (k == 5 || k == 6) ? m : 0.0;
  double* gn = gains + (int64_t)s * 4;
  gn[0] = 0.0; gn[1] = 0.0; gn[2] = m; gn[3] = m;
}

}  // namespace

// the bins of mpx_quality's bands and guards for nbins = nfft / 2 + 1 bins at fs (host): a bin
// belongs to a band if its centre k (fs / nfft) lies in the closed interval
bool sdr_blend_bands(double fs, int nbins, BlendBands* out) {
  const double df = fs / (double)(2 * (nbins - 1));
  auto range = [&](double lo, double hi, int (&r)[2]) {
    r[0] = r[1] = 0;
    bool open = false;
    for (int k = 0; k < nbins; ++k) {
      const double f = (double)k * df;
      if (f >= lo && f <= hi) {
        if (!open) r[0] = k;
        open = true;
        r[1] = k + 1;
      }
    }
  };
  range(18.5e3, 19.5e3, out->band[0]);
  range(16e3, 18e3, out->guard[0][0]);
  range(20e3, 22e3, out->guard[0][1]);
  range(55e3, 59e3, out->band[1]);
  range(60e3, 64e3, out->guard[1][0]);
  out->guard[1][1][0] = out->guard[1][1][1] = 0;
  for (int b = 0; b < 2; ++b) {
    const int ng = (out->guard[b][0][1] - out->guard[b][0][0]) + (out->guard[b][1][1] - out->guard[b][1][0]);
    if (ng < 1 || ng > SDR_BLEND_MAX_GUARD || out->band[b][1] <= out->band[b][0]) return false;
  }
  return true;
}

hipError_t sdr_launch_blend_update(const BlendLaunch& a, hipStream_t st) {
  if (a.power == nullptr || a.state == nullptr || a.gains == nullptr || a.nstreams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(blend_update_kernel, dim3((unsigned)a.nstreams), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t sdr_launch_blend_reset(double* state, double* gains, int nstreams, int mute, hipStream_t st) {
  if (state == nullptr || gains == nullptr || nstreams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(blend_reset_kernel, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, st, state, gains, nstreams, mute);
  return hipGetLastError();
}
