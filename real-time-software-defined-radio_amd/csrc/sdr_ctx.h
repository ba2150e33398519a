// Host-side internals of a libsdr context, shared by the C-ABI translation units
// (capi.hip: the per-call entry points; rx.hip: the multi-stream block receiver, whose stage
// kernels are rx_stage.hip and do not see a context).
// Not part of the public ABI (include/sdr.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <list>
#include <string>
#include <vector>

#include "sdr_launch.h"
#include "../../include/sdr.h"

namespace sdrint {

// scratch slots owned by a context (grown on demand, never shrunk)
enum Slot {
  S_IN, S_IN2, S_OUT, S_OUT2, S_OUT3, S_OUT4, S_STATE, S_STATE2, S_MISC, S_THETA, S_PHI, S_WRAP,
  S_PSD, S_PLLW, S_IIR, S_SPEC,
  S_NSLOT
};

struct TapSet {
  std::vector<double> b;
  TapsF32 h;
  bool sym = false;           // T <= SDR_MAX_TAPS and the f32 taps mirror-equal (linear phase: every firwin design)
  float* dev_f32 = nullptr;   // [0, cap): the taps; then, from dev_rev - 1: 0, the taps reversed, 0, 0
  float* dev_rev = nullptr;   // dev_rev[j] = h[T-1-j], dev_rev[-1] = dev_rev[T] = 0 (packed FIR tiles)
  double* dev_f64 = nullptr;
  int* dev_afr = nullptr;     // T = 101 / 151: the u8 MFMA front end's A fragments (fe_mfma.hip)
};

// a PLL loop's table on the device: the response table (sdr_pll_resp_table) per (Kp, Ki,
// pseudo-block length), or the solve's matrix powers (qtab_host) per (Kp, Ki) with pb = 0
struct PllTable {
  double kp = 0.0, ki = 0.0;
  int64_t pb = 0;
  double* dev = nullptr;
};

// a first-order section's pole-power table on the device (sdr_iir1_table), per a1
struct IirTab {
  double a1 = 0.0;
  double* dev = nullptr;
};

// a second-order cascade's power tables on the device (sos.hip sos_table), per coefficient set
struct SosTab {
  int K = 0;
  double sos[SDR_SOS_MAX_SECTIONS * 6] = {};
  double* dev = nullptr;
};

// the calling thread's last error message; returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace sdrint

struct sdr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  void* slot[sdrint::S_NSLOT] = {};
  size_t cap[sdrint::S_NSLOT] = {};
  // uploaded tap sets (taps are designed once), least recently used first.  A list: a hit
  // is spliced to the back and an overflow evicts the front, so no pointer handed out by
  // a lookup is invalidated by the other lookups of the same entry point (<= 4 per call).
  std::list<sdrint::TapSet> taps;
  // PLL response tables of the long calls made on the context, and the matrix-power tables of
  // its long and spec-only calls: least recently used first, bounded like the tap sets
  std::list<sdrint::PllTable> resp, qtab;
  // pole-power tables of the first-order sections run on the context (a few; never evicted)
  std::list<sdrint::IirTab> iir;
  // power tables of the second-order cascades made on the context (a few; never evicted)
  std::list<sdrint::SosTab> sos;
  // PLL solve counters (SDR_PLL_NSTATS, device; sdr_pll_stats): every PLL launch of the
  // context and of its receivers adds to them
  unsigned long long* pll_stats = nullptr;
};

namespace sdrint {

int set_dev(sdr_ctx* c);
// context scratch slot `s` of at least `bytes` (synchronises the stream when it grows)
int scratch(sdr_ctx* c, Slot s, size_t bytes, void** out);
// device copies (f32, f64) of the tap set b[0..T) (cached per context).  max_T: SDR_MAX_TAPS
// for the FIR kernels, up to SDR_MAX_RESAMPLE_TAPS for the resampler.
int get_taps(sdr_ctx* c, const double* b, int T, const TapSet** out, int max_T = SDR_MAX_TAPS);

// the device response table of loop cfg for a long call of n steps (cached per context);
// *out = NULL when n is not a long call
int get_resp(sdr_ctx* c, const PllCfg& cfg, int64_t n, const double** out);
// the f32 copy get_resp stores after a table of pseudo-block length pb (2 (pb + 5) doubles)
inline const float* resp32_of(const double* resp, int64_t pb) {
  return resp != nullptr ? reinterpret_cast<const float*>(resp + 2 * (pb + 5)) : nullptr;
}
// the device matrix-power table of loop cfg (PllJob::qtab; cached per context)
int get_qtab(sdr_ctx* c, const PllCfg& cfg, const double** out);

// the device pole-power table of a first-order section with denominator [1, a1] (cached per context)
int get_iir_tab(sdr_ctx* c, double a1, const double** out);
// validates the section (finite b, a1, |a1| <= 1), fills a.b0 / b1 / a1 / filter / tab and the
// tile scratch (context slot S_IIR) and launches the stage on the context stream; b == NULL: no
// filter.  `what` names the entry point in error messages.
int run_iir1(sdr_ctx* c, IirLaunch& a, const double* b, double a1, const char* what);

// sdr_blend_params' rules (include/sdr.h): *out = the parameters with NULL's defaults filled in,
// *mute_on = both mute limits finite; `what` names the entry point in error messages
int blend_params(const sdr_blend_params* params, sdr_blend_params* out, bool* mute_on, const char* what);

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr double two_pi = 6.283185307179586476925286766559;

}  // namespace sdrint

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return sdrint::fail(SDR_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define TRY(expr)                 \
  do {                            \
    int r_ = (expr);              \
    if (r_ != SDR_OK) return r_;  \
  } while (0)

#define CHECK_CTX(c) \
  if ((c) == nullptr) return sdrint::fail(SDR_EINVAL, "context is NULL")
#define CHECK_RX(r) \
  if ((r) == nullptr) return sdrint::fail(SDR_EINVAL, "sdr_rx is NULL")

// ---- what the row blocks' entry points share (ddc, pfb, rsmp, spectrum) ------------------------
namespace sdrint {

inline int taps_finite(const double* b, int taps, const char* what) {
  for (int j = 0; j < taps; ++j)
    if (!std::isfinite(b[j])) return fail(SDR_EINVAL, "%s: tap %d is not finite", what, j);
  return SDR_OK;
}

// the call-time rules of a decimating block (an object with a decimation D), for host and device
// buffers alike
template <class Obj>
int decim_check_call(const Obj* d, const void* iq, int64_t n, const float* out, int64_t out_stride, const char* what) {
  if (d == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (iq == nullptr || out == nullptr) return fail(SDR_EINVAL, "%s: iq or out is NULL", what);
  if (n < 1 || n % d->D != 0) return fail(SDR_EINVAL, "%s: n=%lld must be >= 1 and a multiple of decim=%d", what, (long long)n, d->D);
  if (out_stride < n / d->D)
    return fail(SDR_EINVAL, "%s: out_stride=%lld < n/decim=%lld", what, (long long)out_stride, (long long)(n / d->D));
  return SDR_OK;
}

// a device copy of host[0..count), for a create's error chain (the host array is read until the
// stream is synchronised)
template <class T>
hipError_t upload(T** dev, const T* host, size_t count, hipStream_t st) {
  const hipError_t e = hipMalloc(dev, count * sizeof(T));
  return e != hipSuccess ? e : hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, st);
}
// how a create's error chain ends
inline int create_failed(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? SDR_ENOMEM : SDR_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// The device arrays an object owns.  A create calls get() for each and looks at `err` once: the
// first failure stays there and the gets after it do nothing.  zero() clears the arrays that a
// reset clears; release() frees them all, after a partial failure as well.
struct DevMem {
  struct Item {
    void* p;
    size_t bytes;
    bool zeroed;
  };
  std::vector<Item> items;
  hipError_t err = hipSuccess;

  template <class T>
  void get(T** p, size_t count, bool zeroed_on_reset = false) {
    if (err != hipSuccess) return;
    err = hipMalloc(p, count * sizeof(T));
    if (err == hipSuccess) items.push_back(Item{*p, count * sizeof(T), zeroed_on_reset});
  }
  // an array in each of two slots: a call reads slot[cur] and fills the other (rds_seg.h SegCursor)
  template <class T>
  void get2(T* (&slot)[2], size_t count, bool zeroed_on_reset = false) {
    get(&slot[0], count, zeroed_on_reset);
    get(&slot[1], count, zeroed_on_reset);
  }
  hipError_t zero(hipStream_t st) const {
    hipError_t e = hipSuccess;
    for (const Item& it : items)
      if (it.zeroed && e == hipSuccess) e = hipMemsetAsync(it.p, 0, it.bytes, st);
    return e;
  }
  void release() {
    for (const Item& it : items) (void)hipFree(it.p);
    items.clear();
  }
};

// A work array that grows to the largest call: at least `need` elements after fit().  Growing
// waits for the calls in flight on `st`, which may still read the old array.
template <class T>
struct GrowMem {
  T* p = nullptr;
  size_t cap = 0;   // elements
  int fit(size_t need, hipStream_t st, const char* what) {
    if (need <= cap) return SDR_OK;
    HIP_TRY(hipStreamSynchronize(st));
    release();
    const hipError_t e = hipMalloc(&p, need * sizeof(T));
    if (e != hipSuccess) return create_failed(e, what);
    cap = need;
    return SDR_OK;
  }
  void release() {
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// HIP events around the N launches (stages) of a call: mark(k) in front of stage k, mark(N) behind
// the last.  Off until enable(true), which creates the events.
template <int N>
struct StageTimer {
  bool on = false, timed = false;   // timed: a call has been marked to its end
  hipEvent_t ev[N + 1] = {};
  ~StageTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t enable(bool want) {
    if (want && !ev[0])
      for (hipEvent_t& e : ev) {
        const hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) return err;
      }
    on = want;
    return hipSuccess;
  }
  hipError_t mark(int k, hipStream_t st) {
    if (!on) return hipSuccess;
    const hipError_t err = hipEventRecord(ev[k], st);
    if (k == N && err == hipSuccess) timed = true;
    return err;
  }
  // ms[0..N) of the latest call marked to its end, after waiting for it; `refusal` is the error
  // text where there is none
  int elapsed(float* ms, const char* refusal) {
    if (!on || !timed) return fail(SDR_EINVAL, "%s", refusal);
    HIP_TRY(hipEventSynchronize(ev[N]));
    for (int k = 0; k < N; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    return SDR_OK;
  }
};

// The call-time rules of a pass over a capture block (iqc, ingest): n complex samples of es bytes
// at `raw` -- `name` in the messages -- to n complex f32 at out.  es = 0: host buffers, which need
// no alignment and are staged apart.  in_place_ok: out == raw is the one overlap allowed.
inline int capture_check_call(const char* what, const void* obj, const char* name, const void* raw, int es, int64_t n, const float* out,
                              bool in_place_ok) {
  if (obj == nullptr) return fail(SDR_EINVAL, "%s: object is NULL", what);
  if (raw == nullptr || out == nullptr) return fail(SDR_EINVAL, "%s: %s or out is NULL", what, name);
  if (n < 1 || n > INT32_MAX) return fail(SDR_EINVAL, "%s: n=%lld outside [1, 2^31 - 1]", what, (long long)n);
  if (es == 0) return SDR_OK;
  const uintptr_t a0 = (uintptr_t)raw, a1 = a0 + (uintptr_t)n * es, o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n * 8;
  if ((a0 & (es - 1)) != 0 || (o0 & 7) != 0)
    return fail(SDR_EINVAL, "%s: %s must be aligned to one complex sample (%d B) and out to 8 B", what, name, es);
  if (a0 < o1 && o0 < a1 && !(in_place_ok && a0 == o0))
    return fail(SDR_EINVAL, "%s: %s and out overlap (only out == %s of an f32 object may)", what, name, name);
  return SDR_OK;
}

// count elements of a device array on the host, after waiting for the calls in flight
template <class T>
int fetch(sdr_ctx* c, const T* dev, size_t count, T* host) {
  TRY(set_dev(c));
  HIP_TRY(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}
// an object's per-stream struct array
template <class T>
int fetch_states(sdr_ctx* c, const T* dev, int nstreams, std::vector<T>* out) {
  out->resize((size_t)nstreams);
  return fetch(c, dev, out->size(), out->data());
}

// rows of row_bytes bytes each; on the host `pitch` bytes apart, packed on the device
struct HostRows {
  size_t rows, row_bytes, pitch;
};
// A synchronous host call of a block: the input rows to context slot S_IN, call(din, dout) -- the
// block's process_dev on packed rows --, the output rows back from S_OUT (out_host NULL: the block
// has none, dout is NULL), one wait.
template <class F>
int run_staged(sdr_ctx* c, const void* in_host, HostRows in, void* out_host, HostRows out, F&& call) {
  void *din = nullptr, *dout = nullptr;
  TRY(scratch(c, S_IN, in.rows * in.row_bytes, &din));
  if (out_host != nullptr) TRY(scratch(c, S_OUT, out.rows * out.row_bytes, &dout));
  if (in.rows == 1)
    HIP_TRY(hipMemcpyAsync(din, in_host, in.row_bytes, hipMemcpyHostToDevice, c->stream));
  else
    HIP_TRY(hipMemcpy2DAsync(din, in.row_bytes, in_host, in.pitch, in.row_bytes, in.rows, hipMemcpyHostToDevice, c->stream));
  TRY(call(din, dout));
  if (out_host != nullptr)
    HIP_TRY(hipMemcpy2DAsync(out_host, out.pitch, dout, out.row_bytes, out.row_bytes, out.rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

}  // namespace sdrint
