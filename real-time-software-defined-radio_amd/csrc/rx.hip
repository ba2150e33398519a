// Multi-stream block receiver (sdr_rx_*): the per-block loops of model/fmMonoBlock.py:80-173
// (mono + stereo) and model/fmRDSblock.py:127-204 (RDS up to the RRC output) for S
// independent streams at once, every state and intermediate resident in HBM.  This is
// SURVEY §8a C5 (8 streams, mono + stereo + RDS, B = 153 600, src/fm_radio.cpp:783-792 runs
// the same stages as four threads per stream) and the per-block drop-in path of C3/C4.
//
// One block of all S streams is a fixed chain of launches (rx_front, rx_pll, rx_back): FE (RF FIR +
// decimate + demod, fe.hip); stage A (every filter that reads demod: one launch, one job table);
// B (RDS square + BPF); the stereo and RDS PLLs (pll.hip); C (the mixers + LPFs, the L/R combiner
// in the store); D (the RDS resamplers); E (RRC) -- 10 launches at full C5, whatever S is.  Every
// stage launch also carries its filters' lfilter final states (rx_stage.hip); zi and zf live in
// two state banks that swap every block, so no zf write races a zi read.
//
// Host code only: the stage kernels and their launch planning are rx_stage.hip (rx_stage.h); the
// tables of outputs, filters and state slots and the allocations' layout are rx_layout.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "rx_layout.h"
#include "rx_stage.h"
#include "sdr_ctx.h"

using namespace sdrint;
using namespace rxlayout;

namespace {

// What a receiver's blocks decide from its configuration alone (fixed once rx_finalize has run;
// the PLL loops' constants are not: sdr_rx_set_pll stays legal, so their tables are per call)
struct RxPlan {
  bool au, stx, rd;          // the flags: any audio, stereo, RDS
  bool span;                 // mm_span_ok(M): the rows are long enough for the matrix-core kernels
  bool codes;                // spans: the PLLs read sign codes that the pilot BPF's and the RDS x^2 + BPF's tiles store
  bool cres;                 // the RDS LPF + resampler as the composite filter
  bool tiles_ok;             // the stereo mixer's tiles can form the NCO from the phase rows (PRE_NCO)
  bool lng; int64_t pb; int nb;   // M is a long PLL call, of nb pseudo-blocks of pb samples
  bool th32[2];              // per loop: its phase rows in the compact form
};

}  // namespace

struct sdr_rx : RxLayout {             // M, A, R, the rows' lengths and strides, the regions: set by rx_finalize
  sdr_ctx* c = nullptr;
  int S = 0;
  int64_t B = 0;
  int u8 = 0, flags = 0;
  int rf_decim = 10, audio_decim = 5, rds_up = 19, rds_down = 80;
  std::vector<double> taps[SDR_RX_NFILTERS];
  PllCfg pll[2] = {};
  bool ready = false;
  RxPlan plan = {};
  float* out[SDR_RX_NOUTPUTS] = {};    // the rows of the latest block (one of outs[])
  float* outs[3][SDR_RX_NOUTPUTS] = {}; // row sets: nq when pipelined, else one
  void* mem = nullptr;                 // one allocation for outputs, states and phases; its regions (rx_layout.h Reg):
  double *bank[2] = {}, *phase = nullptr, *pll_state[2] = {};   // state banks; demod prev_phase; 6 per stream (stereo, RDS)
  int* wraps = nullptr;                // FE kernel scratch: per-block wrap count, last phase
  float* last_phi = nullptr;
  double *theta = nullptr, *pllc = nullptr;   // PLL phases / per-sample constants: 2 x S rows of ths / cst per row set
  int8_t* pcode = nullptr;             // spans: the PLLs' inputs as sign codes (pll_code): 2 x S rows per row set
  char* pllw = nullptr;                // long blocks (M > SDR_PLL_BLOCK_MAX): the PLL's records, per row set
  void* pin_in = nullptr;              // pinned host staging (sdr_rx_run)
  float* pin_out = nullptr;
  size_t pin_in_cap = 0, pin_out_cap = 0;
  float* mirror[SDR_RX_NOUTPUTS] = {};  // sdr_rx_run: pinned host rows (out_n apart) the producing
                                        // stage stores each requested output into, or null
  int parity = 0; int64_t blocks = 0;  // the state bank the next block reads; blocks since reset
  // sdr_rx_set_pipeline: block k's front half (FE, stage A) runs on `front` while block
  // k-1's back half (B, PLLs, C, D, E) runs on the context stream; row set k % nq
  int pipe = 0;
  hipStream_t last_fs = nullptr;        // the stream block k-1's front half ran on
  int64_t host_done = -1;               // the latest block the host has waited for (deliver)
  int nq = 2;                           // row sets when pipelined (3 with sdr_rx_set_depth >= 2)
  hipStream_t front = nullptr;          // FE, stages A and B
  hipStream_t mid = nullptr;            // the PLLs (prep, lanes, NCO)
  hipEvent_t ev_front[3] = {}, ev_mid[3] = {}, ev_back[3] = {}, ev_done[4] = {};
  hipEvent_t ev_read[3] = {};           // row set q's readers on the context stream (recorded by the next sdr_rx_process_dev)
  // sdr_rx_submit: depth blocks in flight before a submit waits (sdr_rx_set_depth); pinned
  // slots (input and outputs) per block, depth + 1 of them; the blocks in flight, oldest first
  int depth = 1; int64_t subs = 0;
  size_t in_slot = 0, out_slot = 0;
  struct Pending {
    int slot = 0, nout = 0;
    hipEvent_t ev = nullptr;           // the block's completion (ev_done[slot], or its row set's ev_back)
    int64_t blk = 0;                   // its index (sdr_rx::blocks numbering)
    int which[SDR_RX_MAXOUT] = {};
    float* out[SDR_RX_MAXOUT] = {};
    int64_t os[SDR_RX_MAXOUT] = {};
    size_t region[SDR_RX_NOUTPUTS] = {};
  } pq[4];                             // depth + 1 at most (the new block before k-depth leaves)
  int pq_head = 0, pq_n = 0;
  StageTimer<SDR_RX_NSTAGES> tm;       // events between the stages of each block (sdr_rx_set_timing)
  // outputs process_dev materialises (sdr_rx_set_keep; bit o = SDR_RX_O_o): the NCO rows and
  // the RDS LPF rows are intermediates the chain does not need (the mixers form the NCO from
  // the PLL phases, the RDS LPF runs inside the composite resampler)
  uint64_t keep = ~0ull, keep_now = ~0ull;   // keep_now: this call's (sdr_rx_submit: what it was asked for)
  bool made[SDR_RX_NOUTPUTS] = {};     // what the latest block materialised
  float* ctaps = nullptr;              // the composite RDS taps (rx_cres_kernel), device; null: two-stage path
  float* iq_f32 = nullptr;             // u8 blocks the tiled FE kernels cannot take, as f32 for the generic ones (rx_front)
  // sdr_rx_set_deemph: the audio output stage (audio.hip) after the combiner, on the context stream
  bool de_on = false;
  double de_b[2] = {}, de_a1 = 0.0;
  void* de_mem = nullptr;              // the states, then the PCM rows of every row set
  double* de_state = nullptr;          // [S][2]: left (mono without SDR_RX_STEREO), right
  double* de_mono = nullptr;           // [S]: the mono row of a stereo receiver
  int16_t *pcms[3] = {}, *pcm = nullptr;   // interleaved L R rows, pcm_stride int16 apart, per row set; the latest block's
  // sdr_rx_set_blend: the demod rows' spectra -> the gain control -> the audio tail's gains (blend.hip),
  // on the context stream directly before the tail; allocations of their own
  int bl_nfft = 0;                     // 0: off
  sdr_blend_params bl_prm = {};        // checked, defaults filled in
  sdr_rspec* bl_spec = nullptr;
  sdr_blend* bl = nullptr;
  float* bl_power = nullptr;           // [S][bl_nfft / 2 + 1]
  const double* bl_gains = nullptr;    // sdr_blend_gains_dev
};

namespace {

constexpr double kMpxFs = 240e3;     // the multiplex rate sdr_rx_set_blend's spectra assume (the PLLs' default Fs)

PllCfg pll_cfg(double freq, double fs, double scale, double adj, double bw) {
  return PllCfg{freq, fs, scale, adj, bw * 2.666, bw * bw * 3.555};   // model/fmPll.py:7-10
}

bool need_out(const sdr_rx* r, int o) { return produced(r->flags, r->de_on, o); }
bool filter_used(const sdr_rx* r, int f) { return group_on(r->flags, kFilter[f].group); }
// the setters that shape the allocations are legal until rx_finalize has run
int still_open(const sdr_rx* r, const char* what) {
  return r->ready ? fail(SDR_EINVAL, "%s: the receiver has processed a block", what) : SDR_OK;
}
template <class T>   // a region of an allocation as a T* (null when the configuration has none)
void at(void* base, Region rg, T** p) { *p = rg.off < 0 ? nullptr : reinterpret_cast<T*>(static_cast<char*>(base) + rg.off); }

RxPlan rx_plan(const sdr_rx* r) {
  RxPlan p{};
  p.au = group_on(r->flags, G_AUDIO);
  p.stx = group_on(r->flags, G_STEREO);
  p.rd = group_on(r->flags, G_RDS);
  p.span = mm_span_ok(r->M);
  // would launch_stage run filter f of output row `in` on the matrix cores, storing sign codes only?
  auto mm = [&](int f, int in, int pre) {            // (every row set is aligned alike)
    StageJob j{};
    j.kind = JK_FIR; j.D = 1; j.T = (int)r->taps[f].size(); j.pre = pre; j.n = r->M;
    j.x = r->outs[0][in]; j.x_stride = r->out_stride[in]; j.y8 = r->pcode;
    return mmable(j);
  };
  p.codes = (p.stx || p.rd) && r->pcode != nullptr && (!p.stx || mm(SDR_RX_F_PILOT, SDR_RX_O_DEMOD, PRE_NONE)) &&
            (!p.rd || mm(SDR_RX_F_RDS_SQUARE, SDR_RX_O_RDS_EXTRACT, PRE_SQUARE));
  p.cres = p.rd && r->ctaps != nullptr;
  const int tsl = p.stx ? (int)r->taps[SDR_RX_F_STEREO_LPF].size() : 151;
  p.tiles_ok = (tsl == 101 || tsl == 151) && (r->audio_decim == 1 || r->audio_decim == 5);
  p.lng = sdr_pll_long_geom(r->M, &p.pb, &p.nb);
  p.th32[0] = p.lng && p.pb % TH32_LINE == 0 && p.stx;
  p.th32[1] = p.lng && p.pb % TH32_LINE == 0 && p.rd;
  return p;
}

// Allocate and zero everything once the configuration is known (first block).
int rx_finalize(sdr_rx* r) {
  for (int f = 0; f < SDR_RX_NFILTERS; ++f)
    if (filter_used(r, f) && r->taps[f].empty())
      return fail(SDR_EINVAL, "sdr_rx: the %s filter taps are not set", kFilter[f].name);
  if (r->bl_nfft) {                    // (the setters after sdr_rx_set_blend may have undone what it checked)
    if (!r->de_on) return fail(SDR_EINVAL, "sdr_rx_set_blend: the audio output stage is off (sdr_rx_set_deemph)");
    if (ceil_div(r->B, r->rf_decim) < r->bl_nfft)
      return fail(SDR_EINVAL, "sdr_rx_set_blend: nfft %d > %lld demod samples per block", r->bl_nfft,
                  (long long)ceil_div(r->B, r->rf_decim));
  }
  RxGeom g{r->S, r->B, r->rf_decim, r->audio_decim, r->rds_up, r->rds_down, r->flags, r->de_on, r->pipe ? r->nq : 1, {}, 0};
  for (int f = 0; f < SDR_RX_NFILTERS; ++f) g.taps[f] = (int64_t)r->taps[f].size();
  g.pllw_bytes = sdr_pll_work_bytes(2, r->S, g.M());
  const RxLayout& L = static_cast<RxLayout&>(*r) = rx_layout(g);
  TRY(set_dev(r->c));
  hipError_t e = hipMalloc(&r->mem, (size_t)L.total);
  if (e != hipSuccess) return fail(SDR_ENOMEM, "sdr_rx: hipMalloc(%zu): %s", (size_t)L.total, hipGetErrorString(e));
  if ((uintptr_t)r->mem % 256 != 0) {                // (never: hipMalloc's alignment; pllw's offset relies on it)
    (void)hipFree(r->mem);
    r->mem = nullptr;
    return fail(SDR_EHIP, "sdr_rx: hipMalloc's base is not 256-B aligned");
  }
  for (int q = 0; q < g.nsets; ++q)
    for (int o = 0; o < SDR_RX_NOUTPUTS; ++o) at(r->mem, L.out_rg[q][o], &r->outs[q][o]);
  std::memcpy(r->out, r->outs[0], sizeof r->out);
  at(r->mem, L.reg[BANK0], &r->bank[0]); at(r->mem, L.reg[BANK1], &r->bank[1]);
  at(r->mem, L.reg[PHASE], &r->phase); at(r->mem, L.reg[WRAPS], &r->wraps); at(r->mem, L.reg[LAST_PHI], &r->last_phi);
  at(r->mem, L.reg[PLL_STATE0], &r->pll_state[0]); at(r->mem, L.reg[PLL_STATE1], &r->pll_state[1]);
  at(r->mem, L.reg[THETA], &r->theta); at(r->mem, L.reg[PLLC], &r->pllc);
  at(r->mem, L.reg[PLLW], &r->pllw); at(r->mem, L.reg[PCODE], &r->pcode);
  if (group_on(r->flags, G_RDS) && cres_covers(r->rds_up, r->rds_down)) {
    std::vector<float> ct;
    cres_taps(r->taps[SDR_RX_F_RDS_LPF], r->taps[SDR_RX_F_RDS_ANTI], &ct);
    if (!ct.empty()) {
      HIP_TRY(hipMalloc(&r->ctaps, sizeof(float) * ct.size()));
      HIP_TRY(hipMemcpy(r->ctaps, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice));
    }
  }
  if (r->de_on) {
    HIP_TRY(hipMalloc(&r->de_mem, (size_t)L.de_total));
    at(r->de_mem, L.reg[DE_STATE], &r->de_state); at(r->de_mem, L.reg[DE_MONO], &r->de_mono);
    for (int q = 0; q < g.nsets; ++q) at(r->de_mem, L.pcm_rg[q], &r->pcms[q]);
    r->pcm = r->pcms[0];
  }
  if (r->bl_nfft) {
    TRY(sdr_rspec_create(r->c, r->S, r->bl_nfft, nullptr, r->bl_nfft / 2, 0, &r->bl_spec));
    TRY(sdr_blend_create(r->c, r->S, &r->bl_prm, &r->bl));
    TRY(sdr_blend_gains_dev(r->bl, &r->bl_gains));
    HIP_TRY(hipMalloc(&r->bl_power, sizeof(float) * (size_t)r->S * (size_t)(r->bl_nfft / 2 + 1)));
  }
  r->plan = rx_plan(r);
  r->ready = true;
  return sdr_rx_reset(r);
}

}  // namespace

extern "C" {

int sdr_rx_create(sdr_ctx* c, int nstreams, int64_t block, int iq_dtype, int flags, sdr_rx** out) {
  CHECK_CTX(c);
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rx_create: out is NULL");
  *out = nullptr;
  if (nstreams < 1 || block < 1) return fail(SDR_EINVAL, "sdr_rx_create: nstreams %d, block %lld", nstreams, (long long)block);
  if (iq_dtype != SDR_IQ_F32 && iq_dtype != SDR_IQ_U8) return fail(SDR_EINVAL, "sdr_rx_create: iq_dtype %d", iq_dtype);
  if (flags & ~(SDR_RX_AUDIO | SDR_RX_STEREO | SDR_RX_RDS)) return fail(SDR_EINVAL, "sdr_rx_create: flags 0x%x", flags);
  sdr_rx* r = new (std::nothrow) sdr_rx();
  if (!r) return fail(SDR_ENOMEM, "sdr_rx_create: out of memory");
  r->c = c; r->S = nstreams; r->B = block;
  r->u8 = iq_dtype == SDR_IQ_U8; r->flags = flags;
  // model/fmMonoBlock.py:119 (19 kHz, x2, BW 0.01); model/fmRDSblock.py:167 (114 kHz, x0.5)
  r->pll[0] = pll_cfg(19e3, 240e3, 2.0, 0.0, 0.01);
  r->pll[1] = pll_cfg(114e3, 240e3, 0.5, M_PI / 3.3 - M_PI / 1.5, 0.001);
  *out = r;
  return SDR_OK;
}

void sdr_rx_destroy(sdr_rx* r) {
  if (r == nullptr) return;
  if (r->c) {
    (void)hipSetDevice(r->c->device);
    if (r->front) (void)hipStreamSynchronize(r->front);
    if (r->mid) (void)hipStreamSynchronize(r->mid);
    (void)hipStreamSynchronize(r->c->stream);
  }
  sdr_rspec_destroy(r->bl_spec);
  sdr_blend_destroy(r->bl);
  for (void* p : {r->mem, (void*)r->ctaps, (void*)r->iq_f32, r->de_mem, (void*)r->bl_power})
    if (p) (void)hipFree(p);
  for (void* p : {r->pin_in, (void*)r->pin_out})
    if (p) (void)hipHostFree(p);
  auto drop = [](auto& evs) { for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e); };
  drop(r->ev_front); drop(r->ev_mid); drop(r->ev_back); drop(r->ev_read); drop(r->ev_done);
  if (r->front) (void)hipStreamDestroy(r->front);
  if (r->mid) (void)hipStreamDestroy(r->mid);
  delete r;
}

int sdr_rx_set_filter(sdr_rx* r, int which, const double* b, int taps) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_filter"));
  if (which < 0 || which >= SDR_RX_NFILTERS) return fail(SDR_EINVAL, "sdr_rx_set_filter: filter %d", which);
  if (b == nullptr || taps < 1 || taps > SDR_MAX_TAPS)
    return fail(SDR_EINVAL, "sdr_rx_set_filter: taps=%d outside [1, %d]", taps, SDR_MAX_TAPS);
  r->taps[which].assign(b, b + taps);
  return SDR_OK;
}

int sdr_rx_set_decim(sdr_rx* r, int rf_decim, int audio_decim, int rds_up, int rds_down) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_decim"));
  if (rf_decim < 1 || audio_decim < 1 || rds_up < 1 || rds_down < 1) return fail(SDR_EINVAL, "sdr_rx_set_decim: factor < 1");
  r->rf_decim = rf_decim; r->audio_decim = audio_decim;
  r->rds_up = rds_up; r->rds_down = rds_down;
  return SDR_OK;
}

int sdr_rx_set_pll(sdr_rx* r, int which, double freq, double fs, double nco_scale, double phase_adj,
                   double norm_bw) {
  CHECK_RX(r);
  if (which != 0 && which != 1) return fail(SDR_EINVAL, "sdr_rx_set_pll: which=%d (0 stereo, 1 RDS)", which);
  if (!(fs != 0.0)) return fail(SDR_EINVAL, "sdr_rx_set_pll: Fs must be non-zero");
  r->pll[which] = pll_cfg(freq, fs, nco_scale, phase_adj, norm_bw);
  return SDR_OK;
}

int sdr_rx_reset(sdr_rx* r) {
  CHECK_RX(r);
  if (!r->ready) return SDR_OK;   // nothing allocated yet: the first block starts from zero
  TRY(set_dev(r->c));
  hipStream_t st = r->c->stream;
  if (r->front) HIP_TRY(hipStreamSynchronize(r->front));
  if (r->mid) HIP_TRY(hipStreamSynchronize(r->mid));
  r->pq_n = 0;                                   // submitted blocks' outputs are dropped
  // state banks, phases and wrap counters
  HIP_TRY(hipMemsetAsync(static_cast<char*>(r->mem) + r->reset.off, 0, (size_t)r->reset.bytes, st));
  std::vector<double> ps(6 * (size_t)r->S, 0.0);   // per stream 0 0 1 0 1 0: model/fmMonoBlock.py:76, model/fmRDSblock.py:96
  for (size_t s = 0; s < (size_t)r->S; ++s) ps[6 * s + 2] = ps[6 * s + 4] = 1.0;
  HIP_TRY(hipMemcpyAsync(r->pll_state[0], ps.data(), sizeof(double) * ps.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(r->pll_state[1], ps.data(), sizeof(double) * ps.size(), hipMemcpyHostToDevice, st));
  if (r->de_state) HIP_TRY(hipMemsetAsync(r->de_state, 0, (size_t)r->de_reset.bytes, st));
  if (r->bl) TRY(sdr_blend_reset(r->bl));
  HIP_TRY(hipStreamSynchronize(st));
  r->parity = 0; r->blocks = 0;
  r->tm.timed = false;                           // the blocks before the reset are gone
  r->last_fs = nullptr; r->host_done = -1;
  std::memcpy(r->out, r->outs[0], sizeof r->out);
  r->pcm = r->pcms[0];
  return SDR_OK;
}

int sdr_rx_set_deemph(sdr_rx* r, const double* b, double a1) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_deemph"));
  if (b == nullptr) {
    r->de_on = false;
    return SDR_OK;
  }
  if (!group_on(r->flags, G_AUDIO)) return fail(SDR_EINVAL, "sdr_rx_set_deemph: flags 0x%x produce no audio", r->flags);
  if (!std::isfinite(b[0]) || !std::isfinite(b[1]) || !std::isfinite(a1)) return fail(SDR_EINVAL, "sdr_rx_set_deemph: non-finite coefficients");
  if (std::fabs(a1) > 1.0) return fail(SDR_EINVAL, "sdr_rx_set_deemph: |a1| = %g > 1", std::fabs(a1));
  r->de_b[0] = b[0]; r->de_b[1] = b[1]; r->de_a1 = a1;
  r->de_on = true;
  return SDR_OK;
}

int sdr_rx_set_blend(sdr_rx* r, const sdr_blend_params* params, int nfft) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_blend"));
  if (nfft == 0) {
    r->bl_nfft = 0;
    return SDR_OK;
  }
  if (!group_on(r->flags, G_AUDIO)) return fail(SDR_EINVAL, "sdr_rx_set_blend: flags 0x%x produce no audio", r->flags);
  if (!r->de_on) return fail(SDR_EINVAL, "sdr_rx_set_blend: the audio output stage is off (sdr_rx_set_deemph)");
  if (nfft < 512 || nfft > SDR_SPEC_MAX_NFFT || (nfft & (nfft - 1)) != 0)
    return fail(SDR_EINVAL, "sdr_rx_set_blend: nfft=%d must be a power of two in [512, %d]", nfft, SDR_SPEC_MAX_NFFT);
  const int64_t M = ceil_div(r->B, r->rf_decim);
  if (M < nfft) return fail(SDR_EINVAL, "sdr_rx_set_blend: nfft %d > %lld demod samples per block", nfft, (long long)M);
  bool mute_on;
  TRY(blend_params(params, &r->bl_prm, &mute_on, "sdr_rx_set_blend"));   // sdr_blend_create's rules, before any device work
  r->bl_nfft = nfft;
  return SDR_OK;
}

int sdr_rx_blend_state(sdr_rx* r, double* host) {
  CHECK_RX(r);
  if (!r->bl_nfft) return fail(SDR_EINVAL, "sdr_rx_blend_state: the blend is off (sdr_rx_set_blend)");
  if (host == nullptr) return fail(SDR_EINVAL, "sdr_rx_blend_state: host is NULL");
  if (!r->ready) TRY(rx_finalize(r));
  return sdr_blend_state(r->bl, host);
}

int sdr_rx_pcm(sdr_rx* r, int16_t** dev, int64_t* stride, int64_t* n) {
  CHECK_RX(r);
  if (!r->de_on) return fail(SDR_EINVAL, "sdr_rx_pcm: the audio output stage is off (sdr_rx_set_deemph)");
  if (!r->ready) TRY(rx_finalize(r));
  if (dev) *dev = r->pcm;
  if (stride) *stride = r->pcm_stride;
  if (n) *n = 2 * r->A;
  return SDR_OK;
}

int sdr_rx_set_pipeline(sdr_rx* r, int on) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_pipeline"));
  if (on && !r->front) {
    TRY(set_dev(r->c));
    // (default priorities: an A/B of a high-priority PLL stream, a high-priority front stream and
    // low-priority front + PLL streams on one box measured C5 339-349 k against 352-355 k MS/s
    // for equal priorities, profiles/r06/e/prio_ab.txt)
    HIP_TRY(hipStreamCreateWithFlags(&r->front, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&r->mid, hipStreamNonBlocking));
    for (int q = 0; q < 3; ++q)
      for (hipEvent_t* e : {&r->ev_front[q], &r->ev_mid[q], &r->ev_back[q], &r->ev_read[q]}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  r->pipe = on != 0;
  return SDR_OK;
}

namespace {

// One sdr_rx_process_dev call: the row set and state banks it works on, its streams, the tap sets
// and what it materialises beyond the plan (sdr_rx_set_keep / the outputs a submit asks for)
struct RxBlock {
  sdr_rx* r;
  int q;                                // row set
  float** o;                            // its rows
  double *zi, *zf;                      // lfilter states in / out (the banks swap every block)
  hipStream_t st, fs;                   // back half (everything when not pipelined), front half
  const TapSet* ts[SDR_RX_NFILTERS];    // device taps (cached per context; the pointers stay valid for this call)
  int64_t ms;                           // row stride at the demod rate
  // Beyond the chain: the NCO rows, and the RDS LPF rows.  Without them the stage-C mixers
  // form the NCO from the PLL phase rows where they stage their inputs (PRE_NCO, sdr_nco.h) and
  // the RDS LPF + resampler is the composite filter (rx_cres_kernel), which runs either way.
  bool nco_rows, lpf_rows;
  bool de_mono;                         // the de-emphasised mono row of a stereo receiver
  int8_t* c8;                           // plan.codes: the PLLs' sign-code rows, [PLL k][stream], pcs bytes apart
  PllJobs P;
  NcoSrc nsrc[2];                       // per PLL (0 stereo, 1 RDS): where stage C takes its NCO from
};

bool kept(const sdr_rx* r, int o) { return (r->keep_now >> o) & 1ull; }
hipError_t mark(sdr_rx* r, int k, hipStream_t s) { return r->tm.mark(k, s); }
const double* zin(const RxBlock& b, int z) { return b.zi + b.r->zoff[z]; }
double* zout(const RxBlock& b, int z) { return b.zf + b.r->zoff[z]; }
// block k-nq, the last on this row set, may still run (not when the host has waited for it: submissions)
bool set_busy(const sdr_rx* r) { return r->blocks >= r->nq && r->blocks - r->nq > r->host_done; }

// What the block leaves in its rows: the configuration's outputs except the intermediates it skipped
void rx_made(const RxBlock& b) {
  sdr_rx* r = b.r;
  for (int o = 0; o < SDR_RX_NOUTPUTS; ++o)
    r->made[o] = need_out(r, o) && (kOutput[o].role != ROLE_NCO || b.nco_rows) && (kOutput[o].role != ROLE_LPF || b.lpf_rows) &&
                 (kOutput[o].role != ROLE_PLL_IN || !r->plan.codes || kept(r, o)) &&        // (codes: when kept)
                 (o != SDR_RX_O_AUDIO_DE || !r->plan.stx || b.de_mono);
}

// Filter f (state slot z) from the first n samples of output row xo into output row yo (and its
// host mirror); co: a PRE_MIX second operand's row
StageJob fir(const RxBlock& b, int f, int z, int xo, int64_t n, int yo, int D, int pre = PRE_NONE, int co = -1) {
  const sdr_rx* r = b.r;
  StageJob j{};
  j.x = b.o[xo]; j.x_stride = r->out_stride[xo]; j.n = n; j.c = co < 0 ? nullptr : b.o[co];
  j.taps = b.ts[f]->dev_f32; j.rtaps = b.ts[f]->dev_rev; j.taps64 = b.ts[f]->dev_f64;
  j.zi = zin(b, z); j.zf = zout(b, z); j.zi_stride = r->zlen[z];
  j.y = b.o[yo]; j.y_stride = r->out_stride[yo]; j.yh = r->mirror[yo]; j.yh_stride = r->out_n[yo];
  j.gain = 2.0f;                      // the reference's mixer gain (fmMonoBlock.py:156, fmRDSblock.py:173)
  j.pre = pre; j.D = D; j.U = 1; j.kind = JK_FIR; j.T = (int)r->taps[f].size();
  j.sym = b.ts[f]->sym;               // fold_tile may take it
  return j;
}

// Spans (the matrix-core rows): the PLLs take their inputs as sign codes (sdr_nco.h pll_code,
// r06) -- all the recurrence reads of them -- stored by the pilot BPF's and the RDS x^2 + BPF's
// tiles beside (or, when those rows are not kept, instead of) their f32 rows
StageJob coded(const RxBlock& b, StageJob j, int k, int o) {
  if (b.r->plan.codes) {
    j.y8 = b.c8 + (int64_t)k * b.r->S * b.r->pcs; j.y8_stride = b.r->pcs;
    if (!kept(b.r, o)) j.y = nullptr;
  }
  return j;
}

// Front half: FE, stage A, stage B.
int rx_front(RxBlock& b, const void* iq, int64_t xs, bool fast) {
  sdr_rx* r = b.r;
  const RxPlan& pl = r->plan;
  const int S = r->S;
  const int64_t M = r->M, ms = b.ms;
  hipStream_t fs = b.fs;
  if (r->pipe) {
    // states of block k-1 (r04b: not when its front half ran on this same stream, in order)
    if (r->blocks >= 1 && r->last_fs != fs) HIP_TRY(hipStreamWaitEvent(fs, r->ev_front[(b.q + r->nq - 1) % r->nq], 0));
    r->last_fs = fs;
    if (set_busy(r)) {
      HIP_TRY(hipStreamWaitEvent(fs, r->ev_back[b.q], 0));
      HIP_TRY(hipStreamWaitEvent(fs, r->ev_read[b.q], 0));
    }
  }
  HIP_TRY(mark(r, 0, fs));
  // FE: RF FIR + decimate + demod (fe.hip).  The tiled kernels take the reference's RF
  // configurations; their carried state (I/Q zf, demod phase) is finished by workgroups of
  // the stage-A launch.  Other configurations run sdr_rf_frontend_dev's generic path (on the
  // context stream, so a pipelined receiver's front half runs there for such blocks).
  const TapSet* rf = b.ts[SDR_RX_F_RF];
  const int Trf = (int)r->taps[SDR_RX_F_RF].size();
  FeState fst{};
  if (fast) {
    const int G = r->u8 ? 8 : 2;
    const int64_t fstride = S > 1 ? xs : ceil_div(r->B, G) * G;
    FeLaunch a{iq, r->B, fstride, 0, S, rf->dev_f32, &rf->h, Trf, r->rf_decim, r->u8,
               zin(b, Z_FE_I), zin(b, Z_FE_Q), r->zlen[Z_FE_I], r->phase, b.o[SDR_RX_O_DEMOD], ms, nullptr, nullptr,
               r->last_phi, r->wraps, rf->dev_afr};
    HIP_TRY(sdr_launch_fe(a, fs));
    fst = FeState{iq, r->B, xs, rf->dev_f64, zin(b, Z_FE_I), zin(b, Z_FE_Q), zout(b, Z_FE_I), zout(b, Z_FE_Q),
                  r->zlen[Z_FE_I], r->last_phi, r->wraps, r->phase, Trf, r->u8, 1};
  } else {
    const void* x = iq;
    int64_t xst = xs;
    if (r->u8) {
      // the generic kernels read f32: the block as the samples a u8 front end normalises it to,
      // in packed receiver-owned rows (fs is the context stream here, as the generic path's; 64
      // floats behind the last row: the f32 tiles, which take such rows at 101 / 151 taps and
      // decimation 10, load whole 16-B chunks)
      if (r->iq_f32 == nullptr) HIP_TRY(hipMalloc(&r->iq_f32, sizeof(float) * (2 * (size_t)S * (size_t)r->B + 64)));
      HIP_TRY(sdr_launch_iq_u8_f32(iq, r->B, xs, S, r->iq_f32, r->B, fs));
      x = r->iq_f32;
      xst = r->B;
    }
    TRY(sdr_rf_frontend_dev(r->c, x, SDR_IQ_F32, r->B, xst, 0, S, r->taps[SDR_RX_F_RF].data(),
                            Trf, r->rf_decim, zin(b, Z_FE_I), zin(b, Z_FE_Q), r->zlen[Z_FE_I], zout(b, Z_FE_I),
                            zout(b, Z_FE_Q), r->phase, b.o[SDR_RX_O_DEMOD], ms, nullptr, nullptr));
  }
  HIP_TRY(mark(r, 1 + SDR_RX_ST_FE, fs));
  // stage A: every filter of the demodulated signal (model/fmMonoBlock.py:101-105, :117,
  // :151; model/fmRDSblock.py:156)
  std::vector<StageJob> A;
  if (pl.au) A.push_back(fir(b, SDR_RX_F_AUDIO, Z_AUDIO, SDR_RX_O_DEMOD, M, SDR_RX_O_AUDIO, r->audio_decim));
  if (pl.stx) {
    A.push_back(coded(b, fir(b, SDR_RX_F_PILOT, Z_PILOT, SDR_RX_O_DEMOD, M, SDR_RX_O_BPF_RECOVERY, 1), 0, SDR_RX_O_BPF_RECOVERY));
    A.push_back(fir(b, SDR_RX_F_STEREO_BPF, Z_BAND, SDR_RX_O_DEMOD, M, SDR_RX_O_BPF_EXTRACTION, 1));
  }
  if (pl.rd) A.push_back(fir(b, SDR_RX_F_RDS_EXTRACT, Z_EXTRACT, SDR_RX_O_DEMOD, M, SDR_RX_O_RDS_EXTRACT, 1));
  HIP_TRY(launch_stage(A, S, fs, &fst));
  HIP_TRY(mark(r, 1 + SDR_RX_ST_A, fs));
  // stage B: RDS squaring non-linearity + BPF (model/fmRDSblock.py:161-164)
  if (pl.rd) HIP_TRY(launch_stage({coded(b, fir(b, SDR_RX_F_RDS_SQUARE, Z_SQUARE, SDR_RX_O_RDS_EXTRACT, M, SDR_RX_O_RDS_PRE_PLL,
                                                 1, PRE_SQUARE), 1, SDR_RX_O_RDS_PRE_PLL)}, S, fs));
  HIP_TRY(mark(r, 1 + SDR_RX_ST_B, fs));
  return SDR_OK;
}

// Loop k's job (b.P) and where stage C takes its NCO from (b.nsrc[k]).  The tables follow the
// loop's current configuration (sdr_rx_set_pll is legal between blocks).
int rx_pll_job(RxBlock& b, int k, int in, int nco_i, int nco_q) {
  sdr_rx* r = b.r;
  const RxPlan& pl = r->plan;
  const int S = r->S;
  const int64_t M = r->M, ms = b.ms;
  PllJobs& P = b.P;
  float *ni = b.o[nco_i], *nq = nco_q < 0 ? nullptr : b.o[nco_q];
  double* thk = r->theta + ((int64_t)b.q * 2 + k) * S * r->ths;
  double* pck = r->pllc + ((int64_t)b.q * 2 + k) * S * r->cst;
  const double *resp = nullptr, *qtab = nullptr;
  TRY(get_resp(r->c, r->pll[k], M, &resp));
  TRY(get_qtab(r->c, r->pll[k], &qtab));
  const int jq = P.njobs;
  P.j[P.njobs++] = PllJob{b.o[in], ms, r->pll_state[k], thk, r->ths, ni, nq, ms, r->pll[k], pck, r->cst,
                          (double)M * (double)r->blocks, 1, resp, qtab};
  if (pl.codes) {
    P.j[jq].in8 = b.c8 + (int64_t)k * S * r->pcs; P.j[jq].in8_stride = r->pcs;
  }
  NcoSrc& N = b.nsrc[k];
  N.theta = M >= 2 ? thk : nullptr;   // (M < 2: the sequential kernels' Q-form rows; mix from the NCO rows)
  // compact phase rows (sdr_nco.h, r06): half the bytes of the solve's stores and of the mixers'
  // loads.  Every reader decodes them, so the form depends on the geometry alone, not on a block's keep
  if (pl.th32[k]) P.j[jq].th32 = N.th32 = 1;
  N.th_stride = r->ths; N.n = M;
  N.nco_i = ni; N.nco_q = nq; N.out_stride = ms;
  N.w = 2.0 * M_PI * (r->pll[k].freq / r->pll[k].fs); N.scale = r->pll[k].scale; N.adj = r->pll[k].adj;
  if (pl.lng) {                                            // the records follow (stx + rd) x S headers
    N.blk = long_blk0(P.work, (int)pl.stx + (int)pl.rd, S, pl.nb, jq * S);
    N.blk_stride = N.nb = pl.nb; N.pb = pl.pb;
    N.resp = resp; N.resp32 = resp32_of(resp, pl.pb);
  }
  return SDR_OK;
}

// PLLs (model/fmMonoBlock.py:119, model/fmRDSblock.py:167): one lane per recurrence.
// Pipelined, the three launches go to three streams: the per-sample constants with the
// front half (trigOffset = M x blocks since reset, known here), the recurrence alone on
// its own stream -- block k's starts as soon as block k-1's is done, beside block k-1's
// NCO and stages C-E and block k+1's front half -- and the NCO with the back half.  Phase
// and constant rows alternate with the row set; set q is free once block k-2's back half
// (which waited for its recurrence) is done.
int rx_pll(RxBlock& b) {
  sdr_rx* r = b.r;
  const RxPlan& pl = r->plan;
  const int q = b.q;
  PllJobs& P = b.P;
  const bool plls = pl.stx || pl.rd;
  hipStream_t ps = r->pipe ? r->mid : b.st;          // the recurrences' own stream when pipelined
  if (plls) {
    P.nstreams = r->S; P.n = r->M;
    P.stats = r->c->pll_stats; P.nco_rows = b.nco_rows ? 1 : 0;
    P.work = r->pllw_bytes ? r->pllw + (int64_t)q * r->pllw_bytes : nullptr;
    if (pl.stx) TRY(rx_pll_job(b, 0, SDR_RX_O_BPF_RECOVERY, SDR_RX_O_STEREO_NCO, -1));
    if (pl.rd) TRY(rx_pll_job(b, 1, SDR_RX_O_RDS_PRE_PLL, SDR_RX_O_RDS_NCO_I, SDR_RX_O_RDS_NCO_Q));
    HIP_TRY(sdr_launch_pll_prep(P, b.fs));
  }
  if (r->pipe) {
    HIP_TRY(hipEventRecord(r->ev_front[q], b.fs));
    if (plls) {
      HIP_TRY(hipStreamWaitEvent(ps, r->ev_front[q], 0));
      if (set_busy(r)) {
        HIP_TRY(hipStreamWaitEvent(ps, r->ev_back[q], 0));
        HIP_TRY(hipStreamWaitEvent(ps, r->ev_read[q], 0));
      }
    } else {
      HIP_TRY(hipStreamWaitEvent(b.st, r->ev_front[q], 0));
    }
  }
  if (plls) HIP_TRY(sdr_launch_pll_loop(P, ps));
  HIP_TRY(mark(r, 1 + SDR_RX_ST_PLL, ps));
  if (r->pipe && plls) {
    HIP_TRY(hipEventRecord(r->ev_mid[q], ps));
    HIP_TRY(hipStreamWaitEvent(b.st, r->ev_mid[q], 0));
  }
  if (plls) HIP_TRY(sdr_launch_pll_nco(P, b.st));
  return SDR_OK;
}

// stage D with the composite filter: the RDS mixers + LPF + x19 / 80 resampler in one kernel, and
// the LPF's and anti-image filter's final states
int rx_cres(const RxBlock& b) {
  const sdr_rx* r = b.r;
  float** o = b.o;
  CresJob J{};
  J.x = o[SDR_RX_O_RDS_EXTRACT]; J.n = r->M; J.x_stride = b.ms; J.nco = b.nsrc[1];
  J.ctaps = r->ctaps; J.h64 = b.ts[SDR_RX_F_RDS_LPF]->dev_f64; J.g64 = b.ts[SDR_RX_F_RDS_ANTI]->dev_f64;
  J.zi_l[0] = zin(b, Z_RLPF_I); J.zi_l[1] = zin(b, Z_RLPF_Q);
  J.zi_a[0] = zin(b, Z_ANTI_I); J.zi_a[1] = zin(b, Z_ANTI_Q);
  J.zf_l[0] = zout(b, Z_RLPF_I); J.zf_l[1] = zout(b, Z_RLPF_Q);
  J.zf_a[0] = zout(b, Z_ANTI_I); J.zf_a[1] = zout(b, Z_ANTI_Q); J.zs = r->zlen[Z_RLPF_I];
  J.y[0] = o[SDR_RX_O_RDS_RES_I]; J.y[1] = o[SDR_RX_O_RDS_RES_Q];
  J.yh[0] = r->mirror[SDR_RX_O_RDS_RES_I]; J.yh[1] = r->mirror[SDR_RX_O_RDS_RES_Q];
  J.y_stride = r->out_stride[SDR_RX_O_RDS_RES_I]; J.yh_stride = r->out_n[SDR_RX_O_RDS_RES_I];
  J.R = r->R; J.nstreams = r->S;
  if (r->zlen[Z_ANTI_I] != J.zs || !cres_fits(J)) return fail(SDR_EINVAL, "sdr_rx: composite RDS geometry");
  HIP_TRY(launch_cres(J, r->plan.span, b.st));
  return SDR_OK;
}

// a stage-C mixer: the NCO from loop k's phase rows (PRE_NCO) where the tiles can form it
StageJob mixer(const RxBlock& b, StageJob j, int k, int sin_) {
  if (b.nsrc[k].theta != nullptr && (j.T == 101 || j.T == 151) && (j.D == 1 || j.D == 5)) {
    j.pre = PRE_NCO; j.c = nullptr;
    j.nco = b.nsrc[k]; j.nco_sin = sin_;
  }
  return j;
}

// Back half: stage C, the composite or two-stage D, E, the audio output stage.
int rx_back(RxBlock& b) {
  sdr_rx* r = b.r;
  const RxPlan& pl = r->plan;
  const int S = r->S;
  const int64_t M = r->M;
  float** o = b.o;
  hipStream_t st = b.st;
  // stage C: the stereo mixer + LPF (its store also forms L and R); the RDS I/Q mixer + LPF
  // rows only when they are kept (or without the composite filter)
  std::vector<StageJob> C;
  if (pl.stx) {
    StageJob j = fir(b, SDR_RX_F_STEREO_LPF, Z_SLPF, SDR_RX_O_BPF_EXTRACTION, M, SDR_RX_O_STEREO, r->audio_decim,
                     PRE_MIX, SDR_RX_O_STEREO_NCO);                             // fmMonoBlock.py:155-162
    j.mono = o[SDR_RX_O_AUDIO]; j.left = o[SDR_RX_O_LEFT]; j.right = o[SDR_RX_O_RIGHT];   // :166-170 (intended)
    j.lh = r->mirror[SDR_RX_O_LEFT]; j.rh = r->mirror[SDR_RX_O_RIGHT];   // (yh_stride: out_n of stereo == out_n of L and R)
    C.push_back(mixer(b, j, 0, 0));
  }
  if (b.lpf_rows) {                                                            // fmRDSblock.py:173-182
    for (int k = 0; k < 2; ++k) {
      StageJob j = fir(b, SDR_RX_F_RDS_LPF, k ? Z_RLPF_Q : Z_RLPF_I, SDR_RX_O_RDS_EXTRACT, M,
                       k ? SDR_RX_O_RDS_LPF_Q : SDR_RX_O_RDS_LPF_I, 1, PRE_MIX, k ? SDR_RX_O_RDS_NCO_Q : SDR_RX_O_RDS_NCO_I);
      if (pl.cres) j.zf = nullptr;              // the composite kernel writes the LPF's final states
      C.push_back(mixer(b, j, 1, k));
    }
  }
  HIP_TRY(launch_stage(C, S, st));
  HIP_TRY(mark(r, 1 + SDR_RX_ST_C, st));
  if (pl.rd) {
    if (pl.cres) {
      TRY(rx_cres(b));
    } else {
      // stage D: rational resamplers (fmRDSblock.py:184-199)
      std::vector<StageJob> Dj;
      for (int k = 0; k < 2; ++k) {
        StageJob j = fir(b, SDR_RX_F_RDS_ANTI, k ? Z_ANTI_Q : Z_ANTI_I, k ? SDR_RX_O_RDS_LPF_Q : SDR_RX_O_RDS_LPF_I, M,
                         k ? SDR_RX_O_RDS_RES_Q : SDR_RX_O_RDS_RES_I, r->rds_down);
        j.kind = JK_RESAMPLE; j.U = r->rds_up;
        Dj.push_back(j);
      }
      HIP_TRY(launch_stage(Dj, S, st));
    }
    HIP_TRY(mark(r, 1 + SDR_RX_ST_D, st));
    // stage E: RRC (fmRDSblock.py:202-204)
    HIP_TRY(launch_stage({fir(b, SDR_RX_F_RDS_RRC, Z_RRC_I, SDR_RX_O_RDS_RES_I, r->R, SDR_RX_O_RDS_RRC_I, 1),
                          fir(b, SDR_RX_F_RDS_RRC, Z_RRC_Q, SDR_RX_O_RDS_RES_Q, r->R, SDR_RX_O_RDS_RRC_Q, 1)}, S, st));
  } else {
    HIP_TRY(mark(r, 1 + SDR_RX_ST_D, st));
  }
  // the audio output stage (audio.hip): de-emphasis of L / R (mono without SDR_RX_STEREO) into
  // their _DE rows and the interleaved PCM, and of a stereo receiver's mono row when it is kept
  if (r->de_on) {
    const bool stx = pl.stx;
    const int64_t as = r->out_stride[SDR_RX_O_AUDIO];
    const float *xl = o[stx ? SDR_RX_O_LEFT : SDR_RX_O_AUDIO], *xr = stx ? o[SDR_RX_O_RIGHT] : nullptr;
    float *yl = o[stx ? SDR_RX_O_LEFT_DE : SDR_RX_O_AUDIO_DE], *yr = stx ? o[SDR_RX_O_RIGHT_DE] : nullptr;
    if (r->bl) {
      // this block's multiplex spectra -> its quality and gains -> the tail ramps to them
      const int nb = r->bl_nfft / 2 + 1;
      TRY(sdr_rspec_process_dev(r->bl_spec, o[SDR_RX_O_DEMOD], r->M, r->out_stride[SDR_RX_O_DEMOD], r->bl_power, nb));
      TRY(sdr_blend_update_dev(r->bl, r->bl_power, nb, nb, kMpxFs));
      TRY(sdr_audio_blend_dev(r->c, xl, xr, r->A, as, S, r->de_b, r->de_a1, r->de_state, yl, yr, r->pcms[b.q], r->pcm_stride,
                              r->bl_gains));
    } else {
      TRY(sdr_audio_out_dev(r->c, xl, xr, r->A, as, S, r->de_b, r->de_a1, r->de_state, yl, yr, r->pcms[b.q], r->pcm_stride));
    }
    if (b.de_mono)
      TRY(sdr_iir1_dev(r->c, o[SDR_RX_O_AUDIO], r->A, as, S, r->de_b, r->de_a1, r->de_mono, r->de_mono,
                       o[SDR_RX_O_AUDIO_DE], as));
    r->pcm = r->pcms[b.q];
  }
  HIP_TRY(mark(r, 1 + SDR_RX_ST_E, st));
  return SDR_OK;
}

}  // namespace

int sdr_rx_process_dev(sdr_rx* r, const void* iq, int64_t iq_stride) {
  CHECK_RX(r);
  if (iq == nullptr) return fail(SDR_EINVAL, "sdr_rx_process_dev: iq is NULL");
  if (r->S > 1 && iq_stride < r->B) return fail(SDR_EINVAL, "sdr_rx_process_dev: iq_stride %lld < block", (long long)iq_stride);
  if (!r->ready) TRY(rx_finalize(r));
  TRY(set_dev(r->c));
  const RxPlan& pl = r->plan;
  RxBlock b{};
  b.r = r; b.q = r->pipe ? (int)(r->blocks % r->nq) : 0;
  b.o = r->outs[b.q];
  b.zi = r->bank[r->parity]; b.zf = r->bank[r->parity ^ 1];
  const int Trf = (int)r->taps[SDR_RX_F_RF].size();
  const int64_t xs = r->S > 1 ? iq_stride : r->B;
  const bool fast = (Trf == 101 || Trf == 151) && r->rf_decim == 10 && (r->S <= 1 || r->u8 || xs % (r->u8 ? 8 : 2) == 0) &&
                    ((uintptr_t)iq % (r->u8 ? 4 : 16)) == 0;
  b.st = r->c->stream; b.fs = (r->pipe && fast) ? r->front : b.st;
  // Whatever the caller put on the context stream since block k-1 (readers of its rows: the RDS
  // banks, meters, spectra, filters in place) belongs to block k-1's row set: ev_read of that set
  // is recorded behind it, and the front half and the PLLs of block k-1+nq wait for it beside
  // ev_back before they overwrite the set -- the readers come first however far the host runs
  // ahead.  Block k's own front half waits for block k-nq's events only and still overlaps.  An
  // event of its own: ev_back is also a submitted block's completion (sdr_rx_submit), and recorded
  // again here the host's wait for block k-1 ended late (c4 1 290 -> 760 - 1 050 MS/s).
  if (r->pipe && r->blocks >= 1) HIP_TRY(hipEventRecord(r->ev_read[(b.q + r->nq - 1) % r->nq], b.st));
  for (int f = 0; f < SDR_RX_NFILTERS; ++f)
    if (filter_used(r, f)) TRY(get_taps(r->c, r->taps[f].data(), (int)r->taps[f].size(), &b.ts[f]));
  b.ms = r->out_stride[SDR_RX_O_DEMOD];
  b.nco_rows = (pl.stx && kept(r, SDR_RX_O_STEREO_NCO)) || (pl.rd && (kept(r, SDR_RX_O_RDS_NCO_I) || kept(r, SDR_RX_O_RDS_NCO_Q))) ||
               r->M < 2 || (pl.rd && !pl.cres) || !pl.tiles_ok;
  b.lpf_rows = pl.rd && (!pl.cres || kept(r, SDR_RX_O_RDS_LPF_I) || kept(r, SDR_RX_O_RDS_LPF_Q));
  b.de_mono = r->de_on && pl.stx && kept(r, SDR_RX_O_AUDIO_DE);
  b.c8 = pl.codes ? r->pcode + (int64_t)b.q * 2 * r->S * r->pcs : nullptr;
  TRY(rx_front(b, iq, xs, fast));
  TRY(rx_pll(b));
  TRY(rx_back(b));
  rx_made(b);
  if (r->pipe) HIP_TRY(hipEventRecord(r->ev_back[b.q], b.st));
  std::memcpy(r->out, r->outs[b.q], sizeof r->out);
  r->parity ^= 1;
  ++r->blocks;
  return SDR_OK;
}

namespace {
// grow a pinned host buffer (synchronising first: work in flight may use it).  Coherent
// (uncached by the GPU): the device reads the IQ the host wrote for this block, and the
// host reads what the stage kernels stored, with no copy engine in between.
int grow_pinned(sdr_rx* r, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return SDR_OK;
  if (*p) {
    HIP_TRY(hipStreamSynchronize(r->c->stream));
    HIP_TRY(hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  hipError_t e = hipHostMalloc(p, bytes, hipHostMallocCoherent);
  if (e != hipSuccess) return fail(SDR_ENOMEM, "sdr_rx: hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
  *cap = bytes;
  return SDR_OK;
}
// outputs a stage kernel stores (and can store a host copy of); the demod (FE kernel) and
// the NCOs (PLL) come back by copy
bool stage_output(int o) { return kOutput[o].by == BY_STAGE; }

// the oldest block in flight: wait for it, copy its outputs out of its pinned slot
int deliver(sdr_rx* r) {
  if (r->pq_n == 0) return SDR_OK;
  const sdr_rx::Pending& P = r->pq[r->pq_head];
  r->pq_head = (r->pq_head + 1) % 4;
  --r->pq_n;
  HIP_TRY(hipEventSynchronize(P.ev));
  r->host_done = std::max(r->host_done, P.blk);
  const float* base = r->pin_out + (size_t)P.slot * r->out_slot / sizeof(float);
  for (int i = 0; i < P.nout; ++i) {
    const int64_t n = r->out_n[P.which[i]];
    const float* src = base + P.region[P.which[i]];
    for (int s = 0; s < r->S; ++s) std::memcpy(P.out[i] + s * P.os[i], src + s * n, sizeof(float) * (size_t)n);
  }
  return SDR_OK;
}

}  // namespace

int sdr_rx_process(sdr_rx* r, const void* iq_host, int64_t iq_stride) {
  return sdr_rx_run(r, iq_host, iq_stride, 0, nullptr, nullptr, nullptr);
}

// One block from host memory, without waiting for it.  The per-block cost at the
// reference's block sizes is the number of engine hand-offs, not bytes
// (tools/xfer_probe.hip: an SDMA upload, two kernels, an SDMA download and a wait take
// 35 us; the same kernels reading and writing pinned host memory directly, 25 us), so: the
// IQ is copied into a pinned slot and the FE kernel reads it from there over PCIe; each
// requested output is stored into the slot's pinned output region by the stage kernel that
// produces it (the demod and NCO rows, which no stage kernel stores, come back by copy).
// depth + 1 slots (sdr_rx_set_depth, default 1): while block k runs, the host delivers block
// k-depth's outputs (into the buffers given with it) and returns; sdr_rx_flush delivers the rest.
int sdr_rx_submit(sdr_rx* r, const void* iq_host, int64_t iq_stride, int nout, const int* which, float* const* out,
                  const int64_t* out_stride) {
  CHECK_RX(r);
  if (iq_host == nullptr) return fail(SDR_EINVAL, "sdr_rx_submit: iq is NULL");
  if (r->S > 1 && iq_stride < r->B) return fail(SDR_EINVAL, "sdr_rx_submit: iq_stride %lld < block", (long long)iq_stride);
  if (nout < 0 || nout > SDR_RX_MAXOUT || (nout > 0 && (which == nullptr || out == nullptr)))
    return fail(SDR_EINVAL, "sdr_rx_submit: %d outputs (at most %d)", nout, SDR_RX_MAXOUT);
  if (!r->ready) TRY(rx_finalize(r));
  for (int i = 0; i < nout; ++i) {
    if (which[i] < 0 || which[i] >= SDR_RX_NOUTPUTS || !need_out(r, which[i]))
      return fail(SDR_EINVAL, "sdr_rx_submit: output %d is not produced by flags 0x%x", which[i], r->flags);
    if (out[i] == nullptr) return fail(SDR_EINVAL, "sdr_rx_submit: output buffer %d is NULL", i);
    if (r->S > 1 && out_stride && out_stride[i] < r->out_n[which[i]])
      return fail(SDR_EINVAL, "sdr_rx_submit: out_stride[%d] too small", i);
  }
  TRY(set_dev(r->c));
  hipStream_t st = r->c->stream;
  const int64_t es = r->u8 ? 2 : 8;                      // bytes per complex sample
  const int64_t xs = r->S > 1 ? iq_stride : r->B;
  const size_t bytes = (size_t)(xs * (r->S - 1) + r->B) * es;
  // pinned output regions, one per distinct requested output (rows out_n apart)
  sdr_rx::Pending P;
  uint64_t wmask = 0;                                     // the distinct outputs asked for (bit o)
  auto want = [&](int o) { return (wmask >> o) & 1ull; };
  size_t obytes = 0;
  for (int i = 0; i < nout; ++i) {
    const int o = which[i];
    P.which[i] = o;
    P.out[i] = out[i];
    P.os[i] = (r->S > 1 && out_stride) ? out_stride[i] : r->out_n[o];
    if (want(o)) continue;
    wmask |= 1ull << o;
    P.region[o] = obytes / sizeof(float);
    obytes += sizeof(float) * (size_t)(r->out_n[o] * r->S);
  }
  const size_t in_slot = (bytes + 255) / 256 * 256, out_slot = (std::max<size_t>(obytes, 16) + 255) / 256 * 256;
  const int nslot = r->depth + 1;
  if (in_slot > r->in_slot || out_slot > r->out_slot) {   // grow (the blocks in flight are delivered first)
    while (r->pq_n > 0) TRY(deliver(r));
    r->in_slot = std::max(r->in_slot, in_slot);
    r->out_slot = std::max(r->out_slot, out_slot);
    TRY(grow_pinned(r, &r->pin_in, &r->pin_in_cap, nslot * r->in_slot));
    TRY(grow_pinned(r, reinterpret_cast<void**>(&r->pin_out), &r->pin_out_cap, nslot * r->out_slot));
    for (int q = 0; q < nslot; ++q)
      if (!r->ev_done[q]) HIP_TRY(hipEventCreateWithFlags(&r->ev_done[q], hipEventDisableTiming));
  }
  const int slot = (int)(r->subs % nslot);
  // slot `slot` was last used by block k-depth-1, delivered (waited for) by the previous call
  char* pin = static_cast<char*>(r->pin_in) + (size_t)slot * r->in_slot;
  float* pout = r->pin_out + (size_t)slot * r->out_slot / sizeof(float);
  std::memcpy(pin, iq_host, bytes);
  for (int o = 0; o < SDR_RX_NOUTPUTS; ++o) r->mirror[o] = want(o) && stage_output(o) ? pout + P.region[o] : nullptr;
  r->keep_now = wmask;                                    // materialise what this call returns
  const int rc = sdr_rx_process_dev(r, pin, xs);
  r->keep_now = r->keep;
  for (float*& m : r->mirror) m = nullptr;
  TRY(rc);
  bool copied = false;
  for (int o = 0; o < SDR_RX_NOUTPUTS; ++o) {
    if (!want(o) || stage_output(o)) continue;
    copied = true;
    const int64_t n = r->out_n[o];
    HIP_TRY(hipMemcpy2DAsync(pout + P.region[o], sizeof(float) * (size_t)n, r->out[o],
                             sizeof(float) * (size_t)r->out_stride[o], sizeof(float) * (size_t)n, (size_t)r->S,
                             hipMemcpyDeviceToHost, st));
  }
  const int qb = (int)((r->blocks - 1) % r->nq);
  if (r->pipe && !copied && r->depth < r->nq) {
    // nothing after the back half: its row-set event marks the block's completion (one event
    // call fewer per block).  Not at depth 3 (nq 3): block k+3 re-records the set's event
    // before block k is delivered, and the host would wait for the newest block each time --
    // the pipeline drained at every call (c4 1 163 -> 472 MS/s)
    P.ev = r->ev_back[qb];
  } else {
    // the row set is free for block k+nq once these copies have read it too (the event the
    // front half of block k+nq waits for is recorded again, after them)
    if (r->pipe) HIP_TRY(hipEventRecord(r->ev_back[qb], st));
    HIP_TRY(hipEventRecord(r->ev_done[slot], st));
    P.ev = r->ev_done[slot];
  }
  ++r->subs;
  P.slot = slot; P.nout = nout; P.blk = r->blocks - 1;
  r->pq[(r->pq_head + r->pq_n) % 4] = P;
  ++r->pq_n;
  while (r->pq_n > r->depth) TRY(deliver(r));            // block k-depth
  return SDR_OK;
}

int sdr_rx_flush(sdr_rx* r) {
  CHECK_RX(r);
  if (r->pq_n == 0) return SDR_OK;
  TRY(set_dev(r->c));
  while (r->pq_n > 0) TRY(deliver(r));
  return SDR_OK;
}

int sdr_rx_set_depth(sdr_rx* r, int depth) {
  CHECK_RX(r);
  TRY(still_open(r, "sdr_rx_set_depth"));
  if (depth < 1 || depth > 3) return fail(SDR_EINVAL, "sdr_rx_set_depth: depth %d outside [1, 3]", depth);
  r->depth = depth; r->nq = depth >= 2 ? 3 : 2;
  return SDR_OK;
}

// One block from host memory, waited for: the per-block drop-in call of fmMonoBlock.py's loop.
int sdr_rx_run(sdr_rx* r, const void* iq_host, int64_t iq_stride, int nout, const int* which, float* const* out,
               const int64_t* out_stride) {
  if (r != nullptr) TRY(sdr_rx_flush(r));                // an earlier submit's block first
  TRY(sdr_rx_submit(r, iq_host, iq_stride, nout, which, out, out_stride));
  return sdr_rx_flush(r);
}

int sdr_rx_output(sdr_rx* r, int which, float** dev, int64_t* stride, int64_t* n) {
  CHECK_RX(r);
  if (which < 0 || which >= SDR_RX_NOUTPUTS) return fail(SDR_EINVAL, "sdr_rx_output: output %d", which);
  if (!r->ready) TRY(rx_finalize(r));
  if (!need_out(r, which)) return fail(SDR_EINVAL, "sdr_rx_output: output %d is not produced by flags 0x%x", which, r->flags);
  if (dev) *dev = r->out[which];
  if (stride) *stride = r->out_stride[which];
  if (n) *n = r->out_n[which];
  return SDR_OK;
}

int sdr_rx_set_keep(sdr_rx* r, uint64_t mask) {
  CHECK_RX(r);
  r->keep = r->keep_now = mask;
  return SDR_OK;
}

int sdr_rx_fetch(sdr_rx* r, int which, float* host, int64_t host_stride) {
  float* d; int64_t ds, n;
  TRY(sdr_rx_output(r, which, &d, &ds, &n));
  if (!r->made[which])
    return fail(SDR_EINVAL, "sdr_rx_fetch: output %d was not materialised by the latest block (sdr_rx_set_keep)", which);
  if (host == nullptr) return fail(SDR_EINVAL, "sdr_rx_fetch: host is NULL");
  if (r->S > 1 && host_stride < n) return fail(SDR_EINVAL, "sdr_rx_fetch: host_stride %lld < %lld", (long long)host_stride, (long long)n);
  TRY(set_dev(r->c));
  HIP_TRY(hipMemcpy2DAsync(host, sizeof(float) * (size_t)(r->S > 1 ? host_stride : n), d, sizeof(float) * (size_t)ds,
                           sizeof(float) * (size_t)n, (size_t)r->S, hipMemcpyDeviceToHost, r->c->stream));
  HIP_TRY(hipStreamSynchronize(r->c->stream));
  return SDR_OK;
}

int sdr_rx_set_timing(sdr_rx* r, int on) {
  CHECK_RX(r);
  TRY(set_dev(r->c));
  HIP_TRY(r->tm.enable(on != 0));
  return SDR_OK;
}

int sdr_rx_stage_ms(sdr_rx* r, float* ms) {
  if (r == nullptr || ms == nullptr) return fail(SDR_EINVAL, "sdr_rx_stage_ms: NULL argument");
  return r->tm.elapsed(ms, "sdr_rx_stage_ms: no timed block (sdr_rx_set_timing)");
}

int sdr_rx_pll_stats(sdr_rx* r, int64_t* out, int reset) {
  CHECK_RX(r);
  TRY(set_dev(r->c));
  if (r->front) HIP_TRY(hipStreamSynchronize(r->front));
  if (r->mid) HIP_TRY(hipStreamSynchronize(r->mid));
  HIP_TRY(hipStreamSynchronize(r->c->stream));
  return sdr_pll_stats(r->c, out, reset);
}

int sdr_rx_state(sdr_rx* r, double* phase, double* pll_stereo, double* pll_rds) {
  CHECK_RX(r);
  if (!r->ready) TRY(rx_finalize(r));
  TRY(set_dev(r->c));
  hipStream_t st = r->c->stream;
  const size_t S = (size_t)r->S;
  if (phase) HIP_TRY(hipMemcpyAsync(phase, r->phase, sizeof(double) * S, hipMemcpyDeviceToHost, st));
  if (pll_stereo) HIP_TRY(hipMemcpyAsync(pll_stereo, r->pll_state[0], sizeof(double) * 6 * S, hipMemcpyDeviceToHost, st));
  if (pll_rds) HIP_TRY(hipMemcpyAsync(pll_rds, r->pll_state[1], sizeof(double) * 6 * S, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SDR_OK;
}

}  // extern "C"
