/* libsdr.so — C-ABI of the MI355X-native FM-SDR hot path (gfx950 HIP kernels).
 *
 * This is the drop-in boundary for the reference's per-block signal-processing
 * functions.  Plain pointers and sizes only; no torch/numpy types.
 * Each entry point names the reference interface it replaces (file:line under the
 * reference repository m1nty/Real-Time-Software-Defined-Radio).
 *
 * Conventions
 *   - Return value: SDR_OK (0) or a negative SDR_E* code; sdr_last_error() returns
 *     the calling thread's last error message (the Python layer raises ValueError
 *     for SDR_EINVAL, NotImplementedError for SDR_EUNSUPPORTED, RuntimeError else;
 *     mirroring scipy.signal.lfilter's ValueError/NotImplementedError,
 *     scipy/signal/_signaltools.py:2143-2151).
 *   - Filter state `zi` uses scipy.signal.lfilter's convention (length taps-1,
 *     f64): y[n] = (b*x)[n] + zi[n] for n < taps-1, and the returned zf is the tail
 *     of the full convolution.  Host `*_inout` state arrays are overwritten with the
 *     new state, so reference and libsdr calls can be mixed block by block.
 *   - Decimated outputs are y[D*m] for m = 0 .. ceil(n/D)-1 (lfilter(...)[::D]).
 *   - Demod phase state is the reference's accumulated unwrapped phase
 *     (model/fmSupportLib.py:40-44), returned as phi_last + 2*pi*(number of wraps).
 *   - A context (sdr_ctx) owns one HIP stream and scratch memory on one device; it is
 *     not thread-safe: one context per host thread per GPU.
 *   - Host-buffer functions are synchronous.  `*_dev` functions take device
 *     pointers and are asynchronous on the context's stream (sdr_stream()).
 *   - Numerics: samples are processed in f32 (inputs f32 or u8); filter-state (zf)
 *     and PLL phase arithmetic are f64.
 */
#ifndef SDR_H_
#define SDR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDR_ABI_VERSION 1

enum {
  SDR_OK = 0,
  SDR_EINVAL = -1,      /* bad argument (shape, NULL, range) */
  SDR_EHIP = -2,        /* HIP runtime error */
  SDR_ENOMEM = -3,      /* device allocation failed */
  SDR_EUNSUPPORTED = -4, /* valid but not implemented configuration */
  SDR_EDOMAIN = -5       /* math domain error the reference raises (log10 of 0) */
};

enum { SDR_IQ_F32 = 0, SDR_IQ_U8 = 1 };                  /* interleaved IQ sample types */
enum { SDR_IQ_S8 = 2, SDR_IQ_S16 = 3 };                  /* raw capture types: accepted by sdr_ingest_create only */
enum { SDR_PRE_NONE = 0, SDR_PRE_SQUARE = 1, SDR_PRE_MIX = 2 }; /* FIR input pre-ops */
enum { SDR_REAL_F32 = 0, SDR_REAL_F64 = 1 };              /* real sample types (PSD) */
#define SDR_DFT_MAX_N (1 << 16)
#define SDR_MAX_RESAMPLE_TAPS 4096                           /* sdr_resample* filter length */

typedef struct sdr_ctx sdr_ctx;

/* ---- library / context ------------------------------------------------------- */
int sdr_abi_version(void);
const char* sdr_last_error(void);
int sdr_device_count(int* n);
/* Which physical GPU `device` is (bench.py's multi-rank line proves its rank -> device map
 * with it): its PCI bus id ("dddd:bb:dd.f", NUL-terminated into pci[len]) and compute units. */
int sdr_device_info(int device, char* pci, int len, int* cus);
int sdr_create(int device, sdr_ctx** out);
void sdr_destroy(sdr_ctx* ctx);
int sdr_synchronize(sdr_ctx* ctx);
void* sdr_stream(sdr_ctx* ctx); /* the hipStream_t all kernels of this context use */

/* ---- device memory and timing (replace the static float[5][307200] ring and the
 *      std::queue<void*> hand-off of src/fm_radio.cpp:22,51,86-145) ---------------- */
int sdr_malloc(sdr_ctx* ctx, int64_t bytes, void** out);
int sdr_free(sdr_ctx* ctx, void* p);
int sdr_memcpy_h2d(sdr_ctx* ctx, void* dst, const void* src, int64_t bytes);
int sdr_memcpy_d2h(sdr_ctx* ctx, void* dst, const void* src, int64_t bytes);
int sdr_memcpy_d2d(sdr_ctx* ctx, void* dst, const void* src, int64_t bytes); /* async */
int sdr_memset(sdr_ctx* ctx, void* dst, int value, int64_t bytes);          /* async */
int sdr_event_create(sdr_ctx* ctx, void** ev);
int sdr_event_record(sdr_ctx* ctx, void* ev);
int sdr_event_elapsed_ms(void* ev0, void* ev1, float* ms);
int sdr_event_destroy(void* ev);
/* The box's copy-kernel bandwidth (the roofline fraction beside a measured copy):
 * a 16-B-per-lane streaming copy of `bytes` on the context stream, best of `reps` after two
 * warm-ups; *gbs counts read + write.  Synchronous; allocates 2 x bytes for the call. */
int sdr_copy_bandwidth(sdr_ctx* ctx, int64_t bytes, int reps, double* gbs);
/* The read-only stream: `bytes` read once (16 B per lane, nontemporal, 8 loads in flight per
 * lane), best of `reps` after two warm-ups, GB/s.  The ceiling for kernels that read their
 * input once and write little (the front ends). */
int sdr_read_bandwidth(sdr_ctx* ctx, int64_t bytes, int reps, double* gbs);

/* ================================================================================
 * Host-buffer drop-in entry points (synchronous)
 * ================================================================================ */

/* RF front end: lfilter(rf_coeff, 1.0, iq[0::2], zi_i)[::decim], same for Q, then
 * fmDemodArctan(i_ds, q_ds, prev_phase).
 * Replaces model/fmMonoBlock.py:86-98 (model/fmSupportLib.py:15-44) and
 * src/fm_radio.cpp:66-84 -> src/filter.cpp:187-219 (convolveWithDecimIQ) +
 * src/rf_module.cpp:13-34 (fmDemodArctan).  iq: n complex samples interleaved,
 * f32 or u8 ((u8-128)/128, src/iofunc.cpp:61-69).  zi_i/zi_q (taps-1, in/out) may
 * both be NULL (zero initial state, no state out); prev_phase may be NULL (0.0).
 * demod: ceil(n/decim) floats; i_ds/q_ds (optional, both or neither): the decimated
 * filter outputs.  Fast tiled kernel for taps 101/151 at decim 10; other f32 shapes
 * use the generic kernels; u8 needs the fast shape (else SDR_EUNSUPPORTED). */
int sdr_rf_frontend(sdr_ctx* ctx, const void* iq, int iq_dtype, int64_t n, const double* b,
                    int taps, int decim, double* zi_i, double* zi_q, double* prev_phase,
                    float* demod, float* i_ds, float* q_ds);

/* lfilter(b, 1.0, x, zi)[::decim] on a real f32 stream.
 * Replaces model/fmMonoBlock.py:101-105 (audio), :117/:151 (stereo BPFs, decim 1),
 * model/fmRDSblock.py:156/:164/:180/:202 and src/filter.cpp:96-185
 * (convolveFIR, convolveWithDecim, convolveWithDecimPointer). */
int sdr_lfilter_decim(sdr_ctx* ctx, const float* x, int64_t n, const double* b, int taps,
                      int decim, double* zi_inout, float* y);

/* First-order IIR section: scipy.signal.lfilter([b0, b1], [1, a1], x, zi), i.e.
 *   y[n] = b0 x[n] + z[n-1],  z[n] = b1 x[n] - a1 y[n],
 * the state a single f64 in lfilter's zi / zf convention.  Samples f32 in and out, all
 * arithmetic f64 (a parallel scan over the row, csrc/audio.hip).  The FM de-emphasis filter
 * (design.deemphasis_coeffs: the bilinear transform of 1 / (1 + s tau), tau = 75 us or 50 us) is
 * such a section; the reference has no de-emphasis, so there is no reference interface
 * to name.  n >= 1, finite coefficients, |a1| <= 1; y must not overlap x.
 * zi_inout: NULL = zero initial state and no state out. */
int sdr_iir1(sdr_ctx* ctx, const float* x, int64_t n, const double* b /* [b0, b1] */, double a1,
             double* zi_inout, float* y);

/* lfilter with a fused input pre-op: PRE_SQUARE filters x*x
 * (model/fmRDSblock.py:161-164, src/filter.cpp:342-370), PRE_MIX filters
 * (x*mix)*gain (model/fmMonoBlock.py:155-160, model/fmRDSblock.py:173-182,
 * src/filter.cpp:373-401 convolveWithDecimAndMixer). */
int sdr_lfilter(sdr_ctx* ctx, const float* x, const float* mix, float gain, int pre, int64_t n,
                const double* b, int taps, int decim, double* zi_inout, float* y);

/* Rational resampler: lfilter(b, 1.0, zero-stuff(x, up), zi)[::down] * up, without
 * materialising the zero-stuffed stream; zi lives on the upsampled stream.
 * Replaces model/fmRDSblock.py:184-199 and src/filter.cpp:301-339
 * (convolveWithDecimMode1RDS), and the mode-1 audio resampler src/filter.cpp:222-298
 * (convolveWithDecimMode1[Pointer], 24/125 at 6 MHz, src/fm_radio.cpp:174-180, :228) whose
 * output is y/up (the reference applies the up gain at the int16 conversion, :297).
 * taps <= SDR_MAX_RESAMPLE_TAPS.  y: ceil(n*up/down) floats. */
int sdr_resample(sdr_ctx* ctx, const float* x, int64_t n, const double* b, int taps, int up,
                 int down, double* zi_inout, float* y);

/* fmDemodArctan(I, Q, prev_phase): model/fmSupportLib.py:15-44
 * (C++: src/rf_module.cpp:13-34, which is a non-arctan approximation; this follows
 * the Python model).  prev_phase in/out (NULL = 0.0, no state out). */
int sdr_fm_demod(sdr_ctx* ctx, const float* I, const float* Q, int64_t n, double* prev_phase,
                 float* out);

/* fmPll(pllIn, freq, Fs, state, ncoScale, phaseAdjust, normBandwidth):
 * model/fmPll.py:4-46 (C++ src/helper.cpp:13-57 fmPLL, src/helper.h:17-19 state).
 * state6 = [integrator, phaseEst, feedbackI, feedbackQ, ncoOut[0], trigOffset], in/out.
 * nco_i/nco_q: n+1 floats (index 0 = carried value); nco_q may be NULL. */
int sdr_pll(sdr_ctx* ctx, const float* in, int64_t n, double freq, double fs, double nco_scale,
            double phase_adj, double norm_bw, double* state6, float* nco_i, float* nco_q);

/* How the context's PLL calls were solved (device counters, accumulated since the context was
 * created or last reset; sdr_pll*, and the receivers built on the context).  A recurrence is
 * one (stream, PLL) of a call, or one pseudo-block of a long call (n > SDR_PLL_BLOCK_MAX =
 * 16 385 samples, which is cut into pseudo-blocks solved in parallel and chained).
 *   RECURRENCES   recurrences solved
 *   SPEC_R0..R2   ... by the parallel solve (guess + scan + check) in its 1st / 2nd / 3rd round
 *   SEQUENTIAL    ... by the sequential kernel (the fallback: acquisition, 0 / NaN input)
 *   LONG_GUESSED  long calls: pseudo-blocks kept as solved from their pre-roll start guess
 *                 (start within the acceptance bound of the chained state after a 2 pi shift)
 *   LONG_CHAINED  long calls: pseudo-blocks completed from the start the chain computed (the
 *                 linear response to the start error added, or solved again from it)
 *   LONG_MAXGAP   largest bound on the phase deviation between a pseudo-block's solved start
 *                 and the chained state among those kept as solved (radians, the bits of an f64)
 *   LONG_STOPS    long calls: pseudo-blocks whose start guess was beyond the linear bound (the
 *                 chain stopped there that round and re-solved it from the exact start)
 *   LONG_TAIL     long calls: pseudo-blocks left after the rounds, solved sequentially from the
 *                 chain's exact position (also counted in SEQUENTIAL)
 *   LONG_LINEAR   long calls: pseudo-blocks completed by the linear response to their start
 *                 error (every step's wrap further than the deviation bound: also in CHAINED)
 * out: SDR_PLL_NSTATS int64 (LONG_MAXGAP: reinterpret as double).  Synchronises the context
 * stream; reset != 0 zeroes the counters after reading. */
enum {
  SDR_PLL_ST_RECURRENCES, SDR_PLL_ST_SPEC_R0, SDR_PLL_ST_SPEC_R1, SDR_PLL_ST_SPEC_R2, SDR_PLL_ST_SEQUENTIAL,
  SDR_PLL_ST_LONG_GUESSED, SDR_PLL_ST_LONG_CHAINED, SDR_PLL_ST_LONG_MAXGAP, SDR_PLL_ST_LONG_STOPS,
  SDR_PLL_ST_LONG_TAIL, SDR_PLL_ST_LONG_LINEAR, SDR_PLL_NSTATS
};
int sdr_pll_stats(sdr_ctx* ctx, int64_t* out, int reset);

/* Fused mono block: RF front end + audio lfilter + [::audio_decim], intermediate demod
 * kept in HBM.  Replaces the body of model/fmMonoBlock.py:80-109 (one loop
 * iteration) and src/fm_radio.cpp:66-84 + :258.  demod_out optional. */
int sdr_mono_block(sdr_ctx* ctx, const void* iq, int iq_dtype, int64_t n, const double* rf_b,
                   int rf_taps, int rf_decim, double* zi_i, double* zi_q, double* prev_phase,
                   const double* audio_b, int audio_taps, int audio_decim, double* audio_zi,
                   float* demod_out, float* audio_out);

/* ================================================================================
 * Device-pointer entry points (asynchronous on the context stream)
 * Batched over `nstreams` independent streams laid out `stride` elements apart.
 * `hist` = number of valid samples in memory before each stream's index 0 (0: zero
 * pre-history as lfilter).  zf may alias zi (handled through scratch).
 * ================================================================================ */
int sdr_rf_frontend_dev(sdr_ctx* ctx, const void* iq, int iq_dtype, int64_t n, int64_t stride,
                        int64_t hist, int nstreams, const double* b, int taps, int decim,
                        const double* zi_i, const double* zi_q, int64_t zi_stride, double* zf_i,
                        double* zf_q, double* prev_phase, float* demod, int64_t out_stride,
                        float* i_ds, float* q_ds);

/* Fused continuous-stream mono receiver: per stream,
 *   audio = lfilter(audio_b, 1, fmDemodArctan(lfilter(rf_b, 1, I)[::rf_decim],
 *                                             lfilter(rf_b, 1, Q)[::rf_decim]))[::audio_decim]
 * with zero initial filter/demod state -- model/fmMonoBasic.py:70-111 (whole-signal mono
 * path; per block: model/fmMonoBlock.py:86-105, src/fm_radio.cpp:66-84).  The demodulated
 * stream stays on chip (f32 IQ, rf_taps 101/151 at decim 10, audio 151 taps at decim 5);
 * other configurations run the front end into scratch HBM, then the audio filter.
 * audio: nstreams x audio_stride floats, ceil(ceil(n/rf_decim)/audio_decim) per stream. */
/* 1 if sdr_fe_mono_dev runs the single fused kernel for this configuration (16-B aligned f32
 * / 4-B aligned u8 IQ rows, even stride), 0 if it runs the front end + audio FIR pair. */
int sdr_fe_mono_fused(int rf_taps, int rf_decim, int audio_taps, int audio_decim);
int sdr_fe_mono_dev(sdr_ctx* ctx, const void* iq, int iq_dtype, int64_t n, int64_t stride, int nstreams,
                    const double* rf_b, int rf_taps, int rf_decim, const double* audio_b, int audio_taps,
                    int audio_decim, float* audio, int64_t audio_stride);

int sdr_fir_dev(sdr_ctx* ctx, const float* x, const float* mix, float gain, int pre, int64_t n,
                int64_t x_stride, int64_t hist, int nstreams, const double* b, int taps, int decim,
                const double* zi, int64_t zi_stride, double* zf, float* y, int64_t y_stride);

int sdr_resample_dev(sdr_ctx* ctx, const float* x, int64_t n, const double* b, int taps, int up,
                     int down, const double* zi, double* zf, float* y);

int sdr_fm_demod_dev(sdr_ctx* ctx, const float* I, const float* Q, int64_t n, int64_t stride,
                     int nstreams, double* prev_phase, float* out, int64_t out_stride);

int sdr_pll_dev(sdr_ctx* ctx, const float* in, int64_t n, int64_t in_stride, int nstreams,
                double freq, double fs, double nco_scale, double phase_adj, double norm_bw,
                double* state, float* nco_i, float* nco_q, int64_t out_stride);

/* Stereo combiner, intended form of model/fmMonoBlock.py:166-170 (as in
 * src/fm_radio.cpp:250-251): left = (mono+side)/2, right = (mono-side)/2. */
int sdr_stereo_combine_dev(sdr_ctx* ctx, const float* mono, const float* side, int64_t n,
                           float* left, float* right);

/* sdr_iir1 on nstreams device rows (x_stride / y_stride >= n floats apart); zi, zf: nstreams
 * doubles (zi NULL = zero state, zf NULL = no state out, zf may alias zi).  y must not overlap
 * x.  Three launches for rows longer than one 2 048-sample tile (tile end states, one wave per
 * row chaining them, apply), one otherwise; no workgroup waits for another inside a launch. */
int sdr_iir1_dev(sdr_ctx* ctx, const float* x, int64_t n, int64_t x_stride, int nstreams,
                 const double* b, double a1, const double* zi, double* zf, float* y, int64_t y_stride);

/* Audio output stage: the rows left / right (nstreams rows each, `stride` floats apart; right
 * NULL = mono, left on both PCM channels) through the first-order section b, a1 (b NULL = no
 * filter), in any combination into the f32 rows left_out / right_out (same stride; must not
 * overlap the inputs) and the interleaved int16 PCM rows L0 R0 L1 R1 .. (2 n values per stream,
 * pcm_stride >= 2 n int16 elements apart).  state: [nstreams][2] doubles (L, R; in and out),
 * required with a filter.  PCM rule, on the f32 sample x the stage wrote (or read, b NULL):
 * v = x * 16384.0f in f32; NaN -> 0; v >= 32767 -> 32767; v <= -32768 -> -32768; otherwise
 * truncation toward zero -- for finite in-range samples the conversion of
 * src/fm_radio.cpp:286-302, and a defined result (saturation) where that one is undefined.
 * SDR_EINVAL: n < 1, nstreams < 1, stride < n, pcm_stride < 2 n, non-finite coefficients,
 * |a1| > 1, a filter without state, right_out without right, no output requested. */
int sdr_audio_out_dev(sdr_ctx* ctx, const float* left, const float* right, int64_t n, int64_t stride,
                      int nstreams, const double* b, double a1, double* state, float* left_out,
                      float* right_out, int16_t* pcm, int64_t pcm_stride);

/* ---- stereo blend and noise mute from each stream's MPX quality --------------------------
 * What a tuner does with its signal meter, on the device: sdr_blend_update_dev reads one
 * one-sided power spectrum per stream (nbins = nfft / 2 + 1 f32, rows `stride` floats apart: what
 * sdr_rspec_process_dev writes with navg 0 from a receiver's SDR_RX_O_DEMOD rows), computes the
 * stream's quality in f64 -- bin k, centred on k fs / nfft, belongs to a band if its centre lies
 * in the closed interval; a ratio is 10 log10(sum(band) / (median(guard) x bins in band)): the
 * pilot in 18.5 - 19.5 kHz against 16 - 18 kHz and 20 - 22 kHz, RDS in 55 - 59 kHz against
 * 60 - 64 kHz; the median is the mean of the two middle values for an even count; noise_floor is
 * the pilot guard's median -- and from it the targets
 *   target_g = clip((pilot_db - blend_lo_db) / (blend_hi_db - blend_lo_db), 0, 1)
 *   target_m = clip((mute_hi_db - 10 log10(noise_floor)) / (mute_hi_db - mute_lo_db), 0, 1)
 * (a NaN gives target 0; mute off: m is 1 always), smoothed for g and m alike:
 *   prev <- cur;  cur <- cur + k (target - cur),  k = attack if target < cur, else release.
 * NaN and zero floors give what IEEE arithmetic gives; a NaN in a row reaches that row's values
 * only.  One launch per update, one wave per stream (csrc/blend.hip); no host synchronisation.
 * State per stream, f64, device: SDR_BLEND_NSTATE values {pilot_db, rds_db, noise_floor, g_prev,
 * g, m_prev, m, n_updates}; after create / reset all 0 (mono until a pilot has been seen), except
 * m_prev = m = 1 with mute off.  sdr_blend_gains_dev: the device array [nstreams][4] =
 * {g_prev, g, m_prev, m} that sdr_audio_blend_dev ramps over a block.
 * Parameters (NULL = defaults): blend 15 / 25 dB (15: mpx_quality's lamp threshold), mute off
 * (mute_lo_db = mute_hi_db = +inf; on: both finite, full volume at or below mute_lo_db, silence at or
 * above mute_hi_db), attack 1, release 0.25.  SDR_EINVAL: non-finite blend limits, lo >= hi (blend;
 * mute when on), attack or release outside (0, 1], mute limits neither both finite nor both +inf.
 * sdr_blend_update_dev, SDR_EINVAL before any device work: NULL power, nbins < 3, stride < nbins,
 * fs not positive and finite, fs / 2 <= 64 kHz, bins wider than 500 Hz (as mpx_quality), a guard of
 * more than SDR_BLEND_MAX_GUARD bins.  sdr_blend_reset and sdr_blend_update_dev are asynchronous
 * on the context stream; sdr_blend_state (host [nstreams][SDR_BLEND_NSTATE]) synchronises. */
#define SDR_BLEND_NSTATE 8
#define SDR_BLEND_MAX_GUARD 1024
typedef struct sdr_blend_params {
  double blend_lo_db, blend_hi_db, mute_lo_db, mute_hi_db, attack, release;
} sdr_blend_params;
typedef struct sdr_blend sdr_blend;
int  sdr_blend_create(sdr_ctx* ctx, int nstreams, const sdr_blend_params* params, sdr_blend** out);
void sdr_blend_destroy(sdr_blend* blend);
int  sdr_blend_reset(sdr_blend* blend);
int  sdr_blend_update_dev(sdr_blend* blend, const float* power, int nbins, int64_t stride, double fs);
int  sdr_blend_state(sdr_blend* blend, double* host);
int  sdr_blend_gains_dev(sdr_blend* blend, const double** dev);
/* sdr_audio_out_dev with the gains applied in the same pass (same argument rules and launch
 * count; SDR_EINVAL also for NULL gains_dev): with gains_dev[s] = {g0, g1, m0, m1}, sample i of n
 * of stream s becomes, in f64 and rounded once to f32,
 *   t = (i + 1) / n,  g = g0 + (g1 - g0) t,  m = m0 + (m1 - m0) t
 *   L' = (float)(m ((L + R) / 2 + g (L - R) / 2)),  R' = (float)(m ((L + R) / 2 - g (L - R) / 2))
 * (mono, right NULL: L' = (float)(m L)), and that f32 is what the section filters, or with b NULL
 * what is written and converted by the PCM rule.  All gains 1 give L and R (exactly whenever the
 * f64 sums L + R and L - R are exact: always, unless one channel is below 2^-29 of the other);
 * g0 = g1 = 0 gives two bit-identical channels. */
int sdr_audio_blend_dev(sdr_ctx* ctx, const float* left, const float* right, int64_t n, int64_t stride,
                        int nstreams, const double* b, double a1, double* state, float* left_out,
                        float* right_out, int16_t* pcm, int64_t pcm_stride, const double* gains_dev);

/* ---- multi-stream block receiver ----------------------------------
 * The per-block loops of model/fmMonoBlock.py:80-173 (mono, stereo; intended L/R combiner)
 * and model/fmRDSblock.py:127-204 (RDS up to the RRC output) for `nstreams` independent
 * streams at once, every filter state, demod phase and PLL state carried in HBM from block
 * to block (C++: the rf / mono_stereo / rds threads of src/fm_radio.cpp:31-441, 783-792).
 * One block of all streams is a fixed chain of ~10 launches on the context stream,
 * whatever nstreams is: the FE, one launch per stage for all filters of that stage (with
 * their lfilter final states), and one lane per PLL recurrence.
 *   flags: SDR_RX_AUDIO (mono audio), SDR_RX_STEREO (implies AUDIO), SDR_RX_RDS.
 *   Filters (taps f64, designed by the caller, <= SDR_MAX_TAPS, set before the first block):
 *   SDR_RX_F_RF (+ rf_decim), F_AUDIO (+ audio_decim), F_PILOT, F_STEREO_BPF, F_STEREO_LPF
 *   (decim audio_decim), F_RDS_EXTRACT, F_RDS_SQUARE, F_RDS_LPF, F_RDS_ANTI (on the
 *   x rds_up zero-stuffed stream, then [::rds_down] x rds_up), F_RDS_RRC.
 *   PLLs default to the reference's: stereo 19 kHz x2 BW 0.01 (fmMonoBlock.py:119), RDS
 *   114 kHz x0.5 phase pi/3.3-pi/1.5 BW 0.001 (fmRDSblock.py:167), both at Fs 240 kHz.
 * Outputs live in receiver-owned device memory, `stride` floats apart per stream, and are
 * overwritten by the next block: M = ceil(block/rf_decim) demod-rate samples (NCOs: M+1,
 * index 0 = the carried value), A = ceil(M/audio_decim) audio-rate, R = ceil(M*up/down)
 * RDS-rate.  Inputs: nstreams rows of `block` interleaved complex samples, iq_stride
 * complex samples apart (f32 or u8). */
typedef struct sdr_rx sdr_rx;
enum { SDR_RX_AUDIO = 1, SDR_RX_STEREO = 2, SDR_RX_RDS = 4 };
enum {
  SDR_RX_F_RF, SDR_RX_F_AUDIO, SDR_RX_F_PILOT, SDR_RX_F_STEREO_BPF, SDR_RX_F_STEREO_LPF,
  SDR_RX_F_RDS_EXTRACT, SDR_RX_F_RDS_SQUARE, SDR_RX_F_RDS_LPF, SDR_RX_F_RDS_ANTI, SDR_RX_F_RDS_RRC,
  SDR_RX_NFILTERS
};
enum {
  SDR_RX_O_DEMOD, SDR_RX_O_AUDIO,                                   /* fm_demod, audio_block */
  SDR_RX_O_BPF_RECOVERY, SDR_RX_O_STEREO_NCO, SDR_RX_O_BPF_EXTRACTION, SDR_RX_O_STEREO,
  SDR_RX_O_LEFT, SDR_RX_O_RIGHT,                                    /* fmMonoBlock.py:115-170 */
  SDR_RX_O_RDS_EXTRACT, SDR_RX_O_RDS_PRE_PLL, SDR_RX_O_RDS_NCO_I, SDR_RX_O_RDS_NCO_Q,
  SDR_RX_O_RDS_LPF_I, SDR_RX_O_RDS_LPF_Q, SDR_RX_O_RDS_RES_I, SDR_RX_O_RDS_RES_Q,
  SDR_RX_O_RDS_RRC_I, SDR_RX_O_RDS_RRC_Q,                           /* fmRDSblock.py:156-204 */
  SDR_RX_O_AUDIO_DE, SDR_RX_O_LEFT_DE, SDR_RX_O_RIGHT_DE,           /* sdr_rx_set_deemph */
  SDR_RX_NOUTPUTS
};
int sdr_rx_create(sdr_ctx* ctx, int nstreams, int64_t block, int iq_dtype, int flags, sdr_rx** out);
void sdr_rx_destroy(sdr_rx* rx);
int sdr_rx_set_filter(sdr_rx* rx, int which, const double* b, int taps);
int sdr_rx_set_decim(sdr_rx* rx, int rf_decim, int audio_decim, int rds_up, int rds_down);
int sdr_rx_set_pll(sdr_rx* rx, int which /* 0 stereo, 1 RDS */, double freq, double fs,
                   double nco_scale, double phase_adj, double norm_bw);
/* Audio output stage (off by default; set before the first block; b NULL = off): the
 * first-order section b = [b0, b1], a1 (sdr_iir1; FM de-emphasis) applied to the audio rows as
 * one tail step on the context stream after the combiner.  SDR_RX_O_AUDIO_DE / _LEFT_DE /
 * _RIGHT_DE are then ordinary output rows (A samples: the filtered SDR_RX_O_AUDIO / _LEFT /
 * _RIGHT; the L / R rows with SDR_RX_STEREO only, and a stereo receiver filters its mono row
 * only when SDR_RX_O_AUDIO_DE is kept, sdr_rx_set_keep), and sdr_rx_pcm gives the block's
 * interleaved int16 PCM (sdr_audio_out_dev's rule; L / R with SDR_RX_STEREO, else the mono row on
 * both channels; taken from the filtered rows): 2 A values per stream, *stride int16 apart.
 * The f64 states (per stream and row) live in receiver memory, carry from block to block and
 * are zeroed by sdr_rx_reset.  While the stage is off the three rows do not exist (SDR_EINVAL
 * from every call that names them, and from sdr_rx_pcm), occupy no memory and cost no launch. */
int sdr_rx_set_deemph(sdr_rx* rx, const double* b, double a1);
int sdr_rx_pcm(sdr_rx* rx, int16_t** dev, int64_t* stride, int64_t* n);
/* Stereo blend and noise mute in the audio output stage (off by default; set before the first
 * block; nfft 0 = off; params NULL = sdr_blend_create's defaults).  Needs SDR_RX_AUDIO, the audio
 * output stage (sdr_rx_set_deemph) and M >= nfft demod samples per block, nfft a power of two that
 * sdr_rspec and sdr_blend_update_dev accept at the multiplex rate of 240 kHz (512 .. 8192);
 * SDR_EINVAL otherwise (M: when the first block fixes the configuration).  Every block then
 * gets, on the context stream directly before the audio tail, an sdr_rspec of its
 * SDR_RX_O_DEMOD rows (periodic Hann, hop nfft / 2, navg 0) and an sdr_blend_update_dev of those
 * spectra, and the tail's sdr_audio_out_dev call becomes sdr_audio_blend_dev with the updated
 * gains: the block's quality sets the gain its own audio ramps to.  The results land in the
 * existing _DE rows and the PCM (SDR_RX_O_LEFT_DE / _RIGHT_DE, or SDR_RX_O_AUDIO_DE of a receiver
 * without SDR_RX_STEREO, which takes the mute gain alone); a stereo receiver's separately kept
 * SDR_RX_O_AUDIO_DE stays unblended.  The blend's memory is the receiver's own; sdr_rx_reset
 * resets its state.  sdr_rx_blend_state: sdr_blend_state of the receiver's blend (synchronises). */
int sdr_rx_set_blend(sdr_rx* rx, const sdr_blend_params* params, int nfft);
int sdr_rx_blend_state(sdr_rx* rx, double* host /* [nstreams][SDR_BLEND_NSTATE] */);
int sdr_rx_reset(sdr_rx* rx);                       /* all states back to the stream start */
int sdr_rx_process_dev(sdr_rx* rx, const void* iq, int64_t iq_stride);   /* async, device IQ */
int sdr_rx_process(sdr_rx* rx, const void* iq, int64_t iq_stride);       /* sync, host IQ */
/* sync, host IQ in and the `nout` requested outputs (which[i]: SDR_RX_O_*) out into
 * out[i] (nstreams rows, out_stride[i] floats apart; NULL out_stride = packed), through
 * pinned staging with one wait: the per-block drop-in call of fmMonoBlock.py's loop */
int sdr_rx_run(sdr_rx* rx, const void* iq, int64_t iq_stride, int nout, const int* which,
               float* const* out, const int64_t* out_stride);
/* The same without waiting for the block: the IQ is copied into one of two pinned slots and
 * the chain is launched; then the PREVIOUSLY submitted block is waited for and its outputs
 * written into the buffers given with it, and the call returns (so the host prepares block
 * k+1 while block k runs: the reference's rf / audio thread overlap, src/fm_radio.cpp:783-792).
 * The `out` buffers must stay valid until the next sdr_rx_submit / sdr_rx_flush / sdr_rx_run
 * returns.  sdr_rx_flush delivers the last submitted block.  nout <= SDR_RX_MAXOUT. */
enum { SDR_RX_MAXOUT = 32 };
int sdr_rx_submit(sdr_rx* rx, const void* iq, int64_t iq_stride, int nout, const int* which,
                  float* const* out, const int64_t* out_stride);
int sdr_rx_flush(sdr_rx* rx);
/* Submission depth (set before the first block; 1..3, default 1): sdr_rx_submit of block k
 * delivers block k-depth (not k-1), so `depth` blocks stay in flight while the host prepares
 * the next one -- the reference's RF thread running ahead of its audio thread through its
 * queue (src/fm_radio.cpp:783-792).  sdr_rx_flush delivers every block still in flight,
 * oldest first.  With depth >= 2 a pipelined receiver keeps three output row sets (block k's
 * rows stay valid until block k+3 is processed). */
int sdr_rx_set_depth(sdr_rx* rx, int depth);
/* Pipelined receiver (set before the first block): block k's front half (FE and the
 * filters of the demod) runs on a second stream, its PLLs on a third once block k-1's PLLs
 * are done, and its stereo / RDS stages on the context stream -- so block k's PLLs start
 * while block k-1's stages C-E and block k+1's front half run; the output rows alternate
 * between two sets
 * (sdr_rx_output gives the latest block's; block k's stay valid until block k+2 is
 * processed).  sdr_rx_process_dev then does NOT order the front half after earlier work on
 * the context stream: its IQ must be ready when it is called (device-resident data, or an
 * upload that has been waited for).  The back half and everything after it on the context
 * stream see block k complete, as without pipelining.
 * Readers of the rows: work enqueued on the context stream between sdr_rx_process_dev(k) and
 * sdr_rx_process_dev(k+1) sees block k's rows, every one of them, however far the host runs
 * ahead of the GPU -- the call for block k+1 orders the launches that will overwrite the row
 * set (block k+nq's front half and PLLs, nq = 2 or 3 row sets) after it.  Work enqueued later
 * than that call, or on another stream, has no such guarantee: wait for the context stream
 * before block k+nq is processed. */
int sdr_rx_set_pipeline(sdr_rx* rx, int on);
int sdr_rx_output(sdr_rx* rx, int which, float** dev, int64_t* stride, int64_t* n);
int sdr_rx_fetch(sdr_rx* rx, int which, float* host, int64_t host_stride); /* sync, all streams */
/* Outputs sdr_rx_process_dev materialises (bit 1 << SDR_RX_O_*; default: every output of the
 * flags).  The NCO rows (SDR_RX_O_STEREO_NCO, _RDS_NCO_I/_Q) and the RDS LPF rows (_RDS_LPF_I/_Q)
 * are intermediates the chain itself does not need: without them the mixers form the NCO
 * from the PLL phases where they stage their inputs and the RDS LPF runs inside the composite
 * LPF + x19/80 resampler, so neither round-trips through HBM.  On spans (rows of >= 32 768
 * demod samples, the matrix-core tiles) the PLLs' f32 input rows (SDR_RX_O_BPF_RECOVERY,
 * _RDS_PRE_PLL) are such intermediates too: the loops read their inputs as one sign-code
 * byte per sample, which the producing tiles always store (the other outputs, which later
 * stages read, are always written; every output's values are the same either way).
 * sdr_rx_run / sdr_rx_submit materialise what they are asked for.  sdr_rx_fetch of an output
 * the latest block did not materialise is SDR_EINVAL (sdr_rx_output still gives its row). */
int sdr_rx_set_keep(sdr_rx* rx, uint64_t mask);
/* per-stage timing of the last block (HIP events between the receiver's launches, on the
 * context stream): FE, stage A (filters of demod), B (RDS square), PLL, C (mixers + LPFs),
 * D (resamplers), E (RRC); ms: SDR_RX_NSTAGES floats.  Timing adds event records between
 * launches; keep it off in measured loops. */
enum { SDR_RX_ST_FE, SDR_RX_ST_A, SDR_RX_ST_B, SDR_RX_ST_PLL, SDR_RX_ST_C, SDR_RX_ST_D, SDR_RX_ST_E,
       SDR_RX_NSTAGES };
int sdr_rx_set_timing(sdr_rx* rx, int on);
int sdr_rx_stage_ms(sdr_rx* rx, float* ms);
/* carried states (host copies; any may be NULL): demod prev_phase [nstreams], PLL states
 * [nstreams][6] in fmPll's order (model/fmPll.py:39-44) */
int sdr_rx_state(sdr_rx* rx, double* phase, double* pll_stereo, double* pll_rds);
/* sdr_pll_stats of the receiver's context, after waiting for every block in flight */
int sdr_rx_pll_stats(sdr_rx* rx, int64_t* out, int reset);

/* ---- capture ingest: raw sc8 / sc16 / u8 / f32 bytes to the f32 capture, with a level meter ----
 * The stage in front of sdr_iqc: the raw bytes of a capture block in device memory in, the block as
 * interleaved f32 out -- the buffer sdr_iqc / sdr_spec / sdr_ddc / sdr_pfb read -- and the level
 * meter a user sets the front end's gain by, taken where the ADC's codes are still seen.  The
 * reference has no such stage; the definition is rtsdr.ingest_model (capture.py):
 *   code c of a value x: SDR_IQ_U8 x - 128, SDR_IQ_S8 x (bits = 8 both); SDR_IQ_S16 x, a native
 *   little-endian int16 that holds a right-justified, sign-extended ADC code of `bits` bits, 2..16
 *   (16 unless params say otherwise; a 12-bit ADC: 12).  out = f32(c 2^-(bits - 1)), exact for
 *   every code; for u8 the project's (x - 128) / 128.  SDR_IQ_F32 passes through bit for bit, NaN
 *   and infinities included.  swap != 0 exchanges I and Q in out (a front end with an inverted
 *   spectrum); the meter is taken on the input and does not depend on it.
 *   meter of a call, integer types, all exact: n; clipped, the samples whose I or Q code is
 *   >= 2^(bits - 1) - 1 or <= -2^(bits - 1) (codes beyond a narrower `bits` count too); peak_code =
 *   max |c| over I and Q; sumsq_code = sum (cI^2 + cQ^2) (below 2^62); peak = peak_code 2^-(bits - 1)
 *   and sumsq = f64(sumsq_code) 2^-2(bits - 1); nonfinite = 0.
 *   meter of a call, f32: nonfinite, the samples with a non-finite I or Q, left out of everything
 *   else; clipped, |I| >= 1 or |Q| >= 1; peak, the largest |x|; sumsq, the f64 sum of the f64 squares
 *   in the kernels' fixed order; peak_code = sumsq_code = 0.
 *   carried from call to call: calls, total_n, total_clipped.  sdr_ingest_reset zeroes the meter.
 * Two launches per call (csrc/ingest.hip: the conversion with one partial record per workgroup,
 * then one wave that folds them), no host synchronisation, no atomics: the same call gives the same
 * bits.  With meter == 0 the stage is the conversion launch alone and the meter stays as reset left
 * it.  The block is cut into at most 2 048 chunks, none but the last shorter than
 * SDR_INGEST_CHUNK samples, one workgroup each.  sdr_ingest_process_dev: async; raw aligned to one
 * complex sample (2 B u8 / s8, 4 B s16, 8 B f32), out to 8 B; 1 <= n <= 2^31 - 1; all sample offsets
 * are 64-bit.  For f32, out == raw (in place) is allowed; any other overlap of the two extents is
 * refused.  sdr_ingest_meter_get synchronises; sdr_ingest_meter_dev: the device copy, for a
 * consumer on the stream.  Every other entry point that takes an iq_dtype refuses SDR_IQ_S8 and
 * SDR_IQ_S16.
 * SDR_EINVAL (before any device work): NULL pointers, bad dtype, bits outside 2..16 (s16) or not
 * the container's width (the other types; 0 stands for the container's width everywhere), n outside
 * [1, 2^31 - 1], a misaligned pointer, an overlap.  No host fallback. */
#define SDR_INGEST_CHUNK 4096
typedef struct sdr_ingest_params {
  int bits;    /* width of the ADC code in its container; 0: the container's width */
  int swap;    /* exchange I and Q in out */
  int meter;   /* take the level meter */
} sdr_ingest_params;  /* NULL: container width, 0, 1 */
typedef struct sdr_ingest_meter {
  int64_t n, clipped, nonfinite, peak_code;
  uint64_t sumsq_code;
  double peak, sumsq;
  int64_t calls, total_n, total_clipped;
} sdr_ingest_meter;
typedef struct sdr_ingest sdr_ingest;
int  sdr_ingest_create(sdr_ctx* ctx, int iq_dtype /* SDR_IQ_F32 | _U8 | _S8 | _S16 */, const sdr_ingest_params* params, sdr_ingest** out);
void sdr_ingest_destroy(sdr_ingest* ing);
int  sdr_ingest_reset(sdr_ingest* ing);                                                   /* async */
int  sdr_ingest_process_dev(sdr_ingest* ing, const void* raw, int64_t n, float* out);     /* async */
int  sdr_ingest_run(sdr_ingest* ing, const void* raw_host, int64_t n, float* out_host);   /* sync */
int  sdr_ingest_meter_get(sdr_ingest* ing, sdr_ingest_meter* host);                       /* synchronises */
int  sdr_ingest_meter_dev(sdr_ingest* ing, const sdr_ingest_meter** dev);

/* ---- IQ imbalance and DC offset correction of the capture -----------------------------------
 * The stage in front of sdr_spec / sdr_ddc / sdr_pfb: one block of a capture in device memory
 * (interleaved f32, or u8 as (x - 128) / 128) in, the same block as interleaved f32 out, with the
 * front end's DC offset removed and the Q branch's gain and phase error undone -- what keeps a
 * station at +f from leaving an image at -f in another channel of the bank, and the ADC's zero
 * out of the centre bin.  The estimate is blind: a sum of stations away from 0 Hz is a proper
 * complex signal (E[z^2] = 0), so whatever its second moments show beyond equal, uncorrelated I
 * and Q is the front end's, and one 2 x 2 real matrix undoes it.  The model is frequency-
 * independent: one matrix for the whole band.  The reference has no such stage; the definition
 * is rtsdr.IqBalance (iqbalance.py), in f64:
 *   state: smoothed raw moments m = (mI, mQ, pII, pQQ, pIQ); coefficients (dI, dQ, c1, c2),
 *   initially (0, 0, 0, 1); counters updates, skipped, holds.  A call of n samples, estimate != 0:
 *   1. r = (sum I, sum Q, sum I^2, sum Q^2, sum I Q) / n over the block.
 *   2. any of the five not finite: skipped += 1 and nothing else changes.  Else m = r on the
 *      first update, m = m + rate (r - m) later; updates += 1.
 *   3. A = pII - mI mI, B = pQQ - mQ mQ, C = pIQ - mI mQ, t = B - (C / A) C.  If A > 0, t > 0 and
 *      both are finite: c2 = sqrt(A / t), c1 = -(C / A) c2, dI = mI, dQ = mQ (dc == 0: dI = dQ = 0
 *      are installed; balance == 0: c1 = 0, c2 = 1).  Else the coefficients stay, holds += 1 (an
 *      all-zero block, a constant block, Q = I).
 *   4. the same block, with the coefficients just computed:
 *      I' = f32(I - dI), Q' = f32(c1 (I - dI) + c2 (Q - dQ)), evaluated in f64 as written and
 *      rounded once.  A NaN sample stays a NaN at that sample only.
 *   estimate == 0: step 4 only.  sdr_iqc_set installs coefficients (a front end calibrated once),
 *   sdr_iqc_reset returns to the initial state.
 * Three launches per call (csrc/iqc.hip: moments, update, apply), no host synchronisation, no
 * atomics: the same call gives the same bits.  The u8 moments are integer sums, so they equal
 * the definition's exactly; the f32 sums are f64 sums in the kernel's fixed order.  The block is
 * cut into at most 2 048 chunks, none but the last shorter than SDR_IQC_CHUNK samples, one
 * workgroup each.  sdr_iqc_process_dev: async; iq aligned to one complex sample (8 B f32, 2 B
 * u8), out to 8 B; out is the buffer sdr_spec / sdr_ddc / sdr_pfb_process_dev read.  For f32,
 * out == iq (in place) is allowed; any other overlap is refused.  n <= 2^31 - 1; all sample
 * offsets are 64-bit.  sdr_iqc_state (host [SDR_IQC_NSTATE]: mI mQ pII pQQ pIQ dI dQ c1 c2 updates
 * skipped holds) synchronises; sdr_iqc_coeffs_dev: the device array dI dQ c1 c2.
 * SDR_EINVAL (before any device work): NULL pointers, bad dtype, rate outside (0, 1] or not
 * finite, a non-finite coefficient, n < 1, a misaligned pointer, partial overlap.  No host
 * fallback. */
#define SDR_IQC_NSTATE 12
#define SDR_IQC_CHUNK 4096
typedef struct sdr_iqc_params {
  double rate;   /* the share of the way to the block's moments the smoothed ones move, in (0, 1] */
  int dc;        /* remove the DC offset */
  int balance;   /* undo the gain and phase error */
} sdr_iqc_params;  /* NULL: 0.125, 1, 1 */
typedef struct sdr_iqc sdr_iqc;
int  sdr_iqc_create(sdr_ctx* ctx, int iq_dtype /* SDR_IQ_F32 | SDR_IQ_U8 */, const sdr_iqc_params* params, sdr_iqc** out);
void sdr_iqc_destroy(sdr_iqc* iqc);
int  sdr_iqc_reset(sdr_iqc* iqc);                                            /* async */
int  sdr_iqc_set(sdr_iqc* iqc, const double coeff[4] /* dI dQ c1 c2, finite */); /* async */
int  sdr_iqc_process_dev(sdr_iqc* iqc, const void* iq, int64_t n, float* out, int estimate);   /* async */
int  sdr_iqc_run(sdr_iqc* iqc, const void* iq_host, int64_t n, float* out_host, int estimate); /* sync */
int  sdr_iqc_state(sdr_iqc* iqc, double* host /* [SDR_IQC_NSTATE] */);       /* synchronises */
int  sdr_iqc_coeffs_dev(sdr_iqc* iqc, const double** dev /* dI dQ c1 c2 */);
/* per-launch timing of the last call made with an estimate (HIP events between the three launches,
 * on the context stream): moments, update, apply; ms: 3 floats.  Timing adds event records between
 * launches; keep it off in measured loops. */
int  sdr_iqc_set_timing(sdr_iqc* iqc, int on);
int  sdr_iqc_stage_ms(sdr_iqc* iqc, float* ms);

/* ---- wideband channelizer (multi-channel digital down-converter) ---------------------
 * One interleaved-IQ capture (f32, or u8 as (x-128)/128) in, nch rows of interleaved complex
 * f32 at Fs/decim out, row c centred on freq[c]: per channel "mix down, lfilter(b, 1, .),
 * [::decim]",
 *   y_c[m] = sum_j b[j] x[m decim - j] exp(-i 2 pi phi_c(m decim - j)),
 * with x zero before the stream start and carried across calls, and the oscillator an integer
 * phase accumulator: inc_c = rint(freq[c] 2^32) mod 2^32, phi_c(k) = ((inc_c k) mod 2^32) / 2^32
 * turns at absolute sample index k (counted from the last reset) -- exact at any stream
 * position and across any split into calls.  The frequency used is signed(inc_c) / 2^32
 * (sdr_ddc_freq).  The reference has no channelizer: it is an addition, the stage a wideband
 * front end needs before `nstreams` receivers; the rows are laid out as sdr_rx_process_dev
 * reads its input rows (out_stride = its iq_stride, in complex samples).
 * One matrix-core GEMM launch per call for all channels (csrc/ddc.hip) plus the history
 * update; the object keeps the last taps-1 input samples, so the input is read in place.
 * Waves work on windows of SDR_DDC_WINDOW outputs (16 where 126 decim + 2 taps floats exceed
 * the wave's staging memory).  Samples must be finite and below 65 504 in magnitude (f16
 * operands).  sdr_ddc_process_dev: async; iq aligned to one complex sample (8 B f32, 2 B u8),
 * out to 8 B; channel c's n/decim samples start at out + 2 c out_stride floats.
 * SDR_EINVAL (before any device work): nch, taps, decim out of range, a non-finite tap or
 * frequency, |freq| > 0.5, bad dtype, n < 1, n % decim != 0, out_stride < n/decim, a reset
 * position that is negative or no multiple of decim.  No configuration inside the limits is
 * unsupported, and there is no host fallback. */
#define SDR_DDC_MAX_CH 64
#define SDR_DDC_MAX_TAPS 256
#define SDR_DDC_MAX_DECIM 64
#define SDR_DDC_WINDOW 64
typedef struct sdr_ddc sdr_ddc;
int sdr_ddc_create(sdr_ctx* ctx, int nch, const double* freq /* [nch], cycles/sample, |f| <= 0.5 */,
                   const double* b, int taps, int decim, int iq_dtype, sdr_ddc** out);
void sdr_ddc_destroy(sdr_ddc* ddc);
int sdr_ddc_freq(sdr_ddc* ddc, double* actual /* [nch]: signed(inc) / 2^32 */);
int sdr_ddc_reset(sdr_ddc* ddc, int64_t position);   /* zero history; position >= 0, % decim == 0 */
int sdr_ddc_position(sdr_ddc* ddc, int64_t* position);
int sdr_ddc_process_dev(sdr_ddc* ddc, const void* iq, int64_t n, float* out, int64_t out_stride);
int sdr_ddc_run(sdr_ddc* ddc, const void* iq_host, int64_t n, float* out_host, int64_t out_stride); /* sync */

/* ---- polyphase filter bank (uniformly spaced channels) ---------------------------------
 * The channelizer's companion for channels on a uniform grid: nbins bins across the capture,
 * bin k centred on k / nbins cycles per sample (bins >= nbins/2 are the negative frequencies),
 * nch of them selected (any order, repeats allowed), one real prototype filter b of `taps`
 * taps, decimation decim (any: it need not divide nbins, nor nbins it).  Per channel
 *   y_c[m] = sum_j b[j] x[m decim - j] exp(-2 pi i ((bin[c] (k mod nbins)) mod nbins) / nbins),
 *   k = position + m decim - j,
 * x zero before the stream start and carried across calls; the phase is integer arithmetic mod
 * nbins -- exact at any stream position and across any split into calls.  Computed as a
 * polyphase fold (the filter's MACs shared by all channels: `taps` real-by-complex MACs per
 * output time) and an nbins-point DFT for the selected bins on the matrix cores, one launch
 * per call (csrc/pfb.hip) plus the history update; the object keeps the last taps-1 input
 * samples, so the input is read in place.  Workgroups work on windows of SDR_PFB_WINDOW output
 * times (16 where the window's buffers exceed 80 KB of LDS).  Samples must be finite and
 * sum|b| max|x| below 65 504 (f16 operands).  Row layout, alignment and the call-time rules are
 * sdr_ddc_process_dev's: async; iq aligned to one complex sample (8 B f32, 2 B u8), out to 8 B;
 * n >= 1, n % decim == 0, out_stride >= n/decim; channel c's n/decim samples start at
 * out + 2 c out_stride floats -- the rows sdr_rx_process_dev reads.
 * SDR_EINVAL (before any device work): nbins, nch, taps, decim out of range, a bin outside
 * [0, nbins), a non-finite tap, bad dtype, NULL pointers, the call-time rules, a reset position
 * that is negative or no multiple of decim.  No configuration inside the limits is unsupported,
 * and there is no host fallback. */
#define SDR_PFB_MAX_BINS 256
#define SDR_PFB_MAX_CH 256
#define SDR_PFB_MAX_TAPS 4096
#define SDR_PFB_MAX_DECIM 64
#define SDR_PFB_WINDOW 64
typedef struct sdr_pfb sdr_pfb;
int sdr_pfb_create(sdr_ctx* ctx, int nbins, int nch, const int* bin /* [nch], 0 <= bin < nbins */,
                   const double* b, int taps, int decim, int iq_dtype, sdr_pfb** out);
void sdr_pfb_destroy(sdr_pfb* pfb);
int sdr_pfb_reset(sdr_pfb* pfb, int64_t position);   /* zero history; position >= 0, % decim == 0 */
int sdr_pfb_position(sdr_pfb* pfb, int64_t* position);
int sdr_pfb_process_dev(sdr_pfb* pfb, const void* iq, int64_t n, float* out, int64_t out_stride);
int sdr_pfb_run(sdr_pfb* pfb, const void* iq_host, int64_t n, float* out_host, int64_t out_stride); /* sync */

/* ---- rational resampler for device rows ---------------------------------------------------
 * nrows rows of f32 samples in device memory, real (elems = SDR_RSMP_REAL) or interleaved
 * complex (SDR_RSMP_COMPLEX), resampled by up / down through one real filter b of `taps` taps
 * designed at `up` times the input rate -- the stage between a channelizer whose fs / decim is
 * not the receiver's rate and the receiver (2.5 MS/s rows x 24/25 -> 2.4 MS/s), or N audio
 * streams 48 kHz -> 44.1 kHz (147/160).  Per row, sdr_resample's convention, gain included:
 *   y[m] = up sum_j b[j] xu[m down - j],   xu[i] = x[i / up] if up divides i, else 0
 * = up lfilter(b, 1, zero-stuff(x, up))[::down], x zero before the stream start and carried
 * across calls.  Computed in polyphase form, P = ceil(taps / up), b zero-padded to P up,
 * m down = s up + r with 0 <= r < up:
 *   y[m] = sum_{q < P} g[r + q up] x[s - q],   g = f32(up b)
 * an f32 FMA chain over q = 0 .. P - 1 per output and component (the first term a product), so
 * an output's bits depend only on the taps and on the P samples of its window: any split of a
 * stream into calls gives the same bits as one call.  A non-finite sample can make non-finite
 * only the outputs whose window x[s - P + 1 .. s] contains it.
 * Every call takes n >= 1 samples per row with n up % down == 0 and writes exactly n up / down
 * per row, so every call starts at phase 0.  The object keeps the last P - 1 input samples of
 * every row; the input is read in place.  One launch per call for all rows (csrc/rsmp.hip) plus
 * the history update; a workgroup produces up to SDR_RSMP_TILE outputs of one row as a unit.
 * Row r starts r stride samples (elems floats each) into its buffer -- sdr_ddc_process_dev's
 * rows, so complex output rows are what sdr_rx_process_dev reads with iq_stride = out_stride.
 * in and out are aligned to one sample (4 B real, 8 B complex); the in_stride - n and
 * out_stride - n up / down samples between rows are not read into any result and not written.
 * sdr_rsmp_process_dev: async on the context stream.  sdr_rsmp_run: host buffers, synchronous.
 * SDR_EINVAL (before any device work, history and position unchanged): nrows, elems, taps, up,
 * down out of range, ceil(taps / up) > SDR_RSMP_MAX_PHASE_TAPS, a non-finite tap, NULL
 * pointers, n < 1, n up % down != 0, n or n up / down >= 2^31, a stride shorter than its row,
 * misaligned pointers, out's extent overlapping in's.  No configuration inside the limits is
 * unsupported, and there is no host fallback. */
enum { SDR_RSMP_REAL = 1, SDR_RSMP_COMPLEX = 2 };   /* floats per sample */
#define SDR_RSMP_MAX_FACTOR 1024
#define SDR_RSMP_MAX_TAPS 4096
#define SDR_RSMP_MAX_PHASE_TAPS 256
#define SDR_RSMP_MAX_ROWS 65535
#define SDR_RSMP_TILE 2048
typedef struct sdr_rsmp sdr_rsmp;
int  sdr_rsmp_create(sdr_ctx* ctx, int nrows, int elems, const double* b, int taps, int up, int down, sdr_rsmp** out);
void sdr_rsmp_destroy(sdr_rsmp* rsmp);
int  sdr_rsmp_reset(sdr_rsmp* rsmp);                             /* zero history, position 0 */
int  sdr_rsmp_position(sdr_rsmp* rsmp, int64_t* in_samples);     /* taken per row since the last reset */
int  sdr_rsmp_process_dev(sdr_rsmp* rsmp, const float* in, int64_t n, int64_t in_stride, float* out, int64_t out_stride); /* async */
int  sdr_rsmp_run(sdr_rsmp* rsmp, const float* in_host, int64_t n, int64_t in_stride, float* out_host, int64_t out_stride); /* sync */

/* ---- wideband spectrum / waterfall ---------------------------------------------------------
 * Welch periodogram rows of one interleaved-IQ capture in device memory (f32, or u8 as
 * (x - 128) / 128) -- the buffer sdr_ddc_process_dev / sdr_pfb_process_dev read, in place: where
 * are the stations?  With segment s starting at sample s hop, s = 0 .. nseg - 1,
 * nseg = (n - nfft) / hop + 1, and the window w,
 *   X_s[k]    = sum_{i < nfft} w[i] x[s hop + i] exp(-2 pi i k i / nfft)
 *   out[r][j] = (1 / (navg (sum w)^2)) sum_{s in [r navg, (r + 1) navg)} |X_s[k]|^2,
 *   k = (j + nfft / 2) mod nfft
 * linear power in f32, bin j centred on (j - nfft / 2) fs / nfft (ascending, as a waterfall row
 * and np.fft.fftshift).  navg = 0: one row of all nseg segments.  rows = nseg / navg; trailing
 * segments that do not fill a row are ignored.  For hop <= nfft this is scipy.signal.spectrogram(
 * x, window=w, nperseg=nfft, noverlap=nfft-hop, detrend=False, return_onesided=False,
 * scaling='spectrum', mode='psd') averaged over groups of navg columns and shifted; hop > nfft
 * (a sparse monitor) skips samples.  Stateless: nothing is carried between calls.
 * nfft: a power of two in [SDR_SPEC_MIN_NFFT, SDR_SPEC_MAX_NFFT]; hop: 1 .. SDR_SPEC_MAX_HOP,
 * odd or even; navg: 0 or >= 1; window: nfft finite values of any sign with a non-zero sum, NULL
 * for the periodic Hann window 0.5 - 0.5 cos(2 pi i / nfft).
 * An f32 FFT on the device (csrc/spectrum.hip): radix-16 / 8 butterflies in registers, the turns
 * from a table computed in f64 on the host.  A workgroup takes a chunk of consecutive segments
 * of one row and adds their |X|^2 in a fixed order; a row of more than SDR_SPEC_SPLIT_SEGS
 * segments may be cut into several chunks (the call into about 2 048, none shorter than
 * SDR_SPEC_SPLIT_SEGS), whose sums a second launch adds in chunk order: no atomics, the same call
 * gives the same bits.  A non-finite sample makes every bin of its row NaN, and no other row.
 * sdr_spec_rows: host arithmetic only.  sdr_spec_process_dev: async; iq aligned to one complex
 * sample (8 B f32, 2 B u8), out to 4 B; row r starts r out_stride floats into out, and the
 * out_stride - nfft floats between rows are not written.  All sample offsets are 64-bit.
 * SDR_EINVAL (before any device work): nfft no power of two or out of range, hop or navg out of
 * range, a non-finite window value, a window that sums to zero, bad dtype, NULL pointers,
 * n < nfft, an n that yields no complete row, out_stride < nfft.  No configuration inside the
 * limits is unsupported, and there is no host fallback. */
#define SDR_SPEC_MIN_NFFT 64
#define SDR_SPEC_MAX_NFFT 8192
#define SDR_SPEC_MAX_HOP  (1 << 24)
#define SDR_SPEC_SPLIT_SEGS 8
typedef struct sdr_spec sdr_spec;
int  sdr_spec_create(sdr_ctx* ctx, int nfft, const double* window /* [nfft]; NULL = periodic Hann */,
                     int64_t hop, int64_t navg, int iq_dtype, sdr_spec** out);
void sdr_spec_destroy(sdr_spec* spec);
int  sdr_spec_rows(sdr_spec* spec, int64_t n, int64_t* nseg, int64_t* rows);      /* host arithmetic only */
int  sdr_spec_process_dev(sdr_spec* spec, const void* iq, int64_t n, float* out, int64_t out_stride); /* async */
int  sdr_spec_run(sdr_spec* spec, const void* iq_host, int64_t n, float* out_host, int64_t out_stride); /* sync */

/* ---- spectrum of rows of real samples (a receiver's demodulated rows) ----------------------
 * The same Welch periodogram for `nrows` rows of real f32 samples in device memory, one-sided, in
 * one call -- a receiver's "demod" rows (the FM multiplex at 240 kS/s), read in place: does a
 * stream hold a 19 kHz pilot, an RDS subcarrier?  Row q starts q in_stride floats into x.  With
 * segment s of row q starting at sample s hop, N = nfft and the window w,
 *   X_{q,s}[k]   = sum_{i < N} w[i] x_q[s hop + i] exp(-2 pi i k i / N),        k = 0 .. N / 2
 *   out[q][r][k] = (c_k / (navg (sum w)^2)) sum_{s in [r navg, (r + 1) navg)} |X_{q,s}[k]|^2,
 *   c_0 = c_{N/2} = 1, otherwise 2
 * linear power in f32, bin k centred on k fs / N.  For hop <= nfft this is
 * scipy.signal.spectrogram(x_q, window=w, nperseg=N, noverlap=N-hop, detrend=False,
 * return_onesided=True, scaling='spectrum', mode='psd') averaged over groups of navg columns.
 * nseg, navg = 0, rows, trailing segments, nfft, hop and window: as sdr_spec's, per row.
 * nrows: 1 .. SDR_RSPEC_MAX_ROWS.  Stateless.
 * The sdr_spec transform with two real segments of one row per complex transform (segment a the
 * real part, b the imaginary part: |A[k]|^2 + |B[k]|^2 = (|Z[k]|^2 + |Z[N-k]|^2) / 2, folded at
 * the final store); a pair lies inside one chunk of one output row, an odd count pairs the last
 * segment with zeros.  One launch over all rows, output rows and chunks, plus sdr_spec's second
 * launch where an output row is summed in chunks; the chunk rule counts the segments of all
 * nrows rows.  No atomics: the same call gives the same bits.  A non-finite sample makes every
 * bin of its output row NaN, and no other row.
 * sdr_rspec_rows: host arithmetic only; nseg and rows per input row.  sdr_rspec_process_dev:
 * async; x and out aligned to 4 B (rows at any 4-byte alignment; the in_stride - n floats between
 * rows are never read); output row (q, r) starts (q rows + r) out_stride floats into out and
 * holds nfft / 2 + 1 floats, the rest of the stride is not written.  All sample offsets are
 * 64-bit.  sdr_rspec_run: host rows in_stride floats apart, host output rows out_stride apart.
 * SDR_EINVAL (before any device work): nrows, nfft, hop or navg out of range, a non-finite window
 * value, a window that sums to zero, NULL pointers, n < nfft, an n that yields no complete row,
 * in_stride < n, out_stride < nfft / 2 + 1, a misaligned pointer.  No host fallback. */
#define SDR_RSPEC_MAX_ROWS 65535
typedef struct sdr_rspec sdr_rspec;
int  sdr_rspec_create(sdr_ctx* ctx, int nrows, int nfft, const double* window /* [nfft]; NULL = periodic Hann */,
                      int64_t hop, int64_t navg, sdr_rspec** out);
void sdr_rspec_destroy(sdr_rspec* rspec);
int  sdr_rspec_rows(sdr_rspec* rspec, int64_t n, int64_t* nseg, int64_t* rows);   /* host arithmetic only */
int  sdr_rspec_process_dev(sdr_rspec* rspec, const float* x, int64_t n, int64_t in_stride,
                           float* out, int64_t out_stride);                      /* async */
int  sdr_rspec_run(sdr_rspec* rspec, const float* x_host, int64_t n, int64_t in_stride,
                   float* out_host, int64_t out_stride);                         /* sync */

/* ---- modulation meter of rows of real samples (a receiver's demodulated or audio rows) -------
 * What a modulation monitor shows of each stream, taken from the rows where the receiver left
 * them: peaks, sums for the mean and the power, the share of samples beyond a limit, and the
 * histogram of the half-spans of consecutive windows (a 50 ms peak hold).  The reference has no
 * such stage; the definition is rtsdr.RowMeterModel (rowmeter.py).  Per stream, carried from call
 * to call until sdr_rmeter_reset:
 *   a sample is finite or not; a non-finite sample counts in nonfinite and nowhere else.
 *   the call: n finite samples; nonfinite; over, the finite samples with |x| > limit (f32); max and
 *   min (-inf / +inf without a finite sample); sum = sum f64(x) and sumsq = sum f64(x)^2, f64 sums
 *   in the kernels' fixed order; windows, the windows completed by the call.
 *   the totals: calls and the sums, maxima and minima of the calls' values; empty_windows.
 *   windows: the stream -- every sample, counted by a 64-bit position -- is cut into consecutive
 *   windows of `window` samples across calls.  A window that completes with a finite sample in it
 *   adds one to hist[min(nbins - 1, floor(f32(f32(f32(max - min) 0.5f) scale)))], max and min over
 *   its finite samples; one without counts in empty_windows.  wcount, wmax, wmin: the unfinished
 *   window.
 * Two launches per call (csrc/rmeter.hip), no host synchronisation, no atomics: the same calls give
 * the same bits.  The reduce launch cuts every row at the window boundaries: with window >=
 * SDR_RMETER_SEG a window is ceil(window / SDR_RMETER_CHUNK) equal chunks, one workgroup each; below
 * it a chunk is SDR_RMETER_CHUNK / window whole windows, one wave a window.  The fold launch is one
 * wave a stream.  sdr_rmeter_process_dev: async; row s starts s stride floats into rows; rows at
 * any 4-byte alignment; the stride - n floats between rows are never read; 1 <= n <= 2^31 - 1; all
 * offsets are 64-bit.  It may grow the object's work arrays, which waits for the stream once.
 * sdr_rmeter_run: host rows stride floats apart.  sdr_rmeter_records, _hist and _windows
 * synchronise.  sdr_rmeter_windows: the (min, max) pairs of the windows the latest call completed,
 * in order, stream s at host + 2 s cap, at most cap of them; counts[s] (may be NULL) is how many
 * the call completed; a window without a finite sample reads (+inf, -inf).  sdr_rmeter_state_dev:
 * the device arrays, for a consumer on the stream.
 * SDR_EINVAL (before any device work): NULL pointers, nstreams outside 1 .. SDR_RMETER_MAX_STREAMS,
 * window outside [SDR_RMETER_MIN_WINDOW, SDR_RMETER_MAX_WINDOW], nbins outside 1 ..
 * SDR_RMETER_MAX_BINS, a scale that is not finite and positive, a NaN limit, n outside
 * [1, 2^31 - 1], stride < n with more than one stream, a pointer not aligned to 4 B, cap < 0.  No
 * host fallback. */
#define SDR_RMETER_MAX_STREAMS 4096
#define SDR_RMETER_MIN_WINDOW 64
#define SDR_RMETER_MAX_WINDOW 16777216
#define SDR_RMETER_MAX_BINS 1024
#define SDR_RMETER_CHUNK 16384
#define SDR_RMETER_SEG 4096
typedef struct sdr_rmeter_params {
  int64_t window;   /* samples of a window */
  int nbins;        /* histogram bins per stream */
  float scale;      /* bins per unit of the row */
  float limit;      /* |x| beyond it counts in over */
} sdr_rmeter_params;
typedef struct sdr_rmeter_record {
  int64_t n, nonfinite, over, windows;                                    /* the latest call */
  double sum, sumsq;
  float max, min;
  int64_t calls, total_n, total_nonfinite, total_over, total_windows, empty_windows;
  double total_sum, total_sumsq;
  float total_max, total_min;
  int64_t wcount;                                                         /* the unfinished window */
  float wmax, wmin;
} sdr_rmeter_record;
typedef struct sdr_rmeter sdr_rmeter;
int  sdr_rmeter_create(sdr_ctx* ctx, int nstreams, const sdr_rmeter_params* params, sdr_rmeter** out);
void sdr_rmeter_destroy(sdr_rmeter* rm);
int  sdr_rmeter_reset(sdr_rmeter* rm);                                                       /* async */
int  sdr_rmeter_process_dev(sdr_rmeter* rm, const float* rows, int64_t stride, int64_t n);   /* async */
int  sdr_rmeter_run(sdr_rmeter* rm, const float* rows_host, int64_t stride, int64_t n);      /* sync */
int  sdr_rmeter_records(sdr_rmeter* rm, sdr_rmeter_record* host /* [nstreams] */);           /* synchronises */
int  sdr_rmeter_hist(sdr_rmeter* rm, uint64_t* host /* [nstreams][nbins] */);                /* synchronises */
int  sdr_rmeter_windows(sdr_rmeter* rm, float* host /* [nstreams][cap][2] */, int64_t cap, int64_t* counts /* [nstreams] */);
int  sdr_rmeter_state_dev(sdr_rmeter* rm, const sdr_rmeter_record** dev, const uint64_t** hist_dev);
/* per-launch timing of the last call (HIP events around the two launches, on the context stream):
 * reduce, fold; ms: 2 floats.  Keep it off in measured loops. */
int  sdr_rmeter_set_timing(sdr_rmeter* rm, int on);
int  sdr_rmeter_stage_ms(sdr_rmeter* rm, float* ms);

/* ---- cascade of second-order sections on rows of real samples ---------------------------------
 * scipy.signal.sosfilt(sos, x, zi) per row in f64, rounded once to f32: the pilot notch, a sharp
 * audio low-pass, a DC blocker, the K-weighting of ITU-R BS.1770 on a receiver's audio rows.  The
 * reference has no such stage; the definition is rtsdr.sos_model (sosfilter.py).  sos: K rows of
 * (b0, b1, b2, 1, a1, a2), 1 <= K <= SDR_SOS_MAX_SECTIONS; the state is scipy's zi / zf (direct form
 * II transposed), [nrows][K][2] f64 on the device, carried from call to call until sdr_sos_reset.
 * Three launches per call (csrc/sos.hip): the tiles of SDR_SOS_TILE samples from zero state
 * (reduce), one wave per row that chains their end states (carry), every tile from its true state
 * (apply); rows of one tile take the apply launch alone.  No atomics, no waiting between
 * workgroups: the same calls give the same bits.  Every stride power of the recursion is formed on
 * the host in long double and rounded once (a table per coefficient set, cached on the context).
 * A NaN sample makes the rest of its row NaN, as scipy's loop does, and no other row.
 * sdr_sos_process_dev: async; row s starts s x_stride floats into x and s y_stride into y; rows at
 * any 4-byte alignment; the floats between rows are never touched; y == x filters in place; y ==
 * NULL stores nothing and only advances the state.  sdr_sos_run: host rows stride floats apart
 * (y_host may be NULL).  sdr_sos_state / _set_state synchronise.
 * SDR_EINVAL (before any device work): NULL pointers, nrows outside 1 .. SDR_SOS_MAX_ROWS, K
 * outside 1 .. SDR_SOS_MAX_SECTIONS, a non-finite coefficient, a0 != 1, a section with a pole on or
 * outside the unit circle (|a2| >= 1 or |a1| >= 1 + a2), n outside [1, 2^31 - 1], a stride < n, a
 * pointer not aligned to 4 B, y rows that overlap the x rows other than y == x with equal strides.
 * No host fallback. */
#define SDR_SOS_MAX_SECTIONS 4
#define SDR_SOS_MAX_ROWS 4096
#define SDR_SOS_TILE 2048
typedef struct sdr_sos sdr_sos;
int  sdr_sos_create(sdr_ctx* ctx, int nrows, const double* sos /* [K][6] */, int K, sdr_sos** out);
void sdr_sos_destroy(sdr_sos* f);
int  sdr_sos_reset(sdr_sos* f);                                                              /* async */
int  sdr_sos_process_dev(sdr_sos* f, const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t n);   /* async */
int  sdr_sos_run(sdr_sos* f, const float* x_host, float* y_host, int64_t stride, int64_t n); /* sync */
int  sdr_sos_state(sdr_sos* f, double* host /* [nrows][K][2] */);                            /* synchronises */
int  sdr_sos_set_state(sdr_sos* f, const double* host /* [nrows][K][2] */);                  /* synchronises */
/* per-launch timing of the last call: reduce, carry, apply; ms: 3 floats (0 for a launch a short
 * call skips).  Keep it off in measured loops. */
int  sdr_sos_set_timing(sdr_sos* f, int on);
int  sdr_sos_stage_ms(sdr_sos* f, float* ms);

/* ---- programme loudness of audio rows (ITU-R BS.1770 K-weighting, segment energies) ----------
 * Per stream and channel (1 or 2 rows of the same stride: ch0, ch1): the row through the two
 * K-weighting sections at 48 kHz (the cascade above, state carried), times 1 / `reference` -- the
 * row amplitude of PCM full scale, 2.0 for the output stage's x * 16384 -> int16 rule -- and the
 * f64 sum of squares of every completed segment of `segment` samples of stream position; the open
 * segment's partial sum and the position are carried.  The squares are of the f64 filter output,
 * not of a row rounded to f32.  The definition is rtsdr.LoudnessModel; rtsdr.loudness_report turns
 * the energies into momentary, short-term and gated integrated loudness (4 segments of 100 ms are
 * a 400 ms gating block).  The cascade's three launches (its apply launch also leaves, per tile,
 * the sums of squares on either side of the one segment boundary a tile can hold), then one wave
 * per stream that folds them in a fixed order into the open segment and a ring of the latest `cap`
 * completed segments.  sdr_loud_segments: the latest min(cap, completed) segment energies in
 * order, row (s, ch) at host + (s channels + ch) cap, *first the stream index of the first of them,
 * *count how many; synchronises.  sdr_loud_state_dev: the ring [nstreams][channels][cap] (segment g
 * at g % cap) and the open sums [nstreams][channels], for a consumer on the stream.
 * SDR_EINVAL (before any device work): NULL pointers (ch1 non-NULL with one channel, NULL with
 * two), nstreams outside 1 .. SDR_SOS_MAX_ROWS, channels not 1 or 2, segment outside
 * [SDR_LOUD_MIN_SEGMENT, SDR_LOUD_MAX_SEGMENT], cap outside [4, SDR_LOUD_MAX_CAP], a reference
 * that is not finite and positive, n outside [1, 2^31 - 1], stride < n, a pointer not aligned to
 * 4 B.  No host fallback. */
#define SDR_LOUD_MIN_SEGMENT 2048
#define SDR_LOUD_MAX_SEGMENT 16777216
#define SDR_LOUD_MAX_CAP 1048576
typedef struct sdr_loud_params {
  int64_t segment;    /* samples of a segment (4800: 100 ms at 48 kHz) */
  int cap;            /* completed segments kept per stream and channel */
  double reference;   /* row amplitude of full scale */
} sdr_loud_params;
typedef struct sdr_loud sdr_loud;
int  sdr_loud_create(sdr_ctx* ctx, int nstreams, int channels, const sdr_loud_params* params, sdr_loud** out);
void sdr_loud_destroy(sdr_loud* l);
int  sdr_loud_reset(sdr_loud* l);                                                            /* async */
int  sdr_loud_process_dev(sdr_loud* l, const float* ch0, const float* ch1 /* NULL: mono */, int64_t stride, int64_t n);   /* async */
int  sdr_loud_run(sdr_loud* l, const float* ch0_host, const float* ch1_host, int64_t stride, int64_t n);   /* sync */
int  sdr_loud_segments(sdr_loud* l, double* host /* [nstreams][channels][cap] */, int64_t* first, int64_t* count);
int  sdr_loud_state_dev(sdr_loud* l, const double** ring_dev, const double** open_dev);
/* per-launch timing of the last call: reduce, carry, apply, fold; ms: 4 floats */
int  sdr_loud_set_timing(sdr_loud* l, int on);
int  sdr_loud_stage_ms(sdr_loud* l, float* ms);

/* ---- true peak of audio rows (ITU-R BS.1770 annex 2: a polyphase interpolator, maxima only) ---
 * Per stream and channel (1 or 2 rows of the same stride: ch0, ch1) and per input sample at stream
 * position t (samples since the last reset, x[t] = 0 for t < 0) the `up` interpolated values
 *   y[t][p] = sum_{k = 0 .. taps - 1} f64(h[p][k]) f64(x[t - k]),   f64, from 0.0, k ascending
 * (an f32 x f32 product is exact in f64: fused or not, the same bits), of which only maxima are
 * kept: m[t] = max_p |y[t][p]| over the finite y (0.0 if none) and the sample peak q[t] = |x[t]|
 * (0.0 if x[t] is not finite).  A non-finite y counts in `nonfinite` and enters no maximum.  The
 * stream is cut into segments of `segment` samples of position; a segment's true peak is max m[t]
 * and its sample peak max q[t] over its samples.  The open segment's maxima, the position and the
 * last taps - 1 samples are carried from call to call on the device.  h = NULL: the 48-tap, 4-phase
 * table of BS.1770-4 annex 2 (up = 4, taps = 12; rtsdr.design.true_peak_fir), for 48 kHz rows.  The
 * definition is rtsdr.TruePeakModel, which the device equals bit for bit; rtsdr.true_peak_report
 * turns maxima into dBTP (the row amplitude of full scale is 2.0, as for sdr_loud).
 * Two launches per call (csrc/tpeak.hip): one workgroup per piece of a segment -- the pieces are
 * cut at the segment boundaries from the position the host carries -- forms the values in
 * registers and leaves one record; one wave per (stream, channel) folds the records into the open
 * segment, the ring of the latest `cap` completed segments (segment g at g % cap), the call's and
 * the totals' record, and stores the new history.  No atomics: the same calls give the same bits.
 * sdr_tpeak_process_dev: async; row (s, ch) starts s stride floats into ch0 / ch1; rows at any
 * 4-byte alignment; the stride - n floats between rows are never read; 1 <= n <= 2^31 - 1; all
 * offsets are 64-bit.  It may grow the object's work array, which waits for the stream once.
 * sdr_tpeak_run: host rows stride floats apart.  sdr_tpeak_records and _segments synchronise.
 * sdr_tpeak_segments: the latest min(cap, completed) segments' true and sample peaks in order, row
 * (s, ch) at host + (s channels + ch) cap, *first the stream index of the first of them, *count how
 * many.  sdr_tpeak_state_dev: the two rings [nstreams][channels][cap] and the records
 * [nstreams][channels], for a consumer on the stream.
 * SDR_EINVAL (before any device work): NULL pointers (ch1 non-NULL with one channel, NULL with
 * two), nstreams outside 1 .. SDR_SOS_MAX_ROWS, channels not 1 or 2, up outside 1 ..
 * SDR_TPEAK_MAX_UP, taps outside 1 .. SDR_TPEAK_MAX_TAPS (h = NULL: up and taps other than 4 and 12
 * or both 0), a non-finite coefficient, segment outside [SDR_LOUD_MIN_SEGMENT,
 * SDR_LOUD_MAX_SEGMENT], cap outside [4, SDR_LOUD_MAX_CAP], n outside [1, 2^31 - 1], stride < n, a
 * pointer not aligned to 4 B.  No host fallback. */
#define SDR_TPEAK_MAX_UP 8
#define SDR_TPEAK_MAX_TAPS 32
typedef struct sdr_tpeak_params {
  int up, taps;       /* phases, and taps of a phase */
  const float* h;     /* [up][taps]; NULL: BS.1770-4 annex 2, 4 x 12 */
  int64_t segment;    /* samples of a segment (4800: 100 ms at 48 kHz) */
  int cap;            /* completed segments kept per stream and channel */
} sdr_tpeak_params;
typedef struct sdr_tpeak_record {
  int64_t n, nonfinite;                                                   /* the latest call */
  double peak, sample_peak;
  int64_t calls, total_n, total_nonfinite;                                /* since the last reset */
  double total_peak, total_sample_peak;
  int64_t segments;                                                       /* completed since the last reset */
  double open_peak, open_sample_peak;                                     /* the unfinished segment */
} sdr_tpeak_record;
typedef struct sdr_tpeak sdr_tpeak;
int  sdr_tpeak_create(sdr_ctx* ctx, int nstreams, int channels, const sdr_tpeak_params* params, sdr_tpeak** out);
void sdr_tpeak_destroy(sdr_tpeak* tp);
int  sdr_tpeak_reset(sdr_tpeak* tp);                                                         /* async */
int  sdr_tpeak_process_dev(sdr_tpeak* tp, const float* ch0, const float* ch1 /* NULL: mono */, int64_t stride, int64_t n);   /* async */
int  sdr_tpeak_run(sdr_tpeak* tp, const float* ch0_host, const float* ch1_host, int64_t stride, int64_t n);   /* sync */
int  sdr_tpeak_records(sdr_tpeak* tp, sdr_tpeak_record* host /* [nstreams][channels] */);    /* synchronises */
int  sdr_tpeak_segments(sdr_tpeak* tp, double* peaks_host, double* sample_peaks_host /* [nstreams][channels][cap] */, int64_t* first,
                        int64_t* count);
int  sdr_tpeak_state_dev(sdr_tpeak* tp, const double** peaks_dev, const double** sample_peaks_dev, const sdr_tpeak_record** records_dev);
/* per-launch timing of the last call: reduce, fold; ms: 2 floats.  Keep it off in measured loops. */
int  sdr_tpeak_set_timing(sdr_tpeak* tp, int on);
int  sdr_tpeak_stage_ms(sdr_tpeak* tp, float* ms);

/* ---- spectral diagnostics -----------------------------------------
 * Bartlett PSD, model/fmSupportLib.py:66-140 (estimatePSD; the C++ src/fourier.cpp:36-110
 * advances sample and list positions by the same nfft/2 and is not the parity target):
 * floor(n/nfft) non-overlapping segments, Hann window pow(sin(i*pi/nfft), 2), FFT in f64,
 * 10*log10(2/(fs*nfft/2) * |X_k|^2) for k < nfft/2, averaged over segments in dB.
 * psd: nfft/2 doubles (NaN when n < nfft, as the reference's 0/0).  nfft: a power of two in
 * [2, SDR_PSD_MAX_NFFT = 4096].  SDR_EDOMAIN if a bin has zero power (the reference's
 * math.log10 raises).  The frequency axis np.arange(0, fs/2, fs/nfft) is the caller's.
 * sdr_psd: host f64 samples.  sdr_psd_dev: device samples (SDR_REAL_F32 / _F64), device psd. */
int sdr_psd(sdr_ctx* ctx, const double* x, int64_t n, int nfft, double fs, double* psd);
int sdr_psd_dev(sdr_ctx* ctx, const void* x, int dtype, int64_t n, int nfft, double fs, double* psd);

/* Direct DFT, model/fmSupportLib.py:46-60: X_m = sum_k x_k exp(i*2*pi*(-k*m)/n), f64, the
 * angle rounded as the reference's expression rounds it.  X: 2n doubles (re, im
 * interleaved = numpy complex128).  n <= SDR_DFT_MAX_N. */
int sdr_dft(sdr_ctx* ctx, const double* x, int64_t n, double* X);

/* ---- RDS link layer (host code) -----------------------------------
 * model/fmRDSblock.py:207-346 (src/fm_radio.cpp:444-729 frame_thread): per block of the
 * in-phase RRC output (57 kS/s, 24 samples per symbol), clock and data recovery from a
 * carried symbol offset, Manchester decoding of symbol pairs (with the carried lone
 * symbol), differential decoding, and the syndrome scan of every 26-bit window.
 * events: 3 int64 per syndrome match {type 0..3 = A..D, position, accepted}, where
 * accepted = 1 for the reference's "Syndrome X at position N" prints and 0 for its
 * "False positive" prints; positions count across blocks as the reference's printposition.
 * symbols / bits / diff (optional, NULL to skip): the sampled symbols, the Manchester bits
 * and the bits the scan saw (carried bits first), each count written to n_*.
 * The state (offset, start position, lone symbol, previous bit, carried bits, positions)
 * lives in the sdr_rds_link object; one object per stream.  No GPU is used. */
typedef struct sdr_rds_link sdr_rds_link;
enum { SDR_RDS_RESYNC = 4 };   /* event type of a re-sync (only with sdr_rds_link_set_resync) */
int sdr_rds_link_create(sdr_rds_link** out);
void sdr_rds_link_destroy(sdr_rds_link* link);
/* The C++ frame_thread's re-sync rule (src/fm_radio.cpp:697-704): after more than
 * `after_bad_syncs` false-positive syndromes since the last accepted one, forget the frame
 * position (the next syndrome is accepted) and emit an SDR_RDS_RESYNC event.  0 (default):
 * off, as the Python model (model/fmRDSblock.py:299-341), which has no such rule; the C++
 * uses 10. */
int sdr_rds_link_set_resync(sdr_rds_link* link, int after_bad_syncs);
int sdr_rds_link_block(sdr_rds_link* link, const double* rrc_i, int64_t n, int64_t* events,
                       int64_t max_events, int64_t* n_events, double* symbols, int64_t max_symbols,
                       int64_t* n_symbols, uint8_t* bits, int64_t max_bits, int64_t* n_bits,
                       uint8_t* diff, int64_t max_diff, int64_t* n_diff);

/* ---- RDS link layer on the device, for all streams of a call ---------------------------
 * The same link layer (sdr_rds_link_block is its specification, quirks included) for `nstreams`
 * rows of in-phase RRC output in device memory -- a receiver's "rrc_i" rows, read in place: row s
 * starts s * stride floats into rrc_i.  Every stream's state (symbol offset, start position,
 * front / previous bit, lone symbol, carried bits, positions, false-positive count, whether
 * block 0 has run) lives in device memory; bits, scanned bits, events and state equal the host
 * layer's, fed the same f32 samples widened to f64, call by call.  Three launches per call
 * whatever nstreams and n are (csrc/rds.hip).
 * sdr_rds_links_process_dev: async on the context stream; SDR_RDS_LINKS_MIN_N <= n <= max_n
 * (below the minimum the host layer can fail part-way through a state update; from it on only
 * on NaN), stride >= n; SDR_EINVAL before any device work otherwise.
 * sdr_rds_links_events (synchronises): the last call's events, ev[nstreams][max_events][4] =
 * {type 0..3 = A..D or SDR_RDS_RESYNC, position, accepted, word}, word = the window's 16
 * information bits, the first one most significant (0 for a re-sync); n_events[s] is the true
 * count -- beyond max_events the excess is dropped, the state still advances over every match
 * and status[s] has SDR_RDS_LINKS_OVERFLOW.  Where the host layer returns its NaN error (a NaN
 * among block 0's first 24 samples, or a last symbol that is NaN) status[s] has
 * SDR_RDS_LINKS_FAULT, the stream emits nothing and keeps its state, as the host layer does;
 * the other streams are unaffected.  NaN anywhere else compares false, as on the host.
 * sdr_rds_links_bits (synchronises): the last call's Manchester bits and scanned row (carried
 * bits first) of one stream, one byte per bit; either buffer may be NULL. */
#define SDR_RDS_LINKS_MIN_N 1536
#define SDR_RDS_LINKS_MAX_N (1 << 30)
#define SDR_RDS_LINKS_MAX_STREAMS 65535
#define SDR_RDS_LINKS_MAX_EVENTS (1 << 20)
#define SDR_RDS_LINKS_FAULT 1
#define SDR_RDS_LINKS_OVERFLOW 2
typedef struct sdr_rds_links sdr_rds_links;
int sdr_rds_links_create(sdr_ctx* ctx, int nstreams, int64_t max_n, int64_t max_events, sdr_rds_links** out);
void sdr_rds_links_destroy(sdr_rds_links* links);
int sdr_rds_links_set_resync(sdr_rds_links* links, int after_bad_syncs);   /* as sdr_rds_link_set_resync */
int sdr_rds_links_reset(sdr_rds_links* links);                             /* every stream back to block 0 */
int sdr_rds_links_process_dev(sdr_rds_links* links, const float* rrc_i, int64_t n, int64_t stride);
int sdr_rds_links_events(sdr_rds_links* links, int64_t* ev, int64_t* n_events, int32_t* status);
int sdr_rds_links_bits(sdr_rds_links* links, int stream, uint8_t* bits, int64_t max_bits, int64_t* n_bits,
                       uint8_t* diff, int64_t max_diff, int64_t* n_diff);

/* ---- RDS block synchronisation on the device, for all streams of a call -----------------
 * What a tuner does with the differential bits, where the link layer's frame rule stops at the
 * first damaged block: acquisition, a flywheel, the (26, 16) code's burst correction, offset C'.
 * The host model rdssync.py RdsBlockSync is the specification; records, state and counters equal
 * it after every call, whatever the split of a stream into calls (csrc/rds_sync.hip, two
 * launches per call).  Window p is D[p .. p + 25] of the stream's bits since reset, so positions
 * compare with sdr_rds_links event positions.  Slots: A 0, B 1, C and C' 2, D 3.
 *   SEARCH from s0 (0 after reset): the first p with p - 26 >= s0 whose window and the window
 *     26 bits before it have offset syndromes in consecutive slots gives two status-0 records
 *     and SYNC with the next block at p + 26.
 *   SYNC: the block of the expected slot every 26 bits: status 0 error-free, 1 corrected (an
 *     error pattern whose first and last flipped bits are at most max_burst - 1 apart), 2
 *     uncorrectable.  In slot 2 an exact C or C' syndrome decides the type; otherwise the version
 *     bit (bit 11) of the B word 26 bits before does, if that record is of this sync run and of
 *     status <= 1 (else status 2, type C).  bad_run counts blocks in a row that were not
 *     error-free; when it reaches lose_after the block's record is still emitted and SEARCH
 *     resumes with s0 behind it.
 * sdr_rds_sync_set_params: max_burst 0 .. SDR_RDS_SYNC_MAX_BURST (default 2), lose_after
 *   1 .. 255 (default 12); the host builds the 1024-entry syndrome table (synchronises).
 * sdr_rds_sync_process_dev: async on the context stream, nothing is read back.  Row s is the n
 *   bytes at bits + s * stride, only bit 0 of each counts; 0 <= n <= max_bits, stride >= n.
 *   counts_dev: NULL (every stream takes n bits) or a device array of per-stream counts 0 .. n.
 * sdr_rds_sync_process_links: every stream takes exactly the scanned bits the link bank's last
 *   call added (none where that call faulted); call it once after each link call.  Same context
 *   and stream count; max_bits must cover what a link call of the bank's max_n can add.
 * sdr_rds_sync_blocks (synchronises): the last call's records, rec[nstreams][max_records][4] =
 *   {type 0..3 = A..D or 4 = C', position, status, word after correction (as received for status
 *   2)}, max_records = max_bits / 26 + 3 (no call can give more), n_rec[s] of them valid.
 * sdr_rds_sync_state (synchronises): per stream synced[s], next_pos[s] (SYNC: the next block;
 *   SEARCH: s0) and counters[s][5] = blocks of status 0 / 1 / 2, acquisitions, losses since
 *   reset.  Any pointer may be NULL. */
#define SDR_RDS_SYNC_MAX_STREAMS 65535
#define SDR_RDS_SYNC_MAX_BITS (1 << 24)
#define SDR_RDS_SYNC_MAX_BURST 5
typedef struct sdr_rds_sync sdr_rds_sync;
int sdr_rds_sync_create(sdr_ctx* ctx, int nstreams, int64_t max_bits, sdr_rds_sync** out);
void sdr_rds_sync_destroy(sdr_rds_sync* sync);
int sdr_rds_sync_reset(sdr_rds_sync* sync);
int sdr_rds_sync_set_params(sdr_rds_sync* sync, int max_burst, int lose_after);
int sdr_rds_sync_process_dev(sdr_rds_sync* sync, const uint8_t* bits, int64_t n, int64_t stride, const int32_t* counts_dev);
int sdr_rds_sync_process_links(sdr_rds_sync* sync, sdr_rds_links* links);
int sdr_rds_sync_blocks(sdr_rds_sync* sync, int64_t* rec, int64_t* n_rec);
int sdr_rds_sync_state(sdr_rds_sync* sync, int32_t* synced, int64_t* next_pos, int64_t* counters);

/* ---- RDS symbol clock recovery on the device, for all streams of a call ------------------
 * The in-phase RRC rows (24 samples a symbol) -> differential bits, byte per bit, with an int32
 * count per stream, left in device memory for sdr_rds_sync_process_dev.  Where the link layer
 * fixes its sampling offset on the first 24 samples for ever, this stage follows the symbol clock.
 * The host model rdsclock.py RdsSymbolClock is the specification; bits, counts and state equal it
 * after every call, whatever the split of a stream into calls (csrc/rds_clock.hip, six launches
 * per call).  A stream is cut into segments of 768 samples (32 symbols) on its absolute sample
 * grid; only complete segments are worked on, the rest is carried.
 *   Energy: E_g[p] = sum of x[768 g + 24 j + p]^2 over j = 0 .. 31 ascending, in f64, a
 *     non-finite sample counting as 0; A_g = the E of the last min(window, g + 1) segments, oldest
 *     first; phat_g = the first maximum of A_g.
 *   Tracking: phi_0 = phat_0; later phi moves one sample (mod 24) towards phat_g when they are 2
 *     or more apart.  Segment g gives the samples x[768 g + 24 j + phi_g], j = j0 .. 31, j0 = 0
 *     but 1 when phi stepped 23 -> 0 and -1 when it stepped 0 -> 23: instants 23 .. 25 apart.
 *   Pairing: over the symbol pairs (m, m + 1) whose second symbol lies in the last
 *     min(window, g + 1) segments, C0 / C1 count those with even / odd m whose samples differ in
 *     (x > 0).  Segment 0 sets pi = 0 if C0 >= C1 else 1; later pi moves when the other count
 *     leads by more than `hysteresis`.  A pair with m = pi (mod 2) whose first symbol no pair has
 *     used gives bit = x[m] > x[m + 1]; diff = bit xor the bit before it (the first gives none).
 * sdr_rds_clock_set_params: window 1 .. SDR_RDS_CLOCK_MAX_WINDOW (default 4), hysteresis
 *   0 .. SDR_RDS_CLOCK_MAX_HYSTERESIS (default 8); they hold for the calls that follow.
 * sdr_rds_clock_process_dev: async on the context stream, nothing is read back.  Row s is the n
 *   floats at rrc_i + s * stride, at any 4-byte alignment; 0 <= n <= max_n, stride >= n; nothing
 *   beyond n is read.
 * sdr_rds_clock_bits: the rows the next stage reads: row s is the bytes at *dev + s * *stride,
 *   (*counts_dev)[s] of them valid after a call, at most *max_bits = 17 ceil(max_n / 768) + 1:
 *   sdr_rds_sync_process_dev(sync, *dev, *max_bits, *stride, *counts_dev).  Any pointer may be NULL.
 * sdr_rds_clock_fetch (synchronises): the last call's bits[nstreams][max_bits] and counts[nstreams]
 *   to the host; either may be NULL.
 * sdr_rds_clock_state (synchronises): state[nstreams][SDR_RDS_CLOCK_NSTATE] = consumed samples,
 *   segments, phi, pi, symbols, Manchester bits (one more than the differential bits), steps
 *   forward, steps back, wraps, pairing changes since reset. */
#define SDR_RDS_CLOCK_MAX_STREAMS 65535
#define SDR_RDS_CLOCK_MAX_N (1 << 24)
#define SDR_RDS_CLOCK_MAX_WINDOW 16
#define SDR_RDS_CLOCK_MAX_HYSTERESIS (1 << 20)
#define SDR_RDS_CLOCK_NSTATE 10
typedef struct sdr_rds_clock sdr_rds_clock;
int sdr_rds_clock_create(sdr_ctx* ctx, int nstreams, int64_t max_n, sdr_rds_clock** out);
void sdr_rds_clock_destroy(sdr_rds_clock* clk);
int sdr_rds_clock_reset(sdr_rds_clock* clk);
int sdr_rds_clock_set_params(sdr_rds_clock* clk, int window, int hysteresis);
int sdr_rds_clock_process_dev(sdr_rds_clock* clk, const float* rrc_i, int64_t n, int64_t stride);
int sdr_rds_clock_bits(sdr_rds_clock* clk, uint8_t** dev, int64_t* stride, int32_t** counts_dev, int64_t* max_bits);
int sdr_rds_clock_fetch(sdr_rds_clock* clk, uint8_t* bits, int32_t* counts);
int sdr_rds_clock_state(sdr_rds_clock* clk, int64_t* state);

/* ---- RDS carrier phase recovery on the device, in front of the symbol clock ---------------
 * Every stream's rrc_i and rrc_q rows (24 samples a symbol) -> one row per stream, the samples
 * projected onto the axis the data lie on, left in device memory for sdr_rds_clock_process_dev or
 * sdr_rds_links_process_dev; n samples in give n samples out.  The clock, the link layer and the
 * block synchroniser read the in-phase row only: with the 57 kHz carrier's phase off, the symbol
 * energy is in rrc_q.  The host model rdscarrier.py RdsCarrierPhase is the specification; rows,
 * state and moments equal it after every call, whatever the split of a stream into calls
 * (csrc/rds_carrier.hip, four launches per call).  A stream is cut into the clock's segments of
 * 768 samples on its absolute sample grid; the axis of a segment comes from the complete segments
 * before it.
 *   Moments of a complete segment g, the samples widened to f64, a pair with a non-finite value
 *     counting as (0, 0): Sii, Sqq, Siq from i i, q q, i q -- for each p = 0 .. 23 the sum over
 *     j = 0 .. 31 ascending of the product at sample 768 g + 24 j + p, then the 24 sums, p ascending.
 *   Window: for g >= 1, A, B, C = the sums of Sii, Sqq, Siq over the min(window, g) segments before
 *     g, oldest first; P = A - B, Q = 2 C.
 *   Direction: khat in 0 .. 31, the sector (11.25 degrees wide, centred on the multiples of 11.25
 *     degrees) of the doubled angle atan2(Q, P): a = |P|, b = |Q|, swapped if b > a; if not a > 0
 *     the segment holds kappa and `holds` counts it; m = how many t of tan(pi/32), tan(3 pi/32),
 *     tan(5 pi/32), tan(7 pi/32) (decimal literals) give b > a t; m = 8 - m if swapped, 16 - m if
 *     P < 0, (32 - m) mod 32 if Q < 0.
 *   Tracking: the axis index kappa in 0 .. 63, angle pi kappa / 32.  Segment 0 uses 0, segment 1
 *     sets kappa = khat, later kappa moves one step (mod 64) towards khat (known mod 32) the
 *     shorter way when they are 2 or more apart: at most 5.625 degrees per 13.5 ms, 417 degrees/s.
 *   Output: y[v] = float32(f64(c) f64(i[v]) + f64(s) f64(q[v])) for every sample v of segment g,
 *     complete or not, (c, s) = entry kappa_g of the axis table, the samples as they are.
 *   Axis table: 64 float32 pairs (c, s); entries 0 .. 8 are cos and sin of pi kappa / 32 in f64
 *     rounded to float32, entry 0 (1, 0), entry 8 float32(sqrt(1/2)) twice, the others by symmetry,
 *     so entry 16 is exactly (0, 1).
 * sdr_rds_carrier_create: nstreams 1 .. SDR_RDS_CLOCK_MAX_STREAMS, max_n 1 .. SDR_RDS_CLOCK_MAX_N.
 * sdr_rds_carrier_set_params: window 1 .. SDR_RDS_CARRIER_MAX_WINDOW (default 8), for the calls
 *   that follow.
 * sdr_rds_carrier_process_dev: async on the context stream, nothing is read back.  Row s of i and
 *   of q is the n floats at rrc_i + s * stride and rrc_q + s * stride, each at any 4-byte
 *   alignment; 0 <= n <= max_n, stride >= n; nothing beyond n is read.
 * sdr_rds_carrier_rows: the rows the next stage reads: row s is the last call's n floats at
 *   *dev + s * *stride (16-byte aligned).  Either pointer may be NULL.
 * sdr_rds_carrier_fetch (synchronises): rows[nstreams][n], the first n <= max_n floats of every row.
 * sdr_rds_carrier_state (synchronises): state[nstreams][SDR_RDS_CARRIER_NSTATE] = samples taken,
 *   complete segments, kappa of the last complete segment, steps forward, steps back, holds,
 *   wraps (steps 63 <-> 0) since reset.
 * sdr_rds_carrier_moments (synchronises): abc[nstreams][3] = (A, B, C) of the window behind the
 *   last complete segment's direction (zeros before segment 1);
 *   sqrt((A - B)^2 + (2 C)^2) / (A + B) is a lock measure.
 * sdr_rds_carrier_axes: the axis table, out[2 kappa] = c, out[2 kappa + 1] = s. */
#define SDR_RDS_CARRIER_MAX_WINDOW 16
#define SDR_RDS_CARRIER_NSTATE 7
typedef struct sdr_rds_carrier sdr_rds_carrier;
int sdr_rds_carrier_create(sdr_ctx* ctx, int nstreams, int64_t max_n, sdr_rds_carrier** out);
void sdr_rds_carrier_destroy(sdr_rds_carrier* car);
int sdr_rds_carrier_reset(sdr_rds_carrier* car);
int sdr_rds_carrier_set_params(sdr_rds_carrier* car, int window);
int sdr_rds_carrier_process_dev(sdr_rds_carrier* car, const float* rrc_i, const float* rrc_q, int64_t n, int64_t stride);
int sdr_rds_carrier_rows(sdr_rds_carrier* car, float** dev, int64_t* stride);
int sdr_rds_carrier_fetch(sdr_rds_carrier* car, float* rows, int64_t n);
int sdr_rds_carrier_state(sdr_rds_carrier* car, int64_t* state);
int sdr_rds_carrier_moments(sdr_rds_carrier* car, double* abc);
int sdr_rds_carrier_axes(float* out);

#ifdef __cplusplus
}
#endif
#endif /* SDR_H_ */
