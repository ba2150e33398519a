// Internal launcher interface between the block receiver (rx.hip: the sdr_rx object, host code)
// and its stage kernels (rx_stage.hip: the VALU tiles, the matrix-core kernels, the composite
// RDS filter and their launch planning).  One definition of every struct that crosses that
// boundary: both files include this header, so a field change is a compile error in both
// instead of a silent ODR mismatch.  The job structs are kernel arguments, passed by value.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdr_nco.h"
#include "../../include/sdr.h"

enum { JK_FIR = 0, JK_RESAMPLE = 1 };
// PRE_NCO: the mixer of PRE_MIX whose second operand, the PLL's NCO, is formed from the PLL's
// phase rows where the input is staged (sdr_nco.h) instead of read from an NCO row
enum { PRE_NONE = SDR_PRE_NONE, PRE_SQUARE = SDR_PRE_SQUARE, PRE_MIX = SDR_PRE_MIX, PRE_NCO = 3 };

// One filter of a stage, applied to `nstreams` streams.
struct StageJob {
  const float* x;        // input rows, x_stride apart
  const float* c;        // PRE_MIX second operand (same indexing as x)
  const float* taps;     // f32 taps (device)
  const float* rtaps;    // the same reversed, zero at [-1] and [T] (TapSet::dev_rev: fir_tile's pairs)
  const double* taps64;  // f64 taps (device, for zf)
  const double* zi;      // lfilter state in (T-1 per stream, zi_stride apart), nullable
  double* zf;            // lfilter state out (same layout), nullable
  float* y;              // outputs, y_stride apart
  const float* mono;     // combiner: mono audio rows (y_stride apart), or null
  float* left;
  float* right;
  float* yh;             // host mirrors (pinned, rows yh_stride apart) of y / left / right, nullable:
  float* lh;             //   sdr_rx_run's outputs are stored straight into pinned host memory
  float* rh;             //   by the producing tile instead of coming back by a copy
  int64_t n, x_stride, zi_stride, y_stride, yh_stride;
  int64_t b0;            // first workgroup of this job's tiles
  float gain;
  int pre, D, U, kind, T, tiles;
  int small;             // D = 1 FIR: 4 outputs per lane (a launch with few tiles: more workgroups)
  int sym;               // the f32 taps are symmetric (linear phase: every firwin design)
  int fold;              // > 1: the leader of `fold` consecutive symmetric jobs on the same input,
                         //   computed together by fold_tile (the others get no tile workgroups)
  int nco_sin;           // PRE_NCO: the quadrature NCO (sin) instead of cos
  int mma;               // the tiles run on the matrix cores (rx_mma_kernel); this launch keeps its zf
  int wgs;               // rx_mma_kernel: the job's workgroups (each runs every wgs-th tile)
  NcoSrc nco;            // PRE_NCO: where the NCO comes from
  int8_t* y8;            // nullable: the outputs' sign codes too (sdr_nco.h pll_code: a PLL's input),
  int64_t y8_stride;     //   y8_stride bytes apart; y may then be null (matrix-core jobs only)
};

// The front end's carried state, finished by the first stage launch after the FE kernel:
// the I/Q lfilter final states (f64, from the block's last T-1 IQ samples) and the demod
// phase prev = phi_last + 2 pi W (W = the block's wrap count, which is reset for the next
// block).  One workgroup per stream.
struct FeState {
  const void* iq;
  int64_t n, stride;          // complex samples per block / between streams
  const double* b;            // f64 taps
  const double* zi_i;
  const double* zi_q;
  double* zf_i;
  double* zf_q;
  int64_t zs;                 // state stride
  const float* last_phi;
  int* wraps;
  double* phase;
  int T, u8, on;
};

// The composite RDS filter's job (rx_cres_kernel / rx_cresmm_kernel): mixers + LPF + x19 / 80
// resampler of every stream, and both filters' final states
struct CresJob {
  const float* x;            // RDS extract rows (x_stride apart), M samples
  int64_t n, x_stride;
  NcoSrc nco;                // the RDS PLL's NCO: from its phases (theta != null) or rows
  const float* ctaps;        // composite taps (device: what cres_taps gives)
  const double* h64;         // LPF taps (f64, 151)
  const double* g64;         // anti-image taps (f64, 151)
  const double* zi_l[2];     // LPF I / Q lfilter state in (150 per stream, zs apart)
  const double* zi_a[2];     // anti-image I / Q state in
  double* zf_l[2];           // ... out
  double* zf_a[2];
  int64_t zs;
  float* y[2];               // resample I / Q rows (y_stride apart), R = ceil(19 M / 80) outputs
  float* yh[2];              // pinned host mirrors (yh_stride apart), nullable
  int64_t y_stride, yh_stride, R;
  int tiles, nstreams;       // tiles: set by launch_cres
};

// Launch the jobs of one stage (at most 6): the matrix cores' first, their jobs' final states with
// them; fe: the front end's carried state rides on the first launch
hipError_t launch_stage(std::vector<StageJob> jobs, int S, hipStream_t st, const FeState* fe = nullptr);
// rows of n samples are long enough for the matrix-core kernels (spans)
bool mm_span_ok(int64_t n);
// launch_stage would run the job on the matrix cores (only such a job may store sign codes)
bool mmable(const StageJob& j);

// the composite filter covers this resampling ratio (19 / 80)
bool cres_covers(int rds_up, int rds_down);
// the composite taps (host, f64 then f32) of LPF h and anti-image filter g in the kernels' order;
// empty unless both filters have 151 taps
void cres_taps(const std::vector<double>& h, const std::vector<double>& g, std::vector<float>* out);
// the job's grid fits a launch (J.R, J.nstreams): the caller's check before launch_cres
bool cres_fits(const CresJob& J);
// span: the matrix-core form (when the NCO comes from phase rows)
hipError_t launch_cres(const CresJob& job, bool span, hipStream_t st);
