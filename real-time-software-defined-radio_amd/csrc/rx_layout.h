// What the block receiver (rx.hip) knows about its outputs, filters and filter states, one table
// each, and the layout of its device allocations as one pure function.  No HIP here: a host
// compiler alone checks it (tests/test_rx_layout.py).
#pragma once
#include <cstdint>

#include "../../include/sdr.h"

namespace rxlayout {

enum Group { G_ALWAYS, G_AUDIO, G_STEREO, G_RDS };      // the flags an output or a filter needs
// the one decode of the receiver's flags (SDR_RX_STEREO implies audio)
constexpr bool group_on(int flags, Group g) {
  return g == G_ALWAYS || (g == G_AUDIO && (flags & (SDR_RX_AUDIO | SDR_RX_STEREO))) ||
         (g == G_STEREO && (flags & SDR_RX_STEREO)) || (g == G_RDS && (flags & SDR_RX_RDS));
}
enum Len { L_M, L_M1, L_A, L_R };                       // samples per row: M, M + 1, A, R
enum Producer { BY_FE, BY_PLL, BY_STAGE, BY_AUDIO };    // FE, PLL, a stage kernel (can store a host copy too), audio output stage
enum Role { ROLE_NONE, ROLE_NCO, ROLE_LPF, ROLE_PLL_IN };   // intermediates a block may skip (rx_made)
struct OutputInfo { Group group; bool deemph; Len len; Producer by; Role role; };   // deemph: with sdr_rx_set_deemph only
constexpr OutputInfo kOutput[] = {
    {G_ALWAYS, false, L_M, BY_FE, ROLE_NONE},           // SDR_RX_O_DEMOD
    {G_AUDIO, false, L_A, BY_STAGE, ROLE_NONE},         // _AUDIO
    {G_STEREO, false, L_M, BY_STAGE, ROLE_PLL_IN},      // _BPF_RECOVERY
    {G_STEREO, false, L_M1, BY_PLL, ROLE_NCO},          // _STEREO_NCO
    {G_STEREO, false, L_M, BY_STAGE, ROLE_NONE},        // _BPF_EXTRACTION
    {G_STEREO, false, L_A, BY_STAGE, ROLE_NONE},        // _STEREO
    {G_STEREO, false, L_A, BY_STAGE, ROLE_NONE}, {G_STEREO, false, L_A, BY_STAGE, ROLE_NONE},   // _LEFT, _RIGHT
    {G_RDS, false, L_M, BY_STAGE, ROLE_NONE},           // _RDS_EXTRACT
    {G_RDS, false, L_M, BY_STAGE, ROLE_PLL_IN},         // _RDS_PRE_PLL
    {G_RDS, false, L_M1, BY_PLL, ROLE_NCO}, {G_RDS, false, L_M1, BY_PLL, ROLE_NCO},             // _RDS_NCO_I, _Q
    {G_RDS, false, L_M, BY_STAGE, ROLE_LPF}, {G_RDS, false, L_M, BY_STAGE, ROLE_LPF},           // _RDS_LPF_I, _Q
    {G_RDS, false, L_R, BY_STAGE, ROLE_NONE}, {G_RDS, false, L_R, BY_STAGE, ROLE_NONE},         // _RDS_RES_I, _Q
    {G_RDS, false, L_R, BY_STAGE, ROLE_NONE}, {G_RDS, false, L_R, BY_STAGE, ROLE_NONE},         // _RDS_RRC_I, _Q
    {G_AUDIO, true, L_A, BY_AUDIO, ROLE_NONE},          // _AUDIO_DE
    {G_STEREO, true, L_A, BY_AUDIO, ROLE_NONE}, {G_STEREO, true, L_A, BY_AUDIO, ROLE_NONE},     // _LEFT_DE, _RIGHT_DE
};
static_assert(sizeof kOutput / sizeof kOutput[0] == SDR_RX_NOUTPUTS, "one entry per SDR_RX_O_*, in the enum's order");
constexpr bool produced(int flags, bool de_on, int o) { return group_on(flags, kOutput[o].group) && (!kOutput[o].deemph || de_on); }

struct FilterInfo { const char* name; Group group; };
constexpr FilterInfo kFilter[] = {
    {"rf", G_ALWAYS},       {"audio", G_AUDIO},    {"pilot", G_STEREO}, {"stereo_bpf", G_STEREO}, {"stereo_lpf", G_STEREO},
    {"rds_extract", G_RDS}, {"rds_square", G_RDS}, {"rds_lpf", G_RDS},  {"rds_anti", G_RDS},      {"rds_rrc", G_RDS},
};
static_assert(sizeof kFilter / sizeof kFilter[0] == SDR_RX_NFILTERS, "one entry per SDR_RX_F_*");

// state-bank slots (f64 lfilter states, T-1 per stream each) and the filter each belongs to
enum Zs {
  Z_FE_I, Z_FE_Q, Z_AUDIO, Z_PILOT, Z_BAND, Z_EXTRACT, Z_SQUARE, Z_SLPF, Z_RLPF_I, Z_RLPF_Q,
  Z_ANTI_I, Z_ANTI_Q, Z_RRC_I, Z_RRC_Q, Z_N
};
constexpr int kStateFilter[] = {
    SDR_RX_F_RF,       SDR_RX_F_RF,       SDR_RX_F_AUDIO,    SDR_RX_F_PILOT,    SDR_RX_F_STEREO_BPF, SDR_RX_F_RDS_EXTRACT, SDR_RX_F_RDS_SQUARE,
    SDR_RX_F_STEREO_LPF, SDR_RX_F_RDS_LPF, SDR_RX_F_RDS_LPF, SDR_RX_F_RDS_ANTI, SDR_RX_F_RDS_ANTI,  SDR_RX_F_RDS_RRC,     SDR_RX_F_RDS_RRC,
};
static_assert(sizeof kStateFilter / sizeof kStateFilter[0] == Z_N, "one entry per Z_*");

struct RxGeom {
  int64_t S, B;                          // streams, complex samples per block
  int rf_decim, audio_decim, rds_up, rds_down, flags;
  bool de_on; int nsets;                 // row sets: 1, or nq when pipelined
  int64_t taps[SDR_RX_NFILTERS];         // tap counts
  int64_t pllw_bytes;                    // sdr_pll_work_bytes(2, S, M()): the PLLs' scratch per row set
  int64_t M() const { return (B + rf_decim - 1) / rf_decim; }
};
// Regions are bytes from the base of their allocation.  The main one's base is 256-B aligned
// (hipMalloc; rx_finalize checks it: pllw's alignment was once applied to the address itself).
constexpr int kMaxSets = 3;
enum Reg { BANK0, BANK1, PHASE, WRAPS, LAST_PHI, PLL_STATE0, PLL_STATE1, THETA, PLLC, PLLW, PCODE, DE_STATE, DE_MONO, NREG };
struct Region { int64_t off = -1, bytes = 0; };          // off -1: not in this configuration
struct RxLayout {                        // (sdr_rx carries its receiver's)
  int64_t M = 0, A = 0, R = 0;           // samples per block at the demod, audio and RDS symbol-filter rates
  int64_t out_n[SDR_RX_NOUTPUTS] = {}, out_stride[SDR_RX_NOUTPUTS] = {};   // floats; 0 when not produced
  int64_t zoff[Z_N] = {}, zlen[Z_N] = {}, bank_len = 0;                     // doubles: within a bank; per stream; per bank
  int64_t ths = 0, cst = 0, pcs = 0;     // row strides: theta and pllc (doubles), pcode (bytes)
  int64_t pllw_bytes = 0, pcm_stride = 0;   // per row set, rounded to 256; int16 per PCM row
  Region out_rg[kMaxSets][SDR_RX_NOUTPUTS], reg[NREG], pcm_rg[kMaxSets];
  Region reset, de_reset;                // what sdr_rx_reset zeroes: both banks, phase and wraps; the audio stage's states
  int64_t total = 0, de_total = 0;       // the main allocation; the audio output stage's (DE_*, pcm: with de_on)
};

inline RxLayout rx_layout(const RxGeom& g) {
  auto up = [](int64_t v, int64_t m) { return (v + m - 1) / m * m; };
  RxLayout L;
  // One ordered list of regions.  An aligned region budgets its whole alignment, whatever padding
  // it then uses, so the total is the sum of what was asked for and no offset can pass it.
  int64_t cur = 0, slack = 0;
  auto take = [&](int64_t bytes, int64_t align = 1) {
    const int64_t pad = up(cur, align) - cur;
    if (align > 1) slack += align - pad;
    cur += pad + bytes;
    return Region{cur - bytes, bytes};
  };
  const int64_t S = g.S, M = L.M = g.M(), S2 = up(S, 2);
  L.A = (M + g.audio_decim - 1) / g.audio_decim;
  L.R = (M * g.rds_up + g.rds_down - 1) / g.rds_down;
  // f32 output rows: per row set, the produced outputs in enum order, S rows `stride` apart (the M
  // and M + 1 long rows share one stride) and a 64-float gap after each
  for (int q = 0; q < g.nsets; ++q)
    for (int o = 0; o < SDR_RX_NOUTPUTS; ++o) {
      if (!produced(g.flags, g.de_on, o)) continue;
      const Len len = kOutput[o].len;
      L.out_n[o] = len == L_A ? L.A : len == L_R ? L.R : len == L_M1 ? M + 1 : M;
      L.out_stride[o] = up(len == L_A ? L.A : len == L_R ? L.R : M + 1, 64);
      L.out_rg[q][o] = take(4 * (L.out_stride[o] * S + 64));
    }
  // f64: two state banks (they swap every block), then per-stream values in rows of S2 doubles
  // (S2 even keeps what follows 16-B aligned)
  for (int z = 0; z < Z_N; ++z) {
    const int f = kStateFilter[z];
    if (!group_on(g.flags, kFilter[f].group)) continue;
    L.zoff[z] = L.bank_len;
    L.zlen[z] = g.taps[f] - 1 > 1 ? g.taps[f] - 1 : 1;
    L.bank_len += up(L.zlen[z] * S, 2);
  }
  L.ths = up(M, 2) + 2; L.cst = up(M + M / 32, 2) + 2;
  L.pcs = up(M + 16, 256); L.pllw_bytes = up(g.pllw_bytes, 256);
  const int64_t bytes[PCODE + 1] = {8 * L.bank_len, 8 * L.bank_len, 8 * S2 /* S doubles */, 8 * S2 /* S ints */, 8 * S2 /* S floats */,
                                    8 * 6 * S2, 8 * 6 * S2, 8 * g.nsets * 2 * S * L.ths, 8 * g.nsets * 2 * S * L.cst,
                                    g.nsets * L.pllw_bytes, g.nsets * 2 * S * L.pcs};
  for (int k = BANK0; k <= PCODE; ++k)
    if (k != PCODE || (g.flags & (SDR_RX_STEREO | SDR_RX_RDS))) L.reg[k] = take(bytes[k], k == BANK0 ? 64 : k == PLLW ? 256 : 1);
  L.total = cur + slack;
  L.reset = Region{L.reg[BANK0].off, L.reg[LAST_PHI].off - L.reg[BANK0].off};
  if (g.de_on) {
    cur = slack = 0;
    L.pcm_stride = up(2 * L.A, 64);
    L.reg[DE_STATE] = take(8 * 2 * S2);              // [S][2]
    L.reg[DE_MONO] = take(8 * (S2 + 2));             // [S]
    L.de_reset = Region{0, 8 * 3 * S2};
    for (int q = 0; q < g.nsets; ++q) L.pcm_rg[q] = take(2 * S * L.pcm_stride);
    L.de_total = cur;
  }
  return L;
}

}  // namespace rxlayout
