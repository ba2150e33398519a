// RDS link layer on the device (include/sdr.h sdr_rds_links_*): the in-phase RRC rows of
// `nstreams` streams -> symbols, Manchester bits, differential bits, the syndrome of every 26-bit
// window and the frame rule's events, with every stream's carried state in device memory.  The
// host layer (capi.hip sdr_rds_link_block, model/fmRDSblock.py:207-346) is the specification,
// quirks included; this file restates it so that bits, scanned bits, events and state are the
// same, call by call.
//
// Three launches per call, whatever nstreams and n are; no workgroup waits for another:
//   gather  a thread per symbol pair: s[k] = x[io + 24 k] into a compact row, and in block 0 the
//           c0 / c1 pair counts of the start-position screening (one integer atomic per wave).
//   scan    a workgroup per tile of RDS_TILE positions of the scanned row d: each thread forms
//           its bit of d from the symbols (carried bits, front bit and previous bit from the
//           state), the waves pack the tile plus a 26-bit halo into LDS words, and each thread
//           takes its window by a funnel shift: ten masked parities against the four syndromes.
//           The tile's matches are compacted in window order (ballot ranks, no cursor) into the
//           tile's own slots, with their 16 information bits.
//   frame   a workgroup per stream: the NaN rule, the tiles' counts -> a prefix -> one list of
//           the stream's matches in window order; then one wave: the value search for the next
//           symbol offset, the frame rule over the matches only (64 at a time in the lanes, the
//           rule itself a few scalar instructions per match), the events and the next state.
// Everything a launch derives from the state (block 0 or not, offset, start position, counts)
// is derived the same way by all three from `plan_of`, so they agree without a hand-off; the
// frame launch is the only one that writes the state, and it runs last.  The code -- H, the offset
// syndromes, a window out of the LDS words, its information word -- is rds_code.h's.
#include <hip/hip_runtime.h>

#include <new>

#include "rds_code.h"
#include "rds_links.h"
#include "sdr_ctx.h"

using namespace sdrint;

namespace {

constexpr int RDS_T = 256, RDS_TILE = 256, RDS_NW = RDS_T / 64, RDS_SPS = 24;
static_assert(RDS_TILE == RDS_T, "one position of the scanned row per thread");

// the window's syndrome type 0..3 (A..D), or -1: this layer does not know C'
__device__ __forceinline__ int syndrome_type(uint32_t v) {
  const uint32_t s = syndrome_of(v);
  return s == SYN_A ? 0 : s == SYN_B ? 1 : s == SYN_C ? 2 : s == SYN_D ? 3 : -1;
}

// a stream's carried state; all zero = "block 0 has not run" (load_state gives the start values)
struct RdsState {
  int64_t printposition, last_position;
  int started, int_offset, start_pos, front_bit, prebit, bad_sync, ncarried;
  uint32_t carried;             // bit i = carried bit i (the scanned row's first ncarried bits)
  float lonely_bit;
  int pad_;
};

struct RdsArgs {
  const float* x; int64_t n, stride;
  RdsState* state;
  float* sym; int64_t sym_stride;           // the sampled symbols
  uint8_t* bits; int64_t bits_stride;       // the Manchester bits
  uint8_t* diff; int64_t diff_stride;       // the scanned row
  unsigned* cnt;                            // [stream][2]: block 0's c0 / c1; zero between calls
  int* tcount; uint32_t* rec; int64_t tiles_stride;   // per tile: matches, and their records in the tile's slots
  uint2* cm;                                // the stream's matches in window order: {window, type << 16 | word}
  int* nbd;                                 // [stream][2]: the last call's bit and scanned-bit counts
  int* added;                               // [stream][2]: {C, L - C}, the scanned bits the last call added
  int64_t* ev; int64_t* nev; int* status; int64_t max_events;
  int resync;
};

__device__ __forceinline__ RdsState load_state(const RdsState* p) {
  RdsState st = *p;
  if (st.started == 0) {
    st = RdsState{};
    st.last_position = -1;
  }
  return st;
}

// What a call does with one row, from the state and the row's first samples: the symbol offset
// and count, the bit count, and the scanned row's geometry.
struct RdsPlan {
  bool block0;
  int io, ns, nb, off, C, L, W;
};
__device__ __forceinline__ RdsPlan plan_of(const RdsState& st, const float* __restrict__ row, int64_t n) {
  RdsPlan p;
  p.block0 = st.started == 0;
  p.io = st.int_offset;
  if (p.block0) {               // first index of the maximum of the first symbol period
    int best = 0;
    float vb = row[0];
    for (int k = 1; k < RDS_SPS; ++k) {
      const float v = row[k];
      if (v > vb) {
        vb = v;
        best = k;
      }
    }
    p.io = best;
  }
  p.ns = (int)((n - p.io + RDS_SPS - 1) / RDS_SPS);
  p.nb = p.ns / 2;              // with start position 1 the front bit takes the place of the dropped pair
  p.off = p.block0 ? 1 : 0;     // block 0 consumes its first bit as the previous bit
  p.C = p.block0 ? 0 : st.ncarried;
  p.L = p.C + p.nb - p.off;
  p.W = p.L - 26;               // windows 0 .. L - 27
  return p;
}
// the start position: block 0 screens it (a tie gives 0), later calls carry it
__device__ __forceinline__ int start_pos_of(const RdsState& st, const RdsPlan& p, const unsigned* cnt) {
  return p.block0 ? (cnt[0] > cnt[1] ? 1 : 0) : st.start_pos;
}
// the bit in front of the pairs when the start position is 1: the carried lone symbol against
// this call's first symbol, the old front bit on a tie (block 0: the state's, 0)
__device__ __forceinline__ int front_bit_of(const RdsState& st, const RdsPlan& p, int sp, const float* __restrict__ sym) {
  if (sp != 1 || p.block0) return st.front_bit;
  const float s0 = sym[0];
  return st.lonely_bit > s0 ? 1 : st.lonely_bit < s0 ? 0 : st.front_bit;
}

// Manchester bit k of the call (k < nb): a tie or a NaN gives 0
__device__ __forceinline__ int mbit(const float* __restrict__ sym, int k, int sp, int front) {
  if (k < sp) return front;
  const int a = 2 * k - sp;
  return sym[a] > sym[a + 1] ? 1 : 0;
}

__global__ __launch_bounds__(RDS_T) void rds_gather_kernel(const RdsArgs a) {
  const int s = blockIdx.y, lane = threadIdx.x & 63;
  const float* __restrict__ row = a.x + (int64_t)s * a.stride;
  const RdsState st = load_state(a.state + s);
  const RdsPlan p = plan_of(st, row, a.n);
  float* __restrict__ sym = a.sym + (int64_t)s * a.sym_stride;
  const int m = blockIdx.x * RDS_T + threadIdx.x;       // symbols 2 m, 2 m + 1
  const int k0 = 2 * m;
  float s0 = 0.f, s1 = 0.f;
  if (k0 < p.ns) {
    s0 = row[p.io + (int64_t)RDS_SPS * k0];
    sym[k0] = s0;
  }
  if (k0 + 1 < p.ns) {
    s1 = row[p.io + (int64_t)RDS_SPS * (k0 + 1)];
    sym[k0 + 1] = s1;
  }
  if (p.block0) {               // model/fmRDSblock.py:233-249, the `if / elif` per step
    bool v0 = false, v1 = false;
    if (m < p.ns / 4) {         // 2 m + 2 <= 2 (ns / 4) < ns
      const float s2 = row[p.io + (int64_t)RDS_SPS * (k0 + 2)];
      v0 = (s0 > 0.f && s1 > 0.f) || (s0 < 0.f && s1 < 0.f);
      v1 = !v0 && ((s1 > 0.f && s2 > 0.f) || (s1 < 0.f && s2 < 0.f));
    }
    const int n0 = __popcll(__ballot(v0)), n1 = __popcll(__ballot(v1));
    if (lane == 0) {
      if (n0) atomicAdd(a.cnt + 2 * s, (unsigned)n0);
      if (n1) atomicAdd(a.cnt + 2 * s + 1, (unsigned)n1);
    }
  }
}

__global__ __launch_bounds__(RDS_T) void rds_scan_kernel(const RdsArgs a) {
  __shared__ uint32_t dw[2 * RDS_NW + 2];
  __shared__ int wcount[RDS_NW];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* __restrict__ row = a.x + (int64_t)s * a.stride;
  const RdsState st = load_state(a.state + s);
  const RdsPlan p = plan_of(st, row, a.n);
  const float* __restrict__ sym = a.sym + (int64_t)s * a.sym_stride;
  const int sp = start_pos_of(st, p, a.cnt + 2 * s);
  const int front = front_bit_of(st, p, sp, sym);
  const int w0 = blockIdx.x * RDS_TILE;

  // bit i of the scanned row: the carried bits, then b[kb - 1] ^ b[kb] from kb = off on, with
  // the carried previous bit in front of b[0]
  auto dbit = [&](int i, int* kb_out, int* b_out) -> int {
    if (i < p.C) {
      *kb_out = -1;
      return (int)((st.carried >> i) & 1u);
    }
    const int kb = i - p.C + p.off;
    const int cur = mbit(sym, kb, sp, front);
    const int prev = kb == 0 ? st.prebit : mbit(sym, kb - 1, sp, front);
    *kb_out = kb;
    *b_out = cur;
    return prev ^ cur;
  };

  const int i = w0 + tid;
  int d = 0;
  if (i < p.L) {
    int kb = -1, b = 0;
    d = dbit(i, &kb, &b);
    a.diff[(int64_t)s * a.diff_stride + i] = (uint8_t)d;
    if (kb >= 0) {
      uint8_t* __restrict__ bo = a.bits + (int64_t)s * a.bits_stride;
      bo[kb] = (uint8_t)b;
      if (kb == 1 && p.off == 1) bo[0] = (uint8_t)mbit(sym, 0, sp, front);   // block 0's first bit
    }
  }
  const unsigned long long mk = __ballot(d != 0);
  if (lane == 0) {
    dw[2 * wv] = (uint32_t)mk;
    dw[2 * wv + 1] = (uint32_t)(mk >> 32);
  }
  if (wv == 0) {                // the 26 bits after the tile (the next tile's; 0 beyond the row)
    const int i2 = w0 + RDS_TILE + lane;
    int d2 = 0;
    if (lane < 26 && i2 < p.L) {
      int kb, b;
      d2 = dbit(i2, &kb, &b);
    }
    const unsigned long long mh = __ballot(d2 != 0);
    if (lane == 0) {
      dw[2 * RDS_NW] = (uint32_t)mh;
      dw[2 * RDS_NW + 1] = 0u;
    }
  }
  __syncthreads();

  int typ = -1;
  uint32_t v = 0;
  if (i < p.W) {
    v = window_at(dw, tid);
    typ = syndrome_type(v);
  }
  const unsigned long long mm = __ballot(typ >= 0);
  if (lane == 0) wcount[wv] = __popcll(mm);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < RDS_NW; ++w) {
    const int c = wcount[w];
    base += w < wv ? c : 0;
    total += c;
  }
  if (typ >= 0) {
    const int rank = base + __popcll(mm & ((1ull << lane) - 1ull));
    a.rec[(int64_t)s * a.tiles_stride * RDS_TILE + (int64_t)blockIdx.x * RDS_TILE + rank] =
        ((uint32_t)tid << 18) | ((uint32_t)typ << 16) | info_word(v);
  }
  if (tid == 0) a.tcount[(int64_t)s * a.tiles_stride + blockIdx.x] = total;
}

// One workgroup per stream.  All waves: the tiles' counts -> a prefix -> the matches compacted
// into one list in window order (global window index, type and word).  Wave 0 then takes the
// list 64 matches at a time: the lanes load them, the frame rule -- the only sequential part, a
// few scalar instructions per match -- runs over the lanes' values with readlane and leaves two
// bit masks (accepted, re-sync after), and the lanes store their events side by side.
__global__ __launch_bounds__(RDS_T) void rds_frame_kernel(const RdsArgs a) {
  __shared__ int wsum[RDS_NW];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* __restrict__ row = a.x + (int64_t)s * a.stride;
  RdsState st = load_state(a.state + s);
  const RdsPlan p = plan_of(st, row, a.n);
  const float* __restrict__ sym = a.sym + (int64_t)s * a.sym_stride;
  unsigned* cnt = a.cnt + 2 * s;
  const int sp = start_pos_of(st, p, cnt);
  const int front = front_bit_of(st, p, sp, sym);
  // the host layer's two NaN errors, both before it has touched its state: a NaN among block 0's
  // first 24 samples, or a last symbol that is NaN (it is then not found among the last 24).
  // Every wave decides this for itself, the same way.
  const float head = lane < RDS_SPS ? row[lane] : 0.f;
  const float tail = lane < RDS_SPS ? row[a.n - RDS_SPS + lane] : 0.f;
  const float slast = sym[p.ns - 1];
  const bool nan_head = p.block0 && __any(head != head) != 0;
  const unsigned long long eq = __ballot(lane < RDS_SPS && tail == slast);
  const bool fault = nan_head || eq == 0ull;
  __syncthreads();              // every wave has read the screening counts
  if (tid == 0) {               // the next block 0 starts from zero
    cnt[0] = 0u;
    cnt[1] = 0u;
    if (fault) {
      a.status[s] = SDR_RDS_LINKS_FAULT;
      a.nev[s] = 0;
      a.nbd[2 * s] = 0;
      a.nbd[2 * s + 1] = 0;
      a.added[2 * s] = 0;
      a.added[2 * s + 1] = 0;
    }
  }
  if (fault) return;

  // the matches of all tiles as one list, in window order
  const int ntiles = (p.W + RDS_TILE - 1) / RDS_TILE;
  const int* __restrict__ tcount = a.tcount + (int64_t)s * a.tiles_stride;
  const uint32_t* __restrict__ rec = a.rec + (int64_t)s * a.tiles_stride * RDS_TILE;
  uint2* __restrict__ cm = a.cm + (int64_t)s * a.tiles_stride * RDS_TILE;
  int total = 0;
  for (int t0 = 0; t0 < ntiles; t0 += RDS_T) {
    const int tile = t0 + tid;
    const int c = tile < ntiles ? tcount[tile] : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = total;
#pragma unroll
    for (int w = 0; w < RDS_NW; ++w) {
      const int v = wsum[w];
      base += w < wv ? v : 0;
      total += v;
    }
    const int dst = base + incl - c;
    for (int k = 0; k < c; ++k) {
      const uint32_t r = rec[(int64_t)tile * RDS_TILE + k];
      cm[dst + k] = uint2{(uint32_t)(tile * RDS_TILE) + (r >> 18), r & 0x3ffffu};
    }
    __syncthreads();            // wsum is reused; and the list is complete for wave 0 below
  }
  if (wv != 0) return;
  total = __builtin_amdgcn_readfirstlane(total);

  // model/fmRDSblock.py:219, the value search as written: the first of the last 24 samples equal
  // to the last symbol (24 is a legal result)
  const int next_io = RDS_SPS - (__ffsll(eq) - 1);
  const uint8_t* __restrict__ diff = a.diff + (int64_t)s * a.diff_stride;
  const int last_b = a.bits[(int64_t)s * a.bits_stride + p.nb - 1];
  const int cb = lane < 27 ? diff[p.L - 27 + lane] : 0;   // L >= 30 at the minimum n
  const uint32_t carried = (uint32_t)__ballot(cb != 0);

  // the frame rule over the matches (capi.hip sdr_rds_link_block :299-341); window numbers
  // relative to the call's first position, so the state is 32-bit: `last` = last_position - pp0
  // (LAST_NONE for -1; a position further back than that can never be 26 behind a match again)
  constexpr int LAST_NONE = -(1 << 30) - 1, LAST_OLD = -(1 << 30);
  const int64_t pp0 = st.printposition;
  const int64_t rel = st.last_position - pp0;
  int last = __builtin_amdgcn_readfirstlane(st.last_position == -1 ? LAST_NONE : rel < -64 ? LAST_OLD : (int)rel);
  int bad = __builtin_amdgcn_readfirstlane(st.bad_sync);
  const int resync = a.resync;
  int64_t* __restrict__ ev = a.ev + (int64_t)s * a.max_events * 4;
  int64_t ne = 0;
  auto store = [&](int64_t idx, int64_t type, int64_t pos, int64_t ok, int64_t word) {
    if (idx < a.max_events) {
      ev[4 * idx] = type;
      ev[4 * idx + 1] = pos;
      ev[4 * idx + 2] = ok;
      ev[4 * idx + 3] = word;
    }
  };
  // The host checks the re-sync rule at every window, but the count only moves at a match:
  // beyond the matches only window 0 can fire (a threshold lowered between two calls), and
  // only if no match at window 0 comes first.
  if (resync > 0 && bad > resync) {
    const uint32_t w_first = total > 0 ? cm[0].x : 1u;
    if (w_first != 0u) {
      if (lane == 0) store(ne, SDR_RDS_RESYNC, pp0, 0, 0);
      ++ne;
      bad = 0;
      last = LAST_NONE;
    }
  }
  for (int m0 = 0; m0 < total; m0 += 64) {
    const int nm = total - m0 < 64 ? total - m0 : 64;
    uint2 mine = uint2{0u, 0u};
    if (lane < nm) mine = cm[m0 + lane];
    unsigned long long okm = 0ull, rsm = 0ull;
    for (int j = 0; j < nm; ++j) {
      const int w = __builtin_amdgcn_readlane((int)mine.x, j);
      const bool ok = last == LAST_NONE || w - last == 26;
      if (ok) last = w;
      bad = ok ? 0 : bad + 1;
      okm |= (unsigned long long)ok << j;
      if (resync > 0 && bad > resync) {
        rsm |= 1ull << j;
        bad = 0;
        last = LAST_NONE;
      }
    }
    if (lane < nm) {
      const int64_t idx = ne + lane + __popcll(rsm & ((1ull << lane) - 1ull));
      const int64_t pos = pp0 + (int64_t)mine.x;
      store(idx, (mine.y >> 16) & 3u, pos, (okm >> lane) & 1ull, mine.y & 0xffffu);
      if ((rsm >> lane) & 1ull) store(idx + 1, SDR_RDS_RESYNC, pos, 0, 0);
    }
    ne += nm + __popcll(rsm);
  }

  if (lane == 0) {
    st.started = 1;
    st.int_offset = next_io;
    st.start_pos = sp;
    st.front_bit = front;
    st.prebit = last_b;
    if (sp == 1) st.lonely_bit = slast;
    st.carried = carried & 0x7ffffffu;
    st.ncarried = 27;
    st.printposition = pp0 + p.W - 1;      // the last window is the next call's first
    if (last == LAST_NONE) st.last_position = -1;
    else if (last != LAST_OLD) st.last_position = pp0 + last;
    st.bad_sync = bad;
    a.state[s] = st;
    a.nev[s] = ne;
    a.status[s] = ne > a.max_events ? SDR_RDS_LINKS_OVERFLOW : 0;
    a.nbd[2 * s] = p.nb;
    a.nbd[2 * s + 1] = p.L;
    a.added[2 * s] = p.C;
    a.added[2 * s + 1] = p.L - p.C;
  }
}

}  // namespace

struct sdr_rds_links {
  sdr_ctx* ctx = nullptr;
  int S = 0, resync = 0;
  int64_t max_n = 0, max_events = 0;
  int64_t sym_stride = 0, bits_stride = 0, diff_stride = 0, tiles_stride = 0;
  RdsState* state = nullptr;
  float* sym = nullptr;
  uint8_t* bits = nullptr;
  uint8_t* diff = nullptr;
  unsigned* cnt = nullptr;
  int* tcount = nullptr;
  uint32_t* rec = nullptr;
  uint2* cm = nullptr;
  int* nbd = nullptr;
  int* added = nullptr;
  int64_t* ev = nullptr;
  int64_t* nev = nullptr;
  int* status = nullptr;
  DevMem mem;
};

namespace {

// the most symbols, bits and scanned bits a row of n samples gives (offset 0; 27 carried bits)
int64_t max_symbols(int64_t n) { return (n + RDS_SPS - 1) / RDS_SPS; }
int64_t max_scanned(int64_t n) { return 27 + max_symbols(n) / 2; }

}  // namespace

// what the block sync stage (rds_sync.hip) reads of a link bank
sdrint::RdsLinksView sdrint::rds_links_view(const sdr_rds_links* l) {
  return RdsLinksView{l->ctx, l->S, max_scanned(l->max_n) - 27, l->diff, l->diff_stride, l->added};
}

extern "C" {

int sdr_rds_links_create(sdr_ctx* c, int nstreams, int64_t max_n, int64_t max_events, sdr_rds_links** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_create: out is NULL");
  *out = nullptr;
  if (nstreams < 1 || nstreams > SDR_RDS_LINKS_MAX_STREAMS)
    return fail(SDR_EINVAL, "sdr_rds_links_create: nstreams=%d outside [1, %d]", nstreams, SDR_RDS_LINKS_MAX_STREAMS);
  if (max_n < SDR_RDS_LINKS_MIN_N || max_n > SDR_RDS_LINKS_MAX_N)
    return fail(SDR_EINVAL, "sdr_rds_links_create: max_n=%lld outside [%d, %d]", (long long)max_n, SDR_RDS_LINKS_MIN_N,
                SDR_RDS_LINKS_MAX_N);
  if (max_events < 1 || max_events > SDR_RDS_LINKS_MAX_EVENTS)
    return fail(SDR_EINVAL, "sdr_rds_links_create: max_events=%lld outside [1, %d]", (long long)max_events,
                SDR_RDS_LINKS_MAX_EVENTS);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rds_links* l = new (std::nothrow) sdr_rds_links;
  if (l == nullptr) return fail(SDR_ENOMEM, "sdr_rds_links_create: out of host memory");
  l->ctx = c;
  l->S = nstreams;
  l->max_n = max_n;
  l->max_events = max_events;
  l->sym_stride = (max_symbols(max_n) + 3) / 4 * 4;
  l->bits_stride = (max_symbols(max_n) / 2 + 15) / 16 * 16;
  l->diff_stride = (max_scanned(max_n) + 15) / 16 * 16;
  l->tiles_stride = ceil_div(max_scanned(max_n), RDS_TILE);
  const size_t S = (size_t)nstreams;
  DevMem& m = l->mem;             // `true`: what a reset clears
  m.get(&l->state, S, true);
  m.get(&l->sym, S * l->sym_stride);
  m.get(&l->bits, S * l->bits_stride);
  m.get(&l->diff, S * l->diff_stride);
  m.get(&l->cnt, 2 * S, true);
  m.get(&l->tcount, S * l->tiles_stride);
  m.get(&l->rec, S * l->tiles_stride * RDS_TILE);
  m.get(&l->cm, S * l->tiles_stride * RDS_TILE);
  m.get(&l->nbd, 2 * S, true);
  m.get(&l->added, 2 * S, true);
  m.get(&l->ev, 4 * S * (size_t)max_events);
  m.get(&l->nev, S, true);
  m.get(&l->status, S, true);
  if (m.err == hipSuccess) m.err = m.zero(c->stream);
  if (m.err != hipSuccess) {
    const hipError_t e = m.err;
    sdr_rds_links_destroy(l);
    return create_failed(e, "sdr_rds_links_create");
  }
  *out = l;
  return SDR_OK;
}

void sdr_rds_links_destroy(sdr_rds_links* l) {
  if (l == nullptr) return;
  if (l->ctx != nullptr && set_dev(l->ctx) == SDR_OK) (void)hipStreamSynchronize(l->ctx->stream);
  l->mem.release();
  delete l;
}

int sdr_rds_links_set_resync(sdr_rds_links* l, int after_bad_syncs) {
  if (l == nullptr || after_bad_syncs < 0) return fail(SDR_EINVAL, "sdr_rds_links_set_resync: bad arguments");
  l->resync = after_bad_syncs;
  return SDR_OK;
}

int sdr_rds_links_reset(sdr_rds_links* l) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_reset: object is NULL");
  TRY(set_dev(l->ctx));
  HIP_TRY(l->mem.zero(l->ctx->stream));
  return SDR_OK;
}

int sdr_rds_links_process_dev(sdr_rds_links* l, const float* rrc_i, int64_t n, int64_t stride) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_process_dev: object is NULL");
  if (rrc_i == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_process_dev: rrc_i is NULL");
  if (n < SDR_RDS_LINKS_MIN_N || n > l->max_n)
    return fail(SDR_EINVAL, "sdr_rds_links_process_dev: n=%lld outside [%d, max_n=%lld]", (long long)n, SDR_RDS_LINKS_MIN_N,
                (long long)l->max_n);
  if (stride < n) return fail(SDR_EINVAL, "sdr_rds_links_process_dev: stride=%lld < n=%lld", (long long)stride, (long long)n);
  if (((uintptr_t)rrc_i & 3) != 0) return fail(SDR_EINVAL, "sdr_rds_links_process_dev: rrc_i must be aligned to 4 B");
  sdr_ctx* c = l->ctx;
  TRY(set_dev(c));
  RdsArgs a;
  a.x = rrc_i;
  a.n = n;
  a.stride = stride;
  a.state = l->state;
  a.sym = l->sym;
  a.sym_stride = l->sym_stride;
  a.bits = l->bits;
  a.bits_stride = l->bits_stride;
  a.diff = l->diff;
  a.diff_stride = l->diff_stride;
  a.cnt = l->cnt;
  a.tcount = l->tcount;
  a.rec = l->rec;
  a.cm = l->cm;
  a.tiles_stride = l->tiles_stride;
  a.nbd = l->nbd;
  a.added = l->added;
  a.ev = l->ev;
  a.nev = l->nev;
  a.status = l->status;
  a.max_events = l->max_events;
  a.resync = l->resync;
  // grids for the most symbols and scanned bits a row of n gives; the kernels bound themselves
  // by the stream's own counts
  const unsigned gpairs = (unsigned)ceil_div(ceil_div(max_symbols(n), 2), RDS_T);
  const unsigned gtiles = (unsigned)ceil_div(max_scanned(n), RDS_TILE);   // <= tiles_stride: n <= max_n
  hipLaunchKernelGGL(rds_gather_kernel, dim3(gpairs, (unsigned)l->S), dim3(RDS_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_scan_kernel, dim3(gtiles, (unsigned)l->S), dim3(RDS_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_frame_kernel, dim3((unsigned)l->S), dim3(RDS_T), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return SDR_OK;
}

int sdr_rds_links_events(sdr_rds_links* l, int64_t* ev, int64_t* n_events, int32_t* status) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_events: object is NULL");
  sdr_ctx* c = l->ctx;
  TRY(set_dev(c));
  const size_t S = (size_t)l->S;
  if (ev) HIP_TRY(hipMemcpyAsync(ev, l->ev, sizeof(int64_t) * 4 * S * (size_t)l->max_events, hipMemcpyDeviceToHost, c->stream));
  if (n_events) HIP_TRY(hipMemcpyAsync(n_events, l->nev, sizeof(int64_t) * S, hipMemcpyDeviceToHost, c->stream));
  if (status) HIP_TRY(hipMemcpyAsync(status, l->status, sizeof(int) * S, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_rds_links_bits(sdr_rds_links* l, int stream, uint8_t* bits, int64_t max_bits, int64_t* n_bits, uint8_t* diff,
                       int64_t max_diff, int64_t* n_diff) {
  if (l == nullptr) return fail(SDR_EINVAL, "sdr_rds_links_bits: object is NULL");
  if (stream < 0 || stream >= l->S) return fail(SDR_EINVAL, "sdr_rds_links_bits: stream %d outside [0, %d)", stream, l->S);
  sdr_ctx* c = l->ctx;
  TRY(set_dev(c));
  int nbd[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(nbd, l->nbd + 2 * stream, sizeof(nbd), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_bits) *n_bits = nbd[0];
  if (n_diff) *n_diff = nbd[1];
  if (bits && nbd[0] > max_bits) return fail(SDR_EINVAL, "sdr_rds_links_bits: bits buffer too small (%d bits)", nbd[0]);
  if (diff && nbd[1] > max_diff) return fail(SDR_EINVAL, "sdr_rds_links_bits: diff buffer too small (%d bits)", nbd[1]);
  if (bits && nbd[0] > 0)
    HIP_TRY(hipMemcpyAsync(bits, l->bits + (size_t)stream * l->bits_stride, (size_t)nbd[0], hipMemcpyDeviceToHost, c->stream));
  if (diff && nbd[1] > 0)
    HIP_TRY(hipMemcpyAsync(diff, l->diff + (size_t)stream * l->diff_stride, (size_t)nbd[1], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

}  // extern "C"
