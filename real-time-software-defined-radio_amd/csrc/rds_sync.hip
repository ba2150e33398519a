// RDS block synchronisation on the device (include/sdr.h sdr_rds_sync_*): every stream's
// differential bits -> block records {type, position, status, word}, with acquisition on two
// consecutive offset syndromes, a flywheel over bad blocks, the (26, 16) code's burst correction
// and offset C'.  The host model rdssync.py RdsBlockSync is the specification; this file restates
// it so that records, state and counters are the same after every call, whatever the split.
//
// A call's row of a stream is its carried bits (the last <= 51 of the earlier calls) followed by
// the new ones; local index i of the row is stream position base + i.  Two launches per call,
// whatever nstreams and n are; no atomics, no workgroup waits for another:
//   windows  a workgroup per tile of SY_TILE positions: the waves pack the tile's bits plus a
//            32-bit halo on either side into LDS words by ballot, and each thread takes its
//            window and the one 26 bits before it by funnel shifts: the 10-bit syndrome, the
//            offset type, the 16 information bits, and the acquisition predicate (both windows
//            offset syndromes in consecutive slots), which depends on positions only.
//   track    one wave per stream, alternating two parallel searches over those entries.  SYNC: a
//            lane takes a block (64 blocks a round), looks its error syndrome up in the burst
//            table -- a slot-2 lane without an exact C / C' syndrome takes the version bit from
//            its B neighbour's corrected word --, the not-error-free flags are balloted, each
//            lane extends bad_run across the mask with a count of leading zeros, and the first
//            lane to reach lose_after ends the round behind it.  SEARCH: a lane takes a position
//            (512 a round), the predicate is balloted and the first set bit acquires.  The lanes
//            store their records side by side; the wave writes the next state and carried bits.
// The code -- H, the offset syndromes and types, the burst table, a window out of the LDS words,
// its information word -- is rds_code.h's.
#include <hip/hip_runtime.h>

#include <new>

#include "rds_code.h"
#include "rds_links.h"
#include "sdr_ctx.h"

using namespace sdrint;

namespace {

constexpr int SY_T = 256, SY_TILE = 256, SY_NW = SY_T / 64, SY_CARRY = 51, SY_SEARCH = 8;
static_assert(SY_TILE == SY_T, "one position of the row per thread");

// a window's entry: the syndrome, the offset type (TYPE_NONE: none), the acquisition predicate
// and the 16 information bits
constexpr int E_TYPE = 10, E_ACQ = 13, E_WORD = 16;

enum { MODE_SEARCH = 0, MODE_SYNC = 1 };

// a stream's carried state; all zero = reset
struct SyncState {
  int64_t total;                // bits taken since reset
  int64_t pos;                  // SEARCH: s0; SYNC: the next block's position
  int64_t count[5];             // blocks of status 0 / 1 / 2, acquisitions, losses
  unsigned long long carried;   // bit i = carried bit i (the row's first ncarried bits)
  int ncarried, mode, slot, bad_run;
  int bword, bvalid;            // the word of the record 26 bits before `pos`, if it is usable
};

struct SyncArgs {
  const uint8_t* bits; int64_t n, stride;
  const int* counts;            // NULL, or [stream]: the stream's bit count 0 .. n
  const int* added;             // NULL, or [stream][2] = {first byte of the row, count} (a link bank's rows)
  SyncState* state;
  uint32_t* win; int64_t win_stride;
  const uint32_t* table;        // [1024] by error syndrome: 1 << 16 | the information bits to flip; 0 = not correctable
  int64_t* rec; int64_t* nrec; int64_t max_records;
  int lose_after;
};

// the call's row of stream s: ncarried carried bits, then cnt new ones at src
struct SyncRow {
  const uint8_t* src;
  int nc, cnt, L, W;            // W windows: local 0 .. W - 1
};
__device__ __forceinline__ SyncRow row_of(const SyncArgs& a, const SyncState& st, int s) {
  SyncRow r;
  int off = 0;
  int64_t cnt = a.n;
  if (a.added != nullptr) {
    off = a.added[2 * s];
    cnt = a.added[2 * s + 1];
  } else if (a.counts != nullptr) {
    cnt = a.counts[s];
  }
  cnt = cnt < 0 ? 0 : cnt > a.n ? a.n : cnt;
  r.src = a.bits + (int64_t)s * a.stride + off;
  r.nc = st.ncarried;
  r.cnt = (int)cnt;
  r.L = r.nc + r.cnt;
  r.W = r.L - 25;
  return r;
}
__device__ __forceinline__ int row_bit(const SyncRow& r, const SyncState& st, int i) {
  return i < r.nc ? (int)((st.carried >> i) & 1ull) : (int)(r.src[i - r.nc] & 1u);
}

__global__ __launch_bounds__(SY_T) void rds_sync_windows_kernel(const SyncArgs a) {
  __shared__ uint32_t dw[2 * SY_NW + 2];        // bits w0 - 32 .. w0 + SY_TILE + 32
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const SyncState st = a.state[s];
  const SyncRow r = row_of(a, st, s);
  const int w0 = blockIdx.x * SY_TILE;
  if (w0 >= r.W) return;                        // the whole workgroup: no window starts here
  const int i = w0 + tid;
  const int d = i < r.L ? row_bit(r, st, i) : 0;
  const unsigned long long mk = __ballot(d != 0);
  if (lane == 0) {
    dw[1 + 2 * wv] = (uint32_t)mk;
    dw[2 + 2 * wv] = (uint32_t)(mk >> 32);
  }
  if (wv == 0) {                                // the 32 bits before the tile and the 32 after it
    const int i2 = lane < 32 ? w0 - 32 + lane : w0 + SY_TILE + lane - 32;
    const int d2 = i2 >= 0 && i2 < r.L ? row_bit(r, st, i2) : 0;
    const unsigned long long mh = __ballot(d2 != 0);
    if (lane == 0) {
      dw[0] = (uint32_t)mh;
      dw[2 * SY_NW + 1] = (uint32_t)(mh >> 32);
    }
  }
  __syncthreads();
  if (i >= r.W) return;
  const uint32_t v = window_at(dw, 32 + tid), vp = window_at(dw, 6 + tid);      // the thread's, and the one 26 bits before it
  const uint32_t syn = syndrome_of(v);
  const int typ = type_of(syn), typ_p = type_of(syndrome_of(vp));
  const bool acq = i >= 26 && typ != TYPE_NONE && typ_p != TYPE_NONE && slot_of_type(typ) == ((slot_of_type(typ_p) + 1) & 3);
  a.win[(int64_t)s * a.win_stride + i] = (info_word(v) << E_WORD) | ((uint32_t)acq << E_ACQ) | ((uint32_t)typ << E_TYPE) | syn;
}

// a block of the given type: status 0 / 1 / 2 and the information word after correction
__device__ __forceinline__ void classify(uint32_t syn, uint32_t word, int typ, const uint32_t* __restrict__ table, int* status,
                                         uint32_t* cword) {
  const uint32_t e = syn ^ syn_of_type(typ);
  const uint32_t t = table[e];
  *status = e == 0u ? 0 : (t >> 16) != 0u ? 1 : 2;
  *cword = e != 0u && (t >> 16) != 0u ? word ^ (t & 0xffffu) : word;
}

__global__ __launch_bounds__(64) void rds_sync_track_kernel(const SyncArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  SyncState st = a.state[s];
  const SyncRow r = row_of(a, st, s);
  const int64_t base = st.total - st.ncarried;
  const uint32_t* __restrict__ win = a.win + (int64_t)s * a.win_stride;
  const uint32_t* __restrict__ table = a.table;
  int64_t* __restrict__ rec = a.rec + (int64_t)s * a.max_records * 4;
  auto store = [&](int64_t idx, int64_t type, int64_t pos, int64_t status, int64_t word) {
    if (idx < a.max_records) {
      rec[4 * idx] = type;
      rec[4 * idx + 1] = pos;
      rec[4 * idx + 2] = status;
      rec[4 * idx + 3] = word;
    }
  };
  int mode = st.mode, slot = st.slot, bad = st.bad_run, bvalid = st.bvalid;
  uint32_t bword = (uint32_t)st.bword;
  int64_t pos = st.pos, nr = 0;
  int64_t n0 = 0, n1 = 0, n2 = 0, nacq = 0, nloss = 0;

  for (;;) {
    if (mode == MODE_SYNC) {
      if (pos - base >= r.W) break;             // the next block is not complete yet
      const int q = (int)(pos - base);          // >= 0: a block that was not complete lies in the carried bits
      const int nblk = (r.W - 1 - q) / 26 + 1;
      const int m = nblk < 64 ? nblk : 64;
      const bool act = lane < m;
      const int i = q + 26 * lane;
      const int k = (slot + lane) & 3;
      const uint32_t e = act ? win[i] : 0u;
      const uint32_t syn = e & 0x3ffu, word = e >> E_WORD;
      int typ = k;
      bool need_b = false;
      if (k == 2) {                             // an exact C or C' decides; else the B word before it
        if (syn == SYN_CP) typ = TYPE_CP;
        else if (syn != SYN_C) need_b = true;
      }
      int status;
      uint32_t cw;
      classify(syn, word, typ, table, &status, &cw);
      int bst = __shfl_up(status, 1, 64);       // the lane before a slot-2 lane holds slot 1: final already
      uint32_t bw = (uint32_t)__shfl_up((int)cw, 1, 64);
      if (lane == 0) {
        bst = bvalid ? 0 : 2;
        bw = bword;
      }
      if (need_b) {
        if (bst <= 1) {
          typ = ((bw >> 11) & 1u) ? TYPE_CP : 2;
          classify(syn, word, typ, table, &status, &cw);
        } else {
          typ = 2;
          status = 2;
          cw = word;
        }
      }
      // bad_run behind each lane: the run of not-error-free blocks that ends at it
      const unsigned long long nz = __ballot(act && status != 0);
      const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
      const unsigned long long zeros = ~nz & upto;
      const int run = zeros == 0ull ? lane + 1 + bad : lane - (63 - __clzll((long long)zeros));
      const unsigned long long lossm = __ballot(act && run >= a.lose_after);
      const int keep = lossm != 0ull ? __ffsll((long long)lossm) : m;      // blocks 0 .. keep - 1 are this run's
      const bool mine = lane < keep;
      if (mine) store(nr + lane, typ, base + i, status, cw);
      n0 += __popcll(__ballot(mine && status == 0));
      n1 += __popcll(__ballot(mine && status == 1));
      n2 += __popcll(__ballot(mine && status == 2));
      nr += keep;
      pos += 26 * (int64_t)keep;
      slot = (slot + keep) & 3;
      if (lossm != 0ull) {
        ++nloss;
        mode = MODE_SEARCH;                     // s0 = pos, behind the block that lost sync
        bad = 0;
        bvalid = 0;
      } else {
        const int lst = __shfl(status, keep - 1, 64);
        bad = __shfl(run, keep - 1, 64);
        bvalid = lst <= 1;
        bword = (uint32_t)__shfl((int)cw, keep - 1, 64);
      }
    } else {
      // candidates: p - 26 >= s0, and the window 26 before it in this row (an earlier one has
      // been tried by the call that completed it, or lies before s0)
      int64_t i0 = pos + 26 - base;
      if (i0 < 26) i0 = 26;
      int found = -1;
      while (i0 < r.W && found < 0) {
        uint32_t ent[SY_SEARCH];
#pragma unroll
        for (int j = 0; j < SY_SEARCH; ++j) {
          const int64_t idx = i0 + j * 64 + lane;
          ent[j] = idx < r.W ? win[idx] : 0u;
        }
#pragma unroll
        for (int j = 0; j < SY_SEARCH; ++j) {
          const unsigned long long hit = __ballot((ent[j] >> E_ACQ) & 1u);
          if (found < 0 && hit != 0ull) found = (int)i0 + j * 64 + __ffsll((long long)hit) - 1;
        }
        i0 += 64 * SY_SEARCH;
      }
      if (found < 0) break;
      const uint32_t e1 = win[found], e0 = win[found - 26];
      const int t1 = (int)((e1 >> E_TYPE) & 7u), t0 = (int)((e0 >> E_TYPE) & 7u);
      if (lane == 0) {
        store(nr, t0, base + found - 26, 0, e0 >> E_WORD);
        store(nr + 1, t1, base + found, 0, e1 >> E_WORD);
      }
      nr += 2;
      n0 += 2;
      ++nacq;
      mode = MODE_SYNC;
      pos = base + found + 26;
      slot = (slot_of_type(t1) + 1) & 3;
      bad = 0;
      bvalid = 1;
      bword = e1 >> E_WORD;
    }
  }

  // the row's last <= 51 bits are the next call's first
  const int nc2 = r.L < SY_CARRY ? r.L : SY_CARRY;
  const int cb = lane < nc2 ? row_bit(r, st, r.L - nc2 + lane) : 0;
  const unsigned long long carried = __ballot(cb != 0);
  if (lane == 0) {
    st.total += r.cnt;
    st.pos = pos;
    st.count[0] += n0;
    st.count[1] += n1;
    st.count[2] += n2;
    st.count[3] += nacq;
    st.count[4] += nloss;
    st.carried = carried;
    st.ncarried = nc2;
    st.mode = mode;
    st.slot = slot;
    st.bad_run = bad;
    st.bword = (int)bword;
    st.bvalid = bvalid;
    a.state[s] = st;
    a.nrec[s] = nr;
  }
}

}  // namespace

struct sdr_rds_sync {
  sdr_ctx* ctx = nullptr;
  int S = 0, max_burst = 2, lose_after = 12;
  int64_t max_bits = 0, max_records = 0, win_stride = 0;
  SyncState* state = nullptr;
  uint32_t* win = nullptr;
  uint32_t* table = nullptr;
  int64_t* rec = nullptr;
  int64_t* nrec = nullptr;
  uint32_t host_table[1024] = {};
  DevMem mem;
};

namespace {

// the decoder's table (rds_code.h burst_table) to the device
int build_table(sdr_rds_sync* y, int max_burst) {
  if (burst_table(max_burst, y->host_table)) return fail(SDR_EINVAL, "sdr_rds_sync_set_params: burst syndromes collide");
  HIP_TRY(hipMemcpyAsync(y->table, y->host_table, sizeof(y->host_table), hipMemcpyHostToDevice, y->ctx->stream));
  HIP_TRY(hipStreamSynchronize(y->ctx->stream));
  return SDR_OK;
}

int launch_sync(sdr_rds_sync* y, const uint8_t* bits, int64_t n, int64_t stride, const int* counts, const int* added) {
  sdr_ctx* c = y->ctx;
  SyncArgs a;
  a.bits = bits;
  a.n = n;
  a.stride = stride;
  a.counts = counts;
  a.added = added;
  a.state = y->state;
  a.win = y->win;
  a.win_stride = y->win_stride;
  a.table = y->table;
  a.rec = y->rec;
  a.nrec = y->nrec;
  a.max_records = y->max_records;
  a.lose_after = y->lose_after;
  // a grid for the longest row a call of n can give; the kernels bound themselves by the stream's own
  const unsigned gtiles = (unsigned)ceil_div(n + SY_CARRY, SY_TILE);      // <= win_stride / SY_TILE: n <= max_bits
  hipLaunchKernelGGL(rds_sync_windows_kernel, dim3(gtiles, (unsigned)y->S), dim3(SY_T), 0, c->stream, a);
  hipLaunchKernelGGL(rds_sync_track_kernel, dim3((unsigned)y->S), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_rds_sync_create(sdr_ctx* c, int nstreams, int64_t max_bits, sdr_rds_sync** out) {
  if (out == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_create: out is NULL");
  *out = nullptr;
  if (nstreams < 1 || nstreams > SDR_RDS_SYNC_MAX_STREAMS)
    return fail(SDR_EINVAL, "sdr_rds_sync_create: nstreams=%d outside [1, %d]", nstreams, SDR_RDS_SYNC_MAX_STREAMS);
  if (max_bits < 1 || max_bits > SDR_RDS_SYNC_MAX_BITS)
    return fail(SDR_EINVAL, "sdr_rds_sync_create: max_bits=%lld outside [1, %d]", (long long)max_bits, SDR_RDS_SYNC_MAX_BITS);
  CHECK_CTX(c);
  TRY(set_dev(c));
  sdr_rds_sync* y = new (std::nothrow) sdr_rds_sync;
  if (y == nullptr) return fail(SDR_ENOMEM, "sdr_rds_sync_create: out of host memory");
  y->ctx = c;
  y->S = nstreams;
  y->max_bits = max_bits;
  y->max_records = max_bits / 26 + 3;
  y->win_stride = ceil_div(max_bits + SY_CARRY, SY_TILE) * SY_TILE;
  const size_t S = (size_t)nstreams;
  DevMem& m = y->mem;             // `true`: what a reset clears
  m.get(&y->state, S, true);
  m.get(&y->win, S * y->win_stride);
  m.get(&y->table, 1024);
  m.get(&y->rec, 4 * S * (size_t)y->max_records);
  m.get(&y->nrec, S, true);
  if (m.err == hipSuccess) m.err = m.zero(c->stream);
  if (m.err != hipSuccess) {
    const hipError_t e = m.err;
    sdr_rds_sync_destroy(y);
    return create_failed(e, "sdr_rds_sync_create");
  }
  const int rc = build_table(y, y->max_burst);
  if (rc != SDR_OK) {
    sdr_rds_sync_destroy(y);
    return rc;
  }
  *out = y;
  return SDR_OK;
}

void sdr_rds_sync_destroy(sdr_rds_sync* y) {
  if (y == nullptr) return;
  if (y->ctx != nullptr && set_dev(y->ctx) == SDR_OK) (void)hipStreamSynchronize(y->ctx->stream);
  y->mem.release();
  delete y;
}

int sdr_rds_sync_reset(sdr_rds_sync* y) {
  if (y == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_reset: object is NULL");
  TRY(set_dev(y->ctx));
  HIP_TRY(y->mem.zero(y->ctx->stream));
  return SDR_OK;
}

int sdr_rds_sync_set_params(sdr_rds_sync* y, int max_burst, int lose_after) {
  if (y == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_set_params: object is NULL");
  if (max_burst < 0 || max_burst > SDR_RDS_SYNC_MAX_BURST)
    return fail(SDR_EINVAL, "sdr_rds_sync_set_params: max_burst=%d outside [0, %d]", max_burst, SDR_RDS_SYNC_MAX_BURST);
  if (lose_after < 1 || lose_after > 255)
    return fail(SDR_EINVAL, "sdr_rds_sync_set_params: lose_after=%d outside [1, 255]", lose_after);
  TRY(set_dev(y->ctx));
  HIP_TRY(hipStreamSynchronize(y->ctx->stream));      // calls in flight read the table being replaced
  TRY(build_table(y, max_burst));
  y->max_burst = max_burst;
  y->lose_after = lose_after;
  return SDR_OK;
}

int sdr_rds_sync_process_dev(sdr_rds_sync* y, const uint8_t* bits, int64_t n, int64_t stride, const int32_t* counts_dev) {
  if (y == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_process_dev: object is NULL");
  if (bits == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_process_dev: bits is NULL");
  if (n < 0 || n > y->max_bits)
    return fail(SDR_EINVAL, "sdr_rds_sync_process_dev: n=%lld outside [0, max_bits=%lld]", (long long)n, (long long)y->max_bits);
  if (stride < n) return fail(SDR_EINVAL, "sdr_rds_sync_process_dev: stride=%lld < n=%lld", (long long)stride, (long long)n);
  if (((uintptr_t)counts_dev & 3) != 0) return fail(SDR_EINVAL, "sdr_rds_sync_process_dev: counts_dev must be aligned to 4 B");
  TRY(set_dev(y->ctx));
  return launch_sync(y, bits, n, stride, counts_dev, nullptr);
}

int sdr_rds_sync_process_links(sdr_rds_sync* y, sdr_rds_links* links) {
  if (y == nullptr || links == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_process_links: object is NULL");
  const RdsLinksView v = rds_links_view(links);
  if (v.ctx != y->ctx) return fail(SDR_EINVAL, "sdr_rds_sync_process_links: the link bank lives on another context");
  if (v.S != y->S) return fail(SDR_EINVAL, "sdr_rds_sync_process_links: the link bank has %d streams, the sync %d", v.S, y->S);
  if (v.max_added > y->max_bits)
    return fail(SDR_EINVAL, "sdr_rds_sync_process_links: a link call can add %lld bits, max_bits=%lld", (long long)v.max_added,
                (long long)y->max_bits);
  TRY(set_dev(y->ctx));
  return launch_sync(y, v.diff, v.max_added, v.diff_stride, nullptr, v.added);
}

int sdr_rds_sync_blocks(sdr_rds_sync* y, int64_t* rec, int64_t* n_rec) {
  if (y == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_blocks: object is NULL");
  sdr_ctx* c = y->ctx;
  TRY(set_dev(c));
  const size_t S = (size_t)y->S;
  if (rec) HIP_TRY(hipMemcpyAsync(rec, y->rec, sizeof(int64_t) * 4 * S * (size_t)y->max_records, hipMemcpyDeviceToHost, c->stream));
  if (n_rec) HIP_TRY(hipMemcpyAsync(n_rec, y->nrec, sizeof(int64_t) * S, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return SDR_OK;
}

int sdr_rds_sync_state(sdr_rds_sync* y, int32_t* synced, int64_t* next_pos, int64_t* counters) {
  if (y == nullptr) return fail(SDR_EINVAL, "sdr_rds_sync_state: object is NULL");
  std::vector<SyncState> st;
  TRY(fetch_states(y->ctx, y->state, y->S, &st));
  for (int s = 0; s < y->S; ++s) {
    if (synced) synced[s] = st[s].mode == MODE_SYNC;
    if (next_pos) next_pos[s] = st[s].pos;
    if (counters)
      for (int k = 0; k < 5; ++k) counters[5 * s + k] = st[s].count[k];
  }
  return SDR_OK;
}

}  // extern "C"
