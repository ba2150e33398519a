// What the streaming row blocks share (ddc.hip, pfb.hip, rsmp.hip): the history a block carries
// from call to call, and the load that reads a window lying across the seam between that history
// and the caller's buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sdr_mma.h"

namespace sdrint {

// ---- the seam load (device) --------------------------------------------------------------------
// A window of a streaming kernel that begins before the call's first sample, or ends after its
// last, is read element by element through two range-checked buffer descriptors (mm_rsrc): `in`
// over the caller's samples and `hist` over the samples that preceded the call.  Three facts make
// it safe, and every user depends on all three:
//  1. a descriptor reads 0 past its range, so the element comes from exactly one of the two
//     loads and the two results are OR-ed -- no branch, and no access leaves either buffer;
//  2. the range check does not wrap: a load that starts below the range and ends inside it reads
//     0 for the part inside, so a negative offset must not reach the instruction.  An index
//     below a range is turned into an offset past it instead (seam_off);
//  3. that has to hold for what the compiler makes of the loads as well: it may merge two
//     adjacent loads into a wider one, or fold a constant of the index into the instruction's
//     immediate-offset field.  Both are sound for offsets that are non-negative or past the
//     range, which is all seam_off returns.
// UNIT is the bytes per index step, BYTES the width of a load: ddc.hip indexes elements (I or Q)
// and loads complex samples, BYTES = 2 UNIT, so its unrolled loop multiplies by nothing new; pfb.hip
// and rsmp.hip index what they load.  d0 and h0 are the indices of the window's element 0 in the
// caller's range and in the history's: where the window starts, how long the caller's range is
// and whether the history is consulted at all is the kernel's arithmetic.
template <int UNIT>
static __device__ __forceinline__ int seam_off(int e) { return e < 0 ? 0x7ffffff0 : e * UNIT; }

template <int BYTES>
static __device__ __forceinline__ auto seam_ld(__amdgpu_buffer_rsrc_t r, int off) {
  static_assert(BYTES == 2 || BYTES == 4 || BYTES == 8, "a u8 pair, an f32 or an f32 pair");
  if constexpr (BYTES == 2) return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0);   // (the low 16 bits count)
  else if constexpr (BYTES == 4) return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
  else return (u2v)__builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
}

template <int UNIT>
struct Seam {
  __amdgpu_buffer_rsrc_t in, hist;
  int d0, h0;
  // element i + K of the window, from the caller's range alone.  K is a compile-time step added
  // after the window's origin, (d0 + i) + K: one index register then serves the neighbouring
  // loads of an unrolled loop (d0 + (i + K) costs ddc.hip 14 VGPRs and a wave of occupancy)
  template <int BYTES, int K = 0>
  __device__ __forceinline__ auto load_in(int i) const { return seam_ld<BYTES>(in, seam_off<UNIT>(d0 + i + K)); }
  // ... from whichever of the two ranges holds it
  template <int BYTES, int K = 0>
  __device__ __forceinline__ auto load(int i) const { return load_in<BYTES, K>(i) | seam_ld<BYTES>(hist, seam_off<UNIT>(h0 + i + K)); }
};

// ---- the carried history (host) ----------------------------------------------------------------
// the new history: the last HL samples of (old history, the call's n samples), row blockIdx.y
template <typename PT>
__global__ void stream_hist_kernel(const PT* in, const PT* hold, PT* hnew, int64_t n, int64_t in_stride, int HL) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HL) return;
  const int64_t row = blockIdx.y;
  const int64_t k = n - HL + i;
  hnew[row * HL + i] = k >= 0 ? in[row * in_stride + k] : hold[row * HL + HL + k];
}

// The HL samples per row that preceded the next call, in one of two slots: a call reads
// current() while a second launch fills the other slot, which then becomes current.
struct StreamHist {
  void* slot[2] = {nullptr, nullptr};
  size_t bytes = 0;
  int cur = 0;
  int fill = 0;   // the byte of a silent history: 128 for u8 samples (their zero level), 0 for f32

  // for a create's error chain: a partial failure is undone by free()
  hipError_t alloc(size_t nbytes, int fill_byte, hipStream_t st) {
    bytes = std::max<size_t>(16, nbytes);
    fill = fill_byte;
    hipError_t e = hipMalloc(&slot[0], bytes);
    if (e == hipSuccess) e = hipMalloc(&slot[1], bytes);
    if (e == hipSuccess) e = hipMemsetAsync(slot[0], fill, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(slot[1], fill, bytes, st);
    return e;
  }
  const void* current() const { return slot[cur]; }
  hipError_t reset(hipStream_t st) { return hipMemsetAsync(slot[cur], fill, bytes, st); }
  void free() {
    (void)hipFree(slot[0]);
    (void)hipFree(slot[1]);
    slot[0] = slot[1] = nullptr;
  }
  // after the call's own launch: rows of n samples of type PT, in_stride samples apart
  template <typename PT>
  hipError_t advance(hipStream_t st, const void* in, int64_t n, int64_t in_stride, int rows, int HL) {
    if (HL == 0) return hipSuccess;
    stream_hist_kernel<PT><<<dim3((unsigned)((HL + 255) / 256), (unsigned)rows), 256, 0, st>>>(
        static_cast<const PT*>(in), static_cast<const PT*>(slot[cur]), static_cast<PT*>(slot[cur ^ 1]), n, in_stride, HL);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) cur ^= 1;
    return e;
  }
};

}  // namespace sdrint
