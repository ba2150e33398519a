// f32 accuracy from f16 matrix-core operands, shared by the MFMA kernels (rx_stage.hip: the D = 1
// FIRs; ddc.hip: the channelizer): every operand is split as v = hi + lo / 2048
// (hi = f16(v), lo = f16((v - hi) 2048): 22 significant bits) and a product is
//   sum(a_hi b_hi) + (sum(a_hi b_lo) + sum(a_lo b_hi)) / 2048
// with f32 accumulation -- three v_mfma_f32_16x16x32_f16 per K step, the lo x lo term (2^-22)
// dropped (tests/test_mma_fir.py).  Also the wave-uniform buffer descriptor both use.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

constexpr float MM_LO = 2048.f;                   // the lo parts' scale

struct MmHL { _Float16 hi, lo; };
static __device__ __forceinline__ MmHL mm_split(float v) {
  const _Float16 h = (_Float16)v;
  return MmHL{h, (_Float16)((v - (float)h) * MM_LO)};
}
// four samples at once: v_cvt_pk_f16_f32 pairs, the residuals as packed f32 ops
static __device__ __forceinline__ void mm_split4(float4 x, h4v* hi, h4v* lo) {
  const f2 a{x.x, x.y}, c{x.z, x.w};
  const h2v ha = __builtin_convertvector(a, h2v), hc = __builtin_convertvector(c, h2v);
  const f2 ra = (a - __builtin_convertvector(ha, f2)) * MM_LO, rc = (c - __builtin_convertvector(hc, f2)) * MM_LO;
  const h2v la = __builtin_convertvector(ra, h2v), lc = __builtin_convertvector(rc, h2v);
  *hi = h4v{ha.x, ha.y, hc.x, hc.y};
  *lo = h4v{la.x, la.y, lc.x, lc.y};
}

// The A operand of a GEMM whose rows are fixed at create time (ddc.hip, pfb.hip), pre-split in
// fragment order.  A32: [16 NT][32 KS] f32 rows -> afrag [NT KS][hi, lo][64 lanes][8] (lane l of
// step q = t KS + st: A[16 t + (l & 15)][32 st + 8 (l >> 4) + e]).  A template, so that only the
// translation units that launch it emit it.
template <typename T = float>
__global__ void mm_prep_kernel(const T* A32, _Float16* afrag, int NT, int KS) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NT * KS * 64) return;
  const int q = i >> 6, l = i & 63, t = q / KS, st = q - t * KS;
  const T* row = A32 + (size_t)(16 * t + (l & 15)) * (32 * KS) + 32 * st + 8 * (l >> 4);
  _Float16* hi = afrag + ((size_t)q * 2 + 0) * 512 + 8 * l;
  _Float16* lo = afrag + ((size_t)q * 2 + 1) * 512 + 8 * l;
  for (int e = 0; e < 8; ++e) {
    const MmHL p = mm_split(row[e]);
    hi[e] = p.hi;
    lo[e] = p.lo;
  }
}
template <typename T>
hipError_t mm_prep(const T* A32, _Float16* afrag, int NT, int KS, hipStream_t st) {
  mm_prep_kernel<<<(NT * KS * 64 + 255) / 256, 256, 0, st>>>(A32, afrag, NT, KS);
  return hipGetLastError();
}

// A buffer descriptor over bytes [p, p + bytes) from wave-uniform values (readfirstlane: the
// compiler cannot prove a wave-id-derived address uniform and would wrap every access in a
// waterfall loop).  Raw buffer accesses outside it read 0 / are dropped by the hardware.
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t mm_rsrc(const void* p, int64_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)bytes);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uintptr_t)hi << 32) | lo), 0, nb, 0x00020000);
}
