// fp8_widen.h — 8 OCP e4m3 bytes -> 8 T (fp16 / bf16), in byte order: v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1, two
// elements per instruction.  Exact for every finite e4m3 value; NaN bytes stay NaN.  The one definition for the FP8
// weight-streaming kernels (wstream_block_fp8.inc) and dequant_fp8_block_kernel.
#pragma once
#include "hx_common.h"

namespace hx {

template <typename T> struct Fp8Widen;
template <> struct Fp8Widen<BF16> {
  template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  }
};
template <> struct Fp8Widen<F16> {
  template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
  }
};
template <typename T>
__device__ __forceinline__ u16x8 widen(u32x2 q) {
  const u32x4 o = {Fp8Widen<T>::template pk<false>(q[0]), Fp8Widen<T>::template pk<true>(q[0]),
                   Fp8Widen<T>::template pk<false>(q[1]), Fp8Widen<T>::template pk<true>(q[1])};
  return __builtin_bit_cast(u16x8, o);
}

}  // namespace hx
