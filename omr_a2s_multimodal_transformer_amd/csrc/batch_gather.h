// What omr_gather_ragged_batch (batch_gather.hip) and omr_gather_augmented_batch (batch_augment.hip) share: the store's conversion and
// the pad value in the output type.  One definition, so the identity augmentation writes the plain gather's bits.
#pragma once
#include "omr_common.h"

__device__ __forceinline__ float gather_conv(unsigned char v) { return __fdiv_rn((float)v, 255.0f); }
__device__ __forceinline__ float gather_conv(float v) { return v; }
// The pad value in the output type.  A NaN pad in bf16 is written as 0xFFFF, the pattern torch's host fp32 -> bf16 conversion writes for
// every NaN, so that a batch equals the host collate followed by .to(bfloat16) to the bit with a NaN pad as well (a poison value for
// debugging; what the hardware conversion makes of a NaN is another quiet NaN).  fp32 keeps the caller's bits.
template <typename T> __device__ __forceinline__ T gather_pad(float v);
template <> __device__ __forceinline__ float gather_pad<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 gather_pad<bf16>(float v) {
    return v != v ? __builtin_bit_cast(bf16, (unsigned short)0xFFFF) : from_f32<bf16>(v);
}
