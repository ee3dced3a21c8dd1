// tdoa_prep.h -- the integer front end of one packed int16 sample pair, one
// definition for every engine (tdoa_device.h: DIRECT and the fused GCC-PHAT
// kernels; tdoa_phat_lds.h: the LDS GCC-PHAT kernels).  Internal linkage per TU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// rolling_buffer.c:65-66, buffer.c:16, buffer.c:8-9 for one sample
__device__ __forceinline__ uint32_t prep_sample(uint32_t x16, uint32_t off16, int32_t w)
{
    const uint32_t y = (x16 - off16) & 0xFFFFu;                    // (int16)(x - off)
    const int32_t z = (int32_t)(int16_t)(uint16_t)((y << 8) & 0xFFFFu);  // x <<= 8
    const int32_t t = z * w;                                         // (int32)x * W[i]
    return (uint32_t)(t >> 15) & 0xFFFFu;                            // (int16)(tmp >> 15)
}

__device__ __forceinline__ uint32_t prep_word(uint32_t v, uint32_t off16, uint32_t wv)
{
    const int32_t w0 = (int32_t)(int16_t)(wv & 0xFFFFu);
    const int32_t w1 = (int32_t)(int16_t)(wv >> 16);
    return prep_sample(v & 0xFFFFu, off16, w0) | (prep_sample(v >> 16, off16, w1) << 16);
}

// TDOA_SAMPLES_PCM16 (include/tdoa.h) for one sample: y = x - off without the
// wrap, s = (y W) >> 15 as an arithmetic shift (floor).  |y| <= 65535 and
// 0 <= W <= 32767 fit 24 bits and |y W| < 2^31: one v_mul_i32_i24
__device__ __forceinline__ int32_t pcm16_sample(int32_t x, int32_t off, int32_t w)
{
    return __mul24(x - off, w) >> 15;
}

__device__ __forceinline__ int sum_word(uint32_t v)
{
    return (int)(int16_t)(v & 0xFFFFu) + (int)(int16_t)(v >> 16);
}

}  // namespace
