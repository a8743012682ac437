// Internal definitions shared by the HIP backend, the graph builder and the runners.
// Block formats follow ggml's (Q4_K: ggml-common.h block_q4_K, 144 B / 256 weights;
// Q8_0: block_q8_0, 34 B / 32 weights; Q5_0: block_q5_0, 22 B / 32 weights;
// Q4_0: block_q4_0, 18 B / 32 weights; Q6_K: block_q6_K, 210 B / 256 weights) so that weight bytes produced by TTS.cpp's loader
// (/root/reference/src/models/loaders.cpp:79-88) are consumed unchanged.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tts_hip.h"

#ifdef __HIPCC__
#define TTS_HD __host__ __device__ __forceinline__
#else
#define TTS_HD inline
#endif

namespace tts {

constexpr int QK_K = 256;
constexpr int QK8_0 = 32;
constexpr int QK5_0 = 32;
constexpr int QK4_0 = 32;

struct block_q4_K {
    uint16_t d;
    uint16_t dmin;
    uint8_t scales[12];
    uint8_t qs[QK_K / 2];
};
static_assert(sizeof(block_q4_K) == 144, "q4_K block");

struct block_q8_0 {
    uint16_t d;
    int8_t qs[QK8_0];
};
static_assert(sizeof(block_q8_0) == 34, "q8_0 block");

// weight j (j < 16) = d * (((qs[j] & 15) | (bit j of qh) << 4) - 16), weight j + 16 the same from
// qs[j] >> 4 and bit j + 16: a Q8_0 block of the same d whose quants lie in [-16, 15]
struct block_q5_0 {
    uint16_t d;
    uint8_t qh[4];
    uint8_t qs[QK5_0 / 2];
};
static_assert(sizeof(block_q5_0) == 22, "q5_0 block");

// weight j (j < 16) = d * ((qs[j] & 15) - 8), weight j + 16 = d * ((qs[j] >> 4) - 8).  Its dot with a Q8_0
// activation block is ((float)sumi * d_w) * d_x (ggml_vec_dot_q4_0_q8_0), not the Q8_0 / Q5_0 association
struct block_q4_0 {
    uint16_t d;
    uint8_t qs[QK4_0 / 2];
};
static_assert(sizeof(block_q4_0) == 18, "q4_0 block");

// weight e = 128 h + 32 g + l (h = 0, 1; g = 0 .. 3; l = 0 .. 31) = d * scales[e / 16] * (v - 32) with the 6-bit
// v = nibble (g >> 1) of ql[64 h + 32 (g & 1) + l] | (bits 2 g, 2 g + 1 of qh[32 h + l]) << 4.  210 = 2 mod 4: rows of
// an odd number of blocks leave every other row 2-byte aligned only
struct block_q6_K {
    uint8_t ql[QK_K / 2];
    uint8_t qh[QK_K / 4];
    int8_t scales[QK_K / 16];
    uint16_t d;
};
static_assert(sizeof(block_q6_K) == 210, "q6_K block");

// the K-quants, whose products quantize src1 to Q8_K
TTS_HD bool wtype_q8k_act(int t) { return t == TTS_TYPE_Q4_K || t == TTS_TYPE_Q6_K; }

// the activation type a weight type's products quantize src1 to (ggml's vec_dot_type): Q4_0, Q5_0 and Q8_0
// all take Q8_0
TTS_HD bool wtype_q80_act(int t) { return t == TTS_TYPE_Q8_0 || t == TTS_TYPE_Q5_0 || t == TTS_TYPE_Q4_0; }
// those three in a fixed order: the index of a format's option record (tts_hip_backend::b32)
TTS_HD int b32_index(int t) { return t == TTS_TYPE_Q8_0 ? 0 : t == TTS_TYPE_Q5_0 ? 1 : 2; }

// Host fp16 conversion: same bit-exact algorithm as ggml_compute_fp{16,32}_to_fp{32,16}.
inline float fp16_to_fp32_host(uint16_t h) {
    const uint32_t w = (uint32_t)h << 16;
    const uint32_t sign = w & 0x80000000u;
    const uint32_t two_w = w + w;
    uint32_t nb = (two_w >> 4) + (0xE0u << 23);
    float normalized;
    memcpy(&normalized, &nb, 4);
    normalized *= 0x1.0p-112f;
    uint32_t db = (two_w >> 17) | (126u << 23);
    float denorm;
    memcpy(&denorm, &db, 4);
    denorm -= 0.5f;
    uint32_t rb;
    if (two_w < (1u << 27)) memcpy(&rb, &denorm, 4);
    else memcpy(&rb, &normalized, 4);
    rb |= sign;
    float r;
    memcpy(&r, &rb, 4);
    return r;
}

inline uint16_t fp32_to_fp16_host(float f) {
    float base = (__builtin_fabsf(f) * 0x1.0p+112f) * 0x1.0p-110f;
    uint32_t w;
    memcpy(&w, &f, 4);
    const uint32_t shl1_w = w + w;
    const uint32_t sign = w & 0x80000000u;
    uint32_t bias = shl1_w & 0xFF000000u;
    if (bias < 0x71000000u) bias = 0x71000000u;
    uint32_t bb = (bias >> 1) + 0x07800000u;
    float bf;
    memcpy(&bf, &bb, 4);
    base = bf + base;
    uint32_t bits;
    memcpy(&bits, &base, 4);
    const uint32_t exp_bits = (bits >> 13) & 0x00007C00u;
    const uint32_t mantissa_bits = bits & 0x00000FFFu;
    const uint32_t nonsign = exp_bits + mantissa_bits;
    return (uint16_t)((sign >> 16) | (shl1_w > 0xFF000000u ? 0x7E00u : nonsign));
}

}  // namespace tts
