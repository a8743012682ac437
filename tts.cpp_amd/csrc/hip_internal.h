// Internal HIP backend state and kernel launchers (not part of the C-ABI).
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <array>
#include <atomic>
#include <deque>
#include <mutex>
#include <unordered_map>
#include <tuple>
#include <vector>

#include "common.h"

#define TTS_HIP_CHECK(expr)                                                                          \
    do {                                                                                             \
        hipError_t err_ = (expr);                                                                    \
        if (err_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: HIP error %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(err_)); \
            abort();                                                                                 \
        }                                                                                            \
    } while (0)

namespace tts {

constexpr int kArgmaxRows = 4096;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short short2_t __attribute__((ext_vector_type(2)));

// Tensor view handed to kernels by value: data pointer, shape and byte strides (ggml ne/nb).
struct TD {
    char * data;
    int64_t ne[4];
    int64_t nb[4];
    int32_t type;
    int32_t pad;  // tts_tensor.flags (TTS_FLAG_REPACKED matters to kernels)
};

// Transcendentals pinned to the correctly rounded f32 value (evaluated in f64), the same policy
// as the oracle (oracle/ggml_ref.c ref_expf ...), so GPU and CPU agree bit-for-bit except when
// the exact value lies within ~2^-52 of an f32 rounding midpoint.
#ifdef __HIPCC__
__device__ __forceinline__ float cr_expf(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float cr_sinf(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float cr_cosf(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float cr_tanhf(float x) { return (float)tanh((double)x); }
// IEEE-exact f32 sqrt / division (gfx950's f32 sqrt lowering is not correctly rounded); the f64
// result rounded to f32 is the correctly rounded f32 value (53 >= 2*24 + 2).
__device__ __forceinline__ float cr_sqrtf(float x) { return (float)__dsqrt_rn((double)x); }
__device__ __forceinline__ float cr_divf(float a, float b) { return (float)__ddiv_rn((double)a, (double)b); }
// ggml's silu (ggml_vec_silu_f32 / ggml_silu_f32: x / (1 + exp(-x))), correctly rounded pieces
__device__ __forceinline__ float dev_silu(float x) { return cr_divf(x, __fadd_rn(1.0f, cr_expf(-x))); }

// Compiler memory barrier placed after a batch of independent loads: keeps the compiler from
// sinking a load into the (guarded) block that uses it, which would serialize the batch into one
// full memory round trip per load.  Emits no instruction.
#define TTS_PIN_LOADS() asm volatile("" ::: "memory")

// Cache policy of the two big decode streams (build-time, for the MALL-residency study):
// TTS_WLOAD = quantized weight rows (default non-temporal), TTS_KVLOAD = K/V cache rows of decode
// attention (default plain).
// Loads through an explicitly global (address space 1) pointer: a pointer the compiler cannot trace
// to a kernel argument would otherwise be a FLAT load, and flat loads complete out of order, so every
// later wait on any vector load becomes vmcnt(0) -- a wait for the weight stream in the prologue.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T * gptr(const T * p) {
    return (const __attribute__((address_space(1))) T *)p;
}
#ifdef TTS_W_PLAIN
#define TTS_WLOAD(p) (*gptr(p))
#else
#define TTS_WLOAD(p) __builtin_nontemporal_load(gptr(p))
#endif
__device__ __forceinline__ float4 kv_ld4(const float4 * p) {
#ifdef TTS_KV_NT
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = __builtin_nontemporal_load((const f4v *)p);
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
#define TTS_KVLOAD(p) kv_ld4(p)

// ---- wave64 cross-lane helpers on DPP + readlane (no LDS crossbar, no lgkmcnt waits) ----
// DPP controls (gfx9): quad_perm [1,0,3,2] = lane^1, [2,3,0,1] = lane^2, row_half_mirror (i <-> 7-i
// in each 8), row_mirror (i <-> 15-i in each 16), row_shl:n (lane i reads lane i+n in its row).
enum { DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_ROW_SHL0 = 0x100 };
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(dpp_i32<CTRL>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i32<CTRL>((int)(b & 0xFFFFFFFF)), hi = dpp_i32<CTRL>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFF), lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// wave-uniform sum; every lane of a 16-lane row holds the same partial (a+b == b+a), the four row
// partials are added in row order
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_f64<DPP_XOR1>(v);
    v += dpp_f64<DPP_XOR2>(v);
    v += dpp_f64<DPP_HALF_MIRROR>(v);
    v += dpp_f64<DPP_MIRROR>(v);
    return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}
// wave-uniform max of non-negative floats (compared as their bit patterns)
__device__ __forceinline__ float wave_max_nonneg(float x) {
    unsigned v = __float_as_uint(x);
    v = max(v, (unsigned)dpp_i32<DPP_XOR1>((int)v));
    v = max(v, (unsigned)dpp_i32<DPP_XOR2>((int)v));
    v = max(v, (unsigned)dpp_i32<DPP_HALF_MIRROR>((int)v));
    v = max(v, (unsigned)dpp_i32<DPP_MIRROR>((int)v));
    const unsigned a = max((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16));
    const unsigned b = max((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48));
    return __uint_as_float(max(a, b));
}
// sum over the 8 lanes of an octet, result in all 8 lanes
__device__ __forceinline__ int octet_sum_i32(int v) {
    v += dpp_i32<DPP_XOR1>(v);
    v += dpp_i32<DPP_XOR2>(v);
    v += dpp_i32<DPP_HALF_MIRROR>(v);
    return v;
}

// ---- Q8_0 / Q5_0 / Q4_0 block arithmetic shared by the GEMVs (k_gemv.hip) and the quantized LSTM step (k_fused.hip) ----
__device__ __forceinline__ float dev_fp16_to_fp32(uint16_t h) {
    return __half2float(__ushort_as_half(h));
}
// quantize_row_q8_0_ref, one element per lane, the 32 lanes of a half wave holding one block: d = amax/127,
// id = d ? 1/d : 0, q = roundf(v*id).  Returns q; d_out is the block's d rounded to fp16 (what the dot uses).
__device__ __forceinline__ int8_t q80_quant_elem(float v, float & d_out) {
    float a = fabsf(v);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) a = fmaxf(a, __shfl_xor(a, off));
    const float d = cr_divf(a, 127.f);
    const float id = d != 0.f ? cr_divf(1.f, d) : 0.f;
    d_out = __half2float(__float2half_rn(d));
    return (int8_t)roundf(__fmul_rn(v, id));
}
// Q5_0: four weights per dword: nibbles (qs & 0x0F0F0F0F, or qs >> 4 for weights 16 .. 31) give q's low four
// bits per byte; q - 16 in two's complement is that nibble with 0xF0 on top where q's fifth bit is
// clear.  Four bits of ~qh go to the four bytes' bit 0 by one multiply (b * 0x00204081 puts bit k at
// 8 k, the four shifted copies never overlapping), and * 0xF0 widens each to the byte's high nibble.
__device__ __forceinline__ uint32_t q50_himask(uint32_t nqh, int s) {  // nqh = ~qh; weights s .. s + 3
    return ((((nqh >> s) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xF0u;
}
// Q4_0: four weights per dword: a byte's nibble n in 0 .. 15 becomes the int8 n - 8 in four operations on the
// dword (five for the high nibbles' shift): t = n ^ 8 is n - 8 for n >= 8 and n + 8 (bit 3 set) for n < 8, where
// n - 8 is t with 0xF0 on top; (t & 0x08) * 0x1E = 0xF0 stays inside its byte.
__device__ __forceinline__ uint32_t q40_s8(uint32_t nib) {  // nib: four bytes 0 .. 15
    const uint32_t t = nib ^ 0x08080808u;
    return t | ((t & 0x08080808u) * 0x1Eu);
}
// exact int32 dot of a block's 32 int8 weights with 32 int8 activations (x0 = elements 0 .. 15, x1 = 16 .. 31)
__device__ __forceinline__ int q50_dot(const int (&wv)[8], const int4 x0, const int4 x1) {
    int s = __builtin_amdgcn_sdot4(wv[0], x0.x, 0, false);
    s = __builtin_amdgcn_sdot4(wv[1], x0.y, s, false);
    s = __builtin_amdgcn_sdot4(wv[2], x0.z, s, false);
    s = __builtin_amdgcn_sdot4(wv[3], x0.w, s, false);
    s = __builtin_amdgcn_sdot4(wv[4], x1.x, s, false);
    s = __builtin_amdgcn_sdot4(wv[5], x1.y, s, false);
    s = __builtin_amdgcn_sdot4(wv[6], x1.z, s, false);
    s = __builtin_amdgcn_sdot4(wv[7], x1.w, s, false);
    return s;
}
// The three 32-weight formats whose activation is Q8_0, as traits of the shared kernel bodies (k_gemv_b32,
// k_gemv_b32s, k_gemm_b32, k_gemm_b32s in k_gemv.hip; k_lstm_step_q in k_fused.hip).  A block is {f16 d;
// payload}, BYTES in all at a 2-B aligned address, the payload ND = (BYTES - 2) / 4 dwords.  Each trait gives
//   unpack(q, wv)   the payload dwords -> the block's 32 int8 weights, wv[i] = weights 4 i .. 4 i + 3
//   QOFF, sel(kq), nsh(kq), octet(q0, q1, blk, kq, nsh)
//                   the MFMA A operand of lane group kq, weights 8 kq .. 8 kq + 7 paired with the activation's same
//                   octet: q0, q1 are the eight payload bytes at blk + QOFF + 8 * sel(kq) (b32_octet / b32_octet_lds
//                   fetch them); nsh(kq), the nibble shift of the two nibble formats, is taken once at a kernel's top
//   term(sumi, dw, dx)
//                   the block's f32 term with ggml_vec_dot_<format>_q8_0's association and roundings
struct BlkQ8_0 {  // {d; int8 qs[32]}
    static constexpr int TYPE = TTS_TYPE_Q8_0, BYTES = 34, ND = 8;
    static __device__ __forceinline__ void unpack(const uint32_t (&q)[ND], int (&wv)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = (int)q[i];
    }
    static constexpr int QOFF = 2;
    static __device__ __forceinline__ int sel(int kq) { return kq; }
    static __device__ __forceinline__ int nsh(int) { return 0; }
    static __device__ __forceinline__ long octet(uint32_t q0, uint32_t q1, const uint8_t *, int, int) {
        return (long)(((uint64_t)q1 << 32) | q0);
    }
    static __device__ __forceinline__ float term(int sumi, float dw, float dx) {
        return __fmul_rn((float)sumi, __fmul_rn(dw, dx));
    }
};
struct BlkQ5_0 {  // {d; u8 qh[4]; u8 qs[16]}: q[0] = qh, q[1 .. 4] = qs; weights q - 16 in [-16, 15]
    static constexpr int TYPE = TTS_TYPE_Q5_0, BYTES = 22, ND = 5;
    // i < 4: low nibbles, i >= 4: high nibbles
    static __device__ __forceinline__ void unpack(const uint32_t (&q)[ND], int (&wv)[8]) {
        const uint32_t nqh = ~q[0];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wv[i] = (int)((q[1 + i] & 0x0F0F0F0Fu) | q50_himask(nqh, 4 * i));
            wv[4 + i] = (int)(((q[1 + i] >> 4) & 0x0F0F0F0Fu) | q50_himask(nqh, 16 + 4 * i));
        }
    }
    // groups 0, 1 the low nibbles of qs[0..7] / qs[8..15], groups 2, 3 their high nibbles, each with byte kq of qh
    static constexpr int QOFF = 6;
    static __device__ __forceinline__ int sel(int kq) { return kq & 1; }
    static __device__ __forceinline__ int nsh(int kq) { return (kq >> 1) * 4; }  // high nibbles for weights 16 .. 31
    static __device__ __forceinline__ long octet(uint32_t q0, uint32_t q1, const uint8_t * blk, int kq, int nsh) {
        const uint32_t nqh = ~(uint32_t)blk[2 + kq];
        const uint32_t lo = ((q0 >> nsh) & 0x0F0F0F0Fu) | q50_himask(nqh, 0);
        const uint32_t hi = ((q1 >> nsh) & 0x0F0F0F0Fu) | q50_himask(nqh, 4);
        return (long)(((uint64_t)hi << 32) | lo);
    }
    static __device__ __forceinline__ float term(int sumi, float dw, float dx) {
        return __fmul_rn((float)sumi, __fmul_rn(dw, dx));
    }
};
struct BlkQ4_0 {  // {d; u8 qs[16]}: q[0 .. 3] = qs; weights q - 8 in [-8, 7]
    static constexpr int TYPE = TTS_TYPE_Q4_0, BYTES = 18, ND = 4;
    // i < 4: low nibbles, i >= 4: high nibbles
    static __device__ __forceinline__ void unpack(const uint32_t (&q)[ND], int (&wv)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wv[i] = (int)q40_s8(q[i] & 0x0F0F0F0Fu);
            wv[4 + i] = (int)q40_s8((q[i] >> 4) & 0x0F0F0F0Fu);
        }
    }
    // groups 0, 1 the low nibbles of qs[0..7] / qs[8..15], groups 2, 3 their high nibbles, each made q - 8 by q40_s8
    static constexpr int QOFF = 2;
    static __device__ __forceinline__ int sel(int kq) { return kq & 1; }
    static __device__ __forceinline__ int nsh(int kq) { return (kq >> 1) * 4; }  // high nibbles for weights 16 .. 31
    static __device__ __forceinline__ long octet(uint32_t q0, uint32_t q1, const uint8_t *, int, int nsh) {
        const uint32_t lo = q40_s8((q0 >> nsh) & 0x0F0F0F0Fu);
        const uint32_t hi = q40_s8((q1 >> nsh) & 0x0F0F0F0Fu);
        return (long)(((uint64_t)hi << 32) | lo);
    }
    // ((float)sumi * d_w) * d_x, each product rounded -- not the other two formats' sumi * (d_w * d_x), which
    // differs in the last bit for about one term in ten
    static __device__ __forceinline__ float term(int sumi, float dw, float dx) {
        return __fmul_rn(__fmul_rn((float)sumi, dw), dx);
    }
};
// The forms in which the kernel bodies meet a block, the same for every format F.
// A block at any 2-B aligned address `bp` (P: a pointer to its 16-bit words, global or generic): BYTES / 2 16-bit
// loads -> the fp16 d and the payload dwords (then F::unpack)
template <class F, class P>
__device__ __forceinline__ void b32_load(P bp, uint16_t & d, uint32_t (&q)[F::ND]) {
    d = bp[0];
#pragma unroll
    for (int k = 0; k < F::ND; ++k) q[k] = (uint32_t)bp[1 + 2 * k] | ((uint32_t)bp[2 + 2 * k] << 16);
}
// The block pair (2k, 2k + 1) as its BYTES / 2 dwords from a 4-B aligned address: d0 | payload 0 (the funnel-shifted
// dwords) | d1, payload 1 (whole dwords)
template <class F>
__device__ __forceinline__ void b32_pair(const uint32_t (&w)[F::BYTES / 2], float & d0, float & d1, int (&q0)[8], int (&q1)[8]) {
    d0 = dev_fp16_to_fp32((uint16_t)(w[0] & 0xFFFFu));
    d1 = dev_fp16_to_fp32((uint16_t)(w[F::ND] >> 16));
    uint32_t p0[F::ND], p1[F::ND];
#pragma unroll
    for (int i = 0; i < F::ND; ++i) {
        p0[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], 16);
        p1[i] = w[F::ND + 1 + i];
    }
    F::unpack(p0, q0);
    F::unpack(p1, q1);
}
// Lane group kq's MFMA A operand from a 2-B aligned block in global memory: its eight payload bytes as four 16-bit loads
template <class F>
__device__ __forceinline__ long b32_octet(const uint8_t * blk, int kq, int nsh) {
    const uint16_t * q = (const uint16_t *)(blk + F::QOFF + 8 * F::sel(kq));
    const uint32_t q0 = (uint32_t)q[0] | ((uint32_t)q[1] << 16), q1 = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
    return F::octet(q0, q1, blk, kq, nsh);
}
// The same from a staged LDS image (`base` 4-B aligned, the block `boff` bytes into it): the eight bytes start 0 or
// 2 B off a dword, so three dwords and two funnel shifts
template <class F>
__device__ __forceinline__ long b32_octet_lds(const char * base, int boff, int kq, int nsh) {
    const int off = boff + F::QOFF + 8 * F::sel(kq);
    const uint32_t * p = (const uint32_t *)(base + (off & ~3));
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    const uint32_t sh = (off & 3) * 8;
    const uint32_t q0 = __builtin_amdgcn_alignbit(d1, d0, sh), q1 = __builtin_amdgcn_alignbit(d2, d1, sh);
    return F::octet(q0, q1, (const uint8_t *)(base + boff), kq, nsh);
}
#endif

inline TD make_td(const tts_tensor * t) {
    TD d;
    d.data = (char *)t->data;
    for (int i = 0; i < 4; ++i) {
        d.ne[i] = t->ne[i];
        d.nb[i] = (int64_t)t->nb[i];
    }
    d.type = t->type;
    d.pad = t->flags;
    return d;
}
#ifdef __HIPCC__
// element access through a ggml view (F32 / F16 / I32), as the oracle's load_elem / store_elem
static __device__ __forceinline__ void unravel(int64_t k, const int64_t * ne, int64_t & i0, int64_t & i1, int64_t & i2, int64_t & i3) {
    i0 = k % ne[0];
    k /= ne[0];
    i1 = k % ne[1];
    k /= ne[1];
    i2 = k % ne[2];
    i3 = k / ne[2];
}

static __device__ __forceinline__ char * td_ptr(const TD & t, int64_t i0, int64_t i1, int64_t i2, int64_t i3) {
    return t.data + i0 * t.nb[0] + i1 * t.nb[1] + i2 * t.nb[2] + i3 * t.nb[3];
}
static __device__ __forceinline__ float td_load_at(const TD & t, const char * p) {
    if (t.type == TTS_TYPE_F16) return __half2float(*(const __half *)p);
    if (t.type == TTS_TYPE_I32) return (float)*(const int32_t *)p;
    return *(const float *)p;
}
static __device__ __forceinline__ float td_load(const TD & t, int64_t i0, int64_t i1, int64_t i2, int64_t i3) {
    return td_load_at(t, td_ptr(t, i0, i1, i2, i3));
}
static __device__ __forceinline__ void td_store(const TD & t, int64_t i0, int64_t i1, int64_t i2, int64_t i3, float v) {
    char * p = t.data + i0 * t.nb[0] + i1 * t.nb[1] + i2 * t.nb[2] + i3 * t.nb[3];
    if (t.type == TTS_TYPE_F16) *(__half *)p = __float2half_rn(v);
    else if (t.type == TTS_TYPE_I32) *(int32_t *)p = (int32_t)v;
    else *(float *)p = v;
}
#endif

// Device scratch for quantized activations (Q8_K / Q8_0 / F16 copies of a mul_mat src1).
struct ActQuant {
    const void * src = nullptr;  // src1 data pointer the cache entry was built from
    int64_t K = 0, M = 0;
    int vtype = -1;
    int64_t graph_epoch = -1;
    int8_t * qs = nullptr;      // [M][K] int8 (Q8_K / Q8_0) or fp16 [M][K] (F16)
    float * d = nullptr;        // [M][K/256] (Q8_K) or [M][K/32] (Q8_0: fp16-rounded d as float)
    int32_t * bsums = nullptr;  // [M][K/256][8] per-32 sums (Q8_K)
};

// One GEMV launch: up to GEMV_MAX_MATS weight matrices of identical type/shape sharing one
// activation (q/k/v; the 9 codebook heads), y(row n, column m) = Y[i][m*ycs + n*yrs], with an
// optional fused epilogue (GELU table, or + residual(row n, column m) = res[m*rcs + n]).
// EPI_SWIGLU (matrix-core Q4_K kernel only, nmat == 2: gate, up): Y[0] = silu(gate) * up, the
// UNARY SILU and MUL of the SwiGLU MLP (Orpheus model.cpp:296-300); gate / up are never stored.
// EPI_SILU_MUL (Q8_0 / Q5_0 kernels): y = silu(res) * product -- the up product's epilogue reading the gate
// product stored by the previous launch (Dia's MLP: MUL(SILU(gate x), up x)), as UNARY SILU then MUL round.
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_ADD = 2, EPI_SWIGLU = 3, EPI_SILU_MUL = 4 };
constexpr int GEMV_MAX_MATS = 16;
struct GemvJob {
    int wtype = 0;
    int nmat = 1;
    const uint8_t * W[GEMV_MAX_MATS] = {};
    float * Y[GEMV_MAX_MATS] = {};
    int64_t w_row_bytes = 0, K = 0, N = 0, M = 0;
    int64_t ycs[GEMV_MAX_MATS] = {}, yrs[GEMV_MAX_MATS] = {};  // per-matrix output strides
    const float * res = nullptr;
    int64_t rcs = 0;
    int epi = EPI_NONE;
    const uint16_t * gelu = nullptr;
    const float * x = nullptr;  // f32 activation (F32 weights; Q4_K quantizes it in-kernel)
    int64_t xcs = 0;
    ActQuant aq;
    // Q4_K prologue: PRO_QUANT = quantize x to Q8_K in LDS; PRO_LN = first x <- norm(x)*w (+b)
    // (NORM/RMS_NORM -> MUL -> ADD, parler_build_layer_norm), written to lnout by workgroup 0.
    int pro = 0;
    int tiled = 0;  // W in the 4-row tile layout (TTS_FLAG_TILED): k_gemv_q4K_mf
    // matrices of different row counts (tile-layout kernels only): matrix m holds flat rows
    // roff[m] .. roff[m + 1] - 1 (each a multiple of 16); otherwise N rows each
    int hetero = 0;
    int64_t roff[GEMV_MAX_MATS + 1] = {};
    // matrix rep_mat (at most one per launch; -1 = none) is written straight into the GQA copies of a
    // KV cache: row n -> (n / yrg) * yrgs + (n % yrg) * yrs, stored at +k * yrep for k < nrep.  Kept to
    // a few scalars: the job is a kernel argument re-set in every recorded step graph.
    int32_t rep_mat = -1, yrg = 0, nrep = 0;
    int64_t yrgs = 0, yrep = 0;
    int dbg = 0;    // phase study (TTS_HIP_OPT_GEMV_DEBUG): 1 = skip the row phase, 2 = skip the prologue
    const float * lnw = nullptr;
    const float * lnb = nullptr;
    float eps = 0.f;
    int rms = 0;
    float * lnout = nullptr;
    int64_t locs = 0;
    // PRO_COPY (matrix-core kernels): the Q8_K activation already in the kernel's LDS operand layout
    // ([M*nb + 1][256] f16, [M*nb + 1][16] f16 bsum halves, [M*nb + 1] f32 d; bq_bytes, a multiple of
    // 1 KiB), written by k_quant_mf
    const char * bq = nullptr;
    int64_t bq_bytes = 0;
    int64_t bq_tile = 0;  // > 0: columns in tiles of 16, tile c's operands at bq + c * bq_tile (its own slot layout)
    int32_t bq_slot = 0;  // halves per operand slot (0 = QK_K; the prefill GEMM pads slots to QK_K + 8 so a block's
                          // 16 columns sit on different LDS banks)
    unsigned long long * ts = nullptr;  // phase timestamps (scripts/gemv_phase.hip builds only)
    // ragged columns (a coalesced step's KV-cache stores, coalesce.hip): for the matrices in yoff_mats,
    // column m of matrix mat is stored at Y[mat] + m * ycs + yoff[mat * yoff_ld + m] (floats) -- each
    // member's cache row at its own position
    const int64_t * yoff = nullptr;
    int32_t yoff_mats = 0, yoff_ld = 0;
    int32_t xcd_cols = 0;  // many-column K-relay GEMM: a row tile's column tiles on one XCD (TTS_HIP_OPT_GEMM_KR_XCD)
    int32_t kr_tail = 0;   // K-relay kernel: KR_TAIL_* bits (TTS_HIP_OPT_GEMV_KR_TAIL, set by its launcher)
};
// KR_TAIL_RES: an EPI_ADD residual is requested at kernel entry; KR_TAIL_FOLD: K = 1024 folds the chain after one
// barrier; KR_TAIL_BESIDE: the fold's terms lie beside the operand tile in LDS instead of over it
enum { KR_TAIL_RES = 1, KR_TAIL_FOLD = 2, KR_TAIL_BESIDE = 4 };
constexpr int KR_FOLD_BYTES = 4 * 4 * (2 * 64 * 16 + 64 * 4);  // 4 blocks x 4 rows x (two float4 + one float per lane)
__host__ __device__ inline int64_t job_roff(const GemvJob & j, int m) { return j.hetero ? j.roff[m] : (int64_t)m * j.N; }
__host__ __device__ inline int64_t job_rows(const GemvJob & j) { return job_roff(j, j.nmat); }
// In-kernel phase timestamps (s_memrealtime, 100 MHz) per wave, compiled in only by the
// micro-benchmark build (-DTTS_PHASE_TS): ts[(wg * waves + wave) * 8 + k].
#ifdef TTS_PHASE_TS
#define TTS_TS(job, k)                                                                                            \
    do {                                                                                                          \
        if ((job).ts && (threadIdx.x & 63) == 0)                                                                  \
            (job).ts[((((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + \
                      (threadIdx.x >> 6)) * 8 +                                                                   \
                     (k)] = __builtin_amdgcn_s_memrealtime();                                                     \
    } while (0)
#else
#define TTS_TS(job, k) \
    do {               \
    } while (0)
#endif
enum { PRO_QUANT = 1, PRO_LN = 2, PRO_COPY = 3 };  // PRO_COPY: operands pre-quantized at GemvJob::bq
// Cross-attention over a short context folded into the Q4_K GEMV that produces its query
// (k_gemv_q4K_xattn): K view [hd, P, H, B], V view [P, hd, H, B] (f32), out [hd, H, 1, B].
struct XAttnArgs {
    TD k, v;
    const float * mask = nullptr;  // [P] row 0 (n = 1), or null
    float scale = 1.f;
    float * out = nullptr;
    float * out2 = nullptr;        // optional private copy (the next GEMV's input, be->shadow), [hd, H, B] contiguous
    int P = 0, H = 0, B = 0;
    int64_t obs = 0;               // floats between sequences of out (0: H * hd, contiguous)
    int64_t mbs = 0;               // floats between sequences' masks (0: one mask for all)
    // ragged sequences (coalesce.hip): per-sequence K / V byte offsets, mask offsets (floats), key counts
    const int64_t * koff = nullptr;
    const int64_t * voff = nullptr;
    const int64_t * moff = nullptr;
    const int * pseq = nullptr;
};

// A coalesced decode step (coalesce.hip): N one-prompt decode graphs of different backends (TTS.cpp's
// server runs one runner per worker, examples/server/server.cpp:316-321) that differ at most in their KV
// lengths run as ONE plan of member 0's graph with M = N columns / B = N sequences.
//  - Intermediates (every tensor the graph allocator placed, i.e. not a leaf or a view of one) are
//    computed in executor-owned memory laid out as member 0's compute buffer, member k at win + k *
//    stride: one uniform column / sequence stride, which the GEMV, attention, norm and embedding
//    kernels take.  The graph's output node is copied to each member's own tensor afterwards.
//  - Member-owned operands (KV-cache views read by attention and written by the K / V store
//    epilogues, masks and token / position inputs) are each member's own tensors, found by node
//    position in its graph, and reach the kernels as per-member offset tables (ItemTab), together
//    with each member's own key count.
//  - Read-only model data (weights, norms, tables) is read through member 0's copy, checked equal to
//    each member's own copy on the device first.
constexpr int EMBED_MAX_TERMS = 16;
struct BatchCls {
    const char * b0 = nullptr;  // member 0's buffer
    size_t size = 0;
    char * win = nullptr;       // executor memory: member k's copy of the range at win + k * stride
    int64_t stride = 0;
};
// per-item tables of member-owned operands (device pointers, valid for the current coalesced plan)
struct ItemTab {
    const int64_t * yoff = nullptr;  // GEMV: [nmat][N] store offsets (floats) of the matrices in yoff_mats
    int32_t yoff_mats = 0;
    const int64_t *koff = nullptr, *voff = nullptr;  // ATTN: K / V view offsets per member (bytes)
    const int64_t * moff = nullptr;                  // ATTN: mask offsets per member (floats)
    const int * pseq = nullptr;                      // ATTN: key count per member
    int pmax = 0;
    const int64_t * ioff[EMBED_MAX_TERMS] = {};      // EMBED: index offsets per member (elements)
    // MCPY / a ROPE node: member k's destination d at dst[d] + doff[d * N + k] floats (its own cache rows, or its
    // executor copy of an intermediate); member k's rope positions at pos + poff[k] elements (its own input)
    const int64_t * doff = nullptr;
    const int64_t * poff = nullptr;
};
struct BatchCtx {
    int N = 0;
    uint64_t key = 0;  // the group: graph signature and member backends (coalesce.hip caches per key)
    std::vector<BatchCls> cls;  // sorted by b0
    std::vector<tts_tensor * const *> mnodes;  // every member's node list (member 0's first; equal lengths)
    std::vector<tts_hip_backend *> mbe;         // every member's backend (the read-back of its outputs)
    int n_nodes = 0;
    bool checked = false;       // this group's shapes and read-only operands were verified by an earlier step
    int canon = 0;              // the member whose read-only data every other member's is compared with (stable per set)
    bool ragged = false;        // (co_prepare) the members' KV lengths differ
    bool differs = false;       // refused because a member's read-only data differs (not for lack of a batched form)
    std::vector<ItemTab> tabs;  // per plan item (graph_exec.hip)
    // per ROPE node launched once over the members (a plain node, or a NODE item's stand-in): its doff / poff
    std::unordered_map<const tts_tensor *, ItemTab> ntab;
    void * comap = nullptr;     // graph_exec.hip: member 0's tensors -> graph positions (member k's counterparts)
    const BatchCls * find(const void * p) const {
        const char * c = (const char *)p;
        size_t lo = 0, hi = cls.size();
        while (lo < hi) {
            const size_t m = (lo + hi) / 2;
            if (cls[m].b0 <= c) lo = m + 1;
            else hi = m;
        }
        if (lo == 0) return nullptr;
        const BatchCls & b = cls[lo - 1];
        return c < b.b0 + b.size ? &b : nullptr;
    }
    // the executor address of member 0's intermediate p (p itself when it is not one)
    template <typename T>
    T * win(T * p) const {
        const BatchCls * b = p ? find(p) : nullptr;
        return b ? (T *)(b->win + ((const char *)p - b->b0)) : p;
    }
    int64_t stride(const void * p) const {  // bytes between members' copies (0: not an intermediate)
        const BatchCls * b = p ? find(p) : nullptr;
        return b ? b->stride : 0;
    }
    template <typename T>
    T * reloc(T * p, int k) const {  // member k's executor copy of member 0's intermediate p
        const BatchCls * b = p ? find(p) : nullptr;
        return b ? (T *)(b->win + k * b->stride + ((const char *)p - b->b0)) : p;
    }
};

}  // namespace tts

struct tts_hip_backend {
    int device = 0;
    hipStream_t stream = nullptr;
    char name[64] = {0};
    // scratch arena for activation quantization
    char * scratch = nullptr;
    size_t scratch_size = 0;
    // private second copy of an attention output, read by the GEMV that consumes it when the graph
    // allocator has placed that GEMV's output on the attention output's memory
    float * shadow = nullptr;
    size_t shadow_size = 0;
    // outputs of grouped products hoisted over nodes that still use their memory (graph_exec try_gemv)
    void * hoist = nullptr;
    size_t hoist_size = 0;
    // split decode attention: masked, scaled scores [B][n][H][P] and per-chunk maxima between the
    // scores kernel and the softmax + P.V kernel (consumed by the very next launch on the stream)
    float * attn_buf = nullptr;
    size_t attn_floats = 0;
    int attn_split_minp = 128;
    int attn_ks = 2;   // split scores: 128 * attn_ks positions per workgroup (TTS_HIP_OPT_ATTN_KS)
    int attn_pv_mp = 1;  // split P.V: every dim of a (head, query, sequence) in one workgroup (TTS_HIP_OPT_ATTN_PV_MP)
    int attn_one = 1;  // the one-launch 256-thread decode attention where k_attn_pv_mp<8, 4, 4> would run (TTS_HIP_OPT_ATTN_ONE)
    int attn_pv8 = 0;  // split P.V: 8 output dims per workgroup instead of 16 (TTS_HIP_OPT_ATTN_PV8)
    int attn_pv_uv16 = 0;  // split P.V: one 16-chunk V batch per lane for P <= 1024 (TTS_HIP_OPT_ATTN_PV16; measured equal, off)
    int attn_fused_minp = 0;  // the one-launch 1024-thread decode attention from this many keys (0 = off: measured no faster in the Parler step)
    unsigned long long * argmax_keys = nullptr;  // k_greedy_step_wide: per-row keys / arrival counts (self-clearing)
    unsigned * argmax_counts = nullptr;
    // weight_set: Q4_K matrices >= this size use the tile layout + matrix-core GEMV (0 = never)
    int64_t q4k_tile_bytes = 4 << 20;
    // TTS_HIP_OPT_GEMV_DEBUG phase-study bitmask of the matrix-core GEMV: 1 = skip the row phase,
    // 2 = skip the prologue, 4 = plain (cached) weight loads (results invalid; micro-benchmarks only)
    int gemv_dbg = 0;
    // Q4_K GEMVs in the lane layout run the unique-load kernel (k_gemv_q4_K_u) where the shape fits
    int gemv_unique = 1;
    int64_t cus = 256;  // compute units this backend's stream may use (TTS_HIP_OPT_CU_PARTITION); grids are sized to it
    int cu_total = 256;
    int bgemm_f32 = 1;  // TTS_HIP_OPT_BGEMM_F32
    int gemv_f32_wide = 1;  // TTS_HIP_OPT_GEMV_F32_WIDE
    int gemm_kr_nw = 4;     // TTS_HIP_OPT_GEMM_KR_NW: waves per tile of the many-column K-relay GEMM (4 or 8)
    // tile-layout Q4_K GEMVs of at most this many 16-row tiles (M <= 8, K <= 4096) run the K-split
    // matrix-core kernel k_gemv_q4K_ks (0 = never)
    int64_t gemv_ks_tiles = 256;
    int gemv_mf_prequant = 1;  // TTS_HIP_OPT_GEMV_PREQUANT
    int gemv_kr = 1;           // TTS_HIP_OPT_GEMV_KRELAY
    int gemv_kr_loop = 1;      // TTS_HIP_OPT_GEMV_KRELAY_LOOP
    int gemv_kr_tail = 1;      // TTS_HIP_OPT_GEMV_KR_TAIL (0 .. 4; GemvJob::kr_tail carries its KR_TAIL_* bits)
    int gemv_q80_pro = 1;      // TTS_HIP_OPT_GEMV_Q80_PRO
    // the Q8_0 / Q5_0 / Q4_0 kernels' options, one record per format at b32_index(wtype)
    struct B32Opts {
        int slab = 1;    // TTS_HIP_OPT_GEMV_Q80_SLAB / _Q50_SLAB / _Q40_SLAB
        int rw = 0;      // TTS_HIP_OPT_GEMV_Q80_RW / _Q50_RW / _Q40_RW
        int gemm = 1;    // TTS_HIP_OPT_GEMM_Q8 / _Q5 / _Q4_0
        int staged = 2;  // TTS_HIP_OPT_GEMM_Q8_STAGED / _Q5_STAGED / _Q4_0_STAGED
    };
    std::array<B32Opts, 3> b32;
    int64_t gemv_kr_ink = 0;   // TTS_HIP_OPT_GEMV_KR_INKERNEL (max K)
    int gemm_kr_walk = 0;      // TTS_HIP_OPT_GEMM_KR_WALK: row-tile walkers per column tile of a many-column GEMM
    int gemm_pf = 64;          // TTS_HIP_OPT_GEMM_PF: many-column Q4_K products of >= value columns on k_gemm_q4K_pf (0 = off)
    int gemm_pf_nw = 4;        // TTS_HIP_OPT_GEMM_PF_NW: waves per prefill-GEMM workgroup (4 or 8)
    int gemm_kr_cp = 0;        // TTS_HIP_OPT_GEMM_KR_CP: two column tiles per workgroup on parallel wave halves
    int gemm_kr_xcd = 0;       // TTS_HIP_OPT_GEMM_KR_XCD: a row tile's column tiles on one XCD (measured no gain: off)
    int gemm_kr_ct2 = 0;       // TTS_HIP_OPT_GEMM_KR_CT2: two 16-column tiles per K-relay GEMM workgroup (K <= 2048)
    int64_t gemm_kr_ink = 0;   // TTS_HIP_OPT_GEMM_KR_INKERNEL (max M of the many-column K-relay GEMM without the operand pass)
    int gemv_nw_min = 0;       // TTS_HIP_OPT_GEMV_NW_MIN: minimum waves per lane-layout Q4_K GEMV workgroup
    int gemv_mf_rsplit = 1;  // matrix-core GEMV: split a tile's residues over 2 / 4 waves when tiles are few (TTS_HIP_OPT_GEMV_RSPLIT)
    // weight_set: lane-layout Q4_K matrices of >= this size (and below q4k_tile_bytes) also keep a
    // tile-layout copy (TTS_FLAG_TILED_COPY); GEMVs of >= 8 columns read it (0 = never)
    int64_t q4k_dual_bytes = 1 << 20;
    // (the tile-layout copies and the live buffer ranges are process-wide, tiled_copy_find: a weight
    // buffer is allocated and written through one backend and read by the graphs of others -- the
    // ggml adapter's buffer type allocates through a utility backend, each ggml_backend computes on
    // its own stream)
    void * sample_cand = nullptr;  // wide-vocabulary sampling candidates (k_sample.hip)
    size_t sample_cand_size = 0;
    // KV prefetch of the next attention into MALL on a side stream (0 = off; else min KV length)
    int kv_prefetch_minp = 0;  // measured slower (Parler B = 8: 2.04 -> 2.53..3.16 ms/step), off by default
    int kv_prefetch_blocks = 128;
    hipStream_t pf_stream = nullptr;
    hipEvent_t pf_fork = nullptr, pf_join = nullptr;
    // tts_hip_tensor_set_async staging: a pinned ring; a region is reused once the event recorded
    // after its copy has completed (ggml_backend_i::set_tensor_async semantics: the caller may
    // reuse its buffer at once, the copy is ordered on the compute stream)
    uint8_t * pin = nullptr;
    size_t pin_size = 0, pin_head = 0;
    struct PinRec {
        size_t off, size;
        hipEvent_t ev;
    };
    std::deque<PinRec> pin_pending;
    std::vector<hipEvent_t> pin_events;
    std::mutex pin_mu;  // the ring is shared by every thread that uploads through this backend
    // completion of each plan slot's last launch: a slot is re-recorded only after it ran
    hipEvent_t plan_ev[2] = {nullptr, nullptr};
    bool plan_ev_pending[2] = {false, false};
    float * lstm_buf = nullptr;  // fused LSTM chains: per chain [Hd] cell state + [Hd, T] hidden history
    float * conv_stage = nullptr;  // fused conv output staging when it would alias its input and the im2col buffer is too small
    size_t conv_stage_floats = 0;
    float * vec_scratch = nullptr;  // 256K floats: per-channel vectors a fused item copies away from its output
    size_t lstm_floats = 0;
    tts::ActQuant aq;
    int64_t graph_epoch = 0;
    uint16_t * gelu_table = nullptr;  // 65536 fp16 entries (GGML_GELU_FP16 table)
    bool convt_lds = true;  // conv_transpose_1d on the LDS-staged f64 MFMA kernel (A/B knob)
    // f64 partial sums of input-channel-split codec convolutions (short sequences: the output
    // tiles alone would leave most CUs idle), summed in split order by a second pass
    double * conv_part = nullptr;
    size_t conv_part_doubles = 0;
    int conv_vfma = 1;   // TTS_HIP_OPT_CONV_VFMA: 0 = never, 1 = convs of fewer than 8 output channels, 2 = wherever it applies
    int conv_tile96 = 1;  // TTS_HIP_OPT_CONV_TILE96: the 96-row tile of the fused conv_1d when OC % 96 == 0
    int conv_pack = 1;    // TTS_HIP_OPT_CONV_PACK: unsplit fused conv_1d launches stage the kernel from its packed image
    int convt_pack = 1;   // TTS_HIP_OPT_CONVT_PACK: unsplit LDS conv_transpose_1d launches stage the weight from its packed image
    int conv_xreg = 1;    // TTS_HIP_OPT_CONV_XREG: k_conv1d_f64p holds its r -> x-slot table in registers
    bool capturing = false;  // capture_into is recording: no allocation, no launch outside the recorded graph
    int conv_split = 1;  // TTS_HIP_OPT_CONV_SPLIT: 1 = split short convolutions to ~512 workgroups, N > 1 = to ~N, 0 = never
    int fusion = 0x3FFF;  // bitmask of TTS_FUSE_* patterns (all on)
    bool profile_gemv = false;
    double gemv_ms[TTS_TYPE_COUNT] = {0};
    int64_t gemv_launches[TTS_TYPE_COUNT] = {0};
    double gemv_bytes[TTS_TYPE_COUNT] = {0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    std::vector<double> ev_bytes;
    std::vector<int> ev_type;
    std::vector<hipEvent_t> ev_free;
    char * repack_tmp = nullptr;  // device temp for Q4_K matrices not stored repacked
    size_t repack_tmp_size = 0;
    std::vector<char *> repack_retired;  // outgrown repack temps (freed with the backend)
    float * attn_stage = nullptr;  // k_attn_bias' output when the graph's output tensor overlaps an operand (then copied to it)
    size_t attn_stage_size = 0;
    // HIP graph replay of graph_compute (capture -> exec update -> one launch)
    bool use_graphs = false;
    // repeat detection for tts_hip_graph_compute: signatures of the last few graphs (node count, op
    // sequence, first / last shapes), each with its own executable graph so interleaved runners
    // (a decode step between vocoder calls) keep replaying
    static constexpr int N_GSIG = 4;
    uint64_t gsig[N_GSIG] = {};
    hipGraphExec_t gsig_exec[N_GSIG] = {};
    int gsig_next = 0;
    bool conv_f32acc = false;  // conv GEMM on f16 MFMA with f32 accumulation (faster, misses the PCM bar)
    int conv_acc_mode = 0;     // fused conv_1d: 0 = f64 MFMA, 2 = f16 MFMA per 32-term batch + f64 accumulation
    hipStream_t cap_stream = nullptr;  // records graphs (never runs work)
    int64_t graph_updates = 0, graph_instantiations = 0;
    int64_t lstm_chains = 0, lstm_steps = 0;
    int64_t plan_wait_ns = 0;
    int64_t cap_plan_ns = 0, cap_launch_ns = 0, cap_update_ns = 0;  // capture_into phases (host)  // host time spent in graph_prepare waiting for the slot's previous launch  // fused LSTM recurrences launched (tts_hip_counters)
    // two prepared plans (tts_hip_graph_prepare / _launch): step n+1 is recorded while step n runs
    hipGraphExec_t pexec[2] = {nullptr, nullptr};
    tts_tensor * const * plan_nodes[2] = {nullptr, nullptr};
    int plan_n[2] = {0, 0};
    bool plan_eager[2] = {true, true};
    bool plan_prepared[2] = {false, false};  // recorded by graph_prepare, not launched yet
    // step coalescer (coalesce.hip): set while this (hidden, per-device) backend runs a coalesced
    // plan; co_ev orders a member's stream with the coalesced launch
    tts::BatchCtx * bat = nullptr;
    hipEvent_t co_ev = nullptr;
    int64_t * co_tab = nullptr;  // device copy of a coalesced plan's per-item tables (ItemTab)
    size_t co_tab_bytes = 0;
    int64_t co_prep_ns = 0;      // host time of co_prepare + the tables' upload (coalesced steps)
    int64_t co_node_runs = 0;    // node runs made once per member inside coalesced steps (run_node_coalesced)
    bool co_member = true;  // TTS_HIP_OPT_COALESCE: this backend's graph_compute calls may join a coalesced step
    // read-back of a coalesced step's outputs: the executor copies this member's output tensors into
    // rb_host (pinned) in the step's own stream order, so tts_hip_tensor_get of such a range is served
    // from host memory after a stream synchronize instead of one device-to-host copy per member.
    // Entries are valid until this backend's next write or compute call (rb_clear).
    struct RbEnt {
        const char * dev;
        size_t bytes, off;
    };
    char * rb_host = nullptr;
    size_t rb_cap = 0;
    std::vector<RbEnt> rb;
    std::mutex rb_mu;                  // rb: the executor's thread writes it, this backend's callers read / drop it
    std::atomic<bool> rb_any{false};   // rb non-empty (checked before taking rb_mu)
    void rb_clear() {
        if (!rb_any.load(std::memory_order_acquire)) return;
        std::lock_guard<std::mutex> l(rb_mu);
        rb.clear();
        rb_any.store(false, std::memory_order_release);
    }
};

namespace tts {

// ---- process-wide weight registry (backend.hip) ----
// The tile-layout copy of a lane-layout Q4_K weight (TTS_FLAG_TILED_COPY), or null.
const uint8_t * tiled_copy_find(const void * weight);

// ---- profiled launches (k_gemv.hip): a start / stop event pair carried in the dispatch packets
// (hipExtLaunchKernelGGL), folded into tts_hip_gemv_stats under `type` with `bytes` algorithmic bytes
void profile_pair(tts_hip_backend * be, hipEvent_t & e0, hipEvent_t & e1);
void profile_push(tts_hip_backend * be, hipEvent_t e0, hipEvent_t e1, double bytes, int type);

// ---- launchers (k_gemv.hip) ----
// Quantize M columns (column stride xcs floats) of x to the vec_dot type of `wtype`.
void launch_quantize_act(tts_hip_backend * be, int wtype, const float * x, int64_t xcs, int64_t K, int64_t M, ActQuant & aq);
void launch_gemv_job(tts_hip_backend * be, const GemvJob & job);
bool gemv_q6k_ok(const GemvJob & j);  // a Q6_K job k_gemv_q6_K can take (f32 activation for its prologue, one row count, even addresses)
// F32 weights x many columns (k_gemm.hip): bit-identical to the sequential-f64 float dot
bool launch_bgemm_f32(tts_hip_backend * be, const tts_tensor * node);
bool gemm_f32_ok(const GemvJob & j);
void launch_gemm_f32(tts_hip_backend * be, const GemvJob & j);
void launch_copy_cols(tts_hip_backend * be, float * dst, const float * src, int64_t K, int64_t scs, int64_t M);
void launch_profile_spin(tts_hip_backend * be, double us);
void launch_im2col(tts_hip_backend * be, const tts_tensor * node);
// One fused LSTM recurrence step (Kokoro build_lstm_run, src/models/kokoro/model.cpp:56-86): the
// four h-GEMVs, bias and input-projection adds, gate activations and the cell update, gate order
// I, F, G, O (weights[1], [3], [5], [7] of the reference's cell).
constexpr int kLstmQMaxK = 512;  // longest row of the quantized step (k_lstm_step_q, k_fused.hip)
struct LstmStepArgs {
    const float * pre[4];   // column t of each gate's input projection (W_ih x + b_ih), Hd floats
    const void * w[4];      // W_hh [Hd rows of K]: F32 or F16 (16-byte aligned rows), Q8_0, Q5_0 or Q4_0 (2-byte aligned rows,
                            // K % 32 == 0, K <= kLstmQMaxK)
    int64_t w_rs[4];        // row stride, bytes
    const float * bias[4];  // b_hh [Hd]
    const float * hprev;    // [K]
    const float * cprev;    // [Hd]
    float * h;              // [Hd] out
    float * c;              // [Hd] out (may alias cprev: per-unit read-then-write)
    int Hd, K, wtype;
};
// b: a second, independent chain advanced by the same launch (bidirectional pairs), or null
void launch_lstm_step(tts_hip_backend * be, const LstmStepArgs & a, const LstmStepArgs * b = nullptr);
void launch_repeat_interleave1(tts_hip_backend * be, const tts_tensor * dst, const tts_tensor * a, int r);
void launch_copy_bytes(tts_hip_backend * be, void * dst, const void * src, size_t bytes);
void launch_cpy_multi(tts_hip_backend * be, const tts_tensor * src, const tts_tensor * const * dsts, int nd);
void launch_rope_multi(tts_hip_backend * be, const tts_tensor * rope, const tts_tensor * src, const tts_tensor * const * dsts, int nd);
// the same two passes over the N members of a coalesced step (the member is a grid dimension): member k's source
// at src + k * xms bytes, its destination d at dsts[d] + doff[d * N + k] floats, its rope positions at pos + poff[k]
void launch_cpy_multi_co(tts_hip_backend * be, const tts_tensor * src, const tts_tensor * const * dsts, int nd, int N, int64_t xms,
                         const int64_t * doff);
void launch_rope_multi_co(tts_hip_backend * be, const tts_tensor * rope, const tts_tensor * src, const tts_tensor * const * dsts, int nd,
                          int N, int64_t xms, const int64_t * doff, const int64_t * poff);
void launch_greedy_step(tts_hip_backend * be, const float * logits, int B, int NH, int V, int step, int bos, int eos, int32_t * eos_seen,
                        int32_t * hist, int32_t * next);
int launch_sample_step(tts_hip_backend * be, const float * logits, int B, int NH, int V, const tts_sampling * c, int64_t call,
                       int32_t * rep_state, int step, int bos, int eos, int32_t * eos_seen, int32_t * hist, int32_t * next);
struct BatchCtx;
void launch_embed_sum(tts_hip_backend * be, const tts_tensor * out, const tts_tensor * const * gr, int n, const BatchCtx * bat = nullptr,
                      const ItemTab * tab = nullptr);
// recip == nullptr: the kernel evaluates reciprocal() = one[0] / alpha[c] itself (`one` a broadcast scalar)
void launch_snake(tts_hip_backend * be, const tts_tensor * dst, const tts_tensor * x, const tts_tensor * alpha, const tts_tensor * recip,
                  const tts_tensor * one = nullptr, const tts_tensor * mask = nullptr);
void launch_lstm_finish(tts_hip_backend * be, const tts_tensor * final_out, const float * hist, int64_t Hd, int64_t T);
bool audio_op_supported(const tts_tensor * n);
int launch_audio_op(tts_hip_backend * be, const tts_tensor * n);
// w_stable: the planner proved the weight a constant leaf (Planner::const_leaf), so the launch may read its packed image
void launch_conv_transpose_1d(tts_hip_backend * be, const tts_tensor * node, int w_stable = 0);
// conv_1d chain (IM2COL -> MUL_MAT [-> ADD bias] [-> ADD residual]) as one implicit-GEMM kernel
constexpr int CONV1D_MAX_R = 128;
struct Conv1dArgs {
    TD x;                           // input [L, IC] f32 (any strides)
    const void * w = nullptr;       // kernel [K, IC, OC], element strides wk / wic / woc
    int w16 = 0;                    // kernel stored as F16 (else F32)
    int64_t wk = 0, wic = 0, woc = 0;
    float * y = nullptr;            // output [OL, OC]: y[ol + oc * ycs]
    int64_t ycs = 0;
    const float * bias = nullptr;   // bias[oc * bcs] or null
    int64_t bcs = 0;
    const float * res = nullptr;    // residual [OL, OC] (res[ol + oc * rcs]) or null
    int64_t rcs = 0;
    int64_t L = 0, IC = 0, OL = 0, OC = 0;
    int K = 1, s = 1, p = 0, d = 1;
    int icc = 0, xw = 0, rs = 0;    // set by the launcher
    float * copy_dst = nullptr;     // non-null: y is a staging buffer, copied here (contiguous) after the kernel
    uint32_t x_bytes = 0, w_bytes = 0;  // buffer-descriptor ranges (reads past them return 0)
    double * part = nullptr;        // split launch: f64 partial sums [gridDim.z][OC][OL], no epilogue
    int ic_per_split = 0;           // input channels per split (a multiple of icc)
    int w_stable = 0;               // planner: the kernel is a leaf no node of the graph writes (it may have a packed image)
    const float * wimg = nullptr;   // launcher: the kernel's packed image (conv_pack_get), read by k_conv1d_f64p
};
constexpr int CONV1D_XN = 16, CONV1D_WN = 16;  // staged elements per thread (x window, kernel slice)
inline int conv1d_icc(int64_t IC, int K, int xw) {  // input channels per LDS chunk
    // the reduction (icc * K) is padded to whole batches of 32 and held to 64 (so the kernel
    // slice is 64 x 64 floats, CONV1D_WN per thread); the x window (icc * xw floats) to
    // CONV1D_XN per thread.  Pick the icc that wastes the least, preferring larger chunks.
    int best = 0;
    double best_eff = -1.0;
    const int top = (int)(IC < 64 ? IC : 64);
    for (int c = 1; c <= top; ++c) {
        const int r = c * K, rp = (r + 31) & ~31;
        if (rp > 64 || c * xw > 256 * CONV1D_XN) break;
        const double eff = (double)r / rp + 1e-4 * c;
        if (eff > best_eff) best_eff = eff, best = c;
    }
    return best;  // 0: the shape does not fit (K > 64 or a window too wide)
}
bool conv1d_fused_ok(int64_t IC, int K, int s, int d, size_t * lds);
// The packed image of a conv kernel [K, IC, OC] for one tile geometry (oct rows per channel tile, icc input
// channels per chunk, the chunk's reduction padded to rp = 32 or 64): per (channel tile, chunk) the oct x rp
// slice k_conv1d_f64 stages -- f16-rounded floats, zero past the chunk's icc * K taps, past IC and past OC
// -- in the order k_conv1d_f64p holds it in LDS, [16-row tile][16 reduction slots][lane][4]: lane
// (kq = lane >> 4, c16 = lane & 15) finds row 16 t + c16's slots 16 g + 4 j + kq, j = 0..3, as 16
// contiguous bytes, the A operands of its MFMA steps 4 (g & 1) + j of batch g >> 1.  A slice is a straight
// 16-byte-per-thread copy into LDS.  This function alone defines the layout (pack kernel and conv kernel).
__host__ __device__ inline int64_t conv1d_pack_index(int nchunk, int oct, int rp, int ct, int chunk, int row, int r) {
    const int lane = (r & 3) * 16 + (row & 15);
    return (int64_t)(ct * nchunk + chunk) * oct * rp + ((((row >> 4) * (rp >> 4) + (r >> 4)) * 64 + lane) * 4 + ((r >> 2) & 3));
}
// The packed image of a conv_transpose_1d weight [K = 2 S, OC, IC] for k_convt_f64_img: per (tile of 32 output
// channels, chunk of 16 input channels) the 16 x K x 32 slice -- the weight's own f32 values (an F16 weight
// converts exactly), zero past IC and past OC -- in the kernel's LDS order [tap][channel half][ic][16 channels].
// One MFMA step's A read (tap, half; lanes kq = input channel, c16 = channel) covers 64 consecutive floats, and
// a slice is a straight 16-byte-per-thread copy into LDS.  This function alone defines the layout.
__host__ __device__ inline int convt_pack_index(int tap, int half, int icl, int c16) { return (((tap * 2 + half) * 16 + icl) * 16) + c16; }
struct ConvPackKey {  // one image: the backend that owns it, the source bytes' layout, the tile geometry
    const tts_hip_backend * be;
    const void * w;
    int kind = 0;  // 0: conv_1d (conv1d_pack_index), 1: conv_transpose_1d (convt_pack_index: oct 32, icc 16, rp 16 K)
    int w16, K, oct, icc, rp;
    int64_t IC, OC, wk, wic, woc;
    bool operator<(const ConvPackKey & o) const {
        return std::tie(be, w, kind, w16, K, oct, icc, rp, IC, OC, wk, wic, woc) <
               std::tie(o.be, o.w, o.kind, o.w16, o.K, o.oct, o.icc, o.rp, o.IC, o.OC, o.wk, o.wic, o.woc);
    }
    int nchunk() const { return (int)((IC + icc - 1) / icc); }
    int ntile() const { return (int)((OC + oct - 1) / oct); }
    size_t floats() const { return (size_t)ntile() * nchunk() * oct * rp; }
};
void launch_conv1d_pack(hipStream_t stream, const ConvPackKey & k, float * img);  // k_conv.hip
// The image table (backend.hip).  get: the image of `k`, made on be->stream at the first request (null while a
// graph is being recorded and the image does not exist yet, or when memory is short: the caller stages as before).
// written: a write of [p, p + n) through `be` was queued on its stream -- every image whose source overlaps is
// packed again, into the same buffer, on that stream.  freed: the sources in [p, p + n) are gone, their images too.
const float * conv_pack_get(tts_hip_backend * be, const ConvPackKey & k);
void conv_pack_written(tts_hip_backend * be, const void * p, size_t n);
void conv_pack_freed(const tts_hip_backend * be, const void * p, size_t n);
// The image launch_conv1d_fused will ask for (k_conv.hip), or false where this launch keeps k_conv1d_f64's staging.
bool conv1d_pack_key(const tts_hip_backend * be, const Conv1dArgs & a, ConvPackKey * k);
// The same for launch_conv_transpose_1d of `node` (w_stable as there): false where it keeps k_convt_f64_lds.
bool convt_pack_key(const tts_hip_backend * be, const tts_tensor * node, int w_stable, ConvPackKey * k);
// AdaIN (+ snake) per channel row: y[c][t] = snake((norm(x[c])[t] * (1 + g[c])...) -- see k_fused.hip
struct AdainArgs {
    const float * x = nullptr;   // NORM input rows: x[c * xcs + t], t < T
    int64_t xcs = 0;
    float * y = nullptr;         // output rows (the [T, C] tensor after the second transpose)
    int64_t ycs = 0;
    const float *gamma = nullptr, *beta = nullptr, *alpha = nullptr, *recip = nullptr;  // alpha null: no snake
    const float * one = nullptr;  // recip null: recip[c] = one[0] / alpha[c] (reciprocal()'s DIV)
    int stage = 0;  // 1: the output overlaps a vector's memory -> copy the vectors to be->vec_scratch first
    // gamma / beta evaluated in the kernel (their MUL_MAT + bias ADD absorbed): gamma[c] =
    // dot(gw[c * S ...], style) + gb[c], in k_gemv_float's exact order; gw null: read gamma / beta
    const float *gw = nullptr, *gb = nullptr, *bw = nullptr, *bb = nullptr, *style = nullptr;
    int64_t S = 0;
    int64_t gcs = 1, bcs = 1, acs = 1, rcs = 1;
    int64_t T = 0, C = 0;
    float eps = 0.f;
};
bool adain_supported(int64_t T);
void launch_adain_snake(tts_hip_backend * be, const AdainArgs & a);
void launch_conv1d_fused(tts_hip_backend * be, Conv1dArgs a);
bool launch_gemm_f16(tts_hip_backend * be, const tts_tensor * node);
size_t act_quant_bytes(int wtype, int64_t K, int64_t M);
// carve an ActQuant layout for weight type `wtype` out of `base` (no launch)
void act_quant_layout(int wtype, char * base, int64_t K, int64_t M, ActQuant & aq);

void launch_repack_q4_K(tts_hip_backend * be, const void * src, void * dst, int64_t nblocks, int inverse);

// ---- launchers (k_ops.hip) ----
int launch_op(tts_hip_backend * be, const tts_tensor * node);
void launch_copy_stream(tts_hip_backend * be, void * dst, const void * src, int64_t n16);  // tts_hip_copy_stream

// ---- graph execution (graph_exec.hip) and the step coalescer (coalesce.hip) ----
// Plan and launch a node list on be->stream (be->bat set: as a coalesced step of be->bat->N members;
// TTS_STATUS_UNSUPPORTED, before any launch, when the plan has an item without a coalesced form).
int graph_compute_launches(tts_hip_backend * be, tts_tensor * const * nodes, int n_nodes);
// graph_compute of a one-prompt decode graph while other backends on the device submit the same graph:
// one coalesced launch for all of them.  Returns kCoalesceNotTaken when the caller runs the graph itself.
constexpr int kCoalesceNotTaken = 1 << 20;
int coalesce_submit(tts_hip_backend * be, tts_tensor * const * nodes, int n_nodes);
// buffer registry (backend.hip): the live tts_hip_buffer_alloc range holding p
bool buffer_lookup(const void * p, const char ** base, size_t * size);
// a coalesced step's read-only operands read through member 0's copy: (member 0's, member k's, bytes)
// pairs, true when every pair holds equal bytes (checked on the device, cached until a host write)
bool coalesce_check_shared(tts_hip_backend * ex, const std::vector<std::tuple<const void *, const void *, size_t>> & pairs);
void coalesce_backend_gone(const tts_hip_backend * be); // a backend is freed: no longer awaited
void coalesce_written(const void * p, size_t size);     // host writes: content checks over the range are dropped
bool coalesce_enabled();
bool co_debug();  // TTS_HIP_COALESCE_DEBUG=1 (graph_exec.hip)

}  // namespace tts
