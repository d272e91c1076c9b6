// Shared device helpers for the gfx950 kernels (wave = 64 lanes, everywhere): element types and their 16-byte lane accesses,
// register vectors, bf16 pair packing (the precision contract of the fp32-with-bf16-slot path), the bf16 MFMA on packed dwords,
// the 16-byte LDS-DMA and the GEMM epilogue activations.  Every helper is __forceinline__: it costs what its body costs.
// wkv6.hip / wkv6_mfma.inc keep copies of their own (pack_exact, cvt_pk, split_pk, mfma_bf16, lds_dma16, ...): the benchmark
// attributes the scan's measured HBM traffic to the hash of exactly those two files, so they are frozen, and nothing here may
// declare a function or struct under one of their names.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pafc {

constexpr int kWave = 64;

typedef uint16_t bf16_t;  // raw bits; arithmetic is always float

// register vectors (HIP's float4 / uint4 are structs: selects and array elements of them go through memory)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// round-to-nearest-even through the hardware conversion (v_cvt_pk_bf16_f32: one instruction per two values; a
// hand-rolled integer rounding costs ~5 VALU ops per value and was the top cost of the element-wise kernels).
// Same mapping as c10::BFloat16 / the CPU oracle for every non-NaN input; NaN stays a (quiet) NaN.
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
    return (uint32_t)__builtin_bit_cast(unsigned short, static_cast<__bf16>(f));
}

__device__ __forceinline__ float round_bf16(float f) { return static_cast<float>(static_cast<__bf16>(f)); }

template <typename ET> struct Elem;
template <> struct Elem<float> {
    static constexpr int kPerLane = 4;  // elements in one 16-byte lane access
    __device__ static __forceinline__ void unpack(const uint4 &q, float *f) {
        f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y);
        f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
    }
    __device__ static __forceinline__ float load(const float *p) { return *p; }
    __device__ static __forceinline__ void store(float *p, float v) { *p = v; }
    __device__ static __forceinline__ float round(float v) { return v; }
};
template <> struct Elem<bf16_t> {
    static constexpr int kPerLane = 8;
    template <typename Q>   // the 16 bytes as a uint4 or a u32x4
    __device__ static __forceinline__ void unpack(const Q &q, float *f) {
        f[0] = bf16_bits_to_f32(q.x & 0xffffu); f[1] = __uint_as_float(q.x & 0xffff0000u);
        f[2] = bf16_bits_to_f32(q.y & 0xffffu); f[3] = __uint_as_float(q.y & 0xffff0000u);
        f[4] = bf16_bits_to_f32(q.z & 0xffffu); f[5] = __uint_as_float(q.z & 0xffff0000u);
        f[6] = bf16_bits_to_f32(q.w & 0xffffu); f[7] = __uint_as_float(q.w & 0xffff0000u);
    }
    __device__ static __forceinline__ void unpack4(uint2 q, float *f) {   // 8 bytes: the 4-wide half
        f[0] = bf16_bits_to_f32(q.x & 0xffffu); f[1] = __uint_as_float(q.x & 0xffff0000u);
        f[2] = bf16_bits_to_f32(q.y & 0xffffu); f[3] = __uint_as_float(q.y & 0xffff0000u);
    }
    __device__ static __forceinline__ float load(const bf16_t *p) { return bf16_bits_to_f32(*p); }
    __device__ static __forceinline__ void store(bf16_t *p, float v) { *p = (bf16_t)f32_to_bf16_bits(v); }
    __device__ static __forceinline__ float round(float v) { return round_bf16(v); }
};

// 8 consecutive elements of a row <-> 8 floats: fp32 as two float4, bf16 as one uint4 (rounded to nearest even on the way out)
template <typename ET> __device__ __forceinline__ void load8(const ET *p, float *f);
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t *p, float *f) {
    Elem<bf16_t>::unpack(*reinterpret_cast<const uint4 *>(p), f);
}
template <> __device__ __forceinline__ void load8<float>(const float *p, float *f) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <typename ET> __device__ __forceinline__ void store8(ET *p, const float *f);
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t *p, const float *f) {
    uint4 q;
    q.x = f32_to_bf16_bits(f[0]) | (f32_to_bf16_bits(f[1]) << 16);
    q.y = f32_to_bf16_bits(f[2]) | (f32_to_bf16_bits(f[3]) << 16);
    q.z = f32_to_bf16_bits(f[4]) | (f32_to_bf16_bits(f[5]) << 16);
    q.w = f32_to_bf16_bits(f[6]) | (f32_to_bf16_bits(f[7]) << 16);
    *reinterpret_cast<uint4 *>(p) = q;
}
template <> __device__ __forceinline__ void store8<float>(float *p, const float *f) {
    reinterpret_cast<float4 *>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
    reinterpret_cast<float4 *>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

// two floats -> one dword of two bf16, low half = first
__device__ __forceinline__ unsigned pack_bf16_exact(float lo, float hi) {   // both already bf16 values
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack_bf16_rne(float lo, float hi) {     // round to nearest even: one v_cvt_pk_bf16_f32
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// (a, b) = hi + lo with hi, lo packed bf16 pairs (16 significant bits per value)
struct Bf16HiLo { unsigned hi, lo; };
__device__ __forceinline__ Bf16HiLo split_bf16_hilo(float a, float b) {
    Bf16HiLo r;
    r.hi = pack_bf16_rne(a, b);
    r.lo = pack_bf16_rne(a - __uint_as_float(r.hi << 16), b - __uint_as_float(r.hi & 0xffff0000u));
    return r;
}

// v_mfma_f32_16x16x32_bf16 on operands held as four packed dwords (8 bf16 per lane: A[m = l&15][k = 8(l>>4) + e],
// B[k = 8(l>>4) + e][n = l&15]): register vectors by value, or with a uint4 (HIP's struct) among them, read where it lies
__device__ __forceinline__ f32x4 mfma_bf16_packed(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <typename A, typename B> __device__ __forceinline__ f32x4 mfma_bf16_packed(const A &a, const B &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// LDS-DMA: 16 bytes per lane from the lane's global address to (wave-uniform LDS address + 16 * lane)
template <typename ET> __device__ __forceinline__ void global_to_lds16(const ET *src, ET *lds_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_base, 16, 0, 0);
}

// The activation of a GEMM epilogue, act = 0 none, 1 SiLU, 2 tanh, 3 ReLU (the codes of include/pafc_encoder_ops.h), on the
// hardware reciprocal: tanh(v) = 1 - 2 / (exp(2v) + 1) saturates correctly at +-inf.  Compile-time and run-time code.
template <int ACT> __device__ __forceinline__ float epilogue_act(float v) {
    if constexpr (ACT == 1) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));
    if constexpr (ACT == 2) return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * v) + 1.f);
    if constexpr (ACT == 3) return fmaxf(v, 0.f);
    return v;
}
__device__ __forceinline__ float epilogue_act(float v, int act) {
    if (act == 1) return epilogue_act<1>(v);
    if (act == 2) return epilogue_act<2>(v);
    if (act == 3) return epilogue_act<3>(v);
    return v;
}

// logistic function on the exact exponential and a true division (the LSTM gates of the RNN-T predictor)
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// Compute units of the current device, asked once per device and process (host side; 256 if the query fails).
inline int device_cus() {
    static int cached[64];                 // 0 = not asked yet; a racing first call writes the same value twice
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int c = cached[dev];
    if (c <= 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cached[dev] = c;
    }
    return c;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

}  // namespace pafc
