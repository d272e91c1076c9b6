// Shared by the Mamba-2 SSD scan kernels (mamba2_scan.hip, mamba2_scan_bwd.hip): tile sizes, the bf16 MFMA and the packing /
// splitting helpers of its operands.  Included inside namespace pafc { namespace { ... } }.
constexpr int SN = 128, SP = 64, SBL = 16;
typedef float sf32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sbf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int su32x4 __attribute__((ext_vector_type(4)));
typedef float sf32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 sbf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ sf32x4 smfma(su32x4 a, su32x4 b, sf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sbf16x8, a), __builtin_bit_cast(sbf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned spack_exact(float lo, float hi) {   // two floats that ARE bf16 values
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}
__device__ __forceinline__ unsigned scvt_pk(float a, float b) {
    const sf32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, sbf16x2));
}
struct SHiLo { unsigned hi, lo; };
__device__ __forceinline__ SHiLo ssplit_pk(float a, float b) {          // (a, b) = hi + lo, packed bf16 pairs
    SHiLo r;
    r.hi = scvt_pk(a, b);
    r.lo = scvt_pk(a - __uint_as_float(r.hi << 16), b - __uint_as_float(r.hi & 0xffff0000u));
    return r;
}
template <int CTRL>
__device__ __forceinline__ float row_shr_zero(float x) {                 // lane t <- lane t - n of its 16-lane row, 0 outside
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
