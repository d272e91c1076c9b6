// Shared by the Mamba-2 SSD scan kernels (mamba2_scan.hip, mamba2_scan_bwd.hip): tile sizes and the row shifts (the bf16 MFMA
// and the packing / splitting helpers of its operands are pafc_common.h's).  Included inside namespace pafc { namespace { ... } }.
constexpr int SN = 128, SP = 64, SBL = 16;

template <int CTRL>
__device__ __forceinline__ float row_shr_zero(float x) {                 // lane t <- lane t - n of its 16-lane row, 0 outside
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
