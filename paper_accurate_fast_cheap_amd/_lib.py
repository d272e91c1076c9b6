"""ctypes binding of libpafc_hip.so -- the only way product code reaches a kernel.

There is no CPU fallback anywhere in this package: if the library is missing or
a tensor is not on the GPU the call raises.  (The CPU restatement lives under
oracle/ and is test infrastructure; nothing here imports it.)
"""
import ctypes
import os
from ctypes import c_float, c_int, c_long, c_size_t, c_ulonglong, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libpafc_hip.so")

PAFC_F32, PAFC_BF16 = 0, 1
_ERRORS = {
    -1: "null pointer", -2: "bad dims (B, T, C, H must be positive and C == H * 64)", -3: "head size must be 64",
    -4: "workspace too small", -5: "kernel launch failed", -6: "unsupported dtype", -7: "unsupported",
    -8: "r, k, v, w, y must be 16-byte aligned",
}


class PafcError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the C-ABI library; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    variant = os.environ.get("PAFC_SO_PATH")     # A/B measurements: a variant of the library built by csrc.build --extra / --out
    if variant:
        if not os.path.exists(variant):
            raise PafcError(f"PAFC_SO_PATH={variant} does not exist")
        _lib = _bind(ctypes.CDLL(variant))
        return _lib
    if not os.path.exists(SO_PATH):
        raise PafcError(
            f"{SO_PATH} is missing: the HIP extension has not been built "
            "(python -m paper_accurate_fast_cheap_amd.csrc.build). There is no CPU fallback.")
    from .csrc import build as _build
    if _build.built_key() != _build.source_key():
        raise PafcError(
            f"{SO_PATH} was not built from the sources in this tree (libpafc_hip.so.json: {_build.built_key()}, sources: "
            f"{_build.source_key()}): rebuild with python -m paper_accurate_fast_cheap_amd.csrc.build")
    _lib = _bind(ctypes.CDLL(SO_PATH))
    return _lib


# Every prototype of include/*.h: symbol -> (restype, argtypes), grouped by header in header order.  `lib()` applies the
# whole table once, so a kernel call is a plain call on the CDLL's function attribute.  C types map as int: I, long and
# int64_t: G, size_t: Z, float: F, unsigned long long and uint64_t: U, any pointer and pafc_stream_t: P (tests/test_abi.py
# checks the table against the headers).
P, I, G, Z, F, U = c_void_p, c_int, c_long, c_size_t, c_float, c_ulonglong
SIGNATURES = {
    # include/pafc_attention.h
    "pafc_mha_rows": (I, [I, I, I, I, P, G, P, P, G, P, P, P, I, P, G, P]),
    "pafc_logp_gather_rows": (I, [I, G, I, P, G, P, P, P]),
    "pafc_mha_band": (I, [I, I, I, I, I, I, I, P, G, P, P, G, P, G, P, P, P, G, P]),
    "pafc_mha_rows_lse": (I, [I, I, I, I, P, G, P, P, G, P, P, P, I, P, G, P, P]),
    "pafc_mha_rows_bwd_workspace_bytes": (Z, [G, I]),
    "pafc_mha_rows_bwd": (I, [I, I, I, I, G, P, G, P, P, G, P, G, P, G, P, P, P, P, I, P, G, P, P, G, P, Z, P]),
    "pafc_lsm_loss_rows": (I, [I, G, I, P, G, P, F, P, P, P, P]),
    "pafc_lsm_loss_rows_bwd": (I, [I, G, I, P, G, P, F, P, P, P, G, P]),
    "pafc_mha_band_lse": (I, [I, I, I, I, I, I, I, P, G, P, P, G, P, G, P, P, P, G, P, P]),
    "pafc_mha_band_bwd_workspace_bytes": (Z, [I, I, I]),
    "pafc_mha_band_bwd": (I, [I, I, I, I, I, I, I, P, G, P, P, G, P, G, P, P, P, G, P, G, P, P, G, P, P, G, P, G, P, P, P, Z,
                              P]),
    # include/pafc_attn_search.h
    "pafc_mha_step": (I, [I, I, I, I, I, I, P, G, P, P, P, P, P, G, P]),
    "pafc_attn_beam_select_workspace_bytes": (Z, [I, I]),
    "pafc_attn_beam_select": (I, [I, I, I, I, I, I, I, P, G, P, P, P, P, P, P, P, P, P, P, Z, P]),
    # include/pafc_joint_search.h
    "pafc_mha_step_paths": (I, [I, I, I, I, I, I, P, G, P, P, G, P, P, P, P, G, P]),
    "pafc_joint_candidates": (I, [I, I, I, I, I, I, F, P, P, P, P, P, P, P]),
    "pafc_joint_frame": (I, [P, I, I, I, P, G, P, P, I, P]),
    "pafc_joint_collect": (I, [P, P, P, P, P, P, P, P]),
    # include/pafc_encoder_ops.h
    "pafc_dwconv1d_cl": (I, [I, I, I, I, I, I, I, P, P, P, P, I, P, P]),
    "pafc_dwconv1d_cl_ex": (I, [I, I, I, I, I, I, I, P, G, P, P, P, I, P, P]),
    "pafc_dwconv1d_cl_ln_silu": (I, [I, I, I, I, I, I, I, P, G, P, P, P, P, F, P, P, P]),
    "pafc_dwconv1d_cl_wgrad_workspace_bytes": (Z, [I, I, I, I]),
    "pafc_dwconv1d_cl_wgrad": (I, [I, I, I, I, I, I, I, P, G, P, P, P, P, Z, P]),
    "pafc_add_layernorm": (I, [I, I, I, I, P, P, F, P, I, I, P, P, P, P, G, I, I, P, P, P, G, F, P]),
    "pafc_add_layernorm_ex": (I, [I, I, I, I, I, P, P, F, P, I, I, P, P, P, P, G, I, I, P, P, P, G, F, P, P, P]),
    "pafc_gemm_bf16_ph_ln": (I, [G, I, I, P, G, P, G, P, P, G, P, G, F, I, I, P, P, I, F, I, P]),
    "pafc_split_planes": (I, [G, I, P, G, P, G, G, I, P]),
    "pafc_layernorm_bwd_workspace_bytes": (Z, [G, I]),
    "pafc_layernorm_bwd": (I, [I, I, G, I, P, P, P, F, P, P, P, Z, P]),
    "pafc_layernorm_bwd_add": (I, [I, I, G, I, P, P, P, F, P, P, P, P, Z, P]),
    "pafc_layernorm_silu_fwd": (I, [I, I, G, I, P, P, P, F, P, P]),
    "pafc_layernorm_silu_bwd": (I, [I, I, G, I, P, P, P, P, F, P, P, P, Z, P]),
    "pafc_gemm_skinny_bf16": (I, [G, I, I, I, P, G, G, P, G, G, P, G, P, G, G, P, G, G, F, I, P, I, P, F, P, P]),
    "pafc_gemm_skinny_bf16_ex": (I, [G, I, I, I, P, G, G, P, G, G, P, G, P, G, G, P, G, G, F, I, I, P, I, I, P, F, P, P, P, I,
        P, P, F, P]),
    "pafc_decay_lora_skinny_bf16": (I, [G, I, I, P, G, P, P, P, P, G, P]),
    "pafc_tmix_shift_mix": (I, [I, I, I, I, I, I, P, P, P, P, P]),
    "pafc_tmix_mix4": (I, [I, I, I, I, I, I, P, P, P, P, P]),
    "pafc_tmix_lora_mix4_bf16": (I, [I, I, I, I, I, P, P, P, P, P, P]),
    "pafc_tmix_lora_down_bf16": (I, [I, I, I, I, I, I, P, P, P, P, P]),
    "pafc_tmix_shift_mix_prev": (I, [I, I, I, I, I, I, P, P, P, P, P, P]),
    "pafc_tmix_lora_mix4_bf16_prev": (I, [I, I, I, I, I, P, P, P, P, P, P, P]),
    "pafc_tmix_lora_down_bf16_prev": (I, [I, I, I, I, I, I, P, P, P, P, P, P]),
    "pafc_decay_lora_bf16": (I, [G, I, I, I, P, P, P, P, P, P]),
    "pafc_tmix_bwd_workspace_bytes": (Z, [G, I]),
    "pafc_tmix_shift_mix_bwd": (I, [I, I, I, I, I, P, P, P, P, P, P, Z, P]),
    "pafc_tmix_mix4_bwd": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, Z, P]),
    "pafc_tmix_mix4_bwd_rows": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, Z, P]),
    "pafc_conv3x3s2_nhwc_bf16": (I, [I, I, I, I, I, P, P, P, P, I, P]),
    "pafc_conv3x3s2_c1_nhwc_bf16": (I, [I, I, I, I, P, P, P, P, I, P]),
    "pafc_conv3x3s2_c1_wgrad_workspace_bytes": (Z, [I, I, I]),
    "pafc_conv3x3s2_c1_wgrad_bf16": (I, [I, I, I, I, P, P, P, P, P, Z, P]),
    "pafc_conv3x3s2_c1_nhwc_f32split": (I, [I, I, I, I, P, P, P, P, P, I, P]),
    "pafc_conv3x3s2_c1_nhwc_f32split_ps": (I, [I, I, I, I, P, P, P, P, P, G, I, P]),
    "pafc_conv3x3s2_nhwc_f32split": (I, [I, I, I, I, I, P, P, P, P, P, P, I, P]),
    "pafc_gemm_tn_workspace_bytes": (Z, [G, I, I]),
    "pafc_gemm_tn_bf16": (I, [G, I, I, P, G, P, G, P, P, I, P, Z, P]),
    "pafc_gemm_tn_batched_workspace_bytes": (Z, [G, I, I, I]),
    "pafc_gemm_tn_bf16_batched": (I, [G, I, I, I, P, G, G, P, G, G, P, P, I, P, Z, P]),
    "pafc_gemm_bf16_f32out": (I, [G, I, I, P, G, I, P, G, P, P, G, P, I, G, G, F, I, P, Z, P]),
    "pafc_gemm_bf16_f32out_pb": (I, [G, I, I, P, G, I, I, P, G, P, P, G, P, I, G, G, F, I, P, Z, P]),
    "pafc_gemm_bf16_f32out_workspace_bytes": (Z, [G, I, I, I]),
    "pafc_ctc_loss_workspace_bytes": (Z, [I, I, I]),
    "pafc_ctc_loss_forward": (I, [I, I, I, I, P, G, P, P, I, P, I, I, P, P, Z, P]),
    "pafc_ctc_loss_backward": (I, [I, I, I, I, P, G, P, P, I, P, I, I, P, P, F, P, G, P, Z, P]),
    "pafc_rnnt_joint_loss_workspace_bytes": (Z, [I, I, I, G, G, P, I]),
    "pafc_rnnt_joint_loss_forward": (I, [I, I, I, I, I, P, G, G, P, G, G, P, P, P, P, P, I, I, G, P, P, Z, P]),
    "pafc_rnnt_joint_loss_backward": (I, [I, I, I, I, I, P, G, G, P, G, G, P, P, P, P, P, I, I, G, P, G, P, F, I, P, P, P, P,
        P, Z, P, Z, P]),
    "pafc_gemm_f32": (I, [G, I, I, I, P, G, G, P, G, G, P, G, P, G, G, P, G, G, F, I, P]),
    "pafc_mamba2_prep": (I, [I, I, I, I, P, P, G, P, P, P, P, P, P, P, P, P]),
    "pafc_mamba2_finish": (I, [I, I, I, I, P, P, P, P, G, P, G, P, P, P, F, I, P, P]),
    "pafc_mamba2_scan_chunk_len": (I, [I, I, I]),
    "pafc_mamba2_scan_workspace_bytes": (Z, [I, I, I, I]),
    "pafc_mamba2_scan": (I, [I, I, I, P, G, P, P, P, I, P, Z, P]),
    "pafc_mamba2_scan_dir": (I, [I, I, I, P, G, P, P, P, I, I, P, Z, P]),
    "pafc_mamba2_scan_skip_bf16": (I, [I, I, I, P, G, P, P, P, P, I, I, P, Z, P]),
    "pafc_mamba2_gate_norm": (I, [I, G, I, P, P, G, P, F, P, P]),
    "pafc_mamba2_scan_state": (I, [I, I, I, P, G, P, P, P, P, P, P, P, I, I, P, Z, P]),
    "pafc_mamba2_scan_bwd_workspace_bytes": (Z, [I, I, I, I]),
    "pafc_mamba2_scan_backward": (I, [I, I, I, P, G, P, P, P, P, G, P, P, I, I, P, Z, P]),
    "pafc_gemm_bf16": (I, [G, I, I, I, P, G, G, P, G, G, P, G, P, G, G, P, G, G, F, I, P]),
    "pafc_gemm_bf16_glu_half": (I, [G, I, I, I]),
    "pafc_conv3x3s2_nhwc_bf16_ph": (I, [I, I, I, I, I, P, P, P, P, I, I, P]),
    "pafc_gemm_bf16_ph": (I, [G, I, I, I, P, G, G, P, G, G, P, G, P, G, G, P, G, G, F, I, I, I, P]),
    "pafc_gemm_ph_ex": (I, [G, I, I, I, P, G, G, I, P, G, G, P, G, P, I, G, G, P, I, G, G, G, F, I, I, P]),
    "pafc_gemm_ph_ex2": (I, [G, I, I, I, P, G, G, I, I, P, G, G, P, G, P, I, G, G, P, I, G, G, G, F, I, I, P]),
    "pafc_gemm_ph_ktail": (I, [G, I, I, I, P, G, G, I, I, P, G, G, P, G, P, I, G, G, P, I, G, G, G, F, I, I, P, Z, G, I, P]),
    "pafc_gemm_ph_ktail_plan": (I, [G, I, I, I, I, I, P]),
    "pafc_conv3x3s2_nhwc_split_ph": (I, [I, I, I, I, I, P, P, P, P, I, I, P]),
    "pafc_residual_dropout": (I, [I, I, I, G, P, P, P, F, F, U, U, P]),
    "pafc_silu_dropout": (I, [I, I, G, P, P, P, F, U, U, P]),
    "pafc_multi_transpose_bf16": (I, [P, I, I, P]),
    "pafc_multi_cast_bf16": (I, [P, I, I, P]),
    "pafc_rows_gather": (I, [P, P, I, P, P, I, I, P]),
    "pafc_rows_scatter": (I, [P, P, I, P, I, I, P]),
    # include/pafc_fbank.h
    "pafc_fbank_num_frames": (G, [G]),
    "pafc_fbank_tables_cols": (I, []),
    "pafc_fbank_f32": (I, [P, G, P, P, P, P, P, I, P, F, F, P, P]),
    "pafc_fbank_batch": (I, [P, G, P, I, G, P, P, P, P, P, I, P, F, F, P, I, P, P]),
    "pafc_fbank_stream_plan": (I, [I, G, P, P]),
    "pafc_fbank_stream": (I, [P, I, P, G, G, I, P, P, P, P, P, I, F, F, P, I, G, G, P]),
    "pafc_fbank_stream_rows": (I, [P, I, P, P, I, P, G, G, P, P, P, P, P, I, F, F, P, I, I, P]),
    # include/pafc_resample.h
    "pafc_resample_num_out": (G, [G, I, I]),
    "pafc_resample_stream_plan": (I, [I, I, I, I, G, P, P]),
    "pafc_resample_batch": (I, [P, G, P, I, G, I, I, I, P, P, I, P, G, P, P]),
    "pafc_resample_rows": (I, [P, G, I, P, P, I, P, G, G, I, I, I, P, P, I, P, G, P]),
    # include/pafc_search.h
    "pafc_ctc_greedy": (I, [I, I, I, I, P, P, I, P, P, P, P, P]),
    "pafc_log_softmax_rows": (I, [I, G, I, P, P, P]),
    "pafc_ctc_prefix_beam_workspace_bytes": (Z, [I, I, I]),
    "pafc_ctc_prefix_beam_search": (I, [I, I, I, P, P, P, I, I, P, P, P, P, Z, P]),
    "pafc_ctc_prefix_beam_ex_workspace_bytes": (Z, [I, I, I]),
    "pafc_ctc_prefix_beam_search_ex": (I, [I, I, I, P, P, P, I, I, P, P, P, P, P, P, Z, P]),
    "pafc_ctc_beam_stream_workspace_bytes": (Z, [I, I, I, I]),
    "pafc_ctc_beam_stream_reset": (I, [I, I, I, I, P, P, Z, P]),
    "pafc_ctc_beam_stream_feed": (I, [I, I, I, P, P, P, I, I, I, P, I, P, Z, P]),
    "pafc_ctc_beam_stream_drain": (I, [I, I, I, P, I, P, Z, P, I, P, P, P, P, P, P, I, P, P, P]),
    "pafc_ctc_greedy_stream_workspace_bytes": (Z, [I]),
    "pafc_ctc_greedy_stream_reset": (I, [I, P, P, Z, P]),
    "pafc_ctc_greedy_stream": (I, [I, I, I, I, P, P, I, P, Z, P, P, P, P, P]),
    "pafc_ctc_align_workspace_bytes": (Z, [I, I, I]),
    "pafc_ctc_align": (I, [I, I, I, I, P, G, P, P, I, P, I, P, Z, P, P, P, I, P, P, P]),
    "pafc_rnnt_beam_workspace_bytes": (Z, [I, I, I]),
    "pafc_rnnt_beam_init": (I, [I, I, I, I, P, Z, P, P, P]),
    "pafc_rnnt_beam_step": (I, [I, I, I, I, I, P, P, P, P, P, Z, P, P, P]),
    "pafc_rnnt_beam_finish": (I, [I, I, I, P, Z, P, P, P, P]),
    "pafc_rnnt_beam_stream_workspace_bytes": (Z, [I, I, I]),
    "pafc_rnnt_beam_stream_reset": (I, [I, I, I, I, P, P, Z, P, P, P]),
    "pafc_rnnt_beam_stream_feed": (I, [I, I, I, I, P, P, Z, P]),
    "pafc_rnnt_beam_stream_step": (I, [I, I, I, I, I, I, P, P, P, P, Z, P, P, P]),
    "pafc_rnnt_beam_stream_drain": (I, [I, I, I, P, Z, P, I, P, P, P, P, P, P, P]),
    "pafc_rnnt_beam_select_state": (I, [I, I, I, I, I, P, P, P, P, P, P]),
    "pafc_rnnt_greedy_workspace_bytes": (Z, [P, I, I, I]),
    "pafc_rnnt_greedy_init": (I, [P, I, I, I, I, P, P, Z, P]),
    "pafc_rnnt_greedy_step": (I, [P, I, I, I, I, P, P, Z, P, P]),
    "pafc_rnnt_greedy_finish": (I, [P, I, I, I, P, Z, I, P, P, P, P, P, P]),
    "pafc_rnnt_beam_body_workspace_bytes": (Z, [P, I, I]),
    "pafc_rnnt_beam_body": (I, [P, I, I, I, I, P, P, I, P, G, F, F, P, P, P, P, P, P, P, P, Z, P]),
    "pafc_rnnt_beam_body_advance": (I, [P, P]),
    "pafc_rnnt_greedy_stream_workspace_bytes": (Z, [P, I, I, I]),
    "pafc_rnnt_greedy_stream_reset": (I, [P, I, I, I, I, P, P, Z, P]),
    "pafc_rnnt_greedy_stream_feed": (I, [P, I, I, I, I, P, P, Z, P, P]),
    "pafc_rnnt_greedy_stream_drain": (I, [P, I, I, I, P, Z, I, P, P, P, P, P, P]),
    "pafc_rnnt_score_workspace_bytes": (Z, [I, I, I, G]),
    "pafc_rnnt_score": (I, [I, I, I, I, P, G, G, P, G, G, P, P, P, I, I, I, I, P, P, I, I, I, P, P, Z, P]),
    # include/pafc_wkv6.h
    "pafc_abi_version": (I, []),
    "pafc_selftest_lane_ops": (I, [P, P]),
    "pafc_wkv6_pick_chunk_len": (I, [I, I, I, I, I]),
    "pafc_wkv6_fwd_workspace_bytes": (Z, [I, I, I, I, I, I]),
    "pafc_wkv6_forward_bf16": (I, [I, I, I, I, P, P, P, P, P, P, I, P, Z, P]),
    "pafc_wkv6_forward_f32": (I, [I, I, I, I, P, P, P, P, P, P, I, P, Z, P]),
    "pafc_wkv6_forward_state": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, I, I, P, Z, P]),
    "pafc_wkv6_forward_bidir": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, I, P, Z, P]),
    "pafc_wkv6_forward_bidir_wbias": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, P, Z, P]),
    "pafc_wkv6_bwd_workspace_bytes": (Z, [I, I, I, I, I]),
    "pafc_wkv6_backward": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]),
    "pafc_wkv6_backward_state": (I, [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]),

}


def _bind(L):
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise PafcError(f"{name} is declared in include/*.h but missing from {L._name}: rebuild the library") from None
        fn.restype, fn.argtypes = restype, argtypes
    return L


def check(code: int, what: str):
    if code != 0:
        raise PafcError(f"{what}: {_ERRORS.get(code, code)}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return PAFC_F32
    if dt == torch.bfloat16:
        return PAFC_BF16
    raise PafcError(f"kernels take float32 or bfloat16, got {dt}")


# Host cost matters: a decode batch of short utterances is ~300 launches whose GPU time is below what Python needs to issue
# them (5.8 ms per encoder pass before, 4.2 ms after this and the cached plan stamps: profiles/r04o_host_issue_time.txt).
# torch.cuda.current_stream() builds a Stream object per call (~4 us); the raw-stream query is a plain C call.  Pointers and the
# stream stay c_void_p OBJECTS: ctypes passes those pointer-sized whatever a function's declared argtypes say.
def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t: torch.Tensor) -> c_void_p:
    """torch's CURRENT stream on the tensor's device as a raw hipStream_t: the stream the kernels launch on."""
    if _raw_stream is not None:
        idx = t.device.index
        return c_void_p(_raw_stream(idx if idx is not None else torch.cuda.current_device()))
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise PafcError("this op runs on the MI355X only (tensor is on %s); there is no CPU fallback" % t.device)
        if not t.is_contiguous():
            raise PafcError("kernel operands must be contiguous")
