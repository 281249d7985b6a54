"""ctypes view of include/lc_abi.h (libleetcuda_amd.so).  Plumbing only: torch is used for device memory
and streams; every compute call goes through the C-ABI.  Fails loudly if the library is missing."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "libleetcuda_amd.so"
DIAG_LIB_PATH = _PKG / "lib" / "liblc_diag.so"   # probes of include/lc_diag.h (tests / tools only)

LC_OK, LC_ERR_ARG, LC_ERR_SHAPE, LC_ERR_HEADDIM, LC_ERR_LAUNCH, LC_ERR_VENDOR, LC_ERR_DEVICE = 0, -1, -2, -3, -4, -5, -6
LAYOUT_NN, LAYOUT_TN = 0, 1
# lc_hgemm_variant (values 2, 5, 7, 8 were retired round-1 experiments: LC_ERR_ARG)
HGEMM_AUTO, HGEMM_MFMA256, HGEMM_GENERIC, HGEMM_MFMA256P2, HGEMM_MFMA128 = 0, 1, 3, 4, 6
HGEMM_VALU_NAIVE, HGEMM_VALU_SLICED_K, HGEMM_VALU_T8X8_X4, HGEMM_VALU_T16X8_K32 = 20, 21, 22, 30   # the VALU ladder: 20..30
HGEMM_MFMA256W4B, HGEMM_MFMA256W4C, HGEMM_MFMA256W4X, HGEMM_MFMA256W4Y = 9, 10, 12, 13
HGEMM_MID = 14   # the one-round kernel (hgemm_mid.hip)
HGEMM_EDGE = 15  # the vectorised edge kernel (hgemm_edge.hip): any M, N; K % 8 == 0 (NN: N % 8 == 0)
HGEMM_RAGGED = 16  # ragged M / N, K % 32 == 0, N % 8 == 0: the tiled kernels, clamped 128 x 128 tiles of the mid-size kernel on what they do not divide
HGEMM_KPAD = 17    # K % 32 != 0 on a large problem: zero-padded operand copies in the workspace + the tuned kernels
ATTN_SPLIT_Q, ATTN_SHARED_QKV, ATTN_SHARED_KV, ATTN_TILING_QK, ATTN_TILING_QKV, ATTN_SPLIT_KV = range(6)
ATTN_CAUSAL, ATTN_V_TRANSPOSED = 1, 2   # lc_attn_fwd_f16_ex / lc_attn_kernel_name_ex flags
ROPE_INTERLEAVED, ROPE_PACKED_SRC = 1, 2   # lc_rope_append_paged_* flags

# every symbol include/lc_abi.h declares: name -> (restype, argtypes)
_vp, _i, _cp, _fp, _ip = C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
SYMBOLS = {
    "lc_abi_version": (_i, []),
    "lc_status_string": (_cp, [_i]),
    "lc_device_check": (_i, [_ip]),
    "lc_build_info": (_cp, [_ip]),
    "lc_tune_set": (_i, [_cp, _i]),
    "lc_tune_get": (_i, [_cp, _ip, _ip]),
    "lc_tune_count": (_i, []),
    "lc_tune_key": (_cp, [_i]),
    "lc_tune_calibrate": (_i, [_vp, _fp]),
    "lc_workspace_release": (C.c_size_t, []),
    "lc_workspace_bytes": (C.c_size_t, []),
    "lc_hgemm_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_vendor_init": (_i, []),
    "lc_vendor_destroy": (_i, []),
    "lc_hgemm_vendor_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "lc_gemm_fp8_e4m3": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_float, _i, _vp]),
    "lc_mxfp8_pack_scales": (_i, [_vp, _vp, _i, _i, _vp]),
    "lc_gemm_mxfp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, _i, _vp]),
    "lc_hgemm_call": (_i, [_cp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_hgemm_entry_count": (_i, []),
    "lc_hgemm_entry_name": (_cp, [_i]),
    "lc_hgemm_entry_info": (_i, [_cp, _ip, _ip]),
    "lc_attn_fwd_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_attn_fwd_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "lc_attn_fwd_f16_ex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "lc_attn_fwd_f16_gqa": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_attn_decode_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_decode_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "lc_attn_decode_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_decode_paged_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_decode_paged_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "lc_attn_decode_paged_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_decode_paged_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_decode_paged_kv8_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "lc_attn_decode_paged_kv8_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_chunk_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_chunk_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "lc_attn_chunk_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_chunk_paged_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_chunk_paged_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "lc_attn_chunk_paged_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_chunk_paged_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_chunk_paged_kv8_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "lc_attn_chunk_paged_kv8_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_local_f16": (_i, [_vp] * 5 + [_i] * 7 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_local_workspace_bytes": (C.c_size_t, [_i] * 7),
    "lc_attn_local_kernel_name": (_i, [_i] * 8 + [_cp, _i]),
    "lc_attn_local_paged_f16": (_i, [_vp] * 6 + [_i] * 9 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_local_paged_workspace_bytes": (C.c_size_t, [_i] * 8),
    "lc_attn_local_paged_kernel_name": (_i, [_i] * 9 + [_cp, _i]),
    "lc_attn_local_paged_kv8": (_i, [_vp] * 8 + [_i] * 9 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_local_paged_kv8_workspace_bytes": (C.c_size_t, [_i] * 8),
    "lc_attn_local_paged_kv8_kernel_name": (_i, [_i] * 9 + [_cp, _i]),
    "lc_attn_varlen_paged_f16": (_i, [_vp] * 7 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_workspace_bytes": (C.c_size_t, [_i] * 9),
    "lc_attn_varlen_paged_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_kv8": (_i, [_vp] * 9 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_kv8_workspace_bytes": (C.c_size_t, [_i] * 9),
    "lc_attn_varlen_paged_kv8_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_kv_append_paged_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_kv_append_paged_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "lc_kv_append_paged_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_kv_append_paged_kv8_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _cp, _i]),
    "lc_rope_append_paged_f16": (_i, [_vp] * 9 + [_i] * 10 + [C.c_longlong, _i, _vp]),
    "lc_rope_append_paged_kv8": (_i, [_vp] * 11 + [_i] * 10 + [C.c_longlong, _i, _vp]),
    "lc_rope_append_paged_kernel_name": (_i, [_i] * 9 + [C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_paged_kv8_kernel_name": (_i, [_i] * 9 + [C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_f16": (_i, [_vp] * 10 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_kv8": (_i, [_vp] * 12 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_kv8_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    # the bfloat16 ragged entries: argument for argument their fp16 twins (the workspace queries above serve both)
    "lc_attn_varlen_paged_bf16": (_i, [_vp] * 7 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_kv8_bf16": (_i, [_vp] * 9 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_kv8_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_rope_append_varlen_bf16": (_i, [_vp] * 10 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_kv8_bf16": (_i, [_vp] * 12 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_bf16_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_kv8_bf16_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    # the ragged entries that also write each row's log-sum-exp: their twins with `lse` right behind O (the workspace queries above serve them)
    "lc_attn_varlen_paged_lse_f16": (_i, [_vp] * 8 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_lse_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_lse_kv8": (_i, [_vp] * 10 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_lse_kv8_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_lse_bf16": (_i, [_vp] * 8 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_lse_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_lse_kv8_bf16": (_i, [_vp] * 10 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_lse_kv8_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    # the ragged entries with a look-back visibility mask: their lse twins with `tree_mask` right behind lse (the workspace queries above serve them)
    "lc_attn_varlen_paged_tree_f16": (_i, [_vp] * 9 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_tree_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_tree_kv8": (_i, [_vp] * 11 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_tree_kv8_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_tree_bf16": (_i, [_vp] * 9 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_tree_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    "lc_attn_varlen_paged_tree_kv8_bf16": (_i, [_vp] * 11 + [_i] * 10 + [_vp, _i, _vp, C.c_size_t, _vp]),
    "lc_attn_varlen_paged_tree_kv8_bf16_kernel_name": (_i, [_i] * 10 + [_cp, _i]),
    # the ragged rope + append entries with per-token rotary positions: their twins with `pos_ids` right behind cu_q
    "lc_rope_append_varlen_pos_f16": (_i, [_vp] * 11 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_pos_kv8": (_i, [_vp] * 13 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_pos_bf16": (_i, [_vp] * 11 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_pos_kv8_bf16": (_i, [_vp] * 13 + [_i] * 11 + [C.c_longlong, C.c_longlong, _i, _vp]),
    "lc_rope_append_varlen_pos_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_pos_kv8_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_pos_bf16_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    "lc_rope_append_varlen_pos_kv8_bf16_kernel_name": (_i, [_i] * 10 + [C.c_longlong, C.c_longlong, _i, _cp, _i]),
    # merge of two (O, lse) states: Oa, lse_a, Ob, lse_b, Oout, lse_out, cu_q (or NULL), B, T, H, D, stream
    "lc_attn_merge_states_f16": (_i, [_vp] * 7 + [_i] * 4 + [_vp]),
    "lc_attn_merge_states_bf16": (_i, [_vp] * 7 + [_i] * 4 + [_vp]),
    "lc_attn_call": (_i, [_cp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "lc_attn_entry_count": (_i, []),
    "lc_attn_entry_name": (_cp, [_i]),
    "lc_attn_entry_info": (_i, [_cp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "lc_hgemm_time": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _fp]),
    "lc_attn_time": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _fp]),
    "lc_hgemm_kernel_name": (_i, [_i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_kernel_name": (_i, [_i, _i, _i, _i, _cp, _i]),
    "lc_attn_kernel_name_bh": (_i, [_i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_kernel_name_ex": (_i, [_i, _i, _i, _i, _cp, _i]),
    "lc_attn_kernel_name_gqa": (_i, [_i, _i, _i, _i, _i, _cp, _i]),
    "lc_attn_slowpath_stats": (_i, [C.POINTER(C.c_uint), _i]),
    "lc_timer_start": (_i, [_vp, C.POINTER(_vp)]),
    "lc_timer_stop": (_i, [_vp, _fp]),
    "lc_clock_probe": (_i, [_vp, _vp]),
}
# every symbol include/lc_diag.h declares (liblc_diag.so)
DIAG_SYMBOLS = {
    "lc_probe_mid256": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "lc_probe_mfma16": (_i, [_vp, _vp, _vp, _vp]),
    "lc_probe_mfma32": (_i, [_vp, _vp, _vp, _vp]),
    "lc_probe_tr16": (_i, [_vp, _vp, _vp]),
    "lc_probe_coissue": (_i, [_i, _i, _i, _vp, _vp]),
    "lc_probe_attn_mix": (_i, [_i, _i, _vp, _vp]),
    "lc_probe_mfma_form": (_i, [_i, _vp, _vp]),
    "lc_probe_mfma_war": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "lc_diag_pollute": (_i, [C.c_uint, _i, _vp]),
    "lc_diag_attn_w4i": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "lc_diag_attn_w4u_stamps": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
}

_lib = None
_diag = None


class LcError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {status_string(status)} (lc_status {status})")


def load() -> C.CDLL:
    """dlopen the C-ABI library. `import torch` first so libamdhip64.so.7 resolves to the copy PyTorch
    already mapped (one HIP runtime per process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m leetcuda_amd.build` "
            "(there is no CPU or PyTorch fallback for the HIP kernels)")
    try:
        import torch  # noqa: F401  (maps torch/lib/libamdhip64.so first)
        tl = Path(torch.__file__).parent / "lib" / "libhipblaslt.so"
        if tl.exists() and os.environ.get("LC_VENDOR_SYSTEM_HIPBLASLT", "0") != "1":
            C.CDLL(str(tl), mode=C.RTLD_GLOBAL)  # let dlopen("libhipblaslt.so.1") find PyTorch's copy
    except Exception:  # torch is optional for symbol-level use of the ABI
        pass
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def load_diag() -> C.CDLL:
    """dlopen liblc_diag.so (hardware probes; tests and tools only)."""
    global _diag
    if _diag is not None:
        return _diag
    if not DIAG_LIB_PATH.exists():
        raise RuntimeError(f"{DIAG_LIB_PATH} is missing: build it with `python -m leetcuda_amd.build`")
    import torch  # noqa: F401  (maps libamdhip64 first)
    lib = C.CDLL(str(DIAG_LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in DIAG_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _diag = lib
    return lib


def build_info():
    """(flags string, is_diag) of the loaded library."""
    d = C.c_int(0)
    return load().lc_build_info(C.byref(d)).decode(), bool(d.value)


def require_production():
    """bench.py and the parity tests refuse a LC_DIAG=1 library: its diagnosis knobs can make results WRONG."""
    info, diag = build_info()
    if diag:
        raise RuntimeError(f"libleetcuda_amd.so is a DIAGNOSIS build ({info}); rebuild with "
                           "`python -m leetcuda_amd.build --force` (LC_DIAG unset)")


def status_string(status: int) -> str:
    return load().lc_status_string(status).decode()


def check(status: int, what: str):
    if status != LC_OK:
        raise LcError(status, what)


def _ptr(t) -> int:
    return t.data_ptr()


def _stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def _shape_err(what: str):
    # the reference wrappers' message (hgemm_mma_stage.cu:2048-2057 CHECK_TORCH_TENSOR_SHAPE)
    raise RuntimeError(f"Tensor size mismatch! ({what})")


def _gemm_dims(a, b, c, layout=LAYOUT_NN, b_is_nk=False):
    """(M, N, K) after checking a [M,K], b and c [M,N] — a mismatched tensor must fail here with the reference's
    message, not as an out-of-bounds access on the device.  b: NN -> [K,N]; TN -> the reference presents a
    [K,N]-shaped tensor whose STORAGE is [N,K] (tools/utils.py:152-156), so either orientation is accepted;
    b_is_nk (fp8 entry) -> [N,K]."""
    if a.dim() != 2 or b.dim() != 2 or c.dim() != 2:
        _shape_err("2-D tensors expected")
    M, K = a.shape
    N = c.shape[1]
    if c.shape[0] != M:
        _shape_err(f"c {tuple(c.shape)} vs a {tuple(a.shape)}")
    if b_is_nk:
        ok = tuple(b.shape) == (N, K)
    elif layout == LAYOUT_TN:
        ok = tuple(b.shape) in ((K, N), (N, K))
    else:
        ok = tuple(b.shape) == (K, N)
    if not ok:
        _shape_err(f"b {tuple(b.shape)} vs K={K}, N={N}")
    return M, N, K


def _attn_dims(q, k, v, o, v_transposed=False):
    if q.dim() != 4:
        _shape_err("4-D [B,H,N,D] tensors expected")
    B, H, N, D = q.shape
    vshape = (B, H, D, N) if v_transposed else (B, H, N, D)
    if tuple(k.shape) != (B, H, N, D) or tuple(o.shape) != (B, H, N, D) or tuple(v.shape) != vshape:
        _shape_err(f"q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} o {tuple(o.shape)}")
    return B, H, N, D


def _need_gpu(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("leetcuda_amd: tensor must live on the MI355X (no CPU path)")
        if not t.is_contiguous():
            raise RuntimeError("leetcuda_amd: tensor must be contiguous")


def tune(key: str, value: int):
    check(load().lc_tune_set(key.encode(), value), f"lc_tune_set({key})")


def tune_get(key: str):
    """(current, default) of a knob."""
    v, d = C.c_int(0), C.c_int(0)
    check(load().lc_tune_get(key.encode(), C.byref(v), C.byref(d)), f"lc_tune_get({key})")
    return v.value, d.value


def tune_items():
    """{key: (current, default)} of every knob this library accepts."""
    lib = load()
    out = {}
    for i in range(lib.lc_tune_count()):
        k = lib.lc_tune_key(i)
        if k:
            out[k.decode()] = tune_get(k.decode())
    return out


def tune_calibrate():
    """Measure the split-KV rule's constants on the current device (lc_tune_calibrate).  Returns {"adopted": bool, "tau128_us", "tau64_us",
    "x0_us", "bytes_per_us"}; adopted False = the measurement was refused as implausible and the built-in constants stay."""
    out = (C.c_float * 4)()
    rc = load().lc_tune_calibrate(_stream(), out)
    if rc not in (LC_OK, LC_ERR_ARG):
        check(rc, "lc_tune_calibrate")
    return {"adopted": rc == LC_OK, "tau128_us": out[0], "tau64_us": out[1], "x0_us": out[2], "bytes_per_us": out[3]}


def workspace_bytes() -> int:
    """Bytes of internal workspace (split-KV / split-K partials) currently cached, all devices."""
    return int(load().lc_workspace_bytes())


def workspace_release() -> int:
    """hipFree every cached workspace buffer (waits for the devices); returns the bytes given back."""
    return int(load().lc_workspace_release())


def device_check() -> int:
    n = C.c_int(0)
    check(load().lc_device_check(C.byref(n)), "lc_device_check")
    return n.value


# ---- HGEMM ------------------------------------------------------------------------------------------
def hgemm(a, b, c, layout=LAYOUT_NN, variant=HGEMM_AUTO, stages=2, swizzle_stride=1):
    """c[M,N] = a[M,K] @ B ; b is [K,N] (NN) or storage [N,K] (TN). Writes c in place."""
    import torch
    _need_gpu(a, b, c)
    assert a.dtype == b.dtype == c.dtype == torch.half
    M, N, K = _gemm_dims(a, b, c, layout)
    check(load().lc_hgemm_f16(_ptr(a), _ptr(b), _ptr(c), M, N, K, layout, variant, stages, swizzle_stride,
                              _stream()), "lc_hgemm_f16")
    return c


def gemm_fp8(a8, b8_nk, c, alpha=1.0, swizzle_stride=1):
    """c[M,N] (fp16) = alpha * a8[M,K] @ b8_nk[N,K]^T; a8/b8 are torch.float8_e4m3fn (or uint8 views)."""
    _need_gpu(a8, b8_nk, c)
    M, N, K = _gemm_dims(a8, b8_nk, c, b_is_nk=True)
    check(load().lc_gemm_fp8_e4m3(_ptr(a8), _ptr(b8_nk), _ptr(c), M, N, K, float(alpha), swizzle_stride, _stream()),
          "lc_gemm_fp8_e4m3")
    return c


def mxfp8_pack_scales(s):
    """s: uint8 [rows, K/32] E8M0 block scales -> the packed array lc_gemm_mxfp8 consumes (uint8 tensor of the same size, opaque)."""
    import torch
    _need_gpu(s)
    assert s.dtype == torch.uint8 and s.dim() == 2 and s.is_contiguous()
    rows, kb = s.shape
    p = torch.empty(rows * kb, dtype=torch.uint8, device=s.device)
    check(load().lc_mxfp8_pack_scales(_ptr(s), _ptr(p), rows, kb * 32, _stream()), "lc_mxfp8_pack_scales")
    return p


def gemm_mxfp8(a8, pa, b8_nk, pb, c, alpha=1.0, swizzle_stride=1):
    """c[M,N] (fp16) = alpha * (a8 * 2^(sa-127)) @ (b8_nk * 2^(sb-127))^T with per-(row, 32 k) E8M0 scales; pa / pb = mxfp8_pack_scales(sa / sb)."""
    _need_gpu(a8, b8_nk, c, pa, pb)
    M, N, K = _gemm_dims(a8, b8_nk, c, b_is_nk=True)
    assert pa.numel() == M * K // 32 and pb.numel() == N * K // 32
    check(load().lc_gemm_mxfp8(_ptr(a8), _ptr(pa), _ptr(b8_nk), _ptr(pb), _ptr(c), M, N, K, float(alpha), swizzle_stride, _stream()),
          "lc_gemm_mxfp8")
    return c


def hgemm_call(entry: str, a, b, c, stages=2, swizzle=False, swizzle_stride=1):
    _need_gpu(a, b, c)
    lay = C.c_int(LAYOUT_NN)
    load().lc_hgemm_entry_info(entry.encode(), C.byref(lay), None)   # unknown names fail in lc_hgemm_call below
    M, N, K = _gemm_dims(a, b, c, lay.value)
    check(load().lc_hgemm_call(entry.encode(), _ptr(a), _ptr(b), _ptr(c), M, N, K, stages, int(swizzle),
                               swizzle_stride, _stream()), entry)
    return c


def hgemm_vendor(a, b, c, layout=LAYOUT_NN):
    _need_gpu(a, b, c)
    M, N, K = _gemm_dims(a, b, c, layout)
    check(load().lc_hgemm_vendor_f16(_ptr(a), _ptr(b), _ptr(c), M, N, K, layout, _stream()),
          "lc_hgemm_vendor_f16")
    return c


def vendor_init():
    check(load().lc_vendor_init(), "lc_vendor_init")


def vendor_destroy():
    check(load().lc_vendor_destroy(), "lc_vendor_destroy")


def hgemm_time(a, b, c, layout=LAYOUT_NN, variant=HGEMM_AUTO, stages=2, swizzle_stride=1, warmup=2,
               iters=10) -> float:
    """Average ms per launch, HIP events on the launch stream."""
    _need_gpu(a, b, c)
    M, N, K = _gemm_dims(a, b, c, layout)
    ms = C.c_float(0)
    check(load().lc_hgemm_time(_ptr(a), _ptr(b), _ptr(c), M, N, K, layout, variant, stages, swizzle_stride,
                               warmup, iters, _stream(), C.byref(ms)), "lc_hgemm_time")
    return ms.value


def hgemm_entries():
    lib = load()
    out = []
    for i in range(lib.lc_hgemm_entry_count()):
        name = lib.lc_hgemm_entry_name(i)
        lay, na = C.c_int(), C.c_int()
        lib.lc_hgemm_entry_info(name, C.byref(lay), C.byref(na))
        out.append((name.decode(), lay.value, na.value))
    return out


# ---- attention --------------------------------------------------------------------------------------
def attn_fwd(q, k, v, o, v_transposed=False, family=ATTN_SPLIT_Q, acc_f32=False, stages=2, causal=False):
    """causal=True: row i attends to keys j <= i (lc_attn_fwd_f16_ex; fp16, D <= 128; family / acc_f32 / stages select nothing)."""
    import torch
    _need_gpu(q, k, v, o)
    assert q.dtype == k.dtype == v.dtype == o.dtype == torch.half
    B, H, N, D = _attn_dims(q, k, v, o, v_transposed)
    if causal:
        flags = ATTN_CAUSAL | (ATTN_V_TRANSPOSED if v_transposed else 0)
        check(load().lc_attn_fwd_f16_ex(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, N, D, flags, _stream()), "lc_attn_fwd_f16_ex")
        return o
    check(load().lc_attn_fwd_f16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, N, D, int(v_transposed), family,
                                 int(acc_f32), stages, _stream()), "lc_attn_fwd_f16")
    return o


def _attn_dims_gqa(q, k, v, o, v_transposed=False):
    """q, o [B,H,N,D]; k [B,Hkv,N,D]; v [B,Hkv,N,D] or [B,Hkv,D,N]; H % Hkv == 0.  Returns B, H, Hkv, N, D."""
    if q.dim() != 4 or k.dim() != 4:
        _shape_err("4-D [B,H,N,D] / [B,Hkv,N,D] tensors expected")
    B, H, N, D = q.shape
    Hkv = k.shape[1]
    vshape = (B, Hkv, D, N) if v_transposed else (B, Hkv, N, D)
    if tuple(k.shape) != (B, Hkv, N, D) or tuple(o.shape) != (B, H, N, D) or tuple(v.shape) != vshape:
        _shape_err(f"q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} o {tuple(o.shape)}")
    if Hkv < 1 or Hkv > H or H % Hkv != 0:
        _shape_err(f"{H} query heads on {Hkv} K/V heads")
    return B, H, Hkv, N, D


def attn_fwd_gqa(q, k, v, o, v_transposed=False, causal=False):
    """Grouped-query / multi-query forward (lc_attn_fwd_f16_gqa): q, o [B,H,N,D], k / v with Hkv = k.shape[1] heads, H % Hkv == 0;
    query head h reads K / V head h // (H // Hkv).  fp16, D <= 128 when Hkv < H; Hkv == H is attn_fwd(..., causal=causal)'s call."""
    import torch
    _need_gpu(q, k, v, o)
    assert q.dtype == k.dtype == v.dtype == o.dtype == torch.half
    B, H, Hkv, N, D = _attn_dims_gqa(q, k, v, o, v_transposed)
    flags = (ATTN_CAUSAL if causal else 0) | (ATTN_V_TRANSPOSED if v_transposed else 0)
    check(load().lc_attn_fwd_f16_gqa(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, Hkv, N, D, flags, _stream()), "lc_attn_fwd_f16_gqa")
    return o


def _decode_dims(q, k, v, o, cache, kname, vname, batched):
    """What _attn_dims_decode and _attn_dims_decode_paged share: q, o [B,H,Nq,D]; k, v of one 4-D shape with Hkv at 1 and D last (batched: B first);
    H % Hkv == 0.  Returns B, H, Hkv, Nq, D."""
    if q.dim() != 4 or k.dim() != 4:
        _shape_err(f"4-D [B,H,Nq,D] / {cache} tensors expected")
    B, H, Nq, D = q.shape
    Hkv = k.shape[1]
    if k.shape[3] != D or (batched and k.shape[0] != B) or tuple(v.shape) != tuple(k.shape) or tuple(o.shape) != (B, H, Nq, D):
        _shape_err(f"q {tuple(q.shape)} {kname} {tuple(k.shape)} {vname} {tuple(v.shape)} o {tuple(o.shape)}")
    if Hkv < 1 or Hkv > H or H % Hkv != 0:
        _shape_err(f"{H} query heads on {Hkv} K/V heads")
    return B, H, Hkv, Nq, D


def _attn_dims_decode(q, k, v, o, kv_len=None):
    """q, o [B,H,Nq,D]; k, v [B,Hkv,Ncap,D] (the cache); kv_len None or int32 [B]; H % Hkv == 0.  Returns B, H, Hkv, Nq, Ncap, D."""
    B, H, Hkv, Nq, D = _decode_dims(q, k, v, o, "[B,Hkv,Ncap,D]", "k", "v", True)
    if kv_len is not None and tuple(kv_len.shape) != (B,):
        _shape_err(f"kv_len {tuple(kv_len.shape)} for batch {B}")
    return B, H, Hkv, Nq, k.shape[2], D


def _attn_dims_decode_paged(q, k_pool, v_pool, o, block_table, kv_len):
    """q, o [B,H,Nq,D]; k_pool, v_pool [num_pages,Hkv,page_size,D]; block_table int32 [B,max_pages]; kv_len int32 [B]; H % Hkv == 0.
    Returns B, H, Hkv, Nq, num_pages, page_size, max_pages, D."""
    B, H, Hkv, Nq, D = _decode_dims(q, k_pool, v_pool, o, "[num_pages,Hkv,page_size,D]", "k_pool", "v_pool", False)
    if block_table is None or block_table.dim() != 2 or block_table.shape[0] != B:
        _shape_err(f"block_table {None if block_table is None else tuple(block_table.shape)} for batch {B}")
    if kv_len is None or tuple(kv_len.shape) != (B,):
        _shape_err(f"kv_len {None if kv_len is None else tuple(kv_len.shape)} for batch {B}")
    return B, H, Hkv, Nq, k_pool.shape[0], k_pool.shape[2], block_table.shape[1], D


def _workspace_args(workspace):
    """(pointer or None, bytes) of the optional caller workspace of a decode call"""
    if workspace is None:
        return None, 0
    _need_gpu(workspace)
    return _ptr(workspace) or None, workspace.numel() * workspace.element_size()


def _decode_kernel_name(symbol, *shape, causal) -> str:
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(*shape, ATTN_CAUSAL if causal else 0, buf, 128), symbol)
    return buf.value.decode()


def attn_decode(q, k, v, o, kv_len=None, causal=False, workspace=None, *, _entry="lc_attn_decode_f16", _local=()):
    """Decode attention over a KV cache (lc_attn_decode_f16): q, o [B,H,Nq,D] fp16; k, v [B,Hkv,Ncap,D] fp16; kv_len None (= Ncap) or a
    DEVICE int32 [B] tensor of valid cache lengths, read by the kernel; causal: query i sees keys j <= kv_len[b] - Nq + i.  workspace: None or
    a device tensor of at least attn_decode_workspace_bytes(...) bytes (makes the split-KV form legal under graph capture)."""
    import torch
    _need_gpu(q, k, v, o)
    assert q.dtype == k.dtype == v.dtype == o.dtype == torch.half
    dims = _attn_dims_decode(q, k, v, o, kv_len)
    if kv_len is not None:
        _need_gpu(kv_len)
        assert kv_len.dtype == torch.int32
    check(getattr(load(), _entry)(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(kv_len) if kv_len is not None else None, *dims, *_local,
                                  ATTN_CAUSAL if causal else 0, *_workspace_args(workspace), _stream()), _entry)
    return o


def attn_decode_workspace_bytes(B, H, Hkv, Nq, Ncap, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs (0: one launch, no workspace)."""
    return int(load().lc_attn_decode_workspace_bytes(B, H, Hkv, Nq, Ncap, D))


def attn_decode_kernel_name(B, H, Hkv, Nq, Ncap, D, causal=False) -> str:
    """The kernel attn_decode runs for this shape under the current knobs: "attn_decode_kernel<D,RT>", + " xS" with S > 1 KV ranges."""
    return _decode_kernel_name("lc_attn_decode_kernel_name", B, H, Hkv, Nq, Ncap, D, causal=causal)


def attn_decode_paged(q, k_pool, v_pool, o, block_table, kv_len, causal=False, workspace=None, *, _entry="lc_attn_decode_paged_f16", _local=()):
    """Decode attention over a paged KV cache (lc_attn_decode_paged_f16): q, o [B,H,Nq,D] fp16; k_pool, v_pool [num_pages,Hkv,page_size,D]
    fp16, page_size a power of two >= 16; block_table a DEVICE int32 [B,max_pages] tensor of pool page ids; kv_len a DEVICE int32 [B] tensor;
    both are read by the kernel only (page ids are clamped to the pool there).  causal, workspace: as attn_decode."""
    import torch
    _need_gpu(q, k_pool, v_pool, o)
    assert q.dtype == k_pool.dtype == v_pool.dtype == o.dtype == torch.half
    dims = _attn_dims_decode_paged(q, k_pool, v_pool, o, block_table, kv_len)
    _need_gpu(block_table, kv_len)
    assert block_table.dtype == torch.int32 and kv_len.dtype == torch.int32
    check(getattr(load(), _entry)(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(o), _ptr(block_table), _ptr(kv_len), *dims, *_local,
                                  ATTN_CAUSAL if causal else 0, *_workspace_args(workspace), _stream()), _entry)
    return o


def attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs: those of attn_decode at Ncap = max_pages x page_size."""
    return int(load().lc_attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D))


def attn_decode_paged_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False) -> str:
    """The kernel attn_decode_paged runs for this shape under the current knobs: "attn_decode_paged_kernel<D,RT>", + " xS" with S > 1."""
    return _decode_kernel_name("lc_attn_decode_paged_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, causal=causal)


def _kv8_args(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale, v_scale):
    """The dtype and shape checks of attn_decode_paged_kv8 (no GPU needed): fp16 q / o, fp8 e4m3fn or uint8 pools, float32 [Hkv] scales or None.
    Returns _attn_dims_decode_paged's tuple."""
    import torch
    fp8 = (torch.float8_e4m3fn, torch.uint8)
    if q.dtype != torch.half or o.dtype != torch.half:
        raise TypeError(f"q / o must be float16, got {q.dtype} / {o.dtype}")
    if k_pool8.dtype not in fp8 or v_pool8.dtype not in fp8:
        raise TypeError(f"k_pool8 / v_pool8 must be float8_e4m3fn or uint8, got {k_pool8.dtype} / {v_pool8.dtype}")
    dims = _attn_dims_decode_paged(q, k_pool8, v_pool8, o, block_table, kv_len)
    if block_table.dtype != torch.int32 or kv_len.dtype != torch.int32:
        raise TypeError(f"block_table / kv_len must be int32, got {block_table.dtype} / {kv_len.dtype}")
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            continue
        if s.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {s.dtype}")
        if tuple(s.shape) != (dims[2],):
            _shape_err(f"{name} {tuple(s.shape)} for {dims[2]} K/V heads")
    return dims


def attn_decode_paged_kv8(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale=None, v_scale=None, causal=False, workspace=None, *,
                          _entry="lc_attn_decode_paged_kv8", _local=()):
    """Decode attention over a paged KV cache kept in fp8 (lc_attn_decode_paged_kv8): attn_decode_paged with k_pool8, v_pool8
    [num_pages,Hkv,page_size,D] of torch.float8_e4m3fn (or its bytes as uint8) and k_scale, v_scale DEVICE float32 [Hkv] tensors (None = 1.0):
    K = k_scale[g] K8, V = v_scale[g] V8.  The scales are read by the kernel only, like block_table and kv_len."""
    dims = _kv8_args(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale, v_scale)
    _need_gpu(q, k_pool8, v_pool8, o, block_table, kv_len, *(s for s in (k_scale, v_scale) if s is not None))
    check(getattr(load(), _entry)(_ptr(q), _ptr(k_pool8), _ptr(v_pool8), _ptr(o), _ptr(block_table), _ptr(kv_len),
                                  _ptr(k_scale) if k_scale is not None else None, _ptr(v_scale) if v_scale is not None else None,
                                  *dims, *_local, ATTN_CAUSAL if causal else 0, *_workspace_args(workspace), _stream()), _entry)
    return o


def attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs: those of attn_decode_paged for the same shape."""
    return int(load().lc_attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D))


def attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False) -> str:
    """The kernel attn_decode_paged_kv8 runs for this shape under the current knobs: "attn_decode_paged_kv8_kernel<D,RT>", + " xS" with S > 1."""
    return _decode_kernel_name("lc_attn_decode_paged_kv8_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, causal=causal)


# Chunked-prefill attention (lc_attn_chunk_*): the decode calls with R = (H / Hkv) x Nq unbounded.  The arguments and the
# Python-side checks are those of attn_decode*; R <= 64 is the decode call itself (same plan, name and bits).

def attn_chunk(q, k, v, o, kv_len=None, causal=False, workspace=None):
    """attn_decode without the bound R = (H / Hkv) x Nq <= 64 (lc_attn_chunk_f16): a chunk of Nq query tokens per sequence over a contiguous
    cache; kv_len is the length AFTER the chunk was appended, causal is bottom-right aligned."""
    return attn_decode(q, k, v, o, kv_len, causal=causal, workspace=workspace, _entry="lc_attn_chunk_f16")


def attn_chunk_workspace_bytes(B, H, Hkv, Nq, Ncap, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs (0: one launch, no workspace)."""
    return int(load().lc_attn_chunk_workspace_bytes(B, H, Hkv, Nq, Ncap, D))


def attn_chunk_kernel_name(B, H, Hkv, Nq, Ncap, D, causal=False) -> str:
    """The kernel attn_chunk runs: R > 64: "attn_chunk_kernel<D>", + " xS" with S > 1 KV ranges; R <= 64: attn_decode_kernel_name's."""
    return _decode_kernel_name("lc_attn_chunk_kernel_name", B, H, Hkv, Nq, Ncap, D, causal=causal)


def attn_chunk_paged(q, k_pool, v_pool, o, block_table, kv_len, causal=False, workspace=None):
    """attn_decode_paged without the bound on R (lc_attn_chunk_paged_f16): what follows kv_append_paged of a chunk of a prompt."""
    return attn_decode_paged(q, k_pool, v_pool, o, block_table, kv_len, causal=causal, workspace=workspace, _entry="lc_attn_chunk_paged_f16")


def attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs: those of attn_chunk at Ncap = max_pages x page_size."""
    return int(load().lc_attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D))


def attn_chunk_paged_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False) -> str:
    """R > 64: "attn_chunk_paged_kernel<D>", + " xS" with S > 1; R <= 64: attn_decode_paged_kernel_name's."""
    return _decode_kernel_name("lc_attn_chunk_paged_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, causal=causal)


def attn_chunk_paged_kv8(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale=None, v_scale=None, causal=False, workspace=None):
    """attn_decode_paged_kv8 without the bound on R (lc_attn_chunk_paged_kv8): what follows kv_append_paged_kv8 of a chunk of a prompt."""
    return attn_decode_paged_kv8(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale, v_scale, causal=causal, workspace=workspace,
                                 _entry="lc_attn_chunk_paged_kv8")


def attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D) -> int:
    """Bytes of split-KV partials the current plan of this shape needs: those of attn_chunk_paged for the same shape."""
    return int(load().lc_attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D))


def attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False) -> str:
    """R > 64: "attn_chunk_paged_kv8_kernel<D>", + " xS" with S > 1; R <= 64: attn_decode_paged_kv8_kernel_name's."""
    return _decode_kernel_name("lc_attn_chunk_paged_kv8_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, causal=causal)


# Sliding-window and attention-sink attention (lc_attn_local_*): the chunk calls with a window of W keys and a sink
# logit per query head.  window = 0 and sinks = None is the chunk call itself (same plan, name and bits).

def _local_args(q, window, sinks):
    """The checks of the two extra arguments of attn_local* (no GPU needed): window an int >= 0, sinks None or a float32 [H] tensor.  Returns
    what goes between the dims and the flags of the C call; the caller asks for the sinks' device."""
    import torch
    if not isinstance(window, int) or window < 0:
        raise ValueError(f"window must be an int >= 0, got {window!r}")
    if sinks is None:
        return window, None
    if sinks.dtype != torch.float32:
        raise TypeError(f"sinks must be float32, got {sinks.dtype}")
    if q.dim() != 4 or tuple(sinks.shape) != (q.shape[1],):
        _shape_err(f"sinks {tuple(sinks.shape)} for q {tuple(q.shape)}")
    return window, sinks


def _local_ptrs(local):
    window, sinks = local
    if sinks is not None:
        _need_gpu(sinks)
    return window, _ptr(sinks) if sinks is not None else None


def attn_local(q, k, v, o, kv_len=None, causal=False, window=0, sinks=None, workspace=None):
    """attn_chunk with a sliding window and attention sinks (lc_attn_local_f16).  window = W > 0 (causal only): the query at position
    p = kv_len[b] - Nq + i sees keys p - W < j <= p, W keys with its own (the Hugging Face `sliding_window`); 0: no low edge.  sinks: None or
    a DEVICE float32 [H] tensor of one logit per query head, in natural units (not scaled by 1 / sqrt(D)), that joins the softmax denominator
    of every row of its head and contributes no value; read by the kernel only."""
    local = _local_args(q, window, sinks)
    _need_gpu(q)
    return attn_decode(q, k, v, o, kv_len, causal=causal, workspace=workspace, _entry="lc_attn_local_f16", _local=_local_ptrs(local))


def attn_local_workspace_bytes(B, H, Hkv, Nq, Ncap, D, window=0) -> int:
    """Bytes of split-KV partials the current plan of this shape and window needs (0: one launch, no workspace); sinks do not change it."""
    return int(load().lc_attn_local_workspace_bytes(B, H, Hkv, Nq, Ncap, D, window))


def attn_local_kernel_name(B, H, Hkv, Nq, Ncap, D, causal=False, window=0) -> str:
    """The kernel attn_local runs WITHOUT sinks: window > 0: "attn_local_kernel<D,RT>" (R <= 64) / "attn_local_chunk_kernel<D>", + " xS" with
    S > 1 KV ranges; window = 0: attn_chunk_kernel_name's (with sinks: the attn_local_* kernel of the same arguments)."""
    return _decode_kernel_name("lc_attn_local_kernel_name", B, H, Hkv, Nq, Ncap, D, window, causal=causal)


def attn_local_paged(q, k_pool, v_pool, o, block_table, kv_len, causal=False, window=0, sinks=None, workspace=None):
    """attn_chunk_paged with attn_local's window and sinks (lc_attn_local_paged_f16)."""
    local = _local_args(q, window, sinks)
    _need_gpu(q)
    return attn_decode_paged(q, k_pool, v_pool, o, block_table, kv_len, causal=causal, workspace=workspace, _entry="lc_attn_local_paged_f16",
                             _local=_local_ptrs(local))


def attn_local_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D, window=0) -> int:
    """Bytes of split-KV partials the current plan of this shape and window needs: those of attn_local at Ncap = max_pages x page_size."""
    return int(load().lc_attn_local_paged_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D, window))


def attn_local_paged_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False, window=0) -> str:
    """window > 0: "attn_local_paged_kernel<D,RT>" / "attn_local_chunk_paged_kernel<D>", + " xS"; window = 0: attn_chunk_paged_kernel_name's."""
    return _decode_kernel_name("lc_attn_local_paged_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, window, causal=causal)


def attn_local_paged_kv8(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale=None, v_scale=None, causal=False, window=0, sinks=None,
                         workspace=None):
    """attn_chunk_paged_kv8 with attn_local's window and sinks (lc_attn_local_paged_kv8); the sinks are not multiplied by k_scale."""
    local = _local_args(q, window, sinks)
    _kv8_args(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale, v_scale)
    _need_gpu(q)
    return attn_decode_paged_kv8(q, k_pool8, v_pool8, o, block_table, kv_len, k_scale, v_scale, causal=causal, workspace=workspace,
                                 _entry="lc_attn_local_paged_kv8", _local=_local_ptrs(local))


def attn_local_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D, window=0) -> int:
    """Bytes of split-KV partials the current plan of this shape and window needs: those of attn_local_paged for the same shape."""
    return int(load().lc_attn_local_paged_kv8_workspace_bytes(B, H, Hkv, Nq, page_size, max_pages, D, window))


def attn_local_paged_kv8_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, causal=False, window=0) -> str:
    """window > 0: "attn_local_paged_kv8_kernel<D,RT>" / "attn_local_chunk_paged_kv8_kernel<D>", + " xS"; window = 0: the chunk call's name."""
    return _decode_kernel_name("lc_attn_local_paged_kv8_kernel_name", B, H, Hkv, Nq, page_size, max_pages, D, window, causal=causal)


def _kv_append_args(k_new, v_new, k_pool, v_pool, block_table, kv_len, k_scale=None, v_scale=None, kv8=False):
    """The dtype and shape checks of kv_append_paged / kv_append_paged_kv8 (no GPU needed): fp16 k_new, v_new [B,Hkv,Nq,D]; pools
    [num_pages,Hkv,page_size,D] of fp16 (kv8: float8_e4m3fn or uint8); int32 block_table [B,max_pages] and kv_len [B]; kv8: float32 [Hkv] scales
    or None.  Returns B, Hkv, Nq, num_pages, page_size, max_pages, D."""
    import torch
    if k_new.dtype != torch.half or v_new.dtype != torch.half:
        raise TypeError(f"k_new / v_new must be float16, got {k_new.dtype} / {v_new.dtype}")
    return _kv_append_shapes(tuple(k_new.shape), tuple(v_new.shape), k_pool, v_pool, block_table, kv_len, k_scale, v_scale, kv8)


def _kv_append_shapes(k_shape, v_shape, k_pool, v_pool, block_table, kv_len, k_scale=None, v_scale=None, kv8=False):
    """_kv_append_args behind the dtype of k_new / v_new, on their SHAPES: a packed qkv (rope_append_paged_qkv) has the rows but no tensors of them"""
    import torch
    pool_types = (torch.float8_e4m3fn, torch.uint8) if kv8 else (torch.half,)
    if k_pool.dtype not in pool_types or v_pool.dtype not in pool_types:
        raise TypeError(f"k_pool / v_pool must be {' or '.join(str(t) for t in pool_types)}, got {k_pool.dtype} / {v_pool.dtype}")
    if len(k_shape) != 4 or k_pool.dim() != 4:
        _shape_err("4-D [B,Hkv,Nq,D] / [num_pages,Hkv,page_size,D] tensors expected")
    B, Hkv, Nq, D = k_shape
    if v_shape != (B, Hkv, Nq, D) or k_pool.shape[1] != Hkv or k_pool.shape[3] != D or tuple(v_pool.shape) != tuple(k_pool.shape):
        _shape_err(f"k_new {k_shape} v_new {v_shape} k_pool {tuple(k_pool.shape)} v_pool {tuple(v_pool.shape)}")
    if block_table is None or block_table.dim() != 2 or block_table.shape[0] != B:
        _shape_err(f"block_table {None if block_table is None else tuple(block_table.shape)} for batch {B}")
    if kv_len is None or tuple(kv_len.shape) != (B,):
        _shape_err(f"kv_len {None if kv_len is None else tuple(kv_len.shape)} for batch {B}")
    if block_table.dtype != torch.int32 or kv_len.dtype != torch.int32:
        raise TypeError(f"block_table / kv_len must be int32, got {block_table.dtype} / {kv_len.dtype}")
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            continue
        if s.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {s.dtype}")
        if tuple(s.shape) != (Hkv,):
            _shape_err(f"{name} {tuple(s.shape)} for {Hkv} K/V heads")
    return B, Hkv, Nq, k_pool.shape[0], k_pool.shape[2], block_table.shape[1], D


def kv_append_paged(k_new, v_new, k_pool, v_pool, block_table, kv_len):
    """Append to a paged KV cache (lc_kv_append_paged_f16): k_new, v_new [B,Hkv,Nq,D] fp16, the rows of the Nq newest tokens of every sequence, go
    into k_pool, v_pool [num_pages,Hkv,page_size,D] fp16 through block_table (DEVICE int32 [B,max_pages]) and kv_len (DEVICE int32 [B], the
    lengths AFTER the append: what the decode call of the same step is handed).  Token i of entry b lands at position kv_len[b] - Nq + i; a
    negative position is not written (left-padded prompts), a page id outside the pool drops the token.  Returns the pools."""
    dims = _kv_append_args(k_new, v_new, k_pool, v_pool, block_table, kv_len)
    _need_gpu(k_new, v_new, k_pool, v_pool, block_table, kv_len)
    check(load().lc_kv_append_paged_f16(_ptr(k_new), _ptr(v_new), _ptr(k_pool), _ptr(v_pool), _ptr(block_table), _ptr(kv_len), *dims, 0, _stream()),
          "lc_kv_append_paged_f16")
    return k_pool, v_pool


def kv_append_paged_kv8(k_new, v_new, k_pool8, v_pool8, block_table, kv_len, k_scale=None, v_scale=None):
    """Quantise and append to a paged KV cache kept in fp8 (lc_kv_append_paged_kv8): kv_append_paged with k_pool8, v_pool8 of torch.float8_e4m3fn
    (or its bytes as uint8) and k_scale, v_scale DEVICE float32 [Hkv] tensors (None = 1.0): the code of x is e4m3fn(clamp(x / scale, +-448)),
    round to nearest even — the pools attn_decode_paged_kv8 reads with the same scales."""
    dims = _kv_append_args(k_new, v_new, k_pool8, v_pool8, block_table, kv_len, k_scale, v_scale, kv8=True)
    _need_gpu(k_new, v_new, k_pool8, v_pool8, block_table, kv_len, *(s for s in (k_scale, v_scale) if s is not None))
    check(load().lc_kv_append_paged_kv8(_ptr(k_new), _ptr(v_new), _ptr(k_pool8), _ptr(v_pool8), _ptr(block_table), _ptr(kv_len),
                                        _ptr(k_scale) if k_scale is not None else None, _ptr(v_scale) if v_scale is not None else None,
                                        *dims, 0, _stream()), "lc_kv_append_paged_kv8")
    return k_pool8, v_pool8


def kv_append_paged_kernel_name(B, Hkv, Nq, page_size, max_pages, D, kv8=False) -> str:
    """The kernel kv_append_paged (kv8: kv_append_paged_kv8) runs for this shape: "kv_append_paged_kernel<D>" / "kv_append_paged_kv8_kernel<D>"."""
    symbol = "lc_kv_append_paged_kv8_kernel_name" if kv8 else "lc_kv_append_paged_kernel_name"
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(B, Hkv, Nq, page_size, max_pages, D, 0, buf, 128), symbol)
    return buf.value.decode()


def rope_table(max_pos, rot_dim, base=10000.0):
    """The cos_sin table of plain RoPE for rope_append_paged*: float32 [max_pos, rot_dim] on the CPU, row t = cos(t w_j), j = 0 .. rot_dim/2 - 1,
    then sin(t w_j), with w_j = base^(-2j / rot_dim); the angles are computed in float64.  Scaled variants (NTK, YaRN, ...) are the caller's: any
    table of this layout is accepted."""
    import torch
    if max_pos <= 0 or rot_dim < 2 or rot_dim % 2:
        _shape_err(f"rope_table({max_pos}, {rot_dim})")
    j = torch.arange(rot_dim // 2, dtype=torch.float64)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * j / rot_dim)[None, :]
    return torch.cat([ang.cos(), ang.sin()], dim=1).to(torch.float32).contiguous()


def _rope_append_args(q, k_new, v_new, k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale=None, v_scale=None, kv8=False):
    """The dtype and shape checks of rope_append_paged / rope_append_paged_kv8 (no GPU needed): _kv_append_args' on what the append call shares,
    then fp16 q [B,H,Nq,D] with H a multiple of Hkv, float32 cos_sin [max_pos, rot_dim], q_out (if given) fp16 of q's shape.  Returns B, H, Hkv,
    Nq, num_pages, page_size, max_pages, D, rot_dim, max_pos."""
    import torch
    if k_new.dtype != torch.half or v_new.dtype != torch.half:
        raise TypeError(f"k_new / v_new must be float16, got {k_new.dtype} / {v_new.dtype}")
    if q.dtype != torch.half:
        raise TypeError(f"q must be float16, got {q.dtype}")
    return _rope_shapes(tuple(q.shape), tuple(k_new.shape), tuple(v_new.shape), k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale, v_scale, kv8)


def _rope_shapes(q_shape, k_shape, v_shape, k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale, v_scale, kv8):
    """_rope_append_args behind the dtypes of q, k_new and v_new, on their shapes (the dense and the packed call share it)"""
    import torch
    B, Hkv, Nq, P, ps, mp, D = _kv_append_shapes(k_shape, v_shape, k_pool, v_pool, block_table, kv_len, k_scale, v_scale, kv8)
    if q_out is not None and q_out.dtype != torch.half:
        raise TypeError(f"q_out must be float16, got {q_out.dtype}")
    if cos_sin.dtype != torch.float32:
        raise TypeError(f"cos_sin must be float32, got {cos_sin.dtype}")
    if len(q_shape) != 4 or q_shape[0] != B or q_shape[2] != Nq or q_shape[3] != D or q_shape[1] % Hkv != 0:
        _shape_err(f"q {q_shape} for k_new {k_shape}")
    if q_out is not None and tuple(q_out.shape) != q_shape:
        _shape_err(f"q_out {tuple(q_out.shape)} vs q {q_shape}")
    if cos_sin.dim() != 2 or cos_sin.shape[0] < 1 or cos_sin.shape[1] % 16 != 0 or not 16 <= cos_sin.shape[1] <= D:
        _shape_err(f"cos_sin {tuple(cos_sin.shape)}: [max_pos, rot_dim], rot_dim a multiple of 16 in [16, {D}]")
    return B, q_shape[1], Hkv, Nq, P, ps, mp, D, cos_sin.shape[1], cos_sin.shape[0]


def _rope_launch(src_ptrs, q_out, k_pool, v_pool, cos_sin, block_table, kv_len, k_scale, v_scale, dims, stride, flags, kv8):
    """src_ptrs: the addresses of Q, Knew and Vnew (three tensors, or three places in one packed qkv)"""
    _need_gpu(q_out, k_pool, v_pool, cos_sin, block_table, kv_len, *(s for s in (k_scale, v_scale) if s is not None))
    scale_ptrs = [_ptr(s) if s is not None else None for s in (k_scale, v_scale)] if kv8 else []
    symbol = "lc_rope_append_paged_kv8" if kv8 else "lc_rope_append_paged_f16"
    check(getattr(load(), symbol)(*src_ptrs, _ptr(q_out), _ptr(k_pool), _ptr(v_pool), _ptr(cos_sin), _ptr(block_table), _ptr(kv_len), *scale_ptrs,
                                  *dims, stride, flags, _stream()), symbol)
    return q_out


def rope_append_paged(q, k_new, v_new, k_pool, v_pool, cos_sin, block_table, kv_len, q_out=None, interleaved=False):
    """Rotary embedding fused with kv_append_paged (lc_rope_append_paged_f16), ONE launch: q [B,H,Nq,D] and k_new [B,Hkv,Nq,D] are rotated at
    position kv_len[b] - Nq + i with row min(position, max_pos - 1) of cos_sin (DEVICE float32 [max_pos, rot_dim], rope_table's layout; pairs
    (j, j + rot_dim/2), or (2j, 2j + 1) with interleaved=True; elements behind rot_dim are copied); the rotated K and the unrotated v_new go into
    the pools exactly where kv_append_paged puts them.  Returns q_out [B,H,Nq,D] (None: allocated; `q_out is q`: in place), rows of negative
    position zeroed."""
    import torch
    dims = _rope_append_args(q, k_new, v_new, k_pool, v_pool, cos_sin, block_table, kv_len, q_out)
    _need_gpu(q, k_new, v_new)
    return _rope_launch((_ptr(q), _ptr(k_new), _ptr(v_new)), torch.empty_like(q) if q_out is None else q_out, k_pool, v_pool, cos_sin, block_table, kv_len,
                        None, None, dims, 0, ROPE_INTERLEAVED if interleaved else 0, False)


def rope_append_paged_kv8(q, k_new, v_new, k_pool8, v_pool8, cos_sin, block_table, kv_len, q_out=None, interleaved=False, k_scale=None, v_scale=None):
    """rope_append_paged into fp8 pools (lc_rope_append_paged_kv8): the K code is kv_append_paged_kv8's code of the rotated row rounded to fp16,
    so the pools equal kv_append_paged_kv8 fed with what rope_append_paged wrote.  k_scale, v_scale: DEVICE float32 [Hkv] or None = 1.0."""
    import torch
    dims = _rope_append_args(q, k_new, v_new, k_pool8, v_pool8, cos_sin, block_table, kv_len, q_out, k_scale, v_scale, kv8=True)
    _need_gpu(q, k_new, v_new)
    return _rope_launch((_ptr(q), _ptr(k_new), _ptr(v_new)), torch.empty_like(q) if q_out is None else q_out, k_pool8, v_pool8, cos_sin, block_table,
                        kv_len, k_scale, v_scale, dims, 0, ROPE_INTERLEAVED if interleaved else 0, True)


def _rope_qkv_args(qkv, H, Hkv, k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale, v_scale):
    """The checks of rope_append_paged_qkv (no GPU needed): fp16 qkv [B,Nq,(H + 2 Hkv) D] whose last dim is dense and whose two outer strides
    describe ONE row stride (a row-strided view of a wider projection output is accepted); the pool dtype picks the entry.  Returns
    (dims as _rope_append_args, row stride in elements, kv8)."""
    import torch
    if qkv.dtype != torch.half:
        raise TypeError(f"qkv must be float16, got {qkv.dtype}")
    if k_pool.dtype not in (torch.half, torch.float8_e4m3fn, torch.uint8):
        raise TypeError(f"k_pool / v_pool must be float16, float8_e4m3fn or uint8, got {k_pool.dtype} / {v_pool.dtype}")
    kv8 = k_pool.dtype != torch.half
    if not kv8 and (k_scale is not None or v_scale is not None):
        raise TypeError("k_scale / v_scale belong to fp8 pools")
    if qkv.dim() != 3 or k_pool.dim() != 4 or H <= 0 or Hkv <= 0 or H % Hkv != 0:
        _shape_err(f"qkv {tuple(qkv.shape)} [B,Nq,(H + 2 Hkv) D] with H = {H}, Hkv = {Hkv}; k_pool {tuple(k_pool.shape)}")
    B, Nq, W = qkv.shape
    D = k_pool.shape[3]
    if W != (H + 2 * Hkv) * D:
        _shape_err(f"qkv {tuple(qkv.shape)}: last dim is not (H + 2 Hkv) D = {(H + 2 * Hkv) * D}")
    stride = qkv.stride(1) if Nq > 1 else (qkv.stride(0) if B > 1 else W)
    if qkv.stride(2) != 1 or stride < W or stride % 8 != 0 or (B > 1 and qkv.stride(0) != Nq * stride):
        _shape_err(f"qkv strides {tuple(qkv.stride())}: one row stride >= {W}, a multiple of 8, is expected")
    dims = _rope_shapes((B, H, Nq, D), (B, Hkv, Nq, D), (B, Hkv, Nq, D), k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale, v_scale, kv8)
    return dims, stride, kv8


def rope_append_paged_qkv(qkv, H, Hkv, k_pool, v_pool, cos_sin, block_table, kv_len, q_out=None, interleaved=False, k_scale=None, v_scale=None):
    """rope_append_paged / rope_append_paged_kv8 (the pool dtype picks the entry) straight from the QKV projection's token-major output
    (LC_ROPE_PACKED_SRC): qkv [B,Nq,(H + 2 Hkv) D] fp16 — or a row-strided view of it — holds each token's H query heads, then its Hkv key
    heads, then its Hkv value heads.  Returns q_out [B,H,Nq,D] dense (the call transposes too); q_out must not overlap qkv."""
    import torch
    dims, stride, kv8 = _rope_qkv_args(qkv, H, Hkv, k_pool, v_pool, cos_sin, block_table, kv_len, q_out, k_scale, v_scale)
    B, _, _, Nq, _, _, _, D = dims[:8]
    if not qkv.is_cuda:
        raise RuntimeError("leetcuda_amd: tensor must live on the MI355X (no CPU path)")
    if q_out is None:
        q_out = torch.empty((B, H, Nq, D), dtype=torch.half, device=qkv.device)
    base, esz = _ptr(qkv), qkv.element_size()      # three places in one buffer: the kernel strides by `stride`, so qkv need not be contiguous
    return _rope_launch((base, base + H * D * esz, base + (H + Hkv) * D * esz), q_out, k_pool, v_pool, cos_sin, block_table, kv_len, k_scale, v_scale,
                        dims, stride, ROPE_PACKED_SRC | (ROPE_INTERLEAVED if interleaved else 0), kv8)


def rope_append_paged_kernel_name(B, H, Hkv, Nq, page_size, max_pages, D, rot_dim, max_pos, interleaved=False, kv8=False, src_row_stride=0) -> str:
    """The kernel rope_append_paged (kv8: rope_append_paged_kv8; src_row_stride != 0: the packed layout of rope_append_paged_qkv) runs for this
    shape: "rope_append_paged_kernel<D,INTERLEAVED>" / "rope_append_paged_kv8_kernel<D,INTERLEAVED>"."""
    symbol = "lc_rope_append_paged_kv8_kernel_name" if kv8 else "lc_rope_append_paged_kernel_name"
    flags = (ROPE_INTERLEAVED if interleaved else 0) | (ROPE_PACKED_SRC if src_row_stride else 0)
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(B, H, Hkv, Nq, page_size, max_pages, D, rot_dim, max_pos, src_row_stride, flags, buf, 128), symbol)
    return buf.value.decode()


# Ragged-batch (varlen) attention and rotary embedding + append over the paged caches (lc_attn_varlen_paged_*, lc_rope_append_varlen_*; DESIGN.md
# section 4.3l): one continuous-batching step — sequences with different numbers of new tokens — stated once.  The tokens are packed token-major,
# q / o [T,H,D], and cu_q (DEVICE int32 [B + 1]) holds each sequence's first row; max_nq bounds every cu_q[b + 1] - cu_q[b].

def _varlen_dims(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq):
    """The shape checks of attn_varlen_paged* (no GPU needed): q, o [T,H,D]; pools [num_pages,Hkv,page_size,D]; cu_q int32 [B + 1] with B taken
    from block_table [B,max_pages]; kv_len int32 [B]; 1 <= max_nq <= T.  Returns B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D."""
    import torch
    if q.dim() != 3 or k_pool.dim() != 4:
        _shape_err("3-D [T,H,D] / 4-D [num_pages,Hkv,page_size,D] tensors expected")
    T, H, D = q.shape
    Hkv = k_pool.shape[1]
    if k_pool.shape[3] != D or tuple(v_pool.shape) != tuple(k_pool.shape) or tuple(o.shape) != (T, H, D):
        _shape_err(f"q {tuple(q.shape)} k_pool {tuple(k_pool.shape)} v_pool {tuple(v_pool.shape)} o {tuple(o.shape)}")
    if Hkv < 1 or Hkv > H or H % Hkv != 0:
        _shape_err(f"{H} query heads on {Hkv} K/V heads")
    B = _varlen_batch(cu_q, block_table, kv_len)
    if not isinstance(max_nq, int) or max_nq < 1 or max_nq > T:
        raise ValueError(f"max_nq must be an int in [1, T = {T}], got {max_nq!r}")
    return B, H, Hkv, T, max_nq, k_pool.shape[0], k_pool.shape[2], block_table.shape[1], D


def _varlen_batch(cu_q, block_table, kv_len) -> int:
    """B from block_table [B,max_pages]; cu_q int32 [B + 1], kv_len int32 [B]"""
    import torch
    if block_table is None or block_table.dim() != 2:
        _shape_err(f"block_table {None if block_table is None else tuple(block_table.shape)}: [B,max_pages] expected")
    B = block_table.shape[0]
    if kv_len is None or tuple(kv_len.shape) != (B,):
        _shape_err(f"kv_len {None if kv_len is None else tuple(kv_len.shape)} for batch {B}")
    if cu_q is None or tuple(cu_q.shape) != (B + 1,):
        _shape_err(f"cu_q {None if cu_q is None else tuple(cu_q.shape)} for batch {B}: [B + 1] expected")
    if block_table.dtype != torch.int32 or kv_len.dtype != torch.int32 or cu_q.dtype != torch.int32:
        raise TypeError(f"block_table / kv_len / cu_q must be int32, got {block_table.dtype} / {kv_len.dtype} / {cu_q.dtype}")
    return B


def _varlen_local(q, window, sinks):
    """_local_args for a token-major q [T,H,D]"""
    import torch
    if not isinstance(window, int) or window < 0:
        raise ValueError(f"window must be an int >= 0, got {window!r}")
    if sinks is None:
        return window, None
    if sinks.dtype != torch.float32:
        raise TypeError(f"sinks must be float32, got {sinks.dtype}")
    if q.dim() != 3 or tuple(sinks.shape) != (q.shape[1],):
        _shape_err(f"sinks {tuple(sinks.shape)} for q {tuple(q.shape)}")
    return window, sinks


def attn_varlen_paged(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, causal=False, window=0, sinks=None, workspace=None):
    """Attention of a ragged batch over a paged KV cache (lc_attn_varlen_paged_f16): q, o [T,H,D] fp16, token-major; sequence b owns rows
    cu_q[b] .. cu_q[b + 1] - 1 (cu_q a DEVICE int32 [B + 1] tensor, read by the kernel only and clamped there into the T rows and to max_nq
    rows a sequence); kv_len[b] is the length after the step's append, query i of sequence b sits at kv_len[b] - Nq_b + i.  Pools, block_table,
    causal, window, sinks and workspace: attn_local_paged's.  Rows at or past cu_q[B] are not written."""
    return _varlen_attn(q, k_pool, v_pool, o, False, cu_q, block_table, kv_len, max_nq, None, None, causal, window, sinks, workspace, False, False)


def attn_varlen_paged_kv8(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, k_scale=None, v_scale=None, causal=False, window=0,
                          sinks=None, workspace=None):
    """attn_varlen_paged over fp8 pools (lc_attn_varlen_paged_kv8): k_pool8, v_pool8 of torch.float8_e4m3fn (or its bytes as uint8), k_scale,
    v_scale DEVICE float32 [Hkv] or None = 1.0, as attn_local_paged_kv8."""
    return _varlen_attn(q, k_pool8, v_pool8, o, False, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, causal, window, sinks, workspace, True, False)


def attn_varlen_paged_workspace_bytes(B, H, Hkv, T, max_nq, page_size, max_pages, D, window=0, kv8=False) -> int:
    """Bytes of split-KV partials the current plan of this ragged shape needs: S x T H x (D + 1) floats, 0 for one KV range."""
    symbol = "lc_attn_varlen_paged_kv8_workspace_bytes" if kv8 else "lc_attn_varlen_paged_workspace_bytes"
    return int(getattr(load(), symbol)(B, H, Hkv, T, max_nq, page_size, max_pages, D, window))


def attn_varlen_paged_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=False, window=0, kv8=False) -> str:
    """"attn_varlen_paged_kernel<D,RT>" (G max_nq <= 64) / "attn_varlen_chunk_paged_kernel<D>" (kv8: the _kv8 kernels), + " xS" with S > 1."""
    symbol = "lc_attn_varlen_paged_kv8_kernel_name" if kv8 else "lc_attn_varlen_paged_kernel_name"
    return _decode_kernel_name(symbol, B, H, Hkv, T, max_nq, page_size, max_pages, D, window, causal=causal)


def _row_stride(t, what):
    """the row stride, in elements, of a token-major [T,heads,D] tensor whose rows are dense: a view into a wider projection output is accepted"""
    T, heads, D = t.shape
    if t.stride(2) != 1 or (heads > 1 and t.stride(1) != D):
        _shape_err(f"{what} strides {tuple(t.stride())}: rows of heads x D dense elements are expected")
    stride = t.stride(0) if T > 1 else heads * D
    if stride < heads * D or stride % 8 != 0:
        _shape_err(f"{what} strides {tuple(t.stride())}: a row stride >= {heads * D}, a multiple of 8, is expected")
    return stride


def _rope_varlen_args(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, k_scale=None, v_scale=None, kv8=False,
                      bf16=False):
    """The dtype and shape checks of rope_append_varlen / _kv8 and their _bf16 twins (no GPU needed): fp16 (bf16: bfloat16) q [T,H,D], k_new,
    v_new [T,Hkv,D] — dense, or views with one row stride each (k_new and v_new share theirs) —, pools [num_pages,Hkv,page_size,D], float32
    cos_sin [max_pos, rot_dim], q_out (if given) of q's type [T,H,D].  Returns (B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D,
    rot_dim, max_pos, q_row_stride, kv_row_stride)."""
    import torch
    elem, ename = (torch.bfloat16, "bfloat16") if bf16 else (torch.half, "float16")
    if q.dtype != elem or k_new.dtype != elem or v_new.dtype != elem:
        raise TypeError(f"q / k_new / v_new must be {ename}, got {q.dtype} / {k_new.dtype} / {v_new.dtype}")
    pool_types = (torch.float8_e4m3fn, torch.uint8) if kv8 else (elem,)
    if k_pool.dtype not in pool_types or v_pool.dtype not in pool_types:
        raise TypeError(f"k_pool / v_pool must be {' or '.join(str(t) for t in pool_types)}, got {k_pool.dtype} / {v_pool.dtype}")
    if q_out is not None and q_out.dtype != elem:
        raise TypeError(f"q_out must be {ename}, got {q_out.dtype}")
    if cos_sin.dtype != torch.float32:
        raise TypeError(f"cos_sin must be float32, got {cos_sin.dtype}")
    if q.dim() != 3 or k_new.dim() != 3 or k_pool.dim() != 4:
        _shape_err("3-D [T,H,D] / [T,Hkv,D] and 4-D [num_pages,Hkv,page_size,D] tensors expected")
    T, H, D = q.shape
    Hkv = k_pool.shape[1]
    if tuple(k_new.shape) != (T, Hkv, D) or tuple(v_new.shape) != (T, Hkv, D) or k_pool.shape[3] != D or tuple(v_pool.shape) != tuple(k_pool.shape):
        _shape_err(f"q {tuple(q.shape)} k_new {tuple(k_new.shape)} v_new {tuple(v_new.shape)} k_pool {tuple(k_pool.shape)} v_pool {tuple(v_pool.shape)}")
    if Hkv < 1 or H % Hkv != 0:
        _shape_err(f"{H} query heads on {Hkv} K/V heads")
    if q_out is not None and tuple(q_out.shape) != (T, H, D):
        _shape_err(f"q_out {tuple(q_out.shape)} vs q {tuple(q.shape)}")
    if cos_sin.dim() != 2 or cos_sin.shape[0] < 1 or cos_sin.shape[1] % 16 != 0 or not 16 <= cos_sin.shape[1] <= D:
        _shape_err(f"cos_sin {tuple(cos_sin.shape)}: [max_pos, rot_dim], rot_dim a multiple of 16 in [16, {D}]")
    B = _varlen_batch(cu_q, block_table, kv_len)
    if not isinstance(max_nq, int) or max_nq < 1 or max_nq > T:
        raise ValueError(f"max_nq must be an int in [1, T = {T}], got {max_nq!r}")
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            continue
        if not kv8:
            raise TypeError("k_scale / v_scale belong to fp8 pools")
        if s.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {s.dtype}")
        if tuple(s.shape) != (Hkv,):
            _shape_err(f"{name} {tuple(s.shape)} for {Hkv} K/V heads")
    qs, ks = _row_stride(q, "q"), _row_stride(k_new, "k_new")
    if _row_stride(v_new, "v_new") != ks:
        _shape_err(f"k_new / v_new row strides {ks} / {_row_stride(v_new, 'v_new')}: one stride for both is expected")
    if q_out is q and qs != H * D:
        _shape_err("in place (q_out is q) needs a dense q")
    return B, H, Hkv, T, max_nq, k_pool.shape[0], k_pool.shape[2], block_table.shape[1], D, cos_sin.shape[1], cos_sin.shape[0], qs, ks


def _rope_varlen_launch(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, k_scale, v_scale, kv8,
                        bf16=False, pos_ids=None):
    import torch
    args = _rope_varlen_args(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, k_scale, v_scale, kv8, bf16)
    pos = ()
    if pos_ids is not None:      # the _pos_ entries: the rotary position of every token, behind cu_q
        if pos_ids.dtype != torch.int32:
            raise TypeError(f"pos_ids must be int32, got {pos_ids.dtype}")
        if tuple(pos_ids.shape) != (q.shape[0],):
            _shape_err(f"pos_ids {tuple(pos_ids.shape)} for q {tuple(q.shape)}: [T] expected")
        pos = (pos_ids,)
    for t in (q, k_new, v_new):      # (views into a projection output are not contiguous: the kernel strides)
        if not t.is_cuda:
            raise RuntimeError("leetcuda_amd: tensor must live on the MI355X (no CPU path)")
    if q_out is None:
        q_out = torch.empty((args[3], args[1], args[8]), dtype=q.dtype, device=q.device)
    _need_gpu(q_out, k_pool, v_pool, cos_sin, cu_q, *pos, block_table, kv_len, *(s for s in (k_scale, v_scale) if s is not None))
    scale_ptrs = [_ptr(s) if s is not None else None for s in (k_scale, v_scale)] if kv8 else []
    stem = "lc_rope_append_varlen_pos_" if pos else "lc_rope_append_varlen_"
    if bf16:
        symbol = stem + ("kv8_bf16" if kv8 else "bf16")
    else:
        symbol = stem + ("kv8" if kv8 else "f16")
    check(getattr(load(), symbol)(_ptr(q), _ptr(k_new), _ptr(v_new), _ptr(q_out), _ptr(k_pool), _ptr(v_pool), _ptr(cos_sin), _ptr(cu_q),
                                  *(_ptr(t) for t in pos), _ptr(block_table), _ptr(kv_len), *scale_ptrs, *args, ROPE_INTERLEAVED if interleaved else 0,
                                  _stream()), symbol)
    return q_out


def rope_append_varlen(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out=None, interleaved=False):
    """rope_append_paged for a ragged batch (lc_rope_append_varlen_f16), ONE launch: q [T,H,D], k_new, v_new [T,Hkv,D] fp16, token-major — dense
    tensors or views into the QKV projection's output [T,(H + 2 Hkv) D], e.g. qkv[:, :H * D].view(T, H, D).  Token t of the sequence b with
    cu_q[b] <= t < cu_q[b + 1] is rotated at position kv_len[b] - Nq_b + (t - cu_q[b]) and its K and V rows go where kv_append_paged puts
    them; cu_q, max_nq and the clamps are attn_varlen_paged's.  Returns q_out [T,H,D] dense (None: allocated; `q_out is q`: in place, dense q
    only), what attn_varlen_paged reads.  A token at or past cu_q[B] writes nothing."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, None, None, False)


def rope_append_varlen_kv8(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out=None, interleaved=False,
                           k_scale=None, v_scale=None):
    """rope_append_varlen into fp8 pools (lc_rope_append_varlen_kv8): rope_append_paged_kv8's codes and scales."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, k_scale, v_scale, True)


def rope_append_varlen_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, interleaved=False, kv8=False, q_row_stride=None,
                                   kv_row_stride=None) -> str:
    """"rope_append_varlen_kernel<D,INTERLEAVED>" / "rope_append_varlen_kv8_kernel<D,INTERLEAVED>" (strides None: dense)."""
    symbol = "lc_rope_append_varlen_kv8_kernel_name" if kv8 else "lc_rope_append_varlen_kernel_name"
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, H * D if q_row_stride is None else q_row_stride,
                                  Hkv * D if kv_row_stride is None else kv_row_stride, ROPE_INTERLEAVED if interleaved else 0, buf, 128), symbol)
    return buf.value.decode()


# The bfloat16 twins of the four ragged calls (lc_attn_varlen_paged_bf16 / _kv8_bf16, lc_rope_append_varlen_bf16 / _kv8_bf16; DESIGN.md section
# 4.3m): the same shape checks through the same helpers, torch.bfloat16 wherever the twin wants torch.half.  The fp8 pools, the float32 scales,
# sinks and cos_sin table, the workspace and its size (attn_varlen_paged_workspace_bytes) are the twins'.  For bf16 pools the plain append is
# kv_append_paged on the pools' bits: a 16-bit row is copied, whatever it encodes.

def attn_varlen_paged_bf16(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, causal=False, window=0, sinks=None, workspace=None):
    """attn_varlen_paged with bfloat16 q, o [T,H,D] and bfloat16 pools (lc_attn_varlen_paged_bf16): every other argument, the clamps and the
    plan are attn_varlen_paged's."""
    return _varlen_attn(q, k_pool, v_pool, o, False, cu_q, block_table, kv_len, max_nq, None, None, causal, window, sinks, workspace, False, True)


def attn_varlen_paged_kv8_bf16(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, k_scale=None, v_scale=None, causal=False, window=0,
                               sinks=None, workspace=None):
    """attn_varlen_paged_kv8 with bfloat16 q, o (lc_attn_varlen_paged_kv8_bf16): the pools are the same e4m3 bytes under the same float32
    scales — a cache written by either element type is read by both."""
    return _varlen_attn(q, k_pool8, v_pool8, o, False, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, causal, window, sinks, workspace, True, True)


def attn_varlen_paged_bf16_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=False, window=0, kv8=False) -> str:
    """attn_varlen_paged_kernel_name's plan with the bf16 kernel in it: "attn_varlen_paged_bf16_kernel<D,RT>" / "attn_varlen_chunk_paged_bf16_kernel<D>"
    (kv8: "..._paged_kv8_bf16_kernel"), + " xS" with S > 1."""
    symbol = "lc_attn_varlen_paged_kv8_bf16_kernel_name" if kv8 else "lc_attn_varlen_paged_bf16_kernel_name"
    return _decode_kernel_name(symbol, B, H, Hkv, T, max_nq, page_size, max_pages, D, window, causal=causal)


def rope_append_varlen_bf16(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out=None, interleaved=False):
    """rope_append_varlen with bfloat16 sources, pools and q_out (lc_rope_append_varlen_bf16); cos_sin stays float32.  Returns q_out [T,H,D]
    bfloat16, what attn_varlen_paged_bf16 reads."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, None, None, False, True)


def rope_append_varlen_kv8_bf16(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out=None, interleaved=False,
                                k_scale=None, v_scale=None):
    """rope_append_varlen_bf16 into fp8 pools (lc_rope_append_varlen_kv8_bf16): the codes of the rotated row rounded to bfloat16 first."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, k_scale, v_scale, True,
                               True)


def rope_append_varlen_bf16_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, interleaved=False, kv8=False,
                                        q_row_stride=None, kv_row_stride=None) -> str:
    """"rope_append_varlen_bf16_kernel<D,INTERLEAVED>" / "rope_append_varlen_kv8_bf16_kernel<D,INTERLEAVED>" (strides None: dense)."""
    symbol = "lc_rope_append_varlen_kv8_bf16_kernel_name" if kv8 else "lc_rope_append_varlen_bf16_kernel_name"
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, H * D if q_row_stride is None else q_row_stride,
                                  Hkv * D if kv_row_stride is None else kv_row_stride, ROPE_INTERLEAVED if interleaved else 0, buf, 128), symbol)
    return buf.value.decode()


# The ragged calls that also hand back each row's log-sum-exp, the merge of two such states, and the shared-prefix (cascade) step built from
# them (lc_attn_varlen_paged_lse_*, lc_attn_merge_states_*).  lse is float32 [T,H]: row t, head h is the natural log of
# the sum of exp(score) over the keys that row saw, its sink included; -inf for a row that saw none (its O is 0).

def _lse_out(q, lse):
    """the lse tensor of a call on q [T,H,D]: float32 [T,H], allocated next to q when None"""
    import torch
    if lse is None:
        return torch.empty(tuple(q.shape[:2]), dtype=torch.float32, device=q.device)
    if lse.dtype != torch.float32:
        raise TypeError(f"lse must be float32, got {lse.dtype}")
    if q.dim() != 3 or tuple(lse.shape) != tuple(q.shape[:2]) or not lse.is_contiguous():
        _shape_err(f"lse {tuple(lse.shape)} for q {tuple(q.shape)}: contiguous [T,H] expected")
    return lse


def _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, causal, window, sinks, workspace, kv8, bf16,
                 tree=None):
    """The twelve ragged attention calls: the same checks in the same order.  lse False: a plain call (lc_attn_varlen_paged_f16 / _kv8 / _bf16 /
    _kv8_bf16), which returns o; lse None or a tensor: an lse call (`lse` behind o), which returns (o, lse); with `tree` (an int64 [T] tensor of
    look-back words) a tree call, `tree` behind lse"""
    import torch
    el, el_name = (torch.bfloat16, "bfloat16") if bf16 else (torch.half, "float16")
    fp8 = (torch.float8_e4m3fn, torch.uint8)
    if kv8:
        if q.dtype != el or o.dtype != el:
            raise TypeError(f"q / o must be {el_name}, got {q.dtype} / {o.dtype}")
        if k_pool.dtype not in fp8 or v_pool.dtype not in fp8:
            raise TypeError(f"k_pool8 / v_pool8 must be float8_e4m3fn or uint8, got {k_pool.dtype} / {v_pool.dtype}")
    elif q.dtype != el or o.dtype != el or k_pool.dtype != el or v_pool.dtype != el:
        raise TypeError(f"q / o / k_pool / v_pool must be {el_name}, got {q.dtype} / {o.dtype} / {k_pool.dtype} / {v_pool.dtype}")
    dims = _varlen_dims(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq)
    scales = ()
    if kv8:
        for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
            if s is None:
                continue
            if s.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, got {s.dtype}")
            if tuple(s.shape) != (dims[2],):
                _shape_err(f"{name} {tuple(s.shape)} for {dims[2]} K/V heads")
        scales = (_ptr(k_scale) if k_scale is not None else None, _ptr(v_scale) if v_scale is not None else None)
    local = _varlen_local(q, window, sinks)
    plain = lse is False
    outs = () if plain else (_lse_out(q, lse),)
    masks = ()
    if tree is not None:
        if tree.dtype != torch.int64:
            raise TypeError(f"tree_mask must be int64 (the bits of a uint64 word), got {tree.dtype}")
        if tuple(tree.shape) != (q.shape[0],) or not tree.is_contiguous():
            _shape_err(f"tree_mask {tuple(tree.shape)} for q {tuple(q.shape)}: contiguous [T] expected")
        masks = (tree,)
    _need_gpu(q, k_pool, v_pool, o, *outs, *masks, cu_q, block_table, kv_len, *(s for s in (k_scale, v_scale) if kv8 and s is not None))
    symbol = "lc_attn_varlen_paged_" + ("" if plain else "lse_" if tree is None else "tree_") + (("kv8_bf16" if bf16 else "kv8") if kv8 else ("bf16" if bf16 else "f16"))
    check(getattr(load(), symbol)(_ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(o), *(_ptr(t) for t in outs + masks), _ptr(cu_q), _ptr(block_table),
                                  _ptr(kv_len), *scales, *dims, *_local_ptrs(local), ATTN_CAUSAL if causal else 0, *_workspace_args(workspace),
                                  _stream()), symbol)
    return o if plain else (o, outs[0])


def attn_varlen_paged_lse(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, lse=None, causal=False, window=0, sinks=None, workspace=None):
    """attn_varlen_paged that also writes each row's log-sum-exp (lc_attn_varlen_paged_lse_f16): lse float32 [T,H] (None: allocated).  O is
    attn_varlen_paged's, bit for bit; the workspace is attn_varlen_paged_workspace_bytes'.  Returns (o, lse)."""
    return _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, None, None, causal, window, sinks, workspace, False, False)


def attn_varlen_paged_kv8_lse(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, lse=None, k_scale=None, v_scale=None, causal=False,
                              window=0, sinks=None, workspace=None):
    """attn_varlen_paged_kv8 + lse (lc_attn_varlen_paged_lse_kv8): the scores under the log are q.k k_scale / sqrt(D); v_scale does not enter."""
    return _varlen_attn(q, k_pool8, v_pool8, o, lse, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, causal, window, sinks, workspace, True, False)


def attn_varlen_paged_lse_bf16(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, lse=None, causal=False, window=0, sinks=None,
                               workspace=None):
    """attn_varlen_paged_bf16 + lse (lc_attn_varlen_paged_lse_bf16); lse stays float32."""
    return _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, None, None, causal, window, sinks, workspace, False, True)


def attn_varlen_paged_kv8_lse_bf16(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, lse=None, k_scale=None, v_scale=None, causal=False,
                                   window=0, sinks=None, workspace=None):
    """attn_varlen_paged_kv8_bf16 + lse (lc_attn_varlen_paged_lse_kv8_bf16)."""
    return _varlen_attn(q, k_pool8, v_pool8, o, lse, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, causal, window, sinks, workspace, True, True)


def attn_varlen_paged_lse_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=False, window=0, kv8=False, bf16=False) -> str:
    """attn_varlen_paged_kernel_name's (bf16: attn_varlen_paged_bf16_kernel_name's) plan with `_lse` in the kernel's name:
    "attn_varlen_paged_lse_kernel<D,RT>", "attn_varlen_chunk_paged_kv8_lse_bf16_kernel<D>", + " xS" with S > 1."""
    symbol = "lc_attn_varlen_paged_lse_" + ("kv8_" if kv8 else "") + ("bf16_" if bf16 else "") + "kernel_name"
    return _decode_kernel_name(symbol, B, H, Hkv, T, max_nq, page_size, max_pages, D, window, causal=causal)


# Tree-structured speculative decoding on the ragged calls (lc_attn_varlen_paged_tree_*, lc_rope_append_varlen_pos_*): the
# new tokens of a sequence are the nodes of a draft tree in neighbouring cache slots.  tree_mask is int64 [T], the bits of one uint64 look-back
# word per token: bit d lets the token at slot p see key p - d (d < 64; keys further back are not governed); pos_ids is int32 [T], the rotary
# position of every token.  tree_mask() and tree_positions() build both on the host from each sequence's parent array.

def attn_varlen_paged_tree(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, tree_mask, lse=None, window=0, sinks=None, workspace=None):
    """attn_varlen_paged_lse under a look-back visibility mask (lc_attn_varlen_paged_tree_f16), always causal: tree_mask DEVICE int64 [T], one word
    per token row of q; the token at cache slot p sees key j <= p (j > p - window) with d = p - j >= 64, or with bit d of its word set.  A word
    of all ones (-1) is attn_varlen_paged_lse(causal=True), bit for bit.  Plan and workspace are attn_varlen_paged's.  Returns (o, lse)."""
    return _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, None, None, True, window, sinks, workspace, False, False, tree_mask)


def attn_varlen_paged_kv8_tree(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, tree_mask, lse=None, k_scale=None, v_scale=None, window=0,
                               sinks=None, workspace=None):
    """attn_varlen_paged_tree over fp8 pools (lc_attn_varlen_paged_tree_kv8)."""
    return _varlen_attn(q, k_pool8, v_pool8, o, lse, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, True, window, sinks, workspace, True, False,
                       tree_mask)


def attn_varlen_paged_tree_bf16(q, k_pool, v_pool, o, cu_q, block_table, kv_len, max_nq, tree_mask, lse=None, window=0, sinks=None, workspace=None):
    """attn_varlen_paged_tree with bfloat16 q, o and pools (lc_attn_varlen_paged_tree_bf16); lse stays float32."""
    return _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, None, None, True, window, sinks, workspace, False, True, tree_mask)


def attn_varlen_paged_kv8_tree_bf16(q, k_pool8, v_pool8, o, cu_q, block_table, kv_len, max_nq, tree_mask, lse=None, k_scale=None, v_scale=None,
                                    window=0, sinks=None, workspace=None):
    """attn_varlen_paged_kv8_tree with bfloat16 q, o (lc_attn_varlen_paged_tree_kv8_bf16)."""
    return _varlen_attn(q, k_pool8, v_pool8, o, lse, cu_q, block_table, kv_len, max_nq, k_scale, v_scale, True, window, sinks, workspace, True, True,
                       tree_mask)


def attn_varlen_paged_tree_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=True, window=0, kv8=False, bf16=False) -> str:
    """attn_varlen_paged_lse_kernel_name's plan with `tree` in place of `lse`: "attn_varlen_paged_tree_kernel<D,RT>",
    "attn_varlen_chunk_paged_kv8_tree_bf16_kernel<D>", + " xS" with S > 1.  (causal=False: the call is refused, as the run call would be)"""
    symbol = "lc_attn_varlen_paged_tree_" + ("kv8_" if kv8 else "") + ("bf16_" if bf16 else "") + "kernel_name"
    return _decode_kernel_name(symbol, B, H, Hkv, T, max_nq, page_size, max_pages, D, window, causal=causal)


def attn_varlen_paged_kv8_tree_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=True, window=0) -> str:
    return attn_varlen_paged_tree_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal, window, kv8=True)


def attn_varlen_paged_tree_bf16_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=True, window=0) -> str:
    return attn_varlen_paged_tree_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal, window, bf16=True)


def attn_varlen_paged_kv8_tree_bf16_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal=True, window=0) -> str:
    return attn_varlen_paged_tree_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, causal, window, kv8=True, bf16=True)


def rope_append_varlen_pos(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, pos_ids, block_table, kv_len, max_nq, q_out=None, interleaved=False):
    """rope_append_varlen with the rotary position of every token stated (lc_rope_append_varlen_pos_f16): pos_ids DEVICE int32 [T]; token t is
    rotated by row clamp(pos_ids[t], 0, max_pos - 1) of cos_sin and still written to its cache slot kv_len[b] - Nq_b + i.  pos_ids = the slots
    gives rope_append_varlen's bytes."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, None, None, False,
                               False, pos_ids)


def rope_append_varlen_pos_kv8(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, pos_ids, block_table, kv_len, max_nq, q_out=None, interleaved=False,
                               k_scale=None, v_scale=None):
    """rope_append_varlen_pos into fp8 pools (lc_rope_append_varlen_pos_kv8)."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, k_scale, v_scale, True,
                               False, pos_ids)


def rope_append_varlen_pos_bf16(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, pos_ids, block_table, kv_len, max_nq, q_out=None, interleaved=False):
    """rope_append_varlen_pos with bfloat16 sources, pools and q_out (lc_rope_append_varlen_pos_bf16)."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool, v_pool, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, None, None, False,
                               True, pos_ids)


def rope_append_varlen_pos_kv8_bf16(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, pos_ids, block_table, kv_len, max_nq, q_out=None,
                                    interleaved=False, k_scale=None, v_scale=None):
    """rope_append_varlen_pos_bf16 into fp8 pools (lc_rope_append_varlen_pos_kv8_bf16)."""
    return _rope_varlen_launch(q, k_new, v_new, k_pool8, v_pool8, cos_sin, cu_q, block_table, kv_len, max_nq, q_out, interleaved, k_scale, v_scale, True,
                               True, pos_ids)


def rope_append_varlen_pos_kernel_name(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, interleaved=False, kv8=False, bf16=False,
                                       q_row_stride=None, kv_row_stride=None) -> str:
    """"rope_append_varlen_pos_kernel<D,INTERLEAVED>" / "_pos_kv8_kernel" / "_pos_bf16_kernel" / "_pos_kv8_bf16_kernel" (strides None: dense)."""
    symbol = "lc_rope_append_varlen_pos_" + ("kv8_" if kv8 else "") + ("bf16_" if bf16 else "") + "kernel_name"
    buf = C.create_string_buffer(128)
    check(getattr(load(), symbol)(B, H, Hkv, T, max_nq, page_size, max_pages, D, rot_dim, max_pos, H * D if q_row_stride is None else q_row_stride,
                                  Hkv * D if kv_row_stride is None else kv_row_stride, ROPE_INTERLEAVED if interleaved else 0, buf, 128), symbol)
    return buf.value.decode()


TREE_MAX_TOKENS = 64      # a look-back word has 64 bits: the ancestors of token i of a tree are at most i <= 63 slots back


def _tree_host(parents, cu_q):
    """(list of python ints cu_q, device of cu_q or None) after the checks tree_mask and tree_positions share"""
    import torch
    dev = cu_q.device if isinstance(cu_q, torch.Tensor) else None
    cu = [int(x) for x in (cu_q.tolist() if isinstance(cu_q, torch.Tensor) else cu_q)]
    if len(cu) != len(parents) + 1:
        raise ValueError(f"{len(parents)} sequences need {len(parents) + 1} entries of cu_q, got {len(cu)}")
    if cu[0] < 0 or any(b < a for a, b in zip(cu, cu[1:])):
        raise ValueError(f"cu_q must start at >= 0 and not decrease, got {cu}")
    for b, par in enumerate(parents):
        if par is None:
            continue
        par = [int(x) for x in par]
        if len(par) > TREE_MAX_TOKENS:
            raise ValueError(f"sequence {b}: a tree of {len(par)} tokens (at most {TREE_MAX_TOKENS} fit a 64-bit look-back word)")
        if len(par) != cu[b + 1] - cu[b]:
            raise ValueError(f"sequence {b}: {len(par)} parents for {cu[b + 1] - cu[b]} tokens")
        for i, a in enumerate(par):
            if not -1 <= a < i:
                raise ValueError(f"sequence {b}: parents[{i}] = {a} (an earlier token of the tree, or -1 for the prefix, is expected)")
    return cu, dev


def tree_mask(parents, cu_q):
    """The look-back words of a ragged batch for attn_varlen_paged_tree*: int64 [T], T = cu_q[B], on cu_q's device (a host sequence: the CPU).
    parents has one entry per sequence: None = an ordinary decoding or prefilling sequence (all ones), else the parent of each of its tokens —
    parents[i] < i an earlier token of the tree, -1 the prefix; at most 64 tokens (ValueError).  Bit d of row i is set iff token i - d is i
    itself or an ancestor of i, or d > i (the prefix).  Rows in front of cu_q[0] are all ones.  No kernel runs."""
    import torch
    cu, dev = _tree_host(parents, cu_q)
    words = [-1] * cu[-1]
    for b, par in enumerate(parents):
        if par is None:
            continue
        for i in range(len(par)):
            w = (~0 << (i + 1)) & 0xFFFFFFFFFFFFFFFF     # the prefix: every key more than i slots back
            a = i
            while a >= 0:
                w |= 1 << (i - a)
                a = int(par[a])
            words[cu[b] + i] = w - (1 << 64) if w >> 63 else w     # the same bits as a signed 64-bit value
    out = torch.tensor(words, dtype=torch.int64)
    return out.to(dev) if dev is not None else out


def tree_positions(parents, cu_q, kv_len):
    """The rotary positions of a ragged batch for rope_append_varlen_pos*: int32 [T], T = cu_q[B], on cu_q's device.  kv_len[b] is the length
    AFTER the step's append.  A tree sequence (parents as tree_mask's): (kv_len[b] - Nq_b) + depth of token i, a child of the prefix having depth
    0; an ordinary sequence (None): the token's cache slot kv_len[b] - Nq_b + i.  Rows in front of cu_q[0] are 0.  No kernel runs."""
    import torch
    cu, dev = _tree_host(parents, cu_q)
    lens = [int(x) for x in (kv_len.tolist() if isinstance(kv_len, torch.Tensor) else kv_len)]
    if len(lens) != len(parents):
        raise ValueError(f"{len(parents)} sequences need {len(parents)} entries of kv_len, got {len(lens)}")
    pos = [0] * cu[-1]
    for b, par in enumerate(parents):
        nq = cu[b + 1] - cu[b]
        depth = []
        for i in range(nq):
            depth.append(i if par is None else (0 if int(par[i]) < 0 else depth[int(par[i])] + 1))
            pos[cu[b] + i] = lens[b] - nq + depth[i]
    out = torch.tensor(pos, dtype=torch.int32)
    return out.to(dev) if dev is not None else out


def attn_merge_states(o_a, lse_a, o_b, lse_b, out=None, lse_out=None, cu_q=None):
    """Merge two attention states over disjoint key sets (lc_attn_merge_states_f16 / _bf16, picked by o_a's dtype; float32 O is refused):
    o_a, o_b [T,H,D] float16 or bfloat16, lse_a, lse_b float32 [T,H].  out / lse_out: where the merged state goes — None allocates, and either
    may BE an input (in place).  cu_q: None = every row, or the DEVICE int32 [B + 1] offsets of the ragged calls: only the rows of tokens
    cu_q[0] .. cu_q[B] - 1 (clamped into the T rows) are read and written.  A side whose lse is -inf contributes nothing and the other passes
    through bit for bit; both -inf give O = 0, lse = -inf.  Returns (out, lse_out)."""
    import torch
    if o_a.dtype not in (torch.half, torch.bfloat16):
        raise TypeError(f"o_a / o_b must be float16 or bfloat16, got {o_a.dtype}")
    out = torch.empty_like(o_a) if out is None else out
    if o_b.dtype != o_a.dtype or out.dtype != o_a.dtype:
        raise TypeError(f"o_a / o_b / out must share one 16-bit dtype, got {o_a.dtype} / {o_b.dtype} / {out.dtype}")
    if o_a.dim() != 3 or tuple(o_b.shape) != tuple(o_a.shape) or tuple(out.shape) != tuple(o_a.shape):
        _shape_err(f"o_a {tuple(o_a.shape)} o_b {tuple(o_b.shape)} out {tuple(out.shape)}: one [T,H,D] expected")
    if not (o_a.is_contiguous() and o_b.is_contiguous() and out.is_contiguous()):
        _shape_err("o_a / o_b / out must be contiguous")
    lse_a, lse_b, lse_out = _lse_out(o_a, lse_a), _lse_out(o_a, lse_b), _lse_out(o_a, lse_out)
    T, H, D = o_a.shape
    B = 1
    if cu_q is not None:
        if cu_q.dtype != torch.int32:
            raise TypeError(f"cu_q must be int32, got {cu_q.dtype}")
        if cu_q.dim() != 1 or cu_q.shape[0] < 2:
            _shape_err(f"cu_q {tuple(cu_q.shape)}: [B + 1] expected")
        B = cu_q.shape[0] - 1
    _need_gpu(o_a, lse_a, o_b, lse_b, out, lse_out, *(() if cu_q is None else (cu_q,)))
    symbol = "lc_attn_merge_states_bf16" if o_a.dtype == torch.bfloat16 else "lc_attn_merge_states_f16"
    check(getattr(load(), symbol)(_ptr(o_a), _ptr(lse_a), _ptr(o_b), _ptr(lse_b), _ptr(out), _ptr(lse_out), None if cu_q is None else _ptr(cu_q),
                                  B, T, H, D, _stream()), symbol)
    return out, lse_out


def attn_cascade_paged(q, k_pool, v_pool, o, cu_groups, prefix_table, prefix_len, cu_q, block_table, kv_len, max_nq_prefix, max_nq, *, sinks=None,
                       scratch, k_scale=None, v_scale=None, workspaces=(None, None)):
    """One shared-prefix (cascade) attention step over a paged cache, as three library calls on the current stream and no host sync (the whole
    step is graph-capturable):
      1. prefix level — non-causal, window 0, no sinks: prefix group g is ONE ragged "sequence" that owns the tokens cu_groups[g] ..
         cu_groups[g + 1] - 1 (the new tokens of every sequence behind that prefix, which are therefore contiguous in q) and reads the
         prefix_len[g] keys of prefix_table[g] once per 64 query rows instead of once per sequence;  -> scratch (o_prefix, lse_prefix)
      2. suffix level — causal, the ragged call of the step on the PRIVATE keys only: block_table / kv_len hold each sequence's pages and
         length behind the prefix (new tokens included); `sinks` goes here and only here;  -> (o, lse)
      3. merge, in place into (o, lse), on the rows of cu_q.
    q, o [T,H,D] float16 or bfloat16; the pools 16-bit of q's dtype, or fp8 (float8_e4m3fn / uint8) with k_scale / v_scale float32 [Hkv].
    cu_groups int32 [Gp + 1], prefix_table int32 [Gp, pages], prefix_len int32 [Gp], cu_q int32 [B + 1], block_table int32 [B, pages], kv_len
    int32 [B]: all DEVICE tensors, read by the kernels only.  max_nq_prefix bounds the tokens of a group, max_nq those of a sequence.
    scratch = (o_prefix [T,H,D] of q's dtype, lse_prefix float32 [T,H], lse float32 [T,H]): the caller's buffers — nothing is allocated here.
    workspaces: optional split-KV workspaces of the two levels (attn_varlen_paged_workspace_bytes of each level's shape); under capture a level
    without one runs one KV range.
    Caveats.  The prefix must end on a page boundary of the caller's tables (the suffix table starts with a fresh page: a page belongs to one
    level).  A sliding window does not compose with the cascade (the window's lower edge would cut through the levels): there is none.  A
    sink is one more score of a row and must join exactly ONE level: here the suffix.  Every token of cu_q must lie in a group — a sequence
    without a shared prefix is a group of prefix_len 0 (lse -inf: the suffix passes through bit for bit).  Returns (o, lse)."""
    import torch
    if not isinstance(scratch, (tuple, list)) or len(scratch) != 3:
        raise TypeError("scratch must be (o_prefix, lse_prefix, lse)")
    o_p, lse_p, lse = scratch
    kv8 = k_pool.dtype in (torch.float8_e4m3fn, torch.uint8)
    if q.dtype not in (torch.half, torch.bfloat16):
        raise TypeError(f"q must be float16 or bfloat16, got {q.dtype}")
    if sinks is not None and not torch.is_tensor(sinks):
        raise TypeError("sinks must be a float32 tensor or None")
    bf16 = q.dtype == torch.bfloat16
    ks, vs = (k_scale, v_scale) if kv8 else (None, None)
    _varlen_attn(q, k_pool, v_pool, o_p, lse_p, cu_groups, prefix_table, prefix_len, max_nq_prefix, ks, vs, False, 0, None, workspaces[0], kv8, bf16)
    _varlen_attn(q, k_pool, v_pool, o, lse, cu_q, block_table, kv_len, max_nq, ks, vs, True, 0, sinks, workspaces[1], kv8, bf16)
    return attn_merge_states(o, lse, o_p, lse_p, out=o, lse_out=lse, cu_q=cu_q)


def attn_fwd_bf16(q, k, v, o):
    """bfloat16 forward for D in {256, 512} (BASELINE config 5 extension)."""
    import torch
    _need_gpu(q, k, v, o)
    assert q.dtype == k.dtype == v.dtype == o.dtype == torch.bfloat16
    B, H, N, D = _attn_dims(q, k, v, o)
    check(load().lc_attn_fwd_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, N, D, _stream()), "lc_attn_fwd_bf16")
    return o


def attn_call(entry: str, q, k, v, o, stages=2):
    _need_gpu(q, k, v, o)
    vt = C.c_int(0)
    load().lc_attn_entry_info(entry.encode(), None, C.byref(vt), None, None, None, None)
    B, H, N, D = _attn_dims(q, k, v, o, bool(vt.value))
    check(load().lc_attn_call(entry.encode(), _ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, N, D, stages,
                              _stream()), entry)
    return o


def attn_time(q, k, v, o, v_transposed=False, family=ATTN_SPLIT_Q, stages=2, warmup=1, iters=5) -> float:
    _need_gpu(q, k, v, o)
    B, H, N, D = _attn_dims(q, k, v, o, v_transposed)
    ms = C.c_float(0)
    check(load().lc_attn_time(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, N, D, int(v_transposed), family,
                              stages, warmup, iters, _stream(), C.byref(ms)), "lc_attn_time")
    return ms.value


def attn_entries():
    lib = load()
    out = []
    for i in range(lib.lc_attn_entry_count()):
        name = lib.lc_attn_entry_name(i)
        v = [C.c_int() for _ in range(6)]
        lib.lc_attn_entry_info(name, *[C.byref(x) for x in v])
        out.append((name.decode(),) + tuple(x.value for x in v))
    return out


# ---- measurement ------------------------------------------------------------------------------------
class Timer:
    """HIP events on the launch stream around any sequence of ABI launches (lc_timer_start / lc_timer_stop)."""

    def __enter__(self):
        self._t = C.c_void_p()
        check(load().lc_timer_start(_stream(), C.byref(self._t)), "lc_timer_start")
        self.ms = None
        return self

    def __exit__(self, et, ev, tb):
        ms = C.c_float(0)
        rc = load().lc_timer_stop(self._t, C.byref(ms))
        if et is None:
            check(rc, "lc_timer_stop")
            self.ms = ms.value
        return False


def hgemm_kernel_name(M, N, K, layout=LAYOUT_NN, variant=HGEMM_AUTO) -> str:
    buf = C.create_string_buffer(128)
    check(load().lc_hgemm_kernel_name(M, N, K, layout, variant, buf, 128), "lc_hgemm_kernel_name")
    return buf.value.decode()


def attn_slowpath_stats(reset=True):
    """[executions, sum of half-tile indices, non-finite, last offending row sum (float)] of attn_w4n's overflow slow path."""
    import struct
    out = (C.c_uint * 4)()
    check(load().lc_attn_slowpath_stats(out, int(reset)), "lc_attn_slowpath_stats")
    return [out[0], out[1], out[2], struct.unpack("f", struct.pack("I", out[3]))[0]]


def attn_kernel_name(N, D, v_transposed=False, bf16=False, bh=None, causal=False, group=1) -> str:
    """The kernel the dispatcher picks for sequence length N and head dim D; bh = batch x heads of the launch (None: a grid that fills
    the GPU — the choice depends on it for D = 256 only); causal=True: the kernel of attn_fwd(..., causal=True); group = H / Hkv > 1:
    the kernel of attn_fwd_gqa (bh counts QUERY heads)."""
    buf = C.create_string_buffer(128)
    if group != 1:
        assert not bf16, "grouped-query attention is fp16 only"
        flags = (ATTN_CAUSAL if causal else 0) | (ATTN_V_TRANSPOSED if v_transposed else 0)
        check(load().lc_attn_kernel_name_gqa(int(bh) if bh else -1, int(group), N, D, flags, buf, 128), "lc_attn_kernel_name_gqa")
        return buf.value.decode()
    if causal:
        assert not bf16, "causal attention is fp16 only"
        flags = ATTN_CAUSAL | (ATTN_V_TRANSPOSED if v_transposed else 0)
        check(load().lc_attn_kernel_name_ex(int(bh) if bh else -1, N, D, flags, buf, 128), "lc_attn_kernel_name_ex")
        return buf.value.decode()
    check(load().lc_attn_kernel_name_bh(int(bh) if bh else -1, N, D, int(v_transposed), int(bf16), buf, 128), "lc_attn_kernel_name_bh")
    return buf.value.decode()


def clock_probe(out_u64x2):
    """Enqueue the {shader cycles, 100 MHz ticks} probe on the current stream (out: int64 cuda tensor of 2)."""
    check(load().lc_clock_probe(_ptr(out_u64x2), _stream()), "lc_clock_probe")
