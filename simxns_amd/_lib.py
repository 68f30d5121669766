"""ctypes binding of libsimx_hip.so (C ABI declared in include/simx.h).

This is the reference-side stub a maintainer adds: torch supplies
device pointers (`tensor.data_ptr()`) and the current HIP stream; everything else is
plain C.  There is NO fallback: if the shared library is missing the import of any
op fails loudly (the product path must never run on a CPU / eager substitute).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsimx_hip.so")

SIMX_F32, SIMX_BF16, SIMX_F16, SIMX_F32_SPLIT_H, SIMX_F32_SPLIT_B = 0, 1, 2, 3, 4
EPI_NONE, EPI_GELU, EPI_DGELU = 0, 1, 2
LOSS_KL, LOSS_WIKI, LOSS_CEKD, LOSS_CE, LOSS_CE_LOGIT, LOSS_CE_DKD, LOSS_CE_PROB = 0, 1, 2, 3, 4, 5, 6
KD_SOFTMAX, KD_LOGIT, KD_DKD, KD_BI_LOGIT = 0, 1, 2, 3
SIMX_SQNORM_WS_FLOATS = 2048       # floats of scratch simx_sqnorm_accum_det takes (include/simx.h)
(P_WORD, P_POS, P_TYPE, P_EMB_LN_G, P_EMB_LN_B, P_WQKV, P_BQKV, P_WO, P_BO, P_LN1_G, P_LN1_B,
 P_W1, P_B1, P_W2, P_B2, P_LN2_G, P_LN2_B, P_POOL_W, P_POOL_B) = range(19)


class SimxError(RuntimeError):
    pass


class BertCfg(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("layers", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32),
                ("inter", C.c_int32), ("vocab", C.c_int32), ("max_pos", C.c_int32), ("type_vocab", C.c_int32),
                ("eps", C.c_float), ("hidden_dropout", C.c_float), ("attn_dropout", C.c_float), ("dropout_seed", C.c_uint32),
                ("cls_only_last_layer", C.c_int32), ("grad_checkpoint", C.c_int32), ("qkv_layout", C.c_int32),
                ("f32_gemm", C.c_int32), ("stream_lo", C.c_int32), ("grad_scale", C.c_void_p)]


class Dropout(C.Structure):
    _fields_ = [("p", C.c_float), ("seed", C.c_uint32), ("stream", C.c_uint32)]


class LossParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("scale", C.c_float), ("temperature", C.c_float), ("adv_lambda", C.c_float),
                ("ce_w", C.c_float), ("kd_w", C.c_float), ("grad_accum", C.c_float), ("dkd_alpha", C.c_float),
                ("dkd_beta", C.c_float)]


class LeadSlot(C.Structure):
    _fields_ = [("a", C.c_float), ("b", C.c_float), ("w", C.c_float), ("x", C.c_float), ("reweight", C.c_int32)]


LEAD_MAX_SLOTS = 32                # SIMX_LEAD_MAX_SLOTS (include/simx.h)

_p, _i, _f, _d, _z, _l = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_long
_cfgp, _lpp, _dp = C.POINTER(BertCfg), C.POINTER(LossParams), C.POINTER(Dropout)

# name -> (restype, argtypes); every symbol of include/simx.h
SIGNATURES = {
    "simx_version": (_i, []),
    "simx_set_compute_cus": (_i, [_i]),
    "simx_last_error": (C.c_char_p, []),
    "simx_gemm_nt": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _p, _p, _i, _i, _p, _i, _p, _i]),
    "simx_gemm_nt_ex": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _p, _p, _i, _i, _p, _i, _p, _i, _dp]),
    "simx_embed_ln_fwd_ex": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _dp]),
    "simx_embed_ln_bwd_ex": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp]),
    "simx_ln_bwd_ex": (_i, [_p, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp]),
    "simx_ln_bwd_keyed": (_i, [_p, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp, _p]),
    "simx_mha_fwd_ex": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _dp]),
    "simx_mha_bwd_ex": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _dp]),
    "simx_mha_cls_fwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _dp]),
    "simx_mha_cls_bwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _dp]),
    "simx_gemm_tn_workspace_bytes": (_z, [_i, _i, _i]),
    "simx_gemm_tn": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _i, _p, _z]),
    "simx_gemm_tn_bias": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _i, _p, _z, _p]),
    "simx_colsum": (_i, [_p, _i, _i, _i, _p, _i, _p, _i]),
    "simx_cast_weight": (_i, [_p, _p, _i, _i, _p, _p]),
    "simx_transpose_cast": (_i, [_p, _i, _p, _i, _i, _p, _p]),
    "simx_gemm_f32_strided": (_i, [_p, _i, _i, _i, _p, _l, _l, _p, _l, _l, _p, _i, _i]),
    "simx_gemm_f32_strided_ws": (_i, [_p, _i, _i, _i, _p, _l, _l, _p, _l, _l, _p, _i, _i, _p, _z]),
    "simx_embed_ln_fwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p]),
    "simx_embed_ln_bwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p]),
    "simx_embed_ln_bwd_seq": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _p]),
    "simx_ln_fwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _f, _p]),
    "simx_ln_bwd": (_i, [_p, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _p]),
    "simx_mha_fwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p]),
    "simx_mha_bwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p]),
    "simx_cls_gather": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    "simx_cls_scatter": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
    "simx_rows_copy": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "simx_drop_residual_rows": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _dp, _p]),
    "simx_bert_param_count": (_z, [_cfgp]),
    "simx_bert_param_offset": (_z, [_cfgp, _i, _i]),
    "simx_bert_wcache_bytes": (_z, [_cfgp]),
    "simx_bert_act_bytes": (_z, [_cfgp, _i, _i, _i]),
    "simx_bert_bwd_scratch_bytes": (_z, [_cfgp, _i, _i]),
    "simx_bert_cast_weights": (_i, [_p, _cfgp, _p, _p]),
    "simx_bert_fwd": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _i, _p, _p]),
    "simx_bert_bwd": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _z]),
    "simx_bert_bwd_ex": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p, _z]),
    "simx_bert_bwd_range": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p, _z, _i, _i]),
    "simx_bert_fwd_taps": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _i, _p, _p, C.POINTER(C.c_int32), _i, _p]),
    "simx_bert_bwd_taps": (_i, [_p, _cfgp, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p, _z, _i, _i, C.POINTER(C.c_int32), _i, _p]),
    "simx_cls_rows_add_gs": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "simx_seq_mean_fwd":(_i, [_p, _i, _i, _i, _p, _p, _p]),
    "simx_seq_mean_bwd": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    "simx_sim_loss_fwd_bwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _lpp, _p, _p, _p, _p]),
    "simx_gemm_hm_ok": (_i, [_i, _i, _i]),
    "simx_gemm_nt_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _p, _p, _i, _dp, _i, _i]),
    "simx_gemm_nt_pb": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _p, _p, _i, _i, _p, _i, _dp, _i, _i]),
    "simx_gemm_tn_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _i, _p, _z, _p]),
    "simx_mha_fwd_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _dp, _i]),
    "simx_mha_bwd_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _dp, _i]),
    "simx_mha_cls_fwd_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _dp, _i]),
    "simx_mha_cls_bwd_hm": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _dp, _i]),
    "simx_scores_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "simx_scores_nll_fwd_bwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _f, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _z]),
    "simx_scores_kd_fwd_bwd": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _f, _f, _f, _f, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _z]),
    "simx_scores_kd_type_fwd_bwd": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _p, _p, _p, _p, _p,
                                         _p, _z]),
    "simx_lead_scores_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i, _i]),
    "simx_lead_scores_fwd_bwd": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _f, _f, C.POINTER(LeadSlot), _i, _f, _i, _i, _i, _i,
                                      _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _z]),
    "simx_gemm_f32_workspace_bytes": (_z, [_i, _i, _i]),
    "simx_assemble_batch": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "simx_ip_scores": (_i, [_p, _i, _i, _i, _p, _p, _p, C.c_long]),
    "simx_topk_update": (_i, [_p, _i, _i, _p, C.c_long, _p, C.c_long, C.c_int64, _i, _p, _p]),
    "simx_flat_ip_workspace_bytes": (_z, [_i, _i]),
    "simx_flat_ip_search": (_i, [_p, _i, C.c_long, _i, _p, _p, C.c_int64, _i, _i, _p, _z, _p, _p]),
    "simx_ip_scores_f16": (_i, [_p, _i, _i, _i, _p, _p, _p, C.c_long]),
    "simx_flat_ip_search_f16": (_i, [_p, _i, C.c_long, _i, _p, _p, C.c_int64, _i, _i, _p, _z, _p, _p]),
    "simx_flat_ip_fused_workspace_bytes": (_z, [_i, _i, _i]),
    "simx_ip_filter_f16": (_i, [_p, _i, _i, _i, _p, _p, C.c_int64, _i, _p, _p, _p, _p, _i, _p]),
    "simx_topk_fold_lists": (_i, [_p, _i, _p, _p, _i, _p, _i, _p, _p, _p]),
    "simx_flat_ip_search_f16_fused": (_i, [_p, _i, C.c_long, _i, _p, _p, C.c_int64, _i, _i, _i, _i, _p, _z, _p, _p, _p]),
    "simx_ip_scores_planes": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, C.c_long]),
    "simx_ip_filter_planes": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, C.c_int64, _i, _p, _p, _p, _p, _i, _p]),
    "simx_flat_ip_search_planes": (_i, [_p, _i, C.c_long, _i, _p, _p, _p, _p, C.c_int64, _i, _i, _p, _z, _p, _p]),
    "simx_flat_ip_search_planes_fused": (_i, [_p, _i, C.c_long, _i, _p, _p, _p, _p, C.c_int64, _i, _i, _i, _i, _p, _z, _p, _p, _p]),
    "simx_mine_negatives": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "simx_simans_sample": (_i, [_p, _i, _i, _i, _p, _p, _i, _d, _d, _d, C.c_uint64, C.c_uint32, _p, _p, _p, _p]),
    "simx_sqnorm_accum": (_i, [_p, _p, _z, _p]),
    "simx_sqnorm_accum_det": (_i, [_p, _p, _z, _p, _p]),
    "simx_adamw_step": (_i, [_p, _p, _p, _p, _p, _z, _f, _f, _f, _f, _f, _i, _p, _f, _f, _i]),
    "simx_gemm_tn_gs": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p, _i, _i, _p, _z, _p, _i, _p]),
    "simx_colsum_gs": (_i, [_p, _i, _i, _i, _p, _i, _p, _i, _p]),
    "simx_ln_bwd_gs": (_i, [_p, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp, _p, _p]),
    "simx_embed_ln_bwd_seq_gs": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp, _p]),
    "simx_cls_scatter_gs": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "simx_rows_copy_gs": (_i, [_p, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "simx_seq_mean_bwd_gs": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "simx_ln_fwd_res": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p]),
    "simx_ln_bwd_res": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _dp, _p, _p]),
    "simx_embed_ln_fwd_lo": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _dp]),
    "simx_stream_rows": (_i, [_p, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "simx_scaler_init": (_i, [_p, _p, _f, _f, _f]),
    "simx_scaler_update": (_i, [_p, _p, _p]),
    "simx_deterministic": (_i, []),
    "simx_adamw_step_sc": (_i, [_p, _p, _p, _p, _p, _z, _f, _f, _f, _f, _f, _i, _p, _f, _f, _i, _p]),
    "simx_lamb_chunk": (_i, []),
    "simx_lamb_plan_check": (_i, [_p, _i, _p, _p, _i, _z]),
    "simx_lamb_step": (_i, [_p, _p, _p, _p, _p, _z, _p, _i, _p, _p, _i, _p, _p, _f, _d, _d, _f, _p, _f, _f, _i, _p]),
    "simx_gemm_nt_planes_ok": (_i, [_i, _i, _i]),
    "simx_gemm_nt_planes": (_i, [_p, _i, _i, _i, _i, _i, _p, _i, _l, _p, _i, _l, _p, _i, _p, _p, _i, _p, _i, _l, _dp]),
    "simx_gemm_nt_planes_cs": (_i, [_p, _i, _i, _i, _i, _i, _p, _i, _l, _p, _i, _l, _p, _i, _p, _p, _i, _p, _i, _l, _dp, _p, _i]),
    "simx_gemm_tn_planes_workspace_bytes": (_z, [_i, _i, _i]),
    "simx_gemm_tn_planes": (_i, [_p, _i, _i, _i, _p, _i, _l, _p, _i, _l, _p, _i, _i, _p, _z, _p]),
    "simx_planes_from": (_i, [_p, _i, _i, _i, _i, _p, _i, _l, _p, _i, _l]),
    "simx_split_weight": (_i, [_p, _p, _i, _i, _p, _p, _p]),
    "simx_planes_join": (_i, [_p, _i, _i, _i, _p, _i, _l, _p, _i]),
    "simx_ln_fwd_planes": (_i, [_p, _i, _i, _p, _p, _p, _f, _p, _p, _l]),
    "simx_ln_bwd_planes": (_i, [_p, _i, _i, _p, _p, _f, _p, _p, _p, _l, _p, _p, _p, _dp]),
    "simx_embed_ln_fwd_planes": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _l, _dp]),
    "simx_mha_planes_ok": (_i, [_i, _i]),
    "simx_mha_fwd_planes": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _l, _p, _dp]),
    "simx_mha_bwd_planes": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p, _l, _p, _p, _p, _l, _dp]),
    "simx_mha_x3_ok": (_i, [_i, _i]),
    "simx_mha_fwd_x3": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _l, _p, _l, _p, _dp]),
    "simx_mha_bwd_x3": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _l, _p, _l, _p, _p, _p, _l, _dp]),
    "simx_mha_bwd_x3_bias": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _l, _p, _l, _p, _p, _p, _l, _dp, _p]),
    "simx_prof_begin": (_i, [_i]),
    "simx_prof_end": (_i, [_p, _p, _p]),
    "simx_prof_kernel_count": (_i, []),
}
# "gemm_nt_p3" = the persistent NT launches (gemm_nt_p3_kernel and gemm_nt_p5_kernel); "gemm_tn5_tn2" = the large wgrad launches (gemm_tn5_kernel or
# gemm_tn2_kernel + the slab pass; records taken before round 6's last commit call this slot "gemm_tn2")
PROF_NAMES = ["gemm_nt", "gemm_tn", "mha_fwd", "mha_bwd", "ln_fwd", "ln_bwd", "embed_fwd", "embed_bwd", "colsum", "cast",
              "loss", "sampler", "adamw", "other", "collate", "topk", "gemm_nt_p3", "gemm_tn5_tn2", "gemm_nt_xp", "gemm_tn_xp"]

_lib = None


def load():
    """Load the shared library (once).  Raises SimxError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SimxError("libsimx_hip.so not found at %s -- build it with simxns_amd/csrc/build.sh "
                        "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = header/library drift: let it surface
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().simx_last_error().decode("utf8", "replace")
        raise SimxError("%s failed (%d): %s" % (what or "simx call", rc, msg))


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero status."""
    check(getattr(load(), name)(*args), name)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())
