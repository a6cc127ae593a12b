"""ctypes binding of ``libhydra_mp.so`` (C ABI declared in ``include/hydra_mp.h``).

There is deliberately no fallback: if the shared library is missing, or no gfx950 device is
visible, :func:`load` / :func:`require_device` raise and every model/op built on them fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# HMP_LIB selects another build of the same ABI (the profiling variant libhydra_mp_kt.so from `make KTIME=1`)
LIB_PATH = os.environ.get("HMP_LIB") or os.path.join(HERE, "libhydra_mp.so")

MAX_NODE_TYPES, MAX_EDGE_TYPES, MAX_LAYERS, MAX_CONVS = 8, 16, 8, 16
N_KCLASS = 14
# slot 13 ("chain", the removed graph-local launch) is retired and always 0
KCLASS_NAMES = ["plan", "pack", "gemm_fwd", "aggregate_fwd", "loss", "aggregate_bwd", "gemm_bwd", "grad_reduce",
                "adam", "gat_fwd", "gat_bwd", "pool", "front", "chain"]
CONV_SAGE, CONV_GAT = 0, 1
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2


class Plan(C.Structure):
    _fields_ = [
        ("n_src", C.c_int32), ("n_dst", C.c_int32), ("n_edges", C.c_int64),
        ("d_rowptr", C.c_void_p), ("d_col", C.c_void_p), ("d_eid", C.c_void_p),
        ("d_t_rowptr", C.c_void_p), ("d_t_col", C.c_void_p), ("d_t_pos", C.c_void_p),
    ]


class GatArgs(C.Structure):
    _fields_ = [
        ("heads", C.c_int32), ("channels", C.c_int32), ("self_loops", C.c_int32),
        ("edge_dim", C.c_int32), ("dropout_p", C.c_float),
        ("seed", C.c_uint64), ("rng_stream", C.c_uint32), ("rng_step", C.c_uint32),
    ]


class ConvSpec(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("edge_type", C.c_int32), ("src", C.c_int32), ("dst", C.c_int32),
        ("f_out", C.c_int32), ("heads", C.c_int32), ("concat", C.c_int32), ("self_loops", C.c_int32),
        ("edge_dim", C.c_int32), ("fill_mean", C.c_int32), ("shared_lin", C.c_int32), ("active", C.c_int32),
        ("agg_first", C.c_int32), ("att_dropout", C.c_float),
        ("w0", C.c_int64), ("w1", C.c_int64), ("w2", C.c_int64), ("a0", C.c_int64), ("a1", C.c_int64),
        ("a2", C.c_int64), ("b0", C.c_int64),
    ]


class LayerSpec(C.Structure):
    _fields_ = [
        ("n_convs", C.c_int32), ("act", C.c_int32), ("dropout", C.c_float), ("group_mean", C.c_int32),
        ("out_dim", C.c_int32 * MAX_NODE_TYPES),
        ("passthrough", C.c_int32 * MAX_NODE_TYPES),
        ("convs", ConvSpec * MAX_CONVS),
    ]


class NetSpec(C.Structure):
    _fields_ = [
        ("n_node_types", C.c_int32), ("n_edge_types", C.c_int32), ("n_layers", C.c_int32),
        ("in_dim", C.c_int32 * MAX_NODE_TYPES),
        ("edge_src", C.c_int32 * MAX_EDGE_TYPES), ("edge_dst", C.c_int32 * MAX_EDGE_TYPES),
        ("readout_type", C.c_int32), ("pool_edge_type", C.c_int32), ("aux_readout_type", C.c_int32),
        ("n_params", C.c_int64), ("n_active_params", C.c_int64),
        ("layers", LayerSpec * MAX_LAYERS),
        ("tail_act", C.c_int32), ("tail_dropout", C.c_float),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32 * MAX_NODE_TYPES),
        ("d_x", C.c_void_p * MAX_NODE_TYPES),
        ("ldx", C.c_int32 * MAX_NODE_TYPES),
        ("n_edges", C.c_int64 * MAX_EDGE_TYPES),
        ("d_edge_index", C.c_void_p * MAX_EDGE_TYPES),
        ("d_edge_attr", C.c_void_p * MAX_EDGE_TYPES),
        ("n_out", C.c_int32),
        ("d_labels", C.c_void_p),
        ("plan_valid", C.c_int32),
        ("d_node_ptr", C.c_void_p * MAX_NODE_TYPES),
        ("n_graphs", C.c_int32),
        ("max_graph_nodes", C.c_int32),
        ("d_edge_ptr", C.c_void_p * MAX_EDGE_TYPES),
    ]


class TrainArgs(C.Structure):
    _fields_ = [
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
        ("ignored_label", C.c_int64), ("seed", C.c_uint64), ("training", C.c_int32), ("d_step", C.c_void_p),
    ]


class HeadTargets(C.Structure):
    _fields_ = [("d_labels", C.c_void_p * 2), ("d_mask", C.c_void_p * 2)]


class LinearHeads(C.Structure):
    _fields_ = [("F", C.c_int32), ("classes", C.c_int32 * 2), ("w_off", C.c_int64 * 2), ("b_off", C.c_int64 * 2)]


class LinearHeadTargets(C.Structure):
    _fields_ = [("d_labels", C.c_void_p), ("d_mask", C.c_void_p), ("d_member", C.c_void_p * 2)]


class CollateItem(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("d_ptr", C.c_void_p), ("src_total", C.c_int64), ("row_bytes", C.c_int64),
                ("slot", C.c_int32), ("slot_src", C.c_int32), ("slot_dst", C.c_int32)]


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("H", C.c_void_p), ("Cadd", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
        ("ldh", C.c_int32), ("ldadd", C.c_int32), ("trans_a", C.c_int32), ("trans_b", C.c_int32),
        ("n_real", C.c_int32), ("aug_ones", C.c_int32), ("slab_stride", C.c_int64),
        ("epi", C.c_int32), ("act", C.c_int32), ("drop_p", C.c_float),
        ("a_bf16", C.c_int32), ("b_bf16", C.c_int32), ("c_bf16", C.c_int32), ("h_bf16", C.c_int32),
    ]


EPOCH_STOP, EPOCH_EMPTY_VAL, EPOCH_MAX_SEGS = 1, 2, 64


class EpochCtl(C.Structure):
    _fields_ = [("loss_acc", C.c_double), ("weight_acc", C.c_double), ("max_val_acc", C.c_double),
                ("epoch", C.c_int32), ("best_epoch", C.c_int32), ("early_stop_step", C.c_int32), ("status", C.c_int32)]


class EpochRow(C.Structure):
    _fields_ = [("loss", C.c_double), ("val_acc", C.c_double), ("correct", C.c_int64), ("total", C.c_int64),
                ("improved", C.c_int32), ("pad_", C.c_int32)]


class EpochSeg(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("bytes", C.c_int64)]


class TailDesc(C.Structure):
    _fields_ = [
        ("z", C.c_void_p), ("labels", C.c_void_p), ("mask", C.c_void_p), ("grad", C.c_void_p), ("row_lv", C.c_void_p),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("t_rowptr", C.c_void_p), ("t_col", C.c_void_p), ("dpool", C.c_void_p),
        ("ldz", C.c_int32), ("n_rows", C.c_int32), ("classes", C.c_int32), ("ldg", C.c_int32), ("slot", C.c_int32),
        ("n_pool", C.c_int32), ("ldp", C.c_int32),
        ("rng_step", C.c_uint32), ("rng_stream", C.c_uint32), ("p", C.c_float), ("seed", C.c_uint64),
    ]


class LinearHeadsDesc(C.Structure):
    _fields_ = [
        ("z", C.c_void_p), ("W", C.c_void_p * 2), ("bias", C.c_void_p * 2), ("labels", C.c_void_p), ("mask", C.c_void_p),
        ("member", C.c_void_p * 2), ("grad", C.c_void_p), ("row_lv", C.c_void_p), ("slabs", C.c_void_p),
        ("slab_stride", C.c_int64), ("ignored", C.c_int64), ("seed", C.c_uint64),
        ("ldz", C.c_int32), ("n_rows", C.c_int32), ("F", C.c_int32), ("classes", C.c_int32 * 2), ("act", C.c_int32),
        ("ldg", C.c_int32), ("ld_slab", C.c_int32),
        ("rng_step", C.c_uint32), ("rng_stream", C.c_uint32), ("p", C.c_float),
    ]


class PlanJob(C.Structure):
    _fields_ = [
        ("d_edge_index", C.c_void_p), ("plan", Plan), ("d_degf", C.c_void_p),
        ("d_dst_ptr", C.c_void_p), ("d_src_ptr", C.c_void_p), ("d_edge_ptr", C.c_void_p),
        ("n_graphs", C.c_int32), ("d_scratch", C.c_void_p),
    ]


FRONT_MAX_PROB, FRONT_MAX_SEG, FRONT_MAX_SRC = 4, 6, 6
PACK_SUM, PACK_HEADS, PACK_ATTDOT, PACK_ATTDOT_T = range(4)


class FrontSeg(C.Structure):
    _fields_ = [("col0", C.c_int32), ("rows", C.c_int32), ("nsrc", C.c_int32), ("ld", C.c_int32), ("off", C.c_uint32 * FRONT_MAX_SRC)]


class FrontProb(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("C", C.c_void_p),
        ("lda", C.c_int32), ("ldc", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("n_seg", C.c_int32),
        ("seg", FrontSeg * FRONT_MAX_SEG),
    ]


class PackSeg(C.Structure):
    _fields_ = [
        ("dst", C.c_int64),
        ("rows", C.c_int32), ("rows_pad", C.c_int32), ("cols", C.c_int32), ("ld_dst", C.c_int32), ("ld_src", C.c_int32),
        ("nsrc", C.c_int32), ("kind", C.c_int32), ("H", C.c_int32), ("C", C.c_int32), ("Cp", C.c_int32),
        ("att", C.c_int64), ("src", C.c_int64 * 6), ("dst_t", C.c_int64),
        ("ld_dst_t", C.c_int32), ("col_t", C.c_int32), ("pad_t", C.c_int32),
    ]


_STRUCTS = [Plan, GatArgs, ConvSpec, LayerSpec, NetSpec, Batch, TrainArgs, HeadTargets, LinearHeads, LinearHeadTargets, GemmDesc,
            EpochCtl, EpochRow, EpochSeg, TailDesc, LinearHeadsDesc, PlanJob, FrontSeg, FrontProb, PackSeg]

_VP, _I32, _I64, _F32, _U64, _U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64, C.c_uint32

# name -> (restype, argtypes).  Kept in the order of include/hydra_mp.h; tests/test_abi.py checks that
# every function the header declares is listed here and exported by the library.
SIGNATURES = {
    "hmp_abi_version": (C.c_int, []),
    "hmp_last_error": (C.c_char_p, []),
    "hmp_sizeof": (C.c_size_t, [C.c_int]),
    "hmp_device_count": (C.c_int, []),
    "hmp_plan_scratch_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "hmp_plan_build": (C.c_int, [_VP, Plan, _VP, _VP, _VP]),
    "hmp_plan_build_many": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "hmp_segment_mean_fwd": (C.c_int, [_VP, _I32, _I32, Plan, _VP, _I32, _VP]),
    "hmp_segment_mean_bwd": (C.c_int, [_VP, _I32, _I32, Plan, _VP, _I32, _VP]),
    "hmp_gemm_f32": (C.c_int, [_VP, _I32, _I32, _VP, _I32, _I32, _VP, _I32, _I32, _I32, _I32, _VP]),
    "hmp_gemm_bf16": (C.c_int, [_VP, _I32, _I32, _VP, _I32, _I32, _VP, _I32, _I32, _I32, _I32, _VP]),
    "hmp_gemm_bf16_a16": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "hmp_net_set_compute": (C.c_int, [_VP, _I32]),
    "hmp_collate_rows": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, _I32, C.c_int64, _VP, _VP]),
    "hmp_collate_edges": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _I32, C.c_int64, _VP, _VP]),
    "hmp_gat_fwd": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _VP, _VP, Plan, GatArgs, _VP, _VP, _VP, _I32, _VP]),
    "hmp_gat_bwd": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _VP, _I32, _VP, _VP, Plan, GatArgs, _VP, _VP, _VP, _VP, _VP,
                              _VP, _I32, _VP, _I32, _VP, _I32, _VP]),
    "hmp_gat_attention": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _VP, _VP, Plan, GatArgs, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "hmp_saliency_seed": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _VP, _I32, _VP, _I32, _I32, _VP, _I32, _VP]),
    "hmp_saliency_scores": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _I32, _I32, C.POINTER(_I32), C.POINTER(_I32), _VP, _VP, _VP, _VP]),
    "hmp_saliency_topk": (C.c_int, [Plan, _VP, _I32, _I32, _VP, _I32, _VP, _I32, _VP, _VP, _VP]),
    "hmp_masked_ce": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I64, _VP, _I32, _VP, _VP]),
    "hmp_masked_ce_weighted": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I64, _VP, _VP, _I32, _VP, _VP]),
    "hmp_label_counts": (C.c_int, [_VP, _I64, _VP, _I64, _I32, _VP, _VP]),
    "hmp_balanced_class_weights": (C.c_int, [_VP, _I32, _VP, _VP]),
    "hmp_argmax_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "hmp_count_correct_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I64, _VP, _VP, _VP]),
    "hmp_count_correct_rows_by_graph": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I64, _VP, _I32, _VP, _VP]),
    "hmp_predict_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    "hmp_topk_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _VP, _VP, _VP]),
    "hmp_mc_acc_ld": (_I32, [_I32]),
    "hmp_mc_accumulate_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _VP, _I32, _VP]),
    "hmp_mc_finish": (C.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP]),
    "hmp_adam_flat": (C.c_int, [_VP, _VP, _VP, _VP, _I64, _F32, _F32, _F32, _F32, _F32, _I32, _VP, _VP]),
    "hmp_dropout_mask": (C.c_int, [_U64, _U32, _U32, _F32, _I32, _I32, _VP, _VP]),
    "hmp_head_tails": (C.c_int, [C.POINTER(TailDesc), _I32, _I32, _I32, _I64, _VP, _VP, _VP]),
    "hmp_head_tails_weighted": (C.c_int, [C.POINTER(TailDesc), _I32, C.POINTER(_VP), _I32, _I32, _I64, _VP, _VP, _VP]),
    "hmp_head_tails_predict": (C.c_int, [C.POINTER(TailDesc), _I32, _I32, _I32, C.POINTER(_VP), _VP]),
    "hmp_head_tails_topk": (C.c_int, [C.POINTER(TailDesc), _I32, _I32, _I32, _I32, C.POINTER(_VP), C.POINTER(_VP), _VP]),
    "hmp_head_tails_mc": (C.c_int, [C.POINTER(TailDesc), _I32, _I32, _I32, _I32, C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_linear_heads_mc": (C.c_int, [C.POINTER(LinearHeadsDesc), _I32, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32), _VP]),
    "hmp_linear_heads_run": (C.c_int, [C.POINTER(LinearHeadsDesc), _I32, _VP, _VP, C.POINTER(_I32), _VP]),
    "hmp_linear_heads_run_weighted": (C.c_int, [C.POINTER(LinearHeadsDesc), C.POINTER(_VP), _I32, _VP, _VP, C.POINTER(_I32), _VP]),
    "hmp_linear_heads_predict": (C.c_int, [C.POINTER(LinearHeadsDesc), C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_linear_heads_topk": (C.c_int, [C.POINTER(LinearHeadsDesc), _I32, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_net_create": (C.c_int, [C.POINTER(NetSpec), C.POINTER(_VP)]),
    "hmp_net_destroy": (None, [_VP]),
    "hmp_net_workspace_bytes": (C.c_size_t, [_VP, C.POINTER(_I32), C.POINTER(_I64)]),
    "hmp_net_bind_workspace": (C.c_int, [_VP, _VP, C.c_size_t, C.POINTER(_I32), C.POINTER(_I64)]),
    "hmp_net_forward": (C.c_int, [_VP, C.POINTER(Batch), _VP, _I32, _U64, _U32, C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_net_backward": (C.c_int, [_VP, _VP, _I32, _VP, _VP, C.POINTER(_VP), _VP]),
    "hmp_net_aux_output": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32)]),
    "hmp_net_backward2": (C.c_int, [_VP, _VP, _I32, _VP, _I32, _VP, _VP, C.POINTER(_VP), _VP]),
    "hmp_net_step_fwd_bwd": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_step_adam": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_step_fused": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_step2_fwd_bwd": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(HeadTargets), _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_step2_fused": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(HeadTargets), _VP, _VP, _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_count_correct2": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(HeadTargets), _VP, _VP, _VP]),
    "hmp_net_set_linear_heads": (C.c_int, [_VP, C.POINTER(LinearHeads)]),
    "hmp_net_set_head_pools": (C.c_int, [_VP, _I32, _I32]),
    "hmp_net_set_class_weights": (C.c_int, [_VP, _I32, _VP, _I32]),
    "hmp_net_step_heads_fwd_bwd": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(LinearHeadTargets), _VP, _VP, C.POINTER(TrainArgs), _VP]),
    "hmp_net_step_heads_fused": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(LinearHeadTargets), _VP, _VP, _VP, _VP,
                                           C.POINTER(TrainArgs), _VP]),
    "hmp_net_count_correct_heads": (C.c_int, [_VP, C.POINTER(Batch), C.POINTER(LinearHeadTargets), _VP, _VP, _VP]),
    "hmp_net_count_correct_rooms": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _I64, _VP, _VP, _VP]),
    "hmp_net_count_correct_rooms_by_graph": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _I64, _VP, _VP]),
    "hmp_net_predict_rooms": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _VP, _VP]),
    "hmp_net_predict2": (C.c_int, [_VP, C.POINTER(Batch), _VP, C.POINTER(_VP), _VP]),
    "hmp_net_predict_heads": (C.c_int, [_VP, C.POINTER(Batch), _VP, C.POINTER(_VP), C.POINTER(_VP), _VP]),
    "hmp_net_topk_rooms": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _I32, _VP, _VP, _VP]),
    "hmp_net_topk2": (C.c_int, [_VP, C.POINTER(Batch), _VP, _I32, C.POINTER(_VP), C.POINTER(_VP), _VP]),
    "hmp_net_topk_heads": (C.c_int, [_VP, C.POINTER(Batch), _VP, C.POINTER(_VP), _I32, C.POINTER(_VP), C.POINTER(_VP), _VP]),
    "hmp_net_mc_rooms": (C.c_int, [_VP, C.POINTER(Batch), _VP, _VP, _U64, _U32, _I32, _VP, _I32, _VP]),
    "hmp_net_mc2": (C.c_int, [_VP, C.POINTER(Batch), _VP, _U64, _U32, _I32, C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_net_mc_heads": (C.c_int, [_VP, C.POINTER(Batch), _VP, C.POINTER(_VP), _U64, _U32, _I32, C.POINTER(_VP), C.POINTER(_I32), _VP]),
    "hmp_net_attention": (C.c_int, [_VP, C.POINTER(Batch), _VP, _I32, C.POINTER(_VP), _I32, C.POINTER(_VP), C.POINTER(_VP), _VP]),
    "hmp_net_input_gradient": (C.c_int, [_VP, C.POINTER(Batch), _VP, _I32, _VP, _I32, _VP, _I32, _VP, _I32, _I32, C.POINTER(_VP), _VP]),
    "hmp_net_plan": (C.c_int, [_VP, _I32, C.POINTER(Plan)]),
    "hmp_net_hidden":(C.c_int, [_VP, _I32, _I32, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)]),
    "hmp_net_read_state": (C.c_int, [_VP, C.POINTER(_I32), C.POINTER(_I32), _VP]),
    "hmp_graph_begin": (C.c_int, [_VP]),
    "hmp_graph_end": (C.c_int, [_VP, C.POINTER(_VP)]),
    "hmp_graph_launch": (C.c_int, [_VP, _VP]),
    "hmp_graph_destroy": (None, [_VP]),
    "hmp_timer_create": (C.c_int, [C.POINTER(_VP)]),
    "hmp_timer_start": (C.c_int, [_VP, _VP]),
    "hmp_timer_stop": (C.c_int, [_VP, _VP]),
    "hmp_timer_elapsed_ms": (C.c_int, [_VP, C.POINTER(_F32)]),
    "hmp_timer_destroy": (None, [_VP]),
    "hmp_net_profile": (C.c_int, [_VP, _I32]),
    "hmp_net_profile_read": (C.c_int, [_VP, C.POINTER(_F32), C.POINTER(_I32)]),
    "hmp_object_edges_count": (C.c_int, [_VP, _VP, _VP, _I32, C.c_double, C.c_double, C.c_double, _VP, _VP, _VP]),
    "hmp_object_edges_fill": (C.c_int, [_VP, _VP, _VP, _I32, C.c_double, C.c_double, C.c_double, _VP, _VP, _I32, _VP]),
    "hmp_gcn_norm": (C.c_int, [Plan, _VP, _VP]),
    "hmp_segment_wsum": (C.c_int, [_VP, _I32, _I32, Plan, _I32, _VP, _VP, _VP, _I32, _VP]),
    "hmp_bias_act_drop_fwd": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _F32, _U64, _U32, _U32, _VP, _I32, _VP]),
    "hmp_bias_act_drop_bwd": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _I32, _I32, _F32, _VP, _I32, _VP]),
    "hmp_colsum": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "hmp_rowdot_sum": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _I32, _VP, _VP]),
    "hmp_batchnorm_fwd": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _F32, _F32, _I32, _VP, _I32, _VP, _VP]),
    "hmp_batchnorm_bwd": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _VP, _I32, _VP, _VP, _VP]),
    "hmp_collator_create": (C.c_int, [_I32, C.POINTER(_VP), _I64, _I32, C.POINTER(CollateItem), C.POINTER(_VP)]),
    "hmp_collator_run": (C.c_int, [_VP, _VP, _I32, C.POINTER(_VP), C.POINTER(_I64), C.POINTER(_I64), _VP, _I32, _VP]),
    "hmp_collator_set_label_filter": (C.c_int, [_VP, _I32, _VP, _I64]),
    "hmp_collator_destroy": (None, [_VP]),
    "hmp_htree_build": (C.c_int, [_I32, _I32, _VP, _I64, _VP, _I64, _VP, _I64, C.POINTER(_VP)]),
    "hmp_htree_sizes": (C.c_int, [_VP, C.POINTER(_I32), C.POINTER(_I64), C.POINTER(_I64)]),
    "hmp_htree_fill": (C.c_int, [_VP, _VP, _VP, C.POINTER(_VP), C.POINTER(_VP)]),
    "hmp_htree_destroy": (None, [_VP]),
    "hmp_gemm_bf16_dx": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _F32, _VP, _I32, _I32, _I32, _I32, _VP]),
    "hmp_gemm_bf16_dw": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _VP, _I32, _I32, _VP, _I32, _I64, _I32, C.POINTER(_I32), _I32, _I32, _I32, _VP]),
    "hmp_seg_mean_rows": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _VP, _I32, _VP]),
    "hmp_seg_mean_rows_t": (C.c_int, [_VP, _I32, _I32, _VP, _VP, _VP, _I32, _VP, _I32, _I32, _I32, _I32, _F32, _VP, _I32, _I32, _VP]),
    "hmp_gemm_bf16_dx_gather": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _F32, _VP, _I32, _I32, _I32, _I32,
                                          _VP, _VP, _VP, _VP, _I32, _VP, _VP]),
    "hmp_gemm_grouped": (C.c_int, [C.POINTER(GemmDesc), _I32, _I32, _I32, _I32, C.POINTER(_I32), _VP]),
    "hmp_front_run": (C.c_int, [_VP, _I32, _VP, _I64, _VP, _I32, _VP, _I64, _VP, _VP, _VP]),
    "hmp_pack_run": (C.c_int, [_VP, _I32, _I32, _VP, _I64, _VP, _I64, _VP, _VP, _VP]),
    "hmp_comm_unique_id": (C.c_int, [_VP]),
    "hmp_comm_create": (C.c_int, [_VP, _I32, _I32, C.POINTER(_VP)]),
    "hmp_comm_destroy": (None, [_VP]),
    "hmp_comm_query": (C.c_int, [_VP, C.POINTER(_I32), C.POINTER(_I32)]),
    "hmp_comm_allreduce_sum_f32": (C.c_int, [_VP, _VP, _I64, _VP]),
    "hmp_comm_broadcast_f32": (C.c_int, [_VP, _VP, _I64, _I32, _VP]),
    "hmp_epoch_accumulate": (C.c_int, [_VP, _VP, _VP, _VP, C.c_double, _VP]),
    "hmp_epoch_close": (C.c_int, [_VP, _VP, _I32, _VP, _I32, C.c_double, _I32, _I32, _VP, _I32, _I32, _VP]),
    "hmp_epoch_restore": (C.c_int, [_VP, _I32, _I32, _VP]),
    "hmp_epoch_read": (C.c_int, [_VP, _VP, _I32, C.POINTER(EpochCtl), C.POINTER(EpochRow), C.POINTER(_I32), _VP]),
    "hmp_epoch_read_status": (C.c_int, [_VP, C.POINTER(_I32), _VP]),
    "hmp_frame_build": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, C.c_double, C.c_double, C.c_double, _I32, _I32, _I32, _I32,
                                  _I32, C.POINTER(_VP)]),
    "hmp_frame_build_homogeneous": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, C.c_double, C.c_double, C.c_double, _I32, _I32, _I32,
                                              _I32, _I32, C.POINTER(_VP)]),
    "hmp_frame_build_flags": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, C.c_double, C.c_double, C.c_double, _I32, _I32, _I32, _I32,
                                        _I32, _I32, _I32, C.POINTER(_VP)]),
    "hmp_frame_sizes": (C.c_int, [_VP, _VP]),
    "hmp_frame_host_arrays": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "hmp_frame_pack": (C.c_int, [_VP, _VP, _I64]),
    "hmp_frame_destroy": (None, [_VP]),
    "hmp_frame_expand": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "hmp_frame_batch_build": (C.c_int, [_I32, _VP, _I32, _VP, C.POINTER(_VP)]),
    "hmp_frame_batch_items_needed": (C.c_int, [_VP, _I32, _I32, C.POINTER(_I32), C.POINTER(_I32)]),
    "hmp_frame_batch_sizes": (C.c_int, [_VP, _VP]),
    "hmp_frame_batch_host_arrays": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "hmp_frame_batch_pack": (C.c_int, [_VP, _VP, _I64]),
    "hmp_frame_batch_destroy": (None, [_VP]),
    "hmp_frame_expand_batch": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "hmp_store_count_kept": (C.c_int, [_VP, _VP, _I32, C.c_uint64, _VP, _VP]),
    "hmp_store_derive": (C.c_int, [_VP, _I32, _I32, _I32, _VP]),
    "hmp_store_node_split": (C.c_int, [_VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "hmp_store_member_counts": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP]),
}

# include/hydra_mp.h section 14: indices of hmp_frame_sizes, words of an item of the staging block's table
FS_KEPT, FS_DROPPED, FS_ROOMS, FS_E_OO, FS_E_RR, FS_STAGING_BYTES, FS_ARENA_BYTES, FS_ITEMS, FS_BLOCKS = range(9)
FS_HT_COUNTS, FS_HT_EDGES, FS_HT_INIT, FS_COUNT = 9, 13, 23, 26
FRAME_ITEM_WORDS = 12
FI_KIND, FI_TENSOR, FI_ROWS, FI_WIDTH, FI_DST, FI_S0, FI_S1, FI_S2, FI_S3, FI_P0, FI_P1, FI_BLOCK0 = range(12)
FK_FEAT, FK_POS, FK_I64, FK_EDGE, FK_EATTR, FK_CLIQUE, FK_EDGE_SEG, FK_CONST, FK_EATTR_HT = range(9)
FRAME_NO_ROOM_EDGES = 1  # hmp_frame_build_flags: the room layer loses its edges (remove_room_edges_in_dsg)
FRAME_RELPOS_HTREE = 2  # value of hmp_frame_build's relative_pos: relative positions on the edges of an H-tree
FRAME_END_WORDS, FE_DIRECT, FE_GATHER, FE_CLIQUE = 4, 0, 1, 2  # an end of an FK_EATTR_HT item's descriptor section
FT_HTREE, FT_COUNT = 16, 45
FT_HOMOG, FT_HOMOG_COUNT = 45, 9  # the tensors of a homogeneous frame (hmp_frame_build_homogeneous)
# batches of frames (hmp_frame_batch_*): forms, limits, indices of hmp_frame_batch_sizes, the tensors a batch adds
FB_COLLATED, FB_STORE = 0, 1
FRAME_MAX_ITEMS, FRAME_BATCH_MAX_ITEMS = 64, 4096
(FBS_FRAMES, FBS_GRAPHS, FBS_MAX_GRAPH_NODES, FBS_STAGING_BYTES, FBS_ARENA_BYTES, FBS_ITEMS, FBS_GROUPS, FBS_BLOCKS, FBS_NODE_TYPES,
 FBS_EDGE_TYPES, FBS_TENSORS, FBS_COUNT) = range(12)
FT_BATCH, FTB_BATCH, FTB_NODE_PTR, FTB_EDGE_PTR, FTB_Y, FT_BATCH_COUNT = 54, 0, 6, 12, 27, 33
FT_HTREL, FT_HTREL_COUNT = 87, 17  # what FRAME_RELPOS_HTREE adds: pos of the two clique types, edge_attr of the 15 H-tree edge types

# include/hydra_mp.h section 15: words of an item of hmp_store_derive's table, item kinds
SD_ITEM_WORDS, SD_MAX_ITEMS = 16, 4096
(SD_KIND, SD_BLOCK0, SD_SRC, SD_DST, SD_SRC_PTR, SD_DST_OFF, SD_N, SD_SRC_W, SD_SKIP, SD_TAKE, SD_DST_W, SD_A0, SD_A1, SD_A2, SD_A3,
 SD_UNIT) = range(16)
SD_ROWS, SD_FILL, SD_EDGES, SD_RELPOS, SD_COMPACT, SD_ROWS_ZERO = range(6)

COLLATE_MAX_ITEMS, COLLATE_MAX_SLOTS = 40, 24 # csrc/collate.hip CB_MAX_ITEMS / CB_MAX_SLOTS: arrays and types of one collation launch

ABI_VERSION = 4  # the HMP_ABI_VERSION of include/hydra_mp.h this binding was written against (tests/test_abi.py compares them)

_lib: Optional[C.CDLL] = None


class HydraMPError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen the HIP library (no GPU needed for this step) and bind every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7 / libhsa-runtime64: it must be in the process BEFORE our library is
    # dlopen'ed, so that both resolve to ONE HIP runtime (device pointers and streams are shared between them);
    # loading libhydra_mp.so first would pull /opt/rocm's runtime in and leave torch on a second, blind copy.
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise HydraMPError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C hydra-gnn_amd/csrc`.  hydra_gnn_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.hmp_abi_version() != ABI_VERSION:
        raise HydraMPError(f"ABI version mismatch: library {lib.hmp_abi_version()}, binding {ABI_VERSION} (stale build? run make)")
    for i, st in enumerate(_STRUCTS):
        if lib.hmp_sizeof(i) != C.sizeof(st):
            raise HydraMPError(f"struct layout mismatch for {st.__name__}: C {lib.hmp_sizeof(i)} vs ctypes {C.sizeof(st)}")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().hmp_last_error()
        raise HydraMPError(f"libhydra_mp error {rc}: {msg.decode() if msg else '?'}")


def require_device() -> C.CDLL:
    lib = load()
    if lib.hmp_device_count() < 1:
        raise HydraMPError("no gfx950 (MI355X) device visible: hydra_gnn_amd has no CPU fallback")
    return lib


def stream_ptr() -> int:
    """hipStream_t of torch's current stream (torch is the device-memory / stream plumbing)."""
    import torch

    return int(torch.cuda.current_stream().cuda_stream)
