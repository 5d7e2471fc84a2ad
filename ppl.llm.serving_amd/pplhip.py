"""ctypes binding of libpplhip.so (include/pplhip.h) for the parity tests and bench.py.

This is NOT a fallback path: every call goes into the HIP library; if the library is missing or a device call
fails, a PplHipError is raised.  Device tensors used by the single-operator entry points are torch tensors
(PyTorch is only the device-memory allocator here).
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPLHIP_LIB") or os.path.join(_DIR, "csrc", "libpplhip.so")   # PPLHIP_LIB: diagnosis builds (profiles/)
UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 64
COMM_NONE, COMM_RCCL, COMM_P2P = 0, 1, 2
_LIB = None

STATUS = {0: "SUCCESS", -1: "OTHER_ERROR", -2: "INVALID_VALUE", -3: "OUT_OF_MEMORY", -4: "DEVICE_RUNTIME_ERROR",
          -5: "DEVICE_MEMORY_ERROR", -6: "NOT_FOUND", -7: "UNSUPPORTED"}

PROF_ATTN_DECODE, PROF_ATTN_PREFILL, PROF_GEMM, PROF_RUN, PROF_LORA = 0, 1, 2, 3, 4


class PplHipError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [("hidden_dim", C.c_int32), ("intermediate_dim", C.c_int32), ("num_layers", C.c_int32),
                ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32), ("vocab_size", C.c_int32),
                ("norm_eps", C.c_float), ("rope_theta", C.c_float), ("max_position", C.c_int32),
                ("cache_quant_bit", C.c_int32), ("cache_quant_group", C.c_int32), ("cache_layout", C.c_int32),
                ("cache_mode", C.c_int32), ("page_size", C.c_int32), ("weight_quant_bit", C.c_int32),
                ("weight_quant_group", C.c_int32), ("act_quant_bit", C.c_int32)]


# ModelDesc.act_quant_bit values besides 0 (include/pplhip.h)
ACT_QUANT_I8 = 8        # online_i8i8
ACT_QUANT_FP8 = 0x108   # online_f8f8


class Opts(C.Structure):
    _fields_ = [("n_local_ranks", C.c_int32), ("world_size", C.c_int32), ("rank_base", C.c_int32),
                ("device_ids", C.POINTER(C.c_int32)), ("nccl_unique_id", C.c_void_p),
                ("max_running_batch", C.c_int32), ("max_tokens_per_step", C.c_int32), ("enable_penalty", C.c_int32),
                ("decoding_attn_split_k", C.c_int32), ("decoding_attn_tpb", C.c_int32), ("enable_profiling", C.c_int32)]


class Step(C.Structure):
    _fields_ = [("batch", C.c_int64), ("num_tokens", C.c_int64), ("decoding_batches", C.c_int64),
                ("max_seq_len", C.c_int64), ("max_kv_len", C.c_int64), ("max_pages", C.c_int64),
                ("token_inputs", C.c_void_p), ("seq_starts", C.c_void_p), ("kv_starts", C.c_void_p),
                ("start_pos", C.c_void_p), ("cache_indices", C.c_void_p), ("req_list_changed", C.c_int32)]


class SampleArgs(C.Structure):
    _fields_ = [("temperatures", C.c_void_p), ("top_k", C.c_void_p), ("top_p", C.c_void_p), ("batch", C.c_int32),
                ("vocab_size", C.c_int32), ("batch_stride", C.c_int32), ("default_top_k", C.c_int32),
                ("default_top_p", C.c_float), ("req_list_changed", C.c_int32), ("enable_penalty", C.c_int32)]


class SampleRowsArgs(C.Structure):
    _fields_ = [("temperatures", C.c_void_p), ("top_k", C.c_void_p), ("top_p", C.c_void_p), ("seeds", C.c_void_p), ("draws", C.c_void_p),
                ("batch", C.c_int32), ("vocab_size", C.c_int32), ("batch_stride", C.c_int32)]


class SampleRows2Args(C.Structure):
    _fields_ = SampleRowsArgs._fields_ + [("min_p", C.c_void_p), ("typical_p", C.c_void_p)]


TOP_LOGPROBS_MAX = 20   # PPLHIP_TOP_LOGPROBS_MAX


class TopLogprobsArgs(C.Structure):
    _fields_ = [("temperatures", C.c_void_p), ("num_logprobs", C.c_void_p), ("batch", C.c_int32), ("vocab_size", C.c_int32),
                ("batch_stride", C.c_int32)]


LOGIT_BIAS_MAX = 512   # PPLHIP_LOGIT_BIAS_MAX
LOGIT_STOP_MAX = 64    # PPLHIP_LOGIT_STOP_MAX


class LogitRule(C.Structure):
    _fields_ = [("bias_tokens", C.c_void_p), ("bias_values", C.c_void_p), ("n_bias", C.c_int32), ("allowed_bits", C.c_void_p),
                ("stop_tokens", C.c_void_p), ("n_stop", C.c_int32)]


class LogitEditArgs(C.Structure):
    _fields_ = [("batch_slots", C.c_void_p), ("flags", C.c_void_p), ("batch", C.c_int32), ("vocab_size", C.c_int32),
                ("batch_stride", C.c_int32)]


class PromptLogprobsOut(C.Structure):
    _fields_ = [("positions", C.c_int64), ("rows", C.c_void_p), ("logprobs", C.c_void_p), ("ranks", C.c_void_p), ("top_tokens", C.c_void_p),
                ("top_logprobs", C.c_void_p)]


GUIDE_MAX_SLOTS = 16     # PPLHIP_GUIDE_MAX_SLOTS
GUIDE_MAX_STATES = 255   # PPLHIP_GUIDE_MAX_STATES
GUIDE_DEAD = 255


class GuideDesc(C.Structure):
    _fields_ = [("trans", C.c_void_p), ("accept", C.c_void_p), ("n_states", C.c_int32), ("end_tokens", C.c_void_p), ("n_end", C.c_int32)]


class GuideEditArgs(C.Structure):
    _fields_ = [("guide_slots", C.c_void_p), ("states", C.c_void_p), ("batch", C.c_int32), ("vocab_size", C.c_int32),
                ("batch_stride", C.c_int32)]


class PenaltyArgs(C.Structure):
    _fields_ = [("temperatures", C.c_void_p), ("repetition_penalties", C.c_void_p), ("presence_penalties", C.c_void_p),
                ("frequency_penalties", C.c_void_p), ("batch_slots", C.c_void_p), ("batch", C.c_int32),
                ("vocab_size", C.c_int32), ("req_list_changed", C.c_int32)]


class KvView(C.Structure):
    _fields_ = [("cache", C.c_void_p), ("scale", C.c_void_p), ("max_tokens", C.c_int64), ("num_layers", C.c_int32),
                ("kv_heads", C.c_int32), ("head_dim", C.c_int32), ("quant_bit", C.c_int32), ("quant_group", C.c_int32),
                ("layout", C.c_int32), ("mode", C.c_int32), ("page_size", C.c_int32), ("layer", C.c_int32)]


COMM_MODES = {0: "none", 1: "rccl", 2: "direct xGMI kernels (two-shot, all links)"}
COMM_SCHEDULES = {0: "one-stream (collectives in stream)", 1: "two-stream (half-batches, a channel each)", 2: "chunked (collectives on the communication stream)"}


class CommInfo(C.Structure):
    _fields_ = [("mode", C.c_int32), ("selftest", C.c_int32), ("schedule", C.c_int32), ("has_rccl", C.c_int32),
                ("dual_min_rows", C.c_int64), ("dual_max_rows", C.c_int64), ("notes", C.c_char * 512)]


# pplhip_comm_op (test support): the direct collectives as operators
COMM_ALLREDUCE, COMM_ALLREDUCE_NORM, COMM_ALLGATHER = 0, 1, 2


class CommItem(C.Structure):
    _fields_ = [("kind", C.c_int32), ("channel", C.c_int32), ("epoch_advance", C.c_uint32), ("eps", C.c_float), ("count", C.c_int64),
                ("rows", C.c_int64), ("hidden", C.c_int64), ("cols", C.c_int64), ("dst_stride", C.c_int64), ("data_elems", C.c_int64),
                ("image_elems", C.c_int64), ("data", C.c_void_p), ("image0", C.c_void_p), ("image1", C.c_void_p), ("w", C.c_void_p),
                ("skew", C.c_void_p), ("out0", C.c_void_p), ("out1", C.c_void_p)]


class CommOpArgs(C.Structure):
    _fields_ = [("items", C.c_void_p), ("n_items", C.c_int32), ("counters", C.c_void_p)]


# pplhip_op_step_plan (test support): the step schedule as a pure function
SCHED_ONE_LANE, SCHED_TWO_LANES, SCHED_TWO_CHUNKS = 0, 1, 2   # CommInfo.schedule / StepPlan.schedule


class Chunk(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("b0", "bn", "t0", "tn", "nd")]


class PlanSettings(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tp", "tp_on", "comm_mode", "has_comm", "has_comm2", "emulate_tp", "tp_overlap", "dual_mode",
                                          "dual_auto", "has_stream2")] + \
               [(n, C.c_int64) for n in ("tp_overlap_min_tokens", "dual_min_rows", "dual_max_rows")] + \
               [(n, C.c_int32) for n in ("fuse_norm_want", "defer_on", "act_fmt", "hidden_dim", "heads", "kv_heads", "head_dim",
                                          "cache_quant_bit", "cache_quant_group", "decoding_attn_split_k")]


class StepShape(C.Structure):
    _fields_ = [("batch", C.c_int64), ("num_tokens", C.c_int64), ("decoding_batches", C.c_int64), ("max_kv_len", C.c_int64),
                ("seq_starts", C.c_void_p), ("capturing", C.c_int32), ("dump", C.c_int32), ("lora", C.c_int32)]


class StepPlan(C.Structure):
    _fields_ = [("schedule", C.c_int32), ("num_chunks", C.c_int32), ("chunk", Chunk * 2), ("decode_split", C.c_int32 * 2),
                ("fuse_norm", C.c_int32), ("defer_reduce", C.c_int32), ("defer_qkv", C.c_int32), ("lane1_ws_off", C.c_int64)]


# every symbol include/pplhip.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "pplhip_version", "pplhip_device_count", "pplhip_get_unique_id", "pplhip_init", "pplhip_destroy",
    "pplhip_comm_export", "pplhip_comm_connect", "pplhip_comm_mode", "pplhip_comm_fused_norm", "pplhip_comm_info", "pplhip_comm_allreduce_us", "pplhip_comm_op",
    "pplhip_last_error", "pplhip_rank_load", "pplhip_rank_set_tensor", "pplhip_rank_init_synthetic", "pplhip_rank_tie_output",
    "pplhip_kv_block_bytes", "pplhip_kv_capacity", "pplhip_kv_alloc", "pplhip_kv_ptrs", "pplhip_kv_read",
    "pplhip_kv_write", "pplhip_kv_fill_synthetic",
    "pplhip_lora_set_tensor", "pplhip_lora_commit", "pplhip_lora_load", "pplhip_lora_unload", "pplhip_set_adapters", "pplhip_op_lora",
    "pplhip_set_inputs", "pplhip_set_prompt_logprobs", "pplhip_prompt_logprobs", "pplhip_run", "pplhip_debug_run_dump", "pplhip_logits", "pplhip_copy_logits", "pplhip_sync",
    "pplhip_sample", "pplhip_sample_rows", "pplhip_sample_rows2", "pplhip_top_logprobs", "pplhip_logit_rule_set", "pplhip_logit_edit", "pplhip_guide_set_vocab", "pplhip_guide_load", "pplhip_guide_unload", "pplhip_guide_edit", "pplhip_guide_load16", "pplhip_guide16_state_chunk", "pplhip_penalty", "pplhip_profile_reset", "pplhip_profile_get", "pplhip_profile_mode", "pplhip_mem_info",
    "pplhip_op_embedding", "pplhip_op_rmsnorm", "pplhip_op_linear", "pplhip_op_linear_swiglu", "pplhip_op_linear_ex", "pplhip_op_linear_q8_ex", "pplhip_op_step_plan", "pplhip_op_rmsnorm_quant", "pplhip_op_quant_act", "pplhip_op_quant_weight",
    "pplhip_op_linear_i8", "pplhip_op_rmsnorm_quant_f8", "pplhip_op_quant_act_f8", "pplhip_op_quant_weight_f8", "pplhip_op_linear_f8",
    "pplhip_op_silu_mul", "pplhip_op_penalty", "pplhip_op_sample", "pplhip_op_sample_rows", "pplhip_op_sample_rows2", "pplhip_op_sample_uniform", "pplhip_op_top_logprobs", "pplhip_op_prompt_logprobs", "pplhip_op_logit_edit", "pplhip_op_guide_build", "pplhip_op_guide_mask", "pplhip_op_guide_build16", "pplhip_op_guide_mask16", "pplhip_op_rope_kv_write",
    "pplhip_op_attention", "pplhip_build_rope_table",
    "pplhip_op_rmsnorm_form", "pplhip_op_rmsnorm_ex", "pplhip_op_gather_last_rows", "pplhip_op_rope_kv_write_ex", "pplhip_op_linear_defer",
]


def build():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_DIR, "csrc")])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise PplHipError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
        L.pplhip_last_error.restype = C.c_char_p
        L.pplhip_last_error.argtypes = [vp, C.c_int]
        L.pplhip_get_unique_id.argtypes = [vp]
        L.pplhip_init.argtypes = [C.POINTER(ModelDesc), C.POINTER(Opts), C.POINTER(vp)]
        L.pplhip_destroy.argtypes = [vp]
        L.pplhip_destroy.restype = None
        L.pplhip_comm_export.argtypes = [vp, C.c_int, vp]
        L.pplhip_comm_connect.argtypes = [vp, vp]
        L.pplhip_comm_mode.argtypes = [vp]
        L.pplhip_comm_fused_norm.argtypes = [vp]
        L.pplhip_comm_info.argtypes = [vp, i64, C.POINTER(CommInfo)]
        L.pplhip_comm_allreduce_us.argtypes = [vp, C.c_int, i64, i32, i32, C.POINTER(f32)]
        if hasattr(L, "pplhip_comm_op"):   # (PPLHIP_LIB may name a build from before it, as below)
            L.pplhip_comm_op.argtypes = [vp, C.POINTER(CommOpArgs)]
        L.pplhip_rank_load.argtypes = [vp, C.c_int, C.c_char_p]
        L.pplhip_rank_set_tensor.argtypes = [vp, C.c_int, C.c_char_p, vp, u64]
        L.pplhip_rank_init_synthetic.argtypes = [vp, C.c_int, u64]
        L.pplhip_rank_tie_output.argtypes = [vp, C.c_int, i64, u64, f32]
        L.pplhip_kv_block_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.pplhip_kv_capacity.argtypes = [vp, f32, C.POINTER(u64)]
        L.pplhip_kv_alloc.argtypes = [vp, C.c_int, u64]
        L.pplhip_kv_ptrs.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
        L.pplhip_kv_read.argtypes = [vp, C.c_int, C.c_int, u64, vp, u64]
        L.pplhip_kv_write.argtypes = [vp, C.c_int, C.c_int, u64, vp, u64]
        L.pplhip_kv_fill_synthetic.argtypes = [vp, C.c_int, u64]
        L.pplhip_set_inputs.argtypes = [vp, C.c_int, C.POINTER(Step)]
        # (as pplhip_op_step_plan: PPLHIP_LIB may name a build from before multi-LoRA)
        if hasattr(L, "pplhip_lora_commit"):
            L.pplhip_lora_set_tensor.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, vp, u64, i32]
            L.pplhip_lora_commit.argtypes = [vp, C.c_int, C.c_int, f32]
            L.pplhip_lora_load.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
            L.pplhip_lora_unload.argtypes = [vp, C.c_int, C.c_int]
            L.pplhip_set_adapters.argtypes = [vp, C.c_int, vp, i64]
            L.pplhip_op_lora.argtypes = [vp, vp, i64, vp, i64, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp, u64]
        L.pplhip_run.argtypes = [vp, C.c_int, C.c_int]
        L.pplhip_debug_run_dump.argtypes = [vp, C.c_int, vp]
        L.pplhip_logits.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(i64)]
        L.pplhip_copy_logits.argtypes = [vp, C.c_int, vp, i64]
        L.pplhip_sync.argtypes = [vp, C.c_int]
        L.pplhip_sample.argtypes = [vp, vp, C.POINTER(SampleArgs), vp, vp]
        L.pplhip_penalty.argtypes = [vp, vp, C.POINTER(PenaltyArgs)]
        L.pplhip_profile_reset.argtypes = [vp, C.c_int]
        L.pplhip_profile_get.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(C.c_double)]
        L.pplhip_profile_mode.argtypes = [vp, C.c_int]
        L.pplhip_mem_info.argtypes = [vp, C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.pplhip_op_embedding.argtypes = [vp, vp, vp, i64, i32, vp]
        L.pplhip_op_rmsnorm.argtypes = [vp, vp, vp, vp, f32, i64, i32, vp, vp]
        L.pplhip_op_linear.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, i32, vp, i32]
        L.pplhip_op_linear_swiglu.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, i32, vp]
        L.pplhip_op_linear_ex.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, i32, vp, i64, i32, vp, u64, i32, C.c_char_p, i32]
        # (PPLHIP_LIB may name a 1.2 build from before this entry point: bench.py and the profiles/ scripts must still load it for A/B runs;
        # tests/test_abi.py holds the product's own library to the export)
        if hasattr(L, "pplhip_op_step_plan"):
            L.pplhip_op_step_plan.argtypes = [C.POINTER(PlanSettings), C.POINTER(StepShape), C.POINTER(StepPlan)]
        L.pplhip_op_rmsnorm_quant.argtypes = [vp, vp, vp, vp, C.c_float, i64, i32, vp, vp, vp]
        L.pplhip_op_quant_act.argtypes = [vp, vp, i64, i32, vp, vp]
        L.pplhip_op_quant_weight.argtypes = [vp, vp, i32, i32, vp, vp]
        L.pplhip_op_linear_i8.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, i32, i32]
        L.pplhip_op_rmsnorm_quant_f8.argtypes = [vp, vp, vp, vp, C.c_float, i64, i32, vp, vp, vp]
        L.pplhip_op_quant_act_f8.argtypes = [vp, vp, i64, i32, vp, vp]
        L.pplhip_op_quant_weight_f8.argtypes = [vp, vp, i32, i32, vp, vp]
        L.pplhip_op_linear_f8.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, i32, i32]
        if hasattr(L, "pplhip_op_linear_q8_ex"):   # (PPLHIP_LIB may name a build from before it, as above)
            L.pplhip_op_linear_q8_ex.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, i32, vp, i64, i32, i32, C.c_char_p, i32]
        L.pplhip_op_silu_mul.argtypes = [vp, vp, i64, i32, vp]
        L.pplhip_op_penalty.argtypes = [vp] * 10 + [i32, i32, i32, i32, vp]
        L.pplhip_op_sample.argtypes = [vp] * 5 + [i32, i32, i32, i32, f32, vp, vp]
        if hasattr(L, "pplhip_sample_rows"):
            L.pplhip_sample_rows.argtypes = [vp, vp, C.POINTER(SampleRowsArgs), vp, vp]
            L.pplhip_op_sample_rows.argtypes = [vp] * 8 + [i32, i32, i32, vp, vp]
        if hasattr(L, "pplhip_sample_rows2"):
            L.pplhip_sample_rows2.argtypes = [vp, vp, C.POINTER(SampleRows2Args), vp, vp]
            L.pplhip_op_sample_rows2.argtypes = [vp] * 10 + [i32, i32, i32, vp, vp]
            L.pplhip_op_sample_uniform.argtypes = [vp, vp, vp, i32, vp]
        if hasattr(L, "pplhip_top_logprobs"):
            L.pplhip_top_logprobs.argtypes = [vp, vp, C.POINTER(TopLogprobsArgs), C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
            L.pplhip_op_top_logprobs.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
        if hasattr(L, "pplhip_set_prompt_logprobs"):
            L.pplhip_set_prompt_logprobs.argtypes = [vp, C.c_int, vp, i64]
            L.pplhip_prompt_logprobs.argtypes = [vp, C.c_int, C.POINTER(PromptLogprobsOut)]
            L.pplhip_op_prompt_logprobs.argtypes = [vp, vp, i32, i32, vp, i32, vp, i64, vp, vp, vp, vp, vp]
        if hasattr(L, "pplhip_logit_edit"):
            L.pplhip_logit_rule_set.argtypes = [vp, i32, C.POINTER(LogitRule)]
            L.pplhip_logit_edit.argtypes = [vp, vp, C.POINTER(LogitEditArgs)]
            L.pplhip_op_logit_edit.argtypes = [vp, vp, i32, i32, i32] + [vp] * 8 + [i32]
        if hasattr(L, "pplhip_guide_load"):
            L.pplhip_guide_set_vocab.argtypes = [vp, vp, vp, i32]
            L.pplhip_guide_load.argtypes = [vp, i32, C.POINTER(GuideDesc)]
            L.pplhip_guide_unload.argtypes = [vp, i32]
            L.pplhip_guide_edit.argtypes = [vp, vp, C.POINTER(GuideEditArgs)]
            L.pplhip_op_guide_build.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, vp, i64, vp]
            L.pplhip_op_guide_mask.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, i64, vp, i32]
        if hasattr(L, "pplhip_guide_load16"):
            L.pplhip_guide_load16.argtypes = [vp, i32, C.POINTER(GuideDesc)]   # (the descriptor's layout is pplhip_guide_desc's)
            L.pplhip_guide16_state_chunk.argtypes = []
            L.pplhip_guide16_state_chunk.restype = i32
            L.pplhip_op_guide_build16.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, vp, i64, vp]
            L.pplhip_op_guide_mask16.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, i64, vp, i32]
        L.pplhip_op_rope_kv_write.argtypes = [vp, vp, vp, C.POINTER(KvView), vp, vp, vp, i64, i64, i64, i32]
        L.pplhip_op_attention.argtypes = [vp, vp, C.POINTER(KvView), vp, vp, vp, i64, i64, i64, i64, i64, i64, i32, i32,
                                          vp, u64, vp]
        L.pplhip_build_rope_table.argtypes = [vp, i32, i32, f32]
        # (the row-kernel test entries: PPLHIP_LIB may name a build from before them, as above)
        if hasattr(L, "pplhip_op_rmsnorm_form"):
            L.pplhip_op_rmsnorm_form.argtypes = [i64, i32, i32, i32, C.c_char_p, i32]
            L.pplhip_op_rmsnorm_ex.argtypes = [vp, vp, vp, vp, f32, i64, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, i64]
            L.pplhip_op_gather_last_rows.argtypes = [vp, vp, vp, i64, i32, vp]
            L.pplhip_op_rope_kv_write_ex.argtypes = [vp, vp, vp, C.POINTER(KvView), vp, vp, vp, i64, i64, i64, i64, i32, vp, i32, vp, i64]
            L.pplhip_op_linear_defer.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, i32, vp, i64, vp, u64, i32, C.POINTER(i32), C.POINTER(vp),
                                                 C.c_char_p, i32]
        _LIB = L
    return _LIB


def linear_route(x, w, scale, wq_bit, group, M, N, K, y, ldy, epi, ws=None, ws_bytes=0, dry_run=True, stream=None):
    """pplhip_op_linear_ex: (status, route text).  Pointers are integers (device addresses; a dry run never dereferences them)."""
    buf = C.create_string_buffer(1024)
    rc = lib().pplhip_op_linear_ex(stream, x, w, scale, wq_bit, group, M, N, K, y, ldy, epi, ws, ws_bytes, int(dry_run), buf, 1024)
    return rc, buf.value.decode()


def linear_q8_route(xq, sx, w, scale, act_fmt, M, N, K, y, ldy, epi, dry_run=True, stream=None):
    """pplhip_op_linear_q8_ex (act_fmt 8: int8, 0x108: fp8 e4m3): (status, route text).  Pointers are integers, as in linear_route."""
    buf = C.create_string_buffer(1024)
    rc = lib().pplhip_op_linear_q8_ex(stream, xq, sx, w, scale, act_fmt, M, N, K, y, ldy, epi, int(dry_run), buf, 1024)
    return rc, buf.value.decode()


def rmsnorm_form(rows, hidden, quant=0, wide_max_rows=512):
    """pplhip_op_rmsnorm_form (no device): (status, form text)"""
    buf = C.create_string_buffer(64)
    rc = lib().pplhip_op_rmsnorm_form(rows, hidden, quant, wide_max_rows, buf, 64)
    return rc, buf.value.decode()


def linear_defer(x, w, scale, wq_bit, group, M, N, K, y, ldy, ws=None, ws_bytes=0, dry_run=True, stream=None):
    """pplhip_op_linear_defer: (status, route text, splits, slab scale address or None).  Pointers are integers, as in linear_route."""
    buf = C.create_string_buffer(1024)
    sp, sc = C.c_int32(0), C.c_void_p(None)
    rc = lib().pplhip_op_linear_defer(stream, x, w, scale, wq_bit, group, M, N, K, y, ldy, ws, ws_bytes, int(dry_run), C.byref(sp), C.byref(sc),
                                      buf, 1024)
    return rc, buf.value.decode(), sp.value, sc.value


def step_plan(settings, batch, num_tokens, decoding_batches, seq_starts=None, max_kv_len=0, capturing=False, dump=False, lora=False):
    """pplhip_op_step_plan (no device): the plan of a step as a dict.  settings: PlanSettings field -> value (the rest 0);
    seq_starts: the host copy, None when the rank holds none."""
    st = PlanSettings(**settings)
    ss = None if seq_starts is None else np.ascontiguousarray(seq_starts, dtype=np.int64)
    sh = StepShape(batch, num_tokens, decoding_batches, max_kv_len, None if ss is None else ss.ctypes.data, int(capturing), int(dump), int(lora))
    out = StepPlan()
    rc = lib().pplhip_op_step_plan(C.byref(st), C.byref(sh), C.byref(out))
    if rc:
        raise PplHipError(f"pplhip_op_step_plan -> {STATUS.get(rc, rc)}")
    return {"schedule": out.schedule, "chunks": [tuple(getattr(out.chunk[i], n) for n in ("b0", "bn", "t0", "tn", "nd")) for i in range(out.num_chunks)],
            "decode_split": [out.decode_split[i] for i in range(out.num_chunks)], "fuse_norm": bool(out.fuse_norm),
            "defer_reduce": bool(out.defer_reduce), "defer_qkv": bool(out.defer_qkv), "lane1_ws_off": out.lane1_ws_off}


LORA_MAX_SLOTS, LORA_MAX_RANK = 64, 128
LORA_TARGETS = ("attention.wqkv", "attention.wo", "feed_forward.w2")


def lora_ws_bytes(T, n_slots=LORA_MAX_SLOTS):
    """a workspace size that always suffices for pplhip_op_lora (include/pplhip.h)"""
    return 8192 + (T // 16 + n_slots + 1) * 4352


def op_lora(x, ldx, y, ldy, T, N, K, row_slots, A, B, ranks, scales, ws, ws_bytes, stream=None):
    """pplhip_op_lora -> status.  x, y, ws and the entries of A / B are device addresses (integers, None for a slot that is not loaded);
    row_slots [T], ranks and scales [len(A)] are host arrays.  The refusals are decided before any device call."""
    n = len(A)
    rs = np.ascontiguousarray(row_slots, dtype=np.int32)
    pa = (C.c_void_p * max(n, 1))(*[a or None for a in A])
    pb = (C.c_void_p * max(n, 1))(*[b or None for b in B])
    rk = np.ascontiguousarray(ranks, dtype=np.int32)
    sc = np.ascontiguousarray(scales, dtype=np.float32)
    return lib().pplhip_op_lora(stream, x, ldx, y, ldy, T, N, K, rs.ctypes.data, n, pa, pb, rk.ctypes.data, sc.ctypes.data, ws, ws_bytes)


def write_lora_container(path, tensors, scale):
    """lora.pplhip: the weight container with the adapter's factors ({name: fp16 array}) and lora.scale (fp32 [1])"""
    t = {k: np.ascontiguousarray(v, dtype=np.float16) for k, v in tensors.items()}
    t["lora.scale"] = np.array([scale], dtype=np.float32)
    write_container(path, t)


def make_desc(**kw):
    d = ModelDesc()
    defaults = dict(norm_eps=1e-5, rope_theta=10000.0, max_position=4096, cache_quant_bit=0, cache_quant_group=1,
                    cache_layout=3, cache_mode=0, page_size=0, weight_quant_bit=0, weight_quant_group=128, act_quant_bit=0)
    defaults.update(kw)
    for k, v in defaults.items():
        setattr(d, k, v)
    return d


def copy_desc(src, cls=ModelDesc):
    d = cls()
    for name, _ in ModelDesc._fields_:
        setattr(d, name, getattr(src, name))
    return d


def get_unique_id():
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    rc = lib().pplhip_get_unique_id(buf)
    if rc:
        raise PplHipError(f"pplhip_get_unique_id -> {STATUS.get(rc, rc)}")
    return bytes(buf)


def write_container(path, tensors):
    """weights.pplhip: "PPLHIPW1" | u32 count | count x { u32 name_len | name | u64 nbytes | pad to 64 | data }"""
    with open(path, "wb") as f:
        f.write(b"PPLHIPW1")
        f.write(struct.pack("<I", len(tensors)))
        for name, arr in tensors.items():
            arr = np.ascontiguousarray(arr)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)))
            f.write(nb)
            f.write(struct.pack("<Q", arr.nbytes))
            pad = (64 - f.tell() % 64) % 64
            f.write(b"\0" * pad)
            f.write(arr.tobytes())


class Context:
    """One pplhip_ctx.  n_local_ranks ranks in this process; world_size may be larger (one process per GPU)."""

    def __init__(self, desc, max_running_batch, max_tokens_per_step, n_local_ranks=1, world_size=None, rank_base=0,
                 device_ids=None, unique_id=None, enable_penalty=False, split_k=1, tpb=0, profiling=False):
        self.desc = desc
        o = Opts()
        o.n_local_ranks = n_local_ranks
        o.world_size = world_size if world_size else n_local_ranks
        o.rank_base = rank_base
        self._devs = None
        if device_ids is not None:
            self._devs = (C.c_int32 * len(device_ids))(*device_ids)
            o.device_ids = C.cast(self._devs, C.POINTER(C.c_int32))
        self._uid = None
        if unique_id is not None:
            self._uid = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
            o.nccl_unique_id = C.cast(self._uid, C.c_void_p)
        o.max_running_batch, o.max_tokens_per_step = max_running_batch, max_tokens_per_step
        o.enable_penalty = int(enable_penalty)
        o.decoding_attn_split_k, o.decoding_attn_tpb, o.enable_profiling = split_k, tpb, int(profiling)
        self.opts = o
        self.h = C.c_void_p()
        rc = lib().pplhip_init(C.byref(desc), C.byref(o), C.byref(self.h))
        if rc:
            raise PplHipError(f"pplhip_init -> {STATUS.get(rc, rc)}")
        self.n_local = n_local_ranks

    def _ck(self, rc, rank=0, what=""):
        if rc:
            msg = lib().pplhip_last_error(self.h, rank)
            raise PplHipError(f"{what} -> {STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def close(self):
        if self.h:
            lib().pplhip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # tensor-parallel collectives (one process per GPU: export -> all-gather by the launcher -> connect)
    def comm_export(self, rank=0):
        buf = (C.c_uint8 * IPC_HANDLE_BYTES)()
        self._ck(lib().pplhip_comm_export(self.h, rank, buf), rank, "comm_export")
        return bytes(buf)

    def comm_connect(self, all_handles):
        blob = b"".join(all_handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._ck(lib().pplhip_comm_connect(self.h, buf), -1, "comm_connect")

    def comm_mode(self):
        return lib().pplhip_comm_mode(self.h)

    def comm_info(self, rows):
        """what a multi-GPU run does at a pure-decode step of `rows` rows: mode, self-test verdict, schedule, fallbacks taken"""
        ci = CommInfo()
        self._ck(lib().pplhip_comm_info(self.h, rows, C.byref(ci)), -1, "comm_info")
        mode = COMM_MODES[ci.mode]
        if lib().pplhip_comm_fused_norm(self.h) == 1:
            mode += " + residual add and RMSNorm fused between the two shots (sequence-parallel residual stream)"
        return {"mode": mode, "selftest": {0: "not run", 1: "passed", -1: "failed"}[ci.selftest],
                "schedule": COMM_SCHEDULES[ci.schedule], "rccl_communicator": bool(ci.has_rccl),
                "two_stream_rows": [int(ci.dual_min_rows), int(ci.dual_max_rows)], "fallbacks": ci.notes.decode(errors="replace")}

    def comm_allreduce_us(self, rows, iters=20, path=0, rank=0):
        """average microseconds of one all-reduce of fp16 [rows, hidden] (collective call); None when the path does not exist"""
        us = C.c_float(-1.0)
        self._ck(lib().pplhip_comm_allreduce_us(self.h, rank, rows, iters, path, C.byref(us)), rank, "comm_allreduce_us")
        return None if us.value < 0 else float(us.value)

    def comm_op(self, items):
        """pplhip_comm_op: a sequence of direct collectives on every local rank -> (status, outputs, counters).  An item is a dict: kind
        (COMM_*), channel, epoch_advance, and per kind
          all-reduce  count, data: per rank the fp16 image of the data buffer (the first count elements are the partial sums)
          fused form  rows, hidden, eps, data: per rank fp16 [rows, hidden], h / xn: per rank the fp16 images of the residual rows and of
                      the normed matrix, w: per rank fp16 [hidden]
          all-gather  rows, cols, dst_stride, data: per rank fp32 [rows, cols], target: per rank the image of the gather target
                      (any 4-byte type)
        and optionally skew: per rank 0 .. 64 extra device copies in front of the rank's part.  outputs[i] is the list over the ranks
        of what the item may have written: the data buffer, (h, xn), or the target, as arrays like the images.  counters: (epoch of
        channel 0, of channel 1, all-reduces of channel 0, of channel 1) as the call leaves them.  A non-zero status leaves outputs None;
        last_error() has the reason."""
        n = self.n_local
        arr, keep, outs = (CommItem * max(1, len(items)))(), [], []

        def ptrs(arrays):
            assert len(arrays) == n
            p = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
            keep.append((arrays, p))
            return C.cast(p, C.c_void_p)

        def images(arrays, dtype=None):
            a = [np.ascontiguousarray(x) if dtype is None else np.ascontiguousarray(x, dtype=dtype) for x in arrays]
            assert all(x.size == a[0].size and x.itemsize == a[0].itemsize for x in a)
            return a

        for i, it in enumerate(items):
            ci = arr[i]
            ci.kind, ci.channel, ci.epoch_advance = it["kind"], it.get("channel", 0), it.get("epoch_advance", 0)
            ci.eps = it.get("eps", 0.0)
            data = images(it["data"])
            ci.data, ci.data_elems = ptrs(data), data[0].size
            if it["kind"] == COMM_ALLREDUCE:
                assert data[0].itemsize == 2
                ci.count = it["count"]
                out = [np.empty_like(x) for x in data]
                ci.out0 = ptrs(out)
                outs.append(out)
            elif it["kind"] == COMM_ALLREDUCE_NORM:
                h, xn, w = images(it["h"]), images(it["xn"]), images(it["w"])
                assert data[0].itemsize == h[0].itemsize == xn[0].itemsize == w[0].itemsize == 2 and h[0].size == xn[0].size
                assert w[0].size == it["hidden"]
                ci.rows, ci.hidden, ci.image_elems = it["rows"], it["hidden"], h[0].size
                ci.image0, ci.image1, ci.w = ptrs(h), ptrs(xn), ptrs(w)
                oh, ox = [np.empty_like(x) for x in h], [np.empty_like(x) for x in xn]
                ci.out0, ci.out1 = ptrs(oh), ptrs(ox)
                outs.append(list(zip(oh, ox)))
            else:
                tgt = images(it["target"])
                assert data[0].itemsize == tgt[0].itemsize == 4
                ci.rows, ci.cols, ci.dst_stride, ci.image_elems = it["rows"], it["cols"], it["dst_stride"], tgt[0].size
                ci.image0 = ptrs(tgt)
                out = [np.empty_like(x) for x in tgt]
                ci.out0 = ptrs(out)
                outs.append(out)
            if it.get("skew") is not None:
                sk = np.ascontiguousarray(it["skew"], dtype=np.int32)
                assert sk.size == n
                keep.append(sk)
                ci.skew = sk.ctypes.data
        counters = (C.c_uint32 * 4)()
        args = CommOpArgs(C.cast(arr, C.c_void_p), len(items), C.cast(counters, C.c_void_p))
        rc = lib().pplhip_comm_op(self.h, C.byref(args))
        return rc, (outs if rc == 0 else None), tuple(counters)

    def last_error(self, rank=-1):
        msg = lib().pplhip_last_error(self.h, rank)
        return msg.decode() if msg else ""

    # weights
    def set_tensor(self, rank, name, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(lib().pplhip_rank_set_tensor(self.h, rank, name.encode(), arr.ctypes.data, arr.nbytes), rank, f"set_tensor({name})")

    def load(self, rank, slice_dir):
        self._ck(lib().pplhip_rank_load(self.h, rank, slice_dir.encode()), rank, "rank_load")

    def init_synthetic(self, rank, seed):
        self._ck(lib().pplhip_rank_init_synthetic(self.h, rank, seed), rank, "rank_init_synthetic")

    # kv
    def kv_block_bytes(self):
        kb, sb = C.c_uint64(), C.c_uint64()
        self._ck(lib().pplhip_kv_block_bytes(self.h, C.byref(kb), C.byref(sb)))
        return kb.value, sb.value

    def kv_capacity(self, scale):
        t = C.c_uint64()
        self._ck(lib().pplhip_kv_capacity(self.h, scale, C.byref(t)), 0, "kv_capacity")
        return t.value

    def kv_alloc(self, rank, tokens):
        self._ck(lib().pplhip_kv_alloc(self.h, rank, tokens), rank, "kv_alloc")
        self.kv_tokens = tokens

    def kv_read(self, rank, which):
        kb, sb = self.kv_block_bytes()
        n = self.kv_tokens * (sb if which else kb)
        if n == 0:
            return None
        # quantised slabs as bytes: int8 and fp8 one per channel, int4 (cache_quant_bit 4) two channels per byte, low nibble first
        dt = np.float16 if which == 1 or self.desc.cache_quant_bit == 0 else np.int8
        out = np.empty(n // np.dtype(dt).itemsize, dtype=dt)
        self._ck(lib().pplhip_kv_read(self.h, rank, which, 0, out.ctypes.data, n), rank, "kv_read")
        return out

    def kv_write(self, rank, which, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self._ck(lib().pplhip_kv_write(self.h, rank, which, offset, arr.ctypes.data, arr.nbytes), rank, "kv_write")

    def kv_fill_synthetic(self, rank, seed):
        self._ck(lib().pplhip_kv_fill_synthetic(self.h, rank, seed), rank, "kv_fill_synthetic")

    # step
    def set_inputs(self, rank, step):
        self._ck(lib().pplhip_set_inputs(self.h, rank, C.byref(step)), rank, "set_inputs")

    # multi-LoRA
    def lora_set_tensor(self, rank, slot, name, arr, r=None):
        """one factor: lora_a [r, K] or lora_b [N, r] (fp16)"""
        arr = np.ascontiguousarray(arr, dtype=np.float16)
        if r is None:
            r = arr.shape[1] if name.endswith("lora_b") else arr.shape[0]
        self._ck(lib().pplhip_lora_set_tensor(self.h, rank, slot, name.encode(), arr.ctypes.data, arr.nbytes, r), rank, f"lora_set_tensor({name})")

    def lora_commit(self, rank, slot, scale):
        self._ck(lib().pplhip_lora_commit(self.h, rank, slot, scale), rank, "lora_commit")

    def lora_set(self, rank, slot, tensors, scale):
        """every factor of {name: array}, then commit"""
        for name, arr in tensors.items():
            self.lora_set_tensor(rank, slot, name, arr)
        self.lora_commit(rank, slot, scale)

    def lora_load(self, rank, slot, adapter_dir):
        self._ck(lib().pplhip_lora_load(self.h, rank, slot, adapter_dir.encode()), rank, "lora_load")

    def lora_unload(self, rank, slot):
        self._ck(lib().pplhip_lora_unload(self.h, rank, slot), rank, "lora_unload")

    def set_adapters(self, rank, slots):
        """after set_inputs, before run: the adapter slot of every request of the step (-1: none)"""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        self._ck(lib().pplhip_set_adapters(self.h, rank, s.ctypes.data, len(s)), rank, "set_adapters")

    def set_prompt_logprobs(self, rank, ask):
        """after set_inputs, before run: per request of the step -1 (off), 0 (logprob and rank of every prompt token) or n in 1 .. 20
        (also the first n entries of every position's ranking)"""
        a = np.ascontiguousarray(ask, dtype=np.int32)
        self._ck(lib().pplhip_set_prompt_logprobs(self.h, rank, a.ctypes.data, len(a)), rank, "set_prompt_logprobs")

    def prompt_logprobs(self, rank=0):
        """the prompt logprobs of the last run, copied out of the library's pinned block: call it after a synchronisation (sync(),
        copy_logits() or the sampler) and before the next run.  (rows [P], logprobs [P], ranks [P], top_tokens [P, 20], top_logprobs
        [P, 20]); P = 0 when the run had no ask."""
        o = PromptLogprobsOut()
        self._ck(lib().pplhip_prompt_logprobs(self.h, rank, C.byref(o)), rank, "prompt_logprobs")
        P = o.positions

        def arr(p, ct, dt, shape):
            if P == 0:
                return np.empty(shape, dtype=dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=shape).copy()
        return (arr(o.rows, C.c_int32, np.int32, (P,)), arr(o.logprobs, C.c_float, np.float32, (P,)), arr(o.ranks, C.c_int32, np.int32, (P,)),
                arr(o.top_tokens, C.c_int32, np.int32, (P, TOP_LOGPROBS_MAX)), arr(o.top_logprobs, C.c_float, np.float32, (P, TOP_LOGPROBS_MAX)))

    def run(self, rank, cache_prefill=0):
        self._ck(lib().pplhip_run(self.h, rank, cache_prefill), rank, "run")

    def run_dump(self, rank, num_tokens):
        """diagnosis: run the step and return the residual stream after every layer, fp32 [L+1, T, hidden] (oracle convention)"""
        out = np.empty((self.desc.num_layers + 1, num_tokens, self.desc.hidden_dim), dtype=np.float32)
        self._ck(lib().pplhip_debug_run_dump(self.h, rank, out.ctypes.data), rank, "debug_run_dump")
        return out

    def sync(self, rank=0):
        self._ck(lib().pplhip_sync(self.h, rank), rank, "sync")

    def logits_ptr(self, rank=0):
        p, s = C.c_void_p(), C.c_int64()
        self._ck(lib().pplhip_logits(self.h, rank, C.byref(p), C.byref(s)))
        return p.value, s.value

    def copy_logits(self, batch, rank=0):
        out = np.empty((batch, self.desc.vocab_size), dtype=np.float32)
        self._ck(lib().pplhip_copy_logits(self.h, rank, out.ctypes.data, batch), rank, "copy_logits")
        return out

    def sample(self, batch, top_k=1, top_p=0.0, temperatures=None, top_p_list=None, req_list_changed=True,
               enable_penalty=False, logits_ptr=None):
        a = SampleArgs()
        keep = []
        if temperatures is not None:
            t = np.ascontiguousarray(temperatures, dtype=np.float32); keep.append(t); a.temperatures = t.ctypes.data
        if top_p_list is not None:
            t = np.ascontiguousarray(top_p_list, dtype=np.float32); keep.append(t); a.top_p = t.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = batch, self.desc.vocab_size, self.desc.vocab_size
        a.default_top_k, a.default_top_p = top_k, top_p
        a.req_list_changed, a.enable_penalty = int(req_list_changed), int(enable_penalty)
        tok = np.empty(batch, dtype=np.int32)
        lp = np.empty(batch, dtype=np.float32)
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        self._ck(lib().pplhip_sample(self.h, logits_ptr, C.byref(a), tok.ctypes.data, lp.ctypes.data), 0, "sample")
        return tok, lp

    def sample_rows(self, top_k, top_p, seeds, draws, temperatures=None, logits_ptr=None):
        """the per-request sampler on the logits of the last run: every argument one value per batch row"""
        a = SampleRowsArgs()
        k = np.ascontiguousarray(top_k, dtype=np.int32)
        p = np.ascontiguousarray(top_p, dtype=np.float32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        dr = np.ascontiguousarray(draws, dtype=np.uint64)
        t = None if temperatures is None else np.ascontiguousarray(temperatures, dtype=np.float32)
        batch = len(k)
        assert len(p) == len(sd) == len(dr) == batch and (t is None or len(t) == batch)
        a.top_k, a.top_p, a.seeds, a.draws = k.ctypes.data, p.ctypes.data, sd.ctypes.data, dr.ctypes.data
        a.temperatures = None if t is None else t.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = batch, self.desc.vocab_size, self.desc.vocab_size
        tok = np.empty(batch, dtype=np.int32)
        lp = np.empty(batch, dtype=np.float32)
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        self._ck(lib().pplhip_sample_rows(self.h, logits_ptr, C.byref(a), tok.ctypes.data, lp.ctypes.data), 0, "sample_rows")
        return tok, lp

    def sample_rows2(self, top_k, top_p, seeds, draws, min_p=None, typical_p=None, temperatures=None, logits_ptr=None):
        """sample_rows with a min_p and a typical_p per batch row (None: off for every row)"""
        a = SampleRows2Args()
        k = np.ascontiguousarray(top_k, dtype=np.int32)
        p = np.ascontiguousarray(top_p, dtype=np.float32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        dr = np.ascontiguousarray(draws, dtype=np.uint64)
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float32)
        t, mp, ty = f32(temperatures), f32(min_p), f32(typical_p)
        batch = len(k)
        assert len(p) == len(sd) == len(dr) == batch and all(v is None or len(v) == batch for v in (t, mp, ty))
        a.top_k, a.top_p, a.seeds, a.draws = k.ctypes.data, p.ctypes.data, sd.ctypes.data, dr.ctypes.data
        a.temperatures, a.min_p, a.typical_p = (None if v is None else v.ctypes.data for v in (t, mp, ty))
        a.batch, a.vocab_size, a.batch_stride = batch, self.desc.vocab_size, self.desc.vocab_size
        tok = np.empty(batch, dtype=np.int32)
        lp = np.empty(batch, dtype=np.float32)
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        self._ck(lib().pplhip_sample_rows2(self.h, logits_ptr, C.byref(a), tok.ctypes.data, lp.ctypes.data), 0, "sample_rows2")
        return tok, lp

    def top_logprobs(self, num_logprobs, temperatures=None, logits_ptr=None):
        """queues the top-N logprobs of the last run's logits for the rows with num_logprobs > 0 and returns a function that reads them:
        call it after the step's sampler call (or sync()) and before the next top_logprobs; it gives (tokens, logprobs), each
        [asked, TOP_LOGPROBS_MAX] copied out of the library's pinned block, row j = the j-th asking batch row."""
        a = TopLogprobsArgs()
        n = np.ascontiguousarray(num_logprobs, dtype=np.int32)
        t = None if temperatures is None else np.ascontiguousarray(temperatures, dtype=np.float32)
        assert t is None or len(t) == len(n)
        a.num_logprobs = n.ctypes.data
        a.temperatures = None if t is None else t.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = len(n), self.desc.vocab_size, self.desc.vocab_size
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        p_tok, p_lp, rows = C.c_void_p(), C.c_void_p(), C.c_int32(-1)
        self._ck(lib().pplhip_top_logprobs(self.h, logits_ptr, C.byref(a), C.byref(p_tok), C.byref(p_lp), C.byref(rows)), 0, "top_logprobs")
        asked = rows.value

        def read():
            if asked == 0:
                return np.empty((0, TOP_LOGPROBS_MAX), dtype=np.int32), np.empty((0, TOP_LOGPROBS_MAX), dtype=np.float32)
            tok = np.ctypeslib.as_array(C.cast(p_tok, C.POINTER(C.c_int32)), shape=(asked, TOP_LOGPROBS_MAX)).copy()
            lp = np.ctypeslib.as_array(C.cast(p_lp, C.POINTER(C.c_float)), shape=(asked, TOP_LOGPROBS_MAX)).copy()
            return tok, lp
        read.rows = asked
        return read

    def logit_rule_set(self, slot, bias=(), allowed_bits=None, stops=(), check=True):
        """one slot's rule: bias = pairs (token, value), allowed_bits = None or uint32 [ceil(V / 32)], stops = tokens.  Returns the status
        (raises on failure unless check is False)."""
        r = LogitRule()
        bt = np.ascontiguousarray([t for t, _ in bias], dtype=np.int32)
        bv = np.ascontiguousarray([v for _, v in bias], dtype=np.float32)
        st = np.ascontiguousarray(list(stops), dtype=np.int32)
        ab = None if allowed_bits is None else np.ascontiguousarray(allowed_bits, dtype=np.uint32)
        r.bias_tokens, r.bias_values, r.n_bias = bt.ctypes.data, bv.ctypes.data, len(bt)
        r.allowed_bits = None if ab is None else ab.ctypes.data
        r.stop_tokens, r.n_stop = st.ctypes.data, len(st)
        rc = lib().pplhip_logit_rule_set(self.h, int(slot), C.byref(r))
        if check:
            self._ck(rc, 0, "logit_rule_set")
        return rc

    def logit_edit(self, batch_slots, flags, logits_ptr=None, check=True):
        """queues the in-place edit of the last run's logits (rank 0) for the rows with flags != 0; asynchronous."""
        a = LogitEditArgs()
        sl = np.ascontiguousarray(batch_slots, dtype=np.int64)
        fl = np.ascontiguousarray(flags, dtype=np.uint32)
        assert len(sl) == len(fl)
        a.batch_slots, a.flags = sl.ctypes.data, fl.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = len(fl), self.desc.vocab_size, self.desc.vocab_size
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        rc = lib().pplhip_logit_edit(self.h, logits_ptr, C.byref(a))
        if check:
            self._ck(rc, 0, "logit_edit")
        return rc

    def guide_set_vocab(self, token_bytes, check=True):
        """the vocabulary of guided decoding, once: token_bytes = one bytes object per token id (ids behind the list are empty)."""
        off = np.zeros(len(token_bytes) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(b) for b in token_bytes])
        blob = np.frombuffer(b"".join(token_bytes) + b"\0", dtype=np.uint8)
        rc = lib().pplhip_guide_set_vocab(self.h, blob.ctypes.data, off.ctypes.data, len(token_bytes))
        if check:
            self._ck(rc, 0, "guide_set_vocab")
        return rc

    def guide_load(self, slot, trans, accept, end_tokens=(), check=True):
        """builds slot's allowed-token masks from a DFA: trans uint8 [n_states, 256] (255 = dead), accept uint8 [n_states].  Synchronous."""
        tr = np.ascontiguousarray(trans, dtype=np.uint8)
        ac = np.ascontiguousarray(accept, dtype=np.uint8)
        en = np.ascontiguousarray(list(end_tokens), dtype=np.int32)
        assert tr.ndim == 2 and tr.shape[1] == 256 and len(ac) == len(tr)
        g = GuideDesc()
        g.trans, g.accept, g.n_states, g.end_tokens, g.n_end = tr.ctypes.data, ac.ctypes.data, len(tr), en.ctypes.data, len(en)
        rc = lib().pplhip_guide_load(self.h, int(slot), C.byref(g))
        if check:
            self._ck(rc, 0, "guide_load")
        return rc

    def guide_load16(self, slot, trans, accept, end_tokens=(), check=True):
        """guide_load for a wide guide: trans uint16 [n_states, 256] (0xFFFF = dead), up to 4096 states.  Synchronous."""
        tr = np.ascontiguousarray(trans, dtype=np.uint16)
        ac = np.ascontiguousarray(accept, dtype=np.uint8)
        en = np.ascontiguousarray(end_tokens, dtype=np.int32)
        assert tr.ndim == 2 and tr.shape[1] == 256 and len(ac) == len(tr)
        g = GuideDesc()
        g.trans, g.accept, g.n_states, g.end_tokens, g.n_end = tr.ctypes.data, ac.ctypes.data, len(tr), en.ctypes.data, len(en)
        rc = lib().pplhip_guide_load16(self.h, int(slot), C.byref(g))
        if check:
            self._ck(rc, 0, "guide_load16")
        return rc

    def guide_unload(self, slot, check=True):
        rc = lib().pplhip_guide_unload(self.h, int(slot))
        if check:
            self._ck(rc, 0, "guide_unload")
        return rc

    def guide_edit(self, guide_slots, states, logits_ptr=None, check=True):
        """queues the guide masks of the last run's logits (rank 0) for the rows with guide_slots != -1; asynchronous."""
        a = GuideEditArgs()
        gs = np.ascontiguousarray(guide_slots, dtype=np.int32)
        st = np.ascontiguousarray(states, dtype=np.int32)
        assert len(gs) == len(st)
        a.guide_slots, a.states = gs.ctypes.data, st.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = len(gs), self.desc.vocab_size, self.desc.vocab_size
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        rc = lib().pplhip_guide_edit(self.h, logits_ptr, C.byref(a))
        if check:
            self._ck(rc, 0, "guide_edit")
        return rc

    def penalty(self, temperatures, repetition, presence, frequency, batch_slots, req_list_changed=True, logits_ptr=None):
        a = PenaltyArgs()
        B = len(batch_slots)
        t = np.ascontiguousarray(temperatures, dtype=np.float32)
        r = np.ascontiguousarray(repetition, dtype=np.float32)
        p = None if presence is None else np.ascontiguousarray(presence, dtype=np.float32)
        f = None if frequency is None else np.ascontiguousarray(frequency, dtype=np.float32)
        s = np.ascontiguousarray(batch_slots, dtype=np.int64)
        a.temperatures, a.repetition_penalties, a.batch_slots = t.ctypes.data, r.ctypes.data, s.ctypes.data
        a.presence_penalties = None if p is None else p.ctypes.data
        a.frequency_penalties = None if f is None else f.ctypes.data
        a.batch, a.vocab_size, a.req_list_changed = B, self.desc.vocab_size, int(req_list_changed)
        if logits_ptr is None:
            logits_ptr = self.logits_ptr(0)[0]
        self._ck(lib().pplhip_penalty(self.h, logits_ptr, C.byref(a)), 0, "penalty")

    # measurement
    def profile_reset(self, rank=0):
        self._ck(lib().pplhip_profile_reset(self.h, rank), rank, "profile_reset")

    def profile_get(self, cls, rank=0):
        n, ms = C.c_int64(), C.c_double()
        self._ck(lib().pplhip_profile_get(self.h, rank, cls, C.byref(n), C.byref(ms)), rank, "profile_get")
        return n.value, ms.value

    def profile_mode(self, mode):
        self._ck(lib().pplhip_profile_mode(self.h, mode), 0, "profile_mode")

    def mem_info(self, rank=0):
        f, t = C.c_uint64(), C.c_uint64()
        self._ck(lib().pplhip_mem_info(self.h, rank, C.byref(f), C.byref(t)), rank, "mem_info")
        return f.value, t.value


def make_step(token_inputs, seq_starts, start_pos, cache_indices, decoding_batches, max_pages=0, req_list_changed=1):
    tok = np.ascontiguousarray(token_inputs, dtype=np.int64)
    ss = np.ascontiguousarray(seq_starts, dtype=np.int64)
    sp = np.ascontiguousarray(start_pos, dtype=np.int64)
    ci = np.ascontiguousarray(cache_indices, dtype=np.int64)
    B = len(sp)
    seqlens = ss[1:] - ss[:-1]
    kvs = np.zeros(B + 1, dtype=np.int64)
    kvs[1:] = np.cumsum(sp + seqlens)
    st = Step()
    st.batch, st.num_tokens, st.decoding_batches = B, len(tok), decoding_batches
    st.max_seq_len = int(seqlens.max()) if B else 0
    st.max_kv_len = int((sp + seqlens).max()) if B else 0
    st.max_pages = max_pages
    st.token_inputs, st.seq_starts, st.kv_starts = tok.ctypes.data, ss.ctypes.data, kvs.ctypes.data
    st.start_pos, st.cache_indices = sp.ctypes.data, ci.ctypes.data
    st.req_list_changed = req_list_changed
    st._keep = (tok, ss, sp, ci, kvs)
    return st


def shard_weights(weights, desc, tp, rank):
    """Export-side helper: slices an UNSHARDED fp16 weight dict (names of DESIGN.md section 3) for tensor-parallel rank
    `rank` of `tp` -- the partitioning of SURVEY.md 8(e): wqkv / w13 / output on the output dim (heads, inter, vocab),
    wo / w2 on the input dim; embeddings and norms replicated.  (Quantised models are quantised per slice AFTER this.)"""
    H, Hkv, hd = desc.num_heads, desc.num_kv_heads, desc.hidden_dim
    D, inter, V = hd // H, desc.intermediate_dim, desc.vocab_size
    h, hk, it, vl = H // tp, Hkv // tp, inter // tp, V // tp
    out = {}
    for name, w in weights.items():
        w = np.asarray(w)
        if name.endswith("attention.wqkv.weight"):
            w = w.reshape((H + 2 * Hkv) * D, hd)
            q, k, v = w[:H * D], w[H * D:(H + Hkv) * D], w[(H + Hkv) * D:]
            out[name] = np.concatenate([q[rank * h * D:(rank + 1) * h * D], k[rank * hk * D:(rank + 1) * hk * D],
                                        v[rank * hk * D:(rank + 1) * hk * D]], 0)
        elif name.endswith("attention.wo.weight"):
            out[name] = np.ascontiguousarray(w.reshape(hd, H * D)[:, rank * h * D:(rank + 1) * h * D])
        elif name.endswith("feed_forward.w13.weight"):
            w = w.reshape(2 * inter, hd)
            out[name] = np.concatenate([w[rank * it:(rank + 1) * it], w[inter + rank * it:inter + (rank + 1) * it]], 0)
        elif name.endswith("feed_forward.w2.weight"):
            out[name] = np.ascontiguousarray(w.reshape(hd, inter)[:, rank * it:(rank + 1) * it])
        elif name == "output.weight":
            out[name] = np.ascontiguousarray(w.reshape(V, hd)[rank * vl:(rank + 1) * vl])
        else:
            out[name] = w
    return out
