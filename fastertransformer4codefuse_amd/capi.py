"""ctypes binding of libftcf.so (include/ftcf.h).  Fails loudly when the HIP library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("FTCF_LIB_NAME", "libftcf.so"))  # env: kernel-variant experiments

UNIQUE_ID_BYTES = 128
FP32, FP16, BF16 = 0, 1, 2
ACT_NONE, ACT_GELU = 0, 1


class FtcfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libftcf error {code}: {msg}")
        self.code = code


TOKEN_CALLBACK = C.CFUNCTYPE(None, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p)
# ftcf_host_allgather_fn (include/ftcf.h): int (*)(void* user, const void* send, void* recv, size_t bytes_per_rank)
HOST_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
BATCHER_TOKEN_CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_long, C.c_int, C.c_int)


class GptNeoXConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "head_num", "size_per_head", "inter_size", "num_layer", "vocab_size", "rotary_embedding_dim", "start_id",
        "end_id", "tensor_para_size", "tensor_para_rank", "pipeline_para_size", "int8_mode", "dtype",
        "use_gptj_residual", "device")] + [("stream", C.c_void_p), ("comm", C.c_void_p), ("use_hip_graph", C.c_int)]


class GptNeoXWeights(C.Structure):
    _fields_ = [("weights", C.POINTER(C.c_void_p)), ("n_weights", C.c_int),
                ("int8_weights", C.POINTER(C.c_void_p)), ("n_int8_weights", C.c_int),
                ("scales", C.POINTER(C.c_void_p)), ("n_scales", C.c_int)]


class ForwardArgs(C.Structure):
    _fields_ = [
        ("input_ids", C.c_void_p), ("input_lengths", C.c_void_p),
        ("batch_size", C.c_int), ("max_input_len", C.c_int), ("output_len", C.c_int), ("beam_width", C.c_int),
        ("top_k", C.c_void_p), ("n_top_k", C.c_int),
        ("top_p", C.c_void_p), ("n_top_p", C.c_int),
        ("beam_search_diversity_rate", C.c_void_p), ("n_beam_search_diversity_rate", C.c_int),
        ("temperature", C.c_void_p), ("n_temperature", C.c_int),
        ("len_penalty", C.c_void_p), ("n_len_penalty", C.c_int),
        ("repetition_penalty", C.c_void_p), ("n_repetition_penalty", C.c_int),
        ("random_seed", C.c_void_p), ("n_random_seed", C.c_int),
        ("min_length", C.c_void_p), ("n_min_length", C.c_int),
        ("stop_words_list", C.c_void_p), ("stop_words_len", C.c_int),
        ("optional_last_tokens", C.c_void_p), ("optional_last_tokens_count", C.c_int),
        ("return_cum_log_probs", C.c_int),
        ("callback", TOKEN_CALLBACK), ("callback_user", C.c_void_p),
        ("output_ids", C.c_void_p), ("sequence_lengths", C.c_void_p), ("cum_log_probs", C.c_void_p),
        ("debug_logits", C.c_void_p),
        ("output_log_probs", C.c_void_p),
        ("top_logprobs", C.c_int), ("top_logprob_ids", C.c_void_p), ("top_logprob_values", C.c_void_p),
        ("context_log_probs", C.c_void_p),
        ("speculative_tokens", C.c_int), ("speculative_ngram", C.c_int), ("draft_ids", C.c_void_p)]


class SmallmProblem(C.Structure):  # ftcf_smallm_problem
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("scale", C.c_void_p), ("bias", C.c_void_p), ("act", C.c_int),
                ("C", C.c_void_p), ("n", C.c_int), ("k", C.c_int)]


class GemmPlan(C.Structure):  # ftcf_gemm_plan
    _fields_ = [(n, C.c_int) for n in ("family", "tile_rows", "gx", "gy", "slices", "steps_per_slice", "ring", "prefetch",
                                       "two_per_cu", "lone", "grid")]


GEMM_SPLITK, GEMM_ROWS32, GEMM_ONE_WG, GEMM_FOUR_WAVE = 0, 1, 2, 3  # ftcf_gemm_plan.family


class LnGemvArgs(C.Structure):  # ftcf_ln_gemv_args
    _fields_ = [(n, C.c_void_p) for n in ("x", "gamma0", "beta0", "gamma1", "beta1", "W0", "W1", "scale0", "scale1", "bias1",
                                          "out0", "out1")] + [("K", C.c_int), ("N0", C.c_int), ("N1", C.c_int), ("eps", C.c_float)]


class ResidualGemvArgs(C.Structure):  # ftcf_residual_gemv_args
    _fields_ = [(n, C.c_void_p) for n in ("x_a", "x_b", "W_a", "W_b", "scale_a", "scale_b", "bias", "x_in", "out")] + [
        (n, C.c_int) for n in ("N", "K_a", "K_b", "tp", "inplace_variant")]


class DynamicDecodeArgs(C.Structure):  # ftcf_dynamic_decode_args
    _fields_ = [(n, C.c_void_p) for n in (
        "logits", "output_ids", "finished", "seq_len", "cum_log_probs", "output_log_probs", "draw_counter", "pad_count",
        "input_lengths", "stop_words", "optional_last_tokens", "row_len", "top_k", "top_p", "temperature",
        "repetition_penalty", "min_length", "random_seed")] + [
        ("all_finished", C.POINTER(C.c_int)), ("next_step", C.POINTER(C.c_int)), ("form", C.POINTER(C.c_int))] + [
        (n, C.c_int) for n in (
            "n_top_k", "n_top_p", "n_temperature", "n_repetition_penalty", "n_min_length", "n_random_seed", "stop_len",
            "optional_count", "B", "V", "step", "max_input_len", "total_len", "end_id", "return_cum_log_probs", "finish")] + [
        ("top_logprobs", C.c_int), ("top_ids", C.c_void_p), ("top_log_probs", C.c_void_p)]


class LogitProcessArgs(C.Structure):  # ftcf_logit_process_args
    _fields_ = [("struct_size", C.c_int), ("batch_size", C.c_int), ("vocab_size", C.c_int), ("end_id", C.c_int),
                ("logits", C.c_void_p), ("finished", C.c_void_p), ("row_on", C.c_void_p), ("hist", C.c_void_p),
                ("stride_t", C.c_longlong), ("stride_b", C.c_longlong), ("hist_len", C.c_void_p), ("gen_start", C.c_void_p),
                ("hist_len_add", C.c_int), ("bias_stride", C.c_int), ("presence_penalty", C.c_void_p),
                ("frequency_penalty", C.c_void_p), ("min_new_tokens", C.c_void_p), ("bias_ids", C.c_void_p),
                ("bias_values", C.c_void_p), ("n_bias", C.c_void_p), ("bad_words", C.c_void_p), ("bad_words_len", C.c_int),
                ("slice", C.c_int), ("mask", C.c_void_p), ("mask_on", C.c_void_p)]


class VerifyAcceptArgs(C.Structure):  # ftcf_verify_accept_args
    _fields_ = [(n, C.c_int) for n in ("struct_size", "R", "V", "step", "end_id", "max_input_len", "total_len")] + [
        ("logits", C.c_void_p), ("draft", C.c_void_p), ("output_ids", C.c_void_p), ("stop_words", C.c_void_p),
        ("stop_len", C.c_int), ("finished", C.c_void_p), ("seq_len", C.c_void_p), ("cum_log_probs", C.c_void_p),
        ("output_log_probs", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("emitted", C.c_void_p), ("accepted", C.c_void_p), ("tokens", C.c_void_p)]


VERIFY_ACCEPT_WORKSPACE_BYTES = 8192  # FTCF_VERIFY_ACCEPT_WORKSPACE_BYTES


class VerifySampleArgs(C.Structure):  # ftcf_verify_sample_args: ftcf_verify_accept_args, then what the top-k layer draws with
    _fields_ = list(VerifyAcceptArgs._fields_) + [
        ("top_k", C.c_int), ("top_p_topk", C.c_float), ("temperature", C.c_float), ("random_seed", C.c_ulonglong),
        ("draw_counter", C.c_void_p)]


VERIFY_SAMPLE_WORKSPACE_BYTES = 266368  # FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES


class LogitOptions(C.Structure):  # ftcf_logit_options
    _fields_ = [("struct_size", C.c_int), ("presence_penalty", C.c_float), ("frequency_penalty", C.c_float),
                ("min_new_tokens", C.c_int), ("bias_ids", C.POINTER(C.c_int)), ("bias_values", C.POINTER(C.c_float)),
                ("n_bias", C.c_int), ("bad_words", C.POINTER(C.c_int)), ("bad_words_len", C.c_int)]


class BatcherOptions(C.Structure):  # ftcf_batcher_options
    _fields_ = [(n, C.c_int) for n in ("struct_size", "max_batch", "page_tokens", "num_pages", "max_seq_len", "prefix_cache",
                                       "overcommit", "swap_pages")] + [("swap_stage_bytes", C.c_size_t)]


class BeamSearchArgs(C.Structure):  # ftcf_beam_search_args
    _fields_ = [(n, C.c_void_p) for n in (
        "logits", "output_ids", "parent_ids", "finished", "seq_len", "cum_log_probs", "cache_indir", "input_lengths",
        "stop_words", "optional_last_tokens", "temperature", "repetition_penalty", "beam_search_diversity_rate",
        "len_penalty", "min_length")] + [
        (n, C.c_int) for n in (
            "n_temperature", "n_repetition_penalty", "n_beam_search_diversity_rate", "n_len_penalty", "n_min_length",
            "stop_len", "optional_count", "B", "K", "V", "step", "max_input_len", "total_len", "s_max", "end_id")] + [
        ("step_log_probs", C.c_void_p)]


class BeamOptions(C.Structure):  # ftcf_beam_options
    _fields_ = [("struct_size", C.c_int), ("beam_width", C.c_int), ("beam_search_diversity_rate", C.c_float),
                ("len_penalty", C.c_float), ("temperature", C.c_float), ("repetition_penalty", C.c_float),
                ("min_length", C.c_int), ("stop_words", C.POINTER(C.c_int)), ("stop_len", C.c_int),
                ("token_log_probs", C.c_int)]


class ForwardStats(C.Structure):
    _fields_ = [("prefill_ms", C.c_float), ("decode_ms", C.c_float), ("decode_steps", C.c_int),
                ("gemv_ms_sum", C.c_float), ("gemv_launches", C.c_long), ("gemv_bytes", C.c_double),
                ("gemv_kind", C.c_int), ("decode_path", C.c_int), ("prefill_overlap", C.c_int),
                ("prefill_ms_plain", C.c_float), ("prefill_ms_overlapped", C.c_float), ("window_allreduces", C.c_int),
                ("decode_overlap", C.c_int), ("decode_step_ms_plain", C.c_float), ("decode_step_ms_overlapped", C.c_float),
                ("persist_layout", C.c_int),
                ("spec_active", C.c_int), ("spec_steps", C.c_int), ("spec_drafted", C.c_int), ("spec_accepted", C.c_int)]


# the header's name of every mirrored struct (tests/test_capi_abi.py compiles the header and compares size, offsets and field sizes)
STRUCTS = {
    "ftcf_smallm_problem": SmallmProblem, "ftcf_gemm_plan": GemmPlan, "ftcf_ln_gemv_args": LnGemvArgs, "ftcf_residual_gemv_args": ResidualGemvArgs,
    "ftcf_dynamic_decode_args": DynamicDecodeArgs, "ftcf_beam_search_args": BeamSearchArgs,
    "ftcf_logit_process_args": LogitProcessArgs, "ftcf_gptneox_config": GptNeoXConfig, "ftcf_gptneox_weights": GptNeoXWeights,
    "ftcf_forward_args": ForwardArgs, "ftcf_forward_stats": ForwardStats, "ftcf_batcher_options": BatcherOptions,
    "ftcf_logit_options": LogitOptions, "ftcf_beam_options": BeamOptions}

# ... and of the structs the header declares with a tag (`typedef struct NAME { ... } NAME;`): tests/test_speculative_scope_host.py
# compares their layouts the same way
TAGGED_STRUCTS = {"ftcf_verify_accept_args": VerifyAcceptArgs, "ftcf_verify_sample_args": VerifySampleArgs}

# The prototype of every entry point: name -> (restype, argtypes), written out by hand in the header's order and held to the
# header by tests/test_capi_abi.py.  int / ftcf_dtype / ftcf_act -> I, float -> F, size_t -> Z, long -> L, unsigned long long -> U;
# every pointer, array parameter and handle -> P (c_void_p takes None, an address as int, byref(), ctypes arrays and pointers).
I, F, Z, L, U, P = C.c_int, C.c_float, C.c_size_t, C.c_long, C.c_ulonglong, C.c_void_p
_LAYOUT = [P, Z, Z, P]                       # (src, K, N, dst)
_SUBMIT = [P, P, I, I, I, F, F, F, U, P, I]  # (b, prompt_ids, prompt_len, max_new_tokens, top_k, top_p, temperature,
                                             #  repetition_penalty, seed, stop_words, stop_len)
_SUBMIT_BEAM = [P, P, I, I, I, F, F, F, F]   # (b, prompt_ids, prompt_len, max_new_tokens, beam_width, beam_search_diversity_rate,
                                             #  len_penalty, temperature, repetition_penalty)
PROTOTYPES = {
    "ftcf_last_error": (C.c_char_p, []),
    "ftcf_version": (I, []),
    "ftcf_device_count": (I, []),
    "ftcf_symmetric_quantize_int8": (I, [P, I, Z, Z, Z, P, P]),
    "ftcf_symmetric_quantize_int8_device": (I, [P, I, Z, Z, Z, P, P, P, Z, P]),
    "ftcf_symmetric_quantize_int8_device_workspace": (Z, [Z, Z]),
    "ftcf_int8_rowmajor_to_tiled": (I, _LAYOUT),
    "ftcf_int8_tiled_to_rowmajor": (I, _LAYOUT),
    "ftcf_int8_cuda_sm80_to_rowmajor": (I, _LAYOUT),
    "ftcf_int8_rowmajor_to_cuda_sm80": (I, _LAYOUT),
    "ftcf_fp16_rowmajor_to_tiled": (I, [P, Z, Z, P, P]),
    "ftcf_fpA_intB_gemm": (I, [P, P, P, P, I, P, I, I, I, P]),
    "ftcf_fp16_gemm": (I, [P, P, P, I, P, I, I, I, P]),
    "ftcf_gemm_tiled_plan": (I, [I, I, I, I, I, C.POINTER(GemmPlan)]),
    "ftcf_lm_head": (I, [P, P, P, I, I, I, I, P]),
    "ftcf_lm_head_layernorm": (I, [P, P, P, P, F, P, P, I, I, I, I, P]),
    "ftcf_lm_head_log_probs": (I, [P, P, P, P, P, I, I, I, P]),
    "ftcf_gemm_smallm_group": (I, [C.POINTER(SmallmProblem), I, I, I, P, Z, Z, P, P, P]),
    "ftcf_gemm_smallm_workspace_bytes": (Z, [I, I, I, I]),
    "ftcf_gemm_smallm_ticket_bytes": (Z, []),
    "ftcf_residual_dual_layernorm": (I, [P, P, P, P, I, I, P, P, P, P, P, P, I, I, F, I, I, P]),
    "ftcf_add_bias_residual": (I, [P, P, P, P, I, I, P]),
    "ftcf_ln_gemv": (I, [P, I, I, I, P]),
    "ftcf_residual_gemv": (I, [P, I, I, I, P, Z, P, I, I, P]),
    "ftcf_residual_gemv_workspace_bytes": (Z, [I, I, I]),
    "ftcf_layernorm": (I, [P, P, P, P, I, I, F, I, P]),
    "ftcf_add_bias_attn_ffn_residual": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "ftcf_masked_multihead_attention": (I, [P] * 8 + [I] * 6 + [P, P, Z, P]),
    "ftcf_masked_multihead_attention_workspace": (Z, [I, I, I, I]),
    "ftcf_masked_multihead_attention_beams": (I, [I] + [P] * 9 + [I] * 9 + [P, P, Z, P]),
    "ftcf_context_attention": (I, [P] * 5 + [I] * 6 + [P, P]),
    "ftcf_context_attention_range": (I, [I] + [P] * 5 + [I] * 9 + [P, P]),
    "ftcf_verify_attention": (I, [P] * 4 + [I] * 7 + [P, P, Z, P]),
    "ftcf_verify_attention_workspace": (Z, [I, I, I, I]),
    "ftcf_ngram_draft": (I, [P, I, I, I, P, P, P]),
    "ftcf_verify_accept": (I, [P, P]),
    "ftcf_verify_sample": (I, [P, P]),
    "ftcf_paged_attention": (I, [P] * 7 + [I] * 7 + [P, P]),
    "ftcf_scatter_kv_to_pages": (I, [P] * 5 + [I] * 6 + [Z, Z, P]),
    "ftcf_gather_pages_to_kv": (I, [P] * 5 + [I] * 6 + [Z, Z, P]),
    "ftcf_pages_pack": (I, [P] * 4 + [I] * 5 + [Z, P]),
    "ftcf_pages_unpack": (I, [P] * 4 + [I] * 5 + [Z, P]),
    "ftcf_dynamic_decode_step": (I, [P, P]),
    "ftcf_beam_search_step": (I, [P, P]),
    "ftcf_logit_process": (I, [P, P]),
    "ftcf_comm_get_unique_id": (I, [P]),
    "ftcf_comm_init": (I, [P, I, I, I, P]),
    "ftcf_comm_destroy": (I, [P]),
    "ftcf_comm_local_unique_id": (I, [P]),
    "ftcf_comm_init_local": (I, [P, I, I, I, P]),
    "ftcf_comm_init_host_exchange": (I, [I, I, I, HOST_ALLGATHER, P, P]),
    "ftcf_comm_allreduce_sum": (I, [P, P, Z, I, P]),
    "ftcf_comm_allgather": (I, [P, P, Z, I, P]),
    "ftcf_gptneox_create": (I, [P, P, P]),
    "ftcf_gptneox_forward": (I, [P, P]),
    "ftcf_gptneox_begin": (I, [P, P]),
    "ftcf_gptneox_step": (I, [P, I, P]),
    "ftcf_gptneox_finish": (I, [P]),
    "ftcf_gptneox_beam_log_probs": (I, [P, P, Z]),
    "ftcf_gptneox_get_stats": (I, [P, P]),
    "ftcf_gptneox_set_profiling": (I, [P, I]),
    "ftcf_gptneox_set_speculative_scope": (I, [P, I]),
    "ftcf_gptneox_set_speculative_sampling": (I, [P, I]),
    "ftcf_gptneox_destroy": (I, [P]),
    "ftcf_batcher_create": (I, [P, I, I, I, I, P]),
    "ftcf_batcher_create_ex": (I, [P, I, I, I, I, I, P]),
    "ftcf_batcher_create_opts": (I, [P, P, P]),
    "ftcf_batcher_preempt_stats": (I, [P] * 9),
    "ftcf_batcher_prefix_stats": (I, [P] * 9),
    "ftcf_batcher_clear_prefix_cache": (I, [P]),
    "ftcf_batcher_submit": (I, [P, P, I, I, I, F, F, U, P]),
    "ftcf_batcher_submit_ex": (I, _SUBMIT + [P]),
    "ftcf_batcher_submit_opts": (I, _SUBMIT + [P, P]),
    "ftcf_batcher_submit_n": (I, _SUBMIT + [P, I, P]),
    "ftcf_batcher_fork_stats": (I, [P] * 5),
    "ftcf_batcher_set_token_mask": (I, [P, L, P, I]),
    "ftcf_batcher_submit_beam": (I, _SUBMIT_BEAM + [P]),
    "ftcf_batcher_submit_beam_ex": (I, _SUBMIT_BEAM + [I, P, I, P]),
    "ftcf_batcher_beam_result": (I, [P, L, P, P, P, I, P, P]),
    "ftcf_batcher_submit_beam_opts": (I, [P, P, I, I, C.POINTER(BeamOptions), C.POINTER(C.c_long)]),
    "ftcf_batcher_beam_result_ex": (I, [P, L, P, P, P, P, I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ftcf_batcher_step": (I, [P, P, P, P, I, P]),
    "ftcf_batcher_step_ex": (I, [P, P, P, P, P, I, P]),
    "ftcf_batcher_step_top": (I, [P, P, P, P, P, I, P, P, I, P]),
    "ftcf_batcher_set_token_callback": (I, [P, BATCHER_TOKEN_CALLBACK, P]),
    "ftcf_batcher_status": (I, [P] * 4),
    "ftcf_batcher_cancel": (I, [P, L, P]),
    "ftcf_batcher_destroy": (I, [P]),
}
EXPORTED = list(PROTOTYPES)  # every symbol include/ftcf.h declares

_lib = None


def lib():
    """Loads libftcf.so.  Import torch first when both live in one process so that a single HIP runtime is shared."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FtcfError(-5, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc, gfx950). There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if hasattr(_lib, name):  # (FTCF_LIB_NAME may name an older build: the call itself then fails)
                fn = getattr(_lib, name)
                fn.restype, fn.argtypes = restype, argtypes
    return _lib


def check(code):
    if code != 0:
        raise FtcfError(code, lib().ftcf_last_error().decode("utf-8", "replace"))


def device_count():
    return int(lib().ftcf_device_count())


def require_gpu():
    if device_count() <= 0:
        raise FtcfError(-5, "no HIP device visible; the MI355X engine has no CPU fallback")


def vp(x):
    """data pointer of a torch tensor / numpy array / int / None as c_void_p"""
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)
