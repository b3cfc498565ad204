"""ctypes binding of libctok.so (the C ABI declared in include/ctok.h).

No CPU fallback: if the shared library is missing the import fails loudly, and encode calls on
a machine without a HIP device raise DeviceError.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTOK_LIB", os.path.join(_HERE, "libctok.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "complexity_tokenizer: native library not found at %s -- build it with "
        "`make -C complexity-tokenizer_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)


def _share_torch_hip_runtime():
    """torch wheels bundle their own HIP runtime with the same SONAME (libamdhip64.so.7) as
    /opt/rocm's.  Whichever copy loads first serves libctok.so; if /opt/rocm's came first and torch
    were imported later, torch would load its copy next to it and two HIP runtimes in one process
    fail to share the device.  Preloading torch's copy (without importing torch) makes every HIP
    user in the process resolve to one runtime.  CTOK_NO_TORCH_HIP=1 disables this."""
    if os.environ.get("CTOK_NO_TORCH_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


_share_torch_hip_runtime()
lib = ctypes.CDLL(LIB_PATH)

CTOK_OK = 0
CTOK_E_IO = -1
CTOK_E_PARSE = -2
CTOK_E_UNSUPPORTED = -3
CTOK_E_ARG = -4
CTOK_E_CAPACITY = -5
CTOK_E_PANIC = -6
CTOK_E_DEVICE = -7
CTOK_E_NOTFOUND = -8
CTOK_F_TIMING = 1


class Exec(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("stream", ctypes.c_void_p), ("flags", ctypes.c_uint32),
                ("devices", ctypes.POINTER(ctypes.c_int)), ("n_devices", ctypes.c_int),
                ("chunk_mb", ctypes.c_uint32), ("host_threads", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_device", ctypes.c_double), ("ms_pretok", ctypes.c_double),
                ("ms_bpe_short", ctypes.c_double), ("ms_bpe_long", ctypes.c_double),
                ("ms_emit", ctypes.c_double), ("ms_h2d", ctypes.c_double),
                ("ms_d2h", ctypes.c_double), ("bytes_in", ctypes.c_uint64), ("bytes_norm", ctypes.c_uint64),
                ("docs", ctypes.c_uint64), ("pieces", ctypes.c_uint64), ("long_pieces", ctypes.c_uint64),
                ("tokens", ctypes.c_uint64), ("nfc_docs", ctypes.c_uint64), ("ms_segment", ctypes.c_double),
                ("ms_bpe_lo", ctypes.c_double), ("ms_bpe_hi", ctypes.c_double),
                ("class_bytes", ctypes.c_uint64 * 4), ("class_ids", ctypes.c_uint64 * 4),
                ("ms_bpe_med", ctypes.c_double), ("workspace_bytes", ctypes.c_uint64),
                ("long_rounds", ctypes.c_uint64)]

    def as_dict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if isinstance(v, ctypes.Array) else v
        return d


class DecodeStats(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_double), ("ms_device", ctypes.c_double), ("ms_len", ctypes.c_double),
                ("ms_gather", ctypes.c_double), ("ms_clean", ctypes.c_double), ("ms_h2d", ctypes.c_double),
                ("ms_d2h", ctypes.c_double), ("ids", ctypes.c_uint64), ("docs", ctypes.c_uint64),
                ("bytes_raw", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64), ("direct", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


CTOK_D_SKIP_SPECIAL = 1
CTOK_D_CLEANUP = 2

CTOK_P_ADD_SPECIAL = 1
CTOK_P_PAIRS = 2
CTOK_P_TRUNCATE = 4
CTOK_P_PAD_LONGEST = 8
CTOK_P_PAD_TO_MAX = 16
CTOK_P_PAD_LEFT = 32
CTOK_P_PAD_ID = 64
CTOK_P_NO_POSTPROCESS = 128
CTOK_P_WINDOWS = 256
CTOK_PP_SEQUENCE = 0xFFFFFFFF


class PadOpts(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("max_length", ctypes.c_uint64)]


class Tables(ctypes.Structure):  # include/ctok.h ctok_tables
    _fields_ = [("vocab", ctypes.c_char_p), ("vocab_off", ctypes.c_void_p), ("vocab_id", ctypes.c_void_p),
                ("n_vocab", ctypes.c_uint64), ("merge_left", ctypes.c_void_p), ("merge_right", ctypes.c_void_p),
                ("n_merges", ctypes.c_uint64), ("added", ctypes.c_char_p), ("added_off", ctypes.c_void_p),
                ("added_id", ctypes.c_void_p), ("added_flags", ctypes.c_void_p), ("n_added", ctypes.c_uint64),
                ("nfc", ctypes.c_int), ("add_prefix_space", ctypes.c_int)]


class TableProps(ctypes.Structure):  # include/ctok.h ctok_table_props
    _fields_ = [(k, ctypes.c_int) for k in ("narrow", "compact", "short_packed", "ids16", "dev_narrow",
                                            "dev_short_packed", "last_rec16", "last_wire16", "dev_mid_packed")]


class TrainerConfig(ctypes.Structure):  # include/ctok_trainer.h
    _fields_ = [("vocab_size", ctypes.c_uint64), ("min_frequency", ctypes.c_uint32),
                ("min_word_length", ctypes.c_uint64), ("inl_alpha", ctypes.c_float), ("inl_beta", ctypes.c_float),
                ("inl_gate", ctypes.c_float), ("inl_mu_target", ctypes.c_float),
                ("inl_velocity_max", ctypes.c_float), ("inl_beta_max", ctypes.c_float),
                ("special", ctypes.c_char_p), ("special_off", ctypes.POINTER(ctypes.c_uint64)),
                ("n_special", ctypes.c_uint64), ("device", ctypes.c_int)]


class TrainerCountStats(ctypes.Structure):  # include/ctok_trainer.h ctok_trainer_count_info
    _fields_ = [("pieces", ctypes.c_uint64), ("words", ctypes.c_uint64), ("unique_words", ctypes.c_uint64),
                ("chunks", ctypes.c_uint64), ("host_chunks", ctypes.c_uint64), ("rerun_chunks", ctypes.c_uint64),
                ("bytes_d2h", ctypes.c_uint64), ("ms_device", ctypes.c_double), ("ms_host", ctypes.c_double)]


class BpeTrainerConfig(ctypes.Structure):  # include/ctok_bpe_trainer.h
    _fields_ = [("vocab_size", ctypes.c_uint64), ("min_frequency", ctypes.c_uint32),
                ("special", ctypes.c_char_p), ("special_off", ctypes.POINTER(ctypes.c_uint64)),
                ("n_special", ctypes.c_uint64), ("end_of_word_suffix", ctypes.c_char_p),
                ("continuing_subword_prefix", ctypes.c_char_p), ("show_progress", ctypes.c_int),
                ("device", ctypes.c_int)]


class BpeStrings(ctypes.Structure):  # include/ctok_bpe_trainer.h ctok_bpe_strings
    _fields_ = [("bytes", ctypes.c_void_p), ("off", ctypes.POINTER(ctypes.c_uint64)), ("n", ctypes.c_uint64)]


class BpeTrainerStats(ctypes.Structure):  # include/ctok_bpe_trainer.h ctok_bpe_trainer_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("words", "unique_words", "initial_symbols", "merges", "table_capacity",
                                               "rebuilds", "chunks", "host_chunks", "rerun_chunks")] + \
               [(k, ctypes.c_double) for k in ("ms_count", "ms_pairs", "ms_best", "ms_merges", "ms_host")]


class WpTrainerConfig(ctypes.Structure):  # include/ctok_wordpiece.h
    _fields_ = [("vocab_size", ctypes.c_uint64), ("min_frequency", ctypes.c_uint32),
                ("special", ctypes.c_char_p), ("special_off", ctypes.POINTER(ctypes.c_uint64)),
                ("n_special", ctypes.c_uint64), ("continuing_subword_prefix", ctypes.c_char_p),
                ("max_input_chars_per_word", ctypes.c_uint64), ("device", ctypes.c_int)]


class WpTrainerStats(ctypes.Structure):  # include/ctok_wordpiece.h ctok_wp_trainer_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("words", "unique_words", "initial_vocab", "merges", "table_capacity",
                                               "rebuilds", "walked_words", "chunks", "host_chunks", "rerun_chunks",
                                               "lowered_chunks")] + \
               [(k, ctypes.c_double) for k in ("ms_count", "ms_match", "ms_pairs", "ms_add", "ms_walk", "ms_best",
                                               "ms_host")]


class UniTrainerConfig(ctypes.Structure):  # include/ctok_unigram.h
    _fields_ = [("vocab_size", ctypes.c_uint64), ("special", ctypes.c_char_p),
                ("special_off", ctypes.POINTER(ctypes.c_uint64)), ("n_special", ctypes.c_uint64),
                ("initial_vocab_size", ctypes.c_uint64), ("shrinking_factor", ctypes.c_double),
                ("n_iterations", ctypes.c_uint64), ("max_piece_length", ctypes.c_uint64), ("device", ctypes.c_int)]


class UniTrainerStats(ctypes.Structure):  # include/ctok_unigram.h ctok_uni_trainer_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("sentences", "chars", "seed_vocab", "iterations")] + \
               [("vocab_sizes", ctypes.POINTER(ctypes.c_uint64))] + \
               [(k, ctypes.c_uint64) for k in ("window", "table_capacity", "chunks", "rerun_chunks")] + \
               [(k, ctypes.c_double) for k in ("ms_text", "ms_count", "ms_lattice", "ms_viterbi", "ms_host")]


class NormStep(ctypes.Structure):  # include/ctok_normalizer.h ctok_norm_step
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("a", ctypes.c_void_p), ("a_len", ctypes.c_uint64),
                ("b", ctypes.c_void_p), ("b_len", ctypes.c_uint64)]


class NormInfo(ctypes.Structure):  # include/ctok_normalizer.h ctok_normalizer_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("steps", "steps_changed", "bytes_in", "bytes_out", "bytes_peak")]


class PretokStep(ctypes.Structure):  # include/ctok_pretokenizer.h ctok_pretok_step
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("a", ctypes.c_void_p), ("a_len", ctypes.c_uint64),
                ("cp", ctypes.c_uint32)]


class PretokInfo(ctypes.Structure):  # include/ctok_pretokenizer.h ctok_pretokenizer_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("steps", "steps_rewriting", "bytes_in", "bytes_out", "bytes_peak", "words")]


class PretokSplitInfo(ctypes.Structure):  # include/ctok_pretokenizer.h ctok_pretok_split_info
    _fields_ = [("gate", ctypes.c_int32), ("n_symbols", ctypes.c_uint32), ("n_states", ctypes.c_uint32), ("n_nfa", ctypes.c_uint32),
                ("cyclic", ctypes.c_uint32), ("table_in_lds", ctypes.c_uint32), ("longest_match", ctypes.c_uint64),
                ("table_bytes", ctypes.c_uint64), ("reason", ctypes.c_char * 256)]


class PretokLimits(ctypes.Structure):  # include/ctok_pretokenizer.h ctok_pretok_limits_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("max_regex_run", "max_symbols", "max_states", "max_nfa_states", "lds_table_bytes",
                                               "scan_tile_bytes", "scan_round_bytes")]


class DecStep(ctypes.Structure):  # include/ctok_decoder.h ctok_dec_step
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("a", ctypes.c_void_p), ("a_len", ctypes.c_uint64),
                ("b", ctypes.c_void_p), ("b_len", ctypes.c_uint64), ("cp", ctypes.c_uint32), ("start", ctypes.c_uint64),
                ("stop", ctypes.c_uint64)]


class DecInfo(ctypes.Structure):  # include/ctok_decoder.h ctok_decoder_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("steps", "passes", "docs", "tokens", "bytes_in", "bytes_out", "bytes_peak")]


class PpStep(ctypes.Structure):  # include/ctok_postprocessor.h ctok_pp_step
    _fields_ = [("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("single", ctypes.c_void_p), ("single_len", ctypes.c_uint64),
                ("pair", ctypes.c_void_p), ("pair_len", ctypes.c_uint64), ("tok_bytes", ctypes.c_void_p), ("tok_off", ctypes.c_void_p),
                ("tok_id", ctypes.c_void_p), ("n_tok", ctypes.c_uint64), ("id_a", ctypes.c_uint32), ("id_b", ctypes.c_uint32)]


class PpBatch(ctypes.Structure):  # ctok_pp_batch
    _fields_ = [("ids", ctypes.c_void_p), ("off", ctypes.c_void_p), ("pair_ids", ctypes.c_void_p), ("pair_off", ctypes.c_void_p),
                ("has_pair", ctypes.c_void_p), ("n_rows", ctypes.c_uint64)]


class PpOpts(ctypes.Structure):  # ctok_pp_opts
    _fields_ = [("truncate", ctypes.c_uint32), ("strategy", ctypes.c_uint32), ("truncate_to", ctypes.c_uint64),
                ("padded", ctypes.c_uint32), ("pad_left", ctypes.c_uint32), ("pad_to", ctypes.c_uint64), ("pad_id", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class PpOut(ctypes.Structure):  # ctok_pp_out
    _fields_ = [("ids", ctypes.c_void_p), ("ids_cap", ctypes.c_uint64), ("off", ctypes.c_void_p), ("attention_mask", ctypes.c_void_p),
                ("token_type_ids", ctypes.c_void_p), ("special_tokens_mask", ctypes.c_void_p), ("row_len", ctypes.c_void_p),
                ("n_ids", ctypes.c_uint64), ("width", ctypes.c_uint64)]


class PpInfo(ctypes.Structure):  # ctok_postprocessor_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("steps", "items_single", "items_pair", "rows", "ids_in", "pair_ids_in", "ids_out",
                                               "width")]


class PipelineTables(ctypes.Structure):  # include/ctok_pipeline.h ctok_pipeline_tables
    _fields_ = [("vocab_bytes", ctypes.c_void_p), ("vocab_off", ctypes.c_void_p), ("vocab_id", ctypes.c_void_p), ("n_vocab", ctypes.c_uint64),
                ("merge_bytes", ctypes.c_void_p), ("merge_off", ctypes.c_void_p), ("n_merge_strings", ctypes.c_uint64),
                ("added_bytes", ctypes.c_void_p), ("added_off", ctypes.c_void_p), ("added_id", ctypes.c_void_p),
                ("added_flags", ctypes.c_void_p), ("n_added", ctypes.c_uint64)]


class PipelineLimits(ctypes.Structure):  # ctok_pipeline_limits_t
    _fields_ = [("tier1", ctypes.c_uint32), ("tier2", ctypes.c_uint32), ("max_word_symbols", ctypes.c_uint64),
                ("max_flagged_word_bytes", ctypes.c_uint64), ("max_added_tokens", ctypes.c_uint64),
                ("max_added_token_bytes", ctypes.c_uint64), ("max_merges", ctypes.c_uint64), ("max_added_group_bytes", ctypes.c_uint64),
                ("max_batch_bytes", ctypes.c_uint64)]


class PipelineEncodings(ctypes.Structure):  # ctok_pipeline_encodings
    _fields_ = [(k, ctypes.c_void_p) for k in ("ids", "type_ids", "special_tokens_mask", "row_off", "offsets", "word_ids", "seq_ids",
                                               "seq_off", "n_a")] + [("n_rows", ctypes.c_uint64)]


class PipelineEncodingsDevice(ctypes.Structure):  # ctok_pipeline_encodings_device
    _fields_ = [("ids", ctypes.c_void_p), ("type_ids", ctypes.c_void_p), ("special_tokens_mask", ctypes.c_void_p),
                ("cells_cap", ctypes.c_uint64), ("row_off", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("word_ids", ctypes.c_void_p),
                ("seq_ids", ctypes.c_void_p), ("ids_cap", ctypes.c_uint64), ("seq_off", ctypes.c_void_p), ("n_a", ctypes.c_void_p), ("n_cells", ctypes.c_uint64),
                ("n_ids", ctypes.c_uint64)]


class PipelineEncodingLimits(ctypes.Structure):  # ctok_pipeline_encoding_limits_t
    _fields_ = [("max_find_work", ctypes.c_uint64), ("max_special_tokens", ctypes.c_uint64), ("max_find_compares", ctypes.c_uint64)]


class PipelineEncodingInfo(ctypes.Structure):  # ctok_pipeline_encoding_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("rows", "sequences", "words", "ids", "cells", "max_find_work")]


CTOK_PIPELINE_ENCODING_STAGES = 3


class PipelineWindowOpts(ctypes.Structure):  # ctok_pipeline_window_opts
    _fields_ = [("flags", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("max_length", ctypes.c_uint64), ("stride", ctypes.c_uint64),
                ("want", ctypes.c_uint32)]


class PipelineWindows(ctypes.Structure):  # ctok_pipeline_windows
    _fields_ = [(k, ctypes.c_void_p) for k in ("ids", "attention_mask", "type_ids", "special_tokens_mask", "offsets", "word_ids",
                                               "sequence_ids", "win_len", "win_row", "win_start", "win_off_len", "win_seq_len", "row_win")] \
        + [(k, ctypes.c_uint64) for k in ("n_rows", "n_windows", "width")]


class PipelineWindowsDevice(ctypes.Structure):  # ctok_pipeline_windows_device
    _fields_ = [(k, ctypes.c_void_p) for k in ("ids", "attention_mask", "type_ids", "special_tokens_mask", "offsets", "word_ids",
                                               "sequence_ids")] + [("cap", ctypes.c_uint64)] \
        + [(k, ctypes.c_void_p) for k in ("win_len", "win_row", "win_start", "win_off_len", "win_seq_len")] + [("win_cap", ctypes.c_uint64)] \
        + [("row_win", ctypes.c_void_p), ("n_windows", ctypes.c_uint64), ("width", ctypes.c_uint64)]


class PipelineWindowInfo(ctypes.Structure):  # ctok_pipeline_window_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("rows", "windows", "width", "bytes_written")]


CTOK_PIPELINE_WINDOW_STAGES = 2
CTOK_PIPELINE_WIN_OFFSETS, CTOK_PIPELINE_WIN_WORD_IDS, CTOK_PIPELINE_WIN_SEQUENCE_IDS = 1, 2, 4


class PipelineInfo(ctypes.Structure):  # ctok_pipeline_info
    _fields_ = [(k, ctypes.c_uint64) for k in ("texts", "bytes_in", "bytes_normalized", "bytes_words", "words", "segments", "symbols",
                                               "ids", "tier2_segments", "tier3_segments", "max_segment_symbols")]


CTOK_PIPELINE_TOKENIZE = 1
CTOK_PIPELINE_STAGES = 6

_p = ctypes.c_void_p
_u64 = ctypes.c_uint64
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_f64p = ctypes.POINTER(ctypes.c_double)
_sz = ctypes.c_size_t

SIGS = {
    "ctok_last_error": (ctypes.c_char_p, []),
    "ctok_version": (ctypes.c_char_p, []),
    "ctok_create_from_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_p)]),
    "ctok_create_from_buffer": (ctypes.c_int, [ctypes.c_char_p, _sz, ctypes.POINTER(_p)]),
    "ctok_create_from_tables": (ctypes.c_int, [ctypes.POINTER(Tables), ctypes.POINTER(_p)]),
    "ctok_destroy": (None, [_p]),
    "ctok_vocab_size": (_u64, [_p]),
    "ctok_token_to_id": (ctypes.c_int, [_p, ctypes.c_char_p, _sz, _u32p]),
    "ctok_id_to_token": (ctypes.c_int, [_p, ctypes.c_uint32, ctypes.c_char_p, _sz, ctypes.POINTER(_sz)]),
    "ctok_num_special_tokens": (_u64, [_p]),
    "ctok_special_token": (ctypes.c_int, [_p, _u64, ctypes.c_char_p, _sz, ctypes.POINTER(_sz), _u32p]),
    "ctok_ids_bound": (_u64, [_p, _u64, _u64]),
    "ctok_num_piece_added_tokens": (_u64, [_p]),
    "ctok_piece_can_contain": (ctypes.c_int, [ctypes.c_char_p, _sz]),
    "ctok_get_table_props": (ctypes.c_int, [_p, ctypes.c_int, ctypes.POINTER(TableProps)]),
    "ctok_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, _p, _u64, _p, ctypes.POINTER(Exec), ctypes.POINTER(Stats)]),
    "ctok_encode_batch_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, _p, _u64, _p, _u64p, ctypes.POINTER(Exec),
                                                ctypes.POINTER(Stats)]),
    "ctok_device_count": (ctypes.c_int, []),
    "ctok_encode_padded": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(PadOpts), _p, _p, _p, _p, _u64, _p, _u64p,
                                          ctypes.POINTER(Exec), ctypes.POINTER(Stats)]),
    "ctok_encode_padded_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, ctypes.POINTER(PadOpts), _p, _p, _p, _p, _u64, _p,
                                                 _u64p, ctypes.POINTER(Exec), ctypes.POINTER(Stats)]),
    "ctok_encode_windows": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(PadOpts), _u64, _p, _p, _p, _p, _u64, _p, _p,
                                           _p, _u64, _p, _u64p, _u64p, ctypes.POINTER(Exec), ctypes.POINTER(Stats)]),
    "ctok_encode_windows_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, ctypes.POINTER(PadOpts), _u64, _p, _p, _p, _p,
                                                  _u64, _p, _p, _p, _u64, _p, _u64p, _u64p, ctypes.POINTER(Exec),
                                                  ctypes.POINTER(Stats)]),
    "ctok_model_max_length": (_u64, [_p]),
    "ctok_pad_id": (ctypes.c_uint32, [_p]),
    "ctok_num_special_tokens_to_add": (_u64, [_p, ctypes.c_int]),
    "ctok_post_processor": (ctypes.c_int, [_p, _u32p, _u64, ctypes.POINTER(ctypes.c_int64)]),
    "ctok_encode_offsets": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, _p, _u64, _p, ctypes.POINTER(Exec)]),
    "ctok_decode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_uint32, _p, _u64, _p, ctypes.POINTER(Exec),
                                         ctypes.POINTER(DecodeStats)]),
    "ctok_decode_batch_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, ctypes.c_uint32, _p, _u64, _p, _u64p,
                                                ctypes.POINTER(Exec), ctypes.POINTER(DecodeStats)]),
    # include/ctok_trainer.h
    "ctok_trainer_create": (ctypes.c_int, [ctypes.POINTER(TrainerConfig), ctypes.POINTER(_p)]),
    "ctok_trainer_destroy": (None, [_p]),
    "ctok_trainer_count": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_int]),
    "ctok_trainer_clear_counts": (ctypes.c_int, [_p, ctypes.c_int]),
    "ctok_trainer_train": (ctypes.c_int, [_p, ctypes.c_int]),
    "ctok_trainer_train_words": (ctypes.c_int, [_p, _p, _p, _p, _u64]),
    "ctok_trainer_vocab_size": (_u64, [_p]),
    "ctok_trainer_num_merges": (_u64, [_p]),
    "ctok_trainer_json": (ctypes.c_int, [_p, ctypes.c_char_p, _sz, ctypes.POINTER(_sz)]),
    "ctok_trainer_save": (ctypes.c_int, [_p, ctypes.c_char_p]),
    "ctok_trainer_initial_pairs": (ctypes.c_int, [_p, _p, _p, _p, _u64, _u64p]),
    "ctok_trainer_timing": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]),
    "ctok_trainer_word_counts": (ctypes.c_int, [_p, ctypes.c_int, _p, _u64, _p, _p, _u64, _u64p, _u64p]),
    "ctok_trainer_count_stats": (ctypes.c_int, [_p, ctypes.POINTER(TrainerCountStats)]),
    # include/ctok_bpe_trainer.h
    "ctok_bpe_trainer_create": (ctypes.c_int, [ctypes.POINTER(BpeTrainerConfig), ctypes.POINTER(_p)]),
    "ctok_bpe_trainer_destroy": (None, [_p]),
    "ctok_bpe_trainer_count": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_bpe_trainer_train": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_bpe_trainer_train_words": (ctypes.c_int, [_p, _p, _p, _p, _u64]),
    "ctok_bpe_trainer_vocab_size": (_u64, [_p]),
    "ctok_bpe_trainer_num_merges": (_u64, [_p]),
    "ctok_bpe_trainer_result": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u32p),
                                               ctypes.POINTER(BpeStrings)]),
    "ctok_bpe_trainer_word_counts": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u32p)]),
    "ctok_bpe_trainer_stats": (ctypes.c_int, [_p, ctypes.POINTER(BpeTrainerStats)]),
    "ctok_bpe_trainer_symbols": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings)]),
    "ctok_bpe_trainer_pair_counts": (ctypes.c_int, [_p, ctypes.POINTER(_u32p), ctypes.POINTER(_u32p),
                                                    ctypes.POINTER(ctypes.POINTER(ctypes.c_int64)), _u64p]),
    # include/ctok_wordpiece.h
    "ctok_wp_trainer_create": (ctypes.c_int, [ctypes.POINTER(WpTrainerConfig), ctypes.POINTER(_p)]),
    "ctok_wp_trainer_destroy": (None, [_p]),
    "ctok_wp_trainer_count": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_wp_trainer_train": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_wp_trainer_train_words": (ctypes.c_int, [_p, _p, _p, _p, _u64]),
    "ctok_wp_trainer_vocab_size": (_u64, [_p]),
    "ctok_wp_trainer_result": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u32p),
                                              ctypes.POINTER(BpeStrings)]),
    "ctok_wp_trainer_word_counts": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u32p)]),
    "ctok_wp_trainer_tokens": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(BpeStrings),
                                              ctypes.POINTER(_u64p)]),
    "ctok_wp_trainer_stats": (ctypes.c_int, [_p, ctypes.POINTER(WpTrainerStats)]),
    "ctok_wp_trainer_pair_counts": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(BpeStrings),
                                                   ctypes.POINTER(ctypes.POINTER(ctypes.c_int64))]),
    "ctok_wp_model_create": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_char_p, ctypes.c_char_p, _u64, ctypes.c_int,
                                            ctypes.POINTER(_p)]),
    "ctok_wp_model_destroy": (None, [_p]),
    "ctok_wp_model_vocab_size": (_u64, [_p]),
    "ctok_wp_model_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(_u32p), ctypes.POINTER(_u64p)]),
    "ctok_lowercase": (ctypes.c_int, [_p, _p, _u64, ctypes.c_int, _p, _u64, _p]),
    # include/ctok_unigram.h
    "ctok_uni_trainer_create": (ctypes.c_int, [ctypes.POINTER(UniTrainerConfig), ctypes.POINTER(_p)]),
    "ctok_uni_trainer_destroy": (None, [_p]),
    "ctok_uni_trainer_train": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_uni_trainer_train_sentences": (ctypes.c_int, [_p, _p, _p, _u64]),
    "ctok_uni_trainer_vocab_size": (_u64, [_p]),
    "ctok_uni_trainer_result": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_f64p)]),
    "ctok_uni_trainer_sentences": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings)]),
    "ctok_uni_trainer_substring_counts": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u64p)]),
    "ctok_uni_trainer_expected_counts": (ctypes.c_int, [_p, ctypes.POINTER(BpeStrings), ctypes.POINTER(_u64p)]),
    "ctok_uni_trainer_stats": (ctypes.c_int, [_p, ctypes.POINTER(UniTrainerStats)]),
    "ctok_uni_model_create": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_uni_model_destroy": (None, [_p]),
    "ctok_uni_model_vocab_size": (_u64, [_p]),
    "ctok_uni_model_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(_u32p), ctypes.POINTER(_u64p)]),
    # include/ctok_models.h
    "ctok_wl_model_create": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_cbpe_model_create": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, _u64, ctypes.c_char_p, ctypes.c_char_p,
                                              ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_blbpe_model_create": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, _u64, ctypes.c_char_p, ctypes.c_int,
                                               ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_wl_model_destroy": (None, [_p]),
    "ctok_cbpe_model_destroy": (None, [_p]),
    "ctok_blbpe_model_destroy": (None, [_p]),
    "ctok_wl_model_vocab_size": (_u64, [_p]),
    "ctok_cbpe_model_vocab_size": (_u64, [_p]),
    "ctok_blbpe_model_vocab_size": (_u64, [_p]),
    "ctok_wl_model_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(_u32p), ctypes.POINTER(_u64p)]),
    "ctok_cbpe_model_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(_u32p), ctypes.POINTER(_u64p)]),
    "ctok_blbpe_model_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.POINTER(_u32p), ctypes.POINTER(_u64p)]),
    "ctok_models_limits": (None, [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.POINTER(ctypes.c_uint64)]),
    "ctok_models_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double)]),
    # include/ctok_normalizer.h
    "ctok_normalizer_create": (ctypes.c_int, [ctypes.POINTER(NormStep), _u64, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_normalizer_destroy": (None, [_p]),
    "ctok_normalizer_run": (ctypes.c_int, [_p, _p, _p, _u64, _p, _u64, _p]),
    "ctok_normalizer_run_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, _p, _u64, _p, _u64p, _p]),
    "ctok_normalizer_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), _u64, _u64p]),
    "ctok_normalizer_stage_name": (ctypes.c_char_p, [_p, _u64]),
    "ctok_normalizer_stats": (ctypes.c_int, [_p, ctypes.POINTER(NormInfo)]),
    # include/ctok_pretokenizer.h
    "ctok_pretokenizer_create": (ctypes.c_int, [ctypes.POINTER(PretokStep), _u64, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_pretokenizer_destroy": (None, [_p]),
    "ctok_pretok_split_class": (ctypes.c_int, [ctypes.c_char_p, _u64]),
    "ctok_pretok_split_plan": (ctypes.c_int, [ctypes.c_char_p, _u64, ctypes.POINTER(PretokSplitInfo)]),
    "ctok_pretok_limits": (ctypes.c_int, [ctypes.POINTER(PretokLimits)]),
    "ctok_pretokenizer_run": (ctypes.c_int, [_p, _p, _p, _u64, _p, _u64, _p, _u64, _p, _u64p, _u64p]),
    "ctok_pretokenizer_run_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, _p, _u64, _p, _u64, _p, _u64p, _u64p, _p]),
    "ctok_pretokenizer_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), _u64, _u64p]),
    "ctok_pretokenizer_stage_name": (ctypes.c_char_p, [_p, _u64]),
    "ctok_pretokenizer_stats": (ctypes.c_int, [_p, ctypes.POINTER(PretokInfo)]),
    # include/ctok_decoder.h
    "ctok_decoder_create": (ctypes.c_int, [ctypes.POINTER(DecStep), _u64, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_decoder_destroy": (None, [_p]),
    "ctok_decoder_set_vocab": (ctypes.c_int, [_p, _p, _u64, _p, _p, _u64]),
    "ctok_decoder_run": (ctypes.c_int, [_p, _p, _p, _p, _u64, _p, _u64, _p, _u64p]),
    "ctok_decoder_run_ids": (ctypes.c_int, [_p, _p, _p, _u64, _p, _u64, _p, _u64p]),
    "ctok_decoder_fetch": (ctypes.c_int, [_p, _p, _u64, _p, _u64p]),
    "ctok_decoder_run_device": (ctypes.c_int, [_p, _p, _p, _p, _u64, _u64, _u64, _p, _u64, _p, _u64p, _p]),
    "ctok_decoder_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), _u64, _u64p]),
    "ctok_decoder_stage_name": (ctypes.c_char_p, [_p, _u64]),
    "ctok_decoder_stats": (ctypes.c_int, [_p, ctypes.POINTER(DecInfo)]),
    # include/ctok_postprocessor.h
    "ctok_postprocessor_create": (ctypes.c_int, [ctypes.POINTER(PpStep), _u64, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_postprocessor_destroy": (None, [_p]),
    "ctok_postprocessor_run": (ctypes.c_int, [_p, ctypes.POINTER(PpBatch), ctypes.POINTER(PpOpts), ctypes.POINTER(PpOut)]),
    "ctok_postprocessor_fetch": (ctypes.c_int, [_p, ctypes.POINTER(PpOut)]),
    "ctok_postprocessor_run_device": (ctypes.c_int, [_p, ctypes.POINTER(PpBatch), _u64, _u64, ctypes.POINTER(PpOpts), _p, _u64, _p,
                                                     _u64p, _p]),
    "ctok_postprocessor_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), _u64, _u64p]),
    "ctok_postprocessor_stage_name": (ctypes.c_char_p, [_p, _u64]),
    "ctok_postprocessor_stats": (ctypes.c_int, [_p, ctypes.POINTER(PpInfo)]),
    # include/ctok_pipeline.h
    "ctok_pipeline_create": (ctypes.c_int, [ctypes.POINTER(PipelineTables), _p, _p, ctypes.c_int, ctypes.POINTER(_p)]),
    "ctok_pipeline_destroy": (None, [_p]),
    "ctok_pipeline_encode_batch": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_uint32, ctypes.POINTER(_p), ctypes.POINTER(_p)]),
    "ctok_pipeline_encode_batch_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, ctypes.c_uint32, _p, _u64, _p, _u64p, _p]),
    "ctok_pipeline_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double)]),
    "ctok_pipeline_stage_name": (ctypes.c_char_p, [_u64]),
    "ctok_pipeline_limits": (None, [_p, ctypes.POINTER(PipelineLimits)]),
    "ctok_pipeline_stats": (ctypes.c_int, [_p, ctypes.POINTER(PipelineInfo)]),
    "ctok_pipeline_encode_encodings": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, _p, ctypes.POINTER(PipelineEncodings)]),
    "ctok_pipeline_encode_encodings_device": (ctypes.c_int, [_p, _p, _p, _u64, ctypes.c_int, _u64, _p,
                                                             ctypes.POINTER(PipelineEncodingsDevice), _p]),
    "ctok_pipeline_encoding_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double)]),
    "ctok_pipeline_encoding_stage_name": (ctypes.c_char_p, [_u64]),
    "ctok_pipeline_encoding_limits": (None, [_p, ctypes.POINTER(PipelineEncodingLimits)]),
    "ctok_pipeline_encoding_stats": (ctypes.c_int, [_p, ctypes.POINTER(PipelineEncodingInfo)]),
    "ctok_pipeline_encode_windows": (ctypes.c_int, [_p, _p, _p, _u64, _p, _p, _p, ctypes.POINTER(PipelineWindowOpts),
                                                    ctypes.POINTER(PipelineWindows)]),
    "ctok_pipeline_encode_windows_device": (ctypes.c_int, [_p, _p, _p, _u64, _u64, _p, ctypes.POINTER(PipelineWindowOpts),
                                                           ctypes.POINTER(PipelineWindowsDevice), _p]),
    "ctok_pipeline_window_stage_ms": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double)]),
    "ctok_pipeline_window_stage_name": (ctypes.c_char_p, [_u64]),
    "ctok_pipeline_window_stats": (ctypes.c_int, [_p, ctypes.POINTER(PipelineWindowInfo)]),
}

for _name, (_res, _args) in SIGS.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def last_error() -> str:
    return lib.ctok_last_error().decode("utf-8", "replace")
