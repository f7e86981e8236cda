"""ctypes binding of libsrgpu.so (include/srgpu.h) -- the product's C ABI.

Used by tests/ and bench.py to drive the HIP path exactly as a foreign-language host would; no
compute happens in Python and there is no fallback: if the library or a gfx950 device is missing
the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SRGPU_LIB: a differently tuned build of the same library (tools/build_variant.py), for A/B timing only
LIB_PATH = os.environ.get("SRGPU_LIB") or os.path.join(HERE, "libsrgpu.so")

GMM_MFMA, GMM_EXACT, GMM_PREFILTER, GMM_DEFAULT = 0, 1, 2, 3
POOL_GLOBAL, POOL_MIXTURE, POOL_NONE = 0, 1, 2
SEARCH_GENERAL_KERNEL = 1
SEARCH_SLOT_KERNEL = 2
BIGRAM_DENSE_STATES = 1
BIGRAM_GLOBAL_STATES = 2
SR_ECORRUPT = -7
LDA_SKIP = 0xFFFFFFFF  # SR_LDA_SKIP: the class of a frame the LDA statistics leave out
SR_ABI_VERSION = 4
STREAM_NO_WARP = 0xFFFFFFFF  # SR_STREAM_NO_WARP: an utterance of a stream set without a VTLN warp

# every symbol include/srgpu.h declares
SYMBOLS = [
    "sr_abi_version", "sr_model_trim",
    "sr_last_error", "sr_device_count", "sr_model_create", "sr_model_load_mixset", "sr_model_destroy", "sr_model_info",
    "sr_corpus_upload", "sr_corpus_upload_async", "sr_corpus_wait", "sr_corpus_destroy", "sr_shard_utterances", "sr_recognize_batch_multi", "sr_score_corpus", "sr_score_frames", "sr_lexicon_create",
    "sr_lexicon_destroy", "sr_lexicon_describe", "sr_recognize_corpus", "sr_traceback_corpus", "sr_traceback_words", "sr_recognize_batch", "sr_align_corpus", "sr_align_corpus_pruned", "sr_path_scores_corpus", "sr_model_create_from_statistics", "sr_model_create_from_accumulated", "sr_mixset_write", "sr_model_set_tying", "sr_model_tying_info", "sr_model_topology", "sr_accumulate_corpus",
    "sr_model_split", "sr_model_eliminate", "sr_model_tables",
    "sr_state_posteriors_corpus", "sr_baum_welch_corpus", "sr_word_posteriors_corpus", "sr_recognize_confidence_corpus",
    "sr_net_occupancies_corpus", "sr_mmi_statistics_corpus", "sr_model_create_from_mmi_statistics",
    "sr_smbr_max_positions", "sr_net_accuracies_corpus", "sr_smbr_statistics_corpus",
    "sr_word_lattice_corpus", "sr_lattice_nbest",
    "sr_fmllr_statistics_corpus", "sr_fmllr_statistics_bw_corpus", "sr_fmllr_estimate", "sr_corpus_transform",
    "sr_mllr_statistics_corpus", "sr_mllr_statistics_bw_corpus", "sr_mllr_estimate", "sr_model_transform_means",
    "sr_map_statistics_corpus", "sr_map_statistics_bw_corpus", "sr_model_map_adapt",
    "sr_mllt_statistics_corpus", "sr_mllt_statistics_bw_corpus", "sr_mllt_estimate",
    "sr_lda_statistics_corpus", "sr_lda_estimate", "sr_corpus_splice_transform",
    "sr_frontend_create", "sr_frontend_destroy", "sr_frontend_frames", "sr_corpus_from_audio", "sr_corpus_from_cepstra", "sr_mfcc_corpus",
    "sr_corpus_download",
    "sr_frontend_create_warped", "sr_frontend_warps", "sr_corpus_from_audio_warped", "sr_vtln_costs_corpus", "sr_vtln_chunks", "sr_vtln_choose",
    "sr_bigram_create", "sr_bigram_destroy", "sr_bigram_describe", "sr_recognize_bigram_corpus",
    "sr_bigram_word_posteriors_corpus", "sr_recognize_bigram_confidence_corpus",
    "sr_bigram_occupancies_corpus", "sr_bigram_mmi_statistics_corpus",
    "sr_bigram_accuracies_corpus", "sr_bigram_smbr_statistics_corpus",
    "sr_bigram_word_lattice_corpus", "sr_bigram_lattice_nbest",
    "sr_stream_open", "sr_stream_begin", "sr_stream_push", "sr_stream_partial", "sr_stream_end", "sr_stream_destroy",
    "sr_stream_stable", "sr_bigram_stream_stable", "sr_commit_points", "sr_stream_trim",
    "sr_bigram_stream_open", "sr_bigram_stream_begin", "sr_bigram_stream_push", "sr_bigram_stream_partial", "sr_bigram_stream_end",
    "sr_bigram_stream_destroy",
    "sr_stream_set_frontend", "sr_stream_push_audio", "sr_stream_finish_audio",
    "sr_bigram_stream_set_frontend", "sr_bigram_stream_push_audio", "sr_bigram_stream_finish_audio",
    "sr_stream_set_projection", "sr_stream_set_transform", "sr_stream_push_rows",
    "sr_bigram_stream_set_projection", "sr_bigram_stream_set_transform", "sr_bigram_stream_push_rows",
    "sr_stream_set_warp", "sr_bigram_stream_set_warp",
    "sr_probe_fp16_denormals", "sr_probe_fp16_accumulation", "sr_prefilter_masks", "sr_prefilter_range_frames",
    "sr_refine_masks", "sr_refine_geometry",
    "sr_gather_words", "sr_recognize_corpus_scores", "sr_recognize_bigram_corpus_scores", "sr_bigram_route",
    "sr_align_corpus_scores", "sr_state_posteriors_corpus_scores",
    "sr_word_posteriors_corpus_scores", "sr_net_occupancies_corpus_scores", "sr_net_accuracies_corpus_scores",
    "sr_bigram_word_posteriors_corpus_scores", "sr_bigram_occupancies_corpus_scores", "sr_bigram_accuracies_corpus_scores",
    "sr_profile_enable", "sr_profile_reset", "sr_profile_read",
]


class SrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsrgpu error {code}: {msg}")
        self.code = code


def prefilter_range_frames():
    """sr_prefilter_range_frames: a stationary-route prefilter launch of more frames than this has at least two frame ranges"""
    n = C.c_uint32()
    _check(lib().sr_prefilter_range_frames(C.byref(n)))
    return n.value


def smbr_max_positions():
    """the largest lexicon (positions) sr_net_accuracies_corpus / sr_smbr_statistics_corpus take"""
    n = C.c_uint32()
    _check(lib().sr_smbr_max_positions(C.byref(n)))
    return n.value


class SearchParams(C.Structure):
    _fields_ = [("am_threshold", C.c_double), ("word_penalty", C.c_double), ("gmm_kernel", C.c_int), ("flags", C.c_int)]


class BigramParams(C.Structure):
    _fields_ = [("acoustic_pruning", C.c_float), ("lm_pruning", C.c_float), ("gmm_kernel", C.c_int), ("max_word_ends", C.c_uint32), ("flags", C.c_int)]


class MfccParams(C.Structure):
    """sr_mfcc_params"""
    _fields_ = [("sample_rate", C.c_double), ("window", C.c_uint32), ("shift", C.c_uint32), ("n_fft", C.c_uint32), ("n_mel", C.c_uint32),
                ("n_cepstra", C.c_uint32), ("f_low", C.c_double), ("f_high", C.c_double), ("preemphasis", C.c_float),
                ("energy_floor", C.c_float), ("flags", C.c_uint32)]


class FeaturePostParams(C.Structure):
    """sr_feature_post_params"""
    _fields_ = [("n_static", C.c_uint32), ("n_first", C.c_uint32), ("n_second", C.c_uint32), ("deriv_step", C.c_uint32),
                ("energy_max_norm", C.c_int32), ("mean", C.c_void_p), ("stddev", C.c_void_p)]


class VtlnParams(C.Structure):
    """sr_vtln_params"""
    _fields_ = [("n_warps", C.c_uint32), ("alpha", C.c_void_p), ("break_frac", C.c_double)]


class Profile(C.Structure):
    _fields_ = [("gmm_ms", C.c_double), ("gmm_launches", C.c_uint64), ("gmm_flops", C.c_double),
                ("search_ms", C.c_double), ("search_launches", C.c_uint64), ("search_bytes", C.c_double),
                ("frames", C.c_uint64), ("refined_pairs", C.c_uint64), ("refined_densities", C.c_uint64),
                ("prefilter_ms", C.c_double), ("refine_ms", C.c_double)]


_lib = None


def lib():
    """Loads libsrgpu.so (built in-tree by speechrecognition_amd/build.py). Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        if L.sr_abi_version() != SR_ABI_VERSION:  # the struct layouts below are those of include/srgpu.h version SR_ABI_VERSION
            raise RuntimeError(f"{LIB_PATH} has ABI version {L.sr_abi_version()}, this binding was written for {SR_ABI_VERSION}")
        L.sr_last_error.restype = C.c_char_p
        vp, u32, u64, i32, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
        L.sr_device_count.argtypes = [C.POINTER(i32)]
        L.sr_model_create.argtypes = [i32, u32, u32, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.sr_model_load_mixset.argtypes = [C.c_char_p, u32, i32, i32, i32, C.POINTER(vp)]
        L.sr_model_destroy.argtypes = [vp]
        L.sr_model_trim.argtypes = [vp]
        L.sr_model_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
        L.sr_corpus_upload.argtypes = [vp, vp, vp, u32, C.POINTER(vp)]
        L.sr_corpus_destroy.argtypes = [vp]
        L.sr_corpus_upload_async.argtypes = [vp, vp, vp, u32, C.POINTER(vp)]
        L.sr_corpus_wait.argtypes = [vp]
        L.sr_shard_utterances.argtypes = [vp, u32, u32, vp, vp]
        L.sr_recognize_batch_multi.argtypes = [vp, vp, u32, C.POINTER(SearchParams), vp, vp, u32, vp, vp, vp]
        L.sr_score_corpus.argtypes = [vp, vp, i32, vp]
        L.sr_score_frames.argtypes = [vp, vp, u64, i32, vp]
        L.sr_lexicon_create.argtypes = [vp, u32, vp, vp, u32, C.POINTER(dbl * 3), C.c_uint16, C.POINTER(vp)]
        L.sr_lexicon_destroy.argtypes = [vp]
        L.sr_lexicon_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.sr_recognize_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), vp, vp, vp, vp, vp]
        L.sr_recognize_batch.argtypes = [vp, vp, C.POINTER(SearchParams), vp, vp, u32, vp, vp]
        L.sr_traceback_corpus.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.sr_traceback_words.argtypes = [u32, vp, vp, u32, u32, vp, C.POINTER(u32)]
        L.sr_align_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, vp, vp]
        L.sr_align_corpus_pruned.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, dbl, i32, vp, vp]
        L.sr_path_scores_corpus.argtypes = [vp, vp, vp, i32, vp]
        L.sr_model_create_from_statistics.argtypes = [i32, u32, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(vp)]
        L.sr_model_create_from_accumulated.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
        L.sr_model_split.argtypes = [vp, vp, vp, dbl, dbl, i32, C.POINTER(vp), vp]
        L.sr_model_eliminate.argtypes = [vp, vp, vp, dbl, C.POINTER(vp), vp]
        L.sr_model_tables.argtypes = [vp, vp, vp, vp, vp]
        L.sr_mixset_write.argtypes = [C.c_char_p, u32, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp]
        L.sr_model_set_tying.argtypes = [vp, u32, u32, vp, vp]
        L.sr_model_tying_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.sr_model_topology.argtypes = [vp, vp, vp, vp]
        L.sr_accumulate_corpus.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
        L.sr_state_posteriors_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, u32, vp, vp, vp, vp]
        L.sr_baum_welch_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, i32, i32, vp, vp, vp, vp, vp]
        L.sr_fmllr_statistics_corpus.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp]
        L.sr_fmllr_statistics_bw_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, vp, u32, i32, vp, vp, vp, vp]
        L.sr_fmllr_estimate.argtypes = [u32, u32, vp, vp, vp, u32, dbl, vp, vp, vp, vp]
        L.sr_corpus_transform.argtypes = [vp, vp, vp, u32, vp, C.POINTER(vp)]
        L.sr_mllr_statistics_corpus.argtypes = [vp, vp, vp, vp, u32, vp, u32, i32, vp, vp, vp]
        L.sr_mllr_statistics_bw_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, vp, u32, vp, u32, i32, vp, vp, vp,
                                                   vp]
        L.sr_mllr_estimate.argtypes = [u32, u32, u32, u32, vp, vp, vp, vp, dbl, vp, vp, vp]
        L.sr_model_transform_means.argtypes = [vp, vp, u32, vp, C.POINTER(vp)]
        L.sr_map_statistics_corpus.argtypes = [vp, vp, vp, vp, u32, i32, u64, vp, vp, vp, vp]
        L.sr_map_statistics_bw_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, vp, u32, i32, vp, u64, vp, vp, vp, vp]
        L.sr_model_map_adapt.argtypes = [vp, u64, vp, vp, vp, dbl, i32, dbl, C.POINTER(vp)]
        L.sr_mllt_statistics_corpus.argtypes = [vp, vp, vp, i32, vp, vp]
        L.sr_mllt_statistics_bw_corpus.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, i32, vp, vp, vp]
        L.sr_mllt_estimate.argtypes = [u32, dbl, vp, u32, dbl, vp, vp, vp, vp]
        L.sr_lda_statistics_corpus.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, vp]
        L.sr_lda_estimate.argtypes = [u32, u32, vp, vp, vp, u32, i32, dbl, vp, vp, vp]
        L.sr_corpus_splice_transform.argtypes = [vp, vp, vp, u32, vp, C.POINTER(vp)]
        L.sr_frontend_create.argtypes = [vp, C.POINTER(MfccParams), C.POINTER(FeaturePostParams), C.POINTER(vp)]
        L.sr_frontend_destroy.argtypes = [vp]
        L.sr_frontend_frames.argtypes = [vp, u64, C.POINTER(u64)]
        L.sr_corpus_from_audio.argtypes = [vp, vp, vp, u32, C.POINTER(vp), vp]
        L.sr_corpus_from_cepstra.argtypes = [vp, vp, vp, u32, C.POINTER(vp)]
        L.sr_mfcc_corpus.argtypes = [vp, vp, vp, u32, vp, vp]
        L.sr_corpus_download.argtypes = [vp, vp]
        L.sr_frontend_create_warped.argtypes = [vp, C.POINTER(MfccParams), C.POINTER(VtlnParams), C.POINTER(FeaturePostParams), C.POINTER(vp)]
        L.sr_frontend_warps.argtypes = [vp, C.POINTER(u32)]
        L.sr_corpus_from_audio_warped.argtypes = [vp, vp, vp, u32, vp, C.POINTER(vp), vp]
        L.sr_vtln_costs_corpus.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp, vp]
        L.sr_vtln_chunks.argtypes = [vp, u64, u32, C.POINTER(u32)]
        L.sr_vtln_choose.argtypes =[u32, u32, vp, vp, u64, u32, vp]
        L.sr_word_posteriors_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, vp, vp, vp]
        L.sr_recognize_confidence_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, vp, vp, vp, vp, vp]
        L.sr_net_occupancies_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, vp, vp, vp, vp, vp]
        L.sr_mmi_statistics_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, i32, vp, vp] + [vp] * 10
        L.sr_smbr_max_positions.argtypes = [vp]
        L.sr_net_accuracies_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, vp, vp, vp, vp, vp]
        L.sr_smbr_statistics_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, i32, vp] + [vp] * 10
        L.sr_model_create_from_mmi_statistics.argtypes = [vp] + [vp] * 8 + [dbl, dbl, dbl, C.POINTER(vp)]
        L.sr_word_lattice_corpus.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sr_lattice_nbest.argtypes = [u32, u64, vp, vp, vp, vp, u32, u32, vp, u64, vp, vp, C.POINTER(u32)]
        L.sr_bigram_create.argtypes = [vp, u32, vp, vp, u32, vp, vp, C.POINTER(vp)]
        L.sr_bigram_destroy.argtypes = [vp]
        L.sr_bigram_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.sr_recognize_bigram_corpus.argtypes = [vp, vp, vp, C.POINTER(BigramParams), vp, vp, vp, vp]
        L.sr_bigram_word_posteriors_corpus.argtypes = [vp, vp, vp, i32, dbl, dbl, u32, vp, vp, vp, vp]
        L.sr_bigram_occupancies_corpus.argtypes = [vp, vp, vp, i32, dbl, dbl, u32, vp, vp, vp, vp, vp, vp]
        L.sr_bigram_mmi_statistics_corpus.argtypes = [vp, vp, vp, i32, dbl, dbl, i32, vp, vp] + [vp] * 10
        L.sr_bigram_accuracies_corpus.argtypes = [vp, vp, vp, i32, dbl, dbl, u32, vp, vp, vp, vp, vp, vp]
        L.sr_bigram_smbr_statistics_corpus.argtypes = [vp, vp, vp, i32, dbl, dbl, i32, vp] + [vp] * 10
        L.sr_recognize_bigram_confidence_corpus.argtypes = [vp, vp, vp, C.POINTER(BigramParams), dbl, vp, vp, vp, vp, vp]
        L.sr_bigram_word_lattice_corpus.argtypes = [vp, vp, vp, i32, dbl, u64] + [vp] * 10
        L.sr_bigram_lattice_nbest.argtypes = [u32, u64, vp, vp, vp, vp, vp, u32, u32, vp, dbl, u32, vp, u64, vp, vp, C.POINTER(u32)]
        L.sr_stream_open.argtypes = [vp, vp, C.POINTER(SearchParams), u32, u64, C.POINTER(vp)]
        L.sr_stream_begin.argtypes = [vp, C.POINTER(u32)]
        L.sr_stream_push.argtypes = [vp, u32, vp, vp, vp]
        L.sr_stream_partial.argtypes = [vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u64)]
        L.sr_stream_end.argtypes = [vp, u32, vp, u32, C.POINTER(u32), vp, vp, vp]
        L.sr_stream_destroy.argtypes = [vp]
        L.sr_stream_stable.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp]
        L.sr_stream_trim.argtypes = [vp, u32, vp, vp]
        L.sr_bigram_stream_stable.argtypes = [vp, u32, vp, vp, vp, vp, u64, vp, vp]
        L.sr_commit_points.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.sr_bigram_stream_open.argtypes = [vp, vp, C.POINTER(BigramParams), u32, u64, C.POINTER(vp)]
        L.sr_bigram_stream_begin.argtypes = [vp, C.POINTER(u32)]
        L.sr_bigram_stream_push.argtypes = [vp, u32, vp, vp, vp]
        L.sr_bigram_stream_partial.argtypes = [vp, u32, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u64)]
        L.sr_bigram_stream_end.argtypes = [vp, u32, vp, vp, vp, u32, C.POINTER(u32)]
        L.sr_bigram_stream_destroy.argtypes = [vp]
        for fn in ("sr_stream", "sr_bigram_stream"):
            getattr(L, fn + "_set_frontend").argtypes = [vp, vp]
            getattr(L, fn + "_push_audio").argtypes = [vp, u32, vp, vp, vp, vp, u64, vp]
            getattr(L, fn + "_finish_audio").argtypes = [vp, u32, vp, vp, u64, vp]
            getattr(L, fn + "_set_projection").argtypes = [vp, u32, u32, vp]
            getattr(L, fn + "_set_transform").argtypes = [vp, u32, vp]
            getattr(L, fn + "_set_warp").argtypes = [vp, u32, u32]
            getattr(L, fn + "_push_rows").argtypes = [vp, u32, vp, vp, vp, i32, vp, u64, vp]
        L.sr_probe_fp16_denormals.argtypes = [i32, C.POINTER(i32)]
        L.sr_probe_fp16_accumulation.argtypes = [i32, C.POINTER(i32), C.POINTER(dbl)]
        L.sr_prefilter_masks.argtypes = [vp, vp, u64, i32, C.POINTER(u32), vp, u64]
        L.sr_prefilter_range_frames.argtypes = [C.POINTER(u32)]
        L.sr_refine_masks.argtypes = [vp, vp, u64, vp, u64, vp]
        L.sr_refine_geometry.argtypes = [vp, u64, vp]
        L.sr_gather_words.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.sr_recognize_bigram_corpus_scores.argtypes = [vp, vp, vp, C.POINTER(BigramParams), vp, u64, vp, vp, vp, vp]
        L.sr_bigram_route.argtypes = [vp, u32, C.c_char_p, C.c_size_t]
        L.sr_recognize_corpus_scores.argtypes = [vp, vp, vp, C.POINTER(SearchParams), vp, u64, i32, vp, vp, vp, vp, vp, vp]
        L.sr_align_corpus_scores.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, i32, dbl, vp, u64, vp, vp]
        L.sr_state_posteriors_corpus_scores.argtypes = [vp, vp, vp, vp, C.POINTER(dbl * 3), C.c_uint16, vp, u64, dbl, u32, vp, vp, vp, vp]
        L.sr_word_posteriors_corpus_scores.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, u64, vp, vp, vp, vp]
        L.sr_net_occupancies_corpus_scores.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, vp, vp, u64, vp, vp, vp, vp]
        L.sr_net_accuracies_corpus_scores.argtypes = [vp, vp, vp, C.POINTER(SearchParams), dbl, dbl, u32, vp, vp, u64, vp, vp, vp, vp, vp]
        L.sr_bigram_word_posteriors_corpus_scores.argtypes = [vp, vp, vp, dbl, dbl, u32, vp, u64, vp, vp, vp, vp]
        L.sr_bigram_occupancies_corpus_scores.argtypes = [vp, vp, vp, dbl, dbl, u32, vp, vp, vp, u64, vp, vp, vp, vp]
        L.sr_bigram_accuracies_corpus_scores.argtypes = [vp, vp, vp, dbl, dbl, u32, vp, vp, u64, vp, vp, vp, vp, vp]
        L.sr_profile_enable.argtypes = [vp, i32]
        L.sr_profile_reset.argtypes = [vp]
        L.sr_profile_read.argtypes = [vp, C.POINTER(Profile)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise SrError(rc, lib().sr_last_error().decode(errors="replace"))


def device_count():
    n = C.c_int(0)
    _check(lib().sr_device_count(C.byref(n)))
    return n.value


def _ptr(a):
    return a.ctypes.data if a is not None else None


class Model:
    """sr_model handle: the GPU FeatureScorer (MixtureModel, sietill/Mixtures.hpp:18)."""

    def __init__(self, handle):
        self.h = handle
        d, s, c = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(lib().sr_model_info(self.h, C.byref(d), C.byref(s), C.byref(c)))
        self.dim, self.n_states, self.n_densities = d.value, s.value, c.value

    @classmethod
    def from_mixset(cls, path, dim, pooling=POOL_NONE, max_approx=True, device=0):
        h = C.c_void_p()
        _check(lib().sr_model_load_mixset(str(path).encode(), dim, pooling, int(max_approx), device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_tables(cls, dens_off, means, inv_vars, norm, logw, max_approx=True, device=0):
        dens_off = np.ascontiguousarray(dens_off, dtype=np.uint32)
        means = np.ascontiguousarray(means, dtype=np.float64)
        inv_vars = np.ascontiguousarray(inv_vars, dtype=np.float64)
        norm = np.ascontiguousarray(norm, dtype=np.float64)
        logw = np.ascontiguousarray(logw, dtype=np.float64)
        h = C.c_void_p()
        _check(lib().sr_model_create(device, means.shape[1], len(dens_off) - 1, _ptr(dens_off), _ptr(means), _ptr(inv_vars),
                                     _ptr(norm), _ptr(logw), int(max_approx), C.byref(h)))
        return cls(h)

    @classmethod
    def from_statistics(cls, dim, dens_off, dens_mean, dens_var, acc, pooling=POOL_NONE, max_approx=True, device=0):
        """MixtureModel::finalize on EM statistics `acc` = (mean_acc, mean_w, var_acc, var_w) -> new device model."""
        dens_off, dens_mean, dens_var = (np.ascontiguousarray(x, dtype=np.uint32) for x in (dens_off, dens_mean, dens_var))
        ma, mw, va, vw = (np.ascontiguousarray(x, dtype=np.float64) for x in acc)
        h = C.c_void_p()
        _check(lib().sr_model_create_from_statistics(device, dim, len(dens_off) - 1, _ptr(dens_off), len(mw), len(vw), _ptr(dens_mean),
                                                     _ptr(dens_var), _ptr(ma), _ptr(mw), _ptr(va), _ptr(vw), pooling, int(max_approx),
                                                     C.byref(h)))
        return cls(h)

    def from_mmi_statistics(self, num, den, E, tau=0.0, var_floor=1e-6):
        """Extended Baum-Welch update of this model's means and variances from the statistics of Corpus.mmi_statistics
        (sr_model_create_from_mmi_statistics) -> new device model; the mixture weights stay."""
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in tuple(num) + tuple(den)]
        h = C.c_void_p()
        _check(lib().sr_model_create_from_mmi_statistics(self.h, *[_ptr(a) for a in arrs], float(E), float(tau), float(var_floor),
                                                         C.byref(h)))
        return Model(h)

    def topology(self):
        """-> (dens_off u32[S+1], dens_mean u32[C], dens_var u32[C]): what mixset_write / from_statistics take."""
        off = np.zeros(self.n_states + 1, np.uint32)
        dm, dv = np.zeros(self.n_densities, np.uint32), np.zeros(self.n_densities, np.uint32)
        _check(lib().sr_model_topology(self.h, _ptr(off), _ptr(dm), _ptr(dv)))
        return off, dm, dv

    def tying_info(self):
        """-> (n_mean, n_var): the accumulator rows of this model's tying"""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.h, C.byref(nm), C.byref(nv)))
        return nm.value, nv.value

    def tables(self):
        """-> (means f64[C, D], inv_vars f64[C, D], norm f64[C], logw f64[C]): the per-density tables, in from_tables' shape
        (sr_model_tables)."""
        n, D = self.n_densities, self.dim
        means, ivars, norm, logw = np.zeros((n, D)), np.zeros((n, D)), np.zeros(n), np.zeros(n)
        _check(lib().sr_model_tables(self.h, _ptr(means), _ptr(ivars), _ptr(norm), _ptr(logw)))
        return means, ivars, norm, logw

    def _weights(self, weights):
        """the per mean row weights of split() / eliminate(): a Corpus holding statistics of this model, or a host array"""
        if isinstance(weights, Corpus):
            return weights.h, None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if len(w) != self.tying_info()[0]:
            raise ValueError("one weight per mean row")
        return None, w

    def split(self, weights, min_obs, epsilon, pooling=POOL_NONE, parents=False):
        """sr_model_split: every density whose mean row has weight >= min_obs becomes two, epsilon standard deviations apart on
        either side -> new Model [, parent u32[C']].  weights: mean_w as Corpus.accumulate returns it, or the Corpus that
        accumulate_on_device() left the statistics in."""
        c, w = self._weights(weights)
        h = C.c_void_p()
        cap = self.n_densities * 2
        par = np.zeros(max(cap, 1), np.uint32)
        _check(lib().sr_model_split(self.h, c, _ptr(w), float(min_obs), float(epsilon), pooling, C.byref(h), _ptr(par)))
        out = Model(h)
        return (out, par[: out.n_densities].copy()) if parents else out

    def eliminate(self, weights, min_obs, parents=False):
        """sr_model_eliminate: the densities whose mean row has weight < min_obs go (a mixture keeps its heaviest), the rest are
        renormalised and their rows renumbered -> new Model [, parent u32[C']]."""
        c, w = self._weights(weights)
        h = C.c_void_p()
        par = np.zeros(max(self.n_densities, 1), np.uint32)
        _check(lib().sr_model_eliminate(self.h, c, _ptr(w), float(min_obs), C.byref(h), _ptr(par)))
        out = Model(h)
        return (out, par[: out.n_densities].copy()) if parents else out

    def transform_means(self, dens_class, W):
        """MLLR: a new Model whose means are W[dens_class[d]] (mu_d, 1), W f64[R, D, D+1] the transforms of one speaker
        (sr_model_transform_means); topology, tying and every other table are this model's."""
        cls = np.ascontiguousarray(dens_class, dtype=np.uint32)
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert len(cls) == self.n_densities and W.ndim == 3 and W.shape[1:] == (self.dim, self.dim + 1)
        h = C.c_void_p()
        _check(lib().sr_model_transform_means(self.h, _ptr(cls), W.shape[0], _ptr(W), C.byref(h)))
        return Model(h)

    def map_adapt(self, dens, occ, x, tau, tau_w=None):
        """MAP: a new Model whose means are (tau mu + X) / (tau + O) per mean row, from one speaker's entries (dens u32[n] strictly
        ascending, occ f64[n], x f64[n, D]: a slice of Corpus.map_statistics); tau_w not None: the mixture weights are updated too,
        n_d = tau_w w_d + occ_d (sr_model_map_adapt).  This model is the prior; topology, tying and variances are its own."""
        dens = np.ascontiguousarray(dens, dtype=np.uint32)
        occ = np.ascontiguousarray(occ, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(len(dens), self.dim)
        assert len(occ) == len(dens)
        h = C.c_void_p()
        _check(lib().sr_model_map_adapt(self.h, len(dens), _ptr(dens), _ptr(occ), _ptr(x), float(tau), int(tau_w is not None),
                                        float(tau_w if tau_w is not None else 0.0), C.byref(h)))
        return Model(h)

    def close(self):
        if self.h:
            lib().sr_model_destroy(self.h)
            self.h = None

    def trim(self):
        """sr_model_trim: releases the device buffers the model keeps between calls."""
        _check(lib().sr_model_trim(self.h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- scoring -----------------------------------------------------------------------------------
    def score_frames(self, feats, kernel=GMM_PREFILTER):
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        out = np.empty((feats.shape[0], self.n_states), dtype=np.float64)
        _check(lib().sr_score_frames(self.h, _ptr(feats), feats.shape[0], kernel, _ptr(out)))
        return out

    def prefilter_masks(self, feats, route):
        """sr_prefilter_masks (test hook): the prefilter's candidate masks [group][frame][4 state slots], route 0 staged / 1 stationary."""
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        n_groups = C.c_uint32()
        _check(lib().sr_prefilter_masks(self.h, None, feats.shape[0], route, C.byref(n_groups), None, 0))
        out = np.empty((n_groups.value, feats.shape[0], 4), dtype=np.uint32)
        _check(lib().sr_prefilter_masks(self.h, _ptr(feats), feats.shape[0], route, C.byref(n_groups), _ptr(out), out.size))
        return out

    def refine_masks(self, feats, masks):
        """sr_refine_masks (test hook): the refinement alone on the caller's candidate masks [group][frame][4 state slots] (the layout
        prefilter_masks returns) -> the score table [frames, states]."""
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        out = np.empty((feats.shape[0], self.n_states), dtype=np.float64)
        _check(lib().sr_refine_masks(self.h, _ptr(feats), feats.shape[0], _ptr(masks), masks.size, _ptr(out)))
        return out

    def refine_geometry(self, n_frames):
        """sr_refine_geometry -> (threads per workgroup, pseudo-states per workgroup, frames per workgroup, chunks per state) of a
        refinement launch over n_frames"""
        g = np.zeros(4, dtype=np.uint32)
        _check(lib().sr_refine_geometry(self.h, int(n_frames), _ptr(g)))
        return tuple(int(v) for v in g)

    def gather_words(self, frame_off, counts, flags, words):
        """sr_gather_words (test hook): (words, word_off) that a recognition call would return for these search outputs."""
        frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n_utts = len(frame_off) - 1
        assert len(counts) == n_utts and len(flags) == n_utts and len(words) == int(frame_off[-1])
        out = np.empty(max(1, len(words)), dtype=np.uint32)
        off = np.empty(n_utts + 1, dtype=np.uint64)
        _check(lib().sr_gather_words(self.h, n_utts, _ptr(frame_off), _ptr(counts), _ptr(flags), _ptr(words), _ptr(out), _ptr(off)))
        return out[:int(off[-1])].copy(), off

    def upload(self, feats, frame_off, asynchronous=False):
        return Corpus(self, feats, frame_off, asynchronous)

    def frontend(self, mfcc, post, vtln=None):
        """sr_frontend_create: the audio front end of this model.  mfcc: a dict of sr_mfcc_params' fields (sample_rate, window, shift,
        n_fft, n_mel, n_cepstra, f_low, f_high, preemphasis, energy_floor) or None for cepstra in only; post: a dict of n_static,
        n_first, n_second, deriv_step, energy_max_norm and optionally mean, stddev (f64[n_static + n_first + n_second]).
        vtln=dict(alpha=[...], break_frac=...): sr_frontend_create_warped, a filterbank per warp factor beside the unwarped one.
        Close it before the model."""
        return FrontEnd(self, mfcc, post, vtln)

    def recognize_batch(self, lexicon, feats, frame_off, am_threshold, word_penalty, kernel=GMM_PREFILTER):
        """sr_recognize_batch: host buffers in, words out (fed asynchronously while the first chunks are scored)."""
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
        n = len(frame_off) - 1
        words = np.zeros(max(int(frame_off[-1]), 1), dtype=np.uint32)
        woff = np.zeros(n + 1, dtype=np.uint64)
        sp = SearchParams(am_threshold, word_penalty, kernel, 0)
        _check(lib().sr_recognize_batch(self.h, lexicon.h, C.byref(sp), _ptr(feats), _ptr(frame_off), n, _ptr(words), _ptr(woff)))
        return words[: int(woff[-1])].copy(), woff

    def lexicon(self, word_off, automaton, silence_idx, tdp, silence_state):
        return Lexicon(self, word_off, automaton, silence_idx, tdp, silence_state)

    def bigram(self, word_off, mixtures, silence_word, lm, tdp):
        return Bigram(self, word_off, mixtures, silence_word, lm, tdp)

    def stream(self, lexicon, am_threshold, word_penalty, kernel=GMM_PREFILTER, max_streams=1, max_frames=65535):
        """sr_stream_open: a set of up to max_streams concurrently open utterances of up to max_frames frames each."""
        return Stream(self, lexicon, am_threshold, word_penalty, kernel, max_streams, max_frames)

    def bigram_stream(self, bigram, acoustic_pruning=None, lm_pruning=None, kernel=GMM_PREFILTER, max_streams=1, max_frames=65535):
        """sr_bigram_stream_open: up to max_streams concurrently open utterances of up to max_frames frames each on a bigram search
        net (beams default to off, as Corpus.recognize_bigram)."""
        return BigramStream(self, bigram, FLT_MAX if acoustic_pruning is None else acoustic_pruning,
                            FLT_MAX if lm_pruning is None else lm_pruning, kernel, max_streams, max_frames)

    # -- profiling ---------------------------------------------------------------------------------
    def profile(self, on=True):
        _check(lib().sr_profile_enable(self.h, int(on)))
        _check(lib().sr_profile_reset(self.h))

    def profile_read(self):
        p = Profile()
        _check(lib().sr_profile_read(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}


FLT_MAX = float(np.finfo(np.float32).max)


class Bigram:
    """sr_bigram handle: linear lexicon + dense bigram table + transition scores (Teaching::LinearSearch)."""

    def __init__(self, model, word_off, mixtures, silence_word, lm, tdp):
        self.model = model
        word_off = np.ascontiguousarray(word_off, dtype=np.uint32)
        mixtures = np.ascontiguousarray(mixtures, dtype=np.uint16)
        W = len(word_off) - 1
        lm = np.ascontiguousarray(lm, dtype=np.float32)
        assert lm.shape == (W, W)
        tdp = np.ascontiguousarray(tdp, dtype=np.float32)
        assert tdp.size == 8
        self.h = C.c_void_p()
        _check(lib().sr_bigram_create(model.h, W, _ptr(word_off), _ptr(mixtures), silence_word, _ptr(lm), _ptr(tdp), C.byref(self.h)))

    def describe(self):
        """Where the search keeps the state hypotheses with no flags: "registers", "lds" or "global" (sr_bigram_describe)."""
        buf = C.create_string_buffer(32)
        _check(lib().sr_bigram_describe(self.h, buf, len(buf)))
        return buf.value.decode()

    def route(self, dense_states=False, global_states=False):
        """The kernel a recognition with these flags runs, as text (sr_bigram_route): "registers 3 rows4 0b100", "lds 2 x 12",
        "global 8 entries lds", "global 8 entries global", "none"."""
        buf = C.create_string_buffer(64)
        flags = (BIGRAM_DENSE_STATES if dense_states else 0) | (BIGRAM_GLOBAL_STATES if global_states else 0)
        _check(lib().sr_bigram_route(self.h, flags, buf, len(buf)))
        return buf.value.decode()

    def close(self):
        if self.h:
            lib().sr_bigram_destroy(self.h)
            self.h = None


class _StreamSet:
    """What Stream and BigramStream share: the handle of a stream set over a search net (`_fn`_open), begin, push and close.  The
    subclass names its C functions by the prefix `_fn`; partial and end are its own."""

    _fn = None

    def __init__(self, model, net, params, max_streams, max_frames):
        self.model = model
        self.max_frames = int(max_frames)
        self.frames = {}  # frames pushed (searched, for an id fed as audio) per open id
        self.samples = {}  # samples pushed per open id fed as audio
        self.received = {}  # input rows pushed per open id fed with push_rows
        self.frontend = None
        self.in_dim, self.context = None, 0  # the projection's (set_projection)
        self.h = C.c_void_p()
        _check(getattr(lib(), self._fn + "_open")(model.h, net.h, C.byref(params), max_streams, max_frames, C.byref(self.h)))

    def begin(self):
        """-> the id of a fresh utterance"""
        i = C.c_uint32()
        _check(getattr(lib(), self._fn + "_begin")(self.h, C.byref(i)))
        self.frames[i.value] = 0
        self.samples.pop(i.value, None)
        self.received[i.value] = 0
        return i.value

    def push(self, frames):
        """frames: {id: float32 [k x dim]} (in_dim columns with a projection) -> one scoring and one search launch for all of them"""
        ids = np.ascontiguousarray(list(frames.keys()), dtype=np.uint32)
        cols = self.model.dim if self.in_dim is None else self.in_dim
        parts = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, cols) for f in frames.values()]
        off = np.concatenate([[0], np.cumsum([len(f) for f in parts])]).astype(np.uint64)
        feats = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, cols), np.float32))
        _check(getattr(lib(), self._fn + "_push")(self.h, len(ids), _ptr(ids), _ptr(feats) if len(feats) else None, _ptr(off)))
        for i, f in zip(ids, parts):  # (with a projection the search runs `context` rows behind the rows received)
            self.received[int(i)] = self.received.get(int(i), 0) + len(f)
            self.frames[int(i)] = self._rows_out(self.received[int(i)], False)

    def set_projection(self, in_dim, context, M):
        """sr_stream_set_projection: rows of in_dim columns are spliced with `context` neighbours on either side and projected by
        M [dim x ((2 context + 1) in_dim + 1)] (float64; None detaches) on the device before they are scored; only while no id is open."""
        if M is None:
            _check(getattr(lib(), self._fn + "_set_projection")(self.h, 0, 0, None))
            self.in_dim, self.context = None, 0
            return
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.shape != (self.model.dim, (2 * int(context) + 1) * int(in_dim) + 1):
            raise ValueError(f"M must be [{self.model.dim} x {(2 * int(context) + 1) * int(in_dim) + 1}], got {M.shape}")
        _check(getattr(lib(), self._fn + "_set_projection")(self.h, int(in_dim), int(context), _ptr(M)))
        self.in_dim, self.context = int(in_dim), int(context)

    def set_transform(self, id, W):
        """sr_stream_set_transform: the utterance's affine transform W [dim x (dim + 1)] = [A b] (float64; None clears it), applied on
        the device after the projection; between begin and the id's first push."""
        if W is not None:
            W = np.ascontiguousarray(W, dtype=np.float64)
            if W.shape != (self.model.dim, self.model.dim + 1):
                raise ValueError(f"W must be [{self.model.dim} x {self.model.dim + 1}], got {W.shape}")
        _check(getattr(lib(), self._fn + "_set_transform")(self.h, int(id), None if W is None else _ptr(W)))

    def set_warp(self, id, warp):
        """sr_stream_set_warp: the utterance's VTLN warp, an index into the attached warped front end's warps (None or STREAM_NO_WARP
        clears it: the unwarped filters); between begin and the id's first push.  An id with a warp takes audio only."""
        _check(getattr(lib(), self._fn + "_set_warp")(self.h, int(id), STREAM_NO_WARP if warp is None else int(warp)))

    def _rows_out(self, received, finished):
        """the rows searched of an utterance that has received so many input rows (sr_stream_set_projection's delay)"""
        return received if finished else max(received - self.context, 0)

    def _push_rows(self, frames, finish, feats):
        cols = self.model.dim if self.in_dim is None else self.in_dim
        ids = np.ascontiguousarray(list(frames.keys()), dtype=np.uint32)
        parts = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, cols) for f in frames.values()]
        n = len(ids)
        off = np.concatenate([[0], np.cumsum([len(f) for f in parts])]).astype(np.uint64)
        x = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, cols), np.float32))
        ooff, out, cap = np.zeros(n + 1, np.uint64), None, 0
        if feats:
            cap = sum(self._rows_out(self.received[int(i)] + len(f), finish) - self.frames[int(i)] for i, f in zip(ids, parts))
            out = np.zeros((max(cap, 1), self.model.dim), np.float32)
        _check(getattr(lib(), self._fn + "_push_rows")(self.h, n, _ptr(ids), _ptr(x) if len(x) else None, _ptr(off), int(finish),
                                                        None if out is None else _ptr(out), cap, _ptr(ooff)))
        for j, (i, f) in enumerate(zip(ids, parts)):
            self.received[int(i)] += len(f)
            self.frames[int(i)] += int(ooff[j + 1] - ooff[j])
        if feats:
            return {int(i): out[int(ooff[j]):int(ooff[j + 1])].copy() for j, i in enumerate(ids)}
        return {}

    def push_rows(self, frames, finish=False, feats=False):
        """sr_stream_push_rows.  frames: {id: float32 [k x in_dim]} (dim columns without a projection); finish: True -- every named id is
        finished after its rows -- or a list of ids to finish (with or without rows in `frames`; they go in a call of their own).
        feats=True -> {id: float32 [rows x dim]}, the rows this call searched, in the model's space."""
        if finish is True or finish is False:
            got = self._push_rows(frames, bool(finish), feats)
        else:
            last = [int(i) for i in finish]
            cols = self.model.dim if self.in_dim is None else self.in_dim
            got = self._push_rows({i: f for i, f in frames.items() if int(i) not in last}, False, feats)
            got.update(self._push_rows({i: frames.get(i, np.zeros((0, cols), np.float32)) for i in last}, True, feats))
        return got if feats else None

    def set_frontend(self, fe):
        """sr_stream_set_frontend: the front end push_audio runs (None detaches); only while no id is open.  Close it after the set."""
        _check(getattr(lib(), self._fn + "_set_frontend")(self.h, None if fe is None else fe.h))
        self.frontend = fe

    def _audio_rows(self, ids, new_samples, call, feats):
        """one audio call; new_samples: per id, or None for the finish -> {id: float32 [k x dim]} with feats, else None.  The rows a
        call readies follow from the sample counts: max(S' - step, 0) - max(S - step, 0) per id, S = frames(N); all the rest at the finish."""
        n = len(ids)
        off, out, cap = np.zeros(n + 1, np.uint64), None, 0
        if feats and self.frontend is not None:
            fe, step = self.frontend, self.frontend.post.deriv_step
            for j, i in enumerate(ids):
                before = self.samples.get(int(i), 0)
                s0 = fe.frames(before)  # (the front end's rows are the input rows of the projection, if there is one)
                rows_in = s0 if new_samples is None else max(fe.frames(before + new_samples[j]) - step, 0)
                cap += self._rows_out(rows_in, new_samples is None) - self.frames.get(int(i), 0)
        if feats:
            out = np.zeros((max(cap, 1), self.model.dim), np.float32)
        _check(call(_ptr(out), cap, _ptr(off)))
        for j, i in enumerate(ids):
            self.frames[int(i)] += int(off[j + 1] - off[j])
            if new_samples is not None:
                self.samples[int(i)] = self.samples.get(int(i), 0) + new_samples[j]
        if feats:
            return {int(i): out[int(off[j]):int(off[j + 1])].copy() for j, i in enumerate(ids)}
        return None

    def push_audio(self, samples, feats=False):
        """sr_stream_push_audio.  samples: {id: int16[]}, the new samples of every named utterance; the rows that became ready are
        searched.  feats=True -> {id: float32 [k x dim]}, those rows."""
        ids = np.ascontiguousarray(list(samples.keys()), dtype=np.uint32)
        parts = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in samples.values()]
        soff = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
        pcm = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.int16))
        fn = getattr(lib(), self._fn + "_push_audio")
        return self._audio_rows(ids, [len(x) for x in parts],
                                lambda o, cap, off: fn(self.h, len(ids), _ptr(ids), _ptr(pcm) if len(pcm) else None, _ptr(soff), o, cap, off), feats)

    def finish_audio(self, ids, feats=False):
        """sr_stream_finish_audio: the last rows of the utterances, searched; the ids take no more audio.  feats=True -> {id: rows}."""
        ids = np.ascontiguousarray(list(ids), dtype=np.uint32)
        fn = getattr(lib(), self._fn + "_finish_audio")
        return self._audio_rows(ids, None, lambda o, cap, off: fn(self.h, len(ids), _ptr(ids), o, cap, off), feats)

    def close(self):
        if self.h:
            getattr(lib(), self._fn + "_destroy")(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Stream(_StreamSet):
    """sr_stream handle: utterances fed frame by frame (sr_stream_*).  end() returns what Corpus.recognize returns for the whole
    utterance; partial() after t frames what it returns for the first t frames."""

    _fn = "sr_stream"

    def __init__(self, model, lexicon, am_threshold, word_penalty, kernel, max_streams, max_frames):
        super().__init__(model, lexicon, SearchParams(am_threshold, word_penalty, kernel, 0), max_streams, max_frames)

    def _word_cap(self, id):
        """a word takes a frame at least; a trimmed utterance (trim) can hold more frames than max_frames"""
        return max(self.max_frames, self.frames.get(id, 0))

    def partial(self, id, frames=False):
        """-> the words so far (u32[]) [, frames pushed]"""
        out = np.zeros(self._word_cap(id), np.uint32)
        n, t = C.c_uint32(), C.c_uint64()
        _check(lib().sr_stream_partial(self.h, id, _ptr(out), len(out), C.byref(n), C.byref(t)))
        return (out[: n.value].copy(), t.value) if frames else out[: n.value].copy()

    def stable(self, ids):
        """sr_stream_stable -> (words per id: list of u32[], commit u32[n], silence u32[n]): the leading words of partial() that no
        later frame can change, the commit frame they end at, and the frames the best hypothesis has spent in trailing silence"""
        ids = np.ascontiguousarray(list(ids), dtype=np.uint32)
        n = len(ids)
        cap = int(sum(self.frames.get(int(i), 0) for i in ids))  # a word takes a frame at least
        out, off = np.zeros(max(cap, 1), np.uint32), np.zeros(n + 1, np.uint64)
        commit, silence = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        _check(lib().sr_stream_stable(self.h, n, _ptr(ids), _ptr(out), cap, _ptr(off), _ptr(commit), _ptr(silence)))
        return [out[int(off[i]): int(off[i + 1])].copy() for i in range(n)], commit[:n], silence[:n]

    def trim(self, ids):
        """sr_stream_trim -> dropped u32[n]: the frames of every named utterance up to its commit point are dropped on the device and
        their words kept on the host; max_frames bounds what is left, the results stay the whole utterance's.  end(traceback=True) is
        refused on an id that has lost frames."""
        ids = np.ascontiguousarray(list(ids), dtype=np.uint32)
        dropped = np.zeros(max(len(ids), 1), np.uint32)
        _check(lib().sr_stream_trim(self.h, len(ids), _ptr(ids), _ptr(dropped)))
        return dropped[: len(ids)]

    def end(self, id, traceback=False):
        """-> final words (u32[]) [, (tb_score, tb_word, tb_bkp) of T + 1 entries]; frees the id"""
        out = np.zeros(self._word_cap(id), np.uint32)
        n = C.c_uint32()
        tbs = tbw = tbb = None
        if traceback:
            m = self.max_frames + 1
            tbs, tbw, tbb = np.zeros(m, np.float64), np.zeros(m, np.uint16), np.zeros(m, np.uint16)
        _check(lib().sr_stream_end(self.h, id, _ptr(out), len(out), C.byref(n), _ptr(tbs), _ptr(tbw), _ptr(tbb)))
        T = self.frames.pop(id)
        words = out[: n.value].copy()
        if not traceback:
            return words
        return words, (tbs[: T + 1], tbw[: T + 1], tbb[: T + 1])


class BigramStream(_StreamSet):
    """sr_bigram_stream handle: utterances fed frame by frame to the bigram-LM search (sr_bigram_stream_*).  end() returns what
    Corpus.recognize_bigram returns for the whole utterance; partial() after t frames what it returns for the first t frames.
    Items are (words u32[], scores f32[], times u32[])."""

    _fn = "sr_bigram_stream"

    def __init__(self, model, bigram, acoustic_pruning, lm_pruning, kernel, max_streams, max_frames, max_word_ends=0, flags=0):
        p = BigramParams(acoustic_pruning, lm_pruning, kernel, max_word_ends, flags)
        super().__init__(model, bigram, p, max_streams, max_frames)

    def _out(self):
        cap = self.max_frames + 1
        return np.zeros(cap, np.uint32), np.zeros(cap, np.float32), np.zeros(cap, np.uint32)

    def partial(self, id, frames=False):
        """-> the items so far (words, scores, times) [, frames pushed]"""
        ow, osc, ot = self._out()
        n, t = C.c_uint32(), C.c_uint64()
        _check(lib().sr_bigram_stream_partial(self.h, id, _ptr(ow), _ptr(osc), _ptr(ot), len(ow), C.byref(n), C.byref(t)))
        items = (ow[: n.value].copy(), osc[: n.value].copy(), ot[: n.value].copy())
        return (items, t.value) if frames else items

    def stable(self, ids):
        """sr_bigram_stream_stable -> (items per id: list of (words, scores, times), commit u32[n]): the leading items of partial()
        that no later frame can change, and the book time of the entry they end at"""
        ids = np.ascontiguousarray(list(ids), dtype=np.uint32)
        n = len(ids)
        cap = int(sum(self.frames.get(int(i), 0) for i in ids))  # an item takes a frame at least
        ow, osc, ot = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.uint32)
        off, commit = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint32)
        _check(lib().sr_bigram_stream_stable(self.h, n, _ptr(ids), _ptr(ow), _ptr(osc), _ptr(ot), cap, _ptr(off), _ptr(commit)))
        cut = [slice(int(off[i]), int(off[i + 1])) for i in range(n)]
        return [(ow[c].copy(), osc[c].copy(), ot[c].copy()) for c in cut], commit[:n]

    def end(self, id):
        """-> the final items (words, scores, times); frees the id"""
        ow, osc, ot = self._out()
        n = C.c_uint32()
        _check(lib().sr_bigram_stream_end(self.h, id, _ptr(ow), _ptr(osc), _ptr(ot), len(ow), C.byref(n)))
        self.frames.pop(id)
        return ow[: n.value].copy(), osc[: n.value].copy(), ot[: n.value].copy()


class Corpus:
    """sr_corpus handle: device-resident utterance batch (Corpus layout, sietill/Corpus.cpp:89-111)."""

    def __init__(self, model, feats, frame_off, asynchronous=False):
        self.model = model
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        self.frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
        self.n_utts = len(self.frame_off) - 1
        self.n_frames = int(self.frame_off[-1])
        self.h = C.c_void_p()
        if asynchronous:  # the feeder borrows `feats` until wait() / close()
            self._borrowed = feats
            _check(lib().sr_corpus_upload_async(model.h, _ptr(feats), _ptr(self.frame_off), self.n_utts, C.byref(self.h)))
        else:
            _check(lib().sr_corpus_upload(model.h, _ptr(feats), _ptr(self.frame_off), self.n_utts, C.byref(self.h)))

    def wait(self):
        _check(lib().sr_corpus_wait(self.h))
        self._borrowed = None

    def close(self):
        if self.h:
            lib().sr_corpus_destroy(self.h)
            self.h = None

    def download(self):
        """sr_corpus_download: the resident features -> f32[n_frames, dim] (an asynchronous upload is waited for first)"""
        out = np.empty((self.n_frames, self.model.dim), dtype=np.float32)
        _check(lib().sr_corpus_download(self.h, _ptr(out)))
        return out

    def score(self, kernel=GMM_PREFILTER):
        out = np.empty((self.n_frames, self.model.n_states), dtype=np.float64)
        _check(lib().sr_score_corpus(self.model.h, self.h, kernel, _ptr(out)))
        return out

    def recognize(self, lexicon, am_threshold, word_penalty, kernel=GMM_PREFILTER, traceback=False, general_kernel=False, slot_kernel=False):
        """-> (words u32[], word_off u64[n_utts+1]) [, (tb_score, tb_word, tb_bkp)]"""
        words = np.zeros(max(self.n_frames, 1), dtype=np.uint32)
        woff = np.zeros(self.n_utts + 1, dtype=np.uint64)
        sp = SearchParams(am_threshold, word_penalty, kernel, (SEARCH_GENERAL_KERNEL if general_kernel else 0) | (SEARCH_SLOT_KERNEL if slot_kernel else 0))
        tbs = tbw = tbb = None
        if traceback:
            n = self.n_frames + self.n_utts
            tbs, tbw, tbb = np.zeros(n, np.float64), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
        _check(lib().sr_recognize_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), _ptr(words), _ptr(woff), _ptr(tbs),
                                         _ptr(tbw), _ptr(tbb)))
        words = words[: int(woff[-1])].copy()
        if traceback:
            return words, woff, (tbs, tbw, tbb)
        return words, woff

    def recognize_scores(self, lexicon, scores, am_threshold, word_penalty, exact_negative, general_kernel=False, slot_kernel=False):
        """sr_recognize_corpus_scores (test hook): the search alone on the caller's score table [n_frames, n_states] (the corpus's
        features are not read) -> words u32[], word_off u64[n_utts+1], (tb_score, tb_word, tb_bkp), flags u32[n_utts]"""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        words = np.zeros(max(self.n_frames, 1), dtype=np.uint32)
        woff = np.zeros(self.n_utts + 1, dtype=np.uint64)
        sp = SearchParams(am_threshold, word_penalty, GMM_DEFAULT, (SEARCH_GENERAL_KERNEL if general_kernel else 0) | (SEARCH_SLOT_KERNEL if slot_kernel else 0))
        n = self.n_frames + self.n_utts
        tbs, tbw, tbb = np.zeros(n, np.float64), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
        flags = np.zeros(max(self.n_utts, 1), dtype=np.uint32)
        _check(lib().sr_recognize_corpus_scores(self.model.h, self.h, lexicon.h, C.byref(sp), _ptr(scores), scores.size, int(exact_negative),
                                                _ptr(words), _ptr(woff), _ptr(tbs), _ptr(tbw), _ptr(tbb), _ptr(flags)))
        return words[: int(woff[-1])].copy(), woff, (tbs, tbw, tbb), flags[: self.n_utts]

    def retrace(self, lexicon, tb_word, tb_bkp):
        """sr_traceback_corpus: the device's traceback walk alone on dumps in recognize(traceback=True)'s layout."""
        tb_word = np.ascontiguousarray(tb_word, dtype=np.uint16)
        tb_bkp = np.ascontiguousarray(tb_bkp, dtype=np.uint16)
        assert len(tb_word) == len(tb_bkp) == self.n_frames + self.n_utts
        words = np.zeros(max(self.n_frames, 1), dtype=np.uint32)
        woff = np.zeros(self.n_utts + 1, dtype=np.uint64)
        _check(lib().sr_traceback_corpus(self.model.h, self.h, lexicon.h, _ptr(tb_word), _ptr(tb_bkp), _ptr(words), _ptr(woff)))
        return words[: int(woff[-1])].copy(), woff

    def _aut(self, automata):
        flat = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.uint16) for a in automata]), dtype=np.uint16)
        off = np.concatenate([[0], np.cumsum([len(a) for a in automata])]).astype(np.uint64)
        return flat, off

    def align(self, automata, tdp, silence_state, kernel=GMM_PREFILTER, pruning_threshold=None):
        """automata: one state-id sequence per utterance -> (states u16[total_frames], cost f64[n_utts])"""
        flat, off = self._aut(automata)
        states = np.zeros(max(self.n_frames, 1), dtype=np.uint16)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        if pruning_threshold is None:
            _check(lib().sr_align_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel,
                                         _ptr(states), _ptr(cost)))
        else:
            _check(lib().sr_align_corpus_pruned(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state,
                                                float(pruning_threshold), kernel, _ptr(states), _ptr(cost)))
        return states[: self.n_frames], cost[: self.n_utts]

    def align_scores(self, automata, tdp, silence_state, scores, pruning_threshold=None):
        """sr_align_corpus_scores (test hook): align() on the caller's score table [n_frames, n_states] (the corpus's features are not
        read); pruning_threshold None: the full aligner -> (states u16[total_frames], cost f64[n_utts])"""
        flat, off = self._aut(automata)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        states = np.zeros(max(self.n_frames, 1), dtype=np.uint16)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        pruned = pruning_threshold is not None
        _check(lib().sr_align_corpus_scores(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, int(pruned),
                                            float(pruning_threshold) if pruned else 0.0, _ptr(scores), scores.size, _ptr(states),
                                            _ptr(cost)))
        return states[: self.n_frames], cost[: self.n_utts]

    def accumulate_on_device(self, states, first_pass=False, max_approx=True):
        """The same, but the statistics stay in this corpus handle on the device (for next_model())."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        _check(lib().sr_accumulate_corpus(self.model.h, self.h, _ptr(states), int(first_pass), int(max_approx), None, None, None, None))

    def next_model(self, pooling=POOL_NONE, max_approx=True):
        """MixtureModel::finalize of the statistics accumulate_on_device() left on the device -> new Model."""
        h = C.c_void_p()
        _check(lib().sr_model_create_from_accumulated(self.model.h, self.h, pooling, int(max_approx), C.byref(h)))
        return Model(h)

    def accumulate(self, states, first_pass=False, max_approx=True):
        """EM statistics of an alignment (MixtureModel::accumulate) -> (mean_acc, mean_w, var_acc, var_w)."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        ma, mw = np.zeros((nm.value, D)), np.zeros(nm.value)
        va, vw = np.zeros((nv.value, D)), np.zeros(nv.value)
        _check(lib().sr_accumulate_corpus(self.model.h, self.h, _ptr(states), int(first_pass), int(max_approx), _ptr(ma), _ptr(mw),
                                          _ptr(va), _ptr(vw)))
        return ma, mw, va, vw

    def state_posteriors(self, automata, tdp, silence_state, kernel=GMM_DEFAULT, floor=0.0, max_items=8):
        """Forward-backward over the aligner's automata -> (cost f64[n_utts] = -log P(X | automaton), count u16[total_frames],
        state u16[total_frames, max_items], weight f64[total_frames, max_items]): per frame the mixtures with posterior >= floor,
        largest first, at most max_items (sr_state_posteriors_corpus)."""
        flat, off = self._aut(automata)
        F = max(self.n_frames, 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, max(int(max_items), 1)), dtype=np.uint16)
        weight = np.zeros((F, max(int(max_items), 1)), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_state_posteriors_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel, float(floor),
                                                int(max_items), _ptr(cost), _ptr(count), _ptr(state), _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], state[:n], weight[:n]

    def state_posteriors_scores(self, automata, tdp, silence_state, scores, floor=0.0, max_items=8):
        """sr_state_posteriors_corpus_scores (test hook): state_posteriors() on the caller's score table [n_frames, n_states]"""
        flat, off = self._aut(automata)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        F = max(self.n_frames, 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, max(int(max_items), 1)), dtype=np.uint16)
        weight = np.zeros((F, max(int(max_items), 1)), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_state_posteriors_corpus_scores(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, _ptr(scores),
                                                       scores.size, float(floor), int(max_items), _ptr(cost), _ptr(count), _ptr(state),
                                                       _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], state[:n], weight[:n]

    def _baum_welch(self, automata, tdp, silence_state, kernel, floor, first_pass, max_approx, out):
        flat, off = self._aut(automata)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_baum_welch_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel, float(floor),
                                          int(first_pass), int(max_approx), _ptr(cost), *[_ptr(a) for a in out]))
        return cost[: self.n_utts]

    def baum_welch(self, automata, tdp, silence_state, kernel=GMM_DEFAULT, floor=0.0, first_pass=False, max_approx=True):
        """One Baum-Welch E-step (sr_baum_welch_corpus) -> (cost f64[n_utts], (mean_acc, mean_w, var_acc, var_w))."""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        stats = (np.zeros((nm.value, D)), np.zeros(nm.value), np.zeros((nv.value, D)), np.zeros(nv.value))
        cost = self._baum_welch(automata, tdp, silence_state, kernel, floor, first_pass, max_approx, stats)
        return cost, stats

    def baum_welch_on_device(self, automata, tdp, silence_state, kernel=GMM_DEFAULT, floor=0.0, first_pass=False, max_approx=True):
        """The same, the statistics kept in this corpus handle for next_model() -> cost f64[n_utts]."""
        return self._baum_welch(automata, tdp, silence_state, kernel, floor, first_pass, max_approx, (None, None, None, None))

    def _fmllr_out(self, n_speakers):
        D = self.model.dim
        return np.zeros(n_speakers), np.zeros((n_speakers, D, D + 1)), np.zeros((n_speakers, D, D + 1, D + 1))

    def fmllr_statistics(self, states, utt_speaker, n_speakers, max_approx=True):
        """fMLLR statistics of an alignment per speaker (sr_fmllr_statistics_corpus) -> (beta f64[S], k f64[S, D, D+1],
        G f64[S, D, D+1, D+1])."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        assert len(spk) == self.n_utts
        beta, k, G = self._fmllr_out(n_speakers)
        _check(lib().sr_fmllr_statistics_corpus(self.model.h, self.h, _ptr(states), _ptr(spk), n_speakers, int(max_approx), _ptr(beta),
                                                _ptr(k), _ptr(G)))
        return beta, k, G

    def fmllr_statistics_bw(self, automata, tdp, silence_state, utt_speaker, n_speakers, kernel=GMM_DEFAULT, floor=0.0, max_approx=True):
        """The same from the forward-backward posteriors (sr_fmllr_statistics_bw_corpus) -> (cost f64[n_utts], (beta, k, G))."""
        flat, off = self._aut(automata)
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        assert len(spk) == self.n_utts
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        beta, k, G = self._fmllr_out(n_speakers)
        _check(lib().sr_fmllr_statistics_bw_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel, float(floor),
                                                   _ptr(spk), n_speakers, int(max_approx), _ptr(cost), _ptr(beta), _ptr(k), _ptr(G)))
        return cost[: self.n_utts], (beta, k, G)

    def _mllr_args(self, utt_speaker, n_speakers, dens_class, n_classes):
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        cls = np.ascontiguousarray(dens_class, dtype=np.uint32)
        assert len(spk) == self.n_utts and len(cls) == self.model.n_densities
        D, S, R = self.model.dim, n_speakers, n_classes
        return spk, cls, (np.zeros((S, R)), np.zeros((S, R, D, D + 1)), np.zeros((S, R, D, D + 1, D + 1)))

    def mllr_statistics(self, states, utt_speaker, n_speakers, dens_class, n_classes, max_approx=True):
        """MLLR statistics of an alignment per (speaker, regression class) (sr_mllr_statistics_corpus) -> (beta f64[S, R],
        k f64[S, R, D, D+1], G f64[S, R, D, D+1, D+1]); dens_class u32[n_densities] in mixture order."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        spk, cls, (beta, k, G) = self._mllr_args(utt_speaker, n_speakers, dens_class, n_classes)
        _check(lib().sr_mllr_statistics_corpus(self.model.h, self.h, _ptr(states), _ptr(spk), n_speakers, _ptr(cls), n_classes,
                                               int(max_approx), _ptr(beta), _ptr(k), _ptr(G)))
        return beta, k, G

    def mllr_statistics_bw(self, automata, tdp, silence_state, utt_speaker, n_speakers, dens_class, n_classes, kernel=GMM_DEFAULT,
                           floor=0.0, max_approx=True):
        """The same from the forward-backward posteriors (sr_mllr_statistics_bw_corpus) -> (cost f64[n_utts], (beta, k, G))."""
        flat, off = self._aut(automata)
        spk, cls, (beta, k, G) = self._mllr_args(utt_speaker, n_speakers, dens_class, n_classes)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_mllr_statistics_bw_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel, float(floor),
                                                  _ptr(spk), n_speakers, _ptr(cls), n_classes, int(max_approx), _ptr(cost), _ptr(beta),
                                                  _ptr(k), _ptr(G)))
        return cost[: self.n_utts], (beta, k, G)

    def _map_statistics(self, call, n_speakers):
        """the sizing call, then the filled call -> (ent_off u64[S+1], dens u32[n], occ f64[n], x f64[n, D])"""
        D = self.model.dim
        ent_off = np.zeros(n_speakers + 1, np.uint64)
        _check(call(0, ent_off, None, None, None))
        n = int(ent_off[-1])
        dens, occ, x = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1)), np.zeros((max(n, 1), D))
        _check(call(n, ent_off, dens, occ, x))
        return ent_off, dens[:n], occ[:n], x[:n]

    def map_statistics(self, states, utt_speaker, n_speakers, max_approx=True):
        """MAP statistics of an alignment per (speaker, density) with at least one pair (sr_map_statistics_corpus) -> (ent_off
        u64[S+1], dens u32[n], occ f64[n], x f64[n, D]): speaker s owns entries ent_off[s] .. ent_off[s + 1], ascending density id."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        assert len(spk) == self.n_utts
        return self._map_statistics(lambda cap, off, d, o, x: lib().sr_map_statistics_corpus(
            self.model.h, self.h, _ptr(states), _ptr(spk), n_speakers, int(max_approx), cap, _ptr(off), _ptr(d), _ptr(o), _ptr(x)), n_speakers)

    def map_statistics_bw(self, automata, tdp, silence_state, utt_speaker, n_speakers, kernel=GMM_DEFAULT, floor=0.0, max_approx=True):
        """The same from the forward-backward posteriors (sr_map_statistics_bw_corpus) -> (cost f64[n_utts], (ent_off, dens, occ, x))."""
        flat, aoff = self._aut(automata)
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        assert len(spk) == self.n_utts
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        out = self._map_statistics(lambda cap, off, d, o, x: lib().sr_map_statistics_bw_corpus(
            self.model.h, self.h, _ptr(flat), _ptr(aoff), C.byref(t3), silence_state, kernel, float(floor), _ptr(spk), n_speakers,
            int(max_approx), _ptr(cost), cap, _ptr(off), _ptr(d), _ptr(o), _ptr(x)), n_speakers)
        return cost[: self.n_utts], out

    def mllt_statistics(self, states, max_approx=True):
        """MLLT statistics of an alignment (sr_mllt_statistics_corpus) -> (beta float, G f64[D, D, D])."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        D = self.model.dim
        beta, G = np.zeros(1), np.zeros((D, D, D))
        _check(lib().sr_mllt_statistics_corpus(self.model.h, self.h, _ptr(states), int(max_approx), _ptr(beta), _ptr(G)))
        return float(beta[0]), G

    def mllt_statistics_bw(self, automata, tdp, silence_state, kernel=GMM_DEFAULT, floor=0.0, max_approx=True):
        """The same from the forward-backward posteriors (sr_mllt_statistics_bw_corpus) -> (cost f64[n_utts], (beta, G))."""
        flat, off = self._aut(automata)
        D = self.model.dim
        beta, G = np.zeros(1), np.zeros((D, D, D))
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_mllt_statistics_bw_corpus(self.model.h, self.h, _ptr(flat), _ptr(off), C.byref(t3), silence_state, kernel, float(floor),
                                                  int(max_approx), _ptr(cost), _ptr(beta), _ptr(G)))
        return cost[: self.n_utts], (float(beta[0]), G)

    def transform(self, utt_speaker, W):
        """The adapted corpus y = A x + b, W[s] = [A b] of utterance u's speaker utt_speaker[u] (sr_corpus_transform) -> Corpus."""
        spk = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        W = np.ascontiguousarray(W, dtype=np.float64)
        D = self.model.dim
        assert len(spk) == self.n_utts and W.ndim == 3 and W.shape[1:] == (D, D + 1)
        out = Corpus.__new__(Corpus)
        out.model, out.frame_off, out.n_utts, out.n_frames = self.model, self.frame_off, self.n_utts, self.n_frames
        out.h = C.c_void_p()
        _check(lib().sr_corpus_transform(self.model.h, self.h, _ptr(spk), W.shape[0], _ptr(W), C.byref(out.h)))
        return out

    def lda_statistics(self, states, context, class_of_state=None, n_classes=None):
        """LDA statistics of the frames spliced with `context` neighbours on either side (sr_lda_statistics_corpus) ->
        (count f64[K], sum f64[K, E], scatter f64[E, E]), E = (2 context + 1) D.  class_of_state u32[n_states] maps the aligned
        states to classes (LDA_SKIP: the frame is left out); None: the state is the class.  n_classes defaults to the number of
        states, or to the largest class of the map + 1."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        cls = None if class_of_state is None else np.ascontiguousarray(class_of_state, dtype=np.uint32)
        if n_classes is None:
            kept = None if cls is None else cls[cls != LDA_SKIP]
            n_classes = self.model.n_states if cls is None else (int(kept.max()) + 1 if len(kept) else 1)
        assert cls is None or len(cls) == self.model.n_states
        E = (2 * int(context) + 1) * self.model.dim
        count, total, scatter = np.zeros(n_classes), np.zeros((n_classes, E)), np.zeros((E, E))
        _check(lib().sr_lda_statistics_corpus(self.model.h, self.h, _ptr(states), int(context), _ptr(cls), int(n_classes), _ptr(count),
                                              _ptr(total), _ptr(scatter)))
        return count, total, scatter

    def splice_transform(self, target, context, M):
        """The projected corpus y = M (z, 1) of the spliced frames, M f64[p, E+1], as a resident corpus of the Model `target` of
        dimension p (sr_corpus_splice_transform) -> Corpus; close it before `target`."""
        M = np.ascontiguousarray(M, dtype=np.float64)
        E = (2 * int(context) + 1) * self.model.dim
        assert M.shape == (target.dim, E + 1)
        out = Corpus.__new__(Corpus)
        out.model, out.frame_off, out.n_utts, out.n_frames = target, self.frame_off, self.n_utts, self.n_frames
        out.h = C.c_void_p()
        _check(lib().sr_corpus_splice_transform(self.model.h, self.h, target.h, int(context), _ptr(M), C.byref(out.h)))
        return out

    def word_posteriors(self, lexicon, word_penalty, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Forward-backward over the recognition network (sr_word_posteriors_corpus) -> (cost f64[n_utts] = -(1/scale) log P(X),
        count u16[total_frames], word u32[total_frames, max_items], weight f64[total_frames, max_items]): per frame the words with
        posterior >= floor, largest first, at most max_items."""
        return self._word_posteriors(lexicon, word_penalty, scale, kernel, floor, max_items, None)

    def word_posteriors_scores(self, lexicon, word_penalty, scores, scale=1.0, floor=0.0, max_items=8):
        """sr_word_posteriors_corpus_scores (test hook): word_posteriors() on the caller's score table [n_frames, n_states] (the
        corpus's features are not read)"""
        return self._word_posteriors(lexicon, word_penalty, scale, GMM_PREFILTER, floor, max_items,
                                     np.ascontiguousarray(scores, dtype=np.float64))

    def _word_posteriors(self, lexicon, word_penalty, scale, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        word = np.zeros((F, K), dtype=np.uint32)
        weight = np.zeros((F, K), dtype=np.float64)
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        if scores is None:
            _check(lib().sr_word_posteriors_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor), int(max_items),
                                                   _ptr(cost), _ptr(count), _ptr(word), _ptr(weight)))
        else:
            _check(lib().sr_word_posteriors_corpus_scores(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor),
                                                          int(max_items), _ptr(scores), scores.size, _ptr(cost), _ptr(count), _ptr(word),
                                                          _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], word[:n], weight[:n]

    @staticmethod
    def _transcripts(transcripts):
        """list of word-id sequences -> (trans u32[], trans_off u64[n_utts + 1]); None -> (None, None): the free network"""
        if transcripts is None:
            return None, None
        off = np.concatenate([[0], np.cumsum([len(t) for t in transcripts])]).astype(np.uint64)
        flat = np.concatenate([np.asarray(t, dtype=np.uint32) for t in transcripts] + [np.zeros(1, np.uint32)])
        return np.ascontiguousarray(flat, dtype=np.uint32), off

    def net_occupancies(self, lexicon, word_penalty, scale=1.0, transcripts=None, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Mixture occupancies over the recognition network (sr_net_occupancies_corpus): the free network, or -- transcripts = one
        sequence of word ids per utterance, silence not listed -- the network restricted to them -> (cost f64[n_utts], count
        u16[total_frames], state u16[total_frames, max_items], weight f64[total_frames, max_items]) as state_posteriors."""
        return self._net_occupancies(lexicon, word_penalty, scale, transcripts, kernel, floor, max_items, None)

    def net_occupancies_scores(self, lexicon, word_penalty, scores, scale=1.0, transcripts=None, floor=0.0, max_items=8):
        """sr_net_occupancies_corpus_scores (test hook): net_occupancies() on the caller's score table [n_frames, n_states]"""
        return self._net_occupancies(lexicon, word_penalty, scale, transcripts, GMM_PREFILTER, floor, max_items,
                                     np.ascontiguousarray(scores, dtype=np.float64))

    def _net_occupancies(self, lexicon, word_penalty, scale, transcripts, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, K), dtype=np.uint16)
        weight = np.zeros((F, K), dtype=np.float64)
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        flat, off = self._transcripts(transcripts)
        if scores is None:
            _check(lib().sr_net_occupancies_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor), int(max_items),
                                                   _ptr(flat), _ptr(off), _ptr(cost), _ptr(count), _ptr(state), _ptr(weight)))
        else:
            _check(lib().sr_net_occupancies_corpus_scores(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor),
                                                          int(max_items), _ptr(flat), _ptr(off), _ptr(scores), scores.size, _ptr(cost),
                                                          _ptr(count), _ptr(state), _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], state[:n], weight[:n]

    def mmi_statistics(self, lexicon, word_penalty, transcripts, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_approx=True):
        """One MMI E-step (sr_mmi_statistics_corpus) -> (F_num f64[n_utts], F_den f64[n_utts], num, den), each side's statistics
        (mean_acc, mean_w, var_acc, var_w) over the utterances with finite F_num."""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        num, den = ((np.zeros((nm.value, D)), np.zeros(nm.value), np.zeros((nv.value, D)), np.zeros(nv.value)) for _ in range(2))
        fn, fd = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        flat, off = self._transcripts(transcripts)
        _check(lib().sr_mmi_statistics_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor), int(max_approx),
                                              _ptr(flat), _ptr(off), _ptr(fn), _ptr(fd), *[_ptr(a) for a in num + den]))
        return fn[: self.n_utts], fd[: self.n_utts], num, den

    def net_accuracies(self, lexicon, word_penalty, ref_states, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Expected frame accuracy over the free recognition network (sr_net_accuracies_corpus); ref_states u16[total_frames] = the
        reference mixture of every frame -> (cost f64[n_utts], acc f64[n_utts], count u16[total_frames], state u16[total_frames,
        max_items], weight f64[total_frames, max_items]): per frame the signed gamma, largest |gamma| first."""
        return self._net_accuracies(lexicon, word_penalty, ref_states, scale, kernel, floor, max_items, None)

    def net_accuracies_scores(self, lexicon, word_penalty, ref_states, scores, scale=1.0, floor=0.0, max_items=8):
        """sr_net_accuracies_corpus_scores (test hook): net_accuracies() on the caller's score table [n_frames, n_states]"""
        return self._net_accuracies(lexicon, word_penalty, ref_states, scale, GMM_PREFILTER, floor, max_items,
                                    np.ascontiguousarray(scores, dtype=np.float64))

    def _net_accuracies(self, lexicon, word_penalty, ref_states, scale, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost, acc = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, K), dtype=np.uint16)
        weight = np.zeros((F, K), dtype=np.float64)
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        ref = np.ascontiguousarray(np.concatenate([np.asarray(ref_states, dtype=np.uint16), np.zeros(1, np.uint16)]))
        if scores is None:
            _check(lib().sr_net_accuracies_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor), int(max_items),
                                                  _ptr(ref), _ptr(cost), _ptr(acc), _ptr(count), _ptr(state), _ptr(weight)))
        else:
            _check(lib().sr_net_accuracies_corpus_scores(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor),
                                                         int(max_items), _ptr(ref), _ptr(scores), scores.size, _ptr(cost), _ptr(acc),
                                                         _ptr(count), _ptr(state), _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], acc[: self.n_utts], count[:n], state[:n], weight[:n]

    def smbr_statistics(self, lexicon, word_penalty, ref_states, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_approx=True):
        """One sMBR E-step (sr_smbr_statistics_corpus) -> (F f64[n_utts], Abar f64[n_utts], num, den), each side's statistics
        (mean_acc, mean_w, var_acc, var_w) as mmi_statistics': num from the positive gamma, den from the negative."""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        num, den = ((np.zeros((nm.value, D)), np.zeros(nm.value), np.zeros((nv.value, D)), np.zeros(nv.value)) for _ in range(2))
        cost, acc = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        ref = np.ascontiguousarray(np.concatenate([np.asarray(ref_states, dtype=np.uint16), np.zeros(1, np.uint16)]))
        _check(lib().sr_smbr_statistics_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), float(floor), int(max_approx),
                                               _ptr(ref), _ptr(cost), _ptr(acc), *[_ptr(a) for a in num + den]))
        return cost[: self.n_utts], acc[: self.n_utts], num, den

    def recognize_confidence(self, lexicon, am_threshold, word_penalty, scale=1.0, kernel=GMM_PREFILTER):
        """recognize()'s words with a confidence each (sr_recognize_confidence_corpus) -> (words u32[], word_off u64[n_utts+1],
        conf f64[], first u32[], last u32[]): conf = max posterior of the word over its frames first .. last (within the utterance)."""
        F = max(self.n_frames, 1)
        words = np.zeros(F, dtype=np.uint32)
        woff = np.zeros(self.n_utts + 1, dtype=np.uint64)
        conf = np.zeros(F, dtype=np.float64)
        first = np.zeros(F, dtype=np.uint32)
        last = np.zeros(F, dtype=np.uint32)
        sp = SearchParams(am_threshold, word_penalty, kernel, 0)
        _check(lib().sr_recognize_confidence_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(scale), _ptr(words), _ptr(woff),
                                                    _ptr(conf), _ptr(first), _ptr(last)))
        n = int(woff[-1])
        return words[:n].copy(), woff, conf[:n].copy(), first[:n].copy(), last[:n].copy()

    def word_lattice(self, lexicon, word_penalty, lattice_beam=np.inf, kernel=GMM_PREFILTER):
        """Word lattices over the recognition network (sr_word_lattice_corpus: the sizing call, then the filling call) ->
        (arc_off u64[n_utts+1], best f64[n_utts], word u32[], first u32[], last u32[], fwd f64[], bwd f64[], cost f64[]): utterance
        u owns arcs arc_off[u] .. arc_off[u+1], in (last, word) order, the frames counted within the utterance."""
        sp = SearchParams(np.inf, word_penalty, kernel, 0)
        off = np.zeros(self.n_utts + 1, dtype=np.uint64)
        best = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        _check(lib().sr_word_lattice_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(lattice_beam), 0, _ptr(off), _ptr(best),
                                            None, None, None, None, None, None))
        n = int(off[-1])
        cap = max(n, 1)
        word, first, last = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        fwd, bwd, cost = (np.zeros(cap, dtype=np.float64) for _ in range(3))
        _check(lib().sr_word_lattice_corpus(self.model.h, self.h, lexicon.h, C.byref(sp), float(lattice_beam), cap, _ptr(off), _ptr(best),
                                            _ptr(word), _ptr(first), _ptr(last), _ptr(fwd), _ptr(bwd), _ptr(cost)))
        return off, best[: self.n_utts], word[:n], first[:n], last[:n], fwd[:n], bwd[:n], cost[:n]

    def recognize_bigram(self, bigram, acoustic_pruning=FLT_MAX, lm_pruning=FLT_MAX, kernel=GMM_PREFILTER, max_word_ends=0, dense_states=False,
                         global_states=False):
        """-> (words u32[], scores f32[], times u32[], off u64[n_utts+1]): LinearSearch::getResult per utterance.
        dense_states / global_states force the dense LDS image / the state hypotheses in device memory (both: SrError)."""
        cap = max(self.n_frames + self.n_utts, 1)
        ow, osc, ot = np.zeros(cap, np.uint32), np.zeros(cap, np.float32), np.zeros(cap, np.uint32)
        off = np.zeros(self.n_utts + 1, np.uint64)
        p = BigramParams(acoustic_pruning, lm_pruning, kernel, max_word_ends, (BIGRAM_DENSE_STATES if dense_states else 0) | (BIGRAM_GLOBAL_STATES if global_states else 0))
        _check(lib().sr_recognize_bigram_corpus(self.model.h, self.h, bigram.h, C.byref(p), _ptr(ow), _ptr(osc), _ptr(ot), _ptr(off)))
        n = int(off[-1])
        return ow[:n], osc[:n], ot[:n], off

    def recognize_bigram_scores(self, bigram, scores, acoustic_pruning=FLT_MAX, lm_pruning=FLT_MAX, max_word_ends=0, dense_states=False,
                                global_states=False):
        """sr_recognize_bigram_corpus_scores (test hook): the bigram search alone on the caller's score table [n_frames, n_states] (the
        corpus's features are not read) -> as recognize_bigram"""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        cap = max(self.n_frames + self.n_utts, 1)
        ow, osc, ot = np.zeros(cap, np.uint32), np.zeros(cap, np.float32), np.zeros(cap, np.uint32)
        off = np.zeros(self.n_utts + 1, np.uint64)
        p = BigramParams(acoustic_pruning, lm_pruning, GMM_DEFAULT, max_word_ends, (BIGRAM_DENSE_STATES if dense_states else 0) | (BIGRAM_GLOBAL_STATES if global_states else 0))
        _check(lib().sr_recognize_bigram_corpus_scores(self.model.h, self.h, bigram.h, C.byref(p), _ptr(scores), scores.size, _ptr(ow), _ptr(osc),
                                                       _ptr(ot), _ptr(off)))
        n = int(off[-1])
        return ow[:n], osc[:n], ot[:n], off

    def bigram_word_posteriors(self, bigram, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Forward-backward over the bigram search network (sr_bigram_word_posteriors_corpus) -> (cost, count, word, weight) as
        word_posteriors; the silence word's posterior includes its copies."""
        return self._bigram_word_posteriors(bigram, scale, kernel, floor, max_items, None)

    def bigram_word_posteriors_scores(self, bigram, scores, scale=1.0, floor=0.0, max_items=8):
        """sr_bigram_word_posteriors_corpus_scores (test hook): bigram_word_posteriors() on the caller's score table [n_frames,
        n_states] (the corpus's features are not read)"""
        return self._bigram_word_posteriors(bigram, scale, GMM_PREFILTER, floor, max_items, np.ascontiguousarray(scores, dtype=np.float64))

    def _bigram_word_posteriors(self, bigram, scale, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        word = np.zeros((F, K), dtype=np.uint32)
        weight = np.zeros((F, K), dtype=np.float64)
        if scores is None:
            _check(lib().sr_bigram_word_posteriors_corpus(self.model.h, self.h, bigram.h, kernel, float(scale), float(floor), int(max_items),
                                                          _ptr(cost), _ptr(count), _ptr(word), _ptr(weight)))
        else:
            _check(lib().sr_bigram_word_posteriors_corpus_scores(self.model.h, self.h, bigram.h, float(scale), float(floor), int(max_items),
                                                                 _ptr(scores), scores.size, _ptr(cost), _ptr(count), _ptr(word),
                                                                 _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], word[:n], weight[:n]

    def bigram_occupancies(self, bigram, scale=1.0, transcripts=None, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Mixture occupancies over the bigram search network (sr_bigram_occupancies_corpus): the free network, or -- transcripts =
        one sequence of word ids per utterance, silence not listed -- the network restricted to them -> (cost, count, state,
        weight) as net_occupancies."""
        return self._bigram_occupancies(bigram, scale, transcripts, kernel, floor, max_items, None)

    def bigram_occupancies_scores(self, bigram, scores, scale=1.0, transcripts=None, floor=0.0, max_items=8):
        """sr_bigram_occupancies_corpus_scores (test hook): bigram_occupancies() on the caller's score table [n_frames, n_states]"""
        return self._bigram_occupancies(bigram, scale, transcripts, GMM_PREFILTER, floor, max_items,
                                        np.ascontiguousarray(scores, dtype=np.float64))

    def _bigram_occupancies(self, bigram, scale, transcripts, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, K), dtype=np.uint16)
        weight = np.zeros((F, K), dtype=np.float64)
        flat, off = self._transcripts(transcripts)
        if scores is None:
            _check(lib().sr_bigram_occupancies_corpus(self.model.h, self.h, bigram.h, kernel, float(scale), float(floor), int(max_items),
                                                      _ptr(flat), _ptr(off), _ptr(cost), _ptr(count), _ptr(state), _ptr(weight)))
        else:
            _check(lib().sr_bigram_occupancies_corpus_scores(self.model.h, self.h, bigram.h, float(scale), float(floor), int(max_items),
                                                             _ptr(flat), _ptr(off), _ptr(scores), scores.size, _ptr(cost), _ptr(count),
                                                             _ptr(state), _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], count[:n], state[:n], weight[:n]

    def bigram_mmi_statistics(self, bigram, transcripts, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_approx=True):
        """One MMI E-step against the bigram search network (sr_bigram_mmi_statistics_corpus) -> (F_num, F_den, num, den) as
        mmi_statistics.  After Model.from_mmi_statistics the next iteration needs a Model.bigram of the NEW model."""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        num, den = ((np.zeros((nm.value, D)), np.zeros(nm.value), np.zeros((nv.value, D)), np.zeros(nv.value)) for _ in range(2))
        fn, fd = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        flat, off = self._transcripts(transcripts)
        _check(lib().sr_bigram_mmi_statistics_corpus(self.model.h, self.h, bigram.h, kernel, float(scale), float(floor), int(max_approx),
                                                     _ptr(flat), _ptr(off), _ptr(fn), _ptr(fd), *[_ptr(a) for a in num + den]))
        return fn[: self.n_utts], fd[: self.n_utts], num, den

    def bigram_accuracies(self, bigram, ref_states, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_items=8):
        """Expected frame accuracy over the free bigram search network (sr_bigram_accuracies_corpus); ref_states u16[total_frames] =
        the reference mixture of every frame -> (cost, acc, count, state, weight) as net_accuracies: per frame the signed gamma,
        largest |gamma| first."""
        return self._bigram_accuracies(bigram, ref_states, scale, kernel, floor, max_items, None)

    def bigram_accuracies_scores(self, bigram, ref_states, scores, scale=1.0, floor=0.0, max_items=8):
        """sr_bigram_accuracies_corpus_scores (test hook): bigram_accuracies() on the caller's score table [n_frames, n_states]"""
        return self._bigram_accuracies(bigram, ref_states, scale, GMM_PREFILTER, floor, max_items,
                                       np.ascontiguousarray(scores, dtype=np.float64))

    def _bigram_accuracies(self, bigram, ref_states, scale, kernel, floor, max_items, scores):
        F = max(self.n_frames, 1)
        K = max(int(max_items), 1)
        cost, acc = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        count = np.zeros(F, dtype=np.uint16)
        state = np.zeros((F, K), dtype=np.uint16)
        weight = np.zeros((F, K), dtype=np.float64)
        ref = np.ascontiguousarray(np.concatenate([np.asarray(ref_states, dtype=np.uint16), np.zeros(1, np.uint16)]))
        if scores is None:
            _check(lib().sr_bigram_accuracies_corpus(self.model.h, self.h, bigram.h, kernel, float(scale), float(floor), int(max_items),
                                                     _ptr(ref), _ptr(cost), _ptr(acc), _ptr(count), _ptr(state), _ptr(weight)))
        else:
            _check(lib().sr_bigram_accuracies_corpus_scores(self.model.h, self.h, bigram.h, float(scale), float(floor), int(max_items),
                                                            _ptr(ref), _ptr(scores), scores.size, _ptr(cost), _ptr(acc), _ptr(count),
                                                            _ptr(state), _ptr(weight)))
        n = self.n_frames
        return cost[: self.n_utts], acc[: self.n_utts], count[:n], state[:n], weight[:n]

    def bigram_smbr_statistics(self, bigram, ref_states, scale=1.0, kernel=GMM_PREFILTER, floor=0.0, max_approx=True):
        """One sMBR E-step against the bigram search network (sr_bigram_smbr_statistics_corpus) -> (F, Abar, num, den) as
        smbr_statistics.  After Model.from_mmi_statistics the next iteration needs a Model.bigram of the NEW model."""
        nm, nv = C.c_uint32(), C.c_uint32()
        _check(lib().sr_model_tying_info(self.model.h, C.byref(nm), C.byref(nv)))
        D = self.model.dim
        num, den = ((np.zeros((nm.value, D)), np.zeros(nm.value), np.zeros((nv.value, D)), np.zeros(nv.value)) for _ in range(2))
        cost, acc = (np.zeros(max(self.n_utts, 1), dtype=np.float64) for _ in range(2))
        ref = np.ascontiguousarray(np.concatenate([np.asarray(ref_states, dtype=np.uint16), np.zeros(1, np.uint16)]))
        _check(lib().sr_bigram_smbr_statistics_corpus(self.model.h, self.h, bigram.h, kernel, float(scale), float(floor), int(max_approx),
                                                      _ptr(ref), _ptr(cost), _ptr(acc), *[_ptr(a) for a in num + den]))
        return cost[: self.n_utts], acc[: self.n_utts], num, den

    def recognize_bigram_confidence(self, bigram, scale=1.0, acoustic_pruning=FLT_MAX, lm_pruning=FLT_MAX, kernel=GMM_PREFILTER,
                                    max_word_ends=0, dense_states=False, global_states=False):
        """recognize_bigram()'s items with a confidence each (sr_recognize_bigram_confidence_corpus) -> (words u32[], scores f32[],
        times u32[], off u64[n_utts+1], conf f64[]): conf = max posterior of the item's word over its frames."""
        cap = max(self.n_frames + self.n_utts, 1)
        ow, osc, ot = np.zeros(cap, np.uint32), np.zeros(cap, np.float32), np.zeros(cap, np.uint32)
        conf = np.zeros(cap, np.float64)
        off = np.zeros(self.n_utts + 1, np.uint64)
        p = BigramParams(acoustic_pruning, lm_pruning, kernel, max_word_ends, (BIGRAM_DENSE_STATES if dense_states else 0) | (BIGRAM_GLOBAL_STATES if global_states else 0))
        _check(lib().sr_recognize_bigram_confidence_corpus(self.model.h, self.h, bigram.h, C.byref(p), float(scale), _ptr(ow), _ptr(osc),
                                                           _ptr(ot), _ptr(off), _ptr(conf)))
        n = int(off[-1])
        return ow[:n], osc[:n], ot[:n], off, conf[:n]

    def bigram_word_lattice(self, bigram, lattice_beam=np.inf, kernel=GMM_PREFILTER):
        """Word lattices over the bigram search network (sr_bigram_word_lattice_corpus: the sizing call, then the filling call) ->
        (arc_off u64[n_utts+1], best f64[n_utts], word u32[], hist u32[], pred u32[], first u32[], last u32[], fwd f64[], bwd f64[],
        am f64[]): utterance u owns arcs arc_off[u] .. arc_off[u+1], in (last, slot) order, the frames counted within the utterance."""
        off = np.zeros(self.n_utts + 1, dtype=np.uint64)
        best = np.zeros(max(self.n_utts, 1), dtype=np.float64)
        _check(lib().sr_bigram_word_lattice_corpus(self.model.h, self.h, bigram.h, kernel, float(lattice_beam), 0, _ptr(off), _ptr(best),
                                                   *([None] * 8)))
        n = int(off[-1])
        cap = max(n, 1)
        word, hist, pred, first, last = (np.zeros(cap, dtype=np.uint32) for _ in range(5))
        fwd, bwd, am = (np.zeros(cap, dtype=np.float64) for _ in range(3))
        _check(lib().sr_bigram_word_lattice_corpus(self.model.h, self.h, bigram.h, kernel, float(lattice_beam), cap, _ptr(off), _ptr(best),
                                                   _ptr(word), _ptr(hist), _ptr(pred), _ptr(first), _ptr(last), _ptr(fwd), _ptr(bwd),
                                                   _ptr(am)))
        return off, best[: self.n_utts], word[:n], hist[:n], pred[:n], first[:n], last[:n], fwd[:n], bwd[:n], am[:n]

    def path_scores(self, states, kernel=GMM_PREFILTER):
        """Emission cost along a state path (one state per frame): Trainer::calc_am_score's summands."""
        states = np.ascontiguousarray(states, dtype=np.uint16)
        out = np.zeros(max(self.n_frames, 1), dtype=np.float64)
        _check(lib().sr_path_scores_corpus(self.model.h, self.h, _ptr(states), kernel, _ptr(out)))
        return out[: self.n_frames]


class FrontEnd:
    """sr_frontend handle: PCM samples or static cepstra in, a resident Corpus of the model out (Model.frontend)."""

    def __init__(self, model, mfcc, post, vtln=None):
        self.model = model
        self.n_warps = 0
        post = dict(post)
        mean, stddev = post.pop("mean", None), post.pop("stddev", None)
        self._mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        self._stddev = None if stddev is None else np.ascontiguousarray(stddev, dtype=np.float64)
        self.post = FeaturePostParams(mean=_ptr(self._mean), stddev=_ptr(self._stddev), **{k: int(v) for k, v in post.items()})
        self.mfcc_params = None
        if mfcc is not None:
            ints = ("window", "shift", "n_fft", "n_mel", "n_cepstra", "flags")
            self.mfcc_params = MfccParams(**{k: (int(v) if k in ints else float(v)) for k, v in mfcc.items()})
        self.n_static = self.post.n_static
        self.h = C.c_void_p()
        mp = None if self.mfcc_params is None else C.byref(self.mfcc_params)
        if vtln is None:
            _check(lib().sr_frontend_create(model.h, mp, C.byref(self.post), C.byref(self.h)))
            return
        self.alpha = np.ascontiguousarray(vtln["alpha"], dtype=np.float64)
        vp = VtlnParams(n_warps=len(self.alpha), alpha=_ptr(self.alpha), break_frac=float(vtln["break_frac"]))
        _check(lib().sr_frontend_create_warped(model.h, mp, C.byref(vp), C.byref(self.post), C.byref(self.h)))
        n = C.c_uint32()
        _check(lib().sr_frontend_warps(self.h, C.byref(n)))
        self.n_warps = n.value

    def close(self):
        if self.h:
            lib().sr_frontend_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def frames(self, n_samples):
        """sr_frontend_frames: the frames of an utterance of n_samples"""
        n = C.c_uint64()
        _check(lib().sr_frontend_frames(self.h, int(n_samples), C.byref(n)))
        return n.value

    def _corpus(self, handle, frame_off):
        out = Corpus.__new__(Corpus)
        out.model, out.frame_off, out.n_utts, out.n_frames = self.model, frame_off, len(frame_off) - 1, int(frame_off[-1])
        out.h = handle
        return out

    def from_audio(self, samples, sample_off):
        """sr_corpus_from_audio: int16 samples, utterance u's at sample_off[u] .. sample_off[u + 1] -> Corpus (its frame_off tells the
        frames); close it before the model."""
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        n = len(sample_off) - 1
        assert len(samples) >= int(sample_off[-1])
        frame_off = np.zeros(n + 1, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().sr_corpus_from_audio(self.h, _ptr(samples), _ptr(sample_off), n, C.byref(h), _ptr(frame_off)))
        return self._corpus(h, frame_off)

    def from_audio_warped(self, samples, sample_off, utt_warp):
        """sr_corpus_from_audio_warped: from_audio with utterance u through the filters of warp utt_warp[u] (a warped front end)"""
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        utt_warp = np.ascontiguousarray(utt_warp, dtype=np.uint32)
        n = len(sample_off) - 1
        assert len(samples) >= int(sample_off[-1]) and len(utt_warp) == n
        frame_off = np.zeros(n + 1, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().sr_corpus_from_audio_warped(self.h, _ptr(samples), _ptr(sample_off), n, _ptr(utt_warp), C.byref(h), _ptr(frame_off)))
        return self._corpus(h, frame_off)

    def vtln_chunks(self, n_frames, n_utts):
        """sr_vtln_chunks: the chunks of warps vtln_costs takes for that many frames and utterances (the model's SRGPU_VTLN_KB budget)"""
        n = C.c_uint32()
        _check(lib().sr_vtln_chunks(self.h, int(n_frames), int(n_utts), C.byref(n)))
        return n.value

    def vtln_costs(self, samples, sample_off, states, utt_speaker, n_speakers):
        """sr_vtln_costs_corpus: the warp search.  states u16[frames]: an alignment of the unwarped corpus; utt_speaker u32[n_utts]
        -> (cost f64[n_speakers, n_warps], the emission cost of a speaker's utterances under every warp, smaller is better;
        frames u64[n_speakers])"""
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        states = np.ascontiguousarray(states, dtype=np.uint16)
        utt_speaker = np.ascontiguousarray(utt_speaker, dtype=np.uint32)
        n = len(sample_off) - 1
        assert len(samples) >= int(sample_off[-1]) and len(utt_speaker) == n
        if self.mfcc_params is not None and n and (np.diff(sample_off.astype(np.int64)) >= 0).all():
            # sr_frontend_frames' rule on the host: the C side does not know how long `states` is
            lens, window, shift = np.diff(sample_off.astype(np.int64)), self.mfcc_params.window, max(self.mfcc_params.shift, 1)
            assert len(states) == int(np.where(lens < window, 0, 1 + (lens - window) // shift).sum())
        cost = np.zeros((int(n_speakers), self.n_warps), dtype=np.float64)
        frames = np.zeros(int(n_speakers), dtype=np.uint64)
        _check(lib().sr_vtln_costs_corpus(self.h, _ptr(samples), _ptr(sample_off), n, _ptr(states), _ptr(utt_speaker), int(n_speakers),
                                          _ptr(cost), _ptr(frames)))
        return cost, frames

    def from_cepstra(self, cepstra, frame_off):
        """sr_corpus_from_cepstra: static cepstra f32[frames, n_static] -> Corpus; close it before the model."""
        cepstra = np.ascontiguousarray(cepstra, dtype=np.float32)
        frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
        assert cepstra.size == int(frame_off[-1]) * self.n_static
        h = C.c_void_p()
        _check(lib().sr_corpus_from_cepstra(self.h, _ptr(cepstra), _ptr(frame_off), len(frame_off) - 1, C.byref(h)))
        return self._corpus(h, frame_off)

    def mfcc(self, samples, sample_off):
        """sr_mfcc_corpus: the static cepstra alone -> (f32[frames, n_cepstra], frame_off u64[n_utts + 1])"""
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        n = len(sample_off) - 1
        assert len(samples) >= int(sample_off[-1])
        total = sum(self.frames(int(sample_off[u + 1]) - int(sample_off[u])) for u in range(n))
        out = np.empty((total, self.n_static), dtype=np.float32)
        frame_off = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().sr_mfcc_corpus(self.h, _ptr(samples), _ptr(sample_off), n, _ptr(out), _ptr(frame_off)))
        return out, frame_off


class Lexicon:
    """sr_lexicon handle: flattened Lexicon + TdpModel (sietill/Lexicon.hpp:16-33, TdpModel.hpp:13-29)."""

    def __init__(self, model, word_off, automaton, silence_idx, tdp, silence_state):
        word_off = np.ascontiguousarray(word_off, dtype=np.uint32)
        automaton = np.ascontiguousarray(automaton, dtype=np.uint16)
        self.h = C.c_void_p()
        t3 = (C.c_double * 3)(*tdp)
        _check(lib().sr_lexicon_create(model.h, len(word_off) - 1, _ptr(word_off), _ptr(automaton), silence_idx, C.byref(t3),
                                       silence_state, C.byref(self.h)))

    def describe(self):
        """Which search kernel sr_recognize_corpus runs on this lexicon (sr_lexicon_describe)."""
        buf = C.create_string_buffer(128)
        _check(lib().sr_lexicon_describe(self.h, buf, len(buf)))
        return buf.value.decode()

    def close(self):
        if self.h:
            lib().sr_lexicon_destroy(self.h)
            self.h = None


def fmllr_estimate(beta, k, G, n_sweeps=10, min_count=0.0, W=None):
    """Row-by-row fMLLR estimate per speaker (sr_fmllr_estimate; host code) from W (default: identity) -> (W f64[S, D, D+1],
    aux f64[S, n_sweeps+1] = Q after 0 .. n_sweeps sweeps, logdet f64[S], status i32[S])."""
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    k = np.ascontiguousarray(k, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    S, D = k.shape[0], k.shape[1]
    assert beta.shape == (S,) and k.shape == (S, D, D + 1) and G.shape == (S, D, D + 1, D + 1)
    if W is None:
        W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (S, 1, 1))
    W = np.array(W, dtype=np.float64, order="C")
    aux = np.zeros((S, int(n_sweeps) + 1))
    logdet = np.zeros(S)
    status = np.zeros(S, dtype=np.int32)
    _check(lib().sr_fmllr_estimate(D, S, _ptr(beta), _ptr(k), _ptr(G), int(n_sweeps), float(min_count), _ptr(W), _ptr(aux), _ptr(logdet),
                                   _ptr(status)))
    return W, aux, logdet, status


def mllr_estimate(beta, k, G, parent=None, min_count=0.0, W=None):
    """MLLR mean transforms per (speaker, regression class) over a regression-class tree (sr_mllr_estimate; host code):
    parent i32[n_nodes] with the R base classes as nodes 0 .. R-1 (default: no tree), W the start (default: identity)
    -> (W f64[S, R, D, D+1], node i32[S, R] = the node whose statistics gave the transform or -1, aux f64[S, R, 2] = Q of that node at
    the W given and at the result)."""
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    k = np.ascontiguousarray(k, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    S, R, D = k.shape[0], k.shape[1], k.shape[2]
    assert beta.shape == (S, R) and k.shape == (S, R, D, D + 1) and G.shape == (S, R, D, D + 1, D + 1)
    parent = np.full(R, -1, np.int32) if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
    if W is None:
        W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (S, R, 1, 1))
    W = np.array(W, dtype=np.float64, order="C")
    node = np.zeros((S, R), dtype=np.int32)
    aux = np.zeros((S, R, 2))
    _check(lib().sr_mllr_estimate(D, S, R, len(parent), _ptr(parent), _ptr(beta), _ptr(k), _ptr(G), float(min_count), _ptr(W), _ptr(node),
                                  _ptr(aux)))
    return W, node, aux


def mllt_estimate(beta, G, n_sweeps=10, min_count=0.0, A=None):
    """Row-by-row MLLT / global semi-tied estimate (sr_mllt_estimate; host code) from A (default: identity) -> (A f64[D, D],
    aux f64[n_sweeps+1] = Q after 0 .. n_sweeps sweeps, logdet float, status int)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    D = G.shape[0]
    assert G.shape == (D, D, D)
    A = np.array(np.eye(D) if A is None else A, dtype=np.float64, order="C")
    assert A.shape == (D, D)
    aux = np.zeros(int(n_sweeps) + 1)
    logdet = np.zeros(1)
    status = np.zeros(1, dtype=np.int32)
    _check(lib().sr_mllt_estimate(D, float(beta), _ptr(G), int(n_sweeps), float(min_count), _ptr(A), _ptr(aux), _ptr(logdet), _ptr(status)))
    return A, aux, float(logdet[0]), int(status[0])


def lda_estimate(count, sum, scatter, p, remove_mean=False, min_count=0.0, M=None):
    """The LDA projection from Corpus.lda_statistics' output (sr_lda_estimate; host code) -> (M f64[p, E+1] = [A b],
    eig f64[E] descending, status int).  With status 1 or 2 M is the one given (default: zeros) and eig is NaN."""
    count = np.ascontiguousarray(count, dtype=np.float64)
    total = np.ascontiguousarray(sum, dtype=np.float64)
    scatter = np.ascontiguousarray(scatter, dtype=np.float64)
    K, E = total.shape
    assert count.shape == (K,) and scatter.shape == (E, E)
    M = np.array(np.zeros((int(p), E + 1)) if M is None else M, dtype=np.float64, order="C")
    assert M.shape == (int(p), E + 1)
    eig = np.full(E, np.nan)
    status = np.zeros(1, dtype=np.int32)
    _check(lib().sr_lda_estimate(E, K, _ptr(count), _ptr(total), _ptr(scatter), int(p), int(bool(remove_mean)), float(min_count), _ptr(M),
                                 _ptr(eig), _ptr(status)))
    return M, eig, int(status[0])


def mllt_affine(A):
    """[A 0] as f64[1, D, D+1]: the W of Corpus.transform (one speaker) and Model.transform_means (one class) that applies A."""
    A = np.asarray(A, dtype=np.float64)
    return np.ascontiguousarray(np.hstack([A, np.zeros((A.shape[0], 1))])[None])


def commit_points(model, parents, sets, floors=None):
    """sr_commit_points (test hook): per set i the nearest common ancestor of the nodes sets[i] in the tree parents[i] (parents[i][0] = 0,
    parents[i][j] < j), found by the device fold of the stable calls; floors[i] (default 0) is an ancestor of all of sets[i]."""
    n = len(parents)
    assert len(sets) == n
    node_off = np.concatenate([[0], np.cumsum([len(p) for p in parents])]).astype(np.uint64)
    set_off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.uint64)
    parent = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32) for p in parents]) if n else np.zeros(0, np.uint32), dtype=np.uint32)
    nodes = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32) for x in sets]) if n else np.zeros(0, np.uint32), dtype=np.uint32)
    floor = np.ascontiguousarray(np.zeros(n, np.uint32) if floors is None else floors, dtype=np.uint32)
    out = np.zeros(max(n, 1), np.uint32)
    if len(parent) == 0:
        parent = np.zeros(1, np.uint32)
    if len(nodes) == 0:
        nodes = np.zeros(1, np.uint32)
    _check(lib().sr_commit_points(model.h, n, _ptr(node_off), _ptr(parent), _ptr(set_off), _ptr(nodes), _ptr(floor), _ptr(out)))
    return out[:n]


def traceback_words(tb_word, tb_bkp, silence_word, n_words):
    """sr_traceback_words: Recognizer.cpp:222-231 on one utterance's traceback[0..T] (host side, guarded)."""
    tb_word = np.ascontiguousarray(tb_word, dtype=np.uint16)
    tb_bkp = np.ascontiguousarray(tb_bkp, dtype=np.uint16)
    T = len(tb_word) - 1
    out = np.zeros(max(T, 1), dtype=np.uint32)
    n = C.c_uint32(0)
    _check(lib().sr_traceback_words(T, _ptr(tb_word), _ptr(tb_bkp), silence_word, n_words, _ptr(out), C.byref(n)))
    return out[: n.value].copy()


def lattice_nbest(n_frames, word, first, last, cost, silence_word, n_best, words_cap=None):
    """sr_lattice_nbest on one utterance's arcs (host side) -> [(words u32[], cost)]: the n_best cheapest distinct word strings
    among the lattice paths, cheapest first."""
    word, first, last = (np.ascontiguousarray(a, dtype=np.uint32) for a in (word, first, last))
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    assert len(word) == len(first) == len(last) == len(cost)
    K = max(int(n_best), 1)
    cap = K * max(int(n_frames), 1) if words_cap is None else int(words_cap)  # (a path has at most one word per frame)
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    off = np.zeros(K + 1, dtype=np.uint64)
    oc = np.zeros(K, dtype=np.float64)
    n = C.c_uint32(0)
    _check(lib().sr_lattice_nbest(int(n_frames), len(word), _ptr(word), _ptr(first), _ptr(last), _ptr(cost), int(silence_word), int(n_best),
                                  _ptr(out), cap, _ptr(off), _ptr(oc), C.byref(n)))
    return [(out[int(off[k]):int(off[k + 1])].copy(), float(oc[k])) for k in range(n.value)]


def bigram_lattice_nbest(n_frames, word, hist, first, last, am, silence_word, lm, n_best, lm_scale=1.0, words_cap=None):
    """sr_bigram_lattice_nbest on one utterance's arcs (host side) -> [(words u32[], cost)]: the n_best cheapest distinct word
    strings among the lattice paths, cheapest first; lm [W x W] float32 as for Bigram (another table: LM rescoring)."""
    word, hist, first, last = (np.ascontiguousarray(a, dtype=np.uint32) for a in (word, hist, first, last))
    am = np.ascontiguousarray(am, dtype=np.float64)
    lm = np.ascontiguousarray(lm, dtype=np.float32)
    assert len(word) == len(hist) == len(first) == len(last) == len(am) and lm.ndim == 2 and lm.shape[0] == lm.shape[1]
    K = max(int(n_best), 1)
    cap = K * max(int(n_frames), 1) if words_cap is None else int(words_cap)  # (a path has at most one word per frame)
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    off = np.zeros(K + 1, dtype=np.uint64)
    oc = np.zeros(K, dtype=np.float64)
    n = C.c_uint32(0)
    _check(lib().sr_bigram_lattice_nbest(int(n_frames), len(word), _ptr(word), _ptr(hist), _ptr(first), _ptr(last), _ptr(am), lm.shape[0],
                                         int(silence_word), _ptr(lm), float(lm_scale), int(n_best), _ptr(out), cap, _ptr(off), _ptr(oc),
                                         C.byref(n)))
    return [(out[int(off[k]):int(off[k + 1])].copy(), float(oc[k])) for k in range(n.value)]


def mixset_write(path, dim, dens_off, dens_mean, dens_var, acc):
    """MixtureModel::write: EM statistics + topology -> MIXSET v2 file."""
    dens_off, dens_mean, dens_var = (np.ascontiguousarray(x, dtype=np.uint32) for x in (dens_off, dens_mean, dens_var))
    ma, mw, va, vw = (np.ascontiguousarray(x, dtype=np.float64) for x in acc)
    _check(lib().sr_mixset_write(str(path).encode(), dim, len(dens_off) - 1, _ptr(dens_off), len(mw), len(vw), _ptr(dens_mean),
                                 _ptr(dens_var), _ptr(ma), _ptr(mw), _ptr(va), _ptr(vw)))


def vtln_choose(cost, frames, min_frames=0, fallback=0):
    """sr_vtln_choose (host only): cost f64[n_speakers, n_warps], frames u64[n_speakers] -> u32[n_speakers], per speaker the first warp
    of smallest cost; `fallback` for fewer than min_frames frames, a smallest cost that is not finite, or a NaN among the costs"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.uint64)
    assert cost.ndim == 2 and len(frames) == cost.shape[0]
    out = np.zeros(max(cost.shape[0], 1), dtype=np.uint32)
    _check(lib().sr_vtln_choose(cost.shape[0], cost.shape[1], _ptr(cost), _ptr(frames), int(min_frames), int(fallback), _ptr(out)))
    return out[:cost.shape[0]]


def shard_utterances(frame_off, n_shards):
    """sr_shard_utterances: greedy LPT deal by frames -> (shard_of_utt u32[n_utts], shard_frames u64[n_shards])."""
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    n = len(frame_off) - 1
    shard = np.zeros(max(n, 1), dtype=np.uint32)
    load = np.zeros(n_shards, dtype=np.uint64)
    _check(lib().sr_shard_utterances(_ptr(frame_off), n, n_shards, _ptr(shard), _ptr(load)))
    return shard[:n], load


def recognize_batch_multi(models, lexica, feats, frame_off, am_threshold, word_penalty, kernel=GMM_PREFILTER):
    """sr_recognize_batch_multi over (model, lexicon) replicas, one host thread each -> (words, word_off, shard_frames)."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    n, nd = len(frame_off) - 1, len(models)
    mh = (C.c_void_p * nd)(*[m.h for m in models])
    lh = (C.c_void_p * nd)(*[l.h for l in lexica])
    words = np.zeros(max(int(frame_off[-1]), 1), dtype=np.uint32)
    woff = np.zeros(n + 1, dtype=np.uint64)
    load = np.zeros(nd, dtype=np.uint64)
    sp = SearchParams(am_threshold, word_penalty, kernel, 0)
    _check(lib().sr_recognize_batch_multi(mh, lh, nd, C.byref(sp), _ptr(feats), _ptr(frame_off), n, _ptr(words), _ptr(woff), _ptr(load)))
    return words[: int(woff[-1])].copy(), woff, load
