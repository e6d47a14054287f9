"""Python mirror of the reference's pipeline interface over the C ABI.

The reference (szuwgh/whisper.rs, src/main.rs) exposes

    WhisperContext::new(fname) -> WsResult<WhisperContext>          main.rs:366
    whisper_pcm_to_mel(&mut ctx, samples: Arc<Vec<f32>>)            main.rs:1681
    whisper_encode(&mut ctx, n_threads, mel_offset)                 main.rs:1799
    convert_integer_to_float_audio(&[i16]) -> Vec<f32>              main.rs:1673
    WsError (BadMagic, UnknownTensor, WrongSizeTensor, ...)         main.rs:51-72

This module keeps those names, argument meanings and error behaviour, and
binds them with ctypes to libwhisper_mi355x.so (include/whisper_mi355x.h),
whose work runs in hand-written gfx950 kernels.  There is no CPU fallback:
if the shared library or a HIP device is missing, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WMI_LIB") or os.path.join(HERE, "libwhisper_mi355x.so")

WMI_OK = 0


class WsError(RuntimeError):
    """WsError (main.rs:51-72); `code` is the wmi_status value."""
    code = -1

    def __init__(self, msg: str = "", code: int | None = None):
        super().__init__(msg)
        if code is not None:
            self.code = code


class UnexpectIO(WsError): code = 1
class BadMagic(WsError): code = 2
class NotEnoughSpace(WsError): code = 3
class UnknownTensor(WsError): code = 4
class BadRefTensor(WsError): code = 5
class WrongSizeTensor(WsError): code = 6
class WrongShapeTensor(WsError): code = 7
class WrongBytesTensor(WsError): code = 8
class WrongGTensor(WsError): code = 9
class Unexpected(WsError): code = 10
class HipError(WsError): code = 11
class RcclError(WsError): code = 12
class Unsupported(WsError): code = 13
class InvalidArgument(WsError): code = 14


_ERRORS = {c.code: c for c in (UnexpectIO, BadMagic, NotEnoughSpace, UnknownTensor, BadRefTensor, WrongSizeTensor,
                               WrongShapeTensor, WrongBytesTensor, WrongGTensor, Unexpected, HipError, RcclError,
                               Unsupported, InvalidArgument)}

# exported symbols of include/whisper_mi355x.h
EXPORTS = (
    "wmi_init_from_file", "wmi_free", "wmi_strerror", "wmi_last_error", "wmi_last_error_global",
    "wmi_get_hparams", "wmi_get_special_tokens", "wmi_set_audio_ctx", "wmi_token_to_bytes",
    "wmi_read_wav", "wmi_pcm16_to_f32", "wmi_tokens_to_text",
    "wmi_lang_index", "wmi_lang_code", "wmi_lang_count", "wmi_set_language", "wmi_set_task", "wmi_detect_language",
    "wmi_get_language",
    "wmi_decode_timestamps", "wmi_transcribe", "wmi_get_segment", "wmi_get_segment_tokens",
    "wmi_set_no_context", "wmi_decode_timestamps_batch", "wmi_transcribe_batch", "wmi_get_segment_of",
    "wmi_get_segment_tokens_of", "wmi_set_batch_context", "wmi_decode_timestamps_rows",
    "wmi_decode_timestamps_beam", "wmi_set_beam_size",
    "wmi_set_fallback", "wmi_decode_timestamps_sampled", "wmi_get_window_count", "wmi_get_window_info",
    "wmi_set_decode_rules", "wmi_non_speech_tokens", "wmi_decode_timestamps_ruled", "wmi_set_initial_prompt",
    "wmi_set_rules_beam", "wmi_decode_timestamps_ruled_beam",
    "wmi_set_best_of", "wmi_decode_timestamps_best_of", "wmi_best_of_key", "wmi_get_window_candidate",
    "wmi_is_non_speech_token", "wmi_set_token_timestamps", "wmi_token_times",
    "wmi_set_dtw", "wmi_align_tokens", "wmi_dtw_path", "wmi_dtw_path_host", "wmi_get_segment_dtw_of",
    "wmi_audio_to_mel_batch", "wmi_stage_audio", "wmi_transcribe_audio", "wmi_transcribe_audio_batch", "wmi_get_pcm",
    "wmi_get_audio_timing", "wmi_resample_plan", "wmi_resample_taps", "wmi_resampled_length",
    "wmi_set_chunking", "wmi_set_chunk_spans", "wmi_get_chunk_count", "wmi_get_chunk", "wmi_plan_chunks",
    "wmi_plan_chunks_host",
    "wmi_pcm_to_mel", "wmi_pcm_to_mel_batch", "wmi_encode", "wmi_decode_greedy", "wmi_decode_logits",
    "wmi_decode_beam", "wmi_full", "wmi_stage_pcm", "wmi_run_staged", "wmi_run_staged_beam", "wmi_get_tokens", "wmi_get_timings", "wmi_sync",
    "wmi_get_mel", "wmi_get_checksums", "wmi_get_encoder_out", "wmi_get_cross_kv", "wmi_bench_kernel", "wmi_decode_alg_bytes",
    "wmi_selftest", "wmi_debug_read",
    "wmi_dist_id_size", "wmi_dist_make_id", "wmi_dist_init", "wmi_dist_gather_tokens", "wmi_dist_barrier",
)


class Hparams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                         "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_mels", "f16")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SpecialTokens(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("eot", "sot", "prev", "solm", "not_", "beg", "translate", "transcribe",
                                         "is_multilingual")]


class KernelBench(C.Structure):
    _fields_ = [("avg_us", C.c_float), ("alg_bytes", C.c_double), ("alg_flops", C.c_double),
                ("name", C.c_char * 48)]


class TokenData(C.Structure):
    """WhisperTokenData (main.rs:317-331)."""
    _fields_ = [("id", C.c_int32), ("tid", C.c_int32), ("p", C.c_float), ("pt", C.c_float), ("ptsum", C.c_float),
                ("t0", C.c_int64), ("t1", C.c_int64), ("vlen", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FallbackParams(C.Structure):
    """wmi_fallback_params."""
    _fields_ = [("temperature", C.c_float), ("temperature_inc", C.c_float), ("logprob_thold", C.c_float),
                ("entropy_thold", C.c_float), ("no_speech_thold", C.c_float), ("seed", C.c_uint64)]


class DecodeRules(C.Structure):
    """wmi_decode_rules."""
    _fields_ = [("enable", C.c_int32), ("max_initial_ts", C.c_int32), ("suppress_non_speech", C.c_int32),
                ("suppress", C.c_void_p), ("n_suppress", C.c_int32)]


class TokenTsParams(C.Structure):
    """wmi_token_ts_params."""
    _fields_ = [("enable", C.c_int32), ("thold_pt", C.c_float), ("thold_ptsum", C.c_float), ("max_len", C.c_int32),
                ("split_on_word", C.c_int32)]


class DtwParams(C.Structure):
    """wmi_dtw_params."""
    _fields_ = [("enable", C.c_int32), ("n_top", C.c_int32), ("heads", C.c_void_p), ("n_heads", C.c_int32),
                ("medfilt_width", C.c_int32)]


class DtwTime(C.Structure):
    """wmi_dtw_time."""
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64)]


class WindowInfo(C.Structure):
    """wmi_window_info; flags: 1 silence, 2 failed, 4 every attempt rejected, 8 context reset."""
    _fields_ = [("seek", C.c_int64), ("n_attempts", C.c_int32), ("temperature", C.c_float),
                ("avg_logprob", C.c_float), ("entropy", C.c_float), ("no_speech_prob", C.c_float),
                ("flags", C.c_int32), ("first_segment", C.c_int32), ("n_segments", C.c_int32)]


class ChunkParams(C.Structure):
    """wmi_chunk_params."""
    _fields_ = [("enable", C.c_int32), ("max_frames", C.c_int32), ("min_frames", C.c_int32),
                ("smooth_frames", C.c_int32)]


class ChunkInfo(C.Structure):
    """wmi_chunk_info."""
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("first_segment", C.c_int32), ("n_segments", C.c_int32),
                ("first_window", C.c_int32), ("n_windows", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Audio(C.Structure):
    """wmi_audio: raw interleaved frames of one clip (sample_type 0 = f32, 1 = s16)."""
    _fields_ = [("data", C.c_void_p), ("n_frames", C.c_size_t), ("sample_rate", C.c_int32), ("channels", C.c_int32),
                ("sample_type", C.c_int32)]


class Timings(C.Structure):
    _fields_ = [("mel_ms", C.c_float), ("encode_ms", C.c_float), ("cross_kv_ms", C.c_float),
                ("decode_ms", C.c_float), ("n_decode_steps", C.c_int32)]


_lib = None


def lib():
    """Load the HIP library (fails loudly: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not built: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
        L.wmi_init_from_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.wmi_free.argtypes = [vp]
        L.wmi_free.restype = None
        L.wmi_strerror.restype = C.c_char_p
        L.wmi_last_error.argtypes = [vp]
        L.wmi_last_error.restype = C.c_char_p
        L.wmi_last_error_global.restype = C.c_char_p
        L.wmi_get_hparams.argtypes = [vp, C.POINTER(Hparams)]
        L.wmi_get_special_tokens.argtypes = [vp, C.POINTER(SpecialTokens)]
        L.wmi_set_audio_ctx.argtypes = [vp, C.c_int]
        L.wmi_token_to_bytes.argtypes = [vp, i32, C.c_char_p, sz, C.POINTER(sz)]
        L.wmi_read_wav.argtypes = [C.c_char_p, vp, sz, C.POINTER(sz), C.POINTER(i32), C.POINTER(i32)]
        L.wmi_pcm16_to_f32.argtypes = [vp, sz, vp]
        L.wmi_tokens_to_text.argtypes = [vp, vp, C.c_int, C.c_char_p, sz, C.POINTER(sz)]
        L.wmi_lang_index.argtypes = [C.c_char_p, C.POINTER(i32)]
        L.wmi_lang_code.argtypes = [C.c_int]
        L.wmi_lang_code.restype = C.c_char_p
        L.wmi_lang_count.argtypes = [vp, C.POINTER(i32)]
        L.wmi_set_language.argtypes = [vp, C.c_int, C.c_int]
        L.wmi_set_task.argtypes = [vp, C.c_int]
        L.wmi_detect_language.argtypes = [vp, vp, vp]
        L.wmi_get_language.argtypes = [vp, C.c_int, C.POINTER(i32), C.POINTER(C.c_float)]
        L.wmi_decode_timestamps.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(i32)]
        L.wmi_transcribe.argtypes = [vp, vp, sz, C.c_int, C.POINTER(i32)]
        L.wmi_get_segment.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, sz,
                                      C.POINTER(sz)]
        L.wmi_get_segment_tokens.argtypes = [vp, C.c_int, vp, sz, C.POINTER(i32)]
        L.wmi_set_no_context.argtypes = [vp, C.c_int]
        if hasattr(L, "wmi_set_batch_context"):  # (as below: an older build has no text context in the batch)
            L.wmi_set_batch_context.argtypes = [vp, C.c_int]
            L.wmi_decode_timestamps_rows.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
        L.wmi_decode_timestamps_beam.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(i32),
                                                 C.POINTER(C.c_double)]
        L.wmi_set_beam_size.argtypes = [vp, C.c_int]
        L.wmi_set_fallback.argtypes = [vp, C.POINTER(FallbackParams)]
        L.wmi_decode_timestamps_sampled.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, vp,
                                                    C.POINTER(i32), vp, C.POINTER(C.c_float)]
        # (an older build selected with WMI_LIB for an A/B run, scripts/lib_equal.py, has no decoding rules;
        # calling them on it raises AttributeError)
        if hasattr(L, "wmi_set_decode_rules"):
            L.wmi_set_decode_rules.argtypes = [vp, C.POINTER(DecodeRules)]
            L.wmi_non_speech_tokens.argtypes = [vp, vp, sz, C.POINTER(i32)]
            L.wmi_decode_timestamps_ruled.argtypes = L.wmi_decode_timestamps_sampled.argtypes
            L.wmi_set_initial_prompt.argtypes = [vp, vp, C.c_int]
            L.wmi_is_non_speech_token.argtypes = [C.c_char_p, sz]
        if hasattr(L, "wmi_set_rules_beam"):  # (as above: an older build has no ruled beam window)
            L.wmi_set_rules_beam.argtypes = [vp, C.c_int]
            L.wmi_decode_timestamps_ruled_beam.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(i32),
                                                           C.POINTER(C.c_double), C.POINTER(C.c_float)]
        if hasattr(L, "wmi_set_best_of"):  # (as above: an older build has no best-of windows)
            L.wmi_set_best_of.argtypes = [vp, C.c_int]
            L.wmi_decode_timestamps_best_of.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                                        vp, C.POINTER(i32), vp, C.POINTER(C.c_float), C.POINTER(i32), vp, vp]
            L.wmi_best_of_key.argtypes = [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
            L.wmi_get_window_candidate.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32)]
        if hasattr(L, "wmi_set_token_timestamps"):  # (as above: an older build has no token-level timestamps)
            L.wmi_set_token_timestamps.argtypes = [vp, C.POINTER(TokenTsParams)]
            L.wmi_token_times.argtypes = [vp, vp, sz, C.c_int64, C.c_int64, C.c_int64, vp, C.c_int]
        if hasattr(L, "wmi_stage_audio"):  # (as above: an older build has no audio front end)
            L.wmi_audio_to_mel_batch.argtypes = [vp, C.c_int, C.POINTER(Audio)]
            L.wmi_stage_audio.argtypes = [vp, C.c_int, C.POINTER(Audio)]
            L.wmi_transcribe_audio.argtypes = [vp, C.POINTER(Audio), C.c_int, C.POINTER(i32)]
            L.wmi_transcribe_audio_batch.argtypes = [vp, C.c_int, C.POINTER(Audio), C.c_int, vp]
            L.wmi_get_pcm.argtypes = [vp, C.c_int, vp, sz, C.POINTER(sz)]
            L.wmi_get_audio_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i32)]
            L.wmi_resample_plan.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
            L.wmi_resample_taps.argtypes = [i32, vp, sz, C.POINTER(sz)]
            L.wmi_resampled_length.argtypes = [i32, sz, C.POINTER(sz)]
        if hasattr(L, "wmi_set_dtw"):  # (as above: an older build has no alignment)
            L.wmi_set_dtw.argtypes = [vp, C.POINTER(DtwParams)]
            L.wmi_align_tokens.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp]
            L.wmi_dtw_path.argtypes = [vp, vp, C.c_int, C.c_int, vp]
            L.wmi_dtw_path_host.argtypes = [vp, C.c_int, C.c_int, vp]
            L.wmi_get_segment_dtw_of.argtypes = [vp, C.c_int, C.c_int, vp, sz, C.POINTER(i32)]
        if hasattr(L, "wmi_set_chunking"):  # (as above: an older build has no chunking)
            L.wmi_set_chunking.argtypes = [vp, C.POINTER(ChunkParams)]
            L.wmi_set_chunk_spans.argtypes = [vp, C.c_int, vp, C.c_int]
            L.wmi_get_chunk_count.argtypes = [vp, C.c_int, C.POINTER(i32)]
            L.wmi_get_chunk.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ChunkInfo)]
            L.wmi_plan_chunks.argtypes = [vp, C.c_int, vp, sz, C.POINTER(i32)]
            L.wmi_plan_chunks_host.argtypes = [vp, sz, C.POINTER(ChunkParams), C.c_int, vp, sz, C.POINTER(i32)]
        L.wmi_get_window_count.argtypes = [vp, C.c_int, C.POINTER(i32)]
        L.wmi_get_window_info.argtypes = [vp, C.c_int, C.c_int, C.POINTER(WindowInfo)]
        L.wmi_decode_timestamps_batch.argtypes =[vp, vp, C.c_int, C.c_int, vp, vp]
        L.wmi_transcribe_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_int, vp]
        L.wmi_get_segment_of.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p,
                                         sz, C.POINTER(sz)]
        L.wmi_get_segment_tokens_of.argtypes = [vp, C.c_int, C.c_int, vp, sz, C.POINTER(i32)]
        L.wmi_pcm_to_mel.argtypes = [vp, vp, sz]
        L.wmi_pcm_to_mel_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.wmi_stage_pcm.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.wmi_encode.argtypes = [vp, C.c_int, C.c_int]
        L.wmi_decode_greedy.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        L.wmi_decode_logits.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        L.wmi_full.argtypes = [vp, vp, sz, C.c_int, vp, vp]
        L.wmi_run_staged.argtypes = [vp, C.c_int, C.c_int]
        L.wmi_run_staged_beam.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.wmi_decode_beam.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        L.wmi_get_tokens.argtypes = [vp, vp, sz, vp]
        L.wmi_get_timings.argtypes = [vp, C.POINTER(Timings)]
        L.wmi_sync.argtypes = [vp]
        L.wmi_get_mel.argtypes = [vp, C.c_int, vp, sz, C.POINTER(i32), C.POINTER(i32)]
        L.wmi_get_encoder_out.argtypes = [vp, C.c_int, vp, sz]
        L.wmi_get_cross_kv.argtypes = [vp, C.c_int, vp, vp, sz]
        L.wmi_bench_kernel.argtypes = [vp, C.c_int, C.c_int, C.POINTER(KernelBench)]
        L.wmi_decode_alg_bytes.argtypes = [C.POINTER(Hparams), C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.wmi_selftest.argtypes = [vp, C.POINTER(i32)]
        L.wmi_debug_read.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.wmi_get_checksums.argtypes = [vp, vp]
        L.wmi_dist_id_size.restype = sz
        L.wmi_dist_make_id.argtypes = [vp]
        L.wmi_dist_init.argtypes = [vp, C.c_int, C.c_int, vp]
        L.wmi_dist_gather_tokens.argtypes = [vp, vp, sz]
        L.wmi_dist_barrier.argtypes = [vp]
        _lib = L
    return _lib


def _raise(rc: int, ctx=None):
    if rc == WMI_OK:
        return
    L = lib()
    msg = (L.wmi_last_error(ctx) if ctx else L.wmi_last_error_global()) or b""
    cls = _ERRORS.get(rc, WsError)
    raise cls(f"{L.wmi_strerror(rc).decode()}: {msg.decode(errors='replace')}", rc)


def is_non_speech_token(tok: bytes) -> bool:
    """Whether the bytes are a token set_decode_rules(suppress_non_speech=True) masks
    (wmi_is_non_speech_token: host-only, no device)."""
    return lib().wmi_is_non_speech_token(tok, len(tok)) == 1


def decode_alg_bytes(hp: dict, rows: int, steps: int, beam: bool = False, q5: bool = False):
    """(bytes, flops) of one decode (wmi_decode_alg_bytes: host-only, no device)."""
    h = Hparams(**{n: int(hp.get(n, 1)) for n, _ in Hparams._fields_})
    b, f = C.c_double(), C.c_double()
    _raise(lib().wmi_decode_alg_bytes(C.byref(h), rows, steps, int(bool(beam)), int(bool(q5)), C.byref(b),
                                      C.byref(f)))
    return b.value, f.value


LANG_AUTO = -1
TASKS = {"transcribe": 0, "translate": 1}


def lang_index(code: str) -> int:
    """Index of a language code ("en" = 0 ... "yue" = 99); the language token
    is sot + 1 + index.  Raises InvalidArgument on an unknown code."""
    i = C.c_int32()
    _raise(lib().wmi_lang_index(code.encode(), C.byref(i)))
    return i.value


def lang_code(index: int):
    """Code of a language index, or None outside [0, 100)."""
    c = lib().wmi_lang_code(int(index))
    return None if c is None else c.decode()


def convert_integer_to_float_audio(samples) -> np.ndarray:
    """main.rs:1673-1679: s16 -> f32 / 32768.0."""
    return (np.asarray(samples, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def read_wav(path: str):
    """hound::WavReader::open + samples::<i16>() (main.rs:2067-2068) through
    the C ABI: (int16 samples interleaved, sample_rate, channels)."""
    L = lib()
    n, sr, ch = C.c_size_t(), C.c_int32(), C.c_int32()
    _raise(L.wmi_read_wav(os.fsencode(path), None, 0, C.byref(n), C.byref(sr), C.byref(ch)))
    out = np.zeros(n.value, np.int16)
    _raise(L.wmi_read_wav(os.fsencode(path), _ptr(out), out.size, C.byref(n), C.byref(sr), C.byref(ch)))
    return out, sr.value, ch.value


def pcm16_to_f32(s16) -> np.ndarray:
    """convert_integer_to_float_audio (main.rs:1673-1679) through the C ABI."""
    s16 = np.ascontiguousarray(s16, dtype=np.int16)
    out = np.zeros(s16.size, np.float32)
    _raise(lib().wmi_pcm16_to_f32(_ptr(s16), s16.size, _ptr(out)))
    return out


def resample_plan(sample_rate: int):
    """(L, M, K) of the resampler from sample_rate to 16 kHz (wmi_resample_plan:
    host-only, no device).  Raises Unsupported for a rate outside the plan."""
    l, m, k = C.c_int32(), C.c_int32(), C.c_int32()
    _raise(lib().wmi_resample_plan(int(sample_rate), C.byref(l), C.byref(m), C.byref(k)))
    return l.value, m.value, k.value


def resample_taps(sample_rate: int) -> np.ndarray:
    """The resampler's taps [L][2K] f32 (wmi_resample_taps: host-only, no device)."""
    l, _, k = resample_plan(sample_rate)
    h = np.zeros((l, 2 * k), np.float32)
    n = C.c_size_t()
    _raise(lib().wmi_resample_taps(int(sample_rate), _ptr(h), h.size, C.byref(n)))
    return h


def resampled_length(sample_rate: int, n_frames: int) -> int:
    """16 kHz samples that n_frames frames at sample_rate give (wmi_resampled_length)."""
    n = C.c_size_t()
    _raise(lib().wmi_resampled_length(int(sample_rate), int(n_frames), C.byref(n)))
    return n.value


def _audio(clips):
    """The wmi_audio array of clips, each (samples, rate): samples an ndarray
    [frames] or [frames, channels] of int16 or float32, C-contiguous (or an
    Audio already filled in); returns (array, the ndarrays kept alive)."""
    arr = (Audio * max(1, len(clips)))()
    keep = []
    for i, clip in enumerate(clips):
        if isinstance(clip, Audio):
            arr[i] = clip
            continue
        a, rate = clip
        if not isinstance(a, np.ndarray) or a.dtype not in (np.int16, np.float32) or a.ndim not in (1, 2) \
                or not a.flags["C_CONTIGUOUS"]:
            raise InvalidArgument("a clip is a C-contiguous int16 or float32 ndarray [frames] or [frames, channels]", 14)
        keep.append(a)
        arr[i] = Audio(a.ctypes.data, a.shape[0], int(rate), 1 if a.ndim == 1 else a.shape[1],
                       1 if a.dtype == np.int16 else 0)
    return arr, keep


class WhisperContext:
    """WhisperContext (main.rs:333-363), device-resident."""

    def __init__(self, handle, device: int, max_clips: int):
        self._h = handle
        self.device = device
        self.max_clips = max_clips
        hp = Hparams()
        _raise(lib().wmi_get_hparams(self._h, C.byref(hp)), self._h)
        self.hparams = hp.as_dict()
        sp = SpecialTokens()
        _raise(lib().wmi_get_special_tokens(self._h, C.byref(sp)), self._h)
        self.special = {"eot": sp.eot, "sot": sp.sot, "prev": sp.prev, "solm": sp.solm, "not": sp.not_,
                        "beg": sp.beg, "translate": sp.translate, "transcribe": sp.transcribe,
                        "multilingual": sp.is_multilingual}
        self.n_clips = 0
        self.n_ctx = self.hparams["n_audio_ctx"]

    @classmethod
    def new(cls, fname: str, device: int = 0, max_clips: int = 1) -> "WhisperContext":
        """WhisperContext::new (main.rs:366-503); raises the WsError variant."""
        h = C.c_void_p()
        rc = lib().wmi_init_from_file(os.fsencode(fname), device, max_clips, C.byref(h))
        _raise(rc)
        return cls(h, device, max_clips)

    def close(self):
        if getattr(self, "_h", None):
            lib().wmi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # --- knobs -------------------------------------------------------------
    def set_audio_ctx(self, n: int) -> None:
        """exp_n_audio_ctx (main.rs:362, 1803-1807); 0 restores n_audio_ctx."""
        _raise(lib().wmi_set_audio_ctx(self._h, n), self._h)
        self.n_ctx = n or self.hparams["n_audio_ctx"]

    # --- language and task ---------------------------------------------------
    def n_lang(self) -> int:
        """Languages of the model: 0 (.en), 99, or 100 (large-v3)."""
        n = C.c_int32()
        _raise(lib().wmi_lang_count(self._h, C.byref(n)), self._h)
        return n.value

    def set_language(self, lang, clip: int = -1) -> None:
        """lang: a code ("de"), an index, or None = detect per clip at decode
        time (WMI_LANG_AUTO); clip -1 = every clip.  Holds until changed."""
        if lang is None:
            lang = LANG_AUTO
        elif isinstance(lang, str):
            lang = lang_index(lang)
        _raise(lib().wmi_set_language(self._h, clip, int(lang)), self._h)

    def set_task(self, task) -> None:
        """"transcribe" (default) or "translate"."""
        _raise(lib().wmi_set_task(self._h, TASKS[task] if isinstance(task, str) else int(task)), self._h)

    def detect_language(self):
        """(ids [n_clips], probs [n_clips][n_lang]) of the encoded clips."""
        ids = np.zeros(self.n_clips, np.int32)
        probs = np.zeros((self.n_clips, self.n_lang()), np.float32)
        _raise(lib().wmi_detect_language(self._h, _ptr(ids), _ptr(probs)), self._h)
        return ids, probs

    def language(self, clip: int = 0):
        """(index, p) the last decode / transcribe used for clip; p is the
        detection probability, or -1 if the language was set explicitly."""
        i, p = C.c_int32(), C.c_float()
        _raise(lib().wmi_get_language(self._h, clip, C.byref(i), C.byref(p)), self._h)
        return i.value, p.value

    def token_to_str(self, tid: int) -> bytes:
        """id_to_token (main.rs:578-592, 442-467)."""
        n = C.c_size_t()
        buf = C.create_string_buffer(512)
        _raise(lib().wmi_token_to_bytes(self._h, tid, buf, 512, C.byref(n)), self._h)
        return buf.raw[:n.value]

    def tokens_to_text(self, ids) -> bytes:
        """Text bytes of the text tokens of ids (specials / timestamps skipped)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = C.c_size_t()
        rc = lib().wmi_tokens_to_text(self._h, _ptr(ids), ids.size, None, 0, C.byref(n))
        if rc not in (WMI_OK, NotEnoughSpace.code):
            _raise(rc, self._h)
        buf = C.create_string_buffer(max(1, n.value))
        _raise(lib().wmi_tokens_to_text(self._h, _ptr(ids), ids.size, buf, n.value, C.byref(n)), self._h)
        return buf.raw[:n.value]

    # --- timestamps / segments (whisper.cpp-1.0.3 whisper_full) ----------
    def decode_timestamps(self, prompt, max_tokens: int):
        """One timestamp-decoding window of encoded clip 0: [WhisperTokenData dict]."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max_tokens)()
        n = C.c_int32()
        _raise(lib().wmi_decode_timestamps(self._h, _ptr(prompt), prompt.size, max_tokens, out, C.byref(n)), self._h)
        return [out[i].as_dict() for i in range(n.value)]

    def transcribe(self, pcm, max_tokens: int = 220):
        """whisper_full with timestamps: [{"t0", "t1", "text", "tokens"}] (t in 10 ms)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        ns = C.c_int32()
        _raise(lib().wmi_transcribe(self._h, _ptr(pcm), pcm.size, max_tokens, C.byref(ns)), self._h)
        self.n_clips = 1
        segs = []
        for i in range(ns.value):
            t0, t1, ln = C.c_int64(), C.c_int64(), C.c_size_t()
            lib().wmi_get_segment(self._h, i, C.byref(t0), C.byref(t1), None, 0, C.byref(ln))
            buf = C.create_string_buffer(max(1, ln.value))
            _raise(lib().wmi_get_segment(self._h, i, C.byref(t0), C.byref(t1), buf, ln.value, C.byref(ln)), self._h)
            nt = C.c_int32()
            lib().wmi_get_segment_tokens(self._h, i, None, 0, C.byref(nt))
            toks = (TokenData * max(1, nt.value))()
            _raise(lib().wmi_get_segment_tokens(self._h, i, toks, nt.value, C.byref(nt)), self._h)
            segs.append({"t0": t0.value, "t1": t1.value, "text": buf.raw[:ln.value],
                         "tokens": [toks[k].as_dict() for k in range(nt.value)]})
        return segs

    def set_no_context(self, on: bool = True) -> None:
        """Windows of transcribe() decode without the earlier windows' text
        (whisper.cpp no_context); transcribe_batch() does so unless
        set_batch_context(1) is on, and then follows this setting."""
        _raise(lib().wmi_set_no_context(self._h, int(bool(on))), self._h)

    def decode_timestamps_beam(self, beam_size: int, prompt, max_tokens: int):
        """decode_timestamps() with beam search over beam_size (1..8)
        hypotheses under the timestamp rule: ([WhisperTokenData dict] of the
        chosen hypothesis, its summed log-probability)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max(1, max_tokens))()
        n = C.c_int32()
        sc = C.c_double()
        _raise(lib().wmi_decode_timestamps_beam(self._h, beam_size, _ptr(prompt), prompt.size, max_tokens, out,
                                                C.byref(n), C.byref(sc)), self._h)
        return [out[i].as_dict() for i in range(n.value)], sc.value

    def set_beam_size(self, k: int) -> None:
        """Hypotheses of every transcribe() window (1..8; 1, the default, is
        the greedy sampler).  transcribe_batch() refuses a size above 1."""
        _raise(lib().wmi_set_beam_size(self._h, int(k)), self._h)

    def decode_timestamps_batch(self, prompt, max_tokens: int):
        """One timestamp window of every encoded clip after the shared prompt,
        up to 8 clips per decoder step: per clip [WhisperTokenData dict]."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * (max(1, self.n_clips) * max_tokens))()
        n = np.zeros(max(1, self.n_clips), np.int32)
        _raise(lib().wmi_decode_timestamps_batch(self._h, _ptr(prompt), prompt.size, max_tokens, out, _ptr(n)),
               self._h)
        return [[out[c * max_tokens + i].as_dict() for i in range(n[c])] for c in range(self.n_clips)]

    def set_batch_context(self, enable=1) -> None:
        """1: transcribe_batch() gives every recording its own text context, as
        transcribe() does (rows of unequal prompt length are right-aligned
        under the decoder's one step position); 0, the default: every window
        without earlier text.  Neither: InvalidArgument."""
        _raise(lib().wmi_set_batch_context(self._h, int(enable)), self._h)

    def decode_timestamps_rows(self, prompts, max_tokens: int):
        """decode_timestamps_batch() with a prompt per encoded clip (a list of
        id sequences of any lengths): per clip [WhisperTokenData dict]."""
        rows = [np.ascontiguousarray(p, dtype=np.int32).ravel() for p in prompts]
        lens = np.array([r.size for r in rows], np.int32)
        stride = max(1, int(lens.max()) if len(rows) else 1)
        flat = np.zeros((max(1, len(rows)), stride), np.int32)
        for b, r in enumerate(rows):
            flat[b, :r.size] = r
        out = (TokenData * (max(1, self.n_clips) * max_tokens))()
        n = np.zeros(max(1, self.n_clips), np.int32)
        if len(rows) != self.n_clips:
            raise ValueError(f"{len(rows)} prompts for {self.n_clips} clips")
        _raise(lib().wmi_decode_timestamps_rows(self._h, _ptr(flat), _ptr(lens), stride, max_tokens, out, _ptr(n)),
               self._h)
        return [[out[c * max_tokens + i].as_dict() for i in range(n[c])] for c in range(self.n_clips)]

    def segments_of(self, clip: int, n_segments: int):
        """Segments of recording `clip` of the last transcribe_batch."""
        segs = []
        for i in range(n_segments):
            t0, t1, ln = C.c_int64(), C.c_int64(), C.c_size_t()
            lib().wmi_get_segment_of(self._h, clip, i, C.byref(t0), C.byref(t1), None, 0, C.byref(ln))
            buf = C.create_string_buffer(max(1, ln.value))
            _raise(lib().wmi_get_segment_of(self._h, clip, i, C.byref(t0), C.byref(t1), buf, ln.value, C.byref(ln)),
                   self._h)
            nt = C.c_int32()
            lib().wmi_get_segment_tokens_of(self._h, clip, i, None, 0, C.byref(nt))
            toks = (TokenData * max(1, nt.value))()
            _raise(lib().wmi_get_segment_tokens_of(self._h, clip, i, toks, nt.value, C.byref(nt)), self._h)
            segs.append({"t0": t0.value, "t1": t1.value, "text": buf.raw[:ln.value],
                         "tokens": [toks[k].as_dict() for k in range(nt.value)]})
        return segs

    def transcribe_batch(self, clips, max_tokens: int = 220):
        """transcribe() of several recordings (any lengths, at most max_clips)
        with up to 8 of them per decoder step, every window without earlier
        text (or, under set_batch_context(1), each recording with its own):
        per recording the list transcribe() returns."""
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        ptrs = (C.c_void_p * max(1, len(clips)))(*[c.ctypes.data for c in clips])
        ns = (C.c_size_t * max(1, len(clips)))(*[c.size for c in clips])
        nseg = np.zeros(max(1, len(clips)), np.int32)
        _raise(lib().wmi_transcribe_batch(self._h, len(clips), ptrs, ns, max_tokens, _ptr(nseg)), self._h)
        self.n_clips = len(clips)
        return [self.segments_of(c, int(nseg[c])) for c in range(len(clips))]

    # --- temperature fallback ---------------------------------------------
    def set_fallback(self, temperature: float = 0.0, temperature_inc: float = 0.0, logprob_thold: float = -np.inf,
                     entropy_thold: float = -np.inf, no_speech_thold: float = np.inf, seed: int = 0,
                     default: bool = False) -> None:
        """Temperature fallback, quality thresholds and the no-speech skip of
        transcribe() / transcribe_batch() (wmi_set_fallback); the defaults
        (or default=True: a NULL parameter block) switch it off."""
        if default:
            _raise(lib().wmi_set_fallback(self._h, None), self._h)
            return
        p = FallbackParams(temperature, temperature_inc, logprob_thold, entropy_thold, no_speech_thold,
                           int(seed) & 0xFFFFFFFFFFFFFFFF)
        _raise(lib().wmi_set_fallback(self._h, C.byref(p)), self._h)

    def decode_timestamps_sampled(self, prompt, max_tokens: int, temperature: float, seed: int = 0, n: int = 0):
        """One window of encoded clip 0 at one temperature, as attempt ordinal
        n of `seed`: ([WhisperTokenData dict], plog float32 [tokens], p_nosp)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max(1, max_tokens))()
        cnt = C.c_int32()
        plog = np.zeros(max(1, max_tokens), np.float32)
        pn = C.c_float()
        _raise(lib().wmi_decode_timestamps_sampled(self._h, _ptr(prompt), prompt.size, max_tokens, temperature,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, n, out, C.byref(cnt), _ptr(plog),
                                                   C.byref(pn)), self._h)
        return [out[i].as_dict() for i in range(cnt.value)], plog[:cnt.value].copy(), pn.value

    # --- OpenAI decoding rules and the initial prompt -----------------------
    def set_decode_rules(self, enable: bool = True, max_initial_ts: int = -1, suppress_non_speech: bool = False,
                         suppress=(), default: bool = False) -> None:
        """OpenAI's SuppressTokens / ApplyTimestampRules for transcribe(),
        transcribe_batch() and decode_timestamps_ruled() (wmi_set_decode_rules);
        enable=False (or default=True: a NULL parameter block) switches them off."""
        if default:
            _raise(lib().wmi_set_decode_rules(self._h, None), self._h)
            return
        ids = np.ascontiguousarray(suppress, dtype=np.int32)
        p = DecodeRules(int(bool(enable)), int(max_initial_ts), int(bool(suppress_non_speech)),
                        ids.ctypes.data if ids.size else None, ids.size)
        _raise(lib().wmi_set_decode_rules(self._h, C.byref(p)), self._h)

    def non_speech_tokens(self):
        """The ids set_decode_rules(suppress_non_speech=True) adds (wmi_non_speech_tokens)."""
        n = C.c_int32()
        rc = lib().wmi_non_speech_tokens(self._h, None, 0, C.byref(n))
        if rc != NotEnoughSpace.code:
            _raise(rc, self._h)
        ids = np.zeros(max(1, n.value), np.int32)
        if n.value:
            _raise(lib().wmi_non_speech_tokens(self._h, _ptr(ids), n.value, C.byref(n)), self._h)
        return ids[:n.value].tolist()

    def decode_timestamps_ruled(self, prompt, max_tokens: int, temperature: float = 0.0, seed: int = 0, n: int = 0):
        """decode_timestamps_sampled under the rules set."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max(1, max_tokens))()
        cnt = C.c_int32()
        plog = np.zeros(max(1, max_tokens), np.float32)
        pn = C.c_float()
        _raise(lib().wmi_decode_timestamps_ruled(self._h, _ptr(prompt), prompt.size, max_tokens, temperature,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, n, out, C.byref(cnt), _ptr(plog),
                                                 C.byref(pn)), self._h)
        return [out[i].as_dict() for i in range(cnt.value)], plog[:cnt.value].copy(), pn.value

    # --- best-of-N sampled attempts --------------------------------------------
    def set_best_of(self, best_of: int) -> None:
        """Candidates of every T > 0 attempt of transcribe() under set_fallback
        (wmi_set_best_of; 1, the default: the single draw)."""
        _raise(lib().wmi_set_best_of(self._h, int(best_of)), self._h)

    def decode_timestamps_best_of(self, best_of: int, prompt, max_tokens: int, temperature: float, seed: int = 0,
                                  n: int = 0):
        """One best-of window of encoded clip 0 (rules are used if enabled):
        ([WhisperTokenData dict] of the chosen candidate, its plog float32
        [tokens], p_nosp, chosen, cand_avg float32 [best_of], cand_len int32
        [best_of])."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max(1, max_tokens))()
        cnt = C.c_int32()
        plog = np.zeros(max(1, max_tokens), np.float32)
        pn = C.c_float()
        ch = C.c_int32(-1)
        avg = np.zeros(max(1, best_of), np.float32)
        ln = np.zeros(max(1, best_of), np.int32)
        _raise(lib().wmi_decode_timestamps_best_of(self._h, best_of, _ptr(prompt), prompt.size, max_tokens, temperature,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, n, out, C.byref(cnt), _ptr(plog),
                                                   C.byref(pn), C.byref(ch), _ptr(avg), _ptr(ln)), self._h)
        return ([out[i].as_dict() for i in range(cnt.value)], plog[:cnt.value].copy(), pn.value, ch.value,
                avg[:best_of].copy(), ln[:best_of].copy())

    def best_of_counters(self):
        """The last best-of window: (candidates, decoder steps on one row,
        decoder steps on N rows, chosen candidate) (debug read 35)."""
        return tuple(int(v) for v in np.frombuffer(self.debug_read(35, 16), np.int32))

    def best_of_candidates(self):
        """Every candidate of the last best-of window: a list of ([record
        dict {id, tid, p, pt, ptsum}], plog float32 [records]) (debug read 36)."""
        head = np.frombuffer(self.debug_read(36, 8), np.int32)
        N, M = int(head[0]), int(head[1])
        w = np.frombuffer(self.debug_read(36, 4 * (2 + N + 7 * N * M)), np.int32)
        lens = w[2:2 + N]
        rec = w[2 + N:2 + N + 6 * N * M].reshape(N, M, 6)
        pl = w[2 + N + 6 * N * M:].view(np.float32).reshape(N, M)
        out = []
        for c in range(N):
            r = rec[c, :lens[c]]
            f = r[:, 2:5].copy().view(np.float32)
            out.append(([{"id": int(r[i, 0]), "tid": int(r[i, 1]), "p": float(f[i, 0]), "pt": float(f[i, 1]),
                          "ptsum": float(f[i, 2])} for i in range(lens[c])], pl[c, :lens[c]].copy()))
        return out

    def window_candidates(self, clip: int = 0):
        """Per window of windows_of(clip): (chosen candidate, candidates) of
        the attempt that became its result; (-1, 0) where that was no best-of
        attempt (wmi_get_window_candidate)."""
        n = C.c_int32()
        _raise(lib().wmi_get_window_count(self._h, clip, C.byref(n)), self._h)
        out = []
        for i in range(n.value):
            ch, nc = C.c_int32(), C.c_int32()
            _raise(lib().wmi_get_window_candidate(self._h, clip, i, C.byref(ch), C.byref(nc)), self._h)
            out.append((ch.value, nc.value))
        return out

    def set_rules_beam(self, on: bool = True) -> None:
        """With rules and a beam size above 1, transcribe() windows and
        decode_timestamps_beam() take the ruled beam window
        (wmi_set_rules_beam); off, the default, they stay Unsupported."""
        _raise(lib().wmi_set_rules_beam(self._h, int(on)), self._h)

    def decode_timestamps_ruled_beam(self, beam_size: int, prompt, max_tokens: int):
        """decode_timestamps_beam() under the rules set: ([WhisperTokenData
        dict] of the chosen hypothesis, its summed log-probability, p_nosp)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        out = (TokenData * max(1, max_tokens))()
        n = C.c_int32()
        sc = C.c_double()
        pn = C.c_float()
        _raise(lib().wmi_decode_timestamps_ruled_beam(self._h, beam_size, _ptr(prompt), prompt.size, max_tokens, out,
                                                      C.byref(n), C.byref(sc), C.byref(pn)), self._h)
        return [out[i].as_dict() for i in range(n.value)], sc.value, pn.value

    def rule_history(self, n_steps: int) -> np.ndarray:
        """The last ruled beam window's slot histories (debug read 29), int32
        [n_steps][8][3]: after generation step t slot s has {last id was a
        timestamp, the one before was, the last timestamp + 1 (0: none)}."""
        return np.frombuffer(self.debug_read(29, n_steps * 8 * 3 * 4), np.int32).reshape(n_steps, 8, 3).copy()

    def set_initial_prompt(self, ids=()) -> None:
        """Text ids in front of the first window's context (wmi_set_initial_prompt); () clears."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        _raise(lib().wmi_set_initial_prompt(self._h, _ptr(ids) if ids.size else None, ids.size), self._h)

    # --- token-level timestamps, max_len / split_on_word ----------------------
    def set_token_timestamps(self, enable: bool = True, thold_pt: float = 0.01, thold_ptsum: float = 0.01,
                             max_len: int = 0, split_on_word: bool = False, default: bool = False) -> None:
        """t0 / t1 / vlen of every token of transcribe() / transcribe_batch(),
        and with max_len > 0 their segments cut into pieces at those times
        (wmi_set_token_timestamps); enable=False (or default=True: a NULL
        parameter block) switches it off."""
        if default:
            _raise(lib().wmi_set_token_timestamps(self._h, None), self._h)
            return
        p = TokenTsParams(int(bool(enable)), thold_pt, thold_ptsum, int(max_len), int(bool(split_on_word)))
        _raise(lib().wmi_set_token_timestamps(self._h, C.byref(p)), self._h)

    def token_times(self, tokens, seek: int, t0: int, t1: int, pcm=None):
        """The token times of one segment [t0, t1) of the window at frame seek
        (wmi_token_times): tokens as [WhisperTokenData dict] (id, tid, pt and
        ptsum are read), returned with t0, t1 and vlen filled.  pcm None: the
        envelope of the last recording given."""
        arr = (TokenData * max(1, len(tokens)))()
        for i, t in enumerate(tokens):
            arr[i] = TokenData(int(t["id"]), int(t["tid"]), float(t.get("p", 0.0)), float(t["pt"]), float(t["ptsum"]),
                               -1, -1, 0.0)
        if pcm is None:
            ptr, ns = None, 0
        else:
            pcm = np.ascontiguousarray(pcm, dtype=np.float32)
            # (an empty array still stands for a recording, of no samples)
            ptr, ns = (_ptr(pcm) if pcm.size else C.cast(C.pointer(C.c_float()), C.c_void_p)), pcm.size
        _raise(lib().wmi_token_times(self._h, ptr, ns, int(seek), int(t0), int(t1), arr, len(tokens)), self._h)
        return [arr[i].as_dict() for i in range(len(tokens))]

    # --- token times from cross-attention alignment (DTW) ---------------------
    def set_dtw(self, enable: bool = True, heads=(), n_top: int = 0, medfilt_width: int = 7,
                default: bool = False) -> None:
        """Token times from cross-attention alignment for transcribe() /
        transcribe_batch() (wmi_set_dtw): heads as (layer, head) pairs, or
        every head of the last n_top text layers; enable=False keeps the table
        for align_tokens() only; default=True (a NULL parameter block)
        switches it off and clears the table."""
        if default:
            _raise(lib().wmi_set_dtw(self._h, None), self._h)
            return
        hd = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1)
        p = DtwParams(int(bool(enable)), int(n_top), hd.ctypes.data if hd.size else None, hd.size // 2,
                      int(medfilt_width))
        _raise(lib().wmi_set_dtw(self._h, C.byref(p)), self._h)

    def align_tokens(self, prompt, text, n_frames: int, clip: int = 0):
        """The first frame of every text token, and of what follows the text,
        on encoded clip `clip` (wmi_align_tokens): int32 [len(text) + 1]."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        text = np.ascontiguousarray(text, dtype=np.int32)
        out = np.full(text.size + 1, -1, np.int32)
        _raise(lib().wmi_align_tokens(self._h, clip, _ptr(prompt) if prompt.size else None, prompt.size,
                                      _ptr(text) if text.size else None, text.size, int(n_frames), _ptr(out)), self._h)
        return out

    def dtw_path(self, cost):
        """S6 on the device (wmi_dtw_path): cost int32 [rows][cols] -> the
        smallest column of the path in every row, int32 [rows]."""
        cost = np.ascontiguousarray(cost, dtype=np.int32)
        rows, cols = cost.shape
        out = np.full(max(1, rows), -1, np.int32)
        _raise(lib().wmi_dtw_path(self._h, _ptr(cost) if cost.size else _ptr(out), rows, cols, _ptr(out)), self._h)
        return out[:rows]

    def segment_dtw_of(self, clip: int, i: int):
        """(t0, t1) of every token of segment i of recording `clip`, parallel to
        its tokens (wmi_get_segment_dtw_of); (-1, -1): no text token, or off."""
        n = C.c_int32()
        rc = lib().wmi_get_segment_dtw_of(self._h, clip, i, None, 0, C.byref(n))
        if rc not in (0, NotEnoughSpace.code):
            _raise(rc, self._h)
        out = (DtwTime * max(1, n.value))()
        _raise(lib().wmi_get_segment_dtw_of(self._h, clip, i, out, n.value, C.byref(n)), self._h)
        return [(out[k].t0, out[k].t1) for k in range(n.value)]

    def align_debug(self, A: int, n_pos: int, T: int, n: int, M: int):
        """The last aligned pass's scores s float32 [A][n_pos][T], cost matrix
        int32 [n + 1][M] and path int32 [n + 1] (debug reads 25, 26, 27)."""
        s = np.frombuffer(self.debug_read(25, 4 * A * n_pos * T), np.float32).reshape(A, n_pos, T)
        cq = np.frombuffer(self.debug_read(26, 4 * (n + 1) * M), np.int32).reshape(n + 1, M)
        f = np.frombuffer(self.debug_read(27, 4 * (n + 1)), np.int32)
        return s, cq, f

    def energy(self, n: int):
        """Clip 0's energy envelope of the token-level timestamps: (E uint32
        [n], P uint64 [n + 1]) of the last recording given, of n samples (debug
        reads 23, 24)."""
        E = np.frombuffer(self.debug_read(23, 4 * n), np.uint32)
        P = np.frombuffer(self.debug_read(24, 8 * (n + 1)), np.uint64)
        return E, P

    def windows_of(self, clip: int = 0):
        """Window infos of recording `clip` of the last transcribe() /
        transcribe_batch() under set_fallback ([] when it is off)."""
        n = C.c_int32()
        _raise(lib().wmi_get_window_count(self._h, clip, C.byref(n)), self._h)
        out = []
        for i in range(n.value):
            wi = WindowInfo()
            _raise(lib().wmi_get_window_info(self._h, clip, i, C.byref(wi)), self._h)
            out.append({k: getattr(wi, k) for k, _ in WindowInfo._fields_})
        return out

    # --- pipeline ---------------------------------------------------------
    def pcm_to_mel_batch(self, clips) -> None:
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        ptrs = (C.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
        ns = (C.c_size_t * len(clips))(*[c.size for c in clips])
        _raise(lib().wmi_pcm_to_mel_batch(self._h, len(clips), ptrs, ns), self._h)
        self.n_clips = len(clips)

    # --- audio of any format (clips: see _audio) -----------------------------
    def audio_to_mel_batch(self, clips) -> None:
        """pcm_to_mel_batch() of clips of any rate, channel count and sample
        type: downmix, conversion and resampling to 16 kHz run on the device."""
        arr, keep = _audio(clips)
        _raise(lib().wmi_audio_to_mel_batch(self._h, len(clips), arr), self._h)
        self.n_clips = len(clips)

    def stage_audio(self, clips) -> None:
        """stage() of clips of any format."""
        arr, keep = _audio(clips)
        _raise(lib().wmi_stage_audio(self._h, len(clips), arr), self._h)
        self.n_clips = len(clips)

    def transcribe_audio(self, clip, max_tokens: int = 220):
        """transcribe() of one clip of any format."""
        arr, keep = _audio([clip])
        ns = C.c_int32()
        _raise(lib().wmi_transcribe_audio(self._h, arr, max_tokens, C.byref(ns)), self._h)
        self.n_clips = 1
        return self.segments_of(0, ns.value)

    def transcribe_audio_batch(self, clips, max_tokens: int = 220):
        """transcribe_batch() of clips of any format, each its own."""
        arr, keep = _audio(clips)
        nseg = np.zeros(max(1, len(clips)), np.int32)
        _raise(lib().wmi_transcribe_audio_batch(self._h, len(clips), arr, max_tokens, _ptr(nseg)), self._h)
        self.n_clips = len(clips)
        return [self.segments_of(c, int(nseg[c])) for c in range(len(clips))]

    # --- chunked long-form transcription --------------------------------------
    def set_chunking(self, enable: bool = True, max_frames: int = 0, min_frames: int = 0, smooth_frames: int = 0,
                     default: bool = False) -> None:
        """transcribe_batch() / transcribe_audio_batch() cut every recording at
        quiet places into chunks and decode the chunks as the rows of the rounds
        (wmi_set_chunking; at most min(8, max_clips) rows a round).  0 fields:
        max_frames = the window, min_frames = max_frames / 2, smooth_frames = 10.
        enable=False (or default=True: a NULL parameter block) switches it off."""
        if default:
            _raise(lib().wmi_set_chunking(self._h, None), self._h)
            return
        p = ChunkParams(int(bool(enable)), int(max_frames), int(min_frames), int(smooth_frames))
        _raise(lib().wmi_set_chunking(self._h, C.byref(p)), self._h)

    def set_chunk_spans(self, spans, clip: int = -1) -> None:
        """The caller's (start, end) frame spans of recording `clip` (-1: every
        clip) in later chunked calls, instead of the plan; () = back to the plan."""
        a = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
        _raise(lib().wmi_set_chunk_spans(self._h, int(clip), _ptr(a) if a.size else None, a.shape[0]), self._h)

    def chunks_of(self, clip: int = 0):
        """[wmi_chunk_info dict] of recording `clip` in the last chunked call ([] after one with chunking off)."""
        n = C.c_int32()
        _raise(lib().wmi_get_chunk_count(self._h, clip, C.byref(n)), self._h)
        out = []
        for i in range(n.value):
            ci = ChunkInfo()
            _raise(lib().wmi_get_chunk(self._h, clip, i, C.byref(ci)), self._h)
            out.append(ci.as_dict())
        return out

    def plan_chunks(self, clip: int = 0) -> np.ndarray:
        """The built-in plan of loaded recording `clip` on the device: int64 [n][2] (wmi_plan_chunks)."""
        n = C.c_int32()
        rc = lib().wmi_plan_chunks(self._h, clip, None, 0, C.byref(n))
        if rc not in (WMI_OK, NotEnoughSpace.code):
            _raise(rc, self._h)
        out = np.zeros((n.value, 2), np.int64)
        _raise(lib().wmi_plan_chunks(self._h, clip, _ptr(out), n.value, C.byref(n)), self._h)
        return out

    def pcm(self, clip: int = 0) -> np.ndarray:
        """The 16 kHz mono samples clip holds (wmi_get_pcm)."""
        n = C.c_size_t()
        rc = lib().wmi_get_pcm(self._h, clip, None, 0, C.byref(n))
        if rc not in (WMI_OK, 3):
            _raise(rc, self._h)
        out = np.zeros(n.value, np.float32)
        _raise(lib().wmi_get_pcm(self._h, clip, _ptr(out), out.size, C.byref(n)), self._h)
        return out

    def audio_timing(self) -> dict:
        """Device time of the conversion in the last audio call and the clips it ran a kernel for."""
        ms, n = C.c_float(), C.c_int32()
        _raise(lib().wmi_get_audio_timing(self._h, C.byref(ms), C.byref(n)), self._h)
        return {"convert_ms": ms.value, "n_converted": n.value}

    def encode(self, n_threads: int = 1, mel_offset: int = 0) -> None:
        _raise(lib().wmi_encode(self._h, n_threads, mel_offset), self._h)

    def decode_greedy(self, max_tokens: int, suppress_eot: bool = False):
        toks = np.zeros((self.n_clips, max_tokens), np.int32)
        cnt = np.zeros(self.n_clips, np.int32)
        _raise(lib().wmi_decode_greedy(self._h, max_tokens, int(suppress_eot), _ptr(toks), _ptr(cnt)), self._h)
        return [toks[i, :cnt[i]].copy() for i in range(self.n_clips)]

    def decode_beam(self, beam_size: int, max_tokens: int, suppress_eot: bool = False):
        """Beam search per clip: [(tokens, score)] (semantics: oracle/wmi_oracle.h)."""
        toks = np.zeros((self.n_clips, max_tokens), np.int32)
        cnt = np.zeros(self.n_clips, np.int32)
        sc = np.zeros(self.n_clips, np.float64)
        _raise(lib().wmi_decode_beam(self._h, beam_size, max_tokens, int(suppress_eot), _ptr(toks), _ptr(cnt),
                                     _ptr(sc)), self._h)
        return [(toks[i, :cnt[i]].copy(), float(sc[i])) for i in range(self.n_clips)]

    def decode_logits(self, tokens, clip: int = 0) -> np.ndarray:
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros((tokens.size, self.hparams["n_vocab"]), np.float32)
        _raise(lib().wmi_decode_logits(self._h, clip, _ptr(tokens), tokens.size, _ptr(out)), self._h)
        return out

    def full(self, pcm, max_tokens: int = 224) -> np.ndarray:
        """Transcribe: pcm_to_mel -> encode -> greedy decode (token ids)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        toks = np.zeros(max_tokens, np.int32)
        cnt = np.zeros(1, np.int32)
        _raise(lib().wmi_full(self._h, _ptr(pcm), pcm.size, max_tokens, _ptr(toks), _ptr(cnt)), self._h)
        self.n_clips = 1
        return toks[:cnt[0]].copy()

    def stage(self, clips) -> None:
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        ptrs = (C.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
        ns = (C.c_size_t * len(clips))(*[c.size for c in clips])
        _raise(lib().wmi_stage_pcm(self._h, len(clips), ptrs, ns), self._h)
        self.n_clips = len(clips)

    def run_staged(self, n_decode: int = 128, mel_offset: int = 0, beam_size: int = 0) -> None:
        _raise(lib().wmi_run_staged_beam(self._h, mel_offset, n_decode, beam_size), self._h)
        self._n_decode = n_decode

    def tokens(self) -> np.ndarray:
        out = np.zeros((self.n_clips, self._n_decode), np.int32)
        _raise(lib().wmi_get_tokens(self._h, _ptr(out), out.size, None), self._h)
        return out

    def timings(self) -> dict:
        t = Timings()
        _raise(lib().wmi_get_timings(self._h, C.byref(t)), self._h)
        return {"mel_ms": t.mel_ms, "encode_ms": t.encode_ms, "cross_kv_ms": t.cross_kv_ms,
                "decode_ms": t.decode_ms, "n_decode_steps": t.n_decode_steps}

    def bench_kernel(self, which: int, iters: int = 50) -> dict:
        """Mean duration of one kernel of the last run (HIP events, same stream)."""
        kb = KernelBench()
        _raise(lib().wmi_bench_kernel(self._h, which, iters, C.byref(kb)), self._h)
        return {"name": kb.name.decode(), "avg_us": kb.avg_us, "alg_bytes": kb.alg_bytes, "alg_flops": kb.alg_flops}

    def selftest(self) -> int:
        """Mismatches of the device-computed f16 exp vs the host ggml table."""
        n = C.c_int32()
        _raise(lib().wmi_selftest(self._h, C.byref(n)), self._h)
        return n.value

    def checksums(self) -> dict:
        """The reference's stage sums (wmi_get_checksums; WMI_CHECKSUMS=1 contexts)."""
        out = np.zeros(5, np.float32)
        _raise(lib().wmi_get_checksums(self._h, _ptr(out)), self._h)
        return dict(zip(("hann", "samples", "filters", "mel_raw", "mel_window"), out.tolist()))

    def debug_read(self, which: int, nbytes: int) -> bytes:
        """Raw copy of a device buffer of the last decode (wmi_debug_read)."""
        buf = C.create_string_buffer(nbytes)
        _raise(lib().wmi_debug_read(self._h, which, buf, nbytes), self._h)
        return buf.raw

    def step_logits(self, n_pos: int) -> np.ndarray:
        """Every position's logits of the last persistent greedy decode or
        beam search, [n_pos][rows][V] with rows = max(8, max_clips) (contexts
        created with WMI_LOGITS_ALL=1: position p's logits predict the token
        after the one fed at p; greedy: clip b in row b; beam: slot s)."""
        V = self.hparams["n_vocab"]
        rows = int(np.frombuffer(self.debug_read(16, 4), np.int32)[0])
        raw = self.debug_read(13, n_pos * rows * V * 4)
        return np.frombuffer(raw, np.float32).reshape(n_pos, rows, V).copy()

    def beam_history(self, n_steps: int):
        """The last beam search's selections (its last clip): (parent slot,
        token) arrays [n_steps][8] — slot s after generation step t came from
        slot parent[t][s] of step t - 1 and appended token[t][s]."""
        par = np.frombuffer(self.debug_read(14, n_steps * 8 * 4), np.int32).reshape(n_steps, 8).copy()
        tok = np.frombuffer(self.debug_read(15, n_steps * 8 * 4), np.int32).reshape(n_steps, 8).copy()
        return par, tok

    def conv_input(self, slots: int) -> np.ndarray:
        """The conv-1 input of the last encode (debug read 21), [slots][2 *
        n_ctx + 2][up32(n_mels)]: float16, float32 for f32 models; rows 0 and
        2 * n_ctx + 1 are the convolution's zero padding."""
        cp = (self.hparams["n_mels"] + 31) // 32 * 32
        dt = np.float16 if self.hparams["f16"] else np.float32
        shape = (slots, 2 * self.n_ctx + 2, cp)
        raw = self.debug_read(21, int(np.prod(shape)) * np.dtype(dt).itemsize)
        return np.frombuffer(raw, dt).reshape(shape).copy()

    def batch_windows(self):
        """(src, off) of the last round of transcribe_batch (debug read 22):
        slot b encoded recording src[b]'s window at mel frame off[b]."""
        v = np.frombuffer(self.debug_read(22, 17 * 4), np.int32)
        n = int(v[0])
        return v[1:1 + n].copy(), v[9:9 + n].copy()

    # --- parity getters -----------------------------------------------------
    def mel(self, clip: int = 0) -> np.ndarray:
        nm, nl = C.c_int32(), C.c_int32()
        _raise(lib().wmi_get_mel(self._h, clip, None, 0, C.byref(nm), C.byref(nl)), self._h)
        out = np.zeros((nm.value, nl.value), np.float32)
        _raise(lib().wmi_get_mel(self._h, clip, _ptr(out), out.size, C.byref(nm), C.byref(nl)), self._h)
        return out

    def encoder_out(self, clip: int = 0) -> np.ndarray:
        out = np.zeros((self.n_ctx, self.hparams["n_audio_state"]), np.float32)
        _raise(lib().wmi_get_encoder_out(self._h, clip, _ptr(out), out.size), self._h)
        return out

    def cross_kv(self, clip: int = 0):
        shp = (self.hparams["n_text_layer"], self.n_ctx, self.hparams["n_text_state"])
        k = np.zeros(shp, np.uint16)
        v = np.zeros(shp, np.uint16)
        _raise(lib().wmi_get_cross_kv(self._h, clip, _ptr(k), _ptr(v), k.size), self._h)
        return k, v

    # --- multi-GPU ----------------------------------------------------------
    @staticmethod
    def dist_make_id() -> bytes:
        n = lib().wmi_dist_id_size()
        buf = C.create_string_buffer(n)
        _raise(lib().wmi_dist_make_id(buf))
        return buf.raw

    def dist_init(self, rank: int, world: int, uid: bytes) -> None:
        buf = C.create_string_buffer(uid, len(uid))
        _raise(lib().wmi_dist_init(self._h, rank, world, buf), self._h)
        self.rank, self.world = rank, world

    def dist_gather_tokens(self):
        """Root: (tokens [world][clips][n_decode] with -1 padding, counts
        [world][clips]); other ranks: None."""
        rec = self._n_decode + 1
        total = self.world * self.n_clips * rec
        out = np.zeros(total, np.int32) if self.rank == 0 else None
        _raise(lib().wmi_dist_gather_tokens(self._h, _ptr(out) if out is not None else None, total), self._h)
        if out is None:
            return None
        blk = out.reshape(self.world, self.n_clips, rec)
        return blk[:, :, 1:].copy(), blk[:, :, 0].copy()

    def dist_barrier(self) -> None:
        _raise(lib().wmi_dist_barrier(self._h), self._h)


# reference-named free functions -----------------------------------------------
def whisper_pcm_to_mel(ctx: WhisperContext, samples) -> None:
    """main.rs:1681-1707."""
    ctx.pcm_to_mel_batch([samples])


def whisper_encode(ctx: WhisperContext, n_threads: int, mel_offset: int) -> None:
    """main.rs:1799-2063 (n_threads accepted and ignored, as in the reference)."""
    ctx.encode(n_threads, mel_offset)


def plan_chunks_host(P, n_samples: int, window: int, max_frames: int = 0, min_frames: int = 0,
                     smooth_frames: int = 0) -> np.ndarray:
    """The built-in chunk plan from the running envelope sum P (uint64
    [n_samples + 1]) on the host, no context: int64 [n][2] (wmi_plan_chunks_host)."""
    P = np.ascontiguousarray(P, dtype=np.uint64)
    if P.size < int(n_samples) + 1:
        raise ValueError(f"P holds {P.size} entries for {n_samples} samples")
    p = ChunkParams(0, int(max_frames), int(min_frames), int(smooth_frames))
    n = C.c_int32()
    rc = lib().wmi_plan_chunks_host(_ptr(P), int(n_samples), C.byref(p), int(window), None, 0, C.byref(n))
    if rc not in (WMI_OK, NotEnoughSpace.code):
        _raise(rc)
    out = np.zeros((n.value, 2), np.int64)
    _raise(lib().wmi_plan_chunks_host(_ptr(P), int(n_samples), C.byref(p), int(window), _ptr(out), n.value, C.byref(n)))
    return out


def dtw_path_host(cost):
    """S6 on the host, no context (wmi_dtw_path_host)."""
    cost = np.ascontiguousarray(cost, dtype=np.int32)
    rows, cols = cost.shape
    out = np.full(max(1, rows), -1, np.int32)
    rc = lib().wmi_dtw_path_host(_ptr(cost) if cost.size else _ptr(out), rows, cols, _ptr(out))
    if rc:
        _raise(rc, None)
    return out[:rows]


def best_of_key(seed: int, n: int, c: int) -> int:
    """Candidate c's stream key of attempt ordinal n of `seed` (wmi_best_of_key; host only)."""
    k = C.c_uint64()
    rc = lib().wmi_best_of_key(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(c), C.byref(k))
    if rc:
        _raise(rc, None)
    return k.value
