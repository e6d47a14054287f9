/*
 * whisper_mi355x.h — C ABI of the MI355X-native Whisper hot path.
 *
 * This is the drop-in boundary for szuwgh/whisper.rs (snapshot 2024-08-07).
 * Every entry point below names the reference item it replaces
 * (file:line into /root/reference/src/main.rs).  A Rust caller binds this
 * header with a thin `extern "C"` block; the Python mirror
 * whisper.rs_amd/wmi.py binds it with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every array passed in or out is a HOST
 *    array owned by the caller; results are copied out.  Device memory is
 *    owned by the context.
 *  - Every call returns an int status (enum wmi_status).  Nothing aborts.
 *    wmi_last_error() gives the detailed message (tensor name, sizes, ...),
 *    mirroring the formatted WsError variants (main.rs:51-72).
 *  - One context per host thread per GPU; calls are stream-ordered on the
 *    context's HIP stream and synchronous at return (main.rs takes
 *    `&mut WhisperContext`, so the reference is single-caller too).
 *  - Layouts are the reference's: mel [n_mel][n_len] f32 (main.rs:1633),
 *    encoder output [n_ctx][n_state] f32 (ggml ne [n_state, n_ctx]),
 *    cross K/V [n_text_layer][n_ctx][n_state] f16 (main.rs:2018-2030).
 */
#ifndef WHISPER_MI355X_H
#define WHISPER_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* WsError (main.rs:51-72) mapped 1:1, plus device-side codes. */
enum wmi_status {
    WMI_OK = 0,
    WMI_E_IO = 1,             /* WsError::UnexpectIO        main.rs:54-55 */
    WMI_E_BAD_MAGIC = 2,      /* WsError::BadMagic          main.rs:56-57 */
    WMI_E_NO_SPACE = 3,       /* WsError::NotEnoughSpace    main.rs:58-59 */
    WMI_E_UNKNOWN_TENSOR = 4, /* WsError::UnknownTensor     main.rs:60-61 */
    WMI_E_BAD_REF_TENSOR = 5, /* WsError::BadRefTensor      main.rs:62-63 */
    WMI_E_WRONG_SIZE = 6,     /* WsError::WrongSizeTensor   main.rs:64-65 */
    WMI_E_WRONG_SHAPE = 7,    /* WsError::WrongShapeTensor  main.rs:66-67 */
    WMI_E_WRONG_BYTES = 8,    /* WsError::WrongBytesTensor  main.rs:68-69 */
    WMI_E_OP = 9,             /* WsError::WrongGTensor      main.rs:70-71 */
    WMI_E_UNEXPECTED = 10,    /* WsError::Unexpected        main.rs:52-53 */
    WMI_E_HIP = 11,           /* HIP runtime / kernel launch failure */
    WMI_E_RCCL = 12,          /* RCCL failure */
    WMI_E_UNSUPPORTED = 13,   /* valid file, feature not built (e.g. a ggml type other than f32 / f16 / q4_0 / q4_1 / q5_0 / q5_1 / q8_0) */
    WMI_E_INVALID_ARG = 14    /* bad pointer / size / state order */
};

/* WhisperHparams (main.rs:607-619), same field order as the file. */
typedef struct wmi_hparams {
    int32_t n_vocab;
    int32_t n_audio_ctx;
    int32_t n_audio_state;
    int32_t n_audio_head;
    int32_t n_audio_layer;
    int32_t n_text_ctx;
    int32_t n_text_state;
    int32_t n_text_head;
    int32_t n_text_layer;
    int32_t n_mels;
    int32_t f16;
} wmi_hparams;

/* WhisperVocab special ids after the multilingual shift (main.rs:557-575, 433-440). */
typedef struct wmi_special_tokens {
    int32_t eot, sot, prev, solm, not_, beg, translate, transcribe;
    int32_t is_multilingual;
} wmi_special_tokens;

/* Per-stage device times of the last pipeline call, milliseconds (hipEvents).
 * Replaces the never-written t_*_us fields of WhisperContext (main.rs:334-339). */
typedef struct wmi_timings {
    float mel_ms;
    float encode_ms;     /* conv stem -> ln_post */
    float cross_kv_ms;   /* cross-attention K/V precompute */
    float decode_ms;     /* prompt + generated tokens */
    int32_t n_decode_steps;
} wmi_timings;

typedef struct wmi_context wmi_context;

/* ---- lifecycle ------------------------------------------------------ */

/* WhisperContext::new(fname) (main.rs:366-503): open, magic, hparams,
 * filters, vocab (+extra tokens), weights; then upload to `device`.
 * max_clips sizes the device workspace for batched calls (>= 1).  Weight
 * types: f16 and f32 files (hparams.f16 = 1 / 0, main.rs:817-821; f32
 * matrices are kept f32 on the device) and the ggml quantised types.
 * Shapes: n_text_state == n_audio_state, a multiple of 128 up to 1280 with
 * 64-wide heads, n_text_ctx <= 512, any depths and n_audio_ctx; anything
 * else is WMI_E_UNSUPPORTED as soon as the header is parsed (before a tensor
 * is read or the device touched). */
int wmi_init_from_file(const char *path, int device, int max_clips, wmi_context **out);
void wmi_free(wmi_context *ctx);
const char *wmi_strerror(int status);
const char *wmi_last_error(const wmi_context *ctx);
/* Library-level last error (for failures before a context exists). */
const char *wmi_last_error_global(void);

int wmi_get_hparams(const wmi_context *ctx, wmi_hparams *out);
int wmi_get_special_tokens(const wmi_context *ctx, wmi_special_tokens *out);
/* WhisperContext.exp_n_audio_ctx (main.rs:362, 1803-1807): 0 = n_audio_ctx. */
int wmi_set_audio_ctx(wmi_context *ctx, int n_audio_ctx);
/* id_to_token (main.rs:578-592, 442-467): copies the token bytes (not NUL
 * terminated) into buf, *len = byte count; WMI_E_NO_SPACE if cap too small. */
int wmi_token_to_bytes(const wmi_context *ctx, int32_t id, char *buf, size_t cap, size_t *len);

/* ---- language and task ------------------------------------------------ */

/* Languages are indexed in whisper.cpp's order (en = 0, zh = 1, ... yue =
 * 99); the language token of index i is sot + 1 + i.  A multilingual file has
 * 99 languages (100 from large-v3 on), an English-only (.en) file none.
 *
 * The settings live on the context until changed; the defaults are language
 * 0 and transcribe.  They select the prompt [SOT, language, task, NOT] of
 * wmi_decode_greedy, wmi_decode_beam, wmi_full, wmi_run_staged,
 * wmi_run_staged_beam and wmi_transcribe (wmi_decode_logits and
 * wmi_decode_timestamps take explicit tokens).  With WMI_LANG_AUTO a clip's
 * language is detected on the device at the start of the decode and its token
 * goes into the prompt there, without a host round trip; wmi_transcribe
 * detects once, on the first window, and keeps that language.  On an
 * English-only file any language other than 0, WMI_LANG_AUTO, translate and
 * wmi_detect_language return WMI_E_INVALID_ARG. */
#define WMI_LANG_AUTO (-1)
enum wmi_task { WMI_TASK_TRANSCRIBE = 0, WMI_TASK_TRANSLATE = 1 };

/* Language table (host only, no context or device). */
int wmi_lang_index(const char *code, int32_t *index);   /* unknown code: WMI_E_INVALID_ARG */
const char *wmi_lang_code(int index);                   /* NULL outside [0, 100) */
int wmi_lang_count(const wmi_context *ctx, int32_t *n); /* 0 / 99 / 100 */

/* clip in [0, max_clips), or -1 = every clip; lang = index or WMI_LANG_AUTO
 * (an index >= the file's language count: WMI_E_INVALID_ARG). */
int wmi_set_language(wmi_context *ctx, int clip, int lang);
int wmi_set_task(wmi_context *ctx, int task);

/* One decoder step on [SOT] for every encoded clip.  lang[n_clips] = most
 * probable language (ties: lowest index).  probs (optional) is
 * [n_clips][n_lang] f32: the softmax over the language logits, computed in
 * double.  Changes no setting. */
int wmi_detect_language(wmi_context *ctx, int32_t *lang, float *probs);

/* Language index the last decode / transcribe used for `clip` (before any:
 * the explicit setting, or WMI_LANG_AUTO).  *p (optional) = its detection
 * probability, or -1 if the language was set explicitly. */
int wmi_get_language(const wmi_context *ctx, int clip, int32_t *lang, float *p);

/* ---- audio input and text output --------------- */

/* hound::WavReader::open(path) + samples::<i16>() (main.rs:2067-2068):
 * 16-bit integer PCM RIFF/WAVE, samples interleaved as stored.  With
 * samples == NULL only *n_samples (and rate / channels) are filled.
 * WMI_E_IO: missing / malformed file; WMI_E_UNSUPPORTED: not 16-bit PCM;
 * WMI_E_NO_SPACE: cap < *n_samples.  Needs no context or device. */
int wmi_read_wav(const char *path, int16_t *samples, size_t cap, size_t *n_samples, int32_t *sample_rate,
                 int32_t *channels);
/* convert_integer_to_float_audio (main.rs:1673-1679): out[i] = s16[i] / 32768. */
int wmi_pcm16_to_f32(const int16_t *s16, size_t n, float *out);
/* Detokenise: the id_to_token bytes (main.rs:578-592) of the text tokens
 * (id < eot) of ids[0..n), concatenated; special and timestamp tokens are
 * skipped.  *len = byte count; WMI_E_NO_SPACE if cap < *len. */
int wmi_tokens_to_text(const wmi_context *ctx, const int32_t *ids, int n, char *buf, size_t cap, size_t *len);

/* ---- pipeline (reference entry points) ------------------------------ */

/* whisper_pcm_to_mel (main.rs:1681-1707): f32 PCM (s16/32768) -> log-mel. */
int wmi_pcm_to_mel(wmi_context *ctx, const float *pcm, size_t n_samples);
/* Batched form: n_clips independent clips (each <= max_clips). */
int wmi_pcm_to_mel_batch(wmi_context *ctx, int n_clips, const float *const *pcm, const size_t *n_samples);

/* whisper_encode (main.rs:1799-2063): mel window at mel_offset -> conv stem
 * -> encoder blocks -> ln_post -> cross-attention K/V for every decoder
 * layer.  n_threads is accepted and ignored, as in the reference (:1799).
 * Runs on every clip loaded by the last pcm_to_mel call. */
int wmi_encode(wmi_context *ctx, int n_threads, int mel_offset);

/* Greedy decode (the reference declares the decoder but has
 * no forward pass).  Prompt = [SOT] (.en) or [SOT, language, task] as set
 * by wmi_set_language / wmi_set_task (default: en, transcribe; each clip its
 * own language), then NOT.  Generates up to max_tokens ids per clip; stops a clip at EOT
 * unless suppress_eot != 0 (then exactly max_tokens).  tokens is
 * [n_clips][max_tokens]; n_tokens[c] = ids written for clip c. */
int wmi_decode_greedy(wmi_context *ctx, int max_tokens, int suppress_eot,
                      int32_t *tokens, int32_t *n_tokens);

/* Teacher-forced decoder logits for clip `clip`: feeds tokens[0..n) one at a
 * time from position 0 and writes logits[n][n_vocab] (f32). */
int wmi_decode_logits(wmi_context *ctx, int clip, const int32_t *tokens, int n_tokens, float *logits);

/* Beam search (config C5; absent from the reference, semantics after OpenAI
 * whisper's BeamSearchDecoder without length penalty, stated in
 * oracle/wmi_oracle.h).  beam_size <= 8; one clip at a time, beam_size decoder
 * rows.  tokens is [n_clips][max_tokens]: the best hypothesis (ending in EOT
 * if it finished); n_tokens[c] its length; scores[c] (optional) its summed
 * log-probability. */
int wmi_decode_beam(wmi_context *ctx, int beam_size, int max_tokens, int suppress_eot, int32_t *tokens,
                    int32_t *n_tokens, double *scores);

/* Transcribe: pcm_to_mel -> encode -> decode_greedy for one clip. */
int wmi_full(wmi_context *ctx, const float *pcm, size_t n_samples, int max_tokens,
             int32_t *tokens, int32_t *n_tokens);

/* ---- timestamps, segments, long audio ---------- */

/* WhisperTokenData (main.rs:317-331) as sampled: id, tid = most probable
 * timestamp token, p = P(id), pt = P(tid) / (sum of timestamp
 * probabilities + 1e-10), ptsum = that sum.  Token-level t0 / t1 are not
 * computed (-1) and vlen is 0, as in whisper.cpp-1.0.3 by default; under
 * wmi_set_token_timestamps the segment getters of wmi_transcribe /
 * wmi_transcribe_batch fill them (10 ms units), as does wmi_token_times. */
typedef struct wmi_token_data {
    int32_t id, tid;
    float p, pt, ptsum;
    int64_t t0, t1;
    float vlen;
} wmi_token_data;

/* One timestamp-decoding window of the encoded clip 0 after `prompt`
 * (whisper.cpp-1.0.3 sampling: the first token is the most probable
 * timestamp > beg; then a timestamp whenever the timestamp probabilities sum
 * above the most probable text token, else the most probable token other
 * than sot / solm / not).  Stops after EOT or max_tokens; out[max_tokens]. */
int wmi_decode_timestamps(wmi_context *ctx, const int32_t *prompt, int n_prompt, int max_tokens,
                          wmi_token_data *out, int32_t *n_out);
/* whisper_full with timestamps over audio of any length: 30 s windows
 * (2 * n_audio_ctx mel frames) advanced by the last timestamp (mel_offset,
 * main.rs:1822-1823), earlier text as prompt context; fills the context's
 * segment list (WhisperSegment, main.rs:599-604; result_all, main.rs:353).
 * max_tokens caps the tokens per window (<= n_text_ctx / 2 - 4). */
int wmi_transcribe(wmi_context *ctx, const float *pcm, size_t n_samples, int max_tokens, int32_t *n_segments);
/* Segment i of the last transcribe: [t0, t1) in 10 ms units, text bytes. */
int wmi_get_segment(const wmi_context *ctx, int i, int64_t *t0, int64_t *t1, char *text, size_t cap, size_t *len);
/* Its tokens (text and timestamp tokens of the segment). */
int wmi_get_segment_tokens(const wmi_context *ctx, int i, wmi_token_data *out, size_t cap, int32_t *n);

/* no_context = 1: every window of wmi_transcribe decodes from the initial
 * prompt [SOT (, language, task)] alone, without <|prev|> and the earlier
 * text (whisper.cpp's no_context, OpenAI's condition_on_previous_text=False).
 * Default 0.  Holds until changed. */
int wmi_set_no_context(wmi_context *ctx, int no_context);

/* ---- beam search in timestamped decoding ------------------------------- */

/* wmi_decode_timestamps with beam search: K = beam_size (1..8) hypotheses of
 * encoded clip 0; out = the chosen hypothesis' tokens, *score (optional) its
 * summed log-probability under the masked distributions.  Every hypothesis
 * row takes the timestamp rule of wmi_decode_timestamps on its own logits
 * (first token: ids > beg; then the timestamp ids when their probabilities
 * sum above the most probable text token, else every id but sot / solm /
 * not), contributes its K + 1 most probable allowed ids renormalised over
 * that set, and the candidates are ranked, finished and chosen as by
 * wmi_decode_beam (best score / length).  At beam_size 1 the ids and tids
 * are those of wmi_decode_timestamps.  out[max_tokens]. */
int wmi_decode_timestamps_beam(wmi_context *ctx, int beam_size, const int32_t *prompt, int n_prompt,
                               int max_tokens, wmi_token_data *out, int32_t *n_out, double *score);
/* Beam size of wmi_transcribe's windows; default 1 = the greedy sampler,
 * exactly as before.  Holds until changed.  Outside [1, 8]:
 * WMI_E_INVALID_ARG.  wmi_transcribe_batch with a beam size above 1 set is
 * WMI_E_UNSUPPORTED (8 recordings x K hypotheses do not fit the 8 decoder
 * rows); wmi_decode_timestamps and wmi_decode_timestamps_batch ignore it. */
int wmi_set_beam_size(wmi_context *ctx, int beam_size);

/* ---- batched timestamped transcription -------------------------------- */

/* wmi_decode_timestamps for every encoded clip at once: one window per clip
 * after the one shared prompt, up to 8 clips per decoder step.  out is
 * [n_clips][max_tokens]; n_out[c] counts clip c's tokens up to and including
 * its EOT (nothing is written behind it).  A clip that has met EOT waits for
 * the others of its block.  For one clip: what wmi_decode_timestamps returns. */
int wmi_decode_timestamps_batch(wmi_context *ctx, const int32_t *prompt, int n_prompt, int max_tokens,
                                wmi_token_data *out, int32_t *n_out);
/* wmi_transcribe over n_clips recordings (1 <= n_clips <= max_clips) of any,
 * unequal lengths, up to 8 of them per decoder step: per round every active
 * recording's next window is encoded at its own seek and the windows are
 * decoded in lockstep; a recording that reached its end frees its row for a
 * waiting one.  By default windows decode without earlier text (as with
 * wmi_set_no_context(1), whatever that setting is): recording c yields the
 * segments wmi_transcribe gives for it alone with no-context on and the same
 * language and task, whichever other recordings share the batch.  Under
 * wmi_set_batch_context(1) every recording carries its own text context
 * instead.  Language of clip c: wmi_set_language(c, ..);
 * WMI_LANG_AUTO is detected on that recording's first window and kept
 * (wmi_get_language(c)).  n_segments[n_clips]; read the segments with the
 * _of getters below. */
int wmi_transcribe_batch(wmi_context *ctx, int n_clips, const float *const *pcm, const size_t *n_samples, int max_tokens,
                         int32_t *n_segments);
/* wmi_get_segment / wmi_get_segment_tokens for recording `clip` of the last
 * wmi_transcribe_batch (or clip 0 of the last wmi_transcribe); the getters
 * without a clip read clip 0. */
int wmi_get_segment_of(const wmi_context *ctx, int clip, int i, int64_t *t0, int64_t *t1, char *text, size_t cap,
                       size_t *len);
int wmi_get_segment_tokens_of(const wmi_context *ctx, int clip, int i, wmi_token_data *out, size_t cap, int32_t *n);
/* enable 1: wmi_transcribe_batch / wmi_transcribe_audio_batch give every
 * recording its own text context, as wmi_transcribe does: recording c yields
 * the segments wmi_transcribe gives for it alone under the same settings
 * (no_context as set — with wmi_set_no_context(1) the batch stays without
 * context —, language, task, fallback, rules, initial prompt, token times,
 * DTW).  Rows of a round then hold prompts of unequal length.  The decoder
 * keeps its one step position and right-aligns the rows: a row whose prompt is
 * shorter than the round's longest starts that many steps later, so that
 * every row samples its first token at the same step.  Such a row takes its
 * position embedding relative to its own start and its self-attention never
 * looks at keys before it, so from its start on it computes what it computes
 * alone, up to the order of the key sums.  A round costs the steps of its
 * longest prompt.  enable 0 (default): every call runs exactly the kernels it
 * ran before.  Neither 0 nor 1: WMI_E_INVALID_ARG.  Holds until changed.  A
 * beam size above 1 in the batch stays WMI_E_UNSUPPORTED. */
int wmi_set_batch_context(wmi_context *ctx, int enable);
/* wmi_decode_timestamps_batch with a prompt per row: row b (encoded clip b)
 * decodes after prompts[b * prompt_stride .. + n_prompt[b]); out is
 * [n_clips][max_tokens], n_out as there.  Rows of unequal length are
 * right-aligned as under wmi_set_batch_context.  Equal lengths: exactly
 * wmi_decode_timestamps_batch.  n_prompt[b] < 1, > prompt_stride, or
 * max n_prompt + max_tokens > n_text_ctx: WMI_E_INVALID_ARG. */
int wmi_decode_timestamps_rows(wmi_context *ctx, const int32_t *prompts, const int32_t *n_prompt, int prompt_stride,
                               int max_tokens, wmi_token_data *out, int32_t *n_out);

/* ---- temperature fallback, quality thresholds, no-speech ---------------- */

/* The per-window decode loop of OpenAI's decode_with_fallback / whisper.cpp
 * 1.2 for wmi_transcribe and wmi_transcribe_batch.  A window is decoded at
 * T_j = temperature + j * temperature_inc for j = 0, 1, .. while T_j <= 1
 * (one attempt with temperature_inc 0).  At T = 0 the token is the most
 * probable allowed one (wmi_decode_timestamps' pick, or the beam window with
 * wmi_set_beam_size above 1); at T > 0 it is drawn from the allowed set's
 * distribution softmax(l / T) with u_t = (sm64(key + t) >> 11) * 2^-53, sm64 =
 * splitmix64 and key = sm64(seed + n), n = the T > 0 attempts the recording
 * has made before in the call.  Over the window's tokens (EOT included):
 * avg_logprob = the mean log-probability under the masked distribution at
 * temperature 1; entropy = that of the id counts over its last 32 tokens.  An
 * attempt is rejected if the window failed (would skip 100 frames), avg_logprob
 * < logprob_thold or entropy < entropy_thold; the first accepted attempt, or
 * the last one, is the window's result.  After attempt 0, no_speech_prob
 * (P(<|nospeech|>) of the first generated step) > no_speech_thold together
 * with avg_logprob < logprob_thold skips the window without segments.  A
 * result of T > 0.5 clears the text context of later windows.
 * Defaults (also params = NULL): temperature 0, temperature_inc 0,
 * logprob_thold = entropy_thold = -inf, no_speech_thold = +inf, seed 0 — with
 * them every call decodes exactly as without this interface (the same
 * kernels, no window infos).  NaN, temperature outside [0, 1], a negative
 * increment or one in (0, 0.01) (more than 101 attempts a window):
 * WMI_E_INVALID_ARG.  A vocabulary above 65536 ids, or one whose sot / solm /
 * not ids are not below beg (no Whisper vocabulary): WMI_E_UNSUPPORTED.
 * Holds until changed. */
typedef struct wmi_fallback_params {
    float temperature, temperature_inc, logprob_thold, entropy_thold, no_speech_thold;
    uint64_t seed;
} wmi_fallback_params;
int wmi_set_fallback(wmi_context *ctx, const wmi_fallback_params *params);
/* One window of the encoded clip 0 at one temperature, as attempt ordinal n of
 * `seed` (the key of the draws; unused at temperature 0, where ids, tids and
 * records are those of wmi_decode_timestamps).  out[max_tokens];
 * plog[max_tokens] (optional) each token's log-probability as in avg_logprob;
 * *p_nosp (optional) the no-speech probability. */
int wmi_decode_timestamps_sampled(wmi_context *ctx, const int32_t *prompt, int n_prompt, int max_tokens,
                                  float temperature, uint64_t seed, int n, wmi_token_data *out, int32_t *n_out,
                                  float *plog, float *p_nosp);
/* Window i of recording `clip` in the last wmi_transcribe /
 * wmi_transcribe_batch made with fallback parameters other than the defaults
 * (the count is 0 otherwise): the window's start frame, the attempts made, and
 * of the attempt that became the result its temperature, avg_logprob and
 * entropy; the no-speech probability of attempt 0; its segments
 * [first_segment, first_segment + n_segments) of the recording.
 * flags: 1 = skipped as silence, 2 = failed (100-frame skip), 4 = every
 * attempt was rejected, 8 = the text context was reset after it. */
typedef struct wmi_window_info {
    int64_t seek;
    int32_t n_attempts;
    float temperature, avg_logprob, entropy, no_speech_prob;
    int32_t flags, first_segment, n_segments;
} wmi_window_info;
int wmi_get_window_count(const wmi_context *ctx, int clip, int32_t *n);
int wmi_get_window_info(const wmi_context *ctx, int clip, int i, wmi_window_info *out);

/* ---- best-of-N sampled attempts ------------------------------------------ */

/* A best-of window of N candidates (1 <= N <= 8) of an encoded clip after
 * `prompt`, at temperature T in (0, 1], as attempt ordinal n of `seed`
 * (OpenAI's and whisper.cpp's best_of).
 * Candidates and keys: candidate c has the stream key k_0 = sm64(seed + n)
 * (wmi_decode_timestamps_sampled's key) and k_c = sm64(k_0 + c * 2^32) for
 * c >= 1; its draws are u_t = (sm64(k_c + t) >> 11) * 2^-53 as there.  Each
 * candidate is a window of wmi_decode_timestamps_sampled with that key; with
 * rules enabled a window of wmi_decode_timestamps_ruled, with a history of
 * its own.
 * Shared first step: candidate c's first generated token is drawn from the
 * logits of the prompt's last step.  That step is computed once, on one
 * decoder row, and every candidate reads the same row; the no-speech
 * probability is that row's and is computed once.  From the second generated
 * step on candidate c decodes on a decoder row of its own, after its own
 * tokens; the prompt's keys and values are read where the one row left them
 * (nothing is copied).  A candidate that has drawn EOT writes no further
 * record and feeds EOT.  The window ends when every candidate has met EOT, or
 * at max_tokens.
 * Ranking: n_c = candidate c's records, EOT included; S_c = the sum of its
 * f32 log-probabilities (plog), taken in float64 in index order; a_c = S_c /
 * n_c.  The chosen candidate is the one with the largest a_c, ties to the
 * lowest c.  a_c is wmi_set_fallback's avg_logprob: one figure serves the
 * ranking and the threshold (OpenAI divides by the length without EOT for the
 * ranking and with it for the threshold).
 * N = 1 is exactly wmi_decode_timestamps_sampled / wmi_decode_timestamps_ruled:
 * the same kernels and the same bits.
 *
 * wmi_set_best_of: best_of 1..8, default 1; anything else WMI_E_INVALID_ARG.
 * Holds until changed.  Above 1, every attempt of wmi_transcribe /
 * wmi_transcribe_audio at T > 0 under wmi_set_fallback is a best-of window:
 * the chosen candidate is judged and committed as the single draw is, and one
 * attempt still takes one ordinal n.  Attempts at T = 0 are untouched (the
 * greedy pick, the beam window or the ruled beam window).
 * wmi_transcribe_batch, wmi_transcribe_audio_batch and chunked calls are
 * WMI_E_UNSUPPORTED, checked at the call, when best_of is above 1 and a
 * temperature above 0 can be reached (temperature > 0 or temperature_inc >
 * 0): as for a beam size, the rows do not fit.  With best_of 1 every call
 * runs the kernels and code objects it ran before this interface. */
int wmi_set_best_of(wmi_context *ctx, int best_of);
/* One best-of window of the encoded clip 0.  out[max_tokens], *n_out and
 * plog[max_tokens] (optional) receive the chosen candidate, *p_nosp
 * (optional) the no-speech probability, *chosen (optional) its index;
 * cand_avg[best_of] and cand_len[best_of] (optional) every candidate's a_c
 * and n_c.  Rules are used if enabled.  best_of outside [1, 8], or above 1
 * with temperature at or below 0: WMI_E_INVALID_ARG. */
int wmi_decode_timestamps_best_of(wmi_context *ctx, int best_of, const int32_t *prompt, int n_prompt, int max_tokens,
                                  float temperature, uint64_t seed, int n, wmi_token_data *out, int32_t *n_out,
                                  float *plog, float *p_nosp, int32_t *chosen, float *cand_avg, int32_t *cand_len);
/* *key = k_c of attempt ordinal n of `seed` (host only: needs no context and
 * no device).  n < 0 or c outside [0, 8): WMI_E_INVALID_ARG. */
int wmi_best_of_key(uint64_t seed, int n, int c, uint64_t *key);
/* Of the window that wmi_get_window_info(ctx, clip, i) describes: the
 * candidate that became its result and the candidates its attempt drew.
 * *chosen is -1 (and *n_candidates 0) when the window's result did not come
 * from a best-of attempt. */
int wmi_get_window_candidate(const wmi_context *ctx, int clip, int i, int32_t *chosen, int32_t *n_candidates);

/* OpenAI's decoding rules (SuppressTokens and ApplyTimestampRules restated)
 * for every window of wmi_transcribe / wmi_transcribe_batch and for
 * wmi_decode_timestamps_ruled, in the place of the whisper.cpp-1.0.3 rule.
 * Per decoder row and generated-token index t, s[0..t) the ids the row has
 * sampled in this window, all arithmetic in float64 on the f32 logits:
 *   M0 masked always: sot, prev, solm, not, translate, transcribe, every
 *      language id, the suppress list (with suppress_non_speech also
 *      wmi_non_speech_tokens).
 *   M1 last = s[t-1] is a timestamp, penult = t < 2 or s[t-2] is one.
 *      last and penult: no timestamp.  last and not penult: no id below eot
 *      (a timestamp or EOT follows).  x = the last timestamp sampled: no
 *      timestamp below x (last and not penult) or below x + 1 (otherwise).
 *   M2 t = 0: timestamps only, none above beg + max_initial_ts (if >= 0).
 * Over the ids left (A'): sum_ts = P(timestamps), p_tx = the largest P of an id
 * below beg (EOT included); the pick is among the timestamps of A' if sum_ts >
 * p_tx, else among A': its argmax at temperature 0 (ties: lowest id), the
 * draw of wmi_decode_timestamps_sampled otherwise.  Records: tid = id for a
 * timestamp, else the likeliest timestamp of A' (of all, with pt 0, if A'
 * holds none); p, pt and ptsum under the softmax over A'; the log-probability
 * under the softmax over the set picked from.  SuppressBlank is not built: it
 * acts on the first token only, which M2 restricts to timestamps.
 * enable 0 (also params = NULL): every call decodes exactly as without this
 * interface (the same kernels).  A suppress id outside [0, eot):
 * WMI_E_INVALID_ARG; the vocabulary conditions of wmi_set_fallback:
 * WMI_E_UNSUPPORTED.  With rules enabled a beam size above 1 is
 * WMI_E_UNSUPPORTED in wmi_transcribe and wmi_decode_timestamps_beam unless
 * the context has opted into the ruled beam window (wmi_set_rules_beam below).
 * Holds until changed. */
typedef struct wmi_decode_rules {
    int32_t enable;               /* 0 (default, also params = NULL): the sampler as before */
    int32_t max_initial_ts;       /* first timestamp <= beg + this, in 20 ms units; < 0: no cap (OpenAI: 50) */
    int32_t suppress_non_speech;  /* add wmi_non_speech_tokens to the list */
    const int32_t *suppress;      /* copied */
    int32_t n_suppress;
} wmi_decode_rules;
int wmi_set_decode_rules(wmi_context *ctx, const wmi_decode_rules *params);
/* The ids below eot whose token bytes are exactly s or " " + s for s one of
 * " # ( ) * + / : ; < = > @ [ \ ] ^ _ ` { | } ~ 「 」 『 』 << >> <<< >>> -- ---
 * -( -[ (' (" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪ ♩ ♪ ♫ ♬ ♭ ♮ ♯, and the tokens " -"
 * and " '" (whisper.cpp's list; a vocabulary lookup, host only): ascending,
 * unique.  *n = their count; WMI_E_NO_SPACE if cap is below it (ids may be
 * NULL to ask for the count). */
int wmi_non_speech_tokens(const wmi_context *ctx, int32_t *ids, size_t cap, int32_t *n);
/* 1 if the len bytes are one of those tokens, else 0 (the lookup's test of one
 * vocabulary entry; needs no context and no device). */
int wmi_is_non_speech_token(const char *bytes, size_t len);
/* wmi_decode_timestamps_sampled under the rules set (WMI_E_INVALID_ARG if
 * none are enabled). */
int wmi_decode_timestamps_ruled(wmi_context *ctx, const int32_t *prompt, int n_prompt, int max_tokens,
                                float temperature, uint64_t seed, int n, wmi_token_data *out, int32_t *n_out,
                                float *plog, float *p_nosp);
/* ---- the decoding rules in the beam window -------------------------------- */

/* wmi_decode_timestamps_beam under the rules set: K = beam_size (1..8)
 * hypotheses, each active row b with a history s_b, the ids of its own
 * hypothesis in this window.  A' of the row: the masks M0 - M2 above, M1 from
 * s_b.  Over A': sum_ts = P(timestamps), p_tx = the largest P of an id below
 * beg (EOT included; 0 if none); the row's set A = the timestamps of A' if
 * sum_ts > p_tx, else A'.  The row contributes its top K + 1 ids of A by logit
 * (ties: lower id; fewer if A holds fewer), each scored score_b + (l_i -
 * lse_A) in float64.  Ranking, walk, finished list, stop and the final choice
 * are wmi_decode_timestamps_beam's.  A new slot's history is its parent's
 * followed by the id it took.  Records as wmi_decode_timestamps_ruled's (tid,
 * p, pt, ptsum under the softmax over A'), from the row that produced each
 * token; *score = the chosen hypothesis' summed log-probability under its
 * rows' sets A.  At beam_size 1 the ids and tids are
 * wmi_decode_timestamps_ruled's at temperature 0.  score and p_nosp (P(solm)
 * under the unmasked softmax of the first generated step) may be NULL.  No
 * rules enabled, or beam_size outside [1, 8]: WMI_E_INVALID_ARG. */
int wmi_decode_timestamps_ruled_beam(wmi_context *ctx, int beam_size, const int32_t *prompt, int n_prompt,
                                     int max_tokens, wmi_token_data *out, int32_t *n_out, double *score,
                                     float *p_nosp);
/* enable 1: with rules and a beam size above 1, a temperature-0 window of
 * wmi_transcribe / wmi_transcribe_audio is the ruled beam window, and
 * wmi_decode_timestamps_beam under rules is wmi_decode_timestamps_ruled_beam.
 * Under wmi_set_fallback attempt 0 is that window, judged as the beam window
 * is (its score as the summed log-probability, the no-speech probability of
 * its first generated step); attempts at T > 0 draw one hypothesis under the
 * rules, as at beam size 1.  enable 0 (the default): rules with a beam size
 * above 1 stay WMI_E_UNSUPPORTED, and every call runs the kernels it ran
 * before this interface.  wmi_transcribe_batch with a beam size stays
 * WMI_E_UNSUPPORTED either way.  Neither 0 nor 1: WMI_E_INVALID_ARG.  Holds
 * until changed. */
int wmi_set_rules_beam(wmi_context *ctx, int enable);
/* Text ids (below eot, else WMI_E_INVALID_ARG) in front of the text context
 * of wmi_transcribe: window 0 decodes from [prev] + ids + [sot ..], later
 * windows see the tail of ids + text (at most n_text_ctx / 2 ids, of which
 * the last are kept here too); a fallback result of T > 0.5 clears them with
 * the rest.  With wmi_set_no_context(1), and in wmi_transcribe_batch without
 * wmi_set_batch_context(1) (one prompt for all recordings), every window
 * decodes from [prev] + ids + [sot ..] — OpenAI prompts the first window
 * only; this keeps the rows of such a batch at one distance into their
 * prompts.  Under wmi_set_batch_context(1) the ids seed every recording's own
 * context, as in wmi_transcribe.  n = 0 clears.  Independent of the rules. */
int wmi_set_initial_prompt(wmi_context *ctx, const int32_t *ids, int n);

/* ---- token-level timestamps, max_len / split_on_word -------------------- */

/* whisper.cpp-1.0.3's token_timestamps, max_len (-ml) and split_on_word
 * (-sow): a start and an end for every token of every segment, and segments
 * cut into pieces at those times.  Restated order-independently; times in
 * 10 ms units; a text token has id < eot; a segment has tokens tau_0 ..
 * tau_{n-1}, bounds T0, T1 and W = the frame its window started at; N = the
 * recording's samples (at most 2^26 with the feature on, else
 * WMI_E_UNSUPPORTED).
 *   Energy  a_i = min(rint(min(|pcm_i|, 16) * 2^20), 2^24), NaN -> 0;
 *      E_i = sum of a_j over |j - i| <= 32 inside [0, N) (uint32);
 *      P_k = sum of E_i over i < k (uint64).
 *   A  vlen of a text token: over its bytes, in f32, ' ' adds 0.01, ',' 2,
 *      each of . ! ? 0 .. 9 adds 3, any other byte 1.  Other tokens: 0.
 *   B  Text tokens k = 1 .. m, b_0 = T0, b_m = T1, ta = T0.  For k = 2 .. m,
 *      tt = W + 2 (tid_k - beg): if pt_k > thold_pt, ptsum_k > thold_ptsum,
 *      tt > ta and tt <= T1 then b_{k-1} = tt, ta = tt.  A run of unset
 *      boundaries between set b_p and b_q: psum = sum of (double) vlen_k over
 *      k = p+1 .. q; b_r = b_{r-1} + trunc((double)(b_q - b_p) * (double)
 *      vlen_r / psum) (b_{r-1} if psum is 0).  Token k: t0 = b_{k-1}, t1 = b_k.
 *   C  (N > 0) For k = 1 .. m in order: s0 = clamp(160 t0, 0, N-1), s1 likewise
 *      of t1; ss0 = max(s0 - 2000, 0), ss1 = min(s1 + 2000, N), ns = ss1 - ss0,
 *      S = P[ss1] - P[ss0]; above(i): 2 ns E_i > S, below(i): 2 ns E_i < S.
 *      Start: j = s0.  If above(s0) and k > 1: while j > 0 and above(j), j--;
 *      t0 = j / 160; if t0 < t1 of token k-1 (final), t0 = that, else s0 = j.
 *      Otherwise: while below(j) and j < s1, j++; s0 = j, t0 = j / 160.
 *      End: j = s1.  If above(s1): while j < N-1 and above(j), j++; t1 =
 *      j / 160; if k < m and t1 > t0 of token k+1 (from B), t1 = that, else
 *      s1 = j.  Otherwise: while below(j) and j > s0, j--; s1 = j, t1 = j / 160.
 *   D  Another token takes t0 = t1 = T0 before the first text token, T1 after
 *      the last, else the final t1 of the text token before it (m = 0: T0).
 *   E  (max_len > 0) acc = 0; a text token of L bytes closes the piece before
 *      it if acc > 0, acc + L > max_len and (not split_on_word, or its first
 *      byte is ' '): the piece ends and the next starts at this token's t0, acc
 *      = 0; then acc += L.  The last piece ends at T1; a piece's text is its
 *      text tokens' bytes; other tokens stay in the piece they follow.
 * enable != 0: every later wmi_transcribe / wmi_transcribe_batch computes the
 * envelope once per recording and A - E for each window's result, whatever
 * beam size, fallback, rules or prompt chose it; the segment getters, counts
 * and wmi_window_info.first_segment / n_segments then speak of pieces.  The
 * text context of later windows is not affected.  enable 0 (default, also
 * params = NULL): every call runs exactly the kernels it ran without this
 * interface, t0 = t1 = -1 and vlen = 0.  The thresholds and max_len are kept
 * either way (params = NULL: 0.01, 0.01, 0, 0).  NaN thresholds or a negative
 * max_len: WMI_E_INVALID_ARG.  Holds until changed. */
typedef struct wmi_token_ts_params {
    int32_t enable;              /* 0 (default, also params = NULL) */
    float thold_pt, thold_ptsum; /* whisper.cpp: 0.01, 0.01 */
    int32_t max_len;             /* 0: no splitting */
    int32_t split_on_word;
} wmi_token_ts_params;
int wmi_set_token_timestamps(wmi_context *ctx, const wmi_token_ts_params *params);
/* Steps A - D for the n tokens of one segment [t0, t1) of the window at frame
 * seek, under the thresholds set (enabled or not): vlen, t0 and t1 of tokens
 * are written, the rest is read.  pcm [n_samples]: the recording, whose
 * envelope is computed and kept as clip 0's; pcm = NULL: the envelope of the
 * last recording given here or transcribed as clip 0 with the feature on
 * (none yet: WMI_E_INVALID_ARG).  The single-window calls
 * (wmi_decode_timestamps*) leave t0 / t1 at -1: pass their records here. */
int wmi_token_times(wmi_context *ctx, const float *pcm, size_t n_samples, int64_t seek, int64_t t0, int64_t t1,
                    wmi_token_data *tokens, int n);

/* ---- token times from cross-attention alignment (DTW) --------------------- */

/* What OpenAI's word_timestamps (find_alignment) and whisper.cpp's
 * dtw_token_timestamps do: the text tokens of a finished window are
 * teacher-forced through the decoder once more, the cross-attention of
 * selected heads is turned into a cost matrix and dynamic time warping finds
 * each token's first audio frame.  Inputs: an encoded clip of T encoder
 * frames, a prompt P of p >= 1 ids, text ids x_0 .. x_{n-1} (n >= 1, p + n <=
 * n_text_ctx), M frames of real audio (1 <= M <= T), A selected (layer, head)
 * pairs (1 <= A <= 32) in the caller's order, an odd median width w in
 * [1, 15], h = w / 2.
 *   S1  Scores.  F = P ++ x is fed at positions 0 .. p+n-1; s[a][i][j], j < T,
 *       is the f32 the cross-attention softmax of layer l_a, head h_a takes as
 *       its input for key j at position i (all scaling applied), bit for bit.
 *   S2  w32[a][i][j] = (float)(exp((double)s - m) / Z) for j < M, m the maximum
 *       and Z the double sum over j < M.
 *   S3  Per (a, j), over all i in [0, p+n), in double: mu = mean(w32), sd =
 *       sqrt(mean((w32 - mu)^2)); z32 = (float)((w32 - mu) / sd), 0 where sd = 0.
 *   S4  Median along j, width w, reflect padding without edge repeat (-k -> k,
 *       M-1+k -> M-1-k): the h-th order statistic of the w values.  Applied
 *       only if M > h, else z32 stays.
 *   S5  Rows r = 0 .. n, row r = position p-1+r (it predicts x_r; row n what
 *       follows the text): c = -(1/A) * the sum over a = 0 .. A-1, in that
 *       order, in double, of the filtered value; Cq[r][j] = (int32) rint(c *
 *       65536), clamped to +-2^30.
 *   S6  DTW in int64, exact.  R = n+1 rows, M columns; D[0][0] = 0, the rest of
 *       row 0 and column 0 +inf.  For i = 1..R, j = 1..M: c0 = D[i-1][j-1], c1 =
 *       D[i-1][j], c2 = D[i][j-1]; t = 0 if c0 <= c1 and c0 <= c2, else 1 if
 *       c1 <= c2, else 2; D[i][j] = Cq[i-1][j-1] + c_t.  Backtrace from (R, M):
 *       0 -> (i-1, j-1), 1 -> (i-1, j), 2 -> (i, j-1), until (0, 0).  f[r] = the
 *       smallest column of the path in row r (0-based).  A true minimum with
 *       this tie order; OpenAI's dtw_cpu takes branch 2 on a c0 == c1 tie even
 *       when c2 is larger, and that quirk is not restated here.
 *   S7  Times in 10 ms units, W the window's start in mel frames: token x_k
 *       gets t0 = W + 2 f[k], t1 = W + 2 f[k+1].
 * Summation orders in S2, S3 are the kernels' own (a last-bit matter of the
 * float front end); from Cq on every step is integer and exact.
 *
 * wmi_set_dtw: the head table is `heads` (n_heads (layer, head) pairs,
 * copied), or with n_heads = 0 and n_top > 0 every head of the last n_top
 * text layers in (layer, head) order (whisper.cpp's N_TOP_MOST); preset lists
 * per released model are the caller's to pass.  enable != 0: every later
 * wmi_transcribe / wmi_transcribe_audio and their _batch forms aligns each
 * window's accepted result after it is committed, whatever beam size, fallback
 * attempt, rules or prompt produced it: x = the window's text tokens (id < eot)
 * over all its segments in order (none: no pass), P = [sot (, language, task)]
 * ++ [not] (no <|prev|>, no earlier text, no initial prompt), M = max(1,
 * (min(n_len - seek, 2T) + 1) / 2); one pass of p + n decoder steps on the
 * kernel chain and one synchronisation a window.  enable 0 (default, also
 * params = NULL: {0, 0, NULL, 0, 7}): every call runs exactly the kernels and
 * code objects it ran before.  WMI_E_INVALID_ARG: a pair outside the model, a
 * duplicate pair, more than 32 pairs (also through n_top), n_top above the
 * text layers, an even width or one outside [1, 15], enable with an empty
 * table.  Holds until changed. */
typedef struct wmi_dtw_params {
    int32_t enable;          /* 0 (default, also params = NULL) */
    int32_t n_top;           /* used when n_heads == 0: every head of the last n_top text layers */
    const int32_t *heads;    /* n_heads (layer, head) pairs, copied */
    int32_t n_heads;
    int32_t medfilt_width;   /* odd, 1..15; OpenAI: 7 */
} wmi_dtw_params;
typedef struct wmi_dtw_time { int64_t t0, t1; } wmi_dtw_time;
int wmi_set_dtw(wmi_context *ctx, const wmi_dtw_params *params);
/* S1 - S6 for encoded clip `clip` under the table and width set (enabled or
 * not; an empty table: WMI_E_INVALID_ARG): frames[r] = f[r], r = 0 .. n_text.
 * WMI_E_INVALID_ARG: n_prompt or n_text < 1, n_prompt + n_text > n_text_ctx,
 * n_frames outside [1, T], an id outside the vocabulary, no encode yet.  The
 * pass overwrites the decoder's self-attention cache and step state. */
int wmi_align_tokens(wmi_context *ctx, int clip, const int32_t *prompt, int n_prompt, const int32_t *text, int n_text,
                     int n_frames, int32_t *frames /* [n_text + 1] */);
/* S6 alone, on the device and on the host (no context, no device): first[r] =
 * f[r].  rows or cols < 1, rows > 513 or cols > 1500: WMI_E_INVALID_ARG. */
int wmi_dtw_path(wmi_context *ctx, const int32_t *cost, int rows, int cols, int32_t *first /* [rows] */);
int wmi_dtw_path_host(const int32_t *cost, int rows, int cols, int32_t *first);
/* One entry per token of segment i of recording clip, parallel to
 * wmi_get_segment_tokens_of (pieces under max_len carry their tokens' times):
 * S7 for a text token, -1 / -1 for any other token and for every token while
 * the feature is off.  *n = the count; WMI_E_NO_SPACE if cap is below it. */
int wmi_get_segment_dtw_of(const wmi_context *ctx, int clip, int i, wmi_dtw_time *out, size_t cap, int32_t *n);

/* ---- audio of any format: downmix, conversion, resampling on the device --- */

/* A clip is N = n_frames frames of C = channels interleaved samples at R =
 * sample_rate Hz, s16 or f32 (what wmi_read_wav returns for a file: its
 * samples, n_samples / channels frames, rate and channels).  The raw samples go
 * to the device once; these steps run there and leave y, 16 kHz mono f32, in
 * the buffer the mel kernels read.  Each output is stated so that any
 * summation order, tile shape or chunking gives the same bits.
 *   1  Mono x_i, f32, i in [0, N).  s16: x_i = (float)((double)S_i / (32768.0
 *      * C)), S_i the integer sum of the frame's channels (C = 1: exactly
 *      wmi_pcm16_to_f32).  f32: C = 1 the sample unchanged, else x_i =
 *      (float)((sum over c ascending of (double)s_ic) / (double)C).
 *   2  Plan.  g = gcd(R, 16000), L = 16000 / g, M = R / g; Z = 64, K =
 *      ceil(Z max(L, M) / L); a phase has 2K taps.  Accepted: 4000 <= R <=
 *      384000 with L <= 640 (8000, 11025, 12000, 16000, 22050, 24000, 32000,
 *      44100, 48000, 88200, 96000, 176400, 192000 among them; the largest
 *      table, for 11025, has 81,920 entries); any other rate is
 *      WMI_E_UNSUPPORTED.  R = 16000: L = M = 1, no filter, y = x.
 *   3  Taps h[ph][j], ph in [0, L), j in [0, 2K), computed in double on the
 *      host, stored f32: c = 0.95 min(1, L / M), d = (j - K + 1) - ph / L,
 *      h = c sinc(c d) w(d / K); sinc(t) = sin(pi t) / (pi t), 1 at t = 0;
 *      w(r) = I0(10 sqrt(1 - r^2)) / I0(10) for |r| < 1, else 0; I0(x) = the
 *      sum over k of ((x / 2)^k / k!)^2, ascending until a term falls below
 *      2^-60 of the sum.  Each phase row is divided by its own sum in double,
 *      then rounded to f32.
 *   4  Output.  N_out = floor((N L + M - 1) / M).  For n in [0, N_out): p =
 *      n M (64-bit), i0 = p / L, ph = p mod L; s_r = the sum over j = r (mod
 *      4), ascending, of (double)h[ph][j] * (double)x[i0 + j - K + 1], x = 0
 *      outside [0, N); y_n = (float)((s_0 + s_1) + (s_2 + s_3)).  (An f32 x
 *      f32 product is exact in double, so contraction changes no bit.)
 * Each clip has its own format.  Times (segments, token timestamps, seek)
 * are those of y, which is real time; wmi_set_token_timestamps works on y and
 * its 2^26 bound applies to N_out; after wmi_transcribe_audio,
 * wmi_token_times(pcm = NULL) uses that recording.  A clip of 16 kHz, mono,
 * f32 takes exactly the upload of the float entry points (no kernel).
 * WMI_E_INVALID_ARG: channels outside [1, 8], a sample type other than the
 * two, data = NULL with frames, n_frames above 2^31 - 1; WMI_E_UNSUPPORTED: a
 * rate outside the plan.  A failed call leaves the context's clips as they
 * were.  Raw input passes through a bounded device staging buffer in chunks
 * of at most 2^22 frames (WMI_AUDIO_CHUNK = frames overrides, read once per
 * context) plus K-frame halos.  With WMI_CHECKSUMS=1 the samples checksum is
 * taken over y, copied back. */
enum wmi_sample_type { WMI_SAMPLE_F32 = 0, WMI_SAMPLE_S16 = 1 };
typedef struct wmi_audio {
    const void *data;
    size_t n_frames;
    int32_t sample_rate, channels, sample_type;
} wmi_audio;
/* wmi_pcm_to_mel_batch / wmi_stage_pcm / wmi_transcribe / wmi_transcribe_batch on y */
int wmi_audio_to_mel_batch(wmi_context *ctx, int n_clips, const wmi_audio *clips);
int wmi_stage_audio(wmi_context *ctx, int n_clips, const wmi_audio *clips);
int wmi_transcribe_audio(wmi_context *ctx, const wmi_audio *clip, int max_tokens, int32_t *n_segments);
int wmi_transcribe_audio_batch(wmi_context *ctx, int n_clips, const wmi_audio *clips, int max_tokens,
                               int32_t *n_segments);
/* The 16 kHz mono samples clip holds (whichever entry point loaded it); *n =
 * their count; WMI_E_NO_SPACE if cap is below it (out may be NULL to ask). */
int wmi_get_pcm(const wmi_context *ctx, int clip, float *out, size_t cap, size_t *n);
/* Device time of the conversion in the last audio call (hipEvents) and the
 * clips it ran a kernel for (0 for clips that are 16 kHz mono f32). */
int wmi_get_audio_timing(const wmi_context *ctx, float *convert_ms, int32_t *n_converted);
/* Host only, no context, no device: the plan (L, M, K), the table [L][2K]
 * (*n = its entries; WMI_E_NO_SPACE if cap is below; h may be NULL to ask)
 * and N_out.  Any of the out pointers may be NULL. */
int wmi_resample_plan(int32_t sample_rate, int32_t *L, int32_t *M, int32_t *K);
int wmi_resample_taps(int32_t sample_rate, float *h, size_t cap, size_t *n);
int wmi_resampled_length(int32_t sample_rate, size_t n_frames, size_t *n_out);

/* ---- chunked long-form transcription ---------------------------------- *
 * One recording across the decoder rows.  wmi_transcribe walks a recording
 * window by window, every seek waiting for the window before it: one decoder
 * row.  With chunking on, wmi_transcribe_batch / wmi_transcribe_audio_batch
 * cut every recording at quiet places into chunks and decode the chunks as
 * the rows of the rounds.
 *
 * A chunk of recording c is a frame span [s, e), 0 <= s < e <= n_len, in
 * 10 ms mel frames (n_len = n_samples / 160 of the 16 kHz mono samples y).
 * It is a virtual recording: its own seek (from s), its own end e, its own
 * text context, its own fallback attempt ordinal and its own segment and
 * window lists; wherever the loop uses n_len (the window's class, the
 * fallback's judge, the DTW pass's M), e stands.  Times stay absolute in the
 * recording.  A chunk's windows take the recording's mel, normalised over
 * the whole recording, for frames [seek, min(seek + window, e)) and zero from
 * there on, which is what a window past the recording's end gets.
 *
 * Defining property: chunk [s, e) yields the segments the loop yields for a
 * recording whose normalised mel is the first e frames of this recording's,
 * started at seek s, under the same settings (context per wmi_set_no_context
 * / wmi_set_batch_context, language, task, fallback, rules, initial prompt);
 * whichever other chunks or recordings share the rounds, in any order.  The
 * recording's result is its chunks' segments in chunk order; window infos
 * likewise, first_segment renumbered.
 *
 * The built-in plan (exact, integer).  N = samples, P = the running sum of
 * the energy envelope of the token-level timestamps (P[k], k in [0, N],
 * uint64), Cmin <= Cmax and h in frames.  For a frame boundary k
 *     S_k = P[min(160 (k + h), N)] - P[160 max(k - h, 0)]
 * (the energy of h frames each side of the cut).  s_0 = 0; given s_i: if
 * n_len - s_i <= Cmax the last chunk is [s_i, n_len); else s_{i+1} is the k
 * in [s_i + Cmin, s_i + Cmax] of smallest S_k, of equal ones the largest k,
 * and the chunk is [s_i, s_{i+1}).  A recording of 0 frames has no chunk.
 * A recording of more than 2^26 samples is WMI_E_UNSUPPORTED under the plan.
 * Silent chunks are not dropped (the fallback's no-speech rule skips silent
 * windows); a caller with a voice-activity detector passes spans. */
typedef struct wmi_chunk_params {
    int32_t enable;        /* 0 (default, also params = NULL) */
    int32_t max_frames;    /* Cmax; 0 = the window (2 * the audio context in force at the call) */
    int32_t min_frames;    /* Cmin; 0 = Cmax / 2 (at least 1) */
    int32_t smooth_frames; /* h; 0 = 10 */
} wmi_chunk_params;
/* With enable != 0, wmi_transcribe_batch and wmi_transcribe_audio_batch (one
 * recording included) schedule the chunks of all recordings over the rounds
 * in (recording, chunk) order, a freed row taking the next waiting chunk.  A
 * round holds at most min(8, max_clips) rows: eight rows for one recording
 * need a context of max_clips = 8.  WMI_LANG_AUTO: a recording's language is
 * the one detected on its chunk 0's first window (chunk 0 is always in a
 * round no later than its siblings).  Under wmi_set_batch_context(1) each
 * chunk carries text context within itself, seeded by the initial prompt as
 * a recording is.  Token timestamps and DTW work per chunk (the recording's
 * envelope, absolute times, M from the chunk's end).  A beam size above 1
 * stays WMI_E_UNSUPPORTED.  wmi_transcribe and wmi_transcribe_audio ignore
 * the setting.  enable 0: every call runs exactly the kernels it ran before.
 * WMI_E_INVALID_ARG: a negative field, min_frames > max_frames (checked again
 * at the call once 0 has been resolved), smooth_frames > 100, max_frames >
 * 2^20.  Holds until changed. */
int wmi_set_chunking(wmi_context *ctx, const wmi_chunk_params *params);
/* Caller's spans for recording `clip` (-1: every clip) in later chunked calls, instead of the plan:
 * n (start, end) frame pairs, ascending, non-overlapping, start < end; ends are clipped to n_len at the
 * call, spans at or past n_len dropped; audio between spans is not transcribed.  n = 0: back to the plan.
 * WMI_E_INVALID_ARG: spans out of order, overlapping, empty or negative, clip outside [-1, max_clips). */
int wmi_set_chunk_spans(wmi_context *ctx, int clip, const int64_t *spans, int n);
/* Chunk i of recording `clip` in the last chunked call: its span, its
 * segments [first_segment, + n_segments) in the _of getters' list and its
 * window infos [first_window, + n_windows) (0 windows without the fallback).
 * The count is 0 after a call with chunking off. */
typedef struct wmi_chunk_info { int64_t start, end; int32_t first_segment, n_segments, first_window, n_windows; } wmi_chunk_info;
int wmi_get_chunk_count(const wmi_context *ctx, int clip, int32_t *n);
int wmi_get_chunk(const wmi_context *ctx, int clip, int i, wmi_chunk_info *out);
/* The plan alone: on the device for loaded recording `clip` (computes and keeps its envelope), and on
 * the host from P (no context, no device).  out[cap] (start, end) pairs, *n their count; WMI_E_NO_SPACE.
 * Both use the parameters of wmi_set_chunking / params whatever `enable` is (params NULL: the defaults);
 * `window` is the frames a window (2 * the audio context), used where max_frames is 0. */
int wmi_plan_chunks(wmi_context *ctx, int clip, int64_t *out, size_t cap, int32_t *n);
int wmi_plan_chunks_host(const uint64_t *P, size_t n_samples, const wmi_chunk_params *params, int window,
                         int64_t *out, size_t cap, int32_t *n);

/* ---- device-resident benchmark path --------------------------------- */

/* Upload n_clips PCM clips to HBM once (untimed). */
int wmi_stage_pcm(wmi_context *ctx, int n_clips, const float *const *pcm, const size_t *n_samples);
/* mel -> encode -> cross-KV -> decode (n_decode tokens, EOT suppressed) on
 * the staged clips; token ids stay on the device until wmi_get_tokens. */
int wmi_run_staged(wmi_context *ctx, int mel_offset, int n_decode);
/* Same with beam search of beam_size (EOT suppressed, exactly n_decode tokens). */
int wmi_run_staged_beam(wmi_context *ctx, int mel_offset, int n_decode, int beam_size);
int wmi_get_tokens(const wmi_context *ctx, int32_t *tokens, size_t cap, int32_t *n_per_clip);
int wmi_get_timings(const wmi_context *ctx, wmi_timings *out);
/* Block until all work queued on the context's stream is done. */
int wmi_sync(wmi_context *ctx);

/* Re-launch one kernel of the last pipeline call `iters` times between HIP
 * events on the context stream (bench.py's live roofline measurement).
 * which: 14 = the persistent greedy decoder over the staged clips (one launch
 * per 8-row block, as run_staged makes it; algorithmic bytes summed per step),
 * 0 = the kernel chain's logits GEMV + argmax, 1 = encoder MLP-up GEMM of
 * layer 0 (MFMA), 2 = encoder attention of layer 0, 3 = cross-K/V GEMM,
 * 15 / 16 = the beam step under the timestamp rule / under the decoding rules
 * (both kernels of either; K = wmi_set_beam_size, at generated token 1 over
 * the logits rows of the last ruled beam window, which must have run with at
 * least that many hypotheses: WMI_E_INVALID_ARG before one). */
typedef struct wmi_kernel_bench {
    float avg_us;          /* mean launch duration */
    double alg_bytes;      /* algorithmic HBM bytes per launch */
    double alg_flops;      /* algorithmic FLOPs per launch */
    char name[48];
} wmi_kernel_bench;
int wmi_bench_kernel(wmi_context *ctx, int which, int iters, wmi_kernel_bench *out);

/* Algorithmic bytes and FLOPs of one decode on a model of hparams hp (host
 * only, no device): `steps` decoder steps of `rows` rows; beam != 0: the rows
 * are hypotheses of ONE clip (its cross K/V read once a step), else clips
 * decoded in blocks of 8 rows; q5 != 0: the five q5_1 GEMV matrices (Wqkv,
 * Wo, Wco, W0, W1 = 13 n^2 weights) at 24 bytes a 32-weight block, Wcq and the
 * vocabulary f16.  Every step reads each decoder weight once (shared by the
 * block's rows), each row's cross K/V and self K/V rows [0, pos] and writes
 * its new K/V row.  wmi_bench_kernel 14 and bench.py use this one count. */
int wmi_decode_alg_bytes(const wmi_hparams *hp, int rows, int steps, int beam, int q5, double *bytes, double *flops);

/* Device self-test: the decoder computes ggml's f16 exp table entries
 * instead of looking them up; *n_mismatch = entries (of 31745 non-positive
 * f16 inputs) where the computed value differs from the host-built table. */
int wmi_selftest(wmi_context *ctx, int32_t *n_mismatch);

/* The reference's stage checksums (its debug println!s, each a sequential
 * f32 sum): out5 = {_hann (main.rs:1571-1572), the samples (:1682-1686), the
 * filters (:1688-1690), clip 0's mel before clamp_and_normalize
 * (:1645-1647), clip 0's encoder mel window (:1819-1832)}.  Computed (and
 * printed in the reference's order) only when the context was created with
 * WMI_CHECKSUMS=1; the model-only sums (_hann, filters) always. */
int wmi_get_checksums(const wmi_context *ctx, float *out5);

/* Debug: copy a device buffer of the last decode into out (min of its size
 * and bytes).  which: 0 / 1 = the kernel chain's residual-stream buffers
 * [8][n_text_state] f32, 2 = logits [8][n_vocab] f32 (the persistent
 * decoder fills them only with WMI_PERSIST_LOGITS=1), 3 = the persistent
 * decoder's exchange block (8-byte {tag, value} granules), 4-9 = decoder
 * chain scratch, 10 = this context's tuning knobs (11 int32, host copy; the
 * WMI_* environment is read once per context at wmi_init_from_file),
 * 11 = decodes re-run on the kernel chain (int32, host), 12 = the encoder
 * residual stream, 13 = every position's logits [n_text_ctx][rows][n_vocab]
 * f32 of the last greedy decode (clip b in row b) or beam search (slot s in
 * row s), on the persistent decoder or the kernel chain (contexts created
 * with WMI_LOGITS_ALL=1), 14 / 15 = the
 * last beam search's parent slots / tokens [n_text_ctx][8] int32 (its last
 * clip), 16 = the rows of 13 (int32, host: max(8, max_clips)), 17 = the
 * persistent decoder's grid per row count (int32 [9], host; -1 = not sized
 * yet, 0 = kernel chain), 18 = the encoder GELU epilogues' threshold (f32,
 * host: f16 inputs at or above it are computed, the rest read ggml's table;
 * +inf with WMI_GELU_CALC=0), 19 = the prompt of the last timestamp window
 * (wmi_transcribe / wmi_decode_timestamps; int32, host copy: the first
 * bytes / 4 tokens, entries past its length are -1; a batched window's rows
 * follow each other, [rows][n_prompt], as do the K hypothesis rows of a beam
 * window), 20 = the windows and the decoder steps of the last wmi_transcribe
 * (int64 [2], host; every attempt's steps under wmi_set_fallback, and a third
 * int64: the attempts).  13 to 15 also hold the last wmi_decode_timestamps_beam
 * or ruled beam window (19 its prompt rows), and 29 = the last ruled beam
 * window's slot histories after every step, int32 [steps][8][3] = {last id was
 * a timestamp, the one before was, the last timestamp + 1 (0: none)}
 * (WMI_E_INVALID_ARG before one ran); 13 also the last sampled or ruled window
 * (wmi_decode_timestamps_sampled, wmi_decode_timestamps_ruled, a window of
 * wmi_transcribe under wmi_set_fallback or wmi_set_decode_rules; row b in
 * row b).  21 = the conv-1 input of the last encode, [slots][2 * n_ctx + 2]
 * [up32(n_mels)] (f16 bits; f32 models: float; rows 0 and 2 * n_ctx + 1 are
 * conv-1's zero padding), 22 = the slots of the last round of
 * wmi_transcribe_batch, then the recording [8] and the mel offset [8] of each
 * slot (int32 [17], host copy; 0 slots before the first round), 23 / 24 =
 * clip 0's energy envelope E (uint32 [N]) / its running sum P (uint64 [N + 1])
 * of the token-level timestamps (WMI_E_INVALID_ARG before one was computed),
 * 25 / 26 / 27 = the last aligned pass's scores s (f32 [A][p + n][T]) / its
 * cost matrix Cq (int32 [n + 1][M]) / its path f (int32 [n + 1])
 * (WMI_E_INVALID_ARG before a pass), 28 = with WMI_ALIGN_TIMING=1 the summed
 * hipEvent ms of the passes' decoder steps, matrix kernels and DTW, and the
 * passes counted (double [4], host).  30 = the last timestamp run of rows
 * (wmi_decode_timestamps*, a window of wmi_transcribe / a round of
 * wmi_transcribe_batch without a beam): its rows B, its feed steps Pmax and
 * each row's start lo[8] = Pmax - its prompt length (int32 [10], host copy;
 * all 0: rows of equal length).  31 = the last wmi_transcribe_batch (int64
 * [7], host): its rounds, how many of them held rows of unequal prompt
 * length, and summed over the rounds the feed steps Pmax, the rows' prompt
 * lengths, the rows, the decoder steps and rows x Pmax (the last four give a
 * batch's mean prompt length and the share of its feed steps spent in
 * padding: scripts/transcribe_batch_bench.py).  In a run with rows of unequal
 * length row b's position p sits at step p + lo[b]: 13 holds its logits in slab p + lo[b], and 19 is [rows][Pmax] with -1 in the
 * lo[b] entries in front of row b's prompt.  32 = the plan of the last chunked
 * call (int64, host): per recording its chunk count, then its (start, end)
 * pairs, -1 behind the last; 33 = that call's chunks, rounds and summed rows
 * over the rounds (int64 [3], host); 34 = hipEvent ms of the last k_chunk_plan
 * launch (double, host; -1 before one).  In a chunked call 22's recording
 * column names the recording each slot's chunk belongs to.  35 = the last
 * best-of window (int32 [4], host): its candidates N, the decoder steps run
 * on one row, the decoder steps run on N rows, and the chosen candidate (-1
 * before one).  36 = every candidate of that window (int32 words, host): N,
 * M = the longest candidate's records, len [N], the records [N][M] of six
 * words {id, tid, p, pt, ptsum (f32 bits), 0} (-1 behind a candidate's end),
 * and plog [N][M] (f32 bits, 0 behind the end). */
int wmi_debug_read(const wmi_context *ctx, int which, void *out, size_t bytes);

/* ---- parity getters (copy device results into caller-owned buffers) --- */

/* ctx.mel (main.rs:1574-1578): [n_mel][n_len] f32. */
int wmi_get_mel(const wmi_context *ctx, int clip, float *out, size_t cap, int32_t *n_mel, int32_t *n_len);
/* ln_post output (main.rs:1977-1986): [n_ctx][n_audio_state] f32. */
int wmi_get_encoder_out(const wmi_context *ctx, int clip, float *out, size_t cap);
/* memory_cross_k / memory_cross_v (main.rs:2018-2030): f16 bit patterns,
 * [n_text_layer][n_ctx][n_text_state] each. */
int wmi_get_cross_kv(const wmi_context *ctx, int clip, uint16_t *k, uint16_t *v, size_t cap);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ------------------ */

/* Size of the opaque RCCL unique id blob (ncclUniqueId). */
size_t wmi_dist_id_size(void);
/* Rank 0 creates the id; every rank passes the same bytes to init. */
int wmi_dist_make_id(void *id_out);
int wmi_dist_init(wmi_context *ctx, int rank, int world, const void *id);
/* Gather every rank's token block to root 0 over RCCL (ncclGather).  A block
 * is [n_clips][1 + n_decode] int32: per clip its token count, then its tokens
 * (-1 padded) — greedy or beam, whichever the last staged run was.  Every
 * rank must have staged the same n_clips and n_decode (checked with an
 * all-reduce first: WMI_E_INVALID_ARG on every rank otherwise).  out (root
 * only; others may pass NULL) is [world][n_clips][1 + n_decode]. */
int wmi_dist_gather_tokens(wmi_context *ctx, int32_t *out, size_t cap);
/* Device-side barrier over the communicator (an RCCL all-reduce of a
 * dedicated int; gathered tokens are never touched). */
int wmi_dist_barrier(wmi_context *ctx);

#ifdef __cplusplus
}
#endif

#endif /* WHISPER_MI355X_H */
