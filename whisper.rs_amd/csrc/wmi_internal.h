// wmi_internal.h — launch interface between the C-ABI host layer
// (wmi_api.cpp) and the gfx950 kernels (wmi_kernels.hip).
//
// Every launcher enqueues on the given stream and returns hipError_t; no
// launcher allocates, copies or synchronises, so a caller may capture any
// sequence of them into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wmi {

// ---- launch-overhead probes: 0 = empty kernel, 1 = 256 x 4 KiB copy ---------
// device exp (decoder attention) vs the host-built ggml exp table, all inputs
hipError_t launch_selftest(hipStream_t s, const uint16_t *exp_tab, int n_exp, uint32_t *mismatch);

// ---- mel frontend (main.rs:1486-1671) ---------------------------------------
// Constant tables built on the host with the reference's exact f32 formulas
// (main.rs:1495, 1537, 1568), uploaded once.
struct MelTables {
    float hann[400];
    float c400[200], s400[200], c200[100], s200[100], c100[50], s100[50], c50[25], s50[25];
    float dc[625], ds[625];
};
static_assert(sizeof(MelTables) % 16 == 0, "k_mel_frames copies MelTables in 16-byte chunks");

// frames -> raw log10 mel [n_mel][n_len] + per-clip ordered-uint max.
// pcm: n_clips pointers (device) with n_samples each (device arrays).
hipError_t launch_mel_frames(hipStream_t s, const MelTables *tabs, const float *filt_t /*[201][n_mel]*/, int n_mel,
                             const float *const *pcm, const int64_t *n_samples, float *mel, int64_t mel_stride,
                             const int64_t *n_len, int64_t max_len, uint32_t *mel_max, int n_clips,
                             const float *filt_c /* compact bank (wmi_api.cpp), or null: LDS copy of filt_t */, int n_fc);
constexpr int MEL_FC_MAX = 4096;  // floats of the compact filterbank k_mel_frames keeps in LDS
// the state a decode run starts from, in one launch instead of a host copy
// and five memsets (each a separate ~5 us fill kernel): zero `n` byte ranges
// (4-byte aligned, sizes multiple of 4) and write feed[0..n_feed) to dfeed
struct ResetArgs {
    void *ptr[8];
    size_t bytes[8];
    int n;
    int32_t *dfeed;
    int n_feed;
    int32_t feed[64];
};
hipError_t launch_dec_reset(hipStream_t s, const ResetArgs &a);
// clamp_and_normalize in place on mel.
hipError_t launch_mel_norm(hipStream_t s, float *mel, int64_t mel_stride, int n_mel, const int64_t *n_len,
                           int64_t max_len, const uint32_t *mel_max, int n_clips);
// mel window (main.rs:1816-1833) -> conv1 input, f16 time-major, zero-padded
// by one frame at each end and to Cp channels: X[b][T2 + 2][Cp].  With src /
// off (device arrays [n_clips]) encoder slot b takes the window of recording
// src[b] at frame off[b] (n_len[src[b]] frames) instead of clip b's at
// mel_offset: the rows of a batched transcription sit at different seeks.
hipError_t launch_mel_window(hipStream_t s, const float *mel, int64_t mel_stride, int n_mel, const int64_t *n_len,
                             int mel_offset, int T2, int Cp, uint16_t *xconv, int n_clips,
                             float *xconv32 = nullptr, uint16_t *g1 = nullptr, int n = 0,
                             const int32_t *src = nullptr, const int32_t *off = nullptr);

// ---- LayerNorm (ggml norm + mul(repeat(w)) + add(repeat(b))) ----------------
hipError_t launch_layernorm(hipStream_t s, const float *x, int rows, int n, const float *w, const float *b,
                            uint16_t *y16, float *y32);

// ---- MFMA GEMM: C[M][N] = A[M][K] * B[N][K]^T, f16 in, f32 accumulate -------
enum GemmEpi {
    EPI_F32 = 0,        // out32[m][n] = acc + bias
    EPI_RESID = 1,      // out32[m][n] = (acc + bias) + out32[m][n]
    EPI_GELU16 = 2,     // out16[m][n] = gelu_tab[f16(acc + bias)]
    EPI_QKV = 3,        // q/k [b][h][Tp][64], vt [b][h][64][Tp]   (acc + bias) -> f16
    EPI_CONV1 = 4,      // out16[b][t + 1][n] = gelu_tab[f16(acc + bias)]  (padded time-major)
    EPI_CONV2PE = 5,    // out32[b*T + t][n] = pe[t][n] + gelu_tab[f16(acc + bias)]
    EPI_CROSSKV = 6,    // K: f16(acc * kscale), V: f16(acc + bias) -> [l][b][T][ns]
};

// Tuning knobs of one context (WMI_* environment variables read at
// wmi_init_from_file).  Kernel-argument structs carry a pointer to their
// context's copy; a null pointer means the defaults below.
struct Tune {
    int logits_cap = 512;   // WMI_LOGITS_CAP: chain logits grid cap
    int xattn_rows = 1;     // WMI_XATTN_ROWS: beam rows share cross-attention phase A (1 auto, 2 always, 0 never)
    int graph_steps = 8;    // WMI_GRAPH_STEPS: chain decoder steps per captured graph
    int enc_attn_nw = 0;    // WMI_ENC_ATTN_NW: 32-query blocks (four key-part waves each) per k_attn_enc4 workgroup (0 auto, 1, 2, 4)
    int gemm_g = 1;         // WMI_GEMM_G: large-M encoder GEMMs on k_gemm_g (LDS-DMA staging); 0: k_gemm
    // WMI_MEL_G=0: the dense-filterbank mel layout (4 two-frame waves, LDS
    // copy of the whole [201][n_mel] bank) that a file whose bank has more
    // than MEL_FC_MAX non-zero weights takes anyway; tested bitwise equal
    int mel_g = 1;
    int epi_staged = 1;     // WMI_GEMM_EPI: GEMM epilogues through LDS, 16 / 8-byte stores (0: per-lane 2 / 4-byte stores)
    int gelu_calc = 1;      // WMI_GELU_CALC: encoder GELU epilogues compute the table's values above the scanned threshold (0: table only)
    int gemm_p = 1;         // WMI_GEMM_P: one-clip encoder GEMMs on k_gemm_p (LDS-DMA ring); 0: k_gemm
    int gemm32_tile = 0;    // WMI_GEMM32_TILE: k_gemm32 tile of f32 files (0 auto: 128 x 128 from GEMM32_T128_MIN_TILES tiles; 64; 128)
};
// (fixed since round 5; their alternatives measured slower and are removed:
// chain logits grid cap at K <= 512, cooperative chain cross-attention up to
// 512 workgroups, k_gemm_g from 240 128 x 128 tiles)
constexpr int CHAIN_LOGITS_CAP2 = 1024, CHAIN_COOP_MAX = 512, GEMM_G_MIN_TILES = 240;
// k_gemm32 (f32 files) takes its 128 x 128 tile from this many 128 x 128 tiles
// (a rule of its own: GEMM_G_MIN_TILES picks between two f16 kernels)
constexpr int GEMM32_T128_MIN_TILES = 240;
extern const Tune kTuneDefault;
inline const Tune &tune_of(const Tune *t) { return t ? *t : kTuneDefault; }

struct GemmArgs {
    const Tune *tune;   // context knobs (null: defaults)
    const uint16_t *A;  // plain: [M][lda]; conv: X[b][Tin + 2][Cp]
    const uint16_t *B;  // [N][K]
    const float *bias;  // [N] or null
    int M, N, K, lda;
    // implicit-GEMM conv: row m -> (b = m / Tout, t = m % Tout); k -> (tap, c)
    int conv, conv_stride, conv_tin, conv_cp, conv_tout;
    float *out32;
    uint16_t *out16;
    int ldo;
    const uint16_t *gelu_tab;
    float gelu_min = __builtin_huge_valf();  // GELU epilogues compute inputs >= gelu_min (gelu_bits), +inf: table only
    const float *pe;    // EPI_CONV2PE: [T][N]
    int T;              // rows per clip (for b/t split)
    // EPI_QKV
    uint16_t *q, *k, *vt;
    int Tp, n_state;
    // EPI_CROSSKV
    uint16_t *ck, *cv;
    int n_clips;
    float kscale;
    // f32 models (ggml f32 x f32 mul_mat / conv: neither operand rounded):
    // B32 = f32 weights [N][K] selects the f32 MFMA GEMM (wmi_f32.hip); its
    // A operand is A32 (f32) when set, else A (f16: GELU-table outputs, exact)
    const float *A32, *B32;
    int epi_staged;     // set by launch_gemm from the context's knob (Tune::epi_staged)
};
hipError_t launch_gemm(hipStream_t s, int epi, const GemmArgs &a);
// exhaustive scan of gelu_bits' computed path against the table: maxord[0] =
// the largest ord_f32(f) over f16 inputs f whose computed value differs
// (0 if none), maxord[1] = the inputs checked (the caller zeroes both)
hipError_t launch_gelu_scan(hipStream_t s, const uint16_t *gelu_tab, uint32_t *maxord);
hipError_t launch_gemm32(hipStream_t s, int epi, const GemmArgs &a);  // wmi_f32.hip

// ---- encoder self-attention (ggml flash_attn_f16 semantics, exact softmax) --
struct AttnArgs {
    const Tune *tune;  // context knobs (null: defaults)
    const uint16_t *q, *k, *vt;  // [b][h][Tp][64], vt [b][h][64][Tp]
    uint16_t *out;               // [b*T + t][n_state]
    float *out32;                // or f32 output (f32 models: Wo takes it unrounded)
    const uint16_t *exp_tab;     // f16 exp table, negative half
    int n_exp;                   // entries in exp_tab
    int T, Tp, H, n_state, n_clips;
    float scale;
};
hipError_t launch_attn_enc(hipStream_t s, const AttnArgs &a);
// k_attn_enc4 query blocks per workgroup, as launch_attn_enc picks them
int attn_enc_nw(int T, int H, int n_clips, int nw_knob);
int attn_enc_kq(int T, int H);

// ---- decoder step -----------------------------------------
struct DecState {          // device-resident, advanced by the kernels
    int32_t pos;           // position of the token being processed
    int32_t pad[3];
};

enum DecEpi { DEC_QKV = 0, DEC_Q = 1, DEC_GELU = 2, DEC_RESID = 3, DEC_LOGITS = 4 };

struct DecGemvArgs {
    const Tune *tune;  // context knobs (null: defaults)
    const float *x;          // LN input [B][K] f32 (ln != null)
    const float *ln_w, *ln_b;
    const uint16_t *xin16;   // non-LN input [B][K] f16
    const float *parts;      // or: split-key attention partials [B][n_parts][K] f32, summed in order
    int n_parts;
    const uint16_t *W;       // [N][K]
    const uint8_t *Wq5;      // or q5_1 blocks repacked (nibbles [N][K/2], then {5th bits, d | m << 16} [N][K/32])
    const float *bias;       // [N] (null for logits)
    int N, K, B;
    float qscale;            // (n/h)^-0.25
    // outputs
    uint16_t *out16;         // DEC_Q / DEC_GELU / DEC_QKV(q): [B][ldo]
    float *out32;            // DEC_RESID: x [B][N]; DEC_LOGITS: logits [B][N]
    int ldo;
    uint16_t *kcache, *vcache;  // DEC_QKV: [B][n_text_ctx][n]
    int n_text_ctx;
    const DecState *st;
    const uint16_t *gelu_tab;
    unsigned long long *amax;   // DEC_LOGITS: packed argmax, AMAX_SHARDS shards per clip
    int suppress_id;            // DEC_LOGITS: id excluded from argmax (-1 none)
    DecState *st_advance;       // DEC_LOGITS: pos += 1 (block 0)
    // embed prologue (IN = 3, first layer): x = te[tok] + pe[pos], tok from
    // feed[b][pos] while pos < feed_len, else from the previous step's argmax
    const uint16_t *te;
    const float *pe;
    const int32_t *feed;
    int feed_len, feed_stride;
    int32_t *tokens_out;        // [B][out_stride], token of pos - feed_len
    int out_stride;
    float *x_out;               // residual stream written by block 0
    const int32_t *beam_tok;    // beam search: token of row b past the prompt (BeamState::tok), else null
    // f32 models: W32 = f32 weights [N][K] (W / Wq5 unused), te32 = f32 token
    // embedding for IN = 3; activations stay f32 into the dot (wmi_f32.hip)
    const float *W32, *te32;
    // ragged rows (DESIGN.md "Text context in the batch"): row b's prompt starts
    // at step lo[b], its position embedding is pe[max(pos - lo[b], 0)] (null: 0)
    const int32_t *lo;
};
constexpr int AMAX_SHARDS = 64;
constexpr int DEC_ROWS = 8;  // decoder rows per step: clips (greedy) or beam hypotheses
hipError_t launch_dec_gemv(hipStream_t s, int epi, const DecGemvArgs &a);
hipError_t launch_dec_gemv32(hipStream_t s, int epi, const DecGemvArgs &a);  // wmi_f32.hip

struct DecAttnArgs {
    const Tune *tune;  // context knobs (null: defaults)
    const uint16_t *q;       // [B][n]
    const uint16_t *K, *V;   // per clip: rows of n (clip_stride elements apart)
    int64_t clip_stride;     // elements between clips in K/V
    int M_fixed;             // >0: fixed key count (cross); 0: pos + 1 (self)
    int mk;                  // self-attention: key capacity of this launch (64/128/256/512 >= pos + 1)
    const DecState *st;
    float *S;                // scores [B][H][s_stride]
    int s_stride;
    float *cmax;             // per-chunk max [B][H][n_chunks]
    float *opart;            // partial outputs [B][n_chunks][n]
    int n_chunks;            // 128-key chunks in the grid (covers the max M)
    const uint16_t *exp_tab;
    int n_exp, H, n, B;
    unsigned long long *reset_amax;  // self-attn: zero these B * AMAX_SHARDS words (block 0)
    // cross-attention: q = f16((Wq LN(x) + bq) * qscale) computed in the score kernel
    const float *x, *ln_w, *ln_b;
    const uint16_t *Wq;
    const float *bq;
    float qscale;
    // cooperative single-kernel cross-attention: per (clip, head) exchange
    // words for this layer, zeroed at the start of every decode run
    struct XSync *sync;
    uint32_t *err;           // set to 1 if an exchange spin times out
    // beam search: self-attention reads key/value row j < pos of decoder row b
    // from cache slot kv_src[b * kv_src_stride + j] (its hypothesis' history);
    // cross-attention rows b share clip b / clip_div
    const int32_t *kv_src;
    int kv_src_stride;
    int clip_div;
    // self-attention with the output projection fused (Wo null: o_h -> opart):
    // head h writes Wo[:, h*64:(h+1)*64] . f16(o_h) to wo_parts[b][h][n]
    const uint16_t *Wo;
    float *wo_parts;
    // cross-attention prologue (res_parts non-null): x_out = (res_bias +
    // sum_h res_parts[b][h]) + x, the fused self-attention's residual update,
    // then LN(x_out); block (0, 0, b) stores x_out[b] (x_out != x: ping-pong)
    const float *res_parts, *res_bias;
    float *x_out;
    // self-attention of ragged rows: row b attends to keys [min(lo[b], pos), pos]
    // only (k_dec_self_attn<MK, true>; null: every key, the plain instances)
    const int32_t *lo;
};
// exchange words of one (layer, clip, head) for the cooperative kernel
struct XSync {
    uint32_t cnt;            // monotonic arrival counter (target (pos + 1) * n_chunks)
    uint32_t pad[15];
};
hipError_t launch_dec_attn(hipStream_t s, const DecAttnArgs &a);

// ---- beam search (config C5; semantics in oracle/wmi_oracle.h) -------------
constexpr int BEAM_MAX = 8, BEAM_NS = 16, BEAM_TK = BEAM_MAX + 1;
struct BeamPart {            // one vocabulary split of one row
    float m;                 // split max
    float pad;
    double sum;              // sum exp(logit - m) over the split
    float val[BEAM_TK];      // split top-(K+1) by (value desc, id asc)
    int32_t id[BEAM_TK];
};
struct BeamState {
    int32_t n_active, n_fin, done, n_steps;
    double score[BEAM_MAX];      // cumulative log-probability of active slot s
    int32_t tok[BEAM_MAX];       // token slot s feeds at the next step
    int32_t fin_t[BEAM_MAX], fin_beam[BEAM_MAX];
    double fin_score[BEAM_MAX];
};
struct BeamArgs {
    const float *logits;     // [K][V]
    int V, K, suppress_id, eot, feed_len, max_tokens, tctx;
    const DecState *st;
    BeamPart *parts;         // [K][BEAM_NS]
    BeamState *bs;
    int32_t *kv_src;         // [K][tctx]
    int32_t *hist_parent, *hist_tok;  // [max_tokens][BEAM_MAX]
};
hipError_t launch_beam_step(hipStream_t s, const BeamArgs &a);

// ---- timestamp sampling (whisper.cpp-1.0.3 whisper_sample_best /
// whisper_sample_timestamp semantics, restated in oracle/pyoracle.py) --------
struct TsRec {               // WhisperTokenData (main.rs:317-331) as sampled
    int32_t id, tid;
    float p, pt, ptsum;
    int32_t pad;
};
struct TsArgs {
    const float *logits;     // [B][V]
    int V, beg, eot, sot, solm, not_, feed_len, max_rec;
    int B;                   // decoder rows (<= DEC_ROWS): one workgroup each
    const DecState *st;      // pos already advanced by the logits launch
    int32_t *tok_out;        // [B] token row b feeds at the next step
    TsRec *rec;              // [B][max_rec], record t = pos - feed_len
    int32_t *done;           // [B] != 0 once row b sampled EOT: no more records, feeds EOT
};
hipError_t launch_ts_sample(hipStream_t s, const TsArgs &a);

// ---- beam search under the timestamp rule (DESIGN.md "Beam search in
// timestamped decoding"): the rule of k_ts_sample decides each hypothesis
// row's allowed set, the beam step of k_beam_topk / k_beam_select ranks the
// rows' top-(K+1) of their sets ------------------------------------------------
struct TsBeamPart {          // one vocabulary split of one row
    float m_all, m_tx;       // max over the split's ids; over its ids < beg (-inf: none)
    float m_ts, m_tl;        // max over its ids >= beg; over the set of the timestamp list
    int32_t id_ts, pad;      // argmax over its ids >= beg, ties to the lowest id (-1: none)
    double sum_all;          // sum exp(l - m_all) over the split
    double sum_ts;           // sum exp(l - m_ts) over ids >= beg
    double sum_tl;           // sum exp(l - m_tl) over the set of the timestamp list
    double sum_a;            // sum exp(l - a_val[0]) over ids other than sot / solm / not
    float ts_val[BEAM_TK];   // top-(K+1) of ids >= beg (first generated token: ids > beg)
    int32_t ts_id[BEAM_TK];
    float a_val[BEAM_TK];    // top-(K+1) of ids other than sot / solm / not (not at the first token)
    int32_t a_id[BEAM_TK];
};
struct TsBeamArgs {
    BeamArgs b;              // (parts unused; suppress_id -1)
    int beg, sot, solm, not_;
    TsBeamPart *tparts;      // [K][BEAM_NS]
    TsRec *hist_rec;         // [tctx][BEAM_MAX] record of the token slot s took at step t
    TsRec *fin_rec;          // [BEAM_MAX] record of finished hypothesis f's EOT
};
hipError_t launch_tsbeam_step(hipStream_t s, const TsBeamArgs &a);

// ---- temperature sampling under the timestamp rule (wmi_sample.hip; DESIGN.md
// "Temperature fallback"): k_ts_sample's records and rule, the id drawn from
// the allowed set's distribution at the row's temperature -------------------
struct SampRow {             // per decoder row, in device memory (cached graphs replay the launch)
    float T;                 // 0: the argmax of the allowed set (k_ts_sample's pick)
    int32_t pad;
    unsigned long long key;  // stream key: u_t = (sm64(key + t) >> 11) * 2^-53
};
struct TsSampArgs {
    TsArgs t;
    const SampRow *rows;     // [B]
    float *plog;             // [B][max_rec] log-probability of the id under the unscaled masked distribution
    float *p_nosp;           // [B] P(solm) under the unmasked softmax of the first generated step
};
hipError_t launch_ts_sample_t(hipStream_t s, const TsSampArgs &a);
// ---- the sampler under OpenAI's decoding rules (wmi_rules.hip; DESIGN.md
// "OpenAI decoding rules"): k_ts_sample_t's conventions, the allowed set from
// the suppress bitmask and the row's history of this window ----------------
struct RuleHist {            // per decoder row, in device memory behind the rows' done words (reset with them)
    int32_t last, pen;       // the last / the last but one sampled id was a timestamp
    int32_t lts1;            // the last timestamp sampled + 1 (0: none yet)
    int32_t pad;
};
struct TsRuleArgs {
    TsSampArgs s;
    const uint32_t *m0;      // [ceil(V / 32)] bit i set: id i is masked always (M0)
    RuleHist *hist;          // [B]
    int max_initial_ts;      // first timestamp <= beg + this (< 0: no cap)
};
hipError_t launch_ts_sample_r(hipStream_t s, const TsRuleArgs &a);
// ---- best-of-N sampled windows (wmi_bestof.hip; DESIGN.md "Best-of-N sampled
// attempts"): after the prompt's last step, run on one decoder row, workgroup
// c of a.B = N draws candidate c's first token from logits row 0 with rows[c]
// and writes row c of tok_out, done, rec, plog (and hist); workgroup 0 also
// p_nosp[0].  k_ts_sample_t's first step, or with `ruled` k_ts_sample_r's
// (m0, hist and max_initial_ts are read only then) ------------------------------
hipError_t launch_bestof_fan(hipStream_t s, const TsRuleArgs &a, bool ruled);
// ---- beam search under the decoding rules (wmi_rbeam.hip; DESIGN.md "Decoding
// rules in the beam window"): k_ts_sample_r's masks per hypothesis row, each
// row's history following the beam step's parent selection; the ranking, walk
// and records of k_tsbeam_select ------------------------------------------------
struct RBeamPart {           // one vocabulary split of one row
    float m_tx;              // max over the split's text ids (< beg) of A' (-inf: none)
    int32_t pad;
    unsigned long long k_all;  // argmax key over all its ids >= beg, masked or not (0: none)
    double sum_ap;           // sum exp(l - ap_val[0]) over the split's ids of A'
    double sum_ts;           // sum exp(l - ts_val[0]) over its timestamps of A'
    float ap_val[BEAM_TK];   // top-(K+1) of A' (id -1: no such rank)
    int32_t ap_id[BEAM_TK];
    float ts_val[BEAM_TK];   // top-(K+1) of the timestamps of A'
    int32_t ts_id[BEAM_TK];
};
struct RBeamArgs {
    BeamArgs b;              // (parts unused; suppress_id -1)
    int beg;
    int max_initial_ts;      // first timestamp <= beg + this (< 0: no cap)
    const uint32_t *m0;      // [ceil(V / 32)] bit i set: id i is masked always (M0)
    RuleHist *hist;          // [BEAM_MAX] history of the hypothesis in slot s
    RBeamPart *rparts;       // [K][BEAM_NS]
    TsRec *hist_rec;         // [tctx][BEAM_MAX] record of the token slot s took at step t
    TsRec *fin_rec;          // [BEAM_MAX] record of finished hypothesis f's EOT
    int32_t *hist_tab;       // [tctx][BEAM_MAX][3] {last, pen, lts1} of slot s after step t (debug read 29)
};
hipError_t launch_rbeam_step(hipStream_t s, const RBeamArgs &a);
// ---- token-level timestamps (wmi_toktime.hip; DESIGN.md "Token-level
// timestamps"): a recording's energy envelope E [N] and its running sum
// P [N + 1], and the voice-activity pass over each segment's text tokens ------
constexpr long long TT_MAX_SAMPLES = 1ll << 26;  // (2^26 * 65 * 2^24 * 2 ns stays inside 64 bits)
// E, the tile sums (tsum: ceil(N / 1024) words of scratch) and P, three launches
hipError_t launch_energy(hipStream_t s, const float *pcm, long long N, uint32_t *E, unsigned long long *tsum,
                         unsigned long long *P);
struct VadSeg { int32_t first, m; };  // a segment's text tokens: spans [first, first + m)
struct VadArgs {
    const uint32_t *E;
    const unsigned long long *P;
    long long N;
    const VadSeg *segs;      // one workgroup each
    long long *t0, *t1;      // the spans after step B, in 10 ms units; moved in place
};
hipError_t launch_token_vad(hipStream_t s, const VadArgs &a, int n_segs);
// ---- chunked long-form transcription (wmi_chunks.hip; DESIGN.md "Chunked
// long-form transcription"; the plan is stated in the public header) ----
struct ChunkPlanRec {
    const unsigned long long *P;  // the recording's running envelope sum [N + 1] (not read while N / 160 <= Cmax)
    long long N;                  // its samples
    long long *out;               // (start, end) pairs [cap]
    int32_t *count;               // the pairs of the plan (above cap: the list is cut short)
    int32_t cap;
};
// one workgroup a recording (recs: device array [n_recs]); 1 <= Cmin <= Cmax <= 2^20, 1 <= h <= 100
hipError_t launch_chunk_plan(hipStream_t s, const ChunkPlanRec *recs, int n_recs, int Cmax, int Cmin, int h);
// launch_mel_window's slot form with slot b's window ending at frame end[b] of its recording
hipError_t launch_mel_window_end(hipStream_t s, const float *mel, int64_t mel_stride, int n_mel, const int64_t *n_len, int T2,
                                 int Cp, uint16_t *xconv, int slots, float *xconv32, uint16_t *g1, int n, const int32_t *src,
                                 const int32_t *off, const int32_t *end);
// ---- token times from cross-attention alignment (wmi_align.hip; DESIGN.md
// "Token times from cross-attention alignment"; S1 - S7 in the public header) ----
constexpr int AL_HEADS_MAX = 32, AL_WIDTH_MAX = 15;
constexpr int AL_ROWS_MAX = 513, AL_COLS_MAX = 1500;  // rows (text tokens + 1) and columns (frames) of a cost matrix
constexpr int AL_DTW_WG = 576;                        // k_dtw's workgroup: a thread a row
// bytes of k_dtw's trace: a byte a cell, diagonal by diagonal, R bytes a diagonal
constexpr size_t dtw_trace_bytes(int R, int M) { return (size_t)(R + M - 1) * (size_t)R; }
// S1 behind a layer's cross-attention launch of an aligned step (one decoder
// row): workgroup g copies head[g]'s T scores to s[slot[g]][pos][0 .. T),
// s being [A][*np][T]; nothing is written unless pos < *np <= np_max
struct AlCapArgs {
    const float *S;          // the launch's scores [H][s_stride]
    int s_stride, T;
    const DecState *st;
    const int32_t *np;       // device: positions of this pass
    int np_max;              // positions the buffer holds
    float *s;
    int n;                   // selected heads of this layer
    int16_t head[AL_HEADS_MAX], slot[AL_HEADS_MAX];
};
hipError_t launch_align_capture(hipStream_t s, const AlCapArgs &a);
// S2 - S5: s [A][Np][T] -> w [A][Np][M] (softmax, then z-score in place) -> cq [n + 1][M]; three launches
struct AlMatArgs {
    const float *s;
    float *w;
    int32_t *cq;
    int A, Np, T, M, p, n, width;
};
hipError_t launch_align_cost(hipStream_t s, const AlMatArgs &a);
// S6: first[r] = the smallest column of the path in row r; trace holds dtw_trace_bytes(R, M)
hipError_t launch_dtw(hipStream_t s, const int32_t *cq, int R, int M, uint8_t *trace, int32_t *first);
// ---- audio of any format (wmi_audio.hip; DESIGN.md "Audio front end") ----------
constexpr int AUDIO_CH_MAX = 8;                 // channels of a clip
constexpr long long AUDIO_CHUNK_MAX = 1ll << 22;  // frames of raw input on the device at a time (plus halos)
// n frames of C interleaved samples (s16 != 0: int16, else f32) at raw (16-byte aligned) -> mono f32 at out (16-byte aligned)
hipError_t launch_audio_mono(hipStream_t s, const void *raw, long long n, int C, int s16, float *out);
struct FirArgs {
    const float *x;          // mono frames [x0, x0 + xn) of the clip
    long long x0, xn, N;     // N: the clip's frames; a frame outside [0, N) or outside x is 0 and never read
    const float *h;          // taps [L][hs], a row's first 2K entries; hs a multiple of 4, h 16-byte aligned
    int L, M, K, hs;
    long long n_lo, n_hi;    // outputs [n_lo, n_hi) of the clip
    float *y;                // the clip's outputs (y[n])
};
hipError_t launch_audio_fir(hipStream_t s, const FirArgs &a);
struct NoSpeechArgs {        // a beam window's no-speech probability (row 0 of its first generated step)
    const float *logits;     // [V]
    int V, solm, feed_len;
    const DecState *st;      // pos already advanced by the logits launch
    float *p_nosp;
};
hipError_t launch_no_speech(hipStream_t s, const NoSpeechArgs &a);
// WMI_LOGITS_ALL on the kernel chain: logits [rows][V] -> all + (pos - 1) * slab
// (after the step's logits GEMV; positions outside [0, tctx) are dropped)
hipError_t launch_logits_capture(hipStream_t s, const float *logits, float *all, const DecState *st, int rows, int V,
                                 int64_t slab, int tctx);

// ---- language detection and per-clip prompts --------------------------------
// (the language token of index i is sot + 1 + i; whisper.cpp's g_lang order)
constexpr int LANG_MAX = 100;
// One wave per row of a decoder block over the logits of its [SOT] step:
// p_i = exp((double)l_i - (double)max) / sum over the n_lang language logits
// (k_ts_sample's convention), argmax by ts_key (ties: lowest index).
struct LangArgs {
    const float *logits;     // [B][V], row b = clip b0 + b
    int V, first, n_lang;    // language logits [first, first + n_lang), n_lang <= LANG_MAX
    int b0, B;
    const int32_t *is_auto;  // [max_clips] != 0: the clip's language setting is AUTO
    int32_t *lang;           // [max_clips] language the clip's prompt takes (written for AUTO clips only)
    int32_t *det;            // [max_clips] detected language
    float *p;                // [max_clips] its probability
    float *probs;            // [max_clips][n_lang]
};
hipError_t launch_lang_detect(hipStream_t s, const LangArgs &a);
// feed[b * np + i] = prompt[i], slot 1 = sot + 1 + lang[clip of row b] with
// clip = min(clip0 + b * clip_step, n_clips - 1): greedy rows are consecutive
// clips (clip_step 1), beam rows the hypotheses of one clip (clip_step 0)
struct PromptFeedArgs {
    int32_t *feed;           // [rows][np]
    int np, rows;
    int32_t prompt[8];
    int sot;
    const int32_t *lang;     // [max_clips]
    int n_lang;
    int clip0, clip_step, n_clips;
};
hipError_t launch_prompt_feed(hipStream_t s, const PromptFeedArgs &a);

struct DecEmbedArgs {
    const uint16_t *te;      // [V][n]
    const float *pe;         // [n_text_ctx][n]
    float *x;                // [B][n]
    const int32_t *feed;     // [B][feed_stride] tokens fed while pos < feed_len
    int feed_len, feed_stride;
    unsigned long long *amax;
    int32_t *tokens_out;     // [B][out_stride]
    int out_stride;
    const DecState *st;
    int n, B, record_only;
};
hipError_t launch_dec_embed(hipStream_t s, const DecEmbedArgs &a);

// ---- persistent decoder: one launch runs n_steps greedy decoder steps -------
// (wmi_persist.hip).  Every decoder step is a fixed sequence of phases; the
// workgroups of the launch (all co-resident, one per CU) hand each phase's
// outputs to the next through epoch-tagged 8-byte granules {tag, value}
// written and read with agent-scope (sc1) accesses — the data is its own flag,
// so a seam costs one write-through store plus the consumer's poll, not a
// kernel boundary (MI355X_MICROARCH.md handoff / allgather rows; measured
// 1.8 us per all-to-all seam at 256 workgroups vs 2.1 us per graph kernel
// boundary, scripts/seam_probe.hip).
struct PersistLayer {          // decoder layer weights (device pointers)
    const float *ln1_w, *ln1_b;
    const uint16_t *wqkv; const float *bqkv;   // [3n][n], bias [3n] (zero for K)
    const uint16_t *wo; const float *bo;
    const float *lnc_w, *lnc_b;
    const uint16_t *wcq; const float *bcq;
    const uint16_t *wco; const float *bco;
    const float *ln2_w, *ln2_b;
    const uint16_t *w0; const float *b0;       // [4n][n]
    const uint16_t *w1; const float *b1;       // [n][4n]
    // q5_1 repacks of wqkv, wo, wco, w0, w1 (wmi_api.cpp repack_q5), or null
    const uint8_t *wqkv5, *wo5, *wco5, *w05, *w15;
};

// exchange block layout in granules (host and device agree)
struct XLayout {
    int x1, x2, x3, q, k, v, o, xq, oc, h, s, p, a, ctl, total;
};
constexpr int PX_TASKS = 2048;   // cross-attention (row, head, chunk) tasks
constexpr int PX_GMAX = 256;     // workgroups
__host__ __device__ inline XLayout persist_layout(int n, int H, int T) {
    XLayout L{};
    int o = 0;
    const int R = 8;  // DEC_ROWS
    L.x1 = o; o += R * n;
    L.x2 = o; o += R * n;
    L.x3 = o; o += R * n;
    L.q = o; o += R * n / 2;
    L.k = o; o += R * n / 2;
    L.v = o; o += R * n / 2;
    L.o = o; o += R * n / 2;
    L.xq = o; o += R * n / 2;
    L.oc = o; o += R * n / 2;
    L.h = o; o += R * 2 * n;
    // per (row, head, 128-key sub-chunk) of the cross attention: its max m and
    // its exact exp sum S (a double as lo, hi): [R][H][ceil(T / 128)][3]
    L.s = o; o += 3 * R * H * ((T + 127) / 128);
    L.p = o; o += R * H * ((T + 127) / 128) * 64;  // 128-key P.V partials
    L.a = o; o += R * PX_GMAX * 2;
    L.ctl = o; o += 16;             // ctl[0] low word: abort flag
    L.total = (o + 15) / 16 * 16;   // whole 128-byte lines (memset size a multiple of 16 B)
    return L;
}

struct PersistArgs {
    const PersistLayer *layers;  // device array [L]
    const uint16_t *te;          // token embedding [V][n]
    const float *pe;             // positional embedding [n_text_ctx][n]
    const float *dln_w, *dln_b;  // final LayerNorm
    const uint16_t *gelu_tab;    // ggml GELU table [65536]
    float gelu_min = __builtin_huge_valf();  // phase H computes GELU of f16 inputs >= gelu_min (gelu_bits), +inf: table
    const uint16_t *exp_tab;     // ggml exp table, non-positive half [n_exp]
    int n_exp;
    const uint32_t *exp_fb;      // [64] exp fallback list (launch_exp_fallbacks), 0xffffffff-padded
    uint16_t *kcache, *vcache;   // [L][DEC_ROWS][tctx][n]
    const uint16_t *ck, *cv;     // cross K/V [L][Bt][T][n]; row b uses clip b0 + b
    int L, n, V, B, T, tctx, Bt, b0;
    int nch, cl;                 // cross-attention chunks per (row, head), keys per chunk
    float qscale;                // (n / H)^-0.25
    DecState *st;                // pos advanced by n_steps at the end
    const int32_t *feed;         // [B][feed_stride] prompt tokens
    int feed_len, feed_stride;
    int32_t *tokens_out;         // [B][out_stride] generated tokens (index pos - feed_len)
    int out_stride;
    int32_t *cur_tok;            // [8] last argmax, carried to the next launch
    int suppress_id;
    int n_steps;
    uint64_t *xg;                // exchange block (persist_layout), zeroed before a run
    uint32_t *err;               // bit 3: exchange timeout
    unsigned long long *ptrace;  // WMI_PTRACE: [n_steps][L + 1][16][2] phase-end clocks, or null
    int nres;                    // vocabulary rows per workgroup resident in LDS
    float *logits_out;           // [B][V] logits of every step (debug / teacher forcing), or null
    int64_t lg_stride;           // > 0: position p's logits at logits_out + p * lg_stride (all-step capture)
    // beam search (one step per launch; the beam kernels select between launches):
    // rows are the beam slots of clip b0, step 0 feeds cur_tok (the beam state's
    // tokens), self-attention keys j < pos come from cache row kv_src[b][j], and
    // the launch records no argmax
    int beam;
    const int32_t *kv_src;       // [B][kv_src_stride] or null
    int kv_src_stride;
    int q5;                      // GEMVs of phases A, C, G2, H, I read the layers' q5_1 repacks
    // beam launches (rows = hypotheses of one clip, n > 768): one cross-
    // attention task per (head, key chunk) covers every row (PersistArgs::nch
    // then counts the chunks of one head: H * nch tasks)
    int xshare;
    // fault injection (tests): workgroup stall_wg exits at once, as a
    // workgroup that never became resident — every other workgroup's first
    // poll of its rows runs into the bounded spin, raises the abort word and
    // err bit 3, and the grid drains (-1: none)
    int stall_wg;
    // one-row VALU logits (n = 768): the vocabulary rows past the LDS-resident
    // ones stay in registers for the whole launch (an 8-pass WSet per
    // quarter-wave slot, at most 128 rows a workgroup) instead of streaming
    // every step (0: streamed; past 128 rows the kernel streams them anyway)
    int vreg;
    // WMI_EARLY_OPERANDS (one-row greedy instances of n <= PX_EOP_NMAX): the cross
    // tasks run on workgroups H .. H + ntask - 1 (px_e_first_task) and request
    // their K / V rows, Wcq rows and LNc parameters in phase C, ahead of C's
    // poll (0: tasks on workgroups 0 .., operands requested in phase E)
    int early_ops;
    // WMI_A_OFF_B (one-row greedy instances of n <= PX_AOB_NMAX): phase A's Wqkv
    // rows lie on the workgroups from H on (px_a_off_b), and a workgroup that
    // owns none skips phase A: the H self-attention workgroups enter phase B
    // straight from the previous layer's phase I (0: the rows over all workgroups)
    int a_off_b;
    // ragged rows (multi-row instances without beam search): row b's prompt
    // starts at step lo[b]; its layer-0 position embedding is pe[max(pos -
    // lo[b], 0)] and phase B masks its keys below min(lo[b], pos) (null: 0)
    const int32_t *lo;
};
// rows per workgroup of an N-row GEMV over G workgroups, even (f16-pair outputs)
__host__ __device__ constexpr int px_rows_even(int N, int G) { return (((N + G - 1) / G) + 1) & ~1; }
// the largest divisor of kch with rows * ks <= 16 (one pass of 16 quarters)
__host__ __device__ constexpr int split_of(int kch, int rows) {
    int best = 1;
    for (int k = 1; k <= kch; ++k)
        if (kch % k == 0 && rows * k <= 16) best = k;
    return best;
}
// One-row phase-A placement: the 3n Wqkv rows over the G - H workgroups from
// H on, px_rows_even(3n, G - H) each, so that the H self-attention workgroups
// own none.  Taken only where a row's sum stays bitwise what it was and the
// GEMV takes no more passes: the split-K factor the kernel is compiled with
// (split_of at the design grid GD's rows) still fits the rows in its one
// pass, or, without split-K, the rows need no more 16-row passes than the
// partition over all G workgroups.  Else (a small grid, n = 1280, knob off)
// that partition stays.
__host__ __device__ constexpr bool px_a_off_b(bool on, int n, int H, int G, int GD) {
    if (!on || G <= H) return false;
    const int N = 3 * n, old = px_rows_even(N, G), rpw = px_rows_even(N, G - H);
    const int ks = split_of(n / 128, px_rows_even(N, GD));
    return ks > 1 ? rpw * ks <= 16 : split_of(n / 128, rpw) == 1 && (rpw + 15) / 16 <= (old + 15) / 16;
}
__host__ __device__ constexpr int px_a_rpw(bool off_b, int n, int H, int G) {
    return px_rows_even(3 * n, off_b ? G - H : G);
}
// workgroup wg's first Wqkv row (3n: it owns none)
__host__ __device__ constexpr int px_a_row0(bool off_b, int wg, int n, int H, int G) {
    const int s = off_b ? wg - H : wg, r = s * px_a_rpw(off_b, n, H, G);
    return s >= 0 && r < 3 * n ? r : 3 * n;
}
// every row of [0, 3n) owned exactly once (the workgroups' ranges follow one
// another), even starts, and with the placement taken none below workgroup H
constexpr bool px_a_rows_once(bool want, int n, int G, int GD) {
    const int H = n / 64, N = 3 * n;
    const bool ob = px_a_off_b(true, n, H, G, GD);
    if (ob != want) return false;
    int next = 0;
    for (int wg = 0; wg < G; ++wg) {
        const int r0 = px_a_row0(ob, wg, n, H, G), r1 = r0 + px_a_rpw(ob, n, H, G) < N ? r0 + px_a_rpw(ob, n, H, G) : N;
        if (r0 == N) continue;
        if ((ob && wg < H) || r0 != next || (r0 & 1) || r1 <= r0) return false;
        next = r1;
    }
    return next == N;
}
static_assert(px_a_rows_once(true, 128, 256, 256) && px_a_rows_once(true, 384, 256, 256) && px_a_rows_once(true, 512, 256, 256) &&
                  px_a_rows_once(true, 768, 256, 256) && px_a_rows_once(true, 1024, 256, 256),
              "Wqkv rows off the self-attention workgroups");
static_assert(px_a_rpw(true, 128, 2, 256) == 2 && px_a_rpw(true, 384, 6, 256) == 6 && px_a_rpw(true, 512, 8, 256) == 8 &&
                  px_a_rpw(true, 768, 12, 256) == 10 && px_a_rpw(true, 1024, 16, 256) == 14,
              "rows per workgroup of the placement");
static_assert(px_a_rows_once(false, 1280, 256, 256) && px_a_rows_once(false, 512, 192, 192) && px_a_rows_once(false, 512, 64, 256) &&
                  !px_a_off_b(false, 512, 8, 256, 256),
              "the partition over all workgroups where the rows would not fit, or the knob is off");
// the one-row instances that carry the placement (n = 1280 never takes it)
constexpr int PX_AOB_NMAX = 1024;
// One-row cross-attention task placement: workgroup wg runs tasks first,
// first + G, ... below ntask.  early (and room for it: H + ntask <= G): task t
// on workgroup H + t, off the H workgroups whose self-attention task (phase B)
// is on the step's critical path; else task t on workgroup t % G.
__host__ __device__ constexpr bool px_e_early(bool early, int H, int ntask, int G) { return early && H + ntask <= G; }
__host__ __device__ constexpr int px_e_first_task(bool early, int wg, int H, int ntask, int G) {
    return px_e_early(early, H, ntask, G) ? (wg >= H ? wg - H : ntask) : wg;
}
// every task taken by exactly one workgroup, once
constexpr bool px_e_tasks_once(bool early, int H, int nch, int G) {
    const int ntask = H * nch;
    for (int t = 0; t < ntask; ++t) {
        int cnt = 0;
        for (int wg = 0; wg < G; ++wg)
            for (int u = px_e_first_task(early, wg, H, ntask, G); u < ntask; u += G) cnt += u == t;
        if (cnt != 1) return false;
    }
    return true;
}
static_assert(px_e_tasks_once(true, 2, 12, 256) && px_e_tasks_once(true, 6, 12, 256) && px_e_tasks_once(true, 8, 12, 256) &&
                  px_e_tasks_once(true, 12, 12, 256) && px_e_tasks_once(true, 12, 12, 192) && px_e_tasks_once(true, 2, 1, 256),
              "cross tasks beside the self-attention workgroups");
static_assert(px_e_tasks_once(true, 12, 24, 192) && px_e_tasks_once(false, 8, 12, 256) && px_e_tasks_once(false, 12, 12, 64),
              "cross tasks where they do not fit beside them, or the knob is off");
// the one-row instances that take the early placement: up to this n (at
// n = 768 the operands do not fit beside the register-resident vocabulary
// rows without scratch memory)
constexpr int PX_EOP_NMAX = 512;
// WMI_PTRACE's second stamped workgroup: G / 2, or the first cross-task
// workgroup where workgroup 0 has none (px_e_first_task)
inline int persist_trace_wg(const PersistArgs &a, int G) {
    const int H = a.n / 64;
    return a.B == 1 && !a.beam && a.n <= PX_EOP_NMAX && px_e_early(a.early_ops != 0, H, H * a.nch, G) ? H : G / 2;
}
hipError_t launch_dec_persist(hipStream_t s, const PersistArgs &a, int G);
// the inputs whose f32 exp is too close to an f16 midpoint, with their table
// values, into list[64] (count in *n; > 64 means the list is unusable)
hipError_t launch_exp_fallbacks(hipStream_t s, const uint16_t *exp_tab, int n_exp, uint32_t *list, uint32_t *n);
// the persistent decoder's exp vs the host ggml table, every non-positive f16 input
hipError_t launch_persist_selftest(hipStream_t s, const uint16_t *exp_tab, int n_exp, const uint32_t *fb,
                                   uint32_t *mismatch);
// largest co-resident grid for the model (0: not supported for this n / B / T)
// and the vocabulary rows per workgroup that fit in LDS beside the phases' data
int persist_grid(int device, int n, int B, int T, int V, int *nres);
// workgroups of each of two concurrent multi-row launches sharing the
// device's G-workgroup grid (0: the rows per workgroup would not fit)
int persist_split_grid(int n, int G);

}  // namespace wmi
