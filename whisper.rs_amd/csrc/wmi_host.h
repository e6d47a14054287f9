// wmi_host.h — the host-only unit (wmi_host.cpp): everything that reads an
// untrusted file or builds a table on the CPU, with no HIP or RCCL dependency.
//
// This header and wmi_host.cpp include only the public header and the
// standard library, so the unit compiles as plain C++ and links into a
// stand-alone program (loader_check.cpp) without a device runtime.  Functions
// here report failure as a status code plus a message in `err`; the ABI entry
// in another unit passes it to set_err.
//
// The file parser reproduces the reference loader's checks and error order
// (main.rs:1384-1475); wmi_api.cpp then packs the weights once for the
// kernels into one device arena, in place of the reference's four fixed-size
// byte arenas (main.rs:402-418), with a workspace planned from the hparams.
#pragma once
#include <stdint.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/whisper_mi355x.h"

// what crosses a unit boundary inside the library is never exported from it
#define WMI_LOCAL __attribute__((visibility("hidden")))

namespace wmi WMI_LOCAL {

uint16_t f32_to_f16(float f);
uint16_t f64_to_f16(double v);
float f16_to_f32(uint16_t h);
void build_tables(std::vector<uint16_t> &gelu, std::vector<uint16_t> &expt);

struct HostTensor {
    int dtype = 0;  // 0 f32, 1 f16 (quantised matrices are dequantised to f16)
    int qtype = 0;  // ggml type of a quantised matrix in the file (7 = q5_1), else 0
    std::vector<uint8_t> qraw;  // its blocks as read (q5_1 only: the decoder GEMVs read them)
    int n_dims = 0;
    int64_t ne[3] = {1, 1, 1};
    std::vector<uint8_t> data;
    int64_t nel() const { return ne[0] * ne[1] * ne[2]; }
    const float *f32() const { return (const float *)data.data(); }
    const uint16_t *f16() const { return (const uint16_t *)data.data(); }
};

struct Expected {
    int dtype;
    int n_dims;
    int64_t ne[3];
};

struct ParsedModel {
    wmi_hparams hp{};
    int32_t n_filt_mel = 0, n_filt_ff = 0;
    std::vector<float> filters;
    std::vector<std::string> vocab;
    std::map<std::string, HostTensor> tensors;
};

int qblock_bytes(int t);
void dequant_f16(int t, const uint8_t *src, int64_t nel, uint16_t *dst);
int check_shape(const wmi_hparams &hp, std::string &err);
int parse_file(const char *path, ParsedModel &pm, std::string &err);
void init_specials(int32_t n_vocab, wmi_special_tokens &sp);
int read_wav(const char *path, int16_t *samples, size_t cap, size_t *n_samples, int32_t *sample_rate, int32_t *channels,
             std::string &err);
int tokens_to_text(const std::vector<std::string> &vocab, int32_t eot, const int32_t *ids, int n, char *buf, size_t cap,
                   size_t *len);
const std::set<std::string> &non_speech_set();

// ---- token-level timestamps: the host steps (DESIGN.md "Token-level
// timestamps"; step C, the voice-activity pass, runs on the device between
// B and D).  A text token has 0 <= id < eot; its bytes are vocab[id]. --------
struct TokParams {
    float thold_pt = 0.01f, thold_ptsum = 0.01f;
    int32_t max_len = 0, split_on_word = 0;
};
// step A: 0.01 a space, 2 a comma, 3 each of . ! ? and the digits, 1 any other byte, summed in f32 in byte order
float token_vlen(const std::string &bytes);
// steps A and B for the n tokens of a segment [T0, T1) of the window at frame W:
// every token's vlen, the text tokens' t0 / t1; returns the text tokens' indices
std::vector<int> token_bounds(const std::vector<std::string> &vocab, int32_t eot, int32_t beg, const TokParams &p, int64_t W,
                              int64_t T0, int64_t T1, wmi_token_data *tok, int n);
// step D: t0 = t1 of the other tokens
void token_fill_others(int32_t eot, int64_t T0, int64_t T1, wmi_token_data *tok, int n);
// step E: the pieces of a segment under max_len / split_on_word (one piece with max_len 0)
struct TokPiece {
    int64_t t0, t1;
    int first, count;  // its tokens
    std::string text;
};
std::vector<TokPiece> split_segment(const std::vector<std::string> &vocab, int32_t eot, const TokParams &p, int64_t T0,
                                    int64_t T1, const wmi_token_data *tok, int n);

// ---- token times from cross-attention alignment: the host side (DESIGN.md
// "Token times from cross-attention alignment") -------------------------------
// wmi_set_dtw's checks and the head table, (layer, head) pairs in order: from
// p.heads, or every head of the last p.n_top text layers; WMI_E_INVALID_ARG
// with the reason in err
int dtw_head_table(const wmi_hparams &hp, const wmi_dtw_params &p, std::vector<int32_t> &pairs, std::string &err);

// ---- chunked long-form transcription: the plan on the host (the header's
// "chunked long-form transcription" states it) ---------------------------------
// wmi_set_chunking's checks of the fields as given; the reason in err
int chunk_check_params(const wmi_chunk_params &p, std::string &err);
// Cmax, Cmin and h with the zeros resolved for a window of `window` frames; WMI_E_INVALID_ARG if Cmin > Cmax or no Cmax
int chunk_resolve(const wmi_chunk_params &p, int window, int *Cmax, int *Cmin, int *h, std::string &err);
// n (start, end) pairs: ascending, non-overlapping, start < end, none negative
int chunk_check_spans(const int64_t *spans, int n, std::string &err);
// the chain of cuts over P [N + 1] (P may be null while n_len <= Cmax: no cut is then looked for)
std::vector<int64_t> chunk_plan(const uint64_t *P, int64_t N, int Cmax, int Cmin, int h);

// ---- audio of any rate (DESIGN.md "Audio front end"; the header's "audio of
// any format" states the plan and the taps) --------------------------------
// L, M, K of a rate, or WMI_E_UNSUPPORTED outside the plan
int resample_plan(int32_t sample_rate, int32_t *L, int32_t *M, int32_t *K);
// h[ph][j], L rows of 2K taps, each row `stride` >= 2K floats apart (the rest of a row is left as it is)
void resample_taps(int32_t L, int32_t M, int32_t K, float *h, size_t stride);
// N_out of N frames; false if it does not fit a size_t
bool resampled_length(int32_t L, int32_t M, size_t N, size_t *n_out);

}  // namespace wmi
