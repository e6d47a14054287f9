// wmi_host.cpp — host-only code: f16 conversions and the ggml tables, the
// ggml-v1 file parser, the WAV reader, token text and the non-speech table.
//
// No HIP or RCCL header, no wmi_context (wmi_host.h has the rule).  The
// weights and tables built here are compared bitwise by the GPU tests, so the
// unit keeps the other units' -O3 -ffp-contract=off and the pragma below.
#include "wmi_host.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#pragma clang fp contract(off)

namespace wmi WMI_LOCAL {

// ---------------------------------------------------------------------------
// host f16 helpers (round to nearest even, as F16C / v_cvt_f16_f32)
// ---------------------------------------------------------------------------
uint16_t f32_to_f16(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    uint32_t mant = x & 0x7fffffu;
    const int exp = (int)((x >> 23) & 0xffu);
    if (exp == 0xff) return (uint16_t)(sign | 0x7c00u | (mant ? 0x200u : 0u));
    const int e = exp - 127 + 15;
    if (e >= 31) return (uint16_t)(sign | 0x7c00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        mant |= 0x800000u;
        const int shift = 14 - e;
        uint32_t h = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t h = sign | ((uint32_t)e << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (uint16_t)h;
}

// correctly rounded (RNE) double -> f16
uint16_t f64_to_f16(double v) {
    uint64_t x;
    memcpy(&x, &v, 8);
    const uint32_t sign = (uint32_t)(x >> 48) & 0x8000u;
    x &= ~(1ull << 63);
    if (x >= 0x7ff0000000000000ull) return (uint16_t)(sign | 0x7c00u | (x > 0x7ff0000000000000ull ? 0x200u : 0u));
    if (x < 0x0010000000000000ull) return (uint16_t)sign;  // double subnormals: far below f16's range
    const int e = (int)(x >> 52) - 1023;
    const uint64_t mant = (x & ((1ull << 52) - 1)) | (1ull << 52);
    if (e >= 16) return (uint16_t)(sign | 0x7c00u);
    const int shift = e >= -14 ? 42 : 42 + (-14 - e);
    if (shift >= 63) return (uint16_t)sign;
    uint64_t q = mant >> shift;
    const uint64_t rem = mant & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    if (e < -14) return (uint16_t)(sign | q);  // subnormal (a carry into 0x400 is the smallest normal)
    uint32_t ex = (uint32_t)(e + 15);
    if (q >> 11) { q >>= 1; ++ex; }
    if (ex >= 31) return (uint16_t)(sign | 0x7c00u);
    return (uint16_t)(sign | (ex << 10) | (uint32_t)(q & 0x3ffu));
}

float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t x;
    if (e == 0) {
        if (m == 0) x = sign;
        else {
            int ee = -1;
            uint32_t mm = m;
            do { ++ee; mm <<= 1; } while (!(mm & 0x400u));
            x = sign | ((uint32_t)(127 - 15 - ee) << 23) | ((mm & 0x3ffu) << 13);
        }
    } else if (e == 31) {
        x = sign | 0x7f800000u | (m << 13);
    } else {
        x = sign | ((e - 15 + 127) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// ggml_init tables (ggml-1.0.3): GELU and exp over every f16 value
void build_tables(std::vector<uint16_t> &gelu, std::vector<uint16_t> &expt) {
    const float GELU_COEF_A = 0.044715f;
    const float SQRT_2_OVER_PI = 0.79788456080286535587989211986876f;
    gelu.resize(65536);
    expt.resize(65536);
    for (int i = 0; i < 65536; ++i) {
        const float f = f16_to_f32((uint16_t)i);
        gelu[i] = f32_to_f16(0.5f * f * (1.0f + tanhf(SQRT_2_OVER_PI * f * (1.0f + GELU_COEF_A * f * f))));
        expt[i] = f32_to_f16((float)exp((double)f));
    }
}

// ---------------------------------------------------------------------------
// ggml-v1 file parser: WhisperContext::new + WhisperModel::load
// ---------------------------------------------------------------------------
// ggml quantised blocks (QNT version 2).  The
// reference loader rejects them (main.rs:1423-1434); this build dequantises
// every matrix to f16, w = f16(q * d (+ m)) rounded once (a fused multiply-
// add), and keeps q5_1 blocks as well for the bandwidth-bound decoder GEMVs,
// which dequantise on the fly (v_pk_fma_f16) to the same f16 values.
int qblock_bytes(int t) {
    switch (t) {
        case 2: return 18;  // q4_0 {d, qs[16]}
        case 3: return 20;  // q4_1 {d, m, qs[16]}
        case 6: return 22;  // q5_0 {d, qh, qs[16]}
        case 7: return 24;  // q5_1 {d, m, qh, qs[16]}
        case 8: return 34;  // q8_0 {d, qs[32]}
        default: return 0;
    }
}

void dequant_f16(int t, const uint8_t *src, int64_t nel, uint16_t *dst) {
    const int bs = qblock_bytes(t);
    for (int64_t ib = 0; ib < nel / 32; ++ib) {
        const uint8_t *b = src + ib * bs;
        uint16_t *y = dst + ib * 32;
        uint16_t hd, hm = 0;
        memcpy(&hd, b, 2);
        const float d = f16_to_f32(hd);
        float m = 0.0f;
        if (t == 3 || t == 7) {
            memcpy(&hm, b + 2, 2);
            m = f16_to_f32(hm);
        }
        int q[32];
        if (t == 2 || t == 3) {
            const uint8_t *qs = b + (t == 2 ? 2 : 4);
            for (int j = 0; j < 16; ++j) { q[j] = qs[j] & 15; q[j + 16] = qs[j] >> 4; }
        } else if (t == 6 || t == 7) {
            const int o = t == 6 ? 2 : 4;
            uint32_t qh;
            memcpy(&qh, b + o, 4);
            const uint8_t *qs = b + o + 4;
            for (int j = 0; j < 16; ++j) {
                q[j] = (qs[j] & 15) | (int)(((qh >> j) & 1u) << 4);
                q[j + 16] = (qs[j] >> 4) | (int)(((qh >> (j + 16)) & 1u) << 4);
            }
        } else {
            for (int j = 0; j < 32; ++j) q[j] = (int8_t)b[2 + j];
        }
        const int off = t == 2 ? 8 : t == 6 ? 16 : 0;
        // q * d + m is exact in double (|log2(d / m)| <= 37); one rounding to f16
        for (int j = 0; j < 32; ++j) y[j] = f64_to_f16((double)(q[j] - off) * (double)d + (double)m);
    }
}

// The model shapes the kernels implement; anything else is WMI_E_UNSUPPORTED.
// Checked right after the header is parsed (before tensors are read and the
// device is touched) and again by run_encode.
int check_shape(const wmi_hparams &hp, std::string &err) {
    char msg[128];
    const int n = hp.n_audio_state, H = hp.n_audio_head;
    msg[0] = 0;
    if (hp.n_text_state != n) snprintf(msg, sizeof msg, "n_text_state != n_audio_state");
    else if (hp.n_text_ctx > 512) snprintf(msg, sizeof msg, "n_text_ctx %d > 512", hp.n_text_ctx);
    else if (n > 1280 || n % 128) snprintf(msg, sizeof msg, "n_state %d (need a multiple of 128, <= 1280)", n);
    else if (n / H != 64 || hp.n_text_state / hp.n_text_head != 64)
        snprintf(msg, sizeof msg, "head dim %d != 64", n / H != 64 ? n / H : hp.n_text_state / hp.n_text_head);
    if (!msg[0]) return WMI_OK;
    err = msg;
    return WMI_E_UNSUPPORTED;
}

int parse_file(const char *path, ParsedModel &pm, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = std::string("Unexpected IO: cannot open '") + path + "'"; return WMI_E_IO; }
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
    fseek(f, 0, SEEK_END);
    const long fsize = ftell(f);
    fseek(f, 0, SEEK_SET);
    auto rd = [&](void *p, size_t n) { return fread(p, 1, n, f) == n; };
    uint32_t magic = 0;
    if (!rd(&magic, 4)) { err = "Unexpected IO: short read (magic)"; return WMI_E_IO; }
    if (magic != 0x67676d6cu) { err = std::string("invalid model file '") + path + "' (bad magic)"; return WMI_E_BAD_MAGIC; }
    int32_t hpv[11];
    if (!rd(hpv, 44)) { err = "Unexpected IO: short read (hparams)"; return WMI_E_IO; }
    memcpy(&pm.hp, hpv, 44);
    const wmi_hparams &hp = pm.hp;
    for (int i = 0; i < 10; ++i)
        if (hpv[i] <= 0) { err = "Unexpected: non-positive hparam"; return WMI_E_UNEXPECTED; }
    // bounds far above every Whisper model, so no element count derived from
    // them can overflow and nothing is allocated from a corrupt header
    if (hp.n_vocab > (1 << 20) || hp.n_audio_ctx > (1 << 16) || hp.n_text_ctx > (1 << 16) ||
        hp.n_audio_state > (1 << 14) || hp.n_text_state > (1 << 14) || hp.n_audio_head > (1 << 10) ||
        hp.n_text_head > (1 << 10) || hp.n_audio_layer > (1 << 10) || hp.n_text_layer > (1 << 10) ||
        hp.n_mels > (1 << 12)) {
        err = "Unexpected: hparam out of range";
        return WMI_E_UNEXPECTED;
    }
    if (hp.n_audio_state % hp.n_audio_head || hp.n_text_state % hp.n_text_head) {
        err = "Unexpected: state not divisible by heads";
        return WMI_E_UNEXPECTED;
    }
    if (int rc = check_shape(hp, err)) return rc;
    // filters (main.rs:513-535)
    if (!rd(&pm.n_filt_mel, 4) || !rd(&pm.n_filt_ff, 4)) { err = "Unexpected IO: short read (filters)"; return WMI_E_IO; }
    if (pm.n_filt_mel <= 0 || pm.n_filt_ff <= 0 || (int64_t)pm.n_filt_mel * pm.n_filt_ff > (1 << 24) ||
        (int64_t)pm.n_filt_mel * pm.n_filt_ff * 4 > fsize - ftell(f)) {
        err = "Unexpected: bad filter dims";
        return WMI_E_UNEXPECTED;
    }
    pm.filters.resize((size_t)pm.n_filt_mel * pm.n_filt_ff);
    if (!rd(pm.filters.data(), pm.filters.size() * 4)) { err = "Unexpected IO: short read (filters)"; return WMI_E_IO; }
    // vocab (main.rs:430, 578-592)
    int32_t nv = 0;
    if (!rd(&nv, 4) || nv < 0 || (int64_t)nv * 4 > fsize - ftell(f)) { err = "Unexpected IO: vocab"; return WMI_E_IO; }
    pm.vocab.resize(nv);
    for (int32_t i = 0; i < nv; ++i) {
        uint32_t len = 0;
        if (!rd(&len, 4) || len > (1u << 20) || (int64_t)len > fsize - ftell(f)) { err = "Unexpected IO: vocab"; return WMI_E_IO; }
        pm.vocab[i].resize(len);
        if (len && !rd(&pm.vocab[i][0], len)) { err = "Unexpected IO: vocab"; return WMI_E_IO; }
    }
    // expected tensors (main.rs:947-1334)
    std::map<std::string, Expected> exp;
    const int64_t n = hp.n_audio_state, nt = hp.n_text_state;
    const int file_ftype = hp.f16 % 1000;  // ggml ftype + 1000 * quantisation version
    const int W = file_ftype == 0 ? 0 : 1;  // matrices land as f16 (quantised ones dequantised)
    exp["encoder.positional_embedding"] = {0, 2, {n, hp.n_audio_ctx, 1}};
    exp["encoder.conv1.weight"] = {W, 3, {3, hp.n_mels, n}};
    exp["encoder.conv1.bias"] = {0, 2, {1, n, 1}};
    exp["encoder.conv2.weight"] = {W, 3, {3, n, n}};
    exp["encoder.conv2.bias"] = {0, 2, {1, n, 1}};
    exp["encoder.ln_post.weight"] = {0, 1, {n, 1, 1}};
    exp["encoder.ln_post.bias"] = {0, 1, {n, 1, 1}};
    char nm[128];
    for (int i = 0; i < hp.n_audio_layer; ++i) {
        auto E = [&](const char *s, int dt, int nd, int64_t a, int64_t b) {
            snprintf(nm, sizeof nm, "encoder.blocks.%d.%s", i, s);
            exp[nm] = {dt, nd, {a, b, 1}};
        };
        E("mlp_ln.weight", 0, 1, n, 1); E("mlp_ln.bias", 0, 1, n, 1);
        E("mlp.0.weight", W, 2, n, 4 * n); E("mlp.0.bias", 0, 1, 4 * n, 1);
        E("mlp.2.weight", W, 2, 4 * n, n); E("mlp.2.bias", 0, 1, n, 1);
        E("attn_ln.weight", 0, 1, n, 1); E("attn_ln.bias", 0, 1, n, 1);
        E("attn.query.weight", W, 2, n, n); E("attn.query.bias", 0, 1, n, 1);
        E("attn.key.weight", W, 2, n, n);
        E("attn.value.weight", W, 2, n, n); E("attn.value.bias", 0, 1, n, 1);
        E("attn.out.weight", W, 2, n, n); E("attn.out.bias", 0, 1, n, 1);
    }
    exp["decoder.positional_embedding"] = {0, 2, {nt, hp.n_text_ctx, 1}};
    exp["decoder.token_embedding.weight"] = {W, 2, {nt, hp.n_vocab, 1}};
    exp["decoder.ln.weight"] = {0, 1, {nt, 1, 1}};
    exp["decoder.ln.bias"] = {0, 1, {nt, 1, 1}};
    for (int i = 0; i < hp.n_text_layer; ++i) {
        auto E = [&](const char *s, int dt, int nd, int64_t a, int64_t b) {
            snprintf(nm, sizeof nm, "decoder.blocks.%d.%s", i, s);
            exp[nm] = {dt, nd, {a, b, 1}};
        };
        E("mlp_ln.weight", 0, 1, nt, 1); E("mlp_ln.bias", 0, 1, nt, 1);
        E("mlp.0.weight", W, 2, nt, 4 * nt); E("mlp.0.bias", 0, 1, 4 * nt, 1);
        E("mlp.2.weight", W, 2, 4 * nt, nt); E("mlp.2.bias", 0, 1, nt, 1);
        for (const char *a : {"attn", "cross_attn"}) {
            char s[64];
            snprintf(s, sizeof s, "%s_ln.weight", a); E(s, 0, 1, nt, 1);
            snprintf(s, sizeof s, "%s_ln.bias", a); E(s, 0, 1, nt, 1);
            snprintf(s, sizeof s, "%s.query.weight", a); E(s, W, 2, nt, nt);
            snprintf(s, sizeof s, "%s.query.bias", a); E(s, 0, 1, nt, 1);
            snprintf(s, sizeof s, "%s.key.weight", a); E(s, W, 2, nt, nt);
            snprintf(s, sizeof s, "%s.value.weight", a); E(s, W, 2, nt, nt);
            snprintf(s, sizeof s, "%s.value.bias", a); E(s, 0, 1, nt, 1);
            snprintf(s, sizeof s, "%s.out.weight", a); E(s, W, 2, nt, nt);
            snprintf(s, sizeof s, "%s.out.bias", a); E(s, 0, 1, nt, 1);
        }
    }
    // every expected tensor exists, zero-filled, like the reference arena —
    // once the file is large enough to hold them (>= 1 byte per 4 elements:
    // q4 blocks are the densest form), so a small corrupt file allocates nothing
    int64_t exp_nel = 0;
    for (auto &kv : exp) exp_nel += (int64_t)kv.second.ne[0] * kv.second.ne[1] * kv.second.ne[2];
    if (exp_nel / 4 > (int64_t)fsize) {
        err = "Unexpected IO: file too short for its hparams";
        return WMI_E_IO;
    }
    for (auto &kv : exp) {
        HostTensor t;
        t.dtype = kv.second.dtype;
        t.n_dims = kv.second.n_dims;
        for (int i = 0; i < 3; ++i) t.ne[i] = kv.second.ne[i];
        t.data.assign((size_t)t.nel() * (t.dtype ? 2 : 4), 0);
        pm.tensors[kv.first] = std::move(t);
    }
    // record loop (main.rs:1384-1475): until fewer than 12 bytes remain
    for (;;) {
        const long pos = ftell(f);
        if (fsize - pos < 12) break;
        int32_t hdr[3];
        if (!rd(hdr, 12)) { err = "Unexpected IO: short read (tensor header)"; return WMI_E_IO; }
        const int32_t n_dims = hdr[0], len = hdr[1], ftype = hdr[2];
        if (n_dims < 1 || n_dims > 3 || len <= 0 || len > 255) {
            char b[128];
            snprintf(b, sizeof b, "Unexpected: bad tensor header (n_dims %d, name_len %d)", n_dims, len);
            err = b;
            return WMI_E_UNEXPECTED;
        }
        int64_t ne[3] = {1, 1, 1}, nel = 1;
        for (int i = 0; i < n_dims; ++i) {
            int32_t v;
            if (!rd(&v, 4)) { err = "Unexpected IO: short read (dims)"; return WMI_E_IO; }
            ne[i] = v;
            nel *= v;
        }
        std::string name(len, '\0');
        if (!rd(&name[0], len)) { err = "Unexpected IO: short read (name)"; return WMI_E_IO; }
        auto it = pm.tensors.find(name);
        char b[512];
        if (it == pm.tensors.end()) {
            snprintf(b, sizeof b, "unknown tensor '%s' in model file", name.c_str());
            err = b;
            return WMI_E_UNKNOWN_TENSOR;
        }
        HostTensor &t = it->second;
        if (t.nel() != nel) {
            snprintf(b, sizeof b, "tensor %s has wrong size in model file, got:%lld, expected:%lld", name.c_str(),
                     (long long)t.nel(), (long long)nel);
            err = b;
            return WMI_E_WRONG_SIZE;
        }
        for (int i = 0; i < t.n_dims; ++i)
            if (t.ne[i] != ne[i]) {
                snprintf(b, sizeof b, "tensor %s has wrong shape in model file, got:[%lld, %lld, %lld], expected:[%lld, %lld, %lld]",
                         name.c_str(), (long long)t.ne[0], (long long)t.ne[1], (long long)t.ne[2], (long long)ne[0],
                         (long long)ne[1], (long long)ne[2]);
                err = b;
                return WMI_E_WRONG_SHAPE;
            }
        const int qb = (t.dtype == 1 && t.n_dims == 2 && ne[0] % 32 == 0) ? qblock_bytes(ftype) : 0;
        const int64_t file_bytes = qb ? nel / 32 * qb : nel * (ftype == 0 ? 4 : 2);
        if (!qb && file_bytes != (int64_t)t.data.size()) {
            snprintf(b, sizeof b, "tensor %s has wrong bytes in model file, got:%lld, expected:%lld", name.c_str(),
                     (long long)t.data.size(), (long long)file_bytes);
            err = b;
            return WMI_E_WRONG_BYTES;
        }
        if (qb) {
            std::vector<uint8_t> raw((size_t)file_bytes);
            if (!rd(raw.data(), raw.size())) { err = "Unexpected IO: short read (tensor data)"; return WMI_E_IO; }
            dequant_f16(ftype, raw.data(), nel, (uint16_t *)t.data.data());
            t.qtype = ftype;
            if (ftype == 7) t.qraw = std::move(raw);
        } else {
            t.qtype = 0;
            t.qraw.clear();
            if (!rd(t.data.data(), t.data.size())) { err = "Unexpected IO: short read (tensor data)"; return WMI_E_IO; }
        }
    }
    {
        const int ft = hp.f16 % 1000, qv = hp.f16 / 1000;
        const bool ok = ft == 0 || ft == 1 || ((ft == 2 || ft == 3 || ft == 7 || ft == 8 || ft == 9) && qv == 2);
        if (!ok) {
            char b[160];
            snprintf(b, sizeof b, "model ftype %d (hparams.f16 = %d) is not supported by this build", ft, hp.f16);
            err = b;
            return WMI_E_UNSUPPORTED;
        }
    }
    return WMI_OK;
}

// special ids: main.rs:557-575 + multilingual shift main.rs:433-440 (large-v3:
// later whisper.cpp's variable-language shift)
void init_specials(int32_t n_vocab, wmi_special_tokens &sp) {
    int32_t eot = 50256, sot = 50257, prev = 50360, solm = 50361, not_ = 50362, beg = 50363;
    int32_t translate = 50358, transcribe = 50359;
    const int multilingual = n_vocab >= 51865;
    if (multilingual) {
        const int dt = (n_vocab - 51765 - 1) - 98;
        const int extra = dt > 1 ? dt - 1 : 0;
        eot += 1; sot += 1;
        prev += 1 + extra; solm += 1 + extra; not_ += 1 + extra; beg += 1 + extra;
        translate += extra; transcribe += extra;
    }
    sp = {eot, sot, prev, solm, not_, beg, translate, transcribe, multilingual};
}

// a status code with its message, as set_err formats it
static int fail(std::string &err, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// hound::WavReader::open(path) + samples::<i16>() (main.rs:2067-2068): a
// RIFF/WAVE file with 16-bit integer PCM; samples interleaved as stored.
// Chunks other than "fmt " and "data" are skipped (word-aligned, as RIFF
// requires); a data chunk longer than the file is an IO error, as is a
// missing "fmt " before "data".
int read_wav(const char *path, int16_t *samples, size_t cap, size_t *n_samples, int32_t *sample_rate, int32_t *channels,
             std::string &err) {
    if (!path || !n_samples) return fail(err, WMI_E_INVALID_ARG, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(err, WMI_E_IO, "cannot open %s", path);
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    unsigned char hdr[12];
    if (fread(hdr, 1, 12, f) != 12 || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4))
        return fail(err, WMI_E_IO, "%s: not a RIFF/WAVE file", path);
    auto u16 = [](const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); };
    auto u32 = [](const unsigned char *p) {
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    };
    bool have_fmt = false;
    uint32_t fmt_tag = 0, nch = 0, sr = 0, bits = 0;
    for (;;) {
        unsigned char ch[8];
        if (fread(ch, 1, 8, f) != 8) return fail(err, WMI_E_IO, "%s: no data chunk", path);
        const uint32_t size = u32(ch + 4);
        if (!memcmp(ch, "fmt ", 4)) {
            if (size < 16) return fail(err, WMI_E_IO, "%s: short fmt chunk", path);
            std::vector<unsigned char> fmt(size + (size & 1));
            if (fread(fmt.data(), 1, fmt.size(), f) != fmt.size()) return fail(err, WMI_E_IO, "%s: truncated fmt", path);
            fmt_tag = u16(fmt.data());
            nch = u16(fmt.data() + 2);
            sr = u32(fmt.data() + 4);
            bits = u16(fmt.data() + 14);
            if (fmt_tag == 0xFFFE && size >= 26) fmt_tag = u16(fmt.data() + 24);  // WAVE_FORMAT_EXTENSIBLE subformat
            have_fmt = true;
        } else if (!memcmp(ch, "data", 4)) {
            if (!have_fmt) return fail(err, WMI_E_IO, "%s: data before fmt", path);
            if (fmt_tag != 1 || bits != 16 || nch < 1)
                return fail(err, WMI_E_UNSUPPORTED, "%s: format %u, %u bits, %u channels (need 16-bit PCM)", path,
                               fmt_tag, bits, nch);
            const size_t n = size / 2;
            *n_samples = n;
            if (sample_rate) *sample_rate = (int32_t)sr;
            if (channels) *channels = (int32_t)nch;
            if (!samples) return WMI_OK;
            if (cap < n) return WMI_E_NO_SPACE;
            {
                const long here = ftell(f);
                fseek(f, 0, SEEK_END);
                const long end = ftell(f);
                fseek(f, here, SEEK_SET);
                if ((long)size > end - here) return fail(err, WMI_E_IO, "%s: data chunk of %u bytes beyond the file", path, size);
            }
            std::vector<unsigned char> raw(size);
            if (fread(raw.data(), 1, size, f) != size) return fail(err, WMI_E_IO, "%s: truncated data", path);
            for (size_t i = 0; i < n; ++i) samples[i] = (int16_t)u16(raw.data() + 2 * i);
            return WMI_OK;
        } else if (fseek(f, (long)(size + (size & 1)), SEEK_CUR) != 0) {
            return fail(err, WMI_E_IO, "%s: truncated chunk", path);
        }
    }
}

// Text of a token sequence: the id_to_token bytes (main.rs:578-592) of every
// text token (id < eot) concatenated, special and timestamp tokens skipped,
// as whisper.cpp-1.0.3's whisper_full builds a segment's text.
int tokens_to_text(const std::vector<std::string> &vocab, int32_t eot, const int32_t *ids, int n, char *buf, size_t cap,
                   size_t *len) {
    std::string s;
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= (int32_t)vocab.size()) return WMI_E_INVALID_ARG;
        if (ids[i] < eot) s += vocab[ids[i]];
    }
    *len = s.size();
    if (!buf || cap < s.size()) return WMI_E_NO_SPACE;
    memcpy(buf, s.data(), s.size());
    return WMI_OK;
}

// whisper.cpp's non_speech_tokens: symbols whose tokens (bare or after a space) the rules may suppress
static const char *const NON_SPEECH[] = {
    "\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
    "\xe3\x80\x8c", "\xe3\x80\x8d", "\xe3\x80\x8e", "\xe3\x80\x8f",
    "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]", "{{", "}}",
    "\xe2\x99\xaa\xe2\x99\xaa", "\xe2\x99\xaa\xe2\x99\xaa\xe2\x99\xaa",
    "\xe2\x99\xa9", "\xe2\x99\xaa", "\xe2\x99\xab", "\xe2\x99\xac", "\xe2\x99\xad", "\xe2\x99\xae", "\xe2\x99\xaf"};

const std::set<std::string> &non_speech_set() {
    static const std::set<std::string> want = [] {
        std::set<std::string> w{" -", " '"};
        for (const char *s : NON_SPEECH) {
            w.insert(s);
            w.insert(std::string(" ") + s);
        }
        return w;
    }();
    return want;
}

// ---- token-level timestamps: steps A, B, D and E ------------------------------
// (whisper.cpp-1.0.3's whisper_exp_compute_token_level_timestamps and
// whisper_wrap_segment, restated in include/whisper_mi355x.h; this unit is
// compiled with -ffp-contract=off: the fill's multiply and divide round apart)
namespace {
const std::string &token_bytes(const std::vector<std::string> &vocab, int32_t id) {
    static const std::string none;
    return id >= 0 && (size_t)id < vocab.size() ? vocab[(size_t)id] : none;
}
bool is_text(int32_t id, int32_t eot) { return id >= 0 && id < eot; }
}  // namespace

float token_vlen(const std::string &bytes) {
    float v = 0.0f;
    for (const char c : bytes) {
        if (c == ' ') v += 0.01f;
        else if (c == ',') v += 2.0f;
        else if (c == '.' || c == '!' || c == '?' || (c >= '0' && c <= '9')) v += 3.0f;
        else v += 1.0f;
    }
    return v;
}

std::vector<int> token_bounds(const std::vector<std::string> &vocab, int32_t eot, int32_t beg, const TokParams &p, int64_t W,
                              int64_t T0, int64_t T1, wmi_token_data *tok, int n) {
    std::vector<int> tx;
    for (int i = 0; i < n; ++i) {
        const bool text = is_text(tok[i].id, eot);
        tok[i].vlen = text ? token_vlen(token_bytes(vocab, tok[i].id)) : 0.0f;
        if (text) tx.push_back(i);
    }
    const int m = (int)tx.size();
    if (m == 0) return tx;
    // b[k]: the boundary behind text token k (1-based), b[0] = T0, b[m] = T1
    std::vector<int64_t> b((size_t)m + 1, 0);
    std::vector<char> set((size_t)m + 1, 0);
    b[0] = T0; b[(size_t)m] = T1;
    set[0] = set[(size_t)m] = 1;
    int64_t ta = T0;
    for (int k = 2; k <= m; ++k) {
        const wmi_token_data &t = tok[tx[(size_t)k - 1]];
        const int64_t tt = W + 2 * ((int64_t)t.tid - beg);
        if (t.pt > p.thold_pt && t.ptsum > p.thold_ptsum && tt > ta && tt <= T1) {
            b[(size_t)k - 1] = tt;
            set[(size_t)k - 1] = 1;
            ta = tt;
        }
    }
    for (int pp = 0; pp < m;) {
        int q = pp + 1;
        while (!set[(size_t)q]) ++q;
        if (q > pp + 1) {
            double psum = 0.0;
            for (int k = pp + 1; k <= q; ++k) psum += (double)tok[tx[(size_t)k - 1]].vlen;
            for (int r = pp + 1; r < q; ++r) {
                int64_t step = 0;
                if (psum != 0.0) {
                    const double num = (double)(b[(size_t)q] - b[(size_t)pp]) * (double)tok[tx[(size_t)r - 1]].vlen;
                    step = (int64_t)(num / psum);
                }
                b[(size_t)r] = b[(size_t)r - 1] + step;
            }
        }
        pp = q;
    }
    for (int k = 1; k <= m; ++k) {
        tok[tx[(size_t)k - 1]].t0 = b[(size_t)k - 1];
        tok[tx[(size_t)k - 1]].t1 = b[(size_t)k];
    }
    return tx;
}

void token_fill_others(int32_t eot, int64_t T0, int64_t T1, wmi_token_data *tok, int n) {
    int last_text = -1;
    for (int i = 0; i < n; ++i)
        if (is_text(tok[i].id, eot)) last_text = i;
    int64_t cur = T0;  // before the first text token (and with none at all)
    for (int i = 0; i < n; ++i) {
        if (is_text(tok[i].id, eot)) {
            cur = tok[i].t1;
            continue;
        }
        tok[i].t0 = tok[i].t1 = last_text >= 0 && i > last_text ? T1 : cur;
    }
}

std::vector<TokPiece> split_segment(const std::vector<std::string> &vocab, int32_t eot, const TokParams &p, int64_t T0,
                                    int64_t T1, const wmi_token_data *tok, int n) {
    std::vector<TokPiece> out;
    TokPiece cur{T0, T1, 0, 0, {}};
    int64_t acc = 0;
    for (int i = 0; i < n; ++i) {
        if (is_text(tok[i].id, eot)) {
            const std::string &s = token_bytes(vocab, tok[i].id);
            const int64_t L = (int64_t)s.size();
            if (p.max_len > 0 && acc > 0 && acc + L > p.max_len && (!p.split_on_word || (!s.empty() && s[0] == ' '))) {
                cur.t1 = tok[i].t0;
                out.push_back(cur);
                cur = TokPiece{tok[i].t0, T1, i, 0, {}};
                acc = 0;
            }
            acc += L;
            cur.text += s;
        }
        ++cur.count;
    }
    out.push_back(cur);
    return out;
}

// ---------------------------------------------------------------------------
// audio of any rate: the polyphase plan and its Kaiser-windowed sinc taps
// (the header's "audio of any format", steps 2 and 3; all in double)
// ---------------------------------------------------------------------------
int resample_plan(int32_t sample_rate, int32_t *L, int32_t *M, int32_t *K) {
    if (sample_rate < 4000 || sample_rate > 384000) return WMI_E_UNSUPPORTED;
    int64_t a = sample_rate, b = 16000;
    while (b) { const int64_t t = a % b; a = b; b = t; }
    const int64_t l = 16000 / a, m = sample_rate / a;
    if (l > 640) return WMI_E_UNSUPPORTED;
    const int64_t big = l > m ? l : m;
    if (L) *L = (int32_t)l;
    if (M) *M = (int32_t)m;
    if (K) *K = (int32_t)((64 * big + l - 1) / l);
    return WMI_OK;
}

// I0(x) = sum over k of ((x / 2)^k / k!)^2, ascending until a term falls below 2^-60 of the sum
static double bessel_i0(double x) {
    const double q = x / 2.0;
    double t = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        t *= q / (double)k;
        const double term = t * t;
        sum += term;
        if (term < sum * 0x1p-60) break;
    }
    return sum;
}

void resample_taps(int32_t L, int32_t M, int32_t K, float *h, size_t stride) {
    const double PI = 3.14159265358979323846264338327950288;
    const double c = 0.95 * (L < M ? (double)L / (double)M : 1.0), i0_10 = bessel_i0(10.0);
    std::vector<double> row((size_t)2 * K);
    for (int32_t ph = 0; ph < L; ++ph) {
        double sum = 0.0;
        for (int32_t j = 0; j < 2 * K; ++j) {
            const double d = (double)(j - K + 1) - (double)ph / (double)L;
            const double t = c * d, r = d / (double)K;
            const double sinc = t == 0.0 ? 1.0 : sin(PI * t) / (PI * t);
            const double w = fabs(r) < 1.0 ? bessel_i0(10.0 * sqrt(1.0 - r * r)) / i0_10 : 0.0;
            row[(size_t)j] = c * sinc * w;
            sum += row[(size_t)j];
        }
        for (int32_t j = 0; j < 2 * K; ++j) h[(size_t)ph * stride + (size_t)j] = (float)(row[(size_t)j] / sum);
    }
}

bool resampled_length(int32_t L, int32_t M, size_t N, size_t *n_out) {
    const unsigned __int128 v = ((unsigned __int128)N * (unsigned)L + (unsigned)(M - 1)) / (unsigned)M;
    if (v > (unsigned __int128)SIZE_MAX) return false;
    *n_out = (size_t)v;
    return true;
}

int dtw_head_table(const wmi_hparams &hp, const wmi_dtw_params &p, std::vector<int32_t> &pairs, std::string &err) {
    char b[160];
    auto bad = [&](const char *why, long a0, long a1) {
        snprintf(b, sizeof b, why, a0, a1);
        err = b;
        pairs.clear();
        return (int)WMI_E_INVALID_ARG;
    };
    pairs.clear();
    if (p.medfilt_width < 1 || p.medfilt_width > 15 || !(p.medfilt_width & 1))
        return bad("median width %ld is not an odd number in [1, %ld]", p.medfilt_width, 15);
    if (p.n_heads < 0 || p.n_top < 0 || (p.n_heads > 0 && !p.heads)) return bad("n_heads %ld, n_top %ld, or null heads", p.n_heads, p.n_top);
    if (p.n_heads > 32) return bad("%ld (layer, head) pairs, at most %ld", p.n_heads, 32);
    if (p.n_heads > 0) {
        for (int i = 0; i < p.n_heads; ++i) {
            const int32_t l = p.heads[2 * i], h = p.heads[2 * i + 1];
            if (l < 0 || l >= hp.n_text_layer || h < 0 || h >= hp.n_text_head) return bad("pair (%ld, %ld) outside the model", l, h);
            for (int k = 0; k < i; ++k)
                if (pairs[2 * k] == l && pairs[2 * k + 1] == h) return bad("pair (%ld, %ld) twice", l, h);
            pairs.push_back(l);
            pairs.push_back(h);
        }
    } else if (p.n_top > 0) {
        if (p.n_top > hp.n_text_layer) return bad("n_top %ld above the %ld text layers", p.n_top, hp.n_text_layer);
        if ((int64_t)p.n_top * hp.n_text_head > 32) return bad("n_top %ld selects more than %ld heads", p.n_top, 32);
        for (int32_t l = hp.n_text_layer - p.n_top; l < hp.n_text_layer; ++l)
            for (int32_t h = 0; h < hp.n_text_head; ++h) {
                pairs.push_back(l);
                pairs.push_back(h);
            }
    } else if (p.enable) {
        return bad("enabled with neither heads nor n_top (%ld, %ld)", 0, 0);
    }
    return WMI_OK;
}

int chunk_check_params(const wmi_chunk_params &p, std::string &err) {
    char b[160];
    if (p.max_frames < 0 || p.min_frames < 0 || p.smooth_frames < 0) {
        snprintf(b, sizeof b, "negative field (max_frames %d, min_frames %d, smooth_frames %d)", p.max_frames, p.min_frames,
                 p.smooth_frames);
    } else if (p.max_frames > (1 << 20)) {
        snprintf(b, sizeof b, "max_frames %d above 2^20", p.max_frames);
    } else if (p.smooth_frames > 100) {
        snprintf(b, sizeof b, "smooth_frames %d above 100", p.smooth_frames);
    } else if (p.max_frames > 0 && p.min_frames > p.max_frames) {
        snprintf(b, sizeof b, "min_frames %d above max_frames %d", p.min_frames, p.max_frames);
    } else {
        return WMI_OK;
    }
    err = b;
    return WMI_E_INVALID_ARG;
}

int chunk_resolve(const wmi_chunk_params &p, int window, int *Cmax, int *Cmin, int *h, std::string &err) {
    int rc = chunk_check_params(p, err);
    if (rc) return rc;
    char b[160];
    *Cmax = p.max_frames > 0 ? p.max_frames : window;
    if (*Cmax < 1 || *Cmax > (1 << 20)) {
        snprintf(b, sizeof b, "max_frames 0 with a window of %d frames", window);
        err = b;
        return WMI_E_INVALID_ARG;
    }
    *Cmin = p.min_frames > 0 ? p.min_frames : (*Cmax / 2 > 1 ? *Cmax / 2 : 1);
    *h = p.smooth_frames > 0 ? p.smooth_frames : 10;
    if (*Cmin > *Cmax) {
        snprintf(b, sizeof b, "min_frames %d above the %d frames of max_frames / the window", *Cmin, *Cmax);
        err = b;
        return WMI_E_INVALID_ARG;
    }
    return WMI_OK;
}

int chunk_check_spans(const int64_t *spans, int n, std::string &err) {
    int64_t prev = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t s = spans[2 * i], e = spans[2 * i + 1];
        if (s < prev || e <= s) {
            char b[160];
            snprintf(b, sizeof b, "span %d [%lld, %lld) is empty, negative, or starts before %lld", i, (long long)s, (long long)e,
                     (long long)prev);
            err = b;
            return WMI_E_INVALID_ARG;
        }
        prev = e;
    }
    return WMI_OK;
}

std::vector<int64_t> chunk_plan(const uint64_t *P, int64_t N, int Cmax, int Cmin, int h) {
    std::vector<int64_t> out;
    const int64_t n_len = N / 160;
    int64_t s = 0;
    while (n_len - s > Cmax) {
        uint64_t best = 0;
        int64_t at = -1;
        for (int64_t k = s + Cmin; k <= s + Cmax; ++k) {
            const int64_t hi = std::min<int64_t>(160 * (k + h), N), lo = 160 * std::max<int64_t>(k - h, 0);
            const uint64_t S = P[hi] - P[lo];
            if (at < 0 || S <= best) { best = S; at = k; }
        }
        out.push_back(s);
        out.push_back(at);
        s = at;
    }
    if (n_len > 0) {
        out.push_back(s);
        out.push_back(n_len);
    }
    return out;
}

}  // namespace wmi

extern "C" {

int wmi_plan_chunks_host(const uint64_t *P, size_t n_samples, const wmi_chunk_params *params, int window, int64_t *out,
                         size_t cap, int32_t *n) {
    if (!n || (!P && n_samples > 0) || (!out && cap > 0)) return WMI_E_INVALID_ARG;
    if (n_samples > ((size_t)1 << 26)) return WMI_E_UNSUPPORTED;
    try {
        const wmi_chunk_params p = params ? *params : wmi_chunk_params{0, 0, 0, 0};
        int Cmax, Cmin, h;
        std::string err;
        int rc = wmi::chunk_resolve(p, window, &Cmax, &Cmin, &h, err);
        if (rc) return rc;
        const std::vector<int64_t> plan = wmi::chunk_plan(P, (int64_t)n_samples, Cmax, Cmin, h);
        *n = (int32_t)(plan.size() / 2);
        if (plan.size() > 2 * cap) return WMI_E_NO_SPACE;
        if (!plan.empty()) memcpy(out, plan.data(), plan.size() * 8);
    } catch (...) {
        return WMI_E_UNEXPECTED;
    }
    return WMI_OK;
}

// S6 of the header on the host: D row by row in int64, a trace byte a cell
int wmi_dtw_path_host(const int32_t *cost, int rows, int cols, int32_t *first) {
    if (!cost || !first || rows < 1 || rows > 513 || cols < 1 || cols > 1500) return WMI_E_INVALID_ARG;
    try {
        const int64_t INF = (int64_t)1 << 62;
        const size_t R = (size_t)rows, M = (size_t)cols;
        std::vector<uint8_t> trace(R * M);
        std::vector<int64_t> prev(M + 1, INF), cur(M + 1, INF);
        prev[0] = 0;
        for (size_t i = 1; i <= R; ++i) {
            cur[0] = INF;
            for (size_t j = 1; j <= M; ++j) {
                const int64_t c0 = prev[j - 1], c1 = prev[j], c2 = cur[j - 1];
                const int t = (c0 <= c1 && c0 <= c2) ? 0 : (c1 <= c2 ? 1 : 2);
                cur[j] = (int64_t)cost[(i - 1) * M + (j - 1)] + (t == 0 ? c0 : t == 1 ? c1 : c2);
                trace[(i - 1) * M + (j - 1)] = (uint8_t)t;
            }
            prev.swap(cur);
        }
        int i = rows, j = cols;
        for (int k = 0; k < rows + cols && i >= 1 && j >= 1; ++k) {
            first[i - 1] = j - 1;
            const int t = trace[(size_t)(i - 1) * M + (size_t)(j - 1)];
            if (t != 2) --i;
            if (t != 1) --j;
        }
    } catch (...) {
        return WMI_E_UNEXPECTED;
    }
    return WMI_OK;
}

const char *wmi_strerror(int status) {
    switch (status) {
        case WMI_OK: return "ok";
        case WMI_E_IO: return "Unexpected IO";
        case WMI_E_BAD_MAGIC: return "invalid model file (bad magic)";
        case WMI_E_NO_SPACE: return "not enough space";
        case WMI_E_UNKNOWN_TENSOR: return "unknown tensor in model file";
        case WMI_E_BAD_REF_TENSOR: return "invalid ref tensor";
        case WMI_E_WRONG_SIZE: return "tensor has wrong size in model file";
        case WMI_E_WRONG_SHAPE: return "tensor has wrong shape in model file";
        case WMI_E_WRONG_BYTES: return "tensor has wrong bytes in model file";
        case WMI_E_OP: return "tensor op error";
        case WMI_E_UNEXPECTED: return "Unexpected";
        case WMI_E_HIP: return "HIP error";
        case WMI_E_RCCL: return "RCCL error";
        case WMI_E_UNSUPPORTED: return "unsupported";
        case WMI_E_INVALID_ARG: return "invalid argument";
        default: return "unknown status";
    }
}

// convert_integer_to_float_audio (main.rs:1673-1679): f = s / 32768.0
int wmi_pcm16_to_f32(const int16_t *s16, size_t n, float *out) {
    if ((!s16 || !out) && n) return WMI_E_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = (float)s16[i] / 32768.0f;
    return WMI_OK;
}

int wmi_resample_plan(int32_t sample_rate, int32_t *L, int32_t *M, int32_t *K) {
    return wmi::resample_plan(sample_rate, L, M, K);
}

int wmi_resample_taps(int32_t sample_rate, float *h, size_t cap, size_t *n) {
    int32_t L, M, K;
    if (int rc = wmi::resample_plan(sample_rate, &L, &M, &K)) return rc;
    const size_t need = (size_t)L * 2 * (size_t)K;
    if (n) *n = need;
    if (!h || cap < need) return WMI_E_NO_SPACE;
    try {
        wmi::resample_taps(L, M, K, h, (size_t)2 * K);
    } catch (...) {
        return WMI_E_UNEXPECTED;
    }
    return WMI_OK;
}

int wmi_resampled_length(int32_t sample_rate, size_t n_frames, size_t *n_out) {
    int32_t L, M;
    if (int rc = wmi::resample_plan(sample_rate, &L, &M, nullptr)) return rc;
    size_t v = 0;
    if (!wmi::resampled_length(L, M, n_frames, &v)) return WMI_E_INVALID_ARG;
    if (n_out) *n_out = v;
    return WMI_OK;
}

int wmi_decode_alg_bytes(const wmi_hparams *hp, int rows, int steps, int beam, int q5, double *bytes_out,
                         double *flops_out) {
    if (!hp || rows < 1 || steps < 0 || !bytes_out) return WMI_E_INVALID_ARG;
    const double nt = hp->n_text_state, L = hp->n_text_layer, Tx = hp->n_audio_ctx, V = hp->n_vocab;
    // (q5_1 GEMVs: Wqkv, Wo, Wco, W0, W1 = 13 n^2 weights at 24 bytes a
    // 32-weight block; Wcq stays f16)
    const double w_mat = q5 ? 13.0 * nt * nt * 0.75 + 2.0 * nt * nt : 28.0 * nt * nt;
    const double w_step = L * (w_mat + 68.0 * nt) + V * nt * 2 + 2 * nt * 4;
    double bytes = 0, flops = 0;
    for (int b0 = 0; b0 < rows; b0 += beam ? rows : 8) {
        const double r = beam ? rows : (rows - b0 < 8 ? rows - b0 : 8);
        for (int pos = 0; pos < steps; ++pos) {
            bytes += w_step + r * (nt * 2 + nt * 4);                      // weights, token + position rows
            bytes += (beam ? 1.0 : r) * L * Tx * nt * 2 * 2;              // cross K, V (one clip's when beam)
            bytes += r * L * ((double)pos * nt * 2 * 2 + nt * 2 * 2);     // self K, V read + new row
            flops += r * (2.0 * L * (14.0 * nt * nt + 2.0 * Tx * nt + 2.0 * (pos + 1) * nt) + 2.0 * V * nt);
        }
    }
    *bytes_out = bytes;
    if (flops_out) *flops_out = flops;
    return WMI_OK;
}

}  // extern "C"
