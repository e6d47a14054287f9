// loader_check.cpp — the host-only unit (wmi_host.cpp) as a program of its own,
// built with ASan + UBSan by `make loader_check`: no device, nothing preloaded.
//
//   loader_check PATH...
// Each *.wav path goes through read_wav, any other through parse_file; one
// line per path, "<path>\t<status>\t<message>".  Exit status 0 whatever the
// statuses (a sanitizer report aborts), 2 on a usage error.
//   loader_check --token-times FILE
// The host steps of the token-level timestamps on the cases of FILE (below).
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "wmi_host.h"

using namespace wmi;

static size_t file_size(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    fseek(f, 0, SEEK_END);
    const long end = ftell(f);
    fclose(f);
    return end > 0 ? (size_t)end : 0;
}

// loader_check --token-times FILE: the host steps of the token-level
// timestamps (token_bounds, token_fill_others, split_segment; the device's
// voice-activity step between them is left out) on the cases of FILE, which
// tests/test_token_times.py writes and whose results it compares with its
// restatement.  Per case, whitespace-separated:
//   eot beg W T0 T1 thold_pt thold_ptsum max_len split_on_word n n_vocab
//   n_vocab entries: length, then that many byte values
//   n tokens: id tid pt ptsum              (floats as their uint32 bits)
// Out, per case: "case i", per token "t t0 t1 vlen-bits", per piece
// "p t0 t1 first count text-in-hex".
static float bits_f32(unsigned long long u) {
    const uint32_t v = (uint32_t)u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

static int token_times_cases(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) return 2;
    long long eot, beg, W, T0, T1, max_len, sow, n, nv;
    unsigned long long bpt, bps;
    for (int idx = 0; fscanf(f, "%lld %lld %lld %lld %lld %llu %llu %lld %lld %lld %lld", &eot, &beg, &W, &T0, &T1, &bpt, &bps,
                             &max_len, &sow, &n, &nv) == 11; ++idx) {
        if (n < 0 || nv < 0 || n > 100000 || nv > 100000) break;
        std::vector<std::string> vocab((size_t)nv);
        for (auto &s : vocab) {
            long long len = 0;
            if (fscanf(f, "%lld", &len) != 1 || len < 0 || len > 4096) { fclose(f); return 2; }
            for (long long k = 0; k < len; ++k) {
                int b = 0;
                if (fscanf(f, "%d", &b) != 1) { fclose(f); return 2; }
                s.push_back((char)b);
            }
        }
        std::vector<wmi_token_data> tok((size_t)n);
        for (auto &t : tok) {
            long long id, tid;
            unsigned long long pt, ps;
            if (fscanf(f, "%lld %lld %llu %llu", &id, &tid, &pt, &ps) != 4) { fclose(f); return 2; }
            t = wmi_token_data{(int32_t)id, (int32_t)tid, 0.0f, bits_f32(pt), bits_f32(ps), -1, -1, 0.0f};
        }
        TokParams p;
        p.thold_pt = bits_f32(bpt); p.thold_ptsum = bits_f32(bps);
        p.max_len = (int32_t)max_len; p.split_on_word = (int32_t)sow;
        token_bounds(vocab, (int32_t)eot, (int32_t)beg, p, W, T0, T1, tok.data(), (int)n);
        token_fill_others((int32_t)eot, T0, T1, tok.data(), (int)n);
        printf("case %d\n", idx);
        for (const auto &t : tok) {
            uint32_t vb;
            memcpy(&vb, &t.vlen, 4);
            printf("t %lld %lld %u\n", (long long)t.t0, (long long)t.t1, vb);
        }
        for (const TokPiece &pc : split_segment(vocab, (int32_t)eot, p, T0, T1, tok.data(), (int)n)) {
            printf("p %lld %lld %d %d ", (long long)pc.t0, (long long)pc.t1, pc.first, pc.count);
            for (const char c : pc.text) printf("%02x", (unsigned)(unsigned char)c);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "--token-times")) return token_times_cases(argv[2]);
    if (argc < 2) {
        fprintf(stderr, "usage: %s PATH...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        const char *path = argv[i];
        const size_t n = strlen(path);
        std::string err;
        int rc;
        if (n >= 4 && !strcmp(path + n - 4, ".wav")) {
            size_t ns = 0;
            rc = read_wav(path, nullptr, 0, &ns, nullptr, nullptr, err);
            // the claimed count as capacity, a buffer no larger than the file: a data
            // chunk beyond the file must be refused before a sample is written
            std::vector<int16_t> pcm(std::min(ns, file_size(path) / 2 + 1));
            if (!rc) rc = read_wav(path, pcm.data(), ns, &ns, nullptr, nullptr, err);
        } else {
            ParsedModel pm;
            rc = parse_file(path, pm, err);
        }
        printf("%s\t%d\t%s\n", path, rc, err.c_str());
    }
    return 0;
}
