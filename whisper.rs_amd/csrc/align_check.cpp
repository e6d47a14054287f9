// align_check.cpp — the host side of the token alignment (wmi_host.cpp:
// wmi_dtw_path_host, wmi_set_dtw's checks) as a program of its own, built with
// ASan + UBSan by `make align_check`: no device, nothing preloaded.
//
//   align_check [FILE]
// FILE holds cost matrices, each as int32 rows, int32 cols and rows * cols
// int32 costs (native byte order), one after the other.  For each the path
// goes into a buffer of exactly `rows` entries and is printed as
//   path <rows> <cols> <status> <f[0]> ... <f[rows-1]>
// (a refused shape carries no costs and prints its status alone).  Then the
// parameter checks against a model of 4 text layers and 6 heads, one line
// each: `dtw <name> <status> <pairs> [<layer>,<head> ...]`.  Exit status 0 if
// the file parsed and every built-in answer is the expected kind (a sanitizer
// report aborts), 1 otherwise.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "wmi_host.h"

static int check_params() {
    wmi_hparams hp{};
    hp.n_text_layer = 4;
    hp.n_text_head = 6;
    const int32_t two[] = {3, 5, 0, 0}, dup[] = {1, 2, 3, 0, 1, 2}, out_l[] = {4, 0}, out_h[] = {0, 6}, neg[] = {-1, 0};
    std::vector<int32_t> many;
    for (int i = 0; i < 33; ++i) { many.push_back(i / 6 % 4); many.push_back(i % 6); }
    struct Case { const char *name; wmi_dtw_params p; int want; };
    const Case cases[] = {
        {"off_default", {0, 0, nullptr, 0, 7}, WMI_OK},
        {"on_empty", {1, 0, nullptr, 0, 7}, WMI_E_INVALID_ARG},
        {"two_pairs", {1, 0, two, 2, 7}, WMI_OK},
        {"n_top_2", {1, 2, nullptr, 0, 1}, WMI_OK},
        {"n_top_4", {1, 4, nullptr, 0, 15}, WMI_OK},
        {"n_top_5", {1, 5, nullptr, 0, 7}, WMI_E_INVALID_ARG},
        {"heads_win_over_n_top", {0, 9, two, 1, 3}, WMI_OK},
        {"duplicate", {1, 0, dup, 3, 7}, WMI_E_INVALID_ARG},
        {"layer_outside", {1, 0, out_l, 1, 7}, WMI_E_INVALID_ARG},
        {"head_outside", {1, 0, out_h, 1, 7}, WMI_E_INVALID_ARG},
        {"negative", {1, 0, neg, 1, 7}, WMI_E_INVALID_ARG},
        {"33_pairs", {1, 0, many.data(), 33, 7}, WMI_E_INVALID_ARG},
        {"null_heads", {1, 0, nullptr, 2, 7}, WMI_E_INVALID_ARG},
        {"width_even", {1, 1, nullptr, 0, 6}, WMI_E_INVALID_ARG},
        {"width_0", {0, 0, nullptr, 0, 0}, WMI_E_INVALID_ARG},
        {"width_17", {1, 1, nullptr, 0, 17}, WMI_E_INVALID_ARG},
        {"width_negative", {1, 1, nullptr, 0, -7}, WMI_E_INVALID_ARG},
    };
    int bad = 0;
    for (const Case &c : cases) {
        std::vector<int32_t> pairs;
        std::string err;
        const int rc = wmi::dtw_head_table(hp, c.p, pairs, err);
        printf("dtw %s %d %zu", c.name, rc, pairs.size() / 2);
        for (size_t k = 0; k + 1 < pairs.size(); k += 2) printf(" %d,%d", pairs[k], pairs[k + 1]);
        printf("\n");
        if (rc != c.want || (rc != WMI_OK && err.empty())) bad = 1;
    }
    // 8 heads a layer: n_top = 5 of 6 layers selects 40
    hp.n_text_layer = 6;
    hp.n_text_head = 8;
    std::vector<int32_t> pairs;
    std::string err;
    const wmi_dtw_params p40{1, 5, nullptr, 0, 7}, p32{1, 4, nullptr, 0, 7};
    const int r40 = wmi::dtw_head_table(hp, p40, pairs, err), r32 = wmi::dtw_head_table(hp, p32, pairs, err);
    printf("dtw n_top_40_heads %d 0\ndtw n_top_32_heads %d %zu\n", r40, r32, pairs.size() / 2);
    if (r40 != WMI_E_INVALID_ARG || r32 != WMI_OK || pairs.size() != 64) bad = 1;
    return bad;
}

static int check_shapes() {
    int32_t c = 0, f = -7;
    const int shapes[][2] = {{0, 1}, {1, 0}, {-1, 5}, {514, 1}, {1, 1501}};
    int bad = 0;
    for (const auto &s : shapes) {
        const int rc = wmi_dtw_path_host(&c, s[0], s[1], &f);
        printf("shape %d %d %d\n", s[0], s[1], rc);
        if (rc != WMI_E_INVALID_ARG || f != -7) bad = 1;
    }
    if (wmi_dtw_path_host(nullptr, 1, 1, &f) != WMI_E_INVALID_ARG || wmi_dtw_path_host(&c, 1, 1, nullptr) != WMI_E_INVALID_ARG) bad = 1;
    return bad;
}

int main(int argc, char **argv) {
    int bad = 0;
    if (argc > 1) {
        FILE *fp = fopen(argv[1], "rb");
        if (!fp) { printf("cannot open %s\n", argv[1]); return 1; }
        for (;;) {
            int32_t hd[2];
            const size_t got = fread(hd, 4, 2, fp);
            if (got == 0) break;
            if (got != 2) { bad = 1; break; }
            if (hd[0] < 1 || hd[0] > 513 || hd[1] < 1 || hd[1] > 1500) {
                int32_t c = 0, f = 0;
                printf("path %d %d %d\n", hd[0], hd[1], wmi_dtw_path_host(&c, hd[0], hd[1], &f));
                continue;
            }
            std::vector<int32_t> cost((size_t)hd[0] * (size_t)hd[1]), first((size_t)hd[0], -1);
            if (fread(cost.data(), 4, cost.size(), fp) != cost.size()) { bad = 1; break; }
            const int rc = wmi_dtw_path_host(cost.data(), hd[0], hd[1], first.data());
            printf("path %d %d %d", hd[0], hd[1], rc);
            for (int32_t v : first) printf(" %d", v);
            printf("\n");
            if (rc) bad = 1;
        }
        fclose(fp);
    }
    bad |= check_shapes();
    bad |= check_params();
    printf(bad ? "align_check FAILED\n" : "align_check ok\n");
    return bad;
}
