// audio_check.cpp — the audio front end's host side (wmi_host.cpp: the plan,
// the taps, the lengths) as a program of its own, built with ASan + UBSan by
// `make audio_check`: no device, nothing preloaded.
//
//   audio_check
// For every rate the header lists and for rejected ones: the plan, the whole
// table into a buffer of exactly its size (every row's sum and the table's
// extremes are printed), the too-small-buffer answer, and N_out for a few
// lengths up to SIZE_MAX.  One line per rate.  Exit status 0 if every answer
// is the expected kind (a sanitizer report aborts), 1 otherwise.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "wmi_host.h"

int main() {
    const int32_t listed[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000,
                              4000, 384000};
    const int32_t rejected[] = {0, -1, 3999, 16001, 400000, 384001, 44101, INT32_MAX, INT32_MIN};
    const size_t lengths[] = {0, 1, 2, 159, 160, 3001, 480000, 1440000, ((size_t)1 << 31) - 1, SIZE_MAX / 640, SIZE_MAX};
    int bad = 0;
    for (const int32_t R : listed) {
        int32_t L = 0, M = 0, K = 0;
        int rc = wmi_resample_plan(R, &L, &M, &K);
        size_t n = 0;
        const int rc0 = wmi_resample_taps(R, nullptr, 0, &n);
        if (rc || rc0 != WMI_E_NO_SPACE || n != (size_t)L * 2 * (size_t)K) { printf("%d\tplan %d taps %d\n", R, rc, rc0); bad = 1; continue; }
        std::vector<float> h(n);
        std::vector<float> small(n ? n - 1 : 0);
        const int rc1 = wmi_resample_taps(R, small.data(), small.size(), nullptr);
        rc = wmi_resample_taps(R, h.data(), h.size(), &n);
        if (rc || rc1 != WMI_E_NO_SPACE) { printf("%d\ttaps %d small %d\n", R, rc, rc1); bad = 1; continue; }
        double dev = 0.0;
        float lo = h[0], hi = h[0];
        for (int32_t ph = 0; ph < L; ++ph) {
            double s = 0.0;
            for (int32_t j = 0; j < 2 * K; ++j) {
                const float v = h[(size_t)ph * 2 * K + j];
                if (!(v == v)) bad = 1;
                s += (double)v;
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            dev = fmax(dev, fabs(s - 1.0));
        }
        printf("%d\tL %d M %d K %d taps %zu row-sum dev %.3g min %.9g max %.9g lengths", R, L, M, K, n, dev, (double)lo, (double)hi);
        for (const size_t N : lengths) {
            size_t no = 0;
            const int rl = wmi_resampled_length(R, N, &no);
            if (rl == WMI_OK) printf(" %zu", no);
            else printf(" (%d)", rl);
        }
        printf("\n");
        if (dev > 1e-5) bad = 1;
    }
    for (const int32_t R : rejected) {
        int32_t L = -7, M = -7, K = -7;
        size_t n = 99, no = 99;
        float one = 0.0f;
        const int a = wmi_resample_plan(R, &L, &M, &K), b = wmi_resample_taps(R, &one, 1, &n), c = wmi_resampled_length(R, 1000, &no);
        printf("%d\trejected %d %d %d\n", R, a, b, c);
        if (a != WMI_E_UNSUPPORTED || b != WMI_E_UNSUPPORTED || c != WMI_E_UNSUPPORTED || L != -7 || n != 99 || no != 99) bad = 1;
    }
    printf(bad ? "audio_check FAILED\n" : "audio_check ok\n");
    return bad;
}
