// wmi_chunks.hip — chunked long-form transcription (wmi_set_chunking; DESIGN.md
// "Chunked long-form transcription"): the plan that cuts a recording at quiet
// places, and the encoder's window kernel with a per-slot end.
//
// A translation unit of its own, as wmi_toktime.hip: a context that never
// enables the feature launches nothing of it, and the units it does launch
// from are the ones they were.
#include <hip/hip_runtime.h>

#include "wmi_device.h"
#include "wmi_internal.h"

namespace wmi {

namespace {

constexpr int CK_WG = 256;

// the smaller S, of equal ones the larger k (k < 0: no candidate)
__device__ __forceinline__ void ck_take(unsigned long long &S, int &k, unsigned long long S2, int k2) {
    if (k2 >= 0 && (k < 0 || S2 < S || (S2 == S && k2 > k))) { S = S2; k = k2; }
}

}  // namespace

// One workgroup a recording walks the chain of cuts: the candidates k in
// [s + Cmin, s + Cmax] spread over the threads (two P loads each), each thread
// keeps its best, the wave reduces by shuffles, the workgroup through LDS.
// Every thread then holds the cut, so the chain needs no round trip.  A cut is
// only looked for while n_len - s > Cmax: every candidate k < n_len, so
// 160 (k - h) <= 160 k <= N and both P indices lie in [0, N].  s grows by at
// least Cmin >= 1 a cut, the list by one pair: at most n_len / Cmin + 1 pairs
// (r.cap guards the store all the same).  The order of the reduction does not
// matter: (S, k) is a total order.
__global__ __launch_bounds__(CK_WG) void k_chunk_plan(const ChunkPlanRec *recs, int Cmax, int Cmin, int h) {
    __shared__ unsigned long long s_S[2][CK_WG / 64];
    __shared__ int s_k[2][CK_WG / 64];
    const ChunkPlanRec r = recs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long N = r.N, n_len = N / 160;
    long long s = 0;
    int n = 0, par = 0;
    while (n_len - s > Cmax) {
        unsigned long long S = 0;
        int k = -1;
        for (long long c = s + Cmin + tid; c <= s + Cmax; c += CK_WG) {
            const long long hi = 160 * (c + h) < N ? 160 * (c + h) : N, lo = c > h ? 160 * (c - h) : 0;
            ck_take(S, k, r.P[hi] - r.P[lo], (int)(c - s));
        }
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long S2 = __shfl_xor(S, d);
            const int k2 = __shfl_xor(k, d);
            ck_take(S, k, S2, k2);
        }
        if (lane == 0) { s_S[par][w] = S; s_k[par][w] = k; }
        __syncthreads();  // (the two halves alternate: one barrier a cut)
        S = s_S[par][0];
        k = s_k[par][0];
        #pragma unroll
        for (int i = 1; i < CK_WG / 64; ++i) ck_take(S, k, s_S[par][i], s_k[par][i]);
        par ^= 1;
        if (tid == 0 && n < r.cap) { r.out[2 * n] = s; r.out[2 * n + 1] = s + k; }
        ++n;
        s += k;  // (k >= Cmin: Cmin <= Cmax leaves thread 0 a candidate)
    }
    if (tid == 0) {
        if (n_len > 0) {
            if (n < r.cap) { r.out[2 * n] = s; r.out[2 * n + 1] = n_len; }
            ++n;
        }
        *r.count = n;
    }
}

hipError_t launch_chunk_plan(hipStream_t s, const ChunkPlanRec *recs, int n_recs, int Cmax, int Cmin, int h) {
    if (!recs || n_recs < 1 || Cmin < 1 || Cmin > Cmax || Cmax > (1 << 20) || h < 1 || h > 100) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chunk_plan, dim3(n_recs), dim3(CK_WG), 0, s, recs, Cmax, Cmin, h);
    return hipGetLastError();
}

// k_mel_window with slot b's window ending at frame end[b] of its recording
// (a chunk's end; at most the recording's frames): zero from there on, which
// is what a window past the recording's end gets.
__global__ void k_mel_window_end(const float *mel, int64_t mel_stride, int n_mel, const int64_t *n_len,
                                 const int32_t *src, const int32_t *off, const int32_t *end, int T2, int Cp, uint16_t *xconv,
                                 float *xconv32, uint16_t *g1, int n) {
    const int b = blockIdx.y;
    const int clip = src[b];
    const int64_t mel_offset = off[b];
    // (conv2's zero padding rows of g1, as k_mel_window)
    if (g1)
        for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < 2 * (int64_t)n;
             idx += (int64_t)gridDim.x * blockDim.x)
            g1[((int64_t)b * (T2 + 2) + (idx < n ? 0 : T2 + 1)) * n + (idx < n ? idx : idx - n)] = 0;
    const int64_t nl = n_len[clip];
    const int64_t lim = end[b] < nl ? (end[b] > 0 ? end[b] : 0) : nl;
    const int64_t tot = (int64_t)(T2 + 2) * Cp;
    const int64_t i0 = mel_offset < lim ? mel_offset : lim;
    const int64_t i1 = mel_offset + T2 < lim ? mel_offset + T2 : lim;
    const float *p = mel + (int64_t)clip * mel_stride;
    uint16_t *o = xconv + (int64_t)b * tot;
    float *o32 = xconv32 ? xconv32 + (int64_t)b * tot : nullptr;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / Cp;
        const int c = (int)(idx - row * Cp);
        const int64_t t = row - 1;
        float v = 0.0f;
        if (t >= 0 && t < T2 && c < n_mel && i0 + t < i1) v = p[(int64_t)c * nl + i0 + t];
        if (xconv32) o32[idx] = v;
        else o[idx] = f2h_bits(v);
    }
}

hipError_t launch_mel_window_end(hipStream_t s, const float *mel, int64_t mel_stride, int n_mel, const int64_t *n_len, int T2,
                                 int Cp, uint16_t *xconv, int slots, float *xconv32, uint16_t *g1, int n, const int32_t *src,
                                 const int32_t *off, const int32_t *end) {
    if (!src || !off || !end || slots < 1 || slots > DEC_ROWS) return hipErrorInvalidValue;
    const int64_t tot = (int64_t)(T2 + 2) * Cp;
    const int64_t g = (tot + 1023) / 1024;
    dim3 grid((unsigned)(g < 512 ? g : 512), slots);
    hipLaunchKernelGGL(k_mel_window_end, grid, dim3(256), 0, s, mel, mel_stride, n_mel, n_len, src, off, end, T2, Cp, xconv,
                       xconv32, g1, n);
    return hipGetLastError();
}

}  // namespace wmi
