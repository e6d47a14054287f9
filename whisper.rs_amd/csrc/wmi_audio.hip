// wmi_audio.hip — audio of any format (wmi_audio_to_mel_batch, wmi_stage_audio,
// wmi_transcribe_audio*; DESIGN.md "Audio front end"): the downmix and
// conversion of raw interleaved s16 / f32 frames to mono f32, and the
// band-limited polyphase resampler to 16 kHz.
//
// A translation unit of its own, as wmi_toktime.hip: its code object is loaded
// with the first clip that is not 16 kHz mono f32, so a context that is only
// given such clips runs on exactly the code objects it ran on before.
//
// The header states every output as one expression of its own inputs (a
// frame: one division in double; an output: four chains of exact f32 x f32
// products summed in double, in tap order), so the tile shape, the chunking of
// a clip and the launch order change no bit.
#include <hip/hip_runtime.h>

#include "wmi_internal.h"

namespace wmi {

namespace {

constexpr int AU_WG = 256;

// one frame's mono value from its C samples e[0..C)
template <int C>
__device__ __forceinline__ float mono_s16(const int16_t *e) {
    int s = 0;
    #pragma unroll
    for (int c = 0; c < C; ++c) s += (int)e[c];
    return (float)((double)s / (32768.0 * (double)C));
}
template <int C>
__device__ __forceinline__ float mono_f32(const float *e) {
    if (C == 1) return e[0];
    double s = 0.0;
    #pragma unroll
    for (int c = 0; c < C; ++c) s += (double)e[c];
    return (float)(s / (double)C);
}

}  // namespace

// Downmix and conversion.  A lane owns G consecutive frames, 16 * C bytes of
// raw input (G = 8 frames of s16, 4 of f32): C loads of 16 bytes, held in
// registers under compile-time indices, and G floats out as 16-byte stores.
// The clip's last lane group, if it is not whole, goes frame by frame, so no
// read passes the n frames.
template <int C, bool S16>
__global__ __launch_bounds__(AU_WG) void k_audio_mono(const void *__restrict__ raw, long long n, float *__restrict__ out) {
    constexpr int G = S16 ? 8 : 4;
    const long long g = (long long)blockIdx.x * AU_WG + threadIdx.x;
    const long long f0 = g * G;
    if (f0 >= n) return;
    if (f0 + G <= n) {
        union { uint4 q[C]; int16_t h[8 * C]; float f[4 * C]; } u;
        const uint4 *src = reinterpret_cast<const uint4 *>(raw) + g * C;
        #pragma unroll
        for (int k = 0; k < C; ++k) u.q[k] = src[k];
        float o[G];
        #pragma unroll
        for (int i = 0; i < G; ++i) o[i] = S16 ? mono_s16<C>(u.h + i * C) : mono_f32<C>(u.f + i * C);
        float4 *dst = reinterpret_cast<float4 *>(out + f0);
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        if (S16) dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    } else {
        for (long long f = f0; f < n; ++f)
            out[f] = S16 ? mono_s16<C>(reinterpret_cast<const int16_t *>(raw) + f * C)
                         : mono_f32<C>(reinterpret_cast<const float *>(raw) + f * C);
    }
}

// The resampler: a workgroup owns AU_WG consecutive outputs, a lane one.  The
// tile's input span, frames [i0(first) - K + 1, i0(last) + K], lies in LDS as
// one dword a frame (a frame outside the clip or outside the chunk buffer is
// stored as 0 without being read); lane n reads its 2K frames from there at
// stride M / L between lanes and its phase's taps from the table, 16 bytes at a
// time (a row starts 16-byte aligned).  UNI (L = 1): one phase, the tap loads
// are wave-uniform.  The four chains take j = 0, 1, 2, 3 (mod 4) in ascending
// order; 2K is even, so past the last whole four there are two taps or none.
template <bool UNI>
__global__ __launch_bounds__(AU_WG) void k_audio_fir(FirArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const int tid = threadIdx.x;
    const long long nb = a.n_lo + (long long)blockIdx.x * AU_WG;
    const long long nl = nb + AU_WG - 1 < a.n_hi - 1 ? nb + AU_WG - 1 : a.n_hi - 1;
    const long long i_first = nb * a.M / a.L, i_last = nl * a.M / a.L;
    const long long base = i_first - a.K + 1;
    const int span = (int)(i_last - i_first) + 2 * a.K;
    for (int t = tid; t < span; t += AU_WG) {
        const long long f = base + t, idx = f - a.x0;
        s_x[t] = f >= 0 && f < a.N && idx >= 0 && idx < a.xn ? a.x[idx] : 0.0f;
    }
    __syncthreads();
    const long long n = nb + tid;
    if (n >= a.n_hi) return;
    const long long p = n * a.M, i0 = p / a.L;
    const int ph = UNI ? 0 : (int)(p - i0 * a.L);
    const float *__restrict__ hr = a.h + (size_t)ph * a.hs;
    const float *xs = s_x + (int)(i0 - i_first);
    const int K2 = 2 * a.K, J4 = K2 & ~3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    #pragma unroll 2
    for (int j = 0; j < J4; j += 4) {
        const float4 hv = *reinterpret_cast<const float4 *>(hr + j);
        s0 += (double)hv.x * (double)xs[j];
        s1 += (double)hv.y * (double)xs[j + 1];
        s2 += (double)hv.z * (double)xs[j + 2];
        s3 += (double)hv.w * (double)xs[j + 3];
    }
    if (J4 < K2) {
        s0 += (double)hr[J4] * (double)xs[J4];
        s1 += (double)hr[J4 + 1] * (double)xs[J4 + 1];
    }
    a.y[n] = (float)((s0 + s1) + (s2 + s3));
}

namespace {

template <int C>
void mono_launch(hipStream_t s, const void *raw, long long n, int s16, float *out) {
    const long long G = s16 ? 8 : 4, lanes = (n + G - 1) / G;
    const dim3 grid((unsigned)((lanes + AU_WG - 1) / AU_WG));
    if (s16) hipLaunchKernelGGL((k_audio_mono<C, true>), grid, dim3(AU_WG), 0, s, raw, n, out);
    else hipLaunchKernelGGL((k_audio_mono<C, false>), grid, dim3(AU_WG), 0, s, raw, n, out);
}

}  // namespace

hipError_t launch_audio_mono(hipStream_t s, const void *raw, long long n, int C, int s16, float *out) {
    if (!raw || !out || n < 1 || n > AUDIO_CHUNK_MAX + (1 << 13) || ((uintptr_t)raw & 15) || ((uintptr_t)out & 15))
        return hipErrorInvalidValue;
    switch (C) {
        case 1: mono_launch<1>(s, raw, n, s16, out); break;
        case 2: mono_launch<2>(s, raw, n, s16, out); break;
        case 3: mono_launch<3>(s, raw, n, s16, out); break;
        case 4: mono_launch<4>(s, raw, n, s16, out); break;
        case 5: mono_launch<5>(s, raw, n, s16, out); break;
        case 6: mono_launch<6>(s, raw, n, s16, out); break;
        case 7: mono_launch<7>(s, raw, n, s16, out); break;
        case 8: mono_launch<8>(s, raw, n, s16, out); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_audio_fir(hipStream_t s, const FirArgs &a) {
    if (!a.x || !a.h || !a.y || a.L < 1 || a.M < 1 || a.K < 1 || a.hs < 2 * a.K || (a.hs & 3) || ((uintptr_t)a.h & 15) ||
        a.xn < 1 || a.n_lo < 0 || a.n_hi <= a.n_lo || a.n_hi - a.n_lo > (1ll << 31))
        return hipErrorInvalidValue;
    // the widest tile span: outputs AU_WG - 1 apart start at most ceil((AU_WG - 1) M / L) frames apart
    const long long span = ((long long)(AU_WG - 1) * a.M + a.L - 1) / a.L + 2ll * a.K;
    const size_t lds = (size_t)((span + 3) & ~3ll) * 4;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n_hi - a.n_lo + AU_WG - 1) / AU_WG));
    if (a.L == 1) hipLaunchKernelGGL((k_audio_fir<true>), grid, dim3(AU_WG), lds, s, a);
    else hipLaunchKernelGGL((k_audio_fir<false>), grid, dim3(AU_WG), lds, s, a);
    return hipGetLastError();
}

}  // namespace wmi
