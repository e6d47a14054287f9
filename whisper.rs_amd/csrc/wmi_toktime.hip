// wmi_toktime.hip — token-level timestamps (wmi_set_token_timestamps,
// wmi_token_times; DESIGN.md "Token-level timestamps"): the energy envelope of
// a recording, its running sum, and the voice-activity pass that moves each
// text token's start and end to where the envelope crosses the local mean.
//
// A translation unit of its own, as wmi_rules.hip: its code object is loaded
// with the first recording transcribed under the feature, so a context that
// never enables it runs on exactly the code objects it ran on before.
//
// Every quantity is an integer: a sample's magnitude in 2^-20 steps capped at
// 2^24, E the sum of 65 of them (uint32), P the running sum of E (uint64), and
// the comparisons 2 * ns * E against a difference of two P (uint64).  Any
// summation order gives the same bits, so the kernels reduce as they like.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_internal.h"

namespace wmi {

namespace {

constexpr int TT_TILE = 1024;   // samples a workgroup of k_energy / k_prefix
constexpr int TT_HALO = 32;     // samples each side of a sample in its E
constexpr int TT_WG = 256;

// a_i: min(rint(min(|x|, 16) * 2^20), 2^24), NaN -> 0 (the multiply is exact; rint rounds to nearest even)
__device__ __forceinline__ uint32_t tt_mag(float x) {
    if (x != x) return 0u;
    const float m = rintf(fminf(fabsf(x), 16.0f) * 1048576.0f);
    return (uint32_t)fminf(m, 16777216.0f);
}

// inclusive scan over the workgroup's NW waves (thread order); *total = the workgroup's sum
template <int NW>
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long *s_w,
                                                         unsigned long long *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
    #pragma unroll
    for (int i = 0; i < NW; ++i) {
        const unsigned long long x = s_w[i];
        if (i < w) pre += x;
        tot += x;
    }
    __syncthreads();  // (s_w may be written again)
    *total = tot;
    return v + pre;
}

}  // namespace

// E of a tile of TT_TILE samples: the magnitudes of the tile and of 32 samples
// each side lie in LDS as one dword a sample, in sample order.  Thread t owns
// the samples t, t + 256, t + 512 and t + 768 of the tile, so at every one of
// the 65 taps the lanes of a wave read 64 consecutive dwords (ds_read_b32: no
// two lanes of a 32-lane half on one bank).  Samples outside [0, N) count 0,
// which is the clipped range of the sum.  tsum[tile] = the tile's sum of E.
__global__ __launch_bounds__(TT_WG) void k_energy(const float *__restrict__ pcm, int N, uint32_t *__restrict__ E,
                                                  unsigned long long *__restrict__ tsum) {
    __shared__ __attribute__((aligned(16))) uint32_t s_a[TT_TILE + 2 * TT_HALO];
    __shared__ unsigned long long s_w[TT_WG / 64];
    const int tid = threadIdx.x;
    const int base = blockIdx.x * TT_TILE;  // (N <= 2^26)
    const int i4 = base + 4 * tid;
    float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i4 + 3 < N) {
        v = *reinterpret_cast<const float4 *>(pcm + i4);  // (the buffer and the tile start are 16-byte aligned)
    } else {
        if (i4 < N) v.x = pcm[i4];
        if (i4 + 1 < N) v.y = pcm[i4 + 1];
        if (i4 + 2 < N) v.z = pcm[i4 + 2];
    }
    uint4 q;
    q.x = i4 < N ? tt_mag(v.x) : 0u;
    q.y = i4 + 1 < N ? tt_mag(v.y) : 0u;
    q.z = i4 + 2 < N ? tt_mag(v.z) : 0u;
    q.w = i4 + 3 < N ? tt_mag(v.w) : 0u;
    *reinterpret_cast<uint4 *>(s_a + TT_HALO + 4 * tid) = q;
    if (tid < 2 * TT_HALO) {
        const int gi = tid < TT_HALO ? base - TT_HALO + tid : base + TT_TILE + (tid - TT_HALO);
        s_a[tid < TT_HALO ? tid : TT_TILE + tid] = gi >= 0 && gi < N ? tt_mag(pcm[gi]) : 0u;
    }
    __syncthreads();
    unsigned long long acc = 0;
    #pragma unroll
    for (int r = 0; r < TT_TILE / TT_WG; ++r) {
        const int li = tid + TT_WG * r;
        uint32_t e = 0;
        #pragma unroll
        for (int k = 0; k <= 2 * TT_HALO; ++k) e += s_a[li + k];
        if (base + li < N) {
            E[base + li] = e;
            acc += e;
        }
    }
    unsigned long long tot;
    (void)block_scan<TT_WG / 64>(acc, s_w, &tot);
    if (tid == 0) tsum[blockIdx.x] = tot;
}

// the tile sums -> the sum of the tiles before each (in place), one workgroup
__global__ __launch_bounds__(1024) void k_tile_scan(unsigned long long *tsum, int n_tiles) {
    __shared__ unsigned long long s_w[16];
    unsigned long long carry = 0;
    for (int c = 0; c < n_tiles; c += 1024) {
        const int i = c + (int)threadIdx.x;
        const unsigned long long v = i < n_tiles ? tsum[i] : 0ull;
        unsigned long long tot;
        const unsigned long long inc = block_scan<16>(v, s_w, &tot);
        if (i < n_tiles) tsum[i] = carry + inc - v;
        carry += tot;
    }
}

// P[i + 1] = the tile's offset + the sum of E over the tile's samples up to i; P[0] = 0
__global__ __launch_bounds__(TT_WG) void k_prefix(const uint32_t *__restrict__ E, int N,
                                                  const unsigned long long *__restrict__ toff,
                                                  unsigned long long *__restrict__ P) {
    __shared__ unsigned long long s_w[TT_WG / 64];
    const int tid = threadIdx.x;
    const int i4 = blockIdx.x * TT_TILE + 4 * tid;
    uint32_t e[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = i4 + k < N ? E[i4 + k] : 0u;
    const unsigned long long own = (unsigned long long)e[0] + e[1] + e[2] + e[3];
    unsigned long long tot;
    unsigned long long run = toff[blockIdx.x] + block_scan<TT_WG / 64>(own, s_w, &tot) - own;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        run += e[k];
        if (i4 + k < N) P[i4 + k + 1] = run;
    }
    if (blockIdx.x == 0 && tid == 0) P[0] = 0ull;
}

namespace {

// The walk `while (pred(j) && j != lim) j += dir` from j0, 256 samples at a
// time: every lane tests its own sample, a ballot and its first set bit give
// the wave's stop, the first wave with one gives the workgroup's (through LDS,
// one barrier a chunk: the two halves of s_hit alternate).  pred: ABOVE ?
// 2 ns E > S : 2 ns E < S.  A sample at or past lim (in the walk's direction)
// stops without being read, so with j0 and lim in [0, N) every read is, and
// the walk ends after at most N / 256 + 1 chunks.  The result is uniform.
template <bool ABOVE>
__device__ __forceinline__ long long vad_walk(const uint32_t *__restrict__ E, long long j0, int dir, long long lim,
                                              unsigned long long two_ns, unsigned long long S, int (*s_hit)[TT_WG / 64],
                                              int &par) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long long c = 0;; c += TT_WG) {
        const long long idx = j0 + dir * (c + tid);
        bool stop = dir > 0 ? idx >= lim : idx <= lim;
        if (!stop) {
            const unsigned long long x = two_ns * (unsigned long long)E[idx];
            stop = ABOVE ? !(x > S) : !(x < S);
        }
        const unsigned long long mask = __ballot(stop);
        if (lane == 0) s_hit[par][w] = mask ? __ffsll((long long)mask) - 1 : 64;
        __syncthreads();
        int hit = -1;
        #pragma unroll
        for (int i = TT_WG / 64 - 1; i >= 0; --i)
            if (s_hit[par][i] < 64) hit = 64 * i + s_hit[par][i];
        par ^= 1;
        if (hit >= 0) return j0 + dir * (c + hit);
    }
}

__device__ __forceinline__ long long clampll(long long x, long long lo, long long hi) { return x < lo ? lo : x > hi ? hi : x; }

}  // namespace

// Step C for one segment a workgroup, its text tokens in order (each token's
// start is held against the final end of the one before, its end against the
// start of the next).  Every thread carries the same scalars; thread 0 stores.
__global__ __launch_bounds__(TT_WG) void k_token_vad(VadArgs a) {
    __shared__ int s_hit[2][TT_WG / 64];
    int par = 0;
    const VadSeg sg = a.segs[blockIdx.x];
    const long long N = a.N;
    long long prev_t1 = 0;
    for (int k = 0; k < sg.m; ++k) {
        long long t0 = a.t0[sg.first + k], t1 = a.t1[sg.first + k];
        const long long next_t0 = k + 1 < sg.m ? a.t0[sg.first + k + 1] : 0;
        long long s0 = clampll(160 * t0, 0, N - 1), s1 = clampll(160 * t1, 0, N - 1);
        const long long ss0 = s0 - 2000 > 0 ? s0 - 2000 : 0, ss1 = s1 + 2000 < N ? s1 + 2000 : N;
        const unsigned long long two_ns = 2ull * (unsigned long long)(ss1 - ss0);
        const unsigned long long S = a.P[ss1] - a.P[ss0];
        // the start
        if (k > 0 && two_ns * (unsigned long long)a.E[s0] > S) {
            const long long j = vad_walk<true>(a.E, s0, -1, 0, two_ns, S, s_hit, par);
            t0 = j / 160;
            if (t0 < prev_t1) t0 = prev_t1;
            else s0 = j;
        } else {
            const long long j = vad_walk<false>(a.E, s0, 1, s1, two_ns, S, s_hit, par);
            s0 = j;
            t0 = j / 160;
        }
        // the end
        if (two_ns * (unsigned long long)a.E[s1] > S) {
            const long long j = vad_walk<true>(a.E, s1, 1, N - 1, two_ns, S, s_hit, par);
            t1 = j / 160;
            if (k + 1 < sg.m && t1 > next_t0) t1 = next_t0;
        } else {
            const long long j = vad_walk<false>(a.E, s1, -1, s0, two_ns, S, s_hit, par);
            t1 = j / 160;
        }
        if (threadIdx.x == 0) {
            a.t0[sg.first + k] = t0;
            a.t1[sg.first + k] = t1;
        }
        prev_t1 = t1;
    }
}

hipError_t launch_energy(hipStream_t s, const float *pcm, long long N, uint32_t *E, unsigned long long *tsum,
                         unsigned long long *P) {
    if (!pcm || !E || !tsum || !P || N < 1 || N > TT_MAX_SAMPLES) return hipErrorInvalidValue;
    const int n_tiles = (int)((N + TT_TILE - 1) / TT_TILE);
    hipLaunchKernelGGL(k_energy, dim3(n_tiles), dim3(TT_WG), 0, s, pcm, (int)N, E, tsum);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(1024), 0, s, tsum, n_tiles);
    hipLaunchKernelGGL(k_prefix, dim3(n_tiles), dim3(TT_WG), 0, s, E, (int)N, tsum, P);
    return hipGetLastError();
}

hipError_t launch_token_vad(hipStream_t s, const VadArgs &a, int n_segs) {
    if (!a.E || !a.P || !a.segs || !a.t0 || !a.t1 || a.N < 1 || a.N > TT_MAX_SAMPLES || n_segs < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_token_vad, dim3(n_segs), dim3(TT_WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
