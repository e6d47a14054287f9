// wmi_align.hip — token times from cross-attention alignment (wmi_set_dtw,
// wmi_align_tokens, wmi_dtw_path; DESIGN.md "Token times from cross-attention
// alignment"; the header states S1 - S7): the capture of a chain step's
// cross-attention scores, the cost matrix from them, and dynamic time warping
// over it.
//
// A translation unit of its own, as wmi_rules.hip and wmi_toktime.hip: its
// code object is loaded with the first aligned pass, so a context that never
// enables the feature runs on exactly the code objects it ran on before.
//
// The capture copies bits.  S2 - S5 are a float front end in double whose
// summation orders are the kernels' own; the cost is an integer from S5 on and
// S6 is exact in int64, so the path is a function of the cost matrix alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_internal.h"

namespace wmi {

namespace {

constexpr int AL_WG = 256;
constexpr long long AL_INF = 1ll << 62;  // (a path's cost stays inside (513 + 1500) * 2^30)

__device__ __forceinline__ double al_wave_sum(double v) {
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float al_wave_max(float v) {
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

}  // namespace

// S1: after a layer's cross-attention launch of an aligned step (one row, so
// S holds [H][s_stride]) workgroup g copies head[g]'s T scores to
// s[slot[g]][pos][0 .. T).  pos comes from the step state, as in
// k_logits_capture, and the pass's positions from *np, so a captured graph
// replays the launch for every pass of the same head table.
__global__ __launch_bounds__(AL_WG) void k_align_capture(AlCapArgs a) {
    const int pos = a.st->pos, Np = *a.np;
    if (pos < 0 || pos >= Np || Np > a.np_max) return;
    const float *src = a.S + (int64_t)a.head[blockIdx.x] * a.s_stride;
    float *dst = a.s + ((int64_t)a.slot[blockIdx.x] * Np + pos) * a.T;
    for (int j = threadIdx.x; j < a.T; j += AL_WG) dst[j] = src[j];
}

// S2: one workgroup a row (a, i): the maximum over the M real frames, then
// w32 = (float)(exp((double)s - m) / Z) with Z the double sum (lanes, waves in
// order).  T <= 1500: a thread holds at most AL_SU of the row's scores.
constexpr int AL_SU = (AL_COLS_MAX + AL_WG - 1) / AL_WG;
__global__ __launch_bounds__(AL_WG) void k_align_softmax(AlMatArgs a) {
    __shared__ float s_m[AL_WG / 64];
    __shared__ double s_z[AL_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *row = a.s + (int64_t)blockIdx.x * a.T;
    float *out = a.w + (int64_t)blockIdx.x * a.M;
    float sv[AL_SU];
    float m = -INFINITY;
    #pragma unroll
    for (int u = 0; u < AL_SU; ++u) {
        const int j = tid + AL_WG * u;
        sv[u] = j < a.M ? row[j] : -INFINITY;
        m = fmaxf(m, sv[u]);
    }
    m = al_wave_max(m);
    if (lane == 0) s_m[wv] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    double e[AL_SU], z = 0.0;
    #pragma unroll
    for (int u = 0; u < AL_SU; ++u) {
        const int j = tid + AL_WG * u;
        e[u] = j < a.M ? exp((double)sv[u] - (double)m) : 0.0;
        z += e[u];
    }
    z = al_wave_sum(z);
    if (lane == 0) s_z[wv] = z;
    __syncthreads();
    const double Z = ((s_z[0] + s_z[1]) + s_z[2]) + s_z[3];
    #pragma unroll
    for (int u = 0; u < AL_SU; ++u) {
        const int j = tid + AL_WG * u;
        if (j < a.M) out[j] = (float)(e[u] / Z);
    }
}

// S3, in place: a workgroup takes 64 columns j of one head a; its four waves
// each take every fourth position i, so a wave reads 64 consecutive floats of
// a row.  Mean and deviation over all Np positions in double, the four waves'
// partial sums added in wave order.  An element is read and rewritten by the
// one thread that owns it.
__global__ __launch_bounds__(AL_WG) void k_align_zscore(AlMatArgs a) {
    __shared__ double s_p[AL_WG / 64][64];
    const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    const bool on = j < a.M;
    float *col = a.w + (int64_t)blockIdx.y * a.Np * a.M + (on ? j : 0);
    double sum = 0.0;
    for (int i = sl; i < a.Np && on; i += AL_WG / 64) sum += (double)col[(int64_t)i * a.M];
    s_p[sl][c] = sum;
    __syncthreads();
    const double mu = (((s_p[0][c] + s_p[1][c]) + s_p[2][c]) + s_p[3][c]) / (double)a.Np;
    __syncthreads();
    double var = 0.0;
    for (int i = sl; i < a.Np && on; i += AL_WG / 64) {
        const double d = (double)col[(int64_t)i * a.M] - mu;
        var += d * d;
    }
    s_p[sl][c] = var;
    __syncthreads();
    const double sd = sqrt((((s_p[0][c] + s_p[1][c]) + s_p[2][c]) + s_p[3][c]) / (double)a.Np);
    for (int i = sl; i < a.Np && on; i += AL_WG / 64) {
        const double v = (double)col[(int64_t)i * a.M];
        col[(int64_t)i * a.M] = sd == 0.0 ? 0.0f : (float)((v - mu) / sd);
    }
}

// S4 + S5: one thread a cell (r, j) of the cost matrix.  Per head, in the
// caller's order, the W taps of row p - 1 + r around j (reflected at both ends)
// lie in registers and the h-th order statistic is the tap that has exactly h
// taps in front of it, ties by tap index; the heads' medians are summed in
// double.  W = 1 is the unfiltered value (also taken for M <= h).
template <int W>
__global__ __launch_bounds__(AL_WG) void k_align_cost(AlMatArgs a) {
    constexpr int HW = W / 2;
    const int cell = blockIdx.x * AL_WG + threadIdx.x;
    if (cell >= (a.n + 1) * a.M) return;
    const int r = cell / a.M, j = cell - r * a.M;
    int idx[W];
    #pragma unroll
    for (int k = 0; k < W; ++k) {
        int t = j + k - HW;
        if (t < 0) t = -t;
        if (t > a.M - 1) t = 2 * (a.M - 1) - t;
        idx[k] = t;
    }
    double sum = 0.0;
    for (int h = 0; h < a.A; ++h) {
        const float *row = a.w + ((int64_t)h * a.Np + (a.p - 1 + r)) * a.M;
        float v[W];
        #pragma unroll
        for (int k = 0; k < W; ++k) v[k] = row[idx[k]];
        float med = v[0];
        #pragma unroll
        for (int t = 0; t < W; ++t) {
            int rank = 0;
            #pragma unroll
            for (int u = 0; u < W; ++u) rank += (v[u] < v[t] || (v[u] == v[t] && u < t)) ? 1 : 0;
            if (rank == HW) med = v[t];
        }
        sum += (double)med;
    }
    const double c = -(1.0 / (double)a.A) * sum;
    const double q = fmin(fmax(rint(c * 65536.0), -1073741824.0), 1073741824.0);
    a.cq[cell] = (int32_t)q;
}

// S6: one workgroup, thread r owns row r of the R x M matrix and sweeps the
// R + M - 1 anti-diagonals: on diagonal d it holds column d - r.  Its left
// neighbour D(r, j - 1) is its own last value (a register); D(r - 1, j) and
// D(r - 1, j - 1) are thread r - 1's values of the two diagonals before, which
// lie in LDS as int64 (three buffers in turn: the one written on diagonal d was
// last read on d - 1, before that diagonal's barrier).  One barrier a
// diagonal.  The trace byte of cell (r, j) goes to trace[d * R + r], so a
// wave's stores of a diagonal are consecutive bytes.  After the sweep thread 0
// walks the trace back from (R - 1, M - 1): at most R + M - 1 cells.
__global__ __launch_bounds__(AL_DTW_WG) void k_dtw(const int32_t *__restrict__ cq, int R, int M, uint8_t *trace,
                                                   int32_t *first) {
    __shared__ long long s_d[3][AL_DTW_WG];
    const int r = threadIdx.x;
    const int nd = R + M - 1 < AL_ROWS_MAX + AL_COLS_MAX - 1 ? R + M - 1 : AL_ROWS_MAX + AL_COLS_MAX - 1;
    long long left = AL_INF;
    const int32_t *crow = cq + (int64_t)(r < R ? r : 0) * M;
    int32_t cnext = r == 0 ? crow[0] : 0;  // (the cost of this thread's cell on the next diagonal, requested a diagonal ahead)
    for (int d = 0; d < nd; ++d) {
        const int j = d - r;
        const bool on = r < R && j >= 0 && j < M;
        const int32_t cost = cnext;
        const int jn = j + 1;
        if (r < R && jn >= 0 && jn < M) cnext = crow[jn];
        if (on) {
            long long c0, c1;
            const long long c2 = left;
            if (r == 0) {
                c0 = j == 0 ? 0 : AL_INF;
                c1 = AL_INF;
            } else {
                c1 = s_d[(d + 2) % 3][r - 1];
                c0 = j == 0 ? AL_INF : s_d[(d + 1) % 3][r - 1];
            }
            const int t = (c0 <= c1 && c0 <= c2) ? 0 : (c1 <= c2 ? 1 : 2);
            const long long v = (long long)cost + (t == 0 ? c0 : t == 1 ? c1 : c2);
            s_d[d % 3][r] = v;
            left = v;
            trace[(int64_t)d * R + r] = (uint8_t)t;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (r != 0) return;
    int i = R - 1, j = M - 1;
    for (int k = 0; k < AL_ROWS_MAX + AL_COLS_MAX && i >= 0 && j >= 0; ++k) {
        first[i] = j;  // (the walk moves left inside a row: the last store is the smallest column)
        const int t = trace[(int64_t)(i + j) * R + i];
        if (t != 2) --i;
        if (t != 1) --j;
    }
}

hipError_t launch_align_capture(hipStream_t s, const AlCapArgs &a) {
    if (!a.S || !a.st || !a.np || !a.s || a.n < 1 || a.n > AL_HEADS_MAX || a.T < 1 || a.T > a.s_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_capture, dim3(a.n), dim3(AL_WG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_align_cost(hipStream_t s, const AlMatArgs &a) {
    if (!a.s || !a.w || !a.cq || a.A < 1 || a.A > AL_HEADS_MAX || a.p < 1 || a.n < 1 || a.Np != a.p + a.n || a.M < 1 || a.M > a.T ||
        a.T > AL_COLS_MAX || a.n + 1 > AL_ROWS_MAX || a.width < 1 || a.width > AL_WIDTH_MAX || !(a.width & 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_softmax, dim3(a.A * a.Np), dim3(AL_WG), 0, s, a);
    hipLaunchKernelGGL(k_align_zscore, dim3((a.M + 63) / 64, a.A), dim3(AL_WG), 0, s, a);
    const dim3 grid(((a.n + 1) * a.M + AL_WG - 1) / AL_WG);
    switch (a.M > a.width / 2 ? a.width : 1) {
        case 1: hipLaunchKernelGGL(k_align_cost<1>, grid, dim3(AL_WG), 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_align_cost<3>, grid, dim3(AL_WG), 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_align_cost<5>, grid, dim3(AL_WG), 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_align_cost<7>, grid, dim3(AL_WG), 0, s, a); break;
        case 9: hipLaunchKernelGGL(k_align_cost<9>, grid, dim3(AL_WG), 0, s, a); break;
        case 11: hipLaunchKernelGGL(k_align_cost<11>, grid, dim3(AL_WG), 0, s, a); break;
        case 13: hipLaunchKernelGGL(k_align_cost<13>, grid, dim3(AL_WG), 0, s, a); break;
        case 15: hipLaunchKernelGGL(k_align_cost<15>, grid, dim3(AL_WG), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_dtw(hipStream_t s, const int32_t *cq, int R, int M, uint8_t *trace, int32_t *first) {
    if (!cq || !trace || !first || R < 1 || R > AL_ROWS_MAX || M < 1 || M > AL_COLS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dtw, dim3(1), dim3((R + 63) / 64 * 64), 0, s, cq, R, M, trace, first);
    return hipGetLastError();
}

}  // namespace wmi
