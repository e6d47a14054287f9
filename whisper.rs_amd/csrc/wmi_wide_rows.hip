// wmi_wide_rows.hip — the wide step's cross-attention for one hypothesis a
// recording (wmi_set_wide_rounds; DESIGN.md "Wide rounds").
//
// k_wd_cross_attn1: at K = 1 a round's rows are up to 64 different recordings,
// and row c reads the T x 64 encoder keys and values of its own recording's
// head exactly once.  k_wd_cross_attn would stage each of them through LDS to
// fill one of 16 MFMA columns; here they go from global memory straight to
// registers and the products are fdot2 / f32 FMAs:
//
//   workgroup (key chunk, head, recording), four waves; wave w takes the
//   chunk's 32-key blocks w, w + 4, ...; a block is 8 loads of 16 bytes a lane,
//   all issued before the block in front of it is computed (two blocks' loads
//   in flight a wave):
//   scores   four lanes share a key row (16 halfs = two 16-byte loads a lane,
//            dot8 against the lane's 16 query halfs, summed over the four
//            lanes): 16 keys a pass, two passes a block;
//   softmax  the rounding points of k_wd_cross_attn: f32 scores, a running
//            maximum per wave, P = exp_f16_exact(s - m) (an f16 value), the
//            sum in double, alpha = expf(m_old - m_new);
//   P V      eight lanes share a value row (8 halfs = one 16-byte load a
//            lane), a lane's four rows of the block are kg + {0, 8, 16, 24};
//            their P come from the score lanes by a lane permute, so P never
//            passes through memory;
//   merge    the waves' (m, l, o[64]) meet in LDS (4 x 66 floats, the only LDS
//            of the kernel) and the chunk's partial goes out in f32 in the
//            layout k_wd_cross_combine reads (row 0 of the 16 a chunk holds).
//
// Keys past the chunk's end load nothing and score -inf; T needs no alignment.
// A translation unit of its own, loaded with the first round that uses it.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

#pragma clang fp contract(off)

namespace wmi {

namespace {

constexpr int W1_BLK = 32;     // keys a wave's block
constexpr int W1_WAVES = 4;
constexpr int W1_CK = 64;      // keys a tile of wd_cross_split

struct W1Block {
    half8 k[2][2];  // score pass sb: the lane's 16 halfs of key row 16 sb + (lane >> 2)
    half8 v[4];     // the lane's 8 halfs of value rows (lane >> 3) + 8 j
};

__device__ __forceinline__ half8 w1_zero() {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    return __builtin_bit_cast(half8, z);
}

// the lane's pieces of keys [base, base + 32) below `end` (rows at or past it: zeros, no load)
__device__ __forceinline__ void w1_load(W1Block &b, const f16 *Kc, const f16 *Vc, int n, int base, int end, int lane) {
    const int sub = lane & 3, kq = lane >> 2, part = lane & 7, kg = lane >> 3;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int key = base + 16 * sb + kq;
        b.k[sb][0] = b.k[sb][1] = w1_zero();
        if (key < end) {
            const f16 *kr = Kc + (int64_t)key * n + sub * 16;
            b.k[sb][0] = *(const half8 *)kr;
            b.k[sb][1] = *(const half8 *)(kr + 8);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int key = base + kg + 8 * j;
        b.v[j] = w1_zero();
        if (key < end) b.v[j] = *(const half8 *)(Vc + (int64_t)key * n + part * 8);
    }
}

}  // namespace

__global__ __launch_bounds__(64 * W1_WAVES) void k_wd_cross_attn1(WdCrossArgs a) {
    __shared__ float mrg[W1_WAVES][WD_PART];
    const int ch = blockIdx.x, h = blockIdx.y, c = blockIdx.z;
    if (a.rowmap[c] < 0) return;  // (uniform) an idle row; k_wd_cross_combine writes its zeros
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n, T = a.T;
    const int k0 = ch * a.tiles * W1_CK, k1 = min(T, k0 + a.tiles * W1_CK);  // (k0 < T: checked at the launch)
    int clip = a.tb.recs[c].clip;
    clip = clip < 0 ? 0 : clip;
    const f16 *Kc = (const f16 *)a.K + (int64_t)clip * T * n + h * 64, *Vc = (const f16 *)a.V + (int64_t)clip * T * n + h * 64;
    const int sub = lane & 3, kg = lane >> 3;
    const f16 *qr = (const f16 *)a.q + (int64_t)c * n + h * 64 + sub * 16;
    const half8 q0 = *(const half8 *)qr, q1 = *(const half8 *)(qr + 8);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    float m = -INFINITY;
    double l = 0.0;
    int base = k0 + w * W1_BLK;
    W1Block cur;
    w1_load(cur, Kc, Vc, n, base, k1, lane);
    for (; base < k1; base += W1_BLK * W1_WAVES) {  // (uniform over the wave: the block has a key below k1)
        W1Block nxt;
        w1_load(nxt, Kc, Vc, n, base + W1_BLK * W1_WAVES, k1, lane);
        float s[2], tm = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            float v = dot8(cur.k[sb][0], q0, 0.0f);
            v = dot8(cur.k[sb][1], q1, v);
            v = xstep<XSum, 1>(v);
            v = xstep<XSum, 2>(v);
            s[sb] = base + 16 * sb + (lane >> 2) < k1 ? v : -INFINITY;
            tm = fmaxf(tm, s[sb]);
        }
        tm = xstep<XMax, 4>(tm);
        tm = xstep<XMax, 8>(tm);
        tm = xstep<XMax, 16>(tm);
        tm = xstep<XMax, 32>(tm);  // (the block's first key is below k1: finite)
        const float mn = fmaxf(m, tm);
        const float alpha = m == -INFINITY ? 0.0f : expf(m - mn);
        float pe[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) pe[sb] = s[sb] == -INFINITY ? 0.0f : exp_f16_exact(s[sb] - mn);
        const double ps = wave_sum(sub == 0 ? (double)pe[0] + (double)pe[1] : 0.0);  // (a key's four lanes hold one P)
        l = l * (double)alpha + ps;
        m = mn;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = o[e] * alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // value row kg + 8 j is key (kg + 8 (j & 1)) of score pass j >> 1: its P sits in lanes 4 (that key) ..+3
            const float pj = __shfl(pe[j >> 1], 4 * (kg + 8 * (j & 1)), 64);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += pj * (float)cur.v[j][e];
        }
        cur = nxt;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = red_8_16_32(o[e]);  // over the wave's lanes of the same part
    if (lane < 8) {
        if (lane == 0) { mrg[w][0] = m; mrg[w][1] = (float)l; }
#pragma unroll
        for (int e = 0; e < 8; ++e) mrg[w][2 + lane * 8 + e] = o[e];
    }
    __syncthreads();
    if (tid < 64) {  // head dim tid of the chunk's partial (wave 0 has the chunk's first key: M is finite)
        float M = mrg[0][0];
#pragma unroll
        for (int i = 1; i < W1_WAVES; ++i) M = fmaxf(M, mrg[i][0]);
        float L = 0.0f, od = 0.0f;
#pragma unroll
        for (int i = 0; i < W1_WAVES; ++i) {
            const float wgt = mrg[i][0] == -INFINITY ? 0.0f : expf(mrg[i][0] - M);
            L += mrg[i][1] * wgt;
            od += mrg[i][2 + tid] * wgt;
        }
        float *dst = a.part + (((int64_t)c * a.H + h) * a.chunks + ch) * 16 * WD_PART;
        if (tid == 0) { dst[0] = M; dst[1] = L; }
        dst[2 + tid] = od;
    }
}

hipError_t launch_wd_cross_attn1(hipStream_t s, const WdCrossArgs &a) {
    if (a.B < 1 || a.B > WD_ROWS || a.Kb != 1 || a.T < 1 || a.n != a.H * 64 || a.chunks < 1 || a.tiles < 1 ||
        (int64_t)a.chunks * a.tiles * W1_CK < a.T || (int64_t)(a.chunks - 1) * a.tiles * W1_CK >= a.T)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_cross_attn1, dim3(a.chunks, a.H, a.B), dim3(64 * W1_WAVES), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wd_cross_combine(s, a);
}

}  // namespace wmi
