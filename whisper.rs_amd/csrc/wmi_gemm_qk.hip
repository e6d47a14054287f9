// wmi_gemm_qk.hip — the K-quant GEMM of the prompt prefill and the wide step
// (wmi_set_quant_gemm on a q4_K / q5_K / q6_K file; DESIGN.md "K-quant GEMM"):
//   C[M][N] = A[M][K] . dequant(Wq[N][K])^T
// for ggml's 256-weight super-blocks, f16 activations, f32 accumulation on
// v_mfma_f32_32x32x16_f16.
//
// A weight is w = f16(fmaf(q, a, b)) with the effective scale a = d * sc and
// offset b = -(dmin * m) of its sub-block, both exact in f32 (q6_K: a = d * S,
// b = -32 a, so the fma is the f32 product a (q - 32) rounded once): the value
// the host loader stores (dequant_k_f16, wmi_host.cpp), rounded to f32 and then
// to f16.  a and b are products no f16 holds, so unlike k_gemm_q's packed f16
// arithmetic the expansion runs in f32: v_cvt_f32_ubyte, v_fma_f32, v_cvt_f16_f32.
//
// Planes (repack_kblocks, wmi_host.cpp), per super-block of a weight row:
//   qn    128 bytes: the file's nibble bytes (q4_K / q5_K qs, q6_K ql) as they
//         are: 16-byte slot 2 w + lh belongs to wave w, half-wave lh
//   hi    a slot's high bits, transposed on the host so that a shift and a mask
//         put them over the nibbles of a dword: q5_K one word, bit 8 p + dw +
//         4 n of byte p of dword dw, nibble n; q6_K two words (one a nibble),
//         bits 8 p + 2 dw, + 1
//   side  5 words: {d | dmin << 16}, then one word a wave with the 6-bit (q6_K:
//         8-bit) fields of its two sub-blocks unpacked to bytes:
//         {sc, m, sc', m'}, for q6_K {S[lh = 0], S[1], S'[0], S'[1]}
//
// Shape of the work.  A workgroup of four waves owns 32 NF weight rows against
// one tile of 64 activation rows (blockIdx.y).  The weights are the MFMA's A
// operand: lane l holds weight row l & 31, and of every super-block the 32
// weights of slot (w, lh): the low nibbles of its 16 bytes are k = kb .. kb + 15,
// the high nibbles k = kb + HI .. + 15, with kb = 64 w + 16 lh and HI = 32 for
// q4_K / q5_K (sub-blocks 2 w and 2 w + 1) and kb = 128 (w >> 1) + 32 (w & 1) +
// 16 lh, HI = 64 for q6_K (weights l and l + 64 of a half).  The MFMA sums its 16
// k in any order as long as both operands agree, so the four steps of a
// super-block take k = kb, kb + 8, kb + HI, kb + HI + 8 (.. + 7 each) and the
// activation fragments are loaded by the same map.  A weight is fetched by
// exactly one lane, as one 16-byte load a super-block, and never passes through
// LDS; the two effective scales a lane needs are made once a super-block.
//
// The four waves split K by slot, so no two waves read the same activations and
// the fragments come straight from L2.  NF = 2 (64 weight rows) uses each
// activation fragment for two weight fragments, which halves the activation
// bytes a weight; it is taken where the strips still fill the device (the
// vocabulary product), see launch_gemm_qk.  Loads run QK_PD super-blocks ahead
// in a register ring with counted vmcnt waits.  The waves' f32 partial tiles
// meet in LDS and are added in wave order, ((p0 + p1) + p2) + p3, each partial a
// fixed chain of MFMAs over the super-blocks in ascending order, steps 0 .. 3:
// the sum order of an output depends on K alone, not on M, N, NF, the grid or
// which rows are idle.
//
// Ragged edges: rows past M and weight rows past N are loaded from the last
// valid row (in bounds) and dropped by the epilogue.  A product of at most 32
// rows takes instances without the second row half's loads and MFMAs.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_gemm_epi.h"
#include "wmi_gemm_qk.h"
#include "wmi_internal.h"

#pragma clang fp contract(off)

namespace wmi {

constexpr int QK_MT = 64;        // activation rows of a tile
constexpr int QK_PD = 2;         // super-blocks a wave's loads run ahead (64 k each: k_gemm_q's four blocks)
constexpr int QK_LD = 36;        // floats a row of a partial tile in LDS (k_gemm_q's QG_LD)
constexpr int QK_WIDE_N = 16384; // from this N on a workgroup takes 64 weight rows: 256 strips and more

template <int QT> struct KFmt;  // HW: words of high bits a slot; HI: k distance of a byte's two nibbles
template <> struct KFmt<12> { static constexpr int HW = 0, HI = 32; };
template <> struct KFmt<13> { static constexpr int HW = 1, HI = 32; };
template <> struct KFmt<14> { static constexpr int HW = 2, HI = 64; };

template <int QT>
__device__ __forceinline__ int k_base(int w, int lh) {
    return QT == 14 ? 128 * (w >> 1) + 32 * (w & 1) + 16 * lh : 64 * w + 16 * lh;
}

// the effective scale and offset of a slot's low-nibble (0) and high-nibble (1) weights, exact in f32
struct KScale { float a[2], b[2]; };
template <int QT>
__device__ __forceinline__ KScale k_scales(uint32_t dd, uint32_t sw, int lh) {
    KScale s;
    const float d = h2f_bits((uint16_t)(dd & 0xffffu));
    if constexpr (QT == 14) {
        const uint32_t x = sw >> (8 * lh);
        s.a[0] = d * (float)(int)(int8_t)(x & 0xffu);
        s.a[1] = d * (float)(int)(int8_t)((x >> 16) & 0xffu);
        s.b[0] = -32.0f * s.a[0];
        s.b[1] = -32.0f * s.a[1];
    } else {
        const float dmin = h2f_bits((uint16_t)(dd >> 16));
        s.a[0] = d * (float)(sw & 0xffu);
        s.b[0] = -(dmin * (float)((sw >> 8) & 0xffu));
        s.a[1] = d * (float)((sw >> 16) & 0xffu);
        s.b[1] = -(dmin * (float)(sw >> 24));
    }
    return s;
}

// Eight weights: nibble NIB of dwords DW and DW + 1 of a slot (x0, x1), hw its word of high bits.  The high bits go
// over the nibbles by a shift, a mask and an or; a byte becomes f32 by v_cvt_f32_ubyte, then one fma and the rounding
// to f16 (f16_rt keeps the two roundings apart: the backend would fold them into one v_fma_mixlo_f16).
template <int QT, int DW, int NIB>
__device__ __forceinline__ half8 dqk_half8(uint32_t x0, uint32_t x1, uint32_t hw, float a, float b) {
    half8 w;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        uint32_t n = ((c ? x1 : x0) >> (4 * NIB)) & 0x0F0F0F0Fu;
        if constexpr (QT == 13) n |= ((hw >> (DW + c + 4 * NIB)) & 0x01010101u) << 4;
        if constexpr (QT == 14) n |= ((hw >> (2 * (DW + c))) & 0x03030303u) << 4;
#pragma unroll
        for (int p = 0; p < 4; ++p) w[4 * c + p] = f16_rt(__builtin_fmaf((float)((n >> (8 * p)) & 0xffu), a, b));
    }
    return w;
}

// step S of a slot: k = kb + 8 (S & 1) + HI (S >> 1) .. + 7
template <int QT, int S>
__device__ __forceinline__ half8 dqk_step(const uint32_t *q, const uint32_t *h, const KScale &sc) {
    constexpr int DW = 2 * (S & 1), NIB = S >> 1;
    const uint32_t hw = KFmt<QT>::HW == 2 ? h[NIB] : KFmt<QT>::HW == 1 ? h[0] : 0u;
    return dqk_half8<QT, DW, NIB>(q[DW], q[DW + 1], hw, sc.a[NIB], sc.b[NIB]);
}

// what a lane holds of one super-block in flight
template <int QT, int NF>
struct KStage {
    uint32_t q[NF][4];                                   // its slot's nibbles
    uint32_t h[NF][KFmt<QT>::HW ? KFmt<QT>::HW : 1];     // ... high bits
    uint32_t dd[NF], sw[NF];                             // {d | dmin << 16}, the wave's scale word
    half8 a[2][4];                                       // activations [row half][step]
};

template <int QT, int EPI, bool TWO, int NF>
__global__ __launch_bounds__(256) void k_gemm_qk(GemmQKArgs qa) {
    using F = KFmt<QT>;
    __shared__ float part[4][QK_MT][QK_LD];
    const GemmArgs &g = qa.g;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l & 31, lh = l >> 5;
    const int n0 = blockIdx.x * (32 * NF), m0 = blockIdx.y * QK_MT;
    constexpr bool two = TWO;            // the tiles hold a second row half (M > 32)
    const int nsb = g.K >> 8;            // super-blocks a weight row: each wave takes its slots of every one
    const int ar0 = min(m0 + lr, g.M - 1), ar1 = min(m0 + 32 + lr, g.M - 1);
    const int kb = k_base<QT>(w, lh);
    const uint16_t *a0 = g.A + (size_t)ar0 * g.lda + kb, *a1 = g.A + (size_t)ar1 * g.lda + kb;
    size_t sb0[NF];                      // the rows' first super-block
#pragma unroll
    for (int f = 0; f < NF; ++f) sb0[f] = (size_t)min(n0 + 32 * f + lr, g.N - 1) * nsb;

    auto load = [&](KStage<QT, NF> &st, int i) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const size_t sb = sb0[f] + i, slot = sb * 8 + 2 * w + lh;
            const uint4 v = *(const uint4 *)(qa.qn + slot * 16);
            st.q[f][0] = v.x; st.q[f][1] = v.y; st.q[f][2] = v.z; st.q[f][3] = v.w;
            if constexpr (F::HW == 1) st.h[f][0] = qa.hi[slot];
            if constexpr (F::HW == 2) {
                const uint2 hv = *(const uint2 *)(qa.hi + slot * 2);
                st.h[f][0] = hv.x; st.h[f][1] = hv.y;
            }
            st.dd[f] = qa.side[sb * 5];
            st.sw[f] = qa.side[sb * 5 + 1 + w];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 256 * i + 8 * (s & 1) + F::HI * (s >> 1);
            st.a[0][s] = *(const half8 *)(a0 + k);
            if constexpr (two) st.a[1][s] = *(const half8 *)(a1 + k);
        }
    };
    floatx16 acc[NF][2];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[f][0][r] = 0.0f; acc[f][1][r] = 0.0f; }
    auto step = [&](const KStage<QT, NF> &st, int f, int s, half8 wf) {
        acc[f][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, st.a[0][s], acc[f][0], 0, 0, 0);
        if constexpr (two) acc[f][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, st.a[1][s], acc[f][1], 0, 0, 0);
    };
    auto compute = [&](const KStage<QT, NF> &st) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const KScale sc = k_scales<QT>(st.dd[f], st.sw[f], lh);
            step(st, f, 0, dqk_step<QT, 0>(st.q[f], st.h[f], sc));
            step(st, f, 1, dqk_step<QT, 1>(st.q[f], st.h[f], sc));
            step(st, f, 2, dqk_step<QT, 2>(st.q[f], st.h[f], sc));
            step(st, f, 3, dqk_step<QT, 3>(st.q[f], st.h[f], sc));
        }
    };
    // The ring of k_gemm_q: stage i holds super-block b0 + i; the loop body is straight-line, a load past the last
    // super-block repeats it (in bounds, never used), and the last nsb % QK_PD are computed behind the loop.
    KStage<QT, NF> st[QK_PD];
#pragma unroll
    for (int i = 0; i < QK_PD; ++i) load(st[i], min(i, nsb - 1));
    int b0 = 0;
    for (; b0 + QK_PD <= nsb; b0 += QK_PD) {
#pragma unroll
        for (int i = 0; i < QK_PD; ++i) {
            compute(st[i]);
            load(st[i], min(b0 + i + QK_PD, nsb - 1));
        }
    }
#pragma unroll
    for (int i = 0; i < QK_PD - 1; ++i)
        if (b0 + i < nsb) compute(st[i]);
    // a weight fragment at a time through the 36 KB of k_gemm_q's merge: lane (row lr, half lh) holds columns
    // (r & 3) + 8 (r >> 2) + 4 lh of its row; then thread (column t & 31, row group t >> 5) adds four rows of its
    // column in wave order
    const int col = t & 31, rg = t >> 5;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (f) __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            *(floatx4 *)&part[w][lr][8 * c + 4 * lh] =
                floatx4{acc[f][0][4 * c], acc[f][0][4 * c + 1], acc[f][0][4 * c + 2], acc[f][0][4 * c + 3]};
            if constexpr (two)
                *(floatx4 *)&part[w][32 + lr][8 * c + 4 * lh] =
                    floatx4{acc[f][1][4 * c], acc[f][1][4 * c + 1], acc[f][1][4 * c + 2], acc[f][1][4 * c + 3]};
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) break;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 32 * h + 4 * rg + r;
                v[r] = ((part[0][m][col] + part[1][m][col]) + part[2][m][col]) + part[3][m][col];
            }
            gemm_epi4<EPI>(g, m0 + 32 * h + 4 * rg, n0 + 32 * f + col, v);
        }
    }
}

template <int QT, bool TWO, int NF>
static hipError_t gemm_qk_epi(hipStream_t s, int epi, const GemmQKArgs &a) {
    const dim3 grid((unsigned)((a.g.N + 32 * NF - 1) / (32 * NF)), (unsigned)((a.g.M + QK_MT - 1) / QK_MT));
    switch (epi) {
        case EPI_F32: hipLaunchKernelGGL((k_gemm_qk<QT, EPI_F32, TWO, NF>), grid, dim3(256), 0, s, a); break;
        case EPI_RESID: hipLaunchKernelGGL((k_gemm_qk<QT, EPI_RESID, TWO, NF>), grid, dim3(256), 0, s, a); break;
        case EPI_GELU16: hipLaunchKernelGGL((k_gemm_qk<QT, EPI_GELU16, TWO, NF>), grid, dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;  // (the encoder's epilogues have no quantised form)
    }
    return hipGetLastError();
}
// The strip height follows N alone: 64 weight rows where that still leaves a strip for each of the device's 256
// compute units (Whisper's vocabulary product), else 32, which keeps twice the workgroups on the n x n and MLP
// products.  At most 32 activation rows: the instances without the second row half.
template <int QT>
static hipError_t gemm_qk_rows(hipStream_t s, int epi, const GemmQKArgs &a) {
    if (a.g.N >= QK_WIDE_N) return a.g.M > 32 ? gemm_qk_epi<QT, true, 2>(s, epi, a) : gemm_qk_epi<QT, false, 2>(s, epi, a);
    return a.g.M > 32 ? gemm_qk_epi<QT, true, 1>(s, epi, a) : gemm_qk_epi<QT, false, 1>(s, epi, a);
}

hipError_t launch_gemm_qk(hipStream_t s, int epi, const GemmQKArgs &a) {
    const GemmArgs &g = a.g;
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    if (g.K <= 0 || g.K % 256 != 0 || g.lda % 8 != 0 || !a.qn || !a.side || !g.A) return hipErrorInvalidValue;
    if (a.qtype != 12 && !a.hi) return hipErrorInvalidValue;
    switch (a.qtype) {
        case 12: return gemm_qk_rows<12>(s, epi, a);
        case 13: return gemm_qk_rows<13>(s, epi, a);
        case 14: return gemm_qk_rows<14>(s, epi, a);
        default: return hipErrorInvalidValue;
    }
}

// wmi_dequant_blocks: thread i expands slot i & 7 of super-block i >> 3 with the GEMM's own steps
template <int QT>
__global__ __launch_bounds__(256) void k_dequant_qk(const uint8_t *qn, const uint32_t *hi, const uint32_t *side, long long nsb,
                                                    uint16_t *out) {
    using F = KFmt<QT>;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 8 * nsb) return;
    const long long sb = i >> 3;
    const int w = (int)(i >> 1) & 3, lh = (int)i & 1;
    const uint4 v = *(const uint4 *)(qn + i * 16);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t h[2] = {0u, 0u};
    if constexpr (F::HW == 1) h[0] = hi[i];
    if constexpr (F::HW == 2) { h[0] = hi[2 * i]; h[1] = hi[2 * i + 1]; }
    const KScale sc = k_scales<QT>(side[sb * 5], side[sb * 5 + 1 + w], lh);
    uint16_t *o = out + sb * 256 + k_base<QT>(w, lh);
    *(half8 *)o = dqk_step<QT, 0>(q, h, sc);
    *(half8 *)(o + 8) = dqk_step<QT, 1>(q, h, sc);
    *(half8 *)(o + F::HI) = dqk_step<QT, 2>(q, h, sc);
    *(half8 *)(o + F::HI + 8) = dqk_step<QT, 3>(q, h, sc);
}

hipError_t launch_dequant_qk(hipStream_t s, int qtype, const uint8_t *qn, const uint32_t *hi, const uint32_t *side,
                             long long nsb, uint16_t *out) {
    if (nsb <= 0) return hipSuccess;
    const dim3 grid((unsigned)((8 * nsb + 255) / 256));
    switch (qtype) {
        case 12: hipLaunchKernelGGL(k_dequant_qk<12>, grid, dim3(256), 0, s, qn, hi, side, nsb, out); break;
        case 13: hipLaunchKernelGGL(k_dequant_qk<13>, grid, dim3(256), 0, s, qn, hi, side, nsb, out); break;
        case 14: hipLaunchKernelGGL(k_dequant_qk<14>, grid, dim3(256), 0, s, qn, hi, side, nsb, out); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace wmi
