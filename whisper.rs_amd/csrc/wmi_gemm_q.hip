// wmi_gemm_q.hip — the quantised-weight GEMM of the prompt prefill and the
// wide beam step (wmi_set_quant_gemm; DESIGN.md "Quantised-weight GEMM"):
//   C[M][N] = A[M][K] . dequant(Wq[N][K])^T
// for the five ggml block formats (q4_0, q4_1, q5_0, q5_1, q8_0), f16
// activations, f32 accumulation on v_mfma_f32_32x32x16_f16.
//
// A weight is dequantised in registers to exactly the f16 value the host
// loader stores (dequant_f16, wmi_host.cpp): w = f16(fma(q - off, d, m)),
// rounded once (up to the sign of a zero weight, see dq_half8).  The blocks come repacked into aligned planes (repack_blocks,
// wmi_host.cpp): a block's quants in natural k order (16 bytes of nibbles, or
// 32 bytes for q8_0), and a side record per block: {d | m << 16}, for q5_x
// {fifth bits, d | m << 16}.
//
// Shape of the work: a product of at most 64 activation rows against a long
// weight stream.  A workgroup of four waves owns QG_NS = 32 weight rows (output
// columns) against one tile of QG_MT = 64 activation rows (blockIdx.y).  The
// weights are the MFMA's A operand: lane l holds weight row l & 31 and the 8
// k values of its half-wave, which lie inside one 32-weight block, so the
// lane's dword of nibbles, the block's fifth bits and its scale word give the
// operand without any exchange: a weight is fetched by exactly one lane and
// never passes through LDS.  The MFMA sums its 16 k in any order as long as
// both operands agree, so step s of a block takes k = 16 lh + 8 s .. + 7 from
// half-wave lh: the lane's quants of a block are one 8-byte load (16 for
// q8_0), its activations 32 contiguous bytes of the row.
//
// The four waves split K: wave w takes block w of every 128-k chunk (K is a
// multiple of 128, check_shape).  A wave's activation operand is therefore its
// own: no other wave of the workgroup reads the same k, so the fragments come
// straight from L2 (64 rows x K f16 stay resident there) as 16-byte loads,
// and a trip through LDS would only add a round trip.  Loads run QG_PD blocks
// ahead of the MFMAs in a register ring with counted vmcnt waits.  The waves'
// f32 partial tiles meet in LDS and are added in wave order, ((p0 + p1) + p2)
// + p3, each partial a fixed chain of MFMAs over the wave's blocks in
// ascending k: the sum order of an output depends on K alone, not on M, the
// grid, or which rows are idle.  The merge also turns the tile: a lane holds
// 16 output columns of one row, the epilogue (wmi_gemm_epi.h) takes four rows
// of one column and stores 128 contiguous bytes a row.
//
// Ragged edges: rows past M and weight rows past N are loaded from the last
// valid row (in bounds) and dropped by the epilogue; an activation column of
// the MFMA only reaches its own output row.  A product of at most 32 rows takes
// instances without the second row half's loads and MFMAs.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_gemm_epi.h"
#include "wmi_gemm_q.h"
#include "wmi_internal.h"

#pragma clang fp contract(off)

namespace wmi {

constexpr int QG_NS = 32;   // weight rows (output columns) of a workgroup
constexpr int QG_MT = 64;   // activation rows of a tile
constexpr int QG_PD = 4;    // blocks a wave's loads run ahead
constexpr int QG_LD = 36;   // floats a row of a partial tile in LDS: float4 writes of 32 rows 36 dwords apart cover
                            // every bank once per 16 lanes; the merge reads 32 consecutive floats

template <int QT> struct QFmt;  // QB: bytes of a block's quants; SIDE: words of its side record; OFF: the quants' offset
template <> struct QFmt<2> { static constexpr int QB = 16, SIDE = 1, OFF = 8; };
template <> struct QFmt<3> { static constexpr int QB = 16, SIDE = 1, OFF = 0; };
template <> struct QFmt<6> { static constexpr int QB = 16, SIDE = 2, OFF = 16; };
template <> struct QFmt<7> { static constexpr int QB = 16, SIDE = 2, OFF = 0; };
template <> struct QFmt<8> { static constexpr int QB = 32, SIDE = 1, OFF = 128; };

// Eight weights k .. k + 7 of a block: q0 their nibbles in natural order (q8_0: q0, q1 their bytes), hb their fifth
// bits in bits 0 .. 7 (q5_x), dm the block's {d, m}.  Two quants a dword become f16 (1024 + q) by v_perm and an or,
// minus 1024 + off (exact), then one v_pk_fma_f16 a pair: fma(q - off, d, m) rounded once; a format without m takes
// the product alone, v_pk_mul_f16, which is the oracle's value bit for bit (or_dequant: a zero quant under a negative
// d is -0 there; the host copy adds m = +0 and holds +0, the one difference, and none to any product).  q5_half8
// (wmi_device.h) is the q5_1 form.
template <int QT>
__device__ __forceinline__ half8 dq_half8(uint32_t q0, uint32_t q1, uint32_t hb, uint32_t dm) {
    using F = QFmt<QT>;
    const half2v d2 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(dm, dm, 0x01000100u));
    const half2v m2 = __builtin_bit_cast(half2v, __builtin_amdgcn_perm(dm, dm, 0x03020302u));
    const half2v kof = {(f16)(1024.0f + F::OFF), (f16)(1024.0f + F::OFF)};
    const uint32_t lo = q0 & 0x0F0F0F0Fu, hi = (q0 >> 4) & 0x0F0F0F0Fu;  // weights 0, 2, 4, 6 / 1, 3, 5, 7
    half8 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t b;
        if constexpr (QT == 8) {
            const uint32_t src = i < 2 ? q0 : q1;
            const uint32_t sel = 0x0C000C00u | ((uint32_t)(2 * (i & 1) + 1) << 16) | (uint32_t)(2 * (i & 1));
            b = __builtin_amdgcn_perm(src, src, sel) ^ 0x00800080u;  // int8 + 128
        } else {
            b = __builtin_amdgcn_perm(hi, lo, 0x0C000C00u | ((uint32_t)(4 + i) << 16) | (uint32_t)i);
            if constexpr (F::SIDE == 2) b |= ((__builtin_amdgcn_ubfe(hb, 2 * i, 2)) * 0x80010u) & 0x100010u;
        }
        const half2v q2 = __builtin_bit_cast(half2v, b | 0x64006400u) - kof;
        half2v r;
        if constexpr (QT == 3 || QT == 7) r = __builtin_elementwise_fma(q2, d2, m2);
        else r = q2 * d2;
        w[2 * i] = r[0];
        w[2 * i + 1] = r[1];
    }
    return w;
}

// what a lane holds of one block in flight
template <int QT>
struct QStage {
    uint32_t q[QFmt<QT>::QB / 8];  // its half of the block's quants
    uint32_t s[QFmt<QT>::SIDE];    // the side record
    half8 a[2][2];                 // activations [row half][step]
};

template <int QT, int EPI, bool TWO>
__global__ __launch_bounds__(256) void k_gemm_q(GemmQArgs qa) {
    using F = QFmt<QT>;
    constexpr int QW = F::QB / 8;
    __shared__ float part[4][QG_MT][QG_LD];
    const GemmArgs &g = qa.g;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l & 31, lh = l >> 5;
    const int n0 = blockIdx.x * QG_NS, m0 = blockIdx.y * QG_MT;
    constexpr bool two = TWO;            // the tiles hold a second row half (M > 32)
    const int nb = g.K >> 5;             // blocks a weight row
    const int nbw = g.K >> 7;            // ... of them this wave's: blocks w, w + 4, ..
    const int wrow = min(n0 + lr, g.N - 1);
    const int ar0 = min(m0 + lr, g.M - 1), ar1 = min(m0 + 32 + lr, g.M - 1);
    const uint8_t *qrow = qa.qn + (size_t)wrow * nb * F::QB + lh * (F::QB / 2);
    const uint32_t *srow = qa.side + (size_t)wrow * nb * F::SIDE;
    const uint16_t *a0 = g.A + (size_t)ar0 * g.lda + 16 * lh, *a1 = g.A + (size_t)ar1 * g.lda + 16 * lh;

    auto load = [&](QStage<QT> &st, int i) {
        const int kb = 4 * i + w;
        if constexpr (QW == 2) {
            const uint2 v = *(const uint2 *)(qrow + (size_t)kb * F::QB);
            st.q[0] = v.x; st.q[1] = v.y;
        } else {
            const uint4 v = *(const uint4 *)(qrow + (size_t)kb * F::QB);
            st.q[0] = v.x; st.q[1] = v.y; st.q[2] = v.z; st.q[3] = v.w;
        }
        if constexpr (F::SIDE == 2) {
            const uint2 v = *(const uint2 *)(srow + (size_t)kb * 2);
            st.s[0] = v.x; st.s[1] = v.y;
        } else {
            st.s[0] = srow[kb];
        }
        st.a[0][0] = *(const half8 *)(a0 + kb * 32);
        st.a[0][1] = *(const half8 *)(a0 + kb * 32 + 8);
        if constexpr (two) {
            st.a[1][0] = *(const half8 *)(a1 + kb * 32);
            st.a[1][1] = *(const half8 *)(a1 + kb * 32 + 8);
        }
    };
    floatx16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    auto compute = [&](const QStage<QT> &st) {
        const uint32_t dm = st.s[F::SIDE - 1];
        const uint32_t hb = F::SIDE == 2 ? st.s[0] >> (16 * lh) : 0u;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            half8 wf;
            if constexpr (QW == 2) wf = dq_half8<QT>(st.q[s], 0u, hb >> (8 * s), dm);
            else wf = dq_half8<QT>(st.q[2 * s], st.q[2 * s + 1], 0u, dm);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, st.a[0][s], acc0, 0, 0, 0);
            if constexpr (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, st.a[1][s], acc1, 0, 0, 0);
        }
    };
    // The ring: stage i holds block b0 + i.  The loop body is straight-line, so every wait is a counted vmcnt with
    // the other stages' loads still in flight; a load past the wave's last block repeats that block (in bounds,
    // never used), and the last nbw % QG_PD blocks are computed behind the loop.
    QStage<QT> st[QG_PD];
#pragma unroll
    for (int i = 0; i < QG_PD; ++i) load(st[i], min(i, nbw - 1));
    int b0 = 0;
    for (; b0 + QG_PD <= nbw; b0 += QG_PD) {
#pragma unroll
        for (int i = 0; i < QG_PD; ++i) {
            compute(st[i]);
            load(st[i], min(b0 + i + QG_PD, nbw - 1));
        }
    }
#pragma unroll
    for (int i = 0; i < QG_PD - 1; ++i)
        if (b0 + i < nbw) compute(st[i]);
    // the wave's partial: lane (row lr, half lh) holds columns (r & 3) + 8 (r >> 2) + 4 lh of its row
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        *(floatx4 *)&part[w][lr][8 * c + 4 * lh] = floatx4{acc0[4 * c], acc0[4 * c + 1], acc0[4 * c + 2], acc0[4 * c + 3]};
        if constexpr (two)
            *(floatx4 *)&part[w][32 + lr][8 * c + 4 * lh] = floatx4{acc1[4 * c], acc1[4 * c + 1], acc1[4 * c + 2], acc1[4 * c + 3]};
    }
    __syncthreads();
    // thread (column t & 31, row group t >> 5): four rows of its column, the waves' partials in wave order
    const int col = t & 31, rg = t >> 5;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !two) break;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 32 * h + 4 * rg + r;
            v[r] = ((part[0][m][col] + part[1][m][col]) + part[2][m][col]) + part[3][m][col];
        }
        gemm_epi4<EPI>(g, m0 + 32 * h + 4 * rg, n0 + col, v);
    }
}

template <int QT, bool TWO>
static hipError_t gemm_q_epi(hipStream_t s, int epi, const GemmQArgs &a) {
    const dim3 grid((unsigned)((a.g.N + QG_NS - 1) / QG_NS), (unsigned)((a.g.M + QG_MT - 1) / QG_MT));
    switch (epi) {
        case EPI_F32: hipLaunchKernelGGL((k_gemm_q<QT, EPI_F32, TWO>), grid, dim3(256), 0, s, a); break;
        case EPI_RESID: hipLaunchKernelGGL((k_gemm_q<QT, EPI_RESID, TWO>), grid, dim3(256), 0, s, a); break;
        case EPI_GELU16: hipLaunchKernelGGL((k_gemm_q<QT, EPI_GELU16, TWO>), grid, dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;  // (the encoder's epilogues have no quantised form)
    }
    return hipGetLastError();
}
// at most 32 rows: the instances without the second row half's loads and MFMAs
template <int QT>
static hipError_t gemm_q_rows(hipStream_t s, int epi, const GemmQArgs &a) {
    return a.g.M > 32 ? gemm_q_epi<QT, true>(s, epi, a) : gemm_q_epi<QT, false>(s, epi, a);
}

hipError_t launch_gemm_q(hipStream_t s, int epi, const GemmQArgs &a) {
    const GemmArgs &g = a.g;
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    if (g.K <= 0 || g.K % 128 != 0 || g.lda % 8 != 0 || !a.qn || !a.side || !g.A) return hipErrorInvalidValue;
    switch (a.qtype) {
        case 2: return gemm_q_rows<2>(s, epi, a);
        case 3: return gemm_q_rows<3>(s, epi, a);
        case 6: return gemm_q_rows<6>(s, epi, a);
        case 7: return gemm_q_rows<7>(s, epi, a);
        case 8: return gemm_q_rows<8>(s, epi, a);
        default: return hipErrorInvalidValue;
    }
}

// wmi_dequant_blocks: thread i expands weights 8 (i & 3) .. + 7 of block i >> 2 with the GEMM's dq_half8
template <int QT>
__global__ __launch_bounds__(256) void k_dequant_q(const uint8_t *qn, const uint32_t *side, long long nblocks, uint16_t *out) {
    using F = QFmt<QT>;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * nblocks) return;
    const long long b = i >> 2;
    const int p = (int)(i & 3);
    const uint32_t *q = (const uint32_t *)(qn + b * F::QB);
    const uint32_t dm = side[b * F::SIDE + F::SIDE - 1];
    const uint32_t hb = F::SIDE == 2 ? side[b * F::SIDE] >> (8 * p) : 0u;
    const half8 w = F::QB == 32 ? dq_half8<QT>(q[2 * p], q[2 * p + 1], 0u, dm) : dq_half8<QT>(q[p], 0u, hb, dm);
    *(half8 *)(out + 8 * i) = w;
}

hipError_t launch_dequant_q(hipStream_t s, int qtype, const uint8_t *qn, const uint32_t *side, long long nblocks, uint16_t *out) {
    if (nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)((4 * nblocks + 255) / 256));
    switch (qtype) {
        case 2: hipLaunchKernelGGL(k_dequant_q<2>, grid, dim3(256), 0, s, qn, side, nblocks, out); break;
        case 3: hipLaunchKernelGGL(k_dequant_q<3>, grid, dim3(256), 0, s, qn, side, nblocks, out); break;
        case 6: hipLaunchKernelGGL(k_dequant_q<6>, grid, dim3(256), 0, s, qn, side, nblocks, out); break;
        case 7: hipLaunchKernelGGL(k_dequant_q<7>, grid, dim3(256), 0, s, qn, side, nblocks, out); break;
        case 8: hipLaunchKernelGGL(k_dequant_q<8>, grid, dim3(256), 0, s, qn, side, nblocks, out); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace wmi
