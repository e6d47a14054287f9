// wmi_align_pass.hip — the alignment scores of a forced prefill pass
// (wmi_set_dtw_pass, wmi_align_tokens_rows; DESIGN.md "Token times in one
// forced pass"): S1 of the header for every position of up to eight recordings
// at once, behind the cross-attention query projection of a layer of
// prefill_pass.
//
// k_pf_cross_attn is flash-style and never holds a score in memory; the
// alignment needs the scores of a few selected heads, all of them, in f32.
// This kernel is the product S = Q K^T of those heads alone and nothing else:
// no softmax, no V, no LDS.
//
// v_mfma_f32_32x32x16_f16 with the queries as the A operand and the keys as
// the B operand (k_pf_cross_attn has them the other way round, for its row
// maximum): accumulator register r of lane (lr, lh) is query (r & 3) + 8 (r >>
// 2) + 4 lh against key lr, so a wave's store of one register is two runs of
// 32 consecutive floats, 128 bytes each, of two score rows.
//
// A wave owns 32 keys of one (recording, selected head): its four B fragments
// (lane (lr, lh): key lr, head dims 16 ks + 8 lh .. + 7) are four 16-byte
// global loads and stay in registers for the whole kernel.  A key element is
// read by that one wave only, so there is nothing to share through LDS and no
// barrier.  The wave then walks the recording's query tiles of 32 positions
// (at most PF_MAX_KEYS / 32 = 8): four 16-byte loads a lane and tile, the next
// tile's requested before the current tile's four MFMAs and 16 stores.  The
// queries of a head are 32 KB at most and every wave of the head reads them:
// they sit in L2.
//
// A score is one chain of four MFMAs, ks ascending, from a zero accumulator;
// nothing else is applied to it (the queries carry the scaling already,
// k_pf_qkv_store).
//
// A translation unit of its own: its code object is loaded with the first
// forced pass, so a context that never calls wmi_set_dtw_pass(1) or
// wmi_align_tokens_rows runs on exactly the code objects it ran on before.
#include <hip/hip_runtime.h>

#include "wmi_align_pass.h"
#include "wmi_device.h"

namespace wmi {

namespace {

constexpr int AP_KEYS = 32;  // keys a wave, and a workgroup: one wave

// a tile's A fragments: query min(i0 + lr, len - 1), head dims 16 ks + 8 lh .. + 7
__device__ __forceinline__ void ap_load_q(half8 (&qf)[4], const f16 *qb, int n, int i0, int lr, int len) {
    const f16 *qr = qb + (int64_t)min(i0 + lr, len - 1) * n;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const half8 *)(qr + ks * 16);
}

}  // namespace

// grid: (32-key blocks of T, the layer's selected heads, recordings), one wave each
__global__ __launch_bounds__(64) void k_align_scores(AlPassArgs a) {
    const PfRec rec = a.recs.r[blockIdx.z];
    if (rec.len < 1) return;
    const int g = blockIdx.y, h = a.head[g];
    const int lane = threadIdx.x, lr = lane & 31, lh = lane >> 5;
    const int n = a.n, T = a.T, j0 = blockIdx.x * AP_KEYS, j = j0 + lr;
    // (a key at or past T reads the last valid key and is not stored)
    half8 kf[4];
    {
        const f16 *kr = (const f16 *)a.K + ((int64_t)rec.clip * T + min(j, T - 1)) * n + h * 64 + lh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const half8 *)(kr + ks * 16);
    }
    const f16 *qb = (const f16 *)a.q + (int64_t)rec.row0 * n + h * 64 + lh * 8;
    float *out = a.s + a.off[blockIdx.z] + (int64_t)a.slot[g] * rec.len * T + j;
    const int ntile = (rec.len + 31) / 32;
    half8 qf[4], qn[4];
    ap_load_q(qf, qb, n, 0, lr, rec.len);
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) ap_load_q(qn, qb, n, (t + 1) * 32, lr, rec.len);
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qf[ks], kf[ks], acc, 0, 0, 0);
        if (j < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (i < rec.len) out[(int64_t)i * T] = acc[r];
            }
        }
        if (t + 1 < ntile) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
        }
    }
}

hipError_t launch_align_scores(hipStream_t s, const AlPassArgs &a) {
    if (!a.q || !a.K || !a.s || a.nh < 1 || a.nh > AL_HEADS_MAX || a.recs.n < 1 || a.recs.n > DEC_ROWS || a.T < 1 ||
        a.T > AL_COLS_MAX || a.H < 1 || a.n != a.H * 64 || a.recs.max_len < 1 || a.recs.max_len > PF_MAX_KEYS)
        return hipErrorInvalidValue;
    for (int g = 0; g < a.nh; ++g)
        if (a.head[g] < 0 || a.head[g] >= a.H || a.slot[g] < 0 || a.slot[g] >= a.A) return hipErrorInvalidValue;
    for (int r = 0; r < a.recs.n; ++r)
        if (a.recs.r[r].len > a.recs.max_len || a.recs.r[r].row0 < 0 || a.recs.r[r].clip < 0 || a.off[r] < 0)
            return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_scores, dim3((a.T + AP_KEYS - 1) / AP_KEYS, a.nh, a.recs.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
