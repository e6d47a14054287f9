// wmi_gemm_qk.h — launch interface of the K-quant GEMM (wmi_gemm_qk.hip;
// DESIGN.md "K-quant GEMM"), beside wmi_gemm_q.h's: the launchers enqueue on
// the given stream and neither allocate, copy nor synchronise.
#pragma once
#include "wmi_internal.h"

namespace wmi {

// C[M][N] = A[M][K] . dequant(Wq[N][K])^T with the epilogues EPI_F32, EPI_RESID and EPI_GELU16 of launch_gemm, for
// the 256-weight super-blocks q4_K, q5_K and q6_K.  g carries what launch_gemm reads for a plain product; g.B is not
// read.  The weights are the planes of repack_kblocks (wmi_host.h), [N][K / 256] super-blocks each: qn 128 bytes of
// nibbles, hi 0 / 8 / 16 words of high bits, side 5 words of scales.  K a multiple of 256, lda of 8.
struct GemmQKArgs {
    GemmArgs g;
    int qtype;               // ggml type of the super-blocks: 12 q4_K, 13 q5_K, 14 q6_K
    const uint8_t *qn;
    const uint32_t *hi;      // (q4_K: not read)
    const uint32_t *side;
};
hipError_t launch_gemm_qk(hipStream_t s, int epi, const GemmQKArgs &a);
// out[256 nsb] = the f16 bits of the planes' weights, by the GEMM's own device function
hipError_t launch_dequant_qk(hipStream_t s, int qtype, const uint8_t *qn, const uint32_t *hi, const uint32_t *side,
                             long long nsb, uint16_t *out);

}  // namespace wmi
