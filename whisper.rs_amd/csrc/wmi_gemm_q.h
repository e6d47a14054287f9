// wmi_gemm_q.h — launch interface of the quantised-weight GEMM (wmi_gemm_q.hip;
// DESIGN.md "Quantised-weight GEMM"), beside wmi_internal.h's: the launchers
// enqueue on the given stream and neither allocate, copy nor synchronise.
#pragma once
#include "wmi_internal.h"

namespace wmi {

// C[M][N] = A[M][K] . dequant(Wq[N][K])^T with the epilogues EPI_F32, EPI_RESID and EPI_GELU16 of launch_gemm.
// g carries what launch_gemm reads for a plain product (A, lda, bias, M, N, K, the outputs, the GELU table and
// threshold); g.B is not read.  The weights are the planes of repack_blocks (wmi_host.h): qn [N][K / 32] blocks of
// quants, side [N][K / 32] records.  K a multiple of 128, lda of 8.
struct GemmQArgs {
    GemmArgs g;
    int qtype;               // ggml type of the blocks: 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0
    const uint8_t *qn;
    const uint32_t *side;
};
hipError_t launch_gemm_q(hipStream_t s, int epi, const GemmQArgs &a);
// out[32 nblocks] = the f16 bits of the planes' weights, by the GEMM's own device function
hipError_t launch_dequant_q(hipStream_t s, int qtype, const uint8_t *qn, const uint32_t *side, long long nblocks, uint16_t *out);

}  // namespace wmi
