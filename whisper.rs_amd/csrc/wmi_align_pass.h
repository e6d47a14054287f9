// The alignment scores of a forced prefill pass (wmi_align_pass.hip; DESIGN.md
// "Token times in one forced pass").  A header of its own: only the new unit
// and wmi_api.cpp include it.
#pragma once

#include "wmi_internal.h"

namespace wmi {

// S1 behind launch_pf_qkv_store of a layer's cross-attention query: for every
// recording z of the pass and every selected head g of this layer
//   s[off[z] + (slot[g] * len_z + i) * T + j] = q[row0_z + i][head[g]] . K[clip_z * T + j][head[g]]
// for i < len_z, j < T: recording z's block is the [A][len_z][T] AlMatArgs.s takes
struct AlPassArgs {
    PfRecs recs;             // as prefill_pass numbered them (row0, max_len set)
    const uint16_t *q;       // pf_q16 [M][n] f16, scaled (k_pf_qkv_store)
    const uint16_t *K;       // the layer's cross keys [Bt][T][n] f16
    float *s;
    int64_t off[DEC_ROWS];   // floats in front of each recording's block
    int n, H, T, A;          // A: slots of a block (the whole head table)
    int nh;                  // selected heads of this layer
    int16_t head[AL_HEADS_MAX], slot[AL_HEADS_MAX];
};
hipError_t launch_align_scores(hipStream_t s, const AlPassArgs &a);

}  // namespace wmi
