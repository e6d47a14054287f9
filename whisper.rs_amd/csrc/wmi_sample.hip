// wmi_sample.hip — the temperature sampler of the timestamped decoder and the
// no-speech probability of a beam window (wmi_set_fallback,
// wmi_decode_timestamps_sampled; DESIGN.md "Temperature fallback").
//
// A translation unit of its own, as wmi_tsbeam.hip: its code object is loaded
// with the first sampled window, so a context whose fallback parameters are
// the defaults runs on exactly the code objects it ran on before these kernels
// existed.  The keys, the row statistics it has in common with k_ts_sample and
// the draw it has in common with k_ts_sample_r are wmi_pick.h's.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

namespace wmi {

// One workgroup per decoder row b, k_ts_sample's conventions (done words,
// tok_out, records).  Passes 1 and 2 and the record are k_ts_sample's own code
// (row_reduce, row_probs, row_record), so the record {id, tid, p, pt, ptsum}
// of a T = 0 row is bitwise what k_ts_sample writes.  The allowed set A (the
// timestamp rule) is known after pass 2; its maximum is the value in the set's
// argmax key.  Pass 3 goes over A in tiles of 64 consecutive ids (tile_sums):
// the sum of exp(l - m_A) for plog, and for T > 0 each tile's sum of the
// weights w = exp((l - m_A) / T).  The draw u Q is then located by wave 0
// (draw_tile, draw_id).
__global__ __launch_bounds__(1024) void k_ts_sample_t(TsSampArgs sa) {
    const TsArgs &a = sa.t;
    int t;
    if (!samp_begin(a, t)) return;
    const int tid = threadIdx.x, b = blockIdx.x;
    const float *lg = a.logits + (size_t)b * a.V;
    __shared__ RowLds rl;
    __shared__ DrawLds dl;
    dl.tsum[tid] = 0.0;  // (ahead of row_reduce's barriers)
    RowStats r;
    row_reduce(a, lg, rl, r);
    row_probs(lg, rl, r);
    // the allowed set: 0 ids > beg, 1 ids >= beg, 2 every id but sot / solm / not
    const int set = t == 0 ? 0 : r.sum_ts > r.p_maxtx ? 1 : 2;
    const unsigned long long k_a = set == 0 ? r.k_ts1 : set == 1 ? r.k_ts : r.k_all;
    const float m_a = pick_key_val(k_a);
    const float T = sa.rows[b].T;
    auto in_a = [&](int i) {
        return set == 0 ? i > a.beg : set == 1 ? i >= a.beg : (i != a.sot && i != a.solm && i != a.not_);
    };
    tile_sums(dl, lg, a.V, in_a, m_a, T);
    int id = pick_key_id(k_a);
    if (T > 0.0f) {
        // (no group or no tile past the target after rounding: the largest id of A;
        // sot, solm and not lie below beg, so the last id belongs to every set)
        const double target = draw_tile(dl, sa.rows[b].key + (unsigned long long)t, [](int &, double &) {});
        id = draw_id(dl, target, lg, a.V, in_a, m_a, T, a.V - 1);
    }
    if (tid != 0) return;
    samp_feed(a, id);
    if (t == 0) sa.p_nosp[b] = (float)(exp((double)lg[a.solm] - (double)r.mx) / r.Z);
    if (t < a.max_rec) {
        row_record(a, lg, r, t, id);
        sa.plog[(size_t)b * a.max_rec + t] = draw_plog(dl, lg[id], m_a);
    }
}

hipError_t launch_ts_sample_t(hipStream_t s, const TsSampArgs &sa) {
    const TsArgs &a = sa.t;
    // (the tile sums fill 1024 LDS slots of 64 ids; the largest id of a set is
    // V - 1 only while sot, solm and not lie below beg)
    if (a.V < a.beg + 2 || a.V > 65536 || a.B < 1 || a.B > DEC_ROWS || !a.done || !sa.rows || !sa.plog || !sa.p_nosp ||
        a.sot >= a.beg || a.solm >= a.beg || a.not_ >= a.beg || a.solm < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ts_sample_t, dim3(a.B), dim3(1024), 0, s, sa);
    return hipGetLastError();
}

// The no-speech probability of a beam window: after the window's first
// generated step (pos == feed_len) one workgroup reads row 0 of the step's
// logits (step 0 expands hypothesis 0 only): exp(l_solm - max) / Z in double.
__global__ __launch_bounds__(256) void k_no_speech(NoSpeechArgs a) {
    if (a.st->pos != a.feed_len) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ float smax[4];
    __shared__ double ssum[4];
    float mx = -INFINITY;
    for (int i = tid; i < a.V; i += 256) mx = fmaxf(mx, a.logits[i]);
    mx = wave_max(mx);
    if (lane == 0) smax[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    double s = 0.0;
    for (int i = tid; i < a.V; i += 256) s += exp((double)a.logits[i] - (double)mx);
    s = wave_sum(s);
    if (lane == 0) ssum[w] = s;
    __syncthreads();
    if (tid != 0) return;
    const double Z = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
    *a.p_nosp = (float)(exp((double)a.logits[a.solm] - (double)mx) / Z);
}

hipError_t launch_no_speech(hipStream_t s, const NoSpeechArgs &a) {
    if (a.V < 1 || a.solm < 0 || a.solm >= a.V || !a.logits || !a.st || !a.p_nosp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_no_speech, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
