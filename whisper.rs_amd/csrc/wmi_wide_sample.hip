// wmi_wide_sample.hip — sampled rows on the wide decoder step
// (wmi_decode_timestamps_sampled_rows; DESIGN.md "Sampled rows on the wide step").
//
// A sampled wide window holds B recordings of W row slots, row r = c W + k
// candidate k of recording c, B W <= 64.  The step up to the logits is
// wmi_wide.hip's with K = W; its tail is here: the temperature sampler of every
// (candidate, recording), then one wave a recording that moves the position on.
//
// k_wd_sample: grid (W, B), one workgroup of 1024 threads per candidate, so
// blockIdx.x is the candidate's row inside its recording's blocks and
// wmi_pick.h's row helpers index them as they index the eight-row samplers'
// (row_record writes rec[blockIdx.x][t]).  Everything that changes from step to
// step is read from the device tables (WdTable, WdSampTable): the step's launch
// sequence is one captured graph.  At t = 0 a recording has one live row (its
// prompt's last position, n_active = 1): every candidate draws its first token
// from that row with its own stream key, wmi_bestof.hip's fan-out with nothing
// copied.  From t = 1 on candidate k reads row c W + k.  The pick is
// k_ts_sample_t's, with `ruled` k_ts_sample_r's: the passes, the allowed set,
// the draw, the record and the log-probability are wmi_pick.h's one copy; the
// ruled pick is wmi_pick.h's pick_ruled, k_ts_sample_r's body restated word for
// word (wmi_rules.hip keeps its own until it calls that function: a change to
// the set or the record is made in both), so equal logits give the same bits.  A candidate that drew EOT returns at once from then on: its slot of
// BeamState::tok keeps EOT, which its row goes on feeding.
//
// k_wd_sample_advance: grid B, one wave.  Behind the samplers it opens the
// recording's N_c rows after t = 0, moves p_c on and raises the recording's
// done word when every candidate has met EOT, at max_tokens, or at the
// context's end; no sampler has to know whether it is the last to arrive.
//
// k_wd_no_speech: grid B, k_no_speech for every recording of a beam window
// that runs under the fallback, launched ahead of the beam step.
//
// A translation unit of its own: its code object is loaded with the first
// sampled wide window, so a context that never runs one runs on the code
// objects it ran on before.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

#pragma clang fp contract(off)

namespace wmi {

namespace {

// k_ts_sample_t's body behind its prologue: the id (thread 0's), record t and its log-probability
__device__ __forceinline__ int ws_pick_t(const TsArgs &a, const float *lg, int t, const SampRow row, float *plog,
                                         float *p_nosp) {
    const int tid = threadIdx.x;
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
    const float T = row.T;
    auto in_a = [&](int i) {
        return set == 0 ? i > a.beg : set == 1 ? i >= a.beg : (i != a.sot && i != a.solm && i != a.not_);
    };
    tile_sums(dl, lg, a.V, in_a, m_a, T);
    int id = pick_key_id(k_a);
    if (T > 0.0f) {
        const double target = draw_tile(dl, row.key + (unsigned long long)t, [](int &, double &) {});
        id = draw_id(dl, target, lg, a.V, in_a, m_a, T, a.V - 1);
    }
    if (tid != 0) return id;
    if (p_nosp) *p_nosp = (float)(exp((double)lg[a.solm] - (double)r.mx) / r.Z);
    if (t < a.max_rec) {
        row_record(a, lg, r, t, id);
        plog[t] = draw_plog(dl, lg[id], m_a);
    }
    return id;
}

}  // namespace

template <bool RULED>
__global__ __launch_bounds__(1024) void k_wd_sample(WdSampArgs sa) {
    const int k = blockIdx.x, c = blockIdx.y, W = sa.W;
    const WdRec rec = sa.tb.recs[c];
    BeamState *bs = sa.tb.bs + c;
    const int t = rec.p + 1 - rec.np;  // the generated token's index (the prompt's last position is t = 0)
    if (t < 0 || bs->done || k >= sa.st.ncand[c]) return;  // (uniform; the done word is raised by k_wd_sample_advance)
    const int64_t slot = (int64_t)c * W + k;
    if (t > 0 && sa.st.done[slot]) return;  // (tok[k] holds EOT)
    // rows of the recording's blocks as the pick helpers index them: blockIdx.x = k
    TsArgs a{};
    a.V = sa.V; a.beg = sa.beg; a.eot = sa.eot; a.sot = sa.sot; a.solm = sa.solm; a.not_ = sa.not_; a.max_rec = sa.max_rec;
    a.rec = sa.st.rec + (int64_t)c * W * sa.max_rec;
    const float *lg = sa.logits + ((int64_t)c * W + (t == 0 ? 0 : k)) * sa.V;
    float *plog = sa.st.plog + slot * sa.max_rec;
    float *p_nosp = t == 0 && k == 0 ? sa.st.p_nosp + c : nullptr;
    const SampRow row = sa.st.rows[slot];
    const int id = RULED ? pick_ruled(a, lg, t, row, plog, p_nosp, sa.m0, sa.max_initial_ts, sa.st.hist + slot)
                         : ws_pick_t(a, lg, t, row, plog, p_nosp);
    if (threadIdx.x != 0) return;
    bs->tok[k] = id;
    if (id == sa.eot) sa.st.done[slot] = 1;
}

__global__ __launch_bounds__(64) void k_wd_sample_advance(WdSampArgs sa) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const WdRec rec = sa.tb.recs[c];
    BeamState *bs = sa.tb.bs + c;
    const int t = rec.p + 1 - rec.np;
    if (t < 0 || bs->done) return;
    const int N = sa.st.ncand[c];
    const bool live = lane < N && sa.st.done[(int64_t)c * sa.W + lane] == 0;
    const bool any = __ballot(live) != 0ull;
    if (lane != 0) return;
    bs->n_active = N;
    bs->n_steps = t + 1;
    sa.tb.recs[c].p = rec.p + 1;
    if (!any || t + 1 >= rec.max_tokens || rec.p + 1 >= sa.tctx) bs->done = 1;
}

hipError_t launch_wd_sample_step(hipStream_t s, const WdSampArgs &a, bool ruled) {
    // (launch_ts_sample_t's conditions: the tile sums fill 1024 LDS slots of 64 ids; the specials lie below beg)
    if (a.W < 1 || a.W > BEAM_MAX || a.B < 1 || a.B * a.W > WD_ROWS || a.V < a.beg + 2 || a.V > 65536 || a.max_rec < 1 ||
        a.tctx > 512 || !a.logits || !a.st.rows || !a.st.done || !a.st.ncand || !a.st.rec || !a.st.plog || !a.st.p_nosp ||
        a.sot >= a.beg || a.solm >= a.beg || a.not_ >= a.beg || a.solm < 0)
        return hipErrorInvalidValue;
    if (ruled) {
        if (a.eot < 0 || a.eot >= a.beg || !a.m0 || !a.st.hist) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_wd_sample<true>, dim3(a.W, a.B), dim3(1024), 0, s, a);
    } else {
        hipLaunchKernelGGL(k_wd_sample<false>, dim3(a.W, a.B), dim3(1024), 0, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_wd_sample_advance, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---- the no-speech probability of every recording of a beam window ------------------
// k_no_speech (wmi_sample.hip) per recording: exp(l_solm - max) / Z in double over row c K of the step's logits
__global__ __launch_bounds__(256) void k_wd_no_speech(WdTable tb, const float *logits, int K, int V, int solm, float *p_nosp) {
    const int c = blockIdx.x;
    const WdRec rec = tb.recs[c];
    if (rec.p != rec.np - 1 || tb.bs[c].done) return;  // (uniform) not the first generated step
    const float *lg = logits + (int64_t)c * K * V;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ float smax[4];
    __shared__ double ssum[4];
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 256) mx = fmaxf(mx, lg[i]);
    mx = wave_max(mx);
    if (lane == 0) smax[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    double s = 0.0;
    for (int i = tid; i < V; i += 256) s += exp((double)lg[i] - (double)mx);
    s = wave_sum(s);
    if (lane == 0) ssum[w] = s;
    __syncthreads();
    if (tid != 0) return;
    const double Z = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
    p_nosp[c] = (float)(exp((double)lg[solm] - (double)mx) / Z);
}

hipError_t launch_wd_no_speech(hipStream_t s, const WdTable &tb, const float *logits, int B, int K, int V, int solm,
                               float *p_nosp) {
    if (B < 1 || K < 1 || K > BEAM_MAX || B * K > WD_ROWS || V < 1 || solm < 0 || solm >= V || !logits || !p_nosp)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_no_speech, dim3(B), dim3(256), 0, s, tb, logits, K, V, solm, p_nosp);
    return hipGetLastError();
}

}  // namespace wmi
