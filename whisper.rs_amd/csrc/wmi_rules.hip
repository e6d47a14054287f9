// wmi_rules.hip — the timestamp sampler under OpenAI's decoding rules
// (SuppressTokens and ApplyTimestampRules restated; wmi_set_decode_rules,
// wmi_decode_timestamps_ruled; DESIGN.md "OpenAI decoding rules").
//
// A translation unit of its own, as wmi_sample.hip and wmi_tsbeam.hip: its
// code object is loaded with the first ruled window, so a context whose rules
// are off runs on exactly the code objects it ran on before this kernel
// existed.  The keys, the prologue and the draw it has in common with
// k_ts_sample_t are wmi_pick.h's.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

namespace wmi {

// the bits of the ids base .. base + 31 that lie in [a, b]
__device__ __forceinline__ uint32_t range_bits(int base, int a, int b) {
    const int lo = a > base ? a - base : 0, hi = b - base < 31 ? b - base : 31;
    if (lo > hi) return 0u;
    return (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo);
}

// One workgroup per decoder row b, k_ts_sample_t's conventions (done words,
// tok_out, records, plog, p_nosp, per-row {T, key}).  The masks M0 - M2 are a
// predicate over four per-row scalars and the device bitmask of M0: a text id
// (< beg) is allowed from tx_lo on, a timestamp inside [lo, hi].  The scalars
// follow from the row's history {last, penult, last timestamp}, which thread
// 0 advances after the pick; at the first generated token the history counts
// as empty whatever the words hold.  The predicate is evaluated once, 32 ids
// a thread, into a bitmask of A' in LDS (8 KB at 65536 ids); the passes test
// a bit of it (lanes 0..31 and 32..63 of a wave read one word each: broadcast).
//   pass 1  over all ids: the unmasked maximum (p_nosp), the argmax keys of
//           A' over its timestamps and over its text ids, and of all ids >= beg
//   pass 2  over A': sum of exp(l - m') and its timestamp part, m' = max over A'
//   (t == 0 only: the unmasked sum for p_nosp)
//   pass 3  over A in tiles of 64 ids, as k_ts_sample_t: sum exp(l - m_A) for
//           plog, and for T > 0 the tile sums of exp((l - m_A) / T); the draw
//           is located by wave 0 (groups of 16 tiles, tile, id)
__global__ __launch_bounds__(1024) void k_ts_sample_r(TsRuleArgs ra) {
    const TsArgs &a = ra.s.t;
    int t;
    if (!samp_begin(a, t)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const float *lg = a.logits + (size_t)b * a.V;
    // the row's history and the scalars of the mask
    const RuleHist h = ra.hist[b];
    const bool last = t >= 1 && h.last != 0;
    const bool penult = t < 2 || h.pen != 0;
    const int x = t >= 1 ? h.lts1 - 1 : -1;  // the last timestamp sampled in this window (-1: none)
    const int tx_lo = t == 0 ? a.beg : last && !penult ? a.eot : 0;
    int lo = a.beg, hi = a.V - 1;
    if (x >= 0) lo = last && !penult ? x : x + 1;
    if (last && penult) lo = a.V;
    if (t == 0 && ra.max_initial_ts >= 0 && ra.max_initial_ts < hi - a.beg) hi = a.beg + ra.max_initial_ts;
    __shared__ uint32_t s_ap[2048];
    for (int j = tid; j < (a.V + 31) >> 5; j += 1024)
        s_ap[j] = ~ra.m0[j] & (range_bits(32 * j, tx_lo, a.beg - 1) | range_bits(32 * j, lo, hi));
    __syncthreads();
    auto in_ap = [&](int i) { return ((s_ap[i >> 5] >> (i & 31)) & 1u) != 0; };
    __shared__ float smax[16];
    __shared__ double ssum[16], sts[16];
    __shared__ unsigned long long sk[3][16];
    __shared__ DrawLds dl;
    float mx = -INFINITY;
    unsigned long long k_ts = 0, k_tx = 0, k_tsall = 0;
    for (int i = tid; i < a.V; i += 1024) {
        const float l = lg[i];
        mx = fmaxf(mx, l);
        const unsigned long long k = pick_key(l, i);
        if (i >= a.beg) k_tsall = k > k_tsall ? k : k_tsall;
        if (in_ap(i)) {
            if (i >= a.beg) k_ts = k > k_ts ? k : k_ts;
            else k_tx = k > k_tx ? k : k_tx;
        }
    }
    mx = wave_max(mx);
    k_ts = wave_max_u64(k_ts);
    k_tx = wave_max_u64(k_tx);
    k_tsall = wave_max_u64(k_tsall);
    if (lane == 0) { smax[w] = mx; sk[0][w] = k_ts; sk[1][w] = k_tx; sk[2][w] = k_tsall; }
    dl.tsum[tid] = 0.0;  // (ahead of pass 1's barrier)
    __syncthreads();
    mx = smax[0];
    k_ts = sk[0][0]; k_tx = sk[1][0]; k_tsall = sk[2][0];
    for (int i = 1; i < 16; ++i) {
        mx = fmaxf(mx, smax[i]);
        k_ts = sk[0][i] > k_ts ? sk[0][i] : k_ts;
        k_tx = sk[1][i] > k_tx ? sk[1][i] : k_tx;
        k_tsall = sk[2][i] > k_tsall ? sk[2][i] : k_tsall;
    }
    // (A' is never empty: EOT and the timestamps are in no suppress list)
    const unsigned long long k_ap = k_ts > k_tx ? k_ts : k_tx;
    const float m_p = pick_key_val(k_ap);
    double s = 0.0, st = 0.0;
    for (int i = tid; i < a.V; i += 1024) {
        if (!in_ap(i)) continue;
        const double e = exp((double)lg[i] - (double)m_p);
        s += e;
        if (i >= a.beg) st += e;
    }
    s = wave_sum(s);
    st = wave_sum(st);
    if (lane == 0) { ssum[w] = s; sts[w] = st; }
    __syncthreads();
    double Z = 0.0, TS = 0.0;
    for (int i = 0; i < 16; ++i) { Z += ssum[i]; TS += sts[i]; }
    const double sum_ts = TS / Z;
    const double p_maxtx = k_tx ? exp((double)pick_key_val(k_tx) - (double)m_p) / Z : 0.0;
    const bool ts_only = sum_ts > p_maxtx;
    const unsigned long long k_a = ts_only ? k_ts : k_ap;
    const float m_a = pick_key_val(k_a);
    const float T = ra.s.rows[b].T;
    auto in_a = [&](int i) { return (!ts_only || i >= a.beg) && in_ap(i); };
    double Zu = 0.0;
    if (t == 0) {  // the unmasked softmax's sum, for p_nosp
        __syncthreads();  // (ssum is read above)
        double su = 0.0;
        for (int i = tid; i < a.V; i += 1024) su += exp((double)lg[i] - (double)mx);
        su = wave_sum(su);
        if (lane == 0) ssum[w] = su;
        __syncthreads();
        for (int i = 0; i < 16; ++i) Zu += ssum[i];
    }
    tile_sums(dl, lg, a.V, in_a, m_a, T);
    int id = pick_key_id(k_a);
    if (T > 0.0f) {
        const double target = draw_tile(dl, ra.s.rows[b].key + (unsigned long long)t, [&](int &J, double &c) {
            // (rounding left no group past the target: the last tile with any weight, its last such id)
            #pragma unroll 1
            for (int j = 0; j < 1024; ++j)
                if (dl.tsum[j] > 0.0) J = j;
            c = -INFINITY;
        });
        // (a tile there is: A holds m_A's id, whose weight is 1; the argmax stands in for none)
        id = draw_id(dl, target, lg, a.V, in_a, m_a, T, id);
    }
    if (tid != 0) return;
    samp_feed(a, id);
    RuleHist hn;
    hn.last = id >= a.beg;
    hn.pen = t >= 1 ? h.last : 0;
    hn.lts1 = id >= a.beg ? id + 1 : t >= 1 ? h.lts1 : 0;
    hn.pad = 0;
    ra.hist[b] = hn;
    if (t == 0) ra.s.p_nosp[b] = (float)(exp((double)lg[a.solm] - (double)mx) / Zu);
    if (t < a.max_rec) {
        // tid: the id itself if a timestamp, else the best timestamp of A', else (A' holds none) of all
        const bool tid_in = id >= a.beg || k_ts != 0;
        const int id_t = id >= a.beg ? id : pick_key_id(k_ts ? k_ts : k_tsall);
        TsRec r;
        r.id = id;
        r.tid = id_t;
        r.p = (float)(exp((double)lg[id] - (double)m_p) / Z);
        r.pt = tid_in ? (float)((exp((double)lg[id_t] - (double)m_p) / Z) / (sum_ts + 1e-10)) : 0.0f;
        r.ptsum = (float)sum_ts;
        r.pad = 0;
        a.rec[(size_t)b * a.max_rec + t] = r;
        ra.s.plog[(size_t)b * a.max_rec + t] = draw_plog(dl, lg[id], m_a);
    }
}

hipError_t launch_ts_sample_r(hipStream_t s, const TsRuleArgs &ra) {
    const TsArgs &a = ra.s.t;
    // (launch_ts_sample_t's conditions: the tile sums fill 1024 LDS slots of 64 ids; the specials lie below beg)
    if (a.V < a.beg + 2 || a.V > 65536 || a.B < 1 || a.B > DEC_ROWS || !a.done || !ra.s.rows || !ra.s.plog || !ra.s.p_nosp ||
        a.sot >= a.beg || a.solm >= a.beg || a.not_ >= a.beg || a.solm < 0 || a.eot < 0 || a.eot >= a.beg || !ra.m0 || !ra.hist)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ts_sample_r, dim3(a.B), dim3(1024), 0, s, ra);
    return hipGetLastError();
}

}  // namespace wmi
