// wmi_rules.hip — the timestamp sampler under OpenAI's decoding rules
// (SuppressTokens and ApplyTimestampRules restated; wmi_set_decode_rules,
// wmi_decode_timestamps_ruled; DESIGN.md "OpenAI decoding rules").
//
// A translation unit of its own, as wmi_sample.hip and wmi_tsbeam.hip: its
// code object is loaded with the first ruled window, so a context whose rules
// are off runs on exactly the code objects it ran on before this kernel
// existed.  The key helpers and sm64 restate wmi_sample.hip's.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

namespace wmi {

__device__ __forceinline__ unsigned long long ts_key(float v, int id) {
    return ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
}
__device__ __forceinline__ int ts_key_id(unsigned long long k) { return (int)(0xffffffffu - (uint32_t)(k & 0xffffffffu)); }
__device__ __forceinline__ float ts_key_val(unsigned long long k) { return unord_f32((uint32_t)(k >> 32)); }

__device__ __forceinline__ unsigned long long sm64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

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
    const int pos = a.st->pos;
    if (pos < a.feed_len) return;  // still feeding the prompt
    const int t = pos - a.feed_len;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    if (a.done[b]) {  // (uniform over the workgroup; set by a previous launch)
        if (tid == 0) a.tok_out[b] = a.eot;
        return;
    }
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
    __shared__ double ssum[16], sts[16], sse[16];
    __shared__ unsigned long long sk[3][16];
    __shared__ double tsum[1024], gsum[64], wl[64], c_tile;
    __shared__ int j_tile;
    float mx = -INFINITY;
    unsigned long long k_ts = 0, k_tx = 0, k_tsall = 0;
    for (int i = tid; i < a.V; i += 1024) {
        const float l = lg[i];
        mx = fmaxf(mx, l);
        const unsigned long long k = ts_key(l, i);
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
    tsum[tid] = 0.0;
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
    const float m_p = ts_key_val(k_ap);
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
    const double p_maxtx = k_tx ? exp((double)ts_key_val(k_tx) - (double)m_p) / Z : 0.0;
    const bool ts_only = sum_ts > p_maxtx;
    const unsigned long long k_a = ts_only ? k_ts : k_ap;
    const float m_a = ts_key_val(k_a);
    const float T = ra.s.rows[b].T;
    const bool draw = T > 0.0f;
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
    // pass 3: tiles of 64 consecutive ids
    const int nt = (a.V + 63) >> 6;
    double se = 0.0;
    // (one exp per loop, as in k_ts_sample_t: both in one body spill)
    for (int j = w; j < nt; j += 16) {
        const int i = j * 64 + lane;
        if (i < a.V && in_a(i)) se += exp((double)lg[i] - (double)m_a);
    }
    if (draw)
        for (int j = w; j < nt; j += 16) {
            const int i = j * 64 + lane;
            const bool in = i < a.V && in_a(i);
            const double wt = wave_sum(in ? exp(((double)lg[i] - (double)m_a) / (double)T) : 0.0);
            if (lane == 0) tsum[j] = wt;
        }
    se = wave_sum(se);
    if (lane == 0) sse[w] = se;
    __syncthreads();
    int id = ts_key_id(k_a);
    double target = 0.0;
    if (draw) {
        if (w == 0) {
            double g = 0.0;
            for (int k = 0; k < 16; ++k) g += tsum[16 * lane + k];
            gsum[lane] = g;
        }
        __syncthreads();
        if (tid == 0) {
            double Q = 0.0;
            #pragma unroll 1
            for (int g = 0; g < 64; ++g) Q += gsum[g];
            const double u = (double)(sm64(ra.s.rows[b].key + (unsigned long long)t) >> 11) * 0x1.0p-53;
            target = u * Q;
            double c = 0.0;
            int G = -1;
            #pragma unroll 1
            for (int g = 0; g < 64; ++g) {
                if (c + gsum[g] > target) { G = g; break; }
                c += gsum[g];
            }
            int J = -1;
            double cj = c;
            if (G >= 0) {
                // (rounding may leave no tile of the group past the target: its last tile with any weight)
                #pragma unroll 1
                for (int k = 0; k < 16; ++k) {
                    const int j = 16 * G + k;
                    if (tsum[j] > 0.0) { J = j; cj = c; }
                    if (c + tsum[j] > target) break;
                    c += tsum[j];
                }
            } else {
                // (rounding left no group past the target: the last tile with any weight, its last such id)
                #pragma unroll 1
                for (int j = 0; j < 1024; ++j)
                    if (tsum[j] > 0.0) J = j;
                cj = -INFINITY;
            }
            j_tile = J;
            c_tile = cj;
        }
        __syncthreads();
        const int J = j_tile;  // (uniform; >= 0: A holds m_A's id, whose weight is 1)
        if (J >= 0 && w == 0) {
            const int i = J * 64 + lane;
            wl[lane] = i < a.V && in_a(i) ? exp(((double)lg[i] - (double)m_a) / (double)T) : 0.0;
        }
        __syncthreads();
        if (tid == 0 && J >= 0) {
            double c = c_tile;
            #pragma unroll 1
            for (int k = 0; k < 64; ++k) {
                if (wl[k] > 0.0) id = J * 64 + k;
                if (c + wl[k] > target) break;
                c += wl[k];
            }
        }
    }
    if (tid != 0) return;
    double SE = 0.0;
    for (int i = 0; i < 16; ++i) SE += sse[i];
    a.tok_out[b] = id;
    if (id == a.eot) a.done[b] = 1;
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
        const int id_t = id >= a.beg ? id : ts_key_id(k_ts ? k_ts : k_tsall);
        TsRec r;
        r.id = id;
        r.tid = id_t;
        r.p = (float)(exp((double)lg[id] - (double)m_p) / Z);
        r.pt = tid_in ? (float)((exp((double)lg[id_t] - (double)m_p) / Z) / (sum_ts + 1e-10)) : 0.0f;
        r.ptsum = (float)sum_ts;
        r.pad = 0;
        a.rec[(size_t)b * a.max_rec + t] = r;
        ra.s.plog[(size_t)b * a.max_rec + t] = (float)((double)lg[id] - ((double)m_a + log(SE)));
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
