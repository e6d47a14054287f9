// wmi_bestof.hip — the fan-out samplers of a best-of-N window (wmi_set_best_of,
// wmi_decode_timestamps_best_of; DESIGN.md "Best-of-N sampled attempts").
//
// The N candidates of a window share the prompt, so the prompt's last step is
// computed once, on one decoder row, and every candidate draws its first
// token from that one row of logits with its own stream key.  From the second
// generated token on the candidates sit on N decoder rows and the step's tail
// is k_ts_sample_t / k_ts_sample_r as it stands.
//
// A translation unit of its own, as wmi_sample.hip and wmi_rules.hip: its code
// object is loaded with the first best-of window, so a context at best_of = 1
// runs on exactly the code objects it ran on before these kernels existed.
// Both kernels are composed from wmi_pick.h.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

namespace wmi {

// One workgroup per candidate c, k_ts_sample_t's conventions with row c of
// everything but the logits: workgroup c reads logits row 0, draws with
// rows[c], and writes tok_out[c], record 0 and plog 0 of row c and done[c];
// workgroup 0 also writes p_nosp[0].  Nothing happens unless the step just
// taken was the prompt's last (generated-token index 0): passes, allowed set
// and record are k_ts_sample_t's at t = 0, so candidate 0 is bitwise that
// kernel's row.
__global__ __launch_bounds__(1024) void k_bestof_fan_t(TsSampArgs sa) {
    const TsArgs &a = sa.t;
    int t;
    if (!samp_begin(a, t) || t != 0) return;
    const int tid = threadIdx.x, c = blockIdx.x;
    const float *lg = a.logits;  // (the one row of the prompt's last step)
    __shared__ RowLds rl;
    __shared__ DrawLds dl;
    dl.tsum[tid] = 0.0;  // (ahead of row_reduce's barriers)
    RowStats r;
    row_reduce(a, lg, rl, r);
    row_probs(lg, rl, r);
    // the first generated token: ids > beg
    const unsigned long long k_a = r.k_ts1;
    const float m_a = pick_key_val(k_a);
    const float T = sa.rows[c].T;
    auto in_a = [&](int i) { return i > a.beg; };
    tile_sums(dl, lg, a.V, in_a, m_a, T);
    int id = pick_key_id(k_a);
    if (T > 0.0f) {
        const double target = draw_tile(dl, sa.rows[c].key, [](int &, double &) {});
        id = draw_id(dl, target, lg, a.V, in_a, m_a, T, a.V - 1);
    }
    if (tid != 0) return;
    samp_feed(a, id);
    if (c == 0) sa.p_nosp[0] = (float)(exp((double)lg[a.solm] - (double)r.mx) / r.Z);
    row_record(a, lg, r, 0, id);
    sa.plog[(size_t)c * a.max_rec] = draw_plog(dl, lg[id], m_a);
}

// the bits of the ids base .. base + 31 that lie in [a, b]
__device__ __forceinline__ uint32_t bo_range_bits(int base, int a, int b) {
    const int lo = a > base ? a - base : 0, hi = b - base < 31 ? b - base : 31;
    if (lo > hi) return 0u;
    return (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo);
}

// The same under the decoding rules: k_ts_sample_r at t = 0, where the
// history counts as empty, so A' = the timestamps outside M0 up to beg +
// max_initial_ts (M2), the pick is among them, and candidate c's history
// after the pick is {last = 1, pen = 0, lts1 = id + 1}.  The bitmask of M0
// comes from where k_ts_sample_r takes it (TsRuleArgs::m0).
__global__ __launch_bounds__(1024) void k_bestof_fan_r(TsRuleArgs ra) {
    const TsArgs &a = ra.s.t;
    int t;
    if (!samp_begin(a, t) || t != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = blockIdx.x;
    const float *lg = a.logits;  // (the one row of the prompt's last step)
    int hi = a.V - 1;
    if (ra.max_initial_ts >= 0 && ra.max_initial_ts < hi - a.beg) hi = a.beg + ra.max_initial_ts;
    __shared__ uint32_t s_ap[2048];
    for (int j = tid; j < (a.V + 31) >> 5; j += 1024) s_ap[j] = ~ra.m0[j] & bo_range_bits(32 * j, a.beg, hi);
    __syncthreads();
    auto in_ap = [&](int i) { return ((s_ap[i >> 5] >> (i & 31)) & 1u) != 0; };
    __shared__ float smax[16];
    __shared__ double ssum[16];
    __shared__ unsigned long long sk[16];
    __shared__ DrawLds dl;
    // pass 1: the unmasked maximum (p_nosp) and the argmax key of A'
    float mx = -INFINITY;
    unsigned long long k_ts = 0;
    for (int i = tid; i < a.V; i += 1024) {
        const float l = lg[i];
        mx = fmaxf(mx, l);
        const unsigned long long k = pick_key(l, i);
        if (in_ap(i)) k_ts = k > k_ts ? k : k_ts;
    }
    mx = wave_max(mx);
    k_ts = wave_max_u64(k_ts);
    if (lane == 0) { smax[w] = mx; sk[w] = k_ts; }
    dl.tsum[tid] = 0.0;  // (ahead of pass 1's barrier)
    __syncthreads();
    mx = smax[0];
    k_ts = sk[0];
    for (int i = 1; i < 16; ++i) {
        mx = fmaxf(mx, smax[i]);
        k_ts = sk[i] > k_ts ? sk[i] : k_ts;
    }
    // (A' is never empty: the timestamps are in no suppress list)
    const float m_p = pick_key_val(k_ts);
    // pass 2: sum of exp(l - m') over A' (all timestamps: sum_ts = 1, and A = A')
    double s = 0.0;
    for (int i = tid; i < a.V; i += 1024)
        if (in_ap(i)) s += exp((double)lg[i] - (double)m_p);
    s = wave_sum(s);
    if (lane == 0) ssum[w] = s;
    __syncthreads();
    double Z = 0.0;
    for (int i = 0; i < 16; ++i) Z += ssum[i];
    const double sum_ts = Z / Z;
    const float m_a = m_p;
    const float T = ra.s.rows[c].T;
    // the unmasked softmax's sum, for p_nosp
    __syncthreads();  // (ssum is read above)
    double su = 0.0;
    for (int i = tid; i < a.V; i += 1024) su += exp((double)lg[i] - (double)mx);
    su = wave_sum(su);
    if (lane == 0) ssum[w] = su;
    __syncthreads();
    double Zu = 0.0;
    for (int i = 0; i < 16; ++i) Zu += ssum[i];
    tile_sums(dl, lg, a.V, in_ap, m_a, T);
    int id = pick_key_id(k_ts);
    if (T > 0.0f) {
        const double target = draw_tile(dl, ra.s.rows[c].key, [&](int &J, double &cs) {
            // (rounding left no group past the target: the last tile with any weight, its last such id)
            #pragma unroll 1
            for (int j = 0; j < 1024; ++j)
                if (dl.tsum[j] > 0.0) J = j;
            cs = -INFINITY;
        });
        id = draw_id(dl, target, lg, a.V, in_ap, m_a, T, id);
    }
    if (tid != 0) return;
    samp_feed(a, id);
    RuleHist hn;
    hn.last = 1;
    hn.pen = 0;
    hn.lts1 = id + 1;
    hn.pad = 0;
    ra.hist[c] = hn;
    if (c == 0) ra.s.p_nosp[0] = (float)(exp((double)lg[a.solm] - (double)mx) / Zu);
    TsRec r;
    r.id = id;
    r.tid = id;
    r.p = (float)(exp((double)lg[id] - (double)m_p) / Z);
    r.pt = (float)((exp((double)lg[id] - (double)m_p) / Z) / (sum_ts + 1e-10));
    r.ptsum = (float)sum_ts;
    r.pad = 0;
    a.rec[(size_t)c * a.max_rec] = r;
    ra.s.plog[(size_t)c * a.max_rec] = draw_plog(dl, lg[id], m_a);
}

// a.B = N candidates; the conditions of launch_ts_sample_t / launch_ts_sample_r
hipError_t launch_bestof_fan(hipStream_t s, const TsRuleArgs &ra, bool ruled) {
    const TsArgs &a = ra.s.t;
    if (a.V < a.beg + 2 || a.V > 65536 || a.B < 1 || a.B > DEC_ROWS || a.max_rec < 1 || !a.logits || !a.st || !a.tok_out ||
        !a.rec || !a.done || !ra.s.rows || !ra.s.plog || !ra.s.p_nosp || a.sot >= a.beg || a.solm >= a.beg ||
        a.not_ >= a.beg || a.solm < 0)
        return hipErrorInvalidValue;
    if (ruled) {
        if (a.eot < 0 || a.eot >= a.beg || !ra.m0 || !ra.hist) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bestof_fan_r, dim3(a.B), dim3(1024), 0, s, ra);
    } else {
        hipLaunchKernelGGL(k_bestof_fan_t, dim3(a.B), dim3(1024), 0, s, ra.s);
    }
    return hipGetLastError();
}

}  // namespace wmi
