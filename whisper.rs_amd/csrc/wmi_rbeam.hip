// wmi_rbeam.hip — the beam-search step under OpenAI's decoding rules
// (wmi_set_rules_beam, wmi_decode_timestamps_ruled_beam; DESIGN.md "Decoding
// rules in the beam window").
//
// A translation unit of its own, as wmi_tsbeam.hip and wmi_rules.hip: its
// code object is loaded with the first ruled beam window, so every other path
// runs on exactly the code objects it ran on before these kernels existed.
// The keys, the split rounds, the row merge and the back half of the select
// are wmi_pick.h's, shared with wmi_tsbeam.hip (the keys and cand_before with
// wmi_kernels.hip too); the mask scalars are derived as in k_ts_sample_r
// (wmi_rules.hip).
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

namespace wmi {

// One vocabulary split of one row.  The row's A' is a predicate over the
// scalars of its hypothesis' history (tx_lo, lo, hi as k_ts_sample_r derives
// them) and the M0 bitmask, read a bit an id: a split boundary or beg inside a
// 32-id word costs nothing.  Whether the row's set is A' or the timestamps of
// A' is known only after the row-wide comparison of sum_ts with p_tx, so the
// split keeps what either outcome needs: the top-(K+1) of both, each set's sum
// of exponentials against that set's own split maximum (accumulated directly,
// never as a difference), the maximum over the text ids of A', and for the
// record the argmax key over all ids >= beg.  Splits without a timestamp id
// (all but the last one or two) skip the timestamp work.
__global__ __launch_bounds__(256) void k_rbeam_part(RBeamArgs ra) {
    const BeamArgs &a = ra.b;
    const int sp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int pos = a.st->pos;
    if (pos < a.feed_len || a.bs->done || b >= a.bs->n_active) return;
    const int t = pos - a.feed_len;
    // the hypothesis' history and the scalars of the mask (empty at the first generated token)
    const RuleHist h = ra.hist[b];
    const bool last = t >= 1 && h.last != 0;
    const bool penult = t < 2 || h.pen != 0;
    const int x = t >= 1 ? h.lts1 - 1 : -1;
    const int tx_lo = t == 0 ? ra.beg : last && !penult ? a.eot : 0;
    int ts_lo = ra.beg, ts_hi = a.V - 1;
    if (x >= 0) ts_lo = last && !penult ? x : x + 1;
    if (last && penult) ts_lo = a.V;
    if (t == 0 && ra.max_initial_ts >= 0 && ra.max_initial_ts < ts_hi - ra.beg) ts_hi = ra.beg + ra.max_initial_ts;
    __shared__ float redf[4];
    __shared__ double redd[2][4];
    __shared__ unsigned long long redk[2][4];
    constexpr int U = SPLIT_U;
    const int chunk = (a.V + BEAM_NS - 1) / BEAM_NS, lo = sp * chunk, hi = min(a.V, lo + chunk);
    const bool has_ts = hi > ra.beg;  // (uniform over the workgroup)
    const float *row = a.logits + (int64_t)b * a.V;
    float v[U];
    split_load(v, row, lo, hi);
    // membership of this thread's ids in A' and in its timestamps, one bit per id
    uint32_t el_a = 0, el_t = 0;
    float m_tx = -INFINITY;
    unsigned long long k_all = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = lo + tid + 256 * u;
        if (i >= hi) { v[u] = -INFINITY; continue; }
        if (i >= ra.beg) k_all = u64max(k_all, pick_key(v[u], i));
        const bool m0 = ((ra.m0[i >> 5] >> (i & 31)) & 1u) != 0;
        const bool ok = !m0 && (i < ra.beg ? i >= tx_lo : i >= ts_lo && i <= ts_hi);
        if (!ok) continue;
        el_a |= 1u << u;
        if (i >= ra.beg) el_t |= 1u << u;
        else m_tx = fmaxf(m_tx, v[u]);
    }
    m_tx = wave_max(m_tx);
    if (has_ts) k_all = wave_max_u64(k_all);
    if (lane == 0) { redf[w] = m_tx; redk[0][w] = k_all; }
    __syncthreads();
    m_tx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    k_all = u64max(u64max(redk[0][0], redk[0][1]), u64max(redk[0][2], redk[0][3]));
    __syncthreads();
    // the two top-(K+1) lists
    RBeamPart *out = ra.rparts + (int64_t)b * BEAM_NS + sp;
    float m_a, m_t;
    split_rounds(v, lo, a.K, el_a, el_t, true, has_ts, redk, m_a, m_t, [&](int r, float va, int ia, float vt, int it) {
        out->ap_val[r] = va;
        out->ap_id[r] = ia;
        out->ts_val[r] = vt;
        out->ts_id[r] = it;
    });
    // the sets' sums, each against its own maximum (one exp where they coincide)
    double s_a = 0.0, s_t = 0.0;
    if (m_a > -INFINITY) {
        const bool do_t = has_ts && m_t > -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!((el_a >> u) & 1u)) continue;
            const double l = (double)v[u], e = exp(l - (double)m_a);
            s_a += e;
            if (do_t && ((el_t >> u) & 1u)) s_t += m_t == m_a ? e : exp(l - (double)m_t);
        }
    }
    s_a = wave_sum(s_a);
    if (has_ts) s_t = wave_sum(s_t);
    if (lane == 0) { redd[0][w] = s_a; redd[1][w] = s_t; }
    __syncthreads();
    if (tid == 0) {
        out->m_tx = m_tx;
        out->pad = 0;
        out->k_all = k_all;
        out->sum_ap = ((redd[0][0] + redd[0][1]) + redd[0][2]) + redd[0][3];
        out->sum_ts = ((redd[1][0] + redd[1][1]) + redd[1][2]) + redd[1][3];
    }
}

// One workgroup, as k_tsbeam_select: per active row the splits merged into
// the softmax quantities over A' (S', sum_ts, p_tx), with them the row's set,
// its log-sum-exp and merged top-(K+1) (beam_row_merge); then the ranking,
// walk and KV history re-pointing (beam_select_tail), a TsRec per new slot and
// per finished hypothesis (under the softmax over A' of the row that produced
// the token), and each new slot's history: its parent's advanced by the id it
// took.  Every parent's history is read before the first barrier and written
// after the last, since slots and parents alias.
__global__ __launch_bounds__(256) void k_rbeam_select(RBeamArgs ra) {
    const BeamArgs &a = ra.b;
    BeamState *bs = a.bs;
    const int pos = a.st->pos;
    if (pos < a.feed_len || bs->done) return;
    const int t = pos - a.feed_len, TK = a.K + 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    struct Lds : BeamSelLds {  // (one block: apart, each array is padded to 16 bytes)
        double row_m[BEAM_MAX], row_z[BEAM_MAX], row_sts[BEAM_MAX];
        float row_pt[BEAM_MAX];
        int row_tid[BEAM_MAX];
        RuleHist h_old[BEAM_MAX];
    };
    __shared__ Lds sl;
    const int na_old = bs->n_active;
    if (tid < BEAM_MAX) sl.h_old[tid] = ra.hist[tid];  // (every parent's history is read ahead of the first barrier)
    auto record = [&](int c) {  // candidate c as sampled from its row
        const int p = c / TK;
        const double pd = exp((double)sl.cval[c] - sl.row_m[p]) / sl.row_z[p];
        const bool ts = sl.cid[c] >= ra.beg;
        TsRec r;
        r.id = sl.cid[c];
        r.tid = ts ? sl.cid[c] : sl.row_tid[p];
        r.p = (float)pd;
        r.pt = ts ? (float)(pd / (sl.row_sts[p] + 1e-10)) : sl.row_pt[p];
        r.ptsum = (float)sl.row_sts[p];
        r.pad = 0;
        return r;
    };
    // 1. per active row: A' merged, the sum_ts vs p_tx decision, the set's log-sum-exp and top-(K+1)
    for (int b = w; b < na_old; b += 4) {
        const RBeamPart *pp = ra.rparts + (int64_t)b * BEAM_NS;
        const bool in = lane < BEAM_NS;
        const float pm = in && pp[lane].ap_id[0] >= 0 ? pp[lane].ap_val[0] : -INFINITY;
        const float M = wave_max(pm);  // (A' is never empty: EOT and the timestamps are in no suppress list)
        const double Z = wave_sum(pm > -INFINITY ? pp[lane].sum_ap * exp((double)pm - (double)M) : 0.0);
        const bool hts = in && pp[lane].ts_id[0] >= 0;
        const float pts = hts ? pp[lane].ts_val[0] : -INFINITY;
        const float Mts = wave_max(pts);
        const double TS = wave_sum(pts > -INFINITY ? pp[lane].sum_ts * exp((double)pts - (double)Mts) : 0.0);
        const float Mtx = wave_max(in ? pp[lane].m_tx : -INFINITY);
        const unsigned long long kts = wave_max_u64(hts ? pick_key(pts, pp[lane].ts_id[0]) : 0ull);
        const unsigned long long kall = wave_max_u64(in ? pp[lane].k_all : 0ull);
        const double p_maxts = kts ? exp((double)Mts - (double)M) / Z : 0.0;
        const double sum_ts = kts ? TS * p_maxts : 0.0;
        const double p_tx = Mtx > -INFINITY ? exp((double)Mtx - (double)M) / Z : 0.0;
        const bool ts_set = sum_ts > p_tx;  // (the same on every lane)
        if (lane == 0) {
            sl.lse[b] = ts_set ? (double)Mts + log(TS) : (double)M + log(Z);
            sl.row_m[b] = (double)M;
            sl.row_z[b] = Z;
            sl.row_sts[b] = sum_ts;
            // a text id's tid: the likeliest timestamp of A', else (A' holds none) of all ids >= beg with pt 0
            sl.row_tid[b] = kts ? pick_key_id(kts) : kall ? pick_key_id(kall) : -1;
            sl.row_pt[b] = kts ? (float)(p_maxts / (sum_ts + 1e-10)) : 0.0f;
        }
        beam_row_merge(TK, [&](int sp, int r, float &val, int &id) {
            const RBeamPart &q = pp[sp];
            id = ts_set ? q.ts_id[r] : q.ap_id[r];
            val = ts_set ? q.ts_val[r] : q.ap_val[r];
        }, sl.cval + b * TK, sl.cid + b * TK);
    }
    // 2 - 4, with the records and the histories: a slot's is written after the
    // tail's last barrier (the slot hook and the lines below it), from h_old
    auto put_hist = [&](int s, RuleHist hn) {
        ra.hist[s] = hn;
        int32_t *tab = ra.hist_tab + ((int64_t)t * BEAM_MAX + s) * 3;
        tab[0] = hn.last;
        tab[1] = hn.pen;
        tab[2] = hn.lts1;
    };
    const int nn = beam_select_tail(a, sl, pos, na_old, [&](int nf, int c) { ra.fin_rec[nf] = record(c); },
                                    [&](int s, int p, int c) {
                                        const int id = sl.cid[c];
                                        const RuleHist hp = sl.h_old[p];
                                        ra.hist_rec[t * BEAM_MAX + s] = record(c);
                                        put_hist(s, RuleHist{id >= ra.beg, t >= 1 ? hp.last : 0,
                                                             id >= ra.beg ? id + 1 : t >= 1 ? hp.lts1 : 0, 0});
                                    });
    if (tid >= nn && tid < BEAM_MAX) put_hist(tid, RuleHist{0, 0, 0, 0});  // the slots left empty
}

hipError_t launch_rbeam_step(hipStream_t s, const RBeamArgs &a) {
    // (the conditions wmi_set_decode_rules enforces: 16 splits of at most 4096 ids, the specials below beg)
    if (a.b.K < 1 || a.b.K > BEAM_MAX || a.b.tctx > 512 || a.b.max_tokens > a.b.tctx || a.b.V > 65536 ||
        (a.b.V + BEAM_NS - 1) / BEAM_NS > 4096 || a.beg < 1 || a.b.V < a.beg + 2 || a.b.eot < 0 || a.b.eot >= a.beg ||
        !a.m0 || !a.hist || !a.rparts || !a.hist_rec || !a.fin_rec || !a.hist_tab)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rbeam_part, dim3(BEAM_NS, a.b.K), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rbeam_select, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
