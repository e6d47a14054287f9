// wmi_wide_rules.hip — the beam step of the wide decoder step under OpenAI's
// decoding rules (wmi_set_decode_rules + wmi_set_rules_beam + wmi_set_batch_beam,
// wmi_decode_timestamps_ruled_beam_rows; DESIGN.md "Beam search in the batch").
//
// The wide step of wmi_wide.hip ends in a beam step for every recording of the
// round.  When the window is ruled the two kernels here stand in the place of
// k_wd_beam_part / k_wd_beam_select: B recordings x K hypotheses, every
// hypothesis with the rule history {last, pen, lts1} of its own ids, carried
// through the parent selection per recording.  As in the rest of the wide step
// nothing that changes from step to step is a kernel argument: the position and
// prompt length (hence t), the BeamState and the histories are read from device
// memory, so a ruled step is one fixed launch sequence and one captured graph.
//
// k_wd_rbeam_part, grid (BEAM_NS, K, B): one vocabulary split of hypothesis k
// of recording c.  The 16 logits a thread holds stay in registers from the load
// to the sums; membership in A' and in its timestamps is a bit per logit, from
// the M0 bitmask (one for the context, shared by all recordings) and the four
// scalars of the hypothesis' history.
// k_wd_rbeam_select, grid B: a workgroup per recording, a wave per row for the
// merge; the K parents' histories go to LDS ahead of the first barrier and the
// slots' new ones are written from there behind the last, so a permutation of
// parents never reads a slot already overwritten.
//
// The split statistics, the rows' decision and the history hand-over are twins
// of k_rbeam_part / k_rbeam_select in wmi_rbeam.hip, repeated here because that
// unit's code object stays what it is: a change to the masks, the sums or the
// history rule is made in both files.  Keys, split_load, split_rounds, the row
// merge, the ranking, the walk and the kv_src re-pointing are wmi_pick.h's.
//
// A translation unit of its own: its code object is loaded with the first ruled
// wide window.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

#pragma clang fp contract(off)

namespace wmi {

// (twin of k_rbeam_part: the recording's block of every array, t from the table)
__global__ __launch_bounds__(256) void k_wd_rbeam_part(WdRBeamArgs ra) {
    const WdBeamArgs &wa = ra.w;
    const int sp = blockIdx.x, b = blockIdx.y, c = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const WdRec rec = wa.tb.recs[c];
    const BeamState *bs = wa.tb.bs + c;
    const int pos = rec.p + 1;
    if (pos < rec.np || bs->done || b >= bs->n_active) return;  // an idle row
    const int t = pos - rec.np, V = wa.V, beg = wa.beg;
    // the hypothesis' history and the scalars of the mask (empty at the first generated token)
    const RuleHist h = ra.rt.hist[c * BEAM_MAX + b];
    const bool last = t >= 1 && h.last != 0;
    const bool penult = t < 2 || h.pen != 0;
    const int x = t >= 1 ? h.lts1 - 1 : -1;
    const int tx_lo = t == 0 ? beg : last && !penult ? wa.eot : 0;
    int ts_lo = beg, ts_hi = V - 1;
    if (x >= 0) ts_lo = last && !penult ? x : x + 1;
    if (last && penult) ts_lo = V;
    if (t == 0 && ra.max_initial_ts >= 0 && ra.max_initial_ts < ts_hi - beg) ts_hi = beg + ra.max_initial_ts;
    __shared__ float redf[4];
    __shared__ double redd[2][4];
    __shared__ unsigned long long redk[2][4];
    constexpr int U = SPLIT_U;
    const int chunk = (V + BEAM_NS - 1) / BEAM_NS, lo = sp * chunk, hi = min(V, lo + chunk);
    const bool has_ts = hi > beg;  // (uniform over the workgroup)
    const float *row = wa.logits + ((int64_t)c * wa.K + b) * V;
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
        if (i >= beg) k_all = u64max(k_all, pick_key(v[u], i));
        const bool m0 = ((ra.m0[i >> 5] >> (i & 31)) & 1u) != 0;
        const bool ok = !m0 && (i < beg ? i >= tx_lo : i >= ts_lo && i <= ts_hi);
        if (!ok) continue;
        el_a |= 1u << u;
        if (i >= beg) el_t |= 1u << u;
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
    RBeamPart *out = ra.rt.rparts + ((int64_t)c * BEAM_MAX + b) * BEAM_NS + sp;
    float m_a, m_t;
    split_rounds(v, lo, wa.K, el_a, el_t, true, has_ts, redk, m_a, m_t, [&](int r, float va, int ia, float vt, int it) {
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

// (twin of k_rbeam_select for recording blockIdx.x; then the recording's position moves on, as in k_wd_beam_select)
__global__ __launch_bounds__(256) void k_wd_rbeam_select(WdRBeamArgs ra) {
    const WdBeamArgs &wa = ra.w;
    const int c = blockIdx.x, tctx = wa.tctx, beg = wa.beg;
    const WdRec rec = wa.tb.recs[c];
    // the recording's argument block of wmi_pick.h's tail
    BeamArgs a{};
    a.logits = wa.logits + (int64_t)c * wa.K * wa.V;
    a.V = wa.V; a.K = wa.K; a.suppress_id = -1; a.eot = wa.eot;
    a.feed_len = rec.np; a.max_tokens = rec.max_tokens; a.tctx = tctx;
    a.bs = wa.tb.bs + c;
    a.kv_src = wa.tb.kv_src + (int64_t)c * BEAM_MAX * tctx;
    a.hist_parent = wa.tb.hist_parent + (int64_t)c * tctx * BEAM_MAX;
    a.hist_tok = wa.tb.hist_tok + (int64_t)c * tctx * BEAM_MAX;
    TsRec *hist_rec = wa.tb.hist_rec + (int64_t)c * (tctx + 1) * BEAM_MAX, *fin_rec = hist_rec + (int64_t)tctx * BEAM_MAX;
    RuleHist *hist = ra.rt.hist + c * BEAM_MAX;
    BeamState *bs = a.bs;
    const int pos = rec.p + 1;
    if (pos < a.feed_len || bs->done) return;  // (a done recording: histories, records and position stand still)
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
    if (tid < BEAM_MAX) sl.h_old[tid] = hist[tid];  // (every parent's history is read ahead of the first barrier)
    auto record = [&](int cd) {  // candidate cd as sampled from its row
        const int p = cd / TK;
        const double pd = exp((double)sl.cval[cd] - sl.row_m[p]) / sl.row_z[p];
        const bool ts = sl.cid[cd] >= beg;
        TsRec r;
        r.id = sl.cid[cd];
        r.tid = ts ? sl.cid[cd] : sl.row_tid[p];
        r.p = (float)pd;
        r.pt = ts ? (float)(pd / (sl.row_sts[p] + 1e-10)) : sl.row_pt[p];
        r.ptsum = (float)sl.row_sts[p];
        r.pad = 0;
        return r;
    };
    // 1. per active row: A' merged, the sum_ts vs p_tx decision, the set's log-sum-exp and top-(K+1)
    for (int b = w; b < na_old; b += 4) {
        const RBeamPart *pp = ra.rt.rparts + ((int64_t)c * BEAM_MAX + b) * BEAM_NS;
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
        beam_row_merge(TK, [&](int s, int r, float &val, int &id) {
            const RBeamPart &q = pp[s];
            id = ts_set ? q.ts_id[r] : q.ap_id[r];
            val = ts_set ? q.ts_val[r] : q.ap_val[r];
        }, sl.cval + b * TK, sl.cid + b * TK);
    }
    // 2 - 4, with the records and the histories: a slot's is written after the tail's last barrier, from h_old
    const int nn = beam_select_tail(a, sl, pos, na_old, [&](int nf, int cd) { fin_rec[nf] = record(cd); },
                                    [&](int s, int p, int cd) {
                                        const int id = sl.cid[cd];
                                        const RuleHist hp = sl.h_old[p];
                                        hist_rec[t * BEAM_MAX + s] = record(cd);
                                        hist[s] = RuleHist{id >= beg, t >= 1 ? hp.last : 0,
                                                           id >= beg ? id + 1 : t >= 1 ? hp.lts1 : 0, 0};
                                    });
    if (tid >= nn && tid < BEAM_MAX) hist[tid] = RuleHist{0, 0, 0, 0};  // the slots left empty
    if (tid == 0) wa.tb.recs[c].p = pos;  // (every thread read it before the tail's barriers)
}

hipError_t launch_wd_rbeam_step(hipStream_t s, const WdRBeamArgs &ra) {
    const WdBeamArgs &a = ra.w;
    // (launch_wd_beam_step's conditions and launch_rbeam_step's: 16 splits of at most 4096 ids, the specials below beg)
    if (a.K < 1 || a.K > BEAM_MAX || a.B < 1 || a.B * a.K > WD_ROWS || a.tctx > 512 || a.V > 65536 ||
        (a.V + BEAM_NS - 1) / BEAM_NS > 4096 || a.beg < 1 || a.V < a.beg + 2 || a.eot < 0 || a.eot >= a.beg || !ra.m0 ||
        !ra.rt.hist || !ra.rt.rparts)
        return hipErrorInvalidValue;
    hipError_t e;
    if (a.lg_all && (e = launch_wd_logits_capture(s, a)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wd_rbeam_part, dim3(BEAM_NS, a.K, a.B), dim3(256), 0, s, ra);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wd_rbeam_select, dim3(a.B), dim3(256), 0, s, ra);
    return hipGetLastError();
}

}  // namespace wmi
