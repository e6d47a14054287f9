// wmi_tsbeam.hip — the beam-search step under the timestamp rule
// (wmi_decode_timestamps_beam, wmi_transcribe with wmi_set_beam_size > 1).
//
// A translation unit of its own: its code object is loaded with the first
// timestamped beam window, so a process that never asks for one runs on
// exactly the code objects it ran on before these kernels existed (the
// greedy, beam and timestamp paths of wmi_kernels.hip are byte for byte what
// they were).  The keys, the split rounds, the row merge and the back half of
// the select are wmi_pick.h's, shared with wmi_rbeam.hip (the keys and
// cand_before with wmi_kernels.hip too).
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

namespace wmi {

// ============================================================================
// beam search step under the timestamp rule (k_ts_sample's rule per hypothesis
// row, k_beam_select's ranking; DESIGN.md "Beam search in timestamped decoding")
// ============================================================================
// One vocabulary split of one row.  A row's allowed set is known only after
// the row-wide comparison of sum_ts with p_tx, so the split keeps what either
// outcome needs: its top-(K+1) among the timestamp ids and among every id but
// sot / solm / not, and each set's sum of exponentials against that set's own
// split maximum (accumulated directly, never as a difference).  Splits without
// a timestamp id (all but the last one or two) skip the timestamp work.
__global__ __launch_bounds__(256) void k_tsbeam_part(TsBeamArgs ta) {
    const BeamArgs &a = ta.b;
    const int sp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int pos = a.st->pos;
    if (pos < a.feed_len || a.bs->done || b >= a.bs->n_active) return;
    const bool first = pos == a.feed_len;  // t = 0: the allowed set is ids > beg
    __shared__ float redf[2][4];
    __shared__ double redd[4][4];
    __shared__ unsigned long long redk[2][4];
    constexpr int U = SPLIT_U;
    const int chunk = (a.V + BEAM_NS - 1) / BEAM_NS, lo = sp * chunk, hi = min(a.V, lo + chunk);
    const bool has_ts = hi > ta.beg;  // (uniform over the workgroup)
    const float *row = a.logits + (int64_t)b * a.V;
    float v[U];
    split_load(v, row, lo, hi);
    // eligibility of this thread's ids for the two lists, one bit per id
    uint32_t el_a = 0, el_t = 0;
    float m_all = -INFINITY, m_tx = -INFINITY;
    unsigned long long k_ts = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = lo + tid + 256 * u;
        if (i >= hi) { v[u] = -INFINITY; continue; }
        m_all = fmaxf(m_all, v[u]);
        if (i < ta.beg) m_tx = fmaxf(m_tx, v[u]);
        else k_ts = u64max(k_ts, pick_key(v[u], i));
        if (!first && i != ta.sot && i != ta.solm && i != ta.not_) el_a |= 1u << u;
        if (first ? i > ta.beg : i >= ta.beg) el_t |= 1u << u;
    }
    m_all = wave_max(m_all);
    m_tx = wave_max(m_tx);
    if (has_ts) k_ts = wave_max_u64(k_ts);
    if (lane == 0) { redf[0][w] = m_all; redf[1][w] = m_tx; redk[0][w] = k_ts; }
    __syncthreads();
    m_all = fmaxf(fmaxf(redf[0][0], redf[0][1]), fmaxf(redf[0][2], redf[0][3]));
    m_tx = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
    k_ts = u64max(u64max(redk[0][0], redk[0][1]), u64max(redk[0][2], redk[0][3]));
    const float m_ts = k_ts ? pick_key_val(k_ts) : -INFINITY;
    __syncthreads();
    // the two top-(K+1) lists (at the first token the first list's set is empty: its reduction is skipped)
    TsBeamPart *out = ta.tparts + (int64_t)b * BEAM_NS + sp;
    float m_a, m_tl;
    split_rounds(v, lo, a.K, el_a, el_t, !first, has_ts, redk, m_a, m_tl, [&](int r, float va, int ia, float vt, int it) {
        out->a_val[r] = va;
        out->a_id[r] = ia;
        out->ts_val[r] = vt;
        out->ts_id[r] = it;
    });
    // the sets' sums, each against its own maximum (one exp where they coincide)
    double s_all = 0.0, s_a = 0.0, s_ts = 0.0, s_tl = 0.0;
    const bool do_a = !first && m_a > -INFINITY, do_ts = has_ts && m_ts > -INFINITY;
    const bool do_tl = do_ts && first && m_tl > -INFINITY;
    if (m_all > -INFINITY) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = lo + tid + 256 * u;
            if (i >= hi) continue;
            const double l = (double)v[u], e = exp(l - (double)m_all);
            s_all += e;
            if (do_a && i != ta.sot && i != ta.solm && i != ta.not_) s_a += m_a == m_all ? e : exp(l - (double)m_a);
            if (do_ts && i >= ta.beg) {
                const double et = m_ts == m_all ? e : exp(l - (double)m_ts);
                s_ts += et;
                if (do_tl && i > ta.beg) s_tl += m_tl == m_ts ? et : exp(l - (double)m_tl);
            }
        }
    }
    s_all = wave_sum(s_all);
    s_a = wave_sum(s_a);
    if (has_ts) { s_ts = wave_sum(s_ts); s_tl = wave_sum(s_tl); }
    if (lane == 0) { redd[0][w] = s_all; redd[1][w] = s_a; redd[2][w] = s_ts; redd[3][w] = s_tl; }
    __syncthreads();
    if (tid == 0) {
        out->m_all = m_all;
        out->m_tx = m_tx;
        out->m_ts = m_ts;
        out->id_ts = k_ts ? pick_key_id(k_ts) : -1;
        out->pad = 0;
        out->sum_all = ((redd[0][0] + redd[0][1]) + redd[0][2]) + redd[0][3];
        out->sum_a = ((redd[1][0] + redd[1][1]) + redd[1][2]) + redd[1][3];
        out->sum_ts = ((redd[2][0] + redd[2][1]) + redd[2][2]) + redd[2][3];
        // (after the first token the timestamp list's set is ids >= beg itself)
        out->m_tl = first ? m_tl : m_ts;
        out->sum_tl = first ? ((redd[3][0] + redd[3][1]) + redd[3][2]) + redd[3][3] : out->sum_ts;
    }
}

// One workgroup: per active row the unmasked softmax quantities (Z, sum_ts,
// p_tx, id_ts) and with them the row's allowed set; the log-sum-exp and the
// merged top-(K+1) of that set (beam_row_merge); then k_beam_select's ranking,
// walk and KV history re-pointing (beam_select_tail), with a TsRec per new slot
// and per finished hypothesis (under the unmasked softmax of the row that
// produced the token).
__global__ __launch_bounds__(256) void k_tsbeam_select(TsBeamArgs ta) {
    const BeamArgs &a = ta.b;
    BeamState *bs = a.bs;
    const int pos = a.st->pos;
    if (pos < a.feed_len || bs->done) return;
    const int t = pos - a.feed_len, TK = a.K + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    struct Lds : BeamSelLds {  // (one block: apart, each array is padded to 16 bytes)
        double row_m[BEAM_MAX], row_z[BEAM_MAX];
        float row_pt[BEAM_MAX], row_ptsum[BEAM_MAX];
        int row_tid[BEAM_MAX];
    };
    __shared__ Lds sl;
    const int na_old = bs->n_active;
    auto record = [&](int c) {  // candidate c as sampled from its row
        const int p = c / TK;
        TsRec r;
        r.id = sl.cid[c];
        r.tid = sl.row_tid[p];
        r.p = (float)(exp((double)sl.cval[c] - sl.row_m[p]) / sl.row_z[p]);
        r.pt = sl.row_pt[p];
        r.ptsum = sl.row_ptsum[p];
        r.pad = 0;
        return r;
    };
    // 1. per active row: the timestamp rule, the set's log-sum-exp and top-(K+1)
    for (int b = w; b < na_old; b += 4) {
        const TsBeamPart *pp = ta.tparts + (int64_t)b * BEAM_NS;
        const bool in = lane < BEAM_NS;
        const float pm = in ? pp[lane].m_all : -INFINITY;
        const float M = wave_max(pm);
        const double Z = wave_sum(pm > -INFINITY ? pp[lane].sum_all * exp((double)pm - (double)M) : 0.0);
        const float pts = in ? pp[lane].m_ts : -INFINITY;
        const float Mts = wave_max(pts);
        const double TS = wave_sum(pts > -INFINITY ? pp[lane].sum_ts * exp((double)pts - (double)Mts) : 0.0);
        const float Mtx = wave_max(in ? pp[lane].m_tx : -INFINITY);
        const unsigned long long kts =
            wave_max_u64(in && pp[lane].id_ts >= 0 ? pick_key(pts, pp[lane].id_ts) : 0ull);
        const double p_maxts = exp((double)Mts - (double)M) / Z;
        const double sum_ts = TS * p_maxts;
        const double p_tx = Mtx > -INFINITY ? exp((double)Mtx - (double)M) / Z : 0.0;
        const bool ts_set = t == 0 || sum_ts > p_tx;  // (the same on every lane)
        const float sm = !in ? -INFINITY : ts_set ? pp[lane].m_tl : pp[lane].a_val[0];
        const double ss = !in ? 0.0 : ts_set ? pp[lane].sum_tl : pp[lane].sum_a;
        const float SM = wave_max(sm);
        const double SS = wave_sum(sm > -INFINITY ? ss * exp((double)sm - (double)SM) : 0.0);
        if (lane == 0) {
            sl.lse[b] = (double)SM + log(SS);
            sl.row_m[b] = (double)M;
            sl.row_z[b] = Z;
            sl.row_tid[b] = kts ? pick_key_id(kts) : -1;
            sl.row_pt[b] = (float)(p_maxts / (sum_ts + 1e-10));
            sl.row_ptsum[b] = (float)sum_ts;
        }
        beam_row_merge(TK, [&](int sp, int r, float &val, int &id) {
            const TsBeamPart &q = pp[sp];
            id = ts_set ? q.ts_id[r] : q.a_id[r];
            val = ts_set ? q.ts_val[r] : q.a_val[r];
        }, sl.cval + b * TK, sl.cid + b * TK);
    }
    // 2 - 4, with the records
    beam_select_tail(a, sl, pos, na_old, [&](int nf, int c) { ta.fin_rec[nf] = record(c); },
                     [&](int s, int, int c) { ta.hist_rec[t * BEAM_MAX + s] = record(c); });
}

hipError_t launch_tsbeam_step(hipStream_t s, const TsBeamArgs &a) {
    if (a.b.K < 1 || a.b.K > BEAM_MAX || a.b.tctx > 512 || (a.b.V + BEAM_NS - 1) / BEAM_NS > 4096 || a.beg < 1 ||
        a.b.V < a.beg + 2 || !a.tparts || !a.hist_rec || !a.fin_rec)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tsbeam_part, dim3(BEAM_NS, a.b.K), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tsbeam_select, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
