// wmi_tsbeam.hip — the beam-search step under the timestamp rule
// (wmi_decode_timestamps_beam, wmi_transcribe with wmi_set_beam_size > 1).
//
// A translation unit of its own: its code object is loaded with the first
// timestamped beam window, so a process that never asks for one runs on
// exactly the code objects it ran on before these kernels existed (the
// greedy, beam and timestamp paths of wmi_kernels.hip are byte for byte what
// they were).  The ordering helpers restate wmi_kernels.hip's beam_key and
// cand_before.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

namespace wmi {

// (value desc, id asc) as one unsigned key: larger key = earlier in the order
__device__ __forceinline__ unsigned long long beam_key(float v, int id) {
    return ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
}

// candidate i before candidate j in the ranking (score desc, beam asc, rank asc)
__device__ __forceinline__ bool cand_before(double si, int bi, int ri, double sj, int bj, int rj) {
    if (si != sj) return si > sj;
    if (bi != bj) return bi < bj;
    return ri < rj;
}

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
    constexpr int U = 16;  // split length <= 4096
    const int chunk = (a.V + BEAM_NS - 1) / BEAM_NS, lo = sp * chunk, hi = min(a.V, lo + chunk);
    const bool has_ts = hi > ta.beg;  // (uniform over the workgroup)
    const float *row = a.logits + (int64_t)b * a.V;
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = lo + tid + 256 * u;
        v[u] = row[i < hi ? i : 0];
    }
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
        else k_ts = u64max(k_ts, beam_key(v[u], i));
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
    const float m_ts = k_ts ? unord_f32((uint32_t)(k_ts >> 32)) : -INFINITY;
    __syncthreads();
    // the two top-(K+1) lists, one workgroup-wide argmax per rank and list
    TsBeamPart *out = ta.tparts + (int64_t)b * BEAM_NS + sp;
    float m_a = -INFINITY, m_tl = -INFINITY;
    for (int r = 0; r <= a.K; ++r) {
        unsigned long long ba = 0, bt = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned long long k = beam_key(v[u], lo + tid + 256 * u);
            if ((el_a >> u) & 1u) ba = u64max(ba, k);
            if ((el_t >> u) & 1u) bt = u64max(bt, k);
        }
        if (!first) ba = wave_max_u64(ba);
        if (has_ts) bt = wave_max_u64(bt);
        if (lane == 0) { redk[0][w] = ba; redk[1][w] = bt; }
        __syncthreads();
        ba = u64max(u64max(redk[0][0], redk[0][1]), u64max(redk[0][2], redk[0][3]));
        bt = u64max(u64max(redk[1][0], redk[1][1]), u64max(redk[1][2], redk[1][3]));
        const int ia = (int)(0xffffffffu - (uint32_t)(ba & 0xffffffffull)), ra = ia - lo;
        const int it = (int)(0xffffffffu - (uint32_t)(bt & 0xffffffffull)), rt = it - lo;
        if (ba && (ra & 255) == tid) el_a &= ~(1u << (ra >> 8));
        if (bt && (rt & 255) == tid) el_t &= ~(1u << (rt >> 8));
        const float va = ba ? unord_f32((uint32_t)(ba >> 32)) : -INFINITY;
        const float vt = bt ? unord_f32((uint32_t)(bt >> 32)) : -INFINITY;
        if (r == 0) { m_a = va; m_tl = vt; }
        if (tid == 0) {
            out->a_val[r] = va;
            out->a_id[r] = ba ? ia : -1;
            out->ts_val[r] = vt;
            out->ts_id[r] = bt ? it : -1;
        }
        __syncthreads();
    }
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
        out->id_ts = k_ts ? (int)(0xffffffffu - (uint32_t)(k_ts & 0xffffffffull)) : -1;
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
// merged top-(K+1) of that set; then k_beam_select's ranking, walk and KV
// history re-pointing, plus a TsRec per new slot and per finished hypothesis
// (under the unmasked softmax of the row that produced the token).
__global__ __launch_bounds__(256) void k_tsbeam_select(TsBeamArgs ta) {
    const BeamArgs &a = ta.b;
    BeamState *bs = a.bs;
    const int pos = a.st->pos;
    if (pos < a.feed_len || bs->done) return;
    const int t = pos - a.feed_len, K = a.K, TK = K + 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NC = BEAM_MAX * BEAM_TK;
    __shared__ double lse[BEAM_MAX], row_m[BEAM_MAX], row_z[BEAM_MAX];
    __shared__ float row_pt[BEAM_MAX], row_ptsum[BEAM_MAX];
    __shared__ int row_tid[BEAM_MAX];
    __shared__ float cval[NC];
    __shared__ int cid[NC];
    __shared__ double cscore[NC];
    __shared__ int order[NC];
    __shared__ int sel_parent[BEAM_MAX], sel_cand[BEAM_MAX], n_new_s;
    __shared__ int32_t src_old[BEAM_MAX][512];
    const int na_old = bs->n_active;
    auto record = [&](int c) {  // candidate c as sampled from its row
        const int p = c / TK;
        TsRec r;
        r.id = cid[c];
        r.tid = row_tid[p];
        r.p = (float)(exp((double)cval[c] - row_m[p]) / row_z[p]);
        r.pt = row_pt[p];
        r.ptsum = row_ptsum[p];
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
            wave_max_u64(in && pp[lane].id_ts >= 0 ? beam_key(pts, pp[lane].id_ts) : 0ull);
        const double p_maxts = exp((double)Mts - (double)M) / Z;
        const double sum_ts = TS * p_maxts;
        const double p_tx = Mtx > -INFINITY ? exp((double)Mtx - (double)M) / Z : 0.0;
        const bool ts_set = t == 0 || sum_ts > p_tx;  // (the same on every lane)
        const float sm = !in ? -INFINITY : ts_set ? pp[lane].m_tl : pp[lane].a_val[0];
        const double ss = !in ? 0.0 : ts_set ? pp[lane].sum_tl : pp[lane].sum_a;
        const float SM = wave_max(sm);
        const double SS = wave_sum(sm > -INFINITY ? ss * exp((double)sm - (double)SM) : 0.0);
        if (lane == 0) {
            lse[b] = (double)SM + log(SS);
            row_m[b] = (double)M;
            row_z[b] = Z;
            row_tid[b] = kts ? (int)(0xffffffffu - (uint32_t)(kts & 0xffffffffull)) : -1;
            row_pt[b] = (float)(p_maxts / (sum_ts + 1e-10));
            row_ptsum[b] = (float)sum_ts;
        }
        unsigned long long key[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = lane + 64 * k;
            key[k] = 0ull;
            if (c < BEAM_NS * TK) {
                const TsBeamPart &q = pp[c / TK];
                const int id = ts_set ? q.ts_id[c % TK] : q.a_id[c % TK];
                if (id >= 0) key[k] = beam_key(ts_set ? q.ts_val[c % TK] : q.a_val[c % TK], id);
            }
        }
        for (int r = 0; r < TK; ++r) {
            unsigned long long best = key[0] > key[1] ? key[0] : key[1];
            best = key[2] > best ? key[2] : best;
            best = wave_max_u64(best);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (key[k] == best) key[k] = 0ull;
            if (lane == 0) {  // (a set with fewer than K + 1 ids: no candidate, ranked last)
                cval[b * TK + r] = best ? unord_f32((uint32_t)(best >> 32)) : -INFINITY;
                cid[b * TK + r] = best ? (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : -1;
            }
        }
    }
    __syncthreads();
    // 2. scores and ranking
    const int nc = na_old * TK;
    if (tid < nc) cscore[tid] = cid[tid] >= 0 ? bs->score[tid / TK] + ((double)cval[tid] - lse[tid / TK]) : -INFINITY;
    __syncthreads();
    if (tid < nc) {
        int rank = 0;
        const double si = cscore[tid];
        const int bi = tid / TK, ri = tid % TK;
        for (int j = 0; j < nc; ++j)
            if (cand_before(cscore[j], j / TK, j % TK, si, bi, ri)) ++rank;
        order[rank] = tid;
    }
    // history table of the parents, positions < pos - 1
    for (int i = tid; i < na_old * (pos - 1); i += 256) {
        const int r = i / (pos - 1), j = i - r * (pos - 1);
        src_old[r][j] = a.kv_src[r * a.tctx + j];
    }
    __syncthreads();
    // 3. walk the ranking
    if (tid == 0) {
        int na = 0, nf = bs->n_fin;
        for (int k = 0; k < nc && na < K; ++k) {
            const int c = order[k];
            if (cid[c] < 0) continue;
            if (cid[c] == a.eot) {
                if (nf < K) {
                    bs->fin_t[nf] = t;
                    bs->fin_beam[nf] = c / TK;
                    bs->fin_score[nf] = cscore[c];
                    ta.fin_rec[nf] = record(c);
                    ++nf;
                }
                continue;
            }
            sel_parent[na] = c / TK;
            sel_cand[na] = c;
            ++na;
        }
        n_new_s = na;
        bs->n_fin = nf;
        bs->n_active = na;
        bs->n_steps = t + 1;
        if (nf >= K || t + 1 >= a.max_tokens) bs->done = 1;
    }
    __syncthreads();
    // 4. next hypotheses: scores, fed tokens, back-pointers, records, KV history table
    const int nn = n_new_s;
    if (tid < nn) {
        const int c = sel_cand[tid];
        bs->score[tid] = cscore[c];
        bs->tok[tid] = cid[c];
        a.hist_parent[t * BEAM_MAX + tid] = sel_parent[tid];
        a.hist_tok[t * BEAM_MAX + tid] = cid[c];
        ta.hist_rec[t * BEAM_MAX + tid] = record(c);
    }
    for (int i = tid; i < nn * pos; i += 256) {
        const int sl = i / pos, j = i - sl * pos, p = sel_parent[sl];
        a.kv_src[sl * a.tctx + j] = j < pos - 1 ? src_old[p][j] : p;
    }
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
