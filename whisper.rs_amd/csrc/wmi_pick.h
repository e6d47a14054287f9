// wmi_pick.h — the one copy of the device code that the pick kernels share:
// the timestamp samplers (k_ts_sample in wmi_kernels.hip, k_ts_sample_t in
// wmi_sample.hip, k_ts_sample_r in wmi_rules.hip) and the beam steps
// (wmi_tsbeam.hip, wmi_rbeam.hip; k_beam_topk / k_beam_select in
// wmi_kernels.hip take the keys and cand_before only).  Device-only and all
// inline: every unit keeps its kernels, its launch functions and its code
// object (DESIGN.md "Shared pick code").
// What differs between the kernels comes in as a functor; nothing here asks
// which kernel it runs in.
#pragma once
#include "wmi_device.h"
#include "wmi_internal.h"

namespace wmi {

// ---- keys -------------------------------------------------------------------
// (value desc, id asc) as one unsigned key: larger key = earlier in the order;
// 0 is no key (ids stay below 2^32 - 1)
__device__ __forceinline__ unsigned long long pick_key(float v, int id) {
    return ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
}
__device__ __forceinline__ int pick_key_id(unsigned long long k) { return (int)(0xffffffffu - (uint32_t)(k & 0xffffffffull)); }
__device__ __forceinline__ float pick_key_val(unsigned long long k) { return unord_f32((uint32_t)(k >> 32)); }

// candidate i before candidate j in the ranking (score desc, beam asc, rank asc)
__device__ __forceinline__ bool cand_before(double si, int bi, int ri, double sj, int bj, int rj) {
    if (si != sj) return si > sj;
    if (bi != bj) return bi < bj;
    return ri < rj;
}

// splitmix64 (the stream of a row's draws: u_t from sm64(key + t))
__device__ __forceinline__ unsigned long long sm64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- samplers: one workgroup of 1024 threads per decoder row ------------------
// The prologue.  False: nothing to sample (the prompt is still being fed, or
// the row has sampled EOT and feeds EOT); else t is the generated token's index.
__device__ __forceinline__ bool samp_begin(const TsArgs &a, int &t) {
    const int pos = a.st->pos;
    if (pos < a.feed_len) return false;  // still feeding the prompt
    t = pos - a.feed_len;
    if (a.done[blockIdx.x]) {  // (uniform over the workgroup; set by a previous launch)
        if (threadIdx.x == 0) a.tok_out[blockIdx.x] = a.eot;
        return false;
    }
    return true;
}

// the row's pick: fed at the next step; EOT ends the row
__device__ __forceinline__ void samp_feed(const TsArgs &a, int id) {
    a.tok_out[blockIdx.x] = id;
    if (id == a.eot) a.done[blockIdx.x] = 1;
}

// Row statistics of the unmasked softmax (k_ts_sample, k_ts_sample_t).
struct RowLds {
    float smax[16];
    double ssum[16], sts[16];
    unsigned long long sk[4][16];
};
struct RowStats {
    float mx;                                 // (row_reduce) row maximum
    // (row_probs) argmax keys over all ids but sot / solm / not, over ids >= beg, > beg, < beg;
    // sum exp(l - mx); P(ids >= beg), P(k_ts's id), P(k_tx's id)
    unsigned long long k_all, k_ts, k_ts1, k_tx;
    double Z, sum_ts, p_maxts, p_maxtx;
    int id_ts;
};

// passes 1 and 2: the maximum, the four keys (left per wave in LDS), then the
// sums of exp(l - mx) over the row and over ids >= beg, per wave in LDS too
// (ends on a barrier)
__device__ __forceinline__ void row_reduce(const TsArgs &a, const float *lg, RowLds &s, RowStats &r) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float mx = -INFINITY;
    unsigned long long k_all = 0, k_ts = 0, k_ts1 = 0, k_tx = 0;
    for (int i = tid; i < a.V; i += 1024) {
        const float l = lg[i];
        mx = fmaxf(mx, l);
        const unsigned long long k = pick_key(l, i);
        if (i >= a.beg) k_ts = k > k_ts ? k : k_ts;
        else k_tx = k > k_tx ? k : k_tx;
        if (i > a.beg) k_ts1 = k > k_ts1 ? k : k_ts1;
        if (i != a.sot && i != a.solm && i != a.not_) k_all = k > k_all ? k : k_all;
    }
    mx = wave_max(mx);
    k_all = wave_max_u64(k_all);
    k_ts = wave_max_u64(k_ts);
    k_ts1 = wave_max_u64(k_ts1);
    k_tx = wave_max_u64(k_tx);
    if (lane == 0) { s.smax[w] = mx; s.sk[0][w] = k_all; s.sk[1][w] = k_ts; s.sk[2][w] = k_ts1; s.sk[3][w] = k_tx; }
    __syncthreads();
    mx = s.smax[0];
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s.smax[i]);
    double sum = 0.0, st = 0.0;
    for (int i = tid; i < a.V; i += 1024) {
        const double e = exp((double)lg[i] - (double)mx);
        sum += e;
        if (i >= a.beg) st += e;
    }
    sum = wave_sum(sum);
    st = wave_sum(st);
    if (lane == 0) { s.ssum[w] = sum; s.sts[w] = st; }
    __syncthreads();
    r.mx = mx;
}

// the waves' keys and sums merged, and the probabilities the timestamp rule
// compares (the keys wait in LDS over pass 2: held in registers through its
// exp they push a 1024-thread workgroup past its 128 registers)
__device__ __forceinline__ void row_probs(const float *lg, const RowLds &s, RowStats &r) {
    unsigned long long k_all = s.sk[0][0], k_ts = s.sk[1][0], k_ts1 = s.sk[2][0], k_tx = s.sk[3][0];
    for (int i = 1; i < 16; ++i) {
        k_all = s.sk[0][i] > k_all ? s.sk[0][i] : k_all;
        k_ts = s.sk[1][i] > k_ts ? s.sk[1][i] : k_ts;
        k_ts1 = s.sk[2][i] > k_ts1 ? s.sk[2][i] : k_ts1;
        k_tx = s.sk[3][i] > k_tx ? s.sk[3][i] : k_tx;
    }
    r.k_all = k_all; r.k_ts = k_ts; r.k_ts1 = k_ts1; r.k_tx = k_tx;
    double Z = 0.0, TS = 0.0;
    for (int i = 0; i < 16; ++i) { Z += s.ssum[i]; TS += s.sts[i]; }
    r.id_ts = pick_key_id(r.k_ts);
    const int id_tx = pick_key_id(r.k_tx);
    r.p_maxts = exp((double)lg[r.id_ts] - (double)r.mx) / Z;
    r.p_maxtx = exp((double)lg[id_tx] - (double)r.mx) / Z;
    r.sum_ts = TS / Z;
    r.Z = Z;
}

// record t of the row: {id, tid = argmax over ids >= beg, p, pt = max_ts / (sum_ts + 1e-10), ptsum}
__device__ __forceinline__ void row_record(const TsArgs &a, const float *lg, const RowStats &r, int t, int id) {
    TsRec rec;
    rec.id = id;
    rec.tid = r.id_ts;
    rec.p = (float)(exp((double)lg[id] - (double)r.mx) / r.Z);
    rec.pt = (float)(r.p_maxts / (r.sum_ts + 1e-10));
    rec.ptsum = (float)r.sum_ts;
    rec.pad = 0;
    a.rec[(size_t)blockIdx.x * a.max_rec + t] = rec;
}

// The draw from an allowed set A with maximum m_a at temperature T
// (k_ts_sample_t, k_ts_sample_r).  tsum is cleared by its caller, slot
// threadIdx.x each, ahead of any barrier that precedes tile_sums.
struct DrawLds {
    double sse[16], tsum[1024], gsum[64], wl[64], c_tile;
    int j_tile;
};
__device__ __forceinline__ double draw_weight(float l, float m_a, float T) {
    return exp(((double)l - (double)m_a) / (double)T);
}

// pass 3, over A in tiles of 64 consecutive ids, one wave per tile: the waves'
// sums of exp(l - m_a) (for plog) and, for T > 0, each tile's sum of weights
// (ends on a barrier)
template <class InA>
__device__ __forceinline__ void tile_sums(DrawLds &d, const float *lg, int V, InA in_a, float m_a, float T) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nt = (V + 63) >> 6;
    double se = 0.0;
    // (one exp per loop: both in one body spill past the 128 registers of a 1024-thread workgroup)
    for (int j = w; j < nt; j += 16) {
        const int i = j * 64 + lane;
        if (i < V && in_a(i)) se += exp((double)lg[i] - (double)m_a);
    }
    if (T > 0.0f)
        for (int j = w; j < nt; j += 16) {
            const int i = j * 64 + lane;
            const bool in = i < V && in_a(i);
            const double wt = wave_sum(in ? draw_weight(lg[i], m_a, T) : 0.0);
            if (lane == 0) d.tsum[j] = wt;
        }
    se = wave_sum(se);
    if (lane == 0) d.sse[w] = se;
    __syncthreads();
}

// The tile of the draw u Q, u from the row's stream key: 64 groups of 16
// tiles, then the tile inside the group, each a running sum in ascending id
// order (all in double); thread 0 leaves the tile (-1: none) and the running
// sum ahead of it in LDS and returns the target u Q.  Where rounding leaves no
// group past the target, no_group(J, c) decides both.  One barrier.
template <class NoGroup>
__device__ __forceinline__ double draw_tile(DrawLds &d, unsigned long long key, NoGroup no_group) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        double g = 0.0;
        for (int k = 0; k < 16; ++k) g += d.tsum[16 * tid + k];
        d.gsum[tid] = g;
    }
    __syncthreads();
    double target = 0.0;
    if (tid == 0) {
        double Q = 0.0;
        #pragma unroll 1
        for (int g = 0; g < 64; ++g) Q += d.gsum[g];
        const double u = (double)(sm64(key) >> 11) * 0x1.0p-53;
        target = u * Q;
        double c = 0.0;
        int G = -1;
        #pragma unroll 1
        for (int g = 0; g < 64; ++g) {
            if (c + d.gsum[g] > target) { G = g; break; }
            c += d.gsum[g];
        }
        int J = -1;
        double cj = c;
        if (G >= 0) {
            // (rounding may leave no tile of the group past the target: its last tile with any weight)
            #pragma unroll 1
            for (int k = 0; k < 16; ++k) {
                const int j = 16 * G + k;
                if (d.tsum[j] > 0.0) { J = j; cj = c; }
                if (c + d.tsum[j] > target) break;
                c += d.tsum[j];
            }
        } else {
            no_group(J, cj);
        }
        d.j_tile = J;
        d.c_tile = cj;
    }
    return target;
}

// The id inside the tile that draw_tile left (two barriers): the last id with
// any weight up to the one whose running sum passes the target; none_id where
// there is no tile.  Thread 0's result.
template <class InA>
__device__ __forceinline__ int draw_id(DrawLds &d, double target, const float *lg, int V, InA in_a, float m_a, float T,
                                       int none_id) {
    const int tid = threadIdx.x;
    __syncthreads();
    const int J = d.j_tile;  // (uniform)
    if (J >= 0 && tid < 64) {
        const int i = J * 64 + tid;
        d.wl[tid] = i < V && in_a(i) ? draw_weight(lg[i], m_a, T) : 0.0;
    }
    __syncthreads();
    int id = none_id;
    if (tid == 0 && J >= 0) {
        double c = d.c_tile;
        #pragma unroll 1
        for (int k = 0; k < 64; ++k) {
            if (d.wl[k] > 0.0) id = J * 64 + k;
            if (c + d.wl[k] > target) break;
            c += d.wl[k];
        }
    }
    return id;
}

// log-probability of id under the unscaled distribution over A
__device__ __forceinline__ float draw_plog(const DrawLds &d, float l, float m_a) {
    double SE = 0.0;
    for (int i = 0; i < 16; ++i) SE += d.sse[i];
    return (float)((double)l - ((double)m_a + log(SE)));
}

// ---- beam step: the split kernels (256 threads, 16 logits a thread) ---------
constexpr int SPLIT_U = 16;  // split length <= 4096

__device__ __forceinline__ void split_load(float (&v)[SPLIT_U], const float *row, int lo, int hi) {
#pragma unroll
    for (int u = 0; u < SPLIT_U; ++u) {
        const int i = lo + threadIdx.x + 256 * u;
        v[u] = row[i < hi ? i : 0];
    }
}

// The two top-(K+1) lists of a split, one workgroup-wide argmax per rank and
// list: el_a / el_t hold a bit per logit of this thread that is eligible for
// the list.  red_a / red_t (uniform): whether the list's wave reduction runs
// at all (a list known to be empty skips it).  out(r, va, ia, vt, it) on
// thread 0 (id -1, value -inf: no such rank); m_a / m_t are the rank-0 values.
template <class Out>
__device__ __forceinline__ void split_rounds(const float (&v)[SPLIT_U], int lo, int K, uint32_t el_a, uint32_t el_t, bool red_a,
                                             bool red_t, unsigned long long (&redk)[2][4], float &m_a, float &m_t, Out out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    m_a = m_t = -INFINITY;
    for (int r = 0; r <= K; ++r) {
        unsigned long long ba = 0, bt = 0;
#pragma unroll
        for (int u = 0; u < SPLIT_U; ++u) {
            const unsigned long long k = pick_key(v[u], lo + tid + 256 * u);
            if ((el_a >> u) & 1u) ba = u64max(ba, k);
            if ((el_t >> u) & 1u) bt = u64max(bt, k);
        }
        if (red_a) ba = wave_max_u64(ba);
        if (red_t) bt = wave_max_u64(bt);
        if (lane == 0) { redk[0][w] = ba; redk[1][w] = bt; }
        __syncthreads();
        ba = u64max(u64max(redk[0][0], redk[0][1]), u64max(redk[0][2], redk[0][3]));
        bt = u64max(u64max(redk[1][0], redk[1][1]), u64max(redk[1][2], redk[1][3]));
        const int ia = pick_key_id(ba), qa = ia - lo;
        const int it = pick_key_id(bt), qt = it - lo;
        if (ba && (qa & 255) == tid) el_a &= ~(1u << (qa >> 8));
        if (bt && (qt & 255) == tid) el_t &= ~(1u << (qt >> 8));
        const float va = ba ? pick_key_val(ba) : -INFINITY;
        const float vt = bt ? pick_key_val(bt) : -INFINITY;
        if (r == 0) { m_a = va; m_t = vt; }
        if (tid == 0) out(r, va, ba ? ia : -1, vt, bt ? it : -1);
        __syncthreads();
    }
}

// ---- beam step: the select kernels (one workgroup of 256 threads) -----------
constexpr int BEAM_NC = BEAM_MAX * BEAM_TK;
struct BeamSelLds {
    double lse[BEAM_MAX];                 // the log-sum-exp of each row's set (its kernel's step 1)
    float cval[BEAM_NC];                  // candidate b * TK + r: rank r of row b (id -1, value -inf: none)
    int cid[BEAM_NC];
    double cscore[BEAM_NC];
    int order[BEAM_NC];
    int sel_parent[BEAM_MAX], sel_cand[BEAM_MAX], n_new;
    int32_t src_old[BEAM_MAX][512];
};

// One wave merges a row's 16 splits x (K+1) entries into the row's top-(K+1):
// fetch(split, rank, value, id) with id < 0 for no entry.
template <class Fetch>
__device__ __forceinline__ void beam_row_merge(int TK, Fetch fetch, float *cval, int *cid) {
    const int lane = threadIdx.x & 63;
    unsigned long long key[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = lane + 64 * k;
        key[k] = 0ull;
        if (c < BEAM_NS * TK) {
            float val;
            int id;
            fetch(c / TK, c % TK, val, id);
            if (id >= 0) key[k] = pick_key(val, id);
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
            cval[r] = best ? pick_key_val(best) : -INFINITY;
            cid[r] = best ? pick_key_id(best) : -1;
        }
    }
}

// Steps 2 - 4 of a select kernel, after its step 1 has filled lse, cval and
// cid of the na_old active rows: rank the candidates, walk the ranking into
// finished hypotheses and the next slots, update the BeamState and the
// back-pointers, re-point the KV history table.  Opens with a barrier and
// holds three more.  fin(nf, c) on thread 0: hypothesis nf finished with
// candidate c; slot(s, p, c) on thread s after the last barrier: slot s
// continues from parent p with candidate c.  Returns the number of new slots.
template <class Fin, class Slot>
__device__ __forceinline__ int beam_select_tail(const BeamArgs &a, BeamSelLds &s, int pos, int na_old, Fin fin, Slot slot) {
    BeamState *bs = a.bs;
    const int t = pos - a.feed_len, K = a.K, TK = K + 1, tid = threadIdx.x;
    __syncthreads();
    // 2. scores and ranking
    const int nc = na_old * TK;
    if (tid < nc) s.cscore[tid] = s.cid[tid] >= 0 ? bs->score[tid / TK] + ((double)s.cval[tid] - s.lse[tid / TK]) : -INFINITY;
    __syncthreads();
    if (tid < nc) {
        int rank = 0;
        const double si = s.cscore[tid];
        const int bi = tid / TK, ri = tid % TK;
        for (int j = 0; j < nc; ++j)
            if (cand_before(s.cscore[j], j / TK, j % TK, si, bi, ri)) ++rank;
        s.order[rank] = tid;
    }
    // history table of the parents, positions < pos - 1
    for (int i = tid; i < na_old * (pos - 1); i += 256) {
        const int r = i / (pos - 1), j = i - r * (pos - 1);
        s.src_old[r][j] = a.kv_src[r * a.tctx + j];
    }
    __syncthreads();
    // 3. walk the ranking
    if (tid == 0) {
        int na = 0, nf = bs->n_fin;
        for (int k = 0; k < nc && na < K; ++k) {
            const int c = s.order[k];
            if (s.cid[c] < 0) continue;
            if (s.cid[c] == a.eot) {
                if (nf < K) {
                    bs->fin_t[nf] = t;
                    bs->fin_beam[nf] = c / TK;
                    bs->fin_score[nf] = s.cscore[c];
                    fin(nf, c);
                    ++nf;
                }
                continue;
            }
            s.sel_parent[na] = c / TK;
            s.sel_cand[na] = c;
            ++na;
        }
        s.n_new = na;
        bs->n_fin = nf;
        bs->n_active = na;
        bs->n_steps = t + 1;
        if (nf >= K || t + 1 >= a.max_tokens) bs->done = 1;
    }
    __syncthreads();
    // 4. next hypotheses: scores, fed tokens, back-pointers, KV history table
    const int nn = s.n_new;
    if (tid < nn) {
        const int c = s.sel_cand[tid];
        bs->score[tid] = s.cscore[c];
        bs->tok[tid] = s.cid[c];
        a.hist_parent[t * BEAM_MAX + tid] = s.sel_parent[tid];
        a.hist_tok[t * BEAM_MAX + tid] = s.cid[c];
        slot(tid, s.sel_parent[tid], c);
    }
    for (int i = tid; i < nn * pos; i += 256) {
        const int sl = i / pos, j = i - sl * pos, p = s.sel_parent[sl];
        a.kv_src[sl * a.tctx + j] = j < pos - 1 ? s.src_old[p][j] : p;
    }
    return nn;
}

}  // namespace wmi
