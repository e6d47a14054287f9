// wmi_sample.hip — the temperature sampler of the timestamped decoder and the
// no-speech probability of a beam window (wmi_set_fallback,
// wmi_decode_timestamps_sampled; DESIGN.md "Temperature fallback").
//
// A translation unit of its own, as wmi_tsbeam.hip: its code object is loaded
// with the first sampled window, so a context whose fallback parameters are
// the defaults runs on exactly the code objects it ran on before these kernels
// existed.  The key helpers restate wmi_kernels.hip's ts_key / ts_key_id.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

namespace wmi {

__device__ __forceinline__ unsigned long long ts_key(float v, int id) {
    return ((unsigned long long)ord_f32(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
}
__device__ __forceinline__ int ts_key_id(unsigned long long k) { return (int)(0xffffffffu - (uint32_t)(k & 0xffffffffu)); }

// splitmix64 (the stream of a row's draws: u_t from sm64(key + t))
__device__ __forceinline__ unsigned long long sm64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One workgroup per decoder row b, k_ts_sample's conventions (done words,
// tok_out, records).  Passes 1 and 2 are k_ts_sample's, operation for
// operation, so the record {id, tid, p, pt, ptsum} of a T = 0 row is bitwise
// what k_ts_sample writes.  The allowed set A (the timestamp rule) is known
// after pass 2; its maximum is the value in the set's argmax key.  Pass 3 goes
// over A in tiles of 64 consecutive ids, one wave per tile: the sum of
// exp(l - m_A) for plog, and for T > 0 each tile's sum of the weights
// w = exp((l - m_A) / T).  The draw u Q is then located by wave 0: 64 groups
// of 16 tiles, the tile inside the group, the id inside the tile, each a
// running sum in ascending id order (all in double).
__global__ __launch_bounds__(1024) void k_ts_sample_t(TsSampArgs sa) {
    const TsArgs &a = sa.t;
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
    __shared__ float smax[16];
    __shared__ double ssum[16], sts[16], sse[16];
    __shared__ unsigned long long sk[3][16], stx[16];
    __shared__ double tsum[1024], gsum[64], wl[64], c_tile;
    __shared__ int j_tile;
    float mx = -INFINITY;
    unsigned long long k_all = 0, k_ts = 0, k_ts1 = 0, k_tx = 0;
    for (int i = tid; i < a.V; i += 1024) {
        const float l = lg[i];
        mx = fmaxf(mx, l);
        const unsigned long long k = ts_key(l, i);
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
    if (lane == 0) { smax[w] = mx; sk[0][w] = k_all; sk[1][w] = k_ts; sk[2][w] = k_ts1; stx[w] = k_tx; }
    tsum[tid] = 0.0;
    __syncthreads();
    mx = smax[0];
    k_all = sk[0][0]; k_ts = sk[1][0]; k_ts1 = sk[2][0]; k_tx = stx[0];
    for (int i = 1; i < 16; ++i) {
        mx = fmaxf(mx, smax[i]);
        k_all = sk[0][i] > k_all ? sk[0][i] : k_all;
        k_ts = sk[1][i] > k_ts ? sk[1][i] : k_ts;
        k_ts1 = sk[2][i] > k_ts1 ? sk[2][i] : k_ts1;
        k_tx = stx[i] > k_tx ? stx[i] : k_tx;
    }
    double s = 0.0, st = 0.0;
    for (int i = tid; i < a.V; i += 1024) {
        const double e = exp((double)lg[i] - (double)mx);
        s += e;
        if (i >= a.beg) st += e;
    }
    s = wave_sum(s);
    st = wave_sum(st);
    if (lane == 0) { ssum[w] = s; sts[w] = st; }
    __syncthreads();
    double Z = 0.0, TS = 0.0;
    for (int i = 0; i < 16; ++i) { Z += ssum[i]; TS += sts[i]; }
    const int id_ts = ts_key_id(k_ts), id_tx = ts_key_id(k_tx);
    const double p_maxts = exp((double)lg[id_ts] - (double)mx) / Z;
    const double p_maxtx = exp((double)lg[id_tx] - (double)mx) / Z;
    const double sum_ts = TS / Z;
    // the allowed set: 0 ids > beg, 1 ids >= beg, 2 every id but sot / solm / not
    const int set = t == 0 ? 0 : sum_ts > p_maxtx ? 1 : 2;
    const unsigned long long k_a = set == 0 ? k_ts1 : set == 1 ? k_ts : k_all;
    const float m_a = unord_f32((uint32_t)(k_a >> 32));
    const float T = sa.rows[b].T;
    const bool draw = T > 0.0f;
    auto in_a = [&](int i) {
        return set == 0 ? i > a.beg : set == 1 ? i >= a.beg : (i != a.sot && i != a.solm && i != a.not_);
    };
    // pass 3: tiles of 64 consecutive ids
    const int nt = (a.V + 63) >> 6;
    double se = 0.0;
    // (one exp per loop: both in one body spill past the 128 registers of a 1024-thread workgroup)
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
            const double u = (double)(sm64(sa.rows[b].key + (unsigned long long)t) >> 11) * 0x1.0p-53;
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
            }
            j_tile = J;
            c_tile = cj;
        }
        __syncthreads();
        const int J = j_tile;  // (uniform; -1: rounding left no id, the largest of A)
        if (J >= 0 && w == 0) {
            const int i = J * 64 + lane;
            wl[lane] = i < a.V && in_a(i) ? exp(((double)lg[i] - (double)m_a) / (double)T) : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            id = a.V - 1;  // (sot, solm and not lie below beg: the last id belongs to every set)
            if (J >= 0) {
                double c = c_tile;
                #pragma unroll 1
                for (int k = 0; k < 64; ++k) {
                    if (wl[k] > 0.0) id = J * 64 + k;
                    if (c + wl[k] > target) break;
                    c += wl[k];
                }
            }
        }
    }
    if (tid != 0) return;
    double SE = 0.0;
    for (int i = 0; i < 16; ++i) SE += sse[i];
    a.tok_out[b] = id;
    if (id == a.eot) a.done[b] = 1;
    if (t == 0) sa.p_nosp[b] = (float)(exp((double)lg[a.solm] - (double)mx) / Z);
    if (t < a.max_rec) {
        TsRec r;
        r.id = id;
        r.tid = id_ts;
        r.p = (float)(exp((double)lg[id] - (double)mx) / Z);
        r.pt = (float)(p_maxts / (sum_ts + 1e-10));
        r.ptsum = (float)sum_ts;
        r.pad = 0;
        a.rec[(size_t)b * a.max_rec + t] = r;
        sa.plog[(size_t)b * a.max_rec + t] = (float)((double)lg[id] - ((double)m_a + log(SE)));
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
