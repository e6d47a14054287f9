// wmi_wide.hip — the wide decoder step of beam search in the batch
// (wmi_set_batch_beam, wmi_decode_timestamps_beam_rows; DESIGN.md "Beam search
// in the batch").
//
// One step over R = B * K <= 64 rows, row r = c * K + k hypothesis k of
// recording c.  The dense products are launch_gemm's MFMA GEMMs over the packed
// [R][n] activation matrix and LayerNorm is k_layernorm, as in the prompt
// prefill; the kernels here are what a step needs around them: the embedding
// prologue, the store of the QKV product with a guard for idle rows, the two
// attention shapes, and the beam step for every recording of the round.
// Kernel boundaries are the only synchronisation.  Positions, done words and
// histories are read from the device table (WdTable), never from kernel
// arguments, so one step is one fixed launch sequence.
//
// k_wd_self_attn: one workgroup per (row, head).  Four lanes share a key in the
// score pass (a 64-wide head row is four 32-byte pieces, two 16-byte loads a
// lane), eight lanes a key row in the P V pass; each key row is gathered from
// the cache slot the hypothesis' history names.  The softmax is the step
// kernels' (exact row maximum, ggml's table exp of f16(s - max), the sum in
// double, P = f16(e * (1 / sum))); the waves' partial outputs meet in LDS.
//
// k_wd_cross_attn: the K hypotheses of a recording read the same T x 64 encoder
// keys and values of a head, so a workgroup per (key chunk, head, recording)
// takes them as the 16 query columns of v_mfma_f32_16x16x32_f16 (columns past K
// are zero): S^T = K_enc Q^T leaves a lane one query's scores over 4 keys of a
// 16-key tile (rows 4 (lane >> 4) + {0..3}), two such tiles are the 8 k values
// of the lane's P^T operand of O^T = V^T P^T (the MFMA sums over k in any order
// as long as both operands agree), so P never passes through LDS.  A wave owns
// 32 of a 64-key tile's keys and keeps the running (m, l, O^T) of the prefill's
// cross-attention; the two waves merge in LDS and the chunk's partial goes out
// in f32 for k_wd_cross_combine.
// LDS: K [key][72] f16 (a score fragment read is 16 bytes a lane, 16 rows 36
// dwords apart start on the 16 multiples of 4 mod 64: conflict-free) and V^T
// [d][68] f16 (34 dwords a row: the 32 lanes of an 8-byte read pass start on
// 32 distinct even banks: conflict-free).  What conflicts is the staging's
// transposing 2-byte stores into V^T (eight lanes of a key row hit rows 8 apart
// in d: 8 * 34 = 16 mod 64, a 2-way conflict with the next key pair's lanes).
//
// A translation unit of its own: its code object is loaded with the first wide
// window, so a context that never runs one runs on the code objects it ran on
// before.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"
#include "wmi_pick.h"

#pragma clang fp contract(off)

namespace wmi {

namespace {

constexpr int WD_KLD = 72;            // halfs a K row in LDS
constexpr int WD_CK = 64;             // keys a cross-attention tile
constexpr int WD_VLD = WD_CK + 4;     // halfs a V^T row


__device__ __forceinline__ bool wd_idle(const WdTable &tb, int c, int k) {
    const BeamState *bs = tb.bs + c;
    return bs->done != 0 || k >= bs->n_active;
}

}  // namespace

// ---- embedding prologue ---------------------------------------------------------
__global__ __launch_bounds__(64) void k_wd_embed(WdTable tb, int K, const uint16_t *te, const float *pe, int n, int V, int tctx,
                                                 float *x, int32_t *rowmap) {
    const int r = blockIdx.x, c = r / K, k = r - c * K;
    const WdRec rec = tb.recs[c];
    const bool idle = wd_idle(tb, c, k) || rec.p < 0 || rec.p >= tctx;
    if (threadIdx.x == 0) rowmap[r] = idle ? -1 : r * tctx + rec.p;
    float *xr = x + (int64_t)r * n;
    if (idle) {  // (its rows of the GEMMs stay finite)
        for (int e = threadIdx.x * 4; e < n; e += 256) *(float4 *)(xr + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    int tok = rec.p == rec.np - 1 ? rec.last_tok : tb.bs[c].tok[k];
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;  // (the entry points check the ids: never out of the table)
    const f16 *t = (const f16 *)te + (int64_t)tok * n;
    const float *p = pe + (int64_t)rec.p * n;
    for (int e = threadIdx.x * 4; e < n; e += 256) {
        const half4 tv = *(const half4 *)(t + e);
        const float4 pv = *(const float4 *)(p + e);
        *(float4 *)(xr + e) = make_float4((float)tv[0] + pv.x, (float)tv[1] + pv.y, (float)tv[2] + pv.z, (float)tv[3] + pv.w);
    }
}

hipError_t launch_wd_embed(hipStream_t s, const WdTable &tb, int B, int K, const uint16_t *te, const float *pe, int n, int V,
                           int tctx, float *x, int32_t *rowmap) {
    if (B < 1 || K < 1 || K > BEAM_MAX || B * K > WD_ROWS || n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_embed, dim3(B * K), dim3(64), 0, s, tb, K, te, pe, n, V, tctx, x, rowmap);
    return hipGetLastError();
}

// ---- the QKV product into q and the wide cache ------------------------------------
// (k_pf_qkv_store with the guard: an idle row stores no key and no value)
__global__ __launch_bounds__(256) void k_wd_qkv_store(PfQkvArgs a) {
    const int cpr = a.N >> 2;  // 4-column groups a row
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)a.M * cpr) return;
    const int m = (int)(g / cpr), c0 = 4 * (int)(g - (int64_t)m * cpr);
    const int which = c0 / a.n, cc = c0 - which * a.n;  // (n % 4 == 0: a group lies in one part)
    const float4 v = *(const float4 *)(a.acc + (int64_t)m * a.N + c0), b = *(const float4 *)(a.bias + c0);
    ushort4 h;
    if (which == 0) {
        h.x = f2h_bits((v.x + b.x) * a.qscale); h.y = f2h_bits((v.y + b.y) * a.qscale);
        h.z = f2h_bits((v.z + b.z) * a.qscale); h.w = f2h_bits((v.w + b.w) * a.qscale);
        *(ushort4 *)(a.q + (int64_t)m * a.n + cc) = h;
        return;
    }
    const int64_t row = a.rowmap[m];
    if (row < 0) return;
    if (which == 1) {
        h.x = f2h_bits(v.x * a.qscale); h.y = f2h_bits(v.y * a.qscale);
        h.z = f2h_bits(v.z * a.qscale); h.w = f2h_bits(v.w * a.qscale);
        *(ushort4 *)(a.k + row * a.n + cc) = h;
    } else {
        h.x = f2h_bits(b.x + v.x); h.y = f2h_bits(b.y + v.y);
        h.z = f2h_bits(b.z + v.z); h.w = f2h_bits(b.w + v.w);
        *(ushort4 *)(a.v + row * a.n + cc) = h;
    }
}

hipError_t launch_wd_qkv_store(hipStream_t s, const PfQkvArgs &a) {
    if (a.M < 1 || a.n % 4 || (a.N != a.n && a.N != 3 * a.n)) return hipErrorInvalidValue;
    const int64_t groups = (int64_t)a.M * (a.N >> 2);
    hipLaunchKernelGGL(k_wd_qkv_store, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- self-attention of one row over its hypothesis' history ------------------------
__global__ __launch_bounds__(256) void k_wd_self_attn(WdSelfArgs a) {
    __shared__ float sc[512];  // (tctx <= 512, checked at the launch)
    __shared__ float redf[4];
    __shared__ double redd[4];
    __shared__ float op[4][64];
    const int r = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n;
    uint16_t *out = a.out + (int64_t)r * n + h * 64;
    if (a.rowmap[r] < 0) {  // (uniform) an idle row: zeros
        if (tid < 8) *(uint4 *)(out + tid * 8) = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int c = r / a.Kb, k = r - c * a.Kb;
    const int p = a.tb.recs[c].p, nk = p + 1;  // (0 <= p < tctx: k_wd_embed marks the row idle otherwise)
    const int32_t *src = a.tb.kv_src + ((int64_t)c * BEAM_MAX + k) * a.tctx;
    const int64_t base = (int64_t)c * a.Kb * a.tctx;  // the recording's first cache row
    // key j < p lies in the slot the history names (a slot of this recording), key p in the row's own
    auto cache_row = [&](int j) {
        int slot = j < p ? src[j] : k;
        slot = slot < 0 ? 0 : slot >= a.Kb ? a.Kb - 1 : slot;
        return (base + (int64_t)slot * a.tctx + j) * n + h * 64;
    };
    {   // scores: four lanes a key
        const int sub = tid & 3, kq = tid >> 2;
        const f16 *qr = (const f16 *)a.q + (int64_t)r * n + h * 64 + sub * 16;
        const half8 q0 = *(const half8 *)qr, q1 = *(const half8 *)(qr + 8);
        for (int j0 = 0; j0 < nk; j0 += 64) {
            const int j = j0 + kq;
            float s = 0.0f;
            if (j < nk) {
                const f16 *kr = (const f16 *)a.K + cache_row(j) + sub * 16;
                s = dot8(*(const half8 *)kr, q0, 0.0f);
                s = dot8(*(const half8 *)(kr + 8), q1, s);
            }
            s = xstep<XSum, 1>(s);
            s = xstep<XSum, 2>(s);
            if (sub == 0 && j < nk) sc[j] = s;
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < nk; j += 256) mx = fmaxf(mx, sc[j]);
    mx = wave_max(mx);
    if (lane == 0) redf[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));  // (key 0 exists: finite)
    double sum = 0.0;
    for (int j = tid; j < nk; j += 256) {
        const float e = exp_f16_exact(sc[j] - mx);
        sc[j] = e;
        sum += (double)e;
    }
    sum = wave_sum(sum);
    if (lane == 0) redd[w] = sum;
    __syncthreads();
    sum = ((redd[0] + redd[1]) + redd[2]) + redd[3];
    const float inv = (float)(1.0 / sum);
    // O = P V: eight lanes a key row, 32 key rows an iteration
    const int part = tid & 7, kg = tid >> 3;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    for (int j = kg; j < nk; j += 32) {
        const half8 v = *(const half8 *)((const f16 *)a.V + cache_row(j) + part * 8);
        const float pj = (float)f16_rt(sc[j] * inv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += pj * (float)v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = red_8_16_32(o[e]);  // over the wave's lanes of the same part
    if (lane < 8)
#pragma unroll
        for (int e = 0; e < 8; ++e) op[w][lane * 8 + e] = o[e];
    __syncthreads();
    if (tid < 64) out[tid] = f2h_bits(((op[0][tid] + op[1][tid]) + op[2][tid]) + op[3][tid]);
}

hipError_t launch_wd_self_attn(hipStream_t s, const WdSelfArgs &a, int R) {
    if (R < 1 || R > WD_ROWS || a.Kb < 1 || a.Kb > BEAM_MAX || R % a.Kb || a.n != a.H * 64 || a.tctx > 512)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_self_attn, dim3(R, a.H), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- cross-attention: a recording's hypotheses as the MFMA's query columns -----------
void wd_cross_split(int T, int B, int H, int cus, int *chunks, int *tiles) {
    const int ntile = (T + WD_CK - 1) / WD_CK;
    int want = (cus + B * H - 1) / (B * H);
    want = want < 1 ? 1 : want > ntile ? ntile : want;
    *tiles = (ntile + want - 1) / want;
    *chunks = (ntile + *tiles - 1) / *tiles;
}

__global__ __launch_bounds__(128) void k_wd_cross_attn(WdCrossArgs a) {
    __shared__ __attribute__((aligned(16))) f16 Ks[WD_CK * WD_KLD];
    __shared__ __attribute__((aligned(16))) f16 Vt[64 * WD_VLD];
    __shared__ float mrg[16][WD_PART];
    const int ch = blockIdx.x, h = blockIdx.y, c = blockIdx.z;
    if (a.tb.bs[c].done) return;  // (uniform; k_wd_cross_combine writes its rows' zeros)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lq = lane & 15, g = lane >> 4;
    const int n = a.n, T = a.T;
    int clip = a.tb.recs[c].clip;
    clip = clip < 0 ? 0 : clip;
    const uint16_t *Kc = a.K + (int64_t)clip * T * n + h * 64, *Vc = a.V + (int64_t)clip * T * n + h * 64;
    half8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[ks][e] = (f16)0.0f;
        if (lq < a.Kb) qf[ks] = *(const half8 *)((const f16 *)a.q + (int64_t)(c * a.Kb + lq) * n + h * 64 + ks * 32 + g * 8);
    }
    floatx4 O[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int v = 0; v < 4; ++v) O[dt][v] = 0.0f;
    float m = -INFINITY;
    double l = 0.0;
    for (int t = 0; t < a.tiles; ++t) {
        const int key0 = (ch * a.tiles + t) * WD_CK;
        if (key0 >= T) break;  // (uniform)
        for (int i = tid; i < WD_CK * 8; i += 128) {
            const int key = i >> 3, part = i & 7;
            uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;  // (keys past T: zero rows, masked below)
            if (key0 + key < T) {
                kv = *(const uint4 *)(Kc + (int64_t)(key0 + key) * n + part * 8);
                vv = *(const uint4 *)(Vc + (int64_t)(key0 + key) * n + part * 8);
            }
            *(uint4 *)(Ks + key * WD_KLD + part * 8) = kv;
            const half8 hv = __builtin_bit_cast(half8, vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(part * 8 + e) * WD_VLD + key] = hv[e];
        }
        __syncthreads();
        if (key0 + 32 * w < T) {  // (uniform over the wave: it has a key below T)
            floatx4 S[2];
            float tm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                floatx4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const half8 kf = *(const half8 *)(Ks + (32 * w + 16 * kt + lq) * WD_KLD + ks * 32 + g * 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float s = key0 + 32 * w + 16 * kt + 4 * g + v < T ? acc[v] : -INFINITY;
                    S[kt][v] = s;
                    tm = fmaxf(tm, s);
                }
            }
            tm = xstep<XMax, 16>(tm);
            tm = xstep<XMax, 32>(tm);  // (the wave's first key is below T: finite)
            const float mn = fmaxf(m, tm);
            const float alpha = m == -INFINITY ? 0.0f : expf(m - mn);
            double ps = 0.0;
            half8 pf;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float pe = S[kt][v] == -INFINITY ? 0.0f : exp_f16_exact(S[kt][v] - mn);
                    ps += (double)pe;
                    pf[4 * kt + v] = (f16)pe;  // (an f16 value already: exact)
                }
            ps = xstep<XSum, 16>(ps);
            ps = xstep<XSum, 32>(ps);
            l = l * (double)alpha + ps;
            m = mn;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
                for (int v = 0; v < 4; ++v) O[dt][v] = O[dt][v] * alpha;
                // V^T of head dim 16 dt + lq at the keys of pf: 4 g + {0..3} of the wave's two 16-key tiles
                const f16 *vr = Vt + (dt * 16 + lq) * WD_VLD + 32 * w + 4 * g;
                const half4 v0 = *(const half4 *)vr, v1 = *(const half4 *)(vr + 16);
                const half8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                O[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, O[dt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // the two waves' (m, l, O^T) of query lq meet in LDS; wave 0 writes the chunk's partial
    if (w == 1) {
        if (g == 0) { mrg[lq][0] = m; mrg[lq][1] = (float)l; }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int v = 0; v < 4; ++v) mrg[lq][2 + dt * 16 + 4 * g + v] = O[dt][v];
    }
    __syncthreads();
    if (w == 0 && lq < a.Kb) {
        const float m1 = mrg[lq][0];
        const float M = fmaxf(m, m1);  // (wave 0 has the chunk's first key: m is finite)
        const float a0 = m == -INFINITY ? 0.0f : expf(m - M), a1 = m1 == -INFINITY ? 0.0f : expf(m1 - M);
        float *dst = a.part + ((((int64_t)c * a.H + h) * a.chunks + ch) * 16 + lq) * WD_PART;
        if (g == 0) { dst[0] = M; dst[1] = (float)l * a0 + mrg[lq][1] * a1; }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int d = dt * 16 + 4 * g + v;
                dst[2 + d] = O[dt][v] * a0 + mrg[lq][2 + d] * a1;
            }
    }
}

// the chunks of (row, head) merged: out = f16(sum_ch o_ch exp(m_ch - M) / sum_ch l_ch exp(m_ch - M))
__global__ __launch_bounds__(64) void k_wd_cross_combine(WdCrossArgs a) {
    const int r = blockIdx.x, h = blockIdx.y, d = threadIdx.x;
    uint16_t *out = a.out + (int64_t)r * a.n + h * 64;
    if (a.rowmap[r] < 0) { out[d] = 0; return; }  // an idle row: zeros
    const int c = r / a.Kb, k = r - c * a.Kb;
    const float *pp = a.part + ((((int64_t)c * a.H + h) * a.chunks) * 16 + k) * WD_PART;
    const int64_t cs = 16 * WD_PART;
    float M = -INFINITY;
    for (int ch = 0; ch < a.chunks; ++ch) M = fmaxf(M, pp[ch * cs]);
    float L = 0.0f, o = 0.0f;
    for (int ch = 0; ch < a.chunks; ++ch) {
        const float wgt = expf(pp[ch * cs] - M);
        L += pp[ch * cs + 1] * wgt;
        o += pp[ch * cs + 2 + d] * wgt;
    }
    out[d] = f2h_bits(o * (1.0f / L));
}

hipError_t launch_wd_cross_attn(hipStream_t s, const WdCrossArgs &a) {
    if (a.B < 1 || a.Kb < 1 || a.Kb > BEAM_MAX || a.B * a.Kb > WD_ROWS || a.T < 1 || a.n != a.H * 64 || a.chunks < 1 || a.tiles < 1 ||
        (int64_t)a.chunks * a.tiles * WD_CK < a.T || (int64_t)(a.chunks - 1) * a.tiles * WD_CK >= a.T)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_cross_attn, dim3(a.chunks, a.H, a.B), dim3(128), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wd_cross_combine(s, a);
}

hipError_t launch_wd_cross_combine(hipStream_t s, const WdCrossArgs &a) {
    hipLaunchKernelGGL(k_wd_cross_combine, dim3(a.B * a.Kb, a.H), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---- the beam step of every recording -----------------------------------------------
namespace {

// recording c's argument block of wmi_tsbeam.hip's step, and the position behind its step's token
__device__ __forceinline__ TsBeamArgs wd_beam_args(const WdBeamArgs &w, int c, int &pos) {
    const WdRec rec = w.tb.recs[c];
    TsBeamArgs ta{};
    ta.b.logits = w.logits + (int64_t)c * w.K * w.V;
    ta.b.V = w.V; ta.b.K = w.K; ta.b.suppress_id = -1; ta.b.eot = w.eot;
    ta.b.feed_len = rec.np; ta.b.max_tokens = rec.max_tokens; ta.b.tctx = w.tctx;
    ta.b.bs = w.tb.bs + c;
    ta.b.kv_src = w.tb.kv_src + (int64_t)c * BEAM_MAX * w.tctx;
    ta.b.hist_parent = w.tb.hist_parent + (int64_t)c * w.tctx * BEAM_MAX;
    ta.b.hist_tok = w.tb.hist_tok + (int64_t)c * w.tctx * BEAM_MAX;
    ta.beg = w.beg; ta.sot = w.sot; ta.solm = w.solm; ta.not_ = w.not_;
    ta.tparts = w.tb.tparts + (int64_t)c * BEAM_MAX * BEAM_NS;
    ta.hist_rec = w.tb.hist_rec + (int64_t)c * (w.tctx + 1) * BEAM_MAX;
    ta.fin_rec = ta.hist_rec + (int64_t)w.tctx * BEAM_MAX;
    pos = rec.p + 1;
    return ta;
}

}  // namespace

// WMI_LOGITS_ALL: row k of recording c's step t -> lg_all[c][t][k]
__global__ __launch_bounds__(256) void k_wd_logits_capture(WdBeamArgs w) {
    const int r = blockIdx.x, c = r / w.K, k = r - c * w.K;
    if (wd_idle(w.tb, c, k)) return;
    const WdRec rec = w.tb.recs[c];
    const int t = rec.p - (rec.np - 1);
    if (t < 0 || t >= w.lg_steps) return;
    const float *src = w.logits + (int64_t)r * w.V;
    float *dst = w.lg_all + (((int64_t)c * w.lg_steps + t) * w.K + k) * w.V;
    for (int i = threadIdx.x; i < w.V; i += 256) dst[i] = src[i];
}

// k_tsbeam_part for split blockIdx.x of row blockIdx.y of recording blockIdx.z: the split's statistics are
// wmi_tsbeam.hip's, the rounds wmi_pick.h's.  This body and k_wd_beam_select's step 1 are twins of
// k_tsbeam_part / k_tsbeam_select in wmi_tsbeam.hip, kept word for word (moving them into wmi_pick.h changed that
// unit's code object): a change to the statistics or to the rows' rule is made in both files
__global__ __launch_bounds__(256) void k_wd_beam_part(WdBeamArgs wa) {
    int pos;
    const TsBeamArgs ta = wd_beam_args(wa, blockIdx.z, pos);
    const BeamArgs &a = ta.b;
    const int sp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
    TsBeamPart *out = ta.tparts + (int64_t)b * BEAM_NS + sp;
    float m_a, m_tl;
    split_rounds(v, lo, a.K, el_a, el_t, !first, has_ts, redk, m_a, m_tl, [&](int r, float va, int ia, float vt, int it) {
        out->a_val[r] = va;
        out->a_id[r] = ia;
        out->ts_val[r] = vt;
        out->ts_id[r] = it;
    });
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
        out->m_tl = first ? m_tl : m_ts;
        out->sum_tl = first ? ((redd[3][0] + redd[3][1]) + redd[3][2]) + redd[3][3] : out->sum_ts;
    }
}

// k_tsbeam_select for recording blockIdx.x: the rows' rule as in wmi_tsbeam.hip, the merge, ranking, walk and
// history re-pointing wmi_pick.h's; then the recording's position moves on (its done word is the BeamState's)
__global__ __launch_bounds__(256) void k_wd_beam_select(WdBeamArgs wa) {
    int pos;
    const TsBeamArgs ta = wd_beam_args(wa, blockIdx.x, pos);
    const BeamArgs &a = ta.b;
    BeamState *bs = a.bs;
    if (pos < a.feed_len || bs->done) return;
    const int t = pos - a.feed_len, TK = a.K + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    struct Lds : BeamSelLds {
        double row_m[BEAM_MAX], row_z[BEAM_MAX];
        float row_pt[BEAM_MAX], row_ptsum[BEAM_MAX];
        int row_tid[BEAM_MAX];
    };
    __shared__ Lds sl;
    const int na_old = bs->n_active;  // (1 at t = 0: hypothesis 0 alone is expanded)
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
    beam_select_tail(a, sl, pos, na_old, [&](int nf, int c) { ta.fin_rec[nf] = record(c); },
                     [&](int s, int, int c) { ta.hist_rec[t * BEAM_MAX + s] = record(c); });
    if (threadIdx.x == 0) wa.tb.recs[blockIdx.x].p = pos;  // (every thread read it before the tail's barriers)
}

hipError_t launch_wd_beam_step(hipStream_t s, const WdBeamArgs &a) {
    if (a.K < 1 || a.K > BEAM_MAX || a.B < 1 || a.B * a.K > WD_ROWS || a.tctx > 512 || (a.V + BEAM_NS - 1) / BEAM_NS > 4096 ||
        a.beg < 1 || a.V < a.beg + 2)
        return hipErrorInvalidValue;
    hipError_t e;
    if (a.lg_all) {
        hipLaunchKernelGGL(k_wd_logits_capture, dim3(a.B * a.K), dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_wd_beam_part, dim3(BEAM_NS, a.K, a.B), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wd_beam_select, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the capture alone, in front of the ruled pair of wmi_wide_rules.hip
hipError_t launch_wd_logits_capture(hipStream_t s, const WdBeamArgs &a) {
    if (!a.lg_all || a.K < 1 || a.K > BEAM_MAX || a.B < 1 || a.B * a.K > WD_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_logits_capture, dim3(a.B * a.K), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace wmi
