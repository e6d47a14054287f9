// wmi_prefill.hip — the kernels of the prompt prefill (wmi_set_prefill,
// wmi_prefill_logits; DESIGN.md "Prompt prefill").
//
// The prompts of a round's rows go through the decoder layers as one packed
// [M][n] activation matrix: the dense products are launch_gemm's MFMA GEMMs,
// LayerNorm is k_layernorm, and the kernels here are the embedding prologue,
// the store of the QKV product (K and V where and as the step kernels store
// them), the two attention shapes the encoder's k_attn_enc4 does not cover,
// and the hand-over of the step state.
//
// Both attention kernels compute S^T = K Q^T with v_mfma_f32_32x32x16_f16, so
// that a lane holds one query's scores over 16 keys of a 32-key tile (rows
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the accumulator) and the row maximum
// and sum are a loop over its own registers plus one exchange with lane ^ 32.
// O^T = V^T P^T follows without a trip through LDS for P: the MFMA sums over
// its 16 k in any order as long as both operands agree, so k-step s of a key
// tile takes, from half-wave lh, the 8 keys that lane's registers 8 s .. 8 s +
// 7 hold (16 s + 4 lh + {0..3} and 16 s + 8 + 4 lh + {0..3}): the P operand is
// those registers rounded to f16, the V operand two 8-byte reads of a V^T
// image in LDS.  The result again has the query in the lane, so the output's
// four consecutive head dims of a register group are one 8-byte store.
//
// LDS layouts (both kernels):
//   K   [key][72] f16: a 64-wide head row padded to 144 bytes = 36 dwords.  A
//       score fragment read is 16 bytes a lane, row = lane & 31; 16 rows 36
//       dwords apart start on the 16 distinct multiples of 4 mod 64, so each
//       16-lane pass of a ds_read_b128 covers all 64 banks once.
//   V^T [d][keys + 4] f16: 130 dwords a row (self, 256 keys) or 34 (cross, 64
//       keys), both = 2 mod 4 and = 2 (mod 32) * odd, so the 32 rows d of an
//       8-byte fragment read start on 32 distinct even banks: conflict-free.
//       (The staging's transposing 2-byte stores, pf_put_vt, do conflict.)
//
// A translation unit of its own: its code object is loaded with the first
// prefill pass, so a context that never calls wmi_set_prefill or
// wmi_prefill_logits runs on the code objects it ran on before.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

#pragma clang fp contract(off)

namespace wmi {

namespace {

constexpr int PF_QT = 64;                    // queries a workgroup: two waves of 32
constexpr int PF_KLD = 72;                   // halfs a K row in LDS
constexpr int PF_SVLD = PF_MAX_KEYS + 4;     // halfs a V^T row, self-attention
constexpr int PF_CK = 64;                    // keys a cross-attention tile
constexpr int PF_CVLD = PF_CK + 4;           // halfs a V^T row, cross-attention
constexpr int PF_SKT = PF_MAX_KEYS / 32;     // 32-key score tiles a wave holds in registers
constexpr size_t PF_SELF_LDS = ((size_t)PF_MAX_KEYS * PF_KLD + 64 * PF_SVLD) * 2;

// key of accumulator register r in its 32-key tile
__device__ __forceinline__ int pf_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// 8 halfs of V row `key`, head dims 8 part .. 8 part + 7, into the V^T image
__device__ __forceinline__ void pf_put_vt(f16 *vt, int ld, int key, int part, uint4 v) {
    const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[(part * 8 + e) * ld + key] = h[e];
}

// one k-step of O^T += V^T P^T: the V operand of head dims dt * 32 + (lane & 31), keys k0 + {0..3, 8..11}
__device__ __forceinline__ half8 pf_vfrag(const f16 *vt, int ld, int d, int k0) {
    const half4 a0 = *(const half4 *)(vt + d * ld + k0), a1 = *(const half4 *)(vt + d * ld + k0 + 8);
    return half8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
}

// a lane's 2 x 16 outputs (head dims dt * 32 + 8 g + 4 lh + {0..3}) of one query, scaled, as 8-byte stores
__device__ __forceinline__ void pf_store_o(uint16_t *dst, const floatx16 (&O)[2], float scale, int lh) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4 hv;
#pragma unroll
            for (int j = 0; j < 4; ++j) hv[j] = f16_rt(O[dt][4 * g + j] * scale);
            *(half4 *)(dst + dt * 32 + 8 * g + 4 * lh) = hv;
        }
}

}  // namespace

// ---- embedding prologue ---------------------------------------------------------
__global__ __launch_bounds__(64) void k_pf_embed(PfRecs recs, const uint16_t *te, const float *pe, const int32_t *feed,
                                                 int feed_stride, int n, int V, int tctx, float *x, int32_t *rowmap) {
    const PfRec rec = recs.r[blockIdx.y];
    const int i = blockIdx.x;
    if (i >= rec.len) return;
    int tok = feed[(int64_t)blockIdx.y * feed_stride + rec.lo + i];
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;  // (the entry points check the ids: never out of the table)
    const int64_t row = rec.row0 + i;
    if (threadIdx.x == 0) rowmap[row] = rec.slot * tctx + rec.lo + i;
    const f16 *t = (const f16 *)te + (int64_t)tok * n;
    const float *p = pe + (int64_t)i * n;
    for (int e = threadIdx.x * 4; e < n; e += 256) {
        const half4 tv = *(const half4 *)(t + e);
        const float4 pv = *(const float4 *)(p + e);
        *(float4 *)(x + row * n + e) =
            make_float4((float)tv[0] + pv.x, (float)tv[1] + pv.y, (float)tv[2] + pv.z, (float)tv[3] + pv.w);
    }
}

hipError_t launch_pf_embed(hipStream_t s, const PfRecs &recs, const uint16_t *te, const float *pe, const int32_t *feed,
                           int feed_stride, int n, int V, int tctx, float *x, int32_t *rowmap) {
    if (recs.n < 1 || recs.n > DEC_ROWS || recs.max_len < 1 || n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pf_embed, dim3(recs.max_len, recs.n), dim3(64), 0, s, recs, te, pe, feed, feed_stride, n, V, tctx, x,
                       rowmap);
    return hipGetLastError();
}

// ---- the QKV product into q and the self-attention cache -----------------------------
// (a kernel of its own behind an EPI_F32 GEMM, not a GEMM epilogue: the GEMM instances stay the ones every
// context already runs; DESIGN.md "Prompt prefill")
__global__ __launch_bounds__(256) void k_pf_qkv_store(PfQkvArgs a) {
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
    } else if (which == 1) {
        h.x = f2h_bits(v.x * a.qscale); h.y = f2h_bits(v.y * a.qscale);
        h.z = f2h_bits(v.z * a.qscale); h.w = f2h_bits(v.w * a.qscale);
        *(ushort4 *)(a.k + (int64_t)a.rowmap[m] * a.n + cc) = h;
    } else {
        h.x = f2h_bits(b.x + v.x); h.y = f2h_bits(b.y + v.y);
        h.z = f2h_bits(b.z + v.z); h.w = f2h_bits(b.w + v.w);
        *(ushort4 *)(a.v + (int64_t)a.rowmap[m] * a.n + cc) = h;
    }
}

hipError_t launch_pf_qkv_store(hipStream_t s, const PfQkvArgs &a) {
    if (a.M < 1 || a.n % 4 || (a.N != a.n && a.N != 3 * a.n)) return hipErrorInvalidValue;
    const int64_t groups = (int64_t)a.M * (a.N >> 2);
    hipLaunchKernelGGL(k_pf_qkv_store, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- causal self-attention over a prompt ------------------------------------------
// One workgroup per (query tile of 64 positions, head, recording).  The head's K
// and V rows 0 .. last position of the tile are staged once (V transposed); a
// wave owns 32 queries and holds their scores over the whole key range in
// registers (PF_SKT tiles), so the softmax is the step kernels': exact row
// maximum, ggml's table exp of f16(s - max), the sum in double, P = f16(e *
// (1 / sum)), O = P V in f32, rounded to f16 for the output projection.  The
// causal mask is key <= query; a recording's keys start at its own first
// position, so nothing below lo[b] is ever read.
__global__ __launch_bounds__(128) void k_pf_self_attn(PfAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pf_sm[];
    f16 *Ks = (f16 *)pf_sm, *Vt = Ks + PF_MAX_KEYS * PF_KLD;
    const PfRec rec = a.recs.r[blockIdx.z];
    const int h = blockIdx.y, i0 = blockIdx.x * PF_QT;
    if (i0 >= rec.len) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int n = a.n;
    const int nk = min(i0 + PF_QT, rec.len), nkp = (nk + 31) & ~31;  // (len <= PF_MAX_KEYS: nkp too)
    const int64_t crow = (int64_t)rec.slot * a.tctx + rec.lo;
    for (int c = tid; c < nkp * 8; c += 128) {
        const int key = c >> 3, part = c & 7;
        uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;  // (rows past nk: zero, their P entries are 0 too)
        if (key < nk) {
            const int64_t o = (crow + key) * n + h * 64 + part * 8;
            kv = *(const uint4 *)(a.K + o);
            vv = *(const uint4 *)(a.V + o);
        }
        *(uint4 *)(Ks + key * PF_KLD + part * 8) = kv;
        pf_put_vt(Vt, PF_SVLD, key, part, vv);
    }
    __syncthreads();
    const int q0 = i0 + 32 * w;
    if (q0 >= rec.len) return;
    const int iq = q0 + lr;
    const int nkt = min(q0 + 32, nkp) >> 5;  // key tiles this wave's queries reach
    half8 qf[4];
    {
        const f16 *qr = (const f16 *)a.q + (int64_t)(rec.row0 + min(iq, rec.len - 1)) * n + h * 64 + lh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const half8 *)(qr + ks * 16);
    }
    floatx16 S[PF_SKT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < PF_SKT; ++kt) {
        if (kt < nkt) {
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const half8 kf = *(const half8 *)(Ks + (kt * 32 + lr) * PF_KLD + ks * 16 + lh * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = kt * 32 + pf_row(r, lh) <= iq ? acc[r] : -INFINITY;
                S[kt][r] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = xstep<XMax, 32>(mx);  // (key 0 is never masked: finite)
    double sum = 0.0;
#pragma unroll
    for (int kt = 0; kt < PF_SKT; ++kt)
        if (kt < nkt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = S[kt][r] == -INFINITY ? 0.0f : exp_f16_exact(S[kt][r] - mx);
                S[kt][r] = p;
                sum += (double)p;
            }
    sum = xstep<XSum, 32>(sum);
    const float inv = (float)(1.0 / sum);
    floatx16 O[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.0f;
#pragma unroll
    for (int kt = 0; kt < PF_SKT; ++kt)
        if (kt < nkt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                half8 pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = f16_rt(S[kt][8 * s + e] * inv);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf_vfrag(Vt, PF_SVLD, dt * 32 + lr, kt * 32 + 16 * s + 4 * lh),
                                                                   pf, O[dt], 0, 0, 0);
            }
    if (iq < rec.len) pf_store_o(a.out + (int64_t)(rec.row0 + iq) * n + h * 64, O, 1.0f, lh);
}

hipError_t launch_pf_self_attn(hipStream_t s, const PfAttnArgs &a) {
    if (a.recs.n < 1 || a.recs.n > DEC_ROWS || a.recs.max_len < 1 || a.recs.max_len > PF_MAX_KEYS || a.n != a.H * 64)
        return hipErrorInvalidValue;
    // dynamic LDS above 64 KiB is opted into once per device (a context lives on one device)
    static bool allowed[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !allowed[dev]) {
        e = hipFuncSetAttribute((const void *)k_pf_self_attn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PF_SELF_LDS);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) allowed[dev] = true;
    }
    hipLaunchKernelGGL(k_pf_self_attn, dim3((a.recs.max_len + PF_QT - 1) / PF_QT, a.H, a.recs.n), dim3(128), PF_SELF_LDS, s, a);
    return hipGetLastError();
}

// ---- cross-attention of the packed rows ---------------------------------------------
// One workgroup per (query tile of 64 positions, head, recording) walks the T
// encoder keys of the recording's clip in tiles of 64 through two LDS buffers:
// tile t + 1 is requested into registers before tile t's MFMAs and stored behind
// them, one barrier a tile.  A wave owns 32 queries and keeps, per query, the
// running maximum m, the running sum l (double) and O^T in f32: a tile's
// scores give m' = max(m, tile max), e = ggml's table exp of f16(s - m'), l =
// l exp(m - m') + sum e, O = O exp(m - m') + f16(e) V; at the end O / l, rounded
// to f16.  Keys past T (the last tile of T = 1500, a short audio context) are
// masked out of the maximum and the sum and their K / V rows are zero.
__global__ __launch_bounds__(128) void k_pf_cross_attn(PfAttnArgs a) {
    __shared__ __attribute__((aligned(16))) f16 Ks[2][PF_CK * PF_KLD];
    __shared__ __attribute__((aligned(16))) f16 Vt[2][64 * PF_CVLD];
    const PfRec rec = a.recs.r[blockIdx.z];
    const int h = blockIdx.y, i0 = blockIdx.x * PF_QT;
    if (i0 >= rec.len) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int n = a.n, T = a.T, ntile = (T + PF_CK - 1) / PF_CK;
    const uint16_t *Kc = a.K + (int64_t)rec.clip * T * n + h * 64, *Vc = a.V + (int64_t)rec.clip * T * n + h * 64;
    uint4 rk[4], rv[4];
    auto load = [&](int t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + 128 * j, key = t * PF_CK + (c >> 3), part = c & 7;
            rk[j] = rv[j] = make_uint4(0u, 0u, 0u, 0u);
            if (key < T) {
                rk[j] = *(const uint4 *)(Kc + (int64_t)key * n + part * 8);
                rv[j] = *(const uint4 *)(Vc + (int64_t)key * n + part * 8);
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + 128 * j, key = c >> 3, part = c & 7;
            *(uint4 *)(Ks[buf] + key * PF_KLD + part * 8) = rk[j];
            pf_put_vt(Vt[buf], PF_CVLD, key, part, rv[j]);
        }
    };
    const int q0 = i0 + 32 * w, iq = q0 + lr;
    const bool active = q0 < rec.len;  // (a wave without queries still stages its share of every tile)
    half8 qf[4];
    {
        const f16 *qr = (const f16 *)a.q + (int64_t)(rec.row0 + min(iq, rec.len - 1)) * n + h * 64 + lh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const half8 *)(qr + ks * 16);
    }
    floatx16 O[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.0f;
    float m = -INFINITY;
    double l = 0.0;
    load(0);
    store(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntile) load(t + 1);
        if (active) {
            floatx16 S[2];
            float tm = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                floatx16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const half8 kf = *(const half8 *)(Ks[buf] + (kk * 32 + lr) * PF_KLD + ks * 16 + lh * 8);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = t * PF_CK + kk * 32 + pf_row(r, lh) < T ? acc[r] : -INFINITY;
                    S[kk][r] = s;
                    tm = fmaxf(tm, s);
                }
            }
            tm = xstep<XMax, 32>(tm);  // (a tile's first key is below T: finite)
            const float mn = fmaxf(m, tm);
            const float alpha = m == -INFINITY ? 0.0f : expf(m - mn);
            double ps = 0.0;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = S[kk][r] == -INFINITY ? 0.0f : exp_f16_exact(S[kk][r] - mn);
                    S[kk][r] = p;
                    ps += (double)p;
                }
            l = l * (double)alpha + xstep<XSum, 32>(ps);
            m = mn;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[dt][r] = O[dt][r] * alpha;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    half8 pf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[e] = (f16)S[kk][8 * s + e];  // (an f16 value already: exact)
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                            pf_vfrag(Vt[buf], PF_CVLD, dt * 32 + lr, kk * 32 + 16 * s + 4 * lh), pf, O[dt], 0, 0, 0);
                }
        }
        if (t + 1 < ntile) store(buf ^ 1);  // (last read at tile t - 1, before the barrier that ended it)
        __syncthreads();
    }
    if (active && iq < rec.len) pf_store_o(a.out + (int64_t)(rec.row0 + iq) * n + h * 64, O, (float)(1.0 / l), lh);
}

hipError_t launch_pf_cross_attn(hipStream_t s, const PfAttnArgs &a) {
    if (a.recs.n < 1 || a.recs.n > DEC_ROWS || a.recs.max_len < 1 || a.T < 1 || a.n != a.H * 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pf_cross_attn, dim3((a.recs.max_len + PF_QT - 1) / PF_QT, a.H, a.recs.n), dim3(128), 0, s, a);
    return hipGetLastError();
}

// ---- the step state behind a prefill ---------------------------------------------------
__global__ __launch_bounds__(256) void k_pf_start(DecState *st, int pos, XSync *sync, int n_sync, uint32_t cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) st->pos = pos;
    if (i < n_sync) sync[i].cnt = cnt;
}

hipError_t launch_pf_start(hipStream_t s, DecState *st, int pos, XSync *sync, int n_sync, uint32_t cnt) {
    if (!sync) n_sync = 0;
    hipLaunchKernelGGL(k_pf_start, dim3(n_sync / 256 + 1), dim3(256), 0, s, st, pos, sync, n_sync, cnt);
    return hipGetLastError();
}

}  // namespace wmi
