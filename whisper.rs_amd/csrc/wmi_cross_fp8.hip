// wmi_cross_fp8.hip — MXFP8 cross-attention keys and values for the wide
// decoder step (wmi_set_cross_fp8; DESIGN.md "MXFP8 cross keys and values").
//
// The format: a block is 32 consecutive elements along the state dimension of
// one key or value row (a 64-wide head row is two blocks).  Its shared exponent
// s is the smallest integer in [-15, 7] with amax * 2^-s <= 448 (an all-zero
// block: -15), stored as the byte s + 127 (E8M0); its elements are x * 2^-s
// rounded to nearest even into OCP e4m3fn, saturated at +-448.  With that range
// of s every e4m3 * 2^s is an f16 number (at most 4 significant bits, between
// 2^-24 and 57344), so the f16 "rendering" of a quantised row is exact.
//
// Device layout.  The payload keeps the f16 planes' order, [L][clips][T][n]
// bytes.  The scale bytes of plane (layer, clip) lie per head over the keys,
// [ceil(n / 64)][Tp][2] with Tp = T rounded up to 64: the two bytes of (head,
// key) are that head row's two blocks, and a head's 2 Tp bytes are contiguous,
// so an attention lane fetches the scales of four consecutive keys in one
// 8-byte load.  Bytes of keys in [T, Tp) are never written; whatever they hold
// is a finite scale, and the kernels multiply it into zeros.
//
// k_cross_fp8_quant: elementwise over blocks, bandwidth-bound.  A lane takes 16
//   halfs (two 16-byte loads), two lanes share a block: amax of the |x| bit
//   patterns with one quad_perm exchange, s from the f16 exponent and mantissa
//   bits in integer arithmetic, v_cvt_pk_fp8_f32 of x * 2^-s (exact in f32),
//   one 16-byte payload store, and the rendering written back over the f16 row
//   with v_cvt_scalef32_pk_f16_fp8 (two 16-byte stores).
//
// k_wd_cross_attn1_f8: k_wd_cross_attn1 on a 64-byte key row.  Four lanes still
//   share a row, now one 16-byte load each (16 elements, half a scale block),
//   and the same four lanes take the value row's 16 head dims, so P stays in
//   the lanes that computed it (no permute).  A wave's block is 64 keys (pass
//   sb of four: key 4 (lane >> 2) + sb), 8 payload loads of 16 bytes and two
//   scale loads of 8 bytes a lane, two blocks in flight: the f16 kernel's
//   16 KiB a wave, over twice the keys.  Keys are converted unscaled (every
//   e4m3 value is a normal f16 number), dotted with v_dot2_f32_f16 against the
//   f16 query, and the lane's partial sum is multiplied by its block's 2^s
//   (exact); a value element enters as (P 2^s) * e4m3, the same real product as
//   P times the rendered value.  Rounding points are k_wd_cross_attn1's: f32
//   scores, a running maximum per wave, P = exp_f16_exact(s - m), the sum in
//   double, alpha = expf(m_old - m_new).  No MFMA, no LDS but the waves' merge.
//
// k_wd_cross_attn_f8: k_wd_cross_attn with fp8 global loads.  A staging thread
//   loads 16 bytes of a key row and of a value row (a 64-key tile is 2 + 2
//   loads a thread where the f16 kernel issues 4 + 4) and renders them to f16
//   in registers with the scaled convert on the way into the K tile and the
//   transposed V tile, so the LDS layout, the fragment reads and the MFMA
//   (v_mfma_f32_16x16x32_f16, the query not quantised) are unchanged.  Keeping
//   bytes in LDS would halve the tile's store traffic but turn every fragment
//   read into a convert per MFMA operand on each of the four d tiles; the
//   render at staging converts each byte once.  The transposing 2-byte stores
//   keep their 2-way conflict (the four 16-element parts of a key row land on
//   rows 16 apart in d: 16 * 34 dwords = 32 mod 64, parts 0 and 2 collide).
//
// Both attention kernels write partials in k_wd_cross_combine's layout.
// A translation unit and code object of its own.
#include <hip/hip_runtime.h>
#include <math.h>

#include "wmi_device.h"
#include "wmi_internal.h"

#pragma clang fp contract(off)

namespace wmi {

namespace {

constexpr int F1_BLK = 64;     // keys a wave's block
constexpr int F1_WAVES = 4;
constexpr int F8_CK = 64;      // keys a tile of wd_cross_split
constexpr int F8_KLD = 72;     // halfs a K row in LDS
constexpr int F8_VLD = F8_CK + 4;  // halfs a V^T row

__device__ __forceinline__ float f8_exp2(uint32_t e8m0) { return __uint_as_float(e8m0 << 23); }

// 16 e4m3 bytes times `scale` as 16 halfs
__device__ __forceinline__ void f8_render16(const uint4 b, float scale, half8 &lo, half8 &hi) {
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
    half2v p[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        p[2 * i] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[i], scale, false);
        p[2 * i + 1] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[i], scale, true);
    }
    lo = half8{p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], p[3][0], p[3][1]};
    hi = half8{p[4][0], p[4][1], p[5][0], p[5][1], p[6][0], p[6][1], p[7][0], p[7][1]};
}

}  // namespace

// ---- the quantiser --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cross_fp8_quant(F8QuantArgs a) {
    const int per = a.n >> 4;  // lanes a row
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.rows * per) return;  // (a block's two lanes leave together: rows * per is even)
    uint16_t *xp = a.x + g * 16;
    const uint4 x0 = *(const uint4 *)xp, x1 = *(const uint4 *)(xp + 8);
    const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    uint32_t am = 0;  // the largest |x| bit pattern (finite f16: ordered as integers)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t u = w[i] & 0x7fff7fffu;
        am = max(am, max(u & 0xffffu, u >> 16));
    }
    am = max(am, dpp_xor1(am));
    // amax = m 2^e, 1 <= m < 2 (exponent field e + 15): amax 2^-s <= 448 = 1.75 2^8 holds from s = e - 8, and from
    // e - 7 when the mantissa field is above 0x300; adding 0xff carries into the exponent field exactly then.
    // Subnormals and zero come out below -15
    int s = (int)((am + 0xffu) >> 10) - 23;
    s = s < -15 ? -15 : s > 7 ? 7 : s;
    const float inv = f8_exp2((uint32_t)(127 - s)), scl = f8_exp2((uint32_t)(127 + s));
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const half2v h = __builtin_bit_cast(half2v, w[i]);
        // (x 2^-s is exact in f32; beyond +-448 only for |x| > 57344)
        const float f0 = fminf(fmaxf((float)h[0] * inv, -448.0f), 448.0f);
        const float f1 = fminf(fmaxf((float)h[1] * inv, -448.0f), 448.0f);
        if (i & 1) q[i >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, (int)q[i >> 1], true);
        else q[i >> 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
    }
    const uint4 qv = make_uint4(q[0], q[1], q[2], q[3]);
    *(uint4 *)(a.q + g * 16) = qv;
    half8 lo, hi;
    f8_render16(qv, scl, lo, hi);
    *(half8 *)xp = lo;
    *(half8 *)(xp + 8) = hi;
    if ((g & 1) == 0) {
        const int64_t row = g / per;
        const int j = (int)(g - row * per) >> 1;  // the row's block
        const int64_t plane = row / a.T;
        const int t = (int)(row - plane * a.T);
        a.sc[plane * f8_scale_plane_bytes(a.T, a.n) + ((int64_t)(j >> 1) * a.Tp + t) * 2 + (j & 1)] = (uint8_t)(s + 127);
    }
}

hipError_t launch_cross_fp8_quant(hipStream_t s, const F8QuantArgs &a) {
    if (a.rows < 1 || a.n < 32 || a.n % 32 || a.T < 1 || a.rows % a.T || a.Tp != f8_tp(a.T)) return hipErrorInvalidValue;
    const int64_t lanes = a.rows * (a.n / 16);
    if ((lanes + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cross_fp8_quant, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- K = 1: one query a (recording, head), global memory to registers -------------------
namespace {

struct F1Block {
    uint4 k[4], v[4];  // pass sb: the lane's 16 bytes of key / value row 4 (lane >> 2) + sb
    uint2 ks, vs;      // the scale bytes of the lane's four rows: byte 2 sb + block
};

// the lane's pieces of keys [base, base + 64) below `end` (rows at or past it: zeros, no load)
__device__ __forceinline__ void f1_load(F1Block &b, const uint8_t *Kc, const uint8_t *Vc, const uint8_t *Ksc, const uint8_t *Vsc,
                                        int n, int base, int end, int lane) {
    const int sub = lane & 3, kq = lane >> 2;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
        const int key = base + 4 * kq + sb;
        b.k[sb] = b.v[sb] = z;
        if (key < end) {
            b.k[sb] = *(const uint4 *)(Kc + (int64_t)key * n + sub * 16);
            b.v[sb] = *(const uint4 *)(Vc + (int64_t)key * n + sub * 16);
        }
    }
    b.ks = b.vs = make_uint2(0u, 0u);
    if (base + 4 * kq < end) {  // (four keys' bytes, 8-byte aligned; those past `end` lie below Tp and meet zeros)
        b.ks = *(const uint2 *)(Ksc + (int64_t)(base + 4 * kq) * 2);
        b.vs = *(const uint2 *)(Vsc + (int64_t)(base + 4 * kq) * 2);
    }
}

// 2^s of row sb's block `blk` out of a lane's scale bytes
__device__ __forceinline__ float f1_scale(const uint2 w, int sb, int blk) {
    const uint32_t word = sb < 2 ? w.x : w.y;
    return f8_exp2((word >> (8 * (2 * (sb & 1) + blk))) & 0xffu);
}

}  // namespace

__global__ __launch_bounds__(64 * F1_WAVES) void k_wd_cross_attn1_f8(WdCrossF8Args fa) {
    __shared__ float mrg[F1_WAVES][WD_PART];
    const WdCrossArgs &a = fa.a;
    const int ch = blockIdx.x, h = blockIdx.y, c = blockIdx.z;
    if (a.rowmap[c] < 0) return;  // (uniform) an idle row; k_wd_cross_combine writes its zeros
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n, T = a.T;
    const int k0 = ch * a.tiles * F8_CK, k1 = min(T, k0 + a.tiles * F8_CK);  // (k0 < T: checked at the launch)
    int clip = a.tb.recs[c].clip;
    clip = clip < 0 ? 0 : clip;
    const uint8_t *Kc = fa.K8 + (int64_t)clip * T * n + h * 64, *Vc = fa.V8 + (int64_t)clip * T * n + h * 64;
    const int64_t so = (int64_t)clip * f8_scale_plane_bytes(T, n) + (int64_t)h * fa.Tp * 2;
    const uint8_t *Ksc = fa.Ksc + so, *Vsc = fa.Vsc + so;
    const int sub = lane & 3, blk = sub >> 1;
    const f16 *qr = (const f16 *)a.q + (int64_t)c * n + h * 64 + sub * 16;
    const half8 q0 = *(const half8 *)qr, q1 = *(const half8 *)(qr + 8);
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.0f;
    float m = -INFINITY;
    double l = 0.0;
    int base = k0 + w * F1_BLK;
    F1Block cur;
    f1_load(cur, Kc, Vc, Ksc, Vsc, n, base, k1, lane);
    for (; base < k1; base += F1_BLK * F1_WAVES) {  // (uniform over the wave: the block has a key below k1)
        F1Block nxt;
        f1_load(nxt, Kc, Vc, Ksc, Vsc, n, base + F1_BLK * F1_WAVES, k1, lane);
        float s[4], tm = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            half8 klo, khi;
            f8_render16(cur.k[sb], 1.0f, klo, khi);
            float v = dot8(klo, q0, 0.0f);
            v = dot8(khi, q1, v);
            v = v * f1_scale(cur.ks, sb, blk);
            v = xstep<XSum, 1>(v);
            v = xstep<XSum, 2>(v);
            s[sb] = base + 4 * (lane >> 2) + sb < k1 ? v : -INFINITY;
            tm = fmaxf(tm, s[sb]);
        }
        tm = xstep<XMax, 8>(tm);
        tm = xstep<XMax, 4>(tm);
        tm = xstep<XMax, 16>(tm);
        tm = xstep<XMax, 32>(tm);  // (the block's first key is below k1: finite)
        const float mn = fmaxf(m, tm);
        const float alpha = m == -INFINITY ? 0.0f : expf(m - mn);
        float pe[4];
        double pl = 0.0;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            pe[sb] = s[sb] == -INFINITY ? 0.0f : exp_f16_exact(s[sb] - mn);
            pl += (double)pe[sb];
        }
        const double ps = wave_sum(sub == 0 ? pl : 0.0);  // (a key's four lanes hold one P)
        l = l * (double)alpha + ps;
        m = mn;
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = o[e] * alpha;
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
            const float pj = pe[sb] * f1_scale(cur.vs, sb, blk);  // (P 2^s: exact)
            const uint32_t vw[4] = {cur.v[sb].x, cur.v[sb].y, cur.v[sb].z, cur.v[sb].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const auto f0 = __builtin_amdgcn_cvt_pk_f32_fp8(vw[i], false);
                const auto f1 = __builtin_amdgcn_cvt_pk_f32_fp8(vw[i], true);
                o[4 * i] += pj * f0[0];
                o[4 * i + 1] += pj * f0[1];
                o[4 * i + 2] += pj * f1[0];
                o[4 * i + 3] += pj * f1[1];
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {  // over the wave's lanes of the same sub (xor 4 behind xor 8: see wmi_device.h)
        float v = xstep<XSum, 8>(o[e]);
        v = xstep<XSum, 4>(v);
        v = xstep<XSum, 16>(v);
        o[e] = xstep<XSum, 32>(v);
    }
    if (lane < 4) {
        if (lane == 0) { mrg[w][0] = m; mrg[w][1] = (float)l; }
#pragma unroll
        for (int e = 0; e < 16; ++e) mrg[w][2 + lane * 16 + e] = o[e];
    }
    __syncthreads();
    if (tid < 64) {  // head dim tid of the chunk's partial (wave 0 has the chunk's first key: M is finite)
        float M = mrg[0][0];
#pragma unroll
        for (int i = 1; i < F1_WAVES; ++i) M = fmaxf(M, mrg[i][0]);
        float L = 0.0f, od = 0.0f;
#pragma unroll
        for (int i = 0; i < F1_WAVES; ++i) {
            const float wgt = mrg[i][0] == -INFINITY ? 0.0f : expf(mrg[i][0] - M);
            L += mrg[i][1] * wgt;
            od += mrg[i][2 + tid] * wgt;
        }
        float *dst = a.part + (((int64_t)c * a.H + h) * a.chunks + ch) * 16 * WD_PART;
        if (tid == 0) { dst[0] = M; dst[1] = L; }
        dst[2 + tid] = od;
    }
}

namespace {

bool f8_args_ok(const WdCrossF8Args &fa) {
    const WdCrossArgs &a = fa.a;
    return fa.K8 && fa.V8 && fa.Ksc && fa.Vsc && a.T >= 1 && fa.Tp == f8_tp(a.T) && a.n == a.H * 64 && a.chunks >= 1 &&
           a.tiles >= 1 && (int64_t)a.chunks * a.tiles * F8_CK >= a.T && (int64_t)(a.chunks - 1) * a.tiles * F8_CK < a.T;
}

}  // namespace

hipError_t launch_wd_cross_attn1_f8(hipStream_t s, const WdCrossF8Args &fa) {
    const WdCrossArgs &a = fa.a;
    if (a.B < 1 || a.B > WD_ROWS || a.Kb != 1 || !f8_args_ok(fa)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_cross_attn1_f8, dim3(a.chunks, a.H, a.B), dim3(64 * F1_WAVES), 0, s, fa);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wd_cross_combine(s, a);
}

// ---- K >= 2: a recording's hypotheses as the MFMA's query columns ------------------------
__global__ __launch_bounds__(128) void k_wd_cross_attn_f8(WdCrossF8Args fa) {
    __shared__ __attribute__((aligned(16))) f16 Ks[F8_CK * F8_KLD];
    __shared__ __attribute__((aligned(16))) f16 Vt[64 * F8_VLD];
    __shared__ float mrg[16][WD_PART];
    const WdCrossArgs &a = fa.a;
    const int ch = blockIdx.x, h = blockIdx.y, c = blockIdx.z;
    if (a.tb.bs[c].done) return;  // (uniform; k_wd_cross_combine writes its rows' zeros)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lq = lane & 15, g = lane >> 4;
    const int n = a.n, T = a.T;
    int clip = a.tb.recs[c].clip;
    clip = clip < 0 ? 0 : clip;
    const uint8_t *Kc = fa.K8 + (int64_t)clip * T * n + h * 64, *Vc = fa.V8 + (int64_t)clip * T * n + h * 64;
    const int64_t so = (int64_t)clip * f8_scale_plane_bytes(T, n) + (int64_t)h * fa.Tp * 2;
    const uint8_t *Ksc = fa.Ksc + so, *Vsc = fa.Vsc + so;
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
        const int key0 = (ch * a.tiles + t) * F8_CK;
        if (key0 >= T) break;  // (uniform)
        for (int i = tid; i < F8_CK * 4; i += 128) {
            const int key = i >> 2, part = i & 3;  // 16 bytes: half of scale block part >> 1
            uint4 kb = make_uint4(0u, 0u, 0u, 0u), vb = kb;  // (keys past T: zero rows, masked below)
            float ksc = 1.0f, vsc = 1.0f;
            if (key0 + key < T) {
                kb = *(const uint4 *)(Kc + (int64_t)(key0 + key) * n + part * 16);
                vb = *(const uint4 *)(Vc + (int64_t)(key0 + key) * n + part * 16);
                ksc = f8_exp2(Ksc[(int64_t)(key0 + key) * 2 + (part >> 1)]);
                vsc = f8_exp2(Vsc[(int64_t)(key0 + key) * 2 + (part >> 1)]);
            }
            half8 lo, hi;
            f8_render16(kb, ksc, lo, hi);
            *(half8 *)(Ks + key * F8_KLD + part * 16) = lo;
            *(half8 *)(Ks + key * F8_KLD + part * 16 + 8) = hi;
            f8_render16(vb, vsc, lo, hi);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                Vt[(part * 16 + e) * F8_VLD + key] = lo[e];
                Vt[(part * 16 + 8 + e) * F8_VLD + key] = hi[e];
            }
        }
        __syncthreads();
        if (key0 + 32 * w < T) {  // (uniform over the wave: it has a key below T)
            floatx4 S[2];
            float tm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                floatx4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {  // (an MFMA k-slice of 32 is one scale block)
                    const half8 kf = *(const half8 *)(Ks + (32 * w + 16 * kt + lq) * F8_KLD + ks * 32 + g * 8);
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
                const f16 *vr = Vt + (dt * 16 + lq) * F8_VLD + 32 * w + 4 * g;
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

hipError_t launch_wd_cross_attn_f8(hipStream_t s, const WdCrossF8Args &fa) {
    const WdCrossArgs &a = fa.a;
    if (a.B < 1 || a.Kb < 1 || a.Kb > BEAM_MAX || a.B * a.Kb > WD_ROWS || !f8_args_ok(fa)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wd_cross_attn_f8, dim3(a.chunks, a.H, a.B), dim3(128), 0, s, fa);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wd_cross_combine(s, a);
}

}  // namespace wmi
