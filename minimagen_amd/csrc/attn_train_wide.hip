// Training path of the wide presets' attention (Unet() default, Base, Super; dim_head 64): the core softmax(q k^T) v of the multi-query
// Attention (layers.py:52-104, one k / v head) and of the unfolded CrossAttention (layers.py:220-251, a k / v head per head) forward and backward
// without the [queries x context] score tensor.  q [B][n][H*64] token-major, k / v [B][J][KVH*64] (the null row and any context rows already
// concatenated by the caller), an optional key mask [B][J].
//   mi_flash_attn_train_fwd   flash_kv_prep_kernel + flash_attn_mq_kernel<..., TRAIN> (flash_wide.hip.h): the inference kernel, which also
//                             writes lse[B][H][n] (log2 domain); unmasked, its output is mi_flash_attn_fwd's to the bit
//   mi_flash_attn_train_bwd   FlashAttention-2 structure, deterministic:
//     flash_bwd_dsum_kernel   D_i = dO_i . O_i per (query, head)
//     flash_bwd_dq_kernel     a workgroup = 64 queries x 2 heads (multi-query) or 128 queries of one head: walks the K / V chunks (prepared operand
//                             images streamed to LDS by LDS-DMA, double-buffered); S = q k^T and dP = dO v^T recomputed, P = exp2(S - lse),
//                             dS = P (dP - D), dq += dS k
//     flash_bwd_dkv_kernel    a workgroup = one 64-row K / V chunk of one (image, k / v head, query split): walks the split's queries in blocks of 64
//                             for EVERY head that reads this k / v head (all H in the multi-query form), dv += P^T dO, dk += dS^T q
//     flash_bwd_reduce_kernel the query splits' dk / dv partials added in split order (no float atomics: reruns are bit-equal)
// Every product is the forward's 3-term fp16 split (lo*hi + hi*lo + hi*hi, fp32 accumulation) with power-of-two block scales: K / V per 64-row chunk
// (the forward's prepared images: [K | V^T] and, prepared from (v, k), [V | K^T]), q and dO per 16-query tile (dq) or 64-query block (dk / dv),
// P unscaled (in [0, 1]), dS per tile from its own maximum.  Softmax, exp2 and all accumulators are fp32.
#include "common.hip.h"
#include <type_traits>
#include <cstdlib>

namespace {

#include "flash_wide.hip.h"

constexpr float FB_LN2 = 0.69314718055994530942f;
constexpr int FB_CHUNK16 = 6 * FW_PL;          // the dq kernel's LDS image of a chunk: [K hi | K lo] of the forward image + [V hi | V lo | K^T hi | K^T lo]

struct fb_args {
    int B, n, H, KVH, J, nchunk, nsplit, qblk_per_split;
    const float* q; const float* dout; const float* out;
    const uint8_t* mask; const float* lse; float* dsum;
    const uint4* imgA; const uint4* imgB;       // [K | V^T] and [V | K^T] images of every (b, k / v head, chunk), exponents after them
    float* dq; float* dk; float* dv;            // dk / dv: the final tensors (nsplit == 1) or the partials [nsplit][B][J][KVH * 64]
    float q_scale;                              // softmax scale * log2(e)
};

__device__ __forceinline__ const int* fb_exps(const uint4* img, const fb_args& a) {
    return reinterpret_cast<const int*>(img + (size_t)a.B * a.KVH * a.nchunk * FW_CHUNK16);
}
__device__ __forceinline__ bool fb_live(const fb_args& a, int b, int j) {
    return j < a.J && (a.mask == nullptr || a.mask[(size_t)b * a.J + j] != 0);
}
// three-term product of one 16 x 16 x 32 step: acc += A_lo B_hi + A_hi B_lo + A_hi B_hi
__device__ __forceinline__ f32x4 fb_mma3(const fw_f16x8 ah, const fw_f16x8 al, const fw_f16x8 bh, const fw_f16x8 bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}
__device__ __forceinline__ fw_f16x8 fb_frag(const uint4* p) { return __builtin_bit_cast(fw_f16x8, *p); }
// a lane's eight values of a 16 x 64 row block as the B operand (dims 32 hf + 8 lg + e of row `row`), times `scale`; zeros for row < 0
__device__ __forceinline__ void fb_rowfrag(const float* row, float scale, int lg, float (&v)[2][8], float& mx) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (row) { x = *reinterpret_cast<const float4*>(row + 32 * hf + 8 * lg); y = *reinterpret_cast<const float4*>(row + 32 * hf + 8 * lg + 4); }
        const float w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[hf][e] = w[e] * scale; mx = fmaxf(mx, fabsf(v[hf][e])); }
    }
}
__device__ __forceinline__ void fb_split_rows(float (&v)[2][8], int ex, fw_f16x8 (&hi)[2], fw_f16x8 (&lo)[2]) {
    const float s = ldexpf(1.0f, ex);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = v[hf][e] * s;
        uint4 h4, l4;
        fw_split8(w, h4, l4);
        hi[hf] = __builtin_bit_cast(fw_f16x8, h4);
        lo[hf] = __builtin_bit_cast(fw_f16x8, l4);
    }
}

// D[b][h][i] = sum_d dO . O: 16 lanes per (query, head) row, a float4 each
__global__ __launch_bounds__(256) void flash_bwd_dsum_kernel(const fb_args a) {
    const long long rows = (long long)a.B * a.n * a.H;
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const long long rc = row < rows ? row : rows - 1;
    const float4 o = *reinterpret_cast<const float4*>(a.out + rc * 64 + 4 * l), d = *reinterpret_cast<const float4*>(a.dout + rc * 64 + 4 * l);
    float s = o.x * d.x + o.y * d.y + o.z * d.z + o.w * d.w;
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (row < rows && l == 0) {
        const int h = (int)(row % a.H), i = (int)((row / a.H) % a.n), b = (int)(row / ((long long)a.H * a.n));
        a.dsum[((size_t)b * a.H + h) * a.n + i] = s;
    }
}

// dq.  A wave = 16 queries of one head.  Scores as the forward's S^T = K Q^T (a query's scores in one lane + the three lanes 16 apart), dP^T =
// V dO^T the same way; dS^T in that C/D layout is the B operand of dq^T += K^T dS^T for a PAIR of score tiles (K^T staged with permuted context
// rows, as V^T in the forward), so no score moves between lanes.
template <bool PERHEAD>
__global__ __launch_bounds__(512) void flash_bwd_dq_kernel(const fb_args a) {
    constexpr int NW = 8, NH = PERHEAD ? 1 : 2;
    __shared__ __attribute__((aligned(16))) uint4 kv[2][FB_CHUNK16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, lg = lane >> 4;
    const int h = PERHEAD ? (int)blockIdx.y : (int)blockIdx.y * NH + (wave >> 2), b = blockIdx.z;
    const int kvh = a.KVH == 1 ? 0 : h;
    const int tok = (PERHEAD ? (int)blockIdx.x * NW + wave : (int)blockIdx.x * 4 + (wave & 3)) * 16 + lq;
    const bool ok = tok < a.n;
    const int inner = a.H * 64;
    const size_t img0 = ((size_t)b * a.KVH + kvh) * a.nchunk;
    const uint4* const srcA = a.imgA + img0 * FW_CHUNK16;
    const uint4* const srcB = a.imgB + img0 * FW_CHUNK16;
    const int* const exps = fb_exps(a.imgA, a) + img0 * 2;
    auto issue_chunk = [&](int c, int buf) {
        for (int r = wave; r < FB_CHUNK16 / 64; r += NW) {           // 1 KB rows: 16 of [K hi | K lo] from image A, 32 of image B
            const uint4* src = (r < 16 ? srcA + (size_t)c * FW_CHUNK16 + r * 64 : srcB + (size_t)c * FW_CHUNK16 + (r - 16) * 64) + lane;
#if defined(HIPEMU)
            kv[buf][r * 64 + lane] = *src;
#else
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)&kv[buf][r * 64], 16, 0, 0);
#endif
        }
    };
    issue_chunk(0, 0);
    // q (times q_scale) and dO of this lane's query as B operands, each block-scaled per 16-query tile
    fw_f16x8 qh[2], ql[2], oh[2], ol[2];
    int eq, eo;
    {
        const size_t ro = ((size_t)b * a.n + (ok ? tok : a.n - 1)) * inner + h * 64;
        float v[2][8];
        float mq = 0.0f, mo = 0.0f;
        fb_rowfrag(a.q + ro, a.q_scale, lg, v, mq);
        eq = fw_scale_exp(mi_wave_max(mq));
        fb_split_rows(v, eq, qh, ql);
        fb_rowfrag(ok ? a.dout + ro : nullptr, 1.0f, lg, v, mo);
        eo = fw_scale_exp(mi_wave_max(mo));
        fb_split_rows(v, eo, oh, ol);
    }
    const float lse = ok ? a.lse[((size_t)b * a.H + h) * a.n + tok] : INFINITY;       // +inf: P = 0 for the padding queries
    const float dsum = ok ? a.dsum[((size_t)b * a.H + h) * a.n + tok] : 0.0f;
    f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.nchunk; ++c) {
        const int buf = c & 1, j0 = 64 * c;
#if !defined(HIPEMU)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        __syncthreads();
        if (c + 1 < a.nchunk) issue_chunk(c + 1, buf ^ 1);
        const uint4* const KH = kv[buf], * const KL = KH + FW_PL, * const VH = KH + 2 * FW_PL, * const VL = KH + 3 * FW_PL;
        const uint4* const TH = KH + 4 * FW_PL, * const TL = KH + 5 * FW_PL;
        const int ek = exps[2 * c], ev = exps[2 * c + 1];
        f32x4 s[4], dp[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            s[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            dp[jt] = s[jt];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int ix = (4 * hf + lg) * 64 + 16 * jt + lq;
                s[jt] = fb_mma3(fb_frag(KH + ix), fb_frag(KL + ix), qh[hf], ql[hf], s[jt]);
                dp[jt] = fb_mma3(fb_frag(VH + ix), fb_frag(VL + ix), oh[hf], ol[hf], dp[jt]);
            }
        }
        const float us = ldexpf(1.0f, -(ek + eq)), ud = ldexpf(1.0f, -(ev + eo));
        float ds[4][4];
        float md = 0.0f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = fb_live(a, b, j0 + 16 * jt + 4 * lg + r);
                const float pv = live ? __builtin_amdgcn_exp2f(fmaf(s[jt][r], us, -lse)) : 0.0f;
                ds[jt][r] = pv * fmaf(dp[jt][r], ud, -dsum);
                md = fmaxf(md, fabsf(ds[jt][r]));
            }
        const int ed = fw_scale_exp(mi_wave_max(md));
        const float sd = ldexpf(1.0f, ed), ug = ldexpf(1.0f, -(ek + ed));
        fw_f16x8 dh[2], dl[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            float w[8];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) w[4 * u + r] = ds[2 * hf + u][r] * sd;
            uint4 h4, l4;
            fw_split8(w, h4, l4);
            dh[hf] = __builtin_bit_cast(fw_f16x8, h4);
            dl[hf] = __builtin_bit_cast(fw_f16x8, l4);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            f32x4 sl = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int ix = (4 * hf + lg) * 64 + 16 * dt + lq;
                sl = fb_mma3(fb_frag(TH + ix), fb_frag(TL + ix), dh[hf], dl[hf], sl);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[dt][r] = fmaf(sl[r], ug, acc[dt][r]);
        }
    }
    if (ok) {
        const float g = a.q_scale * FB_LN2;                  // the natural-units softmax scale
        float* row = a.dq + ((size_t)b * a.n + tok) * inner + h * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<float4*>(row + 16 * dt + 4 * lg) = make_float4(acc[dt][0] * g, acc[dt][1] * g, acc[dt][2] * g, acc[dt][3] * g);
    }
}

// dk / dv.  A wave = 16 context rows j of the chunk, their k and v (the forward's block-scaled split values, read from the two images) held as
// B operands.  Per 64-query block and head: q (times q_scale) and dO staged in LDS twice -- rows (A operand of S = Q K^T, dP = dO V^T) and
// transposed with the queries of each 32-query half permuted (A operand of dv^T += dO^T P, dk^T += Q^T dS, the pair trick of the forward)
// -- block-scaled per 64-query block.
__global__ __launch_bounds__(256) void flash_bwd_dkv_kernel(const fb_args a) {
    constexpr int EPT = 16, PPR = 4;
    __shared__ __attribute__((aligned(16))) uint4 st[8 * FW_PL];          // Q hi | Q lo | dO hi | dO lo | Q^T hi | Q^T lo | dO^T hi | dO^T lo
    __shared__ float s_lse[64], s_dsum[64], smax[2][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, lg = lane >> 4;
    const int c = blockIdx.x, kvh = (int)blockIdx.y % a.KVH, b = (int)blockIdx.y / a.KVH, split = blockIdx.z;
    const int j = 64 * c + 16 * wave + lq;
    const bool jlive = fb_live(a, b, j);
    const int inner = a.H * 64, kvw = a.KVH * 64;
    const size_t img_i = ((size_t)b * a.KVH + kvh) * a.nchunk + c;
    fw_f16x8 kh[2], kl[2], vh[2], vl[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int ix = (4 * hf + lg) * 64 + 16 * wave + lq;
        kh[hf] = fb_frag(a.imgA + img_i * FW_CHUNK16 + ix); kl[hf] = fb_frag(a.imgA + img_i * FW_CHUNK16 + FW_PL + ix);
        vh[hf] = fb_frag(a.imgB + img_i * FW_CHUNK16 + ix); vl[hf] = fb_frag(a.imgB + img_i * FW_CHUNK16 + FW_PL + ix);
    }
    const int ek = fb_exps(a.imgA, a)[img_i * 2], ev = fb_exps(a.imgA, a)[img_i * 2 + 1];
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
    // staging role: work-item -> (query row of the block, 16 head dims); the row's position in the permuted order of the transposed arrays
    const int srow = tid / PPR, sd0 = (tid % PPR) * EPT;
    const int spos = (srow & 32) | (((srow >> 2) & 3) << 3) | (((srow >> 4) & 1) << 2) | (srow & 3);
    const int qb0 = split * a.qblk_per_split, nqb = (a.n + 63) / 64, qb1 = qb0 + a.qblk_per_split < nqb ? qb0 + a.qblk_per_split : nqb;
    const int h0 = a.KVH == 1 ? 0 : kvh, h1 = a.KVH == 1 ? a.H : kvh + 1;
    for (int qb = qb0; qb < qb1; ++qb)
        for (int h = h0; h < h1; ++h) {
            const int i = 64 * qb + srow;
            const bool iok = i < a.n;
            float qf[EPT], of[EPT];
            {
                const float* qr = a.q + ((size_t)b * a.n + i) * inner + h * 64 + sd0;
                const float* orow = a.dout + ((size_t)b * a.n + i) * inner + h * 64 + sd0;
#pragma unroll
                for (int e = 0; e < EPT; e += 4) {
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
                    if (iok) { x = *reinterpret_cast<const float4*>(qr + e); y = *reinterpret_cast<const float4*>(orow + e); }
                    qf[e] = x.x * a.q_scale; qf[e + 1] = x.y * a.q_scale; qf[e + 2] = x.z * a.q_scale; qf[e + 3] = x.w * a.q_scale;
                    of[e] = y.x; of[e + 1] = y.y; of[e + 2] = y.z; of[e + 3] = y.w;
                }
            }
            float mq = 0.0f, mo = 0.0f;
#pragma unroll
            for (int e = 0; e < EPT; ++e) { mq = fmaxf(mq, fabsf(qf[e])); mo = fmaxf(mo, fabsf(of[e])); }
            mq = mi_wave_max(mq); mo = mi_wave_max(mo);
            __syncthreads();                          // the previous block's operands are no longer read
            if (lane == 0) { smax[0][wave] = mq; smax[1][wave] = mo; }
            if (sd0 == 0) {
                s_lse[srow] = iok ? a.lse[((size_t)b * a.H + h) * a.n + i] : INFINITY;
                s_dsum[srow] = iok ? a.dsum[((size_t)b * a.H + h) * a.n + i] : 0.0f;
            }
            __syncthreads();
            const int eq = fw_scale_exp(fmaxf(fmaxf(smax[0][0], smax[0][1]), fmaxf(smax[0][2], smax[0][3])));
            const int eo = fw_scale_exp(fmaxf(fmaxf(smax[1][0], smax[1][1]), fmaxf(smax[1][2], smax[1][3])));
            {
                const float sq = ldexpf(1.0f, eq), so = ldexpf(1.0f, eo);
                _Float16* const base = reinterpret_cast<_Float16*>(st);
#pragma unroll
                for (int arr = 0; arr < 2; ++arr) {
                    const float* x = arr == 0 ? qf : of;
                    const float sc = arr == 0 ? sq : so;
                    _Float16* const rh = base + (size_t)(2 * arr) * FW_PL * 8;          // rows: [octet of d][row] chunks
                    _Float16* const rl = rh + FW_PL * 8;
                    _Float16* const th = base + (size_t)(4 + 2 * arr) * FW_PL * 8;      // transposed: [octet of the permuted row][d] chunks
                    _Float16* const tl = th + FW_PL * 8;
#pragma unroll
                    for (int e = 0; e < EPT; e += 4) {
                        unsigned hb[2], lb[2];
#pragma unroll
                        for (int q2 = 0; q2 < 2; ++q2) {
                            const float x0 = x[e + 2 * q2] * sc, x1 = x[e + 2 * q2 + 1] * sc;
                            const mi_f16x2 h2 = {(_Float16)x0, (_Float16)x1};
                            hb[q2] = __builtin_bit_cast(unsigned, h2);
                            lb[q2] = mi_split_lo2(hb[q2], x0, x1);
                        }
                        const int ko = ((((sd0 + e) >> 3) * 64 + srow) << 3) + ((sd0 + e) & 7);
                        *reinterpret_cast<uint2*>(rh + ko) = make_uint2(hb[0], hb[1]);
                        *reinterpret_cast<uint2*>(rl + ko) = make_uint2(lb[0], lb[1]);
                    }
#pragma unroll
                    for (int e = 0; e < EPT; ++e) {
                        const float xv = x[e] * sc;
                        const _Float16 hi = (_Float16)xv, lo = (_Float16)(xv - (float)hi);
                        const int vo = (((spos >> 3) * 64 + sd0 + e) << 3) + (spos & 7);
                        th[vo] = hi;
                        tl[vo] = lo;
                    }
                }
            }
            __syncthreads();
            const uint4* const QH = st, * const QL = st + FW_PL, * const OH = st + 2 * FW_PL, * const OL = st + 3 * FW_PL;
            const uint4* const QTH = st + 4 * FW_PL, * const QTL = st + 5 * FW_PL, * const OTH = st + 6 * FW_PL, * const OTL = st + 7 * FW_PL;
            // S[i][j] and dP[i][j] for the block's 64 queries (rows 16 it + 4 lg + r) x this lane's context row j (column lq)
            const float us = ldexpf(1.0f, -(ek + eq)), ud = ldexpf(1.0f, -(ev + eo));
            float pv[4][4], ds[4][4];
            float md = 0.0f;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int ix = (4 * hf + lg) * 64 + 16 * it + lq;
                    s = fb_mma3(fb_frag(QH + ix), fb_frag(QL + ix), kh[hf], kl[hf], s);
                    dp = fb_mma3(fb_frag(OH + ix), fb_frag(OL + ix), vh[hf], vl[hf], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ii = 16 * it + 4 * lg + r;
                    pv[it][r] = jlive ? __builtin_amdgcn_exp2f(fmaf(s[r], us, -s_lse[ii])) : 0.0f;
                    ds[it][r] = pv[it][r] * fmaf(dp[r], ud, -s_dsum[ii]);
                    md = fmaxf(md, fabsf(ds[it][r]));
                }
            }
            const int ed = fw_scale_exp(mi_wave_max(md));
            const float sd = ldexpf(1.0f, ed);
            fw_f16x8 ph[2], pl[2], dh[2], dl[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float w[8], z[8];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { w[4 * u + r] = pv[2 * hf + u][r]; z[4 * u + r] = ds[2 * hf + u][r] * sd; }
                uint4 h4, l4;
                fw_split8(w, h4, l4);
                ph[hf] = __builtin_bit_cast(fw_f16x8, h4);
                pl[hf] = __builtin_bit_cast(fw_f16x8, l4);
                fw_split8(z, h4, l4);
                dh[hf] = __builtin_bit_cast(fw_f16x8, h4);
                dl[hf] = __builtin_bit_cast(fw_f16x8, l4);
            }
            const float uo = ldexpf(1.0f, -eo), ug = ldexpf(1.0f, -(eq + ed));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, sk = sv;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int ix = (4 * hf + lg) * 64 + 16 * dt + lq;
                    sv = fb_mma3(fb_frag(OTH + ix), fb_frag(OTL + ix), ph[hf], pl[hf], sv);
                    sk = fb_mma3(fb_frag(QTH + ix), fb_frag(QTL + ix), dh[hf], dl[hf], sk);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { dv[dt][r] = fmaf(sv[r], uo, dv[dt][r]); dk[dt][r] = fmaf(sk[r], ug, dk[dt][r]); }
            }
        }
    if (j < a.J) {
        const size_t o = (a.nsplit > 1 ? (size_t)split * a.B * a.J * kvw : 0) + ((size_t)b * a.J + j) * kvw + kvh * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            *reinterpret_cast<float4*>(a.dk + o + 16 * dt + 4 * lg) = make_float4(dk[dt][0] * FB_LN2, dk[dt][1] * FB_LN2, dk[dt][2] * FB_LN2, dk[dt][3] * FB_LN2);
            *reinterpret_cast<float4*>(a.dv + o + 16 * dt + 4 * lg) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
        }
    }
}

// out[e] = sum over s (in order) of part[s][e], e over float4s
__global__ __launch_bounds__(256) void flash_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long long n4, int nsplit) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const float4* p = reinterpret_cast<const float4*>(part);
    float4 s = p[e];
    for (int k = 1; k < nsplit; ++k) {
        const float4 x = p[(size_t)k * n4 + e];
        s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
    }
    reinterpret_cast<float4*>(out)[e] = s;
}

long long fb_align(long long x) { return (x + 255) & ~255LL; }

// query splits of the dk / dv kernel: enough workgroups to fill the GPU (>= 1024), at least 256 queries per split
int fb_nsplit(int B, int n, int kv_heads, int J) {
    const long long base = (long long)((J + 63) / 64) * B * kv_heads;
    long long s = (1024 + base - 1) / base;
    const long long most = (n + 255) / 256;
    if (s > most) s = most;
    return s < 1 ? 1 : (int)s;
}

int fb_check(const mi_flash_attn_train_params* p, const char* who, int backward) {
    if (p->B <= 0 || p->n <= 0 || p->heads <= 0 || p->J <= 0 || (p->kv_heads != 1 && p->kv_heads != p->heads)) { mi_set_error("%s: bad shape", who); return MI_ERR_INVALID; }
    if (!p->q || !p->k || !p->v || !p->out || !p->lse || !p->work) { mi_set_error("%s: missing tensor", who); return MI_ERR_INVALID; }
    if (backward && (!p->dout || !p->dq || !p->dk || !p->dv)) { mi_set_error("%s: missing gradient tensor", who); return MI_ERR_INVALID; }
    if (p->work_bytes < mi_flash_attn_train_workspace(p->B, p->n, p->heads, p->kv_heads, p->J, backward)) { mi_set_error("%s: workspace too small", who); return MI_ERR_INVALID; }
    return MI_OK;
}

// the prepared image of (k0, v0) = (first, second) into `img`
void fb_prep(const mi_flash_attn_train_params* t, const float* first, const float* second, void* img, hipStream_t stream) {
    mi_flash_attn_params p{};
    p.B = t->B; p.HW = t->n; p.heads = t->heads; p.kv_heads = t->kv_heads;
    p.k0 = first; p.v0 = second; p.n0 = t->J; p.ld0 = t->kv_heads * 64; p.bs0 = (long long)t->J * p.ld0;
    p.kv_prep = img;
    const int nchunk = (t->J + 63) / 64;
    hipLaunchKernelGGL(flash_kv_prep_kernel, dim3(nchunk, t->kv_heads, t->B), dim3(256), 0, stream, p, nchunk);
}

}  // namespace

extern "C" long long mi_flash_attn_train_workspace(int B, int n, int heads, int kv_heads, int J, int backward) {
    const long long img = fb_align(mi_flash_kv_prep_bytes(B * kv_heads, J));
    if (!backward) return img;
    long long bytes = 2 * img + fb_align((long long)B * heads * n * 4);
    const int ns = fb_nsplit(B, n, kv_heads, J);
    if (ns > 1) bytes += 2 * fb_align((long long)ns * B * J * kv_heads * 64 * 4);
    return bytes;
}

extern "C" int mi_flash_attn_train_fwd(const mi_flash_attn_train_params* t, void* stream) {
    if (int rc = fb_check(t, "mi_flash_attn_train_fwd", 0)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    fb_prep(t, t->k, t->v, t->work, s);
    mi_flash_attn_params p{};
    p.B = t->B; p.HW = t->n; p.heads = t->heads; p.kv_heads = t->kv_heads; p.q = t->q; p.q_scale = t->q_scale;
    p.k0 = t->k; p.v0 = t->v; p.n0 = t->J; p.ld0 = t->kv_heads * 64; p.bs0 = (long long)t->J * p.ld0; p.out = t->out;
    p.kv_prep = t->work; p.kv_prep_bytes = t->work_bytes;
    const int nchunk = (t->J + 63) / 64;
    const fw_train_ext ext{t->mask, t->lse};
    if (t->kv_heads == 1 && (t->heads & 3) == 0)        // mi_flash_attn_fwd's launch forms, so that the output is the same to the bit
        hipLaunchKernelGGL(HIP_KERNEL_NAME(flash_attn_mq_kernel<8, 2, 2, false, true>), dim3((t->n + 63) / 64, t->heads / 4, t->B), dim3(512), 0, s, p, nchunk, ext);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(flash_attn_mq_kernel<8, 2, 2, true, true>), dim3((t->n + 255) / 256, t->heads, t->B), dim3(512), 0, s, p, nchunk, ext);
    return mi_check_launch("mi_flash_attn_train_fwd");
}

extern "C" int mi_flash_attn_train_bwd(const mi_flash_attn_train_params* t, void* stream) {
    if (int rc = fb_check(t, "mi_flash_attn_train_bwd", 1)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const long long img = fb_align(mi_flash_kv_prep_bytes(t->B * t->kv_heads, t->J));
    char* w = static_cast<char*>(t->work);
    fb_args a{};
    a.B = t->B; a.n = t->n; a.H = t->heads; a.KVH = t->kv_heads; a.J = t->J; a.nchunk = (t->J + 63) / 64;
    a.nsplit = fb_nsplit(t->B, t->n, t->kv_heads, t->J);
    const int nqb = (t->n + 63) / 64;
    a.qblk_per_split = (nqb + a.nsplit - 1) / a.nsplit;
    a.q = t->q; a.dout = t->dout; a.out = t->out; a.mask = t->mask; a.lse = t->lse; a.q_scale = t->q_scale;
    a.imgA = reinterpret_cast<const uint4*>(w);
    a.imgB = reinterpret_cast<const uint4*>(w + img);
    a.dsum = reinterpret_cast<float*>(w + 2 * img);
    const long long pbytes = fb_align((long long)a.nsplit * t->B * t->J * t->kv_heads * 64 * 4);
    float* pk = reinterpret_cast<float*>(w + 2 * img + fb_align((long long)t->B * t->heads * t->n * 4));
    a.dq = t->dq;
    a.dk = a.nsplit > 1 ? pk : t->dk;
    a.dv = a.nsplit > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(pk) + pbytes) : t->dv;
    fb_prep(t, t->k, t->v, w, s);                      // [K | V^T]: the forward's image
    fb_prep(t, t->v, t->k, w + img, s);                // [V | K^T]
    const long long rows = (long long)t->B * t->n * t->heads;
    hipLaunchKernelGGL(flash_bwd_dsum_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, a);
    if (t->kv_heads == 1 && (t->heads & 1) == 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(flash_bwd_dq_kernel<false>), dim3(nqb, t->heads / 2, t->B), dim3(512), 0, s, a);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(flash_bwd_dq_kernel<true>), dim3((t->n + 127) / 128, t->heads, t->B), dim3(512), 0, s, a);
    hipLaunchKernelGGL(flash_bwd_dkv_kernel, dim3(a.nchunk, t->B * t->kv_heads, a.nsplit), dim3(256), 0, s, a);
    if (a.nsplit > 1) {
        const long long n4 = (long long)t->B * t->J * t->kv_heads * 16;
        hipLaunchKernelGGL(flash_bwd_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.dk, t->dk, n4, a.nsplit);
        hipLaunchKernelGGL(flash_bwd_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.dv, t->dv, n4, a.nsplit);
    }
    return mi_check_launch("mi_flash_attn_train_bwd");
}
