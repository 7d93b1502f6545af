// Shared by attention_wide.hip (inference) and attn_train_wide.hip (training): the 3-term fp16-split helpers of the wide flash attention,
// the K / V operand-image preparation and the prepared-K/V flash kernel (flash_attn_mq_kernel; TRAIN = true also saves the logsumexp and
// takes a key mask).  Included inside an anonymous namespace by both sources.
// (needs common.hip.h and <type_traits> in front)
#pragma once

typedef _Float16 fw_f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ int fw_scale_exp(float m) {           // k with m * 2^k in [128, 256); 0 for zero / non-finite input
    const int be = (int)((__float_as_uint(m) & 0x7fffffffu) >> 23);
    return (be == 0 || be == 255) ? 0 : 134 - be;
}
__device__ __forceinline__ void fw_split8(const float (&x)[8], uint4& hi, uint4& lo) {
    unsigned h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const mi_f16x2 h2 = {(_Float16)x[2 * e], (_Float16)x[2 * e + 1]};
        h[e] = __builtin_bit_cast(unsigned, h2);
        l[e] = mi_split_lo2(h[e], x[2 * e], x[2 * e + 1]);
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

// ---- multi-query attention with the K / V operands prepared ONCE per launch (p.kv_prep): flash_kv_prep_kernel splits, scales and transposes
// every 64-row context chunk into the operand image the matrix loop reads -- flash_attn_f16x3_kernel's values, octet-major (below): [K hi | K lo | V^T hi | V^T lo], 4 x 8 x 64
// 16-byte chunks, plus the chunk's two block-scaling exponents -- and flash_attn_mq_kernel copies a chunk global -> LDS by LDS-DMA into a
// double buffer, the next chunk under the current one's matrix work, one barrier per chunk.  In the staged form every workgroup (64 queries)
// re-did that preparation for all 65 chunks of a 4096-token context: two reductions, the split, 2-byte scattered LDS writes and three barriers
// per chunk, 64 times per image -- 11.5 us per chunk and workgroup against ~3 us of LDS reads + matrix work.  Same arithmetic, same bits.
// the prepared image of a 64-row chunk: four operand arrays [K hi | K lo | V^T hi | V^T lo], each [octet of the contracted index 8][row 64] 16-byte chunks
// (octet-major: the lanes of two neighbouring octets that a ds_read_b128 serves together -- {0-3, 12-15, 20-27}, ... -- then fall on disjoint banks;
// the row-major pitch-9 layout of the self-staging kernel is a 2-way conflict on this machine's lane groups: 46 % of the LDS cycles, PMC)
constexpr int FW_PL = 8 * 64, FW_CHUNK16 = 4 * FW_PL;          // 16-byte chunks per array / per prepared context chunk (32 768 bytes)

__global__ __launch_bounds__(256) void flash_kv_prep_kernel(const mi_flash_attn_params p, const int nchunk) {
    constexpr int EPT = 16, PPR = 4;
    __shared__ __attribute__((aligned(16))) uint4 img[FW_CHUNK16];          // KsH | KsL | VtH | VtL
    __shared__ float smax[2][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, j0 = 64 * c;       // kvh: which k / v head (0 for the multi-query form)
    const int KVH = gridDim.y;
    const int nnull = p.null_k ? 1 : 0, J = nnull + p.n0 + p.n1;
    const int srow = tid / PPR, sd0 = (tid % PPR) * EPT;
    const int spos = (srow & 32) | (((srow >> 2) & 3) << 3) | (((srow >> 4) & 1) << 2) | (srow & 3);
    float kf[EPT], vf[EPT];
    {
        const int jj = j0 + srow;
        const float* ksrc = nullptr;
        const float* vsrc = nullptr;
        if (jj < J) {
            if (jj < nnull) { ksrc = p.null_k; vsrc = p.null_v; }
            else if (jj - nnull < p.n0) { const size_t o_ = (size_t)b * p.bs0 + (size_t)(jj - nnull) * p.ld0 + kvh * 64; ksrc = p.k0 + o_; vsrc = p.v0 + o_; }
            else { const size_t o_ = (size_t)b * p.bs1 + (size_t)(jj - nnull - p.n0) * p.ld1 + kvh * 64; ksrc = p.k1 + o_; vsrc = p.v1 + o_; }
        }
#pragma unroll
        for (int e = 0; e < EPT; e += 4) {
            float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
            if (ksrc) { k4 = *reinterpret_cast<const float4*>(ksrc + sd0 + e); v4 = *reinterpret_cast<const float4*>(vsrc + sd0 + e); }
            kf[e] = k4.x; kf[e + 1] = k4.y; kf[e + 2] = k4.z; kf[e + 3] = k4.w;
            vf[e] = v4.x; vf[e + 1] = v4.y; vf[e + 2] = v4.z; vf[e + 3] = v4.w;
        }
    }
    float mk = 0.0f, mv = 0.0f;
#pragma unroll
    for (int e = 0; e < EPT; ++e) { mk = fmaxf(mk, fabsf(kf[e])); mv = fmaxf(mv, fabsf(vf[e])); }
    mk = mi_wave_max(mk); mv = mi_wave_max(mv);
    for (int i = tid; i < FW_CHUNK16; i += 256) img[i] = make_uint4(0u, 0u, 0u, 0u);      // (the pad chunks are copied too: keep them defined)
    if (lane == 0) { smax[0][wave] = mk; smax[1][wave] = mv; }
    __syncthreads();
    const float mka = fmaxf(fmaxf(smax[0][0], smax[0][1]), fmaxf(smax[0][2], smax[0][3])), mva = fmaxf(fmaxf(smax[1][0], smax[1][1]), fmaxf(smax[1][2], smax[1][3]));
    const int ek = fw_scale_exp(mka), ev = fw_scale_exp(mva);
    {
        const float sk = ldexpf(1.0f, ek), sv = ldexpf(1.0f, ev);
        _Float16* ksh = reinterpret_cast<_Float16*>(img);
        _Float16* ksl = reinterpret_cast<_Float16*>(img + FW_PL);
        _Float16* vth = reinterpret_cast<_Float16*>(img + 2 * FW_PL);
        _Float16* vtl = reinterpret_cast<_Float16*>(img + 3 * FW_PL);
#pragma unroll
        for (int e = 0; e < EPT; e += 4) {
            unsigned hb[2], lb[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float x0 = kf[e + 2 * q] * sk, x1 = kf[e + 2 * q + 1] * sk;
                const mi_f16x2 h2 = {(_Float16)x0, (_Float16)x1};
                hb[q] = __builtin_bit_cast(unsigned, h2);
                lb[q] = mi_split_lo2(hb[q], x0, x1);
            }
            const int ko = ((((sd0 + e) >> 3) * 64 + srow) << 3) + ((sd0 + e) & 7);       // chunk (octet of d, row), halves within
            *reinterpret_cast<uint2*>(ksh + ko) = make_uint2(hb[0], hb[1]);
            *reinterpret_cast<uint2*>(ksl + ko) = make_uint2(lb[0], lb[1]);
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const float x = vf[e] * sv;
            const _Float16 hi = (_Float16)x, lo = (_Float16)(x - (float)hi);
            const int vo = (((spos >> 3) * 64 + sd0 + e) << 3) + (spos & 7);             // chunk (octet of the permuted context row, d)
            vth[vo] = hi;
            vtl[vo] = lo;
        }
    }
    __syncthreads();
    const size_t img_i = ((size_t)b * KVH + kvh) * nchunk + c;
    uint4* dst = reinterpret_cast<uint4*>(p.kv_prep) + img_i * FW_CHUNK16;
    for (int i = tid; i < FW_CHUNK16; i += 256) dst[i] = img[i];
    if (tid == 0) {
        int* ex = reinterpret_cast<int*>(reinterpret_cast<uint4*>(p.kv_prep) + (size_t)p.B * KVH * nchunk * FW_CHUNK16) + img_i * 2;
        ex[0] = ek; ex[1] = ev;
    }
}

// PERHEAD (k / v per head, the wide presets' cross-attention): a workgroup = NW x QT x 16 queries of ONE head, which share that head's chunks
// TRAIN (mi_flash_attn_train_fwd): the same arithmetic, plus an optional key mask (mask[b][j] == 0: row j takes no part; every query needs one
// live row) and the logsumexp of every (query, head) written to lse[b][h][i] in the log2 domain of the scores, m + log2(l); with no mask the
// output is mi_flash_attn_fwd's to the bit.  PERHEAD with kv_heads == 1: a multi-query launch whose head count is no multiple of four.
struct fw_train_ext { const uint8_t* mask; float* lse; };
template <int NW, int QT, int WPS, bool PERHEAD = false, bool TRAIN = false>
__global__ __launch_bounds__(64 * NW, WPS) void flash_attn_mq_kernel(const mi_flash_attn_params p, const int nchunk, const fw_train_ext ext) {
    // a workgroup = 64 queries x NH heads; a wave = QT 16-query tiles of one head: every K / V fragment read from LDS feeds QT x 3 matrix
    // instructions (with QT = 1 and 16 waves the LDS reads -- each wave reads the whole chunk -- took longer than the matrix work)
    constexpr int D = 64, WPH = 4 / QT, NH = NW / WPH;
    __shared__ __attribute__((aligned(16))) uint4 kv[2][FW_CHUNK16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 15, lg = lane >> 4;
    const int h = PERHEAD ? (int)blockIdx.y : (int)blockIdx.y * NH + wave / WPH, b = blockIdx.z;
    const int inner = p.heads * D;
    const int nnull = p.null_k ? 1 : 0, J = nnull + p.n0 + p.n1;
    const int KVH = PERHEAD ? p.kv_heads : 1;
    const size_t img0 = ((size_t)b * KVH + (PERHEAD && p.kv_heads != 1 ? h : 0)) * nchunk;
    const uint4* const prep = reinterpret_cast<const uint4*>(p.kv_prep) + img0 * FW_CHUNK16;
    const int* const exps = reinterpret_cast<const int*>(reinterpret_cast<const uint4*>(p.kv_prep) + (size_t)p.B * KVH * nchunk * FW_CHUNK16) + img0 * 2;
    auto issue_chunk = [&](int c, int buf) {
        for (int r = wave; r < FW_CHUNK16 / 64; r += NW) {           // one 1 KB row (64 lanes x 16 bytes) per instruction
            const uint4* src = prep + (size_t)c * FW_CHUNK16 + r * 64 + lane;
#if defined(HIPEMU)
            kv[buf][r * 64 + lane] = *src;
#else
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)&kv[buf][r * 64], 16, 0, 0);
#endif
        }
    };
    issue_chunk(0, 0);
    // Q as the B operand (as flash_attn_f16x3_kernel), one block-scaling exponent per 16-query tile
    fw_f16x8 qh[QT][2], ql[QT][2];
    int eq[QT], tok[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        tok[t] = (PERHEAD ? (int)blockIdx.x * (NW * QT) + wave * QT + t : (int)blockIdx.x * 4 + (wave % WPH) * QT + t) * 16 + lq;
        const int tokc = tok[t] < p.HW ? tok[t] : p.HW - 1;
        const float* qr = p.q + ((size_t)b * p.HW + tokc) * inner + h * D;
        float qv[2][8];
        float mq = 0.0f;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const float4 a = *reinterpret_cast<const float4*>(qr + 32 * hf + 8 * lg), c4 = *reinterpret_cast<const float4*>(qr + 32 * hf + 8 * lg + 4);
            const float w[8] = {a.x, a.y, a.z, a.w, c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) { qv[hf][e] = w[e] * p.q_scale; mq = fmaxf(mq, fabsf(qv[hf][e])); }
        }
        eq[t] = fw_scale_exp(mi_wave_max(mq));
        const float sq = ldexpf(1.0f, eq[t]);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            float w[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = qv[hf][e] * sq;
            uint4 hi, lo;
            fw_split8(w, hi, lo);
            qh[t][hf] = __builtin_bit_cast(fw_f16x8, hi);
            ql[t][hf] = __builtin_bit_cast(fw_f16x8, lo);
        }
    }
    float m[QT], l[QT];
    f32x4 o[QT][4];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m[t] = -INFINITY; l[t] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // one context chunk; MASKED only for the last one (the only chunk that can hold rows >= J).  The block scale `us` is a power of two, so
    // max(s) * us and fma(s, us, -max) are the values max(s * us) and s * us - max of the self-staging kernel, without the multiplies.
    auto chunk = [&](const int c, auto masked) {
        const int j0 = 64 * c, buf = c & 1;
#if !defined(HIPEMU)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of chunk c has landed in LDS ...
#endif
        __syncthreads();                                  // ... everybody's has, and nobody reads chunk c - 1's buffer any more
        if (c + 1 < nchunk) issue_chunk(c + 1, buf ^ 1);
        const uint4* const KsH = kv[buf], * const KsL = kv[buf] + FW_PL, * const VtH = kv[buf] + 2 * FW_PL, * const VtL = kv[buf] + 3 * FW_PL;
        const int ek = exps[2 * c], ev = exps[2 * c + 1];
        const float uv = ldexpf(1.0f, -ev);
        f32x4 s[QT][4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
            for (int t = 0; t < QT; ++t) s[t][jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const fw_f16x8 kh = __builtin_bit_cast(fw_f16x8, KsH[(4 * hf + lg) * 64 + 16 * jt + lq]), kl = __builtin_bit_cast(fw_f16x8, KsL[(4 * hf + lg) * 64 + 16 * jt + lq]);
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    s[t][jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[t][hf], s[t][jt], 0, 0, 0);
                    s[t][jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[t][hf], s[t][jt], 0, 0, 0);
                    s[t][jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[t][hf], s[t][jt], 0, 0, 0);
                }
            }
        }
        fw_f16x8 ph[QT][2], pl[QT][2];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const float us = ldexpf(1.0f, -(ek + eq[t]));
            float mx = -INFINITY;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (decltype(masked)::value && j0 + 16 * jt + 4 * lg + r >= J) s[t][jt][r] = -INFINITY;
                    if constexpr (TRAIN) {
                        const int j = j0 + 16 * jt + 4 * lg + r;
                        if (ext.mask && j < J && !ext.mask[(size_t)b * J + j]) s[t][jt][r] = -INFINITY;
                    }
                    mx = fmaxf(mx, s[t][jt][r]);
                }
            mx *= us;
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m[t], mx);
            if (__any(mn != m[t])) {                        // (else every lane's alpha is exp2(0) = 1)
                // (TRAIN: a masked chunk may leave m = mn = -inf; exp2(-inf - -inf) would be NaN)
                const float alpha = (TRAIN && mn == m[t]) ? 1.0f : __builtin_amdgcn_exp2f(m[t] - mn);
                m[t] = mn;
                l[t] = mi_mul_rounded(l[t], alpha);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[t][dt][r] *= alpha;
            }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float pe[8];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pe[4 * u + r] = __builtin_amdgcn_exp2f(fmaf(s[t][2 * hf + u][r], us, -(TRAIN && mn == -INFINITY ? 0.0f : mn))); l[t] += pe[4 * u + r]; }
                uint4 hi, lo;
                fw_split8(pe, hi, lo);
                ph[t][hf] = __builtin_bit_cast(fw_f16x8, hi);
                pl[t][hf] = __builtin_bit_cast(fw_f16x8, lo);
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            f32x4 sl[QT];
#pragma unroll
            for (int t = 0; t < QT; ++t) sl[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const fw_f16x8 vh = __builtin_bit_cast(fw_f16x8, VtH[(4 * hf + lg) * 64 + 16 * dt + lq]), vl = __builtin_bit_cast(fw_f16x8, VtL[(4 * hf + lg) * 64 + 16 * dt + lq]);
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    sl[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph[t][hf], sl[t], 0, 0, 0);
                    sl[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl[t][hf], sl[t], 0, 0, 0);
                    sl[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph[t][hf], sl[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[t][dt][r] = fmaf(sl[t][r], uv, o[t][dt][r]);
        }
    };
    for (int c = 0; c + 1 < nchunk; ++c) chunk(c, std::false_type{});
    chunk(nchunk - 1, std::true_type{});
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float lt = l[t];
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        const float linv = 1.0f / lt;
        if constexpr (TRAIN) {
            if (tok[t] < p.HW && lg == 0) ext.lse[((size_t)b * p.heads + h) * p.HW + tok[t]] = m[t] + log2f(lt);
        }
        if (tok[t] < p.HW) {
            float* orow = p.out + ((size_t)b * p.HW + tok[t]) * inner + h * D;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                *reinterpret_cast<float4*>(orow + 16 * dt + 4 * lg) = make_float4(o[t][dt][0] * linv, o[t][dt][1] * linv, o[t][dt][2] * linv, o[t][dt][3] * linv);
        }
    }
}
