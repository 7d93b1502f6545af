// Sampler epilogue kernels: K11 (CFG combine + x0), K12 (bit-exact dynamic-threshold quantile),
// K13/K15 (posterior step, final clamp), the tail without the select (static clip / no clip), K14 (cubic resize + low-res augmentation) and the
// counter-based normal generator.  All elementwise math keeps the reference's operation order
// with un-fused multiplies/adds (__fmul_rn/__fadd_rn) so the only differences to the reference's
// fp32 results come from the U-Net's summation order.
#include "common.hip.h"

// hipcc contracts a*b+c into FMA by default and its __fmul_rn/__fadd_rn are plain operators: switch contraction
// off for this file so the elementwise sampler math rounds exactly like the reference's separate torch ops.
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ the arithmetic of one denoising step, per element
// Written ONCE: the separate kernels (cfg_x0 / quantile_* / posterior) and the two fused tails (sampler_small / sampler_group) differ in
// where an element lives and how the workgroups meet, never in what is computed.  Every helper is inlined into its caller.
struct step_coef { float ca, cb, c1, c2, sigma, c5; };      // row t of the S x 8 coefficient table; c5: the multistep solvers' history term
template <bool HISTORY>
__device__ __forceinline__ step_coef load_step_coef(const float* coef, int t) {
    const float* r = coef + t * 8;
    return {r[0], r[1], r[2], r[3], r[4], HISTORY ? r[5] : 0.0f};
}

// four consecutive floats of a row of n, from element i (a multiple of 4): one 16-byte access when `vec` (n % 4 == 0), else element by
// element inside the row (loads past the end give 0)
__device__ __forceinline__ void ld_quad(const float* row, int i, int n, bool vec, float (&v)[4]) {
    if (vec) { const float4 q = mi_ldg4(row + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (i + e < n) ? row[i + e] : 0.0f;
    }
}
__device__ __forceinline__ void st_quad(float* row, int i, int n, bool vec, const float (&v)[4]) {
    if (vec) mi_stg4(row + i, make_float4(v[0], v[1], v[2], v[3]));
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
    }
}

// classifier-free guidance combine and the x0 it predicts; pred: the guided noise prediction
__device__ __forceinline__ float guided_x0(float c, float nl, float xt, int two, float cond_scale, const step_coef& cf, float& pred) {
    pred = c;
    if (two) pred = __fadd_rn(nl, __fmul_rn(__fsub_rn(c, nl), cond_scale));     // Unet.py:506
    return __fsub_rn(__fmul_rn(cf.ca, xt), __fmul_rn(cf.cb, pred));             // diffusion_model.py:159-162
}

// digit layout of a non-negative float's bit pattern (bit 31 = 0): pass 0 -> bits 30..20, pass 1 -> 19..9, pass 2 -> 8..0
__device__ __forceinline__ int q_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 9 : 0); }
__device__ __forceinline__ int q_bits(int pass) { return pass == 2 ? 9 : 11; }

// one element of radix pass `pass`: count its digit into lh[sel] for every selected prefix its higher digits match (pass 0 has no prefix
// yet; `second` off: one histogram serves both order statistics)
__device__ __forceinline__ void radix_count(unsigned (&lh)[2][MI_Q_BINS], float v, int pass, unsigned prefix0, unsigned prefix1, bool second) {
    const int shift = q_shift(pass), nb = q_bits(pass);
    const unsigned key = __float_as_uint(fabsf(v));
    const unsigned hi = pass == 0 ? 0u : (key >> (shift + nb)), bin = (key >> shift) & ((1u << nb) - 1u);
    if (hi == prefix0) atomicAdd(&lh[0][bin], 1u);
    if (second && hi == prefix1) atomicAdd(&lh[1][bin], 1u);
}

// the dynamic threshold from the bit patterns of the two order statistics (a, bb: the statistics themselves)
__device__ __forceinline__ float threshold_from_ranks(unsigned prefix0, unsigned prefix1, unsigned nan_count, float w, float& a, float& bb) {
    // torch.quantile returns NaN for a row that contains a NaN (not the order statistic): NaN bit patterns sit above infinity,
    // i.e. in the top bins of pass 0 (0x7F9.. are NaN only; arithmetic produces the canonical 0x7FC00000) -- nan_count is their sum
    a = __uint_as_float(prefix0); bb = __uint_as_float(prefix1);
    if (nan_count) a = bb = __uint_as_float(0x7FC00000u);
    const float d = __fsub_rn(bb, a);
    // ATen lerp: weight < 0.5 ? a + w*d : b - d*(1-w), multiply-add fused
    return (fabsf(w) < 0.5f) ? fmaf(w, d, a) : fmaf(__fsub_rn(w, 1.0f), d, bb);
}
__device__ __forceinline__ float threshold_scale(float sq) { return (sq < 1.0f) ? 1.0f : sq; }      // Imagen.py:320 clamp_(min=1.): a NaN threshold stays NaN, as in torch

// x_{t-1} of one element.  HISTORY: plus c5 * (the PREVIOUS step's thresholded x0, in pv), and pv becomes this step's for the next one.
// CLIP: how x0 is bounded first -- CLIP_DYNAMIC clamp(x0, -s, s) / s with the image's threshold scale s (the reference; the default, and the
// instructions this helper always had), CLIP_STATIC clamp(x0, -1, 1) (the bits of CLIP_DYNAMIC at s = 1.0f: a division by 1 is exact, so it
// is not issued; s is not read), CLIP_NONE x0 as predicted (s is not read)
enum { CLIP_NONE = 0, CLIP_STATIC = 1, CLIP_DYNAMIC = 2 };
template <bool HISTORY, int CLIP = CLIP_DYNAMIC>
__device__ __forceinline__ float posterior_elem(float x0, float x, float z, float s, const step_coef& cf, float& pv) {
    const float c1 = cf.c1, c2 = cf.c2;
    if constexpr (CLIP == CLIP_DYNAMIC) x0 = __fdiv_rn(x0 != x0 ? x0 : fminf(fmaxf(x0, -s), s), s);      // Imagen.py:323 (torch.clamp propagates NaN)
    if constexpr (CLIP == CLIP_STATIC) x0 = x0 != x0 ? x0 : fminf(fmaxf(x0, -1.0f), 1.0f);
    float mean = __fadd_rn(__fmul_rn(c1, x0), __fmul_rn(c2, x));                // diffusion_model.py:118-121
    if constexpr (HISTORY) { mean = __fadd_rn(mean, __fmul_rn(cf.c5, pv)); pv = x0; }
    return __fadd_rn(mean, __fmul_rn(cf.sigma, z));                            // Imagen.py:370
}

// ------------------------------------------------------------------ Philox4x32-10 + Box-Muller
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const unsigned hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const unsigned hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// four N(0,1) draws for (seed, sample, stream, quad index)
__device__ __forceinline__ void randn4(unsigned long long seed, unsigned sample, unsigned stream, unsigned quad, float (&z)[4]) {
    unsigned c[4] = {quad, sample, stream, 0x4D494E49u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const float u0 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u1 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u3 = ((float)(c[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    const float a0 = 6.28318530717958647692f * u1, a1 = 6.28318530717958647692f * u3;
    z[0] = r0 * cosf(a0); z[1] = r0 * sinf(a0);
    z[2] = r1 * cosf(a1); z[3] = r1 * sinf(a1);
}

// the draws of step k (counted from the first step) for quad qd of image b: the injected buffer [T][B][n], or Philox
__device__ __forceinline__ void step_noise4(const mi_posterior_params& pp, int b, int k, int qd, int n, bool vec, float (&z)[4]) {
    if (pp.noise) ld_quad(pp.noise + ((size_t)k * pp.B + b) * n, 4 * qd, n, vec, z);
    else randn4(pp.seed_dev ? *pp.seed_dev : pp.seed, (unsigned)(pp.sample0 + b), (unsigned)(pp.stream_base + k), (unsigned)qd, z);
}

// ------------------------------------------------------------------ the known region of an inpainting call (mi_inpaint_params)
// coefficient columns 6 and 7 of the step's row: sqrt(abar_{k-1}), sqrt(1 - abar_{k-1})
struct known_coef { float c6, c7; };
__device__ __forceinline__ known_coef load_known_coef(const float* coef, int t) { return {coef[t * 8 + 6], coef[t * 8 + 7]}; }

// the mask bytes of the four elements from i (a multiple of 4) of image b: element i uses pixel i % hw.  One 4-byte load when hw % 4 == 0 (a
// quad then lies inside one channel), else byte by byte -- a quad may straddle two channels; past the row's end: 0
__device__ __forceinline__ void ld_mask4(const mi_inpaint_params& ip, int b, int i, int n, unsigned char (&m)[4]) {
    const unsigned char* row = ip.mask + (size_t)b * ip.hw;
    if ((ip.hw & 3) == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(row + i % ip.hw);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = (unsigned char)(w >> (8 * e));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = (i + e < n) ? row[(i + e) % ip.hw] : (unsigned char)0;
    }
}

// the masked replace of one quad: v = m ? a*y + b*z' : v, fadd(fmul(a, y), fmul(b, z')), every operation rounded on its own.  `j`: the blend's
// index (0 behind x_T, s + 1 in the tail of the step counted s from the first) = the index of its draw, from the injected buffer [S][B][n] or
// Philox stream known_stream + j with the step noise's (seed, row, quad) keying; j < 0: no draw, neither read nor generated -- the known
// pixels become y itself (the last blend, whose row holds (1, 0)).  The known image and the mask are read once; a quad without a known pixel draws nothing.
__device__ __forceinline__ void known_blend4(const mi_inpaint_params& ip, unsigned long long seed, int sample0, int B, int b, int j, int qd, int n, bool vec,
                                             float a, float bcoef, float (&v)[4]) {
    unsigned char m[4];
    ld_mask4(ip, b, 4 * qd, n, m);
    if (!(m[0] | m[1] | m[2] | m[3])) return;
    float y[4], z[4];
    ld_quad(ip.known + (size_t)b * n, 4 * qd, n, vec, y);
    if (j < 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (m[e]) v[e] = y[e];
        return;
    }
    if (ip.known_noise) ld_quad(ip.known_noise + ((size_t)j * B + b) * n, 4 * qd, n, vec, z);
    else randn4(seed, (unsigned)(sample0 + b), (unsigned)(ip.known_stream + j), (unsigned)qd, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) if (m[e]) v[e] = __fadd_rn(__fmul_rn(a, y[e]), __fmul_rn(bcoef, z[e]));
}
// ... in the tail of the step at coefficient row t (k = T - 1 - t steps behind the first): blend k + 1 with columns 6 and 7, no draw at row 0
__device__ __forceinline__ void known_step4(const mi_inpaint_params& ip, const mi_posterior_params& pp, int b, int t, int k, int qd, int n, bool vec, float (&v)[4]) {
    const known_coef kc = load_known_coef(pp.coef, t);
    known_blend4(ip, pp.seed_dev ? *pp.seed_dev : pp.seed, pp.sample0, pp.B, b, t > 0 ? k + 1 : -1, qd, n, vec, kc.c6, kc.c7, v);
}

// ------------------------------------------------------------------ K11 epilogue
template <bool HIST>
__global__ __launch_bounds__(256) void cfg_x0_kernel(const mi_cfg_x0_params p) {
    __shared__ unsigned lh[HIST ? MI_Q_BINS : 1];      // pass 0 of the radix select (bits 30..20 of |x0|), fused into the producer of x0
    const int b = blockIdx.y;
    const int t = p.t_state ? *p.t_state - p.t_off : 0;
    const step_coef cf = p.coef ? load_step_coef<false>(p.coef, t) : step_coef{};
    if constexpr (HIST) {
        for (int i = threadIdx.x; i < MI_Q_BINS; i += 256) lh[i] = 0u;
        __syncthreads();
    }
    auto one = [&](float c, float nl, float xt, float& pred, float& x0) {
        x0 = guided_x0(c, nl, xt, p.two, p.cond_scale, cf, pred);
        if constexpr (HIST) { if (p.x0) atomicAdd(&lh[__float_as_uint(fabsf(x0)) >> 20], 1u); }
    };
    if ((p.n & 3) == 0) {                           // 16-byte accesses (every image size the cascade uses)
        const size_t ob = (size_t)b * p.n, on = (size_t)(b + p.B) * p.n;
        for (int q = blockIdx.x * 256 + threadIdx.x; q < (p.n >> 2); q += gridDim.x * 256) {
            const float4 c = mi_ldg4(p.pred2 + ob + 4 * q);
            const float4 nl = p.two ? mi_ldg4(p.pred2 + on + 4 * q) : c;
            const float4 xt = p.x0 ? mi_ldg4(p.x_t + ob + 4 * q) : c;
            float4 pr, x0;
            one(c.x, nl.x, xt.x, pr.x, x0.x); one(c.y, nl.y, xt.y, pr.y, x0.y); one(c.z, nl.z, xt.z, pr.z, x0.z); one(c.w, nl.w, xt.w, pr.w, x0.w);
            if (p.pred_out) mi_stg4(p.pred_out + ob + 4 * q, pr);
            if (p.x0) mi_stg4(p.x0 + ob + 4 * q, x0);
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < p.n; i += gridDim.x * 256) {
            const float c = p.pred2[(size_t)b * p.n + i];
            const float nl = p.two ? p.pred2[(size_t)(b + p.B) * p.n + i] : c;
            const float xt = p.x0 ? p.x_t[(size_t)b * p.n + i] : c;
            float pred, x0;
            one(c, nl, xt, pred, x0);
            if (p.pred_out) p.pred_out[(size_t)b * p.n + i] = pred;
            if (p.x0) p.x0[(size_t)b * p.n + i] = x0;
        }
    }
    if constexpr (HIST) {
        __syncthreads();
        // both order statistics share the pass-0 histogram (no prefix yet): selector slot 0 only, read for both
        unsigned* gh = p.hist0 + ((size_t)b * 2) * MI_Q_BINS;
        for (int i = threadIdx.x; i < MI_Q_BINS; i += 256) {
            const unsigned v = lh[i];
            if (v) atomicAdd(&gh[i], v);
        }
    }
}

// ------------------------------------------------------------------ K12 radix select
// Block-wide: locate the bin of `hist` (MI_Q_BINS entries) that holds 0-based rank r; returns bin and the
// rank inside the bin.  All 256 work-items call it; result broadcast through LDS.
__device__ void q_find_bin(const unsigned* hist, unsigned r, int* sh_scratch, unsigned& bin_out, unsigned& r_out, bool active = true) {
    // `active`: the first 256 work-items of the workgroup scan (8 bins each); larger workgroups pass false for the rest, which only
    // take part in the barriers and receive the broadcast
    unsigned* wsum = reinterpret_cast<unsigned*>(sh_scratch);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned c[8], tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { c[k] = active ? hist[tid * 8 + k] : 0u; tot += c[k]; }
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (active && lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < wave && w < 4; ++w) base += wsum[w];
    unsigned excl = base + inc - tot;
    if (active && r >= excl && r < excl + tot) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (r < excl + c[k]) { wsum[4] = (unsigned)(tid * 8 + k); wsum[5] = r - excl; break; }
            excl += c[k];
        }
    }
    __syncthreads();
    bin_out = wsum[4];
    r_out = wsum[5];
    __syncthreads();
}

template <int PASS>
__global__ __launch_bounds__(256) void quantile_hist_kernel(const mi_quantile_params p) {
    __shared__ unsigned lh[2][MI_Q_BINS];
    __shared__ int scratch[8];
    const int tid = threadIdx.x, b = blockIdx.y;
    // resolve the prefixes chosen by the earlier passes (every workgroup redoes this tiny scan)
    unsigned prefix[2] = {0u, 0u}, rk[2] = {(unsigned)p.k_lo, (unsigned)p.k_hi};
#pragma unroll
    for (int ps = 0; ps < PASS; ++ps) {
#pragma unroll
        for (int sel = 0; sel < 2; ++sel) {
            unsigned bin, rr;
            q_find_bin(p.hist + (((size_t)ps * p.B + b) * 2 + (ps == 0 ? 0 : sel)) * MI_Q_BINS, rk[sel], scratch, bin, rr);      // pass 0: shared slot
            prefix[sel] = (prefix[sel] << q_bits(ps)) | bin;
            rk[sel] = rr;
        }
    }
    for (int i = tid; i < 2 * MI_Q_BINS; i += 256) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const float* xb = p.x0 + (size_t)b * p.n;
    auto count = [&](float v) { radix_count(lh, v, PASS, prefix[0], prefix[1], PASS > 0); };      // pass 0: one histogram serves both order statistics
    if ((p.n & 3) == 0) {
        for (int q = blockIdx.x * 256 + tid; q < (p.n >> 2); q += gridDim.x * 256) {
            const float4 v = mi_ldg4(xb + 4 * q);
            count(v.x); count(v.y); count(v.z); count(v.w);
        }
    } else {
        for (int i = blockIdx.x * 256 + tid; i < p.n; i += gridDim.x * 256) count(xb[i]);
    }
    __syncthreads();
    unsigned* gh = p.hist + (((size_t)PASS * p.B + b) * 2) * MI_Q_BINS;
    for (int i = tid; i < (PASS == 0 ? 1 : 2) * MI_Q_BINS; i += 256) {
        const unsigned v = (&lh[0][0])[i];
        if (v) atomicAdd(&gh[i], v);
    }
}

__global__ __launch_bounds__(256) void quantile_finish_kernel(const mi_quantile_params p) {
    __shared__ int scratch[8];
    const int b = blockIdx.x;
    unsigned prefix[2] = {0u, 0u}, rk[2] = {(unsigned)p.k_lo, (unsigned)p.k_hi};
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {
#pragma unroll
        for (int sel = 0; sel < 2; ++sel) {
            unsigned bin, rr;
            q_find_bin(p.hist + (((size_t)ps * p.B + b) * 2 + (ps == 0 ? 0 : sel)) * MI_Q_BINS, rk[sel], scratch, bin, rr);
            prefix[sel] = (prefix[sel] << q_bits(ps)) | bin;
            rk[sel] = rr;
        }
    }
    if (threadIdx.x == 0) {
        const unsigned* h0 = p.hist + ((size_t)b * 2) * MI_Q_BINS;
        unsigned nan_count = 0;
        for (int k = 0x7F9; k < MI_Q_BINS; ++k) nan_count += h0[k];          // the NaN bins of pass 0 (threshold_from_ranks)
        float a, bb;
        p.s_out[b] = threshold_from_ranks(prefix[0], prefix[1], nan_count, p.w, a, bb);
        if (p.v_out) { p.v_out[2 * b] = a; p.v_out[2 * b + 1] = bb; }
    }
    if (p.self_cleaning) {       // leave this image's counters zeroed for the next denoising step (no memset launch)
        __syncthreads();
        for (int ps = 0; ps < 3; ++ps) {
            unsigned* gh = p.hist + (((size_t)ps * p.B + b) * 2) * MI_Q_BINS;
            for (int i = threadIdx.x; i < 2 * MI_Q_BINS; i += 256) gh[i] = 0u;
        }
    }
}

__global__ __launch_bounds__(256) void randn_fill_kernel(float* out, int n, unsigned long long seed, int sample0, int stream_id) {
    const int b = blockIdx.y;
    const int nq = (n + 3) / 4;
    for (int qd = blockIdx.x * 256 + threadIdx.x; qd < nq; qd += gridDim.x * 256) {
        float z[4];
        randn4(seed, (unsigned)(sample0 + b), (unsigned)stream_id, (unsigned)qd, z);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * qd + k < n) out[(size_t)b * n + 4 * qd + k] = z[k];
    }
}

// ------------------------------------------------------------------ K13
// HISTORY (the three tail kernels): the multistep solvers' term c5 * (the PREVIOUS step's thresholded x0), coefficient column 5, and the
// store of this step's thresholded x0 for the next one.  The history kernels take the extension struct as one more argument.
// INPAINT: the masked replace of the known region (known_step4) behind the step, before the store; one more argument, mi_inpaint_params, last.
// The <false, false> instantiations have the argument list -- and the instructions -- of the kernels before the template parameters existed.
__device__ __forceinline__ float* x0_prev_of() { return nullptr; }
__device__ __forceinline__ float* x0_prev_of(const mi_sampler_ext_params& e) { return e.x0_prev; }
__device__ __forceinline__ float* x0_prev_of(const mi_inpaint_params&) { return nullptr; }
__device__ __forceinline__ float* x0_prev_of(const mi_sampler_ext_params& e, const mi_inpaint_params&) { return e.x0_prev; }
__device__ __forceinline__ mi_inpaint_params known_of() { return {}; }
__device__ __forceinline__ mi_inpaint_params known_of(const mi_sampler_ext_params&) { return {}; }
__device__ __forceinline__ mi_inpaint_params known_of(const mi_inpaint_params& ip) { return ip; }
__device__ __forceinline__ mi_inpaint_params known_of(const mi_sampler_ext_params&, const mi_inpaint_params& ip) { return ip; }

template <bool HISTORY, bool INPAINT, typename... EXT>
__global__ __launch_bounds__(256) void posterior_kernel(const mi_posterior_params p, const EXT... ext) {
    static_assert(sizeof...(EXT) == (HISTORY ? 1 : 0) + (INPAINT ? 1 : 0), "the history kernels take mi_sampler_ext_params, the inpainting kernels mi_inpaint_params");
    const int b = blockIdx.y;
    const int t = *p.t_state - p.t_off;
    const step_coef cf = load_step_coef<HISTORY>(p.coef, t);
    float* const prev = x0_prev_of(ext...);
    [[maybe_unused]] const mi_inpaint_params ip = known_of(ext...);
    const float s = threshold_scale(p.s_q[b]);
    const int k = (p.T - 1) - t;
    const int n = p.n, nq = (n + 3) / 4;
    const bool vec = (n & 3) == 0;
    const size_t ob = (size_t)b * n;
    for (int qd = blockIdx.x * 256 + threadIdx.x; qd < nq; qd += gridDim.x * 256) {
        float z[4], x0[4], x[4], pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        step_noise4(p, b, k, qd, n, vec, z);
        ld_quad(p.x0 + ob, 4 * qd, n, vec, x0);
        ld_quad(p.x + ob, 4 * qd, n, vec, x);
        if constexpr (HISTORY) ld_quad(prev + ob, 4 * qd, n, vec, pv);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = posterior_elem<HISTORY>(x0[e], x[e], z[e], s, cf, pv[e]);      // (past the row's end: on zeros, not stored)
        if constexpr (INPAINT) known_step4(ip, p, b, t, k, qd, n, vec, x);
        st_quad(p.x + ob, 4 * qd, n, vec, x);
        if constexpr (HISTORY) st_quad(prev + ob, 4 * qd, n, vec, pv);
    }
}

// ------------------------------------------------------------------ K11 epilogue + K12 + K13 in one launch (small images)
// One workgroup of 1024 work-items per image; every work-item keeps its quads of x0 in registers, the three radix passes run on
// histograms in LDS.  Operation order per element as in cfg_x0_kernel / quantile_*_kernel / posterior_kernel: bit-identical results.
#ifndef SS_THREADS
#define SS_THREADS 1024
#endif
constexpr int SS_NT = SS_THREADS, SS_MAXQ = MI_SAMPLER_SMALL_N / 4 / SS_NT;      // quads per work-item
template <bool HISTORY, bool INPAINT, typename... EXT>
__global__ __launch_bounds__(SS_NT) void sampler_small_kernel(const mi_cfg_x0_params c, const mi_quantile_params q, const mi_posterior_params pp, const EXT... ext) {
    static_assert(sizeof...(EXT) == (HISTORY ? 1 : 0) + (INPAINT ? 1 : 0), "the history kernels take mi_sampler_ext_params, the inpainting kernels mi_inpaint_params");
    __shared__ unsigned lh[2][MI_Q_BINS];
    __shared__ int scratch[8];
    __shared__ unsigned nan_sh;
    const int tid = threadIdx.x, b = blockIdx.x, n = c.n, nq = (n + 3) / 4;
    const int t = *c.t_state - c.t_off;
    const step_coef cf = load_step_coef<HISTORY>(c.coef, t);
    float* const prev = x0_prev_of(ext...);
    [[maybe_unused]] const mi_inpaint_params ip = known_of(ext...);
    const bool vec = (n & 3) == 0;
    const size_t ob = (size_t)b * n, on = (size_t)(b + c.B) * n;
    float x0v[SS_MAXQ][4], xtv[SS_MAXQ][4];
    for (int i = tid; i < 2 * MI_Q_BINS; i += SS_NT) (&lh[0][0])[i] = 0u;
    if (tid == 0) nan_sh = 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SS_MAXQ; ++u) {
        const int qd = tid + u * SS_NT;
#pragma unroll
        for (int e = 0; e < 4; ++e) xtv[u][e] = x0v[u][e] = 0.0f;
        if (qd < nq) {
            float cc[4], nl[4], pr;
            ld_quad(c.pred2 + ob, 4 * qd, n, vec, cc);
            ld_quad(c.x_t + ob, 4 * qd, n, vec, xtv[u]);
            if (c.two) ld_quad(c.pred2 + on, 4 * qd, n, vec, nl);
            else { nl[0] = cc[0]; nl[1] = cc[1]; nl[2] = cc[2]; nl[3] = cc[3]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x0v[u][e] = guided_x0(cc[e], nl[e], xtv[u][e], c.two, c.cond_scale, cf, pr);
                if (4 * qd + e < n) {
                    atomicAdd(&lh[0][__float_as_uint(fabsf(x0v[u][e])) >> 20], 1u);
                    if (c.pred_out) c.pred_out[ob + 4 * qd + e] = pr;
                    if (c.x0) c.x0[ob + 4 * qd + e] = x0v[u][e];
                }
            }
        }
    }
    __syncthreads();
    if (tid < MI_Q_BINS - 0x7F9) { const unsigned v = lh[0][0x7F9 + tid]; if (v) atomicAdd(&nan_sh, v); }      // the NaN bins of pass 0 (threshold_from_ranks)
    unsigned prefix[2] = {0u, 0u}, rk[2] = {(unsigned)q.k_lo, (unsigned)q.k_hi};
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {
        if (ps > 0) {
            // histogram of the next digit over the elements that carry each selected prefix
            __syncthreads();
            for (int i = tid; i < 2 * MI_Q_BINS; i += SS_NT) (&lh[0][0])[i] = 0u;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < SS_MAXQ; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * (tid + u * SS_NT) + e < n) radix_count(lh, x0v[u][e], ps, prefix[0], prefix[1], true);
            __syncthreads();
        }
#pragma unroll
        for (int sel = 0; sel < 2; ++sel) {
            unsigned bin, rr;
            q_find_bin(&lh[ps == 0 ? 0 : sel][0], rk[sel], scratch, bin, rr, tid < 256);
            prefix[sel] = (prefix[sel] << q_bits(ps)) | bin;
            rk[sel] = rr;
        }
    }
    float a, bb;
    const float sq = threshold_from_ranks(prefix[0], prefix[1], nan_sh, q.w, a, bb);
    if (tid == 0) {
        if (q.s_out) q.s_out[b] = sq;
        if (q.v_out) { q.v_out[2 * b] = a; q.v_out[2 * b + 1] = bb; }
    }
    const float s = threshold_scale(sq);
    const int k = (pp.T - 1) - t;
#pragma unroll
    for (int u = 0; u < SS_MAXQ; ++u) {
        const int qd = tid + u * SS_NT;
        if (qd >= nq) continue;
        float z[4], r[4], pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        step_noise4(pp, b, k, qd, n, vec, z);
        if constexpr (HISTORY) ld_quad(prev + ob, 4 * qd, n, vec, pv);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = posterior_elem<HISTORY>(x0v[u][e], xtv[u][e], z[e], s, cf, pv[e]);
        if constexpr (INPAINT) known_step4(ip, pp, b, t, k, qd, n, vec, r);
        st_quad(pp.x + ob, 4 * qd, n, vec, r);
        if constexpr (HISTORY) st_quad(prev + ob, 4 * qd, n, vec, pv);
    }
}

// ------------------------------------------------------------------ K11 epilogue + K13 in one launch, without the radix select (any image size)
// The tail of a step whose x0 is bounded by a constant (CLIP_STATIC) or not at all (CLIP_NONE): nothing of an image meets, so the step is
// elementwise -- a grid of (chunks, B) workgroups of 256, every work-item its quads of one image from the prediction to the store of x_{t-1}.
// No LDS, no atomics, no sync buffer, no x0 / histogram round trip.  Per element the operations of cfg_x0_kernel and posterior_kernel in their
// order (guided_x0, posterior_elem<HISTORY, CLIP>, known_step4): CLIP_STATIC gives the bits of the dynamic tails wherever their scale is 1.
template <int CLIP, bool HISTORY, bool INPAINT, typename... EXT>
__global__ __launch_bounds__(256) void sampler_direct_kernel(const mi_cfg_x0_params c, const mi_posterior_params pp, const EXT... ext) {
    static_assert(CLIP == CLIP_STATIC || CLIP == CLIP_NONE, "the dynamic threshold needs the select: sampler_small / sampler_group / the separate kernels");
    static_assert(sizeof...(EXT) == (HISTORY ? 1 : 0) + (INPAINT ? 1 : 0), "the history kernels take mi_sampler_ext_params, the inpainting kernels mi_inpaint_params");
    const int b = blockIdx.y, n = c.n, nq = (n + 3) / 4;
    const int t = *c.t_state - c.t_off;
    const step_coef cf = load_step_coef<HISTORY>(c.coef, t);
    float* const prev = x0_prev_of(ext...);
    [[maybe_unused]] const mi_inpaint_params ip = known_of(ext...);
    const bool vec = (n & 3) == 0;
    const size_t ob = (size_t)b * n, on = (size_t)(b + c.B) * n;
    const int k = (pp.T - 1) - t;
    for (int qd = blockIdx.x * 256 + threadIdx.x; qd < nq; qd += gridDim.x * 256) {
        float cc[4], nl[4], x[4], z[4], pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        ld_quad(c.pred2 + ob, 4 * qd, n, vec, cc);
        if (c.two) ld_quad(c.pred2 + on, 4 * qd, n, vec, nl);
        else { nl[0] = cc[0]; nl[1] = cc[1]; nl[2] = cc[2]; nl[3] = cc[3]; }
        ld_quad(c.x_t + ob, 4 * qd, n, vec, x);
        step_noise4(pp, b, k, qd, n, vec, z);
        if constexpr (HISTORY) ld_quad(prev + ob, 4 * qd, n, vec, pv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                                                    // (past the row's end: on zeros, not stored)
            float pr;
            const float x0 = guided_x0(cc[e], nl[e], x[e], c.two, c.cond_scale, cf, pr);
            x[e] = posterior_elem<HISTORY, CLIP>(x0, x[e], z[e], 1.0f, cf, pv[e]);
        }
        if constexpr (INPAINT) known_step4(ip, pp, b, t, k, qd, n, vec, x);
        st_quad(pp.x + ob, 4 * qd, n, vec, x);
        if constexpr (HISTORY) st_quad(prev + ob, 4 * qd, n, vec, pv);
    }
}

// set (set == 1) or advance (by value when set == 2, else by 1) the device-resident step and the timestep the U-Net's conditioning sees.
// MAPPED, a step -> trained-timestep map: *t_state stays the STEP index k (what the coefficient table, the step tables and the noise
// are indexed by), times[b] = t_map[k].  Past the last step (k < 0: the advance behind step 0) times keep t_map[0]; nothing reads them
// before the next mi_step_set_mapped.
template <bool MAPPED>
__global__ void step_advance_kernel(int* t_state, long long* times, int B, int set, int value, const int* t_map) {
    const int k = set == 1 ? value : (*t_state - (set == 2 ? value : 1));
    __syncthreads();
    const long long t = MAPPED ? (long long)t_map[k < 0 ? 0 : k] : (long long)k;
    for (int b = threadIdx.x; b < B; b += blockDim.x) times[b] = t;
    if (threadIdx.x == 0) *t_state = k;
}

__global__ __launch_bounds__(256) void finalize_kernel(const float* x, float* out, long long total, int unnormalize) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const float v = x[i] != x[i] ? x[i] : fminf(fmaxf(x[i], -1.0f), 1.0f);      // torch.clamp propagates NaN
        out[i] = unnormalize ? __fmul_rn(__fadd_rn(v, 1.0f), 0.5f) : v;
    }
}

__global__ __launch_bounds__(256) void lowres_augment_kernel(const float* img, const float* noise, float* out, long long total, float a, float b, int normalize) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float v = img[i];
        if (noise) v = __fadd_rn(__fmul_rn(a, v), __fmul_rn(b, noise[i]));       // diffusion_model.py:142-147
        if (normalize) v = __fsub_rn(__fmul_rn(v, 2.0f), 1.0f);                  // helpers.py:105-110 via Imagen.py:393
        out[i] = v;
    }
}

// blend 0 of an inpainting call, right behind the draw of x_T: x = m ? a*y + b*z'_0 : x (known_blend4 with j = 0)
__global__ __launch_bounds__(256) void known_blend0_kernel(float* x, int B, int n, const mi_inpaint_params ip, float a, float bcoef, unsigned long long seed, int sample0) {
    const int b = blockIdx.y, nq = (n + 3) / 4;
    const bool vec = (n & 3) == 0;
    for (int qd = blockIdx.x * 256 + threadIdx.x; qd < nq; qd += gridDim.x * 256) {
        float v[4];
        ld_quad(x + (size_t)b * n, 4 * qd, n, vec, v);
        known_blend4(ip, seed, sample0, B, b, 0, qd, n, vec, a, bcoef, v);
        st_quad(x + (size_t)b * n, 4 * qd, n, vec, v);
    }
}

// the known image of a stage in the sampler's range: clamp to [0, 1] (NaN stays NaN, as torch.clamp), then *2-1 when `normalize`
__global__ __launch_bounds__(256) void known_image_kernel(const float* img, float* out, long long total, int normalize) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float v = img[i] != img[i] ? img[i] : fminf(fmaxf(img[i], 0.0f), 1.0f);
        if (normalize) v = __fsub_rn(__fmul_rn(v, 2.0f), 1.0f);                  // helpers.py:105-110
        out[i] = v;
    }
}
// the starting point of a loop that begins at an image of the caller's: x = a * y' + b * z with y' the image in the sampler's range (as
// known_image_kernel) and z the draw randn_fill_kernel would have written there (same seed, row, stream, quad) or the injected one.
// fadd(fmul, fmul), every operation rounded on its own; `vec`: n % 4 == 0 and 16-byte aligned pointers
__global__ __launch_bounds__(256) void init_noise_kernel(const float* img, float* x, int n, int normalize, float a, float bcoef, unsigned long long seed,
                                                         int sample0, int stream_id, const float* noise, int vec) {
    const int b = blockIdx.y, nq = (n + 3) / 4;
    const size_t ob = (size_t)b * n;
    for (int qd = blockIdx.x * 256 + threadIdx.x; qd < nq; qd += gridDim.x * 256) {
        float y[4], z[4];
        ld_quad(img + ob, 4 * qd, n, vec != 0, y);
        if (noise) ld_quad(noise + ob, 4 * qd, n, vec != 0, z);
        else randn4(seed, (unsigned)(sample0 + b), (unsigned)stream_id, (unsigned)qd, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = y[e] != y[e] ? y[e] : fminf(fmaxf(y[e], 0.0f), 1.0f);
            if (normalize) v = __fsub_rn(__fmul_rn(v, 2.0f), 1.0f);                  // helpers.py:105-110
            y[e] = __fadd_rn(__fmul_rn(a, v), __fmul_rn(bcoef, z[e]));               // diffusion_model.py:142-147 (q_sample)
        }
        st_quad(x + ob, 4 * qd, n, vec != 0, y);                                     // (past the row's end: computed on zeros, not stored)
    }
}
// the mask at a stage's size: nearest neighbour, source index floor(i * Hin / size) (F.interpolate(mode='nearest')); nonzero -> 1
__global__ __launch_bounds__(256) void known_mask_kernel(const unsigned char* in, unsigned char* out, int Hin, int Win, int size) {
    const int b = blockIdx.y;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < size * size; o += gridDim.x * 256) {
        const int sy = (int)(((long long)(o / size) * Hin) / size), sx = (int)(((long long)(o % size) * Win) / size);
        out[(size_t)b * size * size + o] = in[((size_t)b * Hin + sy) * Win + sx] ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void resize_kernel(const mi_resize_params p) {
    const int plane = blockIdx.y;
    const float* src = p.in + (size_t)plane * p.Hin * p.Win;
    float* dst = p.out + (size_t)plane * p.Hout * p.Wout;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < p.Hout * p.Wout; o += gridDim.x * 256) {
        const int oy = o / p.Wout, ox = o % p.Wout;
        float acc = 0.0f;
        for (int kx = 0; kx < p.KW; ++kx) {
            const int sx = p.idx_w[ox * p.KW + kx];
            float col = 0.0f;                                   // H pass value at (oy, sx)
            for (int ky = 0; ky < p.KH; ++ky) {
                const float v = __fmul_rn(src[(size_t)p.idx_h[oy * p.KH + ky] * p.Win + sx], p.w_h[oy * p.KH + ky]);
                col = ky == 0 ? v : __fadd_rn(col, v);
            }
            const float v = __fmul_rn(col, p.w_w[ox * p.KW + kx]);
            acc = kx == 0 ? v : __fadd_rn(acc, v);
        }
        dst[o] = acc;
    }
}

#ifndef Q_WGS
#define Q_WGS 16
#endif
inline int grid_for(long long n, int cap = 2048) {
    long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}


// ------------------------------------------------------------------ K11 epilogue + K12 + K13 in one launch (large images)
// The tail of a denoising step for images too large for one workgroup: G workgroups of 1024 work-items per image, every work-item keeps its
// SG_MAXQ quads of x0 (and x_t) in registers from the guidance combine to the posterior draw; the three radix passes are LDS histograms
// per workgroup, added into per-image histograms with integer agent-scope atomics, and a counter barrier per pass among the G workgroups of
// the image.  Replaces five launches (cfg_x0 + pass 0, pass 1, pass 2, finish, posterior: 71 us at 256^2, B = 32) and two round trips of x0
// through memory.  Same operations in the same order per element: bit-identical to the separate kernels.
// Inter-workgroup protocol: the workgroups of an image are claimed by ticket after they are resident (no cooperative launch, no deadlock
// inside one launch); everything exchanged is touched by agent-scope atomics / sc1 accesses only; the histograms are double-buffered by
// launch parity and the idle copy is zeroed for the next launch; every spin is bounded.
// FAIL-STOP: a workgroup whose wait runs out sets the sticky error word (sync + 8), overwrites ITS part of x_t with NaN and leaves; every
// workgroup that finds the word set -- its peers at their next poll, every workgroup of every later launch on this sync buffer at its
// start -- does the same without waiting.  So a launch that could not complete never leaves a stale or half-written image behind: the
// image (and everything sampled from it) is NaN, which the reference's own pipeline would return for a NaN state as well, and the host
// raises at its next status poll (Imagen: the word is copied to pinned host memory at the end of every call) and re-zeroes the buffer.
// Header of `sync`: [0] u64 ticket | [8] u32 error | [12] u32 knobs: bits 0..30 spin limit (0: SG_SPIN_LIMIT), bit 31 fault injection (tests
// only: the last workgroup of image 0 never arrives at radix pass 1) -- error and knobs are ONE 8-byte load, in flight with the ticket atomic.
constexpr int SG_NT = 1024, SG_MAXQ = 6;
constexpr unsigned SG_SPIN_LIMIT = 1u << 22;
struct sg_layout { long long counters, hist, total; };
__host__ __device__ inline sg_layout sg_sync_layout(int B) {
    sg_layout l;
    l.counters = 64;                                                        // [0] ticket (u64), [8] error word (u32)
    l.hist = l.counters + (((long long)B * 8 + 63) & ~63ll);               // counters: u64 [B]
    l.total = l.hist + (long long)2 * B * 5 * MI_Q_BINS * 4;               // hist: u32 [parity][B][5 = pass 0 | pass 1 x 2 | pass 2 x 2][MI_Q_BINS]
    return l;
}

template <bool HISTORY, bool INPAINT, typename... EXT>
__global__ __launch_bounds__(SG_NT) void sampler_group_kernel(const mi_cfg_x0_params c, const mi_quantile_params q, const mi_posterior_params pp, char* sync, const int G, const EXT... ext) {
    static_assert(sizeof...(EXT) == (HISTORY ? 1 : 0) + (INPAINT ? 1 : 0), "the history kernels take mi_sampler_ext_params, the inpainting kernels mi_inpaint_params");
    __shared__ unsigned lh[2][MI_Q_BINS];
    __shared__ __attribute__((aligned(16))) unsigned hc[2][MI_Q_BINS];
    __shared__ int scratch[8];
    __shared__ unsigned nan_sh;
    __shared__ mi_u64 sTicket;
    __shared__ int sAbort;
    __shared__ unsigned sLimit, sFault;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = c.n, nq = n >> 2;
    unsigned* const errw = reinterpret_cast<unsigned*>(sync + 8);
    if (tid == 0) {
        const mi_u64 hdr = mi_agent_load_u64(reinterpret_cast<const mi_u64*>(sync + 8));      // error | knobs
        sTicket = mi_agent_add_u64(reinterpret_cast<mi_u64*>(sync), 1ull);
        sAbort = (unsigned)hdr != 0u;                           // an earlier launch on this buffer failed: fail-stop, see above
        const unsigned knobs = (unsigned)(hdr >> 32), lim = knobs & 0x7fffffffu;
        sLimit = lim ? lim : SG_SPIN_LIMIT;
        sFault = knobs >> 31;
        nan_sh = 0u;
    }
    for (int i = tid; i < 2 * MI_Q_BINS; i += SG_NT) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const sg_layout lay = sg_sync_layout(c.B);
    const mi_u64 tk = sTicket, Gt = (mi_u64)c.B * (mi_u64)G, seq = tk / Gt;
    const int local = (int)(tk - seq * Gt), b = local / G, g = local - b * G, par = (int)(seq & 1);
    mi_u64* const counter = reinterpret_cast<mi_u64*>(sync + lay.counters) + b;
    unsigned* const H = reinterpret_cast<unsigned*>(sync + lay.hist) + ((size_t)par * c.B + b) * 5 * MI_Q_BINS;
    const mi_buf hbuf = mi_make_buf(H);
    const mi_buf zbuf = mi_make_buf(sync + lay.hist + ((size_t)(par ^ 1) * c.B + b) * 5 * MI_Q_BINS * 4);
    // the idle parity's histograms of this image, zeroed for the next launch (write-through: the next launch's atomics find zeros in memory)
    for (int i = g * SG_NT + tid; i < 5 * MI_Q_BINS / 4; i += G * SG_NT) mi_buf_store_f32x4_sc1(zbuf, (unsigned)i * 16u, (f32x4){0.f, 0.f, 0.f, 0.f});

    const int t = *c.t_state - c.t_off;
    const step_coef cf = load_step_coef<HISTORY>(c.coef, t);
    float* const prev = x0_prev_of(ext...);
    [[maybe_unused]] const mi_inpaint_params ip = known_of(ext...);
    const size_t ob = (size_t)b * n, on = (size_t)(b + c.B) * n;
    const int q0 = g * SG_NT * SG_MAXQ;                        // this workgroup's quads: q0 + tid + u * SG_NT
    // fail-stop: this workgroup's part of the image becomes NaN (never a stale or half-finished x_t)
    auto poison = [&]() {
        const float qn = __uint_as_float(0x7FC00000u);
        for (int u = 0; u < SG_MAXQ; ++u) {
            const int qd = q0 + tid + u * SG_NT;
            if (qd < nq) mi_stg4(pp.x + ob + 4 * qd, make_float4(qn, qn, qn, qn));
        }
    };
    if (sAbort) { poison(); return; }
    float x0v[SG_MAXQ][4], xtv[SG_MAXQ][4];
#pragma unroll
    for (int u = 0; u < SG_MAXQ; ++u) {
        const int qd = q0 + tid + u * SG_NT;
#pragma unroll
        for (int e = 0; e < 4; ++e) xtv[u][e] = x0v[u][e] = 0.0f;
        if (qd < nq) {
            float cc[4], nl[4], pr;
            ld_quad(c.pred2 + ob, 4 * qd, n, true, cc);
            ld_quad(c.x_t + ob, 4 * qd, n, true, xtv[u]);
            if (c.two) ld_quad(c.pred2 + on, 4 * qd, n, true, nl);
            else { nl[0] = cc[0]; nl[1] = cc[1]; nl[2] = cc[2]; nl[3] = cc[3]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x0v[u][e] = guided_x0(cc[e], nl[e], xtv[u][e], c.two, c.cond_scale, cf, pr);
                atomicAdd(&lh[0][__float_as_uint(fabsf(x0v[u][e])) >> 20], 1u);
                if (c.pred_out) c.pred_out[ob + 4 * qd + e] = pr;
                if (c.x0) c.x0[ob + 4 * qd + e] = x0v[u][e];
            }
        }
    }
    // one pass of the radix select across the image's workgroups: add this workgroup's `nh` LDS histograms into the image's, wait for all
    // G workgroups, copy the totals into LDS (hc)
    auto exchange = [&](int phase, int slot0, int nh) -> bool {
        __syncthreads();
        for (int i = tid; i < nh * MI_Q_BINS; i += SG_NT) {
            const unsigned v = (&lh[0][0])[i];
            if (v) atomicAdd(&H[(size_t)slot0 * MI_Q_BINS + i], v);
        }
        mi_drain_vmem();                                   // every wave's atomics are performed before the arrival is counted
        __syncthreads();
        if (tid == 0 && !(sFault == 1u && phase == 1 && b == 0 && g == G - 1)) mi_agent_add_u64(counter, 1ull);
        if (wave == 0) {
            const mi_u64 target = (seq * 3 + (mi_u64)phase + 1) * (mi_u64)G;
            const unsigned limit = sLimit;
            for (unsigned spins = 0;;) {
                const mi_u64 v = mi_agent_load_u64(counter);
                if (__all(v >= target)) break;
                const bool peer_failed = (spins & 63u) == 63u && mi_agent_load_u32(errw) != 0u;
                if (++spins > limit || peer_failed) {
                    if (lane == 0) { if (!peer_failed) mi_agent_store_u32(errw, 0x300u + (unsigned)phase); sAbort = 1; }
                    break;
                }
                mi_sleep();
            }
        }
        __syncthreads();
        if (sAbort) return false;
        for (int i = tid; i < nh * MI_Q_BINS / 4; i += SG_NT)
            reinterpret_cast<f32x4*>(&hc[0][0])[i] = mi_buf_load_f32x4_sc1(hbuf, (unsigned)((slot0 * MI_Q_BINS + 4 * i) * 4));
        __syncthreads();
        return true;
    };
    if (!exchange(0, 0, 1)) { poison(); return; }
    // torch.quantile returns NaN for a row that contains a NaN: NaN patterns sit in the top bins of pass 0 (as quantile_finish_kernel)
    if (tid < MI_Q_BINS - 0x7F9) { const unsigned v = hc[0][0x7F9 + tid]; if (v) atomicAdd(&nan_sh, v); }
    unsigned prefix[2] = {0u, 0u}, rk[2] = {(unsigned)q.k_lo, (unsigned)q.k_hi};
    bool one = true;
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {
        if (ps > 0) {
            __syncthreads();
            for (int i = tid; i < 2 * MI_Q_BINS; i += SG_NT) (&lh[0][0])[i] = 0u;
            __syncthreads();
            one = prefix[0] == prefix[1];          // both ranks in one bin so far (the usual case: neighbours): one histogram serves both
#pragma unroll
            for (int u = 0; u < SG_MAXQ; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (q0 + tid + u * SG_NT < nq) radix_count(lh, x0v[u][e], ps, prefix[0], prefix[1], !one);
            if (!exchange(ps, 2 * ps - 1, one ? 1 : 2)) { poison(); return; }
        }
#pragma unroll
        for (int sel = 0; sel < 2; ++sel) {
            unsigned bin, rr;
            q_find_bin(&hc[one ? 0 : sel][0], rk[sel], scratch, bin, rr, tid < 256);
            prefix[sel] = (prefix[sel] << q_bits(ps)) | bin;
            rk[sel] = rr;
        }
    }
    float a, bb;
    const float sq = threshold_from_ranks(prefix[0], prefix[1], nan_sh, q.w, a, bb);
    if (tid == 0 && g == 0) {
        if (q.s_out) q.s_out[b] = sq;
        if (q.v_out) { q.v_out[2 * b] = a; q.v_out[2 * b + 1] = bb; }
    }
    const float s = threshold_scale(sq);
    const int k = (pp.T - 1) - t;
#pragma unroll
    for (int u = 0; u < SG_MAXQ; ++u) {
        const int qd = q0 + tid + u * SG_NT;
        if (qd >= nq) continue;
        float z[4], r[4], pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        step_noise4(pp, b, k, qd, n, true, z);
        if constexpr (HISTORY) ld_quad(prev + ob, 4 * qd, n, true, pv);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = posterior_elem<HISTORY>(x0v[u][e], xtv[u][e], z[e], s, cf, pv[e]);
        if constexpr (INPAINT) known_step4(ip, pp, b, t, k, qd, n, true, r);
        st_quad(pp.x + ob, 4 * qd, n, true, r);
        if constexpr (HISTORY) st_quad(prev + ob, 4 * qd, n, true, pv);
    }
}

}  // namespace

extern "C" int mi_cfg_x0_fwd(const mi_cfg_x0_params* p, void* stream) {
    if (p->B <= 0 || p->n <= 0) { mi_set_error("mi_cfg_x0_fwd: empty"); return MI_ERR_INVALID; }
    if (p->x0 && (!p->x_t || !p->coef || !p->t_state)) { mi_set_error("mi_cfg_x0_fwd: x0 needs x_t, coef, t_state"); return MI_ERR_INVALID; }
    if (p->hist0 && !p->x0) { mi_set_error("mi_cfg_x0_fwd: hist0 needs x0"); return MI_ERR_INVALID; }
    if (p->hist0) hipLaunchKernelGGL(HIP_KERNEL_NAME(cfg_x0_kernel<true>), dim3(grid_for(p->n, 128), p->B), dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(cfg_x0_kernel<false>), dim3(grid_for(p->n, 256), p->B), dim3(256), 0, (hipStream_t)stream, *p);
    return mi_check_launch("cfg_x0_kernel");
}

extern "C" int mi_quantile_fwd(const mi_quantile_params* p, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (p->B <= 0 || p->n <= 0 || p->k_lo < 0 || p->k_hi >= p->n || p->k_lo > p->k_hi) { mi_set_error("mi_quantile_fwd: bad ranks"); return MI_ERR_INVALID; }
    if (p->pass0_done && !p->self_cleaning) { mi_set_error("mi_quantile_fwd: pass0_done needs self_cleaning (the memset would erase pass 0)"); return MI_ERR_INVALID; }
    if (!p->self_cleaning && hipMemsetAsync(p->hist, 0, (size_t)3 * p->B * 2 * MI_Q_BINS * sizeof(unsigned), st) != hipSuccess) { mi_set_error("mi_quantile_fwd: memset failed"); return MI_ERR_LAUNCH; }
    const dim3 grid(grid_for((p->n + 15) / 16, Q_WGS), p->B);        // few workgroups per image: every one flushes its histogram with atomics
    if (!p->pass0_done) hipLaunchKernelGGL(HIP_KERNEL_NAME(quantile_hist_kernel<0>), grid, dim3(256), 0, st, *p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(quantile_hist_kernel<1>), grid, dim3(256), 0, st, *p);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(quantile_hist_kernel<2>), grid, dim3(256), 0, st, *p);
    hipLaunchKernelGGL(quantile_finish_kernel, dim3(p->B), dim3(256), 0, st, *p);
    return mi_check_launch("quantile kernels");
}

// what the fused tails ask of their parameter blocks (the blocks of the separate kernels, describing ONE step); q == NULL: a tail without
// the select (mi_sampler_step_direct_fwd)
static int check_step_params(const char* name, const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp) {
    if (c->B <= 0 || c->n <= 0 || pp->B != c->B || pp->n != c->n || (q && (q->B != c->B || q->n != c->n))) { mi_set_error("%s: inconsistent B / n", name); return MI_ERR_INVALID; }
    if (!c->x_t || !c->coef || !c->t_state || !pp->x || c->t_state != pp->t_state || c->t_off != pp->t_off || c->coef != pp->coef || c->x_t != pp->x) {
        mi_set_error("%s: needs x_t == x, one coef table and one t_state / t_off for the step", name); return MI_ERR_INVALID;
    }
    if (q && (q->k_lo < 0 || q->k_hi >= q->n || q->k_lo > q->k_hi)) { mi_set_error("%s: bad ranks", name); return MI_ERR_INVALID; }
    return MI_OK;
}

// what the inpainting entries ask of their block (ip may be NULL: the entry is then its *_ext_fwd form)
static int check_inpaint_params(const char* name, const mi_inpaint_params* ip, int n) {
    if (!ip) return MI_OK;
    if (!ip->known || !ip->mask) { mi_set_error("%s: inpaint block without known image / mask", name); return MI_ERR_INVALID; }
    if (ip->hw <= 0 || n % ip->hw != 0) { mi_set_error("%s: inpaint block with hw = %d for n = %d (n must be a multiple of hw > 0)", name, ip->hw, n); return MI_ERR_INVALID; }
    return MI_OK;
}

static int sampler_step_small(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e,
                              const mi_inpaint_params* ip, void* stream) {
    if (const int rc = check_step_params("mi_sampler_step_small_fwd", c, q, pp)) return rc;
    if (const int rc = check_inpaint_params("mi_sampler_step_small_inpaint_fwd", ip, c->n)) return rc;
    if (c->n > MI_SAMPLER_SMALL_N) { mi_set_error("mi_sampler_step_small_fwd: n = %d > %d", c->n, MI_SAMPLER_SMALL_N); return MI_ERR_UNSUPPORTED; }
    const dim3 grid(c->B), wg(SS_NT);
    hipStream_t st = (hipStream_t)stream;
    if (e && ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_small_kernel<true, true, mi_sampler_ext_params, mi_inpaint_params>), grid, wg, 0, st, *c, *q, *pp, *e, *ip);
    else if (ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_small_kernel<false, true, mi_inpaint_params>), grid, wg, 0, st, *c, *q, *pp, *ip);
    else if (e) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_small_kernel<true, false, mi_sampler_ext_params>), grid, wg, 0, st, *c, *q, *pp, *e);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_small_kernel<false, false>), grid, wg, 0, st, *c, *q, *pp);
    return mi_check_launch("sampler_small_kernel");
}
extern "C" int mi_sampler_step_small_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, void* stream) {
    return sampler_step_small(c, q, pp, nullptr, nullptr, stream);
}
// the *_ext_fwd entries: with e->x0_prev the history kernels, without it (or without e) exactly the plain entries
extern "C" int mi_sampler_step_small_ext_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e, void* stream) {
    return sampler_step_small(c, q, pp, (e && e->x0_prev) ? e : nullptr, nullptr, stream);
}
// the *_inpaint_fwd entries: the *_ext_fwd entry plus the masked replace of the known region; without ip exactly the *_ext_fwd entry
extern "C" int mi_sampler_step_small_inpaint_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e,
                                                 const mi_inpaint_params* ip, void* stream) {
    return sampler_step_small(c, q, pp, (e && e->x0_prev) ? e : nullptr, ip, stream);
}

extern "C" int mi_sampler_group_size(int n) {
    if (n <= 0 || (n & 3)) return 0;
    const int g = ((n >> 2) + SG_NT * SG_MAXQ - 1) / (SG_NT * SG_MAXQ);
    return g <= 256 ? g : 0;
}
extern "C" long long mi_sampler_group_sync_bytes(int B, int n) {
    return (B > 0 && mi_sampler_group_size(n) > 0) ? sg_sync_layout(B).total : 0;
}
static int sampler_step_group(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e,
                              const mi_inpaint_params* ip, void* sync, void* stream) {
    if (const int rc = check_step_params("mi_sampler_step_group_fwd", c, q, pp)) return rc;
    if (const int rc = check_inpaint_params("mi_sampler_step_group_inpaint_fwd", ip, c->n)) return rc;
    const int G = mi_sampler_group_size(c->n);
    if (!G) { mi_set_error("mi_sampler_step_group_fwd: n = %d unsupported (a multiple of 4, at most %d)", c->n, 256 * SG_NT * SG_MAXQ * 4); return MI_ERR_UNSUPPORTED; }
    if (!sync) { mi_set_error("mi_sampler_step_group_fwd: sync buffer missing"); return MI_ERR_INVALID; }
    const dim3 grid(c->B * G), wg(SG_NT);
    hipStream_t st = (hipStream_t)stream;
    if (e && ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_group_kernel<true, true, mi_sampler_ext_params, mi_inpaint_params>), grid, wg, 0, st, *c, *q, *pp, (char*)sync, G, *e, *ip);
    else if (ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_group_kernel<false, true, mi_inpaint_params>), grid, wg, 0, st, *c, *q, *pp, (char*)sync, G, *ip);
    else if (e) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_group_kernel<true, false, mi_sampler_ext_params>), grid, wg, 0, st, *c, *q, *pp, (char*)sync, G, *e);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_group_kernel<false, false>), grid, wg, 0, st, *c, *q, *pp, (char*)sync, G);
    return mi_check_launch("sampler_group_kernel");
}
extern "C" int mi_sampler_step_group_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, void* sync, void* stream) {
    return sampler_step_group(c, q, pp, nullptr, nullptr, sync, stream);
}
extern "C" int mi_sampler_step_group_ext_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e, void* sync, void* stream) {
    return sampler_step_group(c, q, pp, (e && e->x0_prev) ? e : nullptr, nullptr, sync, stream);
}
extern "C" int mi_sampler_step_group_inpaint_fwd(const mi_cfg_x0_params* c, const mi_quantile_params* q, const mi_posterior_params* pp, const mi_sampler_ext_params* e,
                                                 const mi_inpaint_params* ip, void* sync, void* stream) {
    return sampler_step_group(c, q, pp, (e && e->x0_prev) ? e : nullptr, ip, sync, stream);
}

static int posterior_step(const char* name, const mi_posterior_params* p, const mi_sampler_ext_params* e, const mi_inpaint_params* ip, void* stream) {
    if (p->B <= 0 || p->n <= 0) { mi_set_error("%s: empty", name); return MI_ERR_INVALID; }
    if (const int rc = check_inpaint_params(name, ip, p->n)) return rc;
    const dim3 grid(grid_for((p->n + 3) / 4, 256), p->B), wg(256);
    hipStream_t st = (hipStream_t)stream;
    if (e && ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(posterior_kernel<true, true, mi_sampler_ext_params, mi_inpaint_params>), grid, wg, 0, st, *p, *e, *ip);
    else if (ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(posterior_kernel<false, true, mi_inpaint_params>), grid, wg, 0, st, *p, *ip);
    else if (e) hipLaunchKernelGGL(HIP_KERNEL_NAME(posterior_kernel<true, false, mi_sampler_ext_params>), grid, wg, 0, st, *p, *e);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(posterior_kernel<false, false>), grid, wg, 0, st, *p);
    return mi_check_launch("posterior_kernel");
}
extern "C" int mi_posterior_fwd(const mi_posterior_params* p, void* stream) {
    return posterior_step("mi_posterior_fwd", p, nullptr, nullptr, stream);
}
extern "C" int mi_posterior_ext_fwd(const mi_posterior_params* p, const mi_sampler_ext_params* e, void* stream) {
    return (e && e->x0_prev) ? posterior_step("mi_posterior_ext_fwd", p, e, nullptr, stream) : posterior_step("mi_posterior_fwd", p, nullptr, nullptr, stream);
}
extern "C" int mi_posterior_inpaint_fwd(const mi_posterior_params* p, const mi_sampler_ext_params* e, const mi_inpaint_params* ip, void* stream) {
    if (!ip) return mi_posterior_ext_fwd(p, e, stream);
    return posterior_step("mi_posterior_inpaint_fwd", p, (e && e->x0_prev) ? e : nullptr, ip, stream);
}

// the tail without the select: one launch over (chunks, B); e without x0_prev (or NULL) and ip == NULL choose the plain instantiations
template <int CLIP>
static void sampler_step_direct(const mi_cfg_x0_params* c, const mi_posterior_params* pp, const mi_sampler_ext_params* e, const mi_inpaint_params* ip, hipStream_t st) {
    const dim3 grid(grid_for((c->n + 3) / 4, 256), c->B), wg(256);
    if (e && ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_direct_kernel<CLIP, true, true, mi_sampler_ext_params, mi_inpaint_params>), grid, wg, 0, st, *c, *pp, *e, *ip);
    else if (ip) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_direct_kernel<CLIP, false, true, mi_inpaint_params>), grid, wg, 0, st, *c, *pp, *ip);
    else if (e) hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_direct_kernel<CLIP, true, false, mi_sampler_ext_params>), grid, wg, 0, st, *c, *pp, *e);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(sampler_direct_kernel<CLIP, false, false>), grid, wg, 0, st, *c, *pp);
}
extern "C" int mi_sampler_step_direct_fwd(const mi_cfg_x0_params* c, const mi_posterior_params* pp, const mi_sampler_ext_params* e, const mi_inpaint_params* ip, int clip,
                                          void* stream) {
    if (clip != CLIP_STATIC && clip != CLIP_NONE) { mi_set_error("mi_sampler_step_direct_fwd: clip = %d (1: static clamp to [-1, 1], 0: none)", clip); return MI_ERR_INVALID; }
    if (const int rc = check_step_params("mi_sampler_step_direct_fwd", c, nullptr, pp)) return rc;
    if (const int rc = check_inpaint_params("mi_sampler_step_direct_fwd", ip, c->n)) return rc;
    if (!(e && e->x0_prev)) e = nullptr;
    if (clip == CLIP_STATIC) sampler_step_direct<CLIP_STATIC>(c, pp, e, ip, (hipStream_t)stream);
    else sampler_step_direct<CLIP_NONE>(c, pp, e, ip, (hipStream_t)stream);
    return mi_check_launch("sampler_direct_kernel");
}

// blend 0 and the per-stage preparation of an inpainting call
extern "C" int mi_inpaint_blend0_fwd(float* x, int B, int n, const mi_inpaint_params* ip, float a, float b, uint64_t seed, int sample0, void* stream) {
    if (!x || B <= 0 || n <= 0 || !ip) { mi_set_error("mi_inpaint_blend0_fwd: empty"); return MI_ERR_INVALID; }
    if (const int rc = check_inpaint_params("mi_inpaint_blend0_fwd", ip, n)) return rc;
    hipLaunchKernelGGL(known_blend0_kernel, dim3(grid_for((n + 3) / 4, 256), B), dim3(256), 0, (hipStream_t)stream, x, B, n, *ip, a, b, (unsigned long long)seed, sample0);
    return mi_check_launch("known_blend0_kernel");
}
extern "C" int mi_inpaint_prepare_fwd(const float* img, float* known, int B, int n, int normalize, const unsigned char* mask_in, int Hin, int Win, unsigned char* mask_out,
                                      int size, void* stream) {
    if (!img || !known || !mask_in || !mask_out || B <= 0 || n <= 0 || Hin <= 0 || Win <= 0 || size <= 0 || n % (size * size) != 0) {
        mi_set_error("mi_inpaint_prepare_fwd: bad params"); return MI_ERR_INVALID;
    }
    hipLaunchKernelGGL(known_image_kernel, dim3(grid_for((long long)B * n)), dim3(256), 0, (hipStream_t)stream, img, known, (long long)B * n, normalize);
    hipLaunchKernelGGL(known_mask_kernel, dim3(grid_for((long long)size * size, 256), B), dim3(256), 0, (hipStream_t)stream, mask_in, mask_out, Hin, Win, size);
    return mi_check_launch("known_image_kernel / known_mask_kernel");
}

// set: 0 advance by 1 | 1 set to value | 2 advance by value; `mapped`: the entries that take the step -> timestep map from e
static int step_launch(int* t_state, int64_t* times, int B, int set, int value, bool mapped, const mi_sampler_ext_params* e, void* stream) {
    if (mapped && (!e || !e->t_map)) { mi_set_error("mapped step kernels: t_map missing"); return MI_ERR_INVALID; }
    if (mapped) hipLaunchKernelGGL(step_advance_kernel<true>, dim3(1), dim3(64), 0, (hipStream_t)stream, t_state, (long long*)times, B, set, value, e->t_map);
    else hipLaunchKernelGGL(step_advance_kernel<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, t_state, (long long*)times, B, set, value, (const int*)nullptr);
    return mi_check_launch(mapped ? "step_advance_mapped_kernel" : "step_advance_kernel");
}
extern "C" int mi_step_advance(int* t_state, int64_t* times, int B, void* stream) {
    return step_launch(t_state, times, B, 0, 0, false, nullptr, stream);
}
extern "C" int mi_step_advance_by(int* t_state, int64_t* times, int B, int n, void* stream) {
    return step_launch(t_state, times, B, 2, n, false, nullptr, stream);
}
extern "C" int mi_step_set(int* t_state, int64_t* times, int B, int value, void* stream) {
    return step_launch(t_state, times, B, 1, value, false, nullptr, stream);
}
extern "C" int mi_step_advance_mapped(int* t_state, int64_t* times, int B, const mi_sampler_ext_params* e, void* stream) {
    return step_launch(t_state, times, B, 0, 0, true, e, stream);
}
extern "C" int mi_step_advance_by_mapped(int* t_state, int64_t* times, int B, int n, const mi_sampler_ext_params* e, void* stream) {
    if (n <= 0) { mi_set_error("mi_step_advance_by_mapped: n = %d", n); return MI_ERR_INVALID; }
    return step_launch(t_state, times, B, 2, n, true, e, stream);
}
extern "C" int mi_step_set_mapped(int* t_state, int64_t* times, int B, int value, const mi_sampler_ext_params* e, void* stream) {
    if (value < 0) { mi_set_error("mi_step_set_mapped: step %d", value); return MI_ERR_INVALID; }
    return step_launch(t_state, times, B, 1, value, true, e, stream);
}

extern "C" int mi_randn_fill(float* out, int B, int n, uint64_t seed, int sample0, int stream_id, void* stream) {
    hipLaunchKernelGGL(randn_fill_kernel, dim3(grid_for((n + 3) / 4, 256), B), dim3(256), 0, (hipStream_t)stream, out, n, (unsigned long long)seed, sample0, stream_id);
    return mi_check_launch("randn_fill_kernel");
}

extern "C" int mi_init_noise_fwd(const float* img_at_size, float* x, int B, int n, int normalize, float a, float b, uint64_t seed, int sample0, int stream_id,
                                 const float* noise, void* stream) {
    if (!img_at_size || !x || B <= 0 || n <= 0) { mi_set_error("mi_init_noise_fwd: empty"); return MI_ERR_INVALID; }
    const uintptr_t bits = (uintptr_t)img_at_size | (uintptr_t)x | (uintptr_t)noise;
    const int vec = ((n & 3) == 0 && (bits & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(init_noise_kernel, dim3(grid_for((n + 3) / 4, 256), B), dim3(256), 0, (hipStream_t)stream, img_at_size, x, n, normalize, a, b,
                       (unsigned long long)seed, sample0, stream_id, noise, vec);
    return mi_check_launch("init_noise_kernel");
}

extern "C" int mi_finalize_images(const float* x, float* out, int64_t total, int unnormalize, void* stream) {
    hipLaunchKernelGGL(finalize_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)total, unnormalize);
    return mi_check_launch("finalize_kernel");
}

extern "C" int mi_lowres_augment(const float* img, const float* noise, float* out, int64_t total, float a, float b, int normalize, void* stream) {
    hipLaunchKernelGGL(lowres_augment_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, img, noise, out, (long long)total, a, b, normalize);
    return mi_check_launch("lowres_augment_kernel");
}

extern "C" int mi_resize_fwd(const mi_resize_params* p, void* stream) {
    if (p->planes <= 0 || p->KH <= 0 || p->KW <= 0) { mi_set_error("mi_resize_fwd: bad params"); return MI_ERR_INVALID; }
    hipLaunchKernelGGL(resize_kernel, dim3(grid_for((long long)p->Hout * p->Wout, 1024), p->planes), dim3(256), 0, (hipStream_t)stream, *p);
    return mi_check_launch("resize_kernel");
}

// ------------------------------------------------------------------ HIP graphs
extern "C" int mi_graph_begin(void* stream) {
    if (hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed) != hipSuccess) { mi_set_error("hipStreamBeginCapture failed"); return MI_ERR_LAUNCH; }
    return MI_OK;
}
extern "C" int mi_graph_end(void* stream, void** graph_exec) {
    hipGraph_t g = nullptr;
    if (hipStreamEndCapture((hipStream_t)stream, &g) != hipSuccess || g == nullptr) { mi_set_error("hipStreamEndCapture failed"); return MI_ERR_LAUNCH; }
    hipGraphExec_t ge = nullptr;
    const hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { mi_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e)); return MI_ERR_LAUNCH; }
    *graph_exec = (void*)ge;
    return MI_OK;
}
extern "C" int mi_graph_launch(void* graph_exec, void* stream) {
    const hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
    if (e != hipSuccess) { mi_set_error("hipGraphLaunch failed: %s", hipGetErrorString(e)); return MI_ERR_LAUNCH; }
    return MI_OK;
}
extern "C" int mi_graph_destroy(void* graph_exec) {
    if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
    return MI_OK;
}
