// Guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", eq. 15-16): per image, with c
// the conditional and u the null / negative prediction,
//     g = u + (c - u) s        (rounded as guided_x0 of sampler.hip rounds it: __fsub_rn, __fmul_rn, __fadd_rn)
//     f = phi sigma(c) / sigma(g) + (1 - phi)         (standard deviations over the n elements of the image; f = 1 when sigma(g) == 0)
//     prediction = g f         (written over the conditional row: the sampler tails then read B guided rows, no combine)
// Two plain launches, no atomics, no workgroup waits for another (the pattern of mi_grad_sumsq -> mi_grad_clip_coef -> mi_grad_scale):
//   mi_cfg_rescale_stats_fwd   grid (chunks of MI_CFG_RESCALE_CHUNK elements, B): sum c, sum c^2, sum g, sum g^2 of one chunk in fp64 (a product of two
//                              fp32 values is exact there), a fixed reduction tree, one 4-double row of `partials` per workgroup
//   mi_cfg_rescale_apply_fwd   same grid: every workgroup re-adds its image's chunk rows in index order, forms f in fp64, rounds it to fp32 once and
//                              writes __fmul_rn(g, f) over its chunk of the conditional row (c and u of an element are read before it is written)
// The chunking depends on n alone, so an image's result does not depend on the batch it sits in or on the launch.  A NaN / inf in either half
// of an image makes that image's sums, its f and with it every element of its row NaN (fail-stop); the other images are untouched.
// HBM-bound: 2 B n 4 bytes read by each launch, B n 4 written by the second.
//
// Guidance schedules: the scale per step and per row from device memory, s = scale_tab[(*t_state - t_off) * B + b], so that one
// captured graph serves every step of a run and every later call's values.
//   mi_cfg_sched_combine_fwd         same grid: s == 1 ? c : g over the conditional row (the null rows are not written); reads 2 B n 4 bytes,
//                                    writes B n 4
//   mi_cfg_sched_rescale_stats_fwd / mi_cfg_sched_rescale_apply_fwd    the two launches above with the scale read from the table: ONE body each,
//                                    instantiated on the parameter block (scale_of below is all that differs)
#include "common.hip.h"

// g must round like the sampler tails' combine: no a*b+c contraction in this file
#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256;

// four consecutive floats of a row of n from element i (a multiple of 4): one 16-byte access when `vec`, element by element inside the row otherwise
__device__ __forceinline__ void rs_ld4(const float* row, int i, int n, bool vec, float (&v)[4]) {
    if (vec) { const float4 q = mi_ldg4(row + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (i + e < n) ? row[i + e] : 0.0f;
    }
}
__device__ __forceinline__ void rs_st4(float* row, int i, int n, bool vec, const float (&v)[4]) {
    if (vec) mi_stg4(row + i, make_float4(v[0], v[1], v[2], v[3]));
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
    }
}

__device__ __forceinline__ float guided(float c, float u, float s) { return __fadd_rn(u, __fmul_rn(__fsub_rn(c, u), s)); }     // Unet.py:506, as guided_x0

__device__ __forceinline__ float opaque(float v) {          // into a VGPR: no packed fp32 multiply with a scalar operand (csrc/Makefile)
    unsigned b = __float_as_uint(v);
    MI_OPAQUE(b);
    return __uint_as_float(b);
}

// where a launch's scale comes from: the launch scalar, or the step's row of the table (a wave-uniform load)
__device__ __forceinline__ float scale_of(const mi_cfg_rescale_params& p, int) { return opaque(p.cond_scale); }
__device__ __forceinline__ float scale_of(const mi_cfg_sched_params& p, int b) {
    return opaque(p.scale_tab[(size_t)(*p.t_state - p.t_off) * (size_t)p.B + (size_t)b]);
}

// partials[(b * gridDim.x + chunk) * 4 + {0, 1, 2, 3}] = sum c, sum c^2, sum g, sum g^2 over the chunk: two accumulators per work-item and
// statistic, a butterfly over the wave, the four waves added as (0 + 1) + (2 + 3)
template <class P>
__global__ __launch_bounds__(RS_THREADS) void cfg_rescale_stats_kernel(const P p, const int vec) {
    __shared__ double red[RS_THREADS / 64][4];
    const int b = blockIdx.y;
    const float s = scale_of(p, b);
    const float* cr = p.pred2 + (size_t)b * (size_t)p.n;
    const float* ur = p.pred2 + (size_t)(b + p.B) * (size_t)p.n;
    const int i0 = blockIdx.x * MI_CFG_RESCALE_CHUNK;
    const int i1 = (p.n - i0 < MI_CFG_RESCALE_CHUNK) ? p.n : i0 + MI_CFG_RESCALE_CHUNK;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int i = i0 + 4 * (int)threadIdx.x; i < i1; i += 4 * RS_THREADS) {
        float c[4], u[4];
        rs_ld4(cr, i, p.n, vec, c);
        rs_ld4(ur, i, p.n, vec, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = i + k < i1;
            const double cd = in ? (double)c[k] : 0.0, gd = in ? (double)guided(c[k], u[k], s) : 0.0;
            acc[k & 1][0] += cd;
            acc[k & 1][1] += cd * cd;
            acc[k & 1][2] += gd;
            acc[k & 1][3] += gd * gd;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = acc[0][k] + acc[1][k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        p.partials[((size_t)b * gridDim.x + blockIdx.x) * 4 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

template <class P>
__global__ __launch_bounds__(RS_THREADS) void cfg_rescale_apply_kernel(const P p, const int vec) {
    const int b = blockIdx.y, nc = gridDim.x;
    // the image's statistics: its chunk rows in index order (every work-item the same, wave-uniform loads)
    const double* row = p.partials + (size_t)b * nc * 4;
    double sc = 0.0, qc = 0.0, sg = 0.0, qg = 0.0;
    for (int k = 0; k < nc; ++k) {
        sc += row[4 * k];
        qc += row[4 * k + 1];
        sg += row[4 * k + 2];
        qg += row[4 * k + 3];
    }
    const double n = (double)p.n, mc = sc / n, mg = sg / n;
    double vc = qc / n - mc * mc, vg = qg / n - mg * mg;
    vc = vc < 0.0 ? 0.0 : vc;               // (a NaN stays a NaN through both selects)
    vg = vg < 0.0 ? 0.0 : vg;
    const double phi = (double)p.rescale;
    const float f = opaque(vg == 0.0 ? 1.0f : (float)(phi * (sqrt(vc) / sqrt(vg)) + (1.0 - phi)));
    const float s = scale_of(p, b);
    float* cr = p.pred2 + (size_t)b * (size_t)p.n;
    const float* ur = p.pred2 + (size_t)(b + p.B) * (size_t)p.n;
    const int i0 = blockIdx.x * MI_CFG_RESCALE_CHUNK;
    const int i1 = (p.n - i0 < MI_CFG_RESCALE_CHUNK) ? p.n : i0 + MI_CFG_RESCALE_CHUNK;
    for (int i = i0 + 4 * (int)threadIdx.x; i < i1; i += 4 * RS_THREADS) {
        float c[4], u[4], o[4];
        rs_ld4(cr, i, p.n, vec, c);
        rs_ld4(ur, i, p.n, vec, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __fmul_rn(guided(c[k], u[k], s), f);
        rs_st4(cr, i, p.n, vec, o);
    }
}

// the guided prediction of a step whose scale comes from the table, over the conditional row; a row at scale 1 keeps c to the bit
__global__ __launch_bounds__(RS_THREADS) void cfg_sched_combine_kernel(const mi_cfg_sched_params p, const int vec) {
    const int b = blockIdx.y;
    const float s = scale_of(p, b);
    float* cr = p.pred2 + (size_t)b * (size_t)p.n;
    const float* ur = p.pred2 + (size_t)(b + p.B) * (size_t)p.n;
    const int i0 = blockIdx.x * MI_CFG_RESCALE_CHUNK;
    const int i1 = (p.n - i0 < MI_CFG_RESCALE_CHUNK) ? p.n : i0 + MI_CFG_RESCALE_CHUNK;
    if (s == 1.0f) return;                  // (the whole workgroup: s is one value per image)
    for (int i = i0 + 4 * (int)threadIdx.x; i < i1; i += 4 * RS_THREADS) {
        float c[4], u[4], o[4];
        rs_ld4(cr, i, p.n, vec, c);
        rs_ld4(ur, i, p.n, vec, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = guided(c[k], u[k], s);
        rs_st4(cr, i, p.n, vec, o);
    }
}

int rs_check(const mi_cfg_rescale_params* p, const char* what) {
    if (!p || p->B <= 0 || p->n <= 0) { mi_set_error("%s: B and n must be positive", what); return MI_ERR_INVALID; }
    if (!p->pred2 || !p->partials) { mi_set_error("%s: NULL pred2 / partials", what); return MI_ERR_INVALID; }
    if (p->B > 65535 || p->n > (1 << 30)) { mi_set_error("%s: B must not exceed 65535, n 2^30", what); return MI_ERR_INVALID; }
    if (!(p->rescale >= 0.0f && p->rescale <= 1.0f)) { mi_set_error("%s: rescale must be in [0, 1]", what); return MI_ERR_INVALID; }
    if (!(p->cond_scale - p->cond_scale == 0.0f)) { mi_set_error("%s: cond_scale must be finite", what); return MI_ERR_INVALID; }
    return MI_OK;
}

int rs_check(const mi_cfg_sched_params* p, const char* what, bool rescale) {
    if (!p || p->B <= 0 || p->n <= 0) { mi_set_error("%s: B and n must be positive", what); return MI_ERR_INVALID; }
    if (!p->pred2 || !p->scale_tab || !p->t_state) { mi_set_error("%s: NULL pred2 / scale_tab / t_state", what); return MI_ERR_INVALID; }
    if (p->B > 65535 || p->n > (1 << 30)) { mi_set_error("%s: B must not exceed 65535, n 2^30", what); return MI_ERR_INVALID; }
    if (p->t_off < 0) { mi_set_error("%s: t_off must not be negative", what); return MI_ERR_INVALID; }
    if (!(p->rescale >= 0.0f && p->rescale <= 1.0f)) { mi_set_error("%s: rescale must be in [0, 1]", what); return MI_ERR_INVALID; }
    if (rescale && !p->partials) { mi_set_error("%s: NULL partials", what); return MI_ERR_INVALID; }
    return MI_OK;
}

template <class P>
int rs_vec(const P* p) { return (p->n % 4 == 0) && (reinterpret_cast<size_t>(p->pred2) & 15) == 0; }

}  // namespace

extern "C" int mi_cfg_rescale_chunks(int n) { return n <= 0 ? 0 : (n + MI_CFG_RESCALE_CHUNK - 1) / MI_CFG_RESCALE_CHUNK; }

extern "C" int mi_cfg_rescale_stats_fwd(const mi_cfg_rescale_params* p, void* stream) {
    const int rc = rs_check(p, "mi_cfg_rescale_stats_fwd");
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(cfg_rescale_stats_kernel<mi_cfg_rescale_params>, dim3(mi_cfg_rescale_chunks(p->n), p->B), dim3(RS_THREADS), 0, (hipStream_t)stream, *p, rs_vec(p));
    return mi_check_launch("cfg_rescale_stats_kernel");
}

extern "C" int mi_cfg_rescale_apply_fwd(const mi_cfg_rescale_params* p, void* stream) {
    const int rc = rs_check(p, "mi_cfg_rescale_apply_fwd");
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(cfg_rescale_apply_kernel<mi_cfg_rescale_params>, dim3(mi_cfg_rescale_chunks(p->n), p->B), dim3(RS_THREADS), 0, (hipStream_t)stream, *p, rs_vec(p));
    return mi_check_launch("cfg_rescale_apply_kernel");
}

extern "C" int mi_cfg_sched_combine_fwd(const mi_cfg_sched_params* p, void* stream) {
    const int rc = rs_check(p, "mi_cfg_sched_combine_fwd", false);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(cfg_sched_combine_kernel, dim3(mi_cfg_rescale_chunks(p->n), p->B), dim3(RS_THREADS), 0, (hipStream_t)stream, *p, rs_vec(p));
    return mi_check_launch("cfg_sched_combine_kernel");
}

extern "C" int mi_cfg_sched_rescale_stats_fwd(const mi_cfg_sched_params* p, void* stream) {
    const int rc = rs_check(p, "mi_cfg_sched_rescale_stats_fwd", true);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(cfg_rescale_stats_kernel<mi_cfg_sched_params>, dim3(mi_cfg_rescale_chunks(p->n), p->B), dim3(RS_THREADS), 0, (hipStream_t)stream, *p, rs_vec(p));
    return mi_check_launch("cfg_sched_rescale_stats_kernel");
}

extern "C" int mi_cfg_sched_rescale_apply_fwd(const mi_cfg_sched_params* p, void* stream) {
    const int rc = rs_check(p, "mi_cfg_sched_rescale_apply_fwd", true);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(cfg_rescale_apply_kernel<mi_cfg_sched_params>, dim3(mi_cfg_rescale_chunks(p->n), p->B), dim3(RS_THREADS), 0, (hipStream_t)stream, *p, rs_vec(p));
    return mi_check_launch("cfg_sched_rescale_apply_kernel");
}
