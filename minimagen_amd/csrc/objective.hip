// Front and loss of a training step for the prediction objectives (the reference trains the noise objective with a flat weight,
// Imagen.py:512-573): what the U-Net reads and what its output is compared with, for a U-Net that predicts eps, x0 or
// v = sqrt(abar) eps - sqrt(1 - abar) x0 (Salimans & Ho 2022), and the loss with a per-sample weight looked up by timestep on the device
// (min-SNR-gamma, Hang et al. 2023).
//   mi_diffuse_fwd          one launch: [2 x - 1] -> x_t = a x0 + s eps -> [the target]; every product and sum rounded on its own in the order of
//                           the torch expressions of Imagen._p_losses / GaussianDiffusion.q_sample / calculate_v: the same bits
//   mi_objective_loss_fwd   per-chunk sums of l(pred - target) in fp64, no atomics (the pattern of grad_sumsq_kernel), a one-workgroup finish that
//                           writes the loss as one fp32 on the device; the same pass writes g = w l'(d) / (B n) when a gradient is wanted
//   mi_objective_loss_bwd   dpred = g * *grad_out, grad_out read from device memory
// HBM-bound: 8 bytes read + 4 .. 8 written per element (front), 8 read + 0 .. 4 written (loss), 4 + 4 (backward).
#include "common.hip.h"

// the elementwise math must round like separate torch ops (as in sampler.hip): no a*b+c contraction in this file
#pragma clang fp contract(off)

namespace {

constexpr int OBJ_THREADS = 256;

// four consecutive floats of a row of n from element i (a multiple of 4): one 16-byte access when `vec`, element by element inside the row otherwise
__device__ __forceinline__ void obj_ld4(const float* row, int i, int n, bool vec, float (&v)[4]) {
    if (vec) { const float4 q = mi_ldg4(row + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (i + e < n) ? row[i + e] : 0.0f;
    }
}
__device__ __forceinline__ void obj_st4(float* row, int i, int n, bool vec, const float (&v)[4]) {
    if (vec) mi_stg4(row + i, make_float4(v[0], v[1], v[2], v[3]));
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
    }
}

// grid (chunks of MI_OBJECTIVE_CHUNK elements, B).  A timestep outside [0, T) reads no table row: its image comes out NaN.
__global__ __launch_bounds__(OBJ_THREADS) void diffuse_kernel(const mi_diffuse_params p, const int vec) {
    const int b = blockIdx.y;
    const long long t = p.times[b];
    const bool ok = t >= 0 && t < (long long)p.T;
    const float nanv = __uint_as_float(0x7FC00000u);
    const float a = ok ? p.table[2 * t] : nanv, s = ok ? p.table[2 * t + 1] : nanv;
    const size_t row = (size_t)b * (size_t)p.n;
    const float* x = p.x + row;
    const float* z = p.noise + row;
    float* xt = p.x_t + row;
    float* tg = p.target_kind != MI_TARGET_NONE ? p.target + row : nullptr;
    const int i0 = blockIdx.x * MI_OBJECTIVE_CHUNK;
    const int i1 = (p.n - i0 < MI_OBJECTIVE_CHUNK) ? p.n : i0 + MI_OBJECTIVE_CHUNK;
    for (int i = i0 + 4 * (int)threadIdx.x; i < i1; i += 4 * OBJ_THREADS) {
        float x0[4], e[4], o[4], g[4];
        obj_ld4(x, i, p.n, vec, x0);
        obj_ld4(z, i, p.n, vec, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p.normalize) x0[k] = __fsub_rn(__fmul_rn(x0[k], 2.0f), 1.0f);                     // helpers.normalize_neg_one_to_one
            o[k] = __fadd_rn(__fmul_rn(a, x0[k]), __fmul_rn(s, e[k]));                          // q_sample
            g[k] = p.target_kind == MI_TARGET_V ? __fsub_rn(__fmul_rn(a, e[k]), __fmul_rn(s, x0[k])) : x0[k];      // calculate_v | x_start
        }
        obj_st4(xt, i, p.n, vec, o);
        if (tg) obj_st4(tg, i, p.n, vec, g);
    }
}

__device__ __forceinline__ double loss_elem(double d, int loss_type) {
    const double ad = fabs(d);
    if (loss_type == MI_LOSS_L1) return ad;
    if (loss_type == MI_LOSS_L2) return d * d;
    return ad < 1.0 ? 0.5 * d * d : ad - 0.5;                     // smooth-l1, beta = 1 (a NaN difference takes the second arm and stays NaN)
}
__device__ __forceinline__ double loss_slope(double d, int loss_type) {
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);      // torch.sign: 0 at 0, NaN stays NaN
    if (loss_type == MI_LOSS_L1) return sg;
    if (loss_type == MI_LOSS_L2) return 2.0 * d;
    return fabs(d) < 1.0 ? d : sg;
}

// partials[b * gridDim.x + c] = w[times[b]] * sum over chunk c of image b of l(pred - target): the difference in fp32, l and the sum in fp64,
// two accumulators per work-item, a fixed reduction tree.  GRAD: plus g = w l'(d) / (B n), rounded once from fp64.
template <bool GRAD>
__global__ __launch_bounds__(OBJ_THREADS) void objective_loss_kernel(const mi_objective_loss_params p, const int vec) {
    __shared__ double red[OBJ_THREADS / 64];
    const int b = blockIdx.y;
    double w = 1.0;
    if (p.weights) {
        const long long t = p.times[b];
        w = (t >= 0 && t < (long long)p.T) ? (double)p.weights[t] : (double)__uint_as_float(0x7FC00000u);
    }
    const double gscale = w / ((double)p.B * (double)p.n);
    const size_t row = (size_t)b * (size_t)p.n;
    const float* pr = p.pred + row;
    const float* tg = p.target + row;
    float* gr = GRAD ? p.grad + row : nullptr;
    const int i0 = blockIdx.x * MI_OBJECTIVE_CHUNK;
    const int i1 = (p.n - i0 < MI_OBJECTIVE_CHUNK) ? p.n : i0 + MI_OBJECTIVE_CHUNK;
    double s0 = 0.0, s1 = 0.0;
    for (int i = i0 + 4 * (int)threadIdx.x; i < i1; i += 4 * OBJ_THREADS) {
        float a[4], c[4], g[4];
        obj_ld4(pr, i, p.n, vec, a);
        obj_ld4(tg, i, p.n, vec, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)__fsub_rn(a[k], c[k]);
            const double l = (i + k < i1) ? loss_elem(d, p.loss_type) : 0.0;
            if (k & 1) s1 += l; else s0 += l;
            if (GRAD) g[k] = (float)(gscale * loss_slope(d, p.loss_type));
        }
        if (GRAD) obj_st4(gr, i, p.n, vec, g);
    }
    double s = s0 + s1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) p.partials[(size_t)b * gridDim.x + blockIdx.x] = w * ((red[0] + red[1]) + (red[2] + red[3]));
}

// ONE workgroup: loss = (partials[0] + ... + partials[count - 1]) / (B n) in a fixed order (grad_coef_kernel's pattern), written as one fp32
__global__ __launch_bounds__(OBJ_THREADS) void objective_loss_finish_kernel(const double* partials, int count, double inv_count, float* loss) {
    __shared__ double red[OBJ_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += OBJ_THREADS) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = OBJ_THREADS >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * inv_count);
}

__global__ __launch_bounds__(OBJ_THREADS) void objective_loss_bwd_kernel(const float* g, const float* grad_out, float* dpred, long long count, const int vec) {
    unsigned ub = __float_as_uint(*grad_out);
    MI_OPAQUE(ub);                                  // into a VGPR: no packed fp32 multiply with a scalar operand (csrc/Makefile)
    const float u = __uint_as_float(ub);
    const long long i0 = (long long)blockIdx.x * MI_OBJECTIVE_CHUNK;
    const long long i1 = (count - i0 < MI_OBJECTIVE_CHUNK) ? count : i0 + MI_OBJECTIVE_CHUNK;
    for (long long i = i0 + 4 * (long long)threadIdx.x; i < i1; i += 4 * OBJ_THREADS) {
        if (vec) {
            const float4 q = mi_ldg4(g + i);
            mi_stg4(dpred + i, make_float4(__fmul_rn(q.x, u), __fmul_rn(q.y, u), __fmul_rn(q.z, u), __fmul_rn(q.w, u)));
        } else {
            for (long long e = i; e < i + 4 && e < i1; ++e) dpred[e] = __fmul_rn(g[e], u);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mi_objective_chunks(int n) { return n <= 0 ? 0 : (n + MI_OBJECTIVE_CHUNK - 1) / MI_OBJECTIVE_CHUNK; }

extern "C" int mi_diffuse_fwd(const mi_diffuse_params* p, void* stream) {
    if (!p || p->B <= 0 || p->n <= 0 || p->T <= 0) { mi_set_error("mi_diffuse_fwd: B, n and T must be positive"); return MI_ERR_INVALID; }
    if (!p->x || !p->noise || !p->times || !p->table || !p->x_t) { mi_set_error("mi_diffuse_fwd: NULL x / noise / times / table / x_t"); return MI_ERR_INVALID; }
    if (p->target_kind != MI_TARGET_NONE && p->target_kind != MI_TARGET_V && p->target_kind != MI_TARGET_X_START) {
        mi_set_error("mi_diffuse_fwd: target_kind must be MI_TARGET_NONE, MI_TARGET_V or MI_TARGET_X_START");
        return MI_ERR_INVALID;
    }
    if (p->target_kind != MI_TARGET_NONE && !p->target) { mi_set_error("mi_diffuse_fwd: a target is asked for but target is NULL"); return MI_ERR_INVALID; }
    if (p->B > 65535 || p->n > (1 << 30)) { mi_set_error("mi_diffuse_fwd: B must not exceed 65535, n 2^30"); return MI_ERR_INVALID; }
    const int vec = (p->n % 4 == 0) && aligned16(p->x) && aligned16(p->noise) && aligned16(p->x_t) && aligned16(p->target);
    hipLaunchKernelGGL(diffuse_kernel, dim3(mi_objective_chunks(p->n), p->B), dim3(OBJ_THREADS), 0, (hipStream_t)stream, *p, vec);
    return mi_check_launch("diffuse_kernel");
}

extern "C" int mi_objective_loss_fwd(const mi_objective_loss_params* p, void* stream) {
    if (!p || p->B <= 0 || p->n <= 0) { mi_set_error("mi_objective_loss_fwd: B and n must be positive"); return MI_ERR_INVALID; }
    if (!p->pred || !p->target || !p->partials || !p->loss) { mi_set_error("mi_objective_loss_fwd: NULL pred / target / partials / loss"); return MI_ERR_INVALID; }
    if (p->loss_type != MI_LOSS_L1 && p->loss_type != MI_LOSS_L2 && p->loss_type != MI_LOSS_SMOOTH_L1) {
        mi_set_error("mi_objective_loss_fwd: loss_type must be MI_LOSS_L1, MI_LOSS_L2 or MI_LOSS_SMOOTH_L1");
        return MI_ERR_INVALID;
    }
    if (p->weights && (!p->times || p->T <= 0)) { mi_set_error("mi_objective_loss_fwd: weights need times and T > 0"); return MI_ERR_INVALID; }
    if (p->B > 65535 || p->n > (1 << 30)) { mi_set_error("mi_objective_loss_fwd: B must not exceed 65535, n 2^30"); return MI_ERR_INVALID; }
    const int nc = mi_objective_chunks(p->n);
    if ((long long)nc * p->B > 0x7fffffffLL) { mi_set_error("mi_objective_loss_fwd: too many chunks"); return MI_ERR_INVALID; }
    const int vec = (p->n % 4 == 0) && aligned16(p->pred) && aligned16(p->target) && aligned16(p->grad);
    if (p->grad) hipLaunchKernelGGL(objective_loss_kernel<true>, dim3(nc, p->B), dim3(OBJ_THREADS), 0, (hipStream_t)stream, *p, vec);
    else hipLaunchKernelGGL(objective_loss_kernel<false>, dim3(nc, p->B), dim3(OBJ_THREADS), 0, (hipStream_t)stream, *p, vec);
    const int rc = mi_check_launch("objective_loss_kernel");
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(objective_loss_finish_kernel, dim3(1), dim3(OBJ_THREADS), 0, (hipStream_t)stream, (const double*)p->partials, nc * p->B,
                       1.0 / ((double)p->B * (double)p->n), p->loss);
    return mi_check_launch("objective_loss_finish_kernel");
}

extern "C" int mi_objective_loss_bwd(const float* g, const float* grad_out, float* dpred, long long count, void* stream) {
    if (!g || !grad_out || !dpred) { mi_set_error("mi_objective_loss_bwd: NULL g / grad_out / dpred"); return MI_ERR_INVALID; }
    if (count <= 0) { mi_set_error("mi_objective_loss_bwd: count must be positive"); return MI_ERR_INVALID; }
    const long long nc = (count + MI_OBJECTIVE_CHUNK - 1) / MI_OBJECTIVE_CHUNK;
    if (nc > 0x7fffffffLL) { mi_set_error("mi_objective_loss_bwd: too many chunks"); return MI_ERR_INVALID; }
    const int vec = (count % 4 == 0) && aligned16(g) && aligned16(dpred);
    hipLaunchKernelGGL(objective_loss_bwd_kernel, dim3((unsigned)nc), dim3(OBJ_THREADS), 0, (hipStream_t)stream, g, grad_out, dpred, count, vec);
    return mi_check_launch("objective_loss_bwd_kernel");
}
