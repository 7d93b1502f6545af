// Multi-tensor Adam step for the training path (the reference: train.py:99-100 torch.optim.Adam(imagen.parameters(), lr),
// stepped in training.py:375-377).  ONE launch updates every parameter of the model: the tensors are described by a device-resident
// table, the grid is a list of fixed-size chunks (tensor index, offset).  Same update as torch.optim.Adam (no amsgrad):
//     m <- m + (g - m) (1 - beta1)            v <- beta2 v + (1 - beta2) g g            [g <- g + weight_decay p first, if any]
//     p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// in that operation order and in fp32 like ATen's kernels; HBM-bound (16 bytes read, 12 written per element).
// Exponential moving average of the weights, same launch geometry: e <- e + (p - e) (1 - decay), alone (mi_ema_update), inside the
// Adam launch on the new p (mi_adam_ema_step: the same bits as the two launches), and the exchange of p and e (mi_ema_swap).
// Gradient-norm clip (the reference: training.py:363-377 clip_grad_norm_(params, 50)), same tables: per-chunk sums of squares in
// fp64 (mi_grad_sumsq), a one-workgroup finish that writes the norm and torch's coefficient (mi_grad_clip_coef), and either the in-place
// scaling (mi_grad_scale) or nothing at all -- adam_kernel / adam_ema_kernel read the coefficient through grad_scale.
#include "common.hip.h"

namespace {

// one element of torch.optim.Adam's update, the same text in adam_kernel and adam_ema_kernel so that both round alike
#define MI_ADAM_ELEMENT(a, g, p, m, v)                                                                                              \
    if ((a).weight_decay != 0.0f) g = fmaf((a).weight_decay, p, g);                                                                 \
    m = fmaf(g - m, (a).one_minus_beta1, m);                              /* lerp_ */                                               \
    v = fmaf(g * (a).one_minus_beta2, g, v * (a).beta2);                  /* mul_(beta2).addcmul_(g, g, 1 - beta2) */               \
    const float denom = sqrtf(v) / bc2_sqrt + (a).eps;                                                                              \
    p = p - step_size * (m / denom);                                      /* addcdiv_(m, denom, -step_size) */

// e <- e + (p - e) w; w == 1 is the exact copy ((p - e) + e is not p in fp32)
__device__ __forceinline__ float ema_element(float e, float p, float w) { return w == 1.0f ? p : fmaf(p - e, w, e); }

__global__ __launch_bounds__(256) void adam_kernel(const mi_adam_params a) {
    const int c = blockIdx.x;
    const mi_adam_tensor t = a.tensors[a.chunk_tensor[c]];
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    const float gs = a.grad_scale ? *a.grad_scale : 1.0f;
    const float step_size = a.lr / a.bias_correction1, bc2_sqrt = sqrtf(a.bias_correction2);
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        float g = t.g[i] * gs, p = t.p[i], m = t.m[i], v = t.v[i];
        MI_ADAM_ELEMENT(a, g, p, m, v)
        t.p[i] = p; t.m[i] = m; t.v[i] = v;
    }
}

// adam_kernel with the shadow's lerp on the new p while it is in registers: 20 bytes read, 16 written per element
__global__ __launch_bounds__(256) void adam_ema_kernel(const mi_adam_params a, const mi_ema_params sh) {
    const int c = blockIdx.x, k = a.chunk_tensor[c];
    const mi_adam_tensor t = a.tensors[k];
    const mi_ema_tensor s = sh.tensors[k];
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    const float gs = a.grad_scale ? *a.grad_scale : 1.0f;
    const float step_size = a.lr / a.bias_correction1, bc2_sqrt = sqrtf(a.bias_correction2);
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        float g = t.g[i] * gs, p = t.p[i], m = t.m[i], v = t.v[i];
        const float e = s.e[i];
        MI_ADAM_ELEMENT(a, g, p, m, v)
        t.p[i] = p; t.m[i] = m; t.v[i] = v;
        s.e[i] = ema_element(e, p, sh.w);
    }
}

__global__ __launch_bounds__(256) void ema_update_kernel(const mi_ema_params a) {
    const int c = blockIdx.x;
    const mi_ema_tensor t = a.tensors[a.chunk_tensor[c]];
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) t.e[i] = ema_element(t.e[i], t.p[i], a.w);
}

// exchange as 32-bit words: NaN payloads and the sign of zero pass through untouched
__global__ __launch_bounds__(256) void ema_swap_kernel(const mi_ema_params a) {
    const int c = blockIdx.x;
    const mi_ema_tensor t = a.tensors[a.chunk_tensor[c]];
    unsigned* const e = (unsigned*)t.e;
    unsigned* const p = (unsigned*)t.p;
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        const unsigned x = e[i], y = p[i];
        e[i] = y; p[i] = x;
    }
}

// sum of g*g over one chunk, in fp64 from the first element (an fp32 square overflows above |g| = 1.8e19 and vanishes below 1e-23; the kernel
// is its read stream either way).  Two accumulators per thread: the fp64 fma chain of 16 elements would otherwise serialise.  16-byte loads
// when the chunk's first element is 16-byte aligned (an allocator's base + a multiple of 4096 elements), adam_kernel's dword loop otherwise
// (a sliced gradient such as buf[1:]) and for the tail.  No atomics: partials[c] depends on chunk c alone, in a fixed order.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const mi_adam_params a, double* partials) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    const mi_adam_tensor t = a.tensors[a.chunk_tensor[c]];
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    double s0 = 0.0, s1 = 0.0;
    long long i = i0;
    if (i0 < i1 && (reinterpret_cast<size_t>(t.g + i0) & 15) == 0) {
        const long long nv = (i1 - i0) >> 2;
#pragma unroll 4
        for (long long k = threadIdx.x; k < nv; k += 256) {
            const float4 u = mi_ldg4(t.g + i0 + 4 * k);
            const double x = (double)u.x, y = (double)u.y, z = (double)u.z, w = (double)u.w;
            s0 = fma(x, x, s0); s1 = fma(y, y, s1); s0 = fma(z, z, s0); s1 = fma(w, w, s1);
        }
        i = i0 + 4 * nv;
    }
    for (long long j = i + threadIdx.x; j < i1; j += 512) {
        const double x = (double)t.g[j];
        s0 = fma(x, x, s0);
        if (j + 256 < i1) { const double y = (double)t.g[j + 256]; s1 = fma(y, y, s1); }
    }
    double s = s0 + s1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ONE workgroup of T threads: S = partials[0] + ... + partials[n - 1] (+ *extra) in a fixed order, out[0] = the norm, out[1] = torch's
// clip coefficient min(1, max_norm / (norm + 1e-6)).  A NaN sum gives a NaN coefficient (fmin would swallow it), an infinite one gives 0.
template <int T>
__global__ __launch_bounds__(T) void grad_coef_kernel(const double* partials, long long n, const double* extra, float max_norm, float* out) {
    __shared__ double red[T];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += T) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = T >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double S = red[0] + (extra ? *extra : 0.0);
        const double norm = sqrt(S);
        const double r = (double)max_norm / (norm + 1e-6);
        out[0] = (float)norm;
        out[1] = S != S ? (float)S : (float)(r < 1.0 ? r : 1.0);
    }
}

// g <- g * *grad_scale.  The coefficient is read first: a workgroup that finds exactly 1 (nothing to clip) touches neither table nor gradient.
__global__ __launch_bounds__(256) void grad_scale_kernel(const mi_adam_params a) {
    const float g1 = *a.grad_scale;
    if (g1 == 1.0f) return;
    unsigned gb = __float_as_uint(g1);
    MI_OPAQUE(gb);                                  // into a VGPR: no packed fp32 multiply with a scalar operand (csrc/Makefile)
    const float gs = __uint_as_float(gb);
    const int c = blockIdx.x;
    const mi_adam_tensor t = a.tensors[a.chunk_tensor[c]];
    float* const g = const_cast<float*>(t.g);
    const long long i0 = (long long)a.chunk_off[c] * a.chunk;
    const long long i1 = i0 + a.chunk < t.n ? i0 + a.chunk : t.n;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) g[i] = g[i] * gs;
}

bool adam_tables_ok(const mi_adam_params* a, const char* who) {
    if (!a || a->nchunks <= 0 || a->chunk <= 0 || !a->tensors || !a->chunk_tensor || !a->chunk_off) {
        mi_set_error("%s: empty / missing tables", who);
        return false;
    }
    return true;
}

bool ema_tables_ok(const mi_ema_params* a, const char* who) {
    if (!a || a->nchunks <= 0 || a->chunk <= 0 || !a->tensors || !a->chunk_tensor || !a->chunk_off) {
        mi_set_error("%s: empty / missing tables", who);
        return false;
    }
    return true;
}

bool ema_weight_ok(float w, const char* who) {
    if (!(w >= 0.0f && w <= 1.0f)) { mi_set_error("%s: w = 1 - decay must lie in [0, 1]", who); return false; }
    return true;
}

}  // namespace

extern "C" int mi_adam_step(const mi_adam_params* a, void* stream) {
    if (!a || a->nchunks <= 0 || a->chunk <= 0 || !a->tensors || !a->chunk_tensor || !a->chunk_off) { mi_set_error("mi_adam_step: empty / missing tables"); return MI_ERR_INVALID; }
    if (!(a->bias_correction1 > 0.0f) || !(a->bias_correction2 > 0.0f)) { mi_set_error("mi_adam_step: bias corrections must be positive (step >= 1)"); return MI_ERR_INVALID; }
    hipLaunchKernelGGL(adam_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a);
    return mi_check_launch("adam_kernel");
}

extern "C" int mi_adam_ema_step(const mi_adam_params* a, const mi_ema_params* e, void* stream) {
    if (!a || a->nchunks <= 0 || a->chunk <= 0 || !a->tensors || !a->chunk_tensor || !a->chunk_off) { mi_set_error("mi_adam_ema_step: empty / missing tables"); return MI_ERR_INVALID; }
    if (!e || !e->tensors) { mi_set_error("mi_adam_ema_step: empty / missing tables (shadows)"); return MI_ERR_INVALID; }
    if (!(a->bias_correction1 > 0.0f) || !(a->bias_correction2 > 0.0f)) { mi_set_error("mi_adam_ema_step: bias corrections must be positive (step >= 1)"); return MI_ERR_INVALID; }
    if (!ema_weight_ok(e->w, "mi_adam_ema_step")) return MI_ERR_INVALID;
    hipLaunchKernelGGL(adam_ema_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a, *e);
    return mi_check_launch("adam_ema_kernel");
}

extern "C" int mi_ema_update(const mi_ema_params* a, void* stream) {
    if (!ema_tables_ok(a, "mi_ema_update") || !ema_weight_ok(a->w, "mi_ema_update")) return MI_ERR_INVALID;
    hipLaunchKernelGGL(ema_update_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a);
    return mi_check_launch("ema_update_kernel");
}

extern "C" int mi_ema_swap(const mi_ema_params* a, void* stream) {
    if (!ema_tables_ok(a, "mi_ema_swap")) return MI_ERR_INVALID;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a);
    return mi_check_launch("ema_swap_kernel");
}

extern "C" int mi_grad_sumsq(const mi_adam_params* a, double* partials, void* stream) {
    if (!adam_tables_ok(a, "mi_grad_sumsq")) return MI_ERR_INVALID;
    if (!partials) { mi_set_error("mi_grad_sumsq: NULL partials"); return MI_ERR_INVALID; }
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a, partials);
    return mi_check_launch("grad_sumsq_kernel");
}

extern "C" int mi_grad_clip_coef(const double* partials, long long n, const double* extra, float max_norm, float* out, void* stream) {
    if (!out) { mi_set_error("mi_grad_clip_coef: NULL out"); return MI_ERR_INVALID; }
    if (n < 0) { mi_set_error("mi_grad_clip_coef: n must not be negative"); return MI_ERR_INVALID; }
    if (n > 0 && !partials) { mi_set_error("mi_grad_clip_coef: NULL partials"); return MI_ERR_INVALID; }
    if (n == 0 && !extra) { mi_set_error("mi_grad_clip_coef: nothing to sum (n == 0 and no extra)"); return MI_ERR_INVALID; }
    if (!(max_norm >= 0.0f)) { mi_set_error("mi_grad_clip_coef: max_norm must not be negative or NaN"); return MI_ERR_INVALID; }
    if (n > 4096) hipLaunchKernelGGL(grad_coef_kernel<1024>, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, n, extra, max_norm, out);
    else hipLaunchKernelGGL(grad_coef_kernel<256>, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, extra, max_norm, out);
    return mi_check_launch("grad_coef_kernel");
}

extern "C" int mi_grad_scale(const mi_adam_params* a, void* stream) {
    if (!adam_tables_ok(a, "mi_grad_scale")) return MI_ERR_INVALID;
    if (!a->grad_scale) { mi_set_error("mi_grad_scale: NULL grad_scale"); return MI_ERR_INVALID; }
    hipLaunchKernelGGL(grad_scale_kernel, dim3(a->nchunks), dim3(256), 0, (hipStream_t)stream, *a);
    return mi_check_launch("grad_scale_kernel");
}
