// Multi-tensor Adam step for the training path (the reference: train.py:99-100 torch.optim.Adam(imagen.parameters(), lr),
// stepped in training.py:375-377).  ONE launch updates every parameter of the model: the tensors are described by a device-resident
// table, the grid is a list of fixed-size chunks (tensor index, offset).  Same update as torch.optim.Adam (no amsgrad):
//     m <- m + (g - m) (1 - beta1)            v <- beta2 v + (1 - beta2) g g            [g <- g + weight_decay p first, if any]
//     p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// in that operation order and in fp32 like ATen's kernels; HBM-bound (16 bytes read, 12 written per element).
// Exponential moving average of the weights, same launch geometry: e <- e + (p - e) (1 - decay), alone (mi_ema_update), inside the
// Adam launch on the new p (mi_adam_ema_step: the same bits as the two launches), and the exchange of p and e (mi_ema_swap).
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
