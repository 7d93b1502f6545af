"""Development aid: the wide attention core of the training graph on the flash kernels (train_ops.flash_attention, attn_train_wide.hip) against
the torch-op form (einsum -> softmax -> einsum, what MINIMAGEN_FLASH_TRAIN=0 runs), forward + backward, in the same process and alternating,
timed with device events after a warm-up; peak memory of each form over what was allocated before it.  Shapes:
  (a) self-attention of Unet() default at 64 x 64: B = 8, 4096 tokens, 8 heads, J = 4097 (multi-query) -- the core and the whole layer
  (b) self-attention of Base / Super: B = 16, 1024 tokens, J = 1025
  (c) the wide cross-attention: B = 8, 4096 tokens, J = 259 (a k / v head per head, unmasked as in the U-Net)
  (d) one Unet() default training step at 64 x 64, B = 8, MINIMAGEN_FLASH_TRAIN 0 / 1: forward + backward, and with clip + Adam
Algorithmic FLOPs: 4 n J 64 H per image forward, 8 n J 64 H backward (the kernels issue 3-term fp16 products -- three matrix instructions per
product -- and recompute S in both backward kernels and dP in both: 7 n J 64 H x 2 backward).  Kernel times: a separate rocprofv3 run.
usage: python tools/bench_flash_train.py [a b c d ...] [--reps N]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minimagen_amd import train_ops  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
WHICH = [a for a in sys.argv[1:] if a in ("a", "b", "c", "d")] or ["a", "b", "c", "d"]
GB = 2 ** 30


def torch_core(q, k, v, heads, scale):
    """the layers' torch-op core (layers.Attention / CrossAttention.forward) on token-major q [B, n, H*64], k / v [B, J, KVH*64]"""
    B, n, _ = q.shape
    qh = q.reshape(B, n, heads, 64).transpose(1, 2) * scale
    if k.shape[-1] == 64:
        sim = torch.einsum('bhid,bjd->bhij', qh, k)
        attn = sim.softmax(dim=-1, dtype=torch.float32)
        out = torch.einsum('bhij,bjd->bhid', attn, v)
    else:
        kh, vh = (t.reshape(B, -1, heads, 64).transpose(1, 2) for t in (k, v))
        attn = torch.einsum('bhid,bhjd->bhij', qh, kh).softmax(dim=-1, dtype=torch.float32)
        out = torch.einsum('bhij,bhjd->bhid', attn, vh)
    return out.transpose(1, 2).reshape(B, n, -1)


def timed(fn, reps):
    """(ms per call from device events, peak GB over what was allocated before the first call)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, (torch.cuda.max_memory_allocated() - base) / GB


def ab(name, forms, flops, reps=REPS, rounds=3):
    """alternate the forms `rounds` times (one warm-up call each first); report the best round of each"""
    for f in forms.values():
        f()
    best = {k: (1e30, 0.0) for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            ms, mem = timed(f, reps)
            best[k] = (min(best[k][0], ms), max(best[k][1], mem))
    for k, (ms, mem) in best.items():
        rate = f"  {flops / ms * 1e-9:7.1f} TFLOP/s algorithmic" if flops else ""
        print(f"{name:44s} {k:10s} {ms:9.3f} ms  peak +{mem:6.2f} GB{rate}", flush=True)
    ks = list(best)
    print(f"{name:44s} speed-up {best[ks[1]][0] / best[ks[0]][0]:.2f} x, memory {best[ks[0]][1] / max(best[ks[1]][1], 1e-9):.4f} of the torch-op form", flush=True)


def core_case(tag, B, n, H, J, kvh):
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(B, n, H * 64, device=dev, generator=g).requires_grad_()
    k = torch.randn(B, J, kvh * 64, device=dev, generator=g).requires_grad_()
    v = torch.randn(B, J, kvh * 64, device=dev, generator=g).requires_grad_()
    gy = torch.randn(B, n, H * 64, device=dev, generator=g)
    scale = 64 ** -0.5

    def flash():
        q.grad = k.grad = v.grad = None
        train_ops.flash_attention(q, k, v, None, scale).backward(gy)

    def ops():
        q.grad = k.grad = v.grad = None
        torch_core(q, k, v, H, scale).backward(gy)
    fl = 12.0 * B * n * J * 64 * H
    ab(f"({tag}) core B={B} n={n} H={H} J={J} kv_heads={kvh}", {"flash": flash, "torch-ops": ops}, fl)

    def fwd(f):
        with torch.no_grad():
            return f()
    ab(f"({tag}) core forward only", {"flash": lambda: fwd(lambda: train_ops.flash_attention(q, k, v, None, scale)),
                                       "torch-ops": lambda: fwd(lambda: torch_core(q, k, v, H, scale))}, 4.0 * B * n * J * 64 * H)


def layer_case(B, n, dim):
    from minimagen_amd.layers import Attention
    torch.manual_seed(3)
    layer = Attention(dim=dim).train().to(dev)
    x = torch.randn(B, n, dim, device=dev, requires_grad=True)
    gy = torch.randn(B, n, dim, device=dev)

    def run(flash):
        def f():
            train_ops.FLASH_TRAIN = flash
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer(x).backward(gy)
            train_ops.FLASH_TRAIN = True
        return f
    ab(f"(a) whole Attention(dim={dim}) layer B={B} n={n}", {"flash": run(True), "torch-ops": run(False)}, 12.0 * B * n * (n + 1) * 64 * 8)


def unet_step(B=8, size=64):
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    from minimagen_amd.optim import Adam
    from oracle import restated as R
    torch.manual_seed(4)
    im = Imagen((Unet(),), text_encoder_name="t5_small", image_sizes=(size,), timesteps=1000).train().to(dev)
    imgs = torch.rand(B, 3, size, size, device=dev)
    emb, mask = R.synthetic_text(B, length=64, seed=5)
    emb, mask = emb.to(dev), mask.to(dev)
    params = list(im.unets[0].parameters())
    opt = Adam(params, lr=1e-5)

    def run(flash, with_opt):
        def f():
            train_ops.FLASH_TRAIN = flash
            train_ops.begin_step(im.unets[0])
            loss = im(imgs, text_embeds=emb, text_masks=mask, unet_number=1)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            if with_opt:
                torch.nn.utils.clip_grad_norm_(params, 50)
                opt.step()
            train_ops.FLASH_TRAIN = True
        return f
    ab(f"(d) Unet() default step {size}x{size} B={B} fwd+bwd", {"flash": run(True, False), "torch-ops": run(False, False)}, 0, reps=3, rounds=2)
    ab(f"(d) Unet() default step {size}x{size} B={B} + clip + Adam", {"flash": run(True, True), "torch-ops": run(False, True)}, 0, reps=3, rounds=2)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_flash_train needs the MI355X"
    print(f"device {torch.cuda.get_device_name(0)}; reps {REPS}; FLOP/s = algorithmic (12 n J 64 H fwd+bwd, 4 n J 64 H forward) over event time")
    if "a" in WHICH:
        core_case("a", 8, 4096, 8, 4097, 1)
        layer_case(8, 4096, 128)
    if "b" in WHICH:
        core_case("b", 16, 1024, 8, 1025, 1)
    if "c" in WHICH:
        core_case("c", 8, 4096, 8, 259, 8)
    if "d" in WHICH:
        unet_step()
