"""Cost of the prediction objectives on the GPU, on the benched cascade's SR U-Net (unet_1 of tests/golden/unet_params.json) at
B = 32, 256^2.

  python tools/bench_objective.py    1. the front + loss segment of a training step on fixed tensors -- the image and the low-resolution image
                                        corrupted, the 'v' target, the min-SNR-weighted loss of a stand-in prediction and its backward -- on
                                        csrc/objective.hip (5 launches) against the torch-op form of the same train_ops functions, with the bytes
                                        each form moves;
                                     2. ms per whole training step (Imagen.forward + backward + gradient clip + Adam, optim.Adam(max_grad_norm=50))
                                        for the default configuration and for pred_objectives='v' with min_snr_loss_weight=True.
                                     The forms alternate inside one process; `--rounds` passes over all forms, min .. median .. max over the passes
                                     is the run-to-run spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms_per(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def alternate(forms, args):
    """{form: [ms per call, one value per round]}, every round visiting every form"""
    res = {k: [] for k in forms}
    for fn in forms.values():
        ms_per(fn, args.warmup)
    for _ in range(args.rounds):
        for k, fn in forms.items():
            res[k].append(ms_per(fn, args.steps))
    return res


def table(res, args, unit="ms"):
    print(f"{'form':34s} {'min':>9s} {'median':>9s} {'max':>9s}   ({args.rounds} rounds of {args.steps}, {unit})")
    for k, v in res.items():
        print(f"{k:34s} {min(v):9.4f} {statistics.median(v):9.4f} {max(v):9.4f}")


def bench_segment(args, dev):
    from minimagen_amd import train_ops
    from minimagen_amd.diffusion_model import GaussianDiffusion
    B, S, T = args.batch, args.size, args.timesteps
    g = torch.Generator().manual_seed(0)
    x, low = torch.rand(B, 3, S, S, generator=g).to(dev), torch.rand(B, 3, S, S, generator=g).to(dev)
    eps, eps_low = torch.randn(B, 3, S, S, generator=g).to(dev), torch.randn(B, 3, S, S, generator=g).to(dev)
    pred = torch.randn(B, 3, S, S, generator=g).to(dev).requires_grad_()
    times = torch.randint(0, T, (B,), generator=g).to(dev)
    low_times = torch.full((B,), T // 5, dtype=torch.int64, device=dev)
    sched = GaussianDiffusion(timesteps=T).to(dev)
    w = sched.loss_weight_table("v", 5.).to(dev)

    def segment(hip):
        def run():
            train_ops.ENABLED = hip
            try:
                _, target = train_ops.diffuse(x, eps, times, sched, normalize=True, target="v")
                train_ops.diffuse(low, eps_low, low_times, sched, normalize=True, target=None)
                loss = train_ops.objective_loss(pred, target, times, w, "l2")
                pred.grad = None
                loss.backward()
            finally:
                train_ops.ENABLED = True
            return loss
        return run
    forms = {"objective.hip (5 launches)": segment(True), "torch ops": segment(False)}
    la, lb = (float(forms[k]().detach()) for k in ("objective.hip (5 launches)", "torch ops"))
    n_el = B * 3 * S * S
    # kernels: front 8 read + 8 written (x_t, v), low-resolution front 8 + 4, loss 8 + 4 (g), backward 4 + 4 bytes per element.
    # torch ops, counting one read per operand and one write per result of every elementwise launch (broadcast scalars free): x * 2, - 1, a * x0,
    # s * eps, + (8 + 8 + 8 + 8 + 12), the same for the low-resolution image, a * eps, s * x0, - (8 + 8 + 12), mse (12), the two means (4), and
    # autograd's backward of mean / mse (expand 4, 2 * d * g >= 16, and what it re-reads)
    kb, tb = 48 * n_el, (44 + 44 + 28 + 12 + 4 + 20) * n_el
    print(f"## front + loss segment, B = {B}, {S}^2, T = {T}: {n_el / 1e6:.2f} M elements per tensor; loss {la:.7f} (kernels) {lb:.7f} (torch ops)")
    print(f"# bytes moved: kernels {kb / 1e6:.0f} MB (48 B / element), torch ops at least {tb / 1e6:.0f} MB (152 B / element)")
    res = alternate(forms, args)
    table(res, args)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"# kernels: {kb / (med['objective.hip (5 launches)'] * 1e-3) / 1e9:.0f} GB/s of their own bytes; torch ops / kernels = "
          f"{med['torch ops'] / med['objective.hip (5 launches)']:.2f}x")


def build_sr(dev, timesteps, **extra):
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    p = json.load(open(os.path.join(ROOT, "tests", "golden", "unet_params.json")))
    torch.manual_seed(0)
    unets = [Unet(**p["unet0"]), Unet(**p["unet1"])]
    return Imagen(unets, text_encoder_name="t5_small", image_sizes=(64, 256), timesteps=timesteps, cond_drop_prob=0.15, **extra).to(dev).train()


def bench_step(args, dev):
    import bench
    from minimagen_amd.optim import Adam
    B, S = args.batch, args.size
    imgs = torch.rand(B, 3, S, S, device=dev)
    emb, mask = bench.synthetic_text(B)
    emb, mask = emb.to(dev), mask.to(dev)

    def stepper(**extra):
        im = build_sr(dev, args.timesteps, **extra)
        opt = Adam(im.unets[1].parameters(), lr=1e-5, max_grad_norm=50.)
        state = [0]

        def run():
            state[0] += 1
            torch.manual_seed(state[0])
            loss = im(imgs, text_embeds=emb, text_masks=mask, unet_number=2)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss
        return run
    forms = {"default (noise, flat weight)": stepper(), "v + min-SNR (gamma 5)": stepper(pred_objectives="v", min_snr_loss_weight=True)}
    print(f"## whole training step of the SR U-Net (forward + backward + clip + Adam), B = {B}, {S}^2, T = {args.timesteps}")
    res = alternate(forms, args)
    table(res, args)
    d, v = res["default (noise, flat weight)"], res["v + min-SNR (gamma 5)"]
    spread, diff = max(d) - min(d), statistics.median(v) - statistics.median(d)
    print(f"# v + min-SNR - default = {diff:+.4f} ms (medians); the default step's own spread (max - min) = {spread:.4f} ms: "
          f"{'within' if diff <= spread else 'OUTSIDE'} the spread")
    for k, fn in forms.items():
        print(f"# last loss, {k}: {float(fn().detach()):.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--timesteps", type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_objective.py measures on the GPU"
    from minimagen_amd import _lib as L
    dev = torch.device("cuda:0")
    print(f"# tools/bench_objective.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, fp32, host clock around synchronised windows")
    bench_segment(args, dev)
    bench_step(args, dev)


if __name__ == "__main__":
    main()
