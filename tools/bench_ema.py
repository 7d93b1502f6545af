"""Cost of the exponential moving average of the weights on the GPU, for two parameter sets: the benched cascade's SR U-Net
(unet_1 of tests/golden/unet_params.json) and ``Unet()`` default.

  python tools/bench_ema.py        median ms per optimiser step (fixed gradients, no forward / backward) for Adam alone, Adam followed by a
                                   separate EMA.update() -- timed as two independent series, whose difference is the spread of that form
                                   against itself --, and the fused step of an attached EMA; then one enter + exit of average_parameters()
                                   with the first sample() after each against a steady sample().  `--rounds` interleaved passes over all
                                   forms; min .. max over the passes is the run-to-run spread
"""
import argparse
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


def optimiser_forms(named, args):
    """{form: callable of one optimiser step}; every form owns clones of the parameters with fixed gradients"""
    from minimagen_amd.optim import Adam, EMA
    g = torch.Generator().manual_seed(0)
    grads = [(torch.randn(p.shape, generator=g) * 1e-3).to(p.device) for _, p in named]

    def clones():
        ps = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        return ps
    forms = {}
    ps = clones()
    forms["Adam alone"] = Adam(ps, lr=1e-6).step
    for tag in ("A", "B"):
        ps = clones()
        opt, ema = Adam(ps, lr=1e-6), EMA([(n, p) for (n, _), p in zip(named, ps)], decay=args.decay)
        forms[f"Adam + update() [{tag}]"] = (lambda o, e: lambda: (o.step(), e.update()))(opt, ema)
    ps = clones()
    opt = Adam(ps, lr=1e-6)
    EMA([(n, p) for (n, _), p in zip(named, ps)], decay=args.decay).attach(opt)
    forms["fused step"] = opt.step
    return forms


def bench_steps(title, named, args):
    n_el = sum(p.numel() for _, p in named)
    print(f"## {title}: {len(named)} tensors, {n_el / 1e6:.2f} M elements "
          f"(Adam 28 B / element = {28 * n_el / 1e6:.0f} MB, separate update +12 B, fused +8 B)")
    forms = optimiser_forms(named, args)
    res = {k: [] for k in forms}
    for fn in forms.values():
        ms_per(fn, args.warmup)
    for _ in range(args.rounds):                            # interleaved: every pass visits every form
        for k, fn in forms.items():
            res[k].append(ms_per(fn, args.steps))
    print(f"{'form':26s} median ms/step      min      max   ({args.rounds} passes of {args.steps} steps)")
    for k, v in res.items():
        print(f"{k:26s} {statistics.median(v):14.4f} {min(v):8.4f} {max(v):8.4f}")
    med = {k: statistics.median(v) for k, v in res.items()}
    two = [med["Adam + update() [A]"], med["Adam + update() [B]"]]
    print(f"# two launches against themselves: |A - B| = {abs(two[0] - two[1]):.4f} ms; fused - min(A, B) = {med['fused step'] - min(two):+.4f} ms; "
          f"fused - Adam alone = {med['fused step'] - med['Adam alone']:+.4f} ms; separate update = {min(two) - med['Adam alone']:+.4f} ms")


def bench_swap(title, im, module, kw, args):
    from minimagen_amd.optim import EMA
    ema = EMA(module, decay=args.decay)
    for _ in range(2):
        im.sample(**kw)
    steady, enter, first_in, leave, first_out = [], [], [], [], []
    for _ in range(args.rounds):
        steady.append(ms_per(lambda: im.sample(**kw), 2))
        cm = ema.average_parameters()
        enter.append(ms_per(cm.__enter__, 1))
        first_in.append(ms_per(lambda: im.sample(**kw), 1))
        leave.append(ms_per(lambda: cm.__exit__(None, None, None), 1))
        first_out.append(ms_per(lambda: im.sample(**kw), 1))
    im.check_device_status()
    print(f"## {title}: average_parameters(), sample() B = {kw['text_embeds'].shape[0]}, T = {args.timesteps}")
    print(f"{'':26s}      median ms      min      max   ({args.rounds} passes)")
    for k, v in (("steady sample()", steady), ("enter (drain + swap)", enter), ("first sample() inside", first_in), ("exit (drain + swap)", leave),
                 ("first sample() after", first_out)):
        print(f"{k:26s} {statistics.median(v):14.3f} {min(v):8.3f} {max(v):8.3f}")
    m = statistics.median
    print(f"# one visit costs {m(enter) + m(leave) + (m(first_in) - m(steady)) + (m(first_out) - m(steady)):.2f} ms over two steady calls (two exchanges, two re-packs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--timesteps", type=int, default=25)
    ap.add_argument("--no-swap", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_ema.py measures on the GPU"
    import bench
    from minimagen_amd import _lib as L
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    dev = torch.device("cuda:0")
    print(f"# tools/bench_ema.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, decay {args.decay}, fp32, host clock around "
          f"synchronised windows")
    cascade, sizes = bench.build_imagen("cascade64_256", args.timesteps, dev)
    torch.manual_seed(0)
    base = Imagen([Unet()], text_encoder_name="t5_small", image_sizes=(64,), timesteps=args.timesteps, cond_drop_prob=0.15).to(dev)
    emb, mask = bench.synthetic_text(args.batch)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3.)
    for title, im, module in ((f"SR U-Net (unet_1 of the benched cascade {sizes})", cascade, cascade.unets[1]), ("Unet() default @64", base, base.unets[0])):
        bench_steps(title, list(module.named_parameters()), args)
        if not args.no_swap:
            bench_swap(title, im, module, kw, args)


if __name__ == "__main__":
    main()
