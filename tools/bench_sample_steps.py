"""Cost of a sample() call against the number of sampling steps S and the solver, on the benched cascade (64 -> 256, B = 32, cond_scale 3,
T = 100, fp32, synchronous calls).  The expectation it confirms or refutes: ms per call = a fixed part + S x the default call's per-step time.

  python tools/bench_sample_steps.py                      table: ms per call for the default call and every (solver, S), `--rounds` interleaved
                                                          passes over all of them (the spread between passes is the run-to-run noise), then a
                                                          least-squares fixed + per-step fit per solver
  python tools/bench_sample_steps.py --default-only       the default call alone: uses nothing newer than sample() itself, so a copy of this
                                                          file times a checkout from before the keywords existed the same way, same session
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o steps -- python tools/bench_sample_steps.py --trace
                                                          few calls per solver for a kernel trace of its own; then
  python tools/bench_sample_steps.py --tail-stats DIR/.../steps_kernel_stats.csv
                                                          the sampler tail kernels with and without the history term, from that trace
"""
import argparse
import csv
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVERS = ("ddpm", "ddim", "dpmpp_2m")


def ms_per_call(im, kw, extra, calls, warmup):
    for k in range(warmup):
        im.sample(**kw, _seed=2 + k, **extra)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        im.sample(**kw, _seed=2 + warmup + k, **extra)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def tail_stats(path):
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in ("sampler_small_kernel", "sampler_group_kernel", "posterior_kernel"))]
    print(f"# sampler tail kernels in {os.path.basename(path)} (rocprofv3 --kernel-trace --stats): <false> = no history term, <true, ...> = with it")
    for r in sorted(rows, key=lambda r: r["Name"]):
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
        print(f"{name:70s} calls {int(r['Calls']):6d}  avg {float(r['AverageNs']) / 1e3:8.2f} us  min {float(r['MinNs']) / 1e3:8.2f}  max {float(r['MaxNs']) / 1e3:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--steps", default="100,50,25,10")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--tail-stats", default="")
    args = ap.parse_args()
    if args.tail_stats:
        return tail_stats(args.tail_stats)
    import bench
    from minimagen_amd import _lib as L
    dev = torch.device("cuda:0")
    T, B = args.timesteps, args.batch
    im, sizes = bench.build_imagen("cascade64_256", T, dev)
    emb, mask = bench.synthetic_text(B)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3.)
    print(f"# cascade {sizes}, B = {B}, cond_scale 3, T = {T}, fp32, synchronous sample() calls; library {os.path.basename(L.DEFAULT_LIB)}; "
          f"{torch.cuda.get_device_name(0)}")
    if args.trace:
        for extra in ({}, dict(sample_steps=25, sampler="ddim"), dict(sample_steps=25, sampler="dpmpp_2m")):
            ms_per_call(im, kw, extra, 2, 1)
        im.check_device_status()
        return
    if args.default_only:
        for r in range(args.rounds):
            print(f"default call (no keywords)         round {r}: {ms_per_call(im, kw, {}, args.calls, args.warmup if r == 0 else 1):8.2f} ms per call")
        im.check_device_status()
        return
    steps = [int(s) for s in args.steps.split(",")]
    configs = [("default", T, {})] + [(name, S, dict(sample_steps=S, sampler=name)) for name in SOLVERS for S in steps]
    res = {(name, S): [] for name, S, _ in configs}
    for r in range(args.rounds):                            # interleaved: every pass visits every configuration
        for name, S, extra in configs:
            res[name, S].append(ms_per_call(im, kw, extra, args.calls, args.warmup if r == 0 else 1))
    im.check_device_status()
    d = min(res["default", T])
    print(f"{'solver':10s} {'S':>4s}  " + "  ".join(f"round {r} ms" for r in range(args.rounds)) + "   min ms   vs default   ms/step")
    for name, S, _ in configs:
        v = res[name, S]
        print(f"{name:10s} {S:4d}  " + "  ".join(f"{x:10.2f}" for x in v) + f"  {min(v):7.2f}   {min(v) / d:9.3f}   {min(v) / S:7.3f}")
    print(f"# fit  ms per call = fixed + per_step * S  (least squares over S = {steps}, the minimum of the rounds); default call: {d / T:.3f} ms/step")
    for name in SOLVERS:
        xs, ys = steps, [min(res[name, S]) for S in steps]
        n, sx, sy = len(xs), sum(xs), sum(ys)
        slope = (n * sum(x * y for x, y in zip(xs, ys)) - sx * sy) / (n * sum(x * x for x in xs) - sx * sx)
        fixed = (sy - slope * sx) / n
        worst = max(abs(fixed + slope * x - y) for x, y in zip(xs, ys))
        print(f"# {name:9s} fixed {fixed:6.2f} ms, per step {slope:6.3f} ms ({slope / (d / T):.3f} x the default's), worst residual {worst:.2f} ms")


if __name__ == "__main__":
    main()
