"""Cost of conditioning sample() on pixels, on the benched cascade (64 -> 256, B = 32, cond_scale 3, T = 100, fp32, synchronous calls).

  python tools/bench_inpaint.py             ms per call with and without a half mask (images given at 256^2) for the default loop and for
                                            'dpmpp_2m' at S = 25; the full cascade against stop_at_stage=1 and start_at_stage=1 (the image
                                            of the stop call as start_image).  `--rounds` interleaved passes over all configurations: the
                                            spread between the passes is the run-to-run noise
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o inpaint -- python tools/bench_inpaint.py --trace
                                            few calls per configuration for a kernel trace of its own; then
  python tools/bench_inpaint.py --tail-stats DIR/.../inpaint_kernel_stats.csv
                                            the sampler tails per instantiation <HISTORY, INPAINT, ...>, blend 0 and the preparation kernels
"""
import argparse
import csv
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_sample_steps import ms_per_call      # noqa: E402

KERNELS = ("sampler_small_kernel", "sampler_group_kernel", "posterior_kernel", "known_blend0_kernel", "known_image_kernel", "known_mask_kernel", "resize_kernel")


def tail_stats(path):
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in KERNELS)]
    print(f"# sampler tail and known-region kernels in {os.path.basename(path)} (rocprofv3 --kernel-trace --stats); tails: <HISTORY, INPAINT, blocks...>")
    for r in sorted(rows, key=lambda r: r["Name"]):
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
        print(f"{name:90s} calls {int(r['Calls']):6d}  avg {float(r['AverageNs']) / 1e3:8.2f} us  min {float(r['MinNs']) / 1e3:8.2f}  max {float(r['MaxNs']) / 1e3:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
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
    g = torch.Generator().manual_seed(1)
    half = torch.zeros(B, sizes[-1], sizes[-1], dtype=torch.bool)
    half[:, :, :sizes[-1] // 2] = True
    known = dict(inpaint_images=torch.rand(B, 3, sizes[-1], sizes[-1], generator=g).to(dev), inpaint_masks=half.to(dev))
    fast = dict(sample_steps=25, sampler="dpmpp_2m")
    base = im.sample(**kw, stop_at_stage=1).clone()
    configs = [("default loop", {}), ("default loop, half mask", known), ("dpmpp_2m S=25", fast), ("dpmpp_2m S=25, half mask", dict(**fast, **known)),
               ("stop_at_stage=1", dict(stop_at_stage=1)), ("start_at_stage=1", dict(start_at_stage=1, start_image=base))]
    print(f"# cascade {sizes}, B = {B}, cond_scale 3, T = {T}, fp32, synchronous sample() calls; library {os.path.basename(L.DEFAULT_LIB)}; "
          f"{torch.cuda.get_device_name(0)}")
    if args.trace:
        for _, extra in configs[:4]:
            ms_per_call(im, kw, extra, 2, 1)
        im.check_device_status()
        return
    res = {name: [] for name, _ in configs}
    for r in range(args.rounds):                            # interleaved: every pass visits every configuration
        for name, extra in configs:
            res[name].append(ms_per_call(im, kw, extra, args.calls, args.warmup if r == 0 else 1))
    im.check_device_status()
    print(f"{'configuration':28s}  " + "  ".join(f"round {r} ms" for r in range(args.rounds)) + "   min ms")
    for name, _ in configs:
        print(f"{name:28s}  " + "  ".join(f"{x:10.2f}" for x in res[name]) + f"  {min(res[name]):7.2f}")
    m = {name: min(v) for name, v in res.items()}
    print(f"# half mask: default loop +{m['default loop, half mask'] - m['default loop']:.2f} ms per call, dpmpp_2m S=25 +{m['dpmpp_2m S=25, half mask'] - m['dpmpp_2m S=25']:.2f} ms")
    print(f"# full - stop_at_stage=1 = {m['default loop'] - m['stop_at_stage=1']:.2f} ms; start_at_stage=1 = {m['start_at_stage=1']:.2f} ms")


if __name__ == "__main__":
    main()
