"""What starting the loop from an init image saves on the GPU, on the headline configuration of bench.py: base 64^2 + SR 64 -> 256,
B = 32, T = 100, cond_scale 3, fp32, synchronous sample() calls.

  python tools/bench_init_image.py
     1. ms per sample() call for the default call, init_strength = 0.75, 0.5, 0.25 (both stages) and [None, 0.5] (the SR stage only).  The
        forms alternate inside one process; `--rounds` passes over all forms, min .. median .. max over the passes is the run-to-run spread.
        Next to every ratio to the default: the share of U-Net evaluations the call skips, derived from the step counts alone (a stage at
        strength s executes m = min(S, max(1, floor(s S + 0.5))) of its S steps) -- per stage and weighted by the stages' measured share of
        the default call when `--stage-share` is given, unweighted otherwise.  `--forms default` runs on a tree from before the keywords
        existed (the parent's default form: what the default form here has to stay within).
     2. the one new launch alone (mi_init_noise_fwd), Philox and injected noise, at the SR and base shapes, timed with events around each
        launch, against the traffic derived from the shapes: 4 B read + 4 B written per element with Philox, 8 + 4 with injected noise.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("default", "0.75", "0.5", "0.25", "none+0.5")            # init_strength: one value for both stages; none+0.5 = [None, 0.5]
STRENGTHS = {"default": (None, None), "0.75": (0.75, 0.75), "0.5": (0.5, 0.5), "0.25": (0.25, 0.25), "none+0.5": (None, 0.5)}


def ms_per(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def executed(S, s):
    return S if s is None else min(S, max(1, int(s * S + 0.5)))


def bench_calls(args, dev):
    import bench
    im, _ = bench.build_imagen("cascade64_256", args.timesteps, dev)
    B, T, s = args.batch, args.timesteps, args.cond_scale
    emb, mask = (t.to(dev) for t in bench.synthetic_text(B))
    base = dict(text_embeds=emb, text_masks=mask, _seed=2, cond_scale=s)
    y = torch.rand(B, 3, 256, 256, generator=torch.Generator().manual_seed(3)).to(dev)
    extra = {k: ({} if k == "default" else dict(init_images=y, init_strength=[v for v in STRENGTHS[k]])) for k in FORMS}
    forms = {k: (lambda kw=extra[k]: im.sample(**base, **kw)) for k in args.forms}
    print(f"## sample() of the cascade 64 -> 256, B = {B}, T = {T}, cond_scale {s}: ms per call")
    res = {k: [] for k in forms}
    for fn in forms.values():
        ms_per(fn, args.warmup)
    for _ in range(args.rounds):
        for k, fn in forms.items():
            res[k].append(ms_per(fn, args.steps))
    print(f"{'form':28s} {'min':>9s} {'median':>9s} {'max':>9s}   ({args.rounds} rounds of {args.steps}, ms)")
    for k, v in res.items():
        print(f"{k if k == 'default' else 'init_strength ' + str(list(STRENGTHS[k])):28s} {min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}")
    d = res.get("default")
    if d:
        print(f"# the default form's own spread (max - min) = {max(d) - min(d):.3f} ms")
        share = args.stage_share                 # the stages' shares of the default call's time (None: every U-Net evaluation counts the same)
        for k, v in res.items():
            if k == "default":
                continue
            m = [executed(T, st) for st in STRENGTHS[k]]
            kept = sum(m) / (2 * T) if share is None else sum(w * mi / T for w, mi in zip(share, m))
            ratio = statistics.median(v) / statistics.median(d)
            print(f"# init_strength {list(STRENGTHS[k])}: median / default median = {ratio:.3f}; derived: stages execute {m[0]} and {m[1]} of {T} steps = {kept:.3f} of the U-Net "
                  f"evaluations{'' if share is None else f' (weighted {share[0]:.2f} / {share[1]:.2f} by stage)'}; gap {ratio - kept:+.3f} of the default call")
    for u in im.unets:
        for key, ws in u.engine()._ws.items():
            print(f"# workspace {key[2]}^2, {key[1]} rows: graphs per state {[sorted(e['per'] for e in st.graphs.values()) for st in ws.sampler_state.values()]}")
    im.check_device_status()


def bench_launch(args, dev):
    from minimagen_amd import _lib as L
    from minimagen_amd.diffusion_model import GaussianDiffusion
    lib = L.lib()
    B = args.batch
    a, b = GaussianDiffusion(timesteps=args.timesteps).init_start_coefs(None, args.timesteps // 2)
    print(f"## mi_init_noise_fwd alone, B = {B}: us per launch (events around each launch, {args.reps} repetitions)")
    print(f"{'shape':22s} {'noise':9s} {'min':>8s} {'median':>8s} {'max':>8s} {'MB derived':>11s} {'GB/s (median)':>14s}")
    for name, n in (("SR 3 x 256^2", 3 * 256 * 256), ("base 3 x 64^2", 3 * 64 * 64)):
        img = torch.rand(B, n, generator=torch.Generator().manual_seed(1)).to(dev)
        eps = torch.randn(B, n, generator=torch.Generator().manual_seed(2)).to(dev)
        x = torch.empty_like(img)
        for form, noise, per_elem in (("Philox", None, 8), ("injected", eps, 12)):
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.reps + 5)]
            for e0, e1 in ev:
                e0.record()
                L.check(lib.mi_init_noise_fwd(img.data_ptr(), x.data_ptr(), B, n, 1, a, b, 1234, 0, (1 << 19) | 1, L.ptr(noise), L.current_stream()), "mi_init_noise_fwd")
                e1.record()
            torch.cuda.synchronize()
            assert x.isfinite().all()
            us = [t[0].elapsed_time(t[1]) * 1e3 for t in ev[5:]]
            med, nbytes = statistics.median(us), per_elem * B * n
            print(f"{name:22s} {form:9s} {min(us):8.2f} {med:8.2f} {max(us):8.2f} {nbytes / 1e6:11.2f} {nbytes / (med * 1e-6) / 1e9:14.0f}")
    print("# one launch per stage and call; the same inputs every repetition (25 MB + 25 MB at the SR shape: they fit the 256 MB last-level cache, so "
          "the rate is not an HBM rate); Philox: 10 rounds + Box-Muller per quad, in place of the mi_randn_fill launch that does the same work")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="sample() calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--cond-scale", type=float, default=3.0)
    ap.add_argument("--forms", default=",".join(FORMS), help="comma-separated subset of: " + ", ".join(FORMS))
    ap.add_argument("--stage-share", default=None, help="'a,b': the base and SR stages' shares of the default call's time, to weight the derived share")
    ap.add_argument("--no-launch", action="store_true", help="skip part 2 (a tree without mi_init_noise_fwd)")
    args = ap.parse_args()
    args.forms = [f.strip() for f in args.forms.split(",")]
    assert all(f in FORMS for f in args.forms), args.forms
    if args.stage_share is not None:
        args.stage_share = [float(v) for v in args.stage_share.split(",")]
        assert len(args.stage_share) == 2
    assert torch.cuda.is_available(), "tools/bench_init_image.py measures on the GPU"
    from minimagen_amd import _lib as L
    dev = torch.device("cuda:0")
    print(f"# tools/bench_init_image.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, fp32, host clock around synchronised windows")
    bench_calls(args, dev)
    if not args.no_launch:
        bench_launch(args, dev)


if __name__ == "__main__":
    main()
