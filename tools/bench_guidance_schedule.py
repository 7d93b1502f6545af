"""What a guidance interval / schedule saves or costs on the GPU, on the headline configuration of bench.py: base 64^2 + SR 64 -> 256,
B = 32, T = 100, cond_scale 3, fp32, synchronous sample() calls.

  python tools/bench_guidance_schedule.py
     1. ms per sample() call for the default call, guidance_interval = (0.25, 0.75) and a ramp schedule 1 -> cond_scale over the steps.  The
        forms alternate inside one process; `--rounds` passes over all forms, min .. median .. max over the passes is the run-to-run spread.
        Next to the ms saved: the share of U-Net row-evaluations the plan skips, derived from the shapes (an unguided step runs B rows
        instead of 2 B).  `--forms default` runs on a tree from before the keywords existed (the parent's default form: what the default
        form here has to stay within).
     2. the three table-reading launches alone (mi_cfg_sched_combine_fwd, mi_cfg_sched_rescale_stats_fwd, mi_cfg_sched_rescale_apply_fwd) at the
        SR and base shapes, timed with events around each launch, against the traffic derived from the shapes: combine and apply read
        2 B n 4 bytes and write B n 4, stats reads 2 B n 4.  The prediction is restored by a device copy before every repetition (outside
        the timed windows), so every launch finds it as the U-Net's last conv leaves it: just written.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("default", "interval", "ramp")


def ms_per(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def bench_calls(args, dev):
    import bench
    im, _ = bench.build_imagen("cascade64_256", args.timesteps, dev)
    B, T, s = args.batch, args.timesteps, args.cond_scale
    emb, mask = (t.to(dev) for t in bench.synthetic_text(B))
    base = dict(text_embeds=emb, text_masks=mask, _seed=2)
    ramp = lambda u: 1. + (s - 1.) * (1. - u)                  # 1 at the first (noisiest) step, cond_scale at the last
    extra = {"default": dict(cond_scale=s), "interval": dict(cond_scale=s, guidance_interval=(args.lo, args.hi)), "ramp": dict(guidance_schedule=ramp)}
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
        print(f"{k:28s} {min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}")
    d = res.get("default")
    if d:
        spread = max(d) - min(d)
        print(f"# the default form's own spread (max - min) = {spread:.3f} ms")
        plain = {"interval": sum(1 for t in range(T) if not args.lo * (T - 1) <= t <= args.hi * (T - 1)), "ramp": sum(1 for t in range(T) if ramp(t / (T - 1)) == 1.)}
        for k, v in res.items():
            if k != "default":
                diff = statistics.median(v) - statistics.median(d)
                verdict = "faster than the default beyond its spread" if diff < -spread else "NOT faster than the default beyond its spread"
                print(f"# {k} - default = {diff:+.3f} ms per call (medians; {verdict}); derived: {plain[k]} of {T} steps per stage unguided = "
                      f"{plain[k] / (2 * T):.1%} of the U-Net row-evaluations skipped")
    for u in im.unets:
        for key, ws in u.engine()._ws.items():
            print(f"# workspace {key[2]}^2, {key[1]} rows{' (unfolded)' if key[-1] == 'nofold' else ''}: guidance fold "
                  f"{'on' if getattr(ws, 'cfg_fold', None) is not None else 'off'}, graphs per state {[len(st.graphs) for st in ws.sampler_state.values()]}")
    im.check_device_status()


def bench_launches(args, dev):
    from minimagen_amd import _lib as L
    lib = L.lib()
    B, phi, S = args.batch, 0.7, 4
    print(f"## the table-reading launches alone, B = {B}, per-row scales, phi {phi}: us per launch (events around each launch, {args.reps} repetitions)")
    print(f"{'shape':22s} {'launch':8s} {'min':>8s} {'median':>8s} {'max':>8s} {'MB derived':>11s} {'GB/s (median)':>14s}")
    for name, n in (("SR 3 x 256^2", 3 * 256 * 256), ("base 3 x 64^2", 3 * 64 * 64)):
        src = torch.randn(2 * B, n, generator=torch.Generator().manual_seed(1)).to(dev)
        pred2 = torch.empty_like(src)
        part = torch.zeros(B, lib.mi_cfg_rescale_chunks(n), 4, dtype=torch.float64, device=dev)
        tab = (1.5 + torch.rand(S, B, generator=torch.Generator().manual_seed(2)) * 3.).to(dev)
        t_state = torch.tensor([S - 1], dtype=torch.int32).to(dev)
        p = L.MiCfgSchedParams(B, n, pred2.data_ptr(), tab.data_ptr(), t_state.data_ptr(), 1, phi, part.data_ptr())
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(args.reps + 5)]
        for e0, e1, e2, e3, e4 in ev:
            st = L.current_stream()
            pred2.copy_(src)
            e0.record()
            L.check(lib.mi_cfg_sched_combine_fwd(C.byref(p), st), "mi_cfg_sched_combine_fwd")
            e1.record()
            pred2.copy_(src)
            e2.record()
            L.check(lib.mi_cfg_sched_rescale_stats_fwd(C.byref(p), st), "mi_cfg_sched_rescale_stats_fwd")
            e3.record()
            L.check(lib.mi_cfg_sched_rescale_apply_fwd(C.byref(p), st), "mi_cfg_sched_rescale_apply_fwd")
            e4.record()
        torch.cuda.synchronize()
        assert pred2.isfinite().all()
        for launch, a, b, nbytes in (("combine", 0, 1, 3 * B * n * 4), ("stats", 2, 3, 2 * B * n * 4), ("apply", 3, 4, 3 * B * n * 4)):
            us = [t[a].elapsed_time(t[b]) * 1e3 for t in ev[5:]]
            med = statistics.median(us)
            print(f"{name:22s} {launch:8s} {min(us):8.2f} {med:8.2f} {max(us):8.2f} {nbytes / 1e6:11.2f} {nbytes / (med * 1e-6) / 1e9:14.0f}")
    print("# per guided SR step of a table run: combine moves 3 B n 4 = 75.5 MB at B = 32 (derived from the shapes, not measured)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="sample() calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--cond-scale", type=float, default=3.0)
    ap.add_argument("--lo", type=float, default=0.25)
    ap.add_argument("--hi", type=float, default=0.75)
    ap.add_argument("--forms", default=",".join(FORMS), help="comma-separated subset of: " + ", ".join(FORMS))
    ap.add_argument("--no-launches", action="store_true", help="skip part 2 (a tree without the table-reading kernels)")
    args = ap.parse_args()
    args.forms = [f.strip() for f in args.forms.split(",")]
    assert all(f in FORMS for f in args.forms), args.forms
    assert torch.cuda.is_available(), "tools/bench_guidance_schedule.py measures on the GPU"
    from minimagen_amd import _lib as L
    dev = torch.device("cuda:0")
    print(f"# tools/bench_guidance_schedule.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, fp32, host clock around synchronised windows")
    bench_calls(args, dev)
    if not args.no_launches:
        bench_launches(args, dev)


if __name__ == "__main__":
    main()
