"""What the thresholding modes cost on the GPU, on the headline configuration of bench.py: base 64^2 + SR 64 -> 256, B = 32, T = 100,
cond_scale 3, fp32, synchronous sample() calls.

  python tools/bench_thresholding.py
     1. ms per sample() call for thresholding = 'dynamic' (the default call), 'static' and 'none' (both stages).  The forms alternate inside one
        process; `--rounds` passes over all forms, min .. median .. max over the passes is the run-to-run spread.  A form is reported as
        different from 'dynamic' only when its median lies outside the 'dynamic' form's own min .. max.  `--forms default` runs on a tree from
        before the keywords existed (the parent's default form: what the 'dynamic' form here has to stay within).
     2. the tail of ONE step alone, timed with events around each launch, at the SR shape (3 x 256^2: the grouped tail against the direct tail)
        and at the base shape (3 x 64^2: the one-workgroup tail against the direct tail), Philox noise, B guided rows in the prediction (the
        folded U-Net's output) and 2 B rows (`two`), against the traffic derived from the shapes: the direct tail reads the prediction and x
        and writes x, 12 B per element (16 B with `two`) -- a count, not a measurement.
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

FORMS = ("default", "dynamic", "static", "none")                   # default: no keyword at all (also what a tree before the keywords can run)


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
    base = dict(text_embeds=emb, text_masks=mask, _seed=2, cond_scale=s)
    forms = {k: (lambda kw=({} if k == "default" else dict(thresholding=k)): im.sample(**base, **kw)) for k in args.forms}
    print(f"## sample() of the cascade 64 -> 256, B = {B}, T = {T}, cond_scale {s}: ms per call")
    res = {k: [] for k in forms}
    for fn in forms.values():
        ms_per(fn, args.warmup)
    for _ in range(args.rounds):
        for k, fn in forms.items():
            res[k].append(ms_per(fn, args.steps))
    print(f"{'form':28s} {'min':>9s} {'median':>9s} {'max':>9s}   ({args.rounds} rounds of {args.steps}, ms)")
    for k, v in res.items():
        print(f"{k if k == 'default' else 'thresholding ' + k:28s} {min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}")
    d = res.get("dynamic") or res.get("default")
    if d and len(res) > 1:
        print(f"# the dynamic form's own spread: {min(d):.3f} .. {max(d):.3f} ms")
        for k, v in res.items():
            if v is d:
                continue
            med = statistics.median(v)
            where = "inside" if min(d) <= med <= max(d) else "OUTSIDE"
            print(f"# {k}: median {med:.3f} ms = {med / statistics.median(d):.4f} of the dynamic median, {where} the dynamic form's min .. max")
    for u in im.unets:
        for key, ws in u.engine()._ws.items():
            print(f"# workspace {key[2]}^2, {key[1]} rows: graph keys per state {[[k[10:] for k in st.graphs] for st in ws.sampler_state.values()]}, "
                  f"group_sync {[hasattr(st, 'group_sync') for st in ws.sampler_state.values()]}")
    im.check_device_status()


def bench_tail(args, dev):
    from minimagen_amd import _lib as L
    from minimagen_amd.diffusion_model import GaussianDiffusion
    from minimagen_amd.helpers import quantile_rank
    lib, B, T = L.lib(), args.batch, args.timesteps
    coef = GaussianDiffusion(timesteps=T).sampler_coef_table().to(dev).contiguous()
    tstate = torch.tensor([T // 2], dtype=torch.int32, device=dev)
    print(f"## the tail of one step alone, B = {B}: us per launch (events around each launch, {args.reps} repetitions, Philox noise)")
    print(f"{'shape':16s} {'rows':5s} {'tail':22s} {'min':>8s} {'median':>8s} {'max':>8s} {'MB derived':>11s} {'GB/s (median)':>14s}")
    for name, n in (("SR 3 x 256^2", 3 * 256 * 256), ("base 3 x 64^2", 3 * 64 * 64)):
        g = torch.Generator().manual_seed(1)
        pred2 = (torch.randn(2 * B, n, generator=g) * 0.5).to(dev)
        x0 = torch.randn(B, n, generator=g).to(dev)
        k_lo, k_hi, w = quantile_rank(n, 0.9)
        small = n <= 16384
        sync = None if small else torch.zeros(lib.mi_sampler_group_sync_bytes(B, n), dtype=torch.uint8, device=dev)
        for two in (0, 1):
            x = x0.clone()
            cp = L.MiCfgX0Params(B, n, pred2.data_ptr(), two, args.cond_scale, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0)
            qp = L.MiQuantileParams(B, n, 0, k_lo, k_hi, w, 0, 0, 0, 0, 0)
            pp = L.MiPosteriorParams(B, n, T, 0, 0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 1234, 0, 1 << 20, 0, 0)
            st = L.current_stream()
            tails = {}
            if small:
                tails["small (dynamic)"] = lambda: lib.mi_sampler_step_small_ext_fwd(C.byref(cp), C.byref(qp), C.byref(pp), None, st)
            else:
                tails["group (dynamic)"] = lambda: lib.mi_sampler_step_group_ext_fwd(C.byref(cp), C.byref(qp), C.byref(pp), None, sync.data_ptr(), st)
            tails["direct (static)"] = lambda: lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(pp), None, None, 1, st)
            tails["direct (none)"] = lambda: lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(pp), None, None, 0, st)
            for tail, launch in tails.items():
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.reps + 5)]
                for e0, e1 in ev:
                    x.copy_(x0)                                   # (the tail works in place: every repetition starts from the same x)
                    e0.record()
                    L.check(launch(), tail)
                    e1.record()
                torch.cuda.synchronize()
                if sync is not None:
                    assert int(sync[8:12].view(torch.int32).item()) == 0
                us = [t[0].elapsed_time(t[1]) * 1e3 for t in ev[5:]]
                med, nbytes = statistics.median(us), (16 if two else 12) * B * n
                derived = f"{nbytes / 1e6:11.2f} {nbytes / (med * 1e-6) / 1e9:14.0f}" if tail.startswith("direct") else f"{'-':>11s} {'-':>14s}"
                print(f"{name:16s} {('2B' if two else 'B'):5s} {tail:22s} {min(us):8.2f} {med:8.2f} {max(us):8.2f} {derived}")
    print("# the same inputs every repetition (they fit the 256 MB last-level cache, so the rate is not an HBM rate); Philox: 10 rounds + Box-Muller per "
          "quad in every tail; the dynamic tails also select the two order statistics of |x0| per image")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="sample() calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--cond-scale", type=float, default=3.0)
    ap.add_argument("--forms", default="dynamic,static,none", help="comma-separated subset of: " + ", ".join(FORMS))
    ap.add_argument("--no-tail", action="store_true", help="skip part 2 (a tree without mi_sampler_step_direct_fwd)")
    args = ap.parse_args()
    args.forms = [f.strip() for f in args.forms.split(",")]
    assert all(f in FORMS for f in args.forms), args.forms
    assert torch.cuda.is_available(), "tools/bench_thresholding.py measures on the GPU"
    from minimagen_amd import _lib as L
    dev = torch.device("cuda:0")
    print(f"# tools/bench_thresholding.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, fp32, host clock around synchronised windows")
    bench_calls(args, dev)
    if not args.no_tail:
        bench_tail(args, dev)


if __name__ == "__main__":
    main()
