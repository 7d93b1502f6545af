"""Cost of the gradient-norm clip on the GPU, for two parameter sets: the benched cascade's SR U-Net (unet_1 of
tests/golden/unet_params.json) and ``Unet()`` default.

  python tools/bench_clip.py       median ms per optimiser step (fixed gradients, no forward / backward) for torch's clip_grad_norm_ + Adam --
                                   timed as two independent series, whose difference is the spread of that form against itself --,
                                   optim.clip_grad_norm_ + Adam (in place) and Adam(max_grad_norm=) (deferred), each with gradients that are
                                   never clipped (the in-place form's early exit) and with gradients that always are; then the achieved GB/s
                                   of mi_grad_sumsq alone.  `--rounds` interleaved passes over all forms; min .. max over the passes is the
                                   run-to-run spread
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

MAX_NORM = 50.0
SHRINK = 0.9995        # "always clipped": an in-place clip leaves the norm AT max_norm, so every step asks for a little less than the last


def ms_per(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def optimiser_forms(named, clipped):
    """{form: callable of one clip + optimiser step}; every form owns clones of the parameters with fixed gradients"""
    from minimagen_amd.optim import Adam, clip_grad_norm_
    g = torch.Generator().manual_seed(0)
    scale = (20.0 * MAX_NORM if clipped else MAX_NORM / 50.0) / sum(p.numel() for _, p in named) ** 0.5        # a norm of 20 max_norm, or of max_norm / 50
    grads = [(torch.randn(p.shape, generator=g) * scale).to(p.device) for _, p in named]

    def clones():
        ps = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        return ps

    def limit(state):
        if clipped:
            state[0] *= SHRINK
        return state[0]
    forms = {}
    for tag in ("A", "B"):
        ps = clones()
        forms[f"torch clip + Adam [{tag}]"] = (lambda ps, o, s: lambda: (torch.nn.utils.clip_grad_norm_(ps, limit(s)), o.step()))(ps, Adam(ps, lr=1e-6), [MAX_NORM])
    ps = clones()
    forms["device clip + Adam"] = (lambda ps, o, s: lambda: (clip_grad_norm_(ps, limit(s)), o.step()))(ps, Adam(ps, lr=1e-6), [MAX_NORM])
    ps = clones()
    opt = Adam(ps, lr=1e-6, max_grad_norm=MAX_NORM)             # (the gradients are never rewritten: a fixed limit clips at every step)
    forms["Adam(max_grad_norm=)"] = opt.step
    norm = float(torch.sqrt(sum(gr.double().pow(2).sum() for gr in grads)))
    return forms, norm, opt


def bench_steps(title, named, args):
    n_el = sum(p.numel() for _, p in named)
    print(f"## {title}: {len(named)} tensors, {n_el / 1e6:.2f} M elements "
          f"(Adam 28 B / element = {28 * n_el / 1e6:.0f} MB; torch's clip +12 B, in place +4 .. 12 B, deferred +4 B)")
    for clipped in (False, True):
        forms, norm, opt = optimiser_forms(named, clipped)
        print(f"# gradient norm {norm:.3g} against max_norm {MAX_NORM:g}: {'every step clips' if clipped else 'nothing is clipped'}")
        res = {k: [] for k in forms}
        for fn in forms.values():
            ms_per(fn, args.warmup)
        for _ in range(args.rounds):                        # interleaved: every pass visits every form
            for k, fn in forms.items():
                res[k].append(ms_per(fn, args.steps))
        assert (float(opt.grad_norm) > MAX_NORM) == clipped
        print(f"{'form':26s} median ms/step      min      max   ({args.rounds} passes of {args.steps} steps)")
        for k, v in res.items():
            print(f"{k:26s} {statistics.median(v):14.4f} {min(v):8.4f} {max(v):8.4f}")
        med = {k: statistics.median(v) for k, v in res.items()}
        two = [med["torch clip + Adam [A]"], med["torch clip + Adam [B]"]]
        print(f"# torch's form against itself: |A - B| = {abs(two[0] - two[1]):.4f} ms; device clip - min(A, B) = {med['device clip + Adam'] - min(two):+.4f} ms; "
              f"Adam(max_grad_norm=) - min(A, B) = {med['Adam(max_grad_norm=)'] - min(two):+.4f} ms")
        del forms, opt
        torch.cuda.empty_cache()


def bench_sumsq(title, named, args):
    from minimagen_amd import _lib as L
    from minimagen_amd.optim import CHUNK, _upload
    g = torch.Generator().manual_seed(0)
    grads = [(torch.randn(p.shape, generator=g) * 1e-3).to(p.device) for _, p in named]
    dev = grads[0].device
    tens, ct, co, n = _upload([(0, gr.data_ptr(), 0, 0, gr.numel()) for gr in grads], dev)
    a = L.MiAdamParams()
    a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK
    partials = torch.empty(n, dtype=torch.float64, device=dev)
    lib, stream = L.lib(), L.current_stream()
    fn = lambda: L.check(lib.mi_grad_sumsq(C.byref(a), partials.data_ptr(), stream), "mi_grad_sumsq")
    ms_per(fn, args.warmup)
    v = [ms_per(fn, args.steps) for _ in range(args.rounds)]
    nbytes = 4 * sum(gr.numel() for gr in grads)
    gbs = [nbytes / (ms * 1e-3) / 1e9 for ms in v]
    print(f"## {title}: mi_grad_sumsq alone, {nbytes / 1e6:.0f} MB read in {n} workgroups ({n / len(grads):.1f} chunks per tensor), back-to-back launches")
    print(f"{'':26s}      median ms      min      max   ({args.rounds} passes of {args.steps} launches)")
    print(f"{'mi_grad_sumsq':26s} {statistics.median(v):14.4f} {min(v):8.4f} {max(v):8.4f}")
    print(f"# {statistics.median(gbs):.0f} GB/s median ({min(gbs):.0f} .. {max(gbs):.0f}); a float4 copy on this part measures 6.29 TB/s (read + write)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--timesteps", type=int, default=25)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_clip.py measures on the GPU"
    import bench
    from minimagen_amd import _lib as L
    from minimagen_amd.Unet import Unet
    dev = torch.device("cuda:0")
    print(f"# tools/bench_clip.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(L.DEFAULT_LIB)}, max_norm {MAX_NORM:g}, fp32, host clock around "
          f"synchronised windows")
    cascade, sizes = bench.build_imagen("cascade64_256", args.timesteps, dev)
    torch.manual_seed(0)
    base = Unet().to(dev)
    sets = ((f"SR U-Net (unet_1 of the benched cascade {sizes})", list(cascade.unets[1].named_parameters())), ("Unet() default", list(base.named_parameters())))
    for title, named in sets:
        bench_steps(title, named, args)
    bench_sumsq(*sets[1], args)


if __name__ == "__main__":
    main()
