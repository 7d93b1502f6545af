"""Trace of what ``Imagen.sample()`` does on the host for a fixed matrix of calls: a dozen calls on the tiny 16 -> 32 cascade of
tests/test_init_image.py (B = 2, T = 25), made in one process in a fixed order, one per keyword family (and one repeated: a cache hit).
Per call it records
  launches     the names passed to ``_lib.check`` in order, run-length encoded (the U-Net's own launches do not pass through it)
  workspaces   per stage, every workspace key of the engine -> its sampler-state keys -> the graph keys that state holds
all keys as ``repr`` strings.  ``--hash`` adds the SHA-256 of each call's image bytes.

    python tools/dump_sample_trace.py | gzip -n -9 > tests/golden/sample_trace.json.gz        (emulator; zcat shows the text)
    python tools/dump_sample_trace.py --backend gpu --hash -o profiles/sample_trace_gpu.json

tests/test_sample_trace.py regenerates the emulator trace and compares it with the committed one: a change that is meant to leave every
workspace, state, graph key and launch of sample() as it is (a refactor of the call plumbing) must reproduce it word for word.  Only the
public ``sample()`` keywords, ``_lib.check`` and the caches the benchmark reads are used."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from minimagen_amd import _lib as L  # noqa: E402

B, T = 2, 25


def calls(dev):
    """-> [(label, keywords)]; a callable keyword value is called with the previous call's images (the cascade cut in two)"""
    from oracle import restated as R
    from tests.test_init_image import pixels
    emb, mask = (t.to(dev) for t in R.synthetic_text(B, length=16, seed=7))
    neg, nmask = (t.to(dev) for t in R.synthetic_text(B, length=12, seed=9))
    text = dict(text_embeds=emb, text_masks=mask, _seed=11)
    known = dict(inpaint_images=pixels(B, 24, 3).to(dev), inpaint_masks=(pixels(B, 24, 4)[:, 0] > 0.5).to(dev))
    init = pixels(B, 32, 6).to(dev)
    table = torch.tensor([[1., 1.], [1., 1.], [2., 3.], [3., 3.], [3., 1.]])
    return [
        ("default", dict(text, cond_scale=3.)),
        ("default again", dict(text, cond_scale=3.)),
        ("strided ddpm S=5, stop_at_stage=1", dict(text, cond_scale=3., sample_steps=5, stop_at_stage=1)),
        ("start_at_stage=1, ddim eta=0.5 S=(5, 7)", dict(text, cond_scale=3., sample_steps=(5, 7), sampler="ddim", sampler_eta=0.5, start_at_stage=1,
                                                          start_image=lambda prev: prev)),
        ("init + inpaint + dpmpp_2m S=5", dict(text, cond_scale=3., sample_steps=5, sampler="dpmpp_2m", init_images=init, init_strength=0.6, **known)),
        ("inpaint, strided ddpm S=5", dict(text, cond_scale=3., sample_steps=5, **known)),
        ("negative embeds + rescale, ddim S=5", dict(text, cond_scale=3., sample_steps=5, sampler="ddim", negative_text_embeds=neg,
                                                      negative_text_masks=nmask, guidance_rescale=0.5)),
        ("interval (0, 0.5): two runs, S=5", dict(text, cond_scale=3., sample_steps=5, guidance_interval=(0., 0.5))),
        ("schedule [None, [S, B] table], S=5", dict(text, sample_steps=5, guidance_schedule=[None, table])),
        ("init_strength=[0.6, None]", dict(text, cond_scale=3., init_images=init, init_strength=[0.6, None])),
        ("injected noise, S=5", dict(text, cond_scale=3., sample_steps=5, _noise=R.make_randn(8))),
        ("eager, S=5", dict(text, cond_scale=3., sample_steps=5, _use_graph=False)),
    ]


def caches(im):
    """per stage: workspace key -> state key -> [graph keys], as the engines hold them now"""
    return [{repr(wk): {repr(sk): [repr(gk) for gk in st.graphs] for sk, st in ws.sampler_state.items()} for wk, ws in u.engine()._ws.items()}
            for u in im.unets]


def trace(backend: str = "emu", hashes: bool = False):
    """-> the list of per-call records (sets up the backend: tests/_backend.setup)"""
    from tests._backend import setup
    from tests.test_init_image import tiny_cascade
    dev = setup(backend)
    im, _ = tiny_cascade(T, dev)
    names, check = [], L.check

    def recording_check(rc, what=""):
        if names and names[-1][0] == what:
            names[-1][1] += 1
        else:
            names.append([what, 1])
        return check(rc, what)

    out, records = None, []
    L.check = recording_check
    try:
        for label, kw in calls(dev):
            kw = {k: (v(out) if callable(v) and k != "_noise" else v) for k, v in kw.items()}
            del names[:]
            out = im.sample(**kw).clone()
            im.check_device_status()
            rec = dict(call=label, launches=[list(x) for x in names], workspaces=caches(im))
            if hashes:
                rec["sha256"] = hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest()
            records.append(rec)
    finally:
        L.check = check
    return records


def text(records) -> str:
    return json.dumps(records, indent=1) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--backend", choices=("emu", "gpu"), default="emu")
    ap.add_argument("--hash", action="store_true", help="add the SHA-256 of each call's image bytes")
    ap.add_argument("-o", "--output", help="write here instead of the standard output")
    args = ap.parse_args()
    doc = text(trace(args.backend, args.hash))
    if args.output:
        with open(args.output, "w") as f:
            f.write(doc)
    else:
        sys.stdout.write(doc)
