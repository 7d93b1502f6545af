"""Snapshot of the launch plans ``UnetEngine.workspace()`` builds on the emulator backend: one line per launch of ``prog_pre``, ``prog_cond`` and
``prog`` -- entry name, struct type, every non-pointer field (nested structs and arrays included), every pointer reduced to null / non-null.
Fields that are zero (null pointers, all-zero structs and arrays) are not written: what a line does not name is zero.

    python tools/dump_conv_plans.py | gzip -n -9 > tests/golden/conv_plans.txt.gz        (zcat shows the text)

tests/test_unet.py::test_launch_plans_match_the_recorded_snapshot rebuilds the plans and compares them with that file line for line: a change
that is meant to leave every launch as it is (a refactor of the plan builder) must reproduce it word for word.  Only the public plan entries and
struct fields are read.  Nothing is launched; the activations are never touched."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from minimagen_amd import engine as E  # noqa: E402
from minimagen_amd.Unet import Unet  # noqa: E402

_POINTERS = (C.c_void_p, C.c_char_p)


def _value(ctype, v) -> str:
    """"" for a zero / null / all-zero value (such fields are left out of the line: a field that is not named is zero)"""
    if issubclass(ctype, _POINTERS):
        return "ptr" if v else ""
    if issubclass(ctype, C.Structure):
        inner = _fields(v)
        return "{" + inner + "}" if inner else ""
    if issubclass(ctype, C.Array):
        elems = [_value(ctype._type_, e) or "0" for e in v]
        return "[" + ",".join(elems) + "]" if any(e != "0" for e in elems) else ""
    return repr(v) if v else ""


def _fields(s: C.Structure) -> str:
    named = ((name, _value(ctype, getattr(s, name))) for name, ctype in s._fields_)
    return " ".join(f"{name}={val}" for name, val in named if val)


def plan_lines(ws):
    for prog in ("prog_pre", "prog_cond", "prog"):
        for _, p, name in getattr(ws, prog):
            yield f"  {prog} {name} " + ("call" if p is None else f"{type(p).__name__} {_fields(p)}")


@contextlib.contextmanager
def _knobs(**kw):
    old = {k: getattr(E, k) for k in kw}
    for k, v in kw.items():
        setattr(E, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(E, k, v)


def _golden_unet(which):
    from tests import _inputs as I
    u = Unet(**I.unet_params()[which])
    u.load_state_dict(I.load(f"{which}_sd.pt"), strict=True)
    return u.eval()


def _seeded_unet(seed, **kw):
    torch.manual_seed(seed)
    return Unet(**kw).eval()


VARIANTS = (("default", {}), ("pipelined", dict(pipelined=True)), ("half", dict(precision="half")), ("nofold", dict(fold=False)))


def cases():
    """-> (label, knobs, make_unet, [(B, size, workspace kwargs label, workspace kwargs)]): guidance batches, B2 = 2 B"""
    from tests.test_unet import WIDE_SMALL
    u0, u1 = (lambda: _golden_unet("unet0")), (lambda: _golden_unet("unet1"))
    wide = lambda: _seeded_unet(5, **WIDE_SMALL)
    both = VARIANTS[:2]
    yield "unet0", {}, u0, [(B, 64, n, kw) for B in (2, 32) for n, kw in VARIANTS] + [(8, 32, "default", {}), (2, 48, "default", {}), (2, 20, "default", {})]
    yield "unet1", {}, u1, [(B, 256, n, kw) for B in (2, 32) for n, kw in VARIANTS] + [(32, S, n, kw) for S in (128, 64) for n, kw in both] \
        + [(2, 1024, "default", {})]
    yield "unet0 CFG_FOLD=2", dict(CFG_FOLD=2), u0, [(32, 64, "default", {})]
    yield "unet0 CONV_STRIPE=''", dict(CONV_STRIPE=""), u0, [(32, 64, "pipelined", dict(pipelined=True))]
    yield "unet1 CONV_STRIPE=''", dict(CONV_STRIPE=""), u1, [(32, 256, "pipelined", dict(pipelined=True))]
    yield "wide_small", {}, wide, [(B, S, "default", {}) for S in (16, 32, 64, 128) for B in (1, 8)]
    yield "wide_small CONV_WIDE_GEMM=False", dict(CONV_WIDE_GEMM=False), wide, [(B, S, "default", {}) for S in (16, 128) for B in (1, 8)]
    yield "Unet()", {}, (lambda: _seeded_unet(0)), [(8, 64, "default", {})]


def dump():
    """every line of the snapshot (the emulator backend must be set up: tests/_backend.setup("emu"))"""
    lines = []
    for label, knobs, make, shapes in cases():
        with _knobs(**knobs):               # (CONV_WIDE_GEMM is read when the weights are packed too: a fresh U-Net per knob setting)
            u = make()
            for B, S, vname, kw in shapes:
                ws = u.engine().workspace(B, 2 * B, S, S, **kw)
                lines.append(f"# {label} B={B} {S}x{S} {vname}")
                lines += plan_lines(ws)
                u.engine().invalidate()     # one workspace alive at a time
    return lines


if __name__ == "__main__":
    from tests._backend import setup
    setup("emu")
    print("\n".join(dump()))
