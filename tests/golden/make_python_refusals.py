"""Writes tests/golden/python_refusals.json: for every deliberately wrong call of tests/test_python_refusals.py's CASES
the exception class and message the operators of `vampire_amd` raise, device names and addresses normalised, and the
source lines (file, line) of the package the raise came through.

    python tests/golden/make_python_refusals.py [--package ROOT] [--out FILE]    # on a machine with the GPU

with ROOT the checkout whose refusals are to be kept (the commit before the helpers of `_tensors` were factored out;
default: this one) -- it is regenerated only when a refusal is changed on purpose.  Every case must raise, in Python or
from a host-side refusal of the library: a case that raises nothing would have launched, and stops the run there.

The cap: every line of ROOT's operator modules that raises the "needs device tensors" sentence or formats
`vamp_last_error()` must lie on the traceback of at least one case; the lines are written into the fixture."""
import argparse
import glob
import json
import os
import re
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SITE = re.compile(r"needs device tensors \(no CPU fallback\)|vamp_last_error\(\)")


def sites(package):
    """[(file, line)] of the package's refusal sites (the binding's own errcheck, `_capi.py`, is not an operator)."""
    out = []
    for path in sorted(glob.glob(os.path.join(package, "*.py"))):
        if os.path.basename(path) != "_capi.py":
            with open(path) as f:
                out += [(os.path.basename(path), n) for n, line in enumerate(f, 1) if SITE.search(line)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=REPO, help="the checkout whose vampire_amd is recorded")
    ap.add_argument("--out", default=os.path.join(HERE, "python_refusals.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.package)
    sys.path[:0] = [root, os.path.dirname(HERE)]
    import torch
    import vampire_amd
    import test_python_refusals as T
    package = os.path.dirname(os.path.abspath(vampire_amd.__file__))
    assert package == os.path.join(root, "vampire_amd"), package
    assert torch.cuda.is_available(), "the device cases need the GPU"
    want, cases, hit = sites(package), {}, set()
    for (op, what, gpu, mistake), name in zip(T.CASES, T.IDS):
        raises, exc = T.outcome(op, gpu, mistake)
        assert raises is not None, f"{name}: nothing was raised"
        through = [(os.path.basename(fr.filename), fr.lineno) for fr in traceback.extract_tb(exc.__traceback__)
                   if os.path.dirname(os.path.abspath(fr.filename)) == package]
        assert through, f"{name}: {raises} was not raised through the package"
        hit.update(through)
        cases[name] = {"raises": raises, "sites": [list(s) for s in through if s in want]}
        print(f"{name}: {raises[0]}: {raises[1]}", flush=True)
    missed = [s for s in want if s not in hit]
    assert not missed, f"no case reaches {missed}"
    with open(args.out, "w") as f:
        json.dump({"sites": [list(s) for s in want], "cases": cases}, f, indent=1)
        f.write("\n")
    print(len(cases), "cases,", len(want), "sites")


if __name__ == "__main__":
    main()
