#!/usr/bin/env python3
"""Generate tests/golden/align_overlap.npz from the REFERENCE itself.

Runs only where a checkout of the reference exists (TMLIB_REFERENCE, default
/root/reference).  tmlib/workflow/align/registration.py
is loaded on its own, with a stub ``image_registration`` module in
``sys.modules`` (the library is not installed; ``calculate_overlap`` does not
use it), and ``calculate_overlap`` is run on the shift lists below.  Only the
inputs and results are written (data); no reference text is stored.

    python tests/golden/make_align_goldens.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TMLIB_REFERENCE", "/root/reference")

#: (y shifts, x shifts) of one site across its cycles; the reference cycle's 0 included
CASES = [
    ([0], [0]),                                # a single cycle
    ([0, 0, 0], [0, 0, 0]),                    # all zero
    ([0, 5], [0, 3]),                          # positive only
    ([0, -5], [0, -3]),                        # negative only
    ([0, 5], [0, -3]),
    ([0, -5], [0, 3]),
    ([0, 4, -7], [0, -2, 9]),                  # mixed signs
    ([0, -1, -2, -3], [0, 1, 2, 3]),
    ([0, 12, 3, 7], [0, 0, 0, 0]),             # no x shift at all
    ([0, 0, 0], [0, -8, 8]),
    ([3], [-4]),                               # one target, no reference entry
    ([-3], [4]),
    ([0, 1, -1], [0, -1, 1]),
    ([0, 100, -100, 50], [0, -100, 100, -50]),
    ([0, 2, 2, 2], [0, -2, -2, -2]),           # repeated extremes
    ([0, -6, 6, -6, 6], [0, 6, -6, 6, -6]),
    ([5, 4, 3, 2, 1], [1, 2, 3, 4, 5]),        # no zero among them
    ([-5, -4, -3], [-1, -2, -3]),
    ([0, 1080], [0, -1280]),                   # half a full-size site
    ([0, -1, 0, 1, 0], [0, 0, -1, 0, 1]),
    ([], []),                                  # no cycle at all
]


def load_registration():
    sys.modules.setdefault("image_registration", types.ModuleType("image_registration"))
    path = os.path.join(REF, "tmlib", "workflow", "align", "registration.py")
    spec = importlib.util.spec_from_file_location("reference_align_registration", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    reg = load_registration()
    out = {"n_cases": np.array(len(CASES), np.int64)}
    for i, (ys, xs) in enumerate(CASES):
        res = reg.calculate_overlap(list(ys), list(xs))
        out["y_%02d" % i] = np.array(ys, np.int64)
        out["x_%02d" % i] = np.array(xs, np.int64)
        out["overlap_%02d" % i] = np.array([int(v) for v in res], np.int64)  # top, bottom, right, left
    np.savez_compressed(os.path.join(HERE, "align_overlap.npz"), **out)
    print("wrote align_overlap.npz: %d cases" % len(CASES))


if __name__ == "__main__":
    main()
