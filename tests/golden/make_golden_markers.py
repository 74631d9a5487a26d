"""Goldens of the marker counterfactual prompts, recorded by RUNNING THE REFERENCE's `AddMarkers` (cwm/models/perturbation.py:356-476) on the CPU (through
ref_import.py) on the cases of tests/marker_cases.py -> markers.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_markers.py

  markers.npz   per case `<name>_x` [2,2,3,16,24] float32 and `<name>_mask` [2,48] bool: what the reference's forward returns.  The inputs are not stored:
                marker_cases.frames() / mask() / points() rebuild them.

The reference's forward paints a 2- or 3-entry patch index and then fails on it in its un-masking loop (:456).  For those cases the reference is given the
index completed to (b, t, h, w) the way its own painter completes it (:391-403), and the maker checks that the reference's painter, given the short index
itself, paints exactly the same frames -- and that the forward does fail on it.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import marker_cases as MC  # noqa: E402


def run_reference(ns, ctor, call, x, mask):
    call = dict(call)
    short = call.get("patch_idx_list") if "as4" in call else None
    if "as4" in call:
        call["patch_idx_list"] = call.pop("as4")
    if call.pop("points", False):
        call["perturbation_points"] = torch.from_numpy(MC.points())
    A = ns.perturbation.AddMarkers((1, MC.P, MC.P), **ctor)
    xm, mm = A(x.clone(), mask.clone(), **call)
    if short is not None:
        # the painter on the short index itself: the same frames ...
        A2 = ns.perturbation.AddMarkers((1, MC.P, MC.P), **ctor)
        A2.set_shapes(x, mask)
        img = x[:, 0].unsqueeze(1).clone()
        for idx in short:
            img = A2.add_marker_to_patch(img, A2.sample_marker(x), idx)
        assert torch.equal(torch.cat([img, x[:, 1:]], 1), xm), "the reference's painter completes a short index differently"
        # ... and the forward fails on it
        try:
            ns.perturbation.AddMarkers((1, MC.P, MC.P), **ctor)(x.clone(), mask.clone(), patch_idx_list=short)
        except IndexError:
            pass
        else:
            raise AssertionError("the reference's forward accepts a short index now: record it directly")
    return xm, mm


def main():
    ns = ref_import.import_reference()
    x, mask = torch.from_numpy(MC.frames()), torch.from_numpy(MC.mask())
    out = {}
    for name, (ctor, call) in MC.CASES.items():
        xm, mm = run_reference(ns, ctor, call, x, mask)
        assert xm.shape == x.shape and xm.dtype == torch.float32 and mm.shape == mask.shape and mm.dtype == torch.bool, name
        out[name + "_x"], out[name + "_mask"] = xm.numpy(), mm.numpy()
        print("[golden] %-26s %3d pixels changed, mask: %d tokens un-masked" % (name, int((xm != x).any(2).sum()), int((mm != mask).sum())))
    # what the cases are there to show
    assert np.array_equal(out["empty_default_x"], x.numpy()) and np.array_equal(out["empty_default_mask"], mask.numpy())
    assert not out["masked_source_mask"].reshape(MC.B, *MC.GRID)[1, 0, 1, 1] and int((out["masked_source_mask"] != mask.numpy()).sum()) == 2
    assert np.array_equal(out["full_fixed_mask"], mask.numpy()) and not np.array_equal(out["full_fixed_x"], x.numpy())
    assert np.array_equal(out["black_marker_x"], x.numpy()) and not np.array_equal(out["black_marker_mask"], mask.numpy())
    path = os.path.join(HERE, "markers.npz")
    np.savez_compressed(path, **out)
    print("[golden] markers.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
