"""Golden vectors of `InputPadder` (cwm/models/raft/utils.py:9-26), captured by RUNNING THE REFERENCE's class on the CPU (this container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raft_padder.py

raft_input_padder.npz holds, for each of the sizes below and both modes, the `_pad` list the reference computes ([left, right, top, bottom]), and one
seeded 1 x 3 x 7 x 9 array with its padded form and the `unpad` of that, per mode.  The sizes: a Sintel frame (436 x 1024), a KITTI frame (375 x 1242),
a size that needs nothing (224 x 224), one with an odd and an even remainder (129 x 130: 7 and 6 to add) and the small array's own (7 x 9).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_raft import raft_module  # noqa: E402

SIZES = ((436, 1024), (375, 1242), (224, 224), (129, 130), (7, 9))
MODES = ("sintel", "kitti")


def main():
    raft_module()  # puts the reference on the path (and its stubs in place)
    utils = importlib.import_module("cwm.models.raft.utils")
    out = {"sizes": np.array(SIZES, dtype=np.int64), "modes": np.array(MODES)}
    for mode in MODES:
        out["pad_" + mode] = np.array([utils.InputPadder((1, 3, h, w), mode=mode)._pad for h, w in SIZES], dtype=np.int64)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(21)).standard_normal((1, 3, 7, 9)).astype(np.float32))
    out["x"] = x.numpy()
    for mode in MODES:
        padder = utils.InputPadder(x.shape, mode=mode)
        (y,) = padder.pad(x)
        assert y.shape[-2] % 8 == 0 and y.shape[-1] % 8 == 0
        z = padder.unpad(y)
        assert torch.equal(z, x)
        out["padded_" + mode] = y.numpy()
        out["unpadded_" + mode] = z.numpy()
    np.savez_compressed(os.path.join(HERE, "raft_input_padder.npz"), **out)
    print("[golden] raft_input_padder", {k: v.shape for k, v in out.items()}, out["pad_sintel"].tolist(), out["pad_kitti"].tolist())


if __name__ == "__main__":
    main()
