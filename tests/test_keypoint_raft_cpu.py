"""The keypoint RAFT (`output_dim=1`) without a GPU: the state dict against the reference's recorded 183 keys, the parameter count, the
`load_raft_model(None, output_dim=1)` line, checkpoint loading, and the values of `output_dim` that stay unsupported."""
import json
import os

import numpy as np
import pytest
import torch

from counterfactualworldmodels_amd import config as C, synthetic as S
from counterfactualworldmodels_amd import raft as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    return np.load(os.path.join(GOLDEN, "raft_keypoint_224_b1.npz"))


def test_state_dict_matches_the_reference_keys_shapes_and_order():
    g = golden()
    want = [(k, tuple(v)) for k, v in json.loads(str(g["keys"]))]
    assert len(want) == 183
    assert [k for k, _ in want[-4:]] == ["output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"]
    assert list(C.raft_state_dict_schema(output_dim=1).items()) == want
    m = R.RAFT(R._args(output_dim=1))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert sum(v.numel() for v in m.parameters()) == int(g["num_parameters"]) == 5552961
    sd = S.raft_state_dict(3, output_dim=1)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    # the flow model and its generators are what they were
    assert len(R.RAFT().state_dict()) == 179 and R.RAFT().output_block is None
    assert len(C.raft_state_dict_schema()) == 179 and len(S.raft_state_dict(3)) == 179
    assert all(np.array_equal(sd[k], v) for k, v in S.raft_state_dict(3).items())


def test_load_raft_model_without_a_path_creates_a_new_model(capsys):
    m = R.load_raft_model(None, output_dim=1)
    assert capsys.readouterr().out.strip() == "created a new RAFT with 5552961 parameters"  # raft_model.py:94-96
    assert isinstance(m.output_block, torch.nn.Sequential) and m.multiframe and m.scale_inputs and m.output_dim == 1
    assert m.output_block[0].weight.shape == (256, 128, 3, 3) and m.output_block[2].weight.shape == (1, 256, 1, 1)


def test_other_output_dims_stay_unsupported(tmp_path):
    for d in (2, 64):
        with pytest.raises(NotImplementedError):
            R.load_raft_model(None, output_dim=d)
        with pytest.raises(NotImplementedError):
            R.RAFT(R._args(output_dim=d))
    with pytest.raises(ValueError):  # no path and no head: still the reference's error
        R.load_raft_model(None)


def test_reference_style_checkpoint_loads(tmp_path, capsys):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in S.raft_state_dict(1, output_dim=1).items()}
    path = str(tmp_path / "keypoints.pth")
    torch.save({"module." + k: v for k, v in sd.items()}, path)
    m = R.load_raft_model(path, output_dim=1)
    assert "All keys matched successfully" in capsys.readouterr().out
    got = m.state_dict()
    # (`norm3` is the same module as `downsample.1`, listed twice in the state dict: one of the two synthetic tensors wins)
    assert all(torch.equal(got[k], v) for k, v in sd.items() if ".norm3." not in k)
    assert all(torch.equal(got[k], sd[k]) for k in ("output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"))
    # the notebook's way: a fresh model, then load_state_dict of the checkpoint's 'model' entry
    m2 = R.load_raft_model(None, output_dim=1)
    assert str(m2.load_state_dict(sd)) == "<All keys matched successfully>"
    # a flow checkpoint into the keypoint model leaves exactly the head unloaded (strict=False)
    torch.save({k: v for k, v in sd.items() if not k.startswith("output_block")}, path)
    R.load_raft_model(path, output_dim=1)
    out = capsys.readouterr().out
    assert all(k in out for k in ("output_block.0.weight", "output_block.0.bias", "output_block.2.weight", "output_block.2.bias"))
    assert "unexpected_keys=[]" in out and "fnet" not in out.split("unexpected_keys")[0]


def test_forward_without_a_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    m = R.load_raft_model(None, output_dim=1)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 2, 3, 128, 128))
