"""tests/prompt_kernels_restatement.py pinned without a GPU: it reproduces every recorded multi-shift case of the reference (tests/golden/multi_shift.npz,
frames and masks bit for bit) and, for one whole-patch step, equals `oracle.vmae_oracle.create_motion_counterfactuals` on a non-square three-frame case."""
import numpy as np
import torch

import prompt_kernels_restatement as PR
from oracle import vmae_oracle as O
from test_multi_shift_cpu import REQUIRED_CASES, input_frames, load_cases

# every case the fixture must hold, by name: the sixteen 32 x 32 / 32 x 48 cases at P = 4 / 8 and the three at patch sizes that are no multiple of 4
GOLDEN_CASES = ["p8_random", "p4_random_frame0", "wide_k4", "border_subpatch", "negative_subpatch", "axis_and_zero_steps", "odd_sx", "sx_multiples_of_4",
                "chain", "overlap", "leaves_frame", "frame_minus1", "no_points", "base_mask_2d", "k1", "k_max",
                "p6_12x24", "p6_24x12", "p12_24x24"]


def test_restatement_reproduces_every_recorded_multi_shift_case():
    g, meta = load_cases()
    assert list(meta) == GOLDEN_CASES == REQUIRED_CASES
    for tag in GOLDEN_CASES:
        c = meta[tag]
        H, W, P, frame = c["H"], c["W"], c["P"], c["frame"] % 2
        x = input_frames(2, H, W)
        points, base, shifts = PR.tables_of_golden_case(g, c, tag)
        assert points.shape == (2, c["K"], 2 * (H // P) * (W // P)) and shifts.shape == (2, c["K"], 2)
        got_x = PR.multi_shift_frames(x, points, shifts, P, frame)
        got_m = PR.multi_shift_mask(points, base, shifts, P, frame, 2, H, W)
        assert np.array_equal(got_x.view(np.uint32), g["case_%s_x_p" % tag].view(np.uint32)), tag
        assert np.array_equal(got_m, g["case_%s_mask_ps" % tag]), tag
        # the counts the maker recorded, from the restatement alone
        assert int((got_x[:, frame] != x[:, frame]).sum()) == c["moved"] > 0 and int((got_x == 0).sum()) == c["zeros"], tag


def test_one_whole_patch_step_equals_the_oracle_on_a_non_square_three_frame_case():
    """K = 1 with shifts of whole patches is the single-shift prompt: B = 2 movies x S = 3 prompts at 16 x 24, P = 8 (a 2 x 3 grid), T = 3, C = 2, frame 2,
    per-prompt shifts (inside, leaving the grid on either axis, zero), the movie as given and as a static movie."""
    gen = torch.Generator().manual_seed(11)
    B, S_, T, Cc, H, W, P, frame = 2, 3, 3, 2, 16, 24, 8, 2
    gh, gw = H // P, W // P
    n = gh * gw
    x = torch.rand(B, T, Cc, H, W, generator=gen)
    passive = torch.rand(B, T * n, S_, generator=gen) < 0.6
    active = torch.ones(B, T * n, S_, dtype=torch.bool)
    for b in range(B):
        for s in range(S_):
            active[b, frame * n + torch.randperm(n, generator=gen)[:2], s] = False
            active[b, int(torch.randint(n, (1,), generator=gen)), s] = False   # a point of another frame: re-masked, never moved
    shifts = [(1, 0), (0, -1), (-1, 2), (0, 0), (2, 0), (0, 3)]
    R = B * S_
    rows = lambda a: a.permute(0, 2, 1).reshape(R, 1, T * n).numpy()  # noqa: E731  '(b s)' rows, one step
    pixel = (np.array(shifts) * P).reshape(R, 1, 2)
    for fix_passive in (False, True):
        want_x, want_m = O.create_motion_counterfactuals(x, passive, active, shifts, P, frame=frame, fix_passive=fix_passive)
        assert want_x.shape == (R, T, Cc, H, W) and not torch.equal(want_x[:, frame], x[:, 0 if fix_passive else frame].repeat_interleave(S_, 0))
        got_x = PR.multi_shift_frames(x.numpy(), rows(~active), pixel, P, frame, S=S_, fix_passive=int(fix_passive))
        got_m = PR.multi_shift_mask(rows(~active), rows(passive), pixel, P, frame, T, H, W)
        assert np.array_equal(got_x.view(np.uint32), want_x.numpy().view(np.uint32)), fix_passive
        assert np.array_equal(got_m, want_m.numpy()), fix_passive
        if fix_passive:   # the static movie has T frames: every frame but `frame` is frame 0
            assert all(torch.equal(want_x[:, t], x[:, 0].repeat_interleave(S_, 0)) for t in range(T) if t != frame)


def test_prompt_table_expand_restated_against_tensor_operations():
    """In-grid rows against the indexed assignment the kernel replaced; out-of-grid rows clear nothing and keep their shifts."""
    S_, T, gh, gw, frame = 6, 3, 2, 5, 2
    n = gh * gw
    table = np.array([[0, 0, 1, -1], [1, 4, 0, 2], [0, 5, 3, 3], [2, 0, -4, 0], [1, -1, 5, 6], [-1, 2, 7, 8]], dtype=np.int32)
    active, passive, shifts = PR.prompt_table_expand(table, T, gh, gw, frame)
    ref_passive = np.broadcast_to(np.arange(T * n) >= n, (S_, T * n))
    ref_active = ref_passive.copy()
    ref_active[0, frame * n + 0] = False
    ref_active[1, frame * n + 1 * gw + 4] = False
    assert np.array_equal(passive, ref_passive) and np.array_equal(active, ref_active) and np.array_equal(shifts, table[:, 2:])
