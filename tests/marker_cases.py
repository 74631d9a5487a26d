"""The `AddMarkers` cases of tests/golden/markers.npz, stated once: tests/golden/make_golden_markers.py runs the reference on them, tests/test_markers_cpu.py
runs `counterfactualworldmodels_amd.perturbation.AddMarkers`.  Plain data; loads neither the native library nor the reference.

Frames: B = 2 movies of T = 2 frames, 3 x 16 x 24, values k / 255; patches of 4 pixels: a 4 x 6 grid, 48 tokens.  MASK: frame 1 masked, frame 0 visible except
its patches (1, 1) and (3, 5) of row 1."""
import numpy as np

B, T, C, H, W, P = 2, 2, 3, 16, 24, 4
GRID = (T, H // P, W // P)
SEED = 11


def frames():
    return (np.random.RandomState(SEED).randint(0, 256, size=(B, T, C, H, W)) / 255.0).astype(np.float32)


def mask():
    m = np.zeros((B,) + GRID, dtype=bool)
    m[:, 1] = True
    m[1, 0, 1, 1] = m[1, 0, 3, 5] = True
    return m.reshape(B, -1)


def points():
    """perturbation points of the `points` case: True at the first 5 tokens of every row"""
    p = np.zeros((B, int(np.prod(GRID))), dtype=bool)
    p[:, :5] = True
    return p


# name -> (constructor keywords, call keywords).  `as4`: what the reference is given instead of a 2- or 3-entry index (its forward fails on those after
# painting them, perturbation.py:456): the index completed as its own painter completes it (:391-403).
CASES = {
    "full_fixed": (dict(), dict(patch_idx_list=[[0, 0, 1, 2], [1, 0, 3, 4]])),
    "cross_fixed": (dict(marker_shapes=["cross"], marker_color=[0, 1, 0.5]), dict(patch_idx_list=[[0, 0, 0, 0], [1, 0, 2, 3]])),
    "listed_colours": (dict(marker_shapes=["full", "cross"], marker_color=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], seed=3),
                       dict(patch_idx_list=[[0, 0, 0, 1], [0, 0, 2, 2], [1, 0, 3, 0], [1, 0, 0, 5], [0, 0, 3, 3]])),
    "random_colour": (dict(marker_shapes=["full", "cross"], marker_color=None, seed=5), dict(patch_idx_list=[[0, 0, 1, 1], [1, 0, 2, 4], [1, 0, 0, 0], [0, 0, 3, 5]])),
    "two_entries": (dict(marker_shapes=["cross"]), dict(patch_idx_list=[[1, 2]], as4=[[0, 0, 1, 2]])),
    "three_entries": (dict(marker_color=[0.25, 0.5, 1]), dict(patch_idx_list=[[1, 1, 2], [0, 3, 3]], as4=[[1, 0, 1, 2], [0, 0, 3, 3]])),
    "one_flat_index": (dict(), dict(patch_idx_list=[1, 0, 2, 2])),
    "repeated_patch": (dict(marker_shapes=["full", "cross"], marker_color=None, seed=7),
                       dict(patch_idx_list=[[0, 0, 1, 1], [1, 0, 2, 2], [0, 0, 1, 1], [0, 0, 1, 1], [1, 0, 2, 2]])),
    "masked_source": (dict(), dict(patch_idx_list=[[1, 0, 1, 1], [1, 0, 3, 5], [0, 0, 1, 1]])),
    "black_marker": (dict(marker_color=[0, 0, 0]), dict(patch_idx_list=[[1, 0, 1, 1]])),
    "empty_default": (dict(), dict()),
    "frame_none": (dict(marker_shapes=["full", "cross"], marker_color=None, seed=2), dict(patch_idx_list=[[1, 1, 2, 3], [0, 0, 0, 0], [0, 1, 3, 5]], frame=None)),
    "frame_none_empty": (dict(), dict(frame=None)),
    "frame_one": (dict(marker_shapes=["cross"], marker_color=[0, 0, 1]), dict(patch_idx_list=[[1, 0, 1, 2], [0, -1, 0, 5]], frame=1)),
    "random_patches": (dict(marker_shapes=["full", "cross"], marker_color=None, seed=9), dict(num_random_patches=3)),
    "random_patches_any_frame": (dict(marker_shapes=["full", "cross"], marker_color=[[1, 1, 0], [0, 1, 1]], seed=4), dict(num_random_patches=2, frame=None)),
    "points": (dict(), dict(patch_idx_list=[[0, 0, 0, 1], [1, 0, 2, 2]], points=True)),
}
