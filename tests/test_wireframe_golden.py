"""CPU checks of the wireframe step's own numpy statement (tests/wireframe_ref.py): it reproduces every
fixture the real reference made (tests/golden/make_wireframe_golden.py), and its clustering equals
scikit-learn's DBSCAN(eps, min_samples=1) labels on random sets, chains and grids."""
import numpy as np
import pytest

import wireframe_ref
from wireframe_golden_util import S, bar, case_names, check_against_fixture, load_case, recipe_inputs, wf_conf

CASES = ("wf_d128", "wf_forced_b2", "wf_free_b1", "wf_independent_lines", "wf_keep_points", "wf_radius5")


def test_every_case_has_a_fixture():
    assert tuple(case_names()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(name):
    z, meta = load_case(name)
    recipe = meta["recipe"]
    inp = recipe_inputs(recipe)
    got = wireframe_ref.wireframe(inp, wf_conf(recipe), z["fill_junctions"], z["fill_keypoints"], s=S, dtype=np.float64)
    np.testing.assert_array_equal(np.stack(got["labels"]), z["labels"])
    np.testing.assert_array_equal(np.stack(got["removed"]), z["removed"])
    arrays = {k: np.stack(got[k]) for k in ("keypoints", "keypoint_scores", "descriptors", "lines", "lines_junc_idx",
                                            "pl_associativity")}
    arrays.update(line_scores=got["line_scores"], orig_lines=got["orig_lines"], num_junctions=np.asarray(got["num_junctions"]))
    dev = check_against_fixture(z, recipe, inp, arrays)
    print(name, {k: (v, bar(z, k)) for k, v in dev.items()})
    assert sorted(meta["output_keys"]) == sorted(["descriptors", "keypoint_scores", "keypoints", "line_scores", "lines",
                                                  "lines_junc_idx", "num_junctions", "orig_lines", "pl_associativity",
                                                  "valid_lines"])


def _sklearn_labels(pts, eps):
    from sklearn.cluster import DBSCAN

    return DBSCAN(eps=eps, min_samples=1).fit(np.asarray(pts, np.float32)).labels_


def test_labels_equal_sklearn_dbscan():
    rng = np.random.Generator(np.random.PCG64(7))
    sets = []
    for i in range(100):  # dense enough that chains of merges form
        n = int(rng.integers(1, 120))
        sets.append((rng.random((n, 2)) * rng.choice([20.0, 40.0, 80.0]), float(rng.choice([3, 5, 2.5]))))
    chain = np.stack([np.arange(64) * 2.9, np.zeros(64)], 1)
    sets += [(chain, 3.0), (chain[::-1], 3.0), (chain[rng.permutation(64)], 3.0),
             (np.concatenate([chain, chain + [0, 3.5]]), 3.0)]
    gx, gy = np.meshgrid(np.arange(8) * 3.0, np.arange(6) * 3.0)  # exactly eps apart: one component (<=)
    grid = np.stack([gx.ravel(), gy.ravel()], 1)
    sets += [(grid, 3.0), (grid[rng.permutation(len(grid))], 3.0), (grid * 1.01, 3.0)]
    for pts, eps in sets:
        pts = np.asarray(pts, np.float32)
        want = _sklearn_labels(pts, eps)
        got, n = wireframe_ref.cluster_labels(pts, eps)
        np.testing.assert_array_equal(got, want)
        assert n == len(set(want.tolist()))
    assert wireframe_ref.cluster_labels(grid.astype(np.float32), 3.0)[1] == 1
    assert wireframe_ref.cluster_labels((grid * 1.01).astype(np.float32), 3.0)[1] == len(grid)
