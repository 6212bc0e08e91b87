"""Ragged batches for SuperGlue and the Sinkhorn head: everything that needs no GPU.

The C ABI additions, the count validation of the Python entries, the capacity frame of the shared
reference helper (tests/sg_ragged_ref.py) on a case written out by hand, and the near-tie condition
of every seeded SuperGlue case of tests/test_gpu_sg_ragged.py, computed with the CPU oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

import lgamd  # noqa: F401
import sg_ragged_ref as ref
from lightglue_amd import _lib

NEW = ("sg_forward_ragged", "lg_log_optimal_transport_ragged", "lg_filter_matches_ragged")


def test_new_exports_and_abi_version():
    lib = _lib.load()
    for s in NEW:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.lg_abi_version() == 12 and _lib.ABI_VERSION == 12
    assert lib.lg_sinkhorn_rerun_count() >= 0


def test_struct_sizes_unchanged():
    # sg_inputs_t: 3 int32 (+ pad) + 8 pointers + 4 int32; sg_outputs_t: 8 pointers (ABI 12)
    assert ctypes.sizeof(_lib.SGInputs) == 96
    assert ctypes.sizeof(_lib.SGOutputs) == 64


def test_one_null_count_is_invalid_without_touching_the_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the argument check comes first
    assert lib.lg_log_optimal_transport_ragged(None, 1.0, 1, 2, 2, one, None, 1, None, None, 0, None) == _lib.LG_E_INVALID
    assert b"together" in lib.lg_last_error()
    assert lib.lg_filter_matches_ragged(None, 1, 2, 2, 0.0, None, one, None, None, None, None, None, 0, None) == _lib.LG_E_INVALID
    assert lib.sg_forward_ragged(None, None, one, None, None, None, 0, None) == _lib.LG_E_INVALID
    # both NULL is the existing entry (here: its own null-argument error)
    assert lib.lg_log_optimal_transport_ragged(None, 1.0, 1, 2, 2, None, None, 1, None, None, 0, None) == _lib.LG_E_INVALID
    assert b"null" in lib.lg_last_error()


def _sg_data(B=2, M=5, N=4):
    g = torch.Generator().manual_seed(0)
    view = {"image_size": torch.tensor([[640.0, 480.0]] * B)}
    return {"keypoints0": torch.rand((B, M, 2), generator=g) * 400, "keypoints1": torch.rand((B, N, 2), generator=g) * 400,
            "descriptors0": torch.randn((B, M, 256), generator=g), "descriptors1": torch.randn((B, N, 256), generator=g),
            "keypoint_scores0": torch.rand((B, M), generator=g), "keypoint_scores1": torch.rand((B, N), generator=g),
            "view0": view, "view1": dict(view)}


def test_superglue_count_validation():
    from lightglue_amd import SuperGlue

    m = SuperGlue({"GNN_layers": ["self", "cross"]}).eval()
    d = _sg_data()
    ok = torch.tensor([5, 3])
    with pytest.raises(ValueError, match="integer dtype"):
        m({**d, "num_keypoints0": torch.tensor([5.0, 3.0]), "num_keypoints1": ok})
    with pytest.raises(ValueError, match="shape"):
        m({**d, "num_keypoints0": torch.tensor([5, 3, 1]), "num_keypoints1": ok})
    with pytest.raises(ValueError, match="together"):
        m({**d, "num_keypoints0": ok})
    with pytest.raises(NotImplementedError, match="training"):
        m.train()({**d, "num_keypoints0": ok, "num_keypoints1": torch.tensor([4, 2])})
    # valid counts pass the validation and reach the device check (there is no CPU path)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.eval()({**d, "num_keypoints0": ok, "num_keypoints1": torch.tensor([4, 2])})


def test_functional_count_validation():
    from lightglue_amd import filter_matches, log_optimal_transport

    s = torch.zeros(2, 3, 3)
    for fn, args in ((log_optimal_transport, (s, 1.0, 3)), (filter_matches, (torch.zeros(2, 4, 4), 0.1))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args, torch.tensor([1, 2]), torch.tensor([1, 2]))


def test_capacity_frame_by_hand():
    """B = 2 at capacities 2 x 3: pair 0 has (1, 2) real points, pair 1 is empty (n1 = 0)."""
    ninf = -np.inf
    p0 = {"la": np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]),  # [n0+1, n1+1]: block | dustbin column / dustbin row | corner
          "cost": np.array([[7.0, 8.0]]), "m0": np.array([1]), "m1": np.array([-1, 0]), "s0": np.array([0.5]),
          "s1": np.array([0.0, 0.5]), "d0": np.array([[9.0, 9.5]]), "d1": np.array([[1.5, 2.5], [3.5, 4.5]])}
    out = ref.to_capacity([p0, None], 2, 3, ((1, 2), (2, 0)))
    want_la = np.array([[[1.0, 2.0, ninf, 3.0],
                         [ninf, ninf, ninf, ninf],
                         [4.0, 5.0, ninf, 6.0]],
                        [[ninf, ninf, ninf, ninf],
                         [ninf, ninf, ninf, ninf],
                         [ninf, ninf, ninf, 0.0]]], np.float32)
    np.testing.assert_array_equal(out["log_assignment"], want_la)
    np.testing.assert_array_equal(out["matches0"], [[1, -1], [-1, -1]])
    np.testing.assert_array_equal(out["matches1"], [[-1, 0, -1], [-1, -1, -1]])
    np.testing.assert_array_equal(out["matching_scores0"], [[0.5, 0.0], [0.0, 0.0]])
    np.testing.assert_array_equal(out["matching_scores1"], [[0.0, 0.5, 0.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(out["sinkhorn_cost"], [[[7.0, 8.0, 0.0], [0.0, 0.0, 0.0]], np.zeros((2, 3))])
    np.testing.assert_array_equal(out["gnn_descriptors0"], [[[9.0, 9.5], [0.0, 0.0]], np.zeros((2, 2))])
    np.testing.assert_array_equal(out["gnn_descriptors1"][0], [[1.5, 2.5], [3.5, 4.5], [0.0, 0.0]])


def test_sinkhorn_reference_frame_is_the_per_pair_oracle():
    """The Sinkhorn helper on a tiny case: each pair's block is the oracle alone at its own size."""
    import oracle

    g = torch.Generator().manual_seed(3)
    scores = torch.randn((2, 4, 5), generator=g).numpy()
    z = ref.sk_reference(scores, ((4, 5), (2, 3)), 1.0, 5)
    full = oracle.log_optimal_transport(torch.from_numpy(scores[:1]), 1.0, 5)[0].numpy()
    np.testing.assert_array_equal(z[0], full)
    own = oracle.log_optimal_transport(torch.from_numpy(scores[1:, :2, :3].copy()), 1.0, 5)[0].numpy()
    np.testing.assert_array_equal(z[1, :2, :3], own[:2, :3])
    np.testing.assert_array_equal(z[1, :2, 5], own[:2, 3])
    np.testing.assert_array_equal(z[1, 4, :3], own[2, :3])
    assert z[1, 4, 5] == own[2, 3]
    assert np.isneginf(z[1]).sum() == 5 * 6 - (2 * 3 + 2 + 3 + 1)


@pytest.mark.parametrize("name", sorted(ref.SG_CASES))
def test_near_tie_cap_of_the_seeded_cases(name):
    """A condition on the seeds, not a measurement: at most 2 % of a case's real points may lie inside
    the near-tie band (where the GPU test cannot demand the oracle's decision)."""
    r, c, share = ref.sg_decided(name)
    print(name, "near-tie share", share)
    assert share <= ref.NEAR_TIE_CAP, share
    counts = ref.SG_CASES[name]["counts"]
    for b, (n0, n1) in enumerate(counts):  # padding is never "decided": it is checked exactly instead
        assert not r[b, n0:].any() and not c[b, n1:].any()
