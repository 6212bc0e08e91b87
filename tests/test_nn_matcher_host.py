"""Host side of the nearest-neighbour matcher (lightglue_amd.nn_matcher): registry names, the
reference's configuration, the loss rules, the CPU-input error and the argument checks of the two C
entries -- no GPU needed."""
import ctypes

import pytest
import torch

import lgamd  # noqa: F401
from lightglue_amd import _lib
from lightglue_amd.pipeline import TwoViewPipeline, get_model


def test_nn_matcher_resolves_by_both_names_with_the_reference_configuration():
    from lightglue_amd.nn_matcher import NearestNeighborMatcher, __main_model__

    assert get_model("matchers.nearest_neighbor_matcher") is NearestNeighborMatcher
    assert get_model("nearest_neighbor_matcher") is NearestNeighborMatcher
    assert __main_model__ is NearestNeighborMatcher
    m = NearestNeighborMatcher({})
    # nearest_neighbor_matcher.py:39-44 plus the two extra keys
    assert {k: m.conf[k] for k in NearestNeighborMatcher.default_conf} == {
        "ratio_thresh": None, "distance_thresh": None, "mutual_check": True, "loss": None,
        "similarity": True, "log_assignment": True}
    assert list(NearestNeighborMatcher.default_conf)[:4] == ["ratio_thresh", "distance_thresh", "mutual_check", "loss"]
    assert m.required_data_keys == ["descriptors0", "descriptors1"]
    pipe = TwoViewPipeline({"matcher": {"name": "matchers.nearest_neighbor_matcher", "ratio_thresh": 0.8}})
    assert isinstance(pipe.matcher, NearestNeighborMatcher) and pipe.matcher.conf.ratio_thresh == 0.8


def test_nn_matcher_loss_rules():
    m = get_model("nearest_neighbor_matcher")({})
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    with pytest.raises(NotImplementedError, match="N_pair"):
        get_model("nearest_neighbor_matcher")({"loss": "N_pair"})


def test_nn_matcher_rejects_cpu_inputs_and_missing_keys():
    from lightglue_amd.nn_matcher import nn_match

    m = get_model("nearest_neighbor_matcher")({})
    data = {"descriptors0": torch.zeros(1, 4, 8), "descriptors1": torch.zeros(1, 5, 8)}
    with pytest.raises(RuntimeError, match="HIP"):
        m(data)
    with pytest.raises(RuntimeError, match="HIP"):
        nn_match(data["descriptors0"], data["descriptors1"], ratio_thresh=0.8)
    with pytest.raises(AssertionError, match="descriptors1"):
        m({"descriptors0": data["descriptors0"]})


def test_nn_c_entries_check_their_arguments():
    lib = _lib.load()
    assert {"lg_nn_workspace_bytes", "lg_nn_match"} <= set(_lib.EXPORTED_SYMBOLS)
    nb = ctypes.c_size_t()

    def bytes_of(B, M, N, D, flags=0):
        assert lib.lg_nn_workspace_bytes(B, M, N, D, flags, ctypes.byref(nb)) == _lib.LG_OK
        return nb.value

    base_sz = bytes_of(2, 300, 257, 256)
    assert base_sz > 0
    # the descriptor planes (4 bytes per element, rows padded to the tile) and partials of
    # (M ceil(N / 256) + N ceil(M / 256)) entries: nothing of size M * N
    assert bytes_of(2, 2048, 2048, 256) < 2 * 2048 * 2048 * 4 // 2
    assert bytes_of(1, 1, 1, 1) > 0
    assert bytes_of(2, 300, 257, 256) <= bytes_of(3, 300, 257, 256) <= bytes_of(3, 600, 257, 256)
    assert bytes_of(3, 600, 257, 256) <= bytes_of(3, 600, 700, 256) <= bytes_of(3, 600, 700, 512)
    assert bytes_of(2, 130, 77, 96) < bytes_of(2, 130, 77, 100)  # the zero-padded copy of an odd width
    assert bytes_of(2, 300, 257, 256, 7) == base_sz
    assert lib.lg_nn_workspace_bytes(2, 300, 257, 256, 0, None) == _lib.LG_E_INVALID and b"null" in lib.lg_last_error()
    assert lib.lg_nn_workspace_bytes(2, -1, 257, 256, 0, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert b"negative" in lib.lg_last_error()
    assert lib.lg_nn_workspace_bytes(2, 300, 257, 513, 0, ctypes.byref(nb)) == _lib.LG_E_INVALID
    assert b"512" in lib.lg_last_error()
    assert lib.lg_nn_workspace_bytes(2, 300, 257, 0, 0, ctypes.byref(nb)) == _lib.LG_E_INVALID

    # host memory stands in for the device pointers: every call below returns before any launch
    buf = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    # desc0 desc1 | num0 num1 sim la m0 m1 s0 s1
    NULLABLE = {2, 3, 4, 5}

    def call(B=1, M=4, N=4, D=32, ptrs=None, flags=0, ws=p, ws_bytes=1 << 30):
        a = [p] * 10 if ptrs is None else ptrs
        return lib.lg_nn_match(a[0], a[1], B, M, N, D, 0.64, 0.49, flags, *a[2:], ws, ws_bytes, None)

    def with_(**at):
        ptrs = [p] * 10
        for k, v in at.items():
            ptrs[int(k[1:])] = v
        return ptrs

    for k in sorted(set(range(10)) - NULLABLE):
        assert call(ptrs=with_(**{f"i{k}": None})) == _lib.LG_E_INVALID, k
        assert b"null" in lib.lg_last_error()
    assert call(M=-4) == _lib.LG_E_INVALID and b"negative" in lib.lg_last_error()
    assert call(D=-32) == _lib.LG_E_INVALID and b"negative" in lib.lg_last_error()
    assert call(B=2, M=40000, N=40000) == _lib.LG_E_INVALID and b"2^31" in lib.lg_last_error()
    assert call(D=513) == _lib.LG_E_INVALID and b"512" in lib.lg_last_error()
    assert call(D=0) == _lib.LG_E_INVALID and b"512" in lib.lg_last_error()
    assert call(flags=8) == _lib.LG_E_INVALID and b"flag" in lib.lg_last_error()
    assert call(ws_bytes=8) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(ws=None) == _lib.LG_E_INVALID and b"workspace" in lib.lg_last_error()
    assert call(ws=ctypes.c_void_p(base + 16)) == _lib.LG_E_INVALID and b"aligned" in lib.lg_last_error()
    assert call(ptrs=with_(i2=None)) == _lib.LG_E_INVALID and b"both" in lib.lg_last_error()  # one count array alone
    assert call(M=1, flags=1) == _lib.LG_E_INVALID and b"ratio" in lib.lg_last_error()
    assert call(N=1, flags=1) == _lib.LG_E_INVALID and b"ratio" in lib.lg_last_error()
    off4, off2 = ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    assert call(ptrs=with_(i0=off4)) == _lib.LG_E_INVALID and b"16-byte" in lib.lg_last_error()  # D % 32 == 0
    assert call(D=20, ptrs=with_(i1=off2)) == _lib.LG_E_INVALID and b"16-byte" in lib.lg_last_error()
    assert call(ptrs=with_(i6=off4)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # matches0
    assert call(ptrs=with_(i9=off2)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # scores1
    assert call(ptrs=with_(i4=off2)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # similarity
    assert call(ptrs=with_(i5=off2)) == _lib.LG_E_INVALID and b"misaligned" in lib.lg_last_error()  # log assignment
    # the nullable ones may be null, an odd width may be 4-byte aligned: accepted up to the next check
    assert call(D=20, ptrs=with_(i0=off4, i2=None, i3=None, i4=None, i5=None), ws_bytes=8) == _lib.LG_E_INVALID
    assert b"workspace" in lib.lg_last_error()
    # an empty side: OK, nothing launched (no workspace needed either)
    for B, M, N in ((0, 4, 4), (3, 0, 7), (3, 7, 0)):
        assert call(B, M, N, ws=None, ws_bytes=0) == _lib.LG_OK


def test_abi_version_is_unchanged():
    assert _lib.load().lg_abi_version() == 12 == _lib.ABI_VERSION
