"""The four <family>_load_weights entries reject the same malformed state dicts with the same
messages (csrc/weight_schema.h), through ctypes on a handle of each family's smallest config.  No
forward runs: these are argument errors, returned before any launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _module(family):
    from lightglue_amd import ALIKED, LightGlue, SuperGlue, SuperPoint

    if family == "lg":
        return LightGlue({"n_layers": 1})
    if family == "sg":
        return SuperGlue({"GNN_layers": ["self"], "keypoint_encoder": [32]})
    if family == "sp":
        return SuperPoint({})
    return ALIKED({"model_name": "aliked-t16"})


@pytest.mark.parametrize("family", ["lg", "sg", "sp", "sp_aliked"])
def test_load_weights_is_strict_with_the_shared_messages(family):
    from lightglue_amd import _lib

    dev = torch.device("cuda", 0)
    model = _module(family)
    lib = model._ensure_handle(dev, upload=False)
    h = model._handle
    fn = {n: getattr(lib, f"{family}_{n}") for n in ("weight_count", "weight_name", "weight_numel", "load_weights")}
    count = fn["weight_count"](h)
    assert count > 2
    schema = [(fn["weight_name"](h, i).decode(), fn["weight_numel"](h, i)) for i in range(count)]
    assert fn["weight_name"](h, count) is None and fn["weight_numel"](h, count) == -1
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def load(entries):
        """entries: (name, numel passed, numel allocated); returns (code, lg_last_error())."""
        keep = [torch.zeros(alloc, device=dev) for _, _, alloc in entries]
        names = (ctypes.c_char_p * len(entries))(*[n.encode() for n, _, _ in entries])
        ptrs = (ctypes.c_void_p * len(entries))(*[t.data_ptr() for t in keep])
        numels = (ctypes.c_int64 * len(entries))(*[k for _, k, _ in entries])
        rc = fn["load_weights"](h, len(entries), names, ptrs, numels, stream)
        torch.cuda.current_stream(dev).synchronize()
        return rc, lib.lg_last_error().decode()

    exact = [(n, k, k) for n, k in schema]
    assert load(exact)[0] == _lib.LG_OK

    last, last_numel = schema[-1]
    assert last_numel > 1
    first = schema[0][0]
    bad = {
        "extra": (exact + [("not.in.the.schema", 1, 1)], "unexpected key in state_dict: not.in.the.schema"),
        "twice": (exact + [exact[0]], f"duplicate key: {first}"),
        "short": (exact[:-1] + [(last, last_numel - 1, last_numel)],
                  f"size mismatch for {last}: expected {last_numel} got {last_numel - 1}"),
        "missing": (exact[:-1], f"missing key in state_dict: {last}"),
    }
    for what, (entries, message) in bad.items():
        rc, err = load(entries)
        assert rc == _lib.LG_E_WEIGHTS, (family, what, rc, err)
        assert err == message, (family, what)
        assert load(exact)[0] == _lib.LG_OK, (family, what)  # a rejected load leaves the handle usable
