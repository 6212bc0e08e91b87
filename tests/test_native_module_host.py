"""Host-side check of lightglue_amd._native.NativeModule (no GPU, no library): the handle life
cycle, the weight upload keyed by the version counters, and the workspace cache, against a fake
library that records its calls."""
import gc

import pytest
import torch
from torch import nn


class FakeLib:
    def __init__(self):
        self.calls = []

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)

    def x_create(self, h):
        self.calls.append(("x_create",))
        h.value = 0x1234
        return 0

    def x_destroy(self, h):
        self.calls.append(("x_destroy", h.value))
        return 0

    def x_load_weights(self, h, n, names, ptrs, numels, stream):
        self.calls.append(("x_load_weights", h.value, [names[i].decode() for i in range(n)], [ptrs[i] for i in range(n)],
                           [numels[i] for i in range(n)]))
        return 0


class NoStream:
    cuda_stream = 0

    def synchronize(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    from lightglue_amd import _lib

    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "_lib", lib)  # what __del__ reads: it must not load a library
    return lib


def make_module():
    from lightglue_amd._native import NativeModule

    class Two(NativeModule):
        _native_prefix = "x"
        _native_name = "Two: parameter"

        def __init__(self):
            super().__init__()
            self.a = nn.Parameter(torch.arange(6.0).reshape(2, 3))
            self.b = nn.Parameter(torch.zeros(2))
            self._native_init()

        def _create_handle(self, lib, device, h):
            assert lib.x_create(h) == 0

        def _weights_signature(self):
            return tuple((n, p.data_ptr(), p._version) for n, p in self.named_parameters())

        def _upload_stream(self, device):  # the CPU has no stream to upload on
            return NoStream()

    return Two()


CPU = torch.device("cpu")


def test_handle_is_created_once_and_weights_follow_the_version_counters(fake):
    m = make_module()
    assert m._handle is None
    assert m._ensure_handle(CPU, upload=False) is fake
    assert fake.count("x_create") == 1 and fake.count("x_load_weights") == 0  # upload=False: no upload
    assert m._handle.value == 0x1234 and m._handle_device == CPU
    m._ensure_handle(CPU)
    m._ensure_handle(CPU)
    assert fake.count("x_create") == 1 and fake.count("x_load_weights") == 1
    _, h, names, ptrs, numels = fake.calls[-1]
    assert h == 0x1234 and names == ["a", "b"] and numels == [6, 2]
    assert ptrs == [m.a.data_ptr(), m.b.data_ptr()]

    with torch.no_grad():
        m.a.add_(1.0)  # in place: the version counter moves
    m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 2
    m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 2

    m.reload_weights()
    m._ensure_handle(CPU, upload=False)
    assert fake.count("x_load_weights") == 2
    m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 3

    m.to(torch.float32)  # through _apply, even when nothing moves
    m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 4
    assert fake.count("x_create") == 1 and fake.count("x_destroy") == 0


def test_a_parameter_that_is_not_fp32_raises(fake):
    m = make_module().double()
    with pytest.raises(RuntimeError, match=r"Two: parameter a is torch\.float64 on cpu; move the module to cpu in fp32"):
        m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 0
    m.float()
    m._ensure_handle(CPU)
    assert fake.count("x_load_weights") == 1


def test_workspace_only_grows(fake):
    m = make_module()
    ws = m._workspace_bytes(100, CPU)
    assert ws.dtype == torch.uint8 and ws.numel() == 100
    assert m._workspace_bytes(10, CPU) is ws
    assert m._workspace_bytes(100, CPU) is ws
    big = m._workspace_bytes(101, CPU)
    assert big is not ws and big.numel() == 101
    assert m._workspace_bytes(50, CPU) is big


def test_del_destroys_the_handle_exactly_once(fake):
    m = make_module()
    m._ensure_handle(CPU)
    never = make_module()  # no handle: nothing to destroy
    del m, never
    gc.collect()
    assert [c for c in fake.calls if c[0] == "x_destroy"] == [("x_destroy", 0x1234)]


def test_every_model_with_a_handle_is_a_native_module():
    from lightglue_amd import ALIKED, LightGlue, SuperGlue, SuperPoint, SuperPointOpen
    from lightglue_amd._native import NativeModule

    prefixes = {LightGlue: "lg", SuperGlue: "sg", SuperPoint: "sp", SuperPointOpen: "sp", ALIKED: "sp_aliked"}
    for cls, prefix in prefixes.items():
        assert issubclass(cls, NativeModule), cls
        assert cls._native_prefix == prefix
        assert "__del__" not in vars(cls), cls
        assert all("__del__" not in vars(k) for k in cls.__mro__ if k not in (NativeModule, object)), cls
    assert "__del__" in vars(NativeModule)
    assert issubclass(SuperPointOpen, SuperPoint)
