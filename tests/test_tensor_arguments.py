"""What :meth:`Context.asdevice` and :meth:`Context._out` do with a caller's tensor, without a GPU: both are driven unbound
on a context that was never opened (``device = 0``, ``to_device`` and ``empty`` replaced by recorders), with real CPU
tensors of torch and a stand-in for tensors on a GPU."""
import types

import numpy as np
import pytest
import torch

from multimesh_amd.device import Context, DeviceArray


class FakeTensor:
    """What the binding layer reads of a tensor on GPU ``index``: an address, a shape, a dtype, a device."""

    def __init__(self, shape, dtype="torch.float64", index=0, ptr=0x7F0000001000, contiguous=True):
        self.shape, self.dtype, self._ptr, self._contiguous = tuple(shape), dtype, ptr, contiguous
        self.device = types.SimpleNamespace(type="cuda", index=index)

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous


@pytest.fixture()
def ctx():
    c = object.__new__(Context)
    c.handle, c.device = None, 0            # (handle None: nothing is released when it is collected)
    c.uploaded, c.allocated = [], []

    def to_device(array, dtype=None):
        a = np.ascontiguousarray(array, dtype=dtype)
        c.uploaded.append(a)
        return DeviceArray(c, 0xD000, a.shape, a.dtype, owner=False)

    def empty(shape, dtype):
        c.allocated.append((tuple(shape), np.dtype(dtype)))
        return DeviceArray(c, 0xE000, shape, dtype, owner=False)

    c.to_device, c.empty = to_device, empty
    return c


def test_a_cpu_tensor_is_copied_not_wrapped(ctx):
    t = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    got = Context.asdevice(ctx, t, np.float64)
    assert len(ctx.uploaded) == 1 and np.array_equal(ctx.uploaded[0], t.numpy()) and ctx.uploaded[0].dtype == np.float64
    assert got.ptr == 0xD000 and got.ptr != t.data_ptr() and got._keepalive is None
    ids = torch.arange(6, dtype=torch.int64).reshape(3, 2)
    Context.asdevice(ctx, ids, np.int64)
    assert np.array_equal(ctx.uploaded[1], ids.numpy()) and ctx.uploaded[1].dtype == np.int64


def test_a_tensor_on_the_contexts_gpu_is_wrapped(ctx):
    x = FakeTensor((4, 3))
    got = Context.asdevice(ctx, x, np.float64)
    assert got.ptr == x.data_ptr() and got.shape == (4, 3) and got.dtype == np.float64
    assert got._owner is False and got._keepalive is x and not ctx.uploaded
    ids = FakeTensor((5,), "torch.int64")
    got = Context.asdevice(ctx, ids, np.int64)
    assert got.ptr == ids.data_ptr() and got.shape == (5,) and got.dtype == np.int64 and got._keepalive is ids


def test_a_tensor_on_another_gpu_is_refused(ctx):
    with pytest.raises(ValueError, match=r"GPU 1\b.*GPU 0\b"):
        Context.asdevice(ctx, FakeTensor((4, 3), index=1), np.float64)
    assert not ctx.uploaded


def test_an_object_without_a_device_is_wrapped_as_before(ctx):
    x = types.SimpleNamespace(data_ptr=lambda: 0xABC0, shape=(2, 2), dtype="float64")
    got = Context.asdevice(ctx, x, np.float64)
    assert got.ptr == 0xABC0 and got._keepalive is x and not ctx.uploaded
    d = DeviceArray(ctx, 0xF000, (3,), np.float64, owner=False)
    assert Context.asdevice(ctx, d, np.float64) is d


@pytest.mark.parametrize("given, wanted", [("torch.float32", np.float64), ("torch.int32", np.int64),
                                           ("torch.float64", np.int64), ("torch.int64", np.float64)])
def test_a_tensor_of_another_type_is_refused(ctx, given, wanted):
    with pytest.raises(TypeError, match=f"expected {np.dtype(wanted)}"):
        Context.asdevice(ctx, FakeTensor((4,), given), wanted)


def test_a_tensor_that_is_not_contiguous_is_refused(ctx):
    with pytest.raises(ValueError, match="contiguous"):
        Context.asdevice(ctx, FakeTensor((4, 3), contiguous=False), np.float64)


def test_a_slice_is_wrapped_at_its_own_address(ctx):
    """The address arithmetic is torch's: a row slice of a real tensor, with the device of a GPU tensor."""
    base = torch.zeros((8, 3), dtype=torch.float64)
    view = base[2:6]
    x = FakeTensor(view.shape, str(view.dtype), ptr=view.data_ptr(), contiguous=view.is_contiguous())
    got = Context.asdevice(ctx, x, np.float64)
    assert got.ptr == base.data_ptr() + 2 * 3 * 8 and got.shape == (4, 3) and got.nbytes == 4 * 3 * 8


def test_a_tensor_without_rows_is_wrapped_empty(ctx):
    got = Context.asdevice(ctx, FakeTensor((0, 3)), np.float64)
    assert got.size == 0 and got.shape == (0, 3) and not ctx.uploaded


@pytest.mark.parametrize("message", [None, "out must be (4, 3)"])
def test_out_on_the_host_or_another_gpu_is_refused(ctx, message):
    for out in (torch.zeros((4, 3), dtype=torch.float64), FakeTensor((4, 3), index=1), np.zeros((4, 3))):
        with pytest.raises(ValueError, match="out must live on GPU 0"):
            Context._out(ctx, out, (4, 3), message)
    assert not ctx.uploaded and not ctx.allocated


def test_out_on_the_contexts_gpu_is_taken_in_place(ctx):
    x = FakeTensor((4, 3))
    got = Context._out(ctx, x, (4, 3), "out must be (4, 3)")
    assert got.ptr == x.data_ptr() and got._keepalive is x and not ctx.allocated
    with pytest.raises(ValueError, match="out must be"):
        Context._out(ctx, x, (3, 4), "out must be (3, 4)")
    assert Context._out(ctx, x, (12,), "size", size_only=True).ptr == x.data_ptr()
    new = Context._out(ctx, None, (4, 3))
    assert ctx.allocated == [((4, 3), np.dtype(np.float64))] and new.ptr == 0xE000


def test_out_of_another_type_is_refused(ctx):
    with pytest.raises(TypeError, match="expected float64"):
        Context._out(ctx, DeviceArray(ctx, 0xF000, (4, 3), np.int64, owner=False), (4, 3))
    with pytest.raises(TypeError, match="expected float64"):
        Context._out(ctx, FakeTensor((4, 3), "torch.float32"), (4, 3))
    with pytest.raises(TypeError, match="expected int64"):
        Context.asdevice(ctx, DeviceArray(ctx, 0xF000, (4,), np.float64, owner=False), np.int64)
