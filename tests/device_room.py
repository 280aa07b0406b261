"""For the argument-error tests of the services that take caller-owned device memory: a run of n images that ends one byte behind
the allocation its tensor lies in.  The engine refuses by the allocation's end as the HIP runtime reports it, and torch's caching
allocator carves small tensors out of larger blocks, so the stride comes from the same runtime query: for a tensor that is an
allocation of its own it is the image size, and the tensor is one byte short of (n - 1) * image_stride + image_bytes."""
import ctypes as C

import torch


def room(L, ptr):
    """bytes from ptr to the end of its device allocation; L: the loaded engine library (the runtime it links answers)"""
    base, size = C.c_void_p(), C.c_size_t()
    assert L.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(ptr)) == 0
    return base.value + size.value - ptr


def one_byte_short(L, n, image_bytes, fill=0xA5):
    """(tensor, image_stride, bytes to claim): the n-th image ends one byte behind the end of the tensor's allocation"""
    t = torch.full((n * image_bytes - 1,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    left = room(L, t.data_ptr())
    assert left >= t.numel()
    stride = (left + 1 - image_bytes) // (n - 1)
    assert stride >= image_bytes and (n - 1) * stride + image_bytes == left + 1, "n - 1 does not divide what is left"
    return t, stride, left + 1
