"""Shared by the tests that read the VALUE of an amax word (csrc/common.h: 64 bits of device memory, (epoch << 32) | bits of max |x|, written
by the kernel that produced the tensor).  The reference is the word's definition -- the integer maximum over the magnitudes of what was stored,
taken on the tensor read back from the device -- so every comparison here is exact.  No test functions."""
import ctypes

import torch

_hip = []


def read_word(addr):
    """(epoch, bits) of the amax word at device address `addr`: an 8-byte device-to-host copy behind a device synchronisation"""
    if not _hip:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.append(hip)
    host = ctypes.c_uint64(0)
    torch.cuda.synchronize()
    assert _hip[0].hipMemcpy(ctypes.byref(host), ctypes.c_void_p(addr), 8, 2) == 0   # hipMemcpyDeviceToHost
    return int(host.value) >> 32, int(host.value) & 0xFFFFFFFF


def own_word():
    """(int64 cuda tensor of one zero, its address): a word the test owns -- every C-ABI entry that takes an amax word accepts any uint64_t*
    (keep the tensor alive while the address is in use)"""
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    return t, t.data_ptr()


def abs_bits(t):
    """bits of max |t| in the integer order on magnitudes (-0.0 -> 0, any NaN above inf), 0 for an empty tensor; t: a float32 tensor, read
    back from the device first"""
    assert t.dtype == torch.float32
    if t.numel() == 0:
        return 0
    return int((t.detach().cpu().contiguous().view(torch.int32) & 0x7FFFFFFF).max())


def as_float(bits):
    return torch.tensor([bits], dtype=torch.int64).to(torch.int32).view(torch.float32).item()


def expect(addr, epoch, t, what=""):
    """the word at `addr` carries `epoch` and exactly the bits of max |t|"""
    got, want = read_word(addr), (int(epoch) & 0xFFFFFFFF, abs_bits(t))
    assert got == want, "%s amax word: epoch %d, %r (0x%08x); want epoch %d, %r (0x%08x) = max |tensor|" % (
        what, got[0], as_float(got[1]), got[1], want[0], as_float(want[1]), want[1])
