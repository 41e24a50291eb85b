"""What a *_host entry answers to device index -1 when every other argument
is sound: the shared prelude (use_device in csrc/host_common.h) counts the
devices first, so the answer depends on whether the machine has one."""
import os

from audiotools import _atgpu

NO_DEVICE = (_atgpu.ATG_ERR_DEVICE, b"no HIP device available")
OUT_OF_RANGE = (_atgpu.ATG_ERR_INVALID, b"device index out of range")


def gpu_visible():
    return os.path.exists("/dev/kfd") and os.environ.get("HIP_VISIBLE_DEVICES", "x") != ""


def check_refused(status, component):
    """`status` came back from atg_<component>..._host(-1, ...)"""
    lib = _atgpu.load_library()
    got = (status, getattr(lib, "atg_%s_last_error" % component)())
    assert got in (NO_DEVICE, OUT_OF_RANGE), got
    if not gpu_visible():
        assert got == NO_DEVICE, got
    return got
