"""K-mer values of every sequence of a device batch in one launch: what needs no GPU - the exports, the size of the LDS
stage, the refusals that come before the device is touched, the per-sequence view the host derives
(mm_debug_values_batch_view), and the C++ example's compile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mm_values_u64_batch_device_async", "mm_values_u128_batch_device_async", "mm_device_group_values_batch",
           "mm_device_group_batch_values")
DESCRIPTOR_BYTES = 32  # ValuesBatchSeq: aligned address, byte_lo, byte_hi, base0


def test_entry_points_exported_and_wrapped(sm):
    L = sm.lib()
    for name in ENTRIES + ("mm_values_batch_lds_stage", "mm_debug_values_batch_view"):
        assert hasattr(L, name), name
        assert name in sm.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("values_batch_device", "values_batch_lds_stage", "values_batch_view"):
        assert callable(getattr(sm, name)), name
    for name in ("values_batch", "batch_values"):
        assert callable(getattr(sm.DeviceGroup, name)), name
    stage = sm.values_batch_lds_stage()
    assert 2 <= stage
    assert stage * (8 + DESCRIPTOR_BYTES) <= 64 * 1024  # an offset and a descriptor per entry, in a workgroup's 64 KiB


def test_null_workspace_and_null_group_need_no_device(sm):
    L, E = sm.lib(), sm.ERR
    fake = C.c_void_p(4096)  # (never dereferenced: the refusals come first)
    ptrs = (C.c_void_p * 1)(4096)
    one = np.array([16], dtype=np.uint64)
    offs = np.array([0, 4], dtype=np.uint64)
    p = lambda a: sm._p(a, C.c_uint64)
    for name in ENTRIES[:2]:
        assert getattr(L, name)(None, 1, ptrs, p(one), None, p(one), 21, 1, fake, p(offs), fake) == E["NULL"], name
        # with a NULL workspace the answer is MM_ERR_NULL whatever else is wrong
        assert getattr(L, name)(None, 1, ptrs, p(one), None, p(one), 0, 1, fake, p(offs), fake) == E["NULL"], name
    total = C.c_uint64()
    for u128 in (0, 1):
        assert L.mm_device_group_values_batch(None, 21, 1, u128, C.byref(total)) == E["NULL"]
    entry, dv, cnt = C.c_int(), C.POINTER(C.c_uint64)(), C.c_uint64()
    assert L.mm_device_group_batch_values(None, 0, C.byref(entry), C.byref(dv), C.byref(cnt)) == E["NULL"]


@pytest.mark.parametrize("packed_bytes", [0, 1, 3, 4, 5, 64])
def test_view_of_one_descriptor(sm, packed_bytes):
    """Every byte shift 0..3 and base offsets 0..17: the address comes back 4-aligned, byte_lo is the shift, the byte
    range has packed_bytes bytes, [q_lo, q_hi) are exactly the dwords that lie wholly inside it, base0 counts the shift."""
    for shift in range(4):
        for base_offset in range(18):
            address = 0x7F0012345600 + shift
            v = sm.values_batch_view(address, packed_bytes, base_offset)
            assert v["address"] % 4 == 0 and v["address"] == address - shift
            assert v["byte_lo"] == shift
            assert v["byte_hi"] - v["byte_lo"] == packed_bytes
            inside = [q for q in range(0, 20) if 4 * q >= v["byte_lo"] and 4 * q + 4 <= v["byte_hi"]]
            assert list(range(v["q_lo"], v["q_hi"])) == inside, (shift, packed_bytes, v)
            assert v["base0"] == base_offset + 4 * shift
    assert sm.lib().mm_debug_values_batch_view(4096, 4, 0, None) == sm.ERR["NULL"]


def test_cxx_values_batch_example_compiles(sm):
    """tests/cxx/values_batch_example.cpp builds against the header-only mirror and the in-tree library."""
    cxx = os.path.join(ROOT, "tests", "cxx")
    subprocess.run(["make", "-C", cxx, "-f", "values_batch_example.mk"], check=True, capture_output=True)
    assert os.path.exists(os.path.join(cxx, "values_batch_example"))
