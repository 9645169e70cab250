"""FASTA -> records of byte text, the parts that need no device: the per-thread step of fasta2_text_kernel (compact32,
mm_fasta_text.h - the kept bytes of a 32-byte piece moved together) run on the host through mm_debug_compact32 against
numpy boolean indexing, and the argument checks of mm_fasta_text_device_async / mm_fasta_text_device."""
import ctypes as C

import numpy as np


def _bytes32(seed):
    """32 input bytes that include 0x00 and 0xFF (a kept zero byte must not look like 'nothing kept')."""
    a = np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)
    a[[0, 5, 31]] = 0x00
    a[[1, 17, 30]] = 0xFF
    return a


def _compact(sm, data, mask):
    out = np.full(32, 0xA5, dtype=np.uint8)
    n = sm.lib().mm_debug_compact32(data.ctypes.data_as(C.POINTER(C.c_uint8)), int(mask) & 0xFFFFFFFF,
                                    out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return n, out


def _check(sm, data, mask):
    keep = ((int(mask) >> np.arange(32)) & 1).astype(bool)
    want = data[keep]
    n, out = _compact(sm, data, mask)
    assert n == len(want), hex(mask)
    assert np.array_equal(out[:n], want), hex(mask)
    assert not out[n:].any(), hex(mask)  # zeros behind the kept bytes: the kernel ORs them into LDS


def _run(first, length):
    return ((1 << length) - 1) << first


def test_compact32_empty_and_full(sm):
    for seed in range(3):
        data = _bytes32(seed)
        _check(sm, data, 0)
        _check(sm, data, 0xFFFFFFFF)


def test_compact32_every_single_run(sm):
    data = _bytes32(10)
    for first in range(32):
        for length in range(1, 32 - first + 1):
            _check(sm, data, _run(first, length))


def test_compact32_every_pair_of_runs_around_a_line_end(sm):
    """Two runs separated by one ('\\n') or two ('\\r\\n') dropped bytes: a line end inside the piece."""
    data = _bytes32(11)
    n = 0
    for gap in (1, 2):
        for f1 in range(32):
            for l1 in range(1, 32 - f1):
                f2 = f1 + l1 + gap
                for l2 in range(1, 32 - f2 + 1):
                    _check(sm, data, _run(f1, l1) | _run(f2, l2))
                    n += 1
    assert n > 9000


def test_compact32_random_masks(sm):
    """10 000 random masks: nearly all hold more than two runs (the rare path)."""
    rng = np.random.default_rng(12)
    masks = rng.integers(0, 1 << 32, 10_000, dtype=np.uint64)
    masks[::3] &= rng.integers(0, 1 << 32, len(masks[::3]), dtype=np.uint64)   # sparse
    masks[1::3] |= rng.integers(0, 1 << 32, len(masks[1::3]), dtype=np.uint64)  # dense
    for i, m in enumerate(masks):
        _check(sm, _bytes32(100 + i % 7), int(m))


def test_compact32_null_pointers(sm):
    data = _bytes32(1)
    p = data.ctypes.data_as(C.POINTER(C.c_uint8))
    assert sm.lib().mm_debug_compact32(None, 1, p) == sm.ERR["NULL"]
    assert sm.lib().mm_debug_compact32(p, 1, None) == sm.ERR["NULL"]


def test_argument_checks_without_a_device(sm):
    """Refused before any device call: a null workspace (asynchronous form), null out_counts / null workspace
    (synchronous form)."""
    L, E = sm.lib(), sm.ERR
    counts = (C.c_uint64 * 2)()
    fake = C.c_void_p(64)  # (never dereferenced: the checks come first)
    assert L.mm_fasta_text_device_async(None, fake, 10, fake, 16, fake, None, 4, fake) == E["NULL"]
    assert L.mm_fasta_text_device(fake, fake, 10, fake, 16, fake, None, 4, fake, None) == E["NULL"]
    assert L.mm_fasta_text_device(None, fake, 10, fake, 16, fake, None, 4, fake, counts) == E["NULL"]
