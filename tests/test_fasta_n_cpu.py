"""CPU checks of FASTA / FASTQ with N (mm_fasta_pack_n_*, mm_fastq_pack_n_device_async,
mm_run_packed_reads_skip_ambiguous_*): the new symbols and their Python bindings, and every refusal that needs no
device - each comes before the workspace is looked at (ws = NULL here)."""
import ctypes as C

import numpy as np

NEW_SYMBOLS = [
    "mm_fasta_pack_n_device_async", "mm_fastq_pack_n_device_async", "mm_fasta_pack_n_device",
    "mm_run_packed_reads_skip_ambiguous_device_async", "mm_run_packed_reads_skip_ambiguous_device",
    "mm_run_packed_reads_skip_ambiguous_host",
]


def test_symbols_exported_and_bound(sm):
    L = sm.lib()
    for name in NEW_SYMBOLS:
        assert name in sm.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, name
    assert len(L.mm_fasta_pack_n_device.argtypes) == len(L.mm_fasta_pack_device.argtypes) + 2
    assert len(L.mm_run_packed_reads_skip_ambiguous_device.argtypes) == 16
    assert sm.fastx_pack_n_device is sm.fasta_pack_n_device
    for name in ("run_packed_reads_skip_ambiguous_device", "run_reads_skip_ambiguous_host"):
        assert callable(getattr(sm, name))
    assert sm.FastaRecords(None, np.zeros(1, dtype=np.uint64), []).amb is None  # (the plain packer's records: no bits)


def test_run_argument_checks_without_a_device(sm):
    L = sm.lib()
    E = sm.ERR
    canon = sm.Plan(21, 11, True, 0, None)
    forward = sm.Plan(21, 11, False, 0, None)
    text = sm.Plan(21, 11, True, 0, None, text=True)
    cnt = C.c_uint64()
    fake = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused first)

    def dev(plan, n_reads=4, amb=fake, starts=fake, fn=L.mm_run_packed_reads_skip_ambiguous_device, last=None):
        return fn(plan.h, None, fake, 1 << 20, 0, amb, 1 << 20, 0, n_reads, starts, 1000, 300, fake, 1000, fake,
                  last if last is not None else C.byref(cnt))

    for fn, last in ((L.mm_run_packed_reads_skip_ambiguous_device, None),
                     (L.mm_run_packed_reads_skip_ambiguous_device_async, fake)):
        assert dev(forward, fn=fn, last=last) == E["HASHER_NOT_CANONICAL"]  # src/lib.rs:451: canonical builders only
        assert dev(text, fn=fn, last=last) == E["BAD_MODE"]
        assert dev(canon, starts=None, fn=fn, last=last) == E["NULL"]
        assert dev(canon, amb=None, fn=fn, last=last) == E["NULL"]
        assert dev(canon, fn=fn, last=last) == E["NULL"]  # (the workspace, last)
    # syncmer plans are accepted up to the workspace; a forward syncmer plan is not
    assert dev(sm.Plan(15, 17, True, 1, None)) == E["NULL"]
    assert dev(sm.Plan(15, 17, False, 1, None)) == E["HASHER_NOT_CANONICAL"]

    packed = np.zeros(64, dtype=np.uint8)
    amb = np.zeros(64, dtype=np.uint8)
    pos = np.zeros(100, dtype=np.uint32)
    offs = np.zeros(8, dtype=np.uint64)
    starts = np.array([0, 50, 100], dtype=np.uint64)
    u8, u32, u64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

    def host(plan, starts_p=starts.ctypes.data_as(u64), amb_p=amb.ctypes.data_as(u8)):
        return L.mm_run_packed_reads_skip_ambiguous_host(plan.h, None, packed.ctypes.data_as(u8), amb_p, 2, starts_p, 50,
                                                         pos.ctypes.data_as(u32), 100, offs.ctypes.data_as(u64), C.byref(cnt))

    assert host(forward) == E["HASHER_NOT_CANONICAL"]
    assert host(text) == E["BAD_MODE"]
    assert host(canon) == E["NULL"]  # (only the workspace is missing)


def test_packer_argument_checks_without_a_device(sm):
    """d_amb: not NULL and 4-byte aligned (MM_ERR_NULL, what a misaligned d_packed gives), amb_capacity_bytes a non-zero
    multiple of 4 (MM_ERR_CAPACITY) - documented in include/simd_minimizers_amd.h."""
    L = sm.lib()
    E = sm.ERR
    fake = C.c_void_p(0x1000)
    out = (C.c_uint64 * 2)()

    def pack(fn, amb, cap, *tail):
        return fn(None, fake, 100, fake, 64, amb, cap, fake, fake, 4, fake, *tail)

    for fn, tail in ((L.mm_fasta_pack_n_device_async, ()), (L.mm_fastq_pack_n_device_async, ()),
                     (L.mm_fasta_pack_n_device, (out,))):
        assert pack(fn, None, 64, *tail) == E["NULL"]
        for misaligned in (0x1001, 0x1002, 0x1003):
            assert pack(fn, C.c_void_p(misaligned), 64, *tail) == E["NULL"]
        for bad in (0, 1, 3, 6, 63):
            assert pack(fn, fake, bad, *tail) == E["CAPACITY"], bad  # (too small for one dword, or no whole dwords)
        assert pack(fn, fake, 64, *tail) == E["NULL"]  # (well-formed: only the workspace is missing)
    # the plain packers take the arguments they took
    assert L.mm_fasta_pack_device_async(None, fake, 100, fake, 64, fake, fake, 4, fake) == E["NULL"]
