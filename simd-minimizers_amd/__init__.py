"""simd_minimizers_amd — Python harness over the C ABI of the MI355X minimizer engine.

The product is the HIP library ``libsimd_minimizers_amd.so`` (``csrc/``, C ABI in
``include/simd_minimizers_amd.h``).  This module is the thin host-side mirror of the
reference's builder API (rust-seq/simd-minimizers ``src/lib.rs:225-654``): same constructor
names, same argument meaning, same error conditions (the reference's ``assert!``s surface as
``MinimizerError``).  It never computes on the CPU: without the HIP library or without a GPU
every ``run`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MM_LIB_PATH: tests/test_sanitizers.py loads the build whose HOST objects carry AddressSanitizer + UBSan)
LIB_PATH = os.environ.get("MM_LIB_PATH") or os.path.join(_HERE, "libsimd_minimizers_amd.so")

MM_MINIMIZERS, MM_CLOSED_SYNCMERS, MM_OPEN_SYNCMERS = 0, 1, 2
PATH_FUSED, PATH_GENERIC, PATH_SPLIT = 1, 2, 3
U64_MAX = (1 << 64) - 1

ERR = {
    "W_ZERO": -1, "W_TOO_LARGE": -2, "LEN_TOO_LARGE": -3, "EVEN_L": -4,
    "HASHER_NOT_CANONICAL": -5, "OPEN_EVEN_W": -6, "K_ZERO": -7, "CAPACITY": -8, "BAD_MODE": -9,
    "NULL": -10, "VALUE_LEN": -11, "FORMAT": -12, "NO_DEVICE": -20, "HIP": -21, "ALLOC": -22, "ORDER": -23,
    "UNSORTED": -24,
}


class MinimizerError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class Hasher(C.Structure):
    """seq-hash NtHasher tables (see include/simd_minimizers_amd.h: mm_hasher_t)."""
    _fields_ = [("fw", C.c_uint32 * 4), ("rc", C.c_uint32 * 4), ("rot", C.c_uint32),
                ("canonical", C.c_uint32), ("fw_xor", C.c_uint32), ("rc_xor", C.c_uint32), ("kind", C.c_uint32)]

    @staticmethod
    def from_tables(fw, rc, rot=7, canonical=True, fw_xor=0, rc_xor=0) -> "Hasher":
        h = Hasher()
        for i in range(4):
            h.fw[i] = int(fw[i]) & 0xFFFFFFFF
            h.rc[i] = int(rc[i]) & 0xFFFFFFFF
        h.rot = rot
        h.canonical = 1 if canonical else 0
        h.fw_xor, h.rc_xor = int(fw_xor) & 0xFFFFFFFF, int(rc_xor) & 0xFFFFFFFF
        h.kind = 0
        return h

    def is_canonical(self) -> bool:
        return bool(self.canonical)


class TextHasher(C.Structure):
    """The hasher of general byte text: ``Hasher``'s rolling form with 256-entry tables indexed by the byte
    (see include/simd_minimizers_amd.h: mm_text_hasher_t)."""
    _fields_ = [("fw", C.c_uint32 * 256), ("rc", C.c_uint32 * 256), ("rot", C.c_uint32),
                ("canonical", C.c_uint32), ("fw_xor", C.c_uint32), ("rc_xor", C.c_uint32), ("kind", C.c_uint32)]

    @staticmethod
    def from_tables(fw, rc, rot=7, canonical=True, fw_xor=0, rc_xor=0) -> "TextHasher":
        h = TextHasher()
        for i in range(256):
            h.fw[i] = int(fw[i]) & 0xFFFFFFFF
            h.rc[i] = int(rc[i]) & 0xFFFFFFFF
        h.rot = rot
        h.canonical = 1 if canonical else 0
        h.fw_xor, h.rc_xor = int(fw_xor) & 0xFFFFFFFF, int(rc_xor) & 0xFFFFFFFF
        h.kind = 0
        return h

    @staticmethod
    def from_dna(hasher: "Hasher") -> "TextHasher":
        """A 4-symbol hasher over ASCII DNA: fw[c] = hasher.fw[(c >> 1) & 3] (mm_text_hasher_from_dna)."""
        h = TextHasher()
        _check(lib().mm_text_hasher_from_dna(C.byref(h), C.byref(hasher)))
        return h

    def is_canonical(self) -> bool:
        return bool(self.canonical)


_TEXT_TYPES = (bytes, bytearray, memoryview)


class PrepareReport(C.Structure):
    """``mm_prepare_report_t``."""
    _fields_ = [("kernels", C.c_uint32), ("compiled", C.c_uint32), ("from_disk", C.c_uint32),
                ("unavailable", C.c_uint32)]


PREPARE_SEQUENCE, PREPARE_READS, PREPARE_SUPERKMERS = 1, 2, 4
# which reference Seq a byte text stands for when its k-mer values are asked (MM_TEXT_VALUES_*): ``&[u8]`` at 8 bits per
# character, or packed-seq ``AsciiSeq`` at 2
TEXT_VALUES_BYTES, TEXT_VALUES_DNA = 0, 1


def _is_text(seq) -> bool:
    """``&[u8]`` input: bytes, bytearray or a uint8 numpy array (one character per byte, all 256 values legal)."""
    return isinstance(seq, _TEXT_TYPES) or (isinstance(seq, np.ndarray) and seq.dtype == np.uint8)


def _text_array(seq) -> np.ndarray:
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq.reshape(-1))
    return np.frombuffer(bytes(seq), dtype=np.uint8)


_lib = None
_lib_lock = threading.Lock()


def lib():
    """Load the HIP library; fail loudly if it has not been built.  Threads racing on the first call load and bind
    it once."""
    if _lib is not None:
        return _lib
    with _lib_lock:
        return _load_lib()


def _load_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:
            # PyTorch-ROCm bundles its own libamdhip64.so.7; load it first so that the engine and
            # torch share ONE HIP runtime (same SONAME) whatever the import order.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        u8p, u32p, u64p, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p
        L.mm_strerror.restype = C.c_char_p
        L.mm_strerror.argtypes = [C.c_int]
        L.mm_last_error.restype = C.c_char_p
        L.mm_device_count.restype = C.c_int
        L.mm_default_hasher.argtypes = [C.POINTER(Hasher), C.c_int]
        L.mm_mul_hasher.argtypes = [C.POINTER(Hasher), C.c_int]
        L.mm_antilex_hasher.argtypes = [C.POINTER(Hasher), C.c_uint32, C.c_int]
        L.mm_plan_create.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                     C.POINTER(Hasher)]
        L.mm_plan_destroy.argtypes = [vp]
        L.mm_plan_destroy.restype = None
        L.mm_plan_value_len.argtypes = [vp]
        L.mm_plan_value_len.restype = C.c_uint32
        L.mm_workspace_create.argtypes = [C.POINTER(vp), C.c_int, vp]
        L.mm_workspace_destroy.argtypes = [vp]
        L.mm_workspace_destroy.restype = None
        L.mm_workspace_sync.argtypes = [vp]
        L.mm_workspace_check.argtypes = [vp]
        L.mm_device_group_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
        L.mm_device_group_destroy.argtypes = [vp]
        L.mm_device_group_destroy.restype = None
        L.mm_device_group_size.argtypes = [vp]
        L.mm_run_sharded_host.argtypes = [vp, vp, u8p, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint64, u64p]
        L.mm_run_batch_sharded_host.argtypes = [vp, vp, C.c_uint64, C.POINTER(u8p), u64p, u64p, u32p, u32p, C.c_uint64, u64p]
        if hasattr(L, "mm_run_sharded_device"):  # (absent from the round-3 library kept for A/B runs under tools/ab/)
            L.mm_device_group_upload.argtypes = [vp, u8p, C.c_uint64]
            if hasattr(L, "mm_device_group_upload_range"):
                L.mm_device_group_upload_range.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint64]
            L.mm_device_group_adopt.argtypes = [vp, C.POINTER(vp), C.c_uint64]
            L.mm_run_sharded_device.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, u64p, u64p]
            L.mm_device_group_result.argtypes = [vp, C.c_int, C.POINTER(u32p), C.POINTER(u32p), u64p, u64p, u64p]
            L.mm_device_group_gather.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, u64p]
            L.mm_device_group_upload_batch.argtypes = [vp, C.c_uint64, C.POINTER(u8p), u64p]
            L.mm_run_batch_sharded_device.argtypes = [vp, vp, u64p, u64p, C.c_int, u64p, u64p]
            L.mm_device_group_batch_result.argtypes = [vp, C.c_uint64, C.POINTER(C.c_int), C.POINTER(u32p), C.POINTER(u32p), u64p]
            L.mm_device_group_gather_batch.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, u64p]
            L.mm_run_packed_reads_device_async.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                                           C.c_uint32, vp, vp, C.c_uint64, vp, vp]
            L.mm_run_packed_reads_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                                     C.c_uint32, vp, vp, C.c_uint64, vp, u64p]
            L.mm_run_packed_reads_host.argtypes = [vp, vp, u8p, C.c_uint64, u64p, C.c_uint32, u32p, u32p, C.c_uint64, u64p, u64p]
            L.mm_debug_launch_plan.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint64, u64p, u64p, u32p, u32p, u32p,
                                               C.c_uint64, u64p]
        L.mm_clock_probe_begin.argtypes = [vp, C.c_uint64]
        L.mm_clock_probe_end.argtypes = [vp, C.POINTER(C.c_double)]
        L.mm_link_probe.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_double)]
        L.mm_debug_launch_lds.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint64, u64p]
        L.mm_debug_fixed_k_kernel.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        if hasattr(L, "mm_debug_kc_count"):  # (absent from older libraries loaded through MM_LIB_PATH for A/B runs)
            L.mm_debug_kc_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u8p, C.c_uint64,
                                            C.c_int64, u32p]
            L.mm_debug_kc_count.restype = C.c_int
        if hasattr(L, "mm_debug_pair_table"):  # (absent from older libraries loaded through MM_LIB_PATH for A/B runs)
            L.mm_debug_pair_table.argtypes = [C.POINTER(Hasher), u32p]
            L.mm_debug_pair_table.restype = C.c_int
        if hasattr(L, "mm_debug_walk_traits"):  # (absent from older libraries loaded through MM_LIB_PATH for A/B runs)
            L.mm_debug_walk_traits.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u32p, C.c_int]
            L.mm_debug_walk_traits.restype = C.c_int
        L.mm_debug_lane_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, u64p]
        L.mm_debug_last_lane_table.argtypes = [vp, u32p, C.c_uint64, u64p]
        L.mm_fused_overread_bytes.argtypes = []
        L.mm_fused_overread_bytes.restype = C.c_uint64
        L.mm_workspace_force_generic.argtypes = [vp, C.c_int]
        L.mm_workspace_set_blocks_per_lane.argtypes = [vp, C.c_uint32]
        L.mm_workspace_enable_timing.argtypes = [vp, C.c_int]
        L.mm_workspace_kernel_time.argtypes = [vp, C.POINTER(C.c_double), u64p, C.c_int]
        L.mm_workspace_last_path.argtypes = [vp]
        L.mm_workspace_ticket_mode.argtypes = [vp]
        L.mm_workspace_last_lane_table.argtypes = [vp]
        if hasattr(L, "mm_prebuilt_window_sizes"):  # (absent from the round-3 library kept for A/B runs under tools/ab/)
            L.mm_prebuilt_window_sizes.argtypes = [C.c_int, C.c_int, u32p, C.c_int]
            L.mm_prebuilt_window_sizes.restype = C.c_int
        if hasattr(L, "mm_plan_prepare"):  # (absent from older libraries loaded through MM_LIB_PATH for A/B runs)
            L.mm_prebuilt_flavour_window_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, C.c_int]
            L.mm_prebuilt_flavour_window_sizes.restype = C.c_int
            L.mm_plan_prepare.argtypes = [vp, vp, C.c_uint32, C.POINTER(PrepareReport)]
            L.mm_jit_stats.argtypes = [u64p]
        L.mm_run_device_async.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                          C.c_uint64, vp, vp, C.c_uint64, vp]
        L.mm_run_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.c_uint64, vp, vp, C.c_uint64, u64p]
        L.mm_run_host.argtypes = [vp, vp, u8p, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint64, u64p]
        L.mm_run_host_ascii.argtypes = [vp, vp, u8p, C.c_uint64, u32p, u32p, C.c_uint64, u64p]
        if hasattr(L, "mm_plan_create_text"):
            L.mm_text_mul_hasher.argtypes = [C.POINTER(TextHasher), C.c_int]
            L.mm_text_hasher_from_dna.argtypes = [C.POINTER(TextHasher), C.POINTER(Hasher)]
            L.mm_plan_create_text.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                              C.POINTER(TextHasher)]
            text_args = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64]
            L.mm_run_text_device_async.argtypes = text_args + [vp]
            L.mm_run_text_device.argtypes = text_args + [u64p]
            L.mm_run_text_host.argtypes = [vp, vp, u8p, C.c_uint64, u32p, u32p, C.c_uint64, u64p]
            L.mm_text_prebuilt_window_sizes.argtypes = [C.c_int, u32p, C.c_int]
            batch_args = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp]
            L.mm_run_text_batch_device_async.argtypes = batch_args + [vp]
            L.mm_run_text_batch_device.argtypes = batch_args + [u64p]
            L.mm_run_text_batch_host.argtypes = [vp, vp, u8p, C.c_uint64, u64p, u32p, u32p, C.c_uint64, u64p, u64p]
        L.mm_values_u64_device_async.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                                 C.c_uint32, C.c_int, vp, C.c_uint64, vp]
        L.mm_values_u64_host.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, u32p,
                                         C.c_uint64, u64p]
        L.mm_values_u128_device_async.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                                                  C.c_uint32, C.c_int, vp, C.c_uint64, vp]
        L.mm_values_u128_host.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, u32p,
                                          C.c_uint64, u64p]
        values_reads_args = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp,
                             C.c_uint64, vp]
        L.mm_values_u64_reads_device_async.argtypes = values_reads_args
        L.mm_values_u128_reads_device_async.argtypes = values_reads_args
        values_reads_host_args = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.c_uint32, C.c_uint32, C.c_int,
                                  u32p, u64p, u64p]
        L.mm_values_u64_reads_host.argtypes = values_reads_host_args
        L.mm_values_u128_reads_host.argtypes = values_reads_host_args
        L.mm_debug_values_read_of.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64, C.POINTER(C.c_int64)]
        L.mm_values_reads_lds_stage.argtypes = []
        L.mm_values_reads_lds_stage.restype = C.c_uint32
        one_min_reads_tail = [C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32]
        L.mm_one_minimizer_reads_device_async.argtypes = [vp, vp, C.c_uint32, vp] + one_min_reads_tail + [vp]
        L.mm_one_minimizer_reads_host.argtypes = [vp, vp, C.c_uint32, vp] + one_min_reads_tail + [vp]
        L.mm_debug_one_minimizer_reads.argtypes = [vp, C.c_uint32, vp] + one_min_reads_tail + [C.c_uint32, vp]
        one_min_text_tail = [C.c_uint64, C.c_uint64, vp]
        L.mm_one_minimizer_text_batch_device_async.argtypes = [vp, vp, C.c_uint32, vp] + one_min_text_tail + [vp]
        L.mm_one_minimizer_text_batch_host.argtypes = [vp, vp, C.c_uint32, vp] + one_min_text_tail + [vp]
        L.mm_debug_one_minimizer_text_batch.argtypes = [vp, C.c_uint32, vp] + one_min_text_tail + [C.c_uint32, vp]
        # (the counts forms: bounds in place of the counts, d_counts behind the starts)
        L.mm_one_minimizer_text_batch_counts_device_async.argtypes = [vp, vp, C.c_uint32, vp] + [C.c_uint64] * 3 + [vp, vp, vp]
        L.mm_one_minimizer_reads_counts_device_async.argtypes = [vp, vp, C.c_uint32, vp] + [C.c_uint64] * 4 + [vp, vp, vp]
        L.mm_debug_one_minimizer_counts_view.argtypes = [C.c_uint64] * 4 + [vp, vp]
        L.mm_debug_one_minimizer_text_batch_counts.argtypes = [vp, C.c_uint32, vp] + [C.c_uint64] * 3 + [vp, vp, C.c_uint32, vp]
        L.mm_debug_one_minimizer_reads_counts.argtypes = [vp, C.c_uint32, vp] + [C.c_uint64] * 4 + [vp, vp, C.c_uint32, vp]
        amb3 = [vp, C.c_uint64, C.c_uint64]  # (the skip-ambiguous forms: d_amb, amb_bytes, amb_offset)
        L.mm_one_minimizer_reads_skip_ambiguous_device_async.argtypes = (
            [vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64] + amb3 + [C.c_uint64, vp, C.c_uint32, C.c_uint32, vp])
        L.mm_one_minimizer_reads_skip_ambiguous_host.argtypes = (
            [vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64] + amb3 + [C.c_uint64, vp, C.c_uint32, C.c_uint32, vp])
        L.mm_one_minimizer_reads_skip_ambiguous_counts_device_async.argtypes = (
            [vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64] + amb3 + [C.c_uint64, C.c_uint64, vp, vp, vp])
        L.mm_debug_one_minimizer_reads_skip_ambiguous.argtypes = (
            [vp, C.c_uint32, vp, C.c_uint64, C.c_uint64] + amb3 + [C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp])
        L.mm_debug_one_minimizer_reads_skip_ambiguous_counts.argtypes = (
            [vp, C.c_uint32, vp, C.c_uint64, C.c_uint64] + amb3 + [C.c_uint64, C.c_uint64, vp, vp, C.c_uint32, vp])
        L.mm_fastx_stream_one_minimizer.argtypes = [vp, C.POINTER(vp), u64p]
        L.mm_one_minimizer_tile.argtypes = []
        L.mm_one_minimizer_tile.restype = C.c_uint32
        values_batch_args = [vp, C.c_uint64, C.POINTER(vp), u64p, u64p, u64p, C.c_uint32, C.c_int, vp, u64p, vp]
        L.mm_values_u64_batch_device_async.argtypes = values_batch_args
        L.mm_values_u128_batch_device_async.argtypes = values_batch_args
        L.mm_values_batch_lds_stage.argtypes = []
        L.mm_values_batch_lds_stage.restype = C.c_uint32
        L.mm_debug_values_batch_view.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p]
        L.mm_device_group_values_batch.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, u64p]
        L.mm_device_group_batch_values.argtypes = [vp, C.c_uint64, C.POINTER(C.c_int), C.POINTER(u64p), u64p]
        values_text_args = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_int, vp, C.c_uint64, vp]
        L.mm_values_u64_text_device_async.argtypes = values_text_args
        L.mm_values_u128_text_device_async.argtypes = values_text_args
        values_text_host_args = [vp, u8p, C.c_uint64, C.c_int, C.c_uint32, C.c_int, u32p, C.c_uint64, u64p]
        L.mm_values_u64_text_host.argtypes = values_text_host_args
        L.mm_values_u128_text_host.argtypes = values_text_host_args
        values_text_batch_args = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_uint32, C.c_int, vp, vp,
                                  C.c_uint64, vp]
        L.mm_values_u64_text_batch_device_async.argtypes = values_text_batch_args
        L.mm_values_u128_text_batch_device_async.argtypes = values_text_batch_args
        values_text_batch_host_args = [vp, u8p, C.c_uint64, u64p, C.c_int, C.c_uint32, C.c_int, u32p, u64p, u64p]
        L.mm_values_u64_text_batch_host.argtypes = values_text_batch_host_args
        L.mm_values_u128_text_batch_host.argtypes = values_text_batch_host_args
        L.mm_values_text_lds_stage.argtypes = []
        L.mm_values_text_lds_stage.restype = C.c_uint32
        L.mm_debug_values_text.argtypes = [vp, C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.c_int, u64p, C.c_uint64, u64p]
        L.mm_run_batch_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp), u64p, u64p, u64p, vp, vp,
                                          C.c_uint64, u64p]
        reads_args = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp,
                      C.c_uint64, vp]
        L.mm_run_reads_device_async.argtypes = reads_args + [vp]
        L.mm_run_reads_device.argtypes = reads_args + [u64p]
        reads_sk_args = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp,
                         C.c_uint64, vp]
        L.mm_run_reads_superkmers_device_async.argtypes = reads_sk_args + [vp]
        L.mm_run_reads_superkmers_device.argtypes = reads_sk_args + [u64p]
        skip_args = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                     C.c_uint64, C.c_uint64, vp, C.c_uint64]
        L.mm_run_skip_ambiguous_device_async.argtypes = skip_args + [vp]
        L.mm_run_skip_ambiguous_device.argtypes = skip_args + [u64p]
        L.mm_run_skip_ambiguous_host.argtypes = [vp, vp, u8p, C.c_uint64, u8p, C.c_uint64, C.c_uint64, u32p,
                                                 C.c_uint64, u64p]
        L.mm_run_skip_ambiguous_host_ascii.argtypes = [vp, vp, u8p, C.c_uint64, u32p, C.c_uint64, u64p]
        reads_skip_args = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64,
                           C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp]
        L.mm_run_reads_skip_ambiguous_device_async.argtypes = reads_skip_args + [vp]
        L.mm_run_reads_skip_ambiguous_device.argtypes = reads_skip_args + [u64p]
        L.mm_pack_ascii_n_device_async.argtypes = [vp, vp, C.c_uint64, vp, vp]
        L.mm_host_alloc.argtypes = [C.POINTER(vp), C.c_uint64]
        L.mm_host_free.argtypes = [vp]
        L.mm_host_free.restype = None
        L.mm_pack_ascii_device_async.argtypes = [vp, vp, C.c_uint64, vp]
        L.mm_generate_device_async.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
        fasta_args = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp]
        L.mm_fasta_pack_device_async.argtypes = fasta_args
        L.mm_fasta_pack_device.argtypes = fasta_args + [u64p]
        if hasattr(L, "mm_fastq_pack_device_async"):
            L.mm_fastq_pack_device_async.argtypes = fasta_args
        if hasattr(L, "mm_fasta_pack_n_device"):  # (FASTA / FASTQ with N: ambiguity bits from the packers, skipped windows)
            fasta_n_args = fasta_args[:5] + [vp, C.c_uint64] + fasta_args[5:]
            L.mm_fasta_pack_n_device_async.argtypes = fasta_n_args
            L.mm_fastq_pack_n_device_async.argtypes = fasta_n_args
            L.mm_fasta_pack_n_device.argtypes = fasta_n_args + [u64p]
            packed_skip_args = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                C.c_uint32, vp, C.c_uint64, vp]
            L.mm_run_packed_reads_skip_ambiguous_device_async.argtypes = packed_skip_args + [vp]
            L.mm_run_packed_reads_skip_ambiguous_device.argtypes = packed_skip_args + [u64p]
            L.mm_run_packed_reads_skip_ambiguous_host.argtypes = [vp, vp, u8p, u8p, C.c_uint64, u64p, C.c_uint32, u32p,
                                                                  C.c_uint64, u64p, u64p]
        if hasattr(L, "mm_fasta_text_device"):  # (FASTA -> records of byte text)
            L.mm_fasta_text_device_async.argtypes = fasta_args
            L.mm_fasta_text_device.argtypes = fasta_args + [u64p]
            L.mm_debug_compact32.argtypes = [u8p, C.c_uint32, u8p]
        if hasattr(L, "mm_run_text_batch_counts_device"):  # (text batch run and values with their counts on the device)
            counts_args = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp]
            L.mm_run_text_batch_counts_device_async.argtypes = counts_args + [vp]
            L.mm_run_text_batch_counts_device.argtypes = counts_args + [u64p]
            values_counts_args = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, C.c_int, C.c_uint32, C.c_int, vp, vp,
                                  C.c_uint64, vp]
            L.mm_values_u64_text_batch_counts_device_async.argtypes = values_counts_args
            L.mm_values_u128_text_batch_counts_device_async.argtypes = values_counts_args
            L.mm_debug_text_counts_view.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                                    u64p]
        if hasattr(L, "mm_run_packed_reads_counts_device"):  # (packed reads run with its counts on the device)
            rc_args = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp]
            L.mm_run_packed_reads_counts_device_async.argtypes = rc_args + [vp]
            L.mm_run_packed_reads_counts_device.argtypes = rc_args + [u64p]
            rc_skip_args = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp,
                            C.c_uint64, vp]
            L.mm_run_packed_reads_skip_ambiguous_counts_device_async.argtypes = rc_skip_args + [vp]
            L.mm_run_packed_reads_skip_ambiguous_counts_device.argtypes = rc_skip_args + [u64p]
            L.mm_debug_lane_counts_view.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
        if hasattr(L, "mm_fastx_stream_create"):  # (FASTA / FASTQ files of any size through the device in chunks)
            L.mm_fastx_stream_create.argtypes = [C.POINTER(vp), vp, vp]
            L.mm_fastx_stream_feed.argtypes = [vp, vp, C.c_uint64, u64p]
            L.mm_fastx_stream_finish.argtypes = [vp]
            L.mm_fastx_stream_next.argtypes = [vp, vp]
            L.mm_fastx_stream_destroy.argtypes = [vp]
            L.mm_fastx_stream_destroy.restype = None
            L.mm_debug_fastx_cut.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, u64p]
        L.mm_fastx_text_stream_create.argtypes = [C.POINTER(vp), vp, vp]
        L.mm_fastx_text_stream_extras.argtypes = [vp, vp]
        if hasattr(L, "mm_fastx_stream_pieces"):  # (FASTA records longer than a chunk: MM_FASTX_LONG_RECORDS)
            L.mm_fastx_stream_pieces.argtypes = [vp, vp]
            L.mm_debug_fastx_split.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_int, u64p]
        if hasattr(L, "mm_bgzf_scan_host"):  # (BGZF-compressed input, inflated on the device)
            L.mm_bgzf_scan_host.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, u64p, u64p, u64p]
            L.mm_bgzf_inflate_device_async.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.mm_bgzf_inflate_host.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p]
            L.mm_debug_bgzf_inflate.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
            L.mm_fastx_stream_feed_bgzf.argtypes = [vp, vp, C.c_uint64, u64p]
        if hasattr(L, "mm_bgzf_crc32_device_async"):  # (the blocks' CRC32, verified on the device on request)
            L.mm_debug_crc32.argtypes = [vp, C.c_uint64, vp]
            L.mm_bgzf_scan_crc_host.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, u64p, u64p, u64p, vp]
            L.mm_bgzf_crc32_device_async.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
            L.mm_bgzf_inflate_verify_host.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p]
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "mm_strerror", "mm_last_error", "mm_device_count", "mm_default_hasher", "mm_mul_hasher", "mm_antilex_hasher",
    "mm_plan_create",
    "mm_plan_destroy", "mm_plan_value_len", "mm_workspace_create", "mm_workspace_destroy",
    "mm_workspace_sync", "mm_workspace_check", "mm_workspace_force_generic", "mm_workspace_set_blocks_per_lane",
    "mm_workspace_enable_timing", "mm_workspace_kernel_time", "mm_workspace_last_path", "mm_workspace_ticket_mode",
    "mm_workspace_last_lane_table", "mm_prebuilt_window_sizes",
    "mm_run_device_async", "mm_run_device", "mm_run_host", "mm_run_host_ascii",
    "mm_values_u64_device_async", "mm_values_u64_host", "mm_values_u128_device_async",
    "mm_values_u128_host", "mm_run_batch_device", "mm_run_reads_device_async", "mm_run_reads_device",
    "mm_run_reads_superkmers_device_async", "mm_run_reads_superkmers_device",
    "mm_run_skip_ambiguous_device_async", "mm_run_skip_ambiguous_device", "mm_run_skip_ambiguous_host",
    "mm_run_skip_ambiguous_host_ascii", "mm_run_reads_skip_ambiguous_device_async",
    "mm_run_reads_skip_ambiguous_device", "mm_pack_ascii_n_device_async", "mm_pack_ascii_device_async",
    "mm_host_alloc", "mm_host_free",
    "mm_generate_device_async", "mm_fasta_pack_device_async", "mm_fasta_pack_device", "mm_fastq_pack_device_async",
    "mm_clock_probe_begin", "mm_clock_probe_end", "mm_link_probe", "mm_fused_overread_bytes",
    "mm_device_group_create", "mm_device_group_destroy", "mm_device_group_size", "mm_run_sharded_host",
    "mm_run_batch_sharded_host",
    "mm_device_group_upload", "mm_device_group_upload_range", "mm_device_group_adopt", "mm_run_sharded_device", "mm_device_group_result",
    "mm_device_group_gather",
    "mm_device_group_upload_batch", "mm_run_batch_sharded_device", "mm_device_group_batch_result",
    "mm_device_group_gather_batch", "mm_debug_launch_plan", "mm_debug_launch_lds", "mm_debug_lane_plan", "mm_debug_fixed_k_kernel",
    "mm_debug_last_lane_table",
    "mm_run_packed_reads_device_async", "mm_run_packed_reads_device", "mm_run_packed_reads_host",
    "mm_text_mul_hasher", "mm_text_hasher_from_dna", "mm_plan_create_text", "mm_run_text_device_async",
    "mm_run_text_device", "mm_run_text_host", "mm_text_prebuilt_window_sizes",
    "mm_run_text_batch_device_async", "mm_run_text_batch_device", "mm_run_text_batch_host",
    "mm_fasta_pack_n_device_async", "mm_fastq_pack_n_device_async", "mm_fasta_pack_n_device",
    "mm_run_packed_reads_skip_ambiguous_device_async", "mm_run_packed_reads_skip_ambiguous_device",
    "mm_run_packed_reads_skip_ambiguous_host",
    "mm_values_u64_reads_device_async", "mm_values_u128_reads_device_async", "mm_values_u64_reads_host",
    "mm_values_u128_reads_host", "mm_debug_values_read_of", "mm_values_reads_lds_stage",
    "mm_values_u64_batch_device_async", "mm_values_u128_batch_device_async", "mm_values_batch_lds_stage",
    "mm_debug_values_batch_view", "mm_device_group_values_batch", "mm_device_group_batch_values",
    "mm_prebuilt_flavour_window_sizes", "mm_plan_prepare", "mm_jit_stats",
    "mm_values_u64_text_device_async", "mm_values_u128_text_device_async", "mm_values_u64_text_host",
    "mm_values_u128_text_host", "mm_values_u64_text_batch_device_async", "mm_values_u128_text_batch_device_async",
    "mm_values_u64_text_batch_host", "mm_values_u128_text_batch_host", "mm_values_text_lds_stage", "mm_debug_values_text",
    "mm_fasta_text_device_async", "mm_fasta_text_device", "mm_debug_compact32",
    "mm_run_text_batch_counts_device_async", "mm_run_text_batch_counts_device",
    "mm_values_u64_text_batch_counts_device_async", "mm_values_u128_text_batch_counts_device_async",
    "mm_debug_text_counts_view",
    "mm_run_packed_reads_counts_device_async", "mm_run_packed_reads_counts_device",
    "mm_run_packed_reads_skip_ambiguous_counts_device_async", "mm_run_packed_reads_skip_ambiguous_counts_device",
    "mm_debug_lane_counts_view",
    "mm_fastx_stream_create", "mm_fastx_stream_feed", "mm_fastx_stream_finish", "mm_fastx_stream_next",
    "mm_fastx_stream_destroy", "mm_debug_fastx_cut", "mm_fastx_stream_pieces", "mm_debug_fastx_split",
    "mm_one_minimizer_reads_device_async", "mm_one_minimizer_text_batch_device_async", "mm_one_minimizer_reads_host",
    "mm_one_minimizer_text_batch_host", "mm_one_minimizer_tile", "mm_debug_one_minimizer_reads",
    "mm_debug_one_minimizer_text_batch",
    "mm_one_minimizer_text_batch_counts_device_async", "mm_one_minimizer_reads_counts_device_async",
    "mm_debug_one_minimizer_counts_view", "mm_debug_one_minimizer_text_batch_counts", "mm_debug_one_minimizer_reads_counts",
    "mm_fastx_text_stream_create", "mm_fastx_text_stream_extras",
    "mm_one_minimizer_reads_skip_ambiguous_device_async", "mm_one_minimizer_reads_skip_ambiguous_counts_device_async",
    "mm_one_minimizer_reads_skip_ambiguous_host", "mm_debug_one_minimizer_reads_skip_ambiguous",
    "mm_debug_one_minimizer_reads_skip_ambiguous_counts", "mm_fastx_stream_one_minimizer",
    "mm_debug_walk_traits", "mm_debug_kc_count", "mm_debug_pair_table",
    "mm_bgzf_scan_host", "mm_bgzf_inflate_device_async", "mm_bgzf_inflate_host", "mm_debug_bgzf_inflate",
    "mm_fastx_stream_feed_bgzf",
    "mm_debug_crc32", "mm_bgzf_scan_crc_host", "mm_bgzf_crc32_device_async", "mm_bgzf_inflate_verify_host",
]

# the order of mm_debug_walk_traits' values (MM_TRAIT_* of the header)
WALK_TRAITS = ("wide_group_blocks", "wide_dwords", "v2_load", "view_words", "amb_view_words", "sk_shift", "ambi_land",
               "ambi_rows", "amb_row_dwords", "lazy_vote", "table_prefetch", "two_bodies", "entry8", "one_stream",
               "last_view_bases")


def walk_traits(w: int, canonical: bool, mode: int = 0, super_kmers: bool = False, reads: bool = False,
                ambiguous: bool = False) -> dict:
    """What the fused kernel's walk decides at compile time from its window size, for one flavour (mm_debug_walk_traits;
    no device): a dict keyed by WALK_TRAITS."""
    L = lib()
    n = L.mm_debug_walk_traits(int(w), int(canonical), int(mode), int(super_kmers), int(reads), int(ambiguous), None, 0)
    if n != len(WALK_TRAITS):
        raise RuntimeError(f"mm_debug_walk_traits lists {n} values, this package knows {len(WALK_TRAITS)}")
    buf = (C.c_uint32 * n)()
    L.mm_debug_walk_traits(int(w), int(canonical), int(mode), int(super_kmers), int(reads), int(ambiguous), buf, n)
    return dict(zip(WALK_TRAITS, (int(x) for x in buf)))


def prebuilt_window_sizes(canonical: bool, reads: bool = False) -> list:
    """Window sizes with a prebuilt fused kernel (mm_prebuilt_window_sizes): what the tests sweep."""
    L = lib()
    n = L.mm_prebuilt_window_sizes(int(canonical), int(reads), None, 0)
    buf = (C.c_uint32 * max(1, n))()
    L.mm_prebuilt_window_sizes(int(canonical), int(reads), buf, n)
    return [int(x) for x in buf[:n]]


def prebuilt_flavour_window_sizes(canonical: bool, reads: bool = False, mode: int = 0, super_kmers: bool = False) -> list:
    """Window sizes with a prebuilt fused kernel of one flavour (mm_prebuilt_flavour_window_sizes): ``mode`` is
    MM_MINIMIZERS / MM_CLOSED_SYNCMERS / MM_OPEN_SYNCMERS, ``super_kmers`` minimizers with super-k-mer indices."""
    L = lib()
    n = L.mm_prebuilt_flavour_window_sizes(int(canonical), int(reads), int(mode), int(super_kmers), None, 0)
    buf = (C.c_uint32 * max(1, n))()
    L.mm_prebuilt_flavour_window_sizes(int(canonical), int(reads), int(mode), int(super_kmers), buf, n)
    return [int(x) for x in buf[:n]]


def jit_stats() -> dict:
    """Process-wide counters of the run-time compiler (mm_jit_stats); nothing resets them, take differences."""
    out = (C.c_uint64 * 4)()
    _check(lib().mm_jit_stats(out))
    return {"compiled": int(out[0]), "from_disk": int(out[1]), "hits": int(out[2]), "failed": int(out[3])}


def text_prebuilt_window_sizes(canonical: bool) -> list:
    """Window sizes with a prebuilt fused text instance (mm_text_prebuilt_window_sizes): what the text tests sweep."""
    L = lib()
    n = L.mm_text_prebuilt_window_sizes(int(canonical), None, 0)
    buf = (C.c_uint32 * max(1, n))()
    L.mm_text_prebuilt_window_sizes(int(canonical), buf, n)
    return [int(x) for x in buf[:n]]


def _check(code: int):
    if code != 0:
        L = lib()
        msg = L.mm_strerror(code).decode()
        if code in (ERR["HIP"], ERR["ALLOC"], ERR["NO_DEVICE"], ERR["ORDER"]):
            msg += ": " + L.mm_last_error().decode()
        raise MinimizerError(code, msg)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ------------------------------------------------------------------ sequences


class PackedSeq:
    """packed-seq ``PackedSeq``: a borrowed view (bytes, base offset, length)."""

    def __init__(self, data: np.ndarray, offset: int, length: int):
        self.data, self.offset, self.length = data, offset, length

    def __len__(self):
        return self.length

    def slice(self, start: int, end: int) -> "PackedSeq":
        assert 0 <= start <= end <= self.length
        return PackedSeq(self.data, self.offset + start, end - start)

    def as_slice(self) -> "PackedSeq":
        return self

    def codes(self) -> np.ndarray:
        i = np.arange(self.offset, self.offset + self.length, dtype=np.int64)
        return ((self.data[i >> 2] >> (2 * (i & 3)).astype(np.uint8)) & 3).astype(np.uint8)

    def to_revcomp(self) -> "PackedSeqVec":
        return PackedSeqVec.from_codes((self.codes()[::-1] ^ 2).astype(np.uint8))


class PackedSeqVec(PackedSeq):
    """packed-seq ``PackedSeqVec``: owns 2-bit packed bases (A0 C1 T2 G3, 4 per byte)."""

    def __init__(self, data: np.ndarray, length: int):
        super().__init__(data, 0, length)

    @staticmethod
    def from_codes(codes: np.ndarray) -> "PackedSeqVec":
        n = len(codes)
        pad = np.zeros((n + 3) // 4 * 4, dtype=np.uint8)
        pad[:n] = codes
        q = pad.reshape(-1, 4)
        data = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)
        return PackedSeqVec(np.concatenate([data, np.zeros(16, dtype=np.uint8)]), n)

    @staticmethod
    def from_ascii(seq: bytes) -> "PackedSeqVec":
        a = np.frombuffer(bytes(seq), dtype=np.uint8)
        return PackedSeqVec.from_codes(((a >> 1) & 3).astype(np.uint8))

    @staticmethod
    def random(n: int, seed: int = 0) -> "PackedSeqVec":
        rng = np.random.default_rng(seed)
        return PackedSeqVec.from_codes(rng.integers(0, 4, size=n, dtype=np.uint8))


class PackedNSeq:
    """packed-seq ``PackedNSeq``: a PackedSeq view plus one ambiguity bit per base (bit i%8 of byte
    i/8 of ``amb``, with its own bit offset)."""

    def __init__(self, seq: PackedSeq, amb: np.ndarray, amb_offset: int = 0):
        self.seq, self.amb, self.amb_offset = seq, amb, amb_offset

    def __len__(self):
        return len(self.seq)

    def as_slice(self) -> "PackedNSeq":
        return self

    def slice(self, start: int, end: int) -> "PackedNSeq":
        return PackedNSeq(self.seq.slice(start, end), self.amb, self.amb_offset + start)


class PackedNSeqVec(PackedNSeq):
    """packed-seq ``PackedNSeqVec`` (call site src/test.rs:436)."""

    @staticmethod
    def from_ascii(seq: bytes) -> "PackedNSeqVec":
        a = np.frombuffer(bytes(seq), dtype=np.uint8)
        up = a & 0xDF
        isn = ~((up == 65) | (up == 67) | (up == 71) | (up == 84))
        amb = np.concatenate([np.packbits(isn, bitorder="little"), np.zeros(16, dtype=np.uint8)])
        return PackedNSeqVec(PackedSeqVec.from_ascii(seq), amb, 0)


class AsciiSeq:
    """packed-seq ``AsciiSeq``: ACTG/actg characters, mapped with (c >> 1) & 3."""

    def __init__(self, seq: bytes):
        self.seq = bytes(seq)

    def __len__(self):
        return len(self.seq)

    def slice(self, start: int, end: int) -> "AsciiSeq":
        return AsciiSeq(self.seq[start:end])


# ------------------------------------------------------------------ workspace


class Workspace:
    """Device scratch + stream (the reference's thread-local CACHE, src/lib.rs:217-219).  One thread uses a workspace at
    a time (the library holds no lock on it); it may be handed to another thread between calls."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = lib()
        if L.mm_device_count() <= 0:
            raise MinimizerError(ERR["NO_DEVICE"], "no HIP device (this engine has no CPU fallback)")
        h = C.c_void_p()
        _check(L.mm_workspace_create(C.byref(h), device, C.c_void_p(stream)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().mm_workspace_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().mm_workspace_sync(self.h))

    def check(self):
        """Completion status of the asynchronous runs since the last check (mm_workspace_check):
        raises MinimizerError(ORDER) if one of them has to be repeated."""
        _check(lib().mm_workspace_check(self.h))

    def clock_probe_begin(self, duration_us: int):
        """Start sampling the shader clock for ``duration_us`` on a stream of the workspace's own (diagnostics)."""
        _check(lib().mm_clock_probe_begin(self.h, int(duration_us)))

    def clock_probe_end(self) -> float:
        """Mean shader clock in GHz over the sampled span."""
        g = C.c_double()
        _check(lib().mm_clock_probe_end(self.h, C.byref(g)))
        return g.value

    def force_generic(self, on: bool):
        _check(lib().mm_workspace_force_generic(self.h, int(on)))

    def set_blocks_per_lane(self, nblk: int):
        _check(lib().mm_workspace_set_blocks_per_lane(self.h, nblk))

    def enable_timing(self, on: bool):
        _check(lib().mm_workspace_enable_timing(self.h, int(on)))

    def kernel_time(self, reset: bool = True) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        _check(lib().mm_workspace_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def last_path(self) -> int:
        return lib().mm_workspace_last_path(self.h)

    def ticket_mode(self) -> bool:
        """The fused kernels take their tile ids from an atomic ticket on this workspace since a look-back of one of its
        runs timed out (``mm_workspace_ticket_mode``; diagnostics only, results are the same)."""
        return bool(lib().mm_workspace_ticket_mode(self.h))

    def last_lane_table(self) -> bool:
        """The last reads / batch run was ONE lane-table launch (``mm_workspace_last_lane_table``)."""
        return bool(lib().mm_workspace_last_lane_table(self.h))


class DeviceGroup:
    """``mm_device_group_t``: one workspace per listed device (a device may be listed more than once); the
    several-device calls fan one sequence (window ranges, exact seam) or a set of sequences (greedy placement)
    over them - the reference's rayon loop over contigs (bench/src/bin/paper.rs:442-459) behind the C ABI."""

    def __init__(self, devices):
        self.h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().mm_device_group_create(C.byref(self.h), arr, len(devices)))
        self._batch_n = None  # sequences of the resident batch (upload_batch), None: no batch uploaded yet
        self._devices = [int(d) for d in devices]
        self._batch_u128 = False  # the last values_batch() wrote {lo, hi} pairs

    def __len__(self):
        return lib().mm_device_group_size(self.h)

    def close(self):
        if self.h:
            lib().mm_device_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, builder: "Builder", packed: np.ndarray, n_bases: int, base_offset: int = 0, capacity=None, out=None):
        """One host PackedSeq over all entries (``mm_run_sharded_host``): (positions, super-k-mer indices or None).
        ``out``: a caller-owned uint32 array to receive the positions (e.g. page-locked, ``pinned_array``) instead of
        a fresh one per call."""
        plan = builder.plan()
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        l = builder.k + builder.w - 1
        cap = max(1, n_bases - l + 1) if capacity is None else capacity
        if out is not None:
            # (the library writes uint32 positions straight into it)
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.ndim == 1 and out.flags.c_contiguous
                    and out.flags.writeable):
                raise ValueError("out must be a writeable, C-contiguous, one-dimensional uint32 array")
            cap = min(cap, out.size) if capacity is not None else out.size
        pos = out if out is not None else np.empty(cap, dtype=np.uint32)
        sk = np.empty(cap, dtype=np.uint32) if builder._sk is not None else None
        cnt = C.c_uint64()
        code = lib().mm_run_sharded_host(plan.h, self.h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), base_offset, n_bases,
                                         pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         sk.ctypes.data_as(C.POINTER(C.c_uint32)) if sk is not None else None, cap,
                                         C.byref(cnt))
        if code == ERR["CAPACITY"]:
            raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
        _check(code)
        return pos[:cnt.value], (sk[:cnt.value] if sk is not None else None)

    # ---- device-resident shards (mm_device_group_upload / _adopt, mm_run_sharded_device, _result, _gather)
    def upload(self, packed: np.ndarray):
        """The packed sequence to every device of the group, once (kept until the next upload / adopt)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        _check(lib().mm_device_group_upload(self.h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), packed.size))

    def upload_range(self, packed: np.ndarray, n_bases: int, base_offset: int = 0):
        """``mm_device_group_upload_range``: every entry receives only the bytes its share of an N-way split of
        (base_offset, n_bases) reads (+ a halo): the sequence crosses the host link once in total."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        _check(lib().mm_device_group_upload_range(self.h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), packed.size,
                                                  base_offset, n_bases))

    def adopt(self, device_tensors):
        """Device buffers the caller already holds (one per entry, on that entry's device, same bytes)."""
        self._adopted = list(device_tensors)  # keep them alive
        ptrs = (C.c_void_p * len(self._adopted))(*[t.data_ptr() for t in self._adopted])
        _check(lib().mm_device_group_adopt(self.h, ptrs, int(self._adopted[0].numel())))

    def run_device(self, builder: "Builder", n_bases: int, base_offset: int = 0):
        """``mm_run_sharded_device``: one asynchronous launch per entry over its window range of the resident
        sequence; the positions stay on the devices.  Returns the per-entry counts."""
        n = len(self)
        counts = (C.c_uint64 * n)()
        total = C.c_uint64()
        code = lib().mm_run_sharded_device(builder.plan().h, self.h, base_offset, n_bases,
                                           1 if builder._sk is not None else 0, counts, C.byref(total))
        if code == ERR["NULL"]:  # (no resident sequence, or one whose resident ranges do not cover this run: the library says which)
            raise MinimizerError(code, lib().mm_strerror(code).decode() + ": " + lib().mm_last_error().decode())
        _check(code)
        return [int(c) for c in counts]

    def result(self, entry: int):
        """(device address of the positions, of the super-k-mer indices or 0, count, win_begin, win_end) of an entry."""
        dp, ds = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        cnt, wb, we = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().mm_device_group_result(self.h, entry, C.byref(dp), C.byref(ds), C.byref(cnt), C.byref(wb), C.byref(we)))
        addr = lambda p: C.cast(p, C.c_void_p).value or 0
        return addr(dp), addr(ds), int(cnt.value), int(wb.value), int(we.value)

    def gather(self, root: int, d_dst_pos, d_dst_sk=None):
        """``mm_device_group_gather``: the shards, dense and in window order, into device tensors on the root entry's
        device (device-to-device copies; xGMI between the GPUs of a node).  Returns the number of positions."""
        total = C.c_uint64()
        code = lib().mm_device_group_gather(self.h, root, C.c_void_p(d_dst_pos.data_ptr()),
                                            C.c_void_p(d_dst_sk.data_ptr()) if d_dst_sk is not None else None,
                                            int(d_dst_pos.numel()), C.byref(total))
        if code == ERR["CAPACITY"]:
            raise MinimizerError(code, f"gather capacity {int(d_dst_pos.numel())} < {total.value}")
        _check(code)
        return int(total.value)

    # ---- device-resident batches (mm_device_group_upload_batch, mm_run_batch_sharded_device, _gather_batch)
    def upload_batch(self, seqs):
        """Independent host sequences placed greedily on the entries, each copied to its entry's device only."""
        keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in seqs]
        n = len(keep)
        ptrs = (C.POINTER(C.c_uint8) * max(n, 1))(*[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in keep])
        nbytes = (C.c_uint64 * max(n, 1))(*[a.size for a in keep])
        _check(lib().mm_device_group_upload_batch(self.h, n, ptrs, nbytes))
        self._batch_n = n

    def _batch_count(self) -> int:
        if self._batch_n is None:
            raise MinimizerError(ERR["NULL"], "no resident batch: call upload_batch() first")
        return self._batch_n

    def run_batch_device(self, builder: "Builder", n_bases, base_offsets=None):
        """One batch launch per entry over its resident sequences; returns the per-sequence counts (input order)."""
        n = self._batch_count()
        n_bases = list(n_bases)
        base_offsets = list(base_offsets) if base_offsets is not None else [0] * n
        if len(n_bases) != n or len(base_offsets) != n:  # (a short list used to be zero-padded silently)
            raise MinimizerError(ERR["NULL"], f"run_batch_device: {n} sequences are resident (upload_batch), got "
                                              f"{len(n_bases)} lengths and {len(base_offsets)} base offsets")
        lens = (C.c_uint64 * max(n, 1))(*n_bases)
        offs = (C.c_uint64 * max(n, 1))(*base_offsets)
        counts = (C.c_uint64 * max(n, 1))()
        total = C.c_uint64()
        _check(lib().mm_run_batch_sharded_device(builder.plan().h, self.h, offs, lens, 1 if builder._sk is not None else 0,
                                                 counts, C.byref(total)))
        return [int(c) for c in counts[:n]]

    def values_batch(self, builder: "Builder", u128=False) -> int:
        """``mm_device_group_values_batch``: the k-mer values (``Output.values_u64`` / ``values_u128`` per sequence) of the
        last ``run_batch_device``'s positions, one launch per entry over its resident sequences; ``len`` and
        ``canonical`` come from the builder.  The values stay on the devices (``batch_values``) until the next upload or
        run.  Returns their number."""
        total = C.c_uint64()
        _check(lib().mm_device_group_values_batch(self.h, _value_len(builder), int(builder.canonical), int(bool(u128)),
                                                  C.byref(total)))
        self._batch_u128 = bool(u128)
        return int(total.value)

    def batch_values(self, seq: int):
        """``mm_device_group_batch_values``: (entry, values) of sequence ``seq`` after ``values_batch`` - an int64 CUDA
        tensor on the entry's device that ALIASES the group's buffer (``count`` words, ``2 * count`` after ``u128``:
        {lo, hi} per value), valid until the next upload or run on the group."""
        import torch
        entry, dv, cnt = C.c_int(), C.POINTER(C.c_uint64)(), C.c_uint64()
        _check(lib().mm_device_group_batch_values(self.h, int(seq), C.byref(entry), C.byref(dv), C.byref(cnt)))
        words = int(cnt.value) * (2 if self._batch_u128 else 1)
        device = torch.device("cuda", self._devices[entry.value])
        if words == 0:
            return entry.value, torch.empty(0, dtype=torch.int64, device=device)
        return entry.value, torch.as_tensor(_DeviceWords(C.cast(dv, C.c_void_p).value, words), device=device)

    def gather_batch(self, root: int, d_dst_pos, d_dst_sk=None):
        """All sequences' positions, input order, into device tensors on the root entry's device; returns the offsets."""
        n = self._batch_count()
        offs = (C.c_uint64 * (n + 1))()
        code = lib().mm_device_group_gather_batch(self.h, root, C.c_void_p(d_dst_pos.data_ptr()),
                                                  C.c_void_p(d_dst_sk.data_ptr()) if d_dst_sk is not None else None,
                                                  int(d_dst_pos.numel()), offs)
        if code == ERR["CAPACITY"]:
            raise MinimizerError(code, f"gather capacity {int(d_dst_pos.numel())} < {offs[n]}")
        _check(code)
        return [int(o) for o in offs]

    def run_batch(self, builder: "Builder", seqs, n_bases, base_offsets=None, capacity=None):
        """Independent host sequences placed greedily on the entries (``mm_run_batch_sharded_host``): (positions,
        super-k-mer indices or None, n + 1 offsets); sequence-local positions in input order."""
        plan = builder.plan()
        n = len(seqs)
        keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in seqs]
        ptrs = (C.POINTER(C.c_uint8) * max(n, 1))(*[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in keep])
        lens = (C.c_uint64 * max(n, 1))(*n_bases)
        offs = (C.c_uint64 * max(n, 1))(*(base_offsets or [0] * n))
        cap = max(1, sum(n_bases)) if capacity is None else capacity
        pos = np.empty(cap, dtype=np.uint32)
        sk = np.empty(cap, dtype=np.uint32) if builder._sk is not None else None
        out_offsets = (C.c_uint64 * (n + 1))()
        code = lib().mm_run_batch_sharded_host(plan.h, self.h, n, ptrs, offs, lens, pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               sk.ctypes.data_as(C.POINTER(C.c_uint32)) if sk is not None else None, cap,
                                               out_offsets)
        if code == ERR["CAPACITY"]:
            raise MinimizerError(code, f"output capacity {cap} < {out_offsets[n]}")
        _check(code)
        o = [int(x) for x in out_offsets]
        return pos[:o[-1]], (sk[:o[-1]] if sk is not None else None), o


class _DeviceWords:
    """``n`` 64-bit words of device memory at ``address`` for ``torch.as_tensor`` (no copy, no ownership)."""

    def __init__(self, address: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (address, False), "version": 2}


_default_ws = threading.local()  # .by_device: {device: Workspace} of the calling thread


def default_workspace(device: int = 0) -> Workspace:
    """The calling thread's workspace of ``device`` (the reference's thread-local CACHE, src/lib.rs:217-219): one per
    (thread, device), created at the thread's first use and bound to the thread's current torch stream of that device
    when torch is importable, so that tensor fills / copies issued through torch are ordered with the engine's kernels.
    A workspace serves one thread at a time, so threads never share one of these."""
    by_device = getattr(_default_ws, "by_device", None)
    if by_device is None:
        by_device = _default_ws.by_device = {}
    if device not in by_device:
        stream = None
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream(device).cuda_stream
        except ImportError:
            pass
        by_device[device] = Workspace(device, stream)
    return by_device[device]


# -------------------------------------------------------------------- builder


def NtHasher(k: int | None = None, canonical: bool = True) -> Hasher:
    """seq-hash ``NtHasher::<CANONICAL>::new(k)`` (k only rotates tables inside the plan)."""
    h = Hasher()
    _check(lib().mm_default_hasher(C.byref(h), int(canonical)))
    return h


def MulHasher(k: int | None = None, canonical: bool = True) -> Hasher:
    """seq-hash ``MulHasher::<CANONICAL>::new(k)`` (src/lib.rs:71-72).  PARITY UNPINNED: this engine's
    restatement of the published idea (see mm_mul_hasher in the C header); plug the real per-base values
    in through ``Hasher.from_tables`` where they are known."""
    h = Hasher()
    _check(lib().mm_mul_hasher(C.byref(h), int(canonical)))
    return h


def TextMulHasher(k: int | None = None, canonical: bool = True) -> TextHasher:
    """seq-hash ``MulHasher::<CANONICAL>::new(k)`` over bytes, the default hasher of ``&[u8]`` text
    (src/lib.rs:71-72).  PARITY UNPINNED: this engine's restatement (mm_text_mul_hasher in the C header)."""
    h = TextHasher()
    _check(lib().mm_text_mul_hasher(C.byref(h), int(canonical)))
    return h


def AntiLexHasher(k: int, canonical: bool = True) -> Hasher:
    """seq-hash ``AntiLexHasher::<CANONICAL>::new(k)`` (src/test.rs:83,109).  PARITY UNPINNED."""
    h = Hasher()
    _check(lib().mm_antilex_hasher(C.byref(h), k, int(canonical)))
    return h


class Plan:
    def __init__(self, k, w, canonical, mode, hasher, text=False):
        h = C.c_void_p()
        hp = C.byref(hasher) if hasher is not None else None
        create = lib().mm_plan_create_text if text else lib().mm_plan_create
        _check(create(C.byref(h), k, w, int(canonical), mode, hp))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                lib().mm_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def value_len(self) -> int:
        return lib().mm_plan_value_len(self.h)


def _u128_list(words, n: int) -> list:
    """The first ``n`` values of {lo, hi} word pairs as Python ints."""
    return [int(words[2 * i]) | (int(words[2 * i + 1]) << 64) for i in range(n)]


class Output:
    """``Output`` of src/lib.rs:232-237: positions + lazily computed k-mer values."""

    def __init__(self, builder, seq, min_pos):
        self.len = builder.k if builder.mode == MM_MINIMIZERS else builder.k + builder.w - 1
        self.canonical = builder.canonical
        self.seq = seq
        self.min_pos = min_pos
        self._ws = builder._ws()

    def values_u64(self) -> np.ndarray:
        return self.pos_and_values_u64()[1]

    def values_u128(self) -> list:
        """``Output::values_u128`` (src/lib.rs:587-593): Python ints, len <= 64."""
        return self.pos_and_values_u128()[1]

    def pos_and_values_u128(self):
        """``Output::pos_and_values_u128`` (src/lib.rs:615-630): (positions, Python ints)."""
        pos = np.ascontiguousarray(self.min_pos, dtype=np.uint32)
        vals = np.zeros(2 * len(pos), dtype=np.uint64)
        seq = self.seq
        if _is_text(seq):  # ``&[u8]``: 8 bits per character (a canonical builder or len > 16 raises the C ABI's code)
            text = _text_array(seq)
            _check(lib().mm_values_u128_text_host(self._ws.h, _p(text, C.c_uint8), len(text), TEXT_VALUES_BYTES, self.len,
                                                  int(self.canonical), _p(pos, C.c_uint32), len(pos), _p(vals, C.c_uint64)))
            return pos, _u128_list(vals, len(pos))
        if isinstance(seq, AsciiSeq):
            seq = PackedSeqVec.from_ascii(seq.seq)
        if len(pos):
            _check(lib().mm_values_u128_host(self._ws.h, _p(seq.data, C.c_uint8), seq.offset, seq.length,
                                             self.len, int(self.canonical), _p(pos, C.c_uint32),
                                             len(pos), _p(vals, C.c_uint64)))
        return pos, _u128_list(vals, len(pos))

    def pos_and_values_u64(self):
        """``Output::pos_and_values_u64`` (src/lib.rs:598-612)."""
        pos = np.ascontiguousarray(self.min_pos, dtype=np.uint32)
        vals = np.zeros(len(pos), dtype=np.uint64)
        seq = self.seq
        if _is_text(seq):  # ``&[u8]``: 8 bits per character (a canonical builder or len > 8 raises the C ABI's code)
            text = _text_array(seq)
            _check(lib().mm_values_u64_text_host(self._ws.h, _p(text, C.c_uint8), len(text), TEXT_VALUES_BYTES, self.len,
                                                 int(self.canonical), _p(pos, C.c_uint32), len(pos), _p(vals, C.c_uint64)))
            return pos, vals
        if isinstance(seq, AsciiSeq):
            seq = PackedSeqVec.from_ascii(seq.seq)
        if len(pos):
            _check(lib().mm_values_u64_host(self._ws.h, _p(seq.data, C.c_uint8), seq.offset, seq.length,
                                            self.len, int(self.canonical), _p(pos, C.c_uint32),
                                            len(pos), _p(vals, C.c_uint64)))
        return pos, vals


class Builder:
    """``Builder<CANONICAL, H, SkPos, SYNCMER>`` (src/lib.rs:225-230)."""

    def __init__(self, k, w, canonical, mode, hasher=None, sk_pos=None, workspace=None, text_hasher=None):
        self.k, self.w, self.canonical, self.mode = k, w, canonical, mode
        self._hasher, self._sk, self._workspace = hasher, sk_pos, workspace
        self._text_hasher = text_hasher  # hasher of byte text (None: TextMulHasher, the default of ``&[u8]``)
        self._plan = None
        self._text_plan = None
        self._plan_lock = threading.Lock()  # (threads that share a builder create its plans once)

    def hasher(self, hasher) -> "Builder":  # src/lib.rs:327
        """A ``Hasher`` for 2-bit sequences, or a ``TextHasher`` for byte text; the other kind is kept."""
        if isinstance(hasher, TextHasher):
            return Builder(self.k, self.w, self.canonical, self.mode, self._hasher, self._sk, self._workspace, hasher)
        return Builder(self.k, self.w, self.canonical, self.mode, hasher, self._sk, self._workspace, self._text_hasher)

    def super_kmers(self, sk_pos: list) -> "Builder":  # src/lib.rs:341 (minimizers only)
        if self.mode != MM_MINIMIZERS:
            raise MinimizerError(ERR["BAD_MODE"], "super_kmers() is only defined for minimizers")
        return Builder(self.k, self.w, self.canonical, self.mode, self._hasher, sk_pos, self._workspace,
                       self._text_hasher)

    def workspace(self, ws: Workspace) -> "Builder":
        """The same builder on ``ws``; plans already created are shared (they do not depend on the workspace)."""
        b = Builder(self.k, self.w, self.canonical, self.mode, self._hasher, self._sk, ws, self._text_hasher)
        b._plan, b._text_plan = self._plan, self._text_plan
        return b

    def _ws(self) -> Workspace:
        return self._workspace or default_workspace()

    def plan(self) -> Plan:
        """The builder's plan, created at first use; immutable, so any number of threads may run with it."""
        if self._plan is None:
            with self._plan_lock:
                if self._plan is None:
                    self._plan = Plan(self.k, self.w, self.canonical, self.mode, self._hasher)
        return self._plan

    def text_plan(self) -> Plan:
        """The plan of byte-text runs (mm_plan_create_text), created at first use like ``plan``."""
        if self._text_plan is None:
            with self._plan_lock:
                if self._text_plan is None:
                    self._text_plan = Plan(self.k, self.w, self.canonical, self.mode, self._text_hasher, text=True)
        return self._text_plan

    def prepare(self, ws=None, sequence=True, reads=False, super_kmers=None, text=False) -> dict:
        """Get every kernel this builder's runs dispatch to ready on the workspace's device before the first run
        (mm_plan_prepare): loads prebuilt kernels, compiles the others or reads them from the disk cache, launches
        nothing.  ``super_kmers=None``: as this builder was configured.  ``text``: the byte-text plan instead.
        Returns the report: kernels, compiled, from_disk, unavailable."""
        if super_kmers is None:
            super_kmers = self._sk is not None
        what = ((PREPARE_SEQUENCE if sequence else 0) | (PREPARE_READS if reads else 0) |
                (PREPARE_SUPERKMERS if super_kmers else 0))
        rep = PrepareReport()
        plan = self.text_plan() if text else self.plan()
        _check(lib().mm_plan_prepare(plan.h, (ws or self._ws()).h, what, C.byref(rep)))
        return {"kernels": rep.kernels, "compiled": rep.compiled, "from_disk": rep.from_disk,
                "unavailable": rep.unavailable}

    # -- host sequences -------------------------------------------------
    def run(self, seq, min_pos: list) -> Output:
        """``Builder::run``: positions are APPENDED to ``min_pos`` (src/lib.rs:80-81); like the
        reference's SIMD collector a leading result equal to ``min_pos[-1]`` is dropped
        (src/collect.rs:265-271)."""
        pos, sk = self._run_arrays(seq)
        pos, sk = list(map(int, pos)), (list(map(int, sk)) if sk is not None else None)
        if self.mode == MM_MINIMIZERS:
            while pos and min_pos and pos[0] == min_pos[-1]:
                pos = pos[1:]
                sk = sk[1:] if sk is not None else None
        min_pos.extend(pos)
        if self._sk is not None:
            self._sk.extend(sk)
        return Output(self, seq, min_pos)

    def run_once(self, seq) -> list:
        out: list = []
        self.run(seq, out)
        return out

    def run_with_buf(self, seq, min_pos: list, cache: "Workspace") -> Output:
        """``Builder::run_with_buf`` (src/lib.rs:553-576): ``run`` with the scratch passed explicitly -
        the reference's ``Cache`` is this engine's ``Workspace`` (device buffers + stream)."""
        return self.workspace(cache).run(seq, min_pos)

    def run_scalar(self, seq, min_pos: list) -> Output:
        """``Builder::run_scalar`` (src/lib.rs:370-376, :517-543).  The reference's scalar collectors
        OVERWRITE ``min_pos`` from index 0 and truncate it to the result (src/collect.rs:15-37,39-76,
        src/syncmers.rs:19-48) - no append, no ``last()`` rule; a sequence without a window clears
        ``min_pos`` and (like src/collect.rs:45-48) leaves the super-k-mer vector untouched.  Served by
        the same HIP kernel as ``run``: the scalar flavour differs in the collector's contract only."""
        pos, sk = self._run_arrays(seq)
        min_pos[:] = list(map(int, pos))
        if self._sk is not None and len(seq) >= self.k + self.w - 1:
            self._sk[:] = list(map(int, sk))
        return Output(self, seq, min_pos)

    def run_scalar_once(self, seq) -> list:
        """``Builder::run_scalar_once`` (src/lib.rs:358-362, :511-515)."""
        out: list = []
        self.run_scalar(seq, out)
        return out

    def _run_arrays(self, seq):
        L = lib()
        ws = self._ws()
        n = len(seq)
        plan = self.text_plan() if _is_text(seq) else self.plan()
        lwin = self.k + self.w - 1
        cap = max(1, n - lwin + 1) if n >= lwin else 1
        pos = np.zeros(cap, dtype=np.uint32)
        want_sk = self._sk is not None
        sk = np.zeros(cap, dtype=np.uint32) if want_sk else None
        cnt = C.c_uint64()
        skp = _p(sk, C.c_uint32) if want_sk else None
        if _is_text(seq):  # ``&[u8]`` (src/lib.rs:59): the text path
            a = _text_array(seq)
            _check(L.mm_run_text_host(self.text_plan().h, ws.h, _p(a, C.c_uint8) if n else None, n,
                                      _p(pos, C.c_uint32), skp, cap, C.byref(cnt)))
        elif isinstance(seq, AsciiSeq):
            a = np.frombuffer(seq.seq, dtype=np.uint8)
            _check(L.mm_run_host_ascii(plan.h, ws.h, _p(a, C.c_uint8) if n else None, n,
                                       _p(pos, C.c_uint32), skp, cap, C.byref(cnt)))
        else:
            _check(L.mm_run_host(plan.h, ws.h, _p(seq.data, C.c_uint8), seq.offset, seq.length,
                                 _p(pos, C.c_uint32), skp, cap, C.byref(cnt)))
        m = cnt.value
        return pos[:m], (sk[:m] if want_sk else None)

    # -- PackedNSeq: skip windows with ambiguous bases (src/lib.rs:451-496) --
    def run_skip_ambiguous_windows(self, nseq, min_pos: list) -> Output:
        """``Builder::run_skip_ambiguous_windows`` (canonical builders only). ``nseq`` is a
        ``PackedNSeq`` or, as a convenience, an ``AsciiSeq`` (packed on the device)."""
        L = lib()
        ws = self._ws()
        plan = self.plan()
        n = len(nseq)
        lwin = self.k + self.w - 1
        cap = max(1, n - lwin + 1) if n >= lwin else 1
        pos = np.zeros(cap, dtype=np.uint32)
        cnt = C.c_uint64()
        if isinstance(nseq, AsciiSeq):
            a = np.frombuffer(nseq.seq, dtype=np.uint8)
            _check(L.mm_run_skip_ambiguous_host_ascii(plan.h, ws.h, _p(a, C.c_uint8) if n else None, n,
                                                      _p(pos, C.c_uint32), cap, C.byref(cnt)))
            seq = PackedSeqVec.from_ascii(nseq.seq)
        else:
            seq = nseq.seq
            _check(L.mm_run_skip_ambiguous_host(plan.h, ws.h, _p(seq.data, C.c_uint8), seq.offset,
                                                _p(nseq.amb, C.c_uint8), nseq.amb_offset, n,
                                                _p(pos, C.c_uint32), cap, C.byref(cnt)))
        out = list(map(int, pos[:cnt.value]))
        if self.mode == MM_MINIMIZERS:
            while out and min_pos and out[0] == min_pos[-1]:
                out = out[1:]
        min_pos.extend(out)
        return Output(self, seq, min_pos)

    def run_skip_ambiguous_windows_with_buf(self, nseq, min_pos: list, cache: "Workspace") -> Output:
        """``Builder::run_skip_ambiguous_windows_with_buf`` (src/lib.rs:465-496)."""
        return self.workspace(cache).run_skip_ambiguous_windows(nseq, min_pos)

    def run_skip_ambiguous_windows_once(self, nseq) -> list:
        out: list = []
        self.run_skip_ambiguous_windows(nseq, out)
        return out

    def run_skip_ambiguous_device(self, d_packed, d_amb, n_bases: int, out_pos, base_offset: int = 0,
                                  amb_offset: int = 0, win_begin: int = 0, win_end: int = U64_MAX,
                                  sync: bool = True, d_count=None):
        """Device-resident PackedNSeq (torch uint8 CUDA tensors for the codes and the ambiguity bits)."""
        L = lib()
        cap = out_pos.numel() if out_pos is not None else 0
        args = [self.plan().h, self._ws().h, C.c_void_p(d_packed.data_ptr()), d_packed.numel(), base_offset,
                C.c_void_p(d_amb.data_ptr()), d_amb.numel(), amb_offset, n_bases, win_begin, win_end,
                C.c_void_p(out_pos.data_ptr()) if out_pos is not None else None, cap]
        if sync:
            cnt = C.c_uint64()
            code = L.mm_run_skip_ambiguous_device(*args, C.byref(cnt))
            if code == ERR["CAPACITY"]:
                raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
            _check(code)
            return cnt.value
        _check(L.mm_run_skip_ambiguous_device_async(*args, C.c_void_p(d_count.data_ptr()) if d_count is not None else None))
        return None

    # -- device-resident sequences (torch uint8 CUDA tensors) -----------
    def run_device(self, d_packed, n_bases: int, out_pos, out_sk=None, base_offset: int = 0,
                   win_begin: int = 0, win_end: int = U64_MAX, sync: bool = True, d_count=None):
        """Run on a device-resident PackedSeq. ``d_packed``/``out_pos``/``out_sk``/``d_count`` are
        torch CUDA tensors (uint8 / int32-or-uint32 / int64). Returns the count if ``sync``."""
        L = lib()
        ws = self._ws()
        plan = self.plan()
        cap = out_pos.numel() if out_pos is not None else 0
        args = [plan.h, ws.h, C.c_void_p(d_packed.data_ptr()), d_packed.numel(), base_offset, n_bases,
                win_begin, win_end, C.c_void_p(out_pos.data_ptr()) if out_pos is not None else None,
                C.c_void_p(out_sk.data_ptr()) if out_sk is not None else None, cap]
        if sync:
            cnt = C.c_uint64()
            code = L.mm_run_device(*args, C.byref(cnt))
            if code == ERR["CAPACITY"]:
                raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
            _check(code)
            return cnt.value
        _check(L.mm_run_device_async(*args, C.c_void_p(d_count.data_ptr()) if d_count is not None else None))
        return None

    def run_text_device(self, d_text, n: int, out_pos, out_sk=None, win_begin: int = 0, win_end: int = U64_MAX,
                        sync: bool = True, d_count=None):
        """Run on device-resident byte text (``&[u8]``; a torch uint8 CUDA tensor of at least ``n`` bytes).
        ``out_pos``/``out_sk``/``d_count`` as for ``run_device``.  Returns the count if ``sync``."""
        L = lib()
        cap = out_pos.numel() if out_pos is not None else 0
        args = [self.text_plan().h, self._ws().h, C.c_void_p(d_text.data_ptr()) if d_text is not None else None,
                d_text.numel() if d_text is not None else 0, n, win_begin, win_end,
                C.c_void_p(out_pos.data_ptr()) if out_pos is not None else None,
                C.c_void_p(out_sk.data_ptr()) if out_sk is not None else None, cap]
        if sync:
            cnt = C.c_uint64()
            code = L.mm_run_text_device(*args, C.byref(cnt))
            if code == ERR["CAPACITY"]:
                raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
            _check(code)
            return cnt.value
        _check(L.mm_run_text_device_async(*args, C.c_void_p(d_count.data_ptr()) if d_count is not None else None))
        return None


def run_batch_device(builder: "Builder", d_seqs, n_bases, out_pos, out_sk=None, base_offsets=None):
    """Many device-resident sequences (list of torch uint8 CUDA tensors) with one plan; positions
    are sequence-local, written back to back into ``out_pos``. Returns the n_seqs+1 offsets."""
    L = lib()
    ws = builder._ws()
    plan = builder.plan()
    n = len(d_seqs)
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in d_seqs])
    nbytes = (C.c_uint64 * max(n, 1))(*[t.numel() for t in d_seqs])
    lens = (C.c_uint64 * max(n, 1))(*n_bases)
    offs = (C.c_uint64 * max(n, 1))(*(base_offsets or [0] * n))
    out_offsets = (C.c_uint64 * (n + 1))()
    code = L.mm_run_batch_device(plan.h, ws.h, n, ptrs, nbytes, offs, lens, C.c_void_p(out_pos.data_ptr()),
                                 C.c_void_p(out_sk.data_ptr()) if out_sk is not None else None,
                                 out_pos.numel(), out_offsets)
    _check(code)
    return list(out_offsets)


def run_reads_device(builder: "Builder", d_packed, n_reads, read_stride, read_len, out_pos, out_offsets,
                     read_lens=None, base_offset=0, d_count=None, sync=True, d_amb=None, amb_offset=0,
                     out_sk=None):
    """Batched short reads in one packed device buffer (read r at base ``base_offset + r*read_stride``);
    read-local positions go back to back into ``out_pos`` and ``out_offsets`` (int64/uint64 CUDA
    tensor, n_reads+1) delimits the reads; ``out_sk`` also receives the super-k-mer indices
    (read-local window of the first selection). Returns the total count when ``sync``."""
    L = lib()
    ws = builder._ws()
    plan = builder.plan()
    cap = out_pos.numel() if out_pos is not None else 0
    args = [plan.h, ws.h, C.c_void_p(d_packed.data_ptr()), d_packed.numel(), base_offset]
    if d_amb is not None:  # PackedNSeq reads: skip windows with ambiguous bases
        args += [C.c_void_p(d_amb.data_ptr()), d_amb.numel(), amb_offset]
    args += [n_reads, read_stride, read_len, C.c_void_p(read_lens.data_ptr()) if read_lens is not None else None,
             C.c_void_p(out_pos.data_ptr()) if out_pos is not None else None]
    if out_sk is not None:
        if d_amb is not None:
            raise MinimizerError(ERR["BAD_MODE"], "no super-k-mer flavour of the skip-ambiguous run")
        args += [C.c_void_p(out_sk.data_ptr())]
    args += [cap, C.c_void_p(out_offsets.data_ptr())]
    if out_sk is not None:
        fsync, fasync = L.mm_run_reads_superkmers_device, L.mm_run_reads_superkmers_device_async
    else:
        fsync, fasync = ((L.mm_run_reads_skip_ambiguous_device, L.mm_run_reads_skip_ambiguous_device_async)
                         if d_amb is not None else (L.mm_run_reads_device, L.mm_run_reads_device_async))
    if sync:
        cnt = C.c_uint64(0)
        code = fsync(*args, C.byref(cnt))
        if code == ERR["CAPACITY"]:
            raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
        _check(code)
        return cnt.value
    _check(fasync(*args, C.c_void_p(d_count.data_ptr()) if d_count is not None else None))
    return None


def pinned_array(shape, dtype):
    """numpy array backed by page-locked host memory (mm_host_alloc); keep the returned owner alive."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    _check(lib().mm_host_alloc(C.byref(p), max(n, 1)))

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            try:
                lib().mm_host_free(self.ptr)
            except Exception:
                pass

    owner = _Owner(p)
    buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return arr, owner


def minimizers(k, w):  # src/lib.rs:240
    return Builder(k, w, False, MM_MINIMIZERS)


def canonical_minimizers(k, w):  # src/lib.rs:250
    return Builder(k, w, True, MM_MINIMIZERS)


def closed_syncmers(k, w):  # src/lib.rs:269
    return Builder(k, w, False, MM_CLOSED_SYNCMERS)


def canonical_closed_syncmers(k, w):  # src/lib.rs:282
    return Builder(k, w, True, MM_CLOSED_SYNCMERS)


def open_syncmers(k, w):  # src/lib.rs:301
    return Builder(k, w, False, MM_OPEN_SYNCMERS)


def canonical_open_syncmers(k, w):  # src/lib.rs:311
    return Builder(k, w, True, MM_OPEN_SYNCMERS)


# README.md:65 uses this older name for canonical closed syncmers
canonical_syncmers = canonical_closed_syncmers
syncmers = closed_syncmers


def minimizer_positions(seq, k, w):  # src/lib.rs:639
    return minimizers(k, w).run_once(seq)


def canonical_minimizer_positions(seq, k, w):  # src/lib.rs:652
    return canonical_minimizers(k, w).run_once(seq)


class FastaRecords:
    """Records of a FASTA text packed on the device (``fasta_pack_device``): ``packed`` = one 2-bit buffer holding
    all sequences back to back, ``base`` = the n + 1 base offsets delimiting them, ``text_pos`` = byte offset of
    every record's '>' in the text; ``amb`` (``fasta_pack_n_device`` only, else None) = one ambiguity bit per base of
    ``packed``, in the same numbering."""

    def __init__(self, packed, base, text_pos, amb=None):
        self.packed, self.base, self.text_pos, self.amb = packed, base, text_pos, amb

    def __len__(self):
        return len(self.base) - 1

    def lengths(self):
        return [int(self.base[i + 1] - self.base[i]) for i in range(len(self))]

    def views(self):
        """(tensor, base_offset, n_bases) per record, as ``run_batch_device`` takes them."""
        out = []
        for i in range(len(self)):
            b, e = int(self.base[i]), int(self.base[i + 1])
            out.append((self.packed[b // 4:], b % 4, e - b))
        return out

    def header(self, text: bytes, i: int) -> bytes:
        """The header line of record i (without '>' and line end), sliced from the host copy of the text."""
        p = int(self.text_pos[i]) + 1
        q = text.find(b"\n", p)
        return text[p:len(text) if q < 0 else q].rstrip(b"\r")


def _fasta_pack(text, max_records: int, device: int, with_amb: bool) -> FastaRecords:
    """What ``fasta_pack_device`` and ``fasta_pack_n_device`` share: the upload, the buffers, the one call, the slicing."""
    import torch

    dev = f"cuda:{device}"
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    if isinstance(text, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(text)).to(dev) if text.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        t = text
    n = int(t.numel())
    ws = default_workspace(device)
    packed = torch.empty((n // 4 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    amb = torch.empty((n // 8 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev) if with_amb else None
    rec_base = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(max(max_records, 1), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(device)
    out = (C.c_uint64 * 2)()
    head = (ws.h, C.c_void_p(t.data_ptr()) if n else None, n, C.c_void_p(packed.data_ptr()), packed.numel() // 4 * 4)
    tail = (C.c_void_p(rec_base.data_ptr()), C.c_void_p(rec_pos.data_ptr()), max_records, C.c_void_p(counts.data_ptr()), out)
    if with_amb:
        code = lib().mm_fasta_pack_n_device(*head, C.c_void_p(amb.data_ptr()), amb.numel() // 4 * 4, *tail)
    else:
        code = lib().mm_fasta_pack_device(*head, *tail)
    if code == ERR["CAPACITY"]:
        if out[1] > max_records:
            raise MinimizerError(code, f"{out[1]} records > max_records {max_records}")
        raise MinimizerError(code, f"{out[0]} bases do not fit the packed buffer of {packed.numel() // 4 * 4} bytes")
    _check(code)
    n_rec = int(out[1])
    return FastaRecords(packed, rec_base[: n_rec + 1].cpu().numpy().astype(np.uint64),
                        rec_pos[:n_rec].cpu().numpy().astype(np.uint64), amb)


def fasta_pack_device(text, max_records: int = 1 << 16, device: int = 0) -> FastaRecords:
    """needletail::parse_fastx_file + PackedSeqVec::from_ascii of every record (bench/src/lib.rs:51-82) on the
    device: ``text`` = the file's bytes (bytes / numpy uint8 / torch uint8 CUDA tensor), FASTA or - since round 4,
    told apart by the first non-blank byte like needletail does - FASTQ (four-line records)."""
    return _fasta_pack(text, max_records, device, False)


fastx_pack_device = fasta_pack_device  # (the reference's loader call reads both formats)


def fasta_pack_n_device(text, max_records: int = 1 << 16, device: int = 0) -> FastaRecords:
    """``fasta_pack_device`` for texts with ``N``: the same records (FASTA or FASTQ) plus ``.amb``, one ambiguity bit per
    packed base, set for every sequence byte that is not ``ACGT`` / ``acgt`` (PackedNSeqVec::from_ascii per record,
    ``mm_fasta_pack_n_device``).  What ``run_packed_reads_skip_ambiguous_device`` takes."""
    return _fasta_pack(text, max_records, device, True)


fastx_pack_n_device = fasta_pack_n_device


def run_reads_host(builder: "Builder", reads, super_kmers: bool = False):
    """Many short host sequences in ONE call (``mm_run_packed_reads_host``): ``reads`` = list of ``PackedSeq`` / ASCII
    ``bytes``; returns (positions, offsets, indices or None) - read r's read-local positions are
    ``positions[offsets[r]:offsets[r + 1]]``.  The replacement of a per-read loop over ``Builder.run``."""
    codes = []
    for s in reads:
        if isinstance(s, (bytes, bytearray)):
            a = np.frombuffer(bytes(s), dtype=np.uint8)
            codes.append((a >> 1) & 3)
        else:  # PackedSeq view
            a = np.asarray(s.data, dtype=np.uint8)
            idx = np.arange(s.offset, s.offset + s.len)
            codes.append((a[idx // 4] >> (2 * (idx % 4))) & 3)
    lens = [len(c) for c in codes]
    starts = np.zeros(len(lens) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(starts[-1])
    flat = np.concatenate(codes).astype(np.uint8) if total else np.zeros(0, dtype=np.uint8)
    pad = np.zeros((-total) % 4, dtype=np.uint8)
    q = np.concatenate([flat, pad]).reshape(-1, 4)
    packed = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8) if total else np.zeros(1, dtype=np.uint8)
    cap = max(1, total)
    pos = np.empty(cap, dtype=np.uint32)
    sk = np.empty(cap, dtype=np.uint32) if super_kmers else None
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    cnt = C.c_uint64()
    ws = builder._ws()
    _check(lib().mm_run_packed_reads_host(builder.plan().h, ws.h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), len(lens),
                                          starts.ctypes.data_as(C.POINTER(C.c_uint64)), max(lens) if lens else 0,
                                          pos.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          sk.ctypes.data_as(C.POINTER(C.c_uint32)) if sk is not None else None, cap,
                                          offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt)))
    n = int(cnt.value)
    return pos[:n], [int(o) for o in offs], (sk[:n] if sk is not None else None)


def _text_records(records):
    """Records of byte text (``bytes`` / ``bytearray`` / ``memoryview`` / ``np.uint8``) -> (text, starts): the records back
    to back and their [n + 1] starts."""
    arrs = []
    for s in records:
        if not _is_text(s):
            raise TypeError(f"byte-text records are bytes, bytearray or np.uint8 arrays, not {type(s).__name__}")
        arrs.append(_text_array(s))
    starts = np.zeros(len(arrs) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    text = np.concatenate(arrs).astype(np.uint8, copy=False) if int(starts[-1]) else np.zeros(1, dtype=np.uint8)
    return text, starts


def run_text_batch_host(builder: "Builder", records, super_kmers: bool = False):
    """Many records of byte text (``&[u8]``: protein, other alphabets, lines of text) in ONE call
    (``mm_run_text_batch_host``); returns (positions, offsets, indices or None) - record r's record-local positions are
    ``positions[offsets[r]:offsets[r + 1]]``, what ``Builder.run`` returns for it alone.  The text plan of ``builder``
    (its ``TextHasher``, default ``TextMulHasher``) runs."""
    text, starts = _text_records(records)
    n_rec = len(starts) - 1
    total = int(starts[-1])
    cap = max(1, total)
    pos = np.empty(cap, dtype=np.uint32)
    sk = np.empty(cap, dtype=np.uint32) if super_kmers else None
    offs = np.zeros(n_rec + 1, dtype=np.uint64)
    cnt = C.c_uint64()
    ws = builder._ws()
    _check(lib().mm_run_text_batch_host(builder.text_plan().h, ws.h, _p(text, C.c_uint8), n_rec, _p(starts, C.c_uint64),
                                        _p(pos, C.c_uint32), _p(sk, C.c_uint32) if sk is not None else None, cap,
                                        _p(offs, C.c_uint64), C.byref(cnt)))
    n = int(cnt.value)
    return pos[:n], [int(o) for o in offs], (sk[:n] if sk is not None else None)


def run_text_batch_device(builder: "Builder", d_text, d_starts, n_chars: int, out_pos, out_offsets, out_sk=None):
    """Many records of device-resident byte text in one launch (``mm_run_text_batch_device``): ``d_text`` a uint8 CUDA
    tensor, ``d_starts`` an int64 CUDA tensor of n + 1 non-decreasing record starts (``n_chars = d_starts[n]``),
    ``out_offsets`` an int64 CUDA tensor of n + 1; ``out_pos`` (None: count only) / ``out_sk`` int32 tensors.  Returns the
    number of positions."""
    n_rec = d_starts.numel() - 1
    if n_rec < 0:
        raise ValueError("d_starts holds n + 1 starts")
    cap = out_pos.numel() if out_pos is not None else 0
    cnt = C.c_uint64()
    code = lib().mm_run_text_batch_device(
        builder.text_plan().h, builder._ws().h, C.c_void_p(d_text.data_ptr()) if d_text is not None else None,
        d_text.numel() if d_text is not None else 0, n_rec, C.c_void_p(d_starts.data_ptr()), int(n_chars),
        C.c_void_p(out_pos.data_ptr()) if out_pos is not None else None,
        C.c_void_p(out_sk.data_ptr()) if out_sk is not None else None, cap, C.c_void_p(out_offsets.data_ptr()),
        C.byref(cnt))
    if code == ERR["CAPACITY"] and out_pos is not None and cnt.value > cap:
        raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
    _check(code)
    return int(cnt.value)


class FastaTextRecords:
    """Records of a FASTA text as byte text on the device (``fasta_text_device``): ``seq`` = a uint8 CUDA tensor holding
    all sequences back to back, as they stand in the file; ``starts`` = an int64 CUDA tensor of n + 1 byte offsets
    delimiting them - what ``run_text_batch_device`` and ``values_text_batch_device`` take as ``d_text`` / ``d_starts``;
    ``text_pos`` = byte offset of every record's '>' in the text (host array); ``n_chars`` = ``starts[n]``."""

    def __init__(self, seq, starts, text_pos, n_chars):
        self.seq, self.starts, self.text_pos, self.n_chars = seq, starts, text_pos, int(n_chars)

    def __len__(self):
        return int(self.starts.numel()) - 1

    def lengths(self):
        s = self.starts.cpu().numpy()
        return [int(x) for x in s[1:] - s[:-1]]

    header = FastaRecords.header


def fasta_text_device(text, max_records: int = 1 << 16, device: int = 0) -> FastaTextRecords:
    """The records of a FASTA file as byte text, read on the device (``mm_fasta_text_device``): ``text`` = the file's
    bytes (bytes / numpy uint8 / torch uint8 CUDA tensor).  The reader of ``fasta_pack_device``; the sequence bytes are
    kept as they are (protein, any alphabet).  FASTQ raises ``MinimizerError`` (``MM_ERR_FORMAT``)."""
    import torch

    dev = f"cuda:{device}"
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    if isinstance(text, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(text)).to(dev) if text.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        t = text
    n = int(t.numel())
    ws = default_workspace(device)
    seq = torch.empty(max(n, 4), dtype=torch.uint8, device=dev)
    starts = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(max(max_records, 1), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(device)
    out = (C.c_uint64 * 2)()
    code = lib().mm_fasta_text_device(ws.h, C.c_void_p(t.data_ptr()) if n else None, n, C.c_void_p(seq.data_ptr()), n,
                                      C.c_void_p(starts.data_ptr()), C.c_void_p(rec_pos.data_ptr()), max_records,
                                      C.c_void_p(counts.data_ptr()), out)
    if code == ERR["CAPACITY"]:
        raise MinimizerError(code, f"{out[1]} records > max_records {max_records}")
    _check(code)
    n_chars, n_rec = int(out[0]), int(out[1])
    return FastaTextRecords(seq[:n_chars], starts[: n_rec + 1], rec_pos[:n_rec].cpu().numpy().astype(np.uint64), n_chars)


def run_fasta_text_device(builder: "Builder", records: FastaTextRecords, out_pos, out_offsets, out_sk=None):
    """All records of ``fasta_text_device`` in one launch of the text plan (``run_text_batch_device`` on them): record-local
    positions, ``out_offsets`` (int64 CUDA tensor, n + 1) delimits the records.  Returns the number of positions."""
    return run_text_batch_device(builder, records.seq, records.starts, records.n_chars, out_pos, out_offsets, out_sk)


def text_counts_view(k: int, w: int, max_chars: int, max_records: int, n_chars: int, n_records: int) -> dict:
    """What the kernels of the counts calls make of the device's counts and the caller's bounds
    (``mm_debug_text_counts_view``: the function they call, on the host; no GPU)."""
    out = (C.c_uint64 * 4)()
    _check(lib().mm_debug_text_counts_view(k, w, max_chars, max_records, n_chars, n_records, out))
    return {"real_tiles": int(out[0]), "launched_tiles": int(out[1]), "win_end": int(out[2]), "refused": bool(out[3])}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run_text_batch_counts_device(builder: "Builder", d_text, d_starts, d_counts, out_pos, out_offsets, out_sk=None,
                                 max_chars=None, wait=False, d_count=None):
    """``run_text_batch_device`` with the two counts taken from the DEVICE (``mm_run_text_batch_counts_device_async``):
    ``d_counts`` = an int64 CUDA tensor {characters, records} as ``mm_fasta_text_device_async`` writes it, read when the
    kernels run; ``d_starts`` / ``out_offsets`` hold ``max_records + 1`` entries, ``max_chars`` (default: all of ``d_text``)
    bounds the characters.  Queued on the builder's workspace, nothing waits: returns None and ``Workspace.check`` reports
    counts beyond the bounds as ``MM_ERR_CAPACITY`` (``d_count``: an optional int64 CUDA tensor that receives the number of
    positions).  ``wait=True`` (``mm_run_text_batch_counts_device``): one wait, returns (positions, n_chars, n_records)."""
    max_rec = d_starts.numel() - 1
    if max_rec < 0 or out_offsets.numel() < max_rec + 1:
        raise ValueError("d_starts and out_offsets hold max_records + 1 entries each")
    if d_counts.numel() < 2:
        raise ValueError("d_counts holds two words: characters, records")
    text_bytes = d_text.numel() if d_text is not None else 0
    if max_chars is None:
        max_chars = text_bytes
    cap = out_pos.numel() if out_pos is not None else 0
    args = (builder.text_plan().h, builder._ws().h, _ptr(d_text), text_bytes, int(max_chars), max_rec, _ptr(d_starts),
            _ptr(d_counts), _ptr(out_pos), _ptr(out_sk), cap, _ptr(out_offsets))
    if not wait:
        _check_counts(lib().mm_run_text_batch_counts_device_async(*args, _ptr(d_count)))
        return None
    out = (C.c_uint64 * 3)()
    code = lib().mm_run_text_batch_counts_device(*args, out)
    if code == ERR["CAPACITY"]:
        if out_pos is not None and out[0] > cap:
            raise MinimizerError(code, f"output capacity {cap} < {out[0]}")
        raise MinimizerError(code, f"counts ({out[1]} characters, {out[2]} records) beyond max_chars {int(max_chars)} / "
                                   f"max_records {max_rec}")
    _check_counts(code)
    return int(out[0]), int(out[1]), int(out[2])


def _check_counts(code: int):
    """``_check`` that also shows why a counts call refused a plan (``MM_ERR_BAD_MODE`` with ``mm_last_error``)."""
    if code == ERR["BAD_MODE"]:
        L = lib()
        raise MinimizerError(code, L.mm_strerror(code).decode() + ": " + L.mm_last_error().decode())
    _check(code)


def values_text_batch_counts_device(builder: "Builder", d_text, d_starts, d_counts, d_pos, d_out_offsets, n_pos_max, encoding,
                                    u128=False, out=None, max_chars=None):
    """``values_text_batch_device`` for a counts run (``mm_values_u64_text_batch_counts_device_async`` /
    ``mm_values_u128_text_batch_counts_device_async``): ``d_text`` / ``d_starts`` / ``d_counts`` / ``max_chars`` as
    ``run_text_batch_counts_device`` took them, ``d_pos`` / ``d_out_offsets`` as it wrote them.  The number of records and
    the true count are read on the device; counts beyond the bounds and the kernel writes nothing.  Asynchronous on the
    builder's workspace."""
    import torch
    max_rec = d_starts.numel() - 1
    if max_rec < 0 or d_out_offsets.numel() < max_rec + 1:
        raise ValueError("d_starts and d_out_offsets hold max_records + 1 entries each")
    n_pos_max = int(n_pos_max)
    per = 2 if u128 else 1
    if out is None:
        out = torch.zeros(per * n_pos_max, dtype=torch.int64, device=d_pos.device)
        torch.cuda.synchronize(d_pos.device)
    elif out.numel() < per * n_pos_max:
        raise ValueError(f"out holds {out.numel()} words, {per * n_pos_max} needed")
    if d_pos.numel() < n_pos_max:
        raise ValueError(f"d_pos holds {d_pos.numel()} positions, n_pos_max is {n_pos_max}")
    text_bytes = d_text.numel() if d_text is not None else 0
    if max_chars is None:
        max_chars = text_bytes
    f = lib().mm_values_u128_text_batch_counts_device_async if u128 else lib().mm_values_u64_text_batch_counts_device_async
    _check(f(builder._ws().h, _ptr(d_text), text_bytes, int(max_chars), max_rec, _ptr(d_starts), _ptr(d_counts),
             int(encoding), _value_len(builder), int(builder.canonical), _ptr(d_pos), _ptr(d_out_offsets), n_pos_max,
             _ptr(out)))
    return out


class FastaTextPipeline:
    """What ``fasta_text_pipeline_device`` queued: the device tensors of loader, run and values (``seq``, ``starts``,
    ``rec_pos``, ``counts``, ``pos``, ``offsets``, ``count``, ``values`` or None), all still being written until
    ``finish()`` has waited."""

    def __init__(self, builder, ws, seq, starts, rec_pos, counts, pos, offsets, count, values, max_records):
        self.builder, self.ws = builder, ws
        self.seq, self.starts, self.rec_pos, self.counts = seq, starts, rec_pos, counts
        self.pos, self.offsets, self.count, self.values = pos, offsets, count, values
        self.max_records = max_records

    def finish(self):
        """The ONE wait of the pipeline: ``Workspace.check`` (``MinimizerError`` ``MM_ERR_CAPACITY`` when the file holds
        more than ``max_records`` records), then the counts.  Returns (records, n_positions, positions, offsets, values):
        the ``FastaTextRecords`` of ``fasta_text_device``, the count ``run_fasta_text_device`` returns with its
        ``out_pos[:count]`` / ``out_offsets`` (CUDA tensors), and the values tensor of ``values_text_batch_device`` cut to
        the count (None when no encoding was given)."""
        try:
            self.ws.check()
        except MinimizerError as e:
            if e.code == ERR["CAPACITY"]:
                raise MinimizerError(e.code, f"{e} ({lib().mm_last_error().decode()}); max_records was {self.max_records}")
            raise
        n_chars, n_rec = (int(x) for x in self.counts.cpu().numpy())
        cnt = int(self.count.item())
        recs = FastaTextRecords(self.seq[:n_chars], self.starts[: n_rec + 1],
                                self.rec_pos[:n_rec].cpu().numpy().astype(np.uint64), n_chars)
        vals = None
        if self.values is not None:
            per = self.values.numel() // max(1, self.pos.numel())
            vals = self.values[: per * cnt]
        return recs, cnt, self.pos[:cnt], self.offsets[: n_rec + 1], vals


def fasta_text_pipeline_device(builder: "Builder", text, max_records: int, encoding=None, u128=False) -> FastaTextPipeline:
    """File bytes -> records -> positions (-> values) queued on ONE stream with no synchronisation in between:
    ``mm_fasta_text_device_async``, ``mm_run_text_batch_counts_device_async`` and, with an ``encoding``
    (``TEXT_VALUES_BYTES`` / ``TEXT_VALUES_DNA``), ``mm_values_*_text_batch_counts_device_async`` on the builder's
    workspace; the loader's counts never visit the host.  ``text`` = the file's bytes (bytes / numpy uint8 / torch uint8
    CUDA tensor on the workspace's device).  Returns a ``FastaTextPipeline``; its ``finish()`` waits once.  The
    asynchronous loader does NOT look at the first byte: a FASTQ text is read by the FASTA rules (a quality line may begin
    with '>'), so its records are nonsense - the caller knows its format or uses ``fasta_text_device``."""
    import torch

    ws = builder._ws()
    dev = f"cuda:{ws.device}"
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    if isinstance(text, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(text)).to(dev) if text.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        t = text
    n = int(t.numel())
    max_records = int(max_records)
    seq = torch.empty(max(n, 4), dtype=torch.uint8, device=dev)
    starts = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(max(max_records, 1), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    offsets = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    per = 2 if u128 else 1
    values = torch.zeros(per * max(n, 1), dtype=torch.int64, device=dev) if encoding is not None else None
    torch.cuda.synchronize(ws.device)  # (the tensors above are torch's work on its own stream: before, not between)
    _check(lib().mm_fasta_text_device_async(ws.h, _ptr(t) if n else None, n, _ptr(seq), n, _ptr(starts), _ptr(rec_pos),
                                            max_records, _ptr(counts)))
    seq_n = seq[:n] if n else seq[:0]
    run_text_batch_counts_device(builder, seq_n if n else None, starts, counts, pos, offsets, max_chars=n, d_count=count)
    if encoding is not None and n and max_records:
        values_text_batch_counts_device(builder, seq_n, starts, counts, pos, offsets, pos.numel(), encoding, u128=u128,
                                        out=values, max_chars=n)
    return FastaTextPipeline(builder, ws, seq, starts, rec_pos, counts, pos, offsets, count, values, max_records)


def lane_counts_view(max_bases: int, max_records: int, n_bases: int, n_records: int) -> dict:
    """What the lane-table kernels of the reads counts calls make of the device's counts and the caller's bounds
    (``mm_debug_lane_counts_view``: the function they call, on the host; no GPU)."""
    out = (C.c_uint64 * 3)()
    _check(lib().mm_debug_lane_counts_view(max_bases, max_records, n_bases, n_records, out))
    return {"n_reads_eff": int(out[0]), "refused": bool(out[1]), "lane_bound": int(out[2])}


def run_packed_reads_counts_device(builder: "Builder", d_packed, d_starts, d_counts, out_pos, out_offsets, out_sk=None,
                                   max_bases=None, max_records=None, amb=None, sync=True, d_count=None):
    """``run_packed_reads_device`` with the two counts taken from the DEVICE (``mm_run_packed_reads_counts_device*``):
    ``d_packed`` / ``d_starts`` / ``d_counts`` = the packed uint8 buffer, the int64 starts (``max_records + 1``) and the
    int64 {bases, records} as ``mm_fastq_pack_device_async`` / ``mm_fasta_pack_device_async`` write them, read when the
    kernels run.  ``max_bases`` (default: all of ``d_packed``) and ``max_records`` (default: what ``d_starts`` holds)
    bound them; ``out_offsets`` holds ``max_records + 1`` entries and is written whole (reads past the real count are
    empty).  ``amb`` (uint8 CUDA tensor of a ``*_pack_n`` packer): the skip-ambiguous form.  Always a lane-table launch.
    ``sync=True``: one wait, returns (positions, n_bases, n_records).  ``sync=False``: queued on the builder's workspace,
    returns None; ``Workspace.check`` reports counts beyond the bounds as ``MM_ERR_CAPACITY`` (``d_count``: an optional
    int64 CUDA tensor that receives the number of positions)."""
    if max_records is None:
        max_records = d_starts.numel() - 1
    max_records = int(max_records)
    if max_records < 0 or d_starts.numel() < max_records + 1 or out_offsets.numel() < max_records + 1:
        raise ValueError("d_starts and out_offsets hold max_records + 1 entries each")
    if d_counts.numel() < 2:
        raise ValueError("d_counts holds two words: bases, records")
    packed_bytes = int(d_packed.numel())
    if max_bases is None:
        max_bases = 4 * packed_bytes
    if amb is not None and out_sk is not None:
        raise ValueError("the skip-ambiguous form has no super-k-mer indices")
    cap = out_pos.numel() if out_pos is not None else 0
    head = (builder.plan().h, builder._ws().h, _ptr(d_packed), packed_bytes, 0)
    tail = (int(max_bases), max_records, _ptr(d_starts), _ptr(d_counts), _ptr(out_pos))
    if amb is not None:
        args = head + (_ptr(amb), int(amb.numel()), 0) + tail + (cap, _ptr(out_offsets))
        f_async, f_sync = (lib().mm_run_packed_reads_skip_ambiguous_counts_device_async,
                           lib().mm_run_packed_reads_skip_ambiguous_counts_device)
    else:
        args = head + tail + (_ptr(out_sk), cap, _ptr(out_offsets))
        f_async, f_sync = lib().mm_run_packed_reads_counts_device_async, lib().mm_run_packed_reads_counts_device
    if not sync:
        _check_counts(f_async(*args, _ptr(d_count)))
        return None
    out = (C.c_uint64 * 3)()
    code = f_sync(*args, out)
    if code == ERR["CAPACITY"]:
        if out_pos is not None and out[0] > cap:
            raise MinimizerError(code, f"output capacity {cap} < {out[0]}")
        raise MinimizerError(code, f"counts ({out[1]} bases, {out[2]} records) beyond max_bases {int(max_bases)} / "
                                   f"max_records {max_records}")
    _check_counts(code)
    return int(out[0]), int(out[1]), int(out[2])


class FastxPipeline:
    """What ``fastx_pipeline_device`` queued: the device tensors of packer, run and values (``packed``, ``amb`` or None,
    ``starts``, ``rec_pos``, ``counts``, ``pos``, ``offsets``, ``count``, ``values`` or None), all still being written
    until ``finish()`` has waited."""

    def __init__(self, builder, ws, packed, amb, starts, rec_pos, counts, pos, offsets, count, values, max_records):
        self.builder, self.ws = builder, ws
        self.packed, self.amb, self.starts, self.rec_pos, self.counts = packed, amb, starts, rec_pos, counts
        self.pos, self.offsets, self.count, self.values = pos, offsets, count, values
        self.max_records = max_records

    def finish(self):
        """The ONE wait of the pipeline: ``Workspace.check`` (``MinimizerError`` ``MM_ERR_CAPACITY`` when the file holds
        more than ``max_records`` records), then the counts.  Returns (records, n_positions, positions, offsets, values):
        the ``FastaRecords`` of ``fasta_pack_device``, the count ``run_packed_reads_device`` returns with its
        ``out_pos[:count]`` / ``out_offsets[:n + 1]`` (CUDA tensors), and the values tensor of ``values_reads_device``
        cut to the count (None when no values were asked for)."""
        try:
            self.ws.check()
        except MinimizerError as e:
            if e.code == ERR["CAPACITY"]:
                raise MinimizerError(e.code, f"{e} ({lib().mm_last_error().decode()}); max_records was {self.max_records}")
            raise
        _, n_rec = (int(x) for x in self.counts.cpu().numpy())
        cnt = int(self.count.item())
        recs = FastaRecords(self.packed, self.starts[: n_rec + 1].cpu().numpy().astype(np.uint64),
                            self.rec_pos[:n_rec].cpu().numpy().astype(np.uint64), self.amb)
        vals = None
        if self.values is not None:
            per = self.values.numel() // max(1, self.pos.numel())
            vals = self.values[: per * cnt]
        return recs, cnt, self.pos[:cnt], self.offsets[: n_rec + 1], vals


def fastx_pipeline_device(builder: "Builder", text, max_records: int, fmt: str, with_amb=False, values=None,
                          u128=False) -> FastxPipeline:
    """FASTA / FASTQ bytes -> packed records -> positions (-> values) queued on ONE stream with no synchronisation in
    between: ``mm_fastq_pack_device_async`` / ``mm_fasta_pack_device_async`` (``with_amb``: their ``_n`` forms and the
    skip-ambiguous run), ``mm_run_packed_reads_counts_device_async`` and, with ``values`` true (or ``u128``),
    ``mm_values_u64/u128_reads_device_async`` with ``n_reads = max_records`` on the builder's workspace; the packer's counts
    never visit the host.  ``text`` = the file's bytes (bytes / numpy uint8 / torch uint8 CUDA tensor on the workspace's
    device).  ``fmt`` = ``"fasta"`` or ``"fastq"``, given by the caller: looking at the first byte would be a host wait, and
    the asynchronous FASTQ packer wants the text to start at its first ``@``.  Returns a ``FastxPipeline``; its
    ``finish()`` waits once."""
    import torch

    if fmt not in ("fasta", "fastq"):
        raise ValueError('fmt is "fasta" or "fastq"')
    ws = builder._ws()
    dev = f"cuda:{ws.device}"
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    if isinstance(text, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(text)).to(dev) if text.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        t = text
    n = int(t.numel())
    max_records = int(max_records)
    want_values = bool(values) or u128
    packed = torch.empty((n // 4 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    amb = torch.empty((n // 8 + 8 + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev) if with_amb else None
    starts = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    rec_pos = torch.zeros(max(max_records, 1), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    offsets = torch.zeros(max_records + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    per = 2 if u128 else 1
    vals = torch.zeros(per * max(n, 1), dtype=torch.int64, device=dev) if want_values else None
    torch.cuda.synchronize(ws.device)  # (the tensors above are torch's work on its own stream: before, not between)
    L = lib()
    head = (ws.h, _ptr(t) if n else None, n, _ptr(packed), packed.numel() // 4 * 4)
    tail = (_ptr(starts), _ptr(rec_pos), max_records, _ptr(counts))
    if with_amb:
        f = L.mm_fastq_pack_n_device_async if fmt == "fastq" else L.mm_fasta_pack_n_device_async
        _check(f(*head, _ptr(amb), amb.numel() // 4 * 4, *tail))
    else:
        f = L.mm_fastq_pack_device_async if fmt == "fastq" else L.mm_fasta_pack_device_async
        _check(f(*head, *tail))
    run_packed_reads_counts_device(builder, packed, starts, counts, pos, offsets, max_bases=n, max_records=max_records,
                                   amb=amb, sync=False, d_count=count)
    if want_values and max_records:
        values_reads_device(builder, packed, max_records, pos, offsets, read_starts=starts, n_pos_max=pos.numel(), out=vals,
                            u128=u128)
    return FastxPipeline(builder, ws, packed, amb, starts, rec_pos, counts, pos, offsets, count, vals, max_records)


# ---- FASTA / FASTQ files of any size through the device in chunks (mm_fastx_stream_*)
FASTX_AUTO, FASTX_FASTA, FASTX_FASTQ = 0, 1, 2
FASTX_SK, FASTX_SKIP_AMBIGUOUS, FASTX_VALUES_U64, FASTX_VALUES_U128, FASTX_LONG_RECORDS = 1, 2, 4, 8, 16
FASTX_ONE_MINIMIZER = 256  # (mm_fastx_stream_create only; the byte-text stream has FASTX_TEXT_ONE_MINIMIZER)
FASTX_BGZF_CRC = 1024  # (both streams: every block fed through feed_bgzf has its CRC32 verified)
FASTX_NEED_INPUT, FASTX_END = 1, 2
_FASTX_FORMATS = {"auto": FASTX_AUTO, "fasta": FASTX_FASTA, "fastq": FASTX_FASTQ}


class FastxStreamConfig(C.Structure):
    """``mm_fastx_stream_config_t``."""
    _fields_ = [("device", C.c_int), ("format", C.c_int), ("flags", C.c_uint32), ("slots", C.c_uint32),
                ("chunk_bytes", C.c_uint64), ("max_records", C.c_uint64), ("max_positions", C.c_uint64),
                ("first_byte", C.c_uint64)]


class _FastxBatchC(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_bases", C.c_uint64), ("n_positions", C.c_uint64),
                ("text_begin", C.c_uint64), ("text_end", C.c_uint64), ("rec_text_pos", C.c_void_p),
                ("rec_base", C.c_void_p), ("offsets", C.c_void_p), ("pos", C.c_void_p), ("sk", C.c_void_p),
                ("values", C.c_void_p)]


class _FastxPiecesC(C.Structure):
    _fields_ = [("first_continues", C.c_uint32), ("last_open", C.c_uint32), ("first_base", C.c_uint64),
                ("first_overlap", C.c_uint64)]


def _view(address, n, ctype, dtype):
    if not address or n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(address, C.POINTER(ctype)), shape=(n,))


class FastxBatch:
    """One batch of a ``FastxStream``: the records that lie whole inside one chunk.  ``rec_text_pos`` (absolute byte
    offsets of the records' '>' / '@'), ``text_begin`` / ``text_end`` (the absolute byte range the batch covers) are
    64-bit file offsets; ``rec_base`` and ``offsets`` (n_records + 1 each) start at 0 in every batch; ``pos`` (and
    ``sk``) are record-local; ``values``: uint64, two words {lo, hi} per value for u128, or None.  The arrays are VIEWS
    of the stream's page-locked buffers, valid until its following ``next()``; ``copy()`` detaches them.
    With ``long_records`` (``mm_fastx_pieces_t``): ``first_continues`` - record 0 continues the previous batch's last
    record (its ``pos`` / ``sk`` are record-global, its ``rec_text_pos`` the record's real '>', its first
    ``first_overlap`` bases repeat the previous piece and ``first_base`` is the record-global index of its first base);
    ``last_open`` - the last record goes on in the next batch.  ``fastx_join`` puts the pieces together."""

    def __init__(self, c: _FastxBatchC, u128: bool, views=True, pieces: "_FastxPiecesC" = None, extras=None, one_min=None):
        n, p = int(c.n_records), int(c.n_positions)
        self.u128 = u128
        self.first_continues = bool(pieces.first_continues) if pieces is not None else False
        self.last_open = bool(pieces.last_open) if pieces is not None else False
        self.first_base = int(pieces.first_base) if pieces is not None else 0
        self.first_overlap = int(pieces.first_overlap) if pieces is not None else 0
        self.n_records, self.n_bases, self.n_positions = n, int(c.n_bases), p
        self.text_begin, self.text_end = int(c.text_begin), int(c.text_end)
        self.rec_text_pos = _view(c.rec_text_pos, n, C.c_uint64, np.uint64)
        self.rec_base = _view(c.rec_base, n + 1, C.c_uint64, np.uint64)
        self.offsets = _view(c.offsets, n + 1, C.c_uint64, np.uint64)
        self.pos = _view(c.pos, p, C.c_uint32, np.uint32)
        self.sk = _view(c.sk, p, C.c_uint32, np.uint32) if c.sk else None
        self.values = _view(c.values, p * (2 if u128 else 1), C.c_uint64, np.uint64) if c.values else None
        # ``one_min``: one minimizer per record (a stream with ``one_minimizer``, else None); ``seq``: a
        # ``FastxTextStream``'s records' bytes back to back
        self.one_min = self.seq = None
        if one_min:
            self.one_min = _view(one_min, n, C.c_uint32, np.uint32)
        if extras is not None:
            self.one_min = _view(extras.one_min, n, C.c_uint32, np.uint32) if extras.one_min else None
            if extras.seq:
                self.seq = _view(extras.seq, int(self.rec_base[n]) if n else 0, C.c_uint8, np.uint8)

    def copy(self) -> "FastxBatch":
        for name in ("rec_text_pos", "rec_base", "offsets", "pos", "sk", "values", "one_min", "seq"):
            a = getattr(self, name)
            if a is not None:
                setattr(self, name, np.array(a, copy=True))
        return self


class FastxStream:
    """FASTA / FASTQ text of any size through the device in chunks (``mm_fastx_stream_*``): ``feed(bytes) -> consumed``
    (fewer than given only when no slot is free: call ``next()``), ``finish()``, ``next()`` -> a ``FastxBatch``, None
    when the stream wants input first (``MM_FASTX_NEED_INPUT``), ``StopIteration`` once everything is drained.
    ``chunk_bytes`` new bytes per chunk, ``max_records`` / ``max_positions`` per chunk (0: the worst case,
    2 * chunk_bytes positions), ``fmt`` "auto" / "fasta" / "fastq", ``values`` None / "u64" / "u128",
    ``super_kmers`` / ``skip_ambiguous`` as the one-shot calls have them, ``first_byte`` the absolute offset of the
    first byte fed, ``slots`` chunks in flight (0: the default of 3), ``long_records`` FASTA records longer than a chunk
    come in pieces (``MM_FASTX_LONG_RECORDS``; see ``FastxBatch`` and ``fastx_join``), ``one_minimizer`` one minimizer
    per read in ``FastxBatch.one_min`` (``MM_FASTX_ONE_MINIMIZER``: the builder's k and hasher, with ``skip_ambiguous``
    over clean k-mers only, ``NO_MINIMIZER`` for a read without one; refused with ``long_records``), ``bgzf_crc`` the
    CRC32 of every block fed through ``feed_bgzf`` is verified on the device (``MM_FASTX_BGZF_CRC``: a mismatch fails the
    stream with ``MM_ERR_FORMAT``, "CRC32" in its text; nothing changes for plain text).  Iterating yields the remaining batches (after
    ``finish()``).  A failing stream raises ``MinimizerError`` from every later call."""

    def __init__(self, builder: "Builder", chunk_bytes: int, max_records: int, fmt="auto", values=None, super_kmers=False,
                 skip_ambiguous=False, max_positions=0, first_byte=0, slots=0, device=None, long_records=False,
                 one_minimizer=False, bgzf_crc=False):
        if fmt not in _FASTX_FORMATS:
            raise ValueError('fmt is "auto", "fasta" or "fastq"')
        if values not in (None, "u64", "u128"):
            raise ValueError('values is None, "u64" or "u128"')
        flags = (FASTX_SK if super_kmers else 0) | (FASTX_SKIP_AMBIGUOUS if skip_ambiguous else 0)
        flags |= {None: 0, "u64": FASTX_VALUES_U64, "u128": FASTX_VALUES_U128}[values]
        flags |= FASTX_LONG_RECORDS if long_records else 0
        flags |= FASTX_ONE_MINIMIZER if one_minimizer else 0
        flags |= FASTX_BGZF_CRC if bgzf_crc else 0
        self.h = None
        self.long_records = bool(long_records)
        self.one_minimizer = bool(one_minimizer)
        self.u128 = values == "u128"
        self.builder = builder
        self._plan = builder.plan()  # (the stream keeps the plan's handle: it must outlive the stream)
        dev = builder._ws().device if device is None and builder._workspace is not None else (device or 0)
        self.config = FastxStreamConfig(int(dev), _FASTX_FORMATS[fmt], flags, int(slots), int(chunk_bytes), int(max_records),
                                        int(max_positions), int(first_byte))
        h = C.c_void_p()
        code = lib().mm_fastx_stream_create(C.byref(h), self._plan.h, C.byref(self.config))
        if code:
            self._raise(code)
        self.h = h
        self.finished = False

    @staticmethod
    def _raise(code):
        L = lib()
        raise MinimizerError(code, f"{L.mm_strerror(code).decode()}: {L.mm_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            lib().mm_fastx_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def feed(self, data) -> int:
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        took = C.c_uint64(0)
        code = lib().mm_fastx_stream_feed(self.h, buf.ctypes.data if buf.size else None, buf.size, C.byref(took))
        if code:
            self._raise(code)
        return int(took.value)

    def feed_bgzf(self, data) -> int:
        """``feed`` for BGZF-compressed bytes (``mm_fastx_stream_feed_bgzf``): whole blocks are taken, so the return
        value stops in front of an incomplete block (or where no slot is free: call ``next()``) and the caller feeds the
        rest again together with the bytes that follow."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        took = C.c_uint64(0)
        code = lib().mm_fastx_stream_feed_bgzf(self.h, buf.ctypes.data if buf.size else None, buf.size, C.byref(took))
        if code:
            self._raise(code)
        return int(took.value)

    def finish(self):
        code = lib().mm_fastx_stream_finish(self.h)
        if code:
            self._raise(code)
        self.finished = True

    def next(self):
        c = _FastxBatchC()
        code = lib().mm_fastx_stream_next(self.h, C.byref(c))
        if code == FASTX_NEED_INPUT:
            return None
        if code == FASTX_END:
            raise StopIteration
        if code:
            self._raise(code)
        pieces = None
        if self.long_records:
            pieces = _FastxPiecesC()
            _check(lib().mm_fastx_stream_pieces(self.h, C.byref(pieces)))
        one_min = None
        if self.one_minimizer:
            words, n = C.c_void_p(), C.c_uint64()
            _check(lib().mm_fastx_stream_one_minimizer(self.h, C.byref(words), C.byref(n)))
            one_min = words.value
        return FastxBatch(c, self.u128, pieces=pieces, one_min=one_min)

    def __iter__(self):
        return self

    def __next__(self):
        b = self.next()
        if b is None:
            raise RuntimeError("the stream wants input: feed() more bytes or finish() before iterating")
        return b


FASTX_TEXT_ONE_MINIMIZER, FASTX_TEXT_SEQ = 32, 64


class FastxTextStreamConfig(C.Structure):
    """``mm_fastx_text_stream_config_t``."""
    _fields_ = FastxStreamConfig._fields_ + [("values_encoding", C.c_int)]


class _FastxTextExtrasC(C.Structure):
    _fields_ = [("one_min", C.c_void_p), ("seq", C.c_void_p)]


class FastxTextStream(FastxStream):
    """A FASTA of BYTE TEXT (protein, any alphabet) of any size through the device in chunks
    (``mm_fastx_text_stream_create``; feed / finish / next as ``FastxStream``): ``builder`` a text builder, ``values``
    None / "u64" / "u128" with ``encoding`` ``TEXT_VALUES_BYTES`` (the default) / ``TEXT_VALUES_DNA``, ``super_kmers``,
    ``one_minimizer`` (``FastxBatch.one_min``: per record the leftmost position of the minimal ``hash & 0xffff0000`` with
    the builder's k and hasher, ``NO_MINIMIZER`` for a record shorter than k), ``seq`` (``FastxBatch.seq``: the records'
    bytes, record r = ``seq[rec_base[r]:rec_base[r + 1]]``).  ``fmt`` "auto" / "fasta": FASTQ raises ``MM_ERR_FORMAT``.
    ``n_bases`` counts characters.  ``bgzf_crc`` as ``FastxStream`` takes it."""

    def __init__(self, builder: "Builder", chunk_bytes: int, max_records: int, values=None, encoding=None, super_kmers=False,
                 one_minimizer=False, seq=False, fmt="auto", max_positions=0, first_byte=0, slots=0, device=None, bgzf_crc=False):
        if fmt not in _FASTX_FORMATS:
            raise ValueError('fmt is "auto" or "fasta"')
        if values not in (None, "u64", "u128"):
            raise ValueError('values is None, "u64" or "u128"')
        flags = (FASTX_SK if super_kmers else 0) | {None: 0, "u64": FASTX_VALUES_U64, "u128": FASTX_VALUES_U128}[values]
        flags |= (FASTX_TEXT_ONE_MINIMIZER if one_minimizer else 0) | (FASTX_TEXT_SEQ if seq else 0)
        flags |= FASTX_BGZF_CRC if bgzf_crc else 0
        self.h = None
        self.long_records = False
        self.one_minimizer = False  # (the text stream's words come with its extras)
        self.u128 = values == "u128"
        self.builder = builder
        self._plan = builder.text_plan()  # (the stream keeps the plan's handle: it must outlive the stream)
        dev = builder._ws().device if device is None and builder._workspace is not None else (device or 0)
        self.config = FastxTextStreamConfig(int(dev), _FASTX_FORMATS[fmt], flags, int(slots), int(chunk_bytes), int(max_records),
                                            int(max_positions), int(first_byte),
                                            TEXT_VALUES_BYTES if encoding is None else int(encoding))
        h = C.c_void_p()
        code = lib().mm_fastx_text_stream_create(C.byref(h), self._plan.h, C.byref(self.config))
        if code:
            self._raise(code)
        self.h = h
        self.finished = False

    def next(self):
        c = _FastxBatchC()
        code = lib().mm_fastx_stream_next(self.h, C.byref(c))
        if code == FASTX_NEED_INPUT:
            return None
        if code == FASTX_END:
            raise StopIteration
        if code:
            self._raise(code)
        extras = _FastxTextExtrasC()
        _check(lib().mm_fastx_text_stream_extras(self.h, C.byref(extras)))
        return FastxBatch(c, self.u128, extras=extras)


def fastx_cut(text: bytes, fmt: str, last: bool = False) -> dict:
    """The stream's cut rule on a host text (``mm_debug_fastx_cut``: the function the trim kernel calls, no GPU)."""
    buf = np.frombuffer(text, dtype=np.uint8)
    out = (C.c_uint64 * 3)()
    _check(lib().mm_debug_fastx_cut(buf.ctypes.data if buf.size else None, buf.size, _FASTX_FORMATS[fmt], int(last), out))
    return {"cut": int(out[0]), "kept": int(out[1]), "dropped": int(out[2])}


def fastx_split(text: bytes, l: int, last: bool = False) -> dict:
    """The stream's split rule for FASTA records longer than a chunk, on a host text (``mm_debug_fastx_split``, no GPU):
    ``l`` = k + w - 1."""
    buf = np.frombuffer(text, dtype=np.uint8)
    out = (C.c_uint64 * 4)()
    _check(lib().mm_debug_fastx_split(buf.ctypes.data if buf.size else None, buf.size, int(l), int(last), out))
    return {"cut": int(out[0]), "T": int(out[1]), "open": int(out[2]), "overlap": int(out[3])}


def fastx_join(batches):
    """Generator over the RECORDS of a ``long_records`` stream's batches, pieces joined: per record
    ``(rec_text_pos, n_bases, pos, sk, values)`` - ``pos`` (uint32, record-global), ``sk`` and ``values`` (None when the
    stream has none; u128 values keep two words per value) are the concatenation of the pieces' slices."""
    cat = lambda xs, t: np.concatenate(xs) if xs else np.zeros(0, t)  # noqa: E731
    held = None  # [rec_text_pos, n_bases, [pos], [sk] or None, [values] or None]

    def done(h):
        return (h[0], h[1], cat(h[2], np.uint32), None if h[3] is None else cat(h[3], np.uint32),
                None if h[4] is None else cat(h[4], np.uint64))

    for b in batches:
        per = 2 if b.u128 else 1
        for r in range(b.n_records):
            o0, o1 = int(b.offsets[r]), int(b.offsets[r + 1])
            n = int(b.rec_base[r + 1]) - int(b.rec_base[r])
            part = (np.array(b.pos[o0:o1], copy=True), None if b.sk is None else np.array(b.sk[o0:o1], copy=True),
                    None if b.values is None else np.array(b.values[o0 * per:o1 * per], copy=True))
            if r == 0 and b.first_continues:
                if held is None or held[0] != int(b.rec_text_pos[0]):
                    raise ValueError("fastx_join: a continuing piece without the piece before it")
                held[1] += n - b.first_overlap
            else:
                if held is not None:
                    yield done(held)
                held = [int(b.rec_text_pos[r]), n, [], None if part[1] is None else [], None if part[2] is None else []]
            held[2].append(part[0])
            if part[1] is not None:
                held[3].append(part[1])
            if part[2] is not None:
                held[4].append(part[2])
            if not (r == b.n_records - 1 and b.last_open):
                yield done(held)
                held = None
    if held is not None:
        yield done(held)


def is_bgzf(head) -> bool:
    """Do these first bytes of a file begin a BGZF block (gzip magic ``1f 8b``, deflate, FLG bit 2: an extra field)?"""
    h = bytes(head[:4])
    return len(h) == 4 and h[:3] == b"\x1f\x8b\x08" and bool(h[3] & 4)


def _check_bgzf(code: int):
    if code:
        FastxStream._raise(code)  # (with mm_last_error(): it names the block, or plain gzip)


class BgzfBlock(C.Structure):
    _fields_ = [("comp_off", C.c_uint64), ("comp_len", C.c_uint32), ("isize", C.c_uint32), ("out_off", C.c_uint64)]


BGZF_BLOCK_DTYPE = np.dtype([("comp_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("out_off", "<u8")])


def crc32(data) -> int:
    """``mm_debug_crc32`` (no device): the gzip CRC32 of ``data`` (``zlib.crc32``) by the arithmetic the verify kernel runs."""
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    out = C.c_uint32(0)
    _check_bgzf(lib().mm_debug_crc32(buf.ctypes.data if buf.size else None, buf.size, C.byref(out)))
    return int(out.value)


def bgzf_scan(data, max_blocks=None, max_out_bytes=U64_MAX, crc=False) -> dict:
    """``mm_bgzf_scan_host`` (no device): the block table of the BGZF bytes ``data`` as a structured array
    (``BGZF_BLOCK_DTYPE``), ``consumed`` (bytes of whole blocks taken) and ``out_bytes`` (their text's size).
    ``max_blocks`` None: as many as ``data`` can hold.  ``crc``: also ``"crc"``, the CRC32 of every listed block's gzip
    trailer as a uint32 array (``mm_bgzf_scan_crc_host``)."""
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    cap = buf.size // 26 + 1 if max_blocks is None else int(max_blocks)
    blocks = np.zeros(cap, BGZF_BLOCK_DTYPE)
    n, used, out = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if crc:
        crcs = np.zeros(cap, np.uint32)
        _check_bgzf(lib().mm_bgzf_scan_crc_host(buf.ctypes.data if buf.size else None, buf.size, cap, int(max_out_bytes),
                                           blocks.ctypes.data if cap else None, C.byref(n), C.byref(used), C.byref(out),
                                           crcs.ctypes.data if cap else None))
        return {"blocks": blocks[:int(n.value)], "consumed": int(used.value), "out_bytes": int(out.value), "crc": crcs[:int(n.value)]}
    _check_bgzf(lib().mm_bgzf_scan_host(buf.ctypes.data if buf.size else None, buf.size, cap, int(max_out_bytes),
                                   blocks.ctypes.data if cap else None, C.byref(n), C.byref(used), C.byref(out)))
    return {"blocks": blocks[:int(n.value)], "consumed": int(used.value), "out_bytes": int(out.value)}


def debug_bgzf_inflate(payload, isize: int) -> bytes:
    """``mm_debug_bgzf_inflate`` (no device): one BGZF block's deflate payload inflated by the decoder the kernel runs."""
    buf = np.frombuffer(payload, dtype=np.uint8)
    out = np.zeros(max(int(isize), 1), np.uint8)
    _check_bgzf(lib().mm_debug_bgzf_inflate(buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, int(isize)))
    return out[:int(isize)].tobytes()


def bgzf_inflate_device(d_comp, blocks, d_out, d_status=None, ws=None):
    """``mm_bgzf_inflate_device_async``: one launch over the table ``blocks`` (a uint8 device tensor holding
    ``BGZF_BLOCK_DTYPE`` entries, or a host array of them, which is uploaded) - payloads in the uint8 device tensor
    ``d_comp``, text into the uint8 device tensor ``d_out``, one word per block into the int32 / uint32 tensor
    ``d_status`` when given.  Queued on the workspace's stream; ``ws.check()`` judges the launch."""
    import torch

    ws = ws or default_workspace(d_out.device.index or 0)
    if isinstance(blocks, np.ndarray):
        host = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        d_blocks = torch.from_numpy(host.view(np.uint8).copy()).to(d_out.device)
    else:
        d_blocks = blocks
    n = d_blocks.numel() * d_blocks.element_size() // BGZF_BLOCK_DTYPE.itemsize
    _check_bgzf(lib().mm_bgzf_inflate_device_async(ws.h, _ptr(d_comp), d_comp.numel(), _ptr(d_blocks), n, _ptr(d_out), d_out.numel(),
                                              _ptr(d_status) if d_status is not None else None))
    ws._keep_bgzf = (d_comp, d_blocks, d_out, d_status)  # (alive until the queued launch has run)
    return n


def bgzf_crc32_device(d_text, blocks, expect=None, d_status=None, ws=None):
    """``mm_bgzf_crc32_device_async``: one launch over the table ``blocks`` (as ``bgzf_inflate_device`` takes it) and the
    text in the uint8 device tensor ``d_text``; returns the int32 device tensor of the blocks' CRC32s (their bits are the
    uint32 values).  ``expect`` (the trailers' CRC32s: a host array, which is uploaded, or an int32 device tensor): a block
    that differs gets 15 in ``d_status`` and ``ws.check()`` raises ``MM_ERR_FORMAT`` ("CRC32"); a block whose ``d_status``
    word is already non-zero is skipped.  ``d_status`` None with ``expect``: a zeroed array of the call's own (kept as
    ``ws._keep_bgzf_crc[-1]``).  Queued on the workspace's stream."""
    import torch

    ws = ws or default_workspace(d_text.device.index or 0)
    if isinstance(blocks, np.ndarray):
        host = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        d_blocks = torch.from_numpy(host.view(np.uint8).copy()).to(d_text.device)
    else:
        d_blocks = blocks
    n = d_blocks.numel() * d_blocks.element_size() // BGZF_BLOCK_DTYPE.itemsize
    d_expect = None
    if expect is not None:
        if isinstance(expect, torch.Tensor):
            d_expect = expect
        else:
            d_expect = torch.from_numpy(np.ascontiguousarray(expect, dtype=np.uint32).view(np.int32).copy()).to(d_text.device)
        if d_status is None:
            d_status = torch.zeros(max(n, 1), dtype=torch.int32, device=d_text.device)
    d_crc = torch.zeros(max(n, 1), dtype=torch.int32, device=d_text.device)
    _check_bgzf(lib().mm_bgzf_crc32_device_async(ws.h, _ptr(d_text), d_text.numel(), _ptr(d_blocks), n,
                                            _ptr(d_expect) if d_expect is not None else None, _ptr(d_crc),
                                            _ptr(d_status) if d_status is not None else None))
    ws._keep_bgzf_crc = (d_text, d_blocks, d_expect, d_crc, d_status)  # (alive until the queued launch has run)
    return d_crc[:n]


def bgzf_inflate_host(data, ws=None, device: int = 0, verify=False) -> bytes:
    """``mm_bgzf_inflate_host``: a whole BGZF file in host memory inflated on the device; the text as bytes.  ``verify``:
    ``mm_bgzf_inflate_verify_host``, every block's CRC32 checked on the device (``MM_ERR_FORMAT``, "CRC32", on a mismatch)."""
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    ws = ws or default_workspace(device)
    cap = bgzf_scan(buf)["out_bytes"]
    out = np.zeros(max(cap, 1), np.uint8)
    n = C.c_uint64(0)
    _check_bgzf((lib().mm_bgzf_inflate_verify_host if verify else lib().mm_bgzf_inflate_host)(ws.h, buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, cap, C.byref(n)))
    return out[:int(n.value)].tobytes()


def _stream_batches(st, source, read_bytes, bgzf=None):
    """The feed / next loop of ``stream_fastx`` and ``stream_fasta_text`` over an open stream ``st``: numpy COPIES.
    ``bgzf``: the source holds BGZF blocks (None: decided by its first bytes, ``is_bgzf``)."""
    import os

    def pieces():
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                while True:
                    b = f.read(read_bytes)
                    if not b:
                        return
                    yield b
        elif hasattr(source, "read"):
            while True:
                b = source.read(read_bytes)
                if not b:
                    return
                yield b
        else:
            yield from source

    def push(view):
        """feeds ``view``, yields the batches the stream hands out meanwhile, returns the bytes taken: all of them, or with
        BGZF everything in front of an incomplete block (no byte taken twice in a row although ``next()``, which frees the
        slot of the batch handed out before, wanted input in between)"""
        done, stalled = 0, False
        while done < len(view):
            took = st.feed_bgzf(view[done:]) if bgzf else st.feed(view[done:])
            done += took
            stalled = stalled and took == 0
            if done < len(view):
                b = st.next()
                if b is not None:
                    yield b.copy()
                elif bgzf and took == 0:
                    if stalled:
                        break
                    stalled = True
        return done

    with st:
        held = b""  # (BGZF: the front of a block whose rest has not been read yet)
        for piece in pieces():
            if bgzf is None:
                held += bytes(piece)
                if len(held) < 4:
                    continue
                bgzf = is_bgzf(held)
                piece, held = held, b""
            if bgzf:
                piece = held + bytes(piece)
            view = memoryview(piece)
            done = yield from push(view)
            held = bytes(view[done:])
        if held:
            # (a source shorter than 4 bytes is plain text; what is left of a BGZF source is a truncated block, which the
            # stream names at finish)
            yield from push(memoryview(held))
        st.finish()
        for b in st:
            yield b.copy()


def stream_fastx(builder: "Builder", source, chunk_bytes: int = 64 << 20, max_records: int = 1 << 20, read_bytes: int = 8 << 20,
                 bgzf=None, **options):
    """Generator over the batches (``FastxBatch``, numpy COPIES) of a FASTA / FASTQ ``source``: a path, a binary file
    object or an iterable of bytes, of any size.  ``options`` as ``FastxStream`` takes them; ``read_bytes``: how much a
    path or file object is read at a time.  ``bgzf``: the source is BGZF-compressed (bgzip / htslib ``.gz``) and is
    inflated on the device (``FastxStream.feed_bgzf``); None decides by the source's first bytes (``is_bgzf``), True and
    False force the choice.  Plain gzip is refused (``MM_ERR_FORMAT``).  ``bgzf_crc=True`` (an option of ``FastxStream``)
    verifies every BGZF block's CRC32 on the device."""
    yield from _stream_batches(FastxStream(builder, chunk_bytes, max_records, **options), source, read_bytes, bgzf)


def stream_fasta_text(builder: "Builder", source, chunk_bytes: int = 64 << 20, max_records: int = 1 << 20,
                      read_bytes: int = 8 << 20, bgzf=None, **options):
    """``stream_fastx`` for a FASTA of byte text (protein): generator over the batches (``FastxBatch`` with ``one_min`` /
    ``seq``, numpy COPIES) of a ``FastxTextStream`` over ``source``; ``options`` as ``FastxTextStream`` takes them, ``bgzf``
    as ``stream_fastx`` takes it."""
    yield from _stream_batches(FastxTextStream(builder, chunk_bytes, max_records, **options), source, read_bytes, bgzf)


def run_packed_reads_device(builder: "Builder", records: FastaRecords, out_pos, out_offsets, out_sk=None, max_read_len=None):
    """All records of a packed FASTQ / FASTA (``fasta_pack_device``) as READS: one launch of the reads-mode kernel over
    reads of any lengths packed back to back (``mm_run_packed_reads_device``); read-local positions, ``out_offsets``
    (int64 device tensor, n + 1) delimits the reads.  Returns the number of positions."""
    import torch
    n = len(records)
    starts = torch.from_numpy(np.ascontiguousarray(records.base, dtype=np.uint64).view(np.int64)).to(out_pos.device)
    lens = records.lengths()
    mx = max(lens) if lens else 0
    if max_read_len is None:
        max_read_len = mx
    cnt = C.c_uint64()
    ws = builder._ws()
    _check(lib().mm_run_packed_reads_device(builder.plan().h, ws.h, C.c_void_p(records.packed.data_ptr()),
                                            int(records.packed.numel()), 0, n, C.c_void_p(starts.data_ptr()),
                                            int(records.base[-1]) if n else 0, int(max_read_len),
                                            C.c_void_p(out_pos.data_ptr()),
                                            C.c_void_p(out_sk.data_ptr()) if out_sk is not None else None,
                                            int(out_pos.numel()), C.c_void_p(out_offsets.data_ptr()), C.byref(cnt)))
    return int(cnt.value)


def run_packed_reads_skip_ambiguous_device(builder: "Builder", records: FastaRecords, out_pos, out_offsets, max_read_len=None):
    """``run_packed_reads_device`` over the records of ``fasta_pack_n_device`` with ``Builder::run_skip_ambiguous_windows``
    per record (``mm_run_packed_reads_skip_ambiguous_device``): windows that hold an ambiguous base select nothing.
    Canonical builders only, no super-k-mer indices.  Returns the number of positions."""
    import torch
    if records.amb is None:
        raise ValueError("records without ambiguity bits: pack them with fasta_pack_n_device")
    n = len(records)
    starts = torch.from_numpy(np.ascontiguousarray(records.base, dtype=np.uint64).view(np.int64)).to(out_pos.device)
    lens = records.lengths()
    if max_read_len is None:
        max_read_len = max(lens) if lens else 0
    cnt = C.c_uint64()
    ws = builder._ws()
    cap = int(out_pos.numel())
    code = lib().mm_run_packed_reads_skip_ambiguous_device(
        builder.plan().h, ws.h, C.c_void_p(records.packed.data_ptr()), int(records.packed.numel()), 0,
        C.c_void_p(records.amb.data_ptr()), int(records.amb.numel()), 0, n, C.c_void_p(starts.data_ptr()),
        int(records.base[-1]) if n else 0, int(max_read_len), C.c_void_p(out_pos.data_ptr()), cap,
        C.c_void_p(out_offsets.data_ptr()), C.byref(cnt))
    if code == ERR["CAPACITY"]:
        raise MinimizerError(code, f"output capacity {cap} < {cnt.value}")
    _check(code)
    return int(cnt.value)


def run_reads_skip_ambiguous_host(builder: "Builder", reads):
    """Many short host reads with ``N`` in ONE call (``mm_run_packed_reads_skip_ambiguous_host``): ``reads`` = list of
    ASCII ``bytes``; returns (positions, offsets) - read r's read-local positions are
    ``positions[offsets[r]:offsets[r + 1]]``, what ``run_skip_ambiguous_windows`` of ``PackedNSeqVec.from_ascii(read)``
    returns.  Canonical builders only."""
    arrs = [np.frombuffer(bytes(s), dtype=np.uint8) for s in reads]
    lens = [len(a) for a in arrs]
    starts = np.zeros(len(lens) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(starts[-1])
    flat = np.concatenate(arrs) if total else np.zeros(0, dtype=np.uint8)
    q = np.concatenate([(flat >> 1) & 3, np.zeros((-total) % 4, dtype=np.uint8)]).reshape(-1, 4)
    packed = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8) if total else np.zeros(1, dtype=np.uint8)
    up = flat & 0xDF
    bad = ~((up == 65) | (up == 67) | (up == 71) | (up == 84))
    amb = np.packbits(bad, bitorder="little") if total else np.zeros(1, dtype=np.uint8)
    cap = max(1, total)
    pos = np.empty(cap, dtype=np.uint32)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    cnt = C.c_uint64()
    ws = builder._ws()
    _check(lib().mm_run_packed_reads_skip_ambiguous_host(builder.plan().h, ws.h, _p(packed, C.c_uint8), _p(amb, C.c_uint8),
                                                         len(lens), _p(starts, C.c_uint64), max(lens) if lens else 0,
                                                         _p(pos, C.c_uint32), cap, _p(offs, C.c_uint64), C.byref(cnt)))
    n = int(cnt.value)
    return pos[:n], [int(o) for o in offs]


def _value_len(builder: "Builder") -> int:
    """What ``Output.values_u64`` reads per position: k for minimizers, k + w - 1 for syncmers."""
    return builder.k if builder.mode == MM_MINIMIZERS else builder.k + builder.w - 1


def values_read_of(offsets, idx) -> np.ndarray:
    """The reads values kernels' lookup on the host (``mm_debug_values_read_of``, no GPU): for every value index in
    ``idx`` the read r with ``offsets[r] <= idx < offsets[r + 1]`` = ``np.searchsorted(offsets, idx, 'right') - 1``."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    out = np.empty(len(idx), dtype=np.int64)
    _check(lib().mm_debug_values_read_of(_p(offsets, C.c_uint64), len(offsets) - 1, _p(idx, C.c_uint64), len(idx),
                                         out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def values_reads_lds_stage() -> int:
    """Offsets a workgroup of the reads values kernels stages in LDS (``mm_values_reads_lds_stage``); a workgroup whose
    values span more reads searches global memory."""
    return int(lib().mm_values_reads_lds_stage())


def values_batch_lds_stage() -> int:
    """Entries (an offset and a sequence descriptor each) a workgroup of the batch values kernels stages in LDS
    (``mm_values_batch_lds_stage``); a workgroup whose values span more sequences searches global memory."""
    return int(lib().mm_values_batch_lds_stage())


def values_batch_view(address: int, packed_bytes: int, base_offset: int = 0) -> dict:
    """The view the batch values kernels' host side derives for one sequence (``mm_debug_values_batch_view``, no GPU)."""
    out = (C.c_uint64 * 6)()
    _check(lib().mm_debug_values_batch_view(int(address), int(packed_bytes), int(base_offset), out))
    return dict(zip(("address", "byte_lo", "byte_hi", "q_lo", "q_hi", "base0"), (int(x) for x in out)))


def _values_out(d_pos, out, count: int, u128: bool, count_is: str):
    """``out`` of the device values wrappers, for ``count`` values: the caller's tensor checked for its size, or a new
    zero-filled one (waited for).  ``d_pos`` must hold ``count`` positions; ``count_is`` names the count in the message."""
    import torch
    per = 2 if u128 else 1
    if out is None:
        out = torch.zeros(per * count, dtype=torch.int64, device=d_pos.device)
        torch.cuda.synchronize(d_pos.device)
    elif out.numel() < per * count:
        raise ValueError(f"out holds {out.numel()} words, {per * count} needed")
    if d_pos.numel() < count:
        raise ValueError(f"d_pos holds {d_pos.numel()} positions, {count_is} {count}")
    return out


def values_batch_device(builder: "Builder", d_seqs, n_bases, d_pos, offsets, base_offsets=None, u128=False, out=None):
    """K-mer values of EVERY sequence of a device batch in one launch (``mm_values_u64_batch_device_async`` /
    ``mm_values_u128_batch_device_async``): ``d_seqs`` (list of torch uint8 CUDA tensors; ``None`` for a sequence without
    values), ``n_bases`` and ``base_offsets`` as ``run_batch_device`` took them, ``d_pos`` the positions it wrote (int32
    tensor) and ``offsets`` the n_seqs + 1 offsets it returned.  ``len`` and ``canonical`` come from the builder like
    ``Output.values_u64`` takes them.  Fills ``out`` (int64 tensor of ``offsets[-1]`` words, twice that for ``u128``:
    {lo, hi}) or returns a new zero-filled one; the call is asynchronous on the builder's workspace (``Workspace.sync``)."""
    n = len(d_seqs)
    offsets = [int(o) for o in offsets]
    if len(offsets) != n + 1 or len(n_bases) != n or (base_offsets is not None and len(base_offsets) != n):
        raise ValueError(f"{n} sequences need {n} lengths (and base offsets) and {n + 1} offsets")
    out = _values_out(d_pos, out, offsets[-1], u128, "offsets end at")
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() if t is not None and t.numel() else None for t in d_seqs])
    nbytes = (C.c_uint64 * max(n, 1))(*[int(t.numel()) if t is not None else 0 for t in d_seqs])
    lens = (C.c_uint64 * max(n, 1))(*[int(x) for x in n_bases])
    bases = (C.c_uint64 * max(n, 1))(*[int(x) for x in base_offsets]) if base_offsets is not None else None
    offs = (C.c_uint64 * (n + 1))(*offsets)
    f = lib().mm_values_u128_batch_device_async if u128 else lib().mm_values_u64_batch_device_async
    _check(f(builder._ws().h, n, ptrs, nbytes, bases, lens, _value_len(builder), int(builder.canonical),
             C.c_void_p(d_pos.data_ptr()), offs, C.c_void_p(out.data_ptr())))
    return out


def values_reads_device(builder: "Builder", d_packed, n_reads, d_pos, d_out_offsets, read_starts=None, read_stride=0,
                        base_offset=0, n_pos_max=None, out=None, u128=False):
    """K-mer values of EVERY read's positions in one launch (``mm_values_u64_reads_device_async`` /
    ``mm_values_u128_reads_device_async``): ``d_packed`` the packed uint8 CUDA tensor the reads run took, ``d_pos`` its
    read-local positions (int32 tensor), ``d_out_offsets`` its n_reads + 1 offsets (int64 tensor), and the same layout -
    ``read_starts`` (int64 tensor of n_reads + 1 starts: reads back to back) or ``read_stride``.  ``len`` and
    ``canonical`` come from the builder like ``Output.values_u64`` takes them.  The true count is read on the device:
    nothing waits for the host, values at or past it stay as they were.  Fills ``out`` (int64 tensor of ``n_pos_max``
    words, twice that for ``u128``: {lo, hi}) or returns a new zero-filled one; the call is asynchronous on the
    builder's workspace (``Workspace.sync``)."""
    if n_pos_max is None:
        n_pos_max = int(d_pos.numel())
    out = _values_out(d_pos, out, n_pos_max, u128, "n_pos_max is")
    f = lib().mm_values_u128_reads_device_async if u128 else lib().mm_values_u64_reads_device_async
    _check(f(builder._ws().h, C.c_void_p(d_packed.data_ptr()), int(d_packed.numel()), int(base_offset), int(n_reads),
             C.c_void_p(read_starts.data_ptr()) if read_starts is not None else None, int(read_stride),
             _value_len(builder), int(builder.canonical), C.c_void_p(d_pos.data_ptr()),
             C.c_void_p(d_out_offsets.data_ptr()), int(n_pos_max), C.c_void_p(out.data_ptr())))
    return out


def values_text_lds_stage() -> int:
    """Offsets a workgroup of the text batch values kernels stages in LDS (``mm_values_text_lds_stage``); a workgroup whose
    values span more records searches global memory."""
    return int(lib().mm_values_text_lds_stage())


def debug_values_text(text, encoding, length, canonical=False, u128=False, abs_pos=(), address_shift=0):
    """The text values kernels' arithmetic for one value, on the host (``mm_debug_values_text``, no GPU): the values at
    the absolute positions ``abs_pos`` of ``text``, whose first byte is placed ``address_shift`` (0..3) bytes past a
    4-byte boundary.  Returns a uint64 array, or a list of Python ints for ``u128``."""
    text = _text_array(text)
    buf = np.zeros(len(text) + 8, dtype=np.uint8)
    at = (-buf.ctypes.data) % 4 + int(address_shift)
    buf[at:at + len(text)] = text
    pos = np.ascontiguousarray(abs_pos, dtype=np.uint64)
    per = 2 if u128 else 1
    out = np.zeros(max(1, per * len(pos)), dtype=np.uint64)
    _check(lib().mm_debug_values_text(C.c_void_p(buf.ctypes.data + at), len(text), int(encoding), int(length),
                                      int(canonical), int(u128), _p(pos, C.c_uint64), len(pos), _p(out, C.c_uint64)))
    if u128:
        return _u128_list(out, len(pos))
    return out[:len(pos)]


def values_text_device(builder: "Builder", d_text, n, d_pos, n_pos, encoding, u128=False, out=None):
    """K-mer values of device-resident byte text (``mm_values_u64_text_device_async`` /
    ``mm_values_u128_text_device_async``): ``d_text`` the uint8 CUDA tensor a text run took (``n`` characters; every byte
    of the tensor is readable, nothing past it is), ``d_pos`` the ABSOLUTE positions it wrote (int32 tensor, ``n_pos`` of
    them).  ``encoding``: ``TEXT_VALUES_BYTES`` (``&[u8]``, 8 bits per character) or ``TEXT_VALUES_DNA`` (``AsciiSeq``, 2
    bits).  ``len`` and ``canonical`` come from the builder like ``Output.values_u64`` takes them.  Fills ``out`` (int64
    tensor of ``n_pos`` words, twice that for ``u128``: {lo, hi}) or returns a new zero-filled one; the call is
    asynchronous on the builder's workspace (``Workspace.sync``)."""
    n_pos = int(n_pos)
    out = _values_out(d_pos, out, n_pos, u128, "n_pos is")
    f = lib().mm_values_u128_text_device_async if u128 else lib().mm_values_u64_text_device_async
    _check(f(builder._ws().h, C.c_void_p(d_text.data_ptr()), int(d_text.numel()), int(n), int(encoding),
             _value_len(builder), int(builder.canonical), C.c_void_p(d_pos.data_ptr()), n_pos,
             C.c_void_p(out.data_ptr())))
    return out


def values_text_batch_device(builder: "Builder", d_text, d_starts, n_chars, d_pos, d_out_offsets, n_pos_max, encoding,
                             u128=False, out=None):
    """K-mer values of EVERY record of a device text batch in one launch (``mm_values_u64_text_batch_device_async`` /
    ``mm_values_u128_text_batch_device_async``): ``d_text`` / ``d_starts`` / ``n_chars`` as ``run_text_batch_device`` took
    them, ``d_pos`` the record-local positions and ``d_out_offsets`` the n + 1 offsets it wrote.  The true count is read
    on the device: nothing waits for the host, values at or past it (or past ``n_pos_max``) stay as they were.
    ``encoding`` / ``u128`` / ``out`` as for ``values_text_device`` (``out`` holds ``n_pos_max`` values)."""
    n_rec = d_starts.numel() - 1
    if n_rec < 0 or d_out_offsets.numel() != n_rec + 1:
        raise ValueError("d_starts and d_out_offsets hold n + 1 entries each")
    n_pos_max = int(n_pos_max)
    out = _values_out(d_pos, out, n_pos_max, u128, "n_pos_max is")
    f = lib().mm_values_u128_text_batch_device_async if u128 else lib().mm_values_u64_text_batch_device_async
    _check(f(builder._ws().h, C.c_void_p(d_text.data_ptr()), int(d_text.numel()), n_rec, C.c_void_p(d_starts.data_ptr()),
             int(n_chars), int(encoding), _value_len(builder), int(builder.canonical), C.c_void_p(d_pos.data_ptr()),
             C.c_void_p(d_out_offsets.data_ptr()), n_pos_max, C.c_void_p(out.data_ptr())))
    return out


def values_text_batch_host(builder: "Builder", records, pos, offsets, encoding, u128=False):
    """K-mer values of many host records of byte text in ONE call (``mm_values_u64_text_batch_host`` /
    ``mm_values_u128_text_batch_host``): ``records`` as ``run_text_batch_host`` takes them, ``pos`` / ``offsets`` as it
    returns them.  Returns a uint64 array (one value per position), or a list of Python ints for ``u128`` - record r's
    values are ``[offsets[r]:offsets[r + 1]]``, what ``Output.values_u64`` of ``Builder.run(record)`` returns."""
    text, starts = _text_records(records)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(starts):
        raise ValueError(f"{len(starts) - 1} records need {len(starts)} offsets, not {len(offsets)}")
    n = int(offsets[-1]) if len(offsets) else 0
    if len(pos) < n:
        raise ValueError(f"offsets end at {n}, pos holds {len(pos)}")
    per = 2 if u128 else 1
    vals = np.zeros(max(1, per * n), dtype=np.uint64)
    f = lib().mm_values_u128_text_batch_host if u128 else lib().mm_values_u64_text_batch_host
    _check(f(builder._ws().h, _p(text, C.c_uint8), len(starts) - 1, _p(starts, C.c_uint64), int(encoding),
             _value_len(builder), int(builder.canonical), _p(pos, C.c_uint32) if len(pos) else None,
             _p(offsets, C.c_uint64), _p(vals, C.c_uint64)))
    if u128:
        return _u128_list(vals, n)
    return vals[:n]


def _pack_reads(reads):
    """Reads (``PackedSeq`` views / ASCII ``bytes``) -> (packed bytes, starts): the reads packed back to back."""
    codes = []
    for s in reads:
        if isinstance(s, (bytes, bytearray)):
            codes.append((np.frombuffer(bytes(s), dtype=np.uint8) >> 1) & 3)
        else:  # PackedSeq view
            codes.append(s.codes())
    starts = np.zeros(len(codes) + 1, dtype=np.uint64)
    starts[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
    total = int(starts[-1])
    if not total:
        return np.zeros(1, dtype=np.uint8), starts
    q = np.concatenate(codes + [np.zeros((-total) % 4, dtype=np.uint8)]).astype(np.uint8).reshape(-1, 4)
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8), starts


def values_reads_host(builder: "Builder", reads, pos, offsets, u128=False):
    """K-mer values of many host reads in ONE call (``mm_values_u64_reads_host`` / ``mm_values_u128_reads_host``):
    ``reads`` as ``run_reads_host`` takes them, ``pos`` / ``offsets`` as it returns them.  Returns a uint64 array (one
    value per position), or a list of Python ints for ``u128`` - read r's values are ``[offsets[r]:offsets[r + 1]]``,
    what ``Output.values_u64`` of ``Builder.run(read)`` returns."""
    packed, starts = _pack_reads(reads)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(starts):
        raise ValueError(f"{len(starts) - 1} reads need {len(starts)} offsets, not {len(offsets)}")
    n = int(offsets[-1]) if len(offsets) else 0
    if len(pos) < n:
        raise ValueError(f"offsets end at {n}, pos holds {len(pos)}")
    per = 2 if u128 else 1
    vals = np.zeros(max(1, per * n), dtype=np.uint64)
    f = lib().mm_values_u128_reads_host if u128 else lib().mm_values_u64_reads_host
    _check(f(builder._ws().h, _p(packed, C.c_uint8), len(packed), 0, len(starts) - 1, _p(starts, C.c_uint64), 0,
             _value_len(builder), int(builder.canonical), _p(pos, C.c_uint32) if len(pos) else None,
             _p(offsets, C.c_uint64), _p(vals, C.c_uint64)))
    if u128:
        return _u128_list(vals, n)
    return vals[:n]


# ------------------------------------------------------------------ one minimizer per record (src/minimizers.rs:22-28)

NO_MINIMIZER = 0xFFFFFFFF  # MM_NO_MINIMIZER: the record is shorter than k


def one_minimizer_tile() -> int:
    """K-mer start positions one workgroup of the one-minimizer kernel covers (``mm_one_minimizer_tile``)."""
    return int(lib().mm_one_minimizer_tile())


def _vp_of(a):
    """void * of a numpy array or a torch tensor (None stays None)."""
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def debug_one_minimizer_reads(hasher: Hasher, k: int, packed, n_reads: int, read_starts=None, read_stride=0, read_len=0,
                              base_offset=0, tile=0, amb=None, amb_offset=0) -> np.ndarray:
    """The one-minimizer kernel's per-tile function on the host, tile after tile (``mm_debug_one_minimizer_reads``, no
    GPU): ``packed`` a uint8 array, the layout as ``one_minimizer_reads_device`` takes it (``read_starts``: uint64 array
    of n + 1), ``tile`` overrides the tile size (0: the kernel's).  With ``amb`` (a uint8 array of ambiguity bits, base j
    = bit ``amb_offset + j``) the skip-ambiguous form (``mm_debug_one_minimizer_reads_skip_ambiguous``).  Returns
    ``np.uint32[n_reads]``."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    starts = np.ascontiguousarray(read_starts, dtype=np.uint64) if read_starts is not None else None
    out = np.zeros(max(1, int(n_reads)), dtype=np.uint32)
    if amb is not None:
        amb = np.ascontiguousarray(amb, dtype=np.uint8)
        _check(lib().mm_debug_one_minimizer_reads_skip_ambiguous(
            C.byref(hasher), int(k), _vp_of(packed), len(packed), int(base_offset), _vp_of(amb), len(amb), int(amb_offset),
            int(n_reads), _vp_of(starts), int(read_stride), int(read_len), int(tile), _vp_of(out)))
        return out[:int(n_reads)]
    _check(lib().mm_debug_one_minimizer_reads(C.byref(hasher), int(k), _vp_of(packed), len(packed), int(base_offset),
                                              int(n_reads), _vp_of(starts), int(read_stride), int(read_len), int(tile),
                                              _vp_of(out)))
    return out[:int(n_reads)]


def debug_one_minimizer_text_batch(hasher: TextHasher, k: int, text, starts, tile=0) -> np.ndarray:
    """The same for records of byte text (``mm_debug_one_minimizer_text_batch``, no GPU): ``text`` a uint8 array,
    ``starts`` the n + 1 record starts."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.uint64)
    n = len(starts) - 1
    out = np.zeros(max(1, n), dtype=np.uint32)
    _check(lib().mm_debug_one_minimizer_text_batch(C.byref(hasher), int(k), _vp_of(text), len(text), n, _vp_of(starts),
                                                   int(tile), _vp_of(out)))
    return out[:n]


def one_minimizer_reads_device(hasher: Hasher, k: int, d_packed, n_reads=None, out_pos=None, read_starts=None, read_stride=0,
                               read_len=0, base_offset=0, ws=None, amb=None, amb_offset=0):
    """``one_minimizer`` (src/minimizers.rs:22-28) of EVERY read of a packed device buffer in one call
    (``mm_one_minimizer_reads_device_async``): ``d_packed`` a uint8 CUDA tensor - or a ``FastaRecords``, whose starts are
    then taken - and the layout: ``read_starts`` (int64 CUDA tensor of n + 1) or ``read_stride`` / ``read_len``.
    ``out_pos`` (int32 CUDA tensor, n_reads) receives the read-local position of the leftmost minimal
    ``hash & 0xffff0000`` per read, ``NO_MINIMIZER`` for a read shorter than k; a new tensor is returned when it is None.
    With ``amb`` (a uint8 CUDA tensor of ambiguity bits, base j from ``base_offset`` = bit ``amb_offset + j``; a
    ``FastaRecords`` of ``fasta_pack_n_device`` supplies its own) the skip-ambiguous form
    (``mm_one_minimizer_reads_skip_ambiguous_device_async``): only k-mers without an ambiguous base count,
    ``NO_MINIMIZER`` for a read without one.
    Asynchronous on ``ws`` (default: the device's default workspace): ``Workspace.sync`` before reading."""
    import torch
    if isinstance(d_packed, FastaRecords):
        rec = d_packed
        d_packed, n_reads = rec.packed, len(rec)
        if amb is None and rec.amb is not None:
            amb, amb_offset = rec.amb, 0
        read_starts = torch.from_numpy(np.ascontiguousarray(rec.base, dtype=np.uint64).view(np.int64)).to(d_packed.device)
    n_reads = int(n_reads)
    dev = d_packed.device
    if ws is None:
        ws = default_workspace(dev.index or 0)
    if out_pos is None:
        out_pos = torch.zeros(n_reads, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
    elif out_pos.numel() < n_reads:
        raise ValueError(f"out_pos holds {out_pos.numel()} words, {n_reads} needed")
    if read_starts is not None and read_starts.numel() < n_reads + 1:
        raise ValueError(f"{n_reads} reads need {n_reads + 1} starts")
    if amb is not None:
        _check(lib().mm_one_minimizer_reads_skip_ambiguous_device_async(
            ws.h, C.byref(hasher), int(k), _vp_of(d_packed), int(d_packed.numel()), int(base_offset), _vp_of(amb),
            int(amb.numel()), int(amb_offset), n_reads, _vp_of(read_starts), int(read_stride), int(read_len), _vp_of(out_pos)))
        return out_pos
    _check(lib().mm_one_minimizer_reads_device_async(ws.h, C.byref(hasher), int(k), _vp_of(d_packed), int(d_packed.numel()),
                                                     int(base_offset), n_reads, _vp_of(read_starts), int(read_stride),
                                                     int(read_len), _vp_of(out_pos)))
    return out_pos


def one_minimizer_text_batch_device(hasher: TextHasher, k: int, d_text, d_starts=None, n_records=None, out_pos=None, ws=None):
    """``one_minimizer`` of EVERY record of a device text batch in one call
    (``mm_one_minimizer_text_batch_device_async``): ``d_text`` a uint8 CUDA tensor and ``d_starts`` an int64 CUDA tensor of
    n + 1 starts - or a ``FastaTextRecords`` in place of both.  ``out_pos`` as for ``one_minimizer_reads_device``."""
    import torch
    if isinstance(d_text, FastaTextRecords):
        d_text, d_starts = d_text.seq, d_text.starts
    if n_records is None:
        n_records = d_starts.numel() - 1
    n_records = int(n_records)
    if n_records < 0 or d_starts.numel() < n_records + 1:
        raise ValueError("d_starts holds n + 1 starts")
    dev = d_starts.device
    if ws is None:
        ws = default_workspace(dev.index or 0)
    if out_pos is None:
        out_pos = torch.zeros(n_records, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
    elif out_pos.numel() < n_records:
        raise ValueError(f"out_pos holds {out_pos.numel()} words, {n_records} needed")
    _check(lib().mm_one_minimizer_text_batch_device_async(ws.h, C.byref(hasher), int(k),
                                                          _vp_of(d_text) if d_text.numel() else None, int(d_text.numel()),
                                                          n_records, _vp_of(d_starts), _vp_of(out_pos)))
    return out_pos


def debug_one_minimizer_counts_view(max_sym: int, max_records: int, n_sym: int, n: int, starts=None) -> tuple:
    """What every workgroup of the counts forms turns {counts, bounds} into (``mm_debug_one_minimizer_counts_view``, no
    GPU): ``(n, limit, refused)``.  ``starts`` (uint64 array) is read at ``[n]`` only, and not at all for a refused view."""
    starts = np.ascontiguousarray(starts, dtype=np.uint64) if starts is not None else None
    out = np.zeros(3, dtype=np.uint64)
    _check(lib().mm_debug_one_minimizer_counts_view(int(max_sym), int(max_records), int(n_sym), int(n), _vp_of(starts),
                                                    _vp_of(out)))
    return int(out[0]), int(out[1]), bool(out[2])


def debug_one_minimizer_text_batch_counts(hasher: TextHasher, k: int, text, starts, counts, max_chars=None, tile=0,
                                          refused_ok=False) -> np.ndarray:
    """The counts form's per-tile function on the host (``mm_debug_one_minimizer_text_batch_counts``, no GPU): ``starts``
    holds max_records + 1 words, ``counts`` = (characters, records); returns ``np.uint32[max_records]``.  A refused view
    raises (MM_ERR_CAPACITY) unless ``refused_ok``."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    max_records = len(starts) - 1
    out = np.zeros(max(1, max_records), dtype=np.uint32)
    rc = lib().mm_debug_one_minimizer_text_batch_counts(C.byref(hasher), int(k), _vp_of(text), len(text),
                                                        len(text) if max_chars is None else int(max_chars), max_records,
                                                        _vp_of(starts), _vp_of(counts), int(tile), _vp_of(out))
    if not (refused_ok and rc == ERR["CAPACITY"]):
        _check(rc)
    return out[:max_records]


def debug_one_minimizer_reads_counts(hasher: Hasher, k: int, packed, read_starts, counts, max_bases=None, base_offset=0,
                                     tile=0, refused_ok=False, amb=None, amb_offset=0) -> np.ndarray:
    """The same for reads of a packed buffer (``mm_debug_one_minimizer_reads_counts``, no GPU); ``max_bases`` defaults to
    what the buffer holds behind ``base_offset``.  With ``amb`` / ``amb_offset`` the skip-ambiguous form
    (``mm_debug_one_minimizer_reads_skip_ambiguous_counts``)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    starts = np.ascontiguousarray(read_starts, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    max_records = len(starts) - 1
    if max_bases is None:
        max_bases = 4 * len(packed) - int(base_offset)
        if amb is not None:
            max_bases = min(max_bases, 8 * len(amb) - int(amb_offset))
    out = np.zeros(max(1, max_records), dtype=np.uint32)
    if amb is not None:
        amb = np.ascontiguousarray(amb, dtype=np.uint8)
        rc = lib().mm_debug_one_minimizer_reads_skip_ambiguous_counts(
            C.byref(hasher), int(k), _vp_of(packed), len(packed), int(base_offset), _vp_of(amb), len(amb), int(amb_offset),
            int(max_bases), max_records, _vp_of(starts), _vp_of(counts), int(tile), _vp_of(out))
    else:
        rc = lib().mm_debug_one_minimizer_reads_counts(C.byref(hasher), int(k), _vp_of(packed), len(packed), int(base_offset),
                                                       int(max_bases), max_records, _vp_of(starts), _vp_of(counts), int(tile),
                                                       _vp_of(out))
    if not (refused_ok and rc == ERR["CAPACITY"]):
        _check(rc)
    return out[:max_records]


def one_minimizer_text_batch_counts_device(hasher: TextHasher, k: int, d_text, d_starts=None, d_counts=None, max_records=None,
                                           max_chars=None, out_pos=None, ws=None):
    """``one_minimizer`` of every record of a device text batch whose two counts (characters, records) are read on the
    DEVICE (``mm_one_minimizer_text_batch_counts_device_async``): the call queues behind ``fasta_text_device_async`` with no
    host wait.  ``d_text`` uint8, ``d_starts`` int64 of max_records + 1, ``d_counts`` int64 of 2 (what the
    loader writes; ``max_chars`` defaults to all of ``d_text``).  ``out_pos`` (int32, max_records) receives the
    positions of the records there are and ``NO_MINIMIZER`` behind them; counts beyond the bounds give ``NO_MINIMIZER``
    everywhere and MM_ERR_CAPACITY from ``Workspace.check``.  Asynchronous on ``ws``."""
    import torch
    if max_records is None:
        max_records = d_starts.numel() - 1
    max_records = int(max_records)
    if max_records < 0 or d_starts.numel() < max_records + 1:
        raise ValueError("d_starts holds max_records + 1 starts")
    if d_counts is None or d_counts.numel() < 2:
        raise ValueError("d_counts holds two words: characters, records")
    max_chars = int(d_text.numel()) if max_chars is None else int(max_chars)
    dev = d_starts.device
    if ws is None:
        ws = default_workspace(dev.index or 0)
    if out_pos is None:
        out_pos = torch.zeros(max_records, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
    elif out_pos.numel() < max_records:
        raise ValueError(f"out_pos holds {out_pos.numel()} words, {max_records} needed")
    _check(lib().mm_one_minimizer_text_batch_counts_device_async(
        ws.h, C.byref(hasher), int(k), _vp_of(d_text) if d_text.numel() else None, int(d_text.numel()), max_chars,
        max_records, _vp_of(d_starts), _vp_of(d_counts), _vp_of(out_pos)))
    return out_pos


def one_minimizer_reads_counts_device(hasher: Hasher, k: int, d_packed, read_starts, d_counts, max_records=None,
                                      max_bases=None, out_pos=None, base_offset=0, ws=None, amb=None, amb_offset=0):
    """The same for the reads of a packed device buffer (``mm_one_minimizer_reads_counts_device_async``; starts layout
    only): behind ``fasta_pack_device_async`` / ``fastq_pack_device_async`` with no host wait.  ``max_bases`` defaults to
    what the buffer holds behind ``base_offset`` (with ``amb``: what both buffers hold).  With ``amb`` / ``amb_offset``
    (the N packers' bits) the skip-ambiguous form (``mm_one_minimizer_reads_skip_ambiguous_counts_device_async``)."""
    import torch
    if max_records is None:
        max_records = read_starts.numel() - 1
    max_records = int(max_records)
    if max_records < 0 or read_starts.numel() < max_records + 1:
        raise ValueError("read_starts holds max_records + 1 starts")
    if d_counts is None or d_counts.numel() < 2:
        raise ValueError("d_counts holds two words: bases, records")
    if max_bases is None:
        max_bases = 4 * int(d_packed.numel()) - int(base_offset)
        if amb is not None:
            max_bases = min(max_bases, 8 * int(amb.numel()) - int(amb_offset))
    dev = d_packed.device
    if ws is None:
        ws = default_workspace(dev.index or 0)
    if out_pos is None:
        out_pos = torch.zeros(max_records, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
    elif out_pos.numel() < max_records:
        raise ValueError(f"out_pos holds {out_pos.numel()} words, {max_records} needed")
    if amb is not None:
        _check(lib().mm_one_minimizer_reads_skip_ambiguous_counts_device_async(
            ws.h, C.byref(hasher), int(k), _vp_of(d_packed), int(d_packed.numel()), int(base_offset), _vp_of(amb),
            int(amb.numel()), int(amb_offset), int(max_bases), max_records, _vp_of(read_starts), _vp_of(d_counts),
            _vp_of(out_pos)))
        return out_pos
    _check(lib().mm_one_minimizer_reads_counts_device_async(
        ws.h, C.byref(hasher), int(k), _vp_of(d_packed), int(d_packed.numel()), int(base_offset), int(max_bases), max_records,
        _vp_of(read_starts), _vp_of(d_counts), _vp_of(out_pos)))
    return out_pos


def one_minimizer_reads_host(reads, hasher: Hasher, k: int, ws=None, amb=None, amb_offset=0) -> np.ndarray:
    """``one_minimizer`` of many host reads (``PackedSeq`` views / ASCII ``bytes``) in ONE call
    (``mm_one_minimizer_reads_host``): ``np.uint32[n]``, ``NO_MINIMIZER`` for a read shorter than k.  With ``amb`` (a
    uint8 array of ambiguity bits over the reads laid back to back, base j = bit ``amb_offset + j``) the skip-ambiguous
    form (``mm_one_minimizer_reads_skip_ambiguous_host``): ``NO_MINIMIZER`` for a read without a clean k-mer."""
    packed, starts = _pack_reads(reads)
    n = len(starts) - 1
    out = np.zeros(max(1, n), dtype=np.uint32)
    ws = ws or default_workspace(0)
    if amb is not None:
        amb = np.ascontiguousarray(amb, dtype=np.uint8)
        _check(lib().mm_one_minimizer_reads_skip_ambiguous_host(ws.h, C.byref(hasher), int(k), _vp_of(packed), len(packed), 0,
                                                                _vp_of(amb), len(amb), int(amb_offset), n, _vp_of(starts), 0, 0,
                                                                _vp_of(out)))
        return out[:n]
    _check(lib().mm_one_minimizer_reads_host(ws.h, C.byref(hasher), int(k), _vp_of(packed), len(packed), 0, n, _vp_of(starts),
                                             0, 0, _vp_of(out)))
    return out[:n]


def one_minimizer_text_batch_host(records, hasher: TextHasher, k: int, ws=None) -> np.ndarray:
    """``one_minimizer`` of many host records of byte text in ONE call (``mm_one_minimizer_text_batch_host``)."""
    text, starts = _text_records(records)
    n = len(starts) - 1
    out = np.zeros(max(1, n), dtype=np.uint32)
    ws = ws or default_workspace(0)
    _check(lib().mm_one_minimizer_text_batch_host(ws.h, C.byref(hasher), int(k), _vp_of(text), len(text), n, _vp_of(starts),
                                                  _vp_of(out)))
    return out[:n]


def one_minimizer(seq, hasher, k: int) -> int:
    """``one_minimizer(seq, hasher)`` (src/minimizers.rs:22-28): the leftmost position that minimises
    ``hash & 0xffff0000`` over the k-mers of ``seq`` (``PackedSeq``, ``AsciiSeq`` or byte text).  A ``Hasher`` over
    ``AsciiSeq`` / bytes reads them as ASCII DNA (``TextHasher.from_dna``).  Raises ``ValueError`` when ``len(seq) < k``,
    where the reference panics."""
    if len(seq) < k:
        raise ValueError(f"one_minimizer: the sequence has {len(seq)} symbols, k is {k}")
    if isinstance(seq, PackedSeq):
        return int(one_minimizer_reads_host([seq], hasher, k)[0])
    data = seq.seq if isinstance(seq, AsciiSeq) else seq
    if isinstance(hasher, Hasher):
        hasher = TextHasher.from_dna(hasher)
    return int(one_minimizer_text_batch_host([data], hasher, k)[0])


def run_fasta_device(builder: "Builder", records: FastaRecords, out_pos, out_sk=None):
    """All records of a packed FASTA (``fasta_pack_device``) with one plan in one launch (``mm_run_batch_device``);
    record-local positions back to back in ``out_pos``; returns the n + 1 offsets."""
    v = records.views()
    return run_batch_device(builder, [t for t, _, _ in v], [m for _, _, m in v], out_pos, out_sk,
                            base_offsets=[o for _, o, _ in v])


def generate_device(n_bases: int, seed: int, device: int = 0, first_base: int = 0):
    """Synthetic PackedSeq (generator G) written directly into HBM.
    Returns a torch uint8 CUDA tensor of ceil(n/4)+64 bytes."""
    import torch

    ws = default_workspace(device)
    t = torch.zeros((n_bases + 3) // 4 + 64, dtype=torch.uint8, device=f"cuda:{device}")
    torch.cuda.synchronize(device)
    _check(lib().mm_generate_device_async(ws.h, seed, first_base, n_bases, C.c_void_p(t.data_ptr())))
    ws.sync()
    return t
