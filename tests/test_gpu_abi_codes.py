"""Return codes of the C ABI's run, values and packer entry points, pinned: tests/golden/abi_return_codes.json holds, for
every case of the table below, the code the library returned when the fixture was recorded.  Which error a doubly-wrong
call reports is part of the ABI (the Python wrapper and several tests depend on it), and the entry points share their
plumbing: a change that reorders an argument check shows up here.

Every case either returns from an argument check or runs on a valid tiny input - k = 5, w = 3 on 64 bases, 3 reads of
20 bases, a 40-byte text, a two-record FASTA / FASTQ text.  No case hands a launch a pointer that is not a real buffer.

Record the fixture with the library whose behaviour is to be pinned (MM_LIB_PATH selects a build):
    python tests/test_gpu_abi_codes.py --record
A recorded HIP error is refused: such a case does not belong in the table.

The module also runs the entry points that no other GPU test checks against the oracle: mm_values_u128_device_async and
mm_run_host_ascii (its twins mm_run_host and mm_run_skip_ambiguous_host_ascii are covered elsewhere)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_return_codes.json")
MM_ERR_HIP = -21
K, W = 5, 3

# ---------------------------------------------------------------------------------------------- signatures
# p: pointer or handle, q: uint64_t, u: uint32_t, i: int
_RUN = "plan:p ws:p d_packed:p packed_bytes:q base_offset:q n_bases:q win_begin:q win_end:q d_out_pos:p d_out_sk:p capacity:q count:p"
_SKIP = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q d_amb:p amb_bytes:q amb_offset:q n_bases:q win_begin:q win_end:q "
         "d_out_pos:p capacity:q count:p")
_READS = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q n_reads:q read_stride:u read_len:u d_read_lens:p d_out_pos:p "
          "capacity:q d_out_offsets:p count:p")
_READS_SK = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q n_reads:q read_stride:u read_len:u d_read_lens:p d_out_pos:p "
             "d_out_sk:p capacity:q d_out_offsets:p count:p")
_READS_SKIP = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q d_amb:p amb_bytes:q amb_offset:q n_reads:q read_stride:u "
               "read_len:u d_read_lens:p d_out_pos:p capacity:q d_out_offsets:p count:p")
_PACKED = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q n_reads:q d_read_starts:p total_bases:q max_read_len:u "
           "d_out_pos:p d_out_sk:p capacity:q d_out_offsets:p count:p")
_PACKED_SKIP = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q d_amb:p amb_bytes:q amb_offset:q n_reads:q d_read_starts:p "
                "total_bases:q max_read_len:u d_out_pos:p capacity:q d_out_offsets:p count:p")
_TEXT = "plan:p ws:p d_text:p text_bytes:q n:q win_begin:q win_end:q d_out_pos:p d_out_sk:p capacity:q count:p"
_TEXT_BATCH = ("plan:p ws:p d_text:p text_bytes:q n_records:q d_starts:p n_chars:q d_out_pos:p d_out_sk:p capacity:q "
               "d_out_offsets:p count:p")
_VALUES_DEV = "ws:p d_packed:p packed_bytes:q base_offset:q n_bases:q len:u canonical:i d_pos:p n_pos:q d_values:p"
_VALUES_HOST = "ws:p packed:p base_offset:q n_bases:q len:u canonical:i pos:p n_pos:q values:p"
_PACK = "ws:p d_text:p n_bytes:q d_packed:p packed_capacity_bytes:q d_rec_base:p d_rec_text_pos:p max_records:q d_counts:p"
_PACK_N = ("ws:p d_text:p n_bytes:q d_packed:p packed_capacity_bytes:q d_amb:p amb_capacity_bytes:q d_rec_base:p "
           "d_rec_text_pos:p max_records:q d_counts:p")
_PCOUNTS = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q max_bases:q max_records:q d_read_starts:p d_counts:p d_out_pos:p "
            "d_out_sk:p capacity:q d_out_offsets:p")
_PCOUNTS_SKIP = ("plan:p ws:p d_packed:p packed_bytes:q base_offset:q d_amb:p amb_bytes:q amb_offset:q max_bases:q max_records:q "
                 "d_read_starts:p d_counts:p d_out_pos:p capacity:q d_out_offsets:p")
_TCOUNTS = ("plan:p ws:p d_text:p text_bytes:q max_chars:q max_records:q d_starts:p d_counts:p d_out_pos:p d_out_sk:p capacity:q "
            "d_out_offsets:p")
_VREADS_DEV = ("ws:p d_packed:p packed_bytes:q base_offset:q n_reads:q d_read_starts:p read_stride:u len:u canonical:i d_pos:p "
               "d_out_offsets:p n_pos_max:q d_values:p")
_VREADS_HOST = ("ws:p packed:p packed_bytes:q base_offset:q n_reads:q read_starts:p read_stride:u len:u canonical:i pos:p "
                "offsets:p values:p")
_VBATCH = "ws:p n_seqs:q d_packed:p packed_bytes:p base_offsets:p n_bases:p len:u canonical:i d_pos:p offsets:p d_values:p"
_VTEXT_DEV = "ws:p d_text:p text_bytes:q n:q encoding:i len:u canonical:i d_pos:p n_pos:q d_values:p"
_VTEXT_HOST = "ws:p text:p n:q encoding:i len:u canonical:i pos:p n_pos:q values:p"
_VTBATCH_DEV = ("ws:p d_text:p text_bytes:q n_records:q d_starts:p n_chars:q encoding:i len:u canonical:i d_pos:p d_out_offsets:p "
                "n_pos_max:q d_values:p")
_VTCOUNTS = ("ws:p d_text:p text_bytes:q max_chars:q max_records:q d_starts:p d_counts:p encoding:i len:u canonical:i d_pos:p "
             "d_out_offsets:p n_pos_max:q d_values:p")
_VTBATCH_HOST = "ws:p text:p n_records:q starts:p encoding:i len:u canonical:i pos:p offsets:p values:p"
_FTEXT = "ws:p d_text:p n_bytes:q d_seq:p seq_capacity_bytes:q d_rec_start:p d_rec_text_pos:p max_records:q d_counts:p"
SIG = {
    "mm_run_device_async": _RUN, "mm_run_device": _RUN,
    "mm_run_skip_ambiguous_device_async": _SKIP, "mm_run_skip_ambiguous_device": _SKIP,
    "mm_run_host": "plan:p ws:p packed:p base_offset:q n_bases:q out_pos:p out_sk:p capacity:q count:p",
    "mm_run_host_ascii": "plan:p ws:p ascii:p n_bases:q out_pos:p out_sk:p capacity:q count:p",
    "mm_run_skip_ambiguous_host": "plan:p ws:p packed:p base_offset:q amb:p amb_offset:q n_bases:q out_pos:p capacity:q count:p",
    "mm_run_skip_ambiguous_host_ascii": "plan:p ws:p ascii:p n_bases:q out_pos:p capacity:q count:p",
    "mm_run_reads_device_async": _READS, "mm_run_reads_device": _READS,
    "mm_run_reads_superkmers_device_async": _READS_SK, "mm_run_reads_superkmers_device": _READS_SK,
    "mm_run_reads_skip_ambiguous_device_async": _READS_SKIP, "mm_run_reads_skip_ambiguous_device": _READS_SKIP,
    "mm_run_packed_reads_device_async": _PACKED, "mm_run_packed_reads_device": _PACKED,
    "mm_run_packed_reads_skip_ambiguous_device_async": _PACKED_SKIP, "mm_run_packed_reads_skip_ambiguous_device": _PACKED_SKIP,
    "mm_run_packed_reads_host": "plan:p ws:p packed:p n_reads:q read_starts:p max_read_len:u out_pos:p out_sk:p capacity:q "
                                "out_offsets:p count:p",
    "mm_run_packed_reads_skip_ambiguous_host": "plan:p ws:p packed:p amb:p n_reads:q read_starts:p max_read_len:u out_pos:p "
                                               "capacity:q out_offsets:p count:p",
    "mm_run_text_device_async": _TEXT, "mm_run_text_device": _TEXT,
    "mm_run_text_host": "plan:p ws:p text:p n:q out_pos:p out_sk:p capacity:q count:p",
    "mm_run_text_batch_device_async": _TEXT_BATCH, "mm_run_text_batch_device": _TEXT_BATCH,
    "mm_run_text_batch_host": "plan:p ws:p text:p n_records:q starts:p out_pos:p out_sk:p capacity:q out_offsets:p count:p",
    "mm_run_batch_device": "plan:p ws:p n_seqs:q d_packed:p packed_bytes:p base_offsets:p n_bases:p d_out_pos:p d_out_sk:p "
                           "capacity:q out_offsets:p",
    "mm_values_u64_device_async": _VALUES_DEV, "mm_values_u128_device_async": _VALUES_DEV,
    "mm_values_u64_host": _VALUES_HOST, "mm_values_u128_host": _VALUES_HOST,
    "mm_fasta_pack_device_async": _PACK, "mm_fastq_pack_device_async": _PACK, "mm_fasta_pack_device": _PACK + " out_counts:p",
    "mm_fasta_pack_n_device_async": _PACK_N, "mm_fastq_pack_n_device_async": _PACK_N,
    "mm_fasta_pack_n_device": _PACK_N + " out_counts:p",
    "mm_run_sharded_host": "plan:p group:p packed:p base_offset:q n_bases:q out_pos:p out_sk:p capacity:q count:p",
    "mm_run_sharded_device": "plan:p group:p base_offset:q n_bases:q want_superkmers:i counts:p total:p",
    "mm_run_batch_sharded_device": "plan:p group:p base_offsets:p n_bases:p want_superkmers:i out_counts:p total:p",
    "mm_run_batch_sharded_host": "plan:p group:p n_seqs:q packed:p base_offsets:p n_bases:p out_pos:p out_sk:p capacity:q "
                                 "out_offsets:p",
    # ---- the families added after the first recording
    "mm_run_packed_reads_counts_device_async": _PCOUNTS + " d_count:p", "mm_run_packed_reads_counts_device": _PCOUNTS + " out:p",
    "mm_run_packed_reads_skip_ambiguous_counts_device_async": _PCOUNTS_SKIP + " d_count:p",
    "mm_run_packed_reads_skip_ambiguous_counts_device": _PCOUNTS_SKIP + " out:p",
    "mm_run_text_batch_counts_device_async": _TCOUNTS + " d_count:p", "mm_run_text_batch_counts_device": _TCOUNTS + " out:p",
    "mm_values_u64_reads_device_async": _VREADS_DEV, "mm_values_u128_reads_device_async": _VREADS_DEV,
    "mm_values_u64_reads_host": _VREADS_HOST, "mm_values_u128_reads_host": _VREADS_HOST,
    "mm_values_u64_batch_device_async": _VBATCH, "mm_values_u128_batch_device_async": _VBATCH,
    "mm_values_u64_text_device_async": _VTEXT_DEV, "mm_values_u128_text_device_async": _VTEXT_DEV,
    "mm_values_u64_text_host": _VTEXT_HOST, "mm_values_u128_text_host": _VTEXT_HOST,
    "mm_values_u64_text_batch_device_async": _VTBATCH_DEV, "mm_values_u128_text_batch_device_async": _VTBATCH_DEV,
    "mm_values_u64_text_batch_counts_device_async": _VTCOUNTS, "mm_values_u128_text_batch_counts_device_async": _VTCOUNTS,
    "mm_values_u64_text_batch_host": _VTBATCH_HOST, "mm_values_u128_text_batch_host": _VTBATCH_HOST,
    "mm_fasta_text_device_async": _FTEXT, "mm_fasta_text_device": _FTEXT + " out_counts:p",
    "mm_pack_ascii_device_async": "ws:p d_ascii:p n_bases:q d_packed:p",
    "mm_pack_ascii_n_device_async": "ws:p d_ascii:p n_bases:q d_packed:p d_amb:p",
}
_KIND = {"p": C.c_void_p, "q": C.c_uint64, "u": C.c_uint32, "i": C.c_int}

# ---------------------------------------------------------------------------------------------- the case table
# A pointer argument is null (None) or names a buffer of the environment below ("d_*" device, "h_*" host; "+1": one byte
# in, misaligned); a plan is one of canon / fwd / sync (closed syncmers) / text / text_sync; "ws" is the workspace.
BIG = 1 << 32
U64_MAX = (1 << 64) - 1
FASTA = b">r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n>r2\nGGGTTTAAACCC\n"
FASTQ = b"@r1\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n@r2\nGGGTTTAAACCCGGGTTTAA\n+\nIIIIIIIIIIIIIIIIIIII\n"

_run_ok = dict(plan="canon", ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, n_bases=64, win_begin=0,
               win_end=U64_MAX, d_out_pos="d_out", d_out_sk=None, capacity=256)
_skip_ok = dict(plan="canon", ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, d_amb="d_amb", amb_bytes=4096,
                amb_offset=0, n_bases=64, win_begin=0, win_end=U64_MAX, d_out_pos="d_out", capacity=256)
_reads_ok = dict(plan="canon", ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, n_reads=3, read_stride=20,
                 read_len=20, d_read_lens=None, d_out_pos="d_out", capacity=256, d_out_offsets="d_offs")
_reads_sk_ok = dict(_reads_ok, d_out_sk="d_sk")
_reads_skip_ok = dict(_reads_ok, d_amb="d_amb", amb_bytes=4096, amb_offset=0)
_packed_ok = dict(plan="canon", ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, n_reads=3, d_read_starts="d_starts",
                  total_bases=60, max_read_len=20, d_out_pos="d_out", d_out_sk=None, capacity=256, d_out_offsets="d_offs")
_packed_skip_ok = dict({k: v for k, v in _packed_ok.items() if k != "d_out_sk"}, d_amb="d_amb", amb_bytes=4096, amb_offset=0)
_text_ok = dict(plan="text", ws="ws", d_text="d_text", text_bytes=40, n=40, win_begin=0, win_end=U64_MAX, d_out_pos="d_out",
                d_out_sk=None, capacity=256)
_text_batch_ok = dict(plan="text", ws="ws", d_text="d_text", text_bytes=40, n_records=3, d_starts="d_tstarts", n_chars=40,
                      d_out_pos="d_out", d_out_sk=None, capacity=256, d_out_offsets="d_offs")
_host_ok = dict(plan="canon", ws="ws", packed="h_seq", base_offset=0, n_bases=64, out_pos="h_out", out_sk=None, capacity=256,
                count="h_count")
_ascii_ok = dict(plan="canon", ws="ws", ascii="h_ascii", n_bases=64, out_pos="h_out", out_sk=None, capacity=256, count="h_count")
_skip_host_ok = dict(plan="canon", ws="ws", packed="h_seq", base_offset=0, amb="h_amb", amb_offset=0, n_bases=64,
                     out_pos="h_out", capacity=256, count="h_count")
_skip_ascii_ok = dict(plan="canon", ws="ws", ascii="h_ascii", n_bases=64, out_pos="h_out", capacity=256, count="h_count")
_packed_host_ok = dict(plan="canon", ws="ws", packed="h_seq", n_reads=3, read_starts="h_starts", max_read_len=20,
                       out_pos="h_out", out_sk=None, capacity=256, out_offsets="h_offs", count="h_count")
_packed_skip_host_ok = dict({k: v for k, v in _packed_host_ok.items() if k != "out_sk"}, amb="h_amb")
_text_host_ok = dict(plan="text", ws="ws", text="h_text", n=40, out_pos="h_out", out_sk=None, capacity=256, count="h_count")
_text_batch_host_ok = dict(plan="text", ws="ws", text="h_text", n_records=3, starts="h_tstarts", out_pos="h_out", out_sk=None,
                           capacity=256, out_offsets="h_offs", count="h_count")
_values_dev_ok = dict(ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, n_bases=64, len=5, canonical=1,
                      d_pos="d_vpos", n_pos=4, d_values="d_vals")
_values_host_ok = dict(ws="ws", packed="h_seq", base_offset=0, n_bases=64, len=5, canonical=1, pos="h_vpos", n_pos=4,
                       values="h_vals")
_pack_ok = dict(ws="ws", d_text="d_fasta", n_bytes=len(FASTA), d_packed="d_packed", packed_capacity_bytes=4096,
                d_rec_base="d_rec_base", d_rec_text_pos="d_rec_pos", max_records=16, d_counts="d_counts")
_pack_n_ok = dict(_pack_ok, d_amb="d_ambout", amb_capacity_bytes=4096)
_fastq = dict(d_text="d_fastq", n_bytes=len(FASTQ))

# ---- the families added after the first recording: the reads' and the text's {bases / characters, records} are the 2-word
# buffers d_rcounts / d_tcounts; values are asked at the read-local positions *_rpos, delimited by *_voffs
_pcounts_ok = dict(plan="canon", ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, max_bases=60, max_records=3,
                   d_read_starts="d_starts", d_counts="d_rcounts", d_out_pos="d_out", d_out_sk=None, capacity=256, d_out_offsets="d_offs")
_pcounts_skip_ok = dict({k: v for k, v in _pcounts_ok.items() if k != "d_out_sk"}, d_amb="d_amb", amb_bytes=4096, amb_offset=0)
_tcounts_ok = dict(plan="text", ws="ws", d_text="d_text", text_bytes=40, max_chars=40, max_records=3, d_starts="d_tstarts",
                   d_counts="d_tcounts", d_out_pos="d_out", d_out_sk=None, capacity=256, d_out_offsets="d_offs")
_vreads_dev_ok = dict(ws="ws", d_packed="d_seq", packed_bytes=4096, base_offset=0, n_reads=3, d_read_starts="d_starts", read_stride=0,
                      len=5, canonical=1, d_pos="d_rpos", d_out_offsets="d_voffs", n_pos_max=4, d_values="d_vals")
_vreads_host_ok = dict(ws="ws", packed="h_seq", packed_bytes=4096, base_offset=0, n_reads=3, read_starts="h_starts", read_stride=0,
                       len=5, canonical=1, pos="h_rpos", offsets="h_voffs", values="h_vals")
_vbatch_ok = dict(ws="ws", n_seqs=3, d_packed="h_bptrs", packed_bytes="h_bbytes", base_offsets=None, n_bases="h_bbases", len=5,
                  canonical=1, d_pos="d_rpos", offsets="h_voffs", d_values="d_vals")
_vtext_dev_ok = dict(ws="ws", d_text="d_text", text_bytes=40, n=40, encoding=0, len=5, canonical=0, d_pos="d_vpos", n_pos=4,
                     d_values="d_vals")
_vtext_host_ok = dict(ws="ws", text="h_text", n=40, encoding=0, len=5, canonical=0, pos="h_vpos", n_pos=4, values="h_vals")
_vtbatch_dev_ok = dict(ws="ws", d_text="d_text", text_bytes=40, n_records=3, d_starts="d_tstarts", n_chars=40, encoding=0, len=5,
                       canonical=0, d_pos="d_rpos", d_out_offsets="d_voffs", n_pos_max=4, d_values="d_vals")
_vtcounts_ok = dict(ws="ws", d_text="d_text", text_bytes=40, max_chars=40, max_records=3, d_starts="d_tstarts", d_counts="d_tcounts",
                    encoding=0, len=5, canonical=0, d_pos="d_rpos", d_out_offsets="d_voffs", n_pos_max=4, d_values="d_vals")
_vtbatch_host_ok = dict(ws="ws", text="h_text", n_records=3, starts="h_tstarts", encoding=0, len=5, canonical=0, pos="h_rpos",
                        offsets="h_voffs", values="h_vals")
_ftext_ok = dict(ws="ws", d_text="d_fasta", n_bytes=len(FASTA), d_seq="d_packed", seq_capacity_bytes=4096, d_rec_start="d_rec_base",
                 d_rec_text_pos="d_rec_pos", max_records=16, d_counts="d_counts")
_ascii_pack_ok = dict(ws="ws", d_ascii="d_ascii", n_bases=64, d_packed="d_packed")


def _variants(fn, ok, wrong_plan, overrides):
    """The cases every run entry point gets - valid, each handle missing, the plan of the other kind, and the doubly-wrong
    calls that tell the order of those checks apart - then its own."""
    rows = [{}, dict(plan=None), dict(ws=None), dict(plan=wrong_plan), dict(plan=wrong_plan, ws=None), dict(plan=None, ws=None)]
    return [(fn, dict(ok, **o)) for o in rows + overrides]


def _sync_and_async(fn_async, fn_sync, ok, wrong_plan, overrides):
    """(the synchronous form writes its count to host memory, the asynchronous one to device memory)"""
    return (_variants(fn_sync, dict(ok, count="h_count"), wrong_plan, overrides) +
            _variants(fn_async, dict(ok, count="d_count"), wrong_plan, overrides))


def cases():
    t = []
    long_ = [dict(n_bases=BIG), dict(n_bases=BIG, plan="text"), dict(n_bases=BIG, ws=None)]
    small = [dict(capacity=1), dict(d_out_pos=None, capacity=0)]
    t += _sync_and_async("mm_run_device_async", "mm_run_device", _run_ok, "text", long_ + small + [
        dict(plan="sync", d_out_sk="d_sk"), dict(plan="sync", d_out_sk="d_sk", n_bases=BIG), dict(d_out_sk="d_sk"),
        dict(plan="fwd"), dict(d_packed=None), dict(n_bases=0, d_packed=None)])
    t += _sync_and_async("mm_run_skip_ambiguous_device_async", "mm_run_skip_ambiguous_device", _skip_ok, "text", long_ + small + [
        dict(plan="fwd"), dict(plan="fwd", d_amb=None), dict(plan="fwd", n_bases=BIG), dict(d_amb=None), dict(plan="sync")])
    reads_long = [dict(n_reads=BIG), dict(n_reads=BIG, ws=None), dict(n_reads=BIG, plan="text")]
    reads_more = reads_long + small + [dict(d_out_offsets=None), dict(d_out_offsets=None, plan="text"), dict(n_reads=0),
                                       dict(d_read_lens="d_lens"), dict(d_packed=None)]
    t += _sync_and_async("mm_run_reads_device_async", "mm_run_reads_device", _reads_ok, "text", reads_more + [dict(plan="fwd")])
    t += _sync_and_async("mm_run_reads_superkmers_device_async", "mm_run_reads_superkmers_device", _reads_sk_ok, "text", reads_more + [
        dict(d_out_sk=None), dict(d_out_sk=None, ws=None), dict(d_out_sk=None, plan="text"), dict(plan="sync"),
        dict(plan="sync", d_out_offsets=None)])
    t += _sync_and_async("mm_run_reads_skip_ambiguous_device_async", "mm_run_reads_skip_ambiguous_device", _reads_skip_ok, "text",
                         reads_long + small + [dict(plan="fwd"), dict(plan="fwd", d_out_offsets=None), dict(d_amb=None),
                                               dict(plan="fwd", n_reads=BIG), dict(n_reads=0, d_amb=None)])
    packed_more = reads_long + small + [dict(d_read_starts=None), dict(d_read_starts=None, ws=None), dict(d_read_starts=None, plan="text"),
                                        dict(d_read_starts=None, n_reads=0), dict(d_out_offsets=None), dict(total_bases=BIG)]
    t += _sync_and_async("mm_run_packed_reads_device_async", "mm_run_packed_reads_device", _packed_ok, "text", packed_more + [
        dict(plan="sync", d_out_sk="d_sk"), dict(plan="sync", d_out_sk="d_sk", d_out_offsets=None), dict(d_out_sk="d_sk"), dict(plan="fwd")])
    t += _sync_and_async("mm_run_packed_reads_skip_ambiguous_device_async", "mm_run_packed_reads_skip_ambiguous_device",
                         _packed_skip_ok, "text", packed_more + [
        dict(plan="fwd"), dict(plan="fwd", d_amb=None), dict(plan="fwd", ws=None), dict(d_amb=None), dict(d_amb=None, ws=None),
        dict(d_amb=None, n_reads=0), dict(plan="text", d_amb=None)])
    text_long = [dict(n=BIG), dict(n=BIG, plan="canon"), dict(n=BIG, ws=None)]
    t += _sync_and_async("mm_run_text_device_async", "mm_run_text_device", _text_ok, "canon", text_long + small + [
        dict(plan="text_sync", d_out_sk="d_sk"), dict(d_out_sk="d_sk"), dict(d_text=None), dict(text_bytes=39), dict(n=0, d_text=None),
        dict(plan="text_sync", d_out_sk="d_sk", n=BIG)])
    t += _sync_and_async("mm_run_text_batch_device_async", "mm_run_text_batch_device", _text_batch_ok, "canon", small + [
        dict(n_chars=BIG), dict(n_chars=BIG, ws=None), dict(n_records=1 << 31), dict(plan="text_sync", d_out_sk="d_sk"),
        dict(d_out_offsets=None), dict(d_out_offsets=None, ws=None), dict(d_starts=None), dict(text_bytes=39),
        dict(text_bytes=39, d_out_offsets=None), dict(d_text=None), dict(n_records=0), dict(d_out_sk="d_sk")])
    # ---- host entry points
    t += _variants("mm_run_host", _host_ok, "text", long_ + [
        dict(capacity=1), dict(out_pos=None, capacity=0), dict(plan="sync", out_sk="h_sk"), dict(plan="sync", out_sk="h_sk", n_bases=BIG),
        dict(out_sk="h_sk"), dict(packed=None), dict(packed=None, n_bases=0), dict(plan="fwd"), dict(count=None)])
    t += _variants("mm_run_host_ascii", _ascii_ok, "text", long_ + [
        dict(capacity=1), dict(out_pos=None, capacity=0), dict(plan="sync", out_sk="h_sk"), dict(plan="sync", out_sk="h_sk", n_bases=BIG),
        dict(plan="sync", out_sk="h_sk", ascii=None), dict(out_sk="h_sk"), dict(ascii=None), dict(ascii=None, n_bases=0), dict(plan="fwd")])
    t += _variants("mm_run_skip_ambiguous_host", _skip_host_ok, "text", long_ + [
        dict(capacity=1), dict(out_pos=None, capacity=0), dict(plan="fwd"), dict(plan="fwd", n_bases=BIG), dict(plan="fwd", amb=None),
        dict(amb=None), dict(packed=None), dict(amb=None, n_bases=0), dict(plan="sync")])
    t += _variants("mm_run_skip_ambiguous_host_ascii", _skip_ascii_ok, "text", long_ + [
        dict(capacity=1), dict(out_pos=None, capacity=0), dict(plan="fwd"), dict(plan="fwd", n_bases=BIG), dict(plan="fwd", ascii=None),
        dict(ascii=None), dict(ascii=None, n_bases=0)])
    dec = dict(read_starts="h_starts_dec")
    t += _variants("mm_run_packed_reads_host", _packed_host_ok, "text", [
        dict(capacity=1), dict(out_pos=None, capacity=0), dec, dict(dec, out_offsets=None), dict(dec, plan="text"), dict(dec, ws=None),
        dict(dec, plan="sync", out_sk="h_sk"), dict(plan="sync", out_sk="h_sk"), dict(out_sk="h_sk"), dict(out_offsets=None),
        dict(read_starts=None), dict(packed=None), dict(packed=None, n_reads=0, read_starts=None), dict(read_starts="h_starts_big"),
        dict(plan="fwd"), dict(count=None)])
    t += _variants("mm_run_packed_reads_skip_ambiguous_host", _packed_skip_host_ok, "text", [
        dict(capacity=1), dict(out_pos=None, capacity=0), dec, dict(dec, out_offsets=None), dict(dec, plan="text"), dict(dec, ws=None),
        dict(dec, plan="fwd"), dict(dec, amb=None), dict(plan="fwd"), dict(plan="fwd", amb=None), dict(plan="fwd", ws=None),
        dict(amb=None), dict(amb=None, ws=None), dict(amb=None, out_offsets=None), dict(out_offsets=None), dict(read_starts=None),
        dict(packed=None), dict(packed=None, amb=None, n_reads=0, read_starts=None), dict(read_starts="h_starts_big"), dict(count=None)])
    t += _variants("mm_run_text_host", _text_host_ok, "canon", text_long + [
        dict(capacity=1), dict(out_pos=None, capacity=0), dict(plan="text_sync", out_sk="h_sk"), dict(out_sk="h_sk"), dict(text=None),
        dict(text=None, n=0), dict(text=None, plan="text_sync", out_sk="h_sk")])
    tdec = dict(starts="h_tstarts_dec")
    t += _variants("mm_run_text_batch_host", _text_batch_host_ok, "canon", [
        dict(capacity=1), dict(out_pos=None, capacity=0), tdec, dict(tdec, ws=None), dict(tdec, out_offsets=None), dict(tdec, plan="canon"),
        dict(tdec, text=None), dict(plan="text_sync", out_sk="h_sk"), dict(tdec, plan="text_sync", out_sk="h_sk"), dict(out_sk="h_sk"),
        dict(out_offsets=None), dict(starts=None), dict(text=None), dict(n_records=1 << 31), dict(n_records=0, starts=None, text=None),
        dict(starts="h_starts_big"), dict(starts="h_starts_big", ws=None)])
    # ---- the plan guard of the entry points that are otherwise untouched
    t += [("mm_run_batch_device", dict(plan=p, ws=w, n_seqs=0, d_packed=None, packed_bytes=None, base_offsets=None, n_bases=None,
                                       d_out_pos=None, d_out_sk=None, capacity=0, out_offsets=o))
          for p, w, o in (("text", None, None), ("text", "ws", "h_offs"), (None, None, None), ("canon", None, "h_offs"), ("canon", "ws", None),
                          ("canon", "ws", "h_offs"))]
    for p in ("text", "canon", None):
        t.append(("mm_run_sharded_host", dict(plan=p, group=None, packed="h_seq", base_offset=0, n_bases=64, out_pos="h_out", out_sk=None,
                                              capacity=256, count="h_count")))
        t.append(("mm_run_sharded_device", dict(plan=p, group=None, base_offset=0, n_bases=64, want_superkmers=0, counts=None, total=None)))
        t.append(("mm_run_batch_sharded_device", dict(plan=p, group=None, base_offsets=None, n_bases=None, want_superkmers=0,
                                                      out_counts=None, total=None)))
        t.append(("mm_run_batch_sharded_host", dict(plan=p, group=None, n_seqs=0, packed=None, base_offsets=None, n_bases=None,
                                                    out_pos=None, out_sk=None, capacity=0, out_offsets="h_offs")))
    # ---- values
    for words, too_long in ((1, 33), (2, 65)):
        name = "mm_values_u%d" % (64 * words)
        for fn, ok, pk, ps, vs in ((name + "_device_async", _values_dev_ok, "d_packed", "d_pos", "d_values"),
                                   (name + "_host", _values_host_ok, "packed", "pos", "values")):
            ok = dict(ok, len=5 if words == 1 else 33)
            for o in ({}, dict(ws=None), dict(len=0), dict(len=too_long), dict(len=too_long - 1), dict(len=33), dict(len=0, ws=None),
                      dict(len=too_long, ws=None), dict(len=too_long, n_pos=0), dict(n_pos=0), {"n_pos": 0, pk: None}, {pk: None}, {ps: None},
                      {vs: None}, {"len": 0, pk: None}, dict(canonical=0)):
                if o.get("len", 0) in (32, 64):  # a value of the largest length: only position 0 of the 64 bases has room for it
                    o = dict(o, n_pos=1)
                t.append((fn, dict(ok, **o)))
        t.append((name + "_device_async", dict(_values_dev_ok, n_bases=BIG)))  # (more bases than the buffer holds)
    # ---- packers
    def pack_cases(fn, ok, sync):
        rows = [{}, dict(ws=None), dict(d_counts=None), dict(d_rec_base=None), dict(n_bytes=BIG), dict(n_bytes=BIG, ws=None),
                dict(d_packed="d_packed+1"), dict(d_packed="d_packed+1", n_bytes=BIG), dict(d_packed="d_packed+1", ws=None), dict(n_bytes=0),
                dict(n_bytes=0, d_text=None), dict(d_text=None), dict(d_packed=None),
                dict(n_bytes=0, d_counts=None)]
        if "d_amb" in ok:
            rows += [dict(d_amb=None), dict(d_amb="d_ambout+1"), dict(amb_capacity_bytes=0), dict(amb_capacity_bytes=6),
                     dict(d_amb=None, ws=None), dict(amb_capacity_bytes=0, ws=None), dict(d_amb="d_ambout+1", amb_capacity_bytes=0),
                     dict(amb_capacity_bytes=6, n_bytes=BIG), dict(d_amb=None, d_counts=None), dict(n_bytes=0, amb_capacity_bytes=4)]
        if sync:
            rows += [_fastq, dict(out_counts=None), dict(out_counts=None, ws=None), dict(out_counts=None, n_bytes=BIG), dict(packed_capacity_bytes=4),
                     dict(max_records=1), dict(_fastq, packed_capacity_bytes=4), dict(_fastq, max_records=1)]
            if "d_amb" in ok:
                rows += [dict(amb_capacity_bytes=4), dict(_fastq, amb_capacity_bytes=4), dict(out_counts=None, d_amb=None)]
        return [(fn, dict(ok, **o)) for o in rows]
    t += pack_cases("mm_fasta_pack_device_async", _pack_ok, False)
    t += pack_cases("mm_fastq_pack_device_async", dict(_pack_ok, **_fastq), False)
    t += pack_cases("mm_fasta_pack_n_device_async", _pack_n_ok, False)
    t += pack_cases("mm_fastq_pack_n_device_async", dict(_pack_n_ok, **_fastq), False)
    t += pack_cases("mm_fasta_pack_device", dict(_pack_ok, out_counts="h_counts"), True)
    t += pack_cases("mm_fasta_pack_n_device", dict(_pack_n_ok, out_counts="h_counts"), True)
    # ---- the families added after the first recording (appended: the rows above keep their places in the fixture)
    def counts_cases(fn, ok, wrong_plan, overrides):
        return (_variants(fn, dict(ok, out="h_counts"), wrong_plan, overrides) +
                _variants(fn + "_async", dict(ok, d_count="d_count"), wrong_plan, overrides))
    bounds = [dict(max_bases=BIG), dict(max_bases=BIG, plan=None), dict(max_bases=BIG, plan="text"), dict(max_records=1 << 31),
              dict(max_records=1 << 31, d_counts=None), dict(max_bases=BIG, ws=None)]
    pc_more = bounds + small + [dict(d_counts=None), dict(d_counts=None, ws=None), dict(d_read_starts=None), dict(d_out_offsets=None),
                                dict(plan="text", d_out_offsets=None), dict(d_packed=None), dict(packed_bytes=8),
                                dict(packed_bytes=8, ws=None), dict(packed_bytes=8, d_counts=None)]
    t += counts_cases("mm_run_packed_reads_counts_device", _pcounts_ok, "text", pc_more + [
        dict(plan="sync", d_out_sk="d_sk"), dict(plan="sync", d_out_sk="d_sk", d_counts=None), dict(plan="sync", d_out_sk="d_sk", max_bases=BIG),
        dict(d_out_sk="d_sk"), dict(plan="fwd"), dict(plan="sync")])
    t += counts_cases("mm_run_packed_reads_skip_ambiguous_counts_device", _pcounts_skip_ok, "text", pc_more + [
        dict(plan="fwd"), dict(plan="fwd", d_amb=None), dict(plan="fwd", max_bases=BIG), dict(plan="fwd", ws=None), dict(d_amb=None),
        dict(d_amb=None, ws=None), dict(packed_bytes=8, d_amb=None), dict(amb_bytes=4), dict(amb_bytes=4, ws=None),
        dict(plan="text", d_amb=None)])
    t += counts_cases("mm_run_text_batch_counts_device", _tcounts_ok, "canon", small + [
        dict(max_chars=BIG), dict(max_chars=BIG, plan=None), dict(max_chars=BIG, ws=None), dict(max_records=1 << 31), dict(max_chars=41),
        dict(max_chars=41, d_counts=None), dict(max_chars=41, ws=None), dict(plan="text_sync", d_out_sk="d_sk"),
        dict(plan="text_sync", d_out_sk="d_sk", d_counts=None), dict(d_out_sk="d_sk"), dict(d_counts=None), dict(d_counts=None, ws=None),
        dict(d_out_offsets=None), dict(plan="canon", d_out_offsets=None), dict(d_starts=None), dict(d_text=None), dict(max_chars=0)])
    for words in (1, 2):
        name = "mm_values_u%d" % (64 * words)
        dna_long, byte_long = 32 * words + 1, 8 * words + 1
        common = [{}, dict(ws=None), dict(len=0), dict(len=0, ws=None), dict(canonical=0)]
        for fn, ok, pk, ps, os_, vs, st in (
                (name + "_reads_device_async", _vreads_dev_ok, "d_packed", "d_pos", "d_out_offsets", "d_values", "d_read_starts"),
                (name + "_reads_host", _vreads_host_ok, "packed", "pos", "offsets", "values", "read_starts")):
            rows = common + [dict(len=dna_long), dict(len=dna_long, ws=None), {"len": dna_long, pk: None}, dict(n_reads=0),
                             {"n_reads": 0, pk: None}, {pk: None}, {ps: None}, {os_: None}, {vs: None}, {"len": 0, pk: None},
                             {st: None, "read_stride": 20}, {st: None, "read_stride": 20, "packed_bytes": 8}, dict(base_offset=BIG),
                             dict(base_offset=BIG, ws=None)]
            rows += ([dict(n_pos_max=0), {"n_pos_max": 0, pk: None}] if fn.endswith("_async") else
                     [{st: "h_starts_dec"}, {st: "h_starts_dec", "ws": None}, {st: "h_starts_dec", "len": 0}, dict(offsets="h_voffs_dec"),
                      {st: "h_starts_big"}])
            t += [(fn, dict(ok, **o)) for o in rows]
        t += [(name + "_batch_device_async", dict(_vbatch_ok, **o)) for o in common + [
            dict(len=dna_long), dict(len=dna_long, ws=None), dict(len=dna_long, offsets="h_voffs_dec"), dict(n_seqs=0),
            dict(n_seqs=0, d_packed=None), dict(d_packed=None), dict(packed_bytes=None), dict(n_bases=None), dict(d_pos=None),
            dict(offsets=None), dict(d_values=None), dict(offsets="h_voffs_dec"), dict(offsets="h_voffs_dec", ws=None),
            dict(packed_bytes="h_bbytes_small"), dict(packed_bytes="h_bbytes_small", offsets="h_voffs_dec"), dict(d_packed="h_bptrs_null"),
            dict(n_seqs=BIG), dict(n_seqs=BIG, ws=None), dict(base_offsets="h_bbases")]]
        text_rows = common + [dict(len=byte_long), dict(len=byte_long, ws=None), dict(canonical=1), dict(canonical=1, len=byte_long),
                              dict(encoding=1), dict(encoding=1, canonical=1), dict(encoding=1, len=dna_long), dict(encoding=2),
                              dict(encoding=2, len=0), dict(encoding=2, ws=None)]
        t += [(name + "_text_device_async", dict(_vtext_dev_ok, **o)) for o in text_rows + [
            dict(n=BIG), dict(n=BIG, ws=None), dict(n=BIG, encoding=2), dict(n=41), dict(n=41, d_text=None), dict(text_bytes=39),
            dict(n_pos=0), dict(n_pos=0, d_text=None), dict(d_text=None), dict(d_pos=None), dict(d_values=None)]]
        t += [(name + "_text_host", dict(_vtext_host_ok, **o)) for o in text_rows + [
            dict(n=BIG, text=None), dict(n_pos=0), dict(n_pos=0, text=None), dict(text=None), dict(pos=None), dict(values=None)]]
        t += [(name + "_text_batch_device_async", dict(_vtbatch_dev_ok, **o)) for o in text_rows + [
            dict(n_chars=BIG), dict(n_chars=BIG, ws=None), dict(n_records=1 << 31), dict(n_chars=41), dict(text_bytes=39),
            dict(text_bytes=39, d_starts=None), dict(n_records=0), dict(n_pos_max=0), dict(n_pos_max=0, d_text=None), dict(d_text=None),
            dict(d_starts=None), dict(d_pos=None), dict(d_out_offsets=None), dict(d_values=None)]]
        t += [(name + "_text_batch_counts_device_async", dict(_vtcounts_ok, **o)) for o in text_rows + [
            dict(max_chars=BIG), dict(max_chars=BIG, ws=None), dict(max_records=1 << 31), dict(max_chars=41), dict(max_chars=41, d_counts=None),
            dict(max_records=0), dict(max_records=0, d_counts=None), dict(n_pos_max=0), dict(d_text=None), dict(d_starts=None),
            dict(d_counts=None), dict(d_counts=None, ws=None), dict(d_pos=None), dict(d_out_offsets=None), dict(d_values=None)]]
        t += [(name + "_text_batch_host", dict(_vtbatch_host_ok, **o)) for o in text_rows + [
            dict(starts="h_tstarts_dec"), dict(starts="h_tstarts_dec", ws=None), dict(starts="h_tstarts_dec", len=0),
            dict(offsets="h_voffs_dec"), dict(starts="h_starts_big"), dict(n_records=1 << 31), dict(n_records=0),
            dict(n_records=0, text=None, starts=None), dict(text=None), dict(starts=None), dict(pos=None), dict(offsets=None),
            dict(values=None)]]
    ftext_rows = [{}, dict(ws=None), dict(d_counts=None), dict(d_rec_start=None), dict(d_rec_text_pos=None), dict(n_bytes=BIG),
                  dict(n_bytes=BIG, ws=None), dict(d_seq="d_packed+1"), dict(d_seq="d_packed+1", n_bytes=BIG), dict(d_seq="d_packed+1", ws=None),
                  dict(n_bytes=0), dict(n_bytes=0, d_text=None), dict(d_text=None), dict(d_seq=None), dict(n_bytes=0, d_counts=None)]
    t += [("mm_fasta_text_device_async", dict(_ftext_ok, **o)) for o in ftext_rows]
    ftext_sync_ok = dict(_ftext_ok, out_counts="h_counts")
    t += [("mm_fasta_text_device", dict(ftext_sync_ok, **o)) for o in ftext_rows]
    t += [("mm_fasta_text_device", dict(ftext_sync_ok, **o)) for o in (
        _fastq, dict(_fastq, ws=None), dict(out_counts=None), dict(out_counts=None, ws=None), dict(out_counts=None, n_bytes=BIG),
        dict(seq_capacity_bytes=4), dict(max_records=1), dict(_fastq, seq_capacity_bytes=4))]
    ascii_rows = [{}, dict(ws=None), dict(n_bases=0), dict(n_bases=0, d_ascii=None), dict(n_bases=0, ws=None), dict(d_ascii=None),
                  dict(d_packed=None), dict(d_ascii=None, ws=None), dict(n_bases=63)]
    t += [("mm_pack_ascii_device_async", dict(_ascii_pack_ok, **o)) for o in ascii_rows]
    t += [("mm_pack_ascii_n_device_async", dict(dict(_ascii_pack_ok, d_amb="d_ambout"), **o)) for o in ascii_rows + [
        dict(d_amb=None), dict(d_amb=None, ws=None), dict(d_amb=None, n_bases=0), dict(d_amb=None, d_packed=None)]]
    names = {fn: [a.split(":")[0] for a in sig.split()] for fn, sig in SIG.items()}
    for fn, args in t:
        assert sorted(names[fn]) == sorted(args), (fn, sorted(args))
    return [(fn, {name: args[name] for name in names[fn]}) for fn, args in t]  # (arguments in the order of the signature)


# ---------------------------------------------------------------------------------------------- the environment
class Env:
    """The library (a handle of its own: no argtypes), one workspace, the plans and every buffer a case may name."""

    def __init__(self, sm):
        import torch
        self.sm, self.torch = sm, torch
        self.L = C.CDLL(sm.LIB_PATH)
        self.ws = sm.Workspace(0)
        self.plans = {}
        for name, (canonical, mode, text) in dict(canon=(1, 0, 0), fwd=(0, 0, 0), sync=(1, 1, 0), text=(0, 0, 1), text_sync=(0, 1, 1)).items():
            h = C.c_void_p()
            f = self.L.mm_plan_create_text if text else self.L.mm_plan_create
            assert f(C.byref(h), C.c_uint32(K), C.c_uint32(W), C.c_int(canonical), C.c_int(mode), None) == 0
            self.plans[name] = h
        rng = np.random.default_rng(11)
        codes = rng.integers(0, 4, size=64, dtype=np.uint8)
        self.codes = codes
        host = {
            "h_seq": sm.PackedSeqVec.from_codes(codes).data,
            "h_ascii": np.frombuffer(b"ACTG", dtype=np.uint8)[codes],
            "h_amb": np.array([0, 0x10, 0, 0, 0, 0x01, 0, 0], dtype=np.uint8),  # bases 12 and 40 are N
            "h_text": np.frombuffer(b"the quick brown fox jumps over the lazy!", dtype=np.uint8),
            "h_starts": np.array([0, 20, 40, 60], dtype=np.uint64), "h_starts_dec": np.array([0, 40, 20, 60], dtype=np.uint64),
            "h_starts_big": np.array([0, 20, 40, BIG], dtype=np.uint64),
            "h_tstarts": np.array([0, 10, 25, 40], dtype=np.uint64), "h_tstarts_dec": np.array([0, 25, 10, 40], dtype=np.uint64),
            "h_lens": np.array([20, 20, 20], dtype=np.uint32), "h_vpos": np.array([0, 3, 10, 27], dtype=np.uint32),
            "h_fasta": np.frombuffer(FASTA, dtype=np.uint8), "h_fastq": np.frombuffer(FASTQ, dtype=np.uint8),
            "h_rcounts": np.array([60, 3], dtype=np.uint64), "h_tcounts": np.array([40, 3], dtype=np.uint64),
            "h_rpos": np.array([0, 3, 10, 2], dtype=np.uint32), "h_voffs": np.array([0, 2, 3, 4], dtype=np.uint64),
            "h_voffs_dec": np.array([0, 3, 2, 4], dtype=np.uint64),
            "h_bbytes": np.array([10, 10, 10], dtype=np.uint64), "h_bbytes_small": np.array([10, 9, 10], dtype=np.uint64),
            "h_bbases": np.array([40, 40, 40], dtype=np.uint64),
        }
        size = 1 << 16  # (every buffer is far larger than any size a case states)
        self.buf = {}
        for name, a in host.items():
            b = np.zeros(size, dtype=np.uint8)
            b[:a.nbytes] = a.view(np.uint8)
            self.buf[name] = b
            self.buf["d" + name[1:]] = torch.from_numpy(b).cuda()
        for name in ("out", "sk", "offs", "count", "counts", "vals"):
            self.buf["h_" + name] = np.zeros(size, dtype=np.uint8)
        for name in ("out", "sk", "offs", "count", "counts", "vals", "packed", "rec_base", "rec_pos", "ambout"):
            self.buf["d_" + name] = torch.zeros(size, dtype=torch.uint8, device="cuda")
        # the batch values' table of device pointers: three 40-base sequences inside d_seq (and one with a NULL entry)
        for name, ptrs in (("h_bptrs", [0, 10, 20]), ("h_bptrs_null", [0, None, 20])):
            b = np.zeros(size, dtype=np.uint8)
            b[:24] = np.array([0 if p is None else self.buf["d_seq"].data_ptr() + p for p in ptrs], dtype=np.uint64).view(np.uint8)
            self.buf[name] = b
        torch.cuda.synchronize()

    def address(self, name):
        base, _, plus = name.partition("+")
        b = self.buf[base]
        return (b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()) + int(plus or 0)

    def call(self, fn, args):
        argv = []
        for spec in SIG[fn].split():
            name, kind = spec.split(":")
            v = args[name]
            if kind != "p":
                argv.append(_KIND[kind](v))
            elif v is None:
                argv.append(C.c_void_p(None))
            elif name == "plan":
                argv.append(self.plans[v])
            elif v == "ws":
                argv.append(self.ws.h)
            else:
                argv.append(C.c_void_p(self.address(v)))
        rc = getattr(self.L, fn)(*argv)
        # the next case starts from a quiet stream and a checked workspace, whatever this one queued or raised
        self.L.mm_workspace_sync(self.ws.h)
        self.L.mm_workspace_check(self.ws.h)
        return rc

    def close(self):
        for h in self.plans.values():
            self.L.mm_plan_destroy(h)
        self.ws.close()


@pytest.fixture(scope="module")
def env(sm, gpu):
    e = Env(sm)
    yield e
    e.close()


def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _case_id(row):
    return row["fn"]


@pytest.mark.gpu
def test_fixture_is_the_case_table():
    """One recorded row per case of the table, in its order: a case added, dropped or changed needs a new recording."""
    assert [(r["fn"], r["args"]) for r in _recorded()] == [(fn, args) for fn, args in cases()]


@pytest.mark.gpu
@pytest.mark.parametrize("row", _recorded() if os.path.exists(FIXTURE) else [], ids=_case_id)
def test_return_code(env, row):
    assert row["rc"] != MM_ERR_HIP
    got = env.call(row["fn"], row["args"])
    assert got == row["rc"], (row["fn"], row["args"], env.sm.lib().mm_last_error())


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.gpu
def test_values_u128_device_against_the_oracle(env, oracle):
    """mm_values_u128_device_async == the oracle's Output::values_u128 on the 64 bases: lengths either side of one word, both
    strands' choice.  (Its twin mm_values_u64_device_async: test_gpu_round4::test_values_u64_four_per_thread.  Values have
    no capacity to exceed: the case beyond the limit is len = 65, pinned above.)"""
    torch = env.torch
    packed = env.buf["h_seq"]
    for ln in (1, 5, 32, 33, 63, 64):
        for canonical in (1, 0):
            pos = np.unique(np.array([0, 3, 10, 27, 64 - ln], dtype=np.uint32).clip(0, 64 - ln))
            d_pos = torch.from_numpy(pos.view(np.int32)).cuda()
            d_vals = torch.full((2 * len(pos),), -1, dtype=torch.int64, device="cuda")
            rc = env.L.mm_values_u128_device_async(env.ws.h, C.c_void_p(env.address("d_seq")), C.c_uint64(4096), C.c_uint64(0),
                                                   C.c_uint64(64), C.c_uint32(ln), C.c_int(canonical), C.c_void_p(d_pos.data_ptr()),
                                                   C.c_uint64(len(pos)), C.c_void_p(d_vals.data_ptr()))
            assert rc == 0, (ln, canonical)
            env.ws.sync()
            want = oracle.values_u128(packed, ln, pos, bool(canonical))
            assert np.array_equal(d_vals.cpu().numpy().view(np.uint64).reshape(-1, 2), want), (ln, canonical)


@pytest.mark.gpu
def test_host_ascii_against_the_oracle(env, oracle):
    """mm_run_host_ascii == the oracle on the packed form of the same 64 bases - forward and canonical minimizers, with
    super-k-mer indices, closed syncmers - and a capacity below the count: MM_ERR_CAPACITY, the true count, nothing
    written past the capacity."""
    packed, asc = env.buf["h_seq"], env.buf["h_ascii"]
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for plan, canonical, mode in (("fwd", False, oracle.MINIMIZERS), ("canon", True, oracle.MINIMIZERS), ("sync", True, oracle.CLOSED_SYNCMERS)):
        want = oracle.run(packed, 64, K, W, canonical=canonical, mode=mode, super_kmers=mode == oracle.MINIMIZERS)
        want_pos, want_sk = want if mode == oracle.MINIMIZERS else (want, None)
        pos, sk, cnt = np.full(64, 0xFFFFFFFF, dtype=np.uint32), np.full(64, 0xFFFFFFFF, dtype=np.uint32), C.c_uint64()
        rc = env.L.mm_run_host_ascii(env.plans[plan], env.ws.h, asc.ctypes.data_as(u8), C.c_uint64(64), pos.ctypes.data_as(u32),
                                     sk.ctypes.data_as(u32) if want_sk is not None else None, C.c_uint64(64), C.byref(cnt))
        assert rc == 0 and cnt.value == len(want_pos), plan
        assert np.array_equal(pos[:cnt.value], want_pos), plan
        if want_sk is not None:
            assert np.array_equal(sk[:cnt.value], want_sk), plan
        assert len(want_pos) > 2
        pos[:] = 0xFFFFFFFF
        rc = env.L.mm_run_host_ascii(env.plans[plan], env.ws.h, asc.ctypes.data_as(u8), C.c_uint64(64), pos.ctypes.data_as(u32), None,
                                     C.c_uint64(2), C.byref(cnt))
        assert rc == env.sm.ERR["CAPACITY"] and cnt.value == len(want_pos), plan
        assert (pos[2:] == 0xFFFFFFFF).all(), plan


# ---------------------------------------------------------------------------------------------- the recorder
def _record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import simd_minimizers_amd as sm
    env = Env(sm)
    rows, refused = [], []
    for fn, args in cases():
        rc = env.call(fn, args)
        rows.append({"fn": fn, "args": args, "rc": rc})
        if rc == MM_ERR_HIP:
            refused.append((fn, args, sm.lib().mm_last_error()))
    env.close()
    for r in refused:
        print("HIP error - take this case out of the table:", r)
    if refused:
        return 1
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} cases recorded from {sm.LIB_PATH}")
    return 0


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_abi_codes.py --record   (MM_LIB_PATH selects the library to pin)")
    sys.exit(_record())
